// beast_in_format.h — one iteration of readBeast's loop (net_io.c:4737-5018) and decodeBinMessage (:3804-3961) as far as the record:
// ONE framer and parser, __host__ __device__, for the passes of kernels/beast_in.inc and for the host (beast_in_host.cpp:
// mgpu_beast_parse_host and the sequential resolver; tests/host_stub/beast_in_format_check.cpp runs it under ASan and UBSan).
// Everything is integer work or single IEEE double operations (compile with -ffp-contract=off).
//
// beast_in_step(data, nbytes, som, net_ingest, st) is the loop's body for c->som == data + som and c->eod == data + nbytes.  Where
// `som` goes next depends on som and the bytes alone, never on how the scan got there: that is what lets the device treat a tile as a
// function from entry offsets to an exit offset.  The byte at data[nbytes] counts as 0 (the reference NUL-terminates its client
// buffer, :5182); nothing at or beyond nbytes is read.
//   A byte that is no 0x1a is ONE step of its own (BEAST_IN_GARBAGE, one byte of garbage, next = som + 1): the reference's memchr
//   skips a run of them at once and counts the run only when it finds a 0x1a behind it, so the callers count a garbage byte only when a
//   0x1a step follows it on the chain, and leave `consumed` in front of a trailing run (the tail rule, :5010-5015, aside).
//   At a 0x1a, quirk for quirk:
//     0xe8 (:4773-4793): INCOMPLETE when its eight bytes are not all there, else the stop BEAST_IN_STOP_SYNTH.
//     0xe3 (:4819-4857): the escape loop with its eom bookkeeping — a 0x1a in the id followed by another byte that is not the
//       buffer's last abandons the frame with som on the byte BEHIND that 0x1a (p - 1 after two increments), not on it; `eom + 2 >
//       eod` is incomplete and leaves som and the id alone; the id is taken unless net_ingest; som moves to the byte behind the id,
//       and only if that is a 0x1a does the SAME iteration go on with the type byte behind it — where 0xe3 and 0xe8 are then plain
//       unknown types (two bytes of garbage), and 0xe4 still stops.
//     '1' '2' '3' '5' 'P': eom, the first `eom > eod`, the un-escaping (:4936-4971: `1a 1a` one byte and eom one further; `1a` and
//       another byte abandons the frame with som on that 0x1a), the second `eom > eod`; then the handler call (BEAST_IN_FRAME).
//     'W': som += 2, counted.  0xe4: the stop BEAST_IN_STOP_UUID.  Anything else: som += 2, two bytes of garbage.
//   Every `break` is BEAST_IN_INCOMPLETE with next = the som it leaves (the frame's 0x1a; behind a taken 0xe3 prefix the inner one, and
//   the id stays taken).
// A step reads at most kBeastInMaxFrame = 62 bytes from som: 1a e3, eight escaped id bytes, 1a 33 and 21 escaped bytes.
#pragma once
#include <cstdint>

#include "raw_in_format.h"

namespace mgpu {

constexpr uint32_t kBeastInMaxFrame = 62;
constexpr uint32_t kBeastInTail = 256;           // more unconsumed bytes than this at the end are all garbage, net_io.c:5010
// a handler call needs 5 bytes (1a 'P' and three more), a message 11 (1a '1', six, one, two)
constexpr uint64_t beast_in_max_frames(uint64_t nbytes) { return nbytes / 5 + 1; }
constexpr uint64_t beast_in_max_msgs(uint64_t nbytes) { return nbytes / 11 + 1; }

enum : uint32_t { BEAST_IN_GARBAGE = 0, BEAST_IN_SKIP = 1, BEAST_IN_FRAME = 2, BEAST_IN_INCOMPLETE = 3, BEAST_IN_STOP_SYNTH = 4, BEAST_IN_STOP_UUID = 5 };

struct BeastInStep {
    uint64_t next;            // GARBAGE, SKIP, FRAME: the next som.  INCOMPLETE and the stops: the som the loop is left with
    uint64_t frame;           // FRAME: the frame's 0x1a (som at the handler call)
    uint64_t id;              // id_set: the receiver id the step leaves in c->receiverId
    uint32_t kind, garbage;   // the bytes of remote_malformed_beast the step itself adds
    uint32_t id_set, wcmd;    // a 0xe3 prefix taken; a 'W' command
    uint32_t len;             // FRAME: bytes of payload[], the type byte first
    uint8_t payload[24];
};

RAW_IN_HD uint32_t beast_in_step(const uint8_t *d, uint64_t n, uint64_t som, uint32_t net_ingest, BeastInStep &st) {
    st.next = som; st.frame = som; st.id = 0; st.garbage = 0; st.id_set = 0; st.wcmd = 0; st.len = 0;
    if (som >= n) return st.kind = BEAST_IN_INCOMPLETE;
    if (d[som] != 0x1a) { st.next = som + 1; st.garbage = 1; return st.kind = BEAST_IN_GARBAGE; }
    uint64_t p = som + 1, eom;
    if (p >= n) return st.kind = BEAST_IN_INCOMPLETE;
    uint32_t ch = d[p];
    if (ch == 0xe8) {
        ++p;
        if (p + 8 > n) return st.kind = BEAST_IN_INCOMPLETE;
        return st.kind = BEAST_IN_STOP_SYNTH;
    } else if (ch == 0xe3) {
        ++p;
        uint64_t id = 0;
        eom = p + 8;
        for (int j = 0; j < 8 && p < n && p < eom; ++j) {
            ch = d[p++];
            if (ch == 0x1a) {
                ch = p < n ? d[p] : 0u;
                ++p;
                ++eom;
                if (p < n && ch != 0x1a) {
                    st.garbage = (uint32_t) (p - 1 - som);
                    st.next = p - 1;
                    return st.kind = BEAST_IN_SKIP;
                }
            }
            id = id << 8 | (ch & 255u);
        }
        if (eom + 2 > n) return st.kind = BEAST_IN_INCOMPLETE;
        if (!net_ingest) { st.id_set = 1; st.id = id; }
        som = p;
        st.next = som; st.frame = som;
        if (d[p] != 0x1a) return st.kind = BEAST_IN_SKIP;                 // (p <= eom < n)
        ++p;
        if (p >= n) return st.kind = BEAST_IN_INCOMPLETE;
    }
    ch = d[p];
    if (ch == '2') eom = p + 1 + 6 + 1 + 7;
    else if (ch == '3') eom = p + 1 + 6 + 1 + 14;
    else if (ch == '1') eom = p + 1 + 6 + 1 + 2;
    else if (ch == '5') eom = p + 14 + 8;
    else if (ch == 0xe4) return st.kind = BEAST_IN_STOP_UUID;
    else if (ch == 'P') eom = p + 4;
    else if (ch == 'W') { st.wcmd = 1; st.next = som + 2; return st.kind = BEAST_IN_SKIP; }
    else { st.garbage = 2; st.next = som + 2; return st.kind = BEAST_IN_SKIP; }
    if (eom > n) return st.kind = BEAST_IN_INCOMPLETE;
    uint32_t t = 0;
    while (p < eom) {
        if (d[p] == 0x1a) {
            ++p;
            ++eom;
            if (eom > n) return st.kind = BEAST_IN_INCOMPLETE;
            if (d[p] != 0x1a) {
                st.garbage = (uint32_t) (p - 1 - som);
                st.next = p - 1;
                return st.kind = BEAST_IN_SKIP;
            }
        }
        st.payload[t++] = d[p++];
    }
    st.len = t;
    st.next = eom;
    return st.kind = BEAST_IN_FRAME;
}

// What the read handler makes of a frame (decodeBinMessage): the class of the handler call, and for '1' '2' '3' the record as
// raw_in_decode_frame leaves it.  MGPU_BEAST_IN_MODEAC, _BAD, _ACCEPT, _COND and _UNKNOWN are MGPU_RAW_*'s values.
RAW_IN_HD uint32_t beast_in_frame(const BeastInStep &st, int64_t now_ms, const RawInConfig &cfg, const RawInTables &tb, RawInLine &out) {
    raw_in_zero(out);
    const uint32_t type = st.payload[0];
    if (type == '5') return out.cls = MGPU_BEAST_IN_POSITION;
    if (type == 'P') return out.cls = MGPU_BEAST_IN_PONG;
    if (type == '1' && !cfg.mode_ac) return out.cls = MGPU_BEAST_IN_MODEAC_OFF;
    uint64_t ts = 0;
    for (int j = 0; j < 6; ++j) ts = ts << 8 | st.payload[1 + j];
    const uint32_t b = st.payload[7];
    double signal = (double) b / 255.0;
    signal = signal * signal;
    const uint32_t nb = type == '1' ? 2u : type == '2' ? 7u : 14u;
    uint8_t m[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t j = 0; j < nb; ++j) m[j] = st.payload[8 + j];
    return raw_in_decode_frame(m, nb, ts, signal, b, now_ms, cfg, tb, out);
}

// a handler call that reaches the decode (or decodeModeAMessage): a candidate of the filter passes
RAW_IN_HD bool beast_in_is_cand(const BeastInStep &st, const RawInConfig &cfg) {
    const uint32_t type = st.payload[0];
    return type == '2' || type == '3' || (type == '1' && cfg.mode_ac);
}

}  // namespace mgpu
