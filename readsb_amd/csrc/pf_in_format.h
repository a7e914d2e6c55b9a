// pf_in_format.h — readPlanefinder's loop (net_io.c:4670-4735) and decodePfMessage (:3995-4101, with getNextPfUnstuffedByte,
// :3965-3970) as far as the record: ONE framer and parser, __host__ __device__, for the passes of kernels/pf_in.inc and for the host
// (pf_in_host.cpp: mgpu_pf_parse_host and the sequential walk; tests/host_stub/pf_in_format_check.cpp runs it under ASan and UBSan).
// Everything is integer work or single IEEE double operations (compile with -ffp-contract=off).
//
// The stream is d[0 .. n): a byte at an index >= n reads as 0 (the reference NUL-terminates its client buffer) and nothing at or
// beyond n is loaded.  A stretch of it, d[0 .. nf) with nf <= n, is FRAMED: only a DLE below nf is an event, but its lookahead byte
// and the handler's reads come from the whole stream (the host forms' passes frame nf bytes of nf + look staged ones; nf == n
// everywhere else).
//   The loop is a two-state automaton over two predicates with one byte of lookahead:
//     pf_in_is_start(p)  B: DLE at p, p + 1 < n, d[p + 1] neither DLE nor ETX
//     pf_in_is_end(p)    E: DLE at p, p + 1 < n, d[p + 1] == ETX
//   Searching: B opens a frame, any other DLE moves som to p + 1.  In frame: E at q closes it, som = q + 2; B is ignored.  After any
//   event the state no longer depends on what came before, which is what the device's passes rest on.
//   pf_in_step is the loop's body for one som, the plain statement of it; pf_in_fields is the handler's reads (it never needs the
//   frame's end); pf_in_frame the record and its class through raw_in_decode_frame.
// The handler reaches at most kPfInReach = 53 bytes from the start DLE: the DLE, and 26 unstuffed bytes (id, padding, type, signal,
// eight of time, fourteen of message) of two bytes each at the most.
#pragma once
#include <cstdint>

#include "raw_in_format.h"

namespace mgpu {

constexpr uint32_t kPfDle = 0x10, kPfEtx = 0x03, kPfId = 0xc1;
constexpr uint32_t kPfInReach = 53;
static_assert(kPfInReach == 1 + 2 * (1 + 1 + 1 + 1 + 4 + 4 + 14), "the start DLE and 26 unstuffed bytes");
// a complete frame has 4 bytes (DLE, id, DLE, ETX); a stretch may close one whose ETX lies one byte behind it
constexpr uint64_t pf_in_max_frames(uint64_t nbytes) { return nbytes / 4 + 1; }

enum : uint32_t { PF_IN_END = 0, PF_IN_SKIP = 1, PF_IN_OTHER = 2, PF_IN_FRAME = 3, PF_IN_INCOMPLETE = 4 };   // MGPU_PF_STEP_*'s values

RAW_IN_HD bool pf_in_is_start(const uint8_t *d, uint64_t n, uint64_t p) { return d[p] == kPfDle && p + 1 < n && d[p + 1] != kPfDle && d[p + 1] != kPfEtx; }
RAW_IN_HD bool pf_in_is_end(const uint8_t *d, uint64_t n, uint64_t p) { return d[p] == kPfDle && p + 1 < n && d[p + 1] == kPfEtx; }

struct PfInStep {
    uint64_t next;            // the som the step leaves
    uint64_t frame;           // OTHER, FRAME, INCOMPLETE: the start DLE
    uint32_t kind;
};

// the loop's body with c->som == d + som: nf bytes framed of the stream's n
RAW_IN_HD uint32_t pf_in_step(const uint8_t *d, uint64_t nf, uint64_t n, uint64_t som, PfInStep &st) {
    st.next = som; st.frame = som;
    uint64_t p = som;
    while (p < nf && d[p] != kPfDle) ++p;                                 // memchr
    if (p >= nf) return st.kind = PF_IN_END;
    if (!pf_in_is_start(d, n, p)) { st.next = p + 1; return st.kind = PF_IN_SKIP; }
    st.frame = p;
    uint64_t q = p + 2;
    while (q < nf && !pf_in_is_end(d, n, q)) ++q;
    if (q >= nf) return st.kind = PF_IN_INCOMPLETE;
    st.next = q + 2;
    return st.kind = d[p + 1] == kPfId ? PF_IN_FRAME : PF_IN_OTHER;
}

// getNextPfUnstuffedByte over the stream: the reader's place, and whether it read an index > n
struct PfInReader {
    const uint8_t *d;
    uint64_t n, p;
    uint32_t past;
    RAW_IN_HD uint32_t at(uint64_t i) { if (i > n) past = 1; return i < n ? d[i] : 0u; }
    RAW_IN_HD uint32_t next() {
        if (at(p) == kPfDle) ++p;
        return at(p++);
    }
};

struct PfInFields {
    uint64_t ts;              // seconds * 1000000000 + nanoseconds
    uint32_t type, sig, nb;   // the type byte; the signal byte; the message's bytes: 2, 7, 14, or 0 for a type that returns
    uint32_t past;            // the reads went beyond index n
    uint8_t m[14];
};

// The handler's reads for the frame whose start DLE is d[start] (d[start + 1] == 0xc1, which is no DLE).  Returns the class the reads
// alone decide — MGPU_PF_IN_TYPE, MGPU_PF_IN_MODEAC_OFF — or 0: a candidate, which reaches the decode.
RAW_IN_HD uint32_t pf_in_fields(const uint8_t *d, uint64_t n, uint64_t start, int32_t mode_ac, PfInFields &f) {
    PfInReader r = {d, n, start + 1, 0};
    f.ts = 0; f.sig = 0; f.nb = 0; f.past = 0;
    for (int j = 0; j < 14; ++j) f.m[j] = 0;
    (void) r.next();                                                      // the id
    (void) r.next();                                                      // padding
    f.type = r.next();
    const uint32_t t = f.type & 0xFu;
    if (t > 2) { f.past = r.past; return MGPU_PF_IN_TYPE; }
    if (t == 0 && !mode_ac) { f.past = r.past; return MGPU_PF_IN_MODEAC_OFF; }
    f.nb = t == 0 ? 2u : t == 1 ? 7u : 14u;
    f.sig = r.next();
    uint64_t seconds = 0, nanos = 0;
    for (int j = 0; j < 4; ++j) seconds = seconds << 8 | r.next();
    for (int j = 0; j < 4; ++j) nanos = nanos << 8 | r.next();
    f.ts = seconds * 1000000000ull + nanos;
    for (uint32_t j = 0; j < f.nb; ++j) f.m[j] = (uint8_t) r.next();
    f.past = r.past;
    return 0;
}

// a candidate's record and class (MGPU_PF_IN_MODEAC, _BAD, _ACCEPT, _COND are MGPU_RAW_*'s values)
RAW_IN_HD uint32_t pf_in_frame(PfInFields &f, int64_t now_ms, const RawInConfig &cfg, const RawInTables &tb, RawInLine &out) {
    raw_in_zero(out);
    double signal = (double) f.sig / 255.0;
    signal = signal * signal;
    return raw_in_decode_frame(f.m, f.nb, f.ts, signal, f.sig, now_ms, cfg, tb, out);
}

}  // namespace mgpu
