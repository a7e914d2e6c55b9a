// raw_in_format.h — one AVR raw line to the message readsb's raw input leaves (decodeHexMessage, net_io.c:4104-4287, behind
// readAscii, :4599-4641, as far as its call of decodeModesMessage) and the front of decodeModesMessage (mode_s.c:443-606, 766-779) up
// to the one question it cannot answer alone: "is this address in the ICAO filter right now?".  ONE parser, __host__ __device__, for
// the size pass and the classify pass of kernels/raw_in.inc and for the host (raw_in_host.cpp: mgpu_raw_parse_line_host and the
// sequential resolver; tests/host_stub/raw_in_format_check.cpp runs it against the reference's records under ASan and UBSan).
//
// raw_in_line(p, n, now_ms, cfg, tables, out) sees the n bytes of a line without its terminator ('\n' or NUL), a trailing '\r' still
// on it.  Everything here is integer work or single IEEE double operations (compile with -ffp-contract=off): nothing is deferred.
//   The result is a class (MGPU_RAW_*), the address the filter is asked about, the adder flag (a clean DF17, or a clean DF11 with
//   IID 0: the only frames that add to the filter, mode_s.c:766-779 — a frame fixDF17msgtype repaired has correctedbits 1 and never
//   adds), the 64-byte struct mgpu_msg a successful decode leaves, and mm->signalLevel as a double.
//   strtol (the Aerobits suffix, :4144, :4154) is restated in integers with its full semantics: leading isspace, a sign, "0x" in base
//   16, digits up to the first other byte, LONG_MAX / LONG_MIN on overflow.  strtok_r on "," skips empty fields.
//   A non-hex digit of the 12-digit timestamp contributes hexDigitVal's -1 (all ones, in two's-complement 64-bit arithmetic, which is
//   what the compiled reference does); the timestamp is shifted onto what the Aerobits suffix left.
// Not modelled: what follows the record in decodeModesMessage for remote messages (the MLAT / SBS / garbage source overrides,
//   mode_s.c:781-799: they follow from timestamp and addr, which the record keeps); netUseMessage and beyond.
// Departures: an EMPTY line (the reference reads hex[l - 1] with l == 0, the byte in front of the line) is "not a frame" here; and a
//   line longer than kRawInMaxLine bytes is "not a frame" whatever it holds (the reference has no limit but its client buffer; the
//   longest line its own writers produce is 45 bytes, the tile's halo holds kRawInMaxLine).
#pragma once
#include <cstdint>

#include "../../include/modes_gpu.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RAW_IN_HD __host__ __device__ inline
#else
#define RAW_IN_HD inline
#endif

namespace mgpu {

constexpr uint32_t kRawInMaxLine = 256;          // a longer line is not a frame (= kUatHalo: what a tile sees of its last line)
constexpr uint32_t kRawInMinLine = 5;            // l <= 2 * MODEAC_MSG_BYTES is too short, net_io.c:4177
// a line that gives anything has kRawInMinLine bytes and a terminator
constexpr uint64_t raw_in_max_cands(uint64_t nbytes) { return nbytes / (kRawInMinLine + 1) + 1; }

// the tables of a configuration: the CRC's byte table (crc.c:42-57) and the packed syndrome tables modesChecksumInit(nfix_crc) builds
// (tables.h: syndrome << 16 | bit0 << 8 | bit1, 0xff = none, sorted by syndrome)
struct RawInTables {
    const uint32_t *crc_byte;
    const uint64_t *tab_long, *tab_short;
    uint32_t n_long, n_short;
};
struct RawInConfig {
    int32_t nfix_crc, fixDF, mode_ac;
};
struct RawInLine {
    mgpu_msg msg;
    double signal;
    uint32_t cls, addr, adder;
};

RAW_IN_HD bool raw_in_isspace(uint32_t c) { return c == ' ' || (c - 9u) <= 4u; }      // isspace in the C locale: ' ', \t \n \v \f \r
RAW_IN_HD int raw_in_hexval(uint32_t c) {                                              // hexDigitVal, net_io.c:1815-1820
    if (c - '0' <= 9u) return (int) (c - '0');
    if (c - 'A' <= 5u) return (int) (c - 'A' + 10);
    if (c - 'a' <= 5u) return (int) (c - 'a' + 10);
    return -1;
}

// strtol(t, NULL, base) over t[0..n) (the token ends there as strtok_r's NUL would end it), base 10 or 16
RAW_IN_HD long long raw_in_strtol(const uint8_t *t, uint32_t n, uint32_t base) {
    uint32_t i = 0;
    while (i < n && raw_in_isspace(t[i])) ++i;
    bool neg = false;
    if (i < n && (t[i] == '+' || t[i] == '-')) { neg = t[i] == '-'; ++i; }
    if (base == 16 && i + 1 < n && t[i] == '0' && (t[i + 1] == 'x' || t[i + 1] == 'X')) {
        // "0x" is a prefix only in front of a hex digit; otherwise the number is the "0" and the result 0 either way
        if (i + 2 < n && raw_in_hexval(t[i + 2]) >= 0) i += 2;
    }
    const unsigned long long limit = neg ? 0x8000000000000000ull : 0x7fffffffffffffffull;
    unsigned long long v = 0;
    bool over = false;
    for (; i < n; ++i) {
        const int d = raw_in_hexval(t[i]);
        if (d < 0 || (uint32_t) d >= base) break;
        if (over) continue;
        if (v > (limit - (unsigned) d) / base) { over = true; continue; }
        v = v * base + (unsigned) d;
    }
    if (over) v = limit;
    return neg ? (long long) (0ull - v) : (long long) v;
}

// modesChecksum (crc.c:67-82) over the first `bits` of m
RAW_IN_HD uint32_t raw_in_crc(const uint8_t *m, uint32_t bits, const uint32_t *crc_byte) {
    const uint32_t nb = bits / 8;
    uint32_t rem = 0;
    for (uint32_t i = 0; i < nb - 3; ++i) rem = ((rem << 8) ^ crc_byte[m[i] ^ ((rem >> 16) & 0xffu)]) & 0xffffffu;
    return rem ^ ((uint32_t) m[nb - 3] << 16) ^ ((uint32_t) m[nb - 2] << 8) ^ m[nb - 1];
}

// modesChecksumDiagnose (crc.c:383-406) for a nonzero syndrome: the number of bits (1, 2) or -1
RAW_IN_HD int raw_in_diagnose(const uint64_t *tab, uint32_t n, uint32_t synd, uint32_t &b0, uint32_t &b1) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint32_t) (tab[mid] >> 16) < synd) lo = mid + 1; else hi = mid;
    }
    if (lo >= n) return -1;
    const uint64_t e = tab[lo];
    if ((uint32_t) (e >> 16) != synd) return -1;
    b0 = (uint32_t) (e >> 8) & 0xffu;
    b1 = (uint32_t) e & 0xffu;
    return b1 == 0xffu ? 1 : 2;
}

RAW_IN_HD uint32_t raw_in_aa(const uint8_t *m) { return (uint32_t) m[1] << 16 | (uint32_t) m[2] << 8 | m[3]; }   // getbits(msg, 9, 32)

// the beast signal byte the reference writes for mm->signalLevel (net_io.c:1696-1700) of an Aerobits value of mv millivolts:
// nearbyint(sqrt(fmin(1, (mv / 1000)^2)) * 255), at least 1 for a signal above 0.  In integers: |mv| * 255 / 1000 rounded half to
// even (the products with a half are |mv| = 100, 300, 500, 700, 900, where the double arithmetic gives the exact .5 too).
RAW_IN_HD uint32_t raw_in_mv_byte(long long mv) {
    const unsigned long long a = mv < 0 ? 0ull - (unsigned long long) mv : (unsigned long long) mv;
    if (a >= 1000) return 255;
    const uint32_t t = (uint32_t) a * 255u, q = t / 1000u, r = t % 1000u;
    const uint32_t b = q + ((r > 500u || (r == 500u && (q & 1u))) ? 1u : 0u);
    return a != 0 && b < 1 ? 1u : b;
}

RAW_IN_HD void raw_in_zero(RawInLine &o) {
    o.msg.timestamp = 0; o.msg.sysTimestamp = 0; o.msg.sig_sumsq = 0; o.msg.sig_len = 0; o.msg.score = 0; o.msg.phase = 0;
    o.msg.correctedbits = 0; o.msg.msgtype = 0; o.msg.msgbits = 0; o.msg.addr = 0;
    for (int i = 0; i < 14; ++i) { o.msg.msg[i] = 0; o.msg.raw[i] = 0; }
    o.signal = 0.0; o.cls = MGPU_RAW_NONE; o.addr = 0; o.adder = 0;
}

// The tail both inputs share (the beast input, beast_in_format.h, calls it too): a frame's bytes m[0..nbytes), nbytes 2, 7 or 14 and the
// rest zero, its timestamp, mm->signalLevel and the beast signal byte, to the record and the class: decodeModeAMessage, or
// decodeModesMessage (mode_s.c:443-606).  out is zeroed (raw_in_zero) by the caller.  Returns out.cls.
RAW_IN_HD uint32_t raw_in_decode_frame(uint8_t *m, uint32_t nbytes, uint64_t ts, double signal, uint32_t sig_byte, int64_t now_ms, const RawInConfig &cfg,
                                       const RawInTables &tb, RawInLine &out) {
    mgpu_msg &r = out.msg;
    r.timestamp = (int64_t) ts;
    r.sysTimestamp = now_ms;
    r.sig_sumsq = (uint64_t) (257u * sig_byte) * (257u * sig_byte);
    r.sig_len = 1;
    out.signal = signal;
    for (int i = 0; i < 14; ++i) r.raw[i] = m[i];

    if (nbytes == 2) {                                                       // decodeModeAMessage, mode_ac.c:165-200
        r.msgtype = 77;
        r.msgbits = 16;
        r.msg[0] = m[0]; r.msg[1] = m[1];
        r.addr = ((uint32_t) m[0] << 8 | m[1]) & 0xFF7Fu;                // low 24 bits of (ModeA & 0xFF7F) | MODES_NON_ICAO_ADDRESS
        out.addr = r.addr;
        return out.cls = MGPU_RAW_MODEAC;
    }

    // decodeModesMessage, mode_s.c:443-606
    uint32_t cls = MGPU_RAW_BAD, addr = 0, adder = 0, corrected = 0;
    uint32_t df = m[0] >> 3;
    bool zero = true;
    for (int i = 0; i < 7; ++i) zero = zero && m[i] == 0;
    if (!zero) {
        if (cfg.fixDF && cfg.nfix_crc && (df == 1 || df == 25 || df == 21 || df == 19 || df == 16)) {    // fixDF17msgtype, :276-301
            const uint8_t orig = m[0];
            m[0] = (uint8_t) ((orig & 7u) | (17u << 3));
            if (raw_in_crc(m, 112, tb.crc_byte) == 0) { df = 17; corrected = 1; } else m[0] = orig;
        }
        const uint32_t bits = (df & 0x10u) ? 112u : 56u;
        const uint32_t crc = raw_in_crc(m, bits, tb.crc_byte);
        uint32_t b0 = 0xff, b1 = 0xff;
        r.msgbits = (uint8_t) bits;
        if (df == 0 || df == 4 || df == 5 || df == 16 || df == 20 || df == 21 || df >= 24) {             // Address/Parity
            cls = MGPU_RAW_COND;
            addr = crc;
        } else if (df == 11) {
            if (crc & 0xffff80u) {
                const int ne = raw_in_diagnose(tb.tab_short, tb.n_short, crc, b0, b1);
                if (ne == 1) {                                           // (two-bit errors are ambiguous in DF11)
                    corrected = 1;
                    m[b0 >> 3] ^= (uint8_t) (0x80u >> (b0 & 7u));
                    cls = MGPU_RAW_COND;
                    addr = raw_in_aa(m);
                }
            } else {
                cls = MGPU_RAW_ACCEPT;
                addr = raw_in_aa(m);
                adder = (crc & 0x7fu) == 0;
            }
        } else if (df == 17 || df == 18) {
            if (crc != 0) {
                const int ne = raw_in_diagnose(tb.tab_long, tb.n_long, crc, b0, b1);
                if (ne >= 1) {
                    const uint32_t addr1 = raw_in_aa(m);
                    corrected = (uint32_t) ne;
                    m[b0 >> 3] ^= (uint8_t) (0x80u >> (b0 & 7u));
                    if (ne == 2) m[b1 >> 3] ^= (uint8_t) (0x80u >> (b1 & 7u));
                    addr = raw_in_aa(m);
                    cls = addr1 != addr ? MGPU_RAW_COND : MGPU_RAW_ACCEPT;
                }
            } else {
                cls = MGPU_RAW_ACCEPT;
                addr = raw_in_aa(m);
                adder = df == 17 && corrected == 0;
            }
        }
    }
    r.correctedbits = (uint8_t) corrected;
    r.msgtype = (uint8_t) df;
    r.addr = addr;
    for (int i = 0; i < 14; ++i) r.msg[i] = m[i];
    out.addr = addr;
    out.adder = adder;
    return out.cls = cls;
}

// One line.  Returns out.cls.
RAW_IN_HD uint32_t raw_in_line(const uint8_t *p, uint32_t n, int64_t now_ms, const RawInConfig &cfg, const RawInTables &tb, RawInLine &out) {
    raw_in_zero(out);
    if (n > kRawInMaxLine) return MGPU_RAW_NONE;
    // readAscii, net_io.c:4627: one '\r' in front of the terminator, unless it is the line's only byte
    if (n >= 2 && p[n - 1] == '\r') --n;
    // decodeHexMessage :4116-4123
    uint32_t l = n;
    while (l && raw_in_isspace(p[l - 1])) --l;
    while (l && raw_in_isspace(p[0])) { ++p; --l; }
    if (l == 0) return MGPU_RAW_NONE;                                     // (the departure: the reference reads hex[-1])

    uint64_t ts = 0;
    double signal = 0.0;
    uint32_t sig_byte = 0;
    if (p[l - 1] == ')') {                                               // the Aerobits suffix (SIGS,SIGQ,TS), :4129-4165
        uint32_t pos = l - 1;
        while (pos && p[pos] != '(') --pos;
        if (!pos) return MGPU_RAW_NONE;
        // strtok_r over p[pos + 1 .. l - 1) on ","
        uint32_t at = pos + 1;
        const uint32_t end = l - 1;
        uint32_t tok[3], len[3], nt = 0;
        while (nt < 3) {
            while (at < end && p[at] == ',') ++at;
            if (at >= end) break;
            tok[nt] = at;
            while (at < end && p[at] != ',') ++at;
            len[nt] = at - tok[nt];
            ++nt;
            if (at < end) ++at;                                          // the comma strtok_r overwrites
        }
        if (nt < 2) return MGPU_RAW_NONE;
        const long long mv = raw_in_strtol(p + tok[0], len[0], 10);
        signal = (double) mv;
        signal = signal / 1000.0;
        signal = signal * signal;
        signal = signal < 1.0 ? signal : 1.0;                            // fmin(1.0, x); x is never a NaN
        sig_byte = raw_in_mv_byte(mv);
        if (nt == 3) {
            const int after_pps = (int) (uint32_t) (unsigned long long) raw_in_strtol(p + tok[2], len[2], 16);   // the int truncation
            int64_t seconds = now_ms / 1000;
            if ((int64_t) (after_pps / 1000) > (now_ms % 1000) + 500) seconds -= 1;
            ts = ((uint64_t) seconds * 1000000ull + (uint64_t) (int64_t) after_pps) * 12ull;
        } else {
            ts = (uint64_t) (int64_t) ((double) now_ms * 12e3);
        }
        l = pos;
    }
    if (p[l - 1] != ';') return MGPU_RAW_NONE;
    if (l <= 4) return MGPU_RAW_NONE;

    int fl;                                                              // the frame's hex digits: p[fa .. fa + fl)
    uint32_t fa;
    bool beast_sig = false;
    switch (p[0]) {
        case '<': {
            int ll = (int) l - 2;
            if (ll < 12) return MGPU_RAW_NONE;
            for (uint32_t j = 0; j < 12; ++j) ts = (ts << 4) | (uint64_t) (int64_t) raw_in_hexval(p[1 + j]);
            ll -= 12;
            if (ll < 2) return MGPU_RAW_NONE;
            // ((hexDigitVal(a) << 4) | hexDigitVal(b)) / 255.0 as the compiled reference computes it: -1 << 4 is -16
            const int v = (raw_in_hexval(p[13]) * 16) | raw_in_hexval(p[14]);
            signal = (double) v / 255.0;
            signal = signal * signal;
            sig_byte = (uint32_t) (v < 0 ? -v : v);                      // nearbyint(sqrt(signal) * 255)
            beast_sig = true;
            fa = 15; fl = ll - 2;
            break;
        }
        case '@': {
            int ll = (int) l - 2;
            if (ll <= 12) return MGPU_RAW_NONE;
            for (uint32_t j = 0; j < 12; ++j) ts = (ts << 4) | (uint64_t) (int64_t) raw_in_hexval(p[1 + j]);
            fa = 13; fl = ll - 12;
            break;
        }
        case '%': fa = 13; fl = (int) l - 14; break;                     // (shorter than 14: falls out below, nothing beyond l is read)
        case '*':
        case ':': fa = 1; fl = (int) l - 2; break;
        default: return MGPU_RAW_NONE;
    }
    (void) beast_sig;
    if (fl != 4 && fl != 14 && fl != 28) return MGPU_RAW_NONE;
    if (!cfg.mode_ac && fl == 4) return MGPU_RAW_NONE;
    uint8_t m[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < fl; j += 2) {
        const int hi = raw_in_hexval(p[fa + (uint32_t) j]), lo = raw_in_hexval(p[fa + (uint32_t) j + 1]);
        if (hi < 0 || lo < 0) return MGPU_RAW_NONE;
        m[j / 2] = (uint8_t) (hi << 4 | lo);
    }

    return raw_in_decode_frame(m, (uint32_t) fl / 2u, ts, signal, sig_byte, now_ms, cfg, tb, out);
}

}  // namespace mgpu
