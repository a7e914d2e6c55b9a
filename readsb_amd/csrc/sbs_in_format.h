// sbs_in_format.h — one BaseStation (SBS) line to the aircraft record readsb's SBS input leaves (decodeSbsLine, net_io.c:2952-3178,
// behind readAscii, net_io.c:4599-4641; the MLAT, JAERO and PRIO wrappers :81-92), restated: ONE parser, __host__ __device__ and
// templated on how a number outside the plain form is resolved, for the size pass and the write pass of kernels/sbs_in.inc (which
// resolve nothing: such a line is deferred) and for the host (sbs_in_host.cpp: mgpu_sbs_parse_host, which resolves with the host's
// strtol and strtod; tests/host_stub/sbs_in_format_check.cpp runs both against the reference's records under ASan and UBSan).
//
// sbs_in_line(s, n, source, now_ms, resolve, rec) sees the n bytes of a line without its terminator ('\n' or NUL), a trailing '\r'
// still on it; a caller that found no terminator within kSbsInLook bytes passes any n > kSbsInMaxLen: such a line is invalid whatever
// it holds, and nothing of it is read.  The field rules and their line numbers are in include/modes_gpu.h.
//   Numbers: atoi / strtol tokens in the form [+-]?[0-9]{1,9}, strtod tokens in the form [+-]?[0-9]*(\.[0-9]*)? with a digit, at most
//     15 significant digits and at most 22 behind the point, are read here: the latter as M / 10^f, M < 10^15 < 2^53 and
//     10^f = 5^f * 2^f exact (5^22 < 2^53), so the ONE correctly rounded division gives the double nearest to the decimal, which is
//     what strtod returns.  Nothing else in this file is floating point but the conversions to float and two comparisons with 0.
//   Every other form goes to resolve.integer / resolve.real; where that declines, the line is SBS_IN_DEFER.
// Nothing here is indexed at run time but the line: the comma positions are bytes of three words, the callsign one word.
#pragma once
#include <cstdint>

#include "../../include/modes_gpu.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBS_IN_HD __host__ __device__ inline
#else
#define SBS_IN_HD inline
#endif

enum : int { SBS_IN_NONE = 0, SBS_IN_INVALID = 1, SBS_IN_RECORD = 2, SBS_IN_DEFER = 3 };

constexpr uint32_t kSbsInMaxLen = 200;           // max_len, net_io.c:2954: a line of this length or more is invalid
constexpr uint32_t kSbsInMinLen = 20;            // :2960
constexpr uint32_t kSbsInLook = kSbsInMaxLen + 1;   // bytes of a line that decide everything: 200 and a '\r'
constexpr uint32_t kSbsInTokens = 22;            // :2967
// a line that gives a record, or is deferred, has kSbsInMinLen bytes and a terminator
constexpr uint64_t sbs_in_max_recs(uint64_t nbytes) { return nbytes / (kSbsInMinLen + 1) + 1; }

// the device's resolver: nothing but the plain forms
struct SbsInPlainOnly {
    SBS_IN_HD bool integer(const uint8_t *, uint32_t, long long &) const { return false; }
    SBS_IN_HD bool real(const uint8_t *, uint32_t, double &) const { return false; }
};

struct SbsInTok {
    uint32_t at, len;
};

// atoi / strtol of a token
template <class Resolve>
SBS_IN_HD bool sbs_in_long(const uint8_t *t, uint32_t len, const Resolve &res, long long &v) {
    uint32_t i = 0;
    bool neg = false;
    if (len && (t[0] == '+' || t[0] == '-')) { neg = t[0] == '-'; i = 1; }
    const uint32_t nd = len - i;
    if (nd >= 1 && nd <= 9) {
        long long m = 0;
        bool ok = true;
        for (; i < len; ++i) {
            const uint32_t d = (uint32_t) t[i] - '0';
            ok = ok && d <= 9;
            m = m * 10 + (long long) (d & 15u);
        }
        if (ok) { v = neg ? -m : m; return true; }
    }
    return res.integer(t, len, v);
}

// strtod of a token
template <class Resolve>
SBS_IN_HD bool sbs_in_double(const uint8_t *t, uint32_t len, const Resolve &res, double &v) {
    uint32_t i = 0;
    bool neg = false, point = false, ok = true;
    if (len && (t[0] == '+' || t[0] == '-')) { neg = t[0] == '-'; i = 1; }
    uint64_t m = 0;
    uint32_t digits = 0, sig = 0, frac = 0;
    for (; i < len; ++i) {
        const uint32_t c = t[i];
        if (c == '.' && !point) { point = true; continue; }
        const uint32_t d = c - '0';
        if (d > 9) { ok = false; break; }
        ++digits;
        frac += point;
        if (sig || d) ++sig;
        if (sig <= 15) m = m * 10 + d;
    }
    if (ok && digits >= 1 && sig <= 15 && frac <= 22) {
        uint64_t p5 = 1;
        for (uint32_t k = 0; k < frac; ++k) p5 *= 5;
        const double den = (double) p5 * (double) (1ull << frac);    // 10^frac, exact
        const double q = (double) m / den;
        v = neg ? -q : q;
        return true;
    }
    return res.real(t, len, v);
}

SBS_IN_HD bool sbs_in_is(const uint8_t *s, SbsInTok t, char a) { return t.len == 1 && s[t.at] == (uint8_t) a; }
SBS_IN_HD bool sbs_in_is(const uint8_t *s, SbsInTok t, char a, char b) { return t.len == 2 && s[t.at] == (uint8_t) a && s[t.at + 1] == (uint8_t) b; }

SBS_IN_HD int sbs_in_hex(uint32_t c) {           // hexDigitVal, net_io.c:1815
    if (c >= '0' && c <= '9') return (int) c - '0';
    if (c >= 'A' && c <= 'F') return (int) c - 'A' + 10;
    if (c >= 'a' && c <= 'f') return (int) c - 'a' + 10;
    return -1;
}

SBS_IN_HD bool sbs_in_source_ok(uint32_t source) {
    return source == MGPU_SBS_SOURCE_SBS || source == MGPU_SBS_SOURCE_MLAT || source == MGPU_SBS_SOURCE_JAERO || source == MGPU_SBS_SOURCE_PRIO;
}

template <class Resolve>
SBS_IN_HD int sbs_in_line(const uint8_t *s, uint32_t n, uint32_t source, int64_t now_ms, const Resolve &res, mgpu_sbs_rec &r) {
    if (n > kSbsInMaxLen) return SBS_IN_INVALID;                     // 201 bytes: 200 after a '\r' at the most
    if (n >= 2 && s[n - 1] == '\r') --n;                              // readAscii, :4627: p - 1 > c->som
    if (n < 2) return SBS_IN_NONE;                                    // heartbeat, :2958
    if (n < kSbsInMinLen || n >= kSbsInMaxLen) return SBS_IN_INVALID;
    // strsep, :3002-3006: comma k (0 ..) at byte k & 7 of w[k >> 3]
    uint64_t w0 = 0, w1 = 0, w2 = 0;
    uint32_t nc = 0;
    for (uint32_t i = 0; i < n && nc < kSbsInTokens; ++i) {
        if (s[i] != ',') continue;
        const uint64_t bits = (uint64_t) i << (8u * (nc & 7u));
        if (nc < 8) w0 |= bits; else if (nc < 16) w1 |= bits; else w2 |= bits;
        ++nc;
    }
    if (nc < kSbsInTokens - 1) return SBS_IN_INVALID;
    auto comma = [&](uint32_t k) -> uint32_t { return (uint32_t) ((k < 8 ? w0 : k < 16 ? w1 : w2) >> (8u * (k & 7u))) & 255u; };
    auto tok = [&](uint32_t i) -> SbsInTok {                          // t[i], 1 <= i <= 22
        const uint32_t at = i == 1 ? 0u : comma(i - 2) + 1u, end = i <= nc ? comma(i - 1) : n;
        return SbsInTok{at, end - at};
    };
    const SbsInTok t1 = tok(1), t2 = tok(2), t5 = tok(5);
    if (t1.len != 3 || s[0] != 'M' || s[1] != 'S' || s[2] != 'G') return SBS_IN_INVALID;
    if (t2.len != 1) return SBS_IN_INVALID;
    if (t5.len != 6) return SBS_IN_INVALID;
    uint32_t addr = 0;
    for (uint32_t j = 0; j < 6; ++j) {
        const int h = sbs_in_hex(s[t5.at + j]);
        if (h < 0) return SBS_IN_INVALID;
        addr = addr << 4 | (uint32_t) h;
    }
    r = mgpu_sbs_rec{};
    r.sysTimestamp = now_ms;
    r.addr = addr;
    r.source = (uint8_t) source;
    r.addrtype = source == MGPU_SBS_SOURCE_MLAT ? 5 : source == MGPU_SBS_SOURCE_JAERO ? 4 : 6;   // ADDR_MLAT, ADDR_JAERO, ADDR_OTHER
    const uint32_t c2 = (uint32_t) s[t2.at] - '0';
    r.sbsMsgType = (uint8_t) (c2 <= 9 ? c2 : 0);
    uint32_t flags = 0, sbs = 0;
    long long iv = 0;
    double dv = 0;

    const SbsInTok t11 = tok(11);
    if (t11.len) {                                                    // :3035-3051
        uint64_t cs = 0;
        for (uint32_t k = 0; k < 8; ++k)
            if (k < t11.len) cs |= (uint64_t) s[t11.at + k] << (8u * k);
        bool good = true;
        for (uint32_t k = 0; k < 8 && good; ++k) {
            uint32_t c = (uint32_t) (cs >> (8u * k)) & 255u;
            if (c == 0) { c = ' '; cs |= (uint64_t) ' ' << (8u * k); }
            good = (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == ' ';
        }
        for (uint32_t k = 0; k < 8; ++k) r.callsign[k] = (char) (uint8_t) (cs >> (8u * k));
        if (good) flags |= MGPU_F_CALLSIGN_VALID;
    }
    const SbsInTok t12 = tok(12);
    if (t12.len) {                                                    // :3053-3060
        if (!sbs_in_long(s + t12.at, t12.len, res, iv)) return SBS_IN_DEFER;
        r.baro_alt = (int32_t) iv;
        if (r.baro_alt > -5000 && r.baro_alt < 100000) flags |= MGPU_F_BARO_ALT_VALID;      // (baro_alt_unit = UNIT_FEET = 0)
    }
    const SbsInTok t13 = tok(13);
    if (t13.len) {                                                    // :3062-3067
        if (!sbs_in_double(s + t13.at, t13.len, res, dv)) return SBS_IN_DEFER;
        r.gs_v0 = (float) dv;
        if (r.gs_v0 > 0) flags |= MGPU_F_GS_VALID;
    }
    const SbsInTok t14 = tok(14);
    if (t14.len) {                                                    // :3069-3074
        if (!sbs_in_double(s + t14.at, t14.len, res, dv)) return SBS_IN_DEFER;
        r.heading = (float) dv;
        r.heading_type = 1;                                           // HEADING_GROUND_TRACK
        flags |= MGPU_F_HEADING_VALID;
    }
    const SbsInTok t15 = tok(15), t16 = tok(16);
    if (t15.len && t16.len) {                                         // :3076-3082
        if (!sbs_in_double(s + t15.at, t15.len, res, dv)) return SBS_IN_DEFER;
        r.decoded_lat = dv;
        if (!sbs_in_double(s + t16.at, t16.len, res, dv)) return SBS_IN_DEFER;
        r.decoded_lon = dv;
        if (r.decoded_lat != 0 && r.decoded_lon != 0) sbs |= MGPU_SBS_POS_VALID;
    }
    const SbsInTok t17 = tok(17);
    if (t17.len) {                                                    // :3084-3088
        if (!sbs_in_long(s + t17.at, t17.len, res, iv)) return SBS_IN_DEFER;
        r.baro_rate = (int32_t) iv;
        flags |= MGPU_F_BARO_RATE_VALID;
    }
    const SbsInTok t18 = tok(18);
    if (t18.len) {                                                    // :3090-3098
        if (!sbs_in_long(s + t18.at, t18.len, res, iv)) return SBS_IN_DEFER;
        if (iv > 0) {
            const uint32_t q = (uint32_t) iv;
            r.squawkDec = q;
            r.squawkHex = (q / 1000 % 10) * 4096 + (q / 100 % 10) * 256 + (q / 10 % 10) * 16 + q % 10;   // squawkDec2Hex, track.h:742
            flags |= MGPU_F_SQUAWK_VALID;
        }
    }
    const SbsInTok t19 = tok(19), t20 = tok(20), t21 = tok(21), t22 = tok(22);
    if (t19.len) {                                                    // :3100-3111
        if (!sbs_in_long(s + t19.at, t19.len, res, iv)) return SBS_IN_DEFER;
        if (iv > 0 && source == MGPU_SBS_SOURCE_MLAT) r.receiverCountMlat = (int32_t) iv;
        else if (sbs_in_is(s, t19, '0')) flags |= MGPU_F_ALERT_VALID;
        else if (sbs_in_is(s, t19, '-', '1')) flags |= MGPU_F_ALERT_VALID | MGPU_F_ALERT;
    }
    if (t20.len) {                                                    // :3114-3129: the flag's value is read from t[21]
        if (!sbs_in_long(s + t20.at, t20.len, res, iv)) return SBS_IN_DEFER;
        if (iv > 0 && source == MGPU_SBS_SOURCE_MLAT) r.mlatEPU = iv > 65535 ? 65535 : (int32_t) iv;
        else if (sbs_in_is(s, t21, '0')) sbs |= MGPU_SBS_EMERGENCY_VALID;
        else if (sbs_in_is(s, t21, '-', '1')) sbs |= MGPU_SBS_EMERGENCY_VALID | MGPU_SBS_EMERGENCY;
    }
    if (sbs_in_is(s, t21, '1')) flags |= MGPU_F_SPI_VALID | MGPU_F_SPI;          // :3132-3140
    else if (sbs_in_is(s, t21, '0')) flags |= MGPU_F_SPI_VALID;
    if (t22.len >= 2 && s[t22.at] == '-' && s[t22.at + 1] == '1') r.airground = 1;          // :3143-3150: strncmp; AG_GROUND
    else if (t22.len >= 1 && s[t22.at] == '0') r.airground = 2;                              // AG_AIRBORNE
    r.flags = flags;
    r.sbs_flags = sbs;
    return SBS_IN_RECORD;
}
