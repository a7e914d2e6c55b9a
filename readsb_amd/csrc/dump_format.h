// dump_format.h — the decoded-message dump of displayModesMessage (mode_s.c:1809-2239) with the line printACASInfoShort adds
// (json_out.c:443-629, a == NULL), restated from its formats: ONE formatter, __host__ __device__ and templated on the sink, for the
// counting pass and the writing pass of kernels/dump.inc and for the host (behind_out.cpp: mgpu_dump_format_host;
// tests/host_stub/dump_format_check.cpp runs it against the reference's bytes under ASan and UBSan).  The three cannot disagree
// about a length.
//
// A sink has put(c) for one byte and lit(p, n) for n bytes of a literal.  Digits go straight to the sink, most significant first:
// no char buffer indexed at run time, which would live in private memory on the device.
//
// Every %...f is reproduced exactly, in integer arithmetic: dump_scale() multiplies the 53-bit mantissa of the (promoted) double by
// 10^N and shifts, rounding half to even on the bits shifted out — what printf does with the exact binary value.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/modes_gpu.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DUMP_HD __host__ __device__ inline
#else
#define DUMP_HD inline
#endif

enum : int { DUMP_NONE = 0, DUMP_LINE = 1, DUMP_DEFER = 2, DUMP_SKIP = 3 };

constexpr int64_t kDumpMsEnd = 253402300800000ll;                // 10000-01-01: sysTimestamp lies in [0, kDumpMsEnd)
constexpr uint32_t kDumpHexUnknown = 0xDEADBEEFu;                // HEX_UNKNOWN, readsb.h:144
constexpr uint32_t kDumpNonIcao = 1u << 24;                      // MODES_NON_ICAO_ADDRESS, readsb.h:295

// one message as the formatter sees it: the two records and the caller's optional per-message values (0 / null where absent)
struct DumpIn {
    const mgpu_msg *m;
    const mgpu_fields *f;
    const mgpu_position *pos;
    uint64_t receiver_id;
    uint32_t decoded_rc;
    uint8_t reduce_forward, decoded_nic;
};

struct DumpCountSink {
    uint32_t n;
    DUMP_HD void put(uint32_t) { ++n; }
    DUMP_HD void lit(const char *, uint32_t k) { n += k; }
};
struct DumpByteSink {
    uint8_t *p;
    DUMP_HD void put(uint32_t c) { *p++ = (uint8_t) c; }
    DUMP_HD void lit(const char *q, uint32_t k) { for (uint32_t j = 0; j < k; ++j) *p++ = (uint8_t) q[j]; }
};

struct DumpStr { const char *p; uint32_t n; };
#define DUMP_S(x) DumpStr{x, (uint32_t) sizeof(x) - 1u}
#define DUMP_LIT(s, x) (s).lit(x, (uint32_t) sizeof(x) - 1u)

template <class S> DUMP_HD void dump_str(S &s, DumpStr t) { s.lit(t.p, t.n); }
template <class S> DUMP_HD void dump_pad(S &s, int k) { for (; k > 0; --k) s.put(' '); }

DUMP_HD int dump_udigits(uint64_t v) {
    int d = 1;
    for (uint64_t p = 10; d < 20 && v >= p; p *= 10) ++d;
    return d;
}
// the digits of v, at least `mind` of them (zero padded)
template <class S> DUMP_HD void dump_udec(S &s, uint64_t v, int mind = 1) {
    int d = dump_udigits(v);
    for (int k = mind; k > d; --k) s.put('0');
    uint64_t p = 1;
    for (int k = 1; k < d; ++k) p *= 10;
    for (; p; p /= 10) { const uint64_t q = v / p; s.put('0' + (uint32_t) q); v -= q * p; }
}
// %<width>d / %0<width>d of a signed value: the sign counts towards the width
template <class S> DUMP_HD void dump_idec(S &s, int64_t v, int width = 0, bool zero = false) {
    const bool neg = v < 0;
    const uint64_t a = neg ? 0ull - (uint64_t) v : (uint64_t) v;
    const int d = dump_udigits(a) + (neg ? 1 : 0);
    if (!zero) dump_pad(s, width - d);
    if (neg) s.put('-');
    dump_udec(s, a, zero ? width - (neg ? 1 : 0) : 1);
}
// %0<mind>x / %0<mind>X
template <class S> DUMP_HD void dump_hex(S &s, uint64_t v, int mind, bool upper) {
    for (int k = 15; k >= 0; --k) {
        const uint32_t nib = (uint32_t) (v >> (4 * k)) & 15u;
        if (k < mind || (v >> (4 * k))) s.put(nib < 10u ? '0' + nib : (upper ? 'A' : 'a') - 10u + nib);
    }
}
template <class S> DUMP_HD void dump_2(S &s, uint32_t v) { s.put('0' + v / 10u); s.put('0' + v % 10u); }

DUMP_HD uint64_t dump_bits(double x) { uint64_t b; __builtin_memcpy(&b, &x, 8); return b; }
DUMP_HD uint32_t dump_bitsf(float x) { uint32_t b; __builtin_memcpy(&b, &x, 4); return b; }

// round-half-even(|x| * mul) for 0 <= |x| < 2^53, mul <= 10^6, the result below 2^64: |x| = m * 2^-sh with the 53-bit integer m, so
// the product is (m * mul) >> sh with m * mul < 2^73 held in two halves; the bits shifted out are the exact remainder.  Subnormals and
// zero (exponent field 0) take the same path.
DUMP_HD uint64_t dump_scale(double x, uint32_t mul) {
    const uint64_t bits = dump_bits(x);
    const uint32_t ex = (uint32_t) (bits >> 52) & 0x7ffu;
    const uint64_t m = (bits & 0xfffffffffffffull) | (ex ? 1ull << 52 : 0ull);
    uint32_t sh = 1075u - (ex ? ex : 1u);                         // 0 .. 1074 (ex <= 1075 as |x| < 2^53)
    if (sh > 127u) sh = 127u;                                     // beyond 74 everything is remainder below the half: the same answer
    const uint64_t ml = m & 0xffffffffull, mh = m >> 32;
    const uint64_t pl = ml * mul, ph = mh * mul;                  // < 2^52, < 2^41
    const uint64_t lo = pl + (ph << 32);
    const uint64_t hi = (ph >> 32) + (lo < pl ? 1ull : 0ull);
    if (sh == 0u) return lo;
    uint64_t q;
    bool half, sticky;
    if (sh < 64u) {
        q = (lo >> sh) | (hi << (64u - sh));
        half = (lo >> (sh - 1u)) & 1u;
        sticky = (lo & ((1ull << (sh - 1u)) - 1ull)) != 0;
    } else if (sh == 64u) {
        q = hi;
        half = lo >> 63;
        sticky = (lo & 0x7fffffffffffffffull) != 0;
    } else {
        const uint32_t t = sh - 64u;
        q = hi >> t;
        half = (hi >> (t - 1u)) & 1u;
        sticky = (hi & ((1ull << (t - 1u)) - 1ull)) != 0 || lo != 0;
    }
    if (half && (sticky || (q & 1ull))) ++q;
    return q;
}
DUMP_HD uint32_t dump_pow10(int k) { uint32_t p = 1; for (; k > 0; --k) p *= 10u; return p; }

// "<spaces>[-]ip.frac" with `dec` decimals, right-aligned in `width`
template <class S> DUMP_HD void dump_fixed(S &s, bool neg, uint64_t ip, uint32_t frac, int dec, int width) {
    dump_pad(s, width - (dump_udigits(ip) + (neg ? 1 : 0) + 1 + dec));
    if (neg) s.put('-');
    dump_udec(s, ip);
    s.put('.');
    dump_udec(s, frac, dec);
}
// %<width>.<dec>f of a double with |x| < 2^53 / 10^dec, dec <= 6; the sign from the sign bit ("-0.0" for -0.0 and for negatives that
// round to zero)
template <class S> DUMP_HD void dump_f(S &s, double x, int dec, int width = 0) {
    const uint32_t p = dump_pow10(dec);
    const uint64_t v = dump_scale(x, p);
    dump_fixed(s, dump_bits(x) >> 63, v / p, (uint32_t) (v % p), dec, width);
}

// signalLevel exactly as demod_2400.c:447-448 (mgpu_msg_signal_level, for either side)
DUMP_HD double dump_signal_level(const mgpu_msg &m) { return (double) m.sig_sumsq / 65535.0 / 65535.0 / (double) m.sig_len; }
DUMP_HD bool dump_float_ok(float x) { return fabsf(x) < 2147483648.0f; }                    // false for NaN and infinities
DUMP_HD bool dump_has_position(const DumpIn &in) {
    return in.pos && (in.pos->method == MGPU_CPR_GLOBAL || in.pos->method == MGPU_CPR_LOCAL_RECEIVER || in.pos->method == MGPU_CPR_LOCAL_AIRCRAFT);
}

// mm->crc as mode_s.c:466 leaves it: modesChecksum (crc.c:67-82) of the sliced frame after fixDF17msgtype (:276-301) put DF17 into
// its first five bits, before the CRC repair.  Polynomial division bit by bit (generator 0xfff409), bits = 56 or 112.  No table on
// purpose: the division runs once per message and pass, 88 shift / xor steps beside the thousands of steps of the sinks, and a table
// here would be a second copy of tables.h's, indexed at run time, in a header both sides compile.
DUMP_HD uint32_t dump_crc(const mgpu_msg &m, uint32_t msgtype) {
    const int n = m.msgbits / 8;
    uint32_t rem = 0;
    for (int i = 0; i < n - 3; ++i) {
        uint32_t b = m.raw[i];
        if (i == 0 && msgtype == 17u && (b >> 3) != 17u) b = (b & 7u) | (17u << 3);
        rem ^= b << 16;
        for (int k = 0; k < 8; ++k) rem = (rem & 0x800000u) ? ((rem << 1) ^ 0xfff409u) & 0xffffffu : (rem << 1) & 0xffffffu;
    }
    return rem ^ ((uint32_t) m.raw[n - 3] << 16) ^ ((uint32_t) m.raw[n - 2] << 8) ^ (uint32_t) m.raw[n - 1];
}

// The RSSI value, 10 * log10(signalLevel) to one decimal, as tenths: *tenths = round(|y| * 10).  Device (exact_log == false): certain
// iff the fraction of |y| * 10 is at least 2^-20 away from the half; this library's and the host's log10 differ by a few ulp of a value
// below 150, about 1e-13.  Host (exact_log == true): y is the host libm's, the rounding printf's own, never uncertain.
DUMP_HD bool dump_rssi(double level, bool exact_log, uint32_t *tenths) {
    if (level == 1.0) { *tenths = 0; return true; }
    const double y = fabs(10.0 * log10(level));
    if (exact_log) { *tenths = (uint32_t) dump_scale(y, 10u); return true; }
    const double t = y * 10.0, fl = floor(t), fr = t - fl;
    *tenths = (uint32_t) fl + (fr > 0.5 ? 1u : 0u);
    return fabs(fr - 0.5) >= 0x1p-20;
}

// Who gets a dump, in this order: MGPU_DUMP_QUIET (no dump, counted nowhere), the domain of what THIS mode prints (DUMP_SKIP), the one
// transcendental (DUMP_DEFER).  ONLYADDR prints nothing that has a domain; RAW the frame only.
DUMP_HD int dump_classify(const DumpIn &in, uint32_t mode, uint32_t show_only, bool exact_log) {
    const mgpu_msg &m = *in.m;
    const mgpu_fields &f = *in.f;
    if ((mode & MGPU_DUMP_QUIET) && f.addr != show_only) return DUMP_NONE;
    if (mode & MGPU_DUMP_ONLYADDR) return DUMP_LINE;
    // the frame line reads msgbits / 8 bytes of msg[14]; modesChecksum needs three of them
    if (!(m.msgbits == 56u || m.msgbits == 112u || (m.msgbits == 16u && f.msgtype >= 32u))) return DUMP_SKIP;
    if (mode & MGPU_DUMP_RAW) return DUMP_LINE;
    bool ok = m.sysTimestamp >= 0 && m.sysTimestamp < kDumpMsEnd && m.timestamp >= 0 && m.sig_len != 0;
    const uint32_t fl = f.flags;
    if (fl & MGPU_F_HEADING_VALID) ok = ok && dump_float_ok(f.heading);
    if (fl & MGPU_F_TRACK_RATE_VALID) ok = ok && dump_float_ok(f.track_rate);
    if (fl & MGPU_F_ROLL_VALID) ok = ok && dump_float_ok(f.roll);
    if (fl & MGPU_F_GS_VALID) {
        ok = ok && dump_float_ok(f.gs_selected);
        if (f.gs_v0 != f.gs_selected) ok = ok && dump_float_ok(f.gs_v0);
        if (f.gs_v2 != f.gs_selected) ok = ok && dump_float_ok(f.gs_v2);
    }
    if (fl & MGPU_F_MACH_VALID) ok = ok && dump_float_ok(f.mach);
    if (f.nav_flags & MGPU_NAV_HEADING_VALID) ok = ok && dump_float_ok(f.nav_heading);
    if (f.nav_flags & MGPU_NAV_QNH_VALID) ok = ok && dump_float_ok(f.nav_qnh);
    if ((fl & MGPU_F_CPR_VALID) && dump_has_position(in)) ok = ok && fabs(in.pos->lat) <= 90.0 && fabs(in.pos->lon) <= 360.0;   // false for NaN
    if (!ok) return DUMP_SKIP;
    if (m.sig_sumsq != 0) {
        uint32_t tenths;
        if (!dump_rssi(dump_signal_level(m), exact_log, &tenths)) return DUMP_DEFER;
    }
    return DUMP_LINE;
}

// ---- the enum strings (mode_s.c:1557-1806, toString.h) ----

DUMP_HD DumpStr dump_df_name(uint32_t df) {
    if (df == 77u) return DUMP_S("modeac");
    if (df > 32u) return DUMP_S("out of range");
    switch (df) {
    case 0: return DUMP_S("Short Air-Air Surveillance");
    case 4: return DUMP_S("Survelliance, Altitude Reply");
    case 5: return DUMP_S("Survelliance, Identity Reply");
    case 11: return DUMP_S("All Call Reply");
    case 16: return DUMP_S("Long Air-Air ACAS");
    case 17: return DUMP_S("Extended Squitter");
    case 18: return DUMP_S("Extended Squitter (Non-Transponder)");
    case 19: return DUMP_S("Extended Squitter (Military)");
    case 20: return DUMP_S("Comm-B, Altitude Reply");
    case 21: return DUMP_S("Comm-B, Identity Reply");
    case 22: return DUMP_S("Military Use");
    case 24: case 25: case 26: case 27: case 28: case 29: case 30: case 31: return DUMP_S("Comm-D Extended Length Message");
    case 32: return DUMP_S("Mode A/C Reply");
    default: return DUMP_S("reserved");
    }
}
DUMP_HD DumpStr dump_es_name(uint32_t me, uint32_t sub) {
    if (me == 0u) return DUMP_S("No position information (airborne or surface)");
    if (me <= 4u) return DUMP_S("Aircraft identification and category");
    if (me <= 8u) return DUMP_S("Surface position");
    if (me <= 18u) return DUMP_S("Airborne position (barometric altitude)");
    if (me >= 20u && me <= 22u) return DUMP_S("Airborne position (geometric altitude)");
    switch (me) {
    case 19:
        switch (sub) {
        case 1: return DUMP_S("Airborne velocity over ground, subsonic");
        case 2: return DUMP_S("Airborne velocity over ground, supersonic");
        case 3: return DUMP_S("Airspeed and heading, subsonic");
        case 4: return DUMP_S("Airspeed and heading, supersonic");
        default: return DUMP_S("Unknown");
        }
    case 23: return sub == 0u ? DUMP_S("Test message") : sub == 7u ? DUMP_S("National use / 1090-WP-15-20 Mode A squawk") : DUMP_S("Unknown");
    case 24: return DUMP_S("Reserved for surface system status");
    case 27: return DUMP_S("Reserved for trajectory change");
    case 28: return sub == 1u ? DUMP_S("Emergency/priority status") : sub == 2u ? DUMP_S("ACAS RA broadcast") : DUMP_S("Unknown");
    case 29: return sub == 0u ? DUMP_S("Target state and status (V1)") : sub == 1u ? DUMP_S("Target state and status (V2)") : DUMP_S("Unknown");
    case 30: return DUMP_S("Aircraft Operational Coordination");
    case 31: return sub == 0u ? DUMP_S("Aircraft operational status (airborne)") : sub == 1u ? DUMP_S("Aircraft operational status (surface)") : DUMP_S("Unknown");
    default: return DUMP_S("Unknown");
    }
}
DUMP_HD DumpStr dump_commb_name(uint32_t v) {
    switch (v) {
    case 1: return DUMP_S("ambiguous format");
    case 2: return DUMP_S("empty response");
    case 3: return DUMP_S("BDS1,0 Datalink capabilities");
    case 4: return DUMP_S("BDS1,7 Common usage GICB capabilities");
    case 5: return DUMP_S("BDS2,0 Aircraft identification");
    case 6: return DUMP_S("BDS3,0 ACAS resolution advisory");
    case 7: return DUMP_S("BDS4,0 Selected vertical intention");
    case 8: return DUMP_S("BDS5,0 Track and turn report");
    case 9: return DUMP_S("BDS6,0 Heading and speed report");
    case 10: return DUMP_S("BDS4,4 Meteorological routine air report");
    default: return DUMP_S("unknown format");
    }
}
DUMP_HD DumpStr dump_addrtype_name(uint32_t v) {
    switch (v) {
    case 0: return DUMP_S("adsb_icao");
    case 1: return DUMP_S("adsb_icao_nt");
    case 2: return DUMP_S("adsr_icao");
    case 3: return DUMP_S("tisb_icao");
    case 4: return DUMP_S("adsc");
    case 5: return DUMP_S("mlat");
    case 6: return DUMP_S("other");
    case 7: return DUMP_S("mode_s");
    case 8: return DUMP_S("adsb_other");
    case 9: return DUMP_S("adsr_other");
    case 10: return DUMP_S("tisb_trackfile");
    case 11: return DUMP_S("tisb_other");
    case 12: return DUMP_S("mode_ac");
    default: return DUMP_S("unknown");
    }
}
DUMP_HD DumpStr dump_airground_name(uint32_t v) {
    switch (v) {
    case 0: return DUMP_S("invalid");
    case 1: return DUMP_S("ground");
    case 2: return DUMP_S("airborne");
    case 3: return DUMP_S("airborne?");
    default: return DUMP_S("(unknown airground state)");
    }
}
DUMP_HD DumpStr dump_unit_name(uint32_t v) { return v == 0u ? DUMP_S("ft") : v == 1u ? DUMP_S("m") : DUMP_S("(unknown altitude unit)"); }
DUMP_HD DumpStr dump_heading_name(uint32_t v) {
    switch (v) {
    case 1: return DUMP_S("Ground track");
    case 2: return DUMP_S("True heading");
    case 3: return DUMP_S("Mag heading");
    case 4: return DUMP_S("Heading");
    case 5: return DUMP_S("Track/Heading");
    default: return DUMP_S("unknown heading type");
    }
}
DUMP_HD DumpStr dump_cpr_name(uint32_t v) {
    return v == 1u ? DUMP_S("Surface") : v == 2u ? DUMP_S("Airborne") : v == 3u ? DUMP_S("TIS-B Coarse") : DUMP_S("unknown CPR type");
}
DUMP_HD DumpStr dump_sil_type_name(uint32_t v) {
    return v == 1u ? DUMP_S("unknown type") : v == 3u ? DUMP_S("per flight hour") : v == 2u ? DUMP_S("per sample") : DUMP_S("invalid type");
}
DUMP_HD DumpStr dump_emergency_name(uint32_t v) {
    switch (v) {
    case 0: return DUMP_S("no emergency");
    case 1: return DUMP_S("general emergency (7700)");
    case 2: return DUMP_S("lifeguard / medical emergency");
    case 3: return DUMP_S("minimum fuel");
    case 4: return DUMP_S("no communications (7600)");
    case 5: return DUMP_S("unlawful interference (7500)");
    case 6: return DUMP_S("downed aircraft");
    default: return DUMP_S("reserved");
    }
}

// "HH:MM:SS" of a second of the day
template <class S> DUMP_HD void dump_hms(S &s, uint32_t sec) {
    const uint32_t hh = sec / 3600u, mm = (sec - hh * 3600u) / 60u, ss = sec - hh * 3600u - mm * 60u;
    dump_2(s, hh); s.put(':'); dump_2(s, mm); s.put(':'); dump_2(s, ss);
}
// "YYYY-MM-DD" (%F) of a day since 1970: gmtime_r's calendar by the civil-from-days algorithm over eras of 400 years
template <class S> DUMP_HD void dump_ymd(S &s, uint32_t days) {
    const uint32_t z = days + 719468u;
    const uint32_t era = z / 146097u, doe = z - era * 146097u;
    const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
    const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);
    const uint32_t mp = (5u * doy + 2u) / 153u;
    const uint32_t d = doy - (153u * mp + 2u) / 5u + 1u;
    const uint32_t mo = mp < 10u ? mp + 3u : mp - 9u;
    const uint32_t y = yoe + era * 400u + (mo <= 2u ? 1u : 0u);
    dump_2(s, y / 100u); dump_2(s, y % 100u); s.put('-'); dump_2(s, mo); s.put('-'); dump_2(s, d);
}

// the line of sprintACASInfoShort (json_out.c:443-629) with a == NULL and without debug_ACAS, and printACASInfoShort's "\n"
template <class S> DUMP_HD void dump_acas(S &s, const mgpu_msg &m, const mgpu_fields &f) {
    uint64_t mv = 0;                                             // MV = msg[4..10]; getbit(MV, k) = bit 56 - k of it
    for (int k = 4; k < 11; ++k) mv = (mv << 8) | m.msg[k];
#define DUMP_BIT(k) ((uint32_t) (mv >> (56 - (k))) & 1u)
    const uint64_t ms = (uint64_t) m.sysTimestamp;
    const uint32_t days = (uint32_t) (ms / 86400000ull), rem = (uint32_t) (ms - (uint64_t) days * 86400000ull);
    dump_ymd(s, days);
    s.put(',');
    dump_hms(s, rem / 1000u);
    s.put('.'); s.put('0' + (rem % 1000u) / 100u);
    DUMP_LIT(s, ", ");
    dump_hex(s, f.addr, 6, false);
    DUMP_LIT(s, ",DF:,");
    dump_idec(s, f.msgtype, 2);
    DUMP_LIT(s, ",bytes:,");
    dump_hex(s, mv, 14, true);
    DUMP_LIT(s, ",           ,           ,     ,ft,     ,fpm,ARA:,");
    for (int k = 9; k <= 15; ++k) s.put('0' + DUMP_BIT(k));
    DUMP_LIT(s, ",RAT:,"); s.put('0' + DUMP_BIT(27));
    DUMP_LIT(s, ",MTE:,"); s.put('0' + DUMP_BIT(28));
    DUMP_LIT(s, ",RAC:,");
    for (int k = 23; k <= 26; ++k) s.put('0' + DUMP_BIT(k));
    DUMP_LIT(s, ", ");
    if ((mv >> 30) & 15u) {
        if (DUMP_BIT(23)) DUMP_LIT(s, "not below");
        if (DUMP_BIT(24)) DUMP_LIT(s, "not above");
        if (DUMP_BIT(25)) DUMP_LIT(s, "not left ");
        if (DUMP_BIT(26)) DUMP_LIT(s, "not right");
    } else DUMP_LIT(s, "         ");
    DUMP_LIT(s, ", ");
    const bool ara = DUMP_BIT(9), rat = DUMP_BIT(27), mte = DUMP_BIT(28);
    if (rat) DUMP_LIT(s, "Clear of Conflict");
    else if (ara) {
        DUMP_LIT(s, "RA:");
        const bool corr = DUMP_BIT(10), down = DUMP_BIT(11), increase = DUMP_BIT(12), reversal = DUMP_BIT(13), crossing = DUMP_BIT(14), positive = DUMP_BIT(15);
        if (corr && positive) {
            if (reversal && increase) DUMP_LIT(s, " Increase");
            if (down) DUMP_LIT(s, " Descend"); else DUMP_LIT(s, " Climb");
            if (reversal) {
                if (down) DUMP_LIT(s, "; Descend"); else DUMP_LIT(s, "; Climb");
                DUMP_LIT(s, " NOW");
            }
            if (crossing) {
                DUMP_LIT(s, "; Crossing");
                if (down) DUMP_LIT(s, " Descend"); else DUMP_LIT(s, " Climb");
            }
        }
        if (corr && !positive) DUMP_LIT(s, " Level Off");
        if (!corr && positive) {
            DUMP_LIT(s, " Maintain vertical Speed");
            if (crossing) DUMP_LIT(s, "; Crossing Maintain");
        }
        if (!corr && !positive) DUMP_LIT(s, " Monitor vertical Speed");
    } else if (mte) {
        DUMP_LIT(s, "RA multithreat:");
        if (DUMP_BIT(10)) DUMP_LIT(s, " correct upwards;");
        if (DUMP_BIT(11)) DUMP_LIT(s, " climb required;");
        if (DUMP_BIT(12)) DUMP_LIT(s, " correct downwards;");
        if (DUMP_BIT(13)) DUMP_LIT(s, " descent required;");
        if (DUMP_BIT(14)) DUMP_LIT(s, " crossing;");
        if (DUMP_BIT(15)) DUMP_LIT(s, " increase/maintain vertical rate"); else DUMP_LIT(s, "      reduce/limit vertical rate");
    }
    if (((mv >> 26) & 3u) == 1u) {                               // TTI, bits 29-30; the threat's address, bits 31-54
        DUMP_LIT(s, "; TIDh: ");
        dump_hex(s, (mv >> 2) & 0xffffffu, 6, false);
    }
    DUMP_LIT(s, ",\n");
#undef DUMP_BIT
}

// "addr:" + the nine characters of the hex line's address (msgtype < 32) or nothing, + one space
template <class S> DUMP_HD void dump_addr9(S &s, const mgpu_fields &f) {
    if (f.msgtype >= 32u) return;
    const uint32_t a = f.addr != kDumpHexUnknown ? f.addr : 0u;  // maybe_addr is a memset-0 message's
    s.put(a & kDumpNonIcao ? '~' : ' ');
    dump_hex(s, a & 0xffffffu, 6, false);
    if (f.addr != kDumpHexUnknown) DUMP_LIT(s, "  "); else DUMP_LIT(s, " ?");
}
// the bytes msg[from .. from + n) as uppercase hex pairs (print_hex_bytes)
template <class S> DUMP_HD void dump_bytes(S &s, const mgpu_msg &m, int from, int n) {
    for (int k = from; k < from + n; ++k) dump_hex(s, m.msg[k], 2, true);
}
template <class S> DUMP_HD void dump_kv(S &s, const char *key, uint32_t keylen, uint32_t v) {
    s.lit(key, keylen); dump_udec(s, v); s.put('\n');
}
#define DUMP_KV(s, key, v) dump_kv(s, key, (uint32_t) sizeof(key) - 1u, v)

// The dump of a message dump_classify() let through (DUMP_LINE; DUMP_DEFER on the host, with exact_log).
template <class S> DUMP_HD void dump_format(const DumpIn &in, uint32_t mode, bool exact_log, S &s) {
    const mgpu_msg &m = *in.m;
    const mgpu_fields &f = *in.f;
    if (mode & MGPU_DUMP_ONLYADDR) {                             // :1829-1832
        dump_hex(s, f.addr, 6, false); s.put('\n');
        return;
    }
    if ((mode & MGPU_DUMP_MLAT) && m.timestamp != 0) {           // :1835-1842: the whole value, 12 digits at least
        s.put('@');
        dump_hex(s, (uint64_t) m.timestamp, 12, true);
    } else s.put('*');
    for (int k = 0; k < 14; ++k)
        if (k < (int) (m.msgbits / 8u)) dump_hex(s, m.msg[k], 2, false);
    DUMP_LIT(s, ";\n");
    if (mode & MGPU_DUMP_RAW) return;

    const uint32_t df = f.msgtype, fl = f.flags;
    if (df < 32u) {                                              // :1851-1862
        DUMP_LIT(s, "hex: "); dump_addr9(s, f);
        DUMP_LIT(s, " CRC: "); dump_hex(s, dump_crc(m, df), 6, false);
        DUMP_LIT(s, " fixed bits: "); dump_udec(s, m.correctedbits);
        DUMP_LIT(s, " decode: ok\n");
    }
    if (m.sig_sumsq != 0) {                                      // :1864-1865: signalLevel > 0
        const double level = dump_signal_level(m);
        uint32_t tenths;
        (void) dump_rssi(level, exact_log, &tenths);
        DUMP_LIT(s, "RSSI: ");
        dump_fixed(s, level < 1.0, tenths / 10u, tenths % 10u, 1, 8);
        DUMP_LIT(s, " dBFS   ");
    }
    DUMP_LIT(s, "reduce_forward: "); dump_idec(s, (int8_t) in.reduce_forward); s.put('\n');
    if (m.score) { DUMP_LIT(s, "Score: "); dump_idec(s, m.score); s.put('\n'); }
    if (in.receiver_id) {                                        // sprint_uuid1, util.c:542-555
        DUMP_LIT(s, "receiverId: ");
        dump_hex(s, in.receiver_id >> 32, 8, false); s.put('-');
        dump_hex(s, (in.receiver_id >> 16) & 0xffffu, 4, false); s.put('-');
        dump_hex(s, in.receiver_id & 0xffffu, 4, false); s.put('\n');
    }
    if (m.timestamp == 0xFF004D4C4154ll) DUMP_LIT(s, "This is a synthetic MLAT message.\n");
    else if (m.timestamp == 0xFF004D4C4155ll) DUMP_LIT(s, "This is a synthetic UAT message.\n");
    else if (m.timestamp == 0xFF004D4C4160ll) DUMP_LIT(s, "This is a no_forward message.\n");
    else {                                                       // %27.2f of the correctly rounded timestamp / 12.0
        const double q = (double) m.timestamp / 12.0;
        DUMP_LIT(s, "receiverTime: ");
        if (q >= 0x1p53) dump_fixed(s, false, (uint64_t) q, 0u, 2, 27);       // an integer: ".00"
        else dump_f(s, q, 2, 27);
        DUMP_LIT(s, "us\n");
    }
    {                                                            // :1888-1893; epoch: %.3f of ms / 1000.0 is the quotient's own three decimals
        const uint64_t ms = (uint64_t) m.sysTimestamp, sec = ms / 1000ull;
        const uint32_t msec = (uint32_t) (ms - sec * 1000ull);
        DUMP_LIT(s, "utcTime: "); dump_hms(s, (uint32_t) (sec % 86400ull)); s.put('.'); dump_udec(s, msec, 3);
        DUMP_LIT(s, " epoch: "); dump_udec(s, sec); s.put('.'); dump_udec(s, msec, 3); s.put('\n');
    }
    switch (df) {                                                // :1899-1971
    case 0:
        DUMP_LIT(s, "DF:  0 addr:"); dump_addr9(s, f);
        DUMP_LIT(s, " VS:"); dump_udec(s, f.VS); DUMP_LIT(s, " CC:"); dump_udec(s, f.CC); DUMP_LIT(s, " SL:"); dump_udec(s, f.SL);
        DUMP_LIT(s, " RI:"); dump_udec(s, f.RI); DUMP_LIT(s, " AC:"); dump_udec(s, f.AC); s.put('\n');
        break;
    case 4: case 5: case 20: case 21:
        DUMP_LIT(s, "DF: "); dump_idec(s, df, 2); DUMP_LIT(s, " addr:"); dump_addr9(s, f);
        DUMP_LIT(s, " FS:"); dump_udec(s, f.FS); DUMP_LIT(s, " DR:"); dump_udec(s, f.DR); DUMP_LIT(s, " UM:"); dump_udec(s, f.UM);
        if (df & 1u) { DUMP_LIT(s, " ID:"); dump_udec(s, f.ID); } else { DUMP_LIT(s, " AC:"); dump_udec(s, f.AC); }
        if (df >= 20u) { DUMP_LIT(s, " MB:"); dump_bytes(s, m, 4, 7); }
        s.put('\n');
        break;
    case 11:
        DUMP_LIT(s, "DF: 11 AA:"); dump_hex(s, f.AA, 6, true); DUMP_LIT(s, " IID:"); dump_udec(s, f.IID); DUMP_LIT(s, " CA:"); dump_udec(s, f.CA); s.put('\n');
        break;
    case 16:
        DUMP_LIT(s, "DF: 16 addr:"); dump_addr9(s, f);
        DUMP_LIT(s, " VS:"); dump_udec(s, f.VS); DUMP_LIT(s, " SL:"); dump_udec(s, f.SL); DUMP_LIT(s, " RI:"); dump_udec(s, f.RI);
        DUMP_LIT(s, " AC:"); dump_udec(s, f.AC); DUMP_LIT(s, " MV:"); dump_bytes(s, m, 4, 7); s.put('\n');
        if (fl & MGPU_F_ACAS_RA_VALID) dump_acas(s, m, f);
        break;
    case 17: case 18:
        DUMP_LIT(s, "DF: "); dump_idec(s, df, 2); DUMP_LIT(s, " AA:"); dump_hex(s, f.AA, 6, true);
        if (df == 17u) { DUMP_LIT(s, " CA:"); dump_udec(s, f.CA); } else { DUMP_LIT(s, " CF:"); dump_udec(s, f.CF); }
        DUMP_LIT(s, " ME:"); dump_bytes(s, m, 4, 7); s.put('\n');
        break;
    case 24: case 25: case 26: case 27: case 28: case 29: case 30: case 31:
        DUMP_LIT(s, "DF: 24 addr:"); dump_addr9(s, f);
        DUMP_LIT(s, " KE:"); dump_udec(s, f.KE); DUMP_LIT(s, " ND:"); dump_udec(s, f.ND); DUMP_LIT(s, " MD:"); dump_bytes(s, m, 1, 10); s.put('\n');
        break;
    default: break;
    }
    s.put(' '); dump_str(s, dump_df_name(df));
    if (df == 17u || df == 18u) {                                // :1977-1988
        s.put(' '); dump_str(s, dump_es_name(f.metype, f.mesub));
        DUMP_LIT(s, " ("); dump_udec(s, f.metype);
        if (f.metype > 18u && !(f.metype >= 20u && f.metype <= 22u)) { s.put('/'); dump_udec(s, f.mesub); }
        s.put(')');
    }
    s.put('\n');
    if (df == 20u || df == 21u) { DUMP_LIT(s, "  Comm-B format: "); dump_str(s, dump_commb_name(f.commb_format)); s.put('\n'); }
    if (f.addr != kDumpHexUnknown) {
        if (f.addr & kDumpNonIcao) { DUMP_LIT(s, "  Other Address: "); dump_hex(s, f.addr & 0xffffffu, 6, true); }
        else { DUMP_LIT(s, "  ICAO Address:  "); dump_hex(s, f.addr, 6, true); }
        DUMP_LIT(s, " ("); dump_str(s, dump_addrtype_name(f.addrtype)); DUMP_LIT(s, ")\n");
    }
    if (f.airground) { DUMP_LIT(s, "  Air/Ground:    "); dump_str(s, dump_airground_name(f.airground)); s.put('\n'); }
    if (fl & MGPU_F_BARO_ALT_VALID) {
        DUMP_LIT(s, "  Baro altitude:           "); dump_idec(s, f.baro_alt, 8); s.put(' '); dump_str(s, dump_unit_name(f.baro_alt_unit)); s.put('\n');
    }
    if (fl & MGPU_F_GEOM_ALT_VALID) {
        DUMP_LIT(s, "  Geom altitude:           "); dump_idec(s, f.geom_alt, 8); s.put(' '); dump_str(s, dump_unit_name(f.geom_alt_unit)); s.put('\n');
    }
    if (fl & MGPU_F_GEOM_DELTA_VALID) { DUMP_LIT(s, "  Geom - baro:   "); dump_idec(s, f.geom_delta, 8); DUMP_LIT(s, " ft\n"); }
    if (fl & MGPU_F_HEADING_VALID) {                             // "  %-13s     %5.1f\n"
        const DumpStr t = dump_heading_name(f.heading_type);
        DUMP_LIT(s, "  "); dump_str(s, t); dump_pad(s, 13 - (int) t.n); DUMP_LIT(s, "     "); dump_f(s, f.heading, 1, 5); s.put('\n');
    }
    if (fl & MGPU_F_TRACK_RATE_VALID) {
        DUMP_LIT(s, "  Track rate:    "); dump_f(s, f.track_rate, 2, 6); DUMP_LIT(s, " deg/sec ");
        if (f.track_rate < 0) DUMP_LIT(s, "left"); else if (f.track_rate > 0) DUMP_LIT(s, "right");
        s.put('\n');
    }
    if (fl & MGPU_F_ROLL_VALID) {
        DUMP_LIT(s, "  Roll:          "); dump_f(s, f.roll, 1, 5); DUMP_LIT(s, " degrees ");
        if ((double) f.roll < -0.05) DUMP_LIT(s, "left"); else if ((double) f.roll > 0.05) DUMP_LIT(s, "right");
        s.put('\n');
    }
    if (fl & MGPU_F_GS_VALID) {
        DUMP_LIT(s, "  Groundspeed:   "); dump_f(s, f.gs_selected, 1, 5); DUMP_LIT(s, " kt");
        if (f.gs_v0 != f.gs_selected) { DUMP_LIT(s, " (v0: "); dump_f(s, f.gs_v0, 1); DUMP_LIT(s, " kt)"); }
        if (f.gs_v2 != f.gs_selected) { DUMP_LIT(s, " (v2: "); dump_f(s, f.gs_v2, 1); DUMP_LIT(s, " kt)"); }
        s.put('\n');
    }
    if (fl & MGPU_F_IAS_VALID) { DUMP_LIT(s, "  IAS:           "); dump_idec(s, f.ias, 3); DUMP_LIT(s, " kt\n"); }
    if (fl & MGPU_F_TAS_VALID) { DUMP_LIT(s, "  TAS:           "); dump_idec(s, f.tas, 3); DUMP_LIT(s, " kt\n"); }
    if (fl & MGPU_F_MACH_VALID) { DUMP_LIT(s, "  Mach number:   "); dump_f(s, f.mach, 3); s.put('\n'); }
    if (fl & MGPU_F_BARO_RATE_VALID) { DUMP_LIT(s, "  Baro rate:     "); dump_idec(s, f.baro_rate, 6); DUMP_LIT(s, " ft/min\n"); }
    if (fl & MGPU_F_GEOM_RATE_VALID) { DUMP_LIT(s, "  Geom rate:     "); dump_idec(s, f.geom_rate, 6); DUMP_LIT(s, " ft/min\n"); }
    if (fl & MGPU_F_SQUAWK_VALID) { DUMP_LIT(s, "  Squawk:        "); dump_udec(s, f.squawkDec, 4); s.put('\n'); }
    if (fl & MGPU_F_CALLSIGN_VALID) {
        DUMP_LIT(s, "  Ident:         ");
        bool open = true;
        for (int k = 0; k < 8; ++k) {
            const uint32_t ch = (uint8_t) f.callsign[k];
            open = open && ch != 0;
            if (open) s.put(ch);
        }
        s.put('\n');
    }
    if (fl & MGPU_F_CATEGORY_VALID) { DUMP_LIT(s, "  Category:      "); dump_hex(s, f.category, 2, true); s.put('\n'); }
    if (fl & MGPU_F_CPR_VALID) {                                 // :2089-2116
        DUMP_LIT(s, "  CPR type:      "); dump_str(s, dump_cpr_name(f.cpr_type));
        if (fl & MGPU_F_CPR_ODD) DUMP_LIT(s, "\n  CPR odd flag:  odd\n"); else DUMP_LIT(s, "\n  CPR odd flag:  even\n");
        if (dump_has_position(in)) {
            DUMP_LIT(s, "  CPR latitude:  "); dump_f(s, in.pos->lat, 6, 11); DUMP_LIT(s, " ("); dump_idec(s, f.cpr_lat, 5);
            DUMP_LIT(s, ")\n  CPR longitude: "); dump_f(s, in.pos->lon, 6, 11); DUMP_LIT(s, " ("); dump_idec(s, f.cpr_lon, 5);
            if (in.pos->method == MGPU_CPR_GLOBAL) DUMP_LIT(s, ")\n  CPR decoding:  global\n"); else DUMP_LIT(s, ")\n  CPR decoding:  local\n");
            DUMP_KV(s, "  NIC:           ", in.decoded_nic);
            // %.3f of rc / 1000.0 is the quotient's own three decimals; %.1f of the correctly rounded rc / 1852.0
            DUMP_LIT(s, "  Rc:            "); dump_udec(s, in.decoded_rc / 1000u); s.put('.'); dump_udec(s, in.decoded_rc % 1000u, 3);
            DUMP_LIT(s, " km / "); dump_f(s, (double) in.decoded_rc / 1852.0, 1); DUMP_LIT(s, " NM\n");
        } else {
            DUMP_LIT(s, "  CPR latitude:  ("); dump_udec(s, f.cpr_lat);
            DUMP_LIT(s, ")\n  CPR longitude: ("); dump_udec(s, f.cpr_lon);
            DUMP_LIT(s, ")\n  CPR decoding:  none\n");
        }
    }
    const uint32_t acc = f.acc_flags;
    if (acc & MGPU_ACC_NIC_A_VALID) DUMP_KV(s, "  NIC-A:         ", (acc & MGPU_ACC_NIC_A) ? 1u : 0u);
    if (acc & MGPU_ACC_NIC_B_VALID) DUMP_KV(s, "  NIC-B:         ", (acc & MGPU_ACC_NIC_B) ? 1u : 0u);
    if (acc & MGPU_ACC_NIC_C_VALID) DUMP_KV(s, "  NIC-C:         ", (acc & MGPU_ACC_NIC_C) ? 1u : 0u);
    if (acc & MGPU_ACC_NIC_BARO_VALID) DUMP_KV(s, "  NIC-baro:      ", (acc & MGPU_ACC_NIC_BARO) ? 1u : 0u);
    if (acc & MGPU_ACC_NAC_P_VALID) DUMP_KV(s, "  NACp:          ", f.nac_p);
    if (acc & MGPU_ACC_NAC_V_VALID) DUMP_KV(s, "  NACv:          ", f.nac_v);
    if (acc & MGPU_ACC_GVA_VALID) DUMP_KV(s, "  GVA:           ", f.gva);
    if (f.sil_type) {
        DUMP_LIT(s, "  SIL:           "); dump_udec(s, f.sil);
        if (f.sil == 1u) DUMP_LIT(s, " (p <= 0.1%, "); else if (f.sil == 2u) DUMP_LIT(s, " (p <= 0.001%, ");
        else if (f.sil == 3u) DUMP_LIT(s, " (p <= 0.00001%, "); else DUMP_LIT(s, " (p > 0.1%, ");
        dump_str(s, dump_sil_type_name(f.sil_type)); DUMP_LIT(s, ")\n");
    }
    if (acc & MGPU_ACC_SDA_VALID) DUMP_KV(s, "  SDA:           ", f.sda);
    const uint32_t op = f.op_flags;
    if (op & MGPU_OP_VALID) {                                    // :2174-2202
        DUMP_LIT(s, "  Aircraft Operational Status:\n");
        DUMP_KV(s, "    Version:            ", f.op_version & 7u);             // a three-bit member
        DUMP_LIT(s, "    Capability classes: ");
        if (op & MGPU_OP_CC_ACAS) DUMP_LIT(s, "ACAS ");
        if (op & MGPU_OP_CC_CDTI) DUMP_LIT(s, "CDTI ");
        if (op & MGPU_OP_CC_1090_IN) DUMP_LIT(s, "1090IN ");
        if (op & MGPU_OP_CC_ARV) DUMP_LIT(s, "ARV ");
        if (op & MGPU_OP_CC_TS) DUMP_LIT(s, "TS ");
        if (f.op_cc_tc & 3u) { DUMP_LIT(s, "TC="); dump_udec(s, f.op_cc_tc & 3u); s.put(' '); }    // a two-bit member
        if (op & MGPU_OP_CC_UAT_IN) DUMP_LIT(s, "UATIN ");
        if (op & MGPU_OP_CC_POA) DUMP_LIT(s, "POA ");
        if (op & MGPU_OP_CC_B2_LOW) DUMP_LIT(s, "B2-LOW ");
        if (op & MGPU_OP_CC_LW_VALID) { DUMP_LIT(s, "L/W="); dump_udec(s, f.op_cc_lw); s.put(' '); }
        if (f.op_cc_antenna_offset) { DUMP_LIT(s, "GPS-OFFSET="); dump_udec(s, f.op_cc_antenna_offset); s.put(' '); }
        DUMP_LIT(s, "\n    Operational modes:  ");
        if (op & MGPU_OP_OM_ACAS_RA) DUMP_LIT(s, "ACASRA ");
        if (op & MGPU_OP_OM_IDENT) DUMP_LIT(s, "IDENT ");
        if (op & MGPU_OP_OM_ATC) DUMP_LIT(s, "ATC ");
        if (op & MGPU_OP_OM_SAF) DUMP_LIT(s, "SAF ");
        s.put('\n');
        if (f.mesub == 1u) { DUMP_LIT(s, "    Track/heading:      "); dump_str(s, dump_heading_name(f.op_tah)); s.put('\n'); }
        DUMP_LIT(s, "    Heading ref dir:    "); dump_str(s, dump_heading_name(f.op_hrd)); s.put('\n');
    }
    const uint32_t nav = f.nav_flags;
    if (nav & MGPU_NAV_HEADING_VALID) { DUMP_LIT(s, "  Selected heading: "); dump_f(s, f.nav_heading, 1, 5); s.put('\n'); }
    if (nav & MGPU_NAV_FMS_ALT_VALID) { DUMP_LIT(s, "  FMS selected altitude:      "); dump_idec(s, f.nav_fms_altitude, 5); DUMP_LIT(s, " ft\n"); }
    if (nav & MGPU_NAV_MCP_ALT_VALID) { DUMP_LIT(s, "  MCP selected altitude:      "); dump_idec(s, f.nav_mcp_altitude, 5); DUMP_LIT(s, " ft\n"); }
    if (nav & MGPU_NAV_QNH_VALID) { DUMP_LIT(s, "  QNH:                     "); dump_f(s, f.nav_qnh, 1); DUMP_LIT(s, " millibars\n"); }
    if (f.nav_altitude_source) {
        DUMP_LIT(s, "  Target altitude source:  ");
        if (f.nav_altitude_source == 2u) DUMP_LIT(s, "aircraft altitude\n");
        else if (f.nav_altitude_source == 3u) DUMP_LIT(s, "MCP selected altitude\n");
        else if (f.nav_altitude_source == 4u) DUMP_LIT(s, "FMS selected altitude\n");
        else DUMP_LIT(s, "unknown\n");
    }
    if (nav & MGPU_NAV_MODES_VALID) {                            // nav_modes_to_string: the names with one space between them
        DUMP_LIT(s, "  Nav modes:               ");
        const uint32_t md = f.nav_modes & 63u;
        if (md & 1u) { DUMP_LIT(s, "autopilot"); if (md >> 1) s.put(' '); }
        if (md & 2u) { DUMP_LIT(s, "vnav"); if (md >> 2) s.put(' '); }
        if (md & 4u) { DUMP_LIT(s, "althold"); if (md >> 3) s.put(' '); }
        if (md & 8u) { DUMP_LIT(s, "approach"); if (md >> 4) s.put(' '); }
        if (md & 16u) { DUMP_LIT(s, "lnav"); if (md >> 5) s.put(' '); }
        if (md & 32u) DUMP_LIT(s, "tcas");
        s.put('\n');
    }
    if (fl & MGPU_F_EMERGENCY_VALID) { DUMP_LIT(s, "  Emergency/priority:      "); dump_str(s, dump_emergency_name(f.emergency)); s.put('\n'); }
    s.put('\n');
}

// The longest dump, line by line, within the domain dump_classify() admits (|float| < 2^31: "-2147483520.0"-like, 11 + 1 + dec):
//   frame       '@' + 16 digits + 28 + ";\n"                                                     47
//   hex         "hex: " 5 + 9 + " CRC: " 6 + 6 + " fixed bits: " 13 + 3 + " decode: ok\n" 12     54
//   RSSI        "RSSI: " 6 + 8 + " dBFS   " 8                                                    22
//   reduce      "reduce_forward: " 16 + 4 + 1                                                    21
//   score       "Score: " 7 + 6 + 1                                                              14
//   receiverId  12 + 18 + 1                                                                      31
//   time        "receiverTime: " 14 + 27 + "us\n" 3 (a sentence is shorter)                      44
//   utc         "utcTime: " 9 + 12 + " epoch: " 8 + 12 + 4 + 1                                   46
//   DF          DF 20/21: "DF: 20 addr:" 12 + 9 + " FS:" 4+3 + " DR:" 4+3 + " UM:" 4+3 + " ID:" 4+5 + " MB:" 4+14 + 1 = 77;
//               DF 16: 12 + 9 + 4 * (4 + 3) + 2 (AC: five digits) + 4 + 14 + 1 = 70, and the ACAS line: date 10 + 1, time 10,
//               ", " 2, addr 8, ",DF:," 5 + 2, ",bytes:," 8 + 14, the empty columns up to "ARA:," 49, 7 bits, RAT 7, MTE 7, RAC 10,
//               ", " 2, four "not ..." 36, ", " 2 = 180; the advisory ("RA multithreat:" 15 + 17 + 16 + 19 + 18 + 10 + 32 = 127, the
//               single-threat texts are shorter), "; TIDh: " 8 + 6, ",\n" 2 = 143.  Both DF lines are counted.         323 + 70
//   name        1 + 35 + 1 + 45 + " (255/255)" 10 + 1                                            93
//   comm-b      17 + 40 + 1                                                                      58
//   address     17 + 8 + 2 + 14 + 2                                                              43
//   air/ground  17 + 25 + 1                                                                      43
//   altitudes   2 * (27 + 11 + 1 + 23 + 1) = 126, delta 17 + 11 + 4 = 32                        158
//   heading     2 + 20 + 5 + 13 + 1                                                              41
//   track rate  17 + 14 + 9 + 5 + 1 = 46; roll 17 + 13 + 9 + 5 + 1 = 45                          91
//   gs          17 + 13 + 3 + 2 * (6 + 13 + 4) + 1                                               80
//   ias, tas    2 * (17 + 5 + 4)                                                                 52
//   mach        17 + 15 + 1                                                                      33
//   rates       2 * (17 + 11 + 8)                                                                72
//   squawk      17 + 5 + 1 = 23; ident 17 + 8 + 1 = 26; category 17 + 2 + 1 = 20                69
//   CPR         17 + 16 + 1 + 17 + 4 + 1 = 56; decoded: 2 * (17 + 11 + 2 + 10 + 2) = 84, 17 + 6 + 1 = 24, NIC 17 + 3 + 1 = 21,
//               Rc 17 + 7 + 4 + 6 + 9 + 4 = 47                                                  232
//   accuracy    7 * (17 + 3 + 1) = 147 + SDA 21; SIL 17 + 3 + 17 + 15 + 2 = 54                  222
//   opstatus    30 + 24 + 3 + 1 = 28 -> 30 + 28; classes 24 + 5+5+7+4+3+7+6+4+7+8+15 + 1 = 96; modes 24 + 7+6+4+4 + 1 = 46;
//               two heading lines 2 * (24 + 20 + 1) = 90                                        290
//   nav         20 + 13 + 1 = 34; 2 * (30 + 10 + 4) = 88; 27 + 13 + 11 = 51; 27 + 22 = 49; modes 27 + 42 + 1 = 70;
//               emergency 27 + 29 + 1 = 57                                                      349
//   the blank line                                                                                 1
constexpr int kDumpMax = MGPU_DUMP_MAX;
static_assert(kDumpMax == 47 + 54 + 22 + 21 + 14 + 31 + 44 + 46 + 323 + 70 + 93 + 58 + 43 + 43 + 158 + 41 + 91 + 80 + 52 + 33 + 72 + 69 + 232 + 222 + 290 +
              349 + 1, "dump bound");
