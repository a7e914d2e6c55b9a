// uat_format.h — one 978 MHz UAT downlink line of a dump978 feed to its DF18 extended squitters: readsb's --net-uat-in-port path
// (decodeUatMessage, net_io.c:4334-4372 -> uat2esnt_convert_message, uat2esnt/uat2esnt.c:823, uat2esnt/uat_decode.c), restated:
// ONE formatter, __host__ __device__ and templated on what receives the frames, for the size pass and the write pass of
// kernels/uat.inc and for the host (uat_host.cpp: mgpu_uat_format_host; tests/host_stub/uat_format_check.cpp runs it against the
// reference's bytes under ASan and UBSan).  The three cannot disagree about a frame count.
//
// uat_line(p, n, sigtab, emit) sees the n bytes of a line without its '\n' and calls emit.frame(sig, frame) for each squitter, in
// the reference's order (surface position even, odd; airborne position even, odd or altitude only; velocity; callsign or squawk).
//   process_line (uat2esnt.c:756-820): '-' downlink, '+' uplink (never any output), anything else nothing; hex pairs up to the first
//     ';' (a bad pair, a 433rd payload byte, or the end before a ';': nothing); then the walk over the fields (:784-800).
//   The signal byte (generate_esnt:684-691) of a field value in the SIMPLE FORM [+-]?[0-9]{1,3}(\.[0-9])? followed by ';' or the end
//     comes from a table of 19 999 bytes the host builds with sscanf and the reference's expression in its own libm
//     (uat_build_sig_table below).  A '-' line with an ss= / rssi= field in any other form the walk reaches, or longer than
//     kUatDevLineMax bytes, is UAT_DEFER for the device; the host settles it with sscanf and libm (uat_host_line).
//   Decode (uat_decode_adsb_mdb, uat_decode.c:445-484): only what reaches a frame.  atan2 and sqrt (:116-120) feed track and speed,
//     which only the surface frame reads — from the raw fields, for a target on the ground — so there is no libm here but fmod and floor.
//   A payload shorter than its type's decoders read is UAT_SHORT: the reference ignores the length (frame_to_esnt:716) and decodes
//     uninitialised stack; here such a line produces nothing.  Types 0, 4, 7-10: 17 bytes; 3: 27; 1, 2, 5, 6: 31; 11-31: 4.
//   CPR (:139-240) in double with the reference's operand order, contraction off: cprMod over fmod, cprNL's table, floor(x + 0.5).
// Not modelled: replayUatMsg (net_io.c:4341); the "ignore the first UAT message of an aircraft for 300 s" rule (:4357-4366), which
// belongs to the aircraft table; use_tisb = 0 (uat2esnt.c:699: the reference never clears it); uplink frames ('+': no output).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/modes_gpu.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UAT_HD __host__ __device__ inline
#else
#define UAT_HD inline
#endif
#if defined(__clang__)
#define UAT_FP_STRICT _Pragma("clang fp contract(off)")
#else
#define UAT_FP_STRICT
#endif

enum : int { UAT_NONE = 0, UAT_FRAMES = 1, UAT_DEFER = 2, UAT_SHORT = 3 };

constexpr uint32_t kUatDevLineMax = 256;         // a longer '-' line is the host's
constexpr uint32_t kUatMaxPayload = 432;         // UPLINK_FRAME_DATA_BYTES, uat.h:41
constexpr uint32_t kUatFrameText = 45;           // '<' + 12 + 2 + 28 + ";\n"
constexpr uint32_t kUatMaxFrames = 4;
// Frames per byte of text: the shortest line that gives a frame at all is '-', 4 pairs, ';', '\n' = 11 bytes (MDB types 11-31: the one
// altitude-only frame); more than one frame needs the state vector's 17 payload bytes: '-', 17 pairs, ';', '\n' = 37 bytes, for at most 4.
// 1 / 11 < 4 / 37, so whole lines in n bytes give at most 4 n / 37 frames; a run of lines that only START in n bytes — a tile's — adds
// its last line's 4.
constexpr uint32_t kUatBytesPerFourFrames = 37;
constexpr uint64_t uat_max_frames(uint64_t nbytes) { return nbytes * kUatMaxFrames / kUatBytesPerFourFrames + kUatMaxFrames; }
static_assert(11 * kUatMaxFrames >= kUatBytesPerFourFrames, "a one-frame line is no denser than a four-frame line");
// a deferred line is longer than kUatDevLineMax, or has 4 payload bytes and an ss= field: '-', 4 pairs, ';', "ss=", '\n' = 14 bytes at least
constexpr uint64_t uat_max_deferred(uint64_t nbytes) { return nbytes / 14 + 1; }
constexpr int kUatSigSpan = 9999;                // simple-form values are k / 10, |k| <= 9999: table index k + 9999
constexpr uint32_t kUatSigTable = 2 * kUatSigSpan + 1;
constexpr int64_t kUatTimestamp = 0xFF004D4C4155ll;   // MAGIC_UAT_TIMESTAMP, uat2esnt.c:660

// a 112-bit frame: DF | CF | AA, the ME field (56 bits), the parity
struct UatFrame {
    uint32_t hdr, crc;
    uint64_t me;
    UAT_HD uint32_t byte(int k) const {
        return k < 4 ? (hdr >> (24 - 8 * k)) & 0xffu : k < 11 ? (uint32_t) (me >> (48 - 8 * (k - 4))) & 0xffu : (crc >> (16 - 8 * (k - 11))) & 0xffu;
    }
};

// the first 32 payload bytes, big endian in four words (nothing indexed at run time but memory), and how many the line had
struct UatPayload {
    uint64_t w0, w1, w2, w3;
    uint32_t n;
    UAT_HD uint32_t b(int i) const {
        const uint64_t w = i < 8 ? w0 : i < 16 ? w1 : i < 24 ? w2 : w3;
        return (uint32_t) (w >> (56 - 8 * (i & 7))) & 0xffu;
    }
};

UAT_HD int uat_hexval(uint32_t c) {
    return c >= '0' && c <= '9' ? (int) c - '0' : c >= 'a' && c <= 'f' ? (int) c - 'a' + 10 : c >= 'A' && c <= 'F' ? (int) c - 'A' + 10 : -1;
}

// strlen within the line (net_io.c:4337)
UAT_HD uint32_t uat_content_len(const uint8_t *p, uint32_t n) {
    uint32_t len = 0;
    while (len < n && p[len]) ++len;
    return len;
}

// The hex pairs of a '-' line up to the first ';' (process_line's loop).  p[0..len): the content.  false: nothing comes of the line.
// *fields: the index behind the ';'.
UAT_HD bool uat_payload(const uint8_t *p, uint32_t len, UatPayload &f, uint32_t *fields) {
    f.w0 = f.w1 = f.w2 = f.w3 = 0;
    f.n = 0;
    for (uint32_t pos = 1; pos < len; pos += 2) {
        if (p[pos] == ';') { *fields = pos + 1; return true; }
        if (f.n >= kUatMaxPayload) return false;
        const int hi = uat_hexval(p[pos]), lo = pos + 1 < len ? uat_hexval(p[pos + 1]) : -1;      // (behind the content stands the NUL)
        if (hi < 0 || lo < 0) return false;
        if (f.n < 32) {
            const uint64_t v = (uint64_t) (uint32_t) (hi << 4 | lo) << (56 - 8 * (f.n & 7u));
            const uint32_t w = f.n >> 3;
            if (w == 0) f.w0 |= v; else if (w == 1) f.w1 |= v; else if (w == 2) f.w2 |= v; else f.w3 |= v;
        }
        ++f.n;
    }
    return false;
}

// payload bytes the decoders of an MDB type read (uat_decode.c:445-484)
UAT_HD uint32_t uat_bytes_needed(uint32_t type) {
    return type == 1 || type == 2 || type == 5 || type == 6 ? 31u : type == 3 ? 27u : type == 0 || type == 4 || (type >= 7 && type <= 10) ? 17u : 4u;
}

UAT_HD bool uat_starts(const uint8_t *p, uint32_t pos, uint32_t len, const char *lit, uint32_t k) {
    if (pos + k > len) return false;
    for (uint32_t j = 0; j < k; ++j)
        if (p[pos + j] != (uint8_t) lit[j]) return false;
    return true;
}

// The walk over the fields behind the ';' (uat2esnt.c:784-800) where every ss= / rssi= value it reaches is in the simple form.
// *k10: ten times the value that ended the walk (0: none did, or every value was zero).  false: a value in another form.
UAT_HD bool uat_signal_simple(const uint8_t *p, uint32_t pos, uint32_t len, int *k10) {
    int value = 0;
    while (pos < len) {
        const bool ss = uat_starts(p, pos, len, "ss=", 3), rssi = uat_starts(p, pos, len, "rssi=", 5);
        if (ss || rssi) {
            uint32_t q = pos + (ss ? 3u : 5u);
            bool neg = false;
            if (q < len && (p[q] == '+' || p[q] == '-')) { neg = p[q] == '-'; ++q; }
            int v = 0, digits = 0;
            while (q < len && p[q] >= '0' && p[q] <= '9' && digits < 4) { v = v * 10 + (p[q] - '0'); ++digits; ++q; }
            if (digits < 1 || digits > 3) return false;
            v *= 10;
            if (q < len && p[q] == '.') {
                if (q + 1 < len && p[q + 1] >= '0' && p[q + 1] <= '9') { v += p[q + 1] - '0'; q += 2; }
                else return false;
            }
            if (q < len && p[q] != ';') return false;
            value = neg ? -v : v;
        }
        while (pos < len && p[pos] != ';') ++pos;
        if (pos >= len || value != 0) break;
        ++pos;
    }
    *k10 = value;
    return true;
}

// ---- decode: what of struct uat_adsb_mdb reaches a frame ----

struct UatMdb {
    uint32_t aq, address;
    bool position_valid;
    uint32_t raw_lat, raw_lon;
    int altitude_type, altitude;                  // ALT_INVALID 0, ALT_BARO 1, ALT_GEO 2
    int sec_altitude_type, sec_altitude;
    uint32_t airground;                           // AG_SUBSONIC 0, AG_SUPERSONIC 1, AG_GROUND 2, AG_RESERVED 3
    bool ns_valid, ew_valid, speed_valid, track_is_track;
    int ns_vel, ew_vel, vert_rate_source, vert_rate;
    uint32_t speed, track;                        // the ground state's (uint16_t in the reference)
    int callsign_type;                            // CS_INVALID 0, CS_CALLSIGN 1, CS_SQUAWK 2
    uint32_t emitter_category;
    uint64_t callsign;                            // eight characters, the first in the top byte, trailing spaces already NUL
};

UAT_HD uint32_t uat_base40(uint32_t v) { return v < 10 ? '0' + v : v < 36 ? 'A' + (v - 10) : v < 38 ? ' ' : '.'; }

UAT_HD void uat_decode_sv(const UatPayload &f, UatMdb &m) {
    const uint32_t nic = f.b(11) & 15u;
    m.raw_lat = (f.b(4) << 15) | (f.b(5) << 7) | (f.b(6) >> 1);
    m.raw_lon = ((f.b(6) & 1u) << 23) | (f.b(7) << 15) | (f.b(8) << 7) | (f.b(9) >> 1);
    m.position_valid = nic != 0 || m.raw_lat != 0 || m.raw_lon != 0;
    const uint32_t raw_alt = (f.b(10) << 4) | ((f.b(11) & 0xf0u) >> 4);
    if (raw_alt != 0) {
        m.altitude_type = (f.b(9) & 1u) ? 2 : 1;
        m.altitude = ((int) raw_alt - 1) * 25 - 1000;
    }
    m.airground = (f.b(12) >> 6) & 3u;
    const int raw_a = (int) (((f.b(12) & 0x1fu) << 6) | ((f.b(13) & 0xfcu) >> 2));          // N/S velocity, or the ground speed
    const int raw_b = (int) (((f.b(13) & 3u) << 9) | (f.b(14) << 1) | ((f.b(15) & 0x80u) >> 7));   // E/W velocity, or track / heading
    if (m.airground <= 1) {
        if ((raw_a & 0x3ff) != 0) {
            m.ns_valid = true;
            m.ns_vel = (raw_a & 0x3ff) - 1;
            if (raw_a & 0x400) m.ns_vel = 0 - m.ns_vel;
            if (m.airground == 1) m.ns_vel *= 4;
        }
        if ((raw_b & 0x3ff) != 0) {
            m.ew_valid = true;
            m.ew_vel = (raw_b & 0x3ff) - 1;
            if (raw_b & 0x400) m.ew_vel = 0 - m.ew_vel;
            if (m.airground == 1) m.ew_vel *= 4;
        }
        const int raw_vvel = (int) (((f.b(15) & 0x7fu) << 4) | ((f.b(16) & 0xf0u) >> 4));
        if ((raw_vvel & 0x1ff) != 0) {
            m.vert_rate_source = (raw_vvel & 0x400) ? 1 : 2;
            m.vert_rate = ((raw_vvel & 0x1ff) - 1) * 64;
            if (raw_vvel & 0x200) m.vert_rate = 0 - m.vert_rate;
        }
    } else if (m.airground == 2) {
        if (raw_a != 0) {
            m.speed_valid = true;
            m.speed = (uint32_t) ((raw_a & 0x3ff) - 1) & 0xffffu;                            // (a uint16_t: raw 0x400 gives 65535)
        }
        m.track_is_track = ((raw_b & 0x600) >> 9) == 1;
        m.track = (uint32_t) ((raw_b & 0x1ff) * 360 / 512);
    }
}

UAT_HD void uat_decode_ms(const UatPayload &f, UatMdb &m) {
    uint32_t ch[8];
    uint32_t v = (f.b(17) << 8) | f.b(18);
    m.emitter_category = (v / 1600u) % 40u;
    ch[0] = uat_base40((v / 40u) % 40u); ch[1] = uat_base40(v % 40u);
    v = (f.b(19) << 8) | f.b(20);
    ch[2] = uat_base40((v / 1600u) % 40u); ch[3] = uat_base40((v / 40u) % 40u); ch[4] = uat_base40(v % 40u);
    v = (f.b(21) << 8) | f.b(22);
    ch[5] = uat_base40((v / 1600u) % 40u); ch[6] = uat_base40((v / 40u) % 40u); ch[7] = uat_base40(v % 40u);
    bool trailing = true;
    uint64_t cs = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 7; i >= 0; --i) {
        trailing = trailing && ch[i] == ' ';
        cs |= (uint64_t) (trailing ? 0u : ch[i]) << (56 - 8 * i);
    }
    m.callsign = cs;
    if (cs >> 56) m.callsign_type = (f.b(26) & 2u) ? 1 : 2;
}

UAT_HD void uat_decode_auxsv(const UatPayload &f, UatMdb &m) {
    const int raw_alt = (int) ((f.b(29) << 4) | ((f.b(30) & 0xf0u) >> 4));
    if (raw_alt != 0) {
        m.sec_altitude = (raw_alt - 1) * 25 - 1000;
        m.sec_altitude_type = (f.b(9) & 1u) ? 1 : 2;
    }
}

UAT_HD void uat_decode(const UatPayload &f, UatMdb &m) {
    m = UatMdb{};
    const uint32_t type = (f.b(0) >> 3) & 0x1fu;
    m.aq = f.b(0) & 7u;
    m.address = (f.b(1) << 16) | (f.b(2) << 8) | f.b(3);
    if (type <= 10) uat_decode_sv(f, m);
    if (type == 1 || type == 3) uat_decode_ms(f, m);
    if (type == 1 || type == 2 || type == 5 || type == 6) uat_decode_auxsv(f, m);
}

// ---- the encoders of uat2esnt.c:70-240 ----

UAT_HD uint32_t uat_encode_altitude(int ft) {
    int i = (ft + 1000) / 25;
    if (i < 0) i = 0;
    if (i > 0x7FF) i = 0x7FF;
    return (uint32_t) ((i & 0x000F) | 0x0010 | ((i & 0x07F0) << 1));
}
UAT_HD uint32_t uat_encode_ground_speed(int kt) {
    if (kt > 175) return 124;
    if (kt > 100) return (uint32_t) ((kt - 100) / 5 + 108);
    if (kt > 70) return (uint32_t) ((kt - 70) / 2 + 93);
    if (kt > 15) return (uint32_t) ((kt - 15) + 38);
    if (kt > 2) return (uint32_t) ((kt - 2) * 2 + 11);
    if (kt == 2) return 12;
    if (kt == 1) return 8;
    return 1;
}
UAT_HD uint32_t uat_encode_air_speed(int kt, bool supersonic) {
    uint32_t sign = 0;
    if (kt < 0) { sign = 0x0400; kt = -kt; }
    if (supersonic) kt = kt / 4;
    ++kt;
    if (kt > 1023) kt = 1023;
    return (uint32_t) kt | sign;
}
UAT_HD uint32_t uat_encode_vert_rate(int rate) {
    uint32_t sign = 0;
    if (rate < 0) { sign = 0x200; rate = -rate; }
    rate = (rate / 64) + 1;
    if (rate > 511) rate = 511;
    return (uint32_t) rate | sign;
}

UAT_HD double uat_cpr_mod(double a, double b) {
    double res = fmod(a, b);
    if (res < 0) res += b;
    return res;
}
UAT_HD int uat_cpr_nl(double lat) {
    if (lat < 0) lat = -lat;
    const double t[58] = {10.47047130, 14.82817437, 18.18626357, 21.02939493, 23.54504487, 25.82924707, 27.93898710, 29.91135686, 31.77209708, 33.53993436,
                          35.22899598, 36.85025108, 38.41241892, 39.92256684, 41.38651832, 42.80914012, 44.19454951, 45.54626723, 46.86733252, 48.16039128,
                          49.42776439, 50.67150166, 51.89342469, 53.09516153, 54.27817472, 55.44378444, 56.59318756, 57.72747354, 58.84763776, 59.95459277,
                          61.04917774, 62.13216659, 63.20427479, 64.26616523, 65.31845310, 66.36171008, 67.39646774, 68.42322022, 69.44242631, 70.45451075,
                          71.45986473, 72.45884545, 73.45177442, 74.43893416, 75.42056257, 76.39684391, 77.36789461, 78.33374083, 79.29428225, 80.24923213,
                          81.19801349, 82.13956981, 83.07199445, 83.99173563, 84.89166191, 85.75541621, 86.53536998, 87.00000000};
    int nl = 59;
    for (int k = 0; k < 58; ++k)
        if (!(lat < t[k])) nl = 58 - k;              // the first threshold lat is below decides: 59 - (thresholds at or below lat)
    return nl;
}
// encode_cpr_lat / encode_cpr_lon: *yz, *xz before the 17-bit mask
UAT_HD void uat_encode_cpr(double lat, double lon, bool odd, bool surface, int *yz, int *xz) {
    UAT_FP_STRICT
    const int NbPow = surface ? 1 << 19 : 1 << 17;
    const double Dlat = 360.0 / (odd ? 59 : 60);
    const int YZ = (int) floor(NbPow * uat_cpr_mod(lat, Dlat) / Dlat + 0.5);
    const double Rlat = Dlat * (1.0 * YZ / NbPow + floor(lat / Dlat));
    int nl = uat_cpr_nl(Rlat) - (odd ? 1 : 0);
    if (nl < 1) nl = 1;
    const double Dlon = 360.0 / nl;
    const int XZ = (int) floor(NbPow * uat_cpr_mod(lon, Dlon) / Dlon + 0.5);
    *yz = YZ;
    *xz = XZ;
}

// checksum (uat2esnt.c:628-639) over the first 11 bytes, bit by bit: the table's polynomial division
UAT_HD uint32_t uat_crc(uint32_t hdr, uint64_t me) {
    uint32_t rem = 0;
    for (int k = 31; k >= 0; --k) {
        const uint32_t top = ((rem >> 23) ^ (hdr >> k)) & 1u;
        rem = (rem << 1) & 0xffffffu;
        if (top) rem ^= 0xfff409u;
    }
    for (int k = 55; k >= 0; --k) {
        const uint32_t top = ((rem >> 23) ^ (uint32_t) (me >> k)) & 1u;
        rem = (rem << 1) & 0xffffffu;
        if (top) rem ^= 0xfff409u;
    }
    return rem;
}

// setbits on the ME field (bits 1..56): a field of a frame that starts as zeros
UAT_HD uint64_t uat_me(int first, int last, uint32_t value) {
    return ((uint64_t) value & ((1ull << (last - first + 1)) - 1ull)) << (56 - last);
}

UAT_HD uint32_t uat_char_to_ais(uint32_t ch) {
    // "@ABC...Z[\]^_ !"#$%&'()*+,-./0123456789:;<=>?": 0x40-0x5f -> 0-31, 0x20-0x3f -> 32-63, NUL and everything else -> 32
    return ch >= 0x40 && ch <= 0x5f ? ch - 0x40 : ch >= 0x20 && ch <= 0x3f ? ch : 32u;
}

// strtoul(s, NULL, 16) of the callsign's characters (NUL ends them): leading spaces, an optional 0x / 0X (only before a hex digit),
// hex digits, stopping at the first other character.  (strtoul's sign cannot occur: the base-40 alphabet has none.)
UAT_HD uint32_t uat_strtoul16(uint64_t cs) {
    int i = 0;
    auto at = [&](int k) -> uint32_t { return k < 8 ? (uint32_t) (cs >> (56 - 8 * k)) & 0xffu : 0u; };
    while (at(i) == ' ') ++i;
    if (at(i) == '0' && (at(i + 1) == 'X' || at(i + 1) == 'x') && uat_hexval(at(i + 2)) >= 0) i += 2;
    uint32_t v = 0;
    for (; uat_hexval(at(i)) >= 0; ++i) v = (v << 4) | (uint32_t) uat_hexval(at(i));
    return v;
}

UAT_HD uint32_t uat_encode_squawk(uint32_t squawk) {
    uint32_t e = 0;
    if (squawk & 0x1000) e |= 0x0800;
    if (squawk & 0x2000) e |= 0x0200;
    if (squawk & 0x4000) e |= 0x0080;
    if (squawk & 0x0100) e |= 0x0020;
    if (squawk & 0x0200) e |= 0x0008;
    if (squawk & 0x0400) e |= 0x0002;
    if (squawk & 0x0010) e |= 0x1000;
    if (squawk & 0x0020) e |= 0x0400;
    if (squawk & 0x0040) e |= 0x0100;
    if (squawk & 0x0001) e |= 0x0010;
    if (squawk & 0x0002) e |= 0x0004;
    if (squawk & 0x0004) e |= 0x0001;
    return e;
}

// ---- generate_esnt (uat2esnt.c:679-697) ----

template <class E>
UAT_HD void uat_emit(E &e, uint32_t sig, uint32_t hdr, uint64_t me) {
    UatFrame fr;
    fr.hdr = hdr;
    fr.me = me;
    fr.crc = uat_crc(hdr, me);
    e.frame(sig, fr);
}

template <class E>
UAT_HD void uat_generate(const UatMdb &m, uint32_t sig, E &e) {
    if (!m.address) return;
    const uint32_t cf = m.aq == 0 ? 6u : (m.aq == 2 || m.aq == 3) ? 2u : 1u;                     // encode_cf
    const uint32_t imf = (m.aq == 0 || m.aq == 2) ? 0u : 1u;                                     // encode_imf
    const uint32_t hdr = (18u << 27) | (cf << 24) | (m.address & 0xffffffu);
    const bool air = m.airground <= 1;
    double lat = 0, lon = 0;
    if (m.position_valid || m.airground == 2) {                                                  // (uat_decode.c:71-76; an invalid position is 0, 0)
        UAT_FP_STRICT
        if (m.position_valid) {
            lat = m.raw_lat * 360.0 / 16777216.0;
            if (lat > 90) lat -= 180;
            lon = m.raw_lon * 360.0 / 16777216.0;
            if (lon > 180) lon -= 360;
        }
    }
    if (m.airground == 2) {                                                                      // maybe_send_surface_position
        uint64_t me = uat_me(1, 5, 8);
        if (m.speed_valid) me |= uat_me(6, 12, uat_encode_ground_speed((int) m.speed));
        if (m.track_is_track) me |= uat_me(13, 13, 1) | uat_me(14, 20, m.track * 128u / 360u);
        me |= uat_me(21, 21, imf);
        for (int odd = 0; odd < 2; ++odd) {
            int yz, xz;
            uat_encode_cpr(lat, lon, odd != 0, true, &yz, &xz);
            uat_emit(e, sig, hdr, me | uat_me(22, 22, (uint32_t) odd) | uat_me(23, 39, (uint32_t) yz) | uat_me(40, 56, (uint32_t) xz));
        }
    }
    if (air && !m.position_valid) {                                                              // send_altitude_only
        const uint32_t raw_alt = m.altitude_type == 1 ? uat_encode_altitude(m.altitude) : m.sec_altitude_type == 1 ? uat_encode_altitude(m.sec_altitude) : 0u;
        uat_emit(e, sig, hdr, uat_me(8, 8, imf) | uat_me(9, 20, raw_alt));
    } else if (air) {                                                                            // maybe_send_air_position
        const uint32_t raw_alt = m.altitude_type ? uat_encode_altitude(m.altitude) : 0u;
        const uint64_t me = uat_me(1, 5, m.altitude_type == 2 ? 22u : 18u) | uat_me(8, 8, imf) | uat_me(9, 20, raw_alt);
        for (int odd = 0; odd < 2; ++odd) {
            int yz, xz;
            uat_encode_cpr(lat, lon, odd != 0, false, &yz, &xz);
            uat_emit(e, sig, hdr, me | uat_me(22, 22, (uint32_t) odd) | uat_me(23, 39, (uint32_t) yz) | uat_me(40, 56, (uint32_t) xz));
        }
    }
    if (air && (m.ew_valid || m.ns_valid || m.vert_rate_source != 0)) {                          // maybe_send_air_velocity
        const bool supersonic = m.airground == 1;
        uint64_t me = uat_me(1, 5, 19) | uat_me(6, 8, supersonic ? 2u : 1u) | uat_me(9, 9, imf);
        if (m.ew_valid) me |= uat_me(14, 24, uat_encode_air_speed(m.ew_vel, supersonic));
        if (m.ns_valid) me |= uat_me(25, 35, uat_encode_air_speed(m.ns_vel, supersonic));
        if (m.vert_rate_source) me |= uat_me(36, 36, m.vert_rate_source == 2 ? 1u : 0u) | uat_me(37, 46, uat_encode_vert_rate(m.vert_rate));
        if (m.altitude_type != 0 && m.sec_altitude_type != 0) {
            int delta;
            uint32_t sign;
            if (m.altitude < m.sec_altitude) { delta = m.sec_altitude - m.altitude; sign = m.altitude_type == 1 ? 0u : 1u; }
            else { delta = m.altitude - m.sec_altitude; sign = m.altitude_type == 1 ? 1u : 0u; }
            delta = delta / 25 + 1;
            if (delta >= 127) delta = 127;
            me |= uat_me(49, 49, sign) | uat_me(50, 56, (uint32_t) delta);
        }
        uat_emit(e, sig, hdr, me);
    }
    if (m.callsign_type == 1 && !imf) {                                                          // maybe_send_callsign
        const uint32_t ec = m.emitter_category;
        uint64_t me = ec <= 7 ? uat_me(1, 5, 4) : ec <= 15 ? uat_me(1, 5, 3) : ec <= 23 ? uat_me(1, 5, 2) : ec <= 31 ? uat_me(1, 5, 1) : uat_me(1, 5, 4);
        if (ec <= 31) me |= uat_me(6, 8, ec & 7u);
        for (int k = 0; k < 8; ++k) me |= uat_me(9 + 6 * k, 14 + 6 * k, uat_char_to_ais((uint32_t) (m.callsign >> (56 - 8 * k)) & 0xffu));
        uat_emit(e, sig, hdr, me);
    } else if (m.callsign_type == 2) {
        // mapSquawkToEmergency: strcmp with "7500", "7600", "7700" — four characters and the NUL
        const uint64_t cs = m.callsign;
        const uint32_t emergency = cs == 0x3735303000000000ull ? 5u : cs == 0x3736303000000000ull ? 4u : cs == 0x3737303000000000ull ? 1u : 0u;
        uat_emit(e, sig, hdr, uat_me(1, 5, 28) | uat_me(6, 8, 1) | uat_me(9, 11, emergency) | uat_me(12, 24, uat_encode_squawk(uat_strtoul16(cs))) | uat_me(56, 56, imf));
    }
}

// One line.  p[0..n): its bytes without the '\n'.  sigtab: the table of uat_build_sig_table.  sig_override: kUatNoOverride, or — the
// host settling a line — the signal byte it computed itself in bits 0-7 with bit 30 set: then nothing is deferred.
constexpr int32_t kUatNoOverride = INT32_MIN;
template <class E>
UAT_HD int uat_line(const uint8_t *p, uint32_t n, const uint8_t *sigtab, int32_t sig_override, E &e) {
    if (n == 0 || p[0] != '-') return UAT_NONE;                                                   // ('+' and everything else: nothing)
    const bool settle = sig_override != kUatNoOverride;
    if (n > kUatDevLineMax && !settle) return UAT_DEFER;
    const uint32_t len = uat_content_len(p, n);
    UatPayload f;
    uint32_t fields = 0;
    if (!uat_payload(p, len, f, &fields)) return UAT_NONE;
    if (f.n < 4 || f.n < uat_bytes_needed((f.b(0) >> 3) & 0x1fu)) return UAT_SHORT;
    uint32_t sig;
    if (settle) sig = (uint32_t) sig_override & 0xffu;
    else {
        int k10 = 0;
        if (!uat_signal_simple(p, fields, len, &k10)) return UAT_DEFER;
        sig = sigtab[k10 + kUatSigSpan];
    }
    UatMdb m;
    uat_decode(f, m);
    uat_generate(m, sig, e);
    return UAT_FRAMES;
}

struct UatCountEmit {
    uint32_t n;
    UAT_HD void frame(uint32_t, const UatFrame &) { ++n; }
};

// "<FF004D4C4155" + the signal byte + the frame + ";\n" (checksum_and_print, uat2esnt.c:660-674) into a sink with put(c)
template <class S>
UAT_HD void uat_put_hex2(S &s, uint32_t b) {
    const uint32_t h = b >> 4, l = b & 15u;
    s.put(h < 10u ? '0' + h : 'A' - 10u + h);
    s.put(l < 10u ? '0' + l : 'A' - 10u + l);
}
template <class S>
UAT_HD void uat_put_frame(S &s, uint32_t sig, const UatFrame &fr) {
    s.put('<');
    uat_put_hex2(s, 0xFF); uat_put_hex2(s, 0x00); uat_put_hex2(s, 0x4D); uat_put_hex2(s, 0x4C); uat_put_hex2(s, 0x41); uat_put_hex2(s, 0x55);
    uat_put_hex2(s, sig);
    for (int k = 0; k < 14; ++k) uat_put_hex2(s, fr.byte(k));
    s.put(';');
    s.put('\n');
}

// the record decodeHexMessage + decodeModesMessage leave for a frame (modes_gpu.h)
UAT_HD void uat_fill_msg(mgpu_msg &r, uint32_t sig, const UatFrame &fr, int64_t now_ms) {
    r.timestamp = kUatTimestamp;
    r.sysTimestamp = now_ms;
    r.sig_sumsq = (uint64_t) (257u * sig) * (257u * sig);
    r.sig_len = 1;
    r.score = 0;
    r.phase = 0;
    r.correctedbits = 0;
    r.msgtype = 18;
    r.msgbits = 112;
    r.addr = fr.hdr & 0xffffffu;
    for (int k = 0; k < 14; ++k) r.msg[k] = r.raw[k] = (uint8_t) fr.byte(k);
}

// ---- host only ----
namespace mgpu { const uint8_t *uat_sig_table(); }    // kUatSigTable bytes, uat_build_sig_table's, built once (uat_host.cpp)
#include <cstdio>
#include <cstring>
#include <string>

// generate_esnt:684-691 on the host, in its libm
inline uint32_t uat_sig_of(float ss) {
    const double ss_W = pow(10.0, ss / 10.0);
    const double r = round(sqrt(ss_W) * 255.0);
    // (for ss = inf or nan the reference's conversion is undefined; x86-64's cvttsd2si gives it INT_MIN, stated here)
    int sig = r >= -2147483648.0 && r < 2147483648.0 ? (int) r : INT32_MIN;
    if (ss_W > 0 && sig < 1) sig = 1;
    if (sig > 255) sig = 255;
    return (uint32_t) sig & 0xffu;
}

// the table of the simple form: for every text "[-]N.D" the float sscanf reads and the reference's expression
inline void uat_build_sig_table(uint8_t *t) {
    for (int k = -kUatSigSpan; k <= kUatSigSpan; ++k) {
        char text[16];
        const int a = k < 0 ? -k : k;
        snprintf(text, sizeof text, "ss=%s%d.%d", k < 0 ? "-" : "", a / 10, a % 10);
        float ss = 0;
        sscanf(text, "ss=%f;", &ss);
        t[k + kUatSigSpan] = (uint8_t) uat_sig_of(ss);
    }
}

// The reference's walk over the fields (uat2esnt.c:784-800) with its own sscanf, on the NUL-terminated content behind the ';'.
inline float uat_signal_host(const char *p) {
    int done = 0;
    float signal_strength = 0;
    while (*p && !done) {
        if (!strncmp(p, "ss=", 3)) sscanf(p, "ss=%f;", &signal_strength);
        if (!strncmp(p, "rssi=", 5)) sscanf(p, "rssi=%f;", &signal_strength);
        while (*p && *p != ';') p++;
        if (!*p || signal_strength != 0) done = 1;
        else p++;
    }
    return signal_strength;
}

// One line on the host, nothing deferred: a line the device's formatter defers is settled with sscanf and libm.
template <class E>
inline int uat_host_line(const uint8_t *p, uint64_t n, const uint8_t *sigtab, E &e) {
    if (n <= kUatDevLineMax) {
        const int cls = uat_line(p, (uint32_t) n, sigtab, kUatNoOverride, e);
        if (cls != UAT_DEFER) return cls;
    }
    if (n == 0 || p[0] != '-') return UAT_NONE;
    if (n > 0x7fffffffu) return UAT_NONE;
    const std::string s((const char *) p, (size_t) n);               // NUL-terminated, as the reference's buffer
    const uint32_t len = (uint32_t) strlen(s.c_str());
    UatPayload f;
    uint32_t fields = 0;
    if (!uat_payload((const uint8_t *) s.c_str(), len, f, &fields)) return UAT_NONE;
    const uint32_t sig = uat_sig_of(uat_signal_host(s.c_str() + fields));
    return uat_line((const uint8_t *) s.c_str(), len, sigtab, (int32_t) (sig | (1u << 30)), e);
}
