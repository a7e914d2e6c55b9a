// asterix_in_format.h — one ASTERIX record of a received stream to the aircraft record readsb's ASTERIX input leaves
// (decodeAsterixMessage, net_io.c:1922-2407, with readFspec :1867, readAsterixTime :1884, readAsterixHighPrecisionTime :1899, behind
// readAsterix, :4643-4659), restated: ONE parser, __host__ __device__, for the passes of kernels/asterix_in.inc and for the host
// (asterix_in_host.cpp: mgpu_asterix_parse_host; tests/host_stub/asterix_in_format_check.cpp runs it against the reference's records
// under ASan and UBSan).  The rules, their line numbers and the deviations are in include/modes_gpu.h.
//   ast_in_frame(s, at, len)                 the framing rule at one position: a frame of len bytes, or the stop it is
//   ast_in_record(s, at, source, now_ms, r)  the record of the frame at `at`, or why it has none
// Every operation is exact and the same on both sides: integers, products of small integers with constants in double (one IEEE
// multiplication each, no contraction), conversions.  The stream is read a byte at a time through AstBytes, which gives 0 at or
// beyond its end; nothing is indexed at run time but the stream.
#pragma once
#include <cstdint>

#include "../../include/modes_gpu.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AST_IN_HD __host__ __device__ inline
#else
#define AST_IN_HD inline
#endif

enum : int { AST_IN_FRAME = 0, AST_IN_END = 1, AST_IN_ZERO_LEN = 2 };                       // ast_in_frame
enum : int { AST_IN_OTHER = 0, AST_IN_RECORD = 1, AST_IN_CLOSED = 2, AST_IN_UNDEFINED = 3 };   // ast_in_record

constexpr uint32_t kAstInMaxLen = 65535;         // a length is a uint16_t
constexpr uint32_t kAstInMaxChain = 191;         // extension bytes readFspec's allocation holds (:1868: 24 pointers = 192 bytes, byte 0 the first)
constexpr uint32_t kAstInLook = 1024;            // no frame is decided by more bytes than this behind its start
constexpr uint32_t kAstInMaxSource = 11;         // SOURCE_PRIO, readsb.h:159-173
constexpr int64_t kAstInNowEnd = 253402300800000ll;   // now_ms below this, as the ASTERIX writer's
// a frame that gives a record starts with 21 and its length bytes: one of len 1 or 2 is followed by a frame of category 0 or 2, so
// two such frames start 3 bytes apart at the least, however much their items overlap
constexpr uint64_t ast_in_max_recs(uint64_t nbytes) { return nbytes / 3 + 1; }

AST_IN_HD bool ast_in_source_ok(uint32_t source) { return source <= kAstInMaxSource; }
AST_IN_HD bool ast_in_now_ok(int64_t now_ms) { return now_ms >= 0 && now_ms < kAstInNowEnd; }

struct AstBytes {
    const uint8_t *d;
    uint64_t n;
    AST_IN_HD uint32_t operator[](uint64_t p) const { return p < n ? (uint32_t) d[p] : 0u; }
};

// readAsterix's length (:4647): both bytes through a signed char
AST_IN_HD uint32_t ast_in_len(uint32_t hi, uint32_t lo) {
    const int h = hi >= 128u ? (int) hi - 256 : (int) hi, l = lo >= 128u ? (int) lo - 256 : (int) lo;
    return (uint32_t) (h * 256 + l) & 0xffffu;
}

AST_IN_HD int ast_in_frame(const AstBytes &s, uint64_t at, uint32_t &len) {
    len = 0;
    if (at > s.n || s.n - at < 3) return AST_IN_END;
    len = ast_in_len(s.d[at + 1], s.d[at + 2]);
    if (len == 0) return AST_IN_ZERO_LEN;
    if (len > s.n - at) return AST_IN_END;
    return AST_IN_FRAME;
}

// readFspec (:1867-1879): byte k of the chain in bits 8k of `bits` (k < 8; more are never used); false: more than kAstInMaxChain
// extension bytes
AST_IN_HD bool ast_in_fspec(const AstBytes &s, uint64_t &p, uint64_t &bits) {
    uint32_t c = s[p++];
    bits = c;
    for (uint32_t i = 1; c & 1u; ++i) {
        if (i > kAstInMaxChain) return false;
        c = s[p++];
        if (i < 8) bits |= (uint64_t) c << (8 * i);
    }
    return true;
}

// readAsterixTime (:1884-1894); (int)(raw / .128) == raw * 125 / 16 for every raw < 2^24 (asterix_in_format_check.cpp tries them all)
AST_IN_HD uint64_t ast_in_time(const AstBytes &s, uint64_t &p, int64_t now_ms) {
    const uint32_t raw = s[p] << 16 | s[p + 1] << 8 | s[p + 2];
    p += 3;
    const int64_t mssm = (int64_t) ((uint64_t) raw * 125u / 16u);
    const int64_t midnight = now_ms / 86400000 * 86400000;
    const int64_t diff = midnight + mssm - now_ms;                    // (fits the reference's int: now_ms >= 0)
    if ((diff < 0 ? -diff : diff) > 43200000) return (uint64_t) (midnight - 86400000 + mssm);
    return (uint64_t) (midnight + mssm);
}

// readAsterixHighPrecisionTime (:1899-1915) as the reference's x86-64 build computes it (include/modes_gpu.h)
AST_IN_HD uint64_t ast_in_hp_time(const AstBytes &s, uint64_t &p, uint64_t ts) {
    const uint32_t b0 = s[p], fsi = b0 >> 6;
    const uint32_t raw = (b0 & 0x3fu) << 24 | s[p + 1] << 16 | s[p + 2] << 8 | s[p + 3];
    p += 4;
    const double offset = (double) raw * (1.0 / 134217728.0);         // 2^-27: exact
    const uint32_t prod = (uint32_t) (ts / 1000u) * 1000u;            // 32 bits, wrapping
    uint64_t whole = prod >= 0x80000000u ? (uint64_t) prod | 0xffffffff00000000ull : (uint64_t) prod;   // sign-extended
    if (fsi == 1) whole += 1;
    if (fsi == 2) whole -= 1;
    const double sum = (double) whole + offset;
    if (sum >= 18446744073709551616.0) return 0;
    return (uint64_t) sum;
}

AST_IN_HD uint32_t ast_in_ais(uint32_t code) { return code < 32u ? code + 64u : code; }      // ais_charset.c:26

// I021/020 (:2304-2373)
AST_IN_HD uint32_t ast_in_category(uint32_t ecat) {
    uint32_t tc = 0, ca = 0;
    if (ecat == 0) { tc = 0x0e; ca = 0; }
    else if (ecat <= 6) { tc = 4; ca = ecat; }
    else if (ecat == 10) { tc = 4; ca = 7; }
    else if (ecat == 11) { tc = 3; ca = 1; }
    else if (ecat == 12) { tc = 3; ca = 2; }
    else if (ecat == 13) { tc = 3; ca = 6; }
    else if (ecat == 14) { tc = 3; ca = 7; }
    else if (ecat == 15) { tc = 3; ca = 4; }
    else if (ecat == 16) { tc = 3; ca = 3; }
    else if (ecat == 20) { tc = 2; ca = 1; }
    else if (ecat == 21) { tc = 2; ca = 3; }
    else if (ecat == 22) { tc = 2; ca = 4; }
    else if (ecat == 23) { tc = 2; ca = 5; }
    else if (ecat == 24) { tc = 2; ca = 6; }
    return ((0x0eu - tc) << 4) | ca;
}

AST_IN_HD int32_t ast_in_s16(uint32_t v) { return (v & 0x8000u) ? (int32_t) (v & 0xffffu) - 65536 : (int32_t) (v & 0xffffu); }
AST_IN_HD int32_t ast_in_s32(uint32_t v) { return v >= 0x80000000u ? (int32_t) (v - 0x80000000u) - 2147483647 - 1 : (int32_t) v; }

// readsb.h's values
enum : uint32_t { AST_AG_GROUND = 1, AST_AG_AIRBORNE = 2, AST_UNIT_FEET = 0, AST_HEADING_GROUND_TRACK = 1, AST_HEADING_MAGNETIC = 3, AST_SIL_UNKNOWN = 1,
                  AST_SIL_PER_SAMPLE = 2, AST_SIL_PER_HOUR = 3, AST_ADDR_ADSB_ICAO = 0, AST_ADDR_ADSR_ICAO = 2, AST_ADDR_TISB_ICAO = 3, AST_ADDR_ADSB_OTHER = 8,
                  AST_ADDR_ADSR_OTHER = 9, AST_ADDR_TISB_OTHER = 11, AST_ADDR_UNKNOWN = 15 };

// The frame at `at` (its three header bytes lie inside the stream).  AST_IN_RECORD: r is the record.
AST_IN_HD int ast_in_record(const AstBytes &s, uint64_t at, uint32_t source, int64_t now_ms, mgpu_asterix_rec &r) {
    if (s[at] != 21u) return AST_IN_OTHER;
    uint64_t p = at + 3, fspec;
    if (!ast_in_fspec(s, p, fspec)) return AST_IN_UNDEFINED;
    const uint32_t f0 = (uint32_t) fspec & 0xffu, f1 = (uint32_t) (fspec >> 8) & 0xffu, f2 = (uint32_t) (fspec >> 16) & 0xffu, f3 = (uint32_t) (fspec >> 24) & 0xffu,
                   f4 = (uint32_t) (fspec >> 32) & 0xffu;
    if (!(f1 & 0x10u)) return AST_IN_CLOSED;

    int64_t sys = -1;
    double lat = 0, lon = 0, mach = 0;
    uint32_t flags = 0, aflags = 0, addrtype_out = 0, airground = 0, ias = 0, tas = 0, squawk = 0, category = 0, mcp = 0, fms = 0, emergency = 0, nav_modes = 0;
    int32_t baro_alt = 0, geom_alt = 0, baro_rate = 0, geom_rate = 0;
    float gs = 0, heading = 0, roll = 0;
    uint32_t nac_v = 0, nac_p_out = 0, sil_out = 0, sil_type = 0, gva_out = 0, sda_out = 0, nic_baro_out = 0, op_version = 0, heading_type = 0;
    uint64_t callsign = 0;

    if (f0 & 0x80u) p += 2;                                           // I021/010
    uint32_t addrtype = 3;
    if (f0 & 0x40u) {                                                 // I021/040
        uint64_t trd;
        if (!ast_in_fspec(s, p, trd)) return AST_IN_UNDEFINED;
        addrtype = ((uint32_t) trd & 0xe0u) >> 5;
        if (!(trd & 0x18u)) flags |= MGPU_F_ALT_Q_BIT;
        airground = (trd >> 8) & 0x40u ? AST_AG_GROUND : AST_AG_AIRBORNE;
    }
    if (f0 & 0x20u) p += 2;                                           // I021/161
    if (f0 & 0x10u) p += 1;                                           // I021/015
    if (f0 & 0x08u) sys = (int64_t) ast_in_time(s, p, now_ms);        // I021/071
    if (f0 & 0x04u) {                                                 // I021/130
        uint32_t a = s[p] << 16 | s[p + 1] << 8 | s[p + 2], o = s[p + 3] << 16 | s[p + 4] << 8 | s[p + 5];
        p += 6;
        const int32_t ia = a >= 0x800000u ? (int32_t) a - 0x1000000 : (int32_t) a, io = o >= 0x800000u ? (int32_t) o - 0x1000000 : (int32_t) o;
        const double la = ia * (180.0 / 8388608.0), lo = io * (180.0 / 8388608.0);
        if (la <= 90 && la >= -90 && lo >= -180 && lo <= 180) { aflags |= MGPU_AST_POS_VALID; lat = la; lon = lo; }
    }
    if (f0 & 0x02u) {                                                 // I021/131
        const uint32_t a = s[p] << 24 | s[p + 1] << 16 | s[p + 2] << 8 | s[p + 3], o = s[p + 4] << 24 | s[p + 5] << 16 | s[p + 6] << 8 | s[p + 7];
        p += 8;
        const double la = ast_in_s32(a) * (180.0 / 1073741824.0), lo = ast_in_s32(o) * (180.0 / 1073741824.0);
        if (la <= 90 && la >= -90 && lo >= -180 && lo <= 180) { aflags |= MGPU_AST_POS_VALID; lat = la; lon = lo; }
    }
    if (f1 & 0x80u) {                                                 // I021/072
        if (sys == -1) sys = (int64_t) ast_in_time(s, p, now_ms);
        else p += 3;
    }
    if (f1 & 0x40u) {                                                 // I021/150
        const uint32_t raw = (s[p] & 0x7fu) << 8 | s[p + 1];
        if (s[p] & 0x80u) { mach = raw * 0.001; flags |= MGPU_F_MACH_VALID; }
        else { ias = (uint32_t) ((raw * (1.0 / 16384.0)) * 3600); flags |= MGPU_F_IAS_VALID; }
        p += 2;
    }
    if (f1 & 0x20u) {                                                 // I021/151
        if (!(s[p] & 0x80u)) { flags |= MGPU_F_TAS_VALID; tas = (s[p] & 0x7fu) << 8 | s[p + 1]; }
        p += 2;
    }
    uint32_t addr = s[p] << 16 | s[p + 1] << 8 | s[p + 2];            // I021/080
    if (addrtype == 3) addr |= 1u << 24;                              // MODES_NON_ICAO_ADDRESS
    p += 3;
    if (f1 & 0x08u) {                                                 // I021/073, /074
        if (aflags & MGPU_AST_POS_VALID) {
            uint64_t ts = ast_in_time(s, p, now_ms);
            if (f1 & 0x04u) ts = ast_in_hp_time(s, p, ts);
            if (sys == -1) sys = (int64_t) ts;
        } else p += f1 & 0x04u ? 7 : 3;
    }
    if (f1 & 0x02u) {                                                 // I021/075, /076
        if (flags & (MGPU_F_IAS_VALID | MGPU_F_MACH_VALID)) {
            uint64_t ts = ast_in_time(s, p, now_ms);
            if (f2 & 0x80u) ts = ast_in_hp_time(s, p, ts);
            if (sys == -1) sys = (int64_t) ts;
        } else p += f2 & 0x80u ? 7 : 3;
    }
    if (f2 & 0x40u) {                                                 // I021/140
        const double alt = ast_in_s16(s[p] << 8 | s[p + 1]) * 6.25;
        if (alt >= -1500 && alt <= 150000) { flags |= MGPU_F_GEOM_ALT_VALID; geom_alt = (int32_t) alt; }
        p += 2;
    }
    uint32_t nicbaro = 0, nacp = 0, sda = 0, gva = 0;
    if (f2 & 0x20u) {                                                 // I021/090
        uint64_t qi;
        if (!ast_in_fspec(s, p, qi)) return AST_IN_UNDEFINED;
        const uint32_t q0 = (uint32_t) qi & 0xffu, q1 = (uint32_t) (qi >> 8) & 0xffu, q2 = (uint32_t) (qi >> 16) & 0xffu;
        aflags |= MGPU_AST_NAC_V_VALID;
        nac_v = q0 >> 5;
        if (q0 & 1u) {
            nicbaro = q1 >> 7;
            sil_out = (q1 & 0x60u) >> 5;
            nacp = (q1 & 0x1eu) >> 1;
            if (q1 & 1u) {
                sil_type = q2 & 0x20u ? AST_SIL_PER_SAMPLE : AST_SIL_PER_HOUR;
                sda = (q2 & 0x18u) >> 3;
                gva = (q2 & 0x06u) >> 1;
            } else sil_type = AST_SIL_UNKNOWN;
        }
    }
    if (f2 & 0x10u) {                                                 // I021/210
        aflags |= MGPU_AST_OPSTATUS_VALID;
        op_version = (s[p] & 0x38u) >> 3;
        const uint32_t ltt = s[p] & 7u;
        p += 1;
        if (op_version == 1 || op_version == 2) {
            aflags |= MGPU_AST_NAC_P_VALID | MGPU_AST_NIC_BARO_VALID;
            nac_p_out = nacp;
            nic_baro_out = nicbaro;
            if (op_version == 1) sil_type = AST_SIL_UNKNOWN;
            else { aflags |= MGPU_AST_GVA_VALID | MGPU_AST_SDA_VALID; gva_out = gva; sda_out = sda; }
        }
        if (ltt == 0) addrtype_out = !addrtype ? AST_ADDR_TISB_ICAO : AST_ADDR_TISB_OTHER;
        else if (ltt == 1) addrtype_out = !addrtype ? AST_ADDR_ADSR_ICAO : AST_ADDR_ADSR_OTHER;
        else if (ltt == 2) addrtype_out = !addrtype ? AST_ADDR_ADSB_ICAO : AST_ADDR_ADSB_OTHER;
        else addrtype_out = AST_ADDR_UNKNOWN;
    }
    if (f2 & 0x08u) {                                                 // I021/070
        const uint32_t a = s[p], b = s[p + 1];
        squawk = ((a & 0xeu) << 11) + ((a & 1u) << 10) + ((b & 0xc0u) << 2) + ((b & 0x38u) << 1) + (b & 7u);
        flags |= MGPU_F_SQUAWK_VALID;
        p += 2;
    }
    if (f2 & 0x04u) {                                                 // I021/230
        roll = (float) (ast_in_s16(s[p] << 8 | s[p + 1]) * 0.01);
        flags |= MGPU_F_ROLL_VALID;
        p += 2;
    }
    uint32_t baro_alt_unit = 0, geom_alt_unit = 0;                    // UNIT_FEET is 0: set or not, the same byte
    if (f2 & 0x02u) {                                                 // I021/145
        flags |= MGPU_F_BARO_ALT_VALID;
        baro_alt = ast_in_s16(s[p] << 8 | s[p + 1]) * 25;
        p += 2;
    }
    if (f3 & 0x80u) {                                                 // I021/152
        flags |= MGPU_F_HEADING_VALID;
        heading_type = AST_HEADING_MAGNETIC;
        heading = (float) ((s[p] << 8 | s[p + 1]) * (360.0 / 65536.0));
        p += 2;
    }
    if (f3 & 0x40u) {                                                 // I021/200
        const uint32_t b = s[p];
        flags |= MGPU_F_SPI_VALID | MGPU_F_ALERT_VALID | MGPU_F_EMERGENCY_VALID;
        aflags |= MGPU_AST_NAV_MODES_VALID;
        nav_modes |= (b & 0x40u) >> 4;
        emergency = (b & 0x1cu) >> 2;
        if (b & 3u) flags |= MGPU_F_ALERT;
        if ((b & 3u) == 3u) flags |= MGPU_F_SPI;
        p += 1;
    }
    if (f3 & 0x20u) {                                                 // I021/155
        if (!(s[p] & 0x80u)) { flags |= MGPU_F_BARO_RATE_VALID; baro_rate = (int32_t) (ast_in_s16(((s[p] & 0x7fu) << 9) + (s[p + 1] << 1)) * 3.125); }
        p += 2;
    }
    if (f3 & 0x10u) {                                                 // I021/157
        if (!(s[p] & 0x80u)) { flags |= MGPU_F_GEOM_RATE_VALID; geom_rate = (int32_t) (ast_in_s16(((s[p] & 0x7fu) << 9) + (s[p + 1] << 1)) * 3.125); }
        p += 2;
    }
    if (f3 & 0x08u) {                                                 // I021/160
        if (!(s[p] & 0x80u)) {
            const uint32_t g = (s[p] & 0x7fu) << 8 | s[p + 1], ta = s[p + 2] << 8 | s[p + 3];
            flags |= MGPU_F_GS_VALID | MGPU_F_HEADING_VALID;
            heading_type = AST_HEADING_GROUND_TRACK;
            gs = (float) (g * (1.0 / 16384.0) * 3600);
            heading = (float) (ta * (360.0 / 65536.0));
        }
        p += 4;
    }
    if (f3 & 0x04u) p += 2;                                           // I021/165
    if (f3 & 0x02u) {                                                 // I021/077
        const uint64_t tt = ast_in_time(s, p, now_ms);
        if (sys == -1) sys = (int64_t) tt;
    }
    if (f4 & 0x80u) {                                                 // I021/170
        const uint64_t cs = (uint64_t) s[p] << 40 | (uint64_t) s[p + 1] << 32 | (uint64_t) s[p + 2] << 24 | (uint64_t) s[p + 3] << 16 | (uint64_t) s[p + 4] << 8 | s[p + 5];
        bool ok = true;
        for (int i = 0; i < 8; ++i) {
            const uint32_t c = ast_in_ais((uint32_t) (cs >> (42 - 6 * i)) & 0x3fu);
            callsign |= (uint64_t) c << (8 * i);
            ok = ok && ((c >= 'A' && c <= 'Z') || (c >= '-' && c <= '9') || c == ' ' || c == '@');
        }
        if (ok) flags |= MGPU_F_CALLSIGN_VALID;
        p += 6;
    }
    if (f4 & 0x40u) {                                                 // I021/020
        category = ast_in_category(s[p]);
        flags |= MGPU_F_CATEGORY_VALID;
        p += 1;
    }
    if (f4 & 0x20u) {                                                 // I021/220
        uint64_t met;
        if (!ast_in_fspec(s, p, met)) return AST_IN_UNDEFINED;
    }
    if (f4 & 0x10u) {                                                 // I021/146
        const uint32_t b = s[p];
        if ((b & 0x80u) && (b & 0x60u)) {
            const uint32_t alt = (b & 0x1fu) << 8 | s[p + 1];
            if (alt < 0x1000u) {
                if ((b & 0x60u) == 0x40u) { aflags |= MGPU_AST_MCP_ALT_VALID; mcp = alt * 25; }
                else if ((b & 0x60u) == 0x60u) { aflags |= MGPU_AST_FMS_ALT_VALID; fms = alt * 25; }
            }
        }
        p += 2;
    }
    if (sys == -1) sys = now_ms;

    r.sysTimestamp = sys;
    r.decoded_lat = lat; r.decoded_lon = lon; r.mach = mach;
    r.addr = addr; r.flags = flags; r.ast_flags = aflags;
    r.baro_alt = baro_alt; r.geom_alt = geom_alt; r.baro_rate = baro_rate; r.geom_rate = geom_rate;
    r.ias = ias; r.tas = tas; r.squawkHex = squawk;
    r.squawkDec = (squawk & 0xf000u) / 0x1000u * 1000u + (squawk & 0x0f00u) / 0x100u * 100u + (squawk & 0x00f0u) / 0x10u * 10u + (squawk & 0x000fu);   // track.h:737
    r.category = category; r.mcp_altitude = mcp; r.fms_altitude = fms;
    r.gs_v0 = gs; r.heading = heading; r.roll = roll;
    for (int i = 0; i < 8; ++i) r.callsign[i] = (char) (uint8_t) (callsign >> (8 * i));
    r.source = (uint8_t) source; r.addrtype = (uint8_t) addrtype_out; r.airground = (uint8_t) airground; r.emergency = (uint8_t) emergency;
    r.nav_modes = (uint8_t) nav_modes; r.nac_v = (uint8_t) nac_v; r.nac_p = (uint8_t) nac_p_out; r.sil = (uint8_t) sil_out; r.sil_type = (uint8_t) sil_type;
    r.gva = (uint8_t) gva_out; r.sda = (uint8_t) sda_out; r.nic_baro = (uint8_t) nic_baro_out; r.op_version = (uint8_t) op_version;
    r.heading_type = (uint8_t) heading_type; r.baro_alt_unit = (uint8_t) baro_alt_unit; r.geom_alt_unit = (uint8_t) geom_alt_unit;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = 0;
    return AST_IN_RECORD;
}
