// kernels/asterix.inc — the fourth output behind the message list: ASTERIX CAT021 target reports (modesSendAsterixOutput,
// net_io.c:2416-2945) for records in HBM.  Part of the single translation unit kernels.hip (included inside namespace mgpu, after
// text.inc, whose sinks, passes and launcher it uses: AsterixJob is a third job beside SbsJob / RawJob, lane = message).
//
// A record is the category byte 21, a 16-bit big-endian length, an FSPEC of 4 to 6 bytes and the items in the order the reference's
// writer appends them — its source order, NOT the order of the UAP.  Which items a record has follows from the valid flags alone, so
// the formatter settles FSPEC and length first and then runs the items into the sink: one formatter for the counting and the writing
// pass.  Everything the reference does is mirrored, nothing corrected (include/modes_gpu.h lists the points that look like mistakes).
// Every product and quotient is taken in the type C gives it in the reference (readsb.h:996-1054); the library is built with
// -ffp-contract=off and without fast-math, and no expression here could contract anyway (no product feeds a sum).
// --net-asterix-reduce (mm->reduce_forward, the tracker's) is not modelled.

// The longest record, item by item (net_io.c:2436-2889):
//   category 1 + length 2                                                                                       3
//   FSPEC                                                                                                        6
//   I021/010 2, /040 1 + 1 extension, /130 6, /150 2, /151 2, /080 3, /073 3                                    20
//   /075 3 and /160 4 (heading_type == HEADING_GROUND_TRACK) — or /152 2 (HEADING_MAGNETIC): never both           7
//   /140 2, /090 1 + 2 extensions, /210 1, /070 2, /230 2, /145 2                                               12
//   /200 1, /155 2, /157 2, /077 3                                                                               8
//   /170 6, /020 1, /220 1 + 4 (wind) + 2 (temperature), /146 2, /008 1, /400 1                                 18
// = 74.  (A sum over every item gives 76: it counts /152 beside /075 and /160, which one heading_type cannot give.)
constexpr int kAsterixRecordMax = 74;
static_assert(kAsterixRecordMax == 3 + 6 + 20 + 7 + 12 + 8 + 18, "CAT021 record bound");
static_assert(kAsterixRecordMax < kTextDeferred, "a record's meta is its length");
static_assert(kBlock * kAsterixRecordMax + 8 <= 65536 - 64, "k_text_write's static LDS");

// the domain of the reference's float -> integer conversions: finite and below 2^31 in magnitude (false for NaN)
__device__ __forceinline__ bool asx_ok(double x) { return fabs(x) < 2147483648.0; }
__device__ __forceinline__ bool asx_okf(float x) { return fabsf(x) < 2147483648.0f; }

// "int tsm = t - midnight; if (tsm < 0) tsm += 86400000; tsm = (int)(tsm * 0.128)" (net_io.c:2535-2539): the difference truncated to
// 32 bits, the product in double
__device__ __forceinline__ uint32_t asx_time_of_day(int64_t t, int64_t midnight) {
    int32_t tsm = (int32_t) (uint32_t) ((uint64_t) t - (uint64_t) midnight);
    if (tsm < 0) tsm += 86400000;
    return (uint32_t) (int32_t) ((double) tsm * 0.128);
}
template <class S>
__device__ __forceinline__ void put_be16(S &s, uint32_t v) { s.put((v >> 8) & 0xffu); s.put(v & 0xffu); }
template <class S>
__device__ __forceinline__ void put_be24(S &s, uint32_t v) { s.put((v >> 16) & 0xffu); put_be16(s, v); }

// char_to_ais (net_io.c:212-224): the index in "@A-Z[\]^_ !"#$%&'()*+,-./0-9:;<=>?", 32 for NUL and for every other byte
__device__ __forceinline__ uint32_t asx_char_to_ais(uint32_t ch) {
    return ch >= 0x40u && ch <= 0x5fu ? ch - 0x40u : ch >= 0x20u && ch <= 0x3fu ? ch : 32u;
}

// I021/020 (net_io.c:2751-2819).  -> whether the FSPEC bit is set; *byte: the value written, -1: none (a (tc, ca) pair without a case)
__device__ __forceinline__ bool asx_emitter_category(const mgpu_fields &f, uint32_t ac_category, int *byte) {
    *byte = -1;
    if (!(f.flags & MGPU_F_CATEGORY_VALID)) {
        if (ac_category) return false;
        *byte = 0;
        return true;
    }
    const int tc = 0x0e - (int) ((f.category & 0xf0u) >> 4), ca = f.category & 7;
    if (!ca) { *byte = 0; return true; }
    switch (tc) {
    case 2: *byte = ca == 1 ? 20 : ca == 3 ? 21 : ca >= 4 ? 22 : -1; break;
    case 3: *byte = ca == 1 ? 11 : ca == 2 ? 12 : ca == 3 ? 16 : ca == 4 ? 15 : ca == 6 ? 13 : ca == 7 ? 14 : -1; break;
    case 4: *byte = ca == 7 ? 10 : ca; break;
    default: break;
    }
    return true;
}

struct AsterixJob {
    TextAsterixParams a;
    static constexpr int kMax = kAsterixRecordMax;
    static constexpr bool kSkips = true;

    __device__ __forceinline__ bool has_position(uint64_t i) const { return a.positions && sbs_has_position(a.positions[i].method); }
    static __device__ __forceinline__ bool has_velocity(const mgpu_fields &f) {          // I021/075 and I021/160 (:2546, :2709)
        return (f.flags & MGPU_F_GS_VALID) && (f.flags & MGPU_F_HEADING_VALID) && f.heading_type == 1 /* HEADING_GROUND_TRACK */;
    }
    static __device__ __forceinline__ bool has_mag_heading(const mgpu_fields &f) {       // I021/152 (:2668)
        return (f.flags & MGPU_F_HEADING_VALID) && f.heading_type == 3 /* HEADING_MAGNETIC */;
    }

    // The verdict as for the raw lines without MGPU_RAW_NET_RULE (outputMessage, net_io.c:5846, 5882: inside the first-message rule, no
    // aircraft and no correctedbits test), then the domain of modes_gpu.h over the items the record has.  A record outside the domain is
    // TEXT_SKIP whether it was due or deferred.
    __device__ __forceinline__ int classify(uint64_t i) const {
        int cls = TEXT_LINE;
        if (a.verdict) {
            const uint32_t v = a.verdict[i] & 3u;
            if (v == MGPU_GATE_DEFER) cls = TEXT_DEFER;
            else if (v != MGPU_GATE_FORWARD) return TEXT_NONE;
        }
        const mgpu_fields &f = a.fields[i];
        const uint32_t flags = f.flags;
        bool ok = true;
        if (has_position(i)) {
            const double lat = a.positions[i].lat, lon = a.positions[i].lon;
            ok = ok && fabs(lat) <= 90.0 && fabs(lon) <= 360.0;                                   // false for NaN
        }
        if (flags & MGPU_F_MACH_VALID) ok = ok && asx_ok((double) f.mach * 1000);
        if (flags & MGPU_F_ROLL_VALID) ok = ok && asx_okf(f.roll * 100);
        if ((flags & MGPU_F_BARO_ALT_VALID) && f.baro_alt_unit == 1 /* UNIT_METERS */) ok = ok && asx_ok(f.baro_alt * 3.2808);
        if (has_mag_heading(f)) ok = ok && asx_ok((double) f.heading * 182.0444);
        if (has_velocity(f)) ok = ok && asx_ok((double) f.gs_v0 * 4.5511) && asx_ok((double) f.heading * (65536 / 360.0));
        if (flags & MGPU_F_WIND_VALID) ok = ok && asx_okf(f.wind_direction);
        if (flags & MGPU_F_OAT_VALID) ok = ok && asx_okf(f.oat * 4);
        return ok ? cls : TEXT_SKIP;
    }

    // the record of a message classify() let through (net_io.c:2434-2942)
    template <class S>
    __device__ __forceinline__ void line(uint64_t i, S &s) const {
        const mgpu_fields &f = a.fields[i];
        const uint32_t flags = f.flags, acc = f.acc_flags, nav = f.nav_flags, op = f.op_flags;
        const bool pos = has_position(i), vel = has_velocity(f), magh = has_mag_heading(f);
        const bool mach = flags & MGPU_F_MACH_VALID, speed = mach || (flags & MGPU_F_IAS_VALID), tas = flags & MGPU_F_TAS_VALID;
        const bool geom = flags & MGPU_F_GEOM_ALT_VALID, height = geom || (flags & MGPU_F_GEOM_DELTA_VALID);
        const bool ops = op & MGPU_OP_VALID, squawk = flags & MGPU_F_SQUAWK_VALID, roll = flags & MGPU_F_ROLL_VALID;
        const bool baro = flags & MGPU_F_BARO_ALT_VALID;
        const bool status = (flags & (MGPU_F_SPI_VALID | MGPU_F_ALERT_VALID | MGPU_F_EMERGENCY_VALID)) || (nav & MGPU_NAV_MODES_VALID);
        const bool brate = flags & MGPU_F_BARO_RATE_VALID, grate = flags & MGPU_F_GEOM_RATE_VALID, callsign = flags & MGPU_F_CALLSIGN_VALID;
        const bool wind = flags & MGPU_F_WIND_VALID, oat = flags & MGPU_F_OAT_VALID;
        const bool met = wind || oat || (flags & (MGPU_F_TURBULENCE_VALID | MGPU_F_STATIC_PRESSURE_VALID | MGPU_F_HUMIDITY_VALID));
        const bool mcp = nav & MGPU_NAV_MCP_ALT_VALID, sel = mcp || (nav & MGPU_NAV_FMS_ALT_VALID);
        const uint32_t cc_tc = f.op_cc_tc & 3u;                                                  // opstatus.cc_tc is a 2-bit field, version a 3-bit one
        const bool ops8 = ops && ((op & (MGPU_OP_OM_ACAS_RA | MGPU_OP_CC_TS | MGPU_OP_CC_ARV | MGPU_OP_CC_CDTI)) || cc_tc || !(op & MGPU_OP_CC_ACAS));
        const unsigned long long id = a.ids ? a.ids[i] : 0ull;
        int cat_byte;
        const bool cat = asx_emitter_category(f, a.ac_category ? a.ac_category[i] : 0u, &cat_byte);

        // I021/040 (:2441-2459): the extension is tested in bytes[p + 1] before p advances
        uint32_t trd = (f.addr & (1u << 24)) ? 3u << 5 : (f.addrtype == 8 || f.addrtype == 11 || f.addrtype == 9) ? 2u << 5 : 0u;   // ADDR_ADSB_ / TISB_ / ADSR_OTHER
        if (!(flags & MGPU_F_ALT_Q_BIT)) trd |= 1u << 3;
        const bool ground = f.airground == 1;                                                   // AG_GROUND
        // I021/090 (:2576-2601): additions into and ors of unsigned chars; cpr_nucp is never set and contributes 0.  The second
        // extension's bits go to bytes[p + 1] of wherever p stands: the first extension's place when that one stayed empty
        uint32_t q0 = (acc & MGPU_ACC_NAC_V_VALID) ? ((uint32_t) f.nac_v << 5) & 0xffu : 0u, q1 = 0, q2 = 0;
        if (acc & MGPU_ACC_NIC_BARO_VALID) q1 |= (acc & MGPU_ACC_NIC_BARO) ? 0x80u : 0u;
        if (f.sil_type != 0) q1 |= ((uint32_t) f.sil << 5) & 0xffu;                              // != SIL_INVALID
        if (acc & MGPU_ACC_NAC_P_VALID) q1 |= ((uint32_t) f.nac_p << 1) & 0xffu;
        if (f.sil_type == 2) q2 |= 1u << 5;                                                      // SIL_PER_SAMPLE
        if (acc & MGPU_ACC_SDA_VALID) q2 |= ((uint32_t) f.sda << 3) & 0xffu;
        if (acc & MGPU_ACC_GVA_VALID) q2 |= ((uint32_t) f.gva << 1) & 0xffu;

        uint32_t fs0 = 0xc0u | (pos ? 1u << 2 : 0u);
        uint32_t fs1 = (speed ? 1u << 6 : 0u) | (tas ? 1u << 5 : 0u) | 1u << 4 | (pos ? 1u << 3 : 0u) | (vel ? 1u << 1 : 0u);
        uint32_t fs2 = (height ? 1u << 6 : 0u) | 1u << 5 | (ops ? 1u << 4 : 0u) | (squawk ? 1u << 3 : 0u) | (roll ? 1u << 2 : 0u) | (baro ? 1u << 1 : 0u);
        uint32_t fs3 = (magh ? 1u << 7 : 0u) | (status ? 1u << 6 : 0u) | (brate ? 1u << 5 : 0u) | (grate ? 1u << 4 : 0u) | (vel ? 1u << 3 : 0u) | 1u << 1;
        uint32_t fs4 = (callsign ? 1u << 7 : 0u) | (cat ? 1u << 6 : 0u) | (met ? 1u << 5 : 0u) | (sel ? 1u << 4 : 0u);
        const uint32_t fs5 = (ops8 ? 1u << 7 : 0u) | (id ? 1u << 2 : 0u);
        // the extension bits from the back (:2920-2927); fs3 is never 0 (I021/077)
        if (fs5) fs4 |= 1u;
        if (fs4) fs3 |= 1u;
        fs2 |= 1u; fs1 |= 1u; fs0 |= 1u;
        const uint32_t fspec_len = fs5 ? 6u : fs4 ? 5u : 4u;
        const uint32_t items = 2u + 1u + (ground ? 1u : 0u) + (pos ? 6u + 3u : 0u) + (speed ? 2u : 0u) + (tas ? 2u : 0u) + 3u + (vel ? 3u + 4u : 0u)
            + (height ? 2u : 0u) + 1u + (q1 ? 1u : 0u) + (q2 ? 1u : 0u) + (ops ? 1u : 0u) + (squawk ? 2u : 0u) + (roll ? 2u : 0u) + (baro ? 2u : 0u)
            + (magh ? 2u : 0u) + (status ? 1u : 0u) + (brate ? 2u : 0u) + (grate ? 2u : 0u) + 3u + (callsign ? 6u : 0u) + (cat_byte >= 0 ? 1u : 0u)
            + (met ? 1u + (wind ? 4u : 0u) + (oat ? 2u : 0u) : 0u) + (sel ? 2u : 0u) + (ops8 ? 1u : 0u) + (id ? 1u : 0u);

        s.put(21);
        put_be16(s, items + 3u + fspec_len);
        s.put(fs0); s.put(fs1); s.put(fs2); s.put(fs3);
        if (fspec_len > 4u) s.put(fs4);
        if (fspec_len > 5u) s.put(fs5);

        s.put(0); s.put(1);                                                                   // I021/010: SAC 0, SIC 1
        if (ground) { s.put(trd | 1u); s.put(1u << 6); } else s.put(trd);                     // I021/040
        const int64_t midnight = a.now_ms / 1000 / 86400 * 86400000;
        const uint32_t tod_msg = asx_time_of_day(a.msgs[i].sysTimestamp, midnight);
        if (pos) {                                                                            // I021/130 (:2462-2480)
            int32_t lat = (int32_t) (a.positions[i].lat / (180 / 8388608.0)), lon = (int32_t) (a.positions[i].lon / (180 / 8388608.0));
            if (lat < 0) lat += 0x1000000;
            if (lon < 0) lon += 0x1000000;
            put_be24(s, (uint32_t) lat);
            put_be24(s, (uint32_t) lon);
        }
        if (speed) {                                                                          // I021/150 (:2501-2513)
            const uint32_t v = mach ? (uint32_t) (int32_t) ((double) f.mach * 1000) : (uint32_t) (int32_t) (f.ias / 3600.0 * 16384.0);
            s.put((mach ? 1u << 7 : 0u) | ((v & 0x7f00u) >> 8));
            s.put(v & 0xffu);
        }
        if (tas) { s.put((f.tas & 0x7f00u) >> 8); s.put(f.tas & 0xffu); }                     // I021/151
        put_be24(s, f.addr);                                                                  // I021/080
        if (pos) put_be24(s, tod_msg);                                                        // I021/073: follows from the FSPEC bit (:2533)
        if (vel) put_be24(s, tod_msg);                                                        // I021/075
        if (geom) {                                                                           // I021/140 (:2559-2574)
            put_be16(s, (uint32_t) (int32_t) (f.geom_alt_unit == 0 /* UNIT_FEET */ ? f.geom_alt / 6.25 : f.geom_alt / 20.5053));
        } else if (height) {                                                                  // the aircraft's baro_alt + the message's delta, wrapping
            const int32_t sum = (int32_t) ((uint32_t) (a.ac_baro_alt ? a.ac_baro_alt[i] : 0) + (uint32_t) f.geom_delta);
            put_be16(s, (uint32_t) (int32_t) (sum / 6.25));
        }
        if (q1) { s.put(q0 | 1u); if (q2) { s.put(q1 | 1u); s.put(q2); } else s.put(q1); }    // I021/090
        else if (q2) { s.put(q0 | 1u); s.put(q2); }
        else s.put(q0);
        if (ops) {                                                                            // I021/210 (:2604-2636)
            uint32_t v;
            if (a.flags & MGPU_ASTERIX_REMOTE) v = (f.addrtype == 0 || f.addrtype == 8) ? 2u : (f.addrtype == 2 || f.addrtype == 9) ? 1u : 0u;
            else v = f.source == 10 /* SOURCE_ADSB */ ? 2u : f.source == 9 /* SOURCE_ADSR */ ? 1u : 0u;
            s.put(v | ((f.op_version & 7u) << 3));
        }
        if (squawk) {                                                                         // I021/070 (:2639-2647)
            const uint32_t q = f.squawkHex;
            s.put(((q & 0x7000u) >> 11) | ((q & 0x0400u) >> 10));
            s.put(((q & 0x0300u) >> 2) | ((q & 0x0070u) >> 1) | (q & 7u));
        }
        if (roll) put_be16(s, (uint32_t) (int32_t) (f.roll * 100));                           // I021/230: a float product
        if (baro) {                                                                           // I021/145 (:2658-2665)
            const int32_t v = f.baro_alt_unit == 1 /* UNIT_METERS */ ? (int32_t) (f.baro_alt * 3.2808) : f.baro_alt / 25;
            put_be16(s, (uint32_t) v);
        }
        if (magh) put_be16(s, (uint32_t) (int32_t) ((double) f.heading * 182.0444));          // I021/152
        if (status) {                                                                         // I021/200 (:2677-2690)
            uint32_t v = 0;
            if ((nav & MGPU_NAV_MODES_VALID) && (f.nav_modes & 2u)) v |= 1u << 6;
            if (flags & MGPU_F_EMERGENCY_VALID) v |= ((uint32_t) f.emergency << 2) & 0xffu;
            if (flags & MGPU_F_ALERT_VALID) v |= (flags & MGPU_F_ALERT) ? 1u : 0u;
            else if ((flags & MGPU_F_SPI_VALID) && (flags & MGPU_F_SPI)) v |= 3u;
            s.put(v);
        }
        if (brate) {                                                                          // I021/155: (int16_t) and then an arithmetic shift
            const int32_t v = (int32_t) (int16_t) (int32_t) (f.baro_rate / 3.125) >> 1;
            s.put(((uint32_t) v & 0x7f00u) >> 8); s.put((uint32_t) v & 0xffu);
        }
        if (grate) {                                                                          // I021/157
            const int32_t v = (int32_t) (int16_t) (int32_t) (f.geom_rate / 3.125) >> 1;
            s.put(((uint32_t) v & 0x7f00u) >> 8); s.put((uint32_t) v & 0xffu);
        }
        if (vel) {                                                                            // I021/160 (:2709-2718)
            const uint32_t gs = (uint32_t) (int32_t) ((double) f.gs_v0 * 4.5511);
            s.put((gs & 0x7f00u) >> 8); s.put(gs & 0xffu);
            put_be16(s, (uint32_t) (int32_t) ((double) f.heading * (65536 / 360.0)));
        }
        put_be24(s, asx_time_of_day(a.now_ms, midnight));                                     // I021/077
        if (callsign) {                                                                       // I021/170 (:2734-2748)
            uint64_t cs, enc = 0;
            __builtin_memcpy(&cs, f.callsign, 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) enc = (enc << 6) + asx_char_to_ais((uint32_t) (cs >> (8 * k)) & 0xffu);
            put_be24(s, (uint32_t) (enc >> 24));
            put_be24(s, (uint32_t) enc);
        }
        if (cat_byte >= 0) s.put((uint32_t) cat_byte);                                        // I021/020
        if (met) {                                                                            // I021/220 (:2822-2850)
            s.put((wind ? 0xc0u : 0u) | (oat ? 0x20u : 0u));
            if (wind) { put_be16(s, f.wind_speed); put_be16(s, (uint32_t) (int32_t) f.wind_direction); }
            if (oat) put_be16(s, (uint32_t) (int32_t) (f.oat * 4));                           // a float product
        }
        if (sel) {                                                                            // I021/146 (:2853-2867): MCP wins
            const int32_t alt = (int32_t) (mcp ? f.nav_mcp_altitude : f.nav_fms_altitude) / 25;
            s.put((mcp ? 0xc0u : 0xe0u) | (((uint32_t) alt & 0x1f00u) >> 8));
            s.put((uint32_t) alt & 0xffu);
        }
        if (ops8)                                                                             // I021/008 (:2870-2883)
            s.put(((op & MGPU_OP_OM_ACAS_RA) ? 1u << 7 : 0u) | cc_tc << 5 | ((op & MGPU_OP_CC_TS) ? 1u << 4 : 0u) | ((op & MGPU_OP_CC_ARV) ? 1u << 3 : 0u)
                  | ((op & MGPU_OP_CC_CDTI) ? 1u << 2 : 0u) | ((op & MGPU_OP_CC_ACAS) ? 0u : 1u << 1));
        if (id) s.put((uint32_t) id & 0xffu);                                                 // I021/400
    }
};

void launch_asterix_encode(const TextAsterixParams &a, uint64_t n, const TextScratch &w, uint8_t *out, uint64_t cap, mgpu_deferred *deferred, uint64_t def_cap,
                           hipStream_t s) {
    launch_text(AsterixJob{a}, n, w, out, cap, deferred, def_cap, s);
}
