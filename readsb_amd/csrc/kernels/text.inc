// kernels/text.inc — the two text outputs behind the message list: BaseStation (SBS) lines (modesSendSBSOutput, net_io.c:3184-3404)
// and AVR raw lines (modesSendRawOutput, net_io.c:1837-1863) for records in HBM.
// Part of the single translation unit kernels.hip (included inside namespace mgpu, after beast.inc, whose k_beast_scan it uses).

// Lane = message, three passes like beast.inc.  k_text_size runs the line's formatter into a sink that only counts (a length per
// message, three words per workgroup: bytes, deferred messages, skipped messages), k_beast_scan turns the first two into offsets
// and totals (one workgroup, no atomics), k_text_sum adds the third up (SBS only: no raw record is ever skipped), k_text_write runs THE SAME formatter into a sink that stores bytes to LDS — at the
// alignment (mod 4) the workgroup's first byte will have in memory — and copies the workgroup's lines out as whole words.  One
// formatter per line format: the two passes cannot disagree about a length.
// Digits go straight to the sink, most significant first, by divisions by constants: no char buffer indexed at run time, which
// would live in private memory.

// The longest SBS line, field by field (net_io.c:3249-3401), within the domain sbs_class() admits:
//   "MSG,t,1,1," 10 + "%06X," 7 for an address below 2^24 (9 for a record whose addr has bits above 24 set: %06X prints 8 digits)
//   + "1," 2                                                                                                 19 (21)
//   two dates "YYYY/MM/DD," 11 + times "HH:MM:SS.mmm" 12, a comma after the first three                      47
//   ",callsign" 1 + 8                                                                                          9
//   ",%dH" 1 + 11 ("-2147483648") + 1                                                                         13
//   ",%.0f" twice: |x| < 2^31, so at most "-2147483520": 1 + 11                                               24
//   ",%1.6f" |lat| <= 90: 1 + 10 ("-90.000000"); |lon| <= 360: 1 + 11                                         23
//   ",%dH" vertical rate                                                                                      13
//   ",%04d" of the override squawk, any int but -1: 1 + 11                                                    12
//   four flags ",-1"                                                                                          12
//   "\r\n"                                                                                                     2
// = 174 for every address the field decode produces, 176 for any 32-bit addr.
constexpr int kSbsLineMax = 176;
static_assert(kSbsLineMax == 21 + 47 + 9 + 13 + 24 + 23 + 13 + 12 + 12 + 2, "SBS line bound");
// raw: '@' + 12 digits, 14 bytes as hex pairs, ";\n"
constexpr int kRawLineMax = 43;
static_assert(kRawLineMax == 13 + 2 * 14 + 2, "raw line bound");
static_assert(kBlock * kSbsLineMax + 8 <= 65536 - 64, "k_text_write's static LDS");

enum : int { TEXT_NONE = 0, TEXT_LINE = 1, TEXT_DEFER = 2, TEXT_SKIP = 3 };
constexpr uint16_t kTextDeferred = 0x0100;          // meta of a deferred message (a line's meta is its length, <= 176)

struct CountSink {
    uint32_t n;
    __device__ __forceinline__ void put(uint32_t) { ++n; }
};
struct ByteSink {
    uint8_t *p;
    __device__ __forceinline__ void put(uint32_t c) { *p++ = (uint8_t) c; }
};

__host__ __device__ constexpr uint32_t text_pow10(int k) { return k == 0 ? 1u : 10u * text_pow10(k - 1); }

// %d of an unsigned value with at least `mindigits` digits (zero padded)
template <class S>
__device__ __forceinline__ void put_udec(S &s, uint32_t v, int mindigits) {
    uint32_t r = v;
#pragma unroll
    for (int k = 9; k >= 0; --k) {
        const uint32_t p = text_pow10(k);
        const uint32_t d = r / p;
        r -= d * p;
        if (v >= p || k < mindigits) s.put('0' + d);
    }
}
// %0<width>d of an int: the sign counts towards the width, as in printf
template <class S>
__device__ __forceinline__ void put_idec(S &s, int32_t v, int width = 1) {
    if (v < 0) { s.put('-'); put_udec(s, 0u - (uint32_t) v, width > 1 ? width - 1 : 1); }
    else put_udec(s, (uint32_t) v, width);
}
template <class S>
__device__ __forceinline__ void put_2(S &s, uint32_t v) { s.put('0' + v / 10u); s.put('0' + v % 10u); }
template <class S>
__device__ __forceinline__ void put_3(S &s, uint32_t v) { s.put('0' + v / 100u); put_2(s, v % 100u); }
template <class S>
__device__ __forceinline__ void put_hex(S &s, uint32_t nibble) { s.put(nibble < 10u ? '0' + nibble : 'A' - 10u + nibble); }

// %.0f of a float with |x| < 2^31: printf gets the same number as a double and rounds its exact value half to even, which is rint of
// the float; the sign is printed from the sign bit ("-0" for -0.0f and for negatives that round to zero)
template <class S>
__device__ __forceinline__ void put_f0(S &s, float x) {
    if (__float_as_uint(x) >> 31) s.put('-');
    put_udec(s, (uint32_t) rintf(fabsf(x)), 1);
}

// %1.6f of a double with |x| <= 360, exactly: x = m * 2^e with the 53-bit integer m, so x * 10^6 = (m * 10^6) >> -e with m * 10^6 < 2^73
// held in two 64-bit halves; |x| < 2^9 makes e <= -44, always a right shift.  The bits shifted out are the exact remainder: round half
// to even on them.  Subnormals and zero (exponent field 0: e = -1074, no implicit bit) take the same path.
template <class S>
__device__ __forceinline__ void put_f6(S &s, double x) {
    const uint64_t bits = (uint64_t) __double_as_longlong(x);
    const uint32_t ex = (uint32_t) (bits >> 52) & 0x7ffu;
    const uint64_t m = (bits & 0xfffffffffffffull) | (ex ? 1ull << 52 : 0ull);
    uint32_t sh = 1075u - (ex ? ex : 1u);                         // 44 .. 1074
    if (sh > 127u) sh = 127u;                                     // beyond 74 everything is remainder below the half: the same answer
    const uint64_t lo = m * 1000000ull, hi = __umul64hi(m, 1000000ull);
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
    uint32_t v = (uint32_t) q;                                    // <= 360 000 000
    if (half && (sticky || (v & 1u))) ++v;
    if (bits >> 63) s.put('-');
    const uint32_t ip = v / 1000000u;
    put_udec(s, ip, 1);
    s.put('.');
    put_udec(s, v - ip * 1000000u, 6);
}

// "YYYY/MM/DD,HH:MM:SS.mmm" of milliseconds since 1970 in [0, 253402300800000): gmtime_r's calendar (UTC, no leap seconds) by the
// civil-from-days algorithm over eras of 400 years, all in unsigned 32-bit arithmetic once the day is split off
constexpr int64_t kTextMsEnd = 253402300800000ll;                // 10000-01-01
template <class S>
__device__ __forceinline__ void put_date_time(S &s, int64_t ms) {
    const uint64_t u = (uint64_t) ms;
    const uint32_t days = (uint32_t) (u / 86400000ull);
    const uint32_t rem = (uint32_t) (u - (uint64_t) days * 86400000ull);
    const uint32_t z = days + 719468u;
    const uint32_t era = z / 146097u, doe = z - era * 146097u;
    const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
    const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);
    const uint32_t mp = (5u * doy + 2u) / 153u;
    const uint32_t d = doy - (153u * mp + 2u) / 5u + 1u;
    const uint32_t mo = mp < 10u ? mp + 3u : mp - 9u;
    const uint32_t y = yoe + era * 400u + (mo <= 2u ? 1u : 0u);
    put_2(s, y / 100u); put_2(s, y % 100u); s.put('/'); put_2(s, mo); s.put('/'); put_2(s, d); s.put(',');
    const uint32_t sec = rem / 1000u, msec = rem - sec * 1000u;
    const uint32_t hh = sec / 3600u, mm = (sec - hh * 3600u) / 60u, ss = sec - hh * 3600u - mm * 60u;
    put_2(s, hh); s.put(':'); put_2(s, mm); s.put(':'); put_2(s, ss); s.put('.'); put_3(s, msec);
}

// ---- SBS ----

// msgType 1-8 (net_io.c:3207-3245); 0: no line
__device__ __forceinline__ uint32_t sbs_msg_type(uint32_t df, uint32_t me) {
    switch (df) {
    case 4: case 20: return 5;
    case 5: case 21: return 6;
    case 0: case 16: return 7;
    case 11: return 8;
    case 17: case 18: return me >= 1 && me <= 4 ? 1u : me >= 5 && me <= 8 ? 2u : me >= 9 && me <= 18 ? 3u : me == 19 ? 4u : 0u;
    default: return 0;
    }
}
__device__ __forceinline__ bool sbs_float_ok(float x) { return fabsf(x) < 2147483648.0f; }          // false for NaN and infinities
__device__ __forceinline__ bool sbs_has_heading(const mgpu_fields &f) { return (f.flags & MGPU_F_HEADING_VALID) && f.heading_type == 1 /* HEADING_GROUND_TRACK */; }
__device__ __forceinline__ bool sbs_has_position(uint32_t method) {
    return method == MGPU_CPR_GLOBAL || method == MGPU_CPR_LOCAL_RECEIVER || method == MGPU_CPR_LOCAL_AIRCRAFT;
}

struct SbsJob {
    TextSbsParams a;
    static constexpr int kMax = kSbsLineMax;
    static constexpr bool kSkips = true;

    // In this order: the verdict (outputMessage, net_io.c:5846, 5854: the writer is called with an aircraft, inside the first-message
    // rule), whether the format has a line for the record (:3191, :3207-3245), the domain (modes_gpu.h).  A record outside the
    // domain is TEXT_SKIP whether its line was due or deferred.
    __device__ __forceinline__ int classify(uint64_t i) const {
        int cls = TEXT_LINE;
        if (a.verdict) {
            const uint32_t v = a.verdict[i], w = v & 3u;
            if (w == MGPU_GATE_FORWARD && (v & MGPU_GATE_AIRCRAFT_CERTAIN)) cls = TEXT_LINE;
            else if ((w == MGPU_GATE_DEFER || w == MGPU_GATE_FORWARD) && (v & MGPU_GATE_AIRCRAFT_POSSIBLE)) cls = TEXT_DEFER;
            else return TEXT_NONE;
        }
        const mgpu_fields &f = a.fields[i];
        if ((f.addr & (1u << 24)) || !sbs_msg_type(f.msgtype, f.metype)) return TEXT_NONE;
        const int64_t t = a.msgs[i].sysTimestamp;
        bool ok = t >= 0 && t < kTextMsEnd;
        if (f.flags & MGPU_F_GS_VALID) ok = ok && sbs_float_ok(f.gs_selected);
        if (sbs_has_heading(f)) ok = ok && sbs_float_ok(f.heading);
        if (a.positions && sbs_has_position(a.positions[i].method)) {
            const double lat = a.positions[i].lat, lon = a.positions[i].lon;
            ok = ok && fabs(lat) <= 90.0 && fabs(lon) <= 360.0;                                    // false for NaN
        }
        return ok ? cls : TEXT_SKIP;
    }

    // fields 1-22 and "\r\n" (net_io.c:3249-3401) of a record classify() let through
    template <class S>
    __device__ __forceinline__ void line(uint64_t i, S &s) const {
        const mgpu_fields &f = a.fields[i];
        const uint32_t flags = f.flags;
        const bool gnss = (a.flags & MGPU_SBS_USE_GNSS) != 0;
        s.put('M'); s.put('S'); s.put('G'); s.put(','); s.put('0' + sbs_msg_type(f.msgtype, f.metype));
        s.put(','); s.put('1'); s.put(','); s.put('1'); s.put(',');
        const uint32_t addr = f.addr;
#pragma unroll
        for (int k = 7; k >= 0; --k)
            if (k < 6 || (addr >> (4 * k))) put_hex(s, (addr >> (4 * k)) & 15u);
        s.put(','); s.put('1'); s.put(',');
        put_date_time(s, a.msgs[i].sysTimestamp);
        s.put(',');
        put_date_time(s, a.now_ms);
        s.put(',');                                                                           // field 11
        if (flags & MGPU_F_CALLSIGN_VALID) {
            uint64_t cs;
            __builtin_memcpy(&cs, f.callsign, 8);
            bool open = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t ch = (uint32_t) (cs >> (8 * k)) & 0xffu;
                open = open && ch != 0;
                if (open) s.put(ch);
            }
        }
        s.put(',');                                                                           // field 12
        const int32_t delta = a.geom_delta ? a.geom_delta[i] : INT32_MIN;
        const bool baro = flags & MGPU_F_BARO_ALT_VALID, geom = flags & MGPU_F_GEOM_ALT_VALID, dv = delta != INT32_MIN;
        if (gnss) {                                                                           // (sums wrap as 32-bit integers)
            if (geom) { put_idec(s, f.geom_alt); s.put('H'); }
            else if (baro && dv) { put_idec(s, (int32_t) ((uint32_t) f.baro_alt + (uint32_t) delta)); s.put('H'); }
            else if (baro) put_idec(s, f.baro_alt);
        } else {
            if (baro) put_idec(s, f.baro_alt);
            else if (geom && dv) put_idec(s, (int32_t) ((uint32_t) f.geom_alt - (uint32_t) delta));
        }
        s.put(',');                                                                           // field 13
        if (flags & MGPU_F_GS_VALID) put_f0(s, f.gs_selected);
        s.put(',');                                                                           // field 14
        if (sbs_has_heading(f)) put_f0(s, f.heading);
        s.put(',');                                                                           // fields 15, 16
        if (a.positions && sbs_has_position(a.positions[i].method)) {
            put_f6(s, a.positions[i].lat);
            s.put(',');
            put_f6(s, a.positions[i].lon);
        } else s.put(',');
        s.put(',');                                                                           // field 17
        const bool br = flags & MGPU_F_BARO_RATE_VALID, gr = flags & MGPU_F_GEOM_RATE_VALID;
        if (gnss) {
            if (gr) { put_idec(s, f.geom_rate); s.put('H'); }
            else if (br) put_idec(s, f.baro_rate);
        } else {
            if (br) put_idec(s, f.baro_rate);
            else if (gr) put_idec(s, f.geom_rate);
        }
        s.put(',');                                                                           // field 18
        const bool sq = flags & MGPU_F_SQUAWK_VALID;
        if (a.override_squawk != -1) put_idec(s, a.override_squawk, 4);
        else if (sq) put_udec(s, f.squawkDec, 4);
        s.put(',');                                                                           // field 19
        if (flags & MGPU_F_ALERT_VALID) put_flag(s, flags & MGPU_F_ALERT);
        s.put(',');                                                                           // field 20
        if (sq) put_flag(s, f.squawkHex == 0x7500 || f.squawkHex == 0x7600 || f.squawkHex == 0x7700);
        s.put(',');                                                                           // field 21
        if (flags & MGPU_F_SPI_VALID) put_flag(s, flags & MGPU_F_SPI);
        s.put(',');                                                                           // field 22
        if (f.airground == 1) put_flag(s, true);                                              // AG_GROUND
        else if (f.airground == 2) put_flag(s, false);                                        // AG_AIRBORNE
        s.put('\r'); s.put('\n');
    }
    template <class S>
    static __device__ __forceinline__ void put_flag(S &s, bool set) {
        if (set) { s.put('-'); s.put('1'); } else s.put('0');
    }
};

// ---- AVR raw ----

struct RawJob {
    TextRawParams a;
    static constexpr int kMax = kRawLineMax;

    static constexpr bool kSkips = false;           // no record is outside what a raw line can print

    // the verdicts and flags decide as for the beast frames (k_beast_size): the raw writer needs no aircraft (net_io.c:5863)
    __device__ __forceinline__ int classify(uint64_t i) const {
        const uint32_t bits = a.msgs[i].msgbits;
        if (bits != 16u && bits != 56u && bits != 112u) return TEXT_NONE;
        if (a.flags & MGPU_RAW_VERBATIM) return TEXT_LINE;                                     // lifts both forwarding tests
        if ((a.flags & MGPU_RAW_NET_RULE) && a.msgs[i].correctedbits >= 2) return TEXT_NONE;
        if (!a.verdict) return TEXT_LINE;
        const uint32_t v = a.verdict[i] & 3u;
        return v == MGPU_GATE_FORWARD ? TEXT_LINE : v == MGPU_GATE_DEFER ? TEXT_DEFER : TEXT_NONE;
    }

    template <class S>
    __device__ __forceinline__ void line(uint64_t i, S &s) const {
        const mgpu_msg m = a.msgs[i];
        const uint32_t len = m.msgbits / 8u;
        const bool verb = (a.flags & MGPU_RAW_VERBATIM) != 0;
        if ((a.flags & MGPU_RAW_MLAT) && m.timestamp != 0) {
            // "@%012" PRIX64 and then p += 13 (net_io.c:1848-1850): the FIRST twelve digits of what sprintf wrote
            uint64_t t = (uint64_t) m.timestamp;
            const int extra = t >> 48 ? (64 - __builtin_clzll(t) + 3) / 4 - 12 : 0;
            t >>= 4 * extra;
            s.put('@');
#pragma unroll
            for (int k = 11; k >= 0; --k) put_hex(s, (uint32_t) (t >> (4 * k)) & 15u);
        } else s.put('*');
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            if (k < (int) len) {
                const uint32_t b = verb ? m.raw[k] : m.msg[k];
                put_hex(s, b >> 4); put_hex(s, b & 15u);
            }
        }
        s.put(';'); s.put('\n');
    }
};

// ---- the two passes, for either job ----

template <class JOB>
__global__ __launch_bounds__(kBlock) void k_text_size(JOB job, uint64_t n, uint16_t *meta, uint32_t *block_bytes, uint32_t *block_def, uint32_t *block_skip) {
    __shared__ uint32_t s_sum[kBlock / WAVE], s_def[kBlock / WAVE], s_skip[kBlock / WAVE];
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    uint32_t l = 0;
    int cls = TEXT_NONE;
    if (i < n) {
        cls = job.classify(i);
        if (cls == TEXT_LINE) {
            CountSink s = {0};
            job.line(i, s);
            l = s.n;
        }
        meta[i] = cls == TEXT_DEFER ? kTextDeferred : (uint16_t) l;
    }
    const uint32_t w = (uint32_t) wave_sum_u64(l);
    const uint32_t wd = (uint32_t) __popcll(__ballot(cls == TEXT_DEFER)), ws = (uint32_t) __popcll(__ballot(cls == TEXT_SKIP));
    if (lane_id() == 0) { s_sum[threadIdx.x >> 6] = w; s_def[threadIdx.x >> 6] = wd; s_skip[threadIdx.x >> 6] = ws; }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_bytes[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        block_def[blockIdx.x] = s_def[0] + s_def[1] + s_def[2] + s_def[3];
        if (JOB::kSkips) block_skip[blockIdx.x] = s_skip[0] + s_skip[1] + s_skip[2] + s_skip[3];
    }
}

// the number of skipped messages: only the total is wanted, so a sum over the workgroups' counts, not a scan (one workgroup)
__global__ __launch_bounds__(kScanThreads) void k_text_sum(const uint32_t *block_count, uint32_t nblocks, unsigned long long *total) {
    __shared__ unsigned long long s_part[kScanThreads / WAVE];
    unsigned long long sum = 0;
    for (uint32_t k = threadIdx.x; k < nblocks; k += kScanThreads) sum += block_count[k];
    sum = wave_sum_u64(sum);
    if (lane_id() == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int k = 0; k < kScanThreads / WAVE; ++k) all += s_part[k];
        *total = all;
    }
}

template <class JOB>
__global__ __launch_bounds__(kBlock) void k_text_write(JOB job, uint64_t n, const uint16_t *meta, const unsigned long long *block_off, uint8_t *out, uint64_t cap,
                                                       const unsigned long long *block_def_off, mgpu_deferred *deferred, uint64_t def_cap) {
    __shared__ uint32_t s_wave[kBlock / WAVE], s_wdef[kBlock / WAVE];
    __shared__ __attribute__((aligned(16))) uint8_t s_bytes[kBlock * JOB::kMax + 8];
    const uint32_t wv = threadIdx.x >> 6;
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    const uint32_t mt = i < n ? meta[i] : 0u;
    const bool is_def = mt == kTextDeferred;
    const uint32_t l = is_def ? 0u : mt;
    const uint64_t dm = __ballot(is_def);
    int wtotal;
    const int ex = wave_excl_scan((int) l, wtotal);
    if (lane_id() == 0) { s_wave[wv] = (uint32_t) wtotal; s_wdef[wv] = (uint32_t) __popcll(dm); }
    __syncthreads();
    const unsigned long long base = block_off[blockIdx.x];
    // lines are laid out in LDS at the same alignment (mod 4) they will have in memory, so the copy below moves whole words
    const uint32_t mis = (uint32_t) ((reinterpret_cast<uintptr_t>(out) + base) & 3u);
    uint32_t off = mis + (uint32_t) ex;
    for (uint32_t k = 0; k < wv; ++k) off += s_wave[k];
    const uint32_t block_total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (is_def) {                                             // where the line would start, were it written
        uint32_t rank = (uint32_t) __popcll(dm & ((1ull << lane_id()) - 1));
        for (uint32_t k = 0; k < wv; ++k) rank += s_wdef[k];
        const unsigned long long slot = block_def_off[blockIdx.x] + rank;
        if (slot < def_cap) { mgpu_deferred e; e.index = i; e.offset = base + (off - mis); deferred[slot] = e; }
    }
    if (l) {
        ByteSink s = {s_bytes + off};
        job.line(i, s);
    }
    __syncthreads();
    const uint32_t lo = mis, hi = mis + block_total;
    uint8_t *dst = out + base - mis;                          // dst[k] <-> s_bytes[k]; dst is 4-byte aligned
    if (base + block_total <= cap) {
        const uint32_t wlo = (lo + 3u) & ~3u, whi = hi & ~3u;
        if (whi > wlo) {
            const uint32_t *src32 = reinterpret_cast<const uint32_t *>(s_bytes);
            uint32_t *dst32 = reinterpret_cast<uint32_t *>(dst);
            for (uint32_t w = wlo / 4 + threadIdx.x; w < whi / 4; w += kBlock) dst32[w] = src32[w];
            if (threadIdx.x < 3) {                                 // at most three bytes before and after the word run
                const uint32_t h = lo + threadIdx.x, t = whi + threadIdx.x;
                if (h < wlo) dst[h] = s_bytes[h];
                if (t < hi) dst[t] = s_bytes[t];
            }
        } else {
            for (uint32_t k = lo + threadIdx.x; k < hi; k += kBlock) dst[k] = s_bytes[k];
        }
    } else {                                                  // the capacity cuts this workgroup (or lies before it): bytes below it only
        for (uint32_t k = lo + threadIdx.x; k < hi; k += kBlock)
            if (base + (k - mis) < cap) dst[k] = s_bytes[k];
    }
}

// blocks: three runs of `stride` entries each (bytes, deferred, skipped), off: the first two's offsets; total[3]: bytes, deferred, skipped
// (total[2] is written only for a job that can skip)
template <class JOB>
static void launch_text(const JOB &job, uint64_t n, const TextScratch &w, uint8_t *out, uint64_t cap, mgpu_deferred *deferred, uint64_t def_cap, hipStream_t s) {
    if (n == 0) return;
    const unsigned blocks = (unsigned) ((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_text_size<JOB>, dim3(blocks), dim3(kBlock), 0, s, job, n, w.meta, w.blocks, w.blocks + w.stride, w.blocks + 2 * w.stride);
    for (int k = 0; k < 2; ++k)
        hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, w.blocks + k * w.stride, blocks, w.off + k * w.stride, w.total + k);
    if (JOB::kSkips) hipLaunchKernelGGL(k_text_sum, dim3(1), dim3(kScanThreads), 0, s, w.blocks + 2 * w.stride, blocks, w.total + 2);
    hipLaunchKernelGGL(k_text_write<JOB>, dim3(blocks), dim3(kBlock), 0, s, job, n, w.meta, w.off, out, cap, w.off + w.stride, deferred, def_cap);
}

void launch_sbs_encode(const TextSbsParams &a, uint64_t n, const TextScratch &w, uint8_t *out, uint64_t cap, mgpu_deferred *deferred, uint64_t def_cap, hipStream_t s) {
    launch_text(SbsJob{a}, n, w, out, cap, deferred, def_cap, s);
}
void launch_raw_encode(const TextRawParams &a, uint64_t n, const TextScratch &w, uint8_t *out, uint64_t cap, mgpu_deferred *deferred, uint64_t def_cap, hipStream_t s) {
    launch_text(RawJob{a}, n, w, out, cap, deferred, def_cap, s);
}
