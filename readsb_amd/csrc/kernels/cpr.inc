// kernels/cpr.inc — position decode on the device: cpr.c's three decoders (cpr.c:62-374) and the pairing of even / odd position
// messages that updatePosition does around them (track.c:1249-1282, 1827-1850, 843-917), over the message list.
// Part of the single translation unit kernels.hip (included inside namespace mgpu, behind kernels/gate.inc whose sort it uses).
//
// The arithmetic is IEEE double — divide, floor, fmod, compares against the NL table — in the reference's order of operations, and the
// library is built with -ffp-contract=off: every latitude / longitude equals the reference's bit for bit (tests/golden/cpr_cases.npz,
// written by the reference's own object file).
//
// The pairing per position message (MGPU_F_CPR_VALID, DF17 / DF18), in stream order per address:
//   1. the aircraft's even or odd slot becomes this message's words, type, source and time (accept_cpr, track.c:1829-1844);
//   2. max_elapsed: surface 50 s if the message's own ground speed is valid and <= 25 kt, else 25 s (track.c:1266-1269); airborne
//      cfg.airborne_max_elapsed_ms, 0 = the reference's 10 s fallback (track.c:1237);
//   3. a GLOBAL decode iff both slots are filled with the same type and source no further apart than max_elapsed (track.c:1279-1282);
//      surface needs the receiver's location (track.c:763-766), else -1;  0: GLOBAL, -2: BAD, -1 / not attempted: 4;
//   4. a LOCAL decode (track.c:862-914) relative to the aircraft's last GLOBAL result of this stage while it is younger than 10 min,
//      else — airborne only — relative to the receiver, else none.
// Out of scope, the host tracker's business: the speed-dependent airborne window (track.c:1239-1246 reads the tracker's a->gs), the
// range / speed / duplicate checks (track.c:423-745, 784-792, 813-838, 919-956).  The reference's local decode refers to the tracker's
// latest ACCEPTED position (a->lat / a->lon, which a local result may move); here only GLOBAL results of this stage move the
// reference — which makes it "the last flagged message before this one" (a scan) instead of a chain through every message.
//
// The state is a direct-indexed table like the gate's: 2^25 addresses x 64 bytes = 2 GiB, zero = nothing known.  The position messages
// are brought into (address, stream order) by the gate's radix sort (every other message gets a key behind all aircraft), one wave
// walks each address's run, 64 messages per step: "the last even / odd message below this lane" comes from a ballot, its words and
// time from shuffles; the global decodes of the 64 messages are independent of each other; "the last successful global decode below
// this lane" is a second ballot, and the local decodes follow.  Between steps the slots and the reference are wave-uniform carries.

struct CprAc {                   // 64 bytes; all zero = nothing known
    long long t_even, t_odd, t_global;
    double g_lat, g_lon;         // the last GLOBAL result
    uint32_t even_w0, even_w1, odd_w0, odd_w1;   // the slots, as CprInfo's words
    uint32_t valid;              // bit 0: even slot, bit 1: odd slot, bit 2: global reference
    uint32_t pad;
};
static_assert(sizeof(CprAc) == 64, "CprAc");
struct CprInfo {                 // 16 bytes per message of the call
    long long now;               // mm->sysTimestamp
    uint32_t w0;                 // cpr_lat | cpr_type << 17 | odd << 19 | (gs valid and <= 25 kt) << 20 | source << 24
    uint32_t w1;                 // cpr_lon
};
constexpr uint32_t kCprPairMask = (3u << 17) | (0xffu << 24);        // what both halves of a pair must share: type and source
constexpr long long kCprLocalTtl = 10 * 60 * 1000;

// cprNLFunction (cpr.c:79-146): the table of 1090-WP-9-14, NL = 59 - (thresholds <= |lat|); the reference's three shortcuts
// (> 60, > 44.2, > 30) only skip thresholds that are smaller anyway.
__device__ const double kCprNl[58] = {
    10.47047130, 14.82817437, 18.18626357, 21.02939493, 23.54504487, 25.82924707, 27.93898710, 29.91135686, 31.77209708, 33.53993436,
    35.22899598, 36.85025108, 38.41241892, 39.92256684, 41.38651832, 42.80914012, 44.19454951, 45.54626723, 46.86733252, 48.16039128,
    49.42776439, 50.67150166, 51.89342469, 53.09516153, 54.27817472, 55.44378444, 56.59318756, 57.72747354, 58.84763776, 59.95459277,
    61.04917774, 62.13216659, 63.20427479, 64.26616523, 65.31845310, 66.36171008, 67.39646774, 68.42322022, 69.44242631, 70.45451075,
    71.45986473, 72.45884545, 73.45177442, 74.43893416, 75.42056257, 76.39684391, 77.36789461, 78.33374083, 79.29428225, 80.24923213,
    81.19801349, 82.13956981, 83.07199445, 83.99173563, 84.89166191, 85.75541621, 86.53536998, 87.00000000};

__device__ __forceinline__ int cpr_nl(double lat) {
    if (lat < 0) lat = -lat;
    int lo = 0, hi = 58;                                   // the first threshold lat is below (58: none)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lat < kCprNl[mid]) hi = mid; else lo = mid + 1;
    }
    return 59 - lo;
}
__device__ __forceinline__ int cpr_n(double lat, int fflag) {
    const int nl = cpr_nl(lat) - (fflag ? 1 : 0);
    return nl < 1 ? 1 : nl;
}
__device__ __forceinline__ double cpr_dlon(double lat, int fflag, int surface) { return (surface ? 90.0 : 360.0) / cpr_n(lat, fflag); }
__device__ __forceinline__ int cpr_mod_int(int a, int b) { const int r = a % b; return r < 0 ? r + b : r; }
__device__ __forceinline__ double cpr_mod_double(double a, double b) { double r = fmod(a, b); if (r < 0) r += b; return r; }

// decodeCPRairborne (cpr.c:170-221) / decodeCPRsurface (cpr.c:223-319): one body, the two differ in the zone size, in how a
// latitude comes into range and in the surface decode's pull towards the reference location.
__device__ __forceinline__ int cpr_decode_global(bool surface, double reflat, double reflon, int even_lat, int even_lon, int odd_lat, int odd_lon,
                                                 int fflag, double *out_lat, double *out_lon) {
    const double dlat0 = (surface ? 90.0 : 360.0) / 60.0, dlat1 = (surface ? 90.0 : 360.0) / 59.0;
    const double lat0 = even_lat, lat1 = odd_lat, lon0 = even_lon, lon1 = odd_lon;
    const int j = (int) floor(((59 * lat0 - 60 * lat1) / 131072) + 0.5);
    double rlat0 = dlat0 * (cpr_mod_int(j, 60) + lat0 / 131072);
    double rlat1 = dlat1 * (cpr_mod_int(j, 59) + lat1 / 131072);
    if (surface) {                                        // the quadrant nearest to the reference; -90, 0 and +90 all encode to 0
        if (rlat0 == 0) {
            if (reflat < -45) rlat0 = -90;
            else if (reflat > 45) rlat0 = 90;
        } else if ((rlat0 - reflat) > 45) rlat0 -= 90;
        if (rlat1 == 0) {
            if (reflat < -45) rlat1 = -90;
            else if (reflat > 45) rlat1 = 90;
        } else if ((rlat1 - reflat) > 45) rlat1 -= 90;
    } else {
        if (rlat0 >= 270) rlat0 -= 360;
        if (rlat1 >= 270) rlat1 -= 360;
    }
    if (rlat0 < -90 || rlat0 > 90 || rlat1 < -90 || rlat1 > 90) return -2;
    if (cpr_nl(rlat0) != cpr_nl(rlat1)) return -1;        // the pair straddles a latitude zone
    double rlat, rlon;
    if (fflag) {
        const int ni = cpr_n(rlat1, 1);
        const int m = (int) floor((((lon0 * (cpr_nl(rlat1) - 1)) - (lon1 * cpr_nl(rlat1))) / 131072.0) + 0.5);
        rlon = cpr_dlon(rlat1, 1, surface) * (cpr_mod_int(m, ni) + lon1 / 131072);
        rlat = rlat1;
    } else {
        const int ni = cpr_n(rlat0, 0);
        const int m = (int) floor((((lon0 * (cpr_nl(rlat0) - 1)) - (lon1 * cpr_nl(rlat0))) / 131072) + 0.5);
        rlon = cpr_dlon(rlat0, 0, surface) * (cpr_mod_int(m, ni) + lon0 / 131072);
        rlat = rlat0;
    }
    if (surface) rlon += floor((reflon - rlon + 45) / 90) * 90;   // towards the reference by whole quadrants
    rlon -= floor((rlon + 180) / 360) * 360;
    *out_lat = rlat;
    *out_lon = rlon;
    return 0;
}
__device__ int decodeCPRairborne(int even_lat, int even_lon, int odd_lat, int odd_lon, int fflag, double *out_lat, double *out_lon) {
    return cpr_decode_global(false, 0.0, 0.0, even_lat, even_lon, odd_lat, odd_lon, fflag, out_lat, out_lon);
}
__device__ int decodeCPRsurface(double reflat, double reflon, int even_lat, int even_lon, int odd_lat, int odd_lon, int fflag, double *out_lat,
                                double *out_lon) {
    return cpr_decode_global(true, reflat, reflon, even_lat, even_lon, odd_lat, odd_lon, fflag, out_lat, out_lon);
}
// decodeCPRrelative (cpr.c:331-374)
__device__ int decodeCPRrelative(double reflat, double reflon, int cprlat, int cprlon, int fflag, int surface, double *out_lat, double *out_lon) {
    const double flat = cprlat / 131072.0, flon = cprlon / 131072.0;
    const double dlat = (surface ? 90.0 : 360.0) / (fflag ? 59.0 : 60.0);
    const int j = (int) (floor(reflat / dlat) + floor(0.5 + cpr_mod_double(reflat, dlat) / dlat - flat));
    double rlat = dlat * (j + flat);
    if (rlat >= 270) rlat -= 360;
    if (rlat < -90 || rlat > 90) return -1;
    if (fabs(rlat - reflat) > (dlat / 2)) return -1;       // more than half a cell away
    const double dlon = cpr_dlon(rlat, fflag, surface);
    const int m = (int) (floor(reflon / dlon) + floor(0.5 + cpr_mod_double(reflon, dlon) / dlon - flon));
    double rlon = dlon * (m + flon);
    if (rlon > 180) rlon -= 360;
    if (fabs(rlon - reflon) > (dlon / 2)) return -1;
    *out_lat = rlat;
    *out_lon = rlon;
    return 0;
}

// ---- the stateless entry: lane = case ----
__global__ __launch_bounds__(kBlock) void k_cpr_cases(const mgpu_cpr_case *cases, uint64_t n, mgpu_cpr_result *out) {
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const mgpu_cpr_case c = cases[i];
    double lat = 0, lon = 0;
    int rc;
    if (c.fn == 0) rc = decodeCPRairborne(c.even_lat, c.even_lon, c.odd_lat, c.odd_lon, c.fflag, &lat, &lon);
    else if (c.fn == 1) rc = decodeCPRsurface(c.reflat, c.reflon, c.even_lat, c.even_lon, c.odd_lat, c.odd_lon, c.fflag, &lat, &lon);
    else rc = decodeCPRrelative(c.reflat, c.reflon, c.even_lat, c.even_lon, c.fflag, c.surface, &lat, &lon);
    mgpu_cpr_result r;
    r.lat = rc < 0 ? 0.0 : lat; r.lon = rc < 0 ? 0.0 : lon; r.rc = rc; r.pad = 0;
    out[i] = r;
}

// ---- inputs: one key per message, one info record per position message, the all-zero record of every other message ----
__global__ __launch_bounds__(kBlock) void k_cpr_prep(const mgpu_msg *msgs, const mgpu_fields *fields, uint64_t n, uint64_t *keys, CprInfo *info,
                                                     mgpu_position *out) {
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const mgpu_msg &m = msgs[i];
    const mgpu_fields &f = fields[i];
    const bool pos = (f.flags & MGPU_F_CPR_VALID) && (m.msgtype == 17 || m.msgtype == 18);
    CprInfo g = {0, 0, 0};
    if (pos) {
        const bool slow = (f.flags & MGPU_F_GS_VALID) && f.gs_selected <= 25;
        g.now = m.sysTimestamp;
        g.w0 = (f.cpr_lat & 0x1ffffu) | ((uint32_t) (f.cpr_type & 3u) << 17) | ((f.flags & MGPU_F_CPR_ODD) ? 1u << 19 : 0u) | (slow ? 1u << 20 : 0u) |
               ((uint32_t) f.source << 24);
        g.w1 = f.cpr_lon & 0x1ffffu;
        keys[i] = ((uint64_t) (f.addr & 0x1ffffffu) << 32) | i;
    } else {
        keys[i] = ((uint64_t) kGtAcMarker << 32) | i;                              // behind every aircraft, never walked
        mgpu_position z;
        memset(&z, 0, sizeof z);
        out[i] = z;
    }
    info[i] = g;
}

// One wave per run: rules 1-4 above for every position message of one address, 64 messages per step.
__global__ __launch_bounds__(kBlock) void k_cpr_walk(const uint64_t *keys, uint64_t n, const CprInfo *info, const uint32_t *runs, const uint32_t *nruns,
                                                     CprAc *table, mgpu_cpr_config cfg, mgpu_position *out) {
    const int lane = lane_id();
    const uint64_t lt_mask = (1ull << lane) - 1;
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = (gridDim.x * kBlock) >> 6;
    const uint32_t nr = *nruns;
    const long long air_max = cfg.airborne_max_elapsed_ms ? (long long) cfg.airborne_max_elapsed_ms : 10000;
    for (uint32_t r = wave; r < nr; r += nwaves) {
        const uint64_t k0 = runs[r];
        const uint32_t addr = (uint32_t) (keys[k0] >> 32);
        const CprAc st = table[addr];
        // carried from step to step (wave-uniform): slot [0] even, [1] odd — time, words, the message's index in this call's list
        bool s_valid[2] = {(st.valid & 1u) != 0, (st.valid & 2u) != 0};
        long long s_t[2] = {st.t_even, st.t_odd};
        uint32_t s_w0[2] = {st.even_w0, st.odd_w0}, s_w1[2] = {st.even_w1, st.odd_w1};
        uint32_t s_idx[2] = {MGPU_CPR_PARTNER_EARLIER, MGPU_CPR_PARTNER_EARLIER};
        bool g_valid = (st.valid & 4u) != 0;
        long long g_t = st.t_global;
        double g_lat = st.g_lat, g_lon = st.g_lon;
        for (uint64_t kb = k0;; kb += WAVE) {
            const uint64_t k = kb + lane;
            const uint64_t key = k < n ? keys[k] : ~0ull;
            const bool mine = (uint32_t) (key >> 32) == addr;                     // (the run is contiguous: a prefix of the lanes; ~0: behind the list)
            const int cnt = __popcll(__ballot(mine));
            if (cnt == 0) break;                                                  // (a run of a whole number of steps)
            const uint32_t idx = (uint32_t) key;
            CprInfo g = {0, 0, 0};
            if (mine) g = info[idx];
            const long long now = g.now;
            const bool odd = (g.w0 >> 19) & 1u, surface = ((g.w0 >> 17) & 3u) == 1u, slow = (g.w0 >> 20) & 1u;
            const int lat_w = (int) (g.w0 & 0x1ffffu), lon_w = (int) g.w1;
            // the last message of the other parity below this lane, else the carried slot
            const uint64_t m_par[2] = {__ballot(mine && !odd), __ballot(mine && odd)};
            const uint64_t pm = (odd ? m_par[0] : m_par[1]) & lt_mask;
            const int jp = pm ? 63 - __builtin_clzll(pm) : 0;
            const long long tp_s = __shfl(now, jp);
            const uint32_t w0p_s = __shfl(g.w0, jp), w1p_s = __shfl(g.w1, jp), idxp_s = __shfl(idx, jp);
            const bool has_p = mine && (pm != 0 || (odd ? s_valid[0] : s_valid[1]));   // (the other slot)
            const long long tp = pm ? tp_s : (odd ? s_t[0] : s_t[1]);
            const uint32_t w0p = pm ? w0p_s : (odd ? s_w0[0] : s_w0[1]), w1p = pm ? w1p_s : (odd ? s_w1[0] : s_w1[1]);
            const uint32_t idxp = pm ? idxp_s : (odd ? s_idx[0] : s_idx[1]);
            const long long max_elapsed = surface ? (slow ? 50000 : 25000) : air_max;
            const long long dt = now - tp, adt = dt < 0 ? -dt : dt;
            const bool tried = has_p && ((w0p ^ g.w0) & kCprPairMask) == 0 && adt <= max_elapsed;
            int grc = MGPU_CPR_NOT_TRIED, lrc = MGPU_CPR_NOT_TRIED;
            double lat = 0, lon = 0;
            uint32_t method = MGPU_CPR_NONE;
            if (tried) {
                const int plat = (int) (w0p & 0x1ffffu), plon = (int) w1p;
                const int elat = odd ? plat : lat_w, elon = odd ? plon : lon_w, olat = odd ? lat_w : plat, olon = odd ? lon_w : plon;
                if (surface) grc = cfg.ref_valid ? decodeCPRsurface(cfg.ref_lat, cfg.ref_lon, elat, elon, olat, olon, odd, &lat, &lon) : -1;
                else grc = decodeCPRairborne(elat, elon, olat, olon, odd, &lat, &lon);
                if (grc == 0) method = MGPU_CPR_GLOBAL;
                else { lat = 0; lon = 0; if (grc == -2) method = MGPU_CPR_BAD; }
            }
            // the last GLOBAL result below this lane, else the carried reference
            const bool gok = tried && grc == 0;
            const uint64_t mg = __ballot(gok), pg = mg & lt_mask;
            const int jg = pg ? 63 - __builtin_clzll(pg) : 0;
            const long long tg_s = __shfl(now, jg);
            const double rlat_s = __shfl(lat, jg), rlon_s = __shfl(lon, jg);
            if (mine && method == MGPU_CPR_NONE) {
                const bool has_g = pg != 0 || g_valid;
                const long long tg = pg ? tg_s : g_t;
                const double rlat = pg ? rlat_s : g_lat, rlon = pg ? rlon_s : g_lon;
                if (has_g && now < tg + kCprLocalTtl) {
                    lrc = decodeCPRrelative(rlat, rlon, lat_w, lon_w, odd, surface, &lat, &lon);
                    if (lrc == 0) method = MGPU_CPR_LOCAL_AIRCRAFT;
                } else if (!surface && cfg.ref_valid) {
                    lrc = decodeCPRrelative(cfg.ref_lat, cfg.ref_lon, lat_w, lon_w, odd, surface, &lat, &lon);
                    if (lrc == 0) method = MGPU_CPR_LOCAL_RECEIVER;
                }
                if (lrc != 0) { lat = 0; lon = 0; }
            }
            if (mine) {
                mgpu_position p;
                memset(&p, 0, sizeof p);
                p.lat = lat; p.lon = lon;
                p.partner = tried ? idxp : MGPU_CPR_PARTNER_NONE;
                p.partner_dt_ms = tried ? (int32_t) dt : 0;                       // (|dt| <= max_elapsed)
                p.global_result = (int8_t) grc; p.local_result = (int8_t) lrc;
                p.method = (uint8_t) method;
                p.flags = (uint8_t) ((odd ? 1u : 0u) | (surface ? 2u : 0u));
                out[idx] = p;
            }
            // the carries: the step's last even / odd message, its last GLOBAL result
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (m_par[q]) {
                    const int jl = 63 - __builtin_clzll(m_par[q]);
                    s_valid[q] = true;
                    s_t[q] = __shfl(now, jl); s_w0[q] = __shfl(g.w0, jl); s_w1[q] = __shfl(g.w1, jl); s_idx[q] = __shfl(idx, jl);
                }
            }
            if (mg) {
                const int jl = 63 - __builtin_clzll(mg);
                g_valid = true;
                g_t = __shfl(now, jl); g_lat = __shfl(lat, jl); g_lon = __shfl(lon, jl);
            }
            if (cnt < WAVE) break;
        }
        if (lane == 0) {
            CprAc o;
            o.t_even = s_t[0]; o.t_odd = s_t[1]; o.t_global = g_t; o.g_lat = g_lat; o.g_lon = g_lon;
            o.even_w0 = s_w0[0]; o.even_w1 = s_w1[0]; o.odd_w0 = s_w0[1]; o.odd_w1 = s_w1[1];
            o.valid = (s_valid[0] ? 1u : 0u) | (s_valid[1] ? 2u : 0u) | (g_valid ? 4u : 0u); o.pad = 0;
            table[addr] = o;
        }
    }
}

size_t cpr_table_bytes() { return ((size_t) 1 << 25) * sizeof(CprAc) + sizeof(CprAc) * 2; }
size_t cpr_scratch_bytes(uint64_t n) {       // keys x 2, info, runs, hist + counter
    return (size_t) n * (8 + 8 + sizeof(CprInfo) + 4) + (size_t) (256 * kGtWaves + 64) * 4 + 256;
}

// msgs / fields / out in device memory; scratch = cpr_scratch_bytes(n), table = cpr_table_bytes() (zeroed once)
void launch_cpr_track(const mgpu_msg *msgs, const mgpu_fields *fields, uint64_t n, const mgpu_cpr_config &cfg, void *table, void *scratch,
                      mgpu_position *out, hipStream_t s) {
    if (!n) return;
    uint8_t *p = (uint8_t *) scratch;
    uint64_t *keys_a = (uint64_t *) p; p += (size_t) n * 8;
    uint64_t *keys_b = (uint64_t *) p; p += (size_t) n * 8;
    CprInfo *info = (CprInfo *) p; p += (size_t) n * sizeof(CprInfo);
    uint32_t *runs = (uint32_t *) p; p += (size_t) n * 4;
    uint32_t *hist = (uint32_t *) p; p += (size_t) 256 * kGtWaves * 4;
    uint32_t *nruns = (uint32_t *) p;
    const unsigned blocks = (unsigned) ((n + kBlock - 1) / kBlock);
    (void) hipMemsetAsync(nruns, 0, 4, s);
    hipLaunchKernelGGL(k_cpr_prep, dim3(blocks), dim3(kBlock), 0, s, msgs, fields, n, keys_a, info, out);
    uint64_t *src = keys_a, *dst = keys_b;
    for (int shift = 32; shift < 64; shift += 8) {                                 // the gate's sort: 26 address bits, 4 digits
        hipLaunchKernelGGL(k_gate_hist, dim3(kGtBlocks), dim3(kBlock), 0, s, src, n, shift, hist);
        hipLaunchKernelGGL(k_gate_scan, dim3(1), dim3(kBlock), 0, s, hist);
        hipLaunchKernelGGL(k_gate_scatter, dim3(kGtBlocks), dim3(kBlock), 0, s, src, n, shift, hist, dst);
        uint64_t *t = src; src = dst; dst = t;
    }
    hipLaunchKernelGGL(k_gate_runs, dim3(blocks), dim3(kBlock), 0, s, src, n, runs, nruns);
    const unsigned wblocks = blocks < 1024u ? blocks : 1024u;
    hipLaunchKernelGGL(k_cpr_walk, dim3(wblocks), dim3(kBlock), 0, s, src, n, info, runs, nruns, (CprAc *) table, cfg, out);
}

void launch_cpr_cases(const mgpu_cpr_case *cases, uint64_t n, mgpu_cpr_result *out, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_cpr_cases, dim3((unsigned) ((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, cases, n, out);
}
