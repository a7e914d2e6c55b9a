// kernels/slice.inc — k_slice (generation 7): PPM slicer, CRC-24 and scoring over k_sweep's candidate lists.
// Part of the single translation unit kernels.hip (included inside namespace mgpu, after the parts before it).

// ---------------------------------------------------------------------------------------------
// k_slice: slice_byte / score_phase / scoreModesMessage / modesChecksum / modesChecksumDiagnose
// (demod_2400.c:133-258, mode_s.c:276-419, crc.c:67-82,383-406) for the candidates k_sweep found.
//
// Every wave is autonomous (no workgroup barrier after the table preload): it takes tiles of kSlTile positions from a dealer
// (below), one record chain per tile, holds a tile + 304 samples of look-ahead in wave-private LDS (prefetched into registers
// while the previous tile is sliced, together with the heads of the next tile's candidate lists), and per tile:
//   candidates -> (position, phase) pairs -> DF stage (lane = pair: frame bits 0..4; 5 of 8 pairs end here,
//   valid_df_*_bitset, demod_2400.c:223-238) -> ring of valid pairs -> slicing rounds -> sliced frames.
// Slicing round: the waiting frames (at most 32) get L = 2, 3, 4, 5, 6, 8, 11 or 22 lanes each — the most they leave room for —,
// a lane slices I = ceil(22 / L) consecutive groups of five bits of a 112-bit frame (ceil(11 / L) of a 56-bit one) out of
// per-group windows with per-lane coefficients (slicer.inc), ORs its bits into the frame's words in LDS and XORs its partial
// CRC syndrome in (CRC-24 is GF(2)-linear: the syndrome is the XOR of per-group table entries).
// Scoring is deferred: sliced frames wait in a 64-entry LDS buffer, across tiles, and are scored one frame per lane when the
// next round would not fit; records go from registers straight into the wave's reserved slice of the pool, one segment per
// tile touched.
// What bounds the kernel is instruction issue — every instruction, scalar ones included (DESIGN.md §3) — so the tile loop is
// written for few of them: consecutive ifs instead of a state machine, predicates instead of branches on the format.
// ---------------------------------------------------------------------------------------------
constexpr int kSlTile = 2048;                                // positions per tile
constexpr int kSlLists = kSlTile / kSweepTile;               // k_sweep's candidate lists per tile (1 or 2)
static_assert(kSlLists == 1 || kSlLists == 2, "k_slice reads one or two candidate lists per tile");
constexpr int kSlChunks = (kSlTile + kHalo) / 8;             // 16-byte chunks per tile (294)
constexpr int kSlPre = (kSlChunks + WAVE - 1) / WAVE;        // 16-byte loads per lane and tile (5)
constexpr int kSlTilesPerUnit = kUnit / kSlTile;
constexpr int kSlVCap = 128;                                 // ring of valid pairs (power of two)
constexpr int kSlRound = 32;                                 // frames looked at per slicing round
constexpr int kSlFrameCap = WAVE;                            // sliced frames waiting for the scoring pass
constexpr int kSlPartWords = 8;                              // per-workgroup row of counts (5 used)
// The dealer.  The slicer's work per tile follows the traffic (7 frames per 8192 positions on average, Poisson), and the waves of
// a SIMD do not run at one speed (VALU issue goes by age): with a fixed share of tiles per wave the kernel waited for its
// unluckiest, slowest wave — waves alive 63 % of the kernel (profiles/r02_pmc_sq_summary.txt).  Now a wave takes half its
// expected share without asking and the rest one tile at a time from its pool's counter (kSlPools pools, workgroup b in pool
// b mod kSlPools, so every pool mixes early- and late-launched workgroups; a pool = a contiguous range of tiles).  A returning
// device atomic costs ~11 ns, serialised per 64-byte LINE (tools/micro/atomic_cost.hip: 64 counters in four lines made this kernel
// 30 % slower than no dealer at all): the counters sit 256 bytes apart and see ~256 requests each per launch.
constexpr int kSlPools = kDealerCounters;
static_assert(kSweepMaxBlocks * kSlPartWords <= kSweepGridMax * 4, "the rows fit the slot's partial-count buffer");

struct SliceLds {                                            // wave-private LDS, 16-byte aligned members first
    uint16_t mag[kSlTile + kHalo + 8];                       // 4720 B
    SlicedFrame frames[kSlFrameCap];                         // 2048 B
    uint32_t v[kSlVCap];                                     //  512 B  pos_local << 3 | phase - 4 | df << 16
    uint16_t pairs[WAVE * 5];                                //  640 B
};

__global__ __launch_bounds__(kBlock, 3) void k_slice(SweepParams p) {
    __shared__ __attribute__((aligned(16))) SliceLds s_w[kBlock / WAVE];
    __shared__ uint32_t s_gsyn[(kGroupsLong + kGroupsShort) * 32];
    __shared__ uint32_t s_acache[kWAdderCache];
    __shared__ uint32_t s_rt[kSlRound + 1];                  // the slicing rounds' lane deal per number of waiting frames (round_table_row)
    __shared__ uint32_t s_geom[10];                          // slicer geometry per try-phase (geom_table_row): the DF stage
    __shared__ __attribute__((aligned(16))) uint32_t s_wc[kWcRows * kWcRowWords];   // the slicing rounds' per-lane constants (wcoef_table_row)
    __shared__ unsigned long long s_cnt[8];
    extern __shared__ uint32_t s_keys[];   // the two syndrome tables' keys, two levels each (slicer.inc: key_tables)

    const int tid = threadIdx.x, lane = lane_id();
    const int wv = (int) rfl((uint32_t) tid >> 6);
    for (int i = tid; i < (kGroupsLong + kGroupsShort) * 32; i += kBlock) s_gsyn[i] = p.group_syndrome[i];
    for (int i = tid; i < kWAdderCache; i += kBlock) s_acache[i] = 0xFFFFFFFFu;
    key_tables_preload(s_keys, p.tab_long, p.n_long, p.tab_short, p.n_short, tid);
    if (tid < 8) s_cnt[tid] = 0;
    if (tid < 5) geom_table_row(4 + tid, s_geom[2 * tid], s_geom[2 * tid + 1]);
    if (tid >= 2 * WAVE && tid <= 2 * WAVE + kSlRound) s_rt[tid - 2 * WAVE] = round_table_row(tid - 2 * WAVE);
    if (tid >= WAVE && tid < WAVE + kWcRows) wcoef_table_row(tid - WAVE, s_wc + (tid - WAVE) * kWcRowWords);
    __syncthreads();   // the only workgroup barrier before the final counter reduction
    SliceLds &L = s_w[wv];
    const uint32_t *w32 = (const uint32_t *) L.mag;
    const uint64_t lt_mask = (1ull << lane) - 1;
#if MGPU_EXPERIMENTS
    const int dbg = p.debug_stage;      // MGPU_DEBUG_STAGE: timing experiments that leave work out (results are wrong), tools/slice_stages.sh
#define SL_EXP(k) (dbg == (k))
#else
#define SL_EXP(k) false
#endif
    const uint32_t wave_global = blockIdx.x * (kBlock / WAVE) + wv;
    const uint32_t nwaves = gridDim.x * (kBlock / WAVE);

    uint32_t n_rec = 0;
    uint32_t n_cand = 0, n_ph0 = 0, n_ph1 = 0, n_ph2 = 0;   // candidates / with phases 4-5, 6-7, 8 tried: k_sweep leaves the counting to the kernel that reads every code
    // wave-uniform: reserved pool space.  The first slice is the wave's by position — a returning atomic on the shared
    // cursor costs ~11 ns serialised, and every wave of the grid asks for its first slice within the same few microseconds
    uint32_t chunk_base = wave_global * (uint32_t) kPoolChunkRecords, chunk_left = kPoolChunkRecords;
    // chain of the unit whose records are being written (frames wait across units: a pass may close one chain and open the next)
    uint32_t cur_unit = kNone, prev_hdr = kNone;
    bool prev_first = false;                                 // ... whether that segment is the chain's first
    uint32_t prev_cnt = 0, prev_end = 0;                     // ... the records in that chain's last segment, and the pool index behind them
    int fcount = 0;                                          // sliced frames waiting in L.frames (wave-uniform)
    u32x4 pre[kSlPre];
    uint32_t pre_code = 0, pre_count = 0, pre_code2 = 0, pre_count2 = 0;   // (second list: kSlLists == 2)
    bool have_pre = false;

    // Scoring pass over the waiting frames, lane = frame: CRC classification, class planes, adder bitmap, and the
    // records go straight from registers into the wave's slice of the pool, one segment per unit.
    auto score_pass = [&]() __attribute__((always_inline)) {
        if (fcount == 0) return;
        if (SL_EXP(1)) { fcount = 0; return; }
        bool emit = false;
        u32x4 ra = {0, 0, 0, 0}, rb = {0, 0, 0, 0};
        uint32_t funit = 0;
        if (lane < fcount) {
            const u32x4 f0 = *(const u32x4 *) &L.frames[lane].W[0];
            const u32x4 f1 = *(const u32x4 *) &L.frames[lane].synd;
            uint32_t flags = 0, addr = 0;
            emit = classify_frame(p, s_gsyn, s_keys, f0.x, f0.y, f0.z, f0.w, f1.x, f1.y & 0xffu, (int) (f1.y >> 8), f1.z,
                                  ra, rb, flags, addr);
            if (emit) {
                const uint32_t gpos = f1.z;
                funit = gpos / (uint32_t) kSlTile;                  // one record chain per tile
                // (the class bitmap — which positions have records, all of them conditional — is built by the count pass, from the records)
                if (flags & REC_ADDER) adder_publish<kWAdderCache>(p.adder_bitmap, s_acache, addr);
            }
        }
        uint64_t todo = __ballot(emit);
        // (Measured and dropped, round 5: the segments' offsets by lanes — two ballots (who emits, who begins a tile), 64-bit masks and
        // popcounts per lane — instead of this loop: 0.8 M fewer scalar, 1.5 M more vector instructions per launch, the kernel as long
        // as before, gpurun r05aj.  The loop runs ~3 times per pass; its scalar code is cheaper than the masks.)
        while (todo) {                                       // frames are in stream order: one run of lanes per unit
            const uint32_t u = (uint32_t) __builtin_amdgcn_readlane((int) funit, __ffsll((unsigned long long) todo) - 1);
            const uint64_t em = __ballot(emit && funit == u);
            todo &= ~em;
            const int cnt = __popcll(em);
            if (u != cur_unit) {
                cur_unit = u; prev_hdr = kNone;
            }
            // The tile's records so far are the segment this wave wrote last (a scoring pass ended in the middle of the tile): the new ones
            // go right behind them, into the same segment, while it stays within 64 records (the post-sweep passes keep a segment's
            // decisions in a 64-bit mask) — those passes walk a tile's segments one dependent round trip after the other.
            if (prev_hdr != kNone && prev_end == chunk_base && prev_cnt + (uint32_t) cnt <= (uint32_t) WAVE && chunk_left >= (uint32_t) cnt) {
                const uint32_t at = chunk_base;
                chunk_base += (uint32_t) cnt;
                chunk_left -= (uint32_t) cnt;
                if (emit && funit == u && !SL_EXP(3)) {
                    u32x4 *d = (u32x4 *) &p.pool[at + __popcll(em & lt_mask)];
                    d[0] = ra; d[1] = rb;
                }
                prev_cnt += (uint32_t) cnt;
                if (lane == 0) { p.pool[prev_hdr].pos = prev_cnt; if (prev_first) p.unit_count[u] = prev_cnt; }
                prev_end = chunk_base;
                n_rec += cnt;
                continue;
            }
            if (chunk_left < (uint32_t) cnt + 1u) {
                uint32_t b = 0;
                if (lane == 0) b = atomicAdd(p.pool_used, (uint32_t) kPoolChunkRecords);
                chunk_base = nwaves * (uint32_t) kPoolChunkRecords + rfl(b);     // the cursor counts from behind the waves' first slices
                chunk_left = kPoolChunkRecords;
            }
            const uint32_t base = chunk_base;
            chunk_base += (uint32_t) cnt + 1u;
            chunk_left -= (uint32_t) cnt + 1u;
            if ((uint64_t) base + kPoolChunkRecords <= p.pool_cap) {
                if (emit && funit == u && !SL_EXP(3)) {
                    u32x4 *d = (u32x4 *) &p.pool[base + 1 + __popcll(em & lt_mask)];
                    d[0] = ra; d[1] = rb;
                }
                if (lane == 0) {
                    u32x4 h0 = {(uint32_t) cnt, 0xFFu, 0u, kNone}, h1 = {0, 0, 0, 0};
                    u32x4 *hd = (u32x4 *) &p.pool[base];
                    hd[0] = h0; hd[1] = h1;
                    // (unit_count: the records in the chain's first segment — the count pass loads exactly those together with the header)
                    if (prev_hdr == kNone) { p.unit_first[u] = base; p.unit_count[u] = (uint32_t) cnt; } else p.pool[prev_hdr].addr = base;
                }
                prev_first = prev_hdr == kNone;
                prev_hdr = base;
                prev_cnt = (uint32_t) cnt;
                prev_end = chunk_base;
                n_rec += cnt;
            } else if (lane == 0) {
                atomicAdd(&p.counters[CNT_POOL_OVERFLOW], 1ull);
            }
        }
        fcount = 0;
        WAVE_SYNC();
    };

    // ---- the wave's tiles: a static share first, then whatever it can take from its pool (see the dealer above) ----
    const uint32_t ntiles = (uint32_t) ((p.n + kSlTile - 1) / kSlTile);
    const uint32_t npools = gridDim.x < (uint32_t) kSlPools ? gridDim.x : (uint32_t) kSlPools;
    const uint32_t pool = blockIdx.x % npools;
    const uint32_t pool_blocks = (gridDim.x - pool + npools - 1) / npools;                 // workgroups b = pool, pool + npools, ...
    const uint32_t pool_waves = pool_blocks * (kBlock / WAVE), wave_in_pool = (blockIdx.x / npools) * (kBlock / WAVE) + (uint32_t) wv;
    const uint32_t t_lo = (uint32_t) ((uint64_t) ntiles * pool / npools), t_hi = (uint32_t) ((uint64_t) ntiles * (pool + 1) / npools);
    const uint32_t n_static = (t_hi - t_lo) / pool_waves / 2u;                            // tiles every wave of the pool takes without asking
    const uint32_t t_dyn = t_lo + n_static * pool_waves;                                  // the pool's first dealt tile
    uint32_t static_left = n_static, static_next = t_lo + wave_in_pool * n_static;
    // asking = one returning atomic from lane 0 (deal_ask, kernels.hip); the request for the tile after next goes out at the start of a
    // tile and its answer is read at the end of the same tile, into a variable of that iteration (read at once it would be waited
    // for at once: a memory round trip per tile).  The first two tiles are asked for one after the other, with the wait.
    uint32_t *const deal = &p.dealer[pool * (uint32_t) kDealerStride];
    const uint32_t deal_zero = deal_opaque_zero();
    auto next_tile_sync = [&]() __attribute__((always_inline)) -> uint32_t {
        if (static_left) { --static_left; return static_next++; }
        uint32_t t0 = 0;
        if (lane == 0) t0 = deal_ask(deal, deal_zero);
        const uint32_t t = t_dyn + rfl(t0);
        return t < t_hi ? t : kNone;
    };
    uint32_t cur_tile = next_tile_sync();
    uint32_t nxt_tile = cur_tile != kNone ? next_tile_sync() : kNone;

    while (cur_tile != kNone) {
        {
            const bool more = nxt_tile != kNone;
            const bool asking = more && static_left == 0;    // for the tile after next: answered at the end of this tile
            uint32_t ticket;                                 // (declared HERE: see deal_ask)
            if (asking && lane == 0) ticket = deal_ask(deal, deal_zero);
            if (lane == 0) p.unit_first[cur_tile] = kNone;
            // (the post-sweep passes walk a unit's kUnit / kSlTile chains: the last unit's chains behind the last tile are empty)
            if (cur_tile == ntiles - 1 && lane >= 1 && lane < kUnit / kSlTile && ((cur_tile + (uint32_t) lane) & (uint32_t) (kUnit / kSlTile - 1)) > (cur_tile & (uint32_t) (kUnit / kSlTile - 1)))
                p.unit_first[cur_tile + (uint32_t) lane] = kNone;
            const uint64_t D0 = (uint64_t) cur_tile * kSlTile;
            const uint32_t tidx = cur_tile * (uint32_t) kSlLists;                                    // index of the tile's first list
            // ---- tile into LDS (prefetched while the previous tile was sliced) ----
            if (!have_pre) {
#pragma unroll
                for (int k = 0; k < kSlPre; ++k) pre[k] = *(const u32x4 *) &p.mag[D0 + 8 * (lane + k * WAVE)];
                pre_count = p.cand_count[tidx];
                pre_code = p.cand[D0 + lane];
                if (kSlLists == 2) { pre_count2 = p.cand_count[tidx + 1]; pre_code2 = p.cand[D0 + kSweepTile + lane]; }
            }
#pragma unroll
            for (int k = 0; k < kSlPre; ++k) {
                const int i = lane + k * WAVE;
                if (i < kSlChunks) {   // the tile holds the samples with the top bit flipped: see THE BIAS ARITHMETIC, slicer.inc
                    const u32x4 v = {pre[k].x ^ 0x80008000u, pre[k].y ^ 0x80008000u, pre[k].z ^ 0x80008000u, pre[k].w ^ 0x80008000u};
                    *(u32x4 *) &L.mag[8 * i] = v;
                }
            }
            // the tile's candidates = its lists one after the other (codes carry the position in the unit, so nothing else changes)
            const int ccountA = (int) rfl(pre_count), ccount = ccountA + (kSlLists == 2 ? (int) rfl(pre_count2) : 0);
            const uint32_t first_code = pre_code, first_code2 = pre_code2;
            n_cand += (uint32_t) ccount;
            {
                const uint64_t Dn = (uint64_t) nxt_tile * kSlTile;
                const uint32_t tn = nxt_tile * (uint32_t) kSlLists;
                have_pre = nxt_tile != kNone;
                if (have_pre) {
#pragma unroll
                    // every lane issues all kSlPre loads (d_mag has the slack): with a fixed number of loads in flight the wait for
                    // the CURRENT tile's candidate codes below is an exact s_waitcnt vmcnt(N), not a wait for this prefetch
                    for (int k = 0; k < kSlPre; ++k) pre[k] = *(const u32x4 *) &p.mag[Dn + 8 * (lane + k * WAVE)];
                    pre_count = p.cand_count[tn];
                    pre_code = p.cand[Dn + lane];
                    if (kSlLists == 2) { pre_count2 = p.cand_count[tn + 1]; pre_code2 = p.cand[Dn + kSweepTile + lane]; }
                }
            }
            WAVE_SYNC();

            int vhead = 0, vcount = 0;

            // ---- one slicing round over the first (up to kSlRound) frames of the ring ----
            // Lanes per frame = 2, 3, 4, 5, 6, 8, 11 or 22 — the most the waiting frames leave room for (L = 64 / frames, rounded down to
            // the next value at which the groups per lane I = ceil(22 / L) change) —, frame = lane / L, part = the rest: no scan, no
            // lane map; I, L and the reciprocal of L come from a 33-word table (round_table_row).  (Until round 5 powers of two only:
            // nine to sixteen frames — the usual tile — took six steps where 9-10 take four and 11-12 five now.  Generation 5 dealt
            // the lanes in proportion to the frames' lengths, I groups per lane for the smallest I that fits: two wave scans, a map
            // through the LDS and ~170 instructions per round — as much as the slicing itself once a group cost 32 instructions
            // instead of 48 — and at most 16 long frames per round.)
            auto slice_round = [&]() __attribute__((always_inline)) {
                const int navail = vcount < kSlRound ? vcount : kSlRound;
                const uint32_t rt = rfl(s_rt[navail]);
                const int I = (int) (rt & 15u);                                 // groups per lane of a 112-bit frame
                const int Is = (int) ((rt >> 4) & 15u);                         //                    56-bit
                const int Lf = (int) ((rt >> 8) & 31u);                         // lanes per frame
                const int f = (int) (((uint32_t) lane * (rt >> 16)) >> 16), j = lane - f * Lf;
                if (f < navail) {
                    const uint32_t e2 = L.v[(vhead + f) & (kSlVCap - 1)];
                    const uint32_t df = e2 >> 16;
                    const bool is_long = (p.valid_long >> df) & 1;
                    SlicedFrame &fr = L.frames[fcount + f];
                    if (j == 0) {          // (this wave's LDS operations execute in order: the header is there before any part ORs into it)
                        const u32x4 f0 = {df << 27, 0u, 0u, 0u};
                        const u32x4 f1 = {s_gsyn[(is_long ? 0 : kGroupsLong * 32) + df], df | ((4u + (e2 & 7u)) << 8),
                                          (uint32_t) (D0 + ((e2 & 0xffffu) >> 3)), 0u};
                        *(u32x4 *) &fr.W[0] = f0;
                        *(u32x4 *) &fr.synd = f1;
                    }
                    const int If = is_long ? I : Is;
                    const int g0 = 1 + If * j;                                  // this lane's groups: g0 .. g0 + ng - 1 of 1..22 (1..11)
                    int ng = (is_long ? 23 : 12) - g0;
                    if (ng > If) ng = If;
                    if (ng > 0 && !SL_EXP(2)) {
                        SliceWin W;
                        make_win(s_wc, w32, (int) ((e2 & 0xffffu) >> 3), (int) (e2 & 7u), g0, W);   // from the lane's first group on
                        const uint32_t *gs = s_gsyn + (is_long ? 0 : kGroupsLong * 32) + g0 * 32;
                        uint32_t chunkA = 0, chunkB = 0, psyn = 0;               // groups 0..5 and 6..10 of the lane
                        uint32_t tsyn = 0;      // the table entry of the previous group: XORed in one group late, so that its LDS round
                                                // trip runs under the next group's loads instead of ending every iteration with a wait
                        // The lane's dwords pass through a ring of 13 registers: group k's window is R[6k .. 6k + 6 (mod 13)], its last
                        // dword the next group's first, and the six new dwords of group k + 1 are requested before group k's arithmetic
                        // (they land in the six registers group k does not use).  Unrolled by hand: every index is a constant.
                        uint32_t R[13];
                        R[0] = W.pw[0]; R[1] = W.pw[1]; R[2] = W.pw[2]; R[3] = W.pw[3]; R[4] = W.pw[4]; R[5] = W.pw[5]; R[6] = W.pw[6];
#define SL_R(k, j) R[(6 * (k) + (j)) % 13]
#define SL_GROUP(k) \
                        if ((k) >= I) goto groups_done; \
                        if ((k) < ng) { \
                            SL_R(k, 7) = W.pw[6 * (k) + 7]; SL_R(k, 8) = W.pw[6 * (k) + 8]; SL_R(k, 9) = W.pw[6 * (k) + 9]; \
                            SL_R(k, 10) = W.pw[6 * (k) + 10]; SL_R(k, 11) = W.pw[6 * (k) + 11]; SL_R(k, 12) = W.pw[6 * (k) + 12]; \
                            __builtin_amdgcn_sched_barrier(0);          /* keep the requests above, the arithmetic below */ \
                            const uint32_t grp = win_group(SL_R(k, 0), SL_R(k, 1), SL_R(k, 2), SL_R(k, 3), SL_R(k, 4), SL_R(k, 5), SL_R(k, 6), W); \
                            /* (groups 22 and 11 reach past the end of the frame: the table ignores those bits, classify_frame drops them; \
                               the requests behind a lane's last group stay inside the tile's slack) */ \
                            psyn ^= tsyn; \
                            tsyn = gs[(k) * 32 + grp]; \
                            if ((k) < 6) chunkA = (chunkA << 5) | grp; else chunkB = (chunkB << 5) | grp; \
                        }
                        SL_GROUP(0) SL_GROUP(1) SL_GROUP(2) SL_GROUP(3) SL_GROUP(4) SL_GROUP(5)
                        SL_GROUP(6) SL_GROUP(7) SL_GROUP(8) SL_GROUP(9) SL_GROUP(10)
#undef SL_GROUP
#undef SL_R
                    groups_done:
                        // 5 n bits (n <= 6) that are frame bits o .. o + 5 n - 1 (bit 0 = MSB of W[0]): they touch at most two words
                        auto put = [&](uint32_t chunk, int n, int o) __attribute__((always_inline)) {
                            const uint64_t v64 = (uint64_t) chunk << (64 - 5 * n - (o & 31));
                            const uint32_t hi = (uint32_t) (v64 >> 32), lo = (uint32_t) v64;
                            if (hi) __hip_atomic_fetch_or(&fr.W[o >> 5], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (lo) __hip_atomic_fetch_or(&fr.W[(o >> 5) + 1], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        };
                        psyn ^= tsyn;
                        put(chunkA, ng < 6 ? ng : 6, 5 * g0);
                        if (I > 6 && ng > 6) put(chunkB, ng - 6, 5 * (g0 + 6));
                        __hip_atomic_fetch_xor(&fr.synd, psyn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                fcount += navail;
                vhead += navail;
                vcount -= navail;
                WAVE_SYNC();
            };

            // ---- candidates -> pairs -> DF stage -> ring -> slicing rounds.  One iteration = (the next 64 candidates' pairs, when the
            //      last ones are used up) + one DF pass + whatever rounds are due, in that order and as plain consecutive ifs: the
            //      slicing round and the scoring pass are instantiated once (their code is most of the kernel; four inlined copies of
            //      the scoring pass did not fit the instruction cache), and the usual tile — one batch of candidates, one DF pass, one
            //      round — is ONE trip.  (Until round 5 a loop that did one of the three things per trip and `continue`d: the
            //      compiler's state machine for it — a dozen scalar compares and as many copies per trip, four trips per tile — was
            //      a fifth of the kernel's scalar instructions, profiles/r05_slice_stage_pmc.txt.) ----
            int c0 = 0, a0 = 0, npairs = 0;
            bool exhausted = ccount == 0 || SL_EXP(5);
            while (!exhausted) {
                if (a0 >= npairs) {                          // next 64 candidates -> their (position, phase) pairs
                    const int ci = c0 + lane;
                    uint32_t code = 0;
                    if (kSlLists == 1) {
                        if (ci < ccount) code = c0 == 0 ? first_code : (uint32_t) p.cand[D0 + ci];
                    } else {
                        // list A's candidates, then list B's: the first 64 of each were prefetched (B's sit in the lanes they were
                        // loaded by: one bpermute brings B[ci - ccountA] over)
                        const int ib = ci - ccountA;
                        const uint32_t fromB = (uint32_t) __shfl((int) first_code2, ib & (WAVE - 1));
                        if (ci < ccountA) code = ci < WAVE ? first_code : (uint32_t) p.cand[D0 + ci];
                        else if (ci < ccount) code = ib < WAVE ? fromB : (uint32_t) p.cand[D0 + kSweepTile + ib];
                    }
                    const uint32_t mask = code & 7u;
                    n_ph0 += __popcll(__ballot(mask & 1u));
                    n_ph1 += __popcll(__ballot(mask & 2u));
                    n_ph2 += __popcll(__ballot(mask & 4u));
                    const int np = 2 * (int) (mask & 1u) + (int) (mask & 2u) + (int) ((mask >> 2) & 1u);
                    int off = wave_incl_scan_dpp(np, npairs) - np;
                    const uint32_t pl = code & (uint32_t) (((kSlTile - 1) << 3));     // position in the tile << 3
                    if (mask & 1u) { L.pairs[off++] = (uint16_t) (pl | 0u); L.pairs[off++] = (uint16_t) (pl | 1u); }
                    if (mask & 2u) { L.pairs[off++] = (uint16_t) (pl | 2u); L.pairs[off++] = (uint16_t) (pl | 3u); }
                    if (mask & 4u) { L.pairs[off++] = (uint16_t) (pl | 4u); }
                    c0 += WAVE;
                    a0 = 0;
                    WAVE_SYNC();
                }
                if (a0 < npairs) {                           // DF stage, lane = pair
                    const int j = a0 + lane;
                    bool valid = false;
                    uint32_t entry = 0;
                    if (j < npairs && !SL_EXP(6)) {
                        const uint32_t pc = L.pairs[j];
                        // (the window form of the slicing rounds here too — 28 VALU instead of 58 per pass, five 16-byte table reads more —
                        // measured equal: k_slice 129.2 / 129.1 against 130.5 / 129.3 us, gpurun r05g)
                        SliceGeomR g;
                        make_geom_tab(s_geom, w32, (int) (pc >> 3), (int) (pc & 7u), 0, g);
                        const SliceCoef K = slice_coef();           // (six v_mov per pass: cheaper than six registers held through the slicing rounds)
                        const uint32_t df = slice_group_rot(g, 0, K);
                        valid = ((p.valid_long | p.valid_short) >> df) & 1;
                        entry = pc | (df << 16);
                    }
                    const uint64_t vm = __ballot(valid);
                    if (valid) L.v[(vhead + vcount + __popcll(vm & lt_mask)) & (kSlVCap - 1)] = entry;
                    vcount += __popcll(vm);
                    a0 += WAVE;
                    WAVE_SYNC();
                }
                exhausted = a0 >= npairs && c0 >= ccount;
                while (vcount >= kSlRound || (exhausted && vcount > 0)) {
                    // frames wait across tiles and units.  (A pass forced BEFORE a tile's first round once the buffer is 32 / 40 / 48 full — so
                    // that passes end between tiles and no tile's records are split over two segments: no effect on the post-sweep
                    // passes, 0.22 ms per step either way, gpurun r05af — a split tile's second part already lands behind the first.)
                    if (fcount + (vcount < kSlRound ? vcount : kSlRound) > kSlFrameCap) score_pass();
                    slice_round();
                }
            }
            cur_tile = nxt_tile;
            if (!more) nxt_tile = kNone;
            else if (!asking) { --static_left; nxt_tile = static_next++; }
            else { const uint32_t t = t_dyn + rfl(ticket); nxt_tile = t < t_hi ? t : kNone; }
        }
    }
    score_pass();
    if (lane == 0) {
        atomicAdd(&s_cnt[0], (unsigned long long) n_rec);
        atomicAdd(&s_cnt[1], (unsigned long long) n_cand);
        atomicAdd(&s_cnt[2], (unsigned long long) n_ph0);
        atomicAdd(&s_cnt[3], (unsigned long long) n_ph1);
        atomicAdd(&s_cnt[4], (unsigned long long) n_ph2);
    }
    __syncthreads();
    // one row of counts per workgroup (records, candidates, phases 4/5, 6/7, 8), summed by k_prescreen_write's first workgroup:
    // a thousand device atomics on five words at the end of the kernel would serialise at the memory side (tools/micro/atomic_cost.hip)
    if (tid < kSlPartWords) p.sweep_part[blockIdx.x * kSlPartWords + tid] = (uint32_t) s_cnt[tid];
}

// persistent grid = the workgroups resident at once (occupancy x CUs) for this much dynamic LDS
// (the 2-bit syndrome keys of --aggressive take 12 KB: three workgroups per CU instead of four)
unsigned launch_slice(const SweepParams &p, hipStream_t s) {   // returns its grid size = rows of p.sweep_part written
    if (p.nunits == 0) return 0;
    const size_t dyn = ((size_t) p.n_long + p.n_short + 2 * (kKeyBuckets + 1) + 8) / 2 * sizeof(uint32_t);   // halfwords (slicer.inc: key_tables), rounded up to words
    // (per device and table size; two contexts racing here compute the same value twice)
    static std::atomic<uint64_t> cache[64];                  // dyn << 32 | grid
    int dev = 0;
    (void) hipGetDevice(&dev);
    uint64_t e = cache[dev & 63].load(std::memory_order_relaxed);
    if ((uint32_t) e == 0 || (e >> 32) != (uint64_t) dyn) {
        e = ((uint64_t) dyn << 32) | resident_grid((const void *) k_slice, dyn, kSweepMaxBlocks);
        cache[dev & 63].store(e, std::memory_order_relaxed);
    }
    const unsigned cached = (uint32_t) e;
    const unsigned ntiles = (unsigned) ((p.n + kSlTile - 1) / kSlTile);
    const unsigned want = (ntiles + (kBlock / WAVE) - 1) / (kBlock / WAVE);   // at least one tile per wave
    const unsigned blocks = want < cached ? want : cached;
    hipLaunchKernelGGL(k_slice, dim3(blocks), dim3(kBlock), dyn, s, p);
    return blocks;
}
