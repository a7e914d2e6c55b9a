// kernels/sweep.inc — k_sweep (generation 7), the preamble sweep: the kernel the HBM roofline applies to.
// Part of the single translation unit kernels.hip (included inside namespace mgpu, after the parts before it).

// ---------------------------------------------------------------------------------------------
// k_sweep: demodulate2400's scan over every sample position (demod_2400.c:290-378) and nothing else —
// 2 bytes per position in, one u16 code per candidate (~1 % of positions) out.  The slicer, the CRC and
// the scoring live in k_slice (kernels/slice.inc), which walks the candidate lists this kernel leaves.
//
// Work quantum = one STEP of kSwStep = 1024 positions (16 per lane) = one candidate list.  The chunk's steps are dealt
// to the resident waves as CONTIGUOUS RANGES of equal length (+-1 step): generation 5 dealt tiles of 2048 positions
// round-robin, 32768 tiles over 6144 waves = 5.33, and the third of the waves that ran a sixth tile — alone, at two waves
// per SIMD, every stage of the tile a dependent chain — held the kernel for 8-10 us of its 39 (waves alive 56 % of the
// kernel, profiles/r02_pmc_sq_summary.txt).  A wave walks its range in wave-private LDS tiles of two steps (+ 24 samples
// of look-ahead, stored with the top bit of every sample flipped, u16 -> i16); an odd step ends the range as a tile of
// one.  Every wave is autonomous: no workgroup barrier after the counter block is cleared.
//
//   1. pre-check  pa[1] > pa[7] && pa[12] > pa[14] && pa[12] > pa[15]  (demod_2400.c:311-322): 16 positions per
//      lane out of four 16-byte LDS reads, two positions per packed-i16 instruction (saturating subtract, max,
//      arithmetic shift: six instructions per pair); about 1 position in 6 survives;
//   2. the survivors are compacted in position order into an LDS queue: popcount + DPP prefix sum (full-rate VALU, no
//      LDS crossbar), then every lane with a survivor stores its first kSwUnroll positions with unconditional 2-byte LDS
//      writes issued from the LAST to the first — a lane with fewer survivors writes junk into slots of the lanes behind
//      it, which those lanes' own, later, writes replace (proof at the code) — and a short exec-masked loop takes what
//      is left of the rare lane with more (a loop over every survivor ran max-over-lanes = 7 iterations of 10
//      instructions for 2.7 survivors per lane);
//   3. threshold tests (demod_2400.c:324-378), lane = survivor: pa[1..18] as nine sample pairs fetched at the
//      survivor's own alignment (aligned dwords + v_alignbit), then 13 v_dot2_i32_i16 on the biased samples:
//          pa_mag >= (base_noise * thr) >> 5   <=>   32 * pa_mag + 31 - thr * base_noise >= 0
//      (q = floor(R/32): T >= q <=> 32T + 31 >= R for integers), with 32*(+-1, +-2, +-3) and -thr as the packed
//      coefficients and the bias term 32768 * sum(coefficients) folded into the accumulator's start value;
//   4. candidates (position in the unit << 3 | phase mask) appended to their step's list in global memory; the tallies the
//      statistics need (candidates, tried phases) are taken by k_slice, which reads every code anyway.
// ---------------------------------------------------------------------------------------------
constexpr int kSwStep = WAVE * 16;                           // positions per pre-check step = per candidate list (1024)
static_assert(kSweepTile == kSwStep, "one candidate list per pre-check step");
constexpr int kSwHalo = 32;                                  // samples staged behind a step: the pre-check of its last lane reads 16 + 16, the threshold tests pos + 20
constexpr int kSwHalf = kSwStep + kSwHalo;                   // samples per LDS half (one step, self-contained)
constexpr int kSwUnroll = 6;                                 // survivors per lane stored by the unconditional writes
constexpr int kSwPQCap = kSwStep + WAVE + 8;                 // survivor queue: one step's worth + the leftovers + room for the junk writes
constexpr int kSwStepsPerUnit = kUnit / kSwStep;
constexpr int kSwMaxBlocks = kSweepGridMax;                  // resident workgroups of k_sweep
static_assert(kUnit % kSwStep == 0 && kSwUnroll < 8 && (kSwHalf * 2) % 16 == 0, "step geometry");

// timing experiments (tools/micro/sweep_cold.hip only): 1 = staging alone (the memory side of the kernel), 2 = + pre-check and
// prefix sum, 3 = + survivor queue, 0 = the kernel
#ifndef MGPU_SW_STAGE
#define MGPU_SW_STAGE 0
#endif
// Generation 7's dealing: a wave takes HALF of its equal share without asking and the rest from a dealer, two steps at a time (pools
// of workgroups, one counter per pool, 256 bytes apart: k_slice's dealer, see slice.inc).  With equal contiguous shares (generation 6)
// the waves of a launch ended between 45 and 63 us of a 63 us kernel (profiles/r04_sweep_cold.json: waves alive 86 %) — VALU issue
// goes by age, the memory system is not fair, and pacing only narrows the spread.  Nothing in a step depends on which step the wave
// swept before: the survivors left over from the previous step are evaluated out of the OTHER LDS half whatever its step number was
// (`s_prev`), so a dealt block needs no flush and no restart.
// (Measured and dropped: generation 6's contiguous ranges, profiles/r05_sweep_cold_d0.json; an L2 touch two steps ahead, 74.9 us cold,
// DESIGN.md §3; non-temporal magnitude stores in k_sweep_uc8, profiles/r06_sweep_fused.txt; one LDS half with the queue emptied after
// every step, 8 waves per SIMD.)
constexpr uint32_t kSwDealSteps = 2;                         // steps per dealt block (1 and 4 no better: profiles/r05_sweep_cold_b1.json, r05_sweep_cold_b4.json)
// The static half of a wave's share not as ONE contiguous range but as blocks of kSwStaticBlock steps, block j of wave w =
// (j * waves + w): at any time the grid's waves work on one contiguous window of the chunk (waves x B steps = 32 MB of samples and
// as much of magnitudes) instead of 4096 places 32 KB apart.  For k_sweep_uc8 — which sits on its memory time with a 1:1 read /
// write mix — that is 5 % (bracket 0.414-0.420 against 0.423-0.441 ms per 537 M samples, roofline.frac 0.645 against 0.61, three
// interleaved sessions, profiles/r06_sweep_fused.txt (7)); B = 8 the same, B = 2 nothing, dealt blocks of 4 / 8 steps or another
// static share than half: worse.  k_sweep alone (reads only, issue-bound): no difference (cold 65.6 / 65.7 us).
constexpr uint32_t kSwStaticBlock = 4;                       // steps per static block
constexpr uint32_t kSwStaticPct = 50;                        // the static share of a wave's steps, per cent (the rest is dealt)

struct SweepLds {                                            // wave-private LDS
    uint16_t mag[2 * kSwHalf];                               // 4224 B: two steps, each with its own look-ahead
    uint16_t pq[kSwPQCap];                                   // 2192 B: pre-check survivors, sample index in mag[] + 1
};

__device__ __forceinline__ v2i16 pk16(int lo, int hi) { return v2i16{(short) lo, (short) hi}; }

// ---- FUSED (k_sweep_uc8): what the converter did ----
// The exact per-buffer sum(mag) and sum(mag^2) (convert.c:64-108).  A wave keeps its five byte-sum accumulators (cv_acc4, convert.inc)
// running over the CONTIGUOUS steps it sweeps — its static share, a dealt block — and reduces them across the lanes only where a run
// ends: at the next buffer's first step, where the wave's sequence jumps, after kSwRunMax steps (the 32-bit bounds below).  One
// reduction per step (the first form: per-step sums in HBM that k_slice's prologue added up) was 52 of the step's 358 vector
// instructions; per run it is a third of that, and the per-step array and the prologue are gone.  The sums are integers: the order
// of the atomic additions does not matter.  (The launch takes as long as before, 0.43-0.47 ms per four, gpurun r06ae: with the
// instructions down a tenth the kernel sits on its memory time — k_convert_uc8_lean alone took 99.8 us for the same 537 MB.)
// A lane's five accumulators (hh, hl, ll, h, l) are three numbers to reduce, not five: sum(m) = 256 h + l, and
// sum(m^2) = 65536 A + B with A = hh + (hl >> 7), B = 512 (hl & 127) + ll.  Bounds: a run is at most kSwRunMax steps and the 326
// positions in front of a buffer's first step, N <= 16 * kSwRunMax + 16 samples per lane; hh, hl, ll <= 255^2 N, 256 h + l <= 65535 N:
// the sums of 64 lanes stay below 2^32 while N <= 1023.
// (The three DPP chains step in turn: a DPP operand written by the instruction before needs two wait states — one chain after the
// other the compiler filled them with 43 s_nop, each an issue slot; interleaved, every chain's wait is the other two's work.)
constexpr uint32_t kSwRunMax = 32;
static_assert((16ull * kSwRunMax + 16ull) * 65535ull * 64ull < (1ull << 32), "a run's sums are reduced in 32 bits");
__device__ __forceinline__ void sweep_reduce3(const CvAcc &a, uint32_t &level, uint32_t &A, uint32_t &B) {
    int x = (int) (256u * a.h + a.l), y = (int) (a.hh + (a.hl >> 7)), z = (int) (512u * (a.hl & 127u) + a.ll);
#define SW_R3(ctrl, rows) do { \
        const int dx = __builtin_amdgcn_update_dpp(0, x, ctrl, rows, 0xf, false), dy = __builtin_amdgcn_update_dpp(0, y, ctrl, rows, 0xf, false), \
                  dz = __builtin_amdgcn_update_dpp(0, z, ctrl, rows, 0xf, false); \
        x += dx; y += dy; z += dz; } while (0)
    SW_R3(0x111, 0xf); SW_R3(0x112, 0xf); SW_R3(0x114, 0xf); SW_R3(0x118, 0xf);       // row_shr 1, 2, 4, 8
    SW_R3(0x142, 0xa); SW_R3(0x143, 0xc);                                             // row_bcast 15 -> rows 1, 3; row_bcast 31 -> rows 2, 3
#undef SW_R3
    level = (uint32_t) __builtin_amdgcn_readlane(x, WAVE - 1); A = (uint32_t) __builtin_amdgcn_readlane(y, WAVE - 1); B = (uint32_t) __builtin_amdgcn_readlane(z, WAVE - 1);
}
// a run's sums -> its buffer's (zero when the slot is handed out: k_publish; the converter's own kernels add to them the same way)
__device__ __forceinline__ void sweep_flush_sums(CvAcc &run, unsigned long long *sum_level, unsigned long long *sum_power, uint32_t buffer) {
    uint32_t level, A, B;
    sweep_reduce3(run, level, A, B);
    if (lane_id() == 0) {
        atomicAdd(&sum_level[buffer], (unsigned long long) level);
        atomicAdd(&sum_power[buffer], 65536ull * A + B);
    }
    run = CvAcc{0, 0, 0, 0, 0};
}

// A step staged sample by sample: positions 0..325 of the chunk are the 326 magnitudes before it (p.tail; zeros at stream start:
// sdr_ifile.c:209-213), positions from 326 + n on have no sample.  Magnitudes to d_mag (the tail's too: the converter's prologue did
// that), into the LDS half with the top bit flipped (half == nullptr: the steps behind the last scan position, which only exist
// for their magnitudes), the step's sums straight to its buffers'.  The chunk's first step and its last one or two: not worth a fast path.
// Where a fused sweep's samples come from (MODE): 1 = UC8 through the shared table (k_sweep_uc8), 2 / 3 = SC16 / SC16Q11 by arithmetic
// (k_sweep_sc16<15 / 11>: convert.inc's sc16_magsq + sqrt_cr_unit, every float operation rounded on its own as the reference's).
constexpr int kSwPlain = 0, kSwUC8 = 1, kSwSC16 = 2, kSwSC16Q11 = 3;
template <int MODE> constexpr int sw_sc16_shift() { return MODE == kSwSC16 ? 15 : 11; }
template <int SCALE_SHIFT>
__device__ __forceinline__ uint32_t sc16_mag_u16(uint32_t w) {   // convert.c:212-250, 329-367: one sample's magnitude, as k_convert_sc16 forms it
#pragma clang fp contract(off)
    const float mag = sqrt_cr_unit(sc16_magsq<SCALE_SHIFT>(w));
    const float sc = mag * 65535.0f;
    const float rd = sc + 0.5f;
    return (uint32_t) (uint16_t) rd;
}
template <int SCALE_SHIFT>
__device__ __forceinline__ uint32_t sc16_mag_pair(uint32_t w0, uint32_t w1) { return sc16_mag_u16<SCALE_SHIFT>(w0) | (sc16_mag_u16<SCALE_SHIFT>(w1) << 16); }

struct SweepSource { const uint8_t *iq; const uint16_t *tail; uint16_t *mag_w; unsigned long long *sum_level, *sum_power; uint64_t n; uint32_t buf_steps; };
template <int MODE>
__device__ __noinline__ void sweep_stage_careful(SweepSource p, const uint16_t *s_lut, uint32_t st, uint16_t *half) {   // (by value: in registers, no scratch)
    const int lane = lane_id();
    const bool first_of_buffer = (st & (p.buf_steps - 1u)) == 0u;      // (buf_steps: a power of two — launch_sweep's condition for this kernel)
    unsigned long long lv[2] = {0, 0}, pw[2] = {0, 0};
    auto one = [&](uint32_t in_step, bool mine) __attribute__((always_inline)) -> uint32_t {
        const uint64_t D = (uint64_t) st * kSwStep + in_step;
        uint32_t m = 0;
        if (D < (uint64_t) kTrailing) m = p.tail ? p.tail[D] : 0u;
        else if (D - kTrailing < p.n) {
            const uint64_t i = D - kTrailing;
            if constexpr (MODE == kSwUC8) {
                const uint32_t vi = p.iq[2 * i], vq = p.iq[2 * i + 1];
                const uint32_t fi = (vi ^ (0x7fu + (vi >> 7))) & 0xffu, fq = (vq ^ (0x7fu + (vq >> 7))) & 0xffu;
                m = s_lut[fq * 128u + fi];
            } else m = sc16_mag_u16<sw_sc16_shift<MODE>()>(*(const uint32_t *) (p.iq + 4 * i));
            if (MODE == kSwUC8 && mine) { const int k = (first_of_buffer && in_step < (uint32_t) kTrailing) ? 0 : 1; lv[k] += m; pw[k] += (unsigned long long) m * m; }
        }
        if (mine && D < (uint64_t) kTrailing + p.n) p.mag_w[D] = (uint16_t) m;
        return m;
    };
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t ma = one(8u * lane + e, true), mb = one(512u + 8u * lane + e, true);
        if (half) { half[8 * lane + e] = (uint16_t) (ma ^ 0x8000u); half[512 + 8 * lane + e] = (uint16_t) (mb ^ 0x8000u); }
    }
    if (half && lane < 16) {                                  // the look-ahead: the next step's first 32 samples (not this step's to write or to count)
        half[kSwStep + 2 * lane] = (uint16_t) (one((uint32_t) kSwStep + 2u * lane, false) ^ 0x8000u);
        half[kSwStep + 2 * lane + 1] = (uint16_t) (one((uint32_t) kSwStep + 2u * lane + 1u, false) ^ 0x8000u);
    }
    if constexpr (MODE != kSwUC8) return;                    // (the SC16 formats' means are the reference's sequential FLOAT sums: k_fsum_sc16)
    const unsigned long long a = wave_sum_u64(lv[0]), b = wave_sum_u64(pw[0]), c = wave_sum_u64(lv[1]), d = wave_sum_u64(pw[1]);
    if (lane == 0) {                                          // (nothing to add: also the step behind the stream's last buffer, which has no sums)
        const uint32_t buffer = st / p.buf_steps;
        if (a | b) { atomicAdd(&p.sum_level[buffer - 1u], a); atomicAdd(&p.sum_power[buffer - 1u], b); }   // (only a buffer's first step has this part, and step 0's is p.tail: not counted)
        if (c | d) { atomicAdd(&p.sum_level[buffer], c); atomicAdd(&p.sum_power[buffer], d); }
    }
}

// The kernel's body.  BLOCK: threads per workgroup; FUSED (k_sweep_uc8, below): the step's samples come from the UC8 IQ stream and
// are converted on the way into the LDS half (s_lut: the 32 KB symmetric quadrant of k_convert_uc8_lean, shared by the workgroup's
// waves), the magnitudes are written out for k_slice, and the samples' exact sum(mag) / sum(mag^2) are added to their buffers' (p.sum_level, p.sum_power).
template <int BLOCK, int MODE>
__device__ __forceinline__ void sweep_body(const SweepParams &p, SweepLds *s_w, const uint16_t *s_lut) {
    constexpr bool FUSED = MODE != kSwPlain, SC16 = MODE == kSwSC16 || MODE == kSwSC16Q11;
    constexpr int kSh = sw_sc16_shift<MODE>();
    const int lane = lane_id();
    const int wv = (int) rfl((uint32_t) threadIdx.x >> 6);
    SweepLds &L = s_w[wv];
    const uint32_t *w32 = (const uint32_t *) L.mag;
    const uint32_t wave_global = blockIdx.x * (BLOCK / WAVE) + wv;
    const uint32_t nwaves = gridDim.x * (BLOCK / WAVE);
    // the wave's share of the chunk's nsteps: the contiguous steps [st_next, st_end) first, then blocks of kSwDealSteps from its pool
    const uint32_t nsteps = (uint32_t) ((p.n + kSwStep - 1) / kSwStep);
    const uint32_t n_static = (uint32_t) ((uint64_t) nsteps * kSwStaticPct / 100u / nwaves) / kSwStaticBlock * kSwStaticBlock;   // steps every wave takes without asking: whole blocks
    const uint32_t nstat_blk = n_static / kSwStaticBlock;
    uint32_t stat_blk = 0;
    uint32_t st_next = wave_global * kSwStaticBlock;
    const uint32_t st_end = st_next + (n_static ? kSwStaticBlock : 0u);
    // the dealt region [n_static * nwaves, nsteps) in blocks, the blocks in contiguous ranges per pool
    const uint32_t dyn_lo = n_static * nwaves;
    const uint32_t nblk = (nsteps - dyn_lo + kSwDealSteps - 1) / kSwDealSteps;
    const uint32_t npools = gridDim.x < (uint32_t) kDealerCounters ? gridDim.x : (uint32_t) kDealerCounters;
    const uint32_t pool = blockIdx.x % npools;
    const uint32_t b_lo = (uint32_t) ((uint64_t) nblk * pool / npools), b_hi = (uint32_t) ((uint64_t) nblk * (pool + 1) / npools);
    uint32_t *const deal = p.dealer + (size_t) (kDealerCounters + pool) * kDealerStride;    // (k_slice's counters are the first kDealerCounters)

    // Packed coefficients of the threshold tests, NEGATED (see the header comment): the accumulators hold
    // thr * base_noise - 32 * pa_mag - 32, negative <=> the phase reaches the threshold, so a sign bit is a phase bit.
    // Kept in scalar registers: a literal makes every v_dot2c an 8-byte instruction.
    const int thr = p.thr;
    const v2i16 kN_lo = pk16(thr, 0), kN_hi = pk16(0, thr), kN_both = pk16(thr, thr);
    uint32_t cPM = 0x0020ffe0u, cPP = 0xffe0ffe0u, cMP = 0xffe00020u, c6a = 0xffa00000u, c6b = 0x00000060u, c6c = 0x00000020u;
    asm volatile("" : "+s"(cPM), "+s"(cPP), "+s"(cMP), "+s"(c6a), "+s"(c6b), "+s"(c6c));
    const v2i16 kPM = __builtin_bit_cast(v2i16, cPM), kPP = __builtin_bit_cast(v2i16, cPP), kMP = __builtin_bit_cast(v2i16, cMP);   // -(32,-32) -(32,32) -(-32,32)
    const v2i16 k6a = __builtin_bit_cast(v2i16, c6a), k6b = __builtin_bit_cast(v2i16, c6b), k6c = __builtin_bit_cast(v2i16, c6c);   // -(0,96) -(-96,0) -(-32,0)
    const int acc0 = -(32768 * (128 - 5 * thr) + 31) - 1;    // coefficient sums: 4 * 32 (phases 4..7), 3 * 32 (phase 8), -5 thr
    constexpr int kBias6 = 32768 * 32;                       // phase 8's sum is 32 short of the others'
    static_assert((kUnit << 3) == 65536, "a candidate code is the position modulo the unit, 13 bits, and three phase bits");

#if MGPU_EXPERIMENTS
    const unsigned long long dbg_t0 = __builtin_amdgcn_s_memrealtime();      // 100 MHz
    uint32_t dbg_sink = 0;
#endif
    // ---- the wave's sequence of steps: `cur` is swept while the samples of `nxt` are on their way into registers ----
    uint32_t rng_next = st_next, rng_end = st_end;           // what is left of the range being swept: the wave's contiguous share first, then one dealt block after the other
    uint32_t next_blk = 0xffffffffu;                         // the block the pool's dealer has answered with (>= b_hi: the pool is empty)
    bool ask_now = false;                                    // a block was taken in this step: ask for the one after it (below)
    // A request goes out in the step that takes a block — and in the wave's first step — and its answer is read at the end of the same
    // step, a whole step later.  (A wave with fewer than two contiguous steps — a small chunk — waits for its first block at once: the
    // block's first step is prefetched while the step before it is swept, so it has to be known at the top of that one.)
    const uint32_t deal_zero = deal_opaque_zero();
    if (b_lo < b_hi) {
        if (st_end - st_next >= 2u) ask_now = true;
        else {
            uint32_t t0 = 0;
            if (lane == 0) t0 = deal_ask(deal, deal_zero);
            next_blk = b_lo + rfl(t0);
        }
    }
    // the next step of the wave's sequence, kNone = none left (a macro, not a lambda: with the by-reference captures of a lambda the
    // cursors ended up in scratch memory)
#define SW_ADVANCE(dst) do { \
        if (rng_next < rng_end) dst = rng_next++; \
        else if (++stat_blk < nstat_blk) { rng_next = (stat_blk * nwaves + wave_global) * kSwStaticBlock; rng_end = rng_next + kSwStaticBlock; dst = rng_next++; } \
        else if (next_blk < b_hi) { \
            rng_next = dyn_lo + next_blk * kSwDealSteps; \
            rng_end = rng_next + kSwDealSteps < nsteps ? rng_next + kSwDealSteps : nsteps; \
            next_blk = 0xffffffffu; \
            ask_now = true; \
            dst = rng_next++; \
        } else dst = kNone; \
    } while (0)
    if constexpr (FUSED) {
        // the magnitudes behind the last scan position — the last 326 samples, which the last positions' look-ahead and the next
        // chunk's tail read — lie in steps nobody sweeps: one wave stages them, for their magnitudes and sums only
        const uint32_t nconv = (uint32_t) ((p.n + kTrailing + kSwStep - 1) / kSwStep);
        if (wave_global == 0) for (uint32_t st = nsteps; st < nconv; ++st) sweep_stage_careful<MODE>(SweepSource{p.iq, p.tail, p.mag_w, p.sum_level, p.sum_power, p.n, p.buf_steps}, s_lut, st, nullptr);
    }
    uint32_t cur;
    SW_ADVANCE(cur);
    if (cur != kNone) {
    // ---- staging: lane l brings chunks l and l + 64 of a step (8 samples each) and, all lanes alike, one of the four
    //      look-ahead chunks (only lanes 0..3 store theirs): three unconditional loads, no lane-dependent control ----
    const uint16_t *src = p.mag + (uint64_t) cur * kSwStep + 8 * lane;
    const int halo_off = kSwStep - 8 * lane + 8 * (lane & 3);                 // (from src) chunk 128 + (lane & 3)
    u32x4 pre0 = {0, 0, 0, 0}, pre1 = {0, 0, 0, 0}, pre2 = {0, 0, 0, 0};
    u32x4 pre3 = {0, 0, 0, 0};                                                // SC16: a chunk of 8 samples is 32 bytes (pre0 | pre1: chunk l, pre2 | pre3: chunk l + 64)
    uint32_t preh = 0, preh2 = 0;                                             // FUSED: the look-ahead's IQ, two samples in each of lanes 0..15 (UC8: one dword, SC16: two)
    // FUSED: a step whose samples are not all there — the chunk's first (positions 0..325 are the 326 magnitudes before the chunk:
    // p.tail) and the last ones (samples behind p.n) — is staged sample by sample (sweep_stage_careful): a handful per launch
    const uint32_t st_tail = (uint32_t) ((p.n + kTrailing - kSwHalo) / kSwStep);   // (st + 1) * 1024 + 32 > n + 326  <=>  st >= this
    auto careful = [&](uint32_t st) __attribute__((always_inline)) { return st == 0u || st >= st_tail; };
    // the IQ bytes of position D's sample (D >= 326): p.iq + 2 * (D - 326); lane l stages chunks l and l + 64 of a step (8 samples each)
    constexpr int kBps = SC16 ? 4 : 2;                                        // bytes per IQ sample
    auto iq_of = [&](uint32_t st) __attribute__((always_inline)) { return p.iq + kBps * ((int64_t) st * kSwStep + 8 * lane - kTrailing); };
    // the step's IQ into registers (SC16: 326 samples of delay = 1304 bytes: the 16-byte loads are 8-byte aligned)
    auto fetch_iq = [&](uint32_t st) __attribute__((always_inline)) {
        const uint8_t *is = iq_of(st);
        if constexpr (SC16) {
            const u32x4_a8 a = *(const u32x4_a8 *) is, a2 = *(const u32x4_a8 *) (is + 16), b = *(const u32x4_a8 *) (is + 4 * 512), b2 = *(const u32x4_a8 *) (is + 4 * 512 + 16);
            pre0 = u32x4{a.x, a.y, a.z, a.w}; pre1 = u32x4{a2.x, a2.y, a2.z, a2.w}; pre2 = u32x4{b.x, b.y, b.z, b.w}; pre3 = u32x4{b2.x, b2.y, b2.z, b2.w};
            const u32x2_a8 h = *(const u32x2_a8 *) (is + 4 * (kSwStep - 8 * lane) + 8 * (lane & 15));
            preh = h.x; preh2 = h.y;
        } else {
            const u32x4_a4 a = *(const u32x4_a4 *) is, b = *(const u32x4_a4 *) (is + 2 * 512);
            pre0 = u32x4{a.x, a.y, a.z, a.w}; pre1 = u32x4{b.x, b.y, b.z, b.w};
            preh = *(const uint32_t *) (is + 2 * (kSwStep - 8 * lane) + 4 * (lane & 15));
        }
    };
    if constexpr (FUSED) {
        if (!careful(cur)) fetch_iq(cur);
    } else {
        pre0 = *(const u32x4 *) src; pre1 = *(const u32x4 *) (src + 512); pre2 = *(const u32x4 *) (src + halo_off);
    }
    const uint32_t last_bits = (uint32_t) (p.n - (uint64_t) (nsteps - 1) * kSwStep);     // positions of the chunk's last step (1 .. 1024)
    uint32_t nxt = kNone, s_prev = cur - 1u, done = 0;       // s_prev: the step swept before `cur` (its leftovers wait in the other half); done: steps swept
    bool have_prev = false;
    int pqn = 0, pqh = 0;                                    // survivors waiting in L.pq[pqh .. pqn)
    int cnt_cur = 0, cnt_old = 0;                            // candidates in the lists of the step being swept / of the step before it
    int rem_old = 0;                                         // queue entries left over from the step before
    uint32_t vmask = 0xffffu;                                // the lane's positions that exist (all of them, except in the chunk's last step)
    CvAcc run = {0, 0, 0, 0, 0};                             // FUSED: the byte sums of the run of contiguous steps being swept (sweep_flush_sums)
    uint32_t run_steps = 0;
    const uint32_t buf_shift = 31u - (uint32_t) __builtin_clz(p.buf_steps | 1u);   // (buf_steps: a power of two)

    // ---- threshold tests for up to 64 pre-check survivors, lane = survivor.  `s_cur` = the step being swept (its samples are
    //      in the half at hoff_cur); the queue is in the order the wave swept, so what is left of step s_prev comes first ----
    auto eval_round = [&](int take, uint32_t s_cur, int hoff_cur) __attribute__((always_inline)) {
        int x4 = 0, x5 = 0, x6 = 0, idx1 = 0;
        if (lane < take) {
            idx1 = L.pq[pqh + lane];                         // sample index + 1
            const uint32_t *q = w32 + (idx1 >> 1);
            const uint32_t sh = (uint32_t) idx1 << 4;        // (v_alignbit uses the low five bits: 0 or 16)
            uint32_t d[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) d[k] = q[k];
#define PAIR(k) __builtin_bit_cast(v2i16, __builtin_amdgcn_alignbit(d[(k) + 1], d[k], sh))   /* (pa[2k+1], pa[2k+2]), biased */
            const v2i16 P0 = PAIR(0), P1 = PAIR(1), P2 = PAIR(2), P3 = PAIR(3), P4 = PAIR(4), P5 = PAIR(5), P7 = PAIR(7), P8 = PAIR(8);
#undef PAIR
            // thr * (pa[5] + pa[8] + pa[16] + pa[17] + pa[18]) - 32
            int nr = __builtin_amdgcn_sdot2(P2, kN_lo, acc0, false);
            nr = __builtin_amdgcn_sdot2(P3, kN_hi, nr, false);
            nr = __builtin_amdgcn_sdot2(P7, kN_hi, nr, false);
            nr = __builtin_amdgcn_sdot2(P8, kN_both, nr, false);
            // - 32 * (pa[1] - pa[2] + pa[3] + pa[4])
            int c = __builtin_amdgcn_sdot2(P0, kPM, nr, false);
            c = __builtin_amdgcn_sdot2(P1, kPP, c, false);
            // phases 4/5: - 32 * (pa[9] - pa[10] + pa[11] + pa[12]); phases 6/7: - 32 * (pa[9] + pa[10] - pa[11] + pa[12])
            x4 = __builtin_amdgcn_sdot2(P5, kPP, __builtin_amdgcn_sdot2(P4, kPM, c, false), false);
            x5 = __builtin_amdgcn_sdot2(P5, kMP, __builtin_amdgcn_sdot2(P4, kPP, c, false), false);
            // phase 8: 32 * (pa[1] + 2 pa[2] - 2 pa[3] + pa[4] + pa[10] - pa[11] + pa[12]) = the 6/7 sum + 32 * (3 pa[2] - 3 pa[3] - pa[9])
            x6 = __builtin_amdgcn_sdot2(P0, k6a, x5 + kBias6, false);
            x6 = __builtin_amdgcn_sdot2(P1, k6b, x6, false);
            x6 = __builtin_amdgcn_sdot2(P4, k6c, x6, false);
        }
        const int any = x4 | x5 | x6;                        // negative <=> a candidate
        const uint64_t cm = __ballot(any < 0);
        if (cm) {                                            // (nearly every round: one survivor in fourteen is a candidate)
            // slot counted from the list of s_prev: the list of s_cur lies `dlist` slots behind it (1024 when the steps are neighbours)
            const bool is_cur = (idx1 > kSwHalf) == (hoff_cur != 0);
            const int dlist = (int) ((s_cur - s_prev) * (uint32_t) kSwStep);
            const int nall = __popcll(cm), nold = __popcll(cm & ~__ballot(is_cur));
            const int rank = (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (cm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) cm, 0u));
            // (selects of 0 / a scalar and three-operand adds: two instructions per value where a select between two scalars takes four)
            const int slot = rank + cnt_old + (is_cur ? dlist + cnt_cur - nold - cnt_old : 0);
            // position in the chunk = step * 1024 + sample index - the half's offset; the code carries it modulo the unit
            const uint32_t pb_old = s_prev * (uint32_t) kSwStep - (uint32_t) (kSwHalf - hoff_cur) - 1u;
            const uint32_t pb_step = (uint32_t) dlist - (uint32_t) hoff_cur + (uint32_t) (kSwHalf - hoff_cur);   // pb_cur - pb_old
            const uint32_t pos = (uint32_t) idx1 + pb_old + (is_cur ? pb_step : 0u);
            uint32_t code = (pos << 1) | ((uint32_t) x6 >> 31);                          // ... << 3 | phase mask: bit 2 = phase 8, bit 1 = phases 6/7, bit 0 = phases 4/5
            code = (code << 1) | ((uint32_t) x5 >> 31);
            code = (code << 1) | ((uint32_t) x4 >> 31);
            if (any < 0) (p.cand + (int64_t) (int32_t) s_prev * kSwStep)[slot] = (uint16_t) code;   // (16 bits: the position modulo the unit of 8192; s_prev = -1 before the wave's first step)
            cnt_old += nold;
            cnt_cur += nall - nold;
        }
        pqh += take;
    };

    // Pacing.  A SIMD's VALU issue is arbitrated by priority, then AGE (MI355X_MICROARCH.md): of six resident waves with equal
    // shares the oldest ran at twice the youngest's speed, ended at 18 us and left the SIMD to ever fewer waves until 34.  Every
    // wave therefore compares its progress with the clock — steps done against elapsed time / the reference step time the host
    // passes (its own running estimate, launch_sweep) — and raises its priority while it is behind.  A wrong reference puts all
    // waves on one priority, which is the unpaced kernel; nothing but speed depends on it.
    const uint32_t pace = p.pace_recip;                      // 2^32 / reference step time in 10 ns ticks; 0 = off
    const unsigned long long pace_t0 = __builtin_amdgcn_s_memrealtime();
    int hoff = 0;                                            // this step's half of the tile: they alternate
    const uint32_t s_ragged = last_bits < (uint32_t) kSwStep ? nsteps - 1u : kNone;   // the step with positions beyond the end of the stream, if any
    for (; cur != kNone; s_prev = cur, have_prev = true, cur = nxt, ++done, hoff ^= kSwHalf) {
        const uint32_t s = cur;
        if (pace) {
            const uint32_t t = (uint32_t) (__builtin_amdgcn_s_memrealtime() - pace_t0);
            const int behind = (int) __umulhi(t, pace) - (int) done;   // steps the clock is ahead of this wave
            // (a tree of two compares: the chain of four cost twice the scalar instructions, every step)
            if (behind >= 1) { if (behind >= 2) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(2); }
            else { if (behind == 0) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
        }
        // the half is free: nothing of the step that was in it is waiting any more (see the end of the loop body)
        if constexpr (FUSED) {
            if (careful(s)) {
                if (run_steps) { sweep_flush_sums(run, p.sum_level, p.sum_power, (s - 1u) >> buf_shift); run_steps = 0; }   // (a run is contiguous: it ended with step s - 1)
                sweep_stage_careful<MODE>(SweepSource{p.iq, p.tail, p.mag_w, p.sum_level, p.sum_power, p.n, p.buf_steps}, s_lut, s, &L.mag[hoff]);
            } else {
                // the step's 1024 samples -> magnitudes (UC8: two per table read pair, cv_lookup2, convert.inc; SC16: by arithmetic), out
                // to d_mag for k_slice and the window statistics, into the half with the top bits flipped; the 32 samples of look-ahead by lanes 0..15
                uint32_t a0, a1, a2, a3, b0, b1, b2, b3, mh;
                if constexpr (SC16) {
                    a0 = sc16_mag_pair<kSh>(pre0.x, pre0.y); a1 = sc16_mag_pair<kSh>(pre0.z, pre0.w); a2 = sc16_mag_pair<kSh>(pre1.x, pre1.y); a3 = sc16_mag_pair<kSh>(pre1.z, pre1.w);
                    b0 = sc16_mag_pair<kSh>(pre2.x, pre2.y); b1 = sc16_mag_pair<kSh>(pre2.z, pre2.w); b2 = sc16_mag_pair<kSh>(pre3.x, pre3.y); b3 = sc16_mag_pair<kSh>(pre3.z, pre3.w);
                    mh = sc16_mag_pair<kSh>(preh, preh2);
                } else {
                    a0 = cv_lookup2(s_lut, pre0.x); a1 = cv_lookup2(s_lut, pre0.y); a2 = cv_lookup2(s_lut, pre0.z); a3 = cv_lookup2(s_lut, pre0.w);
                    b0 = cv_lookup2(s_lut, pre1.x); b1 = cv_lookup2(s_lut, pre1.y); b2 = cv_lookup2(s_lut, pre1.z); b3 = cv_lookup2(s_lut, pre1.w);
                    mh = cv_lookup2(s_lut, preh);
                }
                uint16_t *out = p.mag_w + (uint64_t) s * kSwStep + 8 * lane;
                *(u32x4 *) out = u32x4{a0, a1, a2, a3};
                *(u32x4 *) (out + 512) = u32x4{b0, b1, b2, b3};
                *(u32x4 *) &L.mag[hoff + 8 * lane] = u32x4{a0 ^ 0x80008000u, a1 ^ 0x80008000u, a2 ^ 0x80008000u, a3 ^ 0x80008000u};
                *(u32x4 *) &L.mag[hoff + 512 + 8 * lane] = u32x4{b0 ^ 0x80008000u, b1 ^ 0x80008000u, b2 ^ 0x80008000u, b3 ^ 0x80008000u};
                if (lane < 16) *(uint32_t *) &L.mag[hoff + kSwStep + 2 * lane] = mh ^ 0x80008000u;
                // the step's samples into the run's sums.  Positions 0..325 of a buffer's first step belong to the buffer before
                // (326 = 8 * 40 + 6): they close the run, the rest opens the next.  (UC8 only: the SC16 formats' means are float sums)
                if constexpr (MODE != kSwUC8) { }
                else if ((s & (p.buf_steps - 1u)) == 0u) {        // (one step in 128)
                    if (lane < 40) { cv_acc4(run, a0, a1); cv_acc4(run, a2, a3); }
                    else if (lane == 40) { cv_acc4(run, a0, a1); cv_acc4(run, a2, 0u); }
                    sweep_flush_sums(run, p.sum_level, p.sum_power, (s >> buf_shift) - 1u);
                    if (lane == 40) cv_acc4(run, a3, 0u);
                    else if (lane > 40) { cv_acc4(run, a0, a1); cv_acc4(run, a2, a3); }
                    cv_acc4(run, b0, b1); cv_acc4(run, b2, b3);
                    run_steps = 1;
                } else {
                    cv_acc4(run, a0, a1); cv_acc4(run, a2, a3); cv_acc4(run, b0, b1); cv_acc4(run, b2, b3);
                    ++run_steps;
                }
            }
        } else {
            const u32x4 a = {pre0.x ^ 0x80008000u, pre0.y ^ 0x80008000u, pre0.z ^ 0x80008000u, pre0.w ^ 0x80008000u};
            const u32x4 b = {pre1.x ^ 0x80008000u, pre1.y ^ 0x80008000u, pre1.z ^ 0x80008000u, pre1.w ^ 0x80008000u};
            const u32x4 c = {pre2.x ^ 0x80008000u, pre2.y ^ 0x80008000u, pre2.z ^ 0x80008000u, pre2.w ^ 0x80008000u};
            *(u32x4 *) &L.mag[hoff + 8 * lane] = a;
            *(u32x4 *) &L.mag[hoff + 512 + 8 * lane] = b;
            if (lane < 4) *(u32x4 *) &L.mag[hoff + kSwStep + 8 * lane] = c;
        }
        SW_ADVANCE(nxt);
        if constexpr (FUSED) {                               // the run ends where the wave's sequence jumps (or ends)
            if (run_steps && (nxt != s + 1u || run_steps >= kSwRunMax)) { sweep_flush_sums(run, p.sum_level, p.sum_power, s >> buf_shift); run_steps = 0; }
        }
        const bool asked_now = ask_now;                      // (also a block taken before the loop, by the wave's very first step)
        ask_now = false;
#define SW_ANSWER() do { if (asked_now) next_blk = b_lo + rfl(ticket); } while (0)   /* the step's last act (wave-uniform; the request is a step old) */
        if constexpr (FUSED) {
            if (nxt != kNone && !careful(nxt)) fetch_iq(nxt);
        } else if (nxt != kNone) {
            src = p.mag + (uint64_t) nxt * kSwStep + 8 * lane;
            pre0 = *(const u32x4 *) src; pre1 = *(const u32x4 *) (src + 512); pre2 = *(const u32x4 *) (src + halo_off);
        }
        // the request for the block after the one just taken: BEHIND the loads (the compiler's waits for them are counted from the
        // youngest operation: a request ahead of them would be waited for with them), into a variable of this iteration (deal_ask)
        uint32_t ticket;
        if (asked_now && lane == 0) ticket = deal_ask(deal, deal_zero);
        WAVE_SYNC();
#if MGPU_SW_STAGE == 1
        dbg_sink += w32[lane];
        SW_ANSWER();
        WAVE_SYNC();
        continue;
#endif
        // ---- pre-check, 16 positions per lane ----
        const int p0 = hoff + lane * 16;
        uint32_t w[16];                                    // w[k] = (m[2k], m[2k+1]), m[i] = sample p0 + i
        {
            const u32x4 a = *(const u32x4 *) &L.mag[p0], b = *(const u32x4 *) &L.mag[p0 + 8], c = *(const u32x4 *) &L.mag[p0 + 16],
                        d = *(const u32x4 *) &L.mag[p0 + 24];
            w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
            w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w; w[12] = d.x; w[13] = d.y; w[14] = d.z; w[15] = d.w;
        }
        uint32_t odd[15];                                  // odd[k] = (m[2k+1], m[2k+2])
#pragma unroll
        for (int k = 0; k < 15; ++k) odd[k] = __builtin_amdgcn_alignbit(w[k + 1], w[k], 16);
        uint32_t sm2 = 0;                                  // bit 2j: position p0+2j passes, bit 17+2j: position p0+2j+1 passes
#pragma unroll
        for (int j = 0; j < 8; ++j) {                      // positions p0+2j (low halves) and p0+2j+1 (high halves)
            // (biased samples: unsigned order of the magnitudes = signed order of what the tile holds)
            const v2i16 A = __builtin_bit_cast(v2i16, odd[j]), B = __builtin_bit_cast(v2i16, odd[j + 3]),
                        C = __builtin_bit_cast(v2i16, w[j + 6]), Dd = __builtin_bit_cast(v2i16, w[j + 7]),
                        E = __builtin_bit_cast(v2i16, odd[j + 7]);
            const v2i16 t1 = __builtin_elementwise_sub_sat(B, A);                                 // < 0 <=> pa[1] > pa[7]
            const v2i16 t2 = __builtin_elementwise_sub_sat(__builtin_elementwise_max(Dd, E), C);  // < 0 <=> pa[12] > max(pa[14], pa[15])
            const v2i16 y = __builtin_elementwise_max(t1, t2) >> 15;                              // 0xffff where both hold
            sm2 |= __builtin_bit_cast(uint32_t, y) & ((1u << (2 * j)) | (1u << (17 + 2 * j)));
        }
        if (s == s_ragged) {                               // positions beyond the end of the stream (the chunk's last step only)
            const int room = (int) last_bits - lane * 16;
            vmask = room >= 16 ? 0xffffu : room <= 0 ? 0u : (1u << room) - 1u;
            asm volatile("" : "+v"(vmask));                // (a branch taken once per launch, not two selects in every step)
        }
        const uint32_t sm = (sm2 | (sm2 >> 16)) & vmask;   // bit e: position p0 + e
        const int cnt = __popc(sm);
        int total;
        int incl = wave_incl_scan_dpp(cnt, total);
        asm volatile("" : "+v"(incl));                     // (keeps the scan a chain of six v_add_dpp: the compiler otherwise rebuilds the exclusive sum from its parts)
#if MGPU_SW_STAGE == 2
        dbg_sink += (uint32_t) incl;
        SW_ANSWER();
        continue;
#endif
        // room for this step's survivors behind the leftovers?  (they move to the front only when there is not)
        if (pqn + total > kSwPQCap - 8) {
            const int rem = pqn - pqh;
            uint16_t t = 0;
            if (lane < rem) t = L.pq[pqh + lane];
            WAVE_SYNC();
            if (lane < rem) L.pq[lane] = t;
            pqn = rem; pqh = 0;
            WAVE_SYNC();
        }
        const int dst = pqn + incl - cnt;
        // ---- the lane's survivors into L.pq[dst .. dst + cnt), in position order ----
        // Lanes with a survivor run kSwUnroll unconditional writes, slot dst + k in the k-th, issued k = kSwUnroll - 1 first.
        // A lane with cnt <= k writes junk into slot dst + k, which lies at or behind dst + cnt = the first slot of the lanes
        // behind it: it is slot dst' + k' of a later lane with dst' >= dst + cnt >= dst + 1, so k' <= k - 1 — that lane's own
        // write of it is issued later (LDS instructions of a wave execute in order) — or it is behind the last survivor of
        // the step (the queue has kSwUnroll slots of slack).  Slots k' >= kSwUnroll are only ever written by their owners.
        // (Release stores at wavefront scope — plain ds_write_b16, no waits: the compiler must neither reorder these stores
        // nor merge them into one 12-byte store, as it does with ordinary ones — within one instruction the order in which
        // the lanes' bytes land is not defined.)
        if (sm) {
            uint32_t t = sm;
            int e[kSwUnroll];
#pragma unroll
            for (int k = 0; k < kSwUnroll; ++k) { e[k] = __builtin_ctz(t); t &= t - 1; }   // (t == 0: a junk value for a junk write)
#pragma unroll
            for (int k = kSwUnroll - 1; k >= 0; --k)
                __hip_atomic_store(&L.pq[dst + k], (uint16_t) (p0 + 1 + e[k]), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WAVEFRONT);
            int d2 = dst + kSwUnroll;
            while (t) {
                const int e2 = __builtin_ctz(t);
                t &= t - 1;
                L.pq[d2++] = (uint16_t) (p0 + 1 + e2);
            }
        }
        pqn += total;
        WAVE_SYNC();
#if MGPU_SW_STAGE == 3
        pqn = pqh = 0;
        SW_ANSWER();
        continue;
#endif
        const bool ran = pqn - pqh >= WAVE;
        while (pqn - pqh >= WAVE) eval_round(WAVE, s, hoff);
        // The other half is staged next: whatever of the step before this one is still waiting goes first.  One full round
        // takes all of it (fewer than 64 were left); without one, a short round of exactly those.
        if (!ran && rem_old) eval_round(rem_old, s, hoff);
        // the previous step's list is complete
        if (have_prev) p.cand_count[s_prev] = (uint32_t) cnt_old;            // (every lane stores the same word)
        cnt_old = cnt_cur; cnt_cur = 0;
        rem_old = pqn - pqh;
        SW_ANSWER();
        WAVE_SYNC();                                           // the other half is rewritten next
    }
#undef SW_ANSWER
#undef SW_ADVANCE
    // what is left of the last step: it is "the step before" of a step that is not swept here, whose half is the other one
    if (pqn > pqh) eval_round(pqn - pqh, s_prev + 1u, hoff);
    p.cand_count[s_prev] = (uint32_t) cnt_old;
    // k_slice reads its tiles' lists in pairs: an odd number of steps leaves the last pair's second list empty
    // (the chunk's last step is the last one of the wave that sweeps it: a wave's steps come in rising order)
    if (s_prev == nsteps - 1u && (nsteps & 1u)) p.cand_count[nsteps] = 0;
    }
#if MGPU_EXPERIMENTS
    if (p.dbg_waves && lane == 0) {                            // the wave's life (tools/micro/sweep_cold.hip)
        p.dbg_waves[2 * wave_global] = dbg_t0;
        p.dbg_waves[2 * wave_global + 1] = __builtin_amdgcn_s_memrealtime() + (dbg_sink == 0x12345678u);
    }
#endif
}

// the sweep over a magnitude array (struct mag_buf entry, SC16 formats, Mode A/C; tools/micro/sweep_cold.hip): the roofline's kernel
__global__ __launch_bounds__(kBlock, 6) void k_sweep(SweepParams p) {
    __shared__ __attribute__((aligned(16))) SweepLds s_w[kBlock / WAVE];
    sweep_body<kBlock, kSwPlain>(p, s_w, nullptr);
}

// ---------------------------------------------------------------------------------------------
// k_sweep_uc8 (round 6): converter and sweep in ONE pass over the samples — the UC8 IQ stream is read once, every step's samples are
// converted on their way into the wave's LDS half, the magnitudes are written once (k_slice and the window statistics read them),
// and k_convert_uc8's launch, its 268 MB read and the sweep's own 268 MB read of the magnitudes are gone: 537 MB per 134 M samples
// where converter + sweep moved 1 074.
// What made it possible is the converter's lean form (convert.inc): 3.5 vector + 1 LDS instruction per sample for the lookup — and a
// table SHARED by a CU's waves: one workgroup of 1024 threads per CU (16 waves, 4 per SIMD; 32 KB of table + 16 x 6.4 KB of halves
// and queues = 135 KB of LDS) instead of six workgroups of 256 with a table each (round 2's fused form: two workgroups per CU, 88 us
// against 52 + 39).  Every wave is as autonomous as in k_sweep: one barrier, behind the table's load.
// The exact per-buffer sums (convert.c:64-108): sweep_flush_sums.
// ---------------------------------------------------------------------------------------------
constexpr int kSwFusedBlock = 1024;
__global__ __launch_bounds__(kSwFusedBlock, 1) void k_sweep_uc8(SweepParams p) {
    __shared__ __attribute__((aligned(16))) SweepLds s_w[kSwFusedBlock / WAVE];
    __shared__ __attribute__((aligned(16))) uint16_t s_lut[128 * 128];
    {
        constexpr int kVec = 128 * 128 / 8, kPer = kVec / kSwFusedBlock;      // 2048 x 16 B, 2 per thread
        const u32x4 *src = (const u32x4 *) p.uc8_sym;
        u32x4 t[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) t[k] = src[threadIdx.x + k * kSwFusedBlock];
#pragma unroll
        for (int k = 0; k < kPer; ++k) ((u32x4 *) s_lut)[threadIdx.x + k * kSwFusedBlock] = t[k];
    }
    __syncthreads();
    sweep_body<kSwFusedBlock, kSwUC8>(p, s_w, s_lut);
}

// k_sweep_sc16<15 / 11> (round 6): the same for SC16 / SC16Q11 input — the conversion is arithmetic (no table: workgroups of 256 as
// k_sweep's), the samples are read once (4 B), the magnitudes written once, k_sweep's own 2 B per sample of reads are gone.  The
// per-buffer mean level / power of these formats stay k_fsum_sc16's (the reference's sequential float sums).
template <int SCALE_SHIFT>
__global__ __launch_bounds__(kBlock, 5) void k_sweep_sc16(SweepParams p) {
    __shared__ __attribute__((aligned(16))) SweepLds s_w[kBlock / WAVE];
    sweep_body<kBlock, SCALE_SHIFT == 15 ? kSwSC16 : kSwSC16Q11>(p, s_w, nullptr);
}

static unsigned resident_grid(const void *kernel, size_t dyn_lds, unsigned max_blocks, int block = kBlock) {
    int per_cu = 0, dev = 0, cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, dyn_lds) != hipSuccess || per_cu < 1) per_cu = block > kBlock ? 1 : 2;
    unsigned resident = (unsigned) (per_cu * cus);
    return resident > max_blocks ? max_blocks : resident;
}

// The reference step time of the pacing (see the kernel): a running estimate from the launches the caller has timed —
// (kernel time - launch overhead) / steps per wave; with every wave on pace that is exactly what a step takes, so the
// estimate settles there.  Per process, not per context: the kernel and the device are the same for all of them.
// (The fetcher threads of every context write it, the feeding threads read it: relaxed atomics — only speed depends on the value,
// and a lost update costs one sample of a running average.)
static std::atomic<float> g_sweep_step_ticks{260.0f};        // 2.6 us: six waves per SIMD, synthetic traffic at 2000 frames/s
static std::atomic<float> g_sweep_sc16_step_ticks{520.0f};   // k_sweep_sc16: five waves per SIMD, ~17 vector instructions per sample more
static std::atomic<float> g_sweep_fused_step_ticks{370.0f};  // k_sweep_uc8: 3.7 us at four waves per SIMD (the two kernels may alternate in one process: their own estimates)
void sweep_pace_feedback(float kernel_us, uint64_t n, unsigned blocks, float bracket_us, int fused) {
    std::atomic<float> &g = fused == 2 ? g_sweep_sc16_step_ticks : fused ? g_sweep_fused_step_ticks : g_sweep_step_ticks;
    // (blocks: in units of kBlock threads — launch_sweep reports the fused kernel's grid that way)
    const double steps_per_wave = (double) ((n + kSwStep - 1) / kSwStep) / ((double) blocks * (kBlock / WAVE));
    if (steps_per_wave < 4.0 || kernel_us <= 8.0f) return;   // (small chunks do not fill the grid: nothing to learn, nothing to pace)
    float ticks = (float) ((kernel_us - bracket_us) * 100.0 / steps_per_wave);   // bracket_us: what the pair of timing events adds (mgpu_event_bracket_us; 4.5 until measured)
    ticks = ticks < 120.0f ? 120.0f : ticks > 800.0f ? 800.0f : ticks;
    g.store(0.5f * g.load(std::memory_order_relaxed) + 0.5f * ticks, std::memory_order_relaxed);
}

// returns the number of workgroups launched
unsigned launch_sweep(const SweepParams &p0, hipStream_t s) {
    if (p0.n == 0) return 0;
    static std::atomic<unsigned> resident_of[64], resident_fused_of[64];   // per device: the grid that is resident there (0 = not asked yet)
    static std::atomic<int> pace_env{-2};
    int dev = 0;
    (void) hipGetDevice(&dev);
    unsigned resident = resident_of[dev & 63].load(std::memory_order_relaxed);
    if (!resident) { resident = resident_grid((const void *) k_sweep, 0, kSwMaxBlocks); resident_of[dev & 63].store(resident, std::memory_order_relaxed); }
    int pace_on = pace_env.load(std::memory_order_relaxed);
    if (pace_on == -2) {
        const char *pe = nullptr;
#if MGPU_EXPERIMENTS
        pe = getenv("MGPU_SWEEP_PACE");                      // 0 = off, else the reference step time in 10 ns ticks (fixed: no feedback)
#endif
        pace_on = pe ? atoi(pe) : -1;
        pace_env.store(pace_on, std::memory_order_relaxed);
    }
    SweepParams p = p0;
    const unsigned nsteps = (unsigned) ((p.n + kSwStep - 1) / kSwStep);
    const float ticks = pace_on > 0 ? (float) pace_on : (p.iq ? g_sweep_fused_step_ticks : g_sweep_step_ticks).load(std::memory_order_relaxed);
    if (p.iq && p.iq_format != 0) {                          // SC16 / SC16Q11: converter and sweep in one, by arithmetic
        static std::atomic<unsigned> resident_sc16_of[64];
        constexpr int wpb = kBlock / WAVE;
        unsigned rf = resident_sc16_of[dev & 63].load(std::memory_order_relaxed);
        if (!rf) { rf = resident_grid((const void *) k_sweep_sc16<11>, 0, kSwMaxBlocks); resident_sc16_of[dev & 63].store(rf, std::memory_order_relaxed); }
        const unsigned want = (nsteps + wpb - 1) / wpb;
        const unsigned blocks = want < rf ? want : rf;
        const float t16 = pace_on > 0 ? (float) pace_on : g_sweep_sc16_step_ticks.load(std::memory_order_relaxed);
        p.pace_recip = (pace_on == 0 || nsteps < 4u * blocks * wpb) ? 0u : (uint32_t) (4294967296.0 / t16);
        if (p.iq_format == 1) hipLaunchKernelGGL(k_sweep_sc16<15>, dim3(blocks), dim3(kBlock), 0, s, p);
        else hipLaunchKernelGGL(k_sweep_sc16<11>, dim3(blocks), dim3(kBlock), 0, s, p);
        return blocks;
    }
    if (p.iq) {                                              // converter and sweep in one: k_sweep_uc8
        constexpr int wpb = kSwFusedBlock / WAVE;
        unsigned rf = resident_fused_of[dev & 63].load(std::memory_order_relaxed);
        if (!rf) { rf = resident_grid((const void *) k_sweep_uc8, 0, 256u * 2u, kSwFusedBlock); resident_fused_of[dev & 63].store(rf, std::memory_order_relaxed); }
        const unsigned want = (nsteps + wpb - 1) / wpb;
        const unsigned blocks = want < rf ? want : rf;
        p.pace_recip = (pace_on == 0 || nsteps < 4u * blocks * wpb) ? 0u : (uint32_t) (4294967296.0 / ticks);
        hipLaunchKernelGGL(k_sweep_uc8, dim3(blocks), dim3(kSwFusedBlock), 0, s, p);
        return blocks * (kSwFusedBlock / kBlock);
    }
    constexpr int wpb = kBlock / WAVE;
    const unsigned want = (nsteps + wpb - 1) / wpb;           // at least one step per wave
    const unsigned blocks = want < resident ? want : resident;
    p.pace_recip = (pace_on == 0 || nsteps < 4u * blocks * wpb) ? 0u : (uint32_t) (4294967296.0 / ticks);
    hipLaunchKernelGGL(k_sweep, dim3(blocks), dim3(kBlock), 0, s, p);
    return blocks;
}
