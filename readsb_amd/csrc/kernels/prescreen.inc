// kernels/prescreen.inc — post-sweep stage: pre-screen count / write passes, class bitmap, scratch publish.
// Part of the single translation unit kernels.hip (included inside namespace mgpu, after the parts before it).

// =============================================================================================
// pre-screen: a conditional record (score_unknown < 0) can only matter if its address has a bit in
// the adder bitmap: one that some clean DF17 / DF11-IID0 frame of this stream carries (the only
// frames that add to the ICAO filter, mode_s.c:766-779; k_slice sets their bits), or one the host
// added from outside (mgpu_filter_add sets its bit: network input the demodulator never sees).
// Everything else is "rejected_unknown_icao" for sure.
// The COUNT pass decides which records live and leaves the decision as a 64-bit mask in each segment header (a segment = the
// records one scoring pass of k_slice wrote for one tile: at most 64); the WRITE pass compacts the live records in stream order.
// It reads the masks, not the adder bitmap: it may run beside the next chunk's sweep, which adds bits to the bitmap (a second
// look could disagree with the counted offsets).
// =============================================================================================

// WRITE pass, one chain after the other, one segment after the other — the form that also computes, for every live record, the
// signal power the reference would report if this record became the accepted frame: sum of mag^2 over d_mag[pos+19 .. pos+19+len),
// len = 268 / 134 by the DF as sliced (demod_2400.c:399,436-457).  A shard pass whose records leave for another rank (which has no
// samples) wants that; the pipeline computes the powers after the walk, for the accepted frames only (k_msg_sig), and writes by
// chains (write_unit_chains below).
__device__ __forceinline__ uint32_t write_unit_sequential(uint32_t u, const PhaseRec *pool, const uint32_t *unit_first, uint32_t cpu, uint32_t nunits,
                                                          uint32_t dst0, PhaseRec *live, const uint16_t *mag, unsigned long long *live_sig) {
    const int lane = lane_id();
    if (u >= nunits) return 0;
    uint32_t nlive = 0;
    // the unit's chains, in stream order (one per k_slice tile): their heads come in one load, not one dependent load per chain
    uint32_t heads = kNone;
    if ((uint32_t) lane < cpu) heads = unit_first[u * cpu + (uint32_t) lane];
    for (uint32_t ch = 0; ch < cpu; ++ch) {
        uint32_t h = (uint32_t) __builtin_amdgcn_readlane((int) heads, (int) ch);
        while (h != kNone) {
            const uint32_t next = pool[h].addr;
            const uint64_t m = ((const unsigned long long *) &pool[h])[2];
            const bool ok = (m >> lane) & 1;
            uint32_t pos = 0, len = 0;
            if (ok) {
                const PhaseRec &r = pool[h + 1 + (uint32_t) lane];
                pos = r.pos;
                len = (r.msg[0] & 0x80) ? 268u : 134u;
                const uint32_t d = dst0 + nlive + __popcll(m & ((1ull << lane) - 1));
                const u32x4 *src = (const u32x4 *) &r;
                u32x4 *dd = (u32x4 *) &live[d];
                dd[0] = src[0]; dd[1] = src[1];
            }
            // signal power of the live records, four records per round: their 20 coalesced loads are in flight
            // together and the four reductions interleave (one record at a time this loop was a chain of
            // load latency + reduction per record — most of the write pass's time)
            uint64_t todo = mag ? m : 0;
            uint32_t k = 0;
            while (todo) {
                uint32_t p0[4], nn[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    p0[j] = 0; nn[j] = 0;
                    if (todo) {
                        const int src_lane = __ffsll((unsigned long long) todo) - 1;
                        todo &= todo - 1;
                        p0[j] = __builtin_amdgcn_readlane(pos, src_lane);
                        nn[j] = __builtin_amdgcn_readlane(len, src_lane);
                    }
                }
                unsigned long long acc[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint16_t *sm = mag + p0[j] + 19;
                    unsigned long long a = 0;
#pragma unroll
                    for (int it = 0; it < 5; ++it) {               // 268 = 4 * 64 + 12 samples at most
                        const uint32_t q = (uint32_t) lane + 64u * it;
                        const uint32_t v = q < nn[j] ? sm[q] : 0u;
                        a += (unsigned long long) (v * v);
                    }
                    acc[j] = a;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = wave_sum_u64(acc[j]);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (nn[j] && lane == 0) live_sig[dst0 + nlive + k + j] = acc[j];
                k += 4;
            }
            nlive += __popcll(m);
            h = next;
        }
    }
    return nlive;
}

// ---------------------------------------------------------------------------------------------
// The two passes as the pipeline runs them (count pass that leaves its decisions in the segment headers, write pass that reads
// them), CPU chains of a unit at a time.  Following one chain after the other, one segment after the other, is
// head -> header -> records -> bitmap words, ~3 dependent memory round trips per segment and ~6 segments per unit — the count pass
// took 45 us per 1024 buffers for 59 MB, a chain of latencies.  Here a round handles the current segment of ALL the unit's chains:
// their headers and (speculatively, 64 records behind every header: a segment holds at most 64) their records in one round trip,
// the bitmap words of all of them in a second.  What the write pass needs to place a segment without having seen the chains before
// it to their ends is left in the headers by the count pass: the live records of its chain before the segment (dword 6), and in a
// chain's FIRST header the chain's total (dword 7).
// Header layout (k_slice: score_pass): dword 0 = records, 1 = 0xFF (phase), 3 = next header, 4-5 = live mask, 6-7 as above.
// ---------------------------------------------------------------------------------------------
// The count pass also builds the unit's words of the class bitmap (1 bit per scan position: the position has records and all of them
// are conditional — what the window statistics ask, k_window_stats): it sees every record's position and REC_COND anyway.  The unit's
// 256 words of both classes are collected in the wave's LDS (`cls`: [2][kUnit / 32]) and leave as one 16-byte store per lane; nc / nu:
// the two class counters.  (Until round 4 k_slice set the bits in two planes in HBM with one atomic per record, and a pass over both
// planes — 50 MB per 1024 buffers, in the remaining workgroups of this launch — combined, counted and zeroed them.)
template <int CPU>
__device__ __forceinline__ uint32_t count_unit_chains(uint32_t u, PhaseRec *pool, uint32_t pool_cap, const uint32_t *unit_first, const uint32_t *first_count, uint32_t nunits,
                                                      const uint32_t *bitmap, unsigned long long *counters, uint32_t *cls, uint32_t *final_bitmap,
                                                      uint32_t &nc, uint32_t &nu) {
    constexpr int kW = kUnit / 32;                             // class words per unit (256)
    const int lane = lane_id();
    nc = nu = 0;
    if (u >= nunits) return 0;
#pragma unroll
    for (int k = 0; k < 2 * kW / WAVE; ++k) cls[lane + k * WAVE] = 0;
    WAVE_SYNC();
    // first_count (four chains per unit: k_slice): the records in every chain's first segment, so that the first round loads exactly
    // those — behind a header whose count is not known yet the loads cover 64 records, three times what an average segment holds
    uint32_t h = kNone, lim = (uint32_t) WAVE;
    if (lane < CPU) { h = unit_first[u * CPU + (uint32_t) lane]; if (first_count) lim = first_count[u * CPU + (uint32_t) lane]; }
    const uint32_t h_first = h;
    uint32_t run[CPU];                                         // wave-uniform: live records of chain ch so far
#pragma unroll
    for (int ch = 0; ch < CPU; ++ch) run[ch] = 0;
    while (__ballot(h != kNone)) {
        u32x4 hd = {0u, 0u, 0u, kNone};
        if (h != kNone) hd = *(const u32x4 *) &pool[h];
        uint32_t hc[CPU];
        u32x4 r[CPU];
#pragma unroll
        for (int ch = 0; ch < CPU; ++ch) {
            hc[ch] = (uint32_t) __builtin_amdgcn_readlane((int) h, ch);
            r[ch] = u32x4{0u, 0u, 0u, 0u};
            if (hc[ch] != kNone && (uint32_t) lane < (uint32_t) __builtin_amdgcn_readlane((int) lim, ch)) {
                uint32_t idx = hc[ch] + 1u + (uint32_t) lane;      // (beyond the segment's last record: somebody else's records, masked below)
                if (idx >= pool_cap) idx = pool_cap - 1u;
                r[ch] = *(const u32x4 *) &pool[idx];
            }
        }
        bool valid[CPU];
        uint32_t bw[CPU];
#pragma unroll
        for (int ch = 0; ch < CPU; ++ch) {
            const uint32_t cnt = (uint32_t) __builtin_amdgcn_readlane((int) hd.x, ch);
            valid[ch] = hc[ch] != kNone && (uint32_t) lane < cnt;
            bw[ch] = 0xFFFFFFFFu;
            if (hc[ch] != kNone && cnt > (uint32_t) __builtin_amdgcn_readlane((int) lim, ch) && lane == 0) atomicAdd(&counters[CNT_POOL_OVERFLOW], 1ull);   // cannot happen: a segment holds at most 64 records, a first segment what first_count says
            if (valid[ch] && ((r[ch].y >> 8) & REC_COND)) bw[ch] = bitmap[(r[ch].w & 0xffffffu) >> 5];
            if (valid[ch]) {                                       // the record's position: conditional or unconditional class
                const uint32_t q = r[ch].x - u * (uint32_t) kUnit;
                __hip_atomic_fetch_or(&cls[(((r[ch].y >> 8) & REC_COND) ? 0 : kW) + ((q >> 5) & (kW - 1))], 1u << (q & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
#pragma unroll
        for (int ch = 0; ch < CPU; ++ch) {
            if (hc[ch] == kNone) continue;                         // wave-uniform
            const uint32_t pos = r[ch].x, addr = r[ch].w;
            const int sk = (int) (int16_t) (r[ch].y >> 16), su = (int) (int16_t) (r[ch].z & 0xffffu);
            bool ok = valid[ch] && ((bw[ch] >> (addr & 31u)) & 1u);
            // Dominated records: an earlier try-phase of the same position with the same address and scores at least as good wins every
            // comparison the walk can make (same address = same filter answer, the best-phase test is a strict '>', demod_2400.c:246) —
            // typically 2 of the 3 records of a clean frame.
            // (Measured, round 5: one shuffle of the positions, the distances that occur at all from shifts of its ballot — records of
            // one position are neighbours —, the other shuffles only for those: 0.36 M fewer LDS instructions per launch of 1.36 M,
            // as many vector and scalar ones more, the pass as long as before, gpurun r05ai.)
            const uint64_t live0 = __ballot(ok);
            bool dom = false;
#pragma unroll
            for (int d = 1; d <= 4; ++d) {
                const uint32_t pj = __shfl_up(pos, d), aj = __shfl_up(addr, d);
                const int kj = __shfl_up(sk, d), uj = __shfl_up(su, d);
                if (lane >= d && ((live0 >> (lane - d)) & 1) && pj == pos && aj == addr && kj >= sk && uj >= su) dom = true;
            }
            ok = ok && !dom;
            const uint64_t m = __ballot(ok);
            if (lane == 0) {
                uint32_t *hw = (uint32_t *) &pool[hc[ch]];
                hw[4] = (uint32_t) m; hw[5] = (uint32_t) (m >> 32); hw[6] = run[ch];
            }
            run[ch] += (uint32_t) __popcll(m);
        }
        WAVE_SYNC();                                               // (the round ends for the whole wave: see write_unit_chains)
        if (h != kNone) h = hd.w;
        lim = (uint32_t) WAVE;
    }
    uint32_t mine = 0, nlive = 0;
#pragma unroll
    for (int ch = 0; ch < CPU; ++ch) { if (lane == ch) mine = run[ch]; nlive += run[ch]; }
    if (h_first != kNone) ((uint32_t *) &pool[h_first])[7] = mine;
    WAVE_SYNC();
    {
        static_assert(kW == 4 * WAVE, "four class words per lane");
        const u32x4 c0 = ((const u32x4 *) cls)[lane], uc = ((const u32x4 *) (cls + kW))[lane];
        const u32x4 cd = {c0.x & ~uc.x, c0.y & ~uc.y, c0.z & ~uc.z, c0.w & ~uc.w};
        ((u32x4 *) final_bitmap)[(size_t) u * (kW / 4) + lane] = cd;
        nc = (uint32_t) wave_sum_u64(__popc(cd.x) + __popc(cd.y) + __popc(cd.z) + __popc(cd.w));
        nu = (uint32_t) wave_sum_u64(__popc(uc.x) + __popc(uc.y) + __popc(uc.z) + __popc(uc.w));
    }
    return nlive;
}

template <int CPU>
__device__ __forceinline__ uint32_t write_unit_chains(uint32_t u, const PhaseRec *pool, const uint32_t *unit_first, uint32_t nunits, uint32_t dst0, PhaseRec *live) {
    static_assert(CPU == 1 || CPU == 4, "one or four chains per unit");
    const int lane = lane_id();
    if (u >= nunits) return 0;
    const uint64_t lt_mask = (1ull << lane) - 1;
    uint32_t h = kNone;
    if (lane < CPU) h = unit_first[u * CPU + (uint32_t) lane];
    // where the chains' records go: their totals are in their first headers, i.e. in the headers of the first round
    uint32_t base0 = dst0, base1 = 0, base2 = 0, base3 = 0, total = 0;
    bool first = true;
    while (__ballot(h != kNone)) {
        u32x4 hd0 = {0u, 0u, 0u, kNone}, hd1 = {0u, 0u, 0u, 0u};
        if (h != kNone) { hd0 = ((const u32x4 *) &pool[h])[0]; hd1 = ((const u32x4 *) &pool[h])[1]; }
        if (first) {
            first = false;
            const uint32_t t0 = (uint32_t) __builtin_amdgcn_readlane((int) hd1.w, 0);     // (a chain without records: the zero above)
            base1 = base0 + t0;
            total = t0;
            if (CPU == 4) {
                const uint32_t t1 = (uint32_t) __builtin_amdgcn_readlane((int) hd1.w, 1), t2 = (uint32_t) __builtin_amdgcn_readlane((int) hd1.w, 2),
                               t3 = (uint32_t) __builtin_amdgcn_readlane((int) hd1.w, 3);
                base2 = base1 + t1; base3 = base2 + t2;
                total = t0 + t1 + t2 + t3;
            }
        }
        // the live records of the round's segments: every load is issued before the first store
#define MGPU_WR_LOAD(ch, base) \
        const uint32_t hc##ch = (uint32_t) __builtin_amdgcn_readlane((int) h, ch); \
        const uint64_t m##ch = (uint64_t) (uint32_t) __builtin_amdgcn_readlane((int) hd1.x, ch) | ((uint64_t) (uint32_t) __builtin_amdgcn_readlane((int) hd1.y, ch) << 32); \
        const bool ok##ch = hc##ch != kNone && ((m##ch >> lane) & 1); \
        const uint32_t d##ch = (base) + (uint32_t) __builtin_amdgcn_readlane((int) hd1.z, ch) + (uint32_t) __popcll(m##ch & lt_mask); \
        u32x4 a##ch = {0u, 0u, 0u, 0u}, b##ch = {0u, 0u, 0u, 0u}; \
        if (ok##ch) { const u32x4 *src = (const u32x4 *) &pool[hc##ch + 1u + (uint32_t) lane]; a##ch = src[0]; b##ch = src[1]; }
#define MGPU_WR_STORE(ch) \
        if (ok##ch) { u32x4 *dd = (u32x4 *) &live[d##ch]; dd[0] = a##ch; dd[1] = b##ch; }
        MGPU_WR_LOAD(0, base0)
        if (CPU == 4) {
            MGPU_WR_LOAD(1, base1) MGPU_WR_LOAD(2, base2) MGPU_WR_LOAD(3, base3)
            MGPU_WR_STORE(0) MGPU_WR_STORE(1) MGPU_WR_STORE(2) MGPU_WR_STORE(3)
        } else {
            MGPU_WR_STORE(0)
        }
#undef MGPU_WR_LOAD
#undef MGPU_WR_STORE
        // The round ends for the whole wave here.  Without this the compiler carries the lanes that did NOT store the last chain's record
        // into the next rounds on their own and lets the others catch up afterwards (nested loops under complementary EXEC masks in the
        // ISA): the next round's header loads, ballots and readlanes then run without some of lanes 0-3 — records lost, wild addresses.
        WAVE_SYNC();
        if (h != kNone) h = hd0.w;
    }
    return total;
}

// COUNT pass: one wave per unit — which records live (left as masks in the segment headers), the unit's words of the class bitmap,
// and per workgroup one row of sums (live records: block_live; the two class counters: part[2 * block ..]) for the write pass, which adds
// them up: no scan kernel, no device atomics.
__global__ __launch_bounds__(kBlock) void k_count(PhaseRec *pool, uint32_t pool_cap, const uint32_t *unit_first, const uint32_t *first_count, uint32_t cpu, uint32_t nunits,
                                                  const uint32_t *bitmap, uint32_t *unit_live, uint32_t *block_live, uint32_t *final_bitmap,
                                                  unsigned long long *counters, uint32_t *part) {
    __shared__ uint32_t s_live[kBlock / WAVE], s_nc[kBlock / WAVE], s_nu[kBlock / WAVE];
    __shared__ __attribute__((aligned(16))) uint32_t s_cls[kBlock / WAVE][2 * (kUnit / 32)];
    const uint32_t wv = threadIdx.x >> 6, u = blockIdx.x * (kBlock / WAVE) + wv;
    uint32_t nlive, nc, nu;
    if (cpu == 4) nlive = count_unit_chains<4>(u, pool, pool_cap, unit_first, first_count, nunits, bitmap, counters, s_cls[wv], final_bitmap, nc, nu);
    else nlive = count_unit_chains<1>(u, pool, pool_cap, unit_first, nullptr, nunits, bitmap, counters, s_cls[wv], final_bitmap, nc, nu);
    if (lane_id() == 0) { s_live[wv] = nlive; s_nc[wv] = nc; s_nu[wv] = nu; if (u < nunits) unit_live[u] = nlive; }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_live[blockIdx.x] = s_live[0] + s_live[1] + s_live[2] + s_live[3];
        part[2 * blockIdx.x] = s_nc[0] + s_nc[1] + s_nc[2] + s_nc[3];
        part[2 * blockIdx.x + 1] = s_nu[0] + s_nu[1] + s_nu[2] + s_nu[3];
    }
}

// WRITE pass.  A workgroup's output offset = the live counts of all workgroups before it (block_live, at most a few
// thousand words out of L2, summed cooperatively) + those of the earlier units of its own four.
// SIG: with the records' signal powers (`mag`), one chain after the other; without, by chains — a kernel of its own, so that it does
// not carry the other's registers (`by_chains` false: the older form here too, for tests/test_gpu_prescreen_chains.py)
template <bool SIG>
__global__ __launch_bounds__(kBlock) void k_prescreen_write(PhaseRec *pool, const uint32_t *unit_first, uint32_t cpu, uint32_t nunits,
                                                            int by_chains, const uint32_t *unit_live, const uint32_t *block_live,
                                                            PhaseRec *live, const uint16_t *mag, unsigned long long *live_sig,
                                                            unsigned long long *counters, const uint32_t *fin_part, uint32_t nb_fin,
                                                            const uint32_t *slice_part, uint32_t slice_blocks) {
    __shared__ uint32_t s_part[kBlock / WAVE];
    if (blockIdx.x == 0 && slice_blocks) {        // k_slice's per-workgroup rows (records, candidates, phases 4/5, 6/7, 8) -> the counter block
        unsigned long long a[5] = {0, 0, 0, 0, 0};
        for (uint32_t r = threadIdx.x; r < slice_blocks; r += kBlock) {
#pragma unroll
            for (int k = 0; k < 5; ++k) a[k] += slice_part[r * kSlPartWords + k];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) a[k] = wave_sum_u64(a[k]);
        if (lane_id() == 0) {
            if (a[0]) atomicAdd(&counters[CNT_RECORDS], a[0]);
            if (a[1]) atomicAdd(&counters[CNT_CANDIDATES], a[1]);
            if (a[2]) { atomicAdd(&counters[CNT_PHASE0 + 0], a[2]); atomicAdd(&counters[CNT_PHASE0 + 1], a[2]); }
            if (a[3]) { atomicAdd(&counters[CNT_PHASE0 + 2], a[3]); atomicAdd(&counters[CNT_PHASE0 + 3], a[3]); }
            if (a[4]) atomicAdd(&counters[CNT_PHASE0 + 4], a[4]);
        }
    }
    if (blockIdx.x == 0 && nb_fin) {              // k_count's per-workgroup class counts -> the counter block
        unsigned long long a = 0, b = 0;
        for (uint32_t i = threadIdx.x; i < nb_fin; i += kBlock) { a += fin_part[2 * i]; b += fin_part[2 * i + 1]; }
        a = wave_sum_u64(a); b = wave_sum_u64(b);
        if (lane_id() == 0) {
            if (a) atomicAdd(&counters[CNT_CLASS_COND], a);
            if (b) atomicAdd(&counters[CNT_CLASS_UNCOND], b);
        }
    }
    uint32_t acc = 0;
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += kBlock) acc += block_live[i];
    acc = (uint32_t) wave_sum_u64(acc);
    const uint32_t wv = threadIdx.x >> 6;
    if (lane_id() == 0) s_part[wv] = acc;
    __syncthreads();
    uint32_t dst0 = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    const uint32_t u = blockIdx.x * (kBlock / WAVE) + wv;
    for (uint32_t v = blockIdx.x * (kBlock / WAVE); v < u && v < nunits; ++v) dst0 += unit_live[v];
    uint32_t nlive;
    if (!SIG && by_chains && cpu == 4) nlive = write_unit_chains<4>(u, pool, unit_first, nunits, dst0, live);
    else if (!SIG && by_chains) nlive = write_unit_chains<1>(u, pool, unit_first, nunits, dst0, live);
    else nlive = write_unit_sequential(u, pool, unit_first, cpu, nunits, dst0, live, SIG ? mag : nullptr, SIG ? live_sig : nullptr);
    if (u == nunits - 1 && lane_id() == 0) counters[CNT_LIVE_TOTAL] = dst0 + nlive;
}

// The chunk's scratch block (counters, pool cursor, per-buffer sums) goes to the host's pinned copy and is
// handed back zeroed for the slot's next chunk: replaces a D2H copy and a memset on the stream.
// (Round 5 folded it into the write pass's last workgroup — nothing another workgroup of that launch does enters the block, so no
// device-wide fence is needed — to save the kernel boundary: exact, and slower: the post-sweep stage 0.25 -> 0.29 ms per step, one
// workgroup pushing 17 KB over the PCIe link is a longer tail than this 5 us kernel on 9 workgroups.  gpurun r05u.)
__global__ __launch_bounds__(kBlock) void k_publish(unsigned long long *d_scratch, unsigned long long *h_scratch, uint32_t nwords, uint32_t *dealer) {
    if (blockIdx.x == 0 && dealer && threadIdx.x < 2 * kDealerCounters) dealer[threadIdx.x * kDealerStride] = 0;   // k_slice's counters, then k_sweep's
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < nwords; i += gridDim.x * kBlock) {
        h_scratch[i] = d_scratch[i];
        d_scratch[i] = 0;
    }
}

#if MGPU_EXPERIMENTS
// what count_unit_chains left in the headers against the chains walked one after the other (PostSweepParams::variant bit 2)
__global__ __launch_bounds__(kBlock) void k_prescreen_check(const PhaseRec *pool, const uint32_t *unit_first, uint32_t cpu, uint32_t nunits, const uint32_t *unit_live, unsigned long long *counters) {
    const uint32_t u = blockIdx.x * kBlock + threadIdx.x;
    if (u >= nunits) return;
    uint32_t all = 0;
    for (uint32_t ch = 0; ch < cpu; ++ch) {
        uint32_t h = unit_first[u * cpu + ch], run = 0, seg = 0;
        const uint32_t h0 = h;
        while (h != kNone) {
            const uint32_t *hw = (const uint32_t *) &pool[h];
            const uint64_t m = (uint64_t) hw[4] | ((uint64_t) hw[5] << 32);
            if (hw[6] != run && atomicAdd(&counters[CNT_DEBUG0], 1ull) < 8)
                printf("check: unit %u chain %u segment %u header %u: prefix %u, expected %u (cnt %u mask %llx next %u)\n", u, ch, seg, h, hw[6], run, hw[0], (unsigned long long) m, hw[3]);
            if (hw[0] < 64 && (m >> hw[0]) && atomicAdd(&counters[CNT_DEBUG0], 1ull) < 8)
                printf("check: unit %u chain %u segment %u header %u: mask %llx beyond cnt %u\n", u, ch, seg, h, (unsigned long long) m, hw[0]);
            run += (uint32_t) __popcll(m);
            h = hw[3];
            ++seg;
        }
        if (h0 != kNone && ((const uint32_t *) &pool[h0])[7] != run && atomicAdd(&counters[CNT_DEBUG0], 1ull) < 8)
            printf("check: unit %u chain %u first header %u: total %u, expected %u (%u segments)\n", u, ch, h0, ((const uint32_t *) &pool[h0])[7], run, seg);
        all += run;
    }
    if (all != unit_live[u] && atomicAdd(&counters[CNT_DEBUG0], 1ull) < 8) printf("check: unit %u: live %u, chains add up to %u\n", u, unit_live[u], all);
}
#endif

#if MGPU_EXPERIMENTS
// ... and the write pass's output against the chains walked one after the other
__global__ __launch_bounds__(kBlock) void k_prescreen_check_live(const PhaseRec *pool, const uint32_t *unit_first, uint32_t cpu, uint32_t nunits, const uint32_t *unit_live, const PhaseRec *live, unsigned long long *counters) {
    const uint32_t u = blockIdx.x * kBlock + threadIdx.x;
    if (u >= nunits) return;
    uint32_t d = 0;
    for (uint32_t v = 0; v < u; ++v) d += unit_live[v];
    if (u == 0) printf("live: checked %u units\n", nunits);
    for (uint32_t ch = 0; ch < cpu; ++ch) {
        uint32_t h = unit_first[u * cpu + ch], seg = 0;
        while (h != kNone) {
            const uint32_t *hw = (const uint32_t *) &pool[h];
            const uint64_t m = (uint64_t) hw[4] | ((uint64_t) hw[5] << 32);
            for (uint32_t i = 0; i < hw[0]; ++i) {
                if (!((m >> i) & 1)) continue;
                const uint32_t *a = (const uint32_t *) &pool[h + 1 + i], *b = (const uint32_t *) &live[d];
                bool same = true;
                for (int k = 0; k < 8; ++k) same = same && a[k] == b[k];
                if (!same && atomicAdd(&counters[CNT_DEBUG0 + 1], 1ull) < 12)
                    printf("live: unit %u chain %u segment %u header %u record %u of %u -> live[%u]: pos %u addr %06x, found pos %u addr %06x (mask %llx prefix %u total7 %u)\n",
                           u, ch, seg, h, i, hw[0], d, a[0], a[3], b[0], b[3], (unsigned long long) m, hw[6], hw[7]);
                ++d;
            }
            h = hw[3];
            ++seg;
        }
    }
}
#endif

// count on `s`; write + publish on `s_write` (== s, or a second stream), ordered after the count pass by `ev_scan`
int launch_prescreen(const PostSweepParams &q, hipStream_t s, hipStream_t s_write, hipEvent_t ev_scan) {
    if (q.nunits == 0) return 0;
    if (q.chains_per_unit != 4 && q.chains_per_unit != 1) return -1;
    const unsigned nb_count = (q.nunits + 3) / 4;
    const unsigned nb_fin = nb_count;             // rows of class counts
    hipLaunchKernelGGL(k_count, dim3(nb_count), dim3(kBlock), 0, s, q.pool, q.pool_cap, q.unit_first, q.first_count, q.chains_per_unit, q.nunits, q.adder_bitmap,
                       q.unit_live, q.block_live, q.class_final, q.counters, q.fin_part);
#if MGPU_EXPERIMENTS
    if (q.variant & 4) hipLaunchKernelGGL(k_prescreen_check, dim3((q.nunits + kBlock - 1) / kBlock), dim3(kBlock), 0, s, q.pool, q.unit_first, q.chains_per_unit, q.nunits, q.unit_live, q.counters);
#endif
    if (s_write != s) {
        if (hipEventRecord(ev_scan, s) != hipSuccess || hipStreamWaitEvent(s_write, ev_scan, 0) != hipSuccess) return -1;
    }
#define MGPU_WRITE_ARGS dim3(nb_count), dim3(kBlock), 0, s_write, q.pool, q.unit_first, q.chains_per_unit, q.nunits, (q.variant & 2) ? 1 : 0, \
                        q.unit_live, q.block_live, q.live, q.mag, q.live_sig, q.counters, q.fin_part, nb_fin, q.slice_part, q.slice_blocks
    if (q.mag) hipLaunchKernelGGL((k_prescreen_write<true>), MGPU_WRITE_ARGS);
    else hipLaunchKernelGGL((k_prescreen_write<false>), MGPU_WRITE_ARGS);
#undef MGPU_WRITE_ARGS
#if MGPU_EXPERIMENTS
    if (q.variant & 4) hipLaunchKernelGGL(k_prescreen_check_live, dim3((q.nunits + kBlock - 1) / kBlock), dim3(kBlock), 0, s_write, q.pool, q.unit_first, q.chains_per_unit, q.nunits, q.unit_live, q.live, q.counters);
#endif
    if (q.live_win)                               // (reads CNT_LIVE_TOTAL: before k_publish hands the counter block back zeroed)
        launch_live_windows(q.mag, q.n, q.cand, q.cand_count, q.class_final, q.live, q.counters + CNT_LIVE_TOTAL, q.buf_len, q.live_win, s_write);
    unsigned pb = (q.scratch_words + kBlock - 1) / kBlock;
    if (pb > 64) pb = 64;
    hipLaunchKernelGGL(k_publish, dim3(pb), dim3(kBlock), 0, s_write, q.d_scratch, q.h_scratch, q.scratch_words, q.dealer);
    return 0;
}
