// kernels/gate.inc — the first stage of the reference's tracker and its forwarding rule on the device (SURVEY.md §8(f).4), as far
// as both are decidable without the position tracker: per accepted message address_reliable (track.c:1688-1693), whether
// trackUpdateFromMessage finds / creates its aircraft and counts it (track.c:1905-1966: aircraftGet / aircraftCreate, a->seen, the
// 45 s rule, a->messages++), and outputMessage's rule over the batch a->messages is read after (net_io.c:5846-5849, 5924-5940):
//     forwarded  <=>  (crc == 0 && correctedbits == 0)  ||  (mm->aircraft && mm->aircraft->messages > 1)  ||  Mode A/C.
// What the position tracker decides — a position message judged bad or duplicate puts the aircraft's copy back, a->messages and
// a->seen with it (track.c:1917-1921, 2625-2627); an aircraft without a reliable position is deleted after 5 silent minutes
// (track.c:2856-2880) — is carried as BOUNDS: messages in [lo, hi], seen in [lo, hi], exists in [lo, hi] per aircraft, and a verdict
// is "deferred to the host's tracker" exactly when the bounds disagree about it.  oracle/modes_oracle_gate.c is the same arithmetic
// on the CPU; tests/golden/gate_*.npz hold what the whole reference program forwarded.
// Part of the single translation unit kernels.hip (included inside namespace mgpu, after the parts before it).
//
// The aircraft state is a direct-indexed table in HBM (2^25 addresses — 24 bits and MODES_NON_ICAO_ADDRESS — x 40 bytes = 1.25 GiB of
// 288: no hashing, no collisions, zero = unknown).  A message's fate depends on the messages of the SAME address before it, so the
// call's messages are brought into (address, stream order) by a stable radix sort on the address (three kernels per 8-bit digit: per-
// wave digit counts, one exclusive scan, the scatter with the ranks from 8 ballots per 64 keys), one wave then walks each address's
// run — 64 messages per step, the state machine as wave scans (k_gate_walk) — and a last kernel reads every message's batch-end counts.  Nothing here touches the sample path; it runs on the message list (~2 messages per 1000 samples).

struct GateAc {                  // 40 bytes; all zero = never seen
    long long seen_lo, seen_hi;  // a->seen, bounds (ms)
    long long cpr_first;         // the aircraft's first position message (0: none yet): the earliest a->seenPosReliable can be
    uint32_t cnt_lo, cnt_hi;     // a->messages, bounds
    uint32_t exists;             // bit 0: for certain, bit 1: possibly
    uint32_t pad;
};
struct GateInfo {                // 16 bytes per message of the call
    long long now;               // mm->sysTimestamp
    uint32_t batch;              // the sample buffer the message came out of ...
    uint32_t flags;              // GT_* | (rank among the buffer's Mode S messages >> 8) << 8: ... and which of its drainMessageBuffer batches of 256
};
enum : uint32_t { GT_MODEAC = 1, GT_RELIABLE = 2, GT_CPR = 4, GT_CLEAN = 8 };
constexpr uint32_t kGtAcMarker = 1u << 25;          // "address" of Mode A/C replies: behind every aircraft, never walked
constexpr long long kGtSeenTtl = 45000, kGtRemove = 5 * 60 * 1000;
// removeStaleRange's other rule (track.c:2835-2866): an aircraft WITH a reliable position goes once that position is older than an
// hour (30 minutes for non-ICAO addresses), however recently it was heard.  Which position was the last reliable one is the position
// tracker's knowledge; the earliest candidate is the aircraft's first position message, so from (first position message + the
// timeout) on the aircraft may have been deleted and re-created at any time: the lower bounds restart at every message, and whatever
// depends on them is answered "deferred".  (The reference's longer timeouts — --json-globe-index, --state-dir — only delete later.)
constexpr long long kGtPosTimeout = 60ll * 60 * 1000, kGtPosTimeoutNonIcao = 30ll * 60 * 1000;
constexpr int kGtBlocks = 32;                       // sorting workgroups (4 waves each): a wave owns one contiguous piece of the keys
constexpr int kGtWaves = kGtBlocks * (kBlock / WAVE);
// per sorted position, after the walk: bits 0-4 as the verdict's bits 2-4 (<< 2) | bit 5: cnt_lo > 1 | bit 6: cnt_hi > 1 (behind this message)

__device__ __forceinline__ uint64_t gate_segment(uint64_t n) { return ((n + kGtWaves - 1) / kGtWaves + WAVE - 1) / WAVE * WAVE; }

// ---- inputs: one key and one info record per message ----
__global__ __launch_bounds__(kBlock) void k_gate_prep(const mgpu_msg *msgs, const mgpu_fields *fields, uint64_t n, uint32_t buf_samples,
                                                      uint64_t *keys, GateInfo *info, uint8_t *verdict) {
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const mgpu_msg &m = msgs[i];
    const mgpu_fields &f = fields[i];
    const uint32_t mt = m.msgtype;
    const long long span = 5ll * buf_samples;
    const long long b = (m.timestamp - 772) / span;                              // timestamp = position * 5 + 768 + phase (4..8): demod_2400.c:406
    GateInfo g;
    g.now = m.sysTimestamp;
    if (mt == 77) {                                                             // DFTYPE_MODEAC: forwarded, no aircraft
        g.batch = 0; g.flags = GT_MODEAC;
        keys[i] = ((uint64_t) kGtAcMarker << 32) | i;
        verdict[i] = 1;
    } else {
        // the buffer's first message (the list is in stream order: its Mode S messages come first, its Mode A/C replies behind them)
        uint64_t lo = 0, hi = i;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((msgs[mid].timestamp - 772) / span < b) lo = mid + 1; else hi = mid;
        }
        const uint32_t addr = f.addr & 0x1ffffffu;
        const bool reliable = mt == 17 || mt == 18 || (mt == 11 && f.IID == 0);
        const bool crc_zero = reliable || (mt != 11 && mt != 17 && mt != 18 && (addr & 0xffffffu) == 0);   // Address/Parity formats: crc = the address
        g.batch = (uint32_t) b;
        g.flags = (reliable ? GT_RELIABLE : 0u) | ((f.flags & MGPU_F_CPR_VALID) ? GT_CPR : 0u) | ((crc_zero && m.correctedbits == 0) ? GT_CLEAN : 0u) |
                  ((uint32_t) ((i - lo) >> 8) << 8);
        keys[i] = ((uint64_t) addr << 32) | i;
    }
    info[i] = g;
}

// ---- stable LSD radix sort on the key's address bits, 8 bits per pass ----
// the lanes (among `valid`) whose digit equals this lane's: eight ballots
__device__ __forceinline__ uint64_t gate_match(uint32_t d, bool valid) {
    uint64_t mask = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        mask &= bit ? bal : ~bal;
    }
    return mask;
}

__global__ __launch_bounds__(kBlock) void k_gate_hist(const uint64_t *keys, uint64_t n, int shift, uint32_t *hist /* [256][kGtWaves] */) {
    __shared__ uint32_t s_cnt[kBlock / WAVE][256];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t w = blockIdx.x * (kBlock / WAVE) + wv;
    uint32_t *cnt = s_cnt[wv];
    for (int d = lane; d < 256; d += WAVE) cnt[d] = 0;
    WAVE_SYNC();
    const uint64_t seg = gate_segment(n), begin = w * seg, end = begin + seg < n ? begin + seg : n;
    for (uint64_t base = begin; base < end; base += WAVE) {
        const uint64_t i = base + lane;
        const bool valid = i < end;
        const uint32_t d = valid ? (uint32_t) (keys[i] >> shift) & 255u : 0u;
        const uint64_t mask = gate_match(d, valid);
        if (valid && lane == __ffsll((unsigned long long) mask) - 1) cnt[d] += (uint32_t) __popcll(mask);   // one leader per digit: distinct words
        WAVE_SYNC();
    }
    for (int d = lane; d < 256; d += WAVE) hist[(size_t) d * kGtWaves + w] = cnt[d];
}

// exclusive prefix sum over hist[256 * kGtWaves] in place, one workgroup: a thread's entries are consecutive
__global__ __launch_bounds__(kBlock) void k_gate_scan(uint32_t *hist) {
    constexpr int kPer = 256 * kGtWaves / kBlock;
    __shared__ uint32_t s_part[kBlock];
    uint32_t *mine = hist + (size_t) threadIdx.x * kPer;
    uint32_t sum = 0;
    for (int k = 0; k < kPer; ++k) sum += mine[k];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int t = 0; t < kBlock; ++t) { const uint32_t v = s_part[t]; s_part[t] = run; run += v; }
    }
    __syncthreads();
    uint32_t run = s_part[threadIdx.x];
    for (int k = 0; k < kPer; ++k) { const uint32_t v = mine[k]; mine[k] = run; run += v; }
}

__global__ __launch_bounds__(kBlock) void k_gate_scatter(const uint64_t *keys, uint64_t n, int shift, const uint32_t *hist, uint64_t *out) {
    __shared__ uint32_t s_base[kBlock / WAVE][256];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t w = blockIdx.x * (kBlock / WAVE) + wv;
    uint32_t *base_of = s_base[wv];
    for (int d = lane; d < 256; d += WAVE) base_of[d] = hist[(size_t) d * kGtWaves + w];
    WAVE_SYNC();
    const uint64_t lt_mask = (1ull << lane) - 1;
    const uint64_t seg = gate_segment(n), begin = w * seg, end = begin + seg < n ? begin + seg : n;
    for (uint64_t base = begin; base < end; base += WAVE) {
        const uint64_t i = base + lane;
        const bool valid = i < end;
        const uint64_t key = valid ? keys[i] : 0ull;
        const uint32_t d = (uint32_t) (key >> shift) & 255u;
        const uint64_t mask = gate_match(d, valid);
        uint32_t pos = 0;
        if (valid) pos = base_of[d] + (uint32_t) __popcll(mask & lt_mask);          // stable: lanes of one digit keep their order
        WAVE_SYNC();
        if (valid && lane == __ffsll((unsigned long long) mask) - 1) base_of[d] += (uint32_t) __popcll(mask);
        if (valid) out[pos] = key;
        WAVE_SYNC();
    }
}

// ---- the addresses' runs ----
__global__ __launch_bounds__(kBlock) void k_gate_runs(const uint64_t *keys, uint64_t n, uint32_t *runs, uint32_t *nruns) {
    const uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const uint32_t a = (uint32_t) (keys[k] >> 32);
    if (a >= kGtAcMarker) return;
    if (k == 0 || (uint32_t) (keys[k - 1] >> 32) != a) runs[atomicAdd(nruns, 1u)] = (uint32_t) k;
}

// One wave per run: trackUpdateFromMessage's first stage for every message of one address — 64 messages per step, as SCANS.
// Message by message the state machine is (oracle/modes_oracle_gate.c):
//     lo dies (exists_lo = 0, cnt_lo = 0, seen_lo = 0) if exists_lo && now - seen_lo > 5 min, or the position timeout above is over;
//     reliable address:  exists_lo = exists_hi = 1; seen_hi = now; cnt_hi++; not a position message: seen_lo = now; cnt_lo++;
//     else, aircraft possibly known:  ok_lo = exists_lo && now - seen_lo <= 45 s, ok_hi = now - seen_hi <= 45 s;  cnt_lo += ok_lo;
//                                     cnt_hi += ok_lo || ok_hi.
// Time does not run backwards in a stream, so every piece of it is a function of "the last ... before this message":
//     R = time of the last reliable message before (or the table's seen_hi), L = of the last reliable non-position message (seen_lo:
//     while lo is alive seen_lo IS L, and once now - L > 5 min it stays dead until the next such message sets L again), C = time of the
//     first position message;   dead = !(L && now - L <= 5 min) || (C && now - C > timeout);
//     cnt_hi = prefix sum of its increments;  cnt_lo = the sum of its increments since the last dead message, that one's included.
// R, L and C come from ballots (the lane of the last / first flagged message below) and one shuffle each, the sums from two DPP
// scans and one shuffle.  Round 5 stepped the machine once per message with wave-uniform values: 64 dependent steps of ~30
// instructions per 64 messages — 0.97 ms for 133 runs of 7 800 messages (profiles/r05_gate.txt).
__global__ __launch_bounds__(kBlock) void k_gate_walk(const uint64_t *keys, uint64_t n, const GateInfo *info, const uint32_t *runs, const uint32_t *nruns,
                                                      GateAc *table, uint8_t *res /* per sorted position */) {
    const int lane = lane_id();
    const uint64_t lt_mask = (1ull << lane) - 1, le_mask = lt_mask | (1ull << lane);
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = (gridDim.x * kBlock) >> 6;
    const uint32_t nr = *nruns;
    for (uint32_t r = wave; r < nr; r += nwaves) {
        const uint64_t k0 = runs[r];
        const uint32_t addr = (uint32_t) (keys[k0] >> 32);
        const GateAc st = table[addr];
        // carried from step to step (wave-uniform): the table's state in the scans' terms
        long long Lc = (st.exists & 1u) ? st.seen_lo : 0, Rc = ((st.exists >> 1) & 1u) ? st.seen_hi : 0, Cc = st.cpr_first;
        uint32_t cnt_lo = st.cnt_lo, cnt_hi = st.cnt_hi;
        bool ex_hi = (st.exists >> 1) & 1u;
        bool fin_ex_lo = st.exists & 1u;                                        // exists_lo / seen_lo as the message-by-message machine leaves them
        long long fin_seen_lo = st.seen_lo;
        const long long pos_timeout = (addr & (1u << 24)) ? kGtPosTimeoutNonIcao : kGtPosTimeout;
        // the keys two steps ahead and the inputs one step ahead are on their way while a step is computed
        auto load_key = [&](uint64_t kb) __attribute__((always_inline)) { const uint64_t k = kb + lane; return k < n ? keys[k] : ~0ull; };
        uint64_t key0 = load_key(k0), key1 = load_key(k0 + WAVE);
        GateInfo g0 = {0, 0, 0};
        if ((uint32_t) (key0 >> 32) == addr) g0 = info[(uint32_t) key0];
        for (uint64_t kb = k0;; kb += WAVE) {
            const uint64_t k = kb + lane;
            const bool mine = (uint32_t) (key0 >> 32) == addr;                    // (the run is contiguous: a prefix of the lanes; ~0: behind the list)
            const uint64_t m = __ballot(mine);
            const int cnt = __popcll(m);
            if (cnt == 0) break;                                                  // (a run of a whole number of steps)
            const GateInfo g = g0;
            const uint64_t key2 = cnt == WAVE ? load_key(kb + 2 * WAVE) : ~0ull;
            GateInfo g1 = {0, 0, 0};
            if (cnt == WAVE && (uint32_t) (key1 >> 32) == addr) g1 = info[(uint32_t) key1];
            const long long now = g.now;
            // a position message counts as one only with a reliable address (the aircraft's copy is kept, and cpr_first set, behind the
            // lookup that drops the others: track.c:1905-1921).  The field decode sets the flag on DF17 / DF18 alone; a caller's records need not
            const bool rel = mine && (g.flags & GT_RELIABLE), cpr = rel && (g.flags & GT_CPR);
            const uint64_t mr = __ballot(rel), mn = __ballot(rel && !cpr), mc = __ballot(cpr);
            // the last reliable / reliable non-position message below this lane, the first position message of all
            const uint64_t pr = mr & lt_mask, pn = mn & lt_mask;
            const int jr = pr ? 63 - __builtin_clzll(pr) : 0, jn = pn ? 63 - __builtin_clzll(pn) : 0;
            const long long Rs = __shfl(now, jr), Ls = __shfl(now, jn);
            const long long R = pr ? Rs : Rc, L = pn ? Ls : Lc;
            const bool exhi = ex_hi || pr != 0;
            const int jc = mc ? __ffsll((unsigned long long) mc) - 1 : 0;
            const long long Cfirst = __shfl(now, jc);
            const long long C = Cc ? Cc : ((mc && jc < lane) ? Cfirst : 0);
            const bool dead = !(L != 0 && now - L <= kGtRemove) || (C != 0 && now - C > pos_timeout);
            uint32_t v, inc_lo, inc_hi;
            if (rel) { inc_hi = 1; inc_lo = cpr ? 0u : 1u; v = 4u | 8u | 16u; }
            else {
                const bool ok_hi = exhi && now - R <= kGtSeenTtl, ok_lo = !dead && now - L <= kGtSeenTtl;
                inc_lo = ok_lo ? 1u : 0u; inc_hi = (ok_lo || ok_hi) ? 1u : 0u;
                v = (inc_hi ? 8u : 0u) | (ok_lo ? 16u : 0u);
            }
            if (!mine) { inc_lo = inc_hi = 0; v = 0; }
            int tot_hi, tot_lo;
            const int ph = wave_incl_scan_dpp((int) inc_hi, tot_hi), pl = wave_incl_scan_dpp((int) inc_lo, tot_lo);
            const uint64_t md = __ballot(mine && dead), pd = md & le_mask;
            const int jd = pd ? 63 - __builtin_clzll(pd) : 0;
            const int pl_d = __shfl(pl, jd), inc_d = __shfl((int) inc_lo, jd);
            const uint32_t c_hi = cnt_hi + (uint32_t) ph;
            const uint32_t c_lo = pd ? (uint32_t) (pl - pl_d + inc_d) : cnt_lo + (uint32_t) pl;
            v |= (c_lo > 1u ? 32u : 0u) | (c_hi > 1u ? 64u : 0u);
            if (mine) res[k] = (uint8_t) v;
            // the carries: the values behind the step's last message
            const int last = cnt - 1;
            cnt_hi = (uint32_t) __builtin_amdgcn_readlane((int) c_hi, last);
            cnt_lo = (uint32_t) __builtin_amdgcn_readlane((int) c_lo, last);
            {
                const bool dead_l = (md >> last) & 1ull, rel_l = (mr >> last) & 1ull, nonpos_l = (mn >> last) & 1ull;
                const long long L_l = __shfl(L, last), now_l = __shfl(now, last);
                fin_ex_lo = rel_l || !dead_l;
                fin_seen_lo = nonpos_l ? now_l : (dead_l ? 0 : L_l);
            }
            if (mn) Lc = __shfl(now, 63 - __builtin_clzll(mn));
            if (mr) { Rc = __shfl(now, 63 - __builtin_clzll(mr)); ex_hi = true; }
            if (!Cc && mc) Cc = Cfirst;
            if (cnt < WAVE) break;
            key0 = key1; key1 = key2; g0 = g1;
        }
        if (lane == 0) {
            GateAc o;
            o.seen_lo = fin_seen_lo; o.seen_hi = Rc; o.cpr_first = Cc; o.cnt_lo = cnt_lo; o.cnt_hi = cnt_hi;
            o.exists = (fin_ex_lo ? 1u : 0u) | (ex_hi ? 2u : 0u); o.pad = 0;
            table[addr] = o;
        }
    }
}

// outputMessage's rule, with a->messages as it stands behind the message's batch
__global__ __launch_bounds__(kBlock) void k_gate_verdict(const uint64_t *keys, uint64_t n, const GateInfo *info, const uint8_t *res, uint8_t *verdict) {
    const uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const uint64_t key = keys[k];
    const uint32_t addr = (uint32_t) (key >> 32), idx = (uint32_t) key;
    if (addr >= kGtAcMarker) return;                                               // Mode A/C: written by k_gate_prep
    const GateInfo g = info[idx];
    uint64_t e = k;                                                                // the last message of this address in this batch (<= 256 steps)
    for (; e + 1 < n && (uint32_t) (keys[e + 1] >> 32) == addr; ++e) {
        const GateInfo h = info[(uint32_t) keys[e + 1]];
        if (h.batch != g.batch || (h.flags >> 8) != (g.flags >> 8)) break;
    }
    const uint32_t own = res[k], end = res[e];
    uint32_t out;
    if (g.flags & GT_CLEAN) out = 1;
    else if (!(own & 8u)) out = 0;
    else if ((own & 16u) && (end & 32u)) out = 1;
    else if (!(end & 64u)) out = 0;
    else out = 2;
    verdict[idx] = (uint8_t) ((own & 0x1cu) | out);
}

size_t gate_table_bytes() { return ((size_t) 1 << 25) * sizeof(GateAc) + sizeof(GateAc) * 2; }
size_t gate_scratch_bytes(uint64_t n) {      // keys x 2, info, res, runs, hist + counter
    return (size_t) n * (8 + 8 + sizeof(GateInfo) + 1 + 4) + (size_t) (256 * kGtWaves + 64) * 4 + 256;
}

// msgs / fields / verdict in device memory; scratch = gate_scratch_bytes(n), table = gate_table_bytes() (zeroed once)
void launch_track_gate(const mgpu_msg *msgs, const mgpu_fields *fields, uint64_t n, uint32_t buf_samples, void *table, void *scratch,
                       uint8_t *verdict, hipStream_t s) {
    if (!n) return;
    uint8_t *p = (uint8_t *) scratch;
    uint64_t *keys_a = (uint64_t *) p; p += (size_t) n * 8;
    uint64_t *keys_b = (uint64_t *) p; p += (size_t) n * 8;
    GateInfo *info = (GateInfo *) p; p += (size_t) n * sizeof(GateInfo);
    uint32_t *runs = (uint32_t *) p; p += (size_t) n * 4;
    uint32_t *hist = (uint32_t *) p; p += (size_t) 256 * kGtWaves * 4;
    uint32_t *nruns = (uint32_t *) p; p += 256;
    uint8_t *res = p;
    const unsigned blocks = (unsigned) ((n + kBlock - 1) / kBlock);
    (void) hipMemsetAsync(nruns, 0, 4, s);
    hipLaunchKernelGGL(k_gate_prep, dim3(blocks), dim3(kBlock), 0, s, msgs, fields, n, buf_samples, keys_a, info, verdict);
    uint64_t *src = keys_a, *dst = keys_b;
    for (int shift = 32; shift < 64; shift += 8) {                                 // 26 address bits: 4 digits
        hipLaunchKernelGGL(k_gate_hist, dim3(kGtBlocks), dim3(kBlock), 0, s, src, n, shift, hist);
        hipLaunchKernelGGL(k_gate_scan, dim3(1), dim3(kBlock), 0, s, hist);
        hipLaunchKernelGGL(k_gate_scatter, dim3(kGtBlocks), dim3(kBlock), 0, s, src, n, shift, hist, dst);
        uint64_t *t = src; src = dst; dst = t;
    }
    hipLaunchKernelGGL(k_gate_runs, dim3(blocks), dim3(kBlock), 0, s, src, n, runs, nruns);
    unsigned wblocks = blocks < 1024u ? blocks : 1024u;
    hipLaunchKernelGGL(k_gate_walk, dim3(wblocks), dim3(kBlock), 0, s, src, n, info, runs, nruns, (GateAc *) table, res);
    hipLaunchKernelGGL(k_gate_verdict, dim3(blocks), dim3(kBlock), 0, s, src, n, info, res, verdict);
}
