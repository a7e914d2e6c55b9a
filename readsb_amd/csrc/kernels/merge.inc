// kernels/merge.inc — the aggregator's time merge: the message lists of several receivers (segments, each anywhere in device memory)
// into one list ordered by timestamp, equal stamps in input order (lower segment first, then position) — numpy's
// argsort(kind="stable") over the concatenation, which is what readsb_amd/gather.py::merge_by_timestamp does on the host.
// Part of the single translation unit kernels.hip (included inside namespace mgpu, after the parts before it).
//
// A segment is NOT assumed sorted (with Mode A/C a receiver's list is only piecewise ordered), so this is a sort: the gate's scheme
// (kernels/gate.inc: LSD radix, 8 bits per pass, three kernels per pass, every wave owns one contiguous piece of the keys, ranks from 8
// ballots per 64 keys — stable by construction) on (u64 key, u32 index) pairs, a timestamp leaving no room for the index in the key.
// key = timestamp with the sign bit flipped (signed order as unsigned order).  k_merge_keys reads the records once for the keys and
// ORs together the bits in which they differ from the first one; the digit passes above the highest such bit are skipped (stamps of a
// few seconds of demodulation differ in ~28 bits: 4 passes of 8), and the first pass takes the index from the position instead of
// reading it.  k_merge_gather reads the records the second time: 4 lanes per 64-byte record.

constexpr int kMgMaxBlocks = 256;                   // sorting workgroups (4 waves each): as many as give every wave 256 keys, at most this

__host__ __device__ __forceinline__ uint32_t merge_blocks(uint64_t n) {
    const uint64_t b = (n + 4 * kBlock - 1) / (4 * kBlock);
    return b < 1 ? 1u : b > (uint64_t) kMgMaxBlocks ? (uint32_t) kMgMaxBlocks : (uint32_t) b;
}
__device__ __forceinline__ uint64_t merge_piece(uint64_t n, uint32_t nwaves) { return ((n + nwaves - 1) / nwaves + WAVE - 1) / WAVE * WAVE; }

// the segment position i of the concatenation lies in: the last one with start <= i (empty segments share a start: the last of them
// that is followed by a record is the one)
__device__ __forceinline__ uint32_t merge_find(const MergeSeg *segs, uint32_t nseg, uint64_t i) {
    uint32_t lo = 0, hi = nseg;                                 // segs[lo].start <= i < segs[hi].start (the list's length behind the last)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (segs[mid].start <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// first = the first record of the concatenation
__global__ __launch_bounds__(kBlock) void k_merge_keys(const MergeSeg *segs, uint32_t nseg, uint64_t n, const mgpu_msg *first, uint64_t *keys,
                                                       unsigned long long *diff) {
    __shared__ unsigned long long s_or[kBlock / WAVE];
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    unsigned long long d = 0;
    if (i < n) {
        const MergeSeg g = segs[merge_find(segs, nseg, i)];
        const uint64_t key = (uint64_t) g.msgs[i - g.start].timestamp ^ (1ull << 63);
        keys[i] = key;
        d = key ^ ((uint64_t) first->timestamp ^ (1ull << 63));
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) d |= __shfl_xor(d, k);
    if (lane_id() == 0) s_or[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long all = s_or[0] | s_or[1] | s_or[2] | s_or[3];
        if (all) atomicOr(diff, all);
    }
}

__global__ __launch_bounds__(kBlock) void k_merge_hist(const uint64_t *keys, uint64_t n, int shift, uint32_t *hist /* [256][nwaves] */) {
    __shared__ uint32_t s_cnt[kBlock / WAVE][256];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t nwaves = gridDim.x * (kBlock / WAVE), w = blockIdx.x * (kBlock / WAVE) + wv;
    uint32_t *cnt = s_cnt[wv];
    for (int d = lane; d < 256; d += WAVE) cnt[d] = 0;
    WAVE_SYNC();
    const uint64_t piece = merge_piece(n, nwaves), begin = w * piece < n ? w * piece : n, end = begin + piece < n ? begin + piece : n;
    for (uint64_t base = begin; base < end; base += WAVE) {
        const uint64_t i = base + lane;
        const bool valid = i < end;
        const uint32_t d = valid ? (uint32_t) (keys[i] >> shift) & 255u : 0u;
        const uint64_t mask = gate_match(d, valid);
        if (valid && lane == __ffsll((unsigned long long) mask) - 1) cnt[d] += (uint32_t) __popcll(mask);   // one leader per digit: distinct words
        WAVE_SYNC();
    }
    for (int d = lane; d < 256; d += WAVE) hist[(size_t) d * nwaves + w] = cnt[d];
}

// exclusive prefix sum over hist[entries] in place, one workgroup: a thread's entries are consecutive (entries = 256 * nwaves: a
// multiple of the 1024 threads)
__global__ __launch_bounds__(kScanThreads) void k_merge_scan(uint32_t *hist, uint32_t entries) {
    __shared__ uint32_t s_part[kScanThreads];
    const uint32_t per = entries / kScanThreads;
    uint32_t *mine = hist + (size_t) threadIdx.x * per;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < per; ++k) sum += mine[k];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const uint32_t add = (int) threadIdx.x >= d ? s_part[threadIdx.x - d] : 0u;
        __syncthreads();
        s_part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = s_part[threadIdx.x] - sum;
    for (uint32_t k = 0; k < per; ++k) { const uint32_t v = mine[k]; mine[k] = run; run += v; }
}

// FIRST: the pass that starts the sort — the index of a key is its position
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void k_merge_scatter(const uint64_t *keys, const uint32_t *idx, uint64_t n, int shift, const uint32_t *hist,
                                                          uint64_t *keys_out, uint32_t *idx_out) {
    __shared__ uint32_t s_base[kBlock / WAVE][256];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t nwaves = gridDim.x * (kBlock / WAVE), w = blockIdx.x * (kBlock / WAVE) + wv;
    uint32_t *base_of = s_base[wv];
    for (int d = lane; d < 256; d += WAVE) base_of[d] = hist[(size_t) d * nwaves + w];
    WAVE_SYNC();
    const uint64_t lt_mask = (1ull << lane) - 1;
    const uint64_t piece = merge_piece(n, nwaves), begin = w * piece < n ? w * piece : n, end = begin + piece < n ? begin + piece : n;
    for (uint64_t base = begin; base < end; base += WAVE) {
        const uint64_t i = base + lane;
        const bool valid = i < end;
        const uint64_t key = valid ? keys[i] : 0ull;
        const uint32_t src = FIRST ? (uint32_t) i : valid ? idx[i] : 0u;
        const uint32_t d = (uint32_t) (key >> shift) & 255u;
        const uint64_t mask = gate_match(d, valid);
        uint32_t pos = 0;
        if (valid) pos = base_of[d] + (uint32_t) __popcll(mask & lt_mask);          // stable: lanes of one digit keep their order
        WAVE_SYNC();
        if (valid && lane == __ffsll((unsigned long long) mask) - 1) base_of[d] += (uint32_t) __popcll(mask);
        if (valid && pos < n) { keys_out[pos] = key; idx_out[pos] = src; }
        WAVE_SYNC();
    }
}

// output record i = record idx[i] of the concatenation (idx == nullptr: i itself); 4 lanes per record, 16 bytes each
__global__ __launch_bounds__(kBlock) void k_merge_gather(const MergeSeg *segs, uint32_t nseg, uint64_t n, const uint32_t *idx, mgpu_msg *out,
                                                         uint64_t *perm, uint64_t *ids, uint8_t *verdict_out) {
    const uint64_t t = (uint64_t) blockIdx.x * kBlock + threadIdx.x, i = t >> 2;
    const uint32_t part = (uint32_t) t & 3u;
    if (i >= n) return;
    const uint64_t src = idx ? idx[i] : i;
    const MergeSeg g = segs[merge_find(segs, nseg, src)];
    const uint64_t k = src - g.start;
    reinterpret_cast<u32x4 *>(out + i)[part] = reinterpret_cast<const u32x4 *>(g.msgs + k)[part];
    if (part == 0) {
        if (perm) perm[i] = src;
        if (ids) ids[i] = g.id;
        if (verdict_out) verdict_out[i] = g.verdict ? g.verdict[k] : 0;
    }
}

// scratch: keys x 2, indices x 2, hist, the segment table, the diff word
static size_t merge_align(size_t v) { return (v + 255) & ~(size_t) 255; }
struct MergeScratch {
    uint64_t *keys_a, *keys_b;
    uint32_t *idx_a, *idx_b, *hist;
    MergeSeg *segs;
    unsigned long long *diff;
    size_t bytes;
};
static MergeScratch merge_layout(void *scratch, uint64_t n, uint32_t nseg) {
    MergeScratch m;
    uint8_t *p = (uint8_t *) scratch;
    m.keys_a = (uint64_t *) p; p += merge_align((size_t) n * 8);
    m.keys_b = (uint64_t *) p; p += merge_align((size_t) n * 8);
    m.idx_a = (uint32_t *) p; p += merge_align((size_t) n * 4);
    m.idx_b = (uint32_t *) p; p += merge_align((size_t) n * 4);
    m.hist = (uint32_t *) p; p += merge_align((size_t) 256 * kMgMaxBlocks * (kBlock / WAVE) * 4);
    m.segs = (MergeSeg *) p; p += merge_align((size_t) (nseg + 1) * sizeof(MergeSeg));
    m.diff = (unsigned long long *) p; p += 256;
    m.bytes = (size_t) (p - (uint8_t *) scratch);
    return m;
}
size_t merge_scratch_bytes(uint64_t n, uint32_t nseg) { return merge_layout(nullptr, n, nseg).bytes; }

// first half: the segment table to the device, the keys, and the bits they differ in -> the returned device word (n > 0, nseg > 0)
const unsigned long long *launch_merge_keys(const MergeSeg *h_segs, uint32_t nseg, uint64_t n, void *scratch, hipStream_t s) {
    const MergeScratch m = merge_layout(scratch, n, nseg);
    (void) hipMemcpyAsync(m.segs, h_segs, (size_t) nseg * sizeof(MergeSeg), hipMemcpyHostToDevice, s);
    (void) hipMemsetAsync(m.diff, 0, 8, s);
    const mgpu_msg *first = nullptr;
    for (uint32_t k = 0; k < nseg && !first; ++k)
        if (h_segs[k].start < (k + 1 < nseg ? h_segs[k + 1].start : n)) first = h_segs[k].msgs;
    hipLaunchKernelGGL(k_merge_keys, dim3((unsigned) ((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, m.segs, nseg, n, first, m.keys_a, m.diff);
    return m.diff;
}

// second half, `diff` read back: the digit passes up to its highest bit, the gather.  Returns the number of passes
int launch_merge_sort(uint32_t nseg, uint64_t n, uint64_t diff, void *scratch, mgpu_msg *out, uint64_t *perm, uint64_t *ids, uint8_t *verdict_out,
                      hipStream_t s) {
    const MergeScratch m = merge_layout(scratch, n, nseg);
    const unsigned blocks = merge_blocks(n);
    const uint32_t entries = 256u * blocks * (kBlock / WAVE);
    int passes = 0;
    while (passes < 8 && (diff >> (8 * passes))) ++passes;
    uint64_t *ksrc = m.keys_a, *kdst = m.keys_b;
    uint32_t *isrc = m.idx_a, *idst = m.idx_b;
    for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(k_merge_hist, dim3(blocks), dim3(kBlock), 0, s, ksrc, n, 8 * p, m.hist);
        hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(kScanThreads), 0, s, m.hist, entries);
        if (p == 0) hipLaunchKernelGGL(k_merge_scatter<true>, dim3(blocks), dim3(kBlock), 0, s, ksrc, nullptr, n, 0, m.hist, kdst, idst);
        else hipLaunchKernelGGL(k_merge_scatter<false>, dim3(blocks), dim3(kBlock), 0, s, ksrc, isrc, n, 8 * p, m.hist, kdst, idst);
        uint64_t *tk = ksrc; ksrc = kdst; kdst = tk;
        uint32_t *ti = isrc; isrc = idst; idst = ti;
    }
    hipLaunchKernelGGL(k_merge_gather, dim3((unsigned) ((4 * n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, m.segs, nseg, n, passes ? isrc : nullptr, out,
                       perm, ids, verdict_out);
    return passes;
}
