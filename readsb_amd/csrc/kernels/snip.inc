// kernels/snip.inc — `readsb --snip <level>` (snipMode, readsb.c:1187-1206) over UC8 samples in HBM: every stretch of quiet samples is
// cut down to its first 32.  Part of the single translation unit kernels.hip (included inside namespace mgpu, after beast.inc, whose
// k_beast_scan it uses).
//
// A sample's fate depends on itself, on the 32 samples before it and on min(c, 33) of the reference's counter at the start of the
// call, so tiles of kSnipTile samples are independent given one word of halo; only where a tile's kept samples go is global.  A
// workgroup takes kSnipGroup consecutive tiles one after the other (the single-workgroup scan between the passes is as long as
// there are workgroups: fewer, larger entries keep it short).  Three passes, the shape of beast.inc and text.inc, and no workgroup
// ever waits for another:
//   k_snip_count  quiet flags from 16-byte loads (a byte of 8 flags per lane and load, put side by side in LDS so that 8 lanes' bytes
//                 read back as one 64-sample word), snip_keep_word() per word, the keep masks to HBM (1/16 of the input), per
//                 workgroup the number of kept samples and where its last loud sample is
//   k_beast_scan  kept counts -> offsets and the total; k_snip_last: the last loud sample of the call (the counter's next value)
//   k_snip_write  reads the keep masks, loads only the 16-byte groups that keep something, compacts them into LDS at the alignment
//                 (mod 16 bytes) the workgroup's output has in memory, and copies the tile's output as whole 16-byte vectors
//                 (2-byte stores before and after them): out + offset is only 2-byte aligned, the stores are coalesced all the same.

constexpr int kSnipTile = (int) kSnipTileSamples;            // samples per tile: what a workgroup holds at a time
constexpr int kSnipGroup = (int) (kSnipGroupSamples / kSnipTileSamples);   // tiles per workgroup
constexpr int kSnipWords = kSnipTile / 64;                   // 64-sample words per tile
constexpr int kSnipLoads = kSnipTile / 8 / kBlock;           // 16-byte loads per lane
static_assert(kSnipWords <= kBlock / 2 && kSnipWords % WAVE == 0 && kSnipLoads * kBlock * 8 == kSnipTile, "k_snip_*: waves 0-1 own the words");

// the quiet flags of 8 samples (16 bytes): bit j = sample j
__device__ __forceinline__ uint32_t snip_quiet8(SnipLevel lv, u32x4 v) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t w = v[j >> 1] >> (16 * (j & 1));
        m |= (snip_quiet(lv, w & 0xffu, (w >> 8) & 0xffu) ? 1u : 0u) << j;
    }
    return m;
}

// iq: 16-byte aligned.  masks: kSnipWords words per tile.  carry: snip_carry_word(c) of the call.
// block_kept[b]: samples the workgroup's tiles keep; block_last[b]: 1 + the index within them of their last loud sample, 0 = they have none.
__global__ __launch_bounds__(kBlock) void k_snip_count(const uint8_t *iq, uint64_t n, SnipLevel lv, uint64_t carry, unsigned long long *masks,
                                                       uint32_t *block_kept, uint32_t *block_last) {
    __shared__ __attribute__((aligned(8))) uint8_t s_q[8 + kSnipTile / 8];       // word 0: the halo, words 1..: the tile
    __shared__ uint32_t s_kept[2], s_last[2];
    uint32_t group_kept = 0, group_last = 0;                                     // thread 0's
    for (int t = 0; t < kSnipGroup; ++t) {
        const uint64_t tile = (uint64_t) blockIdx.x * kSnipGroup + t;
        const uint64_t base = tile * kSnipTile;
        if (base >= n) break;                                                    // (uniform)
        const uint8_t *src = iq + 2 * base;
#pragma unroll
        for (int u = 0; u < kSnipLoads; ++u) {
            const uint32_t g = u * kBlock + threadIdx.x;                         // group of 8 samples within the tile
            const uint64_t s0 = base + 8ull * g;
            uint32_t q = 0;
            if (s0 + 8 <= n) q = snip_quiet8(lv, *reinterpret_cast<const u32x4 *>(src + 16 * g));
            else
                for (uint32_t j = 0; j < 8; ++j)                                // the call's last, incomplete group: sample by sample
                    if (s0 + j < n) q |= (snip_quiet(lv, src[16 * g + 2 * j], src[16 * g + 2 * j + 1]) ? 1u : 0u) << j;
            s_q[8 + g] = (uint8_t) q;
        }
        if (threadIdx.x < 8 && tile) s_q[threadIdx.x] = (uint8_t) snip_quiet8(lv, *reinterpret_cast<const u32x4 *>(src - 128 + 16 * threadIdx.x));
        __syncthreads();
        if (threadIdx.x < kSnipWords) {                                          // waves 0 and 1, whole
            const uint32_t w = threadIdx.x;
            const unsigned long long *q64 = reinterpret_cast<const unsigned long long *>(s_q);
            const uint64_t first = base + 64ull * w;
            const uint64_t valid = first >= n ? 0ull : n - first >= 64 ? ~0ull : (1ull << (n - first)) - 1;
            const uint64_t prev = w || tile ? ~q64[w] : carry;
            const uint64_t loud = ~q64[w + 1] & valid;
            // (the flags beyond the call's end read as loud: they dilate only further beyond it)
            const uint64_t keep = snip_keep_word(prev, ~q64[w + 1]) & valid;
            masks[tile * kSnipWords + w] = keep;
            uint32_t kept = (uint32_t) __popcll(keep);
            uint32_t last = loud ? (uint32_t) t * kSnipTile + 64u * w + 64u - (uint32_t) __builtin_clzll(loud) : 0u;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                kept += __shfl_xor(kept, d);
                const uint32_t o = __shfl_xor(last, d);
                last = o > last ? o : last;
            }
            if (lane_id() == 0) { s_kept[w >> 6] = kept; s_last[w >> 6] = last; }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            group_kept += s_kept[0] + s_kept[1];
            const uint32_t last = s_last[1] ? s_last[1] : s_last[0];
            if (last) group_last = last;
        }
        // (thread 0 has read the sums before it passes the next round's first barrier, and they are stored again only behind it)
    }
    if (threadIdx.x == 0) { block_kept[blockIdx.x] = group_kept; block_last[blockIdx.x] = group_last; }
}

// 1 + the index of the call's last loud sample, 0 = the call has none (one workgroup)
__global__ __launch_bounds__(kScanThreads) void k_snip_last(const uint32_t *block_last, uint32_t nblocks, unsigned long long *last) {
    __shared__ unsigned long long s_part[kScanThreads / WAVE];
    unsigned long long m = 0;
    for (uint32_t k = threadIdx.x; k < nblocks; k += kScanThreads) {
        const uint32_t v = block_last[k];
        const unsigned long long at = (unsigned long long) k * kSnipGroupSamples + v;
        if (v && at > m) m = at;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(m, d);
        m = o > m ? o : m;
    }
    if (lane_id() == 0) s_part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kScanThreads / WAVE; ++k) m = s_part[k] > m ? s_part[k] : m;
        *last = m;
    }
}

// out: 2-byte aligned, cap samples.  Nothing is stored at or beyond out + 2 * cap.
__global__ __launch_bounds__(kBlock) void k_snip_write(const uint8_t *iq, uint64_t n, const unsigned long long *masks, const unsigned long long *block_off,
                                                       uint8_t *out, uint64_t cap) {
    __shared__ unsigned long long s_keep[kSnipWords];
    __shared__ uint32_t s_off[kSnipWords], s_wave[2];                            // a word's first kept sample among its wave's; the two waves' totals
    __shared__ __attribute__((aligned(16))) uint16_t s_out[kSnipTile + 8];
    unsigned long long obase = block_off[blockIdx.x];                            // samples: where the tile's output starts
    for (int t = 0; t < kSnipGroup; ++t) {
        const uint64_t tile = (uint64_t) blockIdx.x * kSnipGroup + t;
        const uint64_t base = tile * kSnipTile;
        if (base >= n) break;                                                    // (uniform)
        const uint8_t *src = iq + 2 * base;
        if (threadIdx.x < kSnipWords) {                                          // waves 0 and 1, whole
            const uint32_t w = threadIdx.x;
            const unsigned long long keep = masks[tile * kSnipWords + w];
            s_keep[w] = keep;
            int wtotal;
            s_off[w] = (uint32_t) wave_excl_scan((int) __popcll(keep), wtotal);
            if (lane_id() == 0) s_wave[w >> 6] = (uint32_t) wtotal;
        }
        __syncthreads();
        const uint32_t total = s_wave[0] + s_wave[1];
        // the tile's output lies in LDS at the alignment (mod 16 bytes) it will have in memory
        const uint32_t mis = (uint32_t) ((reinterpret_cast<uintptr_t>(out) + 2 * obase) & 15u) >> 1;
#pragma unroll
        for (int u = 0; u < kSnipLoads; ++u) {
            const uint32_t g = u * kBlock + threadIdx.x;                         // group of 8 samples within the tile
            const unsigned long long keep = s_keep[g >> 3];
            const uint32_t sh = 8 * (g & 7u);
            const uint32_t m = (uint32_t) (keep >> sh) & 0xffu;
            if (!m) continue;                                                    // nothing of it is kept: it is not loaded
            uint32_t at = mis + s_off[g >> 3] + (g >= 8 * WAVE ? s_wave[0] : 0u) + (uint32_t) __popcll(keep & ((1ull << sh) - 1));
            if (base + 8ull * g + 8 <= n) {
                const u32x4 v = *reinterpret_cast<const u32x4 *>(src + 16 * g);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (m & (1u << j)) s_out[at++] = (uint16_t) (v[j >> 1] >> (16 * (j & 1)));
            } else {
                for (uint32_t j = 0; j < 8; ++j)                                // (keep has no bit beyond the call's end)
                    if (m & (1u << j)) s_out[at++] = (uint16_t) (src[16 * g + 2 * j] | (uint32_t) src[16 * g + 2 * j + 1] << 8);
            }
        }
        __syncthreads();
        const uint32_t lo = mis, hi = mis + total;                               // s_out[lo .. hi) <-> dst[lo .. hi), dst 16-byte aligned
        uint16_t *dst = reinterpret_cast<uint16_t *>(out + 2 * obase) - mis;
        if (obase + total <= cap) {
            const uint32_t vlo = (lo + 7u) >> 3, vhi = hi >> 3;
            if (vhi > vlo) {
                const u32x4 *src128 = reinterpret_cast<const u32x4 *>(s_out);
                u32x4 *dst128 = reinterpret_cast<u32x4 *>(dst);
                for (uint32_t v = vlo + threadIdx.x; v < vhi; v += kBlock) dst128[v] = src128[v];
                if (threadIdx.x < 8) {                                            // at most seven samples before and after the vectors
                    const uint32_t h = lo + threadIdx.x, e = 8 * vhi + threadIdx.x;
                    if (h < 8 * vlo) dst[h] = s_out[h];
                    if (e < hi) dst[e] = s_out[e];
                }
            } else {
                for (uint32_t k = lo + threadIdx.x; k < hi; k += kBlock) dst[k] = s_out[k];
            }
        } else {                                                                 // the capacity cuts this tile (or lies before it): samples below it only
            for (uint32_t k = lo + threadIdx.x; k < hi; k += kBlock)
                if (obase + (k - mis) < cap) dst[k] = s_out[k];
        }
        obase += total;
        // (the next round stores s_keep, s_off and s_wave, which nobody reads behind the barrier above, and s_out only behind its own first barrier)
    }
}

void launch_snip(const uint8_t *iq, uint64_t n, int32_t level, uint64_t quiet_run, const SnipScratch &w, uint8_t *out, uint64_t cap, bool write, hipStream_t s) {
    if (n == 0) return;
    const unsigned blocks = (unsigned) ((n + kSnipGroupSamples - 1) / kSnipGroupSamples);
    hipLaunchKernelGGL(k_snip_count, dim3(blocks), dim3(kBlock), 0, s, iq, n, snip_level(level), snip_carry_word(quiet_run), w.masks, w.blocks, w.blocks + w.stride);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, w.blocks, blocks, w.off, w.total);
    hipLaunchKernelGGL(k_snip_last, dim3(1), dim3(kScanThreads), 0, s, w.blocks + w.stride, blocks, w.total + 1);
    if (write) hipLaunchKernelGGL(k_snip_write, dim3(blocks), dim3(kBlock), 0, s, iq, n, w.masks, w.off, out, cap);
}
