// kernels/convert.inc — IQ -> magnitude converters (convert.c).
// Part of the single translation unit kernels.hip (included inside namespace mgpu, after the parts before it).

// =============================================================================================
// IQ -> magnitude
// =============================================================================================

// Per-thread running (level, power) sums for the buffer the thread is currently inside.  A thread
// that crosses a 131072-sample buffer boundary, or ends, folds its sums into workgroup accumulators
// in LDS (a workgroup's contiguous range touches kBlockBufs buffers at most in the usual geometry;
// anything beyond goes to memory directly); one thread per touched buffer then issues the
// device-scope atomics.  One RMW per thread was ~5x10^5 memory-side atomics on <= 1024 addresses per
// launch and cost more than the conversion itself.
constexpr int kBlockBufs = 4;
struct BlockSums {
    unsigned long long level[kBlockBufs], power[kBlockBufs];
    double flevel[kBlockBufs], fpower[kBlockBufs];
    uint32_t first;          // buffer index of slot 0
};

struct BufSums {
    unsigned long long level, power;
    uint64_t next_boundary;   // first sample index of the next buffer
    uint32_t cur;             // current buffer index
    BlockSums *blk;
    __device__ void init(uint64_t sample, uint32_t B, BlockSums *b) {
        cur = (uint32_t) (sample / B);
        next_boundary = (uint64_t) (cur + 1) * B;
        level = power = 0;
        blk = b;
    }
    __device__ void flush(const ConvertParams &p) {
        if (level | power) {
            const uint32_t k = cur - blk->first;
            if (k < (uint32_t) kBlockBufs) {
                atomicAdd(&blk->level[k], level);
                atomicAdd(&blk->power[k], power);
            } else {
                atomicAdd(&p.sum_level[cur], level);
                atomicAdd(&p.sum_power[cur], power);
            }
        }
        level = power = 0;
    }
    __device__ void advance_to(uint64_t sample, const ConvertParams &p) {
        while (sample >= next_boundary) {
            flush(p);
            ++cur;
            next_boundary += p.buf_samples;
        }
    }
};

__device__ __forceinline__ void block_sums_init(BlockSums &b, uint64_t first_sample, uint32_t B) {
    if (threadIdx.x < kBlockBufs) {
        b.level[threadIdx.x] = b.power[threadIdx.x] = 0;
        b.flevel[threadIdx.x] = b.fpower[threadIdx.x] = 0.0;
    }
    if (threadIdx.x == 0) b.first = (uint32_t) (first_sample / B);
}

// d_mag[0 .. 326) = the 326 magnitudes that preceded this chunk (sdr_ifile.c:209-213): copied from the
// end of the previous chunk's magnitude buffer (p.tail) or zero at stream start, by workgroup 0.
__device__ __forceinline__ void convert_tail_prologue(const ConvertParams &p) {
    if (blockIdx.x != 0) return;
    for (int i = threadIdx.x; i < kTrailing; i += kBlock) p.mag[i] = p.tail ? p.tail[i] : (uint16_t) 0;
}

// UC8: magnitude = table[I | Q<<8] (convert.c:64-108).  The 65536-entry table has two mirror
// symmetries (I -> 255-I, Q -> 255-Q) so a 128x128 quadrant, padded to an odd-ish row stride,
// is staged in LDS (33 KB) and every sample is one ds_read_u16.
// Thread work item: one 16-byte-aligned chunk of 8 output magnitudes d_mag[8c .. 8c+8) =
// samples 8c-326 .. 8c-319; the 16 IQ bytes are one (4-byte aligned) global_load_dwordx4.
__global__ __launch_bounds__(kBlock) void k_convert_uc8(ConvertParams p) {
    __shared__ __attribute__((aligned(16))) uint16_t s_lut[128 * UC8_FOLD_STRIDE];
    {   // 33 KB table: all of a thread's 16-byte loads are issued before the first LDS store
        constexpr int kVec = 128 * UC8_FOLD_STRIDE / 8;                 // 2080 x 16 B
        constexpr int kPer = (kVec + kBlock - 1) / kBlock;
        u32x4 t[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) { const int i = threadIdx.x + k * kBlock; if (i < kVec) t[k] = ((const u32x4 *) p.uc8_folded)[i]; }
#pragma unroll
        for (int k = 0; k < kPer; ++k) { const int i = threadIdx.x + k * kBlock; if (i < kVec) ((u32x4 *) s_lut)[i] = t[k]; }
    }
    convert_tail_prologue(p);

    const uint64_t c_first = kTrailing / 8;                       // chunk holding d_mag[326]
    const uint64_t c_end = (kTrailing + p.n + 7) / 8;
    const uint64_t nchunks = c_end - c_first;
    uint64_t per_block = (nchunks + gridDim.x - 1) / gridDim.x;
    per_block = (per_block + kBlock - 1) / kBlock * kBlock;
    const uint64_t blk_lo = c_first + (uint64_t) blockIdx.x * per_block;
    const uint64_t blk_hi = blk_lo + per_block < c_end ? blk_lo + per_block : c_end;
    if (blk_lo >= c_end) return;                                  // workgroup-uniform
    __shared__ BlockSums s_sums;
    {
        const int64_t b0 = (int64_t) blk_lo * 8 - kTrailing;
        block_sums_init(s_sums, b0 < 0 ? 0 : (uint64_t) b0, p.buf_samples);
    }
    __syncthreads();

    BufSums sums;
    {
        int64_t s0 = (int64_t) (blk_lo + threadIdx.x) * 8 - kTrailing;
        sums.init(s0 < 0 ? 0 : (uint64_t) s0, p.buf_samples, &s_sums);
    }
    // Two 16-byte loads per lane in flight: at 4 waves/SIMD one load per lane is 4 MB in flight on the whole chip, a
    // quarter of what 8 TB/s x ~2 us of HBM latency asks for.  (A third — the chunk after next — measured WORSE in round 5:
    // 0.52 against 0.40 ms per 537 M samples, gpurun r05l.)
    u32x4_a4 pre = {0, 0, 0, 0};
    bool pre_ok = false;
    for (uint64_t c = blk_lo + threadIdx.x; c < blk_hi; c += kBlock) {
        const int64_t i0 = (int64_t) c * 8 - kTrailing;   // sample index of element 0
        uint32_t w[4];
        const bool full = i0 >= 0 && (uint64_t) i0 + 8 <= p.n;
        u32x4_a4 v = pre;
        if (full && !pre_ok) v = *(const u32x4_a4 *) (p.iq + 2 * i0);
        {
            const uint64_t cn = c + kBlock;
            const int64_t in = (int64_t) cn * 8 - kTrailing;
            pre_ok = cn < blk_hi && in >= 0 && (uint64_t) in + 8 <= p.n;
            if (pre_ok) pre = *(const u32x4_a4 *) (p.iq + 2 * in);
        }
        if (full) {
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t x = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    int64_t byte = 2 * i0 + 4 * d + b;
                    if (byte >= 0 && (uint64_t) byte < 2 * p.n) x |= (uint32_t) p.iq[byte] << (8 * b);
                }
                w[d] = x;
            }
        }
        uint32_t out[4];
        uint32_t lvl = 0;
        unsigned long long pw = 0;
        uint16_t m[8];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            // fold all four bytes: v >= 128 ? v - 128 : 127 - v
            const uint32_t hi = (w[d] >> 7) & 0x01010101u;
            const uint32_t f = (w[d] ^ 0x7F7F7F7Fu ^ (hi * 0x7Fu)) & 0x7F7F7F7Fu;
            const uint32_t a0 = f & 0xff, b0 = (f >> 8) & 0xff, a1 = (f >> 16) & 0xff, b1 = f >> 24;
            m[2 * d] = s_lut[a0 * UC8_FOLD_STRIDE + b0];
            m[2 * d + 1] = s_lut[a1 * UC8_FOLD_STRIDE + b1];
            out[d] = (uint32_t) m[2 * d] | ((uint32_t) m[2 * d + 1] << 16);
        }
        if (full) {
            if ((uint64_t) i0 + 7 >= sums.next_boundary || (uint64_t) i0 < sums.next_boundary - p.buf_samples) {
                // chunk straddles (or jumps) a buffer boundary: element-wise
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    sums.advance_to((uint64_t) i0 + e, p);
                    sums.level += m[e];
                    sums.power += (unsigned long long) m[e] * m[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) { lvl += m[e]; pw += (unsigned long long) ((uint32_t) m[e] * (uint32_t) m[e]); }
                sums.level += lvl;
                sums.power += pw;
            }
            u32x4 o = {out[0], out[1], out[2], out[3]};
            *(u32x4 *) (p.mag + c * 8) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int64_t i = i0 + e;
                if (i >= 0 && (uint64_t) i < p.n) {
                    sums.advance_to((uint64_t) i, p);
                    sums.level += m[e];
                    sums.power += (unsigned long long) m[e] * m[e];
                    p.mag[c * 8 + e] = m[e];
                }
            }
        }
    }
    sums.flush(p);
    __syncthreads();
    if (threadIdx.x < kBlockBufs && (s_sums.level[threadIdx.x] | s_sums.power[threadIdx.x])) {
        atomicAdd(&p.sum_level[s_sums.first + threadIdx.x], s_sums.level[threadIdx.x]);
        atomicAdd(&p.sum_power[s_sums.first + threadIdx.x], s_sums.power[threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------------------------
// k_convert_uc8_lean (round 6): the same conversion at a third of the instructions.
//
// k_convert_uc8 above is HBM-bound on its own (5.4 TB/s), but it issues 17.6 lane-operations per sample — 37 M wave-instructions
// per 1024-buffer chunk in a pipeline whose every other kernel is bound by instruction issue — and what it issues is what it costs
// the kernels it runs beside (DESIGN.md §3 "the bound is instruction issue").  Where they went:
//   * 64-bit chunk / sample indices, a `full` test and a buffer-boundary test per chunk: here a workgroup's range is a whole number
//     of iterations of kBlock chunks, the chunk that straddles a buffer boundary is always thread 0's (326 = 8 * 40 + 6 and a
//     buffer is a multiple of 2048 samples: sample k * B is element 6 of chunk 40 + k * B / 8), so the boundary is ONE scalar
//     compare per iteration, and the two chunks of a launch that are not whole (the stream's head: samples -6 .. 1; the ragged
//     end) are one lane's detour;
//   * the fold with a multiply (`hi * 0x7f` with hi = 0x01010101 is v_mul_lo_u32, quarter rate): a folded byte is
//     v ^ (0x7f + (v >> 7)) — 127 - v below 128, v - 128 from there — four full-rate operations per four bytes;
//   * index arithmetic (two extracts, a multiply-add per sample): the quadrant sits in LDS with row stride 128 and is symmetric,
//     so the BYTE address of a sample's entry is (q << 8) | (i << 1) = the folded pair + its own low byte: one SDWA add;
//   * the sums: sum(m) and sum(m^2) as u64 per sample cost 5-6 operations (a 32-bit multiply and a carry chain).  Here four
//     magnitudes are split into their high and low bytes (two v_perm) and sum(h h), sum(h l), sum(l l), sum(h), sum(l) each take
//     one v_dot4_u32_u8 per four samples into 32-bit accumulators: m = 256 h + l, m^2 = 65536 h^2 + 512 h l + l^2, exact, and a
//     lane's accumulators hold 2^14 such steps (65536 samples; a workgroup folds them at every buffer boundary and every
//     kCvFlushEvery iterations at the latest);
//   * two magnitudes share a register through ds_read_u16_d16 / _d16_hi (no pack).
// kCvDepth 16-byte loads per lane in flight: beside k_slice (the side stream, api.cpp) the converter has one wave per SIMD
// and has to keep its share of the memory system busy from there.
// Requires buf_samples % 2048 == 0 and n < 2^34 (launch_convert falls back to k_convert_uc8 otherwise).
// ---------------------------------------------------------------------------------------------
#ifndef MGPU_CV_DEPTH
#define MGPU_CV_DEPTH 4
#endif
constexpr int kCvDepth = MGPU_CV_DEPTH;
constexpr uint32_t kCvFlushEvery = 4096;                      // iterations (8 samples per lane each) between two folds of a lane's accumulators, at most

struct CvAcc { uint32_t hh, hl, ll, h, l; };

__device__ __forceinline__ void cv_acc4(CvAcc &a, uint32_t m0, uint32_t m1) {    // four magnitudes: (m0.lo, m0.hi, m1.lo, m1.hi)
    const uint32_t H = __builtin_amdgcn_perm(m1, m0, 0x07050301u), L = __builtin_amdgcn_perm(m1, m0, 0x06040200u);
    a.hh = __builtin_amdgcn_udot4(H, H, a.hh, false);
    a.hl = __builtin_amdgcn_udot4(H, L, a.hl, false);
    a.ll = __builtin_amdgcn_udot4(L, L, a.ll, false);
    a.h = __builtin_amdgcn_udot4(H, 0x01010101u, a.h, false);
    a.l = __builtin_amdgcn_udot4(L, 0x01010101u, a.l, false);
}
__device__ __forceinline__ unsigned long long cv_level(const CvAcc &a) { return 256ull * a.h + a.l; }
__device__ __forceinline__ unsigned long long cv_power(const CvAcc &a) { return 65536ull * a.hh + 512ull * a.hl + a.ll; }

// two samples (bytes I0 Q0 I1 Q1 of w) -> their magnitudes, packed
__device__ __forceinline__ uint32_t cv_lookup2(const uint16_t *lut, uint32_t w) {
    const uint32_t f = w ^ (((w >> 7) & 0x01010101u) + 0x7f7f7f7fu);          // every byte folded to 0..127
    uint32_t a0, a1;                                                           // byte offsets of the two entries: q << 8 | i << 1
    asm("v_add_u32_sdwa %0, %1, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:BYTE_0" : "=v"(a0) : "v"(f));
    asm("v_add_u32_sdwa %0, %1, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:BYTE_2" : "=v"(a1) : "v"(f));
    v2u16 m;
    m.x = *(const uint16_t *) ((const uint8_t *) lut + a0);
    m.y = *(const uint16_t *) ((const uint8_t *) lut + a1);
    return __builtin_bit_cast(uint32_t, m);
}

// The workgroup's accumulators -> buffer `buf` (every thread calls it; s_acc: two zeroed LDS words, left zeroed)
__device__ __noinline__ void cv_flush(CvAcc acc, unsigned long long *s_acc, unsigned long long *sum_level, unsigned long long *sum_power, int32_t buf) {
    const unsigned long long lv = wave_sum_u64(cv_level(acc)), pw = wave_sum_u64(cv_power(acc));
    if (lane_id() == 0 && (lv | pw)) { atomicAdd(&s_acc[0], lv); atomicAdd(&s_acc[1], pw); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tl = s_acc[0], tp = s_acc[1];
        s_acc[0] = s_acc[1] = 0;                                               // (before the barrier: the next flush may follow at once)
        if (buf >= 0 && (tl | tp)) { atomicAdd(&sum_level[buf], tl); atomicAdd(&sum_power[buf], tp); }
    }
    __syncthreads();
}

// One iteration (kBlock chunks from c0 on) the slow, general way: the iterations that hold the stream's head chunk (samples -6 .. 1:
// d_mag[320 .. 326) is the tail's), the ragged end, lanes behind the end, or a chunk that straddles two buffers (thread 0's: elements
// 0..5 are the last six samples of buffer `buf`, the rest of the iteration belongs to buf + 1).  A launch has a handful of them.
__device__ __noinline__ void cv_slow_iter(const uint8_t *iq, uint16_t *mag, uint64_t n, const uint16_t *lut, unsigned long long *s_acc,
                                          unsigned long long *sum_level, unsigned long long *sum_power, uint32_t c0, int32_t buf, bool boundary) {
    const uint32_t c = c0 + threadIdx.x;
    const uint32_t c_end = (uint32_t) ((kTrailing + n + 7) / 8);
    CvAcc lo = {0, 0, 0, 0, 0}, hi = {0, 0, 0, 0, 0};                            // sums for buf / for buf + 1 (boundary iterations only)
    if (c < c_end) {
        uint32_t w[4] = {0, 0, 0, 0}, valid = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t i = 8 * (int64_t) c - kTrailing + e;
            if (i >= 0 && (uint64_t) i < n) {
                valid |= 1u << e;
                w[e >> 1] |= ((uint32_t) iq[2 * i] | ((uint32_t) iq[2 * i + 1] << 8)) << (16 * (e & 1));
            }
        }
        uint32_t m[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            m[d] = cv_lookup2(lut, w[d]);
            // (elements that are not samples: no store, nothing for the sums)
            m[d] &= ((valid >> (2 * d)) & 1u ? 0xffffu : 0u) | ((valid >> (2 * d + 1)) & 1u ? 0xffff0000u : 0u);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if ((valid >> e) & 1u) mag[8 * (uint64_t) c + e] = (uint16_t) (m[e >> 1] >> (16 * (e & 1)));
        if (boundary && threadIdx.x == 0) { cv_acc4(lo, m[0], m[1]); cv_acc4(lo, m[2], 0u); cv_acc4(hi, m[3], 0u); }
        else if (boundary) { cv_acc4(hi, m[0], m[1]); cv_acc4(hi, m[2], m[3]); }
        else { cv_acc4(lo, m[0], m[1]); cv_acc4(lo, m[2], m[3]); }
    }
    cv_flush(lo, s_acc, sum_level, sum_power, buf);
    if (boundary) cv_flush(hi, s_acc, sum_level, sum_power, buf + 1);
}

__global__ __launch_bounds__(kBlock) void k_convert_uc8_lean(ConvertParams p) {
    __shared__ __attribute__((aligned(16))) uint16_t s_lut[128 * 128];
    __shared__ unsigned long long s_acc[2];
    {   // 32 KB table: all of a thread's 16-byte loads are issued before the first LDS store
        constexpr int kVec = 128 * 128 / 8, kPer = kVec / kBlock;              // 2048 x 16 B, 8 per thread
        const u32x4 *src = (const u32x4 *) (p.uc8_folded + UC8_SYM_OFFSET);
        u32x4 t[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) t[k] = src[threadIdx.x + k * kBlock];
#pragma unroll
        for (int k = 0; k < kPer; ++k) ((u32x4 *) s_lut)[threadIdx.x + k * kBlock] = t[k];
        if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    }
    convert_tail_prologue(p);
    const uint32_t tid = threadIdx.x;
    const uint32_t c_first = kTrailing / 8;                                    // chunk 40 holds d_mag[320 .. 328): samples -6 .. 1
    const uint32_t c_end = (uint32_t) ((kTrailing + p.n + 7) / 8);
    const uint32_t c_whole_end = (uint32_t) ((kTrailing + p.n) / 8);           // chunks c_first < c < c_whole_end have all eight samples
    uint32_t per_block = (c_end - c_first + gridDim.x - 1) / gridDim.x;
    per_block = (per_block + kBlock - 1) / kBlock * kBlock;
    const uint32_t blk_lo = c_first + blockIdx.x * per_block;
    if (blk_lo >= c_end) return;                                               // workgroup-uniform
    const uint32_t blk_hi = blk_lo + per_block < c_end ? blk_lo + per_block : c_end;
    const uint32_t niter = (blk_hi - blk_lo + kBlock - 1) / kBlock;
    const uint32_t cpb = p.buf_samples / 8;                                    // chunks per buffer (a multiple of kBlock)
    // the buffer the range's accumulators belong to, and the chunk that carries the next boundary (its elements 0..5 are still the
    // old buffer's).  A range that begins with a boundary chunk starts "in the buffer before" with nothing accumulated.
    int32_t cur_buf = (int32_t) ((blk_lo - c_first + cpb - 1) / cpb) - 1;
    uint32_t cb_next = c_first + (uint32_t) (cur_buf + 1) * cpb;
    __syncthreads();

    CvAcc acc = {0, 0, 0, 0, 0};
    uint32_t since_flush = 0;                                                  // fast iterations since the accumulators were last folded
    const uint8_t *src = p.iq + 16 * (int64_t) (blk_lo + tid) - 2 * kTrailing;   // the chunk's sixteen IQ bytes (4-byte aligned)
    uint16_t *dst = p.mag + 8 * (uint64_t) (blk_lo + tid);
    // whole = every one of the iteration's kBlock chunks has all eight samples (uniform): their sixteen bytes may be loaded as one.
    // Such an iteration takes the fast path unless its first chunk straddles two buffers (its prefetched samples are then ignored).
    auto whole = [&](uint32_t it) __attribute__((always_inline)) {
        const uint32_t c0 = blk_lo + it * kBlock;
        return it < niter && c0 > c_first && c0 + kBlock <= c_whole_end;
    };
    u32x4_a4 pre[kCvDepth];
#pragma unroll
    for (int k = 0; k < kCvDepth; ++k) {
        pre[k] = u32x4_a4{0, 0, 0, 0};
        if (whole((uint32_t) k)) pre[k] = *(const u32x4_a4 *) (src + (size_t) k * 16 * kBlock);
    }
    for (uint32_t it0 = 0; it0 < niter; it0 += kCvDepth) {
#pragma unroll
        for (int k = 0; k < kCvDepth; ++k) {                                   // (unrolled: the registers of the loads in flight keep their names)
            const uint32_t it = it0 + (uint32_t) k;
            if (it >= niter) break;                                            // uniform
            const uint32_t c0 = blk_lo + it * kBlock;
            const bool is_fast = whole(it) && c0 != cb_next;
            const u32x4_a4 v = pre[k];
            pre[k] = u32x4_a4{0, 0, 0, 0};
            if (whole(it + kCvDepth)) pre[k] = *(const u32x4_a4 *) (src + (size_t) kCvDepth * 16 * kBlock);
            if (is_fast && ++since_flush == kCvFlushEvery) {                   // (a lane's 32-bit accumulators hold 2^14 steps of four samples)
                cv_flush(acc, s_acc, p.sum_level, p.sum_power, cur_buf);
                acc = CvAcc{0, 0, 0, 0, 0};
                since_flush = 0;
            }
            if (is_fast) {
                const uint32_t m0 = cv_lookup2(s_lut, v.x), m1 = cv_lookup2(s_lut, v.y), m2 = cv_lookup2(s_lut, v.z), m3 = cv_lookup2(s_lut, v.w);
                *(u32x4 *) dst = u32x4{m0, m1, m2, m3};
                cv_acc4(acc, m0, m1);
                cv_acc4(acc, m2, m3);
            } else {
                const bool boundary = c0 == cb_next;
                cv_flush(acc, s_acc, p.sum_level, p.sum_power, cur_buf);
                acc = CvAcc{0, 0, 0, 0, 0};
                since_flush = 0;
                cv_slow_iter(p.iq, p.mag, p.n, s_lut, s_acc, p.sum_level, p.sum_power, c0, cur_buf, boundary);
                if (boundary) { ++cur_buf; cb_next += cpb; }
            }
            src += 16 * kBlock;
            dst += 8 * kBlock;
        }
    }
    cv_flush(acc, s_acc, p.sum_level, p.sum_power, cur_buf);
}

// Correctly rounded square root of x in {0} u [2^-30, 1] (what the SC16 converters feed it): the hardware's v_sqrt_f32 is good to
// about one unit in the last place; the two neighbours are tried with exact residuals (fma) — the same two steps the compiler's
// own sqrtf ends with, without its rescaling of tiny and special inputs, which cannot occur here.  Checked against sqrtf over
// all 4096^2 SC16Q11 pairs and a sweep of SC16 ones (tests/test_gpu_convert.py).
__device__ __forceinline__ float sqrt_cr_unit(float x) {
    float y = __builtin_amdgcn_sqrtf(x);
    const float dn = __builtin_bit_cast(float, __builtin_bit_cast(int, y) - 1), up = __builtin_bit_cast(float, __builtin_bit_cast(int, y) + 1);
    const float vp = __builtin_fmaf(-dn, y, x);            // x - dn * y <= 0: y is too large
    const float vs = __builtin_fmaf(-up, y, x);            // x - up * y > 0: y is too small
    y = vp <= 0.0f ? dn : y;
    y = vs > 0.0f ? up : y;
    return y;
}

// SC16 / SC16Q11: mag = sqrtf(min(1, fI*fI + fQ*fQ)), fI = I/scale, u16 = (uint16_t)(mag*65535+0.5)
// (convert.c:212-250, 329-367).  Every float operation is rounded on its own (the reference is
// scalar SSE built with -std=c11, i.e. no FMA contraction); sqrtf is the correctly rounded one.
template <int SCALE_SHIFT>
__device__ __forceinline__ float sc16_magsq(uint32_t w) {
#pragma clang fp contract(off)
    constexpr float inv = 1.0f / (float) (1 << SCALE_SHIFT);   // power of two: I * inv == I / scale exactly
    if (SCALE_SHIFT <= 11) {
        // For |I|, |Q| <= 2^11: I^2, Q^2 and their sum are integers below 2^24 — every float the reference forms on the way
        // (fI, fI * fI, fQ * fQ, their sum: convert.c:342-349) is exact, so the sum of squares is ONE integer dot product,
        // the clamp an integer minimum, and the float comes out of one exact conversion and a power-of-two scale.  Larger
        // inputs end in the clamp either way: rounding is monotone and 2^22 is a float, so no float sum above it comes out at or below it.
        const v2i16 iqv = __builtin_bit_cast(v2i16, w);
        int sq = __builtin_amdgcn_sdot2(iqv, iqv, 0, true);    // (saturating: I = Q = -32768 would wrap; anything above 2^22 is clamped to 1.0 anyway)
        sq = sq > (1 << (2 * SCALE_SHIFT)) ? (1 << (2 * SCALE_SHIFT)) : sq;
        return (float) sq * (inv * inv);
    } else {
        const float fI = (float) (int16_t) (w & 0xffff) * inv;
        const float fQ = (float) (int16_t) (w >> 16) * inv;
        const float a = fI * fI;
        const float b = fQ * fQ;
        float magsq = a + b;
        if (magsq > 1.0f) magsq = 1.0f;
        return magsq;
    }
}

// The magnitudes alone; the per-buffer mean level and power of these formats are sequential FLOAT sums in the reference
// (convert.c:225-249, 342-366) and come from k_fsum_sc16 below, not from here.
template <int SCALE_SHIFT>
__global__ __launch_bounds__(kBlock) void k_convert_sc16(ConvertParams p) {
#pragma clang fp contract(off)
    convert_tail_prologue(p);
    const uint64_t c_first = kTrailing / 8;
    const uint64_t c_end = (kTrailing + p.n + 7) / 8;
    const uint64_t nchunks = c_end - c_first;
    uint64_t per_block = (nchunks + gridDim.x - 1) / gridDim.x;
    per_block = (per_block + kBlock - 1) / kBlock * kBlock;
    const uint64_t blk_lo = c_first + (uint64_t) blockIdx.x * per_block;
    const uint64_t blk_hi = blk_lo + per_block < c_end ? blk_lo + per_block : c_end;
    if (blk_lo >= c_end) return;                                  // workgroup-uniform
    // two 16-byte loads per lane of the next chunk in flight while this one is computed (see k_convert_uc8)
    u32x4_a8 pre0 = {0, 0, 0, 0}, pre1 = {0, 0, 0, 0};
    bool pre_ok = false;
    for (uint64_t c = blk_lo + threadIdx.x; c < blk_hi; c += kBlock) {
        const int64_t i0 = (int64_t) c * 8 - kTrailing;
        uint16_t m[8];
        const bool full = i0 >= 0 && (uint64_t) i0 + 8 <= p.n;
        uint32_t w[8];
        u32x4_a8 v0 = pre0, v1 = pre1;
        if (full && !pre_ok) {
            v0 = *(const u32x4_a8 *) (p.iq + 4 * i0);
            v1 = *(const u32x4_a8 *) (p.iq + 4 * i0 + 16);
        }
        {
            const uint64_t cn = c + kBlock;
            const int64_t in = (int64_t) cn * 8 - kTrailing;
            pre_ok = cn < blk_hi && in >= 0 && (uint64_t) in + 8 <= p.n;
            if (pre_ok) {
                pre0 = *(const u32x4_a8 *) (p.iq + 4 * in);
                pre1 = *(const u32x4_a8 *) (p.iq + 4 * in + 16);
            }
        }
        if (full) {
            w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w;
            w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int64_t i = i0 + e;
                w[e] = (i >= 0 && (uint64_t) i < p.n) ? *(const uint32_t *) (p.iq + 4 * i) : 0u;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float mag = sqrt_cr_unit(sc16_magsq<SCALE_SHIFT>(w[e]));
            const float sc = mag * 65535.0f;
            const float rd = sc + 0.5f;
            m[e] = (uint16_t) rd;
        }
        if (full) {
            u32x4 o = {(uint32_t) m[0] | ((uint32_t) m[1] << 16), (uint32_t) m[2] | ((uint32_t) m[3] << 16),
                       (uint32_t) m[4] | ((uint32_t) m[5] << 16), (uint32_t) m[6] | ((uint32_t) m[7] << 16)};
            *(u32x4 *) (p.mag + c * 8) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int64_t i = i0 + e;
                if (i >= 0 && (uint64_t) i < p.n) p.mag[c * 8 + e] = m[e];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_fsum_sc16: the per-buffer mean level / mean power of the SC16 formats, bit for bit.
//
// convert_sc16_nodc / convert_sc16q11_nodc accumulate `sum_level += mag; sum_power += magsq;` in FLOAT over the buffer's
// 131072 samples (convert.c:225-249, 342-366): every one of the additions rounds, so the result depends on their order, and
// demodulate2400AC's noise floor (demod_2400.c:579-580) and the noise statistics (:474-479) are made of it.  Summed any
// other way (round 2: in double, by atomics) the means differ in the fifth digit.
//
// What makes the sequential sum parallel after all: while the running sum s stays inside one binade [2^e, 2^(e+1)) every
// addition rounds to the same grid g = 2^(e-23).  With s = S g (S an integer in [2^23, 2^24)) and x = (d + f) g, 0 <= f < 1,
// RN(s + x) = (S + d + [f > 1/2]) g — unless f is exactly 1/2 (a tie: the result depends on the parity of S + d, i.e. on every
// earlier rounding) or the sum leaves the binade.  d + [f > 1/2] is what the FPU computes in RN(2^e + x): the mantissa field of
// that sum.  So ONE WAVE per buffer and sum walks the buffer in blocks of 512 samples (eight consecutive ones per lane): every
// lane turns its samples into grid steps against the binade of the sum so far and flags ties (the residual
// x - (RN(2^e + x) - 2^e) is half a step); if S + the block's total stays below 2^24 the block is ONE integer addition — exact,
// whatever the order.
//     Ties are not rare: SC16Q11's squared magnitudes are small integers times 2^-22, and while the grid is only a few bits
//     coarser than that, one sample in 2^k is a tie.  But a tie always leaves the sum EVEN (round half to even), so the carry of
//     a tie is the parity of the steps taken since the previous tie: with Z = running parity of the steps inside the block,
//     carry(tie i) = Z_i xor Z_(previous tie) — ballots and a popcount — and only the block's first tie needs the parity of the
//     sum the block starts from.
// A block in which the sum would leave its binade (~17 per buffer, and a buffer's first) is added sample by sample, in order, by
// v_readlane + v_add_f32.  No LDS, no barrier, 64 VGPRs, one wave per workgroup: 512 (with the level sum: 1024) waves on the
// chip's 1024 SIMDs — what still fits beside k_slice's four waves of 112 VGPRs per SIMD and its 153 of 160 KB of LDS per CU
// without sending one of its (persistent) workgroups to wait; the first version of this kernel that was fast on its own — four
// waves per buffer, a relay through LDS — made k_slice half again as slow.  A buffer is a chain of 256 dependent blocks, beside
// the chunk's other kernels on a stream of its own.  Mode S needs the mean power only (noise statistics); the level sum (Mode
// A/C's noise floor, mgpu_convert) costs a square root per sample more and runs only on request.  The state is read from and left
// in fsum[] as a double holding the float (so a buffer may span launches: mgpu_convert).
// ---------------------------------------------------------------------------------------------
template <int SCALE_SHIFT>
__global__ __launch_bounds__(WAVE) void k_fsum_sc16(const uint8_t *iq, uint64_t n, uint32_t buf_samples, double *fsum_level, double *fsum_power,
                                                     int nsum, int fresh) {
#pragma clang fp contract(off)
    __builtin_amdgcn_s_setprio(3);                             // a dependent chain, one wave per SIMD at most: at no priority beside the main stream's kernels it takes
                                                               // 2-4 x as long and its stream backs up (137-150 against 175 Gsamples/s, r04h / r04f)
    constexpr int kPer = 8, kBlk = kPer * WAVE;
    const uint32_t b = blockIdx.x / (uint32_t) nsum;
    const bool level = (blockIdx.x % (uint32_t) nsum) != 0;    // workgroup 2b: power, 2b + 1: level (nsum == 2)
    const uint64_t first = (uint64_t) b * buf_samples;
    if (first >= n) return;
    const uint64_t len = n - first < buf_samples ? n - first : buf_samples;
    const int lane = lane_id();
    const uint64_t lt_mask = (1ull << lane) - 1;
    double *state = (level ? fsum_level : fsum_power) + b;
    const uint8_t *src = iq + 4 * first;
    const uint64_t nblk = (len + kBlk - 1) / kBlk;
    float s = fresh ? 0.0f : (float) *state;                   // fresh: every buffer's sum starts at zero (the pipeline's chunks; the results may then go straight into page-locked host memory)
    constexpr int kAhead = 3;                                  // blocks in flight: a block is ~0.6 us, HBM latency 2-3 us
    u32x4_a4 pre[kAhead][kPer / 4];
    auto fetch = [&](uint64_t blk, u32x4_a4 *out) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < kPer / 4; ++h) {
            const uint64_t i = blk * kBlk + kPer * (uint64_t) lane + 4 * h;
            u32x4_a4 v = {0, 0, 0, 0};                          // (samples behind the buffer's end: I = Q = 0 -> + 0.0f, which changes nothing)
            if (blk < nblk) {
                if (i + 4 <= len) v = *(const u32x4_a4 *) (src + 4 * i);
                else {
                    if (i + 0 < len) v.x = *(const uint32_t *) (src + 4 * (i + 0));
                    if (i + 1 < len) v.y = *(const uint32_t *) (src + 4 * (i + 1));
                    if (i + 2 < len) v.z = *(const uint32_t *) (src + 4 * (i + 2));
                }
            }
            out[h] = v;
        }
    };
#pragma unroll
    for (int k = 0; k < kAhead; ++k) fetch((uint64_t) k, pre[k]);
#pragma nounroll
    for (uint64_t blk = 0; blk < nblk; ++blk) {                 // (one copy of the body: the registers of the loads in flight shift instead)
        uint32_t w[kPer];
#pragma unroll
        for (int h = 0; h < kPer / 4; ++h) { w[4 * h] = pre[0][h].x; w[4 * h + 1] = pre[0][h].y; w[4 * h + 2] = pre[0][h].z; w[4 * h + 3] = pre[0][h].w; }
#pragma unroll
        for (int k = 0; k + 1 < kAhead; ++k)
#pragma unroll
            for (int h = 0; h < kPer / 4; ++h) pre[k][h] = pre[k + 1][h];
        fetch(blk + kAhead, pre[kAhead - 1]);
        float x[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const float magsq = sc16_magsq<SCALE_SHIFT>(w[j]);
            x[j] = level ? sqrt_cr_unit(magsq) : magsq;
        }
        // the block against the binade the sum is in
        const uint32_t sbits = rfl(__float_as_uint(s));
        const uint32_t eb = sbits & 0x7f800000u;                               // 2^e as bits (0: nothing to align to yet)
        const float M = __uint_as_float(eb), halfg = __uint_as_float(eb - (24u << 23));
        uint32_t inc = 0, par = 0, zbits = 0, ties = 0;                          // zbits / ties: bit j = sample j of this lane
        bool big = false;                                                         // a sample of 2^22 grid steps and more: see below
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const float t = M + x[j];                                             // rounds x to the binade's grid (a tie: to the even side of 2^e + x)
            uint32_t d = __float_as_uint(t) - eb;                                 // ... in grid steps (2^23 and more: x alone leaves the binade)
            const float r = x[j] - (t - M);                                       // exact
            const bool tie = __builtin_fabsf(r) == halfg;
            d -= (tie && r < 0.0f) ? 1u : 0u;                                     // a tie's steps without its carry
            // a sample a quarter of the binade and more (a strong pulse while the sum is still small): its steps are not a small
            // integer any more (RN(2^e + x) may sit in a higher binade, where the mantissa field counts a coarser grid), and one to
            // three of them would pass the "stays below 2^24" test on a clamped count.  Such a block is added in order.
            big |= d >= (1u << 22);
            d = d < (1u << 22) ? d : (1u << 22);                                  // (keeps the wave's total inside 32 bits)
            inc += d;
            par ^= d & 1u;
            zbits |= par << j;                                                    // parity of the lane's steps through sample j
            ties |= (tie ? 1u : 0u) << j;
        }
        // Z = parity of the steps from the block's start through each sample: the lanes before this one by ballot + popcount
        const uint64_t bp = __ballot(par != 0);
        zbits ^= (__popcll(bp & lt_mask) & 1) ? (1u << kPer) - 1u : 0u;
        // every tie's carry = Z there xor Z at the tie before it; the block's first: Z there xor the parity of the sum so far
        const uint64_t tm = __ballot(ties != 0);
        if (tm) {
            const uint32_t z_last = ties ? (zbits >> (31 - __builtin_clz(ties))) & 1u : 0u;
            const uint64_t zl = __ballot(z_last != 0);
            if (ties) {
                const uint64_t before = tm & lt_mask;
                uint32_t zp = before ? (uint32_t) (zl >> (63 - __builtin_clzll(before))) & 1u : (sbits & 1u);
#pragma unroll
                for (int j = 0; j < kPer; ++j)
                    if ((ties >> j) & 1u) { const uint32_t z = (zbits >> j) & 1u; inc += z ^ zp; zp = z; }
            }
        }
        int total;
        (void) wave_incl_scan_dpp((int) inc, total);                              // (<= 512 * (2^22 + 1): fits; 2^24 and more: the block leaves the binade)
        const uint64_t S2 = (uint64_t) ((sbits & 0x7fffffu) | 0x800000u) + (uint32_t) total;
        if (eb != 0 && S2 < (1ull << 24) && !__ballot(big)) {
            s = __uint_as_float(eb | ((uint32_t) S2 & 0x7fffffu));
        } else {                                                                  // in order, one rounding per addition
#pragma nounroll
            for (int l0 = 0; l0 < WAVE; ++l0) {
#pragma unroll
                for (int j = 0; j < kPer; ++j) s = s + __uint_as_float((uint32_t) __builtin_amdgcn_readlane((int) __float_as_uint(x[j]), l0));
            }
        }
    }
    if (lane == 0) *state = (double) s;
}

#if MGPU_EXPERIMENTS   // (measured and not shipped: see the comment; tests/test_gpu_kernel_generations.py keeps it exact)
// ---------------------------------------------------------------------------------------------
// The same sums for the pipeline's chunks, WIDE (round 4).  k_fsum_sc16 above is a chain of 256 dependent block steps per buffer:
// ~0.35 ms per chunk with the VALU to itself at s_setprio 3, a multiple beside the main stream's kernels — on some boxes it bounded
// the SC16 configurations (105-175 Gsamples/s from run to run).  What a block needs from the chain is one thing only: the binade
// the sum is in when the block starts.  PREDICT it, and the blocks are independent:
//   k_fsum_approx  one wave per block of 512 samples: the block's sum from the u16 magnitudes the converter has just written
//                  ((m / 65535)^2: good to ~1e-4 — a prediction only has to be roughly right);
//   k_fsum_prep    one wave per block: the buffer's approximate prefix up to the block (<= 255 values, lane-parallel) -> the
//                  predicted binade; the block's grid steps against it, ties resolved by step parity (fsum_block_steps, the code
//                  k_fsum_sc16 runs per block) -> {total steps as if the incoming sum were even, has a tie, Z at the first tie,
//                  no sample of 2^22 steps or more, the binade};
//   k_fsum_apply   one wave per buffer and sum: 256 summaries = 256 integer additions on the sum's mantissa while the premise
//                  holds (the sum IS in the predicted binade, the block stays in it, no oversized sample); a block whose premise
//                  fails (the ~17 binade crossings of a buffer, its first block, a misprediction next to a crossing) is loaded and
//                  added exactly as k_fsum_sc16 adds it.  ~20 exact blocks + 256 scalar steps.
// MEASURED (profiles/r04_fsum_wide.txt): alone 61 + 147 + 115 us per 1024-buffer chunk, beside the main stream's kernels 179 + 305 +
// 180 us, and the second pass over the samples (536 MB per chunk) costs the main stream more than the chain's one wave per SIMD did:
// SC16Q11 --aggressive 111-165 Gsamples/s against 106-182 with the chain.  Not shipped; kept exact in the experiments build
// (MGPU_FSUM_WIDE=1) because the next step — the summaries computed by the CONVERTER, which has every sample's square in registers
// anyway, against binades predicted from a subsampled pre-pass — starts from it.
// Same arithmetic, same result bit for bit (tests/test_gpu_convert.py, test_gpu_formats.py, test_gpu_modeac.py compare the means
// with the reference's); tests/test_float_sum_model.py pins the block arithmetic without a GPU.
// ---------------------------------------------------------------------------------------------
constexpr int kFsPer = 8, kFsBlk = kFsPer * WAVE;              // samples per lane / per block (512)
constexpr uint32_t kFsValid = 1u, kFsTie = 2u, kFsZ = 4u;      // summary flags (low bits of the binade word)

struct FsumSummary { uint32_t total, meta; };                  // meta = 2^e as float bits (bits 23-30) | flags

// The block against the binade `eb` (2^e as float bits, != 0): grid steps of every sample, ties' carries by step parity, the
// first tie's as if the incoming sum were even.  Returns the wave's total; has_tie / z_first / big are wave-uniform.
__device__ __forceinline__ uint32_t fsum_block_steps(const float (&x)[kFsPer], uint32_t eb, uint64_t lt_mask, int lane, bool &has_tie, uint32_t &z_first, bool &big_any) {
#pragma clang fp contract(off)
    const float M = __uint_as_float(eb), halfg = __uint_as_float(eb - (24u << 23));
    uint32_t inc = 0, par = 0, zbits = 0, ties = 0;
    bool big = false;
#pragma unroll
    for (int j = 0; j < kFsPer; ++j) {
        const float t = M + x[j];                                             // rounds x to the binade's grid (a tie: to the even side of 2^e + x)
        uint32_t d = __float_as_uint(t) - eb;                                 // ... in grid steps
        const float r = x[j] - (t - M);                                       // exact
        const bool tie = __builtin_fabsf(r) == halfg;
        d -= (tie && r < 0.0f) ? 1u : 0u;                                     // a tie's steps without its carry
        big |= d >= (1u << 22);                                               // (see k_fsum_sc16: such a block is added in order)
        d = d < (1u << 22) ? d : (1u << 22);
        inc += d;
        par ^= d & 1u;
        zbits |= par << j;
        ties |= (tie ? 1u : 0u) << j;
    }
    const uint64_t bp = __ballot(par != 0);
    zbits ^= (__popcll(bp & lt_mask) & 1) ? (1u << kFsPer) - 1u : 0u;
    const uint64_t tm = __ballot(ties != 0);
    has_tie = tm != 0;
    z_first = 0;
    if (tm) {
        const uint32_t z_last = ties ? (zbits >> (31 - __builtin_clz(ties))) & 1u : 0u;
        const uint64_t zl = __ballot(z_last != 0);
        // Z at the block's first tie (the lowest lane with a tie, its lowest tie)
        const int first_lane = __ffsll((unsigned long long) tm) - 1;
        const uint32_t zf = ties ? (zbits >> (__builtin_ctz(ties))) & 1u : 0u;
        z_first = (uint32_t) __builtin_amdgcn_readlane((int) zf, first_lane);
        if (ties) {
            const uint64_t before = tm & lt_mask;
            uint32_t zp = before ? (uint32_t) (zl >> (63 - __builtin_clzll(before))) & 1u : 0u;   // (the block's first tie: an even incoming sum)
#pragma unroll
            for (int j = 0; j < kFsPer; ++j)
                if ((ties >> j) & 1u) { const uint32_t z = (zbits >> j) & 1u; inc += z ^ zp; zp = z; }
        }
    }
    big_any = __ballot(big) != 0;
    int total;
    (void) wave_incl_scan_dpp((int) inc, total);
    return (uint32_t) total;
}

template <int SCALE_SHIFT>
__device__ __forceinline__ void fsum_load_block(const uint8_t *src, uint64_t len, uint64_t blk, int lane, bool level, float (&x)[kFsPer]) {
#pragma clang fp contract(off)
    uint32_t w[kFsPer];
#pragma unroll
    for (int h = 0; h < kFsPer / 4; ++h) {
        const uint64_t i = blk * kFsBlk + kFsPer * (uint64_t) lane + 4 * h;
        u32x4_a4 v = {0, 0, 0, 0};                              // (samples behind the buffer's end: + 0.0f, which changes nothing)
        if (i + 4 <= len) v = *(const u32x4_a4 *) (src + 4 * i);
        else {
            if (i + 0 < len) v.x = *(const uint32_t *) (src + 4 * (i + 0));
            if (i + 1 < len) v.y = *(const uint32_t *) (src + 4 * (i + 1));
            if (i + 2 < len) v.z = *(const uint32_t *) (src + 4 * (i + 2));
        }
        w[4 * h] = v.x; w[4 * h + 1] = v.y; w[4 * h + 2] = v.z; w[4 * h + 3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < kFsPer; ++j) {
        const float magsq = sc16_magsq<SCALE_SHIFT>(w[j]);
        x[j] = level ? sqrt_cr_unit(magsq) : magsq;
    }
}

// approximate block sums from the magnitudes (d_mag[kTrailing + i] = magnitude of sample i): approx[sum][global block]
__global__ __launch_bounds__(kBlock) void k_fsum_approx(const uint16_t *mag, uint64_t n, uint32_t buf_samples, float *approx, uint32_t nblk_total, uint32_t bpb, int nsum) {
    const int lane = lane_id();
    const uint32_t q = blockIdx.x * (kBlock / WAVE) + ((uint32_t) threadIdx.x >> 6);
    if (q >= nblk_total) return;
    const uint32_t b = q / bpb, j = q % bpb;
    const uint64_t first = (uint64_t) b * buf_samples;
    const uint64_t len = first < n ? (n - first < buf_samples ? n - first : buf_samples) : 0;
    const uint64_t i0 = (uint64_t) j * kFsBlk + kFsPer * (uint64_t) lane;
    float sp = 0.0f, sl = 0.0f;
    if (i0 < len) {
        const uint16_t *src = mag + kTrailing + first + i0;
        u32x4_a4 v = {0, 0, 0, 0};
        if (i0 + kFsPer <= len) v = *(const u32x4_a4 *) src;
        else { uint16_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0}; for (uint64_t e = 0; e < len - i0; ++e) t[e] = src[e]; v = u32x4_a4{(uint32_t) t[0] | ((uint32_t) t[1] << 16), (uint32_t) t[2] | ((uint32_t) t[3] << 16), (uint32_t) t[4] | ((uint32_t) t[5] << 16), (uint32_t) t[6] | ((uint32_t) t[7] << 16)}; }
        const uint32_t ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = (float) (ww[e] & 0xffffu) * (1.0f / 65535.0f), c = (float) (ww[e] >> 16) * (1.0f / 65535.0f);
            sl += a + c;
            sp += a * a + c * c;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { sp += __shfl_xor(sp, off); sl += __shfl_xor(sl, off); }
    if (lane == 0) { approx[q] = sp; if (nsum == 2) approx[nblk_total + q] = sl; }
}

template <int SCALE_SHIFT>
__global__ __launch_bounds__(kBlock) void k_fsum_prep(const uint8_t *iq, uint64_t n, uint32_t buf_samples, const float *approx, FsumSummary *sums,
                                                      uint32_t nblk_total, uint32_t bpb) {
#pragma clang fp contract(off)
    const int lane = lane_id();
    const uint64_t lt_mask = (1ull << lane) - 1;
    const uint32_t q = blockIdx.x * (kBlock / WAVE) + ((uint32_t) threadIdx.x >> 6);
    const bool level = blockIdx.y != 0;
    if (q >= nblk_total) return;
    const uint32_t b = q / bpb, j = q % bpb;
    const uint64_t first = (uint64_t) b * buf_samples;
    const uint64_t len = first < n ? (n - first < buf_samples ? n - first : buf_samples) : 0;
    FsumSummary out = {0u, 0u};
    if ((uint64_t) j * kFsBlk < len) {
        float x[kFsPer];
        fsum_load_block<SCALE_SHIFT>(iq + 4 * first, len, j, lane, level, x);
        // where the sum roughly is when this block starts: the approximate sums of the buffer's blocks before it
        const float *ap = approx + (level ? nblk_total : 0u) + (size_t) b * bpb;
        float pre = 0.0f;
        for (uint32_t i = (uint32_t) lane; i < j; i += WAVE) pre += ap[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) pre += __shfl_xor(pre, off);
        const uint32_t eb = rfl(__float_as_uint(pre)) & 0x7f800000u;
        if (eb != 0 && eb < 0x7f800000u && eb > (24u << 23)) {
            bool has_tie, big;
            uint32_t z_first;
            const uint32_t total = fsum_block_steps(x, eb, lt_mask, lane, has_tie, z_first, big);
            out.total = total;
            out.meta = eb | (big ? 0u : kFsValid) | (has_tie ? kFsTie : 0u) | (z_first ? kFsZ : 0u);
        }
    }
    if (lane == 0) sums[(level ? nblk_total : 0u) + q] = out;
}

template <int SCALE_SHIFT>
__global__ __launch_bounds__(WAVE) void k_fsum_apply(const uint8_t *iq, uint64_t n, uint32_t buf_samples, const FsumSummary *sums, uint32_t nblk_total, uint32_t bpb,
                                                     double *fsum_level, double *fsum_power, int nsum) {
#pragma clang fp contract(off)
    if (nsum == 2) __builtin_amdgcn_s_setprio(3);               // (Mode A/C waits for these on the main stream)
    const uint32_t b = blockIdx.x / (uint32_t) nsum;
    const bool level = (blockIdx.x % (uint32_t) nsum) != 0;
    const uint64_t first = (uint64_t) b * buf_samples;
    if (first >= n) return;
    const uint64_t len = n - first < buf_samples ? n - first : buf_samples;
    const int lane = lane_id();
    const uint64_t lt_mask = (1ull << lane) - 1;
    double *state = (level ? fsum_level : fsum_power) + b;
    const uint8_t *src = iq + 4 * first;
    const uint32_t nblk = (uint32_t) ((len + kFsBlk - 1) / kFsBlk);
    const FsumSummary *sb = sums + (level ? nblk_total : 0u) + (size_t) b * bpb;
    float s = (float) *state;
    for (uint32_t j0 = 0; j0 < nblk; j0 += WAVE) {
        FsumSummary mine = {0u, 0u};
        if (j0 + (uint32_t) lane < nblk) mine = sb[j0 + lane];
        const uint32_t cnt = nblk - j0 < (uint32_t) WAVE ? nblk - j0 : (uint32_t) WAVE;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t total = (uint32_t) __builtin_amdgcn_readlane((int) mine.total, (int) k);
            const uint32_t meta = (uint32_t) __builtin_amdgcn_readlane((int) mine.meta, (int) k);
            const uint32_t sbits = rfl(__float_as_uint(s));
            const uint32_t eb = sbits & 0x7f800000u;
            if ((meta & kFsValid) && eb != 0 && (meta & 0x7f800000u) == eb) {
                const uint32_t S = (sbits & 0x7fffffu) | 0x800000u;
                // an odd incoming sum turns the first tie's carry round (the summary took it for even)
                const uint32_t S2 = S + total + (((meta & kFsTie) && (S & 1u)) ? ((meta & kFsZ) ? 0xffffffffu : 1u) : 0u);
                if (S2 < (1u << 24)) { s = __uint_as_float(eb | (S2 & 0x7fffffu)); continue; }
            }
            // the premise fails: this block exactly, against the binade the sum is really in (k_fsum_sc16's step)
            float x[kFsPer];
            fsum_load_block<SCALE_SHIFT>(src, len, j0 + k, lane, level, x);
            bool done = false;
            if (eb != 0) {
                bool has_tie, big;
                uint32_t z_first;
                uint32_t tot = fsum_block_steps(x, eb, lt_mask, lane, has_tie, z_first, big);
                const uint32_t S = (sbits & 0x7fffffu) | 0x800000u;
                if (has_tie && (S & 1u)) tot += z_first ? 0xffffffffu : 1u;
                const uint64_t S2 = (uint64_t) S + tot;
                if (!big && S2 < (1ull << 24)) { s = __uint_as_float(eb | ((uint32_t) S2 & 0x7fffffu)); done = true; }
            }
            if (!done) {                                                          // in order, one rounding per addition
#pragma nounroll
                for (int l0 = 0; l0 < WAVE; ++l0) {
#pragma unroll
                    for (int jj = 0; jj < kFsPer; ++jj) s = s + __uint_as_float((uint32_t) __builtin_amdgcn_readlane((int) __float_as_uint(x[jj]), l0));
                }
            }
        }
    }
    if (lane == 0) *state = (double) s;
}

#endif  // MGPU_EXPERIMENTS

void launch_fsum_sc16(int format, const uint8_t *iq, uint64_t n, uint32_t buf_samples, double *fsum_level, double *fsum_power, int want_level,
                      hipStream_t s, int fresh) {
    if (n == 0 || format == 0) return;
    const uint32_t nbuf = (uint32_t) ((n + buf_samples - 1) / buf_samples);
    const int nsum = want_level ? 2 : 1;
    if (format == 1) hipLaunchKernelGGL(k_fsum_sc16<15>, dim3(nbuf * nsum), dim3(WAVE), 0, s, iq, n, buf_samples, fsum_level, fsum_power, nsum, fresh);
    else hipLaunchKernelGGL(k_fsum_sc16<11>, dim3(nbuf * nsum), dim3(WAVE), 0, s, iq, n, buf_samples, fsum_level, fsum_power, nsum, fresh);
}

#if MGPU_EXPERIMENTS
// scratch of the wide form: approx[nsum][blocks] floats + summaries[nsum][blocks]
size_t fsum_wide_scratch_bytes(uint64_t max_samples, uint32_t buf_samples) {
    const uint64_t bpb = (buf_samples + kFsBlk - 1) / kFsBlk, nbuf = (max_samples + buf_samples - 1) / buf_samples + 1;
    return (size_t) (nbuf * bpb) * 2 * (sizeof(float) + sizeof(FsumSummary)) + 256;
}

void launch_fsum_sc16_wide(int format, const uint8_t *iq, const uint16_t *mag, uint64_t n, uint32_t buf_samples, double *fsum_level, double *fsum_power,
                           int want_level, void *scratch, hipStream_t s) {
    if (n == 0 || format == 0) return;
    const uint32_t nbuf = (uint32_t) ((n + buf_samples - 1) / buf_samples);
    const uint32_t bpb = (buf_samples + kFsBlk - 1) / kFsBlk, nblk_total = nbuf * bpb;
    const int nsum = want_level ? 2 : 1;
    float *approx = (float *) scratch;
    FsumSummary *sums = (FsumSummary *) ((uint8_t *) scratch + (((size_t) nblk_total * 2 * sizeof(float) + 255) & ~(size_t) 255));
    const unsigned wgs = (nblk_total + kBlock / WAVE - 1) / (kBlock / WAVE);
    hipLaunchKernelGGL(k_fsum_approx, dim3(wgs), dim3(kBlock), 0, s, mag, n, buf_samples, approx, nblk_total, bpb, nsum);
    if (format == 1) {
        hipLaunchKernelGGL(k_fsum_prep<15>, dim3(wgs, nsum), dim3(kBlock), 0, s, iq, n, buf_samples, approx, sums, nblk_total, bpb);
        hipLaunchKernelGGL(k_fsum_apply<15>, dim3(nbuf * nsum), dim3(WAVE), 0, s, iq, n, buf_samples, sums, nblk_total, bpb, fsum_level, fsum_power, nsum);
    } else {
        hipLaunchKernelGGL(k_fsum_prep<11>, dim3(wgs, nsum), dim3(kBlock), 0, s, iq, n, buf_samples, approx, sums, nblk_total, bpb);
        hipLaunchKernelGGL(k_fsum_apply<11>, dim3(nbuf * nsum), dim3(WAVE), 0, s, iq, n, buf_samples, sums, nblk_total, bpb, fsum_level, fsum_power, nsum);
    }
}
#endif  // MGPU_EXPERIMENTS

// the grid's upper bound: 1024 = four workgroups of 33 KB LDS per CU
void launch_convert(int format, const ConvertParams &p, hipStream_t s) {
    if (p.n == 0) return;
    const uint64_t nchunks = (kTrailing + p.n + 7) / 8 - kTrailing / 8;
    uint64_t blocks = (nchunks + kBlock * 8 - 1) / (kBlock * 8);   // >= 8 chunks per thread
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    const bool lean_ok = p.buf_samples % 2048u == 0 && p.buf_samples >= 2048u && p.n < (1ull << 34);
    if (format == 0 && lean_ok) hipLaunchKernelGGL(k_convert_uc8_lean, dim3((unsigned) blocks), dim3(kBlock), 0, s, p);
    else if (format == 0) hipLaunchKernelGGL(k_convert_uc8, dim3((unsigned) blocks), dim3(kBlock), 0, s, p);
    else if (format == 1) hipLaunchKernelGGL(k_convert_sc16<15>, dim3((unsigned) blocks * 2), dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL(k_convert_sc16<11>, dim3((unsigned) blocks * 2), dim3(kBlock), 0, s, p);
}

// A kernel of KNOWN duration (it spins on the 100 MHz s_memrealtime counter): mgpu_event_bracket_us measures what a pair of timing
// HIP events around one kernel in a busy stream reports beyond the kernel itself (tools/micro/event_overhead.hip).
__global__ void k_spin(unsigned ticks, unsigned long long *sink) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) { }
    if (sink && threadIdx.x == 0 && blockIdx.x == 0) *sink = t0;
}
void launch_spin(unsigned us, unsigned blocks, unsigned long long *sink, hipStream_t s) {
    hipLaunchKernelGGL(k_spin, dim3(blocks), dim3(kBlock), 0, s, us * 100u, sink);
}
