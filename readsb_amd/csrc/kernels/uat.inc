// kernels/uat.inc — UAT input: a stream of dump978 downlink lines in HBM to the DF18 extended squitters readsb's --net-uat-in-port
// path makes of them (decodeUatMessage, net_io.c:4334-4372 -> uat2esnt/uat2esnt.c, uat_decode.c).  Part of the single translation
// unit kernels.hip (included inside namespace mgpu, after text.inc, whose ByteSink and k_text_sum it uses, and beast.inc's
// k_beast_scan).  The formatter is uat_format.h's, the one the host compiles too.
//
// Workgroup = tile of kUatTile bytes of text, three passes, no workgroup waits for another:
//   k_uat_index   newline masks from 16-byte loads: per tile the number of '\n' and the place of the last one
//   k_beast_scan  -> the index of every tile's first line, the number of lines; k_uat_last -> the bytes consumed
//   k_uat_size    the tile and kUatHalo bytes behind it through LDS (coalesced 16-byte loads at any alignment of the text; a newline
//                 mask per vector beside them).  A line belongs to the tile that holds its first byte; a lane takes the lines that
//                 start in its 32 bytes of the tile, finds each one's end in the masks and runs the formatter into the counting
//                 emitter: frames and deferred lines per lane (a halfword each), frames | deferred | short lines per tile.  Line starts
//                 are never written to memory: both passes find them in LDS.
//   k_beast_scan  twice, k_text_sum
//   k_uat_write   the same staging; THE SAME formatter into an emitter that writes the AVR lines to LDS at the alignment (mod 16) the
//                 tile's first output byte has in memory — a frame is 45 bytes, its place is known from the counts — and the records
//                 straight to memory; the tile's text leaves as whole aligned 16-byte vectors, byte stores at its two ends only.
// Text gives at most 4 frames per 37 bytes (uat_format.h: uat_max_frames), so the lines that start in a tile give at most kUatTileFrames
// frames; several frame-giving lines can start in a lane's 32 bytes (an 11-byte line of MDB types 11-31 gives one frame): a lane
// loops over its lines and its emitter moves on.
constexpr uint32_t kUatLds = kUatTile + kUatHalo + 32;           // staged bytes: 16 before the tile's aligned start, the tile, the halo, the misalignment
constexpr uint32_t kUatVecs = kUatLds / 16;
constexpr uint32_t kUatChunk = kUatTile / kBlock;                // bytes of the tile whose line starts a lane takes
constexpr uint32_t kUatTileFrames = (uint32_t) uat_max_frames(kUatTile);
static_assert(kUatChunk == 32 && uat_max_frames(kUatChunk) < 256, "a lane's starts are the bits of one word; its frames fit its meta's byte");
static_assert(kUatHalo == kUatDevLineMax && kUatLds % 16 == 0, "the halo holds the longest line the device takes");
static_assert(kUatLds + 2 * kUatVecs + kUatTileFrames * kUatFrameText + 16 + 256 <= 65536, "k_uat_write's static LDS");
static_assert((uint64_t) kUatTileFrames * kUatFrameText < (1u << 16), "a tile's bytes fit the scans' int");

// bit j: byte j of the vector is '\n'
__device__ __forceinline__ uint32_t uat_nl16(u32x4 v) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t x = v[j] ^ 0x0a0a0a0au;
        const uint32_t y = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);       // 0x80 in every byte that was '\n', exactly
        m |= (((y >> 7) & 1u) | ((y >> 14) & 2u) | ((y >> 21) & 4u) | ((y >> 28) & 8u)) << (4 * j);
    }
    return m;
}
// bits j with lo <= j < hi, of 16
__device__ __forceinline__ uint32_t uat_range16(long long lo, long long hi) {
    const uint32_t l = lo < 0 ? 0u : lo > 16 ? 16u : (uint32_t) lo, h = hi < 0 ? 0u : hi > 16 ? 16u : (uint32_t) hi;
    return h > l ? ((1u << h) - 1u) & ~((1u << l) - 1u) : 0u;
}
// the aligned vectors that hold a byte of [text, text + nbytes): nothing else is loaded
__device__ __forceinline__ u32x4 uat_load(uintptr_t a, const uint8_t *text, uint64_t nbytes) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(text) & ~(uintptr_t) 15, hi = (reinterpret_cast<uintptr_t>(text) + nbytes + 15) & ~(uintptr_t) 15;
    u32x4 x = {0u, 0u, 0u, 0u};
    if (a >= lo && a < hi) x = *reinterpret_cast<const u32x4 *>(a);
    return x;
}

__global__ __launch_bounds__(kBlock) void k_uat_index(const uint8_t *text, uint64_t nbytes, uint32_t *block_nl, uint32_t *block_last) {
    __shared__ uint32_t s_sum[kBlock / WAVE], s_max[kBlock / WAVE];
    const uint64_t tile_pos = (uint64_t) blockIdx.x * kUatTile;
    const uintptr_t g = reinterpret_cast<uintptr_t>(text) + tile_pos;
    const uint32_t mis = (uint32_t) (g & 15u);
    const long long tile_end = (long long) (tile_pos + kUatTile < nbytes ? tile_pos + kUatTile : nbytes);
    uint32_t count = 0, last = 0;
    for (uint32_t v = threadIdx.x; v < kUatTile / 16 + 1; v += kBlock) {
        const u32x4 x = uat_load((g & ~(uintptr_t) 15) + 16u * v, text, nbytes);
        const long long p0 = (long long) tile_pos + 16ll * v - mis;                      // the stream position of the vector's byte 0
        const uint32_t m = uat_nl16(x) & uat_range16((long long) tile_pos - p0, tile_end - p0);
        count += (uint32_t) __popc(m);
        if (m) last = 16u * v - mis + (32u - (uint32_t) __clz(m));                     // 1 + the offset in the tile: later vectors are larger
    }
    const uint32_t ws = (uint32_t) wave_sum_u64(count);
    uint32_t wm = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(wm, d); wm = o > wm ? o : wm; }
    if (lane_id() == 0) { s_sum[threadIdx.x >> 6] = ws; s_max[threadIdx.x >> 6] = wm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t mx = 0;
        for (int k = 0; k < kBlock / WAVE; ++k) mx = s_max[k] > mx ? s_max[k] : mx;
        block_nl[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        block_last[blockIdx.x] = mx;
    }
}

// bytes up to and including the stream's last '\n' (one workgroup)
__global__ __launch_bounds__(kScanThreads) void k_uat_last(const uint32_t *block_last, uint32_t nblocks, unsigned long long *consumed) {
    __shared__ unsigned long long s_part[kScanThreads];
    unsigned long long best = 0;
    for (uint32_t k = threadIdx.x; k < nblocks; k += kScanThreads)
        if (block_last[k]) best = (unsigned long long) k * kUatTile + block_last[k];     // (k ascends: the last one found is the largest)
    s_part[threadIdx.x] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int k = 0; k < kScanThreads; ++k) all = s_part[k] > all ? s_part[k] : all;
        *consumed = all;
    }
}

// The tile of this workgroup in LDS: s_in[i] is the byte at stream position tile_pos + i - mis - 16 (zeros where no vector of the text
// lies), s_nl[v] the newline mask of s_in[16 v .. 16 v + 16) over positions inside the stream.  Returns mis.
__device__ __forceinline__ uint32_t uat_stage(const uint8_t *text, uint64_t nbytes, uint8_t *s_in, uint16_t *s_nl) {
    const uint64_t tile_pos = (uint64_t) blockIdx.x * kUatTile;
    const uintptr_t g = reinterpret_cast<uintptr_t>(text) + tile_pos;
    const uint32_t mis = (uint32_t) (g & 15u);
    const uintptr_t a0 = (g & ~(uintptr_t) 15) - 16u;
    for (uint32_t v = threadIdx.x; v < kUatVecs; v += kBlock) {
        const u32x4 x = uat_load(a0 + 16u * v, text, nbytes);
        *reinterpret_cast<u32x4 *>(s_in + 16u * v) = x;
        const long long p0 = (long long) tile_pos + 16ll * v - mis - 16;
        s_nl[v] = (uint16_t) (uat_nl16(x) & uat_range16(-p0, (long long) nbytes - p0));
    }
    __syncthreads();
    return mis;
}

// the bytes from s_in[at] to the next '\n' of the stream: 0 .. kUatDevLineMax, or kUatDevLineMax + 1 when there is none that near
__device__ __forceinline__ uint32_t uat_line_len(const uint16_t *s_nl, uint32_t at) {
    uint32_t v = at >> 4;
    const uint32_t m = (uint32_t) s_nl[v] >> (at & 15u);
    if (m) return (uint32_t) __ffs(m) - 1u;
    for (uint32_t got = 16u - (at & 15u); got <= kUatDevLineMax; got += 16u) {
        const uint32_t mv = s_nl[++v];
        if (mv) { const uint32_t r = got + (uint32_t) __ffs(mv) - 1u; return r <= kUatDevLineMax ? r : kUatDevLineMax + 1u; }
    }
    return kUatDevLineMax + 1u;
}

// What a lane takes: bit b of `starts`: a line starts at byte b of its chunk; bit b of `own`: that byte is a '\n'.
__device__ __forceinline__ void uat_lane_lines(const uint16_t *s_nl, uint32_t mis, uint32_t &starts, uint32_t &own) {
    const uint32_t i0 = kUatChunk * threadIdx.x + mis + 15u;                            // s_in's index of the byte before the chunk
    const uint32_t v0 = i0 >> 4, sh = i0 & 15u;
    const uint64_t m48 = (uint64_t) s_nl[v0] | (uint64_t) s_nl[v0 + 1] << 16 | (uint64_t) s_nl[v0 + 2] << 32;
    starts = (uint32_t) (m48 >> sh);
    own = (uint32_t) (m48 >> (sh + 1u));
    if (blockIdx.x == 0 && threadIdx.x == 0) starts |= 1u;                              // the stream's first line
}

// exclusive prefix sum over the workgroup; s_wave: kBlock / WAVE words of LDS nobody else uses meanwhile
__device__ __forceinline__ uint32_t uat_block_scan(uint32_t v, uint32_t *s_wave, uint32_t &total) {
    int wtotal;
    const int ex = wave_excl_scan((int) v, wtotal);
    __syncthreads();
    if (lane_id() == 0) s_wave[threadIdx.x >> 6] = (uint32_t) wtotal;
    __syncthreads();
    uint32_t before = (uint32_t) ex;
    for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k) before += s_wave[k];
    total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    return before;
}

// meta of a lane: frames of its lines | deferred lines << 8
__global__ __launch_bounds__(kBlock) void k_uat_size(UatParams a, const unsigned long long *off_nl, const unsigned long long *total, uint16_t *meta, uint32_t *block_frames,
                                                     uint32_t *block_def, uint32_t *block_short) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ uint16_t s_nl[kUatVecs];
    __shared__ uint32_t s_wave[kBlock / WAVE];
    const uint32_t mis = uat_stage(a.text, a.nbytes, s_in, s_nl);
    uint32_t starts, own, tile_nl;
    uat_lane_lines(s_nl, mis, starts, own);
    const uint32_t nl_before = uat_block_scan((uint32_t) __popc(own), s_wave, tile_nl);
    const unsigned long long nlines = total[0], first = off_nl[blockIdx.x] + nl_before;
    uint32_t frames = 0, def = 0, shrt = 0;
    for (uint32_t rest = starts; rest; rest &= rest - 1u) {
        const uint32_t b = (uint32_t) __ffs(rest) - 1u;
        const uint32_t at = kUatChunk * threadIdx.x + b + mis + 16u;
        const uint32_t n = uat_line_len(s_nl, at);
        const unsigned long long index = first + (uint32_t) __popc(own & ((1u << b) - 1u));
        if (n > kUatDevLineMax && index >= nlines) continue;                            // bytes behind the last '\n': not a line
        UatCountEmit e = {0};
        const int cls = uat_line(s_in + at, n, a.sigtab, kUatNoOverride, e);
        frames += e.n;
        def += cls == UAT_DEFER;
        shrt += cls == UAT_SHORT;
    }
    meta[(size_t) blockIdx.x * kBlock + threadIdx.x] = (uint16_t) (frames | def << 8);
    uint32_t tf, td, ts;
    uat_block_scan(frames, s_wave, tf);
    uat_block_scan(def, s_wave, td);
    uat_block_scan(shrt, s_wave, ts);
    if (threadIdx.x == 0) { block_frames[blockIdx.x] = tf; block_def[blockIdx.x] = td; block_short[blockIdx.x] = ts; }
}

// a frame's text to LDS, its record to memory
struct UatWriteEmit {
    uint8_t *p;
    const UatParams &a;
    unsigned long long at, line;
    __device__ __forceinline__ void frame(uint32_t s, const UatFrame &fr) {
        ByteSink sink = {p};
        uat_put_frame(sink, s, fr);
        p = sink.p;
        if (at < a.msgs_cap) {
            if (a.msgs) { mgpu_msg r; uat_fill_msg(r, s, fr, a.now_ms); a.msgs[at] = r; }
            if (a.sig) a.sig[at] = (uint8_t) s;
            if (a.line_of) a.line_of[at] = line;
        }
        ++at;
    }
};

__global__ __launch_bounds__(kBlock) void k_uat_write(UatParams a, const unsigned long long *off_nl, const unsigned long long *total, const uint16_t *meta,
                                                      const unsigned long long *off_frames, const unsigned long long *off_def) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[kUatTileFrames * kUatFrameText + 16];
    __shared__ uint16_t s_nl[kUatVecs];
    __shared__ uint32_t s_wave[kBlock / WAVE];
    const uint32_t mis = uat_stage(a.text, a.nbytes, s_in, s_nl);
    uint32_t starts, own, tile_nl, tile_frames, tile_def;
    uat_lane_lines(s_nl, mis, starts, own);
    const uint32_t nl_before = uat_block_scan((uint32_t) __popc(own), s_wave, tile_nl);
    const uint32_t mt = meta[(size_t) blockIdx.x * kBlock + threadIdx.x];
    const uint32_t frames_before = uat_block_scan(mt & 0xffu, s_wave, tile_frames);
    const uint32_t def_before = uat_block_scan(mt >> 8, s_wave, tile_def);
    const unsigned long long nlines = total[0], first = off_nl[blockIdx.x] + nl_before;
    const unsigned long long base = off_frames[blockIdx.x] * kUatFrameText;             // the tile's first output byte
    const uint32_t mis_out = (uint32_t) ((reinterpret_cast<uintptr_t>(a.out) + base) & 15u);
    if (mt && tile_frames <= kUatTileFrames) {                                          // (the bound is proved above; never trust a proof with an LDS buffer)
        UatWriteEmit e = {s_out + mis_out + frames_before * kUatFrameText, a, off_frames[blockIdx.x] + frames_before, 0};
        unsigned long long slot = off_def[blockIdx.x] + def_before;
        for (uint32_t rest = starts; rest; rest &= rest - 1u) {
            const uint32_t b = (uint32_t) __ffs(rest) - 1u;
            const uint32_t at = kUatChunk * threadIdx.x + b + mis + 16u;
            const uint32_t n = uat_line_len(s_nl, at);
            const unsigned long long index = first + (uint32_t) __popc(own & ((1u << b) - 1u));
            if (n > kUatDevLineMax && index >= nlines) continue;
            e.line = a.line_base + index;
            const int cls = uat_line(s_in + at, n, a.sigtab, kUatNoOverride, e);
            if (cls == UAT_DEFER) {
                if (slot < a.deferred_cap) a.deferred[slot] = a.line_base + index;
                ++slot;
            }
        }
    }
    __syncthreads();
    if (tile_frames > kUatTileFrames) return;
    // s_out[k] <-> dst[k]; dst is 16-byte aligned
    const uint32_t lo = mis_out, hi = mis_out + tile_frames * kUatFrameText;
    if (hi == lo || base >= a.cap) return;
    uint8_t *dst = a.out + base - mis_out;
    if (base + (hi - lo) <= a.cap) {
        const uint32_t vlo = (lo + 15u) & ~15u, vhi = hi & ~15u;
        if (vhi > vlo) {
            for (uint32_t k = vlo / 16 + threadIdx.x; k < vhi / 16; k += kBlock) reinterpret_cast<u32x4 *>(dst)[k] = reinterpret_cast<const u32x4 *>(s_out)[k];
            if (threadIdx.x < 15) {                                                     // at most fifteen bytes before and after the vector run
                const uint32_t h = lo + threadIdx.x, t = vhi + threadIdx.x;
                if (h < vlo) dst[h] = s_out[h];
                if (t < hi) dst[t] = s_out[t];
            }
        } else {
            for (uint32_t k = lo + threadIdx.x; k < hi; k += kBlock) dst[k] = s_out[k];
        }
    } else {                                                                            // the capacity cuts this tile: the bytes below it only
        for (uint32_t k = lo + threadIdx.x; k < hi; k += kBlock)
            if (base + (k - mis_out) < a.cap) dst[k] = s_out[k];
    }
}

void launch_uat_encode(const UatParams &a, const UatScratch &w, hipStream_t s) {
    if (a.nbytes == 0) return;
    const unsigned tiles = (unsigned) ((a.nbytes + kUatTile - 1) / kUatTile);
    uint32_t *b_nl = w.blocks, *b_last = w.blocks + w.stride, *b_frames = w.blocks + 2 * w.stride, *b_def = w.blocks + 3 * w.stride, *b_short = w.blocks + 4 * w.stride;
    unsigned long long *off_nl = w.off, *off_frames = w.off + w.stride, *off_def = w.off + 2 * w.stride;
    hipLaunchKernelGGL(k_uat_index, dim3(tiles), dim3(kBlock), 0, s, a.text, a.nbytes, b_nl, b_last);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, b_nl, tiles, off_nl, w.total);
    hipLaunchKernelGGL(k_uat_last, dim3(1), dim3(kScanThreads), 0, s, b_last, tiles, w.total + 1);
    hipLaunchKernelGGL(k_uat_size, dim3(tiles), dim3(kBlock), 0, s, a, off_nl, w.total, w.meta, b_frames, b_def, b_short);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, b_frames, tiles, off_frames, w.total + 2);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, b_def, tiles, off_def, w.total + 3);
    hipLaunchKernelGGL(k_text_sum, dim3(1), dim3(kScanThreads), 0, s, b_short, tiles, w.total + 4);
    hipLaunchKernelGGL(k_uat_write, dim3(tiles), dim3(kBlock), 0, s, a, off_nl, w.total, w.meta, off_frames, off_def);
}
