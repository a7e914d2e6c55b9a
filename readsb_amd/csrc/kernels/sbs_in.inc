// kernels/sbs_in.inc — SBS input: a stream of BaseStation lines in HBM to the aircraft records readsb's --net-sbs-in-port, MLAT result,
// JAERO and PRIO ports make of them (decodeSbsLine, net_io.c:2952-3178, behind readAscii, :4599-4641).  Part of the single translation
// unit kernels.hip (included inside namespace mgpu, after uat.inc, whose tiles, loads, scans and line search it uses, text.inc's
// k_text_sum and beast.inc's k_beast_scan).  The parser is sbs_in_format.h's, the one the host compiles too.
//
// The passes are uat.inc's, with two differences.  A line ends at '\n' OR at a NUL byte (readAscii turns every NUL into '\n' first),
// so the index pass and the staging here build their own terminator masks; everything that reads the masks is uat.inc's.  And the
// output is fixed-size records:
//   k_sbs_in_index   terminator masks from 16-byte loads: per tile the number of terminators and the place of the last one
//   k_beast_scan     -> the index of every tile's first line, the number of lines; k_uat_last -> the bytes consumed
//   k_sbs_in_size    the tile and its halo through LDS; a lane takes the lines that start in its 32 bytes of the tile and runs the
//                    parser: records and deferred lines per lane (a halfword), records | deferred | invalid lines per tile
//   k_beast_scan     twice, k_text_sum
//   k_sbs_in_write   the same staging, THE SAME parser; a lane stores its records straight to memory.  A record is 96 bytes at a
//                    multiple of 96 from recs — six whole 16-byte vectors wherever recs is 16-byte aligned — and one lane owns all
//                    of it, so a pass through LDS (390 records a tile at the most = 37 KiB beside the 9 KiB staged) would change who
//                    issues the same vectors, not how many there are (DESIGN.md).
// A line that gives a record or is deferred has 20 bytes and a terminator, so at most two of either start in a lane's 32 bytes.
// The halo (kUatHalo = 256) is longer than the kSbsInLook = 201 bytes that decide a line; uat_line_len's "none that near" is > 200.
static_assert(kUatHalo >= kSbsInLook && kUatDevLineMax >= kSbsInMaxLen, "the halo holds every byte that decides a line");
static_assert(kUatChunk / (kSbsInMinLen + 1) + 1 < 256, "a lane's records fit its meta's byte");

// bit j: byte j of the vector equals the byte repeated in `pattern`
__device__ __forceinline__ uint32_t sbs_in_eq16(u32x4 v, uint32_t pattern) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t x = v[j] ^ pattern;
        const uint32_t y = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);       // 0x80 in every byte that was equal, exactly
        m |= (((y >> 7) & 1u) | ((y >> 14) & 2u) | ((y >> 21) & 4u) | ((y >> 28) & 8u)) << (4 * j);
    }
    return m;
}
// bit j: byte j of the vector is '\n' or NUL
__device__ __forceinline__ uint32_t sbs_in_term16(u32x4 v) { return sbs_in_eq16(v, 0x0a0a0a0au) | sbs_in_eq16(v, 0u); }

// k_uat_index with the terminator mask
__global__ __launch_bounds__(kBlock) void k_sbs_in_index(const uint8_t *text, uint64_t nbytes, uint32_t *block_nl, uint32_t *block_last) {
    __shared__ uint32_t s_sum[kBlock / WAVE], s_max[kBlock / WAVE];
    const uint64_t tile_pos = (uint64_t) blockIdx.x * kUatTile;
    const uintptr_t g = reinterpret_cast<uintptr_t>(text) + tile_pos;
    const uint32_t mis = (uint32_t) (g & 15u);
    const long long tile_end = (long long) (tile_pos + kUatTile < nbytes ? tile_pos + kUatTile : nbytes);
    uint32_t count = 0, last = 0;
    for (uint32_t v = threadIdx.x; v < kUatTile / 16 + 1; v += kBlock) {
        const u32x4 x = uat_load((g & ~(uintptr_t) 15) + 16u * v, text, nbytes);
        const long long p0 = (long long) tile_pos + 16ll * v - mis;                      // the stream position of the vector's byte 0
        const uint32_t m = sbs_in_term16(x) & uat_range16((long long) tile_pos - p0, tile_end - p0);
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

// uat_stage with the terminator mask: s_in[i] is the byte at stream position tile_pos + i - mis - 16 (zeros where no vector of the text
// lies), s_nl[v] the terminator mask of s_in[16 v .. 16 v + 16) over positions inside the stream.  Returns mis.
__device__ __forceinline__ uint32_t sbs_in_stage(const uint8_t *text, uint64_t nbytes, uint8_t *s_in, uint16_t *s_nl) {
    const uint64_t tile_pos = (uint64_t) blockIdx.x * kUatTile;
    const uintptr_t g = reinterpret_cast<uintptr_t>(text) + tile_pos;
    const uint32_t mis = (uint32_t) (g & 15u);
    const uintptr_t a0 = (g & ~(uintptr_t) 15) - 16u;
    for (uint32_t v = threadIdx.x; v < kUatVecs; v += kBlock) {
        const u32x4 x = uat_load(a0 + 16u * v, text, nbytes);
        *reinterpret_cast<u32x4 *>(s_in + 16u * v) = x;
        const long long p0 = (long long) tile_pos + 16ll * v - mis - 16;
        s_nl[v] = (uint16_t) (sbs_in_term16(x) & uat_range16(-p0, (long long) nbytes - p0));
    }
    __syncthreads();
    return mis;
}

// meta of a lane: records of its lines | deferred lines << 8
__global__ __launch_bounds__(kBlock) void k_sbs_in_size(SbsInParams a, const unsigned long long *off_nl, const unsigned long long *total, uint16_t *meta,
                                                        uint32_t *block_recs, uint32_t *block_def, uint32_t *block_inv) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ uint16_t s_nl[kUatVecs];
    __shared__ uint32_t s_wave[kBlock / WAVE];
    const uint32_t mis = sbs_in_stage(a.text, a.nbytes, s_in, s_nl);
    uint32_t starts, own, tile_nl;
    uat_lane_lines(s_nl, mis, starts, own);
    const uint32_t nl_before = uat_block_scan((uint32_t) __popc(own), s_wave, tile_nl);
    const unsigned long long nlines = total[0], first = off_nl[blockIdx.x] + nl_before;
    uint32_t recs = 0, def = 0, inv = 0;
    for (uint32_t rest = starts; rest; rest &= rest - 1u) {
        const uint32_t b = (uint32_t) __ffs(rest) - 1u;
        const uint32_t at = kUatChunk * threadIdx.x + b + mis + 16u;
        const uint32_t n = uat_line_len(s_nl, at);
        const unsigned long long index = first + (uint32_t) __popc(own & ((1u << b) - 1u));
        if (index >= nlines) continue;                                                  // bytes behind the last terminator: not a line
        mgpu_sbs_rec r;
        const int cls = sbs_in_line(s_in + at, n, a.source, a.now_ms, SbsInPlainOnly{}, r);
        recs += cls == SBS_IN_RECORD;
        def += cls == SBS_IN_DEFER;
        inv += cls == SBS_IN_INVALID;
    }
    meta[(size_t) blockIdx.x * kBlock + threadIdx.x] = (uint16_t) (recs | def << 8);
    uint32_t tr, td, ti;
    uat_block_scan(recs, s_wave, tr);
    uat_block_scan(def, s_wave, td);
    uat_block_scan(inv, s_wave, ti);
    if (threadIdx.x == 0) { block_recs[blockIdx.x] = tr; block_def[blockIdx.x] = td; block_inv[blockIdx.x] = ti; }
}

__global__ __launch_bounds__(kBlock) void k_sbs_in_write(SbsInParams a, const unsigned long long *off_nl, const unsigned long long *total, const uint16_t *meta,
                                                         const unsigned long long *off_recs, const unsigned long long *off_def) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ uint16_t s_nl[kUatVecs];
    __shared__ uint32_t s_wave[kBlock / WAVE];
    const uint32_t mis = sbs_in_stage(a.text, a.nbytes, s_in, s_nl);
    uint32_t starts, own, tile_nl, tile_recs, tile_def;
    uat_lane_lines(s_nl, mis, starts, own);
    const uint32_t nl_before = uat_block_scan((uint32_t) __popc(own), s_wave, tile_nl);
    const uint32_t mt = meta[(size_t) blockIdx.x * kBlock + threadIdx.x];
    const uint32_t recs_before = uat_block_scan(mt & 0xffu, s_wave, tile_recs);
    const uint32_t def_before = uat_block_scan(mt >> 8, s_wave, tile_def);
    if (!mt) return;                                                                    // (behind the last barrier)
    const unsigned long long nlines = total[0], first = off_nl[blockIdx.x] + nl_before;
    unsigned long long out = off_recs[blockIdx.x] + recs_before, slot = off_def[blockIdx.x] + def_before;
    for (uint32_t rest = starts; rest; rest &= rest - 1u) {
        const uint32_t b = (uint32_t) __ffs(rest) - 1u;
        const uint32_t at = kUatChunk * threadIdx.x + b + mis + 16u;
        const uint32_t n = uat_line_len(s_nl, at);
        const unsigned long long index = first + (uint32_t) __popc(own & ((1u << b) - 1u));
        if (index >= nlines) continue;
        mgpu_sbs_rec r;
        const int cls = sbs_in_line(s_in + at, n, a.source, a.now_ms, SbsInPlainOnly{}, r);
        if (cls == SBS_IN_RECORD) {
            if (out < a.recs_cap) {
                a.recs[out] = r;
                if (a.line_of) a.line_of[out] = a.line_base + index;
            }
            ++out;
        } else if (cls == SBS_IN_DEFER) {
            if (slot < a.deferred_cap) a.deferred[slot] = a.line_base + index;
            ++slot;
        }
    }
}

void launch_sbs_decode(const SbsInParams &a, const UatScratch &w, hipStream_t s) {
    if (a.nbytes == 0) return;
    const unsigned tiles = (unsigned) ((a.nbytes + kUatTile - 1) / kUatTile);
    uint32_t *b_nl = w.blocks, *b_last = w.blocks + w.stride, *b_recs = w.blocks + 2 * w.stride, *b_def = w.blocks + 3 * w.stride, *b_inv = w.blocks + 4 * w.stride;
    unsigned long long *off_nl = w.off, *off_recs = w.off + w.stride, *off_def = w.off + 2 * w.stride;
    hipLaunchKernelGGL(k_sbs_in_index, dim3(tiles), dim3(kBlock), 0, s, a.text, a.nbytes, b_nl, b_last);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, b_nl, tiles, off_nl, w.total);
    hipLaunchKernelGGL(k_uat_last, dim3(1), dim3(kScanThreads), 0, s, b_last, tiles, w.total + 1);
    hipLaunchKernelGGL(k_sbs_in_size, dim3(tiles), dim3(kBlock), 0, s, a, off_nl, w.total, w.meta, b_recs, b_def, b_inv);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, b_recs, tiles, off_recs, w.total + 2);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, b_def, tiles, off_def, w.total + 3);
    hipLaunchKernelGGL(k_text_sum, dim3(1), dim3(kScanThreads), 0, s, b_inv, tiles, w.total + 4);
    hipLaunchKernelGGL(k_sbs_in_write, dim3(tiles), dim3(kBlock), 0, s, a, off_nl, w.total, w.meta, off_recs, off_def);
}
