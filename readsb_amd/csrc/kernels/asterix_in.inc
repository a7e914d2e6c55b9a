// kernels/asterix_in.inc — ASTERIX input: a stream of length-prefixed records in HBM to the aircraft records readsb's
// --net-asterix-in-port makes of its CAT021 records (readAsterix, net_io.c:4643-4659, in front of decodeAsterixMessage, :1922-2407).
// Part of the single translation unit kernels.hip (included inside namespace mgpu, after beast.inc's k_beast_scan and text.inc's
// k_text_sum).  The parser and the framing rule are asterix_in_format.h's, the ones the host compiles too.
//
// Where record k + 1 starts is known only from record k, so the stream cannot be cut at a byte as a text can at '\n'.  But a length
// is below 65536 = kAstTile: the chain that enters a tile at some offset leaves it into the NEXT tile at some offset, so a tile is a
// function from 16-bit entry offsets to 16-bit entry offsets, and such functions compose.  No workgroup waits for another; the
// launches are ordered on one stream:
//   k_ast_in_map      per tile (but the last): the step of every one of its 65536 offsets (an offset inside the tile, or itself
//                     where the step leaves the tile or the chain stops) as halfwords in LDS, doubled in place until nothing moves
//                     (16 rounds at the most, 11 for records of 40 bytes): every offset then holds the LAST offset of its chain
//                     inside the tile, whose own step gives the exit.  A round reads a lane's 64 values into registers
//                     before one is written, so the rounds need no second buffer.
//   k_ast_in_compose  per group of kAstGroup tiles (but the last): the composition of their maps, for every entry offset; 16 workgroups
//                     per group, 16 independent chains of gathers in flight per lane
//   k_ast_in_walk     one lane: the entry of every group, a dependent load per GROUP; k_ast_in_expand: a lane per group, the entry of
//                     each of its tiles, a dependent load per tile of the group
//   k_ast_in_mark     per tile the chain enters: the same doubling, with a bitmap beside it: in round k every marked offset marks
//                     the offset 2^k steps on, so after it the first 2^(k+1) starts of the chain are marked (here a round reads
//                     every value before one is written: the steps must be exact).  Then a lane per 64 bytes classifies the marked
//                     starts with the parser: three bitmaps per tile (frames | those that give a record | those of another
//                     category), the first frame that closes the client as a minimum over the stream, the place the chain ends
//   k_ast_in_count    per tile: the counts below that minimum; k_beast_scan twice, k_text_sum twice, k_ast_in_finish
//   k_ast_in_decode   per tile: a lane per 64 bytes runs THE SAME parser on the starts of its bits straight from the stream and
//                     stores the record, eight 16-byte vectors, at its scanned slot
constexpr int kAstBlock = 1024;
constexpr uint32_t kAstPer = kAstTile / kAstBlock;        // offsets per lane in the doubling; also the bytes whose starts a lane classifies
constexpr uint32_t kAstEnd = 0xffffu;                     // a map's value for "the chain ends in this tile"; an exit offset is at most 65534
static_assert(kAstPer == 64 && kAstWords == 2 * kAstBlock && kAstInMaxLen < kAstTile, "a lane owns two words of a tile's bitmaps; a step reaches the next tile only");
static_assert(kAstTile * 2 + kAstWords * 4 + 256 <= 160 * 1024, "k_ast_in_mark's static LDS");

// the step at offset o of the tile at tile_pos: the offset of the next start counted from the tile's (past kAstTile: in the next tile), or kNone
__device__ __forceinline__ uint32_t ast_in_step(const AstBytes &s, uint64_t tile_pos, uint32_t o) {
    uint32_t len;
    return ast_in_frame(s, tile_pos + o, len) == AST_IN_FRAME ? o + len : kNone;
}

__device__ __forceinline__ void ast_in_steps(const AstBytes &s, uint64_t tile_pos, uint16_t *s_j) {
    for (uint32_t o = threadIdx.x; o < kAstTile; o += kAstBlock) {
        const uint32_t v = ast_in_step(s, tile_pos, o);
        s_j[o] = (uint16_t) (v < kAstTile ? v : o);
    }
    __syncthreads();
}

// s_j[o] <- the last offset of o's chain inside the tile.  MARK: s_mark <- every start of the chains from the offsets marked at entry.
template <bool MARK>
__device__ __forceinline__ void ast_in_double(uint16_t *s_j, uint32_t *s_mark) {
    for (int round = 0; round < 16; ++round) {
        if (MARK) {
            for (uint32_t w = threadIdx.x; w < kAstWords; w += kAstBlock)
                for (uint32_t m = s_mark[w]; m; m &= m - 1u) {
                    const uint32_t o = 32u * w + (uint32_t) __ffs(m) - 1u, t = s_j[o];
                    if (t != o) atomicOr(&s_mark[t >> 5], 1u << (t & 31u));   // (an offset marked meanwhile marks a start too: only starts are ever marked)
                }
            __syncthreads();
        }
        uint16_t nj[kAstPer];
        bool moved = false;
#pragma unroll
        for (uint32_t i = 0; i < kAstPer; ++i) {
            const uint32_t v = s_j[i * kAstBlock + threadIdx.x];
            nj[i] = s_j[v];
            moved |= nj[i] != v;
        }
        const int any = __syncthreads_or(moved);                      // every value is read before one is written: a round is 2^round steps exactly
#pragma unroll
        for (uint32_t i = 0; i < kAstPer; ++i) s_j[i * kAstBlock + threadIdx.x] = nj[i];
        __syncthreads();
        if (!any) break;
    }
}

__global__ __launch_bounds__(kAstBlock) void k_ast_in_map(const uint8_t *data, uint64_t nbytes, uint16_t *maps) {
    __shared__ uint16_t s_j[kAstTile];
    const AstBytes s = {data, nbytes};
    const uint64_t tile_pos = (uint64_t) blockIdx.x * kAstTile;
    ast_in_steps(s, tile_pos, s_j);
    ast_in_double<false>(s_j, nullptr);
    for (uint32_t o = threadIdx.x; o < kAstTile; o += kAstBlock) {
        const uint32_t v = ast_in_step(s, tile_pos, s_j[o]);          // of the chain's last offset in the tile: it leaves, or the chain stops
        maps[(size_t) blockIdx.x * kAstTile + o] = (uint16_t) (v == kNone ? kAstEnd : v - kAstTile);
    }
}

// a workgroup takes kAstComposePer * kBlock entry offsets of one group: 16 slices per group, so that 21 groups fill the device
constexpr uint32_t kAstComposePer = 16, kAstComposeSlices = kAstTile / (kAstComposePer * kBlock);
__global__ __launch_bounds__(kBlock) void k_ast_in_compose(const uint16_t *maps, uint16_t *gmaps) {
    const uint32_t g = blockIdx.x / kAstComposeSlices, first = (blockIdx.x % kAstComposeSlices) * (kAstComposePer * kBlock);
    uint16_t v[kAstComposePer];
#pragma unroll
    for (uint32_t i = 0; i < kAstComposePer; ++i) v[i] = (uint16_t) (first + i * kBlock + threadIdx.x);
    for (uint32_t t = 0; t < kAstGroup; ++t) {
        const uint16_t *m = maps + ((size_t) g * kAstGroup + t) * kAstTile;
#pragma unroll
        for (uint32_t i = 0; i < kAstComposePer; ++i)
            if (v[i] != kAstEnd) v[i] = m[v[i]];
    }
#pragma unroll
    for (uint32_t i = 0; i < kAstComposePer; ++i) gmaps[(size_t) g * kAstTile + first + i * kBlock + threadIdx.x] = v[i];
}

__global__ void k_ast_in_walk(const uint16_t *gmaps, uint32_t groups, uint32_t *gentry, unsigned long long *total) {
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 6; ++k) total[k] = 0;
    total[6] = ~0ull;
    total[7] = 0;
    total[8] = AST_IN_END;
    uint32_t e = 0;
    for (uint32_t g = 0; g < groups; ++g) {
        gentry[g] = e;
        if (g + 1 < groups && e != kNone) {
            const uint32_t v = gmaps[(size_t) g * kAstTile + e];
            e = v == kAstEnd ? kNone : v;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_ast_in_expand(const uint16_t *maps, uint32_t tiles, uint32_t groups, const uint32_t *gentry, uint32_t *entry) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= groups) return;
    uint32_t e = gentry[g];
    for (uint32_t t = g * kAstGroup; t < (g + 1) * kAstGroup && t < tiles; ++t) {
        entry[t] = e;
        if (t + 1 < tiles && e != kNone) {
            const uint32_t v = maps[(size_t) t * kAstTile + e];
            e = v == kAstEnd ? kNone : v;
        }
    }
}

__global__ __launch_bounds__(kAstBlock) void k_ast_in_mark(AstInParams a, const uint32_t *entry, uint32_t *bits, size_t tiles, unsigned long long *total) {
    __shared__ uint16_t s_j[kAstTile];
    __shared__ uint32_t s_mark[kAstWords];
    uint32_t *marks = bits + (size_t) blockIdx.x * kAstWords, *recs = marks + tiles * kAstWords, *other = recs + tiles * kAstWords;
    const uint32_t e = entry[blockIdx.x];
    if (e == kNone) {                                                 // (the whole workgroup)
        for (uint32_t w = threadIdx.x; w < kAstWords; w += kAstBlock) { marks[w] = 0; recs[w] = 0; other[w] = 0; }
        return;
    }
    const AstBytes s = {a.data, a.nbytes};
    const uint64_t tile_pos = (uint64_t) blockIdx.x * kAstTile;
    for (uint32_t w = threadIdx.x; w < kAstWords; w += kAstBlock) s_mark[w] = w == (e >> 5) ? 1u << (e & 31u) : 0u;
    ast_in_steps(s, tile_pos, s_j);
    ast_in_double<true>(s_j, s_mark);
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t w = 2u * threadIdx.x + k;
        uint32_t mk = 0, rc = 0, ot = 0;
        for (uint32_t m = s_mark[w]; m; m &= m - 1u) {
            const uint32_t b = (uint32_t) __ffs(m) - 1u;
            const uint64_t pos = tile_pos + 32u * w + b;
            uint32_t len;
            const int st = ast_in_frame(s, pos, len);
            if (st != AST_IN_FRAME) {                                 // where the chain ends: one place in the stream
                total[7] = pos;
                total[8] = (unsigned long long) st;
                continue;
            }
            mgpu_asterix_rec r;
            const int cls = ast_in_record(AstBytes{a.data, a.nbytes + a.look}, pos, a.source, a.now_ms, r);
            mk |= 1u << b;
            rc |= (uint32_t) (cls == AST_IN_RECORD) << b;
            ot |= (uint32_t) (cls == AST_IN_OTHER) << b;
            if (cls == AST_IN_CLOSED) atomicMin(total + 6, (unsigned long long) pos);
        }
        marks[w] = mk; recs[w] = rc; other[w] = ot;
    }
}

// the bits of word w of a tile's bitmap whose stream positions are <= last
__device__ __forceinline__ uint32_t ast_in_upto(uint64_t tile_pos, uint32_t w, unsigned long long last) {
    const uint64_t base = tile_pos + 32u * w;
    return base > last ? 0u : last - base >= 31u ? ~0u : (2u << (uint32_t) (last - base)) - 1u;
}

// exclusive prefix sum over the workgroup of kAstBlock; s_wave: kAstBlock / WAVE words of LDS nobody else uses meanwhile
__device__ __forceinline__ uint32_t ast_in_block_scan(uint32_t v, uint32_t *s_wave, uint32_t &total) {
    int wtotal;
    const int ex = wave_excl_scan((int) v, wtotal);
    __syncthreads();
    if (lane_id() == 0) s_wave[threadIdx.x >> 6] = (uint32_t) wtotal;
    __syncthreads();
    uint32_t before = (uint32_t) ex, all = 0;
    for (uint32_t k = 0; k < kAstBlock / WAVE; ++k) {
        if (k < (threadIdx.x >> 6)) before += s_wave[k];
        all += s_wave[k];
    }
    total = all;
    return before;
}

__global__ __launch_bounds__(kAstBlock) void k_ast_in_count(const uint32_t *bits, size_t tiles, const unsigned long long *total, uint32_t *b_frames, uint32_t *b_recs,
                                                            uint32_t *b_other, uint32_t *b_undef) {
    __shared__ uint32_t s_wave[kAstBlock / WAVE];
    const uint32_t *marks = bits + (size_t) blockIdx.x * kAstWords, *recs = marks + tiles * kAstWords, *other = recs + tiles * kAstWords;
    const unsigned long long closed = total[6];
    const uint64_t tile_pos = (uint64_t) blockIdx.x * kAstTile;
    uint32_t nf = 0, nr = 0, no = 0, nu = 0;
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t w = 2u * threadIdx.x + k, keep = ast_in_upto(tile_pos, w, closed);
        const uint32_t mk = marks[w] & keep, rc = recs[w] & keep, ot = other[w] & keep;
        uint32_t un = mk & ~rc & ~ot;
        if (closed - (tile_pos + 32u * w) < 32u) un &= ~(1u << (uint32_t) (closed - (tile_pos + 32u * w)));   // the closing frame is not undefined
        nf += (uint32_t) __popc(mk); nr += (uint32_t) __popc(rc); no += (uint32_t) __popc(ot); nu += (uint32_t) __popc(un);
    }
    uint32_t tf, tr, to, tu;
    ast_in_block_scan(nf, s_wave, tf);
    ast_in_block_scan(nr, s_wave, tr);
    ast_in_block_scan(no, s_wave, to);
    ast_in_block_scan(nu, s_wave, tu);
    if (threadIdx.x == 0) { b_frames[blockIdx.x] = tf; b_recs[blockIdx.x] = tr; b_other[blockIdx.x] = to; b_undef[blockIdx.x] = tu; }
}

__global__ void k_ast_in_finish(const uint8_t *data, uint64_t nbytes, unsigned long long *total) {
    if (threadIdx.x != 0) return;
    const unsigned long long closed = total[6];
    if (closed != ~0ull) {
        uint32_t len;
        ast_in_frame(AstBytes{data, nbytes}, closed, len);
        total[4] = closed + len;
        total[5] = MGPU_AST_STOP_CLOSED;
    } else {
        total[4] = total[7];
        total[5] = total[8] == AST_IN_ZERO_LEN ? MGPU_AST_STOP_ZERO_LEN : MGPU_AST_STOP_END;
    }
}

__global__ __launch_bounds__(kAstBlock) void k_ast_in_decode(AstInParams a, const uint32_t *bits, size_t tiles, const unsigned long long *total,
                                                             const unsigned long long *off_frames, const unsigned long long *off_recs) {
    __shared__ uint32_t s_wave[kAstBlock / WAVE];
    const uint32_t *marks = bits + (size_t) blockIdx.x * kAstWords, *recs = marks + tiles * kAstWords;
    const unsigned long long closed = total[6];
    const uint64_t tile_pos = (uint64_t) blockIdx.x * kAstTile;
    uint32_t mk[2], rc[2];
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t w = 2u * threadIdx.x + k, keep = ast_in_upto(tile_pos, w, closed);
        mk[k] = marks[w] & keep;
        rc[k] = recs[w] & keep;
    }
    uint32_t tile_frames, tile_recs;
    const uint32_t frames_before = ast_in_block_scan((uint32_t) (__popc(mk[0]) + __popc(mk[1])), s_wave, tile_frames);
    const uint32_t recs_before = ast_in_block_scan((uint32_t) (__popc(rc[0]) + __popc(rc[1])), s_wave, tile_recs);
    if (!(rc[0] | rc[1])) return;                                     // (behind the last barrier)
    const AstBytes s = {a.data, a.nbytes + a.look};
    unsigned long long out = off_recs[blockIdx.x] + recs_before, frame = a.frame_base + off_frames[blockIdx.x] + frames_before;
    for (uint32_t k = 0; k < 2; ++k) {
        for (uint32_t m = rc[k]; m; m &= m - 1u) {
            const uint32_t b = (uint32_t) __ffs(m) - 1u;
            if (out < a.recs_cap) {
                __attribute__((aligned(16))) mgpu_asterix_rec r;
                ast_in_record(s, tile_pos + 64u * threadIdx.x + 32u * k + b, a.source, a.now_ms, r);
                const u32x4 *v = reinterpret_cast<const u32x4 *>(&r);
                u32x4 *dst = reinterpret_cast<u32x4 *>(a.recs + out);
#pragma unroll
                for (int j = 0; j < (int) (sizeof r / 16); ++j) dst[j] = v[j];
                if (a.frame_of) a.frame_of[out] = frame + (uint32_t) __popc(mk[k] & ((1u << b) - 1u));
            }
            ++out;
        }
        frame += (uint32_t) __popc(mk[k]);
    }
}

void launch_asterix_decode(const AstInParams &a, const AstInScratch &w, hipStream_t s) {
    if (a.nbytes == 0) return;
    const uint32_t tiles = (uint32_t) ast_in_tiles(a.nbytes), groups = (uint32_t) ast_in_groups(a.nbytes);
    uint32_t *gentry = w.entry + tiles;
    uint32_t *b_frames = w.blocks, *b_recs = w.blocks + w.stride, *b_other = w.blocks + 2 * w.stride, *b_undef = w.blocks + 3 * w.stride;
    unsigned long long *off_frames = w.off, *off_recs = w.off + w.stride;
    if (tiles > 1) hipLaunchKernelGGL(k_ast_in_map, dim3(tiles - 1), dim3(kAstBlock), 0, s, a.data, a.nbytes, w.maps);
    if (groups > 1) hipLaunchKernelGGL(k_ast_in_compose, dim3((groups - 1) * kAstComposeSlices), dim3(kBlock), 0, s, w.maps, w.gmaps);
    hipLaunchKernelGGL(k_ast_in_walk, dim3(1), dim3(WAVE), 0, s, w.gmaps, groups, gentry, w.total);
    hipLaunchKernelGGL(k_ast_in_expand, dim3((groups + kBlock - 1) / kBlock), dim3(kBlock), 0, s, w.maps, tiles, groups, gentry, w.entry);
    hipLaunchKernelGGL(k_ast_in_mark, dim3(tiles), dim3(kAstBlock), 0, s, a, w.entry, w.bits, (size_t) tiles, w.total);
    hipLaunchKernelGGL(k_ast_in_count, dim3(tiles), dim3(kAstBlock), 0, s, w.bits, (size_t) tiles, w.total, b_frames, b_recs, b_other, b_undef);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, b_frames, tiles, off_frames, w.total);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, b_recs, tiles, off_recs, w.total + 1);
    hipLaunchKernelGGL(k_text_sum, dim3(1), dim3(kScanThreads), 0, s, b_other, tiles, w.total + 2);
    hipLaunchKernelGGL(k_text_sum, dim3(1), dim3(kScanThreads), 0, s, b_undef, tiles, w.total + 3);
    hipLaunchKernelGGL(k_ast_in_finish, dim3(1), dim3(WAVE), 0, s, a.data, a.nbytes, w.total);
    hipLaunchKernelGGL(k_ast_in_decode, dim3(tiles), dim3(kAstBlock), 0, s, a, w.bits, (size_t) tiles, w.total, off_frames, off_recs);
}
