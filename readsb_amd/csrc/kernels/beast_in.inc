// kernels/beast_in.inc — beast input: a binary stream in HBM to the messages readsb's --net-bi-port accepts (readBeast,
// net_io.c:4737-5018, with decodeBinMessage, :3804-3961, as its read handler).  Part of the single translation unit kernels.hip
// (included inside namespace mgpu, after raw_in.inc, whose filter passes it ends in, uat.inc's tiles, vector loads and scans, text.inc's
// k_text_sum and beast.inc's k_beast_scan).  The framer and the parser are beast_in_format.h's, the ones the host compiles too.
//
// Where the scan goes from an offset depends on the offset and the bytes alone (beast_in_format.h), and a step reaches at most
// kBeastInMaxFrame = 62 bytes: the chain that passes through a tile of kUatTile bytes enters the NEXT tile at one of its first
// kBeastInHalo = 64 offsets, so a tile is a function from 64 entry offsets to an exit offset, and such functions compose.  No
// workgroup waits for another; the launches are ordered on one stream:
//   k_beast_in_map      per tile (but the last): the tile through LDS in 16-byte loads, the successor of every one of its offsets as
//                       halfwords in LDS (a lane takes every 256th offset), then a lane per entry offset walks the successors to the exit
//   k_beast_in_compose  per group of kBeastInGroup tiles (but the last): the composition of their maps, a lane per entry offset
//   k_beast_in_entries  one workgroup: a lane walks the groups (a dependent load per GROUP), then a lane per group gives each of its
//                       tiles its entry (a dependent load per tile of the group)
//   k_beast_in_mark     per tile the chain enters: the successors again, one lane marks the chain's offsets in a bitmap; every lane then
//                       takes the 0x1a steps among its 32 offsets: the first stop as a minimum over the stream (its offset, the som it
//                       leaves, its kind in one word), the last som of the loop as a maximum
//   k_beast_in_count    per tile, below the stop: garbage bytes (a byte that is no 0x1a counts only in front of the last som: memchr
//                       found a 0x1a behind it), 'W' commands, prefixes taken, handler calls, candidates (handler calls that reach the
//                       decode), Mode A/C frames dropped; per lane and per tile the last receiver id set
//   k_beast_scan twice, k_raw_in_sum; k_beast_in_ids: the id in force at every tile's first offset (last-set over the tiles)
//   k_beast_in_classify per tile: THE SAME framer once more on the marked steps, the id in force carried from lane to lane by a ballot;
//                       per handler call its offset (and its class, unless the filter decides it), per candidate the shared decode
//                       (raw_in_decode_frame) to the raw input's candidate arrays, with the id beside it
// and then raw_in.inc's passes over the candidates (launch_raw_in_resolve): the filter's answers in stream order, the counters, the
// accepted compacted to msgs / receiver_id / frame_of / signal_level and the class per handler call.
constexpr uint32_t kBeastInHalo = 64;            // entry offsets of a tile
constexpr uint32_t kBeastInEnd = 0xffu;          // a map's value for "the chain ends in this tile"
constexpr uint32_t kBeastInSuccEnd = 0xffffu;
static_assert(kBeastInMaxFrame <= kBeastInHalo && kBeastInHalo + kBeastInMaxFrame <= kUatHalo, "a step from a tile's offsets reads staged bytes and exits into the next tile's halo");
static_assert(kUatTile + kBeastInHalo < kBeastInSuccEnd && kUatChunk == 32, "a successor is a halfword; a lane's offsets are one word of the bitmap");
static_assert(kUatLds + 2 * kUatTile + 4 * kBlock + 1024 + 256 <= 65536, "k_beast_in_mark's static LDS");

struct BeastInTile {
    const uint8_t *base;              // LDS: base[o] is the byte at offset o of the tile
    uint64_t n;                       // the stream's bytes from the tile's start on, capped at what is staged
    uint64_t pos;                     // the tile's place in the stream
};

__device__ __forceinline__ BeastInTile beast_in_stage(const uint8_t *data, uint64_t nbytes, uint8_t *s_in) {
    const uint64_t tile_pos = (uint64_t) blockIdx.x * kUatTile;
    const uintptr_t g = reinterpret_cast<uintptr_t>(data) + tile_pos;
    const uint32_t mis = (uint32_t) (g & 15u);
    const uintptr_t a0 = (g & ~(uintptr_t) 15) - 16u;
    for (uint32_t v = threadIdx.x; v < kUatVecs; v += kBlock) *reinterpret_cast<u32x4 *>(s_in + 16u * v) = uat_load(a0 + 16u * v, data, nbytes);
    __syncthreads();
    const uint64_t rest = nbytes - tile_pos;                            // (a grid has nbytes / kUatTile + 1 tiles)
    return BeastInTile{s_in + mis + 16u, rest < kUatTile + kUatHalo ? rest : kUatTile + kUatHalo, tile_pos};
}

__device__ __forceinline__ void beast_in_succ(const BeastInTile &t, uint32_t net_ingest, uint16_t *s_succ) {
    for (uint32_t o = threadIdx.x; o < kUatTile; o += kBlock) {
        BeastInStep st;
        const uint32_t kind = beast_in_step(t.base, t.n, o, net_ingest, st);
        s_succ[o] = (uint16_t) (kind <= BEAST_IN_FRAME ? (uint32_t) st.next : kBeastInSuccEnd);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void k_beast_in_map(const uint8_t *data, uint64_t nbytes, uint32_t net_ingest, uint8_t *maps) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ uint16_t s_succ[kUatTile];
    const BeastInTile t = beast_in_stage(data, nbytes, s_in);
    beast_in_succ(t, net_ingest, s_succ);
    if (threadIdx.x >= kBeastInHalo) return;
    uint32_t o = threadIdx.x;
    while (o < kUatTile) {
        const uint32_t s = s_succ[o];
        if (s == kBeastInSuccEnd) { o = kNone; break; }
        o = s;
    }
    maps[(size_t) blockIdx.x * kBeastInHalo + threadIdx.x] = (uint8_t) (o == kNone ? kBeastInEnd : o - kUatTile);
}

__global__ __launch_bounds__(kBeastInHalo) void k_beast_in_compose(const uint8_t *maps, uint8_t *gmaps) {
    uint32_t v = threadIdx.x;
    for (uint32_t k = 0; k < kBeastInGroup; ++k)
        if (v != kBeastInEnd) v = maps[((size_t) blockIdx.x * kBeastInGroup + k) * kBeastInHalo + v];
    gmaps[(size_t) blockIdx.x * kBeastInHalo + threadIdx.x] = (uint8_t) v;
}

// entry[tiles] then entry[tiles + g] for the groups; total[6] the first stop (all ones: none), total[7] the last som
__global__ __launch_bounds__(kBlock) void k_beast_in_entries(const uint8_t *maps, const uint8_t *gmaps, uint32_t tiles, uint32_t groups, uint32_t *entry,
                                                              unsigned long long *total) {
    uint32_t *gentry = entry + tiles;
    if (threadIdx.x == 0) {
        total[6] = ~0ull;
        total[7] = 0;
        uint32_t e = 0;
        for (uint32_t g = 0; g < groups; ++g) {
            gentry[g] = e;
            if (g + 1 < groups && e != kNone) {
                const uint32_t v = gmaps[(size_t) g * kBeastInHalo + e];
                e = v == kBeastInEnd ? kNone : v;
            }
        }
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < groups; g += kBlock) {
        uint32_t e = gentry[g];
        for (uint32_t t = g * kBeastInGroup; t < (g + 1) * kBeastInGroup && t < tiles; ++t) {
            entry[t] = e;
            if (t + 1 < tiles && e != kNone) {
                const uint32_t v = maps[(size_t) t * kBeastInHalo + e];
                e = v == kBeastInEnd ? kNone : v;
            }
        }
    }
}

__device__ __forceinline__ unsigned long long beast_in_wave_max(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}

// the stop's word: the step's offset << 8 | (the som it leaves - the offset) << 3 | kind
__global__ __launch_bounds__(kBlock) void k_beast_in_mark(const uint8_t *data, uint64_t nbytes, uint32_t net_ingest, const uint32_t *entry, uint32_t *marks,
                                                           unsigned long long *total) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ uint16_t s_succ[kUatTile];
    __shared__ uint32_t s_mark[kBlock];
    const uint32_t e = entry[blockIdx.x];
    if (e == kNone) {                                                   // (the whole workgroup)
        marks[(size_t) blockIdx.x * kBlock + threadIdx.x] = 0;
        return;
    }
    s_mark[threadIdx.x] = 0;
    const BeastInTile t = beast_in_stage(data, nbytes, s_in);
    beast_in_succ(t, net_ingest, s_succ);
    if (threadIdx.x == 0) {
        uint32_t o = e;
        while (o < kUatTile) {
            s_mark[o >> 5] |= 1u << (o & 31u);
            const uint32_t s = s_succ[o];
            if (s == kBeastInSuccEnd) break;
            o = s;
        }
    }
    __syncthreads();
    const uint32_t word = s_mark[threadIdx.x];
    marks[(size_t) blockIdx.x * kBlock + threadIdx.x] = word;
    unsigned long long last = 0;
    for (uint32_t m = word; m; m &= m - 1u) {
        const uint32_t o = kUatChunk * threadIdx.x + (uint32_t) __ffs(m) - 1u;
        if (o >= t.n || t.base[o] != 0x1a) continue;
        BeastInStep st;
        const uint32_t kind = beast_in_step(t.base, t.n, o, net_ingest, st);
        if (kind == BEAST_IN_STOP_SYNTH || kind == BEAST_IN_STOP_UUID)
            atomicMin(total + 6, (unsigned long long) (t.pos + o) << 8 | (unsigned long long) (st.next - o) << 3 | kind);
        last = t.pos + st.next;                                         // (a lane's steps ascend)
    }
    last = beast_in_wave_max(last);
    if (lane_id() == 0 && last) atomicMax(total + 7, last);
}

// What of a marked offset counts: everything below the stop's step; the stop's step itself gives its receiver id only
struct BeastInBound {
    bool has_stop;
    unsigned long long stop_at, last;
};
__device__ __forceinline__ BeastInBound beast_in_bound(const unsigned long long *total) {
    const unsigned long long key = total[6];
    return BeastInBound{key != ~0ull, key >> 8, total[7]};
}

// meta of a lane: handler calls | candidates << 4 | a receiver id set << 15.  blocks[k * tiles + tile], k = 0..5: handler calls,
// candidates, garbage bytes, 'W' commands, prefixes taken, Mode A/C frames dropped
__global__ __launch_bounds__(kBlock) void k_beast_in_count(BeastInParams a, const uint32_t *marks, const unsigned long long *total, uint16_t *meta,
                                                            unsigned long long *lane_ids, uint32_t *blocks, unsigned long long *tile_id, uint32_t *tile_idflag) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ uint32_t s_wave[kBlock / WAVE];
    __shared__ unsigned long long s_wid[kBlock / WAVE];
    __shared__ uint32_t s_whas[kBlock / WAVE];
    const BeastInTile t = beast_in_stage(a.data, a.nbytes, s_in);
    const BeastInBound bd = beast_in_bound(total);
    uint32_t cnt[6] = {0, 0, 0, 0, 0, 0}, has = 0;
    unsigned long long id = 0;
    for (uint32_t m = marks[(size_t) blockIdx.x * kBlock + threadIdx.x]; m; m &= m - 1u) {
        const uint32_t o = kUatChunk * threadIdx.x + (uint32_t) __ffs(m) - 1u;
        const unsigned long long pos = t.pos + o;
        if (o >= t.n) continue;
        if (t.base[o] != 0x1a) { cnt[2] += bd.has_stop ? pos < bd.stop_at : pos < bd.last; continue; }
        if (bd.has_stop && pos > bd.stop_at) continue;
        BeastInStep st;
        const uint32_t kind = beast_in_step(t.base, t.n, o, a.net_ingest, st);
        if (st.id_set) { has = 1; id = st.id; ++cnt[4]; }
        if (bd.has_stop && pos == bd.stop_at) continue;
        cnt[2] += st.garbage;
        cnt[3] += st.wcmd;
        if (kind != BEAST_IN_FRAME) continue;
        ++cnt[0];
        if (beast_in_is_cand(st, a.cfg)) ++cnt[1];
        else if (st.payload[0] == '1') ++cnt[5];
    }
    const size_t lane = (size_t) blockIdx.x * kBlock + threadIdx.x;
    meta[lane] = (uint16_t) (cnt[0] | cnt[1] << 4 | has << 15);
    if (has) lane_ids[lane] = id;
    // the tile's last id: the highest lane that set one
    const unsigned long long bal = __ballot(has);
    const int top = bal ? 63 - __clzll((long long) bal) : -1;
    const unsigned long long wid = __shfl(id, top < 0 ? 0 : top);
    if (lane_id() == 0) { s_whas[threadIdx.x >> 6] = bal != 0; s_wid[threadIdx.x >> 6] = wid; }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        uint32_t tot;
        uat_block_scan(cnt[k], s_wave, tot);
        if (threadIdx.x == 0) blocks[(size_t) k * gridDim.x + blockIdx.x] = tot;
    }
    if (threadIdx.x == 0) {                                             // (the scans' barriers stand behind s_whas and s_wid)
        uint32_t f = 0;
        unsigned long long v = 0;
        for (int k = 0; k < kBlock / WAVE; ++k)
            if (s_whas[k]) { f = 1; v = s_wid[k]; }
        tile_idflag[blockIdx.x] = f;
        tile_id[blockIdx.x] = v;
    }
}

// entry_id[t]: the id in force at tile t's first offset; total[8]: the id the call leaves
__global__ __launch_bounds__(kBlock) void k_beast_in_ids(const unsigned long long *tile_id, const uint32_t *tile_idflag, uint32_t tiles, unsigned long long id_in,
                                                          unsigned long long *entry_id, unsigned long long *total) {
    __shared__ unsigned long long s_id[kBlock];
    __shared__ uint32_t s_has[kBlock];
    const uint32_t per = (tiles + kBlock - 1) / kBlock, t0 = threadIdx.x * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    uint32_t has = 0;
    unsigned long long id = 0;
    for (uint32_t t = t0; t < t1; ++t)
        if (tile_idflag[t]) { has = 1; id = tile_id[t]; }
    s_has[threadIdx.x] = has;
    s_id[threadIdx.x] = id;
    __syncthreads();
    unsigned long long cur = id_in;
    for (int k = (int) threadIdx.x - 1; k >= 0; --k)
        if (s_has[k]) { cur = s_id[k]; break; }
    for (uint32_t t = t0; t < t1; ++t) {
        entry_id[t] = cur;
        if (tile_idflag[t]) cur = tile_id[t];
    }
    if (threadIdx.x == 0) {
        unsigned long long out = id_in;
        for (int k = kBlock - 1; k >= 0; --k)
            if (s_has[k]) { out = s_id[k]; break; }
        total[8] = out;
    }
}

__global__ __launch_bounds__(kBlock) void k_beast_in_classify(BeastInParams a, RawInParams p, const uint32_t *marks, const unsigned long long *total, const uint16_t *meta,
                                                               const unsigned long long *lane_ids, const unsigned long long *entry_id,
                                                               const unsigned long long *off_frames, const unsigned long long *off_cands) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ uint32_t s_wave[kBlock / WAVE];
    __shared__ int s_last[kBlock / WAVE];
    __shared__ uint32_t s_crc[256];
    const RawInTables tb = raw_in_stage_crc(p.tb, s_crc);
    const BeastInTile t = beast_in_stage(a.data, a.nbytes, s_in);
    const BeastInBound bd = beast_in_bound(total);
    const size_t lane0 = (size_t) blockIdx.x * kBlock;
    const uint32_t mt = meta[lane0 + threadIdx.x];
    uint32_t tile_frames, tile_cands;
    const uint32_t frames_before = uat_block_scan(mt & 15u, s_wave, tile_frames);
    const uint32_t cands_before = uat_block_scan((mt >> 4) & 7u, s_wave, tile_cands);
    // the id in force at the lane's first offset: the last lane in front of it that set one, or the tile's
    const unsigned long long bal = __ballot((mt >> 15) & 1u);
    if (lane_id() == 0) s_last[threadIdx.x >> 6] = bal ? (int) (threadIdx.x & ~63u) + 63 - __clzll((long long) bal) : -1;
    __syncthreads();
    const unsigned long long below = bal & ((1ull << lane_id()) - 1ull);
    int src = below ? (int) (threadIdx.x & ~63u) + 63 - __clzll((long long) below) : -1;
    for (int w = (int) (threadIdx.x >> 6) - 1; w >= 0 && src < 0; --w) src = s_last[w];
    if (!(mt & 0x7fu)) return;                                          // no handler call of this lane's (behind the last barrier)
    unsigned long long id = src >= 0 ? lane_ids[lane0 + (uint32_t) src] : entry_id[blockIdx.x];
    unsigned long long frame = off_frames[blockIdx.x] + frames_before, slot = off_cands[blockIdx.x] + cands_before;
    for (uint32_t m = marks[lane0 + threadIdx.x]; m; m &= m - 1u) {
        const uint32_t o = kUatChunk * threadIdx.x + (uint32_t) __ffs(m) - 1u;
        const unsigned long long pos = t.pos + o;
        if (o >= t.n || t.base[o] != 0x1a || (bd.has_stop && pos >= bd.stop_at)) continue;
        BeastInStep st;
        const uint32_t kind = beast_in_step(t.base, t.n, o, a.net_ingest, st);
        if (st.id_set) id = st.id;
        if (kind != BEAST_IN_FRAME) continue;
        if (a.frame_off && frame < a.frames_cap) a.frame_off[frame] = a.off_base + t.pos + st.frame;
        if (beast_in_is_cand(st, a.cfg)) {
            RawInLine r;
            const uint32_t cls = beast_in_frame(st, p.now_ms, p.cfg, tb, r);
            if (slot < p.cand_cap) {
                p.cand_rec[slot] = r.msg;
                p.cand_sig[slot] = r.signal;
                p.cand_line[slot] = (uint32_t) frame;
                p.cand_meta[slot] = (r.addr & kRawMetaAddr) | cls << kRawMetaClsShift | (uint32_t) r.msg.correctedbits << kRawMetaCorrShift | (r.adder ? kRawMetaAdder : 0u);
                a.cand_id[slot] = id;
            }
            ++slot;
        } else if (a.frame_class && frame < a.frames_cap) {
            const uint32_t type = st.payload[0];
            a.frame_class[frame] = (uint8_t) (type == '5' ? MGPU_BEAST_IN_POSITION : type == 'P' ? MGPU_BEAST_IN_PONG : MGPU_BEAST_IN_MODEAC_OFF);
        }
        ++frame;
    }
}

// total: [0] handler calls, [1] candidates, [2] garbage bytes, [3] 'W' commands, [4] prefixes taken, [5] Mode A/C frames dropped,
// [6] the first stop (all ones: none), [7] the last som, [8] the receiver id the call leaves
void launch_beast_in_front(const BeastInParams &a, const RawInParams &p, const BeastInScratch &w, hipStream_t s) {
    const uint32_t tiles = (uint32_t) beast_in_tiles(a.nbytes), groups = (uint32_t) beast_in_groups(a.nbytes);
    unsigned long long *off_frames = w.off, *off_cands = w.off + tiles;
    if (tiles > 1) hipLaunchKernelGGL(k_beast_in_map, dim3(tiles - 1), dim3(kBlock), 0, s, a.data, a.nbytes, a.net_ingest, w.maps);
    if (groups > 1) hipLaunchKernelGGL(k_beast_in_compose, dim3(groups - 1), dim3(kBeastInHalo), 0, s, w.maps, w.gmaps);
    hipLaunchKernelGGL(k_beast_in_entries, dim3(1), dim3(kBlock), 0, s, w.maps, w.gmaps, tiles, groups, w.entry, w.total);
    hipLaunchKernelGGL(k_beast_in_mark, dim3(tiles), dim3(kBlock), 0, s, a.data, a.nbytes, a.net_ingest, w.entry, w.marks, w.total);
    hipLaunchKernelGGL(k_beast_in_count, dim3(tiles), dim3(kBlock), 0, s, a, w.marks, w.total, w.meta, w.lane_ids, w.blocks, w.tile_id, w.tile_idflag);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, w.blocks, tiles, off_frames, w.total);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, w.blocks + tiles, tiles, off_cands, w.total + 1);
    hipLaunchKernelGGL(k_raw_in_sum, dim3(4), dim3(kScanThreads), 0, s, w.blocks + 2 * (size_t) tiles, tiles, w.total + 1);
    hipLaunchKernelGGL(k_beast_in_ids, dim3(1), dim3(kBlock), 0, s, w.tile_id, w.tile_idflag, tiles, a.receiver_id_in, w.entry_id, w.total);
    hipLaunchKernelGGL(k_beast_in_classify, dim3(tiles), dim3(kBlock), 0, s, a, p, w.marks, w.total, w.meta, w.lane_ids, w.entry_id, off_frames, off_cands);
}
