// kernels/pf_in.inc — Planefinder input: a DLE-framed binary stream in HBM to the messages readsb's --net-pfms-in-port accepts
// (readPlanefinder, net_io.c:4670-4735, with decodePfMessage, :3995-4101, as its read handler).  Part of the single translation unit
// kernels.hip (included inside namespace mgpu, after beast_in.inc, whose tile view it uses, raw_in.inc, whose filter passes it ends in,
// uat.inc's tiles, vector loads and scans, and beast.inc's k_beast_scan).  The predicates and the parser are pf_in_format.h's, the
// ones the host compiles too.
//
// The framer is a two-state automaton over two per-byte predicates with one byte of lookahead (pf_in_format.h): B, a DLE that can
// start a frame, and E, a DLE in front of an ETX.  After any event the state is the event's kind, so the state at an offset is the
// kind of the last event in front of it; a B starts a frame iff the last event in front of it is no B; a start is complete iff an E
// lies behind it, and the handler never needs the frame's end.  A frame has no bounded length, so nothing here follows a chain: no
// serial walk over the stream, no workgroup waits for another; the launches are ordered on one stream:
//   k_pf_in_events   per tile: a DLE mask and an ETX mask per 16-byte vector, straight from the loads to LDS (the bytes are not
//                    staged); a lane forms the B and E masks of its 32 bytes, the lookahead bit from the next lane's vector.  Per tile:
//                    the last event's kind, the last E and the kind of the event in front of it, the first B behind it, and the last
//                    DLE that is no B in front of that B
//   k_pf_in_states   one workgroup: the state at every tile's first byte (last-kind over the tiles), the stream's last E, and the
//                    bytes consumed: the larger of the last closed end + 2 and the last DLE met while searching + 1, which is the
//                    last non-B DLE in front of the first B behind the last E
//   k_pf_in_count    per tile, the tile and its halo through LDS: the state carried from lane to lane by a ballot; per complete start
//                    the packet id, and for 0xc1 the handler's reads (pf_in_fields): handler calls, candidates (calls that reach the
//                    decode), frames of another id, calls that read past the end
//   k_beast_scan twice, k_raw_in_sum
//   k_pf_in_classify the same once more: per handler call its offset (and its class, unless the filter decides it), per candidate
//                    the shared decode (raw_in_decode_frame) to the raw input's candidate arrays
// and then raw_in.inc's passes over the candidates (launch_raw_in_resolve).
static_assert(kPfInReach <= kUatHalo, "a handler call from a tile's last byte reads staged bytes");
static_assert(kUatChunk == 32, "a lane's bytes are one word of each mask");
constexpr uint32_t kPfInEventVecs = kUatTile / 16 + 3;          // the vectors that hold the tile and its one byte of lookahead

// bit j: byte j of the vector equals c
__device__ __forceinline__ uint32_t pf_in_eq16(u32x4 v, uint32_t c) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t x = v[j] ^ (c * 0x01010101u);
        const uint32_t y = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);       // 0x80 in every byte that equals c, exactly
        m |= (((y >> 7) & 1u) | ((y >> 14) & 2u) | ((y >> 21) & 4u) | ((y >> 28) & 8u)) << (4 * j);
    }
    return m;
}

// The tile of this workgroup: s_dle[v] and s_etx[v] the masks of vector v (positions inside the stream only), and with s_in the bytes
// as beast_in_stage leaves them.  n: the stream's bytes, what may be loaded; nvecs <= kUatVecs.
__device__ __forceinline__ BeastInTile pf_in_stage(const uint8_t *data, uint64_t n, uint32_t nvecs, uint8_t *s_in, uint16_t *s_dle, uint16_t *s_etx, uint32_t &mis) {
    const uint64_t tile_pos = (uint64_t) blockIdx.x * kUatTile;
    const uintptr_t g = reinterpret_cast<uintptr_t>(data) + tile_pos;
    mis = (uint32_t) (g & 15u);
    const uintptr_t a0 = (g & ~(uintptr_t) 15) - 16u;
    for (uint32_t v = threadIdx.x; v < nvecs; v += kBlock) {
        const u32x4 x = uat_load(a0 + 16u * v, data, n);
        if (s_in) *reinterpret_cast<u32x4 *>(s_in + 16u * v) = x;
        const long long p0 = (long long) tile_pos + 16ll * v - mis - 16;
        const uint32_t in = uat_range16(-p0, (long long) n - p0);
        s_dle[v] = (uint16_t) (pf_in_eq16(x, kPfDle) & in);
        s_etx[v] = (uint16_t) (pf_in_eq16(x, kPfEtx) & in);
    }
    __syncthreads();
    const uint64_t rest = n - tile_pos;                                  // (a grid has ceil(nf / kUatTile) tiles, nf <= n)
    return BeastInTile{s_in ? s_in + mis + 16u : nullptr, rest < kUatTile + kUatHalo ? rest : kUatTile + kUatHalo, tile_pos};
}

// bits b of a lane's word with pos0 + b < x
__device__ __forceinline__ uint32_t pf_in_below(uint64_t pos0, uint64_t x) {
    return x <= pos0 ? 0u : x - pos0 >= 32u ? 0xffffffffu : (1u << (uint32_t) (x - pos0)) - 1u;
}

// What a lane takes: bit b of B / E / X: byte b of its chunk is a start candidate / an end / a DLE that is no start candidate; only
// DLEs below nf are events, the lookahead needs p + 1 < n
__device__ __forceinline__ void pf_in_lane_events(const uint16_t *s_dle, const uint16_t *s_etx, uint32_t mis, uint64_t tile_pos, uint64_t nf, uint64_t n, uint32_t &B, uint32_t &E,
                                                  uint32_t &X) {
    const uint32_t i0 = kUatChunk * threadIdx.x + mis + 16u;                            // the chunk's first byte among the staged ones
    const uint32_t v0 = i0 >> 4, sh = i0 & 15u;
    const uint64_t d48 = (uint64_t) s_dle[v0] | (uint64_t) s_dle[v0 + 1] << 16 | (uint64_t) s_dle[v0 + 2] << 32;
    const uint64_t e48 = (uint64_t) s_etx[v0] | (uint64_t) s_etx[v0 + 1] << 16 | (uint64_t) s_etx[v0 + 2] << 32;
    const uint64_t pos0 = tile_pos + kUatChunk * threadIdx.x;
    const uint32_t D = (uint32_t) (d48 >> sh) & pf_in_below(pos0, nf);
    const uint32_t Dn = (uint32_t) (d48 >> (sh + 1u)), En = (uint32_t) (e48 >> (sh + 1u));
    const uint32_t look = D & pf_in_below(pos0, n ? n - 1 : 0);                         // p + 1 < n
    E = look & En;
    B = look & ~Dn & ~En;
    X = D & ~B;
}

__device__ __forceinline__ uint32_t pf_in_block_max(uint32_t v, uint32_t *s_red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(v, d); v = o > v ? o : v; }
    __syncthreads();
    if (lane_id() == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t m = s_red[0];
    for (int k = 1; k < kBlock / WAVE; ++k) m = s_red[k] > m ? s_red[k] : m;
    return m;
}

constexpr uint32_t PF_EV_NONE = 0, PF_EV_B = 1, PF_EV_E = 2;

// ev[k * tiles + tile]: k = 0 the kind of the tile's last event; 1 + the offset in the tile (0: none) of: k = 1 its last E, k = 2 its
// first B behind that E, k = 3 its last non-B DLE in front of that B; k = 4 the kind of the event in front of its last E (none: 0)
__global__ __launch_bounds__(kBlock) void k_pf_in_events(const uint8_t *data, uint64_t nf, uint64_t n, uint32_t *ev) {
    __shared__ uint16_t s_dle[kPfInEventVecs], s_etx[kPfInEventVecs];
    __shared__ uint32_t s_red[kBlock / WAVE];
    uint32_t mis;
    const BeastInTile t = pf_in_stage(data, n, kPfInEventVecs, nullptr, s_dle, s_etx, mis);
    uint32_t B, E, X;
    pf_in_lane_events(s_dle, s_etx, mis, t.pos, nf, n, B, E, X);
    const uint32_t o0 = kUatChunk * threadIdx.x;
    const uint32_t last_e = pf_in_block_max(E ? o0 + 32u - (uint32_t) __clz(E) : 0u, s_red);
    const uint32_t last_b = pf_in_block_max(B ? o0 + 32u - (uint32_t) __clz(B) : 0u, s_red);
    // the first B behind the last E, as a maximum of the complement
    const uint32_t b_after = B & ~pf_in_below(o0, last_e);                              // bits with o0 + b >= last_e, i.e. behind the E at last_e - 1
    const uint32_t first_b_inv = pf_in_block_max(b_after ? kUatTile - (o0 + (uint32_t) __ffs(b_after) - 1u) : 0u, s_red);
    const uint32_t first_b = first_b_inv ? kUatTile - first_b_inv + 1u : 0u;            // 1 + its offset
    const uint32_t x_before = first_b ? X & pf_in_below(o0, first_b - 1u) : X;
    const uint32_t last_x = pf_in_block_max(x_before ? o0 + 32u - (uint32_t) __clz(x_before) : 0u, s_red);
    // the event in front of the last E: 2 * (1 + its offset) | it is a B
    const uint32_t ev_before = last_e ? (B | E) & pf_in_below(o0, last_e - 1u) : 0u;
    const uint32_t top_before = ev_before ? 31u - (uint32_t) __clz(ev_before) : 0u;
    const uint32_t prev = pf_in_block_max(ev_before ? 2u * (o0 + top_before + 1u) | ((B >> top_before) & 1u) : 0u, s_red);
    if (threadIdx.x == 0) {
        const size_t tiles = gridDim.x;
        ev[4 * tiles + blockIdx.x] = !prev ? PF_EV_NONE : (prev & 1u) ? PF_EV_B : PF_EV_E;
        ev[blockIdx.x] = last_b > last_e ? PF_EV_B : last_e ? PF_EV_E : PF_EV_NONE;
        ev[tiles + blockIdx.x] = last_e;
        ev[2 * tiles + blockIdx.x] = first_b;
        ev[3 * tiles + blockIdx.x] = last_x;
    }
}

// in_frame[t]: the state at tile t's first byte; total[4] the bytes consumed, total[5] 1 + the stream's last E (0: none)
__global__ __launch_bounds__(kBlock) void k_pf_in_states(const uint32_t *ev, uint32_t tiles, uint8_t *in_frame, unsigned long long *total) {
    __shared__ uint32_t s_kind[kBlock], s_found[kBlock];
    __shared__ unsigned long long s_e[kBlock], s_x[kBlock];
    const uint32_t *kind = ev, *last_e = ev + tiles, *first_b = ev + 2 * (size_t) tiles, *last_x = ev + 3 * (size_t) tiles;
    const uint32_t per = (tiles + kBlock - 1) / kBlock, t0 = threadIdx.x * per < tiles ? threadIdx.x * per : tiles, t1 = t0 + per < tiles ? t0 + per : tiles;
    uint32_t k = PF_EV_NONE;
    unsigned long long e = 0;
    for (uint32_t t = t0; t < t1; ++t) {
        if (kind[t]) k = kind[t];
        if (last_e[t]) e = (unsigned long long) t * kUatTile + last_e[t];
    }
    s_kind[threadIdx.x] = k;
    s_e[threadIdx.x] = e;
    __syncthreads();
    uint32_t cur = PF_EV_NONE;
    for (int j = (int) threadIdx.x - 1; j >= 0; --j)
        if (s_kind[j]) { cur = s_kind[j]; break; }
    for (uint32_t t = t0; t < t1; ++t) {
        in_frame[t] = cur == PF_EV_B;
        if (kind[t]) cur = kind[t];
    }
    unsigned long long qe1 = 0;                                          // 1 + the last E (the chunks ascend)
    for (int j = 0; j < kBlock; ++j)
        if (s_e[j]) qe1 = s_e[j];
    // from the last E's tile on: the last non-B DLE up to the first tile with a B behind that E
    const uint32_t te = qe1 ? (uint32_t) ((qe1 - 1) / kUatTile) : 0u;
    unsigned long long x = 0;
    uint32_t found = 0;
    for (uint32_t t = t0 > te ? t0 : te; t < t1 && !found; ++t) {
        if (last_x[t]) x = (unsigned long long) t * kUatTile + last_x[t];
        found = first_b[t] != 0;
    }
    s_x[threadIdx.x] = x;
    s_found[threadIdx.x] = found;
    __syncthreads();
    if (threadIdx.x == 0) {
        // the last E closes a frame iff the event in front of it is a B; one met while searching is a DLE like any other, and counts below
        const bool closes = qe1 && (ev[4 * (size_t) tiles + te] ? ev[4 * (size_t) tiles + te] == PF_EV_B : in_frame[te] != 0);
        unsigned long long consumed = closes ? qe1 + 1 : 0;              // the last closed end + 2
        for (int j = 0; j < kBlock; ++j) {
            consumed = s_x[j] > consumed ? s_x[j] : consumed;            // a DLE met while searching + 1
            if (s_found[j]) break;
        }
        total[4] = consumed;
        total[5] = qe1;
    }
}

// The state in front of a lane's bytes: the kind of the last event of the lanes in front of it, or the tile's entry state
__device__ __forceinline__ bool pf_in_lane_state(uint32_t B, uint32_t E, bool tile_in_frame, uint32_t *s_wkind) {
    const uint32_t k = (B | E) == 0 ? PF_EV_NONE : B > E ? PF_EV_B : PF_EV_E;           // (the higher top bit is the larger word)
    const unsigned long long bal = __ballot(k != PF_EV_NONE);
    const int top = bal ? 63 - __clzll((long long) bal) : 0;
    const uint32_t wk = __shfl(k, top);
    if (lane_id() == 0) s_wkind[threadIdx.x >> 6] = bal ? wk : PF_EV_NONE;
    const unsigned long long below = bal & ((1ull << lane_id()) - 1ull);
    const uint32_t pk = __shfl(k, below ? 63 - __clzll((long long) below) : 0);
    __syncthreads();
    uint32_t cur = below ? pk : PF_EV_NONE;
    for (int w = (int) (threadIdx.x >> 6) - 1; w >= 0 && cur == PF_EV_NONE; --w) cur = s_wkind[w];
    return cur == PF_EV_NONE ? tile_in_frame : cur == PF_EV_B;
}

// the frame starts among a lane's B bits: those in front of which the state is "searching"
__device__ __forceinline__ uint32_t pf_in_lane_starts(uint32_t B, uint32_t E, bool in_frame) {
    uint32_t starts = 0;
    for (uint32_t m = B | E; m; m &= m - 1u) {
        const uint32_t bit = m & (0u - m);
        if (B & bit) { if (!in_frame) starts |= bit; in_frame = true; } else in_frame = false;
    }
    return starts;
}

// meta of a lane: handler calls | candidates << 8.  blocks[k * tiles + tile], k = 0..3: handler calls, candidates, frames of another
// packet id, handler calls that read past the end
__global__ __launch_bounds__(kBlock) void k_pf_in_count(PfInParams a, const uint8_t *tile_in_frame, const unsigned long long *total, uint16_t *meta, uint32_t *blocks) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ uint16_t s_dle[kUatVecs], s_etx[kUatVecs];
    __shared__ uint32_t s_wave[kBlock / WAVE];
    uint32_t mis;
    const uint64_t n = a.nbytes + a.look;
    const BeastInTile t = pf_in_stage(a.data, n, kUatVecs, s_in, s_dle, s_etx, mis);
    uint32_t B, E, X;
    pf_in_lane_events(s_dle, s_etx, mis, t.pos, a.nbytes, n, B, E, X);
    const bool in_frame = pf_in_lane_state(B, E, tile_in_frame[blockIdx.x] != 0, s_wave);
    const unsigned long long qe1 = total[5];
    uint32_t cnt[4] = {0, 0, 0, 0};
    for (uint32_t m = pf_in_lane_starts(B, E, in_frame); m; m &= m - 1u) {
        const uint32_t o = kUatChunk * threadIdx.x + (uint32_t) __ffs(m) - 1u;
        if (t.pos + o + 1 >= qe1) continue;                             // no E behind it: the stream's last start, incomplete
        if (t.base[o + 1] != kPfId) { ++cnt[2]; continue; }
        PfInFields f;
        const uint32_t cls = pf_in_fields(t.base, t.n, o, a.cfg.mode_ac, f);
        ++cnt[0];
        cnt[1] += cls == 0;
        cnt[3] += f.past;
    }
    meta[(size_t) blockIdx.x * kBlock + threadIdx.x] = (uint16_t) (cnt[0] | cnt[1] << 8);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t tot;
        uat_block_scan(cnt[k], s_wave, tot);
        if (threadIdx.x == 0) blocks[(size_t) k * gridDim.x + blockIdx.x] = tot;
    }
}

__global__ __launch_bounds__(kBlock) void k_pf_in_classify(PfInParams a, RawInParams p, const uint8_t *tile_in_frame, const unsigned long long *total, const uint16_t *meta,
                                                            const unsigned long long *off_frames, const unsigned long long *off_cands) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ uint16_t s_dle[kUatVecs], s_etx[kUatVecs];
    __shared__ uint32_t s_wave[kBlock / WAVE];
    __shared__ uint32_t s_crc[256];
    const RawInTables tb = raw_in_stage_crc(p.tb, s_crc);
    uint32_t mis;
    const uint64_t n = a.nbytes + a.look;
    const BeastInTile t = pf_in_stage(a.data, n, kUatVecs, s_in, s_dle, s_etx, mis);
    uint32_t B, E, X;
    pf_in_lane_events(s_dle, s_etx, mis, t.pos, a.nbytes, n, B, E, X);
    const bool in_frame = pf_in_lane_state(B, E, tile_in_frame[blockIdx.x] != 0, s_wave);
    const uint32_t mt = meta[(size_t) blockIdx.x * kBlock + threadIdx.x];
    uint32_t tile_frames, tile_cands;
    const uint32_t frames_before = uat_block_scan(mt & 0xffu, s_wave, tile_frames);
    const uint32_t cands_before = uat_block_scan(mt >> 8, s_wave, tile_cands);
    if (!mt) return;                                                    // no handler call of this lane's (behind the last barrier)
    const unsigned long long qe1 = total[5];
    unsigned long long frame = off_frames[blockIdx.x] + frames_before, slot = off_cands[blockIdx.x] + cands_before;
    for (uint32_t m = pf_in_lane_starts(B, E, in_frame); m; m &= m - 1u) {
        const uint32_t o = kUatChunk * threadIdx.x + (uint32_t) __ffs(m) - 1u;
        if (t.pos + o + 1 >= qe1 || t.base[o + 1] != kPfId) continue;
        PfInFields f;
        const uint32_t early = pf_in_fields(t.base, t.n, o, a.cfg.mode_ac, f);
        if (a.frame_off && frame < a.frames_cap) a.frame_off[frame] = a.off_base + t.pos + o;
        if (!early) {
            RawInLine r;
            const uint32_t cls = pf_in_frame(f, p.now_ms, p.cfg, tb, r);
            if (slot < p.cand_cap) {
                p.cand_rec[slot] = r.msg;
                p.cand_sig[slot] = r.signal;
                p.cand_line[slot] = (uint32_t) frame;
                p.cand_meta[slot] = (r.addr & kRawMetaAddr) | cls << kRawMetaClsShift | (uint32_t) r.msg.correctedbits << kRawMetaCorrShift | (r.adder ? kRawMetaAdder : 0u);
            }
            ++slot;
        } else if (a.frame_class && frame < a.frames_cap) a.frame_class[frame] = (uint8_t) early;
        ++frame;
    }
}

// total: [0] handler calls, [1] candidates, [2] frames of another packet id, [3] handler calls that read past the end, [4] the bytes
// consumed, [5] 1 + the stream's last E
void launch_pf_in_front(const PfInParams &a, const RawInParams &p, const PfInScratch &w, hipStream_t s) {
    const uint32_t tiles = (uint32_t) pf_in_tiles(a.nbytes);
    unsigned long long *off_frames = w.off, *off_cands = w.off + tiles;
    hipLaunchKernelGGL(k_pf_in_events, dim3(tiles), dim3(kBlock), 0, s, a.data, a.nbytes, a.nbytes + a.look, w.ev);
    hipLaunchKernelGGL(k_pf_in_states, dim3(1), dim3(kBlock), 0, s, w.ev, tiles, w.in_frame, w.total);
    hipLaunchKernelGGL(k_pf_in_count, dim3(tiles), dim3(kBlock), 0, s, a, w.in_frame, w.total, w.meta, w.blocks);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, w.blocks, tiles, off_frames, w.total);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, w.blocks + tiles, tiles, off_cands, w.total + 1);
    hipLaunchKernelGGL(k_raw_in_sum, dim3(2), dim3(kScanThreads), 0, s, w.blocks + 2 * (size_t) tiles, tiles, w.total + 1);
    hipLaunchKernelGGL(k_pf_in_classify, dim3(tiles), dim3(kBlock), 0, s, a, p, w.in_frame, w.total, w.meta, off_frames, off_cands);
}
