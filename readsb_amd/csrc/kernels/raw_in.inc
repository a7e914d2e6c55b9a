// kernels/raw_in.inc — raw input: a stream of AVR lines in HBM to the messages readsb's --net-ri-port accepts (processHexMessage ->
// decodeHexMessage, net_io.c:4104-4317, behind readAscii, :4599-4641; the front of decodeModesMessage, mode_s.c:443-606, and its
// icaoFilterAdd, :766-779).  Part of the single translation unit kernels.hip (included inside namespace mgpu, after sbs_in.inc, whose
// terminator masks, staging and index pass it uses, uat.inc's tiles, halo, scans and line search, text.inc's k_text_sum and
// beast.inc's k_beast_scan).  The parser is raw_in_format.h's, the one the host compiles too.  No workgroup waits for another.
//
// Over the text (workgroup = tile of kUatTile bytes, a lane takes the lines that start in its 32 bytes):
//   k_sbs_in_index, k_beast_scan, k_uat_last   the lines of every tile, the bytes consumed
//   k_raw_in_size      the parser per line: per lane the lines that are CANDIDATES (any class but "not a frame")
//   k_beast_scan       -> every tile's first candidate slot
//   k_raw_in_classify  THE SAME parser, once more, and per candidate, in line order, to library scratch: the 64-byte record, the
//                      signal double, the line, and a word class | correctedbits | adder | address.  (Scratch and not the record's
//                      final place: that place is the number of ACCEPTED lines in front, which is the filter's answer.)
// Over the candidates (lane = candidate; j = its index, which ascends with the line):
//   k_raw_in_first     every adder: first[addr] = min(first[addr], j) — a 2^24-entry table, all ones outside a call
//   k_raw_in_new       a NEW ADD is an adder that is the first of its address, whose address the ACTIVE generation does not hold: it
//                      is what makes the reference's `occupied` grow.  Per workgroup their number; k_beast_scan numbers them
//   k_raw_in_mark      the new adds compacted in line order; the k*-th one (k* = buckets / 3 - occupied + 1, icao_filter.c:127)
//                      makes the table grow, which drops the inactive generation (icaoFilterResize, :65-93): L* = its j
//   k_raw_in_verdict   a conditional candidate passes iff its address is in the active generation, or j <= L* and it is in the
//                      inactive one, or first[addr] < j; the final class; per workgroup the accepted and the six counters (in LDS:
//                      global atomics on the same seven words from every wave made this pass the longest); k_raw_in_sum adds them up
//   k_beast_scan, k_raw_in_write   the accepted compacted in line order to msgs / line_of / signal_level, the class per line, and
//                      first[] put back to all ones by the adders themselves.
// The generation bitmaps and first[] are read by dependent loads, one or two a candidate: the candidates are a sixth of the text's
// bytes at the most and the passes over them are a small part of the whole (DESIGN.md §4).
static_assert(kUatHalo >= kRawInMaxLine && kUatDevLineMax >= kRawInMaxLine, "the halo holds every byte that decides a line");
static_assert(kUatChunk / (kRawInMinLine + 1) + 1 < 256, "a lane's candidates fit its meta's byte");

constexpr uint32_t kRawMetaAddr = 0xffffffu, kRawMetaClsShift = 24, kRawMetaCorrShift = 28, kRawMetaAdder = 1u << 31;

__device__ __forceinline__ RawInTables raw_in_stage_crc(const RawInTables &tb, uint32_t *s_crc) {
    for (uint32_t k = threadIdx.x; k < 256u; k += kBlock) s_crc[k] = tb.crc_byte[k];   // (the staging's barrier covers it)
    RawInTables t = tb;
    t.crc_byte = s_crc;
    return t;
}

__global__ __launch_bounds__(kBlock) void k_raw_in_size(RawInParams a, const unsigned long long *off_nl, const unsigned long long *total, uint16_t *meta,
                                                        uint32_t *block_cands) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ uint16_t s_nl[kUatVecs];
    __shared__ uint32_t s_wave[kBlock / WAVE];
    __shared__ uint32_t s_crc[256];
    const RawInTables tb = raw_in_stage_crc(a.tb, s_crc);
    const uint32_t mis = sbs_in_stage(a.text, a.nbytes, s_in, s_nl);
    uint32_t starts, own, tile_nl;
    uat_lane_lines(s_nl, mis, starts, own);
    const uint32_t nl_before = uat_block_scan((uint32_t) __popc(own), s_wave, tile_nl);
    const unsigned long long nlines = total[0], first = off_nl[blockIdx.x] + nl_before;
    uint32_t cands = 0;
    for (uint32_t rest = starts; rest; rest &= rest - 1u) {
        const uint32_t b = (uint32_t) __ffs(rest) - 1u;
        const uint32_t at = kUatChunk * threadIdx.x + b + mis + 16u;
        const uint32_t n = uat_line_len(s_nl, at);
        const unsigned long long index = first + (uint32_t) __popc(own & ((1u << b) - 1u));
        if (index >= nlines) continue;                                                  // bytes behind the last terminator: not a line
        RawInLine r;
        cands += raw_in_line(s_in + at, n, a.now_ms, a.cfg, tb, r) != MGPU_RAW_NONE;
    }
    meta[(size_t) blockIdx.x * kBlock + threadIdx.x] = (uint16_t) cands;
    uint32_t tc;
    uat_block_scan(cands, s_wave, tc);
    if (threadIdx.x == 0) block_cands[blockIdx.x] = tc;
}

__global__ __launch_bounds__(kBlock) void k_raw_in_classify(RawInParams a, const unsigned long long *off_nl, const unsigned long long *total, const uint16_t *meta,
                                                            const unsigned long long *off_cands) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kUatLds];
    __shared__ uint16_t s_nl[kUatVecs];
    __shared__ uint32_t s_wave[kBlock / WAVE];
    __shared__ uint32_t s_crc[256];
    const RawInTables tb = raw_in_stage_crc(a.tb, s_crc);
    const uint32_t mis = sbs_in_stage(a.text, a.nbytes, s_in, s_nl);
    uint32_t starts, own, tile_nl, tile_cands;
    uat_lane_lines(s_nl, mis, starts, own);
    const uint32_t nl_before = uat_block_scan((uint32_t) __popc(own), s_wave, tile_nl);
    const uint32_t mt = meta[(size_t) blockIdx.x * kBlock + threadIdx.x];
    const uint32_t cands_before = uat_block_scan(mt, s_wave, tile_cands);
    if (!mt) return;                                                                    // (behind the last barrier)
    const unsigned long long nlines = total[0], first = off_nl[blockIdx.x] + nl_before;
    unsigned long long slot = off_cands[blockIdx.x] + cands_before;
    for (uint32_t rest = starts; rest; rest &= rest - 1u) {
        const uint32_t b = (uint32_t) __ffs(rest) - 1u;
        const uint32_t at = kUatChunk * threadIdx.x + b + mis + 16u;
        const uint32_t n = uat_line_len(s_nl, at);
        const unsigned long long index = first + (uint32_t) __popc(own & ((1u << b) - 1u));
        if (index >= nlines) continue;
        RawInLine r;
        const uint32_t cls = raw_in_line(s_in + at, n, a.now_ms, a.cfg, tb, r);
        if (cls == MGPU_RAW_NONE) continue;
        if (slot < a.cand_cap) {
            a.cand_rec[slot] = r.msg;
            a.cand_sig[slot] = r.signal;
            a.cand_line[slot] = (uint32_t) index;
            a.cand_meta[slot] = (r.addr & kRawMetaAddr) | cls << kRawMetaClsShift | (uint32_t) r.msg.correctedbits << kRawMetaCorrShift | (r.adder ? kRawMetaAdder : 0u);
        }
        ++slot;
    }
}

__device__ __forceinline__ bool raw_in_bit(const uint32_t *bitmap, uint32_t addr) { return (bitmap[addr >> 5] >> (addr & 31u)) & 1u; }

// the members of a generation into its bitmap (set != 0) or out of it: the bitmaps are all zero outside a call
__global__ __launch_bounds__(kBlock) void k_raw_in_scatter(const uint32_t *members, uint32_t n, uint32_t *bitmap, int set) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const uint32_t a = members[k];
    if (a > kRawMetaAddr) return;
    if (set) atomicOr(bitmap + (a >> 5), 1u << (a & 31u)); else atomicAnd(bitmap + (a >> 5), ~(1u << (a & 31u)));
}

__global__ __launch_bounds__(kBlock) void k_raw_in_first(RawInParams a, uint32_t ncand) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= ncand) return;
    const uint32_t m = a.cand_meta[j];
    // (a value only falls during this pass: an entry read at or below j stays there, and the atomic would change nothing — with few
    // aircraft and many frames nearly every adder ends here instead of queueing on its address's word)
    if ((m & kRawMetaAdder) && a.first[m & kRawMetaAddr] > j) atomicMin(a.first + (m & kRawMetaAddr), j);
}

__device__ __forceinline__ bool raw_in_new_add(const RawInParams &a, uint32_t j, uint32_t ncand, uint32_t &addr) {
    if (j >= ncand) return false;
    const uint32_t m = a.cand_meta[j];
    addr = m & kRawMetaAddr;
    return (m & kRawMetaAdder) && a.first[addr] == j && !raw_in_bit(a.gen_active, addr);
}

__global__ __launch_bounds__(kBlock) void k_raw_in_new(RawInParams a, uint32_t ncand, uint32_t *block_new) {
    __shared__ uint32_t s_wave[kBlock / WAVE];
    uint32_t addr, tn;
    const bool is_new = raw_in_new_add(a, blockIdx.x * kBlock + threadIdx.x, ncand, addr);
    uat_block_scan(is_new, s_wave, tn);
    if (threadIdx.x == 0) block_new[blockIdx.x] = tn;
}

// misc[8]: L*, all ones before
__global__ __launch_bounds__(kBlock) void k_raw_in_mark(RawInParams a, uint32_t ncand, const unsigned long long *off_new, unsigned long long *misc) {
    __shared__ uint32_t s_wave[kBlock / WAVE];
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    uint32_t addr, tn;
    const bool is_new = raw_in_new_add(a, j, ncand, addr);
    const unsigned long long rank = off_new[blockIdx.x] + uat_block_scan(is_new, s_wave, tn);
    if (!is_new) return;
    if (rank < a.cand_cap) a.new_adds[rank] = addr;
    if (rank + 1 == a.kstar) misc[8] = j;
}

// block_cnt[k * nblocks + workgroup], k = 0..5: Mode A/C records, rejected unknown, rejected bad, accepted with 0, 1, 2 corrected bits
// (one atomic per wave and counter on the workgroup's own LDS words; no workgroup touches another's)
__global__ __launch_bounds__(kBlock) void k_raw_in_verdict(RawInParams a, uint32_t ncand, const unsigned long long *misc, uint32_t *block_acc, uint32_t *block_cnt) {
    __shared__ uint32_t s_wave[kBlock / WAVE];
    __shared__ uint32_t s_cnt[6];
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long lstar = misc[8];
    if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
    uint32_t cls = MGPU_RAW_NONE, corr = 0;
    if (j < ncand) {
        const uint32_t m = a.cand_meta[j];
        const uint32_t addr = m & kRawMetaAddr;
        cls = (m >> kRawMetaClsShift) & 7u;
        corr = (m >> kRawMetaCorrShift) & 3u;
        if (cls == MGPU_RAW_COND) {
            const bool pass = raw_in_bit(a.gen_active, addr) || (j <= lstar && raw_in_bit(a.gen_inactive, addr)) || a.first[addr] < j;
            cls = pass ? MGPU_RAW_ACCEPT : MGPU_RAW_UNKNOWN;
            a.cand_meta[j] = (m & ~(7u << kRawMetaClsShift)) | cls << kRawMetaClsShift;
        }
    }
    const bool acc = cls == MGPU_RAW_ACCEPT || cls == MGPU_RAW_MODEAC;
    uint32_t ta;
    uat_block_scan(acc, s_wave, ta);                                                     // (its barriers stand behind s_cnt's zeroes)
    if (threadIdx.x == 0) block_acc[blockIdx.x] = ta;
    const bool flag[6] = {cls == MGPU_RAW_MODEAC, cls == MGPU_RAW_UNKNOWN, cls == MGPU_RAW_BAD,
                          cls == MGPU_RAW_ACCEPT && corr == 0, cls == MGPU_RAW_ACCEPT && corr == 1, cls == MGPU_RAW_ACCEPT && corr == 2};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t n = (uint32_t) __popcll(__ballot(flag[k]));
        if (lane_id() == 0 && n) atomicAdd(s_cnt + k, n);
    }
    __syncthreads();
    if (threadIdx.x < 6) block_cnt[(size_t) threadIdx.x * gridDim.x + blockIdx.x] = s_cnt[threadIdx.x];
}

// k_text_sum for the six counters at once: workgroup k adds up block_cnt[k * nblocks ..) into misc[1 + k]; misc[0] is theirs to add
__global__ __launch_bounds__(kScanThreads) void k_raw_in_sum(const uint32_t *block_cnt, uint32_t nblocks, unsigned long long *misc) {
    __shared__ unsigned long long s_part[kScanThreads / WAVE];
    unsigned long long sum = 0;
    for (uint32_t k = threadIdx.x; k < nblocks; k += kScanThreads) sum += block_cnt[(size_t) blockIdx.x * nblocks + k];
    sum = wave_sum_u64(sum);
    if (lane_id() == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int k = 0; k < kScanThreads / WAVE; ++k) all += s_part[k];
        misc[1 + blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kBlock) void k_raw_in_write(RawInParams a, uint32_t ncand, const unsigned long long *off_acc) {
    __shared__ uint32_t s_wave[kBlock / WAVE];
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    uint32_t m = 0, cls = MGPU_RAW_NONE, ta;
    if (j < ncand) { m = a.cand_meta[j]; cls = (m >> kRawMetaClsShift) & 7u; }
    const bool acc = cls == MGPU_RAW_ACCEPT || cls == MGPU_RAW_MODEAC;
    const unsigned long long out = off_acc[blockIdx.x] + uat_block_scan(acc, s_wave, ta);
    if (j >= ncand) return;
    if (m & kRawMetaAdder) a.first[m & kRawMetaAddr] = 0xffffffffu;                      // (every adder of the address stores the same)
    const uint32_t line = a.cand_line[j];
    if (a.line_class && line < a.line_class_cap) a.line_class[line] = (uint8_t) cls;
    if (acc && out < a.msgs_cap) {
        // eight 8-byte stores: msgs is 8-byte aligned, not more
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(a.cand_rec + j);
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(a.msgs + out);
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = src[k];
        if (a.line_of) a.line_of[out] = a.line_base + line;
        if (a.signal_level) a.signal_level[out] = a.cand_sig[j];
        if (a.receiver_id) a.receiver_id[out] = a.cand_id[j];              // (the beast input)
    }
}

void launch_raw_in_scatter(const uint32_t *members, uint32_t n, uint32_t *bitmap, int set, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_raw_in_scatter, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, members, n, bitmap, set);
}

// total[0] lines, [1] bytes consumed, [2] candidates
void launch_raw_in_front(const RawInParams &a, const UatScratch &w, hipStream_t s) {
    const unsigned tiles = (unsigned) ((a.nbytes + kUatTile - 1) / kUatTile);
    uint32_t *b_nl = w.blocks, *b_last = w.blocks + w.stride, *b_cands = w.blocks + 2 * w.stride;
    unsigned long long *off_nl = w.off, *off_cands = w.off + w.stride;
    hipLaunchKernelGGL(k_sbs_in_index, dim3(tiles), dim3(kBlock), 0, s, a.text, a.nbytes, b_nl, b_last);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, b_nl, tiles, off_nl, w.total);
    hipLaunchKernelGGL(k_uat_last, dim3(1), dim3(kScanThreads), 0, s, b_last, tiles, w.total + 1);
    hipLaunchKernelGGL(k_raw_in_size, dim3(tiles), dim3(kBlock), 0, s, a, off_nl, w.total, w.meta, b_cands);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, b_cands, tiles, off_cands, w.total + 2);
    hipLaunchKernelGGL(k_raw_in_classify, dim3(tiles), dim3(kBlock), 0, s, a, off_nl, w.total, w.meta, off_cands);
}

// cb: [8 * nblocks] words, co: [2 * nblocks] offsets, nblocks = ceil(ncand / kBlock); misc[1..7) the counters (Mode A/C, rejected
// unknown, rejected bad, accepted[0..2]), misc[8] L* (all ones before), misc[9] new adds, misc[10] accepted
void launch_raw_in_resolve(const RawInParams &a, uint32_t ncand, uint32_t *cb, unsigned long long *co, unsigned long long *misc, hipStream_t s) {
    if (!ncand) return;
    const unsigned nb = (ncand + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_raw_in_first, dim3(nb), dim3(kBlock), 0, s, a, ncand);
    hipLaunchKernelGGL(k_raw_in_new, dim3(nb), dim3(kBlock), 0, s, a, ncand, cb);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, cb, nb, co, misc + 9);
    hipLaunchKernelGGL(k_raw_in_mark, dim3(nb), dim3(kBlock), 0, s, a, ncand, co, misc);
    hipLaunchKernelGGL(k_raw_in_verdict, dim3(nb), dim3(kBlock), 0, s, a, ncand, misc, cb + nb, cb + 2 * nb);
    hipLaunchKernelGGL(k_raw_in_sum, dim3(6), dim3(kScanThreads), 0, s, cb + 2 * nb, nb, misc);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, cb + nb, nb, co + nb, misc + 10);
    hipLaunchKernelGGL(k_raw_in_write, dim3(nb), dim3(kBlock), 0, s, a, ncand, co + nb);
}
