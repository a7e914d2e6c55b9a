// kernels/dump.inc — the decoded-message dump (displayModesMessage, mode_s.c:1809-2239) for records in HBM.
// Part of the single translation unit kernels.hip (included inside namespace mgpu, after text.inc, whose k_text_sum it uses, and
// beast.inc's k_beast_scan).  The formatter is dump_format.h's, the one the host compiles too.

// Lane = message, three passes like text.inc.  k_dump_size runs the formatter into the counting sink (a word per message: the dump's
// length, or the deferred mark; three words per workgroup: bytes, deferred, skipped), k_beast_scan turns the first two into offsets
// and totals, k_text_sum adds the third up, k_dump_write runs THE SAME formatter into a sink that writes memory.
// A dump is up to kDumpMax = 2599 bytes: a workgroup's dumps do not fit LDS (kBlock * kDumpMax = 650 KiB), so k_dump_write does not
// stage them as k_text_write does.  Its sink packs bytes into a 64-bit register kept aligned to the ABSOLUTE output address and
// stores each filled word with one 8-byte store; the word a dump starts in and the word it ends in belong to the neighbours too — who
// may already have written them — so those two go out as byte stores of the lane's own bytes only.  Nothing is indexed at run time
// but memory: the accumulator is one register pair shifted by a computed amount.
static_assert(kDumpMax < (1 << 16) && (uint64_t) kBlock * kDumpMax < (1ull << 31), "a wave's and a workgroup's bytes fit the scans' int");

constexpr uint32_t kDumpDeferred = 0x80000000u;     // meta of a deferred message (a dump's meta is its length)

__device__ __forceinline__ DumpIn dump_in(const DumpParams &a, uint64_t i) {
    DumpIn in;
    in.m = a.msgs + i;
    in.f = a.fields + i;
    in.pos = a.positions ? a.positions + i : nullptr;
    in.receiver_id = a.receiver_ids ? a.receiver_ids[i] : 0ull;
    in.decoded_rc = a.decoded_rc ? a.decoded_rc[i] : 0u;
    in.reduce_forward = a.reduce_forward ? a.reduce_forward[i] : (uint8_t) 0;
    in.decoded_nic = a.decoded_nic ? a.decoded_nic[i] : (uint8_t) 0;
    return in;
}

struct DumpPackSink {
    uint64_t acc;               // the bytes of the word being filled, each at its place
    uintptr_t at;               // the address of the next byte
    uintptr_t first, limit;     // the dump's first byte; out + cap: no byte below the one, at or beyond the other is stored
    __device__ __forceinline__ void put(uint32_t c) {
        acc |= (uint64_t) (c & 0xffu) << (8u * (uint32_t) (at & 7u));
        ++at;
        if ((at & 7u) == 0) flush();
    }
    __device__ __forceinline__ void lit(const char *p, uint32_t n) {
        for (uint32_t k = 0; k < n; ++k) put((uint8_t) p[k]);
    }
    // the word that holds byte at - 1: whole if all eight bytes are this dump's and below the limit, else the lane's own bytes one by one
    __device__ __forceinline__ void flush() {
        const uintptr_t w = (at - 1) & ~(uintptr_t) 7;
        const uintptr_t lo = w > first ? w : first, hi = at < limit ? at : limit;
        if (lo == w && hi == w + 8) *reinterpret_cast<uint64_t *>(w) = acc;
        else
            for (uintptr_t b = lo; b < hi; ++b) *reinterpret_cast<uint8_t *>(b) = (uint8_t) (acc >> (8u * (uint32_t) (b - w)));
        acc = 0;
    }
    __device__ __forceinline__ void finish() { if (at & 7u) flush(); }
};

__global__ __launch_bounds__(kBlock) void k_dump_size(DumpParams a, uint64_t n, uint32_t *meta, uint32_t *block_bytes, uint32_t *block_def, uint32_t *block_skip) {
    __shared__ uint32_t s_sum[kBlock / WAVE], s_def[kBlock / WAVE], s_skip[kBlock / WAVE];
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    uint32_t l = 0;
    int cls = DUMP_NONE;
    if (i < n) {
        const DumpIn in = dump_in(a, i);
        cls = dump_classify(in, a.flags, a.show_only, false);
        if (cls == DUMP_LINE) {
            DumpCountSink s = {0};
            dump_format(in, a.flags, false, s);
            l = s.n;
        }
        meta[i] = cls == DUMP_DEFER ? kDumpDeferred : l;
    }
    const uint32_t w = (uint32_t) wave_sum_u64(l);
    const uint32_t wd = (uint32_t) __popcll(__ballot(cls == DUMP_DEFER)), ws = (uint32_t) __popcll(__ballot(cls == DUMP_SKIP));
    if (lane_id() == 0) { s_sum[threadIdx.x >> 6] = w; s_def[threadIdx.x >> 6] = wd; s_skip[threadIdx.x >> 6] = ws; }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_bytes[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        block_def[blockIdx.x] = s_def[0] + s_def[1] + s_def[2] + s_def[3];
        block_skip[blockIdx.x] = s_skip[0] + s_skip[1] + s_skip[2] + s_skip[3];
    }
}

__global__ __launch_bounds__(kBlock) void k_dump_write(DumpParams a, uint64_t n, const uint32_t *meta, const unsigned long long *block_off, uint8_t *out, uint64_t cap,
                                                       const unsigned long long *block_def_off, mgpu_deferred *deferred, uint64_t def_cap) {
    __shared__ uint32_t s_wave[kBlock / WAVE], s_wdef[kBlock / WAVE];
    const uint32_t wv = threadIdx.x >> 6;
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    const uint32_t mt = i < n ? meta[i] : 0u;
    const bool is_def = mt == kDumpDeferred;
    const uint32_t l = is_def ? 0u : mt;
    const uint64_t dm = __ballot(is_def);
    int wtotal;
    const int ex = wave_excl_scan((int) l, wtotal);
    if (lane_id() == 0) { s_wave[wv] = (uint32_t) wtotal; s_wdef[wv] = (uint32_t) __popcll(dm); }
    __syncthreads();
    unsigned long long start = block_off[blockIdx.x] + (uint32_t) ex;
    for (uint32_t k = 0; k < wv; ++k) start += s_wave[k];
    if (is_def) {                                             // where the dump would start, were it written
        uint32_t rank = (uint32_t) __popcll(dm & ((1ull << lane_id()) - 1));
        for (uint32_t k = 0; k < wv; ++k) rank += s_wdef[k];
        const unsigned long long slot = block_def_off[blockIdx.x] + rank;
        if (slot < def_cap) { mgpu_deferred e; e.index = i; e.offset = start; deferred[slot] = e; }
    }
    if (l && start < cap) {                                   // (the capacity may cut this dump: the bytes below it only)
        DumpPackSink s;
        s.acc = 0;
        s.first = reinterpret_cast<uintptr_t>(out) + start;
        s.at = s.first;
        s.limit = reinterpret_cast<uintptr_t>(out) + cap;
        dump_format(dump_in(a, i), a.flags, false, s);
        s.finish();
    }
}

// w.blocks: three runs of `stride` entries each (bytes, deferred, skipped), w.off: the first two's offsets; w.total[3]: bytes, deferred, skipped
void launch_dump_encode(const DumpParams &a, uint64_t n, const DumpScratch &w, uint8_t *out, uint64_t cap, mgpu_deferred *deferred, uint64_t def_cap, hipStream_t s) {
    if (n == 0) return;
    const unsigned blocks = (unsigned) ((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_dump_size, dim3(blocks), dim3(kBlock), 0, s, a, n, w.meta, w.blocks, w.blocks + w.stride, w.blocks + 2 * w.stride);
    for (int k = 0; k < 2; ++k)
        hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, w.blocks + k * w.stride, blocks, w.off + k * w.stride, w.total + k);
    hipLaunchKernelGGL(k_text_sum, dim3(1), dim3(kScanThreads), 0, s, w.blocks + 2 * w.stride, blocks, w.total + 2);
    hipLaunchKernelGGL(k_dump_write, dim3(blocks), dim3(kBlock), 0, s, a, n, w.meta, w.off, out, cap, w.off + w.stride, deferred, def_cap);
}
