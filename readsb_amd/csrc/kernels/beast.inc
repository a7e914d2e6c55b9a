// kernels/beast.inc — beast wire encoder (modesSendBeastOutput, net_io.c:1655-1714) for message records in HBM.
// Part of the single translation unit kernels.hip (included inside namespace mgpu, after the parts before it).

// One frame per message: 0x1a, type '2' (7 bytes) / '3' (14) / '1' (Mode A/C, 2), the 12 MHz timestamp as 6 bytes
// big-endian (netTimestamp, :1620-1648), one byte of signal level (:1696-1700), the message bytes; every 0x1a
// payload byte doubled.  With per-message receiver ids (--net-receiver-id, :1667-1680) a frame whose id differs from the id of the
// message modesSendBeastOutput was last called for is preceded by 0x1a 0xe3 and the id as 8 bytes big-endian, 0x1a doubled: below.
// Lane = message.  k_beast_size sizes the frames (a byte per message, a word per workgroup), k_beast_scan turns the
// workgroup sizes into offsets (one workgroup, no atomics), k_beast_write assembles a workgroup's frames in LDS at the
// alignment they will have in memory and copies them out as whole words.

// Pass 1 also keeps the signal byte (one double sqrt per message) for pass 2: meta = length | signal << 8.

__device__ __forceinline__ uint32_t beast_signal(const mgpu_msg &m) {
#pragma clang fp contract(off)
    // mm->signalLevel = sum(mag^2) / 65535 / 65535 / samples (demod_2400.c:447-448), then sqrt * 255, round half to even
    const double level = (double) m.sig_sumsq / 65535.0 / 65535.0 / (double) m.sig_len;
    int sig = (int) rint(__dsqrt_rn(level) * 255.0);
    if (level > 0 && sig < 1) sig = 1;
    if (sig > 255) sig = 255;
    return (uint32_t) sig;
}

__device__ __forceinline__ uint32_t beast_type(uint32_t msg_len) {
    return msg_len == 7 ? '2' : msg_len == 14 ? '3' : msg_len == 2 ? '1' : 0;   // 0: the format does not carry it (:1687)
}

// payload byte k (0..20): timestamp 6, signal 1, message bytes (VERB: as sliced, mm->verbatim, :1662)
template <bool VERB = false>
__device__ __forceinline__ uint32_t beast_byte(const mgpu_msg &m, uint32_t sig, int k) {
    return k < 6 ? (uint32_t) ((uint64_t) m.timestamp >> (40 - 8 * k)) & 0xffu : k == 6 ? sig : VERB ? m.raw[k - 7] : m.msg[k - 7];
}

// Variants of the two kernels (template parameter): the plain instances are the code they were before the variants existed.
enum : int { BEAST_IDS = 1, BEAST_VERBATIM = 2 };
// BEAST_VERBATIM (--net-verbatim): raw[] for msg[], and every carried message gets a frame: outputMessage's first-message rule and its
// correctedbits < 2 test both have `|| Modes.net_verbatim` (net_io.c:5846, 5869), so the verdicts decide nothing and nothing is deferred.
// BEAST_IDS: `ids` = one receiver id per message.  A message is a CALLER when the reference would call modesSendBeastOutput for it (a
// frame is due by flags and verdicts, whatever its length); the prefix goes before a caller's frame iff its id differs from the caller's
// before it (writer->lastReceiverId, :1669-1670).  A caller of a length the format does not carry writes nothing — the return at :1690
// skips completeWrite — but has moved lastReceiverId already.  The previous caller of a workgroup's FIRST caller is in another workgroup:
// k_beast_size leaves {has a caller, first caller: thread, id, carried; last caller's id} per workgroup, k_beast_idscan carries the id
// through them (workgroups without a caller pass it on) and adds the first callers' prefixes: a word {1 << 31 | length << 16 | thread}
// per workgroup for k_beast_write, and the bytes on the workgroup's sum.  meta of a caller: bit 6 = prefix (known inside the workgroup),
// length (<= 62) in bits 0-5.
constexpr uint32_t kBeastPrefix = 0x40, kBeastLenMask = 0x3f;
constexpr int kBeastFrameMax = 44, kBeastFrameMaxIds = 62;
struct BeastIdScratch {             // per workgroup; null pointers without ids
    unsigned long long *first_id, *last_id;
    uint32_t *info;                 // bit 0: has a caller, bit 1: its first caller's length is carried, bits 8-: that caller's thread
    uint32_t *fix;                  // k_beast_idscan's word for k_beast_write
};
__device__ __forceinline__ uint32_t beast_prefix_len(unsigned long long id) {
    uint32_t l = 10;
#pragma unroll
    for (int k = 0; k < 8; ++k) l += ((id >> (8 * k)) & 0xffull) == 0x1aull ? 1u : 0u;
    return l;
}

// The gated form (mgpu_beast_encode_gated*, SURVEY.md §8(f).4): `verdict` = the tracking gate's byte per message (kernels/gate.inc).
// A frame is produced for the messages the reference forwards FOR CERTAIN (outputMessage, net_io.c:5846-5849; with net_rule also its
// correctedbits < 2 test for the beast / raw network outputs, :5863-5872 — the --dump-beast file has none); a message whose fate is
// the position tracker's (MGPU_GATE_DEFER) gets no frame but an entry {its index, the stream offset its frame would go to} in a list
// in stream order: the host's tracker settles those few and splices their frames in.  meta of a deferred message: length 0, signal 1.
constexpr uint16_t kBeastDeferred = 0x0100;

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_beast_size(const mgpu_msg *msgs, uint64_t n, uint16_t *meta, uint32_t *block_bytes,
                                                       const uint8_t *verdict, int net_rule, uint32_t *block_def,
                                                       const unsigned long long *ids, BeastIdScratch idw) {
    constexpr bool VERB = (MODE & BEAST_VERBATIM) != 0, IDS = (MODE & BEAST_IDS) != 0;
    __shared__ uint32_t s_sum[kBlock / WAVE], s_def[kBlock / WAVE];
    __shared__ unsigned long long s_wlast[IDS ? kBlock / WAVE : 1];
    __shared__ uint32_t s_whas[IDS ? kBlock / WAVE : 1];
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    uint32_t l = 0;
    bool deferred = false, caller = false;
    if (i < n) {
        const mgpu_msg m = msgs[i];
        const uint32_t msg_len = m.msgbits / 8u;
        uint32_t sig = 0;
        bool keep = true;
        if (!VERB && verdict) {
            const uint32_t v = verdict[i] & 3u;
            const bool wire_ok = !net_rule || m.correctedbits < 2;
            keep = v == 1u && wire_ok;
            deferred = v == 2u && wire_ok && beast_type(msg_len) != 0;
        }
        if (keep && beast_type(msg_len)) {
            sig = beast_signal(m);
            l = 2 + 7 + msg_len;
#pragma unroll
            for (int k = 0; k < 21; ++k) l += (k < 7 + (int) msg_len && beast_byte<VERB>(m, sig, k) == 0x1a) ? 1u : 0u;
        }
        caller = keep;
        if (!IDS) meta[i] = deferred ? kBeastDeferred : (uint16_t) (l | (sig << 8));
        else l |= sig << 8;
    }
    if (IDS) {
        // the caller before this one: in the wave (a ballot and a shuffle), else the last caller of an earlier wave, else another workgroup's
        const int lane = lane_id(), wv = threadIdx.x >> 6;
        const unsigned long long id = caller ? ids[i] : 0ull;
        const uint64_t cm = __ballot(caller), below = cm & ((1ull << lane) - 1);
        unsigned long long prev = __shfl(id, below ? 63 - __builtin_clzll(below) : 0);
        bool have = below != 0;
        if (cm && lane == 63 - __builtin_clzll(cm)) s_wlast[wv] = id;
        if (lane == 0) s_whas[wv] = cm != 0;
        __syncthreads();
        for (int k = wv - 1; k >= 0 && !have; --k)
            if (s_whas[k]) { prev = s_wlast[k]; have = true; }
        const uint32_t sig8 = l & 0xff00u;
        l &= 0xffu;
        if (caller && l && have && id != prev) l = (l + beast_prefix_len(id)) | kBeastPrefix;
        if (caller && !have) {                                   // the workgroup's first caller: one thread
            idw.first_id[blockIdx.x] = id;
            idw.info[blockIdx.x] = 1u | (l ? 2u : 0u) | ((uint32_t) threadIdx.x << 8);
        }
        if (threadIdx.x == 0) {
            int last = -1;
            for (int k = 0; k < kBlock / WAVE; ++k) if (s_whas[k]) last = k;
            if (last >= 0) idw.last_id[blockIdx.x] = s_wlast[last];
            else idw.info[blockIdx.x] = 0;
        }
        if (i < n) meta[i] = deferred ? kBeastDeferred : (uint16_t) (l | sig8);
        l &= kBeastLenMask;
    }
    const uint32_t w = (uint32_t) wave_sum_u64(l);
    const uint32_t wd = (uint32_t) __popcll(__ballot(deferred));
    if (lane_id() == 0) { s_sum[threadIdx.x >> 6] = w; s_def[threadIdx.x >> 6] = wd; }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_bytes[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        if (block_def) block_def[blockIdx.x] = s_def[0] + s_def[1] + s_def[2] + s_def[3];
    }
}

// Exclusive prefix over the workgroups' byte counts: one workgroup, every thread a contiguous run of entries.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_beast_scan(const uint32_t *block_bytes, uint32_t nblocks, unsigned long long *block_off,
                                                             unsigned long long *total) {
    __shared__ unsigned long long s_part[kScanThreads];
    const uint32_t per = (nblocks + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = threadIdx.x * per, hi = lo + per < nblocks ? lo + per : nblocks;
    unsigned long long sum = 0;
    for (uint32_t k = lo; k < hi; ++k) sum += block_bytes[k];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {           // Hillis-Steele over 1024 partial sums
        const unsigned long long add = (int) threadIdx.x >= d ? s_part[threadIdx.x - d] : 0ull;
        __syncthreads();
        s_part[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned long long run = s_part[threadIdx.x] - sum;
    for (uint32_t k = lo; k < hi; ++k) { block_off[k] = run; run += block_bytes[k]; }
    if (threadIdx.x == kScanThreads - 1) *total = s_part[kScanThreads - 1];
}

// BEAST_IDS: the id of the last caller before every workgroup — an inclusive scan of {has a caller, last caller's id} under "the right
// operand wins if it has one", seeded with the writer's lastReceiverId — and with it the prefix of every workgroup's first caller.
__global__ __launch_bounds__(kScanThreads) void k_beast_idscan(BeastIdScratch idw, uint32_t nblocks, uint32_t *block_bytes, unsigned long long last_in,
                                                               unsigned long long *last_out) {
    __shared__ unsigned long long s_id[kScanThreads];
    __shared__ uint32_t s_has[kScanThreads];
    const uint32_t per = (nblocks + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = threadIdx.x * per < nblocks ? threadIdx.x * per : nblocks, hi = lo + per < nblocks ? lo + per : nblocks;
    unsigned long long id = 0;
    uint32_t has = 0;
    for (uint32_t k = lo; k < hi; ++k)
        if (idw.info[k] & 1u) { id = idw.last_id[k]; has = 1; }
    s_id[threadIdx.x] = id; s_has[threadIdx.x] = has;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const bool take = (int) threadIdx.x >= d && !has;
        const unsigned long long oid = take ? s_id[threadIdx.x - d] : 0ull;
        const uint32_t ohas = take ? s_has[threadIdx.x - d] : 0u;
        __syncthreads();
        if (take && ohas) { id = oid; has = 1; s_id[threadIdx.x] = id; s_has[threadIdx.x] = 1; }
        __syncthreads();
    }
    unsigned long long cur = threadIdx.x && s_has[threadIdx.x - 1] ? s_id[threadIdx.x - 1] : last_in;
    for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t info = idw.info[k];
        uint32_t fix = 0;
        if (info & 1u) {
            const unsigned long long first = idw.first_id[k];
            if ((info & 2u) && first != cur) {
                const uint32_t pl = beast_prefix_len(first);
                fix = (1u << 31) | (pl << 16) | (info >> 8);
                block_bytes[k] += pl;
            }
            cur = idw.last_id[k];
        }
        idw.fix[k] = fix;
    }
    if (threadIdx.x == kScanThreads - 1) *last_out = cur;
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_beast_write(const mgpu_msg *msgs, uint64_t n, const uint16_t *meta, const unsigned long long *block_off,
                                                        uint8_t *out, uint64_t cap, const unsigned long long *block_def_off, mgpu_deferred *deferred,
                                                        uint64_t def_cap, const unsigned long long *ids, const uint32_t *id_fix) {
    constexpr bool VERB = (MODE & BEAST_VERBATIM) != 0, IDS = (MODE & BEAST_IDS) != 0;
    __shared__ uint32_t s_wave[kBlock / WAVE], s_wdef[kBlock / WAVE];
    __shared__ __attribute__((aligned(16))) uint8_t s_bytes[kBlock * (IDS ? kBeastFrameMaxIds : kBeastFrameMax) + 8];
    const uint32_t wv = threadIdx.x >> 6;
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    const uint32_t mt = i < n ? meta[i] : 0u;
    uint32_t l = mt & (IDS ? kBeastLenMask : 0xffu);
    bool prefix = IDS && (mt & kBeastPrefix);
    if (IDS) {                                                // the workgroup's first caller: k_beast_idscan decided
        const uint32_t fix = id_fix[blockIdx.x];
        if ((fix >> 31) && (fix & 0xffffu) == threadIdx.x) { l += (fix >> 16) & 0xffu; prefix = true; }
    }
    const bool is_def = deferred && mt == kBeastDeferred;
    const uint64_t dm = __ballot(is_def);
    int wtotal;
    const int ex = wave_excl_scan((int) l, wtotal);
    if (lane_id() == 0) { s_wave[wv] = (uint32_t) wtotal; s_wdef[wv] = (uint32_t) __popcll(dm); }
    __syncthreads();
    const unsigned long long base = block_off[blockIdx.x];
    // frames are laid out in LDS at the same alignment (mod 4) they will have in memory, so the copy below moves whole words
    const uint32_t mis = (uint32_t) ((reinterpret_cast<uintptr_t>(out) + base) & 3u);
    uint32_t off = mis + (uint32_t) ex;
    for (uint32_t k = 0; k < wv; ++k) off += s_wave[k];
    const uint32_t block_total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (is_def) {                                             // where the frame would start, were it forwarded
        uint32_t rank = (uint32_t) __popcll(dm & ((1ull << lane_id()) - 1));
        for (uint32_t k = 0; k < wv; ++k) rank += s_wdef[k];
        const unsigned long long slot = block_def_off[blockIdx.x] + rank;
        if (slot < def_cap) { mgpu_deferred e; e.index = i; e.offset = base + (off - mis); deferred[slot] = e; }
    }
    if (l) {
        const mgpu_msg m = msgs[i];
        const uint32_t msg_len = m.msgbits / 8u, sig = mt >> 8;
        uint8_t *p = s_bytes + off;
        if (IDS && prefix) {
            const unsigned long long id = ids[i];
            *p++ = 0x1a;
            *p++ = 0xe3;
#pragma unroll
            for (int k = 7; k >= 0; --k) {
                const uint8_t b = (uint8_t) (id >> (8 * k));
                *p++ = b;
                if (b == 0x1a) *p++ = 0x1a;
            }
        }
        *p++ = 0x1a;
        *p++ = (uint8_t) beast_type(msg_len);
#pragma unroll
        for (int k = 0; k < 21; ++k) {
            if (k < 7 + (int) msg_len) {
                const uint32_t b = beast_byte<VERB>(m, sig, k);
                *p++ = (uint8_t) b;
                if (b == 0x1a) *p++ = 0x1a;
            }
        }
    }
    __syncthreads();
    const uint32_t lo = mis, hi = mis + block_total;
    uint8_t *dst = out + base - mis;                          // dst[k] <-> s_bytes[k]; dst is 4-byte aligned
    if (base + block_total <= cap) {
        const uint32_t wlo = (lo + 3u) & ~3u, whi = hi & ~3u;
        if (whi > wlo) {
            const uint32_t *src32 = reinterpret_cast<const uint32_t *>(s_bytes);
            uint32_t *dst32 = reinterpret_cast<uint32_t *>(dst);
            for (uint32_t w = wlo / 4 + threadIdx.x; w < whi / 4; w += kBlock) dst32[w] = src32[w];
            if (threadIdx.x < 3) {                                 // at most three bytes before and after the word run
                const uint32_t h = lo + threadIdx.x, t = whi + threadIdx.x;
                if (h < wlo) dst[h] = s_bytes[h];
                if (t < hi) dst[t] = s_bytes[t];
            }
        } else {
            for (uint32_t k = lo + threadIdx.x; k < hi; k += kBlock) dst[k] = s_bytes[k];
        }
    } else {
        for (uint32_t k = lo + threadIdx.x; k < hi; k += kBlock)
            if (base + (k - mis) < cap) dst[k] = s_bytes[k];
    }
}

// verdict == nullptr: every message's frame (mgpu_beast_encode*).  Gated: block_def / block_def_off [blocks] are scratch, total[1]
// receives the number of deferred messages (all of them counted, the first def_cap listed).  ids: idw's arrays [blocks] are scratch,
// total[2] receives the last caller's id (last_id if there was none).  verbatim: verdict and net_rule decide nothing
template <int MODE>
static void launch_beast_mode(const mgpu_msg *msgs, uint64_t n, uint16_t *meta, uint32_t *block_bytes, unsigned long long *block_off, uint8_t *out,
                              uint64_t cap, unsigned long long *total, hipStream_t s, const uint8_t *verdict, int net_rule, uint32_t *block_def,
                              unsigned long long *block_def_off, mgpu_deferred *deferred, uint64_t def_cap, const unsigned long long *ids,
                              unsigned long long last_id, const BeastIdScratch &idw) {
    const unsigned blocks = (unsigned) ((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_beast_size<MODE>, dim3(blocks), dim3(kBlock), 0, s, msgs, n, meta, block_bytes, verdict, net_rule, verdict ? block_def : nullptr, ids, idw);
    if (MODE & BEAST_IDS) hipLaunchKernelGGL(k_beast_idscan, dim3(1), dim3(kScanThreads), 0, s, idw, blocks, block_bytes, last_id, total + 2);
    hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, block_bytes, blocks, block_off, total);
    if (verdict) hipLaunchKernelGGL(k_beast_scan, dim3(1), dim3(kScanThreads), 0, s, block_def, blocks, block_def_off, total + 1);
    hipLaunchKernelGGL(k_beast_write<MODE>, dim3(blocks), dim3(kBlock), 0, s, msgs, n, meta, block_off, out, cap, block_def_off, verdict ? deferred : nullptr, def_cap,
                       ids, idw.fix);
}

void launch_beast_encode(const mgpu_msg *msgs, uint64_t n, uint16_t *meta, uint32_t *block_bytes, unsigned long long *block_off, uint8_t *out,
                         uint64_t cap, unsigned long long *total, hipStream_t s, const uint8_t *verdict, int net_rule, uint32_t *block_def,
                         unsigned long long *block_def_off, mgpu_deferred *deferred, uint64_t def_cap, int verbatim, const unsigned long long *ids,
                         unsigned long long last_id, void *id_scratch) {
    if (n == 0) return;
    const size_t blocks = (size_t) ((n + kBlock - 1) / kBlock);
    BeastIdScratch idw = {nullptr, nullptr, nullptr, nullptr};
    if (ids) {
        idw.first_id = (unsigned long long *) id_scratch; idw.last_id = idw.first_id + blocks;
        idw.info = (uint32_t *) (idw.last_id + blocks); idw.fix = idw.info + blocks;
    }
    if (verbatim) verdict = nullptr;
#define BEAST_GO(MODE) launch_beast_mode<MODE>(msgs, n, meta, block_bytes, block_off, out, cap, total, s, verdict, net_rule, block_def, block_def_off, deferred, def_cap, ids, last_id, idw)
    if (ids) { if (verbatim) BEAST_GO(BEAST_IDS | BEAST_VERBATIM); else BEAST_GO(BEAST_IDS); }
    else { if (verbatim) BEAST_GO(BEAST_VERBATIM); else BEAST_GO(0); }
#undef BEAST_GO
}
size_t beast_id_scratch_bytes(uint64_t n) { return (size_t) ((n + kBlock - 1) / kBlock + 1) * 24; }
