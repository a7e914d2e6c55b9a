// shard.cpp — the shard protocol of the C ABI (include/modes_gpu.h: mgpu_shard_*, BASELINE config 5).
#include "ctx.h"

extern "C" {

// ---- one capture sharded by buffer ranges over several contexts / GPUs (BASELINE config 5) ------------------
// Buffers are independent except for the ICAO filter, and the pre-screen needs the adder addresses of the WHOLE
// capture (a frame is only "conditional" with respect to adds that may lie in an earlier shard).  So a shard runs
// twice: pass 1 (mode 1) sweeps it for its adder bitmap; the bitmaps are OR-ed across shards (the exchange step:
// 2 MiB per rank); pass 2 (mode 2) runs convert, sweep and pre-screen against the global bitmap and keeps every
// chunk's live records as a packet.  The packets of all shards, in stream order, go through mgpu_walk_packets on
// one context: the ordered walk and the message build, exactly as for an unsharded stream.

// A context that starts (or continues) in the middle of a capture: its sample clock, and the 326 magnitudes that precede the first
// sample (sdr_ifile.c:209-213) from the 326 IQ samples before it.
static int start_mid_stream(mgpu_ctx *c, uint64_t first_sample, const void *history_iq) {
    c->stream_pos = first_sample;
    c->eof = false;
    c->tail_src = nullptr;
    if (first_sample) {
        const size_t bps = c->cfg.format == MGPU_FMT_UC8 ? 2 : 4;
        if (!c->d_hist) {
            HIPCHK(c, hipMalloc(&c->d_hist, (2 * kTrailing + 64) * sizeof(uint16_t)));
            HIPCHK(c, hipMalloc(&c->d_hist_iq, kTrailing * 4 + 64));
            HIPCHK(c, hipMalloc(&c->d_hist_sums, 8 * sizeof(unsigned long long)));
        }
        hipStream_t s = c->stream;
        HIPCHK(c, hipMemcpyAsync(c->d_hist_iq, history_iq, kTrailing * bps, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(c->d_hist_sums, 0, 8 * sizeof(unsigned long long), s));
        ConvertParams cp{};
        cp.iq = c->d_hist_iq; cp.mag = c->d_hist; cp.n = kTrailing; cp.buf_samples = 0x80000000u;
        cp.uc8_folded = c->d_uc8_folded;
        cp.sum_level = c->d_hist_sums; cp.sum_power = c->d_hist_sums + 1;
        cp.fsum_level = (double *) (c->d_hist_sums + 2); cp.fsum_power = (double *) (c->d_hist_sums + 3);
        launch_convert(c->cfg.format, cp, s);
        HIPCHK(c, hipStreamSynchronize(s));
        c->tail_src = c->d_hist + kTrailing;   // d_hist[326 + i] = magnitude of history sample i
    }
    return MGPU_OK;
}

int mgpu_shard_begin(mgpu_ctx *c, uint64_t first_sample, const void *history_iq, int mode) {
    if (!c || mode < 1 || mode > 3 || first_sample % c->cfg.buf_samples || c->deferred) return MGPU_E_INVAL;
    if (first_sample && !history_iq) return MGPU_E_INVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->shard_mode = mode;
    if (mode == 2)                           // the packets carry every live record's would-be skip-window counts
        for (auto &sl : c->slot)
            if (!sl.d_live_win) {
                HIPCHK(c, hipMalloc(&sl.d_live_win, c->cap_pool * sizeof(unsigned long long)));
                HIPCHK(c, hipHostMalloc(&sl.h_live_win, c->cap_pool * sizeof(unsigned long long)));
            }
    c->shard_packets.clear();
    c->shard_est.clear(); c->shard_est_pos.clear(); c->shard_est_off.clear();
    { const int rc = start_mid_stream(c, first_sample, history_iq); if (rc != MGPU_OK) return rc; }
    return MGPU_OK;
}

int mgpu_adder_bitmap_get(mgpu_ctx *c, uint32_t *words) {
    if (!c || !words) return MGPU_E_INVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpy(words, c->d_adder_bitmap, (1u << 24) / 8, hipMemcpyDeviceToHost));
    return MGPU_OK;
}

int mgpu_adder_bitmap_set(mgpu_ctx *c, const uint32_t *words) {
    if (!c || !words) return MGPU_E_INVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpy(c->d_adder_bitmap, words, (1u << 24) / 8, hipMemcpyHostToDevice));
    return MGPU_OK;
}

int mgpu_shard_packets(mgpu_ctx *c, const void **packets, uint64_t *bytes) {
    if (!c || !packets || !bytes) return MGPU_E_INVAL;
    *packets = c->shard_packets.data();
    *bytes = c->shard_packets.size();
    return MGPU_OK;
}

// One packet = one chunk of some rank's range, as fetcher_main lays it out.
struct PacketView {
    uint64_t pos = 0, n = 0, nrecs = 0, nbuf = 0;
    uint64_t hdr[kPacketWords] = {};
    const PhaseRec *recs = nullptr;                            // nrecs records + the walk's sentinel
    const unsigned long long *sig = nullptr, *win = nullptr;    // per record: its would-be signal power, the counts of its would-be skip window
    const unsigned long long *sums = nullptr;                   // level[nbuf], power[nbuf]: integers (UC8) or doubles, eight bytes each
};

// The packets may come from other ranks over a gather: nothing in a header is trusted before it is checked against the bytes
// that are really there (record count without a 64-bit overflow) and the context's capacity; `check_records`: the order the walk
// relies on, record by record (a rank's own packets, made by this library in this process, are taken as they are).
static int parse_packet(mgpu_ctx *c, const uint8_t *&p, const uint8_t *end, PacketView &v, bool check_records) {
    constexpr uint64_t kRecBytes = sizeof(PhaseRec) + 16;       // record + its signal power + its window counts
    if ((size_t) (end - p) < sizeof(v.hdr)) { c->err = "shard packets: truncated packet header"; return MGPU_E_INVAL; }
    std::memcpy(v.hdr, p, sizeof(v.hdr));
    p += sizeof(v.hdr);
    v.pos = v.hdr[0]; v.n = v.hdr[1]; v.nrecs = v.hdr[2]; v.nbuf = v.hdr[10];
    if (v.hdr[3] != kPacketMagic || v.n == 0 || v.n > c->cap_samples || v.n > 0xFFFFFFF0ull ||
        v.nbuf != (v.n + c->cfg.buf_samples - 1) / c->cfg.buf_samples || (uint64_t) (end - p) < sizeof(PhaseRec) ||
        v.nrecs > ((uint64_t) (end - p) - sizeof(PhaseRec)) / kRecBytes ||
        (uint64_t) (end - p) - sizeof(PhaseRec) - v.nrecs * kRecBytes < v.nbuf * 16) {
        c->err = "shard packets: a packet must lie within max_samples, with all its records present";
        return MGPU_E_INVAL;
    }
    // the records are walked where they lie (packets are 8-byte aligned and a sentinel record follows the last one)
    v.recs = (const PhaseRec *) p;
    p += (v.nrecs + 1) * sizeof(PhaseRec);
    v.sig = (const unsigned long long *) p;
    p += v.nrecs * 8;
    v.win = (const unsigned long long *) p;
    p += v.nrecs * 8;
    v.sums = (const unsigned long long *) p;
    p += v.nbuf * 16;
    if (v.recs[v.nrecs].pos != 0xFFFFFFFFu) { c->err = "shard packets: malformed record list"; return MGPU_E_INVAL; }
    if (check_records)
        for (uint64_t i = 0; i < v.nrecs; ++i) {                 // sorted by position, inside the packet's samples, a real phase
            const PhaseRec &r = v.recs[i];
            if (r.pos >= v.n || (i && r.pos < v.recs[i - 1].pos) || r.phase < 4 || r.phase > 8) {
                c->err = "shard packets: malformed record list";
                return MGPU_E_INVAL;
            }
        }
    return MGPU_OK;
}

// A packet's ordered walk (the walker's team, as for a chunk of an unsharded stream); build: its messages appended to
// c->pending and every statistic an unsharded run keeps — the sweep-side tallies and the per-buffer sums ride in the packet,
// what the accepted frames' skip windows hide is the sum of the accepted records' window counts; noise_terms (when given): what
// each buffer adds to noise_power_sum, in order (a double sum is order-dependent: the rank that combines ranges re-adds them).
static int walk_one_packet(mgpu_ctx *c, const PacketView &v, bool build, std::vector<double> *noise_terms) {
    HostJob &job = c->job[0];
    mgpu_counters &k = c->counters;
    const uint64_t nrecs = v.nrecs, nbuf = v.nbuf, n = v.n;
    const PhaseRec *recs = v.recs;
    const unsigned long long *sig = v.sig, *win = v.win, *sums = v.sums;
    ifile_grid(c, v.pos, n, job.buffers);
    const uint64_t cap = nrecs + 1;
    job.pos.resize(cap); c->w_limit.resize(cap); c->w_skip.resize(cap);
    job.rc = ResolveCounts();
    const double t0 = wall_ms();
    const int64_t wn = host_walk(c, job, recs, job.buffers, nrecs, cap);
    c->acc.resolve_ms += (float) (wall_ms() - t0);
    if (wn < 0) return MGPU_E_OVERFLOW;
    if (!build) return MGPU_OK;
    const double t1 = wall_ms();
    const size_t first = c->pending.size();
    if (!c->pending.grow_for((size_t) wn)) return c->pending.external ? MGPU_E_OVERFLOW : MGPU_E_NOMEM;
    {
        mgpu_msg *dst = c->pending.data() + first;
        const int parts = wn >= 4096 ? c->build_threads : 1;
        c->build_team.run(parts, [&](int i) {
            const uint64_t lo = (uint64_t) wn * i / parts, hi = (uint64_t) wn * (i + 1) / parts;
            Resolver::build_messages(recs, sig, nullptr, job.buffers, job.acc.data() + lo, hi - lo, dst + lo);
        });
    }
    c->pending.n = first + (size_t) wn;
    // ---- the statistics: feed_end's and build_job's, from what the packet carries ----
    const ResolveCounts &rc = job.rc;
    for (int i = 0; i < 3; ++i) k.demod_accepted[i] += rc.accepted[i];
    for (int i = 0; i < 5; ++i) k.demod_bestPhase[i] += rc.best_phase[i];
    uint64_t hw[5] = {0, 0, 0, 0, 0};                        // what the accepted frames' skip windows hide: candidates, phases 4/5, 6/7, 8, conditional-only
    std::vector<uint64_t> buf_scaled(nbuf, 0);
    for (int64_t i = 0; i < wn; ++i) {
        const Accepted &a = job.acc[(size_t) i];
        const unsigned long long w = win[a.rec];
        hw[0] += w & 0xff; hw[1] += (w >> 8) & 0xff; hw[2] += (w >> 16) & 0xff; hw[3] += (w >> 24) & 0xff; hw[4] += (w >> 32) & 0xff;
        const unsigned long long sumsq = sig[a.rec];
        const unsigned sig_len = (recs[a.rec].msg[0] & 0x80) ? 268u : 134u;    // msglen * 12 / 5, demod_2400.c:439
        const double signal_power = (double) sumsq / 65535.0 / 65535.0, level = signal_power / sig_len;
        k.signal_power_sum += signal_power;
        k.signal_power_count += sig_len;
        if (level > k.peak_signal_power) k.peak_signal_power = level;
        if (level > 0.50119) k.strong_signal_count++;
        if (a.buffer < nbuf) buf_scaled[a.buffer] += sumsq;
    }
    const uint64_t C = v.hdr[4], U = v.hdr[8], R = v.hdr[9], cW = hw[0], uW = hw[4];
    k.demod_preambles += C - cW;
    k.demod_preamblePhase[0] += v.hdr[5] - hw[1];
    k.demod_preamblePhase[1] += v.hdr[5] - hw[1];
    k.demod_preamblePhase[2] += v.hdr[6] - hw[2];
    k.demod_preamblePhase[3] += v.hdr[6] - hw[2];
    k.demod_preamblePhase[4] += v.hdr[7] - hw[3];
    k.demod_rejected_bad += (C - U - R) - (cW - uW - rc.skipped_uncond_groups) + rc.rejected_bad;
    k.demod_rejected_unknown_icao += rc.rejected_unknown + (U - rc.visited_cond_groups - uW);
    for (uint64_t b = 0; b < nbuf; ++b) {                    // noise power per buffer (demod_2400.c:474-479)
        const BufferClock &bc = job.buffers[b];
        double mean_power;
        if (c->cfg.format == MGPU_FMT_UC8) mean_power = (double) sums[nbuf + b] / 65535.0 / 65535.0 / bc.length;   // convert.c:105-107
        else { double f; std::memcpy(&f, &sums[nbuf + b], 8); mean_power = (double) ((float) f / (float) bc.length); }
        const double term = mean_power * bc.length - (double) buf_scaled[b] / 65535.0 / 65535.0;
        k.noise_power_sum += term;
        if (noise_terms) noise_terms->push_back(term);
        k.noise_power_count += bc.length;
        k.samples_lost += c->cfg.buf_samples - bc.length;    // readsb.c:886
    }
    k.samples_processed += n;
    k.nbuffers += nbuf;
    k.nflips = c->resolver.nflips();
    c->acc.build_ms += (float) (wall_ms() - t1);
    c->acc.n_messages += (uint64_t) wn;
    return MGPU_OK;
}

// Packets that continue the context's stream: per packet the ordered walk, the messages, the statistics.
static int walk_packets_checked(mgpu_ctx *c, const void *packets, uint64_t bytes) {
    const uint8_t *p = (const uint8_t *) packets, *end = p + bytes;
    if ((uintptr_t) packets & 7) { c->err = "mgpu_walk_packets: the packets must be 8-byte aligned"; return MGPU_E_INVAL; }
    while (p < end) {
        PacketView v;
        int rc = parse_packet(c, p, end, v, true);
        if (rc != MGPU_OK) return rc;
        if (v.pos != c->stream_pos) { c->err = "mgpu_walk_packets: packets must continue the stream in order"; return MGPU_E_INVAL; }
        rc = walk_one_packet(c, v, true, nullptr);
        if (rc != MGPU_OK) return rc;
        c->stream_pos += v.n;
        if (v.n % c->cfg.buf_samples) c->eof = true;
    }
    return MGPU_OK;
}

// The context's own packets (one rank holds the whole capture): reset, then walk them where the shard pass left them.
int mgpu_walk_packets(mgpu_ctx *c, const void *packets, uint64_t bytes) {
    if (!c || (!packets && bytes)) return MGPU_E_INVAL;
    if (c->eof) return MGPU_E_EOF;
    if (c->shard_mode != 0 || c->deferred) { c->err = "mgpu_walk_packets: the context is in the middle of a shard pass (or in deferred mode)"; return MGPU_E_INVAL; }
    { std::lock_guard<std::mutex> lk(c->mu); c->hot.store(true, std::memory_order_relaxed); }
    c->cv.notify_all();                      // the walker's team polls instead of sleeping while the packets are walked
    const int rc = guarded(c, [&] { return walk_packets_checked(c, packets, bytes); });
    c->hot.store(false, std::memory_order_relaxed);
    return rc;
}

// ---- config 5 with the ordered walk itself sharded: every rank walks its OWN range (include/modes_gpu.h) ----------------------
//
// What ties the ranges of one capture together is the ICAO filter: its two generations, `occupied`, the table size, and the clock
// of its 60 s expiry — which is data-dependent at millisecond granularity (the expiry after a buffer is tested against the
// timestamp of the buffer's last scored candidate, and the next is due 60 s after THAT: demod_2400.c:412-414, readsb.c:1227-1231),
// so a rank cannot know the schedule from the buffer grid.  The protocol (readsb_amd/shard.py):
//   1. every rank puts warm-up (two filter generations before its range) + range through the GPU pipeline and keeps the packets;
//   2. every rank ESTIMATES its buffers' end clocks from the records alone (mgpu_shard_clock_estimate); all-gather; the schedule
//      is the chain over all end clocks (mgpu_flip_schedule);
//   3. every rank walks warm-up + range with that schedule IMPOSED, from an empty filter at the warm-up's first sample (rank 0:
//      from the reference's initial state), and reports its true end clocks, the state it had at its range's first sample, the
//      state it ended with;
//   4. all-gather; done iff the chain over the true end clocks reproduces the schedule and every rank's state at its first
//      sample equals the state the rank before it ended with.  Otherwise: the new schedule, and a rank whose seam failed starts
//      its range from the imported state of its predecessor instead of its own warm-up; again from 3.
// At the fixed point every rank's walk IS the serial walk's (induction over buffers: rank 0 starts from the true state; the true
// rule expires the filter after buffer b iff the chain says so, because the chain runs the same rule on the same end clocks).
// Every range's messages are built by its own rank; integer counters add up; the two order-dependent double sums are re-added in
// stream order by whoever combines the ranges (mgpu_seqsum*, from the per-buffer terms / the messages themselves).

uint64_t mgpu_flip_schedule(const int64_t *end_clock, uint64_t nbuf, int64_t startup_ms, int filter_clock, uint64_t *flip_after, uint64_t cap) {
    std::vector<uint64_t> f;
    flip_schedule(end_clock, nbuf, startup_ms, filter_clock, f);
    for (size_t i = 0; i < f.size() && i < cap; ++i) flip_after[i] = f[i];
    return f.size();
}

uint64_t mgpu_expiry_windows(uint64_t nbuf_total, uint32_t buf_samples, int64_t startup_ms, int filter_clock, uint8_t *mask) {
    if (!mask && nbuf_total) return 0;
    return expiry_windows(nbuf_total, buf_samples ? buf_samples : 131072u, startup_ms, filter_clock, mask);
}

// What every rank concludes from a round's all-gather — the same on every rank, so no further exchange is needed.
int mgpu_shard_round(const int64_t *sched, uint64_t nsched, uint32_t world, const int64_t *const *clocks, const uint64_t *nclocks,
                     const void *const *state_first, const uint64_t *state_first_bytes, const void *const *state_end, const uint64_t *state_end_bytes,
                     uint64_t nsamples, uint32_t buf_samples, int64_t startup_ms, int filter_clock,
                     int64_t *next_sched, uint64_t cap, uint64_t *n_next, int32_t *import_from, int32_t *done) {
    if (!world || !clocks || !nclocks || !n_next || !import_from || !done || (nsched && !sched)) return MGPU_E_INVAL;
    if (!buf_samples) buf_samples = 131072;
    std::vector<int64_t> all;
    for (uint32_t r = 0; r < world; ++r) all.insert(all.end(), clocks[r], clocks[r] + nclocks[r]);
    if (nsamples % buf_samples == 0) all.push_back((int64_t) ((nsamples * 5) / 12000) + startup_ms);   // the EOF buffer (sdr_ifile.c:223-237): mgpu_finish's clock
    std::vector<uint64_t> f;
    flip_schedule(all.data(), all.size(), startup_ms, filter_clock, f);
    *n_next = f.size();
    bool same = f.size() == nsched;
    for (size_t i = 0; i < f.size(); ++i) {
        const int64_t ts = (int64_t) (f[i] * buf_samples) * 5;
        if (i < cap && next_sched) next_sched[i] = ts;
        if (same && sched[i] != ts) same = false;
    }
    if (f.size() > cap) return MGPU_E_CAPACITY;
    bool seams = true;
    int32_t prev = -1;                                          // the last rank with a range of its own (an empty range passes its neighbour's state through)
    for (uint32_t r = 0; r < world; ++r) {
        import_from[r] = -1;
        if (nclocks[r] == 0) continue;
        if (prev >= 0 && (state_first_bytes[r] != state_end_bytes[prev] || std::memcmp(state_first[r], state_end[prev], (size_t) state_end_bytes[prev]) != 0)) {
            import_from[r] = prev;
            seams = false;
        }
        prev = (int32_t) r;
    }
    *done = same && seams;
    return MGPU_OK;
}

static int shard_packets_span(mgpu_ctx *c, const void *&packets, uint64_t &bytes) {
    if (!packets) { packets = c->shard_packets.data(); bytes = c->shard_packets.size(); }
    if ((uintptr_t) packets & 7) { c->err = "shard packets must be 8-byte aligned"; return MGPU_E_INVAL; }
    return MGPU_OK;
}

int mgpu_shard_clock_estimate(mgpu_ctx *c, const void *packets, uint64_t bytes, uint64_t own_first, int64_t *end_clocks, uint64_t cap, uint64_t *n_out) {
    if (!c || !end_clocks || !n_out) return MGPU_E_INVAL;
    *n_out = 0;
    if (!packets && !c->shard_est_pos.empty()) {              // the context's own packets: the fetcher has estimated them as they came
        { const int rc = wait_all(c); if (rc != MGPU_OK) return rc; }
        size_t k = 0;
        while (k < c->shard_est_pos.size() && c->shard_est_pos[k] < own_first) ++k;
        const size_t off = k < c->shard_est_off.size() ? (size_t) c->shard_est_off[k] : c->shard_est.size();
        const size_t cnt = c->shard_est.size() - off;
        if (cnt > cap) { c->err = "mgpu_shard_clock_estimate: more buffers than the caller's array holds"; return MGPU_E_CAPACITY; }
        std::memcpy(end_clocks, c->shard_est.data() + off, cnt * sizeof(int64_t));
        *n_out = cnt;
        return MGPU_OK;
    }
    { const int rc = shard_packets_span(c, packets, bytes); if (rc != MGPU_OK) return rc; }
    const uint8_t *p = (const uint8_t *) packets, *end = p + bytes;
    std::vector<BufferClock> bufs;
    std::vector<int64_t> clocks;
    while (p < end) {
        PacketView v;
        const int rc = parse_packet(c, p, end, v, false);
        if (rc != MGPU_OK) return rc;
        if (v.pos < own_first) continue;
        ifile_grid(c, v.pos, v.n, bufs);
        estimate_end_clocks(v.recs, v.nrecs, bufs, clocks);
    }
    if (clocks.size() > cap) { c->err = "mgpu_shard_clock_estimate: more buffers than the caller's array holds"; return MGPU_E_CAPACITY; }
    std::memcpy(end_clocks, clocks.data(), clocks.size() * sizeof(int64_t));
    *n_out = clocks.size();
    return MGPU_OK;
}

static int shard_walk_checked(mgpu_ctx *c, const void *packets, uint64_t bytes, const mgpu_shard_walk_args *a, int64_t *end_clocks, uint64_t cap, uint64_t *n_out) {
    const uint8_t *p = (const uint8_t *) packets, *end = p + bytes;
    const double t_all = wall_ms();
    std::vector<PacketView> views;
    while (p < end) {
        PacketView v;
        const int rc = parse_packet(c, p, end, v, a->check_records != 0);
        if (rc != MGPU_OK) return rc;
        views.push_back(v);
    }
    c->pending.clear();
    std::memset(&c->counters, 0, sizeof(c->counters));
    std::memset(&c->acc, 0, sizeof(c->acc));
    c->shard_noise.clear();
    c->shard_sig.clear();
    c->eof = false;
    c->spec_segments = c->spec_batches = 0;
    c->shard_sched.assign(a->flip_after, a->flip_after + a->nflips);
    ShardWalkPlan plan;
    plan.own_first = a->own_first; plan.buf_samples = c->cfg.buf_samples; plan.startup_ms = c->cfg.startup_time_ms; plan.clock_mode = (int) c->cfg.filter_clock;
    plan.sched = c->shard_sched.data(); plan.nsched = c->shard_sched.size();
    plan.start_state = (const uint8_t *) a->start_state; plan.start_state_bytes = a->start_state_bytes;
    ShardWalkOut &out = c->shard_out;
    const char *err = "";
    double t_own = 0;
    const int rc = shard_walk_core(c->resolver, plan, views.size(),
        [&](size_t i, uint64_t &pos, uint64_t &n) { pos = views[i].pos; n = views[i].n; },
        [&](size_t i, bool own) {
            if (own && t_own == 0) { t_own = wall_ms(); c->acc.resolve_ms = 0; }          // (resolve_ms: the own range's walk; d2h_ms below: the warm-up's)
            const int wrc = walk_one_packet(c, views[i], own, own ? &c->shard_noise : nullptr);
            if (wrc == MGPU_OK && own) { c->stream_pos = views[i].pos + views[i].n; if (views[i].n % c->cfg.buf_samples) c->eof = true; }
            return wrc;
        }, out, &err);
    if (rc == -1) { c->err = std::string("mgpu_shard_walk: ") + err; return MGPU_E_INVAL; }
    if (rc != MGPU_OK) return rc;
    c->counters.nflips = c->resolver.nflips();
    if (out.clocks.size() > cap) { c->err = "mgpu_shard_walk: more buffers than the caller's array holds"; return MGPU_E_CAPACITY; }
    std::memcpy(end_clocks, out.clocks.data(), out.clocks.size() * sizeof(int64_t));
    *n_out = out.clocks.size();
    c->acc.d2h_ms = t_own > 0 ? (float) (t_own - t_all) : 0;
    c->acc.total_ms = (float) (wall_ms() - t_all);
    c->timing = c->acc;
    return MGPU_OK;
}

int mgpu_shard_walk(mgpu_ctx *c, const void *packets, uint64_t bytes, const struct mgpu_shard_walk_args *a, int64_t *end_clocks, uint64_t cap, uint64_t *n_out) {
    if (!c || !a || !end_clocks || !n_out || (a->nflips && !a->flip_after) || (a->start_state && !a->start_state_bytes)) return MGPU_E_INVAL;
    *n_out = 0;
    if (c->deferred || c->cfg.mode_ac || c->cfg.filter_clock == MGPU_FILTER_CLOCK_EXTERNAL || a->own_first % c->cfg.buf_samples) {
        c->err = "mgpu_shard_walk: not in deferred mode, not with Mode A/C or an external filter clock; ranges are whole buffers";
        return MGPU_E_INVAL;
    }
    { const int rc = wait_all(c); if (rc != MGPU_OK) return rc; }
    { const int rc = shard_packets_span(c, packets, bytes); if (rc != MGPU_OK) return rc; }
    { std::lock_guard<std::mutex> lk(c->mu); c->hot.store(true, std::memory_order_relaxed); }
    c->cv.notify_all();                      // the walker's team polls instead of sleeping while the packets are walked
    const int rc = guarded(c, [&] { return shard_walk_checked(c, packets, bytes, a, end_clocks, cap, n_out); });
    c->hot.store(false, std::memory_order_relaxed);
    return rc;
}

// ---- the same rank, its pass through the ORDINARY pipeline (walk and build overlapped with the GPU) ----
// mgpu_shard_walk above walks a range's packets after its GPU pass: nothing overlaps, and of a rank's 26 ms for an eighth of the
// one-hour capture 14 were walk and build (profiles/r04_config5_one_hour_emulate8.json).  When the schedule is known BEFORE the pass
// (readsb_amd/shard.py: it is the chain over end clocks of a few buffers around every expiry's possible positions — a pre-pass over
// ~5 % of the capture), warm-up and range go through the pipeline every other stream goes through: begin (cold start or imported
// state, schedule imposed), feed the warm-up, mark, feed the range, end.  Same outputs as mgpu_shard_walk: true end clocks, the
// states at the range's two ends, per-buffer noise terms; messages and counters by mgpu_collect.
int mgpu_shard_stream_begin(mgpu_ctx *c, const struct mgpu_shard_stream_args *a) {
    if (!c || !a || (a->nflips && !a->flip_after) || (a->start_state && !a->start_state_bytes)) return MGPU_E_INVAL;
    if (c->cfg.mode_ac || c->cfg.filter_clock == MGPU_FILTER_CLOCK_EXTERNAL || a->own_first % c->cfg.buf_samples || a->first_sample % c->cfg.buf_samples ||
        a->first_sample > a->own_first || (a->first_sample && !a->history_iq) || (a->start_state && a->first_sample != a->own_first)) {
        c->err = "mgpu_shard_stream_begin: whole-buffer ranges, no Mode A/C, no external filter clock; an imported state starts at the range's first sample";
        return MGPU_E_INVAL;
    }
    { const int rc = mgpu_reset(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    { const int rc = start_mid_stream(c, a->first_sample, a->history_iq); if (rc != MGPU_OK) return rc; }
    c->shard_sched.assign(a->flip_after, a->flip_after + a->nflips);
    for (size_t i = 1; i < c->shard_sched.size(); ++i)
        if (c->shard_sched[i] <= c->shard_sched[i - 1]) { c->err = "mgpu_shard_stream_begin: the schedule must be ascending"; return MGPU_E_INVAL; }
    Resolver &res = c->resolver;
    c->shard_stream_cold = false;
    if (a->start_state) {
        if (!res.import_state((const uint8_t *) a->start_state, a->start_state_bytes)) { c->err = "mgpu_shard_stream_begin: not a filter state"; return MGPU_E_INVAL; }
    } else if (a->first_sample == 0) res.reset(c->cfg.startup_time_ms, (int) c->cfg.filter_clock);
    else { res.reset_empty(c->cfg.startup_time_ms); c->shard_stream_cold = true; }
    res.set_schedule(c->shard_sched.data(), c->shard_sched.size());
    c->shard_stream = true;
    c->shard_marked = false;
    c->shard_noise_on = true;                                  // (the builder skips the warm-up's chunks altogether: only the range's buffers log a term)
    c->shard_stream_own_first = a->own_first;
    c->shard_out.clocks.clear(); c->shard_out.state_first.clear(); c->shard_out.state_end.clear();
    c->shard_noise.clear();
    c->shard_sig.clear();
    return MGPU_OK;
}

// What the walker does when the range begins (in stream order: behind the warm-up's last chunk, ahead of the range's first).
void shard_mark_now(mgpu_ctx *c) {
    Resolver &res = c->resolver;
    if (c->shard_stream_cold) {                                // the expiries before the range, counted from the schedule
        const int64_t ts0 = (int64_t) c->shard_stream_own_first * 5;
        res.set_nflips((uint64_t) (std::lower_bound(c->shard_sched.begin(), c->shard_sched.end(), ts0) - c->shard_sched.begin()) +
                       (c->cfg.filter_clock == MGPU_FILTER_CLOCK_BEFORE_FIRST ? 1u : 0u));
    }
    res.export_state(c->shard_out.state_first);
    res.log_end_clocks(&c->shard_out.clocks);
    c->shard_marked = true;
}

// Between the warm-up's feeds and the range's.  Synchronous feeds: the warm-up has been walked, the range begins here.  Deferred
// feeds (round 5): nothing waits — the warm-up's chunks may still be anywhere in the pipeline, the walker marks the range's begin
// itself when it gets to its first chunk (walk_job), and the range's kernels run while the warm-up is still being walked.  The
// warm-up's statistics are kept out of every accumulator chunk by chunk (fetch_slot, walk_job, build_job), so one accounting
// period covers the whole pass.
int mgpu_shard_stream_mark(mgpu_ctx *c) {
    if (!c || !c->shard_stream) return MGPU_E_INVAL;
    if (c->stream_pos != c->shard_stream_own_first) { c->err = "mgpu_shard_stream_mark: behind the warm-up's feeds, at the range's first sample"; return MGPU_E_INVAL; }
    if (c->deferred) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    c->pending.clear();                                        // (the warm-up leaves no messages and no statistics; nflips is set at the end)
    std::memset(&c->counters, 0, sizeof(c->counters));
    if (!c->shard_marked) shard_mark_now(c);
    return MGPU_OK;
}

int mgpu_shard_stream_end(mgpu_ctx *c, int64_t *end_clocks, uint64_t cap, uint64_t *n_out) {
    if (!c || !c->shard_stream || !end_clocks || !n_out) return MGPU_E_INVAL;
    *n_out = 0;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    if (!c->shard_marked) shard_mark_now(c);                   // (an empty range: no chunk of it ever reached the walker)
    c->resolver.log_end_clocks(nullptr);
    c->shard_noise_on = false;
    c->resolver.export_state(c->shard_out.state_end);
    c->counters.nflips = c->resolver.nflips();
    if (c->shard_out.clocks.size() > cap) { c->err = "mgpu_shard_stream_end: more buffers than the caller's array holds"; return MGPU_E_CAPACITY; }
    std::memcpy(end_clocks, c->shard_out.clocks.data(), c->shard_out.clocks.size() * sizeof(int64_t));
    *n_out = c->shard_out.clocks.size();
    return MGPU_OK;
}

int mgpu_shard_state(mgpu_ctx *c, int which, const void **blob, uint64_t *bytes) {
    if (!c || !blob || !bytes || which < 0 || which > 1) return MGPU_E_INVAL;
    const std::vector<uint8_t> &st = which ? c->shard_out.state_end : c->shard_out.state_first;
    *blob = st.data(); *bytes = st.size();
    return MGPU_OK;
}

int mgpu_shard_signal_terms(mgpu_ctx *c, const uint64_t **terms, uint64_t *n) {
    if (!c || !terms || !n) return MGPU_E_INVAL;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    if (c->cfg.mode_ac) { *terms = nullptr; *n = 0; return MGPU_OK; }      // (Mode A/C replies sit between the messages and carry no power: the message form)
    *terms = c->shard_sig.data(); *n = c->shard_sig.size();
    return MGPU_OK;
}

int mgpu_shard_noise_terms(mgpu_ctx *c, const double **terms, uint64_t *n) {
    if (!c || !terms || !n) return MGPU_E_INVAL;
    *terms = c->shard_noise.data(); *n = c->shard_noise.size();
    return MGPU_OK;
}

}  // extern "C"
