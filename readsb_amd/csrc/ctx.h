// ctx.h — private to the library: what the translation units behind the C ABI (api.cpp, affinity.cpp, shard.cpp, behind_out.cpp, behind_in.cpp) share —
// the context, its slots and jobs, and the few functions that cross files.
#pragma once
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <dirent.h>
#include <sched.h>

#include <cctype>
#include <algorithm>
#include <atomic>
#include <functional>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/modes_gpu.h"
#include "kernels.h"
#include "resolve.h"
#include "tables.h"

using namespace mgpu;

struct Behind;                                                // behind.h
struct Snip;                                                  // snip.h

constexpr int kPacketWords = 12;                              // header of a shard packet, 64-bit words: stream position, samples, live records,
constexpr uint64_t kPacketMagic = 0x3354454b4341504dull;      // magic, candidates, phases 4/5, 6/7, 8 tried, conditional-only / unconditional candidates, buffers, 0

namespace {
double wall_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}
}  // namespace

// A few persistent helper threads for fork-join over small task counts (the caller takes tasks too).
// Helpers spin briefly before blocking: the forks come every few hundred microseconds while a feed runs.
class Team {
  public:
    ~Team() { stop(); }
    // while *hot is set (a feed is running) idle helpers never block: a core that sleeps between two forks a few hundred
    // microseconds apart drops into a deep C-state, and the wake-up latency then costs more than the work (seen as a
    // 2.4x slower walker stage in the first run on an idle box)
    void start(int helpers, const std::atomic<bool> *hot = nullptr) {
        hot_ = hot;
        for (int i = 0; i < helpers; ++i) threads.emplace_back([this] { loop(); });
    }
    void stop() {
        { std::lock_guard<std::mutex> lk(mu_); quit_ = true; ++gen_; }
        wake_.fetch_add(1, std::memory_order_release);
        cv_work_.notify_all();
        for (auto &t : threads) if (t.joinable()) t.join();
        threads.clear();
    }
    void run(int ntasks, const std::function<void(int)> &fn) {
        if (ntasks <= 0) return;
        if (threads.empty() || ntasks == 1) { for (int i = 0; i < ntasks; ++i) fn(i); return; }
        uint32_t g;
        {
            std::lock_guard<std::mutex> lk(mu_);
            g = ++gen_;
            fn_ = &fn; ntasks_ = ntasks;
            pending_.store(ntasks, std::memory_order_relaxed);
            ticket_.store((uint64_t) g << 32, std::memory_order_release);
        }
        wake_.fetch_add(1, std::memory_order_release);
        cv_work_.notify_all();
        work(g, &fn, ntasks);
        // The helpers' last tasks: while a feed runs the caller POLLS for them too.  Asleep on the condition variable it came back
        // a scheduler wake-up later — tens of microseconds on an idle box, a millisecond on a loaded one, per fork — and the walk
        // forks several times per chunk: a candidate for the "slow mode" in which one stage of one process runs 1.2-8 x slower with
        // nothing else different (profiles/r05_headline_runs.txt, r06_host_4rank.txt), like the stage threads' sleeping GPU waits
        // before it (wait_event_spin).
        if (hot_ && hot_->load(std::memory_order_relaxed)) {
            for (unsigned spin = 0; pending_.load(std::memory_order_acquire) != 0 && spin < (1u << 22); ++spin) {
                __builtin_ia32_pause();
                if ((spin & 255) == 255) sched_yield();
            }
        }
        std::unique_lock<std::mutex> lk(mu_);
        cv_done_.wait(lk, [&] { return pending_.load(std::memory_order_acquire) == 0; });
        fn_ = nullptr;
    }
    std::vector<std::thread> threads;

  private:
    // tasks are handed out through one word that also carries the generation, so a helper that is late
    // leaving generation g can never take a task of generation g+1 with g's function
    void work(uint32_t g, const std::function<void(int)> *fn, int n) {
        int done = 0;
        uint64_t t = ticket_.load(std::memory_order_acquire);
        for (;;) {
            if ((uint32_t) (t >> 32) != g || (int) (uint32_t) t >= n) break;
            if (!ticket_.compare_exchange_weak(t, t + 1, std::memory_order_acq_rel)) continue;
            (*fn)((int) (uint32_t) t);
            ++done;
            t = ticket_.load(std::memory_order_acquire);
        }
        if (done && pending_.fetch_sub(done, std::memory_order_acq_rel) == done) {
            std::lock_guard<std::mutex> lk(mu_);
            cv_done_.notify_all();
        }
    }
    void loop() {
        uint64_t seen = wake_.load(std::memory_order_acquire);
        for (;;) {
            // spin (giving the core away in between: a helper that spins through its time slice starves whatever else the
            // scheduler put on this core); block only when no feed is running
            for (int spin = 0; wake_.load(std::memory_order_acquire) == seen; ++spin) {
                __builtin_ia32_pause();
                if ((spin & 63) == 63) sched_yield();
                if (spin >= 4000 && !(hot_ && hot_->load(std::memory_order_relaxed))) break;
            }
            const std::function<void(int)> *fn;
            int n;
            uint32_t g;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_work_.wait(lk, [&] { return quit_ || wake_.load(std::memory_order_acquire) != seen; });
                if (quit_) return;
                seen = wake_.load(std::memory_order_acquire);
                fn = fn_; n = ntasks_; g = gen_;
            }
            if (fn) work(g, fn, n);
        }
    }
    std::mutex mu_;
    std::condition_variable cv_work_, cv_done_;
    const std::function<void(int)> *fn_ = nullptr;
    int ntasks_ = 0;
    uint32_t gen_ = 0;
    std::atomic<uint64_t> ticket_{0}, wake_{0};
    std::atomic<int> pending_{0};
    const std::atomic<bool> *hot_ = nullptr;
    bool quit_ = false;
};

// One pipeline stage's worth of buffers: a chunk of the stream is converted, swept and pre-screened
// into a slot on the GPU while the worker thread walks the previous chunk's records on the host.
struct Slot {
    // device
    uint16_t *d_mag = nullptr;
    PhaseRec *d_pool = nullptr;
    uint32_t *d_dealer = nullptr;         // k_slice's tile dealer and, behind it, k_sweep's step dealer: 2 x 64 counters, one per 256 bytes (handed back zeroed by k_publish)
    uint32_t *d_pool_used = nullptr, *d_unit_first = nullptr, *d_unit_count = nullptr, *d_unit_live = nullptr;
    uint32_t *d_class_final = nullptr, *d_cand_count = nullptr, *d_sweep_part = nullptr;
    uint16_t *d_cand = nullptr;
    size_t class_bytes = 0;
    // one zero-initialised scratch block per chunk: counters | pool_used | per-buffer sums (1 memset, 1 copy back)
    unsigned long long *d_scratch = nullptr, *h_scratch = nullptr;
    size_t scratch_bytes = 0;
    unsigned long long *d_counters = nullptr, *d_sum_level = nullptr, *d_sum_power = nullptr, *d_win = nullptr, *d_msg_sig = nullptr;
    unsigned long long *d_win_part = nullptr;   // k_window_stats: per-workgroup totals of the chunk's skip windows
    double *d_fsum_level = nullptr, *d_fsum_power = nullptr;
    uint32_t *d_msg_pos = nullptr, *d_msg_limit = nullptr;
    uint16_t *d_msg_len = nullptr, *d_msg_skip = nullptr;
    PhaseRec *d_live = nullptr;          // k_prescreen_write: the surviving records, in stream order ...
    unsigned long long *d_live_sig = nullptr;   // ... and each one's would-be signal power
    unsigned long long *d_live_win = nullptr, *h_live_win = nullptr;   // shard passes (allocated by the first): ... and what its would-be skip window holds (k_window_stats_t<true>)
    // pinned host
    PhaseRec *h_live = nullptr;          // their copies: the fetcher pulls exactly nlive records over the copy engine (a kernel storing
    unsigned long long *h_live_sig = nullptr;   // into page-locked host memory waited 64 us per chunk on PCIe write latency)
    hipEvent_t ev_window = nullptr;       // k_window_stats of this slot's last use has run (stream2)
    bool window_pending = false;
    unsigned long long *h_counters = nullptr, *h_sums = nullptr, *h_win = nullptr, *h_sig = nullptr;
    double *h_fsums = nullptr;
    double *d_fsx = nullptr, *h_fsx = nullptr;   // SC16 formats: the float sums' own device / page-locked buffers (k_fsum_sc16 runs beside the chunk and ends on its own)
    uint32_t *h_msg_pos = nullptr, *h_msg_limit = nullptr;
    uint16_t *h_msg_len = nullptr, *h_msg_skip = nullptr;
    hipEvent_t ev_done = nullptr;        // the chunk is complete: recorded behind every chunk, WITHOUT a timestamp (a timed event is a marker the next kernel waits for)
    hipEvent_t ev[5] = {};               // 3: the end of the post-sweep stage (timed chunks only) | stage timing, sampled chunks only (timed): 0 1 convert, 1 4 k_sweep, 4 2 k_slice, 2 3 post-sweep (a timing event costs ~4.5 us of idle stream: neighbouring brackets share theirs)
    bool timed = false;
    uint32_t slice_blocks = 0;            // rows of d_sweep_part the chunk's k_slice wrote
    uint32_t sweep_blocks = 0;            // grid of the chunk's k_sweep
    uint32_t *d_ac_noise = nullptr;       // Mode A/C: per-buffer noise level
    AcCand *h_ac = nullptr;               // ... candidates, written by k_modeac straight into pinned host memory
    hipEvent_t ev_h2d = nullptr;          // the chunk's IQ samples have arrived in HBM (copy stream)
    // SC16 formats: the per-buffer float sums run beside the chunk's kernels on stream2 (k_fsum_sc16): what the converter waited
    // for | the sums are there | the converter has read the samples too
    hipEvent_t ev_pre = nullptr, ev_fsum = nullptr, ev_convdone = nullptr;
    bool fsum_pending = false;
    const uint8_t *fsum_iq = nullptr;     // the chunk's IQ samples (SC16 formats), for the float sums enqueued behind k_sweep
    int fsum_idx = -1;                    // which entry of mgpu_ctx::fsum_ring holds the chunk's float sums
    hipEvent_t ev_scan = nullptr;         // pre-screen offsets are final (main stream) -> the write pass may start (second stream)
    // the second stream keeps out of k_sweep's way (walk_job: hold_behind_sweep): the chunk's k_sweep has run | which chunk that was
    hipEvent_t ev_swept = nullptr;
    std::atomic<uint64_t> swept_seq{~0ull};
    // converter and sweep in one kernel (mgpu_ctx::sweep_fused, k_sweep_uc8): the chunk's samples and the 326 magnitudes before it, as
    // enqueue_convert found them (no converter launch); the per-step sums the kernel leaves for k_slice's prologue
    const uint8_t *fused_iq = nullptr;
    const uint16_t *fused_tail = nullptr;
    uint64_t seq = 0;                     // the chunk's number in the context's life (slot = seq % kSlots)
    // the job
    uint64_t n = 0, stream_pos = 0;
    uint8_t *d_wk_in = nullptr;           // the walk on the device: its input blob (read again by k_build_messages: the buffer clocks) ...
    void *d_wk_acc = nullptr;             // ... the chunk's ordered accept list ...
    unsigned long long *d_wk_sig = nullptr;   // ... and per accepted frame the signal power | long flag
    uint8_t *h_blob = nullptr, *d_blob = nullptr;   // device-messages mode: the walker's accept list + buffer clocks, page-locked host / device
    bool sig_late = false;                // the signal powers of this chunk are computed after the walk, for the accepted frames (k_msg_sig)
    int feed = -1;                        // deferred feeds: which FeedSlot the chunk's messages go to (-1: mgpu_ctx::pending)
    int32_t thr = 58;                     // preamble threshold of this chunk (raised after drops, demod_2400.c:335-338)
    bool have_mag = false, busy = false;
    bool have_noise = false;              // mag_buf entry with the caller's mean_level: Mode A/C noise level computed on the host
    uint32_t given_noise = 0;
    std::vector<BufferClock> buffers;
    std::vector<double> given_mean_power;
};

// Decoded messages waiting for mgpu_collect: a 64-byte aligned array that grows geometrically and is
// never value-initialised (the builder writes every byte of every message with streaming stores).
struct MsgBuf {
    mgpu_msg *p = nullptr;
    size_t n = 0, cap = 0;
    bool external = false;                            // p is the caller's buffer (mgpu_set_message_buffer): never grown, never freed
    ~MsgBuf() { if (!external) free(p); }
    size_t size() const { return n; }
    mgpu_msg *data() { return p; }
    void clear() { n = 0; }
    bool grow_for(size_t extra) {                     // room for `extra` more messages
        if (cap - n >= extra) return true;
        if (external) return false;
        size_t want = n + extra;
        if (want < 2 * cap) want = 2 * cap;
        void *q = nullptr;
        if (posix_memalign(&q, 64, want * sizeof(mgpu_msg)) != 0) return false;
        if (n) std::memcpy(q, p, n * sizeof(mgpu_msg));
        free(p);
        p = (mgpu_msg *) q;
        cap = want;
        return true;
    }
    void drop_front(size_t k) {
        if (k < n) std::memmove(p, p + k, (n - k) * sizeof(mgpu_msg));
        n -= k;
    }
    void use_external(mgpu_msg *buf, size_t capacity) {
        if (!external) free(p);
        p = buf; cap = capacity; n = 0; external = buf != nullptr;
        if (!external) { p = nullptr; cap = 0; }
    }
};

// What the builder thread needs of a chunk once its slot has gone back to the GPU.
struct HostJob {
    std::vector<PhaseRec> recs;              // the chunk's live records (heap copy of Slot::h_live)
    std::vector<unsigned long long> sig;
    std::vector<unsigned long long> win;     // shard passes: per live record the packed counts of its would-be skip window
    std::vector<Accepted> acc;               // the walker's decisions
    std::vector<uint32_t> pos;               // their chunk-relative scan positions
    std::vector<BufferClock> buffers;
    std::vector<double> given_mean_power;
    std::vector<unsigned long long> sums;    // per-buffer level / power sums of the converter
    std::vector<double> fsums;
    int fsum_idx = -1;                       // >= 0: the float sums are still on their way (mgpu_ctx::fsum_ring): the builder waits for them, not the fetcher
    std::vector<AcCand> ac;                  // Mode A/C candidates of the chunk (cfg.mode_ac)
    ResolveCounts rc;
    uint64_t nlive = 0;
    uint32_t nmsg = 0;                       // accepted frames: acc[0..nmsg), pos[0..nmsg)
    uint64_t stream_pos = 0;                 // stream position of the chunk's first sample
    int slot = -1;                           // the slot the chunk ran in (the walker still needs its device side)
    int feed = -1;                           // Slot::feed
    bool busy = false;
    // the walk ran on the device (MGPU_DEVICE_WALK=1): no records here; per message the signal power (bit 63: a 112-bit frame as
    // sliced) and — unless the messages stay on the device — the records k_build_messages made, both copied into page-locked memory
    bool from_device = false;
    bool sig_late = false;                   // Slot::sig_late: sig[] is empty, h_msig holds the accepted frames' signal powers (ev_copied)
    bool fetched = false;                    // recs / sig hold the chunk's live records
    mgpu_msg *h_msgs = nullptr;
    unsigned long long *h_msig = nullptr;
    hipEvent_t ev_copied = nullptr;          // ... the copies have landed (stream2)
    std::vector<uint32_t> buf_nacc;          // accepted frames per buffer
};

// Deferred feeds (mgpu_set_deferred): a feed call returns once its chunks are enqueued, the next one may follow at once, and
// mgpu_collect waits for the oldest uncollected feed only.  Each feed in flight has its own message list.
struct FeedSlot {
    MsgBuf msgs;
    // device-messages mode (mgpu_set_device_messages): the feed's messages are built by k_build_messages into d_msgs
    mgpu_msg *d_msgs = nullptr;
    mgpu_msg *d_ext = nullptr;                // mode 1: the caller's own device buffer for this feed's records (mgpu_set_device_message_buffer), else d_msgs
    uint64_t d_ext_cap = 0;
    mgpu_msg *d_list = nullptr;               // ... whichever of the two this feed's k_build_messages write to,
    uint64_t d_list_cap = 0;                  // ... and the records it holds
    mgpu_msg *host_dev = nullptr;             // mode 2 (device-built, host-delivered): the device address of msgs.p, the caller's page-locked array
    uint64_t d_cap = 0, d_count = 0;          // d_count: walker thread only, read by the caller after the feed is complete
    hipEvent_t ev_built = nullptr;            // the last k_build_messages of the feed has run (stream2)
    uint64_t jobs_total = 0, jobs_built = 0;  // chunks submitted / chunks whose messages are complete (under mgpu_ctx::mu)
    bool closed = false;                      // every chunk of the feed has been submitted
};

struct mgpu_ctx {
    // Ten slots (round 6; four in rounds 4-5, three before): a slot is held from the moment the feeding thread enqueues the chunk's
    // kernels until its walk is done.  With four, a caller that keeps two feeds of four chunks in flight (feed k + 1 before
    // collect k: bench.py, the C hosts) spent most of every feed call waiting for a slot, the GPU's queue was never more than one
    // or two chunks deep, and every hiccup of a host stage was a bubble on the GPU: 1.42-1.44 ms per 537 M samples with 4, 5 or 6
    // slots, 1.335 — the kernels' sum — with 8, 10 or 12 (profiles/r06_slots.txt).  Ten = the eight chunks of two feeds + two of
    // slack; ~1.5 GB of HBM each at the default chunk size, out of 288.
#ifndef MGPU_SLOTS
#define MGPU_SLOTS 10
#endif
    static constexpr int kSlots = MGPU_SLOTS;
    static constexpr int kJobs = MGPU_SLOTS + 2;              // fetched -> walked -> built: a job outlives its slot by the builder's stage
    static constexpr int kFsumRing = 2 * MGPU_SLOTS + 4;      // > kSlots + kJobs: an entry is free again before its index comes round
    mgpu_config cfg{};
    hipStream_t stream = nullptr, stream2 = nullptr, stream_w = nullptr;   // main | window statistics | pre-screen write pass / IQ uploads
    hipStream_t stream_d2h = nullptr;                                      // the fetcher's record copies
    // SC16 formats: the float sums of the chunks in flight — a ring, not the slots' own buffers, so that nobody has to wait for a chunk's
    // sums before the chunk's slot goes back to the GPU (chunk seq uses entry seq % kFsumRing)
    struct FsumRing { double *d = nullptr, *h = nullptr; void *scratch = nullptr; hipEvent_t ev = nullptr; } fsum_ring[kFsumRing];
    uint32_t prescreen_variant = 3;                                        // PostSweepParams::variant (the experiments build can ask for the older passes)
    hipStream_t stream_f = nullptr;                                        // SC16 formats: the float sums' chains (k_fsum_sc16), so that what follows a walk does not queue behind them
    int sweep_fused = 3;                                                   // without Mode A/C the sweep converts on the way (no converter launch, the magnitudes written once) — bit 0: UC8, k_sweep_uc8; bit 1: SC16 / SC16Q11, k_sweep_sc16; 0: k_convert_* + k_sweep (experiments build: MGPU_SWEEP_FUSED)
    hipStream_t s_post = nullptr;                                          // what follows the walk (window statistics, messages on the device): stream2, or stream_wk
    hipStream_t stream_wk = nullptr;                                       // the walk on the device: highest priority, its small kernels must not queue behind the main stream's
    std::string err;

    uint64_t cap_samples = 0;      // per feed call (cfg.max_samples)
    uint64_t chunk_samples = 0;    // per pipeline slot
    uint64_t cap_units = 0, cap_buffers = 0, cap_pool = 0, cap_msgs = 0, cap_ac = 0;   // per slot

    uint8_t *d_iq = nullptr;
    // host feeds upload chunk i of a feed into region i of d_iq (copy stream); the converter that read region i last (main stream)
    // must have run before the next upload into it may start — with deferred feeds of one or two chunks nothing else orders them
    std::vector<hipEvent_t> ev_iq_read;   // per region: recorded behind the converter of the last chunk uploaded there
    std::vector<char> iq_region_used;
    const uint16_t *tail_src = nullptr;   // device: the 326 magnitudes before the next chunk (end of the previous chunk's d_mag)
    uint64_t chunk_seq = 0;               // chunks alternate between the two slots across feeds
    uint32_t *d_adder_bitmap = nullptr;
    uint32_t *d_bit_syndrome = nullptr, *d_group_syndrome = nullptr;
    uint64_t *d_parity = nullptr, *d_tab_long = nullptr, *d_tab_short = nullptr;
    uint16_t *d_uc8_folded = nullptr;
    int n_long = 0, n_short = 0;
    Slot slot[kSlots];
    unsigned long long *d_win = nullptr, *h_win = nullptr;   // skip-window totals of the current feed
    uint64_t feed_cand[8] = {0, 0, 0, 0, 0, 0, 0, 0};         // C, phase[5], U, R of the current feed
    ResolveCounts feed_rc;
    std::vector<uint32_t> w_limit;                            // walker scratch (ordinary memory)
    std::vector<uint16_t> w_skip;
    HostJob job[kJobs];                                         // fetcher -> walker -> builder hand-off ring
    uint64_t job_seq = 0;

    std::vector<SyndromeEntry> tab_long, tab_short;
    uint32_t valid_long = 0, valid_short = 0;

    Resolver resolver;
    MsgBuf pending;
    static constexpr int kFeeds = 4;
    FeedSlot feed[kFeeds];                                    // deferred mode: ring of feeds in flight / uncollected
    uint64_t feed_head = 0, feed_tail = 0;                    // oldest uncollected feed, next feed to open
    bool deferred = false;
    int device_msgs = 0;                                      // mgpu_set_device_messages: 1 = the records stay in HBM (FeedSlot::d_msgs), 2 = k_build_messages stores them into the caller's page-locked array
    bool sig_late = true;                                     // MGPU_SIG_LATE=0: signal power of every live record in the pre-screen write pass (as in shard passes) instead of the accepted frames' after the walk
    int timing_every = 15;                                    // chunks per set of stage timing events (1 = every chunk; MGPU_TIMING_EVERY in the experiments build).  Odd: with feeds of four chunks the sampled chunk is not always a feed's first
    bool fsum_wide = false;                                   // (experiments build: MGPU_FSUM_WIDE=1) the float sums as three wide kernels instead of one chain per buffer
    float event_bracket_us = 4.5f;                            // what a pair of timing events adds to the kernel it brackets (mgpu_event_bracket_us measures it)
    uint64_t timing_seq = 0;
    bool accounting_open = false;                             // feed_begin has run, feed_end has not (deferred: spans several feeds)
    double acct_t0 = 0;
    mgpu_counters counters{};
    mgpu_timing timing{}, acc{};
    uint64_t stream_pos = 0;
    bool eof = false;

    // host pipeline behind the GPU: the walker thread takes the slots in submission order (record copy,
    // ordered accept walk, window-statistics launch) and hands a HostJob to the builder thread
    // (messages, signal / noise statistics), so that the serial walk is all the walker does
    std::thread fetcher, worker, builder;
    Team walk_team, build_team;                               // helpers of the walker / builder stage (MGPU_WALK_THREADS, MGPU_BUILD_THREADS)
    int walk_threads = 4, build_threads = 3;
    std::atomic<bool> hot{false};                             // a feed is running: the stage threads and helpers poll instead of sleeping
    std::vector<int> host_cpus;                               // the CPUs the host threads were pinned to (empty: not pinned)
    std::vector<SegmentWalk> segs;                            // the walker's buffer ranges
    std::vector<mgpu_msg> b_stage;                            // builder scratch (Mode A/C merge)
    // time-sharded capture (config 5, mgpu_shard_*): 0 = normal, 1 = sweep for the adder bitmap only, 2 = keep the
    // pre-screened records of every chunk as packets instead of walking them
    int shard_mode = 0;
    std::vector<uint8_t> shard_packets;
    // the sharded walk (mgpu_shard_walk): the imposed expiry schedule (the resolver points into it), the range's end clocks, what
    // each of its buffers adds to noise_power_sum, the filter state at the range's first sample / at its end
    std::vector<int64_t> shard_sched;
    std::vector<int64_t> shard_est;                           // the fetcher's estimate of every buffer's end clock, packet by packet
    std::vector<uint64_t> shard_est_pos, shard_est_off;       // ... the packets' first samples / offsets into shard_est
    std::vector<double> shard_noise;
    std::vector<uint64_t> shard_sig;                          // ... and every accepted message's sum of squared magnitudes (its signal power's numerator): 8 bytes
                                                              // per message for the sum blocks, where the messages themselves are 64
    ShardWalkOut shard_out;
    bool shard_noise_on = false;                              // a rank's pass through the ordinary pipeline (mgpu_shard_stream_*): the builder logs every buffer's noise term
    uint64_t shard_stream_own_first = 0;
    bool shard_stream = false, shard_stream_cold = false;
    bool shard_marked = false;                                // ... the range has begun for the walker (shard_mark_now): with deferred feeds the walker gets there on its own
    int device_slot = -1;                                     // which of the device's pipeline core groups this context pinned to
    // the ordered walk on the device (kernels/walk.inc).  MGPU_DEVICE_WALK=1: the walker thread only checks the walk's premises
    // and catches the filter up (Resolver::apply_device_walk), the chunk's records stay in HBM; =check: beside the host walk,
    // every decision compared (mgpu_debug_device_walk)
    int device_walk = 0;                                      // 0 off, 1 on, 2 check
    bool wk_serial_only = false;                              // MGPU_DBG_WK_SERIAL: every buffer through k_walk's serial decision loop (cross-check of the lane-parallel one)
    WalkBuffers wk{};
    uint8_t *h_wk_in = nullptr, *h_wk_sum = nullptr;
    size_t wk_in_cap = 0;
    mgpu_msg *d_wk_msgs = nullptr;                            // k_build_messages' output when the messages go to the host
    uint32_t wk_acc_cap = 0;                                  // accepted frames per buffer the walk has room for
    hipEvent_t ev_wk = nullptr;
    Resolver wk_shadow;                                       // check mode: the state before the host walk, for apply_device_walk
    uint64_t wk_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // chunks, taken from the device, not converged, premises failed (host walk), refused, walks, mismatches, -
    hipStream_t stream_aux = nullptr;                         // field decode / beast encoder / tracking gate: synchronous calls, not behind the pipeline's queued chunks
    std::unique_ptr<Behind> behind;                           // ... and their device state (behind.h)
    std::unique_ptr<Snip> snip;                               // mgpu_snip's (snip.h)
    uint16_t *d_hist = nullptr;                               // magnitudes of the 326 samples before the shard
    uint8_t *d_hist_iq = nullptr;
    unsigned long long *d_hist_sums = nullptr;
    // experiment / debug switches, read once at creation
    bool dbg_print = false;
    int dbg_stage = 0;
    std::string dump_dir;
    double feed_t0 = 0;                                       // wall clock at feed start (MGPU_DEBUG_PRINT timeline)
    uint64_t spec_segments = 0, spec_batches = 0;            // ranges walked, batches it took
    std::mutex mu;
    std::condition_variable cv;
    std::deque<int> queue, walk_queue, build_queue;
    bool stop = false;
    int worker_rc = MGPU_OK;
};

#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
            return e_ == hipErrorOutOfMemory ? MGPU_E_NOMEM : MGPU_E_HIP;                          \
        }                                                                                          \
    } while (0)

// affinity.cpp: host CPU affinity and the device's pipeline slots
struct NearDevice {
    cpu_set_t saved;
    bool moved = false;
    explicit NearDevice(int device);
    ~NearDevice();
};
int take_device_slot(int device);
void release_device_slot(int device, int slot);
void bind_near_device(std::thread *const *walk, int nwalk, std::thread *const *rest, int nrest, int device, int device_slot,
                      std::vector<int> *pinned);

extern "C" {
// api.cpp
int drain(mgpu_ctx *c);
int wait_all(mgpu_ctx *c);
int guarded(mgpu_ctx *c, const std::function<int()> &f);
void ifile_grid(const mgpu_ctx *c, uint64_t pos0, uint64_t n, std::vector<BufferClock> &v);
int64_t host_walk(mgpu_ctx *c, HostJob &job, const PhaseRec *recs, const std::vector<BufferClock> &buffers, uint64_t nlive, uint64_t aux_cap);
// shard.cpp
void shard_mark_now(mgpu_ctx *c);
}
