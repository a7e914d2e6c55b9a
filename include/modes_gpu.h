/* modes_gpu.h — C ABI of libmodes_gpu.so, the MI355X (gfx950) implementation of readsb's
 * Mode-S demodulator hot path:
 *
 *     IQ bytes -> magnitude (convert.c) -> 2.4 MSps preamble sweep + PPM bit slicer
 *     (demod_2400.c demodulate2400) -> CRC-24 + 1/2-bit repair (crc.c) -> scored, ordered
 *     message records ready for decodeModesMessage()/track.c.
 *
 * Everything here is `extern "C"`, plain pointers and sizes; the caller owns all host
 * memory, the library owns all device memory.  One context = one SDR stream on one GPU;
 * calls into a context must come from one thread at a time (the reference calls demodulate2400
 * from one decode thread only, readsb.c:871); inside, a context runs its own host threads
 * (mgpu_host_cpus).  Each entry point names the reference interface it replaces
 * (file:line under the reference tree).
 *
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md.
 */
#ifndef MODES_GPU_H
#define MODES_GPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* input_format_t, convert.h:28-31 (same numeric values) */
#define MGPU_FMT_UC8     0
#define MGPU_FMT_SC16    1
#define MGPU_FMT_SC16Q11 2

/* status codes (0 = ok, negative = error; text via mgpu_strerror) */
#define MGPU_OK              0
#define MGPU_E_INVAL        -1   /* bad argument / bad state */
#define MGPU_E_NODEVICE     -2   /* no usable HIP device: the library never falls back to the CPU */
#define MGPU_E_HIP          -3   /* a HIP runtime call failed (message via mgpu_last_error) */
#define MGPU_E_NOMEM        -4
#define MGPU_E_OVERFLOW     -5   /* a device-side pool was too small; recreate with a larger pool */
#define MGPU_E_CAPACITY     -6   /* more samples than cfg.max_samples in one call */
#define MGPU_E_EOF          -7   /* stream already ended on a short buffer (sdr_ifile.c:223-237) */

/* Bumped whenever a struct of this header grows or an entry point changes meaning.  5 (round 5): mgpu_config.abi_version is checked
 * by mgpu_create, mgpu_abi_version() exported; 4 (round 4): mgpu_config.chunk_buffers; with MGPU_FILTER_CLOCK_EXTERNAL the filter
 * starts EMPTY since 3 (the host mirrors modesInit's icaoFilterAdd(Modes.show_only)). */
#define MGPU_ABI_VERSION 6
/* The version the loaded library was built with: a host compares it with the MGPU_ABI_VERSION of the header it was compiled against. */
uint32_t mgpu_abi_version(void);

typedef struct mgpu_ctx mgpu_ctx;

/* Options of the hot path, named after the struct _Modes fields they mirror. */
struct mgpu_config {
    int32_t  device;              /* HIP device ordinal */
    int32_t  format;              /* MGPU_FMT_*: --iformat (sdr_ifile.c:82-108) */
    int32_t  nfix_crc;            /* Modes.nfix_crc: 0 --no-fix, 1 --fix (default, readsb.c:150), 2 --aggressive */
    int32_t  fixDF;               /* Modes.fixDF (readsb.c:194), 0 with --no-fix-df */
    int32_t  preamble_threshold;  /* Modes.preambleThreshold, default 58 (readsb.c:2268); 1 .. 4095 (the reference clamps to 40 .. 400,
                                   * readsb.c:1473; beyond 6000 k_sweep's 32-bit accumulators could overflow): MGPU_E_INVAL otherwise */
    uint32_t buf_samples;         /* Modes.sdr_buf_samples, default 131072 (readsb.c:2212); multiple of 4096 */
    uint32_t trailing_samples;    /* Modes.trailing_samples = 326 (readsb.c:288); must be 326 */
    uint32_t mode_ac;             /* Modes.mode_ac (--modeac): also run demodulate2400AC on every buffer, readsb.c:871-874.  Every
                                   * format: its noise floor comes from the buffer's mean level / power, which for SC16 / SC16Q11 are
                                   * the reference's sequential float sums (convert.c:225-249), reproduced bit for bit.
                                   * Capacity: the scan works on a pipeline chunk (max_samples rounded up to whole buffers, at most
                                   * chunk_buffers of them) in tiles of 2048 positions and appends a tile's candidates (the positions
                                   * that pass every test of the loop body, before the skip over an accepted reply) to list
                                   * (tile mod 64) of 64 lists, each with room for (chunk samples / 256 + 65536) / 64 candidates: 1032
                                   * with a chunk of one buffer, where a list serves one tile and a tile has at most 1024, so that
                                   * nothing can overflow; 1536 with 64 buffers, 2560 with 1024.  Larger chunks are sized for one
                                   * reply per 256 samples: a chunk that gives one list more than its room (replies packed 70
                                   * samples apart over 64 buffers do) fails its feed with MGPU_E_OVERFLOW; no reply is ever
                                   * dropped without that error, and mgpu_reset leaves the context usable again. */
    uint64_t max_samples;         /* largest number of new samples one mgpu_feed_* call may carry */
    int64_t  startup_time_ms;     /* Modes.startup_time: wall clock (ms) the 12 MHz sample clock is anchored to */
    uint64_t record_pool_records; /* device pool for per-phase candidate records; 0 = max_samples/16 + 65536 */
    uint64_t max_messages;        /* cap on accepted messages kept per feed; 0 = max_samples/64 + 65536 */
    uint32_t filter_clock;        /* MGPU_FILTER_CLOCK_*: who runs icaoFilterExpire (readsb.c:1227-1231), see below */
    uint32_t streams_on_device;   /* how many contexts this process runs on the device (0 / 1: this one alone).  With several, every one of them
                                   * keeps its host stages small (4 walkers, 3 builders): the stage threads poll while a feed runs, and eight
                                   * contexts with a lone stream's teams (8 + 6) oversubscribe the device's two L3 groups — measured, 8 streams:
                                   * 9.4 Gsamples/s, with small teams 18.7 (profiles/r03_fanin.txt) */
    uint32_t chunk_buffers;       /* buffers per pipeline chunk (one launch of every kernel); 0 = 1024 (half as many kernel boundaries and tails
                                   * as 512: 325 against 300 Gsamples/s, profiles/r04_chunk_buffers.txt); a host that wants its messages sooner
                                   * takes fewer (latency = three chunks), one that wants throughput takes 2048 and keeps two feeds of 4096
                                   * buffers enqueued ahead of the one it collects (1.12 against 1.21 ms per 537 M samples: the kernels'
                                   * ramps and tails again; the host's ordered walk takes a chunk in rounds of 1024 buffers whatever its
                                   * length, profiles/r06_chunk_2048.txt; memory per context doubles with it: ten slots of ~3 GB) */
    uint32_t abi_version;         /* MGPU_ABI_VERSION of the header the HOST was compiled against (mgpu_config_defaults below passes it);
                                   * mgpu_create() refuses another (MGPU_E_INVAL) — a host built against an older, shorter struct would
                                   * otherwise have the bytes behind its struct read as chunk_buffers.  (The last field: it sits where such a
                                   * host's struct has ended.) */
};

/* The ICAO filter's 60 s expiry (backgroundTasks, readsb.c:1227-1231: `static next_flip = 0`, so the first
 * icaoFilterExpire() runs at the first backgroundTasks call).  The reference program itself has two start-up orders:
 * its decode thread either finds the first buffer waiting (flip AFTER buffer 0, next one 60 s after the clock at the end
 * of buffer 0) or does not (flip BEFORE buffer 0, on the still empty filter, next one 60 s after start-up) — thread
 * scheduling decides (readsb.c:857-902).  The orders differ in which filter generation buffer 0's addresses land in, and
 * therefore in what the next table resize drops (icao_filter.c:65-93).
 *   AFTER_FIRST   the library runs the clock on the buffers' sysTimestamp, first expiry after buffer 0 (default; what the
 *                 oracle, the goldens and a reference run with a slow decode-thread start do)
 *   BEFORE_FIRST  the same clock, first expiry before buffer 0 (anchored to startup_time_ms)
 *   EXTERNAL      the library never expires on its own: the host forwards every icaoFilterExpire() it performs with
 *                 mgpu_filter_expire() (and foreign icaoFilterAdd()s, e.g. from network input, with mgpu_filter_add())
 *                 between two feed calls.  This is what a readsb process linked against the library uses
 *                 (readsb_amd/host/readsb_tree/demod_gpu_wrap.c wraps icaoFilterExpire): its own filter and the
 *                 library's then flip at the same buffer boundaries whatever clock the host runs (synthetic or wall).
 *                 In this mode the filter starts EMPTY: the host's own first add — modesInit's icaoFilterAdd(Modes.show_only),
 *                 readsb.c:310, whatever --show-only is — must be mirrored with mgpu_filter_add() like every other one. */
#define MGPU_FILTER_CLOCK_AFTER_FIRST  0
#define MGPU_FILTER_CLOCK_BEFORE_FIRST 1
#define MGPU_FILTER_CLOCK_EXTERNAL     2

/* Fills cfg with the reference defaults (configSetDefaults, readsb.c:150-228). */
/* Defaults of every field.  C / C++ hosts get the macro: it hands the library the size and the version of the struct THEY were compiled
 * with, the library writes no byte beyond that size and records the version for mgpu_create's check.  The plain entry point writes
 * sizeof(the LIBRARY's struct) bytes and the library's own version: safe only for a caller whose struct is this header revision's —
 * a binding that looks symbols up at run time should carry its own version constant and call mgpu_config_defaults_abi with it, as
 * readsb_amd/binding.py does (ABI_VERSION; it also refuses a library whose mgpu_abi_version() differs). */
void mgpu_config_defaults_abi(struct mgpu_config *cfg, uint32_t struct_bytes, uint32_t abi_version);
void mgpu_config_defaults(struct mgpu_config *cfg);
#ifndef MGPU_NO_DEFAULTS_MACRO
#define mgpu_config_defaults(cfg) mgpu_config_defaults_abi((cfg), (uint32_t) sizeof(struct mgpu_config), MGPU_ABI_VERSION)
#endif

/* One accepted message, in stream order: everything demodulate2400 hands to
 * decodeModesMessage()/netUseMessage() (demod_2400.c:401-471).  64 bytes. */
struct mgpu_msg {
    int64_t  timestamp;       /* mm->timestamp, 12 MHz ticks, end of bit 56 (demod_2400.c:406) */
    int64_t  sysTimestamp;    /* mm->sysTimestamp, ms (demod_2400.c:409) */
    uint64_t sig_sumsq;       /* sum of mag^2 over the signal window (demod_2400.c:442-445) */
    uint16_t sig_len;         /* samples in that window: msglen*12/5 = 268 or 134 */
    int16_t  score;           /* mm->score (scoreModesMessage, mode_s.c:309) */
    uint8_t  phase;           /* bestphase 4..8 */
    uint8_t  correctedbits;   /* mm->correctedbits after decodeModesMessage */
    uint8_t  msgtype;         /* DF after DF repair (mm->msgtype) */
    uint8_t  msgbits;         /* 56 or 112 after DF repair (mm->msgbits) */
    uint32_t addr;            /* address the CRC stage settled on (AA, or the AP syndrome) */
    uint8_t  msg[14];         /* corrected frame = mm->msg after decodeModesMessage */
    uint8_t  raw[14];         /* frame as sliced = what demodulate2400 copies into mm->msg (:420) */
};
/* signalLevel exactly as demod_2400.c:447-448 */
static inline double mgpu_msg_signal_level(const struct mgpu_msg *m) {
    return (double) m->sig_sumsq / 65535.0 / 65535.0 / (double) m->sig_len;
}

/* struct stats demod counters the reference updates inside demodulate2400
 * (stats.h:62-82; demod_2400.c:216,387-456,474-479), accumulated since create/reset. */
struct mgpu_counters {
    uint64_t demod_preambles;
    uint64_t demod_rejected_bad;
    uint64_t demod_rejected_unknown_icao;
    uint64_t demod_accepted[3];
    uint64_t demod_preamblePhase[5];
    uint64_t demod_bestPhase[5];
    uint64_t strong_signal_count;
    uint64_t signal_power_count;
    uint64_t noise_power_count;
    uint64_t samples_processed;
    uint64_t samples_lost;
    uint64_t nbuffers;
    uint64_t nflips;             /* icaoFilterExpire() calls made by the filter clock */
    double   signal_power_sum;
    double   noise_power_sum;
    double   peak_signal_power;
    uint64_t demod_modeac;       /* Mode A/C replies accepted (stats.h:72), only with cfg.mode_ac */
};

/* Where the last feed's time went (ms).  The four kernel figures are pairs of HIP events on the context's main stream around ONE
 * kernel / one group of kernels, on the first chunk since the figures were last reset and every fifteenth after it (seventh until round 6; n_timed_chunks: a timing event costs ~5 us of idle stream; neighbouring figures share an event); a pair adds
 * a constant ~4 us to what it brackets (mgpu_event_bracket_us measures it).  The host figures are wall-clock sums of stage threads
 * that run beside each other and beside the GPU: they overlap, they do not add up to total_ms. */
struct mgpu_timing {
    float h2d_ms;        /* host time spent issuing the IQ block's host->device copies (0 for resident input) */
    float convert_ms;    /* k_convert_* (UC8 / SC16 / SC16Q11 -> magnitudes, per-buffer sums) */
    float sweep_ms;      /* k_sweep alone: the preamble sweep, the kernel the HBM roofline applies to */
    float prescreen_ms;  /* the post-sweep passes: k_count (+ class bitmap) + k_prescreen_write + k_publish */
    float resolve_ms;    /* walker team: the ordered accept / skip-ahead / ICAO filter walk (host wall time) */
    float sigpower_ms;   /* walker thread: launching what follows the walk on the second stream (k_stage_in, k_window_stats incl. the signal powers, k_build_messages) */
    float d2h_ms;        /* fetcher thread: waiting for the chunk, the live records HBM -> page-locked memory -> the walk's memory (host wall time) */
    float total_ms;      /* wall time of the whole call (deferred feeds: since the accounting was opened) */
    uint64_t n_candidates;   /* positions that passed a preamble threshold */
    uint64_t n_records;      /* per-phase records the slicer emitted */
    uint64_t n_live_records; /* records that survived the pre-screen (reach the ordered walk) */
    uint64_t n_messages;     /* accepted messages */
    uint64_t n_chunks;       /* pipeline chunks = launches of each kernel */
    float slice_ms;          /* k_slice: bit slicer + CRC-24 + the filter-independent half of the scoring */
    float build_ms;          /* builder team: struct modesMessage fields + signal / noise statistics — the stage's own work (host wall time;
                              * until ABI 6 this figure also held the wait below) */
    uint64_t n_timed_chunks; /* chunks that carried the stage timing events: convert_ms, sweep_ms, slice_ms and prescreen_ms are sums
                              * over THESE (every 15th chunk; experiments build: MGPU_TIMING_EVERY) */
    float build_wait_ms;     /* builder thread: waiting for the chunk's signal powers (second stream) / the SC16 formats' float sums: idle, not work (ABI 6) */
    float sweep_fused_chunks; /* of the timed chunks, those whose sweep_ms is k_sweep_uc8's — converter and sweep in one kernel (UC8 without Mode A/C):
                               * convert_ms holds nothing for them, the kernel reads the IQ samples and writes the magnitudes (4 B per sample) */
};

/* ---- lifecycle -------------------------------------------------------------------- */

/* Replaces modesInit()'s hot-path part: modesChecksumInit(nfix_crc), icaoFilterInit(),
 * icaoFilterAdd(show_only), init_converter() (readsb.c:306-310, sdr_ifile.c:156).
 * The filter starts holding show_only's default (0xff123456, readsb.h:296) — EXCEPT with cfg.filter_clock ==
 * MGPU_FILTER_CLOCK_EXTERNAL, where it starts EMPTY and the host mirrors its own icaoFilterAdd(Modes.show_only) with mgpu_filter_add
 * like every other add: with a user --show-only a default entry added here as well would leave `occupied` one ahead of the host's
 * and the table resizes (icao_filter.c:65-93) on different adds (readsb_tree/demod_gpu_wrap.c replays the host's early adds). */
int  mgpu_create(const struct mgpu_config *cfg, mgpu_ctx **out);
void mgpu_destroy(mgpu_ctx *ctx);
/* Back to the state right after mgpu_create (sample clock 0, filter = {show_only's default}; empty with the EXTERNAL clock). */
int  mgpu_reset(mgpu_ctx *ctx);
const char *mgpu_strerror(int code);
const char *mgpu_last_error(mgpu_ctx *ctx);
/* 1 when a gfx950-class HIP device is visible, 0 otherwise (never throws). */
int  mgpu_device_count(void);

/* ---- whole hot path: what sdr_ifile.c's reader + the decode thread do per block ------ */

/* ifileRun's read+convert (sdr_ifile.c:194-259) followed by demodulate2400() per
 * 131072-sample buffer (readsb.c:871) and the per-buffer filter clock (readsb.c:1227-1231),
 * for `nsamples` new IQ samples continuing the stream.  nsamples need not be a multiple of
 * buf_samples; a short last buffer ends the stream exactly like a short read() does.
 * Synchronous (unless mgpu_set_deferred): on return the accepted messages are available to mgpu_collect(). */
int mgpu_feed_iq(mgpu_ctx *ctx, const void *iq_host, uint64_t nsamples);

/* Deferred feeds — a continuous stream handed over block after block without the pipeline running empty in between.
 * With on != 0, mgpu_feed_iq / mgpu_feed_iq_device return as soon as the block's chunks are enqueued (they still block while
 * all three pipeline slots are busy), the next block may follow at once, and mgpu_collect() waits for the OLDEST uncollected
 * feed only and returns exactly that feed's messages — so the caller's loop is  feed(k+1); collect(k).  At most 4 feeds may be
 * uncollected.  mgpu_set_message_buffer() then names the array of the NEXT feed (alternate two arrays).  The demod counters
 * settle when nothing is in flight: passing `counters` to mgpu_collect, and mgpu_finish / mgpu_last_timing / mgpu_reset /
 * mgpu_filter_* / mgpu_set_deferred, wait for everything enqueued so far (they "drain"); mgpu_last_timing then covers everything
 * since the previous drain.  The result — messages, their order, every counter — is identical to feeding the same blocks
 * synchronously.  The struct mag_buf entries and the shard calls are refused (MGPU_E_INVAL) while deferred mode is on.
 * Lifetime of the caller's block: a deferred mgpu_feed_iq returns when the last byte of `iq_host` has been copied to the device
 * (the kernels are still to run), so the block may be reused at once, exactly as after a synchronous feed; a device block
 * (mgpu_feed_iq_device) is read by kernels that are still to run and must stay untouched until that feed has been collected.
 * While feeds are in flight the CALLING thread's waits (for a free slot in a feed call, for the oldest feed in mgpu_collect) poll —
 * pauses and sched_yield, as the stage threads' do — instead of sleeping on a condition variable: a wake-up that comes a
 * millisecond late on a loaded host is as long as the work the GPU still has queued. */
int mgpu_set_deferred(mgpu_ctx *ctx, int on);

/* Device-resident messages (deferred mode only, no Mode A/C): the accepted frames' records are built on the GPU
 * (k_build_messages: demod_2400.c:399-445 + the CRC stage's repair, mode_s.c:443-606, lane = message) from the walk's accept
 * list and the live records that already are in HBM, into a list per feed; the host builds nothing and no message crosses PCIe
 * unless asked for.  mgpu_collect_device() waits for the oldest uncollected feed like mgpu_collect() and returns the device
 * pointer of its `*n` records, in stream order — valid until three more feeds have been started — ready for
 * mgpu_decode_fields_device / mgpu_beast_encode_device or an aggregator's RCCL gather (readsb_amd/gather.py: submit_device).
 * mgpu_collect() in this mode copies the whole feed to the host (MGPU_E_OVERFLOW if `cap` is smaller than the feed).
 * The list of a feed holds (chunks per feed) x cfg.max_messages records (default per chunk: samples / 64 + 65536).
 * on == 2 (round 6): built on the GPU the same way, but k_build_messages stores the records straight into the array
 * mgpu_set_message_buffer() named for the feed — which must be page-locked (mgpu_host_alloc / mgpu_host_register; MGPU_E_INVAL
 * from the feed call otherwise): the host has its list, identical bytes, and builds nothing; its builder stage keeps the two
 * order-dependent sums.  mgpu_collect() then waits for the feed's last k_build_messages and returns the count (no copy when
 * `out` is that array).  The mode for hosts that take struct modesMessage fields on the CPU from an HBM-resident pipeline. */
int mgpu_set_device_messages(mgpu_ctx *ctx, int on);
/* Mode 1: the NEXT feed's records are built into the caller's own device buffer (capacity records) instead of the library's list —
 * e.g. the fixed-size buffer an RCCL gather sends from (readsb_amd/gather.py: no device-to-device copy between the demodulator
 * and the collective; the buffer's lifetime is the caller's).  mgpu_collect_device() then returns that pointer.  NULL: back to the
 * library's list.  Named before every feed that wants it, like mgpu_set_message_buffer. */
int mgpu_set_device_message_buffer(mgpu_ctx *ctx, struct mgpu_msg *d_buf, uint64_t capacity);
int mgpu_collect_device(mgpu_ctx *ctx, const struct mgpu_msg **d_msgs, uint64_t *n, struct mgpu_counters *counters);

/* Same, for IQ already resident in device memory (HBM): d_iq is a device pointer to
 * nsamples samples of cfg.format.  This is the entry the benchmark times. */
int mgpu_feed_iq_device(mgpu_ctx *ctx, const void *d_iq, uint64_t nsamples);

/* Host -> HBM copy only (no processing): stages nsamples IQ samples in the context's device
 * input buffer, whose address mgpu_device_iq_buffer() returns; follow with
 * mgpu_feed_iq_device(ctx, mgpu_device_iq_buffer(ctx), nsamples) to demodulate them in place. */
int   mgpu_upload_iq(mgpu_ctx *ctx, const void *iq_host, uint64_t nsamples);
void *mgpu_device_iq_buffer(mgpu_ctx *ctx);

/* The CPUs the context pinned its host threads to (one physical core each, one L3; 0 = not pinned, e.g. with
 * MGPU_NO_AFFINITY=1).  An application that wants the full speed keeps its own busy threads off these cores and
 * their SMT siblings: a thread of the application sharing a core with a pipeline stage costs up to 30 %.
 * The cores are chosen among the CPUs the process could run on when the library was LOADED (cgroups, taskset) — not among those
 * the creating thread may use at the moment, so that an application following the advice above can create further contexts. */
int mgpu_host_cpus(mgpu_ctx *ctx, int32_t *cpus, int32_t cap);

/* Page-locked host memory placed on the device's NUMA node (hipHostMalloc while the calling thread sits on that node), for the
 * arrays the library writes at full speed: the message arrays of mgpu_set_message_buffer (an aggregator's staging buffers that
 * go on to the GPU), sample buffers.  Pinned memory allocated from a thread on the other socket costs the builder ~10 % of the
 * step.  Free with mgpu_host_free. */
void *mgpu_host_alloc(mgpu_ctx *ctx, uint64_t bytes);
void  mgpu_host_free(mgpu_ctx *ctx, void *ptr);

/* Optional: page-lock a host buffer the caller keeps feeding from (the SDR plugin's read buffer, the
 * ifile reader's `readbuf`, sdr_ifile.c:140) so that mgpu_feed_iq's chunked uploads run at PCIe speed
 * and overlap the kernels.  Unregister before freeing the buffer. */
int mgpu_host_register(mgpu_ctx *ctx, void *ptr, uint64_t bytes);
int mgpu_host_unregister(mgpu_ctx *ctx, void *ptr);

/* EOF handling of ifileRun: when the stream length is an exact multiple of buf_samples the
 * reference pushes one more zero-length buffer (sdr_ifile.c:223-237).  Call once at end. */
int mgpu_finish(mgpu_ctx *ctx);

/* Messages of the calls since the last collect, in stream order (netUseMessage order,
 * demod_2400.c:471).  Copies up to `cap` messages, *n = number copied; remaining count
 * via mgpu_pending_messages().  counters may be NULL. */
int mgpu_collect(mgpu_ctx *ctx, struct mgpu_msg *out, uint64_t cap, uint64_t *n,
                 struct mgpu_counters *counters);
/* Optional: have the messages built straight into the caller's array (capacity records) instead of an
 * internal list.  After a feed, mgpu_collect(ctx, buf, capacity, &n, ...) with the same pointer only
 * reports n and makes the array writable again — no copy (the builder threads have written the 64-byte
 * records with streaming stores; 16-byte alignment of buf keeps that fast).  A feed that needs more
 * room than capacity fails with MGPU_E_OVERFLOW.  buf = NULL returns to the internal list.  The array
 * may be replaced between feeds (e.g. alternating staging buffers) once the pending messages are
 * collected. */
int mgpu_set_message_buffer(mgpu_ctx *ctx, struct mgpu_msg *buf, uint64_t capacity);

uint64_t mgpu_pending_messages(mgpu_ctx *ctx);

/* icaoFilterExpire() (icao_filter.c:96-110) / icaoFilterAdd() (:112-130) on the context's filter, between two feed
 * calls.  mgpu_filter_expire is how a host drives the filter with cfg.filter_clock = MGPU_FILTER_CLOCK_EXTERNAL (it is
 * refused with MGPU_E_INVAL in the other modes: two clocks would double-flip); mgpu_filter_add mirrors adds the host
 * makes outside the demodulator (decodeModesMessage on network input, mode_s.c:766-779) and is allowed in every mode: an
 * address added this way is known to the device's pre-screen too, whether or not the stream ever carries it as DF11 / DF17.
 * Both calls wait for deferred feeds in flight first. */
int mgpu_filter_expire(mgpu_ctx *ctx);
int mgpu_filter_add(mgpu_ctx *ctx, uint32_t addr);

int mgpu_last_timing(mgpu_ctx *ctx, struct mgpu_timing *t);
/* What mgpu_timing's per-kernel figures (convert_ms, sweep_ms, slice_ms: a pair of timing HIP events around ONE kernel in a busy
 * stream) contain beyond the kernel's own duration: measured here, now, with a kernel of known duration (it spins 20 us on the
 * GPU's 100 MHz counter) between two such events — 4.0 us on an MI355X under ROCm 7.2, whatever the kernel's length
 * (tools/micro/event_overhead.hip).  bench.py subtracts it from its per-launch figures and reports both. */
int mgpu_event_bracket_us(mgpu_ctx *ctx, float *us);

/* ---- the two plugin-surface pieces on their own ----------------------------------- */

/* iq_convert_fn (convert.h:34-39) for the non-DC-filter converters convert_uc8_nodc,
 * convert_sc16_nodc, convert_sc16q11_nodc (convert.c:64,212,329): nsamples IQ samples in
 * host memory -> nsamples u16 magnitudes in host memory; out_mean_* may be NULL.  Not in the middle of a stream fed through
 * mgpu_feed_iq* on the same context (MGPU_E_INVAL: it would overwrite the stream's 326-sample tail): one context per role. */
int mgpu_convert(mgpu_ctx *ctx, const void *iq_host, uint16_t *mag_host, uint32_t nsamples,
                 double *out_mean_level, double *out_mean_power);

/* demodulate2400(struct mag_buf *) (demod_2400.h:38) on one magnitude buffer laid out as
 * struct mag_buf.data (readsb.h:450-464): trailing_samples of overlap then `length` new
 * samples.  The caller passes the struct's scalar fields; messages come back through
 * mgpu_collect().  The stream position / filter clock advance exactly as for mgpu_feed_iq.
 * dropped: nonzero = the host has recently dropped samples (what demod_2400.c:335-338 reads from
 * Modes.stats_15min.samples_dropped): this buffer is swept with max(PREAMBLE_THRESHOLD_PIZERO = 75,
 * cfg.preamble_threshold), as the reference does. */
int mgpu_demod_mag_buf(mgpu_ctx *ctx, const uint16_t *data, uint32_t length,
                       int64_t sampleTimestamp, int64_t sysTimestamp,
                       double mean_power, uint32_t dropped);
/* The same when cfg.mode_ac is set — demodulate2400(buf) followed by demodulate2400AC(buf) (readsb.c:871-874): the Mode A/C
 * demodulator derives its noise floor from mag_buf.mean_level and mean_power (demod_2400.c:579-580), so the caller passes
 * both.  (mgpu_demod_mag_buf on a mode_ac context is refused with MGPU_E_INVAL rather than decoded without Mode A/C.) */
int mgpu_demod_mag_buf_ac(mgpu_ctx *ctx, const uint16_t *data, uint32_t length,
                          int64_t sampleTimestamp, int64_t sysTimestamp,
                          double mean_level, double mean_power, uint32_t dropped);

/* ---- one capture sharded by buffer ranges over several contexts / GPUs (BASELINE config 5) ----
 * Buffers are independent except for the ICAO filter; the pre-screen needs (a superset of) the addresses the filter may
 * hold: those some clean DF17 / DF11-IID0 frame carried within the last two filter generations (120 s of samples).
 *   the context that owns the capture's FIRST range: mgpu_reset; mgpu_feed_iq*(its samples) as for any stream;
 *   every other range (a context, after mgpu_reset):
 *     pass 1: mgpu_shard_begin(ctx, range_first - 120 s (whole buffers, >= 0), history, 1); mgpu_feed_iq*(those samples up to
 *             range_first); mgpu_adder_bitmap_get()                       -> the addresses that may still be known at range_first
 *     pass 2: mgpu_reset; mgpu_adder_bitmap_set(that); mgpu_shard_begin(ctx, range_first, history, 2);
 *             mgpu_feed_iq*(the range's samples); mgpu_shard_packets()    -> the range's live records
 *   the first context again: mgpu_walk_packets() over the other ranges' packets in stream order, mgpu_finish(),
 *   mgpu_collect(): the message list AND every counter of the unsharded stream, bit for bit.
 * (Any superset of the needed addresses is exact too, e.g. the OR of pass-1 bitmaps over all ranges.)
 * A packet (one per chunk of the shard's range, 8-byte aligned) carries what the walking rank cannot compute without
 * the samples: per live record its would-be signal power and the counts of its would-be skip window, per buffer the
 * converter's level / power sums, per chunk the sweep's candidate tallies.
 * first_sample is a multiple of buf_samples; history = the 326 IQ samples before it (NULL for 0). */
int mgpu_shard_begin(mgpu_ctx *ctx, uint64_t first_sample, const void *history_iq, int mode);
int mgpu_adder_bitmap_get(mgpu_ctx *ctx, uint32_t *words /* 2^19 */);
int mgpu_adder_bitmap_set(mgpu_ctx *ctx, const uint32_t *words /* 2^19 */);
int mgpu_shard_packets(mgpu_ctx *ctx, const void **packets, uint64_t *bytes);   /* valid until the next reset */
int mgpu_walk_packets(mgpu_ctx *ctx, const void *packets, uint64_t bytes);   /* continues the context's stream: the packets' first sample = where it stands */

/* ---- config 5 with the ordered walk itself sharded across the ranks (round 4) ----
 * The form above leaves the ordered walk and the message build of the WHOLE capture to the first rank; this one has every
 * rank walk and build its own range.  What ties the ranges together is the ICAO filter (icao_filter.c:65-130: two generations,
 * `occupied`, the table size with its grow / shrink hysteresis) and the clock of its expiry, which is data-dependent: after a
 * buffer the reference tests Modes.synthetic_now — the timestamp of the buffer's last scored candidate, demod_2400.c:412-414 —
 * against next_flip and re-arms it 60 s after THAT (readsb.c:1227-1231).  Protocol (readsb_amd/shard.py: ShardWalkRank):
 *   1. rank r: mgpu_reset; mgpu_shard_begin(ctx, warmup_first, history, 2); mgpu_feed_iq*(warm-up: the two filter generations
 *      before its range), mgpu_feed_iq*(its range) — two feeds, so that no packet straddles the range's first sample;
 *   2. mgpu_shard_clock_estimate(): its buffers' end clocks, estimated from the records alone; all-gather;
 *      mgpu_flip_schedule() over all buffers' clocks = the expiry schedule;
 *   3. mgpu_shard_walk(): warm-up + range walked with that schedule imposed (rank 0, whose packets start at sample 0: from the
 *      reference's initial state; the others: from an empty filter at the warm-up's first sample), the range's messages built,
 *      its counters kept; out: the range's TRUE end clocks, the filter state at the range's first sample and at its end
 *      (mgpu_shard_state);
 *   4. all-gather clocks and states.  Done iff mgpu_flip_schedule over the true clocks reproduces the schedule and every rank's
 *      state at its first sample equals the state the rank before it ended with (byte-equal blobs).  Otherwise again from 3 with
 *      the new schedule, a rank whose seam failed starting from its predecessor's end state (args.start_state);
 *   5. the last rank: mgpu_finish (the EOF buffer; its clock belongs to the schedule too); every rank: mgpu_collect — its range's
 *      messages and counters.  Integer counters add up over the ranks; nflips is the last rank's; peak_signal_power the maximum;
 *      signal_power_sum / noise_power_sum are sequential double sums in the reference (demod_2400.c:445-479): re-add them in
 *      stream order with mgpu_seqsum_signal_power (over the gathered messages) / mgpu_seqsum (over mgpu_shard_noise_terms).
 * At the fixed point every rank's walk is the serial walk's.  tests/test_gpu_shard.py, tests/test_shard_walk.py. */
struct mgpu_shard_walk_args {
    uint64_t own_first;          /* first sample of the rank's own range (a multiple of buf_samples); packets before it are warm-up */
    const int64_t *flip_after;   /* the imposed expiry schedule: sampleTimestamp (12 MHz ticks = sample * 5) of every buffer of the
                                  * CAPTURE after which the filter expires, ascending */
    uint64_t nflips;
    const void *start_state;     /* NULL: start at the first packet (see 3. above); else the filter state at own_first — the end
                                  * state of the rank before — and the warm-up packets are skipped */
    uint64_t start_state_bytes;
    int32_t check_records;       /* 1: validate every record of the packets (packets that came over a network) */
    int32_t reserved;
};
/* packets == NULL: the context's own (mgpu_shard_packets).  end_clocks[cap]: the range's buffers' end clocks (ms), *n of them. */
int mgpu_shard_clock_estimate(mgpu_ctx *ctx, const void *packets, uint64_t bytes, uint64_t own_first,
                              int64_t *end_clocks, uint64_t cap, uint64_t *n);
int mgpu_shard_walk(mgpu_ctx *ctx, const void *packets, uint64_t bytes, const struct mgpu_shard_walk_args *args,
                    int64_t *end_clocks, uint64_t cap, uint64_t *n);
int mgpu_shard_state(mgpu_ctx *ctx, int which /* 0: at own_first, 1: at the range's end */, const void **blob, uint64_t *bytes);
int mgpu_shard_noise_terms(mgpu_ctx *ctx, const double **terms, uint64_t *n);   /* per buffer of the range: its addend to noise_power_sum */
int mgpu_shard_signal_terms(mgpu_ctx *ctx, const uint64_t **terms, uint64_t *n);   /* per accepted message of the range: sig_sumsq (n = 0 with Mode A/C: use the messages) */
/* The same rank with its pass through the ORDINARY pipeline — ordered walk and message build overlapped with the kernels, as for any
 * stream — for when the schedule is known before the pass (shard.py derives it from a pre-pass over the few buffers around every
 * expiry's possible positions):  mgpu_shard_stream_begin (resets the context; first_sample = the warm-up's first sample, or own_first
 * with start_state) | mgpu_feed_iq*(warm-up) | mgpu_shard_stream_mark (the state at own_first is kept, clocks are logged from
 * there; the warm-up leaves no messages and no statistics) | mgpu_feed_iq*(range) with mgpu_collect as for any stream |
 * mgpu_shard_stream_end -> the range's true end clocks; states by mgpu_shard_state, noise terms by mgpu_shard_noise_terms.
 * Synchronous or DEFERRED feeds (mgpu_set_deferred before _begin): with deferred feeds nothing waits at the mark — the walker marks
 * the range's begin itself when it reaches the range's first chunk, and the range's kernels run while the warm-up is still being
 * walked (one pipeline fill and drain per pass instead of two); every feed call still has its own message list to be collected,
 * the warm-up's are empty.
 * The rounds that follow are those of mgpu_shard_walk; a rank whose premise failed runs its pass again. */
struct mgpu_shard_stream_args {
    uint64_t first_sample;       /* where the pass starts (a multiple of buf_samples) */
    const void *history_iq;      /* the 326 IQ samples before it (NULL for 0) */
    uint64_t own_first;          /* first sample of the rank's own range */
    const int64_t *flip_after;   /* the imposed expiry schedule (as in mgpu_shard_walk_args) */
    uint64_t nflips;
    const void *start_state;     /* NULL, or the filter state at own_first (then first_sample == own_first) */
    uint64_t start_state_bytes;
};
int mgpu_shard_stream_begin(mgpu_ctx *ctx, const struct mgpu_shard_stream_args *args);
int mgpu_shard_stream_mark(mgpu_ctx *ctx);
int mgpu_shard_stream_end(mgpu_ctx *ctx, int64_t *end_clocks, uint64_t cap, uint64_t *n);
/* The expiry schedule from every buffer's end clock, by the reference's rule (readsb.c:1227-1231; filter_clock as in
 * mgpu_config): returns the number of expiries, flip_after[i < cap] = index of the buffer the i-th one follows. */
uint64_t mgpu_flip_schedule(const int64_t *end_clock, uint64_t nbuf, int64_t startup_ms, int filter_clock,
                            uint64_t *flip_after, uint64_t cap);
/* The buffers an expiry of the filter CAN follow, whatever the data (mask[b] = 1; returns how many): what the stream form's pre-pass
 * looks at.  T_k + 60 000 <= T_(k+1) < T_k + 60 111 ms for the clocks T_k the expiries are due at, so the windows widen by 111 ms per
 * expiry: ~6 % of a one-hour capture's buffers. */
uint64_t mgpu_expiry_windows(uint64_t nbuf_total, uint32_t buf_samples, int64_t startup_ms, int filter_clock, uint8_t *mask);
/* What every rank concludes from a round's all-gather (step 4 above; the same on every rank): the schedule the true clocks give
 * (next_sched[cap], *n_next entries), *done = it is the imposed one AND every range's state at its first sample equals the state the
 * range before it ended with; import_from[r] = the rank whose end state rank r has to start its next pass from, or -1.  clocks[r] /
 * nclocks[r]: rank r's end clocks (an empty range: 0 of them; its states are ignored). */
int mgpu_shard_round(const int64_t *sched, uint64_t nsched, uint32_t world, const int64_t *const *clocks, const uint64_t *nclocks,
                     const void *const *state_first, const uint64_t *state_first_bytes, const void *const *state_end, const uint64_t *state_end_bytes,
                     uint64_t nsamples, uint32_t buf_samples, int64_t startup_ms, int filter_clock,
                     int64_t *next_sched, uint64_t cap, uint64_t *n_next, int32_t *import_from, int32_t *done);
double mgpu_seqsum(double start, const double *terms, uint64_t n);                               /* ((start + t0) + t1) + ... */
double mgpu_seqsum_signal_power(double start, const struct mgpu_msg *msgs, uint64_t n);          /* ... of sig_sumsq / 65535^2 */
/* The same sequential sum of the messages' signal powers, prepared by ranges and applied in O(blocks) (readsb_amd/csrc/seqsum.cpp):
 * a block of `block` messages is ONE integer addition on the running sum's mantissa while the sum stays in the binade the block
 * was prepared for (every addition then rounds to the same grid; ties carry the parity of the steps since the tie before).
 * mgpu_seqsum_blocks (every rank, over its own messages): approx_start = roughly what the sum is where the range begins (the
 * earlier ranges' totals, added any which way); out[ceil(n / block)].  mgpu_seqsum_apply (the combining rank, ranges in stream
 * order, start = the exact sum so far): blocks whose premise fails — the sum is not in the predicted binade, or leaves it — are
 * re-added message by message (*fallbacks counts them; may be NULL).  Returns exactly mgpu_seqsum_signal_power(start, msgs, n). */
struct mgpu_sum_block { uint64_t total; int32_t e; uint32_t flags; };
int    mgpu_seqsum_blocks(double approx_start, const struct mgpu_msg *msgs, uint64_t n, uint32_t block, struct mgpu_sum_block *out);
/* the same blocks from the 8-byte numerators of the messages' signal powers (mgpu_shard_signal_terms: one per accepted message of the
 * range, logged by the builder during the pass; none with Mode A/C) instead of from the 64-byte messages — an eighth of the memory read */
int    mgpu_seqsum_blocks_terms(double approx_start, const uint64_t *sumsq, uint64_t n, uint32_t block, struct mgpu_sum_block *out);
double mgpu_seqsum_apply(double start, const struct mgpu_msg *msgs, uint64_t n, uint32_t block, const struct mgpu_sum_block *blocks,
                         uint64_t *fallbacks);

/* ---- beast wire output (modesSendBeastOutput, net_io.c:1655-1714) ------------------------------------
 * Per message: 0x1a, type '2' (56-bit) / '3' (112-bit) / '1' (Mode A/C), the 12 MHz timestamp as 6 bytes
 * big-endian, one signal byte clamp(nearbyint(sqrt(signalLevel) * 255), 1..255), the (corrected) message
 * bytes; every 0x1a payload byte doubled.  Encoded on the GPU.  These two entries write no 0x1a 0xe3 receiverId prefix and
 * the corrected bytes; mgpu_beast_encode_ex* below adds --net-receiver-id and --net-verbatim.
 * _device: d_msgs / d_out are device pointers (e.g. the records an aggregator gathered into its HBM);
 * *bytes = size of the stream; MGPU_E_OVERFLOW (with *bytes set) if it does not fit cap. */
int mgpu_beast_encode_device(mgpu_ctx *ctx, const struct mgpu_msg *d_msgs, uint64_t n, uint8_t *d_out, uint64_t cap, uint64_t *bytes);
int mgpu_beast_encode(mgpu_ctx *ctx, const struct mgpu_msg *msgs, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *bytes);

/* ---- per-message field decode (decodeModesMessage behind the CRC stage, mode_s.c:598-760; decodeExtendedSquitter and
 * its ME decoders, mode_s.c:806-1555; decodeCommB, comm_b.c; decodeModeAMessage, mode_ac.c:171-200) ---------------------------------------
 * One record per message, same index, decoded on the GPU from the corrected frame: the raw Annex-10 fields, altitude,
 * squawk, callsign, velocity, CPR words, the accuracy / operational-status / target-state groups — the members of
 * struct modesMessage (readsb.h:887-1143) under the same names; enums carry the reference's numeric values
 * (addrtype_t readsb.h:178, datasource_t :159, airground_t :216, heading_type_t :239, sil_type_t :224, cpr_type_t :229,
 * nav_modes_t :263, nav_altitude_source_t :287, emergency_t :275, altitude_unit_t :204).  What a memset-0 modesMessage
 * would hold stays 0.  MB/MD/ME/MV are msg[4..10] / msg[1..10] of the message record and are not repeated.
 * DF20/21: decodeCommB's register inference (comm_b.c:52-961) fills commb_format (commb_format_t, readsb.h:249) and the
 * fields of the register it settles on (callsign; selected altitude / QNH / modes; roll, track, ground speed, track
 * rate, TAS; heading, IAS, Mach, vertical rates; the BDS4,4 weather group).  mach is the float the reference stores
 * into its double.  176 bytes. */
struct mgpu_fields {
    uint32_t addr;              /* mm->addr (with MODES_NON_ICAO_ADDRESS = 1<<24 where the ME decode says so) */
    uint32_t AA;
    uint32_t flags;             /* MGPU_F_* */
    uint16_t acc_flags;         /* MGPU_ACC_* */
    uint8_t  nav_flags;         /* MGPU_NAV_* */
    uint8_t  msgtype;           /* DF, 77 = Mode A/C */
    uint8_t  addrtype, source, airground, metype;
    uint8_t  mesub, CA, CC, CF;
    uint8_t  DR, FS, KE, ND;
    uint8_t  RI, SL, UM, VS;
    uint8_t  IID, category, emergency, cpr_type;
    uint16_t AC, ID;
    uint16_t squawkHex, squawkDec;
    int32_t  baro_alt, geom_alt;
    int32_t  geom_delta, baro_rate, geom_rate;
    uint16_t ias, tas;
    float    heading, gs_v0, gs_v2, gs_selected;
    uint32_t cpr_lat, cpr_lon;
    char     callsign[8];
    uint8_t  baro_alt_unit, geom_alt_unit, heading_type, sil_type;
    uint8_t  nac_p, nac_v, sil, gva;
    uint8_t  sda, op_version, op_hrd, op_tah;
    uint16_t op_flags;          /* MGPU_OP_* */
    uint8_t  op_cc_lw, op_cc_antenna_offset;
    uint8_t  op_cc_tc, nav_heading_type, nav_altitude_source, nav_modes;
    uint32_t nav_fms_altitude, nav_mcp_altitude;
    float    nav_qnh, nav_heading;
    float    roll, track_rate, mach;          /* Comm-B BDS5,0 / 6,0 (mm->mach is a double holding this float) */
    float    oat, humidity, wind_direction;   /* Comm-B BDS4,4 */
    uint16_t wind_speed, static_pressure;
    uint8_t  commb_format, met_source, turbulence, pad0;
    uint8_t  reserved[8];
};

/* flags: the bools of struct modesMessage (readsb.h:954-993) */
#define MGPU_F_BARO_ALT_VALID   (1u << 0)
#define MGPU_F_GEOM_ALT_VALID   (1u << 1)
#define MGPU_F_HEADING_VALID    (1u << 2)
#define MGPU_F_GS_VALID         (1u << 3)
#define MGPU_F_IAS_VALID        (1u << 4)
#define MGPU_F_TAS_VALID        (1u << 5)
#define MGPU_F_BARO_RATE_VALID  (1u << 6)
#define MGPU_F_GEOM_RATE_VALID  (1u << 7)
#define MGPU_F_SQUAWK_VALID     (1u << 8)
#define MGPU_F_CALLSIGN_VALID   (1u << 9)
#define MGPU_F_CPR_VALID        (1u << 10)
#define MGPU_F_CPR_ODD          (1u << 11)
#define MGPU_F_CATEGORY_VALID   (1u << 12)
#define MGPU_F_GEOM_DELTA_VALID (1u << 13)
#define MGPU_F_SPI_VALID        (1u << 14)
#define MGPU_F_SPI              (1u << 15)
#define MGPU_F_ALERT_VALID      (1u << 16)
#define MGPU_F_ALERT            (1u << 17)
#define MGPU_F_EMERGENCY_VALID  (1u << 18)
#define MGPU_F_ALT_Q_BIT        (1u << 19)
#define MGPU_F_ACAS_RA_VALID    (1u << 20)
#define MGPU_F_ROLL_VALID       (1u << 21)
#define MGPU_F_TRACK_RATE_VALID (1u << 22)
#define MGPU_F_MACH_VALID       (1u << 23)
#define MGPU_F_WIND_VALID       (1u << 24)
#define MGPU_F_OAT_VALID        (1u << 25)
#define MGPU_F_STATIC_PRESSURE_VALID (1u << 26)
#define MGPU_F_TURBULENCE_VALID (1u << 27)
#define MGPU_F_HUMIDITY_VALID   (1u << 28)
#define MGPU_F_MET_SOURCE_VALID (1u << 29)
/* acc_flags: mm->accuracy (readsb.h:1061-1086) */
#define MGPU_ACC_NIC_A_VALID    (1u << 0)
#define MGPU_ACC_NIC_B_VALID    (1u << 1)
#define MGPU_ACC_NIC_C_VALID    (1u << 2)
#define MGPU_ACC_NIC_BARO_VALID (1u << 3)
#define MGPU_ACC_NAC_P_VALID    (1u << 4)
#define MGPU_ACC_NAC_V_VALID    (1u << 5)
#define MGPU_ACC_GVA_VALID      (1u << 6)
#define MGPU_ACC_SDA_VALID      (1u << 7)
#define MGPU_ACC_NIC_A          (1u << 8)
#define MGPU_ACC_NIC_B          (1u << 9)
#define MGPU_ACC_NIC_C          (1u << 10)
#define MGPU_ACC_NIC_BARO       (1u << 11)
/* nav_flags: mm->nav (readsb.h:1127-1142) */
#define MGPU_NAV_HEADING_VALID  (1u << 0)
#define MGPU_NAV_FMS_ALT_VALID  (1u << 1)
#define MGPU_NAV_MCP_ALT_VALID  (1u << 2)
#define MGPU_NAV_QNH_VALID      (1u << 3)
#define MGPU_NAV_MODES_VALID    (1u << 4)
/* op_flags: the one-bit members of mm->opstatus (readsb.h:1103-1120) */
#define MGPU_OP_VALID       (1u << 0)
#define MGPU_OP_OM_ACAS_RA  (1u << 1)
#define MGPU_OP_OM_IDENT    (1u << 2)
#define MGPU_OP_OM_ATC      (1u << 3)
#define MGPU_OP_OM_SAF      (1u << 4)
#define MGPU_OP_CC_ACAS     (1u << 5)
#define MGPU_OP_CC_CDTI     (1u << 6)
#define MGPU_OP_CC_1090_IN  (1u << 7)
#define MGPU_OP_CC_ARV      (1u << 8)
#define MGPU_OP_CC_TS       (1u << 9)
#define MGPU_OP_CC_UAT_IN   (1u << 10)
#define MGPU_OP_CC_POA      (1u << 11)
#define MGPU_OP_CC_B2_LOW   (1u << 12)
#define MGPU_OP_CC_LW_VALID (1u << 13)

/* msgs / out in host memory (copied through the context's device scratch), or both in device memory. */
int mgpu_decode_fields(mgpu_ctx *ctx, const struct mgpu_msg *msgs, uint64_t n, struct mgpu_fields *out);
int mgpu_decode_fields_device(mgpu_ctx *ctx, const struct mgpu_msg *d_msgs, uint64_t n, struct mgpu_fields *d_out);

/* ---- first stage of the tracker + the forwarding rule --------------------------------------------------------
 * What the reference decides about an accepted message before and around its position tracker, on the device, over the message
 * list: address_reliable (track.c:1688-1693); whether trackUpdateFromMessage finds or creates the message's aircraft and counts it
 * (track.c:1905-1966: aircraftGet / aircraftCreate for reliable addresses only, a->seen, the 45 s rule for the formats whose
 * address is the CRC residue, a->messages++); and outputMessage's rule (net_io.c:5846-5849) over the batch drainMessageBuffer
 * hands it (net_io.c:5924-5940: one sample buffer's messages, cut every 256, all updates before all outputs):
 *     forwarded  <=>  (crc == 0 && correctedbits == 0)  ||  (mm->aircraft && mm->aircraft->messages > 1)  ||  Mode A/C
 * (the beast and raw outputs additionally want correctedbits < 2, net_io.c:5863-5872: the caller's test, it needs nothing from here).
 * The position tracker's checks (the speed / range checks, track.c:423-745; cpr.c itself: mgpu_cpr_track below) stay on the host: when it judges a position
 * message bad or duplicate it puts the aircraft's copy back, a->messages and a->seen with it (track.c:2625-2627), and it deletes
 * aircraft without a reliable position after 5 silent minutes (track.c:2856-2880).  The gate carries both as BOUNDS per aircraft
 * and answers "deferred" exactly where the bounds disagree — in practice inside an aircraft's first two messages only: 0.2 % of a
 * 200-aircraft minute (tests/golden/gate_*.npz: every other verdict equals what the whole reference program forwarded).
 *   verdict[i]: bits 0-1  MGPU_GATE_DROP / _FORWARD / _DEFER;  bit 2  address_reliable;  bit 3  mm->aircraft may be set;
 *               bit 4  mm->aircraft is set for certain.
 * msgs: the accepted messages in netUseMessage order (what mgpu_collect returns), WHOLE sample buffers per call, timestamps on the
 * ifile grid (buffer = (timestamp - 772) / 5 / cfg.buf_samples).  The aircraft table (device memory, 1.25 GiB, allocated by the first
 * call) lives from call to call until mgpu_track_gate_reset / mgpu_destroy.
 * Long streams: removeStaleRange also deletes an aircraft WITH a reliable position once that position is an hour old (30 minutes:
 * non-ICAO addresses; track.c:2835-2866).  Which position was the last reliable one is the tracker's knowledge, so from an aircraft's
 * first position message + that timeout on, its non-clean messages (repaired bits, Address/Parity formats) are answered DEFER: certain
 * verdicts stay what the reference did however long the stream runs, and an aircraft heard for more than an hour costs the host's
 * tracker its non-clean messages.
 * These entries (and the field decode / beast encoder) run on a stream of their own: they do not wait for chunks a deferred feed has
 * queued.  One context is not thread-safe, and the entries share its staging buffers. */
#define MGPU_GATE_DROP     0
#define MGPU_GATE_FORWARD  1
#define MGPU_GATE_DEFER    2
#define MGPU_GATE_ADDRESS_RELIABLE  4
#define MGPU_GATE_AIRCRAFT_POSSIBLE 8
#define MGPU_GATE_AIRCRAFT_CERTAIN  16
int mgpu_track_gate(mgpu_ctx *ctx, const struct mgpu_msg *msgs, uint64_t n, uint8_t *verdict);                 /* host arrays; decodes the fields it needs itself */
int mgpu_track_gate_device(mgpu_ctx *ctx, const struct mgpu_msg *d_msgs, const struct mgpu_fields *d_fields, uint64_t n, uint8_t *d_verdict);   /* everything in device memory */
int mgpu_track_gate_reset(mgpu_ctx *ctx);

/* The gate applied to the encoder — what an aggregator that only forwards needs of the tracker: the beast stream
 * of the messages the reference forwards FOR CERTAIN (outputMessage, net_io.c:5822-5885: first messages of an aircraft are suppressed
 * unless crc == 0 && correctedbits == 0, :5846-5849), in stream order, and — in stream order too — the list of the messages whose fate
 * is the position tracker's (MGPU_GATE_DEFER): {index in msgs, the offset in the stream its frame would start at}.  The host's tracker
 * settles those few (0.2 % of a 200-aircraft minute), encodes the ones it forwards (mgpu_beast_encode on that handful) and splices them
 * in at their offsets: the result is byte for byte what the whole reference program writes (tests/test_gpu_beast.py against
 * tests/golden/beast_*.bin, written by the program's --dump-beast).
 * flags: MGPU_BEAST_NET_RULE = also the beast / raw NETWORK outputs' test correctedbits < 2 (net_io.c:5863-5872; --net-verbatim
 * lifts it); 0 = the --dump-beast file's rule (no such test).
 * mgpu_beast_encode_gated: msgs in host memory, WHOLE sample buffers per call in netUseMessage order like mgpu_track_gate (it runs the
 * field decode and the gate itself, continuing the context's aircraft table).  _device: messages, verdicts (mgpu_track_gate_device's),
 * stream and list all in device memory.  MGPU_E_OVERFLOW: the stream (*bytes = what it needs) or the list (*ndeferred) does not fit.
 * readsb_amd/host/readsb_gpu_gather.c --forward-only uses it on the gathered records (/root/reference/net_io.c:1655-1714 is what
 * consumes such a stream on the other side). */
struct mgpu_deferred {
    uint64_t index;               /* of the message in msgs */
    uint64_t offset;              /* bytes of certain frames before it: where its frame goes if the tracker forwards it */
};
#define MGPU_BEAST_NET_RULE 1u
int mgpu_beast_encode_gated(mgpu_ctx *ctx, const struct mgpu_msg *msgs, uint64_t n, uint32_t flags, uint8_t *out, uint64_t cap, uint64_t *bytes,
                            struct mgpu_deferred *deferred, uint64_t deferred_cap, uint64_t *ndeferred);
int mgpu_beast_encode_gated_device(mgpu_ctx *ctx, const struct mgpu_msg *d_msgs, const uint8_t *d_verdict, uint64_t n, uint32_t flags,
                                   uint8_t *d_out, uint64_t cap, uint64_t *bytes, struct mgpu_deferred *d_deferred, uint64_t deferred_cap,
                                   uint64_t *ndeferred);

/* The encoder with the aggregator's two options (mgpu_beast_encode_ex*): one sized argument block, so that later options need no new entry.
 *   flags & MGPU_BEAST_VERBATIM (--net-verbatim, net_io.c:1662, 5846, 5863-5869): the payload bytes are raw[] — the frame as sliced —
 *     instead of msg[]; length and type still come from msgbits.  The flag also lifts both forwarding tests (first-message suppression
 *     and correctedbits < 2), so EVERY message of a carried length gets a frame: verdicts, if given, decide nothing, nothing is
 *     deferred (*ndeferred = 0), and MGPU_BEAST_NET_RULE has no effect.
 *   ids != NULL (--net-receiver-id, modesSendBeastOutput, net_io.c:1667-1680): one receiver id per message (mgpu_merge_by_time* writes
 *     them).  Call a message a CALLER when the reference would call modesSendBeastOutput for it: a frame is due by flags and verdicts.
 *     Before a caller's frame goes the prefix 0x1a 0xe3 + the id as 8 bytes big-endian, every 0x1a among them doubled (10 .. 18 bytes),
 *     iff its id differs from the caller's before it; for the first caller, from *last_id (a fresh writer starts at 0, net_io.c:343: id
 *     0 at the start gets no prefix).  On return *last_id is the last caller's id (unchanged without one): a list cut into several calls
 *     with *last_id carried along gives the bytes of one call.  last_id == NULL stands for a fresh writer whose state is dropped.
 *     As in the reference, a caller whose length the format does not carry writes NOTHING, not even a prefix, yet moves the writer's id
 *     (the assignment at :1670 precedes the return at :1690 that skips completeWrite): the next frame of that same id has no prefix.
 *   verdict (NULL: every message is a caller), flags & MGPU_BEAST_NET_RULE, deferred / deferred_cap / ndeferred: as in
 *     mgpu_beast_encode_gated_device; ndeferred may be NULL without verdicts.  Unlike mgpu_beast_encode_gated the host-array form takes
 *     the verdicts from the caller (mgpu_track_gate's), it does not run the gate.
 *   ids together with MGPU_GATE_DEFER verdicts: a deferred message is not a caller.  It is listed as ever — index, and the offset at
 *     which its frame (prefix first) would start — and the stream is exact for "every deferred message dropped".  A host that forwards a
 *     deferred message cannot just splice its frame in: the prefixes behind it depend on it.  It has to encode again from that message
 *     on with the verdict settled (MGPU_GATE_FORWARD), *last_id = the id of the last caller before it.
 * With ids == NULL and without MGPU_BEAST_VERBATIM the result is that of the four entries above, which are thin calls into these.
 * args->size = sizeof(struct mgpu_beast_args) of the caller's header (MGPU_E_INVAL if smaller than this library knows fields for).
 * _device: msgs, verdict, ids, out and deferred are device pointers; last_id, bytes and ndeferred are host pointers in both forms. */
#define MGPU_BEAST_VERBATIM 2u
struct mgpu_beast_args {
    uint32_t size;                     /* sizeof(struct mgpu_beast_args) */
    uint32_t flags;                    /* MGPU_BEAST_NET_RULE | MGPU_BEAST_VERBATIM */
    const struct mgpu_msg *msgs;
    uint64_t n;
    const uint8_t *verdict;            /* [n] or NULL */
    const uint64_t *ids;               /* [n] or NULL */
    uint64_t *last_id;                 /* host, in/out, or NULL */
    uint8_t *out;
    uint64_t cap;
    uint64_t *bytes;                   /* host, out */
    struct mgpu_deferred *deferred;    /* [deferred_cap] or NULL */
    uint64_t deferred_cap;
    uint64_t *ndeferred;               /* host, out; may be NULL without verdicts */
};
int mgpu_beast_encode_ex(mgpu_ctx *ctx, const struct mgpu_beast_args *args);
int mgpu_beast_encode_ex_device(mgpu_ctx *ctx, const struct mgpu_beast_args *args);

/* ---- the aggregator's time merge (kernels/merge.inc) ----------------------------------------------------------------------------
 * nseg message lists (one per receiver) into ONE list ordered by timestamp — compared as a signed 64-bit integer — with equal stamps
 * in input order: lower segment first, then position.  It is numpy's argsort(kind="stable") over the concatenation
 * (readsb_amd/gather.py::merge_by_timestamp), whatever the input: the segments need not be sorted (with Mode A/C a receiver's list is
 * only piecewise ordered).  This is the order a forwarder that merges N receivers writes in, and the per-message ids are what
 * mgpu_beast_encode_ex* needs for --net-receiver-id (the consumer's side: readBeast's 0xe3 case in net_io.c; track.c:318-344, 588-642
 * depend on it).
 *   d_segments[k] / counts[k]: host arrays of nseg device pointers (16-byte aligned) and lengths; empty segments and n = 0 are valid.
 *   segment_ids: host array of nseg ids, or NULL (ids 0).   d_verdict_in: host array of nseg device pointers to the segments' verdict
 *   bytes (an entry may be NULL: zeros), or NULL.
 *   d_out [n] merged records (must not overlap a segment);  optional (NULL: not wanted) d_perm [n] u64 = index of each output record in
 *   the concatenation, d_ids [n] u64 = segment_ids[its segment], d_verdict_out [n] = its verdict byte.
 * Limits: nseg <= 4096 (MGPU_E_INVAL beyond), n = sum of counts <= 2^32 - 1 (MGPU_E_CAPACITY beyond).  24 bytes of scratch per record
 * belong to the context (allocated by the first call, grown on demand, freed by mgpu_destroy).  Runs on the stream the gate and the
 * encoder use.  mgpu_merge_by_time: the same on host arrays (segments[k], verdict_in[k], out, perm, ids, verdict_out in host memory).
 * mgpu_merge_last_passes: the 8-bit digit passes the last merge took (only those up to the highest bit its keys differed in: 0 .. 8). */
int mgpu_merge_by_time_device(mgpu_ctx *ctx, const struct mgpu_msg *const *d_segments, const uint64_t *counts, uint32_t nseg,
                              const uint64_t *segment_ids, const uint8_t *const *d_verdict_in, struct mgpu_msg *d_out, uint64_t *d_perm,
                              uint64_t *d_ids, uint8_t *d_verdict_out);
int mgpu_merge_by_time(mgpu_ctx *ctx, const struct mgpu_msg *const *segments, const uint64_t *counts, uint32_t nseg, const uint64_t *segment_ids,
                       const uint8_t *const *verdict_in, struct mgpu_msg *out, uint64_t *perm, uint64_t *ids, uint8_t *verdict_out);
int mgpu_merge_last_passes(mgpu_ctx *ctx);

/* ---- position decode: CPR pairing and cpr.c over the message list (kernels/cpr.inc) ---------------------------------------------
 * What updatePosition does with a position message before its plausibility checks, on the device, one record per message (same
 * index).  Per position message (MGPU_F_CPR_VALID, DF17 / DF18), in stream order per address (fields.addr & 0x1ffffff):
 *   1. the aircraft's even or odd slot becomes this message's {cpr_lat, cpr_lon, cpr_type, source, sysTimestamp} (accept_cpr,
 *      track.c:1829-1844);
 *   2. max_elapsed = surface (cpr_type == CPR_SURFACE): 50 000 ms if MGPU_F_GS_VALID && gs_selected <= 25, else 25 000
 *      (track.c:1266-1269); airborne: cfg.airborne_max_elapsed_ms, 0 = 10 000, the reference's fallback (track.c:1237);
 *   3. GLOBAL decode (doGlobalCPR's decode, track.c:758-799: decodeCPRsurface / decodeCPRairborne, cpr.c:170-319) iff both slots are
 *      filled, of the same cpr_type and source, and |t_even - t_odd| <= max_elapsed (track.c:1279-1282); fflag = this message is odd;
 *      surface needs cfg.ref_valid (the user location, track.c:763-766), result -1 without it.  0: method GLOBAL; -2: method BAD, no
 *      position; -1 or not attempted: 4;
 *   4. LOCAL decode (doLocalCPR's decode, track.c:862-914: decodeCPRrelative, cpr.c:331-374) relative to the aircraft's last GLOBAL
 *      result of this stage if one exists and now < its time + 10 min (method LOCAL_AIRCRAFT), else if airborne && cfg.ref_valid relative
 *      to the receiver (LOCAL_RECEIVER), else none; a result < 0 gives method NONE.
 * Every other message (Mode A/C, no position, MGPU_F_CPR_VALID clear) gets an all-zero record and touches no state.
 * Differences from the reference, by design — the host's tracker keeps the plausibility checks (speed_check, the greatcircle range
 * limits, accept_data, duplicates: track.c:423-745, 784-792, 813-838, 919-956) and receives a candidate position per message instead
 * of two integers:
 *   - the speed-dependent airborne window (track.c:1239-1246) reads the tracker's a->gs: not here, set airborne_max_elapsed_ms;
 *   - the reference's local decode refers to the tracker's latest ACCEPTED position (a->lat / a->lon, track.c:862-864), which a local
 *     result may have moved; here only GLOBAL results of this stage move the per-aircraft reference;
 *   - the slots never expire on their own (the reference invalidates stale ones elsewhere); the window of rule 3 bounds their age.
 * The arithmetic is the reference's in IEEE double, operation for operation: lat / lon equal cpr.c's bit for bit.
 * The aircraft table (device memory, 2^25 addresses x 64 bytes = 2 GiB, allocated by the first call) lives from call to call until
 * mgpu_cpr_reset / mgpu_destroy: one list cut into several calls gives the same records as one call (but for `partner`, which
 * counts in the call's own list).  Preconditions as for mgpu_track_gate: netUseMessage order, n < 2^32 - 2.  n == 0 is MGPU_OK; a NULL
 * cfg or a non-finite reference location is MGPU_E_INVAL.  The entries run on the stream the gate and the encoder use: they do not
 * wait for queued feeds. */
struct mgpu_cpr_config {
    double   ref_lat, ref_lon;    /* Modes.fUserLat / fUserLon */
    uint32_t ref_valid;           /* Modes.userLocationValid */
    uint32_t airborne_max_elapsed_ms;   /* 0 = 10 000 */
};
#define MGPU_CPR_NONE            0
#define MGPU_CPR_GLOBAL          1
#define MGPU_CPR_LOCAL_RECEIVER  2
#define MGPU_CPR_LOCAL_AIRCRAFT  3
#define MGPU_CPR_BAD             4
#define MGPU_CPR_NOT_TRIED       1            /* global_result / local_result: that decode was not attempted */
#define MGPU_CPR_PARTNER_NONE    0xffffffffu  /* no global decode attempted */
#define MGPU_CPR_PARTNER_EARLIER 0xfffffffeu  /* the other half arrived in an earlier call */
struct mgpu_position {            /* 32 bytes, one per message, same index */
    double   lat, lon;            /* set for GLOBAL / LOCAL_*; 0 otherwise */
    uint32_t partner;             /* index in THIS call's list of the opposite-parity message the global decode used, or MGPU_CPR_PARTNER_* */
    int32_t  partner_dt_ms;       /* this message's sysTimestamp - the partner's (0 without one) */
    int8_t   global_result, local_result;   /* cpr.c's 0 / -1 / -2; MGPU_CPR_NOT_TRIED */
    uint8_t  method;              /* MGPU_CPR_NONE / _GLOBAL / _LOCAL_RECEIVER / _LOCAL_AIRCRAFT / _BAD */
    uint8_t  flags;               /* bit 0 odd, bit 1 surface */
    uint8_t  reserved[4];
};
int mgpu_cpr_track(mgpu_ctx *ctx, const struct mgpu_cpr_config *cfg, const struct mgpu_msg *msgs, uint64_t n, struct mgpu_position *out);   /* host arrays; decodes the fields itself, like mgpu_track_gate */
int mgpu_cpr_track_device(mgpu_ctx *ctx, const struct mgpu_cpr_config *cfg, const struct mgpu_msg *d_msgs, const struct mgpu_fields *d_fields,
                          uint64_t n, struct mgpu_position *d_out);   /* everything in device memory */
int mgpu_cpr_reset(mgpu_ctx *ctx);

/* cpr.c's decoders alone, one case per record (stateless): decodeCPRairborne (cpr.c:170-221), decodeCPRsurface (:223-319),
 * decodeCPRrelative (:331-374) with cprNLFunction (:79-146) behind them. */
struct mgpu_cpr_case {
    double   reflat, reflon;      /* fn 1, 2 */
    int32_t  even_lat, even_lon, odd_lat, odd_lon;   /* fn 2: the message's words in even_* */
    uint8_t  fn;                  /* 0 airborne, 1 surface, 2 relative */
    uint8_t  fflag, surface;      /* surface: fn 2 only */
    uint8_t  pad[5];
};
struct mgpu_cpr_result {
    double   lat, lon;            /* rc < 0: 0 */
    int32_t  rc;                  /* 0 / -1 / -2 as cpr.c returns them */
    int32_t  pad;
};
int mgpu_cpr_decode(mgpu_ctx *ctx, const struct mgpu_cpr_case *cases, uint64_t n, struct mgpu_cpr_result *out);
int mgpu_cpr_decode_device(mgpu_ctx *ctx, const struct mgpu_cpr_case *d_cases, uint64_t n, struct mgpu_cpr_result *d_out);

/* ---- text outputs: BaseStation (SBS) lines and AVR raw lines (kernels/text.inc) ---------------------------------------------------
 * The two other outputs outputMessage (net_io.c:5822-5885) serves from the point the beast stream leaves at, formatted on the device
 * from the records the stages above left in HBM.  Streams, offsets and deferred lists work as in mgpu_beast_encode_ex*: the stream of
 * the lines that are due for certain, in list order; {index, offset its line would start at} for every message whose fate is the host
 * tracker's, in stream order (*ndeferred counts all of them, the first deferred_cap are written; more than deferred_cap is
 * MGPU_E_OVERFLOW); MGPU_E_OVERFLOW with *bytes = what the stream needs when it does not fit cap — nothing at or beyond out + cap is
 * written then (the device form leaves the bytes below cap as they would be, the host form copies nothing).  n == 0 is MGPU_OK.
 * args->size = sizeof of the caller's struct (MGPU_E_INVAL if smaller than this library's).  Host form: every array in host memory.
 * _device: msgs, fields, positions, verdict, geom_delta, out and deferred are device pointers; bytes, ndeferred, nskipped are host
 * pointers in both forms (ndeferred may be NULL without verdicts, nskipped always).  Same stream as the gate and the encoder.
 *
 * mgpu_sbs_encode_ex* replaces modesSendSBSOutput (net_io.c:3184-3404, port 30003), fields 1-22 and "\r\n" as at :3249-3401:
 *   msgType (:3207-3245) from fields.msgtype / metype: DF4/20 5, DF5/21 6, DF0/16 7, DF11 8, DF17/18 by ME type 1-4 1, 5-8 2, 9-18 3,
 *     19 4; every other DF, Mode A/C and ME types 0 / 20-31: no line.  fields.addr as %06X; bit 24 (MODES_NON_ICAO_ADDRESS): no line (:3191).
 *   fields 7, 8: msgs[i].sysTimestamp; fields 9, 10: now_ms, ONE value for the whole call (the reference reads the clock per message).
 *   callsign: fields.callsign up to 8 bytes or its first NUL, iff MGPU_F_CALLSIGN_VALID.  Altitudes and rates as stored, with both
 *     branches of Modes.use_gnss (MGPU_SBS_USE_GNSS) and their H suffixes (:3275-3293, :3317-3333); the aircraft's geom_delta
 *     (trackDataValid(&a->geom_delta_valid)) is geom_delta[i], INT32_MIN or a NULL array = not valid; the sums wrap as 32-bit integers.
 *   gs_selected iff MGPU_F_GS_VALID, heading iff MGPU_F_HEADING_VALID and heading_type == HEADING_GROUND_TRACK (readsb.h:239-242), %.0f.
 *   position: positions[i].lat / lon as %1.6f iff its method is MGPU_CPR_GLOBAL / _LOCAL_RECEIVER / _LOCAL_AIRCRAFT; a NULL array or any
 *     other method: ",,".  By design: the reference prints only positions its tracker accepted, so a host tracker vetoes a candidate by
 *     clearing `method` before the call.
 *   squawk %04d of fields.squawkDec iff MGPU_F_SQUAWK_VALID; override_squawk != -1 (Modes.sbsOverrideSquawk) wins.  Fields 19-22: alert,
 *     emergency by the squawk (squawkHex 0x7500 / 0x7600 / 0x7700, :3366-3372), SPI, airground (AG_GROUND "-1", AG_AIRBORNE "0").
 *   receiverCountMlat, mlatEPU, squawk_emergency_valid and sbs_in are 0 for every demodulated message: those branches do not exist here.
 *     --sbs-reduce, the sbs_out_mlat / _replay / _jaero / _prio writers and net_forward_min_messages are not modelled.
 *   Who gets a line (outputMessage calls the writer with an aircraft, :5854, inside its first-message rule, :5846): verdict == NULL:
 *     every message (a consumer that tracks for itself).  Else with v = verdict[i] (mgpu_track_gate's): due iff (v & 3) == MGPU_GATE_FORWARD
 *     && (v & MGPU_GATE_AIRCRAFT_CERTAIN); deferred iff MGPU_GATE_AIRCRAFT_POSSIBLE and either (v & 3) == MGPU_GATE_DEFER or FORWARD
 *     without _CERTAIN; no line otherwise.  A deferred message is listed only if the format has a line for it.
 *   Domain: a message whose line is due or deferred, but whose sysTimestamp is outside [0, 253402300800000) (years 1970-9999), or whose
 *     float to be printed is not finite or has |x| >= 2^31, or whose position to be printed is not finite or has |lat| > 90 or |lon| > 360,
 *     gets no line, no list entry, and adds one to *nskipped: the reference's 200-byte buffer and gmtime_r are undefined there.  A line
 *     is at most 176 bytes (174 for addresses below 2^25).  now_ms outside the same range is MGPU_E_INVAL.
 *   fields == NULL, host form only: the library decodes the fields itself, as mgpu_track_gate does; _device: MGPU_E_INVAL.
 *   The printf conversions are reproduced exactly, in integer arithmetic: %1.6f and %.0f round the binary value half to even.
 *
 * mgpu_raw_encode_ex* replaces modesSendRawOutput (net_io.c:1837-1863, port 30002): '*', or '@' and 12 hex digits iff MGPU_RAW_MLAT
 *   (Modes.mlat) and timestamp != 0; msgbits / 8 bytes as uppercase hex pairs; ";\n".  The 12 digits are the 12 MOST significant hex
 *   digits of the timestamp as uint64 zero-padded to 12 — what sprintf("@%012" PRIX64) followed by p += 13 leaves (:1848-1850); below
 *   2^48 simply the value.  Only msgbits 16, 56, 112 get a line.  MGPU_RAW_VERBATIM (--net-verbatim): raw[] for msg[], both forwarding
 *   tests lifted, nothing deferred.  MGPU_RAW_NET_RULE: also correctedbits < 2 (:5863).  verdict: MGPU_GATE_FORWARD a line,
 *   MGPU_GATE_DEFER listed, NULL every message (the raw writer needs no aircraft): mgpu_beast_encode_ex's rules without ids. */
#define MGPU_SBS_USE_GNSS  1u
struct mgpu_sbs_args {
    uint32_t size;                     /* sizeof(struct mgpu_sbs_args) */
    uint32_t flags;                    /* MGPU_SBS_USE_GNSS */
    const struct mgpu_msg *msgs;
    const struct mgpu_fields *fields;  /* [n]; NULL (host form): decoded by the library */
    const struct mgpu_position *positions;   /* [n] or NULL */
    const uint8_t *verdict;            /* [n] or NULL */
    const int32_t *geom_delta;         /* [n] or NULL */
    uint64_t n;
    int64_t now_ms;
    int32_t override_squawk;           /* -1: none */
    uint8_t *out;
    uint64_t cap;
    uint64_t *bytes;                   /* host, out */
    struct mgpu_deferred *deferred;    /* [deferred_cap] or NULL */
    uint64_t deferred_cap;
    uint64_t *ndeferred, *nskipped;    /* host, out; may be NULL (ndeferred: without verdicts) */
};
int mgpu_sbs_encode_ex(mgpu_ctx *ctx, const struct mgpu_sbs_args *args);
int mgpu_sbs_encode_ex_device(mgpu_ctx *ctx, const struct mgpu_sbs_args *args);

#define MGPU_RAW_NET_RULE  1u
#define MGPU_RAW_VERBATIM  2u
#define MGPU_RAW_MLAT      4u
struct mgpu_raw_args {
    uint32_t size;                     /* sizeof(struct mgpu_raw_args) */
    uint32_t flags;                    /* MGPU_RAW_* */
    const struct mgpu_msg *msgs;
    const uint8_t *verdict;            /* [n] or NULL */
    uint64_t n;
    uint8_t *out;
    uint64_t cap;
    uint64_t *bytes;                   /* host, out */
    struct mgpu_deferred *deferred;    /* [deferred_cap] or NULL */
    uint64_t deferred_cap;
    uint64_t *ndeferred;               /* host, out; may be NULL without verdicts */
};
int mgpu_raw_encode_ex(mgpu_ctx *ctx, const struct mgpu_raw_args *args);
int mgpu_raw_encode_ex_device(mgpu_ctx *ctx, const struct mgpu_raw_args *args);

/* ---- ASTERIX CAT021 target reports (kernels/asterix.inc) ------------------------------------------------------------------------------
 * mgpu_asterix_encode_ex* replaces modesSendAsterixOutput (net_io.c:2416-2945, --net-asterix-out-port / the asterix_out connector), the
 * fourth writer outputMessage serves, over the same records and with the stream, offset, deferred-list, overflow, n == 0, size and stream
 * rules of mgpu_sbs_encode_ex* above.  A record: the category byte 21, a 16-bit big-endian length, an FSPEC of 4 to 6 bytes with the
 * extension bits set from the back (:2920-2927), the items in the order the reference appends them (NOT the order of the UAP).  The
 * writer is mirrored operation for operation; what looks like a mistake in it is kept:
 *   I021/010 SAC 0, SIC 1 (:2436-2439).  I021/040 (:2441-2459): ATP 3 for fields.addr bit 24, 2 for addrtype ADDR_ADSB_OTHER / _TISB_OTHER /
 *     _ADSR_OTHER; bit 3 iff !MGPU_F_ALT_Q_BIT; one extension 0x40 iff airground == AG_GROUND.
 *   I021/130 (:2462-2480) iff positions[i].method is MGPU_CPR_GLOBAL / _LOCAL_RECEIVER / _LOCAL_AIRCRAFT (the reference's cpr_decoded ||
 *     sbs_pos_valid; a NULL array: no position): (int32_t)(lat / (180 / 2^23)) in double, + 2^24 if negative, three bytes each.
 *   I021/150 (:2501-2513) iff MGPU_F_IAS_VALID or _MACH_VALID: Mach wins, (uint16_t)(mach * 1000) in double (mach is the float the
 *     reference stored into its double), else (uint16_t)(ias / 3600.0 * 16384).  I021/151 (:2516-2520) tas.  I021/080 (:2523-2526) addr.
 *   I021/073 (:2533-2543) iff I021/130's FSPEC bit; I021/075 (:2546-2556) and I021/160 (:2709-2718) iff MGPU_F_GS_VALID and _HEADING_VALID and
 *     heading_type == HEADING_GROUND_TRACK: gs_v0 * 4.5511 and heading * (65536 / 360.0) in double.  I021/077 (:2721-2731) always.
 *     The clocks: now = mstime() and time(NULL) are ONE now_ms for the whole call; midnight = now_ms / 1000 / 86400 * 86400000;
 *     int tsm = sysTimestamp - midnight truncated to 32 bits, + 86400000 if negative, (int)(tsm * 0.128) in double; three bytes.
 *   I021/140 (:2559-2574): geom_alt / 6.25 (UNIT_FEET) or / 20.5053 as int16_t; else iff MGPU_F_GEOM_DELTA_VALID the AIRCRAFT's
 *     baro_alt (ac_baro_alt[i]; NULL: 0, a fresh aircraft) + fields.geom_delta (the sum wraps as a 32-bit integer), / 6.25.
 *   I021/090 (:2576-2601) always: nac_v << 5 ADDED into an unsigned char; cpr_nucp, which nothing in the reference sets, contributes 0;
 *     first extension nic_baro << 7 | sil << 5 (sil_type != SIL_INVALID) | nac_p << 1, second 0x20 (SIL_PER_SAMPLE) | sda << 3 | gva << 1,
 *     each truncated to a byte.  The extensions are tested in bytes[p + 1] and only then p advances: with an empty first extension the
 *     second's bits stand in the first's place.
 *   I021/210 (:2604-2636) iff MGPU_OP_VALID: 2 / 1 / 0 for source SOURCE_ADSB / _ADSR / other — with MGPU_ASTERIX_REMOTE (mm->remote)
 *     for addrtype ADDR_ADSB_ICAO, _ADSB_OTHER / ADDR_ADSR_ICAO, _ADSR_OTHER / other — | (op_version & 7) << 3 (a 3-bit field).
 *   I021/070 (:2639-2647) squawkHex's bits as the reference shifts them.  I021/230 (:2650-2655) (int16_t)(roll * 100), a FLOAT product.
 *   I021/145 (:2658-2665) baro_alt / 25 as integers, or (int)(baro_alt * 3.2808) iff baro_alt_unit == UNIT_METERS.
 *   I021/152 (:2668-2674) iff MGPU_F_HEADING_VALID and heading_type == HEADING_MAGNETIC: (int)(heading * 182.0444) in double.
 *   I021/200 (:2677-2690) iff SPI, alert, emergency or nav modes are valid.  I021/155, /157 (:2693-2706): (int16_t)(rate / 3.125) >> 1.
 *   I021/170 (:2734-2748) callsign through char_to_ais (:212-224) over all 8 bytes (NUL and bytes outside the set: 32).
 *   I021/020 (:2751-2819): with MGPU_F_CATEGORY_VALID and category & 7 != 0 the FSPEC bit is set and the byte written only where the
 *     (tc, ca) pair has a case — otherwise NO byte; category & 7 == 0: a 0 byte; not valid: a 0 byte and the bit iff the AIRCRAFT's
 *     category (ac_category[i]; NULL: 0) is 0.
 *   I021/220 (:2822-2850) iff any of the five BDS4,4 valid flags: wind_speed, (int)wind_direction, (int16_t)(oat * 4), a FLOAT product.
 *   I021/146 (:2853-2867) MCP wins over FMS, (int)altitude / 25.  I021/008 (:2870-2883) iff MGPU_OP_VALID and one of its bits (op_cc_tc & 3).
 *   I021/400 (:2886-2889) the low byte of ids[i] iff ids[i] != 0 (the array mgpu_beast_encode_ex* takes; NULL: absent).
 *   from_mlat and from_tisb are set by nothing in the reference: they suppress no record.  I021/131 and I021/295 are commented out there.
 *   A record is at most 74 bytes (I021/152 excludes I021/075 and /160).  --net-asterix-reduce (reduce_forward is the tracker's), CAT020
 *     and sockets are not modelled.  ASTERIX input: mgpu_asterix_decode*, the section "ASTERIX input" below.
 *   Who gets a record (outputMessage calls the writer inside its first-message rule, :5846, with no aircraft and no correctedbits test,
 *     :5882): mgpu_raw_encode_ex's rule without MGPU_RAW_NET_RULE — verdict == NULL: every message, Mode A/C included; (v & 3) ==
 *     MGPU_GATE_FORWARD a record, MGPU_GATE_DEFER listed as {index, offset}, no record otherwise.
 *   Domain: the reference converts doubles and floats to int, int16_t and uint16_t, undefined in C where the value does not fit.  A
 *     message whose record is due or deferred, but one of whose scaled values to be converted (mach * 1000, roll * 100, baro_alt * 3.2808,
 *     heading * 182.0444, gs_v0 * 4.5511, heading * (65536 / 360.0), wind_direction, oat * 4 — only those of items the record has) is
 *     not finite or has magnitude >= 2^31, or whose position is not finite or has |lat| > 90 or |lon| > 360, gets no record, no list
 *     entry, and adds one to *nskipped.  Inside the domain a narrowing conversion keeps the low bits of the value truncated towards
 *     zero, which is what the reference's x86-64 build does (tests/host_stub/asterix_ref_harness.c is the judge of that).
 *     now_ms outside [0, 253402300800000) is MGPU_E_INVAL; sysTimestamp may be any int64.
 *   fields == NULL, host form only: the library decodes the fields itself; _device: MGPU_E_INVAL.  _device: msgs, fields, positions,
 *     verdict, ids, ac_baro_alt, ac_category, out and deferred are device pointers; bytes, ndeferred, nskipped host pointers. */
#define MGPU_ASTERIX_REMOTE 1u
struct mgpu_asterix_args {
    uint32_t size;                     /* sizeof(struct mgpu_asterix_args) */
    uint32_t flags;                    /* MGPU_ASTERIX_REMOTE */
    const struct mgpu_msg *msgs;
    const struct mgpu_fields *fields;  /* [n]; NULL (host form): decoded by the library */
    const struct mgpu_position *positions;   /* [n] or NULL */
    const uint8_t *verdict;            /* [n] or NULL */
    const uint64_t *ids;               /* [n] or NULL */
    const int32_t *ac_baro_alt;        /* [n] or NULL */
    const uint8_t *ac_category;        /* [n] or NULL */
    uint64_t n;
    int64_t now_ms;
    uint8_t *out;
    uint64_t cap;
    uint64_t *bytes;                   /* host, out */
    struct mgpu_deferred *deferred;    /* [deferred_cap] or NULL */
    uint64_t deferred_cap;
    uint64_t *ndeferred, *nskipped;    /* host, out; may be NULL (ndeferred: without verdicts) */
};
int mgpu_asterix_encode_ex(mgpu_ctx *ctx, const struct mgpu_asterix_args *args);
int mgpu_asterix_encode_ex_device(mgpu_ctx *ctx, const struct mgpu_asterix_args *args);

/* ---- the decoded-message dump (kernels/dump.inc, csrc/dump_format.h) ---------------------------------------------------------------
 * What the reference prints to stdout for every message it hands to the tracker unless --quiet is given: displayModesMessage
 * (mode_s.c:1809-2239, called from track.c:2688-2697), including the line printACASInfoShort adds with a == NULL for DF16 with
 * MGPU_F_ACAS_RA_VALID (json_out.c:443-629).  Streams, offsets, MGPU_E_OVERFLOW (with *bytes = what the stream needs and nothing
 * written at or beyond out + cap), n == 0 and the size check are those of mgpu_sbs_encode_ex*; same stream as the gate and the
 * encoders.  No verdicts: the reference dumps every message.  _device: msgs, fields, reduce_forward, receiver_ids, positions,
 * decoded_nic, decoded_rc, out and deferred are device pointers; bytes, ndeferred, nskipped host pointers in both forms.
 *   The message is one whose members are the two records', under the same names: msg, msgbits, correctedbits, score, timestamp,
 *     sysTimestamp and signalLevel (mgpu_msg_signal_level) from the message record; msgtype (77: Mode A/C) and everything else from the
 *     field record.  reduce_forward (printed as the int8_t it is), receiverId, decoded_nic and decoded_rc are the caller's arrays;
 *     cpr_decoded iff positions[i].method is MGPU_CPR_GLOBAL / _LOCAL_RECEIVER / _LOCAL_AIRCRAFT, cpr_relative iff _LOCAL_*; a NULL
 *     positions array, or any other method: the "CPR decoding:  none" form.  A host tracker vetoes a candidate by clearing `method`.
 *     Members neither record carries are a memset-0 message's: sbs_in, sbs_pos_valid, mlatEPU, geom_alt_derived and decodeResult are
 *     0 ("decode: ok"), maybe_addr is 0 — those branches do not exist here (a field record whose addr is HEX_UNKNOWN prints
 *     " 000000 ?" on its hex line and no address line).  --filter-DF and the debug_* variants are not modelled.
 *   "CRC:" is mm->crc as mode_s.c:466 leaves it: modesChecksum of raw[] after fixDF17msgtype (fields.msgtype == 17 with another DF in
 *     raw[0]: the first five bits become 17), over msgbits bits.
 *   MGPU_DUMP_MLAT: "@%012" PRIX64 prints the WHOLE timestamp (more than 12 digits from 2^48), unlike the raw writer.
 *   Every %...f is reproduced exactly, in integer arithmetic, from the float promoted to double (or the correctly rounded double
 *     quotient: timestamp / 12.0, decoded_rc / 1852.0), rounding half to even on the exact binary value.
 *   Domain — a message that would get a dump but lies outside what the mode prints gets none, no list entry, and adds one to
 *     *nskipped.  MGPU_DUMP_ONLYADDR: no message.  Every other mode: msgbits other than 56 or 112 (16 for msgtype >= 32): the frame
 *     line would read past msg[].  Without MGPU_DUMP_RAW also: sysTimestamp outside [0, 253402300800000), timestamp < 0, sig_len == 0,
 *     a float to be printed (heading, track_rate, roll, gs_selected and gs_v0 / gs_v2 where they differ from it, mach, nav_qnh,
 *     nav_heading, each under its valid flag) that is not finite or has |x| >= 2^31, a position to be printed (MGPU_F_CPR_VALID and a
 *     decoded method) with |lat| > 90 or |lon| > 360 or not finite.  A message that gets no dump because of MGPU_DUMP_QUIET is
 *     counted nowhere.  A dump is at most MGPU_DUMP_MAX = 2599 bytes (proved line by line in dump_format.h).
 *     Why msgbits belongs to the domain: the reference's frame loop prints msgbits / 8 bytes starting at msg[] and so runs on into
 *     verbatim[], which these records do not carry, and modesChecksum asserts a whole number of at least three bytes.
 *   Deferred — "RSSI: %8.1f" of 10 * log10(signalLevel) is the one transcendental, and no device log10 is the host libm's bit for
 *     bit.  The sign comes from comparing signalLevel with 1.0 (1.0 itself prints 0.0); the magnitude y from the device's double
 *     log10, and with t = |y| * 10 the rounding is certain iff |t - floor(t) - 0.5| >= 2^-20 (both libraries' errors are a few ulp of a value below 150, about 1e-13).
 *     An uncertain message (about two per million) is not formatted: it is listed in `deferred` as {index, offset its dump would
 *     start at} and counted in *ndeferred, with the overflow rule of the SBS list; the stream is exact for "deferred dropped".  The host
 *     formats those with mgpu_dump_format_host — the same formatter compiled for the host, log10 the host's — and splices the text in
 *     at the offset.  Nothing is deferred with MGPU_DUMP_ONLYADDR or _RAW.
 *   fields == NULL, host form only: the library decodes the fields itself; _device: MGPU_E_INVAL. */
#define MGPU_DUMP_MAX 2599      /* bytes of the longest dump */
#define MGPU_DUMP_ONLYADDR 1u   /* Modes.onlyaddr: "%06x\n" of addr and nothing else (mode_s.c:1829-1832) */
#define MGPU_DUMP_RAW      2u   /* Modes.raw: stop after the frame line (:1844-1847) */
#define MGPU_DUMP_MLAT     4u   /* Modes.mlat: '@' + timestamp instead of '*' when timestamp != 0 (:1835-1839) */
#define MGPU_DUMP_QUIET    8u   /* Modes.quiet: only messages whose fields.addr == show_only get a dump (track.c:2688-2690) */
struct mgpu_dump_args {
    uint32_t size, flags;                    /* sizeof(struct mgpu_dump_args); MGPU_DUMP_* */
    const struct mgpu_msg *msgs;
    const struct mgpu_fields *fields;        /* [n]; NULL (host form only): decoded by the library */
    const uint8_t *reduce_forward;           /* [n] or NULL = 0: mm->reduce_forward, the host tracker's */
    const uint64_t *receiver_ids;            /* [n] or NULL = 0: mm->receiverId (the "receiverId:" line, sprint_uuid1) */
    const struct mgpu_position *positions;   /* [n] or NULL: cpr_decoded iff method GLOBAL / LOCAL_*; cpr_relative iff LOCAL_* */
    const uint8_t  *decoded_nic;             /* [n] or NULL = 0 */
    const uint32_t *decoded_rc;              /* [n] or NULL = 0 */
    uint64_t n;
    uint32_t show_only;                      /* with MGPU_DUMP_QUIET */
    uint8_t *out; uint64_t cap; uint64_t *bytes;
    struct mgpu_deferred *deferred; uint64_t deferred_cap;
    uint64_t *ndeferred, *nskipped;          /* host, out; may be NULL */
};
int mgpu_dump_encode_ex(mgpu_ctx *ctx, const struct mgpu_dump_args *args);          /* every array in host memory */
int mgpu_dump_encode_ex_device(mgpu_ctx *ctx, const struct mgpu_dump_args *args);   /* arrays are device pointers; bytes / ndeferred / nskipped host */
/* The dump of message `index` of a HOST-memory view of the same arguments (fields must be given; out, cap, bytes, deferred and the
 * counts are not read), formatted on the host: up to `cap` bytes to `text` (MGPU_DUMP_MAX always suffices), returns the dump's length (0: the message gets none in
 * this mode), or MGPU_E_INVAL.  Needs no context and no GPU. */
int64_t mgpu_dump_format_host(const struct mgpu_dump_args *args, uint64_t index, uint8_t *text, uint64_t cap);

/* ---- snip: strip quiet stretches from a UC8 capture (snipMode, readsb.c:1187-1206; `readsb --snip <level>`, :1581-1583) ----------
 *
 * A sample is two bytes (i, q); it is quiet iff abs(i - 127) < level && abs(q - 127) < level in int arithmetic (:1197) — level <= 0:
 * nothing is quiet, level >= 129: everything is.  A counter c (uint64_t, 0 at the start of a stream, :1194) counts the quiet samples
 * since the last one that was not; a quiet sample is dropped iff c > 32 (MODES_PREAMBLE_SIZE) after counting it (:1198-1199), every
 * other sample is kept, in order, with its bytes (:1203-1204).  A trailing odd byte is the caller's to drop (:1196 reads pairs).
 *   *quiet_run is that c: read before the call, written after it, so that a stream cut into any calls gives the bytes and the final c
 *     of one call.  NULL: a fresh stream (c = 0) whose state is dropped.
 *   The context's format is irrelevant: snip is defined on bytes.  The calls run on the stream of the other synchronous entries and
 *     do not wait for queued feeds.
 *   args->size smaller than sizeof(struct mgpu_snip_args), NULL ctx, args or nout, out overlapping iq: MGPU_E_INVAL.  nsamples == 0:
 *     MGPU_OK, *nout = 0, *quiet_run unchanged.  More kept than cap_samples: MGPU_E_OVERFLOW with *nout = what is needed, nothing
 *     stored at or beyond out + 2 * cap_samples, *quiet_run unchanged.
 *   mgpu_snip: iq and out in host memory; the input goes through the library's device scratch in passes of pass_samples samples
 *     (0: the library's default), so it may be larger than the device's memory.
 *   mgpu_snip_device: iq and out device pointers, iq 16-byte aligned (MGPU_E_INVAL otherwise), out 2-byte aligned — successive calls
 *     can append into one buffer; pass_samples is ignored.  nout and quiet_run are host pointers in both. */
struct mgpu_snip_args {
    uint32_t size;                     /* sizeof(struct mgpu_snip_args) */
    int32_t level;
    const uint8_t *iq;                 /* nsamples x 2 bytes */
    uint64_t nsamples;
    uint8_t *out;                      /* cap_samples x 2 bytes; must not overlap iq */
    uint64_t cap_samples;
    uint64_t *nout;                    /* host, out: samples kept */
    uint64_t *quiet_run;               /* host, in/out: the reference's c; NULL = a fresh stream whose state is dropped */
    uint64_t pass_samples;             /* host form: samples staged per pass; 0 = the library's default */
};
int mgpu_snip(mgpu_ctx *ctx, const struct mgpu_snip_args *args);
int mgpu_snip_device(mgpu_ctx *ctx, const struct mgpu_snip_args *args);

/* ---- UAT input: uat2esnt over a stream of dump978 downlink lines (`--net-uat-in-port`; decodeUatMessage, net_io.c:4334-4372 ->
 *      uat2esnt_convert_message, uat2esnt/uat2esnt.c:823, uat2esnt/uat_decode.c) -----------------------------------------------------
 *
 * text is a byte stream.  A line is the bytes between two '\n'; bytes behind the last '\n' are not consumed: *consumed says how many
 * were, and the caller carries the rest into its next call, as readsb's client buffer does.  Within a line a NUL ends the content
 * (strlen, net_io.c:4337); a trailing '\r' is ordinary content.  Every line gives zero to four DF18 extended squitters, each an AVR
 * line of 45 bytes, "<FF004D4C4155" + two hex digits of the signal byte + 28 hex digits + ";\n", in the reference's order; out gets
 * them in line order.  Per frame, in the same order and optionally: msgs (the record decodeHexMessage + decodeModesMessage leave:
 * timestamp 0xFF004D4C4155, sysTimestamp now_ms, msgtype 18, msgbits 112, correctedbits 0, score 0, phase 0, addr = AA, msg == raw
 * = the frame, sig_sumsq = (257 * sig)^2 with sig_len 1), sig (the signal byte) and line_of (the index of the source line, counted
 * from the start of this call's text); msgs_cap entries each.
 *   With that sig_sumsq mgpu_msg_signal_level differs from the reference's (sig / 255.0)^2 in the last bits for 126 of the 256 byte
 *     values (evaluated on the CPU); the signal byte the beast encoder recomputes from it equals sig for all 256.  The exact byte is
 *     in the sig array.
 *   The signal byte (generate_esnt, uat2esnt.c:684-691) of an ss= / rssi= value in the simple form [+-]?[0-9]{1,3}(\.[0-9])? followed
 *     by ';' or the end of the line — the %.1f dump978 prints — comes from a table the library builds once with the host's sscanf and
 *     libm.  A '-' line with an ss= / rssi= field in another form where the reference's walk reads it, or longer than 256 bytes, is
 *     DEFERRED: nothing is written for it, its index is listed in `deferred` (ascending; *ndeferred of them), and
 *     mgpu_uat_format_host gives its frames, which belong in front of the first frame whose line_of is larger.
 *   A documented departure: a downlink line whose payload has fewer bytes than the decoders of its MDB type read (types 0, 4, 7-10:
 *     17; 3: 27; 1, 2, 5, 6: 31; 11-31: 4) produces nothing and is counted in *nshort; the reference ignores the length
 *     (frame_to_esnt, uat2esnt.c:716) and decodes uninitialised stack.  (A deferred line is not counted, whatever the host finds.)
 *   Not modelled: replayUatMsg (net_io.c:4341); the "ignore the first UAT message of an aircraft for 300 s" rule (:4357-4366), which
 *     belongs to the aircraft table; use_tisb = 0 (the reference never clears it); uplink frames ('+' lines: never any output).
 *   args->size smaller than sizeof(struct mgpu_uat_args), a NULL ctx, args, bytes, consumed, nlines or nframes, text NULL with
 *     nbytes != 0, out NULL with cap != 0, deferred or ndeferred NULL with deferred_cap != 0, out overlapping text: MGPU_E_INVAL.  nbytes == 0: MGPU_OK with zeros.  More text than cap, more frames than msgs_cap (where msgs, sig or line_of
 *     is given) or more deferred lines than deferred_cap: MGPU_E_OVERFLOW with *bytes, *nframes and *ndeferred = what is needed;
 *     nothing is stored at or beyond any capacity.
 *   mgpu_uat_encode: every array in host memory; the text goes through the library's device scratch in passes of pass_bytes bytes
 *     (0: the library's default) cut at line ends, so it may be larger than the device's memory.
 *   mgpu_uat_encode_device: text, out, msgs, sig, line_of device pointers (no alignment asked of any); the counters and the deferred
 *     list are in host memory in both forms.  nbytes < 2^32 * 8192 / 2.  pass_bytes is ignored. */
struct mgpu_uat_args {
    uint32_t size;                     /* sizeof(struct mgpu_uat_args) */
    uint32_t reserved;                 /* 0 */
    const uint8_t *text;
    uint64_t nbytes;
    uint8_t *out;                      /* cap bytes; must not overlap text */
    uint64_t cap;
    struct mgpu_msg *msgs;             /* optional, msgs_cap entries: one record per frame */
    uint8_t *sig;                      /* optional, msgs_cap entries: the signal byte per frame */
    uint64_t *line_of;                 /* optional, msgs_cap entries: the source line per frame */
    uint64_t msgs_cap;
    uint64_t *deferred;                /* host, deferred_cap entries: the indices of the deferred lines */
    uint64_t deferred_cap;
    int64_t now_ms;                    /* the records' sysTimestamp */
    uint64_t *bytes;                   /* host, out: bytes of text written = 45 * *nframes */
    uint64_t *consumed;                /* host, out: bytes of text up to and including the last '\n' */
    uint64_t *nlines;                  /* host, out: lines in them */
    uint64_t *nframes;                 /* host, out */
    uint64_t *nshort;                  /* host, out, optional */
    uint64_t *ndeferred;               /* host, out, optional (required with deferred_cap != 0) */
    uint64_t pass_bytes;               /* host form: bytes staged per pass; 0 = the library's default */
};
int mgpu_uat_encode(mgpu_ctx *ctx, const struct mgpu_uat_args *args);
int mgpu_uat_encode_device(mgpu_ctx *ctx, const struct mgpu_uat_args *args);
/* Line `line_index` of a HOST-memory text (args->text, args->nbytes, args->now_ms; nothing else of args is read), formatted on the
 * host with nothing deferred: up to `cap` bytes of its AVR lines to `text` (180 always suffice), and — where not NULL — its records
 * to msgs[0..4) and its signal byte to *sig.  Returns the number of bytes (45 per frame; 0: the line gives nothing), or MGPU_E_INVAL
 * (args, a line that does not exist).  Needs no context and no GPU. */
int64_t mgpu_uat_format_host(const struct mgpu_uat_args *args, uint64_t line_index, uint8_t *text, uint64_t cap, struct mgpu_msg *msgs, uint8_t *sig);
/* The same for a line given by its bytes (without the '\n'). */
int64_t mgpu_uat_format_line_host(const uint8_t *line, uint64_t len, int64_t now_ms, uint8_t *text, uint64_t cap, struct mgpu_msg *msgs, uint8_t *sig);

/* ---- tables, for known-answer tests against crc.c --------------------------------- */

/* These run on the host (they are how the device tables are built) and need no context. */
uint32_t mgpu_crc_checksum(const uint8_t *msg, int bits);                 /* modesChecksum, crc.c:67 */
/* modesChecksumDiagnose (crc.c:383) for the tables modesChecksumInit(nfix_crc) builds:
 * returns #error bits 0..2 (positions in *bit0,*bit1, -1 = unused), or -1 if uncorrectable */
int mgpu_crc_diagnose(int nfix_crc, uint32_t syndrome, int bits, int *bit0, int *bit1);
int mgpu_crc_table_size(int nfix_crc, int bits);                           /* crctests' table sizes */
/* the 65536-entry UC8 magnitude table (init_uc8_lookup, convert.c:35-62), index I | Q<<8 */
const uint16_t *mgpu_uc8_table(void);

/* ---- diagnostics ------------------------------------------------------------------------------
 * Host-logic self-check, needs no GPU: walks a seeded synthetic record stream (aircraft that appear,
 * go quiet long enough to expire from the ICAO filter, and return) once serially and once as
 * `nsegments` speculative buffer ranges per chunk, and compares every decision, counter and the
 * final filter.  0 = identical, k > 0 = first differing chunk + 1, < 0 = bad arguments.
 * *speculated_permille (may be NULL) = share of chunks whose ranges all committed in the first batch. */
int mgpu_selftest_walk(uint64_t seed, uint32_t nchunks, uint32_t buffers_per_chunk, uint32_t nsegments,
                       uint32_t naircraft, uint32_t *speculated_permille);

/* Which of a node's GPUs a PCI function is — its place among the functions with the same vendor, device id and local CPU list
 * under `pci_devices_dir` (the library reads /sys/bus/pci/devices), by bus address; what the pipeline's threads choose their L3
 * groups by (a container that holds ONE of a node's GPUs sees HIP ordinal 0 whichever it is).  -1 = not found, -2 = bad arguments. */
int mgpu_selftest_device_index(const char *pci_devices_dir, const char *bus_id);

/* Same idea for the walk on the device (below), needs no GPU either: its algorithm restated on the host — every buffer walked on
 * its own against the filter at the start of the chunk plus a table of first adds, iterated (at most max_walks times) until the
 * table reproduces itself, then the premise check — against the serial walk on the same seeded streams.  Chunks that do not
 * settle or whose premises fail are walked serially, as the library does.  0 = identical, k > 0 = first differing chunk + 1.
 * stats (may be NULL): [0] chunks decided by the model, [1] chunks walked serially after all, [2] walks in all, [3] most walks
 * one chunk took. */
int mgpu_selftest_device_walk(uint64_t seed, uint32_t nchunks, uint32_t buffers_per_chunk, uint32_t naircraft,
                              uint32_t max_walks, uint64_t stats[4]);

/* The sharded walk's protocol (mgpu_shard_walk above), needs no GPU: a seeded synthetic record stream of nchunks chunks is dealt
 * to `nranks` ranks in whole chunks; every rank walks warm-up + range (nsegments speculative buffer ranges per chunk, 1 = the
 * serial loop) from an empty filter with the schedule from ESTIMATED end clocks imposed, and the rounds over (schedule, seam
 * states) run as they would with all-gathers in between — against the serial walk of the whole stream: every decision of every
 * chunk, every buffer's end clock, the counts, the final filter state.  front_extra more aircraft transmit during the first 150 s
 * only (the filter's table grows for them and shrinks one size per expiry afterwards: state no warm-up can rebuild, so seams fail
 * and ranks import).  flags bit 0: the first schedule from the buffers' start clocks; bit 1: a deliberately wrong first schedule.
 * 0 = identical, k > 0 = first differing chunk + 1, -2 = the rounds did not settle.  stats (may be NULL): [0] rounds, [1] walks
 * of a range in all, [2] seams that failed in some round, [3] rounds in which the schedule changed, [4] expiries, [5] ranges that
 * ended up starting from an imported state. */
int mgpu_selftest_shard_walk(uint64_t seed, uint32_t nchunks, uint32_t buffers_per_chunk, uint32_t naircraft, uint32_t front_extra,
                             uint32_t nranks, uint32_t nsegments, uint32_t flags, uint64_t stats[6]);

/* The ordered walk on the device (environment MGPU_DEVICE_WALK=1, or =check to run it beside the host walk and compare every
 * decision): out[0] chunks, [1] chunks whose decisions came from the device (check: were compared), [2] chunks the fixed point
 * did not settle on in time, [3] chunks whose premises failed afterwards (the filter table grew, the expiry moved), [4] chunks
 * the walk does not model, [5] walks run in all, [6] differences found (check mode; must be 0), [7] reserved.
 * [2]-[4] are walked on the host. */
int mgpu_debug_device_walk(mgpu_ctx *ctx, uint64_t out[8]);

/* The magnitudes the pipeline's LAST chunk was demodulated from, as they lie in HBM: out[i] = magnitude of the chunk's sample i,
 * i < n <= the chunk's length (MGPU_E_INVAL beyond it, or before any feed).  Since round 6 the pipeline's magnitudes are not
 * mgpu_convert()'s kernels' — for UC8 input they come out of k_sweep_uc8 (converter and sweep in one pass), for SC16 / SC16Q11 out
 * of k_sweep_sc16 — so the exhaustive converter tests (every UC8 byte pair, every 12-bit SC16Q11 pair: convert.c:64-108, 212-250,
 * 329-367) are run against this too (tests/test_gpu_convert.py).  Drains the pipeline first.  Test support: nothing in readsb
 * reads magnitudes back. */
int mgpu_debug_last_magnitudes(mgpu_ctx *ctx, uint16_t *out, uint64_t n);

/* ---- SBS input: BaseStation lines to aircraft records (`--net-sbs-in-port`, the MLAT results port, the JAERO and PRIO ports;
 *      decodeSbsLine, net_io.c:2952-3178, behind readAscii, net_io.c:4599-4641) ------------------------------------------------------
 *
 * text is a byte stream.  Framing as readAscii's (:4607-4631): a line ends at '\n' or at a NUL byte (the reference turns every NUL
 * into '\n' first); bytes behind the last terminator are not consumed: *consumed says how many were, and the caller carries the rest
 * into its next call, as readsb's client buffer does.  One trailing '\r' of a line of two bytes or more is removed before the length
 * is taken (:4627).  Length below 2: a heartbeat, no record, counted nowhere (:2958).  Length below 20 or at least 200: invalid
 * (:2960), counted in *ninvalid.  No line needs more than 201 bytes looked at, so none is deferred for its length.
 *   One record per valid line, in line order, to recs; line_of (optional) gets the index of its source line, counted from the start
 *   of this call's text over every terminated line.  A record holds every member decodeSbsLine leaves in a memset-0 modesMessage,
 *   under the reference's names (struct mgpu_sbs_rec below).
 *   Fields (t[1] .. t[22] of :3002-3006): fewer than 21 commas is invalid; everything behind the 22nd comma is ignored.  t[1] must be
 *     "MSG" (:3009).  t[2] has length 1 (:3012); sbsMsgType is its digit, 0 for any other character (atoi, :3015).  t[5] is six hex
 *     digits of either case (:3017-3030).  Callsign (:3035-3051): strncpy of 9 bytes with byte 8 cleared; NULs up to the first bad
 *     character (not A-Z, 0-9, ' ') become spaces and the loop breaks there, so the bytes behind it stay as copied; all 8 bytes are in
 *     the record whether MGPU_F_CALLSIGN_VALID or not.  baro_alt (:3053-3060) is stored even where the range test (-5000, 100000)
 *     leaves MGPU_F_BARO_ALT_VALID clear.  MGPU_F_GS_VALID iff the float gs_v0 > 0 (:3062-3067).  heading with HEADING_GROUND_TRACK
 *     (:3069-3074).  decoded_lat / decoded_lon only where both tokens are non-empty, MGPU_SBS_POS_VALID iff both values != 0
 *     (:3076-3082).  baro_rate (:3084-3088).  The squawk only if strtol > 0, squawkHex = squawkDec2Hex (:3090-3098, track.h:742).
 *     t[19] (:3100-3111): receiverCountMlat if > 0 and source == SOURCE_MLAT, otherwise "0" / "-1" set the alert.  t[20] (:3114-3129):
 *     mlatEPU, clamped to 65535, if > 0 and SOURCE_MLAT; otherwise the emergency flag, decided by comparing t[21] — not t[20] — with
 *     "0" / "-1" (:3122-3127), exactly as written.  t[21] (:3132-3140): SPI from "1" / "0" only; the "-1" the reference's own writer
 *     prints is not recognised.  t[22] (:3143-3150): matched by prefix, "-1" (AG_GROUND) then "0" (AG_AIRBORNE).
 *   Numbers, exact: the device takes a numeric token in plain form only.  atoi / strtol tokens (t[12], t[17] - t[20]):
 *     [+-]?[0-9]{1,9} up to the token's end.  strtod tokens (t[13] - t[16]): [+-]?[0-9]*(\.[0-9]*)? with at least one digit, at most
 *     15 significant digits behind the leading zeros and at most 22 digits behind the point: the value is M / 10^f with M < 2^53 and
 *     10^f exact, one IEEE double division, which is what glibc's strtod returns; gs_v0 and heading are that double converted to
 *     float, as the reference's assignment does.  A line that would be valid but holds a numeric token the reference parses in any
 *     other form (exponent, blanks, inf, hex, trailing garbage, no digit, too many digits) is DEFERRED: it gets no record, its index
 *     is listed in `deferred` (ascending; *ndeferred of them), and mgpu_sbs_parse_host gives its record with the host's libc; that
 *     record belongs in front of the first record whose line_of is larger.
 *   Not modelled: Modes.receiver_focus (:2956); the debug_garbage log (:3170-3175); the statistics counters
 *     remote_received_basestation_valid / _invalid, which *nrecs (+ the deferred lines) and *ninvalid give.
 *   args->size smaller than sizeof(struct mgpu_sbs_in_args), a NULL ctx, args, consumed, nlines or nrecs, text NULL with nbytes != 0,
 *     recs NULL with recs_cap != 0, deferred or ndeferred NULL with deferred_cap != 0, a source other than SOURCE_SBS (3), SOURCE_MLAT
 *     (4), SOURCE_JAERO (6), SOURCE_PRIO (11) — what `remote - 64` selects, :2970-2991 —: MGPU_E_INVAL.  nbytes == 0: MGPU_OK with
 *     zeros.  More records than recs_cap or more deferred lines than deferred_cap: MGPU_E_OVERFLOW with *nrecs and *ndeferred = what
 *     is needed; nothing is stored at or beyond any capacity.
 *   mgpu_sbs_decode: every array in host memory; the text goes through the library's device scratch in passes of pass_bytes bytes
 *     (0: the library's default) cut at line ends, so it may be larger than the device's memory.
 *   mgpu_sbs_decode_device: text, recs, line_of device pointers (text at any alignment, recs and line_of 8-byte aligned); the
 *     counters and the deferred list are in host memory in both forms.  nbytes < 2^31 * 8192.  pass_bytes is ignored. */
#define MGPU_SBS_POS_VALID        (1u << 0)   /* sbs_pos_valid */
#define MGPU_SBS_EMERGENCY_VALID  (1u << 1)   /* squawk_emergency_valid */
#define MGPU_SBS_EMERGENCY        (1u << 2)   /* squawk_emergency */
#define MGPU_SBS_SOURCE_SBS   3u              /* datasource_t, readsb.h:159-173 */
#define MGPU_SBS_SOURCE_MLAT  4u
#define MGPU_SBS_SOURCE_JAERO 6u
#define MGPU_SBS_SOURCE_PRIO  11u
/* 96 bytes = six 16-byte vectors; no implicit padding, and the reserved members are ZERO: records are compared bytewise. */
struct mgpu_sbs_rec {
    int64_t sysTimestamp;              /* now_ms (:3160) */
    double decoded_lat, decoded_lon;
    uint32_t addr;
    uint32_t flags;                    /* MGPU_F_BARO_ALT_VALID, _GS_VALID, _HEADING_VALID, _BARO_RATE_VALID, _SQUAWK_VALID, _CALLSIGN_VALID,
                                        * _SPI_VALID, _SPI, _ALERT_VALID, _ALERT */
    uint32_t sbs_flags;                /* MGPU_SBS_* */
    int32_t baro_alt, baro_rate;
    float gs_v0, heading;
    uint32_t squawkDec, squawkHex;
    int32_t receiverCountMlat, mlatEPU;
    char callsign[8];
    uint8_t sbsMsgType, source, addrtype, airground;
    uint8_t baro_alt_unit, heading_type;
    uint8_t reserved[14];              /* 0 */
};
#ifdef __cplusplus
static_assert(sizeof(struct mgpu_sbs_rec) == 96, "struct mgpu_sbs_rec");
#else
_Static_assert(sizeof(struct mgpu_sbs_rec) == 96, "struct mgpu_sbs_rec");
#endif
struct mgpu_sbs_in_args {
    uint32_t size;                     /* sizeof(struct mgpu_sbs_in_args) */
    uint32_t source;                   /* MGPU_SBS_SOURCE_* */
    const uint8_t *text;
    uint64_t nbytes;
    int64_t now_ms;                    /* the records' sysTimestamp */
    struct mgpu_sbs_rec *recs;         /* recs_cap entries: one record per valid line */
    uint64_t *line_of;                 /* optional, recs_cap entries: the source line per record */
    uint64_t recs_cap;
    uint64_t *deferred;                /* host, deferred_cap entries: the indices of the deferred lines */
    uint64_t deferred_cap;
    uint64_t *consumed;                /* host, out: bytes of text up to and including the last terminator */
    uint64_t *nlines;                  /* host, out: lines in them */
    uint64_t *nrecs;                   /* host, out */
    uint64_t *ninvalid;                /* host, out, optional */
    uint64_t *ndeferred;               /* host, out, optional (required with deferred_cap != 0) */
    uint64_t pass_bytes;               /* host form: bytes staged per pass; 0 = the library's default */
};
int mgpu_sbs_decode(mgpu_ctx *ctx, const struct mgpu_sbs_in_args *args);
int mgpu_sbs_decode_device(mgpu_ctx *ctx, const struct mgpu_sbs_in_args *args);
/* Line `line_index` of a HOST-memory text (args->text, args->nbytes, args->source, args->now_ms; nothing else of args is read),
 * parsed on the host with every number resolved by the host's strtol and strtod.  Returns 1 with *rec filled, 0 for a line that gives
 * no record (a heartbeat, an invalid line; *rec is zeroed), or MGPU_E_INVAL (args, rec, a line that does not exist).  Needs no
 * context and no GPU. */
int mgpu_sbs_parse_host(const struct mgpu_sbs_in_args *args, uint64_t line_index, struct mgpu_sbs_rec *rec);
/* The same for a line given by its bytes (without the terminator; a trailing '\r' still on it). */
int mgpu_sbs_parse_line_host(const uint8_t *line, uint64_t len, uint32_t source, int64_t now_ms, struct mgpu_sbs_rec *rec);

/* ---- ASTERIX input: CAT021 records to aircraft records (`--net-asterix-in-port`, the asterix_in connector; readAsterix,
 *      net_io.c:4643-4659, in front of decodeAsterixMessage, :1922-2407, with readFspec :1867, readAsterixTime :1884 and
 *      readAsterixHighPrecisionTime :1899; kernels/asterix_in.inc, csrc/asterix_in_format.h) --------------------------------------------
 *
 * data is a byte stream: a chain of length-prefixed records.  Framing as readAsterix's: a record starts at s, the first at 0; its
 * length is (uint16_t)(((signed char) d[s+1] << 8) + (signed char) d[s+2]) — BOTH bytes sign-extended, as the reference's plain
 * `char` arithmetic does on x86-64: a low byte of 0x80 or more takes 256 off, a high byte of 0x80 or more wraps through uint16_t —
 * and the next record starts at s + len, for len 1 or 2 inside this record's own header.  Framing stops at the first of
 *   MGPU_AST_STOP_END       fewer than 3 bytes are left at s, or s + len > nbytes: *consumed = s, the caller carries the rest over.
 *                           DEVIATION: the reference decodes the partial record from whatever its buffer holds behind the data.
 *   MGPU_AST_STOP_ZERO_LEN  len == 0: *consumed = s.  DEVIATION: the reference never leaves its loop on such a record.
 *   MGPU_AST_STOP_CLOSED    a category-21 record without the I021/080 bit (fspec[1] & 0x10): the handler returns -1 and readAsterix
 *                           closes the client (:1946-1949, :4650-4655).  *consumed = s + len; the record counts in *nframes and
 *                           gives no record; nothing behind it is framed.
 * and *stop says which.  *nframes: the frames consumed; those of another category count in *nother and give no record (their FSPEC
 * is not looked at: DEVIATION where the reference's readFspec would run off its allocation, below).
 *   Decode: one record per consumed category-21 frame, in stream order, to recs; frame_of (optional) gets the index of its frame.
 *   The decoder starts at s + 3 and is NOT bounded by len: items that run past the record read the following bytes of the stream, as
 *   the reference does; bytes at or beyond nbytes read as 0 (a harness of the reference must pad its buffer with zeros to agree).
 *   readFspec follows an extension chain of any length into a 192-byte allocation; a chain of more than 191 extension bytes — the
 *   main FSPEC, I021/040, I021/090 or I021/220 — writes outside it.  DEVIATION: such a frame gives no record and counts in
 *   *nundefined, also where MGPU_AST_STOP_CLOSED would otherwise stop at it; so no frame is decided by more than 1 KiB behind its
 *   start.  Bytes 0-4 of the main FSPEC, 0-1 of I021/040 and 0-2 of I021/090 are used.  The items are read in the reference's order
 *   (:1950-2396), not the UAP's, with its skips and conditions: I021/073 + /074 are times only where sbs_pos_valid is set already;
 *   I021/075 + /076 only where ias_valid or mach_valid is; I021/072 only where sysTimestamp is still -1; I021/155, /157, /160 are
 *   skipped with "range exceeded"; an emitter category without a case gives category 0xE0; I021/146 needs the source bits and
 *   alt < 0x1000; I021/210 takes the accuracy members from the I021/090 in front of it, zeros without one; I021/200 ORs 4 into
 *   nav_modes; the callsign is valid iff all 8 characters are A-Z, '-' to '9', ' ' or '@'.  Positions are int32 * (180 / 2^23) and
 *   int32 * (180 / 2^30) in double, the int32 the two's-complement value of the big-endian bytes; mach = raw * 0.001 in double;
 *   ias = (unsigned)(raw * 2^-14 * 3600); gs_v0, heading, roll the double products converted to float; geom_alt, baro_rate,
 *   geom_rate the double products converted to int.
 *   readAsterixTime: every mstime() of a call is now_ms; (int)(raw / .128) — equal to raw * 125 / 16 in integers for every 24-bit
 *   raw, which is what is computed —, midnight = now_ms / 86400000 * 86400000, the previous day where |midnight + t - now_ms| >
 *   43200000.  readAsterixHighPrecisionTime's `(int)(ts / 1000) * 1000` overflows an int; what the reference's x86-64 build does is
 *   written out: ts / 1000 truncated to 32 bits, times 1000 with 32-bit wrap-around, sign-extended to 64 bits; + 1 / - 1 (a
 *   millisecond, as written) for FSI 1 / 2; converted to double, + offset * 2^-27, converted to uint64_t; a sum of 2^64 or more
 *   gives 0.  sysTimestamp still -1 at the end becomes now_ms.
 *   Not in the record, constant: remote = 1, sbs_in = 1, signalLevel = 0, receiverId = the client's.  Not modelled:
 *   Modes.incrementId, the statistics, sockets.
 *   args->size smaller than sizeof(struct mgpu_asterix_in_args), a NULL ctx, args, consumed, nframes, nrecs or stop, data NULL with
 *     nbytes != 0, recs NULL with recs_cap != 0, a source above SOURCE_PRIO (11; the datasource_t `remote - 64` selects,
 *     SOURCE_INDIRECT = 1 below 64), now_ms outside [0, 253402300800000): MGPU_E_INVAL.  nbytes == 0: MGPU_OK with zeros.  More
 *     records than recs_cap: MGPU_E_OVERFLOW with *nrecs = what is needed; nothing is stored at or beyond the capacity.
 *   mgpu_asterix_decode: every array in host memory; the stream goes through the library's device scratch in passes of pass_bytes
 *     bytes (0: the library's default), each framed first and its unconsumed tail carried into the next, so the stream may be larger
 *     than the device's memory.
 *   mgpu_asterix_decode_device: data, recs, frame_of device pointers (data at any alignment, recs 16-byte and frame_of 8-byte
 *     aligned); the counters in host memory in both forms.  pass_bytes is ignored; the framing scratch is about 2.5 bytes per byte. */
#define MGPU_AST_STOP_END      0u
#define MGPU_AST_STOP_ZERO_LEN 1u
#define MGPU_AST_STOP_CLOSED   2u
/* ast_flags: the valid flags mgpu_fields' `flags` has no bit for */
#define MGPU_AST_POS_VALID       (1u << 0)   /* sbs_pos_valid */
#define MGPU_AST_NAC_V_VALID     (1u << 1)
#define MGPU_AST_NAC_P_VALID     (1u << 2)
#define MGPU_AST_GVA_VALID       (1u << 3)
#define MGPU_AST_SDA_VALID       (1u << 4)
#define MGPU_AST_NIC_BARO_VALID  (1u << 5)
#define MGPU_AST_OPSTATUS_VALID  (1u << 6)
#define MGPU_AST_NAV_MODES_VALID (1u << 7)
#define MGPU_AST_MCP_ALT_VALID   (1u << 8)
#define MGPU_AST_FMS_ALT_VALID   (1u << 9)
/* 128 bytes = eight 16-byte vectors; no implicit padding, and the reserved members are ZERO: records are compared bytewise. */
struct mgpu_asterix_rec {
    int64_t sysTimestamp;
    double decoded_lat, decoded_lon, mach;
    uint32_t addr;                     /* with MODES_NON_ICAO_ADDRESS (1 << 24) for ATP 3 or no I021/040 */
    uint32_t flags;                    /* MGPU_F_BARO_ALT_VALID, _GEOM_ALT_VALID, _HEADING_VALID, _GS_VALID, _IAS_VALID, _TAS_VALID, _BARO_RATE_VALID,
                                        * _GEOM_RATE_VALID, _SQUAWK_VALID, _CALLSIGN_VALID, _CATEGORY_VALID, _SPI_VALID, _SPI, _ALERT_VALID, _ALERT,
                                        * _EMERGENCY_VALID, _ALT_Q_BIT, _ROLL_VALID, _MACH_VALID */
    uint32_t ast_flags;                /* MGPU_AST_* */
    int32_t baro_alt, geom_alt, baro_rate, geom_rate;
    uint32_t ias, tas, squawkHex, squawkDec, category, mcp_altitude, fms_altitude;
    float gs_v0, heading, roll;
    char callsign[8];
    uint8_t source, addrtype, airground, emergency, nav_modes, nac_v, nac_p, sil, sil_type, gva, sda, nic_baro, op_version, heading_type,
            baro_alt_unit, geom_alt_unit;
    uint8_t reserved[4];               /* 0 */
};
#ifdef __cplusplus
static_assert(sizeof(struct mgpu_asterix_rec) == 128, "struct mgpu_asterix_rec");
#else
_Static_assert(sizeof(struct mgpu_asterix_rec) == 128, "struct mgpu_asterix_rec");
#endif
struct mgpu_asterix_in_args {
    uint32_t size;                     /* sizeof(struct mgpu_asterix_in_args) */
    uint32_t source;                   /* datasource_t, 0 .. 11: mm->source */
    const uint8_t *data;
    uint64_t nbytes;
    int64_t now_ms;                    /* every mstime() of the call */
    struct mgpu_asterix_rec *recs;     /* recs_cap entries */
    uint64_t *frame_of;                /* optional, recs_cap entries: the frame per record, counted from the start of this call's data */
    uint64_t recs_cap;
    uint64_t pass_bytes;               /* host form: bytes staged per pass; 0 = the library's default */
    uint64_t *consumed;                /* host, out */
    uint64_t *nframes;                 /* host, out */
    uint64_t *nrecs;                   /* host, out */
    uint32_t *stop;                    /* host, out: MGPU_AST_STOP_* */
    uint64_t *nother;                  /* host, out, optional */
    uint64_t *nundefined;              /* host, out, optional */
};
int mgpu_asterix_decode(mgpu_ctx *ctx, const struct mgpu_asterix_in_args *args);
int mgpu_asterix_decode_device(mgpu_ctx *ctx, const struct mgpu_asterix_in_args *args);
/* Frame `frame_index` of a HOST-memory stream (args->data, nbytes, source, now_ms; nothing else of args is read).  Returns 1 with
 * *rec filled, 0 for a consumed frame that gives no record (another category, undefined, the one MGPU_AST_STOP_CLOSED stops at;
 * *rec is zeroed), or MGPU_E_INVAL (args, rec, a frame that is not consumed).  Needs no context and no GPU. */
int mgpu_asterix_parse_host(const struct mgpu_asterix_in_args *args, uint64_t frame_index, struct mgpu_asterix_rec *rec);
/* The same for the record that starts at `offset` (< nbytes), whether or not the chain from 0 reaches it or its length fits. */
int mgpu_asterix_parse_record_host(const uint8_t *data, uint64_t nbytes, uint64_t offset, uint32_t source, int64_t now_ms, struct mgpu_asterix_rec *rec);

/* ---- Raw input: AVR lines to accepted message records (`--net-ri-port`, 30001 by convention; processHexMessage -> decodeHexMessage,
 * net_io.c:4104-4317, behind readAscii, :4599-4641; the front of decodeModesMessage, mode_s.c:443-606, and its icaoFilterAdd,
 * :766-779; kernels/raw_in.inc, raw_in_format.h) ---------------------------------------------------------------------------------
 * A stream of AVR lines — what mgpu_raw_encode_ex and readsb_gpu_fanin --out-prefix write, and the Aerobits form — to the messages
 * decodeHexMessage hands to netUseMessage, the counters it keeps, and the context's ICAO filter moved to where the reference's
 * stands after the stream.
 *   Lines (readAscii :4609-4631): a line ends at '\n' or at a NUL byte; one '\r' in front of the terminator is removed where
 *     `p - 1 > som`.  Bytes behind the last terminator are not consumed.
 *   A line (decodeHexMessage :4116-4262): isspace trimmed on both sides; the Aerobits suffix "(SIGS,SIGQ,TS)" (:4129-4165: strtok_r on
 *     ",", strtol base 10 and 16, the int truncation of after_pps, the second rollback, now * 12e3, signalLevel = fmin(1, (mV/1000)^2));
 *     the ';' (:4173) and length (:4177) checks; the lead characters '<', '@', '%', '*', ':' (:4180-4243) — the 12 timestamp digits
 *     are shifted onto what the suffix left, a non-hex digit contributes -1; the three legal lengths (:4245-4249), Mode A/C only with
 *     cfg.mode_ac (:4251-4254), the hex check (:4256-4262).
 *   The decode (mode_s.c:443-606): the all-zero test, the DF, fixDF17msgtype (:276-301) under cfg.fixDF && cfg.nfix_crc, the length by
 *     DF, the syndrome, per DF modesChecksumDiagnose / modesChecksumFix with the context's tables.  A DF0/4/5/16/20/21/24-31 frame, a
 *     repaired DF11 and a DF17/18 whose repair changed the address are accepted iff their address is in the ICAO filter AS IT STANDS
 *     AT THAT LINE: the filter at the start of the call, plus the clean DF17 and clean DF11-IID-0 lines in front of it (:766-779),
 *     minus what the first growth of the table drops (icaoFilterResize re-inserts the active generation only, icao_filter.c:65-93).
 *     The device resolves that in parallel and exactly; afterwards the context's filter holds the new addresses, in the
 *     reference's order, and the demodulator's pre-screen knows them (as after mgpu_filter_add).  The calls drain the pipeline first.
 *   A record: timestamp as parsed, sysTimestamp = now_ms, score 0, phase 0, correctedbits / msgtype / msgbits after the decode, addr =
 *     AA after the fix for DF11/17/18 and the syndrome otherwise, msg the corrected frame, raw the frame as received.  sig_len 1 and
 *     sig_sumsq = (257 b)^2 with b the beast signal byte the reference would write for mm->signalLevel (the byte of a '<' line; 0
 *     where the line carries no signal); signal_level[] receives mm->signalLevel itself, bit for bit, and is the authority.  A Mode
 *     A/C line gives msgtype 77, msgbits 16, addr = ModeA & 0xFF7F (decodeModeAMessage, mode_ac.c:165-200), like the demodulator's.
 *   line_class (optional): one byte per line of the stream, MGPU_RAW_*, the filter's verdict resolved.
 *   counters: Modes.stats_current.remote_received_modes, _modeac, remote_rejected_unknown_icao, remote_rejected_bad and
 *     remote_accepted[0..2] (:4268-4283), of this call.
 *   Not modelled: what follows in decodeModesMessage for remote messages (the MLAT / SBS / garbage overrides, mode_s.c:781-799, which
 *     follow from timestamp and addr); netUseMessage and beyond.  Departures: an empty line (the reference reads the byte in front of
 *     it, hex[l - 1] with l == 0) and a line longer than 256 bytes are "not a frame".
 *   args->size smaller than sizeof(struct mgpu_raw_in_args), a NULL ctx, args, consumed, nlines, nmsgs or counters, text NULL with
 *     nbytes != 0, msgs NULL with msgs_cap != 0, line_class NULL with line_class_cap != 0, now_ms outside [0, 253402300800000):
 *     MGPU_E_INVAL.  nbytes == 0: MGPU_OK with zeros.  More messages than msgs_cap, or (with line_class) more lines than
 *     line_class_cap: MGPU_E_OVERFLOW with *nmsgs and *nlines = what is needed; nothing is stored at or beyond a capacity and the
 *     filter is left untouched.
 *   mgpu_raw_decode: every array in host memory; the text goes through device scratch in passes of pass_bytes bytes (0: the library's
 *     default) cut at line ends; the filter state carries from pass to pass (and on MGPU_E_OVERFLOW in any pass goes back to where
 *     it stood before the call).  nbytes < 2^32 in this form too: line indices are 32 bits on the device.
 *   mgpu_raw_decode_device: text, msgs, line_of, signal_level, line_class device pointers (text at any alignment; msgs, line_of and
 *     signal_level 8-byte aligned); the counts are in host memory.  nbytes < 2^32.  pass_bytes is ignored. */
#define MGPU_RAW_NONE     0u   /* not a frame: decodeHexMessage returned 0 before the decode */
#define MGPU_RAW_MODEAC   1u   /* a Mode A/C record (accepted) */
#define MGPU_RAW_BAD      2u   /* rejected bad, decodeModesMessage -2 */
#define MGPU_RAW_ACCEPT   3u   /* accepted */
#define MGPU_RAW_COND     4u   /* mgpu_raw_parse_line_host only: accepted iff addr is in the filter */
#define MGPU_RAW_UNKNOWN  5u   /* rejected unknown ICAO, decodeModesMessage -1 */
struct mgpu_raw_in_counters {
    uint64_t remote_received_modes, remote_received_modeac, remote_rejected_unknown_icao, remote_rejected_bad, remote_accepted[3];
};
struct mgpu_raw_in_config {
    uint32_t size;                     /* sizeof(struct mgpu_raw_in_config) */
    int32_t nfix_crc, fixDF;           /* as in struct mgpu_config */
    uint32_t mode_ac;
};
struct mgpu_raw_in_line {              /* 88 bytes */
    struct mgpu_msg msg;               /* zero unless cls is MGPU_RAW_MODEAC, _ACCEPT or _COND */
    double signal_level;
    uint32_t cls;                      /* MGPU_RAW_NONE, _MODEAC, _BAD, _ACCEPT or _COND */
    uint32_t addr;                     /* the address the filter is asked about (_COND) or learns (adder) */
    uint32_t adder;                    /* 1: a clean DF17 or a clean DF11 with IID 0 — icaoFilterAdd(addr), mode_s.c:766-779 */
    uint32_t reserved;                 /* 0 */
};
struct mgpu_raw_in_args {
    uint32_t size, reserved;           /* sizeof(struct mgpu_raw_in_args), 0 */
    const uint8_t *text;
    uint64_t nbytes;
    int64_t now_ms;
    struct mgpu_msg *msgs;             /* msgs_cap entries: the accepted messages in line order */
    uint64_t *line_of;                 /* optional, msgs_cap entries: the source line per message */
    double *signal_level;              /* optional, msgs_cap entries: mm->signalLevel */
    uint64_t msgs_cap;
    uint8_t *line_class;               /* optional, line_class_cap entries: MGPU_RAW_* per line */
    uint64_t line_class_cap;
    uint64_t *consumed, *nlines, *nmsgs;   /* host, out */
    struct mgpu_raw_in_counters *counters;   /* host, out */
    uint64_t pass_bytes;               /* host form: bytes staged per pass; 0 = the library's default */
};
int mgpu_raw_decode(mgpu_ctx *ctx, const struct mgpu_raw_in_args *args);          /* every array in host memory, text staged in passes cut at line ends */
int mgpu_raw_decode_device(mgpu_ctx *ctx, const struct mgpu_raw_in_args *args);   /* text, msgs, line_of, signal_level, line_class device pointers */
/* One line given by its bytes (without the terminator; a trailing '\r' still on it) parsed on the host by the same parser, the CRC
 * tables of cfg->nfix_crc built once per value.  Returns 1 with *out filled (cls != MGPU_RAW_NONE), 0 for a line that is not a
 * frame (*out zeroed), or MGPU_E_INVAL.  Needs no context and no GPU. */
int mgpu_raw_parse_line_host(const uint8_t *line, uint64_t len, int64_t now_ms, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_line *out);

/* ---- Beast input: a binary stream to accepted message records (`--net-bi-port`, the beast_in connectors, sdr_beast.c; readBeast,
 * net_io.c:4737-5018, with decodeBinMessage, :3804-3961, as its read handler; kernels/beast_in.inc, beast_in_format.h) ------------
 * One call is one readBeast over [data, data + nbytes) with remote = 1 and now = now_ms: the stream mgpu_beast_encode_ex* and
 * readsb_gpu_gather --merge write, read back to the struct mgpu_msg records the demodulator and the raw input give, each with the
 * receiver id in force at its frame.  The byte at data[nbytes] counts as 0 (the reference NUL-terminates its client buffer, :5182);
 * nothing at or beyond nbytes is read.
 *   Modelled, quirk for quirk:
 *     garbage up to the next 0x1a, counted in remote_malformed_beast when a 0x1a is found behind it (:4746-4752);
 *     the 0xe3 receiver-id prefix with its own escape loop and eom bookkeeping (:4819-4857): an id byte 0x1a followed by another byte
 *       abandons the prefix with the scan resuming BEHIND that 0x1a; `eom + 2 > eod` is incomplete; with cfg.net_ingest the id is
 *       not taken; behind the id the same iteration goes on only at a 0x1a, and 0xe3 / 0xe8 there are unknown types.
 *       c->receiverId enters as receiver_id_in and leaves as *receiver_id_out;
 *     the type bytes: '1' '2' '3' (2, 7, 14 bytes behind type, six timestamp bytes and a signal byte), '5' (eom = p + 22), 'P' (eom
 *       = p + 4), 'W' (som += 2, counted in ncommands; the ping it may send is not modelled), anything else som += 2 and two bytes
 *       of garbage;
 *     body un-escaping (:4936-4971): `1a 1a` is one byte and extends eom; `1a` and another byte abandons the frame, everything up to
 *       that 0x1a is garbage and scanning resumes at it;
 *     every "incomplete, retry later" break: *consumed is the frame's 0x1a (behind a taken prefix the inner one; the id stays taken);
 *     the tail rule (:5010-5015): more than 256 unconsumed bytes at the end are all garbage and are consumed;
 *     decodeBinMessage for '1' '2' '3': timestamp the six bytes big endian, signalLevel = (b / 255.0)^2 in two double operations,
 *       sysTimestamp = now_ms; Mode A/C with cfg.mode_ac off is counted in remote_received_modeac and dropped (:3825-3831; the raw
 *       input does not count it); then decodeModeAMessage, or the decode and the filter question of the raw input (above), the
 *       filter moved on and the pre-screen taught as there.  A record is what mgpu_raw_decode leaves: raw the bytes as received,
 *       sig_sumsq = (257 b)^2, sig_len 1.  '5' and 'P' frames are framed, classed and located, nothing else.
 *   Stops, as the ASTERIX input reports its stops: *consumed = *stop_off = the stopping frame's 0x1a, *stop says which:
 *     MGPU_BEAST_STOP_SYNTH  0xe8, a synthetic timestamp (all eight bytes there): the reference disconnects without
 *                            --devel=accept_synthetic;
 *     MGPU_BEAST_STOP_UUID   0xe4: read_uuid depends on receiverIdLocked and can step beyond the buffer; once per connection, so the
 *                            host handles it and calls again.  (Behind a taken 0xe3 prefix the id is taken and the stop is the inner 0x1a.)
 *     Only the first stop on the chain from offset 0 counts; the same bytes in a payload or in garbage stop nothing.
 *     MGPU_BEAST_STOP_END otherwise, *stop_off = *consumed.
 *   Not modelled: Modes.receiver_focus, incrementId, ping and rtt rejection, unreasonable_messagerate and receiverCheckBad; the
 *     c->garbage disconnect bookkeeping; handle_radarcape_position and pongReceived; the 'H' type (never framed by readBeast);
 *     netUseMessage and beyond.
 *   Per message, in stream order: msgs, receiver_id (the array mgpu_beast_encode_ex takes as ids), signal_level (optional),
 *     frame_of (optional: the handler call that gave it).  Per handler call (optional, frames_cap entries): frame_class
 *     (MGPU_BEAST_IN_*) and frame_off (the offset of the frame's 0x1a).
 *   Bounds: a handler call needs 5 bytes, so *nframes <= nbytes / 5 + 1; a message needs 11, so *nmsgs <= nbytes / 11 + 1.
 *   args->size smaller than sizeof(struct mgpu_beast_in_args), a NULL ctx, args, consumed, nframes, nmsgs, stop, stop_off,
 *     receiver_id_out or counters, data NULL with nbytes != 0, msgs or receiver_id NULL with msgs_cap != 0, frame_class and frame_off
 *     both NULL with frames_cap != 0, nbytes >= 2^32, now_ms outside [0, 253402300800000): MGPU_E_INVAL.  nbytes == 0: MGPU_OK
 *     with zeros (and *receiver_id_out = receiver_id_in).  More messages than msgs_cap, or (with frame_class or frame_off) more
 *     handler calls than frames_cap: MGPU_E_OVERFLOW with *nmsgs and *nframes = what is needed; nothing is stored at or beyond a
 *     capacity and the filter goes back to where it stood before the call.  The calls drain the pipeline first.
 *   mgpu_beast_decode: every array in host memory; the stream is staged in passes of pass_bytes (0: the library's default), each cut
 *     at the last som it reached, the remainder, the receiver id and the filter carried, the tail rule applied at the real end only:
 *     exactly the result of one call over the whole stream.
 *   mgpu_beast_decode_device: data, msgs, receiver_id, signal_level, frame_of, frame_class, frame_off device pointers (data at any
 *     alignment; the 8-byte arrays 8-byte aligned); the counts are in host memory.  pass_bytes is ignored. */
#define MGPU_BEAST_IN_MODEAC     1u   /* a Mode A/C record (accepted); the values up to _UNKNOWN are MGPU_RAW_*'s */
#define MGPU_BEAST_IN_BAD        2u   /* rejected bad */
#define MGPU_BEAST_IN_ACCEPT     3u   /* accepted */
#define MGPU_BEAST_IN_COND       4u   /* mgpu_beast_parse_host only: accepted iff addr is in the filter */
#define MGPU_BEAST_IN_UNKNOWN    5u   /* rejected unknown ICAO */
#define MGPU_BEAST_IN_MODEAC_OFF 6u   /* '1' with cfg.mode_ac off: counted, no record */
#define MGPU_BEAST_IN_POSITION   7u   /* '5' */
#define MGPU_BEAST_IN_PONG       8u   /* 'P' */
#define MGPU_BEAST_STOP_END      0u
#define MGPU_BEAST_STOP_SYNTH    1u
#define MGPU_BEAST_STOP_UUID     2u
/* what mgpu_beast_parse_host says of the step at an offset */
#define MGPU_BEAST_STEP_GARBAGE    0u   /* the byte is no 0x1a: one byte of garbage if a 0x1a follows on the chain */
#define MGPU_BEAST_STEP_SKIP       1u   /* an abandoned frame or prefix, a prefix without a frame, 'W', an unknown type */
#define MGPU_BEAST_STEP_FRAME      2u   /* a handler call */
#define MGPU_BEAST_STEP_INCOMPLETE 3u   /* "retry later": next = the som the loop is left with */
#define MGPU_BEAST_STEP_SYNTH      4u
#define MGPU_BEAST_STEP_UUID       5u
struct mgpu_beast_in_counters {
    uint64_t remote_received_modes, remote_received_modeac, remote_rejected_unknown_icao, remote_rejected_bad, remote_accepted[3];
    uint64_t remote_malformed_beast;   /* bytes */
    uint64_t nreceiver_ids;            /* 0xe3 prefixes taken */
    uint64_t ncommands;                /* 'W' commands */
};
struct mgpu_beast_in_config {
    uint32_t size;                     /* sizeof(struct mgpu_beast_in_config) */
    int32_t nfix_crc, fixDF;           /* as in struct mgpu_config */
    uint32_t mode_ac, net_ingest;
    uint32_t reserved;                 /* 0 */
};
struct mgpu_beast_in_frame {           /* 128 bytes */
    struct mgpu_msg msg;               /* zero unless cls is MGPU_BEAST_IN_MODEAC, _ACCEPT or _COND */
    double signal_level;
    uint64_t next;                     /* the successor offset (step INCOMPLETE, SYNTH, UUID: the som the loop is left with) */
    uint64_t frame_off;                /* step FRAME: the frame's 0x1a */
    uint64_t receiver_id;              /* id_set: the id the step leaves in force */
    uint32_t step;                     /* MGPU_BEAST_STEP_* */
    uint32_t cls;                      /* step FRAME: MGPU_BEAST_IN_* (never _UNKNOWN); 0 otherwise */
    uint32_t addr;                     /* the address the filter is asked about (_COND) or learns (adder) */
    uint32_t adder;                    /* 1: a clean DF17 or a clean DF11 with IID 0 — icaoFilterAdd(addr) */
    uint32_t garbage;                  /* bytes of remote_malformed_beast the step adds */
    uint32_t id_set;                   /* 1: a 0xe3 prefix taken */
    uint32_t command;                  /* 1: a 'W' command */
    uint32_t reserved;                 /* 0 */
};
struct mgpu_beast_in_args {
    uint32_t size, reserved;           /* sizeof(struct mgpu_beast_in_args), 0 */
    const uint8_t *data;
    uint64_t nbytes;
    int64_t now_ms;
    uint64_t receiver_id_in;           /* c->receiverId before the call */
    uint32_t net_ingest, reserved2;    /* Modes.netIngest; 0 */
    struct mgpu_msg *msgs;             /* msgs_cap entries: the accepted messages in stream order */
    uint64_t *receiver_id;             /* msgs_cap entries: the id in force at each message's frame */
    double *signal_level;              /* optional, msgs_cap entries: mm->signalLevel */
    uint64_t *frame_of;                /* optional, msgs_cap entries: the handler call per message */
    uint64_t msgs_cap;
    uint8_t *frame_class;              /* optional, frames_cap entries: MGPU_BEAST_IN_* per handler call */
    uint64_t *frame_off;               /* optional, frames_cap entries: the offset of each handler call's 0x1a */
    uint64_t frames_cap;
    uint64_t *consumed, *nframes, *nmsgs;   /* host, out */
    uint32_t *stop;                    /* host, out: MGPU_BEAST_STOP_* */
    uint64_t *stop_off;                /* host, out */
    uint64_t *receiver_id_out;         /* host, out: c->receiverId after the call */
    struct mgpu_beast_in_counters *counters;   /* host, out */
    uint64_t pass_bytes;               /* host form: bytes staged per pass; 0 = the library's default */
};
int mgpu_beast_decode(mgpu_ctx *ctx, const struct mgpu_beast_in_args *args);          /* every array in host memory */
int mgpu_beast_decode_device(mgpu_ctx *ctx, const struct mgpu_beast_in_args *args);   /* data and the per-message / per-call arrays device pointers */
/* The step of readBeast's loop at `offset` of a host buffer, by the same framer and parser (the CRC tables of cfg->nfix_crc built
 * once per value): the successor, the kind, and for a handler call its class, record, signal, the address asked about and the adder
 * flag (MGPU_RAW_COND style).  Returns 1 for a handler call, 0 for any other step, or MGPU_E_INVAL (a NULL argument, offset >=
 * nbytes).  Needs no context and no GPU. */
int mgpu_beast_parse_host(const uint8_t *data, uint64_t nbytes, uint64_t offset, int64_t now_ms, const struct mgpu_beast_in_config *cfg, struct mgpu_beast_in_frame *out);

/* ---- Planefinder input: a DLE-framed binary stream to accepted message records (`--net-pfms-in-port`, the planefinder_in
 * connector; readPlanefinder, net_io.c:4670-4735, with decodePfMessage, :3995-4101, as its read handler and getNextPfUnstuffedByte,
 * :3965-3970; kernels/pf_in.inc, pf_in_format.h) ------------
 * One call is one readPlanefinder over [data, data + nbytes) with now = now_ms.  DLE = 0x10, ETX = 0x03.
 *   The framer, quirk for quirk: from som, memchr finds the next DLE at p.  It is a frame start iff p + 1 < nbytes and data[p + 1] is
 *     neither DLE nor ETX; any other DLE moves som to p + 1 (a DLE in the buffer's last byte is consumed).  From start + 2 the end is
 *     the first q with data[q] == DLE, q + 1 < nbytes and data[q + 1] == ETX (`DLE DLE ETX` in a stuffed body ends the frame at its
 *     second DLE).  Without an end the call returns with som where it stood before this start was found; with one, som = q + 2, and
 *     the handler is called iff data[start + 1] == 0xc1 (any other packet id, the 0x41 of the reference's comment included, is
 *     skipped and counted in nskipped).  A frame has no bounded length.
 *   The handler does not respect the frame's end: it skips the start DLE and reads unstuffed bytes (a DLE is dropped and the byte
 *     behind it taken, whatever it is), at most 53 bytes from the start, through the end marker and the frames behind it if need be:
 *     the id, a padding byte, a type byte t — t & 0xF == 0 Mode A/C with 2 bytes (with cfg.mode_ac off it returns WITHOUT counting:
 *     the beast input counts this case), 1 and 2 Mode S with 7 and 14, anything else returns — a signal byte b with signalLevel =
 *     (b / 255.0)^2 in two double operations, four bytes of seconds and four of nanoseconds, big endian, timestamp = seconds *
 *     1000000000 + nanoseconds, sysTimestamp = now_ms, then the message bytes.  Then decodeModeAMessage, or the decode and the filter
 *     question of the raw input (above), the filter moved on and the pre-screen taught as there.  A record is what mgpu_raw_decode
 *     leaves: raw the bytes as unstuffed, sig_sumsq = (257 b)^2, sig_len 1.  mm->receiverId stays 0: there are no receiver ids.
 *   Reads behind the buffer: every byte at an index >= nbytes reads as 0 (the reference puts a NUL at data[nbytes] and reads what
 *     earlier reads left behind it); nothing at or beyond nbytes is loaded.  counters->past_end counts the handler calls whose decode
 *     read an index > nbytes: for those the result is one of the results the reference can give, not the only one.
 *   A caller that feeds a stream block by block stays exact with args->look: that many bytes at data[nbytes ..) are the stream's too.
 *     They are not framed — only a DLE below nbytes is an event — but they are the lookahead of the DLE in the last byte and what a
 *     handler call reads behind nbytes, and the end that past_end counts against is nbytes + look.  With look >= 53 (or everything
 *     that is left of the stream) and the remainder from *consumed carried, the calls give exactly what one call over the whole
 *     stream gives; *consumed can then be nbytes + 1 (a frame's ETX in data[nbytes]).  readsb_gpu_pf_in.c reads this way.
 *   Not modelled: debug_planefinder, unreasonable_messagerate, receiverCheckBad; netUseMessage and beyond.  Rejected messages leave
 *     no record.
 *   Per message, in stream order: msgs, signal_level (optional), frame_of (optional: the handler call that gave it).  Per handler
 *     call (optional, frames_cap entries): frame_class (MGPU_PF_IN_*) and frame_off (the offset of the frame's start DLE).
 *   Bounds: a handler call needs 4 bytes, so *nframes <= nbytes / 4 and *nmsgs <= *nframes.
 *   args->size smaller than sizeof(struct mgpu_pf_in_args), a NULL ctx, args, consumed, nframes, nmsgs or counters, data NULL with
 *     nbytes != 0, msgs NULL with msgs_cap != 0, frame_class and frame_off both NULL with frames_cap != 0, nbytes + look >= 2^32, now_ms
 *     outside [0, 253402300800000): MGPU_E_INVAL.  nbytes == 0: MGPU_OK with zeros.  More messages than msgs_cap, or (with frame_class
 *     or frame_off) more handler calls than frames_cap: MGPU_E_OVERFLOW with *nmsgs and *nframes = what is needed; nothing is stored
 *     at or beyond a capacity, and the filter and the pre-screen stay where they stood.  The calls drain the pipeline first.
 *   mgpu_pf_decode: every array in host memory; the stream is staged in passes of pass_bytes (0: the library's default) with the 53
 *     bytes behind each, a pass cut at the som it reached (a pass that is not the last judges the DLE in its last byte by the byte
 *     behind it), the remainder and the filter carried, past_end counted against the real end only: exactly the result of one call
 *     over the whole stream.  A frame longer than a pass makes the pass double.
 *   mgpu_pf_decode_device: data, msgs, signal_level, frame_of, frame_class, frame_off device pointers (data at any alignment; the
 *     8-byte arrays 8-byte aligned); the counts are in host memory.  pass_bytes is ignored. */
#define MGPU_PF_IN_MODEAC     1u   /* a Mode A/C record (accepted); the values up to _UNKNOWN are MGPU_RAW_*'s */
#define MGPU_PF_IN_BAD        2u   /* rejected bad */
#define MGPU_PF_IN_ACCEPT     3u   /* accepted */
#define MGPU_PF_IN_COND       4u   /* mgpu_pf_parse_host only: accepted iff addr is in the filter */
#define MGPU_PF_IN_UNKNOWN    5u   /* rejected unknown ICAO */
#define MGPU_PF_IN_MODEAC_OFF 6u   /* Mode A/C with cfg.mode_ac off: no record, nothing counted */
#define MGPU_PF_IN_TYPE       7u   /* a type nibble of 3 to 15: no record, nothing counted */
/* what mgpu_pf_parse_host says of the step at an offset */
#define MGPU_PF_STEP_END        0u   /* no DLE at or behind the offset: the loop ends, som stays */
#define MGPU_PF_STEP_SKIP       1u   /* a DLE that starts no frame: next = its offset + 1 */
#define MGPU_PF_STEP_OTHER      2u   /* a complete frame of another packet id: next = its end + 2 */
#define MGPU_PF_STEP_FRAME      3u   /* a handler call: next = the frame's end + 2 */
#define MGPU_PF_STEP_INCOMPLETE 4u   /* a start without an end: the call returns, som stays */
struct mgpu_pf_in_counters {
    uint64_t remote_received_modes, remote_received_modeac, remote_rejected_unknown_icao, remote_rejected_bad, remote_accepted[3];
    uint64_t nskipped;                 /* complete frames with another packet id */
    uint64_t past_end;                 /* handler calls whose decode read an index > nbytes */
};
struct mgpu_pf_in_frame {              /* 112 bytes */
    struct mgpu_msg msg;               /* zero unless cls is MGPU_PF_IN_MODEAC, _ACCEPT or _COND */
    double signal_level;
    uint64_t next;                     /* the som the step leaves (END, INCOMPLETE: the offset itself) */
    uint64_t frame_off;                /* OTHER, FRAME, INCOMPLETE: the start DLE */
    uint32_t step;                     /* MGPU_PF_STEP_* */
    uint32_t cls;                      /* step FRAME: MGPU_PF_IN_* (never _UNKNOWN); 0 otherwise */
    uint32_t addr;                     /* the address the filter is asked about (_COND) or learns (adder) */
    uint32_t adder;                    /* 1: a clean DF17 or a clean DF11 with IID 0 — icaoFilterAdd(addr) */
    uint32_t past_end;                 /* 1: the decode read an index > nbytes */
    uint32_t reserved;                 /* 0 */
};
struct mgpu_pf_in_args {
    uint32_t size;                     /* sizeof(struct mgpu_pf_in_args) */
    uint32_t look;                     /* bytes at data[nbytes ..) that are the stream's too (see above); 0: nbytes ends the stream */
    const uint8_t *data;
    uint64_t nbytes;
    int64_t now_ms;
    struct mgpu_msg *msgs;             /* msgs_cap entries: the accepted messages in stream order */
    double *signal_level;              /* optional, msgs_cap entries: mm->signalLevel */
    uint64_t *frame_of;                /* optional, msgs_cap entries: the handler call per message */
    uint64_t msgs_cap;
    uint8_t *frame_class;              /* optional, frames_cap entries: MGPU_PF_IN_* per handler call */
    uint64_t *frame_off;               /* optional, frames_cap entries: the offset of each handler call's start DLE */
    uint64_t frames_cap;
    uint64_t *consumed, *nframes, *nmsgs;   /* host, out */
    struct mgpu_pf_in_counters *counters;   /* host, out */
    uint64_t pass_bytes;               /* host form: bytes staged per pass; 0 = the library's default */
};
int mgpu_pf_decode(mgpu_ctx *ctx, const struct mgpu_pf_in_args *args);          /* every array in host memory */
int mgpu_pf_decode_device(mgpu_ctx *ctx, const struct mgpu_pf_in_args *args);   /* data and the per-message / per-call arrays device pointers */
/* The step of readPlanefinder's loop with som at `offset` of a host buffer, by the same framer and parser (cfg: the raw input's;
 * the CRC tables of cfg->nfix_crc built once per value): the som it leaves, the kind, and for a handler call its class, record,
 * signal, the address asked about and the adder flag (MGPU_RAW_COND style).  Returns 1 for a handler call, 0 for any other step, or
 * MGPU_E_INVAL (a NULL argument, offset >= nbytes).  Needs no context and no GPU. */
int mgpu_pf_parse_host(const uint8_t *data, uint64_t nbytes, uint64_t offset, int64_t now_ms, const struct mgpu_raw_in_config *cfg, struct mgpu_pf_in_frame *out);

#ifdef __cplusplus
}
#endif
#endif
