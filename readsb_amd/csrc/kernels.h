// kernels.h — device data layout and kernel launchers of the Mode-S hot path (gfx950).
//
// HBM layout of one feed of n new samples (one context = one stream):
//   d_iq   : raw IQ, n * {2,4} bytes (UC8 / SC16, SC16Q11)
//   d_mag  : u16 magnitudes, the reference's "delayed stream": d_mag[0..326) = the 326
//            samples that preceded this feed (zeros at stream start), d_mag[326 + i] =
//            magnitude of new sample i.  Index D of d_mag is exactly the scan position
//            `pa - m` of demodulate2400 summed over the 131072-sample buffers
//            (demod_2400.c:287-290, sdr_ifile.c:209-213), so D in [0, n) are the preamble
//            start positions and a position reads d_mag[D .. D+289].
//   pool   : PhaseRec[], per-tile chains of segments written by k_slice
//   live   : PhaseRec[], records surviving the pre-screen, globally ordered by (pos, phase)
#pragma once
#ifndef MGPU_EXPERIMENTS
#define MGPU_EXPERIMENTS 0
#endif
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/modes_gpu.h"   // struct mgpu_msg (the beast encoder reads it on the device)
#include "raw_in_format.h"
#include "beast_in_format.h"
#include "pf_in_format.h"

namespace mgpu {

constexpr int kWinPartWords = 8192 * 8;  // k_window_stats: one row of 8 words per workgroup (kWinMaxBlocks rows)
constexpr int kTrailing = 326;          // Modes.trailing_samples (readsb.c:288)
constexpr int kTile = 4096;             // scan positions per LDS tile
constexpr int kHalo = 304;              // >= 290 samples of look-ahead (demod reads pa[0..289]), multiple of 8
constexpr int kTilesPerUnit = 2;
constexpr int kUnit = kTile * kTilesPerUnit;   // positions per unit (one record chain per unit, one wave's share)
constexpr int kBlock = 256;
// k_sweep: positions per candidate list = one of its pre-check steps (16 positions per lane); k_slice's tiles are 2048 = two lists
constexpr int kSweepTile = 1024;
#ifndef MGPU_SL_WGS_PER_CU
#define MGPU_SL_WGS_PER_CU 4
#endif
constexpr int kSweepMaxBlocks = 256 * MGPU_SL_WGS_PER_CU;  // resident workgroups of k_slice (at most 4 per CU)
constexpr int kSweepGridMax = 256 * 8;    // resident workgroups of k_sweep (at most 8 per CU) = rows of sweep_part
constexpr int kDealerCounters = 64;       // k_slice's tile dealer: pools of workgroups, one counter each ...
constexpr int kDealerStride = 64;         // ... 256 bytes apart: device atomics on words of one 64-byte line serialise with each other (tools/micro/atomic_cost.hip)
constexpr int kPoolChunkRecords = 256;    // pool records a wave reserves per returning atomic
constexpr int kSweepMaxWaves = kSweepMaxBlocks * (kBlock / 64);
constexpr uint32_t kNone = 0xFFFFFFFFu;

// flags of a PhaseRec
enum : uint8_t {
    REC_ACCEPT_IF_UNKNOWN = 1,   // decodeModesMessage accepts it even when the address is not in the ICAO filter
    REC_ADDER = 2,               // a clean DF17 / DF11 IID 0: accepted => icaoFilterAdd(addr) (mode_s.c:766-779)
    REC_DFFIX = 4,               // DF repaired to 17 (fixDF17msgtype, mode_s.c:276-301); fixbit0 = DF bit index
    REC_LONG = 8,                // 14 bytes were sliced (else 7)
    REC_CORR_SHIFT = 4,          // bits 4-5: mm->correctedbits decodeModesMessage will report
    REC_COND = 64,               // score_unknown < 0: only alive if the address is (or may become) known
};

// One scored (candidate position, phase) pair whose score is not -2: the filter-independent
// part of score_phase()+scoreModesMessage() (demod_2400.c:215-258, mode_s.c:309-419).
// A record with phase == 0xFF is a segment header: pos = record count, addr = index of the
// next segment header of the same unit (kNone = last).
struct PhaseRec {
    uint32_t pos;            // scan position D within the feed
    uint8_t phase;           // try-phase 4..8
    uint8_t flags;
    int16_t score_known;     // score if `addr` is in the ICAO filter
    int16_t score_unknown;   // score if it is not (-1 = rejected as unknown ICAO)
    uint8_t fixbit0, fixbit1;  // frame bits decodeModesMessage flips (0xFF = none)
    uint32_t addr;           // address the filter is asked about (AA after repair, or the AP syndrome)
    uint8_t msg[14];         // frame as sliced
    uint16_t pad;
};
static_assert(sizeof(PhaseRec) == 32, "PhaseRec must be 32 bytes");
static_assert(sizeof(mgpu_msg) == 64 && sizeof(mgpu_fields) == 176, "C-ABI record sizes");
static_assert(sizeof(mgpu_position) == 32 && sizeof(mgpu_cpr_case) == 40 && sizeof(mgpu_cpr_result) == 24 && sizeof(mgpu_cpr_config) == 24, "C-ABI record sizes");

// counters produced on the device (indices into a u64 array)
enum {
    CNT_CANDIDATES = 0,      // positions with >= 1 phase tried, before any skip-ahead
    CNT_PHASE0 = 1,          // .. CNT_PHASE0+4: score_phase calls per try-phase 4..8, before skip-ahead
    CNT_RECORDS = 6,
    CNT_POOL_OVERFLOW = 7,
    CNT_CLASS_COND = 8,      // candidates whose records are all conditional (REC_COND)
    CNT_CLASS_UNCOND = 9,    // candidates with >= 1 unconditional record
    CNT_DEBUG0 = 16,         // .. 30: the experiments build's checking kernels count what they print here
    CNT_LIVE_TOTAL = 31,     // records surviving the pre-screen (written by k_scan_units)
    CNT_NUM = 32,
};

struct SweepParams {
    const uint16_t *mag;      // d_mag
    uint64_t n;               // number of scan positions (= new samples)
    int32_t thr;              // preamble threshold (demod_2400.c:335-338)
    uint32_t valid_long;      // valid_df_long_bitset  (demod_2400.c:112-128)
    uint32_t valid_short;     // valid_df_short_bitset
    int32_t fix_df;           // Modes.fixDF && Modes.nfix_crc
    const uint32_t *bit_syndrome;   // [112]
    const uint64_t *parity;         // PH[24], PL[24], PS[24]
    const uint32_t *group_syndrome;  // [23][32] long + [12][32] short (tables.h build_group_syndromes)
    const uint64_t *tab_long;       // packed syndrome table for 112-bit frames
    const uint64_t *tab_short;      // packed syndrome table for 56-bit frames
    int32_t n_long, n_short;
    PhaseRec *pool;
    uint32_t pool_cap;
    uint32_t *pool_used;      // device counter (records incl. headers)
    uint32_t *unit_first;     // k_slice: [tiles of 2048 positions] index of the tile's first segment header, kNone if empty
    uint32_t *unit_count;     // k_slice: [tiles] records in the tile's first segment
    uint32_t *dealer;         // k_slice: [kDealerCounters] tiles dealt from each pool so far, kDealerStride words apart (zero at launch); behind them k_sweep: [kDealerCounters] blocks of steps dealt
    uint32_t nunits;
    uint16_t *cand;           // candidate codes (position in the unit << 3 | phase mask), one list per step of kSweepTile positions, kSweepTile slots each
    uint32_t *cand_count;     // [steps], + one empty list behind an odd number of steps
    uint32_t pace_recip;      // k_sweep: 2^32 / reference step time in 10 ns ticks (set by launch_sweep; 0 = no pacing)
    uint32_t *sweep_part;     // [k_slice workgroups][8] partial counters (records, candidates, phases 4/5, 6/7, 8), summed by the pre-screen write pass
    uint32_t *adder_bitmap;   // 2^24 bits: addresses some clean DF17 / DF11 IID 0 frame carries, and those the host added (mgpu_filter_add)
    unsigned long long *counters;   // [CNT_NUM]
    // k_sweep_uc8 (converter and sweep in one; iq == nullptr: k_sweep over the magnitudes in `mag`): the chunk's UC8 samples, the 326
    // magnitudes before the chunk (nullptr: zeros), the 128 x 128 symmetric table (tables.h: UC8_SYM_OFFSET), where the magnitudes
    // go (= mag), the buffers' exact sum(mag) / sum(mag^2) the kernel adds its samples' to (zero at launch), steps per sample buffer
    const uint8_t *iq;
    uint32_t iq_format;       // of `iq`: MGPU_FMT_UC8 (k_sweep_uc8) / SC16 / SC16Q11 (k_sweep_sc16<15 / 11>: 4 bytes per sample, no table, no integer sums)
    const uint16_t *tail;
    const uint16_t *uc8_sym;
    uint16_t *mag_w;
    unsigned long long *sum_level, *sum_power;
    uint32_t buf_steps;
#if MGPU_EXPERIMENTS
    int32_t debug_stage;      // k_slice with one part left out (timing experiments, MGPU_DEBUG_STAGE, tools/slice_stages.sh)
    unsigned long long *dbg_waves;   // k_sweep: [waves][2] start / end of every wave, 100 MHz (tools/micro/sweep_cold.hip), or null
#endif
};

struct ConvertParams {
    const uint8_t *iq;
    uint16_t *mag;            // d_mag (written from index kTrailing on)
    uint64_t n;
    uint32_t buf_samples;
    const uint16_t *tail;           // 326 magnitudes preceding the chunk (device), nullptr = zeros
    const uint16_t *uc8_folded;     // device copy of the folded UC8 table
    unsigned long long *sum_level;  // [nbuffers] UC8: exact integer sum of mag
    unsigned long long *sum_power;  // [nbuffers] UC8: exact integer sum of mag^2
    double *fsum_level;             // [nbuffers] SC16*: sum of mag (0..1), double accumulation
    double *fsum_power;             // [nbuffers] SC16*: sum of magsq
};

void launch_convert(int format, const ConvertParams &p, hipStream_t s);   // UC8: k_convert_uc8_lean where the buffer geometry allows, else k_convert_uc8
void launch_spin(unsigned us, unsigned blocks, unsigned long long *sink, hipStream_t s);   // a kernel that lasts `us` microseconds (event calibration)
// SC16 formats: the per-buffer sequential float sums of mag / magsq (convert.c:225-249), exact; state in and out as doubles holding floats
void launch_fsum_sc16(int format, const uint8_t *iq, uint64_t n, uint32_t buf_samples, double *fsum_level, double *fsum_power, int want_level,
                      hipStream_t s, int fresh = 0);   // fresh: the sums start at zero (else they continue what fsum_* holds)
#if MGPU_EXPERIMENTS
// the same sums for the pipeline's chunks, wide: approximate block sums from the magnitudes -> per-block summaries against predicted
// binades -> a short apply chain per buffer (kernels/convert.inc); scratch = fsum_wide_scratch_bytes()
size_t fsum_wide_scratch_bytes(uint64_t max_samples, uint32_t buf_samples);
void launch_fsum_sc16_wide(int format, const uint8_t *iq, const uint16_t *mag, uint64_t n, uint32_t buf_samples, double *fsum_level, double *fsum_power,
                           int want_level, void *scratch, hipStream_t s);
#endif
unsigned launch_sweep(const SweepParams &p, hipStream_t s);        // k_sweep: preamble sweep -> per-step candidate lists; returns its grid size
void sweep_pace_feedback(float kernel_us, uint64_t n, unsigned blocks, float bracket_us, int fused = 0);   // a timed k_sweep launch: feeds the pacing's step-time estimate
unsigned launch_slice(const SweepParams &p, hipStream_t s);        // k_slice: slicer + CRC + scoring over the candidate lists -> record pool; returns its grid size (rows of sweep_part)
// pre-screen: count / write the records whose address may matter to the ordered walk
// (the write pass also stores each live record's would-be signal power: sum of mag^2 over its frame)
// everything between the sweep and the host: class planes -> class bitmap (+ counters, planes zeroed again),
// pre-screen count / scan / write, scratch block to the host (and zeroed again)
struct PostSweepParams {
    PhaseRec *pool;                       // (the count pass leaves live masks and output offsets in the segment headers)
    uint32_t pool_cap;                    // records the pool holds
    uint32_t variant;                     // bit 1: the write pass by chains (write_unit_chains; else the older one, one chain after the other); bit 2 (experiments build): checking kernels; 3 = the product
    const uint32_t *unit_first;           // first segment header of every chain, chains_per_unit consecutive chains per unit
    const uint32_t *first_count;          // four chains per unit: the records in every chain's first segment (SweepParams::unit_count)
    uint32_t chains_per_unit;             // 4: one chain per k_slice tile of 2048 positions
    uint32_t nunits;
    const uint32_t *adder_bitmap;
    uint32_t *unit_live;                  // live records per unit (count pass)
    uint32_t *block_live;                 // ... per count-pass workgroup (4 units)
    PhaseRec *live;                       // pinned host memory
    const uint16_t *mag;
    unsigned long long *live_sig;         // pinned host memory
    unsigned long long *counters;
    uint32_t *class_final;                // the class bitmap (1 bit per scan position: records, all of them conditional), written by the count pass: kUnit / 32 words per unit
    uint64_t class_words;
    uint32_t *dealer;                     // k_slice's dealer counters: zeroed again by k_publish
    const uint16_t *cand; const uint32_t *cand_count;   // k_sweep's candidate lists of the chunk (the live records' windows are counted from them)
    unsigned long long *live_win;         // shard passes: per live record the packed counts of its would-be skip window (null: not wanted)
    uint64_t n; int32_t thr; uint32_t buf_len;   // ... and what that kernel needs: the chunk's positions, the threshold, the buffer length
    unsigned long long *d_scratch, *h_scratch;
    uint32_t scratch_words;
    uint32_t *fin_part;                   // [count-pass workgroups][2] class counts, summed by the write pass
    const uint32_t *slice_part;           // k_slice's rows of counts (SweepParams::sweep_part), summed by the write pass; slice_blocks = 0: none
    uint32_t slice_blocks;
};
int launch_prescreen(const PostSweepParams &q, hipStream_t s, hipStream_t s_write, hipEvent_t ev_scan);
// ---- Mode A/C (demodulate2400AC, demod_2400.c:575-761), only when mgpu_config.mode_ac is set ----
// A position that passes every test of the reference's loop body: the reply is accepted unless an earlier accepted
// reply of the same buffer hides it (f1_sample += 69, :765) — decided in order on the host.
constexpr int kAcLists = 64;   // k_modeac appends to one of 64 lists (own counter word, own slice of the output)
struct AcCand {
    uint32_t pos;        // scan position D in the chunk (f1_sample = D - buffer start)
    uint32_t f2_clock;   // 60 MHz cycles from the buffer start to the F2 pulse: timestamp = sampleTimestamp + f2_clock / 5 (:755)
    uint32_t modeac;     // 00 A4 A2 A1  00 B4 B2 B1  SPI C4 C2 C1  00 D4 D2 D1 (:731-744)
};
void launch_modeac(const uint16_t *mag, uint64_t n, uint32_t buf_samples, int format, const unsigned long long *sum_level,
                   const unsigned long long *sum_power, const double *fsum_level, const double *fsum_power,
                   uint32_t *noise_level, AcCand *out, uint32_t cap, unsigned long long *list_counts /* [kAcLists], zero */,
                   unsigned long long *counters, hipStream_t s);
// beast wire frames (modesSendBeastOutput, net_io.c:1655-1714) of n message records in device memory; len [n] and
// block_bytes [ceil(n/256)] are scratch; *total (device) receives the number of bytes the frames take
void launch_modeac_scan(const uint16_t *mag, uint64_t n, uint32_t buf_samples, const uint32_t *noise_level, AcCand *out, uint32_t cap,
                        unsigned long long *list_counts, unsigned long long *counters, hipStream_t s);
void launch_decode_fields(const mgpu_msg *msgs, uint64_t n, mgpu_fields *out, const double *roll_tan, hipStream_t s);
void launch_beast_encode(const mgpu_msg *msgs, uint64_t n, uint16_t *meta, uint32_t *block_bytes, unsigned long long *block_off, uint8_t *out,
                         uint64_t cap, unsigned long long *total /* [2]: bytes, deferred */, hipStream_t s, const uint8_t *verdict = nullptr, int net_rule = 0,
                         uint32_t *block_def = nullptr, unsigned long long *block_def_off = nullptr, mgpu_deferred *deferred = nullptr, uint64_t def_cap = 0,
                         int verbatim = 0, const unsigned long long *ids = nullptr /* per message: total[2] = the last caller's */,
                         unsigned long long last_id = 0, void *id_scratch = nullptr /* beast_id_scratch_bytes(n), with ids */);
size_t beast_id_scratch_bytes(uint64_t n);
// the text outputs (kernels/text.inc): SBS lines (modesSendSBSOutput, net_io.c:3184-3404) and AVR raw lines (modesSendRawOutput,
// net_io.c:1837-1863) of n records in device memory.  Everything a job reads is a device pointer; null where modes_gpu.h allows it.
struct TextSbsParams {
    const mgpu_msg *msgs;
    const mgpu_fields *fields;
    const mgpu_position *positions;
    const uint8_t *verdict;
    const int32_t *geom_delta;
    int64_t now_ms;
    int32_t override_squawk;
    uint32_t flags;                   // MGPU_SBS_*
};
struct TextRawParams {
    const mgpu_msg *msgs;
    const uint8_t *verdict;
    uint32_t flags;                   // MGPU_RAW_*
};
struct TextScratch {
    uint16_t *meta;                   // [n] a line's length, or the deferred mark
    uint32_t *blocks;                 // [3 * stride] per workgroup: bytes | deferred messages | skipped messages
    unsigned long long *off;          // [3 * stride] the exclusive prefix sums of the first two
    unsigned long long *total;        // [3] the totals (skipped: SBS and ASTERIX only)
    size_t stride;                    // >= ceil(n / kBlock)
};
void launch_sbs_encode(const TextSbsParams &a, uint64_t n, const TextScratch &w, uint8_t *out, uint64_t cap, mgpu_deferred *deferred, uint64_t def_cap, hipStream_t s);
void launch_raw_encode(const TextRawParams &a, uint64_t n, const TextScratch &w, uint8_t *out, uint64_t cap, mgpu_deferred *deferred, uint64_t def_cap, hipStream_t s);
// ASTERIX CAT021 target reports (kernels/asterix.inc; modesSendAsterixOutput, net_io.c:2416-2945): a third job over the same passes and scratch
struct TextAsterixParams {
    const mgpu_msg *msgs;
    const mgpu_fields *fields;
    const mgpu_position *positions;
    const uint8_t *verdict;
    const unsigned long long *ids;    // the receiver ids of mgpu_merge_by_time
    const int32_t *ac_baro_alt;       // the aircraft's state: a->baro_alt, a->category
    const uint8_t *ac_category;
    int64_t now_ms;
    uint32_t flags;                   // MGPU_ASTERIX_*
};
void launch_asterix_encode(const TextAsterixParams &a, uint64_t n, const TextScratch &w, uint8_t *out, uint64_t cap, mgpu_deferred *deferred, uint64_t def_cap,
                           hipStream_t s);
// the decoded-message dump (kernels/dump.inc; displayModesMessage, mode_s.c:1809-2239): the passes of the text outputs with a write pass of its own
struct DumpParams {
    const mgpu_msg *msgs;
    const mgpu_fields *fields;
    const uint8_t *reduce_forward;    // the five optional arrays: null where modes_gpu.h allows it
    const unsigned long long *receiver_ids;
    const mgpu_position *positions;
    const uint8_t *decoded_nic;
    const uint32_t *decoded_rc;
    uint32_t flags;                   // MGPU_DUMP_*
    uint32_t show_only;
};
struct DumpScratch {
    uint32_t *meta;                   // [n] a dump's length, or the deferred mark
    uint32_t *blocks;                 // [3 * stride] per workgroup: bytes | deferred messages | skipped messages
    unsigned long long *off;          // [3 * stride] the exclusive prefix sums of the first two
    unsigned long long *total;        // [3] the totals
    size_t stride;                    // >= ceil(n / kBlock)
};
void launch_dump_encode(const DumpParams &a, uint64_t n, const DumpScratch &w, uint8_t *out, uint64_t cap, mgpu_deferred *deferred, uint64_t def_cap, hipStream_t s);
// `readsb --snip` over UC8 samples (kernels/snip.inc; snipMode, readsb.c:1187-1206)
constexpr uint64_t kSnipTileSamples = 8192;   // samples per tile of its passes, and per workgroup: consecutive tiles
constexpr uint64_t kSnipGroupSamples = 4 * kSnipTileSamples;
struct SnipScratch {
    unsigned long long *masks;        // [stride * kSnipGroupSamples / 64] the keep masks, a bit per sample
    uint32_t *blocks;                 // [2 * stride] per workgroup: samples kept | 1 + the tile's last loud sample (0: none)
    unsigned long long *off;          // [stride] the exclusive prefix sums of the first
    unsigned long long *total;        // [2] samples kept; 1 + the call's last loud sample (0: none)
    size_t stride;                    // >= ceil(n / kSnipGroupSamples)
};
// iq 16-byte aligned, out 2-byte aligned; quiet_run: the reference's counter before the call; write == false: the counts only
void launch_snip(const uint8_t *iq, uint64_t n, int32_t level, uint64_t quiet_run, const SnipScratch &w, uint8_t *out, uint64_t cap, bool write, hipStream_t s);
// UAT input (kernels/uat.inc; uat2esnt over dump978 downlink lines, uat_format.h): a workgroup per tile of the text
constexpr uint32_t kUatTile = 8192;           // bytes of text per workgroup; a line belongs to the tile that holds its first byte
constexpr uint32_t kUatHalo = 256;            // = kUatDevLineMax: what a line that starts on a tile's last byte may reach into the next
constexpr uint64_t kUatMaxBytes = (uint64_t) kUatTile * 0x7fffffffull;   // a grid's limit
struct UatParams {
    const uint8_t *text;              // any alignment
    uint64_t nbytes;
    const uint8_t *sigtab;            // uat_build_sig_table()
    uint8_t *out;                     // the AVR lines; nothing at or beyond out + cap is stored
    uint64_t cap;
    mgpu_msg *msgs;                   // the three optional per-frame arrays, msgs_cap entries each
    uint8_t *sig;
    unsigned long long *line_of;
    uint64_t msgs_cap;
    unsigned long long *deferred;     // deferred_cap line indices
    uint64_t deferred_cap;
    uint64_t line_base;               // added to every line index (the host form's passes)
    int64_t now_ms;
};
struct UatScratch {
    uint16_t *meta;                   // [stride * kBlock] per lane of a tile: frames of its lines | deferred lines << 8
    uint32_t *blocks;                 // [5 * stride] per tile: newlines | 1 + the last one's offset (0: none) | frames | deferred lines | short lines
    unsigned long long *off;          // [3 * stride] the exclusive prefix sums of newlines, frames, deferred lines
    unsigned long long *total;        // [5] lines, bytes consumed, frames, deferred lines, short lines
    size_t stride;                    // >= ceil(nbytes / kUatTile)
};
void launch_uat_encode(const UatParams &a, const UatScratch &w, hipStream_t s);
// SBS input (kernels/sbs_in.inc; decodeSbsLine over BaseStation lines, sbs_in_format.h): the tiles, the halo and the scratch layout of
// the UAT input; UatScratch's words per lane and per tile count records where it says frames, invalid lines where it says short lines
struct SbsInParams {
    const uint8_t *text;              // any alignment
    uint64_t nbytes;
    mgpu_sbs_rec *recs;               // nothing at or beyond recs + recs_cap is stored
    unsigned long long *line_of;      // optional, recs_cap entries
    uint64_t recs_cap;
    unsigned long long *deferred;     // deferred_cap line indices
    uint64_t deferred_cap;
    uint64_t line_base;               // added to every line index (the host form's passes)
    int64_t now_ms;
    uint32_t source;
};
void launch_sbs_decode(const SbsInParams &a, const UatScratch &w, hipStream_t s);
// Raw input (kernels/raw_in.inc; decodeHexMessage + the front of decodeModesMessage over AVR lines, raw_in_format.h): the tiles, the halo
// and the per-tile scratch of the UAT input (UatScratch's words per lane and per tile count candidates where it says frames), then
// passes over the candidates that settle the ICAO filter's answers in parallel
struct RawInParams {
    const uint8_t *text;              // any alignment
    uint64_t nbytes;
    int64_t now_ms;
    RawInConfig cfg;
    RawInTables tb;                   // device pointers
    mgpu_msg *cand_rec;               // per candidate, in line order: the record, the signal, the line, class | correctedbits | adder | address
    double *cand_sig;
    uint32_t *cand_line, *cand_meta;
    uint64_t cand_cap;
    const uint32_t *gen_active, *gen_inactive;   // 2^24 bits each: the filter's generations at the start of the call
    uint32_t *first;                  // 2^24 words, all ones outside a call: the first adder candidate of an address
    uint32_t *new_adds;               // cand_cap words: the addresses that enter the active generation, in line order
    uint64_t kstar;                   // the new add that makes the table grow (1-based); 0: none can
    mgpu_msg *msgs;                   // nothing at or beyond msgs + msgs_cap is stored
    unsigned long long *line_of;      // optional
    double *signal_level;             // optional
    uint64_t msgs_cap;
    uint8_t *line_class;              // optional: nothing at or beyond line_class + line_class_cap is stored
    uint64_t line_class_cap;
    uint64_t line_base;               // added to every line_of (the host form's passes)
    const unsigned long long *cand_id = nullptr;   // the beast input: per candidate the receiver id in force, and where the accepted
    unsigned long long *receiver_id = nullptr;     // ones' go (msgs_cap entries); both null for the raw input
};
void launch_raw_in_scatter(const uint32_t *members, uint32_t n, uint32_t *bitmap, int set, hipStream_t s);
void launch_raw_in_front(const RawInParams &a, const UatScratch &w, hipStream_t s);
void launch_raw_in_resolve(const RawInParams &a, uint32_t ncand, uint32_t *cb, unsigned long long *co, unsigned long long *misc, hipStream_t s);
// Beast input (kernels/beast_in.inc; readBeast + decodeBinMessage over a binary stream, beast_in_format.h): the UAT input's tiles; a
// step reaches at most 62 bytes, so the chain that passes a tile enters the next at one of its first 64 offsets.  It ends in the raw
// input's candidate arrays and filter passes (RawInParams: a "line" is a handler call)
constexpr uint32_t kBeastInGroup = 64;        // tiles whose exit maps are composed into one
constexpr size_t beast_in_tiles(uint64_t nbytes) { return (size_t) (nbytes / kUatTile + 1); }   // (the chain may end AT nbytes)
constexpr size_t beast_in_groups(uint64_t nbytes) { return (beast_in_tiles(nbytes) + kBeastInGroup - 1) / kBeastInGroup; }
struct BeastInParams {
    const uint8_t *data;              // any alignment
    uint64_t nbytes;
    uint32_t net_ingest;
    RawInConfig cfg;
    uint64_t receiver_id_in;
    unsigned long long *cand_id;      // cand_cap entries beside RawInParams' candidate arrays
    uint8_t *frame_class;             // optional: the classes the filter does not decide; nothing at or beyond frames_cap is stored
    unsigned long long *frame_off;    // optional
    uint64_t frames_cap;
    uint64_t off_base;                // added to every frame_off (the host form's passes)
};
struct BeastInScratch {
    uint8_t *maps;                    // [tiles * 64] a tile's exit map: entry offset -> entry offset of the next tile, 0xff: the chain ends here
    uint8_t *gmaps;                   // [groups * 64] the same over a group of tiles
    uint32_t *entry;                  // [tiles + groups] where the chain from 0 enters each tile (kNone: it does not), then each group
    uint32_t *marks;                  // [tiles * kBlock] the chain's offsets, a bit per byte
    uint16_t *meta;                   // [tiles * kBlock] per lane: handler calls | candidates << 4 | an id set << 15
    unsigned long long *lane_ids;     // [tiles * kBlock] the last id a lane's steps set
    uint32_t *blocks;                 // [6 * tiles] per tile: handler calls | candidates | garbage | commands | ids taken | Mode A/C dropped
    unsigned long long *off;          // [2 * tiles] the exclusive prefix sums of the first two
    unsigned long long *tile_id;      // [tiles] the last id a tile's steps set, [tiles] the id in force at its start
    unsigned long long *entry_id;
    uint32_t *tile_idflag;            // [tiles]
    unsigned long long *total;        // [9] see launch_beast_in_front
};
void launch_beast_in_front(const BeastInParams &a, const RawInParams &p, const BeastInScratch &w, hipStream_t s);
// Planefinder input (kernels/pf_in.inc; readPlanefinder + decodePfMessage over a DLE-framed stream, pf_in_format.h): the UAT input's
// tiles; the framer is a two-state automaton whose state at an offset is the kind of the last event in front of it, so the tiles need
// one scan of their last events and no chain.  It ends in the raw input's candidate arrays and filter passes (RawInParams: a "line" is
// a handler call)
constexpr size_t pf_in_tiles(uint64_t nbytes) { return (size_t) ((nbytes + kUatTile - 1) / kUatTile); }
struct PfInParams {
    const uint8_t *data;              // any alignment
    uint64_t nbytes;                  // what is framed
    uint64_t look;                    // bytes behind them that are the stream's too: lookahead and the handler's reads (the host form's passes)
    RawInConfig cfg;
    uint8_t *frame_class;             // optional: the classes the filter does not decide; nothing at or beyond frames_cap is stored
    unsigned long long *frame_off;    // optional
    uint64_t frames_cap;
    uint64_t off_base;                // added to every frame_off (the host form's passes)
};
struct PfInScratch {
    uint32_t *ev;                     // [5 * tiles] per tile: see k_pf_in_events
    uint8_t *in_frame;                // [tiles] the framer's state at the tile's first byte
    uint16_t *meta;                   // [tiles * kBlock] per lane: handler calls | candidates << 8
    uint32_t *blocks;                 // [4 * tiles] per tile: handler calls | candidates | frames of another packet id | reads past the end
    unsigned long long *off;          // [2 * tiles] the exclusive prefix sums of the first two
    unsigned long long *total;        // [6] see launch_pf_in_front
};
void launch_pf_in_front(const PfInParams &a, const RawInParams &p, const PfInScratch &w, hipStream_t s);
// ASTERIX input (kernels/asterix_in.inc; readAsterix + decodeAsterixMessage over a length-chained stream, asterix_in_format.h)
constexpr uint32_t kAstTile = 65536;          // bytes per tile: a length is below 65536, so a chain that enters tile t leaves it into tile t + 1
constexpr uint32_t kAstGroup = 32;            // tiles whose exit maps are composed into one
constexpr uint32_t kAstWords = kAstTile / 32; // words of a tile's bitmap, a bit per byte
constexpr uint64_t kAstMaxBytes = (uint64_t) kAstTile * 0x7ffffffeull;   // a grid's limit
constexpr size_t ast_in_tiles(uint64_t nbytes) { return (size_t) (nbytes / kAstTile + 1); }   // (the chain may end AT nbytes)
constexpr size_t ast_in_groups(uint64_t nbytes) { return (ast_in_tiles(nbytes) + kAstGroup - 1) / kAstGroup; }
struct AstInParams {
    const uint8_t *data;              // any alignment
    uint64_t nbytes;                  // what is framed
    uint64_t look;                    // bytes behind them an item that overruns its record may read (the host form's passes)
    mgpu_asterix_rec *recs;           // 16-byte aligned; nothing at or beyond recs + recs_cap is stored
    unsigned long long *frame_of;     // optional, recs_cap entries
    uint64_t recs_cap;
    uint64_t frame_base;              // added to every frame index (the host form's passes)
    int64_t now_ms;
    uint32_t source;
};
struct AstInScratch {
    uint16_t *maps;                   // [(tiles - 1) * kAstTile] a tile's exit map: entry offset -> entry offset of the next tile, 0xffff: the chain ends here
    uint16_t *gmaps;                  // [(groups - 1) * kAstTile] the same over a group of tiles
    uint32_t *entry;                  // [tiles + groups] where the chain from 0 enters each tile (kNone: it does not), then each group
    uint32_t *bits;                   // [3 * tiles * kAstWords] per tile: frame starts | those that give a record | those of another category
    uint32_t *blocks;                 // [4 * stride] per tile: frames | records | other | undefined
    unsigned long long *off;          // [2 * stride] the exclusive prefix sums of the first two
    unsigned long long *total;        // [9] frames, records, other, undefined, consumed, stop | the first closing frame (~0: none), the chain's end, its kind
    size_t stride;                    // >= tiles
};
void launch_asterix_decode(const AstInParams &a, const AstInScratch &w, hipStream_t s);
// stable merge of message lists by timestamp (kernels/merge.inc): segs [nseg] in device memory, scratch = merge_scratch_bytes(n, nseg)
struct MergeSeg {
    const mgpu_msg *msgs;
    const uint8_t *verdict;       // may be null
    uint64_t start;               // of the segment in the concatenation
    uint64_t id;
};
constexpr uint32_t kMergeMaxSeg = 4096;
size_t merge_scratch_bytes(uint64_t n, uint32_t nseg);
// the two halves of a merge (n > 0): the keys + the bits they differ in (the returned device word), then — that word read back — the
// digit passes up to its highest bit and the gather; returns the number of passes
const unsigned long long *launch_merge_keys(const MergeSeg *h_segs, uint32_t nseg, uint64_t n, void *scratch, hipStream_t s);
int launch_merge_sort(uint32_t nseg, uint64_t n, uint64_t diff, void *scratch, mgpu_msg *out, uint64_t *perm, uint64_t *ids, uint8_t *verdict_out,
                      hipStream_t s);
// first stage of the tracker + the forwarding rule over a message list in device memory (kernels/gate.inc): table = gate_table_bytes()
// bytes, zeroed once and kept from call to call; scratch = gate_scratch_bytes(n); verdict: one byte per message (include/modes_gpu.h)
size_t gate_table_bytes();
size_t gate_scratch_bytes(uint64_t n);
void launch_track_gate(const mgpu_msg *msgs, const mgpu_fields *fields, uint64_t n, uint32_t buf_samples, void *table, void *scratch,
                       uint8_t *verdict, hipStream_t s);
// CPR pairing + position decode over a message list in device memory (kernels/cpr.inc): table = cpr_table_bytes() bytes, zeroed once and
// kept from call to call; scratch = cpr_scratch_bytes(n); out: one record per message.  launch_cpr_cases: cpr.c's decoders, lane = case
size_t cpr_table_bytes();
size_t cpr_scratch_bytes(uint64_t n);
void launch_cpr_track(const mgpu_msg *msgs, const mgpu_fields *fields, uint64_t n, const mgpu_cpr_config &cfg, void *table, void *scratch,
                      mgpu_position *out, hipStream_t s);
void launch_cpr_cases(const mgpu_cpr_case *cases, uint64_t n, mgpu_cpr_result *out, hipStream_t s);
// signal power of accepted messages: sum of mag^2 over d_mag[pos+19 .. pos+19+len)
void launch_signal_power(const uint16_t *mag, const uint32_t *pos, const uint16_t *len, uint32_t nmsg,
                         unsigned long long *out, hipStream_t s);
// candidates / tried phases / conditional-class candidates inside the skip-ahead window of
// each accepted message (positions pos+1 .. pos+skip, clipped to `limit`), for the stats fix-up
// struct modesMessage fields of the accepted frames on the device (kernels/build.inc): acc = Accepted[nacc], bufs = BufferClock[]
void launch_build_messages(const PhaseRec *live, const unsigned long long *live_sig, const unsigned long long *msg_sig, const void *d_acc,
                           const void *d_bufs, uint32_t nacc, mgpu_msg *out, hipStream_t s);   // msg_sig (per accepted frame) or, when null, live_sig (per live record)
void launch_stage_blob(const void *h_src, void *d_dst, uint64_t bytes, hipStream_t s);   // page-locked host -> device, small grid

// ---- the ordered accept walk on the device (kernels/walk.inc) ----
constexpr uint32_t kWkNoAdd = 0xffffffffu;
constexpr uint32_t kWkTouchedCap = 1u << 16;        // distinct adder addresses per chunk and table
constexpr int kWkCounts = 16;                       // per-buffer counters (WKC_* in kernels/walk.inc, the order of ResolveCounts)
constexpr int32_t kWkNoFlip = 0x7fffffff;
struct WalkIn {                  // head of the per-chunk input blob; then (at kWkInHead) BufferClock[nbuf], active[n_active], inactive[n_inactive]
    int64_t next_flip;           // Resolver::next_flip(): the expiry is due at the first buffer end with clock >= this
    uint32_t nbuf, n_active, n_inactive, acc_cap;   // acc_cap: accept-list capacity per buffer
    uint32_t nlive, buf_len, pad[2];   // live records of the chunk (the device's own counter block is back to zero by now); buffer b = positions [b * buf_len, ..)
};
static_assert(sizeof(WalkIn) == 40, "WalkIn");
constexpr uint32_t kWkInHead = 48;                  // the buffer clocks start here
struct WalkState {
    int32_t flip;                // the expiry is assumed after this buffer (kWkNoFlip: not in this chunk)
    uint32_t converged, iterations, bad;
    uint32_t n_touched[2];
    uint32_t cur, done;          // done: workgroups of the running kernel that have finished (last one does the serial part)
};
struct WalkBuffers {             // device memory of the walk (one set per context)
    uint32_t *bit_active, *bit_inactive;             // 2^24 bits each: the filter's two generations when the chunk starts
    uint32_t *first[2];                              // 2^24 entries each: first buffer of the chunk that adds the address
    uint32_t *touched[2];                            // addresses with an entry in first[t]
    WalkState *state;
    uint32_t *rec_lo;                                // [nbuf + 1]: first live record at or after the buffer's first position
    uint32_t *nacc, *nadds, *counts;                 // per buffer
    long long *end_clock;                            // per buffer: Modes.synthetic_now at its end
    uint32_t *acc;                                   // per buffer acc_cap x (record index, score)
    uint32_t *adds;                                  // per buffer acc_cap addresses, in order of their first add in the buffer
    uint32_t *offs, *aoffs;                          // [nbuf + 1] prefix of nacc / of nadds
};
struct WalkSummary {             // what the host reads (page-locked): this, then per buffer 6 words {accepted, adds, end clock lo, hi,
    uint32_t converged, bad, iterations, nmsg;       // offset into the adds, offset into the accept list}, then the adds
    int32_t flip; uint32_t nadds_total, nbuf, pad;
    unsigned long long counts[kWkCounts];
};
size_t walk_summary_bytes(uint32_t nbuf, uint32_t acc_cap);
size_t walk_input_bytes(uint32_t nbuf, uint32_t n_active, uint32_t n_inactive);
void launch_device_walk(const uint8_t *h_in, uint8_t *d_in, size_t in_bytes, const WalkBuffers &w, const PhaseRec *live, uint32_t nbuf,
                        void *h_summary, void *d_acc, uint32_t *msg_pos, uint32_t *msg_limit, uint16_t *msg_skip, uint32_t msg_cap, hipStream_t s);
// signal power of the accepted frames after the walk: out[i] = sum of mag^2 over frame i | 1 << 63 for a 112-bit frame
void launch_msg_sig(const uint16_t *mag, const uint32_t *d_pos, const uint16_t *d_skip, uint32_t n, unsigned long long *d_out, unsigned long long *h_out,
                    hipStream_t s);   // h_out (page-locked host memory, may be null): a second copy for the builder
void launch_stage_in(const uint32_t *h_pos, const uint32_t *h_limit, const uint16_t *h_skip, uint32_t *d_pos, uint32_t *d_limit,
                     uint16_t *d_skip, uint32_t n, hipStream_t s);   // page-locked host arrays -> device, small grid
// shard passes: the same numbers for every live record's would-be window, packed into out[record] (kernels/window_stats.inc)
void launch_live_windows(const uint16_t *mag, uint64_t n, const uint16_t *cand, const uint32_t *cand_count, const uint32_t *class_bitmap, const PhaseRec *live, const unsigned long long *nlive_dev,
                         uint32_t buf_len, unsigned long long *out, hipStream_t s);
void launch_window_stats(const uint16_t *mag, uint64_t n, const uint16_t *cand, const uint32_t *cand_count, const uint32_t *class_bitmap, const uint32_t *pos,   // cand / cand_count: k_sweep's lists of the chunk
                         const uint16_t *skip, const uint32_t *limit, uint32_t nmsg, unsigned long long *part, unsigned long long *out,
                         hipStream_t s, unsigned long long *sig_out = nullptr, unsigned long long *sig_host = nullptr,
                         hipEvent_t ev_sig = nullptr);   // sig_out: also the frames' signal powers (k_msg_sig's form), sig_host: a second copy in page-locked host memory, ev_sig: recorded behind them

}  // namespace mgpu
