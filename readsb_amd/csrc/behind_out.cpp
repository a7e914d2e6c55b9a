// behind_out.cpp — behind the message list, the outputs over it: beast encoder, time merge, field decode, tracking gate, position decode,
// the text outputs, ASTERIX out and the message dump; at the bottom the CRC / table diagnostics.  (The stream inputs: behind_in.cpp.)
#include "behind.h"

#include <cmath>
#include <cstring>
#include <optional>

#include "dump_format.h"

// What every encoder entry does once its arguments passed: the caller's counts zeroed (each but the first may be null) and, for a
// list that is not empty, the device set.  An answer: the entry's, already (the empty list's MGPU_OK, or an error).
static std::optional<int> encode_begin(mgpu_ctx *c, uint64_t n, uint64_t *bytes, uint64_t *ndeferred, uint64_t *nskipped) {
    *bytes = 0;
    if (ndeferred) *ndeferred = 0;
    if (nskipped) *nskipped = 0;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return std::nullopt;
}

// One optional per-message array of a host-array form into the staging buffer of its role: *arr becomes the device copy (a null
// array stays null).
template <class T>
static int stage_optional(mgpu_ctx *c, DevBuf &buf, const T **arr, uint64_t n) {
    if (!*arr) return MGPU_OK;
    if (int rc = buf.reserve(c, n * sizeof(T))) return rc;
    HIPCHK(c, hipMemcpyAsync(buf.p, *arr, n * sizeof(T), hipMemcpyHostToDevice, c->stream_aux));
    *arr = buf.as<T>();
    return MGPU_OK;
}

extern "C" {

// ---- beast wire format (net_io.c:1655-1714) for message records that already are in HBM -----------------------

// What follows the message list — field decode, beast encoder, tracking gate — runs on a stream of its own (stream_aux): these calls
// are synchronous, and on the pipeline's main stream they waited for every chunk a deferred feed had queued there.  Each operation
// has one core (*_dev) that takes device pointers, reserves the operation's scratch and enqueues; the `_device` entry and the
// host-array entry (which stages its arrays in the context's buffers) both call it.

// d_verdict == nullptr: every message's frame.  Everything in device memory; *ndeferred (may be null without a verdict).
// d_ids / *last_id (host, may be null): the receiver-id prefixes; MGPU_BEAST_VERBATIM in flags (include/modes_gpu.h)
static int beast_encode_dev(mgpu_ctx *c, const mgpu_msg *d_msgs, const uint8_t *d_verdict, uint64_t n, uint32_t flags, uint8_t *d_out, uint64_t cap,
                            uint64_t *bytes, mgpu_deferred *d_deferred, uint64_t deferred_cap, uint64_t *ndeferred, const uint64_t *d_ids = nullptr,
                            uint64_t *last_id = nullptr) {
    Behind &b = *c->behind;
    const size_t nb = (size_t) (n / kBlock + 2);                 // per workgroup: frame bytes | deferred messages, nb entries each
    if (int rc = b.d_beast_len.reserve(c, n * sizeof(uint16_t))) return rc;
    if (int rc = b.d_beast_blocks.reserve(c, 2 * nb * sizeof(uint32_t))) return rc;
    if (int rc = b.d_beast_off.reserve(c, 2 * nb * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_beast_total.reserve_exact(c, 4 * sizeof(unsigned long long))) return rc;   // bytes, deferred, last id
    if (d_ids)
        if (int rc = b.d_beast_idw.reserve(c, beast_id_scratch_bytes(n))) return rc;
    const bool verbatim = (flags & MGPU_BEAST_VERBATIM) != 0, gated = d_verdict && !verbatim;
    uint32_t *blocks = b.d_beast_blocks.as<uint32_t>();
    unsigned long long *off = b.d_beast_off.as<unsigned long long>(), *d_total = b.d_beast_total.as<unsigned long long>();
    launch_beast_encode(d_msgs, n, b.d_beast_len.as<uint16_t>(), blocks, off, d_out, cap, d_total, c->stream_aux, d_verdict,
                        (flags & MGPU_BEAST_NET_RULE) ? 1 : 0, blocks + nb, off + nb, d_deferred, deferred_cap, verbatim ? 1 : 0,
                        (const unsigned long long *) d_ids, last_id ? *last_id : 0ull, b.d_beast_idw.p);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(total, d_total, (d_ids ? 3 : gated ? 2 : 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    *bytes = total[0];
    if (ndeferred) *ndeferred = gated ? total[1] : 0;
    if (d_ids && last_id) *last_id = total[2];
    if (total[0] > cap) { c->err = "mgpu_beast_encode: output buffer too small"; return MGPU_E_OVERFLOW; }
    if (gated && total[1] > deferred_cap) { c->err = "mgpu_beast_encode_gated: more deferred messages than the list holds"; return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

// host lists -> d_list back to back (and, with `verdicts`, their verdict bytes -> d_list_verdict; a list's may be null)
static int stage_messages(mgpu_ctx *c, const struct mgpu_msg *const *lists, const uint64_t *counts, uint32_t nlists, uint64_t n,
                          const uint8_t *const *verdicts = nullptr) {
    Behind &b = *c->behind;
    if (int rc = b.d_list.reserve(c, n * sizeof(mgpu_msg))) return rc;
    if (verdicts)
        if (int rc = b.d_list_verdict.reserve(c, n)) return rc;
    uint64_t at = 0;
    for (uint32_t k = 0; k < nlists; at += counts[k++]) {
        if (!counts[k]) continue;
        HIPCHK(c, hipMemcpyAsync(b.d_list.as<mgpu_msg>() + at, lists[k], counts[k] * sizeof(mgpu_msg), hipMemcpyHostToDevice, c->stream_aux));
        if (verdicts && verdicts[k])
            HIPCHK(c, hipMemcpyAsync(b.d_list_verdict.as<uint8_t>() + at, verdicts[k], counts[k], hipMemcpyHostToDevice, c->stream_aux));
    }
    return MGPU_OK;
}
static int stage_messages(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n, const uint8_t *verdict = nullptr) {
    return stage_messages(c, &msgs, &n, 1, n, verdict ? &verdict : nullptr);
}

// the staged outputs of a host-array form: room for them before the launch (*out and *deferred become the device buffers), the stream
// and the listed entries back after it
static int staged_out_reserve(mgpu_ctx *c, uint64_t cap, bool gated, uint64_t deferred_cap, uint8_t **out, struct mgpu_deferred **deferred) {
    Behind &b = *c->behind;
    if (int rc = b.d_out.reserve(c, cap + 64)) return rc;                        // (an encoder may store a vector past the stream's end)
    if (gated)
        if (int rc = b.d_deferred.reserve(c, (deferred_cap + 64) * sizeof(mgpu_deferred))) return rc;
    *out = b.d_out.as<uint8_t>();
    *deferred = b.d_deferred.as<mgpu_deferred>();
    return MGPU_OK;
}
static int staged_out_fetch(mgpu_ctx *c, uint8_t *out, uint64_t bytes, struct mgpu_deferred *deferred, const uint64_t *ndeferred) {
    Behind &b = *c->behind;
    if (bytes) HIPCHK(c, hipMemcpy(out, b.d_out.p, bytes, hipMemcpyDeviceToHost));
    if (ndeferred && *ndeferred) HIPCHK(c, hipMemcpy(deferred, b.d_deferred.p, *ndeferred * sizeof(mgpu_deferred), hipMemcpyDeviceToHost));
    return MGPU_OK;
}

// the encoder over the staged list (d_verdict / d_ids: the staged arrays it is to read, or null): stream -> out, deferred list -> deferred
static int beast_encode_staged(mgpu_ctx *c, const uint8_t *d_verdict, const uint64_t *d_ids, uint64_t n, uint32_t flags, uint8_t *out, uint64_t cap,
                               uint64_t *bytes, mgpu_deferred *deferred, uint64_t deferred_cap, uint64_t *ndeferred, uint64_t *last_id) {
    uint8_t *d_out;
    mgpu_deferred *d_deferred;
    if (int rc = staged_out_reserve(c, cap, d_verdict != nullptr, deferred_cap, &d_out, &d_deferred)) return rc;
    if (int rc = beast_encode_dev(c, c->behind->d_list.as<mgpu_msg>(), d_verdict, n, flags, d_out, cap, bytes, d_deferred, deferred_cap, ndeferred, d_ids, last_id)) return rc;
    return staged_out_fetch(c, out, *bytes, deferred, ndeferred);
}

// ---- the encoder with receiver ids and --net-verbatim (include/modes_gpu.h) ----
static bool beast_args_ok(const struct mgpu_beast_args *a) {
    if (!a || a->size < sizeof(struct mgpu_beast_args) || !a->bytes) return false;
    if (a->flags & ~(MGPU_BEAST_NET_RULE | MGPU_BEAST_VERBATIM)) return false;
    if (a->n && (!a->msgs || !a->out)) return false;
    const bool gated = a->verdict && !(a->flags & MGPU_BEAST_VERBATIM);
    if (gated && (!a->ndeferred || (a->deferred_cap && !a->deferred))) return false;
    return true;
}

int mgpu_beast_encode_ex_device(mgpu_ctx *c, const struct mgpu_beast_args *a) {
    if (!c || !beast_args_ok(a)) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, a->n, a->bytes, a->ndeferred, nullptr)) return *done;
    return beast_encode_dev(c, a->msgs, a->verdict, a->n, a->flags, a->out, a->cap, a->bytes, a->deferred, a->deferred_cap, a->ndeferred, a->ids, a->last_id);
}

int mgpu_beast_encode_ex(mgpu_ctx *c, const struct mgpu_beast_args *a) {
    if (!c || !beast_args_ok(a)) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, a->n, a->bytes, a->ndeferred, nullptr)) return *done;
    Behind &b = *c->behind;
    const uint64_t n = a->n;
    const bool gated = a->verdict && !(a->flags & MGPU_BEAST_VERBATIM);
    if (int rc = stage_messages(c, a->msgs, n, gated ? a->verdict : nullptr)) return rc;
    const uint64_t *d_ids = a->ids;
    if (int rc = stage_optional(c, b.d_opt_ids, &d_ids, n)) return rc;
    return beast_encode_staged(c, gated ? b.d_list_verdict.as<uint8_t>() : nullptr, d_ids, n, a->flags, a->out, a->cap, a->bytes, a->deferred, a->deferred_cap,
                               a->ndeferred, a->last_id);
}

// the entries from before the argument block: the same checks as beast_args_ok makes once the block is filled in
static struct mgpu_beast_args beast_plain_args(const struct mgpu_msg *msgs, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *bytes) {
    struct mgpu_beast_args a = {};
    a.size = sizeof a; a.msgs = msgs; a.n = n; a.out = out; a.cap = cap; a.bytes = bytes;
    return a;
}

int mgpu_beast_encode_device(mgpu_ctx *c, const struct mgpu_msg *d_msgs, uint64_t n, uint8_t *d_out, uint64_t cap, uint64_t *bytes) {
    const struct mgpu_beast_args a = beast_plain_args(d_msgs, n, d_out, cap, bytes);
    return mgpu_beast_encode_ex_device(c, &a);
}

int mgpu_beast_encode(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *bytes) {
    const struct mgpu_beast_args a = beast_plain_args(msgs, n, out, cap, bytes);
    return mgpu_beast_encode_ex(c, &a);
}

int mgpu_beast_encode_gated_device(mgpu_ctx *c, const struct mgpu_msg *d_msgs, const uint8_t *d_verdict, uint64_t n, uint32_t flags, uint8_t *d_out,
                                   uint64_t cap, uint64_t *bytes, struct mgpu_deferred *d_deferred, uint64_t deferred_cap, uint64_t *ndeferred) {
    if (!c || !bytes || !ndeferred || (n && (!d_msgs || !d_verdict || !d_out)) || (deferred_cap && !d_deferred)) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, n, bytes, ndeferred, nullptr)) return *done;
    return beast_encode_dev(c, d_msgs, d_verdict, n, flags, d_out, cap, bytes, d_deferred, deferred_cap, ndeferred);
}

// ---- the aggregator's time merge (kernels/merge.inc) ----

static int merge_dev(mgpu_ctx *c, const struct mgpu_msg *const *d_segments, const uint64_t *counts, uint32_t nseg, const uint64_t *segment_ids,
                     const uint8_t *const *d_verdict_in, struct mgpu_msg *d_out, uint64_t *d_perm, uint64_t *d_ids, uint8_t *d_verdict_out, uint64_t n) {
    Behind &b = *c->behind;
    std::vector<MergeSeg> segs(nseg);
    uint64_t start = 0;
    for (uint32_t k = 0; k < nseg; ++k) {
        segs[k].msgs = d_segments[k];
        segs[k].verdict = d_verdict_in ? d_verdict_in[k] : nullptr;
        segs[k].start = start;
        segs[k].id = segment_ids ? segment_ids[k] : 0;
        start += counts[k];
    }
    if (int rc = b.d_merge_scratch.reserve(c, merge_scratch_bytes(n, nseg))) return rc;
    const unsigned long long *d_diff = launch_merge_keys(segs.data(), nseg, n, b.d_merge_scratch.p, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long diff = 0;
    HIPCHK(c, hipMemcpyAsync(&diff, d_diff, sizeof diff, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));            // (the segment table has left `segs` by now, too)
    b.merge_passes = launch_merge_sort(nseg, n, diff, b.d_merge_scratch.p, d_out, d_perm, d_ids, d_verdict_out, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    return MGPU_OK;
}

// the arguments both forms check; *n = the sum of the counts
static int merge_args(mgpu_ctx *c, const struct mgpu_msg *const *segments, const uint64_t *counts, uint32_t nseg, const uint8_t *const *verdict_in,
                      const void *out, const void *verdict_out, uint64_t *n) {
    if (!c || nseg > kMergeMaxSeg || (nseg && (!segments || !counts))) return MGPU_E_INVAL;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < nseg; ++k) {
        if (counts[k] > 0xffffffffull) { c->err = "mgpu_merge_by_time: more than 2^32 - 1 records"; return MGPU_E_CAPACITY; }
        sum += counts[k];
        if (counts[k] && (!segments[k] || ((uintptr_t) segments[k] & 15u))) return MGPU_E_INVAL;
    }
    if (sum > 0xffffffffull) { c->err = "mgpu_merge_by_time: more than 2^32 - 1 records"; return MGPU_E_CAPACITY; }
    if (sum && (!out || (verdict_out && !verdict_in))) return MGPU_E_INVAL;
    *n = sum;
    return MGPU_OK;
}

int mgpu_merge_by_time_device(mgpu_ctx *c, const struct mgpu_msg *const *d_segments, const uint64_t *counts, uint32_t nseg, const uint64_t *segment_ids,
                              const uint8_t *const *d_verdict_in, struct mgpu_msg *d_out, uint64_t *d_perm, uint64_t *d_ids, uint8_t *d_verdict_out) {
    uint64_t n = 0;
    if (int rc = merge_args(c, d_segments, counts, nseg, d_verdict_in, d_out, d_verdict_out, &n)) return rc;
    c->behind->merge_passes = 0;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = merge_dev(c, d_segments, counts, nseg, segment_ids, d_verdict_in, d_out, d_perm, d_ids, d_verdict_out, n)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

int mgpu_merge_by_time(mgpu_ctx *c, const struct mgpu_msg *const *segments, const uint64_t *counts, uint32_t nseg, const uint64_t *segment_ids,
                       const uint8_t *const *verdict_in, struct mgpu_msg *out, uint64_t *perm, uint64_t *ids, uint8_t *verdict_out) {
    uint64_t n = 0;
    if (int rc = merge_args(c, segments, counts, nseg, verdict_in, out, verdict_out, &n)) return rc;
    Behind &b = *c->behind;
    b.merge_passes = 0;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // staged: the concatenation in d_list, its verdicts in d_list_verdict; results: records | permutation | ids | verdicts in d_merge_out
    if (int rc = stage_messages(c, segments, counts, nseg, n, verdict_in)) return rc;
    if (int rc = b.d_merge_out.reserve(c, n * (sizeof(mgpu_msg) + 8 + 8 + 1))) return rc;
    std::vector<const mgpu_msg *> d_seg(nseg);
    std::vector<const uint8_t *> d_ver(nseg);
    uint64_t at = 0;
    for (uint32_t k = 0; k < nseg; at += counts[k++]) {
        d_seg[k] = b.d_list.as<mgpu_msg>() + at;
        d_ver[k] = counts[k] && verdict_in && verdict_in[k] ? b.d_list_verdict.as<uint8_t>() + at : nullptr;
    }
    mgpu_msg *d_out = b.d_merge_out.as<mgpu_msg>();
    uint64_t *d_perm = (uint64_t *) (d_out + n), *d_ids = d_perm + n;
    uint8_t *d_vout = (uint8_t *) (d_ids + n);
    if (int rc = merge_dev(c, d_seg.data(), counts, nseg, segment_ids, verdict_in ? d_ver.data() : nullptr, d_out, perm ? d_perm : nullptr, ids ? d_ids : nullptr,
                           verdict_out ? d_vout : nullptr, n))
        return rc;
    HIPCHK(c, hipMemcpyAsync(out, d_out, n * sizeof(mgpu_msg), hipMemcpyDeviceToHost, c->stream_aux));
    if (perm) HIPCHK(c, hipMemcpyAsync(perm, d_perm, n * 8, hipMemcpyDeviceToHost, c->stream_aux));
    if (ids) HIPCHK(c, hipMemcpyAsync(ids, d_ids, n * 8, hipMemcpyDeviceToHost, c->stream_aux));
    if (verdict_out) HIPCHK(c, hipMemcpyAsync(verdict_out, d_vout, n, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

int mgpu_merge_last_passes(mgpu_ctx *c) { return c ? c->behind->merge_passes : MGPU_E_INVAL; }

// ---- per-message field decode (mode_s.c:598-760, 806-1555; mode_ac.c:171-200) --------------------------------------

static int fields_dev(mgpu_ctx *c, const struct mgpu_msg *d_msgs, uint64_t n, struct mgpu_fields *d_out) {
    DevBuf &tan = c->behind->d_roll_tan;
    if (!tan.p) {
        const std::vector<double> t = build_roll_tangent_table();
        if (int rc = tan.reserve_exact(c, t.size() * sizeof(double))) return rc;
        HIPCHK(c, hipMemcpy(tan.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    launch_decode_fields(d_msgs, n, d_out, tan.as<double>(), c->stream_aux);
    return MGPU_OK;
}

int mgpu_decode_fields_device(mgpu_ctx *c, const struct mgpu_msg *d_msgs, uint64_t n, struct mgpu_fields *d_out) {
    if (!c || (n && (!d_msgs || !d_out))) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = fields_dev(c, d_msgs, n, d_out)) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

// host list -> d_list, its field records -> d_fields
static int fields_staged(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n) {
    Behind &b = *c->behind;
    if (int rc = b.d_fields.reserve(c, n * sizeof(mgpu_fields))) return rc;
    if (int rc = stage_messages(c, msgs, n)) return rc;
    return fields_dev(c, b.d_list.as<mgpu_msg>(), n, b.d_fields.as<mgpu_fields>());
}

// The list of a text, ASTERIX or dump host form: *msgs -> d_list; its field records, the caller's or decoded here -> d_fields; its
// verdicts (no pointer, or a null array: none) -> d_list_verdict.  The three become the device copies.
static int stage_list(mgpu_ctx *c, const struct mgpu_msg **msgs, const struct mgpu_fields **fields_io, const uint8_t **verdict_io, uint64_t n) {
    Behind &b = *c->behind;
    const struct mgpu_fields *fields = *fields_io;
    const uint8_t *verdict = verdict_io ? *verdict_io : nullptr;
    if (fields) {
        if (int rc = stage_messages(c, *msgs, n, verdict)) return rc;
        if (int rc = b.d_fields.reserve(c, n * sizeof(mgpu_fields))) return rc;
        HIPCHK(c, hipMemcpyAsync(b.d_fields.p, fields, n * sizeof(mgpu_fields), hipMemcpyHostToDevice, c->stream_aux));
    } else {
        if (int rc = fields_staged(c, *msgs, n)) return rc;
        if (verdict) {
            if (int rc = b.d_list_verdict.reserve(c, n)) return rc;
            HIPCHK(c, hipMemcpyAsync(b.d_list_verdict.p, verdict, n, hipMemcpyHostToDevice, c->stream_aux));
        }
    }
    *msgs = b.d_list.as<mgpu_msg>();
    *fields_io = b.d_fields.as<mgpu_fields>();
    if (verdict) *verdict_io = b.d_list_verdict.as<uint8_t>();
    return MGPU_OK;
}

int mgpu_decode_fields(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n, struct mgpu_fields *out) {
    if (!c || (n && (!msgs || !out))) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = fields_staged(c, msgs, n)) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->behind->d_fields.p, n * sizeof(mgpu_fields), hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

// ---- first stage of the tracker + forwarding rule (track.c:1688-1693, 1905-1966; net_io.c:5846-5849, 5924-5940), kernels/gate.inc ----

// An aircraft table (the gate's, the position decode's): allocated at its size and zeroed by the first call, then carried from call to call
static int table_ready(mgpu_ctx *c, DevBuf &table, uint64_t bytes) {
    if (table.p) return MGPU_OK;
    if (int rc = table.reserve_exact(c, bytes)) return rc;
    HIPCHK(c, hipMemsetAsync(table.p, 0, bytes, c->stream_aux));
    return MGPU_OK;
}

static int table_reset(mgpu_ctx *c, DevBuf &table) {
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (table.p) {
        HIPCHK(c, hipMemsetAsync(table.p, 0, table.cap, c->stream_aux));
        HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    }
    return MGPU_OK;
}

static int gate_dev(mgpu_ctx *c, const struct mgpu_msg *d_msgs, const struct mgpu_fields *d_fields, uint64_t n, uint8_t *d_verdict) {
    Behind &b = *c->behind;
    if (int rc = table_ready(c, b.d_gate_table, gate_table_bytes())) return rc;
    if (int rc = b.d_gate_scratch.reserve(c, gate_scratch_bytes(n))) return rc;
    launch_track_gate(d_msgs, d_fields, n, c->cfg.buf_samples, b.d_gate_table.p, b.d_gate_scratch.p, d_verdict, c->stream_aux);
    return MGPU_OK;
}

int mgpu_track_gate_reset(mgpu_ctx *c) { return c ? table_reset(c, c->behind->d_gate_table) : MGPU_E_INVAL; }

int mgpu_track_gate_device(mgpu_ctx *c, const struct mgpu_msg *d_msgs, const struct mgpu_fields *d_fields, uint64_t n, uint8_t *d_verdict) {
    if (!c || (n && (!d_msgs || !d_fields || !d_verdict)) || n > 0xffffffffull) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = gate_dev(c, d_msgs, d_fields, n, d_verdict)) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

// host list -> d_list, its field records -> d_fields, its verdicts (continuing the context's aircraft table) -> d_gate_verdict
static int gate_staged(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n) {
    Behind &b = *c->behind;
    if (int rc = fields_staged(c, msgs, n)) return rc;
    if (int rc = b.d_gate_verdict.reserve(c, n)) return rc;
    if (int rc = gate_dev(c, b.d_list.as<mgpu_msg>(), b.d_fields.as<mgpu_fields>(), n, b.d_gate_verdict.as<uint8_t>())) return rc;
    HIPCHK(c, hipGetLastError());
    return MGPU_OK;
}

int mgpu_track_gate(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n, uint8_t *verdict) {
    if (!c || (n && (!msgs || !verdict)) || n > 0xffffffffull) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = gate_staged(c, msgs, n)) return rc;
    HIPCHK(c, hipMemcpyAsync(verdict, c->behind->d_gate_verdict.p, n, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

// The gate's verdict applied to the encoder: the beast stream of what the reference forwards for certain + the list of the
// messages its position tracker has to settle (include/modes_gpu.h).  Host arrays; the aircraft table goes on from call to call.
// (Its own checks, not beast_args_ok's: it wants ndeferred whatever the flags, and lets unknown flags pass.)
int mgpu_beast_encode_gated(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n, uint32_t flags, uint8_t *out, uint64_t cap, uint64_t *bytes,
                            struct mgpu_deferred *deferred, uint64_t deferred_cap, uint64_t *ndeferred) {
    if (!c || !bytes || !ndeferred || (n && (!msgs || !out)) || (deferred_cap && !deferred) || n > 0xffffffffull) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, n, bytes, ndeferred, nullptr)) return *done;
    if (int rc = gate_staged(c, msgs, n)) return rc;
    return beast_encode_staged(c, c->behind->d_gate_verdict.as<uint8_t>(), nullptr, n, flags, out, cap, bytes, deferred, deferred_cap, ndeferred, nullptr);
}

// ---- CPR pairing + position decode (track.c:1249-1282, 1827-1850, 758-799, 862-914; cpr.c:62-374), kernels/cpr.inc ----

static int cpr_track_dev(mgpu_ctx *c, const struct mgpu_cpr_config *cfg, const struct mgpu_msg *d_msgs, const struct mgpu_fields *d_fields, uint64_t n,
                         struct mgpu_position *d_out) {
    Behind &b = *c->behind;
    if (int rc = table_ready(c, b.d_cpr_table, cpr_table_bytes())) return rc;
    if (int rc = b.d_cpr_scratch.reserve(c, cpr_scratch_bytes(n))) return rc;
    launch_cpr_track(d_msgs, d_fields, n, *cfg, b.d_cpr_table.p, b.d_cpr_scratch.p, d_out, c->stream_aux);
    return MGPU_OK;
}

static bool cpr_config_ok(const struct mgpu_cpr_config *cfg) { return cfg && std::isfinite(cfg->ref_lat) && std::isfinite(cfg->ref_lon); }

int mgpu_cpr_reset(mgpu_ctx *c) { return c ? table_reset(c, c->behind->d_cpr_table) : MGPU_E_INVAL; }

int mgpu_cpr_track_device(mgpu_ctx *c, const struct mgpu_cpr_config *cfg, const struct mgpu_msg *d_msgs, const struct mgpu_fields *d_fields, uint64_t n,
                          struct mgpu_position *d_out) {
    if (!c || !cpr_config_ok(cfg) || (n && (!d_msgs || !d_fields || !d_out)) || n >= 0xfffffffeull) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = cpr_track_dev(c, cfg, d_msgs, d_fields, n, d_out)) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

int mgpu_cpr_track(mgpu_ctx *c, const struct mgpu_cpr_config *cfg, const struct mgpu_msg *msgs, uint64_t n, struct mgpu_position *out) {
    if (!c || !cpr_config_ok(cfg) || (n && (!msgs || !out)) || n >= 0xfffffffeull) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    if (int rc = fields_staged(c, msgs, n)) return rc;
    if (int rc = b.d_cpr_out.reserve(c, n * sizeof(mgpu_position))) return rc;
    if (int rc = cpr_track_dev(c, cfg, b.d_list.as<mgpu_msg>(), b.d_fields.as<mgpu_fields>(), n, b.d_cpr_out.as<mgpu_position>())) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, b.d_cpr_out.p, n * sizeof(mgpu_position), hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

// (cpr.c's decoders need no scratch: the launcher is the core both forms call)
int mgpu_cpr_decode_device(mgpu_ctx *c, const struct mgpu_cpr_case *d_cases, uint64_t n, struct mgpu_cpr_result *d_out) {
    if (!c || (n && (!d_cases || !d_out))) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    launch_cpr_cases(d_cases, n, d_out, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

int mgpu_cpr_decode(mgpu_ctx *c, const struct mgpu_cpr_case *cases, uint64_t n, struct mgpu_cpr_result *out) {
    if (!c || (n && (!cases || !out))) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    DevBuf &buf = c->behind->d_cpr_cases;                        // cases, and their results behind them
    if (int rc = buf.reserve(c, n * (sizeof(mgpu_cpr_case) + sizeof(mgpu_cpr_result)))) return rc;
    mgpu_cpr_case *d_cases = buf.as<mgpu_cpr_case>();
    mgpu_cpr_result *d_out = (mgpu_cpr_result *) (d_cases + n);
    HIPCHK(c, hipMemcpyAsync(d_cases, cases, n * sizeof(mgpu_cpr_case), hipMemcpyHostToDevice, c->stream_aux));
    launch_cpr_cases(d_cases, n, d_out, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_out, n * sizeof(mgpu_cpr_result), hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

// ---- text outputs: SBS lines (modesSendSBSOutput, net_io.c:3184-3404) and AVR raw lines (modesSendRawOutput, net_io.c:1837-1863), kernels/text.inc ----

// (len_bytes: of a message's length word: 2, the dump's 4)
static int text_scratch(mgpu_ctx *c, uint64_t n, TextScratch *w, size_t len_bytes = sizeof(uint16_t)) {
    Behind &b = *c->behind;
    const size_t nb = (size_t) (n / kBlock + 2);                 // per workgroup: bytes | deferred | skipped, nb entries each
    if (int rc = b.d_text_len.reserve(c, n * len_bytes)) return rc;
    if (int rc = b.d_text_blocks.reserve(c, 3 * nb * sizeof(uint32_t))) return rc;
    if (int rc = b.d_text_off.reserve(c, 3 * nb * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_text_total.reserve_exact(c, 4 * sizeof(unsigned long long))) return rc;
    *w = {b.d_text_len.as<uint16_t>(), b.d_text_blocks.as<uint32_t>(), b.d_text_off.as<unsigned long long>(), b.d_text_total.as<unsigned long long>(), nb};
    return MGPU_OK;
}

// behind either launch: the three totals back, the caller's counts, the overflow answers
static int text_finish(mgpu_ctx *c, const TextScratch &w, bool gated, uint64_t cap, uint64_t deferred_cap, uint64_t *bytes, uint64_t *ndeferred,
                       uint64_t *nskipped, bool skips) {
    HIPCHK(c, hipGetLastError());
    unsigned long long total[3] = {0, 0, 0};                     // (the third is computed only for a job that can skip: SBS, ASTERIX)
    HIPCHK(c, hipMemcpyAsync(total, w.total, (skips ? 3 : 2) * sizeof total[0], hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    *bytes = total[0];
    if (ndeferred) *ndeferred = gated ? total[1] : 0;
    if (nskipped) *nskipped = total[2];
    if (total[0] > cap) { c->err = "text encode: output buffer too small"; return MGPU_E_OVERFLOW; }
    if (gated && total[1] > deferred_cap) { c->err = "text encode: more deferred messages than the list holds"; return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

// a: every array a device pointer
static int sbs_encode_dev(mgpu_ctx *c, const struct mgpu_sbs_args &a) {
    TextScratch w;
    if (int rc = text_scratch(c, a.n, &w)) return rc;
    const TextSbsParams p = {a.msgs, a.fields, a.positions, a.verdict, a.geom_delta, a.now_ms, a.override_squawk, a.flags};
    launch_sbs_encode(p, a.n, w, a.out, a.cap, a.deferred, a.verdict ? a.deferred_cap : 0, c->stream_aux);
    return text_finish(c, w, a.verdict != nullptr, a.cap, a.deferred_cap, a.bytes, a.ndeferred, a.nskipped, true);
}

static int raw_encode_dev(mgpu_ctx *c, const struct mgpu_raw_args &a) {
    TextScratch w;
    if (int rc = text_scratch(c, a.n, &w)) return rc;
    const bool gated = a.verdict && !(a.flags & MGPU_RAW_VERBATIM);
    const TextRawParams p = {a.msgs, gated ? a.verdict : nullptr, a.flags};
    launch_raw_encode(p, a.n, w, a.out, a.cap, a.deferred, gated ? a.deferred_cap : 0, c->stream_aux);
    return text_finish(c, w, gated, a.cap, a.deferred_cap, a.bytes, a.ndeferred, nullptr, false);
}

static bool sbs_args_ok(const struct mgpu_sbs_args *a, bool device) {
    if (!a || a->size < sizeof(struct mgpu_sbs_args) || !a->bytes) return false;
    if (a->flags & ~MGPU_SBS_USE_GNSS) return false;
    if (a->now_ms < 0 || a->now_ms >= 253402300800000ll) return false;       // years 1970-9999, as for every sysTimestamp
    if (a->n && (!a->msgs || !a->out || (device && !a->fields))) return false;
    if (a->verdict && (!a->ndeferred || (a->deferred_cap && !a->deferred))) return false;
    return true;
}

static bool raw_args_ok(const struct mgpu_raw_args *a) {
    if (!a || a->size < sizeof(struct mgpu_raw_args) || !a->bytes) return false;
    if (a->flags & ~(MGPU_RAW_NET_RULE | MGPU_RAW_VERBATIM | MGPU_RAW_MLAT)) return false;
    if (a->n && (!a->msgs || !a->out)) return false;
    const bool gated = a->verdict && !(a->flags & MGPU_RAW_VERBATIM);
    if (gated && (!a->ndeferred || (a->deferred_cap && !a->deferred))) return false;
    return true;
}

int mgpu_sbs_encode_ex_device(mgpu_ctx *c, const struct mgpu_sbs_args *a) {
    if (!c || !sbs_args_ok(a, true)) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, a->n, a->bytes, a->ndeferred, a->nskipped)) return *done;
    return sbs_encode_dev(c, *a);
}

int mgpu_sbs_encode_ex(mgpu_ctx *c, const struct mgpu_sbs_args *a) {
    if (!c || !sbs_args_ok(a, false)) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, a->n, a->bytes, a->ndeferred, a->nskipped)) return *done;
    Behind &b = *c->behind;
    const uint64_t n = a->n;
    struct mgpu_sbs_args d = *a;
    if (int rc = stage_list(c, &d.msgs, &d.fields, &d.verdict, n)) return rc;
    if (int rc = stage_optional(c, b.d_opt_pos, &d.positions, n)) return rc;
    if (int rc = stage_optional(c, b.d_opt_word, &d.geom_delta, n)) return rc;
    if (int rc = staged_out_reserve(c, a->cap, a->verdict != nullptr, a->deferred_cap, &d.out, &d.deferred)) return rc;
    if (int rc = sbs_encode_dev(c, d)) return rc;
    return staged_out_fetch(c, a->out, *a->bytes, a->deferred, a->verdict ? a->ndeferred : nullptr);
}

int mgpu_raw_encode_ex_device(mgpu_ctx *c, const struct mgpu_raw_args *a) {
    if (!c || !raw_args_ok(a)) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, a->n, a->bytes, a->ndeferred, nullptr)) return *done;
    return raw_encode_dev(c, *a);
}

int mgpu_raw_encode_ex(mgpu_ctx *c, const struct mgpu_raw_args *a) {
    if (!c || !raw_args_ok(a)) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, a->n, a->bytes, a->ndeferred, nullptr)) return *done;
    Behind &b = *c->behind;
    const uint64_t n = a->n;
    const bool gated = a->verdict && !(a->flags & MGPU_RAW_VERBATIM);
    if (int rc = stage_messages(c, a->msgs, n, gated ? a->verdict : nullptr)) return rc;
    struct mgpu_raw_args d = *a;
    if (int rc = staged_out_reserve(c, a->cap, gated, a->deferred_cap, &d.out, &d.deferred)) return rc;
    d.msgs = b.d_list.as<mgpu_msg>();
    d.verdict = gated ? b.d_list_verdict.as<uint8_t>() : nullptr;
    if (int rc = raw_encode_dev(c, d)) return rc;
    return staged_out_fetch(c, a->out, *a->bytes, a->deferred, gated ? a->ndeferred : nullptr);
}

// ---- ASTERIX CAT021 target reports (modesSendAsterixOutput, net_io.c:2416-2945), kernels/asterix.inc: a third job over the text outputs' scratch ----

// a: every array a device pointer
static int asterix_encode_dev(mgpu_ctx *c, const struct mgpu_asterix_args &a) {
    TextScratch w;
    if (int rc = text_scratch(c, a.n, &w)) return rc;
    const TextAsterixParams p = {a.msgs, a.fields, a.positions, a.verdict, (const unsigned long long *) a.ids, a.ac_baro_alt, a.ac_category, a.now_ms, a.flags};
    launch_asterix_encode(p, a.n, w, a.out, a.cap, a.deferred, a.verdict ? a.deferred_cap : 0, c->stream_aux);
    return text_finish(c, w, a.verdict != nullptr, a.cap, a.deferred_cap, a.bytes, a.ndeferred, a.nskipped, true);
}

static bool asterix_args_ok(const struct mgpu_asterix_args *a, bool device) {
    if (!a || a->size < sizeof(struct mgpu_asterix_args) || !a->bytes) return false;
    if (a->flags & ~MGPU_ASTERIX_REMOTE) return false;
    if (a->now_ms < 0 || a->now_ms >= 253402300800000ll) return false;       // years 1970-9999, as for the SBS lines
    if (a->n && (!a->msgs || !a->out || (device && !a->fields))) return false;
    if (a->verdict && (!a->ndeferred || (a->deferred_cap && !a->deferred))) return false;
    return true;
}

int mgpu_asterix_encode_ex_device(mgpu_ctx *c, const struct mgpu_asterix_args *a) {
    if (!c || !asterix_args_ok(a, true)) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, a->n, a->bytes, a->ndeferred, a->nskipped)) return *done;
    return asterix_encode_dev(c, *a);
}

int mgpu_asterix_encode_ex(mgpu_ctx *c, const struct mgpu_asterix_args *a) {
    if (!c || !asterix_args_ok(a, false)) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, a->n, a->bytes, a->ndeferred, a->nskipped)) return *done;
    Behind &b = *c->behind;
    const uint64_t n = a->n;
    struct mgpu_asterix_args d = *a;
    if (int rc = stage_list(c, &d.msgs, &d.fields, &d.verdict, n)) return rc;
    if (int rc = stage_optional(c, b.d_opt_pos, &d.positions, n)) return rc;
    if (int rc = stage_optional(c, b.d_opt_ids, &d.ids, n)) return rc;
    if (int rc = stage_optional(c, b.d_opt_word, &d.ac_baro_alt, n)) return rc;
    if (int rc = stage_optional(c, b.d_opt_byte, &d.ac_category, n)) return rc;
    if (int rc = staged_out_reserve(c, a->cap, a->verdict != nullptr, a->deferred_cap, &d.out, &d.deferred)) return rc;
    if (int rc = asterix_encode_dev(c, d)) return rc;
    return staged_out_fetch(c, a->out, *a->bytes, a->deferred, a->verdict ? a->ndeferred : nullptr);
}

// ---- the decoded-message dump (displayModesMessage, mode_s.c:1809-2239), kernels/dump.inc: the text outputs' workgroup scratch, a length word per message ----

// a: every array a device pointer
static int dump_encode_dev(mgpu_ctx *c, const struct mgpu_dump_args &a) {
    TextScratch t;
    if (int rc = text_scratch(c, a.n, &t, sizeof(uint32_t))) return rc;
    const DumpScratch w = {(uint32_t *) t.meta, t.blocks, t.off, t.total, t.stride};
    const DumpParams p = {a.msgs, a.fields, a.reduce_forward, (const unsigned long long *) a.receiver_ids, a.positions, a.decoded_nic, a.decoded_rc, a.flags, a.show_only};
    launch_dump_encode(p, a.n, w, a.out, a.cap, a.deferred, a.deferred_cap, c->stream_aux);
    return text_finish(c, t, true, a.cap, a.deferred_cap, a.bytes, a.ndeferred, a.nskipped, true);
}

static bool dump_args_ok(const struct mgpu_dump_args *a, bool device) {
    if (!a || a->size < sizeof(struct mgpu_dump_args) || !a->bytes) return false;
    if (a->flags & ~(MGPU_DUMP_ONLYADDR | MGPU_DUMP_RAW | MGPU_DUMP_MLAT | MGPU_DUMP_QUIET)) return false;
    if (a->n && (!a->msgs || (device && !a->fields))) return false;
    if ((a->cap && !a->out) || (a->deferred_cap && !a->deferred)) return false;
    return true;
}

int mgpu_dump_encode_ex_device(mgpu_ctx *c, const struct mgpu_dump_args *a) {
    if (!c || !dump_args_ok(a, true)) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, a->n, a->bytes, a->ndeferred, a->nskipped)) return *done;
    return dump_encode_dev(c, *a);
}

int mgpu_dump_encode_ex(mgpu_ctx *c, const struct mgpu_dump_args *a) {
    if (!c || !dump_args_ok(a, false)) return MGPU_E_INVAL;
    if (const auto done = encode_begin(c, a->n, a->bytes, a->ndeferred, a->nskipped)) return *done;
    Behind &b = *c->behind;
    const uint64_t n = a->n;
    struct mgpu_dump_args d = *a;
    if (int rc = stage_list(c, &d.msgs, &d.fields, nullptr, n)) return rc;
    if (int rc = stage_optional(c, b.d_opt_byte, &d.reduce_forward, n)) return rc;
    if (int rc = stage_optional(c, b.d_opt_ids, &d.receiver_ids, n)) return rc;
    if (int rc = stage_optional(c, b.d_opt_pos, &d.positions, n)) return rc;
    if (int rc = stage_optional(c, b.d_opt_byte2, &d.decoded_nic, n)) return rc;
    if (int rc = stage_optional(c, b.d_opt_word, &d.decoded_rc, n)) return rc;
    if (int rc = staged_out_reserve(c, a->cap, true, a->deferred_cap, &d.out, &d.deferred)) return rc;
    uint64_t nd = 0;
    d.ndeferred = &nd;
    const int rc = dump_encode_dev(c, d);
    if (a->ndeferred) *a->ndeferred = nd;
    if (rc) return rc;
    return staged_out_fetch(c, a->out, *a->bytes, a->deferred, &nd);
}

// the same formatter on the host, where log10 is the host libm's: no context, no GPU
int64_t mgpu_dump_format_host(const struct mgpu_dump_args *a, uint64_t index, uint8_t *text, uint64_t cap) {
    if (!a || a->size < sizeof(struct mgpu_dump_args) || !a->msgs || !a->fields || index >= a->n || (cap && !text)) return MGPU_E_INVAL;
    if (a->flags & ~(MGPU_DUMP_ONLYADDR | MGPU_DUMP_RAW | MGPU_DUMP_MLAT | MGPU_DUMP_QUIET)) return MGPU_E_INVAL;
    const DumpIn in = {a->msgs + index, a->fields + index, a->positions ? a->positions + index : nullptr, a->receiver_ids ? a->receiver_ids[index] : 0ull,
                       a->decoded_rc ? a->decoded_rc[index] : 0u, a->reduce_forward ? a->reduce_forward[index] : (uint8_t) 0,
                       a->decoded_nic ? a->decoded_nic[index] : (uint8_t) 0};
    if (dump_classify(in, a->flags, a->show_only, true) != DUMP_LINE) return 0;
    DumpCountSink count = {0};
    dump_format(in, a->flags, true, count);
    if (count.n > (uint32_t) kDumpMax) return MGPU_E_INVAL;      // (the bound is proved in dump_format.h; never trust a proof with a stack buffer)
    uint8_t buf[kDumpMax];
    DumpByteSink s = {buf};
    dump_format(in, a->flags, true, s);
    const uint64_t len = (uint64_t) (s.p - buf);
    if (cap) memcpy(text, buf, len < cap ? len : cap);
    return (int64_t) len;
}

// ---- the CRC and table diagnostics (no context, no GPU) ----

uint32_t mgpu_crc_checksum(const uint8_t *msg, int bits) { return crc_tables().checksum(msg, bits); }

static const std::vector<SyndromeEntry> &host_table(int nfix, int bits) {
    static std::vector<SyndromeEntry> cache[3][2];
    static bool built[3][2];
    const int n = nfix < 0 ? 0 : nfix > 2 ? 2 : nfix, b = bits == 56 ? 0 : 1;
    if (!built[n][b]) { cache[n][b] = build_syndrome_table(bits == 56 ? 56 : 112, n); built[n][b] = true; }
    return cache[n][b];
}

int mgpu_crc_diagnose(int nfix_crc, uint32_t syndrome, int bits, int *bit0, int *bit1) {
    if (bit0) *bit0 = -1;
    if (bit1) *bit1 = -1;
    if (syndrome == 0) return 0;
    const std::vector<SyndromeEntry> &t = host_table(nfix_crc, bits);
    size_t lo = 0, hi = t.size();
    while (lo < hi) {
        size_t mid = (lo + hi) / 2;
        if (t[mid].syndrome < syndrome) lo = mid + 1; else hi = mid;
    }
    if (lo == t.size() || t[lo].syndrome != syndrome) return -1;
    if (bit0) *bit0 = t[lo].bit0;
    if (bit1 && t[lo].nerr > 1) *bit1 = t[lo].bit1;
    return t[lo].nerr;
}

int mgpu_crc_table_size(int nfix_crc, int bits) { return (int) host_table(nfix_crc, bits).size(); }

const uint16_t *mgpu_uc8_table(void) { return uc8_table(); }

}  // extern "C"
