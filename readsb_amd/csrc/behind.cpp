// behind.cpp — behind the message list: beast encoder, field decode, tracking gate, position decode, the text outputs, and the CRC / table diagnostics.
#include "behind.h"

#include <cmath>
#include <cstring>

#include "dump_format.h"
#include "uat_format.h"
#include "sbs_in_format.h"
#include "raw_in_format.h"
#include "beast_in_host.h"
#include "asterix_in_format.h"

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

// host lists -> d_beast_in back to back (and, with `verdicts`, their verdict bytes -> d_beast_verdict; a list's may be null)
static int stage_messages(mgpu_ctx *c, const struct mgpu_msg *const *lists, const uint64_t *counts, uint32_t nlists, uint64_t n,
                          const uint8_t *const *verdicts = nullptr) {
    Behind &b = *c->behind;
    if (int rc = b.d_beast_in.reserve(c, n * sizeof(mgpu_msg))) return rc;
    if (verdicts)
        if (int rc = b.d_beast_verdict.reserve(c, n)) return rc;
    uint64_t at = 0;
    for (uint32_t k = 0; k < nlists; at += counts[k++]) {
        if (!counts[k]) continue;
        HIPCHK(c, hipMemcpyAsync(b.d_beast_in.as<mgpu_msg>() + at, lists[k], counts[k] * sizeof(mgpu_msg), hipMemcpyHostToDevice, c->stream_aux));
        if (verdicts && verdicts[k])
            HIPCHK(c, hipMemcpyAsync(b.d_beast_verdict.as<uint8_t>() + at, verdicts[k], counts[k], hipMemcpyHostToDevice, c->stream_aux));
    }
    return MGPU_OK;
}
static int stage_messages(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n, const uint8_t *verdict = nullptr) {
    return stage_messages(c, &msgs, &n, 1, n, verdict ? &verdict : nullptr);
}

// the encoder over the staged list (d_verdict / d_ids: the staged arrays it is to read, or null): stream -> out, deferred list -> deferred
static int beast_encode_staged(mgpu_ctx *c, const uint8_t *d_verdict, const uint64_t *d_ids, uint64_t n, uint32_t flags, uint8_t *out, uint64_t cap,
                               uint64_t *bytes, mgpu_deferred *deferred, uint64_t deferred_cap, uint64_t *ndeferred, uint64_t *last_id) {
    Behind &b = *c->behind;
    if (int rc = b.d_beast_out.reserve(c, cap + 64)) return rc;                        // (the encoder may store a vector past the stream's end)
    if (d_verdict)
        if (int rc = b.d_deferred.reserve(c, (deferred_cap + 64) * sizeof(mgpu_deferred))) return rc;
    if (int rc = beast_encode_dev(c, b.d_beast_in.as<mgpu_msg>(), d_verdict, n, flags, b.d_beast_out.as<uint8_t>(), cap, bytes, b.d_deferred.as<mgpu_deferred>(),
                                  deferred_cap, ndeferred, d_ids, last_id))
        return rc;
    HIPCHK(c, hipMemcpy(out, b.d_beast_out.p, *bytes, hipMemcpyDeviceToHost));
    if (ndeferred && *ndeferred) HIPCHK(c, hipMemcpy(deferred, b.d_deferred.p, *ndeferred * sizeof(mgpu_deferred), hipMemcpyDeviceToHost));
    return MGPU_OK;
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
    *a->bytes = 0;
    if (a->ndeferred) *a->ndeferred = 0;
    if (a->n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return beast_encode_dev(c, a->msgs, a->verdict, a->n, a->flags, a->out, a->cap, a->bytes, a->deferred, a->deferred_cap, a->ndeferred, a->ids, a->last_id);
}

int mgpu_beast_encode_ex(mgpu_ctx *c, const struct mgpu_beast_args *a) {
    if (!c || !beast_args_ok(a)) return MGPU_E_INVAL;
    *a->bytes = 0;
    if (a->ndeferred) *a->ndeferred = 0;
    const uint64_t n = a->n;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    const bool gated = a->verdict && !(a->flags & MGPU_BEAST_VERBATIM);
    if (int rc = stage_messages(c, a->msgs, n, gated ? a->verdict : nullptr)) return rc;
    if (a->ids) {
        if (int rc = b.d_beast_ids.reserve(c, n * sizeof(uint64_t))) return rc;
        HIPCHK(c, hipMemcpyAsync(b.d_beast_ids.p, a->ids, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream_aux));
    }
    return beast_encode_staged(c, gated ? b.d_beast_verdict.as<uint8_t>() : nullptr, a->ids ? b.d_beast_ids.as<uint64_t>() : nullptr, n, a->flags, a->out, a->cap,
                               a->bytes, a->deferred, a->deferred_cap, a->ndeferred, a->last_id);
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
    *bytes = 0; *ndeferred = 0;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
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
    // staged: the concatenation in d_beast_in, its verdicts in d_beast_verdict; results: records | permutation | ids | verdicts in d_merge_out
    if (int rc = stage_messages(c, segments, counts, nseg, n, verdict_in)) return rc;
    if (int rc = b.d_merge_out.reserve(c, n * (sizeof(mgpu_msg) + 8 + 8 + 1))) return rc;
    std::vector<const mgpu_msg *> d_seg(nseg);
    std::vector<const uint8_t *> d_ver(nseg);
    uint64_t at = 0;
    for (uint32_t k = 0; k < nseg; at += counts[k++]) {
        d_seg[k] = b.d_beast_in.as<mgpu_msg>() + at;
        d_ver[k] = counts[k] && verdict_in && verdict_in[k] ? b.d_beast_verdict.as<uint8_t>() + at : nullptr;
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

// host list -> d_beast_in, its field records -> d_fields
static int fields_staged(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n) {
    Behind &b = *c->behind;
    if (int rc = b.d_fields.reserve(c, n * sizeof(mgpu_fields))) return rc;
    if (int rc = stage_messages(c, msgs, n)) return rc;
    return fields_dev(c, b.d_beast_in.as<mgpu_msg>(), n, b.d_fields.as<mgpu_fields>());
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

// host list -> d_beast_in, its field records -> d_fields, its verdicts (continuing the context's aircraft table) -> d_gate_verdict
static int gate_staged(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n) {
    Behind &b = *c->behind;
    if (int rc = fields_staged(c, msgs, n)) return rc;
    if (int rc = b.d_gate_verdict.reserve(c, n)) return rc;
    if (int rc = gate_dev(c, b.d_beast_in.as<mgpu_msg>(), b.d_fields.as<mgpu_fields>(), n, b.d_gate_verdict.as<uint8_t>())) return rc;
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
    *bytes = 0; *ndeferred = 0;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
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
    if (int rc = cpr_track_dev(c, cfg, b.d_beast_in.as<mgpu_msg>(), b.d_fields.as<mgpu_fields>(), n, b.d_cpr_out.as<mgpu_position>())) return rc;
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

static int text_scratch(mgpu_ctx *c, uint64_t n, TextScratch *w) {
    Behind &b = *c->behind;
    const size_t nb = (size_t) (n / kBlock + 2);                 // per workgroup: bytes | deferred | skipped, nb entries each
    if (int rc = b.d_text_len.reserve(c, n * sizeof(uint16_t))) return rc;
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

// the staged outputs of a host-array form: room for them before the launch, the stream and the listed entries back after it
static int text_out_reserve(mgpu_ctx *c, uint64_t cap, bool gated, uint64_t deferred_cap) {
    Behind &b = *c->behind;
    if (int rc = b.d_beast_out.reserve(c, cap + 64)) return rc;
    if (gated)
        if (int rc = b.d_deferred.reserve(c, (deferred_cap + 64) * sizeof(mgpu_deferred))) return rc;
    return MGPU_OK;
}
static int text_out_fetch(mgpu_ctx *c, uint8_t *out, uint64_t bytes, struct mgpu_deferred *deferred, const uint64_t *ndeferred) {
    Behind &b = *c->behind;
    if (bytes) HIPCHK(c, hipMemcpy(out, b.d_beast_out.p, bytes, hipMemcpyDeviceToHost));
    if (ndeferred && *ndeferred) HIPCHK(c, hipMemcpy(deferred, b.d_deferred.p, *ndeferred * sizeof(mgpu_deferred), hipMemcpyDeviceToHost));
    return MGPU_OK;
}

int mgpu_sbs_encode_ex_device(mgpu_ctx *c, const struct mgpu_sbs_args *a) {
    if (!c || !sbs_args_ok(a, true)) return MGPU_E_INVAL;
    *a->bytes = 0;
    if (a->ndeferred) *a->ndeferred = 0;
    if (a->nskipped) *a->nskipped = 0;
    if (a->n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return sbs_encode_dev(c, *a);
}

int mgpu_sbs_encode_ex(mgpu_ctx *c, const struct mgpu_sbs_args *a) {
    if (!c || !sbs_args_ok(a, false)) return MGPU_E_INVAL;
    *a->bytes = 0;
    if (a->ndeferred) *a->ndeferred = 0;
    if (a->nskipped) *a->nskipped = 0;
    const uint64_t n = a->n;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    struct mgpu_sbs_args d = *a;
    if (a->fields) {
        if (int rc = stage_messages(c, a->msgs, n, a->verdict)) return rc;
        if (int rc = b.d_fields.reserve(c, n * sizeof(mgpu_fields))) return rc;
        HIPCHK(c, hipMemcpyAsync(b.d_fields.p, a->fields, n * sizeof(mgpu_fields), hipMemcpyHostToDevice, c->stream_aux));
    } else {
        if (int rc = fields_staged(c, a->msgs, n)) return rc;
        if (a->verdict) {
            if (int rc = b.d_beast_verdict.reserve(c, n)) return rc;
            HIPCHK(c, hipMemcpyAsync(b.d_beast_verdict.p, a->verdict, n, hipMemcpyHostToDevice, c->stream_aux));
        }
    }
    d.msgs = b.d_beast_in.as<mgpu_msg>();
    d.fields = b.d_fields.as<mgpu_fields>();
    if (a->verdict) d.verdict = b.d_beast_verdict.as<uint8_t>();
    if (a->positions) {
        if (int rc = b.d_text_pos.reserve(c, n * sizeof(mgpu_position))) return rc;
        HIPCHK(c, hipMemcpyAsync(b.d_text_pos.p, a->positions, n * sizeof(mgpu_position), hipMemcpyHostToDevice, c->stream_aux));
        d.positions = b.d_text_pos.as<mgpu_position>();
    }
    if (a->geom_delta) {
        if (int rc = b.d_text_delta.reserve(c, n * sizeof(int32_t))) return rc;
        HIPCHK(c, hipMemcpyAsync(b.d_text_delta.p, a->geom_delta, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream_aux));
        d.geom_delta = b.d_text_delta.as<int32_t>();
    }
    if (int rc = text_out_reserve(c, a->cap, a->verdict != nullptr, a->deferred_cap)) return rc;
    d.out = b.d_beast_out.as<uint8_t>();
    d.deferred = b.d_deferred.as<mgpu_deferred>();
    if (int rc = sbs_encode_dev(c, d)) return rc;
    return text_out_fetch(c, a->out, *a->bytes, a->deferred, a->verdict ? a->ndeferred : nullptr);
}

int mgpu_raw_encode_ex_device(mgpu_ctx *c, const struct mgpu_raw_args *a) {
    if (!c || !raw_args_ok(a)) return MGPU_E_INVAL;
    *a->bytes = 0;
    if (a->ndeferred) *a->ndeferred = 0;
    if (a->n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return raw_encode_dev(c, *a);
}

int mgpu_raw_encode_ex(mgpu_ctx *c, const struct mgpu_raw_args *a) {
    if (!c || !raw_args_ok(a)) return MGPU_E_INVAL;
    *a->bytes = 0;
    if (a->ndeferred) *a->ndeferred = 0;
    const uint64_t n = a->n;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    const bool gated = a->verdict && !(a->flags & MGPU_RAW_VERBATIM);
    if (int rc = stage_messages(c, a->msgs, n, gated ? a->verdict : nullptr)) return rc;
    if (int rc = text_out_reserve(c, a->cap, gated, a->deferred_cap)) return rc;
    struct mgpu_raw_args d = *a;
    d.msgs = b.d_beast_in.as<mgpu_msg>();
    d.verdict = gated ? b.d_beast_verdict.as<uint8_t>() : nullptr;
    d.out = b.d_beast_out.as<uint8_t>();
    d.deferred = b.d_deferred.as<mgpu_deferred>();
    if (int rc = raw_encode_dev(c, d)) return rc;
    return text_out_fetch(c, a->out, *a->bytes, a->deferred, gated ? a->ndeferred : nullptr);
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

// one optional host array into its staging buffer: -> the device copy through *dev (a null array stays null)
static int asterix_stage(mgpu_ctx *c, DevBuf &buf, const void *host, uint64_t bytes, const void **dev) {
    *dev = nullptr;
    if (!host) return MGPU_OK;
    if (int rc = buf.reserve(c, bytes)) return rc;
    HIPCHK(c, hipMemcpyAsync(buf.p, host, bytes, hipMemcpyHostToDevice, c->stream_aux));
    *dev = buf.p;
    return MGPU_OK;
}

int mgpu_asterix_encode_ex_device(mgpu_ctx *c, const struct mgpu_asterix_args *a) {
    if (!c || !asterix_args_ok(a, true)) return MGPU_E_INVAL;
    *a->bytes = 0;
    if (a->ndeferred) *a->ndeferred = 0;
    if (a->nskipped) *a->nskipped = 0;
    if (a->n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return asterix_encode_dev(c, *a);
}

int mgpu_asterix_encode_ex(mgpu_ctx *c, const struct mgpu_asterix_args *a) {
    if (!c || !asterix_args_ok(a, false)) return MGPU_E_INVAL;
    *a->bytes = 0;
    if (a->ndeferred) *a->ndeferred = 0;
    if (a->nskipped) *a->nskipped = 0;
    const uint64_t n = a->n;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    struct mgpu_asterix_args d = *a;
    if (a->fields) {
        if (int rc = stage_messages(c, a->msgs, n, a->verdict)) return rc;
        if (int rc = b.d_fields.reserve(c, n * sizeof(mgpu_fields))) return rc;
        HIPCHK(c, hipMemcpyAsync(b.d_fields.p, a->fields, n * sizeof(mgpu_fields), hipMemcpyHostToDevice, c->stream_aux));
    } else {
        if (int rc = fields_staged(c, a->msgs, n)) return rc;
        if (a->verdict) {
            if (int rc = b.d_beast_verdict.reserve(c, n)) return rc;
            HIPCHK(c, hipMemcpyAsync(b.d_beast_verdict.p, a->verdict, n, hipMemcpyHostToDevice, c->stream_aux));
        }
    }
    d.msgs = b.d_beast_in.as<mgpu_msg>();
    d.fields = b.d_fields.as<mgpu_fields>();
    if (a->verdict) d.verdict = b.d_beast_verdict.as<uint8_t>();
    const void *d_pos, *d_ids, *d_alt, *d_cat;
    if (int rc = asterix_stage(c, b.d_text_pos, a->positions, n * sizeof(mgpu_position), &d_pos)) return rc;
    if (int rc = asterix_stage(c, b.d_asx_ids, a->ids, n * sizeof(uint64_t), &d_ids)) return rc;
    if (int rc = asterix_stage(c, b.d_asx_baro_alt, a->ac_baro_alt, n * sizeof(int32_t), &d_alt)) return rc;
    if (int rc = asterix_stage(c, b.d_asx_category, a->ac_category, n, &d_cat)) return rc;
    d.positions = (const mgpu_position *) d_pos;
    d.ids = (const uint64_t *) d_ids;
    d.ac_baro_alt = (const int32_t *) d_alt;
    d.ac_category = (const uint8_t *) d_cat;
    if (int rc = text_out_reserve(c, a->cap, a->verdict != nullptr, a->deferred_cap)) return rc;
    d.out = b.d_beast_out.as<uint8_t>();
    d.deferred = b.d_deferred.as<mgpu_deferred>();
    if (int rc = asterix_encode_dev(c, d)) return rc;
    return text_out_fetch(c, a->out, *a->bytes, a->deferred, a->verdict ? a->ndeferred : nullptr);
}

// ---- the decoded-message dump (displayModesMessage, mode_s.c:1809-2239), kernels/dump.inc: the text outputs' workgroup scratch, a length word per message ----

// a: every array a device pointer
static int dump_encode_dev(mgpu_ctx *c, const struct mgpu_dump_args &a) {
    Behind &b = *c->behind;
    const size_t nb = (size_t) (a.n / kBlock + 2);                 // per workgroup: bytes | deferred | skipped, nb entries each
    if (int rc = b.d_text_blocks.reserve(c, 3 * nb * sizeof(uint32_t))) return rc;
    if (int rc = b.d_text_off.reserve(c, 3 * nb * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_text_total.reserve_exact(c, 4 * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_dump_len.reserve(c, a.n * sizeof(uint32_t))) return rc;
    const DumpScratch w = {b.d_dump_len.as<uint32_t>(), b.d_text_blocks.as<uint32_t>(), b.d_text_off.as<unsigned long long>(), b.d_text_total.as<unsigned long long>(), nb};
    const DumpParams p = {a.msgs, a.fields, a.reduce_forward, (const unsigned long long *) a.receiver_ids, a.positions, a.decoded_nic, a.decoded_rc, a.flags, a.show_only};
    launch_dump_encode(p, a.n, w, a.out, a.cap, a.deferred, a.deferred_cap, c->stream_aux);
    const TextScratch t = {nullptr, w.blocks, w.off, w.total, nb};
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
    *a->bytes = 0;
    if (a->ndeferred) *a->ndeferred = 0;
    if (a->nskipped) *a->nskipped = 0;
    if (a->n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return dump_encode_dev(c, *a);
}

int mgpu_dump_encode_ex(mgpu_ctx *c, const struct mgpu_dump_args *a) {
    if (!c || !dump_args_ok(a, false)) return MGPU_E_INVAL;
    *a->bytes = 0;
    if (a->ndeferred) *a->ndeferred = 0;
    if (a->nskipped) *a->nskipped = 0;
    const uint64_t n = a->n;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    struct mgpu_dump_args d = *a;
    if (a->fields) {
        if (int rc = stage_messages(c, a->msgs, n)) return rc;
        if (int rc = b.d_fields.reserve(c, n * sizeof(mgpu_fields))) return rc;
        HIPCHK(c, hipMemcpyAsync(b.d_fields.p, a->fields, n * sizeof(mgpu_fields), hipMemcpyHostToDevice, c->stream_aux));
    } else if (int rc = fields_staged(c, a->msgs, n)) return rc;
    d.msgs = b.d_beast_in.as<mgpu_msg>();
    d.fields = b.d_fields.as<mgpu_fields>();
    const void *d_rf, *d_ids, *d_pos, *d_nic, *d_rc;
    if (int rc = asterix_stage(c, b.d_dump_forward, a->reduce_forward, n, &d_rf)) return rc;
    if (int rc = asterix_stage(c, b.d_dump_ids, a->receiver_ids, n * sizeof(uint64_t), &d_ids)) return rc;
    if (int rc = asterix_stage(c, b.d_dump_pos, a->positions, n * sizeof(mgpu_position), &d_pos)) return rc;
    if (int rc = asterix_stage(c, b.d_dump_nic, a->decoded_nic, n, &d_nic)) return rc;
    if (int rc = asterix_stage(c, b.d_dump_rc, a->decoded_rc, n * sizeof(uint32_t), &d_rc)) return rc;
    d.reduce_forward = (const uint8_t *) d_rf;
    d.receiver_ids = (const uint64_t *) d_ids;
    d.positions = (const mgpu_position *) d_pos;
    d.decoded_nic = (const uint8_t *) d_nic;
    d.decoded_rc = (const uint32_t *) d_rc;
    if (int rc = text_out_reserve(c, a->cap, true, a->deferred_cap)) return rc;
    d.out = b.d_beast_out.as<uint8_t>();
    d.deferred = b.d_deferred.as<mgpu_deferred>();
    uint64_t nd = 0;
    d.ndeferred = &nd;
    const int rc = dump_encode_dev(c, d);
    if (a->ndeferred) *a->ndeferred = nd;
    if (rc) return rc;
    return text_out_fetch(c, a->out, *a->bytes, a->deferred, &nd);
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

// ---- UAT input: uat2esnt over dump978 downlink lines (uat_format.h, kernels/uat.inc) ----

struct UatCounts { uint64_t lines, consumed, frames, deferred, nshort; };

// a: text, out and the three per-frame arrays device pointers; a.deferred a HOST array.  The counts of this text; the deferred lines'
// indices (line_base added) to a.deferred[listed ..] as far as deferred_cap reaches.  Overflows are the caller's to judge.
static int uat_encode_dev(mgpu_ctx *c, const struct mgpu_uat_args &a, uint64_t line_base, uint64_t listed, UatCounts *n) {
    Behind &b = *c->behind;
    if (!b.d_uat_sig_table.p) {
        if (int rc = b.d_uat_sig_table.reserve_exact(c, kUatSigTable)) return rc;
        HIPCHK(c, hipMemcpy(b.d_uat_sig_table.p, uat_sig_table(), kUatSigTable, hipMemcpyHostToDevice));
    }
    const size_t nb = (size_t) (a.nbytes / kUatTile + 2);
    const uint64_t def_room = std::min<uint64_t>(a.deferred_cap > listed ? a.deferred_cap - listed : 0, uat_max_deferred(a.nbytes));   // (no more than the text can defer)
    if (int rc = b.d_uat_meta.reserve(c, nb * kBlock * sizeof(uint16_t))) return rc;
    if (int rc = b.d_uat_blocks.reserve(c, 5 * nb * sizeof(uint32_t))) return rc;
    if (int rc = b.d_uat_off.reserve(c, 3 * nb * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_uat_total.reserve_exact(c, 8 * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_uat_deferred.reserve(c, (def_room + 64) * sizeof(unsigned long long))) return rc;
    const UatScratch w = {b.d_uat_meta.as<uint16_t>(), b.d_uat_blocks.as<uint32_t>(), b.d_uat_off.as<unsigned long long>(), b.d_uat_total.as<unsigned long long>(), nb};
    const bool records = a.msgs || a.sig || a.line_of;
    const UatParams p = {a.text, a.nbytes, b.d_uat_sig_table.as<uint8_t>(), a.out, a.cap, a.msgs, a.sig, (unsigned long long *) a.line_of, records ? a.msgs_cap : 0,
                         b.d_uat_deferred.as<unsigned long long>(), def_room, line_base, a.now_ms};
    launch_uat_encode(p, w, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[5] = {0, 0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    *n = {total[0], total[1], total[2], total[3], total[4]};
    const uint64_t fetch = std::min<uint64_t>(total[3], def_room);
    if (fetch) HIPCHK(c, hipMemcpy(a.deferred + listed, b.d_uat_deferred.p, fetch * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return MGPU_OK;
}

static bool uat_args_ok(const struct mgpu_uat_args *a) {
    if (!a || a->size < sizeof(struct mgpu_uat_args) || !a->bytes || !a->consumed || !a->nlines || !a->nframes) return false;
    if (a->nbytes > kUatMaxBytes || a->cap > UINT64_MAX / 2) return false;
    if (a->nbytes && !a->text) return false;
    if ((a->cap && !a->out) || (a->deferred_cap && (!a->deferred || !a->ndeferred))) return false;
    if (a->nbytes && a->cap) {                                // out must not overlap text
        const uintptr_t i0 = (uintptr_t) a->text, i1 = i0 + a->nbytes, o0 = (uintptr_t) a->out, o1 = o0 + a->cap;
        if (i0 < o1 && o0 < i1) return false;
    }
    return true;
}

static void uat_report(const struct mgpu_uat_args *a, const UatCounts &n) {
    *a->bytes = n.frames * kUatFrameText;
    *a->consumed = n.consumed;
    *a->nlines = n.lines;
    *a->nframes = n.frames;
    if (a->nshort) *a->nshort = n.nshort;
    if (a->ndeferred) *a->ndeferred = n.deferred;
}

static int uat_verdict(mgpu_ctx *c, const struct mgpu_uat_args *a, const UatCounts &n) {
    if (n.frames * kUatFrameText > a->cap) { c->err = "uat encode: output buffer too small"; return MGPU_E_OVERFLOW; }
    if ((a->msgs || a->sig || a->line_of) && n.frames > a->msgs_cap) { c->err = "uat encode: more frames than the per-frame arrays hold"; return MGPU_E_OVERFLOW; }
    if (n.deferred > a->deferred_cap) { c->err = "uat encode: more deferred lines than the list holds"; return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

int mgpu_uat_encode_device(mgpu_ctx *c, const struct mgpu_uat_args *a) {
    if (!c || !uat_args_ok(a)) return MGPU_E_INVAL;
    UatCounts n = {0, 0, 0, 0, 0};
    uat_report(a, n);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = uat_encode_dev(c, *a, 0, 0, &n)) return rc;
    uat_report(a, n);
    return uat_verdict(c, a, n);
}

constexpr uint64_t kUatDefaultPass = 64ull << 20;            // bytes the host form stages per pass, pass_bytes == 0

int mgpu_uat_encode(mgpu_ctx *c, const struct mgpu_uat_args *a) {
    if (!c || !uat_args_ok(a)) return MGPU_E_INVAL;
    UatCounts all = {0, 0, 0, 0, 0};
    uat_report(a, all);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    const bool records = a->msgs || a->sig || a->line_of;
    uint64_t pass = std::min<uint64_t>(a->pass_bytes ? a->pass_bytes : kUatDefaultPass, a->nbytes);
    for (uint64_t at = 0; at < a->nbytes;) {
        const uint64_t nb = std::min<uint64_t>(pass, a->nbytes - at);
        // what this pass may write: what the caller's buffers still hold, and no more than nb bytes of text can give
        const uint64_t most = uat_max_frames(nb);
        const uint64_t out_room = a->cap > all.frames * kUatFrameText ? std::min<uint64_t>(a->cap - all.frames * kUatFrameText, most * kUatFrameText) : 0;
        const uint64_t rec_room = records && a->msgs_cap > all.frames ? std::min<uint64_t>(a->msgs_cap - all.frames, most) : 0;
        if (int rc = b.d_uat_in.reserve(c, nb + 64)) return rc;
        if (int rc = b.d_uat_out.reserve(c, out_room + 64)) return rc;
        struct mgpu_uat_args d = *a;
        d.text = b.d_uat_in.as<uint8_t>(); d.nbytes = nb;
        d.out = b.d_uat_out.as<uint8_t>(); d.cap = out_room;
        d.msgs = nullptr; d.sig = nullptr; d.line_of = nullptr; d.msgs_cap = rec_room;
        if (a->msgs) { if (int rc = b.d_uat_msgs.reserve(c, (rec_room + 1) * sizeof(mgpu_msg))) return rc; d.msgs = b.d_uat_msgs.as<mgpu_msg>(); }
        if (a->sig) { if (int rc = b.d_uat_sig.reserve(c, rec_room + 64)) return rc; d.sig = b.d_uat_sig.as<uint8_t>(); }
        if (a->line_of) { if (int rc = b.d_uat_line_of.reserve(c, (rec_room + 1) * sizeof(uint64_t))) return rc; d.line_of = b.d_uat_line_of.as<uint64_t>(); }
        HIPCHK(c, hipMemcpyAsync(b.d_uat_in.p, a->text + at, nb, hipMemcpyHostToDevice, c->stream_aux));
        UatCounts n;
        if (int rc = uat_encode_dev(c, d, all.lines, std::min<uint64_t>(all.deferred, a->deferred_cap), &n)) return rc;
        if (n.consumed == 0 && at + nb < a->nbytes) {         // a line longer than the pass: a larger pass
            pass = pass > a->nbytes / 2 ? a->nbytes : 2 * pass;
            continue;
        }
        // (the pass stored the bytes and records below its rooms only: the copies stay inside the caller's buffers)
        const uint64_t nout = std::min<uint64_t>(n.frames * kUatFrameText, out_room), nrec = std::min<uint64_t>(n.frames, rec_room);
        if (nout) HIPCHK(c, hipMemcpy(a->out + all.frames * kUatFrameText, d.out, nout, hipMemcpyDeviceToHost));
        if (nrec && a->msgs) HIPCHK(c, hipMemcpy(a->msgs + all.frames, d.msgs, nrec * sizeof(mgpu_msg), hipMemcpyDeviceToHost));
        if (nrec && a->sig) HIPCHK(c, hipMemcpy(a->sig + all.frames, d.sig, nrec, hipMemcpyDeviceToHost));
        if (nrec && a->line_of) HIPCHK(c, hipMemcpy(a->line_of + all.frames, d.line_of, nrec * sizeof(uint64_t), hipMemcpyDeviceToHost));
        all.lines += n.lines; all.frames += n.frames; all.deferred += n.deferred; all.nshort += n.nshort;
        if (n.consumed == 0) break;                           // the rest has no '\n'
        at += n.consumed;
        all.consumed = at;
    }
    uat_report(a, all);
    return uat_verdict(c, a, all);
}

// ---- SBS input: decodeSbsLine over BaseStation lines (sbs_in_format.h, kernels/sbs_in.inc) ----

struct SbsInCounts { uint64_t lines, consumed, recs, deferred, invalid; };

// a: text, recs and line_of device pointers; a.deferred a HOST array.  The counts of this text; the deferred lines' indices (line_base
// added) to a.deferred[listed ..] as far as deferred_cap reaches.  Overflows are the caller's to judge.
static int sbs_decode_dev(mgpu_ctx *c, const struct mgpu_sbs_in_args &a, uint64_t line_base, uint64_t listed, SbsInCounts *n) {
    Behind &b = *c->behind;
    const size_t nb = (size_t) (a.nbytes / kUatTile + 2);
    const uint64_t def_room = std::min<uint64_t>(a.deferred_cap > listed ? a.deferred_cap - listed : 0, sbs_in_max_recs(a.nbytes));   // (no more than the text can defer)
    if (int rc = b.d_sbs_in_meta.reserve(c, nb * kBlock * sizeof(uint16_t))) return rc;
    if (int rc = b.d_sbs_in_blocks.reserve(c, 5 * nb * sizeof(uint32_t))) return rc;
    if (int rc = b.d_sbs_in_off.reserve(c, 3 * nb * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_sbs_in_total.reserve_exact(c, 8 * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_sbs_in_deferred.reserve(c, (def_room + 64) * sizeof(unsigned long long))) return rc;
    const UatScratch w = {b.d_sbs_in_meta.as<uint16_t>(), b.d_sbs_in_blocks.as<uint32_t>(), b.d_sbs_in_off.as<unsigned long long>(), b.d_sbs_in_total.as<unsigned long long>(), nb};
    const SbsInParams p = {a.text, a.nbytes, a.recs, (unsigned long long *) a.line_of, a.recs ? a.recs_cap : 0, b.d_sbs_in_deferred.as<unsigned long long>(), def_room,
                           line_base, a.now_ms, a.source};
    launch_sbs_decode(p, w, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[5] = {0, 0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    *n = {total[0], total[1], total[2], total[3], total[4]};
    const uint64_t fetch = std::min<uint64_t>(total[3], def_room);
    if (fetch) HIPCHK(c, hipMemcpy(a.deferred + listed, b.d_sbs_in_deferred.p, fetch * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return MGPU_OK;
}

static bool sbs_in_args_ok(const struct mgpu_sbs_in_args *a) {
    if (!a || a->size < sizeof(struct mgpu_sbs_in_args) || !a->consumed || !a->nlines || !a->nrecs) return false;
    if (!sbs_in_source_ok(a->source) || a->nbytes > kUatMaxBytes || a->recs_cap > UINT64_MAX / sizeof(mgpu_sbs_rec)) return false;
    if (a->nbytes && !a->text) return false;
    if ((a->recs_cap && !a->recs) || (a->deferred_cap && (!a->deferred || !a->ndeferred))) return false;
    return true;
}

static void sbs_in_report(const struct mgpu_sbs_in_args *a, const SbsInCounts &n) {
    *a->consumed = n.consumed;
    *a->nlines = n.lines;
    *a->nrecs = n.recs;
    if (a->ninvalid) *a->ninvalid = n.invalid;
    if (a->ndeferred) *a->ndeferred = n.deferred;
}

static int sbs_in_verdict(mgpu_ctx *c, const struct mgpu_sbs_in_args *a, const SbsInCounts &n) {
    if (n.recs > a->recs_cap) { c->err = "sbs decode: more records than the array holds"; return MGPU_E_OVERFLOW; }
    if (n.deferred > a->deferred_cap) { c->err = "sbs decode: more deferred lines than the list holds"; return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

int mgpu_sbs_decode_device(mgpu_ctx *c, const struct mgpu_sbs_in_args *a) {
    if (!c || !sbs_in_args_ok(a)) return MGPU_E_INVAL;
    if (((uintptr_t) a->recs | (uintptr_t) a->line_of) & 7u) return MGPU_E_INVAL;
    SbsInCounts n = {0, 0, 0, 0, 0};
    sbs_in_report(a, n);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = sbs_decode_dev(c, *a, 0, 0, &n)) return rc;
    sbs_in_report(a, n);
    return sbs_in_verdict(c, a, n);
}

int mgpu_sbs_decode(mgpu_ctx *c, const struct mgpu_sbs_in_args *a) {
    if (!c || !sbs_in_args_ok(a)) return MGPU_E_INVAL;
    SbsInCounts all = {0, 0, 0, 0, 0};
    sbs_in_report(a, all);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    uint64_t pass = std::min<uint64_t>(a->pass_bytes ? a->pass_bytes : kUatDefaultPass, a->nbytes);
    for (uint64_t at = 0; at < a->nbytes;) {
        const uint64_t nb = std::min<uint64_t>(pass, a->nbytes - at);
        // what this pass may write: what the caller's arrays still hold, and no more than nb bytes of text can give
        const uint64_t rec_room = a->recs_cap > all.recs ? std::min<uint64_t>(a->recs_cap - all.recs, sbs_in_max_recs(nb)) : 0;
        if (int rc = b.d_sbs_in_text.reserve(c, nb + 64)) return rc;
        if (int rc = b.d_sbs_in_recs.reserve(c, (rec_room + 1) * sizeof(mgpu_sbs_rec))) return rc;
        struct mgpu_sbs_in_args d = *a;
        d.text = b.d_sbs_in_text.as<uint8_t>(); d.nbytes = nb;
        d.recs = b.d_sbs_in_recs.as<mgpu_sbs_rec>(); d.recs_cap = rec_room;
        d.line_of = nullptr;
        if (a->line_of) { if (int rc = b.d_sbs_in_line_of.reserve(c, (rec_room + 1) * sizeof(uint64_t))) return rc; d.line_of = b.d_sbs_in_line_of.as<uint64_t>(); }
        HIPCHK(c, hipMemcpyAsync(b.d_sbs_in_text.p, a->text + at, nb, hipMemcpyHostToDevice, c->stream_aux));
        SbsInCounts n;
        if (int rc = sbs_decode_dev(c, d, all.lines, std::min<uint64_t>(all.deferred, a->deferred_cap), &n)) return rc;
        if (n.consumed == 0 && at + nb < a->nbytes) {         // a line longer than the pass: a larger pass
            pass = pass > a->nbytes / 2 ? a->nbytes : 2 * pass;
            continue;
        }
        // (the pass stored the records below its room only: the copies stay inside the caller's arrays)
        const uint64_t nrec = std::min<uint64_t>(n.recs, rec_room);
        if (nrec) HIPCHK(c, hipMemcpy(a->recs + all.recs, d.recs, nrec * sizeof(mgpu_sbs_rec), hipMemcpyDeviceToHost));
        if (nrec && a->line_of) HIPCHK(c, hipMemcpy(a->line_of + all.recs, d.line_of, nrec * sizeof(uint64_t), hipMemcpyDeviceToHost));
        all.lines += n.lines; all.recs += n.recs; all.deferred += n.deferred; all.invalid += n.invalid;
        if (n.consumed == 0) break;                           // the rest has no terminator
        at += n.consumed;
        all.consumed = at;
    }
    sbs_in_report(a, all);
    return sbs_in_verdict(c, a, all);
}

// ---- Raw input: decodeHexMessage + the front of decodeModesMessage over AVR lines (raw_in_format.h, kernels/raw_in.inc) ----

struct RawInCounts {
    uint64_t lines = 0, consumed = 0, msgs = 0;
    uint64_t cn[7] = {0, 0, 0, 0, 0, 0, 0};
};

// The filter passes' side of a call (launch_raw_in_resolve), shared with the beast input: the candidate arrays and the tables reserved,
// the filter's generations scattered into their bitmaps, p's candidate, table and filter fields set.
struct RawInResolve {
    uint32_t *d_members, *gen_active, *gen_inactive;
    uint32_t na, ni;
};
static int raw_in_resolve_begin(mgpu_ctx *c, uint64_t cand_cap, RawInParams &p, RawInResolve &r) {
    Behind &b = *c->behind;
    const uint64_t ncb = cand_cap / kBlock + 1;
    if (int rc = b.d_raw_in_cand_rec.reserve(c, cand_cap * sizeof(mgpu_msg))) return rc;
    if (int rc = b.d_raw_in_cand_sig.reserve(c, cand_cap * sizeof(double))) return rc;
    if (int rc = b.d_raw_in_cand_line.reserve(c, cand_cap * sizeof(uint32_t))) return rc;
    if (int rc = b.d_raw_in_cand_meta.reserve(c, cand_cap * sizeof(uint32_t))) return rc;
    if (int rc = b.d_raw_in_new_adds.reserve(c, cand_cap * sizeof(uint32_t))) return rc;
    if (int rc = b.d_raw_in_cb.reserve(c, 8 * ncb * sizeof(uint32_t))) return rc;
    if (int rc = b.d_raw_in_co.reserve(c, 2 * ncb * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_raw_in_misc.reserve_exact(c, 16 * sizeof(unsigned long long))) return rc;
    if (!b.d_raw_in_first.p) {                                  // the tables, once: first[] all ones, the bitmaps zero, the CRC's bytes
        if (int rc = b.d_raw_in_first.reserve_exact(c, (uint64_t) sizeof(uint32_t) << 24)) return rc;
        HIPCHK(c, hipMemsetAsync(b.d_raw_in_first.p, 0xff, (size_t) sizeof(uint32_t) << 24, c->stream_aux));
    }
    if (!b.d_raw_in_gen.p) {
        if (int rc = b.d_raw_in_gen.reserve_exact(c, 2 * ((1u << 24) / 8))) return rc;
        HIPCHK(c, hipMemsetAsync(b.d_raw_in_gen.p, 0, 2 * ((1u << 24) / 8), c->stream_aux));
    }
    if (!b.d_raw_in_crc.p) {
        if (int rc = b.d_raw_in_crc.reserve_exact(c, 256 * sizeof(uint32_t))) return rc;
        HIPCHK(c, hipMemcpy(b.d_raw_in_crc.p, crc_tables().byte_table, 256 * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    // the filter's generations into their bitmaps
    IcaoFilter &flt = c->resolver.filter();
    const std::vector<uint32_t> &ma = flt.members(true), &mi = flt.members(false);
    r.na = (uint32_t) ma.size(); r.ni = (uint32_t) mi.size();
    if (int rc = b.d_raw_in_members.reserve(c, ((uint64_t) r.na + r.ni + 1) * sizeof(uint32_t))) return rc;
    r.d_members = b.d_raw_in_members.as<uint32_t>(); r.gen_active = b.d_raw_in_gen.as<uint32_t>(); r.gen_inactive = r.gen_active + (1u << 24) / 32;
    if (r.na) HIPCHK(c, hipMemcpyAsync(r.d_members, ma.data(), r.na * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream_aux));
    if (r.ni) HIPCHK(c, hipMemcpyAsync(r.d_members + r.na, mi.data(), r.ni * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream_aux));
    launch_raw_in_scatter(r.d_members, r.na, r.gen_active, 1, c->stream_aux);
    launch_raw_in_scatter(r.d_members + r.na, r.ni, r.gen_inactive, 1, c->stream_aux);
    // occupied > buckets / 3 makes the table grow (icao_filter.c:127); between calls occupied <= buckets / 3
    const uint64_t buckets = 1ull << flt.table_bits(), third = buckets / 3;
    const uint64_t kstar = flt.table_bits() >= 20 ? 0 : (flt.occupied() <= third ? third - flt.occupied() + 1 : 1);
    p.cfg = RawInConfig{c->cfg.nfix_crc, c->cfg.fixDF, (int32_t) c->cfg.mode_ac};
    p.tb = RawInTables{b.d_raw_in_crc.as<uint32_t>(), c->d_tab_long, c->d_tab_short, (uint32_t) c->n_long, (uint32_t) c->n_short};
    p.cand_rec = b.d_raw_in_cand_rec.as<mgpu_msg>(); p.cand_sig = b.d_raw_in_cand_sig.as<double>();
    p.cand_line = b.d_raw_in_cand_line.as<uint32_t>(); p.cand_meta = b.d_raw_in_cand_meta.as<uint32_t>(); p.cand_cap = cand_cap;
    p.gen_active = r.gen_active; p.gen_inactive = r.gen_inactive; p.first = b.d_raw_in_first.as<uint32_t>();
    p.new_adds = b.d_raw_in_new_adds.as<uint32_t>(); p.kstar = kstar;
    return MGPU_OK;
}

// The passes over ncand candidates, the bitmaps put back, the stream drained; misc[16] as launch_raw_in_resolve leaves it (zeros for no
// candidates); the new adds appended to *adds and moved into the context's filter.  ncls: bytes of p.line_class to zero first.
static int raw_in_resolve_end(mgpu_ctx *c, const RawInParams &p, const RawInResolve &r, uint64_t ncand, size_t ncls, unsigned long long *misc, std::vector<uint32_t> *adds) {
    Behind &b = *c->behind;
    memset(misc, 0, 16 * sizeof(unsigned long long));
    if (ncand) {
        unsigned long long *d_misc = b.d_raw_in_misc.as<unsigned long long>();
        HIPCHK(c, hipMemsetAsync(d_misc, 0, 16 * sizeof(unsigned long long), c->stream_aux));
        HIPCHK(c, hipMemsetAsync(d_misc + 8, 0xff, sizeof(unsigned long long), c->stream_aux));
        if (ncls) HIPCHK(c, hipMemsetAsync(p.line_class, 0, ncls, c->stream_aux));
        launch_raw_in_resolve(p, (uint32_t) ncand, b.d_raw_in_cb.as<uint32_t>(), b.d_raw_in_co.as<unsigned long long>(), d_misc, c->stream_aux);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(misc, d_misc, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream_aux));
    } else if (ncls) HIPCHK(c, hipMemsetAsync(p.line_class, 0, ncls, c->stream_aux));
    launch_raw_in_scatter(r.d_members, r.na, r.gen_active, 0, c->stream_aux);
    launch_raw_in_scatter(r.d_members + r.na, r.ni, r.gen_inactive, 0, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    if (misc[9]) {                                              // the new adds, in the reference's order, into the context's filter
        IcaoFilter &flt = c->resolver.filter();
        const size_t at = adds->size();
        adds->resize(at + misc[9]);
        HIPCHK(c, hipMemcpy(adds->data() + at, p.new_adds, misc[9] * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t k = at; k < adds->size(); ++k) flt.add((*adds)[k]);
    }
    return MGPU_OK;
}

// a: text, msgs, line_of, signal_level, line_class device pointers, the capacities what this text may store (line_class indexed by
// this text's own lines).  The counts of this text; the context's filter moved on by the text's new adds, which are appended to
// *adds (the caller publishes them to the pre-screen's bitmap, or puts the filter back).
static int raw_decode_passes(mgpu_ctx *c, const struct mgpu_raw_in_args &a, uint64_t line_base, RawInCounts *n, std::vector<uint32_t> *adds) {
    Behind &b = *c->behind;
    const size_t nb = (size_t) (a.nbytes / kUatTile + 2);
    const uint64_t cand_cap = raw_in_max_cands(a.nbytes);
    if (int rc = b.d_raw_in_meta.reserve(c, nb * kBlock * sizeof(uint16_t))) return rc;
    if (int rc = b.d_raw_in_blocks.reserve(c, 5 * nb * sizeof(uint32_t))) return rc;
    if (int rc = b.d_raw_in_off.reserve(c, 3 * nb * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_raw_in_total.reserve_exact(c, 8 * sizeof(unsigned long long))) return rc;
    RawInParams p;
    RawInResolve r;
    if (int rc = raw_in_resolve_begin(c, cand_cap, p, r)) return rc;

    const UatScratch w = {b.d_raw_in_meta.as<uint16_t>(), b.d_raw_in_blocks.as<uint32_t>(), b.d_raw_in_off.as<unsigned long long>(), b.d_raw_in_total.as<unsigned long long>(), nb};
    p.text = a.text; p.nbytes = a.nbytes; p.now_ms = a.now_ms;
    p.msgs = a.msgs; p.line_of = (unsigned long long *) a.line_of; p.signal_level = a.signal_level; p.msgs_cap = a.msgs ? a.msgs_cap : 0;
    p.line_class = a.line_class; p.line_class_cap = a.line_class ? a.line_class_cap : 0; p.line_base = line_base;
    launch_raw_in_front(p, w, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    unsigned long long misc[16];
    int rc = MGPU_OK;
    const size_t ncls = p.line_class ? (size_t) std::min<uint64_t>(total[0], p.line_class_cap) : 0;   // "not a frame" is 0: only candidates store a class
    if (total[2] > cand_cap) { c->err = "raw decode: more candidates than the text can hold"; rc = MGPU_E_OVERFLOW; }   // (cannot happen: raw_in_max_cands)
    if (int rc2 = raw_in_resolve_end(c, p, r, rc ? 0 : total[2], rc ? 0 : ncls, misc, adds)) return rc2;
    if (rc) return rc;
    n->lines = total[0]; n->consumed = total[1]; n->msgs = misc[10];
    for (int k = 1; k < 7; ++k) n->cn[k] = misc[k];
    n->cn[0] = misc[2] + misc[3] + misc[4] + misc[5] + misc[6];   // remote_received_modes: every Mode S line that reached the decode
    return MGPU_OK;
}

// The generation bitmaps are zero and first[] is all ones OUTSIDE a call: a call that ends early (a HIP error between the scatter-in
// and the passes that put them back) gives the three tables up, and the next call allocates and initialises them again.
static int raw_decode_dev(mgpu_ctx *c, const struct mgpu_raw_in_args &a, uint64_t line_base, RawInCounts *n, std::vector<uint32_t> *adds) {
    const int rc = raw_decode_passes(c, a, line_base, n, adds);
    if (rc != MGPU_OK) {
        (void) hipStreamSynchronize(c->stream_aux);
        c->behind->d_raw_in_first.release();
        c->behind->d_raw_in_gen.release();
    }
    return rc;
}

static bool raw_in_args_ok(const struct mgpu_raw_in_args *a) {
    if (!a || a->size < sizeof(struct mgpu_raw_in_args) || !a->consumed || !a->nlines || !a->nmsgs || !a->counters) return false;
    if (a->nbytes >= (1ull << 32) || a->msgs_cap > UINT64_MAX / sizeof(mgpu_msg)) return false;
    if (a->now_ms < 0 || a->now_ms >= 253402300800000ll) return false;
    if (a->nbytes && !a->text) return false;
    if ((a->msgs_cap && !a->msgs) || (a->line_class_cap && !a->line_class)) return false;
    return true;
}

static void raw_in_report(const struct mgpu_raw_in_args *a, const RawInCounts &n) {
    *a->consumed = n.consumed;
    *a->nlines = n.lines;
    *a->nmsgs = n.msgs;
    struct mgpu_raw_in_counters &k = *a->counters;
    k.remote_received_modes = n.cn[0]; k.remote_received_modeac = n.cn[1]; k.remote_rejected_unknown_icao = n.cn[2]; k.remote_rejected_bad = n.cn[3];
    for (int i = 0; i < 3; ++i) k.remote_accepted[i] = n.cn[4 + i];
}

// the end of a call: on overflow the filter goes back to where it stood; otherwise the pre-screen learns the new addresses, as
// mgpu_filter_add teaches it one (nothing is in flight behind the drain)
// the pre-screen learns the addresses a call added to the filter, as mgpu_filter_add teaches it one (nothing is in flight behind the
// drain); the raw input's and the beast input's
static int raw_in_publish_adds(mgpu_ctx *c, const std::vector<uint32_t> &adds) {
    if (adds.empty()) return MGPU_OK;
    Behind &b = *c->behind;
    if (int rc = b.d_raw_in_members.reserve(c, adds.size() * sizeof(uint32_t))) return rc;
    HIPCHK(c, hipMemcpyAsync(b.d_raw_in_members.p, adds.data(), adds.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream_aux));
    launch_raw_in_scatter(b.d_raw_in_members.as<uint32_t>(), (uint32_t) adds.size(), c->d_adder_bitmap, 1, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

static int raw_in_finish(mgpu_ctx *c, const struct mgpu_raw_in_args *a, const RawInCounts &n, const IcaoFilter::Snapshot &before, const std::vector<uint32_t> &adds) {
    if (n.msgs > a->msgs_cap || (a->line_class && n.lines > a->line_class_cap)) {
        c->resolver.filter().restore(before);
        c->err = n.msgs > a->msgs_cap ? "raw decode: more messages than the array holds" : "raw decode: more lines than line_class holds";
        return MGPU_E_OVERFLOW;
    }
    return raw_in_publish_adds(c, adds);
}

int mgpu_raw_decode_device(mgpu_ctx *c, const struct mgpu_raw_in_args *a) {
    if (!c || !raw_in_args_ok(a)) return MGPU_E_INVAL;
    if (((uintptr_t) a->msgs | (uintptr_t) a->line_of | (uintptr_t) a->signal_level) & 7u) return MGPU_E_INVAL;
    RawInCounts n;
    raw_in_report(a, n);
    if (a->nbytes == 0) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    IcaoFilter::Snapshot before;
    c->resolver.filter().snapshot(before);
    std::vector<uint32_t> adds;
    if (int rc = raw_decode_dev(c, *a, 0, &n, &adds)) { c->resolver.filter().restore(before); return rc; }
    raw_in_report(a, n);
    return raw_in_finish(c, a, n, before, adds);
}

int mgpu_raw_decode(mgpu_ctx *c, const struct mgpu_raw_in_args *a) {
    if (!c || !raw_in_args_ok(a)) return MGPU_E_INVAL;
    RawInCounts all;
    raw_in_report(a, all);
    if (a->nbytes == 0) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    IcaoFilter::Snapshot before;
    c->resolver.filter().snapshot(before);
    std::vector<uint32_t> adds;
    uint64_t pass = std::min<uint64_t>(a->pass_bytes ? a->pass_bytes : kUatDefaultPass, a->nbytes);
    for (uint64_t at = 0; at < a->nbytes;) {
        const uint64_t nb = std::min<uint64_t>(pass, a->nbytes - at);
        // what this pass may write: what the caller's arrays still hold, and no more than nb bytes of text can give
        const uint64_t msg_room = a->msgs_cap > all.msgs ? std::min<uint64_t>(a->msgs_cap - all.msgs, raw_in_max_cands(nb)) : 0;
        const uint64_t cls_room = a->line_class_cap > all.lines ? std::min<uint64_t>(a->line_class_cap - all.lines, nb) : 0;
        int rc;
        if ((rc = b.d_raw_in_text.reserve(c, nb + 64)) || (rc = b.d_raw_in_msgs.reserve(c, (msg_room + 1) * sizeof(mgpu_msg))) ||
            (rc = b.d_raw_in_line_of.reserve(c, (msg_room + 1) * sizeof(uint64_t))) || (rc = b.d_raw_in_sig.reserve(c, (msg_room + 1) * sizeof(double))) ||
            (rc = b.d_raw_in_cls.reserve(c, cls_room + 1))) { c->resolver.filter().restore(before); return rc; }
        struct mgpu_raw_in_args d = *a;
        d.text = b.d_raw_in_text.as<uint8_t>(); d.nbytes = nb;
        d.msgs = b.d_raw_in_msgs.as<mgpu_msg>(); d.msgs_cap = msg_room;
        d.line_of = a->line_of ? b.d_raw_in_line_of.as<uint64_t>() : nullptr;
        d.signal_level = a->signal_level ? b.d_raw_in_sig.as<double>() : nullptr;
        d.line_class = a->line_class ? b.d_raw_in_cls.as<uint8_t>() : nullptr; d.line_class_cap = cls_room;
        HIPCHK(c, hipMemcpyAsync(b.d_raw_in_text.p, a->text + at, nb, hipMemcpyHostToDevice, c->stream_aux));
        RawInCounts n;
        const size_t adds_before = adds.size();
        IcaoFilter::Snapshot pass_before;
        const bool may_repeat = at + nb < a->nbytes;
        if (may_repeat) c->resolver.filter().snapshot(pass_before);
        if ((rc = raw_decode_dev(c, d, all.lines, &n, &adds))) { c->resolver.filter().restore(before); return rc; }
        if (n.consumed == 0 && may_repeat) {                  // a line longer than the pass: a larger pass, from the same filter
            c->resolver.filter().restore(pass_before);
            adds.resize(adds_before);
            pass = pass > a->nbytes / 2 ? a->nbytes : 2 * pass;
            continue;
        }
        // (the pass stored below its rooms only: the copies stay inside the caller's arrays)
        const uint64_t nmsg = std::min<uint64_t>(n.msgs, msg_room), ncls = std::min<uint64_t>(n.lines, cls_room);
        if (nmsg) HIPCHK(c, hipMemcpy(a->msgs + all.msgs, d.msgs, nmsg * sizeof(mgpu_msg), hipMemcpyDeviceToHost));
        if (nmsg && a->line_of) HIPCHK(c, hipMemcpy(a->line_of + all.msgs, d.line_of, nmsg * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (nmsg && a->signal_level) HIPCHK(c, hipMemcpy(a->signal_level + all.msgs, d.signal_level, nmsg * sizeof(double), hipMemcpyDeviceToHost));
        if (ncls && a->line_class) HIPCHK(c, hipMemcpy(a->line_class + all.lines, d.line_class, ncls, hipMemcpyDeviceToHost));
        all.lines += n.lines; all.msgs += n.msgs;
        for (int k = 0; k < 7; ++k) all.cn[k] += n.cn[k];
        if (n.consumed == 0) break;                           // the rest has no terminator
        at += n.consumed;
        all.consumed = at;
    }
    raw_in_report(a, all);
    return raw_in_finish(c, a, all, before, adds);
}

// ---- Beast input: readBeast + decodeBinMessage over a binary stream (beast_in_format.h, kernels/beast_in.inc) ----

// a: data and the per-message / per-call arrays device pointers, the capacities what this stretch may store (frame_class and frame_off
// indexed by this stretch's own handler calls); frame_base and off_base are added to frame_of and frame_off.  final: the tail rule
// applies.  The counts of this stretch; the filter moved on as in raw_decode_passes.
static int beast_decode_passes(mgpu_ctx *c, const struct mgpu_beast_in_args &a, uint64_t frame_base, uint64_t off_base, bool final, BeastInCounts *n,
                               std::vector<uint32_t> *adds) {
    Behind &b = *c->behind;
    const size_t tiles = beast_in_tiles(a.nbytes), groups = beast_in_groups(a.nbytes);
    const uint64_t cand_cap = beast_in_max_msgs(a.nbytes);
    if (int rc = b.d_bin_maps.reserve(c, tiles * 64)) return rc;
    if (int rc = b.d_bin_gmaps.reserve(c, groups * 64)) return rc;
    if (int rc = b.d_bin_entry.reserve(c, (tiles + groups) * sizeof(uint32_t))) return rc;
    if (int rc = b.d_bin_marks.reserve(c, tiles * kBlock * sizeof(uint32_t))) return rc;
    if (int rc = b.d_bin_meta.reserve(c, tiles * kBlock * sizeof(uint16_t))) return rc;
    if (int rc = b.d_bin_lane_ids.reserve(c, tiles * kBlock * sizeof(uint64_t))) return rc;
    if (int rc = b.d_bin_blocks.reserve(c, 6 * tiles * sizeof(uint32_t))) return rc;
    if (int rc = b.d_bin_off.reserve(c, 2 * tiles * sizeof(uint64_t))) return rc;
    if (int rc = b.d_bin_tile_id.reserve(c, tiles * sizeof(uint64_t))) return rc;
    if (int rc = b.d_bin_entry_id.reserve(c, tiles * sizeof(uint64_t))) return rc;
    if (int rc = b.d_bin_idflag.reserve(c, tiles * sizeof(uint32_t))) return rc;
    if (int rc = b.d_bin_total.reserve_exact(c, 16 * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_bin_cand_id.reserve(c, cand_cap * sizeof(uint64_t))) return rc;
    RawInParams p;
    RawInResolve r;
    if (int rc = raw_in_resolve_begin(c, cand_cap, p, r)) return rc;
    p.text = a.data; p.nbytes = a.nbytes; p.now_ms = a.now_ms;
    p.msgs = a.msgs; p.line_of = (unsigned long long *) a.frame_of; p.signal_level = a.signal_level; p.msgs_cap = a.msgs ? a.msgs_cap : 0;
    p.line_class = a.frame_class; p.line_class_cap = a.frame_class ? a.frames_cap : 0; p.line_base = frame_base;
    p.cand_id = b.d_bin_cand_id.as<unsigned long long>(); p.receiver_id = (unsigned long long *) a.receiver_id;
    BeastInParams q;
    q.data = a.data; q.nbytes = a.nbytes; q.net_ingest = a.net_ingest ? 1u : 0u; q.cfg = p.cfg; q.receiver_id_in = a.receiver_id_in;
    q.cand_id = b.d_bin_cand_id.as<unsigned long long>();
    q.frame_class = a.frame_class; q.frame_off = (unsigned long long *) a.frame_off; q.frames_cap = (a.frame_class || a.frame_off) ? a.frames_cap : 0; q.off_base = off_base;
    const BeastInScratch w = {b.d_bin_maps.as<uint8_t>(), b.d_bin_gmaps.as<uint8_t>(), b.d_bin_entry.as<uint32_t>(), b.d_bin_marks.as<uint32_t>(), b.d_bin_meta.as<uint16_t>(),
                              b.d_bin_lane_ids.as<unsigned long long>(), b.d_bin_blocks.as<uint32_t>(), b.d_bin_off.as<unsigned long long>(),
                              b.d_bin_tile_id.as<unsigned long long>(), b.d_bin_entry_id.as<unsigned long long>(), b.d_bin_idflag.as<uint32_t>(),
                              b.d_bin_total.as<unsigned long long>()};
    launch_beast_in_front(q, p, w, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[9];
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    unsigned long long misc[16];
    int rc = MGPU_OK;
    if (total[1] > cand_cap) { c->err = "beast decode: more candidates than the stream can hold"; rc = MGPU_E_OVERFLOW; }   // (cannot happen: beast_in_max_msgs)
    // (every handler call's class is stored, by k_beast_in_classify or by the filter passes: nothing to zero)
    if (int rc2 = raw_in_resolve_end(c, p, r, rc ? 0 : total[1], 0, misc, adds)) return rc2;
    if (rc) return rc;
    n->frames = total[0]; n->msgs = misc[10]; n->id = total[8];
    uint64_t garbage = total[2];
    if (total[6] != ~0ull) {
        const uint64_t at = total[6] >> 8, delta = (total[6] >> 3) & 31u;
        n->stop = (total[6] & 7u) == BEAST_IN_STOP_SYNTH ? MGPU_BEAST_STOP_SYNTH : MGPU_BEAST_STOP_UUID;
        n->consumed = at + delta;
    } else {
        n->consumed = total[7];
        if (final && a.nbytes - n->consumed > kBeastInTail) {   // net_io.c:5010-5015
            garbage += a.nbytes - n->consumed;
            n->consumed = a.nbytes;
        }
    }
    n->stop_off = n->consumed;
    n->cn[0] = misc[2] + misc[3] + misc[4] + misc[5] + misc[6];   // remote_received_modes: every Mode S frame that reached the decode
    n->cn[1] = misc[1] + total[5];                              // remote_received_modeac: the records, and the frames dropped with mode_ac off
    for (int k = 2; k < 7; ++k) n->cn[k] = misc[k];
    n->cn[7] = garbage; n->cn[8] = total[4]; n->cn[9] = total[3];
    return MGPU_OK;
}

static int beast_decode_dev(mgpu_ctx *c, const struct mgpu_beast_in_args &a, uint64_t frame_base, uint64_t off_base, bool final, BeastInCounts *n, std::vector<uint32_t> *adds) {
    const int rc = beast_decode_passes(c, a, frame_base, off_base, final, n, adds);
    if (rc != MGPU_OK) {                                        // (as raw_decode_dev: the tables are given up)
        (void) hipStreamSynchronize(c->stream_aux);
        c->behind->d_raw_in_first.release();
        c->behind->d_raw_in_gen.release();
    }
    return rc;
}

static bool beast_in_args_ok(const struct mgpu_beast_in_args *a) {
    if (!a || a->size < sizeof(struct mgpu_beast_in_args) || !a->consumed || !a->nframes || !a->nmsgs || !a->stop || !a->stop_off || !a->receiver_id_out || !a->counters) return false;
    if (a->nbytes >= (1ull << 32) || a->msgs_cap > UINT64_MAX / sizeof(mgpu_msg) || a->frames_cap > UINT64_MAX / sizeof(uint64_t)) return false;
    if (a->now_ms < 0 || a->now_ms >= 253402300800000ll) return false;
    if (a->nbytes && !a->data) return false;
    if ((a->msgs_cap && (!a->msgs || !a->receiver_id)) || (a->frames_cap && !a->frame_class && !a->frame_off)) return false;
    return true;
}

static void beast_in_report(const struct mgpu_beast_in_args *a, const BeastInCounts &n) {
    *a->consumed = n.consumed; *a->nframes = n.frames; *a->nmsgs = n.msgs; *a->stop = n.stop; *a->stop_off = n.stop_off; *a->receiver_id_out = n.id;
    beast_in_counters_of(n, a->counters);
}

static int beast_in_finish(mgpu_ctx *c, const struct mgpu_beast_in_args *a, const BeastInCounts &n, const IcaoFilter::Snapshot &before, const std::vector<uint32_t> &adds) {
    const bool want_frames = a->frame_class || a->frame_off;
    if (n.msgs > a->msgs_cap || (want_frames && n.frames > a->frames_cap)) {
        c->resolver.filter().restore(before);
        c->err = n.msgs > a->msgs_cap ? "beast decode: more messages than the arrays hold" : "beast decode: more handler calls than the frame arrays hold";
        return MGPU_E_OVERFLOW;
    }
    return raw_in_publish_adds(c, adds);                        // the pre-screen learns the new addresses, as after mgpu_raw_decode
}

int mgpu_beast_decode_device(mgpu_ctx *c, const struct mgpu_beast_in_args *a) {
    if (!c || !beast_in_args_ok(a)) return MGPU_E_INVAL;
    if (((uintptr_t) a->msgs | (uintptr_t) a->receiver_id | (uintptr_t) a->frame_of | (uintptr_t) a->signal_level | (uintptr_t) a->frame_off) & 7u) return MGPU_E_INVAL;
    BeastInCounts n;
    n.id = a->receiver_id_in;
    beast_in_report(a, n);
    if (a->nbytes == 0) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    IcaoFilter::Snapshot before;
    c->resolver.filter().snapshot(before);
    std::vector<uint32_t> adds;
    if (int rc = beast_decode_dev(c, *a, 0, 0, true, &n, &adds)) { c->resolver.filter().restore(before); return rc; }
    beast_in_report(a, n);
    return beast_in_finish(c, a, n, before, adds);
}

int mgpu_beast_decode(mgpu_ctx *c, const struct mgpu_beast_in_args *a) {
    if (!c || !beast_in_args_ok(a)) return MGPU_E_INVAL;
    BeastInCounts all;
    all.id = a->receiver_id_in;
    beast_in_report(a, all);
    if (a->nbytes == 0) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    IcaoFilter::Snapshot before;
    c->resolver.filter().snapshot(before);
    std::vector<uint32_t> adds;
    const bool want_frames = a->frame_class || a->frame_off;
    size_t adds_before = 0;
    IcaoFilter::Snapshot pass_before;
    const int prc = beast_in_passes(a->nbytes, a->pass_bytes ? a->pass_bytes : kUatDefaultPass, all,
        [&](uint64_t at, uint64_t nb, bool final, const BeastInCounts &so_far, BeastInCounts &n) -> int {
            // what this pass may write: what the caller's arrays still hold, and no more than nb bytes can give
            const uint64_t msg_room = a->msgs_cap > so_far.msgs ? std::min<uint64_t>(a->msgs_cap - so_far.msgs, beast_in_max_msgs(nb)) : 0;
            const uint64_t frame_room = want_frames && a->frames_cap > so_far.frames ? std::min<uint64_t>(a->frames_cap - so_far.frames, beast_in_max_frames(nb)) : 0;
            int rc;
            if ((rc = b.d_bin_data.reserve(c, nb + 64)) || (rc = b.d_bin_msgs.reserve(c, (msg_room + 1) * sizeof(mgpu_msg))) ||
                (rc = b.d_bin_ids.reserve(c, (msg_room + 1) * sizeof(uint64_t))) || (rc = b.d_bin_frame_of.reserve(c, (msg_room + 1) * sizeof(uint64_t))) ||
                (rc = b.d_bin_sig.reserve(c, (msg_room + 1) * sizeof(double))) || (rc = b.d_bin_cls.reserve(c, frame_room + 1)) ||
                (rc = b.d_bin_frame_off.reserve(c, (frame_room + 1) * sizeof(uint64_t)))) return rc;
            struct mgpu_beast_in_args d = *a;
            d.data = b.d_bin_data.as<uint8_t>(); d.nbytes = nb; d.receiver_id_in = so_far.id;
            d.msgs = b.d_bin_msgs.as<mgpu_msg>(); d.receiver_id = b.d_bin_ids.as<uint64_t>(); d.msgs_cap = msg_room;
            d.frame_of = a->frame_of ? b.d_bin_frame_of.as<uint64_t>() : nullptr;
            d.signal_level = a->signal_level ? b.d_bin_sig.as<double>() : nullptr;
            d.frame_class = a->frame_class ? b.d_bin_cls.as<uint8_t>() : nullptr;
            d.frame_off = a->frame_off ? b.d_bin_frame_off.as<uint64_t>() : nullptr;
            d.frames_cap = frame_room;
            HIPCHK(c, hipMemcpyAsync(b.d_bin_data.p, a->data + at, nb, hipMemcpyHostToDevice, c->stream_aux));
            adds_before = adds.size();
            c->resolver.filter().snapshot(pass_before);
            if ((rc = beast_decode_dev(c, d, so_far.frames, at, final, &n, &adds))) return rc;
            // (the pass stored below its rooms only: the copies stay inside the caller's arrays)
            const uint64_t nmsg = std::min<uint64_t>(n.msgs, msg_room), nfr = std::min<uint64_t>(n.frames, frame_room);
            if (nmsg) HIPCHK(c, hipMemcpy(a->msgs + so_far.msgs, d.msgs, nmsg * sizeof(mgpu_msg), hipMemcpyDeviceToHost));
            if (nmsg) HIPCHK(c, hipMemcpy(a->receiver_id + so_far.msgs, d.receiver_id, nmsg * sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (nmsg && a->frame_of) HIPCHK(c, hipMemcpy(a->frame_of + so_far.msgs, d.frame_of, nmsg * sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (nmsg && a->signal_level) HIPCHK(c, hipMemcpy(a->signal_level + so_far.msgs, d.signal_level, nmsg * sizeof(double), hipMemcpyDeviceToHost));
            if (nfr && a->frame_class) HIPCHK(c, hipMemcpy(a->frame_class + so_far.frames, d.frame_class, nfr, hipMemcpyDeviceToHost));
            if (nfr && a->frame_off) HIPCHK(c, hipMemcpy(a->frame_off + so_far.frames, d.frame_off, nfr * sizeof(uint64_t), hipMemcpyDeviceToHost));
            return MGPU_OK;
        },
        [&] { c->resolver.filter().restore(pass_before); adds.resize(adds_before); });
    if (prc != MGPU_OK) { c->resolver.filter().restore(before); return prc; }
    beast_in_report(a, all);
    return beast_in_finish(c, a, all, before, adds);
}

// ---- ASTERIX input: readAsterix + decodeAsterixMessage over a length-chained stream (asterix_in_format.h, kernels/asterix_in.inc) ----

struct AstInCounts { uint64_t frames, recs, other, undefined, consumed; uint32_t stop; };

// a: data, recs and frame_of device pointers; `look` bytes behind a.nbytes are the stream's too.  The counts of this stretch.
// Overflows are the caller's to judge.
static int asterix_decode_dev(mgpu_ctx *c, const struct mgpu_asterix_in_args &a, uint64_t look, uint64_t frame_base, AstInCounts *n) {
    Behind &b = *c->behind;
    const size_t tiles = ast_in_tiles(a.nbytes), groups = ast_in_groups(a.nbytes);
    if (int rc = b.d_ast_in_maps.reserve(c, (uint64_t) tiles * kAstTile * sizeof(uint16_t))) return rc;
    if (int rc = b.d_ast_in_gmaps.reserve(c, (uint64_t) groups * kAstTile * sizeof(uint16_t))) return rc;
    if (int rc = b.d_ast_in_entry.reserve(c, (tiles + groups) * sizeof(uint32_t))) return rc;
    if (int rc = b.d_ast_in_bits.reserve(c, 3 * (uint64_t) tiles * kAstWords * sizeof(uint32_t))) return rc;
    if (int rc = b.d_ast_in_blocks.reserve(c, 4 * tiles * sizeof(uint32_t))) return rc;
    if (int rc = b.d_ast_in_off.reserve(c, 2 * tiles * sizeof(unsigned long long))) return rc;
    if (int rc = b.d_ast_in_total.reserve_exact(c, 16 * sizeof(unsigned long long))) return rc;
    const AstInScratch w = {b.d_ast_in_maps.as<uint16_t>(), b.d_ast_in_gmaps.as<uint16_t>(), b.d_ast_in_entry.as<uint32_t>(), b.d_ast_in_bits.as<uint32_t>(),
                            b.d_ast_in_blocks.as<uint32_t>(), b.d_ast_in_off.as<unsigned long long>(), b.d_ast_in_total.as<unsigned long long>(), tiles};
    const AstInParams p = {a.data, a.nbytes, look, a.recs, (unsigned long long *) a.frame_of, a.recs ? a.recs_cap : 0, frame_base, a.now_ms, a.source};
    launch_asterix_decode(p, w, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[6] = {0, 0, 0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    *n = {total[0], total[1], total[2], total[3], total[4], (uint32_t) total[5]};
    return MGPU_OK;
}

static bool asterix_in_args_ok(const struct mgpu_asterix_in_args *a) {
    if (!a || a->size < sizeof(struct mgpu_asterix_in_args) || !a->consumed || !a->nframes || !a->nrecs || !a->stop) return false;
    if (!ast_in_source_ok(a->source) || !ast_in_now_ok(a->now_ms) || a->nbytes > kAstMaxBytes || a->recs_cap > UINT64_MAX / sizeof(mgpu_asterix_rec)) return false;
    if (a->nbytes && !a->data) return false;
    if (a->recs_cap && !a->recs) return false;
    return true;
}

static void asterix_in_report(const struct mgpu_asterix_in_args *a, const AstInCounts &n) {
    *a->consumed = n.consumed;
    *a->nframes = n.frames;
    *a->nrecs = n.recs;
    *a->stop = n.stop;
    if (a->nother) *a->nother = n.other;
    if (a->nundefined) *a->nundefined = n.undefined;
}

static int asterix_in_verdict(mgpu_ctx *c, const struct mgpu_asterix_in_args *a, const AstInCounts &n) {
    if (n.recs > a->recs_cap) { c->err = "asterix decode: more records than the array holds"; return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

int mgpu_asterix_decode_device(mgpu_ctx *c, const struct mgpu_asterix_in_args *a) {
    if (!c || !asterix_in_args_ok(a)) return MGPU_E_INVAL;
    if (((uintptr_t) a->recs & 15u) || ((uintptr_t) a->frame_of & 7u)) return MGPU_E_INVAL;
    AstInCounts n = {0, 0, 0, 0, 0, MGPU_AST_STOP_END};
    asterix_in_report(a, n);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = asterix_decode_dev(c, *a, 0, 0, &n)) return rc;
    asterix_in_report(a, n);
    return asterix_in_verdict(c, a, n);
}

constexpr uint64_t kAstInDefaultPass = 16ull << 20;          // bytes the host form stages per pass, pass_bytes == 0

int mgpu_asterix_decode(mgpu_ctx *c, const struct mgpu_asterix_in_args *a) {
    if (!c || !asterix_in_args_ok(a)) return MGPU_E_INVAL;
    AstInCounts all = {0, 0, 0, 0, 0, MGPU_AST_STOP_END};
    asterix_in_report(a, all);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    uint64_t pass = std::min<uint64_t>(a->pass_bytes ? a->pass_bytes : kAstInDefaultPass, a->nbytes);
    for (uint64_t at = 0;;) {
        // a pass frames nb bytes; its items may read kAstInLook more, which decide every frame that starts inside the pass
        const uint64_t nb = std::min<uint64_t>(pass, a->nbytes - at), look = std::min<uint64_t>(kAstInLook, a->nbytes - at - nb);
        const uint64_t rec_room = a->recs_cap > all.recs ? std::min<uint64_t>(a->recs_cap - all.recs, ast_in_max_recs(nb)) : 0;
        if (int rc = b.d_ast_in_data.reserve(c, nb + look + 64)) return rc;
        if (int rc = b.d_ast_in_recs.reserve(c, (rec_room + 1) * sizeof(mgpu_asterix_rec))) return rc;
        struct mgpu_asterix_in_args d = *a;
        d.data = b.d_ast_in_data.as<uint8_t>(); d.nbytes = nb;
        d.recs = b.d_ast_in_recs.as<mgpu_asterix_rec>(); d.recs_cap = rec_room;
        d.frame_of = nullptr;
        if (a->frame_of) { if (int rc = b.d_ast_in_frame_of.reserve(c, (rec_room + 1) * sizeof(uint64_t))) return rc; d.frame_of = b.d_ast_in_frame_of.as<uint64_t>(); }
        HIPCHK(c, hipMemcpyAsync(b.d_ast_in_data.p, a->data + at, nb + look, hipMemcpyHostToDevice, c->stream_aux));
        AstInCounts n;
        if (int rc = asterix_decode_dev(c, d, look, all.frames, &n)) return rc;
        const bool last = at + nb == a->nbytes;
        if (n.consumed == 0 && n.stop == MGPU_AST_STOP_END && !last) {   // a record longer than the pass: a larger pass
            pass = pass > a->nbytes / 2 ? a->nbytes : 2 * pass;
            continue;
        }
        // (the pass stored the records below its room only: the copies stay inside the caller's arrays)
        const uint64_t nrec = std::min<uint64_t>(n.recs, rec_room);
        if (nrec) HIPCHK(c, hipMemcpy(a->recs + all.recs, d.recs, nrec * sizeof(mgpu_asterix_rec), hipMemcpyDeviceToHost));
        if (nrec && a->frame_of) HIPCHK(c, hipMemcpy(a->frame_of + all.recs, d.frame_of, nrec * sizeof(uint64_t), hipMemcpyDeviceToHost));
        all.frames += n.frames; all.recs += n.recs; all.other += n.other; all.undefined += n.undefined;
        at += n.consumed;
        all.consumed = at;
        all.stop = n.stop;
        if (n.stop != MGPU_AST_STOP_END || last) break;             // the unconsumed tail is the next pass's head
    }
    asterix_in_report(a, all);
    return asterix_in_verdict(c, a, all);
}

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
