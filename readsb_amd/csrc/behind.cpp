// behind.cpp — behind the message list: beast encoder, field decode, tracking gate, position decode, and the CRC / table diagnostics.
#include "ctx.h"

#include <cmath>

extern "C" {

// ---- beast wire format (net_io.c:1655-1714) for message records that already are in HBM -----------------------

// What follows the message list — field decode, beast encoder, tracking gate — runs on a stream of its own (stream_aux): these calls
// are synchronous, and on the pipeline's main stream they waited for every chunk a deferred feed had queued there.
static int beast_reserve(mgpu_ctx *c, uint64_t n) {
    if (n > c->beast_cap_msgs) {
        if (c->d_beast_len) (void) hipFree(c->d_beast_len);
        if (c->d_beast_blocks) (void) hipFree(c->d_beast_blocks);
        if (c->d_beast_off) (void) hipFree(c->d_beast_off);
        c->d_beast_len = nullptr; c->d_beast_blocks = nullptr; c->d_beast_off = nullptr; c->beast_cap_msgs = 0;
        const uint64_t want = n + n / 4 + 1024;
        HIPCHK(c, hipMalloc(&c->d_beast_len, want * sizeof(uint16_t)));
        HIPCHK(c, hipMalloc(&c->d_beast_blocks, 2 * (want / kBlock + 2) * sizeof(uint32_t)));              // frame bytes | deferred messages per workgroup
        HIPCHK(c, hipMalloc(&c->d_beast_off, 2 * (want / kBlock + 2) * sizeof(unsigned long long)));
        c->beast_cap_msgs = want;
    }
    if (!c->d_beast_total) HIPCHK(c, hipMalloc(&c->d_beast_total, 4 * sizeof(unsigned long long)));   // bytes, deferred, last id
    return MGPU_OK;
}

// grow-on-demand device scratch of the context
static int reserve_bytes(mgpu_ctx *c, void **p, uint64_t *cap, uint64_t want) {
    if (want <= *cap) return MGPU_OK;
    if (*p) (void) hipFree(*p);
    *p = nullptr; *cap = 0;
    want += want / 4 + 1024;
    HIPCHK(c, hipMalloc(p, want));
    *cap = want;
    return MGPU_OK;
}

// d_verdict == nullptr: every message's frame.  Everything in device memory; *ndeferred (may be null without a verdict).
// d_ids / *last_id (host, may be null): the receiver-id prefixes; MGPU_BEAST_VERBATIM in flags (include/modes_gpu.h)
static int beast_encode_dev(mgpu_ctx *c, const mgpu_msg *d_msgs, const uint8_t *d_verdict, uint64_t n, uint32_t flags, uint8_t *d_out, uint64_t cap,
                            uint64_t *bytes, mgpu_deferred *d_deferred, uint64_t deferred_cap, uint64_t *ndeferred, const uint64_t *d_ids = nullptr,
                            uint64_t *last_id = nullptr) {
    if (int rc = beast_reserve(c, n)) return rc;
    if (d_ids)
        if (int rc = reserve_bytes(c, &c->d_beast_idw, &c->beast_cap_idw, beast_id_scratch_bytes(n))) return rc;
    const bool verbatim = (flags & MGPU_BEAST_VERBATIM) != 0, gated = d_verdict && !verbatim;
    const size_t nb = (size_t) (c->beast_cap_msgs / kBlock + 2);
    launch_beast_encode(d_msgs, n, c->d_beast_len, c->d_beast_blocks, c->d_beast_off, d_out, cap, c->d_beast_total, c->stream_aux, d_verdict,
                        (flags & MGPU_BEAST_NET_RULE) ? 1 : 0, c->d_beast_blocks + nb, c->d_beast_off + nb, d_deferred, deferred_cap, verbatim ? 1 : 0,
                        (const unsigned long long *) d_ids, last_id ? *last_id : 0ull, c->d_beast_idw);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(total, c->d_beast_total, (d_ids ? 3 : gated ? 2 : 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    *bytes = total[0];
    if (ndeferred) *ndeferred = gated ? total[1] : 0;
    if (d_ids && last_id) *last_id = total[2];
    if (total[0] > cap) { c->err = "mgpu_beast_encode: output buffer too small"; return MGPU_E_OVERFLOW; }
    if (gated && total[1] > deferred_cap) { c->err = "mgpu_beast_encode_gated: more deferred messages than the list holds"; return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

int mgpu_beast_encode_device(mgpu_ctx *c, const struct mgpu_msg *d_msgs, uint64_t n, uint8_t *d_out, uint64_t cap, uint64_t *bytes) {
    if (!c || !bytes || (n && (!d_msgs || !d_out))) return MGPU_E_INVAL;
    *bytes = 0;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return beast_encode_dev(c, d_msgs, nullptr, n, 0, d_out, cap, bytes, nullptr, 0, nullptr);
}

int mgpu_beast_encode_gated_device(mgpu_ctx *c, const struct mgpu_msg *d_msgs, const uint8_t *d_verdict, uint64_t n, uint32_t flags, uint8_t *d_out,
                                   uint64_t cap, uint64_t *bytes, struct mgpu_deferred *d_deferred, uint64_t deferred_cap, uint64_t *ndeferred) {
    if (!c || !bytes || !ndeferred || (n && (!d_msgs || !d_verdict || !d_out)) || (deferred_cap && !d_deferred)) return MGPU_E_INVAL;
    *bytes = 0; *ndeferred = 0;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return beast_encode_dev(c, d_msgs, d_verdict, n, flags, d_out, cap, bytes, d_deferred, deferred_cap, ndeferred);
}

static int stage_messages(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n) {          // host list -> d_beast_in
    if (n * sizeof(mgpu_msg) > c->beast_cap_in) {
        if (c->d_beast_in) (void) hipFree(c->d_beast_in);
        c->d_beast_in = nullptr; c->beast_cap_in = 0;
        const uint64_t want = (n + n / 4 + 1024) * sizeof(mgpu_msg);
        HIPCHK(c, hipMalloc(&c->d_beast_in, want));
        c->beast_cap_in = want;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_beast_in, msgs, n * sizeof(mgpu_msg), hipMemcpyHostToDevice, c->stream_aux));
    return MGPU_OK;
}

static int reserve_beast_out(mgpu_ctx *c, uint64_t cap) {
    if (cap > c->beast_cap_out) {
        if (c->d_beast_out) (void) hipFree(c->d_beast_out);
        c->d_beast_out = nullptr; c->beast_cap_out = 0;
        HIPCHK(c, hipMalloc(&c->d_beast_out, cap + 64));
        c->beast_cap_out = cap;
    }
    return MGPU_OK;
}

int mgpu_beast_encode(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *bytes) {
    if (!c || !bytes || (n && (!msgs || !out))) return MGPU_E_INVAL;
    *bytes = 0;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = stage_messages(c, msgs, n)) return rc;
    if (int rc = reserve_beast_out(c, cap)) return rc;
    const int rc = beast_encode_dev(c, (const mgpu_msg *) c->d_beast_in, nullptr, n, 0, c->d_beast_out, cap, bytes, nullptr, 0, nullptr);
    if (rc != MGPU_OK) return rc;
    HIPCHK(c, hipMemcpy(out, c->d_beast_out, *bytes, hipMemcpyDeviceToHost));
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
    if (int rc = stage_messages(c, a->msgs, n)) return rc;
    if (int rc = reserve_beast_out(c, a->cap)) return rc;
    const bool gated = a->verdict && !(a->flags & MGPU_BEAST_VERBATIM);
    if (gated) {
        if (int rc = reserve_bytes(c, &c->d_beast_verdict, &c->beast_cap_verdict, n)) return rc;
        HIPCHK(c, hipMemcpyAsync(c->d_beast_verdict, a->verdict, n, hipMemcpyHostToDevice, c->stream_aux));
        if (a->deferred_cap + 64 > c->deferred_cap) {
            if (c->d_deferred) (void) hipFree(c->d_deferred);
            c->d_deferred = nullptr; c->deferred_cap = 0;
            HIPCHK(c, hipMalloc(&c->d_deferred, (a->deferred_cap + 64) * sizeof(mgpu_deferred)));
            c->deferred_cap = a->deferred_cap + 64;
        }
    }
    if (a->ids) {
        if (int rc = reserve_bytes(c, &c->d_beast_ids, &c->beast_cap_ids, n * sizeof(uint64_t))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->d_beast_ids, a->ids, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream_aux));
    }
    const int rc = beast_encode_dev(c, (const mgpu_msg *) c->d_beast_in, gated ? (const uint8_t *) c->d_beast_verdict : nullptr, n, a->flags, c->d_beast_out, a->cap,
                                    a->bytes, c->d_deferred, a->deferred_cap, a->ndeferred, a->ids ? (const uint64_t *) c->d_beast_ids : nullptr, a->last_id);
    if (rc != MGPU_OK) return rc;
    HIPCHK(c, hipMemcpy(a->out, c->d_beast_out, *a->bytes, hipMemcpyDeviceToHost));
    if (gated && *a->ndeferred) HIPCHK(c, hipMemcpy(a->deferred, c->d_deferred, *a->ndeferred * sizeof(mgpu_deferred), hipMemcpyDeviceToHost));
    return MGPU_OK;
}

// ---- the aggregator's time merge (kernels/merge.inc) ----

static int merge_dev(mgpu_ctx *c, const struct mgpu_msg *const *d_segments, const uint64_t *counts, uint32_t nseg, const uint64_t *segment_ids,
                     const uint8_t *const *d_verdict_in, struct mgpu_msg *d_out, uint64_t *d_perm, uint64_t *d_ids, uint8_t *d_verdict_out, uint64_t n) {
    std::vector<MergeSeg> segs(nseg);
    uint64_t start = 0;
    for (uint32_t k = 0; k < nseg; ++k) {
        segs[k].msgs = d_segments[k];
        segs[k].verdict = d_verdict_in ? d_verdict_in[k] : nullptr;
        segs[k].start = start;
        segs[k].id = segment_ids ? segment_ids[k] : 0;
        start += counts[k];
    }
    if (int rc = reserve_bytes(c, &c->d_merge_scratch, &c->merge_cap_scratch, merge_scratch_bytes(n, nseg))) return rc;
    const unsigned long long *d_diff = launch_merge_keys(segs.data(), nseg, n, c->d_merge_scratch, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long diff = 0;
    HIPCHK(c, hipMemcpyAsync(&diff, d_diff, sizeof diff, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));            // (the segment table has left `segs` by now, too)
    c->merge_passes = launch_merge_sort(nseg, n, diff, c->d_merge_scratch, d_out, d_perm, d_ids, d_verdict_out, c->stream_aux);
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
    c->merge_passes = 0;
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
    c->merge_passes = 0;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // staged: the concatenation in d_beast_in, its verdicts in d_beast_verdict; results: records | permutation | ids | verdicts in d_merge_out
    if (n * sizeof(mgpu_msg) > c->beast_cap_in) {
        if (c->d_beast_in) (void) hipFree(c->d_beast_in);
        c->d_beast_in = nullptr; c->beast_cap_in = 0;
        const uint64_t want = (n + n / 4 + 1024) * sizeof(mgpu_msg);
        HIPCHK(c, hipMalloc(&c->d_beast_in, want));
        c->beast_cap_in = want;
    }
    if (verdict_in)
        if (int rc = reserve_bytes(c, &c->d_beast_verdict, &c->beast_cap_verdict, n)) return rc;
    if (int rc = reserve_bytes(c, &c->d_merge_out, &c->merge_cap_out, n * (sizeof(mgpu_msg) + 8 + 8 + 1))) return rc;
    std::vector<const mgpu_msg *> d_seg(nseg);
    std::vector<const uint8_t *> d_ver(nseg);
    uint64_t at = 0;
    for (uint32_t k = 0; k < nseg; ++k) {
        d_seg[k] = (const mgpu_msg *) c->d_beast_in + at;
        d_ver[k] = nullptr;
        if (counts[k]) {
            HIPCHK(c, hipMemcpyAsync(c->d_beast_in + at * sizeof(mgpu_msg), segments[k], counts[k] * sizeof(mgpu_msg), hipMemcpyHostToDevice, c->stream_aux));
            if (verdict_in && verdict_in[k]) {
                d_ver[k] = (const uint8_t *) c->d_beast_verdict + at;
                HIPCHK(c, hipMemcpyAsync((uint8_t *) c->d_beast_verdict + at, verdict_in[k], counts[k], hipMemcpyHostToDevice, c->stream_aux));
            }
        }
        at += counts[k];
    }
    mgpu_msg *d_out = (mgpu_msg *) c->d_merge_out;
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

int mgpu_merge_last_passes(mgpu_ctx *c) { return c ? c->merge_passes : MGPU_E_INVAL; }

// ---- per-message field decode (mode_s.c:598-760, 806-1555; mode_ac.c:171-200) --------------------------------------

static int fields_tables(mgpu_ctx *c) {
    if (c->d_roll_tan) return MGPU_OK;
    const std::vector<double> t = build_roll_tangent_table();
    HIPCHK(c, hipMalloc(&c->d_roll_tan, t.size() * sizeof(double)));
    HIPCHK(c, hipMemcpy(c->d_roll_tan, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    return MGPU_OK;
}

int mgpu_decode_fields_device(mgpu_ctx *c, const struct mgpu_msg *d_msgs, uint64_t n, struct mgpu_fields *d_out) {
    if (!c || (n && (!d_msgs || !d_out))) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = fields_tables(c)) return rc;
    launch_decode_fields(d_msgs, n, d_out, c->d_roll_tan, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

static int fields_reserve(mgpu_ctx *c, uint64_t n) {
    if (n > c->fields_cap) {
        if (c->d_fields) (void) hipFree(c->d_fields);
        c->d_fields = nullptr; c->fields_cap = 0;
        const uint64_t want = n + n / 4 + 1024;
        HIPCHK(c, hipMalloc(&c->d_fields, want * sizeof(mgpu_fields)));
        c->fields_cap = want;
    }
    return fields_tables(c);
}

int mgpu_decode_fields(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n, struct mgpu_fields *out) {
    if (!c || (n && (!msgs || !out))) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = fields_reserve(c, n)) return rc;
    if (int rc = stage_messages(c, msgs, n)) return rc;
    launch_decode_fields((const mgpu_msg *) c->d_beast_in, n, c->d_fields, c->d_roll_tan, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->d_fields, n * sizeof(mgpu_fields), hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

// ---- first stage of the tracker + forwarding rule (track.c:1688-1693, 1905-1966; net_io.c:5846-5849, 5924-5940), kernels/gate.inc ----

static int gate_reserve(mgpu_ctx *c, uint64_t n) {
    if (!c->d_gate_table) {
        HIPCHK(c, hipMalloc(&c->d_gate_table, gate_table_bytes()));
        HIPCHK(c, hipMemsetAsync(c->d_gate_table, 0, gate_table_bytes(), c->stream_aux));
    }
    if (n > c->gate_cap) {
        if (c->d_gate_scratch) (void) hipFree(c->d_gate_scratch);
        if (c->d_gate_verdict) (void) hipFree(c->d_gate_verdict);
        c->d_gate_scratch = nullptr; c->d_gate_verdict = nullptr; c->gate_cap = 0;
        const uint64_t want = n + n / 4 + 1024;
        HIPCHK(c, hipMalloc(&c->d_gate_scratch, gate_scratch_bytes(want)));
        HIPCHK(c, hipMalloc(&c->d_gate_verdict, want));
        c->gate_cap = want;
    }
    return MGPU_OK;
}

int mgpu_track_gate_reset(mgpu_ctx *c) {
    if (!c) return MGPU_E_INVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->d_gate_table) {
        HIPCHK(c, hipMemsetAsync(c->d_gate_table, 0, gate_table_bytes(), c->stream_aux));
        HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    }
    return MGPU_OK;
}

int mgpu_track_gate_device(mgpu_ctx *c, const struct mgpu_msg *d_msgs, const struct mgpu_fields *d_fields, uint64_t n, uint8_t *d_verdict) {
    if (!c || (n && (!d_msgs || !d_fields || !d_verdict)) || n > 0xffffffffull) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = gate_reserve(c, n)) return rc;
    launch_track_gate(d_msgs, d_fields, n, c->cfg.buf_samples, c->d_gate_table, c->d_gate_scratch, d_verdict, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

// host list -> d_beast_in, its field records -> d_fields, its verdicts (continuing the context's aircraft table) -> d_gate_verdict
static int gate_staged(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n) {
    if (int rc = fields_reserve(c, n)) return rc;
    if (int rc = gate_reserve(c, n)) return rc;
    if (int rc = stage_messages(c, msgs, n)) return rc;
    launch_decode_fields((const mgpu_msg *) c->d_beast_in, n, c->d_fields, c->d_roll_tan, c->stream_aux);
    launch_track_gate((const mgpu_msg *) c->d_beast_in, c->d_fields, n, c->cfg.buf_samples, c->d_gate_table, c->d_gate_scratch, c->d_gate_verdict, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    return MGPU_OK;
}

int mgpu_track_gate(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n, uint8_t *verdict) {
    if (!c || (n && (!msgs || !verdict)) || n > 0xffffffffull) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = gate_staged(c, msgs, n)) return rc;
    HIPCHK(c, hipMemcpyAsync(verdict, c->d_gate_verdict, n, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

// The gate's verdict applied to the encoder: the beast stream of what the reference forwards for certain + the list of the
// messages its position tracker has to settle (include/modes_gpu.h).  Host arrays; the aircraft table goes on from call to call.
int mgpu_beast_encode_gated(mgpu_ctx *c, const struct mgpu_msg *msgs, uint64_t n, uint32_t flags, uint8_t *out, uint64_t cap, uint64_t *bytes,
                            struct mgpu_deferred *deferred, uint64_t deferred_cap, uint64_t *ndeferred) {
    if (!c || !bytes || !ndeferred || (n && (!msgs || !out)) || (deferred_cap && !deferred) || n > 0xffffffffull) return MGPU_E_INVAL;
    *bytes = 0; *ndeferred = 0;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = gate_staged(c, msgs, n)) return rc;
    if (int rc = reserve_beast_out(c, cap)) return rc;
    if (deferred_cap > c->deferred_cap) {
        if (c->d_deferred) (void) hipFree(c->d_deferred);
        c->d_deferred = nullptr; c->deferred_cap = 0;
        HIPCHK(c, hipMalloc(&c->d_deferred, (deferred_cap + 64) * sizeof(mgpu_deferred)));
        c->deferred_cap = deferred_cap + 64;
    }
    const int rc = beast_encode_dev(c, (const mgpu_msg *) c->d_beast_in, c->d_gate_verdict, n, flags, c->d_beast_out, cap, bytes, c->d_deferred, deferred_cap, ndeferred);
    if (rc != MGPU_OK) return rc;
    HIPCHK(c, hipMemcpy(out, c->d_beast_out, *bytes, hipMemcpyDeviceToHost));
    if (*ndeferred) HIPCHK(c, hipMemcpy(deferred, c->d_deferred, *ndeferred * sizeof(mgpu_deferred), hipMemcpyDeviceToHost));
    return MGPU_OK;
}

// ---- CPR pairing + position decode (track.c:1249-1282, 1827-1850, 758-799, 862-914; cpr.c:62-374), kernels/cpr.inc ----

static int cpr_reserve(mgpu_ctx *c, uint64_t n) {
    if (!c->d_cpr_table) {
        HIPCHK(c, hipMalloc(&c->d_cpr_table, cpr_table_bytes()));
        HIPCHK(c, hipMemsetAsync(c->d_cpr_table, 0, cpr_table_bytes(), c->stream_aux));
    }
    if (n > c->cpr_cap) {
        if (c->d_cpr_scratch) (void) hipFree(c->d_cpr_scratch);
        if (c->d_cpr_out) (void) hipFree(c->d_cpr_out);
        c->d_cpr_scratch = nullptr; c->d_cpr_out = nullptr; c->cpr_cap = 0;
        const uint64_t want = n + n / 4 + 1024;
        HIPCHK(c, hipMalloc(&c->d_cpr_scratch, cpr_scratch_bytes(want)));
        HIPCHK(c, hipMalloc(&c->d_cpr_out, want * sizeof(mgpu_position)));
        c->cpr_cap = want;
    }
    return MGPU_OK;
}

static bool cpr_config_ok(const struct mgpu_cpr_config *cfg) { return cfg && std::isfinite(cfg->ref_lat) && std::isfinite(cfg->ref_lon); }

int mgpu_cpr_reset(mgpu_ctx *c) {
    if (!c) return MGPU_E_INVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->d_cpr_table) {
        HIPCHK(c, hipMemsetAsync(c->d_cpr_table, 0, cpr_table_bytes(), c->stream_aux));
        HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    }
    return MGPU_OK;
}

int mgpu_cpr_track_device(mgpu_ctx *c, const struct mgpu_cpr_config *cfg, const struct mgpu_msg *d_msgs, const struct mgpu_fields *d_fields, uint64_t n,
                          struct mgpu_position *d_out) {
    if (!c || !cpr_config_ok(cfg) || (n && (!d_msgs || !d_fields || !d_out)) || n >= 0xfffffffeull) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = cpr_reserve(c, n)) return rc;
    launch_cpr_track(d_msgs, d_fields, n, *cfg, c->d_cpr_table, c->d_cpr_scratch, d_out, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

int mgpu_cpr_track(mgpu_ctx *c, const struct mgpu_cpr_config *cfg, const struct mgpu_msg *msgs, uint64_t n, struct mgpu_position *out) {
    if (!c || !cpr_config_ok(cfg) || (n && (!msgs || !out)) || n >= 0xfffffffeull) return MGPU_E_INVAL;
    if (n == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = fields_reserve(c, n)) return rc;
    if (int rc = cpr_reserve(c, n)) return rc;
    if (int rc = stage_messages(c, msgs, n)) return rc;
    launch_decode_fields((const mgpu_msg *) c->d_beast_in, n, c->d_fields, c->d_roll_tan, c->stream_aux);
    launch_cpr_track((const mgpu_msg *) c->d_beast_in, c->d_fields, n, *cfg, c->d_cpr_table, c->d_cpr_scratch, (mgpu_position *) c->d_cpr_out, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->d_cpr_out, n * sizeof(mgpu_position), hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

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
    if (n > c->cpr_cases_cap) {                                  // cases, and their results behind them
        if (c->d_cpr_cases) (void) hipFree(c->d_cpr_cases);
        c->d_cpr_cases = nullptr; c->cpr_cases_cap = 0;
        const uint64_t want = n + n / 4 + 1024;
        HIPCHK(c, hipMalloc(&c->d_cpr_cases, want * (sizeof(mgpu_cpr_case) + sizeof(mgpu_cpr_result))));
        c->cpr_cases_cap = want;
    }
    mgpu_cpr_case *d_cases = (mgpu_cpr_case *) c->d_cpr_cases;
    mgpu_cpr_result *d_out = (mgpu_cpr_result *) (d_cases + c->cpr_cases_cap);
    HIPCHK(c, hipMemcpyAsync(d_cases, cases, n * sizeof(mgpu_cpr_case), hipMemcpyHostToDevice, c->stream_aux));
    launch_cpr_cases(d_cases, n, d_out, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_out, n * sizeof(mgpu_cpr_result), hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
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
