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
    if (!c->d_beast_total) HIPCHK(c, hipMalloc(&c->d_beast_total, 2 * sizeof(unsigned long long)));
    return MGPU_OK;
}

// d_verdict == nullptr: every message's frame.  Everything in device memory; *ndeferred (may be null without a verdict)
static int beast_encode_dev(mgpu_ctx *c, const mgpu_msg *d_msgs, const uint8_t *d_verdict, uint64_t n, uint32_t flags, uint8_t *d_out, uint64_t cap,
                            uint64_t *bytes, mgpu_deferred *d_deferred, uint64_t deferred_cap, uint64_t *ndeferred) {
    if (int rc = beast_reserve(c, n)) return rc;
    const size_t nb = (size_t) (c->beast_cap_msgs / kBlock + 2);
    launch_beast_encode(d_msgs, n, c->d_beast_len, c->d_beast_blocks, c->d_beast_off, d_out, cap, c->d_beast_total, c->stream_aux, d_verdict,
                        (flags & MGPU_BEAST_NET_RULE) ? 1 : 0, c->d_beast_blocks + nb, c->d_beast_off + nb, d_deferred, deferred_cap);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(total, c->d_beast_total, (d_verdict ? 2 : 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    *bytes = total[0];
    if (ndeferred) *ndeferred = total[1];
    if (total[0] > cap) { c->err = "mgpu_beast_encode: output buffer too small"; return MGPU_E_OVERFLOW; }
    if (d_verdict && total[1] > deferred_cap) { c->err = "mgpu_beast_encode_gated: more deferred messages than the list holds"; return MGPU_E_OVERFLOW; }
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
