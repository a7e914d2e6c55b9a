// snip.cpp — `readsb --snip <level>` (snipMode, readsb.c:1187-1206) on UC8 samples: mgpu_snip (host arrays, in passes through the
// context's scratch) and mgpu_snip_device (everything in HBM), both over one enqueue core.
#include "snip.h"

#include <algorithm>

constexpr uint64_t kSnipDefaultPass = 32ull << 20;           // samples the host form stages per pass (64 MiB), pass_samples == 0
constexpr uint64_t kSnipMaxSamples = kSnipGroupSamples * 0x7fffffffull;  // a grid's limit

// d_iq (16-byte aligned), d_out: device pointers.  c_in: the reference's counter before these n samples.  *kept: what the call keeps
// (more than cap: nothing at or beyond d_out + 2 * cap was stored); *c_out: the counter behind them.  write == false: those two only.
static int snip_dev(mgpu_ctx *c, const uint8_t *d_iq, uint64_t n, int32_t level, uint64_t c_in, uint8_t *d_out, uint64_t cap, bool write, uint64_t *kept,
                    uint64_t *c_out) {
    Snip &s = *c->snip;
    const size_t nb = (size_t) ((n + kSnipGroupSamples - 1) / kSnipGroupSamples);
    if (int rc = s.d_masks.reserve(c, nb * (kSnipGroupSamples / 64) * sizeof(unsigned long long))) return rc;
    if (int rc = s.d_blocks.reserve(c, 2 * nb * sizeof(uint32_t))) return rc;
    if (int rc = s.d_off.reserve(c, nb * sizeof(unsigned long long))) return rc;
    if (int rc = s.d_total.reserve_exact(c, 2 * sizeof(unsigned long long))) return rc;
    const SnipScratch w = {s.d_masks.as<unsigned long long>(), s.d_blocks.as<uint32_t>(), s.d_off.as<unsigned long long>(), s.d_total.as<unsigned long long>(), nb};
    launch_snip(d_iq, n, level, c_in, w, d_out, cap, write, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    *kept = total[0];
    *c_out = total[1] ? n - total[1] : c_in + n;              // trailing quiet samples; a call without a loud one extends the run (uint64, as the reference's c)
    return MGPU_OK;
}

static bool snip_args_ok(const struct mgpu_snip_args *a) {
    if (!a || a->size < sizeof(struct mgpu_snip_args) || !a->nout) return false;
    if (a->nsamples > kSnipMaxSamples || a->cap_samples > UINT64_MAX / 2) return false;
    if (a->nsamples && (!a->iq || (a->cap_samples && !a->out))) return false;
    if (a->nsamples && a->cap_samples) {                      // out must not overlap iq
        const uintptr_t i0 = (uintptr_t) a->iq, i1 = i0 + 2 * a->nsamples, o0 = (uintptr_t) a->out, o1 = o0 + 2 * a->cap_samples;
        if (i0 < o1 && o0 < i1) return false;
    }
    return true;
}

extern "C" {

int mgpu_snip_device(mgpu_ctx *c, const struct mgpu_snip_args *a) {
    if (!c || !snip_args_ok(a)) return MGPU_E_INVAL;
    if (a->nsamples && (((uintptr_t) a->iq & 15u) || ((uintptr_t) a->out & 1u))) return MGPU_E_INVAL;
    *a->nout = 0;
    if (a->nsamples == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    uint64_t kept = 0, run = 0;
    if (int rc = snip_dev(c, a->iq, a->nsamples, a->level, a->quiet_run ? *a->quiet_run : 0, a->out, a->cap_samples, true, &kept, &run)) return rc;
    *a->nout = kept;
    if (kept > a->cap_samples) { c->err = "mgpu_snip_device: output buffer too small"; return MGPU_E_OVERFLOW; }
    if (a->quiet_run) *a->quiet_run = run;
    return MGPU_OK;
}

int mgpu_snip(mgpu_ctx *c, const struct mgpu_snip_args *a) {
    if (!c || !snip_args_ok(a)) return MGPU_E_INVAL;
    *a->nout = 0;
    if (a->nsamples == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Snip &s = *c->snip;
    const uint64_t pass = std::min(a->pass_samples ? a->pass_samples : kSnipDefaultPass, a->nsamples);
    if (int rc = s.d_in.reserve_exact(c, 2 * pass)) return rc;
    if (int rc = s.d_out.reserve_exact(c, 2 * pass)) return rc;
    uint64_t run = a->quiet_run ? *a->quiet_run : 0, produced = 0;
    bool fits = true;                                         // once it does not, the remaining passes only count: *nout = what is needed
    for (uint64_t at = 0; at < a->nsamples; at += pass) {
        const uint64_t n = std::min(pass, a->nsamples - at);
        HIPCHK(c, hipMemcpyAsync(s.d_in.p, a->iq + 2 * at, 2 * n, hipMemcpyHostToDevice, c->stream_aux));
        uint64_t kept = 0;
        if (int rc = snip_dev(c, s.d_in.as<uint8_t>(), n, a->level, run, s.d_out.as<uint8_t>(), n, fits, &kept, &run)) return rc;
        fits = fits && kept <= a->cap_samples - produced;     // (produced <= cap_samples as long as it fits)
        if (fits && kept) HIPCHK(c, hipMemcpy(a->out + 2 * produced, s.d_out.p, 2 * kept, hipMemcpyDeviceToHost));
        produced += kept;
    }
    *a->nout = produced;
    if (!fits) { c->err = "mgpu_snip: output buffer too small"; return MGPU_E_OVERFLOW; }
    if (a->quiet_run) *a->quiet_run = run;
    return MGPU_OK;
}

}  // extern "C"
