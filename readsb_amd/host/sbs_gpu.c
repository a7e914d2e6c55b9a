/* sbs_gpu.c — the BaseStation feed of a sample file with everything resident (readsb_gpu_ifile --sbs-out): what outputMessage's
 * SBS branch (net_io.c:5846-5857, modesSendSBSOutput :3184-3404) writes for the capture, with deferred messages dropped.
 * With opts.asterix (--asterix-out) the same chain ends in mgpu_asterix_encode_ex_device: the ASTERIX CAT021 stream of the capture
 * (:5882, modesSendAsterixOutput :2416-2945), no receiver ids and fresh aircraft state. */
#define __HIP_PLATFORM_AMD__ 1
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <hip/hip_runtime_api.h>

#include "readsb_gpu_host.h"

/* The resident chain.  Every chunk of the file is one deferred feed whose records k_build_messages leaves in HBM
 * (mgpu_set_device_messages); mgpu_collect_device hands their device pointer to the stages behind the list. */
#define SBS_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return MGPU_E_HIP; } } while (0)
#define SBS_MGPU(call) do { int rc_ = (call); if (rc_ != MGPU_OK) { fprintf(stderr, "%s: %s (%s)\n", #call, mgpu_strerror(rc_), mgpu_last_error(ctx)); return rc_; } } while (0)

int gpu_sbs_run(mgpu_ctx *ctx, int fd, input_format_t fmt, unsigned chunk_buffers, const struct gpu_sbs_opts *o, struct mgpu_counters *counters) {
    FILE *out = fopen(o->path, "wb");
    if (!out) { perror(o->path); return MGPU_E_INVAL; }
    const size_t bps = fmt == INPUT_UC8 ? 2 : 4, want = (size_t) chunk_buffers * 131072 * bps;
    uint8_t *buf = malloc(want), *text = NULL;
    if (!buf) return MGPU_E_NOMEM;
    SBS_MGPU(mgpu_set_deferred(ctx, 1));
    SBS_MGPU(mgpu_set_device_messages(ctx, 1));
    struct mgpu_cpr_config cpr = {o->lat, o->lon, (uint32_t) o->have_ref, 0};
    struct mgpu_fields *d_fields = NULL;
    struct mgpu_position *d_pos = NULL;
    struct mgpu_deferred *d_def = NULL;
    uint8_t *d_verdict = NULL, *d_text = NULL;
    uint64_t cap = 0, text_cap = 0, lines_bytes = 0, dropped = 0, skipped = 0, nmsg = 0;
    for (int last = 0; !last;) {
        size_t have = 0;
        while (have < want) {                       /* sdr_ifile.c:221-235 */
            ssize_t r = read(fd, buf + have, want - have);
            if (r <= 0) break;
            have += (size_t) r;
        }
        last = have < want;
        if (have / bps == 0) break;
        SBS_MGPU(mgpu_feed_iq(ctx, buf, have / bps));
        const struct mgpu_msg *d_msgs = NULL;
        uint64_t n = 0;
        SBS_MGPU(mgpu_collect_device(ctx, &d_msgs, &n, NULL));
        if (!n) continue;
        if (n > cap) {                              /* the stages' arrays, grown to the largest feed */
            (void) hipFree(d_fields); (void) hipFree(d_pos); (void) hipFree(d_def); (void) hipFree(d_verdict); (void) hipFree(d_text);
            cap = n + n / 4 + 1024;
            SBS_HIP(hipMalloc((void **) &d_fields, cap * sizeof(*d_fields)));
            SBS_HIP(hipMalloc((void **) &d_pos, cap * sizeof(*d_pos)));
            SBS_HIP(hipMalloc((void **) &d_def, cap * sizeof(*d_def)));
            SBS_HIP(hipMalloc((void **) &d_verdict, cap));
            SBS_HIP(hipMalloc((void **) &d_text, cap * 176));
        }
        SBS_MGPU(mgpu_decode_fields_device(ctx, d_msgs, n, d_fields));
        SBS_MGPU(mgpu_track_gate_device(ctx, d_msgs, d_fields, n, d_verdict));
        SBS_MGPU(mgpu_cpr_track_device(ctx, &cpr, d_msgs, d_fields, n, d_pos));
        uint64_t bytes = 0, nd = 0, ns = 0;
        if (o->asterix) {
            struct mgpu_asterix_args a;
            memset(&a, 0, sizeof a);
            a.size = sizeof a;
            a.msgs = d_msgs; a.fields = d_fields; a.positions = d_pos; a.verdict = d_verdict; a.n = n;
            a.now_ms = o->now_ms;
            a.out = d_text; a.cap = cap * 176; a.bytes = &bytes;                               /* (a record is at most 74 bytes) */
            a.deferred = d_def; a.deferred_cap = cap; a.ndeferred = &nd; a.nskipped = &ns;
            SBS_MGPU(mgpu_asterix_encode_ex_device(ctx, &a));
        } else {
            struct mgpu_sbs_args a;
            memset(&a, 0, sizeof a);
            a.size = sizeof a; a.flags = o->gnss ? MGPU_SBS_USE_GNSS : 0;
            a.msgs = d_msgs; a.fields = d_fields; a.positions = d_pos; a.verdict = d_verdict; a.n = n;
            a.now_ms = o->now_ms; a.override_squawk = -1;
            a.out = d_text; a.cap = cap * 176; a.bytes = &bytes;
            a.deferred = d_def; a.deferred_cap = cap; a.ndeferred = &nd; a.nskipped = &ns;      /* listed, then dropped */
            SBS_MGPU(mgpu_sbs_encode_ex_device(ctx, &a));
        }
        if (bytes > text_cap) {
            free(text);
            text_cap = bytes + bytes / 4;
            if (!(text = malloc(text_cap))) return MGPU_E_NOMEM;
        }
        if (bytes) {
            SBS_HIP(hipMemcpy(text, d_text, bytes, hipMemcpyDeviceToHost));
            if (fwrite(text, 1, bytes, out) != bytes) { perror(o->path); return MGPU_E_INVAL; }
        }
        lines_bytes += bytes; dropped += nd; skipped += ns; nmsg += n;
    }
    SBS_MGPU(mgpu_finish(ctx));
    {
        const struct mgpu_msg *d_msgs = NULL;
        uint64_t n = 0;
        SBS_MGPU(mgpu_collect_device(ctx, &d_msgs, &n, counters));
    }
    (void) hipFree(d_fields); (void) hipFree(d_pos); (void) hipFree(d_def); (void) hipFree(d_verdict); (void) hipFree(d_text);
    free(text); free(buf);
    if (o->asterix)
        fprintf(stderr, "asterix: %" PRIu64 " messages, %" PRIu64 " bytes of records, %" PRIu64 " message(s) left to a position tracker dropped, %" PRIu64
                " outside the domain\n", nmsg, lines_bytes, dropped, skipped);
    else
        fprintf(stderr, "sbs: %" PRIu64 " messages, %" PRIu64 " bytes of lines, %" PRIu64 " message(s) left to a position tracker dropped, %" PRIu64
                " outside the printable domain\n", nmsg, lines_bytes, dropped, skipped);
    return fclose(out) ? MGPU_E_INVAL : MGPU_OK;
}

