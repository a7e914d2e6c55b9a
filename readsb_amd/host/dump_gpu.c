/* dump_gpu.c — the decoded-message dump of a sample file with everything resident (readsb_gpu_ifile --dump-out): what
 * displayModesMessage (mode_s.c:1809-2239) prints to stdout for the capture without --quiet.  The resident chain of sbs_gpu.c with the
 * dump encoder at its end: feed -> field decode -> mgpu_dump_encode_ex_device; the few messages whose RSSI rounding the device leaves
 * to the host's log10 are formatted here by mgpu_dump_format_host and spliced in at their offsets, so the file is complete.
 * No tracker runs: reduce_forward prints 0 and every CPR block has the "decoding: none" form. */
#define __HIP_PLATFORM_AMD__ 1
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <hip/hip_runtime_api.h>

#include "readsb_gpu_host.h"

#define DUMP_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return MGPU_E_HIP; } } while (0)
#define DUMP_MGPU(call) do { int rc_ = (call); if (rc_ != MGPU_OK) { fprintf(stderr, "%s: %s (%s)\n", #call, mgpu_strerror(rc_), mgpu_last_error(ctx)); return rc_; } } while (0)
#define DUMP_DEFERRED 4096      /* entries of the deferred list: about two messages per million land there */

/* what a run holds: released by gpu_dump_run whichever way dump_run leaves */
struct dump_run_state {
    FILE *out;
    uint8_t *buf, *text, *d_text;
    struct mgpu_fields *d_fields;
    struct mgpu_deferred *d_def;
};

static int dump_run(struct dump_run_state *st, mgpu_ctx *ctx, int fd, input_format_t fmt, unsigned chunk_buffers, const struct gpu_dump_opts *o,
                    struct mgpu_counters *counters) {
    const size_t bps = fmt == INPUT_UC8 ? 2 : 4, want = (size_t) chunk_buffers * 131072 * bps;
    if (!(st->buf = malloc(want))) return MGPU_E_NOMEM;
    DUMP_MGPU(mgpu_set_deferred(ctx, 1));
    DUMP_MGPU(mgpu_set_device_messages(ctx, 1));
    struct mgpu_deferred def[DUMP_DEFERRED];
    uint64_t cap = 0, d_text_cap = 0, text_cap = 0, total = 0, spliced = 0, skipped = 0, nmsg = 0;
    DUMP_HIP(hipMalloc((void **) &st->d_def, sizeof def));
    for (int last = 0; !last;) {
        size_t have = 0;
        while (have < want) {                       /* sdr_ifile.c:221-235 */
            ssize_t r = read(fd, st->buf + have, want - have);
            if (r <= 0) break;
            have += (size_t) r;
        }
        last = have < want;
        if (have / bps == 0) break;
        DUMP_MGPU(mgpu_feed_iq(ctx, st->buf, have / bps));
        const struct mgpu_msg *d_msgs = NULL;
        uint64_t n = 0;
        DUMP_MGPU(mgpu_collect_device(ctx, &d_msgs, &n, NULL));
        if (!n) continue;
        if (n > cap) {
            (void) hipFree(st->d_fields);
            st->d_fields = NULL;
            cap = n + n / 4 + 1024;
            DUMP_HIP(hipMalloc((void **) &st->d_fields, cap * sizeof(*st->d_fields)));
        }
        DUMP_MGPU(mgpu_decode_fields_device(ctx, d_msgs, n, st->d_fields));
        uint64_t bytes = 0, nd = 0, ns = 0;
        struct mgpu_dump_args a;
        memset(&a, 0, sizeof a);
        a.size = sizeof a; a.flags = o->flags; a.show_only = o->show_only;
        a.msgs = d_msgs; a.fields = st->d_fields; a.n = n;
        a.out = st->d_text; a.cap = d_text_cap; a.bytes = &bytes;
        a.deferred = st->d_def; a.deferred_cap = DUMP_DEFERRED; a.ndeferred = &nd; a.nskipped = &ns;
        int rc = mgpu_dump_encode_ex_device(ctx, &a);
        if (rc == MGPU_E_OVERFLOW && bytes > d_text_cap) {          /* the stream's size is known now: room for it, and once more */
            (void) hipFree(st->d_text);
            st->d_text = NULL;
            d_text_cap = bytes + bytes / 4 + 4096;
            DUMP_HIP(hipMalloc((void **) &st->d_text, d_text_cap));
            a.out = st->d_text; a.cap = d_text_cap;
            rc = mgpu_dump_encode_ex_device(ctx, &a);
        }
        DUMP_MGPU(rc);
        if (bytes > text_cap) {
            free(st->text);
            st->text = NULL;
            text_cap = bytes + bytes / 4;
            if (!(st->text = malloc(text_cap))) return MGPU_E_NOMEM;
        }
        if (bytes) DUMP_HIP(hipMemcpy(st->text, st->d_text, bytes, hipMemcpyDeviceToHost));
        if (nd) DUMP_HIP(hipMemcpy(def, st->d_def, nd * sizeof def[0], hipMemcpyDeviceToHost));
        uint64_t at = 0;
        for (uint64_t k = 0; k < nd; ++k) {                          /* the stream up to a deferred message's place, then the host's st->text of it */
            struct mgpu_msg m;
            struct mgpu_fields f;
            uint8_t one[MGPU_DUMP_MAX];
            DUMP_HIP(hipMemcpy(&m, d_msgs + def[k].index, sizeof m, hipMemcpyDeviceToHost));
            DUMP_HIP(hipMemcpy(&f, st->d_fields + def[k].index, sizeof f, hipMemcpyDeviceToHost));
            struct mgpu_dump_args h = a;
            h.msgs = &m; h.fields = &f; h.n = 1;
            const int64_t len = mgpu_dump_format_host(&h, 0, one, sizeof one);
            if (len < 0) { fprintf(stderr, "mgpu_dump_format_host: %s\n", mgpu_strerror((int) len)); return (int) len; }
            if (fwrite(st->text + at, 1, def[k].offset - at, st->out) != def[k].offset - at || fwrite(one, 1, (size_t) len, st->out) != (size_t) len) { perror(o->path); return MGPU_E_INVAL; }
            at = def[k].offset;
            total += (uint64_t) len;
        }
        if (fwrite(st->text + at, 1, bytes - at, st->out) != bytes - at) { perror(o->path); return MGPU_E_INVAL; }
        total += bytes; spliced += nd; skipped += ns; nmsg += n;
    }
    DUMP_MGPU(mgpu_finish(ctx));
    {
        const struct mgpu_msg *d_msgs = NULL;
        uint64_t n = 0;
        DUMP_MGPU(mgpu_collect_device(ctx, &d_msgs, &n, counters));
    }
    fprintf(stderr, "dump: %" PRIu64 " messages, %" PRIu64 " bytes, %" PRIu64 " message(s) formatted on the host, %" PRIu64 " outside the printable domain\n",
            nmsg, total, spliced, skipped);
    return MGPU_OK;
}

int gpu_dump_run(mgpu_ctx *ctx, int fd, input_format_t fmt, unsigned chunk_buffers, const struct gpu_dump_opts *o, struct mgpu_counters *counters) {
    struct dump_run_state st;
    memset(&st, 0, sizeof st);
    if (!(st.out = fopen(o->path, "wb"))) { perror(o->path); return MGPU_E_INVAL; }
    int rc = dump_run(&st, ctx, fd, fmt, chunk_buffers, o, counters);
    (void) hipFree(st.d_fields); (void) hipFree(st.d_def); (void) hipFree(st.d_text);
    free(st.text); free(st.buf);
    if (fclose(st.out) && rc == MGPU_OK) { perror(o->path); rc = MGPU_E_INVAL; }
    return rc;
}
