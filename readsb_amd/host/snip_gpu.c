/* snip_gpu.c — readsb_gpu_ifile --snip LEVEL: `readsb --snip <level>` (snipMode, readsb.c:1187-1206, dispatched at :1581-1583) with
 * the filter on the GPU.  UC8 bytes from `fd` to stdout in blocks through mgpu_snip, the quiet-run counter carried from block to
 * block; a trailing odd byte is dropped, as the reference's pairs of getchar() drop it. */
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include "readsb_gpu_host.h"

#define SNIP_BLOCK_SAMPLES (32u << 20)             /* 64 MiB of input per call */

int gpu_snip_run(const struct mgpu_config *cfg_in, int fd, int level) {
    struct mgpu_config cfg = *cfg_in;
    cfg.max_samples = 131072;                      /* no feed is made: the demodulator's buffers at their smallest */
    mgpu_ctx *ctx = NULL;
    int rc = mgpu_create(&cfg, &ctx);
    if (rc != MGPU_OK) { fprintf(stderr, "mgpu_create: %s\n", mgpu_strerror(rc)); return rc; }
    const size_t want = (size_t) SNIP_BLOCK_SAMPLES * 2;
    uint8_t *in = malloc(want), *out = malloc(want);
    if (!in || !out) { free(in); free(out); mgpu_destroy(ctx); return MGPU_E_NOMEM; }
    uint64_t run = 0;
    for (int last = 0; !last && rc == MGPU_OK;) {
        size_t have = 0;
        while (have < want) {
            ssize_t r = read(fd, in + have, want - have);
            if (r <= 0) break;
            have += (size_t) r;
        }
        last = have < want;
        uint64_t nout = 0;
        struct mgpu_snip_args a = {sizeof a, level, in, have / 2, out, have / 2, &nout, &run, 0};
        rc = mgpu_snip(ctx, &a);
        if (rc != MGPU_OK) fprintf(stderr, "mgpu_snip: %s (%s)\n", mgpu_strerror(rc), mgpu_last_error(ctx));
        else if (nout && fwrite(out, 2, nout, stdout) != nout) { perror("stdout"); rc = MGPU_E_INVAL; }
    }
    if (rc == MGPU_OK && fflush(stdout)) { perror("stdout"); rc = MGPU_E_INVAL; }
    free(in); free(out);
    mgpu_destroy(ctx);
    return rc;
}
