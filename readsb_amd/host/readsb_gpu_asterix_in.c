/* readsb_gpu_asterix_in.c — readsb's ASTERIX input as a filter, with the framing and the decode on the GPU: an ASTERIX capture on stdin
 * (what arrives on --net-asterix-in-port), the records decodeAsterixMessage (net_io.c:1922-2407) leaves for its CAT021 records on
 * stdout as binary struct mgpu_asterix_rec, in stream order.  Blocks of stdin go through mgpu_asterix_decode; the bytes behind the last
 * complete record of a block are carried into the next one.  It stops at a record of length 0, where the reference never returns, and
 * at a CAT021 record without an address, where the reference closes the client; an incomplete last record is not a record.
 *   readsb_gpu_asterix_in [--source N] [--stats] [--now MS] [--block BYTES] [--device N]
 * --source: the reference's datasource_t, 0 .. 11 (1: SOURCE_INDIRECT).
 * --stats: no records; one line "frames N records R other O undefined U bytes B stop S" on stdout instead. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "../../include/modes_gpu.h"

int main(int argc, char **argv) {
    size_t block = 16u << 20;
    uint32_t source = 1;
    int stats = 0;
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    int64_t now_ms = (int64_t) ts.tv_sec * 1000 + ts.tv_nsec / 1000000;
    struct mgpu_config cfg;
    mgpu_config_defaults(&cfg);
    cfg.max_samples = 131072;                      /* no feed is made: the demodulator's buffers at their smallest */
    for (int k = 1; k < argc; ++k) {
        if (!strcmp(argv[k], "--block") && k + 1 < argc) block = (size_t) strtoull(argv[++k], NULL, 0);
        else if (!strcmp(argv[k], "--device") && k + 1 < argc) cfg.device = atoi(argv[++k]);
        else if (!strcmp(argv[k], "--now") && k + 1 < argc) now_ms = atoll(argv[++k]);
        else if (!strcmp(argv[k], "--stats")) stats = 1;
        else if (!strcmp(argv[k], "--source") && k + 1 < argc) source = (uint32_t) strtoul(argv[++k], NULL, 0);
        else { fprintf(stderr, "usage: %s [--source N] [--stats] [--now MS] [--block BYTES] [--device N]\n", argv[0]); return 2; }
    }
    if (block < 1) block = 1;
    mgpu_ctx *ctx = NULL;
    int rc = mgpu_create(&cfg, &ctx);
    if (rc != MGPU_OK) { fprintf(stderr, "mgpu_create: %s\n", mgpu_strerror(rc)); return 1; }
    size_t room = block, have = 0, rec_room = 0;
    uint8_t *in = malloc(room);
    struct mgpu_asterix_rec *recs = NULL;
    uint64_t all_frames = 0, all_recs = 0, all_other = 0, all_undefined = 0, all_bytes = 0;
    uint32_t stop = MGPU_AST_STOP_END;
    int eof = 0;
    while (rc == MGPU_OK && in && stop == MGPU_AST_STOP_END && !(eof && have == 0)) {
        while (!eof && have < room) {
            ssize_t r = read(0, in + have, room - have);
            if (r > 0) have += (size_t) r;
            else if (r == 0) eof = 1;
            else if (errno != EINTR) { perror("stdin"); rc = MGPU_E_INVAL; break; }
        }
        if (rc != MGPU_OK) break;
        uint64_t consumed = 0, nframes = 0, nrecs = 0, nother = 0, nundefined = 0;
        struct mgpu_asterix_in_args a;
        memset(&a, 0, sizeof a);
        a.size = sizeof a;
        a.source = source;
        a.data = in; a.nbytes = have;
        a.now_ms = now_ms;
        a.consumed = &consumed; a.nframes = &nframes; a.nrecs = &nrecs; a.stop = &stop; a.nother = &nother; a.nundefined = &nundefined;
        for (int attempt = 0; attempt < 2; ++attempt) {   /* how many records a block gives is known from a first call */
            a.recs = recs; a.recs_cap = rec_room;
            rc = mgpu_asterix_decode(ctx, &a);
            if (rc != MGPU_E_OVERFLOW || attempt) break;
            free(recs);
            rec_room = nrecs + nrecs / 4 + 16;
            recs = malloc(rec_room * sizeof *recs);
            if (!recs) { rc = MGPU_E_NOMEM; break; }
        }
        if (rc != MGPU_OK) { fprintf(stderr, "mgpu_asterix_decode: %s (%s)\n", mgpu_strerror(rc), mgpu_last_error(ctx)); break; }
        if (!stats && nrecs && fwrite(recs, sizeof *recs, nrecs, stdout) != nrecs) { perror("stdout"); rc = MGPU_E_INVAL; break; }
        if (consumed == 0 && stop == MGPU_AST_STOP_END && !eof) {   /* a record longer than the buffer: a larger buffer */
            uint8_t *bigger = realloc(in, 2 * room);
            if (!bigger) { rc = MGPU_E_NOMEM; break; }
            in = bigger; room *= 2;
            continue;
        }
        all_frames += nframes; all_recs += nrecs; all_other += nother; all_undefined += nundefined; all_bytes += consumed;
        if (eof) have = 0;
        else { memmove(in, in + consumed, have - consumed); have -= consumed; }
    }
    if (!in) rc = MGPU_E_NOMEM;
    if (rc == MGPU_OK && stats)
        printf("frames %llu records %llu other %llu undefined %llu bytes %llu stop %u\n", (unsigned long long) all_frames, (unsigned long long) all_recs,
               (unsigned long long) all_other, (unsigned long long) all_undefined, (unsigned long long) all_bytes, stop);
    if (rc == MGPU_OK && fflush(stdout)) { perror("stdout"); rc = MGPU_E_INVAL; }
    free(in); free(recs);
    mgpu_destroy(ctx);
    return rc == MGPU_OK ? 0 : 1;
}
