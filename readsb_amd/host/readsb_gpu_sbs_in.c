/* readsb_gpu_sbs_in.c — readsb's SBS input as a filter, with the parse on the GPU: a BaseStation capture on stdin (what arrives on
 * --net-sbs-in-port, the MLAT results port, the JAERO and PRIO ports), the records decodeSbsLine (net_io.c:2952-3178) leaves on stdout as
 * binary struct mgpu_sbs_rec, in line order.  Blocks of stdin go through mgpu_sbs_decode; the bytes behind a block's last terminator
 * ('\n' or NUL) are carried into the next one; the lines the device defers (a number outside the plain forms) are settled by
 * mgpu_sbs_parse_host and written where they belong.  A last line without a terminator is not a line, as in readsb's client buffer.
 *   readsb_gpu_sbs_in [--source sbs|mlat|jaero|prio] [--stats] [--now MS] [--block BYTES] [--device N]
 * --stats: no records; one line "lines N records R invalid I deferred D bytes B" on stdout instead. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "../../include/modes_gpu.h"

int main(int argc, char **argv) {
    size_t block = 16u << 20;
    uint32_t source = MGPU_SBS_SOURCE_SBS;
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
        else if (!strcmp(argv[k], "--source") && k + 1 < argc) {
            const char *s = argv[++k];
            if (!strcmp(s, "sbs")) source = MGPU_SBS_SOURCE_SBS;
            else if (!strcmp(s, "mlat")) source = MGPU_SBS_SOURCE_MLAT;
            else if (!strcmp(s, "jaero")) source = MGPU_SBS_SOURCE_JAERO;
            else if (!strcmp(s, "prio")) source = MGPU_SBS_SOURCE_PRIO;
            else { fprintf(stderr, "--source sbs|mlat|jaero|prio\n"); return 2; }
        } else { fprintf(stderr, "usage: %s [--source sbs|mlat|jaero|prio] [--stats] [--now MS] [--block BYTES] [--device N]\n", argv[0]); return 2; }
    }
    if (block < 1) block = 1;
    mgpu_ctx *ctx = NULL;
    int rc = mgpu_create(&cfg, &ctx);
    if (rc != MGPU_OK) { fprintf(stderr, "mgpu_create: %s\n", mgpu_strerror(rc)); return 1; }
    size_t room = block, have = 0, rec_room = 0;
    uint8_t *in = malloc(room);
    struct mgpu_sbs_rec *recs = NULL;
    uint64_t *line_of = NULL, *deferred = NULL;
    uint64_t all_lines = 0, all_recs = 0, all_invalid = 0, all_deferred = 0, all_bytes = 0;
    int eof = 0;
    while (rc == MGPU_OK && in && !(eof && have == 0)) {
        while (!eof && have < room) {
            ssize_t r = read(0, in + have, room - have);
            if (r > 0) have += (size_t) r;
            else if (r == 0) eof = 1;
            else if (errno != EINTR) { perror("stdin"); rc = MGPU_E_INVAL; break; }
        }
        if (rc != MGPU_OK) break;
        const size_t most = have / 21 + 1;          /* a record, or a deferred line, has 20 bytes and a terminator */
        if (most > rec_room) {
            free(recs); free(line_of); free(deferred);
            recs = malloc(most * sizeof *recs); line_of = malloc(most * sizeof *line_of); deferred = malloc(most * sizeof *deferred);
            rec_room = most;
        }
        if (!recs || !line_of || !deferred) { rc = MGPU_E_NOMEM; break; }
        uint64_t consumed = 0, nlines = 0, nrecs = 0, ninvalid = 0, ndef = 0;
        struct mgpu_sbs_in_args a;
        memset(&a, 0, sizeof a);
        a.size = sizeof a;
        a.source = source;
        a.text = in; a.nbytes = have;
        a.now_ms = now_ms;
        a.recs = recs; a.line_of = line_of; a.recs_cap = rec_room;
        a.deferred = deferred; a.deferred_cap = rec_room;
        a.consumed = &consumed; a.nlines = &nlines; a.nrecs = &nrecs; a.ninvalid = &ninvalid; a.ndeferred = &ndef;
        rc = mgpu_sbs_decode(ctx, &a);
        if (rc != MGPU_OK) { fprintf(stderr, "mgpu_sbs_decode: %s (%s)\n", mgpu_strerror(rc), mgpu_last_error(ctx)); break; }
        uint64_t at = 0;                            /* records written so far */
        for (uint64_t d = 0; d <= ndef && rc == MGPU_OK; ++d) {
            uint64_t upto = nrecs;                  /* the records in front of deferred line d, then the line's own */
            if (d < ndef) for (upto = at; upto < nrecs && line_of[upto] < deferred[d]; ++upto) {}
            if (!stats && upto > at && fwrite(recs + at, sizeof *recs, upto - at, stdout) != upto - at) rc = MGPU_E_INVAL;
            at = upto;
            if (d < ndef) {
                struct mgpu_sbs_rec r;
                const int n = mgpu_sbs_parse_host(&a, deferred[d], &r);
                if (n < 0 || (n == 1 && !stats && fwrite(&r, sizeof r, 1, stdout) != 1)) rc = MGPU_E_INVAL;
                if (n == 1) ++all_recs;
            }
        }
        if (rc != MGPU_OK) { perror("stdout"); break; }
        if (consumed == 0 && !eof) {                /* a line longer than the buffer: a larger buffer */
            uint8_t *bigger = realloc(in, 2 * room);
            if (!bigger) { rc = MGPU_E_NOMEM; break; }
            in = bigger; room *= 2;
            continue;
        }
        all_lines += nlines; all_recs += nrecs; all_invalid += ninvalid; all_deferred += ndef; all_bytes += consumed;
        if (eof) have = 0;
        else { memmove(in, in + consumed, have - consumed); have -= consumed; }
    }
    if (!in) rc = MGPU_E_NOMEM;
    if (rc == MGPU_OK && stats)
        printf("lines %llu records %llu invalid %llu deferred %llu bytes %llu\n", (unsigned long long) all_lines, (unsigned long long) all_recs,
               (unsigned long long) all_invalid, (unsigned long long) all_deferred, (unsigned long long) all_bytes);
    if (rc == MGPU_OK && fflush(stdout)) { perror("stdout"); rc = MGPU_E_INVAL; }
    free(in); free(recs); free(line_of); free(deferred);
    mgpu_destroy(ctx);
    return rc == MGPU_OK ? 0 : 1;
}
