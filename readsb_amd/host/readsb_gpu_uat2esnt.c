/* readsb_gpu_uat2esnt.c — dump978's uat2esnt as a filter, with the conversion on the GPU: 978 MHz UAT lines of a dump978 feed on stdin,
 * the DF18 extended squitters readsb's --net-uat-in-port path makes of them (uat2esnt_convert_message, uat2esnt/uat2esnt.c:823) as AVR
 * lines on stdout.  Blocks of stdin go through mgpu_uat_encode; the bytes behind a block's last '\n' are carried into the next one;
 * the lines the device defers (a signal value outside dump978's %.1f form, a line longer than 256 bytes) are settled by
 * mgpu_uat_format_host and written where they belong.  A last line without '\n' is not a line, as in readsb's client buffer.
 *   readsb_gpu_uat2esnt [--block BYTES] [--device N] */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/modes_gpu.h"

#define UAT_TEXT 45u                               /* bytes of one AVR line */

int main(int argc, char **argv) {
    size_t block = 16u << 20;
    struct mgpu_config cfg;
    mgpu_config_defaults(&cfg);
    cfg.max_samples = 131072;                      /* no feed is made: the demodulator's buffers at their smallest */
    for (int k = 1; k < argc; ++k) {
        if (!strcmp(argv[k], "--block") && k + 1 < argc) block = (size_t) strtoull(argv[++k], NULL, 0);
        else if (!strcmp(argv[k], "--device") && k + 1 < argc) cfg.device = atoi(argv[++k]);
        else { fprintf(stderr, "usage: %s [--block BYTES] [--device N]\n", argv[0]); return 2; }
    }
    if (block < 1) block = 1;
    mgpu_ctx *ctx = NULL;
    int rc = mgpu_create(&cfg, &ctx);
    if (rc != MGPU_OK) { fprintf(stderr, "mgpu_create: %s\n", mgpu_strerror(rc)); return 1; }
    size_t room = block, have = 0;
    uint8_t *in = malloc(room), *out = NULL;
    uint64_t *line_of = NULL, *deferred = NULL;
    size_t out_frames = 0, def_room = 0;
    int eof = 0;
    while (rc == MGPU_OK && in && !(eof && have == 0)) {
        while (!eof && have < room) {
            ssize_t r = read(0, in + have, room - have);
            if (r > 0) have += (size_t) r;
            else if (r == 0) eof = 1;
            else if (errno != EINTR) { perror("stdin"); rc = MGPU_E_INVAL; break; }
        }
        if (rc != MGPU_OK) break;
        const size_t frames = have * 4 / 37 + 4, defs = have / 14 + 1;   /* at most 4 frames per 37 bytes of text, a deferred line per 14 */
        if (frames > out_frames) {
            free(out); free(line_of);
            out = malloc(frames * UAT_TEXT); line_of = malloc(frames * sizeof *line_of);
            out_frames = frames;
        }
        if (defs > def_room) { free(deferred); deferred = malloc(defs * sizeof *deferred); def_room = defs; }
        if (!out || !line_of || !deferred) { rc = MGPU_E_NOMEM; break; }
        uint64_t nbytes = 0, consumed = 0, nlines = 0, nframes = 0, nshort = 0, ndef = 0;
        struct mgpu_uat_args a;
        memset(&a, 0, sizeof a);
        a.size = sizeof a;
        a.text = in; a.nbytes = have;
        a.out = out; a.cap = out_frames * UAT_TEXT;
        a.line_of = line_of; a.msgs_cap = out_frames;
        a.deferred = deferred; a.deferred_cap = def_room;
        a.bytes = &nbytes; a.consumed = &consumed; a.nlines = &nlines; a.nframes = &nframes; a.nshort = &nshort; a.ndeferred = &ndef;
        rc = mgpu_uat_encode(ctx, &a);
        if (rc != MGPU_OK) { fprintf(stderr, "mgpu_uat_encode: %s (%s)\n", mgpu_strerror(rc), mgpu_last_error(ctx)); break; }
        uint64_t at = 0;                            /* frames written so far */
        for (uint64_t d = 0; d <= ndef && rc == MGPU_OK; ++d) {
            uint64_t upto = nframes;                /* the frames in front of deferred line d, then the line itself */
            if (d < ndef) for (upto = at; upto < nframes && line_of[upto] < deferred[d]; ++upto) {}
            if (upto > at && fwrite(out + at * UAT_TEXT, UAT_TEXT, upto - at, stdout) != upto - at) rc = MGPU_E_INVAL;
            at = upto;
            if (d < ndef) {
                uint8_t text[4 * UAT_TEXT];
                const int64_t n = mgpu_uat_format_host(&a, deferred[d], text, sizeof text, NULL, NULL);
                if (n < 0 || (n > 0 && fwrite(text, 1, (size_t) n, stdout) != (size_t) n)) rc = MGPU_E_INVAL;
            }
        }
        if (rc != MGPU_OK) { perror("stdout"); break; }
        if (consumed == 0 && !eof) {                /* a line longer than the buffer: a larger buffer */
            uint8_t *bigger = realloc(in, 2 * room);
            if (!bigger) { rc = MGPU_E_NOMEM; break; }
            in = bigger; room *= 2;
            continue;
        }
        if (eof) have = 0;
        else { memmove(in, in + consumed, have - consumed); have -= consumed; }
    }
    if (!in) rc = MGPU_E_NOMEM;
    if (rc == MGPU_OK && fflush(stdout)) { perror("stdout"); rc = MGPU_E_INVAL; }
    free(in); free(out); free(line_of); free(deferred);
    mgpu_destroy(ctx);
    return rc == MGPU_OK ? 0 : 1;
}
