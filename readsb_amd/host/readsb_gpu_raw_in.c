/* readsb_gpu_raw_in.c — readsb's raw input as a filter, with the parse, the CRC stage and the ICAO filter's answers on the GPU: AVR
 * text on stdin (what arrives on --net-ri-port), the messages decodeHexMessage (net_io.c:4104-4287) accepts on stdout as a beast
 * stream (mgpu_beast_encode: modesSendBeastOutput, net_io.c:1655-1714), in line order; the counters of decodeHexMessage on stderr.
 * Blocks of stdin go through mgpu_raw_decode; the bytes behind a block's last terminator ('\n' or NUL) are carried into the next
 * one, and the context's filter carries what the earlier blocks taught it.  A last line without a terminator is not a line, as in
 * readsb's client buffer.
 *   readsb_gpu_raw_in [--fix | --aggressive | --no-fix] [--no-fix-df] [--modeac] [--now MS] [--block BYTES] [--device N]
 * The filter starts empty and nothing expires it (cfg.filter_clock = MGPU_FILTER_CLOCK_EXTERNAL): a host that runs the reference's
 * 60 s clock calls mgpu_filter_expire between blocks. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "../../include/modes_gpu.h"

int main(int argc, char **argv) {
    size_t block = 16u << 20;
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    int64_t now_ms = (int64_t) ts.tv_sec * 1000 + ts.tv_nsec / 1000000;
    struct mgpu_config cfg;
    mgpu_config_defaults(&cfg);
    cfg.max_samples = 131072;                      /* no feed is made: the demodulator's buffers at their smallest */
    cfg.filter_clock = MGPU_FILTER_CLOCK_EXTERNAL;
    for (int k = 1; k < argc; ++k) {
        if (!strcmp(argv[k], "--block") && k + 1 < argc) block = (size_t) strtoull(argv[++k], NULL, 0);
        else if (!strcmp(argv[k], "--device") && k + 1 < argc) cfg.device = atoi(argv[++k]);
        else if (!strcmp(argv[k], "--now") && k + 1 < argc) now_ms = atoll(argv[++k]);
        else if (!strcmp(argv[k], "--fix")) cfg.nfix_crc = 1;
        else if (!strcmp(argv[k], "--no-fix")) cfg.nfix_crc = 0;
        else if (!strcmp(argv[k], "--aggressive")) cfg.nfix_crc = 2;
        else if (!strcmp(argv[k], "--no-fix-df")) cfg.fixDF = 0;
        else if (!strcmp(argv[k], "--modeac")) cfg.mode_ac = 1;
        else { fprintf(stderr, "usage: %s [--fix | --aggressive | --no-fix] [--no-fix-df] [--modeac] [--now MS] [--block BYTES] [--device N]\n", argv[0]); return 2; }
    }
    if (block < 1) block = 1;
    mgpu_ctx *ctx = NULL;
    int rc = mgpu_create(&cfg, &ctx);
    if (rc != MGPU_OK) { fprintf(stderr, "mgpu_create: %s\n", mgpu_strerror(rc)); return 1; }
    size_t room = block, have = 0, msg_room = 0;
    uint8_t *in = malloc(room), *out = NULL;
    struct mgpu_msg *msgs = NULL;
    struct mgpu_raw_in_counters all;
    memset(&all, 0, sizeof all);
    uint64_t all_lines = 0, all_msgs = 0, all_bytes = 0;
    int eof = 0;
    while (rc == MGPU_OK && in && !(eof && have == 0)) {
        while (!eof && have < room) {
            ssize_t r = read(0, in + have, room - have);
            if (r > 0) have += (size_t) r;
            else if (r == 0) eof = 1;
            else if (errno != EINTR) { perror("stdin"); rc = MGPU_E_INVAL; break; }
        }
        if (rc != MGPU_OK) break;
        const size_t most = have / 6 + 1;           /* a line that gives a message has 5 bytes and a terminator */
        if (most > msg_room) {
            free(msgs); free(out);
            msgs = malloc(most * sizeof *msgs);
            out = malloc(most * 46);                /* a beast frame: 0x1a, the type, and at most 2 * (6 + 1 + 14) escaped bytes */
            msg_room = most;
        }
        if (!msgs || !out) { rc = MGPU_E_NOMEM; break; }
        uint64_t consumed = 0, nlines = 0, nmsgs = 0, bytes = 0;
        struct mgpu_raw_in_counters cn;
        struct mgpu_raw_in_args a;
        memset(&a, 0, sizeof a);
        a.size = sizeof a;
        a.text = in; a.nbytes = have;
        a.now_ms = now_ms;
        a.msgs = msgs; a.msgs_cap = msg_room;
        a.consumed = &consumed; a.nlines = &nlines; a.nmsgs = &nmsgs; a.counters = &cn;
        /* (a line longer than the block: mgpu_raw_decode consumes nothing and leaves the filter alone; the block grows) */
        rc = mgpu_raw_decode(ctx, &a);
        if (rc != MGPU_OK) { fprintf(stderr, "mgpu_raw_decode: %s (%s)\n", mgpu_strerror(rc), mgpu_last_error(ctx)); break; }
        if (consumed == 0 && !eof) {                /* a line longer than the buffer: a larger buffer */
            uint8_t *bigger = realloc(in, 2 * room);
            if (!bigger) { rc = MGPU_E_NOMEM; break; }
            in = bigger; room *= 2;
            continue;
        }
        if (nmsgs) {
            rc = mgpu_beast_encode(ctx, msgs, nmsgs, out, msg_room * 46, &bytes);
            if (rc != MGPU_OK) { fprintf(stderr, "mgpu_beast_encode: %s (%s)\n", mgpu_strerror(rc), mgpu_last_error(ctx)); break; }
            if (fwrite(out, 1, bytes, stdout) != bytes) { perror("stdout"); rc = MGPU_E_INVAL; break; }
        }
        all.remote_received_modes += cn.remote_received_modes; all.remote_received_modeac += cn.remote_received_modeac;
        all.remote_rejected_unknown_icao += cn.remote_rejected_unknown_icao; all.remote_rejected_bad += cn.remote_rejected_bad;
        for (int k = 0; k < 3; ++k) all.remote_accepted[k] += cn.remote_accepted[k];
        all_lines += nlines; all_msgs += nmsgs; all_bytes += consumed;
        if (eof) have = 0;
        else { memmove(in, in + consumed, have - consumed); have -= consumed; }
    }
    if (!in) rc = MGPU_E_NOMEM;
    if (rc == MGPU_OK && fflush(stdout)) { perror("stdout"); rc = MGPU_E_INVAL; }
    if (rc == MGPU_OK)
        fprintf(stderr, "lines %llu messages %llu bytes %llu remote_received_modes %llu remote_received_modeac %llu remote_rejected_unknown_icao %llu "
                "remote_rejected_bad %llu remote_accepted %llu %llu %llu\n", (unsigned long long) all_lines, (unsigned long long) all_msgs, (unsigned long long) all_bytes,
                (unsigned long long) all.remote_received_modes, (unsigned long long) all.remote_received_modeac, (unsigned long long) all.remote_rejected_unknown_icao,
                (unsigned long long) all.remote_rejected_bad, (unsigned long long) all.remote_accepted[0], (unsigned long long) all.remote_accepted[1],
                (unsigned long long) all.remote_accepted[2]);
    free(in); free(msgs); free(out);
    mgpu_destroy(ctx);
    return rc == MGPU_OK ? 0 : 1;
}
