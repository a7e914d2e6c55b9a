/* readsb_gpu_pf_in.c — readsb's Planefinder input as a filter, with the framing, the CRC stage and the ICAO filter's answers on the
 * GPU: the Planefinder binary feed on stdin or from a file (what arrives on --net-pfms-in-port), the messages decodePfMessage
 * (net_io.c:3995-4101) accepts on stdout as a beast stream (mgpu_beast_encode_ex: modesSendBeastOutput, net_io.c:1655-1714), repaired,
 * in stream order; the counters on stderr.
 * Blocks of the input go through mgpu_pf_decode.  A frame has no bounded length and its decode reads up to 53 bytes from its start
 * whatever they are, so a block is framed without its last 53 bytes while more input can come: they are handed over as args->look, and
 * the bytes behind the som a block reached are carried into the next one.  The context's filter carries what the earlier blocks
 * taught it.  The output is that of one call over the whole input.
 *   readsb_gpu_pf_in [--fix | --aggressive | --no-fix] [--no-fix-df] [--mode-ac] [--verbatim] [--now MS] [--block BYTES] [--device N] [FILE]
 * --verbatim writes the frames as received (--net-verbatim).  The filter starts empty and nothing expires it (cfg.filter_clock =
 * MGPU_FILTER_CLOCK_EXTERNAL). */
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "../../include/modes_gpu.h"

#define PF_REACH 53                                 /* what a handler call reads from its start DLE at the most */

int main(int argc, char **argv) {
    size_t block = 16u << 20;
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    int64_t now_ms = (int64_t) ts.tv_sec * 1000 + ts.tv_nsec / 1000000;
    struct mgpu_config cfg;
    mgpu_config_defaults(&cfg);
    cfg.max_samples = 131072;                      /* no feed is made: the demodulator's buffers at their smallest */
    cfg.filter_clock = MGPU_FILTER_CLOCK_EXTERNAL;
    uint32_t verbatim = 0;
    const char *path = NULL;
    for (int k = 1; k < argc; ++k) {
        if (!strcmp(argv[k], "--block") && k + 1 < argc) block = (size_t) strtoull(argv[++k], NULL, 0);
        else if (!strcmp(argv[k], "--device") && k + 1 < argc) cfg.device = atoi(argv[++k]);
        else if (!strcmp(argv[k], "--now") && k + 1 < argc) now_ms = atoll(argv[++k]);
        else if (!strcmp(argv[k], "--fix")) cfg.nfix_crc = 1;
        else if (!strcmp(argv[k], "--no-fix")) cfg.nfix_crc = 0;
        else if (!strcmp(argv[k], "--aggressive")) cfg.nfix_crc = 2;
        else if (!strcmp(argv[k], "--no-fix-df")) cfg.fixDF = 0;
        else if (!strcmp(argv[k], "--mode-ac") || !strcmp(argv[k], "--modeac")) cfg.mode_ac = 1;
        else if (!strcmp(argv[k], "--verbatim")) verbatim = 1;
        else if (argv[k][0] != '-' && !path) path = argv[k];
        else {
            fprintf(stderr, "usage: %s [--fix | --aggressive | --no-fix] [--no-fix-df] [--mode-ac] [--verbatim] [--now MS] [--block BYTES] [--device N] [FILE]\n", argv[0]);
            return 2;
        }
    }
    int fd = 0;
    if (path && (fd = open(path, O_RDONLY)) < 0) { perror(path); return 1; }
    if (block < 4 * PF_REACH) block = 4 * PF_REACH;
    mgpu_ctx *ctx = NULL;
    int rc = mgpu_create(&cfg, &ctx);
    if (rc != MGPU_OK) { fprintf(stderr, "mgpu_create: %s\n", mgpu_strerror(rc)); return 1; }
    size_t room = block, have = 0, msg_room = 0;
    uint8_t *in = malloc(room), *out = NULL;
    struct mgpu_msg *msgs = NULL;
    struct mgpu_pf_in_counters all;
    memset(&all, 0, sizeof all);
    uint64_t all_frames = 0, all_msgs = 0, all_bytes = 0;
    int eof = 0;
    while (rc == MGPU_OK && in && !(eof && have == 0)) {
        while (!eof && have < room) {
            ssize_t r = read(fd, in + have, room - have);
            if (r > 0) have += (size_t) r;
            else if (r == 0) eof = 1;
            else if (errno != EINTR) { perror("read"); rc = MGPU_E_INVAL; break; }
        }
        if (rc != MGPU_OK) break;
        /* while more can come, the last PF_REACH bytes are looked at and read, not framed (the buffer is full here: have == room) */
        const size_t look = eof ? 0 : PF_REACH, framed = have - look;
        const size_t most = framed / 4 + 1;         /* a handler call needs 4 bytes */
        if (most > msg_room) {
            free(msgs); free(out);
            msgs = malloc(most * sizeof *msgs);
            out = malloc(most * 64);                /* a frame: at most 2 + 2 * (6 + 1 + 14) bytes */
            msg_room = most;
        }
        if (!msgs || !out) { rc = MGPU_E_NOMEM; break; }
        uint64_t consumed = 0, nframes = 0, nmsgs = 0, bytes = 0;
        struct mgpu_pf_in_counters cn;
        struct mgpu_pf_in_args a;
        memset(&a, 0, sizeof a);
        a.size = sizeof a;
        a.data = in; a.nbytes = framed; a.look = (uint32_t) look;
        a.now_ms = now_ms;
        a.msgs = msgs; a.msgs_cap = msg_room;
        a.consumed = &consumed; a.nframes = &nframes; a.nmsgs = &nmsgs; a.counters = &cn;
        rc = mgpu_pf_decode(ctx, &a);
        if (rc != MGPU_OK) { fprintf(stderr, "mgpu_pf_decode: %s (%s)\n", mgpu_strerror(rc), mgpu_last_error(ctx)); break; }
        if (nmsgs) {
            struct mgpu_beast_args e;
            memset(&e, 0, sizeof e);
            e.size = sizeof e;
            e.flags = verbatim ? MGPU_BEAST_VERBATIM : 0;
            e.msgs = msgs; e.n = nmsgs;
            e.out = out; e.cap = msg_room * 64; e.bytes = &bytes;
            rc = mgpu_beast_encode_ex(ctx, &e);
            if (rc != MGPU_OK) { fprintf(stderr, "mgpu_beast_encode_ex: %s (%s)\n", mgpu_strerror(rc), mgpu_last_error(ctx)); break; }
            if (fwrite(out, 1, bytes, stdout) != bytes) { perror("stdout"); rc = MGPU_E_INVAL; break; }
        }
        all.remote_received_modes += cn.remote_received_modes; all.remote_received_modeac += cn.remote_received_modeac;
        all.remote_rejected_unknown_icao += cn.remote_rejected_unknown_icao; all.remote_rejected_bad += cn.remote_rejected_bad;
        for (int k = 0; k < 3; ++k) all.remote_accepted[k] += cn.remote_accepted[k];
        all.nskipped += cn.nskipped; all.past_end += cn.past_end;
        all_frames += nframes; all_msgs += nmsgs;
        all_bytes += consumed;
        if (eof) break;                             /* what is left is a frame without an end, or nothing */
        if (consumed == 0) {                        /* a frame longer than the buffer, or no DLE in it: more of the input at once */
            uint8_t *bigger = realloc(in, 2 * room);
            if (!bigger) { rc = MGPU_E_NOMEM; break; }
            in = bigger; room *= 2;
            continue;
        }
        memmove(in, in + consumed, have - consumed);
        have -= consumed;
    }
    if (!in) rc = MGPU_E_NOMEM;
    if (rc == MGPU_OK && fflush(stdout)) { perror("stdout"); rc = MGPU_E_INVAL; }
    if (rc == MGPU_OK)
        fprintf(stderr, "frames %llu messages %llu consumed %llu remote_received_modes %llu remote_received_modeac %llu remote_rejected_unknown_icao %llu "
                "remote_rejected_bad %llu remote_accepted %llu %llu %llu nskipped %llu past_end %llu\n", (unsigned long long) all_frames, (unsigned long long) all_msgs,
                (unsigned long long) all_bytes, (unsigned long long) all.remote_received_modes, (unsigned long long) all.remote_received_modeac,
                (unsigned long long) all.remote_rejected_unknown_icao, (unsigned long long) all.remote_rejected_bad, (unsigned long long) all.remote_accepted[0],
                (unsigned long long) all.remote_accepted[1], (unsigned long long) all.remote_accepted[2], (unsigned long long) all.nskipped, (unsigned long long) all.past_end);
    free(in); free(msgs); free(out);
    if (fd > 0) close(fd);
    mgpu_destroy(ctx);
    return rc == MGPU_OK ? 0 : 1;
}
