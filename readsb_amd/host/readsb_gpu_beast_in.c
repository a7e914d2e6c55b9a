/* readsb_gpu_beast_in.c — readsb's beast input as a filter, with the framing, the CRC stage and the ICAO filter's answers on the GPU:
 * beast binary on stdin or from a file (what arrives on --net-bi-port), the messages decodeBinMessage (net_io.c:3804-3961) accepts
 * on stdout as a beast stream again (mgpu_beast_encode_ex: modesSendBeastOutput, net_io.c:1655-1714), repaired and each behind the
 * receiver id that was in force at its frame, in stream order; the counters on stderr.
 * Blocks of the input go through mgpu_beast_decode; the bytes behind the last som a block reached are carried into the next one with
 * the receiver id, and the context's filter carries what the earlier blocks taught it.  A UUID (0xe4) or synthetic-time (0xe8) frame
 * stops a call: it is reported on stderr and stepped over here on the host as the reference steps over it — 0x1a 0xe8 and the eight
 * bytes memcpy'd as the timestamp (:4781-4797, no un-escaping there); 0x1a 0xe4 and what read_uuid's scan takes (:5744-5789: up to
 * 128 bytes, 32 hex digits, '-' and ' ' passed over, ending behind a 0x1a or an illegal byte it meets) — neither the time nor the UUID
 * is used; the bytes stepped over are counted on stderr (skipped).
 *   readsb_gpu_beast_in [--fix | --aggressive | --no-fix] [--no-fix-df] [--mode-ac] [--verbatim] [--net-ingest] [--now MS]
 *                       [--block BYTES] [--device N] [FILE]
 * --verbatim writes the frames as received (--net-verbatim); --net-ingest ignores the stream's receiver ids (the id stays 0).
 * The filter starts empty and nothing expires it (cfg.filter_clock = MGPU_FILTER_CLOCK_EXTERNAL). */
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "../../include/modes_gpu.h"

/* the bytes of the stopping frame at in[0 .. have): what the reference's loop leaves behind it */
static size_t stop_length(const uint8_t *in, size_t have, uint32_t stop, int *cut) {
    *cut = 0;
    if (stop == MGPU_BEAST_STOP_SYNTH) return 10;   /* (the stop is reported only with its eight bytes there) */
    size_t p = 2;                                   /* read_uuid with receiverIdLocked == 0 */
    int j = 0;
    for (int i = 0; i < 128 && j < 32; i++) {
        if (p >= have) { *cut = 1; break; }         /* the scan ran into the end of what is here */
        const uint8_t ch = in[p++];
        if (ch == 0x1a) break;
        if (ch == '-' || ch == ' ') continue;
        if (!((ch >= 'a' && ch <= 'f') || (ch >= '0' && ch <= '9') || (ch >= 'A' && ch <= 'F'))) break;
        j++;
    }
    return p;
}

int main(int argc, char **argv) {
    size_t block = 16u << 20;
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    int64_t now_ms = (int64_t) ts.tv_sec * 1000 + ts.tv_nsec / 1000000;
    struct mgpu_config cfg;
    mgpu_config_defaults(&cfg);
    cfg.max_samples = 131072;                      /* no feed is made: the demodulator's buffers at their smallest */
    cfg.filter_clock = MGPU_FILTER_CLOCK_EXTERNAL;
    uint32_t verbatim = 0, net_ingest = 0;
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
        else if (!strcmp(argv[k], "--net-ingest")) net_ingest = 1;
        else if (argv[k][0] != '-' && !path) path = argv[k];
        else {
            fprintf(stderr, "usage: %s [--fix | --aggressive | --no-fix] [--no-fix-df] [--mode-ac] [--verbatim] [--net-ingest] [--now MS] [--block BYTES] [--device N] [FILE]\n", argv[0]);
            return 2;
        }
    }
    int fd = 0;
    if (path && (fd = open(path, O_RDONLY)) < 0) { perror(path); return 1; }
    if (block < 64) block = 64;
    mgpu_ctx *ctx = NULL;
    int rc = mgpu_create(&cfg, &ctx);
    if (rc != MGPU_OK) { fprintf(stderr, "mgpu_create: %s\n", mgpu_strerror(rc)); return 1; }
    size_t room = block, have = 0, msg_room = 0;
    uint8_t *in = malloc(room), *out = NULL;
    struct mgpu_msg *msgs = NULL;
    uint64_t *ids = NULL;
    struct mgpu_beast_in_counters all;
    memset(&all, 0, sizeof all);
    uint64_t all_frames = 0, all_msgs = 0, all_bytes = 0, receiver_id = 0, writer_id = 0, stops = 0, skipped = 0;
    int eof = 0;
    while (rc == MGPU_OK && in && !(eof && have == 0)) {
        while (!eof && have < room) {
            ssize_t r = read(fd, in + have, room - have);
            if (r > 0) have += (size_t) r;
            else if (r == 0) eof = 1;
            else if (errno != EINTR) { perror("read"); rc = MGPU_E_INVAL; break; }
        }
        if (rc != MGPU_OK) break;
        const size_t most = have / 11 + 1;          /* a message needs 11 bytes */
        if (most > msg_room) {
            free(msgs); free(out); free(ids);
            msgs = malloc(most * sizeof *msgs);
            ids = malloc(most * sizeof *ids);
            out = malloc(most * 64);                /* a prefix and a frame: at most 18 + 2 + 2 * (6 + 1 + 14) bytes */
            msg_room = most;
        }
        if (!msgs || !out || !ids) { rc = MGPU_E_NOMEM; break; }
        uint64_t consumed = 0, nframes = 0, nmsgs = 0, stop_off = 0, bytes = 0;
        uint32_t stop = MGPU_BEAST_STOP_END;
        struct mgpu_beast_in_counters cn;
        struct mgpu_beast_in_args a;
        memset(&a, 0, sizeof a);
        a.size = sizeof a;
        a.data = in; a.nbytes = have;
        a.now_ms = now_ms;
        a.receiver_id_in = receiver_id; a.net_ingest = net_ingest;
        a.msgs = msgs; a.receiver_id = ids; a.msgs_cap = msg_room;
        a.consumed = &consumed; a.nframes = &nframes; a.nmsgs = &nmsgs; a.stop = &stop; a.stop_off = &stop_off; a.receiver_id_out = &receiver_id; a.counters = &cn;
        rc = mgpu_beast_decode(ctx, &a);
        if (rc != MGPU_OK) { fprintf(stderr, "mgpu_beast_decode: %s (%s)\n", mgpu_strerror(rc), mgpu_last_error(ctx)); break; }
        if (nmsgs) {
            struct mgpu_beast_args e;
            memset(&e, 0, sizeof e);
            e.size = sizeof e;
            e.flags = verbatim ? MGPU_BEAST_VERBATIM : 0;
            e.msgs = msgs; e.n = nmsgs; e.ids = ids; e.last_id = &writer_id;
            e.out = out; e.cap = msg_room * 64; e.bytes = &bytes;
            rc = mgpu_beast_encode_ex(ctx, &e);
            if (rc != MGPU_OK) { fprintf(stderr, "mgpu_beast_encode_ex: %s (%s)\n", mgpu_strerror(rc), mgpu_last_error(ctx)); break; }
            if (fwrite(out, 1, bytes, stdout) != bytes) { perror("stdout"); rc = MGPU_E_INVAL; break; }
        }
        all.remote_received_modes += cn.remote_received_modes; all.remote_received_modeac += cn.remote_received_modeac;
        all.remote_rejected_unknown_icao += cn.remote_rejected_unknown_icao; all.remote_rejected_bad += cn.remote_rejected_bad;
        for (int k = 0; k < 3; ++k) all.remote_accepted[k] += cn.remote_accepted[k];
        all.remote_malformed_beast += cn.remote_malformed_beast; all.nreceiver_ids += cn.nreceiver_ids; all.ncommands += cn.ncommands;
        all_frames += nframes; all_msgs += nmsgs;
        int cut = 0;
        const size_t len = stop != MGPU_BEAST_STOP_END ? stop_length(in + stop_off, have - stop_off, stop, &cut) : 0;
        if (stop != MGPU_BEAST_STOP_END && cut && !eof) {   /* a UUID that runs into the end of the buffer: up to it now, the frame with more input */
            consumed = stop_off;
            if (consumed == 0 && have == room) {
                uint8_t *bigger = realloc(in, 2 * room);
                if (!bigger) { rc = MGPU_E_NOMEM; break; }
                in = bigger; room *= 2;
            }
        } else if (stop != MGPU_BEAST_STOP_END) {   /* reported and stepped over on the host */
            fprintf(stderr, "%s frame at byte %llu: skipped %llu bytes\n", stop == MGPU_BEAST_STOP_UUID ? "UUID (0xe4)" : "synthetic timestamp (0xe8)",
                    (unsigned long long) (all_bytes + stop_off), (unsigned long long) len);
            consumed = stop_off + len;
            skipped += len;
            ++stops;
        } else if (consumed == 0 && !eof) {         /* a frame that needs more than the buffer holds cannot be: the buffer has 64 bytes at least */
            uint8_t *bigger = realloc(in, 2 * room);
            if (!bigger) { rc = MGPU_E_NOMEM; break; }
            in = bigger; room *= 2;
            continue;
        }
        all_bytes += consumed;
        if (eof && stop == MGPU_BEAST_STOP_END) have = 0;
        else { memmove(in, in + consumed, have - consumed); have -= consumed; }
    }
    if (!in) rc = MGPU_E_NOMEM;
    if (rc == MGPU_OK && fflush(stdout)) { perror("stdout"); rc = MGPU_E_INVAL; }
    if (rc == MGPU_OK)
        fprintf(stderr, "frames %llu messages %llu bytes %llu stops %llu skipped %llu remote_received_modes %llu remote_received_modeac %llu remote_rejected_unknown_icao %llu "
                "remote_rejected_bad %llu remote_accepted %llu %llu %llu remote_malformed_beast %llu receiver_ids %llu commands %llu\n", (unsigned long long) all_frames,
                (unsigned long long) all_msgs, (unsigned long long) all_bytes, (unsigned long long) stops, (unsigned long long) skipped, (unsigned long long) all.remote_received_modes,
                (unsigned long long) all.remote_received_modeac, (unsigned long long) all.remote_rejected_unknown_icao, (unsigned long long) all.remote_rejected_bad,
                (unsigned long long) all.remote_accepted[0], (unsigned long long) all.remote_accepted[1], (unsigned long long) all.remote_accepted[2],
                (unsigned long long) all.remote_malformed_beast, (unsigned long long) all.nreceiver_ids, (unsigned long long) all.ncommands);
    free(in); free(msgs); free(out); free(ids);
    if (fd > 0) close(fd);
    mgpu_destroy(ctx);
    return rc == MGPU_OK ? 0 : 1;
}
