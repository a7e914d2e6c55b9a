/* pf_in_ref_harness.c — runs the REFERENCE's Planefinder input, readPlanefinder (net_io.c:4670-4735) with a read handler that calls
 * decodePfMessage (:3995-4101), the reference's own decodeModesMessage, CRC tables and ICAO filter behind it, over byte streams, and
 * writes what it leaves: tests/golden/make_pf_in_golden.py, tests/test_pf_in_reference.py, tools/bench_pf_in.py (tests/pf_in_util.py:
 * build_ref_harness / run_ref_harness).  The functions are static, so the reference's net_io.c is INCLUDED here (compile with the
 * flags of `make -C oracle full` and -I<reference>) and the program is linked against the other objects of oracle/_ref/full, readsb.o
 * with its main renamed.
 *   pf_in_ref_harness <now_ms> <nfix_crc> <fixDF> <mode_ac> <filter.bin> <reps> <stream.bin> [...]
 * filter.bin: int32 values that prepare the filter after icaoFilterInit(): >= 0 icaoFilterAdd(value), -1 icaoFilterExpire().
 * The streams are run one after the other against the same filter, each as a fresh client.
 * stdout, per stream: uint64 consumed, handler calls, messages, remote_received_modes, remote_received_modeac,
 * remote_rejected_unknown_icao, remote_rejected_bad, remote_accepted[0..2]; per handler call a class byte (MGPU_PF_IN_*, from what the
 * reference counted for it; where it counted nothing, from the type byte its own getNextPfUnstuffedByte gives) and a uint64 offset of
 * its start DLE; per message a uint64 handler-call index, mm->signalLevel, a struct mgpu_msg filled as raw_in_ref_harness.c fills it.
 * Only accepted messages are written (decodePfMessage passes rejected ones to netUseMessage too; the handler takes them off again).
 * The 64 bytes behind the stream are zero: the handler reads up to 53 bytes from a frame's start whatever they are, and the
 * library counts every byte at or beyond the end as 0.
 * reps > 1: everything is run that many times from a fresh filter (for timing; the output is the last run's). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "net_io.c"

#include "modes_gpu.h"

static uint64_t harness_frame, *harness_frame_of, *harness_off;
static uint8_t *harness_class;
static char *harness_buf;

static int harness_read(struct client *c, char *p, int remote, int64_t now, struct messageBuffer *mb) {
    const int before = mb->len;
    const struct stats *st = &Modes.stats_current;
    const uint64_t ac = st->remote_received_modeac, unknown = st->remote_rejected_unknown_icao, bad = st->remote_rejected_bad, modes = st->remote_received_modes;
    harness_off[harness_frame] = (uint64_t) (p - harness_buf);
    const int rc = decodePfMessage(c, p, remote, now, mb);
    uint8_t cls = st->remote_received_modeac != ac ? MGPU_PF_IN_MODEAC : st->remote_rejected_unknown_icao != unknown ? MGPU_PF_IN_UNKNOWN :
                  st->remote_rejected_bad != bad ? MGPU_PF_IN_BAD : st->remote_received_modes != modes ? MGPU_PF_IN_ACCEPT : 0;
    if (!cls) {                                     /* it returned in front of the counters: by the type byte */
        char *q = p + 1;
        (void) getNextPfUnstuffedByte(&q);
        (void) getNextPfUnstuffedByte(&q);
        cls = (getNextPfUnstuffedByte(&q) & 0xF) == 0 ? MGPU_PF_IN_MODEAC_OFF : MGPU_PF_IN_TYPE;
    }
    /* decodePfMessage hands a message it rejected to netUseMessage all the same; the records here are the accepted messages, so a
     * rejected one is taken off the buffer again */
    if (cls == MGPU_PF_IN_UNKNOWN || cls == MGPU_PF_IN_BAD) mb->len = before;
    if (mb->len != before) harness_frame_of[before] = harness_frame;
    harness_class[harness_frame] = cls;
    ++harness_frame;
    return rc;
}

static char *slurp(const char *path, long *size) {
    FILE *in = fopen(path, "rb");
    if (!in) { perror(path); exit(1); }
    fseek(in, 0, SEEK_END);
    *size = ftell(in);
    fseek(in, 0, SEEK_SET);
    char *data = malloc((size_t) *size + 1);
    if (fread(data, 1, (size_t) *size, in) != (size_t) *size) { perror("read"); exit(1); }
    fclose(in);
    return data;
}

int main(int argc, char **argv) {
    if (argc < 8) { fprintf(stderr, "usage: %s now_ms nfix_crc fixDF mode_ac filter.bin reps stream.bin...\n", argv[0]); return 2; }
    const int64_t now = atoll(argv[1]);
    Modes.nfix_crc = atoi(argv[2]);
    Modes.fixDF = atoi(argv[3]);
    Modes.mode_ac = atoi(argv[4]);
    Modes.net_verbatim = 1;
    long fsize = 0;
    int32_t *fops = (int32_t *) slurp(argv[5], &fsize);
    const int reps = atoi(argv[6]);
    const int nstreams = argc - 7;
    modesChecksumInit(Modes.nfix_crc);

    struct net_service service;
    memset(&service, 0, sizeof service);
    service.descr = "planefinder in";
    service.read_handler = harness_read;
    service.read_mode = READ_MODE_PLANEFINDER;

    for (int rep = 0; rep < reps; ++rep) {
        const int last = rep == reps - 1;
        icaoFilterInit();
        for (long k = 0; k < fsize / 4; ++k) {
            if (fops[k] >= 0) icaoFilterAdd((uint32_t) fops[k]); else icaoFilterExpire();
        }
        for (int s = 0; s < nstreams; ++s) {
            long size = 0;
            char *stream = slurp(argv[7 + s], &size);
            char *buf = calloc((size_t) size + 64, 1);
            memcpy(buf, stream, (size_t) size);
            const size_t most = (size_t) size / 4 + 2;
            struct messageBuffer mb;
            memset(&mb, 0, sizeof mb);
            mb.msg = malloc(most * sizeof(struct modesMessage));
            mb.alloc = (int) most;
            harness_frame_of = calloc(most, sizeof(uint64_t));
            harness_off = calloc(most, sizeof(uint64_t));
            harness_class = calloc(most, 1);
            harness_frame = 0;
            harness_buf = buf;
            struct client c;
            memset(&c, 0, sizeof c);
            c.service = &service;
            c.buf = buf;
            c.som = buf;
            c.eod = buf + size;
            c.remote = 1;
            memset(&Modes.stats_current, 0, sizeof Modes.stats_current);
            if (readPlanefinder(&c, now, &mb) != 0) { fprintf(stderr, "readPlanefinder closed the client\n"); return 1; }
            if (last) {
                const struct stats *st = &Modes.stats_current;
                const uint64_t head[10] = {(uint64_t) (c.som - buf), harness_frame, (uint64_t) mb.len, st->remote_received_modes, st->remote_received_modeac,
                                           st->remote_rejected_unknown_icao, st->remote_rejected_bad, st->remote_accepted[0], st->remote_accepted[1], st->remote_accepted[2]};
                fwrite(head, sizeof head, 1, stdout);
                fwrite(harness_class, 1, (size_t) harness_frame, stdout);
                fwrite(harness_off, sizeof(uint64_t), (size_t) harness_frame, stdout);
                fwrite(harness_frame_of, sizeof(uint64_t), (size_t) mb.len, stdout);
                for (int k = 0; k < mb.len; ++k) fwrite(&mb.msg[k].signalLevel, sizeof(double), 1, stdout);
                for (int k = 0; k < mb.len; ++k) {
                    const struct modesMessage *mm = &mb.msg[k];
                    struct mgpu_msg r;
                    memset(&r, 0, sizeof r);
                    int sig = nearbyint(sqrt(mm->signalLevel) * 255);
                    if (mm->signalLevel > 0 && sig < 1) sig = 1;
                    if (sig > 255) sig = 255;
                    r.timestamp = mm->timestamp;
                    r.sysTimestamp = mm->sysTimestamp;
                    r.sig_sumsq = (uint64_t) (257u * (unsigned) sig) * (257u * (unsigned) sig);
                    r.sig_len = 1;
                    r.correctedbits = (uint8_t) mm->correctedbits;
                    r.msgtype = (uint8_t) mm->msgtype;
                    r.msgbits = (uint8_t) mm->msgbits;
                    r.addr = mm->addr & 0xffffffu;             /* (Mode A/C: without MODES_NON_ICAO_ADDRESS, as the demodulator's records) */
                    memcpy(r.msg, mm->msg, 14);
                    memcpy(r.raw, mm->verbatim, 14);
                    fwrite(&r, sizeof r, 1, stdout);
                }
            }
            free(mb.msg); free(harness_frame_of); free(harness_off); free(harness_class); free(buf); free(stream);
        }
    }
    return fflush(stdout) ? 1 : 0;
}
