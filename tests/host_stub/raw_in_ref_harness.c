/* raw_in_ref_harness.c — runs the REFERENCE's raw input, readAscii (net_io.c:4599-4641) with processHexMessage -> decodeHexMessage
 * (net_io.c:4104-4317) as the service's read handler and the reference's own decodeModesMessage, CRC tables and ICAO filter behind
 * it, over byte streams, and writes what it leaves in every message that was used: tests/golden/make_raw_in_golden.py,
 * tests/test_raw_in_reference.py, tools/bench_raw_in.py (tests/raw_in_util.py: build_ref_harness / run_ref_harness).  The functions
 * are static, so the reference's net_io.c is INCLUDED here (compile with the flags of `make -C oracle full` and -I<reference>) and
 * the program is linked against the other objects of oracle/_ref/full (mode_s.o, crc.o, icao_filter.o, mode_ac.o among them),
 * readsb.o with its main renamed (objcopy --redefine-sym main=readsb_main).
 *   raw_in_ref_harness <now_ms> <nfix_crc> <fixDF> <mode_ac> <filter.bin> <reps> <stream.bin> [<stream.bin> ...]
 * filter.bin: int32 values that prepare the filter after icaoFilterInit(): >= 0 icaoFilterAdd(value), -1 icaoFilterExpire().
 * The streams are run one after the other against the same filter.  stdout, per stream: uint64 consumed, lines, messages, then the
 * counters remote_received_modes, remote_received_modeac, remote_rejected_unknown_icao, remote_rejected_bad, remote_accepted[0..2];
 * per line a class byte (MGPU_RAW_*, from what the reference counted for the line); per message a uint64 line index; per message mm->signalLevel; per message a struct mgpu_msg (include/modes_gpu.h), filled member by
 * member from the modesMessage — raw from mm->verbatim, which decodeModesMessage fills before it repairs anything when
 * Modes.net_verbatim is set; sig_sumsq from the signal byte the reference's beast writer gives mm->signalLevel (net_io.c:1696-1700).
 * The byte in front of the first line is a NUL (an empty line makes the reference read it).
 * reps > 1: everything is run that many times from a fresh filter (for timing; the output is the last run's). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "net_io.c"

#include "modes_gpu.h"

static uint64_t harness_line, *harness_line_of;
static uint8_t *harness_class;

static int harness_read(struct client *c, char *line, int remote, int64_t now, struct messageBuffer *mb) {
    const int before = mb->len;
    const struct stats *st = &Modes.stats_current;
    const uint64_t ac = st->remote_received_modeac, unknown = st->remote_rejected_unknown_icao, bad = st->remote_rejected_bad, modes = st->remote_received_modes;
    const int rc = processHexMessage(c, line, remote, now, mb);
    if (mb->len != before) harness_line_of[before] = harness_line;
    /* the line's class from what the reference counted for it (MGPU_RAW_*) */
    harness_class[harness_line] = st->remote_received_modeac != ac ? MGPU_RAW_MODEAC : st->remote_rejected_unknown_icao != unknown ? MGPU_RAW_UNKNOWN :
                                  st->remote_rejected_bad != bad ? MGPU_RAW_BAD : st->remote_received_modes != modes ? MGPU_RAW_ACCEPT : MGPU_RAW_NONE;
    ++harness_line;
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
    service.descr = "raw in";
    service.read_sep = "\n";
    service.read_sep_len = 1;
    service.read_handler = harness_read;
    service.read_mode = READ_MODE_ASCII;

    for (int rep = 0; rep < reps; ++rep) {
        const int last = rep == reps - 1;
        icaoFilterInit();
        for (long k = 0; k < fsize / 4; ++k) {
            if (fops[k] >= 0) icaoFilterAdd((uint32_t) fops[k]); else icaoFilterExpire();
        }
        for (int s = 0; s < nstreams; ++s) {
            long size = 0;
            char *stream = slurp(argv[7 + s], &size);
            char *mem = malloc((size_t) size + 2), *buf = mem + 1;
            mem[0] = 0;
            memcpy(buf, stream, (size_t) size);
            buf[size] = 0;                                     /* readAscii's strstr ends here */
            size_t most = 2;
            for (long k = 0; k < size; ++k) most += stream[k] == '\n' || stream[k] == 0;
            struct messageBuffer mb;
            memset(&mb, 0, sizeof mb);
            mb.msg = malloc(most * sizeof(struct modesMessage));
            mb.alloc = (int) most;
            harness_line_of = calloc(most, sizeof(uint64_t));
            harness_class = calloc(most, 1);
            harness_line = 0;
            struct client c;
            memset(&c, 0, sizeof c);
            c.service = &service;
            c.buf = buf;
            c.som = buf;
            c.eod = buf + size;
            c.remote = 1;
            memset(&Modes.stats_current, 0, sizeof Modes.stats_current);
            if (readAscii(&c, now, &mb) != 0) { fprintf(stderr, "readAscii closed the client\n"); return 1; }
            if (last) {
                const struct stats *st = &Modes.stats_current;
                const uint64_t head[10] = {(uint64_t) (c.som - buf), harness_line, (uint64_t) mb.len, st->remote_received_modes, st->remote_received_modeac,
                                           st->remote_rejected_unknown_icao, st->remote_rejected_bad, st->remote_accepted[0], st->remote_accepted[1], st->remote_accepted[2]};
                fwrite(head, sizeof head, 1, stdout);
                fwrite(harness_class, 1, (size_t) harness_line, stdout);
                fwrite(harness_line_of, sizeof(uint64_t), (size_t) mb.len, stdout);
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
            free(mb.msg); free(harness_line_of); free(harness_class); free(mem); free(stream);
        }
    }
    return fflush(stdout) ? 1 : 0;
}
