/* sbs_in_ref_harness.c — runs the REFERENCE's SBS input, readAscii (net_io.c:4599-4641) with decodeSbsLine (net_io.c:2952-3178) or its
 * Mlat / Jaero / Prio wrappers (:81-92) as the service's read handler, over a byte stream and writes the members it leaves in every
 * message: tests/golden/make_sbs_in_golden.py, tests/test_sbs_in_reference.py, tools/bench_sbs_in.py (tests/sbs_in_util.py:
 * build_ref_harness / run_ref_harness).  The functions are static, so the reference's net_io.c is INCLUDED here (compile with the flags
 * of `make -C oracle full` and -I<reference>) and the program is linked against the other objects of oracle/_ref/full, readsb.o with
 * its main renamed (objcopy --redefine-sym main=readsb_main).
 *   sbs_in_ref_harness <stream.bin> <source: 3 sbs | 4 mlat | 6 jaero | 11 prio> <now_ms> [reps]
 * stdout: uint64 consumed, lines, records, invalid (the reference's counter), valid (its counter); then per record a uint64 line index;
 * then per record a struct mgpu_sbs_rec (include/modes_gpu.h), filled member by member from the modesMessage.
 * The message buffer is large enough never to drain.  reps > 1: the stream is run that many times (for timing; the output is the last
 * run's). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "net_io.c"

#include "modes_gpu.h"

static read_fn harness_handler;
static uint64_t harness_line, *harness_line_of;

static int harness_read(struct client *c, char *line, int remote, int64_t now, struct messageBuffer *mb) {
    const int before = mb->len;
    const int rc = harness_handler(c, line, remote, now, mb);
    if (mb->len != before) harness_line_of[before] = harness_line;
    ++harness_line;
    return rc;
}

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s stream.bin source now_ms [reps]\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror("open"); return 1; }
    fseek(in, 0, SEEK_END);
    const long size = ftell(in);
    fseek(in, 0, SEEK_SET);
    char *stream = malloc((size_t) size + 1), *buf = malloc((size_t) size + 1);
    if (fread(stream, 1, (size_t) size, in) != (size_t) size) { perror("read"); return 1; }
    fclose(in);
    const int source = atoi(argv[2]);
    const int64_t now = atoll(argv[3]);
    const int reps = argc > 4 ? atoi(argv[4]) : 1;

    size_t most = 2;
    for (long k = 0; k < size; ++k) most += stream[k] == '\n' || stream[k] == 0;
    struct messageBuffer mb;
    memset(&mb, 0, sizeof mb);
    mb.msg = malloc(most * sizeof(struct modesMessage));
    mb.alloc = (int) most;
    harness_line_of = calloc(most, sizeof(uint64_t));

    struct net_service service;
    memset(&service, 0, sizeof service);
    service.descr = "sbs in";
    service.read_sep = "\n";
    service.read_sep_len = 1;
    service.read_handler = harness_read;
    service.read_mode = READ_MODE_ASCII;
    harness_handler = source == SOURCE_MLAT ? decodeSbsLineMlat : source == SOURCE_JAERO ? decodeSbsLineJaero : source == SOURCE_PRIO ? decodeSbsLinePrio : decodeSbsLine;
    if (source != SOURCE_SBS && source != SOURCE_MLAT && source != SOURCE_JAERO && source != SOURCE_PRIO) { fprintf(stderr, "source\n"); return 2; }

    struct client c;
    uint64_t consumed = 0;
    for (int rep = 0; rep < reps; ++rep) {
        memcpy(buf, stream, (size_t) size);
        buf[size] = 0;                                     /* readAscii's strstr ends here */
        memset(&c, 0, sizeof c);
        c.service = &service;
        c.buf = buf;
        c.som = buf;
        c.eod = buf + size;
        c.remote = 0;                                      /* below 64: decodeSbsLine's own SOURCE_SBS; the wrappers pass theirs */
        mb.len = 0;
        harness_line = 0;
        Modes.stats_current.remote_received_basestation_valid = 0;
        Modes.stats_current.remote_received_basestation_invalid = 0;
        if (readAscii(&c, now, &mb) != 0) { fprintf(stderr, "readAscii closed the client\n"); return 1; }
        consumed = (uint64_t) (c.som - buf);
    }

    const uint64_t head[5] = {consumed, harness_line, (uint64_t) mb.len, Modes.stats_current.remote_received_basestation_invalid,
                              Modes.stats_current.remote_received_basestation_valid};
    fwrite(head, sizeof head, 1, stdout);
    fwrite(harness_line_of, sizeof(uint64_t), (size_t) mb.len, stdout);
    for (int k = 0; k < mb.len; ++k) {
        const struct modesMessage *mm = &mb.msg[k];
        struct mgpu_sbs_rec r;
        memset(&r, 0, sizeof r);
        r.sysTimestamp = mm->sysTimestamp;
        r.decoded_lat = mm->decoded_lat;
        r.decoded_lon = mm->decoded_lon;
        r.addr = mm->addr;
        r.flags = (mm->baro_alt_valid ? MGPU_F_BARO_ALT_VALID : 0) | (mm->gs_valid ? MGPU_F_GS_VALID : 0) | (mm->heading_valid ? MGPU_F_HEADING_VALID : 0) |
                  (mm->baro_rate_valid ? MGPU_F_BARO_RATE_VALID : 0) | (mm->squawk_valid ? MGPU_F_SQUAWK_VALID : 0) | (mm->callsign_valid ? MGPU_F_CALLSIGN_VALID : 0) |
                  (mm->spi_valid ? MGPU_F_SPI_VALID : 0) | (mm->spi ? MGPU_F_SPI : 0) | (mm->alert_valid ? MGPU_F_ALERT_VALID : 0) | (mm->alert ? MGPU_F_ALERT : 0);
        r.sbs_flags = (mm->sbs_pos_valid ? MGPU_SBS_POS_VALID : 0) | (mm->squawk_emergency_valid ? MGPU_SBS_EMERGENCY_VALID : 0) |
                      (mm->squawk_emergency ? MGPU_SBS_EMERGENCY : 0);
        r.baro_alt = mm->baro_alt;
        r.baro_rate = mm->baro_rate;
        r.gs_v0 = mm->gs.v0;
        r.heading = mm->heading;
        r.squawkDec = mm->squawkDec;
        r.squawkHex = mm->squawkHex;
        r.receiverCountMlat = mm->receiverCountMlat;
        r.mlatEPU = mm->mlatEPU;
        memcpy(r.callsign, mm->callsign, 8);
        r.sbsMsgType = (uint8_t) mm->sbsMsgType;
        r.source = (uint8_t) mm->source;
        r.addrtype = (uint8_t) mm->addrtype;
        r.airground = (uint8_t) mm->airground;
        r.baro_alt_unit = (uint8_t) mm->baro_alt_unit;
        r.heading_type = (uint8_t) mm->heading_type;
        fwrite(&r, sizeof r, 1, stdout);
    }
    return fflush(stdout) ? 1 : 0;
}
