/* asterix_in_ref_harness.c — runs the REFERENCE's ASTERIX input, readAsterix (net_io.c:4643-4659) with decodeAsterixMessage
 * (net_io.c:1922-2407) as the service's read handler, over a byte stream and writes the members it leaves in every message:
 * tests/golden/make_asterix_in_golden.py, tests/test_asterix_in_reference.py, tools/bench_asterix_in.py (tests/asterix_in_util.py:
 * build_ref_harness / run_ref_harness).  The functions are static, so the reference's net_io.c is INCLUDED here (compile with the flags
 * of `make -C oracle full` and -I<reference>) and the program is linked against the other objects of oracle/_ref/full, readsb.o with
 * its main renamed (objcopy --redefine-sym main=readsb_main).
 *   asterix_in_ref_harness <stream.bin> <source: datasource_t 0 .. 11> <now_ms> [reps]
 * stdout: uint64 consumed, frames, records, frames of another category, stop (0 end, 2 the client was closed); then per record a
 * uint64 frame index; then per record a struct mgpu_asterix_rec (include/modes_gpu.h), filled member by member from the modesMessage.
 * The stream lies in a buffer with 4096 zero bytes behind it: the decoder is not bounded by a record's length.  readAsterix knows no
 * incomplete record (it decodes what its buffer holds), so it is given the stream up to the first place where fewer than 3 bytes are
 * left or the length, computed with ITS expression on ITS char, reaches past the end; that place is `consumed`.  A length of 0 never
 * ends its loop and a chain of 192 extension bytes or more runs off readFspec's allocation: such streams must not be given to this
 * program.  The clocks — mstime() — answer <now_ms>: Modes.synthetic_now, and time, gettimeofday and clock_gettime are defined here
 * for every object this is linked from.  The -1 path runs modesCloseClient on this program's client: it needs a service and no more.
 * The message buffer is large enough never to drain.  reps > 1: the stream is run that many times (for timing). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <time.h>

static int64_t harness_now_ms;
time_t time(time_t *t) {
    const time_t s = (time_t) (harness_now_ms / 1000);
    if (t) *t = s;
    return s;
}
int gettimeofday(struct timeval *restrict tv, void *restrict tz) {
    (void) tz;
    tv->tv_sec = (time_t) (harness_now_ms / 1000);
    tv->tv_usec = (suseconds_t) (harness_now_ms % 1000) * 1000;
    return 0;
}
int clock_gettime(clockid_t id, struct timespec *ts) {
    (void) id;
    ts->tv_sec = (time_t) (harness_now_ms / 1000);
    ts->tv_nsec = (long) (harness_now_ms % 1000) * 1000000L;
    return 0;
}

#include "net_io.c"

#define MGPU_NO_DEFAULTS_MACRO
#include "modes_gpu.h"

static uint64_t harness_frame, harness_other, *harness_frame_of;

static int harness_read(struct client *c, char *p, int remote, int64_t now, struct messageBuffer *mb) {
    const int before = mb->len;
    if (*p != 21) ++harness_other;
    const int rc = decodeAsterixMessage(c, p, remote, now, mb);
    if (mb->len != before) harness_frame_of[before] = harness_frame;
    ++harness_frame;
    return rc;
}

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s stream.bin source now_ms [reps]\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror("open"); return 1; }
    fseek(in, 0, SEEK_END);
    const long size = ftell(in);
    fseek(in, 0, SEEK_SET);
    char *buf = calloc((size_t) size + 4096, 1);
    if (fread(buf, 1, (size_t) size, in) != (size_t) size) { perror("read"); return 1; }
    fclose(in);
    const int source = atoi(argv[2]);
    harness_now_ms = atoll(argv[3]);
    Modes.synthetic_now = harness_now_ms;
    const int reps = argc > 4 ? atoi(argv[4]) : 1;
    if (source < 0 || source > SOURCE_PRIO) { fprintf(stderr, "source\n"); return 2; }

    /* the complete records, by readAsterix's own expression (:4647) */
    long end = 0;
    size_t most = 2;
    while (size - end >= 3) {
        const char *p = buf + end;
        const uint16_t msgLen = (*(p + 1) << 8) + *(p + 2);
        if (msgLen == 0) { fprintf(stderr, "a record of length 0: the reference would not return\n"); return 2; }
        if (end + msgLen > size) break;
        end += msgLen;
        ++most;
    }

    struct messageBuffer mb;
    memset(&mb, 0, sizeof mb);
    mb.msg = malloc(most * sizeof(struct modesMessage));
    mb.alloc = (int) most;
    harness_frame_of = calloc(most, sizeof(uint64_t));

    struct net_service service;
    struct client c;
    uint64_t consumed = 0, stop = 0;
    for (int rep = 0; rep < reps; ++rep) {
        memset(&service, 0, sizeof service);
        service.descr = "asterix in";
        service.read_handler = harness_read;
        memset(&c, 0, sizeof c);
        c.service = &service;
        c.fd = -1;
        c.buf = buf;
        c.som = buf;
        c.eod = buf + end;
        c.remote = 64 + source;                            /* mm->source = remote - 64 (:1929) */
        mb.len = 0;
        harness_frame = 0;
        harness_other = 0;
        stop = readAsterix(&c, harness_now_ms, &mb) != 0 ? 2 : 0;
        consumed = (uint64_t) (c.som - buf);
        if (!stop && consumed != (uint64_t) end) { fprintf(stderr, "readAsterix ended at %llu, not at %ld\n", (unsigned long long) consumed, end); return 1; }
    }

    const uint64_t head[5] = {consumed, harness_frame, (uint64_t) mb.len, harness_other, stop};
    fwrite(head, sizeof head, 1, stdout);
    fwrite(harness_frame_of, sizeof(uint64_t), (size_t) mb.len, stdout);
    for (int k = 0; k < mb.len; ++k) {
        const struct modesMessage *mm = &mb.msg[k];
        struct mgpu_asterix_rec r;
        memset(&r, 0, sizeof r);
        r.sysTimestamp = mm->sysTimestamp;
        r.decoded_lat = mm->decoded_lat;
        r.decoded_lon = mm->decoded_lon;
        r.mach = mm->mach;
        r.addr = mm->addr;
        r.flags = (mm->baro_alt_valid ? MGPU_F_BARO_ALT_VALID : 0) | (mm->geom_alt_valid ? MGPU_F_GEOM_ALT_VALID : 0) | (mm->heading_valid ? MGPU_F_HEADING_VALID : 0) |
                  (mm->gs_valid ? MGPU_F_GS_VALID : 0) | (mm->ias_valid ? MGPU_F_IAS_VALID : 0) | (mm->tas_valid ? MGPU_F_TAS_VALID : 0) |
                  (mm->baro_rate_valid ? MGPU_F_BARO_RATE_VALID : 0) | (mm->geom_rate_valid ? MGPU_F_GEOM_RATE_VALID : 0) | (mm->squawk_valid ? MGPU_F_SQUAWK_VALID : 0) |
                  (mm->callsign_valid ? MGPU_F_CALLSIGN_VALID : 0) | (mm->category_valid ? MGPU_F_CATEGORY_VALID : 0) | (mm->spi_valid ? MGPU_F_SPI_VALID : 0) |
                  (mm->spi ? MGPU_F_SPI : 0) | (mm->alert_valid ? MGPU_F_ALERT_VALID : 0) | (mm->alert ? MGPU_F_ALERT : 0) |
                  (mm->emergency_valid ? MGPU_F_EMERGENCY_VALID : 0) | (mm->alt_q_bit ? MGPU_F_ALT_Q_BIT : 0) | (mm->roll_valid ? MGPU_F_ROLL_VALID : 0) |
                  (mm->mach_valid ? MGPU_F_MACH_VALID : 0);
        r.ast_flags = (mm->sbs_pos_valid ? MGPU_AST_POS_VALID : 0) | (mm->accuracy.nac_v_valid ? MGPU_AST_NAC_V_VALID : 0) |
                      (mm->accuracy.nac_p_valid ? MGPU_AST_NAC_P_VALID : 0) | (mm->accuracy.gva_valid ? MGPU_AST_GVA_VALID : 0) |
                      (mm->accuracy.sda_valid ? MGPU_AST_SDA_VALID : 0) | (mm->accuracy.nic_baro_valid ? MGPU_AST_NIC_BARO_VALID : 0) |
                      (mm->opstatus.valid ? MGPU_AST_OPSTATUS_VALID : 0) | (mm->nav.modes_valid ? MGPU_AST_NAV_MODES_VALID : 0) |
                      (mm->nav.mcp_altitude_valid ? MGPU_AST_MCP_ALT_VALID : 0) | (mm->nav.fms_altitude_valid ? MGPU_AST_FMS_ALT_VALID : 0);
        r.baro_alt = mm->baro_alt;
        r.geom_alt = mm->geom_alt;
        r.baro_rate = mm->baro_rate;
        r.geom_rate = mm->geom_rate;
        r.ias = mm->ias;
        r.tas = mm->tas;
        r.squawkHex = mm->squawkHex;
        r.squawkDec = mm->squawkDec;
        r.category = mm->category;
        r.mcp_altitude = mm->nav.mcp_altitude;
        r.fms_altitude = mm->nav.fms_altitude;
        r.gs_v0 = mm->gs.v0;
        r.heading = mm->heading;
        r.roll = mm->roll;
        memcpy(r.callsign, mm->callsign, 8);
        r.source = (uint8_t) mm->source;
        r.addrtype = (uint8_t) mm->addrtype;
        r.airground = (uint8_t) mm->airground;
        r.emergency = (uint8_t) mm->emergency;
        r.nav_modes = (uint8_t) mm->nav.modes;
        r.nac_v = (uint8_t) mm->accuracy.nac_v;
        r.nac_p = (uint8_t) mm->accuracy.nac_p;
        r.sil = (uint8_t) mm->accuracy.sil;
        r.sil_type = (uint8_t) mm->accuracy.sil_type;
        r.gva = (uint8_t) mm->accuracy.gva;
        r.sda = (uint8_t) mm->accuracy.sda;
        r.nic_baro = (uint8_t) mm->accuracy.nic_baro;
        r.op_version = (uint8_t) mm->opstatus.version;
        r.heading_type = (uint8_t) mm->heading_type;
        r.baro_alt_unit = (uint8_t) mm->baro_alt_unit;
        r.geom_alt_unit = (uint8_t) mm->geom_alt_unit;
        fwrite(&r, sizeof r, 1, stdout);
    }
    return fflush(stdout) ? 1 : 0;
}
