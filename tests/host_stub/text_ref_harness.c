/* text_ref_harness.c — runs the REFERENCE's two text writers, modesSendSBSOutput (net_io.c:3184-3404) and modesSendRawOutput
 * (net_io.c:1837-1863), over a file of case records and writes what they wrote: tests/golden/make_text_golden.py,
 * tests/test_text_reference.py (tests/sbs_util.py: build_ref_harness / run_ref_harness).  Both writers are static, so the reference's
 * net_io.c is INCLUDED here (compile with the flags of `make -C oracle full` and -I<reference>) and the program is linked against the
 * other objects of oracle/_ref/full, readsb.o with its main renamed (objcopy --redefine-sym main=readsb_main).
 *   text_ref_harness <cases.bin> <now_ms> <use_gnss> <override_squawk> <mlat> <verbatim>
 * stdout: one int32 length per case, then the bytes of all lines.
 * The clock the SBS writer reads per message is replaced by <now_ms>.  Nothing flushes: the writers' buffers are local, with one
 * pretended connection each and a flush size no line reaches. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static int64_t harness_now_ms;
static int harness_clock_gettime(clockid_t id, struct timespec *ts) {
    (void) id;
    ts->tv_sec = (time_t) (harness_now_ms / 1000);
    ts->tv_nsec = (long) (harness_now_ms % 1000) * 1000000L;
    return 0;
}
#define clock_gettime harness_clock_gettime
#include "net_io.c"
#undef clock_gettime

/* struct mgpu_fields (include/modes_gpu.h): the members the SBS line reads, at their offsets */
struct case_fields {
    uint32_t addr, AA, flags;
    uint16_t acc_flags;
    uint8_t nav_flags, msgtype, addrtype, source, airground, metype;
    uint8_t skip0[16];
    uint16_t AC, ID, squawkHex, squawkDec;
    int32_t baro_alt, geom_alt, geom_delta, baro_rate, geom_rate;
    uint16_t ias, tas;
    float heading, gs_v0, gs_v2, gs_selected;
    uint32_t cpr_lat, cpr_lon;
    char callsign[8];
    uint8_t baro_alt_unit, geom_alt_unit, heading_type, sil_type;
    uint8_t rest[72];
};
struct text_case {
    int64_t sysTimestamp, timestamp;
    double lat, lon;
    int32_t geom_delta, msgbits;
    uint8_t has_pos, delta_valid, kind, pad[5];
    uint8_t msg[14], raw[14], pad2[4];
    struct case_fields f;
};
_Static_assert(sizeof(struct case_fields) == 176, "struct mgpu_fields");
_Static_assert(sizeof(struct text_case) == 256, "case record");

#define F(bit) ((c->f.flags >> (bit)) & 1u)

int main(int argc, char **argv) {
    if (argc != 7) { fprintf(stderr, "usage: %s cases.bin now_ms use_gnss override_squawk mlat verbatim\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror("open"); return 1; }
    fseek(in, 0, SEEK_END);
    const long size = ftell(in);
    fseek(in, 0, SEEK_SET);
    const long n = size / (long) sizeof(struct text_case);
    struct text_case *cases = malloc(size ? size : 1);
    if (fread(cases, sizeof(struct text_case), n, in) != (size_t) n) { perror("read"); return 1; }
    fclose(in);

    harness_now_ms = atoll(argv[2]);
    Modes.use_gnss = atoi(argv[3]);
    Modes.sbsOverrideSquawk = atoi(argv[4]);
    Modes.mlat = atoi(argv[5]);
    Modes.net_verbatim = atoi(argv[6]);
    Modes.net_output_flush_size = 1 << 30;

    static char sbs_buf[4096], raw_buf[4096];
    struct net_writer sbs;
    memset(&sbs, 0, sizeof sbs);
    sbs.data = sbs_buf;
    sbs.connections = 1;
    memset(&Modes.raw_out, 0, sizeof Modes.raw_out);
    Modes.raw_out.data = raw_buf;
    Modes.raw_out.connections = 1;

    int32_t *lens = calloc(n ? n : 1, sizeof(int32_t));
    char *all = malloc((size_t) n * 256 + 1);
    size_t used = 0;
    for (long k = 0; k < n; ++k) {
        const struct text_case *c = &cases[k];
        struct modesMessage mm;
        struct aircraft a;
        memset(&mm, 0, sizeof mm);
        memset(&a, 0, sizeof a);
        struct net_writer *w;
        if (c->kind == 0) {
            mm.addr = c->f.addr;
            mm.msgtype = c->f.msgtype;
            mm.metype = c->f.metype;
            mm.sysTimestamp = c->sysTimestamp;
            mm.callsign_valid = F(9);
            memcpy(mm.callsign, c->f.callsign, 8);
            mm.baro_alt_valid = F(0); mm.baro_alt = c->f.baro_alt;
            mm.geom_alt_valid = F(1); mm.geom_alt = c->f.geom_alt;
            mm.gs_valid = F(3); mm.gs.selected = c->f.gs_selected;
            mm.heading_valid = F(2); mm.heading = c->f.heading; mm.heading_type = c->f.heading_type;
            mm.cpr_decoded = c->has_pos; mm.decoded_lat = c->lat; mm.decoded_lon = c->lon;
            mm.baro_rate_valid = F(6); mm.baro_rate = c->f.baro_rate;
            mm.geom_rate_valid = F(7); mm.geom_rate = c->f.geom_rate;
            mm.squawk_valid = F(8); mm.squawkDec = c->f.squawkDec; mm.squawkHex = c->f.squawkHex;
            mm.alert_valid = F(16); mm.alert = F(17);
            mm.spi_valid = F(14); mm.spi = F(15);
            mm.airground = c->f.airground;
            a.geom_delta = c->geom_delta;
            a.geom_delta_valid.source = c->delta_valid ? SOURCE_ADSB : SOURCE_INVALID;
            w = &sbs;
            w->dataUsed = 0;
            modesSendSBSOutput(&mm, &a, w);
        } else {
            mm.msgbits = c->msgbits;
            mm.timestamp = c->timestamp;
            memcpy(mm.msg, c->msg, 14);
            memcpy(mm.verbatim, c->raw, 14);
            w = &Modes.raw_out;
            w->dataUsed = 0;
            modesSendRawOutput(&mm);
        }
        lens[k] = (int32_t) w->dataUsed;
        memcpy(all + used, w->data, w->dataUsed);
        used += w->dataUsed;
    }
    fwrite(lens, sizeof(int32_t), n, stdout);
    fwrite(all, 1, used, stdout);
    return fflush(stdout) ? 1 : 0;
}
