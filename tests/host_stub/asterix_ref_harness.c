/* asterix_ref_harness.c — runs the REFERENCE's ASTERIX CAT021 writer, modesSendAsterixOutput (net_io.c:2416-2945), over a file of case
 * records and writes what it wrote: tests/golden/make_asterix_golden.py, tests/test_asterix_reference.py (tests/asterix_util.py:
 * build_ref_harness / run_ref_harness).  The writer is static, so the reference's net_io.c is INCLUDED here (compile with the flags of
 * `make -C oracle full`, -I<reference> and -I<this repository>/include) and the program is linked against the other objects of
 * oracle/_ref/full, readsb.o with its main renamed (objcopy --redefine-sym main=readsb_main).
 *   asterix_ref_harness <cases.bin> <now_ms> <remote>
 * stdout: one int32 length per case, then the bytes of all records.
 * The clocks the writer reads per message — mstime() and time(NULL) — answer <now_ms>: this program defines time, gettimeofday and
 * clock_gettime itself, for every object it is linked from.  The aircraft the writer looks up (aircraftGet / aircraftCreate) is one
 * struct aircraft filled from the case.  Nothing flushes: the writer's buffer is local, with one pretended connection and a flush
 * size no record reaches. */
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

struct aircraft;
static struct aircraft *harness_aircraft(uint32_t addr);
#define aircraftGet harness_aircraft
#define aircraftCreate harness_aircraft
#include "net_io.c"
#undef aircraftGet
#undef aircraftCreate

#define MGPU_NO_DEFAULTS_MACRO
#include "modes_gpu.h"

static struct aircraft the_aircraft;
static struct aircraft *harness_aircraft(uint32_t addr) { (void) addr; return &the_aircraft; }

struct asterix_case {
    int64_t sysTimestamp;
    double lat, lon;
    uint64_t id;
    int32_t ac_baro_alt;
    uint8_t has_pos, ac_category, pad[2];
    struct mgpu_fields f;
};
_Static_assert(sizeof(struct mgpu_fields) == 176, "struct mgpu_fields");
_Static_assert(sizeof(struct asterix_case) == 216, "case record");

#define F(bit) ((c->f.flags & (bit)) != 0)
#define ACC(bit) ((c->f.acc_flags & (bit)) != 0)
#define NAV(bit) ((c->f.nav_flags & (bit)) != 0)
#define OP(bit) ((c->f.op_flags & (bit)) != 0)

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s cases.bin now_ms remote\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror("open"); return 1; }
    fseek(in, 0, SEEK_END);
    const long size = ftell(in);
    fseek(in, 0, SEEK_SET);
    const long n = size / (long) sizeof(struct asterix_case);
    struct asterix_case *cases = malloc(size ? size : 1);
    if (fread(cases, sizeof(struct asterix_case), n, in) != (size_t) n) { perror("read"); return 1; }
    fclose(in);

    harness_now_ms = atoll(argv[2]);
    const int remote = atoi(argv[3]);
    Modes.synthetic_now = 0;
    Modes.net_output_flush_size = 4096;          /* the writer's scratch is a VLA of twice this */

    static char buf[16384];
    struct net_writer w;
    memset(&w, 0, sizeof w);
    w.data = buf;
    w.connections = 1;

    int32_t *lens = calloc(n ? n : 1, sizeof(int32_t));
    char *all = malloc((size_t) n * 128 + 1);
    size_t used = 0;
    for (long k = 0; k < n; ++k) {
        const struct asterix_case *c = &cases[k];
        struct modesMessage mm;
        memset(&mm, 0, sizeof mm);
        memset(&the_aircraft, 0, sizeof the_aircraft);
        the_aircraft.baro_alt = c->ac_baro_alt;
        the_aircraft.category = c->ac_category;

        mm.remote = remote;
        mm.sysTimestamp = c->sysTimestamp;
        mm.receiverId = c->id;
        mm.addr = c->f.addr; mm.addrtype = c->f.addrtype; mm.source = c->f.source; mm.airground = c->f.airground;
        mm.alt_q_bit = F(MGPU_F_ALT_Q_BIT);
        mm.cpr_decoded = c->has_pos; mm.decoded_lat = c->lat; mm.decoded_lon = c->lon;
        mm.ias_valid = F(MGPU_F_IAS_VALID); mm.ias = c->f.ias;
        mm.mach_valid = F(MGPU_F_MACH_VALID); mm.mach = c->f.mach;
        mm.tas_valid = F(MGPU_F_TAS_VALID); mm.tas = c->f.tas;
        mm.gs_valid = F(MGPU_F_GS_VALID); mm.gs.v0 = c->f.gs_v0; mm.gs.v2 = c->f.gs_v2; mm.gs.selected = c->f.gs_selected;
        mm.heading_valid = F(MGPU_F_HEADING_VALID); mm.heading = c->f.heading; mm.heading_type = c->f.heading_type;
        mm.geom_alt_valid = F(MGPU_F_GEOM_ALT_VALID); mm.geom_alt = c->f.geom_alt; mm.geom_alt_unit = c->f.geom_alt_unit;
        mm.geom_delta_valid = F(MGPU_F_GEOM_DELTA_VALID); mm.geom_delta = c->f.geom_delta;
        mm.accuracy.nac_v_valid = ACC(MGPU_ACC_NAC_V_VALID); mm.accuracy.nac_v = c->f.nac_v;
        mm.accuracy.nic_baro_valid = ACC(MGPU_ACC_NIC_BARO_VALID); mm.accuracy.nic_baro = ACC(MGPU_ACC_NIC_BARO);
        mm.accuracy.sil_type = c->f.sil_type; mm.accuracy.sil = c->f.sil;
        mm.accuracy.nac_p_valid = ACC(MGPU_ACC_NAC_P_VALID); mm.accuracy.nac_p = c->f.nac_p;
        mm.accuracy.sda_valid = ACC(MGPU_ACC_SDA_VALID); mm.accuracy.sda = c->f.sda;
        mm.accuracy.gva_valid = ACC(MGPU_ACC_GVA_VALID); mm.accuracy.gva = c->f.gva;
        mm.opstatus.valid = OP(MGPU_OP_VALID); mm.opstatus.version = c->f.op_version;
        mm.opstatus.om_acas_ra = OP(MGPU_OP_OM_ACAS_RA); mm.opstatus.cc_tc = c->f.op_cc_tc; mm.opstatus.cc_ts = OP(MGPU_OP_CC_TS);
        mm.opstatus.cc_arv = OP(MGPU_OP_CC_ARV); mm.opstatus.cc_cdti = OP(MGPU_OP_CC_CDTI); mm.opstatus.cc_acas = OP(MGPU_OP_CC_ACAS);
        mm.squawk_valid = F(MGPU_F_SQUAWK_VALID); mm.squawkHex = c->f.squawkHex; mm.squawkDec = c->f.squawkDec;
        mm.roll_valid = F(MGPU_F_ROLL_VALID); mm.roll = c->f.roll;
        mm.baro_alt_valid = F(MGPU_F_BARO_ALT_VALID); mm.baro_alt = c->f.baro_alt; mm.baro_alt_unit = c->f.baro_alt_unit;
        mm.spi_valid = F(MGPU_F_SPI_VALID); mm.spi = F(MGPU_F_SPI);
        mm.alert_valid = F(MGPU_F_ALERT_VALID); mm.alert = F(MGPU_F_ALERT);
        mm.emergency_valid = F(MGPU_F_EMERGENCY_VALID); mm.emergency = c->f.emergency;
        mm.nav.modes_valid = NAV(MGPU_NAV_MODES_VALID); mm.nav.modes = c->f.nav_modes;
        mm.baro_rate_valid = F(MGPU_F_BARO_RATE_VALID); mm.baro_rate = c->f.baro_rate;
        mm.geom_rate_valid = F(MGPU_F_GEOM_RATE_VALID); mm.geom_rate = c->f.geom_rate;
        mm.callsign_valid = F(MGPU_F_CALLSIGN_VALID); memcpy(mm.callsign, c->f.callsign, 8);
        mm.category_valid = F(MGPU_F_CATEGORY_VALID); mm.category = c->f.category;
        mm.wind_valid = F(MGPU_F_WIND_VALID); mm.wind_speed = c->f.wind_speed; mm.wind_direction = c->f.wind_direction;
        mm.oat_valid = F(MGPU_F_OAT_VALID); mm.oat = c->f.oat;
        mm.turbulence_valid = F(MGPU_F_TURBULENCE_VALID); mm.static_pressure_valid = F(MGPU_F_STATIC_PRESSURE_VALID);
        mm.humidity_valid = F(MGPU_F_HUMIDITY_VALID);
        mm.nav.fms_altitude_valid = NAV(MGPU_NAV_FMS_ALT_VALID); mm.nav.fms_altitude = c->f.nav_fms_altitude;
        mm.nav.mcp_altitude_valid = NAV(MGPU_NAV_MCP_ALT_VALID); mm.nav.mcp_altitude = c->f.nav_mcp_altitude;

        w.dataUsed = 0;
        modesSendAsterixOutput(&mm, &w);
        lens[k] = (int32_t) w.dataUsed;
        memcpy(all + used, w.data, w.dataUsed);
        used += w.dataUsed;
    }
    fwrite(lens, sizeof(int32_t), n, stdout);
    fwrite(all, 1, used, stdout);
    return fflush(stdout) ? 1 : 0;
}
