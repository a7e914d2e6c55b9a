/* dump_ref_harness.c — runs the REFERENCE's displayModesMessage (mode_s.c:1809-2239) over a file of case records, its stdout going to
 * a file, and writes the length it printed per case: tests/golden/make_dump_golden.py, tests/test_dump_reference.py (tests/dump_util.py:
 * build_ref_harness / run_ref_harness).  Compile with the flags of `make -C oracle full` and -I<reference>, link against the objects of
 * oracle/_ref/full, readsb.o with its main renamed (objcopy --redefine-sym main=readsb_main).
 *   dump_ref_harness <cases.bin> <out.bin> <lens.bin> <onlyaddr> <raw> <mlat>
 * A case is the message record, the field record and the caller's per-message values (include/modes_gpu.h: struct mgpu_dump_args);
 * the struct modesMessage is a memset-0 one with the records' members under their names.  mm->crc is what decodeModesMessage leaves
 * (mode_s.c:461-466): the reference's modesChecksum of the sliced frame after fixDF17msgtype's change to its first byte.  A case with
 * run == 0 (outside the domain the library prints) is not given to the reference: length 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "readsb.h"

struct case_msg {
    int64_t timestamp, sysTimestamp;
    uint64_t sig_sumsq;
    uint16_t sig_len;
    int16_t score;
    uint8_t phase, correctedbits, msgtype, msgbits;
    uint32_t addr;
    uint8_t msg[14], raw[14];
};
struct case_fields {
    uint32_t addr, AA, flags;
    uint16_t acc_flags;
    uint8_t nav_flags, msgtype, addrtype, source, airground, metype;
    uint8_t mesub, CA, CC, CF, DR, FS, KE, ND, RI, SL, UM, VS, IID, category, emergency, cpr_type;
    uint16_t AC, ID, squawkHex, squawkDec;
    int32_t baro_alt, geom_alt, geom_delta, baro_rate, geom_rate;
    uint16_t ias, tas;
    float heading, gs_v0, gs_v2, gs_selected;
    uint32_t cpr_lat, cpr_lon;
    char callsign[8];
    uint8_t baro_alt_unit, geom_alt_unit, heading_type, sil_type;
    uint8_t nac_p, nac_v, sil, gva, sda, op_version, op_hrd, op_tah;
    uint16_t op_flags;
    uint8_t op_cc_lw, op_cc_antenna_offset, op_cc_tc, nav_heading_type, nav_altitude_source, nav_modes;
    uint32_t nav_fms_altitude, nav_mcp_altitude;
    float nav_qnh, nav_heading, roll, track_rate, mach, oat, humidity, wind_direction;
    uint16_t wind_speed, static_pressure;
    uint8_t commb_format, met_source, turbulence, pad0, reserved[8];
};
struct dump_case {
    struct case_msg m;
    struct case_fields f;
    double lat, lon;
    uint64_t receiver_id;
    uint32_t decoded_rc;
    uint8_t method, has_positions, decoded_nic, run;    /* method: struct mgpu_position's, read iff has_positions */
    int8_t reduce_forward;
    uint8_t pad[7];
};
_Static_assert(sizeof(struct case_msg) == 64, "struct mgpu_msg");
_Static_assert(sizeof(struct case_fields) == 176, "struct mgpu_fields");
_Static_assert(sizeof(struct dump_case) == 280, "case record");

#define F(bit) ((c->f.flags >> (bit)) & 1u)
#define ACC(bit) ((c->f.acc_flags >> (bit)) & 1u)
#define NAV(bit) ((c->f.nav_flags >> (bit)) & 1u)
#define OP(bit) ((c->f.op_flags >> (bit)) & 1u)

int main(int argc, char **argv) {
    if (argc != 7) { fprintf(stderr, "usage: %s cases.bin out.bin lens.bin onlyaddr raw mlat\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror("open"); return 1; }
    fseek(in, 0, SEEK_END);
    const long size = ftell(in);
    fseek(in, 0, SEEK_SET);
    const long n = size / (long) sizeof(struct dump_case);
    struct dump_case *cases = malloc(size ? size : 1);
    if (fread(cases, sizeof(struct dump_case), n, in) != (size_t) n) { perror("read"); return 1; }
    fclose(in);
    FILE *lens_file = fopen(argv[3], "wb");
    if (!lens_file || !freopen(argv[2], "wb", stdout)) { perror("output"); return 1; }

    Modes.onlyaddr = atoi(argv[4]);
    Modes.raw = atoi(argv[5]);
    Modes.mlat = atoi(argv[6]);
    modesChecksumInit(1);

    int32_t *lens = calloc(n ? n : 1, sizeof(int32_t));
    long at = 0;
    for (long k = 0; k < n; ++k) {
        const struct dump_case *c = &cases[k];
        if (!c->run) continue;
        struct modesMessage mm;
        memset(&mm, 0, sizeof mm);
        memcpy(mm.msg, c->m.msg, 14);
        mm.signalLevel = (double) c->m.sig_sumsq / 65535.0 / 65535.0 / (double) c->m.sig_len;
        mm.timestamp = c->m.timestamp;
        mm.sysTimestamp = c->m.sysTimestamp;
        mm.receiverId = c->receiver_id;
        mm.msgtype = c->f.msgtype;
        mm.msgbits = c->m.msgbits;
        mm.score = c->m.score;
        mm.correctedbits = c->m.correctedbits;
        if (mm.msgbits == 56 || mm.msgbits == 112) {
            uint8_t sliced[14];
            memcpy(sliced, c->m.raw, 14);
            if (mm.msgtype == 17 && (sliced[0] >> 3) != 17) sliced[0] = (sliced[0] & 7) | (17 << 3);
            mm.crc = modesChecksum(sliced, mm.msgbits);
        }
        mm.addr = c->f.addr;
        mm.addrtype = c->f.addrtype;
        mm.reduce_forward = c->reduce_forward;
        mm.source = c->f.source;
        mm.IID = c->f.IID; mm.AA = c->f.AA; mm.AC = c->f.AC; mm.CA = c->f.CA; mm.CC = c->f.CC; mm.CF = c->f.CF; mm.DR = c->f.DR;
        mm.FS = c->f.FS; mm.ID = c->f.ID; mm.KE = c->f.KE; mm.ND = c->f.ND; mm.RI = c->f.RI; mm.SL = c->f.SL; mm.UM = c->f.UM; mm.VS = c->f.VS;
        mm.metype = c->f.metype; mm.mesub = c->f.mesub;
        memcpy(mm.MB, c->m.msg + 4, 7); memcpy(mm.ME, c->m.msg + 4, 7); memcpy(mm.MV, c->m.msg + 4, 7); memcpy(mm.MD, c->m.msg + 1, 10);
        mm.baro_alt_valid = F(0); mm.geom_alt_valid = F(1); mm.heading_valid = F(2); mm.gs_valid = F(3); mm.ias_valid = F(4); mm.tas_valid = F(5);
        mm.baro_rate_valid = F(6); mm.geom_rate_valid = F(7); mm.squawk_valid = F(8); mm.callsign_valid = F(9); mm.cpr_valid = F(10); mm.cpr_odd = F(11);
        mm.category_valid = F(12); mm.geom_delta_valid = F(13); mm.spi_valid = F(14); mm.spi = F(15); mm.alert_valid = F(16); mm.alert = F(17);
        mm.emergency_valid = F(18); mm.alt_q_bit = F(19); mm.acas_ra_valid = F(20); mm.roll_valid = F(21); mm.track_rate_valid = F(22); mm.mach_valid = F(23);
        mm.baro_alt = c->f.baro_alt; mm.baro_alt_unit = c->f.baro_alt_unit; mm.geom_alt = c->f.geom_alt; mm.geom_alt_unit = c->f.geom_alt_unit;
        mm.geom_delta = c->f.geom_delta; mm.heading = c->f.heading; mm.heading_type = c->f.heading_type; mm.track_rate = c->f.track_rate; mm.roll = c->f.roll;
        mm.gs.v0 = c->f.gs_v0; mm.gs.v2 = c->f.gs_v2; mm.gs.selected = c->f.gs_selected;
        mm.ias = c->f.ias; mm.tas = c->f.tas; mm.mach = c->f.mach; mm.baro_rate = c->f.baro_rate; mm.geom_rate = c->f.geom_rate;
        memcpy(mm.callsign, c->f.callsign, 8);
        mm.squawkHex = c->f.squawkHex; mm.squawkDec = c->f.squawkDec; mm.category = c->f.category; mm.emergency = c->f.emergency;
        mm.cpr_type = c->f.cpr_type; mm.cpr_lat = c->f.cpr_lat; mm.cpr_lon = c->f.cpr_lon; mm.airground = c->f.airground;
        mm.cpr_decoded = c->has_positions && c->method >= 1 && c->method <= 3; mm.cpr_relative = mm.cpr_decoded && c->method >= 2; mm.decoded_lat = c->lat; mm.decoded_lon = c->lon;
        mm.decoded_nic = c->decoded_nic; mm.decoded_rc = c->decoded_rc;
        mm.commb_format = c->f.commb_format;
        mm.accuracy.nic_a_valid = ACC(0); mm.accuracy.nic_b_valid = ACC(1); mm.accuracy.nic_c_valid = ACC(2); mm.accuracy.nic_baro_valid = ACC(3);
        mm.accuracy.nac_p_valid = ACC(4); mm.accuracy.nac_v_valid = ACC(5); mm.accuracy.gva_valid = ACC(6); mm.accuracy.sda_valid = ACC(7);
        mm.accuracy.nic_a = ACC(8); mm.accuracy.nic_b = ACC(9); mm.accuracy.nic_c = ACC(10); mm.accuracy.nic_baro = ACC(11);
        mm.accuracy.nac_p = c->f.nac_p; mm.accuracy.nac_v = c->f.nac_v; mm.accuracy.sil = c->f.sil; mm.accuracy.gva = c->f.gva; mm.accuracy.sda = c->f.sda;
        mm.accuracy.sil_type = c->f.sil_type;
        mm.opstatus.tah = c->f.op_tah; mm.opstatus.hrd = c->f.op_hrd; mm.opstatus.cc_lw = c->f.op_cc_lw; mm.opstatus.cc_antenna_offset = c->f.op_cc_antenna_offset;
        mm.opstatus.valid = OP(0); mm.opstatus.version = c->f.op_version; mm.opstatus.om_acas_ra = OP(1); mm.opstatus.om_ident = OP(2); mm.opstatus.om_atc = OP(3);
        mm.opstatus.om_saf = OP(4); mm.opstatus.cc_acas = OP(5); mm.opstatus.cc_cdti = OP(6); mm.opstatus.cc_1090_in = OP(7); mm.opstatus.cc_arv = OP(8);
        mm.opstatus.cc_ts = OP(9); mm.opstatus.cc_tc = c->f.op_cc_tc; mm.opstatus.cc_uat_in = OP(10); mm.opstatus.cc_poa = OP(11); mm.opstatus.cc_b2_low = OP(12);
        mm.opstatus.cc_lw_valid = OP(13);
        mm.nav.fms_altitude = c->f.nav_fms_altitude; mm.nav.mcp_altitude = c->f.nav_mcp_altitude; mm.nav.qnh = c->f.nav_qnh; mm.nav.heading = c->f.nav_heading;
        mm.nav.heading_valid = NAV(0); mm.nav.fms_altitude_valid = NAV(1); mm.nav.mcp_altitude_valid = NAV(2); mm.nav.qnh_valid = NAV(3); mm.nav.modes_valid = NAV(4);
        mm.nav.heading_type = c->f.nav_heading_type; mm.nav.altitude_source = c->f.nav_altitude_source; mm.nav.modes = c->f.nav_modes;
        displayModesMessage(&mm);
        fflush(stdout);
        const long now = ftell(stdout);
        lens[k] = (int32_t) (now - at);
        at = now;
    }
    fwrite(lens, sizeof(int32_t), n, lens_file);
    return fclose(lens_file) || fflush(stdout) ? 1 : 0;
}
