/* cpr_ref_harness.c — runs the REFERENCE's three CPR decoders (cpr.c, linked as the object file oracle/_ref/full/cpr.o that
 * `make -C oracle full` builds) over a file of cases and writes what they return: tests/golden/make_cpr_golden.py,
 * tests/test_cpr_golden.py.  Link with -no-pie (the object is not position independent) and -lm.
 *   cpr_ref_harness <cases.bin> <results.bin>
 * cases.bin: records of struct mgpu_cpr_case (include/modes_gpu.h), results.bin: records of struct mgpu_cpr_result.  The outputs
 * are zeroed before every call: a decoder that fails leaves them alone, so a failing case reads lat = lon = 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int decodeCPRairborne(int even_cprlat, int even_cprlon, int odd_cprlat, int odd_cprlon, int fflag, double *out_lat, double *out_lon);
int decodeCPRsurface(double reflat, double reflon, int even_cprlat, int even_cprlon, int odd_cprlat, int odd_cprlon, int fflag, double *out_lat,
                     double *out_lon);
int decodeCPRrelative(double reflat, double reflon, int cprlat, int cprlon, int fflag, int surface, double *out_lat, double *out_lon);

struct cpr_case {
    double reflat, reflon;
    int32_t even_lat, even_lon, odd_lat, odd_lon;
    uint8_t fn, fflag, surface, pad[5];
};
struct cpr_result {
    double lat, lon;
    int32_t rc, pad;
};

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 1; }
    struct cpr_case c;
    while (fread(&c, sizeof c, 1, in) == 1) {
        struct cpr_result r;
        memset(&r, 0, sizeof r);
        if (c.fn == 0) r.rc = decodeCPRairborne(c.even_lat, c.even_lon, c.odd_lat, c.odd_lon, c.fflag, &r.lat, &r.lon);
        else if (c.fn == 1) r.rc = decodeCPRsurface(c.reflat, c.reflon, c.even_lat, c.even_lon, c.odd_lat, c.odd_lon, c.fflag, &r.lat, &r.lon);
        else r.rc = decodeCPRrelative(c.reflat, c.reflon, c.even_lat, c.even_lon, c.fflag, c.surface, &r.lat, &r.lon);
        if (fwrite(&r, sizeof r, 1, out) != 1) { perror("write"); return 1; }
    }
    fclose(in);
    return fclose(out) ? 1 : 0;
}
