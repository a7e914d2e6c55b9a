// uat_ref_harness.c — the reference's own uat2esnt (oracle/_ref/full/uat2esnt_uat2esnt.o, uat2esnt_uat_decode.o: `make -C oracle full`)
// over a stream of lines, for tests/golden/make_uat_golden.py, tests/test_uat_reference.py and tools/bench_uat.py.
//   uat_ref_harness <stream.bin> <out.bin> <lens.bin> [repeat]
// The stream is cut at '\n' as readClient cuts a client's buffer (the '\n' becomes a NUL; bytes behind the last one are left), each
// line goes through uat2esnt_convert_message as decodeUatMessage calls it (net_io.c:4337-4343: end = msg + strlen(msg), 512 bytes of
// output), and what it printed is appended to out.bin, its length (int32) to lens.bin.  With `repeat` the conversion of the whole
// stream runs that many times and only the time per pass is printed: "seconds <s> lines <n>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

void uat2esnt_initCrcTables(void);
void uat2esnt_convert_message(char *p, char *end, char *out, char *out_end);

int main(int argc, char **argv) {
    if (argc != 4 && argc != 5) { fprintf(stderr, "usage: %s stream.bin out.bin lens.bin [repeat]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    char *buf = malloc((size_t) size + 1);
    if (!buf || fread(buf, 1, (size_t) size, f) != (size_t) size) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    fclose(f);
    buf[size] = 0;
    const int repeat = argc == 5 ? atoi(argv[4]) : 0;
    uat2esnt_initCrcTables();

    // the lines: '\n' -> NUL once, so that the timed passes do what the reference does per message and no more
    size_t nlines = 0;
    for (long k = 0; k < size; ++k) nlines += buf[k] == '\n';
    char **starts = malloc((nlines + 1) * sizeof *starts);
    if (!starts) return 1;
    {
        size_t n = 0;
        long start = 0;
        for (long k = 0; k < size; ++k)
            if (buf[k] == '\n') { buf[k] = 0; starts[n++] = buf + start; start = k + 1; }
    }

    char output[512];
    if (repeat > 0) {
        struct timespec t0, t1;
        size_t sink = 0;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (int r = 0; r < repeat; ++r)
            for (size_t k = 0; k < nlines; ++k) {
                char *msg = starts[k];
                uat2esnt_convert_message(msg, msg + strlen(msg), output, output + sizeof output);
                sink += (unsigned char) output[0];
            }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        printf("seconds %.6f lines %zu sink %zu\n", ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec)) / repeat, nlines, sink);
        return 0;
    }
    FILE *fo = fopen(argv[2], "wb"), *fl = fopen(argv[3], "wb");
    if (!fo || !fl) { perror("output"); return 1; }
    for (size_t k = 0; k < nlines; ++k) {
        char *msg = starts[k];
        uat2esnt_convert_message(msg, msg + strlen(msg), output, output + sizeof output);
        const int32_t len = (int32_t) strlen(output);
        fwrite(output, 1, (size_t) len, fo);
        fwrite(&len, sizeof len, 1, fl);
    }
    fclose(fo);
    fclose(fl);
    return 0;
}
