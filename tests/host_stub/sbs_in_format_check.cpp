// sbs_in_format_check.cpp — readsb_amd/csrc/sbs_in_format.h, the parser the kernels of kernels/sbs_in.inc run, compiled for the host
// and run against the reference's records (tests/test_sbs_in_reference.py, tests/golden/make_sbs_in_golden.py).  Linked with
// readsb_amd/csrc/sbs_in_host.cpp; plain g++, also under ASan and UBSan.
//   sbs_in_format_check <stream.bin> <source> <now_ms> <want_line_of.bin> <want_recs.bin>
// Frames the stream as readAscii does ('\n' or NUL ends a line; the rest is not consumed).  Every line is parsed in a heap copy of
// exactly its bytes (so a read beyond it is ASan's to find), twice: with nothing resolved (the device's way) and through
// mgpu_sbs_parse_line_host.  A plain record must equal the host's and the reference's for that line; a deferred line's host record
// must equal the reference's; a line that gives nothing must have no reference record.  mgpu_sbs_parse_host by index agrees.
// stdout: "ok lines N recs R invalid I consumed C deferred d0 d1 ..." or the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sbs_in_format.h"

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static int fail(const char *what, uint64_t line, const mgpu_sbs_rec *got, const mgpu_sbs_rec *want) {
    printf("DIFF %s at line %llu\n", what, (unsigned long long) line);
    for (int pass = 0; pass < 2; ++pass) {
        const mgpu_sbs_rec *r = pass ? want : got;
        if (!r) continue;
        printf("  %s:", pass ? "want" : "got ");
        for (size_t k = 0; k < sizeof *r; ++k) printf("%s%02x", k % 8 ? "" : " ", ((const uint8_t *) r)[k]);
        printf("\n");
    }
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 6) { fprintf(stderr, "usage: %s stream.bin source now_ms want_line_of.bin want_recs.bin\n", argv[0]); return 2; }
    const std::vector<uint8_t> stream = slurp(argv[1]), lo = slurp(argv[4]), wr = slurp(argv[5]);
    const uint32_t source = (uint32_t) atoi(argv[2]);
    const int64_t now_ms = atoll(argv[3]);
    const size_t nwant = wr.size() / sizeof(mgpu_sbs_rec);
    if (lo.size() != nwant * sizeof(uint64_t) || wr.size() % sizeof(mgpu_sbs_rec)) { fprintf(stderr, "bad want files\n"); return 2; }
    std::vector<uint64_t> want_line(nwant);
    std::vector<mgpu_sbs_rec> want(nwant);
    if (nwant) { memcpy(want_line.data(), lo.data(), lo.size()); memcpy(want.data(), wr.data(), wr.size()); }

    struct mgpu_sbs_in_args args;
    memset(&args, 0, sizeof args);
    args.size = sizeof args;
    args.source = source;
    args.text = stream.data();
    args.nbytes = stream.size();
    args.now_ms = now_ms;

    uint64_t nlines = 0, nrecs = 0, ninvalid = 0, consumed = 0;
    size_t at_want = 0;
    std::vector<uint64_t> deferred;
    for (size_t p = 0; p < stream.size();) {
        size_t q = p;
        while (q < stream.size() && stream[q] != '\n' && stream[q] != 0) ++q;
        if (q >= stream.size()) break;
        const size_t len = q - p;
        uint8_t *copy = (uint8_t *) malloc(len ? len : 1);
        memcpy(copy, stream.data() + p, len);
        mgpu_sbs_rec plain, host, byindex;
        memset(&plain, 0xa5, sizeof plain);
        // (the kernels pass 257 for "no terminator within 256 bytes"; any length above 200 is the same verdict)
        const int cls = sbs_in_line(copy, (uint32_t) (len > 257 ? 257 : len), source, now_ms, SbsInPlainOnly{}, plain);
        const int rc = mgpu_sbs_parse_line_host(copy, len, source, now_ms, &host);
        const int rc2 = mgpu_sbs_parse_host(&args, nlines, &byindex);
        free(copy);
        if (rc < 0 || rc2 != rc || memcmp(&host, &byindex, sizeof host)) return fail("mgpu_sbs_parse_host by index", nlines, &byindex, &host);
        const bool has_want = at_want < nwant && want_line[at_want] == nlines;
        const mgpu_sbs_rec *w = has_want ? &want[at_want] : nullptr;
        if (cls == SBS_IN_RECORD || cls == SBS_IN_DEFER) {
            if (!w) return fail("a record the reference does not have", nlines, &host, nullptr);
            if (rc != 1 || memcmp(&host, w, sizeof host)) return fail("host record", nlines, &host, w);
            if (cls == SBS_IN_RECORD) {
                if (memcmp(&plain, w, sizeof plain)) return fail("plain record", nlines, &plain, w);
                ++nrecs;
            } else {
                deferred.push_back(nlines);
            }
            ++at_want;
        } else {
            if (w) return fail("no record where the reference has one", nlines, nullptr, w);
            if (rc != 0) return fail("host gives a record, the plain parse none", nlines, &host, nullptr);
            ninvalid += cls == SBS_IN_INVALID;
        }
        ++nlines;
        p = q + 1;
        consumed = p;
    }
    if (at_want != nwant) return fail("reference records left over", nlines, nullptr, &want[at_want]);
    mgpu_sbs_rec none;
    if (mgpu_sbs_parse_host(&args, nlines, &none) != MGPU_E_INVAL) return fail("a line behind the last one", nlines, nullptr, nullptr);
    printf("ok lines %llu recs %llu invalid %llu consumed %llu deferred", (unsigned long long) nlines, (unsigned long long) nrecs, (unsigned long long) ninvalid,
           (unsigned long long) consumed);
    for (uint64_t d : deferred) printf(" %llu", (unsigned long long) d);
    printf("\n");
    return 0;
}
