// dump_format_check.cpp — readsb_amd/csrc/dump_format.h, the formatter the kernels of kernels/dump.inc run, compiled for the host and
// run over a file of case records against the bytes the reference's displayModesMessage printed for them (tests/test_dump_reference.py;
// the case record is tests/host_stub/dump_ref_harness.c's).  Its own process, built with and without ASan / UBSan.
//   dump_format_check <cases.bin> <want.bin> <lens.bin> <flags> <show_only>
// Per case and for both policies of the one transcendental (the device's: defer when the rounding is uncertain; the host's: exact):
// the class agrees with the case's `run` mark and the reference's length, the counting sink and the byte sink agree about the length,
// the bytes are the reference's, nothing is written outside them, and no dump is longer than kDumpMax.
// stdout: "ok <dumps> deferred <indices...>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dump_format.h"

struct DumpCase {
    mgpu_msg m;
    mgpu_fields f;
    double lat, lon;
    uint64_t receiver_id;
    uint32_t decoded_rc;
    uint8_t method, has_positions, decoded_nic, run;
    int8_t reduce_forward;
    uint8_t pad[7];
};
static_assert(sizeof(DumpCase) == 280, "case record");

static std::vector<uint8_t> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(1); }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

int main(int argc, char **argv) {
    if (argc != 6) { fprintf(stderr, "usage: %s cases.bin want.bin lens.bin flags show_only\n", argv[0]); return 2; }
    const std::vector<uint8_t> cases_raw = slurp(argv[1]), want = slurp(argv[2]), lens_raw = slurp(argv[3]);
    const uint32_t flags = (uint32_t) strtoul(argv[4], nullptr, 0), show_only = (uint32_t) strtoul(argv[5], nullptr, 0);
    const size_t n = cases_raw.size() / sizeof(DumpCase);
    if (lens_raw.size() != n * sizeof(int32_t)) { fprintf(stderr, "lens.bin does not match cases.bin\n"); return 1; }
    std::vector<DumpCase> cases(n);
    std::vector<int32_t> lens(n);
    if (n) { memcpy(cases.data(), cases_raw.data(), n * sizeof(DumpCase)); memcpy(lens.data(), lens_raw.data(), n * sizeof(int32_t)); }

    size_t at = 0, dumps = 0;
    std::vector<size_t> deferred;
    std::vector<uint8_t> buf(kDumpMax + 64);
    for (size_t k = 0; k < n; ++k) {
        const DumpCase &c = cases[k];
        mgpu_position pos = {};
        pos.lat = c.lat; pos.lon = c.lon; pos.method = c.method;
        const DumpIn in = {&c.m, &c.f, c.has_positions ? &pos : nullptr, c.receiver_id, c.decoded_rc, (uint8_t) c.reduce_forward, c.decoded_nic};
        const int host_cls = dump_classify(in, flags, show_only, true), dev_cls = dump_classify(in, flags, show_only, false);
        const bool dumped = host_cls == DUMP_LINE;
        if (host_cls == DUMP_DEFER || (dev_cls != host_cls && !(dev_cls == DUMP_DEFER && dumped))) {        // the host never defers; the device defers dumps only
            fprintf(stderr, "case %zu: classes %d / %d\n", k, host_cls, dev_cls);
            return 1;
        }
        if (dumped != (lens[k] != 0) || (host_cls == DUMP_SKIP && c.run)) {
            fprintf(stderr, "case %zu: class %d, run %d, the reference printed %d bytes\n", k, host_cls, c.run, lens[k]);
            return 1;
        }
        if (!dumped) continue;
        ++dumps;
        if (dev_cls == DUMP_DEFER) deferred.push_back(k);
        for (int policy = 0; policy < 2; ++policy) {
            const bool exact = policy == 0;
            if (!exact && dev_cls != DUMP_LINE) continue;
            DumpCountSink count = {0};
            dump_format(in, flags, exact, count);
            if (count.n != (uint32_t) lens[k] || count.n > (uint32_t) kDumpMax) {
                fprintf(stderr, "case %zu: the counting sink says %u bytes, the reference printed %d (bound %d)\n", k, count.n, lens[k], kDumpMax);
                return 1;
            }
            memset(buf.data(), 0xA5, buf.size());
            DumpByteSink bytes = {buf.data() + 32};
            dump_format(in, flags, exact, bytes);
            const size_t wrote = (size_t) (bytes.p - (buf.data() + 32));
            if (wrote != count.n || at + wrote > want.size() || memcmp(buf.data() + 32, want.data() + at, wrote) != 0) {
                fprintf(stderr, "case %zu (policy %d): %zu bytes differ from the reference's %d:\n--- got\n%.*s--- want\n%.*s", k, policy, wrote, lens[k], (int) wrote,
                        (const char *) buf.data() + 32, (int) lens[k], at + lens[k] <= want.size() ? (const char *) want.data() + at : "");
                return 1;
            }
            for (size_t j = 0; j < buf.size(); ++j)
                if ((j < 32 || j >= 32 + wrote) && buf[j] != 0xA5) { fprintf(stderr, "case %zu: a byte outside the dump was written\n", k); return 1; }
        }
        at += (size_t) lens[k];
    }
    if (at != want.size()) { fprintf(stderr, "the reference printed %zu bytes, the cases account for %zu\n", want.size(), at); return 1; }
    printf("ok %zu deferred", dumps);
    for (size_t k : deferred) printf(" %zu", k);
    printf("\n");
    return 0;
}
