// raw_in_format_check.cpp — the raw input's parser (readsb_amd/csrc/raw_in_format.h) and the sequential resolver
// (raw_in_host.cpp: raw_in_decode_sequential over icao_filter.h's IcaoFilter) on the host against what the REFERENCE left for a stream (tests/golden/raw_in_cases.npz,
// written out by tests/golden/make_raw_in_golden.py: run_check).  Plain g++, with -fsanitize=address,undefined too; every line is
// also parsed in a heap copy of exactly its bytes, so that a read beyond a line is an error.
//   raw_in_format_check <stream.bin> <now_ms> <nfix_crc> <fixDF> <mode_ac> <filter.bin> <head.bin> <class.bin> <line_of.bin> <signal.bin> <msgs.bin>
// filter.bin: int32 values, >= 0 icaoFilterAdd(value), -1 icaoFilterExpire().  Prints "ok lines L msgs M" or the first difference.
// Without arguments but "mv": the signal byte of every Aerobits value -1100..1100 mV against the reference's formula
// (net_io.c:4144-4147, 1696-1700).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "raw_in_host.h"

static std::vector<uint8_t> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
    fclose(f);
    return d;
}

static int check_mv() {
    for (long mv = -1100; mv <= 1100; ++mv) {
        double s = (double) mv;
        s /= 1000;
        s = s * s;
        s = fmin(1.0, s);
        int sig = (int) nearbyint(sqrt(s) * 255);
        if (s > 0 && sig < 1) sig = 1;
        if (sig > 255) sig = 255;
        if ((uint32_t) sig != mgpu::raw_in_mv_byte(mv)) { printf("mv %ld: reference %d, parser %u\n", mv, sig, mgpu::raw_in_mv_byte(mv)); return 1; }
        // ... and through the parser itself: the record's byte and the double
        char line[96];
        const int n = snprintf(line, sizeof line, "*8D4840D6202CC371C32CE0576098;(%ld,1,10)", mv);
        uint8_t *copy = (uint8_t *) malloc((size_t) n);
        memcpy(copy, line, (size_t) n);
        const mgpu_raw_in_config cfg = {sizeof cfg, 1, 1, 0};
        mgpu_raw_in_line out;
        const int rc = mgpu_raw_parse_line_host(copy, (uint64_t) n, 1700000123456ll, &cfg, &out);
        free(copy);
        if (rc != 1 || out.msg.sig_sumsq != (uint64_t) (257 * sig) * (uint64_t) (257 * sig) || memcmp(&out.signal_level, &s, 8)) { printf("mv %ld through the parser\n", mv); return 1; }
    }
    printf("ok mv\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "mv")) return check_mv();
    if (argc != 12) { fprintf(stderr, "usage\n"); return 2; }
    const std::vector<uint8_t> stream = slurp(argv[1]);
    const int64_t now = atoll(argv[2]);
    const mgpu_raw_in_config cfg = {sizeof cfg, atoi(argv[3]), atoi(argv[4]), (uint32_t) atoi(argv[5])};
    const std::vector<uint8_t> fops = slurp(argv[6]), head_b = slurp(argv[7]), want_cls = slurp(argv[8]), want_line = slurp(argv[9]), want_sig = slurp(argv[10]), want_msgs = slurp(argv[11]);
    if (head_b.size() != 80) { printf("head\n"); return 1; }
    uint64_t head[10];
    memcpy(head, head_b.data(), 80);

    // the filter's preparation, through the library's model of icao_filter.c
    mgpu::IcaoFilter flt;
    for (size_t k = 0; k + 4 <= fops.size(); k += 4) {
        int32_t op;
        memcpy(&op, fops.data() + k, 4);
        if (op >= 0) flt.add((uint32_t) op); else flt.expire();
    }
    const uint64_t nl_most = stream.size() + 1, cap = stream.size() / 6 + 1;

    std::vector<mgpu_msg> msgs(cap);
    std::vector<uint64_t> line_of(cap);
    std::vector<double> sig(cap);
    std::vector<uint8_t> cls(nl_most);
    uint64_t consumed = 0, nlines = 0, nmsgs = 0;
    mgpu_raw_in_counters cn;
    // the text in a heap copy of exactly its bytes
    uint8_t *text = (uint8_t *) malloc(stream.size() ? stream.size() : 1);
    memcpy(text, stream.data(), stream.size());
    mgpu_raw_in_args a;
    memset(&a, 0, sizeof a);
    a.size = sizeof a; a.text = text; a.nbytes = stream.size(); a.now_ms = now;
    a.msgs = msgs.data(); a.line_of = line_of.data(); a.signal_level = sig.data(); a.msgs_cap = cap;
    a.line_class = cls.data(); a.line_class_cap = nl_most;
    a.consumed = &consumed; a.nlines = &nlines; a.nmsgs = &nmsgs; a.counters = &cn;
    const int rc = mgpu::raw_in_decode_sequential(&a, &cfg, flt);
    if (rc != MGPU_OK) { printf("raw_in_decode_sequential %d\n", rc); return 1; }
    const uint64_t got[10] = {consumed, nlines, nmsgs, cn.remote_received_modes, cn.remote_received_modeac, cn.remote_rejected_unknown_icao, cn.remote_rejected_bad,
                              cn.remote_accepted[0], cn.remote_accepted[1], cn.remote_accepted[2]};
    for (int k = 0; k < 10; ++k)
        if (got[k] != head[k]) { printf("count %d: reference %llu, here %llu\n", k, (unsigned long long) head[k], (unsigned long long) got[k]); }
    if (want_cls.size() != nlines) { printf("lines\n"); return 1; }
    // every line once more in a heap copy of its own
    {
        const uint8_t *p = text, *end = text + stream.size();
        uint64_t k = 0;
        while (p < end) {
            const uint8_t *q = p;
            while (q < end && *q != '\n' && *q != 0) ++q;
            if (q >= end) break;
            const size_t n = (size_t) (q - p);
            uint8_t *copy = (uint8_t *) malloc(n ? n : 1);
            memcpy(copy, p, n);
            mgpu_raw_in_line one;
            (void) mgpu_raw_parse_line_host(n ? copy : nullptr, n, now, &cfg, &one);
            free(copy);
            const uint32_t c = cls[k];
            const bool fits = one.cls == c || (one.cls == MGPU_RAW_COND && (c == MGPU_RAW_ACCEPT || c == MGPU_RAW_UNKNOWN));
            if (!fits) { printf("line %llu: its own parse gives class %u, the stream's %u\n", (unsigned long long) k, one.cls, c); return 1; }
            if (c != want_cls[k]) { printf("line %llu: class %u, reference %u: %.*s\n", (unsigned long long) k, c, want_cls[k], (int) n, (const char *) p); return 1; }
            ++k;
            p = q + 1;
        }
    }
    if (memcmp(got, head, 80)) return 1;
    if (want_msgs.size() != nmsgs * 64 || want_line.size() != nmsgs * 8 || want_sig.size() != nmsgs * 8) { printf("sizes\n"); return 1; }
    for (uint64_t k = 0; k < nmsgs; ++k) {
        if (memcmp(&line_of[k], want_line.data() + 8 * k, 8)) { printf("message %llu: line\n", (unsigned long long) k); return 1; }
        if (memcmp(&sig[k], want_sig.data() + 8 * k, 8)) { printf("message %llu (line %llu): signal\n", (unsigned long long) k, (unsigned long long) line_of[k]); return 1; }
        if (memcmp(&msgs[k], want_msgs.data() + 64 * k, 64)) {
            const uint8_t *g = (const uint8_t *) &msgs[k], *w = want_msgs.data() + 64 * k;
            int at = 0;
            while (g[at] == w[at]) ++at;
            printf("message %llu (line %llu): byte %d is %02x, reference %02x\n", (unsigned long long) k, (unsigned long long) line_of[k], at, g[at], w[at]);
            return 1;
        }
    }
    free(text);
    printf("ok lines %llu msgs %llu\n", (unsigned long long) nlines, (unsigned long long) nmsgs);
    return 0;
}
