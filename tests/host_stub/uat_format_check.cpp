// uat_format_check.cpp — readsb_amd/csrc/uat_format.h, the formatter the kernels of kernels/uat.inc run, compiled for the host
// together with readsb_amd/csrc/uat_host.cpp and run over a stream against the bytes the reference's uat2esnt printed for it
// (tests/test_uat_reference.py).  Its own process, built with and without ASan / UBSan.
//   uat_format_check <stream.bin> <want.bin> <lens.bin>
// Per line: the device's policy (uat_line without an override: may defer) with the counting emitter and the byte emitter, which must
// agree; where it does not defer, the bytes are the reference's and no line is short; where it does, mgpu_uat_format_host settles the
// line to the reference's bytes.  Every line also goes through mgpu_uat_format_line_host, with its records checked against the text.
// The table of signal bytes must not decrease with ss where the reference's expression is defined.  stdout: "ok <lines> frames <n> short <n> deferred <indices...>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "uat_format.h"


static std::vector<uint8_t> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(1); }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

struct ByteEmit {
    uint8_t *p;
    uint32_t n;
    struct Sink { uint8_t *&p; void put(uint32_t c) { *p++ = (uint8_t) c; } };
    void frame(uint32_t sig, const UatFrame &fr) { Sink s{p}; uat_put_frame(s, sig, fr); ++n; }
};

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s stream.bin want.bin lens.bin\n", argv[0]); return 2; }
    const std::vector<uint8_t> stream = slurp(argv[1]), want = slurp(argv[2]), lens_raw = slurp(argv[3]);
    std::vector<int32_t> lens(lens_raw.size() / sizeof(int32_t));
    if (!lens.empty()) memcpy(lens.data(), lens_raw.data(), lens.size() * sizeof(int32_t));
    const uint8_t *tab = mgpu::uat_sig_table();
    // non-decreasing in ss as far as the reference's expression is defined: from ss = 138.6 on sqrt(10^(ss/10)) * 255 is beyond int, the
    // conversion undefined, and what the reference gets on x86-64 (INT_MIN, then "at least 1") is the 1 the table holds there
    const uint32_t defined_end = (uint32_t) kUatSigSpan + 1386u;
    for (uint32_t k = 1; k < kUatSigTable; ++k)
        if (k < defined_end ? tab[k] < tab[k - 1] : tab[k] != 1) { fprintf(stderr, "the signal table is wrong at %u\n", k); return 1; }
    if (tab[0] != 1 || tab[kUatSigSpan] != 255 || tab[defined_end - 1] != 255) { fprintf(stderr, "the signal table's ends\n"); return 1; }

    struct mgpu_uat_args args;
    memset(&args, 0, sizeof args);
    args.size = sizeof args;
    args.text = stream.data();
    args.nbytes = stream.size();
    args.now_ms = 1234567;

    size_t at = 0, line = 0, frames = 0, nshort = 0, start = 0;
    std::vector<size_t> deferred;
    for (size_t pos = 0; pos < stream.size(); ++pos) {
        if (stream[pos] != '\n') continue;
        if (line >= lens.size()) { fprintf(stderr, "more lines than lengths\n"); return 1; }
        // a copy of exactly the line's bytes: the sanitizer sees a read beyond them
        std::vector<uint8_t> text(stream.begin() + start, stream.begin() + pos);
        const uint8_t *p = text.empty() ? (const uint8_t *) "" : text.data();
        const size_t wlen = (size_t) lens[line];
        if (at + wlen > want.size()) { fprintf(stderr, "line %zu: the reference's bytes end early\n", line); return 1; }
        int cls = UAT_DEFER;
        if (text.size() <= 0xffffffffu) {
            UatCountEmit count = {0};
            cls = uat_line(p, (uint32_t) text.size(), tab, kUatNoOverride, count);
            uint8_t buf[64 + kUatMaxFrames * kUatFrameText];
            memset(buf, 0xA5, sizeof buf);
            ByteEmit bytes = {buf + 32, 0};
            const int cls2 = uat_line(p, (uint32_t) text.size(), tab, kUatNoOverride, bytes);
            const size_t wrote = (size_t) (bytes.p - (buf + 32));
            if (cls2 != cls || bytes.n != count.n || count.n > kUatMaxFrames || wrote != count.n * kUatFrameText) {
                fprintf(stderr, "line %zu: the two emitters disagree (%d/%d, %u/%u frames)\n", line, cls, cls2, count.n, bytes.n);
                return 1;
            }
            for (size_t j = 0; j < sizeof buf; ++j)
                if ((j < 32 || j >= 32 + wrote) && buf[j] != 0xA5) { fprintf(stderr, "line %zu: a byte outside the frames was written\n", line); return 1; }
            if (cls != UAT_FRAMES && count.n) { fprintf(stderr, "line %zu: class %d with frames\n", line, cls); return 1; }
            if (cls != UAT_DEFER && (wrote != wlen || memcmp(buf + 32, want.data() + at, wlen) != 0)) {
                fprintf(stderr, "line %zu (class %d): %zu bytes differ from the reference's %zu:\n--- got\n%.*s--- want\n%.*s", line, cls, wrote, wlen, (int) wrote,
                        (const char *) buf + 32, (int) wlen, (const char *) want.data() + at);
                return 1;
            }
            frames += count.n;
        }
        if (cls == UAT_SHORT) ++nshort;
        if (cls == UAT_DEFER) deferred.push_back(line);
        // the host's formatter, by index and by bytes: the reference's bytes for every line, the records and the signal byte the text's
        uint8_t host[kUatMaxFrames * kUatFrameText + 8];
        mgpu_msg msgs[kUatMaxFrames];
        uint8_t sig = 0;
        memset(host, 0xA5, sizeof host);
        const int64_t hl = cls == UAT_DEFER ? mgpu_uat_format_host(&args, line, host, kUatMaxFrames * kUatFrameText, msgs, &sig)
                                            : mgpu_uat_format_line_host(p, text.size(), args.now_ms, host, kUatMaxFrames * kUatFrameText, msgs, &sig);
        if (cls == UAT_SHORT ? hl != 0 : (hl != (int64_t) wlen || memcmp(host, want.data() + at, wlen) != 0)) {
            fprintf(stderr, "line %zu (class %d): the host formatter gives %lld bytes, the reference %zu\n", line, cls, (long long) hl, wlen);
            return 1;
        }
        for (size_t j = (size_t) (hl > 0 ? hl : 0); j < sizeof host; ++j)
            if (host[j] != 0xA5) { fprintf(stderr, "line %zu: the host formatter wrote beyond its bytes\n", line); return 1; }
        for (int64_t k = 0; k < hl / kUatFrameText; ++k) {
            const mgpu_msg &m = msgs[k];
            char hex[29];
            for (int j = 0; j < 14; ++j) snprintf(hex + 2 * j, 3, "%02X", m.msg[j]);
            char sg[3];
            snprintf(sg, sizeof sg, "%02X", sig);
            const uint8_t *t = host + k * kUatFrameText;
            if (memcmp(hex, t + 15, 28) != 0 || memcmp(sg, t + 13, 2) != 0 || memcmp(m.msg, m.raw, 14) != 0 || m.timestamp != kUatTimestamp || m.sysTimestamp != args.now_ms ||
                m.msgtype != 18 || m.msgbits != 112 || m.correctedbits || m.score || m.phase || m.sig_len != 1 || m.sig_sumsq != (uint64_t) (257u * sig) * (257u * sig) ||
                m.addr != ((uint32_t) m.msg[1] << 16 | (uint32_t) m.msg[2] << 8 | m.msg[3])) {
                fprintf(stderr, "line %zu: record %lld does not match its text\n", line, (long long) k);
                return 1;
            }
        }
        at += wlen;
        ++line;
        start = pos + 1;
    }
    if (at != want.size() || line != lens.size()) { fprintf(stderr, "the reference printed %zu bytes for %zu lines, the stream accounts for %zu and %zu\n", want.size(), lens.size(), at, line); return 1; }
    if (mgpu_uat_format_host(&args, line, nullptr, 0, nullptr, nullptr) != MGPU_E_INVAL) { fprintf(stderr, "a line behind the last one\n"); return 1; }
    printf("ok %zu frames %zu short %zu deferred", line, frames, nshort);
    for (size_t k : deferred) printf(" %zu", k);
    printf("\n");
    return 0;
}
