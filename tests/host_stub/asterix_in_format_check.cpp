// asterix_in_format_check.cpp — readsb_amd/csrc/asterix_in_format.h, the parser and the framing rule the kernels of
// kernels/asterix_in.inc run, compiled for the host and run against the reference's records (tests/test_asterix_in_reference.py,
// tests/golden/make_asterix_in_golden.py).  Linked with readsb_amd/csrc/asterix_in_host.cpp; plain g++, also under ASan and UBSan.
//   asterix_in_format_check <stream.bin> <source> <now_ms> <want_frame_of.bin> <want_recs.bin>
// The stream is framed and parsed in a heap copy of exactly its bytes (a read beyond it is ASan's to find); every record must equal
// the reference's for that frame, and mgpu_asterix_parse_host by index must agree.
//   asterix_in_format_check rules
// the rules that have no reference: the time of all 2^24 raw values against (int)(raw / .128); the high-precision arithmetic against
// figures worked by hand (the golden streams hold it to the reference); MGPU_AST_STOP_ZERO_LEN, MGPU_AST_STOP_END, and chains longer
// than 191 extension bytes.
// stdout: "ok frames N recs R other O undefined U consumed C stop S" or the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "asterix_in_format.h"

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

static int fail(const char *what, uint64_t frame, const mgpu_asterix_rec *got, const mgpu_asterix_rec *want) {
    printf("DIFF %s at frame %llu\n", what, (unsigned long long) frame);
    for (int pass = 0; pass < 2; ++pass) {
        const mgpu_asterix_rec *r = pass ? want : got;
        if (!r) continue;
        printf("  %s:", pass ? "want" : "got ");
        for (size_t k = 0; k < sizeof *r; ++k) printf("%s%02x", k % 8 ? "" : " ", ((const uint8_t *) r)[k]);
        printf("\n");
    }
    return 1;
}

struct Walk { uint64_t frames, recs, other, undefined, consumed; uint32_t stop; };

// the whole rule over a stream, as a call of mgpu_asterix_decode reports it
static Walk walk(const uint8_t *d, uint64_t n, uint32_t source, int64_t now_ms, std::vector<mgpu_asterix_rec> *recs, std::vector<uint64_t> *frame_of) {
    Walk w = {0, 0, 0, 0, 0, MGPU_AST_STOP_END};
    const AstBytes s = {d, n};
    for (uint64_t at = 0;;) {
        uint32_t len;
        const int st = ast_in_frame(s, at, len);
        w.consumed = at;
        if (st != AST_IN_FRAME) { w.stop = st == AST_IN_ZERO_LEN ? MGPU_AST_STOP_ZERO_LEN : MGPU_AST_STOP_END; return w; }
        mgpu_asterix_rec r;
        const int cls = ast_in_record(s, at, source, now_ms, r);
        if (cls == AST_IN_RECORD) { if (recs) recs->push_back(r); if (frame_of) frame_of->push_back(w.frames); ++w.recs; }
        w.other += cls == AST_IN_OTHER;
        w.undefined += cls == AST_IN_UNDEFINED;
        ++w.frames;
        at += len;
        if (cls == AST_IN_CLOSED) { w.consumed = at; w.stop = MGPU_AST_STOP_CLOSED; return w; }
    }
}

#define CHECK(cond) do { if (!(cond)) { printf("DIFF rule: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

static int rules() {
    // readAsterixTime's division, all 2^24 raw values, at a now_ms that keeps the day
    const int64_t now = 1700000000000ll - 1700000000000ll % 86400000 + 43200000;
    for (uint32_t raw = 0; raw < (1u << 24); ++raw) {
        const uint8_t b[3] = {(uint8_t) (raw >> 16), (uint8_t) (raw >> 8), (uint8_t) raw};
        uint64_t p = 0;
        const uint64_t t = ast_in_time(AstBytes{b, 3}, p, now);
        const int mssm = (int) (raw / .128);
        const int64_t midnight = now / 86400000 * 86400000;
        const int64_t diff = midnight + mssm - now;
        const int64_t want = (diff < 0 ? -diff : diff) > 43200000 ? midnight - 86400000 + mssm : midnight + mssm;
        if (p != 3 || (int64_t) t != want) { printf("DIFF time raw %u: %lld, want %lld\n", raw, (long long) t, (long long) want); return 1; }
    }
    // readAsterixHighPrecisionTime as the reference's x86-64 build computes it
    {
        const uint8_t zero[4] = {0, 0, 0, 0}, fsi1[4] = {0x40, 0, 0, 0}, fsi2[4] = {0x80, 0, 0, 0}, frac[4] = {0x04, 0, 0, 0};
        uint64_t p = 0;
        CHECK(ast_in_hp_time(AstBytes{zero, 4}, p, 1700000000123ull) == 18446744072902502400ull && p == 4);
        p = 0;
        CHECK(ast_in_hp_time(AstBytes{fsi1, 4}, p, 1792468800999ull) == 1467437569ull);
        p = 0;
        CHECK(ast_in_hp_time(AstBytes{fsi2, 4}, p, 1792468800999ull) == 1467437567ull);
        p = 0;
        CHECK(ast_in_hp_time(AstBytes{frac, 4}, p, 1792468800999ull) == 1467437568ull);      // + 0.5: truncated
        p = 0;
        CHECK(ast_in_hp_time(AstBytes{fsi2, 4}, p, 999ull) == 0);                             // 0 - 1 wraps to 2^64 - 1, a double of 2^64: 0
    }
    // the framing rules without a reference
    {
        std::vector<uint8_t> s = {21, 0, 6, 0x01, 0x10, 0xaa, 21, 0, 0, 1, 2, 3};                 // a record of 6, then a length of 0
        Walk w = walk(s.data(), s.size(), 1, now, nullptr, nullptr);
        CHECK(w.frames == 1 && w.recs == 1 && w.consumed == 6 && w.stop == MGPU_AST_STOP_ZERO_LEN);
        s = {21, 0, 6, 0x01, 0x10, 0xaa, 21, 0, 7, 1, 2, 3};                                       // .. then a record one byte too long
        w = walk(s.data(), s.size(), 1, now, nullptr, nullptr);
        CHECK(w.frames == 1 && w.consumed == 6 && w.stop == MGPU_AST_STOP_END);
        s = {21, 0, 6, 0x01, 0x10, 0xaa, 21, 0};                                                    // .. then two bytes
        w = walk(s.data(), s.size(), 1, now, nullptr, nullptr);
        CHECK(w.frames == 1 && w.consumed == 6 && w.stop == MGPU_AST_STOP_END);
        s = {21, 0, 6, 0x01, 0x10, 0xaa};                                                           // the stream ends at a record's end
        w = walk(s.data(), s.size(), 1, now, nullptr, nullptr);
        CHECK(w.frames == 1 && w.consumed == 6 && w.stop == MGPU_AST_STOP_END);
        s = {21, 0, 5, 0x01, 0x00, 21, 0, 5, 0x01, 0x10};                                           // no address: closed, nothing behind it
        w = walk(s.data(), s.size(), 1, now, nullptr, nullptr);
        CHECK(w.frames == 1 && w.recs == 0 && w.undefined == 0 && w.consumed == 5 && w.stop == MGPU_AST_STOP_CLOSED);
        s = {0x80, 0x80, 0x80};                                                                     // (-128 << 8) + -128 = 0x7f80 as uint16_t
        uint32_t len;
        CHECK(ast_in_frame(AstBytes{s.data(), 3}, 0, len) == AST_IN_END && len == 0x7f80 && ast_in_len(0xff, 0xff) == 0xfeff && ast_in_len(0x01, 0x80) == 0x0080);
    }
    // chains: 191 extension bytes are read, 192 are not; in the main FSPEC (with and without the address bit), I021/040, /090, /220
    for (int which = 0; which < 5; ++which)
        for (uint32_t ext = 190; ext <= 193; ++ext) {
            std::vector<uint8_t> s = {21, 0, 0};
            std::vector<uint8_t> ch(ext + 1, 0x01);
            ch[ext] = 0;
            if (which <= 1) {                                                                       // the main FSPEC itself
                ch[1] = which == 0 ? 0x11 : 0x01;
                s.insert(s.end(), ch.begin(), ch.end());
            } else {
                const uint8_t f[5] = {(uint8_t) (which == 2 ? 0x41 : 0x01), 0x11, (uint8_t) (which == 3 ? 0x21 : 0x01), 0x01, (uint8_t) (which == 4 ? 0x20 : 0x00)};
                s.insert(s.end(), f, f + 5);
                if (which == 2) s.insert(s.end(), ch.begin(), ch.end());
                s.insert(s.end(), {0x4a, 0xc8, 0xb3});
                if (which != 2) s.insert(s.end(), ch.begin(), ch.end());
            }
            s[1] = (uint8_t) (s.size() >> 8);
            s[2] = (uint8_t) s.size();
            if (s[2] >= 0x80) s[1] += 1;
            s.insert(s.end(), {21, 0, 5, 0x01, 0x10});                                              // a record behind it: framing goes on
            const Walk w = walk(s.data(), s.size(), 1, now, nullptr, nullptr);
            const bool defined = ext <= kAstInMaxChain;
            if (which == 1 && defined) CHECK(w.stop == MGPU_AST_STOP_CLOSED && w.frames == 1 && w.recs == 0 && w.undefined == 0);
            else CHECK(w.stop == MGPU_AST_STOP_END && w.consumed == s.size() && w.frames == 2 && w.undefined == (defined ? 0u : 1u) && w.recs == (defined ? 2u : 1u));
        }
    printf("ok rules\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "rules")) return rules();
    if (argc != 6) { fprintf(stderr, "usage: %s stream.bin source now_ms want_frame_of.bin want_recs.bin | rules\n", argv[0]); return 2; }
    const std::vector<uint8_t> file = slurp(argv[1]), fo = slurp(argv[4]), wr = slurp(argv[5]);
    const uint32_t source = (uint32_t) atoi(argv[2]);
    const int64_t now_ms = atoll(argv[3]);
    const size_t nwant = wr.size() / sizeof(mgpu_asterix_rec);
    if (fo.size() != nwant * sizeof(uint64_t) || wr.size() % sizeof(mgpu_asterix_rec)) { fprintf(stderr, "bad want files\n"); return 2; }
    std::vector<uint64_t> want_frame(nwant);
    std::vector<mgpu_asterix_rec> want(nwant);
    if (nwant) { memcpy(want_frame.data(), fo.data(), fo.size()); memcpy(want.data(), wr.data(), wr.size()); }
    uint8_t *stream = (uint8_t *) malloc(file.size() ? file.size() : 1);                           // exactly its bytes
    if (file.size()) memcpy(stream, file.data(), file.size());

    std::vector<mgpu_asterix_rec> recs;
    std::vector<uint64_t> frame_of;
    const Walk w = walk(stream, file.size(), source, now_ms, &recs, &frame_of);
    for (size_t k = 0; k < recs.size() || k < nwant; ++k) {
        if (k >= nwant) return fail("a record the reference has not", frame_of[k], &recs[k], nullptr);
        if (k >= recs.size()) return fail("no record where the reference has one", want_frame[k], nullptr, &want[k]);
        if (frame_of[k] != want_frame[k]) return fail("the record's frame", frame_of[k], &recs[k], &want[k]);
        if (memcmp(&recs[k], &want[k], sizeof(mgpu_asterix_rec)) != 0) return fail("record", frame_of[k], &recs[k], &want[k]);
    }
    struct mgpu_asterix_in_args args;
    memset(&args, 0, sizeof args);
    args.size = sizeof args;
    args.source = source;
    args.data = stream;
    args.nbytes = file.size();
    args.now_ms = now_ms;
    size_t at = 0;
    for (uint64_t f = 0; f < w.frames; f += 1 + f / 8) {                                           // by index: the first ones, then thinning out
        while (at < nwant && want_frame[at] < f) ++at;
        mgpu_asterix_rec r;
        const int rc = mgpu_asterix_parse_host(&args, f, &r);
        const bool has = at < nwant && want_frame[at] == f;
        if (rc != (has ? 1 : 0) || (has && memcmp(&r, &want[at], sizeof r) != 0)) return fail("mgpu_asterix_parse_host", f, &r, has ? &want[at] : nullptr);
    }
    mgpu_asterix_rec r;
    if (mgpu_asterix_parse_host(&args, w.frames, &r) != MGPU_E_INVAL) return fail("mgpu_asterix_parse_host behind the last frame", w.frames, nullptr, nullptr);
    free(stream);
    printf("ok frames %llu recs %llu other %llu undefined %llu consumed %llu stop %u\n", (unsigned long long) w.frames, (unsigned long long) w.recs,
           (unsigned long long) w.other, (unsigned long long) w.undefined, (unsigned long long) w.consumed, w.stop);
    return 0;
}
