// pf_in_format_check.cpp — the Planefinder input's framer and parser (readsb_amd/csrc/pf_in_format.h) and the sequential walk
// (pf_in_host.cpp: pf_in_decode_sequential over icao_filter.h's IcaoFilter) on the host against what the REFERENCE left for a stream
// (tests/golden/pf_in_cases.npz, written out by tests/pf_in_util.py's callers).  Plain g++, with -fsanitize=address,undefined too; the
// stream is walked in a heap copy of exactly its bytes, so that a read at or beyond nbytes is an error.
//   pf_in_format_check <stream.bin> <now_ms> <nfix_crc> <fixDF> <mode_ac> <filter.bin> <head.bin> <class.bin> <off.bin> <frame_of.bin> <signal.bin> <msgs.bin>
// filter.bin: int32 values, >= 0 icaoFilterAdd(value), -1 icaoFilterExpire().  Prints "ok frames F msgs M skipped S past P" or the
// first difference.
//   pf_in_format_check prefixes <stream.bin> <now_ms> <nfix_crc> <fixDF> <mode_ac>
// every prefix of the stream, each in a heap copy of exactly its bytes: the sequential walk, whole and in passes of 1, 7 and 33 bytes,
// against a walk over mgpu_pf_parse_host alone, step by step (consumed, handler calls with offset and class, skipped frames, reads past
// the end), and what holds of any result (consumed <= nbytes, nframes <= nbytes / 4, offsets ascending and below consumed).  Prints
// "ok prefixes N".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pf_in_host.h"

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

struct Result {
    std::vector<mgpu_msg> msgs;
    std::vector<uint64_t> frame_of, off;
    std::vector<double> sig;
    std::vector<uint8_t> cls;
    uint64_t consumed = 0, nframes = 0, nmsgs = 0;
    mgpu_pf_in_counters cn;
};

static int run(const uint8_t *data, uint64_t n, int64_t now, const mgpu_raw_in_config &cfg, uint64_t pass_bytes, mgpu::IcaoFilter &flt, Result &r) {
    const uint64_t cap = n / 4 + 1;
    r.msgs.assign(cap, mgpu_msg()); r.frame_of.assign(cap, 0); r.sig.assign(cap, 0.0); r.cls.assign(cap, 0); r.off.assign(cap, 0);
    mgpu_pf_in_args a;
    memset(&a, 0, sizeof a);
    a.size = sizeof a; a.data = data; a.nbytes = n; a.now_ms = now; a.pass_bytes = pass_bytes;
    a.msgs = r.msgs.data(); a.signal_level = r.sig.data(); a.frame_of = r.frame_of.data(); a.msgs_cap = cap;
    a.frame_class = r.cls.data(); a.frame_off = r.off.data(); a.frames_cap = cap;
    a.consumed = &r.consumed; a.nframes = &r.nframes; a.nmsgs = &r.nmsgs; a.counters = &r.cn;
    return mgpu::pf_in_decode_sequential(&a, &cfg, flt);
}

static bool same(const Result &a, const Result &b) {
    if (a.consumed != b.consumed || a.nframes != b.nframes || a.nmsgs != b.nmsgs || memcmp(&a.cn, &b.cn, sizeof a.cn)) return false;
    if (memcmp(a.cls.data(), b.cls.data(), a.nframes) || memcmp(a.off.data(), b.off.data(), 8 * a.nframes)) return false;
    return !memcmp(a.msgs.data(), b.msgs.data(), 64 * a.nmsgs) && !memcmp(a.frame_of.data(), b.frame_of.data(), 8 * a.nmsgs) && !memcmp(a.sig.data(), b.sig.data(), 8 * a.nmsgs);
}

static int check_prefixes(int argc, char **argv) {
    if (argc != 7) { fprintf(stderr, "usage\n"); return 2; }
    const std::vector<uint8_t> stream = slurp(argv[2]);
    const int64_t now = atoll(argv[3]);
    const mgpu_raw_in_config cfg = {sizeof cfg, atoi(argv[4]), atoi(argv[5]), (uint32_t) atoi(argv[6])};
    mgpu::IcaoFilter flt, pflt;                                            // (two bitmaps of 2 MB each: made once, emptied per run)
    const mgpu::IcaoFilter::Snapshot empty;
    for (size_t n = 0; n <= stream.size(); ++n) {
        uint8_t *copy = (uint8_t *) malloc(n ? n : 1);
        memcpy(copy, stream.data(), n);
        flt.restore(empty);
        Result r;
        const int rc = run(copy, n, now, cfg, 0, flt, r);
        if (rc != MGPU_OK) { printf("prefix %zu: %d\n", n, rc); return 1; }
        for (uint64_t pass : {1, 7, 33}) {
            pflt.restore(empty);
            Result pr;
            if (run(copy, n, now, cfg, pass, pflt, pr) != MGPU_OK || !same(r, pr)) { printf("prefix %zu: passes of %llu differ from the whole call\n", n, (unsigned long long) pass); return 1; }
        }
        // the plain walk over mgpu_pf_parse_host
        uint64_t som = 0, frames = 0, skipped = 0, past = 0;
        while (som < n) {
            mgpu_pf_in_frame f;
            const int one = mgpu_pf_parse_host(copy, n, som, now, &cfg, &f);
            if (one < 0) { printf("prefix %zu: parse at %llu gives %d\n", n, (unsigned long long) som, one); return 1; }
            if (f.step == MGPU_PF_STEP_END || f.step == MGPU_PF_STEP_INCOMPLETE) {
                if (f.next != som) { printf("prefix %zu: a step that ends the loop moves som\n", n); return 1; }
                break;
            }
            if (f.next <= som || f.next > n) { printf("prefix %zu: step at %llu goes to %llu\n", n, (unsigned long long) som, (unsigned long long) f.next); return 1; }
            const uint64_t at = som;
            som = f.next;
            skipped += f.step == MGPU_PF_STEP_OTHER;
            if (f.step == MGPU_PF_STEP_FRAME) {
                if (one != 1 || frames >= r.nframes || r.off[frames] != f.frame_off || f.frame_off < at || f.frame_off + 4 > som) { printf("prefix %zu: handler call %llu\n", n, (unsigned long long) frames); return 1; }
                const uint32_t c = r.cls[frames];
                if (!(f.cls == c || (f.cls == MGPU_PF_IN_COND && (c == MGPU_PF_IN_ACCEPT || c == MGPU_PF_IN_UNKNOWN)))) { printf("prefix %zu: class of call %llu\n", n, (unsigned long long) frames); return 1; }
                if (frames && r.off[frames] <= r.off[frames - 1]) { printf("prefix %zu: offsets\n", n); return 1; }
                past += f.past_end;
                ++frames;
            }
        }
        if (som != r.consumed || frames != r.nframes || skipped != r.cn.nskipped || past != r.cn.past_end || r.consumed > n || r.nframes > n / 4 || r.nmsgs > r.nframes) {
            printf("prefix %zu: walk consumed %llu frames %llu skipped %llu past %llu, resolver %llu %llu %llu %llu\n", n, (unsigned long long) som, (unsigned long long) frames,
                   (unsigned long long) skipped, (unsigned long long) past, (unsigned long long) r.consumed, (unsigned long long) r.nframes, (unsigned long long) r.cn.nskipped,
                   (unsigned long long) r.cn.past_end);
            return 1;
        }
        free(copy);
    }
    printf("ok prefixes %zu\n", stream.size() + 1);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "prefixes")) return check_prefixes(argc, argv);
    if (argc != 13) { fprintf(stderr, "usage\n"); return 2; }
    const std::vector<uint8_t> stream = slurp(argv[1]);
    const int64_t now = atoll(argv[2]);
    const mgpu_raw_in_config cfg = {sizeof cfg, atoi(argv[3]), atoi(argv[4]), (uint32_t) atoi(argv[5])};
    const std::vector<uint8_t> fops = slurp(argv[6]), head_b = slurp(argv[7]), want_cls = slurp(argv[8]), want_off = slurp(argv[9]), want_frame = slurp(argv[10]),
                               want_sig = slurp(argv[11]), want_msgs = slurp(argv[12]);
    if (head_b.size() != 80) { printf("head\n"); return 1; }
    uint64_t head[10];
    memcpy(head, head_b.data(), 80);
    mgpu::IcaoFilter flt;
    for (size_t k = 0; k + 4 <= fops.size(); k += 4) {
        int32_t op;
        memcpy(&op, fops.data() + k, 4);
        if (op >= 0) flt.add((uint32_t) op); else flt.expire();
    }
    uint8_t *data = (uint8_t *) malloc(stream.size() ? stream.size() : 1);
    memcpy(data, stream.data(), stream.size());
    Result r;
    const int rc = run(data, stream.size(), now, cfg, 0, flt, r);
    if (rc != MGPU_OK) { printf("pf_in_decode_sequential %d\n", rc); return 1; }
    const uint64_t got[10] = {r.consumed, r.nframes, r.nmsgs, r.cn.remote_received_modes, r.cn.remote_received_modeac, r.cn.remote_rejected_unknown_icao, r.cn.remote_rejected_bad,
                              r.cn.remote_accepted[0], r.cn.remote_accepted[1], r.cn.remote_accepted[2]};
    int bad = 0;
    for (int k = 0; k < 10; ++k)
        if (got[k] != head[k]) { printf("count %d: reference %llu, here %llu\n", k, (unsigned long long) head[k], (unsigned long long) got[k]); bad = 1; }
    if (bad) return 1;
    if (want_cls.size() != r.nframes || want_off.size() != r.nframes * 8) { printf("frames\n"); return 1; }
    for (uint64_t k = 0; k < r.nframes; ++k) {
        if (r.cls[k] != want_cls[k]) { printf("handler call %llu at %llu: class %u, reference %u\n", (unsigned long long) k, (unsigned long long) r.off[k], r.cls[k], want_cls[k]); return 1; }
        if (memcmp(&r.off[k], want_off.data() + 8 * k, 8)) { printf("handler call %llu: offset\n", (unsigned long long) k); return 1; }
    }
    if (want_msgs.size() != r.nmsgs * 64 || want_frame.size() != r.nmsgs * 8 || want_sig.size() != r.nmsgs * 8) { printf("sizes\n"); return 1; }
    for (uint64_t k = 0; k < r.nmsgs; ++k) {
        if (memcmp(&r.frame_of[k], want_frame.data() + 8 * k, 8)) { printf("message %llu: handler call\n", (unsigned long long) k); return 1; }
        if (memcmp(&r.sig[k], want_sig.data() + 8 * k, 8)) { printf("message %llu (call %llu): signal\n", (unsigned long long) k, (unsigned long long) r.frame_of[k]); return 1; }
        if (memcmp(&r.msgs[k], want_msgs.data() + 64 * k, 64)) {
            const uint8_t *g = (const uint8_t *) &r.msgs[k], *w = want_msgs.data() + 64 * k;
            int at = 0;
            while (g[at] == w[at]) ++at;
            printf("message %llu (call %llu): byte %d is %02x, reference %02x\n", (unsigned long long) k, (unsigned long long) r.frame_of[k], at, g[at], w[at]);
            return 1;
        }
    }
    free(data);
    printf("ok frames %llu msgs %llu skipped %llu past %llu\n", (unsigned long long) r.nframes, (unsigned long long) r.nmsgs, (unsigned long long) r.cn.nskipped,
           (unsigned long long) r.cn.past_end);
    return 0;
}
