// beast_in_format_check.cpp — the beast input's framer and parser (readsb_amd/csrc/beast_in_format.h) and the sequential walk
// (beast_in_host.cpp: beast_in_decode_sequential over icao_filter.h's IcaoFilter) on the host against what the REFERENCE left for a
// stream (tests/golden/beast_in_cases.npz, written out by tests/beast_in_util.py's callers).  Plain g++, with
// -fsanitize=address,undefined too; the stream is walked in a heap copy of exactly its bytes, so that a read at or beyond nbytes is an error.
//   beast_in_format_check <stream.bin> <now_ms> <nfix_crc> <fixDF> <mode_ac> <net_ingest> <receiver_id_in> <filter.bin> <head.bin> <class.bin> <off.bin>
//                         <frame_of.bin> <ids.bin> <signal.bin> <msgs.bin>
// filter.bin: int32 values, >= 0 icaoFilterAdd(value), -1 icaoFilterExpire().  Prints "ok frames F msgs M" or the first difference.
//   beast_in_format_check prefixes <stream.bin> <now_ms> <nfix_crc> <fixDF> <mode_ac> <net_ingest>
// every prefix of the stream, each in a heap copy of exactly its bytes: the sequential walk against a walk over
// mgpu_beast_parse_host alone, step by step (consumed, stop, garbage, handler calls, ids, commands), and what holds of any result
// (consumed <= nbytes; every handler call's offset ascending and below consumed).  Prints "ok prefixes N".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "beast_in_host.h"

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
    std::vector<uint64_t> ids, frame_of, off;
    std::vector<double> sig;
    std::vector<uint8_t> cls;
    uint64_t consumed = 0, nframes = 0, nmsgs = 0, stop_off = 0, id_out = 0;
    uint32_t stop = 0;
    mgpu_beast_in_counters cn;
};

static int run(const uint8_t *data, uint64_t n, int64_t now, const mgpu_raw_in_config &cfg, uint32_t net_ingest, uint64_t id_in, mgpu::IcaoFilter &flt, Result &r) {
    const uint64_t cap = mgpu::beast_in_max_msgs(n), fcap = mgpu::beast_in_max_frames(n);
    r.msgs.resize(cap); r.ids.resize(cap); r.frame_of.resize(cap); r.sig.resize(cap); r.cls.resize(fcap); r.off.resize(fcap);
    mgpu_beast_in_args a;
    memset(&a, 0, sizeof a);
    a.size = sizeof a; a.data = data; a.nbytes = n; a.now_ms = now; a.receiver_id_in = id_in; a.net_ingest = net_ingest;
    a.msgs = r.msgs.data(); a.receiver_id = r.ids.data(); a.signal_level = r.sig.data(); a.frame_of = r.frame_of.data(); a.msgs_cap = cap;
    a.frame_class = r.cls.data(); a.frame_off = r.off.data(); a.frames_cap = fcap;
    a.consumed = &r.consumed; a.nframes = &r.nframes; a.nmsgs = &r.nmsgs; a.stop = &r.stop; a.stop_off = &r.stop_off; a.receiver_id_out = &r.id_out; a.counters = &r.cn;
    return mgpu::beast_in_decode_sequential(&a, &cfg, flt);
}

static int check_prefixes(int argc, char **argv) {
    if (argc != 8) { fprintf(stderr, "usage\n"); return 2; }
    const std::vector<uint8_t> stream = slurp(argv[2]);
    const int64_t now = atoll(argv[3]);
    const mgpu_raw_in_config cfg = {sizeof cfg, atoi(argv[4]), atoi(argv[5]), (uint32_t) atoi(argv[6])};
    const mgpu_beast_in_config pcfg = {sizeof pcfg, cfg.nfix_crc, cfg.fixDF, cfg.mode_ac, (uint32_t) atoi(argv[7]), 0};
    for (size_t n = 0; n <= stream.size(); ++n) {
        uint8_t *copy = (uint8_t *) malloc(n ? n : 1);
        memcpy(copy, stream.data(), n);
        mgpu::IcaoFilter flt;
        Result r;
        const int rc = run(copy, n, now, cfg, pcfg.net_ingest, 7, flt, r);
        if (rc != MGPU_OK) { printf("prefix %zu: %d\n", n, rc); return 1; }
        // the plain walk over mgpu_beast_parse_host
        uint64_t som = 0, pending = 0, garbage = 0, frames = 0, ids = 0, cmds = 0, id = 7;
        uint32_t stop = MGPU_BEAST_STOP_END;
        bool left = false;
        while (som < n) {
            mgpu_beast_in_frame f;
            const int one = mgpu_beast_parse_host(copy, n, som, now, &pcfg, &f);
            if (one < 0) { printf("prefix %zu: parse at %llu gives %d\n", n, (unsigned long long) som, one); return 1; }
            if (f.step == MGPU_BEAST_STEP_GARBAGE) { ++pending; som = f.next; continue; }
            if (f.next < som || f.next > n || f.next - som > mgpu::kBeastInMaxFrame) { printf("prefix %zu: step at %llu goes to %llu\n", n, (unsigned long long) som, (unsigned long long) f.next); return 1; }
            garbage += pending + f.garbage; pending = 0;
            if (f.id_set) { ++ids; id = f.receiver_id; }
            cmds += f.command;
            const uint64_t at = som;
            som = f.next;
            if (f.step == MGPU_BEAST_STEP_INCOMPLETE) { left = true; break; }
            if (f.step == MGPU_BEAST_STEP_SYNTH || f.step == MGPU_BEAST_STEP_UUID) { left = true; stop = f.step == MGPU_BEAST_STEP_SYNTH ? MGPU_BEAST_STOP_SYNTH : MGPU_BEAST_STOP_UUID; break; }
            if (som <= at) { printf("prefix %zu: no progress at %llu\n", n, (unsigned long long) at); return 1; }
            if (f.step == MGPU_BEAST_STEP_FRAME) {
                if (frames >= r.nframes || r.off[frames] != f.frame_off || f.frame_off < at || f.frame_off >= som) { printf("prefix %zu: handler call %llu\n", n, (unsigned long long) frames); return 1; }
                const uint32_t c = r.cls[frames];
                if (!(f.cls == c || (f.cls == MGPU_BEAST_IN_COND && (c == MGPU_BEAST_IN_ACCEPT || c == MGPU_BEAST_IN_UNKNOWN)))) { printf("prefix %zu: class of call %llu\n", n, (unsigned long long) frames); return 1; }
                ++frames;
            }
        }
        if (!left) som = n - pending;
        if (stop == MGPU_BEAST_STOP_END && n - som > mgpu::kBeastInTail) { garbage += n - som; som = n; }
        if (som != r.consumed || stop != r.stop || r.stop_off != r.consumed || garbage != r.cn.remote_malformed_beast || frames != r.nframes || ids != r.cn.nreceiver_ids ||
            cmds != r.cn.ncommands || id != r.id_out || r.consumed > n) {
            printf("prefix %zu: walk consumed %llu stop %u garbage %llu frames %llu, resolver %llu %u %llu %llu\n", n, (unsigned long long) som, stop, (unsigned long long) garbage,
                   (unsigned long long) frames, (unsigned long long) r.consumed, r.stop, (unsigned long long) r.cn.remote_malformed_beast, (unsigned long long) r.nframes);
            return 1;
        }
        free(copy);
    }
    printf("ok prefixes %zu\n", stream.size() + 1);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "prefixes")) return check_prefixes(argc, argv);
    if (argc != 16) { fprintf(stderr, "usage\n"); return 2; }
    const std::vector<uint8_t> stream = slurp(argv[1]);
    const int64_t now = atoll(argv[2]);
    const mgpu_raw_in_config cfg = {sizeof cfg, atoi(argv[3]), atoi(argv[4]), (uint32_t) atoi(argv[5])};
    const uint32_t net_ingest = (uint32_t) atoi(argv[6]);
    const uint64_t id_in = strtoull(argv[7], nullptr, 0);
    const std::vector<uint8_t> fops = slurp(argv[8]), head_b = slurp(argv[9]), want_cls = slurp(argv[10]), want_off = slurp(argv[11]), want_frame = slurp(argv[12]),
                               want_ids = slurp(argv[13]), want_sig = slurp(argv[14]), want_msgs = slurp(argv[15]);
    if (head_b.size() != 96) { printf("head\n"); return 1; }
    uint64_t head[12];
    memcpy(head, head_b.data(), 96);
    mgpu::IcaoFilter flt;
    for (size_t k = 0; k + 4 <= fops.size(); k += 4) {
        int32_t op;
        memcpy(&op, fops.data() + k, 4);
        if (op >= 0) flt.add((uint32_t) op); else flt.expire();
    }
    uint8_t *data = (uint8_t *) malloc(stream.size() ? stream.size() : 1);
    memcpy(data, stream.data(), stream.size());
    Result r;
    const int rc = run(data, stream.size(), now, cfg, net_ingest, id_in, flt, r);
    if (rc != MGPU_OK) { printf("beast_in_decode_sequential %d\n", rc); return 1; }
    const uint64_t got[12] = {r.consumed, r.nframes, r.nmsgs, r.cn.remote_received_modes, r.cn.remote_received_modeac, r.cn.remote_rejected_unknown_icao, r.cn.remote_rejected_bad,
                              r.cn.remote_accepted[0], r.cn.remote_accepted[1], r.cn.remote_accepted[2], r.cn.remote_malformed_beast, r.id_out};
    int bad = 0;
    for (int k = 0; k < 12; ++k)
        if (got[k] != head[k]) { printf("count %d: reference %llu, here %llu\n", k, (unsigned long long) head[k], (unsigned long long) got[k]); bad = 1; }
    if (bad || r.stop != MGPU_BEAST_STOP_END) return 1;
    if (want_cls.size() != r.nframes || want_off.size() != r.nframes * 8) { printf("frames\n"); return 1; }
    for (uint64_t k = 0; k < r.nframes; ++k) {
        if (r.cls[k] != want_cls[k]) { printf("handler call %llu at %llu: class %u, reference %u\n", (unsigned long long) k, (unsigned long long) r.off[k], r.cls[k], want_cls[k]); return 1; }
        if (memcmp(&r.off[k], want_off.data() + 8 * k, 8)) { printf("handler call %llu: offset\n", (unsigned long long) k); return 1; }
    }
    if (want_msgs.size() != r.nmsgs * 64 || want_frame.size() != r.nmsgs * 8 || want_sig.size() != r.nmsgs * 8 || want_ids.size() != r.nmsgs * 8) { printf("sizes\n"); return 1; }
    for (uint64_t k = 0; k < r.nmsgs; ++k) {
        if (memcmp(&r.frame_of[k], want_frame.data() + 8 * k, 8)) { printf("message %llu: handler call\n", (unsigned long long) k); return 1; }
        if (memcmp(&r.ids[k], want_ids.data() + 8 * k, 8)) { printf("message %llu (call %llu): receiver id\n", (unsigned long long) k, (unsigned long long) r.frame_of[k]); return 1; }
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
    printf("ok frames %llu msgs %llu\n", (unsigned long long) r.nframes, (unsigned long long) r.nmsgs);
    return 0;
}
