// stream_passes_check.cpp — the host forms' pass driver (readsb_amd/csrc/stream_passes.h) over a format made up here: lines that end
// in '\n'; a stretch is consumed through its last '\n', its lines are counted, and the sum of their lengths serves as a checksum.  A
// line that starts with '!' is the second policy's stop: the call ends in front of it.  No HIP, no library: plain g++, under ASan and
// UBSan too.  Prints "ok <cases>" and returns 0, or says what failed and returns 1.
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "stream_passes.h"

namespace {

struct Counts {
    uint64_t consumed = 0, lines = 0, sum = 0;
    uint32_t stop = 0;
    bool stopped() const { return stop != 0; }
    void add(const Counts &n) { lines += n.lines; sum += n.sum; stop = n.stop; }
};

// the fake format's one call: [at, at + nb) of text, which starts at a line's start
Counts scan(const std::string &text, uint64_t at, uint64_t nb, bool stops) {
    Counts n;
    uint64_t start = at;
    for (uint64_t p = at; p < at + nb; ++p) {
        if (stops && p == start && text[p] == '!') { n.stop = 1; break; }
        if (text[p] == '\n') { ++n.lines; n.sum += p - start; start = p + 1; }
    }
    n.consumed = start - at;
    return n;
}

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::fprintf(stderr, "FAILED %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } while (0)

unsigned floor_log2(uint64_t x) { unsigned k = 0; while (x >>= 1) ++k; return k; }

// one text at one pass size under one policy; `what` names the case
void drive(const std::string &text, uint64_t pass, bool tail_pass, bool stops, const char *what) {
    const uint64_t len = text.size();
    const Counts want = scan(text, 0, len, stops);
    struct Run { uint64_t at, nb, consumed; bool final, undone, stopped; };
    std::vector<Run> runs;
    int undo_due = 0, undo_stray = 0, repeats = 0;
    Counts all;
    const int rc = mgpu::stream_passes(len, pass, tail_pass, all,
        [&](uint64_t at, uint64_t nb, bool final, const Counts &so_far, Counts &n) -> int {
            if (undo_due) ++undo_stray;                          // a repeat without its undo
            CHECK(nb > 0 && at + nb <= len && final == (at + nb == len), "%s pass %llu: stretch [%llu, +%llu) final %d of %llu", what, (unsigned long long) pass,
                  (unsigned long long) at, (unsigned long long) nb, (int) final, (unsigned long long) len);
            CHECK(so_far.consumed == at, "%s pass %llu: the sum stands at %llu, the stretch at %llu", what, (unsigned long long) pass, (unsigned long long) so_far.consumed,
                  (unsigned long long) at);
            CHECK(n.consumed == 0 && n.lines == 0 && n.stop == 0, "%s: a pass's counts do not start fresh", what);
            n = scan(text, at, nb, stops);
            runs.push_back({at, nb, n.consumed, final, false, n.stopped()});
            if (n.consumed == 0 && !n.stopped() && !final) undo_due = 1;
            return 0;
        },
        [&] {
            if (undo_due == 1 && !runs.empty()) { undo_due = 0; runs.back().undone = true; ++repeats; }
            else ++undo_stray;
        });
    CHECK(rc == 0, "%s pass %llu: rc %d", what, (unsigned long long) pass, rc);
    CHECK(undo_due == 0 && undo_stray == 0, "%s pass %llu: undo must run exactly once before each repeat and never otherwise", what, (unsigned long long) pass);
    // the totals of one call over the whole text
    CHECK(all.lines == want.lines && all.sum == want.sum && all.consumed == want.consumed && all.stop == want.stop,
          "%s pass %llu: lines %llu/%llu sum %llu/%llu consumed %llu/%llu stop %u/%u", what, (unsigned long long) pass, (unsigned long long) all.lines,
          (unsigned long long) want.lines, (unsigned long long) all.sum, (unsigned long long) want.sum, (unsigned long long) all.consumed, (unsigned long long) want.consumed,
          all.stop, want.stop);
    // the committed stretches are contiguous from 0; a repeat starts where the undone one did, twice as long or to the end
    uint64_t at = 0;
    for (size_t k = 0; k < runs.size(); ++k) {
        CHECK(runs[k].at == at, "%s pass %llu: run %zu starts at %llu, not %llu", what, (unsigned long long) pass, k, (unsigned long long) runs[k].at, (unsigned long long) at);
        if (runs[k].undone) {
            CHECK(k + 1 < runs.size() && (runs[k + 1].nb == 2 * runs[k].nb || runs[k + 1].final), "%s pass %llu: run %zu is not repeated twice as long", what,
                  (unsigned long long) pass, k);
        } else at += runs[k].consumed;
    }
    CHECK(at == want.consumed, "%s pass %llu: committed to %llu of %llu", what, (unsigned long long) pass, (unsigned long long) at, (unsigned long long) want.consumed);
    if (len) CHECK(repeats <= (int) floor_log2(len) + 1, "%s pass %llu: %d repeats for %llu bytes", what, (unsigned long long) pass, repeats, (unsigned long long) len);
    if (len == 0) { CHECK(runs.empty(), "%s: a run over nothing", what); return; }
    if (pass == 0 || pass >= len) CHECK(runs[0].nb == len && repeats == 0, "%s pass %llu: not the whole text at once", what, (unsigned long long) pass);
    // how the passes end: at a stop with nothing behind it; with the tail pass, by a stretch that consumed all or a last one that consumed
    // nothing; without it, by the first stretch that reaches the end of the text
    const Run &last = runs.back();
    if (want.stop) {
        size_t stopped = 0;
        for (const Run &r : runs) stopped += r.stopped;
        CHECK(last.stopped && stopped == 1 && last.at + last.consumed == want.consumed, "%s pass %llu: a run behind the stop", what, (unsigned long long) pass);
    } else if (tail_pass) {
        CHECK(last.final && (last.at + last.consumed == len || last.consumed == 0), "%s pass %llu: the tail was not looked at once more", what, (unsigned long long) pass);
        if (want.consumed && want.consumed < len)
            CHECK(last.at == want.consumed && last.consumed == 0, "%s pass %llu: no pass over the tail alone", what, (unsigned long long) pass);
    } else {
        size_t finals = 0;
        for (const Run &r : runs) finals += r.final;
        CHECK(last.final && finals == 1, "%s pass %llu: %zu stretches reached the end", what, (unsigned long long) pass, finals);
    }
}

}  // namespace

int main() {
    std::vector<std::pair<const char *, std::string>> texts;
    texts.push_back({"empty", ""});
    texts.push_back({"no newline", std::string(50, 'a')});
    texts.push_back({"only newlines", std::string(40, '\n')});
    uint64_t seed = 12345;
    auto rnd = [&] { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (seed >> 33); };
    std::string lines;
    for (int k = 0; k < 300; ++k) lines += std::string(rnd() % 301, (char) ('a' + k % 26)) + "\n";
    texts.push_back({"random lines, ends with a newline", lines});
    texts.push_back({"random lines, ends without", lines + std::string(77, 'z')});
    std::string one = "ab\ncde\n\nf\n";
    texts.push_back({"one long line", one + std::string(5 * one.size(), 'L') + "\ngh\n"});
    // the stop policy's texts: a '!' line in the middle, at the very start, behind the long line
    std::vector<std::pair<const char *, std::string>> stops;
    stops.push_back({"stop in the middle", lines.substr(0, lines.size() / 2) + (lines[lines.size() / 2 - 1] == '\n' ? "" : "\n") + "!stop\n" + lines.substr(lines.size() / 2)});
    stops.push_back({"stop at the start", "!stop\n" + one});
    stops.push_back({"stop behind the long line", std::string(700, 'L') + "\n!stop\nab\n"});
    stops.push_back({"no stop at all", lines});

    int cases = 0;
    auto all_passes = [&](const std::string &text, bool tail_pass, bool with_stops, const char *what) {
        const uint64_t len = text.size();
        std::vector<uint64_t> passes = {0, 1, 2, 3, 7, 255, 256, len, len + 1};
        if (len) passes.push_back(len - 1);
        for (uint64_t pass : passes) { drive(text, pass, tail_pass, with_stops, what); ++cases; }
    };
    for (const auto &t : texts) {
        all_passes(t.second, true, false, t.first);                // the line formats' policy
        all_passes(t.second, false, false, t.first);               // ... and the policy that ends with the stream, without a stop
    }
    for (const auto &t : stops) {
        Counts probe = scan(t.second, 0, t.second.size(), true);
        if (t.first[0] == 's') CHECK(probe.stop == 1 && probe.consumed < t.second.size(), "%s: the text has no stop", t.first);
        all_passes(t.second, false, true, t.first);                // the beast policy: a counts type with a stop code
    }
    if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
    std::printf("ok %d\n", cases);
    return 0;
}
