// raw_in_resolve_check.cpp — the PARALLEL rule by which kernels/raw_in.inc settles the ICAO filter's answers, restated in plain C++
// pass by pass, against the sequential walk over the library's model of icao_filter.c (readsb_amd/csrc/icao_filter.h: IcaoFilter), on
// drawn streams: small address pools, random starting generations, table sizes 256 to 1024, 50 to 600 lines.  Every line's verdict and the filter
// afterwards must be equal.  Plain g++, with -fsanitize=address,undefined too.
//   raw_in_resolve_check [streams = 10000] [seed = 1]
// The rule: the filter line i sees is the filter at the start, plus the adders in front of i, minus what the FIRST growth of the table
// drops (icaoFilterResize re-inserts the active generation only, icao_filter.c:65-93; later growths find the other generation empty).
//   first[a]   = the first adder line of address a
//   new add    = an adder line that is first[a] of its address a, a not in the active generation
//   L*         = the line of the k*-th new add, k* = buckets / 3 - occupied + 1 (icao_filter.c:127); none: infinity
//   line i with address a passes iff a is active, or i <= L* and a is inactive, or first[a] < i.
// Afterwards the new adds are replayed, in line order, into the filter.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "icao_filter.h"

struct Line {
    uint32_t addr;
    bool adder, cond;                 // adder: accepted whatever the filter holds, and icaoFilterAdd(addr); cond: accepted iff the filter holds addr
};

int main(int argc, char **argv) {
    const int streams = argc > 1 ? atoi(argv[1]) : 10000;
    std::mt19937_64 rng(argc > 2 ? (uint64_t) atoll(argv[2]) : 1);
    auto draw = [&](uint64_t n) { return (uint32_t) (rng() % n); };
    uint64_t lines_total = 0, grown = 0, dropped_after = 0;
    mgpu::IcaoFilter start, seq, par;                 // (2 x 2^24 bits each: made once, restored per stream)
    for (int s = 0; s < streams; ++s) {
        // a starting filter: a table size, an inactive generation, an active one that leaves room below the growth, and at random
        // entries of addresses >= 2^24 in the active generation: they match no frame, but take buckets and are re-inserted at a growth
        mgpu::IcaoFilter::Snapshot st;
        st.filter_bits = 8 + draw(3);
        const uint32_t third = (1u << st.filter_bits) / 3, pool = 20 + draw(s % 3 == 0 ? 60 : 400), base = 0x400000 + 0x10000 * draw(8);
        const uint32_t n_inactive = draw(pool / 2 + 1), n_active = draw(third < pool ? third : pool);
        std::unordered_set<uint32_t> in_inactive, in_active;
        for (uint32_t k = 0; k < n_inactive; ++k) { const uint32_t a = base + draw(pool); if (in_inactive.insert(a).second) st.members[1].push_back(a); }
        for (uint32_t k = 0; k < n_active; ++k) { const uint32_t a = base + draw(pool); if (in_active.insert(a).second) st.members[0].push_back(a); }
        uint32_t nbig = draw(4) == 0 ? draw(third - (uint32_t) in_active.size() + 1) : 0;
        if (s % 5 == 0) { const uint32_t room = third - (uint32_t) in_active.size(), back = draw(3 < room ? 3 : 1); nbig = room - back; }   // close to the growth
        for (uint32_t k = 0; k < nbig; ++k) st.big[0].push_back(0x01000000u + k);
        st.active = 0;
        st.occupied = (uint32_t) in_active.size() + nbig;
        start.restore(st);
        const uint32_t n = 50 + draw(551);
        std::vector<Line> lines(n);
        for (Line &l : lines) {
            const uint32_t kind = draw(10);
            l.addr = base + draw(pool + 10);
            l.adder = kind < 3;
            l.cond = kind >= 3 && kind < 9;
        }
        lines_total += n;

        // sequential
        seq.restore(st);
        std::vector<uint8_t> want(n);
        for (uint32_t i = 0; i < n; ++i) {
            const Line &l = lines[i];
            want[i] = l.cond ? seq.test(l.addr) : 1;
            if (l.adder) seq.add(l.addr);
        }

        // parallel, pass by pass
        std::unordered_map<uint32_t, uint32_t> first;
        for (uint32_t i = 0; i < n; ++i)
            if (lines[i].adder) { auto it = first.find(lines[i].addr); if (it == first.end() || i < it->second) first[lines[i].addr] = i; }
        std::vector<uint32_t> new_adds;
        const uint64_t buckets = 1ull << start.table_bits();
        const uint64_t kstar = start.table_bits() >= 20 ? 0 : (start.occupied() <= buckets / 3 ? buckets / 3 - start.occupied() + 1 : 1);
        uint64_t lstar = UINT64_MAX;
        for (uint32_t i = 0; i < n; ++i) {
            const Line &l = lines[i];
            if (l.adder && first[l.addr] == i && !start.in_generation(l.addr, true)) {
                new_adds.push_back(l.addr);
                if (new_adds.size() == kstar) lstar = i;
            }
        }
        for (uint32_t i = 0; i < n; ++i) {
            const Line &l = lines[i];
            uint8_t pass = 1;
            if (l.cond) {
                auto it = first.find(l.addr);
                pass = start.in_generation(l.addr, true) || (i <= lstar && start.in_generation(l.addr, false)) || (it != first.end() && it->second < i);
                if (i > lstar && start.in_generation(l.addr, false) && !pass) ++dropped_after;
            }
            if (pass != want[i]) { printf("stream %d line %u: parallel %d, sequential %d\n", s, i, pass, want[i]); return 1; }
        }
        par.restore(st);
        for (uint32_t a : new_adds) par.add(a);
        if (!par.same_as(seq)) { printf("stream %d: the filters differ afterwards\n", s); return 1; }
        grown += lstar != UINT64_MAX;
    }
    printf("ok streams %d lines %llu grown %llu dropped_after_growth %llu\n", streams, (unsigned long long) lines_total, (unsigned long long) grown,
           (unsigned long long) dropped_after);
    return 0;
}
