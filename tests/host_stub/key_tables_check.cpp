/* key_tables_check.cpp — CPU test of the slicer kernels' syndrome lookup (readsb_amd/csrc/kernels/crc_lookup.inc: key_tables,
 * key_tables_preload, lane_diagnose), compiled for the host AS IT IS: __device__ and __forceinline__ defined away, kBlock handed in
 * by the test (-DK_BLOCK=<kernels.h's value>).  The tables are the ones mgpu_create uploads (build_syndrome_table +
 * pack_syndrome_table of the product library), the block of "LDS" has the size launch_slice asks for (kernels/slice.inc), the preload
 * runs for tid 0 .. kBlock-1 like the workgroup's threads, and then ALL 2^24 syndromes are looked up in both tables for nfix 0, 1
 * and 2 and compared with the host's mgpu_crc_diagnose: hits, misses and bit positions.  That covers what no stream of frames can
 * show — a false hit on a noise syndrome — and every bucket edge of start[] (empty buckets, first and last entry, top byte 0x00 and
 * 0xff, a search that ends at the bucket's end, no table at all).
 *   key_tables_check        prints one line per nfix, exit status 0 when everything agrees */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/modes_gpu.h"
#include "../../readsb_amd/csrc/tables.h"

#define __device__
#define __forceinline__ inline
namespace mgpu {
constexpr int kBlock = K_BLOCK;
#include "../../readsb_amd/csrc/kernels/crc_lookup.inc"
}
using namespace mgpu;

static int check(int nfix) {
    const std::vector<uint64_t> pl = pack_syndrome_table(build_syndrome_table(112, nfix)), ps = pack_syndrome_table(build_syndrome_table(56, nfix));
    const int n_long = (int) pl.size(), n_short = (int) ps.size();
    std::vector<uint64_t> tl(pl), ts(ps);
    tl.push_back(~0ull); ts.push_back(~0ull);                                   /* mgpu_create allocates one entry more: never a null table */
    const size_t words = ((size_t) n_long + n_short + 2 * (kKeyBuckets + 1) + 8) / 2, guard = 64;   /* launch_slice's dynamic LDS */
    std::vector<uint32_t> lds[2];
    for (int pass = 0; pass < 2; ++pass) {                                      /* LDS comes uninitialised: two different fills must give the same tables */
        lds[pass].assign(words + guard, pass ? 0xA5A5A5A5u : 0u);
        for (int tid = 0; tid < kBlock; ++tid) key_tables_preload(lds[pass].data(), tl.data(), n_long, ts.data(), n_short, tid);
        for (size_t g = 0; g < guard; ++g)
            if (lds[pass][words + g] != (pass ? 0xA5A5A5A5u : 0u)) { printf("nfix %d: preload wrote behind the block (word %zu)\n", nfix, words + g); return 1; }
    }
    const size_t used = (size_t) n_long + n_short + 2 * (kKeyBuckets + 1);    /* halfwords */
    if (memcmp(lds[0].data(), lds[1].data(), used * sizeof(uint16_t))) { printf("nfix %d: preload left halfwords unwritten\n", nfix); return 1; }
    const KeyTables kt = key_tables(lds[1].data(), n_long, n_short);
    long bad = 0, hits[2] = {0, 0};
    for (int t = 0; t < 2; ++t) {
        const uint16_t *lo16 = t ? kt.lo_short : kt.lo_long, *start = t ? kt.start_short : kt.start_long;
        const uint64_t *tab = t ? ts.data() : tl.data();
        const int n = t ? n_short : n_long, bits = t ? 56 : 112;
        if (start[0] != 0 || start[kKeyBuckets] != n) { printf("nfix %d bits %d: start[0] = %d, start[256] = %d, n = %d\n", nfix, bits, start[0], start[kKeyBuckets], n); ++bad; }
        for (int h = 0; h < kKeyBuckets; ++h)
            if (start[h] > start[h + 1]) { printf("nfix %d bits %d: start[%d] = %d > start[%d] = %d\n", nfix, bits, h, start[h], h + 1, start[h + 1]); ++bad; }
        for (uint32_t synd = 0; synd < (1u << 24); ++synd) {
            int b0 = 0xff, b1 = 0xff, x = -1, y = -1;
            const int got = lane_diagnose(lo16, start, tab, synd, b0, b1);
            /* syndrome 0 is "no error" on the host and never looked up on the device (classify_frame): it must simply not be an entry */
            const int want = synd == 0 ? -1 : mgpu_crc_diagnose(nfix, synd, bits, &x, &y);
            const bool ok = got == want && (got < 1 || b0 == x) && (got != 2 || b1 == y) && (got != 1 || b1 == 0xff) && (got >= 1 || (b0 == 0xff && b1 == 0xff));
            if (!ok && bad++ < 10) printf("nfix %d bits %d syndrome %06x: lookup %d (%d, %d), host %d (%d, %d)\n", nfix, bits, synd, got, b0, b1, want, x, y);
            if (got >= 1) ++hits[t];
        }
        if (hits[t] != n) { printf("nfix %d bits %d: %ld hits, table has %d entries\n", nfix, bits, hits[t], n); ++bad; }
    }
    printf("nfix %d: long %d entries %ld hits, short %d entries %ld hits, 16777216 syndromes each, %ld differences\n", nfix, n_long, hits[0], n_short, hits[1], bad);
    return bad != 0;
}

int main() {
    int rc = 0;
    for (int nfix = 0; nfix <= 2; ++nfix) rc |= check(nfix);
    return rc;
}
