// kernels/crc_lookup.inc — the slicer kernels' syndrome lookup: the two-level key tables in LDS, their workgroup-wide preload and the
// per-lane search.  Part of the single translation unit kernels.hip (included from kernels/slicer.inc, inside namespace mgpu).
// Plain C++ apart from the __device__ __forceinline__ qualifiers and kBlock (kernels.h): tests/host_stub/key_tables_check.cpp compiles
// this file as it is for the host and looks up all 2^24 syndromes in it.

// per-lane modesChecksumDiagnose (crc.c:383-406): the sorted syndromes are staged in LDS (a miss — the common case for noise —
// never touches global memory; dependent global loads under a streaming kernel cost thousands of cycles each); a hit fetches the
// packed entry (syndrome<<16 | bit0<<8 | bit1) from the global table.
// In LDS a table is two levels: start[h] = index of the first syndrome whose top byte is >= h (257 entries), and the syndromes' low
// 16 bits.  Half the bytes of 32-bit keys — the 2-bit tables of --aggressive (3831 + 1326 syndromes) take 12.4 KB instead of 20.6,
// which is the difference between two and three workgroups of k_slice per CU — and a search of ~4 steps inside a bucket of ~20
// instead of 12 over the whole table.
constexpr int kKeyBuckets = 256;
struct KeyTables {                       // views into the dynamic LDS block: [lo16 long | lo16 short | start long | start short]
    const uint16_t *lo_long, *lo_short, *start_long, *start_short;
};
__device__ __forceinline__ KeyTables key_tables(const uint32_t *dyn_lds, int n_long, int n_short) {
    const uint16_t *b = (const uint16_t *) dyn_lds;
    return KeyTables{b, b + n_long, b + n_long + n_short, b + n_long + n_short + kKeyBuckets + 1};
}
// workgroup-wide preload (before the kernel's first barrier): every thread takes the entries tid, tid + kBlock, ...
__device__ __forceinline__ void key_tables_preload(uint32_t *dyn_lds, const uint64_t *tab_long, int n_long, const uint64_t *tab_short, int n_short, int tid) {
    uint16_t *b = (uint16_t *) dyn_lds;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint64_t *tab = t ? tab_short : tab_long;
        const int n = t ? n_short : n_long;
        uint16_t *lo = b + (t ? n_long : 0), *start = b + n_long + n_short + (t ? kKeyBuckets + 1 : 0);
        for (int i = tid; i < n; i += kBlock) {
            const uint32_t key = (uint32_t) (tab[i] >> 16);                       // 24 bits
            lo[i] = (uint16_t) key;
            // the buckets that begin at i: those above the previous syndrome's top byte up to this one's
            const int h1 = (int) (key >> 16), h0 = i ? (int) ((uint32_t) (tab[i - 1] >> 16) >> 16) + 1 : 0;
            for (int h = h0; h <= h1; ++h) start[h] = (uint16_t) i;
        }
        // ... and the ones behind the last syndrome's
        const int hl = n ? (int) ((uint32_t) (tab[n - 1] >> 16) >> 16) + 1 : 0;
        for (int h = hl + tid; h <= kKeyBuckets; h += kBlock) start[h] = (uint16_t) n;
    }
}
__device__ __forceinline__ int lane_diagnose(const uint16_t *lo16, const uint16_t *start, const uint64_t *tab, uint32_t synd, int &b0, int &b1) {
    const uint32_t h = (synd >> 16) & 0xffu;
    const uint16_t want = (uint16_t) synd;
    int lo = start[h], hi = start[h + 1];
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lo16[mid] < want) lo = mid + 1; else hi = mid;
    }
    if (lo >= end || lo16[lo] != want) return -1;
    const uint64_t e = tab[lo];
    b0 = (int) ((e >> 8) & 0xff);
    b1 = (int) (e & 0xff);
    return b1 == 0xff ? 1 : 2;
}
