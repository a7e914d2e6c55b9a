// snip_mask.h — the per-word decision of `readsb --snip` (snipMode, readsb.c:1187-1206), shared by kernels/snip.inc and the host
// (tests/host_stub/snip_mask_check.cpp checks it against the reference's sequential loop).
//
// The stream is cut into words of 64 samples, bit k of a word = sample k of it.  A word's `loud` mask has a bit per sample that is
// NOT quiet.  The reference keeps a quiet sample iff it is among the first 32 of its quiet run, that is iff one of the 32 samples
// before it is loud: keep = the loud mask dilated upwards by 32 positions, with the word before supplying the bits that shift in.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SNIP_HD __host__ __device__ inline
#else
#define SNIP_HD inline
#endif

constexpr int kSnipRun = 32;                                  // MODES_PREAMBLE_SIZE (readsb.h:118-120)

// keep mask of a word from its loud mask and the loud mask of the word before it: OR of (prev:cur) << j for j = 0..32, by doubling
SNIP_HD uint64_t snip_keep_word(uint64_t loud_prev, uint64_t loud_cur) {
    uint64_t lo = loud_prev, hi = loud_cur;
    for (int s = 1; s < kSnipRun; s <<= 1) {                  // j = 0..31 after shifts by 1, 2, 4, 8, 16
        hi |= (hi << s) | (lo >> (64 - s));
        lo |= lo << s;
    }
    return hi | (hi << 1) | (lo >> 63);                       // ... and j = 32
}

// the loud mask that stands in for "the word before" at the start of a call: the reference's counter c says the c samples before
// the call were quiet and the one before them was not
SNIP_HD uint64_t snip_carry_word(uint64_t quiet_run) {
    return quiet_run >= 64 ? 0ull : ~0ull >> quiet_run;
}

// quiet(k) = |i - 127| < level && |q - 127| < level for every int level, as one unsigned compare per byte:
// |b - 127| < level  <=>  b in [128 - level, 126 + level]  <=>  (unsigned)(b - lo) < width, lo = 128 - level, width = 2 * level - 1,
// with level clamped to 0 (nothing is quiet: width 0) .. 129 (everything is: lo -1, width 257)
struct SnipLevel {
    int32_t lo;
    uint32_t width;
};
SNIP_HD SnipLevel snip_level(int32_t level) {
    const int32_t l = level < 0 ? 0 : level > 129 ? 129 : level;
    return {128 - l, l ? (uint32_t) (2 * l - 1) : 0u};
}
SNIP_HD bool snip_quiet(SnipLevel v, uint32_t i, uint32_t q) {
    return (uint32_t) ((int32_t) i - v.lo) < v.width && (uint32_t) ((int32_t) q - v.lo) < v.width;
}
