// snip_mask_check.cpp — TEST INFRASTRUCTURE: the per-word functions of readsb_amd/csrc/snip_mask.h (what kernels/snip.inc computes
// with) against the sequential loop of snipMode (readsb.c:1187-1206) restated on quiet flags.  A program of its own, built with
// -fsanitize=address,undefined by tests/test_snip_reference.py.  Exit 0 and "ok" = every case agrees.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../readsb_amd/csrc/snip_mask.h"

// the reference's loop over quiet flags: keep[k], and the counter behind the last sample
static uint64_t sequential(const std::vector<uint8_t> &quiet, uint64_t c, std::vector<uint8_t> &keep) {
    keep.assign(quiet.size(), 0);
    for (size_t k = 0; k < quiet.size(); ++k) {
        if (quiet[k]) {
            c++;
            if (c > 32) continue;
        } else {
            c = 0;
        }
        keep[k] = 1;
    }
    return c;
}

// the words' way: loud masks, the carry word in front, snip_keep_word per word
static int check_words(const std::vector<uint64_t> &quiet_words, uint64_t c, const char *what) {
    std::vector<uint8_t> quiet, want;
    for (uint64_t w : quiet_words)
        for (int b = 0; b < 64; ++b) quiet.push_back((w >> b) & 1);
    sequential(quiet, c, want);
    uint64_t prev = snip_carry_word(c);
    for (size_t i = 0; i < quiet_words.size(); ++i) {
        const uint64_t loud = ~quiet_words[i], keep = snip_keep_word(prev, loud);
        uint64_t w = 0;
        for (int b = 0; b < 64; ++b) w |= (uint64_t) want[64 * i + b] << b;
        if (keep != w) {
            std::printf("%s: carry %llu word %zu quiet %016llx prev loud %016llx: keep %016llx, the loop keeps %016llx\n", what, (unsigned long long) c, i,
                        (unsigned long long) quiet_words[i], (unsigned long long) prev, (unsigned long long) keep, (unsigned long long) w);
            return 1;
        }
        prev = loud;
    }
    return 0;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {                                        // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main() {
    // every 16-bit pattern x every carry 0..34 on a word pair that is quiet elsewhere (where the dilation decides): the pattern at the
    // call's start, where the carry meets it, and again across the words' boundary
    for (uint64_t pat = 0; pat < 65536; ++pat) {
        const uint64_t q0 = ~(0xffffull | 0xffull << 56) | pat | (pat & 0xff) << 56, q1 = ~0xffull | pat >> 8;
        for (uint64_t c = 0; c <= 34; ++c) {
            uint64_t want[2] = {0, 0}, run = c;
            for (int k = 0; k < 128; ++k) {
                const bool quiet = ((k < 64 ? q0 : q1) >> (k & 63)) & 1;
                run = quiet ? run + 1 : 0;
                if (!quiet || run <= 32) want[k >> 6] |= 1ull << (k & 63);
            }
            const uint64_t k0 = snip_keep_word(snip_carry_word(c), ~q0), k1 = snip_keep_word(~q0, ~q1);
            if (k0 != want[0] || k1 != want[1]) {
                std::printf("pattern %04llx carry %llu: keep %016llx %016llx, the loop keeps %016llx %016llx\n", (unsigned long long) pat, (unsigned long long) c,
                            (unsigned long long) k0, (unsigned long long) k1, (unsigned long long) want[0], (unsigned long long) want[1]);
                return 1;
            }
        }
    }
    // 10^5 random 64-bit words as one stream, bits at densities from mostly loud to mostly quiet, a few large carries
    const uint64_t carries[] = {0, 1, 31, 32, 33, 63, 64, 65, 1ull << 40};
    for (uint64_t c : carries) {
        std::vector<uint64_t> words;
        for (int i = 0; i < 10000; ++i) {
            uint64_t w = rng();
            const int thin = (int) (rng() % 4);                // AND or OR of several words: quiet densities 1/2 .. 1/16 and 1/2 .. 15/16
            for (int t = 0; t < thin; ++t) w = (i & 1) ? w & rng() : w | rng();
            words.push_back(w);
        }
        if (check_words(words, c, "random")) return 1;
    }
    // snip_quiet against abs() in int arithmetic: every byte pair's diagonal and edges at every level that matters and a few beyond
    const int levels[] = {-2147483647 - 1, -5, 0, 1, 2, 3, 64, 127, 128, 129, 130, 1000, 2147483647};
    for (int level : levels) {
        const SnipLevel lv = snip_level(level);
        for (int i = 0; i < 256; ++i)
            for (int q = 0; q < 256; ++q) {
                const int di = i - 127, dq = q - 127;
                const bool want = (di < 0 ? -di : di) < level && (dq < 0 ? -dq : dq) < level;
                if (snip_quiet(lv, (uint32_t) i, (uint32_t) q) != want) {
                    std::printf("quiet: level %d i %d q %d: %d, abs() says %d\n", level, i, q, (int) !want, (int) want);
                    return 1;
                }
            }
    }
    std::puts("ok");
    return 0;
}
