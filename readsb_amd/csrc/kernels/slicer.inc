// kernels/slicer.inc — device code shared by the slicer kernels: slicer geometry, the five correlators, CRC diagnose,
// frame classification, adder publish.
// Part of the single translation unit kernels.hip (included inside namespace mgpu, after the parts before it).

// Frame bit k of try-phase t uses correlator row (t + 2k) % 5 at sample pa + 19 + t/5 +
// (t%5 + 12k)/5 (closed form of slice_byte, demod_2400.c:133-213).  With k = 5g + i the row is
// (p + 2i) % 5, p = t % 5, so inside every group of five bits each row is used exactly once:
// iterating rows 0..4 (compile-time coefficients) visits bit i_r = 3(r - p) mod 5 of the group at
// sample offset 12g + (p + 12 i_r)/5.

// Publish "a clean DF17 / DF11-IID0 frame of this stream carries `addr`" (mode_s.c:766-779) in the
// 2^24-bit adder bitmap.  Device-scope RMWs execute at the memory side (the 8 XCD L2s are not
// coherent with each other) and serialise per address; a few hundred aircraft addresses are hit
// millions of times, and sending every sighting doubled the sweep kernel's run time.  So: a
// direct-mapped LDS cache of what this workgroup already published, and — bits are only ever
// set — a look (agent-scope load) before the RMW.
template <int CACHE>
__device__ __forceinline__ void adder_publish(uint32_t *bitmap, uint32_t *cache, uint32_t addr) {
    const uint32_t h = (addr ^ (addr >> 10) ^ (addr >> 17)) & (CACHE - 1);
    if (cache[h] == addr) return;
    cache[h] = addr;
    const uint32_t bit = 1u << (addr & 31);
    if (!(__hip_atomic_load(&bitmap[addr >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(&bitmap[addr >> 5], bit);
}


struct SliceGeom {          // per lane, derived from the try-phase
    int wi[5];              // dword index (into the LDS tile viewed as u32) of the even sample at or below row r's first tap
    int par[5];             // 0 / 16: first tap is the low / high half of that dword
    int sh[5];              // position (4 - i_r) of row r's bit inside the 5-bit group value
};

__device__ __forceinline__ void make_geom(int pos_local, int t, SliceGeom &g) {
    const int p = t % 5;
    const int base = pos_local + 19 + t / 5;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        int i = (r - p + 5) * 3;
        i -= (i / 5) * 5;
        const int s = base + (p + 12 * i) / 5;
        g.wi[r] = s >> 1;
        g.par[r] = (s & 1) * 16;
        g.sh[r] = 4 - i;
    }
}

// k_slice's form of the same (generation 6).  The closed form above costs ~80 instructions per lane — three divisions by five per
// row — and the slicer evaluates it for every (candidate, phase) pair and every lane of every slicing round; and placing row r's bit
// at 4 - i_r costs a shift by a register per row.  Instead: a ten-word table (one row of two words per try-phase 4..8, built once
// per workgroup), and the rows' sign bits are collected in the FIXED order 0, 2, 4, 1, 3 (X = b0 b2 b4 b1 b3, one v_alignbit
// each) — frame bit i of the group sits at row p + 2i = 2 (i + 3p) mod 5, i.e. at place (i + 3p) mod 5 of that order, so the
// group value is X rotated by 3p mod 5 places: (X | X << 5) >> (5 - 3p mod 5) & 31, two instructions.
//   word 0: per row r the sample offset of its first tap from the scan position, six bits each; word 1: the rotation 5 - 3p mod 5
typedef const __attribute__((address_space(3))) uint32_t *lds_u32p;   // (an explicit LDS address: 32 bits, ds_read)
struct SliceGeomR {
    lds_u32p pw[5];        // LDS address of the dword holding row r's first tap (the tile viewed as u32), of the lane's first group
    int par[5];             // as SliceGeom (only bits 0..4 count: the shifts take them modulo 32)
    int rot;                // 1..5
};
__device__ __forceinline__ void geom_table_row(int t, uint32_t &w0, uint32_t &w1) {
    SliceGeom g;
    make_geom(0, t, g);
    w0 = 0;
#pragma unroll
    for (int r = 0; r < 5; ++r) w0 |= (uint32_t) (2 * g.wi[r] + g.par[r] / 16) << (6 * r);
    w1 = (uint32_t) (5 - (3 * (t % 5)) % 5);
}
// g0 = the lane's first group (0 for the DF stage): the addresses are formed once, the groups behind are immediate offsets
__device__ __forceinline__ void make_geom_tab(const uint32_t *tab, const uint32_t *w32, int pos_local, int ti /* try-phase - 4 */, int g0, SliceGeomR &g) {
    const uint32_t w0 = tab[2 * ti];
    g.rot = (int) tab[2 * ti + 1];
    const int base = pos_local + 12 * g0;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int s = base + (int) ((w0 >> (6 * r)) & 63u);
        g.pw[r] = (lds_u32p) w32 + (s >> 1);
        g.par[r] = s << 4;
        asm volatile("" : "+v"(g.pw[r]));       // (kept as an address: the compiler otherwise re-forms it from the index for every group)
    }
}

// The correlators' first-tap coefficients, NEGATED (see THE BIAS ARITHMETIC below), pinned in VGPRs: the three-operand v_dot2_i32_i16 takes
// no literal, and the two-operand v_dot2c the compiler prefers needs its accumulator zeroed by a v_mov per row and group.
struct SliceCoef { uint32_t k0a, k1a, k2a, k3a, k4a, init2; };
__device__ __forceinline__ SliceCoef slice_coef() {
    SliceCoef K = {0x000fffeeu /* {-18, 15} */, 0x0005fff2u /* {-14, 5} */, 0xfffbfff0u /* {-16, -5} */, 0xfff5fff9u /* {-7, -11} */,
                   0xfff1fffcu /* {-4, -15} */, 0xffff8000u /* -32768: row 2's threshold */};
    asm volatile("" : "+v"(K.k0a), "+v"(K.k1a), "+v"(K.k2a), "+v"(K.k3a), "+v"(K.k4a), "+v"(K.init2));
    return K;
}
__device__ __forceinline__ int dot_first(uint32_t x, uint32_t k) {
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(d) : "v"(x), "v"(k));
    return d;
}
__device__ __forceinline__ int dot_first(uint32_t x, uint32_t k, uint32_t init) {
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(x), "v"(k), "v"(init));
    return d;
}
// five bits of a frame starting gw dwords behind the geometry's group 0 (see THE BIAS ARITHMETIC below)
__device__ __forceinline__ uint32_t slice_group_rot(const SliceGeomR &g, int gw, const SliceCoef &K) {
    uint32_t a[5], b[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) { a[r] = g.pw[r][gw]; b[r] = g.pw[r][gw + 1]; }
    const uint32_t c4 = g.pw[4][gw + 2];
    __builtin_amdgcn_sched_barrier(0);          // keep the loads above, the arithmetic below
    const v2i16 k0b = {3, 0}, k1b = {9, 0}, k2b = {20, 0}, k3b = {18, 0}, k4b = {20, -1};
#define PK01(R) __builtin_amdgcn_alignbit(b[R], a[R], g.par[R])                               /* taps 0, 1 */
#define PK2(R) __builtin_bit_cast(v2i16, __builtin_amdgcn_alignbit(0u, b[R], g.par[R]))      /* tap 2 in the low half (a shift modulo 32) */
    const int s0 = __builtin_amdgcn_sdot2(PK2(0), k0b, dot_first(PK01(0), K.k0a), false);
    const int s1 = __builtin_amdgcn_sdot2(PK2(1), k1b, dot_first(PK01(1), K.k1a), false);
    const int s2 = __builtin_amdgcn_sdot2(PK2(2), k2b, dot_first(PK01(2), K.k2a, K.init2), false);
    const int s3 = __builtin_amdgcn_sdot2(PK2(3), k3b, dot_first(PK01(3), K.k3a), false);
    const v2i16 y4 = __builtin_bit_cast(v2i16, __builtin_amdgcn_alignbit(c4, b[4], g.par[4]));   // taps 2, 3
    const int s4 = __builtin_amdgcn_sdot2(y4, k4b, dot_first(PK01(4), K.k4a), false);
#undef PK01
#undef PK2
    uint32_t X = (uint32_t) s0 >> 31;
    X = __builtin_amdgcn_alignbit(X, (uint32_t) s2, 31);     // (X << 1) | sign
    X = __builtin_amdgcn_alignbit(X, (uint32_t) s4, 31);
    X = __builtin_amdgcn_alignbit(X, (uint32_t) s1, 31);
    X = __builtin_amdgcn_alignbit(X, (uint32_t) s3, 31);
    return __builtin_amdgcn_ubfe((X << 5) | X, (uint32_t) g.rot, 5u);
}

// ---- generation 7 of the slicing rounds' inner step: one WINDOW of seven dwords per group, per-lane coefficients ----
// slice_group_rot reads eleven dwords per group (five rows x the dword pair holding the row's taps, + one) out of the seven
// distinct ones the group's 14 samples lie in, and spends ten v_alignbit on bringing every row's taps to the front of a register
// pair.  Measured (profiles/r04_pmc_sq_summary.txt): during the slicing rounds the CU's LDS pipe, not the VALUs, is what the
// waves queue on — 7 LDS instructions per group at ~8 cycles each (half of them bank conflicts) against 30 VALU / 4 SIMDs.
// Here a lane walks its consecutive groups as ONE stream of dwords: group g of the lane is dwords 6g .. 6g + 6 behind the even
// sample at or below the lane's first tap (six new dwords per group, three ds_read2_b32, requested one group ahead), and the
// alignment moves from the data into the COEFFICIENTS: iterate the group's bits i = 0..4 (not the rows), bit i's 3-4 taps start
// at sample x_i = e + floor((p + 12 i) / 5) of the window (e = parity of the frame's first data sample, p = try-phase mod 5) and
// — checked for all 10 (phase, e) combinations, tools/dev_check.py slicer-window — always lie inside dwords i, i+1, i+2.  So
//     S_i = init_i + dot2(w[i], K[i][0]) + dot2(w[i+1], K[i][1]) + dot2(w[i+2], K[i][2]),   bit i = S_i < 0
// with the row's (negated) coefficients placed in the halves of K[i][0..2] where its taps fall, zeros elsewhere, and init_i =
// -32768 for the bit that uses row 2 (see THE BIAS ARITHMETIC below): 15 v_dot2 per group, no v_alignbit, the
// bits arrive in frame order (no rotation), and a lane's 15 + 5 constants come from a 10-row table in LDS (one row per (phase,
// e), five 16-byte reads per lane and round).  4 LDS + 23 VALU instructions per group (was 7 + 30).
constexpr int kWcRowWords = 28;          // 15 coefficient words, 5 accumulator starts; rows 112 bytes apart (16-byte aligned, and rows 0..7 start in eight different bank groups)
constexpr int kWcRows = 10;              // (try-phase 4..8) x e
__device__ __constant__ const signed char kCorrTaps[5][4] = {{18, -15, -3, 0}, {14, -5, -9, 0}, {16, 5, -20, 0}, {7, 11, -18, 0}, {4, 15, -20, 1}};   // slice_phase0..4, demod_2400.c:74-93
// The slicing rounds' deal of the wave's lanes to n waiting frames (1 .. 32): I = the fewest groups per lane of a 112-bit frame
// for which n * ceil(22 / I) lanes fit the wave, L = ceil(22 / I) lanes per frame, Is = ceil(11 / L) groups per lane of a 56-bit
// frame: I | Is << 4 | L << 8 | ceil(65536 / L) << 16 (lane * that >> 16 = lane / L for lane < 64).
__device__ inline uint32_t round_table_row(int n) {
    if (n < 1) n = 1;
    int I = 1;
    while (n * ((22 + I - 1) / I) > WAVE) ++I;
    const int L = (22 + I - 1) / I, Is = (11 + L - 1) / L;
    return (uint32_t) I | ((uint32_t) Is << 4) | ((uint32_t) L << 8) | ((uint32_t) ((65536 + L - 1) / L) << 16);
}

__device__ inline void wcoef_table_row(int row, uint32_t *out) {            // one thread per row, once per workgroup
    const int p = (4 + (row >> 1)) % 5, e = row & 1;
    for (int k = 0; k < kWcRowWords; ++k) out[k] = 0;
    for (int i = 0; i < 5; ++i) {
        const int r = (p + 2 * i) % 5, x = e + (p + 12 * i) / 5;
        for (int j = 0; j < 4; ++j) {
            const int c = kCorrTaps[r][j];
            if (c == 0) continue;                                              // (the fourth tap of a three-tap row)
            const uint32_t h = (uint32_t) (uint16_t) (-c);
            out[3 * i + ((x + j) >> 1) - i] |= ((x + j) & 1) ? h << 16 : h;
        }
        out[15 + i] = r == 2 ? 0xffff8000u : 0u;
    }
}
struct SliceWin {
    lds_u32p pw;            // LDS address of the dword holding the even sample at or below the first tap of the lane's first group
    uint32_t K[15];
    uint32_t init[5];
};
// pos_local: the frame's scan position in the tile, ti = try-phase - 4, g0 = the lane's first group
__device__ __forceinline__ void make_win(const uint32_t *s_wc, const uint32_t *w32, int pos_local, int ti, int g0, SliceWin &W) {
    const int base = pos_local + 19 + (ti != 0 ? 1 : 0);                     // + t / 5
    const u32x4 *row = (const u32x4 *) (s_wc + (2 * ti + (base & 1)) * kWcRowWords);
    const u32x4 a = row[0], b = row[1], c = row[2], d = row[3], f = row[4];
    W.K[0] = a.x; W.K[1] = a.y; W.K[2] = a.z; W.K[3] = a.w; W.K[4] = b.x; W.K[5] = b.y; W.K[6] = b.z; W.K[7] = b.w;
    W.K[8] = c.x; W.K[9] = c.y; W.K[10] = c.z; W.K[11] = c.w; W.K[12] = d.x; W.K[13] = d.y; W.K[14] = d.z;
    W.init[0] = d.w; W.init[1] = f.x; W.init[2] = f.y; W.init[3] = f.z; W.init[4] = f.w;
    W.pw = (lds_u32p) w32 + ((base + 12 * g0) >> 1);
    asm volatile("" : "+v"(W.pw));
}
// the group whose window is w0 .. w6
__device__ __forceinline__ uint32_t win_group(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5, uint32_t w6, const SliceWin &W) {
#define WIN_BIT(I, A, B, C) __builtin_amdgcn_sdot2(__builtin_bit_cast(v2i16, C), __builtin_bit_cast(v2i16, W.K[3 * (I) + 2]), \
                                __builtin_amdgcn_sdot2(__builtin_bit_cast(v2i16, B), __builtin_bit_cast(v2i16, W.K[3 * (I) + 1]), \
                                    dot_first(A, W.K[3 * (I)], W.init[I]), false), false)
    const int s0 = WIN_BIT(0, w0, w1, w2), s1 = WIN_BIT(1, w1, w2, w3), s2 = WIN_BIT(2, w2, w3, w4), s3 = WIN_BIT(3, w3, w4, w5),
              s4 = WIN_BIT(4, w4, w5, w6);
#undef WIN_BIT
    uint32_t X = (uint32_t) s0 >> 31;                        // frame bit i of the group at place 4 - i
    X = __builtin_amdgcn_alignbit(X, (uint32_t) s1, 31);     // (X << 1) | sign
    X = __builtin_amdgcn_alignbit(X, (uint32_t) s2, 31);
    X = __builtin_amdgcn_alignbit(X, (uint32_t) s3, 31);
    X = __builtin_amdgcn_alignbit(X, (uint32_t) s4, 31);
    return X;
}

// THE BIAS ARITHMETIC both forms above rest on.  The tile holds the samples with the top bit flipped (u16 m -> i16 m - 32768), so that
// two taps go through one v_dot2_i32_i16:  sum(c_j * m_j) > 0  <=>  sum(c_j * (m_j - 32768)) > -32768 * sum(c_j), and the rows'
// coefficient sums are 0, 0, 1, 0, 0 (demod_2400.c:74-93).  With NEGATED coefficients the bit is the sign bit of the sum — one shift
// and one v_lshl_or / v_alignbit per bit instead of compare, select, shift, or — and row 2's threshold (sum > -32768) goes into its
// accumulator's start value: -(sum) - 32768 < 0.

#include "crc_lookup.inc"       // key_tables, key_tables_preload, lane_diagnose


__device__ __forceinline__ uint32_t fix_aa(uint32_t aa, int bit) {       // a repaired bit inside the AA field (frame bits 8..31)
    return (bit >= 8 && bit <= 31) ? aa ^ (1u << (31 - bit)) : aa;
}

constexpr int kWAdderCache = 512;                            // direct-mapped LDS cache of adder addresses already published

struct SlicedFrame {          // 32 bytes: a frame as sliced, waiting for CRC classification
    uint32_t W[4];            // frame bits 0..127, bit 0 = MSB of W[0]
    uint32_t synd;            // CRC-24 syndrome (112- or 56-bit, by DF)
    uint32_t meta;            // df | try-phase << 8
    uint32_t pos;             // scan position within the chunk
    uint32_t pad;
};

#define WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// Everything scoreModesMessage / decodeModesMessage's CRC stage decide about one sliced frame without
// the ICAO filter (mode_s.c:276-419, 443-606): fills the two record halves, returns false when the
// frame scores -2 whatever the filter holds.
__device__ __forceinline__ bool classify_frame(const SweepParams &p, const uint32_t *s_gsyn, const uint32_t *s_keys,
                                               uint32_t W0, uint32_t W1, uint32_t W2, uint32_t W3, uint32_t synd, uint32_t df,
                                               int t, uint32_t pos, u32x4 &ra, u32x4 &rb, uint32_t &flags_out, uint32_t &addr_out) {
    // Straight-line: every test is a per-lane predicate (the format tests are one bit of a constant mask: as `df == a || df == b ...`
    // under nested ifs the compiler built decision trees on the exec mask — half of the scoring pass's instructions were scalar).
    const bool is_long = (p.valid_long >> df) & 1;
    const uint32_t aa = W0 & 0xffffffu;          // getbits(msg, 9, 32)
    const uint32_t dfb = 1u << df;
    constexpr uint32_t kDfFix = (1u << 1) | (1u << 16) | (1u << 19) | (1u << 21) | (1u << 25);   // DF17 with one bit of the DF field flipped
    constexpr uint32_t kDfApLong = (1u << 16) | (1u << 20) | (1u << 21), kDfEs = (1u << 17) | (1u << 18);
    const bool nonzero = !(W0 == 0 && (W1 >> 8) == 0);
    const int jfix = 5 - __ffs((df ^ 17u) | 32u);                     // which DF bit (df == 17: -1 + ... never used)
    // fixDF17msgtype, mode_s.c:276-301: the syndrome is that of the flipped bit (s_gsyn[16 >> j] == bit_syndrome[j])
    const bool handled = is_long && p.fix_df && (dfb & kDfFix) && synd == s_gsyn[(16u >> (jfix & 7)) & 31u];
    const bool live = nonzero && !handled;
    const bool ap = live && (is_long ? (dfb & kDfApLong) != 0 : df != 11);          // Address/Parity: the syndrome IS the address
    const bool es = live && is_long && (dfb & kDfEs);                                // DF17 / DF18
    const bool s11 = live && !is_long && df == 11;
    const bool s11_out = (synd & 0xffff80u) != 0;                                    // syndrome outside the IID bits
    // The one syndrome lookup a frame can need — DF17/18 with a nonzero syndrome in the 112-bit table, DF11 with a syndrome
    // outside the IID bits in the 56-bit table — as ONE search for the whole wave (the lanes differ in table, not in code):
    // two separate searches in two divergent branches were a third of the scoring pass.
    const bool look_long = es && synd != 0, look_short = s11 && s11_out;
    int nerr = 0, b0 = 0xff, b1 = 0xff;
    if (look_long || look_short)
    {
        const KeyTables kt = key_tables(s_keys, p.n_long, p.n_short);
        nerr = lane_diagnose(look_short ? kt.lo_short : kt.lo_long, look_short ? kt.start_short : kt.start_long, look_short ? p.tab_short : p.tab_long, synd, b0, b1);
    }
    const bool es_ok = es && nerr >= 0;
    const bool s11_fix = s11 && s11_out && nerr == 1;                                // (2-bit errors are ambiguous in DF11)
    const bool s11_clean = s11 && !s11_out && (synd & 0x7fu) == 0, s11_iid = s11 && !s11_out && (synd & 0x7fu) != 0;
    const bool emit = handled || ap || es_ok || s11_fix || s11_clean || s11_iid;
    const uint32_t a_b0 = fix_aa(aa, b0);
    const uint32_t a2 = nerr >= 2 ? fix_aa(a_b0, b1) : nerr >= 1 ? a_b0 : aa;
    int sk = 1000, su = -1, fb0 = 0xff, fb1 = 0xff;                                  // ap / s11_iid
    uint32_t addr = ap ? synd : aa, flags = (is_long ? REC_LONG : 0) | REC_COND;
    if (handled) { sk = 900; su = 700; flags = REC_LONG | REC_ACCEPT_IF_UNKNOWN | REC_DFFIX | (1u << REC_CORR_SHIFT); fb0 = jfix; }
    if (es_ok) {
        sk = nerr == 0 ? 1800 : nerr == 1 ? 900 : 600; su = nerr == 0 ? 1400 : nerr == 1 ? 700 : 466;   // 1800 / (nerr + 1), 1400 / (nerr + 1)
        addr = a2;
        flags = REC_LONG | ((uint32_t) nerr << REC_CORR_SHIFT) | (a2 == aa ? REC_ACCEPT_IF_UNKNOWN : 0u)      // mode_s.c:560: only a changed AA needs the filter
              | ((nerr == 0 && df == 17) ? REC_ADDER : 0u);
        fb0 = nerr >= 1 ? b0 : 0xff; fb1 = nerr >= 2 ? b1 : 0xff;
    }
    if (s11_fix) { sk = 800; addr = a_b0; flags = REC_COND | (1u << REC_CORR_SHIFT); fb0 = b0; }
    if (s11_clean) { sk = 1600; su = 750; flags = REC_ACCEPT_IF_UNKNOWN | REC_ADDER; }
    if (!emit) return false;
    ra.x = pos;
    ra.y = (uint32_t) t | (flags << 8) | ((uint32_t) (uint16_t) sk << 16);
    ra.z = (uint32_t) (uint16_t) su | ((uint32_t) fb0 << 16) | ((uint32_t) fb1 << 24);
    ra.w = addr;
    if (!is_long) { W1 &= 0xffffff00u; W2 = 0; W3 = 0; }
    rb.x = __builtin_bswap32(W0); rb.y = __builtin_bswap32(W1);
    rb.z = __builtin_bswap32(W2); rb.w = __builtin_bswap32(W3) & 0xffffu;
    flags_out = flags;
    addr_out = addr;
    return true;
}

