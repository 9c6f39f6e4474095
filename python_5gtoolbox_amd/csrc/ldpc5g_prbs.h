// ldpc5g_prbs.h — the parts of the Gold sequence c(n) of py5gphy/common/nrPRBS.py:5-25 (gen_nrPRBS)
// that ldpc5g_phy.hip (scrambling codes) and ldpc5g_slot.hip (DMRS sequences) share: the constexpr
// generator of the jump-ahead matrices T^(2^i), the 32-position step, and the row-form device
// table with the wave-wide jump that ldpc5g_slot.hip uses for both of its sequence sources (the
// Gold DMRS bits; the group / sequence hopping of the low-PAPR DMRS).  ldpc5g_phy.hip builds its
// column-form device table from the generator itself.
#pragma once
#include <stdint.h>

#include "ldpc5g_common.h"

namespace ldpc5g_impl {

constexpr int kPrbsPow = 26;   // jumps up to 2^26 positions (G + 1600 < 67 M bits)
struct PrbsTables {
    uint32_t t[2][kPrbsPow][31];   // [x1 / x2][i][column j] of T^(2^i), T = one LFSR step
};
// State S(n) of an m-sequence: bit i = x(n + i), i = 0..30.  One step: bit i <- bit i+1,
// bit 30 <- x(n+31) = XOR of the taps (x1: x(n+3) + x(n); x2: x(n+3) + x(n+2) + x(n+1) + x(n)).
__host__ __device__ constexpr uint32_t mat_apply(const uint32_t (&M)[31], uint32_t v) {
    uint32_t r = 0;
    for (int j = 0; j < 31; ++j)
        if ((v >> j) & 1u) r ^= M[j];
    return r;
}
constexpr PrbsTables make_prbs_tables() {
    PrbsTables P{};
    for (int q = 0; q < 2; ++q) {
        const uint32_t taps = q == 0 ? 0x9u : 0xfu;   // x1: {0, 3}; x2: {0, 1, 2, 3}
        for (int j = 0; j < 31; ++j)
            P.t[q][0][j] = (j >= 1 ? 1u << (j - 1) : 0u) | (((taps >> j) & 1u) ? 1u << 30 : 0u);
        for (int i = 1; i < kPrbsPow; ++i)
            for (int j = 0; j < 31; ++j) P.t[q][i][j] = mat_apply(P.t[q][i - 1], P.t[q][i - 1][j]);
    }
    return P;
}

// x(m .. m+31) of an m-sequence from its state at m; `s` becomes the state at m + 32.
__device__ __forceinline__ uint32_t prbs_step32(uint32_t& s, bool x2) {
    uint64_t W = s;
    const uint64_t n1 = x2 ? (W ^ (W >> 1) ^ (W >> 2) ^ (W >> 3)) : (W ^ (W >> 3));
    W |= (n1 & 0x0FFFFFFFull) << 31;                      // x(m+31 .. m+58)
    const uint64_t n2 = x2 ? ((W >> 28) ^ (W >> 29) ^ (W >> 30) ^ (W >> 31)) : ((W >> 28) ^ (W >> 31));
    W |= (n2 & 0xFull) << 59;                             // x(m+59 .. m+62)
    s = (uint32_t)(W >> 32) & 0x7FFFFFFFu;
    return (uint32_t)W;
}

// The jump-ahead matrices T^(2^i) in ROW form, r[q][i][b] bit j = bit b of column j:
// bit b of T^(2^i) s is the parity of s & r[q][i][b], so a wave applies one matrix to a wave-uniform
// state with one AND, one population count and one ballot, lane b making bit b.  Levels 0..12 reach
// every position below 8192: the last bit a DMRS sequence can need is 1600 + 2 * 6 * 275 = 4900, and
// the idle waves of a last workgroup start at most 4 * 255 bits further on.
constexpr int kDmrsLevels = 13;
struct PrbsRows {
    uint32_t r[2][kDmrsLevels][32];
};
constexpr PrbsRows make_prbs_rows() {
    const PrbsTables P = make_prbs_tables();
    PrbsRows R{};
    for (int q = 0; q < 2; ++q)
        for (int i = 0; i < kDmrsLevels; ++i)
            for (int b = 0; b < 31; ++b)
                for (int j = 0; j < 31; ++j) R.r[q][i][b] |= ((P.t[q][i][j] >> b) & 1u) << j;
    return R;
}
__device__ const PrbsRows kPrbsRows = make_prbs_rows();

// T^n s for wave-uniform s and n < 2^kDmrsLevels; every lane of the wave must be active.
__device__ __forceinline__ uint32_t prbs_jump_wave(int q, uint32_t s, uint32_t n) {
    const int b = threadIdx.x & 31;
    uint32_t rows[kDmrsLevels];
#pragma unroll
    for (int i = 0; i < kDmrsLevels; ++i) rows[i] = kPrbsRows.r[q][i][b];   // all loads in flight at once
#pragma unroll
    for (int i = 0; i < kDmrsLevels; ++i)
        if ((n >> i) & 1u) s = (uint32_t)__ballot(__popc(s & rows[i]) & 1) & 0x7FFFFFFFu;
    return s;
}

}  // namespace ldpc5g_impl
