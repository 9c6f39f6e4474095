// ldpc5g_prbs.h — the parts of the Gold sequence c(n) of py5gphy/common/nrPRBS.py:5-25 (gen_nrPRBS)
// that ldpc5g_phy.hip (scrambling codes) and ldpc5g_slot.hip (DMRS sequences) share: the constexpr
// generator of the jump-ahead matrices T^(2^i) and the 32-position step.  Each translation unit
// builds the device table it needs from the generator (column form there, row form here).
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

}  // namespace ldpc5g_impl
