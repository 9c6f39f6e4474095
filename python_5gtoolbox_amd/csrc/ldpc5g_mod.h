// ldpc5g_mod.h — the modulation mapper's levels (py5gphy/common/nrModulation.py:4-42), shared by
// scramble_modulate_kernel (ldpc5g_phy.hip) and the placeholder-aware one of ldpc5g_uci.hip.
#pragma once
#include <stdint.h>

#include "ldpc5g_common.h"

namespace ldpc5g_impl {

// u[i] = 1 - 2 b'(i) of the symbol's QM scrambled bits; symbol = (level_re + j level_im) * scl.
// QM = 1: BPSK (re = im = 1 - 2b, nrModulation.py:15-16); with PI2, odd symbols re = 2b - 1
// (pi/2-BPSK, :17-21).  QM = 10: 1024QAM (:38-42).
template <int QM, bool PI2>
__device__ __forceinline__ float2 mod_symbol(const float (&u)[QM], int64_t m, float scl) {
    float re, im;
    if constexpr (QM == 1) {
        re = (PI2 && (m & 1)) ? -u[0] : u[0], im = u[0];
    } else if constexpr (QM == 2) {
        re = u[0], im = u[1];
    } else if constexpr (QM == 4) {
        re = u[0] * (2.0f - u[2]), im = u[1] * (2.0f - u[3]);
    } else if constexpr (QM == 6) {
        re = u[0] * (4.0f - u[2] * (2.0f - u[4]));
        im = u[1] * (4.0f - u[3] * (2.0f - u[5]));
    } else if constexpr (QM == 8) {
        re = u[0] * (8.0f - u[2] * (4.0f - u[4] * (2.0f - u[6])));
        im = u[1] * (8.0f - u[3] * (4.0f - u[5] * (2.0f - u[7])));
    } else {
        re = u[0] * (16.0f - u[2] * (8.0f - u[4] * (4.0f - u[6] * (2.0f - u[8]))));
        im = u[1] * (16.0f - u[3] * (8.0f - u[5] * (4.0f - u[7] * (2.0f - u[9]))));
    }
    return make_float2(re * scl, im * scl);
}

}  // namespace ldpc5g_impl
