// ldpc5g_lowpapr.h — one point of the low-PAPR (Zadoff-Chu) base sequence rbar_{u,v}(m) of 38.211
// 5.2.2 (py5gphy/common/lowPAPR_seq.py:5-41, gen_lowPAPR_seq), shared by ldpc5g_tp.hip
// (ldpc5g_low_papr_seq) and ldpc5g_slot.hip (the low-PAPR DMRS of the slot front end).
// MZC = 30: the closed form exp(-j pi (u+1)(m+1)(m+2) / 31).  MZC >= 36: x_q(m mod N_ZC), x_q(n) =
// exp(-j pi q n (n+1) / N_ZC), with q from integers and the phase index reduced mod 2 N_ZC in
// 64-bit integers before the one sincospi.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ldpc5g_common.h"

namespace ldpc5g_impl {

__device__ __forceinline__ int64_t zc_q(int NZC, int u, int v) {
    const int64_t A = (int64_t)NZC * (u + 1);       // qbar = A / 31
    const int64_t q = (2 * A + 31) / 62;            // floor(qbar + 1/2)
    return q + (((2 * A / 31) & 1) ? -(int64_t)v : (int64_t)v);
}

__device__ __forceinline__ void low_papr_point(int u, int v, int m, int MZC, int NZC, double& re, double& im) {
    int64_t idx, den;
    if (MZC == 30) {
        idx = ((int64_t)(u + 1) * (m + 1) * (m + 2)) % 62, den = 31;
    } else {
        const int64_t n = m % NZC;
        idx = (zc_q(NZC, u, v) * (n * (n + 1) % (2 * (int64_t)NZC))) % (2 * (int64_t)NZC), den = NZC;
    }
    double s, c;
    sincospi(-(double)idx / (double)den, &s, &c);
    re = c, im = s;
}

inline int largest_prime_below(int n) {
    for (int p = n - 1; p >= 2; --p) {
        bool prime = true;
        for (int d = 2; d * d <= p; ++d)
            if (p % d == 0) { prime = false; break; }
        if (prime) return p;
    }
    return 0;
}

// N_ZC of a sequence of length MZC >= 30
inline int low_papr_nzc(int MZC) { return MZC == 30 ? 31 : largest_prime_below(MZC); }

}  // namespace ldpc5g_impl
