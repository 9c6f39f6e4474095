// ldpc5g_demod.h — device code of the soft demodulator + LLR descrambling shared by the
// stand-alone kernel (ldpc5g_phy.hip: demod_descramble_kernel) and the fused receive front end
// (ldpc5g_sch.hip: demod_raterecover_kernel):
//   py5gphy/demodulation/nr_Demodulation.py:12-46, demod_{qpsk,16qam,64qam,256qam,1024qam}.py,
//   py5gphy/nr_pdsch/nr_pdsch.py:268-274.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ldpc5g_common.h"

namespace ldpc5g_impl {

// n <= 8 bits of a packed scrambling code (bit k of word w = c(32w + k)) from bit `pos`
__device__ __forceinline__ uint32_t prbs_bits(const uint32_t* w, int64_t pos, int n) {   // n <= 8
    const int64_t q = pos >> 5;
    const int sh = (int)(pos & 31);
    uint32_t v = w[q] >> sh;
    if (sh + n > 32) v |= w[q + 1] << (32 - sh);
    return v & ((1u << n) - 1u);
}

// ===================================================================== soft demodulation
// Piecewise-linear max-log segments of the reference's demod_*.py, per PAM bit pair p (bits 2p /
// 2p+1 from the real / imaginary part): r < thr*A  ->  LLR = (k*A) * (s*r + (s*c)*A) / nv, or
// (k*A) * r / nv when c = 0.  The 1024QAM table is extracted from demod_1024qam.py by
// tools/gen_demod_tables.py (its if/elif chains, verbatim coefficients).
struct Seg {
    int8_t thr, k, s, c;   // thr = 127: +inf
};
constexpr int kSegMax = 31;
struct SegTable {
    int8_t nseg[5];
    Seg seg[5][kSegMax];
};
constexpr SegTable kSegQpsk = {{1}, {{{127, 4, 1, 0}}}};
constexpr SegTable kSeg16 = {{3, 2},
                             {{{-2, 8, 1, 1}, {2, 4, 1, 0}, {127, 8, 1, -1}},
                              {{0, 4, 1, 2}, {127, 4, -1, -2}}}};
constexpr SegTable kSeg64 = {{7, 6, 4},
                             {{{-6, 16, 1, 3}, {-4, 12, 1, 2}, {-2, 8, 1, 1}, {2, 4, 1, 0}, {4, 8, 1, -1}, {6, 12, 1, -2}, {127, 16, 1, -3}},
                              {{-6, 8, 1, 5}, {-2, 4, 1, 4}, {0, 8, 1, 3}, {2, 8, -1, -3}, {6, 4, -1, -4}, {127, 8, -1, -5}},
                              {{-4, 4, 1, 6}, {0, 4, -1, 2}, {4, 4, 1, -2}, {127, 4, -1, -6}}}};
constexpr SegTable kSeg256 = {{15, 14, 12, 8},
                              {{{-14, 32, 1, 7}, {-12, 28, 1, 6}, {-10, 24, 1, 5}, {-8, 20, 1, 4}, {-6, 16, 1, 3}, {-4, 12, 1, 2}, {-2, 8, 1, 1}, {2, 4, 1, 0},
                                {4, 8, 1, -1}, {6, 12, 1, -2}, {8, 16, 1, -3}, {10, 20, 1, -4}, {12, 24, 1, -5}, {14, 28, 1, -6}, {127, 32, 1, -7}},
                               {{-14, 16, 1, 11}, {-12, 12, 1, 10}, {-10, 8, 1, 9}, {-6, 4, 1, 8}, {-4, 8, 1, 7}, {-2, 12, 1, 6}, {0, 16, 1, 5},
                                {2, 16, -1, -5}, {4, 12, -1, -6}, {6, 8, -1, -7}, {10, 4, -1, -8}, {12, 8, -1, -9}, {14, 12, -1, -10}, {127, 16, -1, -11}},
                               {{-14, 8, 1, 13}, {-10, 4, 1, 12}, {-8, 8, 1, 11}, {-6, 8, -1, 5}, {-2, 4, -1, 4}, {0, 8, -1, 3}, {2, 8, 1, -3},
                                {6, 4, 1, -4}, {8, 8, 1, -5}, {10, 8, -1, -11}, {14, 4, -1, -12}, {127, 8, -1, -13}},
                               {{-12, 4, 1, 14}, {-8, 4, -1, 10}, {-4, 4, 1, 6}, {0, 4, -1, 2}, {4, 4, 1, -2}, {8, 4, -1, -6}, {12, 4, 1, -10},
                                {127, 4, -1, -14}}}};
#include "ldpc5g_demod1024.h"
template <int QM>
constexpr const SegTable& seg_table() {
    if constexpr (QM == 2) return kSegQpsk;
    else if constexpr (QM == 4) return kSeg16;
    else if constexpr (QM == 6) return kSeg64;
    else if constexpr (QM == 8) return kSeg256;
    else return kSeg1024;
}

// One LLR in the arithmetic type C of the input symbols: double for complex128; float for
// complex64, where numpy >= 2 evaluates demod_*.py's scalar expressions in float32 with every
// Python-float constant (k*A, c*A, thr*A) rounded to float32 first (NEP 50) — comparisons too.
template <int QM, int P, typename C>
__device__ __forceinline__ C demod_llr(C r, double A, C nv) {
    constexpr const SegTable& T = seg_table<QM>();
    constexpr int n = T.nseg[P];
    // the reference's if / elif chain: the first segment with r < thr * A; scanned from the top
    // so the lowest matching segment is selected last (all selects, no branches)
    constexpr Seg top = T.seg[P][n - 1];
    C kA = (C)((double)top.k * A), sr = (C)top.s, cA = (C)((double)(top.s * top.c) * A);
    bool noc = top.c == 0;
    sfor<0, n - 1>([&](auto ic) {
        constexpr int i = n - 2 - decltype(ic)::value;
        constexpr Seg g = T.seg[P][i];
        const bool hit = r < (C)((double)g.thr * A);
        kA = hit ? (C)((double)g.k * A) : kA;
        sr = hit ? (C)g.s : sr;
        cA = hit ? (C)((double)(g.s * g.c) * A) : cA;
        noc = hit ? (g.c == 0) : noc;
    });
    const C x = noc ? r : sr * r + cA;
    return (kA * x) / nv;
}

template <typename T>
__device__ __forceinline__ T flip_sign(T v, uint32_t bit) {
    if constexpr (sizeof(T) == 4) return __uint_as_float(__float_as_uint(v) ^ (bit << 31));
    else return __longlong_as_double(__double_as_longlong(v) ^ ((long long)bit << 63));
}

// The QM LLRs of one symbol (re, im) with noise variance nv, before descrambling, in the
// symbol's arithmetic type C and stored as Tout (float32 as nr_Demodulation.py stores them).
// QM = 1: BPSK LLR = 4 (re + im) A / nv (demod_bpsk.py:9); `odd` (pi/2-BPSK, the symbol's index
// in its transport-block row is odd) uses 4 (-re + im) A / nv (demod_pi2_bpsk.py:11-12).
// Tout = double only for BPSK on complex128 input, whose reference result stays float64 (no
// float32 store in demod_bpsk.py).
template <int QM, typename C, typename Tout>
__device__ __forceinline__ void demod_symbol(C re, C im, C nv, double A, bool odd, Tout (&v)[QM]) {
    if constexpr (QM == 1) {
        const C sre = odd ? -re + im : re + im;
        v[0] = (Tout)(((C)4 * sre) * (C)A / nv);
    } else {
        sfor<0, QM / 2>([&](auto pc) {
            constexpr int p = decltype(pc)::value;
            v[2 * p] = (Tout)demod_llr<QM, p>(re, A, nv);
            v[2 * p + 1] = (Tout)demod_llr<QM, p>(im, A, nv);
        });
    }
}

// modulation id -> (Qm, pi/2): LDPC5G_PI2_BPSK = -1, otherwise the order Qm itself
inline int mod_scale(int Qm) {   // sqrt(scale) of nrModulation.py / A = 1 / sqrt(scale) of demod_*.py
    return Qm == 1 ? 2 : Qm == 2 ? 2 : Qm == 4 ? 10 : Qm == 6 ? 42 : Qm == 8 ? 170 : 682;
}
inline bool mod_ok(int mod) { return mod == -1 || mod == 1 || mod == 2 || mod == 4 || mod == 6 || mod == 8 || mod == 10; }

}  // namespace ldpc5g_impl
