// ldpc5g_eq.hip — batched linear MIMO equalisation, the producer of the receive chain's symbols
// and noise variances (ldpc5g_equalize, include/ldpc5g.h):
//   ZF / ZF-IRC ........ py5gphy/channel_equalization/ZF.py:47-79 / :5-45
//   MMSE / MMSE-IRC .... py5gphy/channel_equalization/MMSE.py:58-103 / :5-56
// called once per resource element by channel_equ_and_demod (nr_channel_eq.py:12-50) from the
// double loop of Pdsch.RX_process (nr_pdsch.py:245-263) and its PUSCH twin (nr_pusch.py:147-165).
//
// One thread per data resource element; the kernel is a template on <Nr, NL, algorithm, storage
// type> and every matrix lives in fully unrolled registers (all loop bounds and indices are
// compile-time constants).  Arithmetic is float64 whatever the storage type.  cov and W1 are
// Hermitian positive semidefinite: only their lower triangle and the real part of their diagonal
// are read / formed, and they are inverted through an unpivoted LDL^H factorisation
//   A = L D L^H,  A^-1 = L^-H D^-1 L^-1.
// The reference regularises A (+ 0.0012 max|A| I) when np.linalg.matrix_rank(A) < n; here the
// test is NOT(min_k d_k > 2^-40 max_ij |A_ij|) on the pivots d_k (the rule and its agreement band
// with numpy's SVD test: include/ldpc5g.h).  The complex helpers, Herm, the LDL^H inverse and the
// pivot rule live in ldpc5g_eq.h, shared with the ML detectors (ldpc5g_ml.hip).
//
// H is read straight from memory, 16 bytes per load per lane.  Building with
// -DLDPC5G_EQ_STAGE_LDS=1 instead stages H of a workgroup's resource elements through LDS with
// coalesced loads (one padded row per resource element); that variant exists for the A/B timing of
// tools/eq_probe.py and gives the same results bit for bit.
#include "ldpc5g_eq.h"

#ifndef LDPC5G_EQ_STAGE_LDS
#define LDPC5G_EQ_STAGE_LDS 0
#endif

namespace ldpc5g_impl {
namespace {

#if LDPC5G_EQ_STAGE_LDS
constexpr int kEqThreads = 64;    // one wave: 64 padded rows of H fit the static LDS limit
#else
constexpr int kEqThreads = 256;
#endif

template <int NR, int NL, int ALGO, typename C>
__global__ __launch_bounds__(kEqThreads) void equalize_kernel(const C* __restrict__ y, int64_t ldy,
                                                              const C* __restrict__ h, int64_t ldh,
                                                              const C* __restrict__ cov, int64_t ldcov,
                                                              const int32_t* __restrict__ re_idx, int64_t R,
                                                              int64_t nre, int32_t re_per_cov,
                                                              C* __restrict__ sym, int64_t ldsym,
                                                              float* __restrict__ nvar, int64_t ldnv) {
    using S = decltype(C{}.x);
    constexpr bool IRC = ALGO == LDPC5G_EQ_ZF_IRC || ALGO == LDPC5G_EQ_MMSE_IRC;
    constexpr bool MMSE = ALGO == LDPC5G_EQ_MMSE || ALGO == LDPC5G_EQ_MMSE_IRC;
    constexpr int NE = NR * NL;
    const int t = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kEqThreads + threadIdx.x;
    const bool live = i < nre;
    int64_t r = live ? (re_idx ? (int64_t)re_idx[i] : i) : -1;
    const bool valid = live && r >= 0 && r < R;   // an index outside 0..R-1 reads nothing: NaN out
    if (!valid) r = -1;
    const C* hT = h + (int64_t)t * ldh;

    cx H[NR][NL];
#if LDPC5G_EQ_STAGE_LDS
    __shared__ C stage[kEqThreads][NE + 1];
    __shared__ int64_t rows[kEqThreads];
    rows[threadIdx.x] = r;
    __syncthreads();
    for (int q = threadIdx.x; q < kEqThreads * NE; q += kEqThreads) {
        const int k = q / NE, e = q - k * NE;
        const int64_t rr = rows[k];
        if (rr >= 0) stage[k][e] = hT[rr * NE + e];
    }
    __syncthreads();
#endif
    if (!live) return;
    C* out = sym + (int64_t)t * ldsym + i * NL;
    float* nvo = nvar + (int64_t)t * ldnv + i * NL;
    if (!valid) {
#pragma unroll
        for (int l = 0; l < NL; ++l) out[l] = C{(S)NAN, (S)NAN}, nvo[l] = NAN;
        return;
    }
#pragma unroll
    for (int q = 0; q < NR; ++q) {
#pragma unroll
        for (int l = 0; l < NL; ++l) {
#if LDPC5G_EQ_STAGE_LDS
            H[q][l] = widen(stage[threadIdx.x][q * NL + l]);
#else
            H[q][l] = widen(hT[r * NE + q * NL + l]);
#endif
        }
    }
    cx Y[NR];
    const C* yT = y + (int64_t)t * ldy + r * NR;
#pragma unroll
    for (int q = 0; q < NR; ++q) Y[q] = widen(yT[q]);
    // covariance of the block this resource element belongs to: lower triangle (IRC) or diagonal
    const C* cT = cov + (int64_t)t * ldcov + (r / re_per_cov) * (NR * NR);
    Herm<NR> Cv;
#pragma unroll
    for (int a = 0; a < NR; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b)
            if (IRC || a == b) Cv.a[a][b] = widen(cT[a * NR + b]);
    }

    cx s[NL];
    double nv[NL];
    if constexpr (NR == 1) {
        // s = Y / H, noise_var = Re(cov / (conj(H) H)); H == 0 gives inf / NaN
        const double hh = H[0][0].re * H[0][0].re + H[0][0].im * H[0][0].im;
        const cx p = cmulcb(Y[0], H[0][0]);
        s[0] = {p.re / hh, p.im / hh};
        nv[0] = Cv.a[0][0].re / hh;
    } else {
        cx z[NL];          // H^H Y (MMSE-IRC: H^H cov^-1 Y)
        Herm<NL> W1, V;
        double rs = 1.0, sigma2 = 0.0;
        if constexpr (ALGO == LDPC5G_EQ_MMSE_IRC) {
            Herm<NR> Ci;
            herm_inverse_reg(Cv, Ci);
            cx A[NR][NL];   // cov^-1 H
#pragma unroll
            for (int q = 0; q < NR; ++q) {
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    cx acc = {0.0, 0.0};
#pragma unroll
                    for (int k = 0; k < NR; ++k) cacc(acc, cmul(herm_at(Ci, q, k), H[k][l]));
                    A[q][l] = acc;
                }
            }
#pragma unroll
            for (int a = 0; a < NL; ++a) {
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                    cx acc = {0.0, 0.0};
#pragma unroll
                    for (int q = 0; q < NR; ++q) cacc(acc, cmulc(H[q][a], A[q][b]));
                    W1.a[a][b] = acc;
                }
                W1.a[a][a].re += 1.0;
                cx acc = {0.0, 0.0};
#pragma unroll
                for (int q = 0; q < NR; ++q) cacc(acc, cmulc(A[q][a], Y[q]));
                z[a] = acc;
            }
        } else {
#pragma unroll
            for (int q = 0; q < NR; ++q) sigma2 += Cv.a[q][q].re;
            sigma2 = sigma2 / NR;   // np.mean(np.diagonal(cov))
            if constexpr (MMSE) rs = 1.0 / sigma2;   // numpy divides by the complex (sigma_2, 0): a reciprocal
#pragma unroll
            for (int a = 0; a < NL; ++a) {
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                    cx acc = {0.0, 0.0};
#pragma unroll
                    for (int q = 0; q < NR; ++q) cacc(acc, cmulc(H[q][a], H[q][b]));
                    W1.a[a][b] = MMSE ? cscale(acc, rs) : acc;
                }
                if constexpr (MMSE) W1.a[a][a].re += 1.0;
                cx acc = {0.0, 0.0};
#pragma unroll
                for (int q = 0; q < NR; ++q) cacc(acc, cmulc(H[q][a], Y[q]));
                z[a] = acc;
            }
        }
        herm_inverse_reg(W1, V);
        if constexpr (ALGO == LDPC5G_EQ_ZF_IRC) {
            // W = W1^-1 H^H; s = W Y; noise_var = diag(W cov W^H)
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                cx W[NR];
                cx acc = {0.0, 0.0};
#pragma unroll
                for (int q = 0; q < NR; ++q) {
                    cx w = {0.0, 0.0};
#pragma unroll
                    for (int k = 0; k < NL; ++k) cacc(w, cmulcb(herm_at(V, l, k), H[q][k]));
                    W[q] = w;
                    cacc(acc, cmul(w, Y[q]));
                }
                s[l] = acc;
                double v = 0.0;
#pragma unroll
                for (int a = 0; a < NR; ++a) {
                    cx u = {0.0, 0.0};   // (W cov)[l][a]
#pragma unroll
                    for (int b = 0; b < NR; ++b) cacc(u, cmul(W[b], herm_at(Cv, b, a)));
                    v += cmulcb(u, W[a]).re;
                }
                nv[l] = v;
            }
        } else {
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                cx acc = {0.0, 0.0};
#pragma unroll
                for (int k = 0; k < NL; ++k) cacc(acc, cmul(herm_at(V, l, k), z[k]));
                if constexpr (ALGO == LDPC5G_EQ_ZF) {
                    s[l] = acc;
                    nv[l] = sigma2 * V.a[l][l].re;
                } else {
                    if constexpr (ALGO == LDPC5G_EQ_MMSE) acc = cscale(acc, rs);
                    const double comp = 1.0 - V.a[l][l].re;
                    s[l] = {acc.re / comp, acc.im / comp};
                    nv[l] = 1.0 / comp - 1.0;
                }
            }
        }
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        out[l] = C{(S)s[l].re, (S)s[l].im};
        nvo[l] = (float)nv[l];
    }
}

template <int NR, int NL, typename C>
void launch_eq_algo(int algo, dim3 grid, hipStream_t st, const C* y, int64_t ldy, const C* h, int64_t ldh,
                    const C* cov, int64_t ldcov, const int32_t* re_idx, int64_t R, int64_t nre, int32_t rpc,
                    C* sym, int64_t ldsym, float* nv, int64_t ldnv) {
#define LDPC5G_EQ(ALGO)                                                                              \
    hipLaunchKernelGGL((equalize_kernel<NR, NL, ALGO, C>), grid, dim3(kEqThreads), 0, st, y, ldy, h, ldh, cov, \
                       ldcov, re_idx, R, nre, rpc, sym, ldsym, nv, ldnv)
    if constexpr (NR == 1) {   // the Nr == 1 shortcut is the same for the four algorithms
        LDPC5G_EQ(LDPC5G_EQ_ZF);
    } else {
        switch (algo) {
            case LDPC5G_EQ_ZF: LDPC5G_EQ(LDPC5G_EQ_ZF); break;
            case LDPC5G_EQ_ZF_IRC: LDPC5G_EQ(LDPC5G_EQ_ZF_IRC); break;
            case LDPC5G_EQ_MMSE: LDPC5G_EQ(LDPC5G_EQ_MMSE); break;
            default: LDPC5G_EQ(LDPC5G_EQ_MMSE_IRC); break;
        }
    }
#undef LDPC5G_EQ
}

template <typename C>
void launch_eq(int Nr, int NL, int algo, dim3 grid, hipStream_t st, const void* y, int64_t ldy, const void* h,
               int64_t ldh, const void* cov, int64_t ldcov, const int32_t* re_idx, int64_t R, int64_t nre,
               int32_t rpc, void* sym, int64_t ldsym, float* nv, int64_t ldnv) {
#define LDPC5G_EQ_SHAPE(NR, NLL)                                                                          \
    launch_eq_algo<NR, NLL, C>(algo, grid, st, (const C*)y, ldy, (const C*)h, ldh, (const C*)cov, ldcov, re_idx, R, \
                               nre, rpc, (C*)sym, ldsym, nv, ldnv)
    switch (Nr * 8 + NL) {
        case 1 * 8 + 1: LDPC5G_EQ_SHAPE(1, 1); break;
        case 2 * 8 + 1: LDPC5G_EQ_SHAPE(2, 1); break;
        case 2 * 8 + 2: LDPC5G_EQ_SHAPE(2, 2); break;
        case 4 * 8 + 1: LDPC5G_EQ_SHAPE(4, 1); break;
        case 4 * 8 + 2: LDPC5G_EQ_SHAPE(4, 2); break;
        case 4 * 8 + 3: LDPC5G_EQ_SHAPE(4, 3); break;
        default: LDPC5G_EQ_SHAPE(4, 4); break;
    }
#undef LDPC5G_EQ_SHAPE
}

}  // namespace
}  // namespace ldpc5g_impl

using namespace ldpc5g_impl;

extern "C" {

int ldpc5g_equalize(const void* y, int64_t ldy, const void* h, int64_t ldh, const void* cov, int64_t ldcov,
                    int32_t in_dtype, const int32_t* re_idx, int64_t R, int64_t nre, int32_t re_per_cov, int32_t T,
                    int32_t Nr, int32_t NL, int32_t algo, void* sym, int64_t ldsym, float* noise_var, int64_t ldnv,
                    void* stream) {
    clear_error();
    if (!(Nr == 1 || Nr == 2 || Nr == 4) || NL < 1 || NL > Nr)
        return fail(LDPC5G_ESIZE, "Nr=%d NL=%d (Nr in {1, 2, 4}, 1 <= NL <= Nr)", Nr, NL);
    if (algo < LDPC5G_EQ_ZF || algo > LDPC5G_EQ_MMSE_IRC)
        return fail(LDPC5G_ESIZE, "bad algo %d (0 ZF, 1 ZF-IRC, 2 MMSE, 3 MMSE-IRC)", algo);
    if (in_dtype != LDPC5G_F32 && in_dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad dtype %d", in_dtype);
    if (re_per_cov < 1) return fail(LDPC5G_ESIZE, "bad re_per_cov %d", re_per_cov);
    if (T <= 0 || R <= 0 || nre <= 0 || nre > R || R > INT32_MAX || T > 65535)
        return fail(LDPC5G_ESIZE, "bad sizes T=%d R=%lld nre=%lld", T, (long long)R, (long long)nre);
    if (!re_idx && nre != R)
        return fail(LDPC5G_ESIZE, "bad sizes: re_idx NULL means all R=%lld resource elements, nre=%lld", (long long)R,
                    (long long)nre);
    const int64_t ncov = (R + re_per_cov - 1) / re_per_cov;
    if (ldy < R * Nr || ldh < R * Nr * NL || ldcov < ncov * Nr * Nr || ldsym < nre * NL || ldnv < nre * NL)
        return fail(LDPC5G_ESIZE, "bad strides: a row stride is shorter than its row");
    if (!y || !h || !cov || !sym || !noise_var) return fail(LDPC5G_ESIZE, "null buffer");
    const dim3 grid((unsigned)((nre + kEqThreads - 1) / kEqThreads), T);
    hipStream_t st = (hipStream_t)stream;
    if (in_dtype == LDPC5G_F64)
        launch_eq<double2>(Nr, NL, algo, grid, st, y, ldy, h, ldh, cov, ldcov, re_idx, R, nre, re_per_cov, sym, ldsym,
                           noise_var, ldnv);
    else
        launch_eq<float2>(Nr, NL, algo, grid, st, y, ldy, h, ldh, cov, ldcov, re_idx, R, nre, re_per_cov, sym, ldsym,
                          noise_var, ldnv);
    return check_hip(hipGetLastError(), "equalize launch");
}

}  // extern "C"
