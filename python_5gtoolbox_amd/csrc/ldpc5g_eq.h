// ldpc5g_eq.h — the per-resource-element building blocks shared by the linear equaliser
// (ldpc5g_eq.hip) and the maximum-likelihood detectors (ldpc5g_ml.hip): complex float64 helpers,
// the widening loader, the Hermitian matrix type, its inverse through the unpivoted LDL^H
// factorisation and the pivot rule that stands in for the reference's matrix_rank test
// (include/ldpc5g.h, "Regularisation").  Everything is a fully unrolled register computation:
// all loop bounds and indices are compile-time constants.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ldpc5g_common.h"

namespace ldpc5g_impl {
namespace {

struct cx {
    double re, im;
};
__device__ __forceinline__ cx cmul(cx a, cx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
// conj(a) * b
__device__ __forceinline__ cx cmulc(cx a, cx b) { return {a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re}; }
// a * conj(b)
__device__ __forceinline__ cx cmulcb(cx a, cx b) { return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im}; }
__device__ __forceinline__ cx cscale(cx a, double s) { return {a.re * s, a.im * s}; }
__device__ __forceinline__ void cacc(cx& s, cx p) { s.re += p.re, s.im += p.im; }
__device__ __forceinline__ void csub(cx& s, cx p) { s.re -= p.re, s.im -= p.im; }

template <typename C>
__device__ __forceinline__ cx widen(C v) { return {(double)v.x, (double)v.y}; }

// Hermitian N x N matrix: a[i][j] is meaningful for i >= j only, and a[i][i].im is never read.
template <int N>
struct Herm {
    cx a[N][N];
};
template <int N>
__device__ __forceinline__ cx herm_at(const Herm<N>& A, int i, int j) {   // i, j compile-time after unrolling
    if (i == j) return {A.a[i][i].re, 0.0};
    if (i > j) return A.a[i][j];
    return {A.a[j][i].re, -A.a[j][i].im};
}

// max_ij |A_ij| (np.abs(A).max())
template <int N>
__device__ __forceinline__ double herm_maxabs(const Herm<N>& A) {
    double m = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = 0; j < i; ++j) m = fmax(m, sqrt(A.a[i][j].re * A.a[i][j].re + A.a[i][j].im * A.a[i][j].im));
        m = fmax(m, fabs(A.a[i][i].re));
    }
    return m;
}

// V = A^-1 through the unpivoted LDL^H factorisation.  Returns whether every pivot exceeds thr
// (false also for a NaN pivot); V is meaningless then.
template <int N>
__device__ __forceinline__ bool herm_inverse(const Herm<N>& A, double thr, Herm<N>& V) {
    cx L[N][N], M[N][N];
    double d[N], rd[N];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double dj = A.a[j][j].re;
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= (L[j][k].re * L[j][k].re + L[j][k].im * L[j][k].im) * d[k];
        d[j] = dj;
        ok = ok && (dj > thr);
        rd[j] = 1.0 / dj;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            cx s = A.a[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) csub(s, cscale(cmulcb(L[i][k], L[j][k]), d[k]));
            L[i][j] = cscale(s, rd[j]);
        }
    }
    // M = L^-1 (unit lower triangular)
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            cx s = {-L[i][j].re, -L[i][j].im};
#pragma unroll
            for (int k = j + 1; k < i; ++k) csub(s, cmul(L[i][k], M[k][j]));
            M[i][j] = s;
        }
    }
    // V = M^H D^-1 M, lower triangle
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            cx s = (j == i) ? cx{rd[i], 0.0} : cscale(M[i][j], rd[i]);
#pragma unroll
            for (int k = i + 1; k < N; ++k) cacc(s, cscale(cmulc(M[k][i], M[k][j]), rd[k]));
            V.a[i][j] = s;
        }
    }
    return ok;
}

// The reference's "if matrix_rank(A) < n: A += 0.0012 * abs(A).max() * I" followed by inv(A),
// with the pivot rule in place of the SVD.
template <int N>
__device__ __forceinline__ void herm_inverse_reg(Herm<N>& A, Herm<N>& V) {
    const double mx = herm_maxabs(A);
    if (!herm_inverse(A, 0x1p-40 * mx, V)) {
        const double add = mx * 0.0012;
#pragma unroll
        for (int i = 0; i < N; ++i) A.a[i][i].re += add;
        herm_inverse(A, 0.0, V);
    }
}

}  // namespace
}  // namespace ldpc5g_impl
