// ldpc5g_ml.hip — batched maximum-likelihood MIMO detection, the second producer of the receive
// chain: it emits LLRs directly (ldpc5g_ml_detect, include/ldpc5g.h), bypassing the demodulator.
//   ML-soft / ML-hard (+IRC) ....... py5gphy/channel_equalization/ML.py:47-98 / :9-45
//   ML2-soft (+IRC) ................ ML2.py:47-161 / :9-45
//   MMSE-ML (+IRC) ................. MMSE_ML.py:47-105 / :12-45
//   opt-rank2-ML (+IRC) ............ opt_rank2_ML.py:38-171 / :9-36
// called once per resource element by channel_equ_and_demod (nr_channel_eq.py:27-46).
//
// Constellation.  The points are get_mod_list's (nrModulation.py:47-74): the float32 results of
// nrModulate, widened to float64; point index m has the binary digits of m, MSB first, as its
// bits.  They are rebuilt with the mapper arithmetic of scramble_modulate_kernel (exact integer
// levels times the float32 reciprocal of sqrt(scale)) into an LDS table per workgroup.  pi/2-BPSK
// equals BPSK here: get_mod_list and get_oppisite_syms only ever modulate symbol index 0, whose
// pi/2 rotation is the identity (a quirk of the reference, kept).
//
// Per resource element: load Y, H and the covariance of its block as ldpc5g_equalize does.
// Without IRC sigma^2 = mean(diag(cov)).real.  With IRC the system is whitened by U = D^-1/2 L^-1
// of the unpivoted LDL^H factorisation cov = L D L^H (U^H U = cov^-1; the metric does not depend
// on which such U is used, the reference takes one from eigh) and sigma^2 = 1; cov is regularised
// by the pivot rule of ldpc5g_eq.h first.  The metric is the direct form
//   v(S) = sum_q |Y_q - sum_l H_ql S_l|^2 / sigma^2
// in float64, whatever the storage type.
//
// Lane mapping (template TPR = lanes per resource element):
//   exhaustive search, M^NL <= 64 ........... one thread per RE
//                      M^NL <= 4096 ......... one wave per RE (4 REs per workgroup)
//                      M^NL <= 65536 ........ one 256-thread workgroup per RE
//   subset (MMSE-ML) and rank-2 searches .... one thread per RE
// Lane j evaluates candidates j, j + TPR, ... in itertools.product order (layer 0 slowest) and
// keeps a running (min, argmin) — for ML2 also min0 / min1 of each of the NL*Qm <= 16 bits, all in
// registers — which are reduced across the wave by shuffles and across waves through LDS.  Ties
// go to the lowest candidate index, as the reference's strict `<` gives.
#include "ldpc5g_eq.h"
#include "ldpc5g_demod.h"

namespace ldpc5g_impl {
namespace {

constexpr int kMlThreads = 256;
constexpr int kMlMaxPoints = 1024;   // 1024QAM
constexpr int kMlMaxBits = 16;       // exhaustive search: NL * Qm <= 16, 65 536 candidates

enum { kModeExh = 0, kModeSubset = 1, kModeRank2 = 2 };

struct MlArgs {
    const void *y, *h, *cov;
    int64_t ldy, ldh, ldcov;
    const int32_t* re_idx;
    int64_t R, nre;
    int32_t rpc, Qm, irc, hard;
    float scl;
    const uint32_t* prbs;
    int64_t ldw;
    void* llr;
    int32_t llr_f32;
    int64_t ldllr;
    float2* sym;
    int64_t ldsym;
    void* nv;
    int64_t ldnv;
    int8_t* hb;
    int64_t ldhb;
};

// value of the PAM level whose HQ bits (MSB first) are k: u0 (2^(HQ-1) - u1 (... (2 - u_{HQ-1})))
// with u = 1 - 2 bit, in float32, times scl (nrModulation.py:24-44)
__device__ __forceinline__ double axis_value(int k, int HQ, float scl) {
    float t = 1.0f - 2.0f * (float)(k & 1);
    for (int j = HQ - 2; j >= 0; --j) {
        const float u = 1.0f - 2.0f * (float)((k >> (HQ - 1 - j)) & 1);
        t = u * ((float)(1 << (HQ - 1 - j)) - t);
    }
    return (double)(t * scl);
}
// point index m (Qm bits, MSB first: b0 b1 b2 ...) -> real-axis pattern (b0 b2 ...) and
// imaginary-axis pattern (b1 b3 ...)
__device__ __forceinline__ void split_axes(int m, int HQ, int& kx, int& ky) {
    kx = 0, ky = 0;
    for (int j = 0; j < HQ; ++j) {
        const int two = (m >> (2 * (HQ - 1 - j))) & 3;
        kx = (kx << 1) | (two >> 1);
        ky = (ky << 1) | (two & 1);
    }
}
__device__ __forceinline__ int join_axes(int kx, int ky, int HQ) {
    int m = 0;
    for (int j = 0; j < HQ; ++j)
        m = (m << 2) | (((kx >> (HQ - 1 - j)) & 1) << 1) | ((ky >> (HQ - 1 - j)) & 1);
    return m;
}
// get_oppisite_syms (nrModulation.py:76-137): flip bit b of the point; of the later bits on the
// same axis the first becomes 0 and the rest 1 (the nearest point with the other value of bit b)
__device__ __forceinline__ int opposite_point(int m, int b, int Qm) {
    int r = m ^ (1 << (Qm - 1 - b));
    for (int j = b + 2; j < Qm; j += 2) {
        const int bit = 1 << (Qm - 1 - j);
        r = (j == b + 2) ? (r & ~bit) : (r | bit);
    }
    return r;
}

// U = D^-1/2 L^-1 of cov = L D L^H, as M = L^-1 (unit lower triangular) and rs = d^-1/2, with the
// regularisation of herm_inverse_reg: cov += 0.0012 max|cov| I when NOT(min d_k > 2^-40 max|cov|).
template <int N>
__device__ __forceinline__ bool herm_ldl(const Herm<N>& A, double thr, cx (&M)[N][N], double (&rs)[N]) {
    cx L[N][N];
    double d[N];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double dj = A.a[j][j].re;
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= (L[j][k].re * L[j][k].re + L[j][k].im * L[j][k].im) * d[k];
        d[j] = dj;
        ok = ok && (dj > thr);
        rs[j] = 1.0 / sqrt(dj);
        const double rd = 1.0 / dj;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            cx s = A.a[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) csub(s, cscale(cmulcb(L[i][k], L[j][k]), d[k]));
            L[i][j] = cscale(s, rd);
        }
    }
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
    return ok;
}
template <int N>
__device__ __forceinline__ void herm_whitener(Herm<N>& A, cx (&M)[N][N], double (&rs)[N]) {
    const double mx = herm_maxabs(A);
    if (!herm_ldl(A, 0x1p-40 * mx, M, rs)) {
        const double add = mx * 0.0012;
#pragma unroll
        for (int i = 0; i < N; ++i) A.a[i][i].re += add;
        herm_ldl(A, 0.0, M, rs);
    }
}

// The MMSE / MMSE-IRC estimate of equalize_kernel (MMSE.py:58-103 / :5-56), symbols only.
template <int NR, int NL>
__device__ __forceinline__ void mmse_estimate(const cx (&Y)[NR], const cx (&H)[NR][NL], Herm<NR> Cv, bool irc,
                                              cx (&s)[NL]) {
    if constexpr (NR == 1) {
        const double hh = H[0][0].re * H[0][0].re + H[0][0].im * H[0][0].im;
        const cx p = cmulcb(Y[0], H[0][0]);
        s[0] = {p.re / hh, p.im / hh};
    } else {
        cx z[NL];
        Herm<NL> W1, V;
        double rs = 1.0;
        if (irc) {
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
            double sigma2 = 0.0;
#pragma unroll
            for (int q = 0; q < NR; ++q) sigma2 += Cv.a[q][q].re;
            sigma2 = sigma2 / NR;
            rs = 1.0 / sigma2;
#pragma unroll
            for (int a = 0; a < NL; ++a) {
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                    cx acc = {0.0, 0.0};
#pragma unroll
                    for (int q = 0; q < NR; ++q) cacc(acc, cmulc(H[q][a], H[q][b]));
                    W1.a[a][b] = cscale(acc, rs);
                }
                W1.a[a][a].re += 1.0;
                cx acc = {0.0, 0.0};
#pragma unroll
                for (int q = 0; q < NR; ++q) cacc(acc, cmulc(H[q][a], Y[q]));
                z[a] = acc;
            }
        }
        herm_inverse_reg(W1, V);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            cx acc = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < NL; ++k) cacc(acc, cmul(herm_at(V, l, k), z[k]));
            if (!irc) acc = cscale(acc, rs);
            const double comp = 1.0 - V.a[l][l].re;
            s[l] = {acc.re / comp, acc.im / comp};
        }
    }
}

// (Y - H S)^H (Y - H S) / sigma^2 in the reference's order (ML.py:159-164)
template <int NR, int NL>
__device__ __forceinline__ double ml_metric(const cx (&Y)[NR], const cx (&H)[NR][NL], const cx (&S)[NL],
                                            double sigma2) {
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        cx hs = {0.0, 0.0};
#pragma unroll
        for (int l = 0; l < NL; ++l) cacc(hs, cmul(H[q][l], S[l]));
        const double dr = Y[q].re - hs.re, di = Y[q].im - hs.im;
        acc += dr * dr + di * di;
    }
    return acc / sigma2;
}

__device__ __forceinline__ void take_min(double& v, uint32_t& c, double ov, uint32_t oc) {
    if (ov < v || (ov == v && oc < c)) v = ov, c = oc;
}

template <int NR, int NL, typename C, int MODE, int TPR, bool ML2>
__global__ __launch_bounds__(kMlThreads) void ml_detect_kernel(const MlArgs a) {
    static_assert(MODE == kModeExh || (TPR == 1 && !ML2), "subset and rank-2 searches: one thread per RE");
    constexpr int NE = NR * NL;
    constexpr int RPB = kMlThreads / TPR;   // resource elements per workgroup
    constexpr int NB16 = ML2 ? kMlMaxBits : 1;
    __shared__ cx pts[kMlMaxPoints];
    __shared__ double ax[32];
    __shared__ double red_v[ML2 ? 4 * (1 + 2 * kMlMaxBits) : 4];
    __shared__ uint32_t red_c[4];

    const int Qm = a.Qm, M = 1 << Qm, HQ = Qm >> 1, NA = Qm == 1 ? 2 : 1 << HQ;
    const int NB = NL * Qm;
    for (int k = threadIdx.x; k < NA; k += kMlThreads) ax[k] = Qm == 1 ? axis_value(k, 1, a.scl) : axis_value(k, HQ, a.scl);
    for (int m = threadIdx.x; m < M; m += kMlThreads) {
        if (Qm == 1) {
            const double v = axis_value(m, 1, a.scl);
            pts[m] = {v, v};
        } else {
            int kx, ky;
            split_axes(m, HQ, kx, ky);
            pts[m] = {axis_value(kx, HQ, a.scl), axis_value(ky, HQ, a.scl)};
        }
    }
    __syncthreads();

    const int t = blockIdx.y;
    const int lane = TPR == 1 ? 0 : (int)(threadIdx.x % TPR);
    const int64_t i = (int64_t)blockIdx.x * RPB + threadIdx.x / TPR;
    const bool live = i < a.nre;
    int64_t r = live ? (a.re_idx ? (int64_t)a.re_idx[i] : i) : -1;
    const bool valid = live && r >= 0 && r < a.R;   // an index outside 0..R-1 reads nothing: NaN out
    if (!valid) r = 0;   // R >= 1: a readable RE, its result is discarded

    // ---- prologue: Y, H, cov of this RE; whitening (every lane of the RE's group repeats it)
    cx H[NR][NL], Y[NR];
    const C* hT = (const C*)a.h + (int64_t)t * a.ldh + r * NE;
    const C* yT = (const C*)a.y + (int64_t)t * a.ldy + r * NR;
    const C* cT = (const C*)a.cov + (int64_t)t * a.ldcov + (r / a.rpc) * (NR * NR);
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        Y[q] = widen(yT[q]);
#pragma unroll
        for (int l = 0; l < NL; ++l) H[q][l] = widen(hT[q * NL + l]);
    }
    const bool irc = a.irc != 0;
    Herm<NR> Cv;
#pragma unroll
    for (int p = 0; p < NR; ++p) {
#pragma unroll
        for (int b = 0; b <= p; ++b) Cv.a[p][b] = (irc || p == b) ? widen(cT[p * NR + b]) : cx{0.0, 0.0};
    }
    cx est[NL];   // MMSE-ML: the linear estimate on the system as given
    if constexpr (MODE == kModeSubset) mmse_estimate<NR, NL>(Y, H, Cv, irc, est);
    double sigma2 = 1.0;
    if (irc) {
        cx Mi[NR][NR];
        double rs[NR];
        herm_whitener(Cv, Mi, rs);
        cx Yw[NR], Hw[NR][NL];
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            cx s = Y[q];
#pragma unroll
            for (int k = 0; k < q; ++k) cacc(s, cmul(Mi[q][k], Y[k]));
            Yw[q] = cscale(s, rs[q]);
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                cx w = H[q][l];
#pragma unroll
                for (int k = 0; k < q; ++k) cacc(w, cmul(Mi[q][k], H[k][l]));
                Hw[q][l] = cscale(w, rs[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            Y[q] = Yw[q];
#pragma unroll
            for (int l = 0; l < NL; ++l) H[q][l] = Hw[q][l];
        }
    } else {
        sigma2 = 0.0;
#pragma unroll
        for (int q = 0; q < NR; ++q) sigma2 += Cv.a[q][q].re;
        sigma2 = sigma2 / NR;   // np.mean(np.diagonal(cov)).real
    }

    // ---- search
    double minv = INFINITY;
    int idx[NL];   // decided point index per layer
    cx S[NL];      // decided points
    double mn0[NB16], mn1[NB16];   // ML2: indexed by bit position from the LSB of the candidate
    if constexpr (MODE == kModeExh) {
        uint32_t best = 0xffffffffu;
        if constexpr (ML2) {
#pragma unroll
            for (int p = 0; p < NB16; ++p) mn0[p] = INFINITY, mn1[p] = INFINITY;
        }
        const uint32_t ncand = 1u << NB;
        for (uint32_t c = lane; c < ncand; c += TPR) {
            cx Sc[NL];
#pragma unroll
            for (int l = 0; l < NL; ++l) Sc[l] = pts[(c >> (Qm * (NL - 1 - l))) & (M - 1)];
            const double v = ml_metric<NR, NL>(Y, H, Sc, sigma2);
            if (v < minv) minv = v, best = c;
            if constexpr (ML2) {
#pragma unroll
                for (int p = 0; p < NB16; ++p) {
                    if ((c >> p) & 1u) mn1[p] = fmin(mn1[p], v);
                    else mn0[p] = fmin(mn0[p], v);
                }
            }
        }
        if constexpr (TPR > 1) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double ov = __shfl_xor(minv, off);
                const uint32_t oc = (uint32_t)__shfl_xor((int)best, off);
                take_min(minv, best, ov, oc);
                if constexpr (ML2) {
#pragma unroll
                    for (int p = 0; p < NB16; ++p) {
                        mn0[p] = fmin(mn0[p], __shfl_xor(mn0[p], off));
                        mn1[p] = fmin(mn1[p], __shfl_xor(mn1[p], off));
                    }
                }
            }
        }
        if constexpr (TPR == kMlThreads) {   // four waves of one RE: through LDS
            constexpr int W = ML2 ? 1 + 2 * kMlMaxBits : 1;
            const int w = threadIdx.x >> 6;
            if ((threadIdx.x & 63) == 0) {
                red_v[w * W] = minv, red_c[w] = best;
                if constexpr (ML2) {
#pragma unroll
                    for (int p = 0; p < NB16; ++p) red_v[w * W + 1 + p] = mn0[p], red_v[w * W + 1 + NB16 + p] = mn1[p];
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) {
#pragma unroll
                for (int k = 1; k < 4; ++k) {
                    take_min(minv, best, red_v[k * W], red_c[k]);
                    if constexpr (ML2) {
#pragma unroll
                        for (int p = 0; p < NB16; ++p) {
                            mn0[p] = fmin(mn0[p], red_v[k * W + 1 + p]);
                            mn1[p] = fmin(mn1[p], red_v[k * W + 1 + NB16 + p]);
                        }
                    }
                }
            }
        }
        if (best == 0xffffffffu) best = 0;   // every metric NaN
#pragma unroll
        for (int l = 0; l < NL; ++l) idx[l] = (best >> (Qm * (NL - 1 - l))) & (M - 1);
    } else if constexpr (MODE == kModeSubset) {
        // per layer the min(4, M) points nearest the MMSE estimate, nearest first
        // (MMSE_ML.py:89-95), packed 10 bits each
        const int kb = M < 4 ? Qm : 2, K = 1 << kb;
        uint64_t sel[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            double d0 = INFINITY, d1 = INFINITY, d2 = INFINITY, d3 = INFINITY;
            int i0 = 0, i1 = 0, i2 = 0, i3 = 0;
            for (int m = 0; m < M; ++m) {
                const double dr = pts[m].re - est[l].re, di = pts[m].im - est[l].im;
                const double d = dr * dr + di * di;
                if (d < d3) {
                    d3 = d, i3 = m;
                    if (d3 < d2) { const double td = d2; d2 = d3, d3 = td; const int ti = i2; i2 = i3, i3 = ti; }
                    if (d2 < d1) { const double td = d1; d1 = d2, d2 = td; const int ti = i1; i1 = i2, i2 = ti; }
                    if (d1 < d0) { const double td = d0; d0 = d1, d1 = td; const int ti = i0; i0 = i1, i1 = ti; }
                }
            }
            sel[l] = (uint64_t)i0 | ((uint64_t)i1 << 10) | ((uint64_t)i2 << 20) | ((uint64_t)i3 << 30);
        }
        uint64_t bestsel = 0;
        const uint32_t ncand = 1u << (kb * NL);
        for (uint32_t c = 0; c < ncand; ++c) {
            cx Sc[NL];
            uint64_t code = 0;
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const int dgt = (c >> (kb * (NL - 1 - l))) & (K - 1);
                const int m = (int)((sel[l] >> (10 * dgt)) & 1023u);
                Sc[l] = pts[m];
                code = (code << 10) | (uint64_t)m;
            }
            const double v = ml_metric<NR, NL>(Y, H, Sc, sigma2);
            if (v < minv) minv = v, bestsel = code;
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) idx[l] = (int)((bestsel >> (10 * (NL - 1 - l))) & 1023u);
    } else {
        // opt_rank2_ML.py:62-109 (NL == 2): for each s0 the best s1 is found per axis.  The
        // reference also runs the mirrored loop over s1 and asserts that both agree; its result is
        // the first loop's, which is all that is computed here.
        static_assert(MODE != kModeRank2 || NL == 2, "rank-2 search");
        cx yh0 = {0.0, 0.0}, yh1 = {0.0, 0.0}, h01 = {0.0, 0.0};
        double a2 = 0.0, a3 = 0.0, yy = 0.0;
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            cacc(yh0, cmulc(Y[q], H[q][0]));
            cacc(yh1, cmulc(Y[q], H[q][NL - 1]));
            cacc(h01, cmulc(H[q][0], H[q][NL - 1]));
            a2 += cmulc(H[q][0], H[q][0]).re;
            a3 += cmulc(H[q][NL - 1], H[q][NL - 1]).re;
            yy += cmulc(Y[q], Y[q]).re;
        }
        const double a0i = yh0.re, a0q = yh0.im, a1i = yh1.re, a1q = yh1.im, a4i = h01.re, a4q = h01.im;
        double L2min = INFINITY;
        int b0 = 0, bkx = 0, bky = 0;
        for (int m = 0; m < M; ++m) {
            const double x0 = pts[m].re, y0 = pts[m].im;
            const float fx = (float)x0, fy = (float)y0;   // x0**2 + y0**2 is float32 in the reference
            const double L21 = a2 * (double)(fx * fx + fy * fy) - 2.0 * a0i * x0 + 2.0 * a0q * y0;
            const double gx = -a1i + a4i * x0 + a4q * y0, gy = a1q + a4i * y0 - a4q * x0;
            const double xh = -gx / a3, yh = -gy / a3;
            int kx = 0, ky = 0;
            double dx = fabs(ax[0] - xh), dy = fabs(ax[0] - yh);
            for (int k = 1; k < NA; ++k) {   // nearest level (a3 > 0), else the farthest
                const double ex = fabs(ax[k] - xh), ey = fabs(ax[k] - yh);
                if (a3 > 0 ? ex < dx : ex > dx) dx = ex, kx = k;
                if (a3 > 0 ? ey < dy : ey > dy) dy = ey, ky = k;
            }
            const double cx1 = ax[kx], cy1 = ax[ky];
            const double L22 = a3 * cx1 * cx1 + 2.0 * gx * cx1;
            const double L23 = a3 * cy1 * cy1 + 2.0 * gy * cy1;
            const double L2 = L21 + L22 + L23;
            if (L2 < L2min) L2min = L2, b0 = m, bkx = kx, bky = ky;
        }
        minv = (yy + L2min) / sigma2;
        idx[0] = b0;
        // BPSK: the two axes are sliced independently, so re != im can come out; bit = real axis
        idx[NL - 1] = Qm == 1 ? bkx : join_axes(bkx, bky, HQ);
        S[NL - 1] = {ax[bkx], ax[bky]};
    }
    if (lane != 0 || !live) return;

    // ---- outputs, by the first lane of the RE's group
    const int64_t o = i * NL;
    int8_t* hbo = a.hb ? a.hb + (int64_t)t * a.ldhb + o * Qm : nullptr;
    float2* so = a.sym ? a.sym + (int64_t)t * a.ldsym + o : nullptr;
    const uint32_t* w = a.prbs ? a.prbs + (int64_t)t * a.ldw : nullptr;
    auto put = [&](int64_t n, double v) {
        if (a.llr_f32) ((float*)a.llr)[(int64_t)t * a.ldllr + n] = (float)v;
        else ((double*)a.llr)[(int64_t)t * a.ldllr + n] = v;
    };
    if (!valid) {
        for (int n = 0; n < NB; ++n) {
            put(o * Qm + n, NAN);
            if (hbo) hbo[n] = 0;
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (so) so[l] = make_float2(NAN, NAN);
            if (a.nv) {
                if (a.llr_f32) ((float*)a.nv)[(int64_t)t * a.ldnv + o + l] = NAN;
                else ((double*)a.nv)[(int64_t)t * a.ldnv + o + l] = NAN;
            }
        }
        return;
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        if (MODE != kModeRank2 || l == 0) S[l] = pts[idx[l]];
        if (so) so[l] = make_float2((float)S[l].re, (float)S[l].im);
        if (a.nv) {
            if (a.llr_f32) ((float*)a.nv)[(int64_t)t * a.ldnv + o + l] = (float)minv;
            else ((double*)a.nv)[(int64_t)t * a.ldnv + o + l] = minv;
        }
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const uint32_t c = w ? prbs_bits(w, (o + l) * Qm, Qm) : 0u;
        for (int m = 0; m < Qm; ++m) {
            const int bit = (idx[l] >> (Qm - 1 - m)) & 1;
            if (hbo) hbo[l * Qm + m] = (int8_t)bit;
            if constexpr (ML2) continue;
            double v;
            if (a.hard) {
                v = 1.0 - 2.0 * bit;
            } else {   // ML_soft_LLR_est, ML.py:100-139
                cx So[NL];
#pragma unroll
                for (int k = 0; k < NL; ++k) So[k] = S[k];
                So[l] = pts[opposite_point(idx[l], m, Qm)];
                const double dis = ml_metric<NR, NL>(Y, H, So, sigma2);
                v = bit ? minv - dis : -minv + dis;
            }
            put((o + l) * Qm + m, flip_sign(v, (c >> m) & 1u));
        }
    }
    if constexpr (ML2) {   // min over candidates with the bit 1 minus with the bit 0 (ML2.py:138-160)
#pragma unroll
        for (int p = 0; p < NB16; ++p) {
            if (p < NB) {
                const int n = NB - 1 - p;
                const uint32_t c = w ? prbs_bits(w, o * Qm + n, 1) : 0u;
                put(o * Qm + n, flip_sign(mn1[p] - mn0[p], c));
            }
        }
    }
}

template <int NR, int NL, typename C, int MODE, int TPR, bool ML2>
void launch_ml_one(const MlArgs& a, int T, hipStream_t st) {
    constexpr int RPB = kMlThreads / TPR;
    const dim3 grid((unsigned)((a.nre + RPB - 1) / RPB), T);
    hipLaunchKernelGGL((ml_detect_kernel<NR, NL, C, MODE, TPR, ML2>), grid, dim3(kMlThreads), 0, st, a);
}

template <int NR, int NL, typename C>
void launch_ml_shape(const MlArgs& a, int mode, bool ml2, int T, hipStream_t st) {
    if (mode == kModeSubset) return launch_ml_one<NR, NL, C, kModeSubset, 1, false>(a, T, st);
    if constexpr (NL == 2)
        if (mode == kModeRank2) return launch_ml_one<NR, NL, C, kModeRank2, 1, false>(a, T, st);
    const int nb = NL * a.Qm;
    if (nb <= 6) {
        if (ml2) launch_ml_one<NR, NL, C, kModeExh, 1, true>(a, T, st);
        else launch_ml_one<NR, NL, C, kModeExh, 1, false>(a, T, st);
    } else if (nb <= 12) {
        if (ml2) launch_ml_one<NR, NL, C, kModeExh, 64, true>(a, T, st);
        else launch_ml_one<NR, NL, C, kModeExh, 64, false>(a, T, st);
    } else {
        if (ml2) launch_ml_one<NR, NL, C, kModeExh, kMlThreads, true>(a, T, st);
        else launch_ml_one<NR, NL, C, kModeExh, kMlThreads, false>(a, T, st);
    }
}

template <typename C>
void launch_ml(int Nr, int NL, const MlArgs& a, int mode, bool ml2, int T, hipStream_t st) {
    switch (Nr * 8 + NL) {
        case 1 * 8 + 1: launch_ml_shape<1, 1, C>(a, mode, ml2, T, st); break;
        case 2 * 8 + 1: launch_ml_shape<2, 1, C>(a, mode, ml2, T, st); break;
        case 2 * 8 + 2: launch_ml_shape<2, 2, C>(a, mode, ml2, T, st); break;
        case 4 * 8 + 1: launch_ml_shape<4, 1, C>(a, mode, ml2, T, st); break;
        case 4 * 8 + 2: launch_ml_shape<4, 2, C>(a, mode, ml2, T, st); break;
        case 4 * 8 + 3: launch_ml_shape<4, 3, C>(a, mode, ml2, T, st); break;
        default: launch_ml_shape<4, 4, C>(a, mode, ml2, T, st); break;
    }
}

}  // namespace
}  // namespace ldpc5g_impl

using namespace ldpc5g_impl;

extern "C" {

int ldpc5g_ml_detect(const void* y, int64_t ldy, const void* h, int64_t ldh, const void* cov, int64_t ldcov,
                     int32_t in_dtype, const int32_t* re_idx, int64_t R, int64_t nre, int32_t re_per_cov, int32_t T,
                     int32_t Nr, int32_t NL, int32_t mod, int32_t algo, int32_t irc, const uint32_t* prbs,
                     int64_t ldw, void* llr, int32_t llr_dtype, int64_t ldllr, void* sym, int64_t ldsym,
                     void* noise_var, int64_t ldnv, int8_t* hardbits, int64_t ldhb, void* stream) {
    clear_error();
    if (!(Nr == 1 || Nr == 2 || Nr == 4) || NL < 1 || NL > Nr)
        return fail(LDPC5G_ESIZE, "Nr=%d NL=%d (Nr in {1, 2, 4}, 1 <= NL <= Nr)", Nr, NL);
    if (!mod_ok(mod)) return fail(LDPC5G_ESIZE, "modulation %d (1 BPSK, -1 pi/2-BPSK, 2/4/6/8/10 QPSK..1024QAM)", mod);
    if (algo < LDPC5G_ML_SOFT || algo > LDPC5G_ML_OPT_RANK2)
        return fail(LDPC5G_ESIZE, "bad algo %d (0 ML-soft, 1 ML-hard, 2 ML2-soft, 3 MMSE-ML, 4 opt-rank2-ML)", algo);
    if (irc != 0 && irc != 1) return fail(LDPC5G_ESIZE, "bad irc %d (0 or 1)", irc);
    if (in_dtype != LDPC5G_F32 && in_dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad dtype %d", in_dtype);
    if (llr_dtype != LDPC5G_F32 && llr_dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad llr dtype %d", llr_dtype);
    if (re_per_cov < 1) return fail(LDPC5G_ESIZE, "bad re_per_cov %d", re_per_cov);
    const int Qm = mod < 0 ? 1 : mod;
    int mode = kModeExh;
    if (algo == LDPC5G_ML_MMSE) mode = kModeSubset;
    else if (algo == LDPC5G_ML_OPT_RANK2 && NL == 2) mode = kModeRank2;   // NL != 2: ML-soft (opt_rank2_ML.py:44-45)
    if (mode == kModeExh && NL * Qm > kMlMaxBits)
        return fail(LDPC5G_ESIZE,
                    "exhaustive search over M^NL = 2^%d candidates (Qm=%d, NL=%d) exceeds the cap of 65536; "
                    "opt-rank2-ML searches two layers in O(M)", NL * Qm, Qm, NL);
    if (T <= 0 || R <= 0 || nre <= 0 || nre > R || R > INT32_MAX || T > 65535)
        return fail(LDPC5G_ESIZE, "bad sizes T=%d R=%lld nre=%lld", T, (long long)R, (long long)nre);
    if (!re_idx && nre != R)
        return fail(LDPC5G_ESIZE, "bad sizes: re_idx NULL means all R=%lld resource elements, nre=%lld", (long long)R,
                    (long long)nre);
    const int64_t ncov = (R + re_per_cov - 1) / re_per_cov;
    const int64_t nbits = nre * NL * Qm;
    if (ldy < R * Nr || ldh < R * Nr * NL || ldcov < ncov * Nr * Nr || ldllr < nbits || (sym && ldsym < nre * NL) ||
        (noise_var && ldnv < nre * NL) || (hardbits && ldhb < nbits) || (prbs && ldw < (nbits + 31) / 32))
        return fail(LDPC5G_ESIZE, "bad strides: a row stride is shorter than its row");
    if (!y || !h || !cov || !llr) return fail(LDPC5G_ESIZE, "null buffer");
    MlArgs a;
    a.y = y, a.h = h, a.cov = cov, a.ldy = ldy, a.ldh = ldh, a.ldcov = ldcov;
    a.re_idx = re_idx, a.R = R, a.nre = nre, a.rpc = re_per_cov, a.Qm = Qm, a.irc = irc;
    a.hard = algo == LDPC5G_ML_HARD;
    a.scl = 1.0f / (float)sqrt((double)mod_scale(Qm));
    a.prbs = prbs, a.ldw = ldw, a.llr = llr, a.llr_f32 = llr_dtype == LDPC5G_F32, a.ldllr = ldllr;
    a.sym = (float2*)sym, a.ldsym = ldsym, a.nv = noise_var, a.ldnv = ldnv, a.hb = hardbits, a.ldhb = ldhb;
    hipStream_t st = (hipStream_t)stream;
    const bool ml2 = algo == LDPC5G_ML2_SOFT;
    if (in_dtype == LDPC5G_F64) launch_ml<double2>(Nr, NL, a, mode, ml2, T, st);
    else launch_ml<float2>(Nr, NL, a, mode, ml2, T, st);
    return check_hip(hipGetLastError(), "ml_detect launch");
}

}  // extern "C"
