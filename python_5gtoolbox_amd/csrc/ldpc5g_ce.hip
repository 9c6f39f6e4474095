// ldpc5g_ce.hip — batched DMRS channel estimation, the producer of the equaliser's and the ML
// detectors' `h` and `cov` (ldpc5g_channel_estimate / ldpc5g_to_compensate, include/ldpc5g.h):
//   DFT / DCT .................. py5gphy/channel_estimate/dft_dct_CE.py:10-257
//   DFT / DCT, symmetric ....... py5gphy/channel_estimate/dft_dct_symmetric_CE.py:11-118
//   timing offset .............. py5gphy/channel_estimate/nr_channel_estimation.py:66-83,150-221
// Up to three launches per call, all float64 arithmetic whatever the storage type, no atomics and
// a fixed summation order everywhere (results are bit-identical from run to run):
//   ce_to_kernel ........ (only with timing-offset work) one workgroup per slot: peak (nr, nt)
//                         pair, TO_est per DMRS symbol, their mean
//   ce_tap_kernel ....... one workgroup per (slot, DMRS symbol, nr, nt) sequence: compensation on
//                         load, edge extension, forward transform, noise power and tap mask, back
//                         transform of the kept taps, frequency interpolation and crop; writes the
//                         float64 H_est and the residual H_LS - H_est[::D] to the workspace
//   ce_expand_cov_kernel  14-symbol line fit of H_est (elementwise, HBM-bound) and, in the extra
//                         workgroups at the end of the grid, one (slot, 16-PRB group) covariance
// The transforms are direct sums (M is never a power of two: 72..1748 on real carriers), the
// forward DFT after one decimation step by the largest power of two <= 8 dividing M.
// Twiddles come from an LDS table indexed by the REDUCED integer index (k n) mod M (DFT) or
// k (2n+1) mod 4M (DCT), advanced by integer addition, and every table entry is one sincospi /
// cospi evaluation of the exact rational j/M: no running products, no sin of an unreduced argument.
#include "ldpc5g_eq.h"

// The forward DFT splits M by R = the largest power of two <= LDPC5G_CE_MAX_RADIX dividing M;
// -DLDPC5G_CE_MAX_RADIX=1 builds the direct O(M^2) sum, for the A/B timing of tools/ce_probe.py
// (DESIGN.md §4.9).
#ifndef LDPC5G_CE_MAX_RADIX
#define LDPC5G_CE_MAX_RADIX 8
#endif

namespace ldpc5g_impl {
namespace {

constexpr int kCeThreads = 256;
constexpr int kCeMaxM = 2048;
constexpr int kCePer = kCeMaxM / kCeThreads;   // transform outputs held in registers per thread
constexpr int kCeMaxS = 4;
constexpr int kCeSyms = 14;

struct CeGeom {
    int32_t S, N, Nr, Nt, D, eK, reK, M, Mh, L_left, L_right, P, ND, scs, cdm, to_comp, R;
    int32_t sym[kCeMaxS];
};
struct CeWeights {   // H(s) = sum_m w[s][m] H_est(m): the degree-1 least-squares line at symbol s
    double w[kCeSyms][kCeMaxS];
};
struct CeWork {      // workspace views (float64)
    double* to_avg;  // [T]
    double* to_est;  // [T][kCeMaxS]
    double2* hest;   // [T][S][Nr*Nt][ND]   planar per sequence
    double2* nhs;    // [T][S][Nr*Nt][N]    H_LS (compensated) - H_est[::D]
};

// fixed-order workgroup sum; `red` holds kCeThreads doubles
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = kCeThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// exp(-j 2 pi avg step n scs 1000) in the reference's operation order
// (nr_channel_estimation.py:203 with step = RE_distance, :215 with step = 1)
__device__ __forceinline__ cx to_phase(double avg, int step, int64_t n, int scs) {
    const double th = ((((2.0 * 3.141592653589793 * avg) * (double)step) * (double)n) * (double)scs) * 1000.0;
    double s, c;
    sincos(th, &s, &c);
    return {c, -s};
}

template <typename C>
__device__ __forceinline__ C narrow(cx v) {
    using S = decltype(C{}.x);
    return C{(S)v.re, (S)v.im};
}

// ------------------------------------------------------------------ timing-offset estimate
template <typename C>
__global__ __launch_bounds__(kCeThreads) void ce_to_kernel(const C* __restrict__ hls, int64_t ldhls, CeGeom g,
                                                           CeWork ws, double* __restrict__ to_est_out,
                                                           double* __restrict__ to_avg_out) {
    __shared__ double red[kCeThreads];
    __shared__ int peak_s;
    const int t = blockIdx.x, tid = threadIdx.x;
    const int NE = g.Nr * g.Nt;
    const C* x = hls + (int64_t)t * ldhls;
    // power of every (nr, nt) pair over (S, N)
    double acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0;
    for (int i = tid; i < g.S * g.N; i += kCeThreads) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (q < NE) {
                const cx v = widen(x[(int64_t)i * NE + q]);
                acc[q] += v.re * v.re + v.im * v.im;
            }
    }
    double pw[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) pw[q] = q < NE ? block_sum(acc[q], red) / (double)(g.S * g.N) : 0.0;
    if (tid == 0) {   // nt outer, nr inner, strict >: the first maximum wins (find_peak_H_LS)
        double best = 0.0;
        int loc = 0;
        for (int nt = 0; nt < g.Nt; ++nt)
            for (int nr = 0; nr < g.Nr; ++nr) {
                double p = 0.0;
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (q == nr * g.Nt + nt) p = pw[q];
                if (p > best) best = p, loc = nr * g.Nt + nt;
            }
        peak_s = loc;
    }
    __syncthreads();
    const int pk = peak_s;
    const double den = 2.0 * 3.141592653589793 * (double)g.D * (double)g.scs * 1000.0;
    double sum = 0.0;
    for (int m = 0; m < g.S; ++m) {
        double a = 0.0;
        for (int n = tid; n < g.N - 1; n += kCeThreads) {
            const cx u = widen(x[((int64_t)m * g.N + n) * NE + pk]);
            const cx v = widen(x[((int64_t)m * g.N + n + 1) * NE + pk]);
            const cx c = cmulcb(v, u);
            a += atan2(c.im, c.re) / den;
        }
        const double e = block_sum(a, red) / (double)(g.N - 1);
        sum += e;
        if (tid == 0) {
            ws.to_est[t * kCeMaxS + m] = e;
            if (to_est_out) to_est_out[(int64_t)t * g.S + m] = e;
        }
    }
    if (tid == 0) {
        const double avg = sum / (double)g.S;
        ws.to_avg[t] = avg;
        if (to_avg_out) to_avg_out[t] = avg;
    }
}

// ------------------------------------------------------------------ one sequence: steps 0-7
// LDS: xr[M], xi[M] (the extended sequence, then the kept taps, then the cropped f), the twiddle
// table (DFT: cos/sin of 2 pi j / M for j = 0..M/2; DCT: cos of pi j / (2M) for j = 0..M) and the
// reduction scratch.  8-byte structure-of-arrays accesses: a wave's sample reads hit one or two
// addresses (broadcasts), the table reads are the scattered ones and what bounds the kernel.
template <bool DCT>
__device__ __forceinline__ void tw_lookup(const double* tc, const double* ts, int j, int M, double& c, double& s) {
    if constexpr (DCT) {   // j in [0, 4M): cos(pi j / (2M)) from the quarter wave
        if (j > 2 * M) j = 4 * M - j;
        const bool neg = j > M;
        const double v = tc[neg ? 2 * M - j : j];
        c = neg ? -v : v;
        s = 0.0;
    } else {               // j in [0, M): exp(+2 pi i j / M) from the half wave
        const bool up = j > (M >> 1);
        const int jj = up ? M - j : j;
        c = tc[jj];
        const double v = ts[jj];
        s = up ? -v : v;
    }
}

template <bool DCT, typename C>
__global__ __launch_bounds__(kCeThreads) void ce_tap_kernel(const C* __restrict__ hls, int64_t ldhls, CeGeom g,
                                                            CeWork ws, C* __restrict__ hls_comp, int64_t ldhc,
                                                            C* __restrict__ h_est_out,
                                                            double* __restrict__ noise_out,
                                                            uint8_t* __restrict__ taps_out) {
    extern __shared__ __align__(16) unsigned char ce_smem[];
    const int M = g.M, N = g.N, tid = threadIdx.x;
    double* xr = (double*)ce_smem;
    double* xi = xr + M;
    double* tc = xi + M;
    double* ts = tc + (DCT ? M + 1 : (M >> 1) + 1);
    double* red = DCT ? tc + M + 2 : ts + (M >> 1) + 1;
    const int t = blockIdx.y;
    const int NE = g.Nr * g.Nt;
    const int m = blockIdx.x / NE, q = blockIdx.x - m * NE;
    const int64_t seq = ((int64_t)t * g.S + m) * NE + q;
    const C* x = hls + (int64_t)t * ldhls + (int64_t)m * N * NE + q;
    const double avg = g.to_comp ? ws.to_avg[t] : 0.0;
    const int nq = (M + kCeThreads - 1) / kCeThreads;

    // twiddle table: one sincospi / cospi per entry, of the exactly reduced index
    if constexpr (DCT) {
        for (int j = tid; j <= M; j += kCeThreads) tc[j] = cospi((double)j / (double)(2 * M));
    } else {
        for (int j = tid; j <= (M >> 1); j += kCeThreads) {
            double s, c;
            sincospi((double)(2 * j) / (double)M, &s, &c);
            tc[j] = c, ts[j] = s;
        }
    }
    // step 0 + load: the (nr, nt) column of H_LS, timing offset compensated
    for (int n = tid; n < N; n += kCeThreads) {
        cx v = widen(x[(int64_t)n * NE]);
        if (g.to_comp) {
            v = cmul(v, to_phase(avg, g.D, n, g.scs));
            if (hls_comp) hls_comp[(int64_t)t * ldhc + ((int64_t)m * N + n) * NE + q] = narrow<C>(v);
        }
        xr[g.eK + n] = v.re, xi[g.eK + n] = v.im;
    }
    __syncthreads();
    // step 1: degree-1 least-squares line through the first / last P points, evaluated outside
    {
        const int P = g.P;
        const double xm = 0.5 * (double)(P - 1);
        for (int o = tid; o < g.eK + g.reK; o += kCeThreads) {
            const bool left = o < g.eK;
            const int base = left ? g.eK : g.eK + N - P;           // LDS position of fit point 0
            const double xq = left ? (double)(o - g.eK) : (double)(P + (o - g.eK));   // in fit coordinates
            double sr = 0.0, si = 0.0, sxx = 0.0;
            for (int p = 0; p < P; ++p) sr += xr[base + p], si += xi[base + p];
            const double mr = sr / (double)P, mi = si / (double)P;
            double br = 0.0, bi = 0.0;
            for (int p = 0; p < P; ++p) {
                const double d = (double)p - xm;
                br += d * (xr[base + p] - mr), bi += d * (xi[base + p] - mi), sxx += d * d;
            }
            br = br / sxx, bi = bi / sxx;
            const int pos = left ? o : N + o;   // right: eK + N + (o - eK)
            xr[pos] = mr + br * (xq - xm), xi[pos] = mi + bi * (xq - xm);
        }
    }
    __syncthreads();
    if (M != g.Mh) {   // symmetric algorithms: append the mirrored sequence
        for (int i = tid; i < g.Mh; i += kCeThreads) xr[g.Mh + i] = xr[g.Mh - 1 - i], xi[g.Mh + i] = xi[g.Mh - 1 - i];
        __syncthreads();
    }

    // step 2: forward transform, outputs k = tid + 256 j in registers
    cx acc[kCePer];
    int idx[kCePer], stp[kCePer];
    const int mod = DCT ? 4 * M : M;
    if constexpr (DCT) {
#pragma unroll
        for (int j = 0; j < kCePer; ++j) {
            const int k = tid + j * kCeThreads;
            const int kk = k < M ? k : 0;
            acc[j] = {0.0, 0.0};
            idx[j] = kk;           // k (2n + 1) mod 4M
            stp[j] = 2 * kk;
        }
        for (int n = 0; n < M; ++n) {
            const double a = xr[n], b = xi[n];
#pragma unroll
            for (int j = 0; j < kCePer; ++j)
                if (j < nq) {
                    double c, s;
                    tw_lookup<true>(tc, ts, idx[j], M, c, s);
                    acc[j].re = fma(a, c, acc[j].re);
                    acc[j].im = fma(b, c, acc[j].im);
                    idx[j] += stp[j];
                    if (idx[j] >= mod) idx[j] -= mod;
                }
        }
    } else {
        // One decimation step by R = g.R (the largest power of two <= 8 dividing M; M is even):
        //   Y_r[k'] = sum_j x[j R + r] W^(R j k'),  k' < M/R      (M/R terms for each of M outputs)
        //   g[k]    = sum_r W^(r k) Y_r[k mod M/R]                (R terms)
        // i.e. M^2/R + M R terms instead of the direct sum's M^2 (R = 1 is the direct sum).  All
        // twiddles still come from the table by reduced integer index.
        const int R = g.R, Mr = M / R;
        int xo[kCePer];
#pragma unroll
        for (int j = 0; j < kCePer; ++j) {
            const int p = tid + j * kCeThreads;
            const int pp = p < M ? p : 0;
            const int r = pp / Mr, kp = pp - r * Mr;
            acc[j] = {0.0, 0.0};
            xo[j] = r;
            idx[j] = 0;
            stp[j] = (R * kp) % M;
        }
        for (int n = 0; n < M; n += R) {
#pragma unroll
            for (int j = 0; j < kCePer; ++j)
                if (j < nq) {
                    const double a = xr[n + xo[j]], b = xi[n + xo[j]];
                    double c, s;
                    tw_lookup<false>(tc, ts, idx[j], M, c, s);
                    acc[j].re = fma(a, c, acc[j].re);   // x exp(+2 pi i idx / M)
                    acc[j].re = fma(-b, s, acc[j].re);
                    acc[j].im = fma(a, s, acc[j].im);
                    acc[j].im = fma(b, c, acc[j].im);
                    idx[j] += stp[j];
                    if (idx[j] >= mod) idx[j] -= mod;
                }
        }
        if (R > 1) {
            __syncthreads();   // x is dead: the buffer takes Y
#pragma unroll
            for (int j = 0; j < kCePer; ++j) {
                const int p = tid + j * kCeThreads;
                if (p < M) xr[p] = acc[j].re, xi[p] = acc[j].im;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kCePer; ++j) {
                const int k = tid + j * kCeThreads;
                const int kk = k < M ? k : 0;
                const int km = kk % Mr;
                cx sum = {0.0, 0.0};
                int id = 0;
                for (int r = 0; r < R; ++r) {
                    const double a = xr[r * Mr + km], b = xi[r * Mr + km];
                    double c, s;
                    tw_lookup<false>(tc, ts, id, M, c, s);
                    sum.re = fma(a, c, sum.re);
                    sum.re = fma(-b, s, sum.re);
                    sum.im = fma(a, s, sum.im);
                    sum.im = fma(b, c, sum.im);
                    id += kk;
                    if (id >= M) id -= M;
                }
                acc[j] = sum;
            }
        }
    }
    // steps 3-4: scale, noise power over [L_left, M - L_right), mask
    const double rsM = 1.0 / sqrt((double)M), rs2M = sqrt(2.0 / (double)M);
    double a2[kCePer], np = 0.0;
#pragma unroll
    for (int j = 0; j < kCePer; ++j) {
        const int k = tid + j * kCeThreads;
        const double sc = (DCT && k != 0) ? rs2M : rsM;
        acc[j] = cscale(acc[j], sc);
        a2[j] = acc[j].re * acc[j].re + acc[j].im * acc[j].im;
        if (k < M && k >= g.L_left && k < M - g.L_right) np += a2[j];
    }
    const double noise = block_sum(np, red) / (double)(M - g.L_left - g.L_right);   // also the barrier after x's last read
    const double thr = sqrt(noise / 2.0);
    if (tid == 0 && noise_out) noise_out[seq] = noise;
#pragma unroll
    for (int j = 0; j < kCePer; ++j) {
        const int k = tid + j * kCeThreads;
        if (k < M) {
            const bool keep = !(sqrt(a2[j]) < thr) && (k < g.L_left || k >= M - g.L_right);
            // the back transform's scale is folded into the stored tap
            const double sc = (DCT && k != 0) ? rs2M : rsM;
            xr[k] = keep ? acc[j].re * sc : 0.0, xi[k] = keep ? acc[j].im * sc : 0.0;
            if (taps_out) taps_out[seq * M + k] = keep ? 1 : 0;
        }
    }
    __syncthreads();

    // step 5: back transform of the taps outside the window, at f[eK .. eK + N] only
    // N + 1 outputs: the last one feeds the interpolation of the final interval, unless the
    // sequence ends there (eK = 0), where np.interp holds the last value
    const int no = N + 1 <= M - g.eK ? N + 1 : M - g.eK;
    const int nqo = (no + kCeThreads - 1) / kCeThreads;
    cx f[kCePer];
    int fi[kCePer];
#pragma unroll
    for (int j = 0; j < kCePer; ++j) {
        const int o = tid + j * kCeThreads;
        fi[j] = g.eK + (o < no ? o : 0);
        f[j] = {0.0, 0.0};
    }
    for (int part = 0; part < 2; ++part) {
        const int k0 = part ? M - g.L_right : 0, k1 = part ? M : g.L_left;
#pragma unroll
        for (int j = 0; j < kCePer; ++j) {
            // DFT: exp(-2 pi i i k / M): index i k mod M, step i; DCT: k (2i + 1) mod 4M
            stp[j] = DCT ? (2 * fi[j] + 1) % mod : fi[j];
            idx[j] = (int)(((int64_t)k0 * stp[j]) % mod);
        }
        for (int k = k0; k < k1; ++k) {
            const double a = xr[k], b = xi[k];
#pragma unroll
            for (int j = 0; j < kCePer; ++j)
                if (j < nqo) {
                    double c, s;
                    tw_lookup<DCT>(tc, ts, idx[j], M, c, s);
                    if constexpr (DCT) {
                        f[j].re = fma(a, c, f[j].re);
                        f[j].im = fma(b, c, f[j].im);
                    } else {   // g[k] (c - i s)
                        f[j].re = fma(a, c, f[j].re);
                        f[j].re = fma(b, s, f[j].re);
                        f[j].im = fma(b, c, f[j].im);
                        f[j].im = fma(-a, s, f[j].im);
                    }
                    idx[j] += stp[j];
                    if (idx[j] >= mod) idx[j] -= mod;
                }
        }
    }
    __syncthreads();   // every thread has read its taps: the buffer now takes f[eK + o] at o
#pragma unroll
    for (int j = 0; j < kCePer; ++j) {
        const int o = tid + j * kCeThreads;
        if (o < no) xr[o] = f[j].re, xi[o] = f[j].im;
    }
    __syncthreads();

    // residual for the covariance: compensated H_LS - H_est[::D] (H_est[n D] is f[eK + n] exactly)
    double2* nh = ws.nhs + seq * N;
    for (int n = tid; n < N; n += kCeThreads) {
        cx v = widen(x[(int64_t)n * NE]);
        if (g.to_comp) v = cmul(v, to_phase(avg, g.D, n, g.scs));
        nh[n] = double2{v.re - xr[n], v.im - xi[n]};
    }
    // steps 6-7: linear interpolation to every subcarrier, cropped
    double2* he = ws.hest + seq * g.ND;
    const double rD = (double)g.D;
    for (int e = tid; e < g.ND; e += kCeThreads) {
        const int i = e / g.D, jj = e - i * g.D;
        const int i1 = i + 1 < no ? i + 1 : no - 1;
        const double w = (double)jj / rD;
        const cx v = {xr[i] + w * (xr[i1] - xr[i]), xi[i] + w * (xi[i1] - xi[i])};
        he[e] = double2{v.re, v.im};
        if (h_est_out)
            h_est_out[(((int64_t)t * g.S + m) * g.ND + e) * NE + q] = narrow<C>(v);
    }
}

// ------------------------------------------------------------------ steps 8-9
// Expand: thread -> VEC consecutive (subcarrier, nr, nt) elements of all 14 symbols; 16-byte
// stores (one complex128 or two complex64 per lane).  Covariance: the workgroups past `nexp`, one
// per 16-PRB group (the residue merged into the last), all S DMRS symbols, then the same line.
template <typename C, int VEC>
__global__ __launch_bounds__(kCeThreads) void ce_expand_cov_kernel(CeGeom g, CeWeights W, CeWork ws, int nexp,
                                                                   C* __restrict__ h, int64_t ldh,
                                                                   C* __restrict__ cov, int64_t ldcov) {
    const int t = blockIdx.y, tid = threadIdx.x;
    const int NE = g.Nr * g.Nt;
    const int64_t row = (int64_t)g.ND * NE;
    if ((int)blockIdx.x < nexp) {
        const int64_t e0 = ((int64_t)blockIdx.x * kCeThreads + tid) * VEC;
        if (e0 >= row) return;
        cx v[VEC][kCeMaxS];
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
            const int64_t e = e0 + u;
            const int64_t sc = e / NE;
            const int q = (int)(e - sc * NE);
#pragma unroll
            for (int m = 0; m < kCeMaxS; ++m)
                if (m < g.S) {
                    const double2 d = ws.hest[(((int64_t)t * g.S + m) * NE + q) * g.ND + sc];
                    v[u][m] = {d.x, d.y};
                }
        }
        C* out = h + (int64_t)t * ldh + e0;
#pragma unroll
        for (int s = 0; s < kCeSyms; ++s) {
            C o[VEC];
#pragma unroll
            for (int u = 0; u < VEC; ++u) {
                cx a = cscale(v[u][0], W.w[s][0]);
#pragma unroll
                for (int m = 1; m < kCeMaxS; ++m)
                    if (m < g.S) a.re = fma(W.w[s][m], v[u][m].re, a.re), a.im = fma(W.w[s][m], v[u][m].im, a.im);
                o[u] = narrow<C>(a);
            }
            if constexpr (VEC == 2) {
                *(float4*)(out + (int64_t)s * row) = float4{o[0].x, o[0].y, o[1].x, o[1].y};
            } else {
                out[(int64_t)s * row] = o[0];
            }
        }
        return;
    }
    // ---- covariance of one group
    __shared__ double pr[4][64], pi[4][64];
    __shared__ double cr[kCeMaxS][16], ci[kCeMaxS][16];
    const int grp = (int)blockIdx.x - nexp;
    const int per = 16 * 12 / g.D;
    const int ngrp = g.N / per;
    const int prb = g.ND / 12;
    const int r0 = grp * per, cnt = grp == ngrp - 1 ? g.N - r0 : per;
    const int p0 = grp * 16, pcnt = grp == ngrp - 1 ? prb - p0 : 16;
    const int NN = g.Nr * g.Nr;
    const int o = tid & 63, part = tid >> 6;   // output (m, a, b); partial sum over re = part mod 4
    const int m = o / NN, ab = o - m * NN, a = ab / g.Nr, b = ab - a * g.Nr;
    double sr = 0.0, si = 0.0;
    if (m < g.S) {
        const double2* na = ws.nhs + (((int64_t)t * g.S + m) * NE + a * g.Nt) * g.N;
        const double2* nb = ws.nhs + (((int64_t)t * g.S + m) * NE + b * g.Nt) * g.N;
        for (int re = r0 + part; re < r0 + cnt; re += 4) {
            double tr = 0.0, ti = 0.0;   // (sel_d @ sel_d^H)[a][b] of this RE
            for (int nt = 0; nt < g.Nt; ++nt) {
                const double2 u = na[(int64_t)nt * g.N + re], w = nb[(int64_t)nt * g.N + re];
                tr += u.x * w.x + u.y * w.y;
                ti += u.y * w.x - u.x * w.y;
            }
            sr += tr, si += ti;
        }
    }
    pr[part][o] = sr, pi[part][o] = si;
    __syncthreads();
    if (part == 0 && m < g.S) {
        double xr = ((pr[0][o] + pr[1][o]) + pr[2][o]) + pr[3][o];
        double xi = ((pi[0][o] + pi[1][o]) + pi[2][o]) + pi[3][o];
        xr = xr / (double)cnt / (double)g.Nt, xi = xi / (double)cnt / (double)g.Nt;
        if (g.cdm == 1) xr *= 2.0, xi *= 2.0;
        cr[m][ab] = xr, ci[m][ab] = xi;
    }
    __syncthreads();
    const int total = kCeSyms * pcnt * NN;
    for (int i = tid; i < total; i += kCeThreads) {
        const int s = i / (pcnt * NN), r = i - s * (pcnt * NN);
        const int p = r / NN, e = r - p * NN;
        cx v = {W.w[s][0] * cr[0][e], W.w[s][0] * ci[0][e]};
        for (int mm = 1; mm < g.S; ++mm) v.re = fma(W.w[s][mm], cr[mm][e], v.re), v.im = fma(W.w[s][mm], ci[mm][e], v.im);
        cov[(int64_t)t * ldcov + ((int64_t)s * prb + p0 + p) * NN + e] = narrow<C>(v);
    }
}

// ------------------------------------------------------------------ data REs (comp_pdsch_timing_offset)
template <typename C>
__global__ __launch_bounds__(kCeThreads) void ce_to_comp_kernel(const C* __restrict__ y, int64_t ldy,
                                                                C* __restrict__ out, int64_t ldo,
                                                                const double* __restrict__ to_avg, int64_t nsym,
                                                                int64_t RE, int Nr, int scs) {
    const int t = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kCeThreads + threadIdx.x;   // (symbol, RE)
    if (i >= nsym * RE) return;
    const int64_t k = i % RE;
    const cx ph = to_phase(to_avg[t], 1, k, scs);
    for (int r = 0; r < Nr; ++r) {
        const cx v = cmul(widen(y[(int64_t)t * ldy + i * Nr + r]), ph);
        out[(int64_t)t * ldo + i * Nr + r] = narrow<C>(v);
    }
}

size_t ce_lds_bytes(int M, bool dct) {
    const size_t tab = dct ? (size_t)M + 2 : 2 * ((size_t)(M >> 1) + 1);
    return (2 * (size_t)M + tab + kCeThreads) * sizeof(double);
}

int64_t ce_ws_bytes(int64_t T, int64_t S, int64_t N, int64_t NE, int64_t D) {
    const int64_t head = ((T * (1 + kCeMaxS) * 8 + 15) / 16) * 16;
    return head + T * S * NE * (N * D + N) * 16;
}

template <typename C>
int ce_run(const void* hls_, int64_t ldhls, const CeGeom& g, const CeWeights& W, int T, int dct, bool want_to,
           void* h, int64_t ldh, void* cov, int64_t ldcov, unsigned char* work, void* hls_comp, int64_t ldhc,
           void* h_est, double* noise, uint8_t* taps, double* to_est, double* to_avg, hipStream_t st) {
    const C* hls = (const C*)hls_;
    const int NE = g.Nr * g.Nt;
    const int64_t head = (((int64_t)T * (1 + kCeMaxS) * 8 + 15) / 16) * 16;
    CeWork ws;
    ws.to_avg = (double*)work;
    ws.to_est = ws.to_avg + T;
    ws.hest = (double2*)(work + head);
    ws.nhs = ws.hest + (int64_t)T * g.S * NE * g.ND;
    if (want_to)
        hipLaunchKernelGGL((ce_to_kernel<C>), dim3(T), dim3(kCeThreads), 0, st, hls, ldhls, g, ws, to_est, to_avg);
    const dim3 grid(g.S * NE, T);
    const size_t lds = ce_lds_bytes(g.M, dct);
    if (dct)
        hipLaunchKernelGGL((ce_tap_kernel<true, C>), grid, dim3(kCeThreads), lds, st, hls, ldhls, g, ws, (C*)hls_comp,
                           ldhc, (C*)h_est, noise, taps);
    else
        hipLaunchKernelGGL((ce_tap_kernel<false, C>), grid, dim3(kCeThreads), lds, st, hls, ldhls, g, ws,
                           (C*)hls_comp, ldhc, (C*)h_est, noise, taps);
    const int64_t row = (int64_t)g.ND * NE;
    const int ngrp = g.N / (16 * 12 / g.D);
    // two complex64 per lane need 16-byte aligned rows
    const bool vec2 = sizeof(C) == 8 && (ldh % 2 == 0) && ((uintptr_t)h % 16 == 0);
    if (vec2) {
        if constexpr (sizeof(C) == 8) {
            const int nexp = (int)((row / 2 + kCeThreads - 1) / kCeThreads);
            hipLaunchKernelGGL((ce_expand_cov_kernel<C, 2>), dim3(nexp + ngrp, T), dim3(kCeThreads), 0, st, g, W, ws,
                               nexp, (C*)h, ldh, (C*)cov, ldcov);
        }
    } else {
        const int nexp = (int)((row + kCeThreads - 1) / kCeThreads);
        hipLaunchKernelGGL((ce_expand_cov_kernel<C, 1>), dim3(nexp + ngrp, T), dim3(kCeThreads), 0, st, g, W, ws, nexp,
                           (C*)h, ldh, (C*)cov, ldcov);
    }
    return check_hip(hipGetLastError(), "channel estimate launch");
}

}  // namespace
}  // namespace ldpc5g_impl

using namespace ldpc5g_impl;

extern "C" {

int64_t ldpc5g_ce_workspace_bytes(int32_t T, int32_t S, int32_t N, int32_t Nr, int32_t Nt, int32_t D) {
    if (T <= 0 || S <= 0 || N <= 0 || Nr <= 0 || Nt <= 0 || D <= 0) return 0;
    return ce_ws_bytes(T, S, N, (int64_t)Nr * Nt, D);
}

int ldpc5g_channel_estimate(const void* h_ls, int64_t ldhls, int32_t in_dtype, int32_t T, int32_t S, int32_t N,
                            int32_t Nr, int32_t Nt, int32_t D, const int32_t* sym_idx, int32_t algo, int32_t eK,
                            int32_t L_left, int32_t L_right, int32_t num_cdm_groups, int32_t to_comp, int32_t scs,
                            void* h, int64_t ldh, void* cov, int64_t ldcov, void* work, int64_t work_bytes,
                            void* h_ls_comp, int64_t ldhc, void* h_est, double* noise_power, uint8_t* taps,
                            double* to_est, double* to_avg, void* stream) {
    clear_error();
    if (!(Nr == 1 || Nr == 2 || Nr == 4) || Nt < 1 || Nt > Nr)
        return fail(LDPC5G_ESIZE, "Nr=%d Nt=%d (Nr in {1, 2, 4}, 1 <= Nt <= Nr)", Nr, Nt);
    if (algo < LDPC5G_CE_DFT || algo > LDPC5G_CE_DCT_SYMMETRIC)
        return fail(LDPC5G_ESIZE, "bad algo %d (0 DFT, 1 DCT, 2 DFT_symmetric, 3 DCT_symmetric)", algo);
    if (in_dtype != LDPC5G_F32 && in_dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad dtype %d", in_dtype);
    if (S < 1 || S > kCeMaxS) return fail(LDPC5G_ESIZE, "S=%d DMRS symbols (1 <= S <= 4)", S);
    if (!sym_idx) return fail(LDPC5G_ESIZE, "null sym_idx");
    for (int m = 0; m < S; ++m)
        if (sym_idx[m] < 0 || sym_idx[m] >= kCeSyms || (m > 0 && sym_idx[m] <= sym_idx[m - 1]))
            return fail(LDPC5G_ESIZE, "bad symbols: sym_idx[%d]=%d (strictly ascending in 0..13)", m, sym_idx[m]);
    if (D != 2 && D != 4) return fail(LDPC5G_ESIZE, "D=%d (RE_distance in {2, 4})", D);
    if (scs != 15 && scs != 30) return fail(LDPC5G_ESIZE, "scs=%d kHz (15 or 30)", scs);
    if (T <= 0 || T > 65535) return fail(LDPC5G_ESIZE, "bad sizes T=%d", T);
    if (N <= 0 || N > kCeMaxM || ((int64_t)N * D) % 12 != 0)
        return fail(LDPC5G_ESIZE, "N=%d D=%d: N*D must be a positive multiple of 12", N, D);
    const int PRB = N * D / 12;
    if (PRB < 16)
        return fail(LDPC5G_ESIZE, "PRB=%d < 16: the reference's covariance grouping has no group (dft_dct_CE.py:199-206)",
                    PRB);
    if (eK < 0 || eK > kCeMaxM) return fail(LDPC5G_ESIZE, "bad eK %d", eK);
    const bool symm = algo == LDPC5G_CE_DFT_SYMMETRIC || algo == LDPC5G_CE_DCT_SYMMETRIC;
    const bool dct = algo == LDPC5G_CE_DCT || algo == LDPC5G_CE_DCT_SYMMETRIC;
    const int reK = eK + (N + eK) % 2;
    const int64_t Mh = (int64_t)N + eK + reK, M = symm ? 2 * Mh : Mh;
    if (M > kCeMaxM) return fail(LDPC5G_ESIZE, "M=%lld > %d (extended sequence length)", (long long)M, kCeMaxM);
    if (L_left < 0 || L_right < 0 || (int64_t)L_left + L_right >= M)
        return fail(LDPC5G_ESIZE, "L_left=%d L_right=%d: need 0 <= L_left, L_right and L_left + L_right < M=%lld", L_left,
                    L_right, (long long)M);
    if (num_cdm_groups < 1 || num_cdm_groups > 3) return fail(LDPC5G_ESIZE, "bad num_cdm_groups %d", num_cdm_groups);
    const int64_t NE = (int64_t)Nr * Nt;
    if (ldhls < (int64_t)S * N * NE || ldh < (int64_t)kCeSyms * N * D * NE || ldcov < (int64_t)kCeSyms * PRB * Nr * Nr ||
        (h_ls_comp && ldhc < (int64_t)S * N * NE))
        return fail(LDPC5G_ESIZE, "bad strides: a row stride is shorter than its row");
    const int64_t need = ce_ws_bytes(T, S, N, NE, D);
    if (work_bytes < need)
        return fail(LDPC5G_ESIZE, "workspace too small: %lld < %lld bytes", (long long)work_bytes, (long long)need);
    if (!h_ls || !h || !cov || !work) return fail(LDPC5G_ESIZE, "null buffer");
    if (h_ls_comp && !to_comp) return fail(LDPC5G_ESIZE, "h_ls_comp is written only with to_comp");
    if (h_ls_comp == h_ls) return fail(LDPC5G_ESIZE, "h_ls_comp must not overlap h_ls");

    CeGeom g;
    g.S = S, g.N = N, g.Nr = Nr, g.Nt = Nt, g.D = D, g.eK = eK, g.reK = reK, g.M = (int)M, g.Mh = (int)Mh;
    g.L_left = L_left, g.L_right = L_right, g.P = 24 / D, g.ND = N * D, g.scs = scs, g.cdm = num_cdm_groups;
    g.to_comp = to_comp ? 1 : 0;
    g.R = 1;
    while (g.R < LDPC5G_CE_MAX_RADIX && g.M % (2 * g.R) == 0) g.R *= 2;
    for (int m = 0; m < kCeMaxS; ++m) g.sym[m] = m < S ? sym_idx[m] : 0;
    // the degree-1 least-squares line over the DMRS symbols as per-symbol weights
    // (timing_interpolate_to_14_symbol, dft_dct_CE.py:159-178; S = 1 copies)
    CeWeights W;
    double xm = 0.0, sxx = 0.0;
    for (int m = 0; m < S; ++m) xm += (double)sym_idx[m];
    xm = xm / (double)S;
    for (int m = 0; m < S; ++m) sxx += ((double)sym_idx[m] - xm) * ((double)sym_idx[m] - xm);
    for (int s = 0; s < kCeSyms; ++s)
        for (int m = 0; m < kCeMaxS; ++m)
            W.w[s][m] = m >= S ? 0.0 : (S == 1 ? 1.0 : 1.0 / (double)S + ((double)s - xm) * ((double)sym_idx[m] - xm) / sxx);
    const bool want_to = to_comp || to_est || to_avg;
    hipStream_t st = (hipStream_t)stream;
    if (in_dtype == LDPC5G_F64)
        return ce_run<double2>(h_ls, ldhls, g, W, T, dct, want_to, h, ldh, cov, ldcov, (unsigned char*)work, h_ls_comp,
                               ldhc, h_est, noise_power, taps, to_est, to_avg, st);
    return ce_run<float2>(h_ls, ldhls, g, W, T, dct, want_to, h, ldh, cov, ldcov, (unsigned char*)work, h_ls_comp, ldhc,
                          h_est, noise_power, taps, to_est, to_avg, st);
}

int ldpc5g_to_compensate(const void* y, int64_t ldy, void* out, int64_t ldo, int32_t in_dtype, const double* to_avg,
                         int32_t T, int64_t nsym, int64_t RE, int32_t Nr, int32_t scs, void* stream) {
    clear_error();
    if (Nr < 1 || Nr > 64) return fail(LDPC5G_ESIZE, "Nr=%d (1..64)", Nr);
    if (in_dtype != LDPC5G_F32 && in_dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad dtype %d", in_dtype);
    if (scs != 15 && scs != 30) return fail(LDPC5G_ESIZE, "scs=%d kHz (15 or 30)", scs);
    if (T <= 0 || T > 65535 || nsym <= 0 || RE <= 0 || nsym > 1024 || RE > (1 << 20))
        return fail(LDPC5G_ESIZE, "bad sizes T=%d nsym=%lld RE=%lld", T, (long long)nsym, (long long)RE);
    if (ldy < nsym * RE * Nr || ldo < nsym * RE * Nr)
        return fail(LDPC5G_ESIZE, "bad strides: a row stride is shorter than its row");
    if (!y || !out || !to_avg) return fail(LDPC5G_ESIZE, "null buffer");
    const dim3 grid((unsigned)((nsym * RE + kCeThreads - 1) / kCeThreads), T);
    hipStream_t st = (hipStream_t)stream;
    if (in_dtype == LDPC5G_F64)
        hipLaunchKernelGGL((ce_to_comp_kernel<double2>), grid, dim3(kCeThreads), 0, st, (const double2*)y, ldy,
                           (double2*)out, ldo, to_avg, nsym, RE, Nr, scs);
    else
        hipLaunchKernelGGL((ce_to_comp_kernel<float2>), grid, dim3(kCeThreads), 0, st, (const float2*)y, ldy,
                           (float2*)out, ldo, to_avg, nsym, RE, Nr, scs);
    return check_hip(hipGetLastError(), "to_compensate launch");
}

}  // extern "C"
