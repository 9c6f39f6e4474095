// ldpc5g_tp.hip — PUSCH transform precoding (DFT-s-OFDM), batched:
//   spreading DFT ................. py5gphy/nr_pusch/nr_pusch_process.py:39-54
//   de-spreading IDFT ............. py5gphy/nr_pusch/nr_pusch.py:170-194
//   low-PAPR (Zadoff-Chu) sequence  py5gphy/common/lowPAPR_seq.py:5-41 (gen_lowPAPR_seq)
// (ldpc5g_transform_precode / ldpc5g_low_papr_seq, include/ldpc5g.h).  The low-PAPR DMRS of the slot
// front end is a sequence source of ldpc5g_slot.hip; the sequence's points are ldpc5g_lowpapr.h.
// The transform length is M = 12 rb_size with rb_size = 2^a 3^b 5^c: never a useful power of two.
// tp_dft_kernel runs a mixed-radix Stockham (self-sorting) transform in LDS, one 256-thread
// workgroup per M-block (or per G blocks while G M <= 768): load, one pass per radix, store.  The
// radices come from the host as a packed plan, odd ones first (3, 5, then 4, then 2): a pass
// writes runs of Ns consecutive points Ns R apart, which stays (almost) free of bank conflicts
// while Ns is odd or a multiple of 16, and every pass reads consecutive points.  Above M = 2048, where
// two buffers would leave one workgroup per CU, tp_dft_single_kernel runs the same passes in one
// buffer, a thread's butterflies held in registers across a barrier.
// Twiddles come from an LDS table w[j] = (cos, sin)(2 pi j / M), j = 0..M/2, one sincospi of the
// exact rational per entry, the upper half by symmetry; a pass indexes it with r k M / (Ns R),
// which is below M without any reduction.  Forward and inverse differ only in the sign of sin.
// float64 arithmetic whatever the storage type, a fixed operation order, no atomics.
#include <math.h>
#include <stdint.h>

#include "ldpc5g_common.h"
#include "ldpc5g_lowpapr.h"

namespace ldpc5g_impl {
namespace {

constexpr int kTpThreads = 256;
constexpr int kTpMaxPass = 12;
constexpr int kTpPackPoints = 768;   // a workgroup takes G = 768 / M blocks (at least one)
constexpr int kTpMaxG = 64;

struct TpPlan {
    int32_t M, G, nsym, npass;
    int64_t nblk;        // T * nsym
    uint64_t radix;      // 4 bits per pass, pass 0 in the low bits
    int32_t tab;         // padded entries of one half-wave table
    int32_t inverse;
    double scale;        // 1 / sqrt(M)
};

// table slot of entry j: one pad per 32 entries spreads the power-of-two strides of the middle
// passes over the banks (ds_read_b64: 32 doubles per bank row)
__host__ __device__ __forceinline__ int tw_slot(int j) { return j + (j >> 5); }

struct TpLds {
    double *ar, *ai, *br, *bi, *tc, *ts;
};

// exp(-+ 2 pi i j / M) for j in [0, M): (c, s) with the transform's sign applied to s
__device__ __forceinline__ void tp_tw(const TpLds& L, int j, int M, double sgn, double& c, double& s) {
    const bool up = j > (M >> 1);
    const int jj = tw_slot(up ? M - j : j);
    c = L.tc[jj];
    const double v = L.ts[jj];
    s = up ? -v * sgn : v * sgn;
}

// (a + i b) (c + i s)
__device__ __forceinline__ void tp_mul(double& a, double& b, double c, double s) {
    const double x = a * c - b * s, y = a * s + b * c;
    a = x, b = y;
}

// DFT_R of v in place; sgn = -1 forward (exp(-2 pi i / R)), +1 inverse
template <int R>
__device__ __forceinline__ void tp_butterfly(double (&vr)[R], double (&vi)[R], double sgn) {
    if constexpr (R == 2) {
        const double ar = vr[0] + vr[1], ai = vi[0] + vi[1];
        vr[1] = vr[0] - vr[1], vi[1] = vi[0] - vi[1];
        vr[0] = ar, vi[0] = ai;
    } else if constexpr (R == 3) {
        const double h = 0.86602540378443864676 * sgn;   // sgn sin(2 pi / 3)
        const double sr = vr[1] + vr[2], si = vi[1] + vi[2];
        const double dr = vr[1] - vr[2], di = vi[1] - vi[2];
        const double mr = vr[0] - 0.5 * sr, mi = vi[0] - 0.5 * si;
        vr[0] = vr[0] + sr, vi[0] = vi[0] + si;
        // i h (d): (-h di, h dr)
        vr[1] = mr - h * di, vi[1] = mi + h * dr;
        vr[2] = mr + h * di, vi[2] = mi - h * dr;
    } else if constexpr (R == 4) {
        const double s0r = vr[0] + vr[2], s0i = vi[0] + vi[2];
        const double d0r = vr[0] - vr[2], d0i = vi[0] - vi[2];
        const double s1r = vr[1] + vr[3], s1i = vi[1] + vi[3];
        const double d1r = vr[1] - vr[3], d1i = vi[1] - vi[3];
        // sgn i (d1): (-sgn d1i, sgn d1r)
        const double er = -sgn * d1i, ei = sgn * d1r;
        vr[0] = s0r + s1r, vi[0] = s0i + s1i;
        vr[2] = s0r - s1r, vi[2] = s0i - s1i;
        vr[1] = d0r + er, vi[1] = d0i + ei;
        vr[3] = d0r - er, vi[3] = d0i - ei;
    } else {
        static_assert(R == 5, "radix 2, 3, 4 or 5");
        const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;    // cos(2 pi / 5), cos(4 pi / 5)
        const double h1 = 0.95105651629515357212 * sgn, h2 = 0.58778525229247312917 * sgn;   // sgn sin(.)
        const double s1r = vr[1] + vr[4], s1i = vi[1] + vi[4], d1r = vr[1] - vr[4], d1i = vi[1] - vi[4];
        const double s2r = vr[2] + vr[3], s2i = vi[2] + vi[3], d2r = vr[2] - vr[3], d2i = vi[2] - vi[3];
        const double m1r = (vr[0] + c1 * s1r) + c2 * s2r, m1i = (vi[0] + c1 * s1i) + c2 * s2i;
        const double m2r = (vr[0] + c2 * s1r) + c1 * s2r, m2i = (vi[0] + c2 * s1i) + c1 * s2i;
        const double n1r = h1 * d1r + h2 * d2r, n1i = h1 * d1i + h2 * d2i;
        const double n2r = h2 * d1r - h1 * d2r, n2i = h2 * d1i - h1 * d2i;
        vr[0] = (vr[0] + s1r) + s2r, vi[0] = (vi[0] + s1i) + s2i;
        // X1 = m1 + i n1, X4 = m1 - i n1, X2 = m2 + i n2, X3 = m2 - i n2
        vr[1] = m1r - n1i, vi[1] = m1i + n1r;
        vr[4] = m1r + n1i, vi[4] = m1i - n1r;
        vr[2] = m2r - n2i, vi[2] = m2i + n2r;
        vr[3] = m2r + n2i, vi[3] = m2i - n2r;
    }
}

// One Stockham pass of radix R over `cnt` blocks: butterfly j < M/R of a block reads points
// j + r M/R, turns point r by w^(r k), k = j mod Ns, and writes the DFT_R to (j / Ns) Ns R + k + r Ns.
template <int R, bool MULTI>
__device__ __forceinline__ void tp_pass(const TpLds& L, const double* __restrict__ sr, const double* __restrict__ si,
                                        double* __restrict__ dr, double* __restrict__ di, int M, int Ns, int cnt,
                                        double sgn) {
    const int nb = M / R;
    const int step = nb / Ns;   // M / (Ns R): the table stride of this pass
    const int total = MULTI ? cnt * nb : nb;
    for (int i = threadIdx.x; i < total; i += kTpThreads) {
        int base = 0, j = i;
        if constexpr (MULTI) {
            const int g = i / nb;
            j = i - g * nb;
            base = g * M;
        }
        const int q = j / Ns, k = j - q * Ns;
        double vr[R], vi[R];
#pragma unroll
        for (int r = 0; r < R; ++r) vr[r] = sr[base + j + r * nb], vi[r] = si[base + j + r * nb];
        if (Ns > 1) {
            const int t1 = k * step;
#pragma unroll
            for (int r = 1; r < R; ++r) {
                double c, s;
                tp_tw(L, r * t1, M, sgn, c, s);
                tp_mul(vr[r], vi[r], c, s);
            }
        }
        tp_butterfly<R>(vr, vi, sgn);
        const int o = base + q * Ns * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) dr[o + r * Ns] = vr[r], di[o + r * Ns] = vi[r];
    }
}

template <typename C, bool MULTI>
__global__ __launch_bounds__(kTpThreads) void tp_dft_kernel(const C* x, int64_t ldx, C* out, int64_t ldo, TpPlan p) {   // out may be x
    extern __shared__ __align__(16) unsigned char tp_smem[];
    using S = decltype(C{}.x);
    const int M = p.M, tid = threadIdx.x;
    const int GM = MULTI ? p.G * M : M;
    TpLds L;
    L.ar = (double*)tp_smem, L.ai = L.ar + GM, L.br = L.ai + GM, L.bi = L.br + GM;
    L.tc = L.bi + GM, L.ts = L.tc + p.tab;
    const int64_t blk0 = (int64_t)blockIdx.x * (MULTI ? p.G : 1);
    const int64_t left = p.nblk - blk0;   // the last workgroup of a launch may be partial
    const int cnt = MULTI ? (int)(left < p.G ? left : p.G) : 1;

    for (int j = tid; j <= (M >> 1); j += kTpThreads) {
        double s, c;
        sincospi((double)(2 * j) / (double)M, &s, &c);
        L.tc[tw_slot(j)] = c, L.ts[tw_slot(j)] = s;
    }
    const int total = cnt * M;
    for (int i = tid; i < total; i += kTpThreads) {
        int g = 0, k = i;
        if constexpr (MULTI) g = i / M, k = i - g * M;
        const int64_t blk = blk0 + g;
        const int64_t t = blk / p.nsym, s = blk - t * p.nsym;
        const C v = x[t * ldx + s * M + k];
        L.ar[i] = (double)v.x, L.ai[i] = (double)v.y;
    }
    __syncthreads();

    const double sgn = p.inverse ? 1.0 : -1.0;
    double *sr = L.ar, *si = L.ai, *dr = L.br, *di = L.bi;
    int Ns = 1;
    for (int ps = 0; ps < p.npass; ++ps) {
        const int R = (int)((p.radix >> (4 * ps)) & 15u);
        switch (R) {
            case 2: tp_pass<2, MULTI>(L, sr, si, dr, di, M, Ns, cnt, sgn); break;
            case 3: tp_pass<3, MULTI>(L, sr, si, dr, di, M, Ns, cnt, sgn); break;
            case 4: tp_pass<4, MULTI>(L, sr, si, dr, di, M, Ns, cnt, sgn); break;
            default: tp_pass<5, MULTI>(L, sr, si, dr, di, M, Ns, cnt, sgn); break;
        }
        Ns *= R;
        double* t0 = sr; sr = dr, dr = t0;
        double* t1 = si; si = di, di = t1;
        __syncthreads();
    }

    for (int i = tid; i < total; i += kTpThreads) {
        int g = 0, k = i;
        if constexpr (MULTI) g = i / M, k = i - g * M;
        const int64_t blk = blk0 + g;
        const int64_t t = blk / p.nsym, s = blk - t * p.nsym;
        C v;
        v.x = (S)(sr[i] * p.scale), v.y = (S)(si[i] * p.scale);
        out[t * ldo + s * M + k] = v;
    }
}

// ---- the longest blocks: one buffer instead of two
// Above kTpSingleMinM the ping-pong buffers and the table pass 80 KiB, i.e. one workgroup (one wave
// per SIMD) per CU.  There a thread keeps the butterflies of a pass in registers across a barrier —
// at most 16 points, ITER butterflies of radix R — and writes them back into the buffer it read:
// M = 3240 takes 78 576 B, two workgroups per CU.  Same operations in the same order as tp_pass.
constexpr int kTpMaxM = 3240;
constexpr int kTpSingleMinM = 2048;
constexpr int tp_iters(int R) { return (kTpMaxM / R + kTpThreads - 1) / kTpThreads; }

template <int R>
__device__ __forceinline__ void tp_pass_single(const TpLds& L, int M, int Ns, double sgn) {
    constexpr int ITER = tp_iters(R);
    const int nb = M / R;
    const int step = nb / Ns;
    double vr[ITER][R], vi[ITER][R];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int j = (int)threadIdx.x + it * kTpThreads;
        if (j < nb) {
#pragma unroll
            for (int r = 0; r < R; ++r) vr[it][r] = L.ar[j + r * nb], vi[it][r] = L.ai[j + r * nb];
            if (Ns > 1) {
                const int t1 = (j % Ns) * step;
#pragma unroll
                for (int r = 1; r < R; ++r) {
                    double c, s;
                    tp_tw(L, r * t1, M, sgn, c, s);
                    tp_mul(vr[it][r], vi[it][r], c, s);
                }
            }
            tp_butterfly<R>(vr[it], vi[it], sgn);
        }
    }
    __syncthreads();   // every point of the pass is in registers: the buffer takes the results
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int j = (int)threadIdx.x + it * kTpThreads;
        if (j < nb) {
            const int q = j / Ns, k = j - q * Ns;
            const int o = q * Ns * R + k;
#pragma unroll
            for (int r = 0; r < R; ++r) L.ar[o + r * Ns] = vr[it][r], L.ai[o + r * Ns] = vi[it][r];
        }
    }
    __syncthreads();
}

template <typename C>
__global__ __launch_bounds__(kTpThreads) void tp_dft_single_kernel(const C* x, int64_t ldx, C* out, int64_t ldo,
                                                                   TpPlan p) {   // out may be x
    extern __shared__ __align__(16) unsigned char tp_smem[];
    using S = decltype(C{}.x);
    const int M = p.M, tid = threadIdx.x;
    TpLds L;
    L.ar = (double*)tp_smem, L.ai = L.ar + M, L.br = L.bi = nullptr;
    L.tc = L.ai + M, L.ts = L.tc + p.tab;
    const int64_t blk = blockIdx.x;
    const int64_t t = blk / p.nsym, s = blk - t * p.nsym;
    for (int j = tid; j <= (M >> 1); j += kTpThreads) {
        double sn, cs;
        sincospi((double)(2 * j) / (double)M, &sn, &cs);
        L.tc[tw_slot(j)] = cs, L.ts[tw_slot(j)] = sn;
    }
    for (int i = tid; i < M; i += kTpThreads) {
        const C v = x[t * ldx + s * M + i];
        L.ar[i] = (double)v.x, L.ai[i] = (double)v.y;
    }
    __syncthreads();
    const double sgn = p.inverse ? 1.0 : -1.0;
    int Ns = 1;
    for (int ps = 0; ps < p.npass; ++ps) {
        const int R = (int)((p.radix >> (4 * ps)) & 15u);
        switch (R) {
            case 2: tp_pass_single<2>(L, M, Ns, sgn); break;
            case 3: tp_pass_single<3>(L, M, Ns, sgn); break;
            case 4: tp_pass_single<4>(L, M, Ns, sgn); break;
            default: tp_pass_single<5>(L, M, Ns, sgn); break;
        }
        Ns *= R;
    }
    for (int i = tid; i < M; i += kTpThreads) {
        C v;
        v.x = (S)(L.ar[i] * p.scale), v.y = (S)(L.ai[i] * p.scale);
        out[t * ldo + s * M + i] = v;
    }
}

size_t tp_lds_bytes(const TpPlan& p) { return ((size_t)4 * p.G * p.M + 2 * (size_t)p.tab) * sizeof(double); }

bool make_plan(TpPlan& p, int M) {
    int n = M, e2 = 0, e3 = 0, e5 = 0;
    while (n % 2 == 0) n /= 2, ++e2;
    while (n % 3 == 0) n /= 3, ++e3;
    while (n % 5 == 0) n /= 5, ++e5;
    if (n != 1) return false;
    int np = 0;
    uint64_t rad = 0;
    auto push = [&](int r) { rad |= (uint64_t)r << (4 * np), ++np; };
    for (int i = 0; i < e3; ++i) push(3);
    for (int i = 0; i < e5; ++i) push(5);
    for (int i = 0; i < e2 / 2; ++i) push(4);
    if (e2 & 1) push(2);
    if (np > kTpMaxPass) return false;
    p.M = M, p.npass = np, p.radix = rad;
    p.G = kTpPackPoints / M < 1 ? 1 : (kTpPackPoints / M > kTpMaxG ? kTpMaxG : kTpPackPoints / M);
    p.tab = tw_slot(M >> 1) + 1;
    p.scale = 1.0 / sqrt((double)M);
    return true;
}

template <typename C, bool MULTI>
int tp_launch(const void* x, int64_t ldx, void* out, int64_t ldo, const TpPlan& p, hipStream_t st) {
    const size_t lds = tp_lds_bytes(p);
    if (lds > 64 * 1024) {
        const int rc = set_lds_once<tp_dft_kernel<C, MULTI>>(160 * 1024);
        if (rc) return rc;
    }
    const int64_t nwg = (p.nblk + p.G - 1) / p.G;
    hipLaunchKernelGGL((tp_dft_kernel<C, MULTI>), dim3((unsigned)nwg), dim3(kTpThreads), lds, st, (const C*)x, ldx,
                       (C*)out, ldo, p);
    return check_hip(hipGetLastError(), "tp_dft_kernel launch");
}

template <typename C>
int tp_launch_single(const void* x, int64_t ldx, void* out, int64_t ldo, const TpPlan& p, hipStream_t st) {
    const size_t lds = (2 * (size_t)p.M + 2 * (size_t)p.tab) * sizeof(double);
    if (lds > 64 * 1024) {
        const int rc = set_lds_once<tp_dft_single_kernel<C>>(80 * 1024);
        if (rc) return rc;
    }
    hipLaunchKernelGGL((tp_dft_single_kernel<C>), dim3((unsigned)p.nblk), dim3(kTpThreads), lds, st, (const C*)x, ldx,
                       (C*)out, ldo, p);
    return check_hip(hipGetLastError(), "tp_dft_single_kernel launch");
}

// ------------------------------------------------------------------ low-PAPR sequence
// out[i][m] = exp(j alpha m) rbar_{u[i], v[i]}(m) (38.211 5.2.2; gen_lowPAPR_seq), rbar from
// low_papr_point (ldpc5g_lowpapr.h).
__global__ __launch_bounds__(kTpThreads) void low_papr_kernel(const int32_t* __restrict__ u, const int32_t* __restrict__ v,
                                                              double alpha, int MZC, int NZC, double2* __restrict__ out) {
    const int i = blockIdx.y;
    const int m = blockIdx.x * kTpThreads + (int)threadIdx.x;
    if (m >= MZC) return;
    double re, im;
    low_papr_point(u[i], v[i], m, MZC, NZC, re, im);
    double s, c;
    sincos(alpha * (double)m, &s, &c);
    out[(int64_t)i * MZC + m] = double2{c * re - s * im, c * im + s * re};
}

}  // namespace
}  // namespace ldpc5g_impl

using namespace ldpc5g_impl;

extern "C" {

int ldpc5g_transform_precode(const void* x, int64_t ldx, void* out, int64_t ldo, int32_t in_dtype, int32_t T,
                             int32_t nsym, int32_t rb_size, int32_t inverse, void* stream) {
    clear_error();
    if (in_dtype != LDPC5G_F32 && in_dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad dtype %d", in_dtype);
    if (T < 1 || T > 65535) return fail(LDPC5G_ESIZE, "T=%d outside 1..65535", T);
    if (nsym < 1 || nsym > 14) return fail(LDPC5G_ESIZE, "nsym=%d outside 1..14", nsym);
    if (rb_size < 1 || rb_size > 275 || !smooth235(rb_size))
        return fail(LDPC5G_ESIZE, "rb_size=%d: 2^a 3^b 5^c in 1..275 (38.211 6.3.1.4)", rb_size);
    if (inverse != 0 && inverse != 1) return fail(LDPC5G_ESIZE, "inverse=%d outside 0..1", inverse);
    const int M = 12 * rb_size;
    if (ldx < (int64_t)nsym * M) return fail(LDPC5G_ESIZE, "x stride %lld shorter than nsym*12*rb_size", (long long)ldx);
    if (ldo < (int64_t)nsym * M) return fail(LDPC5G_ESIZE, "out stride %lld shorter than nsym*12*rb_size", (long long)ldo);
    if (!x || !out) return fail(LDPC5G_ESIZE, "null buffer (x, out)");
    const size_t al = in_dtype == LDPC5G_F64 ? 16 : 8;
    if (!aligned(x, al) || !aligned(out, al)) return fail(LDPC5G_ESIZE, "a buffer is not aligned to its element size");
    if (out == x && ldo != ldx) return fail(LDPC5G_ESIZE, "in place (out == x) needs equal strides");
    TpPlan p{};
    if (!make_plan(p, M)) return fail(LDPC5G_ESIZE, "rb_size=%d: no radix plan", rb_size);
    p.nsym = nsym, p.nblk = (int64_t)T * nsym, p.inverse = inverse;
    hipStream_t st = (hipStream_t)stream;
    if (p.G > 1)
        return in_dtype == LDPC5G_F64 ? tp_launch<double2, true>(x, ldx, out, ldo, p, st)
                                      : tp_launch<float2, true>(x, ldx, out, ldo, p, st);
    if (M > kTpSingleMinM)
        return in_dtype == LDPC5G_F64 ? tp_launch_single<double2>(x, ldx, out, ldo, p, st)
                                      : tp_launch_single<float2>(x, ldx, out, ldo, p, st);
    return in_dtype == LDPC5G_F64 ? tp_launch<double2, false>(x, ldx, out, ldo, p, st)
                                  : tp_launch<float2, false>(x, ldx, out, ldo, p, st);
}

int ldpc5g_low_papr_seq(const int32_t* u, const int32_t* v, int32_t n, double alpha, int32_t MZC, void* out,
                        void* stream) {
    clear_error();
    if (n < 1 || n > 65535) return fail(LDPC5G_ESIZE, "n=%d outside 1..65535", n);
    if (MZC < 6 || MZC > 3300 || MZC % 6) return fail(LDPC5G_ESIZE, "MZC=%d: a multiple of 6 in 6..3300", MZC);
    if (MZC <= 24)
        return fail(LDPC5G_ESIZE, "MZC=%d: the sequences of length 6, 12, 18, 24 are the tables of 38.211 5.2.2.2, "
                                  "not provided (pass them as base_seq)", MZC);
    if (!(alpha == alpha) || alpha - alpha != 0.0) return fail(LDPC5G_ESIZE, "alpha is not finite");
    if (!u || !v || !out) return fail(LDPC5G_ESIZE, "null buffer (u, v, out)");
    if (!aligned(u, 4) || !aligned(v, 4) || !aligned(out, 16))
        return fail(LDPC5G_ESIZE, "a buffer is not aligned to its element size");
    const int NZC = low_papr_nzc(MZC);
    const dim3 g((unsigned)((MZC + kTpThreads - 1) / kTpThreads), n);
    hipLaunchKernelGGL(low_papr_kernel, g, dim3(kTpThreads), 0, (hipStream_t)stream, u, v, alpha, MZC, NZC, (double2*)out);
    return check_hip(hipGetLastError(), "low_papr_kernel launch");
}

}  // extern "C"

