// ldpc5g_tp.hip — PUSCH transform precoding (DFT-s-OFDM), batched:
//   spreading DFT ................. py5gphy/nr_pusch/nr_pusch_process.py:39-54
//   de-spreading IDFT ............. py5gphy/nr_pusch/nr_pusch.py:170-194
//   low-PAPR (Zadoff-Chu) sequence  py5gphy/common/lowPAPR_seq.py:5-41 (gen_lowPAPR_seq)
// (ldpc5g_transform_precode / ldpc5g_low_papr_seq, include/ldpc5g.h).
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
#include "ldpc5g_prbs.h"

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

// rb_size = 2^a 3^b 5^c ?
bool smooth235(int n) {
    if (n < 1) return false;
    for (int f : {2, 3, 5})
        while (n % f == 0) n /= f;
    return n == 1;
}

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
// out[i][m] = exp(j alpha m) rbar_{u[i], v[i]}(m) (38.211 5.2.2; gen_lowPAPR_seq).  MZC = 30: the
// closed form exp(-j pi (u+1)(m+1)(m+2) / 31).  MZC >= 36: x_q(m mod N_ZC), x_q(n) =
// exp(-j pi q n (n+1) / N_ZC), with q from integers and the phase index reduced mod 2 N_ZC in
// 64-bit integers before the one sincospi.
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

int largest_prime_below(int n) {
    for (int p = n - 1; p >= 2; --p) {
        bool prime = true;
        for (int d = 2; d * d <= p; ++d)
            if (p % d == 0) { prime = false; break; }
        if (prime) return p;
    }
    return 0;
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

// ------------------------------------------------------------------ low-PAPR DMRS: LS and map
constexpr int kTpSyms = 14;

struct TpDmrs {            // by value: what is the same for every slot
    int32_t carrier_re, rb_start, rb_size, S;
    int32_t sym[4];        // DMRS symbol indices
    int32_t port;          // port - 1000 of the one layer
    int32_t id, hopping;   // nPuschID; 0 neither, 1 group, 2 sequence hopping
    int32_t MZC, NZC;      // 6 rb_size and the largest prime below it
    double scaling;        // 10^(-3/20): NumCDMGroupsWithoutData == 2
    double inv;            // LS: 1 / (2 scaling)
};

__device__ __forceinline__ int tp_dmrs_sym(const TpDmrs& c, int m) {   // c.sym[m] without a dynamic index
    return m == 0 ? c.sym[0] : m == 1 ? c.sym[1] : m == 2 ? c.sym[2] : c.sym[3];
}

// (u, v) of DMRS symbol `sym` of slot `slot` (_gen_seq_with_transform_precoding, nr_pusch_dmrs.py:216-249).
// Wave-uniform; every lane of the wave must be active (prbs_jump_wave).  The Gold bits c(n) are the
// low bits of the two jumped states: bit i of a state at n is x(n + i).  The reference makes one
// frame of bits (slot < 20); a position past the jump tables' 8192 wraps instead of reading beyond.
__device__ __forceinline__ void tp_uv(const TpDmrs& c, int32_t slot, int sym, int& u, int& v) {
    u = c.id % 30, v = 0;
    const uint32_t pos = (uint32_t)(14 * slot + sym);
    if (c.hopping == 1) {
        const uint32_t n = __builtin_amdgcn_readfirstlane((1600u + 8u * pos) & 8191u);
        const uint32_t s1 = prbs_jump_wave(0, 1u, n), s2 = prbs_jump_wave(1, (uint32_t)(c.id / 30), n);
        u = (int)((((s1 ^ s2) & 255u) % 30u + (uint32_t)c.id) % 30u);
    } else if (c.hopping == 2 && c.MZC >= 72) {
        const uint32_t n = __builtin_amdgcn_readfirstlane((1600u + pos) & 8191u);
        const uint32_t s1 = prbs_jump_wave(0, 1u, n), s2 = prbs_jump_wave(1, (uint32_t)c.id, n);
        v = (int)((s1 ^ s2) & 1u);
    }
}

// r(2k), r(2k+1) of DMRS symbol m of slot t: the caller's base_seq, or generated (alpha = 0)
__device__ __forceinline__ void tp_dmrs_pair(const TpDmrs& c, const double2* __restrict__ base_seq, int t, int m, int u,
                                             int v, int k, double2& r0, double2& r1) {
    if (base_seq) {
        const double2* b = base_seq + ((int64_t)t * c.S + m) * c.MZC + 2 * k;
        r0 = b[0], r1 = b[1];
    } else {
        low_papr_point(u, v, 2 * k, c.MZC, c.NZC, r0.x, r0.y);
        low_papr_point(u, v, 2 * k + 1, c.MZC, c.NZC, r1.x, r1.y);
    }
}

// One lane per DMRS RE k of DMRS symbol m of slot t, as slot_ls_kernel (ldpc5g_slot.hip) for one
// layer: h_ls[t][m][k][r] = (Y[4k+d] conj(r(2k)) +- Y[4k+d+2] conj(r(2k+1))) * inv, d = (port/2) % 2,
// minus for odd ports (nr_pusch_dmrs.py:174-190), in float64.
template <typename C, int NR>
__global__ __launch_bounds__(kTpThreads) void tp_ls_kernel(const C* __restrict__ grid, int64_t ldg,
                                                           const int32_t* __restrict__ slots, TpDmrs c,
                                                           const double2* __restrict__ base_seq, C* __restrict__ h_ls,
                                                           int64_t ldh) {
    using R = decltype(C{}.x);
    const int t = blockIdx.z, m = blockIdx.y;
    const int N = 3 * c.rb_size;
    const int k = blockIdx.x * kTpThreads + (int)threadIdx.x;
    const int sym = tp_dmrs_sym(c, m);
    int u = 0, v = 0;
    if (!base_seq) tp_uv(c, slots[t], sym, u, v);   // uniform branch, before any lane leaves
    if (k >= N) return;
    double2 r0, r1;
    tp_dmrs_pair(c, base_seq, t, m, u, v, k, r0, r1);
    const int d = (c.port >> 1) & 1;
    const bool odd = c.port & 1;
    const C* src = grid + (int64_t)t * ldg + (int64_t)sym * c.carrier_re + 12 * c.rb_start + 4 * k + d;
    C* dst = h_ls + (int64_t)t * ldh + ((int64_t)m * N + k) * NR;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const C y0 = src[(int64_t)r * kTpSyms * c.carrier_re], y1 = src[(int64_t)r * kTpSyms * c.carrier_re + 2];
        const double y0r = (double)y0.x, y0i = (double)y0.y, y1r = (double)y1.x, y1i = (double)y1.y;
        // Y conj(r) = (yr a + yi b) + j (yi a - yr b), r = a + j b
        const double d0r = y0r * r0.x + y0i * r0.y, d0i = y0i * r0.x - y0r * r0.y;
        const double d1r = y1r * r1.x + y1i * r1.y, d1i = y1i * r1.x - y1r * r1.y;
        C o;
        o.x = (R)((odd ? d0r - d1r : d0r + d1r) * c.inv);
        o.y = (R)((odd ? d0i - d1i : d0i + d1i) * c.inv);
        dst[r] = o;
    }
}

struct TpPrecode {
    float2 w[4];   // [antenna] of the one layer
    int32_t identity;
};

// blockIdx.y == 0: one lane per data RE i, grid[t][a][re_idx[i]'s position] = w[a] sym[t][i] in
// float32 (identity: antenna 0 takes sym, the others 0).  An index outside 0 .. 14*12*rb - 1 writes
// nothing.  blockIdx.y == 1 + m: one lane per DMRS RE k of DMRS symbol m: float32(scaling r(2k)) at RE
// 4k + d and float32(+- scaling r(2k+1)) at 4k + d + 2 (nr_pusch_dmrs.py:76-101), precoded the same
// way; the other comb is left untouched.
template <int NA>
__global__ __launch_bounds__(kTpThreads) void tp_map_kernel(const float2* __restrict__ sym, int64_t ldsym,
                                                            const int32_t* __restrict__ re_idx, int64_t nre,
                                                            const int32_t* __restrict__ slots, TpDmrs c,
                                                            const double2* __restrict__ base_seq, TpPrecode P,
                                                            float2* __restrict__ grid, int64_t ldg) {
    const int t = blockIdx.z;
    float2* g = grid + (int64_t)t * ldg;
    const int nre_sym = 12 * c.rb_size;
    auto precode = [&](float2 x, int a) {
        if (P.identity) return a == 0 ? x : make_float2(0.0f, 0.0f);
        return make_float2(P.w[a].x * x.x - P.w[a].y * x.y, P.w[a].x * x.y + P.w[a].y * x.x);
    };
    if (blockIdx.y == 0) {
        const int64_t i = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
        if (i >= nre) return;
        const int32_t idx = re_idx[i];
        if (idx < 0 || idx >= kTpSyms * nre_sym) return;
        const float2 x = sym[(int64_t)t * ldsym + i];
        const int s = idx / nre_sym, re = idx - s * nre_sym;
        float2* dst = g + (int64_t)s * c.carrier_re + 12 * c.rb_start + re;
#pragma unroll
        for (int a = 0; a < NA; ++a) dst[(int64_t)a * kTpSyms * c.carrier_re] = precode(x, a);
        return;
    }
    const int m = (int)blockIdx.y - 1;
    const int N = 3 * c.rb_size;
    const int k0 = blockIdx.x * kTpThreads;
    if (k0 >= N) return;   // uniform: the launch is as wide as the data part
    const int k = k0 + (int)threadIdx.x;
    const int sm = tp_dmrs_sym(c, m);
    int u = 0, v = 0;
    if (!base_seq) tp_uv(c, slots[t], sm, u, v);
    if (k >= N) return;
    double2 r0, r1;
    tp_dmrs_pair(c, base_seq, t, m, u, v, k, r0, r1);
    const double s1 = (c.port & 1) ? -c.scaling : c.scaling;
    const float2 x0 = make_float2((float)(c.scaling * r0.x), (float)(c.scaling * r0.y));
    const float2 x1 = make_float2((float)(s1 * r1.x), (float)(s1 * r1.y));
    float2* dst = g + (int64_t)sm * c.carrier_re + 12 * c.rb_start + 4 * k + ((c.port >> 1) & 1);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        dst[(int64_t)a * kTpSyms * c.carrier_re] = precode(x0, a);
        dst[(int64_t)a * kTpSyms * c.carrier_re + 2] = precode(x1, a);
    }
}

// the checks ldpc5g_slot_rx_frontend_tp and ldpc5g_slot_map_tp share
int check_tp_dmrs(TpDmrs& c, int32_t T, int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t port, int32_t S,
                  const int32_t* sym_idx, int32_t nPuschID, int32_t hopping, const void* base_seq) {
    if (T < 1 || T > 65535) return fail(LDPC5G_ESIZE, "T=%d outside 1..65535", T);
    if (carrier_re < 12 || carrier_re % 12 || carrier_re / 12 > 275)
        return fail(LDPC5G_ESIZE, "carrier_re=%d: a multiple of 12 up to 275 PRB", carrier_re);
    if (rb_size < 1 || rb_size > 275 || !smooth235(rb_size))
        return fail(LDPC5G_ESIZE, "rb_size=%d: 2^a 3^b 5^c in 1..275 (38.211 6.3.1.4)", rb_size);
    if (rb_start < 0 || rb_start > 275 || rb_start + rb_size > carrier_re / 12)
        return fail(LDPC5G_ESIZE, "rb_start=%d + rb_size=%d beyond the carrier's %d PRB", rb_start, rb_size, carrier_re / 12);
    if (port < 0 || port > 3) return fail(LDPC5G_ESIZE, "port=%d: port 1000..1003 as 0..3", port);
    if (S < 1 || S > 4) return fail(LDPC5G_ESIZE, "S=%d DMRS symbols outside 1..4", S);
    if (!sym_idx) return fail(LDPC5G_ESIZE, "sym_idx is null");
    for (int m = 0; m < S; ++m)
        if (sym_idx[m] < 0 || sym_idx[m] > 13 || (m > 0 && sym_idx[m] <= sym_idx[m - 1]))
            return fail(LDPC5G_ESIZE, "sym_idx[%d]=%d: strictly ascending in 0..13", m, sym_idx[m]);
    if (nPuschID < 0 || nPuschID > 1007) return fail(LDPC5G_ESIZE, "nPuschID=%d outside 0..1007", nPuschID);
    if (hopping < 0 || hopping > 2) return fail(LDPC5G_ESIZE, "hopping=%d outside 0..2 (neither, group, sequence)", hopping);
    if (rb_size <= 4 && !base_seq)
        return fail(LDPC5G_ESIZE, "base_seq is null at rb_size=%d: the sequences of length 6..24 are tables "
                                  "(38.211 5.2.2.2), pass them", rb_size);
    if (!aligned(base_seq, 16)) return fail(LDPC5G_ESIZE, "base_seq is not aligned to its element size");
    c.carrier_re = carrier_re, c.rb_start = rb_start, c.rb_size = rb_size, c.S = S, c.port = port;
    for (int m = 0; m < 4; ++m) c.sym[m] = m < S ? sym_idx[m] : 0;
    c.id = nPuschID, c.hopping = hopping;
    c.MZC = 6 * rb_size, c.NZC = c.MZC == 30 ? 31 : largest_prime_below(c.MZC);
    c.scaling = pow(10.0, -3.0 / 20.0);   // nr_pusch_dmrs.py:150-154 with NumCDMGroupsWithoutData == 2
    c.inv = 1.0 / (2.0 * c.scaling);
    return LDPC5G_OK;
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
    const int NZC = MZC == 30 ? 31 : largest_prime_below(MZC);
    const dim3 g((unsigned)((MZC + kTpThreads - 1) / kTpThreads), n);
    hipLaunchKernelGGL(low_papr_kernel, g, dim3(kTpThreads), 0, (hipStream_t)stream, u, v, alpha, MZC, NZC, (double2*)out);
    return check_hip(hipGetLastError(), "low_papr_kernel launch");
}

int ldpc5g_slot_rx_frontend_tp(const void* grid, int64_t ldgrid, int32_t in_dtype, const int32_t* slots, int32_t T,
                               int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t Nr, int32_t port,
                               int32_t S, const int32_t* sym_idx, int32_t nPuschID, int32_t hopping,
                               const void* base_seq, void* h_ls, int64_t ldh, void* y, int64_t ldy, void* stream) {
    clear_error();
    if (in_dtype != LDPC5G_F32 && in_dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad grid dtype %d", in_dtype);
    if (Nr != 1 && Nr != 2 && Nr != 4) return fail(LDPC5G_ESIZE, "Nr=%d: supported Nr in {1, 2, 4}", Nr);
    TpDmrs c{};
    const int rc = check_tp_dmrs(c, T, carrier_re, rb_start, rb_size, port, S, sym_idx, nPuschID, hopping, base_seq);
    if (rc) return rc;
    const int64_t N = 3 * (int64_t)rb_size;
    if (ldgrid < (int64_t)Nr * kTpSyms * carrier_re)
        return fail(LDPC5G_ESIZE, "grid stride %lld shorter than Nr*14*carrier_re", (long long)ldgrid);
    if (h_ls && ldh < S * N * Nr) return fail(LDPC5G_ESIZE, "h_ls stride %lld shorter than S*N*Nr", (long long)ldh);
    if (y && ldy < kTpSyms * 4 * N * Nr) return fail(LDPC5G_ESIZE, "y stride %lld shorter than 14*12*rb_size*Nr", (long long)ldy);
    if (!grid || !slots) return fail(LDPC5G_ESIZE, "null buffer (grid, slots)");
    if (!h_ls && !y) return fail(LDPC5G_ESIZE, "null buffer: both h_ls and y are NULL, nothing to do");
    const size_t al = in_dtype == LDPC5G_F64 ? 16 : 8;
    if (!aligned(grid, al) || !aligned(h_ls, al) || !aligned(y, al) || !aligned(slots, 4))
        return fail(LDPC5G_ESIZE, "a buffer is not aligned to its element size");
    hipStream_t st = (hipStream_t)stream;
    if (h_ls) {
        const dim3 g((unsigned)((N + kTpThreads - 1) / kTpThreads), S, T), b(kTpThreads);
        const double2* bs = (const double2*)base_seq;
#define LDPC5G_TP_LS(C, NR) \
    hipLaunchKernelGGL((tp_ls_kernel<C, NR>), g, b, 0, st, (const C*)grid, ldgrid, slots, c, bs, (C*)h_ls, ldh)
#define LDPC5G_TP_LS_NR(C) \
    if (Nr == 1) LDPC5G_TP_LS(C, 1); else if (Nr == 2) LDPC5G_TP_LS(C, 2); else LDPC5G_TP_LS(C, 4)
        if (in_dtype == LDPC5G_F32) { LDPC5G_TP_LS_NR(float2); } else { LDPC5G_TP_LS_NR(double2); }
#undef LDPC5G_TP_LS_NR
#undef LDPC5G_TP_LS
        const int rl = check_hip(hipGetLastError(), "tp_ls_kernel launch");
        if (rl) return rl;
    }
    if (y) {   // the extraction does not depend on the DMRS: the existing kernel, through its entry point
        const int32_t ports[1] = {port};
        return ldpc5g_slot_rx_frontend(grid, ldgrid, in_dtype, slots, T, carrier_re, rb_start, rb_size, Nr, 1, ports, S,
                                       sym_idx, 0, 0, 2, nullptr, 0, y, ldy, stream);
    }
    return LDPC5G_OK;
}

int ldpc5g_slot_map_tp(const void* sym, int64_t ldsym, const int32_t* re_idx, int64_t nre, const int32_t* slots,
                       int32_t T, int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t num_ant, int32_t port,
                       const float* precoding, int32_t S, const int32_t* sym_idx, int32_t nPuschID, int32_t hopping,
                       const void* base_seq, void* grid, int64_t ldgrid, void* stream) {
    clear_error();
    if (num_ant != 1 && num_ant != 2 && num_ant != 4) return fail(LDPC5G_ESIZE, "num_ant=%d: supported num_ant in {1, 2, 4}", num_ant);
    TpDmrs c{};
    const int rc = check_tp_dmrs(c, T, carrier_re, rb_start, rb_size, port, S, sym_idx, nPuschID, hopping, base_seq);
    if (rc) return rc;
    if (nre < 0 || nre > (int64_t)kTpSyms * 12 * rb_size) return fail(LDPC5G_ESIZE, "nre=%lld outside 0..14*12*rb_size", (long long)nre);
    if (ldgrid < (int64_t)num_ant * kTpSyms * carrier_re)
        return fail(LDPC5G_ESIZE, "grid stride %lld shorter than num_ant*14*carrier_re", (long long)ldgrid);
    if (nre > 0 && ldsym < nre) return fail(LDPC5G_ESIZE, "sym stride %lld shorter than nre", (long long)ldsym);
    if (!grid || !slots || (nre > 0 && (!sym || !re_idx))) return fail(LDPC5G_ESIZE, "null buffer (sym, re_idx, slots, grid)");
    if (!aligned(grid, 8) || !aligned(sym, 8) || !aligned(re_idx, 4) || !aligned(slots, 4))
        return fail(LDPC5G_ESIZE, "a buffer is not aligned to its element size");
    TpPrecode P{};
    P.identity = precoding ? 0 : 1;
    if (precoding)
        for (int a = 0; a < num_ant; ++a) P.w[a] = make_float2(precoding[2 * a], precoding[2 * a + 1]);
    const int64_t N = 3 * (int64_t)rb_size;
    const int64_t wide = nre > N ? nre : N;
    const dim3 g((unsigned)((wide + kTpThreads - 1) / kTpThreads), 1 + S, T), b(kTpThreads);
    hipStream_t st = (hipStream_t)stream;
    const float2* s2 = (const float2*)sym;
    const double2* bs = (const double2*)base_seq;
    float2* g2 = (float2*)grid;
#define LDPC5G_TP_MAP(NA) \
    hipLaunchKernelGGL((tp_map_kernel<NA>), g, b, 0, st, s2, ldsym, re_idx, nre, slots, c, bs, P, g2, ldgrid)
    if (num_ant == 1) LDPC5G_TP_MAP(1); else if (num_ant == 2) LDPC5G_TP_MAP(2); else LDPC5G_TP_MAP(4);
#undef LDPC5G_TP_MAP
    return check_hip(hipGetLastError(), "tp_map_kernel launch");
}

}  // extern "C"
