// ldpc5g_ofdm.hip — OFDM low-PHY, batched over T slots x Nr antennas x 14 symbols:
//   demodulation ... py5gphy/nr_lowphy/rx_lowphy_process.py:35-98 (Rx_low_phy)
//   modulation ..... py5gphy/nr_lowphy/tx_lowphy_process.py:10-80 (Tx_low_phy)
// (ldpc5g_ofdm_demod / ldpc5g_ofdm_mod, include/ldpc5g.h).
// One power-of-two Stockham (self-sorting) transform per (slot, antenna, symbol) block, resident in
// LDS, with the rest of the stage folded into its two ends: the first pass reads its points from
// HBM (demodulation: the half-CP window times the carrier phase scalar; modulation: the occupied
// bins placed at the centre of a zeroed, ifftshifted array, with the optional per-symbol timing
// ramp), the last pass writes HBM from registers (demodulation: fftshift, the half-CP ramp, the
// crop to the carrier; modulation: the carrier phase scalar and the cyclic prefix; both the
// orthonormal 1/sqrt(N)).  A symbol is read once and only what the caller keeps is written.
// Passes are radix 8 with a radix-4 tail (128 = 8 4 4 ... 4096 = 8 8 8 8), all compile-time.  A
// workgroup of 256 threads holds 2048 points (G = 2048 / N blocks; one block at N = 4096), i.e. 256
// radix-8 butterflies per pass, in ONE buffer: a thread keeps its butterflies (at most 16 points) in
// registers across a barrier and writes them back where the pass read.  The first pass writes runs
// of 1 point 8 apart: the buffer carries one pad per 32 doubles, which spreads them over all banks.
// Twiddles: a quarter-wave LDS table cos(2 pi m / N), m = 0..N/4, one sincospi of the exact
// rational per entry, the rest of the circle by symmetry; a radix-8 butterfly looks up w, w^2, w^4
// and forms the other four by products.  The half-CP ramp is an entry of the same table.
// float64 arithmetic whatever the storage type, a fixed operation order, no atomics.
#include <math.h>
#include <stdint.h>

#include "ldpc5g_common.h"

namespace ldpc5g_impl {
namespace {

constexpr int kOfThreads = 256;
constexpr int kOfPack = 2048;   // points of a workgroup (N = 4096: one block)
constexpr int kOfSyms = 14;

struct OfdmArgs {
    int64_t ld_td_slot, ld_td_ant, ld_g_slot, ld_g_ant;   // complex elements
    int64_t carrier_mod, fs;   // carrier_hz mod fs in 0..fs-1; fs = N scs 1000
    int32_t nblk;              // T * Nr * 14
    int32_t Nr, carrier_re;
    int32_t cp_short, cp_long, long7;   // long7: symbol 7 has the long prefix too (15 kHz)
    int32_t h;                 // cp_short / 2
    double scs;                // kHz, as the reference multiplies it
};

struct OfBlk {
    int64_t td, g;   // element offsets of the symbol's first sample (prefix included) and first RE
    int32_t t, sym, cp, n0;   // n0: samples of the slot before the symbol's useful part
    bool ok;
};

template <int N>
__device__ __forceinline__ OfBlk of_block(const OfdmArgs& a, int blk) {
    OfBlk b;
    b.ok = blk < a.nblk;
    const int bb = b.ok ? blk : 0;
    const int tr = bb / kOfSyms;
    b.sym = bb - tr * kOfSyms;
    b.t = tr / a.Nr;
    const int r = tr - b.t * a.Nr;
    const bool lng = b.sym == 0 || (a.long7 && b.sym == 7);
    const int before = (b.sym > 0 ? 1 : 0) + ((a.long7 && b.sym > 7) ? 1 : 0);
    b.cp = lng ? a.cp_long : a.cp_short;
    const int off = b.sym * (N + a.cp_short) + before * (a.cp_long - a.cp_short);
    b.n0 = off + b.cp;
    b.td = (int64_t)b.t * a.ld_td_slot + (int64_t)r * a.ld_td_ant + off;
    b.g = (int64_t)b.t * a.ld_g_slot + (int64_t)r * a.ld_g_ant + (int64_t)b.sym * a.carrier_re;
    return b;
}

// exp(sgn 2 pi j carrier_hz n0 / fs): the phase is the exact rational (carrier_hz n0 mod fs) / fs
__device__ __forceinline__ void of_carrier(const OfdmArgs& a, int n0, double sgn, double& c, double& s) {
    const int64_t num = (a.carrier_mod * (int64_t)n0) % a.fs;   // below 2^27 * 2^16
    double sn, cs;
    sincospi(2.0 * (double)num / (double)a.fs, &sn, &cs);
    c = cs, s = sgn * sn;
}

__host__ __device__ constexpr int of_slot(int i) { return i + (i >> 5); }

// exp(sgn 2 pi i j / N), 0 <= j < N, from tab[m] = cos(2 pi m / N), m = 0..N/4
template <int N>
__device__ __forceinline__ void of_tw(const double* __restrict__ tab, int j, double sgn, double& c, double& s) {
    constexpr int Q = N / 4;
    const int q = (int)((unsigned)j / (unsigned)Q), m = j & (Q - 1);
    const double a = tab[m], b = tab[Q - m];
    const double cc = (q & 1) ? b : a, ss = (q & 1) ? a : b;
    c = (q == 1 || q == 2) ? -cc : cc;
    s = sgn * ((q >= 2) ? -ss : ss);
}

// (a + i b) (c + i s)
__device__ __forceinline__ void of_mul(double& a, double& b, double c, double s) {
    const double x = a * c - b * s, y = a * s + b * c;
    a = x, b = y;
}

// DFT_R of v in place; SG = -1 forward (exp(-2 pi i / R)), +1 inverse
template <int R, int SG>
__device__ __forceinline__ void of_butterfly(double (&vr)[R], double (&vi)[R]) {
    constexpr double sgn = (double)SG;
    if constexpr (R == 4) {
        const double s0r = vr[0] + vr[2], s0i = vi[0] + vi[2];
        const double d0r = vr[0] - vr[2], d0i = vi[0] - vi[2];
        const double s1r = vr[1] + vr[3], s1i = vi[1] + vi[3];
        const double d1r = vr[1] - vr[3], d1i = vi[1] - vi[3];
        const double er = -sgn * d1i, ei = sgn * d1r;   // sgn i (d1)
        vr[0] = s0r + s1r, vi[0] = s0i + s1i;
        vr[2] = s0r - s1r, vi[2] = s0i - s1i;
        vr[1] = d0r + er, vi[1] = d0i + ei;
        vr[3] = d0r - er, vi[3] = d0i - ei;
    } else {
        static_assert(R == 8, "radix 4 or 8");
        double er[4] = {vr[0], vr[2], vr[4], vr[6]}, ei[4] = {vi[0], vi[2], vi[4], vi[6]};
        double pr[4] = {vr[1], vr[3], vr[5], vr[7]}, pi[4] = {vi[1], vi[3], vi[5], vi[7]};
        of_butterfly<4, SG>(er, ei);
        of_butterfly<4, SG>(pr, pi);
        const double h = 0.70710678118654752440;   // w = (1 + sgn i) h, w^2 = sgn i, w^3 = (-1 + sgn i) h
        double t = pr[1];
        pr[1] = h * (t - sgn * pi[1]), pi[1] = h * (pi[1] + sgn * t);
        t = pr[2];
        pr[2] = -sgn * pi[2], pi[2] = sgn * t;
        t = pr[3];
        pr[3] = h * (-t - sgn * pi[3]), pi[3] = h * (sgn * t - pi[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            vr[k] = er[k] + pr[k], vi[k] = ei[k] + pi[k];
            vr[k + 4] = er[k] - pr[k], vi[k + 4] = ei[k] - pi[k];
        }
    }
}

constexpr int of_log2(int n) { return n <= 1 ? 0 : 1 + of_log2(n / 2); }
// the radix of the pass that follows NS transformed points: 8 while that leaves a power of four
constexpr int of_radix(int N, int NS) {
    const int e = of_log2(N / NS);
    return (e >= 3 && e != 4) ? 8 : 4;
}

template <typename C, bool DEMOD, int N>
struct OfCtx {
    const C* __restrict__ src;
    C* __restrict__ dst;
    const double* __restrict__ dm;
    double *re, *im, *tab;
    int blk0;
};

// point m of the first pass's input; (pc, ps) is the carrier scalar (demodulation) or pc the
// symbol's dm (modulation)
template <typename C, bool DEMOD, int N>
__device__ __forceinline__ void of_load(const OfdmArgs& a, const OfCtx<C, DEMOD, N>& x, const OfBlk& b, int m,
                                        double pc, double ps, double& vr, double& vi) {
    using S = decltype(C{}.x);
    if constexpr (DEMOD) {
        const C v = x.src[b.td + (b.cp - a.h) + m];
        vr = (double)v.x, vi = (double)v.y;
        if (a.carrier_mod) of_mul(vr, vi, pc, ps);
    } else {
        // ifftshift: input m of the transform is position (m + N/2) mod N of the centred array
        const int k = ((m + N / 2) & (N - 1)) - (N - a.carrier_re) / 2;
        vr = 0.0, vi = 0.0;
        if (k >= 0 && k < a.carrier_re) {
            const C v = x.src[b.g + k];
            vr = (double)v.x, vi = (double)v.y;
            if (x.dm) {   // exp(2 pi j k scs 1000 dm), the product rounded to the storage type
                double sn, cs;
                sincos(((((2.0 * M_PI) * (double)k) * a.scs) * 1000.0) * pc, &sn, &cs);
                of_mul(vr, vi, cs, sn);
                vr = (double)(S)vr, vi = (double)(S)vi;
            }
        }
    }
}

// output o of the transform
template <typename C, bool DEMOD, int N>
__device__ __forceinline__ void of_store(const OfdmArgs& a, const OfCtx<C, DEMOD, N>& x, const OfBlk& b, int o,
                                         double pc, double ps, double vr, double vi, double scale) {
    using S = decltype(C{}.x);
    if constexpr (DEMOD) {
        const int i = (o + N / 2) & (N - 1);   // fftshift
        const int k = i - (N - a.carrier_re) / 2;
        if (k < 0 || k >= a.carrier_re) return;
        double c, s;
        of_tw<N>(x.tab, (a.h * i) & (N - 1), 1.0, c, s);
        of_mul(vr, vi, c, s);
        C v;
        v.x = (S)(vr * scale), v.y = (S)(vi * scale);
        x.dst[b.g + k] = v;
    } else {
        vr *= scale, vi *= scale;
        if (a.carrier_mod) of_mul(vr, vi, pc, ps);
        C v;
        v.x = (S)vr, v.y = (S)vi;
        x.dst[b.td + b.cp + o] = v;
        if (o >= N - b.cp) x.dst[b.td + (o - (N - b.cp))] = v;
    }
}

// The pass after NS transformed points, then the rest.  Butterfly j < N/R of a block reads points
// j + r N/R, turns point r by w^(r k), k = j mod NS, and writes the DFT_R to (j / NS) NS R + k + r NS.
template <typename C, bool DEMOD, int N, int NS>
__device__ __forceinline__ void of_pass(const OfdmArgs& a, const OfCtx<C, DEMOD, N>& x) {
    constexpr int G = N >= kOfPack ? 1 : kOfPack / N;
    constexpr int R = of_radix(N, NS);
    constexpr int SG = DEMOD ? -1 : 1;
    constexpr bool FIRST = NS == 1, LAST = NS * R == N;
    constexpr int nb = N / R, step = nb / NS;
    constexpr int ITER = G * nb / kOfThreads;
    static_assert(ITER >= 1 && ITER * kOfThreads == G * nb && ITER * R <= 16, "a thread holds at most 16 points");
    double vr[ITER][R], vi[ITER][R];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int i = (int)threadIdx.x + it * kOfThreads;
        const int g = i / nb, j = i & (nb - 1);
        if constexpr (FIRST) {
            const OfBlk b = of_block<N>(a, x.blk0 + g);
            double pc = 1.0, ps = 0.0;
            if constexpr (DEMOD) {
                if (a.carrier_mod) of_carrier(a, b.n0, 1.0, pc, ps);
            } else {
                if (x.dm && b.ok) pc = x.dm[(int64_t)b.t * kOfSyms + b.sym];
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                vr[it][r] = 0.0, vi[it][r] = 0.0;
                if (b.ok) of_load<C, DEMOD, N>(a, x, b, j + r * nb, pc, ps, vr[it][r], vi[it][r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int s = of_slot(g * N + j + r * nb);
                vr[it][r] = x.re[s], vi[it][r] = x.im[s];
            }
            const int t1 = (j & (NS - 1)) * step;
            double c1, s1, c2, s2;
            of_tw<N>(x.tab, t1, (double)SG, c1, s1);
            of_tw<N>(x.tab, 2 * t1, (double)SG, c2, s2);
            double c3 = c1, s3 = s1;
            of_mul(c3, s3, c2, s2);
            of_mul(vr[it][1], vi[it][1], c1, s1);
            of_mul(vr[it][2], vi[it][2], c2, s2);
            of_mul(vr[it][3], vi[it][3], c3, s3);
            if constexpr (R == 8) {
                double c4, s4;
                of_tw<N>(x.tab, 4 * t1, (double)SG, c4, s4);
                of_mul(vr[it][4], vi[it][4], c4, s4);
                double c = c4, s = s4;
                of_mul(c, s, c1, s1);
                of_mul(vr[it][5], vi[it][5], c, s);
                c = c4, s = s4;
                of_mul(c, s, c2, s2);
                of_mul(vr[it][6], vi[it][6], c, s);
                c = c4, s = s4;
                of_mul(c, s, c3, s3);
                of_mul(vr[it][7], vi[it][7], c, s);
            }
        }
        of_butterfly<R, SG>(vr[it], vi[it]);
    }
    if constexpr (!FIRST && !LAST) __syncthreads();   // every point of the pass is in registers
    if constexpr (LAST) {
        const double scale = 1.0 / sqrt((double)N);   // both directions orthonormal: fft / sqrt(N), ifft (its 1/N) * sqrt(N)
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int i = (int)threadIdx.x + it * kOfThreads;
            const int g = i / nb, j = i & (nb - 1);   // NS = nb: q = 0, k = j
            const OfBlk b = of_block<N>(a, x.blk0 + g);
            if (!b.ok) continue;
            double pc = 1.0, ps = 0.0;
            if constexpr (!DEMOD) {
                if (a.carrier_mod) of_carrier(a, b.n0, -1.0, pc, ps);
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
                of_store<C, DEMOD, N>(a, x, b, j + r * NS, pc, ps, vr[it][r], vi[it][r], scale);
        }
    } else {
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int i = (int)threadIdx.x + it * kOfThreads;
            const int g = i / nb, j = i & (nb - 1);
            const int q = j / NS, k = j & (NS - 1);
            const int o = g * N + q * NS * R + k;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int s = of_slot(o + r * NS);
                x.re[s] = vr[it][r], x.im[s] = vi[it][r];
            }
        }
        __syncthreads();
        of_pass<C, DEMOD, N, NS * R>(a, x);
    }
}

template <int N>
constexpr int of_buf() { return of_slot((N >= kOfPack ? N : kOfPack) - 1) + 1; }   // doubles of one padded buffer
template <int N>
constexpr size_t of_lds_bytes() { return ((size_t)2 * of_buf<N>() + N / 4 + 1) * sizeof(double); }

template <typename C, bool DEMOD, int N>
__global__ __launch_bounds__(kOfThreads) void ofdm_kernel(const C* __restrict__ src, C* __restrict__ dst,
                                                          const double* __restrict__ dm, OfdmArgs a) {
    extern __shared__ __align__(16) unsigned char of_smem[];
    constexpr int G = N >= kOfPack ? 1 : kOfPack / N;
    OfCtx<C, DEMOD, N> x;
    x.src = src, x.dst = dst, x.dm = dm;
    x.re = (double*)of_smem, x.im = x.re + of_buf<N>(), x.tab = x.im + of_buf<N>();
    x.blk0 = (int)blockIdx.x * G;   // the last workgroup of a launch may hold fewer than G blocks
    for (int m = threadIdx.x; m <= N / 4; m += kOfThreads) {
        double s, c;
        sincospi((double)(2 * m) / (double)N, &s, &c);
        x.tab[m] = c;
    }
    of_pass<C, DEMOD, N, 1>(a, x);   // its first barrier publishes the table
}

template <typename C, bool DEMOD, int N>
int of_launch_n(const void* src, void* dst, const double* dm, const OfdmArgs& a, hipStream_t st) {
    constexpr int G = N >= kOfPack ? 1 : kOfPack / N;
    constexpr size_t lds = of_lds_bytes<N>();
    if constexpr (lds > 64 * 1024) {
        const int rc = set_lds_once<ofdm_kernel<C, DEMOD, N>>(lds);
        if (rc) return rc;
    }
    const unsigned nwg = (unsigned)((a.nblk + G - 1) / G);
    hipLaunchKernelGGL((ofdm_kernel<C, DEMOD, N>), dim3(nwg), dim3(kOfThreads), lds, st, (const C*)src, (C*)dst, dm, a);
    return check_hip(hipGetLastError(), "ofdm_kernel launch");
}

template <typename C, bool DEMOD>
int of_launch(int nfft, const void* src, void* dst, const double* dm, const OfdmArgs& a, hipStream_t st) {
    switch (nfft) {
        case 128: return of_launch_n<C, DEMOD, 128>(src, dst, dm, a, st);
        case 256: return of_launch_n<C, DEMOD, 256>(src, dst, dm, a, st);
        case 512: return of_launch_n<C, DEMOD, 512>(src, dst, dm, a, st);
        case 1024: return of_launch_n<C, DEMOD, 1024>(src, dst, dm, a, st);
        case 2048: return of_launch_n<C, DEMOD, 2048>(src, dst, dm, a, st);
        default: return of_launch_n<C, DEMOD, 4096>(src, dst, dm, a, st);
    }
}

inline bool of_aligned(const void* p, size_t al) { return ((uintptr_t)p % al) == 0; }

// the checks the two entry points share; `ant` names the antenna count in the messages
int of_check(OfdmArgs& a, const char* ant, const void* td, int64_t ld_td_slot, int64_t ld_td_ant, const void* grid,
             int64_t ld_g_slot, int64_t ld_g_ant, int32_t dtype, int32_t T, int32_t Nr, int32_t nfft,
             int32_t carrier_re, int32_t scs, int64_t carrier_hz) {
    if (dtype != LDPC5G_F32 && dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad dtype %d", dtype);
    if (T < 1 || T > 65535) return fail(LDPC5G_ESIZE, "T=%d outside 1..65535", T);
    if (Nr != 1 && Nr != 2 && Nr != 4) return fail(LDPC5G_ESIZE, "%s=%d: supported %s in {1, 2, 4}", ant, Nr, ant);
    if (nfft != 128 && nfft != 256 && nfft != 512 && nfft != 1024 && nfft != 2048 && nfft != 4096)
        return fail(LDPC5G_ESIZE, "nfft=%d: one of 128, 256, 512, 1024, 2048, 4096", nfft);
    if (carrier_re < 12 || carrier_re % 12 || carrier_re > nfft)
        return fail(LDPC5G_ESIZE, "carrier_re=%d: a multiple of 12 in 12..nfft=%d", carrier_re, nfft);
    if (scs != 15 && scs != 30) return fail(LDPC5G_ESIZE, "scs=%d: 15 or 30 (kHz)", scs);
    const int64_t row_td = 15 * (int64_t)nfft, row_g = (int64_t)kOfSyms * carrier_re;
    if (T > 1 && ld_td_slot < row_td)
        return fail(LDPC5G_ESIZE, "ld_td_slot=%lld shorter than a slot of 15*nfft samples", (long long)ld_td_slot);
    if (Nr > 1 && ld_td_ant < row_td)
        return fail(LDPC5G_ESIZE, "ld_td_ant=%lld shorter than a slot of 15*nfft samples", (long long)ld_td_ant);
    if (T > 1 && ld_g_slot < row_g)
        return fail(LDPC5G_ESIZE, "ld_g_slot=%lld shorter than 14*carrier_re", (long long)ld_g_slot);
    if (Nr > 1 && ld_g_ant < row_g)
        return fail(LDPC5G_ESIZE, "ld_g_ant=%lld shorter than 14*carrier_re", (long long)ld_g_ant);
    if (!td) return fail(LDPC5G_ESIZE, "null buffer (td)");
    if (!grid) return fail(LDPC5G_ESIZE, "null buffer (grid)");
    const size_t al = dtype == LDPC5G_F64 ? 16 : 8;
    if (!of_aligned(td, al)) return fail(LDPC5G_ESIZE, "td is not aligned to its element size");
    if (!of_aligned(grid, al)) return fail(LDPC5G_ESIZE, "grid is not aligned to its element size");
    const int sc = 4096 / nfft;
    a.ld_td_slot = ld_td_slot, a.ld_td_ant = ld_td_ant, a.ld_g_slot = ld_g_slot, a.ld_g_ant = ld_g_ant;
    a.fs = (int64_t)nfft * scs * 1000;
    a.carrier_mod = ((carrier_hz % a.fs) + a.fs) % a.fs;
    a.nblk = T * Nr * kOfSyms;
    a.Nr = Nr, a.carrier_re = carrier_re;
    a.cp_short = 288 / sc, a.cp_long = (scs == 15 ? 320 : 352) / sc, a.long7 = scs == 15;
    a.h = a.cp_short / 2;
    a.scs = (double)scs;
    return LDPC5G_OK;
}

}  // namespace
}  // namespace ldpc5g_impl

using namespace ldpc5g_impl;

extern "C" {

int ldpc5g_ofdm_demod(const void* td, int64_t ld_td_slot, int64_t ld_td_ant, void* grid, int64_t ld_g_slot,
                      int64_t ld_g_ant, int32_t dtype, int32_t T, int32_t Nr, int32_t nfft, int32_t carrier_re,
                      int32_t scs, int64_t carrier_hz, void* stream) {
    clear_error();
    OfdmArgs a{};
    const int rc = of_check(a, "Nr", td, ld_td_slot, ld_td_ant, grid, ld_g_slot, ld_g_ant, dtype, T, Nr, nfft,
                            carrier_re, scs, carrier_hz);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    return dtype == LDPC5G_F64 ? of_launch<double2, true>(nfft, td, grid, nullptr, a, st)
                               : of_launch<float2, true>(nfft, td, grid, nullptr, a, st);
}

int ldpc5g_ofdm_mod(const void* grid, int64_t ld_g_slot, int64_t ld_g_ant, const double* dm, void* td,
                    int64_t ld_td_slot, int64_t ld_td_ant, int32_t dtype, int32_t T, int32_t num_ant, int32_t nfft,
                    int32_t carrier_re, int32_t scs, int64_t carrier_hz, void* stream) {
    clear_error();
    OfdmArgs a{};
    const int rc = of_check(a, "num_ant", td, ld_td_slot, ld_td_ant, grid, ld_g_slot, ld_g_ant, dtype, T, num_ant,
                            nfft, carrier_re, scs, carrier_hz);
    if (rc) return rc;
    if (!of_aligned(dm, 8)) return fail(LDPC5G_ESIZE, "dm is not aligned to its element size");
    hipStream_t st = (hipStream_t)stream;
    return dtype == LDPC5G_F64 ? of_launch<double2, false>(nfft, grid, td, dm, a, st)
                               : of_launch<float2, false>(nfft, grid, td, dm, a, st);
}

}  // extern "C"
