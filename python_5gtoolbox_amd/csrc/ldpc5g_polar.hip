// ldpc5g_polar.hip — TS 38.212 polar code (§5.3.1, §5.4.1): host-built plan, batched encode, rate
// matching / recovery, and the SC / CA-PC-SCL decoder of DESIGN.md §4.13 in float64.
//
// Decoder: one 64-lane workgroup (one wave) per codeword, so every exchange through LDS is ordered
// by a single-wave barrier.  Lane l owns path slot l (L <= 32): its metric lives in the lane's
// registers; LLR layers, packed partial sums and decided bits live in LDS.  An LLR layer is always
// rewritten whole, so a clone shares its parent's layers by index (own[layer][path]) and takes a
// private array only when it next writes that layer: no LLR is ever copied.
#include "ldpc5g_common.h"
#include "ldpc5g_polar_tables.h"

#include <math.h>
#include <string.h>

#include <vector>

namespace ldpc5g_impl {
namespace {

constexpr uint32_t kPolarMagic = 0x504c5235u;   // "5RLP"
constexpr uint32_t kPolarVersion = 1;
constexpr int kPolarLdsMax = 160 * 1024;
constexpr int kPolarWsSlots = 1024;   // workgroups of a decode that uses the global workspace

struct PolarPlan {   // header of the plan blob; offsets are bytes from the blob's start
    uint32_t magic, version;
    int32_t bytes;
    int32_t K, E, nMax, iIL, crclen, padCRC, rnti;
    int32_t N, n, nPC, nPCwm, qPC[3], mode;   // mode: 0 repetition, 1 puncturing, 2 shortening
    uint32_t crc_mask24;                      // bit c: mask of distributed CRC bit c
    int32_t off_F, off_kind, off_cksrc, off_usrc, off_pil, off_dep, off_pcmask, off_crcmask, off_il, off_ilinv;
    int32_t T, pad;
};

enum : uint8_t { kFrozen = 0, kInfo = 1, kPc = 2, kCrc = 3 };   // kind[phase] & 3; index in the high bits

constexpr int kSub[32] = {0,  1,  2,  4,  3,  5,  6,  7,  8,  16, 9,  17, 10, 18, 11, 19,
                          12, 20, 13, 21, 14, 22, 15, 23, 24, 25, 26, 28, 27, 29, 30, 31};   // Table 5.4.1.1-1

__host__ __device__ inline int sub_j(int i, int N) {   // J(i) of §5.4.1.1
    const int q = N >> 5;
#ifdef __HIP_DEVICE_COMPILE__
    constexpr int8_t t[32] = {0,  1,  2,  4,  3,  5,  6,  7,  8,  16, 9,  17, 10, 18, 11, 19,
                              12, 20, 13, 21, 14, 22, 15, 23, 24, 25, 26, 28, 27, 29, 30, 31};
    return t[i / q] * q + (i & (q - 1));
#else
    return kSub[i / q] * q + (i & (q - 1));
#endif
}

uint32_t crc_poly(int L) { return L == 6 ? 0x21u : L == 11 ? 0x621u : 0xB2B117u; }

// remainder register after one more message bit (M(x) x^L mod G, MSB first)
__host__ __device__ inline uint32_t crc_step(uint32_t reg, int bit, int L, uint32_t g) {
    const uint32_t fb = ((reg >> (L - 1)) & 1u) ^ (uint32_t)bit;
    reg = (reg << 1) & ((1u << L) - 1u);
    return fb ? reg ^ g : reg;
}

int ceil_log2(int64_t v) {
    int c = 0;
    while (((int64_t)1 << c) < v) ++c;
    return c;
}

// ------------------------------------------------------------------------------------------ plan
int plan_check(int K, int E, int nMax, int iIL, int crclen, int padCRC, int rnti) {
    if (!((nMax == 9 && iIL == 1 && crclen == 24) || (nMax == 10 && iIL == 0 && (crclen == 6 || crclen == 11))))
        return fail(LDPC5G_ESIZE, "(nMax, iIL, CRCLEN)=(%d, %d, %d): one of (9, 1, 24), (10, 0, 6), (10, 0, 11)", nMax,
                    iIL, crclen);
    if (E < 1 || E > 8192) return fail(LDPC5G_ESIZE, "E=%d outside 1..8192", E);
    if (padCRC != 0 && padCRC != 1) return fail(LDPC5G_ESIZE, "padCRC=%d: 0 or 1", padCRC);
    if (rnti < 0 || rnti > 0xffffff) return fail(LDPC5G_ESIZE, "rnti=%d outside 0..2^24-1", rnti);
    if (K <= crclen) return fail(LDPC5G_ESIZE, "K=%d does not exceed its CRC of %d bits", K, crclen);
    if (nMax == 10 && !((K >= 18 && K <= 25) || K > 30))
        return fail(LDPC5G_ESIZE, "K=%d outside the UL ranges 18..25 and > 30", K);
    if (nMax == 10 && K > 1023) return fail(LDPC5G_ESIZE, "K=%d exceeds N=1024", K);
    if (iIL && K > kPolarKilMax) return fail(LDPC5G_ESIZE, "K=%d exceeds the interleaver's %d", K, kPolarKilMax);
    return LDPC5G_OK;
}

int64_t plan_build(int K, int E, int nMax, int iIL, int crclen, int padCRC, int rnti, void* out, int64_t cap) {
    if (int rc = plan_check(K, E, nMax, iIL, crclen, padCRC, rnti)) return rc;
    // N of §5.3.1
    const int c = ceil_log2(E);   // E > K > CRCLEN >= 6, so c >= 3
    const int n1 = (8 * E <= 9 * (1 << (c - 1)) && 16 * K < 9 * E) ? c - 1 : c;
    const int n2 = ceil_log2(8 * (int64_t)K);
    int n = n1 < n2 ? n1 : n2;
    if (nMax < n) n = nMax;
    if (n < 5) n = 5;
    const int N = 1 << n;
    int nPC = 0, nPCwm = 0;
    if (nMax == 10 && K <= 25) nPC = 3, nPCwm = (E - K + 3 > 192) ? 1 : 0;
    if (K + nPC > E) return fail(LDPC5G_ESIZE, "K + nPC = %d exceeds E=%d", K + nPC, E);
    if (K + nPC > N) return fail(LDPC5G_ESIZE, "K + nPC = %d exceeds N=%d", K + nPC, N);
    const int mode = E >= N ? 0 : (16 * K <= 7 * E ? 1 : 2);
    // pre-frozen set of §5.4.1.1
    std::vector<uint8_t> pre(N, 0);
    if (mode == 1) {
        for (int i = 0; i < N - E; ++i) pre[sub_j(i, N)] = 1;
        const int ulim = 4 * E >= 3 * N ? (3 * N - 2 * E + 3) / 4 : (9 * N - 4 * E + 15) / 16;
        for (int i = 0; i < ulim && i < N; ++i) pre[i] = 1;
    } else if (mode == 2) {
        for (int i = E; i < N; ++i) pre[sub_j(i, N)] = 1;
    }
    std::vector<int> qI;   // most reliable first
    for (int i = kPolarNmax - 1; i >= 0 && (int)qI.size() < K + nPC; --i) {
        const int q = kPolarQ[i];
        if (q < N && !pre[q]) qI.push_back(q);
    }
    if ((int)qI.size() < K + nPC)
        return fail(LDPC5G_ESIZE, "K + nPC = %d: only %d positions of N=%d are left unfrozen by rate matching", K + nPC,
                    (int)qI.size(), N);
    std::vector<uint8_t> F(N, 1);
    for (int q : qI) F[q] = 0;
    int qPC[3] = {-1, -1, -1};
    if (nPC) {
        for (int j = 0; j < nPC - nPCwm; ++j) qPC[j] = qI[qI.size() - (nPC - nPCwm) + j];
        if (nPCwm) {   // the most reliable of the minimum row weight 2^popcount among the K best
            int best = -1, bw = 99;
            for (int j = 0; j < (int)qI.size() - nPC; ++j) {
                const int w = __builtin_popcount((unsigned)qI[j]);
                if (w < bw) bw = w, best = qI[j];
            }
            qPC[nPC - 1] = best;
        }
    }
    auto is_pc = [&](int i) { return i == qPC[0] || i == qPC[1] || i == qPC[2]; };
    std::vector<int> info;
    for (int i = 0; i < N; ++i)
        if (!F[i] && !is_pc(i)) info.push_back(i);
    if ((int)info.size() != K) return fail(LDPC5G_ESIZE, "internal: %d information positions for K=%d", (int)info.size(), K);
    std::vector<int16_t> pil(K), dep(K), cksrc(K), usrc(N, -1);
    if (iIL) {
        int k = 0;
        for (int m = 0; m < kPolarKilMax; ++m)
            if (kPolarPiIlMax[m] >= kPolarKilMax - K) pil[k++] = (int16_t)(kPolarPiIlMax[m] - (kPolarKilMax - K));
    } else {
        for (int k = 0; k < K; ++k) pil[k] = (int16_t)k;
    }
    for (int k = 0; k < K; ++k) dep[pil[k]] = (int16_t)k;
    for (int i = 0; i < K; ++i) cksrc[i] = (int16_t)info[dep[i]];
    for (int k = 0; k < K; ++k) usrc[info[k]] = pil[k];
    std::vector<uint8_t> kind(N, kFrozen);
    for (int i = 0; i < N; ++i)
        if (!F[i]) kind[i] = kInfo;
    std::vector<uint32_t> pcmask(3 * 32, 0), crcmask(24 * 32, 0);
    for (int j = 0; j < nPC; ++j) {
        const int p = qPC[j];
        kind[p] = (uint8_t)(kPc | (j << 2));
        usrc[p] = (int16_t)(-2 - j);
        for (int i = p - 5; i >= 0; i -= 5)
            if (!F[i] && !is_pc(i)) pcmask[j * 32 + (i >> 5)] |= 1u << (i & 31);
    }
    uint32_t crc_mask24 = 0;
    if (iIL) {
        const int A = K - 24;
        const uint32_t g = crc_poly(24);
        uint32_t r = g;   // x^24 mod G: the remainder of the unit vector at the last position
        for (int nn = A - 1; nn >= 0; --nn) {
            for (int cb = 0; cb < 24; ++cb)
                if ((r >> (23 - cb)) & 1u) crcmask[cb * 32 + (cksrc[nn] >> 5)] ^= 1u << (cksrc[nn] & 31);
            r = ((r << 1) & 0xffffffu) ^ ((r & 0x800000u) ? g : 0u);
        }
        for (int cb = 0; cb < 24; ++cb) {
            const int p = cksrc[A + cb];
            crcmask[cb * 32 + (p >> 5)] ^= 1u << (p & 31);
            kind[p] = (uint8_t)(kCrc | (cb << 2));
        }
        if (padCRC) {
            uint32_t reg = 0;
            for (int i = 0; i < 24 + A; ++i) reg = crc_step(reg, i < 24 ? 1 : 0, 24, g);
            reg ^= (uint32_t)rnti & 0xffffffu;
            for (int cb = 0; cb < 24; ++cb)
                if ((reg >> (23 - cb)) & 1u) crc_mask24 |= 1u << cb;
        }
    }
    // channel interleaver of §5.4.1.3: f[k] = e[il[k]], e[j] = f[ilinv[j]]
    int T = 0;
    while (T * (T + 1) / 2 < E) ++T;
    std::vector<int16_t> il(E), ilinv(E);
    {
        int k = 0;
        for (int col = 0; col < T; ++col)
            for (int row = 0; row < T - col; ++row) {
                const int idx = row * T - row * (row - 1) / 2 + col;   // rows 0..row-1 hold T, T-1, ... entries
                if (idx < E) il[k++] = (int16_t)idx;
            }
        for (int j = 0; j < E; ++j) ilinv[il[j]] = (int16_t)j;
    }
    PolarPlan h{};
    auto al = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
    int64_t off = al(sizeof(PolarPlan));
    h.off_F = (int32_t)off, off = al(off + N);
    h.off_kind = (int32_t)off, off = al(off + N);
    h.off_cksrc = (int32_t)off, off = al(off + 2 * K);
    h.off_usrc = (int32_t)off, off = al(off + 2 * N);
    h.off_pil = (int32_t)off, off = al(off + 2 * K);
    h.off_dep = (int32_t)off, off = al(off + 2 * K);
    h.off_pcmask = (int32_t)off, off = al(off + 4 * 3 * 32);
    h.off_crcmask = (int32_t)off, off = al(off + 4 * 24 * 32);
    h.off_il = (int32_t)off, off = al(off + 2 * E);
    h.off_ilinv = (int32_t)off, off = al(off + 2 * E);
    if (!out) return off;
    if (cap < off) return fail(LDPC5G_ESIZE, "plan_bytes=%lld: the plan needs %lld", (long long)cap, (long long)off);
    h.magic = kPolarMagic, h.version = kPolarVersion, h.bytes = (int32_t)off;
    h.K = K, h.E = E, h.nMax = nMax, h.iIL = iIL, h.crclen = crclen, h.padCRC = padCRC, h.rnti = rnti;
    h.N = N, h.n = n, h.nPC = nPC, h.nPCwm = nPCwm, h.mode = mode, h.crc_mask24 = crc_mask24, h.T = T;
    for (int j = 0; j < 3; ++j) h.qPC[j] = qPC[j];
    uint8_t* p = (uint8_t*)out;
    memset(p, 0, (size_t)off);
    memcpy(p, &h, sizeof h);
    memcpy(p + h.off_F, F.data(), N);
    memcpy(p + h.off_kind, kind.data(), N);
    memcpy(p + h.off_cksrc, cksrc.data(), 2 * (size_t)K);
    memcpy(p + h.off_usrc, usrc.data(), 2 * (size_t)N);
    memcpy(p + h.off_pil, pil.data(), 2 * (size_t)K);
    memcpy(p + h.off_dep, dep.data(), 2 * (size_t)K);
    memcpy(p + h.off_pcmask, pcmask.data(), 4 * 3 * 32);
    memcpy(p + h.off_crcmask, crcmask.data(), 4 * 24 * 32);
    memcpy(p + h.off_il, il.data(), 2 * (size_t)E);
    memcpy(p + h.off_ilinv, ilinv.data(), 2 * (size_t)E);
    return off;
}

// the host copy of a plan, validated (magic, version, ranges the kernels index by)
int plan_open(const void* plan_host, const void* plan_dev, PolarPlan& h) {
    if (!plan_host) return fail(LDPC5G_ESIZE, "null buffer (plan_host)");
    if (!plan_dev) return fail(LDPC5G_ESIZE, "null buffer (plan_dev)");
    memcpy(&h, plan_host, sizeof h);
    if (h.magic != kPolarMagic) return fail(LDPC5G_ESIZE, "bad plan magic 0x%08x", h.magic);
    if (h.version != kPolarVersion) return fail(LDPC5G_ESIZE, "plan version %u, library %u", h.version, kPolarVersion);
    if (h.n < 5 || h.n > 10 || h.N != (1 << h.n) || h.K < 1 || h.K > h.N || h.E < 1 || h.E > 8192 || h.mode < 0 || h.mode > 2)
        return fail(LDPC5G_ESIZE, "plan fields out of range (N=%d K=%d E=%d)", h.N, h.K, h.E);
    return LDPC5G_OK;
}

int batch_check(int32_t B) {
    if (B < 1 || B > (1 << 22)) return fail(LDPC5G_ESIZE, "B=%d outside 1..2^22", B);
    return LDPC5G_OK;
}

// ---------------------------------------------------------------------------------------- encode
constexpr int kEncThreads = 256;

__global__ __launch_bounds__(kEncThreads) void polar_enc_kernel(const int8_t* __restrict__ bits, int64_t ldb,
                                                                int8_t* __restrict__ out, int64_t ldo,
                                                                const uint8_t* __restrict__ plan, int B) {
    __shared__ uint8_t u[1024];   // G codewords of N bits, G * N <= 1024 ... 512 used below N = 1024
    const PolarPlan& h = *(const PolarPlan*)plan;
    const int N = h.N, half = N >> 1;
    const int tpc = half < kEncThreads ? half : kEncThreads;   // threads per codeword
    const int G = kEncThreads / tpc;
    const int g = (int)threadIdx.x / tpc, t = (int)threadIdx.x % tpc;
    const int b = (int)blockIdx.x * G + g;   // the last workgroup may hold fewer than G codewords
    const bool live = b < B;
    const int16_t* usrc = (const int16_t*)(plan + h.off_usrc);
    const uint8_t* kind = plan + h.off_kind;
    uint8_t* x = u + g * N;
    if (live)
        for (int i = t; i < N; i += tpc) {
            const int s = usrc[i];
            x[i] = s >= 0 ? (uint8_t)(bits[(int64_t)b * ldb + s] & 1) : 0;
        }
    __syncthreads();
    if (live && t < h.nPC) {   // PC bit = cell 0 of the 5-bit cyclic register: parity of the information bits 5 apart
        const int p = h.qPC[t];
        int acc = 0;
        for (int i = p - 5; i >= 0; i -= 5)
            if ((kind[i] & 3) == kInfo) acc ^= x[i];
        x[p] = (uint8_t)acc;
    }
    __syncthreads();
    for (int hh = 1; hh < N; hh <<= 1) {   // x = u G_N, log2 N butterfly stages
        if (live)
            for (int q = t; q < half; q += tpc) {
                const int i = ((q / hh) * hh << 1) + (q & (hh - 1));
                x[i] ^= x[i + hh];
            }
        __syncthreads();
    }
    if (live)
        for (int i = t; i < N; i += tpc) out[(int64_t)b * ldo + i] = (int8_t)x[i];
}

// ------------------------------------------------------------------------- rate match / recovery
__global__ __launch_bounds__(256) void polar_rm_kernel(const int8_t* __restrict__ d, int64_t ldi, int8_t* __restrict__ f,
                                                       int64_t ldo, const uint8_t* __restrict__ plan, int B, int iBIL) {
    const PolarPlan& h = *(const PolarPlan*)plan;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)B * h.E) return;
    const int b = (int)(gid / h.E), k = (int)(gid % h.E);
    const int16_t* il = (const int16_t*)(plan + h.off_il);
    const int j = iBIL ? il[k] : k;
    const int y = h.mode == 0 ? j % h.N : (h.mode == 1 ? j + h.N - h.E : j);
    f[(int64_t)b * ldo + k] = d[(int64_t)b * ldi + sub_j(y, h.N)];
}

__global__ __launch_bounds__(256) void polar_rr_kernel(const double* __restrict__ llr, int64_t ldi, double* __restrict__ out,
                                                       int64_t ldo, const uint8_t* __restrict__ plan, int B, int iBIL,
                                                       double limit, int quirk) {
    const PolarPlan& h = *(const PolarPlan*)plan;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)B * h.N) return;
    const int b = (int)(gid / h.N), i = (int)(gid % h.N);
    const int16_t* ilinv = (const int16_t*)(plan + h.off_ilinv);
    const double* in = llr + (int64_t)b * ldi;
    const int N = h.N, E = h.E;
    double v;
    if (h.mode == 0) {   // whole copies in order, then the remainder: sequential float64 adds from 0
        const bool deil = iBIL && !quirk;
        v = 0.0;
        for (int o = i; o < E; o += N) v = v + in[deil ? ilinv[o] : o];
    } else if (h.mode == 1) {
        const int j = i - (N - E);
        v = j >= 0 ? in[iBIL ? ilinv[j] : j] : 0.0;
    } else {
        v = i < E ? in[iBIL ? ilinv[i] : i] : limit;
    }
    out[(int64_t)b * ldo + sub_j(i, N)] = v;
}

// ---------------------------------------------------------------------------------------- decode
struct PolarDecArgs {
    const double* llr;
    int64_t ldl, ldc, ws_slot;   // ws_slot: doubles of workspace per workgroup
    int8_t* ck;
    uint8_t* status;
    double* pm;
    const uint8_t* plan;
    double* ws;
    int32_t B, L, G, sc;   // G: layers 1..G live in the workspace, the rest in LDS
};

struct PolarLds {   // offsets in bytes of the dynamic LDS block
    int cand, words, own, small, total, W, Ew;
};

__host__ __device__ inline int layer_words(int N, int lam) { return (N >> lam) >= 32 ? (N >> lam) >> 5 : 1; }

__host__ __device__ inline PolarLds polar_lds(int N, int m, int L, int G) {
    PolarLds s;
    int ew = 0;
    for (int lam = 1; lam <= m; ++lam) ew += layer_words(N, lam);
    s.Ew = ew, s.W = 2 * ew + (N >> 5);
    int off = 8 * L * ((N >> G) - 1);
    s.cand = off, off += 8 * 66;        // 64 candidates + the two order statistics
    s.words = off, off += 4 * L * s.W;
    s.own = off, off += 32 * (m + 1);
    s.small = off, off += 32 * 4 + 4 * 12;   // par, clt, cls, act list; word offsets of the layers
    s.total = (off + 15) & ~15;
    return s;
}

__device__ __forceinline__ uint32_t spread16(uint32_t x) {
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

__device__ __forceinline__ int nth_bit(uint32_t f, int r) {   // index of the r-th (0-based) set bit
    for (int i = 0; i < r; ++i) f &= f - 1;
    return __ffs(f) - 1;
}

__global__ __launch_bounds__(64) void polar_dec_kernel(PolarDecArgs a) {
    extern __shared__ __align__(16) unsigned char pd_smem[];
    const PolarPlan& h = *(const PolarPlan*)a.plan;
    const int lane = (int)threadIdx.x;
    const int N = h.N, m = h.n, K = h.K, L = a.L, G = a.G;
    const PolarLds s = polar_lds(N, m, L, G);
    double* P = (double*)pd_smem;
    double* cand = (double*)(pd_smem + s.cand);
    uint32_t* words = (uint32_t*)(pd_smem + s.words);
    uint8_t* own = pd_smem + s.own;
    uint8_t* par = pd_smem + s.small;
    uint8_t* clt = par + 32;
    uint8_t* cls = par + 64;
    uint8_t* alist = par + 96;
    int* woff = (int*)(par + 128);
    const int W = s.W, Ew = s.Ew;
    const uint8_t* kind = a.plan + h.off_kind;
    const int16_t* cksrc = (const int16_t*)(a.plan + h.off_cksrc);
    const uint32_t* pcmask = (const uint32_t*)(a.plan + h.off_pcmask);
    const uint32_t* crcmask = (const uint32_t*)(a.plan + h.off_crcmask);
    double* wsg = a.ws ? a.ws + (int64_t)blockIdx.x * a.ws_slot : nullptr;
    const uint32_t Lmask = L >= 32 ? 0xffffffffu : ((1u << L) - 1u);
    const uint32_t below = lane >= 32 ? 0xffffffffu : ((1u << lane) - 1u);
    const int ldsN = N >> G;

    // element e of physical array `arr` of layer lam
    auto ld = [&](int lam, int arr, int e) -> double {
        if (lam <= G) return wsg[(int64_t)L * (N - (N >> (lam - 1))) + (int64_t)arr * (N >> lam) + e];
        return P[L * (ldsN - (N >> (lam - 1))) + arr * (N >> lam) + e];
    };
    auto st = [&](int lam, int arr, int e, double v) {
        if (lam <= G) wsg[(int64_t)L * (N - (N >> (lam - 1))) + (int64_t)arr * (N >> lam) + e] = v;
        else P[L * (ldsN - (N >> (lam - 1))) + arr * (N >> lam) + e] = v;
    };

    if (lane == 0) {
        int o = 0;
        for (int lam = 1; lam <= m; ++lam) woff[lam] = o, o += layer_words(N, lam);
    }
    for (int b = (int)blockIdx.x; b < a.B; b += (int)gridDim.x) {
        __syncthreads();
        const double* in = a.llr + (int64_t)b * a.ldl;
        for (int i = lane; i < 32 * (m + 1); i += 64) own[i] = (uint8_t)(i & 31);
        uint32_t amask = 1u;
        double PM = 0.0;
        if (lane == 0) alist[0] = 0;
        bool failed = false;
        __syncthreads();
        for (int ph = 0; ph < N; ++ph) {
            const int A = __popc(amask);
            const bool act = lane < 32 && ((amask >> lane) & 1u);
            // ---- LLRs of this phase: layers low..m, each from the one below
            const int low = ph == 0 ? 1 : m - (__ffs(ph) - 1);
            for (int lam = low; lam <= m; ++lam) {
                // a path that shares its array of this layer with a lower-numbered path takes a free one
                if (A > 1) {
                    int o = lane < 32 ? own[lam * 32 + lane] : 0;
                    uint32_t used = 0;
                    bool dup = false;
                    for (int arr = 0; arr < L; ++arr) {
                        const uint32_t mk = (uint32_t)__ballot(act && o == arr);
                        if (mk) used |= 1u << arr;
                        if (act && o == arr && (mk & below)) dup = true;
                    }
                    const uint32_t dmask = (uint32_t)__ballot(act && dup);
                    if (act && dup) own[lam * 32 + lane] = (uint8_t)nth_bit(~used & Lmask, __popc(dmask & below));
                    __syncthreads();
                }
                const int sh = m - lam, cnt = A << sh;
                const bool fstep = ((ph >> sh) & 1) == 0;
                for (int idx = lane; idx < cnt; idx += 64) {
                    const int l = alist[idx >> sh], br = idx & ((1 << sh) - 1);
                    double x, y;
                    if (lam == 1) {   // layer 0 is the bit-reversed input, shared by every path
                        x = in[__brev((unsigned)(2 * br)) >> (32 - m)];
                        y = in[__brev((unsigned)(2 * br + 1)) >> (32 - m)];
                    } else {
                        const int src = own[(lam - 1) * 32 + l];
                        x = ld(lam - 1, src, 2 * br), y = ld(lam - 1, src, 2 * br + 1);
                    }
                    double v;
                    if (fstep) {
                        const double mn = fmin(fabs(x), fabs(y));
                        v = (x == 0.0 || y == 0.0) ? 0.0 : (((x < 0.0) != (y < 0.0)) ? -mn : mn);
                    } else {
                        const uint32_t bw = words[l * W + woff[lam] + (br >> 5)];   // even-slot partial sum
                        v = ((bw >> (br & 31)) & 1u) ? y - x : y + x;
                    }
                    st(lam, own[lam * 32 + l], br, v);
                }
                __syncthreads();
            }
            // ---- decision
            const int kd = kind[ph];
            const int kt = kd & 3;
            const double v = act ? ld(m, own[m * 32 + lane], 0) : 0.0;
            const double av = fabs(v);
            const double n0 = PM + (v > 0.0 ? 0.0 : av), n1 = PM + (v > 0.0 ? av : 0.0);
            int u = 0;
            if (kt == kFrozen) {
                if (act) PM = n0;
            } else if (a.sc) {
                u = v > 0.0 ? 0 : 1;
                if (act) PM = u ? n1 : n0;
            } else {
                if (lane < 32) par[lane] = 0xff, cand[lane] = n0, cand[32 + lane] = n1;
                __syncthreads();
                uint32_t keep = amask, free_;
                bool cloner = false;
                if (2 * A <= L) {
                    cloner = act;
                    free_ = ~amask & Lmask;
                    if (act) PM = n0;
                } else {
                    // order statistics A-1 and A of the 2A candidates, by counting
                    const bool valid = ((amask >> (lane & 31)) & 1u) != 0;
                    const double c = cand[lane];
                    int cl = 0, cle = 0;
                    for (uint32_t mm = amask; mm; mm &= mm - 1) {
                        const int i = __ffs(mm) - 1;
                        const double c0 = cand[i], c1 = cand[32 + i];
                        cl += (c0 < c) + (c1 < c), cle += (c0 <= c) + (c1 <= c);
                    }
                    if (valid && cl <= A - 1 && A - 1 < cle) cand[64] = c;   // equal values: any writer will do
                    if (valid && cl <= A && A < cle) cand[65] = c;
                    __syncthreads();
                    const double thr = (cand[64] + cand[65]) / 2;
                    const bool k0 = n0 < thr, k1 = n1 < thr;
                    keep = amask & ~(uint32_t)__ballot(act && !k0 && !k1);
                    free_ = ~keep & Lmask;
                    cloner = act && k0 && k1;
                    if (act && (k0 || k1)) u = k0 ? 0 : 1, PM = u ? n1 : n0;
                }
                const uint32_t cmask = (uint32_t)__ballot(cloner);
                if (cloner) {   // the k-th cloner takes the k-th lowest free slot (there are enough unless an LLR is NaN)
                    const int t = nth_bit(free_, __popc(cmask & below));
                    if (t >= 0) par[t] = (uint8_t)lane;
                }
                __syncthreads();
                const int src = lane < 32 ? par[lane] : 0xff;
                const bool born = src != 0xff;
                const uint32_t tmask = (uint32_t)__ballot(born);
                if (born) {
                    PM = cand[32 + src], u = 1;
                    for (int lam = 1; lam <= m; ++lam) own[lam * 32 + lane] = own[lam * 32 + src];
                    const int r = __popc(tmask & below);
                    clt[r] = (uint8_t)lane, cls[r] = (uint8_t)src;
                }
                amask = keep | tmask;
                __syncthreads();
                const int nT = __popc(tmask);
                for (int idx = lane; idx < nT * W; idx += 64) {
                    const int k = idx / W, w = idx - k * W;
                    words[clt[k] * W + w] = words[cls[k] * W + w];
                }
                __syncthreads();
            }
            bool alive = lane < 32 && ((amask >> lane) & 1u);
            if (alive) {
                uint32_t* U = words + lane * W + 2 * Ew;
                if ((ph & 31) == 0) U[ph >> 5] = (uint32_t)u;
                else U[ph >> 5] |= (uint32_t)u << (ph & 31);
                words[lane * W + (ph & 1) * Ew + woff[m]] = (uint32_t)u;
            }
            if (!a.sc && (kt == kPc || kt == kCrc)) {
                const uint32_t* mk = (kt == kPc ? pcmask : crcmask) + (kd >> 2) * 32;
                uint32_t acc = 0;
                if (alive) {
                    const uint32_t* U = words + lane * W + 2 * Ew;
                    for (int w = 0; w <= (ph >> 5); ++w) acc ^= U[w] & mk[w];
                }
                const int parity = __popc(acc) & 1;
                const bool bad = kt == kPc ? (u != parity) : (parity != (int)((h.crc_mask24 >> (kd >> 2)) & 1u));
                amask &= ~(uint32_t)__ballot(alive && bad);
                alive = lane < 32 && ((amask >> lane) & 1u);
            }
            if (amask == 0) {
                failed = true;
                break;
            }
            if (alive) alist[__popc(amask & below)] = (uint8_t)lane;
            __syncthreads();
            // ---- partial sums: every trailing one of the phase folds one layer into the layer below
            if (ph & 1) {
                const int A2 = __popc(amask);
                int pp = ph;
                for (int lam = m; lam > 1 && (pp & 1); --lam) {
                    pp >>= 1;
                    const int slot = pp & 1, tw = layer_words(N, lam - 1), cnt = A2 * tw;
                    for (int idx = lane; idx < cnt; idx += 64) {
                        const int l = alist[idx / tw], w = idx % tw;
                        const uint32_t e = words[l * W + woff[lam] + (w >> 1)], o = words[l * W + Ew + woff[lam] + (w >> 1)];
                        const int shb = (w & 1) * 16;
                        words[l * W + slot * Ew + woff[lam - 1] + w] =
                            spread16(((e ^ o) >> shb) & 0xffffu) | (spread16((o >> shb) & 0xffffu) << 1);
                    }
                    __syncthreads();
                }
            }
        }
        // ---- pick the path to return
        int win = -1;
        if (!failed) {
            const bool alive = lane < 32 && ((amask >> lane) & 1u);
            bool ok = alive;
            if (alive && !a.sc && !h.iIL) {   // the final CRC with the rnti mask, one path per lane
                const uint32_t* U = words + lane * W + 2 * Ew;
                const int Lc = h.crclen;
                const uint32_t g = Lc == 6 ? 0x21u : 0x621u;
                uint32_t reg = 0, tx = 0;
                for (int i = 0; i < K; ++i) {
                    const int p = cksrc[i];
                    const int bit = (int)((U[p >> 5] >> (p & 31)) & 1u);
                    if (i < K - Lc) reg = crc_step(reg, bit, Lc, g);
                    else tx = (tx << 1) | (uint32_t)bit;
                }
                ok = (reg ^ ((uint32_t)h.rnti & ((1u << Lc) - 1u))) == tx;
            }
            const uint32_t okm = (uint32_t)__ballot(ok);
            if (lane < 32) cand[lane] = PM;
            __syncthreads();
            bool best = ok;
            for (uint32_t mm = okm; mm && best; mm &= mm - 1) {
                const int i = __ffs(mm) - 1;
                const double c = cand[i];
                if (c < PM || (c == PM && i < lane)) best = false;
            }
            const uint32_t bm = (uint32_t)__ballot(best);
            win = bm ? __ffs(bm) - 1 : -1;
        }
        int8_t* ck = a.ck + (int64_t)b * a.ldc;
        if (win < 0) {
            for (int i = lane; i < K; i += 64) ck[i] = -1;
            if (lane == 0) a.status[b] = 0, a.pm[b] = INFINITY;
        } else {
            const uint32_t* U = words + win * W + 2 * Ew;
            for (int i = lane; i < K; i += 64) {
                const int p = cksrc[i];
                ck[i] = (int8_t)((U[p >> 5] >> (p & 31)) & 1u);
            }
            if (lane == win) a.status[b] = 1, a.pm[b] = PM;
        }
    }
}

}  // namespace
}  // namespace ldpc5g_impl

using namespace ldpc5g_impl;

extern "C" {

int64_t ldpc5g_polar_plan(int32_t K, int32_t E, int32_t nMax, int32_t iIL, int32_t crclen, int32_t padCRC, int32_t rnti,
                          void* plan, int64_t plan_bytes) {
    clear_error();
    return plan_build(K, E, nMax, iIL, crclen, padCRC, rnti, plan, plan_bytes);
}

int ldpc5g_polar_encode(const void* plan_dev, const void* plan_host, const int8_t* bits, int64_t ldb, int8_t* out,
                        int64_t ldo, int32_t B, void* stream) {
    clear_error();
    PolarPlan h;
    if (int rc = plan_open(plan_host, plan_dev, h)) return rc;
    if (int rc = batch_check(B)) return rc;
    if (!bits || !out) return fail(LDPC5G_ESIZE, "null buffer (%s)", !bits ? "bits" : "out");
    if (ldb < h.K) return fail(LDPC5G_ESIZE, "ldb=%lld shorter than K=%d", (long long)ldb, h.K);
    if (ldo < h.N) return fail(LDPC5G_ESIZE, "ldo=%lld shorter than N=%d", (long long)ldo, h.N);
    const int tpc = h.N / 2 < kEncThreads ? h.N / 2 : kEncThreads, G = kEncThreads / tpc;
    hipLaunchKernelGGL(polar_enc_kernel, dim3((unsigned)((B + G - 1) / G)), dim3(kEncThreads), 0, (hipStream_t)stream, bits,
                       ldb, out, ldo, (const uint8_t*)plan_dev, B);
    return check_hip(hipGetLastError(), "polar_enc_kernel launch");
}

int ldpc5g_polar_rate_match(const void* plan_dev, const void* plan_host, const int8_t* d, int64_t ldi, int8_t* f,
                            int64_t ldo, int32_t B, int32_t iBIL, void* stream) {
    clear_error();
    PolarPlan h;
    if (int rc = plan_open(plan_host, plan_dev, h)) return rc;
    if (int rc = batch_check(B)) return rc;
    if (iBIL != 0 && iBIL != 1) return fail(LDPC5G_ESIZE, "iBIL=%d: 0 or 1", iBIL);
    if (!d || !f) return fail(LDPC5G_ESIZE, "null buffer (%s)", !d ? "d" : "f");
    if (ldi < h.N) return fail(LDPC5G_ESIZE, "ldi=%lld shorter than N=%d", (long long)ldi, h.N);
    if (ldo < h.E) return fail(LDPC5G_ESIZE, "ldo=%lld shorter than E=%d", (long long)ldo, h.E);
    const int64_t n = (int64_t)B * h.E;
    hipLaunchKernelGGL(polar_rm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d, ldi, f, ldo,
                       (const uint8_t*)plan_dev, B, iBIL);
    return check_hip(hipGetLastError(), "polar_rm_kernel launch");
}

int ldpc5g_polar_rate_recover(const void* plan_dev, const void* plan_host, const double* llr, int64_t ldi, double* out,
                              int64_t ldo, int32_t B, int32_t iBIL, double llr_limit, int32_t reference_repetition,
                              void* stream) {
    clear_error();
    PolarPlan h;
    if (int rc = plan_open(plan_host, plan_dev, h)) return rc;
    if (int rc = batch_check(B)) return rc;
    if (iBIL != 0 && iBIL != 1) return fail(LDPC5G_ESIZE, "iBIL=%d: 0 or 1", iBIL);
    if (reference_repetition != 0 && reference_repetition != 1)
        return fail(LDPC5G_ESIZE, "reference_repetition=%d: 0 or 1", reference_repetition);
    if (!llr || !out) return fail(LDPC5G_ESIZE, "null buffer (%s)", !llr ? "llr" : "out");
    if (ldi < h.E) return fail(LDPC5G_ESIZE, "ldi=%lld shorter than E=%d", (long long)ldi, h.E);
    if (ldo < h.N) return fail(LDPC5G_ESIZE, "ldo=%lld shorter than N=%d", (long long)ldo, h.N);
    const int64_t n = (int64_t)B * h.N;
    hipLaunchKernelGGL(polar_rr_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, llr, ldi, out,
                       ldo, (const uint8_t*)plan_dev, B, iBIL, llr_limit, reference_repetition);
    return check_hip(hipGetLastError(), "polar_rr_kernel launch");
}

int ldpc5g_polar_decode(const void* plan_dev, const void* plan_host, const double* llr, int64_t ldl, int8_t* ck,
                        int64_t ldc, uint8_t* status, double* pm, int32_t B, int32_t algo, int32_t L, void* stream) {
    clear_error();
    PolarPlan h;
    if (int rc = plan_open(plan_host, plan_dev, h)) return rc;
    if (int rc = batch_check(B)) return rc;
    if (algo != LDPC5G_POLAR_SC && algo != LDPC5G_POLAR_SCL) return fail(LDPC5G_ESIZE, "algo=%d: LDPC5G_POLAR_SC or _SCL", algo);
    if (L < 1 || L > 32) return fail(LDPC5G_ESIZE, "L=%d outside 1..32", L);
    if (h.N < 32 || h.N > 1024) return fail(LDPC5G_ESIZE, "N=%d outside 32..1024", h.N);
    if (!llr || !ck || !status || !pm)
        return fail(LDPC5G_ESIZE, "null buffer (%s)", !llr ? "llr" : !ck ? "ck" : !status ? "status" : "pm");
    if (((uintptr_t)llr | (uintptr_t)pm) & 7) return fail(LDPC5G_ESIZE, "llr or pm is not aligned to 8 bytes");
    if (ldl < h.N) return fail(LDPC5G_ESIZE, "ldl=%lld shorter than N=%d", (long long)ldl, h.N);
    if (ldc < h.K) return fail(LDPC5G_ESIZE, "ldc=%lld shorter than K=%d", (long long)ldc, h.K);
    PolarDecArgs a{};
    a.llr = llr, a.ldl = ldl, a.ck = ck, a.ldc = ldc, a.status = status, a.pm = pm, a.plan = (const uint8_t*)plan_dev;
    a.B = B, a.sc = algo == LDPC5G_POLAR_SC, a.L = a.sc ? 1 : L;
    int G = 0;
    while (G < h.n - 1 && polar_lds(h.N, h.n, a.L, G).total > kPolarLdsMax) ++G;
    const PolarLds s = polar_lds(h.N, h.n, a.L, G);
    if (s.total > kPolarLdsMax) return fail(LDPC5G_ESIZE, "internal: %d bytes of LDS for N=%d L=%d", s.total, h.N, a.L);
    a.G = G;
    hipStream_t st = (hipStream_t)stream;
    unsigned nwg = (unsigned)B;
    if (G > 0) {   // the largest layers in a stream-ordered workspace, one slot per resident workgroup
        if (nwg > (unsigned)kPolarWsSlots) nwg = kPolarWsSlots;
        a.ws_slot = (int64_t)a.L * (h.N - (h.N >> G));
        void* p = nullptr;
        if (int rc = check_hip(hipMallocAsync(&p, (size_t)nwg * a.ws_slot * sizeof(double), st), "hipMallocAsync(polar workspace)"))
            return rc;
        a.ws = (double*)p;
    }
    int rc = LDPC5G_OK;
    if (s.total > 64 * 1024) rc = set_lds_once<polar_dec_kernel>((size_t)kPolarLdsMax);
    if (!rc) {
        hipLaunchKernelGGL(polar_dec_kernel, dim3(nwg), dim3(64), (size_t)s.total, st, a);
        rc = check_hip(hipGetLastError(), "polar_dec_kernel launch");
    }
    if (a.ws) {
        const int rc2 = check_hip(hipFreeAsync(a.ws, st), "hipFreeAsync(polar workspace)");
        if (!rc) rc = rc2;
    }
    return rc;
}

}  // extern "C"
