// ldpc5g_phy.hip — the symbol-level steps either side of the DL-SCH chain,
// on the GPU and batched over transport blocks:
//   Gold-sequence scrambling code c(n) ....... py5gphy/common/nrPRBS.py:5-25 (gen_nrPRBS)
//   scrambling + modulation mapper ........... py5gphy/nr_pdsch/nr_pdsch_process.py:17-25,
//                                              py5gphy/common/nrModulation.py:4-42 (all seven)
//   soft demodulation + descrambling ......... py5gphy/demodulation/nr_Demodulation.py:12-46,
//                                              demod_{bpsk,pi2_bpsk,qpsk,16qam,64qam,256qam,1024qam}.py,
//                                              py5gphy/nr_pdsch/nr_pdsch.py:268-274
// All elementwise / HBM-bound.  The scrambling code is produced 32 bits per word (packed LSB
// first, bit k of word w = c(32w + k)): a thread jumps both m-sequences to its first word with
// constexpr GF(2) matrix powers T^(2^i), then steps 32 positions at a time with shifts.
#include <math.h>
#include <stdint.h>

#include "ldpc5g_common.h"
#include "ldpc5g_demod.h"
#include "ldpc5g_mod.h"
#include "ldpc5g_prbs.h"

namespace ldpc5g_impl {
namespace {

// ============================================================================ Gold sequence
// (the matrix generator make_prbs_tables and prbs_step32: ldpc5g_prbs.h, shared with ldpc5g_slot.hip)
__constant__ PrbsTables kPrbs = make_prbs_tables();

__device__ uint32_t prbs_jump(int q, uint32_t s, uint32_t n) {
    for (int i = 0; i < kPrbsPow; ++i) {
        if ((n >> i) & 1u) {
            uint32_t r = 0;
#pragma unroll
            for (int j = 0; j < 31; ++j) r ^= ((s >> j) & 1u) ? kPrbs.t[q][i][j] : 0u;
            s = r;
        }
    }
    return s;
}

constexpr int kPrbsWordsPerThread = 8;
constexpr int kPrbsLaneLog = 8;   // log2(32 * kPrbsWordsPerThread): bits per thread
static_assert(32 * kPrbsWordsPerThread == 1 << kPrbsLaneLog, "bits per thread must be 2^kPrbsLaneLog");

// T^(m 2^kPrbsLaneLog) s for m < 256: the per-thread part of the jump
__device__ __forceinline__ uint32_t prbs_jump_lane(int q, uint32_t s, uint32_t m) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if ((m >> i) & 1u) {
            uint32_t r = 0;
#pragma unroll
            for (int j = 0; j < 31; ++j) r ^= ((s >> j) & 1u) ? kPrbs.t[q][kPrbsLaneLog + i][j] : 0u;
            s = r;
        }
    }
    return s;
}

// words[t][w] = c(32w .. 32w+31) of transport block t (gen_nrPRBS(cinit[t], ...) packed).  The
// jump to the workgroup's first bit is uniform (scalar); each thread then jumps by
// threadIdx.x * 256 bits with at most 8 matrix products.
__global__ __launch_bounds__(256) void prbs_kernel(const uint32_t* __restrict__ cinit, int64_t nw,
                                                   uint32_t* __restrict__ words, int64_t ldw) {
    const int t = blockIdx.y;
    const int64_t wb = (int64_t)blockIdx.x * 256 * kPrbsWordsPerThread;
    const int64_t w0 = wb + (int64_t)threadIdx.x * kPrbsWordsPerThread;
    const uint32_t nb = 1600u + 32u * (uint32_t)wb;
    uint32_t s1 = prbs_jump(0, 1u, nb);
    uint32_t s2 = prbs_jump(1, cinit[t] & 0x7FFFFFFFu, nb);
    if (w0 >= nw) return;
    s1 = prbs_jump_lane(0, s1, threadIdx.x);
    s2 = prbs_jump_lane(1, s2, threadIdx.x);
    uint32_t* out = words + (int64_t)t * ldw;
#pragma unroll
    for (int k = 0; k < kPrbsWordsPerThread; ++k) {
        const uint32_t c = prbs_step32(s1, false) ^ prbs_step32(s2, true);
        if (w0 + k < nw) out[w0 + k] = c;
    }
}

// ======================================================================== modulation mapper
// scrambled bit b'(i) = b(i) + c(i) mod 2; symbol = (level_re + j level_im) / sqrt(scale) in the
// reference's float32 arithmetic: levels exact, then numpy's complex64 division by a real scalar,
// i.e. a multiply by the float32 reciprocal scl = 1 / float32(sqrt(scale)).
// (the levels: mod_symbol, ldpc5g_mod.h, shared with ldpc5g_uci.hip)
template <int QM, bool PI2>
__global__ __launch_bounds__(256) void scramble_modulate_kernel(const int8_t* __restrict__ bits,
                                                                int64_t ldb,
                                                                const uint32_t* __restrict__ prbs,
                                                                int64_t ldw, int64_t nsym,
                                                                float scl, float2* __restrict__ sym,
                                                                int64_t ldsym) {
    const int t = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nsym) return;
    const int8_t* b = bits + (int64_t)t * ldb + m * QM;
    uint32_t c = prbs ? prbs_bits(prbs + (int64_t)t * ldw, m * QM, QM) : 0u;
    float u[QM];
#pragma unroll
    for (int i = 0; i < QM; ++i) u[i] = 1.0f - 2.0f * (float)(((uint32_t)b[i] ^ (c >> i)) & 1u);
    sym[(int64_t)t * ldsym + m] = mod_symbol<QM, PI2>(u, m, scl);
}

// ===================================================================== soft demodulation
// (segment tables, demod_llr / demod_symbol, flip_sign, prbs_bits: ldpc5g_demod.h)
// QM = 1: BPSK LLR = 4 (re + im) A / nv (demod_bpsk.py:9); with PI2, odd symbols use
// 4 (-re + im) A / nv (demod_pi2_bpsk.py:11-12).  Tout = double only for BPSK on complex128
// input, whose reference result stays float64 (no float32 store in demod_bpsk.py).
template <int QM, bool PI2, typename Tin, typename Tout>
__global__ __launch_bounds__(256) void demod_descramble_kernel(const Tin* __restrict__ sym,
                                                               int64_t ldsym,
                                                               const float* __restrict__ nvar,
                                                               int64_t ldnv,
                                                               const uint32_t* __restrict__ prbs,
                                                               int64_t ldw, int64_t nsym, double A,
                                                               Tout* __restrict__ llr,
                                                               int64_t ldllr) {
    using C = decltype(Tin{}.x);
    const int t = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nsym) return;
    const Tin y = sym[(int64_t)t * ldsym + m];
    const C re = y.x, im = y.y;
    const C nv = (C)nvar[(int64_t)t * ldnv + m];
    const uint32_t c = prbs ? prbs_bits(prbs + (int64_t)t * ldw, m * QM, QM) : 0u;
    Tout v[QM];
    demod_symbol<QM>(re, im, nv, A, PI2 && (m & 1), v);
    Tout* out = llr + (int64_t)t * ldllr + m * QM;
#pragma unroll
    for (int i = 0; i < QM; ++i)   // descrambling: LLR * (1 - 2c), an exact sign flip
        out[i] = flip_sign(v[i], (c >> i) & 1u);
}

}  // namespace
}  // namespace ldpc5g_impl

using namespace ldpc5g_impl;

extern "C" {

int ldpc5g_prbs(const uint32_t* cinit, int32_t T, int64_t nbits, uint32_t* words, int64_t ldw,
                void* stream) {
    clear_error();
    const int64_t nw = (nbits + 31) / 32;
    if (T < 0 || nbits < 0 || (T > 1 && ldw < nw)) return fail(LDPC5G_ESIZE, "bad sizes T=%d nbits=%lld ldw=%lld", T, (long long)nbits, (long long)ldw);
    if (1600 + 32 * (nw + kPrbsWordsPerThread) >= (int64_t(1) << kPrbsPow)) return fail(LDPC5G_ESIZE, "nbits=%lld too long", (long long)nbits);
    if (T == 0 || nw == 0) return LDPC5G_OK;
    if (!cinit || !words) return fail(LDPC5G_ESIZE, "null buffer");
    const int64_t nthr = (nw + kPrbsWordsPerThread - 1) / kPrbsWordsPerThread;
    hipLaunchKernelGGL(prbs_kernel, dim3((unsigned)((nthr + 255) / 256), T), dim3(256), 0,
                       (hipStream_t)stream, cinit, nw, words, ldw);
    return check_hip(hipGetLastError(), "prbs_kernel launch");
}

int ldpc5g_scramble_modulate(const int8_t* bits, int64_t ldb, const uint32_t* prbs, int64_t ldw,
                             int32_t T, int64_t nbits, int32_t mod, void* sym, int64_t ldsym,
                             void* stream) {
    clear_error();
    if (!mod_ok(mod)) return fail(LDPC5G_ESIZE, "modulation %d (1 BPSK, -1 pi/2-BPSK, 2/4/6/8/10 QPSK..1024QAM)", mod);
    const int Qm = mod < 0 ? 1 : mod;
    if (T < 0 || nbits < 0 || nbits % Qm) return fail(LDPC5G_ESIZE, "bad sizes T=%d nbits=%lld", T, (long long)nbits);
    const int64_t nsym = nbits / Qm;
    if (T > 1 && (ldb < nbits || ldsym < nsym || (prbs && ldw < (nbits + 31) / 32))) return fail(LDPC5G_ESIZE, "bad strides");
    if (T == 0 || nsym == 0) return LDPC5G_OK;
    if (!bits || !sym) return fail(LDPC5G_ESIZE, "null buffer");
    const float scl = 1.0f / (float)sqrt((double)mod_scale(Qm));
    const dim3 grid((unsigned)((nsym + 255) / 256), T), blk(256);
    hipStream_t st = (hipStream_t)stream;
    float2* out = (float2*)sym;
#define LDPC5G_MOD(QM, PI2) \
    hipLaunchKernelGGL((scramble_modulate_kernel<QM, PI2>), grid, blk, 0, st, bits, ldb, prbs, ldw, nsym, scl, out, ldsym)
    switch (mod) {
        case -1: LDPC5G_MOD(1, true); break;
        case 1: LDPC5G_MOD(1, false); break;
        case 2: LDPC5G_MOD(2, false); break;
        case 4: LDPC5G_MOD(4, false); break;
        case 6: LDPC5G_MOD(6, false); break;
        case 8: LDPC5G_MOD(8, false); break;
        default: LDPC5G_MOD(10, false); break;
    }
#undef LDPC5G_MOD
    return check_hip(hipGetLastError(), "scramble_modulate launch");
}

int ldpc5g_demod_descramble(const void* sym, int32_t sym_dtype, int64_t ldsym, const float* noise_var,
                            int64_t ldnv, const uint32_t* prbs, int64_t ldw, int32_t T, int64_t nsym,
                            int32_t mod, void* llr, int32_t llr_dtype, int64_t ldllr, void* stream) {
    clear_error();
    if (!mod_ok(mod)) return fail(LDPC5G_ESIZE, "modulation %d (1 BPSK, -1 pi/2-BPSK, 2/4/6/8/10 QPSK..1024QAM)", mod);
    const int Qm = mod < 0 ? 1 : mod;
    if (sym_dtype != LDPC5G_F32 && sym_dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad symbol dtype %d", sym_dtype);
    if (llr_dtype != LDPC5G_F32 && !(llr_dtype == LDPC5G_F64 && mod == 1 && sym_dtype == LDPC5G_F64))
        return fail(LDPC5G_ESIZE, "float64 LLRs only for BPSK on complex128 symbols (demod_bpsk.py)");
    if (T < 0 || nsym < 0) return fail(LDPC5G_ESIZE, "bad sizes");
    if (T > 1 && (ldsym < nsym || ldnv < nsym || ldllr < nsym * Qm || (prbs && ldw < (nsym * Qm + 31) / 32)))
        return fail(LDPC5G_ESIZE, "bad strides");
    if (T == 0 || nsym == 0) return LDPC5G_OK;
    if (!sym || !noise_var || !llr) return fail(LDPC5G_ESIZE, "null buffer");
    const dim3 grid((unsigned)((nsym + 255) / 256), T), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const double A = 1.0 / sqrt((double)mod_scale(Qm));   // A = 1/math.sqrt(scale) (demod_*.py)
#define LDPC5G_DEMOD(QM, PI2, TIN, TOUT)                                                          \
    hipLaunchKernelGGL((demod_descramble_kernel<QM, PI2, TIN, TOUT>), grid, blk, 0, st,         \
                       (const TIN*)sym, ldsym, noise_var, ldnv, prbs, ldw, nsym, A, (TOUT*)llr, ldllr)
#define LDPC5G_DEMOD_ALL(TIN)                               \
    switch (mod) {                                          \
        case -1: LDPC5G_DEMOD(1, true, TIN, float); break;  \
        case 1: LDPC5G_DEMOD(1, false, TIN, float); break;  \
        case 2: LDPC5G_DEMOD(2, false, TIN, float); break;  \
        case 4: LDPC5G_DEMOD(4, false, TIN, float); break;  \
        case 6: LDPC5G_DEMOD(6, false, TIN, float); break;  \
        case 8: LDPC5G_DEMOD(8, false, TIN, float); break;  \
        default: LDPC5G_DEMOD(10, false, TIN, float); break; \
    }
    if (llr_dtype == LDPC5G_F64) LDPC5G_DEMOD(1, false, double2, double);
    else if (sym_dtype == LDPC5G_F32) { LDPC5G_DEMOD_ALL(float2) }
    else { LDPC5G_DEMOD_ALL(double2) }
#undef LDPC5G_DEMOD_ALL
#undef LDPC5G_DEMOD
    return check_hip(hipGetLastError(), "demod_descramble launch");
}

}  // extern "C"
