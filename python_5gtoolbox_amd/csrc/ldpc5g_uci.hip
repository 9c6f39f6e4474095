// ldpc5g_uci.hip — uplink control information on PUSCH, batched over T rows:
//   rate-matching arithmetic (host) ......... py5gphy/nr_pusch/nr_ulsch_info.py:6-170 (38.212 §6.3.2.4)
//   the §6.2.7 map (host, linear in Gtotal) .. py5gphy/nr_pusch/nr_pusch_datactrl_multiplex.py:7-539
//   multiplex / separate by that map ......... the same file; separation also descrambles and erases
//   placeholder-aware scrambling + mapper .... py5gphy/nr_pusch/nr_pusch_process.py:14-30
//   (32, K) small-block code ................. py5gphy/smallblock/nr_smallblock_{encoder,decoder}.py,
//                                              py5gphy/nr_pusch/nr_pusch_uci.py:22-32 (repetition to E)
// Everything on the device is a gather or a few adds per element; the small-block decoder is
// 2^(K-6) masked 32-point Hadamard transforms in the lanes of one wave per codeword.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ldpc5g_common.h"
#include "ldpc5g_demod.h"
#include "ldpc5g_mod.h"

namespace ldpc5g_impl {
namespace {

// ============================================================================ plan layout
// int32 header[kHdr], then fwd (uint32 [Gtotal]) at byte hdr[14], then inv (uint32 [ninv]) at byte
// hdr[15]; ninv = len[0] + .. + len[3], the four streams' inverse maps one after another.
// Entry bits: 0..23 index (fwd: index within the owning stream; inv: position t of g_seq),
// 24..26 stream (0 UL-SCH, 1 ACK, 2 CSI1, 3 CSI2, 4 none), 27..28 kind (0 data, 1 x, 2 y), 29 punctured
// (fwd: the position's final owner is a 1-2 bit HARQ-ACK that overwrote another stream; inv: that
// other stream's element, which still points at the position, as data_control_separate reads it).
constexpr int32_t kMagic = 0x50494355;   // "UCIP"
constexpr int32_t kVersion = 1;
constexpr int kHdr = 32;
enum { H_MAGIC, H_VERSION, H_BYTES, H_G, H_QM, H_NL, H_OACK, H_OCSI1, H_OCSI2, H_ULSCH, H_LEN0, H_LEN1, H_LEN2, H_LEN3,
       H_OFF_FWD, H_OFF_INV, H_NPUNCT, H_NINV, H_NX, H_NY };
constexpr uint32_t kIdxMask = 0xFFFFFFu;
constexpr int kStreamShift = 24, kKindShift = 27, kPunctBit = 29;
enum { S_ULSCH, S_ACK, S_CSI1, S_CSI2, S_NONE };
enum { K_DATA, K_X, K_Y };
constexpr int64_t kMaxG = int64_t(1) << 24;

// TS 38.212 Table 5.3.3.3-1: bit k of kSbRows[i] is M_{i,k}
constexpr uint16_t kSbRowsH[32] = {0x403, 0x607, 0x749, 0x50d, 0x48f, 0x5d3, 0x755, 0x599, 0x69b, 0x65d, 0x6e5,
                                   0x567, 0x7a9, 0x6ab, 0x4b1, 0x6f3, 0x277, 0x139, 0x0fb, 0x061, 0x445, 0x60b,
                                   0x591, 0x717, 0x3df, 0x4e3, 0x32d, 0x3af, 0x175, 0x1fd, 0x7ff, 0x001};
struct SbTables {
    uint16_t rows[32];
    uint8_t inv[32];   // inv[p]: the codeword position i whose columns 1..5 read p (a permutation: the code is
};                     // first-order Reed-Muller in columns 0..5, columns 6..10 are masks)
constexpr SbTables make_sb_tables() {
    SbTables t{};
    for (int i = 0; i < 32; ++i) {
        t.rows[i] = kSbRowsH[i];
        t.inv[(kSbRowsH[i] >> 1) & 31] = (uint8_t)i;
    }
    return t;
}
constexpr bool sb_is_permutation() {
    uint32_t seen = 0;
    for (int i = 0; i < 32; ++i) seen |= 1u << ((kSbRowsH[i] >> 1) & 31);
    for (int i = 0; i < 32; ++i)
        if (!(kSbRowsH[i] & 1)) return false;
    return seen == 0xFFFFFFFFu;
}
static_assert(sb_is_permutation(), "columns 1..5 must enumerate 0..31 and column 0 be all ones");
__constant__ SbTables kSb = make_sb_tables();

__host__ __device__ inline int sb_N(int K, int Qm) { return K == 1 ? Qm : K == 2 ? 3 * Qm : 32; }
// kind of position i of the K = 1 / K = 2 codeword (Tables 5.3.3.1-1, 5.3.3.2-1)
__host__ __device__ inline int sb_kind(int K, int Qm, int i) {
    if (K == 1) return i == 0 ? K_DATA : i == 1 ? K_Y : K_X;
    if (K == 2) return (i % Qm) >= 2 ? K_X : K_DATA;
    return K_DATA;
}

// ============================================================================ kernels
struct Rows4 {
    const void* p[4];
    int64_t ld[4];
};
struct RowsOut4 {
    void* p[4];
    int64_t ld[4];
    int32_t off[4];   // first entry of each stream in inv
};

// g[t] = stream[index]: one thread per position; consecutive t read consecutive stream elements
// except at the seams between resource elements of different streams.
__global__ __launch_bounds__(256) void uci_mux_kernel(const uint32_t* __restrict__ fwd, int32_t G, Rows4 in,
                                                      int8_t* __restrict__ g, int64_t ldg) {
    const int32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= G) return;
    const int64_t row = blockIdx.y;
    const uint32_t e = fwd[t];
    const int s = (e >> kStreamShift) & 7;
    int8_t v = 0;
    if (s != S_NONE) {
        const int8_t* p = (const int8_t*)(s == 0 ? in.p[0] : s == 1 ? in.p[1] : s == 2 ? in.p[2] : in.p[3]);
        const int64_t ld = s == 0 ? in.ld[0] : s == 1 ? in.ld[1] : s == 2 ? in.ld[2] : in.ld[3];
        v = p[row * ld + (e & kIdxMask)];
    }
    g[row * ldg + t] = v;
}

// One thread per OUTPUT element j of the four streams laid end to end: the writes are contiguous, the
// reads follow the map's runs (NL * Qm consecutive positions per resource element, usually many REs).
// A thread decodes its map entry once and serves kDemuxRows rows with it, their loads in flight together.
constexpr int kDemuxRows = 4;
template <typename T>
__global__ __launch_bounds__(256) void uci_demux_kernel(const uint32_t* __restrict__ inv, int32_t ninv,
                                                        const T* __restrict__ llr, int64_t ldl,
                                                        const uint32_t* __restrict__ prbs, int64_t ldw, int erase,
                                                        RowsOut4 out, int32_t nrows) {
    const int32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ninv) return;
    const int64_t row0 = (int64_t)blockIdx.y * kDemuxRows;
    const uint32_t e = inv[j];
    const int32_t t = (int32_t)(e & kIdxMask);
    const int s = (e >> kStreamShift) & 3;
    const int kind = (e >> kKindShift) & 3;
    // a y repeats the scrambled bit before it (t >= 1: it is never the first bit of its RE)
    const int32_t tc = kind == K_Y ? t - 1 : t;
    const bool zero = (prbs && kind == K_X) || (erase && ((e >> kPunctBit) & 1u));
    T* o = (T*)(s == 0 ? out.p[0] : s == 1 ? out.p[1] : s == 2 ? out.p[2] : out.p[3]);
    const int64_t ld = s == 0 ? out.ld[0] : s == 1 ? out.ld[1] : s == 2 ? out.ld[2] : out.ld[3];
    const int32_t off = s == 0 ? out.off[0] : s == 1 ? out.off[1] : s == 2 ? out.off[2] : out.off[3];
    T v[kDemuxRows];
    uint32_t c[kDemuxRows];
#pragma unroll
    for (int r = 0; r < kDemuxRows; ++r) {
        const bool on = row0 + r < nrows;
        v[r] = on ? llr[(row0 + r) * ldl + t] : (T)0;
        c[r] = on && prbs ? (prbs[(row0 + r) * ldw + (tc >> 5)] >> (tc & 31)) & 1u : 0u;
    }
#pragma unroll
    for (int r = 0; r < kDemuxRows; ++r)
        if (row0 + r < nrows) o[(row0 + r) * ld + (j - off)] = zero ? (T)0 : flip_sign(v[r], c[r]);
}

// 38.211 §6.3.1.1 with placeholders (x -> 1, y -> the scrambled bit before it), then the mapper.
template <int QM, bool PI2>
__global__ __launch_bounds__(256) void uci_scramble_modulate_kernel(const int8_t* __restrict__ bits, int64_t ldb,
                                                                    const uint32_t* __restrict__ prbs, int64_t ldw,
                                                                    int64_t nsym, float scl, float2* __restrict__ sym,
                                                                    int64_t ldsym) {
    const int64_t t = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nsym) return;
    const int8_t* b = bits + t * ldb + m * QM;
    const uint32_t* w = prbs + t * ldw;
    const uint32_t c = prbs_bits(w, m * QM, QM);
    uint32_t prev = 0;
    if (b[0] == -2 && m > 0) {   // a y that opens a symbol (QM = 1, or input no plan made): walk back over a run of y to
        const int8_t* row = bits + t * ldb;   // the bit it repeats; a run reaching the row's start repeats 0, as
        int64_t pos = m * QM - 1;             // the reference's scrambled[-1] of a zeroed array does
        while (pos > 0 && row[pos] == -2) --pos;
        const int8_t gp = row[pos];
        prev = gp == -1 ? 1u : gp == -2 ? 0u : ((uint32_t)gp ^ prbs_bits(w, pos, 1)) & 1u;
    }
    float u[QM];
#pragma unroll
    for (int i = 0; i < QM; ++i) {
        const int8_t g = b[i];
        const uint32_t s = g == -1 ? 1u : g == -2 ? prev : ((uint32_t)g ^ (c >> i)) & 1u;
        prev = s;
        u[i] = 1.0f - 2.0f * (float)s;
    }
    sym[t * ldsym + m] = mod_symbol<QM, PI2>(u, m, scl);
}

// §5.3.3 fused with the repetition to E: one thread per output bit.
__global__ __launch_bounds__(256) void sb_encode_kernel(const int8_t* __restrict__ bits, int64_t ldb, int K, int Qm,
                                                        int8_t* __restrict__ out, int64_t ldo, int32_t E) {
    const int32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t row = blockIdx.y;
    const int8_t* b = bits + row * ldb;
    const int N = sb_N(K, Qm);
    const int i = e % N;
    int8_t v;
    if (K >= 3) {
        uint32_t msg = 0;
        for (int k = 0; k < K; ++k) msg |= ((uint32_t)b[k] & 1u) << k;
        v = (int8_t)(__popc(msg & kSb.rows[i]) & 1);
    } else {
        const int kind = sb_kind(K, Qm, i);
        if (kind == K_X) v = -1;
        else if (kind == K_Y) v = -2;
        else if (K == 1) v = b[0] & 1;
        else {
            const int nd = Qm < 2 ? Qm : 2;
            const int c = (nd * (i / Qm) + i % Qm) % 3;   // c0 c1 c2 c0 c1 c2 over the data positions
            v = c == 0 ? (b[0] & 1) : c == 1 ? (b[1] & 1) : ((b[0] ^ b[1]) & 1);
        }
    }
    out[row * ldo + e] = v;
}

// Soft rate recovery + maximum-likelihood decision, one wave per codeword, no LDS.
// K >= 3: lane (h, p), p = lane & 31, holds the folded LLR of the position whose columns 1..5 read p.
// For mask combination u (message bits 6..K-1) the lanes flip the masked positions and run a 32-point
// Hadamard transform with five lane exchanges: lane p then holds H[a = p] = sum_i (-1)^(<a, idx_i> + mask_i) f_i,
// the metric of (c0 = 0, a, u); c0 = 1 negates it.  The two halves of the wave take two u at a time.
template <typename T>
__global__ __launch_bounds__(256) void sb_decode_kernel(const T* __restrict__ llr, int64_t ldl, int32_t E, int K, int Qm,
                                                        int8_t* __restrict__ out, int64_t ldo, int32_t B) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;   // wave-uniform
    const T* x = llr + row * ldl;
    int8_t* o = out + row * ldo;
    if (K <= 2) {
        const int N = sb_N(K, Qm);
        double f = 0.0;
        if (lane < N)
            for (int32_t e = lane; e < E; e += N) f += (double)x[e];
        if (K == 1) {
            double s = __shfl(f, 0);
            if (Qm >= 2) s += __shfl(f, 1);
            if (lane == 0) o[0] = s < 0.0 ? 1 : 0;
            return;
        }
        const int nd = Qm < 2 ? Qm : 2;
        double S[3] = {0.0, 0.0, 0.0};
        for (int g = 0; g < 3; ++g)
            for (int j = 0; j < nd; ++j) {
                const double v = __shfl(f, g * Qm + j);
                const int c = (nd * g + j) % 3;
                S[0] += c == 0 ? v : 0.0, S[1] += c == 1 ? v : 0.0, S[2] += c == 2 ? v : 0.0;
            }
        int bm = 0;
        double best = S[0] + S[1] + S[2];
        for (int m = 1; m < 4; ++m) {
            const int c0 = m >> 1, c1 = m & 1;
            const double met = (c0 ? -S[0] : S[0]) + (c1 ? -S[1] : S[1]) + ((c0 ^ c1) ? -S[2] : S[2]);
            if (met > best) best = met, bm = m;
        }
        if (lane < 2) o[lane] = (int8_t)((bm >> (1 - lane)) & 1);
        return;
    }
    const int p = lane & 31, h = lane >> 5;
    const int i = kSb.inv[p];
    double f = 0.0;
    for (int32_t e = i; e < E; e += 32) f += (double)x[e];
    const uint32_t maskbits = (uint32_t)kSb.rows[i] >> 6;
    const int nmask = K > 6 ? 1 << (K - 6) : 1;
    const bool a_ok = K >= 6 || p < (1 << (K - 1));
    uint32_t ma = 0;   // the message bits 1..5 of a = p, in place (bit k of the message at K - 1 - k)
    for (int j = 0; j < 5 && j < K - 1; ++j) ma |= (uint32_t)((p >> j) & 1) << (K - 2 - j);
    double best = -INFINITY;
    uint32_t bestm = 0xFFFFFFFFu;
    for (int u0 = 0; u0 < nmask; u0 += 2) {
        const int u = u0 + h;
        double w = (__popc((uint32_t)u & maskbits) & 1) ? -f : f;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const double ow = __shfl_xor(w, 1 << s);
            w = ((p >> s) & 1) ? ow - w : w + ow;
        }
        uint32_t m = ma | (w < 0.0 ? 1u << (K - 1) : 0u);
        for (int j = 0; j < K - 6; ++j) m |= (uint32_t)((u >> j) & 1) << (K - 7 - j);
        const double met = fabs(w);
        if (a_ok && u < nmask && (met > best || (met == best && m < bestm))) best = met, bestm = m;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const uint32_t om = (uint32_t)__shfl_xor((int)bestm, off);
        if (ob > best || (ob == best && om < bestm)) best = ob, bestm = om;
    }
    if (lane < K) o[lane] = (int8_t)((bestm >> (K - 1 - lane)) & 1u);
}

// ============================================================================ host: §6.3.2.4
const double kBetaAck[16] = {1.000, 2.000, 2.500, 3.125, 4.000, 5.000, 6.250, 8.000,
                             10.000, 12.625, 15.875, 20.000, 31.000, 50.000, 80.000, 126.000};   // 38.213 Table 9.3-1
const double kBetaCsi[19] = {1.125, 1.250, 1.375, 1.625, 1.750, 2.000, 2.250, 2.500, 2.875, 3.125,
                             3.500, 4.000, 5.000, 6.250, 8.000, 10.000, 12.625, 15.875, 20.000};   // Table 9.3-2
int plus_L(int n) { return n <= 11 ? n : n >= 360 ? n + 11 : n <= 19 ? n + 6 : n + 11; }
int64_t min_capacity(int A) {
    if (A <= 11) return A;
    if (A <= 19) return A + 6 + 3;
    return A < 1013 ? A + 11 : A + (A % 2) + 22;
}

// the allocation arguments that ldpc5g_uci_rm_info and ldpc5g_uci_map_plan share; 0 or the failure code
int check_alloc(int32_t RBSize, int32_t StartSymbolIndex, int32_t NrOfSymbols, const int32_t* dmrs_symlist, int32_t num_dmrs,
                int32_t NL, int32_t Qm) {
    if (!dmrs_symlist) return fail(LDPC5G_ESIZE, "null dmrs_symlist");
    if (RBSize < 1 || RBSize > 275 || NrOfSymbols < 1 || NrOfSymbols > 14 || StartSymbolIndex < 0 ||
        StartSymbolIndex + NrOfSymbols > 14 || num_dmrs < 1 || num_dmrs > 14)
        return fail(LDPC5G_ESIZE, "bad allocation RBSize=%d StartSymbolIndex=%d NrOfSymbols=%d num_dmrs=%d", RBSize,
                    StartSymbolIndex, NrOfSymbols, num_dmrs);
    for (int i = 0; i < num_dmrs; ++i)
        if (dmrs_symlist[i] < 0 || dmrs_symlist[i] > 13)
            return fail(LDPC5G_ESIZE, "bad allocation: dmrs_symlist[%d]=%d outside 0..13", i, dmrs_symlist[i]);
    if (NL < 1 || NL > 4 || !(Qm == 1 || Qm == 2 || Qm == 4 || Qm == 6 || Qm == 8)) return fail(LDPC5G_ESIZE, "bad NL=%d or Qm=%d", NL, Qm);
    return 0;
}

bool plan_ok(const void* plan_host, const int32_t** hdr) {
    if (!plan_host) return fail(LDPC5G_ESIZE, "plan_host is null"), false;
    const int32_t* h = (const int32_t*)plan_host;
    if (h[H_MAGIC] != kMagic) return fail(LDPC5G_ESIZE, "not a UCI map plan (magic)"), false;
    if (h[H_VERSION] != kVersion) return fail(LDPC5G_ESIZE, "UCI map plan version %d, expected %d", h[H_VERSION], kVersion), false;
    const int64_t G = h[H_G];
    int64_t ninv = 0;
    bool ok = G >= 1 && G < kMaxG;
    for (int s = 0; s < 4; ++s) ok = ok && h[H_LEN0 + s] >= 0 && h[H_LEN0 + s] <= G, ninv += h[H_LEN0 + s];
    ok = ok && ninv == h[H_NINV] && ninv <= 2 * G && h[H_OFF_FWD] == kHdr * 4 && h[H_OFF_INV] == h[H_OFF_FWD] + 4 * G &&
         h[H_BYTES] == h[H_OFF_INV] + 4 * ninv;
    if (!ok) return fail(LDPC5G_ESIZE, "UCI map plan header out of range"), false;
    *hdr = h;
    return true;
}

}  // namespace
}  // namespace ldpc5g_impl

using namespace ldpc5g_impl;

extern "C" {

int ldpc5g_uci_rm_info(int32_t RBSize, int32_t StartSymbolIndex, int32_t NrOfSymbols, const int32_t* dmrs_symlist,
                       int32_t num_dmrs, int32_t NL, int32_t Qm, double coderateby1024, int64_t ULSCH_size,
                       int32_t EnableULSCH, int32_t OACK, int32_t OCSI1, int32_t OCSI2, int32_t I_HARQ_ACK_offset,
                       int32_t I_CSI1offset, int32_t I_CSI2offset, double UCIScaling, int64_t Gtotal, int64_t* out) {
    clear_error();
    if (!out) return fail(LDPC5G_ESIZE, "null out");
    if (int rc = check_alloc(RBSize, StartSymbolIndex, NrOfSymbols, dmrs_symlist, num_dmrs, NL, Qm)) return rc;
    if (OACK < 0 || OCSI1 < 0 || OCSI2 < 0 || OACK > 1706 || OCSI1 > 1706 || OCSI2 > 1706)
        return fail(LDPC5G_ESIZE, "payload sizes OACK=%d OCSI1=%d OCSI2=%d outside 0..1706", OACK, OCSI1, OCSI2);
    if (EnableULSCH != 0 && EnableULSCH != 1) return fail(LDPC5G_ESIZE, "EnableULSCH=%d", EnableULSCH);
    if (Gtotal < 0 || ULSCH_size < 0 || !(UCIScaling > 0.0 && UCIScaling <= 1.0) || !(coderateby1024 > 0.0))
        return fail(LDPC5G_ESIZE, "bad Gtotal, ULSCH_size, UCIScaling or coderate");
    // the reference reads the HARQ-ACK table for every OACK (the reserved set of OACK <= 2 included)
    if (I_HARQ_ACK_offset < 0 || I_HARQ_ACK_offset > 15) return fail(LDPC5G_ESIZE, "I_HARQ_ACK_offset=%d outside the table (0..15)", I_HARQ_ACK_offset);
    if (OCSI1 > 0 && (I_CSI1offset < 0 || I_CSI1offset > 18)) return fail(LDPC5G_ESIZE, "I_CSI1offset=%d outside the table (0..18)", I_CSI1offset);
    if (OCSI2 > 0 && (I_CSI2offset < 0 || I_CSI2offset > 18)) return fail(LDPC5G_ESIZE, "I_CSI2offset=%d outside the table (0..18)", I_CSI2offset);
    if (EnableULSCH && ULSCH_size == 0) return fail(LDPC5G_ESIZE, "ULSCH_size=0 with EnableULSCH=1");
    const double total = (double)((int64_t)(NrOfSymbols - num_dmrs) * RBSize * 12);
    const int till_L0 = dmrs_symlist[0] + 1 - StartSymbolIndex - 1;
    const double from_L0 = (double)((int64_t)(NrOfSymbols - num_dmrs - till_L0) * RBSize * 12);
    const double usz = (double)ULSCH_size;
    const double rate = (double)Qm * coderateby1024 / 1024.0;
    // ceil(NumbitsPlusL * beta * TotalMUCI / ULSCH_size) in the reference's order, double arithmetic
    auto q_ack = [&](int O) -> int64_t {
        const double n = (double)plus_L(O), beta = kBetaAck[I_HARQ_ACK_offset];
        const double cap = ceil(UCIScaling * from_L0);
        const double d1 = EnableULSCH ? ceil(n * beta * total / usz) : ceil(n * beta / rate);
        return (int64_t)(d1 < cap ? d1 : cap);
    };
    const int64_t Qack = OACK == 0 ? 0 : q_ack(OACK);
    const int64_t Qrvd = OACK <= 2 ? q_ack(2) : 0;
    const int64_t q = (int64_t)NL * Qm;
    int64_t Qcsi1 = 0, Qcsi2 = 0;
    const int64_t itotal = (int64_t)total;
    if (OCSI1 > 0) {
        const double n = (double)plus_L(OCSI1), beta = kBetaCsi[I_CSI1offset];
        const int64_t qa = OACK > 2 ? Qack : Qrvd;
        if (EnableULSCH) {
            const int64_t d1 = (int64_t)ceil(n * beta * total / usz), cap = (int64_t)ceil(UCIScaling * total) - qa;
            Qcsi1 = d1 < cap ? d1 : cap;
        } else if (OCSI2 > 0) {
            const int64_t d1 = (int64_t)ceil(n * beta / rate), cap = itotal - qa;
            Qcsi1 = d1 < cap ? d1 : cap;
        } else {
            Qcsi1 = itotal - qa;
        }
    }
    if (OCSI2 > 0) {
        const double n = (double)plus_L(OCSI2), beta = kBetaCsi[I_CSI2offset];
        const int64_t qa = OACK > 2 ? Qack : 0;
        if (EnableULSCH) {
            const int64_t d1 = (int64_t)ceil(n * beta * total / usz), cap = (int64_t)ceil(UCIScaling * total) - qa - Qcsi1;
            Qcsi2 = d1 < cap ? d1 : cap;
        } else {
            Qcsi2 = itotal - qa - Qcsi1;
        }
    }
    const int64_t Eack = q * Qack, Ercd = q * Qrvd, E1 = q * Qcsi1, E2 = q * Qcsi2;
    if (Gtotal < E1 + E2) return fail(LDPC5G_ESIZE, "Gtotal=%lld < Euci_CSI1 + Euci_CSI2 = %lld", (long long)Gtotal, (long long)(E1 + E2));
    if (E1 > 8192 || E2 > 8192 || Eack > 8192) return fail(LDPC5G_ESIZE, "E > 8192 (Euci_ack=%lld Euci_CSI1=%lld Euci_CSI2=%lld)", (long long)Eack, (long long)E1, (long long)E2);
    if (Eack < min_capacity(OACK) || E1 < min_capacity(OCSI1) || E2 < min_capacity(OCSI2))
        return fail(LDPC5G_ESIZE, "E below the minimum capacity (Euci_ack=%lld Euci_CSI1=%lld Euci_CSI2=%lld)", (long long)Eack, (long long)E1, (long long)E2);
    out[0] = Eack, out[1] = Qack, out[2] = E1, out[3] = Qcsi1, out[4] = E2, out[5] = Qcsi2, out[6] = Ercd, out[7] = Qrvd;
    out[8] = !EnableULSCH ? 0 : OACK > 2 ? Gtotal - E1 - E2 - Eack : Gtotal - E1 - E2;
    return LDPC5G_OK;
}

int64_t ldpc5g_uci_map_plan(int32_t RBSize, int32_t StartSymbolIndex, int32_t NrOfSymbols, const int32_t* dmrs_symlist,
                            int32_t num_dmrs, int32_t NumCDMGroupsWithoutData, int32_t NL, int32_t Qm, int32_t OACK,
                            int32_t OCSI1, int32_t OCSI2, int32_t EnableULSCH, int32_t frequency_hopping, int64_t Euci_ack,
                            int64_t Euci_CSI1, int64_t Euci_CSI2, int64_t Euci_ackrvd, int64_t G_ULSCH, int64_t Gtotal,
                            void* plan, int64_t plan_bytes) {
    clear_error();
    if (frequency_hopping) return fail(LDPC5G_ESIZE, "frequency hopping is not provided");
    if (int rc = check_alloc(RBSize, StartSymbolIndex, NrOfSymbols, dmrs_symlist, num_dmrs, NL, Qm)) return rc;
    if (NumCDMGroupsWithoutData != 1 && NumCDMGroupsWithoutData != 2) return fail(LDPC5G_ESIZE, "NumCDMGroupsWithoutData=%d (1 or 2)", NumCDMGroupsWithoutData);
    if (OACK < 0 || OCSI1 < 0 || OCSI2 < 0 || (EnableULSCH != 0 && EnableULSCH != 1)) return fail(LDPC5G_ESIZE, "bad payload sizes or EnableULSCH");
    const int q = NL * Qm, M = RBSize * 12, nsym = NrOfSymbols;
    for (int64_t e : {Euci_ack, Euci_CSI1, Euci_CSI2, Euci_ackrvd, G_ULSCH})
        if (e < 0 || e > Gtotal || e % q) return fail(LDPC5G_ESIZE, "stream length %lld: not a multiple of NL * Qm in 0..Gtotal", (long long)e);
    uint32_t is_dmrs = 0;
    for (int i = 0; i < num_dmrs; ++i) is_dmrs |= 1u << dmrs_symlist[i];
    int mul[14], muci[14];
    int64_t nre = 0;
    for (int L = 0; L < nsym; ++L) {
        const bool d = (is_dmrs >> (StartSymbolIndex + L)) & 1u;
        mul[L] = d ? (NumCDMGroupsWithoutData == 1 ? RBSize * 6 : 0) : M;
        muci[L] = d ? 0 : M;
        nre += mul[L];
    }
    if (Gtotal != nre * q) return fail(LDPC5G_ESIZE, "Gtotal=%lld is not the allocation's %lld bits", (long long)Gtotal, (long long)(nre * q));
    if (Gtotal < 1 || Gtotal >= kMaxG) return fail(LDPC5G_ESIZE, "Gtotal=%lld outside 1..2^24-1", (long long)Gtotal);
    const int64_t len_in[4] = {EnableULSCH ? G_ULSCH : 0, OACK ? Euci_ack : 0, OCSI1 ? Euci_CSI1 : 0, OCSI2 ? Euci_CSI2 : 0};
    const int64_t ninv = len_in[0] + len_in[1] + len_in[2] + len_in[3];
    if (ninv > 2 * Gtotal) return fail(LDPC5G_ESIZE, "streams longer than the allocation");
    const int64_t bytes = kHdr * 4 + 4 * Gtotal + 4 * ninv;
    if (!plan) return bytes;
    if (plan_bytes < bytes) return fail(LDPC5G_ESIZE, "plan_bytes=%lld < %lld", (long long)plan_bytes, (long long)bytes);

    // flags per resource element: linear in Gtotal (the reference scans lists, quadratic per symbol)
    const size_t R = (size_t)nsym * M;
    std::vector<uint8_t> uci_av(R, 0), ul_av(R, 0), rvd(R, 0), owner(R, S_NONE);
    std::vector<uint8_t> over_s(R, S_NONE);   // the stream a 1-2 bit HARQ-ACK overwrites (step 5), and its index
    std::vector<int32_t> first(R, 0), over_first(R, 0), cand((size_t)M);
    int n_uci[14], n_ul[14], n_rvd[14] = {0};
    for (int L = 0; L < nsym; ++L) {
        for (int k = 0; k < muci[L]; ++k) uci_av[(size_t)L * M + k] = 1;
        for (int k = 0; k < mul[L]; ++k) ul_av[(size_t)L * M + k] = 1;
        n_uci[L] = muci[L], n_ul[L] = mul[L];
    }
    const int L1 = dmrs_symlist[0] + 1;   // used as an index relative to the allocation, as the reference does
    const int Lcsi = ((is_dmrs >> StartSymbolIndex) & 1u) ? StartSymbolIndex + 1 : StartSymbolIndex;
    const char* err = nullptr;
    enum { STEP1, STEP2, STEP_CSI1, STEP_CSI2, STEP5 };
    // one of the reference's five "while count < G" loops
    auto spread = [&](int step, int64_t G, int L) {
        int64_t n = 0;
        const int s = step == STEP2 || step == STEP5 ? S_ACK : step == STEP_CSI1 ? S_CSI1 : S_CSI2;
        while (n < G && !err) {
            if (L >= nsym) { err = "the UCI does not fit the allocation's symbols"; return; }
            uint8_t* ua = &uci_av[(size_t)L * M];
            uint8_t* la = &ul_av[(size_t)L * M];
            uint8_t* rv = &rvd[(size_t)L * M];
            const int64_t c = step == STEP_CSI1 ? n_uci[L] - n_rvd[L] : step == STEP5 ? n_rvd[L] : n_uci[L];
            if (c > 0) {
                int64_t d = 1, m;
                if (G - n >= c * q) m = step == STEP1 || step == STEP2 ? n_ul[L] : c;
                else d = (c * q) / (G - n), m = (G - n + q - 1) / q;
                int nc = 0;
                for (int k = 0; k < M; ++k) {
                    const bool in = step == STEP1 ? la[k] : step == STEP_CSI1 ? (ua[k] && !rv[k]) : step == STEP5 ? rv[k] : ua[k];
                    if (in) cand[nc++] = k;
                }
                if (m > 0 && (m - 1) * d >= nc) { err = "the UCI does not fit a symbol's resource elements"; return; }
                for (int64_t j = 0; j < m; ++j) {
                    const size_t r = (size_t)L * M + cand[(size_t)(j * d)];
                    if (step == STEP1) {
                        rvd[r] = 1;
                        continue;
                    }
                    if (step == STEP5) {
                        over_s[r] = owner[r], over_first[r] = first[r];
                    } else {
                        n_uci[L] -= uci_av[r], n_ul[L] -= ul_av[r];
                        uci_av[r] = 0, ul_av[r] = 0;
                    }
                    owner[r] = (uint8_t)s;
                    first[r] = (int32_t)(n + j * q);
                }
                if (step == STEP1)
                    for (int k = 0, z = 0; k < M; ++k) z += rv[k], n_rvd[L] = z;
                n += m * q;
            }
            ++L;
        }
    };
    if (OACK <= 2) spread(STEP1, Euci_ackrvd, L1);
    if (!err && OACK > 2) spread(STEP2, Euci_ack, L1);
    if (!err && OCSI1 > 0) {
        int L = Lcsi;
        while (L < nsym && n_uci[L] - n_rvd[L] <= 0) ++L;
        spread(STEP_CSI1, Euci_CSI1, L);
    }
    if (!err && OCSI2 > 0) {
        int L = Lcsi;
        while (L < nsym && n_uci[L] <= 0) ++L;
        spread(STEP_CSI2, Euci_CSI2, L);
    }
    if (err) return fail(LDPC5G_ESIZE, "%s", err);
    int64_t nul = 0;
    if (EnableULSCH)
        for (int L = 0; L < nsym; ++L)
            for (int k = 0; k < M; ++k) {
                const size_t r = (size_t)L * M + k;
                if (ul_av[r]) owner[r] = S_ULSCH, first[r] = (int32_t)nul, nul += q;
            }
    if (EnableULSCH && nul != G_ULSCH) return fail(LDPC5G_ESIZE, "G_ULSCH=%lld, the map leaves %lld bits to the UL-SCH", (long long)G_ULSCH, (long long)nul);
    if (OACK == 1 || OACK == 2) spread(STEP5, Euci_ack, L1);
    if (err) return fail(LDPC5G_ESIZE, "%s", err);

    int32_t* h = (int32_t*)plan;
    memset(h, 0, kHdr * 4);
    uint32_t* fwd = (uint32_t*)((char*)plan + kHdr * 4);
    uint32_t* inv = fwd + Gtotal;
    int64_t off[4] = {0, len_in[0], len_in[0] + len_in[1], len_in[0] + len_in[1] + len_in[2]};
    for (int64_t j = 0; j < ninv; ++j) inv[j] = 0xFFFFFFFFu;
    int64_t t = 0, npunct = 0, nx = 0, ny = 0;
    const int NA = sb_N(OACK, Qm);
    for (int L = 0; L < nsym; ++L)
        for (int k = 0; k < mul[L]; ++k) {
            const size_t r = (size_t)L * M + k;
            const int s = owner[r];
            for (int v = 0; v < q; ++v, ++t) {
                if (s == S_NONE) {
                    fwd[t] = (uint32_t)S_NONE << kStreamShift;
                    continue;
                }
                const int64_t ix = (int64_t)first[r] + v;
                if (ix >= len_in[s]) return fail(LDPC5G_ESIZE, "stream %d: index %lld beyond its length %lld", s, (long long)ix, (long long)len_in[s]);
                const int kind = s == S_ACK && OACK <= 2 ? sb_kind(OACK, Qm, (int)(ix % NA)) : K_DATA;
                nx += kind == K_X, ny += kind == K_Y;
                if (kind == K_Y && v == 0) return fail(LDPC5G_ESIZE, "a y placeholder opens a resource element");
                const uint32_t fl = ((uint32_t)s << kStreamShift) | ((uint32_t)kind << kKindShift);
                fwd[t] = (uint32_t)ix | fl;
                inv[off[s] + ix] = (uint32_t)t | fl;
                if (over_s[r] != S_NONE) {   // a 1-2 bit HARQ-ACK overwrites this UL-SCH (or CSI part 2) bit
                    fwd[t] |= 1u << kPunctBit;
                    inv[off[over_s[r]] + over_first[r] + v] = (uint32_t)t | ((uint32_t)over_s[r] << kStreamShift) | (1u << kPunctBit);
                    ++npunct;
                }
            }
        }
    for (int64_t j = 0; j < ninv; ++j)
        if (inv[j] == 0xFFFFFFFFu) return fail(LDPC5G_ESIZE, "the map leaves stream elements without a position (lengths do not match the allocation)");
    h[H_MAGIC] = kMagic, h[H_VERSION] = kVersion, h[H_BYTES] = (int32_t)bytes, h[H_G] = (int32_t)Gtotal, h[H_QM] = Qm, h[H_NL] = NL;
    h[H_OACK] = OACK, h[H_OCSI1] = OCSI1, h[H_OCSI2] = OCSI2, h[H_ULSCH] = EnableULSCH;
    for (int s = 0; s < 4; ++s) h[H_LEN0 + s] = (int32_t)len_in[s];
    h[H_OFF_FWD] = kHdr * 4, h[H_OFF_INV] = (int32_t)(kHdr * 4 + 4 * Gtotal), h[H_NPUNCT] = (int32_t)npunct, h[H_NINV] = (int32_t)ninv;
    h[H_NX] = (int32_t)nx, h[H_NY] = (int32_t)ny;
    return bytes;
}

int ldpc5g_uci_mux(const void* plan_dev, const void* plan_host, const int8_t* g_ulsch, int64_t ld_ulsch, const int8_t* g_ack,
                   int64_t ld_ack, const int8_t* g_csi1, int64_t ld_csi1, const int8_t* g_csi2, int64_t ld_csi2, int8_t* g_seq,
                   int64_t ldg, int32_t T, void* stream) {
    clear_error();
    const int32_t* h;
    if (!plan_ok(plan_host, &h)) return LDPC5G_ESIZE;
    if (!plan_dev) return fail(LDPC5G_ESIZE, "plan_dev is null");
    if (T < 1 || T > 65535) return fail(LDPC5G_ESIZE, "T=%d outside 1..65535", T);
    if (!g_seq) return fail(LDPC5G_ESIZE, "g_seq is null");
    if (ldg < h[H_G]) return fail(LDPC5G_ESIZE, "ldg=%lld < Gtotal=%d", (long long)ldg, h[H_G]);
    Rows4 in{{g_ulsch, g_ack, g_csi1, g_csi2}, {ld_ulsch, ld_ack, ld_csi1, ld_csi2}};
    static const char* names[4] = {"g_ulsch", "g_ack", "g_csi1", "g_csi2"};
    for (int s = 0; s < 4; ++s) {
        if (h[H_LEN0 + s] == 0) continue;
        if (!in.p[s]) return fail(LDPC5G_ESIZE, "%s is null", names[s]);
        if (in.ld[s] < h[H_LEN0 + s]) return fail(LDPC5G_ESIZE, "stride of %s: %lld < %d", names[s], (long long)in.ld[s], h[H_LEN0 + s]);
    }
    const uint32_t* fwd = (const uint32_t*)((const char*)plan_dev + h[H_OFF_FWD]);
    hipLaunchKernelGGL(uci_mux_kernel, dim3((unsigned)((h[H_G] + 255) / 256), T), dim3(256), 0, (hipStream_t)stream, fwd,
                       h[H_G], in, g_seq, ldg);
    return check_hip(hipGetLastError(), "uci_mux launch");
}

int ldpc5g_uci_demux(const void* plan_dev, const void* plan_host, const void* llr, int32_t dtype, int64_t ldl,
                     const uint32_t* prbs, int64_t ldw, int32_t erase_punctured, void* g_ulsch, int64_t ld_ulsch, void* g_ack,
                     int64_t ld_ack, void* g_csi1, int64_t ld_csi1, void* g_csi2, int64_t ld_csi2, int32_t T, void* stream) {
    clear_error();
    const int32_t* h;
    if (!plan_ok(plan_host, &h)) return LDPC5G_ESIZE;
    if (!plan_dev) return fail(LDPC5G_ESIZE, "plan_dev is null");
    if (dtype != LDPC5G_F32 && dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad LLR dtype %d", dtype);
    if (T < 1 || T > 65535) return fail(LDPC5G_ESIZE, "T=%d outside 1..65535", T);
    if (!llr) return fail(LDPC5G_ESIZE, "llr is null");
    if (ldl < h[H_G]) return fail(LDPC5G_ESIZE, "ldl=%lld < Gtotal=%d", (long long)ldl, h[H_G]);
    if (prbs && ldw < (h[H_G] + 31) / 32) return fail(LDPC5G_ESIZE, "ldw=%lld < %d words", (long long)ldw, (h[H_G] + 31) / 32);
    if (erase_punctured != 0 && erase_punctured != 1) return fail(LDPC5G_ESIZE, "erase_punctured=%d", erase_punctured);
    RowsOut4 out{{g_ulsch, g_ack, g_csi1, g_csi2}, {ld_ulsch, ld_ack, ld_csi1, ld_csi2}, {0, 0, 0, 0}};
    static const char* names[4] = {"g_ulsch", "g_ack", "g_csi1", "g_csi2"};
    int32_t off = 0;
    for (int s = 0; s < 4; ++s) {
        out.off[s] = off;
        off += h[H_LEN0 + s];
        if (h[H_LEN0 + s] == 0) continue;
        if (!out.p[s]) return fail(LDPC5G_ESIZE, "%s is null", names[s]);
        if (out.ld[s] < h[H_LEN0 + s]) return fail(LDPC5G_ESIZE, "stride of %s: %lld < %d", names[s], (long long)out.ld[s], h[H_LEN0 + s]);
    }
    const int32_t ninv = h[H_NINV];
    if (ninv == 0) return LDPC5G_OK;
    const uint32_t* inv = (const uint32_t*)((const char*)plan_dev + h[H_OFF_INV]);
    const dim3 grid((unsigned)((ninv + 255) / 256), (unsigned)((T + kDemuxRows - 1) / kDemuxRows)), blk(256);
    if (dtype == LDPC5G_F32)
        hipLaunchKernelGGL(uci_demux_kernel<float>, grid, blk, 0, (hipStream_t)stream, inv, ninv, (const float*)llr, ldl, prbs, ldw,
                           erase_punctured, out, T);
    else
        hipLaunchKernelGGL(uci_demux_kernel<double>, grid, blk, 0, (hipStream_t)stream, inv, ninv, (const double*)llr, ldl, prbs,
                           ldw, erase_punctured, out, T);
    return check_hip(hipGetLastError(), "uci_demux launch");
}

int ldpc5g_uci_scramble_modulate(const int8_t* bits, int64_t ldb, const uint32_t* prbs, int64_t ldw, int32_t T, int64_t nbits,
                                 int32_t mod, void* sym, int64_t ldsym, void* stream) {
    clear_error();
    if (!(mod == -1 || mod == 1 || mod == 2 || mod == 4 || mod == 6 || mod == 8))
        return fail(LDPC5G_ESIZE, "modulation %d (1 BPSK, -1 pi/2-BPSK, 2/4/6/8: the orders §5.3.3 defines placeholders for)", mod);
    const int Qm = mod < 0 ? 1 : mod;
    if (T < 1 || T > 65535 || nbits < 1 || nbits >= kMaxG * 4 || nbits % Qm) return fail(LDPC5G_ESIZE, "bad sizes T=%d nbits=%lld", T, (long long)nbits);
    const int64_t nsym = nbits / Qm;
    if (!bits || !sym || !prbs) return fail(LDPC5G_ESIZE, "null buffer");
    if (ldb < nbits) return fail(LDPC5G_ESIZE, "ldb=%lld < nbits", (long long)ldb);
    if (ldsym < nsym) return fail(LDPC5G_ESIZE, "ldsym=%lld < the symbols of a row", (long long)ldsym);
    if (ldw < (nbits + 31) / 32) return fail(LDPC5G_ESIZE, "ldw=%lld < the words of a row", (long long)ldw);
    const float scl = 1.0f / (float)sqrt((double)mod_scale(Qm));
    const dim3 grid((unsigned)((nsym + 255) / 256), T), blk(256);
    hipStream_t st = (hipStream_t)stream;
    float2* out = (float2*)sym;
#define LDPC5G_UMOD(QM, PI2) \
    hipLaunchKernelGGL((uci_scramble_modulate_kernel<QM, PI2>), grid, blk, 0, st, bits, ldb, prbs, ldw, nsym, scl, out, ldsym)
    switch (mod) {
        case -1: LDPC5G_UMOD(1, true); break;
        case 1: LDPC5G_UMOD(1, false); break;
        case 2: LDPC5G_UMOD(2, false); break;
        case 4: LDPC5G_UMOD(4, false); break;
        case 6: LDPC5G_UMOD(6, false); break;
        default: LDPC5G_UMOD(8, false); break;
    }
#undef LDPC5G_UMOD
    return check_hip(hipGetLastError(), "uci_scramble_modulate launch");
}

static int sb_args(int32_t K, int32_t Qm, int64_t E, int32_t T) {
    if (K < 1 || K > 11) return fail(LDPC5G_ESIZE, "K=%d outside 1..11", K);
    if (!(Qm == 1 || Qm == 2 || Qm == 4 || Qm == 6 || Qm == 8)) return fail(LDPC5G_ESIZE, "Qm=%d", Qm);
    if (E < 1 || E > 8192) return fail(LDPC5G_ESIZE, "E=%lld outside 1..8192", (long long)E);
    if (T < 1 || T > (1 << 22)) return fail(LDPC5G_ESIZE, "T=%d outside 1..2^22", T);
    return 0;
}

int ldpc5g_smallblock_encode(const int8_t* bits, int64_t ldb, int32_t K, int32_t Qm, int8_t* out, int64_t ldo, int32_t E,
                             int32_t T, void* stream) {
    clear_error();
    if (int rc = sb_args(K, Qm, E, T)) return rc;
    if (T > 65535) return fail(LDPC5G_ESIZE, "T=%d outside 1..65535", T);
    if (!bits || !out) return fail(LDPC5G_ESIZE, "null buffer");
    if (ldb < K) return fail(LDPC5G_ESIZE, "ldb=%lld < K", (long long)ldb);
    if (ldo < E) return fail(LDPC5G_ESIZE, "ldo=%lld < E", (long long)ldo);
    hipLaunchKernelGGL(sb_encode_kernel, dim3((unsigned)((E + 255) / 256), T), dim3(256), 0, (hipStream_t)stream, bits, ldb, K, Qm,
                       out, ldo, E);
    return check_hip(hipGetLastError(), "smallblock_encode launch");
}

int ldpc5g_smallblock_decode(const void* llr, int32_t dtype, int64_t ldl, int32_t E, int32_t K, int32_t Qm, int8_t* out,
                             int64_t ldo, int32_t T, void* stream) {
    clear_error();
    if (int rc = sb_args(K, Qm, E, T)) return rc;
    if (dtype != LDPC5G_F32 && dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad LLR dtype %d", dtype);
    if (!llr || !out) return fail(LDPC5G_ESIZE, "null buffer");
    if (ldl < E) return fail(LDPC5G_ESIZE, "ldl=%lld < E", (long long)ldl);
    if (ldo < K) return fail(LDPC5G_ESIZE, "ldo=%lld < K", (long long)ldo);
    const dim3 grid((unsigned)((T + 3) / 4)), blk(256);
    if (dtype == LDPC5G_F32)
        hipLaunchKernelGGL(sb_decode_kernel<float>, grid, blk, 0, (hipStream_t)stream, (const float*)llr, ldl, E, K, Qm, out, ldo, T);
    else
        hipLaunchKernelGGL(sb_decode_kernel<double>, grid, blk, 0, (hipStream_t)stream, (const double*)llr, ldl, E, K, Qm, out, ldo, T);
    return check_hip(hipGetLastError(), "smallblock_decode launch");
}

}  // extern "C"
