// ldpc5g_slot.hip — the slot front end: the frequency-domain resource grid on one side, the
// channel estimator's H_LS and the equaliser's interleaved y on the other, batched over slots:
//   DMRS least-squares estimate ........ py5gphy/nr_pdsch/nr_pdsch_dmrs.py:139-227 (pdsch_dmrs_LS_est),
//                                        py5gphy/nr_pusch/nr_pusch_dmrs.py:107-200 (pusch_dmrs_LS_est)
//   DMRS sequence r(n) ................. nr_pdsch_dmrs.py:244-256 (_gen_seq), nrPRBS.py:5-25
//   extraction of the allocation ....... py5gphy/nr_pdsch/nrpdsch_resource_mapping.py:87-129
//   DMRS generation and mapping ........ nr_pdsch_dmrs.py:90-120 (pdsch_dmrs_process)
//   data precoding and RE mapping ...... py5gphy/nr_pdsch/nr_pdsch_process.py:27-42,
//                                        nrpdsch_resource_mapping.py:58-85
// All three kernels are HBM-bound copies with a little arithmetic: one lane per resource element
// (extraction, data mapping) or per DMRS resource element (LS, DMRS mapping).  Loads run along the
// subcarrier axis of one antenna plane, so a wave reads contiguous runs; a lane stores its Nr (or
// Nr*Nt) contiguous output elements with 16-byte stores where size and alignment allow.
// The DMRS sequence is made on the device: cinit from slots[t], then every wave jumps both
// m-sequences to its own first bit with the jump-ahead matrices of ldpc5g_prbs.h (applied across
// the lanes, one ballot per matrix) and steps out the 256 bits (4 per DMRS RE) its lanes need.
#include <math.h>
#include <stdint.h>

#include "ldpc5g_common.h"
#include "ldpc5g_prbs.h"

namespace ldpc5g_impl {
namespace {

constexpr int kSlotThreads = 256;
constexpr int kSlotSyms = 14;

struct SlotDmrs {          // by value: everything about the DMRS that is the same for every slot
    int32_t carrier_re, rb_start, rb_size, S;
    int32_t sym[4];        // DMRS symbol indices
    int32_t port[4];       // port - 1000 of layer / transmit index p
    int32_t nid, nscid;
    double inv;            // LS: 1 / (2 scaling)
    float scaling;         // map: float32(scaling)
};

__device__ __forceinline__ int dmrs_sym(const SlotDmrs& c, int m) {   // c.sym[m] without a dynamic index
    return m == 0 ? c.sym[0] : m == 1 ? c.sym[1] : m == 2 ? c.sym[2] : c.sym[3];
}

// cinit of nr_pdsch_dmrs.py:249-251 for slot number `slot` and symbol `sym`
__device__ __forceinline__ uint32_t dmrs_cinit(const SlotDmrs& c, int32_t slot, int sym) {
    const uint64_t a = (uint64_t)(uint32_t)(14 * slot + sym + 1) * (uint64_t)(2 * c.nid + 1);
    return (uint32_t)(((a << 17) + (uint64_t)(2 * c.nid + c.nscid)) & 0x7FFFFFFFull);
}

// The lane's four sequence bits c(bit0 + 4 lane .. + 3), lane = threadIdx.x % 64, of the sequence
// started by cinit; bit0 is wave-uniform.  Each wave makes its own 256 bits: the jump above, then
// eight uniform 32-bit steps.  No LDS, no barrier.
__device__ __forceinline__ uint32_t dmrs_lane_bits(uint32_t cinit, uint32_t bit0) {
    const uint32_t n = __builtin_amdgcn_readfirstlane(1600u + bit0);
    uint32_t s1 = prbs_jump_wave(0, 1u, n);
    uint32_t s2 = prbs_jump_wave(1, __builtin_amdgcn_readfirstlane(cinit), n);
    const uint32_t g = (threadIdx.x >> 3) & 7u;
    uint32_t w = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t c = prbs_step32(s1, false) ^ prbs_step32(s2, true);
        w = g == i ? c : w;
    }
    return (w >> (4 * (threadIdx.x & 7))) & 15u;
}

// CNT consecutive complex elements to / from p; v16: p is 16-byte aligned (complex128 always is)
template <typename C, int CNT>
__device__ __forceinline__ void store_run(C* p, const C (&v)[CNT], bool v16) {
    if constexpr (sizeof(C) == 8 && CNT % 2 == 0) {
        if (v16) {
#pragma unroll
            for (int i = 0; i < CNT; i += 2)
                reinterpret_cast<float4*>(p)[i / 2] = make_float4(v[i].x, v[i].y, v[i + 1].x, v[i + 1].y);
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < CNT; ++i) p[i] = v[i];
}
template <typename C, int CNT>
__device__ __forceinline__ void load_run(const C* p, C (&v)[CNT], bool v16) {
    if constexpr (sizeof(C) == 8 && CNT % 2 == 0) {
        if (v16) {
#pragma unroll
            for (int i = 0; i < CNT; i += 2) {
                const float4 q = reinterpret_cast<const float4*>(p)[i / 2];
                v[i].x = q.x, v[i].y = q.y, v[i + 1].x = q.z, v[i + 1].y = q.w;
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < CNT; ++i) v[i] = p[i];
}

// ================================================================== LS estimate (grid -> h_ls)
// One lane per DMRS RE k of DMRS symbol m of slot t.  Per antenna the lane loads the four REs
// 4k .. 4k+3 once (32 or 64 contiguous bytes; a wave reads one contiguous run of the plane): they
// serve both CDM groups.  h_ls[t][m][k][r][p] = (Y[4k+d] conj(r(2k)) +- Y[4k+d+2] conj(r(2k+1)))
// * inv, d = (port/2) % 2, minus for odd ports (nr_pdsch_dmrs.py:207-215), in float64.
template <typename C, int NR, int NT>
__global__ __launch_bounds__(kSlotThreads) void slot_ls_kernel(const C* __restrict__ grid, int64_t ldg,
                                                               const int32_t* __restrict__ slots, SlotDmrs c,
                                                               C* __restrict__ h_ls, int64_t ldh, int ld16,
                                                               int st16) {
    using R = decltype(C{}.x);
    const int t = blockIdx.z, m = blockIdx.y;
    const int N = 3 * c.rb_size;
    const int k0 = blockIdx.x * kSlotThreads;
    const int k = k0 + (int)threadIdx.x;
    const int sym = dmrs_sym(c, m);
    C Y[NR][4];
    if (k < N) {
        const C* src = grid + (int64_t)t * ldg + (int64_t)sym * c.carrier_re + 12 * c.rb_start + 4 * k;
#pragma unroll
        for (int r = 0; r < NR; ++r) load_run<C, 4>(src + (int64_t)r * kSlotSyms * c.carrier_re, Y[r], ld16 != 0);
    }
    const uint32_t b = dmrs_lane_bits(dmrs_cinit(c, slots[t], sym),
                                      (uint32_t)(12 * c.rb_start + 4 * (k0 + (int)(threadIdx.x & ~63u))));
    if (k >= N) return;
    const double q = 0.70710678118654752440;   // 1 / sqrt(2)
    // conj(r(2k)) = a0 - j b0, conj(r(2k+1)) = a1 - j b1
    const double a0 = (b & 1u) ? -q : q, b0 = (b & 2u) ? -q : q;
    const double a1 = (b & 4u) ? -q : q, b1 = (b & 8u) ? -q : q;
    C out[NR * NT];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        double d0r[2], d0i[2], d1r[2], d1i[2];   // [delta]
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const double y0r = (double)Y[r][d].x, y0i = (double)Y[r][d].y;
            const double y1r = (double)Y[r][d + 2].x, y1i = (double)Y[r][d + 2].y;
            d0r[d] = y0r * a0 + y0i * b0, d0i[d] = y0i * a0 - y0r * b0;
            d1r[d] = y1r * a1 + y1i * b1, d1i[d] = y1i * a1 - y1r * b1;
        }
#pragma unroll
        for (int p = 0; p < NT; ++p) {
            const int d = (c.port[p] >> 1) & 1;
            const bool odd = c.port[p] & 1;
            const double e0r = d ? d0r[1] : d0r[0], e0i = d ? d0i[1] : d0i[0];
            const double e1r = d ? d1r[1] : d1r[0], e1i = d ? d1i[1] : d1i[0];
            const double hr = (odd ? e0r - e1r : e0r + e1r) * c.inv;
            const double hi = (odd ? e0i - e1i : e0i + e1i) * c.inv;
            out[r * NT + p].x = (R)hr, out[r * NT + p].y = (R)hi;
        }
    }
    store_run<C, NR * NT>(h_ls + (int64_t)t * ldh + ((int64_t)m * N + k) * (NR * NT), out, st16 != 0);
}

// ================================================================== extraction (grid -> y)
// One lane per RE of the allocation: y[t][s*12*rb + re][r] = grid[t][r][s*carrier_re + 12*rb_start + re].
template <typename C, int NR>
__global__ __launch_bounds__(kSlotThreads) void slot_extract_kernel(const C* __restrict__ grid, int64_t ldg,
                                                                    int carrier_re, int rb_start, int nre_sym,
                                                                    C* __restrict__ y, int64_t ldy, int st16) {
    const int t = blockIdx.z, s = blockIdx.y;
    const int re = blockIdx.x * kSlotThreads + (int)threadIdx.x;
    if (re >= nre_sym) return;
    const C* src = grid + (int64_t)t * ldg + (int64_t)s * carrier_re + 12 * rb_start + re;
    C v[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) v[r] = src[(int64_t)r * kSlotSyms * carrier_re];
    store_run<C, NR>(y + (int64_t)t * ldy + ((int64_t)s * nre_sym + re) * NR, v, st16 != 0);
}

// ================================================================== transmit map (sym -> grid)
struct SlotPrecode {
    float2 w[4][4];   // [antenna][layer]
    int32_t identity;
};

// blockIdx.y == 0: one lane per data RE i.  x = sym[t][i*NL .. i*NL + NL-1] (the layer mapping of
// nr_pdsch_process.py:27-32), grid[t][a][re_idx[i]'s position] = sum_l w[a][l] x[l] in float32,
// l ascending (identity: x[a], or 0 for a >= NL).  An index outside 0 .. 14*12*rb - 1 writes nothing.
// blockIdx.y == 1 + m: one lane per DMRS RE k of DMRS symbol m.  Layer l is port 1000 + l: at RE
// 4k + d and 4k + d + 2, d = (l/2) % 2, it sends float32(scaling) * r(2k) and
// float32(scaling * (1 - 2 (l % 2))) * r(2k+1) (nr_pdsch_dmrs.py:96-106), precoded the same way.
// Only the REs of CDM groups that carry a layer are written.
template <int NA, int NL>
__global__ __launch_bounds__(kSlotThreads) void slot_map_kernel(const float2* __restrict__ sym, int64_t ldsym,
                                                                const int32_t* __restrict__ re_idx, int64_t nre,
                                                                const int32_t* __restrict__ slots, SlotDmrs c,
                                                                SlotPrecode P, float2* __restrict__ grid,
                                                                int64_t ldg, int ld16) {
    const int t = blockIdx.z;
    float2* g = grid + (int64_t)t * ldg;
    const int nre_sym = 12 * c.rb_size;
    auto precode = [&](const float2 (&x)[NL], int a) {
        if (P.identity) return a < NL ? x[a < NL ? a : 0] : make_float2(0.0f, 0.0f);
        float re = 0.0f, im = 0.0f;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            re += P.w[a][l].x * x[l].x - P.w[a][l].y * x[l].y;
            im += P.w[a][l].x * x[l].y + P.w[a][l].y * x[l].x;
        }
        return make_float2(re, im);
    };
    if (blockIdx.y == 0) {
        const int64_t i = (int64_t)blockIdx.x * kSlotThreads + threadIdx.x;
        if (i >= nre) return;
        const int32_t idx = re_idx[i];
        if (idx < 0 || idx >= kSlotSyms * nre_sym) return;
        float2 x[NL];
        load_run<float2, NL>(sym + (int64_t)t * ldsym + i * NL, x, ld16 != 0);
        const int s = idx / nre_sym, re = idx - s * nre_sym;
        float2* dst = g + (int64_t)s * c.carrier_re + 12 * c.rb_start + re;
#pragma unroll
        for (int a = 0; a < NA; ++a) dst[(int64_t)a * kSlotSyms * c.carrier_re] = precode(x, a);
        return;
    }
    const int m = (int)blockIdx.y - 1;
    const int N = 3 * c.rb_size;
    const int k0 = blockIdx.x * kSlotThreads;
    if (k0 >= N) return;   // uniform: the launch is as wide as the data part
    const int k = k0 + (int)threadIdx.x;
    const int sm = dmrs_sym(c, m);
    const uint32_t b = dmrs_lane_bits(dmrs_cinit(c, slots[t], sm),
                                      (uint32_t)(12 * c.rb_start + 4 * (k0 + (int)(threadIdx.x & ~63u))));
    if (k >= N) return;
    const float q = 1.0f / (float)sqrt(2.0);   // nrModulate's complex64 division by sqrt(2)
    const float2 r0 = make_float2((b & 1u) ? -q : q, (b & 2u) ? -q : q);
    const float2 r1 = make_float2((b & 4u) ? -q : q, (b & 8u) ? -q : q);
    float2* dst = g + (int64_t)sm * c.carrier_re + 12 * c.rb_start + 4 * k;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        if (d == 1 && NL <= 2) break;   // layers 2, 3 are the second CDM group
        float2 x0[NL], x1[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const bool mine = ((l >> 1) & 1) == d;
            const float s0 = mine ? c.scaling : 0.0f;
            const float s1 = mine ? ((l & 1) ? -c.scaling : c.scaling) : 0.0f;
            x0[l] = make_float2(s0 * r0.x, s0 * r0.y);
            x1[l] = make_float2(s1 * r1.x, s1 * r1.y);
        }
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            dst[(int64_t)a * kSlotSyms * c.carrier_re + d] = precode(x0, a);
            dst[(int64_t)a * kSlotSyms * c.carrier_re + d + 2] = precode(x1, a);
        }
    }
}

// ------------------------------------------------------------------------------ host checks
int check_dmrs(SlotDmrs& c, int32_t T, int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t S,
               const int32_t* sym_idx, int32_t nNIDnSCID, int32_t nSCID, int32_t num_cdm_groups) {
    if (T < 1 || T > 65535) return fail(LDPC5G_ESIZE, "T=%d outside 1..65535", T);
    if (carrier_re < 12 || carrier_re % 12 || carrier_re / 12 > 275)
        return fail(LDPC5G_ESIZE, "carrier_re=%d: a multiple of 12 up to 275 PRB", carrier_re);
    if (rb_size < 1 || rb_size > 275) return fail(LDPC5G_ESIZE, "rb_size=%d outside 1..275", rb_size);
    if (rb_start < 0 || rb_start > 275 || rb_start + rb_size > carrier_re / 12)
        return fail(LDPC5G_ESIZE, "rb_start=%d + rb_size=%d beyond the carrier's %d PRB", rb_start, rb_size, carrier_re / 12);
    if (S < 1 || S > 4) return fail(LDPC5G_ESIZE, "S=%d DMRS symbols outside 1..4", S);
    if (!sym_idx) return fail(LDPC5G_ESIZE, "sym_idx is null");
    for (int m = 0; m < S; ++m)
        if (sym_idx[m] < 0 || sym_idx[m] > 13 || (m > 0 && sym_idx[m] <= sym_idx[m - 1]))
            return fail(LDPC5G_ESIZE, "sym_idx[%d]=%d: strictly ascending in 0..13", m, sym_idx[m]);
    if (nNIDnSCID < 0 || nNIDnSCID > 65535) return fail(LDPC5G_ESIZE, "nNIDnSCID=%d outside 0..65535", nNIDnSCID);
    if (nSCID < 0 || nSCID > 1) return fail(LDPC5G_ESIZE, "nSCID=%d outside 0..1", nSCID);
    if (num_cdm_groups < 1 || num_cdm_groups > 2)
        return fail(LDPC5G_ESIZE, "num_cdm_groups=%d outside 1..2 (DMRS configuration type 1)", num_cdm_groups);
    c.carrier_re = carrier_re, c.rb_start = rb_start, c.rb_size = rb_size, c.S = S;
    for (int m = 0; m < 4; ++m) c.sym[m] = m < S ? sym_idx[m] : 0;
    c.nid = nNIDnSCID, c.nscid = nSCID;
    const double scaling = num_cdm_groups == 1 ? 1.0 : pow(10.0, -3.0 / 20.0);   // nr_pdsch_dmrs.py:171-174
    c.inv = 1.0 / (2.0 * scaling);
    c.scaling = (float)scaling;
    return LDPC5G_OK;
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

template <typename C>
int launch_frontend(const void* grid, int64_t ldg, const int32_t* slots, int T, const SlotDmrs& c, int Nr, int Nt,
                    void* h_ls, int64_t ldh, void* y, int64_t ldy, hipStream_t st) {
    const bool c64 = sizeof(C) == 8;
    const int ld16 = !c64 || (aligned(grid, 16) && ldg % 2 == 0);
    if (h_ls) {
        const int N = 3 * c.rb_size;
        const int st16 = !c64 || (aligned(h_ls, 16) && ldh % 2 == 0);
        const dim3 g((unsigned)((N + kSlotThreads - 1) / kSlotThreads), c.S, T), b(kSlotThreads);
#define LDPC5G_LS(NR, NT) \
    hipLaunchKernelGGL((slot_ls_kernel<C, NR, NT>), g, b, 0, st, (const C*)grid, ldg, slots, c, (C*)h_ls, ldh, ld16, st16)
#define LDPC5G_LS_NT(NR)                        \
    switch (Nt) {                               \
        case 1: LDPC5G_LS(NR, 1); break;        \
        case 2: LDPC5G_LS(NR, 2); break;        \
        case 3: LDPC5G_LS(NR, 3); break;        \
        default: LDPC5G_LS(NR, 4); break;       \
    }
        if (Nr == 1) { LDPC5G_LS_NT(1) } else if (Nr == 2) { LDPC5G_LS_NT(2) } else { LDPC5G_LS_NT(4) }
#undef LDPC5G_LS_NT
#undef LDPC5G_LS
        const int rc = check_hip(hipGetLastError(), "slot_ls_kernel launch");
        if (rc) return rc;
    }
    if (y) {
        const int nre_sym = 12 * c.rb_size;
        const int st16 = !c64 || (aligned(y, 16) && ldy % 2 == 0);
        const dim3 g((unsigned)((nre_sym + kSlotThreads - 1) / kSlotThreads), kSlotSyms, T), b(kSlotThreads);
#define LDPC5G_EX(NR) \
    hipLaunchKernelGGL((slot_extract_kernel<C, NR>), g, b, 0, st, (const C*)grid, ldg, c.carrier_re, c.rb_start, nre_sym, (C*)y, ldy, st16)
        if (Nr == 1) LDPC5G_EX(1); else if (Nr == 2) LDPC5G_EX(2); else LDPC5G_EX(4);
#undef LDPC5G_EX
        return check_hip(hipGetLastError(), "slot_extract_kernel launch");
    }
    return LDPC5G_OK;
}

template <int NA>
void launch_map_na(int NL, dim3 g, hipStream_t st, const float2* sym, int64_t ldsym, const int32_t* re_idx,
                   int64_t nre, const int32_t* slots, const SlotDmrs& c, const SlotPrecode& P, float2* grid,
                   int64_t ldg, int ld16) {
    const dim3 b(kSlotThreads);
#define LDPC5G_MAP(NL_) \
    hipLaunchKernelGGL((slot_map_kernel<NA, NL_>), g, b, 0, st, sym, ldsym, re_idx, nre, slots, c, P, grid, ldg, ld16)
    switch (NL) {
        case 1: LDPC5G_MAP(1); break;
        case 2: LDPC5G_MAP(2); break;
        case 3: LDPC5G_MAP(3); break;
        default: LDPC5G_MAP(4); break;
    }
#undef LDPC5G_MAP
}

}  // namespace
}  // namespace ldpc5g_impl

using namespace ldpc5g_impl;

extern "C" {

int ldpc5g_slot_rx_frontend(const void* grid, int64_t ldgrid, int32_t in_dtype, const int32_t* slots, int32_t T,
                            int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t Nr, int32_t Nt,
                            const int32_t* ports, int32_t S, const int32_t* sym_idx, int32_t nNIDnSCID,
                            int32_t nSCID, int32_t num_cdm_groups, void* h_ls, int64_t ldh, void* y, int64_t ldy,
                            void* stream) {
    clear_error();
    if (in_dtype != LDPC5G_F32 && in_dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad grid dtype %d", in_dtype);
    if (Nr != 1 && Nr != 2 && Nr != 4) return fail(LDPC5G_ESIZE, "Nr=%d: supported Nr in {1, 2, 4}", Nr);
    if (Nt < 1 || Nt > 4) return fail(LDPC5G_ESIZE, "Nt=%d outside 1..4", Nt);
    if (!ports) return fail(LDPC5G_ESIZE, "ports is null");
    SlotDmrs c{};
    for (int p = 0; p < Nt; ++p) {
        if (ports[p] < 0 || ports[p] > 3) return fail(LDPC5G_ESIZE, "ports[%d]=%d: port 1000..1003 as 0..3", p, ports[p]);
        for (int o = 0; o < p; ++o)
            if (ports[o] == ports[p]) return fail(LDPC5G_ESIZE, "ports[%d]=%d repeats ports[%d]", p, ports[p], o);
        c.port[p] = ports[p];
    }
    const int rc = check_dmrs(c, T, carrier_re, rb_start, rb_size, S, sym_idx, nNIDnSCID, nSCID, num_cdm_groups);
    if (rc) return rc;
    const int64_t N = 3 * (int64_t)rb_size;
    if (ldgrid < (int64_t)Nr * kSlotSyms * carrier_re)
        return fail(LDPC5G_ESIZE, "grid stride %lld shorter than Nr*14*carrier_re", (long long)ldgrid);
    if (h_ls && ldh < S * N * Nr * Nt) return fail(LDPC5G_ESIZE, "h_ls stride %lld shorter than S*N*Nr*Nt", (long long)ldh);
    if (y && ldy < kSlotSyms * 4 * N * Nr) return fail(LDPC5G_ESIZE, "y stride %lld shorter than 14*12*rb_size*Nr", (long long)ldy);
    if (!grid || !slots) return fail(LDPC5G_ESIZE, "null buffer (grid, slots)");
    if (!h_ls && !y) return fail(LDPC5G_ESIZE, "null buffer: both h_ls and y are NULL, nothing to do");
    const size_t al = in_dtype == LDPC5G_F64 ? 16 : 8;
    if (!aligned(grid, al) || !aligned(h_ls, al) || !aligned(y, al) || !aligned(slots, 4))
        return fail(LDPC5G_ESIZE, "a buffer is not aligned to its element size");
    hipStream_t st = (hipStream_t)stream;
    if (in_dtype == LDPC5G_F32) return launch_frontend<float2>(grid, ldgrid, slots, T, c, Nr, Nt, h_ls, ldh, y, ldy, st);
    return launch_frontend<double2>(grid, ldgrid, slots, T, c, Nr, Nt, h_ls, ldh, y, ldy, st);
}

int ldpc5g_slot_map(const void* sym, int64_t ldsym, const int32_t* re_idx, int64_t nre, const int32_t* slots,
                    int32_t T, int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t num_ant, int32_t NL,
                    const float* precoding, int32_t S, const int32_t* sym_idx, int32_t nNIDnSCID, int32_t nSCID,
                    int32_t num_cdm_groups, void* grid, int64_t ldgrid, void* stream) {
    clear_error();
    if (num_ant != 1 && num_ant != 2 && num_ant != 4) return fail(LDPC5G_ESIZE, "num_ant=%d: supported num_ant in {1, 2, 4}", num_ant);
    if (NL < 1 || NL > 4) return fail(LDPC5G_ESIZE, "NL=%d outside 1..4", NL);
    if (!precoding && NL > num_ant) return fail(LDPC5G_ESIZE, "NL=%d > num_ant=%d needs a precoding matrix", NL, num_ant);
    SlotDmrs c{};
    for (int l = 0; l < NL; ++l) c.port[l] = l;   // row l of the reference's map is port 1000 + l
    const int rc = check_dmrs(c, T, carrier_re, rb_start, rb_size, S, sym_idx, nNIDnSCID, nSCID, num_cdm_groups);
    if (rc) return rc;
    if (nre < 0 || nre > (int64_t)kSlotSyms * 12 * rb_size) return fail(LDPC5G_ESIZE, "nre=%lld outside 0..14*12*rb_size", (long long)nre);
    if (ldgrid < (int64_t)num_ant * kSlotSyms * carrier_re)
        return fail(LDPC5G_ESIZE, "grid stride %lld shorter than num_ant*14*carrier_re", (long long)ldgrid);
    if (nre > 0 && ldsym < nre * NL) return fail(LDPC5G_ESIZE, "sym stride %lld shorter than nre*NL", (long long)ldsym);
    if (!grid || !slots || (nre > 0 && (!sym || !re_idx))) return fail(LDPC5G_ESIZE, "null buffer (sym, re_idx, slots, grid)");
    if (!aligned(grid, 8) || !aligned(sym, 8) || !aligned(re_idx, 4) || !aligned(slots, 4))
        return fail(LDPC5G_ESIZE, "a buffer is not aligned to its element size");
    SlotPrecode P{};
    P.identity = precoding ? 0 : 1;
    if (precoding)
        for (int a = 0; a < num_ant; ++a)
            for (int l = 0; l < NL; ++l) P.w[a][l] = make_float2(precoding[2 * (a * NL + l)], precoding[2 * (a * NL + l) + 1]);
    const int64_t N = 3 * (int64_t)rb_size;
    const int64_t wide = nre > N ? nre : N;
    const dim3 g((unsigned)((wide + kSlotThreads - 1) / kSlotThreads), 1 + S, T);
    const int ld16 = aligned(sym, 16) && ldsym % 2 == 0;
    hipStream_t st = (hipStream_t)stream;
    const float2* s2 = (const float2*)sym;
    float2* g2 = (float2*)grid;
    if (num_ant == 1) launch_map_na<1>(NL, g, st, s2, ldsym, re_idx, nre, slots, c, P, g2, ldgrid, ld16);
    else if (num_ant == 2) launch_map_na<2>(NL, g, st, s2, ldsym, re_idx, nre, slots, c, P, g2, ldgrid, ld16);
    else launch_map_na<4>(NL, g, st, s2, ldsym, re_idx, nre, slots, c, P, g2, ldgrid, ld16);
    return check_hip(hipGetLastError(), "slot_map_kernel launch");
}

}  // extern "C"
