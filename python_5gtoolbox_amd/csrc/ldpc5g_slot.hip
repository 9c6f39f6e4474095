// ldpc5g_slot.hip — the slot front end: the frequency-domain resource grid on one side, the
// channel estimator's H_LS and the equaliser's interleaved y on the other, batched over slots:
//   DMRS least-squares estimate ........ py5gphy/nr_pdsch/nr_pdsch_dmrs.py:139-227 (pdsch_dmrs_LS_est),
//                                        py5gphy/nr_pusch/nr_pusch_dmrs.py:107-200 (pusch_dmrs_LS_est)
//   DMRS sequence r(n), Gold / QPSK .... nr_pdsch_dmrs.py:244-256 (_gen_seq), nrPRBS.py:5-25
//   DMRS sequence r(n), low-PAPR ....... nr_pusch_dmrs.py:216-249 (_gen_seq_with_transform_precoding)
//   extraction of the allocation ....... py5gphy/nr_pdsch/nrpdsch_resource_mapping.py:87-129
//   DMRS generation and mapping ........ nr_pdsch_dmrs.py:90-120 (pdsch_dmrs_process),
//                                        nr_pusch_dmrs.py:66-101 (transform precoding)
//   data precoding and RE mapping ...... py5gphy/nr_pdsch/nr_pdsch_process.py:27-42,
//                                        nrpdsch_resource_mapping.py:58-85
// (ldpc5g_slot_rx_frontend / ldpc5g_slot_map and their _tp forms, include/ldpc5g.h).
// All three kernels are HBM-bound copies with a little arithmetic: one lane per resource element
// (extraction, data mapping) or per DMRS resource element (LS, DMRS mapping).  Loads run along the
// subcarrier axis of one antenna plane, so a wave reads contiguous runs; a lane stores its Nr (or
// Nr*Nt) contiguous output elements with 16-byte stores where size and alignment allow.
// The LS and map kernels take the DMRS sequence as a compile-time source type (GoldSeq,
// LowPaprSeq): a wave-uniform part that every lane of a wave runs before any lane leaves, and a
// per-lane part that yields r(2k), r(2k+1).  Both are made on the device from slots[t].  Gold: cinit,
// then every wave jumps both m-sequences to its own first bit with the jump-ahead matrices of
// ldpc5g_prbs.h (applied across the lanes, one ballot per matrix) and steps out the 256 bits (4 per
// DMRS RE) its lanes need.  Low-PAPR: the hopping (u, v) from the same jump, then one point of
// ldpc5g_lowpapr.h per sequence element, or the caller's base sequence.
#include <math.h>
#include <stdint.h>

#include "ldpc5g_common.h"
#include "ldpc5g_lowpapr.h"
#include "ldpc5g_prbs.h"

namespace ldpc5g_impl {
namespace {

constexpr int kSlotThreads = 256;
constexpr int kSlotSyms = 14;

struct SlotDmrs {          // by value: what is the same for every slot and either sequence
    int32_t carrier_re, rb_start, rb_size, S;
    int32_t sym[4];        // DMRS symbol indices
    int32_t port[4];       // port - 1000 of layer / transmit index p
    double inv;            // LS: 1 / (2 scaling)
    double scaling;        // map
};

__device__ __forceinline__ int dmrs_sym(const SlotDmrs& c, int m) {   // c.sym[m] without a dynamic index
    return m == 0 ? c.sym[0] : m == 1 ? c.sym[1] : m == 2 ? c.sym[2] : c.sym[3];
}

// ------------------------------------------------------------------ the two sequence sources
// A source S has
//   S::Wave wave(c, slot, sym, k0)   the wave-uniform part for DMRS symbol `sym` of slot number
//                                    `slot`, k0 the workgroup's first DMRS RE.  It ends in
//                                    prbs_jump_wave: every lane of the wave must be active.
//   pair(c, w, t, m, k, r)           the lane's r(2k) = r[0] + j r[1], r(2k+1) = r[2] + j r[3] of DMRS
//                                    symbol m of slot t, in float64 (LS) or S::MapReal (map)
//   S::MapReal                       the type in which the map forms scaling * r before float32
//   S::kAcc0                         what the precoding sum over the layers starts from
//   S::kOneLayer                     only Nt = NL = 1 is instantiated
//   map_port(c, l)                   port - 1000 of layer l of the map

// Gold sequence, QPSK (nr_pdsch_dmrs.py:244-256).  w: the lane's four bits c(2(2k)) .. c(2(2k+1)+1).
struct GoldSeq {
    int32_t nid, nscid;
    using Wave = uint32_t;
    using MapReal = float;                    // nrModulate's complex64 and float32 products
    static constexpr float kAcc0 = 0.0f;      // the reference's matrix product: a sum from zero
    static constexpr bool kOneLayer = false;
    static __device__ __forceinline__ int map_port(const SlotDmrs&, int l) { return l; }   // the reference's row l

    // cinit of nr_pdsch_dmrs.py:249-251, then the bits c(bit0 + 4 lane .. + 3), lane = threadIdx.x %
    // 64, bit0 the wave's first.  Each wave makes its own 256 bits: the jump, then eight uniform
    // 32-bit steps.  No LDS, no barrier.
    __device__ __forceinline__ Wave wave(const SlotDmrs& c, int32_t slot, int sym, int k0) const {
        const uint64_t a = (uint64_t)(uint32_t)(14 * slot + sym + 1) * (uint64_t)(2 * nid + 1);
        const uint32_t cinit = (uint32_t)(((a << 17) + (uint64_t)(2 * nid + nscid)) & 0x7FFFFFFFull);
        const uint32_t bit0 = (uint32_t)(12 * c.rb_start + 4 * (k0 + (int)(threadIdx.x & ~63u)));
        const uint32_t n = __builtin_amdgcn_readfirstlane(1600u + bit0);
        uint32_t s1 = prbs_jump_wave(0, 1u, n);
        uint32_t s2 = prbs_jump_wave(1, __builtin_amdgcn_readfirstlane(cinit), n);
        const uint32_t g = (threadIdx.x >> 3) & 7u;
        uint32_t w = 0;
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t b = prbs_step32(s1, false) ^ prbs_step32(s2, true);
            w = g == i ? b : w;
        }
        return (w >> (4 * (threadIdx.x & 7))) & 15u;
    }
    template <typename F>
    __device__ __forceinline__ void pair(const SlotDmrs&, Wave b, int, int, int, F (&r)[4]) const {
        F q;
        if constexpr (sizeof(F) == 8) q = 0.70710678118654752440;   // 1 / sqrt(2)
        else q = 1.0f / (float)sqrt(2.0);                           // nrModulate's complex64 division by sqrt(2)
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = ((b >> i) & 1u) ? -q : q;
    }
};

// Low-PAPR sequence rbar_{u,v}, alpha = 0 (nr_pusch_dmrs.py:216-249), or the caller's base_seq.
struct LowPaprSeq {
    int32_t id, hopping;       // nPuschID; 0 neither, 1 group, 2 sequence hopping
    int32_t MZC, NZC;          // 6 rb_size and the largest prime below it
    const double2* base_seq;   // [T][S][MZC] instead of the generated sequence, or null
    struct Wave {
        int u, v;
    };
    using MapReal = double;                   // float32(double scaling * double r)
    static constexpr float kAcc0 = -0.0f;     // one layer, one product, no sum: x + -0 is x, sign kept
    static constexpr bool kOneLayer = true;
    static __device__ __forceinline__ int map_port(const SlotDmrs& c, int) { return c.port[0]; }

    // (u, v) of the symbol.  The Gold bits c(n) are the low bits of the two jumped states: bit i of a
    // state at n is x(n + i).  The reference makes one frame of bits (slot < 20); a position past the
    // jump tables' 8192 wraps instead of reading beyond.  A uniform branch around the jumps.
    __device__ __forceinline__ Wave wave(const SlotDmrs&, int32_t slot, int sym, int) const {
        Wave w{id % 30, 0};
        if (base_seq) return w;
        const uint32_t pos = (uint32_t)(14 * slot + sym);
        if (hopping == 1) {
            const uint32_t n = __builtin_amdgcn_readfirstlane((1600u + 8u * pos) & 8191u);
            const uint32_t s1 = prbs_jump_wave(0, 1u, n), s2 = prbs_jump_wave(1, (uint32_t)(id / 30), n);
            w.u = (int)((((s1 ^ s2) & 255u) % 30u + (uint32_t)id) % 30u);
        } else if (hopping == 2 && MZC >= 72) {
            const uint32_t n = __builtin_amdgcn_readfirstlane((1600u + pos) & 8191u);
            const uint32_t s1 = prbs_jump_wave(0, 1u, n), s2 = prbs_jump_wave(1, (uint32_t)id, n);
            w.v = (int)((s1 ^ s2) & 1u);
        }
        return w;
    }
    __device__ __forceinline__ void pair(const SlotDmrs& c, Wave w, int t, int m, int k, double (&r)[4]) const {
        if (base_seq) {
            const double2* b = base_seq + ((int64_t)t * c.S + m) * MZC + 2 * k;
            r[0] = b[0].x, r[1] = b[0].y, r[2] = b[1].x, r[3] = b[1].y;
        } else {
            low_papr_point(w.u, w.v, 2 * k, MZC, NZC, r[0], r[1]);
            low_papr_point(w.u, w.v, 2 * k + 1, MZC, NZC, r[2], r[3]);
        }
    }
};

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
// * inv, d = (port/2) % 2, minus for odd ports (nr_pdsch_dmrs.py:207-215, nr_pusch_dmrs.py:174-190),
// in float64.
template <typename C, int NR, int NT, typename Seq>
__global__ __launch_bounds__(kSlotThreads) void slot_ls_kernel(const C* __restrict__ grid, int64_t ldg,
                                                               const int32_t* __restrict__ slots, SlotDmrs c, Seq q,
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
    const typename Seq::Wave w = q.wave(c, slots[t], sym, k0);   // before any lane leaves
    if (k >= N) return;
    double s[4];   // conj(r(2k)) = s[0] - j s[1], conj(r(2k+1)) = s[2] - j s[3]
    q.pair(c, w, t, m, k, s);
    C out[NR * NT];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        double d0r[2], d0i[2], d1r[2], d1i[2];   // [delta]; a single layer fills only [0], with its own delta
#pragma unroll
        for (int d = 0; d < (NT == 1 ? 1 : 2); ++d) {
            const bool up = NT == 1 ? (c.port[0] >> 1) & 1 : d;
            const C lo0 = Y[r][0], lo1 = Y[r][2], up0 = Y[r][1], up1 = Y[r][3];   // read all, then choose values
            const double y0r = (double)(up ? up0.x : lo0.x), y0i = (double)(up ? up0.y : lo0.y);
            const double y1r = (double)(up ? up1.x : lo1.x), y1i = (double)(up ? up1.y : lo1.y);
            d0r[d] = y0r * s[0] + y0i * s[1], d0i[d] = y0i * s[0] - y0r * s[1];
            d1r[d] = y1r * s[2] + y1i * s[3], d1i[d] = y1i * s[2] - y1r * s[3];
        }
#pragma unroll
        for (int p = 0; p < NT; ++p) {
            const int d = NT == 1 ? 0 : (c.port[p] >> 1) & 1;
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
// blockIdx.y == 1 + m: one lane per DMRS RE k of DMRS symbol m.  Layer l on port map_port(l): at RE
// 4k + d and 4k + d + 2, d = (port/2) % 2, it sends float32(scaling r(2k)) and float32(+- scaling
// r(2k+1)), minus for odd ports, the products in Seq::MapReal (nr_pdsch_dmrs.py:96-106,
// nr_pusch_dmrs.py:76-101), precoded the same way; a layer of the other CDM group adds signed zeros.
// Only the REs of CDM groups that carry a layer are written.
template <int NA, int NL, typename Seq>
__global__ __launch_bounds__(kSlotThreads) void slot_map_kernel(const float2* __restrict__ sym, int64_t ldsym,
                                                                const int32_t* __restrict__ re_idx, int64_t nre,
                                                                const int32_t* __restrict__ slots, SlotDmrs c, Seq q,
                                                                SlotPrecode P, float2* __restrict__ grid,
                                                                int64_t ldg, int ld16) {
    const int t = blockIdx.z;
    float2* g = grid + (int64_t)t * ldg;
    const int nre_sym = 12 * c.rb_size;
    auto precode = [&](const float2 (&x)[NL], int a) {
        if (P.identity) return a < NL ? x[a < NL ? a : 0] : make_float2(0.0f, 0.0f);
        float re = Seq::kAcc0, im = Seq::kAcc0;
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
    const typename Seq::Wave w = q.wave(c, slots[t], sm, k0);   // before any lane leaves
    if (k >= N) return;
    using F = typename Seq::MapReal;
    F r[4];
    q.pair(c, w, t, m, k, r);
    const F sc = (F)c.scaling;
    float2* dst = g + (int64_t)sm * c.carrier_re + 12 * c.rb_start + 4 * k;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        bool used = false;
        float2 x0[NL], x1[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const int port = Seq::map_port(c, l);
            const bool mine = ((port >> 1) & 1) == d;
            used |= mine;
            const F s0 = mine ? sc : (F)0;
            const F s1 = mine ? ((port & 1) ? -sc : sc) : (F)0;
            x0[l] = make_float2((float)(s0 * r[0]), (float)(s0 * r[1]));
            x1[l] = make_float2((float)(s1 * r[2]), (float)(s1 * r[3]));
        }
        if (!used) continue;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            dst[(int64_t)a * kSlotSyms * c.carrier_re + d] = precode(x0, a);
            dst[(int64_t)a * kSlotSyms * c.carrier_re + d + 2] = precode(x1, a);
        }
    }
}

// ------------------------------------------------------------------------------ host checks
// what every entry point checks of the allocation and the DMRS symbols
int check_dmrs(SlotDmrs& c, int32_t T, int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t S,
               const int32_t* sym_idx) {
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
    c.carrier_re = carrier_re, c.rb_start = rb_start, c.rb_size = rb_size, c.S = S;
    for (int m = 0; m < 4; ++m) c.sym[m] = m < S ? sym_idx[m] : 0;
    return LDPC5G_OK;
}

void set_scaling(SlotDmrs& c, int num_cdm_groups) {   // nr_pdsch_dmrs.py:171-174, nr_pusch_dmrs.py:150-154
    c.scaling = num_cdm_groups == 1 ? 1.0 : pow(10.0, -3.0 / 20.0);
    c.inv = 1.0 / (2.0 * c.scaling);
}

int check_gold(SlotDmrs& c, GoldSeq& q, int32_t nNIDnSCID, int32_t nSCID, int32_t num_cdm_groups) {
    if (nNIDnSCID < 0 || nNIDnSCID > 65535) return fail(LDPC5G_ESIZE, "nNIDnSCID=%d outside 0..65535", nNIDnSCID);
    if (nSCID < 0 || nSCID > 1) return fail(LDPC5G_ESIZE, "nSCID=%d outside 0..1", nSCID);
    if (num_cdm_groups < 1 || num_cdm_groups > 2)
        return fail(LDPC5G_ESIZE, "num_cdm_groups=%d outside 1..2 (DMRS configuration type 1)", num_cdm_groups);
    q.nid = nNIDnSCID, q.nscid = nSCID;
    set_scaling(c, num_cdm_groups);
    return LDPC5G_OK;
}

// after check_dmrs: one layer on `port`, NumCDMGroupsWithoutData == 2
int check_low_papr(SlotDmrs& c, LowPaprSeq& q, int32_t port, int32_t nPuschID, int32_t hopping, const void* base_seq) {
    if (!smooth235(c.rb_size)) return fail(LDPC5G_ESIZE, "rb_size=%d: 2^a 3^b 5^c in 1..275 (38.211 6.3.1.4)", c.rb_size);
    if (port < 0 || port > 3) return fail(LDPC5G_ESIZE, "port=%d: port 1000..1003 as 0..3", port);
    if (nPuschID < 0 || nPuschID > 1007) return fail(LDPC5G_ESIZE, "nPuschID=%d outside 0..1007", nPuschID);
    if (hopping < 0 || hopping > 2) return fail(LDPC5G_ESIZE, "hopping=%d outside 0..2 (neither, group, sequence)", hopping);
    if (c.rb_size <= 4 && !base_seq)
        return fail(LDPC5G_ESIZE, "base_seq is null at rb_size=%d: the sequences of length 6..24 are tables "
                                  "(38.211 5.2.2.2), pass them", c.rb_size);
    if (!aligned(base_seq, 16)) return fail(LDPC5G_ESIZE, "base_seq is not aligned to its element size");
    c.port[0] = port;
    q.id = nPuschID, q.hopping = hopping, q.MZC = 6 * c.rb_size, q.NZC = low_papr_nzc(q.MZC);
    q.base_seq = (const double2*)base_seq;
    set_scaling(c, 2);
    return LDPC5G_OK;
}

template <typename C, typename Seq>
int launch_frontend(const void* grid, int64_t ldg, const int32_t* slots, int T, const SlotDmrs& c, const Seq& q, int Nr,
                    int Nt, void* h_ls, int64_t ldh, void* y, int64_t ldy, hipStream_t st) {
    const bool c64 = sizeof(C) == 8;
    const int ld16 = !c64 || (aligned(grid, 16) && ldg % 2 == 0);
    if (h_ls) {
        const int N = 3 * c.rb_size;
        const int st16 = !c64 || (aligned(h_ls, 16) && ldh % 2 == 0);
        const dim3 g((unsigned)((N + kSlotThreads - 1) / kSlotThreads), c.S, T), b(kSlotThreads);
#define LDPC5G_LS(NR, NT) \
    hipLaunchKernelGGL((slot_ls_kernel<C, NR, NT, Seq>), g, b, 0, st, (const C*)grid, ldg, slots, c, q, (C*)h_ls, ldh, ld16, st16)
#define LDPC5G_LS_NT(NR)                            \
    if constexpr (Seq::kOneLayer) LDPC5G_LS(NR, 1); \
    else switch (Nt) {                              \
        case 1: LDPC5G_LS(NR, 1); break;            \
        case 2: LDPC5G_LS(NR, 2); break;            \
        case 3: LDPC5G_LS(NR, 3); break;            \
        default: LDPC5G_LS(NR, 4); break;           \
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

// the dtype, antenna, stride, null and alignment checks of a front-end call, then its launches
template <typename Seq>
int run_frontend(const SlotDmrs& c, const Seq& q, const void* grid, int64_t ldgrid, int32_t in_dtype,
                 const int32_t* slots, int32_t T, int32_t Nr, int32_t Nt, void* h_ls, int64_t ldh, void* y, int64_t ldy,
                 void* stream) {
    if (in_dtype != LDPC5G_F32 && in_dtype != LDPC5G_F64) return fail(LDPC5G_ESIZE, "bad grid dtype %d", in_dtype);
    if (Nr != 1 && Nr != 2 && Nr != 4) return fail(LDPC5G_ESIZE, "Nr=%d: supported Nr in {1, 2, 4}", Nr);
    const int64_t N = 3 * (int64_t)c.rb_size;
    if (ldgrid < (int64_t)Nr * kSlotSyms * c.carrier_re)
        return fail(LDPC5G_ESIZE, "grid stride %lld shorter than Nr*14*carrier_re", (long long)ldgrid);
    if (h_ls && ldh < c.S * N * Nr * Nt) return fail(LDPC5G_ESIZE, "h_ls stride %lld shorter than S*N*Nr*Nt", (long long)ldh);
    if (y && ldy < kSlotSyms * 4 * N * Nr) return fail(LDPC5G_ESIZE, "y stride %lld shorter than 14*12*rb_size*Nr", (long long)ldy);
    if (!grid || !slots) return fail(LDPC5G_ESIZE, "null buffer (grid, slots)");
    if (!h_ls && !y) return fail(LDPC5G_ESIZE, "null buffer: both h_ls and y are NULL, nothing to do");
    const size_t al = in_dtype == LDPC5G_F64 ? 16 : 8;
    if (!aligned(grid, al) || !aligned(h_ls, al) || !aligned(y, al) || !aligned(slots, 4))
        return fail(LDPC5G_ESIZE, "a buffer is not aligned to its element size");
    hipStream_t st = (hipStream_t)stream;
    if (in_dtype == LDPC5G_F32) return launch_frontend<float2>(grid, ldgrid, slots, T, c, q, Nr, Nt, h_ls, ldh, y, ldy, st);
    return launch_frontend<double2>(grid, ldgrid, slots, T, c, q, Nr, Nt, h_ls, ldh, y, ldy, st);
}

// the antenna, size, stride, null and alignment checks of a map call, then its launch;
// precoding: [num_ant][NL] complex64 as float pairs, or null for identity
template <typename Seq>
int run_map(const SlotDmrs& c, const Seq& q, const void* sym, int64_t ldsym, const int32_t* re_idx, int64_t nre,
            const int32_t* slots, int32_t T, int32_t num_ant, int32_t NL, const float* precoding, void* grid,
            int64_t ldgrid, void* stream) {
    if (num_ant != 1 && num_ant != 2 && num_ant != 4) return fail(LDPC5G_ESIZE, "num_ant=%d: supported num_ant in {1, 2, 4}", num_ant);
    if (!precoding && NL > num_ant) return fail(LDPC5G_ESIZE, "NL=%d > num_ant=%d needs a precoding matrix", NL, num_ant);
    if (nre < 0 || nre > (int64_t)kSlotSyms * 12 * c.rb_size) return fail(LDPC5G_ESIZE, "nre=%lld outside 0..14*12*rb_size", (long long)nre);
    if (ldgrid < (int64_t)num_ant * kSlotSyms * c.carrier_re)
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
    const int64_t N = 3 * (int64_t)c.rb_size;
    const int64_t wide = nre > N ? nre : N;
    const dim3 g((unsigned)((wide + kSlotThreads - 1) / kSlotThreads), 1 + c.S, T), b(kSlotThreads);
    const int ld16 = aligned(sym, 16) && ldsym % 2 == 0;
#define LDPC5G_MAP(NA, NL_)                                                                                           \
    hipLaunchKernelGGL((slot_map_kernel<NA, NL_, Seq>), g, b, 0, (hipStream_t)stream, (const float2*)sym, ldsym, re_idx, \
                       nre, slots, c, q, P, (float2*)grid, ldgrid, ld16)
#define LDPC5G_MAP_NL(NA)                            \
    if constexpr (Seq::kOneLayer) LDPC5G_MAP(NA, 1); \
    else switch (NL) {                               \
        case 1: LDPC5G_MAP(NA, 1); break;            \
        case 2: LDPC5G_MAP(NA, 2); break;            \
        case 3: LDPC5G_MAP(NA, 3); break;            \
        default: LDPC5G_MAP(NA, 4); break;           \
    }
    if (num_ant == 1) { LDPC5G_MAP_NL(1) } else if (num_ant == 2) { LDPC5G_MAP_NL(2) } else { LDPC5G_MAP_NL(4) }
#undef LDPC5G_MAP_NL
#undef LDPC5G_MAP
    return check_hip(hipGetLastError(), "slot_map_kernel launch");
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
    if (Nt < 1 || Nt > 4) return fail(LDPC5G_ESIZE, "Nt=%d outside 1..4", Nt);
    if (!ports) return fail(LDPC5G_ESIZE, "ports is null");
    SlotDmrs c{};
    GoldSeq q{};
    for (int p = 0; p < Nt; ++p) {
        if (ports[p] < 0 || ports[p] > 3) return fail(LDPC5G_ESIZE, "ports[%d]=%d: port 1000..1003 as 0..3", p, ports[p]);
        for (int o = 0; o < p; ++o)
            if (ports[o] == ports[p]) return fail(LDPC5G_ESIZE, "ports[%d]=%d repeats ports[%d]", p, ports[p], o);
        c.port[p] = ports[p];
    }
    int rc = check_dmrs(c, T, carrier_re, rb_start, rb_size, S, sym_idx);
    if (!rc) rc = check_gold(c, q, nNIDnSCID, nSCID, num_cdm_groups);
    if (rc) return rc;
    return run_frontend(c, q, grid, ldgrid, in_dtype, slots, T, Nr, Nt, h_ls, ldh, y, ldy, stream);
}

int ldpc5g_slot_map(const void* sym, int64_t ldsym, const int32_t* re_idx, int64_t nre, const int32_t* slots,
                    int32_t T, int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t num_ant, int32_t NL,
                    const float* precoding, int32_t S, const int32_t* sym_idx, int32_t nNIDnSCID, int32_t nSCID,
                    int32_t num_cdm_groups, void* grid, int64_t ldgrid, void* stream) {
    clear_error();
    if (NL < 1 || NL > 4) return fail(LDPC5G_ESIZE, "NL=%d outside 1..4", NL);
    SlotDmrs c{};
    GoldSeq q{};
    int rc = check_dmrs(c, T, carrier_re, rb_start, rb_size, S, sym_idx);
    if (!rc) rc = check_gold(c, q, nNIDnSCID, nSCID, num_cdm_groups);
    if (rc) return rc;
    return run_map(c, q, sym, ldsym, re_idx, nre, slots, T, num_ant, NL, precoding, grid, ldgrid, stream);
}

int ldpc5g_slot_rx_frontend_tp(const void* grid, int64_t ldgrid, int32_t in_dtype, const int32_t* slots, int32_t T,
                               int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t Nr, int32_t port,
                               int32_t S, const int32_t* sym_idx, int32_t nPuschID, int32_t hopping,
                               const void* base_seq, void* h_ls, int64_t ldh, void* y, int64_t ldy, void* stream) {
    clear_error();
    SlotDmrs c{};
    LowPaprSeq q{};
    int rc = check_dmrs(c, T, carrier_re, rb_start, rb_size, S, sym_idx);
    if (!rc) rc = check_low_papr(c, q, port, nPuschID, hopping, base_seq);
    if (rc) return rc;
    return run_frontend(c, q, grid, ldgrid, in_dtype, slots, T, Nr, 1, h_ls, ldh, y, ldy, stream);
}

int ldpc5g_slot_map_tp(const void* sym, int64_t ldsym, const int32_t* re_idx, int64_t nre, const int32_t* slots,
                       int32_t T, int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t num_ant, int32_t port,
                       const float* precoding, int32_t S, const int32_t* sym_idx, int32_t nPuschID, int32_t hopping,
                       const void* base_seq, void* grid, int64_t ldgrid, void* stream) {
    clear_error();
    SlotDmrs c{};
    LowPaprSeq q{};
    int rc = check_dmrs(c, T, carrier_re, rb_start, rb_size, S, sym_idx);
    if (!rc) rc = check_low_papr(c, q, port, nPuschID, hopping, base_seq);
    if (rc) return rc;
    return run_map(c, q, sym, ldsym, re_idx, nre, slots, T, num_ant, 1, precoding, grid, ldgrid, stream);
}

}  // extern "C"
