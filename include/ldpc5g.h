/*
 * ldpc5g.h — C ABI of the MI355X-native 5G NR LDPC engine (libldpc5g.so, gfx950).
 *
 * The engine replaces the hot path of the reference py5gphy/ldpc package:
 *   ldpc5g_encode        <- py5gphy/ldpc/nr_ldpc_encode.py:8     encode_ldpc(ck, bgn)
 *                           (+ _gen_ldpc_parity_bit :52-115), batched over codeblocks
 *   ldpc5g_decode_ms     <- py5gphy/ldpc/nr_ldpc_decode.py:11    nr_decode_ldpc(LLRin, Zc, bgn, L,
 *                           'min-sum', alpha, beta) and decode_ldpc :51-143 / _min_sum_process
 *                           :178-227, batched over codeblocks
 *   ldpc5g_decode_ms_mixed  the same over a batch of codeblocks with per-codeblock (bgn, Zc),
 *                           the shape DLSCHDecode (py5gphy/nr_pdsch/nr_dlsch_decode.py:62-91)
 *                           and ULSCH_decoding (py5gphy/nr_pusch/nr_ulsch_decode.py:92) feed
 *   ldpc5g_find_ils      <- py5gphy/ldpc/ldpc_info.py:81         find_iLS(Zc)
 *
 * Conventions
 *   - All buffer pointers are DEVICE pointers (hipMalloc / torch tensors); the library never
 *     allocates or frees caller buffers.  `stream` is a hipStream_t (NULL = default stream).
 *   - Bits are int8 per bit (0/1, -1 = filler), LLRs are log(P0/P1) (positive => bit 0).
 *   - Calls are asynchronous on `stream` and reentrant; ldpc5g_last_error() is thread-local.
 *   - Return 0 on success, or a negative code: the Python host maps them to AssertionError,
 *     as the reference's `assert` checks (nr_ldpc_encode.py:18,29; nr_ldpc_decode.py:23-37).
 */
#ifndef LDPC5G_H
#define LDPC5G_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC5G_OK 0
#define LDPC5G_EBGN (-1)   /* bgn not in {1,2}                                 */
#define LDPC5G_EZC (-2)    /* Zc not a TS 38.212 lifting size (find_iLS == 255) */
#define LDPC5G_ESIZE (-3)  /* bad batch / stride / L / dtype / schedule        */
#define LDPC5G_EHIP (-4)   /* HIP runtime error (launch failure)               */

/* LLR element types */
#define LDPC5G_F64 0       /* float64: bit-exact with the reference's numpy float64 decoder */
#define LDPC5G_F32 1       /* float32 */

/* decode flags */
#define LDPC5G_LLR_FULL 1  /* LLR rows hold all Nf = 68Zc/52Zc columns, the 2Zc punctured ones
                              included (decode_ldpc(LLRin, H, ...) input, nr_ldpc_decode.py:51) */
#define LDPC5G_RATE_MATCHED 2  /* LLR rows come from rate recovery (nr_ldpc_raterecover.py:6-65):
                              extension columns that were never transmitted hold +0.0.  The
                              decoder detects rows whose extension column is +0.0 in every
                              codeblock of a workgroup and skips their (provably null) updates;
                              results are bit-identical to the plain decode.  Ignored by launches
                              of <= 64 codeblock slots (one small codeblock) and by BF / BP. */

/* decoding schedules */
#define LDPC5G_FLOODING 0  /* the reference's two-phase (Jacobi) schedule, nr_ldpc_decode.py:105-131 */
#define LDPC5G_LAYERED 1   /* row-block serial schedule (perf mode, float32 only)                  */

/* Lifting-set index 0..7 of Zc (TS 38.212 Table 5.3.2-1), 255 if Zc is not a lifting size. */
int ldpc5g_find_ils(int32_t Zc);

/* Encode B codeblocks.
 *   ck : [B][ldk] int8, first K = 22*Zc (bgn 1) / 10*Zc (bgn 2) entries used, values 0/1/-1
 *   dn : [B][ldn] int8, first N = 66*Zc / 50*Zc entries written:
 *        dn[0:K-2Zc] = ck[2Zc:K] (fillers stay -1), dn[K-2Zc:N] = parity bits.
 *   Parity treats ck[k] = -1 (k >= 2Zc) as 0, exactly as the reference zeroes fillers before
 *   encoding.  ck is not modified (the reference's in-place filler zeroing is done host-side). */
int ldpc5g_encode(const int8_t* ck, int8_t* dn, int32_t B, int32_t bgn, int32_t Zc,
                  int64_t ldk, int64_t ldn, void* stream);

/* Min-sum decode (MS / normalized alpha<1 / offset beta>0 / mixed) of B codeblocks.
 *   llr    : [B][ldl] of llr_dtype, N = 66*Zc / 50*Zc entries (2*Zc systematic bits punctured,
 *            decoded with LLR 0), or Nf = 68*Zc / 52*Zc entries when flags & LDPC5G_LLR_FULL
 *   ck     : [B][ldc] int8, Nf = 68*Zc / 52*Zc hard decisions written (blkandcrc = ck[0:K])
 *   status : [B] uint8, 1 iff ck satisfies every parity check
 *   iters  : [B] int32, check-node updates performed (flooding: the reference's loop index at
 *            its early return, else L; layered: iterations run)
 *   schedule LDPC5G_FLOODING works with F64 (bit-exact with the reference) and F32;
 *   LDPC5G_LAYERED requires F32.
 *   The codeblocks sharing a workgroup (up to 768 / Zc of them) are addressed with 32-bit byte
 *   offsets: G * ldl * sizeof(element) >= 4 GiB returns LDPC5G_ESIZE (an ldl of 2^26 or more). */
int ldpc5g_decode_ms(const void* llr, int32_t llr_dtype, int8_t* ck, uint8_t* status,
                     int32_t* iters, int32_t B, int32_t bgn, int32_t Zc, int32_t L,
                     double alpha, double beta, int32_t schedule, int32_t flags, int64_t ldl,
                     int64_t ldc, void* stream);

/* Per-codeblock drop-in shape, HOST buffers in and out  <- py5gphy/ldpc/nr_ldpc_decode.py:11-49
 * nr_decode_ldpc(LLRin, Zc, bgn, L, 'min-sum', alpha, beta) and nr_ldpc_encode.py:8 encode_ldpc(ck,
 * bgn), called one codeblock at a time by the reference's callers (nr_dlsch_decode.py:91,
 * scripts/internal/sim_ldpc_internal.py:50-58).  float64 flooding min-sum (bit-exact with the
 * reference) / the encoder on B contiguous host rows (llr [B][N or Nf], ck [B][Nf], status [B],
 * iters [B]; ck [B][K], dn [B][N]): the rows go through a pinned staging buffer and a device
 * buffer kept per thread AND per device ordinal (< 64; grown on demand and held for the life of
 * the process, so a thread that alternates devices reuses each device's pair), one H2D copy,
 * the kernel, one D2H copy and one synchronisation of `stream` — no caller-side device memory.
 * Synchronous: returns when the outputs are written.  beta < 0 is rejected (see decode_sparse). */
int ldpc5g_decode_ms_host(const double* llr, int8_t* ck, uint8_t* status, int32_t* iters,
                          int32_t B, int32_t bgn, int32_t Zc, int32_t L, double alpha, double beta,
                          int32_t flags, void* stream);
int ldpc5g_encode_host(const int8_t* ck, int8_t* dn, int32_t B, int32_t bgn, int32_t Zc,
                       void* stream);

/* Hard-decision bit flipping (algo='BF')  <- py5gphy/ldpc/ldpc_decoder_bit_flipping.py:5-73
 * reached through nr_decode_ldpc(..., algo='BF') (nr_ldpc_decode.py:65-67).  Same buffers as
 * ldpc5g_decode_ms; ck holds the 0/1 decisions (the reference returns them as float64), status
 * is 0 after L iterations without a zero syndrome (the reference checks only at loop start). */
int ldpc5g_decode_bf(const void* llr, int32_t llr_dtype, int8_t* ck, uint8_t* status,
                     int32_t* iters, int32_t B, int32_t bgn, int32_t Zc, int32_t L,
                     int32_t flags, int64_t ldl, int64_t ldc, void* stream);

/* Float64 sum-product, flooding (algo='BP')  <- nr_ldpc_decode.py:51-143 + _BP_process :145-176.
 * Per-edge messages do not compress: the caller provides a float64 device scratch of
 * ldpc5g_bp_scratch_elems(B, bgn, Zc) elements (-1 on bad arguments). */
int64_t ldpc5g_bp_scratch_elems(int32_t B, int32_t bgn, int32_t Zc);
int ldpc5g_decode_bp(const double* llr, int8_t* ck, uint8_t* status, int32_t* iters,
                     double* scratch, int64_t scratch_elems, int32_t B, int32_t bgn, int32_t Zc,
                     int32_t L, int32_t flags, int64_t ldl, int64_t ldc, void* stream);

/* ---- arbitrary parity-check matrix  <- py5gphy/ldpc/nr_ldpc_decode.py:51-143 decode_ldpc(LLRin, H,
 * L, algo, alpha, beta) for ANY binary H (the 38.212 expansions have the specialised entry points
 * above).  H is passed as a CSR of its rows plus a CSC of its columns (DEVICE int32 arrays):
 *   row_ptr [M+1], col_idx [E]   edges of row m = col_idx[row_ptr[m] .. row_ptr[m+1]), columns
 *                                ascending (np.where(H[m,:] == 1), :80-83); edges numbered row-major
 *   col_ptr [N+1], col_edge [E], col_row [E]   entries of column n, rows ascending (np.where(
 *                                H[:,n] == 1), :88-91): the edge id and its row
 * algo LDPC5G_ALGO_MS: the min-sum family with the reference's zero-count branches (:178-227), any
 * beta; LDPC5G_ALGO_BP: sum-product (:145-176); LDPC5G_ALGO_BF: bit flipping
 * (ldpc_decoder_bit_flipping.py:5-73).  All float64, flooding, B codeblocks of N LLRs each:
 *   llr [B][ldl] float64, ck [B][ldc] int8 (N decisions), status [B] uint8, iters [B] int32.
 * A min-sum row of degree < 2 makes the reference raise (np.sort(...)[1]) once a check-node update
 * runs; the kernel computes on, and the Python host raises the reference's error from iters/status.
 * Per-codeblock state lives in LDS when it fits (ldpc5g_sparse_scratch_bytes returns 0), else in
 * a caller DEVICE scratch of ldpc5g_sparse_scratch_bytes(B, M, N, E, algo) bytes (-1: bad args). */
#define LDPC5G_ALGO_MS 0
#define LDPC5G_ALGO_BP 1
#define LDPC5G_ALGO_BF 2
int64_t ldpc5g_sparse_scratch_bytes(int32_t B, int32_t M, int32_t N, int32_t E, int32_t algo);
int ldpc5g_decode_sparse(const double* llr, int64_t ldl, int32_t B, int32_t M, int32_t N, int32_t E,
                         const int32_t* row_ptr, const int32_t* col_idx, const int32_t* col_ptr,
                         const int32_t* col_edge, const int32_t* col_row, int32_t L, int32_t algo,
                         double alpha, double beta, int8_t* ck, int64_t ldc, uint8_t* status,
                         int32_t* iters, void* scratch, int64_t scratch_bytes, void* stream);

/* One codeblock of a mixed batch: base graph, lifting size, element offsets of its LLR row
 * (into llr_base, in elements) and of its ck row (into ck_base, in bytes). */
typedef struct {
    int32_t bgn;
    int32_t Zc;
    int64_t llr_off;
    int64_t ck_off;
} ldpc5g_cb_desc_t;

/* Decode a batch of codeblocks with heterogeneous (bgn, Zc) in at most two launches (one per
 * base graph).  `desc` is a HOST array of B descriptors; status[b] / iters[b] follow desc order.
 * The work list is built on the host and copied into a stream-ordered allocation
 * (hipMallocAsync / hipFreeAsync on `stream`) from a per-thread pool of pinned staging buffers:
 * the call returns once the copy is queued.  The pool grows with the plans in flight (a slot is
 * reused once its copy has completed) up to 64 slots per thread, and only past 64 plans in flight
 * does a call wait for the oldest copy.  The pool's pinned memory is held by each calling thread
 * for the life of the process (about the size of its largest plans).  Repeated decodes of one batch shape should build the
 * plan once instead (ldpc5g_mixed_plan + ldpc5g_decode_ms_mixed_plan). */
int ldpc5g_decode_ms_mixed(const ldpc5g_cb_desc_t* desc, int32_t B, const void* llr_base,
                           int32_t llr_dtype, int8_t* ck_base, uint8_t* status, int32_t* iters,
                           int32_t L, double alpha, double beta, int32_t schedule,
                           int32_t flags, void* stream);

/* Build the work list (plan) of a mixed batch into the caller's HOST buffer `plan` (pinned memory
 * recommended, `plan_bytes` long).  Returns the plan size in bytes (>= 0; the buffer is untouched
 * when it is too small, so a first call with plan_bytes = 0 sizes it) or a negative error.  The
 * plan depends only on (desc, B, schedule).  Layout (opaque to callers): a 32-byte header, the
 * workgroups of each base graph by lifting size (BG1 Zc = 384 last, a partly filled workgroup
 * before the full ones), the codeblock references (sorted by llr_off within a workgroup: the
 * kernels address a workgroup's rows from its lowest one with 32-bit offsets, so the rows of the
 * codeblocks packed together — same (bgn, Zc), consecutive in desc order — must span < 4 GiB,
 * else LDPC5G_ESIZE). */
int64_t ldpc5g_mixed_plan(const ldpc5g_cb_desc_t* desc, int32_t B, int32_t schedule, void* plan,
                          int64_t plan_bytes);

/* Decode with a plan the caller copied to the device (`plan_dev`, the bytes ldpc5g_mixed_plan
 * wrote, on this stream's device): <= 2 launches, nothing else — no allocation, no copy, no
 * synchronisation.  schedule must be the one the plan was built for. */
int ldpc5g_decode_ms_mixed_plan(const void* plan_dev, const void* plan_host, const void* llr_base,
                                int32_t llr_dtype, int8_t* ck_base, uint8_t* status,
                                int32_t* iters, int32_t L, double alpha, double beta,
                                int32_t schedule, int32_t flags, void* stream);

/* ============================================================ DL-SCH / UL-SCH transport chain
 * TS 38.212 §7.2 (DL-SCH) / §6.2 (UL-SCH) around the codec, batched over T transport blocks that
 * share one configuration.  Bits are int8 0/1 (fillers -1); CRC remainders are uint32 with the
 * first CRC bit in bit L-1.  */

/* CRC generator ids (py5gphy/crc/crc.py:94-106) */
#define LDPC5G_CRC6 0
#define LDPC5G_CRC11 1
#define LDPC5G_CRC16 2
#define LDPC5G_CRC24A 3
#define LDPC5G_CRC24B 4
#define LDPC5G_CRC24C 5

/* CRC of `rows` bit rows ([rows][ld] int8, nbits each): rem[r] = M(x) x^L mod g(x), the parity
 * nr_crc_encode appends (crc.py:4-41, mask 0, bit L-1 first); a row that ends in its own CRC gives
 * 0 iff nr_crc_decode reports no error (crc.py:43-88).  rem must not alias bits. */
int ldpc5g_crc(const int8_t* bits, int64_t ld, int64_t nbits, int32_t rows, int32_t poly,
               uint32_t* rem, void* stream);

/* Shared-configuration geometry of a transport block (host struct, filled by ldpc5g_sch_config). */
typedef struct {
    int32_t A;            /* TBSize                                                           */
    int32_t B;            /* A + TB CRC length                                                */
    int32_t tb_crc_poly;  /* LDPC5G_CRC24A (A > 3824) or LDPC5G_CRC16 (nr_dlsch.py:34-40)      */
    int32_t bgn;          /* base graph (nr_dlsch.py:44-49)                                   */
    int32_t C, cbz, Lcb, F, K, K_apo, Zc;   /* get_cbs_info (ldpc_info.py:5-78); K_apo = cbz+Lcb */
    int32_t N, Ncb, k0;   /* codeword length, circular buffer (Nref / N), rv start             */
    int32_t Qm, NL, rv;
    int32_t E_lo, E_hi, c_switch;   /* Er: codeblocks c < c_switch get E_lo, the others E_hi    */
    int64_t G;            /* the G that sized Er (nr_ldpc_ratematch.py:5-27)                   */
    int64_t E_total;      /* sum of Er = bits of g per transport block                         */
} ldpc5g_sch_cfg_t;

/* Fill cfg for a transport block: TBSize A, modulation order Qm, code rate * 1024, layers NL,
 * redundancy version rv, TBS_LBRM (> 0: DL-SCH limited buffer Nref = floor(TBS_LBRM / (2C/3)),
 * nr_dlsch.py:63-65; 0: UL-SCH Ncb = N, nr_ulsch.py:55-58) and G (rate-matching output bits).
 * Float arithmetic of the reference (base-graph thresholds, k0, Er) is reproduced in double. */
int ldpc5g_sch_config(int32_t A, int32_t Qm, double coderateby1024, int32_t NL, int32_t rv,
                      int64_t TBS_LBRM, int64_t G, ldpc5g_sch_cfg_t* cfg);

/* DLSCHEncode (py5gphy/nr_pdsch/nr_dlsch.py:12-74) / ULSCH_Crc_CodeBlockSegment +
 * ULSCH_encoding_ratematch (nr_pusch/nr_ulsch.py:13-70) of T transport blocks:
 *   trblk [T][lda] int8 -> g [T][ldg] int8 (E_total bits each).
 * Workspaces (device, caller-owned): ck [T*C][K] int8 (codeblocks with CRC24B and -1 fillers,
 * as ldpc_cbsegment returns them), dn [T*C][N] int8 (encoder output), tb_crc [T] uint32 (the
 * TB CRC, also an output). */
int ldpc5g_sch_encode(const int8_t* trblk, int64_t lda, int8_t* g, int64_t ldg,
                      const ldpc5g_sch_cfg_t* cfg, int32_t T, int8_t* ck, int8_t* dn,
                      uint32_t* tb_crc, void* stream);

/* The two halves of ldpc5g_sch_encode:
 *   ldpc5g_sch_segment   TB CRC + codeblock segmentation + CRC24B (nr_dlsch.py:32-56,
 *                        ULSCH_Crc_CodeBlockSegment nr_ulsch.py:13-35): trblk -> ck, tb_crc
 *   ldpc5g_sch_ratematch LDPC encode + rate matching + concatenation (nr_dlsch.py:58-74,
 *                        ULSCH_encoding_ratematch nr_ulsch.py:37-70): ck -> dn -> g
 * ldpc5g_sch_ratematch reads only the codeblock fields of cfg (bgn, C, cbz, Lcb, K, K_apo, Zc,
 * N, Ncb, k0, Qm, E_lo, E_hi, c_switch). */
int ldpc5g_sch_segment(const int8_t* trblk, int64_t lda, const ldpc5g_sch_cfg_t* cfg, int32_t T,
                       int8_t* ck, uint32_t* tb_crc, void* stream);
int ldpc5g_sch_ratematch(const int8_t* ck, const ldpc5g_sch_cfg_t* cfg, int32_t T, int8_t* dn,
                         int8_t* g, int64_t ldg, void* stream);

/* Rate recovery (nr_ldpc_raterecover.py:6-65) of every codeblock + optional HARQ combining with
 * the previous decoder inputs (nr_dlsch_decode.py:73-88):
 *   llr [T][ldg] (llr_dtype) -> llr_dn [T*C][N] (dn_dtype); harq_in NULL or [T*C][N] dn_dtype,
 *   either disjoint from llr_dn or llr_dn itself (in-place combining with the previous call's
 *   output); a partial overlap is not supported.  (Every rate-recovery entry point below too.)
 * Computed in float64 like the reference (a float32 llr_dn is the float64 result rounded once). */
int ldpc5g_sch_raterecover(const void* llr, int32_t llr_dtype, int64_t ldg,
                           const ldpc5g_sch_cfg_t* cfg, int32_t T, const void* harq_in,
                           void* llr_dn, int32_t dn_dtype, void* stream);

/* TB reassembly and CRC checks (nr_dlsch_decode.py:93-106): ck [T*C][ldc] int8 hard decisions
 * -> tbblk [T][ldb] int8 (B = A + CRC bits: the TB and its CRC), cb_crc_ok [T*C] (CRC24B when
 * C > 1, else 1), tb_ok [T] (TB CRC), tb_rem [T] uint32 (TB CRC remainder, scratch + output). */
int ldpc5g_sch_tb_check(const int8_t* ck, int64_t ldc, const ldpc5g_sch_cfg_t* cfg, int32_t T,
                        int8_t* tbblk, int64_t ldb, uint8_t* cb_crc_ok, uint32_t* tb_rem,
                        uint8_t* tb_ok, void* stream);

/* DLSCHDecode (nr_dlsch_decode.py:13-110) / ULSCH_decoding (nr_ulsch_decode.py:13-110) with the
 * min-sum decoder: ldpc5g_sch_raterecover -> ldpc5g_decode_ms over the T*C codeblocks (ck
 * [T*C][Nf], status / iters [T*C]) -> ldpc5g_sch_tb_check.  Asynchronous on `stream`. */
int ldpc5g_sch_decode(const void* llr, int32_t llr_dtype, int64_t ldg, const ldpc5g_sch_cfg_t* cfg,
                      int32_t T, const void* harq_in, void* llr_dn, int32_t dn_dtype, int8_t* ck,
                      uint8_t* status, int32_t* iters, int32_t L, double alpha, double beta,
                      int32_t schedule, int8_t* tbblk, int64_t ldb, uint8_t* cb_crc_ok,
                      uint32_t* tb_rem, uint8_t* tb_ok, void* stream);

/* ---- transport blocks with per-TB configurations (the reference configures every TB of a slot
 * independently: nr_pdsch.py:212-281 -> DLSCHDecode at :281, nr_dlsch.py:12-74 per TB).
 * cfgs[T] (host, each from ldpc5g_sch_config); TB t's codeblocks occupy consecutive rows of the
 * flat workspaces, TB after TB: ck rows of K_t, dn / llr_dn rows of N_t, decoder ck rows of
 * Nf_t = 68/52 Zc_t, status / iters / cb_crc_ok one entry per codeblock.  trblk [T][lda] (A_t
 * bits used), g / llr [T][ldg] (E_total_t used), tbblk [T][ldb] (B_t used).
 * sizes[7] = {ck elements, dn elements, decoder-ck elements, codeblocks, max A, max B, max E}.
 * The per-TB geometry goes to the device like the mixed-Zc work list (stream-ordered allocation,
 * pinned staging pool: see ldpc5g_decode_ms_mixed). */
int ldpc5g_sch_multi_sizes(const ldpc5g_sch_cfg_t* cfgs, int32_t T, int64_t* sizes);
int ldpc5g_sch_encode_multi(const int8_t* trblk, int64_t lda, int8_t* g, int64_t ldg,
                            const ldpc5g_sch_cfg_t* cfgs, int32_t T, int8_t* ck, int8_t* dn,
                            uint32_t* tb_crc, void* stream);
/* rate recovery alone (raterecover_ldpc, py5gphy/ldpc/nr_ldpc_raterecover.py:6-65, + HARQ) of every
 * codeblock of the T transport blocks in ONE launch, into the flat llr_dn rows (N_t per codeblock,
 * TB after TB): the input of a mixed-Zc decode (ldpc5g_decode_ms_mixed_plan). */
int ldpc5g_sch_raterecover_multi(const void* llr, int32_t llr_dtype, int64_t ldg,
                                 const ldpc5g_sch_cfg_t* cfgs, int32_t T, const void* harq_in,
                                 void* llr_dn, int32_t dn_dtype, void* stream);
/* The same with the geometry built once: ldpc5g_sch_multi_plan writes the plan's host bytes (returns
 * the size needed; call with plan = NULL first), the caller copies them to device memory once, and
 * every ldpc5g_sch_raterecover_multi_plan(plan_dev, plan_host, ...) only launches (no host-side
 * validation, allocation or copy per call; asynchronous on `stream`). */
int64_t ldpc5g_sch_multi_plan(const ldpc5g_sch_cfg_t* cfgs, int32_t T, void* plan, int64_t plan_bytes);
int ldpc5g_sch_raterecover_multi_plan(const void* plan_dev, const void* plan_host, const void* llr,
                                      int32_t llr_dtype, int64_t ldg, const void* harq_in, void* llr_dn,
                                      int32_t dn_dtype, void* stream);
/* decode: rate recovery (+ HARQ, harq_in laid out like llr_dn) -> mixed-Zc min-sum decode of all
 * codeblocks (ldpc5g_decode_ms_mixed) -> TB reassembly + CRCs.  Asynchronous on `stream`. */
int ldpc5g_sch_decode_multi(const void* llr, int32_t llr_dtype, int64_t ldg,
                            const ldpc5g_sch_cfg_t* cfgs, int32_t T, const void* harq_in,
                            void* llr_dn, int32_t dn_dtype, int8_t* ck, uint8_t* status,
                            int32_t* iters, int32_t L, double alpha, double beta, int32_t schedule,
                            int8_t* tbblk, int64_t ldb, uint8_t* cb_crc_ok, uint32_t* tb_rem,
                            uint8_t* tb_ok, void* stream);

/* ================================================ scrambling, modulation, soft demodulation
 * The symbol-level steps either side of the DL-SCH chain (TS 38.211 5.2.1, 5.1, 7.3.1.1-2),
 * batched over T transport blocks with one scrambling init each.  Packed bit words: bit k of
 * word w = element 32w + k. */

/* gen_nrPRBS (py5gphy/common/nrPRBS.py:5-25) of every TB: words [T][ldw] uint32 receive
 * c(0 .. nbits-1) for c_init = cinit[t] (cinit: DEVICE array of T values). */
int ldpc5g_prbs(const uint32_t* cinit, int32_t T, int64_t nbits, uint32_t* words, int64_t ldw,
                void* stream);

/* Modulation ids: the order Qm for QPSK..1024QAM, 1 for BPSK and LDPC5G_PI2_BPSK for pi/2-BPSK
 * (nrModulation.py:14-42 / nr_Demodulation.py:30-43 accept all seven). */
#define LDPC5G_PI2_BPSK (-1)

/* Scrambling + modulation mapper (nr_pdsch_process.py:17-25, nrModulation.py:4-42), mod = 1, -1,
 * 2, 4, 6, 8, 10: bits [T][ldb] int8 (nbits each, a multiple of Qm) XOR prbs words (NULL: no
 * scrambling) -> complex64 symbols [T][ldsym] (float2), bit-exact with the reference's float32
 * arithmetic (pi/2-BPSK: odd symbol index within each row rotated, :17-21). */
int ldpc5g_scramble_modulate(const int8_t* bits, int64_t ldb, const uint32_t* prbs, int64_t ldw,
                             int32_t T, int64_t nbits, int32_t mod, void* sym, int64_t ldsym,
                             void* stream);

/* Soft demodulation (nr_Demodulation.py:12-46, demod_{bpsk,pi2_bpsk,qpsk,16qam,64qam,256qam,
 * 1024qam}.py) + LLR descrambling (nr_pdsch.py:268-274): symbols [T][ldsym] complex64
 * (sym_dtype LDPC5G_F32) or complex128 (LDPC5G_F64), noise variances [T][ldnv] float32 -> LLRs
 * [T][ldllr] (nsym*Qm each), multiplied by 1 - 2c(n) when prbs is not NULL.  The arithmetic
 * follows the reference's operation order in the symbols' precision: float64 for complex128;
 * float32 for complex64 with every constant (k*A, c*A, threshold*A) rounded to float32 first, as
 * numpy >= 2 evaluates demod_*.py then.  llr_dtype LDPC5G_F32 always works; LDPC5G_F64 is accepted
 * for BPSK on complex128 input, whose reference LLRs are float64 (demod_bpsk.py:9). */
int ldpc5g_demod_descramble(const void* sym, int32_t sym_dtype, int64_t ldsym,
                            const float* noise_var, int64_t ldnv, const uint32_t* prbs,
                            int64_t ldw, int32_t T, int64_t nsym, int32_t mod, void* llr,
                            int32_t llr_dtype, int64_t ldllr, void* stream);

/* ---- fused receive front end: symbols in, rate-recovered LLRs (or the decoded TB) out.
 * The receive chain of a transport block (nr_pdsch.py:245-281 -> nr_dlsch_decode.py:62-106;
 * UL-SCH: nr_pusch.py:194 -> nr_ulsch_decode.py:63-89) demodulates (nr_Demodulation.py:12-46), descrambles
 * (nr_pdsch.py:268-274), then rate-recovers every codeblock (nr_ldpc_raterecover.py:25-64) and
 * combines it with the HARQ buffer (nr_dlsch_decode.py:73-88).  ldpc5g_sch_demod_raterecover does
 * all of that in ONE launch: the workgroup of a codeblock demodulates the codeblock's own E/Qm
 * symbols into LDS and rate-recovers from there, so the demodulated LLRs never go to memory.  The
 * result is, bit for bit, ldpc5g_demod_descramble followed by ldpc5g_sch_raterecover:
 *   sym [T][ldsym] complex64 (sym_dtype LDPC5G_F32) / complex128 (LDPC5G_F64) and noise_var
 *   [T][ldnv] float32, nsym = cfg->E_total / cfg->Qm of each used; prbs NULL (no descrambling) or
 *   the packed words [T][ldw] of ldpc5g_prbs (>= E_total bits); mod as ldpc5g_demod_descramble, with
 *   |mod| == cfg->Qm (mod distinguishes BPSK from pi/2-BPSK, whose odd/even rule follows the
 *   symbol's index in the TB row, demod_pi2_bpsk.py:11-12); harq_in / llr_dn / dn_dtype as
 *   ldpc5g_sch_raterecover (harq_in may be llr_dn itself).
 * The demodulated LLRs are float32 as nr_Demodulation.py stores them — float64 for BPSK on
 * complex128 symbols (demod_bpsk.py:9 stores nothing).  A configuration with a codeblock whose E
 * LLRs exceed the 64 KiB LDS stage (ldpc5g_sch_rx_scratch_elems != 0) needs llr_ws: scratch
 * [T][ldws] of that LLR type, ldws >= E_total, through which the call runs the two separate
 * kernels (same result); without it the call fails with LDPC5G_ESIZE.  llr_ws may be NULL
 * otherwise.  Asynchronous on `stream`. */
int ldpc5g_sch_demod_raterecover(const void* sym, int32_t sym_dtype, int64_t ldsym,
                                 const float* noise_var, int64_t ldnv, const uint32_t* prbs,
                                 int64_t ldw, int32_t mod, const ldpc5g_sch_cfg_t* cfg, int32_t T,
                                 const void* harq_in, void* llr_dn, int32_t dn_dtype, void* llr_ws,
                                 int64_t ldws, void* stream);
/* Elements per TB row of the llr_ws scratch the configuration needs (E_total), 0 when every
 * codeblock fits the stage, or a negative error code.  No reference counterpart. */
int64_t ldpc5g_sch_rx_scratch_elems(const ldpc5g_sch_cfg_t* cfg, int32_t mod, int32_t sym_dtype);
/* The receive chain from symbols to transport block (nr_pdsch.py:245-281 -> DLSCHDecode
 * nr_dlsch_decode.py:13-110 / ULSCH_decoding nr_ulsch_decode.py:13-110) with the min-sum decoder:
 * ldpc5g_sch_demod_raterecover -> ldpc5g_decode_ms -> ldpc5g_sch_tb_check, chained as in
 * ldpc5g_sch_decode (same ck / status / iters / tbblk / cb_crc_ok / tb_rem / tb_ok).
 * Asynchronous on `stream`. */
int ldpc5g_sch_rx_decode(const void* sym, int32_t sym_dtype, int64_t ldsym, const float* noise_var,
                         int64_t ldnv, const uint32_t* prbs, int64_t ldw, int32_t mod,
                         const ldpc5g_sch_cfg_t* cfg, int32_t T, const void* harq_in, void* llr_dn,
                         int32_t dn_dtype, void* llr_ws, int64_t ldws, int8_t* ck, uint8_t* status,
                         int32_t* iters, int32_t L, double alpha, double beta, int32_t schedule,
                         int8_t* tbblk, int64_t ldb, uint8_t* cb_crc_ok, uint32_t* tb_rem,
                         uint8_t* tb_ok, void* stream);

/* ================================================ linear MIMO equalisation (before the chain)
 * The producer of the `sym` / `noise_var` arguments above: the four linear algorithms of
 * channel_equ_and_demod (py5gphy/channel_equalization/nr_channel_eq.py:12-50), which the
 * reference calls once per resource element (RE) from the double loop of Pdsch.RX_process
 * (nr_pdsch.py:245-263) and its PUSCH twin (nr_pusch.py:147-165), batched over the data REs of T
 * transport blocks in one launch, one thread per RE. */
#define LDPC5G_EQ_ZF 0        /* ZF.py:47-79   */
#define LDPC5G_EQ_ZF_IRC 1    /* ZF.py:5-45    */
#define LDPC5G_EQ_MMSE 2      /* MMSE.py:58-103 */
#define LDPC5G_EQ_MMSE_IRC 3  /* MMSE.py:5-56  */
/* Layout, per transport block t (row strides ld* in COMPLEX elements):
 *   y   [t][r][Nr]                    received vector of RE r
 *   h   [t][r][Nr][NL]                channel estimate of RE r
 *   cov [t][r / re_per_cov][Nr][Nr]   noise-interference covariance of the block of RE r
 * r = 0..R-1 is the flat RE index m*RE_num + re of the reference's loops; re_per_cov = 12
 * reproduces its prb = re // 12 (RE_num is a multiple of 12).  re_idx: nre ascending flat indices
 * of the data REs (the pdsch_RE_usage == 0 positions), shared by the T blocks, or NULL for all R
 * (then nre must equal R).  An index outside 0..R-1 reads nothing and yields NaN outputs.
 * in_dtype LDPC5G_F64: complex128 in, complex128 symbols out; LDPC5G_F32: complex64 storage in
 * and out.  The arithmetic is float64 in both cases (the kernel is memory-bound, and a float32
 * inversion loses the result at the condition numbers MIMO channels reach): the complex64 result
 * is, bit for bit, the complex128 result on the widened inputs rounded to complex64.  Noise
 * variances are always float32, as nr_Demodulation.py:24 casts them.
 * Output: sym[t][i*NL + l] and noise_var[t][i*NL + l] for data RE i and layer l — the
 * de-layer-mapped order in which RX_process concatenates its LLRs, i.e. the sym / noise_var of
 * ldpc5g_demod_descramble, ldpc5g_sch_demod_raterecover and ldpc5g_sch_rx_decode with
 * nsym = nre*NL.
 * Supported: Nr in {1, 2, 4}, 1 <= NL <= Nr.  Anything else, a bad algo / in_dtype /
 * re_per_cov (< 1), a row stride shorter than its row (ldy < R*Nr, ldh < R*Nr*NL,
 * ldcov < ceil(R/re_per_cov)*Nr*Nr, ldsym or ldnv < nre*NL), nre > R, T, R or nre <= 0, or a null
 * buffer returns LDPC5G_ESIZE; all of it is checked on the host before any HIP call.
 * Formulas and operation order follow the reference: the Nr == 1 shortcut s = Y/H,
 * noise_var = Re(cov / (conj(H) H)) for all four algorithms (H == 0 gives inf / NaN where the
 * reference asserts); sigma_2 = mean of cov's diagonal; comp = 1 - diag(inv_W1), s = s_hat/comp,
 * noise_var = 1/comp - 1 for the two MMSE forms; diag(W cov W^H) for ZF-IRC.
 * cov and W1 (H^H H, H^H H / sigma_2 + I, H^H cov^-1 H + I) are Hermitian positive semidefinite,
 * and the kernel relies on it: of cov it reads only the lower triangle (row >= column) and the
 * real part of the diagonal (ZF and MMSE read the diagonal alone).
 * Regularisation.  The reference adds 0.0012 * max|A| * I to A (W1 and, in MMSE-IRC, cov) when
 * np.linalg.matrix_rank(A) < n, an SVD test with threshold n*eps*sigma_max whose outcome on nearly
 * singular input is rounding noise even in numpy.  Here A is factored by unpivoted LDL^H and is
 * regularised, then factored again, iff NOT(min_k d_k > 2^-40 * max_ij |A_ij|); the negated form
 * also catches NaN and negative pivots.  For positive semidefinite A every pivot is >= lambda_min
 * and max|A_ij| <= lambda_max, so the rule never fires when sigma_min/sigma_max >= 1e-8 and always
 * fires on exactly singular input, whose last pivot is at rounding level.  Between 2^-40 (9.1e-13)
 * and numpy's ~1e-15 the two tests may disagree; there the reference's own result has fewer than
 * three significant digits.  Asynchronous on `stream`. */
int ldpc5g_equalize(const void* y, int64_t ldy, const void* h, int64_t ldh,
                    const void* cov, int64_t ldcov, int32_t in_dtype,
                    const int32_t* re_idx, int64_t R, int64_t nre, int32_t re_per_cov,
                    int32_t T, int32_t Nr, int32_t NL, int32_t algo,
                    void* sym, int64_t ldsym, float* noise_var, int64_t ldnv, void* stream);

/* ================================================ maximum-likelihood MIMO detection
 * The second producer of the receive chain: the ML family of channel_equ_and_demod
 * (nr_channel_eq.py:27-46) emits LLRs directly, so its output feeds ldpc5g_sch_decode and bypasses
 * ldpc5g_demod_descramble.  Batched over the data REs of T transport blocks in one launch. */
#define LDPC5G_ML_SOFT 0       /* ML.py:47-98 "soft"; irc: ML.py:9-45.  LLRs by ML_soft_LLR_est, :100-139 */
#define LDPC5G_ML_HARD 1       /* ML.py:47-98 "hard": LLR = 1 - 2 bit (:93-94)                          */
#define LDPC5G_ML2_SOFT 2      /* ML2.py:47-161; irc: ML2.py:9-45.  LLR = min1 - min0 per bit (:138-160) */
#define LDPC5G_ML_MMSE 3       /* MMSE_ML.py:47-105 (subset_ML :71-105); irc: MMSE_ML.py:12-45          */
#define LDPC5G_ML_OPT_RANK2 4  /* opt_rank2_ML.py:38-171; irc: :9-36.  NL != 2 runs LDPC5G_ML_SOFT (:44) */
/* y, h, cov, in_dtype, re_idx, R, nre, re_per_cov, T, Nr, NL: exactly as ldpc5g_equalize (layouts,
 * the cov triangle that is read, NaN outputs for an index outside 0..R-1).  mod: the modulation id
 * used elsewhere; pi/2-BPSK (-1) detects as BPSK, because the reference's get_mod_list and
 * get_oppisite_syms only ever modulate symbol index 0.  irc: 0, or 1 for the -IRC form of `algo`.
 * The arithmetic is float64 for both storage types; the complex64 run is bit-equal to the
 * complex128 run on the widened inputs.
 * Per RE.  Without irc sigma^2 = Re(mean(diag(cov))).  With irc Y and H are whitened by
 * U = D^-1/2 L^-1 of the unpivoted LDL^H factorisation of cov (U^H U = cov^-1; the metric does not
 * depend on the choice of U, the reference's cov_inverse_decompose takes one from eigh) and
 * sigma^2 = 1; cov is first regularised (+ 0.0012 max|cov| I) by the pivot rule described under
 * ldpc5g_equalize, which stands in for cov_inverse_decompose's matrix_rank loop.  The metric is
 * v(S) = |Y - H S|^2 / sigma^2 over the reference's constellation (get_mod_list: float32 mapper
 * values widened; point m has the binary digits of m, MSB first, as bits).
 *   ML-soft, ML-hard, ML2-soft: all M^NL candidates in itertools.product order (layer 0 slowest);
 *     ties go to the LOWEST candidate index (the reference's strict `<`).  Cap: M^NL <= 65536, i.e.
 *     NL*Qm <= 16 (QPSK / 16QAM to NL = 4, 64QAM / 256QAM to NL = 2, 1024QAM at NL = 1).
 *   MMSE-ML: the MMSE (irc: MMSE-IRC) estimate of ldpc5g_equalize, then per layer its min(4, M)
 *     nearest points, and the search over their <= 256 combinations; no cap.
 *   opt-rank2-ML at NL = 2: the reference's O(M) loop over s0 with the per-axis choice of s1; no
 *     cap (the only search for 1024QAM on two layers).  The reference repeats the loop with the
 *     layers swapped and asserts that both agree; the result is the first loop's.
 * Outputs, for data RE i, layer l, bit m (positive LLR means bit 0):
 *   llr[t][(i*NL + l)*Qm + m], float64 (llr_dtype LDPC5G_F64, the reference's type) or float32
 *     (the float64 value rounded once); multiplied by 1 - 2 c(n) when prbs (ldpc5g_prbs words,
 *     row stride ldw) is given, as ldpc5g_demod_descramble does;
 *   sym[t][i*NL + l] complex64 or NULL: the decided point (min_S is 'c8' in the reference);
 *   noise_var[t][i*NL + l] or NULL, in llr_dtype: the minimum metric (the same for every layer);
 *   hardbits[t][(i*NL + l)*Qm + m] int8 or NULL: the decided bits.
 * Every unsupported combination (Nr, NL, mod, algo, irc, dtypes, re_per_cov < 1, NL*Qm over the
 * cap — that message names opt-rank2-ML), a row stride shorter than its row, bad sizes or a null
 * required buffer returns LDPC5G_ESIZE with a message; all of it is checked on the host before
 * any HIP call.  Asynchronous on `stream`. */
int ldpc5g_ml_detect(const void* y, int64_t ldy, const void* h, int64_t ldh,
                     const void* cov, int64_t ldcov, int32_t in_dtype,
                     const int32_t* re_idx, int64_t R, int64_t nre, int32_t re_per_cov,
                     int32_t T, int32_t Nr, int32_t NL, int32_t mod, int32_t algo, int32_t irc,
                     const uint32_t* prbs, int64_t ldw, void* llr, int32_t llr_dtype, int64_t ldllr,
                     void* sym, int64_t ldsym, void* noise_var, int64_t ldnv,
                     int8_t* hardbits, int64_t ldhb, void* stream);

/* ================================================ DMRS channel estimation (before the detectors)
 * The producer of the `h` and `cov` arguments of ldpc5g_equalize / ldpc5g_ml_detect: the four
 * CE_algo values of NrChannelEstimation.channel_est (py5gphy/channel_estimate/
 * nr_channel_estimation.py:116-126), batched over T slots, with the noise-plus-interference
 * covariance and the timing-offset estimate and compensation.  Frequency-offset estimation and
 * compensation (nr_channel_estimation.py:224-327) and the CubicSpline / PchipInterpolator
 * frequency interpolators (dft_dct_CE.py:147-152) are not provided. */
#define LDPC5G_CE_DFT 0            /* dft_dct_CE.py:10-102, model "DFT"            */
#define LDPC5G_CE_DCT 1            /* dft_dct_CE.py:10-102, model "DCT"            */
#define LDPC5G_CE_DFT_SYMMETRIC 2  /* dft_dct_symmetric_CE.py:11-118, model "DFT" */
#define LDPC5G_CE_DCT_SYMMETRIC 3  /* dft_dct_symmetric_CE.py:11-118, model "DCT" */
/* Layout, per slot t (row strides ld* in COMPLEX elements):
 *   h_ls [t][m][n][Nr][Nt]        least-squares estimate at DMRS symbol m (slot symbol sym_idx[m],
 *                                 a HOST array of S entries), reference RE n = 0..N-1, D = RE_distance
 *                                 subcarriers apart; PRB = N*D/12
 *   h    [t][s*N*D + k][Nr][Nt]   H_result, s = 0..13: ldpc5g_equalize's h with R = 14*N*D
 *   cov  [t][s*PRB + p][Nr][Nr]   cov_m: ldpc5g_equalize's cov with re_per_cov = 12
 * in_dtype LDPC5G_F64 (complex128) or LDPC5G_F32 (complex64 storage in and out).  All arithmetic
 * is float64 for both (the reference transforms complex64 data in single precision; its own
 * rounding is the floor of any comparison): the complex64 result is, bit for bit, the complex128
 * result on the widened inputs rounded to complex64.  Results are bit-identical from run to run
 * (fixed summation order, no atomics).  At most three kernel launches, asynchronous on `stream`,
 * no host synchronisation and no allocation: intermediates (float64 H_est, the residual, the
 * timing offsets) live in `work`, at least ldpc5g_ce_workspace_bytes(T, S, N, Nr, Nt, D) bytes of
 * 16-byte aligned device memory that must not be shared by calls that may run concurrently.
 * Per sequence x = h_ls[t][m][:][nr][nt] (dft_dct_CE.py:48-94, dft_dct_symmetric_CE.py:50-110):
 *   0 (to_comp != 0) timing offset: the (nr, nt) pair with the largest mean |x|^2 over (S, N), nt
 *     outer, nr inner, strict > (find_peak_H_LS, nr_channel_estimation.py:66-83); TO_est[m] =
 *     mean_n atan2(c.imag, c.real) / (2 pi D scs 1000), c = pk[m][n+1] conj(pk[m][n]) (:150-172);
 *     every h_ls[m][n] is multiplied by exp(-j 2 pi mean(TO_est) D n scs 1000) (:174-207);
 *   1 edge extension (HLS_extra, dft_dct_CE.py:104-133): reK = eK + (N + eK) % 2; the degree-1
 *     least-squares line through the first 24/D points gives eK points on the left, the one
 *     through the last 24/D points reK on the right; the symmetric algorithms append the mirrored
 *     sequence (dft_dct_symmetric_CE.py:60-62).  M = N + eK + reK, or twice that; eK is the
 *     caller's eRB*12 // D;
 *   2 orthonormal inverse DFT of the ifftshift-ed sequence (dft_dct_CE.py:59) or orthonormal
 *     DCT-II of the real and imaginary parts (:61);
 *   3 window in samples, L_left / L_right, computed BY THE CALLER with the reference's own double
 *     expressions, which the two files word differently (dft_dct_CE.py:64-68,
 *     dft_dct_symmetric_CE.py:73-79);
 *   4 P = mean |tap[L_left : M - L_right]|^2; tap k is kept iff |tap[k]| >= sqrt(P / 2) and k is
 *     outside [L_left, M - L_right) (dft_dct_CE.py:71-80);
 *   5 orthonormal forward DFT + fftshift, or inverse DCT, of the kept taps (:83-86);
 *   6 linear interpolation to every subcarrier, the last value held (np.interp, :135-157); the
 *     symmetric algorithms interpolate the full-length sequence (their H_comb is never used,
 *     dft_dct_symmetric_CE.py:98-105);
 *   7 crop: H_est[m][:][nr][nt] = intp[eK*D : eK*D + N*D] (:92).
 * Per slot: 8 the degree-1 least-squares line over sym_idx per (subcarrier, nr, nt), evaluated at
 * symbols 0..13; S = 1 copies (timing_interpolate_to_14_symbol, :159-178).  9 covariance
 * (cov_m_estimate, :180-257): nHS = h_ls (compensated) - H_est[:, ::D]; groups of 16 PRB
 * (16*12/D DMRS REs), a residue merged into the last full group; per DMRS symbol and group
 * sum_re nHS[re] nHS[re]^H / count / Nt for every PRB of the group; times 2 when num_cdm_groups
 * == 1; then the time rule of step 8.
 * Twiddles: an on-chip table filled by one sincospi per entry of the exact rational j/M and
 * indexed by the reduced integer (k n) mod M (DCT: k (2n+1) mod 4M) — accurate to float64 for
 * every M; the transforms are direct sums (M is not a power of two), the forward DFT after one
 * decimation step by the largest power of two <= 8 that divides M.
 * Optional outputs (NULL to skip), contiguous:
 *   h_ls_comp [t][m][n][Nr][Nt] (row stride ldhc; to_comp only; must not overlap h_ls): the
 *             compensated h_ls, what comp_H_LS_timing_offset leaves in the caller's array
 *   h_est     [t][m][N*D][Nr][Nt], in_dtype         noise_power [t][m][Nr][Nt] float64 (P of step 4)
 *   taps      [t][m][Nr][Nt][M] uint8 kept mask     to_est [t][S], to_avg [t] float64 (seconds;
 *             computed whenever either is asked for, also without to_comp, as channel_est does)
 * Limits, all checked on the host BEFORE any HIP call (LDPC5G_ESIZE and a ldpc5g_last_error()
 * message naming the field): Nr in {1, 2, 4} and 1 <= Nt <= Nr (the equaliser's); 1 <= S <= 4
 * with sym_idx strictly ascending in 0..13; D in {2, 4}; N*D a multiple of 12 and PRB >= 16 (below
 * that the reference's grouping has num_of_M_prbs = -1 and indexes out of range, :199-206: there is
 * nothing to reproduce); M <= 2048, which covers 275 PRB at D = 4 with the symmetric extension up
 * to eRB = 8 (2*(825 + 24 + 25) = 1748); at D = 2 the symmetric extension reaches it near 160 PRB; 0 <= L_left,
 * L_right and L_left + L_right < M (otherwise the reference's noise mean is over an empty slice);
 * scs in {15, 30} (nr_channel_estimation.py:60); num_cdm_groups in 1..3; a known in_dtype and
 * algo; row strides at least their rows; T in 1..65535; a large enough workspace; non-null
 * required buffers. */
int64_t ldpc5g_ce_workspace_bytes(int32_t T, int32_t S, int32_t N, int32_t Nr, int32_t Nt, int32_t D);
int ldpc5g_channel_estimate(const void* h_ls, int64_t ldhls, int32_t in_dtype, int32_t T, int32_t S,
                            int32_t N, int32_t Nr, int32_t Nt, int32_t D, const int32_t* sym_idx,
                            int32_t algo, int32_t eK, int32_t L_left, int32_t L_right,
                            int32_t num_cdm_groups, int32_t to_comp, int32_t scs,
                            void* h, int64_t ldh, void* cov, int64_t ldcov,
                            void* work, int64_t work_bytes, void* h_ls_comp, int64_t ldhc,
                            void* h_est, double* noise_power, uint8_t* taps, double* to_est,
                            double* to_avg, void* stream);
/* Timing-offset compensation of the data REs (comp_pdsch_timing_offset,
 * nr_channel_estimation.py:209-221): out[t][m][k][r] = y[t][m][k][r] *
 * exp(-j 2 pi to_avg[t] k scs 1000) for nsym symbols of RE resource elements (k the RE index in
 * the allocation) and Nr antennas; to_avg: T float64 on the device (ldpc5g_channel_estimate's
 * to_avg).  out may be y (in place).  float64 arithmetic; in_dtype as above.  Nr in 1..64, scs in
 * {15, 30}, T in 1..65535, nsym in 1..1024, RE in 1..2^20, row strides (complex elements) at least
 * nsym*RE*Nr, non-null buffers: anything else returns LDPC5G_ESIZE before any HIP call. */
int ldpc5g_to_compensate(const void* y, int64_t ldy, void* out, int64_t ldo, int32_t in_dtype,
                         const double* to_avg, int32_t T, int64_t nsym, int64_t RE, int32_t Nr,
                         int32_t scs, void* stream);

/* ================================================ slot front end (before the channel estimator)
 * The producer of ldpc5g_channel_estimate's h_ls and of the equaliser's / detectors' y, from the
 * frequency-domain slot grid rx_fd_slot_data that Pdsch.H_LS_est and Pdsch.RX_process take
 * (py5gphy/nr_pdsch/nr_pdsch.py:212-284, 345-352), batched over T slots; and its transmit-side
 * inverse.  DMRS configuration type 1, single-symbol DMRS, no SSB / CSI-RS / PDCCH in the slot (the
 * reference's LS estimate does not handle them either, nr_pdsch_dmrs.py:193-194).
 * Layout, per slot t (row strides ld* in COMPLEX elements, only the slot stride is free):
 *   grid [t][r][s*carrier_re + k]   antenna-planar, s = 0..13, k = 0..carrier_re-1 subcarriers
 *   h_ls [t][m][n][Nr][Nt]          ldpc5g_channel_estimate's input, m = 0..S-1, n = 0..N-1, N = 3*rb_size
 *   y    [t][s*12*rb_size + re][Nr] the allocation's PRBs of all 14 symbols: ldpc5g_equalize's /
 *                                   ldpc5g_ml_detect's y with R = 14*12*rb_size, ldpc5g_to_compensate's
 *                                   y with nsym = 14, RE = 12*rb_size
 * slots: T int32 slot numbers ON THE DEVICE; ports (Nt entries: PortIndexList[p] - 1000, in the
 * caller's order) and sym_idx (S DMRS symbol indices) are HOST arrays read during the call.
 *
 * ldpc5g_slot_rx_frontend.  h_ls (pdsch_dmrs_LS_est, nr_pdsch_dmrs.py:196-219; pusch_dmrs_LS_est
 * with transform precoding disabled, nr_pusch_dmrs.py:163-190): for DMRS RE n of port p0, delta =
 * (p0 / 2) % 2, d0 = Y[4n + delta] conj(r(2n)), d1 = Y[4n + delta + 2] conj(r(2n + 1)), h_ls =
 * (d0 + d1) / (2 scaling) for even p0 and (d0 - d1) / (2 scaling) for odd p0; scaling = 1 when
 * num_cdm_groups == 1, else 10^(-3/20) (:170-174).  r is the QPSK mapping of the Gold sequence
 * (nrPRBS.py:5-25) from bit 2 (6 rb_start + n) on, cinit = (((14 slot + sym + 1)(2 nNIDnSCID + 1)
 * << 17) + 2 nNIDnSCID + nSCID) mod 2^31 (_gen_seq, :244-256), formed in the kernel from slots[t]
 * and generated there by jump-ahead: no host sequence, no table upload.  y (copy_Rx_pdsch_resource,
 * nrpdsch_resource_mapping.py:116-124) is a copy, bit for bit.  Either of h_ls / y may be NULL to
 * skip that half.  in_dtype LDPC5G_F32 (complex64) or LDPC5G_F64 (complex128) is the type of grid,
 * h_ls and y; the arithmetic is float64 for both (the reference multiplies in complex64).  At most
 * two launches (one per output), asynchronous on `stream`, no allocation, no synchronisation, no
 * atomics; results are bit-identical from run to run and a batch equals its slots run one by one.
 *
 * ldpc5g_slot_map (one launch).  sym [t][i*NL + l]: complex64 layer-interleaved modulated symbols
 * of data RE i (ldpc5g_scramble_modulate's output; the layer mapping of nr_pdsch_process.py:27-32);
 * re_idx: nre ascending flat indices s*12*rb_size + re of the data REs on the device (an index
 * outside 0..14*12*rb_size-1 writes nothing); precoding: HOST array of num_ant*NL complex64
 * (row-major [antenna][layer], interleaved re, im) or NULL for identity (needs NL <= num_ant).
 * Layer l is port 1000 + l (the reference's transmit map indexes rows by port,
 * nr_pdsch_dmrs.py:81-84).  Into the complex64 grid [t][a][.] it writes, for every antenna a,
 *   - the DMRS of nr_pdsch_dmrs.py:90-120 (wf = [1, 1 - 2 (l % 2)], wt = 1), times float32(scaling),
 *     precoded, at the REs 4n + delta and 4n + delta + 2 of the CDM groups that carry a layer;
 *   - the precoded data sum_l w[a][l] sym[.][l] (float32, l ascending; nr_pdsch_process.py:34-42) at
 *     the data REs (pdsch_data_re_mapping, nrpdsch_resource_mapping.py:58-85).
 * Every other RE of the grid is left untouched (the caller zeroes it).
 *
 * Limits, all checked on the host BEFORE any HIP call (LDPC5G_ESIZE and a ldpc5g_last_error()
 * message naming the argument): Nr, num_ant in {1, 2, 4}; 1 <= Nt, NL <= 4; ports in 0..3 and
 * distinct; 1 <= S <= 4 with sym_idx strictly ascending in 0..13; carrier_re a multiple of 12 and
 * carrier_re / 12 <= 275; 1 <= rb_size, 0 <= rb_start, rb_start + rb_size <= carrier_re / 12;
 * nNIDnSCID in 0..65535, nSCID in 0..1, num_cdm_groups in 1..2; T in 1..65535; 0 <= nre <=
 * 14*12*rb_size; a known in_dtype; row strides at least their rows; buffers aligned to their
 * element size; non-null required buffers (both h_ls and y NULL is refused). */
int ldpc5g_slot_rx_frontend(const void* grid, int64_t ldgrid, int32_t in_dtype, const int32_t* slots, int32_t T,
                            int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t Nr, int32_t Nt,
                            const int32_t* ports, int32_t S, const int32_t* sym_idx, int32_t nNIDnSCID,
                            int32_t nSCID, int32_t num_cdm_groups, void* h_ls, int64_t ldh, void* y, int64_t ldy,
                            void* stream);
int ldpc5g_slot_map(const void* sym, int64_t ldsym, const int32_t* re_idx, int64_t nre, const int32_t* slots,
                    int32_t T, int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t num_ant, int32_t NL,
                    const float* precoding, int32_t S, const int32_t* sym_idx, int32_t nNIDnSCID, int32_t nSCID,
                    int32_t num_cdm_groups, void* grid, int64_t ldgrid, void* stream);

/* ================================================ PUSCH transform precoding (DFT-s-OFDM)
 * The nTransPrecode = 1 branch of the reference's PUSCH, batched over T slots: the spreading DFT
 * (nr_pusch_process.py:39-54), the de-spreading IDFT before demodulation (nr_pusch.py:170-194),
 * the low-PAPR DMRS sequence (common/lowPAPR_seq.py:5-41) with its group / sequence hopping
 * (nr_pusch_dmrs.py:216-249), and the slot front end and transmit map that use it.  One layer
 * (the reference asserts it, nr_pusch_process.py:45), NumCDMGroupsWithoutData = 2 (with 1 the
 * reference's own assert at nr_pusch.py:179 fails), DMRS configuration type 1, single-symbol DMRS.
 * rb_size must be 2^a 3^b 5^c (38.211 6.3.1.4).  Row strides in COMPLEX elements; in_dtype
 * LDPC5G_F32 (complex64) or LDPC5G_F64 (complex128) is the storage type, the arithmetic is float64
 * for both and the complex64 result is the complex128 result rounded, bit for bit.  Every call is
 * asynchronous on `stream`, with no allocation, no synchronisation and no atomics; results are
 * bit-identical from run to run and a batch equals its rows run one by one.
 *
 * ldpc5g_transform_precode (one launch).  x [t][s*M + k], s < nsym, M = 12 rb_size: every M-block
 * is transformed on its own.  inverse = 0: out = DFT(x) / sqrt(M) (np.fft.fft(.) / sqrt(M),
 * nr_pusch_process.py:53); inverse = 1: out = IDFT(x) sqrt(M) (np.fft.ifft(.) * sqrt(M),
 * nr_pusch.py:188): both orthonormal.  out may equal x (in place, then ldo == ldx); any other
 * overlap is undefined.  A mixed-radix Stockham transform in LDS (radix 3, 5, 4, 2 passes), twiddles
 * from a table of sincospi(2 j / M) indexed by an exact integer.  Limits: T in 1..65535, nsym in
 * 1..14, rb_size in 1..275 and 2^a 3^b 5^c, inverse in 0..1, strides at least nsym*M, buffers
 * non-null and aligned to their element size.
 *
 * ldpc5g_low_papr_seq (one launch).  u, v: n int32 each ON THE DEVICE (group number 0..29, base
 * sequence number 0..1; v = 0 for MZC < 72); out [n][MZC] complex128 = exp(j alpha m) rbar_{u,v}(m)
 * of gen_lowPAPR_seq (lowPAPR_seq.py:5-41).  MZC = 30: exp(-j pi (u+1)(m+1)(m+2) / 31) (:30).
 * MZC >= 36: x_q(m mod N_ZC), x_q(i) = exp(-j pi q i (i+1) / N_ZC) (:32-38), N_ZC the largest prime
 * below MZC (found on the host), q = floor(qbar + 1/2) + v (-1)^floor(2 qbar), qbar = N_ZC (u+1) /
 * 31, all from integers; the phase index q i (i+1) is reduced mod 2 N_ZC in 64-bit integers before
 * the one sincospi (the reference evaluates pi q i (i+1) / N_ZC in floating point at arguments up
 * to ~1e7 rad and sits up to 2e-9 away).  Limits: n in 1..65535; MZC a multiple of 6 in 30..3300 —
 * MZC in {6, 12, 18, 24} are the tables of 38.211 5.2.2.2, not provided, and refused; alpha finite.
 *
 * ldpc5g_slot_rx_frontend_tp: ldpc5g_slot_rx_frontend for pusch_dmrs_LS_est with nTransPrecode = 1
 * (nr_pusch_dmrs.py:163-190): one layer on port `port` (0..3; delta and the sign of d1 as above),
 * scaling 10^(-3/20), h_ls [t][m][n][Nr][1]; y by ldpc5g_slot_rx_frontend's extraction.  The
 * sequence of (t, m) has alpha = 0 and length 6 rb_size and is formed in the kernel from slots[t]
 * and sym_idx[m] (_gen_seq_with_transform_precoding, :216-249):
 *   hopping 0 (neither):  u = nPuschID % 30, v = 0
 *   hopping 1 (group):    f_gh = (sum_{i<8} 2^i c(8 (14 slot + sym) + i)) mod 30 with cinit =
 *                         floor(nPuschID / 30); u = (f_gh + nPuschID) % 30, v = 0       (:230-239)
 *   hopping 2 (sequence): u = nPuschID % 30; v = c(14 slot + sym) with cinit = nPuschID (as the
 *                         reference has it) when 6 rb_size >= 72, else 0                  (:223-225, 241-249)
 * with the Gold bits by jump-ahead (no host sequence); slots[t] in 0..19 (the reference makes one
 * frame of hopping bits).  base_seq: optional complex128 [T][S][6 rb_size] ON THE DEVICE that
 * replaces the generated sequence; required (NULL refused) when rb_size <= 4.  Limits: those of
 * ldpc5g_slot_rx_frontend, and port in 0..3, nPuschID in 0..1007, hopping in 0..2, rb_size of the
 * form 2^a 3^b 5^c.  At most two launches.
 *
 * ldpc5g_slot_map_tp (one launch): ldpc5g_slot_map for the same case.  sym [t][i]: the complex64
 * (already transform-precoded) symbol of data RE i; precoding: HOST array of num_ant complex64
 * ([antenna][0], interleaved re, im) or NULL for identity (antenna 0 carries the layer, the others
 * zeros); base_seq as above.  Into the complex64 grid it writes float32(scaling r(2n)) at RE 4n +
 * delta and float32(+- scaling r(2n+1)) at 4n + delta + 2 of every DMRS symbol (nr_pusch_dmrs.py:76-101;
 * the other comb stays untouched), and the data at the data REs, both precoded with float32
 * products.  Limits: those of ldpc5g_slot_map with NL = 1, and the ones above. */
int ldpc5g_transform_precode(const void* x, int64_t ldx, void* out, int64_t ldo, int32_t in_dtype, int32_t T,
                             int32_t nsym, int32_t rb_size, int32_t inverse, void* stream);
int ldpc5g_low_papr_seq(const int32_t* u, const int32_t* v, int32_t n, double alpha, int32_t MZC, void* out,
                        void* stream);
int ldpc5g_slot_rx_frontend_tp(const void* grid, int64_t ldgrid, int32_t in_dtype, const int32_t* slots, int32_t T,
                               int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t Nr, int32_t port,
                               int32_t S, const int32_t* sym_idx, int32_t nPuschID, int32_t hopping,
                               const void* base_seq, void* h_ls, int64_t ldh, void* y, int64_t ldy, void* stream);
int ldpc5g_slot_map_tp(const void* sym, int64_t ldsym, const int32_t* re_idx, int64_t nre, const int32_t* slots,
                       int32_t T, int32_t carrier_re, int32_t rb_start, int32_t rb_size, int32_t num_ant, int32_t port,
                       const float* precoding, int32_t S, const int32_t* sym_idx, int32_t nPuschID, int32_t hopping,
                       const void* base_seq, void* grid, int64_t ldgrid, void* stream);

/* ================================================ OFDM low-PHY: time-domain slot <-> resource grid
 * Rx_low_phy (nr_lowphy/rx_lowphy_process.py:35-98) and Tx_low_phy (tx_lowphy_process.py:10-80),
 * batched over T slots and Nr (num_ant) antennas, one launch each.  td holds slots of 15 nfft
 * samples (14 symbols, each its cyclic prefix then nfft samples), sample n of antenna r of slot t at
 * td[t * ld_td_slot + r * ld_td_ant + n]; grid holds RE k of symbol s at grid[t * ld_g_slot +
 * r * ld_g_ant + s * carrier_re + k].  All four strides are free, in COMPLEX elements: the slot
 * front end's [t][r][.] and the reference's waveform layout [r][slot * 15 nfft + n] are the same
 * call.  CP lengths are the reference's 4096-point lists divided by 4096 / nfft: [352] + [288]*13
 * (scs 30), [320] + [288]*6 + [320] + [288]*6 (scs 15).  dtype LDPC5G_F32 (complex64) or LDPC5G_F64
 * (complex128) is the storage type of td and grid; the arithmetic is float64 for both and the
 * complex64 result is the complex128 one rounded.  Asynchronous on `stream`, no allocation, no
 * synchronisation, no atomics; bit-identical from run to run, a batch equals its slots one by one.
 * td and grid must not overlap.  The antennas are never permuted (the reference's fftshift without
 * axes also rolls them; that belongs to the Python drop-ins).
 *
 * ldpc5g_ofdm_demod, symbol s with off samples before it, cp its prefix, h = cp_short / 2: the
 * nfft samples from off + cp - h on, times exp(+2 pi j carrier_hz (off + cp) / fs), fs = nfft scs
 * 1000 (skipped when carrier_hz is a multiple of fs; the phase is the exact rational (carrier_hz
 * (off + cp) mod fs) / fs); forward FFT / sqrt(nfft); fftshift; position i of the shifted array
 * times exp(2 pi j h i / nfft); positions (nfft - carrier_re) / 2 ... go to the grid.
 *
 * ldpc5g_ofdm_mod, the inverse: the carrier_re REs at the centre of a zeroed nfft array — with dm
 * (DEVICE float64 [T][14], or NULL) RE k first times exp(2 pi j k scs 1000 dm[t][s]), that product
 * rounded to the storage type — ifftshift, inverse FFT * sqrt(nfft), then cp + nfft samples
 * td[n] = x[(n - cp) mod nfft] times exp(-2 pi j carrier_hz (off + cp) / fs).  The grid is not
 * written.
 *
 * Limits, checked on the host BEFORE any HIP call (LDPC5G_ESIZE and a message naming the
 * argument): a known dtype; T in 1..65535; Nr / num_ant in {1, 2, 4}; nfft in {128, 256, 512, 1024,
 * 2048, 4096}; carrier_re a multiple of 12 in 12..nfft; scs in {15, 30}; ld_td_slot (T > 1) and
 * ld_td_ant (Nr > 1) at least 15 nfft, ld_g_slot and ld_g_ant at least 14 carrier_re; td, grid
 * non-null; td, grid, dm aligned to their element. */
int ldpc5g_ofdm_demod(const void* td, int64_t ld_td_slot, int64_t ld_td_ant, void* grid, int64_t ld_g_slot,
                      int64_t ld_g_ant, int32_t dtype, int32_t T, int32_t Nr, int32_t nfft, int32_t carrier_re,
                      int32_t scs, int64_t carrier_hz, void* stream);
int ldpc5g_ofdm_mod(const void* grid, int64_t ld_g_slot, int64_t ld_g_ant, const double* dm, void* td,
                    int64_t ld_td_slot, int64_t ld_td_ant, int32_t dtype, int32_t T, int32_t num_ant, int32_t nfft,
                    int32_t carrier_re, int32_t scs, int64_t carrier_hz, void* stream);

/* ================================================ polar code (TS 38.212 §5.3.1, §5.4.1)
 * The reference's py5gphy/polar, batched: B blocks per launch, bits int8, LLRs float64.
 *
 * ldpc5g_polar_plan is host-only.  For one (K, E, nMax, iIL, CRCLEN, padCRC, rnti) — K counts the
 * CRC — it builds what the kernels need (polar_construct.construct and §5.3.1.2 / §5.4.1.1): N,
 * the frozen mask F, qPC with nPC and nPCwm (row weight 2^popcount), the u -> ck map, the input
 * interleaver and its inverse, the PC parity masks, for iIL = 1 the 24 distributed-CRC parity masks
 * (over u positions) and the 24-bit CRC mask, and the channel interleaver of E.  It returns the
 * plan's size in bytes (plan == NULL: size only) or a negative error.  The plan is an opaque blob
 * with a magic number and a version; the caller keeps the host copy and uploads one device copy,
 * and every entry point below takes both (plan_dev, plan_host) and checks the host copy's magic
 * and version.  Its first 18 int32: magic, version, bytes, K, E, nMax, iIL, CRCLEN, padCRC, rnti,
 * N, n, nPC, nPCwm, qPC[3], mode (0 repetition, 1 puncturing, 2 shortening); F (N bytes) follows
 * at byte offset int32[19].
 *
 * Limits, all checked on the host BEFORE any HIP call (LDPC5G_ESIZE and a ldpc5g_last_error()
 * message): (nMax, iIL, CRCLEN) in {(9, 1, 24), (10, 0, 6), (10, 0, 11)}; E in 1..8192; K > CRCLEN;
 * for nMax = 10, K in 18..25 or > 30; for iIL = 1, K <= 164; K + nPC <= E and <= N; padCRC in
 * {0, 1}; rnti in 0..2^24-1; B in 1..2^22; row strides at least their rows (K, N or E); non-null
 * buffers; a plan with the right magic and version; for decode, algo SC or SCL, L in 1..32 and N in
 * 32..1024.
 *
 *   encode        bits [B][ldb] (K used) -> out [B][ldo] (N): interleave (iIL), PC bits, x = u G_N
 *   rate_match    d [B][ldi] (N) -> f [B][ldo] (E): sub-block interleaver, bit selection, and with
 *                 iBIL the triangular channel interleaver
 *   rate_recover  llr [B][ldi] (E) -> out [B][ldo] (N): repetitions summed whole copies first, then
 *                 the remainder, sequential float64 adds; punctured positions 0; shortened positions
 *                 llr_limit.  reference_repetition = 1 reproduces nr_polar_raterecover.py:40, which
 *                 with iBIL = 1 sums the LLRs it did not de-interleave.
 *   decode        llr [B][ldl] (N) -> ck [B][ldc] (K), status [B] (1 decoded, 0 failed: that ck row
 *                 is all -1), pm [B] (the returned path's metric; +inf on failure).  SC ignores L
 *                 and always reports 1.  N = 1024 with L > 16 keeps its largest one or two LLR layers in a
 *                 stream-ordered allocation (hipMallocAsync / hipFreeAsync on `stream`), at most
 *                 1024 workgroups' worth; every other shape runs from LDS alone. */
#define LDPC5G_POLAR_SC 0
#define LDPC5G_POLAR_SCL 1
int64_t ldpc5g_polar_plan(int32_t K, int32_t E, int32_t nMax, int32_t iIL, int32_t crclen, int32_t padCRC,
                          int32_t rnti, void* plan, int64_t plan_bytes);
int ldpc5g_polar_encode(const void* plan_dev, const void* plan_host, const int8_t* bits, int64_t ldb, int8_t* out,
                        int64_t ldo, int32_t B, void* stream);
int ldpc5g_polar_rate_match(const void* plan_dev, const void* plan_host, const int8_t* d, int64_t ldi, int8_t* f,
                            int64_t ldo, int32_t B, int32_t iBIL, void* stream);
int ldpc5g_polar_rate_recover(const void* plan_dev, const void* plan_host, const double* llr, int64_t ldi,
                              double* out, int64_t ldo, int32_t B, int32_t iBIL, double llr_limit,
                              int32_t reference_repetition, void* stream);
int ldpc5g_polar_decode(const void* plan_dev, const void* plan_host, const double* llr, int64_t ldl, int8_t* ck,
                        int64_t ldc, uint8_t* status, double* pm, int32_t B, int32_t algo, int32_t L,
                        void* stream);

/* ================================================ UCI on PUSCH (TS 38.212 §5.3.3, §6.2.7, §6.3.2.4)
 * The reference's py5gphy/smallblock, nr_ulsch_info.py and nr_pusch_datactrl_multiplex.py, batched over
 * T rows (slots / transport blocks), bits int8, LLRs float32 or float64 (LDPC5G_F32 / LDPC5G_F64).
 *
 * ldpc5g_uci_rm_info is host-only: getULSCH_RM_info (nr_ulsch_info.py:6-170) with O = Enable * NumBits
 * for each of HARQ-ACK, CSI part 1 and CSI part 2.  out[9] = Euci_ack, Qbar_ACK, Euci_CSI1, Qbar_CSI1,
 * Euci_CSI2, Qbar_CSI2, Euci_ackrvd, Qbar_ACKrvd, G_ULSCH.  The ceilings are taken of the reference's
 * double products in its order.  Where the reference asserts (an E above 8192 or below the payload's
 * minimum capacity, Gtotal < Euci_CSI1 + Euci_CSI2, an offset index outside its table) or divides by
 * ULSCH_size = 0, LDPC5G_ESIZE and a message.  Both host functions check the allocation the same way: RBSize
 * 1..275, the symbols inside the slot, 1..14 DMRS symbols each in 0..13, NL 1..4, Qm in {1, 2, 4, 6, 8}.
 *
 * ldpc5g_uci_map_plan is host-only and linear in Gtotal (flags per resource element): the §6.2.7 map
 * of nr_pusch_datactrl_multiplex.py:7-267 for one configuration, no frequency hopping (refused),
 * NumCDMGroupsWithoutData 1 or 2, no UCI on DMRS symbols.  It returns the plan's size in bytes (plan ==
 * NULL: size only) or a negative error (LDPC5G_ESIZE also where the reference would index past a list:
 * UCI that does not fit, stream lengths that are not the allocation's).  The caller keeps the host copy
 * and uploads one device copy; the entry points take both and check the host copy's header.  Layout:
 *   int32 header[32]: magic "UCIP", version, bytes, Gtotal, Qm, NL, OACK, OCSI1, OCSI2, EnableULSCH,
 *                     len[4] (UL-SCH, ACK, CSI1, CSI2 stream lengths; 0 for an absent stream),
 *                     byte offset of fwd, byte offset of inv, punctured bits, ninv = sum of len,
 *                     x placeholders, y placeholders; the rest 0
 *   uint32 fwd[Gtotal]: for position t of g_seq, the stream that finally owns it and the index in it
 *   uint32 inv[ninv]:   for each stream element (the four streams one after another), its position t
 *   entry bits: 0..23 index or t; 24..26 stream (0 UL-SCH, 1 ACK, 2 CSI1, 3 CSI2, 4 none: left 0);
 *               27..28 kind of a 1-2 bit HARQ-ACK position (0 data, 1 placeholder x, 2 placeholder y);
 *               29 punctured: in fwd, a 1-2 bit HARQ-ACK position that overwrites another stream (step 5
 *               on the reserved set); in inv, the overwritten element of that stream (UL-SCH, or CSI
 *               part 2 placed on reserved resource elements), which still points at the position.
 *
 * Kernels, asynchronous on `stream`, no allocation, one launch each.  Limits, checked on the host
 * BEFORE any HIP call: a plan with the right magic, version and sizes; T in 1..65535 (small-block
 * decode: 1..2^22); every row stride at least its row; non-null buffers for every stream the plan holds.
 *   uci_mux       g_seq[t] = stream[index] (data_control_multiplex; a position without a stream is 0)
 *   uci_demux     the four streams of llr [T][ldl] (Gtotal used).  prbs == NULL: the permutation of
 *                 data_control_separate, punctured LLRs left inside g_ulsch as the reference leaves
 *                 them.  prbs != NULL (packed words of ldpc5g_prbs, the input still scrambled):
 *                 ordinary positions times 1 - 2 c[t], a y position times 1 - 2 c[t - 1], an x position
 *                 +0.  erase_punctured = 1 writes +0 for elements marked punctured.
 *   uci_scramble_modulate   38.211 §6.3.1.1 with placeholders (x = -1 -> 1, y = -2 -> the scrambled
 *                 bit before it, everything else XOR c) and the mapper of ldpc5g_scramble_modulate;
 *                 mod in {1, -1, 2, 4, 6, 8}; prbs is required.  A y may stand anywhere: one that opens a symbol, or
 *                 follows other y, repeats the nearest scrambled bit before the run (0 if the run starts the row),
 *                 as the reference's sequential loop does.  Values other than 0, 1, -1, -2 are not checked.
 *   smallblock_encode   bits [T][ldb] (K in 1..11 used) -> out [T][ldo] (E in 1..8192): §5.3.3 repeated
 *                 to E (encode_uci_on_ulsch); K = 1, 2 use Qm and produce the placeholders -1 / -2.
 *   smallblock_decode   llr [T][ldl] (E used) -> K bits: the E LLRs folded modulo N (Qm, 3 Qm or 32) by
 *                 summing the repetitions in ascending order in float64, then the maximum-likelihood
 *                 message, ties to the smallest message read MSB first; placeholders x are ignored,
 *                 K = 1 with Qm >= 2 adds the y position. */
int ldpc5g_uci_rm_info(int32_t RBSize, int32_t StartSymbolIndex, int32_t NrOfSymbols, const int32_t* dmrs_symlist,
                       int32_t num_dmrs, int32_t NL, int32_t Qm, double coderateby1024, int64_t ULSCH_size,
                       int32_t EnableULSCH, int32_t OACK, int32_t OCSI1, int32_t OCSI2, int32_t I_HARQ_ACK_offset,
                       int32_t I_CSI1offset, int32_t I_CSI2offset, double UCIScaling, int64_t Gtotal, int64_t* out);
int64_t ldpc5g_uci_map_plan(int32_t RBSize, int32_t StartSymbolIndex, int32_t NrOfSymbols, const int32_t* dmrs_symlist,
                            int32_t num_dmrs, int32_t NumCDMGroupsWithoutData, int32_t NL, int32_t Qm, int32_t OACK,
                            int32_t OCSI1, int32_t OCSI2, int32_t EnableULSCH, int32_t frequency_hopping, int64_t Euci_ack,
                            int64_t Euci_CSI1, int64_t Euci_CSI2, int64_t Euci_ackrvd, int64_t G_ULSCH, int64_t Gtotal,
                            void* plan, int64_t plan_bytes);
int ldpc5g_uci_mux(const void* plan_dev, const void* plan_host, const int8_t* g_ulsch, int64_t ld_ulsch, const int8_t* g_ack,
                   int64_t ld_ack, const int8_t* g_csi1, int64_t ld_csi1, const int8_t* g_csi2, int64_t ld_csi2, int8_t* g_seq,
                   int64_t ldg, int32_t T, void* stream);
int ldpc5g_uci_demux(const void* plan_dev, const void* plan_host, const void* llr, int32_t dtype, int64_t ldl,
                     const uint32_t* prbs, int64_t ldw, int32_t erase_punctured, void* g_ulsch, int64_t ld_ulsch, void* g_ack,
                     int64_t ld_ack, void* g_csi1, int64_t ld_csi1, void* g_csi2, int64_t ld_csi2, int32_t T, void* stream);
int ldpc5g_uci_scramble_modulate(const int8_t* bits, int64_t ldb, const uint32_t* prbs, int64_t ldw, int32_t T, int64_t nbits,
                                 int32_t mod, void* sym, int64_t ldsym, void* stream);
int ldpc5g_smallblock_encode(const int8_t* bits, int64_t ldb, int32_t K, int32_t Qm, int8_t* out, int64_t ldo, int32_t E,
                             int32_t T, void* stream);
int ldpc5g_smallblock_decode(const void* llr, int32_t dtype, int64_t ldl, int32_t E, int32_t K, int32_t Qm, int8_t* out,
                             int64_t ldo, int32_t T, void* stream);

/* ================================================ gather records (multi-GPU)
 * Record r (a row of rec, stride ldr bytes) = the nbits int8 bits of row r of `bits` (values 0/1)
 * packed in np.packbits order (bit i -> byte i/8, bit 7 - i%8, tail zero-padded), then
 * status[r] (one byte, if status != NULL), then iters[r] (int32 little-endian, if iters != NULL).
 * One record per codeblock (bits = its K info bits) or per transport block (its tbblk + CRC
 * flag): a rank's results become one contiguous block for a single gather.  unpack reverses it;
 * any of bits / status / iters may be NULL there to skip that field.  No reference counterpart
 * (the reference runs in one process); the unpacked bits are the reference's blkandcrc / tbblk
 * (nr_ldpc_decode.py:47-49, nr_dlsch_decode.py:103-109). */
int ldpc5g_pack_records(const int8_t* bits, int64_t ldb, int32_t R, int64_t nbits,
                        const uint8_t* status, const int32_t* iters, uint8_t* rec, int64_t ldr,
                        void* stream);
int ldpc5g_unpack_records(const uint8_t* rec, int64_t ldr, int32_t R, int64_t nbits, int8_t* bits,
                          int64_t ldb, uint8_t* status, int32_t* iters, int64_t fstride,
                          void* stream);   /* status / iters of record r at [r * fstride] */

/* Message of the last failed call on this thread ("" if none). */
const char* ldpc5g_last_error(void);

/* Library version string. */
const char* ldpc5g_version(void);

/* Diagnostics: decoder workgroups that can be resident on one CU (HIP occupancy calculator) for
 * (bgn, llr_dtype, schedule).  No reference counterpart. */
int ldpc5g_dec_blocks_per_cu(int32_t bgn, int32_t llr_dtype, int32_t schedule);

/* ---- the multi-workgroup float64 decoder (few large codeblocks per call).
 * ldpc5g_decode_ms / ldpc5g_decode_ms_host / ldpc5g_sch_decode with float64 flooding and at most
 * ~24 codeblocks of Zc >= 64 (the per-codeblock drop-ins' shape) run each codeblock over W (9-18)
 * workgroups, one per CU, that synchronise through global memory twice per iteration.  It assumes:
 *   - co-residency: a codeblock's W workgroups run at the same time.  Workgroups take their
 *     (codeblock, part) by arrival ticket, so one launch never waits on itself, and launches use at
 *     most 7/8 of the device's CUs; but a kernel of another library or process that holds CUs
 *     indefinitely (a persistent kernel) could keep parts from starting.  A barrier wait therefore
 *     gives up after 4 s: the codeblock is returned with status 0 and iters -1 (never silently
 *     wrong), the device's timeout count grows (below), and the library stays usable;
 *   - serialisation: split launches of one device are chained by one hidden event (they share a
 *     per-device sync area and scratch), so they run one after another whatever their streams;
 *   - the first split launch on a device, and one needing more scratch, allocate (hipMalloc /
 *     hipMemset / a device synchronisation, or an event wait + hipFree when growing): not capturable.
 *     A stream in capture (hipStreamIsCapturing) never takes this path — such launches run the
 *     one-workgroup-per-codeblock kernels instead (same results, bit for bit).
 * ldpc5g_split_timeouts: the number of codeblocks of the current device whose split decode timed
 * out since the process started (waits for the device's last split launch).  No reference
 * counterpart. */
int ldpc5g_split_timeouts(uint32_t* count);

#ifdef __cplusplus
}
#endif

#endif /* LDPC5G_H */
