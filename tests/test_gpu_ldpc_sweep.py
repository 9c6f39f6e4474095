"""GPU: every lifting size (51 Zc x 2 base graphs = 102 pairs) through every decoder dispatch path and
the encoder, bit-exact with the oracle; the reference's own outputs at the mid sizes through the drop-in.

Inputs come from one recipe (ldpc_sweep_ref.sweep_input; tests/test_ldpc_sweep_inputs.py shows on the CPU
that they separate a right decoder from a wrong one): L = 8, NMS alpha = 0.75 unless said otherwise.  The
bar is ck, status and iters equal to the oracle's unless said otherwise.  G = codeblocks per workgroup =
max(T // Zc, 1) with T = 768 (layered) or 384 (flooding) threads (ldpc5g_common.h dec_G); "rm" = the
same launch with rate_matched=True on an input whose last 5 + (index of Zc) % 20 columns are +0.0.

  path (test)                  kernel file                      dispatch condition (ldpc5g_dec.hip launch_dec)       B
  ---------------------------  -------------------------------  ---------------------------------------------------  ---------------------
  layered f32 (batch_f32)      ldpc5g_dec_l.hip                 schedule layered                                     max(2G + 1, 5)
  layered f32 dead rows        ldpc5g_dec_l_dead.hip            ... and LDPC5G_RATE_MATCHED                          same
  flooding f32 (batch_f32)     ldpc5g_dec_f32.hip               flooding, G * Zc > 64 slots                          max(2G + 1, 5)
  flooding f32 dead rows       ldpc5g_dec_dead_f32.hip          ... and LDPC5G_RATE_MATCHED                          same
  flooding f64 batch           ldpc5g_dec.hip (flood_t)         float64, !split_wanted, G * Zc > 64, Zc != 384       f64_batch_size:
  flooding f64 dead rows       ldpc5g_dec_dead.hip              ... and LDPC5G_RATE_MATCHED                           max(2G + 1, 5,
  Zc = 384 frame kernel        ldpc5g_dec_frame{1,2}[_dead].hip  float64, !split_wanted, Zc == kFrameZc (live/dead)    224 // w2 + 1)
  flooding f64 split           ldpc5g_dec_split.hip             float64 and split_wanted(bgn, B, Zc): Zc >= 64       1 (drop-in), 3
                                                                (BG1) / Zc > 64 (BG2), B * split_parts <= maxwg
  small launches               ldpc5g_dec_small.h (small_fits)  min(G, B) * Zc <= kFloodSmallCS = 64                 1 and 64 // Zc
                               else ldpc5g_dec_flood16[_f32].hip  (BG1 Zc = 64 float64: split_wanted comes first)
  mixed-Zc work lists          launch_dec_mixed: *_mixed_* of   ldpc5g_decode_ms_mixed_plan (MixedBatch)             3 of each of the 51
                               the files above                                                                      sizes, per base graph
  BF, BP                       ldpc5g_bfbp.hip                  algo                                                 5
  encode                       ldpc5g_enc.hip                   -                                                    33

Whoever moves one of these thresholds moves the B of the row with it.  The LLR tensors are exactly sized
(numpy in, a fresh device tensor per call); test_tail_reads_stay_inside_the_batch repeats one launch per
batched path on a view whose following rows are NaN."""
import numpy as np
import pytest

import ldpc_sweep_ref as S
from oracle import ldpc_oracle as O

pytestmark = pytest.mark.gpu

PAIR = pytest.mark.parametrize("pair", S.PAIRS, ids=S.pair_id)
BATCH_PATHS = [("layered", np.float32, "layered"), ("flooding", np.float32, "flooding-f32"),
               ("flooding", np.float64, "flooding-f64")]
MIDZC = S.load_midzc_cases()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a ROCm GPU"
    return t


@pytest.fixture(scope="module")
def dec(torch):
    from python_5gtoolbox_amd import nr_ldpc_decode
    return nr_ldpc_decode


@pytest.fixture(scope="module")
def enc(torch):
    from python_5gtoolbox_amd import nr_ldpc_encode
    return nr_ldpc_encode


def _same(got, ref, what):
    for name, g, r in zip(("ck", "status", "iters"), got, ref):
        assert np.array_equal(np.asarray(g), r), (name,) + tuple(what)


def _batch_B(bg, Zc, schedule, dtype):
    return S.f64_batch_size(bg, Zc) if dtype == np.float64 else S.batch_size(Zc, schedule == "layered")


# ------------------------------------------------------------------- uniform batches, min-sum
@PAIR
@pytest.mark.parametrize("schedule,dtype,tag", BATCH_PATHS, ids=[p[2] for p in BATCH_PATHS])
def test_batch_kernels_vs_oracle(dec, schedule, dtype, tag, pair):
    """Full workgroups and a last one holding a single codeblock, plain and with dead rows.  The
    float64 batch is large enough that the split kernel does not take it (S.f64_batch_size)."""
    bg, Zc = pair
    B = _batch_B(bg, Zc, schedule, dtype)
    for rm in (False, True):
        _, llr = S.sweep_input(bg, Zc, tag + ("-rm" if rm else ""), B, dtype, S.n_zeroed(Zc) if rm else 0)
        got = dec.nr_decode_ldpc_batch(llr, Zc, bg, S.L, "min-sum", S.ALPHA, S.BETA, schedule, rate_matched=rm)
        _same(got, S.oracle_decode(llr, bg, Zc, schedule), (bg, Zc, tag, rm, B))


@pytest.mark.parametrize("bg", [1, 2])
def test_frame_kernel_mixed_liveness_batch(dec, bg):
    """Zc = 384 float64, rate_matched=True, in a batch the split kernel cannot take (25 BG1 / 29
    BG2 codeblocks, S.f64_batch_size), with a different zeroed tail per codeblock (0, 1, 7, 25,
    all but one extension column, a -0.0 tail, a dead tail with one live entry): the frame kernel
    chooses the dead-row or the plain iterations per workgroup from what it loads, so one launch
    runs both.  NMS and OMS."""
    Zc = 384
    B = S.f64_batch_size(bg, Zc)
    _, llr = S.sweep_input(bg, Zc, "frame-liveness", B, np.float64)
    nx = S.DIMS[bg][3] - 4
    for b in range(B):
        kind = b % 7
        if kind in (1, 2, 3, 4):
            llr[b, -(1, 7, 25, nx - 1)[kind - 1] * Zc:] = 0.0
        elif kind == 5:
            llr[b, -7 * Zc:] = -0.0            # live: the bit pattern is not +0.0
        elif kind == 6:
            llr[b, -7 * Zc:] = 0.0
            llr[b, -1] = 1.5
    for alpha, beta in ((S.ALPHA, S.BETA), (1.0, 0.5)):
        got = dec.nr_decode_ldpc_batch(llr, Zc, bg, S.L, "min-sum", alpha, beta, "flooding", rate_matched=True)
        _same(got, S.oracle_decode(llr, bg, Zc, "flooding", alpha, beta), (bg, alpha, beta))


@pytest.mark.parametrize("schedule,dtype,tag", BATCH_PATHS + [("flooding", np.float64, "split")],
                         ids=[p[2] for p in BATCH_PATHS] + ["split"])
def test_tail_reads_stay_inside_the_batch(torch, dec, schedule, dtype, tag):
    """BG2 Zc = 104 (G = 3 flooding with 72 idle lanes, G = 7 layered; a partial last wave): the
    same launches on a view of a taller tensor whose rows past the batch are NaN, so a read past
    the batch that reached a real slot would change its result."""
    bg, Zc = 2, 104
    B = 3 if tag == "split" else _batch_B(bg, Zc, schedule, dtype)
    _, llr = S.sweep_input(bg, Zc, tag, B, dtype)
    ref = S.oracle_decode(llr, bg, Zc, schedule)
    pad = torch.full((B + 4, llr.shape[1]), float("nan"), dtype=torch.from_numpy(llr).dtype, device="cuda")
    pad[:B] = torch.from_numpy(llr).cuda()
    ck, st, it = dec.nr_decode_ldpc_batch(pad[:B], Zc, bg, S.L, "min-sum", S.ALPHA, S.BETA, schedule)
    _same((ck.cpu().numpy(), st.cpu().numpy().astype(bool), it.cpu().numpy()), ref, (tag, B))


# --------------------------------------------------------- float64 split kernel and the drop-in
@pytest.mark.parametrize("pair", [p for p in S.PAIRS if S.split_serves(*p)], ids=S.pair_id)
def test_split_kernel_vs_oracle(dec, pair):
    """Every size the multi-workgroup kernel serves: one codeblock through the nr_decode_ldpc
    drop-in, three through the batched call with NMS, OMS, and rate_matched=True on a zeroed tail."""
    bg, Zc = pair
    _, llr = S.sweep_input(bg, Zc, "split", 3, np.float64)
    nms = S.oracle_decode(llr, bg, Zc, "flooding")
    blk, ck, st = dec.nr_decode_ldpc(llr[0], Zc, bg, S.L, "min-sum", S.ALPHA, S.BETA)
    assert np.array_equal(ck, nms[0][0]) and st == bool(nms[1][0]), (bg, Zc, "drop-in")
    _same(dec.nr_decode_ldpc_batch(llr, Zc, bg, S.L, "min-sum", S.ALPHA, S.BETA, "flooding"), nms, (bg, Zc, "NMS"))
    got = dec.nr_decode_ldpc_batch(llr, Zc, bg, S.L, "min-sum", 1.0, 0.5, "flooding")
    _same(got, S.oracle_decode(llr, bg, Zc, "flooding", 1.0, 0.5), (bg, Zc, "OMS"))
    _, x = S.sweep_input(bg, Zc, "split-rm", 3, np.float64, S.n_zeroed(Zc))
    got = dec.nr_decode_ldpc_batch(x, Zc, bg, S.L, "min-sum", S.ALPHA, S.BETA, "flooding", rate_matched=True)
    _same(got, S.oracle_decode(x, bg, Zc, "flooding"), (bg, Zc, "rm"))


def _case_id(c):
    return "%s-bg%d-z%d-a%g%s" % (c["algo"], c["bg"], c["Zc"], c["alpha"], "-tail0" if c["nzero"] else "")


@pytest.mark.parametrize("c", [c for c in MIDZC if c["algo"] == "min-sum"], ids=_case_id)
def test_midzc_golden_dropin(dec, c):
    """The reference's own ck and status at Zc 104 ... 352 and BG2 Zc = 384 (NMS / OMS, half with a
    zeroed tail, which makes the drop-in set LDPC5G_RATE_MATCHED itself) through nr_decode_ldpc."""
    blk, ck, st = dec.nr_decode_ldpc(c["llr"], c["Zc"], c["bg"], c["L"], "min-sum", c["alpha"], c["beta"])
    assert ck.dtype == np.int8 and np.array_equal(ck, c["ck"]) and st == c["status"]


@pytest.mark.parametrize("c", [c for c in MIDZC if c["algo"] != "min-sum"], ids=_case_id)
def test_midzc_golden_bf_bp_dropin(dec, c):
    """The bars of test_decode_bf_golden_bitexact / test_decode_bp_golden at the mid sizes: BF bit
    for bit (float64 ck); BP the same status, and the same ck where the reference converged."""
    blk, ck, st = dec.nr_decode_ldpc(c["llr"], c["Zc"], c["bg"], c["L"], c["algo"])
    assert st == c["status"]
    if c["algo"] == "BF":
        assert ck.dtype == np.float64 and np.array_equal(ck, c["ck"])
    else:
        assert ck.dtype == np.int8
        if c["status"]:
            assert np.array_equal(ck, c["ck"])


# ----------------------------------------------------------------------------- small launches
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("pair", [p for p in S.PAIRS if p[1] <= 64], ids=S.pair_id)
def test_small_launches_vs_oracle(dec, pair, dtype):
    """B * Zc <= 64: one codeblock, and as many as fit 64 slots — the small-codeblock kernel at
    each of its nodes-per-thread instantiations, the 16-part configuration where it does not fit."""
    bg, Zc = pair
    B = 64 // Zc
    _, llr = S.sweep_input(bg, Zc, "small", B, dtype)
    ref = S.oracle_decode(llr, bg, Zc, "flooding")
    for n in sorted({1, B}):
        got = dec.nr_decode_ldpc_batch(llr[:n], Zc, bg, S.L, "min-sum", S.ALPHA, S.BETA, "flooding")
        _same(got, [r[:n] for r in ref], (bg, Zc, n))


# --------------------------------------------------------------------------------- mixed Zc
@pytest.mark.parametrize("bg", [1, 2])
@pytest.mark.parametrize("schedule,dtype,tag", BATCH_PATHS, ids=[p[2] for p in BATCH_PATHS])
def test_mixed_batch_all_sizes_vs_oracle(torch, schedule, dtype, tag, bg):
    """One MixedBatch holding three codeblocks of each of the 51 lifting sizes; every other group
    has a zeroed tail.  Decoded with rate_matched off and on (same input, same expected output),
    compared group by group with the oracle."""
    from python_5gtoolbox_amd.nr_ldpc_decode_mixed import MixedBatch
    groups = []
    for k, Zc in enumerate(S.ZLIST):
        _, llr = S.sweep_input(bg, Zc, "mixed-" + tag, 3, dtype, S.n_zeroed(Zc) if k % 2 == 0 else 0)
        groups.append((Zc, llr))
    mb = MixedBatch([(bg, Zc, torch.from_numpy(llr).cuda()) for Zc, llr in groups])
    ref = [S.oracle_decode(llr, bg, Zc, schedule) for Zc, llr in groups]
    for rm in (False, True):
        ck, st, it = (x.cpu().numpy() for x in mb.decode(S.L, S.ALPHA, S.BETA, schedule, rm))
        k = 0
        for (Zc, llr), r in zip(groups, ref):
            for row in range(3):
                co, nf = mb.rows[k]
                assert np.array_equal(ck[co:co + nf], r[0][row]), (bg, Zc, row, rm)
                assert st[k] == r[1][row] and it[k] == r[2][row], (bg, Zc, row, rm)
                k += 1


# ---------------------------------------------------------------------------------- BF / BP
BF_SNR = (3.0, 9.0)   # dB; bit flipping converges in 20 ... 60 iterations there, or not at all
BF_L = 64


@PAIR
def test_bf_vs_oracle(dec, pair):
    bg, Zc = pair
    _, llr = S.sweep_input(bg, Zc, "bf", 5, np.float64, snr_range=BF_SNR)
    got = dec.nr_decode_ldpc_batch(llr, Zc, bg, BF_L, "BF")
    _same(got, O.decode_bf(llr, Zc, bg, BF_L), (bg, Zc))


@PAIR
def test_bp_vs_oracle(dec, pair):
    """The GPU's tanh / atanh are not numpy's: status equal, ck and iters equal wherever the
    oracle converged (the bar of test_decode_bp_batch_vs_oracle)."""
    bg, Zc = pair
    _, llr = S.sweep_input(bg, Zc, "bp", 5, np.float64)
    got = dec.nr_decode_ldpc_batch(llr, Zc, bg, S.L, "BP")
    ref = O.decode_bp(llr, Zc, bg, S.L)
    assert np.array_equal(got[1], ref[1]), (bg, Zc)
    ok = ref[1]
    assert np.array_equal(got[0][ok], ref[0][ok]) and np.array_equal(got[2][ok], ref[2][ok]), (bg, Zc)


# ----------------------------------------------------------------------------------- encode
@PAIR
def test_encode_vs_oracle(torch, enc, pair):
    """33 codeblocks, every third with filler bits: contiguous, and through an odd-offset view of
    rows with an odd stride into a sentinel-filled output whose padding must stay untouched."""
    bg, Zc = pair
    Kb, Nb = S.DIMS[bg][:2]
    K, N = Kb * Zc, Nb * Zc
    rng = np.random.default_rng([bg, Zc, 33])
    ck = rng.integers(0, 2, (33, K)).astype(np.int8)
    for b in range(0, 33, 3):
        ck[b, K - int(rng.integers(1, K - 2 * Zc)):] = -1
    ref = O.encode(ck, bg)
    assert np.array_equal(enc.encode_ldpc_batch(ck, bg), ref), (bg, Zc)
    src = torch.full((33, K + 7), 9, dtype=torch.int8, device="cuda")
    src[:, 3:3 + K] = torch.from_numpy(ck).cuda()
    out = torch.full((33, N + 5), 7, dtype=torch.int8, device="cuda")
    enc.encode_ldpc_batch(src[:, 3:3 + K], bg, out=out)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :N], ref) and (got[:, N:] == 7).all(), (bg, Zc)
