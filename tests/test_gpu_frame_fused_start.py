"""GPU tests of the frame kernel's fused start (ldpc5g_dec_frame_iter.h, FUSED): for BG1 the float64
Zc = 384 flooding decoder runs iteration 0 and iteration 1's check-node pass as one walk over the
rows.  Every case is bit-exact (ck, status, iters) with the oracle's float64 decode_flooding.

All cases are BG1 at Zc = 384 (the only size the kernel runs) with at most four distinct codeblocks,
and reach the kernel two ways as tests/test_gpu_frame_first_iter.py does: through a mixed plan, and
with the rows repeated to 32 through the batch call.  What that file does not pin down:
an exit exactly at iteration 1, L = 2 and 3 (the state the fused start leaves, read by the final
pass and by a general iteration), ties against the punctured edge, and BG2 rows (the plain peeled
iteration) in the same mixed plan as BG1 rows.
"""
import numpy as np
import pytest

from oracle import ldpc_oracle as O

pytestmark = pytest.mark.gpu

ZC = 384
REP = 8   # 4 codeblocks x 8 = 32 rows: the batch call's frame kernel
NMS, OMS, NEG = (0.75, 0.0), (1.0, 0.5), (-0.75, 0.0)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a ROCm GPU"
    return t


@pytest.fixture(scope="module")
def dec():
    from python_5gtoolbox_amd import nr_ldpc_decode
    return nr_ldpc_decode


@pytest.fixture(scope="module")
def mx():
    from python_5gtoolbox_amd import nr_ldpc_decode_mixed
    return nr_ldpc_decode_mixed


_CW = {}


def _codewords(bg):
    """Four codewords of base graph bg (encoded once per module); codeword 2 has all-zero punctured
    bits, the others random ones."""
    if bg not in _CW:
        rng = np.random.default_rng(2000 + bg)
        ck = rng.integers(0, 2, (4, (22 if bg == 1 else 10) * ZC)).astype(np.int8)
        ck[2, :2 * ZC] = 0
        assert ck[0, :2 * ZC].any() and ck[1, :2 * ZC].any()
        dn = O.encode(ck, bg)
        dn.setflags(write=False)
        _CW[bg] = dn
    return _CW[bg]


def _awgn(dn, snr_db, rng):
    return np.asarray(O.bpsk_awgn_llr(dn, snr_db, rng), np.float64)


def _llr_exit1(bg=1):
    """Two noiseless codewords with nonzero punctured bits (the raw syndrome fails, the syndrome of
    LQ after iteration 0 passes: exit at iteration 1), one with zero punctured bits (exit at
    iteration 0), and -3 dB (never converges)."""
    dn = _codewords(bg)
    rng = np.random.default_rng(5 + bg)
    return np.stack([(1.0 - 2.0 * dn[0]) * 4.0, (1.0 - 2.0 * dn[1]) * 4.0, (1.0 - 2.0 * dn[2]) * 4.0,
                     _awgn(dn[3], -3.0, rng)])


def _llr_channel(bg=1):
    """-3 dB, 1 dB, 2 dB, 3 dB."""
    dn = _codewords(bg)
    rng = np.random.default_rng(17 + bg)
    return np.stack([_awgn(dn[k], snr, rng) for k, snr in enumerate((-3.0, 1.0, 2.0, 3.0))])


def _llr_ties(bg=1):
    """Every |LLR| ties with the punctured edge's candidates: +-1 with 5 % sign flips (twice), and
    integer LLRs in [-4, 4] with planted -0.0 (twice, different codewords)."""
    dn = _codewords(bg)
    rng = np.random.default_rng(29 + bg)
    out = []
    for k in (0, 1):
        out.append((1.0 - 2.0 * dn[k]) * np.where(rng.random(dn[k].shape) < 0.05, -1.0, 1.0))
    for k in (2, 3):
        c = ((1 - 2 * dn[k]) * rng.integers(0, 4, dn[k].shape) + rng.integers(-1, 2, dn[k].shape)).astype(np.float64)
        assert np.abs(c).max() <= 4
        c[::19] = -0.0
        out.append(c)
    return np.stack(out)


def _same(got, ref, what):
    for k in range(len(ref[0])):
        assert np.array_equal(np.asarray(got[0][k]), ref[0][k]), (what, k, "ck")
    assert np.array_equal(np.asarray(got[1], bool), ref[1]), (what, "status", got[1], ref[1])
    assert np.array_equal(np.asarray(got[2]), ref[2]), (what, "iters", got[2], ref[2])


def _check(dec, mx, llr, L, alpha, beta, bg=1):
    ref = O.decode_flooding(llr, ZC, bg, L, alpha, beta, np.float64)
    got = mx.decode_mixed([(bg, ZC, row) for row in llr], L, alpha, beta, "flooding")
    _same(got, ref, ("mixed plan", L, alpha, beta))
    got = dec.nr_decode_ldpc_batch(np.tile(llr, (REP, 1)), ZC, bg, L, "min-sum", alpha, beta, "flooding")
    _same(got, tuple(np.tile(r, (REP,) + (1,) * (r.ndim - 1)) for r in ref), ("batch", L, alpha, beta))
    return ref


@pytest.mark.parametrize("L", [2, 3, 8])
def test_fused_start_exit_at_iteration_1(torch, dec, mx, L):
    """Noiseless codewords whose punctured bits are not all zero leave at iteration 1 with the
    decisions of LQ after iteration 0."""
    llr = _llr_exit1()
    for alpha, beta in (NMS, OMS, NEG):
        ref = _check(dec, mx, llr, L, alpha, beta)
        if alpha > 0:
            assert ref[1][0] and ref[2][0] == 1 and ref[1][1] and ref[2][1] == 1
        assert ref[1][2] and ref[2][2] == 0
        assert ref[2][3] == L


@pytest.mark.parametrize("L", [2, 3])
def test_fused_start_short_runs(torch, dec, mx, L):
    """L = 2: the final pass reads the state the fused start leaves; L = 3: a general iteration
    reads it."""
    llr = _llr_channel()
    for alpha, beta in (NMS, OMS, NEG):
        _check(dec, mx, llr, L, alpha, beta)


@pytest.mark.parametrize("L", [2, 3, 8])
def test_fused_start_ties_against_punctured_edge(torch, dec, mx, L):
    """+-1 LLRs and small integers with planted -0.0: |q| of the punctured edge ties with the
    other edges' minima; NMS, OMS and alpha < 0."""
    llr = _llr_ties()
    for alpha, beta in (NMS, OMS, NEG):
        _check(dec, mx, llr, L, alpha, beta)


def test_fused_start_beside_bg2_in_one_plan(torch, mx):
    """BG1 rows (fused start) and BG2 rows (plain peeled iteration) in one mixed plan."""
    rng = np.random.default_rng(83)
    b1, b2 = _llr_exit1(1), _llr_channel(2)
    t1 = _llr_ties(1)
    items = [(1, ZC, b1[0]), (1, ZC, b1[3]), (1, ZC, t1[2]), (2, ZC, b2[0]), (2, ZC, b2[3]),
             (2, ZC, (1.0 - 2.0 * _codewords(2)[0]) * 4.0)]
    items = [items[i] for i in rng.permutation(len(items))]
    for L, (alpha, beta) in ((2, OMS), (8, NMS)):
        outs, st, it = mx.decode_mixed(items, L, alpha, beta, "flooding")
        for k, (bg, Zc, llr) in enumerate(items):
            ref = O.decode_flooding(llr[None], Zc, bg, L, alpha, beta, np.float64)
            assert np.array_equal(outs[k], ref[0][0]) and st[k] == ref[1][0] and it[k] == ref[2][0], (L, k, bg)
