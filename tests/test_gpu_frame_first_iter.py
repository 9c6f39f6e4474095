"""GPU tests of the frame kernel's peeled first iteration (ldpc5g_dec_frame_iter.h, FIRST): the
float64 Zc = 384 flooding decoder runs iteration 0 on the zero state with columns 0 and 1 known to
be +0.0.  Every case is bit-exact (ck, status, iters) with the oracle's float64 decode_ldpc.

Each case holds at most four distinct codeblocks, so the oracle runs in a fraction of a second.
They reach the frame kernel two ways: through a mixed plan (the work / cbs addressing, however few
codeblocks), and through the batch call with the four rows repeated to 32 — up to 24 BG1 / 28 BG2
float64 codeblocks the batch call takes the multi-workgroup kernel instead.
L = 1 returns the decisions right after the peeled iteration, L = 2 checks the state it leaves.
"""
import numpy as np
import pytest

from oracle import ldpc_oracle as O

pytestmark = pytest.mark.gpu

ZC = 384
REP = 8   # 4 codeblocks x 8 = 32 rows: the batch call's frame kernel
ALGOS = ((0.75, 0.0), (1.0, 0.5))   # NMS, OMS


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
    """Four codewords of base graph bg (encoded once per module)."""
    if bg not in _CW:
        rng = np.random.default_rng(1000 + bg)
        ck = rng.integers(0, 2, (4, (22 if bg == 1 else 10) * ZC)).astype(np.int8)
        ck[2, :2 * ZC] = 0   # punctured bits 0: its noiseless LLRs satisfy every check at once
        dn = O.encode(ck, bg)
        dn.setflags(write=False)
        _CW[bg] = dn
    return _CW[bg]


def _awgn(dn, snr_db, rng):
    return np.asarray(O.bpsk_awgn_llr(dn, snr_db, rng), np.float64)


def _llr_channel(bg):
    """-3 dB (never converges), 1 dB, noiseless (exit at iteration 0), 3 dB (early exit)."""
    dn = _codewords(bg)
    rng = np.random.default_rng(11 + bg)
    return np.stack([_awgn(dn[0], -3.0, rng), _awgn(dn[1], 1.0, rng), (1.0 - 2.0 * dn[2]) * 4.0,
                     _awgn(dn[3], 3.0, rng)])


def _llr_zeros(bg):
    """Planted zeros and ties: -0.0 and +0.0 scattered over core columns >= 2 and extension columns
    at -3 dB; a whole core column +0.0 and a whole extension column -0.0 at 1 dB; integer LLRs in
    [-4, 4] (equal magnitudes in every row, zeros of both signs); +-1 with 5 % sign flips (every
    |LLR| in every row ties)."""
    dn = _codewords(bg)
    kb = 22 if bg == 1 else 10
    rng = np.random.default_rng(23 + bg)
    a = _awgn(dn[0], -3.0, rng)
    a[::17] = -0.0
    a[5::23] = 0.0
    b = _awgn(dn[1], 1.0, rng)
    b[3 * ZC:4 * ZC] = 0.0                       # core column 5
    b[(kb + 7) * ZC:(kb + 8) * ZC] = -0.0        # an extension column (live: not +0.0)
    c = ((1 - 2 * dn[2]) * rng.integers(0, 4, dn[2].shape) + rng.integers(-1, 2, dn[2].shape)).astype(np.float64)
    c[::19] = -0.0
    d = (1.0 - 2.0 * dn[3]) * np.where(rng.random(dn[3].shape) < 0.05, -1.0, 1.0)
    return np.stack([a, b, c, d])


def _llr_rate_matched(bg):
    """Never-transmitted (+0.0) extension columns: the last 20; the last 7 but one live entry; one
    dead column between live ones and -0.0 (live) in the tail; none dead."""
    dn = _codewords(bg)
    kb = 22 if bg == 1 else 10
    rng = np.random.default_rng(37 + bg)
    x = np.stack([_awgn(dn[0], 1.0, rng), _awgn(dn[1], -3.0, rng), _awgn(dn[2], 2.0, rng), _awgn(dn[3], 1.0, rng)])
    x[0, -20 * ZC:] = 0.0
    x[1, -7 * ZC:] = 0.0
    x[1, -1] = 1.5
    x[2, (kb + 10) * ZC:(kb + 11) * ZC] = 0.0
    x[2, -3 * ZC:] = -0.0
    return x


def _same(got, ref, what):
    for k in range(len(ref[0])):
        assert np.array_equal(np.asarray(got[0][k]), ref[0][k]), (what, k, "ck")
    assert np.array_equal(np.asarray(got[1], bool), ref[1]), (what, "status", got[1], ref[1])
    assert np.array_equal(np.asarray(got[2]), ref[2]), (what, "iters", got[2], ref[2])


def _check(dec, mx, bg, llr, L, alpha, beta, rm=False):
    ref = O.decode_flooding(llr, ZC, bg, L, alpha, beta, np.float64)
    got = mx.decode_mixed([(bg, ZC, row) for row in llr], L, alpha, beta, "flooding", rate_matched=rm)
    _same(got, ref, ("mixed plan", bg, L, alpha, beta, rm))
    got = dec.nr_decode_ldpc_batch(np.tile(llr, (REP, 1)), ZC, bg, L, "min-sum", alpha, beta, "flooding",
                                   rate_matched=rm)
    _same(got, tuple(np.tile(r, (REP,) + (1,) * (r.ndim - 1)) for r in ref), ("batch", bg, L, alpha, beta, rm))
    return ref


@pytest.mark.parametrize("L", [1, 2, 8])
@pytest.mark.parametrize("bg", [1, 2])
def test_first_iter_channel(torch, dec, mx, bg, L):
    """AWGN at -3 dB, 1 dB and 3 dB and a noiseless codeword, NMS and OMS."""
    llr = _llr_channel(bg)
    for alpha, beta in ALGOS:
        ref = _check(dec, mx, bg, llr, L, alpha, beta)
        assert ref[1][2] and ref[2][2] == 0   # the noiseless codeword leaves at iteration 0
        if L == 8:
            assert not ref[1][0] and ref[2][0] == 8 and ref[1][3] and 0 < ref[2][3] < 8


@pytest.mark.parametrize("L", [1, 2, 8])
@pytest.mark.parametrize("bg", [1, 2])
def test_first_iter_planted_zeros_and_ties(torch, dec, mx, bg, L):
    """-0.0 / +0.0 in core and extension columns, a zero core column, ties in |LLR|."""
    llr = _llr_zeros(bg)
    for alpha, beta in ALGOS:
        _check(dec, mx, bg, llr, L, alpha, beta)


@pytest.mark.parametrize("L", [1, 2, 8])
@pytest.mark.parametrize("bg", [1, 2])
def test_first_iter_rate_matched(torch, dec, mx, bg, L):
    """rate_matched=True (the dead-row variant) on codeblocks with dead extension rows and with
    different liveness per codeblock; and the same rows through the plain variant."""
    llr = _llr_rate_matched(bg)
    for alpha, beta in ALGOS:
        _check(dec, mx, bg, llr, L, alpha, beta, rm=True)
    _check(dec, mx, bg, llr, L, 0.75, 0.0, rm=False)


def _oracle_full(full, bg, L, a, b):
    """The oracle's flooding decode with caller-given LLRs on every column, columns 0 and 1
    included (decode_ldpc on a full-length row)."""
    g = O.graph(bg, ZC)
    T = np.float64
    Lfull = full[None].astype(T)
    LQ = Lfull.copy()
    Lr = [np.zeros((1, g.rs[i + 1] - g.rs[i], ZC), T) for i in range(g.Mb)]
    for it in range(L):
        hd = LQ < 0
        if not O._row_hd_fail(hd, g)[0]:
            return hd[0].astype(np.int8), True, it
        acc = np.zeros_like(LQ)
        for i in range(g.Mb):
            cols = g.rows_cols(i)
            Lr[i] = O._cn_update(LQ[:, cols] - Lr[i], T(a), T(b), T)
            acc[:, cols] += Lr[i]
        LQ = Lfull + acc
    hd = LQ <= 0
    return hd[0].astype(np.int8), not O._row_hd_fail(hd, g)[0], L


@pytest.mark.parametrize("bg", [1, 2])
def test_first_iter_full_length(torch, dec, bg):
    """A full-length call (pc == 0): columns 0 and 1 carry nonzero LLRs, so nothing about them may
    be assumed; two noisy rows and a noiseless one, L = 1 and 8."""
    g = O.graph(bg, ZC)
    rng = np.random.default_rng(53 + bg)
    rows = []
    for k, snr in enumerate((-3.0, 1.0, None)):
        # a full codeword needs the two punctured systematic columns: re-encode known info bits
        ck = rng.integers(0, 2, (1, g.K)).astype(np.int8)
        cw = np.concatenate([ck[0, :2 * ZC], O.encode(ck, bg)[0]])
        rows.append((1.0 - 2.0 * cw) * 4.0 if snr is None else _awgn(cw, snr, rng))
    full = np.stack(rows)
    assert np.count_nonzero(full[:, :2 * ZC]) == full[:, :2 * ZC].size
    for L, (alpha, beta) in ((1, ALGOS[0]), (8, ALGOS[0]), (8, ALGOS[1])):
        ck, st, it = dec.nr_decode_ldpc_batch(np.tile(full, (10, 1)), ZC, bg, L, "min-sum", alpha, beta,
                                              "flooding", full=True)
        refs = [_oracle_full(row, bg, L, alpha, beta) for row in full]
        for k in range(30):
            rck, rst, rit = refs[k % 3]
            assert np.array_equal(ck[k], rck) and st[k] == rst and it[k] == rit, (L, alpha, beta, k)
        assert refs[2][1] and refs[2][2] == 0


def test_first_iter_mixed_plan_two_codeblocks(torch, mx):
    """Two float64 Zc = 384 codeblocks of each base graph among small codeblocks of one mixed plan
    (their own frame-kernel launch addressed through work / cbs)."""
    rng = np.random.default_rng(71)
    items = []
    for bg in (1, 2):
        llr = _llr_channel(bg)
        items += [(bg, ZC, llr[0]), (bg, ZC, llr[1])]
        for Zc in (12, 40):
            dn = O.encode(rng.integers(0, 2, (2, (22 if bg == 1 else 10) * Zc)).astype(np.int8), bg)
            items += [(bg, Zc, _awgn(dn[k], 1.0, rng)) for k in range(2)]
    items = [items[i] for i in rng.permutation(len(items))]
    for L, (alpha, beta) in ((1, ALGOS[1]), (8, ALGOS[0])):
        outs, st, it = mx.decode_mixed(items, L, alpha, beta, "flooding")
        for k, (bg, Zc, llr) in enumerate(items):
            ref = O.decode_flooding(llr[None], Zc, bg, L, alpha, beta, np.float64)
            assert np.array_equal(outs[k], ref[0][0]) and st[k] == ref[1][0] and it[k] == ref[2][0], (L, k, bg, Zc)


@pytest.mark.parametrize("bg", [1, 2])
def test_first_iter_L0(torch, dec, mx, bg):
    """L = 0 runs no iteration, peeled or not: the final pass reads the zero state straight from
    the prologue, so its LDS rows must be filled.  320 rows (more workgroups than CUs) after an
    L = 8 launch of the same shape, so the LDS a workgroup finds holds an earlier one's state."""
    llr = _llr_channel(bg)
    big = np.tile(llr, (80, 1))
    dec.nr_decode_ldpc_batch(big, ZC, bg, 8, "min-sum", 0.75, 0.0, "flooding")
    for alpha, beta in ALGOS:
        ref = O.decode_flooding(llr, ZC, bg, 0, alpha, beta, np.float64)
        got = dec.nr_decode_ldpc_batch(big, ZC, bg, 0, "min-sum", alpha, beta, "flooding")
        _same(got, tuple(np.tile(r, (80,) + (1,) * (r.ndim - 1)) for r in ref), ("batch L=0", bg, alpha, beta))
        got = mx.decode_mixed([(bg, ZC, row) for row in llr], 0, alpha, beta, "flooding")
        _same(got, ref, ("mixed plan L=0", bg, alpha, beta))


@pytest.mark.parametrize("L", [1, 2, 8])
@pytest.mark.parametrize("bg", [1, 2])
def test_first_iter_negative_alpha(torch, dec, mx, bg, L):
    """alpha < 0: the zero minimum's message alpha * 0 is -0.0, which still takes the peeled
    iteration (its dropped messages are -+0, its kept ones change sign)."""
    for llr in (_llr_channel(bg), _llr_zeros(bg)):
        _check(dec, mx, bg, llr, L, -0.75, 0.0)
        _check(dec, mx, bg, llr, L, -1.0, 0.5)


@pytest.mark.parametrize("bg", [1, 2])
def test_first_iter_guard_not_zero_message(torch, dec, mx, bg):
    """The peeled iteration's guard: with alpha = inf the zero minimum's message alpha * 0 is NaN,
    not +-0, so iteration 0 must take the general path (beta < 0, the other way to a nonzero
    message, is refused by the API).  Every row with a punctured column then sends NaN to its
    other columns, which the peeled path would have dropped.  L = 1 only: one check-node update
    on finite inputs, sums in the reference's order (inf - inf = NaN on both sides), decisions
    NaN <= 0 = 0; a second iteration would take minima of NaNs, where fmin and numpy differ."""
    llr = _llr_channel(bg)
    with np.errstate(invalid="ignore"):
        _check(dec, mx, bg, llr, 1, np.inf, 0.0)
