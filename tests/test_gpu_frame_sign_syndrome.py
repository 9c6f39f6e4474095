"""GPU tests of two steps of the float64 Zc = 384 frame kernel (ldpc5g_dec_frame.h,
ldpc5g_dec_frame_iter.h): the general check-node pass keeps a row's old and new sign bits in one
shift register, and the pass after the last iteration takes the syndrome of the decisions as
384-bit vectors (a table of 64-bit windows) instead of walking every edge in float64.  Every case
is bit-exact (ck, status, iters) with the oracle's float64 decode_flooding.

All cases run at Zc = 384 (the only size the kernel runs).  The sign-word cases use four distinct
codeblocks per base graph and reach the kernel two ways as tests/test_gpu_frame_fused_start.py
does: a mixed plan, and the rows repeated to 32 through the batch call.

Sign-word formats (FramePlan::ph, from the plan's rule: in each half, the VGPR rows in row order;
a row of degree > 12 has a word of its own, format 0; the others pair up, the first of a pair in
format 1 (low field), the second in format 2 (high field, the one whose register carries the
other row's field above the new signs)).  Every VGPR row of either base graph has degree <= 10,
so each half's VGPR rows alternate formats 1 and 2.  The plan as compiled (printed from the
constexpr tables on the host):
  BG1: LDS rows 0-3 (degree 19), 5, 7, 8, 9, 11, 12; format 2: rows 10, 13, 16, 17, 20, 21, 24, 25,
       28, 29, 32, 33, 36, 37, 40, 41, 44, 45; format 1: the other 18 VGPR rows.
  BG2: LDS rows 0, 2, 4, 5, 8, 10, 13, 19; format 2: rows 6, 7, 12, 15, 16, 20, 21, 24, 25, 27, 30,
       31, 34, 35, 37, 40; format 1: the other 18 VGPR rows (rows 1 and 3, degree 10, among them).
Format 0 (a VGPR row of degree > 12) occurs in neither 5G base graph: the rows of degree > 12 are
LDS rows; its register layout (p << (32 - d)) is format 1's and the LDS rows'.
"""
import numpy as np
import pytest

from oracle import ldpc_oracle as O

pytestmark = pytest.mark.gpu

ZC = 384
REP = 8   # 4 codeblocks x 8 = 32 rows: the batch call's frame kernel
NMS, OMS, NEG = (0.75, 0.0), (1.0, 0.5), (-0.75, 0.0)
KB = {1: 22, 2: 10}


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


_CW, _REF = {}, {}


def _codewords(bg):
    """Four random codewords of base graph bg (encoded once per module)."""
    if bg not in _CW:
        rng = np.random.default_rng(3100 + bg)
        ck = rng.integers(0, 2, (4, KB[bg] * ZC)).astype(np.int8)
        dn = O.encode(ck, bg)
        dn.setflags(write=False)
        _CW[bg] = dn
    return _CW[bg]


# SNRs (dB) of the four codeblocks: -3 dB never converges; the others leave at different iterations
SNRS = {1: (-3.0, 2.0, 3.0, 4.0), 2: (-3.0, -1.0, 0.0, 1.0)}


def _llr(bg, ndead):
    """-3 dB and three SNRs with exits at different iterations; ndead > 0: the last ndead extension
    columns were never transmitted (+0.0, rate recovery's fill)."""
    dn = _codewords(bg)
    rng = np.random.default_rng(41 + bg)
    llr = np.stack([np.asarray(O.bpsk_awgn_llr(dn[k], snr, rng), np.float64) for k, snr in enumerate(SNRS[bg])])
    if ndead:
        llr[:, -ndead * ZC:] = 0.0
    llr.setflags(write=False)
    return llr


def _ref(bg, ndead, L, ab):
    key = (bg, ndead, L, ab)
    if key not in _REF:
        _REF[key] = O.decode_flooding(_llr(bg, ndead), ZC, bg, L, ab[0], ab[1], np.float64)
    return _REF[key]


def _same(got, ref, what):
    for k in range(len(ref[0])):
        assert np.array_equal(np.asarray(got[0][k]), ref[0][k]), (what, k, "ck")
    assert np.array_equal(np.asarray(got[1], bool), ref[1]), (what, "status", got[1], ref[1])
    assert np.array_equal(np.asarray(got[2]), ref[2]), (what, "iters", got[2], ref[2])


def _check(dec, mx, bg, ndead, L, ab, rm):
    llr, ref = _llr(bg, ndead), _ref(bg, ndead, L, ab)
    got = mx.decode_mixed([(bg, ZC, row) for row in llr], L, ab[0], ab[1], "flooding", rate_matched=rm)
    _same(got, ref, ("mixed plan", bg, ndead, L, ab, rm))
    got = dec.nr_decode_ldpc_batch(np.tile(llr, (REP, 1)), ZC, bg, L, "min-sum", ab[0], ab[1], "flooding",
                                   rate_matched=rm)
    _same(got, tuple(np.tile(r, (REP,) + (1,) * (r.ndim - 1)) for r in ref), ("batch", bg, ndead, L, ab, rm))
    return ref


@pytest.mark.parametrize("L", [3, 8])
@pytest.mark.parametrize("bg", [1, 2])
def test_merged_sign_word_plain(torch, dec, mx, bg, L):
    """The plain kernels: the general check-node pass runs at least once after the peeled start
    (L = 3) and six times (L = 8); NMS, OMS and alpha < 0."""
    for ab in (NMS, OMS, NEG):
        ref = _check(dec, mx, bg, 0, L, ab, False)
        assert ref[2][0] == L and not ref[1][0]   # -3 dB: status 0 through the final pass
        if L == 8 and ab == NMS:
            # exits inside the general loop, at more than one iteration
            mid = {int(i) for i in ref[2] if 2 <= i < L}
            assert len(mid) >= 2, ref[2]


@pytest.mark.parametrize("ndead", [0, 12])
@pytest.mark.parametrize("L", [3, 8])
@pytest.mark.parametrize("bg", [1, 2])
def test_merged_sign_word_rate_matched(torch, dec, mx, bg, L, ndead):
    """The rate-matched kernels' two loop copies: a codeblock with dead extension rows (the last 12
    extension columns never transmitted) takes the dead-row copy, one with none the plain copy."""
    for ab in (NMS, OMS, NEG):
        ref = _check(dec, mx, bg, ndead, L, ab, True)
        assert ref[2][0] == L and not ref[1][0]


# ---- the final pass's syndrome: false alarms and misses, L = 0 (the pass reads the decisions of
# ---- the input LLRs: LQ <= 0, the punctured columns' +0.0 decide 1)
def _syndrome_set(bg):
    """A noiseless codeword whose punctured 2 Zc bits are all 1 (clean: status 1), copies with the
    sign of one extension-column LLR flipped, one per (extension row, 64-entry word) at entries
    that include 0, 63, 64 and 383 (each breaks exactly one check), and copies with one core-column
    flip at word boundaries."""
    g = O.graph(bg, ZC)
    rng = np.random.default_rng(7000 + bg)
    ck = rng.integers(0, 2, KB[bg] * ZC).astype(np.int8)
    ck[:2 * ZC] = 1
    base = (1.0 - 2.0 * O.encode(ck, bg).astype(np.float64)) * 4.0
    flips = []
    for i in range(4, g.Mb):
        for w in range(6):
            flips.append(((KB[bg] + i) * ZC + 64 * w + (63 if (i + w) % 2 else 0)))
    ents = {f % ZC for f in flips}
    assert {0, 63, 64, 383} <= ents
    for j in (2, 3, KB[bg] - 1, KB[bg], KB[bg] + 3):
        for z in (0, 63, 64, 383):
            flips.append(j * ZC + z)
    llr = np.tile(base, (2 + len(flips), 1))
    for n, f in enumerate(flips):
        llr[2 + n, f - 2 * ZC] *= -1.0
    return llr, len(flips)


@pytest.mark.parametrize("rm", [False, True])
@pytest.mark.parametrize("bg", [1, 2])
def test_final_syndrome_single_flips(torch, dec, mx, bg, rm):
    llr, nf = _syndrome_set(bg)
    ref = O.decode_flooding(llr, ZC, bg, 0, 0.75, 0.0, np.float64)
    assert ref[1][0] and ref[1][1] and not ref[1][2:].any() and (ref[2] == 0).all()
    got = dec.nr_decode_ldpc_batch(llr, ZC, bg, 0, "min-sum", 0.75, 0.0, "flooding", rate_matched=rm)
    bad = np.nonzero(np.asarray(got[1], bool) != ref[1])[0]
    assert bad.size == 0, ("status", bg, rm, bad[:16])
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
    # a few of them through a mixed plan
    pick = [0, 2, 3, 2 + nf // 2, 1 + nf]
    got = mx.decode_mixed([(bg, ZC, llr[k]) for k in pick], 0, 0.75, 0.0, "flooding", rate_matched=rm)
    _same(got, tuple(r[pick] for r in ref), ("mixed plan", bg, rm))


@pytest.mark.parametrize("bg", [1, 2])
def test_final_syndrome_after_one_iteration(torch, dec, bg):
    """A subset of the same flips at L = 1: the raw syndrome fails (the punctured columns decide 0
    at `LQ < 0`), one iteration runs (BG1: the general loop from the zero state; BG2: the peeled
    iteration) and the final pass reads the decisions it leaves."""
    llr, nf = _syndrome_set(bg)
    llr = llr[np.r_[0:2, 2:2 + nf:7, 2 + nf - 20:2 + nf]]
    ref = O.decode_flooding(llr, ZC, bg, 1, 0.75, 0.0, np.float64)
    assert (ref[2] == 1).all()
    got = dec.nr_decode_ldpc_batch(llr, ZC, bg, 1, "min-sum", 0.75, 0.0, "flooding")
    _same(got, ref, ("batch", bg))
