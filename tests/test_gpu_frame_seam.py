"""GPU tests of the seam between two iterations of the float64 Zc = 384 frame kernel
(ldpc5g_dec_frame.h, ldpc5g_dec_frame_iter.h, LDPC5G_FR_SEAM): in the plain kernels the loop closes
with a plain barrier instead of a vote through LDS, the LQ update's core LLRs go out before the
syndrome flag is read, the LQ update reads all its own entries before the first add, and phase A's
waves set their issue priority row by row.  All of it is bit-neutral, so every case is bit-exact
(ck, status, iters) with the oracle's float64 decode_flooding.  The rate-matched kernels keep
their code; their cases guard the shared header.

The seam runs once per iteration and differs on the loop's first trip (after BG1's fused start it
skips phase A), on the last trip and on an early exit, so the cases are a few codeblocks at
Zc = 384 (the only size the kernel runs) over every way of entering and leaving the loop.  A
codeblock reaches the frame kernel two ways, as in tests/test_gpu_frame_sign_syndrome.py: through a
mixed plan (work / cbs, any number of codeblocks) and through the batch call with the rows repeated
to 32 or more (fewer go to the multi-workgroup decoder).

tests/golden/decode_golden.npz holds its `ties` and `zeros` kinds only at Zc <= 26 (gen_golden.py),
none at Zc = 384, so there is nothing of those kinds for this kernel to read.
"""
import numpy as np
import pytest

from oracle import ldpc_oracle as O

pytestmark = pytest.mark.gpu

ZC = 384
NMS, OMS = (0.75, 0.0), (1.0, 0.5)
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


_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _MEMO[key] = v
    return _MEMO[key]


def _noisy(bg):
    """Three codeblocks at -3 dB: none converges within 8 iterations."""
    def make():
        rng = np.random.default_rng(5100 + bg)
        dn = O.encode(rng.integers(0, 2, (3, KB[bg] * ZC)).astype(np.int8), bg)
        return np.stack([np.asarray(O.bpsk_awgn_llr(dn[k], -3.0, rng), np.float64) for k in range(3)])
    return _memo(("noisy", bg), make)


# SNRs (dB) of the early-exit batch; codeblock 0 has zero punctured bits, so its raw LLRs already
# satisfy every check (the loop's test decides a punctured +0.0 as 0)
EXIT_SNRS = (40.0, 40.0, 14.0, 12.0, 10.0, 9.0, 8.0, 7.0, -3.0, -3.0)


def _exits(bg):
    def make():
        rng = np.random.default_rng(5200 + bg)
        ck = rng.integers(0, 2, (len(EXIT_SNRS), KB[bg] * ZC)).astype(np.int8)
        ck[0, :2 * ZC] = 0
        dn = O.encode(ck, bg)
        return np.stack([np.asarray(O.bpsk_awgn_llr(dn[k], s, rng), np.float64) for k, s in enumerate(EXIT_SNRS)])
    return _memo(("exits", bg), make)


def _ref(name, llr, bg, L, ab):
    return _memo(("ref", name, bg, L, ab), lambda: O.decode_flooding(llr, ZC, bg, L, ab[0], ab[1], np.float64))


def _same(got, ref, what):
    for k in range(len(ref[0])):
        assert np.array_equal(np.asarray(got[0][k]), ref[0][k]), (what, k, "ck")
    assert np.array_equal(np.asarray(got[1], bool), ref[1]), (what, "status", got[1], ref[1])
    assert np.array_equal(np.asarray(got[2]), ref[2]), (what, "iters", got[2], ref[2])


def _both_ways(dec, mx, bg, llr, ref, L, ab, rm, what):
    """The rows through a mixed plan, and repeated to >= 32 rows through the batch call."""
    got = mx.decode_mixed([(bg, ZC, row) for row in llr], L, ab[0], ab[1], "flooding", rate_matched=rm)
    _same(got, ref, ("mixed plan",) + what)
    rep = -(-32 // len(llr))
    got = dec.nr_decode_ldpc_batch(np.tile(llr, (rep, 1)), ZC, bg, L, "min-sum", ab[0], ab[1], "flooding",
                                   rate_matched=rm)
    _same(got, tuple(np.tile(r, (rep,) + (1,) * (r.ndim - 1)) for r in ref), ("batch",) + what)


@pytest.mark.parametrize("L", [0, 1, 2, 3, 8])
@pytest.mark.parametrize("bg", [1, 2])
def test_no_convergence(torch, dec, mx, bg, L):
    """-3 dB, B = 1 and 3, NMS and OMS (the OFS kernels).  L = 0: no iteration; L = 1: BG1 takes
    the general loop with no fused start, BG2 the peeled iteration alone; L = 2: the first trip
    after BG1's fused start (no phase A) is also the last; L = 3: one full trip follows it;
    L = 8: the headline's length."""
    for ab in (NMS, OMS):
        for B in (1, 3):
            llr = _noisy(bg)[:B]
            ref = _ref(("noisy", B), llr, bg, L, ab)
            assert (ref[2] == L).all() and not ref[1].any()
            _both_ways(dec, mx, bg, llr, ref, L, ab, False, (bg, B, L, ab))


@pytest.mark.parametrize("rm", [False, True])
@pytest.mark.parametrize("bg", [1, 2])
def test_early_exit_at_every_trip(torch, dec, mx, bg, rm):
    """Codeblocks that leave at iters = 0 (the raw LLRs' syndrome), 1, 2 and later, beside ones that
    never converge, in one batch: a workgroup that leaves the loop has loaded the LQ update's LLRs
    for nothing.
    rm: the same rows through the rate-matched kernels' plain loop copy (no dead row)."""
    llr = _exits(bg)
    for ab in (NMS, OMS):
        ref = _ref("exits", llr, bg, 8, ab)
        its = set(int(i) for i in ref[2])
        assert {0, 1, 2, 8} <= its and any(2 < i < 8 for i in its), ref[2]
        assert ref[1][ref[2] < 8].all() and not ref[1][-2:].any()
        _both_ways(dec, mx, bg, llr, ref, 8, ab, rm, (bg, ab, rm))
    # and with fewer iterations than some exits need: the last trip decides them
    for L in (2, 3):
        ref = _ref("exits", llr, bg, L, NMS)
        assert {0, 1, L} <= set(int(i) for i in ref[2])
        _both_ways(dec, mx, bg, llr, ref, L, NMS, rm, (bg, L, rm))


def _oracle_full(full, bg, L, a, b):
    """decode_flooding's loop (the oracle's own check-node update and syndrome) with caller-given
    LLRs on every column, columns 0 and 1 included: decode_ldpc on a full-length row."""
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
def test_full_length_input(torch, dec, bg):
    """pc == 0: LLRs on columns 0 and 1 too, so no iteration is peeled and the loop starts cold at
    it = 0; one row that never converges, two that leave early."""
    g = O.graph(bg, ZC)
    rng = np.random.default_rng(5300 + bg)
    rows = []
    for snr in (-3.0, 3.0, 9.0):
        ck = rng.integers(0, 2, (1, g.K)).astype(np.int8)
        cw = np.concatenate([ck[0, :2 * ZC], O.encode(ck, bg)[0]])
        rows.append(np.asarray(O.bpsk_awgn_llr(cw, snr, rng), np.float64))
    full = np.stack(rows)
    for L, ab in ((1, NMS), (2, NMS), (8, NMS), (8, OMS)):
        refs = [_oracle_full(row, bg, L, ab[0], ab[1]) for row in full]
        ck, st, it = dec.nr_decode_ldpc_batch(np.tile(full, (11, 1)), ZC, bg, L, "min-sum", ab[0], ab[1],
                                              "flooding", full=True)
        for k in range(33):
            rck, rst, rit = refs[k % 3]
            assert np.array_equal(ck[k], rck) and st[k] == rst and it[k] == rit, (bg, L, ab, k)
        if L == 8:
            assert refs[0][2] == 8 and 0 < refs[2][2] < refs[1][2] < 8, [r[2] for r in refs]


def _dead_rows(bg):
    """Rate-matched rows: codeblock 0 has every extension column live (the plain loop copy),
    1 and 2 never got their last 12 / 30 extension columns (the dead-row copy; 30 dead rows make
    whole barrier groups of extension rows skip their barrier), 3 is codeblock 2 at high SNR
    (an early exit from the dead-row copy)."""
    def make():
        rng = np.random.default_rng(5400 + bg)
        dn = O.encode(rng.integers(0, 2, (4, KB[bg] * ZC)).astype(np.int8), bg)
        llr = np.stack([np.asarray(O.bpsk_awgn_llr(dn[k], s, rng), np.float64)
                        for k, s in enumerate((-3.0, -3.0, -3.0, 9.0))])
        llr[1, -12 * ZC:] = 0.0
        llr[2:, -30 * ZC:] = 0.0
        return llr
    return _memo(("dead", bg), make)


@pytest.mark.parametrize("L", [1, 2, 8])
@pytest.mark.parametrize("bg", [1, 2])
def test_rate_matched_dead_rows(torch, dec, mx, bg, L):
    """The rate-matched kernels (no peeled start): both loop copies, a codeblock whose
    dead rows make whole groups skip their barrier, an early exit among them."""
    llr = _dead_rows(bg)
    for ab in (NMS, OMS):
        ref = _ref("dead", llr, bg, L, ab)
        assert (ref[2][:3] == L).all() and not ref[1][:3].any()
        if L == 8:
            assert 0 < ref[2][3] < 8 and ref[1][3], ref[2]
        _both_ways(dec, mx, bg, llr, ref, L, ab, True, (bg, L, ab))


@pytest.mark.parametrize("rm", [False, True])
def test_mixed_zc_plan_one_384_group(torch, mx, rm):
    """Three Zc = 384 codeblocks as one group of a mixed-Zc plan (the work / cbs path), behind and
    between small codeblocks that put their rows at uneven offsets: every row length (66 Zc, 50 Zc)
    is even, so an element offset is never odd; the BG2 Zc = 3 row in front makes the first one's
    LLR offset 150 elements (an odd multiple of 2; 1200 bytes, no multiple of 64) and its ck
    offset 156 bytes (no multiple of 16: the staged ck store's unaligned path)."""
    rng = np.random.default_rng(5500)
    big = _exits(1)[[8, 4, 1]]   # never converges, leaves at iteration 2, at iteration 1
    small = []
    for bg, Zc in ((2, 3), (1, 5), (2, 12)):
        dn = O.encode(rng.integers(0, 2, KB[bg] * Zc).astype(np.int8), bg)
        small.append((bg, Zc, np.asarray(O.bpsk_awgn_llr(dn, 1.0, rng), np.float64)))
    items = [small[0], (1, ZC, big[0]), small[1], (1, ZC, big[1]), (1, ZC, big[2]), small[2]]
    assert sum(it[2].size for it in items[:1]) == 150
    for ab in (NMS, OMS):
        got = mx.decode_mixed(items, 8, ab[0], ab[1], "flooding", rate_matched=rm)
        for k, (bg, Zc, llr) in enumerate(items):
            r = O.decode_flooding(llr[None], Zc, bg, 8, ab[0], ab[1], np.float64)
            assert np.array_equal(got[0][k], r[0][0]) and got[1][k] == r[1][0] and got[2][k] == r[2][0], (k, ab, rm)
        ref = _ref("exits", _exits(1), 1, 8, ab)
        assert [int(got[2][k]) for k in (1, 3, 4)] == [int(ref[2][j]) for j in (8, 4, 1)]
