"""Parity sweep of the polar codec against tests/polar_ref.py, bit for bit (ck, status, pm; encoded, rate-matched
and rate-recovered rows): the reference-recorded sweep fixture (960 shapes on a quarter-step LLR grid), a live
sweep of the whole chain with continuous noise, zero and saturated rows (E to 8192, K to 1023), N = 1024 across
the list size at which the decoder's largest layers move from LDS to the global workspace, the workspace
launch's workgroup loop (B beyond its 1024 workgroups), strided outputs with poisoned padding through the C
ABI, and repeatability.  The shape lists live in polar_ref.py; tests/test_polar_host.py checks the plans of
the same lists on the CPU.

N follows from (K, E), and N = 32 and 64 end at E = 36 and 72 (K >= 18 makes 8K > 128), so
E = 8192 is swept at N = 256, 512 and 1024 (32 wraps at most) and N = 32 and 64 at their longest E.  N = 1024
has neither PC bits (K <= 25) nor a distributed CRC (nMax = 9); its codewords die early only when every
candidate ties at the median, which the all-zero row does once the list is full.
"""
import functools
import os

import numpy as np
import pytest

import polar_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NS = (32, 64, 128, 256, 512, 1024)
CLASSES = ("early", "crc_fail", "not_best", "pc_kills", "median_ties", "crc_kills")
SWEEP_PER_N = 160


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def sweep_fixture():
    return R.load_sweep(os.path.join(GOLD, "polar_golden_sweep.npz"))


def cu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, what=""):
    """Bit for bit: same dtype, same shape, same values (inf == inf for the pm of a failed block)."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


def ref_decode(s, rr):
    """polar_ref over the rows of rr -> (ck [B, K] int8, status [B] uint8, pm [B] float64, [info])."""
    res = [R.decode(s["algo"], y, s["E"], s["K"], s["L"], s["nMax"], s["iIL"], s["CRCLEN"], s["padCRC"], s["rnti"])
           for y in rr]
    return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.uint8),
            np.array([r[2] for r in res], np.float64), [r[3] for r in res])


# --------------------------------------------------------------------------------- recorded sweep
@pytest.mark.parametrize("N", NS)
def test_recorded_sweep(torch, N):
    """rate_recover(reference_repetition=True) equals the recomputed reference row and decode equals the
    reference's (ck, status) and polar_ref's pm, for every case of the fixture."""
    from python_5gtoolbox_amd import polar
    allc = sweep_fixture()
    assert len(allc) == 6 * SWEEP_PER_N
    cases = [c for c in allc if c[0]["N"] == N]
    assert len(cases) == SWEEP_PER_N
    st = [c[0]["status"] for c in cases]
    assert sum(st) >= 3 and len(st) - sum(st) >= 3
    groups = {}
    for c in cases:
        groups.setdefault(tuple(c[0][k] for k in R.SWEEP_FIELDS), []).append(c)
    done = 0
    for key, lst in groups.items():
        s = dict(zip(R.SWEEP_FIELDS, key))
        p = polar.plan(*R.plan_args(s))
        assert p.N == N
        rr = polar.rate_recover(cu(torch, np.stack([c[1] for c in lst])), p, s["iBIL"], 20.0, reference_repetition=True)
        same(rr, np.stack([R.rate_recover(c[1], s["K"], N, s["iBIL"], 20.0, reference_repetition=True) for c in lst]), s)
        ck, status, pm = polar.decode(rr, p, s["algo"], s["L"])
        same(ck, np.stack([c[2] for c in lst]), s)
        same(status, np.array([c[0]["status"] for c in lst], np.uint8), s)
        same(pm, np.array([float.fromhex(c[0]["pm"]) for c in lst], np.float64), s)
        done += len(lst)
    assert done == SWEEP_PER_N


def test_recorded_sweep_holds_every_class():
    meta = [c[0] for c in sweep_fixture()]
    R.sweep_coverage(meta)
    for k in CLASSES:
        assert sum(1 for c in meta if c["info"][k]) >= 3, k


# ------------------------------------------------------------------------------------- live sweep
OFFSETS = (0.0, 2.5, 1.0)   # dB above the capacity limit of rate K / E: noisy, noisy, rounded to integers


@functools.lru_cache(maxsize=None)
def live(N):
    """The live sweep's inputs and polar_ref's result of every stage, for the shapes of one N.  Per shape: two
    noisy rows, one rounded to integers, one all-zero row; the first shape of each N also gets a saturated row."""
    out = []
    shapes = R.live_shapes()
    for i, s in enumerate(shapes):
        K, E, nMax, iIL, crclen, pad, rnti, iBIL = (s[k] for k in R.SWEEP_FIELDS[:8])
        if 1 << R.n_value(K, E, nMax) != N:
            continue
        rng = np.random.default_rng([R.LIVE_SEED, i])
        blk = np.stack([R.crc_attach(rng.integers(0, 2, K - crclen), crclen, rnti, pad) for _ in range(4)])
        enc = np.stack([R.encode(b, E, nMax, iIL) for b in blk])
        rm = np.stack([R.rate_match(d, K, E, iBIL) for d in enc])
        wf = R.waterfall_db(K, E)
        llr = np.stack([R.channel_llr(rng, rm[j], wf + OFFSETS[j]) for j in range(3)] + [np.zeros(E)])
        llr[2] = np.round(llr[2])
        if not out:
            llr = np.concatenate([llr, 20.0 * np.where(llr[:1] < 0, -1.0, 1.0)])
        rr = np.stack([R.rate_recover(x, K, N, iBIL, 20.0) for x in llr])
        rq = np.stack([R.rate_recover(x, K, N, iBIL, 20.0, reference_repetition=True) for x in llr])
        out.append(dict(s=s, blk=blk, enc=enc, rm=rm, llr=llr, rr=rr, rq=rq, dec=ref_decode(s, rr)))
    return out


def run_chain(torch, c):
    """The GPU's seven outputs for one live case, as numpy arrays."""
    from python_5gtoolbox_amd import polar
    s = c["s"]
    p = polar.plan(*R.plan_args(s))
    enc = polar.encode(cu(torch, c["blk"]), p)
    rm = polar.rate_match(enc, p, s["iBIL"])
    x = cu(torch, c["llr"])
    rr = polar.rate_recover(x, p, s["iBIL"])
    rq = polar.rate_recover(x, p, s["iBIL"], 20.0, reference_repetition=True)
    ck, st, pm = polar.decode(rr, p, s["algo"], s["L"])
    return [t.cpu().numpy() for t in (enc, rm, rr, rq, ck, st, pm)]


@pytest.mark.parametrize("N", NS)
def test_live_sweep(torch, N):
    cases = live(N)
    assert len(cases) >= R.LIVE_PER_N
    for c in cases:
        got = run_chain(torch, c)
        for g, w, name in zip(got, (c["enc"], c["rm"], c["rr"], c["rq"]) + c["dec"][:3],
                              ("encode", "rate_match", "rate_recover", "rate_recover(reference)", "ck", "status", "pm")):
            same(g, w, (name, c["s"]))


def test_live_sweep_reaches_every_class():
    """From polar_ref's own results: a quarter of the codewords succeed, a quarter fail, at least three of each
    in every N, every class of the decoder's bookkeeping at least three times; and the list covers what it says."""
    shapes = R.live_shapes()
    assert len(shapes) == 6 * R.LIVE_PER_N + len(R.LIVE_FORCED) >= 120
    R.sweep_coverage(shapes)
    assert {s["E"] for s in shapes} >= {8192, 8128, 2080} and max(s["K"] for s in shapes) == 1023
    assert max(s["L"] for s in shapes if R.n_value(s["K"], s["E"], s["nMax"]) == 10) == 16
    ok = total = 0
    have = dict.fromkeys(CLASSES, 0)
    for N in NS:
        st = np.concatenate([c["dec"][1] for c in live(N)])
        assert st.sum() >= 3 and (st == 0).sum() >= 3, (N, st)
        ok, total = ok + int(st.sum()), total + st.size
        for c in live(N):
            for info in c["dec"][3]:
                for k in CLASSES:
                    have[k] += bool(info[k])
    assert 4 * ok >= total and 4 * (total - ok) >= total, (ok, total)
    assert all(v >= 3 for v in have.values()), have


def test_live_sweep_repeats_bit_for_bit(torch):
    for c in live(128):
        a, b = run_chain(torch, c), run_chain(torch, c)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), c["s"]


# ------------------------------------------------------------- N = 1024: LDS / workspace switch
LDS_MAX = 160 * 1024
WS_SLOTS = 1024
SWITCH_L = (16, 17, 18, 19, 20, 21, 24, 31, 32)
BIG = dict(K=211, E=1024, nMax=10, iIL=0, CRCLEN=11, padCRC=0, rnti=0, iBIL=0, algo="SCL")


def lds_bytes(N, L, G):
    """DESIGN.md §4.13's LDS budget: LLR layers G+1..m, 66 candidates, L rows of packed bits, the ownership
    table, the small tables."""
    m = N.bit_length() - 1
    ew = sum(max((N >> lam) >> 5, 1) for lam in range(1, m + 1))
    W = 2 * ew + (N >> 5)
    return (8 * L * ((N >> G) - 1) + 8 * 66 + 4 * L * W + 32 * (m + 1) + 32 * 4 + 4 * 12 + 15) & ~15


def ws_layers(N, L):
    """G: how many of the largest LLR layers the launch puts into the global workspace."""
    G = 0
    while G < N.bit_length() - 2 and lds_bytes(N, L, G) > LDS_MAX:
        G += 1
    return G


def first_ws_L(N=1024):
    return min(L for L in range(1, 33) if ws_layers(N, L) > 0)


def test_switch_list_straddles_the_switch():
    Lw = first_ws_L()
    assert Lw - 1 in SWITCH_L and Lw in SWITCH_L and ws_layers(1024, Lw - 1) == 0 and ws_layers(1024, Lw) > 0
    assert all(ws_layers(N, 32) == 0 for N in NS[:-1])   # only N = 1024 ever uses the workspace


@functools.lru_cache(maxsize=None)
def big_rows():
    """Seven rate-recovered rows of the N = 1024 shape: below, at and above the waterfall, one rounded, one
    all-zero, one saturated."""
    rng = np.random.default_rng([R.LIVE_SEED, 1024])
    K, E = BIG["K"], BIG["E"]
    wf = R.waterfall_db(K, E)
    rows = []
    for off in (-1.0, 3.0, 0.5, -0.5, 2.0):
        blk = R.crc_attach(rng.integers(0, 2, K - 11), 11)
        rows.append(R.channel_llr(rng, R.rate_match(R.encode(blk, E, 10, 0), K, E, 0), wf + off))
    rows[4] = np.round(rows[4])
    rows += [np.zeros(E), 20.0 * np.where(rows[0] < 0, -1.0, 1.0)]
    return np.stack([R.rate_recover(x, K, 1024, 0) for x in rows])


@functools.lru_cache(maxsize=None)
def big_ref(L, rows=(0, 1, 2)):
    return ref_decode(dict(BIG, L=L), big_rows()[list(rows)])


@pytest.mark.parametrize("L", SWITCH_L)
def test_n1024_across_the_switch(torch, L):
    from python_5gtoolbox_amd import polar
    want = big_ref(L)
    assert sorted(set(want[1].tolist())) == [0, 1]   # B = 3 with mixed outcomes
    got = polar.decode(cu(torch, big_rows()[:3]), polar.plan(*R.plan_args(BIG)), "SCL", L)
    for g, w, name in zip(got, want, ("ck", "status", "pm")):
        same(g, w, (name, L))


# -------------------------------------------------------------------------------- workspace loop
@pytest.mark.parametrize("L,B", [(32, WS_SLOTS + 37), (first_ws_L(), 2 * WS_SLOTS + 5)])
def test_workspace_loop(torch, L, B):
    """More codewords than workspace slots: a workgroup decodes codeword w, then w + 1024 (then w + 2048) in the
    same slot.  Seven distinct rows tiled, so its codewords differ, in both orders of failing and succeeding."""
    from python_5gtoolbox_amd import polar
    assert ws_layers(1024, L) > 0 and B > WS_SLOTS and WS_SLOTS % 7 != 0
    ck, st, pm, info = big_ref(L, tuple(range(7)))
    assert st.sum() >= 2 and any(i["crc_fail"] for i in info) and any(i["early"] for i in info)
    idx = np.arange(B) % 7
    first, second = st[idx[:B - WS_SLOTS]], st[idx[WS_SLOTS:]]   # of the workgroups that loop
    assert np.any((first == 0) & (second == 1)) and np.any((first == 1) & (second == 0))
    got = polar.decode(cu(torch, big_rows()[idx]), polar.plan(*R.plan_args(BIG)), "SCL", L)
    same(got[0], ck[idx])
    same(got[1], st[idx])
    same(got[2], pm[idx])


# ------------------------------------------------------------------ leading dimensions, padding
PAD = 13
LD_SHAPES = [dict(K=28, E=32, nMax=9, iIL=1, CRCLEN=24, padCRC=0, rnti=0, iBIL=0),        # N = 32
             dict(K=45, E=101, nMax=10, iIL=0, CRCLEN=11, padCRC=0, rnti=5, iBIL=1),      # N = 128; K, E no multiples of 16
             dict(K=19, E=45, nMax=10, iIL=0, CRCLEN=6, padCRC=0, rnti=0, iBIL=1),        # K = 19, N = 64
             dict(K=1023, E=1031, nMax=10, iIL=0, CRCLEN=11, padCRC=0, rnti=0, iBIL=0)]   # K = 1023, N = 1024


def padded(torch, rows, width, dtype):
    """[rows, width + 13] filled with poison (0x55 / NaN) -> (buffer, its poison as numpy)."""
    if dtype == torch.float64:
        buf = torch.full((rows, width + PAD), float("nan"), dtype=dtype, device="cuda")
    else:
        buf = torch.full((rows, width + PAD), 0x55, dtype=dtype, device="cuda")
    return buf


def check_padded(buf, width, want, what):
    got = buf.cpu().numpy()
    same(np.ascontiguousarray(got[:, :width]), want, what)
    pad = got[:, width:]
    assert np.all(np.isnan(pad)) if pad.dtype == np.float64 else np.all(pad == 0x55), ("padding written", what)


def offset_view(torch, a):
    """a's rows as a view at offset 8 of a wider poisoned buffer -> (view, ld)."""
    a = cu(torch, a)
    wide = padded(torch, a.shape[0], a.shape[1] + 8, a.dtype)
    wide[:, 8:8 + a.shape[1]] = a
    return wide[:, 8:8 + a.shape[1]], wide.stride(0)


@pytest.mark.parametrize("i", range(len(LD_SHAPES)))
def test_leading_dimensions_and_padding(torch, i):
    """The four entry points through the C ABI with output ld = width + 13 and strided inputs: results equal
    polar_ref, the padding keeps its poison.  encode at B around its codewords per workgroup."""
    from python_5gtoolbox_amd import _lib, polar
    s = dict(LD_SHAPES[i], algo="SCL", L=4)
    K, E, nMax, iIL, crclen, pad, rnti, iBIL = (s[k] for k in R.SWEEP_FIELDS[:8])
    p = polar.plan(*R.plan_args(s))
    N = p.N
    lib, ptr, sp = _lib.lib(), _lib.ptr, _lib.stream_ptr
    pd = ptr(p.dev("cuda"))
    rng = np.random.default_rng([R.LIVE_SEED, 77, i])
    G = 256 // min(N // 2, 256)   # codewords per workgroup of the encoder
    Bmax = max(G + 1, 3)
    blk = np.stack([R.crc_attach(rng.integers(0, 2, K - crclen), crclen, rnti, pad) for _ in range(Bmax)])
    enc = np.stack([R.encode(b, E, nMax, iIL) for b in blk])
    rm = np.stack([R.rate_match(d, K, E, iBIL) for d in enc])
    for B in sorted({1, max(G - 1, 1), G, G + 1}):
        x, ld = offset_view(torch, blk[:B])
        out = padded(torch, B, N, torch.int8)
        _lib.check(lib.ldpc5g_polar_encode(pd, p.host, ptr(x), ld, ptr(out), N + PAD, B, sp()))
        check_padded(out, N, enc[:B], ("encode", s, B))
    B = 3
    x, ld = offset_view(torch, enc[:B])
    out = padded(torch, B, E, torch.int8)
    _lib.check(lib.ldpc5g_polar_rate_match(pd, p.host, ptr(x), ld, ptr(out), E + PAD, B, iBIL, sp()))
    check_padded(out, E, rm[:B], ("rate_match", s))
    llr = np.stack([R.channel_llr(rng, rm[j], R.waterfall_db(K, E) + (0.0, 3.0, 6.0)[j]) for j in range(B)])
    x, ld = offset_view(torch, llr)
    for quirk in (0, 1):
        out = padded(torch, B, N, torch.float64)
        _lib.check(lib.ldpc5g_polar_rate_recover(pd, p.host, ptr(x), ld, ptr(out), N + PAD, B, iBIL, 20.0, quirk, sp()))
        check_padded(out, N, np.stack([R.rate_recover(v, K, N, iBIL, 20.0, bool(quirk)) for v in llr]),
                     ("rate_recover", s, quirk))
    rr = np.stack([R.rate_recover(v, K, N, iBIL, 20.0) for v in llr])
    want = ref_decode(s, rr)
    assert want[1].any()
    x, ld = offset_view(torch, rr)
    ck = padded(torch, B, K, torch.int8)
    st = torch.full((B + PAD,), 0x55, dtype=torch.uint8, device="cuda")
    pm = torch.full((B + PAD,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.ldpc5g_polar_decode(pd, p.host, ptr(x), ld, ptr(ck), K + PAD, ptr(st), ptr(pm), B, polar.SCL, s["L"],
                                       sp()))
    check_padded(ck, K, want[0], ("decode ck", s))
    check_padded(st[None], B, want[1][None], ("decode status", s))
    check_padded(pm[None], B, want[2][None], ("decode pm", s))
