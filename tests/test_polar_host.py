"""CPU tests of the polar codec's host side: the two standard tables, tests/polar_ref.py against every
fixture the reference produced (tests/golden/polar_golden_*.npz), ldpc5g_polar_plan against the
construction fixtures and the restatement's layout, and every entry point refusing unsupported
arguments before any HIP call.  No kernel is launched here."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import polar_ref as R
from conftest import GOLD
from python_5gtoolbox_amd import _lib, polar

P = ctypes.c_void_p(4096)   # a non-null, aligned "buffer" (never dereferenced)


def load(name):
    return np.load(os.path.join(GOLD, f"polar_golden_{name}.npz"))


@pytest.fixture(scope="module")
def construct():
    return load("construct")


@pytest.fixture(scope="module")
def chain():
    return load("chain")


@pytest.fixture(scope="module")
def dec():
    d = load("decode")
    return d, json.loads(str(d["meta"]))


N_DECODE = len(json.loads(str(load("decode")["meta"])))
SWEEP = R.load_sweep(os.path.join(GOLD, "polar_golden_sweep.npz"))


def test_tables_are_permutations():
    Q, PI = R.tables()
    assert Q.shape == (1024,) and sorted(Q.tolist()) == list(range(1024))
    for n in range(5, 11):
        assert sorted(Q[Q < (1 << n)].tolist()) == list(range(1 << n))
    assert PI.shape == (164,) and sorted(PI.tolist()) == list(range(164))


def test_table_header_is_the_generated_one():
    import re
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "python_5gtoolbox_amd", "csrc", "ldpc5g_polar_tables.h")) as f:
        text = f.read()
    Q, PI = R.tables()
    for name, tab in (("kPolarQ", Q), ("kPolarPiIlMax", PI)):
        body = re.search(name + r"\[\d+\] = \{(.*?)\};", text, re.S).group(1)
        assert [int(v) for v in body.replace("\n", " ").split(",")] == tab.tolist()


def test_restatement_construction(construct):
    meta = construct["meta"]
    assert len(meta) >= 200
    for i, row in enumerate(meta.tolist()):
        K, E, nMax, N, nPC, nPCwm = row[:6]
        F, qPC, n2, p2, w2 = R.construct(K, E, nMax)
        assert (n2, p2, w2) == (N, nPC, nPCwm), row
        assert np.array_equal(F, construct[f"F{i}"]) and qPC.tolist() == row[6:6 + nPC], row


def test_plan_construction(construct):
    """F, qPC, N, nPC, nPCwm of the C plan equal the reference's on every triple, and the plan's maps
    equal the restatement's layout."""
    for i, row in enumerate(construct["meta"].tolist()):
        K, E, nMax, N, nPC, nPCwm = row[:6]
        iIL, crclen = (1, 24) if nMax == 9 else (0, 6 if K <= 25 else 11)
        p = polar.Plan(polar.plan_blob(K, E, nMax, iIL, crclen, 1 if iIL else 0, 0x4321 if iIL else 0))
        assert (p.N, p.nPC, p.nPCwm) == (N, nPC, nPCwm), row
        assert np.array_equal(p.F, construct[f"F{i}"]) and p.qPC.tolist() == row[6:6 + nPC], row
        assert p.magic == 0x504c5235 and p.bytes == p.blob.size
        if i % 8 == 0:
            lay = R.layout(K, E, nMax, iIL, crclen, 1 if iIL else 0, 0x4321 if iIL else 0)
            hdr = p.blob[:128].view(np.int32)
            cksrc = p.blob[hdr[21]:hdr[21] + 2 * K].view(np.int16)
            assert np.array_equal(cksrc, lay["ck_src"]) and p.mode_name[:3] == lay["mode"][:3]
            if iIL:
                assert [(int(hdr[18]) >> c) & 1 for c in range(24)] == lay["crc_mask"].tolist()
            il = p.blob[hdr[27]:hdr[27] + 2 * E].view(np.int16)
            assert np.array_equal(il, R.chan_il(E))


def test_restatement_chain(chain):
    for i, (K, E, nMax, iIL, iBIL, N, quirk) in enumerate(chain["meta"].tolist()):
        blk, enc, rm, llr, rr = (chain[f"{k}{i}"] for k in ("blk", "enc", "rm", "llr", "rr"))
        assert np.array_equal(R.encode(blk, E, nMax, iIL), enc)
        assert np.array_equal(R.rate_match(enc, K, E, iBIL), rm)
        assert np.array_equal(R.rate_recover(llr, K, N, iBIL, 20.0, reference_repetition=True), rr)
        assert (not np.array_equal(R.rate_recover(llr, K, N, iBIL, 20.0), rr)) == bool(quirk)
    assert any(q for *_, q in chain["meta"].tolist())
    for j, (A, Euci, C, Er) in enumerate(chain["seg_meta"].tolist()):
        blks, c2, e2 = R.cbsegment(chain[f"seg_in{j}"], Euci)
        assert (c2, e2) == (C, Er) and np.array_equal(blks, chain[f"seg_out{j}"])


def test_decode_fixtures_hold_every_class(dec):
    _, meta = dec
    for k in ("early", "crc_fail", "not_best", "pc_kills", "median_ties"):
        assert sum(1 for c in meta if c["info"][k]) >= 3, k
    have = {(c["algo"], c["L"]) for c in meta}
    assert {("SC", 1)} | {("SCL", L) for L in (1, 2, 3, 8, 16, 32)} <= have
    assert {1 << R.n_value(c["K"], c["E"], c["nMax"]) for c in meta} >= {32, 64, 256, 512, 1024}
    assert any(c["L"] == 32 and R.n_value(c["K"], c["E"], c["nMax"]) == 10 for c in meta)


@pytest.mark.parametrize("i", range(N_DECODE))
def test_restatement_decode(dec, i):
    d, meta = dec
    c = meta[i]
    ck, st, pm, info = R.decode(c["algo"], d[f"llr{i}"], c["E"], c["K"], c["L"], c["nMax"], c["iIL"], c["CRCLEN"],
                                c["padCRC"], c["rnti"])
    assert int(st) == c["status"] and np.array_equal(ck, d[f"ck{i}"])
    assert pm == float.fromhex(c["pm"]) and {k: int(v) for k, v in info.items()} == c["info"]
    assert st or (np.all(ck == -1) and math.isinf(pm))


@pytest.mark.parametrize("i", range(len(SWEEP)))
def test_restatement_sweep(i):
    """polar_ref reproduces the reference's (ck, status) of every recorded sweep case, and its own pm and classes."""
    c, llr, want = SWEEP[i]
    rr = R.rate_recover(llr, c["K"], c["N"], c["iBIL"], 20.0, reference_repetition=True)
    ck, st, pm, info = R.decode(c["algo"], rr, c["E"], c["K"], c["L"], c["nMax"], c["iIL"], c["CRCLEN"], c["padCRC"],
                                c["rnti"])
    assert int(st) == c["status"] and ck.dtype == want.dtype and np.array_equal(ck, want)
    assert pm == float.fromhex(c["pm"]) and {k: int(v) for k, v in info.items()} == c["info"]
    assert st or (np.all(ck == -1) and math.isinf(pm))


def test_sweep_fixture_is_the_committed_shape_list():
    meta = [c for c, _, _ in SWEEP]
    assert len(meta) == 960 and all(len(llr) == c["E"] <= 2048 for c, llr, _ in SWEEP)
    shapes = R.fixture_shapes(160)   # recorded round robin over the six N
    assert [{k: c[k] for k in R.SWEEP_FIELDS} for c in meta] == [shapes[n * 160 + r] for r in range(160) for n in range(6)]
    byN = R.sweep_coverage(meta)
    for N, lst in byN.items():
        st = [c["status"] for c in lst]
        assert len(st) == 160 and sum(st) >= 3 and len(st) - sum(st) >= 3, N
    for k in ("early", "crc_fail", "not_best", "pc_kills", "median_ties", "crc_kills"):
        assert sum(1 for c in meta if c["info"][k]) >= 3, k
    assert {(c["nMax"], c["iBIL"]) for c in meta} == {(9, 0), (9, 1), (10, 0), (10, 1)}


PLAN_LISTS = {"fixture": [c for c, _, _ in SWEEP], "live": R.live_shapes()}


@pytest.mark.parametrize("which,N", [(w, N) for w in PLAN_LISTS for N in (32, 64, 128, 256, 512, 1024)])
def test_plan_maps_of_every_sweep_shape(which, N):
    """F, qPC, cksrc, crc_mask, il, mode and N of the C plan equal the restatement's, for every shape the GPU
    sweeps use (the live list holds the triangular E = 2080 and 8128, and E = 8192)."""
    shapes = [s for s in PLAN_LISTS[which] if 1 << R.n_value(s["K"], s["E"], s["nMax"]) == N]
    assert len(shapes) >= 8
    if which == "live":
        assert {s["E"] for s in PLAN_LISTS[which]} >= {2080, 8128, 8192}
    for s in shapes:
        K, E = s["K"], s["E"]
        p = polar.Plan(polar.plan_blob(*R.plan_args(s)))
        lay = R.layout(*R.plan_args(s))
        assert (p.N, p.nPC, p.nPCwm) == (N, lay["nPC"], lay["nPCwm"]) == (lay["N"], p.nPC, p.nPCwm), s
        assert np.array_equal(p.F, lay["F"]) and p.qPC.tolist() == lay["qPC"].tolist(), s
        hdr = p.blob[:128].view(np.int32)
        assert np.array_equal(p.blob[hdr[21]:hdr[21] + 2 * K].view(np.int16), lay["ck_src"]), s
        assert p.mode_name[:3] == lay["mode"][:3], s
        want = lay["crc_mask"].tolist() if s["iIL"] else [0] * 24
        assert [(int(hdr[18]) >> c) & 1 for c in range(24)] == want, s
        il = R.chan_il(E)
        assert np.array_equal(p.blob[hdr[27]:hdr[27] + 2 * E].view(np.int16), il), s
        assert np.array_equal(p.blob[hdr[28]:hdr[28] + 2 * E].view(np.int16), np.argsort(il)), s


# ------------------------------------------------------------------------------------- refusals
PLAN_BAD = [
    (dict(nMax=8), b"nMax"), (dict(nMax=11), b"nMax"), (dict(iIL=0), b"nMax"), (dict(crclen=11), b"nMax"),
    (dict(nMax=10, iIL=0, crclen=24), b"nMax"), (dict(nMax=10, iIL=1, crclen=11), b"nMax"),
    (dict(E=0), b"E="), (dict(E=8193), b"E="), (dict(E=-5), b"E="),
    (dict(padCRC=2), b"padCRC"), (dict(rnti=-1), b"rnti"), (dict(rnti=1 << 24), b"rnti"),
    (dict(K=24), b"CRC"), (dict(K=165, E=400), b"interleaver"),
    (dict(K=64, E=60), b"exceeds E"),
    (dict(nMax=10, iIL=0, crclen=11, K=17, E=100), b"UL ranges"),
    (dict(nMax=10, iIL=0, crclen=11, K=28, E=100), b"UL ranges"),
    (dict(nMax=10, iIL=0, crclen=6, K=20, E=22), b"exceeds E"),
    (dict(nMax=10, iIL=0, crclen=11, K=1024, E=2000), b"N=1024"),
]


def _plan(lib, K=64, E=216, nMax=9, iIL=1, crclen=24, padCRC=0, rnti=0, buf=None, cap=0):
    return lib.ldpc5g_polar_plan(K, E, nMax, iIL, crclen, padCRC, rnti, buf, cap)


@pytest.mark.parametrize("i", range(len(PLAN_BAD)))
def test_plan_refuses(i):
    kw, word = PLAN_BAD[i]
    lib = _lib.lib()
    assert _plan(lib, **kw) == _lib.ESIZE
    assert word in lib.ldpc5g_last_error(), (word, lib.ldpc5g_last_error())


def test_plan_refuses_a_short_buffer():
    lib = _lib.lib()
    n = _plan(lib)
    assert n > 0
    buf = np.zeros(n, np.uint8)
    assert _plan(lib, buf=ctypes.c_void_p(buf.ctypes.data), cap=n - 1) == _lib.ESIZE
    assert b"plan_bytes" in lib.ldpc5g_last_error()


def _calls(lib, blob, **kw):
    """The four entry points with valid arguments by default (DCI shape: K 64, E 216, N 256)."""
    a = dict(pd=P, ph=ctypes.c_void_p(blob.ctypes.data), x=P, y=P, st=P, pm=P, ldK=64, ldN=256, ldE=216, B=3, iBIL=0,
             algo=polar.SCL, L=8, quirk=0, keep=blob)   # keep: the host plan outlives the call
    a.update(kw)
    return {
        "encode": lambda: lib.ldpc5g_polar_encode(a["pd"], a["ph"], a["x"], a["ldK"], a["y"], a["ldN"], a["B"], None),
        "rate_match": lambda: lib.ldpc5g_polar_rate_match(a["pd"], a["ph"], a["x"], a["ldN"], a["y"], a["ldE"], a["B"],
                                                          a["iBIL"], None),
        "rate_recover": lambda: lib.ldpc5g_polar_rate_recover(a["pd"], a["ph"], a["x"], a["ldE"], a["y"], a["ldN"],
                                                              a["B"], a["iBIL"], 20.0, a["quirk"], None),
        "decode": lambda: lib.ldpc5g_polar_decode(a["pd"], a["ph"], a["x"], a["ldN"], a["y"], a["ldK"], a["st"], a["pm"],
                                                  a["B"], a["algo"], a["L"], None),
    }


ALL = ("encode", "rate_match", "rate_recover", "decode")
CALL_BAD = [(f, kw, w) for f in ALL for kw, w in (
    (dict(pd=None), b"plan_dev"), (dict(ph=None), b"plan_host"), (dict(x=None), b"null"), (dict(y=None), b"null"),
    (dict(B=0), b"B="), (dict(B=-1), b"B="), (dict(B=(1 << 22) + 1), b"B="))]
CALL_BAD += [("encode", dict(ldK=63), b"ldb"), ("encode", dict(ldN=255), b"ldo"),
             ("rate_match", dict(ldN=255), b"ldi"), ("rate_match", dict(ldE=215), b"ldo"),
             ("rate_match", dict(iBIL=2), b"iBIL"), ("rate_recover", dict(ldE=215), b"ldi"),
             ("rate_recover", dict(ldN=0), b"ldo"), ("rate_recover", dict(iBIL=-1), b"iBIL"),
             ("rate_recover", dict(quirk=2), b"reference_repetition"),
             ("decode", dict(ldN=255), b"ldl"), ("decode", dict(ldK=-64), b"ldc"), ("decode", dict(L=0), b"L="),
             ("decode", dict(L=33), b"L="), ("decode", dict(L=-8), b"L="), ("decode", dict(algo=2), b"algo"),
             ("decode", dict(algo=-1), b"algo"), ("decode", dict(st=None), b"status"), ("decode", dict(pm=None), b"pm"),
             ("decode", dict(x=ctypes.c_void_p(4100)), b"aligned")]


@pytest.mark.parametrize("i", range(len(CALL_BAD)), ids=lambda i: f"{CALL_BAD[i][0]}-{i}")
def test_entry_points_refuse_before_touching_the_gpu(i):
    f, kw, word = CALL_BAD[i]
    lib = _lib.lib()
    rc = _calls(lib, polar.plan_blob(64, 216, 9, 1, 24), **kw)[f]()
    assert rc == _lib.ESIZE
    assert word in lib.ldpc5g_last_error(), (word, lib.ldpc5g_last_error())


@pytest.mark.parametrize("f", ALL)
@pytest.mark.parametrize("what", ["magic", "version", "N"])
def test_a_damaged_plan_is_refused(f, what):
    lib = _lib.lib()
    blob = polar.plan_blob(64, 216, 9, 1, 24).copy()
    hdr = blob[:80].view(np.int32)
    if what == "magic":
        hdr[0] ^= 1
    elif what == "version":
        hdr[1] += 1
    else:
        hdr[10] = 2048   # N beyond what the kernels index
    assert _calls(lib, blob)[f]() == _lib.ESIZE
    assert {"magic": b"magic", "version": b"version", "N": b"range"}[what] in lib.ldpc5g_last_error()


def test_python_surface_raises_the_librarys_message():
    with pytest.raises(AssertionError, match="UL ranges"):
        polar.plan_blob(28, 100, 10, 0, 11)
    with pytest.raises(AssertionError, match="exceeds E"):
        polar.plan_blob(64, 60, 9, 1, 24)
