"""CPU tests of the maximum-likelihood detectors' host side and of their numpy restatement:
ldpc5g_ml_detect refuses every unsupported argument combination before any HIP call,
tests/ml_ref.py reproduces the reference's recorded outputs (tests/golden/ml_golden.npz) within
the bound |got - ref| <= 1e-10 * scale with every decision equal, and the library's pivot rule,
restated in numpy, takes the branch the reference's np.linalg.matrix_rank took (fired_cov).  No
kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import eq_ref
import ml_ref
from conftest import GOLD, ROOT
from python_5gtoolbox_amd import _lib

P = ctypes.c_void_p(4096)   # a non-null "buffer" (never dereferenced)


@pytest.fixture(scope="module")
def golden():
    return ml_ref.load_golden(os.path.join(GOLD, "ml_golden.npz"))


def _call(lib, y=P, ldy=None, h=P, ldh=None, cov=P, ldcov=None, dtype=_lib.F64, re_idx=None, R=72, nre=None,
          rpc=12, T=2, Nr=4, NL=2, mod=4, algo=0, irc=1, prbs=None, ldw=0, llr=P, llr_dtype=_lib.F64, ldllr=None,
          sym=None, ldsym=0, nv=None, ldnv=0, hb=None, ldhb=0):
    nre = R if nre is None else nre
    ncov = -(-R // rpc) if rpc > 0 else 1
    return lib.ldpc5g_ml_detect(
        y, R * Nr if ldy is None else ldy, h, R * Nr * NL if ldh is None else ldh, cov,
        ncov * Nr * Nr if ldcov is None else ldcov, dtype, re_idx, R, nre, rpc, T, Nr, NL, mod, algo, irc,
        prbs, ldw, llr, llr_dtype, nre * NL * abs(mod) if ldllr is None else ldllr, sym, ldsym, nv, ldnv, hb, ldhb,
        None)


def _bad(lib, rc):
    assert rc == _lib.ESIZE
    msg = lib.ldpc5g_last_error()
    assert msg, "an argument error must leave a message"
    return msg


def test_ml_detect_refuses_unsupported_arguments_before_touching_the_gpu():
    lib = _lib.lib()
    for Nr, NL in ((3, 1), (8, 2), (0, 0), (2, 3), (4, 5), (4, 0), (1, 2), (-1, 1)):
        assert b"Nr" in _bad(lib, _call(lib, Nr=Nr, NL=NL))
    for mod in (0, 3, 5, 12, -2):
        assert b"modulation" in _bad(lib, _call(lib, mod=mod))
    for algo in (-1, 5, 17):
        assert b"algo" in _bad(lib, _call(lib, algo=algo))
    for irc in (-1, 2):
        assert b"irc" in _bad(lib, _call(lib, irc=irc))
    for dt in (-1, 2, 7):
        assert b"dtype" in _bad(lib, _call(lib, dtype=dt))
        assert b"llr dtype" in _bad(lib, _call(lib, llr_dtype=dt))
    for rpc in (0, -12):
        assert b"re_per_cov" in _bad(lib, _call(lib, rpc=rpc))
    for kw in (dict(T=0), dict(T=-1), dict(R=0), dict(R=-5), dict(nre=0, re_idx=P), dict(nre=-1, re_idx=P),
               dict(nre=73, re_idx=P)):
        assert b"sizes" in _bad(lib, _call(lib, **kw))
    assert b"sizes" in _bad(lib, _call(lib, nre=54, re_idx=None))   # NULL re_idx means all R
    nb = 72 * 2 * 4
    for T in (1, 2):   # a row stride shorter than its row, T = 1 included
        assert b"stride" in _bad(lib, _call(lib, T=T, ldy=72 * 4 - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, ldh=72 * 8 - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, ldcov=6 * 16 - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, ldllr=nb - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, sym=P, ldsym=72 * 2 - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, nv=P, ldnv=72 * 2 - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, hb=P, ldhb=nb - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, prbs=P, ldw=nb // 32 - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, nre=54, re_idx=P, ldllr=54 * 8 - 1))
    assert b"stride" in _bad(lib, _call(lib, R=73, ldcov=6 * 16))    # 73 REs need a 7th covariance
    for null in ("y", "h", "cov", "llr"):
        assert b"null" in _bad(lib, _call(lib, **{null: None}))


OVER_CAP = [(2, 2, 10), (4, 3, 6), (4, 4, 6), (4, 3, 8), (4, 4, 8), (4, 3, 10), (4, 4, 10), (4, 2, 10)]
AT_CAP = [(1, 1, 10), (2, 2, 8), (4, 2, 8), (4, 4, 4), (4, 4, 2), (4, 4, 1), (4, 4, -1), (4, 2, 6), (4, 3, 4)]


@pytest.mark.parametrize("Nr,NL,mod", OVER_CAP)
def test_every_over_cap_combination_is_refused_and_names_the_way_out(Nr, NL, mod):
    lib = _lib.lib()
    for algo in (0, 1, 2) + ((4,) if NL != 2 else ()):   # opt-rank2-ML with NL != 2 is ML-soft
        for irc in (0, 1):
            msg = _bad(lib, _call(lib, Nr=Nr, NL=NL, mod=mod, algo=algo, irc=irc))
            assert b"65536" in msg and b"opt-rank2-ML" in msg
    # the subset search has no cap, nor has the rank-2 search on two layers
    assert b"null" in _bad(lib, _call(lib, Nr=Nr, NL=NL, mod=mod, algo=3, y=None))
    if NL == 2:
        assert b"null" in _bad(lib, _call(lib, Nr=Nr, NL=NL, mod=mod, algo=4, y=None))


@pytest.mark.parametrize("Nr,NL,mod", AT_CAP)
def test_every_supported_combination_passes_the_checks(Nr, NL, mod):
    """Each supported (shape, mod, algo, irc, dtypes) reaches the buffer check."""
    lib = _lib.lib()
    for algo in range(5):
        for irc in (0, 1):
            for dt in (_lib.F32, _lib.F64):
                assert b"null" in _bad(lib, _call(lib, Nr=Nr, NL=NL, mod=mod, algo=algo, irc=irc, dtype=dt,
                                                  llr_dtype=dt, y=None))


def test_binding_matches_header():
    src = open(os.path.join(ROOT, "include", "ldpc5g.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bldpc5g_ml_detect\s*\(([^)]*)\)", src)
    assert m
    assert len(m.group(1).split(",")) == 29 == len(_lib.SIGNATURES["ldpc5g_ml_detect"][1])
    assert hasattr(_lib.lib(), "ldpc5g_ml_detect")
    for name, val in (("ML_SOFT", 0), ("ML_HARD", 1), ("ML2_SOFT", 2), ("ML_MMSE", 3), ("ML_OPT_RANK2", 4)):
        assert re.search(r"#define\s+LDPC5G_%s\s+%d\b" % (name, val), src), name
    assert sorted(_lib.ML_ALGO) == sorted(ml_ref.ALGOS)
    assert sorted(set(_lib.ML_ALGO.values())) == [(a, i) for a in range(5) for i in (0, 1)]


def test_fixture_is_what_the_issue_describes(golden):
    assert list(golden) == list(ml_ref.SETS)
    for (Nr, NL, mod), c in golden.items():
        kind = c["kind"]
        Qm = ml_ref.QM[mod]
        big = NL * Qm >= 16
        want0 = 12 if NL * Qm > 16 else 4 if big else 24
        assert (kind == 0).sum() == want0
        assert (kind == 2).sum() == (12 if Nr >= 2 and not big else 0)
        assert (kind == 3).sum() == (12 if NL >= 2 and not big else 0)
        assert c["y"].shape == (kind.size, Nr) and c["h"].shape == (kind.size, Nr, NL)
        assert c["cov"].shape == (-(-kind.size // 12), Nr, Nr)
        assert np.array_equal(c["cov"], np.conj(c["cov"].transpose(0, 2, 1))), "cov exactly Hermitian"
        assert np.all(c["h"][kind == 3][:, :, NL - 1] == 0)
        if (kind == 2).any():
            assert np.all(np.linalg.matrix_rank(c["cov"][kind[::12] == 2]) == 1)
        algos = ml_ref.set_algos(Nr, NL, mod)
        assert len(algos) == (4 if NL * Qm > 16 else 10)
        for a in algos:
            search, irc = ml_ref.ALGOS[a]
            ok = (kind == 0) | ((kind == 2) & bool(irc)) | ((kind == 3) & (search in ml_ref.EXHAUSTIVE))
            assert np.array_equal(c[a]["ok"], ok), a
            assert np.array_equal(c[a]["fired_cov"], (kind == 2) & bool(irc)), a


def test_kind3_ties_go_to_the_first_point_and_give_zero_llrs(golden):
    """H[:, NL-1] = 0: the reference's strict `<` keeps mod_array[0] for that layer."""
    for (Nr, NL, mod), c in golden.items():
        k3 = c["kind"] == 3
        if not k3.any():
            continue
        Qm = ml_ref.QM[mod]
        p0 = ml_ref.constellation(mod)[0][0]
        for a in ml_ref.set_algos(Nr, NL, mod):
            search = ml_ref.ALGOS[a][0]
            if search not in ml_ref.EXHAUSTIVE:
                continue
            assert np.all(c[a]["s"][k3][:, NL - 1] == p0), a
            assert np.all(c[a]["hb"][k3][:, (NL - 1) * Qm:] == 0), a
            if search != "hard":
                assert np.all(c[a]["llr"][k3][:, (NL - 1) * Qm:] == 0), a


@pytest.mark.parametrize("algo", sorted(ml_ref.ALGOS))
def test_restatement_reproduces_the_reference_and_takes_its_branch(golden, algo):
    worst = 0.0
    for (Nr, NL, mod), c in golden.items():
        if algo not in ml_ref.set_algos(Nr, NL, mod):
            continue
        ref = c[algo]
        for r in np.nonzero(ref["ok"])[0]:
            o = ml_ref.detect_one(c["y"][r], c["h"][r], c["cov"][r // 12], mod, algo)
            where = (Nr, NL, mod, int(r))
            assert np.array_equal(o["sym"], ref["s"][r]) and np.array_equal(o["hardbits"], ref["hb"][r]), where
            err = max(np.abs(o["llr"] - ref["llr"][r]).max(), abs(o["nv"] - ref["nv"][r])) / ref["scale"][r]
            worst = max(worst, err)
            assert err <= ml_ref.TOL, where
            assert abs(o["scale"] - ref["scale"][r]) <= 1e-9 * ref["scale"][r], where
            # the LDL^H pivot rule against the reference's matrix_rank outcome
            assert o["fired_cov"] == ref["fired_cov"][r], where
            if ml_ref.ALGOS[algo][1]:
                assert bool(eq_ref.rule_fires(c["cov"][r // 12])[0]) == ref["fired_cov"][r], where
    print(f"{algo}: worst |got - ref| / scale = {worst:.2e}")


def test_constellation_and_opposite_rule():
    """Point m carries the binary digits of m; unit average energy; the opposite point differs in
    the asked bit and is the nearest such point on its axis."""
    for mod, Qm in ml_ref.QM.items():
        pts, bits = ml_ref.constellation(mod)
        assert pts.dtype == np.complex64 and pts.size == 1 << Qm
        assert abs((np.abs(pts.astype(np.complex128)) ** 2).mean() - 1) < 1e-6
        assert np.unique(pts).size == pts.size
        for m in range(0, pts.size, 7):
            for b in range(Qm):
                o = ml_ref.opposite_index(m, b, Qm)
                assert bits[o][b] != bits[m][b]
                other = np.nonzero(bits[:, b] != bits[m][b])[0]
                assert np.isclose(np.abs(pts[o] - pts[m]), np.abs(pts[other] - pts[m]).min())
