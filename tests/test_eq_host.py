"""CPU tests of the batched equaliser's host side and of its numpy restatement: ldpc5g_equalize
refuses every unsupported argument combination before any HIP call, tests/eq_ref.py reproduces the
reference's recorded outputs (tests/golden/eq_golden.npz), and the library's regularisation rule
(unpivoted LDL^H pivots against 2^-40 max|A|), restated in numpy, takes the branch the reference's
np.linalg.matrix_rank took on every fixture case.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import eq_ref
from conftest import GOLD, ROOT
from python_5gtoolbox_amd import _lib

P = ctypes.c_void_p(4096)   # a non-null "buffer" (never dereferenced)
TOL = 1e-9


@pytest.fixture(scope="module")
def golden():
    return eq_ref.load_golden(os.path.join(GOLD, "eq_golden.npz"))


def _call(lib, y=P, ldy=None, h=P, ldh=None, cov=P, ldcov=None, dtype=_lib.F64, re_idx=None, R=72, nre=None,
          rpc=12, T=2, Nr=4, NL=2, algo=3, sym=P, ldsym=None, nv=P, ldnv=None):
    nre = R if nre is None else nre
    ncov = -(-R // rpc) if rpc > 0 else 1
    return _lib.invoke(
        "ldpc5g_equalize", y=y, ldy=R * Nr if ldy is None else ldy, h=h, ldh=R * Nr * NL if ldh is None else ldh,
        cov=cov, ldcov=ncov * Nr * Nr if ldcov is None else ldcov, in_dtype=dtype, re_idx=re_idx, R=R, nre=nre,
        re_per_cov=rpc, T=T, Nr=Nr, NL=NL, algo=algo, sym=sym, ldsym=nre * NL if ldsym is None else ldsym,
        noise_var=nv, ldnv=nre * NL if ldnv is None else ldnv, stream=None)


def _bad(lib, rc):
    assert rc == _lib.ESIZE
    msg = lib.ldpc5g_last_error()
    assert msg, "an argument error must leave a message"
    return msg


def test_equalize_refuses_unsupported_arguments_before_touching_the_gpu():
    lib = _lib.lib()
    for Nr, NL in ((3, 1), (8, 2), (0, 0), (2, 3), (4, 5), (4, 0), (1, 2), (-1, 1)):
        assert b"Nr" in _bad(lib, _call(lib, Nr=Nr, NL=NL))
    for algo in (-1, 4, 17):
        assert b"algo" in _bad(lib, _call(lib, algo=algo))
    for dt in (-1, 2, 7):
        assert b"dtype" in _bad(lib, _call(lib, dtype=dt))
    for rpc in (0, -12):
        assert b"re_per_cov" in _bad(lib, _call(lib, rpc=rpc))
    for kw in (dict(T=0), dict(T=-1), dict(R=0), dict(R=-5), dict(nre=0, re_idx=P), dict(nre=-1, re_idx=P),
               dict(nre=73, re_idx=P)):
        assert b"sizes" in _bad(lib, _call(lib, **kw))
    assert b"sizes" in _bad(lib, _call(lib, nre=54, re_idx=None))   # NULL re_idx means all R
    # a row stride shorter than its row, T = 1 included
    for T in (1, 2):
        assert b"stride" in _bad(lib, _call(lib, T=T, ldy=72 * 4 - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, ldh=72 * 8 - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, ldcov=6 * 16 - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, ldsym=72 * 2 - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, ldnv=72 * 2 - 1))
        assert b"stride" in _bad(lib, _call(lib, T=T, nre=54, re_idx=P, ldsym=54 * 2 - 1))
    assert b"stride" in _bad(lib, _call(lib, R=73, ldcov=6 * 16))    # 73 REs need a 7th covariance
    for null in ("y", "h", "cov", "sym", "nv"):
        assert b"null" in _bad(lib, _call(lib, **{null: None}))


@pytest.mark.parametrize("Nr,NL", eq_ref.SHAPES)
def test_every_supported_shape_passes_the_shape_check(Nr, NL):
    """Each supported (Nr, NL, algo, dtype) reaches the buffer check: the error is the null buffer."""
    lib = _lib.lib()
    for algo in range(4):
        for dt in (_lib.F32, _lib.F64):
            assert b"null" in _bad(lib, _call(lib, Nr=Nr, NL=NL, algo=algo, dtype=dt, y=None))


def test_binding_matches_header():
    src = open(os.path.join(ROOT, "include", "ldpc5g.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bldpc5g_equalize\s*\(([^)]*)\)", src)
    assert m
    assert len(m.group(1).split(",")) == 20 == len(_lib.SIGNATURES["ldpc5g_equalize"][1])
    assert hasattr(_lib.lib(), "ldpc5g_equalize")
    for name, val in (("ZF", 0), ("ZF_IRC", 1), ("MMSE", 2), ("MMSE_IRC", 3)):
        assert re.search(r"#define\s+LDPC5G_EQ_%s\s+%d\b" % (name, val), src), name
        assert _lib.EQ_ALGO[name.replace("_", "-")] == val


def test_fixture_meets_the_bounds_the_tolerance_is_derived_from(golden):
    """sigma_min/sigma_max(H^H H) >= 1e-4 and kappa(cov) <= 1e2 on the regular cases; the singular
    constructions are what they claim; every shape has its cases."""
    assert sorted(golden) == sorted(eq_ref.SHAPES)
    for (Nr, NL), c in golden.items():
        kind = c["kind"]
        assert c["y"].shape == (kind.size, Nr) and c["h"].shape == (kind.size, Nr, NL)
        assert c["cov"].shape == (kind.size // 12, Nr, Nr) and kind.size % 12 == 0
        assert (kind == 0).sum() == 96 and (kind == 1).sum() == (12 if NL >= 2 else 0)
        assert (kind == 2).sum() == (12 if Nr >= 2 else 0)
        assert np.array_equal(c["cov"], np.conj(c["cov"].transpose(0, 2, 1))), "cov exactly Hermitian"
        h = c["h"]
        sv = np.linalg.svd(np.conj(h.transpose(0, 2, 1)) @ h, compute_uv=False)
        assert (sv[kind != 1, -1] / sv[kind != 1, 0]).min() >= 1e-4
        assert np.array_equal(h[kind == 1][:, :, NL - 1], h[kind == 1][:, :, 0])
        cov_kind = kind[::12]
        assert np.linalg.cond(c["cov"][cov_kind != 2]).max(initial=1.0) <= 1e2
        if Nr >= 2:
            assert np.all(np.linalg.matrix_rank(c["cov"][cov_kind == 2]) == 1)


@pytest.mark.parametrize("algo", eq_ref.ALGOS)
def test_restatement_reproduces_the_reference_and_takes_its_branch(golden, algo):
    for (Nr, NL), c in golden.items():
        s, nv, fired = eq_ref.equalize(c["y"], c["h"], c["cov"], algo)
        ref = c[algo]
        s, nv = s.reshape(-1, NL), nv.reshape(-1, NL)
        assert np.all(np.abs(s - ref["s"]).max(1) <= TOL * np.abs(ref["s"]).max(1)), (Nr, NL)
        assert np.all(np.abs(nv - ref["nv"]).max(1) <= TOL * np.abs(ref["nv"]).max(1)), (Nr, NL)
        # the LDL^H rule against the reference's matrix_rank outcome, every RE
        assert np.array_equal(fired["w1"], ref["fired_w1"]), (Nr, NL)
        assert np.array_equal(fired["cov"], ref["fired_cov"]), (Nr, NL)
        # and the singular cases are really exercised where they should be
        kind = c["kind"]
        if Nr >= 2:
            assert np.array_equal(ref["fired_w1"], (kind == 1) & (algo in ("ZF", "ZF-IRC")))
            assert np.array_equal(ref["fired_cov"], (kind == 2) & (algo == "MMSE-IRC"))


def test_rule_margins():
    """The rule is silent at sigma_min/sigma_max = 1e-8 and fires on exactly singular matrices,
    NaN and indefinite input (the negated comparison)."""
    rng = np.random.default_rng(7)
    for n in (2, 3, 4):
        q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        lam = np.ones(n)
        lam[-1] = 1e-8
        A = (q * lam) @ np.conj(q.T)
        A = (A + np.conj(A.T)) / 2
        assert not eq_ref.rule_fires(A)[0]
        g = rng.standard_normal((n, 1)) + 1j * rng.standard_normal((n, 1))
        assert eq_ref.rule_fires(g @ np.conj(g.T))[0]
        assert eq_ref.rule_fires(-np.identity(n, dtype=complex))[0]
        B = np.identity(n, dtype=complex)
        B[n - 1, n - 1] = np.nan
        assert eq_ref.rule_fires(B)[0]
