"""numpy restatement of the batched equaliser (ldpc5g_equalize, include/ldpc5g.h): the four
linear algorithms of py5gphy's ZF.py / MMSE.py vectorised over resource elements, with the
library's regularisation rule (unpivoted LDL^H pivots against 2^-40 max|A|) in place of the
reference's np.linalg.matrix_rank.  It is this project's own code; tests/test_eq_host.py pins it
to the reference's recorded outputs (tests/golden/eq_golden.npz), and the GPU tests use it where
the fixture has no case (strides, gaps, several transport blocks).
"""
import numpy as np

ALGOS = ("ZF", "ZF-IRC", "MMSE", "MMSE-IRC")
SHAPES = ((1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 3), (4, 4))
REG = 0.0012            # ZF.py:35, MMSE.py:34,43,90
PIVOT_RATIO = 2.0 ** -40


def ldl_pivots(A):
    """Pivots d (..., n) of the unpivoted factorisation A = L D L^H of Hermitian A (..., n, n)."""
    n = A.shape[-1]
    L = np.zeros(A.shape, np.complex128)
    d = np.zeros(A.shape[:-1], np.float64)
    with np.errstate(all="ignore"):
        for j in range(n):
            dj = A[..., j, j].real.copy()
            for k in range(j):
                dj -= (L[..., j, k].real ** 2 + L[..., j, k].imag ** 2) * d[..., k]
            d[..., j] = dj
            for i in range(j + 1, n):
                s = A[..., i, j].copy()
                for k in range(j):
                    s -= L[..., i, k] * np.conj(L[..., j, k]) * d[..., k]
                L[..., i, j] = s / dj
    return d


def rule_fires(A):
    """The library's rule: regularise iff NOT(min_k d_k > 2^-40 max_ij |A_ij|)."""
    mx = np.abs(A).max(axis=(-1, -2))
    return ~(ldl_pivots(A).min(axis=-1) > PIVOT_RATIO * mx), mx


def reg_inv(A):
    """(inverse of A, regularised where the rule fires; fired (...,) bool)"""
    fired, mx = rule_fires(A)
    A = A + (fired * mx * REG)[..., None, None] * np.identity(A.shape[-1])
    return np.linalg.inv(A), fired


def equalize(y, h, cov, algo, re_idx=None, re_per_cov=12):
    """y (R, Nr), h (R, Nr, NL), cov (ceil(R/re_per_cov), Nr, Nr) complex128 of one transport
    block -> (sym (nre*NL,) complex128, noise_var (nre*NL,) float64, {"w1": fired, "cov": fired})."""
    assert algo in ALGOS
    y, h, cov = (np.asarray(a, np.complex128) for a in (y, h, cov))
    R, Nr = y.shape
    NL = h.shape[2]
    idx = np.arange(R) if re_idx is None else np.asarray(re_idx, np.int64)
    Y, H, C = y[idx], h[idx], cov[idx // re_per_cov]
    none = np.zeros(idx.size, bool)
    if Nr == 1:
        hh = (np.conj(H[:, 0, 0]) * H[:, 0, 0]).real
        return (Y[:, 0] / H[:, 0, 0]), C[:, 0, 0].real / hh, {"w1": none, "cov": none}
    Hh = np.conj(H).transpose(0, 2, 1)
    eye = np.identity(NL)
    sigma = np.diagonal(C, axis1=1, axis2=2).real.mean(axis=1)[:, None, None]
    fired_cov = none
    if algo in ("ZF", "ZF-IRC"):
        V, fired = reg_inv(Hh @ H)
        W = V @ Hh
        s = (W @ Y[..., None])[..., 0]
        if algo == "ZF":
            nv = sigma[:, 0] * np.diagonal(V, axis1=1, axis2=2).real
        else:
            nv = np.einsum("nli,nij,nlj->nl", W, C, np.conj(W)).real
    else:
        if algo == "MMSE":
            V, fired = reg_inv(Hh @ H / sigma + eye)
            W = V @ Hh / sigma
        else:
            Ci, fired_cov = reg_inv(C)
            V, fired = reg_inv(Hh @ Ci @ H + eye)
            W = V @ Hh @ Ci
        s_hat = (W @ Y[..., None])[..., 0]
        comp = 1 - np.diagonal(V, axis1=1, axis2=2).real
        s = s_hat / comp
        nv = 1 / comp - 1
    return s.reshape(-1), nv.reshape(-1), {"w1": fired, "cov": fired_cov}


def load_golden(path):
    """{(Nr, NL): dict(y, h, cov, kind, and per algorithm s / nv / fired_w1 / fired_cov)} from
    eq_golden.npz (tests/golden/gen_eq_golden.py)."""
    d = np.load(path)
    out = {}
    for Nr, NL in SHAPES:
        p = f"s{Nr}{NL}_"
        c = {k: d[p + k] for k in ("y", "h", "cov", "kind")}
        for a in ALGOS:
            c[a] = {k: d[p + a + "_" + k] for k in ("s", "nv", "fired_w1", "fired_cov")}
        out[(Nr, NL)] = c
    return out
