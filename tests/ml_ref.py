"""numpy restatement of the batched maximum-likelihood detectors (ldpc5g_ml_detect,
include/ldpc5g.h): py5gphy's ML.py / ML2.py / MMSE_ML.py / opt_rank2_ML.py, vectorised over the
candidates of one resource element.  It is this project's own code and deliberately differs from
both the reference and the kernel in how it gets there: IRC whitening is by a Cholesky factor of
the (regularised) covariance, where the reference uses eigh of its inverse and the kernel LDL^H.
tests/test_ml_host.py pins it to the reference's recorded outputs (tests/golden/ml_golden.npz),
and the GPU tests use it where the fixture has no case (strides, gaps, several transport blocks).
"""
import itertools
import math

import numpy as np

import eq_ref

QM = {"pi/2-bpsk": 1, "bpsk": 1, "qpsk": 2, "16qam": 4, "64qam": 6, "256qam": 8, "1024qam": 10}
SCALE = {1: 2, 2: 2, 4: 10, 6: 42, 8: 170, 10: 682}
# name -> (search, irc); the ten ML names of channel_equ_and_demod (nr_channel_eq.py:27-46)
ALGOS = {"ML-soft": ("soft", 0), "ML-IRC-soft": ("soft", 1), "ML-hard": ("hard", 0), "ML-IRC-hard": ("hard", 1),
         "ML2-soft": ("ml2", 0), "ML2-IRC-soft": ("ml2", 1), "MMSE-ML": ("subset", 0),
         "MMSE-ML-IRC": ("subset", 1), "opt-rank2-ML": ("rank2", 0), "opt-rank2-ML-IRC": ("rank2", 1)}
EXHAUSTIVE = ("soft", "hard", "ml2")
MAX_BITS = 16   # exhaustive search cap: M^NL <= 65536
# (Nr, NL, mod) sets of the fixture, in its order
SETS = ((1, 1, "1024qam"), (2, 1, "256qam"), (2, 2, "bpsk"), (2, 2, "qpsk"), (2, 2, "16qam"), (2, 2, "64qam"),
        (4, 2, "16qam"), (4, 3, "16qam"), (4, 4, "qpsk"), (2, 2, "256qam"), (4, 4, "16qam"), (2, 2, "1024qam"))
TOL = 1e-10   # |got - ref| <= TOL * scale, every LLR and noise variance


def set_algos(Nr, NL, mod):
    """The algorithms the fixture holds for a set."""
    if NL * QM[mod] > MAX_BITS:
        return tuple(a for a, (s, _) in ALGOS.items() if s in ("subset", "rank2"))
    return tuple(ALGOS)


def axis_levels(Qm):
    """float32 PAM level per axis-bit pattern k (bits MSB first), before scaling: 38.211 5.1."""
    HQ = max(Qm // 2, 1)
    k = np.arange(1 << HQ)
    u = [(1 - 2 * ((k >> (HQ - 1 - j)) & 1)).astype(np.float32) for j in range(HQ)]
    t = u[HQ - 1]
    for j in range(HQ - 2, -1, -1):
        t = u[j] * (np.float32(1 << (HQ - 1 - j)) - t)
    return t


def constellation(mod):
    """(points complex64 (M,), bits int8 (M, Qm)): point m has the binary digits of m, MSB first."""
    Qm = QM[mod]
    M = 1 << Qm
    m = np.arange(M)
    bits = ((m[:, None] >> (Qm - 1 - np.arange(Qm))) & 1).astype(np.int8)
    lev = axis_levels(Qm)
    if Qm == 1:
        re = im = lev[m]
    else:
        HQ = Qm // 2
        kx = np.zeros(M, int)
        ky = np.zeros(M, int)
        for j in range(HQ):
            kx = (kx << 1) | bits[:, 2 * j]
            ky = (ky << 1) | bits[:, 2 * j + 1]
        re, im = lev[kx], lev[ky]
    pts = (re + 1j * im) / math.sqrt(SCALE[Qm])   # complex64 / python float, as nrModulate
    assert pts.dtype == np.complex64
    return pts, bits


def opposite_index(m, b, Qm):
    """Index of the point get_oppisite_syms gives for bit b of point m: bit b flipped, the next
    bit on the same axis 0 and the later ones 1."""
    r = m ^ (1 << (Qm - 1 - b))
    for j in range(b + 2, Qm, 2):
        bit = 1 << (Qm - 1 - j)
        r = (r & ~bit) if j == b + 2 else (r | bit)
    return r


def whiten(Y, H, C):
    """(Y', H', fired): U Y, U H with U^H U = inv(C regularised by the library's pivot rule)."""
    fired, mx = eq_ref.rule_fires(C)
    C = C + (fired * mx * eq_ref.REG) * np.identity(C.shape[0])
    L = np.linalg.cholesky(C)
    return np.linalg.solve(L, Y), np.linalg.solve(L, H), bool(fired)


def metrics(Y, H, S, sigma2):
    """v(S) for S (n, NL)"""
    d = Y[None, :] - S @ H.T
    return (d.real ** 2 + d.imag ** 2).sum(axis=1) / sigma2


def candidates(NL, Qm):
    """(ncand, NL) point indices in itertools.product order, layer 0 slowest."""
    c = np.arange(1 << (NL * Qm))
    return (c[:, None] >> (Qm * (NL - 1 - np.arange(NL)))) & ((1 << Qm) - 1)


def _rank2(Y, H, pts, sigma2):
    """opt_rank2_ML.py:62-109, the loop over s0 (vectorised), including its float32 |s0|^2."""
    lev = np.unique(pts.real)   # float32 levels
    YH = np.conj(Y) @ H
    HH = np.conj(H.T) @ H
    a0i, a0q, a1i, a1q = YH[0].real, YH[0].imag, YH[1].real, YH[1].imag
    a2, a3, a4i, a4q = HH[0, 0].real, HH[1, 1].real, HH[0, 1].real, HH[0, 1].imag
    x0, y0 = pts.real, pts.imag   # float32
    L21 = a2 * (x0 ** 2 + y0 ** 2).astype(np.float64) - 2 * a0i * x0 + 2 * a0q * y0
    gx = -a1i + a4i * x0 + a4q * y0
    gy = a1q + a4i * y0 - a4q * x0
    pick = np.argmin if a3 > 0 else np.argmax
    with np.errstate(all="ignore"):
        cx1 = lev[pick(np.abs(lev[None, :] - (-gx / a3)[:, None]), axis=1)].astype(np.float64)
        cy1 = lev[pick(np.abs(lev[None, :] - (-gy / a3)[:, None]), axis=1)].astype(np.float64)
    L2 = L21 + (a3 * cx1 * cx1 + 2 * gx * cx1) + (a3 * cy1 * cy1 + 2 * gy * cy1)
    k = int(np.argmin(L2))
    s1 = np.complex64(cx1[k] + 1j * cy1[k])
    yy = (np.conj(Y) @ Y).real
    return k, s1, (yy + L2[k]) / sigma2


def detect_one(Y, H, C, mod, algo):
    """One resource element -> dict(sym (NL,) complex64, nv float, hardbits (NL*Qm,) int8,
    llr (NL*Qm,) float64, fired_cov bool, gap: second-smallest minus smallest metric of the
    search (None for rank2), scale)."""
    search, irc = ALGOS[algo]
    Nr, NL = H.shape
    Qm = QM[mod]
    if search == "rank2" and NL != 2:
        search = "soft"
    pts, bits = constellation(mod)
    p64 = pts.astype(np.complex128)
    M = pts.size
    est = None
    if search == "subset":
        est = eq_ref.equalize(Y[None], H[None], C[None], "MMSE-IRC" if irc else "MMSE", re_per_cov=1)[0]
    fired = False
    if irc:
        Y, H, fired = whiten(Y, H, C)
        sigma2 = 1.0
    else:
        sigma2 = np.diagonal(C).real.sum() / Nr
    scale = (np.linalg.norm(Y) + np.linalg.norm(H) * math.sqrt(NL) * np.abs(p64).max()) ** 2 / sigma2
    gap = None
    ml2 = None
    if search in EXHAUSTIVE:
        assert NL * Qm <= MAX_BITS
        cand = candidates(NL, Qm)
        v = metrics(Y, H, p64[cand], sigma2)
        k = int(np.argmin(v))
        idx, minv = cand[k], v[k]
        gap = np.partition(v, 1)[1] - minv if v.size > 1 else np.inf
        if search == "ml2":
            c = np.arange(v.size)
            ml2 = np.empty(NL * Qm)
            for n in range(NL * Qm):
                one = ((c >> (NL * Qm - 1 - n)) & 1).astype(bool)
                ml2[n] = v[one].min() - v[~one].min()
        S = p64[idx]
    elif search == "subset":
        sel = [np.argsort(np.abs(pts - e), kind="stable")[:min(M, 4)] for e in est]
        cand = np.array(list(itertools.product(*sel)))
        v = metrics(Y, H, p64[cand], sigma2)
        k = int(np.argmin(v))
        idx, minv = cand[k], v[k]
        S = p64[idx]
    else:
        k, s1, minv = _rank2(Y, H, pts, sigma2)
        S = np.array([p64[k], np.complex128(s1)])
        hit = np.nonzero(pts == s1)[0]
        # BPSK slices the two axes independently: a point off the constellation takes the bit of
        # its real axis (the reference raises there; such cases are not in the fixture)
        i1 = int(hit[0]) if hit.size else int(np.nonzero(pts.real == s1.real)[0][0])
        idx = np.array([k, i1])
    hb = bits[idx].reshape(-1)
    if search == "hard":
        llr = 1.0 - 2.0 * hb
    elif search == "ml2":
        llr = ml2
    else:
        llr = np.empty(NL * Qm)
        for l in range(NL):
            for m in range(Qm):
                So = S.copy()
                So[l] = p64[opposite_index(int(idx[l]), m, Qm)]
                dis = metrics(Y, H, So[None], sigma2)[0]
                llr[l * Qm + m] = minv - dis if hb[l * Qm + m] else -minv + dis
    return dict(sym=S.astype(np.complex64), nv=float(minv), hardbits=hb, llr=llr, fired_cov=fired, gap=gap,
                scale=float(scale))


def ml_detect(y, h, cov, mod, algo, re_idx=None, re_per_cov=12):
    """y (R, Nr), h (R, Nr, NL), cov (ceil(R/re_per_cov), Nr, Nr) of one transport block ->
    dict(llr (nre*NL*Qm,), sym (nre*NL,) complex64, nv (nre*NL,), hardbits (nre*NL*Qm,) int8,
    fired_cov (nre,), scale (nre,)) in the layout of ldpc5g_ml_detect."""
    y, h, cov = (np.asarray(a, np.complex128) for a in (y, h, cov))
    R = y.shape[0]
    NL = h.shape[2]
    idx = np.arange(R) if re_idx is None else np.asarray(re_idx, np.int64)
    rs = [detect_one(y[r], h[r], cov[r // re_per_cov], mod, algo) for r in idx]
    return dict(llr=np.concatenate([r["llr"] for r in rs]), sym=np.concatenate([r["sym"] for r in rs]),
                nv=np.repeat([r["nv"] for r in rs], NL), hardbits=np.concatenate([r["hardbits"] for r in rs]),
                fired_cov=np.array([r["fired_cov"] for r in rs]), scale=np.array([r["scale"] for r in rs]))


def load_golden(path):
    """{(Nr, NL, mod): dict(y, h, cov, kind, and per algorithm dict(s, nv, hb, llr, fired_cov,
    scale, ok))} from ml_golden.npz (tests/golden/gen_ml_golden.py).  ok marks the REs the
    algorithm was run on (kind 2: IRC forms only; kind 3: exhaustive searches only)."""
    d = np.load(path)
    out = {}
    for i, (Nr, NL, mod) in enumerate(SETS):
        p = f"s{i}_"
        c = {k: d[p + k] for k in ("y", "h", "cov", "kind")}
        for a in set_algos(Nr, NL, mod):
            c[a] = {k: d[p + a + "_" + k] for k in ("s", "nv", "hb", "llr", "fired_cov", "scale", "ok")}
        out[(Nr, NL, mod)] = c
    return out
