"""Generate tests/golden/ml_golden.npz by running the REFERENCE's maximum-likelihood detectors
(py5gphy channel_equalization/ML.py, ML2.py, MMSE_ML.py, opt_rank2_ML.py) one resource element at
a time, as channel_equ_and_demod does.  The reference never travels: only the inputs and its
outputs below are committed.

    python tests/golden/gen_ml_golden.py <root of a py5gphy checkout>

Sets (Nr, NL, mod): ml_ref.SETS.  Each is laid out as one transport block of ldpc5g_ml_detect
(covariance per 12 REs):
  kind 0  regular REs: Y = H s + noise for a random constellation vector s, complex Gaussian H,
          cov = (I + 0.5 g g^H) / snr made exactly Hermitian, snr log-uniform in [1, 1e4], noise
          drawn with that covariance.  24 REs (two covariance blocks); 4 for the two sets with
          65 536 candidates, 12 for (2, 2, 1024qam), which only has MMSE-ML and opt-rank2-ML.
  kind 2  (Nr >= 2) 12 REs with the rank-1 cov = g g^H, run on the IRC forms only; kept only if
          the reference's own matrix_rank test fired (np.linalg.matrix_rank wrapped while it runs)
  kind 3  (NL >= 2) 12 REs with H[:, NL-1] = 0, run on the exhaustive searches only: every
          candidate of that layer ties exactly
The two sets with 65 536 candidates and (2, 2, 1024qam) have kind 0 only.
An RE is redrawn unless, for every algorithm it is run on: the reference raised nothing
(opt_rank2_ML's assert can fire); the two smallest metrics of the search differ by at least
1e-6 * scale (kind 3 excepted); for MMSE-ML the 4th and 5th nearest distances to the MMSE estimate
differ by at least 1e-6; kind 0 did not fire the rank test.
Stored per set i under the prefix s<i>_: y (R, Nr), h (R, Nr, NL), cov (R/12, Nr, Nr) complex128,
kind (R,) int8, and per algorithm <algo>_s (R, NL) complex64, <algo>_nv (R,), <algo>_llr
(R, NL*Qm) float64, <algo>_hb (R, NL*Qm) int8, <algo>_fired_cov (R,) bool, <algo>_scale (R,),
<algo>_ok (R,) bool (the algorithm was run on this RE).  scale = (|Y'| + |H'|_F sqrt(NL)
max|a|)^2 / sigma^2 with Y', H' the inputs the ML core sees: for IRC the reference's own
cov_inverse_decompose applied, sigma^2 = 1.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import ml_ref  # noqa: E402

PER_COV = 12
GAP = 1e-6


def crandn(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def hermitian(a):
    a = (a + np.conj(a.T)) / 2
    a[np.diag_indices_from(a)] = np.diagonal(a).real
    return a


class Ref:
    def __init__(self, root):
        sys.path.insert(0, root)
        from py5gphy.channel_equalization import ML, ML2, MMSE, MMSE_ML, nr_channel_eq, opt_rank2_ML
        from py5gphy.common import nrModulation
        self.eq = nr_channel_eq
        self.mmse = MMSE
        self.mod = nrModulation
        self.funcs = {
            "ML-soft": lambda Y, H, c, m: ML.ML(Y, H, c, m, "soft"),
            "ML-IRC-soft": lambda Y, H, c, m: ML.ML_IRC(Y, H, c, m, "soft"),
            "ML-hard": lambda Y, H, c, m: ML.ML(Y, H, c, m, "hard"),
            "ML-IRC-hard": lambda Y, H, c, m: ML.ML_IRC(Y, H, c, m, "hard"),
            "ML2-soft": lambda Y, H, c, m: ML2.ML(Y, H, c, m, "soft"),
            "ML2-IRC-soft": lambda Y, H, c, m: ML2.ML_IRC(Y, H, c, m, "soft"),
            "MMSE-ML": MMSE_ML.MMSE_ML, "MMSE-ML-IRC": MMSE_ML.MMSE_ML_IRC,
            "opt-rank2-ML": opt_rank2_ML.opt_rank2_ML, "opt-rank2-ML-IRC": opt_rank2_ML.opt_rank2_ML_IRC}

    def run(self, algo, Y, H, cov, mod):
        """(s, nv, hb, llr, fired_cov, scale) of the reference, or None if it raised."""
        Nr, NL = H.shape
        irc = ml_ref.ALGOS[algo][1]
        real_rank = np.linalg.matrix_rank
        calls = []

        def spy(A, *a, **k):
            r = real_rank(A, *a, **k)
            calls.append(bool(r < A.shape[0]))
            return r
        np.linalg.matrix_rank = spy
        try:
            with np.errstate(all="ignore"):
                s, nv, hb, llr = self.funcs[algo](Y.copy(), H.copy(), cov.copy(), mod)
        except (AssertionError, IndexError):
            return None
        finally:
            np.linalg.matrix_rank = real_rank
        # MMSE-ML-IRC tests cov inside MMSE_IRC first; every IRC form then in cov_inverse_decompose
        fired = bool(calls[0]) if irc else False
        if irc:
            U = self.eq.cov_inverse_decompose(cov.copy())
            Yw, Hw, sigma2 = U @ Y, U @ H, 1.0
        else:
            Yw, Hw, sigma2 = Y, H, np.mean(np.diagonal(cov)).real
        amax = np.abs(self.mod.get_mod_list(mod)[0].astype(np.complex128)).max()
        scale = (np.linalg.norm(Yw) + np.linalg.norm(Hw) * np.sqrt(NL) * amax) ** 2 / sigma2
        nv = np.asarray(nv, np.float64).reshape(-1)
        assert np.all(nv == nv[0])
        return (np.asarray(s).reshape(NL).astype(np.complex64), float(nv[0]), np.asarray(hb, np.int8).reshape(-1),
                np.asarray(llr, np.float64).reshape(-1), fired, float(scale))

    def mmse_gap_ok(self, Y, H, cov, mod, irc):
        est, _ = (self.mmse.MMSE_IRC if irc else self.mmse.MMSE)(Y.copy(), H.copy(), cov.copy())
        pts = self.mod.get_mod_list(mod)[0]
        if pts.size <= 4:
            return True
        for e in np.asarray(est).reshape(-1):
            d = np.sort(np.abs(pts - e))
            if d[4] - d[3] < GAP:
                return False
        return True


def applies(algo, kd):
    search, irc = ml_ref.ALGOS[algo]
    if kd == 2:
        return bool(irc)
    if kd == 3:
        return search in ml_ref.EXHAUSTIVE
    return True


def gap_ok(Y, H, cov, mod, irc):
    """The two smallest metrics over ALL candidates (a superset of every search) differ by
    >= GAP * scale, on the plain or whitened system (ml_ref, chunked over layer 0)."""
    Nr, NL = H.shape
    Qm = ml_ref.QM[mod]
    pts = ml_ref.constellation(mod)[0].astype(np.complex128)
    if irc:
        Y, H, _ = ml_ref.whiten(Y, H, cov)
        sigma2 = 1.0
    else:
        sigma2 = np.diagonal(cov).real.sum() / Nr
    scale = (np.linalg.norm(Y) + np.linalg.norm(H) * np.sqrt(NL) * np.abs(pts).max()) ** 2 / sigma2
    if NL == 1:
        v = ml_ref.metrics(Y, H, pts[:, None], sigma2)
    else:
        rest = ml_ref.candidates(NL - 1, Qm)
        best = []
        for m0 in range(pts.size):   # layer 0 fixed: Y - H[:, 0] s0 against the other layers
            v = ml_ref.metrics(Y - H[:, 0] * pts[m0], H[:, 1:], pts[rest], sigma2)
            best.extend(np.partition(v, 1)[:2])
        v = np.array(best)
    two = np.partition(v, 1)[:2]
    return two[1] - two[0] >= GAP * scale


def main():
    ref = Ref(sys.argv[1] if len(sys.argv) > 1 else os.environ["PY5GPHY_ROOT"])
    rng = np.random.default_rng(20261019)
    store = {}
    for si, (Nr, NL, mod) in enumerate(ml_ref.SETS):
        Qm = ml_ref.QM[mod]
        algos = ml_ref.set_algos(Nr, NL, mod)
        big = NL * Qm >= 16
        pts = ref.mod.get_mod_list(mod)[0]
        if NL * Qm > ml_ref.MAX_BITS:
            blocks = [(0, 12)]
        elif big:
            blocks = [(0, 4)]
        else:
            blocks = [(0, 12), (0, 12)] + ([(2, 12)] if Nr >= 2 else []) + ([(3, 12)] if NL >= 2 else [])
        ys, hs, covs, kind = [], [], [], []
        res = {a: [] for a in algos}
        redraws = 0
        for kd, n in blocks:
            while True:   # one covariance block; a rank-1 cov whose rank test does not fire is redrawn whole
                g = crandn(rng, Nr)
                snr = 10 ** rng.uniform(0, 4)
                cov = hermitian(np.outer(g, np.conj(g))) if kd == 2 else \
                    hermitian((np.identity(Nr) + 0.5 * np.outer(g, np.conj(g))) / snr)
                blk = []
                tries = 0
                while len(blk) < n and tries < 40 * n:
                    tries += 1
                    H = crandn(rng, Nr, NL)
                    if kd == 3:
                        H[:, NL - 1] = 0
                    s = pts[rng.integers(0, pts.size, NL)].astype(np.complex128)
                    Lc = np.linalg.cholesky(cov + (1e-6 if kd == 2 else 0) * np.identity(Nr))
                    Y = H @ s + Lc @ crandn(rng, Nr)
                    ok = True
                    r = {}
                    for irc in (0, 1):
                        if not any(applies(a, kd) and ml_ref.ALGOS[a][1] == irc for a in algos):
                            continue
                        if kd != 3 and not gap_ok(Y, H, cov, mod, irc):
                            ok = False
                        if ok and kd != 3 and not ref.mmse_gap_ok(Y, H, cov, mod, irc):
                            ok = False
                    for a in algos:
                        if not ok:
                            break
                        if not applies(a, kd):
                            continue
                        r[a] = ref.run(a, Y, H, cov, mod)
                        if r[a] is None or r[a][4] != (kd == 2):
                            ok = False
                    if not ok:
                        redraws += 1
                        continue
                    blk.append((Y, H, r))
                if len(blk) == n:
                    break
            covs.append(cov)
            for Y, H, r in blk:
                ys.append(Y), hs.append(H), kind.append(kd)
                for a in algos:
                    res[a].append(r.get(a))
        p = f"s{si}_"
        R = len(ys)
        store[p + "y"] = np.array(ys, np.complex128)
        store[p + "h"] = np.array(hs, np.complex128)
        store[p + "cov"] = np.array(covs, np.complex128)
        store[p + "kind"] = np.array(kind, np.int8)
        for a in algos:
            ok = np.array([x is not None for x in res[a]])
            s = np.zeros((R, NL), np.complex64)
            nv = np.zeros(R)
            hb = np.zeros((R, NL * Qm), np.int8)
            llr = np.zeros((R, NL * Qm))
            fired = np.zeros(R, bool)
            scale = np.ones(R)
            for i, x in enumerate(res[a]):
                if x is not None:
                    s[i], nv[i], hb[i], llr[i], fired[i], scale[i] = x
            for k, v in (("s", s), ("nv", nv), ("hb", hb), ("llr", llr), ("fired_cov", fired), ("scale", scale),
                         ("ok", ok)):
                store[p + a + "_" + k] = v
        print(Nr, NL, mod, "REs", R, "kinds", [kind.count(k) for k in (0, 2, 3)], "redraws", redraws, flush=True)
    path = os.path.join(OUT, "ml_golden.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    assert size <= 512 * 1024, size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
