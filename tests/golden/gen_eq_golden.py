"""Generate tests/golden/eq_golden.npz by running the REFERENCE's linear equalisers (py5gphy
channel_equalization/ZF.py and MMSE.py) one resource element at a time, as channel_equ_and_demod
does.  The reference never travels: only the inputs and its outputs below are committed.

    python tests/golden/gen_eq_golden.py <root of a py5gphy checkout>

Per (Nr, NL) in {(1,1), (2,1), (2,2), (4,1), (4,2), (4,3), (4,4)}, one input set shared by the
four algorithms, laid out as one transport block of ldpc5g_equalize (covariance per 12 REs):
  kind 0  96 regular REs (8 covariance blocks): complex Gaussian H and Y,
          cov = (I + 0.5 g g^H) / snr made exactly Hermitian, snr log-uniform in [1, 1e4];
          redrawn until sigma_min/sigma_max(H^H H) >= 1e-4; kappa(cov) <= 1e2 asserted
  kind 1  12 REs whose last column of H duplicates column 0 (NL >= 2): singular W1 for ZF / ZF-IRC
  kind 2  12 REs with the rank-1 cov = g g^H (Nr >= 2): singular cov for MMSE-IRC
The branch the reference took is recorded from its own np.linalg.matrix_rank calls (wrapped while
it runs): fired_w1 / fired_cov per RE and algorithm.  A singular case is kept only if the rank
test fired; a regular case only if it did not.
Stored per shape under the prefix s<Nr><NL>_: y (R, Nr), h (R, Nr, NL), cov (R/12, Nr, Nr)
complex128, kind (R,) int8, and per algorithm <algo>_s (R, NL) complex128, <algo>_nv (R, NL)
float64, <algo>_fired_w1 / <algo>_fired_cov (R,) bool.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
from eq_ref import ALGOS, SHAPES  # noqa: E402

PER_COV = 12


def crandn(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def hermitian(a):
    a = (a + np.conj(a.T)) / 2
    a[np.diag_indices_from(a)] = np.diagonal(a).real
    return a


def run_reference(funcs, Y, H, cov):
    """{algo: (s (NL,), nv (NL,), fired_w1, fired_cov)} with the outcomes of the reference's own
    matrix_rank tests."""
    Nr, NL = H.shape
    out = {}
    real_rank = np.linalg.matrix_rank
    for algo in ALGOS:
        calls = []

        def spy(A, *a, **k):
            r = real_rank(A, *a, **k)
            calls.append(bool(r < A.shape[0]))
            return r
        np.linalg.matrix_rank = spy
        try:
            s, nv = funcs[algo](Y.copy(), H.copy(), cov.copy())
        finally:
            np.linalg.matrix_rank = real_rank
        if Nr == 1:
            assert not calls
            fw, fc = False, False
        elif algo == "MMSE-IRC":
            fc, fw = calls
        else:
            (fw,), fc = calls, False
        s = np.asarray(s, np.complex128).reshape(NL)
        nv = np.asarray(nv)
        if np.iscomplexobj(nv):   # the Nr == 1 shortcut returns cov / (conj(H) H) as a complex number
            assert np.all(np.abs(nv.imag) <= 1e-15 * np.abs(nv.real)), nv
        out[algo] = (s, nv.real.astype(np.float64).reshape(NL), fw, fc)
    return out


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ["PY5GPHY_ROOT"]
    sys.path.insert(0, ref_root)
    from py5gphy.channel_equalization import MMSE, ZF
    funcs = {"ZF": ZF.ZF, "ZF-IRC": ZF.ZF_IRC, "MMSE": MMSE.MMSE, "MMSE-IRC": MMSE.MMSE_IRC}
    rng = np.random.default_rng(20261019)
    store = {}
    for Nr, NL in SHAPES:
        kinds = [0] * 8 + ([1] if NL >= 2 else []) + ([2] if Nr >= 2 else [])
        ys, hs, covs, kind = [], [], [], []
        res = {a: ([], [], [], []) for a in ALGOS}
        for kd in kinds:
            while True:   # one covariance block of 12 REs; redrawn as a whole if a case is unfit
                g = crandn(rng, Nr)
                snr = 10 ** rng.uniform(0, 4)
                cov = hermitian(np.outer(g, np.conj(g))) if kd == 2 else \
                    hermitian((np.identity(Nr) + 0.5 * np.outer(g, np.conj(g))) / snr)
                if kd != 2:
                    assert np.linalg.cond(cov) <= 1e2
                blk = []
                for _ in range(PER_COV):
                    H = crandn(rng, Nr, NL)
                    if kd == 1:
                        H[:, NL - 1] = H[:, 0]
                    Y = crandn(rng, Nr)
                    sv = np.linalg.svd(np.conj(H.T) @ H, compute_uv=False)
                    if kd != 1 and sv[-1] / sv[0] < 1e-4:
                        break
                    r = run_reference(funcs, Y, H, cov)
                    fw = [r[a][2] for a in ALGOS]
                    fc = [r[a][3] for a in ALGOS]
                    want_w = [kd == 1 and Nr > 1, kd == 1 and Nr > 1, False, False]   # ZF / ZF-IRC: H^H H singular
                    want_c = [False, False, False, kd == 2]
                    if fw != want_w or fc != want_c:
                        break
                    blk.append((Y, H, r))
                if len(blk) == PER_COV:
                    break
            covs.append(cov)
            for Y, H, r in blk:
                ys.append(Y), hs.append(H), kind.append(kd)
                for a in ALGOS:
                    for lst, v in zip(res[a], r[a]):
                        lst.append(v)
        p = f"s{Nr}{NL}_"
        store[p + "y"] = np.array(ys, np.complex128)
        store[p + "h"] = np.array(hs, np.complex128)
        store[p + "cov"] = np.array(covs, np.complex128)
        store[p + "kind"] = np.array(kind, np.int8)
        for a in ALGOS:
            store[p + a + "_s"] = np.array(res[a][0], np.complex128)
            store[p + a + "_nv"] = np.array(res[a][1], np.float64)
            store[p + a + "_fired_w1"] = np.array(res[a][2], bool)
            store[p + a + "_fired_cov"] = np.array(res[a][3], bool)
        print(Nr, NL, "REs", len(ys), "singular-H", kind.count(1), "rank-1 cov", kind.count(2))
    path = os.path.join(OUT, "eq_golden.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    assert size <= 512 * 1024, size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
