"""Vectorised float64 numpy restatement of the reference's DFT / DCT channel estimators
(py5gphy/channel_estimate/dft_dct_CE.py:10-257, dft_dct_symmetric_CE.py:11-118) with the timing
offset of nr_channel_estimation.py:66-83,150-221 — the role eq_ref.py / ml_ref.py play for the
detectors.  It is what include/ldpc5g.h describes under ldpc5g_channel_estimate, step by step, for
one slot; the reference itself stores complex64 and transforms in single precision, so it agrees
with this only to its own rounding (the gaps tests/golden/gen_ce_golden.py stores per case)."""
import glob
import os

import numpy as np

ALGOS = ("DFT", "DCT", "DFT_symmetric", "DCT_symmetric")
NSYM = 14


def lengths(N, algo, eRB, D=4):
    """(eK, right_eK, M)"""
    eK = eRB * 12 // D
    reK = eK + (N + eK) % 2
    Mh = N + eK + reK
    return eK, reK, 2 * Mh if algo.endswith("_symmetric") else Mh


def window(algo, M, scs, D, l_left_ns, l_right_ns):
    """(L_left, L_right) — the two files' own wordings (dft_dct_CE.py:64-68,
    dft_dct_symmetric_CE.py:73-79)."""
    if algo.endswith("_symmetric"):
        rate = M * scs * 1000 * D
        L = int(l_left_ns / (10**9 / rate))
        L = min(M // 3 + M // 16, L)
        return L, L
    rate = scs * 1000 * D * M
    return int(l_left_ns * 1e-9 * rate), int(l_right_ns * 1e-9 * rate)


def line_weights(sym_map):
    """w (14, S): the degree-1 least-squares line through (sym_map, y) evaluated at 0..13 is w @ y;
    S = 1 copies."""
    x = np.asarray(sym_map, np.float64)
    S = x.size
    if S == 1:
        return np.ones((NSYM, 1))
    xm = x.sum() / S
    sxx = ((x - xm) ** 2).sum()
    s = np.arange(NSYM, dtype=np.float64)[:, None]
    return 1.0 / S + (s - xm) * (x - xm)[None, :] / sxx


def _edge_fit(pts, xq):
    """Degree-1 least-squares line through pts (..., P) at abscissae 0..P-1, evaluated at xq."""
    P = pts.shape[-1]
    x = np.arange(P, dtype=np.float64)
    xm = 0.5 * (P - 1)
    mean = pts.sum(-1, keepdims=True) / P
    b = ((x - xm) * (pts - mean)).sum(-1, keepdims=True) / ((x - xm) ** 2).sum()
    return mean + b * (np.asarray(xq, np.float64) - xm)


def _dct_matrix(M):
    """C[k, n] = cos(pi k (2n + 1) / (2M)) from the reduced index k (2n + 1) mod 4M."""
    k = np.arange(M, dtype=np.int64)[:, None]
    n = np.arange(M, dtype=np.int64)[None, :]
    return np.cos(2.0 * np.pi * ((k * (2 * n + 1)) % (4 * M)) / (4.0 * M))


def timing_offset(H_LS, scs, D):
    """(TO_est (S,), avg, peak (nr, nt)) — find_peak_H_LS and timing_offset_est."""
    S, N, Nr, Nt = H_LS.shape
    best, loc = 0.0, (0, 0)
    for nt in range(Nt):
        for nr in range(Nr):
            x = H_LS[:, :, nr, nt]
            p = abs(np.mean(x * np.conj(x)))
            if p > best:
                best, loc = p, (nr, nt)
    pk = H_LS[:, :, loc[0], loc[1]]
    c = pk[:, 1:] * np.conj(pk[:, :-1])
    to = (np.arctan2(c.imag, c.real) / (2 * np.pi * D * scs * 1000)).mean(axis=1)
    return to, float(np.mean(to)), loc


def to_phase(avg, step, n, scs):
    return np.exp(-1j * 2 * np.pi * avg * step * np.arange(n) * scs * 1000)


def estimate(H_LS, sym_map, algo, scs, eRB, l_left_ns, l_right_ns, D=4, num_cdm_groups=2, to_comp=False):
    """One slot.  H_LS: (S, N, Nr, Nt).  Returns a dict: h (14, N*D, Nr, Nt), cov (14, PRB, Nr, Nr),
    h_est (S, N*D, Nr, Nt), noise_power (S, Nr, Nt), taps (S, Nr, Nt, M) bool, margin (the smallest
    | |tap| / sqrt(P/2) - 1 | over the taps the threshold decides), to_est (S,), to_avg, h_ls_comp."""
    H_LS = np.asarray(H_LS, np.complex128)
    S, N, Nr, Nt = H_LS.shape
    assert algo in ALGOS and len(sym_map) == S
    sym, dct = algo.endswith("_symmetric"), algo.startswith("DCT")
    to_est, to_avg, _ = timing_offset(H_LS, scs, D)
    if to_comp:
        H_LS = H_LS * to_phase(to_avg, D, N, scs)[None, :, None, None]
    eK, reK, M = lengths(N, algo, eRB, D)
    L_left, L_right = window(algo, M, scs, D, l_left_ns, l_right_ns)
    assert L_left + L_right < M
    x = np.moveaxis(H_LS, 1, -1)   # (S, Nr, Nt, N)
    P = 24 // D
    left = _edge_fit(x[..., :P], np.arange(-eK, 0))
    right = _edge_fit(x[..., N - P:], np.arange(P, P + reK))
    ext = np.concatenate([left, x, right], axis=-1)
    if sym:
        ext = np.concatenate([ext, ext[..., ::-1]], axis=-1)
    assert ext.shape[-1] == M
    if dct:
        Cm = _dct_matrix(M)
        sk = np.full(M, np.sqrt(2.0 / M))
        sk[0] = 1.0 / np.sqrt(M)
        tap = (ext @ Cm.T) * sk
    else:
        tap = np.fft.ifft(np.fft.ifftshift(ext, axes=-1), axis=-1) * np.sqrt(M)
    mag = np.abs(tap)
    noise = np.mean(mag[..., L_left:M - L_right] ** 2, axis=-1)
    thr = np.sqrt(noise / 2)[..., None]
    outside = np.ones(M, bool)
    outside[L_left:M - L_right] = False
    keep = (mag >= thr) & outside
    margin = float(np.abs(mag[..., outside] / thr - 1).min()) if outside.any() else np.inf
    tap = np.where(keep, tap, 0)
    if dct:
        f = (tap * sk) @ Cm
    else:
        f = np.fft.fftshift(np.fft.fft(tap, axis=-1), axes=-1) / np.sqrt(M)
    # linear interpolation to every subcarrier, the last value held
    nxt = np.concatenate([f[..., 1:], f[..., -1:]], axis=-1)
    j = np.arange(D, dtype=np.float64) / D
    intp = (f[..., :, None] + j * (nxt - f)[..., :, None]).reshape(S, Nr, Nt, M * D)
    h_est = np.moveaxis(intp[..., eK * D:eK * D + N * D], -1, 1)   # (S, N*D, Nr, Nt)
    W = line_weights(sym_map)
    h = np.tensordot(W, h_est, axes=(1, 0))
    # covariance
    nHS = H_LS - h_est[:, ::D]
    per = 16 * 12 // D
    ng = N // per
    PRB = N * D // 12
    cov_m = np.zeros((S, PRB, Nr, Nr), np.complex128)
    for g in range(ng):
        r0 = g * per
        r1 = N if g == ng - 1 else r0 + per
        p1 = PRB if g == ng - 1 else (g + 1) * 16
        d = nHS[:, r0:r1]
        c = np.einsum("sran,srbn->sab", d, np.conj(d)) / (r1 - r0) / Nt
        cov_m[:, g * 16:p1] = c[:, None]
    if num_cdm_groups == 1:
        cov_m = cov_m * 2
    cov = np.tensordot(W, cov_m, axes=(1, 0))
    return dict(h=h, cov=cov, h_est=h_est, noise_power=noise, taps=keep, margin=margin, to_est=to_est,
                to_avg=to_avg, h_ls_comp=H_LS, M=M, L_left=L_left, L_right=L_right)


def compensate_data(y, to_avg, scs):
    """comp_pdsch_timing_offset: y (nsym, RE, Nr)."""
    return np.asarray(y, np.complex128) * to_phase(to_avg, 1, y.shape[1], scs)[None, :, None]


# ---------------------------------------------------------------- the committed fixture
CASES = {   # name: PRB, RSSymMap, Nr, Nt, algo, D, eRB, (left ns, right ns), CDM groups, TO compensation
    "A": dict(PRB=16, sym_map=[2], Nr=1, Nt=1, algo="DFT", D=4, eRB=4, win=(1400, 1200), cdm=1, to_comp=False),
    "B": dict(PRB=17, sym_map=[2, 11], Nr=2, Nt=1, algo="DCT", D=4, eRB=4, win=(1400, 1200), cdm=2, to_comp=False),
    "C": dict(PRB=20, sym_map=[2, 11], Nr=2, Nt=2, algo="DFT_symmetric", D=4, eRB=4, win=(1400, 1200), cdm=2,
              to_comp=False),
    "D": dict(PRB=36, sym_map=[2, 7, 11], Nr=4, Nt=2, algo="DCT_symmetric", D=4, eRB=4, win=(1400, 1200), cdm=2,
              to_comp=False),
    "E": dict(PRB=17, sym_map=[2, 5, 8, 11], Nr=4, Nt=4, algo="DFT", D=4, eRB=2, win=(100, 200), cdm=2,
              to_comp=False),
    "F": dict(PRB=16, sym_map=[2, 11], Nr=2, Nt=2, algo="DFT_symmetric", D=2, eRB=4, win=(1400, 1200), cdm=2,
              to_comp=False),
    "G": dict(PRB=20, sym_map=[2, 11], Nr=2, Nt=2, algo="DFT_symmetric", D=4, eRB=4, win=(1400, 1200), cdm=2,
              to_comp=True),
}
SCS = 30


def run_case(cfg, H_LS):
    return estimate(H_LS, cfg["sym_map"], cfg["algo"], SCS, cfg["eRB"], cfg["win"][0], cfg["win"][1], cfg["D"],
                    cfg["cdm"], cfg["to_comp"])


def load_golden(gold_dir):
    """{case: dict(cfg, h_ls, h, cov, taps (S, Nr, Nt, M) bool, gap_h, gap_cov[, to_est, h_ls_comp])}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(gold_dir, "ce_golden_*.npz"))):
        name = os.path.basename(path)[len("ce_golden_"):-len(".npz")]
        d = np.load(path)
        c = dict(cfg=CASES[name], h_ls=d["h_ls"], h=d["h"], cov=d["cov"], gap_h=float(d["gap_h"]),
                 gap_cov=float(d["gap_cov"]))
        shape = tuple(d["taps_shape"])
        c["taps"] = np.unpackbits(d["taps"])[:int(np.prod(shape))].astype(bool).reshape(shape)
        if "to_est" in d.files:
            c["to_est"], c["h_ls_comp"] = d["to_est"], d["h_ls_comp"]
        out[name] = c
    return out
