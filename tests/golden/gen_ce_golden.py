"""Generate tests/golden/ce_golden_<case>.npz by running the REFERENCE's channel estimators
(py5gphy/channel_estimate/dft_dct_CE.py, dft_dct_symmetric_CE.py and, for case G,
NrChannelEstimation.channel_est of nr_channel_estimation.py).  The reference never travels: only
the inputs and its outputs below are committed.

    python tests/golden/gen_ce_golden.py <root of a py5gphy checkout>

The cases (tests/ce_ref.py CASES) are the smallest shapes that reach every branch.  H_LS is a sum
of three complex exponentials per (nr, nt) with delays in 0..300 ns (case G: 80 ns more on every
path) plus complex Gaussian noise at 10..30 dB, cast to complex64; scs = 30 kHz.
The reference's kept-tap mask of every sequence is recorded while it runs, by wrapping
scipy.fft.fft / scipy.fft.idct (the back transforms) and noting which inputs are non-zero.
Asserted here, on every sequence of every case:
  1. every tap the threshold decides has | |tap| / sqrt(P/2) - 1 | >= 1e-4 in ce_ref (the noise is
     redrawn otherwise): the reference transforms in single precision, so a tap closer than ~1e-6
     could fall either way;
  2. ce_ref's mask equals the reference's mask;
  3. gap_h, gap_cov = max |ce_ref - reference| / max |reference| <= 64 * 2^-23.
Stored per case: h_ls (S, N, Nr, Nt) complex64, h (14, N*D, Nr, Nt) and cov (14, PRB, Nr, Nr)
complex64 as the reference returns them, taps (packed bits of (S, Nr, Nt, M)) and taps_shape,
gap_h, gap_cov; case G also to_est (S,) float64 and h_ls_comp, the reference's H_LS after its
in-place compensation.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import ce_ref  # noqa: E402

GAP_MAX = 64 * 2.0 ** -23
MARGIN = 1e-4


def draw_signal(rng, cfg):
    S, D = len(cfg["sym_map"]), cfg["D"]
    N = cfg["PRB"] * 12 // D
    Nr, Nt = cfg["Nr"], cfg["Nt"]
    f = np.arange(N) * D * ce_ref.SCS * 1000.0
    sig = np.zeros((S, N, Nr, Nt), np.complex128)
    extra = 80e-9 if cfg["to_comp"] else 0.0
    for nr in range(Nr):
        for nt in range(Nt):
            for _ in range(3):
                tau = rng.uniform(0, 300e-9) + extra
                amp = (rng.standard_normal() + 1j * rng.standard_normal()) / np.sqrt(2)
                drift = rng.uniform(-0.02, 0.02)   # a slow rotation over the slot: the line fit has a slope
                for m, s in enumerate(cfg["sym_map"]):
                    sig[m, :, nr, nt] += amp * np.exp(1j * drift * s) * np.exp(-2j * np.pi * tau * f)
    return sig


def draw_noise(rng, sig):
    snr_db = rng.uniform(10, 30)
    p = np.mean(np.abs(sig) ** 2)
    n = (rng.standard_normal(sig.shape) + 1j * rng.standard_normal(sig.shape)) / np.sqrt(2)
    return n * np.sqrt(p / 10 ** (snr_db / 10))


def run_reference(mods, cfg, H_LS):
    """(H_result, cov_m, mask (S, Nr, Nt, M), extras) with the mask read off the back transforms."""
    import scipy.fft
    S, N, Nr, Nt = H_LS.shape
    RS_info = {"RE_distance": cfg["D"], "scs": ce_ref.SCS, "RSSymMap": list(cfg["sym_map"]),
               "NumCDMGroupsWithoutData": cfg["cdm"]}
    CE_config = {"enable_TO_comp": cfg["to_comp"], "enable_FO_est": False, "enable_FO_comp": False,
                 "CE_algo": cfg["algo"], "L_symm_left_in_ns": cfg["win"][0], "L_symm_right_in_ns": cfg["win"][1],
                 "eRB": cfg["eRB"], "freq_intp_method": "linear", "timing_intp_method": "linear"}
    seen = []
    real_fft, real_idct = scipy.fft.fft, scipy.fft.idct

    def spy_fft(x, *a, **k):
        seen.append(np.asarray(x) != 0)
        return real_fft(x, *a, **k)

    def spy_idct(x, *a, **k):
        seen.append(np.asarray(x) != 0)
        return real_idct(x, *a, **k)
    scipy.fft.fft, scipy.fft.idct = spy_fft, spy_idct
    extras = {}
    try:
        H = H_LS.copy()
        if cfg["to_comp"]:
            ce = mods["nce"].NrChannelEstimation(H, RS_info, CE_config)
            Hr, cov = ce.channel_est()
            extras = {"to_est": np.asarray(ce.TO_est, np.float64), "h_ls_comp": H}
        else:
            model = "DCT" if cfg["algo"].startswith("DCT") else "DFT"
            fn = mods["sym"].DFT_DCT_symmetric_channel_estimate if cfg["algo"].endswith("_symmetric") else \
                mods["plain"].DFT_DCT_channel_estimate
            Hr, cov = fn(H, RS_info, CE_config, model)
    finally:
        scipy.fft.fft, scipy.fft.idct = real_fft, real_idct
    assert len(seen) == S * Nr * Nt, (len(seen), S, Nr, Nt)
    M = seen[0].size
    mask = np.zeros((S, Nr, Nt, M), bool)
    i = 0
    for m in range(S):          # the reference's loop order: symbol, nt, nr
        for nt in range(Nt):
            for nr in range(Nr):
                mask[m, nr, nt] = seen[i]
                i += 1
    return Hr, cov, mask, extras


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ["PY5GPHY_ROOT"]
    sys.path.insert(0, ref_root)
    from py5gphy.channel_estimate import dft_dct_CE, dft_dct_symmetric_CE, nr_channel_estimation
    mods = {"plain": dft_dct_CE, "sym": dft_dct_symmetric_CE, "nce": nr_channel_estimation}
    rng = np.random.default_rng(20261020)
    for name, cfg in ce_ref.CASES.items():
        sig = draw_signal(rng, cfg)
        redraws = 0
        while True:
            H_LS = (sig + draw_noise(rng, sig)).astype(np.complex64)
            mine = ce_ref.run_case(cfg, H_LS)
            if mine["margin"] >= MARGIN:
                break
            redraws += 1
        Hr, cov, mask, extras = run_reference(mods, cfg, H_LS)
        assert Hr.dtype == np.complex64 and cov.dtype == np.complex64
        assert mask.shape == mine["taps"].shape and np.array_equal(mask, mine["taps"]), name
        gap_h = float(np.abs(mine["h"] - Hr).max() / np.abs(Hr).max())
        gap_cov = float(np.abs(mine["cov"] - cov).max() / np.abs(cov).max())
        assert gap_h <= GAP_MAX and gap_cov <= GAP_MAX, (name, gap_h, gap_cov)
        store = dict(h_ls=H_LS, h=Hr, cov=cov, taps=np.packbits(mask), taps_shape=np.array(mask.shape, np.int32),
                     gap_h=np.float64(gap_h), gap_cov=np.float64(gap_cov))
        if extras:
            assert np.abs(extras["to_est"] - mine["to_est"]).max() <= 4e-7 * np.abs(extras["to_est"]).max()
            store.update(extras)
        path = os.path.join(OUT, f"ce_golden_{name}.npz")
        np.savez_compressed(path, **store)
        size = os.path.getsize(path)
        assert size <= 512 * 1024, size
        print(f"{name}: M={mask.shape[-1]} kept={int(mask.sum())} margin={mine['margin']:.2e} redraws={redraws} "
              f"gap_h={gap_h:.2e} gap_cov={gap_cov:.2e} {size} bytes")


if __name__ == "__main__":
    main()
