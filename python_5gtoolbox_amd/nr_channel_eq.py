"""Drop-in for py5gphy/channel_equalization/nr_channel_eq.py (and the ZF / ZF_IRC / MMSE /
MMSE_IRC functions of ZF.py and MMSE.py beside it) — one resource element per call on the GPU
(ldpc5g_equalize, float64 arithmetic).  The reference calls these from a Python double loop over
the slot; phy.equalize / sch.sch_eq_rx_batch take the whole slot in one launch and are the fast
path, these exist for callers that keep the loop.

    ZF / ZF_IRC / MMSE / MMSE_IRC (Y (Nr,), H (Nr, NL), cov (Nr, Nr))
        -> (s_est complex128 (NL,), noise_var float64 (NL,))
    channel_equ_and_demod(Y, H, cov, modtype, CEQ_config) -> (s_est, noise_var, hardbits, LLR)

noise_var holds the float32 values the demodulator uses (nr_Demodulation.py:24 casts them),
widened to float64.  For Nr == 1 the reference returns (1, 1) arrays and a complex noise_var with
zero imaginary part; here both are (1,) and noise_var is real.  Only the four linear algorithms
run on the GPU: the ML family of CEQ_config["algo"] raises NotImplementedError.
"""
import numpy as np

from . import _lib, nr_Demodulation, phy

LINEAR_ALGOS = ("ZF", "ZF-IRC", "MMSE", "MMSE-IRC")


def _equalize(Y, H, cov, algo):
    H = np.asarray(H)
    assert H.ndim == 2
    Nr, NL = H.shape
    Y = np.asarray(Y)
    cov = np.asarray(cov)
    assert Nr >= NL
    assert Nr == Y.size
    assert cov.ndim == 2 and Nr == cov.shape[0] and Nr == cov.shape[1]
    if Nr == 1:
        assert np.abs(H) > 0   # H should not be zero (ZF.py:23)
    t = _lib.require_gpu()

    def dev(a, shape):
        return t.from_numpy(np.array(a, dtype=np.complex128).reshape(shape)).cuda()
    sym, nv = phy.equalize(dev(Y, (1, 1, Nr)), dev(H, (1, 1, Nr, NL)), dev(cov, (1, 1, Nr, Nr)), algo,
                           re_per_cov=1)
    return sym[0].cpu().numpy(), nv[0].cpu().numpy().astype(np.float64)


def ZF(Y, H, cov):
    """ZF.py:47-79"""
    return _equalize(Y, H, cov, "ZF")


def ZF_IRC(Y, H, cov):
    """ZF.py:5-45"""
    return _equalize(Y, H, cov, "ZF-IRC")


def MMSE(Y, H, cov):
    """MMSE.py:58-103"""
    return _equalize(Y, H, cov, "MMSE")


def MMSE_IRC(Y, H, cov):
    """MMSE.py:5-56"""
    return _equalize(Y, H, cov, "MMSE-IRC")


def channel_equ_and_demod(Y, H, cov, modtype, CEQ_config):
    """nr_channel_eq.py:12-50 for the linear algorithms: equalise, then nrDemodulate."""
    algo = CEQ_config["algo"]
    if algo not in LINEAR_ALGOS:
        raise NotImplementedError(
            f"channel equalisation algo {algo!r}: only {', '.join(LINEAR_ALGOS)} run on the GPU "
            "(the ML detectors are not implemented)")
    s_est, noise_var = _equalize(Y, H, cov, algo)
    de_hardbits, LLR_a = nr_Demodulation.nrDemodulate(s_est, modtype, noise_var)
    return s_est, noise_var, de_hardbits, LLR_a
