"""Drop-in for py5gphy/channel_equalization/MMSE_ML.py — MMSE estimate, then a maximum-likelihood
search over the 4 constellation points nearest to it per layer; one resource element per call on
the GPU (ldpc5g_ml_detect).

    MMSE_ML / MMSE_ML_IRC (Y (Nr,), H (Nr, NL), cov (Nr, Nr), modtype)
        -> (s_est complex64 (NL,), noise_var float64 (NL,), de_hardbits int64 (NL*Qm,),
            LLR_a float64 (NL*Qm,))
"""
from ._ml_dropin import detect


def MMSE_ML_IRC(Y, H, cov, modtype):
    """MMSE_ML.py:12-45"""
    return detect(Y, H, cov, modtype, "MMSE-ML-IRC")


def MMSE_ML(Y, H, cov, modtype):
    """MMSE_ML.py:47-69"""
    return detect(Y, H, cov, modtype, "MMSE-ML")
