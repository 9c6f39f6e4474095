"""Drop-in for py5gphy/channel_equalization/opt_rank2_ML.py — the O(M) maximum-likelihood search
for two layers; one resource element per call on the GPU (ldpc5g_ml_detect).  NL != 2 runs
ML-soft, as the reference does (whatever demod_decision says, opt_rank2_ML.py:15-16, 44-45).

    opt_rank2_ML / opt_rank2_ML_IRC (Y (Nr,), H (Nr, NL), cov (Nr, Nr), modtype, demod_decision="soft")
        -> (s_est complex64 (NL,), noise_var float64 (NL,), de_hardbits int64 (NL*Qm,),
            LLR_a float64 (NL*Qm,))
"""
import numpy as np

from ._ml_dropin import detect


def _run(Y, H, cov, modtype, demod_decision, algo):
    assert demod_decision in ("soft", "hard"), demod_decision
    s_est, noise_var, de_hardbits, LLR_a = detect(Y, H, cov, modtype, algo)
    if demod_decision == "hard" and np.asarray(H).shape[1] == 2:
        LLR_a = 1 - 2 * de_hardbits   # opt_rank2_ML.py:166-167
    return s_est, noise_var, de_hardbits, LLR_a


def opt_rank2_ML_IRC(Y, H, cov, modtype, demod_decision="soft"):
    """opt_rank2_ML.py:9-36"""
    return _run(Y, H, cov, modtype, demod_decision, "opt-rank2-ML-IRC")


def opt_rank2_ML(Y, H, cov, modtype, demod_decision="soft"):
    """opt_rank2_ML.py:38-171"""
    return _run(Y, H, cov, modtype, demod_decision, "opt-rank2-ML")
