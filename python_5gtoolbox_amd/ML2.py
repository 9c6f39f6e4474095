"""Drop-in for py5gphy/channel_equalization/ML2.py — exhaustive maximum-likelihood detection
whose soft LLR of a bit is the minimum metric over all candidates with that bit 1 minus the
minimum with it 0; one resource element per call on the GPU (ldpc5g_ml_detect).  The "hard"
decision is ML.py's (the two files share it line for line).

    ML / ML_IRC (Y (Nr,), H (Nr, NL), cov (Nr, Nr), modtype, demod_decision="soft")
        -> (s_est complex64 (NL,), noise_var float64 (NL,), de_hardbits int64 (NL*Qm,),
            LLR_a float64 (NL*Qm,))
"""
from ._ml_dropin import detect


def _algo(irc, demod_decision):
    assert demod_decision in ("soft", "hard"), demod_decision
    if demod_decision == "hard":
        return "ML-IRC-hard" if irc else "ML-hard"
    return "ML2-IRC-soft" if irc else "ML2-soft"


def ML_IRC(Y, H, cov, modtype, demod_decision="soft"):
    """ML2.py:9-45"""
    return detect(Y, H, cov, modtype, _algo(True, demod_decision))


def ML(Y, H, cov, modtype, demod_decision="soft"):
    """ML2.py:47-161"""
    return detect(Y, H, cov, modtype, _algo(False, demod_decision))
