"""Drop-in for py5gphy/channel_equalization/ML.py — exhaustive maximum-likelihood detection of
one resource element per call on the GPU (ldpc5g_ml_detect, float64 arithmetic).  phy.ml_detect /
sch.sch_ml_rx_batch take the whole slot in one launch and are the fast path; these exist for
callers that keep the reference's loop over the slot.

    ML / ML_IRC (Y (Nr,), H (Nr, NL), cov (Nr, Nr), modtype, demod_decision="soft")
        -> (s_est complex64 (NL,), noise_var float64 (NL,), de_hardbits int64 (NL*Qm,),
            LLR_a float64 (NL*Qm,))

M^NL is capped at 65 536 candidates (include/ldpc5g.h); beyond it the call raises AssertionError
naming opt-rank2-ML.
"""
from ._ml_dropin import detect


def _algo(irc, demod_decision):
    assert demod_decision in ("soft", "hard"), demod_decision
    return ("ML-IRC-" if irc else "ML-") + demod_decision


def ML_IRC(Y, H, cov, modtype, demod_decision="soft"):
    """ML.py:9-45"""
    return detect(Y, H, cov, modtype, _algo(True, demod_decision))


def ML(Y, H, cov, modtype, demod_decision="soft"):
    """ML.py:47-98"""
    return detect(Y, H, cov, modtype, _algo(False, demod_decision))
