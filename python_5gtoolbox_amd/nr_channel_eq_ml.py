"""channel_equ_and_demod of py5gphy/channel_equalization/nr_channel_eq.py with all fourteen
algorithms: the four linear ones delegate to nr_channel_eq (equalise, then nrDemodulate), the ten
maximum-likelihood ones run on ldpc5g_ml_detect (ML.py, ML2.py, MMSE_ML.py, opt_rank2_ML.py here).
One resource element per call; phy.ml_detect / sch.sch_ml_rx_batch take the whole slot in one
launch and are the fast path.

    channel_equ_and_demod(Y, H, cov, modtype, CEQ_config) -> (s_est, noise_var, de_hardbits, LLR_a)

nr_channel_eq.channel_equ_and_demod itself still refuses the ML names; import this module to get
them.
"""
from . import _lib, nr_channel_eq
from ._ml_dropin import detect

ML_ALGOS = tuple(_lib.ML_ALGO)
ALGOS = nr_channel_eq.LINEAR_ALGOS + ML_ALGOS


def channel_equ_and_demod(Y, H, cov, modtype, CEQ_config):
    """nr_channel_eq.py:12-50"""
    algo = CEQ_config["algo"]
    if algo in nr_channel_eq.LINEAR_ALGOS:
        return nr_channel_eq.channel_equ_and_demod(Y, H, cov, modtype, CEQ_config)
    assert algo in _lib.ML_ALGO, f"channel equalisation algo {algo!r}: one of {', '.join(ALGOS)}"
    return detect(Y, H, cov, modtype, algo)
