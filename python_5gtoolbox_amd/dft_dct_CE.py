"""Drop-in for py5gphy/channel_estimate/dft_dct_CE.py: DFT / DCT channel estimation of one slot on
the GPU (ldpc5g_channel_estimate, float64 arithmetic).  phy.channel_estimate takes T slots per
call and keeps the result on the device for phy.equalize / phy.ml_detect; this exists for callers
that keep the reference's per-slot call.

    DFT_DCT_channel_estimate(H_LS (S, N, Nr, Nt), RS_info, CE_config, model "DFT" | "DCT")
        -> (H_result (14, N*D, Nr, Nt) complex64, extended_cov_m (14, PRB, Nr, Nr) complex64)

CE_config["freq_intp_method"] "CubicSpline" / "PchipInterpolator" raise NotImplementedError.
"""
from . import _ce_dropin


def DFT_DCT_channel_estimate(H_LS, RS_info, CE_config, model):
    """dft_dct_CE.py:10-102"""
    return _ce_dropin.estimate(H_LS, RS_info, CE_config, "DFT" if model == "DFT" else "DCT")
