"""Drop-in for py5gphy/channel_estimate/dft_dct_symmetric_CE.py: DFT / DCT channel estimation with
the symmetric extension, one slot on the GPU (ldpc5g_channel_estimate).  See dft_dct_CE.py here.

    DFT_DCT_symmetric_channel_estimate(H_LS (S, N, Nr, Nt), RS_info, CE_config, model "DFT" | "DCT")
        -> (H_result (14, N*D, Nr, Nt) complex64, extended_cov_m (14, PRB, Nr, Nr) complex64)
"""
from . import _ce_dropin


def DFT_DCT_symmetric_channel_estimate(H_LS, RS_info, CE_config, model):
    """dft_dct_symmetric_CE.py:11-118"""
    return _ce_dropin.estimate(H_LS, RS_info, CE_config,
                               "DFT_symmetric" if model == "DFT" else "DCT_symmetric")
