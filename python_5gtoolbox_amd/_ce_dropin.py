"""Shared body of the channel-estimation drop-ins (dft_dct_CE.py, dft_dct_symmetric_CE.py,
nr_channel_estimation.py): one slot through phy.channel_estimate, results as the reference returns
them (numpy complex64)."""
import numpy as np

from . import _lib, phy

SPLINES = ("CubicSpline", "PchipInterpolator")


def check_config(CE_config, freq_offset=None):
    """The reference's options that are not provided are refused by name, before any GPU work."""
    if CE_config.get("enable_FO_est") or CE_config.get("enable_FO_comp"):
        raise NotImplementedError(
            "enable_FO_est / enable_FO_comp: frequency-offset estimation and compensation "
            "(nr_channel_estimation.py:224-327) are not implemented")
    if freq_offset is not None:
        raise NotImplementedError(
            f"freq_offset={freq_offset!r}: frequency-offset compensation "
            "(nr_channel_estimation.py:268-327) is not implemented")
    method = CE_config.get("freq_intp_method")
    if method in SPLINES:   # any other name is np.interp in the reference too (dft_dct_CE.py:153-155)
        raise NotImplementedError(
            f"freq_intp_method {method!r}: only the linear frequency interpolation "
            "(np.interp, dft_dct_CE.py:145-155) is implemented")


def estimate(H_LS, RS_info, CE_config, algo, to_comp=False, want=()):
    """(H_result (14, N*D, Nr, Nt) complex64, cov_m (14, PRB, Nr, Nr) complex64[, extras as numpy])"""
    check_config(CE_config)
    H = np.asarray(H_LS)
    assert H.ndim == 4
    assert (H.shape[1] * RS_info["RE_distance"] // 12) != 1, "one-PRB assignments are not supported"
    t = _lib.require_gpu()
    d = t.from_numpy(np.ascontiguousarray(H, dtype=np.complex64)[None]).cuda()
    res = phy.channel_estimate(
        d, RS_info["RSSymMap"], algo, RS_info["scs"], CE_config["eRB"], CE_config["L_symm_left_in_ns"],
        CE_config["L_symm_right_in_ns"], re_distance=RS_info["RE_distance"],
        num_cdm_groups=RS_info["NumCDMGroupsWithoutData"], to_comp=to_comp, want=want)
    S, N, Nr, Nt = H.shape
    D = RS_info["RE_distance"]
    h = res[0][0].cpu().numpy().reshape(14, N * D, Nr, Nt)
    cov = res[1][0].cpu().numpy().reshape(14, N * D // 12, Nr, Nr)
    if want:
        return h, cov, {k: v[0].cpu().numpy() for k, v in res[2].items()}
    return h, cov
