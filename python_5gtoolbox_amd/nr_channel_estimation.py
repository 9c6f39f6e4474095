"""Drop-in for py5gphy/channel_estimate/nr_channel_estimation.py: the NrChannelEstimation class
with the timing-offset estimate and compensation and the four CE_algo values, one slot per call on
the GPU (ldpc5g_channel_estimate / ldpc5g_to_compensate, float64 arithmetic).

    ce = NrChannelEstimation(H_LS (S, N, Nr, Nt), RS_info, CE_config)
    H_result, cov_m = ce.channel_est()          # numpy complex64, as the reference
    pdsch_resource = ce.process_pdsch_data(pdsch_resource, pdsch_start_sym)   # timing offset only
    ce.TO_est, ce.H_result, ce.cov_m, ce.FO_status (False), ce.FO_est (0)

With CE_config["enable_TO_comp"] channel_est compensates the caller's H_LS IN PLACE, as the
reference's comp_H_LS_timing_offset does.  Frequency-offset estimation and compensation
(enable_FO_est, enable_FO_comp, a freq_offset argument) and the spline frequency interpolators
raise NotImplementedError.
"""
import numpy as np

from . import _ce_dropin, _lib, phy


class NrChannelEstimation():
    """nr_channel_estimation.py:10-221"""

    def __init__(self, H_LS, RS_info, CE_config):
        self.H_LS = H_LS
        self.RS_info = RS_info
        if "freq_intp_method" not in CE_config:
            CE_config["freq_intp_method"] = "linear"
        if "timing_intp_method" not in CE_config:
            CE_config["timing_intp_method"] = "linear"
        self.CE_config = CE_config
        self.freq_offset = None
        sym_num, RE_num, Nr, Nt = H_LS.shape
        assert sym_num == len(RS_info["RSSymMap"])
        assert RS_info["scs"] in [15, 30]
        _ce_dropin.check_config(CE_config)

    def _estimate(self, to_comp, want):
        algo = self.CE_config["CE_algo"]
        assert algo in _lib.CE_ALGO, algo
        return _ce_dropin.estimate(self.H_LS, self.RS_info, self.CE_config, algo, to_comp=to_comp, want=want)

    def channel_est(self, freq_offset=None):
        """nr_channel_estimation.py:85-131: timing-offset estimate, optional compensation of H_LS
        (in place) and the CE_algo estimator, in one call on the GPU."""
        _ce_dropin.check_config(self.CE_config, freq_offset)
        self.freq_offset = freq_offset
        to_comp = bool(self.CE_config["enable_TO_comp"])
        H_result, cov_m, extra = self._estimate(to_comp, ("to_est", "h_ls_comp") if to_comp else ("to_est",))
        self.TO_est = extra["to_est"]
        if to_comp:
            self.H_LS[...] = extra["h_ls_comp"]
        self.FO_status = False
        self.FO_est = 0
        self.H_result = H_result
        self.cov_m = cov_m
        return H_result, cov_m

    def timing_offset_est(self):
        """nr_channel_estimation.py:150-172: each RS symbol's timing offset in seconds."""
        _, _, extra = self._estimate(False, ("to_est",))
        self.TO_est = extra["to_est"]
        return self.TO_est

    def _compensate(self, a, step):
        """a (nsym, RE, K) times exp(-j 2 pi mean(TO_est) step k scs 1000), in place."""
        t = _lib.require_gpu()
        avg = t.tensor([float(np.mean(self.TO_est)) * step], dtype=t.float64, device="cuda")
        y = t.from_numpy(np.ascontiguousarray(a)[None]).cuda()
        phy.to_compensate(y, avg, self.RS_info["scs"], out=y)
        a[...] = y[0].cpu().numpy()
        return a

    def comp_H_LS_timing_offset(self):
        """nr_channel_estimation.py:174-207: compensates self.H_LS (the caller's array) in place."""
        sym_num, RE_num, Nr, Nt = self.H_LS.shape
        flat = np.ascontiguousarray(self.H_LS).reshape(sym_num, RE_num, Nr * Nt)
        self.H_LS[...] = self._compensate(flat, self.RS_info["RE_distance"]).reshape(self.H_LS.shape)

    def process_pdsch_data(self, pdsch_resource, pdsch_start_sym):
        """nr_channel_estimation.py:133-148, the timing offset only."""
        _ce_dropin.check_config(self.CE_config, self.freq_offset)
        if self.CE_config["enable_TO_comp"]:
            pdsch_resource = self._compensate(pdsch_resource, 1)
        return pdsch_resource
