"""Drop-in for the receive side of py5gphy/nr_pusch/nr_pusch_dmrs.py: the DMRS least-squares
estimate of one slot on the GPU (ldpc5g_slot_rx_frontend, float64 arithmetic), transform precoding
disabled — with nTransPrecode != 0 pusch_dmrs_LS_est raises NotImplementedError, and
pusch_dmrs_LS_est_tp (ldpc5g_slot_rx_frontend_tp, the low-PAPR sequence) takes that case.

    pusch_dmrs_LS_est(fd_slot_data (Nr, 14*carrier_RE_size), pusch_config, slot)
        -> (H_LS (S, 3*RBSize, Nr, num_of_layers) complex64, RS_info with "precoding_matrix")
    pusch_dmrs_LS_est_tp(fd_slot_data, pusch_config, slot, base_seq=None) -> the same, nTransPrecode = 1
    get_DMRS_symlist(Ld, DMRSAddPos) -> list
"""
import numpy as np

from . import _slot_dropin, nr_pusch_precoding, phy


def pusch_dmrs_LS_est(fd_slot_data, pusch_config, slot):
    """nr_pusch_dmrs.py:107-200"""
    H_LS, RS_info = _slot_dropin.ls_est(fd_slot_data, pusch_config, slot, "nr_pusch")
    RS_info["precoding_matrix"] = nr_pusch_precoding.get_precoding_matrix(
        pusch_config["num_of_layers"], pusch_config["nNrOfAntennaPorts"], pusch_config["nPMI"])
    return H_LS, RS_info


def pusch_dmrs_LS_est_tp(fd_slot_data, pusch_config, slot, base_seq=None):
    """nr_pusch_dmrs.py:107-200 with nTransPrecode = 1 (:171-172, 216-249).  base_seq: the DMRS
    base sequences (S, 6*RBSize) complex128 instead of the generated ones, needed for RBSize <= 4."""
    p = phy._tp_params(pusch_config, base_seq)   # the reference's asserts and refusals come first
    grid, slots = _slot_dropin._device_grid(fd_slot_data, slot)
    (h_ls,) = phy.pusch_tp_frontend(grid, slots, pusch_config, want=("h_ls",), base_seq=base_seq)
    RS_info = {"type": "nr_pusch", "RSSymMap": p["symlist"], "PortIndexList": list(pusch_config["PortIndexList"])[:1],
               "RE_distance": 4, "NumCDMGroupsWithoutData": p["cdm"],
               "precoding_matrix": nr_pusch_precoding.get_precoding_matrix(
                   1, pusch_config["nNrOfAntennaPorts"], pusch_config["nPMI"])}
    return h_ls[0].cpu().numpy().astype(np.complex64, copy=False), RS_info


def get_DMRS_symlist(Ld, DMRSAddPos):
    """nr_pusch_dmrs.py:251-286"""
    return phy.dmrs_symlist(Ld, DMRSAddPos, "pusch")
