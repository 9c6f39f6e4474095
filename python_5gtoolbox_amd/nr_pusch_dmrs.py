"""Drop-in for the receive side of py5gphy/nr_pusch/nr_pusch_dmrs.py: the DMRS least-squares
estimate of one slot on the GPU (ldpc5g_slot_rx_frontend, float64 arithmetic), transform precoding
disabled.  nTransPrecode != 0 raises NotImplementedError.

    pusch_dmrs_LS_est(fd_slot_data (Nr, 14*carrier_RE_size), pusch_config, slot)
        -> (H_LS (S, 3*RBSize, Nr, num_of_layers) complex64, RS_info with "precoding_matrix")
    get_DMRS_symlist(Ld, DMRSAddPos) -> list
"""
from . import _slot_dropin, nr_pusch_precoding, phy


def pusch_dmrs_LS_est(fd_slot_data, pusch_config, slot):
    """nr_pusch_dmrs.py:107-200"""
    H_LS, RS_info = _slot_dropin.ls_est(fd_slot_data, pusch_config, slot, "nr_pusch")
    RS_info["precoding_matrix"] = nr_pusch_precoding.get_precoding_matrix(
        pusch_config["num_of_layers"], pusch_config["nNrOfAntennaPorts"], pusch_config["nPMI"])
    return H_LS, RS_info


def get_DMRS_symlist(Ld, DMRSAddPos):
    """nr_pusch_dmrs.py:251-286"""
    return phy.dmrs_symlist(Ld, DMRSAddPos, "pusch")
