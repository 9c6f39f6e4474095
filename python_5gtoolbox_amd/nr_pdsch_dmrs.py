"""Drop-in for the receive side of py5gphy/nr_pdsch/nr_pdsch_dmrs.py: the DMRS least-squares
estimate of one slot on the GPU (ldpc5g_slot_rx_frontend, float64 arithmetic).
phy.slot_frontend takes T slots per call and keeps H_LS on the device for phy.channel_estimate;
this exists for callers that keep the reference's per-slot call.

    pdsch_dmrs_LS_est(fd_slot_data (Nr, 14*carrier_RE_size), pdsch_config, slot)
        -> (H_LS (S, 3*RBSize, Nr, num_of_layers) complex64, RS_info)
    get_DMRS_symlist(Ld, DMRSAddPos) -> list
"""
from . import _slot_dropin, phy


def pdsch_dmrs_LS_est(fd_slot_data, pdsch_config, slot):
    """nr_pdsch_dmrs.py:139-227"""
    return _slot_dropin.ls_est(fd_slot_data, pdsch_config, slot, "nr_pdsch")


def get_DMRS_symlist(Ld, DMRSAddPos):
    """nr_pdsch_dmrs.py:258-297"""
    return phy.dmrs_symlist(Ld, DMRSAddPos, "pdsch")
