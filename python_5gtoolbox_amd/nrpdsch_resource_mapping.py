"""Drop-in for the receive side of py5gphy/nr_pdsch/nrpdsch_resource_mapping.py: the allocation's
resource elements of one slot, gathered on the GPU (ldpc5g_slot_rx_frontend).  phy.slot_frontend
takes T slots per call and keeps y on the device for phy.equalize / phy.ml_detect; this exists for
callers that keep the reference's per-slot call.

    copy_Rx_pdsch_resource(rx_fd_slot_data (Nr, 14*carrier_RE_size), pdsch_config)
        -> (pdsch_resource (NrOfSymbols, 12*RBSize, Nr) complex64, pdsch_RE_usage float64)
"""
from . import _slot_dropin


def copy_Rx_pdsch_resource(rx_fd_slot_data, pdsch_config):
    """nrpdsch_resource_mapping.py:87-129"""
    return _slot_dropin.copy_resource(rx_fd_slot_data, pdsch_config)
