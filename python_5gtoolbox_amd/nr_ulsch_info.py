"""UCI rate-matching parameters (TS 38.212 §6.3.2.4) — drop-in for py5gphy/nr_pusch/nr_ulsch_info.py:6-170, on the
host through ldpc5g_uci_rm_info."""
from . import uci


def getULSCH_RM_info(pusch_config, DMRS_symlist, ULSCH_size, Qm, coderateby1024, Gtotal):
    return uci.rm_info(pusch_config, DMRS_symlist, ULSCH_size, Qm, coderateby1024, Gtotal)
