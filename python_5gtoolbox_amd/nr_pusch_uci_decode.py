"""UL-SCH and UCI decoding of one PUSCH slot — drop-in for py5gphy/nr_pusch/nr_pusch_uci_decode.py:19-62.

Like the reference it separates the four streams (plain permutation, the HARQ-ACK-punctured LLRs left in the
UL-SCH stream) and decodes the UL-SCH only; sch.sch_uci_rx_batch is the batched receiver that also decodes
the UCI."""
import numpy as np

from . import nr_pusch_datactrl_multiplex, nr_pusch_dmrs, nr_ulsch_decode, nr_ulsch_info, ul_tbsize
from .sch import sch_config


def ULSCHandUCIDecodeProcess(LLr,pusch_config, rv, LDPC_decoder_config,HARQ_on=False,current_LLr_dns=np.array([])):
    LLr = np.asarray(LLr)
    Gtotal = LLr.size
    Ld = pusch_config['StartSymbolIndex'] + pusch_config['NrOfSymbols']
    DMRS_symlist = nr_pusch_dmrs.get_DMRS_symlist(Ld, pusch_config["DMRS"]["DMRSAddPos"])
    TBSize, Qm, coderateby1024 = ul_tbsize.gen_tbsize(pusch_config)
    EnableULSCH = pusch_config['EnableULSCH']
    ULSCH_size = 0
    if EnableULSCH == 1:   # codeblocks x their length with fillers, from the geometry alone
        g = sch_config(TBSize, 2, coderateby1024, 1, 0, 0, 2)   # Qm / NL / rv / G do not influence segmentation
        ULSCH_size = g.C * g.K
    RMinfo = nr_ulsch_info.getULSCH_RM_info(pusch_config, DMRS_symlist, ULSCH_size, Qm, coderateby1024, Gtotal)
    g_ulsch, g_ack, g_csi1, g_csi2 = nr_pusch_datactrl_multiplex.data_control_separate(LLr, pusch_config, DMRS_symlist,
                                                                                      RMinfo, Qm)
    if EnableULSCH == 1:
        return nr_ulsch_decode.ULSCH_decoding(g_ulsch, TBSize, coderateby1024, Qm, RMinfo['G_ULSCH'],
                                              pusch_config['num_of_layers'], rv, LDPC_decoder_config, HARQ_on, current_LLr_dns)
    return False, np.array([]), np.array([])
