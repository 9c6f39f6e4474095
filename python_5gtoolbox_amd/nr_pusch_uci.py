"""UL-SCH and UCI bit processing of one PUSCH slot (TS 38.212 §6.2, §6.3.1.2 - §6.3.1.6) — drop-in for
py5gphy/nr_pusch/nr_pusch_uci.py:16-107: encode_uci_on_ulsch around uci.encode (small-block kernel up to 11
bits, CRC + polar codec above) and ULSCHandUCIProcess around the UL-SCH drop-ins, the rate-matching
arithmetic and the multiplexer.  sch.sch_uci_tx_batch is the batched form."""
import numpy as np

from . import _lib, nr_pusch_datactrl_multiplex, nr_ulsch, nr_ulsch_info, uci, ul_tbsize


def encode_uci_on_ulsch(UCIbits, NumUCIBits, Etot, Qm):
    t = _lib.require_gpu()
    A = NumUCIBits
    bits = np.ascontiguousarray(np.asarray(UCIbits).reshape(1, -1), dtype=np.int8)
    assert bits.shape[1] == A
    return uci.encode(t.from_numpy(bits).cuda(), Etot, Qm)[0].cpu().numpy()


def ULSCHandUCIProcess(pusch_config, trblk, Gtotal, rv, DMRS_symlist):
    TBSize, Qm, coderateby1024 = ul_tbsize.gen_tbsize(pusch_config)
    EnableULSCH = pusch_config['EnableULSCH']
    ULSCH_size = 0
    if EnableULSCH == 1:
        cbs, Zc, bgn = nr_ulsch.ULSCH_Crc_CodeBlockSegment(trblk, TBSize, coderateby1024)
        ULSCH_size = cbs.shape[0] * cbs.shape[1]
    RMinfo = nr_ulsch_info.getULSCH_RM_info(pusch_config, DMRS_symlist, ULSCH_size, Qm, coderateby1024, Gtotal)
    g_ulsch = np.array([])
    if EnableULSCH == 1:
        g_ulsch = nr_ulsch.ULSCH_encoding_ratematch(cbs, Zc, bgn, Qm, RMinfo['G_ULSCH'], pusch_config['num_of_layers'], rv)
    g = {}
    for name, key, E in (("ack", "ACK", 'Euci_ack'), ("csi1", "CSI1", 'Euci_CSI1'), ("csi2", "CSI2", 'Euci_CSI2')):
        n = pusch_config['Num' + key + 'Bits']
        if pusch_config['Enable' + key] * n > 0:
            bits = pusch_config[key + 'bits']
            assert n == len(bits)
            g[name] = encode_uci_on_ulsch(bits, n, RMinfo[E], Qm)
        else:
            g[name] = np.array([])
    return nr_pusch_datactrl_multiplex.data_control_multiplex(g_ulsch, g["ack"], g["csi1"], g["csi2"], pusch_config, Gtotal,
                                                              DMRS_symlist, RMinfo, Qm)
