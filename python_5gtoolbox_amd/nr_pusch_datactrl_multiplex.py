"""Data and control multiplexing (TS 38.212 §6.2.7) — drop-in for
py5gphy/nr_pusch/nr_pusch_datactrl_multiplex.py:7-539: the map is built once per configuration in time linear
in Gtotal (ldpc5g_uci_map_plan, cached) and applied on the GPU (uci.mux / uci.demux in plain mode)."""
import numpy as np

from . import _lib, uci


def _dev(x, dtype):
    t = _lib.require_gpu()
    return t.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(1, -1), dtype=dtype)).cuda()


def data_control_multiplex(g_ulsch, g_ack, g_csi1, g_csi2, pusch_config, Gtotal,
        DMRS_symlist,RMinfo, Qm):
    p = uci.plan(pusch_config, DMRS_symlist, RMinfo, Qm, Gtotal)
    ins = []
    for n, g in zip(uci.STREAMS, (g_ulsch, g_ack, g_csi1, g_csi2)):
        assert len(g) >= p.lens[n] if p.lens[n] else True, f"g_{n}: {p.lens[n]} bits expected"
        ins.append(_dev(g, np.int8) if p.lens[n] else None)
    return uci.mux(p, *ins)[0].cpu().numpy()


def data_control_separate(LLr, pusch_config,
        DMRS_symlist,RMinfo, Qm):
    LLr = np.asarray(LLr, np.float64)
    p = uci.plan(pusch_config, DMRS_symlist, RMinfo, Qm, LLr.size)
    s = uci.demux(p, _dev(LLr, np.float64), erase_punctured=False)
    g_ulsch, g_ack, g_csi1, g_csi2 = (x[0].cpu().numpy() for x in s)
    return g_ulsch, g_ack, g_csi1, g_csi2 if p.lens["csi2"] else []   # the reference's empty g_csi2 is a list
