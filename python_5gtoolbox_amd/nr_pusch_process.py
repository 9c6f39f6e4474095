"""Drop-in for py5gphy/nr_pusch/nr_pusch_process.py (38.211 6.3.1) on the GPU: scrambling,
modulation, layer mapping, transform precoding (ldpc5g_transform_precode, float64 arithmetic) and
precoding of one slot's g_seq.

    nr_pusch_process(g_seq, rnti, nID, Qm, num_of_layers, nTransPrecode, RBSize, nNrOfAntennaPorts,
                     precoding_matrix) -> (nNrOfAntennaPorts, G / Qm / num_of_layers) complex64

A g_seq holding the UCI placeholders -1 / -2 is refused here (UCI on PUSCH is not provided by this
drop-in): uci.scramble_modulate is the batched entry point that applies the placeholder rules.
"""
import numpy as np

from . import _lib, phy


def nr_pusch_process(g_seq, rnti, nID, Qm, num_of_layers, nTransPrecode, RBSize, nNrOfAntennaPorts, precoding_matrix):
    """nr_pusch_process.py:9-60"""
    g = np.asarray(g_seq)
    assert g.ndim == 1
    if (g < 0).any():
        raise NotImplementedError("g_seq holds UCI placeholder bits (-1 / -2): UCI on PUSCH is not provided by this "
                                  "drop-in; uci.scramble_modulate scrambles and maps a g_seq with placeholders")
    assert Qm in [1, 2, 4, 6, 8]
    assert nTransPrecode in [0, 1]
    NL = int(num_of_layers)
    assert (g.size // Qm) % NL == 0
    if nTransPrecode:
        assert NL == 1
        phy._tp_check_rb(RBSize)
        assert (g.size // Qm) % (RBSize * 12) == 0
    t = _lib.require_gpu()
    bits = t.from_numpy(np.ascontiguousarray(g, dtype=np.int8)[None]).cuda()
    cinit = t.tensor([int(rnti) * 2 ** 15 + int(nID)], dtype=t.int32, device="cuda")
    sym = phy.scramble_modulate(bits, -1 if Qm == 1 else Qm, cinit)   # Qm 1 is pi/2-BPSK here (:29)
    if nTransPrecode:
        sym = phy.transform_precode(sym, RBSize)
    yi = sym[0].cpu().numpy().reshape(-1, NL).T   # layer mapping (:33-37)
    W = np.asarray(precoding_matrix)
    W = W.reshape(nNrOfAntennaPorts, NL) if W.ndim < 2 else W
    return (W @ yi).astype(np.complex64)
