"""Small-block rate recovery with hard decision (TS 38.212 §5.4.3) — drop-in for
py5gphy/smallblock/nr_smallblock_raterecover.py:4-35, on the host (the batched decoder folds the soft
repetitions inside its kernel: uci.smallblock_decode)."""
import numpy as np


def raterecover_smallblock(LLRin, N):
    LLRin = np.asarray(LLRin)
    dn = np.zeros(N, 'i1')
    E = LLRin.size
    if E <= N:
        dn[0:E] = LLRin < 0
        return dn
    out = np.zeros(N)
    off = 0
    while off + N <= E:      # whole copies first, then the remainder: the reference's order of additions
        out += LLRin[off:off + N]
        off += N
    if off < E:
        out[0:E - off] += LLRin[off:]
    dn[out < 0] = 1
    return dn
