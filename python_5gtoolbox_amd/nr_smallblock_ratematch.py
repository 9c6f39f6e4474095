"""Small-block rate matching (TS 38.212 §5.4.3) — drop-in for py5gphy/smallblock/nr_smallblock_ratematch.py:4-23,
on the host (the batched encoder repeats to E inside its kernel: uci.smallblock_encode)."""
import numpy as np


def ratematch_smallblock(dn, E):
    dn = np.asarray(dn)
    N = dn.size
    if E <= N:
        return dn[0:E]
    return np.array(np.tile(dn, -(-E // N))[0:E], 'i1')
