"""Small-block encoding (TS 38.212 §5.3.3) — drop-in for py5gphy/smallblock/nr_smallblock_encoder.py:54-86.

One block per call around `ldpc5g_smallblock_encode` (uci.smallblock_encode is the batched form)."""
import numpy as np

from . import _lib, uci


def encode_smallblock(inbits, Qm=2):
    """-> N bits (Qm, 3 Qm or 32), placeholders (x, y) as (-1, -2)."""
    inbits = np.asarray(inbits)
    K = inbits.size
    assert K < 12
    assert Qm in [1, 2, 4, 6, 8]
    assert K >= 1
    t = _lib.require_gpu()
    bits = t.from_numpy(np.ascontiguousarray(inbits.reshape(1, K) & 1, dtype=np.int8)).cuda()
    return uci.smallblock_encode(bits, uci.sb_N(K, Qm), Qm)[0].cpu().numpy()
