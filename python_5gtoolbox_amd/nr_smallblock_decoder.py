"""Small-block decoding (TS 38.212 §5.3.3) — drop-in for py5gphy/smallblock/nr_smallblock_decoder.py:54-101.

The hard bits are mapped to +-1 LLRs (placeholders to 0) and decided by `ldpc5g_smallblock_decode`.  The
reference searches for the codeword EQUAL to dn and leaves `ck` unbound when there is none; this returns the
nearest codeword instead (ties to the smallest message), which is the same answer whenever the reference has one."""
import numpy as np

from . import _lib, uci


def decode_smallblock(dn, K, Qm=2):
    dn = np.asarray(dn)
    N = dn.size
    assert K < 12
    assert Qm in [1, 2, 4, 6, 8]
    if K == 1:
        assert N == Qm
    elif K == 2:
        assert N == 3 * Qm
    else:
        assert N == 32
    if K <= 2:
        return dn[0:K].astype('i1')   # nr_smallblock_decoder.py:75-78: the systematic bits as they are
    t = _lib.require_gpu()
    llr = np.where(dn == 1, -1.0, np.where(dn == 0, 1.0, 0.0)).reshape(1, N)
    return uci.smallblock_decode(t.from_numpy(llr).cuda(), K, Qm)[0].cpu().numpy()
