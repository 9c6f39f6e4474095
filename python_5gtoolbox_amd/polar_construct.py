"""Polar code construction (TS 38.212 §5.3.1.2, §5.4.1.1) — drop-in for
py5gphy/polar/polar_construct.py:10-137, answered from the host-built plan (`ldpc5g_polar_plan`)."""
import numpy as np

from . import _polar_dropin as D, polar


def construct(K, E, nMax):
    """-> F (int8, 1 = frozen), qPC (int16), N, nPC, nPCwm."""
    assert nMax in [9, 10]
    if nMax == 10:
        assert (K in range(18, 26)) or (K > 30)
    p = polar.plan(K, E, nMax, 1 if nMax == 9 else 0, D.crclen_of(K, nMax))
    return p.F.copy(), np.array(p.qPC, 'i2'), p.N, p.nPC, p.nPCwm
