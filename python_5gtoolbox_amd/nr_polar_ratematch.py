"""Polar rate matching (TS 38.212 §5.4.1) — drop-in for py5gphy/polar/nr_polar_ratematch.py:6-73.

One block per call around `ldpc5g_polar_rate_match` (polar.rate_match is the batched form)."""
import numpy as np

from . import _lib, _polar_dropin as D, polar


def ratematch_polar(inbits, K, E, iBIL):
    assert E <= 8192
    if iBIL:
        assert (K in range(18, 26)) or (K > 30)
    inbits = np.asarray(inbits)
    N = inbits.size
    assert N in [2 ** 5, 2 ** 6, 2 ** 7, 2 ** 8, 2 ** 9, 2 ** 10]
    p = D.plan_for_N(K, E, N)
    return _lib.to_host(polar.rate_match(D.dev(inbits, np.int8, "polar_rm"), p, 1 if iBIL else 0), "polar_rm")[0]
