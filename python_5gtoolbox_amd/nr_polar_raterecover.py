"""Polar rate recovery (TS 38.212 §5.4.1) — drop-in for py5gphy/polar/nr_polar_raterecover.py:6-63.

One block per call around `ldpc5g_polar_rate_recover`.  Like the reference (:40), repetition with
iBIL = 1 sums the LLRs that were NOT de-interleaved; polar.rate_recover de-interleaves unless asked
for reference_repetition=True."""
import numpy as np

from . import _lib, _polar_dropin as D, polar


def ratemrecover_polar(LLRin, K, N, iBIL, LLR_limit=20):
    LLRin = np.asarray(LLRin, np.float64)
    E = LLRin.size
    assert E <= 8192
    if iBIL:
        assert not ((K > 25) and (K <= 30))
        assert K > 18
    p = D.plan_for_N(K, E, N)
    out = polar.rate_recover(D.dev(LLRin, np.float64, "polar_rr"), p, 1 if iBIL else 0, float(LLR_limit),
                             reference_repetition=True)
    return _lib.to_host(out, "polar_rr")[0]
