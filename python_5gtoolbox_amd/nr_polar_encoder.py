"""Polar encoding (TS 38.212 §5.3.1) — drop-in for py5gphy/polar/nr_polar_encoder.py:9-64.

One block per call around `ldpc5g_polar_encode` (polar.encode is the batched form)."""
import numpy as np

from . import _lib, _polar_dropin as D, polar


def encode_polar(inbits, E, nMax, iIL):
    inbits = np.asarray(inbits)
    assert (not np.any(np.nonzero(inbits < 0))) and (not np.any(np.nonzero(inbits > 1)))
    assert [nMax, iIL] in [[9, 1], [10, 0]]
    K = inbits.size
    p = polar.plan(K, E, nMax, iIL, D.crclen_of(K, nMax))
    return _lib.to_host(polar.encode(D.dev(inbits, np.int8, "polar_enc"), p), "polar_enc")[0]
