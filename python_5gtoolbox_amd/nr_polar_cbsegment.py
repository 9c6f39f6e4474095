"""Polar code block segmentation and CRC attachment (TS 38.212 §5.2.1, §6.3.1.2.1) — drop-in for
py5gphy/polar/nr_polar_cbsegment.py:6-54, on the host with crc.py."""
import numpy as np

from . import crc


def polar_cbsegment(uciBits, Euci):
    """-> (C x (A' + L) int8 blocks with CRC, C, Er)."""
    uciBits = np.asarray(uciBits)
    A = uciBits.size
    assert (A >= 12) and (A <= 1706)
    if (A >= 1013) or ((A >= 360) and (Euci >= 1088)):
        assert (Euci % 2) == 0
        C, L, poly = 2, 11, '11'
        padded = np.concatenate((np.zeros(A % 2, 'i1'), uciBits.astype('i1')))   # one zero in front of an odd A
        cbs = padded.reshape(2, -1)
    else:
        C, cbs = 1, uciBits.astype('i1').reshape(1, -1)
        L, poly = (6, '6') if A <= 19 else (11, '11')
    out = np.zeros((C, cbs.shape[1] + L), 'i1')
    for m in range(C):
        out[m, :] = crc.nr_crc_encode(cbs[m], poly, 0)
    return out, C, Euci // C
