"""Polar input interleaver (TS 38.212 §5.3.1.1) — drop-in for py5gphy/polar/polar_interleaver.py:21-56,
on the host from Table 5.3.1.1-1 (data/nr_polar_tables.json); the batched encoder interleaves in its
kernel from the plan."""
import json
import os

import numpy as np

_T = []


def _pi_il_max():
    if not _T:
        here = os.path.dirname(os.path.abspath(__file__))
        with open(os.path.join(here, "data", "nr_polar_tables.json")) as f:
            _T.append(json.load(f)["interleaver_5_3_1_1_1"])
    return _T[0]


def get_pattern_table(K):
    kilmax = 164
    assert K <= kilmax
    return [v - (kilmax - K) for v in _pi_il_max() if v >= kilmax - K]


def gen_deinterleave_table(K):
    pitable = get_pattern_table(K)
    depitable = [0] * K
    for m, v in enumerate(pitable):
        depitable[v] = m
    return depitable


def interleave(inbits, K):
    return np.asarray(inbits)[get_pattern_table(K)]


def deinterleave(ck_itrl, K):
    return np.asarray(ck_itrl)[gen_deinterleave_table(K)]
