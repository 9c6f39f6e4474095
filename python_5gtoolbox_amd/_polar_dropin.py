"""Shared by the flat polar drop-ins (nr_polar_*.py, polar_construct.py): numpy in, numpy out, one block
per call through the batched kernels of polar.py, with the reference's asserts in front."""
import numpy as np

from . import _lib, polar

CONFIGS = ((9, 1, 24), (10, 0, 11), (10, 0, 6))


def crclen_of(K, nMax):
    return 24 if nMax == 9 else (6 if K <= 25 else 11)


def plan_for_N(K, E, N):
    """ratematch_polar / ratemrecover_polar are told N, not nMax: the plan of the first standard
    configuration that accepts (K, E) and gives that N (their steps depend on K, E and N only)."""
    last = None
    for nMax, iIL, crclen in CONFIGS:
        try:
            p = polar.plan(K, E, nMax, iIL, crclen)
        except AssertionError as e:
            last = e
            continue
        if p.N == N:
            return p
    raise AssertionError(f"no polar configuration with K={K}, E={E} has N={N}" + (f" ({last})" if last else ""))


def dev(a, dtype, key):
    return _lib.to_device(np.ascontiguousarray(np.asarray(a), dtype=dtype), key)
