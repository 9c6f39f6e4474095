"""Batched polar codec on device tensors (TS 38.212 §5.3.1 / §5.4.1).

    p = polar.plan(K, E, nMax, iIL, CRCLEN=24, padCRC=0, rnti=0)    # host-built, cached, uploaded once per device
    d = polar.encode(bits, p)                 # [B, K] int8 -> [B, N] int8
    f = polar.rate_match(d, p, iBIL)          # [B, N] -> [B, E]
    y = polar.rate_recover(llr, p, iBIL)      # [B, E] float64 -> [B, N]
    ck, status, pm = polar.decode(y, p, "SCL", L)

K counts the CRC bits.  There is no CPU path: the kernels of libldpc5g.so do the work.
"""
import ctypes
import functools

import numpy as np

from . import _lib

SC, SCL = 0, 1
ALGOS = {"SC": SC, "SC_optionB": SC, "SCL": SCL, "SCL_optionB": SCL}   # the optionB recursions compute the same values
_FIELDS = ("magic", "version", "bytes", "K", "E", "nMax", "iIL", "CRCLEN", "padCRC", "rnti", "N", "n", "nPC", "nPCwm",
           "qPC0", "qPC1", "qPC2", "mode")
MODES = ("repetition", "puncturing", "shortening")


class Plan:
    """Host copy of a ldpc5g_polar_plan blob plus one device copy per device."""

    def __init__(self, blob):
        self.blob = blob                                   # numpy uint8, owns the host bytes
        hdr = blob[:80].view(np.int32)
        for i, n in enumerate(_FIELDS):
            setattr(self, n, int(hdr[i]))
        self.qPC = np.array([self.qPC0, self.qPC1, self.qPC2][:self.nPC], np.int16)
        off_F = int(hdr[19])
        self.F = blob[off_F:off_F + self.N].view(np.int8).copy()
        self.mode_name = MODES[self.mode]
        self._dev = {}

    @property
    def host(self):
        return ctypes.c_void_p(self.blob.ctypes.data)

    def dev(self, device):
        t = _lib.torch()
        key = t.device(device).index if t.device(device).index is not None else t.cuda.current_device()
        d = self._dev.get(key)
        if d is None:
            d = self._dev[key] = t.from_numpy(self.blob).to(f"cuda:{key}")
        return d


def plan_blob(K, E, nMax, iIL, CRCLEN=24, padCRC=0, rnti=0):
    """The plan's bytes (numpy uint8); AssertionError with the library's message for refused arguments."""
    args = dict(K=int(K), E=int(E), nMax=int(nMax), iIL=int(iIL), crclen=int(CRCLEN), padCRC=int(padCRC), rnti=int(rnti))
    n = _lib.call("ldpc5g_polar_plan", **args, plan=None, plan_bytes=0)
    blob = np.zeros(int(n), np.uint8)
    _lib.call("ldpc5g_polar_plan", **args, plan=blob, plan_bytes=int(n))
    return blob


@functools.lru_cache(maxsize=512)
def plan(K, E, nMax, iIL, CRCLEN=24, padCRC=0, rnti=0):
    return Plan(plan_blob(K, E, nMax, iIL, CRCLEN, padCRC, rnti))


def _rows(x, width, dtype, name):
    t = _lib.require_gpu()
    assert x.is_cuda and x.dtype == dtype, f"{name}: a cuda {dtype} tensor"
    if x.dim() == 1:
        x = x[None]
    assert x.dim() == 2 and x.shape[1] == width, f"{name}: [B, {width}], got {tuple(x.shape)}"
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < width):
        x = x.contiguous()
    return t, x, (x.stride(0) if x.shape[0] > 1 else width)


def encode(bits, p):
    t, bits, ld = _rows(bits, p.K, _lib.torch().int8, "bits")
    out = t.empty((bits.shape[0], p.N), dtype=t.int8, device=bits.device)
    _lib.call("ldpc5g_polar_encode", bits.device, plan_dev=p.dev(bits.device), plan_host=p.host, bits=bits, ldb=ld,
              out=out, ldo=p.N, B=bits.shape[0])
    return out


def rate_match(d, p, iBIL):
    t, d, ld = _rows(d, p.N, _lib.torch().int8, "d")
    out = t.empty((d.shape[0], p.E), dtype=t.int8, device=d.device)
    _lib.call("ldpc5g_polar_rate_match", d.device, plan_dev=p.dev(d.device), plan_host=p.host, d=d, ldi=ld, f=out,
              ldo=p.E, B=d.shape[0], iBIL=int(iBIL))
    return out


def rate_recover(llr, p, iBIL, LLR_limit=20.0, reference_repetition=False):
    """reference_repetition=True sums the repetitions of an iBIL = 1 block without de-interleaving
    them, as nr_polar_raterecover.py:40 does; the default de-interleaves."""
    t, llr, ld = _rows(llr, p.E, _lib.torch().float64, "llr")
    out = t.empty((llr.shape[0], p.N), dtype=t.float64, device=llr.device)
    _lib.call("ldpc5g_polar_rate_recover", llr.device, plan_dev=p.dev(llr.device), plan_host=p.host, llr=llr, ldi=ld,
              out=out, ldo=p.N, B=llr.shape[0], iBIL=int(iBIL), llr_limit=float(LLR_limit),
              reference_repetition=int(bool(reference_repetition)))
    return out


def decode(llr, p, algo="SCL", L=8):
    """-> (ck [B, K] int8, status [B] uint8, pm [B] float64).  A failed block has status 0, a row of
    -1 and pm = +inf."""
    assert algo in ALGOS, f"algo {algo!r}: one of {sorted(ALGOS)}"
    t, llr, ld = _rows(llr, p.N, _lib.torch().float64, "llr")
    B = llr.shape[0]
    ck = t.empty((B, p.K), dtype=t.int8, device=llr.device)
    status = t.empty(B, dtype=t.uint8, device=llr.device)
    pm = t.empty(B, dtype=t.float64, device=llr.device)
    _lib.call("ldpc5g_polar_decode", llr.device, plan_dev=p.dev(llr.device), plan_host=p.host, llr=llr, ldl=ld, ck=ck,
              ldc=p.K, status=status, pm=pm, B=B, algo=ALGOS[algo], L=int(L))
    return ck, status, pm


def polar_tx(bits, p, E=None, iBIL=0):
    assert E is None or E == p.E
    return rate_match(encode(bits, p), p, iBIL)


def polar_rx(llr, p, E=None, iBIL=0, algo="SCL", L=8, LLR_limit=20.0, reference_repetition=False):
    assert E is None or E == p.E
    return decode(rate_recover(llr, p, iBIL, LLR_limit, reference_repetition), p, algo, L)
