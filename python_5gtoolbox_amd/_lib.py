"""ctypes binding of libldpc5g.so (include/ldpc5g.h) plus device-buffer helpers.

PyTorch-ROCm is used only for device memory and the current HIP stream; no torch ops run on
the hot path.  There is no CPU fallback: if the library or a GPU is missing, calls raise.
"""
import collections
import ctypes
import os
import re
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LDPC5G_LIB") or os.path.join(HERE, "libldpc5g.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "ldpc5g.h")

F64, F32 = 0, 1
FLOODING, LAYERED = 0, 1
LLR_FULL = 1
RATE_MATCHED = 2   # LDPC5G_RATE_MATCHED: rate-recovered rows, untransmitted columns +0.0
ALGO_MS, ALGO_BP, ALGO_BF = 0, 1, 2
EBGN, EZC, ESIZE, EHIP = -1, -2, -3, -4
EQ_ALGO = {"ZF": 0, "ZF-IRC": 1, "MMSE": 2, "MMSE-IRC": 3}   # LDPC5G_EQ_*: nr_channel_eq.py:15-26
# nr_channel_eq.py:27-46 names -> (LDPC5G_ML_* algo, irc)
ML_ALGO = {"ML-soft": (0, 0), "ML-IRC-soft": (0, 1), "ML-hard": (1, 0), "ML-IRC-hard": (1, 1),
           "ML2-soft": (2, 0), "ML2-IRC-soft": (2, 1), "MMSE-ML": (3, 0), "MMSE-ML-IRC": (3, 1),
           "opt-rank2-ML": (4, 0), "opt-rank2-ML-IRC": (4, 1)}
# CE_config["CE_algo"] (nr_channel_estimation.py:117-124) -> LDPC5G_CE_*
CE_ALGO = {"DFT": 0, "DCT": 1, "DFT_symmetric": 2, "DCT_symmetric": 3}

OPTIONAL = {"ldpc5g_dec_blocks_per_cu", "ldpc5g_split_timeouts"}   # absent from older libraries

_RESTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}
_ARGTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "int": ctypes.c_int, "double": ctypes.c_double, "float": ctypes.c_float}


def _parse_header(path):
    """Every `ldpc5g_*` prototype of the header -> (SIGNATURES, PARAMS).  Any pointer parameter is a
    c_void_p (struct pointers included).  A prototype or a type outside the two tables above raises
    and names the line: nothing is guessed."""
    with open(path) as f:
        src = f.read()
    def blank(m):   # keep offsets, so line numbers stay true
        return re.sub(r"[^\n]", " ", m.group())
    src = re.sub(r"//[^\n]*", blank, re.sub(r"/\*.*?\*/", blank, src, flags=re.S))
    sigs, params = {}, {}
    for m in re.finditer(r"\b(int|int64_t|const\s+char\s*\*)\s*(ldpc5g_\w+)\s*\(([^()]*)\)\s*;", src):
        where = f"{path}:{src.count(chr(10), 0, m.start(2)) + 1}: {m.group(2)}"
        argtypes, names = [], []
        plist = m.group(3).strip()
        for p in ([] if plist == "void" else plist.split(",")):
            pm = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*", p)
            if not pm or not (pm.group(2) or pm.group(1) in _ARGTYPE):
                raise ImportError(f"{where}: parameter {p.strip()!r} has no ctypes mapping")
            argtypes.append(ctypes.c_void_p if pm.group(2) else _ARGTYPE[pm.group(1)])
            names.append(pm.group(3))
        sigs[m.group(2)] = (_RESTYPE[re.sub(r"\s+", " ", m.group(1)).replace(" *", "*")], argtypes)
        params[m.group(2)] = tuple(names)
    for m in re.finditer(r"\b(ldpc5g_\w+)\s*\(", src):
        if m.group(1) not in sigs:
            raise ImportError(f"{path}:{src.count(chr(10), 0, m.start()) + 1}: {m.group(1)}: "
                              "not a prototype `int | int64_t | const char* name(params);`")
    return sigs, params


# every function include/ldpc5g.h declares: name -> (restype, argtypes), name -> parameter names
SIGNATURES, PARAMS = _parse_header(HEADER)
# per function, resolved once: indices of the pointer parameters; whether `stream` comes last
_POINTERS = {n: tuple(i for i, a in enumerate(args) if a is ctypes.c_void_p)
             for n, (_, args) in SIGNATURES.items()}
_STREAMED = {n for n, p in PARAMS.items() if p[-1:] == ("stream",)}


class CbDesc(ctypes.Structure):
    """ldpc5g_cb_desc_t"""
    _fields_ = [("bgn", ctypes.c_int32), ("Zc", ctypes.c_int32),
                ("llr_off", ctypes.c_int64), ("ck_off", ctypes.c_int64)]


CRC_IDS = {"6": 0, "11": 1, "16": 2, "24A": 3, "24B": 4, "24C": 5}


class SchCfg(ctypes.Structure):
    """ldpc5g_sch_cfg_t"""
    _fields_ = [(n, ctypes.c_int32) for n in
                ("A", "B", "tb_crc_poly", "bgn", "C", "cbz", "Lcb", "F", "K", "K_apo", "Zc", "N",
                 "Ncb", "k0", "Qm", "NL", "rv", "E_lo", "E_hi", "c_switch")] + \
               [("G", ctypes.c_int64), ("E_total", ctypes.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class LdpcLibError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libldpc5g.so (raises LdpcLibError if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LdpcLibError(
                f"{LIB_PATH} is missing: build it with `python -m python_5gtoolbox_amd.build` "
                "(there is no CPU fallback for the LDPC hot path)")
        _lib = bind(ctypes.CDLL(LIB_PATH))
    return _lib


def bind(handle):
    """Set restype / argtypes of every declared function on a CDLL and return it."""
    for name, (res, args) in SIGNATURES.items():
        if name in OPTIONAL and not hasattr(handle, name):
            continue   # diagnostics absent from an older library (A/B builds)
        f = getattr(handle, name)
        f.restype = res
        f.argtypes = args
    return handle


def invoke(name, **kw):
    """Call the library function `name` with its arguments by the header's parameter names and
    return the raw result.  kw must hold exactly PARAMS[name]: anything else is a TypeError before
    the library is entered.  Pointer parameters take a torch tensor (data_ptr()), a numpy array
    (.ctypes.data), None, an int or a ctypes object (byref, array, c_void_p); the other parameters
    pass through unchanged."""
    return _invoke(name, kw)


def _address(a):
    """Address of a numpy array's first element.  a.ctypes.data builds an object per call (about
    1 us, a third of a whole drop-in call's marshalling); a ctypes view of the buffer costs a third
    of that, but exists only for writable, contiguous, non-empty arrays."""
    try:
        return ctypes.addressof(ctypes.c_char.from_buffer(a))
    except (TypeError, ValueError, BufferError):
        return a.ctypes.data


def _invoke(name, kw):
    names = PARAMS[name]
    try:
        args = [kw[n] for n in names]
    except KeyError:
        args = None
    if args is None or len(kw) != len(names):
        raise TypeError(f"{name}: missing {sorted(set(names) - set(kw))}, "
                        f"unexpected {sorted(set(kw) - set(names))}")
    for i in _POINTERS[name]:
        v = args[i]
        if v is not None and type(v) is not int:
            if isinstance(v, np.ndarray):
                args[i] = _address(v)
            else:
                p = getattr(v, "data_ptr", None)
                if p is not None:
                    args[i] = p()
    return getattr(lib(), name)(*args)


def call(name, device=None, **kw):
    """invoke() in the frame every wrapper repeats: under torch.cuda.device(device) when one is
    given, with the current stream of `device` for a trailing `stream` the caller left out, and
    with the result through check().  Returns None for an `int` status and the value of an
    `int64_t` size (negative: check() raises)."""
    if device is None:
        if "stream" not in kw and name in _STREAMED:
            kw["stream"] = torch().cuda.current_stream().cuda_stream
        rc = _invoke(name, kw)
    else:
        t = torch()
        with t.cuda.device(device):
            if "stream" not in kw and name in _STREAMED:
                kw["stream"] = t.cuda.current_stream(device).cuda_stream
            rc = _invoke(name, kw)
    res = SIGNATURES[name][0]
    if res is ctypes.c_int:
        return check(rc)
    if res is ctypes.c_int64 and rc < 0:
        check(rc)
    return rc


def row_stride(x, d, row):
    """Stride of dimension d of x for the ABI's ld* arguments; the stride of a size-1 dimension is
    arbitrary in torch (and unused by the library), so `row`, the dense value, stands in for it."""
    return x.stride(d) if x.shape[d] > 1 else row


def dtype_id(dt, llr=False):
    """LDPC5G_F32 / LDPC5G_F64 of a real or complex torch dtype; llr=True accepts only the real two."""
    t = torch()
    if dt == t.float32 or (dt == t.complex64 and not llr):
        return F32
    if dt == t.float64 or (dt == t.complex128 and not llr):
        return F64
    raise AssertionError("LLRs must be float32 or float64" if llr else
                         f"dtype {dt}: float32 / float64 or complex64 / complex128")


def check(rc):
    """Map a negative return code to the reference's error behaviour (AssertionError for
    argument errors, as its `assert` checks) or LdpcLibError for HIP failures."""
    if rc == 0:
        return
    msg = lib().ldpc5g_last_error().decode()
    if rc in (EBGN, EZC, ESIZE):
        raise AssertionError(msg)
    raise LdpcLibError(f"libldpc5g error {rc}: {msg}")


_torch = None


def torch():
    global _torch
    if _torch is None:
        import torch as t
        _torch = t
    return _torch


def require_gpu():
    t = torch()
    if not t.cuda.is_available():
        raise LdpcLibError("no ROCm GPU visible: the LDPC engine runs only on the GPU "
                           "(no CPU fallback)")
    return t


def stream_ptr(device=None):
    t = torch()
    return ctypes.c_void_p(t.cuda.current_stream(device).cuda_stream)


def ptr(tensor):
    return ctypes.c_void_p(tensor.data_ptr())


_tls = threading.local()
STAGING_MAX = int(os.environ.get("LDPC5G_STAGING_MAX", "32"))


def staging(key, make):
    """Per-thread cache of pinned-host / device buffers for the per-codeblock drop-ins (the
    reference's callers decode one codeblock per call, sim_ldpc_internal.py:51-58): a call then
    costs one pinned H2D copy, the launch and one D2H copy, with no allocation.  Bounded: at most
    STAGING_MAX entries per thread, least recently used evicted (a sweep over MCS / TBS / PRB
    configurations keeps only the recent ones; an evicted buffer is freed when its last user drops
    it — torch's allocators order the reuse after the stream work that used it)."""
    d = getattr(_tls, "bufs", None)
    if d is None:
        d = _tls.bufs = collections.OrderedDict()
    b = d.get(key)
    if b is None:
        b = d[key] = make()
        while len(d) > STAGING_MAX:
            d.popitem(last=False)
    else:
        d.move_to_end(key)
    return b


def staging_entries():
    """Number of cached staging entries of this thread."""
    return len(getattr(_tls, "bufs", ()))


def to_device(a, key):
    """numpy array -> device tensor through a per-thread cached pinned buffer (the drop-ins'
    host inputs; pageable copies measured milliseconds per call).  The device buffer is reused by
    the next call with the same key and shape: callers synchronise (to_host) before returning."""
    t = torch()
    a = np.ascontiguousarray(a)
    dev = t.cuda.current_device()
    tdt = t.from_numpy(a[:0] if a.ndim else a.reshape(1)[:0]).dtype

    def make():
        return (t.empty(a.shape, dtype=tdt, pin_memory=True), t.empty(a.shape, dtype=tdt, device=dev))
    hin, din = staging((key, "in", dev, a.shape, a.dtype.str), make)
    hin.numpy()[...] = a
    din.copy_(hin, non_blocking=True)
    return din


def to_host(x, key):
    """device tensor -> numpy copy through a per-thread cached pinned buffer; synchronises."""
    t = torch()
    dev = x.device.index if x.device.index is not None else t.cuda.current_device()
    hout = staging((key, "out", dev, tuple(x.shape), str(x.dtype)),
                   lambda: t.empty(tuple(x.shape), dtype=x.dtype, pin_memory=True))
    hout.copy_(x, non_blocking=True)
    t.cuda.current_stream().synchronize()
    return hout.numpy().copy()


def split_timeouts():
    """Codeblocks of the current device whose multi-workgroup float64 decode gave up waiting for
    its parts to be co-resident (status 0, iters -1; include/ldpc5g.h ldpc5g_split_timeouts)."""
    n = ctypes.c_uint32(0)
    call("ldpc5g_split_timeouts", count=ctypes.byref(n))
    return int(n.value)
