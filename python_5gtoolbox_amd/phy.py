"""Batched GPU scrambling / modulation / soft demodulation — the C-ABI
entry points ldpc5g_prbs, ldpc5g_scramble_modulate, ldpc5g_demod_descramble (include/ldpc5g.h).

    prbs_words(cinit (T,), nbits) -> (T, ceil(nbits/32)) int32 packed c(n)   (nrPRBS.py:5-25)
    scramble_modulate(bits (T, G), mod, cinit=None) -> (T, G/Qm) complex64      (nr_pdsch_process.py:17-25)
    demod_descramble(sym (T, n), noise_var (T, n), mod, cinit=None) -> (T, n*Qm) float32 LLR
                                                      (nr_Demodulation.py:12-46, nr_pdsch.py:268-274)
    equalize(y (T, R, Nr), h (T, R, Nr, NL), cov (T, R/12, Nr, Nr), algo, re_idx=None)
        -> (sym (T, nre*NL), noise_var (T, nre*NL) float32)   (nr_channel_eq.py:12-26, ZF.py, MMSE.py)
    ml_detect(y, h, cov, mod, algo, re_idx=None, ...) -> (T, nre*NL*Qm) float64 LLR [, sym, noise_var, hardbits]
                                      (nr_channel_eq.py:27-46, ML.py, ML2.py, MMSE_ML.py, opt_rank2_ML.py)
mod: a MOD_ID value (the order Qm for QPSK..1024QAM, 1 BPSK, -1 pi/2-BPSK).
Device tensors in and out; asynchronous on the current stream.
"""
from . import _lib

# nrModulation.py:14 / nr_Demodulation.py:29 modulation names -> ABI modulation id
MOD_ID = {"pi/2-bpsk": -1, "bpsk": 1, "qpsk": 2, "16qam": 4, "64qam": 6, "256qam": 8, "1024qam": 10}
QM_OF = {k: abs(v) for k, v in MOD_ID.items()}   # bits per symbol


def bits_per_symbol(mod):
    return abs(int(mod))


def prbs_words(cinit, nbits, out=None):
    """Packed scrambling codes: bit k of word w of row t = gen_nrPRBS(cinit[t], ...)[32w + k]."""
    t = _lib.require_gpu()
    assert cinit.dim() == 1 and cinit.dtype in (t.int32, t.int64)
    c = cinit.to(t.int32).contiguous()
    T = c.shape[0]
    nw = (int(nbits) + 31) // 32
    w = out if out is not None else t.empty((T, max(nw, 1)), dtype=t.int32, device=c.device)
    with t.cuda.device(c.device):
        _lib.check(_lib.lib().ldpc5g_prbs(_lib.ptr(c), T, int(nbits), _lib.ptr(w), w.stride(0),
                                          _lib.stream_ptr(c.device)))
    return w


def scramble_modulate(bits, mod, cinit=None, words=None, out=None):
    """bits: (T, G) int8 0/1 device tensor; mod: MOD_ID value; cinit: (T,) device tensor or None
    (no scrambling); words: precomputed prbs_words (reused across calls) instead of cinit."""
    t = _lib.require_gpu()
    assert bits.dim() == 2 and bits.dtype == t.int8 and bits.stride(1) == 1
    T, G = bits.shape
    Qm = bits_per_symbol(mod)
    w = words if words is not None else (prbs_words(cinit, G) if cinit is not None else None)
    sym = out if out is not None else t.empty((T, G // Qm), dtype=t.complex64, device=bits.device)
    with t.cuda.device(bits.device):
        _lib.check(_lib.lib().ldpc5g_scramble_modulate(
            _lib.ptr(bits), bits.stride(0), _lib.ptr(w) if w is not None else None,
            w.stride(0) if w is not None else 0, T, G, int(mod), _lib.ptr(sym), sym.stride(0),
            _lib.stream_ptr(bits.device)))
    return sym


def equalize(y, h, cov, algo, re_idx=None, re_per_cov=12, out=None):
    """Linear MIMO equalisation of the data resource elements of T transport blocks
    (ldpc5g_equalize; ZF.py / MMSE.py through nr_channel_eq.py:12-26).  y: (T, R, Nr), h:
    (T, R, Nr, NL), cov: (T, ceil(R/re_per_cov), Nr, Nr) complex64 / complex128 device tensors of
    one dtype (rows may be padded: only stride(0) is free); algo: "ZF", "ZF-IRC", "MMSE" or
    "MMSE-IRC"; re_idx: (nre,) int32 ascending flat indices of the data REs, None for all R.
    Returns (sym (T, nre*NL) of the input dtype, noise_var (T, nre*NL) float32), or fills
    out=(sym, noise_var)."""
    t = _lib.require_gpu()
    assert algo in _lib.EQ_ALGO, f"algo {algo!r}: one of {sorted(_lib.EQ_ALGO)}"
    assert y.dim() == 3 and h.dim() == 4 and cov.dim() == 4
    assert y.dtype in (t.complex64, t.complex128) and h.dtype == y.dtype and cov.dtype == y.dtype
    T, R, Nr = y.shape
    NL = h.shape[3]
    ncov = (R + int(re_per_cov) - 1) // int(re_per_cov) if re_per_cov >= 1 else 0
    assert h.shape == (T, R, Nr, NL) and cov.shape[0] == T and cov.shape[1] >= ncov and cov.shape[2:] == (Nr, Nr)
    assert y[0].is_contiguous() and h[0].is_contiguous() and cov[0].is_contiguous(), \
        "only the transport-block stride is free"
    if re_idx is not None:
        assert re_idx.dim() == 1 and re_idx.dtype == t.int32 and re_idx.is_contiguous()
        assert re_idx.device == y.device
    nre = re_idx.shape[0] if re_idx is not None else R
    if out is not None:
        sym, nv = out
        assert sym.dtype == y.dtype and sym.shape == (T, nre * NL) and sym.stride(1) == 1
        assert nv.dtype == t.float32 and nv.shape == (T, nre * NL) and nv.stride(1) == 1
    else:
        sym = t.empty((T, nre * NL), dtype=y.dtype, device=y.device)
        nv = t.empty((T, nre * NL), dtype=t.float32, device=y.device)
    def ld(x, row):   # the stride of a size-1 dimension is arbitrary in torch (and unused here)
        return x.stride(0) if T > 1 else row
    with t.cuda.device(y.device):
        _lib.check(_lib.lib().ldpc5g_equalize(
            _lib.ptr(y), ld(y, R * Nr), _lib.ptr(h), ld(h, R * Nr * NL), _lib.ptr(cov),
            ld(cov, cov.shape[1] * Nr * Nr), _lib.F32 if y.dtype == t.complex64 else _lib.F64,
            _lib.ptr(re_idx) if re_idx is not None else None, R, nre, int(re_per_cov), T, Nr, NL,
            _lib.EQ_ALGO[algo], _lib.ptr(sym), ld(sym, nre * NL), _lib.ptr(nv), ld(nv, nre * NL),
            _lib.stream_ptr(y.device)))
    return sym, nv


def ml_detect(y, h, cov, mod, algo, re_idx=None, re_per_cov=12, cinit=None, words=None, llr_dtype=None,
              want=()):
    """Maximum-likelihood MIMO detection of the data resource elements of T transport blocks,
    straight to LLRs (ldpc5g_ml_detect; ML.py, ML2.py, MMSE_ML.py, opt_rank2_ML.py through
    nr_channel_eq.py:27-46).  y, h, cov, re_idx, re_per_cov as equalize; mod: MOD_ID value; algo:
    the reference's name, one of _lib.ML_ALGO ("ML-soft", "ML-IRC-soft", "ML-hard", "ML-IRC-hard",
    "ML2-soft", "ML2-IRC-soft", "MMSE-ML", "MMSE-ML-IRC", "opt-rank2-ML", "opt-rank2-ML-IRC");
    cinit (T,) or precomputed prbs `words`: descramble the LLRs; llr_dtype: torch.float64 (default,
    the reference's type) or torch.float32.  Returns llr (T, nre*NL*Qm) — positive means bit 0 —
    or, with want=("sym", "noise_var", "hardbits") in any selection, the tuple (llr, *wanted in
    that order): sym (T, nre*NL) complex64 decided points, noise_var (T, nre*NL) of llr's dtype
    (the minimum metric), hardbits (T, nre*NL*Qm) int8."""
    t = _lib.require_gpu()
    assert algo in _lib.ML_ALGO, f"algo {algo!r}: one of {sorted(_lib.ML_ALGO)}"
    assert all(w in ("sym", "noise_var", "hardbits") for w in want), want
    assert y.dim() == 3 and h.dim() == 4 and cov.dim() == 4
    assert y.dtype in (t.complex64, t.complex128) and h.dtype == y.dtype and cov.dtype == y.dtype
    T, R, Nr = y.shape
    NL = h.shape[3]
    Qm = bits_per_symbol(mod)
    ncov = (R + int(re_per_cov) - 1) // int(re_per_cov) if re_per_cov >= 1 else 0
    assert h.shape == (T, R, Nr, NL) and cov.shape[0] == T and cov.shape[1] >= ncov and cov.shape[2:] == (Nr, Nr)
    assert y[0].is_contiguous() and h[0].is_contiguous() and cov[0].is_contiguous(), \
        "only the transport-block stride is free"
    if re_idx is not None:
        assert re_idx.dim() == 1 and re_idx.dtype == t.int32 and re_idx.is_contiguous()
        assert re_idx.device == y.device
    nre = re_idx.shape[0] if re_idx is not None else R
    llr_dtype = llr_dtype or t.float64
    assert llr_dtype in (t.float32, t.float64)
    nbits = nre * NL * Qm
    w = words if words is not None else (prbs_words(cinit, nbits) if cinit is not None else None)
    llr = t.empty((T, nbits), dtype=llr_dtype, device=y.device)
    outs = {"sym": t.empty((T, nre * NL), dtype=t.complex64, device=y.device) if "sym" in want else None,
            "noise_var": t.empty((T, nre * NL), dtype=llr_dtype, device=y.device) if "noise_var" in want else None,
            "hardbits": t.empty((T, nbits), dtype=t.int8, device=y.device) if "hardbits" in want else None}
    def ld(x, row):   # the stride of a size-1 dimension is arbitrary in torch (and unused here)
        return x.stride(0) if T > 1 else row
    def opt(x):
        return _lib.ptr(x) if x is not None else None
    code, irc = _lib.ML_ALGO[algo]
    with t.cuda.device(y.device):
        _lib.check(_lib.lib().ldpc5g_ml_detect(
            _lib.ptr(y), ld(y, R * Nr), _lib.ptr(h), ld(h, R * Nr * NL), _lib.ptr(cov),
            ld(cov, cov.shape[1] * Nr * Nr), _lib.F32 if y.dtype == t.complex64 else _lib.F64,
            opt(re_idx), R, nre, int(re_per_cov), T, Nr, NL, int(mod), code, irc,
            opt(w), ld(w, (nbits + 31) // 32) if w is not None else 0, _lib.ptr(llr),
            _lib.F64 if llr_dtype == t.float64 else _lib.F32, nbits,
            opt(outs["sym"]), nre * NL, opt(outs["noise_var"]), nre * NL, opt(outs["hardbits"]), nbits,
            _lib.stream_ptr(y.device)))
    return (llr, *(outs[k] for k in want)) if want else llr


def demod_descramble(sym, noise_var, mod, cinit=None, words=None, out=None, llr_dtype=None):
    """sym: (T, n) complex64 / complex128 device tensor, noise_var: (T, n) float32; mod: MOD_ID
    value; cinit: (T,) or None (no descrambling), or precomputed prbs `words`.  Returns (T, n*Qm)
    LLRs, float32 (llr_dtype=torch.float64 only for BPSK on complex128, demod_bpsk.py:9)."""
    t = _lib.require_gpu()
    assert sym.dim() == 2 and sym.dtype in (t.complex64, t.complex128) and sym.stride(1) == 1
    T, n = sym.shape
    Qm = bits_per_symbol(mod)
    llr_dtype = llr_dtype or t.float32
    nv = noise_var if noise_var.dtype == t.float32 and noise_var.is_contiguous() else \
        noise_var.to(t.float32).contiguous()
    assert nv.shape == (T, n)
    w = words if words is not None else (prbs_words(cinit, n * Qm) if cinit is not None else None)
    llr = out if out is not None else t.empty((T, n * Qm), dtype=llr_dtype, device=sym.device)
    assert llr.dtype in (t.float32, t.float64) and llr.shape == (T, n * Qm) and llr.stride(1) == 1
    with t.cuda.device(sym.device):
        _lib.check(_lib.lib().ldpc5g_demod_descramble(
            _lib.ptr(sym), _lib.F32 if sym.dtype == t.complex64 else _lib.F64, sym.stride(0),
            _lib.ptr(nv), nv.stride(0), _lib.ptr(w) if w is not None else None,
            w.stride(0) if w is not None else 0, T, n, int(mod), _lib.ptr(llr),
            _lib.F64 if llr.dtype == t.float64 else _lib.F32, llr.stride(0),
            _lib.stream_ptr(sym.device)))
    return llr
