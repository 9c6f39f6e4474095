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
    channel_estimate(h_ls (T, S, N, Nr, Nt), sym_map, algo, scs, eRB, l_left_ns, l_right_ns, ...)
        -> (h (T, 14*N*D, Nr, Nt), cov (T, 14*PRB, Nr, Nr))   (dft_dct_CE.py, dft_dct_symmetric_CE.py,
                                                              nr_channel_estimation.py:66-83,150-221)
    to_compensate(y (T, nsym, RE, Nr), to_avg (T,), scs)       (nr_channel_estimation.py:209-221)
    slot_frontend(grid (T, Nr, 14*carrier_re), slots (T,), pdsch_config)
        -> (h_ls (T, S, 3*RBSize, Nr, NL), y (T, 14*12*RBSize, Nr))   (nr_pdsch_dmrs.py:139-227,
                                            nr_pusch_dmrs.py:107-200, nrpdsch_resource_mapping.py:87-129)
    slot_map(sym (T, nre*NL), slots, pdsch_config, carrier_prbs, num_ant) -> grid (T, num_ant, 14*carrier_re)
                        (nr_pdsch_dmrs.py:90-120, nr_pdsch_process.py:27-42, nrpdsch_resource_mapping.py:58-85)
    dmrs_symlist(Ld, DMRSAddPos), slot_data_re_idx(pdsch_config) -> (re_idx, usage): host helpers
    transform_precode(x (T, nsym*12*RBSize), rb_size, inverse=False) -> same shape: the DFT / IDFT of
        every 12*RBSize block                            (nr_pusch_process.py:39-54, nr_pusch.py:170-194)
    low_papr_seq(u, v, MZC, alpha=0.0) -> (n, MZC) complex128              (lowPAPR_seq.py:5-41)
    pusch_tp_frontend / pusch_tp_map: slot_frontend / slot_map for a pusch_config with nTransPrecode = 1
        (the low-PAPR DMRS with group / sequence hopping, nr_pusch_dmrs.py:216-249)
    ofdm_params(scs, carrier_prbs) -> (nfft, cp_list, slot_len)
    ofdm_demod(td (T, Nr, 15*nfft), scs, carrier_prbs, carrier_frequency_in_mhz=0) -> grid (T, Nr, 14*12*prbs)
    ofdm_mod(grid, scs, carrier_prbs, carrier_frequency_in_mhz=0, dm=None) -> td   (nr_lowphy/rx_lowphy_process.py:35-98,
                                                                                   tx_lowphy_process.py:10-80)
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
    _lib.call("ldpc5g_prbs", c.device, cinit=c, T=T, nbits=int(nbits), words=w, ldw=w.stride(0))
    return w


def scramble_modulate(bits, mod, cinit=None, words=None, out=None):
    """bits: (T, G) int8 0/1 device tensor; mod: MOD_ID value; cinit: (T,) device tensor or None
    (no scrambling); words: precomputed prbs_words (reused across calls) instead of cinit."""
    t = _lib.require_gpu()
    assert bits.dim() == 2 and bits.dtype == t.int8 and bits.stride(1) == 1
    T, G = bits.shape
    Qm = bits_per_symbol(mod)
    w = words if words is not None else (None if cinit is None else prbs_words(cinit, G))
    sym = out if out is not None else t.empty((T, G // Qm), dtype=t.complex64, device=bits.device)
    _lib.call("ldpc5g_scramble_modulate", bits.device, bits=bits, ldb=bits.stride(0), prbs=w,
              ldw=w.stride(0) if w is not None else 0, T=T, nbits=G, mod=int(mod), sym=sym, ldsym=sym.stride(0))
    return sym


def _mimo_inputs(t, y, h, cov, re_idx, re_per_cov):
    """The checks of y, h, cov and re_idx that equalize and ml_detect share -> (T, NL, nre, the
    library arguments y .. NL that ldpc5g_equalize and ldpc5g_ml_detect have in common)."""
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
    ld = _lib.row_stride
    return T, NL, nre, dict(y=y, ldy=ld(y, 0, R * Nr), h=h, ldh=ld(h, 0, R * Nr * NL), cov=cov,
                            ldcov=ld(cov, 0, cov.shape[1] * Nr * Nr), in_dtype=_lib.dtype_id(y.dtype),
                            re_idx=re_idx, R=R, nre=nre, re_per_cov=int(re_per_cov), T=T, Nr=Nr, NL=NL)


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
    T, NL, nre, args = _mimo_inputs(t, y, h, cov, re_idx, re_per_cov)
    if out is not None:
        sym, nv = out
        assert sym.dtype == y.dtype and sym.shape == (T, nre * NL) and sym.stride(1) == 1
        assert nv.dtype == t.float32 and nv.shape == (T, nre * NL) and nv.stride(1) == 1
    else:
        sym = t.empty((T, nre * NL), dtype=y.dtype, device=y.device)
        nv = t.empty((T, nre * NL), dtype=t.float32, device=y.device)
    _lib.call("ldpc5g_equalize", y.device, **args, algo=_lib.EQ_ALGO[algo], sym=sym,
              ldsym=_lib.row_stride(sym, 0, nre * NL), noise_var=nv, ldnv=_lib.row_stride(nv, 0, nre * NL))
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
    T, NL, nre, args = _mimo_inputs(t, y, h, cov, re_idx, re_per_cov)
    Qm = bits_per_symbol(mod)
    llr_dtype = llr_dtype or t.float64
    assert llr_dtype in (t.float32, t.float64)
    nbits = nre * NL * Qm
    w = words if words is not None else (None if cinit is None else prbs_words(cinit, nbits))
    llr = t.empty((T, nbits), dtype=llr_dtype, device=y.device)
    outs = {"sym": t.empty((T, nre * NL), dtype=t.complex64, device=y.device) if "sym" in want else None,
            "noise_var": t.empty((T, nre * NL), dtype=llr_dtype, device=y.device) if "noise_var" in want else None,
            "hardbits": t.empty((T, nbits), dtype=t.int8, device=y.device) if "hardbits" in want else None}
    code, irc = _lib.ML_ALGO[algo]
    _lib.call("ldpc5g_ml_detect", y.device, **args, mod=int(mod), algo=code, irc=irc, prbs=w,
              ldw=0 if w is None else w.stride(0) if T > 1 else (nbits + 31) // 32, llr=llr,
              llr_dtype=_lib.dtype_id(llr_dtype), ldllr=nbits, sym=outs["sym"], ldsym=nre * NL,
              noise_var=outs["noise_var"], ldnv=nre * NL, hardbits=outs["hardbits"], ldhb=nbits)
    return (llr, *(outs[k] for k in want)) if want else llr


def ce_lengths(n, algo, eRB, re_distance=4):
    """(eK, right_eK, M): extension points per side and the transform length of an N-point DMRS
    sequence (dft_dct_CE.py:29,38; dft_dct_symmetric_CE.py:60)."""
    eK = int(eRB) * 12 // int(re_distance)
    right_eK = eK + (int(n) + eK) % 2
    M = int(n) + eK + right_eK
    return eK, right_eK, 2 * M if algo.endswith("_symmetric") else M


def ce_window(algo, M, scs, re_distance, l_left_ns, l_right_ns):
    """(L_left, L_right) in samples: the reference's own double expressions, which its two files
    word differently (dft_dct_CE.py:64-68; dft_dct_symmetric_CE.py:73-79)."""
    if algo.endswith("_symmetric"):
        h_sym_sample_rate_in_hz = M * scs * 1000 * re_distance
        L_left = int(l_left_ns / (10**9 / h_sym_sample_rate_in_hz))
        L_left = min(M // 3 + M // 16, L_left)
        return L_left, L_left
    h_sym_sample_rate_in_hz = scs * 1000 * re_distance * M
    return int(l_left_ns * 1e-9 * h_sym_sample_rate_in_hz), int(l_right_ns * 1e-9 * h_sym_sample_rate_in_hz)


CE_WANT = ("h_est", "noise_power", "taps", "to_est", "to_avg", "h_ls_comp")


def channel_estimate(h_ls, sym_map, algo, scs, eRB, l_left_ns, l_right_ns, re_distance=4, num_cdm_groups=2,
                     to_comp=False, out=None, want=(), work=None):
    """DFT / DCT channel estimation of T slots with the noise-plus-interference covariance and the
    optional timing-offset compensation (ldpc5g_channel_estimate; dft_dct_CE.py,
    dft_dct_symmetric_CE.py, nr_channel_estimation.py:66-83,150-221).  h_ls: (T, S, N, Nr, Nt)
    complex64 / complex128 device tensor (only stride(0) is free); sym_map: the S DMRS symbol
    indices (RSSymMap); algo: "DFT", "DCT", "DFT_symmetric" or "DCT_symmetric"; scs in kHz; eRB
    extra PRBs per side; l_left_ns / l_right_ns the window lengths in ns.  Returns (h (T,
    14*N*D, Nr, Nt), cov (T, 14*PRB, Nr, Nr)) of the input dtype — phy.equalize's and
    phy.ml_detect's h and cov with re_per_cov = 12 — or fills out=(h, cov).  With want= (any of
    "h_est" (T, S, N*D, Nr, Nt), "noise_power" (T, S, Nr, Nt) float64, "taps" (T, S, Nr, Nt, M)
    uint8 kept mask, "to_est" (T, S) and "to_avg" (T,) float64 seconds, "h_ls_comp" the compensated
    h_ls (to_comp only)) a dict of those is returned as a third value."""
    t = _lib.require_gpu()
    assert algo in _lib.CE_ALGO, f"algo {algo!r}: one of {sorted(_lib.CE_ALGO)}"
    assert all(w in CE_WANT for w in want), want
    assert h_ls.dim() == 5 and h_ls.dtype in (t.complex64, t.complex128)
    assert h_ls[0].is_contiguous(), "only the slot stride is free"
    T, S, N, Nr, Nt = h_ls.shape
    D = int(re_distance)
    sym = [int(s) for s in sym_map]
    assert len(sym) == S, f"{len(sym)} symbol indices for S={S} DMRS symbols"
    eK, _, M = ce_lengths(N, algo, eRB, D)
    L_left, L_right = ce_window(algo, M, int(scs), D, l_left_ns, l_right_ns)
    ND = N * D
    PRB = ND // 12
    dev = h_ls.device
    if out is not None:
        h, cov = out
        assert h.dtype == h_ls.dtype and h.shape == (T, 14 * ND, Nr, Nt) and h[0].is_contiguous()
        assert cov.dtype == h_ls.dtype and cov.shape == (T, 14 * PRB, Nr, Nr) and cov[0].is_contiguous()
    else:
        h = t.empty((T, 14 * ND, Nr, Nt), dtype=h_ls.dtype, device=dev)
        cov = t.empty((T, 14 * PRB, Nr, Nr), dtype=h_ls.dtype, device=dev)
    need = int(_lib.invoke("ldpc5g_ce_workspace_bytes", T=T, S=S, N=N, Nr=Nr, Nt=Nt, D=D))
    if work is None:
        work = t.empty((max(need, 16),), dtype=t.uint8, device=dev)
    assert work.dtype == t.uint8 and work.is_contiguous() and work.device == dev
    outs = {
        "h_est": t.empty((T, S, ND, Nr, Nt), dtype=h_ls.dtype, device=dev) if "h_est" in want else None,
        "noise_power": t.empty((T, S, Nr, Nt), dtype=t.float64, device=dev) if "noise_power" in want else None,
        "taps": t.empty((T, S, Nr, Nt, M), dtype=t.uint8, device=dev) if "taps" in want else None,
        "to_est": t.empty((T, S), dtype=t.float64, device=dev) if "to_est" in want else None,
        "to_avg": t.empty((T,), dtype=t.float64, device=dev) if "to_avg" in want else None,
        "h_ls_comp": t.empty((T, S, N, Nr, Nt), dtype=h_ls.dtype, device=dev) if "h_ls_comp" in want else None}
    ld = _lib.row_stride
    sym_arr = (_lib.ctypes.c_int32 * max(S, 1))(*sym)
    _lib.call("ldpc5g_channel_estimate", dev, h_ls=h_ls, ldhls=ld(h_ls, 0, S * N * Nr * Nt),
              in_dtype=_lib.dtype_id(h_ls.dtype), T=T, S=S, N=N, Nr=Nr, Nt=Nt, D=D, sym_idx=sym_arr,
              algo=_lib.CE_ALGO[algo], eK=eK, L_left=L_left, L_right=L_right, num_cdm_groups=int(num_cdm_groups),
              to_comp=1 if to_comp else 0, scs=int(scs), h=h, ldh=ld(h, 0, 14 * ND * Nr * Nt), cov=cov,
              ldcov=ld(cov, 0, 14 * PRB * Nr * Nr), work=work, work_bytes=work.numel(),
              h_ls_comp=outs["h_ls_comp"], ldhc=S * N * Nr * Nt, h_est=outs["h_est"],
              noise_power=outs["noise_power"], taps=outs["taps"], to_est=outs["to_est"], to_avg=outs["to_avg"])
    return (h, cov, {k: outs[k] for k in want}) if want else (h, cov)


def to_compensate(y, to_avg, scs, out=None):
    """Timing-offset compensation of the data REs (ldpc5g_to_compensate; comp_pdsch_timing_offset,
    nr_channel_estimation.py:209-221): y (T, nsym, RE, Nr) complex64 / complex128 times
    exp(-j 2 pi to_avg[t] k scs 1000), k the RE index; to_avg: (T,) float64 device tensor
    (channel_estimate's want="to_avg").  Returns a new tensor, or fills out (which may be y)."""
    t = _lib.require_gpu()
    assert y.dim() == 4 and y.dtype in (t.complex64, t.complex128) and y[0].is_contiguous()
    T, nsym, RE, Nr = y.shape
    assert to_avg.shape == (T,) and to_avg.dtype == t.float64 and to_avg.is_contiguous() and to_avg.device == y.device
    if out is None:
        out = t.empty((T, nsym, RE, Nr), dtype=y.dtype, device=y.device)
    assert out.dtype == y.dtype and out.shape == y.shape and out[0].is_contiguous()
    row = nsym * RE * Nr
    _lib.call("ldpc5g_to_compensate", y.device, y=y, ldy=_lib.row_stride(y, 0, row), out=out,
              ldo=_lib.row_stride(out, 0, row), in_dtype=_lib.dtype_id(y.dtype), to_avg=to_avg, T=T, nsym=nsym,
              RE=RE, Nr=Nr, scs=int(scs))
    return out


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
    w = words if words is not None else (None if cinit is None else prbs_words(cinit, n * Qm))
    llr = out if out is not None else t.empty((T, n * Qm), dtype=llr_dtype, device=sym.device)
    assert llr.dtype in (t.float32, t.float64) and llr.shape == (T, n * Qm) and llr.stride(1) == 1
    _lib.call("ldpc5g_demod_descramble", sym.device, sym=sym, sym_dtype=_lib.dtype_id(sym.dtype),
              ldsym=sym.stride(0), noise_var=nv, ldnv=nv.stride(0), prbs=w, ldw=w.stride(0) if w is not None else 0,
              T=T, nsym=n, mod=int(mod), llr=llr, llr_dtype=_lib.dtype_id(llr.dtype), ldllr=llr.stride(0))
    return llr


# ------------------------------------------------------------------ the slot front end
def dmrs_symlist(Ld, DMRSAddPos, channel="pdsch"):
    """DMRS symbol indices of a mapping-type-A, single-symbol allocation whose last symbol is
    Ld - 1: 38.211 Table 7.4.1.1.2-3 (nr_pdsch_dmrs.py:258-297, get_DMRS_symlist) and Table
    6.4.1.1.3-3 with dmrs-TypeA-Position pos2 (nr_pusch_dmrs.py:251-286), which hold the same
    entries."""
    assert channel in ("pdsch", "pusch"), channel
    assert 0 <= DMRSAddPos <= 3, f"DMRSAddPos {DMRSAddPos}"
    if Ld <= 7 or DMRSAddPos == 0:
        return [2]
    if Ld <= 9:
        return [2, 7]
    if Ld <= 12:
        return [[2, 9], [2, 6, 9], [2, 6, 9] if Ld <= 11 else [2, 5, 8, 11]][DMRSAddPos - 1]
    return [[2, 11], [2, 7, 11], [2, 5, 8, 11]][DMRSAddPos - 1]


def _slot_params(config):
    """The fields of the reference's pdsch_config / pusch_config dict that the slot front end
    uses, after the reference's own asserts (nr_pdsch_dmrs.py:155-165, nr_pusch_dmrs.py:127-142)."""
    dm = config["DMRS"]
    pusch = "nTransPrecode" in config
    assert dm["DMRSConfigType"] == 1
    assert dm["NrOfDMRSSymbols"] == 1
    assert dm["PUSCHMappintType" if pusch else "PDSCHMappintType"] == "A"
    assert dm["DMRSAddPos"] <= 3
    nscid = int(dm["nSCID"])
    if pusch:
        assert dm["dmrs_TypeA_Position"] == "pos2"
        if config["nTransPrecode"] != 0:
            raise NotImplementedError("nTransPrecode != 0: transform precoding (the low-PAPR DMRS sequence, "
                                      "nr_pusch_dmrs.py:216-228) is not provided here: see pusch_tp_frontend, "
                                      "pusch_tp_map and sch.sch_pusch_tp_rx_batch")
        nid = dm["transformPrecodingDisabled"]["NID0" if nscid == 0 else "NID1"]
    else:
        nid = dm["nNIDnSCID"]
    NL = int(config["num_of_layers"])
    start, nsym = int(config["StartSymbolIndex"]), int(config["NrOfSymbols"])
    return dict(rb_start=int(config["ResAlloType1"]["RBStart"]), rb_size=int(config["ResAlloType1"]["RBSize"]),
                NL=NL, ports=[int(p) for p in list(config["PortIndexList"])[:NL]], start=start, nsym=nsym,
                symlist=dmrs_symlist(start + nsym, int(dm["DMRSAddPos"]), "pusch" if pusch else "pdsch"),
                cdm=int(dm["NumCDMGroupsWithoutData"]), nid=int(nid), nscid=nscid, pusch=pusch)


def slot_data_re_idx(pdsch_config):
    """(re_idx, usage) of an allocation.  usage: copy_Rx_pdsch_resource's (NrOfSymbols, 12*RBSize)
    float64 map, 1 where a DMRS symbol's RE is not available for data
    (nrpdsch_resource_mapping.py:102-127): all twelve REs of a PRB when NumCDMGroupsWithoutData == 2,
    otherwise the even REs if a used port is 1000 or 1001 and the odd REs if one is 1002 or 1003.
    re_idx: the ascending int32 flat indices sym * 12*RBSize + re, over the slot's 14 symbols, of the
    data REs (usage == 0) of symbols StartSymbolIndex .. StartSymbolIndex + NrOfSymbols - 1 — the
    re_idx of equalize / ml_detect on slot_frontend's y.  Host arrays (numpy)."""
    import numpy as np
    p = _slot_params(pdsch_config)
    prb = np.zeros(12)
    if p["cdm"] == 2:
        prb[:] = 1
    else:
        if 1000 in p["ports"] or 1001 in p["ports"]:
            prb[0::2] = 1
        if 1002 in p["ports"] or 1003 in p["ports"]:
            prb[1::2] = 1
    n = 12 * p["rb_size"]
    usage = np.zeros((p["nsym"], n))
    for s in p["symlist"]:
        if p["start"] <= s < p["start"] + p["nsym"]:
            usage[s - p["start"]] = np.tile(prb, p["rb_size"])
    m, re = np.nonzero(usage == 0)
    return ((m + p["start"]) * n + re).astype(np.int32), usage


def slot_data_re_idx_device(pdsch_config, device):
    """slot_data_re_idx's re_idx uploaded to `device`: a new tensor per call.  A caller that
    receives many batches of one allocation uploads once and passes it as re_idx= to
    sch.sch_slot_rx_batch / slot_map."""
    _slot_params(pdsch_config)   # the reference's asserts come before any GPU work
    t = _lib.require_gpu()
    return t.from_numpy(slot_data_re_idx(pdsch_config)[0]).to(device)


def _frontend(grid, slots, want, params, entry, seq_args):
    """What slot_frontend and pusch_tp_frontend share.  params(): the configuration's fields after
    the asserts and refusals that come before any GPU work; entry: the library call; seq_args(p, T,
    S, dev): the keyword arguments only that entry has (the layers' ports and the DMRS sequence's)."""
    assert want and all(w in ("h_ls", "y") for w in want), f"want {want!r}: a selection of 'h_ls', 'y'"
    p = params()
    t = _lib.require_gpu()
    assert grid.dim() == 3 and grid.dtype in (t.complex64, t.complex128) and grid[0].is_contiguous(), \
        "grid: (T, Nr, 14*carrier_re) complex, only the slot stride is free"
    T, Nr, W = grid.shape
    assert W % 14 == 0, f"grid rows of {W} elements are not 14 symbols"
    assert slots.shape == (T,) and slots.dtype == t.int32 and slots.is_contiguous() and slots.device == grid.device
    S, N, NL = len(p["symlist"]), 3 * p["rb_size"], p["NL"]
    dev = grid.device
    variant = seq_args(p, T, S, dev)
    h_ls = t.empty((T, S, N, Nr, NL), dtype=grid.dtype, device=dev) if "h_ls" in want else None
    y = t.empty((T, 14 * 4 * N, Nr), dtype=grid.dtype, device=dev) if "y" in want else None
    syms = (_lib.ctypes.c_int32 * 4)(*p["symlist"])
    _lib.call(entry, dev, grid=grid, ldgrid=_lib.row_stride(grid, 0, Nr * W), in_dtype=_lib.dtype_id(grid.dtype),
              slots=slots, T=T, carrier_re=W // 14, rb_start=p["rb_start"], rb_size=p["rb_size"], Nr=Nr, S=S,
              sym_idx=syms, h_ls=h_ls, ldh=S * N * Nr * NL, y=y, ldy=14 * 4 * N * Nr, **variant)
    outs = {"h_ls": h_ls, "y": y}
    return tuple(outs[w] for w in want)


def slot_frontend(grid, slots, pdsch_config, want=("h_ls", "y")):
    """The received slot grids of T slots to the channel estimator's and the detectors' inputs
    (ldpc5g_slot_rx_frontend; pdsch_dmrs_LS_est, nr_pdsch_dmrs.py:139-227, or pusch_dmrs_LS_est,
    nr_pusch_dmrs.py:107-200, and copy_Rx_pdsch_resource, nrpdsch_resource_mapping.py:87-129).
    grid: (T, Nr, 14*carrier_re) complex64 / complex128 device tensor, antenna-planar as the
    reference's rx_fd_slot_data (only the slot stride is free); slots: (T,) int32 device tensor of
    slot numbers; pdsch_config: the reference's pdsch_config (or pusch_config) dict.  Returns, in
    the order of `want`, a tuple of h_ls (T, S, 3*RBSize, Nr, NL) — channel_estimate's input — and
    y (T, 14*12*RBSize, Nr) — the allocation's PRBs of all 14 symbols, interleaved — of grid's dtype."""
    def seq_args(p, T, S, dev):
        ports = (_lib.ctypes.c_int32 * 4)(*[q - 1000 for q in p["ports"]])
        return dict(Nt=p["NL"], ports=ports, nNIDnSCID=p["nid"], nSCID=p["nscid"], num_cdm_groups=p["cdm"])
    return _frontend(grid, slots, want, lambda: _slot_params(pdsch_config), "ldpc5g_slot_rx_frontend", seq_args)


def _map(t, sym, slots, p, carrier_prbs, num_ant, precoding, out, re_idx, entry, seq_args, prepare=None):
    """What slot_map and pusch_tp_map share, after their parameter extraction.  re_idx: the
    device tensor; entry: the library call; seq_args(T, S, dev): the keyword arguments only that
    entry has (the layers and the DMRS sequence's); prepare: what becomes of sym on its way into
    the call."""
    import numpy as np
    NL, dev, num_ant = p["NL"], sym.device, int(num_ant)
    assert re_idx.dim() == 1 and re_idx.dtype == t.int32 and re_idx.is_contiguous() and re_idx.device == dev
    nre = re_idx.shape[0]
    assert sym.dim() == 2 and sym.dtype == t.complex64 and sym.stride(1) == 1
    T = sym.shape[0]
    assert sym.shape[1] == nre * NL, f"sym has {sym.shape[1]} symbols per slot, the allocation holds nre*NL = {nre}*{NL}"
    assert slots.shape == (T,) and slots.dtype == t.int32 and slots.is_contiguous() and slots.device == dev
    W = 14 * 12 * int(carrier_prbs)
    if out is None:
        out = t.zeros((T, num_ant, W), dtype=t.complex64, device=dev)
    assert out.dtype == t.complex64 and out.shape == (T, num_ant, W) and out[0].is_contiguous() and out.device == dev
    pm = None
    if precoding is not None:
        w = np.asarray(precoding, np.complex64)
        w = np.ascontiguousarray((w.reshape(-1, 1) if NL == 1 else w)[:num_ant, :NL])
        assert w.shape == (num_ant, NL), f"precoding {w.shape}: (num_ant, NL) = ({num_ant}, {NL}) wanted"
        pm = w   # (num_ant, NL) complex64 = the ABI's interleaved float pairs
    S = len(p["symlist"])
    variant = seq_args(T, S, dev)
    if prepare is not None:
        sym = prepare(sym)
    syms = (_lib.ctypes.c_int32 * 4)(*p["symlist"])
    _lib.call(entry, dev, sym=sym, ldsym=_lib.row_stride(sym, 0, nre * NL), re_idx=re_idx, nre=nre, slots=slots,
              T=T, carrier_re=W // 14, rb_start=p["rb_start"], rb_size=p["rb_size"], num_ant=num_ant,
              precoding=pm, S=S, sym_idx=syms, grid=out, ldgrid=_lib.row_stride(out, 0, num_ant * W), **variant)
    return out


def slot_map(sym, slots, pdsch_config, carrier_prbs, num_ant, precoding=None, out=None, re_idx=None):
    """The transmit-side inverse of slot_frontend (ldpc5g_slot_map; pdsch_dmrs_process,
    nr_pdsch_dmrs.py:90-120, the precoding of nr_pdsch_process.py:27-42 and pdsch_data_re_mapping,
    nrpdsch_resource_mapping.py:58-85).  sym: (T, nre*NL) complex64 layer-interleaved modulated
    symbols (scramble_modulate's output), nre = len(slot_data_re_idx(pdsch_config)[0]); slots: (T,)
    int32 device tensor; precoding: (num_ant, NL) array-like or None for identity.  Layers use ports
    1000 .. 1000 + NL - 1 in order; re_idx: slot_data_re_idx_device's tensor, to save its upload.
    Writes DMRS and data into out (T, num_ant, 14*12*carrier_prbs)
    complex64 — every other RE is left as it is — or into a new zeroed grid, and returns it."""
    p = _slot_params(pdsch_config)
    t = _lib.require_gpu()
    NL = p["NL"]
    assert p["ports"] == [1000 + l for l in range(NL)], \
        f"PortIndexList {p['ports']}: the transmit map needs ports 1000..{999 + NL} in order (nr_pdsch_dmrs.py:81-84)"
    if re_idx is None:
        re_idx = slot_data_re_idx_device(pdsch_config, sym.device)
    return _map(t, sym, slots, p, carrier_prbs, num_ant, precoding, out, re_idx, "ldpc5g_slot_map",
                lambda T, S, dev: dict(NL=NL, nNIDnSCID=p["nid"], nSCID=p["nscid"], num_cdm_groups=p["cdm"]))


# ------------------------------------------------------------------ PUSCH transform precoding
HOPPING_ID = {"neither": 0, "groupHopping": 1, "sequenceHopping": 2}   # groupOrSequenceHopping -> ABI


def tp_rb_ok(rb_size):
    """RBSize = 2^a 3^b 5^c in 1..275 (38.211 6.3.1.4): the lengths the transform is built for."""
    n = int(rb_size)
    if not 1 <= n <= 275:
        return False
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


def _tp_check_rb(rb_size):
    if not tp_rb_ok(rb_size):
        raise NotImplementedError(f"RBSize {rb_size}: transform precoding needs RBSize = 2^a 3^b 5^c in 1..275 "
                                  "(38.211 6.3.1.4)")


def transform_precode(x, rb_size, inverse=False, out=None):
    """The transform precoding of 38.211 6.3.1.4 and its inverse (ldpc5g_transform_precode): every
    block of M = 12*rb_size elements of a row of x is replaced by its orthonormal DFT
    (np.fft.fft(.) / sqrt(M), nr_pusch_process.py:53) or, with inverse=True, IDFT (np.fft.ifft(.) *
    sqrt(M), nr_pusch.py:188).  x: (T, nsym*M) complex64 / complex128 device tensor (only the row
    stride is free), nsym <= 14; float64 arithmetic for both.  Returns a new tensor or fills out,
    which may be x itself."""
    _tp_check_rb(rb_size)
    t = _lib.require_gpu()
    M = 12 * int(rb_size)
    assert x.dim() == 2 and x.dtype in (t.complex64, t.complex128) and x.stride(1) == 1, \
        "x: (T, nsym*12*rb_size) complex, only the row stride is free"
    T, W = x.shape
    assert W % M == 0 and 1 <= W // M <= 14, f"rows of {W} elements are not 1..14 blocks of 12*rb_size = {M}"
    if out is None:
        out = t.empty((T, W), dtype=x.dtype, device=x.device)
    assert out.dtype == x.dtype and out.shape == (T, W) and out.stride(1) == 1 and out.device == x.device
    _lib.call("ldpc5g_transform_precode", x.device, x=x, ldx=_lib.row_stride(x, 0, W), out=out,
              ldo=_lib.row_stride(out, 0, W), in_dtype=_lib.dtype_id(x.dtype), T=T, nsym=W // M,
              rb_size=int(rb_size), inverse=1 if inverse else 0)
    return out


def low_papr_seq(u, v, MZC, alpha=0.0, device=None):
    """Low-PAPR sequences exp(j alpha m) rbar_{u,v}(m), m < MZC (ldpc5g_low_papr_seq;
    gen_lowPAPR_seq, lowPAPR_seq.py:5-41).  u, v: integers or sequences of n integers (group 0..29,
    base sequence 0..1, 0 when MZC < 72 — checked as the reference asserts), or (n,) int32 device
    tensors (not checked).  Returns an (n, MZC) complex128 device tensor.  MZC in {6, 12, 18, 24}
    are the tables of 38.211 5.2.2.2, which are not provided."""
    import numpy as np
    MZC = int(MZC)
    assert MZC % 6 == 0 and 6 <= MZC <= 3300, f"MZC {MZC}: a multiple of 6 in 6..3300"
    if MZC in (6, 12, 18, 24):
        raise NotImplementedError(f"MZC {MZC}: the sequences of length 6, 12, 18, 24 are the tables of 38.211 "
                                  "5.2.2.2, which are not provided")
    host = not hasattr(u, "data_ptr")
    if host:
        u = np.atleast_1d(np.asarray(u)).astype(np.int32)
        v = np.broadcast_to(np.atleast_1d(np.asarray(v)).astype(np.int32), u.shape).copy()
        assert u.ndim == 1 and u.size >= 1
        assert ((u >= 0) & (u < 30)).all(), "u in range(30)"
        assert ((v >= 0) & (v <= (1 if MZC >= 72 else 0))).all(), "v == 0 for MZC <= 60, v in [0, 1] for MZC >= 72"
    t = _lib.require_gpu()
    if host:
        dev = t.device("cuda", t.cuda.current_device()) if device is None else t.device(device)
        u, v = t.from_numpy(u).to(dev), t.from_numpy(v).to(dev)
    assert u.dim() == 1 and u.dtype == t.int32 and u.is_contiguous()
    assert v.shape == u.shape and v.dtype == t.int32 and v.is_contiguous() and v.device == u.device
    n = u.shape[0]
    out = t.empty((n, MZC), dtype=t.complex128, device=u.device)
    _lib.call("ldpc5g_low_papr_seq", u.device, u=u, v=v, n=n, alpha=float(alpha), MZC=MZC, out=out)
    return out


def _tp_params(config, base_seq=None, need_seq=True):
    """_slot_params for a pusch_config with nTransPrecode = 1: the reference's asserts
    (nr_pusch_dmrs.py:127-145, nr_pusch_process.py:45, nr_pusch.py:176-179) and this library's
    refusals."""
    assert "nTransPrecode" in config, "a pusch_config is wanted"
    assert config["nTransPrecode"] == 1, f"nTransPrecode {config['nTransPrecode']}: 1 wanted (0: slot_frontend / slot_map)"
    p = _slot_params(dict(config, nTransPrecode=0))
    assert p["NL"] == 1, f"num_of_layers {p['NL']}: transform precoding has one layer (nr_pusch_process.py:45)"
    assert p["cdm"] == 2, ("NumCDMGroupsWithoutData 1: data on the DMRS symbols breaks the reference's "
                           "assert demod_LLRs.size % MPUSCHSC == 0 (nr_pusch.py:179)")
    _tp_check_rb(p["rb_size"])
    en = config["DMRS"]["transformPrecodingEnabled"]
    nid = int(en["nPuschID"])
    assert 0 <= nid <= 1007, f"nPuschID {nid} outside 0..1007"
    hop = en["groupOrSequenceHopping"]
    assert hop in HOPPING_ID, f"groupOrSequenceHopping {hop!r}: one of {sorted(HOPPING_ID)}"
    if need_seq and p["rb_size"] <= 4 and base_seq is None:
        raise NotImplementedError(f"RBSize <= 4 (RBSize {p['rb_size']}): the DMRS sequences of length 6..24 are the "
                                  "tables of 38.211 5.2.2.2, which are not provided: pass them as base_seq")
    return dict(p, npuschid=nid, hopping=HOPPING_ID[hop])


def pusch_tp_data_re_idx(pusch_config):
    """slot_data_re_idx for a pusch_config with nTransPrecode = 1 (the RE usage does not depend on
    the DMRS sequence)."""
    _tp_params(pusch_config, need_seq=False)
    return slot_data_re_idx(dict(pusch_config, nTransPrecode=0))


def _tp_base_seq(base_seq, T, S, MZC, dev):
    """base_seq as a (T, S, MZC) complex128 contiguous device tensor; an array (S, MZC) or
    (T, S, MZC) on the host is uploaded."""
    import numpy as np
    t = _lib.torch()
    if base_seq is None:
        return None
    if not hasattr(base_seq, "data_ptr"):
        a = np.asarray(base_seq, np.complex128)
        assert a.shape in ((S, MZC), (T, S, MZC)), f"base_seq {a.shape}: ({S}, {MZC}) or ({T}, {S}, {MZC}) wanted"
        base_seq = t.from_numpy(np.array(np.broadcast_to(a, (T, S, MZC)))).to(dev)   # a writable copy
    assert base_seq.dtype == t.complex128 and base_seq.shape == (T, S, MZC) and base_seq.is_contiguous() \
        and base_seq.device == dev, f"base_seq: ({T}, {S}, {MZC}) complex128 contiguous on {dev}"
    return base_seq


def _tp_seq_args(p, base_seq, T, S, dev):
    """The keyword arguments only the two _tp library calls have"""
    bs = _tp_base_seq(base_seq, T, S, 6 * p["rb_size"], dev)
    return dict(port=p["ports"][0] - 1000, nPuschID=p["npuschid"], hopping=p["hopping"], base_seq=bs)


def pusch_tp_frontend(grid, slots, pusch_config, want=("h_ls", "y"), base_seq=None):
    """slot_frontend for a pusch_config with nTransPrecode = 1 (ldpc5g_slot_rx_frontend_tp;
    pusch_dmrs_LS_est, nr_pusch_dmrs.py:107-200 with the low-PAPR sequence of :216-249, its group /
    sequence hopping following slots).  One layer, NumCDMGroupsWithoutData = 2, RBSize = 2^a 3^b 5^c.
    base_seq: the DMRS base sequences, (S, 6*RBSize) or (T, S, 6*RBSize) complex128 (host array or
    device tensor), instead of the generated ones; needed for RBSize <= 4.  Returns, in the order of
    `want`, h_ls (T, S, 3*RBSize, Nr, 1) and y (T, 14*12*RBSize, Nr) of grid's dtype."""
    return _frontend(grid, slots, want, lambda: _tp_params(pusch_config, base_seq), "ldpc5g_slot_rx_frontend_tp",
                     lambda p, T, S, dev: _tp_seq_args(p, base_seq, T, S, dev))


def pusch_tp_map(sym, slots, pusch_config, carrier_prbs, num_ant, precoding=None, out=None, re_idx=None,
                 base_seq=None):
    """slot_map for a pusch_config with nTransPrecode = 1: transform_precode on the modulated
    symbols (nr_pusch_process.py:39-54), then ldpc5g_slot_map_tp — the low-PAPR DMRS of
    nr_pusch_dmrs.py:66-101, the precoding and the data RE mapping.  sym: (T, nre) complex64
    modulated symbols of the one layer, nre = len(pusch_tp_data_re_idx(pusch_config)[0]) — whole
    symbols of 12*RBSize; precoding: (num_ant, 1) array-like or None (antenna 0 carries the layer);
    the layer's port is PortIndexList[0]; base_seq as pusch_tp_frontend.  Returns the grid
    (T, num_ant, 14*12*carrier_prbs) complex64 (out, or a new zeroed one)."""
    p = _tp_params(pusch_config, base_seq)
    t = _lib.require_gpu()
    if re_idx is None:
        re_idx = t.from_numpy(pusch_tp_data_re_idx(pusch_config)[0]).to(sym.device)
    return _map(t, sym, slots, p, carrier_prbs, num_ant, precoding, out, re_idx, "ldpc5g_slot_map_tp",
                lambda T, S, dev: _tp_seq_args(p, base_seq, T, S, dev),
                prepare=lambda x: transform_precode(x, p["rb_size"]))


# ------------------------------------------------------------------ OFDM low-PHY
OFDM_NFFT = (128, 256, 512, 1024, 2048, 4096)   # Rx_low_phy's assert (rx_lowphy_process.py:57)
_CP4096 = {30: [352] + [288] * 13, 15: [320] + [288] * 6 + [320] + [288] * 6}


def ofdm_params(scs, carrier_prbs):
    """(nfft, cp_list, slot_len) of a carrier: nfft = 2**ceil(log2(12*prbs/0.85)) (get_FFT_IFFT_size,
    nr_slot.py:64-69), the 14 cyclic-prefix lengths — the reference's 4096-point lists divided by
    4096/nfft (rx_lowphy_process.py:60-69) — and the slot length sum(cp) + 14*nfft = 15*nfft samples.
    Raises NotImplementedError for a subcarrier spacing other than 15 / 30 kHz or an nfft outside
    128..4096."""
    scs, prbs = int(scs), int(carrier_prbs)
    if scs not in _CP4096:
        raise NotImplementedError(f"scs {scs}: the low-PHY's CP tables are those of 15 and 30 kHz")
    assert prbs >= 1, f"carrier_prbs {carrier_prbs}"
    nfft = 1
    while 17 * nfft < 240 * prbs:   # nfft >= 12 prbs / 0.85, in integers
        nfft *= 2
    if nfft not in OFDM_NFFT:
        raise NotImplementedError(f"carrier_prbs {prbs}: nfft {nfft} outside {OFDM_NFFT}")
    cp = [c * nfft // 4096 for c in _CP4096[scs]]
    return nfft, cp, sum(cp) + 14 * nfft


def _carrier_hz(carrier_frequency_in_mhz):
    return int(carrier_frequency_in_mhz * (10 ** 6))   # rx_lowphy_process.py:49


def _ofdm_check(t, x, name, W, other):
    assert x.dim() == 3 and x.dtype in (t.complex64, t.complex128) and x.shape[2] == W and x.stride(2) == 1, \
        f"{name}: (T, Nr, {W}) complex64 / complex128, strides free on the first two dimensions"
    assert x.shape[1] in (1, 2, 4), f"{name}: {x.shape[1]} antennas, 1, 2 or 4 supported"
    if other is not None:
        assert other.dtype == x.dtype and other.device == x.device and other.shape[:2] == x.shape[:2], \
            f"out: dtype, device and (T, Nr) of {name}"


def ofdm_demod(td, scs, carrier_prbs, carrier_frequency_in_mhz=0, out=None):
    """Rx_low_phy (rx_lowphy_process.py:35-98) for T slots x Nr antennas in one launch
    (ldpc5g_ofdm_demod): the per-symbol carrier phase correction, the half-CP window, the FFT, the
    half-CP ramp and the crop to the carrier.  td: (T, Nr, 15*nfft) complex64 / complex128 device
    tensor, any strides on the first two dimensions (a transposed unflatten view of a multi-slot
    waveform works without a copy).  Returns the grid (T, Nr, 14*12*carrier_prbs) of td's dtype —
    sch_slot_rx_batch's input — or fills out.  float64 arithmetic for both dtypes.  Antennas are
    never permuted (the reference's fftshift without axes rolls them: rx_lowphy_process.Rx_low_phy
    here reproduces that)."""
    nfft, _, S = ofdm_params(scs, carrier_prbs)
    hz = _carrier_hz(carrier_frequency_in_mhz)
    t = _lib.require_gpu()
    W = 14 * 12 * int(carrier_prbs)
    _ofdm_check(t, td, "td", S, None)
    T, Nr = td.shape[:2]
    if out is None:
        out = t.empty((T, Nr, W), dtype=td.dtype, device=td.device)
    _ofdm_check(t, out, "out", W, td)
    ld = _lib.row_stride
    _lib.call("ldpc5g_ofdm_demod", td.device, td=td, ld_td_slot=ld(td, 0, S), ld_td_ant=ld(td, 1, S), grid=out,
              ld_g_slot=ld(out, 0, W), ld_g_ant=ld(out, 1, W), dtype=_lib.dtype_id(td.dtype), T=T, Nr=Nr, nfft=nfft,
              carrier_re=W // 14, scs=int(scs), carrier_hz=hz)
    return out


def ofdm_mod(grid, scs, carrier_prbs, carrier_frequency_in_mhz=0, dm=None, out=None):
    """Tx_low_phy (tx_lowphy_process.py:10-80) for T slots x num_ant antennas in one launch
    (ldpc5g_ofdm_mod): the IFFT, the cyclic prefix and the per-symbol carrier phase compensation of
    38.211 5.4.  grid: (T, num_ant, 14*12*carrier_prbs) complex64 / complex128 device tensor, any
    strides on the first two dimensions; dm: None or the per-symbol timing errors in seconds, (T, 14)
    or (14,) — RE k of symbol s is first turned by exp(2 pi j k scs 1000 dm[t][s]), the product rounded
    to grid's dtype (:54-55); grid itself is not written.  Returns td (T, num_ant, 15*nfft) of grid's
    dtype or fills out."""
    nfft, _, S = ofdm_params(scs, carrier_prbs)
    hz = _carrier_hz(carrier_frequency_in_mhz)
    t = _lib.require_gpu()
    W = 14 * 12 * int(carrier_prbs)
    _ofdm_check(t, grid, "grid", W, None)
    T, Na = grid.shape[:2]
    if dm is not None:
        dm = t.as_tensor(dm, dtype=t.float64, device=grid.device)
        assert dm.shape in ((14,), (T, 14)), f"dm {tuple(dm.shape)}: (14,) or (T, 14) seconds per symbol"
        dm = dm.expand(T, 14).contiguous()
    if out is None:
        out = t.empty((T, Na, S), dtype=grid.dtype, device=grid.device)
    _ofdm_check(t, out, "out", S, grid)
    ld = _lib.row_stride
    _lib.call("ldpc5g_ofdm_mod", grid.device, grid=grid, ld_g_slot=ld(grid, 0, W), ld_g_ant=ld(grid, 1, W), dm=dm,
              td=out, ld_td_slot=ld(out, 0, S), ld_td_ant=ld(out, 1, S), dtype=_lib.dtype_id(grid.dtype), T=T,
              num_ant=Na, nfft=nfft, carrier_re=W // 14, scs=int(scs), carrier_hz=hz)
    return out
