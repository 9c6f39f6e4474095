"""Batched GPU DL-SCH / UL-SCH chain (TS 38.212 §7.2 / §6.2) over transport blocks that share
one configuration — the C-ABI entry points ldpc5g_sch_* of include/ldpc5g.h.

    sch_config(A, Qm, coderateby1024, NL, rv, TBS_LBRM, G) -> SchCfg      (host only)
    crc_rows(bits[R, >=n], poly, nbits=None) -> rem[R] uint32             (crc.py:4-88)
    sch_encode_batch(trblk[T, A], cfg) -> g[T, E_total]                    (nr_dlsch.py:12-74)
    sch_decode_batch(llr[T, E_total], cfg, L, ...) -> SchDecodeResult      (nr_dlsch_decode.py)
    sch_demod_raterecover_batch(sym[T, E_total/Qm], noise_var, mod, cfg, ...) -> llr_dn[T*C, N]
    sch_rx_batch(sym, noise_var, mod, cfg, L, ...) -> SchDecodeResult      (nr_pdsch.py:245-281)
    sch_eq_rx_batch(y, h, cov, algo, re_idx, mod, cfg, L, ...) -> SchDecodeResult   (the same, from
        the received resource grid, channel estimate and covariance: phy.equalize first)
    sch_ml_rx_batch(y, h, cov, algo, re_idx, mod, cfg, L, ...) -> SchDecodeResult   (the same with a
        maximum-likelihood detector: phy.ml_detect, whose LLRs go straight to sch_decode_batch)
    sch_ce_eq_rx_batch / sch_ce_ml_rx_batch(y, h_ls, ce, algo, re_idx, mod, cfg, L, ...)   (the same
        from the DMRS least-squares estimate: phy.channel_estimate first)
    sch_uci_tx_batch(trblk, uci_bits, uci_plan, cfg, mod, cinit) -> sym[T, Gtotal/Qm]   (UCI on PUSCH:
    sch_uci_rx_batch(sym, noise_var, mod, uci_plan, cfg, L, cinit) -> (SchDecodeResult, dict)   uci.py)

Device tensors in, device tensors out, everything asynchronous on the current stream; torch only
allocates the buffers.  The per-transport-block drop-ins (nr_dlsch.DLSCHEncode,
nr_dlsch_decode.DLSCHDecode, nr_ulsch.*, nr_ulsch_decode.ULSCH_decoding) wrap these.
"""
from collections import namedtuple

from . import _lib

SchDecodeResult = namedtuple(
    "SchDecodeResult", "tb_ok tbblk llr_dn ck status iters cb_crc_ok tb_rem")


def sch_config(A, Qm, coderateby1024, NL, rv, TBS_LBRM, G):
    """Transport-block geometry (ldpc5g_sch_config).  TBS_LBRM > 0: DL-SCH limited-buffer Ncb
    (nr_dlsch.py:63-65); TBS_LBRM = 0: UL-SCH Ncb = N (nr_ulsch.py:55-58)."""
    cfg = _lib.SchCfg()
    _lib.call("ldpc5g_sch_config", A=int(A), Qm=int(Qm), coderateby1024=float(coderateby1024), NL=int(NL),
              rv=int(rv), TBS_LBRM=int(TBS_LBRM), G=int(G), cfg=_lib.ctypes.byref(cfg))
    return cfg


def cfg_from_codeblocks(C, K, K_apo, Zc, bgn, Qm, G, NL, rv, Ncb=None):
    """Configuration of ULSCH_encoding_ratematch(cbs, Zc, bgn, Qm, G_ULSCH, NL, rv)
    (nr_ulsch.py:37-70), which knows the codeblocks but not the TB size: only the codeblock and
    rate-matching fields are used by ldpc5g_sch_ratematch; A / B are made self-consistent."""
    from .nr_ldpc_ratematch import get_Er_ldpc, get_k0
    cfg = _lib.SchCfg()
    N = (66 if bgn == 1 else 50) * Zc
    Lcb = 24 if C > 1 else 0
    cbz = K_apo - Lcb
    B = C * cbz
    ltb = 24 if B - 24 > 3824 else 16
    Ncb = N if Ncb is None else Ncb
    Er = get_Er_ldpc(G, C, Qm, NL)
    E_lo, E_hi = min(Er), max(Er)
    vals = dict(A=B - ltb, B=B, tb_crc_poly=_lib.CRC_IDS["24A" if ltb == 24 else "16"], bgn=bgn,
                C=C, cbz=cbz, Lcb=Lcb, F=K - K_apo, K=K, K_apo=K_apo, Zc=Zc, N=N, Ncb=Ncb,
                k0=get_k0(Ncb, bgn, rv, Zc), Qm=Qm, NL=NL, rv=rv, E_lo=E_lo, E_hi=E_hi,
                c_switch=sum(1 for e in Er if e == E_lo) if E_lo != E_hi else C,
                G=G, E_total=sum(Er))
    for k, v in vals.items():
        setattr(cfg, k, int(v))
    return cfg


def crc_rows(bits, poly, nbits=None):
    """CRC remainders of the rows of a (R, n) int8 device tensor of 0/1 bits (ldpc5g_crc):
    nr_crc_encode's parity (crc.py:4-41, mask 0) as uint32 (int64 tensor), 0 for rows ending in
    a valid CRC (nr_crc_decode, crc.py:43-88)."""
    t = _lib.require_gpu()
    assert bits.dim() == 2 and bits.dtype == t.int8 and bits.stride(1) == 1
    n = bits.shape[1] if nbits is None else int(nbits)
    R = bits.shape[0]
    rem = t.empty((max(R, 1),), dtype=t.int32, device=bits.device)
    _lib.call("ldpc5g_crc", bits.device, bits=bits, ld=bits.stride(0), nbits=n, rows=R,
              poly=_lib.CRC_IDS[poly.upper()], rem=rem)
    return rem[:R].to(t.int64) & 0xFFFFFFFF


class SchWorkspace:
    """Device buffers of one batch shape (reused across calls of the bench / a TB stream)."""

    def __init__(self, cfg, T, device, dn_dtype=None):
        t = _lib.require_gpu()
        C, K, N = cfg.C, cfg.K, cfg.N
        Nf = N + 2 * cfg.Zc
        self.T = T
        self.ck = t.empty((T * C, K), dtype=t.int8, device=device)
        self.dn = t.empty((T * C, N), dtype=t.int8, device=device)
        self.tb_crc = t.empty((T,), dtype=t.int32, device=device)
        self.g = t.empty((T, max(cfg.E_total, 1)), dtype=t.int8, device=device)
        self.dec_ck = t.empty((T * C, Nf), dtype=t.int8, device=device)
        self.status = t.empty((T * C,), dtype=t.uint8, device=device)
        self.iters = t.empty((T * C,), dtype=t.int32, device=device)
        self.tbblk = t.empty((T, cfg.B), dtype=t.int8, device=device)
        self.cb_ok = t.empty((T * C,), dtype=t.uint8, device=device)
        self.tb_rem = t.empty((T,), dtype=t.int32, device=device)
        self.tb_ok = t.empty((T,), dtype=t.uint8, device=device)
        self.llr_dn = {}
        self.rx_llr = {}
        self.device = device

    def dn_buf(self, dtype, cfg):
        t = _lib.torch()
        if dtype not in self.llr_dn:
            self.llr_dn[dtype] = t.empty((self.T * cfg.C, cfg.N), dtype=dtype, device=self.device)
        return self.llr_dn[dtype]

    def rx_scratch(self, dtype, cfg):
        """Demodulated-LLR scratch (T, E_total) of the fused receive front end, for configurations
        whose codeblocks do not fit its LDS stage; allocated on first use."""
        t = _lib.torch()
        if dtype not in self.rx_llr:
            self.rx_llr[dtype] = t.empty((self.T, max(cfg.E_total, 1)), dtype=dtype, device=self.device)
        return self.rx_llr[dtype]


def sch_segment_batch(trblk, cfg, ws=None):
    """TB CRC + codeblock segmentation + CRC24B of T transport blocks (ldpc5g_sch_segment):
    returns (ck (T*C, K) int8 with -1 fillers, tb_crc (T,) int32)."""
    t = _lib.require_gpu()
    assert trblk.dim() == 2 and trblk.dtype == t.int8 and trblk.stride(1) == 1
    T = trblk.shape[0]
    assert trblk.shape[1] >= cfg.A
    ws = ws or SchWorkspace(cfg, T, trblk.device)
    _lib.call("ldpc5g_sch_segment", trblk.device, trblk=trblk, lda=trblk.stride(0),
              cfg=_lib.ctypes.byref(cfg), T=T, ck=ws.ck, tb_crc=ws.tb_crc)
    return ws.ck, ws.tb_crc


def sch_ratematch_batch(ck, cfg, T, ws=None):
    """LDPC encode + rate matching + concatenation of T*C codeblocks (ldpc5g_sch_ratematch):
    ck (T*C, K) int8 -> g (T, E_total) int8."""
    t = _lib.require_gpu()
    assert ck.dim() == 2 and ck.dtype == t.int8 and ck.shape == (T * cfg.C, cfg.K) and ck.is_contiguous()
    ws = ws or SchWorkspace(cfg, T, ck.device)
    _lib.call("ldpc5g_sch_ratematch", ck.device, ck=ck, cfg=_lib.ctypes.byref(cfg), T=T, dn=ws.dn,
              g=ws.g, ldg=ws.g.stride(0))
    return ws.g[:, :cfg.E_total]


def sch_encode_batch(trblk, cfg, ws=None):
    """DLSCHEncode / ULSCH encode of T transport blocks (ldpc5g_sch_encode): trblk (T, >=A) int8
    device tensor -> g (T, E_total) int8 device tensor (a view into the workspace)."""
    t = _lib.require_gpu()
    assert trblk.dim() == 2 and trblk.dtype == t.int8 and trblk.stride(1) == 1
    T = trblk.shape[0]
    assert trblk.shape[1] >= cfg.A
    ws = ws or SchWorkspace(cfg, T, trblk.device)
    _lib.call("ldpc5g_sch_encode", trblk.device, trblk=trblk, lda=trblk.stride(0), g=ws.g,
              ldg=ws.g.stride(0), cfg=_lib.ctypes.byref(cfg), T=T, ck=ws.ck, dn=ws.dn, tb_crc=ws.tb_crc)
    return ws.g[:, :cfg.E_total]


def sch_raterecover_batch(llr, cfg, harq_in=None, dn_dtype=None, ws=None):
    """Rate recovery + HARQ combining (ldpc5g_sch_raterecover): llr (T, >=E_total) float32/64
    -> llr_dn (T*C, N) of dn_dtype (default: llr's dtype)."""
    t = _lib.require_gpu()
    assert llr.dim() == 2 and llr.stride(1) == 1
    T = llr.shape[0]
    assert llr.shape[1] >= cfg.E_total
    dn_dtype = dn_dtype or llr.dtype
    ws = ws or SchWorkspace(cfg, T, llr.device)
    out = ws.dn_buf(dn_dtype, cfg)
    if harq_in is not None:
        assert harq_in.dtype == dn_dtype and harq_in.shape == out.shape and harq_in.is_contiguous()
    _lib.call("ldpc5g_sch_raterecover", llr.device, llr=llr, llr_dtype=_lib.dtype_id(llr.dtype, llr=True),
              ldg=llr.stride(0), cfg=_lib.ctypes.byref(cfg), T=T, harq_in=harq_in, llr_dn=out,
              dn_dtype=_lib.dtype_id(dn_dtype, llr=True))
    return out


def _tb_outputs(ws):
    """The TB reassembly outputs of ldpc5g_sch_tb_check and of the decode chains that end in it."""
    return dict(tbblk=ws.tbblk, ldb=ws.tbblk.stride(0), cb_crc_ok=ws.cb_ok, tb_rem=ws.tb_rem, tb_ok=ws.tb_ok)


def sch_tb_check_batch(ck, cfg, T, ws=None):
    """TB reassembly + CB / TB CRC checks (ldpc5g_sch_tb_check) of decoded ck (T*C, >=K_apo)."""
    t = _lib.require_gpu()
    assert ck.dim() == 2 and ck.dtype == t.int8 and ck.stride(1) == 1 and ck.shape[0] == T * cfg.C
    ws = ws or SchWorkspace(cfg, T, ck.device)
    _lib.call("ldpc5g_sch_tb_check", ck.device, ck=ck, ldc=ck.stride(0), cfg=_lib.ctypes.byref(cfg), T=T,
              **_tb_outputs(ws))
    return ws.tb_ok, ws.tbblk, ws.cb_ok, ws.tb_rem


def sch_decode_batch(llr, cfg, L, algo="min-sum", alpha=1.0, beta=0.0, schedule="flooding",
                     harq_in=None, dn_dtype=None, ws=None):
    """DLSCHDecode / ULSCH_decoding of T transport blocks on the GPU.

    llr: (T, >=E_total) float32/64 device tensor of demodulated LLRs.  schedule 'flooding' with
    float64 (the default dn_dtype for float64 llr) is bit-exact with the reference chain;
    'layered' needs float32.  algo 'BF' / 'BP' decode through the batched decoders.
    Returns SchDecodeResult(tb_ok (T,) uint8, tbblk (T, B) int8 — TB bits then its CRC,
    llr_dn (T*C, N) — the reference's new_LLr_dns, ck, status, iters, cb_crc_ok, tb_rem)."""
    t = _lib.require_gpu()
    assert algo in ["BF", "BP", "min-sum"]
    T = llr.shape[0]
    ws = ws or SchWorkspace(cfg, T, llr.device)
    if algo == "min-sum" and not beta >= 0:
        # the reference decodes each codeblock with nr_decode_ldpc (nr_dlsch_decode.py:91,
        # nr_ulsch_decode.py:92), which keeps min-sum's literal zero branches for beta < 0
        # (nr_ldpc_decode.py:186-225): the float64 sparse flooding kernel on the base graph, as
        # nr_decode_ldpc here.  beta < 0 therefore always runs the reference's float64 flooding
        # chain: a layered schedule or a float32 dn_dtype is refused, not silently ignored.
        from .nr_ldpc_decode import SparseGraph, _sparse_graph, decode_ldpc_batch
        assert schedule == "flooding", "beta < 0 decodes with the float64 flooding sparse kernel only"
        assert dn_dtype in (None, t.float64), "beta < 0: rate recovery must be float64 (dn_dtype)"
        dn_dtype = t.float64
        llr_dn = sch_raterecover_batch(llr, cfg, harq_in, dn_dtype, ws)
        x = t.zeros((T * cfg.C, cfg.N + 2 * cfg.Zc), dtype=t.float64, device=llr.device)
        x[:, 2 * cfg.Zc:] = llr_dn   # punctured systematic columns: LLR 0 (nr_ldpc_decode.py:43)
        g = _sparse_graph(("bg", cfg.bgn, cfg.Zc),
                          lambda: SparseGraph.from_base_graph(cfg.bgn, cfg.Zc, llr.device), llr.device)
        decode_ldpc_batch(x, g, L, algo, alpha, beta, out=(ws.dec_ck, ws.status, ws.iters))
        sch_tb_check_batch(ws.dec_ck, cfg, T, ws)
    elif algo == "min-sum":
        dn_dtype = dn_dtype or (t.float32 if schedule == "layered" else llr.dtype)
        out = ws.dn_buf(dn_dtype, cfg)
        if harq_in is not None:
            assert harq_in.dtype == dn_dtype and harq_in.shape == out.shape and harq_in.is_contiguous()
        assert llr.dim() == 2 and llr.stride(1) == 1 and llr.shape[1] >= cfg.E_total
        sched = {"flooding": _lib.FLOODING, "layered": _lib.LAYERED}[schedule]
        _lib.call("ldpc5g_sch_decode", llr.device, llr=llr, llr_dtype=_lib.dtype_id(llr.dtype, llr=True),
                  ldg=llr.stride(0), cfg=_lib.ctypes.byref(cfg), T=T, harq_in=harq_in, llr_dn=out,
                  dn_dtype=_lib.dtype_id(dn_dtype, llr=True), ck=ws.dec_ck, status=ws.status, iters=ws.iters,
                  L=int(L), alpha=float(alpha), beta=float(beta), schedule=sched, **_tb_outputs(ws))
        llr_dn = out
    else:
        from .nr_ldpc_decode import nr_decode_ldpc_batch
        dn_dtype = dn_dtype or (t.float32 if schedule == "layered" else llr.dtype)
        llr_dn = sch_raterecover_batch(llr, cfg, harq_in, dn_dtype, ws)
        nr_decode_ldpc_batch(llr_dn, cfg.Zc, cfg.bgn, L, algo, alpha, beta, "flooding",
                             out=(ws.dec_ck, ws.status, ws.iters), rate_matched=True)
        sch_tb_check_batch(ws.dec_ck, cfg, T, ws)
    return SchDecodeResult(ws.tb_ok, ws.tbblk, llr_dn, ws.dec_ck, ws.status, ws.iters, ws.cb_ok,
                           ws.tb_rem)


# ------------------------------------------------------------ fused receive front end
def _rx_args(sym, noise_var, mod, cfg, cinit, words, harq_in, dn_dtype, ws):
    """Checked inputs of the fused front end -> (T, workspace, the keyword arguments that
    ldpc5g_sch_demod_raterecover and ldpc5g_sch_rx_decode share, llr_dn).  The keywords hold the
    temporaries the launch reads (nv, w): the caller keeps them until the call returns."""
    from . import phy
    t = _lib.require_gpu()
    assert sym.dim() == 2 and sym.dtype in (t.complex64, t.complex128) and sym.stride(1) == 1
    assert phy.bits_per_symbol(mod) == cfg.Qm, "modulation does not match cfg.Qm"
    T, nsym = sym.shape[0], cfg.E_total // cfg.Qm
    assert sym.shape[1] >= nsym
    nv = noise_var if noise_var.dtype == t.float32 and noise_var.stride(1) == 1 else \
        noise_var.to(t.float32).contiguous()
    assert nv.dim() == 2 and nv.shape[0] == T and nv.shape[1] >= nsym
    w = words if words is not None else \
        (None if cinit is None else phy.prbs_words(cinit, cfg.E_total))
    if w is not None:
        assert w.dim() == 2 and w.shape[0] == T and w.stride(1) == 1 and w.shape[1] * 32 >= cfg.E_total
    ws = ws or SchWorkspace(cfg, T, sym.device)
    out = ws.dn_buf(dn_dtype, cfg)
    if harq_in is not None:
        assert harq_in.dtype == dn_dtype and harq_in.shape == out.shape and harq_in.is_contiguous()
    sdt = _lib.dtype_id(sym.dtype)
    need = _lib.call("ldpc5g_sch_rx_scratch_elems", cfg=_lib.ctypes.byref(cfg), mod=int(mod), sym_dtype=sdt)
    scr = None
    if need:   # a codeblock too large for the LDS stage: the two kernels through this scratch
        scr = ws.rx_scratch(t.float64 if int(mod) == 1 and sdt == _lib.F64 else t.float32, cfg)
    args = dict(sym=sym, sym_dtype=sdt, ldsym=sym.stride(0), noise_var=nv, ldnv=nv.stride(0), prbs=w,
                ldw=w.stride(0) if w is not None else 0, mod=int(mod), cfg=_lib.ctypes.byref(cfg), T=T,
                harq_in=harq_in, llr_dn=out, dn_dtype=_lib.dtype_id(dn_dtype, llr=True), llr_ws=scr,
                ldws=scr.stride(0) if scr is not None else 0)
    return T, ws, args, out


def sch_demod_raterecover_batch(sym, noise_var, mod, cfg, cinit=None, words=None, harq_in=None,
                                dn_dtype=None, ws=None):
    """Soft demodulation + descrambling + rate recovery + HARQ combining in one launch
    (ldpc5g_sch_demod_raterecover): sym (T, >= E_total/Qm) complex64/128 and noise_var (same
    shape, float32) device tensors, mod a phy.MOD_ID value with |mod| == cfg.Qm, cinit (T,) or
    precomputed phy.prbs_words `words` (neither: no descrambling) -> llr_dn (T*C, N) of dn_dtype
    (default float64 for complex128 symbols, float32 for complex64).  Bit for bit
    sch_raterecover_batch(phy.demod_descramble(...)), without the LLRs' trip through memory."""
    t = _lib.require_gpu()
    dn_dtype = dn_dtype or (t.float64 if sym.dtype == t.complex128 else t.float32)
    T, ws, args, out = _rx_args(sym, noise_var, mod, cfg, cinit, words, harq_in, dn_dtype, ws)
    _lib.call("ldpc5g_sch_demod_raterecover", sym.device, **args)
    return out


def sch_rx_batch(sym, noise_var, mod, cfg, L, algo="min-sum", alpha=1.0, beta=0.0,
                 schedule="flooding", cinit=None, words=None, harq_in=None, dn_dtype=None, ws=None,
                 fused=True):
    """The receive chain of T transport blocks from equalised symbols to TB bits (the tail of the
    reference's RX_process, nr_pdsch.py:245-281, and DLSCHDecode / ULSCH_decoding): demodulate,
    descramble, rate-recover (+ HARQ), decode, CRC.  Arguments as sch_demod_raterecover_batch and
    sch_decode_batch; dn_dtype defaults to float64 for 'flooding' and float32 for 'layered'.
    fused=True runs the front end as one launch (ldpc5g_sch_rx_decode); fused=False runs
    phy.demod_descramble then sch_decode_batch.  Both give the same SchDecodeResult."""
    from . import phy
    t = _lib.require_gpu()
    assert algo in ["BF", "BP", "min-sum"]
    sparse = algo == "min-sum" and not beta >= 0   # see sch_decode_batch
    if sparse:
        assert schedule == "flooding", "beta < 0 decodes with the float64 flooding sparse kernel only"
        assert dn_dtype in (None, t.float64), "beta < 0: rate recovery must be float64 (dn_dtype)"
    dn_dtype = dn_dtype or (t.float32 if schedule == "layered" else t.float64)
    if not fused:
        nsym = cfg.E_total // cfg.Qm
        f64 = int(mod) == 1 and sym.dtype == t.complex128   # demod_bpsk.py:9 keeps float64
        llr = phy.demod_descramble(sym[:, :nsym], noise_var[:, :nsym], mod, cinit, words,
                                   llr_dtype=t.float64 if f64 else None)
        return sch_decode_batch(llr, cfg, L, algo, alpha, beta, schedule, harq_in, dn_dtype, ws)
    if algo == "min-sum" and not sparse:
        T, ws, args, llr_dn = _rx_args(sym, noise_var, mod, cfg, cinit, words, harq_in, dn_dtype, ws)
        sched = {"flooding": _lib.FLOODING, "layered": _lib.LAYERED}[schedule]
        _lib.call("ldpc5g_sch_rx_decode", sym.device, **args, ck=ws.dec_ck, status=ws.status, iters=ws.iters,
                  L=int(L), alpha=float(alpha), beta=float(beta), schedule=sched, **_tb_outputs(ws))
    else:
        T = sym.shape[0]
        ws = ws or SchWorkspace(cfg, T, sym.device)
        llr_dn = sch_demod_raterecover_batch(sym, noise_var, mod, cfg, cinit, words, harq_in, dn_dtype, ws)
        if sparse:
            from .nr_ldpc_decode import SparseGraph, _sparse_graph, decode_ldpc_batch
            x = t.zeros((T * cfg.C, cfg.N + 2 * cfg.Zc), dtype=t.float64, device=sym.device)
            x[:, 2 * cfg.Zc:] = llr_dn   # punctured systematic columns: LLR 0 (nr_ldpc_decode.py:43)
            g = _sparse_graph(("bg", cfg.bgn, cfg.Zc),
                              lambda: SparseGraph.from_base_graph(cfg.bgn, cfg.Zc, sym.device), sym.device)
            decode_ldpc_batch(x, g, L, algo, alpha, beta, out=(ws.dec_ck, ws.status, ws.iters))
        else:
            from .nr_ldpc_decode import nr_decode_ldpc_batch
            nr_decode_ldpc_batch(llr_dn, cfg.Zc, cfg.bgn, L, algo, alpha, beta, "flooding",
                                 out=(ws.dec_ck, ws.status, ws.iters), rate_matched=True)
        sch_tb_check_batch(ws.dec_ck, cfg, T, ws)
    return SchDecodeResult(ws.tb_ok, ws.tbblk, llr_dn, ws.dec_ck, ws.status, ws.iters, ws.cb_ok,
                           ws.tb_rem)


# ------------------------------------------------------------ UCI on PUSCH
def sch_uci_tx_batch(trblk, uci_bits, uci_plan, cfg, mod, cinit=None, words=None, ws=None):
    """The transmit chain of T PUSCH slots that carry UCI (ULSCHandUCIProcess, nr_pusch_uci.py:52-107,
    then nr_pusch_process.py:14-30): trblk (T, >= A) int8 (None when the plan holds no UL-SCH), uci_bits a
    dict with the payloads "ack" / "csi1" / "csi2" as (T, O) int8 for every stream the plan holds, cfg the
    UL-SCH's sch_config with G = G_ULSCH -> symbols (T, Gtotal / Qm) complex64, scrambled by cinit (T,) or
    precomputed phy.prbs_words of Gtotal bits."""
    from . import phy, uci
    t = _lib.require_gpu()
    p = uci_plan
    assert phy.bits_per_symbol(mod) == p.Qm, "modulation does not match the plan's Qm"
    assert cinit is not None or words is not None, "cinit or words: the placeholders are defined by the scrambler"
    g = {n: None for n in uci.STREAMS}
    if p.lens["ulsch"]:
        assert cfg.E_total == p.lens["ulsch"] and cfg.Qm == p.Qm, "cfg must be the UL-SCH's configuration with G = G_ULSCH"
        g["ulsch"] = sch_encode_batch(trblk, cfg, ws)
    for n, A in (("ack", p.OACK), ("csi1", p.OCSI1), ("csi2", p.OCSI2)):
        if A:
            b = uci_bits[n]
            assert b.dim() == 2 and b.dtype == t.int8 and b.shape[1] == A, f"uci_bits[{n!r}]: (T, {A}) int8"
            g[n] = uci.encode(b, p.lens[n], p.Qm)
    return uci.scramble_modulate(uci.mux(p, g["ulsch"], g["ack"], g["csi1"], g["csi2"]), mod, cinit, words)


def sch_uci_rx_batch(sym, noise_var, mod, uci_plan, cfg, L, cinit=None, words=None, algo="min-sum", alpha=1.0, beta=0.0,
                     schedule="flooding", harq_in=None, dn_dtype=None, ws=None, uci_L=8, erase_punctured=True):
    """The receive chain of T PUSCH slots that carry UCI, from equalised symbols (T, >= Gtotal / Qm) and
    their noise variances: phy.demod_descramble without descrambling, uci.demux in descrambling mode
    (placeholders by their rule, punctured UL-SCH LLRs erased unless erase_punctured=False),
    sch_decode_batch on the UL-SCH stream (cfg: its sch_config with G = G_ULSCH; skipped when the plan
    holds no UL-SCH) and uci.decode on every UCI stream with list size uci_L.
    Returns (SchDecodeResult or None, dict): the dict holds "ack" / "csi1" / "csi2" -> (T, O) int8 bits and
    "<name>_crc_ok" -> (T,) bool for payloads of 12 bits and more (None below), for the streams present."""
    from . import phy, uci
    t = _lib.require_gpu()
    p = uci_plan
    assert phy.bits_per_symbol(mod) == p.Qm, "modulation does not match the plan's Qm"
    assert cinit is not None or words is not None, "cinit or words: the placeholders are defined by the scrambler"
    nsym = p.Gtotal // p.Qm
    assert sym.dim() == 2 and sym.shape[1] >= nsym and noise_var.shape[1] >= nsym
    f64 = int(mod) == 1 and sym.dtype == t.complex128   # demod_bpsk.py:9 keeps float64
    llr = phy.demod_descramble(sym[:, :nsym], noise_var[:, :nsym], mod, llr_dtype=t.float64 if f64 else None)
    s = uci.demux(p, llr, cinit, words, erase_punctured)
    res = None
    if p.lens["ulsch"]:
        assert cfg.E_total == p.lens["ulsch"] and cfg.Qm == p.Qm, "cfg must be the UL-SCH's configuration with G = G_ULSCH"
        dn_dtype = dn_dtype or (t.float32 if schedule == "layered" else t.float64)
        res = sch_decode_batch(s.ulsch, cfg, L, algo, alpha, beta, schedule, harq_in, dn_dtype, ws)
    out = {}
    for n, A in (("ack", p.OACK), ("csi1", p.OCSI1), ("csi2", p.OCSI2)):
        if A:
            out[n], out[n + "_crc_ok"] = uci.decode(getattr(s, n), A, p.lens[n], p.Qm, uci_L)
    return res, out


def sch_eq_rx_batch(y, h, cov, algo, re_idx, mod, cfg, L, re_per_cov=12, **kw):
    """The body of the reference's RX_process from (pdsch_resource, H_result, cov_m) to the
    transport block (nr_pdsch.py:245-281): phy.equalize (ZF / ZF-IRC / MMSE / MMSE-IRC per data
    resource element) followed by sch_rx_batch, whose keyword arguments all pass through.  y, h,
    cov, algo, re_idx, re_per_cov as phy.equalize; mod, cfg, L as sch_rx_batch.  The data REs must
    carry exactly the transport block: nre * NL * Qm == cfg.G."""
    from . import phy
    nre = re_idx.shape[0] if re_idx is not None else y.shape[1]
    NL = h.shape[3]
    assert nre * NL * phy.bits_per_symbol(mod) == cfg.G, \
        f"nre*NL*Qm = {nre}*{NL}*{phy.bits_per_symbol(mod)} != G = {cfg.G}"
    sym, nv = phy.equalize(y, h, cov, algo, re_idx, re_per_cov)
    return sch_rx_batch(sym, nv, mod, cfg, L, **kw)


def sch_ml_rx_batch(y, h, cov, algo, re_idx, mod, cfg, L, re_per_cov=12, cinit=None, **kw):
    """sch_eq_rx_batch for the maximum-likelihood detectors of channel_equ_and_demod
    (nr_channel_eq.py:27-46), which emit LLRs themselves: phy.ml_detect (descrambling with cinit
    fused) followed by sch_decode_batch, whose keyword arguments all pass through (its `algo` is
    given as dec_algo=).  y, h, cov, algo, re_idx, re_per_cov as phy.ml_detect; mod, cfg, L as
    sch_decode_batch.  The LLRs are float32 for schedule="layered" and float64 otherwise.  The
    data REs must carry exactly the transport block: nre * NL * Qm == cfg.G."""
    from . import phy
    t = _lib.require_gpu()
    nre = re_idx.shape[0] if re_idx is not None else y.shape[1]
    NL = h.shape[3]
    assert nre * NL * phy.bits_per_symbol(mod) == cfg.G, \
        f"nre*NL*Qm = {nre}*{NL}*{phy.bits_per_symbol(mod)} != G = {cfg.G}"
    if "dec_algo" in kw:
        kw["algo"] = kw.pop("dec_algo")
    llr_dtype = t.float32 if kw.get("schedule") == "layered" else t.float64
    llr = phy.ml_detect(y, h, cov, mod, algo, re_idx, re_per_cov, cinit=cinit, llr_dtype=llr_dtype)
    return sch_decode_batch(llr, cfg, L, **kw)


def _ce_stage(y, h_ls, ce):
    """channel_estimate (and, with to_comp, the data REs' compensation) for the two chains below:
    (y (T, R, Nr), h, cov), everything on the device and on the current stream."""
    from . import phy
    ce = dict(ce)
    ce_algo = ce.pop("algo")
    to_comp = bool(ce.get("to_comp", False))
    T, R, Nr = y.shape
    N, D = h_ls.shape[2], int(ce.get("re_distance", 4))
    assert R == 14 * N * D, f"y has R = {R} resource elements, the slot has 14*N*D = {14 * N * D}"
    if to_comp:
        h, cov, extra = phy.channel_estimate(h_ls, algo=ce_algo, want=("to_avg",), **ce)
        y = phy.to_compensate(y.reshape(T, 14, N * D, Nr), extra["to_avg"], ce["scs"]).view(T, R, Nr)
    else:
        h, cov = phy.channel_estimate(h_ls, algo=ce_algo, **ce)
    return y, h, cov


def sch_ce_eq_rx_batch(y, h_ls, ce, algo, re_idx, mod, cfg, L, **kw):
    """The reference's receiver from (pdsch_resource, H_LS) to the transport block:
    phy.channel_estimate, then sch_eq_rx_batch on its h and cov, with no host round trip between
    the stages.  y: (T, 14*N*D, Nr) the slot's resource grid; h_ls: (T, S, N, Nr, Nt); ce: the
    channel estimator's arguments as a dict (sym_map, algo, scs, eRB, l_left_ns, l_right_ns and
    optionally re_distance, num_cdm_groups, to_comp — with to_comp the data REs are compensated
    too, process_pdsch_data); algo, re_idx, mod, cfg, L and the keyword arguments as
    sch_eq_rx_batch (re_per_cov is 12)."""
    y, h, cov = _ce_stage(y, h_ls, ce)
    return sch_eq_rx_batch(y, h, cov, algo, re_idx, mod, cfg, L, **kw)


def sch_ce_ml_rx_batch(y, h_ls, ce, algo, re_idx, mod, cfg, L, **kw):
    """sch_ce_eq_rx_batch for the maximum-likelihood detectors: phy.channel_estimate, then
    sch_ml_rx_batch."""
    y, h, cov = _ce_stage(y, h_ls, ce)
    return sch_ml_rx_batch(y, h, cov, algo, re_idx, mod, cfg, L, **kw)


def _slot_chain_params(pdsch_config, algo):
    """sch_slot_rx_batch's refusals, which come before any GPU work; phy._slot_params' fields."""
    from . import phy
    assert algo in _lib.EQ_ALGO or algo in _lib.ML_ALGO, \
        f"algo {algo!r}: one of {sorted(_lib.EQ_ALGO) + sorted(_lib.ML_ALGO)}"
    return phy._slot_params(pdsch_config)


def _tp_chain_params(pusch_config, algo, base_seq):
    """sch_pusch_tp_rx_batch's refusals, which come before any GPU work; phy._tp_params' fields."""
    from . import phy
    if algo in _lib.ML_ALGO:
        raise NotImplementedError(f"algo {algo!r}: with transform precoding the reference demodulates after the "
                                  "de-spreading IDFT and throws the ML detectors' LLRs away (nr_pusch.py:178-194); "
                                  f"use one of {sorted(_lib.EQ_ALGO)}")
    assert algo in _lib.EQ_ALGO, f"algo {algo!r}: one of {sorted(_lib.EQ_ALGO)}"
    return phy._tp_params(pusch_config, base_seq)


def sch_slot_rx_batch(grid, slots, pdsch_config, ce, algo, mod, cfg, L, re_idx=None, **kw):
    """The reference's receiver from the slot grid to the transport block — Pdsch.H_LS_est,
    NrChannelEstimation.channel_est and Pdsch.RX_process (nr_pdsch.py:212-284, 345-352) — for T
    slots: phy.slot_frontend, then the channel estimator, then sch_eq_rx_batch (algo "ZF", "ZF-IRC",
    "MMSE", "MMSE-IRC") or sch_ml_rx_batch (the ten ML names), all on the device and on the current
    stream.  grid: (T, Nr, 14*carrier_re) complex64 / complex128 device tensor; slots: (T,) int32
    device tensor; pdsch_config: the reference's dict; ce: the channel estimator's arguments as in
    sch_ce_eq_rx_batch, whose sym_map and num_cdm_groups are filled in from pdsch_config; mod, cfg,
    L and the keyword arguments as the chosen chain's; re_idx: phy.slot_data_re_idx_device's tensor
    (uploaded here, once per call, when it is not given).  The data REs (phy.slot_data_re_idx) must
    carry exactly the transport block: nre * NL * Qm == cfg.G."""
    from . import phy
    p = _slot_chain_params(pdsch_config, algo)
    h_ls, y = phy.slot_frontend(grid, slots, pdsch_config)
    if re_idx is None:
        re_idx = phy.slot_data_re_idx_device(pdsch_config, grid.device)
    ce = dict(ce, sym_map=p["symlist"], num_cdm_groups=p["cdm"])
    y, h, cov = _ce_stage(y, h_ls, ce)
    if algo in _lib.EQ_ALGO:
        return sch_eq_rx_batch(y, h, cov, algo, re_idx, mod, cfg, L, **kw)
    return sch_ml_rx_batch(y, h, cov, algo, re_idx, mod, cfg, L, **kw)


def sch_pusch_tp_rx_batch(grid, slots, pusch_config, ce, algo, mod, cfg, L, re_idx=None, base_seq=None, **kw):
    """sch_slot_rx_batch for a pusch_config with nTransPrecode = 1 (NrPUSCH.H_LS_est,
    NrChannelEstimation.channel_est and NrPUSCH.RX_process with its de-spreading branch,
    nr_pusch.py:116-219): phy.pusch_tp_frontend, the channel estimator, phy.equalize,
    phy.transform_precode(inverse=True) on the equalised symbols of every data symbol (:184-191) and
    sch_rx_batch, all on the device and on the current stream.  The noise variances go to the
    demodulator unchanged, per RE, as nr_pusch.py:190 has them.  algo: "ZF", "ZF-IRC", "MMSE" or
    "MMSE-IRC"; the ML names are refused, the reference discards their LLRs on this branch (:178).
    re_idx: the device tensor of phy.pusch_tp_data_re_idx(pusch_config)[0] (uploaded here when not
    given); base_seq as phy.pusch_tp_frontend; everything else as sch_slot_rx_batch."""
    from . import phy
    p = _tp_chain_params(pusch_config, algo, base_seq)
    h_ls, y = phy.pusch_tp_frontend(grid, slots, pusch_config, base_seq=base_seq)
    t = _lib.torch()
    if re_idx is None:
        re_idx = t.from_numpy(phy.pusch_tp_data_re_idx(pusch_config)[0]).to(grid.device)
    nre = re_idx.shape[0]
    assert nre * phy.bits_per_symbol(mod) == cfg.G, f"nre*Qm = {nre}*{phy.bits_per_symbol(mod)} != G = {cfg.G}"
    ce = dict(ce, sym_map=p["symlist"], num_cdm_groups=p["cdm"])
    y, h, cov = _ce_stage(y, h_ls, ce)
    sym, nv = phy.equalize(y, h, cov, algo, re_idx)
    phy.transform_precode(sym, p["rb_size"], inverse=True, out=sym)
    return sch_rx_batch(sym, nv, mod, cfg, L, **kw)


def sch_td_rx_batch(td, slots, config, carrier, ce, algo, mod, cfg, L, **kw):
    """The reference's receiver from time-domain samples to the transport block for T slots:
    Rx_low_phy (rx_lowphy_process.py:35-98) by phy.ofdm_demod, then sch_slot_rx_batch — or, when
    config["nTransPrecode"] == 1, sch_pusch_tp_rx_batch — all on the device and on the current
    stream, with no host round trip.  td: (T, Nr, 15*nfft) complex64 / complex128 device tensor, any
    strides on the first two dimensions; carrier: the reference's carrier_config (its "scs", "BW" and
    "carrier_frequency_in_mhz" are read); config: the pdsch_config or pusch_config; everything else,
    the keyword arguments included, as the chain's that runs.  Antennas keep their order (the
    reference's Rx_low_phy rolls them, which no receiver here depends on)."""
    from . import nr_slot, phy
    scs = carrier["scs"]
    prbs = nr_slot.get_carrier_prb_size(scs, carrier["BW"])
    tp = config.get("nTransPrecode", 0) == 1
    if tp:   # the chain's own refusals come before any GPU work
        _tp_chain_params(config, algo, kw.get("base_seq"))
    else:
        _slot_chain_params(config, algo)
    grid = phy.ofdm_demod(td, scs, prbs, carrier.get("carrier_frequency_in_mhz", 0))
    chain = sch_pusch_tp_rx_batch if tp else sch_slot_rx_batch
    return chain(grid, slots, config, ce, algo, mod, cfg, L, **kw)


# ------------------------------------------------------------ per-TB configurations (multi)
SchMultiResult = namedtuple(
    "SchMultiResult", "tb_ok tbblk llr_dn ck status iters cb_crc_ok tb_rem rows")


def multi_layout(cfgs):
    """Workspace geometry of a batch whose transport blocks each have their own configuration
    (ldpc5g_sch_multi_sizes): dict(ck, dn, dck, ncb, max_A, max_B, max_E) plus `rows`: per TB
    (first codeblock, C, dn element offset, N, decoder-ck offset, Nf) in workspace order."""
    T = len(cfgs)
    arr = (_lib.SchCfg * max(T, 1))(*cfgs)
    sizes = (_lib.ctypes.c_int64 * 7)()
    _lib.call("ldpc5g_sch_multi_sizes", cfgs=arr, T=T, sizes=sizes)
    rows, cb, dn, dck = [], 0, 0, 0
    for c in cfgs:
        nf = (68 if c.bgn == 1 else 52) * c.Zc
        rows.append((cb, c.C, dn, c.N, dck, nf))
        cb, dn, dck = cb + c.C, dn + c.C * c.N, dck + c.C * nf
    return dict(ck=sizes[0], dn=sizes[1], dck=sizes[2], ncb=sizes[3], max_A=sizes[4],
                max_B=sizes[5], max_E=sizes[6], rows=rows, arr=arr)


def sch_encode_multi(trblk, cfgs):
    """DLSCHEncode / UL-SCH encode of T transport blocks with per-TB configurations in one call
    (ldpc5g_sch_encode_multi).  trblk: (T, >= max A) int8 device tensor (TB t uses A_t bits).
    Returns g (T, max E_total) int8 (TB t's first E_total_t entries valid)."""
    t = _lib.require_gpu()
    T = len(cfgs)
    lay = multi_layout(cfgs)
    assert trblk.dim() == 2 and trblk.shape[0] == T and trblk.dtype == t.int8 and trblk.stride(1) == 1
    assert trblk.shape[1] >= lay["max_A"]
    dev = trblk.device
    g = t.empty((T, max(lay["max_E"], 1)), dtype=t.int8, device=dev)
    ck = t.empty((max(lay["ck"], 1),), dtype=t.int8, device=dev)
    dn = t.empty((max(lay["dn"], 1),), dtype=t.int8, device=dev)
    crc = t.empty((max(T, 1),), dtype=t.int32, device=dev)
    _lib.call("ldpc5g_sch_encode_multi", dev, trblk=trblk, lda=trblk.stride(0), g=g, ldg=g.stride(0),
              cfgs=lay["arr"], T=T, ck=ck, dn=dn, tb_crc=crc)
    return g


def sch_raterecover_multi(llr, cfgs, harq_in=None, dn_dtype=None, out=None, lay=None):
    """Rate recovery (raterecover_ldpc, py5gphy/ldpc/nr_ldpc_raterecover.py:6-65) of T transport
    blocks with per-TB configurations in ONE launch (ldpc5g_sch_raterecover_multi).
    llr: (T, >= max E_total) float32/64 device tensor.  Returns the flat llr_dn (codeblock rows of
    N_t, TB after TB; multi_layout(cfgs)["rows"] locates them) of dn_dtype (default llr's)."""
    t = _lib.require_gpu()
    T = len(cfgs)
    lay = lay or multi_layout(cfgs)
    assert llr.dim() == 2 and llr.shape[0] == T and llr.stride(1) == 1 and llr.shape[1] >= lay["max_E"]
    dn_dtype = dn_dtype or llr.dtype
    if out is None:
        out = t.empty((max(lay["dn"], 1),), dtype=dn_dtype, device=llr.device)
    assert out.dtype == dn_dtype and out.numel() >= lay["dn"] and out.is_contiguous()
    if harq_in is not None:
        assert harq_in.dtype == dn_dtype and harq_in.numel() >= lay["dn"] and harq_in.is_contiguous()
    _lib.call("ldpc5g_sch_raterecover_multi", llr.device, llr=llr, llr_dtype=_lib.dtype_id(llr.dtype, llr=True),
              ldg=llr.stride(0), cfgs=lay["arr"], T=T, harq_in=harq_in, llr_dn=out,
              dn_dtype=_lib.dtype_id(dn_dtype, llr=True))
    return out


class SchRaterecoverPlan:
    """sch_raterecover_multi for repeated use: the per-TB geometry is validated and copied to the
    device once (ldpc5g_sch_multi_plan); each call only launches the kernel
    (ldpc5g_sch_raterecover_multi_plan), asynchronously on the current stream."""

    def __init__(self, cfgs, device):
        t = _lib.require_gpu()
        self.lay = multi_layout(cfgs)
        self.T = len(cfgs)
        n = _lib.call("ldpc5g_sch_multi_plan", cfgs=self.lay["arr"], T=self.T, plan=None, plan_bytes=0)
        self.host = t.empty((max(n, 1),), dtype=t.uint8, pin_memory=True)
        _lib.call("ldpc5g_sch_multi_plan", cfgs=self.lay["arr"], T=self.T, plan=self.host, plan_bytes=n)
        self.dev = self.host.to(device, non_blocking=True)

    def __call__(self, llr, out, harq_in=None):
        assert llr.dim() == 2 and llr.shape[0] == self.T and llr.stride(1) == 1
        assert llr.shape[1] >= self.lay["max_E"] and out.is_contiguous() and out.numel() >= self.lay["dn"]
        if harq_in is not None:
            assert harq_in.dtype == out.dtype and harq_in.numel() >= self.lay["dn"] and harq_in.is_contiguous()
        _lib.call("ldpc5g_sch_raterecover_multi_plan", llr.device, plan_dev=self.dev, plan_host=self.host, llr=llr,
                  llr_dtype=_lib.dtype_id(llr.dtype, llr=True), ldg=llr.stride(0), harq_in=harq_in, llr_dn=out,
                  dn_dtype=_lib.dtype_id(out.dtype, llr=True))
        return out


def sch_decode_multi(llr, cfgs, L, alpha=1.0, beta=0.0, schedule="flooding", harq_in=None,
                     dn_dtype=None):
    """DLSCHDecode / ULSCH_decoding of T transport blocks with per-TB configurations in one call
    (ldpc5g_sch_decode_multi): rate recovery, every codeblock decoded by the mixed-Zc decoder,
    TB reassembly and CRCs.  llr: (T, >= max E_total) float32/64 device tensor.
    Returns SchMultiResult(tb_ok (T,), tbblk (T, max B) — TB t's first B_t bits, llr_dn flat
    (the HARQ buffers new_LLr_dns of every TB, rows[t] locates them), ck flat, status, iters,
    cb_crc_ok (per codeblock), tb_rem, rows)."""
    t = _lib.require_gpu()
    T = len(cfgs)
    lay = multi_layout(cfgs)
    assert llr.dim() == 2 and llr.shape[0] == T and llr.stride(1) == 1 and llr.shape[1] >= lay["max_E"]
    dn_dtype = dn_dtype or (t.float32 if schedule == "layered" else llr.dtype)
    dev = llr.device
    llr_dn = t.empty((max(lay["dn"], 1),), dtype=dn_dtype, device=dev)
    if harq_in is not None:
        assert harq_in.dtype == dn_dtype and harq_in.numel() >= lay["dn"] and harq_in.is_contiguous()
    ck = t.empty((max(lay["dck"], 1),), dtype=t.int8, device=dev)
    n = max(lay["ncb"], 1)
    status = t.empty((n,), dtype=t.uint8, device=dev)
    iters = t.empty((n,), dtype=t.int32, device=dev)
    cb_ok = t.empty((n,), dtype=t.uint8, device=dev)
    tbblk = t.empty((T, max(lay["max_B"], 1)), dtype=t.int8, device=dev)
    tb_rem = t.empty((max(T, 1),), dtype=t.int32, device=dev)
    tb_ok = t.empty((max(T, 1),), dtype=t.uint8, device=dev)
    sched = {"flooding": _lib.FLOODING, "layered": _lib.LAYERED}[schedule]
    _lib.call("ldpc5g_sch_decode_multi", dev, llr=llr, llr_dtype=_lib.dtype_id(llr.dtype, llr=True),
              ldg=llr.stride(0), cfgs=lay["arr"], T=T, harq_in=harq_in, llr_dn=llr_dn,
              dn_dtype=_lib.dtype_id(dn_dtype, llr=True), ck=ck, status=status, iters=iters, L=int(L),
              alpha=float(alpha), beta=float(beta), schedule=sched, tbblk=tbblk, ldb=tbblk.stride(0),
              cb_crc_ok=cb_ok, tb_rem=tb_rem, tb_ok=tb_ok)
    return SchMultiResult(tb_ok[:T], tbblk, llr_dn, ck, status, iters, cb_ok, tb_rem, lay["rows"])
