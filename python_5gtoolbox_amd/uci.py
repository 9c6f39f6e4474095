"""Batched UCI on PUSCH on device tensors (TS 38.212 §5.3.3, §6.2.7, §6.3.1, §6.3.2.4).

    rm = uci.rm_info(pusch_config, dmrs_symlist, ULSCH_size, Qm, coderateby1024, Gtotal)   # host, the reference's dict
    p = uci.plan(pusch_config, dmrs_symlist, rm, Qm)           # host-built §6.2.7 map, cached, uploaded once per device
    g_ack = uci.encode(bits, E, Qm)                            # [T, A] int8 -> [T, E] int8 (placeholders -1 / -2)
    g_seq = uci.mux(p, g_ulsch, g_ack, g_csi1, g_csi2)         # [T, Gtotal] int8
    sym = uci.scramble_modulate(g_seq, mod, cinit)             # [T, Gtotal / Qm] complex64
    s = uci.demux(p, llr, cinit=..., erase_punctured=True)     # UciStreams(ulsch, ack, csi1, csi2) of llr's dtype
    bits, crc_ok = uci.decode(s.ack, A, E, Qm, L=8)            # crc_ok is None for A <= 11

Payloads of 1..11 bits use the small-block kernels, 12 and more the polar codec (polar.py) with the CRC,
segmentation and settings of encode_uci_on_ulsch (nr_pusch_uci.py:16-49).  There is no CPU path.
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np

from . import _lib, phy, polar

UciStreams = namedtuple("UciStreams", "ulsch ack csi1 csi2")
RM_KEYS = ("Euci_ack", "Qbar_ACK", "Euci_CSI1", "Qbar_CSI1", "Euci_CSI2", "Qbar_CSI2", "Euci_ackrvd", "Qbar_ACKrvd",
           "G_ULSCH")
STREAMS = ("ulsch", "ack", "csi1", "csi2")
ULSCH, ACK, CSI1, CSI2, NONE = 0, 1, 2, 3, 4
DATA, X, Y = 0, 1, 2
_HDR = ("magic", "version", "bytes", "Gtotal", "Qm", "NL", "OACK", "OCSI1", "OCSI2", "EnableULSCH", "len_ulsch", "len_ack",
        "len_csi1", "len_csi2", "off_fwd", "off_inv", "n_punct", "n_inv", "n_x", "n_y")


def _payloads(cfg):
    return (int(cfg["EnableACK"]) * int(cfg["NumACKBits"]), int(cfg["EnableCSI1"]) * int(cfg["NumCSI1Bits"]),
            int(cfg["EnableCSI2"]) * int(cfg["NumCSI2Bits"]))


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))


def rm_info(pusch_config, dmrs_symlist, ULSCH_size, Qm, coderateby1024, Gtotal):
    """getULSCH_RM_info (nr_ulsch_info.py:6-170) on the host (ldpc5g_uci_rm_info): the reference's dict;
    AssertionError with the library's message where the reference asserts.  A disabled payload counts as
    0 bits everywhere (the reference reads NumACKBits / NumCSI2Bits unmasked in three places)."""
    c = pusch_config
    oack, ocsi1, ocsi2 = _payloads(c)
    d = _i32(dmrs_symlist)
    out = np.zeros(9, np.int64)
    _lib.call("ldpc5g_uci_rm_info", RBSize=int(c["ResAlloType1"]["RBSize"]), StartSymbolIndex=int(c["StartSymbolIndex"]),
              NrOfSymbols=int(c["NrOfSymbols"]), dmrs_symlist=d, num_dmrs=d.size, NL=int(c["num_of_layers"]), Qm=int(Qm),
              coderateby1024=float(coderateby1024), ULSCH_size=int(ULSCH_size), EnableULSCH=int(c["EnableULSCH"]), OACK=oack,
              OCSI1=ocsi1, OCSI2=ocsi2, I_HARQ_ACK_offset=int(c["I_HARQ_ACK_offset"]), I_CSI1offset=int(c["I_CSI1offset"]),
              I_CSI2offset=int(c["I_CSI2offset"]), UCIScaling=float(c["UCIScaling"]), Gtotal=int(Gtotal), out=out)
    return {k: int(v) for k, v in zip(RM_KEYS, out)}


class Plan:
    """Host copy of a ldpc5g_uci_map_plan blob plus one device copy per device."""

    def __init__(self, blob):
        self.blob = blob
        hdr = blob[:128].view(np.int32)
        for i, n in enumerate(_HDR):
            setattr(self, n, int(hdr[i]))
        self.lens = {n: getattr(self, "len_" + n) for n in STREAMS}
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

    def expand(self):
        """The map on the host: dict(stream, index, kind, punct: [Gtotal]; inv / inv_kind / inv_punct: per stream)."""
        fwd = self.blob[self.off_fwd:self.off_fwd + 4 * self.Gtotal].view(np.uint32)
        inv = self.blob[self.off_inv:self.off_inv + 4 * self.n_inv].view(np.uint32)
        out = {"stream": ((fwd >> 24) & 7).astype(np.int8), "index": (fwd & 0xFFFFFF).astype(np.int64),
               "kind": ((fwd >> 27) & 3).astype(np.int8), "punct": ((fwd >> 29) & 1).astype(bool),
               "inv": {}, "inv_kind": {}, "inv_punct": {}}
        off = 0
        for n in STREAMS:
            e = inv[off:off + self.lens[n]]
            off += self.lens[n]
            out["inv"][n] = (e & 0xFFFFFF).astype(np.int64)
            out["inv_kind"][n] = ((e >> 27) & 3).astype(np.int8)
            out["inv_punct"][n] = ((e >> 29) & 1).astype(bool)
        return out


def plan_blob(RBSize, StartSymbolIndex, NrOfSymbols, dmrs_symlist, NumCDMGroupsWithoutData, NL, Qm, OACK, OCSI1, OCSI2,
              EnableULSCH, Euci_ack, Euci_CSI1, Euci_CSI2, Euci_ackrvd, G_ULSCH, Gtotal, frequency_hopping=0):
    """The plan's bytes (numpy uint8); AssertionError with the library's message for refused arguments."""
    d = _i32(dmrs_symlist)
    args = dict(RBSize=int(RBSize), StartSymbolIndex=int(StartSymbolIndex), NrOfSymbols=int(NrOfSymbols), dmrs_symlist=d,
                num_dmrs=d.size, NumCDMGroupsWithoutData=int(NumCDMGroupsWithoutData), NL=int(NL), Qm=int(Qm), OACK=int(OACK),
                OCSI1=int(OCSI1), OCSI2=int(OCSI2), EnableULSCH=int(EnableULSCH), frequency_hopping=int(frequency_hopping),
                Euci_ack=int(Euci_ack), Euci_CSI1=int(Euci_CSI1), Euci_CSI2=int(Euci_CSI2), Euci_ackrvd=int(Euci_ackrvd),
                G_ULSCH=int(G_ULSCH), Gtotal=int(Gtotal))
    n = _lib.call("ldpc5g_uci_map_plan", **args, plan=None, plan_bytes=0)
    blob = np.zeros(int(n), np.uint8)
    _lib.call("ldpc5g_uci_map_plan", **args, plan=blob, plan_bytes=int(n))
    return blob


@functools.lru_cache(maxsize=64)
def _plan(*key):
    return Plan(plan_blob(*key[:3], key[3], *key[4:]))


def slot_bits(pusch_config, dmrs_symlist, Qm):
    """Gtotal of an allocation whose data resource elements are all the PUSCH's own."""
    c = pusch_config
    RB, start, nsym = int(c["ResAlloType1"]["RBSize"]), int(c["StartSymbolIndex"]), int(c["NrOfSymbols"])
    dre = 6 if int(c["DMRS"]["NumCDMGroupsWithoutData"]) == 1 else 0
    nre = sum(RB * dre if s in list(dmrs_symlist) else RB * 12 for s in range(start, start + nsym))
    return nre * int(c["num_of_layers"]) * int(Qm)


def plan(pusch_config, dmrs_symlist, rm, Qm, Gtotal=None):
    """The §6.2.7 map of one configuration (cached).  Gtotal defaults to the allocation's bits."""
    c = pusch_config
    oack, ocsi1, ocsi2 = _payloads(c)
    G = slot_bits(c, dmrs_symlist, Qm) if Gtotal is None else int(Gtotal)
    hop = int(str(c.get("FrequencyHopping", 0)).lower() not in ("0", "false", "none", "neither", "disabled", ""))
    return _plan(int(c["ResAlloType1"]["RBSize"]), int(c["StartSymbolIndex"]), int(c["NrOfSymbols"]),
                 tuple(int(x) for x in dmrs_symlist), int(c["DMRS"]["NumCDMGroupsWithoutData"]), int(c["num_of_layers"]), int(Qm),
                 oack, ocsi1, ocsi2, int(c["EnableULSCH"]), rm["Euci_ack"], rm["Euci_CSI1"], rm["Euci_CSI2"],
                 rm["Euci_ackrvd"], rm["G_ULSCH"], G, hop)


def _rows(x, width, dtypes, name):
    t = _lib.require_gpu()
    assert x.is_cuda and x.dtype in dtypes, f"{name}: a cuda tensor of {dtypes}"
    if x.dim() == 1:
        x = x[None]
    assert x.dim() == 2 and x.shape[1] >= width, f"{name}: [T, >= {width}], got {tuple(x.shape)}"
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < width):
        x = x.contiguous()
    return t, x, (x.stride(0) if x.shape[0] > 1 else max(width, x.shape[1]))


# ---------------------------------------------------------------------------- small-block + polar codec
def sb_N(K, Qm):
    return Qm if K == 1 else 3 * Qm if K == 2 else 32


def smallblock_encode(bits, E, Qm):
    t, bits, ld = _rows(bits, 1, (_lib.torch().int8,), "bits")
    T, K = bits.shape
    out = t.empty((T, int(E)), dtype=t.int8, device=bits.device)
    _lib.call("ldpc5g_smallblock_encode", bits.device, bits=bits, ldb=ld, K=K, Qm=int(Qm), out=out, ldo=int(E), E=int(E),
              T=T)
    return out


def smallblock_decode(llr, K, Qm):
    t = _lib.torch()
    t, llr, ld = _rows(llr, 1, (t.float32, t.float64), "llr")
    T, E = llr.shape
    out = t.empty((T, int(K)), dtype=t.int8, device=llr.device)
    _lib.call("ldpc5g_smallblock_decode", llr.device, llr=llr, dtype=_lib.dtype_id(llr.dtype), ldl=ld, E=E, K=int(K),
              Qm=int(Qm), out=out, ldo=int(K), T=T)
    return out


def _segments(A, E):
    """nr_polar_cbsegment.py:6-54 -> (C, pad, L, poly, Er)."""
    assert 12 <= A <= 1706
    if A >= 1013 or (A >= 360 and E >= 1088):
        assert E % 2 == 0
        return 2, A % 2, 11, "11", E // 2
    return (1, 0, 6, "6", E) if A <= 19 else (1, 0, 11, "11", E)


def _crc_bits(t, blk, L, poly):
    from . import sch
    rem = sch.crc_rows(blk, poly)
    sh = t.arange(L - 1, -1, -1, device=blk.device, dtype=t.int64)
    return ((rem[:, None] >> sh) & 1).to(t.int8)


def encode(bits, E, Qm):
    """encode_uci_on_ulsch (nr_pusch_uci.py:16-49) of T payloads: bits [T, A] int8 -> [T, E] int8."""
    t = _lib.require_gpu()
    if bits.dim() == 1:
        bits = bits[None]
    T, A = bits.shape
    if A <= 11:
        return smallblock_encode(bits, E, Qm)
    C, pad, L, poly, Er = _segments(A, int(E))
    x = bits if not pad else t.cat([t.zeros((T, 1), dtype=t.int8, device=bits.device), bits], 1)
    blk = x.reshape(T * C, -1).contiguous()
    blk = t.cat([blk, _crc_bits(t, blk, L, poly)], 1)
    p = polar.plan(blk.shape[1], Er, 10, 0, L)
    return polar.polar_tx(blk, p, Er, 1).reshape(T, C * Er)


def decode(llr, A, E, Qm, L=8):
    """The inverse of encode on LLRs [T, E] (float32 or float64): -> (bits [T, A] int8, crc_ok [T] bool or
    None for A <= 11).  A <= 11: soft maximum-likelihood small-block decision.  A >= 12: CA-PC-SCL polar
    decoding with list size L per segment; crc_ok is every segment's CRC."""
    t = _lib.require_gpu()
    if llr.dim() == 1:
        llr = llr[None]
    assert llr.shape[1] == int(E)
    if A <= 11:
        return smallblock_decode(llr, A, Qm), None
    T = llr.shape[0]
    C, pad, Lc, poly, Er = _segments(int(A), int(E))
    K = (A + pad) // C + Lc
    p = polar.plan(K, Er, 10, 0, Lc)
    x = llr[:, :C * Er].to(t.float64).reshape(T * C, Er).contiguous()
    ck, status, _ = polar.polar_rx(x, p, Er, 1, "SCL", int(L))
    ok = (status.reshape(T, C) == 1).all(1)
    out = ck[:, :K - Lc].reshape(T, -1)[:, pad:]
    return out.contiguous(), ok


# ---------------------------------------------------------------------------- the three map kernels
def mux(p, g_ulsch=None, g_ack=None, g_csi1=None, g_csi2=None):
    """data_control_multiplex (nr_pusch_datactrl_multiplex.py:7-267): the coded streams [T, len] int8
    (None for a stream the plan does not hold) -> g_seq [T, Gtotal] int8."""
    t = _lib.require_gpu()
    ins, T, dev = {}, None, None
    for n, x in zip(STREAMS, (g_ulsch, g_ack, g_csi1, g_csi2)):
        if p.lens[n] == 0:
            ins["g_" + n], ins["ld_" + n] = None, 0
            continue
        assert x is not None, f"g_{n}: the plan holds {p.lens[n]} bits of it"
        _, x, ld = _rows(x, p.lens[n], (t.int8,), "g_" + n)
        assert T in (None, x.shape[0]), "the streams must have the same number of rows"
        T, dev = x.shape[0], x.device
        ins["g_" + n], ins["ld_" + n] = x, ld
    assert T is not None
    g = t.empty((T, p.Gtotal), dtype=t.int8, device=dev)
    _lib.call("ldpc5g_uci_mux", dev, plan_dev=p.dev(dev), plan_host=p.host, **ins, g_seq=g, ldg=p.Gtotal, T=T)
    return g


def demux(p, llr, cinit=None, words=None, erase_punctured=True):
    """The four LLR streams of llr [T, Gtotal] (float32 / float64), as UciStreams of the same dtype (an
    absent stream has width 0).  Without cinit / words: the permutation of data_control_separate
    (nr_pusch_datactrl_multiplex.py:269-539) of already descrambled LLRs.  With cinit [T] (or precomputed
    phy.prbs_words): llr is still scrambled; ordinary positions are descrambled, a y placeholder by the
    bit before it, an x placeholder becomes 0.  erase_punctured zeroes the UL-SCH (or CSI part 2) LLRs
    that a 1-2 bit HARQ-ACK overwrote; the reference leaves them in."""
    t = _lib.torch()
    t, llr, ld = _rows(llr, p.Gtotal, (t.float32, t.float64), "llr")
    T = llr.shape[0]
    w = words if words is not None else (None if cinit is None else phy.prbs_words(cinit, p.Gtotal))
    if w is not None:
        assert w.dim() == 2 and w.shape[0] == T and w.stride(1) == 1 and w.shape[1] * 32 >= p.Gtotal
    outs = [t.empty((T, p.lens[n]), dtype=llr.dtype, device=llr.device) for n in STREAMS]
    args = {}
    for n, o in zip(STREAMS, outs):
        args["g_" + n], args["ld_" + n] = (o if p.lens[n] else None), p.lens[n]
    _lib.call("ldpc5g_uci_demux", llr.device, plan_dev=p.dev(llr.device), plan_host=p.host, llr=llr,
              dtype=_lib.dtype_id(llr.dtype), ldl=ld, prbs=w, ldw=_lib.row_stride(w, 0, w.shape[1]) if w is not None else 0,
              erase_punctured=int(bool(erase_punctured)), **args, T=T)
    return UciStreams(*outs)


def scramble_modulate(g_seq, mod, cinit=None, words=None):
    """38.211 §6.3.1.1 / §6.3.1.2 of a g_seq [T, G] int8 that may hold the placeholders x = -1 and y = -2
    (nr_pusch_process.py:14-30) -> [T, G / Qm] complex64.  mod: a phy.MOD_ID value up to 256QAM."""
    t, g, ld = _rows(g_seq, 1, (_lib.torch().int8,), "g_seq")
    T, G = g.shape
    Qm = phy.bits_per_symbol(mod)
    assert G % Qm == 0
    w = words if words is not None else phy.prbs_words(cinit, G)
    assert w.dim() == 2 and w.shape[0] == T and w.stride(1) == 1 and w.shape[1] * 32 >= G
    sym = t.empty((T, G // Qm), dtype=t.complex64, device=g.device)
    _lib.call("ldpc5g_uci_scramble_modulate", g.device, bits=g, ldb=ld, prbs=w, ldw=_lib.row_stride(w, 0, w.shape[1]), T=T,
              nbits=G, mod=int(mod), sym=sym, ldsym=G // Qm)
    return sym
