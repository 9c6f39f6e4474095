"""CPU tests of the fused receive front end's host side: ldpc5g_sch_demod_raterecover and
ldpc5g_sch_rx_decode validate their arguments before touching the GPU, and the binding declares
them as the header does.  No kernel is launched here."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from python_5gtoolbox_amd import _lib
from python_5gtoolbox_amd.sch import sch_config

CFG = (12000, 4, 517, 1, 0, 30000, 25000)            # C = 2, Qm = 4, E = 12500 per codeblock: staged
BIG = (2000, 2, 500, 1, 0, 60000, 60000)             # one codeblock of E = 60000: 240 KB of float32
P = ctypes.c_void_p(4096)                             # a non-null "buffer" (never dereferenced)


def _front(lib, cfg, sym=P, sym_dtype=_lib.F32, ldsym=None, nv=P, ldnv=None, prbs=None, ldw=0, mod=None,
           T=2, harq=None, dn=P, dn_dtype=_lib.F32, llr_ws=None, ldws=0):
    nsym = cfg.E_total // cfg.Qm
    return lib.ldpc5g_sch_demod_raterecover(
        sym, sym_dtype, nsym if ldsym is None else ldsym, nv, nsym if ldnv is None else ldnv, prbs, ldw,
        cfg.Qm if mod is None else mod, ctypes.byref(cfg), T, harq, dn, dn_dtype, llr_ws, ldws, None)


def _bad(lib, rc):
    assert rc == _lib.ESIZE
    msg = lib.ldpc5g_last_error()
    assert msg, "an argument error must leave a message"
    return msg


def test_demod_raterecover_validates_before_touching_the_gpu():
    lib = _lib.lib()
    cfg = sch_config(*CFG)
    nsym = cfg.E_total // cfg.Qm
    assert b"Qm" in _bad(lib, _front(lib, cfg, mod=2))            # |mod| != cfg.Qm
    assert b"Qm" in _bad(lib, _front(lib, cfg, mod=-1))           # pi/2-BPSK on a 16QAM configuration
    _bad(lib, _front(lib, cfg, mod=3))                            # not a modulation at all
    assert b"dtype" in _bad(lib, _front(lib, cfg, sym_dtype=7))
    assert b"dtype" in _bad(lib, _front(lib, cfg, dn_dtype=7))
    assert b"stride" in _bad(lib, _front(lib, cfg, ldsym=nsym - 1))
    assert b"stride" in _bad(lib, _front(lib, cfg, ldnv=nsym - 1))
    assert b"stride" in _bad(lib, _front(lib, cfg, prbs=P, ldw=(cfg.E_total + 31) // 32 - 1))
    assert _front(lib, cfg, ldsym=nsym - 1, T=1, sym=None) == _lib.ESIZE   # T = 1: strides unused; null sym
    for null in ("sym", "nv", "dn"):
        assert b"null" in _bad(lib, _front(lib, cfg, **{null: None}))
    _bad(lib, _front(lib, cfg, T=-1))
    bad = _lib.SchCfg.from_buffer_copy(cfg)
    bad.K_apo += 1
    _bad(lib, _front(lib, bad))
    assert lib.ldpc5g_sch_demod_raterecover(None, _lib.F32, 0, None, 0, None, 0, cfg.Qm, None, 1, None, None,
                                            _lib.F32, None, 0, None) == _lib.ESIZE   # null cfg
    assert _front(lib, cfg, T=0, sym=None, nv=None, dn=None) == 0   # empty batch: nothing to do
    assert lib.ldpc5g_last_error() == b""


def test_rows_larger_than_the_stage_need_scratch():
    lib = _lib.lib()
    big = sch_config(*BIG)
    assert lib.ldpc5g_sch_rx_scratch_elems(ctypes.byref(big), 2, _lib.F32) == big.E_total
    msg = _bad(lib, _front(lib, big, llr_ws=None))
    assert b"LDS stage" in msg and b"llr_ws" in msg and b"60000" in msg
    assert b"ldws" in _bad(lib, _front(lib, big, llr_ws=P, ldws=big.E_total - 1))
    assert _front(lib, big, T=0) == 0
    cfg = sch_config(*CFG)
    assert lib.ldpc5g_sch_rx_scratch_elems(ctypes.byref(cfg), 4, _lib.F64) == 0
    assert lib.ldpc5g_sch_rx_scratch_elems(ctypes.byref(cfg), 2, _lib.F64) == _lib.ESIZE
    # BPSK on complex128 stages float64 LLRs (demod_bpsk.py:9): half as many fit
    bpsk = sch_config(9000, 1, 400, 1, 0, 0, 19998)   # E = 9999 per codeblock
    assert lib.ldpc5g_sch_rx_scratch_elems(ctypes.byref(bpsk), 1, _lib.F32) == 0
    assert lib.ldpc5g_sch_rx_scratch_elems(ctypes.byref(bpsk), -1, _lib.F64) == 0
    assert lib.ldpc5g_sch_rx_scratch_elems(ctypes.byref(bpsk), 1, _lib.F64) == bpsk.E_total


def test_rx_decode_validates_like_the_front_end():
    lib = _lib.lib()
    cfg = sch_config(*CFG)
    nsym = cfg.E_total // cfg.Qm

    def call(mod=cfg.Qm, T=1, sym=P):
        return lib.ldpc5g_sch_rx_decode(sym, _lib.F32, nsym, P, nsym, None, 0, mod, ctypes.byref(cfg), T, None,
                                        P, _lib.F32, None, 0, None, None, None, 8, 0.8, 0.0, _lib.LAYERED,
                                        None, cfg.B, None, None, None, None)
    _bad(lib, call(mod=6))
    assert b"null" in _bad(lib, call(sym=None))
    assert call(T=0) == 0


def test_binding_matches_header_argument_counts():
    src = open(os.path.join(ROOT, "include", "ldpc5g.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    for name, n in (("ldpc5g_sch_demod_raterecover", 16), ("ldpc5g_sch_rx_decode", 28),
                    ("ldpc5g_sch_rx_scratch_elems", 3)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)


@pytest.mark.parametrize("mod", [1, -1, 2, 4, 6, 8, 10])
def test_every_modulation_is_accepted_with_its_qm(mod):
    lib = _lib.lib()
    Qm = abs(mod)
    cfg = sch_config(3000, Qm, 300, 1, 0, 0, 600 * Qm)
    assert _front(lib, cfg, mod=mod, T=0) == 0
    assert b"null" in _bad(lib, _front(lib, cfg, mod=mod, T=1, sym=None))
