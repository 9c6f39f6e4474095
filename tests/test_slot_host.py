"""CPU tests of the slot front end's host side and of its numpy restatement: ldpc5g_slot_rx_frontend
and ldpc5g_slot_map refuse every unsupported argument before any HIP call, tests/slot_ref.py
reproduces the reference's recorded LS estimates (tests/golden/slot_golden_L*.npz) within the gap
stored with each case and its transmit grids (slot_golden_M*.npz), and phy.dmrs_symlist /
phy.slot_data_re_idx equal the recorded symbol lists, usage maps and data-RE indices.  No kernel is
launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import slot_ref
from conftest import GOLD, ROOT
from python_5gtoolbox_amd import _lib, phy

P = ctypes.c_void_p(4096)   # a non-null, aligned "buffer" (never dereferenced)
GAP_MAX = 64 * 2.0 ** -23


@pytest.fixture(scope="module")
def golden():
    return slot_ref.load_golden(GOLD)


def _arr(v):
    return (ctypes.c_int32 * max(len(v), 1))(*v) if v is not None else None


def _fe(lib, grid=P, ldgrid=None, dtype=_lib.F32, slots=P, T=2, carrier_re=288, rb_start=3, rb_size=16, Nr=2, Nt=2,
        ports=(0, 1), S=2, sym=(2, 11), nid=1, nscid=0, cdm=2, h_ls=P, ldh=None, y=P, ldy=None):
    """A valid ldpc5g_slot_rx_frontend call by default: 16 PRB at 3 of 24, 2x2, DMRS symbols [2, 11]."""
    N = 3 * rb_size
    return lib.ldpc5g_slot_rx_frontend(
        grid, Nr * 14 * carrier_re if ldgrid is None else ldgrid, dtype, slots, T, carrier_re, rb_start, rb_size, Nr,
        Nt, _arr(ports), S, _arr(sym), nid, nscid, cdm, h_ls, S * N * Nr * Nt if ldh is None else ldh, y,
        14 * 4 * N * Nr if ldy is None else ldy, None)


def _map(lib, sym_=P, ldsym=None, re_idx=P, nre=1920, slots=P, T=2, carrier_re=288, rb_start=3, rb_size=16, num_ant=2,
         NL=2, precoding=None, S=2, sym=(2, 11), nid=1, nscid=0, cdm=2, grid=P, ldgrid=None):
    """A valid ldpc5g_slot_map call by default."""
    pm = (ctypes.c_float * len(precoding))(*precoding) if precoding is not None else None
    return lib.ldpc5g_slot_map(
        sym_, nre * NL if ldsym is None else ldsym, re_idx, nre, slots, T, carrier_re, rb_start, rb_size, num_ant, NL,
        pm, S, _arr(sym), nid, nscid, cdm, grid, num_ant * 14 * carrier_re if ldgrid is None else ldgrid, None)


def _bad(lib, rc, field):
    assert rc == _lib.ESIZE
    msg = lib.ldpc5g_last_error()
    assert field in msg, (field, msg)


def _common_refusals(lib, call):
    """The limits the two entry points share."""
    for S, sym in ((0, ()), (5, (1, 2, 3, 4, 5)), (-1, ())):
        _bad(lib, call(lib, S=S, sym=sym), b"S=")
    for sym in ((11, 2), (2, 2), (2, 14), (-1, 3)):
        _bad(lib, call(lib, sym=sym), b"sym_idx")
    _bad(lib, call(lib, sym=None), b"sym_idx")
    for rb in (0, -1, 276):
        _bad(lib, call(lib, rb_size=rb), b"rb_size")
    for start, size in ((9, 16), (-1, 16), (24, 1), (0, 25)):
        _bad(lib, call(lib, rb_start=start, rb_size=size), b"rb_start")
    for cre in (0, 287, 12 * 276, -12):
        _bad(lib, call(lib, carrier_re=cre, rb_start=0, rb_size=1), b"carrier_re")
    for nid in (-1, 65536):
        _bad(lib, call(lib, nid=nid), b"nNIDnSCID")
    for nscid in (-1, 2):
        _bad(lib, call(lib, nscid=nscid), b"nSCID")
    for cdm in (0, 3):
        _bad(lib, call(lib, cdm=cdm), b"num_cdm_groups")
    for T in (0, -1, 65536):
        _bad(lib, call(lib, T=T), b"T=")
    _bad(lib, call(lib, slots=None), b"null")
    _bad(lib, call(lib, grid=None), b"null")
    for T in (1, 2):   # a row stride shorter than its row, T = 1 included
        _bad(lib, call(lib, T=T, ldgrid=2 * 14 * 288 - 1), b"stride")


def test_rx_frontend_refuses_unsupported_arguments_before_touching_the_gpu():
    lib = _lib.lib()
    _bad(lib, _fe(lib, grid=None), b"null")   # the default call is valid up to the buffer check
    _common_refusals(lib, _fe)
    for Nr in (0, 3, 8, -1):
        _bad(lib, _fe(lib, Nr=Nr), b"Nr")
    for Nt in (0, 5, -1):
        _bad(lib, _fe(lib, Nt=Nt, ports=(0, 1, 2, 3)), b"Nt")
    for ports in ((0, 4), (-1, 0), (2, 2)):
        _bad(lib, _fe(lib, ports=ports), b"ports")
    _bad(lib, _fe(lib, ports=None), b"ports")
    for dt in (-1, 2, 7):
        _bad(lib, _fe(lib, dtype=dt), b"dtype")
    for T in (1, 2):
        _bad(lib, _fe(lib, T=T, ldh=2 * 48 * 4 - 1), b"stride")
        _bad(lib, _fe(lib, T=T, ldy=14 * 192 * 2 - 1), b"stride")
    _bad(lib, _fe(lib, h_ls=None, y=None), b"null")
    _bad(lib, _fe(lib, dtype=_lib.F64, grid=ctypes.c_void_p(4104)), b"aligned")
    _bad(lib, _fe(lib, y=ctypes.c_void_p(4100)), b"aligned")


@pytest.mark.parametrize("Nr", [1, 2, 4])
def test_every_supported_frontend_shape_passes_the_shape_check(Nr):
    lib = _lib.lib()
    for Nt in (1, 2, 3, 4):
        for dt in (_lib.F32, _lib.F64):
            for S, sym in ((1, (2,)), (4, (2, 5, 8, 11))):
                for skip in ({}, {"h_ls": None}, {"y": None}):   # either half alone is a valid call
                    _bad(lib, _fe(lib, Nr=Nr, Nt=Nt, ports=(3, 1, 0, 2)[:Nt], dtype=dt, S=S, sym=sym, rb_start=0,
                                  rb_size=24, slots=None, **skip), b"null")


def test_slot_map_refuses_unsupported_arguments_before_touching_the_gpu():
    lib = _lib.lib()
    _bad(lib, _map(lib, grid=None), b"null")
    _common_refusals(lib, _map)
    for na in (0, 3, 8):
        _bad(lib, _map(lib, num_ant=na), b"num_ant")
    for NL in (0, 5):
        _bad(lib, _map(lib, NL=NL), b"NL")
    _bad(lib, _map(lib, num_ant=2, NL=4), b"precoding")   # identity needs NL <= num_ant
    _bad(lib, _map(lib, num_ant=2, NL=4, precoding=[0.5] * 16, grid=None), b"null")
    for nre in (-1, 14 * 192 + 1):
        _bad(lib, _map(lib, nre=nre), b"nre")
    for T in (1, 2):
        _bad(lib, _map(lib, T=T, ldsym=1920 * 2 - 1), b"stride")
    _bad(lib, _map(lib, sym_=None), b"null")
    _bad(lib, _map(lib, re_idx=None), b"null")
    _bad(lib, _map(lib, nre=0, sym_=None, re_idx=None, grid=None), b"null")   # DMRS only: sym may be NULL
    _bad(lib, _map(lib, grid=ctypes.c_void_p(4100)), b"aligned")


def test_binding_matches_header():
    src = open(os.path.join(ROOT, "include", "ldpc5g.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n in (("ldpc5g_slot_rx_frontend", 21), ("ldpc5g_slot_map", 20)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name)


def test_fixture_covers_the_cases(golden):
    want = ["L" + n for n in slot_ref.LS_CASES] + list(slot_ref.MAP_CASES) + list(slot_ref.E2E_CASES) + ["symlists"]
    assert sorted(golden) == sorted(want)
    S = set()
    for name, (kind, kw, Nr, slot) in slot_ref.LS_CASES.items():
        c = golden["L" + name]
        p = slot_ref.params(slot_ref.make_config(kind, kw))
        assert c["grid"].shape == (Nr, 14 * 12 * slot_ref.CARRIER_PRB) and c["grid"].dtype == np.complex64
        assert c["h_ls"].shape == (len(p["syms"]), 3 * kw["rb_size"], Nr, len(kw["ports"]))
        assert c["h_ls"].dtype == np.complex64 and int(c["slot"]) == slot and 0 < float(c["gap"]) <= GAP_MAX
        S.add(len(p["syms"]))
    assert S == {1, 2, 3, 4}
    for name in slot_ref.E2E_CASES:
        assert bool(golden[name]["status"]) and np.array_equal(golden[name]["tbblk"][:int(golden[name]["meta"][0])],
                                                               golden[name]["trblk"])


@pytest.mark.parametrize("name", sorted(slot_ref.LS_CASES))
def test_restatement_reproduces_the_reference_ls_estimate(golden, name):
    kind, kw, Nr, slot = slot_ref.LS_CASES[name]
    c = golden["L" + name]
    mine = slot_ref.ls_est(c["grid"], slot_ref.make_config(kind, kw), slot)
    gap = np.abs(mine - c["h_ls"]).max() / np.abs(c["h_ls"]).max()
    print(name, "gap", gap, "stored", float(c["gap"]))
    assert gap <= float(c["gap"]) * (1 + 1e-6)


def test_symbol_lists_equal_the_recorded_tables(golden):
    tab = golden["symlists"]["table"]
    for c, channel in enumerate(("pdsch", "pusch")):
        for Ld in range(3, 15):
            for ap in range(4):
                want = [int(v) for v in tab[c, Ld - 3, ap] if v >= 0]
                assert phy.dmrs_symlist(Ld, ap, channel) == want, (channel, Ld, ap)
                assert slot_ref.symlist(Ld, ap, channel) == want
    with pytest.raises(AssertionError):
        phy.dmrs_symlist(14, 4)
    with pytest.raises(AssertionError):
        phy.dmrs_symlist(14, 1, "pucch")


@pytest.mark.parametrize("name", sorted(slot_ref.MAP_CASES))
def test_usage_map_re_idx_and_mapper_equal_the_reference(golden, name):
    kw, num_ant, pm, slot = slot_ref.MAP_CASES[name]
    cfg = slot_ref.pdsch_config(**kw)
    c = golden[name]
    re_idx, usage = phy.slot_data_re_idx(cfg)
    assert re_idx.dtype == np.int32 and usage.dtype == np.float64
    assert np.array_equal(usage, c["usage"]) and np.array_equal(re_idx, c["re_idx"])
    assert np.all(np.diff(re_idx) > 0)
    idx2, usage2 = slot_ref.data_re_idx(cfg)
    assert np.array_equal(usage2, c["usage"]) and np.array_equal(idx2, c["re_idx"])
    NL = len(kw["ports"])
    mine = slot_ref.slot_map(c["sym"], cfg, slot, slot_ref.CARRIER_PRB, num_ant, pm)
    if pm is None:
        assert np.all(mine == c["grid"])   # ==, so -0.0 passes
    else:
        assert np.abs(mine - c["grid"]).max() <= 4 * NL * 2.0 ** -23 * np.abs(c["grid"]).max()


def test_usage_rules_beyond_the_fixture():
    """One CDM group: only the used groups' REs are taken; a short allocation drops the DMRS symbols
    after its end; ports beyond num_of_layers do not count."""
    cfg = slot_ref.pdsch_config(rb_start=0, rb_size=2, ports=[1002], add_pos=1, cdm=1, start=2, nsym=8)   # Ld = 10
    re_idx, usage = phy.slot_data_re_idx(cfg)
    assert usage.shape == (8, 24) and list(np.nonzero(usage.sum(1))[0]) == [0, 7]   # symbols 2 and 9
    assert np.array_equal(usage[0], np.tile([0, 1], 12))
    assert len(re_idx) == 8 * 24 - 2 * 12 and re_idx[0] == 2 * 24 and re_idx[-1] == 9 * 24 + 22
    cfg = slot_ref.pdsch_config(rb_start=0, rb_size=1, ports=[1001, 1003], cdm=1)
    cfg["num_of_layers"] = 1   # only port 1001 is used
    _, usage = phy.slot_data_re_idx(cfg)
    assert np.array_equal(usage[0], np.tile([1, 0], 6))
    for cf in (slot_ref.pdsch_config(0, 3, [1000, 1002], cdm=1), slot_ref.pdsch_config(0, 3, [1000], cdm=2)):
        a, b = phy.slot_data_re_idx(cf), slot_ref.data_re_idx(cf)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1][0].sum() == 36
