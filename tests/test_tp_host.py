"""CPU tests of the host side of PUSCH transform precoding and of its numpy restatement:
ldpc5g_transform_precode, ldpc5g_low_papr_seq, ldpc5g_slot_rx_frontend_tp and ldpc5g_slot_map_tp
refuse every unsupported argument before any HIP call, and tests/tp_ref.py reproduces the
reference's recorded sequences, hopping table, LS estimates and transmit processing
(tests/golden/tp_golden_*.npz) within the gap stored with each case.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import tp_ref
from conftest import GOLD, ROOT
from python_5gtoolbox_amd import _lib

P = ctypes.c_void_p(4096)   # a non-null, aligned "buffer" (never dereferenced)
GAP_MAX = 64 * 2.0 ** -23


@pytest.fixture(scope="module")
def golden():
    return tp_ref.load_golden(GOLD)


def _arr(v):
    return (ctypes.c_int32 * max(len(v), 1))(*v) if v is not None else None


def _dft(lib, x=P, ldx=None, out=P, ldo=None, dtype=_lib.F32, T=2, nsym=3, rb_size=16, inverse=0):
    """A valid ldpc5g_transform_precode call by default (in place)."""
    row = nsym * 12 * rb_size
    return lib.ldpc5g_transform_precode(x, row if ldx is None else ldx, out, row if ldo is None else ldo, dtype, T,
                                        nsym, rb_size, inverse, None)


def _seq(lib, u=P, v=P, n=3, alpha=0.0, MZC=72, out=P):
    return lib.ldpc5g_low_papr_seq(u, v, n, alpha, MZC, out, None)


def _fe(lib, grid=P, ldgrid=None, dtype=_lib.F32, slots=P, T=2, carrier_re=288, rb_start=3, rb_size=16, Nr=2, port=0,
        S=2, sym=(2, 11), nid=77, hopping=1, base_seq=None, h_ls=P, ldh=None, y=P, ldy=None):
    """A valid ldpc5g_slot_rx_frontend_tp call by default: 16 PRB at 3 of 24, 1x2, DMRS symbols [2, 11]."""
    N = 3 * rb_size
    return lib.ldpc5g_slot_rx_frontend_tp(
        grid, Nr * 14 * carrier_re if ldgrid is None else ldgrid, dtype, slots, T, carrier_re, rb_start, rb_size, Nr,
        port, S, _arr(sym), nid, hopping, base_seq, h_ls, S * N * Nr if ldh is None else ldh, y,
        14 * 4 * N * Nr if ldy is None else ldy, None)


def _map(lib, sym_=P, ldsym=None, re_idx=P, nre=1920, slots=P, T=2, carrier_re=288, rb_start=3, rb_size=16, num_ant=2,
         port=0, precoding=None, S=2, sym=(2, 11), nid=77, hopping=1, base_seq=None, grid=P, ldgrid=None):
    """A valid ldpc5g_slot_map_tp call by default."""
    pm = (ctypes.c_float * len(precoding))(*precoding) if precoding is not None else None
    return lib.ldpc5g_slot_map_tp(
        sym_, nre if ldsym is None else ldsym, re_idx, nre, slots, T, carrier_re, rb_start, rb_size, num_ant, port, pm,
        S, _arr(sym), nid, hopping, base_seq, grid, num_ant * 14 * carrier_re if ldgrid is None else ldgrid, None)


def _bad(lib, rc, field):
    assert rc == _lib.ESIZE
    msg = lib.ldpc5g_last_error()
    assert field in msg, (field, msg)


# (entry point, keyword arguments, the word its message must hold)
REFUSALS = [
    (_dft, dict(rb_size=7), b"rb_size"), (_dft, dict(rb_size=11), b"rb_size"), (_dft, dict(rb_size=276), b"rb_size"),
    (_dft, dict(rb_size=0), b"rb_size"), (_dft, dict(rb_size=-1), b"rb_size"),
    (_dft, dict(T=0), b"T="), (_dft, dict(T=65536), b"T="), (_dft, dict(T=-1), b"T="),
    (_dft, dict(nsym=0), b"nsym"), (_dft, dict(nsym=15), b"nsym"),
    (_dft, dict(inverse=2), b"inverse"), (_dft, dict(inverse=-1), b"inverse"),
    (_dft, dict(dtype=2), b"dtype"), (_dft, dict(dtype=-1), b"dtype"),
    (_dft, dict(ldx=3 * 192 - 1), b"stride"), (_dft, dict(ldo=3 * 192 - 1), b"stride"),
    (_dft, dict(T=1, ldx=3 * 192 - 1), b"stride"),
    (_dft, dict(x=None), b"null"), (_dft, dict(out=None), b"null"),
    (_dft, dict(dtype=_lib.F64, x=ctypes.c_void_p(4104)), b"aligned"), (_dft, dict(out=ctypes.c_void_p(4100)), b"aligned"),
    (_dft, dict(ldo=3 * 192 + 2), b"in place"),
    (_seq, dict(MZC=6), b"MZC"), (_seq, dict(MZC=12), b"MZC"), (_seq, dict(MZC=18), b"MZC"), (_seq, dict(MZC=24), b"MZC"),
    (_seq, dict(MZC=0), b"MZC"), (_seq, dict(MZC=35), b"MZC"), (_seq, dict(MZC=3306), b"MZC"),
    (_seq, dict(n=0), b"n="), (_seq, dict(n=65536), b"n="), (_seq, dict(alpha=float("nan")), b"alpha"),
    (_seq, dict(alpha=float("inf")), b"alpha"),
    (_seq, dict(u=None), b"null"), (_seq, dict(v=None), b"null"), (_seq, dict(out=None), b"null"),
    (_seq, dict(out=ctypes.c_void_p(4104)), b"aligned"), (_seq, dict(u=ctypes.c_void_p(4098)), b"aligned"),
]
for _call in (_fe, _map):
    REFUSALS += [
        (_call, dict(rb_size=7, rb_start=0), b"rb_size"), (_call, dict(rb_size=11, rb_start=0), b"rb_size"),
        (_call, dict(rb_size=276), b"rb_size"), (_call, dict(rb_size=0), b"rb_size"),
        (_call, dict(rb_start=9), b"rb_start"), (_call, dict(rb_start=-1), b"rb_start"),
        (_call, dict(carrier_re=287, rb_start=0, rb_size=1, base_seq=P), b"carrier_re"),
        (_call, dict(carrier_re=12 * 276), b"carrier_re"),
        (_call, dict(hopping=3), b"hopping"), (_call, dict(hopping=-1), b"hopping"),
        (_call, dict(nid=1008), b"nPuschID"), (_call, dict(nid=-1), b"nPuschID"),
        (_call, dict(port=4), b"port"), (_call, dict(port=-1), b"port"),
        (_call, dict(rb_size=4), b"base_seq"), (_call, dict(rb_size=1), b"base_seq"),
        (_call, dict(base_seq=ctypes.c_void_p(4104)), b"base_seq"),
        (_call, dict(S=0, sym=()), b"S="), (_call, dict(S=5, sym=(1, 2, 3, 4, 5)), b"S="),
        (_call, dict(sym=(11, 2)), b"sym_idx"), (_call, dict(sym=(2, 14)), b"sym_idx"), (_call, dict(sym=None), b"sym_idx"),
        (_call, dict(T=0), b"T="), (_call, dict(T=65536), b"T="),
        (_call, dict(slots=None), b"null"), (_call, dict(grid=None), b"null"),
        (_call, dict(ldgrid=2 * 14 * 288 - 1), b"stride"), (_call, dict(T=1, ldgrid=2 * 14 * 288 - 1), b"stride"),
        (_call, dict(grid=ctypes.c_void_p(4100)), b"aligned"),
    ]
REFUSALS += [
    (_fe, dict(Nr=0), b"Nr"), (_fe, dict(Nr=3), b"Nr"), (_fe, dict(Nr=8), b"Nr"),
    (_fe, dict(dtype=2), b"dtype"), (_fe, dict(ldh=2 * 48 * 2 - 1), b"stride"), (_fe, dict(ldy=14 * 192 * 2 - 1), b"stride"),
    (_fe, dict(T=1, ldh=2 * 48 * 2 - 1), b"stride"), (_fe, dict(h_ls=None, y=None), b"null"),
    (_fe, dict(dtype=_lib.F64, grid=ctypes.c_void_p(4104)), b"aligned"), (_fe, dict(y=ctypes.c_void_p(4100)), b"aligned"),
    (_map, dict(num_ant=0), b"num_ant"), (_map, dict(num_ant=3), b"num_ant"), (_map, dict(num_ant=8), b"num_ant"),
    (_map, dict(nre=-1), b"nre"), (_map, dict(nre=14 * 192 + 1), b"nre"),
    (_map, dict(ldsym=1919), b"stride"), (_map, dict(T=1, ldsym=1919), b"stride"),
    (_map, dict(sym_=None), b"null"), (_map, dict(re_idx=None), b"null"),
    (_map, dict(nre=0, sym_=None, re_idx=None, grid=None), b"null"),   # DMRS only: sym may be NULL
    (_map, dict(sym_=ctypes.c_void_p(4100)), b"aligned"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)), ids=lambda i: f"{REFUSALS[i][0].__name__}-{i}")
def test_unsupported_arguments_are_refused_before_touching_the_gpu(i):
    call, kw, word = REFUSALS[i]
    lib = _lib.lib()
    _bad(lib, call(lib, **kw), word)


def test_every_supported_shape_passes_the_shape_checks():
    """Each default call, and every length / antenna count / dtype, is valid up to the buffer check."""
    lib = _lib.lib()
    for rb in tp_ref.RB_SIZES:
        for dt in (_lib.F32, _lib.F64):
            for inv in (0, 1):
                _bad(lib, _dft(lib, rb_size=rb, dtype=dt, inverse=inv, nsym=14, x=None), b"null")
        start = 0 if rb > 24 else 24 - rb
        cre = 12 * max(24, rb)
        bs = P if rb <= 4 else None
        for hop in (0, 1, 2):
            _bad(lib, _fe(lib, rb_size=rb, rb_start=start, carrier_re=cre, hopping=hop, base_seq=bs, grid=None), b"null")
            _bad(lib, _map(lib, rb_size=rb, rb_start=start, carrier_re=cre, hopping=hop, base_seq=bs, nre=12 * 12 * rb,
                           grid=None), b"null")
    for MZC in (30, 36, 72, 1620, 3300):
        _bad(lib, _seq(lib, MZC=MZC, out=None), b"null")
    for Nr in (1, 2, 4):
        for port in range(4):
            for skip in ({}, {"h_ls": None}, {"y": None}):
                _bad(lib, _fe(lib, Nr=Nr, port=port, slots=None, **skip), b"null")
            _bad(lib, _map(lib, num_ant=Nr, port=port, precoding=[0.5] * 8, slots=None), b"null")
    _bad(lib, _fe(lib, nid=1007, grid=None), b"null")


def test_binding_matches_header():
    src = open(os.path.join(ROOT, "include", "ldpc5g.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n in (("ldpc5g_transform_precode", 10), ("ldpc5g_low_papr_seq", 7), ("ldpc5g_slot_rx_frontend_tp", 20),
                    ("ldpc5g_slot_map_tp", 20)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name)


def test_fixture_inventory_and_dtypes(golden):
    want = ["seq", "hop"] + ["L" + n for n in tp_ref.LS_CASES] + list(tp_ref.MAP_CASES) + list(tp_ref.E2E_CASES)
    assert sorted(golden) == sorted(want)
    s = golden["seq"]
    for name, (u, v, alpha, MZC) in tp_ref.SEQ_CASES.items():
        assert s[name].shape == (MZC,) and s[name].dtype == np.complex128 and 0 <= float(s[name + "_gap"]) <= 1e-8
    for MZC in tp_ref.SHORT_MZC:
        assert s[f"short{MZC}"].shape == (len(tp_ref.SHORT_U), MZC) and s[f"short{MZC}"].dtype == np.complex128
    assert golden["hop"]["table"].shape == (5, 3, 3, 3, 2) and golden["hop"]["table"].dtype == np.int16
    S = set()
    for name, (kw, Nr, slot) in tp_ref.LS_CASES.items():
        c = golden["L" + name]
        p = tp_ref.tp_params(tp_ref.pusch_config(**kw))
        assert c["grid"].shape == (Nr, 14 * 12 * tp_ref.CARRIER_PRB) and c["grid"].dtype == np.complex64
        assert c["h_ls"].shape == (len(p["syms"]), 3 * kw["rb_size"], Nr, 1) and c["h_ls"].dtype == np.complex64
        assert int(c["slot"]) == slot and 0 < float(c["gap"]) <= GAP_MAX
        S.add(len(p["syms"]))
    assert S == {1, 2, 4}
    for name, (kw, num_ant, slot) in tp_ref.MAP_CASES.items():
        c = golden[name]
        assert c["grid"].shape == (num_ant, 14 * 12 * tp_ref.CARRIER_PRB) and c["grid"].dtype == np.complex64
        assert c["sym"].dtype == np.complex64 and c["sym"].shape == c["re_idx"].shape and c["re_idx"].dtype == np.int32
        assert c["precoded"].shape == (num_ant, c["sym"].size) and c["precoded"].dtype == np.complex64
        assert c["precoding"].shape == ((2, 1) if num_ant == 2 else (0, 1)) and int(c["slot"]) == slot
        assert 0 < float(c["gap_process"]) <= GAP_MAX and 0 < float(c["gap_grid"]) <= GAP_MAX
    for name, e in tp_ref.E2E_CASES.items():
        c = golden[name]
        assert c["grid"].shape == (e["Nr"], 14 * 12 * tp_ref.CARRIER_PRB) and c["grid"].dtype == np.complex64
        assert bool(c["status"]) and np.array_equal(c["tbblk"][:int(c["meta"][0])], c["trblk"])


def test_restatement_reproduces_the_reference_sequences(golden):
    s = golden["seq"]
    for name, (u, v, alpha, MZC) in tp_ref.SEQ_CASES.items():
        gap = np.abs(tp_ref.low_papr_seq(u, v, alpha, MZC) - s[name]).max()
        print(name, "gap", gap, "stored", float(s[name + "_gap"]))
        assert gap <= float(s[name + "_gap"]) * (1 + 1e-6) + 1e-15


def test_q_comes_out_of_integers_as_out_of_the_reference_expression():
    """floor(qbar + 1/2) + v (-1)^floor(2 qbar) (lowPAPR_seq.py:33-34) for every length and group."""
    import math
    for MZC in range(36, 3301, 6):
        N = tp_ref.largest_prime_below(MZC)
        for u in range(30):
            q_bar = N * (u + 1) / 31
            for v in (0, 1):
                assert tp_ref.zc_q(N, u, v) == math.floor(q_bar + 1 / 2) + v * ((-1) ** math.floor(2 * q_bar)), (MZC, u, v)


def test_restatement_reproduces_the_hopping_table_exactly(golden):
    tab = golden["hop"]["table"]
    for a, nid in enumerate(tp_ref.HOP_IDS):
        for b, mode in enumerate(tp_ref.HOPPING):
            for c, slot in enumerate(tp_ref.HOP_SLOTS):
                for d, sym in enumerate(tp_ref.HOP_SYMS):
                    assert tp_ref.hop_uv(nid, mode, 120, slot, sym) == tuple(int(x) for x in tab[a, b, c, d])
    assert tp_ref.hop_uv(77, "sequenceHopping", 66, 7, 5) == (17, 0)   # below 72 there is no sequence hopping


def _base(golden, kw, S):
    if kw["rb_size"] > 4:
        return None
    row = golden["seq"][f"short{6 * kw['rb_size']}"][tp_ref.SHORT_U.index(kw.get("npuschid", 77) % 30)]
    return np.tile(row, (S, 1))


@pytest.mark.parametrize("name", sorted(tp_ref.LS_CASES))
def test_restatement_reproduces_the_reference_ls_estimate(golden, name):
    kw, Nr, slot = tp_ref.LS_CASES[name]
    c = golden["L" + name]
    mine = tp_ref.ls_est(c["grid"], tp_ref.pusch_config(**kw), slot, _base(golden, kw, c["h_ls"].shape[0]))
    gap = np.abs(mine - c["h_ls"]).max() / np.abs(c["h_ls"]).max()
    print(name, "gap", gap, "stored", float(c["gap"]))
    assert gap <= float(c["gap"]) * (1 + 1e-6)


@pytest.mark.parametrize("name", sorted(tp_ref.MAP_CASES))
def test_restatement_reproduces_the_reference_transmit_side(golden, name):
    kw, num_ant, slot = tp_ref.MAP_CASES[name]
    c = golden[name]
    cfg = tp_ref.pusch_config(**kw)
    pm = c["precoding"] if c["precoding"].size else None
    assert np.array_equal(tp_ref.data_re_idx(cfg)[0], c["re_idx"])
    mine = tp_ref.process(c["sym"], kw["rb_size"], pm)
    gap = np.abs(mine - c["precoded"]).max() / np.abs(c["precoded"]).max()
    grid = tp_ref.tp_map(c["sym"], cfg, slot, tp_ref.CARRIER_PRB, num_ant, pm)
    gap_g = np.abs(grid - c["grid"]).max() / np.abs(c["grid"]).max()
    print(name, "gaps", gap, gap_g, "stored", float(c["gap_process"]), float(c["gap_grid"]))
    assert gap <= float(c["gap_process"]) * (1 + 1e-6) and gap_g <= float(c["gap_grid"]) * (1 + 1e-6)
    assert np.all((grid != 0) == (c["grid"] != 0))


def test_restatement_transform_is_orthonormal_and_inverts():
    rng = np.random.default_rng(5)
    for rb in (1, 5, 27, 270):
        x = rng.standard_normal((2, 3 * 12 * rb)) + 1j * rng.standard_normal((2, 3 * 12 * rb))
        y = tp_ref.transform_precode(x, rb)
        assert abs(np.linalg.norm(y) / np.linalg.norm(x) - 1) < 1e-13
        assert np.abs(tp_ref.transform_precode(y, rb, inverse=True) - x).max() < 1e-12
