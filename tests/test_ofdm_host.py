"""CPU tests of the host side of the OFDM low-PHY and of its numpy restatement: ldpc5g_ofdm_demod and
ldpc5g_ofdm_mod refuse every unsupported argument before any HIP call, tests/ofdm_ref.py reproduces
the reference's recorded outputs (tests/golden/ofdm_golden_*.npz) within the gap stored with each
case, and the nr_slot mirrors equal the pinned tables.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import ofdm_ref
from conftest import GOLD, ROOT
from python_5gtoolbox_amd import _lib, nr_slot, phy

P = ctypes.c_void_p(4096)   # a non-null, aligned "buffer" (never dereferenced)
GAP_MAX = 64 * 2.0 ** -23


@pytest.fixture(scope="module")
def golden():
    return ofdm_ref.load_golden(GOLD)


def _demod(lib, td=P, ld_td_slot=None, ld_td_ant=None, grid=P, ld_g_slot=None, ld_g_ant=None, dtype=_lib.F32, T=2, Nr=2,
           nfft=512, carrier_re=288, scs=30, hz=3840 * 10 ** 6):
    """A valid ldpc5g_ofdm_demod call by default: the 24-PRB carrier, two slots, two antennas."""
    S, W = 15 * nfft, 14 * carrier_re
    return lib.ldpc5g_ofdm_demod(td, Nr * S if ld_td_slot is None else ld_td_slot, S if ld_td_ant is None else ld_td_ant,
                                 grid, Nr * W if ld_g_slot is None else ld_g_slot, W if ld_g_ant is None else ld_g_ant,
                                 dtype, T, Nr, nfft, carrier_re, scs, hz, None)


def _mod(lib, td=P, ld_td_slot=None, ld_td_ant=None, grid=P, ld_g_slot=None, ld_g_ant=None, dm=None, dtype=_lib.F32, T=2,
         Nr=2, nfft=512, carrier_re=288, scs=30, hz=3840 * 10 ** 6):
    """A valid ldpc5g_ofdm_mod call by default."""
    S, W = 15 * nfft, 14 * carrier_re
    return lib.ldpc5g_ofdm_mod(grid, Nr * W if ld_g_slot is None else ld_g_slot, W if ld_g_ant is None else ld_g_ant, dm,
                               td, Nr * S if ld_td_slot is None else ld_td_slot, S if ld_td_ant is None else ld_td_ant,
                               dtype, T, Nr, nfft, carrier_re, scs, hz, None)


def _bad(lib, rc, field):
    assert rc == _lib.ESIZE
    msg = lib.ldpc5g_last_error()
    assert field in msg, (field, msg)


# (keyword arguments, the word the message must hold), for both entry points
COMMON = [
    (dict(nfft=0), b"nfft"), (dict(nfft=64), b"nfft"), (dict(nfft=384), b"nfft"), (dict(nfft=8192), b"nfft"),
    (dict(nfft=-512), b"nfft"),
    (dict(carrier_re=0), b"carrier_re"), (dict(carrier_re=100), b"carrier_re"), (dict(carrier_re=-12), b"carrier_re"),
    (dict(carrier_re=516), b"carrier_re"), (dict(nfft=128, carrier_re=132), b"carrier_re"),
    (dict(scs=60), b"scs"), (dict(scs=0), b"scs"), (dict(scs=120), b"scs"),
    (dict(T=0), b"T="), (dict(T=65536), b"T="), (dict(T=-1), b"T="),
    (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
    (dict(td=None), b"td"), (dict(grid=None), b"grid"),
    (dict(td=ctypes.c_void_p(4100)), b"td"), (dict(grid=ctypes.c_void_p(4100)), b"grid"),
    (dict(dtype=_lib.F64, td=ctypes.c_void_p(4104)), b"td"), (dict(dtype=_lib.F64, grid=ctypes.c_void_p(4104)), b"grid"),
    (dict(ld_td_slot=15 * 512 - 1), b"ld_td_slot"), (dict(ld_td_ant=15 * 512 - 1), b"ld_td_ant"),
    (dict(ld_g_slot=14 * 288 - 1), b"ld_g_slot"), (dict(ld_g_ant=14 * 288 - 1), b"ld_g_ant"),
    (dict(ld_td_slot=0), b"ld_td_slot"), (dict(ld_g_ant=-1), b"ld_g_ant"),
]
REFUSALS = [(c, kw, w) for c in (_demod, _mod) for kw, w in COMMON]
REFUSALS += [(_demod, dict(Nr=n), b"Nr") for n in (0, 3, 8, -1)]
REFUSALS += [(_mod, dict(Nr=n), b"num_ant") for n in (0, 3, 8, -1)]
REFUSALS += [(_mod, dict(dm=ctypes.c_void_p(4100)), b"dm")]


@pytest.mark.parametrize("i", range(len(REFUSALS)), ids=lambda i: f"{REFUSALS[i][0].__name__}-{i}")
def test_unsupported_arguments_are_refused_before_touching_the_gpu(i):
    call, kw, word = REFUSALS[i]
    lib = _lib.lib()
    _bad(lib, call(lib, **kw), word)


def test_every_supported_shape_passes_the_shape_checks():
    """Every nfft, spacing, antenna count and dtype, the smallest and the widest carrier, the
    waveform layout, a size-1 dimension's arbitrary stride and a negative carrier are valid up to
    the buffer check (the last one made)."""
    lib = _lib.lib()
    for call in (_demod, _mod):
        for nfft in phy.OFDM_NFFT:
            for cre in (12, nfft // 12 * 12):
                for scs in (15, 30):
                    for dt in (_lib.F32, _lib.F64):
                        for Nr in (1, 2, 4):
                            _bad(lib, call(lib, nfft=nfft, carrier_re=cre, scs=scs, dtype=dt, Nr=Nr, td=None), b"null")
        _bad(lib, call(lib, ld_td_slot=15 * 512, ld_td_ant=2 * 15 * 512, td=None), b"null")   # [r][slot * S + n]
        _bad(lib, call(lib, T=1, ld_td_slot=0, ld_g_slot=0, td=None), b"null")
        _bad(lib, call(lib, Nr=1, ld_td_ant=0, ld_g_ant=0, ld_td_slot=15 * 512, ld_g_slot=14 * 288, td=None), b"null")
        _bad(lib, call(lib, hz=-3500500000, T=65535, td=None), b"null")
        _bad(lib, call(lib, hz=0, td=None), b"null")


def test_binding_matches_header():
    src = open(os.path.join(ROOT, "include", "ldpc5g.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n in (("ldpc5g_ofdm_demod", 14), ("ldpc5g_ofdm_mod", 15)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name)


def test_fixture_inventory_and_dtypes(golden):
    assert sorted(golden) == sorted(list(ofdm_ref.CASES) + ["DM", "E2E"])
    nffts = set()
    for name, (scs, bw, prbs, nr, mhz, syms) in ofdm_ref.CASES.items():
        c = golden[name]
        nfft = ofdm_ref.nfft_of(prbs)
        nffts.add(nfft)
        n = 14 if syms is None else len(syms)
        assert c["rx"].shape == (nr, n * 12 * prbs) and c["rx"].dtype == np.complex64
        assert c["tx"].shape == (nr, ofdm_ref.sym_slices(name, "td").size) and c["tx"].dtype == np.complex64
        assert 0 < float(c["gap_rx"]) <= GAP_MAX and 0 < float(c["gap_tx"]) <= GAP_MAX
        if nr > 1:   # without the antenna roll the reference is somewhere else entirely
            assert float(c["noroll_rx"]) > 0.1 and float(c["noroll_tx"]) > 0.1
    assert nffts == {256, 512, 1024, 2048, 4096}
    assert golden["DM"]["fd"].dtype == np.complex64 and 0 <= float(golden["DM"]["gap_fd"]) <= GAP_MAX
    e = golden["E2E"]
    assert e["td"].shape == (2, 15 * 512) and e["td"].dtype == np.complex64
    assert bool(e["status"]) and np.array_equal(e["tbblk"][:int(e["meta"][0])], e["trblk"])


@pytest.mark.parametrize("name", sorted(ofdm_ref.CASES))
def test_restatement_reproduces_the_reference(golden, name):
    scs, bw, prbs, nr, mhz, syms = ofdm_ref.CASES[name]
    c = golden[name]
    td, fd = ofdm_ref.case_inputs(name)
    hz = int(mhz * 10 ** 6)
    rx = ofdm_ref.roll(ofdm_ref.demod(td, scs, prbs, hz))[:, ofdm_ref.sym_slices(name, "grid")]
    tx = ofdm_ref.roll(ofdm_ref.mod(fd, scs, prbs, hz))[:, ofdm_ref.sym_slices(name, "td")]
    gr = np.abs(rx - c["rx"]).max() / np.abs(c["rx"]).max()
    gt = np.abs(tx - c["tx"]).max() / np.abs(c["tx"]).max()
    print(name, "gap rx", gr, "tx", gt, "stored", float(c["gap_rx"]), float(c["gap_tx"]))
    assert gr <= float(c["gap_rx"]) * (1 + 1e-6) and gt <= float(c["gap_tx"]) * (1 + 1e-6)


def test_restatement_reproduces_the_reference_with_dm(golden):
    scs, bw, prbs, nr, mhz, _ = ofdm_ref.CASES[ofdm_ref.DM_CASE]
    c = golden["DM"]
    _, fd = ofdm_ref.case_inputs(ofdm_ref.DM_CASE)
    mutated = ofdm_ref.dm_rotate(fd, scs, prbs, ofdm_ref.DM)
    assert not np.array_equal(c["fd"], fd)
    assert np.abs(mutated - c["fd"]).max() / np.abs(c["fd"]).max() <= float(c["gap_fd"]) * (1 + 1e-6)
    tx = ofdm_ref.roll(ofdm_ref.mod(fd, scs, prbs, int(mhz * 10 ** 6), dm=ofdm_ref.DM))
    assert np.abs(tx - c["tx"]).max() / np.abs(c["tx"]).max() <= float(c["gap_tx"]) * (1 + 1e-6)


def test_restatement_round_trip_carries_the_sign_of_the_half_cp():
    """Rx(Tx(x)) = (-1)^h x: the ramp is indexed by position, not by signed frequency.  h = 9 at nfft 256."""
    for scs, prbs, hz in ((30, 11, 0), (30, 11, 3840 * 10 ** 6), (15, 25, 3500500000), (30, 10, 0), (30, 51, 10 ** 9)):
        nfft, cps, S = phy.ofdm_params(scs, prbs)
        x = ofdm_ref.formula_input((2, 14 * 12 * prbs), 7, np.complex128)
        back = ofdm_ref.demod(ofdm_ref.mod(x, scs, prbs, hz), scs, prbs, hz)
        sign = -1 if (cps[1] // 2) % 2 else 1
        assert np.abs(back - sign * x).max() <= 1e-12 * np.abs(x).max(), (scs, prbs)
    assert phy.ofdm_params(30, 11)[1][1] // 2 == 9


def test_formula_input_is_exact_and_spread():
    x = ofdm_ref.formula_input((3, 1000), 5)
    assert x.dtype == np.complex64 and np.array_equal(x * 32, np.round(x * 32)) and np.abs(x * 32).max() <= 43
    assert len(np.unique(x)) > 1500 and not np.array_equal(x, ofdm_ref.formula_input((3, 1000), 6))
    assert np.array_equal(ofdm_ref.formula_input((3, 1000), 5, np.complex128), x.astype(np.complex128))


def test_nr_slot_mirrors_equal_the_pinned_tables():
    assert len(ofdm_ref.PINNED) == 25
    for (scs, bw), (prbs, nfft, rate, cps) in ofdm_ref.PINNED.items():
        assert nr_slot.get_carrier_prb_size(scs, bw) == prbs
        assert nr_slot.get_FFT_IFFT_size(prbs) == nfft
        r, c = nr_slot.get_sample_rate_and_CP_size(scs, bw)
        assert (r, c) == (rate, cps) and all(isinstance(v, int) for v in c)
        assert phy.ofdm_params(scs, prbs) == (nfft, cps, 15 * nfft)
    assert {v[1] for v in ofdm_ref.PINNED.values()} == {256, 512, 1024, 2048, 4096}
    for scs, first, n in ((15, 160, 2048), (30, 352, 4096)):
        sec, smp = nr_slot.get_symbol_timing_offset(scs)
        assert smp[0] == first and smp[13] == 15 * n - n and np.allclose(sec, smp / (n * scs * 1000))
    fd, use = nr_slot.init_fd_slot(2, 24)
    assert fd.shape == use.shape == (2, 14 * 12 * 24) and fd.dtype == np.complex64 and use.dtype == np.int8
    assert not fd.any() and not use.any()
    assert nr_slot.get_REusage_type(32) == "PDSCH-DATA" and nr_slot.get_REusage_value("PUSCH-DMRS") == 61
    assert len(nr_slot.REusage_types) == 22
