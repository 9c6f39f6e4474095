"""The call surface of the OFDM low-PHY: the drop-ins (python_5gtoolbox_amd/nr_slot.py,
rx_lowphy_process.py, tx_lowphy_process.py) carry the reference's names, argument order and
defaults — compared with the pinned table on every machine and, where a checkout of the reference
is readable, with its source — the batched functions exist with their documented arguments, every
refusal arrives before any GPU work, and without a GPU every new entry point raises."""
import inspect
import os

import numpy as np
import pytest

import slot_ref
import tp_ref
from python_5gtoolbox_amd import _lib, nr_slot, phy, rx_lowphy_process, sch, tx_lowphy_process

from test_dropin_surface import REF as PY5GPHY
from test_slot_surface import _ref_function

# (module, function) -> (module object, path in the reference, parameters, number of defaults)
FUNCTIONS = {
    ("nr_slot", "init_fd_slot"): (nr_slot, "common/nr_slot.py", ["num_of_ant", "carrier_prbsize"], 0),
    ("nr_slot", "get_REusage_type"): (nr_slot, "common/nr_slot.py", ["value"], 0),
    ("nr_slot", "get_REusage_value"): (nr_slot, "common/nr_slot.py", ["type"], 0),
    ("nr_slot", "get_carrier_prb_size"): (nr_slot, "common/nr_slot.py", ["scs", "BW"], 0),
    ("nr_slot", "get_FFT_IFFT_size"): (nr_slot, "common/nr_slot.py", ["carrier_prb_size"], 0),
    ("nr_slot", "get_symbol_timing_offset"): (nr_slot, "common/nr_slot.py", ["scs"], 0),
    ("nr_slot", "get_sample_rate_and_CP_size"): (nr_slot, "common/nr_slot.py", ["scs", "BW"], 0),
    ("rx_lowphy_process", "Rx_low_phy"): (rx_lowphy_process, "nr_lowphy/rx_lowphy_process.py", ["td_slot", "carrier_config"], 0),
    ("rx_lowphy_process", "channel_filter"): (rx_lowphy_process, "nr_lowphy/rx_lowphy_process.py",
                                              ["rx_waveform", "carrier_config", "sample_rate_in_hz"], 0),
    ("rx_lowphy_process", "waveform_rx_processing"): (rx_lowphy_process, "nr_lowphy/rx_lowphy_process.py",
                                                      ["rx_waveform", "carrier_config", "sample_rate_in_hz"], 0),
    ("tx_lowphy_process", "Tx_low_phy"): (tx_lowphy_process, "nr_lowphy/tx_lowphy_process.py",
                                          ["fd_slot", "carrier_config", "Dm"], 1),
    ("tx_lowphy_process", "channel_filter"): (tx_lowphy_process, "nr_lowphy/tx_lowphy_process.py",
                                              ["td_waveform", "carrier_config", "sample_rate_in_hz"], 0),
}
CARRIER = {"carrier_frequency_in_mhz": 3840, "BW": 10, "scs": 30, "num_of_ant": 2, "Nr": 2}


@pytest.mark.parametrize("key", sorted(FUNCTIONS))
def test_function_signature_matches_reference(key):
    mod, path, pinned, ndef = FUNCTIONS[key]
    params = list(inspect.signature(getattr(mod, key[1])).parameters.values())
    assert [p.name for p in params] == pinned
    assert sum(p.default is not p.empty for p in params) == ndef
    full = os.path.join(PY5GPHY, path)
    if os.access(full, os.R_OK):
        assert _ref_function(full, key[1]) == (pinned, ndef)


def test_defaults_and_tables():
    assert inspect.signature(tx_lowphy_process.Tx_low_phy).parameters["Dm"].default == []
    assert nr_slot.REusage_types[0] == "empty" and nr_slot.REusage_types[67] == "PUSCH-CSI2"


def test_batched_surface_exists():
    for fn, first in ((phy.ofdm_params, ["scs", "carrier_prbs"]),
                      (phy.ofdm_demod, ["td", "scs", "carrier_prbs", "carrier_frequency_in_mhz", "out"]),
                      (phy.ofdm_mod, ["grid", "scs", "carrier_prbs", "carrier_frequency_in_mhz", "dm", "out"]),
                      (sch.sch_td_rx_batch, ["td", "slots", "config", "carrier", "ce", "algo", "mod", "cfg", "L", "kw"])):
        assert list(inspect.signature(fn).parameters) == first
    sig = inspect.signature(phy.ofdm_demod).parameters
    assert sig["carrier_frequency_in_mhz"].default == 0 and sig["out"].default is None
    sig = inspect.signature(phy.ofdm_mod).parameters
    assert sig["carrier_frequency_in_mhz"].default == 0 and sig["dm"].default is None and sig["out"].default is None
    assert inspect.signature(sch.sch_td_rx_batch).parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD


def test_ofdm_params():
    assert phy.ofdm_params(30, 273) == (4096, [352] + [288] * 13, 61440)
    assert phy.ofdm_params(15, 25) == (512, [40] + [36] * 6 + [40] + [36] * 6, 7680)
    assert phy.ofdm_params(30, 11)[:2] == (256, [22] + [18] * 13)
    assert phy.ofdm_params(30, 5)[0] == 128 and phy.ofdm_params(30, 9)[0] == 128 and phy.ofdm_params(30, 10)[0] == 256
    for prbs in range(1, 400):
        nfft = nr_slot.get_FFT_IFFT_size(prbs)
        if nfft in phy.OFDM_NFFT:
            assert phy.ofdm_params(15, prbs)[0] == nfft
        else:   # prbs 1..4 (nfft 16..64) and above 290 (nfft 8192): Rx_low_phy's own assert
            assert prbs < 5 or prbs > 290
            with pytest.raises(NotImplementedError, match="nfft"):
                phy.ofdm_params(15, prbs)


def test_the_filters_are_refused_before_any_gpu_work():
    w = np.zeros((2, 100), np.complex64)
    for call in (lambda: rx_lowphy_process.channel_filter(w, CARRIER, 245.76e6),
                 lambda: rx_lowphy_process.waveform_rx_processing(w, CARRIER, 245.76e6),
                 lambda: tx_lowphy_process.channel_filter(w, CARRIER, 245.76e6)):
        with pytest.raises(NotImplementedError, match="channel_filter"):
            call()


def test_other_refusals_come_before_any_gpu_work():
    for scs in (60, 120, 7):
        with pytest.raises(NotImplementedError, match="scs"):
            phy.ofdm_demod(None, scs, 24)
        with pytest.raises(NotImplementedError, match="scs"):
            phy.ofdm_mod(None, scs, 24)
    for prbs in (342, 400):   # nfft 8192
        with pytest.raises(NotImplementedError, match="nfft"):
            phy.ofdm_demod(None, 30, prbs)
        with pytest.raises(NotImplementedError, match="nfft"):
            phy.ofdm_mod(None, 30, prbs)
    with pytest.raises(KeyError):   # as the reference: a bandwidth that is not in its table
        rx_lowphy_process.Rx_low_phy(np.zeros((2, 7680), np.complex64), dict(CARRIER, BW=7))
    with pytest.raises(AssertionError, match="td_slot"):
        rx_lowphy_process.Rx_low_phy(np.zeros((2, 7679), np.complex64), CARRIER)
    with pytest.raises(AssertionError, match="fd_slot"):
        tx_lowphy_process.Tx_low_phy(np.zeros((1, 14 * 288), np.complex64), CARRIER)
    with pytest.raises(NotImplementedError, match="subcarriers"):
        tx_lowphy_process.Tx_low_phy(np.zeros((2, 14 * 276), np.complex64), CARRIER)
    pdsch = slot_ref.pdsch_config(rb_start=0, rb_size=16, ports=[1000])
    with pytest.raises(AssertionError, match="algo"):
        sch.sch_td_rx_batch(None, None, pdsch, CARRIER, {}, "LMMSE", 2, None, 8)
    pusch = tp_ref.pusch_config(rb_start=0, rb_size=16)
    with pytest.raises(NotImplementedError, match="ML"):
        sch.sch_td_rx_batch(None, None, pusch, CARRIER, {}, "ML-soft", 2, None, 8)
    with pytest.raises(NotImplementedError, match="RBSize"):
        sch.sch_td_rx_batch(None, None, tp_ref.pusch_config(rb_start=0, rb_size=7), CARRIER, {}, "MMSE", 2, None, 8)
    with pytest.raises(NotImplementedError, match="scs"):
        sch.sch_td_rx_batch(None, None, pdsch, dict(CARRIER, scs=60, BW=100), {}, "MMSE", 2, None, 8)


def test_every_new_entry_point_raises_without_a_gpu(monkeypatch):
    """No CPU fallback.  torch.cuda.is_available is patched so the test says the same on every machine."""
    torch = _lib.torch()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    td = torch.zeros((1, 2, 7680), dtype=torch.complex64)
    grid = torch.zeros((1, 2, 14 * 288), dtype=torch.complex64)
    slots = torch.zeros((1,), dtype=torch.int32)
    pdsch = slot_ref.pdsch_config(rb_start=0, rb_size=16, ports=[1000])
    pusch = tp_ref.pusch_config(rb_start=0, rb_size=16)
    fd = np.ones((2, 14 * 288), np.complex64)
    calls = [lambda: phy.ofdm_demod(td, 30, 24),
             lambda: phy.ofdm_mod(grid, 30, 24, 3840, dm=[0.0] * 14),
             lambda: sch.sch_td_rx_batch(td, slots, pdsch, CARRIER, {}, "MMSE", 2, None, 8),
             lambda: sch.sch_td_rx_batch(td, slots, pusch, CARRIER, {}, "MMSE", 2, None, 8),
             lambda: rx_lowphy_process.Rx_low_phy(td[0].numpy(), CARRIER),
             lambda: tx_lowphy_process.Tx_low_phy(fd, CARRIER),
             lambda: tx_lowphy_process.Tx_low_phy(fd, CARRIER, [1e-7] * 14)]
    for call in calls:
        with pytest.raises(_lib.LdpcLibError, match="no ROCm GPU"):
            call()
    assert np.all(fd == 1)   # the refusal came before Dm touched the caller's array
