"""The call surface of PUSCH transform precoding: the drop-ins (python_5gtoolbox_amd/lowPAPR_seq.py,
nr_pusch_process.py, nr_pusch_dmrs.pusch_dmrs_LS_est_tp) carry the reference's names and argument
order — compared with the pinned table on every machine and, where a checkout of the reference is
readable, with its source — the batched functions exist with their documented arguments, every
refusal arrives before any GPU work, and without a GPU every new entry point raises."""
import inspect
import os

import numpy as np
import pytest

import tp_ref
from python_5gtoolbox_amd import _lib, lowPAPR_seq, nr_pusch_dmrs, nr_pusch_process, phy, sch

from test_dropin_surface import REF as PY5GPHY
from test_slot_surface import _ref_function

FUNCTIONS = {
    ("lowPAPR_seq", "gen_lowPAPR_seq"): (lowPAPR_seq, "common/lowPAPR_seq.py", ["u", "v", "alpha", "MZC"]),
    ("nr_pusch_process", "nr_pusch_process"): (
        nr_pusch_process, "nr_pusch/nr_pusch_process.py",
        ["g_seq", "rnti", "nID", "Qm", "num_of_layers", "nTransPrecode", "RBSize", "nNrOfAntennaPorts", "precoding_matrix"]),
}


@pytest.mark.parametrize("key", sorted(FUNCTIONS))
def test_function_signature_matches_reference(key):
    mod, path, pinned = FUNCTIONS[key]
    params = list(inspect.signature(getattr(mod, key[1])).parameters.values())
    assert [p.name for p in params] == pinned
    assert all(p.default is p.empty for p in params)
    full = os.path.join(PY5GPHY, path)
    if os.access(full, os.R_OK):
        assert _ref_function(full, key[1]) == (pinned, 0)


def test_batched_surface_exists():
    for fn, first in ((phy.transform_precode, ["x", "rb_size", "inverse", "out"]),
                      (phy.low_papr_seq, ["u", "v", "MZC", "alpha"]),
                      (phy.pusch_tp_frontend, ["grid", "slots", "pusch_config", "want", "base_seq"]),
                      (phy.pusch_tp_map, ["sym", "slots", "pusch_config", "carrier_prbs", "num_ant", "precoding", "out",
                                          "re_idx", "base_seq"]),
                      (sch.sch_pusch_tp_rx_batch, ["grid", "slots", "pusch_config", "ce", "algo", "mod", "cfg", "L",
                                                   "re_idx", "base_seq"]),
                      (nr_pusch_dmrs.pusch_dmrs_LS_est_tp, ["fd_slot_data", "pusch_config", "slot", "base_seq"])):
        assert list(inspect.signature(fn).parameters)[:len(first)] == first
    sig = inspect.signature(phy.transform_precode).parameters
    assert sig["inverse"].default is False and sig["out"].default is None
    assert inspect.signature(phy.low_papr_seq).parameters["alpha"].default == 0.0
    sig = inspect.signature(phy.pusch_tp_frontend).parameters
    assert sig["want"].default == ("h_ls", "y") and sig["base_seq"].default is None
    sig = inspect.signature(phy.pusch_tp_map).parameters
    assert all(sig[k].default is None for k in ("precoding", "out", "re_idx", "base_seq"))
    sig = inspect.signature(sch.sch_pusch_tp_rx_batch).parameters
    assert sig["re_idx"].default is None and sig["base_seq"].default is None


GRID = np.zeros((2, 14 * 12 * 24), np.complex64)


def _cfg(rb_size=16, **kw):
    return tp_ref.pusch_config(rb_start=0, rb_size=rb_size, **kw)


def _every_entry(cfg, base_seq=None):
    """Each way into the feature that takes a pusch_config, with no device argument at all."""
    return [lambda: phy.pusch_tp_frontend(None, None, cfg, base_seq=base_seq),
            lambda: phy.pusch_tp_map(None, None, cfg, 24, 1, base_seq=base_seq),
            lambda: sch.sch_pusch_tp_rx_batch(None, None, cfg, {}, "ZF", 2, None, 8, base_seq=base_seq),
            lambda: nr_pusch_dmrs.pusch_dmrs_LS_est_tp(GRID, cfg, 0, base_seq=base_seq)]


@pytest.mark.parametrize("rb", [7, 11, 14, 22, 275])
def test_an_allocation_the_transform_is_not_built_for_is_refused(rb):
    for call in _every_entry(_cfg(rb)):
        with pytest.raises(NotImplementedError, match="RBSize"):
            call()
    with pytest.raises(NotImplementedError, match="RBSize"):
        phy.transform_precode(None, rb)
    with pytest.raises(NotImplementedError, match="RBSize"):
        nr_pusch_process.nr_pusch_process(np.zeros(24 * rb, np.int8), 1, 1, 2, 1, 1, rb, 1, np.ones(1))


def test_short_allocations_need_base_seq():
    for rb in (1, 2, 3, 4):
        for call in _every_entry(_cfg(rb)):
            with pytest.raises(NotImplementedError, match="RBSize <= 4.*base_seq"):
                call()
    for MZC in (6, 12, 18, 24):
        with pytest.raises(NotImplementedError, match="MZC"):
            phy.low_papr_seq(0, 0, MZC)
        with pytest.raises(NotImplementedError, match="MZC"):
            lowPAPR_seq.gen_lowPAPR_seq(0, 0, 0, MZC)


def test_the_reference_asserts_are_assertion_errors():
    bad = [_cfg(), _cfg(), _cfg(), _cfg(), _cfg(), _cfg(), _cfg()]
    bad[0]["nTransPrecode"] = 0
    bad[1]["num_of_layers"], bad[1]["PortIndexList"] = 2, [1000, 1001]
    bad[2]["DMRS"]["NumCDMGroupsWithoutData"] = 1   # the reference's assert demod_LLRs.size % MPUSCHSC == 0 fails
    bad[3]["DMRS"]["DMRSConfigType"] = 2
    bad[4]["DMRS"]["dmrs_TypeA_Position"] = "pos3"
    bad[5]["DMRS"]["transformPrecodingEnabled"]["nPuschID"] = 1008
    bad[6]["DMRS"]["transformPrecodingEnabled"]["groupOrSequenceHopping"] = "both"
    for cfg in bad:
        for call in _every_entry(cfg):
            with pytest.raises(AssertionError):
                call()
    for args in ((30, 0, 0, 36), (0, 1, 0, 36), (0, 2, 0, 72), (0, 0, 0, 35)):
        with pytest.raises(AssertionError):
            lowPAPR_seq.gen_lowPAPR_seq(*args)
    with pytest.raises(AssertionError):
        phy.low_papr_seq([0, 30], [0, 0], 72)
    with pytest.raises(AssertionError):
        phy.low_papr_seq(0, 0, 3306)


def test_other_refusals_come_before_any_gpu_work():
    for algo in ("ML-soft", "MMSE-ML", "opt-rank2-ML-IRC"):   # the reference throws their LLRs away on this branch
        with pytest.raises(NotImplementedError, match="ML"):
            sch.sch_pusch_tp_rx_batch(None, None, _cfg(), {}, algo, 2, None, 8)
    with pytest.raises(AssertionError, match="algo"):
        sch.sch_pusch_tp_rx_batch(None, None, _cfg(), {}, "LMMSE", 2, None, 8)
    with pytest.raises(AssertionError, match="want"):
        phy.pusch_tp_frontend(None, None, _cfg(), want=("h",))
    with pytest.raises(NotImplementedError, match="UCI"):
        nr_pusch_process.nr_pusch_process(np.array([0, 1, -1, -2] * 48), 1, 1, 2, 1, 1, 1, 1, np.ones(1))
    with pytest.raises(AssertionError):
        nr_pusch_process.nr_pusch_process(np.zeros(2 * 13, np.int8), 1, 1, 2, 1, 1, 1, 1, np.ones(1))   # not whole symbols


def test_the_old_entry_points_keep_refusing_and_point_here():
    with pytest.raises(NotImplementedError, match="nTransPrecode.*pusch_tp_frontend"):
        phy.slot_frontend(None, None, _cfg())
    with pytest.raises(NotImplementedError, match="nTransPrecode"):
        nr_pusch_dmrs.pusch_dmrs_LS_est(GRID, _cfg(), 0)


def test_data_re_idx_of_a_transform_precoded_allocation():
    cfg = _cfg(5, add_pos=1)
    re_idx, usage = phy.pusch_tp_data_re_idx(cfg)
    ref_idx, ref_usage = tp_ref.data_re_idx(cfg)
    assert re_idx.dtype == np.int32 and np.array_equal(re_idx, ref_idx) and np.array_equal(usage, ref_usage)
    assert len(re_idx) == 10 * 60   # whole symbols: two DMRS symbols carry no data
    assert sum(phy.tp_rb_ok(n) for n in range(-3, 400)) == 53 and [n for n in tp_ref.RB_SIZES if not phy.tp_rb_ok(n)] == []


def test_every_new_entry_point_raises_without_a_gpu(monkeypatch):
    """No CPU fallback.  torch.cuda.is_available is patched so the test says the same on every machine."""
    torch = _lib.torch()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = _cfg(add_pos=1)
    grid = torch.zeros((1, 2, 14 * 12 * 24), dtype=torch.complex64)
    slots = torch.zeros((1,), dtype=torch.int32)
    sym = torch.zeros((1, len(phy.pusch_tp_data_re_idx(cfg)[0])), dtype=torch.complex64)
    short = np.ones((1, 12), np.complex128)
    calls = [lambda: phy.transform_precode(sym, 16),
             lambda: phy.low_papr_seq(3, 1, 72),
             lambda: phy.pusch_tp_frontend(grid, slots, cfg),
             lambda: phy.pusch_tp_frontend(grid, slots, _cfg(2), base_seq=short),
             lambda: phy.pusch_tp_map(sym, slots, cfg, 24, 1),
             lambda: sch.sch_pusch_tp_rx_batch(grid, slots, cfg, {}, "MMSE", 2, None, 8),
             lambda: lowPAPR_seq.gen_lowPAPR_seq(3, 1, 0.5, 72),
             lambda: nr_pusch_process.nr_pusch_process(np.zeros(2 * 192, np.int8), 1, 1, 2, 1, 1, 16, 1, np.ones(1)),
             lambda: nr_pusch_dmrs.pusch_dmrs_LS_est_tp(GRID, cfg, 0)]
    for call in calls:
        with pytest.raises(_lib.LdpcLibError, match="no ROCm GPU"):
            call()
