"""The channel-estimation drop-ins (python_5gtoolbox_amd/dft_dct_CE.py, dft_dct_symmetric_CE.py,
nr_channel_estimation.py) expose the reference's call surface: names, argument names and order,
compared with the pinned table below on every machine and, where a checkout of the reference is
readable, with the reference's source.  The options that are not provided are refused by name
before any GPU work."""
import ast
import inspect
import os

import numpy as np
import pytest

from python_5gtoolbox_amd import dft_dct_CE, dft_dct_symmetric_CE, nr_channel_estimation, sch, phy

from test_dropin_surface import REF as PY5GPHY

REF = os.path.join(PY5GPHY, "channel_estimate")

FUNCTIONS = {
    "DFT_DCT_channel_estimate": (dft_dct_CE, "dft_dct_CE.py", ["H_LS", "RS_info", "CE_config", "model"]),
    "DFT_DCT_symmetric_channel_estimate": (dft_dct_symmetric_CE, "dft_dct_symmetric_CE.py",
                                           ["H_LS", "RS_info", "CE_config", "model"]),
}
METHODS = {
    "__init__": ["self", "H_LS", "RS_info", "CE_config"],
    "channel_est": ["self", "freq_offset"],
    "timing_offset_est": ["self"],
    "comp_H_LS_timing_offset": ["self"],
    "process_pdsch_data": ["self", "pdsch_resource", "pdsch_start_sym"],
}


def _ref_function_args(path, name):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return [a.arg for a in node.args.args]
    raise AssertionError(f"{name} not in {path}")


def _ref_method_args(path, cls, name):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name == name:
                    return [a.arg for a in sub.args.args]
    raise AssertionError(f"{cls}.{name} not in {path}")


@pytest.mark.parametrize("name", sorted(FUNCTIONS))
def test_function_signature_matches_reference(name):
    mod, path, pinned = FUNCTIONS[name]
    params = list(inspect.signature(getattr(mod, name)).parameters.values())
    assert [p.name for p in params] == pinned
    assert all(p.default is p.empty for p in params)
    full = os.path.join(REF, path)
    if os.access(full, os.R_OK):
        assert _ref_function_args(full, name) == pinned


@pytest.mark.parametrize("name", sorted(METHODS))
def test_method_signature_matches_reference(name):
    pinned = METHODS[name]
    fn = getattr(nr_channel_estimation.NrChannelEstimation, name)
    assert [p.name for p in inspect.signature(fn).parameters.values()] == pinned
    if name == "channel_est":
        assert inspect.signature(fn).parameters["freq_offset"].default is None
    full = os.path.join(REF, "nr_channel_estimation.py")
    if os.access(full, os.R_OK):
        assert _ref_method_args(full, "NrChannelEstimation", name) == pinned


def _config(**kw):
    cfg = {"enable_TO_comp": False, "enable_FO_est": False, "enable_FO_comp": False, "CE_algo": "DFT_symmetric",
           "L_symm_left_in_ns": 1400, "L_symm_right_in_ns": 1200, "eRB": 4}
    cfg.update(kw)
    return cfg


RS_INFO = {"RE_distance": 4, "scs": 30, "RSSymMap": [2, 11], "NumCDMGroupsWithoutData": 2}
H_LS = np.ones((2, 60, 2, 2), np.complex64)


@pytest.mark.parametrize("kw,word", [(dict(enable_FO_est=True), "enable_FO_est"),
                                     (dict(enable_FO_comp=True), "enable_FO_comp"),
                                     (dict(freq_intp_method="CubicSpline"), "CubicSpline"),
                                     (dict(freq_intp_method="PchipInterpolator"), "PchipInterpolator")])
def test_refused_options_raise_not_implemented(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        nr_channel_estimation.NrChannelEstimation(H_LS.copy(), dict(RS_INFO), _config(**kw))
    for fn in (dft_dct_CE.DFT_DCT_channel_estimate, dft_dct_symmetric_CE.DFT_DCT_symmetric_channel_estimate):
        with pytest.raises(NotImplementedError, match=word):
            fn(H_LS.copy(), dict(RS_INFO), _config(**kw), "DFT")


def test_freq_offset_argument_is_refused_and_defaults_are_filled():
    cfg = _config()
    ce = nr_channel_estimation.NrChannelEstimation(H_LS.copy(), dict(RS_INFO), cfg)
    assert cfg["freq_intp_method"] == "linear" and cfg["timing_intp_method"] == "linear"
    with pytest.raises(NotImplementedError, match="freq_offset"):
        ce.channel_est(freq_offset=120.0)
    with pytest.raises(AssertionError):
        nr_channel_estimation.NrChannelEstimation(H_LS.copy(), dict(RS_INFO, scs=60), _config())
    with pytest.raises(AssertionError):
        nr_channel_estimation.NrChannelEstimation(H_LS.copy(), dict(RS_INFO, RSSymMap=[2]), _config())


def test_batched_surface_exists():
    for fn, first in ((phy.channel_estimate, ["h_ls", "sym_map", "algo", "scs", "eRB", "l_left_ns", "l_right_ns"]),
                      (phy.to_compensate, ["y", "to_avg", "scs"]),
                      (sch.sch_ce_eq_rx_batch, ["y", "h_ls", "ce", "algo", "re_idx", "mod", "cfg", "L"]),
                      (sch.sch_ce_ml_rx_batch, ["y", "h_ls", "ce", "algo", "re_idx", "mod", "cfg", "L"])):
        assert list(inspect.signature(fn).parameters)[:len(first)] == first
    sig = inspect.signature(phy.channel_estimate).parameters
    assert sig["re_distance"].default == 4 and sig["num_cdm_groups"].default == 2
    assert sig["to_comp"].default is False and sig["want"].default == ()
