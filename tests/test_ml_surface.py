"""The ML drop-ins (python_5gtoolbox_amd/ML.py, ML2.py, MMSE_ML.py, opt_rank2_ML.py,
nr_channel_eq_ml.py) expose the reference's call surface: argument names, order and defaults,
compared with the pinned table below on every machine and, where a checkout of the reference is
readable, with the reference's source.  nr_channel_eq_ml accepts all fourteen algorithm names."""
import ast
import importlib
import inspect
import os
import warnings

import pytest

from test_dropin_surface import REF as PY5GPHY

REF = os.path.join(PY5GPHY, "channel_equalization")
SOFT = ["Y", "H", "cov", "modtype", ("demod_decision", "soft")]

SURFACE = {
    ("ML", "ML"): SOFT, ("ML", "ML_IRC"): SOFT,
    ("ML2", "ML"): SOFT, ("ML2", "ML_IRC"): SOFT,
    ("MMSE_ML", "MMSE_ML"): ["Y", "H", "cov", "modtype"], ("MMSE_ML", "MMSE_ML_IRC"): ["Y", "H", "cov", "modtype"],
    ("opt_rank2_ML", "opt_rank2_ML"): SOFT, ("opt_rank2_ML", "opt_rank2_ML_IRC"): SOFT,
    ("nr_channel_eq_ml", "channel_equ_and_demod"): ["Y", "H", "cov", "modtype", "CEQ_config"],
}
REF_FILE = {"nr_channel_eq_ml": "nr_channel_eq.py"}
FOURTEEN = ["ZF", "ZF-IRC", "MMSE", "MMSE-IRC", "ML-IRC-soft", "ML-soft", "ML-IRC-hard", "ML-hard", "MMSE-ML",
            "MMSE-ML-IRC", "opt-rank2-ML", "opt-rank2-ML-IRC", "ML2-IRC-soft", "ML2-soft"]


def _ref_args(path, name):
    with warnings.catch_warnings():   # the reference's docstrings hold invalid escape sequences
        warnings.simplefilter("ignore")
        tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            args = [a.arg for a in node.args.args]
            for k, d in enumerate(reversed(node.args.defaults)):
                args[-1 - k] = (args[-1 - k], ast.literal_eval(d))
            return args
    raise AssertionError(f"{name} not in {path}")


@pytest.mark.parametrize("module,name", sorted(SURFACE))
def test_signature_matches_reference(module, name):
    pinned = SURFACE[(module, name)]
    fn = getattr(importlib.import_module("python_5gtoolbox_amd." + module), name)
    params = [p for p in inspect.signature(fn).parameters.values() if p.kind is not p.KEYWORD_ONLY]
    assert [p.name if p.default is p.empty else (p.name, p.default) for p in params] == pinned
    full = os.path.join(REF, REF_FILE.get(module, module + ".py"))
    if os.access(full, os.R_OK):
        assert _ref_args(full, name) == pinned


def test_all_fourteen_names_are_accepted():
    from python_5gtoolbox_amd import _lib, nr_channel_eq, nr_channel_eq_ml
    assert sorted(nr_channel_eq_ml.ALGOS) == sorted(FOURTEEN)
    assert sorted(nr_channel_eq_ml.ML_ALGOS) == sorted(set(FOURTEEN) - set(nr_channel_eq.LINEAR_ALGOS))
    assert sorted(_lib.ML_ALGO) == sorted(nr_channel_eq_ml.ML_ALGOS)
    path = os.path.join(REF, "nr_channel_eq.py")
    if os.access(path, os.R_OK):   # the names the reference's dispatcher compares against
        names = [n.value for n in ast.walk(ast.parse(open(path).read()))
                 if isinstance(n, ast.Constant) and isinstance(n.value, str) and n.value in FOURTEEN]
        assert sorted(set(names)) == sorted(FOURTEEN)


def test_an_unknown_name_is_refused_by_name():
    from python_5gtoolbox_amd import nr_channel_eq_ml
    with pytest.raises(AssertionError, match="nonsense"):
        nr_channel_eq_ml.channel_equ_and_demod(None, None, None, "qpsk", {"algo": "nonsense"})
