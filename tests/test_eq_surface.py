"""The equaliser drop-in (python_5gtoolbox_amd/nr_channel_eq.py) exposes the reference's call
surface: the argument names and order of ZF, ZF_IRC, MMSE, MMSE_IRC and channel_equ_and_demod,
compared with the pinned table below on every machine and, where a checkout of the reference is
readable, with the reference's source.  The ML family is refused by name."""
import ast
import inspect
import os

import pytest

from python_5gtoolbox_amd import nr_channel_eq

from test_dropin_surface import REF as PY5GPHY

REF = os.path.join(PY5GPHY, "channel_equalization")

SURFACE = {
    "ZF": ("ZF.py", ["Y", "H", "cov"]),
    "ZF_IRC": ("ZF.py", ["Y", "H", "cov"]),
    "MMSE": ("MMSE.py", ["Y", "H", "cov"]),
    "MMSE_IRC": ("MMSE.py", ["Y", "H", "cov"]),
    "channel_equ_and_demod": ("nr_channel_eq.py", ["Y", "H", "cov", "modtype", "CEQ_config"]),
}


def _ref_args(path, name):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            assert not node.args.defaults
            return [a.arg for a in node.args.args]
    raise AssertionError(f"{name} not in {path}")


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_signature_matches_reference(name):
    path, pinned = SURFACE[name]
    params = [p for p in inspect.signature(getattr(nr_channel_eq, name)).parameters.values()
              if p.kind is not p.KEYWORD_ONLY]
    assert [p.name for p in params] == pinned
    assert all(p.default is p.empty for p in params)
    full = os.path.join(REF, path)
    if os.access(full, os.R_OK):
        assert _ref_args(full, name) == pinned


@pytest.mark.parametrize("algo", ["ML-IRC-soft", "ML-soft", "ML-IRC-hard", "ML-hard", "MMSE-ML", "MMSE-ML-IRC",
                                  "opt-rank2-ML", "opt-rank2-ML-IRC", "ML2-IRC-soft", "ML2-soft", "nonsense"])
def test_other_algorithms_are_refused_by_name(algo):
    with pytest.raises(NotImplementedError, match=algo):
        nr_channel_eq.channel_equ_and_demod(None, None, None, "qpsk", {"algo": algo})


def test_linear_algorithm_names():
    from python_5gtoolbox_amd import _lib
    assert tuple(nr_channel_eq.LINEAR_ALGOS) == ("ZF", "ZF-IRC", "MMSE", "MMSE-IRC")
    assert sorted(_lib.EQ_ALGO) == sorted(nr_channel_eq.LINEAR_ALGOS)
