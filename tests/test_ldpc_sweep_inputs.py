"""CPU: the inputs of the all-lifting-sizes sweep (tests/test_gpu_ldpc_sweep.py) can tell a right
decoder from a wrong one.  The recipe (ldpc_sweep_ref.sweep_input) runs through the oracle alone:

  * every (bg, Zc, schedule) launch of the float32 sweep holds a codeblock that converges and one
    that does not, stopping at two or more different iteration counts, so early exit, the
    exhausted path and per-codeblock stop masks are all exercised at every size;
  * between a quarter and three quarters of all codeblocks fail, per base graph and schedule;
  * the rate-matched inputs still converge somewhere, and their zeroed tail covers at least one
    whole barrier group of rows (a skipped group) and cuts another one (a partly dead group);
  * one circulant shift off by one changes the outputs: a wrong wrap or shift cannot pass.
"""
import copy

import numpy as np
import pytest

import ldpc_sweep_ref as S
from oracle import ldpc_oracle as O

SCHEDULES = (("layered", "layered"), ("flooding", "flooding-f32"))   # (schedule, path tag)

# (bg, Zc, schedule) launches allowed to miss the mixed-outcome bar: at most 3 % of the 204.  None does.
EXEMPT = ()
MAX_EXEMPT = 6


def _decode_all(rm):
    out = {}
    for schedule, tag in SCHEDULES:
        for bg, Zc in S.PAIRS:
            B = S.batch_size(Zc, schedule == "layered")
            _, llr = S.sweep_input(bg, Zc, tag + ("-rm" if rm else ""), B, np.float32, S.n_zeroed(Zc) if rm else 0)
            _, st, it = S.oracle_decode(llr, bg, Zc, schedule)
            out[(bg, Zc, schedule)] = (st, it)
    return out


@pytest.fixture(scope="module")
def plain():
    return _decode_all(False)


@pytest.mark.slow
def test_every_launch_has_mixed_outcomes(plain):
    assert len(plain) == 204 and len(EXEMPT) <= MAX_EXEMPT
    missed = []
    for key, (st, it) in plain.items():
        assert st.size >= 5
        if st.all() or not st.any() or np.unique(it).size < 2:
            missed.append(key)
    assert sorted(missed) == sorted(EXEMPT), missed


@pytest.mark.slow
def test_failure_rate_per_base_graph_and_schedule(plain):
    for schedule, _ in SCHEDULES:
        for bg in (1, 2):
            st = np.concatenate([v[0] for k, v in plain.items() if k[0] == bg and k[2] == schedule])
            assert 0.25 <= 1 - st.mean() <= 0.75, (bg, schedule, 1 - st.mean())


@pytest.mark.slow
def test_rate_matched_inputs_converge_somewhere():
    for key, (st, it) in _decode_all(True).items():
        assert st.any(), key


def test_row_groups_restate_the_kernels():
    """32 / 28 barrier groups (ldpc5g_dec_body.h RowGroups), rows 0 ... 3 each alone."""
    for bg, n in ((1, 32), (2, 28)):
        gr = S.row_groups(bg)
        assert len(gr) == n and gr[:4] == [(0, 1), (1, 2), (2, 3), (3, 4)]
        assert gr[-1][1] == S.DIMS[bg][3] and all(a[1] == b[0] for a, b in zip(gr, gr[1:]))


def test_zeroed_tail_covers_and_cuts_row_groups():
    """From the graph: in every rate-matched input the dead rows (those whose degree-1 column is
    zeroed) contain a whole row group, which the dead-row kernels skip together with its barrier;
    the zeroed columns are exactly those rows' extension columns; and over the sweep the cut falls
    both on group boundaries and inside a group (a group with live and dead rows)."""
    inside = boundary = 0
    for bg, Zc in S.PAIRS:
        nz = S.n_zeroed(Zc)
        Kb, _, Nb, Mb = S.DIMS[bg]
        g = O.graph(bg, Zc)
        dead = S.dead_rows(bg, nz)
        for i in dead:   # row i's last edge is its own degree-1 column Kb + i, among the zeroed ones
            j = int(g.bj[g.rs[i + 1] - 1])
            assert j == Kb + i >= Nb - nz and (g.bj == j).sum() == 1
        groups = S.row_groups(bg)
        assert any(set(range(a, b)) <= dead for a, b in groups), (bg, Zc)
        cut = Mb - nz
        if any(a < cut < b for a, b in groups):
            inside += 1
        else:
            boundary += 1
        _, llr = S.sweep_input(bg, Zc, "layered-rm", 2, np.float32, nz)
        assert not llr[:, -nz * Zc:].any() and not np.signbit(llr[:, -nz * Zc:]).any()
        assert (llr[:, -(nz + 1) * Zc:-nz * Zc] != 0).all()
    assert inside >= 10 and boundary >= 10, (inside, boundary)


def _perturbed(bg, Zc, edge):
    """The (bg, Zc) graph with the circulant shift of base edge `edge` increased by one."""
    g = copy.copy(O.graph(bg, Zc))
    g.bv = g.bv.copy()
    g.ecol = g.ecol.copy()
    g.bv[edge] = (g.bv[edge] + 1) % Zc
    g.ecol[edge] = g.bj[edge] * Zc + (np.arange(Zc) + g.bv[edge]) % Zc
    return g


# one or two sizes of every lifting set among 104 ... 352
SENSITIVITY = [(1, 128), (2, 192), (1, 160), (2, 112), (1, 144), (2, 176), (1, 104), (2, 120), (1, 208), (2, 352)]


@pytest.mark.parametrize("pair", SENSITIVITY, ids=S.pair_id)
def test_one_shift_off_by_one_changes_the_outputs(monkeypatch, pair):
    """Decode the sweep input with a graph in which one circulant shift is one too large: a core
    edge of row 1, and the degree-1 edge of the last row.  ck, status or iters must differ from
    the true graph's for both schedules, so a kernel with a wrong wrap at that size fails the
    sweep.  (The oracle's decoders look the graph up by name; only that lookup is redirected.)"""
    bg, Zc = pair
    assert {O.find_iLS(z) for _, z in SENSITIVITY} == set(range(8))
    true = O.graph(bg, Zc)
    for schedule, tag in SCHEDULES:
        _, llr = S.sweep_input(bg, Zc, tag, 5, np.float32)
        ref = S.oracle_decode(llr, bg, Zc, schedule)
        assert ref[1].any()
        for edge in (int(true.rs[1]) + 2, len(true.bi) - 1):
            bad = _perturbed(bg, Zc, edge)
            with monkeypatch.context() as m:
                m.setattr(O, "graph", lambda b, z: bad)
                got = S.oracle_decode(llr, bg, Zc, schedule)
            assert O.graph(bg, Zc) is true
            assert not np.array_equal(got[0], ref[0]) or not np.array_equal(got[1], ref[1]), (schedule, edge)
