"""Host test of the lemma behind the frame kernel's peeled first iteration
(ldpc5g_dec_frame_iter.h, FIRST), stated on the oracle: with the punctured columns 0 and 1 at +0.0
and a zero message state, a row that holds a punctured column sends +-0 to every other column.
So after the first check-node update the column sums are nonzero only in columns 0 and 1 and in
the columns of rows without a punctured column, and no sum is -0.0."""
import numpy as np
import pytest

from oracle import ldpc_oracle as O


@pytest.mark.parametrize("alpha,beta", [(0.75, 0.0), (1.0, 0.5)])
@pytest.mark.parametrize("bg,Zc", [(1, 8), (2, 8), (1, 22), (2, 15)])
def test_first_update_sums(bg, Zc, alpha, beta):
    g = O.graph(bg, Zc)
    T = np.float64
    rng = np.random.default_rng(bg * 100 + Zc)
    B = 6
    llr = rng.normal(size=(B, g.N)) * 4.0
    llr[:, ::7] = -0.0     # planted zeros of both signs, core and extension columns
    llr[:, 3::11] = 0.0
    llr[1] = np.round(llr[1])   # ties
    LQ = np.concatenate([np.zeros((B, 2 * Zc), T), llr], axis=1)
    acc = np.zeros((B, g.Nf), T)
    free_cols = np.zeros(g.Nb, bool)   # base columns of rows without a punctured column
    n_free = 0
    for i in range(g.Mb):
        cols = g.rows_cols(i)
        r = O._cn_update(LQ[:, cols] - T(0), T(alpha), T(beta), T)
        acc[:, cols] += r
        base = g.bj[g.rs[i]:g.rs[i + 1]]
        if base.min() >= 2:
            free_cols[base] = True
            n_free += 1
        else:
            # the row's first edge is its first punctured column; every other message is +-0
            assert base[0] < 2 and not r[:, 1:][:, base[1:] >= 2].any()
            if (base < 2).sum() == 2:
                assert not r.any()
    assert n_free == (0 if bg == 1 else 5)
    nz = (acc != 0).reshape(B, g.Nb, Zc).any(axis=(0, 2))
    assert nz[0] and nz[1]
    assert not (nz[2:] & ~free_cols[2:]).any()
    assert not (np.signbit(acc) & (acc == 0)).any()
    # what the kernel writes for an untouched column, LLR + (+0.0), is the general LLR + sum
    full = LQ + acc
    quiet = np.repeat(~free_cols, Zc)
    quiet[:2 * Zc] = False
    assert np.array_equal(full[:, quiet].view(np.uint64), (LQ[:, quiet] + T(0)).view(np.uint64))
