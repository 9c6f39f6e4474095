"""Host test of the identity behind the frame kernel's fused start (ldpc5g_dec_frame_iter.h, FUSED),
stated on the oracle.  BG1, punctured columns 0 and 1 at +0.0, zero message state, and a zero
minimum's message alpha * max(0 - beta, 0) = +-0:

 2. after iteration 0 the LQ of every column >= 2 is LLR + (+0.0) bit for bit;
 3. in iteration 1 every edge but the row's first punctured edge has r_old = +-0, so |q| and q < 0
    on the non-punctured edges are those of LLR + (+0.0);
 4. iteration 1's check-node update is the update over the same non-punctured inputs that iteration
    0 walked plus the punctured edge(s): q_0 = LQ(0) - r_old for a row with one punctured column,
    q = LQ(0) bit for bit on both edges for a row with both;
 5. the two-min / argmin of the non-punctured edges alone (what the kernel parks in iteration 0),
    combined with the punctured edge(s) in front (they keep the argmin on a tie), gives the same
    messages.

BG2 has five rows without a punctured column, which send real messages in iteration 0: it keeps
the plain peeled iteration.
"""
import numpy as np
import pytest

from oracle import ldpc_oracle as O

T = np.float64


def _bits(x):
    return np.ascontiguousarray(x, T).view(np.uint64)


def _llrs(g, rng, B=6):
    llr = rng.normal(size=(B, g.N)) * 4.0
    llr[:, ::7] = -0.0     # planted zeros of both signs, core and extension columns
    llr[:, 3::11] = 0.0
    llr[1] = np.round(llr[1])                       # a row of integer LLRs: ties everywhere
    llr[2] = np.round(llr[2] / 4.0)                 # small integers: ties against the punctured edge
    llr[2, 1::5] = -0.0
    return llr.astype(T)


def _combine(q_np, q_p, alpha, beta):
    """The kernel's form: (min1', min2', first argmin') over the non-punctured edges q_np
    (B, d - npun, Zc), then the punctured edges q_p (B, npun, Zc) folded in, first edge last so
    that it wins ties; messages as _cn_update makes them."""
    a = np.abs(q_np)
    idx = a.argmin(axis=1)                          # first occurrence
    s = np.sort(a, axis=1)
    m1, m2 = s[:, 0], s[:, 1] if a.shape[1] > 1 else np.full_like(s[:, 0], np.inf)
    npun = q_p.shape[1]
    idx = idx + npun
    for k in range(npun - 1, -1, -1):
        aq = np.abs(q_p[:, k])
        idx = np.where(m1 < aq, idx, k)             # strict: the earlier edge keeps a tie
        m2 = np.minimum(m2, np.maximum(m1, aq))
        m1 = np.minimum(m1, aq)
    q = np.concatenate([q_p, q_np], axis=1)
    neg = q < 0
    sg = np.bitwise_xor.reduce(neg, axis=1, keepdims=True)
    d = q.shape[1]
    own = np.arange(d)[None, :, None] == idx[:, None, :]
    mag = np.where(own, m2[:, None, :], m1[:, None, :])
    m = T(alpha) * np.maximum(mag - T(beta), T(0))
    return np.where(neg ^ sg, -m, m).astype(T)


@pytest.mark.parametrize("alpha,beta", [(0.75, 0.0), (1.0, 0.5), (-0.75, 0.0)])
@pytest.mark.parametrize("Zc", [8, 22])
def test_second_iteration_from_first_pass(Zc, alpha, beta):
    g = O.graph(1, Zc)
    rng = np.random.default_rng(100 + Zc)
    llr = _llrs(g, rng)
    B = llr.shape[0]
    Lfull = np.concatenate([np.zeros((B, 2 * Zc), T), llr], axis=1)
    # iteration 0 as the oracle runs it
    acc = np.zeros_like(Lfull)
    Lr0 = []
    for i in range(g.Mb):
        cols = g.rows_cols(i)
        r = O._cn_update(Lfull[:, cols] - T(0), T(alpha), T(beta), T)
        Lr0.append(r)
        acc[:, cols] += r
    LQ1 = Lfull + acc
    # 2: columns >= 2, core and extension, hold LLR + (+0.0); only columns 0 and 1 changed
    plain = Lfull + T(0)
    assert np.array_equal(_bits(LQ1[:, 2 * Zc:]), _bits(plain[:, 2 * Zc:]))
    assert (LQ1[:, :2 * Zc] != 0).any()
    assert not (np.signbit(LQ1) & (LQ1 == 0)).any()
    for i in range(g.Mb):
        cols = g.rows_cols(i)
        base = g.bj[g.rs[i]:g.rs[i + 1]]
        npun = int((base < 2).sum())
        assert npun >= 1 and (base[:npun] < 2).all() and (base[npun:] >= 2).all()   # punctured edges first
        q = LQ1[:, cols] - Lr0[i]
        # 3: r_old = +-0 on every edge but the first punctured one
        assert not Lr0[i][:, 1:].any()
        sub = plain[:, cols[npun:]]
        assert np.array_equal(_bits(np.abs(q[:, npun:])), _bits(np.abs(sub)))
        assert np.array_equal(q[:, npun:] < 0, sub < 0)
        if npun == 2:
            assert not Lr0[i][:, 0].any()
            assert np.array_equal(_bits(q[:, :2]), _bits(LQ1[:, cols[:2]]))
        # 4: the update on the substituted inputs is the update on the true q
        qs = np.concatenate([q[:, :1] if npun == 1 else LQ1[:, cols[:2]], sub], axis=1)
        ref = O._cn_update(q, T(alpha), T(beta), T)
        assert np.array_equal(_bits(O._cn_update(qs, T(alpha), T(beta), T)), _bits(ref))
        # 5: parked minima of the non-punctured edges + the punctured edges, ties to the front
        assert np.array_equal(_bits(_combine(sub, qs[:, :npun], alpha, beta)), _bits(ref))


def test_bg2_has_rows_without_a_punctured_column():
    g = O.graph(2, 8)
    free = [i for i in range(g.Mb) if g.bj[g.rs[i]:g.rs[i + 1]].min() >= 2]
    assert len(free) == 5
