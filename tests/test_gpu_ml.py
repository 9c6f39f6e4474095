"""GPU tests of the batched maximum-likelihood detectors (ldpc5g_ml_detect through phy.ml_detect,
sch.sch_ml_rx_batch and the per-RE drop-ins).

Bound, every LLR and noise variance: |got - ref| <= 1e-10 * scale, scale = (|Y'| + |H'|_F sqrt(NL)
max|a|)^2 / sigma^2 on the system the ML core sees (recorded per RE in the fixture).  Rounding
costs c * eps * kappa(cov) ~ 1e-12 of that with kappa <~ 1e3 after regularisation; the fixture's
two smallest metrics differ by >= 1e-6 * scale, so within the bound every decision is equal, and
decisions are compared exactly.  The reference values are the reference's own recorded outputs
(tests/golden/ml_golden.npz); where the fixture has no case (gaps, strides, several transport
blocks) the reference is tests/ml_ref.py, which test_ml_host.py pins to the fixture.
"""
import os

import numpy as np
import pytest

import ml_ref
from conftest import GOLD

pytestmark = pytest.mark.gpu

TOL = ml_ref.TOL
MOD_ID = {"pi/2-bpsk": -1, "bpsk": 1, "qpsk": 2, "16qam": 4, "64qam": 6, "256qam": 8, "1024qam": 10}
CASES = [(s, a) for s in ml_ref.SETS for a in ml_ref.set_algos(*s)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a ROCm GPU"
    return t


@pytest.fixture(scope="module")
def phy():
    from python_5gtoolbox_amd import phy as p
    return p


@pytest.fixture(scope="module")
def golden():
    g = ml_ref.load_golden(os.path.join(GOLD, "ml_golden.npz"))
    for c in g.values():
        for a in (c["y"], c["h"], c["cov"]):
            a.setflags(write=False)
    return g


def _dev(torch, a, dtype=None):
    x = torch.tensor(a).cuda()
    return x if dtype is None else x.to(dtype)


def _run(torch, phy, c, mod, algo, dtype=None, **kw):
    """phy.ml_detect on one fixture set as a single transport block ->
    (llr (R, NL*Qm), sym (R, NL), nv (R, NL), hb (R, NL*Qm))"""
    NL = c["h"].shape[2]
    R = c["y"].shape[0]
    llr, sym, nv, hb = phy.ml_detect(_dev(torch, c["y"][None], dtype), _dev(torch, c["h"][None], dtype),
                                     _dev(torch, c["cov"][None], dtype), MOD_ID[mod], algo,
                                     want=("sym", "noise_var", "hardbits"), **kw)
    return (llr[0].cpu().numpy().reshape(R, -1), sym[0].cpu().numpy().reshape(R, NL),
            nv[0].cpu().numpy().reshape(R, NL), hb[0].cpu().numpy().reshape(R, -1))


def _id(v):
    return v if isinstance(v, str) else f"Nr{v[0]}NL{v[1]}-{v[2]}"


@pytest.mark.parametrize("shape,algo", CASES, ids=_id)
def test_fixture_parity_complex128(torch, phy, golden, shape, algo):
    """Decisions equal, LLR and noise_var within the bound, on every RE the reference was run on
    (kind 2: rank-1 cov for the IRC forms; kind 3: an all-zero last column of H, exact ties)."""
    c = golden[shape]
    ref = c[algo]
    ok = ref["ok"]
    llr, sym, nv, hb = _run(torch, phy, c, shape[2], algo)
    assert llr.dtype == np.float64 and nv.dtype == np.float64 and sym.dtype == np.complex64 and hb.dtype == np.int8
    assert np.array_equal(hb[ok], ref["hb"][ok])
    assert np.array_equal(sym[ok], ref["s"][ok])
    assert np.all(nv == nv[:, :1])
    e_llr = np.abs(llr - ref["llr"]).max(axis=1)[ok] / ref["scale"][ok]
    e_nv = np.abs(nv[:, 0] - ref["nv"])[ok] / ref["scale"][ok]
    print(f"{shape} {algo}: worst LLR error {e_llr.max():.2e}, noise_var {e_nv.max():.2e} (x scale), "
          f"{int(ok.sum())} REs")
    assert np.all(e_llr <= TOL) and np.all(e_nv <= TOL)
    assert np.isfinite(llr[ok]).all()
    k3 = ok & (c["kind"] == 3)
    if k3.any():   # every candidate of the last layer ties exactly: first point, LLRs exactly 0
        Qm = ml_ref.QM[shape[2]]
        assert np.all(sym[k3][:, -1] == ml_ref.constellation(shape[2])[0][0])
        if ml_ref.ALGOS[algo][0] != "hard":
            assert np.all(llr[k3][:, -Qm:] == 0)
        print(f"kind 3: {int(k3.sum())} REs tie exactly")


@pytest.mark.parametrize("shape", ml_ref.SETS, ids=_id)
def test_exact_properties(torch, phy, golden, shape):
    """No reference needed: ML-hard LLRs are exactly 1 - 2 hardbits; ML2-soft has LLR >= 0 exactly
    where the decided bit is 0; on two layers opt-rank2-ML decides as ML-soft does."""
    c = golden[shape]
    algos = ml_ref.set_algos(*shape)
    reg = c["kind"] == 0
    for irc in ("", "IRC-"):
        if "ML-hard" in algos:
            llr, _, _, hb = _run(torch, phy, c, shape[2], f"ML-{irc}hard")
            assert np.array_equal(llr, 1.0 - 2.0 * hb)
            llr2, sym2, _, hb2 = _run(torch, phy, c, shape[2], f"ML2-{irc}soft")
            assert np.array_equal(hb2, hb)
            assert np.array_equal(llr2[reg] >= 0, hb2[reg] == 0)
            if shape[1] == 2:
                _, sym_s, _, hb_s = _run(torch, phy, c, shape[2], f"ML-{irc}soft")
                _, sym_r, _, hb_r = _run(torch, phy, c, shape[2], "opt-rank2-ML" + ("-IRC" if irc else ""))
                assert np.array_equal(sym_s[reg], sym_r[reg]) and np.array_equal(hb_s[reg], hb_r[reg])


@pytest.mark.parametrize("shape,algo", [(s, a) for s, a in CASES if a.endswith(("soft", "ML", "IRC"))
                                        and s in (ml_ref.SETS[1], ml_ref.SETS[4], ml_ref.SETS[7],
                                                  ml_ref.SETS[9], ml_ref.SETS[11])], ids=_id)
def test_complex64_storage_and_float32_llr(torch, phy, golden, shape, algo):
    """complex64 storage is bit-equal to the complex128 run on the widened inputs; a float32 llr
    (and noise_var) is the float64 one rounded once."""
    c = golden[shape]
    c32 = {k: c[k].astype(np.complex64) for k in ("y", "h", "cov")}
    wide = {k: v.astype(np.complex128) for k, v in c32.items()}
    a = _run(torch, phy, c32, shape[2], algo)
    b = _run(torch, phy, wide, shape[2], algo)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)
    f = _run(torch, phy, wide, shape[2], algo, llr_dtype=torch.float32)
    assert f[0].dtype == np.float32 and f[2].dtype == np.float32
    assert np.array_equal(f[0], b[0].astype(np.float32), equal_nan=True)
    assert np.array_equal(f[2], b[2].astype(np.float32), equal_nan=True)
    assert np.array_equal(f[1], b[1], equal_nan=True) and np.array_equal(f[3], b[3])


def _indexing_inputs(R, T, Nr, NL, mod, seed):
    """Y = H s + noise per RE, one covariance per 12 REs (as the fixture's regular REs)."""
    rng = np.random.default_rng(seed)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)
    pts = ml_ref.constellation(mod)[0].astype(np.complex128)
    h = cn(T, R, Nr, NL)
    ncov = -(-R // 12)
    g = cn(T, ncov, Nr, 1)
    snr = 10 ** rng.uniform(0.5, 3, (T, ncov, 1, 1))
    cov = (np.identity(Nr) + 0.5 * g @ np.conj(g.transpose(0, 1, 3, 2))) / snr
    cov = (cov + np.conj(cov.transpose(0, 1, 3, 2))) / 2
    s = pts[rng.integers(0, pts.size, (T, R, NL))]
    noise = cn(T, R, Nr) / np.sqrt(np.repeat(snr[:, :, 0, 0], 12, axis=1)[:, :R, None])
    y = (h @ s[..., None])[..., 0] + noise
    return y, h, cov


def _check(got, ref, NL):
    """got: (llr, sym, nv, hb) rows of one transport block; ref: ml_ref.ml_detect's dict"""
    llr, sym, nv, hb = got
    assert np.array_equal(hb, ref["hardbits"]) and np.array_equal(sym, ref["sym"])
    scale = ref["scale"]
    nb = llr.size // scale.size
    assert np.all(np.abs(llr - ref["llr"]).reshape(-1, nb).max(axis=1) <= TOL * scale)
    assert np.all(np.abs(nv - ref["nv"]).reshape(-1, NL).max(axis=1) <= TOL * scale)


def _padded(torch, a, pad, poison):
    """Device copy of a (T, ...) whose rows are `pad` elements longer than needed, the padding
    poisoned: (view of the data, the whole (T, row + pad) buffer)."""
    T = a.shape[0]
    row = int(np.prod(a.shape[1:]))
    buf = torch.full((T, row + pad), poison, dtype=torch.complex128, device="cuda")
    buf[:, :row] = torch.from_numpy(np.ascontiguousarray(a).reshape(T, row)).cuda()
    strides = (row + pad,) + tuple(int(np.prod(a.shape[i + 1:])) for i in range(1, a.ndim))
    return buf.as_strided(a.shape, strides), buf


INDEX_ALGOS = ["ML-soft", "ML2-IRC-soft", "MMSE-ML-IRC", "opt-rank2-ML"]


@pytest.mark.parametrize("algo", INDEX_ALGOS)
def test_gaps_partial_wave_and_padded_strides(torch, phy, algo):
    """(2, 2, 16qam), T = 2, R = 88; re_idx drops every second RE of the first 36 (nre = 70: a
    partial wave with covariance boundaries inside it); every input row stride is padded and the
    padding poisoned."""
    T, R, Nr, NL, mod = 2, 88, 2, 2, "16qam"
    y, h, cov = _indexing_inputs(R, T, Nr, NL, mod, 11)
    idx = np.concatenate([np.arange(0, 36, 2), np.arange(36, 88)]).astype(np.int32)
    nre = idx.size
    assert nre == 70
    bad = complex(float("nan"), float("nan"))
    yd, ybuf = _padded(torch, y, 5, bad)
    hd, hbuf = _padded(torch, h, 3, bad)
    cd, cbuf = _padded(torch, cov, 7, bad)
    llr, sym, nv, hb = phy.ml_detect(yd, hd, cd, 4, algo, torch.from_numpy(idx).cuda(),
                                     want=("sym", "noise_var", "hardbits"))
    assert llr.shape == (T, nre * NL * 4) and sym.shape == (T, nre * NL) and hb.shape == llr.shape
    for t in range(T):
        ref = ml_ref.ml_detect(y[t], h[t], cov[t], mod, algo, idx)
        _check((llr[t].cpu().numpy(), sym[t].cpu().numpy(), nv[t].cpu().numpy(), hb[t].cpu().numpy()), ref, NL)
    # the inputs (padding included) are untouched
    assert torch.isnan(ybuf[:, -5:].real).all() and torch.isnan(hbuf[:, -3:].real).all()
    assert torch.isnan(cbuf[:, -7:].real).all()
    assert torch.equal(ybuf[:, :R * Nr], torch.from_numpy(y.reshape(T, -1)).cuda())


@pytest.mark.parametrize("mod,algo", [("16qam", a) for a in INDEX_ALGOS] + [("qpsk", "ML-soft"), ("qpsk", "ML2-soft")])
def test_all_res_across_a_workgroup_boundary(torch, phy, mod, algo):
    """R = 300 REs, none selected away: more than one workgroup for every lane mapping (one thread
    per RE: 256 REs per workgroup; a wave per RE: 4)."""
    T, R, Nr, NL = 1, 300, 2, 2
    y, h, cov = _indexing_inputs(R, T, Nr, NL, mod, 12)
    out = phy.ml_detect(_dev(torch, y), _dev(torch, h), _dev(torch, cov), MOD_ID[mod], algo,
                        want=("sym", "noise_var", "hardbits"))
    ref = ml_ref.ml_detect(y[0], h[0], cov[0], mod, algo)
    _check(tuple(o[0].cpu().numpy() for o in out), ref, NL)


def test_index_outside_the_grid_reads_nothing(torch, phy):
    """A resource-element index outside 0..R-1 yields NaN for that RE and leaves the others alone."""
    T, R, Nr, NL, mod = 1, 24, 2, 2, "16qam"
    y, h, cov = _indexing_inputs(R, T, Nr, NL, mod, 13)
    idx = np.array([0, 5, R, 7, -1, 23], np.int32)
    llr, nv = phy.ml_detect(_dev(torch, y), _dev(torch, h), _dev(torch, cov), 4, "ML-soft",
                            torch.from_numpy(idx).cuda(), want=("noise_var",))
    llr, nv = llr[0].cpu().numpy().reshape(6, -1), nv[0].cpu().numpy().reshape(6, -1)
    good = np.array([0, 1, 3, 5])
    ref = ml_ref.ml_detect(y[0], h[0], cov[0], mod, "ML-soft", idx[good])
    assert np.isnan(llr[[2, 4]]).all() and np.isnan(nv[[2, 4]]).all()
    assert np.all(np.abs(llr[good] - ref["llr"].reshape(4, -1)).max(axis=1) <= TOL * ref["scale"])


@pytest.mark.parametrize("algo", ["ML-soft", "ML2-IRC-soft"])
def test_descrambling_is_a_sign_flip_by_the_prbs(torch, phy, algo):
    """Two transport blocks with different cinit: LLR_descrambled = LLR * (1 - 2 c(n)), exactly."""
    from python_5gtoolbox_amd import nrPRBS
    T, R, Nr, NL, mod = 2, 36, 2, 2, "16qam"
    y, h, cov = _indexing_inputs(R, T, Nr, NL, mod, 14)
    cinit = [4660 * 2 ** 15 + 42, 77 * 2 ** 15 + 1001]
    args = (_dev(torch, y), _dev(torch, h), _dev(torch, cov), 4, algo)
    plain = phy.ml_detect(*args).cpu().numpy()
    got = phy.ml_detect(*args, cinit=torch.tensor(cinit, dtype=torch.int64, device="cuda")).cpu().numpy()
    n = plain.shape[1]
    assert n == R * NL * 4
    for t in range(T):
        c = np.asarray(nrPRBS.gen_nrPRBS(cinit[t], n)).astype(np.float64)
        assert np.array_equal(got[t], plain[t] * (1 - 2 * c))
    assert not np.array_equal(got[0] * plain[0] > 0, got[1] * plain[1] > 0)


def test_dropins(torch, golden):
    """Shapes, dtypes and values of the per-RE drop-ins on one fixture RE each."""
    from python_5gtoolbox_amd import ML, ML2, MMSE_ML, nr_channel_eq_ml, opt_rank2_ML
    shape = (2, 2, "16qam")
    c = golden[shape]
    NL, Qm, i = 2, 4, 17
    Y, H, cov = c["y"][i], c["h"][i], c["cov"][i // 12]

    def check(out, algo):
        s, nv, hb, llr = out
        ref = c[algo]
        assert isinstance(s, np.ndarray) and s.dtype == np.complex64 and s.shape == (NL,)
        assert nv.dtype == np.float64 and nv.shape == (NL,)
        assert hb.dtype == np.int64 and hb.shape == (NL * Qm,)
        assert llr.dtype == np.float64 and llr.shape == (NL * Qm,)
        assert np.array_equal(s, ref["s"][i]) and np.array_equal(hb, ref["hb"][i])
        assert np.abs(llr - ref["llr"][i]).max() <= TOL * ref["scale"][i]
        assert np.abs(nv - ref["nv"][i]).max() <= TOL * ref["scale"][i]
    check(ML.ML(Y, H, cov, "16qam"), "ML-soft")
    check(ML.ML(Y, H, cov, "16qam", "hard"), "ML-hard")
    check(ML.ML_IRC(Y, H, cov, "16qam"), "ML-IRC-soft")
    check(ML2.ML_IRC(Y, H, cov, "16qam"), "ML2-IRC-soft")
    check(ML2.ML(Y, H, cov, "16qam", demod_decision="soft"), "ML2-soft")
    check(MMSE_ML.MMSE_ML(Y, H, cov, "16qam"), "MMSE-ML")
    check(MMSE_ML.MMSE_ML_IRC(Y, H, cov, "16qam"), "MMSE-ML-IRC")
    check(opt_rank2_ML.opt_rank2_ML(Y, H, cov, "16qam"), "opt-rank2-ML")
    check(opt_rank2_ML.opt_rank2_ML_IRC(Y, H, cov, "16qam"), "opt-rank2-ML-IRC")
    s, nv, hb, llr = opt_rank2_ML.opt_rank2_ML(Y, H, cov, "16qam", "hard")
    assert np.array_equal(llr, 1 - 2 * hb)
    for algo in ml_ref.ALGOS:
        check(nr_channel_eq_ml.channel_equ_and_demod(Y, H, cov, "16qam", {"algo": algo}), algo)
    # a linear name goes through nr_channel_eq unchanged
    from python_5gtoolbox_amd import nr_channel_eq
    a = nr_channel_eq_ml.channel_equ_and_demod(Y, H, cov, "16qam", {"algo": "MMSE-IRC"})
    b = nr_channel_eq.channel_equ_and_demod(Y, H, cov, "16qam", {"algo": "MMSE-IRC"})
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # over the cap: refused with the way out named
    c4 = golden[(4, 4, "16qam")]
    with pytest.raises(AssertionError, match="opt-rank2-ML"):
        ML.ML(c4["y"][0], c4["h"][0], c4["cov"][0], "64qam")


def test_end_to_end_transport_block(torch, phy):
    """A = 904, 16QAM, NL = 2, Nr = 4: encoded, scrambled and modulated on the GPU, sent through a
    per-RE random 4x2 channel plus noise at 15 dB, received through sch.sch_ml_rx_batch with
    ML2-IRC-soft."""
    from python_5gtoolbox_amd import sch
    A, Qm, NL, Nr, nre = 904, 4, 2, 4, 300
    G = nre * NL * Qm
    cfg = sch.sch_config(A, Qm, 400, NL, 0, A, G)
    assert cfg.E_total == G and nre % 12 == 0
    gen = torch.Generator(device="cuda")
    gen.manual_seed(904)
    tb = torch.randint(0, 2, (1, A), dtype=torch.int8, device="cuda", generator=gen)
    cinit = torch.tensor([4660 * 2 ** 15 + 42], dtype=torch.int64, device="cuda")
    x = phy.scramble_modulate(sch.sch_encode_batch(tb, cfg), Qm, cinit).to(torch.complex128)

    def cn(*shape):
        return torch.complex(torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen),
                             torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)) / 2 ** 0.5
    h = cn(1, nre, Nr, NL)
    sigma2 = 10 ** (-15 / 10)
    y = (h @ x.view(1, nre, NL, 1))[..., 0] + cn(1, nre, Nr) * sigma2 ** 0.5
    cov = (sigma2 * torch.eye(Nr, dtype=torch.complex128, device="cuda")).repeat(1, nre // 12, 1, 1)
    r = sch.sch_ml_rx_batch(y.contiguous(), h, cov, "ML2-IRC-soft", None, Qm, cfg, 20, schedule="flooding",
                            cinit=cinit)
    assert bool(r.tb_ok.all())
    assert torch.equal(r.tbblk[:, :A], tb)
    assert bool(r.status.all()) and r.status.numel() == cfg.C
    with pytest.raises(AssertionError, match="G ="):
        sch.sch_ml_rx_batch(y[:, :-12].contiguous(), h[:, :-12].contiguous(), cov[:, :-1], "ML2-IRC-soft", None, Qm,
                            cfg, 20)
