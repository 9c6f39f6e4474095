"""GPU tests of PUSCH transform precoding (ldpc5g_transform_precode, ldpc5g_low_papr_seq,
ldpc5g_slot_rx_frontend_tp, ldpc5g_slot_map_tp; phy.transform_precode, phy.low_papr_seq,
phy.pusch_tp_frontend, phy.pusch_tp_map, sch.sch_pusch_tp_rx_batch and the drop-ins).

Bounds (relative to the largest magnitude of the reference array unless stated):
  transform vs np.fft in complex128 .... 1e-12 for complex128 (a float64 transform of <= 3240 points
                                         errs by a few 1e-16 per pass), 2^-22 for complex64 (the output
                                         rounding); the complex64 result IS the complex128 one rounded
  low-PAPR sequence vs tests/tp_ref.py . 1e-13 absolute (both reduce the index exactly; one
                                         sincospi against one cos / sin)
  low-PAPR sequence vs the reference ... 4 x the gap stored with the case
  h_ls vs tests/tp_ref.py .............. 1e-12 (complex128), 2^-22 (complex64)
  h_ls vs the reference's output ....... 4 x the gap stored with the case
  transmit grid vs the reference's ..... the gap stored with the case (identity precoding), 4 2^-23
                                         max|grid| with a precoding matrix
"""
import functools

import numpy as np
import pytest

import slot_ref
import tp_ref
from conftest import GOLD

pytestmark = pytest.mark.gpu

PRB = tp_ref.CARRIER_PRB
CE = dict(algo="DFT_symmetric", scs=30, eRB=4, l_left_ns=1400, l_right_ns=1200)
FIELDS = ("llr_dn", "ck", "status", "iters", "tb_ok", "tbblk")


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
def sch():
    from python_5gtoolbox_amd import sch as s
    return s


@pytest.fixture(scope="module")
def golden():
    g = tp_ref.load_golden(GOLD)
    for c in g.values():
        for a in c.values():
            a.setflags(write=False)
    return g


def _relmax(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _slots(torch, *s):
    return torch.tensor(list(s), dtype=torch.int32, device="cuda")


def _same_bits(torch, a, b):
    return a.shape == b.shape and torch.equal(torch.view_as_real(a).view(torch.uint8), torch.view_as_real(b).view(torch.uint8))


def _rand(rng, shape, dtype):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


# ------------------------------------------------------------------ the transform
@pytest.mark.parametrize("inverse", [False, True])
def test_all_53_lengths_both_storage_types(torch, phy, inverse):
    """T = 2, nsym = 3 at every length 12 * 2^a 3^b 5^c: against np.fft, complex64 = complex128
    rounded bit for bit, and forward then inverse returns the input."""
    assert len(tp_ref.RB_SIZES) == 53
    rng = np.random.default_rng(53 + inverse)
    worst = {np.complex64: 0.0, np.complex128: 0.0, "round trip": 0.0}
    for rb in tp_ref.RB_SIZES:
        x32 = _rand(rng, (2, 3 * 12 * rb), np.complex64)
        ref = tp_ref.transform_precode(x32, rb, inverse)
        g32 = phy.transform_precode(torch.tensor(x32).cuda(), rb, inverse)
        d128 = torch.tensor(x32.astype(np.complex128)).cuda()
        g128 = phy.transform_precode(d128, rb, inverse)
        assert g32.dtype == torch.complex64 and g128.dtype == torch.complex128 and g128.shape == d128.shape
        e32, e128 = _relmax(g32.cpu().numpy(), ref), _relmax(g128.cpu().numpy(), ref)
        worst[np.complex64], worst[np.complex128] = max(worst[np.complex64], e32), max(worst[np.complex128], e128)
        assert e128 <= 1e-12 and e32 <= 2.0 ** -22, (rb, e128, e32)
        assert _same_bits(torch, g32, g128.to(torch.complex64)), rb
        back = phy.transform_precode(g128, rb, not inverse)
        rt = float((back - d128).abs().max())
        worst["round trip"] = max(worst["round trip"], rt)
        assert rt <= 1e-12, (rb, rt)
    print("inverse" if inverse else "forward", {str(k): v for k, v in worst.items()})


@pytest.mark.parametrize("rb", [1, 5, 32])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_small_block_packing_with_a_partial_last_workgroup(torch, phy, rb, dtype):
    """M = 12, 60 (64 and 12 blocks per workgroup) and 384 (two): T = 37, nsym = 13 leaves the last
    workgroup partial.  Equal to np.fft, and bit for bit to the rows run one by one."""
    rng = np.random.default_rng(rb)
    T, nsym = 37, 13
    x = _rand(rng, (T, nsym * 12 * rb), dtype)
    d = torch.tensor(x).cuda()
    got = phy.transform_precode(d, rb)
    assert _relmax(got.cpu().numpy(), tp_ref.transform_precode(x, rb)) <= (1e-12 if dtype == np.complex128 else 2.0 ** -22)
    rows = torch.cat([phy.transform_precode(d[t:t + 1].contiguous(), rb) for t in range(T)])
    assert _same_bits(torch, rows, got)


@pytest.mark.parametrize("rb", [2, 18, 270])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_padded_strides_in_place_and_repeatability(torch, phy, rb, dtype):
    """Row strides padded by 7 elements (complex64 rows that are not 16-byte aligned), different for
    input and output; in place equals out of place; a second call gives the same bits."""
    rng = np.random.default_rng(7 * rb)
    T, W = 3, 4 * 12 * rb
    x = _rand(rng, (T, W), dtype)
    tdt = torch.complex64 if dtype == np.complex64 else torch.complex128
    src = torch.zeros((T, W + 7), dtype=tdt, device="cuda")[:, :W]
    src.copy_(torch.tensor(x))
    dst = torch.full((T, W + 14), 7 - 3j, dtype=tdt, device="cuda")
    assert src.stride(0) == W + 7
    for inverse in (False, True):
        plain = phy.transform_precode(torch.tensor(x).cuda(), rb, inverse)
        res = phy.transform_precode(src, rb, inverse, out=dst[:, :W])
        assert res.data_ptr() == dst.data_ptr() and _same_bits(torch, res, plain)
        assert bool((dst[:, W:] == 7 - 3j).all()), "the padding of out was written"
        again = phy.transform_precode(src, rb, inverse)
        assert _same_bits(torch, again, plain)
        work = torch.zeros((T, W + 7), dtype=tdt, device="cuda")[:, :W]
        work.copy_(src)
        phy.transform_precode(work, rb, inverse, out=work)
        assert _same_bits(torch, work, plain)
    assert np.array_equal(src.cpu().numpy(), x), "the input was written"


# ------------------------------------------------------------------ the sequence
def test_low_papr_sequences(torch, phy, golden):
    s = golden["seq"]
    for name, (u, v, alpha, MZC) in tp_ref.SEQ_CASES.items():
        got = phy.low_papr_seq(u, v, MZC, alpha)
        assert got.shape == (1, MZC) and got.dtype == torch.complex128
        got = got[0].cpu().numpy()
        e_ref, e_fix = np.abs(got - tp_ref.low_papr_seq(u, v, alpha, MZC)).max(), np.abs(got - s[name]).max()
        print(name, "vs tp_ref", e_ref, "vs reference", e_fix, "stored gap", float(s[name + "_gap"]))
        assert e_ref <= 1e-13 and e_fix <= 4 * float(s[name + "_gap"])
    # a batch, every group, both base sequences, the longest length
    u = np.repeat(np.arange(30), 2).astype(np.int32)
    v = np.tile([0, 1], 30).astype(np.int32)
    for MZC in (36, 30, 3300):
        vv = v if MZC >= 72 else np.zeros_like(v)
        got = phy.low_papr_seq(torch.tensor(u).cuda(), torch.tensor(vv).cuda(), MZC).cpu().numpy()
        ref = np.stack([tp_ref.low_papr_seq(int(a), int(b), 0.0, MZC) for a, b in zip(u, vv)])
        assert np.abs(got - ref).max() <= 1e-13
    from python_5gtoolbox_amd import lowPAPR_seq
    one = lowPAPR_seq.gen_lowPAPR_seq(29, 1, 0, 72)
    assert one.shape == (72,) and one.dtype == np.complex128 and np.abs(one - s["z72v1"]).max() <= 4 * float(s["z72v1_gap"])


# ------------------------------------------------------------------ the LS estimate
def _base(golden, kw, S):
    if kw["rb_size"] > 4:
        return None
    row = golden["seq"][f"short{6 * kw['rb_size']}"][tp_ref.SHORT_U.index(kw.get("npuschid", 77) % 30)]
    return np.tile(row, (S, 1))


@pytest.fixture(scope="module")
def restated(golden):
    out = {}
    for name, (kw, Nr, slot) in tp_ref.LS_CASES.items():
        c = golden["L" + name]
        out[name] = tp_ref.ls_est(c["grid"], tp_ref.pusch_config(**kw), slot, _base(golden, kw, c["h_ls"].shape[0]))
    return out


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("name", sorted(tp_ref.LS_CASES))
def test_frontend_against_the_restatement_and_the_reference(torch, phy, golden, restated, name, dtype):
    kw, Nr, slot = tp_ref.LS_CASES[name]
    cfg = tp_ref.pusch_config(**kw)
    c = golden["L" + name]
    base = _base(golden, kw, c["h_ls"].shape[0])
    grid = torch.tensor(c["grid"].astype(dtype)[None]).cuda()
    h_ls, y = phy.pusch_tp_frontend(grid, _slots(torch, slot), cfg, base_seq=base)
    ref = restated[name]
    assert h_ls.dtype == grid.dtype and h_ls.shape == (1,) + ref.shape and y.shape == (1, 14 * 12 * kw["rb_size"], Nr)
    got = h_ls[0].cpu().numpy()
    err = _relmax(got, ref)
    print(name, np.dtype(dtype).name, "h_ls vs tp_ref", err, "vs reference", _relmax(got, c["h_ls"]), "gap", float(c["gap"]))
    assert err <= (1e-12 if dtype == np.complex128 else 2.0 ** -22)
    assert _relmax(got, c["h_ls"]) <= 4 * float(c["gap"])
    want_y = slot_ref.extract(c["grid"].astype(dtype), cfg)
    assert np.array_equal(y[0].cpu().numpy().view(np.uint8), want_y.view(np.uint8))
    (h_only,) = phy.pusch_tp_frontend(grid, _slots(torch, slot), cfg, want=("h_ls",), base_seq=base)
    assert _same_bits(torch, h_only, h_ls)
    if dtype == np.complex64:   # the drop-in returns the reference's shapes and values
        from python_5gtoolbox_amd import nr_pusch_dmrs
        H, info = nr_pusch_dmrs.pusch_dmrs_LS_est_tp(c["grid"].copy(), cfg, slot, base_seq=base)
        assert H.dtype == np.complex64 and np.array_equal(H, got)
        assert info["RSSymMap"] == tp_ref.tp_params(cfg)["syms"] and info["RE_distance"] == 4


@pytest.mark.parametrize("hopping", ["groupHopping", "sequenceHopping"])
def test_hopping_follows_the_slots_and_base_seq_equals_the_generated_path(torch, phy, hopping):
    """RBSize 16, T = 3 with slots [19, 0, 7] and a padded slot stride: equal to tp_ref per slot, bit
    for bit to the slots run one by one, and to the call that is handed the same sequences as
    base_seq."""
    cfg = tp_ref.pusch_config(rb_start=8, rb_size=16, port=1003, add_pos=3, hopping=hopping, npuschid=1007)
    p = tp_ref.tp_params(cfg)
    Nr, W, slots = 2, 14 * 12 * PRB, [19, 0, 7]
    rng = np.random.default_rng(16)
    g = _rand(rng, (3, Nr, W), np.complex128)
    buf = torch.zeros((3, Nr * W + 7), dtype=torch.complex128, device="cuda")
    grid = buf[:, :Nr * W].view(3, Nr, W)
    grid.copy_(torch.tensor(g))
    (h_ls,) = phy.pusch_tp_frontend(grid, _slots(torch, *slots), cfg, want=("h_ls",))
    uv = [tp_ref.hop_uv(1007, hopping, 96, s, sym) for s in slots for sym in p["syms"]]
    assert len(set(uv)) > 1, "the case does not hop"
    for t in range(3):
        assert _relmax(h_ls[t].cpu().numpy(), tp_ref.ls_est(g[t], cfg, slots[t])) <= 1e-12
        (h1,) = phy.pusch_tp_frontend(grid[t:t + 1].contiguous(), _slots(torch, slots[t]), cfg, want=("h_ls",))
        assert _same_bits(torch, h1[0], h_ls[t])
    base = phy.low_papr_seq([a for a, _ in uv], [b for _, b in uv], 96).view(3, len(p["syms"]), 96)
    (h_b,) = phy.pusch_tp_frontend(grid, _slots(torch, *slots), cfg, want=("h_ls",), base_seq=base)
    assert _same_bits(torch, h_b, h_ls)


# RBSize 90 at RBStart 5 of a 96-PRB carrier: N = 270 DMRS REs per symbol, so a second workgroup whose
# first wave has 14 live lanes and whose other three have none.  The recorded cases stop at N = 60.
WIDE_PRB, WIDE_SLOTS = 96, (19, 0, 7)
WIDE_PORT = {1: 1002, 2: 1001, 4: 1003}


def _wide_cfg(**kw):
    return tp_ref.pusch_config(rb_start=5, rb_size=90, **kw)


@functools.lru_cache(maxsize=None)
def _wide_ls(hopping, Nr):
    """(config, grid (3, Nr, 14*12*96) of complex64 values, tp_ref's H_LS per slot), made once and read-only."""
    cfg = _wide_cfg(port=WIDE_PORT[Nr], add_pos=3, hopping=hopping, npuschid=1007)
    g = _rand(np.random.default_rng(90 + Nr), (3, Nr, 14 * 12 * WIDE_PRB), np.complex64)
    refs = [tp_ref.ls_est(g[t], cfg, WIDE_SLOTS[t]) for t in range(3)]
    for a in [g] + refs:
        a.setflags(write=False)
    return cfg, g, refs


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("Nr", [1, 2, 4])
@pytest.mark.parametrize("hopping", ["groupHopping", "sequenceHopping"])
def test_frontend_second_workgroup_and_unaligned_rows(torch, phy, hopping, Nr, dtype):
    """T = 3, slots [19, 0, 7], the slot stride padded by 6 and by 7 elements (7: complex64 rows that
    are not 16-byte aligned): h_ls equal to tp_ref per slot, y bit for bit slot_ref.extract, the batch
    bit for bit the slots run one by one and the call handed the same sequences as base_seq."""
    cfg, g, refs = _wide_ls(hopping, Nr)
    p = tp_ref.tp_params(cfg)
    S, W, MZC = len(p["syms"]), 14 * 12 * WIDE_PRB, 6 * 90
    uv = [tp_ref.hop_uv(1007, hopping, MZC, s, sym) for s in WIDE_SLOTS for sym in p["syms"]]
    assert len(set(uv)) > 1, "the case does not hop"
    base = phy.low_papr_seq([a for a, _ in uv], [b for _, b in uv], MZC).view(3, S, MZC)
    slots = _slots(torch, *WIDE_SLOTS)
    want_y = [slot_ref.extract(g[t].astype(dtype), cfg) for t in range(3)]
    for pad in (6, 7):
        buf = torch.zeros((3, Nr * W + pad), dtype=torch.complex64 if dtype == np.complex64 else torch.complex128,
                          device="cuda")
        grid = buf[:, :Nr * W].view(3, Nr, W)
        grid.copy_(torch.tensor(g.astype(dtype)))
        assert grid.stride(0) == Nr * W + pad
        h_ls, y = phy.pusch_tp_frontend(grid, slots, cfg)
        assert h_ls.shape == (3, S, 270, Nr, 1) and y.shape == (3, 14 * 12 * 90, Nr) and h_ls.dtype == y.dtype == grid.dtype
        for t in range(3):
            err = _relmax(h_ls[t].cpu().numpy(), refs[t])
            print(hopping, Nr, np.dtype(dtype).name, "pad", pad, "slot", WIDE_SLOTS[t], "h_ls vs tp_ref", err)
            assert err <= (1e-12 if dtype == np.complex128 else 2.0 ** -22)
            assert np.array_equal(y[t].cpu().numpy().view(np.uint8), want_y[t].view(np.uint8))
            h1, y1 = phy.pusch_tp_frontend(grid[t:t + 1].contiguous(), _slots(torch, WIDE_SLOTS[t]), cfg)
            assert _same_bits(torch, h1[0], h_ls[t]) and _same_bits(torch, y1[0], y[t])
        (h_b,) = phy.pusch_tp_frontend(grid, slots, cfg, want=("h_ls",), base_seq=base)
        assert _same_bits(torch, h_b, h_ls)


# ------------------------------------------------------------------ the transmit side
@pytest.mark.parametrize("name", sorted(tp_ref.MAP_CASES))
def test_transmit_grid_and_process_equal_the_reference(torch, phy, golden, name):
    kw, num_ant, slot = tp_ref.MAP_CASES[name]
    cfg = tp_ref.pusch_config(**kw)
    c = golden[name]
    pm = c["precoding"] if c["precoding"].size else None
    gmax = float(np.abs(c["grid"]).max())
    tol = 4 * 2.0 ** -23 * gmax if pm is not None else float(c["gap_grid"]) * gmax
    sym = np.stack([c["sym"], c["sym"][::-1].copy()])
    slots = [slot, slot + 1]
    sentinel = np.complex64(7 - 3j)
    out = torch.full((2, num_ant, 14 * 12 * PRB), complex(sentinel), dtype=torch.complex64, device="cuda")
    res = phy.pusch_tp_map(torch.tensor(sym).cuda(), _slots(torch, *slots), cfg, PRB, num_ant, precoding=pm, out=out)
    assert res is out
    got = out.cpu().numpy()
    for t in range(2):
        ref = tp_ref.tp_map(sym[t], cfg, slots[t], PRB, num_ant, pm,
                            grid=np.full((num_ant, 14 * 12 * PRB), np.nan + 0j, np.complex64))
        written = ~np.isnan(ref.real)
        assert written.sum() > 0 and np.all(got[t][~written] == sentinel), "an RE outside the map was written"
        assert np.abs(got[t][written] - ref[written]).max() <= 4 * 2.0 ** -23 * gmax
        if t == 0:
            assert np.all(c["grid"][~written] == 0)
            err = np.abs(got[t][written] - c["grid"][written]).max()
            print(name, "grid vs reference", err, "tol", tol)
            assert err <= tol
    fresh = phy.pusch_tp_map(torch.tensor(sym).cuda(), _slots(torch, *slots), cfg, PRB, num_ant, precoding=pm)
    assert np.abs(fresh[0].cpu().numpy() - c["grid"]).max() <= tol


WIDE_PM = {1: None, 2: [0.5 + 0.5j, -0.5j], 4: [0.5, -0.5, 0.5j, 0]}   # a zero weight: signed zeros


@pytest.mark.parametrize("num_ant", [1, 2, 4])
@pytest.mark.parametrize("port", [1001, 1002])
def test_transmit_grid_second_workgroup(torch, phy, port, num_ant):
    """RBSize 90 on the 96-PRB carrier, T = 2, ports 1001 and 1002, one antenna without and two and
    four with a precoding vector: the written REs equal tp_ref.tp_map, every other RE keeps the
    sentinel (the other comb of the DMRS symbols included)."""
    cfg = _wide_cfg(port=port, add_pos=1, hopping="groupHopping", npuschid=301)
    pm = None if WIDE_PM[num_ant] is None else np.array(WIDE_PM[num_ant], np.complex64).reshape(-1, 1)
    nre = len(phy.pusch_tp_data_re_idx(cfg)[0])
    sym = _rand(np.random.default_rng(port + num_ant), (2, nre), np.complex64)
    slots = [9, 10]
    sentinel = np.complex64(7 - 3j)
    W = 14 * 12 * WIDE_PRB
    out = torch.full((2, num_ant, W), complex(sentinel), dtype=torch.complex64, device="cuda")
    res = phy.pusch_tp_map(torch.tensor(sym).cuda(), _slots(torch, *slots), cfg, WIDE_PRB, num_ant, precoding=pm, out=out)
    assert res is out
    got = out.cpu().numpy()
    for t in range(2):
        ref = tp_ref.tp_map(sym[t], cfg, slots[t], WIDE_PRB, num_ant, pm, grid=np.full((num_ant, W), np.nan + 0j, np.complex64))
        written = ~np.isnan(ref.real)
        assert written.sum() == num_ant * (nre + 2 * 2 * 270)
        assert np.all(got[t][~written] == sentinel), "an RE outside the map was written"
        err, gmax = np.abs(got[t][written] - ref[written]).max(), float(np.abs(ref[written]).max())
        print("port", port, "num_ant", num_ant, "slot", slots[t], "grid vs tp_ref", err, "tol", 4 * 2.0 ** -23 * gmax)
        assert err <= 4 * 2.0 ** -23 * gmax


def test_process_dropin(torch, golden):
    """nr_pusch_process from bits: scrambled and modulated here, spread and precoded; against the
    reference's output through the symbols it modulated."""
    from python_5gtoolbox_amd import nr_pusch_process, phy as P
    c = golden["P18"]
    kw, num_ant, slot = tp_ref.MAP_CASES["P18"]
    rng = np.random.default_rng(18)
    Qm, n = 4, c["sym"].size
    g = rng.integers(0, 2, n * Qm).astype(np.int8)
    out = nr_pusch_process.nr_pusch_process(g, 1, 1, Qm, 1, 1, kw["rb_size"], num_ant, c["precoding"])
    assert out.dtype == np.complex64 and out.shape == (num_ant, n)
    cinit = torch.tensor([2 ** 15 + 1], dtype=torch.int32, device="cuda")
    sym = P.scramble_modulate(torch.tensor(g[None]).cuda(), Qm, cinit)[0].cpu().numpy()
    assert _relmax(out, tp_ref.process(sym, kw["rb_size"], c["precoding"])) <= 4 * 2.0 ** -23
    with pytest.raises(NotImplementedError, match="UCI"):
        nr_pusch_process.nr_pusch_process(np.where(np.arange(n * Qm) == 5, -1, g), 1, 1, Qm, 1, 1, kw["rb_size"], num_ant,
                                          c["precoding"])


@pytest.mark.parametrize("mod", [2, -1])
def test_loopback_transport_block_to_grid_and_back(torch, phy, sch, mod):
    """sch_encode_batch -> scramble_modulate -> pusch_tp_map -> the grid taken as the received grid
    (Nr = 1) -> sch_pusch_tp_rx_batch with ZF: every TB's bits come back, for QPSK and pi/2-BPSK.
    No reference involved."""
    cfg = tp_ref.pusch_config(rb_start=2, rb_size=16, add_pos=1, hopping="groupHopping", npuschid=301)
    re_idx, _ = phy.pusch_tp_data_re_idx(cfg)
    Qm, T = abs(mod), 2
    G = len(re_idx) * Qm
    A = 500 * Qm
    scfg = sch.sch_config(A, Qm, 300, 1, 0, 0, G)
    rng = np.random.default_rng(3 + mod)
    trblk = torch.tensor(rng.integers(0, 2, (T, A)).astype(np.int8)).cuda()
    cinit = torch.tensor([32769, 40000], dtype=torch.int32, device="cuda")
    g = sch.sch_encode_batch(trblk, scfg)
    sym = phy.scramble_modulate(g.contiguous(), mod, cinit)
    slots = _slots(torch, 3, 12)
    grid = phy.pusch_tp_map(sym, slots, cfg, PRB, 1)
    res = sch.sch_pusch_tp_rx_batch(grid, slots, cfg, CE, "ZF", mod, scfg, 8, cinit=cinit)
    print("loopback mod", mod, "tb_ok", res.tb_ok.cpu().tolist(), "iters", res.iters.cpu().tolist())
    assert res.tb_ok.cpu().tolist() == [1] * T
    assert torch.equal(res.tbblk[:, :A], trblk)


@pytest.mark.parametrize("name", sorted(tp_ref.E2E_CASES))
def test_end_to_end_on_the_reference_receptions(torch, phy, sch, golden, name):
    """The received grids the reference decoded with nTransPrecode = 1: sch_pusch_tp_rx_batch gives the
    reference's transport block and equals, field for field, the chain composed by hand."""
    case = tp_ref.E2E_CASES[name]
    cfg = tp_ref.pusch_config(**case["cfg"])
    c = golden[name]
    A, Qm, G = (int(v) for v in c["meta"])
    scfg = sch.sch_config(A, Qm, float(c["coderate"]), 1, 0, 0, G)
    grid = torch.tensor(c["grid"][None]).cuda()
    slots = _slots(torch, case["slot"])
    cinit = torch.tensor([cfg["rnti"] * 2 ** 15 + cfg["nNid"]], dtype=torch.int32, device="cuda")
    ce = dict(CE, to_comp=True)
    kw = dict(alpha=0.8, beta=0.3, cinit=cinit)
    res = sch.sch_pusch_tp_rx_batch(grid, slots, cfg, ce, "MMSE", Qm, scfg, 8, **kw)
    assert bool(c["status"]) and res.tb_ok.cpu().tolist() == [1]
    assert np.array_equal(res.tbblk[0, :A].cpu().numpy(), c["tbblk"][:A])
    assert np.array_equal(c["tbblk"][:A], c["trblk"])
    h_ls, y = phy.pusch_tp_frontend(grid, slots, cfg)
    re_idx = torch.tensor(phy.pusch_tp_data_re_idx(cfg)[0]).cuda()
    held = sch.sch_pusch_tp_rx_batch(grid, slots, cfg, ce, "MMSE", Qm, scfg, 8, re_idx=re_idx, **kw)
    assert torch.equal(res.tbblk, held.tbblk) and torch.equal(res.llr_dn, held.llr_dn)
    ce2 = dict(ce, sym_map=tp_ref.tp_params(cfg)["syms"], num_cdm_groups=2)
    y2, h, cov = sch._ce_stage(y, h_ls, ce2)
    sym, nv = phy.equalize(y2, h, cov, "MMSE", re_idx)
    sym = phy.transform_precode(sym, case["cfg"]["rb_size"], inverse=True)
    hand = sch.sch_rx_batch(sym, nv, Qm, scfg, 8, **kw)
    for f in FIELDS:
        assert torch.equal(getattr(res, f), getattr(hand, f)), f
