"""GPU tests of the polar codec: every fixture the reference produced through the batched entry points
and through the drop-ins (bits, status and the -1 rows equal the reference's, pm bit-equal to
tests/polar_ref.py's, recorded with the fixtures), batch shapes, strided views, repeatability, mixed
failing / succeeding neighbours, both storage paths of N = 1024, and noise-free round trips."""
import json
import os

import numpy as np
import pytest

import polar_ref as R
from conftest import GOLD

pytestmark = pytest.mark.gpu


def load(name):
    return np.load(os.path.join(GOLD, f"polar_golden_{name}.npz"))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def groups():
    """Decode fixtures grouped by everything a launch shares: {key: [(llr, ck, status, pm), ...]}."""
    d = load("decode")
    out = {}
    for i, c in enumerate(json.loads(str(d["meta"]))):
        key = (c["K"], c["E"], c["nMax"], c["iIL"], c["CRCLEN"], c["padCRC"], c["rnti"], c["algo"], c["L"])
        out.setdefault(key, []).append((d[f"llr{i}"], d[f"ck{i}"], c["status"], float.fromhex(c["pm"])))
    return out


def _decode(torch, key, llr, **kw):
    from python_5gtoolbox_amd import polar
    p = polar.plan(*key[:7])
    x = llr if torch.is_tensor(llr) else torch.from_numpy(np.ascontiguousarray(llr)).cuda()
    ck, st, pm = polar.decode(x, p, key[7], key[8], **kw)
    return ck.cpu().numpy(), st.cpu().numpy(), pm.cpu().numpy()


def _expect(cases):
    return (np.stack([c[1] for c in cases]), np.array([c[2] for c in cases], np.uint8),
            np.array([c[3] for c in cases], np.float64))


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)   # pm: bit for bit (inf == inf on failure)


def test_every_decode_fixture_batched(torch, groups):
    assert len(groups) >= 60
    for key, cases in groups.items():
        _same(_decode(torch, key, np.stack([c[0] for c in cases])), _expect(cases))


def test_every_decode_fixture_through_the_dropin(torch, groups):
    from python_5gtoolbox_amd import nr_polar_decoder
    for key, cases in groups.items():
        K, E, nMax, iIL, crclen, pad, rnti, algo, L = key
        for llr, ck, status, _ in cases:
            for name in (algo, algo + "_optionB"):
                g, st = nr_polar_decoder.nr_decode_polar(name, llr, E, K, L, nMax, iIL, crclen, pad, rnti)
                assert st is bool(status)
                assert np.array_equal(g, ck) if status else g == [-1]


def test_batch_shapes_strides_and_repeatability(torch, groups):
    """B = 1, B = 3, a batch that is no multiple of anything (67), a strided view, the same call twice."""
    for key, cases in groups.items():
        if key[7:] not in (("SCL", 8), ("SC", 1), ("SCL", 3)) or key[0] > 64:
            continue
        ex = _expect(cases)
        for B in (1, 3, 67):
            idx = np.arange(B) % len(cases)
            llr = np.stack([cases[i][0] for i in idx])
            got = _decode(torch, key, llr)
            _same(got, [e[idx] for e in ex])
            _same(_decode(torch, key, llr), got)
        N = cases[0][0].size
        wide = torch.full((len(cases), N + 24), float("nan"), dtype=torch.float64, device="cuda")
        wide[:, 8:8 + N] = torch.from_numpy(np.stack([c[0] for c in cases])).cuda()
        view = wide[:, 8:8 + N]
        assert not view.is_contiguous()
        _same(_decode(torch, key, view), ex)


def test_failing_and_succeeding_neighbours(torch, groups):
    seen = 0
    for key, cases in groups.items():
        ok = [c for c in cases if c[2]]
        bad = [c for c in cases if not c[2]]
        if not ok or not bad:
            continue
        seen += 1
        mix = [ok[0], bad[0], ok[-1], bad[-1], bad[0], ok[0], ok[0]]
        got = _decode(torch, key, np.stack([c[0] for c in mix]))
        _same(got, _expect(mix))
        assert np.all(got[0][got[1] == 0] == -1) and np.all(np.isinf(got[2][got[1] == 0]))
    assert seen >= 3


def test_list_and_size_corners(torch, groups):
    """N = 32 at L = 32; N = 1024 at L = 16 (all state in LDS) and at L = 32 (two layers in the workspace)."""
    corner = {(32, 32): 0, (1024, 16): 0, (1024, 32): 0}
    for key, cases in groups.items():
        N = cases[0][0].size
        if key[7] == "SCL" and (N, key[8]) in corner:
            corner[(N, key[8])] += len(cases)
            B = 5   # more than one workgroup, each looping once
            idx = np.arange(B) % len(cases)
            _same(_decode(torch, key, np.stack([cases[i][0] for i in idx])), [e[idx] for e in _expect(cases)])
    assert all(corner.values()), corner


def test_chain_fixtures(torch):
    from python_5gtoolbox_amd import nr_polar_encoder, nr_polar_ratematch, nr_polar_raterecover, polar, polar_construct
    d = load("chain")
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    for i, (K, E, nMax, iIL, iBIL, N, quirk) in enumerate(d["meta"].tolist()):
        blk, enc, rm, llr, rr = (d[f"{k}{i}"] for k in ("blk", "enc", "rm", "llr", "rr"))
        p = polar.plan(K, E, nMax, iIL, 24 if iIL else (6 if K <= 25 else 11))
        assert p.N == N
        for B in (1, 3, 17):
            assert np.array_equal(polar.encode(cu(np.tile(blk, (B, 1))), p).cpu().numpy(), np.tile(enc, (B, 1)))
        assert np.array_equal(polar.rate_match(cu(np.tile(enc, (3, 1))), p, iBIL).cpu().numpy(), np.tile(rm, (3, 1)))
        assert np.array_equal(polar.polar_tx(cu(blk), p, E, iBIL).cpu().numpy()[0], rm)
        got = polar.rate_recover(cu(np.tile(llr, (3, 1))), p, iBIL, 20.0, reference_repetition=True).cpu().numpy()
        assert np.array_equal(got, np.tile(rr, (3, 1)))
        mine = polar.rate_recover(cu(llr), p, iBIL).cpu().numpy()[0]
        assert np.array_equal(mine, R.rate_recover(llr, K, N, iBIL, 20.0))
        assert (not np.array_equal(mine, rr)) == bool(quirk)
        # the drop-ins, name for name
        assert np.array_equal(nr_polar_encoder.encode_polar(blk, E, nMax, iIL), enc)
        assert np.array_equal(nr_polar_ratematch.ratematch_polar(enc, K, E, iBIL), rm)
        assert np.array_equal(nr_polar_raterecover.ratemrecover_polar(llr, K, N, iBIL), rr)
        F, qPC, n2, nPC, nPCwm = polar_construct.construct(K, E, nMax)
        f2, q2, n3, p3, w3 = R.construct(K, E, nMax)
        assert np.array_equal(F, f2) and np.array_equal(qPC, q2) and (n2, nPC, nPCwm) == (n3, p3, w3)


ROUND = [(64, 216, 9), (40, 60, 9), (100, 512, 9), (140, 1000, 9), (20, 64, 10), (20, 256, 10), (60, 70, 10),
         (211, 900, 10), (150, 512, 10), (311, 2100, 10)]


def test_round_trip_without_noise(torch):
    """Every rate-matching mode and both iBIL decode with the default rate recovery."""
    from python_5gtoolbox_amd import polar
    rng = np.random.default_rng(7)
    modes = set()
    for K, E, nMax in ROUND:
        iIL, crclen = (1, 24) if nMax == 9 else (0, 6 if K <= 25 else 11)
        p = polar.plan(K, E, nMax, iIL, crclen)
        modes.add(p.mode_name)
        blk = np.stack([R.crc_attach(rng.integers(0, 2, K - crclen), crclen) for _ in range(3)])
        for iBIL in (0, 1):
            if iBIL and nMax == 9 and 25 < K <= 30:
                continue
            f = polar.polar_tx(torch.from_numpy(blk).cuda(), p, E, iBIL)
            llr = 4.0 * (1.0 - 2.0 * f.to(torch.float64))
            ck, st, pm = polar.polar_rx(llr, p, E, iBIL, "SCL", 8)
            assert st.cpu().numpy().tolist() == [1, 1, 1] and np.array_equal(ck.cpu().numpy(), blk), (K, E, nMax, iBIL)
            assert np.all(pm.cpu().numpy() == 0.0)
    assert modes == {"repetition", "puncturing", "shortening"}


def test_reference_repetition_fails_the_uplink_repetition_case(torch):
    from python_5gtoolbox_amd import polar
    d = load("chain")
    blk, llr = d["quirk_blk"], d["quirk_llr"]
    p = polar.plan(311, 2100, 10, 0, 11)
    x = torch.from_numpy(llr).cuda()
    ck, st, _ = polar.polar_rx(x, p, 2100, 1, "SCL", 8)
    assert int(st[0]) == 1 and np.array_equal(ck.cpu().numpy()[0], blk)
    ck, st, _ = polar.polar_rx(x, p, 2100, 1, "SCL", 8, reference_repetition=True)
    assert int(st[0]) == int(d["quirk_status"][0]) == 0 and np.all(ck.cpu().numpy() == -1)
    y = polar.rate_recover(x, p, 1, reference_repetition=True).cpu().numpy()[0]
    assert np.array_equal(y, d["quirk_rr"])
