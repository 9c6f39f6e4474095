"""CPU tests of the UCI-on-PUSCH host code (ldpc5g_uci_rm_info, ldpc5g_uci_map_plan) and of the numpy
restatement tests/uci_ref.py against the recorded outputs of the reference (tests/golden/uci_golden_*).
No kernel is launched here."""
import ctypes
import os
import re
import time

import numpy as np
import pytest

import uci_ref as R
from conftest import GOLD, ROOT
from python_5gtoolbox_amd import _lib, uci, ul_tbsize

CASES = R.load_cases(GOLD)
NAMES = list(R.CASES)


def _plan(name):
    c = CASES[name]
    return uci.plan(c["cfg"], c["dmrs"], c["rm"], c["Qm"])


def test_the_eleven_cases_are_recorded():
    assert set(CASES) == set(R.CASES) and len(CASES) == 11
    assert CASES["A1"]["rm"]["Euci_ack"] == 28 and CASES["A1"]["rm"]["Euci_ackrvd"] == 52 and CASES["A1"]["Gtotal"] == 1056
    assert CASES["BIG"]["Gtotal"] == 27648 and CASES["BIG"]["rm"]["Euci_CSI2"] == 1352
    assert CASES["A2C"]["rm"]["G_ULSCH"] == 3416 and CASES["U0a"]["rm"]["Euci_CSI1"] == 2232


@pytest.mark.parametrize("name", NAMES)
def test_rm_info_cases(name):
    c = CASES[name]
    got = uci.rm_info(c["cfg"], c["dmrs"], c["ULSCH_size"], c["Qm"], c["coderateby1024"], c["Gtotal"])
    assert got == c["rm"]
    assert list(got) == list(uci.RM_KEYS) and all(type(v) is int for v in got.values())


def test_rm_info_random_configurations():
    d = np.load(os.path.join(GOLD, "uci_golden_rminfo.npz"))
    lib = _lib.lib()
    refused = 0
    for row, dm, cr, s, want, bad in zip(d["inputs"].tolist(), d["dmrs"], d["coderate"], d["scaling"], d["out"], d["refused"]):
        RB, start, nsym, _, NL, Qm, usize, en, oack, ocsi1, ocsi2, ia, i1, i2, G = row
        dm = np.ascontiguousarray(dm[dm >= 0], np.int32)
        out = np.zeros(9, np.int64)
        rc = lib.ldpc5g_uci_rm_info(RB, start, nsym, ctypes.c_void_p(dm.ctypes.data), dm.size, NL, Qm, float(cr), usize, en, oack,
                                    ocsi1, ocsi2, ia, i1, i2, float(s), G, ctypes.c_void_p(out.ctypes.data))
        if bad:
            assert rc == _lib.ESIZE and lib.ldpc5g_last_error(), row
            refused += 1
        else:
            assert rc == 0 and out.tolist() == want.tolist(), (row, out.tolist(), want.tolist())
    assert d["inputs"].shape[0] == 200 and 20 < refused < 150


def test_rm_info_refuses_where_the_reference_asserts():
    c = CASES["ALL"]
    base = (c["cfg"], c["dmrs"], c["ULSCH_size"], c["Qm"], c["coderateby1024"], c["Gtotal"])
    for key, val, word in (("I_HARQ_ACK_offset", 16, "I_HARQ_ACK_offset"), ("I_CSI1offset", 19, "I_CSI1offset"),
                           ("I_CSI2offset", -1, "I_CSI2offset")):
        cfg = dict(c["cfg"], **{key: val})
        with pytest.raises(AssertionError, match=word):
            uci.rm_info(cfg, *base[1:])
    with pytest.raises(AssertionError, match="Gtotal"):
        uci.rm_info(base[0], base[1], base[2], base[3], base[4], 100)
    wide = dict(c["cfg"], ResAlloType1={"RBStart": 0, "RBSize": 273}, NumCSI2Bits=1706)
    with pytest.raises(AssertionError, match="8192"):
        uci.rm_info(wide, c["dmrs"], 8448, c["Qm"], c["coderateby1024"], 273 * 12 * 11 * 6)
    with pytest.raises(AssertionError, match="ULSCH_size"):
        uci.rm_info(base[0], base[1], 0, *base[3:])
    for bad in ([2, 14], [-1, 11], list(range(15))):        # the same allocation checks as the plan builder
        with pytest.raises(AssertionError, match="allocation"):
            uci.rm_info(base[0], bad, *base[2:])
        with pytest.raises(AssertionError, match="allocation"):
            uci.plan(base[0], bad, c["rm"], c["Qm"], c["Gtotal"])
    with pytest.raises(AssertionError, match="minimum capacity"):   # 11 bits cannot fit 1 RE of QPSK
        uci.rm_info(dict(CASES["Q2"]["cfg"], NumACKBits=11, I_HARQ_ACK_offset=0), CASES["Q2"]["dmrs"], 10 ** 6, 2, 193.0, 528)


@pytest.mark.parametrize("name", NAMES)
def test_plan_reproduces_the_references_map(name):
    c = CASES[name]
    p = _plan(name)
    m = p.expand()
    assert p.Gtotal == c["Gtotal"] and p.Qm == c["Qm"]
    lens = {"ulsch": c["rm"]["G_ULSCH"], "ack": c["rm"]["Euci_ack"], "csi1": c["rm"]["Euci_CSI1"], "csi2": c["rm"]["Euci_CSI2"]}
    assert p.lens == lens
    # the separated arange streams ARE the inverse map
    for n in R.STREAMS:
        assert np.array_equal(m["inv"][n], c[n]), n
    # the forward map reproduces g_seq from the recorded coded streams, placeholders included
    d = np.load(os.path.join(GOLD, "uci_golden_map.npz"))
    for r in range(3):
        g = np.zeros(p.Gtotal, np.int8)
        for s, n in enumerate(R.STREAMS):
            sel = m["stream"] == s
            g[sel] = d[f"{name}_in_{n}"][r][m["index"][sel]]
        assert np.array_equal(g, d[f"{name}_g_seq"][r])
        assert np.array_equal(m["kind"] == R.X, g == -1) and np.array_equal(m["kind"] == R.Y, g == -2)
    assert p.n_x == int((d[f"{name}_g_seq"][0] == -1).sum()) and p.n_y == int((d[f"{name}_g_seq"][0] == -2).sum())
    # and equals the numpy restatement field by field
    ref = R.build_map(c["cfg"], c["dmrs"], c["rm"], c["Qm"], c["Gtotal"])
    for k in ("stream", "index", "kind"):
        assert np.array_equal(m[k], ref[k]), k
    for n in R.STREAMS:
        assert np.array_equal(m["inv"][n], ref["inv"][n]) and np.array_equal(m["inv_punct"][n], ref["punct"][n])
    assert p.n_punct == sum(int(v.sum()) for v in ref["punct"].values())
    if name in ("A1", "Q2", "A2", "A2C", "SC5"):
        assert p.n_punct == c["rm"]["Euci_ack"] and m["inv_punct"]["ulsch"].sum() == p.n_punct
        # a punctured UL-SCH element and the ACK element that overwrote it share the position
        assert set(m["inv"]["ulsch"][m["inv_punct"]["ulsch"]]) == set(m["inv"]["ack"])
    else:
        assert p.n_punct == 0


@pytest.mark.parametrize("name", NAMES)
def test_uci_ref_equals_the_goldens(name):
    c = CASES[name]
    d = np.load(os.path.join(GOLD, "uci_golden_map.npz"))
    m = R.build_map(c["cfg"], c["dmrs"], c["rm"], c["Qm"], c["Gtotal"])
    for r in range(3):
        assert np.array_equal(R.mux(m, {n: d[f"{name}_in_{n}"][r] for n in R.STREAMS}), d[f"{name}_g_seq"][r])
    sep = R.demux(m, np.arange(c["Gtotal"], dtype=np.float64))
    for n in R.STREAMS:
        assert np.array_equal(sep[n], c[n])
    # the coded UCI streams of payloads up to 11 bits are the small-block code repeated to E
    for n, key in (("ack", "NumACKBits"), ("csi1", "NumCSI1Bits"), ("csi2", "NumCSI2Bits")):
        A = c["cfg"][key]
        if 1 <= A <= 11:
            assert np.array_equal(R.sb_encode_rm(d[f"{name}_bits_{n}"], m["lens"][n], c["Qm"]), d[f"{name}_in_{n}"])


def test_uci_ref_smallblock_code():
    d = np.load(os.path.join(GOLD, "uci_golden_smallblock.npz"))
    total = 0
    for K in range(1, 12):
        msgs = (np.arange(2 ** K)[:, None] >> (K - 1 - np.arange(K))) & 1
        total += 2 ** K
        if K <= 2:
            for Qm in (1, 2, 4, 6, 8):
                assert np.array_equal(R.sb_encode(msgs, Qm), d[f"K{K}_Qm{Qm}"])
                assert np.array_equal(R.sb_kinds(K, Qm) == R.X, d[f"K{K}_Qm{Qm}"][0] == -1)
                assert np.array_equal(R.sb_kinds(K, Qm) == R.Y, d[f"K{K}_Qm{Qm}"][0] == -2)
        else:
            cw = np.unpackbits(d[f"K{K}"], axis=1)[:, :32].astype(np.int8)
            assert np.array_equal(R.sb_encode(msgs, 2), cw)
            # noiseless soft decisions return the message; the code's minimum distance
            assert np.array_equal(R.sb_decode(1.0 - 2.0 * cw, K, 2), msgs)
            if K in (3, 6, 11):
                w = cw[1:].sum(1)
                assert len({tuple(r) for r in cw.tolist()}) == 2 ** K and w.min() == (16 if K <= 6 else 10)
    assert total == 4094


def test_uci_ref_soft_decisions_on_placeholders_and_ties():
    rng = np.random.default_rng(5)
    for Qm in (1, 2, 4, 6, 8):
        for K in (1, 2):
            msgs = (np.arange(2 ** K)[:, None] >> (K - 1 - np.arange(K))) & 1
            for E in (R.sb_N(K, Qm), 3 * R.sb_N(K, Qm) + 1):
                cw = R.sb_encode_rm(msgs, E, Qm)
                llr = np.where(cw < 0, rng.normal(size=cw.shape) * 50, 1.0 - 2.0 * cw)   # placeholders carry junk
                if K == 1 and Qm >= 2:
                    llr[:, 1::Qm] = 1.0 - 2.0 * cw[:, 0:1]     # y repeats the data bit once descrambled
                    llr[:, 0] *= 0.25                          # ... and decides when the data position is weak
                assert np.array_equal(R.sb_decode(llr, K, Qm), msgs), (K, Qm, E)
    assert R.sb_decode(np.zeros((1, 32)), 11, 2).tolist() == [[0] * 11]
    assert R.sb_decode(np.zeros((1, 7)), 2, 4).tolist() == [[0, 0]] and R.sb_decode(np.zeros((1, 4)), 1, 4).tolist() == [[0]]


def test_uci_ref_scrambling_equals_the_goldens_bits():
    d = np.load(os.path.join(GOLD, "uci_golden_symbols.npz"))
    for Qm in (2, 4, 6, 8):
        g, (rnti, nID) = d[f"g{Qm}"], d[f"id{Qm}"]
        s = R.scramble(g, R.prbs(int(rnti) * 2 ** 15 + int(nID), g.size))
        sym = d[f"sym{Qm}"]
        # the first two bits of a symbol are the signs of its real and imaginary parts
        assert np.array_equal(s[0::Qm], (sym.real < 0).astype(np.int8)) and np.array_equal(s[1::Qm], (sym.imag < 0).astype(np.int8))


def test_uci_ref_descrambling_mode_inverts_the_scrambler():
    c = CASES["A1"]
    d = np.load(os.path.join(GOLD, "uci_golden_map.npz"))
    m = R.build_map(c["cfg"], c["dmrs"], c["rm"], c["Qm"], c["Gtotal"])
    g = d["A1_g_seq"][0]
    cc = R.prbs(12345, g.size)
    llr = (1.0 - 2.0 * R.scramble(g, cc)) * np.arange(1, g.size + 1)
    out = R.demux(m, llr, cc, erase_punctured=True)
    ack_in = d["A1_in_ack"][0]
    k = m["kind"][m["inv"]["ack"]]
    assert np.array_equal(out["ack"][k == R.X], np.zeros((k == R.X).sum())) and (k == R.X).sum() == 14 and (k == R.Y).sum() == 7
    assert np.array_equal(out["ack"][k != R.X] < 0, np.where(k == R.Y, np.roll(ack_in, 1), ack_in)[k != R.X] == 1)
    assert np.array_equal(out["ulsch"][m["punct"]["ulsch"]], np.zeros(28))
    keep = ~m["punct"]["ulsch"]
    assert np.array_equal(out["ulsch"][keep] < 0, d["A1_in_ulsch"][0][keep] == 1)
    plain = R.demux(m, llr)
    assert np.array_equal(plain["ulsch"], llr[m["inv"]["ulsch"]]) and np.array_equal(plain["ack"], llr[m["inv"]["ack"]])


def test_gen_tbsize_equals_its_golden():
    d = np.load(os.path.join(GOLD, "uci_golden_tbsize.npz"))
    tables = [str(t) for t in d["tables"]]
    seen = set()
    for (ti, pi, mcs, RB, nsym, NL, addpos, cdm), (tbs, Qm, cr) in zip(d["inputs"].tolist(), d["out"].tolist()):
        cfg = {"mcs_table": tables[ti], "mcs_index": mcs, "nTpPi2BPSK": pi, "num_of_layers": NL, "NrOfSymbols": nsym,
               "ResAlloType1": {"RBSize": RB}, "DMRS": {"DMRSConfigType": 1, "NrOfDMRSSymbols": 1,
                                                        "NumCDMGroupsWithoutData": cdm, "DMRSAddPos": addpos}}
        got = ul_tbsize.gen_tbsize(cfg)
        assert got == (tbs, Qm, cr), (cfg, got, (tbs, Qm, cr))
        assert type(got[0]) is int and type(got[1]) is int
        seen.add((ti, pi, mcs))
    # every MCS index of every table, both tp-pi2BPSK settings of the two transform-precoding tables
    assert len(seen) == 2 * 28 + 2 * 28 + 28 + 29 and d["inputs"].shape[0] == 8 * len(seen)
    for name, c in CASES.items():   # and the eleven cases' (TBSize, Qm, rate)
        assert ul_tbsize.gen_tbsize(c["cfg"]) == (c["TBSize"], c["Qm"], c["coderateby1024"]), name
    assert ul_tbsize.gen_tbsize(dict(CASES["A1"]["cfg"], mcs_table="64qamlowse"))[1] == 2   # these two names in any case
    with pytest.raises(NameError):
        ul_tbsize.gen_tbsize(dict(CASES["A1"]["cfg"], mcs_table="mcstable61411"))             # ... these not
    for table, top in (("256QAM", 28), ("64QAMLowSE", 29), ("MCStable61411", 28), ("MCStable61412", 28)):
        with pytest.raises(AssertionError):
            ul_tbsize.gen_tbsize(dict(CASES["A1"]["cfg"], mcs_table=table, mcs_index=top))


def test_plan_is_linear_in_gtotal():
    cfg = R.case_config("ALL")
    cfg["ResAlloType1"]["RBSize"] = 273
    cfg["num_of_layers"] = 4
    cfg.update(NumACKBits=4, NumCSI1Bits=20, NumCSI2Bits=40)
    dmrs, Qm = [2, 11], 8
    G = uci.slot_bits(cfg, dmrs, Qm)
    assert G == 273 * 12 * 12 * 4 * 8
    rm = uci.rm_info(cfg, dmrs, 1277952, Qm, 948.0, G)
    t0 = time.perf_counter()
    blob = uci.plan_blob(273, 0, 14, dmrs, 2, 4, Qm, 4, 20, 40, 1, rm["Euci_ack"], rm["Euci_CSI1"], rm["Euci_CSI2"],
                         rm["Euci_ackrvd"], rm["G_ULSCH"], G)
    dt = time.perf_counter() - t0
    assert dt < 1.0, dt   # a guard against a quadratic builder, not a measurement
    p = uci.Plan(blob)
    m = p.expand()
    assert p.lens["ulsch"] == rm["G_ULSCH"] and sorted(np.concatenate(list(m["inv"].values())).tolist()) == list(range(G))


def test_plan_refusals():
    c = CASES["A2C"]
    rm = c["rm"]
    args = [3, 0, 14, c["dmrs"], 2, 2, 4, 2, 7, 0, 1, rm["Euci_ack"], rm["Euci_CSI1"], rm["Euci_CSI2"], rm["Euci_ackrvd"],
            rm["G_ULSCH"], c["Gtotal"]]
    assert uci.plan_blob(*args).size == 128 + 4 * c["Gtotal"] + 4 * (rm["G_ULSCH"] + rm["Euci_ack"] + rm["Euci_CSI1"])
    with pytest.raises(AssertionError, match="hopping"):
        uci.plan_blob(*args, frequency_hopping=1)
    with pytest.raises(AssertionError, match="hopping"):
        uci.plan(dict(c["cfg"], FrequencyHopping="intraSlot"), c["dmrs"], rm, 4)
    for i, v, word in ((16, c["Gtotal"] - 8, "Gtotal"), (15, rm["G_ULSCH"] - 8, "G_ULSCH"), (4, 3, "NumCDMGroups"),
                       (11, rm["Euci_ack"] + 3, "multiple"), (11, 8 * 200, "fit"), (6, 3, "Qm"), (0, 0, "allocation")):
        bad = list(args)
        bad[i] = v
        with pytest.raises(AssertionError, match=word):
            uci.plan_blob(*bad)
    n = _lib.lib().ldpc5g_uci_map_plan
    d = np.asarray(c["dmrs"], np.int32)
    buf = np.zeros(64, np.uint8)
    a = args[:3] + [ctypes.c_void_p(d.ctypes.data), d.size] + args[4:11] + [0] + args[11:]
    assert n(*a, ctypes.c_void_p(buf.ctypes.data), 64) == _lib.ESIZE and b"plan_bytes" in _lib.lib().ldpc5g_last_error()


def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "ldpc5g.h")) as f:
        h = f.read()
    for name, n in (("ldpc5g_uci_rm_info", 19), ("ldpc5g_uci_map_plan", 21), ("ldpc5g_uci_mux", 14), ("ldpc5g_uci_demux", 18),
                    ("ldpc5g_uci_scramble_modulate", 10), ("ldpc5g_smallblock_encode", 9), ("ldpc5g_smallblock_decode", 10)):
        m = re.search(name + r"\(([^;]*)\);", h)
        assert m, name
        assert len(m.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
