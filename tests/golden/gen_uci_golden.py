"""Generate tests/golden/uci_golden_{cases.json,map.npz,smallblock.npz,rminfo.npz,symbols.npz,tbsize.npz,decode.json,decode.npz} by running the
REFERENCE's UCI-on-PUSCH code.  The reference never travels: only its outputs and the inputs no formula
gives are committed.

    cd <root of a py5gphy checkout> && python <this repository>/tests/golden/gen_uci_golden.py
    (... gen_uci_golden.py --new writes only the tbsize and decode fixtures and leaves the other files untouched)

cases      per case of tests/uci_ref.py CASES: DMRS symbols, Qm, code rate, TBSize, ULSCH_size, Gtotal and
           getULSCH_RM_info's dict.
map        per case, three rows of different content: the four coded streams (random UL-SCH bits of length
           G_ULSCH, encode_uci_on_ulsch of random payloads), data_control_multiplex's g_seq, and the four
           streams data_control_separate makes of arange(Gtotal).
smallblock encode_smallblock of every message: K = 1, 2 per Qm in {1, 2, 4, 6, 8}; K = 3..11 (bit-packed).
rminfo     getULSCH_RM_info for 200 seeded random configurations, with a flag where the reference asserts
           (or divides by zero / indexes out of its tables).
symbols    nr_pusch_process on a g_seq with x and y placeholders for Qm = 2, 4, 6, 8.
tbsize     gen_tbsize for every MCS index of every table (both tp-pi2BPSK settings for the two transform
           precoding tables) over eight allocations (PRBs, symbols, layers, DMRS positions and CDM groups).
decode     two noisy receptions (cases A1 and A2C; ULSCHandUCIProcess of a random transport block, BPSK-style
           LLRs stored float32, junk at the placeholders): ULSCHandUCIDecodeProcess's status, transport block
           and the sha256 of the float64 bytes of its new LLRs; the second is noisy enough to fail its CRC.
Checked here: tests/uci_ref.py reproduces every recorded map, stream and codeword.
"""
import copy
import json
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.getcwd())
import uci_ref as R  # noqa: E402

from py5gphy.nr_pusch import (nr_pusch_datactrl_multiplex, nr_pusch_dmrs, nr_pusch_process, nr_pusch_uci,  # noqa: E402
                              nr_ulsch, nr_ulsch_info, ul_tbsize)
from py5gphy.smallblock import nr_smallblock_encoder  # noqa: E402

with open("py5gphy/nr_default_config/default_pusch_config.json") as f:
    DEFAULT = json.load(f)


def full_config(name):
    cfg = copy.deepcopy(DEFAULT)
    c = R.case_config(name)
    for k, v in c.items():
        if isinstance(v, dict):
            cfg[k].update(v)
        else:
            cfg[k] = v
    return cfg


def gen_cases():
    meta, arrs = {}, {}
    for ci, name in enumerate(R.CASES):
        cfg = full_config(name)
        dmrs = nr_pusch_dmrs.get_DMRS_symlist(cfg["StartSymbolIndex"] + cfg["NrOfSymbols"], cfg["DMRS"]["DMRSAddPos"])
        TBSize, Qm, cr = ul_tbsize.gen_tbsize(cfg)
        if cfg["EnableULSCH"] == 1:
            cbs, _, _ = nr_ulsch.ULSCH_Crc_CodeBlockSegment(np.zeros(TBSize, "i1"), TBSize, cr)
            usize = int(cbs.shape[0] * cbs.shape[1])
        else:
            usize = 0
        RB, nsym, start = cfg["ResAlloType1"]["RBSize"], cfg["NrOfSymbols"], cfg["StartSymbolIndex"]
        dre = 6 if cfg["DMRS"]["NumCDMGroupsWithoutData"] == 1 else 0
        nre = sum(RB * dre if s in dmrs else RB * 12 for s in range(start, start + nsym))
        G = Qm * cfg["num_of_layers"] * nre
        rm = nr_ulsch_info.getULSCH_RM_info(cfg, dmrs, usize, Qm, cr, G)
        rm = {k: int(v) for k, v in rm.items()}
        meta[name] = {"dmrs": [int(x) for x in dmrs], "Qm": int(Qm), "coderateby1024": float(cr), "TBSize": int(TBSize),
                      "ULSCH_size": usize, "Gtotal": int(G), "rm": rm}
        rng = np.random.default_rng(6270 + ci)
        rows = {k: [] for k in ("g_seq", "in_ulsch", "in_ack", "in_csi1", "in_csi2", "bits_ack", "bits_csi1", "bits_csi2")}
        for r in range(3):
            ins = {"ulsch": rng.integers(0, 2, rm["G_ULSCH"]).astype("i1")}
            for key, num, E in (("ack", "NumACKBits", "Euci_ack"), ("csi1", "NumCSI1Bits", "Euci_CSI1"),
                                ("csi2", "NumCSI2Bits", "Euci_CSI2")):
                A = cfg[num]
                b = rng.integers(0, 2, A).astype("i1")
                rows["bits_" + key].append(b)
                ins[key] = nr_pusch_uci.encode_uci_on_ulsch(b, A, rm[E], Qm).astype("i1") if A else np.zeros(0, "i1")
            g = nr_pusch_datactrl_multiplex.data_control_multiplex(ins["ulsch"], ins["ack"], ins["csi1"], ins["csi2"], cfg, G,
                                                                   dmrs, rm, Qm)
            rows["g_seq"].append(g.astype("i1"))
            for k in R.STREAMS:
                rows["in_" + k].append(ins[k])
        for k, v in rows.items():
            arrs[f"{name}_{k}"] = np.stack(v).astype(np.int8)
        sep = nr_pusch_datactrl_multiplex.data_control_separate(np.arange(G, dtype=np.float64), cfg, dmrs, rm, Qm)
        for k, v in zip(R.STREAMS, sep):
            arrs[f"{name}_{k}"] = np.asarray(v, np.float64).astype(np.int32)
        # the restatement against what was just recorded
        m = R.build_map(R.case_config(name), meta[name]["dmrs"], rm, Qm, G)
        for r in range(3):
            got = R.mux(m, {k: arrs[f"{name}_in_{k}"][r] for k in R.STREAMS})
            assert np.array_equal(got, arrs[f"{name}_g_seq"][r]), name
        d = R.demux(m, np.arange(G, dtype=np.float64))
        for k in R.STREAMS:
            assert np.array_equal(d[k], arrs[f"{name}_{k}"]), (name, k)
        print(name, meta[name], "placeholders", int((arrs[f"{name}_g_seq"][0] < 0).sum()), "punct", int(m["punct"]["ulsch"].sum()))
    with open(os.path.join(OUT, "uci_golden_cases.json"), "w") as f:
        json.dump({"cases": meta}, f, indent=1)
    np.savez_compressed(os.path.join(OUT, "uci_golden_map.npz"), **arrs)


def gen_smallblock():
    arrs = {}
    for K in (1, 2):
        for Qm in (1, 2, 4, 6, 8):
            msgs = (np.arange(2 ** K)[:, None] >> (K - 1 - np.arange(K))) & 1
            cw = np.stack([nr_smallblock_encoder.encode_smallblock(m.astype("i1"), Qm) for m in msgs])
            arrs[f"K{K}_Qm{Qm}"] = cw.astype(np.int8)
            assert np.array_equal(R.sb_encode(msgs, Qm), cw)
    for K in range(3, 12):
        msgs = (np.arange(2 ** K)[:, None] >> (K - 1 - np.arange(K))) & 1
        cw = np.stack([nr_smallblock_encoder.encode_smallblock(m.astype("i1")) for m in msgs]).astype(np.int8)
        assert np.array_equal(R.sb_encode(msgs, 2), cw)
        arrs[f"K{K}"] = np.packbits(cw.astype(np.uint8), axis=1)
    np.savez_compressed(os.path.join(OUT, "uci_golden_smallblock.npz"), **arrs)


RM_IN = ("RBSize", "StartSymbolIndex", "NrOfSymbols", "DMRSAddPos", "NL", "Qm", "ULSCH_size", "EnableULSCH", "OACK",
         "OCSI1", "OCSI2", "I_ack", "I_csi1", "I_csi2", "Gtotal")
RM_OUT = ("Euci_ack", "Qbar_ACK", "Euci_CSI1", "Qbar_CSI1", "Euci_CSI2", "Qbar_CSI2", "Euci_ackrvd", "Qbar_ACKrvd", "G_ULSCH")


def gen_rminfo():
    rng = np.random.default_rng(63241)
    ins, crs, scal, outs, bad, dm = [], [], [], [], [], []
    while len(ins) < 200:
        RB = int(rng.choice([1, 2, 3, 6, 11, 24, 52, 106, 273]))
        start = int(rng.choice([0, 0, 2]))
        nsym = int(rng.integers(6, 15 - start))
        addpos = int(rng.integers(0, 3))
        NL = int(rng.choice([1, 1, 2, 4]))
        Qm = int(rng.choice([2, 4, 6, 8]))
        cr = float(rng.choice([120, 193, 308, 378, 466.5, 567, 682.5, 797, 948]))
        en = int(rng.random() < 0.8)
        oack = int(rng.choice([0, 1, 2, 3, 7, 11, 12, 19, 20, 40]))
        ocsi1 = int(rng.choice([0, 0, 5, 11, 12, 20, 60]))
        ocsi2 = int(rng.choice([0, 0, 7, 15, 40, 400])) if ocsi1 else 0
        ia, i1, i2 = int(rng.integers(0, 17)), int(rng.integers(0, 20)), int(rng.integers(0, 20))
        s = float(rng.choice([0.5, 0.65, 0.8, 1]))
        dmrs = nr_pusch_dmrs.get_DMRS_symlist(start + nsym, addpos)
        nre = sum(0 if sy in dmrs else RB * 12 for sy in range(start, start + nsym))
        G = Qm * NL * nre
        usize = int(rng.integers(1, 40) * G // 40 // 8 * 8) if en else 0
        cfg = {"EnableULSCH": en, "UCIScaling": s, "EnableACK": int(oack > 0), "NumACKBits": oack, "I_HARQ_ACK_offset": ia,
               "EnableCSI1": int(ocsi1 > 0), "NumCSI1Bits": ocsi1, "I_CSI1offset": i1, "EnableCSI2": int(ocsi2 > 0),
               "NumCSI2Bits": ocsi2, "I_CSI2offset": i2, "ResAlloType1": {"RBSize": RB}, "StartSymbolIndex": start,
               "NrOfSymbols": nsym, "num_of_layers": NL}
        try:
            rm = nr_ulsch_info.getULSCH_RM_info(cfg, dmrs, usize, Qm, cr, G)
            o, b = [int(rm[k]) for k in RM_OUT], 0
        except (AssertionError, ZeroDivisionError, IndexError):
            o, b = [0] * 9, 1
        ins.append([RB, start, nsym, addpos, NL, Qm, usize, en, oack, ocsi1, ocsi2, ia, i1, i2, G])
        dm.append(list(dmrs) + [-1] * (4 - len(dmrs)))
        crs.append(cr), scal.append(s), outs.append(o), bad.append(b)
    print("rminfo: refused", sum(bad), "of", len(bad))
    assert 20 < sum(bad) < 150
    np.savez_compressed(os.path.join(OUT, "uci_golden_rminfo.npz"), inputs=np.array(ins, np.int64), dmrs=np.array(dm, np.int32),
                        coderate=np.array(crs), scaling=np.array(scal), out=np.array(outs, np.int64), refused=np.array(bad, np.int8))


def gen_symbols():
    rng = np.random.default_rng(6311)
    arrs = {}
    for Qm in (2, 4, 6, 8):
        parts = []
        for i in range(12):
            parts.append(rng.integers(0, 2, Qm * int(rng.integers(1, 6))).astype("i1"))
            K = 1 + i % 2
            parts.append(nr_smallblock_encoder.encode_smallblock(rng.integers(0, 2, K).astype("i1"), Qm))
        g = np.concatenate(parts).astype("i1")
        rnti, nID = 1000 + Qm, 37 * Qm
        sym = nr_pusch_process.nr_pusch_process(g, rnti, nID, Qm, 1, 0, 1, 1, np.ones((1, 1)))
        arrs[f"g{Qm}"] = g
        arrs[f"sym{Qm}"] = np.asarray(sym).reshape(-1).astype(np.complex64)
        arrs[f"id{Qm}"] = np.array([rnti, nID])
        c = R.prbs(rnti * 2 ** 15 + nID, g.size)
        assert (g == -2).sum() >= 6 and ((g == -1).sum() > 0) == (Qm > 2)
        from py5gphy.common import nrModulation
        mod = {2: "QPSK", 4: "16QAM", 6: "64QAM", 8: "256QAM"}[Qm]
        assert np.array_equal(nrModulation.nrModulate(R.scramble(g, c), mod).astype(np.complex64), arrs[f"sym{Qm}"])
    np.savez_compressed(os.path.join(OUT, "uci_golden_symbols.npz"), **arrs)


ALLOCS = [(1, 14, 1, 0, 2), (2, 12, 1, 0, 2), (3, 14, 2, 1, 2), (24, 14, 1, 1, 1), (52, 9, 2, 1, 2), (106, 7, 4, 3, 1),
          (273, 14, 4, 2, 2), (273, 11, 1, 3, 2)]     # RBSize, NrOfSymbols, layers, DMRSAddPos, CDM groups
TABLES = [("MCStable61411", 28, (0, 1)), ("MCStable61412", 28, (0, 1)), ("256QAM", 28, (0,)), ("64QAMLowSE", 29, (0,))]


def gen_tbsize():
    rows, out = [], []
    for ti, (table, n, pis) in enumerate(TABLES):
        for pi in pis:
            for mcs in range(n):
                for RB, nsym, NL, addpos, cdm in ALLOCS:
                    cfg = {"mcs_table": table, "mcs_index": mcs, "nTpPi2BPSK": pi, "num_of_layers": NL, "NrOfSymbols": nsym,
                           "ResAlloType1": {"RBSize": RB}, "DMRS": {"DMRSConfigType": 1, "NrOfDMRSSymbols": 1,
                                                                    "NumCDMGroupsWithoutData": cdm, "DMRSAddPos": addpos}}
                    tbs, Qm, cr = ul_tbsize.gen_tbsize(cfg)
                    rows.append([ti, pi, mcs, RB, nsym, NL, addpos, cdm])
                    out.append([float(tbs), float(Qm), float(cr)])
    print("tbsize rows", len(rows))
    np.savez_compressed(os.path.join(OUT, "uci_golden_tbsize.npz"), tables=np.array([t[0] for t in TABLES]),
                        inputs=np.array(rows, np.int32), out=np.array(out, np.float64))


DEC = {"L": 6, "algo": "min-sum", "alpha": 0.8, "beta": 0.0}


def gen_decode():
    import hashlib

    from py5gphy.nr_pusch import nr_pusch_uci_decode
    rng = np.random.default_rng(6262)
    meta, arrs = [], {}
    for i, (name, sigma) in enumerate((("A1", 0.5), ("A2C", 1.3))):
        cfg = full_config(name)
        cfg["ACKbits"] = rng.integers(0, 2, cfg["NumACKBits"]).astype("i1")     # the reference wants arrays here
        cfg["CSI1bits"] = rng.integers(0, 2, cfg["NumCSI1Bits"]).astype("i1")
        dmrs = nr_pusch_dmrs.get_DMRS_symlist(cfg["StartSymbolIndex"] + cfg["NrOfSymbols"], cfg["DMRS"]["DMRSAddPos"])
        TBSize, Qm, cr = ul_tbsize.gen_tbsize(cfg)
        G = R.load_cases(OUT)[name]["Gtotal"]
        trblk = rng.integers(0, 2, TBSize).astype("i1")
        g = nr_pusch_uci.ULSCHandUCIProcess(cfg, trblk, G, 0, dmrs)
        llr = (np.where(g < 0, 0.0, 1.0 - 2.0 * g) + sigma * rng.normal(size=G)) * 2 / sigma ** 2
        llr = llr.astype(np.float32)
        ok, tbblk, new = nr_pusch_uci_decode.ULSCHandUCIDecodeProcess(llr.astype(np.float64), cfg, 0, DEC)
        meta.append({"case": name, "ACKbits": cfg["ACKbits"].tolist(), "CSI1bits": cfg["CSI1bits"].tolist(), "ok": bool(ok), "TBSize": int(TBSize),
                     "decoded_right": bool(np.array_equal(tbblk, trblk)), "new_shape": list(np.shape(new)),
                     "new_sha": hashlib.sha256(np.ascontiguousarray(new, np.float64).tobytes()).hexdigest()})
        arrs[f"trblk{i}"], arrs[f"g{i}"], arrs[f"llr{i}"] = trblk, g.astype(np.int8), llr
        arrs[f"tbblk{i}"] = np.asarray(tbblk).astype(np.int8)
        print("decode", meta[-1]["case"], "ok", ok, "right", meta[-1]["decoded_right"], np.shape(new))
    assert meta[0]["ok"] and not meta[1]["ok"]
    with open(os.path.join(OUT, "uci_golden_decode.json"), "w") as f:
        json.dump({"decoder": DEC, "cases": meta}, f, indent=1)
    np.savez_compressed(os.path.join(OUT, "uci_golden_decode.npz"), **arrs)


if __name__ == "__main__":
    if "--new" in sys.argv:      # only the fixtures added last: the others stay byte for byte
        gen_tbsize()
        gen_decode()
        sys.exit(0)
    gen_smallblock()
    gen_rminfo()
    gen_symbols()
    gen_cases()
    gen_tbsize()
    gen_decode()
    for n in sorted(os.listdir(OUT)):
        if n.startswith("uci_golden"):
            print(n, os.path.getsize(os.path.join(OUT, n)))
