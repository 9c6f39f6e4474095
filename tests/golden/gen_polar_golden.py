"""Generate tests/golden/polar_golden_{construct,chain,decode}.npz by running the REFERENCE's polar
code (py5gphy/polar).  The reference never travels: only its outputs and the inputs no formula gives
are committed.

    cd <root of a py5gphy checkout> && python <this repository>/tests/golden/gen_polar_golden.py

construct  F, qPC, N, nPC, nPCwm of polar_construct.construct for ~200 (K, E, nMax) triples; asserted to
           cover every N in 32..1024, repetition, shortening, puncturing with both ulim branches, and
           nPC = 3 with nPCwm 0 and 1; (19, 30, 10), (20, 256, 10) and (18, 25, 10) are forced in.
chain      for a subset of those shapes and both iBIL: random block, encode_polar, ratematch_polar,
           noisy LLRs, ratemrecover_polar (the UL repetition case (311, 2100) shows the reference's
           quirk); polar_cbsegment for six (A, E), among them C = 2 with odd A.
decode     rate-recovered LLRs with nr_decode_polar's (ck, status) and polar_ref's path metric pm
           (float.hex; inf on failure): SC and SCL with L in
           {1, 2, 3, 8, 16, 32}, DL with padCRC 0 and 1 (rnti), UL CRC6 with PC bits, UL CRC11,
           N in {32, 64, 256, 512, 1024}, N = 1024 at L = 32, punctured inputs with exact zeros.
           Seeds are searched until each of five classes has >= 3 cases: early termination, no path
           passing the final CRC, a returned path that is not the lowest-metric one, a path killed
           at a PC bit, a split with a metric equal to the median (classified with tests/polar_ref.py).
           Every second searched input has its LLRs rounded to integers: with continuous noise two
           equal metrics at the median did not occur in 4000 decodes, on an integer grid they do.
pins       tests/golden/polar_bler_pins.json: the 224 BLER values the reference published in
           out/polar_decode_result_all.pickle and out/polar_decode_result_all_testcases.pickle, each with
           algo, L, test case [K, N, nMax, iIL, CRCLEN, padCRC, rnti] (K before the CRC), snr and n_ref,
           the smallest trial count of the stopping rule (200 / 400 / 800 / 2000 trials with at least
           10 / 5 / 2 / 0 failures) consistent with the value.  `--pins` writes only this file.
Checked here: polar_ref reproduces every recorded output; SCL_optionB == SCL and SC_optionB == SC.
"""
import json
import os
import sys
import time

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.getcwd())
import polar_ref as R  # noqa: E402

from py5gphy.crc import crc  # noqa: E402
from py5gphy.polar import (nr_polar_cbsegment, nr_polar_decoder, nr_polar_encoder, nr_polar_ratematch,  # noqa: E402
                           nr_polar_raterecover, polar_construct)

FORCED = [(19, 30, 10), (20, 256, 10), (18, 25, 10)]


def cfg_of(K, nMax):
    """(iIL, CRCLEN) the standard pairs with (K, nMax)."""
    return (1, 24) if nMax == 9 else (0, 6 if K <= 25 else 11)


def triples():
    rng = np.random.default_rng(38212)
    out = list(FORCED)
    while len(out) < 200:
        nMax = int(rng.choice([9, 10]))
        if nMax == 9:
            K = int(rng.integers(25, 165))
        else:
            K = int(rng.integers(18, 26)) if rng.random() < 0.3 else int(rng.integers(31, 600))
        kind = rng.random()
        lo = K + 3
        if kind < 0.35:
            E = int(rng.integers(lo, max(lo + 1, 3 * K)))
        elif kind < 0.7:
            E = int(rng.integers(lo, min(8192, 12 * K) + 1))
        else:
            E = int(rng.integers(lo, 8193))
        if (K, E, nMax) not in out:
            out.append((K, E, nMax))
    return out


def gen_construct(tr):
    store, seen = {}, set()
    meta = []
    for i, (K, E, nMax) in enumerate(tr):
        F, qPC, N, nPC, nPCwm = polar_construct.construct(K, E, nMax)
        f2, q2, n2, p2, w2 = R.construct(K, E, nMax)
        assert np.array_equal(F, f2) and np.array_equal(qPC, q2) and (N, nPC, nPCwm) == (n2, p2, w2), (K, E, nMax)
        store[f"F{i}"] = np.asarray(F, np.int8)
        meta.append([K, E, nMax, int(N), int(nPC), int(nPCwm)] + [int(v) for v in qPC] + [-1] * (3 - len(qPC)))
        m = R.mode(K, E, N)
        seen.add(("N", int(N)))
        seen.add(m if m != "punct" else ("punct", 4 * E >= 3 * N))
        seen.add(("pc", int(nPC), int(nPCwm)))
    want = {("N", 1 << n) for n in range(5, 11)} | {"rep", "short", ("punct", True), ("punct", False), ("pc", 3, 0),
                                                   ("pc", 3, 1), ("pc", 0, 0)}
    assert want <= seen, want - seen
    store["meta"] = np.array(meta, np.int32)
    np.savez_compressed(os.path.join(OUT, "polar_golden_construct.npz"), **store)
    print("construct:", len(tr), "triples")


def attach(rng, K, crclen, padCRC, rnti):
    poly = {6: "6", 11: "11", 24: "24C"}[crclen]
    a = rng.integers(0, 2, K - crclen).astype(np.int8)
    if padCRC:
        blk = crc.nr_crc_encode(np.concatenate((np.ones(24, "i1"), a)), poly, rnti)[24:]
    else:
        blk = crc.nr_crc_encode(a, poly, rnti if crclen != 24 else 0)
    assert np.array_equal(blk, R.crc_attach(a, crclen, rnti if (padCRC or crclen != 24) else 0, padCRC))
    return blk.astype(np.int8)


def rx_llr(rng, K, E, nMax, iIL, iBIL, snr_db, blk):
    enc = nr_polar_encoder.encode_polar(blk, E, nMax, iIL)
    rm = nr_polar_ratematch.ratematch_polar(enc, K, E, iBIL)
    sigma = 10 ** (-snr_db / 20)
    llr_e = 2 * ((1 - 2.0 * rm) + rng.normal(0, sigma, E)) / sigma ** 2
    rr = nr_polar_raterecover.ratemrecover_polar(llr_e, K, enc.size, iBIL)
    return enc, rm, llr_e, rr


CHAIN = [(19, 30, 10), (20, 256, 10), (25, 64, 10), (40, 64, 9), (40, 60, 9), (32, 100, 9), (64, 216, 9), (100, 512, 9),
         (140, 1000, 9), (33, 150, 10), (150, 512, 10), (211, 1024, 10), (211, 900, 10), (400, 800, 10),
         (311, 2100, 10), (60, 70, 10)]


def gen_chain():
    rng = np.random.default_rng(5341)
    store, meta = {}, []
    for K, E, nMax in CHAIN:
        iIL, crclen = cfg_of(K, nMax)
        for iBIL in (0, 1):
            i = len(meta)
            blk = attach(rng, K, crclen, 0, 0)
            enc, rm, llr_e, rr = rx_llr(rng, K, E, nMax, iIL, iBIL, 6.0, blk)
            N = enc.size
            assert np.array_equal(enc, R.encode(blk, E, nMax, iIL)), (K, E, nMax)
            assert np.array_equal(rm, R.rate_match(enc, K, E, iBIL)), (K, E, nMax, iBIL)
            assert np.array_equal(rr, R.rate_recover(llr_e, K, N, iBIL, 20.0, reference_repetition=True))
            quirk = int(not np.array_equal(rr, R.rate_recover(llr_e, K, N, iBIL, 20.0)))
            assert quirk == int(iBIL == 1 and E >= N), (K, E, iBIL, quirk)
            store.update({f"blk{i}": blk, f"enc{i}": enc.astype(np.int8), f"rm{i}": rm.astype(np.int8),
                          f"llr{i}": llr_e, f"rr{i}": rr})
            meta.append([K, E, nMax, iIL, iBIL, N, quirk])
    # the quirk's consequence: the reference's own UL repetition chain fails where the de-interleaved sum decodes
    K, E, nMax = 311, 2100, 10
    blk = attach(rng, K, 11, 0, 0)
    enc, rm, llr_e, rr = rx_llr(rng, K, E, nMax, 0, 1, 30.0, blk)
    ck, st = nr_polar_decoder.nr_decode_polar("SCL", rr, E, K, 8, nMax, 0, 11)
    assert not (st and np.array_equal(ck, blk))
    ck2, st2, _, _ = R.decode("SCL", R.rate_recover(llr_e, K, 1024, 1), E, K, 8, nMax, 0, 11)
    assert st2 and np.array_equal(ck2, blk)
    store.update(quirk_blk=blk, quirk_llr=llr_e, quirk_rr=rr, quirk_status=np.array([int(st)]))
    seg = []
    for j, (A, Euci) in enumerate([(12, 60), (19, 100), (20, 100), (361, 1088), (1013, 2000), (360, 1000)]):
        bits = rng.integers(0, 2, A).astype(np.int8)
        blks, C, Er = nr_polar_cbsegment.polar_cbsegment(bits, Euci)
        b2, c2, e2 = R.cbsegment(bits, Euci)
        assert np.array_equal(blks, b2) and (C, Er) == (c2, e2)
        store[f"seg_in{j}"], store[f"seg_out{j}"] = bits, np.asarray(blks, np.int8)
        seg.append([A, Euci, C, Er])
    assert any(c == 2 and a % 2 for a, _, c, _ in seg)
    store["meta"], store["seg_meta"] = np.array(meta, np.int32), np.array(seg, np.int32)
    np.savez_compressed(os.path.join(OUT, "polar_golden_chain.npz"), **store)
    print("chain:", len(meta), "cases,", len(seg), "segmentations")


# (name, K, E, nMax, padCRC, rnti): DL plain, DL DCI with rnti, UL CRC6 + PC, UL CRC11
SHAPES = [("dl32", 28, 32, 9, 0, 0), ("dl64", 40, 64, 9, 1, 0x1234), ("dl256p", 64, 216, 9, 1, 0xbeef),
          ("dl512", 100, 512, 9, 0, 0), ("ul32pc", 19, 30, 10, 0, 0), ("ul64pc", 20, 64, 10, 0, 0),
          ("ul256pc", 20, 256, 10, 0, 0), ("ul64", 40, 64, 10, 0, 0), ("ul512", 150, 512, 10, 0, 0),
          ("ul1024", 211, 1024, 10, 0, 0), ("ul1024p", 211, 900, 10, 0, 0), ("ul256p", 40, 200, 10, 0, 0x15)]
ALGOS = [("SC", 1), ("SCL", 1), ("SCL", 2), ("SCL", 3), ("SCL", 8), ("SCL", 16), ("SCL", 32)]


def gen_decode():
    rng = np.random.default_rng(20261020)
    cases = []   # dicts: params, llr, ck, status

    def run(shape, algo, L, snr, check_b=True, quant=False):
        name, K, E, nMax, padCRC, rnti = shape
        iIL, crclen = cfg_of(K, nMax)
        blk = attach(rng, K, crclen, padCRC, rnti)
        _, _, _, rr = rx_llr(rng, K, E, nMax, iIL, 0, snr, blk)
        if quant:   # LLRs on an integer grid, as a fixed-point front end delivers: equal metrics become common
            rr = np.round(rr)
        ck, st = nr_polar_decoder.nr_decode_polar(algo, rr, E, K, L, nMax, iIL, crclen, padCRC, rnti)
        ck2, st2, pm, info = R.decode(algo, rr, E, K, L, nMax, iIL, crclen, padCRC, rnti)
        ckf = np.asarray(ck, np.int8) if st else -np.ones(K, np.int8)
        assert bool(st) == bool(st2) and np.array_equal(ckf, ck2), (shape, algo, L, snr)
        if check_b:
            ckb, stb = nr_polar_decoder.nr_decode_polar(algo + "_optionB", rr, E, K, L, nMax, iIL, crclen, padCRC, rnti)
            assert bool(stb) == bool(st) and np.array_equal(np.asarray(ckb), np.asarray(ck)), (shape, algo, L)
        return dict(name=name, K=K, E=E, nMax=nMax, iIL=iIL, CRCLEN=crclen, padCRC=padCRC, rnti=rnti, algo=algo, L=L,
                    snr=snr, status=int(bool(st)), pm=float(pm).hex(), ok=int(bool(st) and np.array_equal(ckf, blk)),
                    info={k: int(v) for k, v in info.items()}), rr, ckf

    for shape in SHAPES:
        N = 1 << R.n_value(shape[1], shape[2], shape[3])
        for algo, L in ALGOS:
            if N == 1024 and (algo, L) in (("SCL", 1), ("SCL", 2), ("SCL", 3)):
                continue
            for snr in ((1.0, 4.0) if N <= 256 else (2.0,)):
                t0 = time.time()
                cases.append(run(shape, algo, L, snr, check_b=N < 1024 or L <= 8))
                if N == 1024:
                    print(f"  {shape[0]} {algo} L={L}: {time.time() - t0:.1f} s", flush=True)
    # the classes the fixtures must hold, searched on small shapes where a decode takes milliseconds
    need = {"early": 3, "crc_fail": 3, "not_best": 3, "pc_kills": 3, "median_ties": 3}
    have = {k: sum(1 for c in cases if c[0]["info"][k]) for k in need}
    small = [s for s in SHAPES if (1 << R.n_value(s[1], s[2], s[3])) <= 256]
    tries = 0
    while any(have[k] < need[k] for k in need) and tries < 4000:
        tries += 1
        shape = small[int(rng.integers(len(small)))]
        L = int(rng.choice([2, 3, 4, 8]))
        c = run(shape, "SCL", L, float(rng.choice([-1.0, 0.0, 1.0, 2.0, 3.0])), check_b=False,
                quant=tries % 2 == 1)
        gain = [k for k in need if c[0]["info"][k] and have[k] < need[k]]
        if gain:
            cases.append(c)
            for k in need:
                have[k] += bool(c[0]["info"][k])
    assert all(have[k] >= need[k] for k in need), have
    print("decode:", len(cases), "cases; classes", have, "after", tries, "searched")
    store = {"meta": np.array(json.dumps([c[0] for c in cases]))}
    for i, (_, rr, ck) in enumerate(cases):
        store[f"llr{i}"], store[f"ck{i}"] = rr, ck
    path = os.path.join(OUT, "polar_golden_decode.npz")
    np.savez_compressed(path, **store)
    assert os.path.getsize(path) <= 512 * 1024, os.path.getsize(path)


def n_ref(p):
    for n, lim in ((200, 10), (400, 5), (800, 2), (2000, 0)):
        f = p * n
        if abs(f - round(f)) < 1e-6 and round(f) >= lim:
            return n
    raise AssertionError(f"BLER {p} is not attainable under the stopping rule")


def gen_pins():
    import pickle
    pins = []
    for src in ("polar_decode_result_all", "polar_decode_result_all_testcases"):
        with open(os.path.join("out", src + ".pickle"), "rb") as f:
            _, _, results = pickle.load(f)
        for row in results:
            algo, L, tc = row[0]
            for snr, bler in row[1:]:
                pins.append(dict(src=src, algo=algo, L=int(L), testcase=[int(v) for v in tc], snr=float(snr),
                                 bler=float(bler), n_ref=n_ref(float(bler))))
    assert len(pins) == 224, len(pins)
    with open(os.path.join(OUT, "polar_bler_pins.json"), "w") as f:
        json.dump({"pins": pins}, f, indent=0)
    print("pins:", len(pins))


if __name__ == "__main__":
    if "--pins" in sys.argv:
        gen_pins()
        sys.exit(0)
    gen_pins()
    gen_construct(triples())
    gen_chain()
    gen_decode()
