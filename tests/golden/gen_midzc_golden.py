"""Generate tests/golden/decode_midzc_golden.npz by running the REFERENCE's nr_decode_ldpc
(py5gphy/ldpc/nr_ldpc_decode.py:11) at the lifting sizes the other decode fixtures leave out: the 15
sizes 104 ... 352 of both base graphs, and BG2 Zc = 384.  Only inputs and outputs are committed.

    cd <root of a py5gphy checkout> && PYTHONDONTWRITEBYTECODE=1 python <this repository>/tests/golden/gen_midzc_golden.py

(the reference opens its tables through a path relative to its root, so the cwd must be that root.)

Cases
  min-sum  per (bg, Zc): one NMS (alpha 0.75, beta 0) and one OMS (alpha 1, beta 0.5) codeblock,
           L = 8; one of the two (alternating with the size's index and the base graph) has its
           last 5 + index % 20 extension columns zeroed, as rate recovery leaves columns that
           were never transmitted.  31 pairs, 62 cases.
  BF, BP   one codeblock each at (1, 104), (2, 144), (1, 208), (2, 352); L = 8 for BP and 64 for BF
           (bit flipping needs 30 ... 60 iterations to converge at these sizes).

Inputs.  A random codeword (the oracle's encoder, itself pinned by encode_golden.npz), BPSK + AWGN,
LLRs rounded to quarter steps and stored as int8 q (llr = q / 4, |llr| <= 31.75): exact in float32
and float64, and equal magnitudes are common on such a grid.  The SNR of a case comes from a ladder
of 0.25 dB steps applied to ONE noise draw: cases alternate between "the lowest rung at which the
oracle converges" and "the highest rung at which it does not", so about half of the reference's
statuses are True and every case sits at its waterfall.  The oracle only picks the rung: every
recorded ck / status is the reference's, and oracle == reference is asserted on every case.

The reference expands a dense H (7.7 GB of float64 state at BG1 Zc = 384), so cases run in a small
pool, largest first, one task per worker process; on 8 cores and 62 GB the file takes a few minutes.
"""
import multiprocessing as mp
import os
import sys
import time

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.getcwd())
import oracle_shim as O  # noqa: E402

MID = [104, 112, 120, 128, 144, 160, 176, 192, 208, 224, 240, 256, 288, 320, 352]
ALGO_PAIRS = [(1, 104), (2, 144), (1, 208), (2, 352)]
L = {"min-sum": 8, "BP": 8, "BF": 64}   # bit flipping needs 30 ... 60 iterations at these sizes
LADDER = {"min-sum": np.arange(4.0, -8.01, -0.25), "BP": np.arange(4.0, -8.01, -0.25),
          "BF": np.arange(9.0, 0.99, -0.25)}


def quantise(llr):
    return np.clip(np.rint(4 * llr), -127, 127).astype(np.int8)


def _oracle(q, bg, Zc, algo, alpha, beta):
    x = q.astype(np.float64) / 4
    if algo == "BF":
        return O.decode_bf(x, Zc, bg, L[algo])
    if algo == "BP":
        return O.decode_bp(x, Zc, bg, L[algo])
    return O.decode_flooding(x, Zc, bg, L[algo], alpha, beta, np.float64)


def make_case(rng, bg, Zc, algo, alpha, beta, nzero, want):
    """q int8[N] at the rung of the SNR ladder that `want` asks for (see the module docstring)."""
    K = (22 if bg == 1 else 10) * Zc
    dn = O.encode(rng.integers(0, 2, K).astype(np.int8), bg)
    noise = rng.normal(size=dn.size)
    snrs = LADDER[algo]
    q = np.stack([quantise(2 * ((1 - 2.0 * dn) + noise * 10 ** (-s / 20)) / 10 ** (-s / 10)) for s in snrs])
    if nzero:
        q[:, -nzero * Zc:] = 0
    st = _oracle(q, bg, Zc, algo, alpha, beta)[1]
    if want:
        k = int(np.nonzero(st)[0].max()) if st.any() else 0          # lowest SNR that converges
    else:
        k = int(np.nonzero(~st)[0].min()) if not st.all() else len(snrs) - 1   # highest that fails
    return q[k], float(snrs[k])


def _run(args):
    bg, Zc, algo, alpha, beta, q = args
    from py5gphy.ldpc import nr_ldpc_decode
    t = time.time()
    _, ck, status = nr_ldpc_decode.nr_decode_ldpc(q.astype(np.float64) / 4, Zc, bg, L[algo], algo, alpha, beta)
    return np.packbits(np.asarray(ck) != 0), bool(status), time.time() - t


def _offs(lst):
    return np.concatenate([[0], np.cumsum([x.size for x in lst])]).astype(np.int64)


def main():
    rng = np.random.default_rng(20261021)
    cases = []   # (bg, Zc, algo, alpha, beta, q, nzero, snr)
    n = 0
    for idx, Zc in enumerate(MID + [384]):
        for bg in ((1, 2) if Zc != 384 else (2,)):
            for k, (alpha, beta) in enumerate(((0.75, 0.0), (1.0, 0.5))):
                nzero = (5 + idx % 20) if (idx + bg + k) % 2 == 0 else 0
                # want True / False in turn, shifted so that both statuses meet both zeroed / plain
                q, snr = make_case(rng, bg, Zc, "min-sum", alpha, beta, nzero, (n + n // 4) % 2 == 0)
                cases.append((bg, Zc, "min-sum", alpha, beta, q, nzero, snr))
                n += 1
    for j, (bg, Zc) in enumerate(ALGO_PAIRS):
        for a, algo in enumerate(("BF", "BP")):
            q, snr = make_case(rng, bg, Zc, algo, 1.0, 0.0, 0, (j + a) % 2 == 0)
            cases.append((bg, Zc, algo, 1.0, 0.0, q, 0, snr))
    print("cases", len(cases), flush=True)
    order = sorted(range(len(cases)), key=lambda i: -cases[i][5].size)   # largest first
    t0 = time.time()
    with mp.Pool(4, maxtasksperchild=1) as pool:
        res_o = pool.map(_run, [cases[i][:6] for i in order], chunksize=1)
    res = [None] * len(cases)
    for i, r in zip(order, res_o):
        res[i] = r
    print("reference decodes done in %.0f s (sum of case times %.0f s)" % (time.time() - t0, sum(r[2] for r in res)))
    for c, r in zip(cases, res):   # oracle == reference, on every case
        ock, ost, _ = _oracle(c[5][None], c[0], c[1], c[2], c[3], c[4])
        assert np.array_equal(np.packbits(ock[0] != 0), r[0]) and bool(ost[0]) == r[1], c[:5]
    ms = [r[1] for c, r in zip(cases, res) if c[2] == "min-sum"]
    print("min-sum cases", len(ms), "reference status True", sum(ms))
    print("BF / BP cases", len(res) - len(ms), "status True", sum(r[1] for r in res) - sum(ms))
    assert 0.4 * len(ms) <= sum(ms) <= 0.6 * len(ms)
    path = os.path.join(OUT, "decode_midzc_golden.npz")
    np.savez_compressed(
        path, bg=np.array([c[0] for c in cases], np.int32), Zc=np.array([c[1] for c in cases], np.int32),
        algo=np.array([c[2] for c in cases]), L=np.array([L[c[2]] for c in cases], np.int32),
        alpha=np.array([c[3] for c in cases]), beta=np.array([c[4] for c in cases]),
        nzero=np.array([c[6] for c in cases], np.int32), snr=np.array([c[7] for c in cases]),
        q=np.concatenate([c[5] for c in cases]), q_off=_offs([c[5] for c in cases]),
        ck_bits=np.concatenate([r[0] for r in res]), ck_off=_offs([r[0] for r in res]),
        status=np.array([r[1] for r in res]))
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
