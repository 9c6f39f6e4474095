"""Generate tests/golden/polar_golden_sweep.npz by running the REFERENCE's polar code (py5gphy/polar) over
the stratified shape list of tests/polar_ref.py (fixture_shapes).  Only the outputs are committed.

    cd <root of a py5gphy checkout> && python <this repository>/tests/golden/gen_polar_sweep_golden.py [--seconds 600]

Per case: one shape of the list (every N in 32..1024, every rate-matching branch that N admits, PC bits
with nPCwm 0 and 1, CRC 6 / 11 / 24, padCRC, rnti for DL and UL, both iBIL, SC and SCL with L in
{1, 2, 3, 4, 5, 7, 8, 12, 16}, L <= 8 at N = 1024, E <= 2048) and one random block through encode_polar and
ratematch_polar, BPSK + AWGN at an SNR around the shape's waterfall, and the E channel LLRs rounded to
quarter steps (stored as int8 q, llr = q / 4, |llr| <= 31.75: exact in float64, and equal metrics are
common on such a grid).  Recorded: q, nr_decode_polar's (ck, status) of ratemrecover_polar's output,
polar_ref's pm (float.hex) and info classes, and whether the sent block came back.  The rate-recovered
row is not stored: polar_ref.rate_recover(reference_repetition=True) is asserted to reproduce it.

Candidates (PER_N per N) are visited round robin over N, so every stratum grows evenly, until `--seconds` of
reference decoding have passed (default 600) or the candidates are used up.  With L <= 8 at N = 1024 the
reference needs about 60 ms per case, so the 512 KiB cap binds long before ten minutes do: the committed
file holds 960 cases, 160 per N, decoded by the reference in 60 s, in 294110 bytes.  DL shapes stop at
K = 151 (see polar_ref.fixture_shapes).
Asserted here: polar_ref equals the reference on every case (rate recovery, ck, status); every info class
occurs at least 3 times; both statuses occur at least 3 times in every N stratum; at least 8 shapes per N;
the file is at most 512 KiB.
"""
import json
import os
import sys
import time

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, OUT)
sys.path.insert(0, os.getcwd())
import polar_ref as R  # noqa: E402
from gen_polar_golden import attach  # noqa: E402

from py5gphy.polar import nr_polar_decoder, nr_polar_encoder, nr_polar_ratematch, nr_polar_raterecover  # noqa: E402

PER_N = 160
OFFSETS = (-0.5, 1.0, 2.5, 4.0, 0.25, 1.75)   # dB above the capacity limit of rate K / E
CLASSES = ("early", "crc_fail", "not_best", "pc_kills", "median_ties", "crc_kills")


def main():
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 600.0
    shapes = R.fixture_shapes(PER_N)
    R.sweep_coverage(shapes)
    order = [n * PER_N + r for r in range(PER_N) for n in range(6)]   # round robin over the six N
    rng = np.random.default_rng(R.FIXTURE_SEED)
    meta, qs, cks = [], [], []
    spent = 0.0
    for j, i in enumerate(order):
        if spent > seconds and j % 6 == 0 and j >= 48:
            break
        s = shapes[i]
        K, E, nMax, iIL, crclen, pad, rnti, iBIL, algo, L = (s[k] for k in R.SWEEP_FIELDS)
        blk = attach(rng, K, crclen, pad, rnti)
        enc = nr_polar_encoder.encode_polar(blk, E, nMax, iIL)
        N = enc.size
        rm = nr_polar_ratematch.ratematch_polar(enc, K, E, iBIL)
        assert np.array_equal(enc, R.encode(blk, E, nMax, iIL)) and np.array_equal(rm, R.rate_match(enc, K, E, iBIL)), s
        snr = R.waterfall_db(K, E) + OFFSETS[(j // 6) % len(OFFSETS)]
        q = np.clip(np.round(4 * R.channel_llr(rng, rm, snr)), -127, 127).astype(np.int8)
        llr = q / 4.0
        t0 = time.time()
        rr = nr_polar_raterecover.ratemrecover_polar(llr, K, N, iBIL)
        ck, st = nr_polar_decoder.nr_decode_polar(algo, rr, E, K, L, nMax, iIL, crclen, pad, rnti)
        spent += time.time() - t0
        assert np.array_equal(rr, R.rate_recover(llr, K, N, iBIL, 20.0, reference_repetition=True)), s
        ck2, st2, pm, info = R.decode(algo, rr, E, K, L, nMax, iIL, crclen, pad, rnti)
        ckf = np.asarray(ck, np.int8) if st else -np.ones(K, np.int8)
        assert bool(st) == bool(st2) and np.array_equal(ckf, ck2), (s, snr)
        meta.append(dict(s, N=int(N), snr=round(float(snr), 3), status=int(bool(st)), pm=float(pm).hex(),
                         ok=int(bool(st) and np.array_equal(ckf, blk)), info={k: int(v) for k, v in info.items()}))
        qs.append(q)
        cks.append(ckf)
        if j % 24 == 0:
            print(f"  {j} cases, {spent:.0f} s of reference decoding", flush=True)
    have = {k: sum(1 for c in meta if c["info"][k]) for k in CLASSES}
    assert all(v >= 3 for v in have.values()), have
    for N in (32, 64, 128, 256, 512, 1024):
        st = [c["status"] for c in meta if c["N"] == N]
        assert len(st) >= 8 and sum(st) >= 3 and len(st) - sum(st) >= 3, (N, len(st), sum(st))
    R.sweep_coverage(meta)
    path = os.path.join(OUT, "polar_golden_sweep.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), q=np.concatenate(qs), ck=np.concatenate(cks))
    assert os.path.getsize(path) <= 512 * 1024, os.path.getsize(path)
    print(f"sweep: {len(meta)} cases in {spent:.0f} s of reference decoding; classes {have}; "
          f"{sum(c['status'] for c in meta)} succeed; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
