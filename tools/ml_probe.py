"""ML detector probe: ldpc5g_ml_detect at BASELINE config 5's slot shape (nre = 36036 data REs)
on a 2x2 channel with 256QAM — 65 536 candidates per RE for the exhaustive searches — for each of
the ten algorithm names, complex128 storage, float64 LLRs.  Every call is event-timed on its own:
warm-ups, then interleaved steps of every variant, min / median / max.  The same loop times the
linear path it stands beside, equalize (MMSE) followed by demod_descramble, as the comparison.
Nothing is required of these times; they are recorded.

    python tools/ml_probe.py [--T 1] [--steps 7] [--warmup 2] [--out profiles/ml/probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from python_5gtoolbox_amd import _lib, phy  # noqa: E402

NRE, NR, NL, QM = 36036, 2, 2, 8


def ev(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"min_ms": round(min(ms), 5), "median_ms": round(statistics.median(ms), 5),
            "max_ms": round(max(ms), 5), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ml", "probe.json"))
    args = ap.parse_args()
    T = args.T
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)

    def cn(*shape):
        return torch.complex(torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen),
                             torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)) / 2 ** 0.5
    bits = torch.randint(0, 2, (T, NRE * NL * QM), dtype=torch.int8, device="cuda", generator=gen)
    x = phy.scramble_modulate(bits, QM).to(torch.complex128)
    h = cn(T, NRE, NR, NL)
    sigma2 = 10 ** (-25 / 10)
    y = ((h @ x.view(T, NRE, NL, 1))[..., 0] + cn(T, NRE, NR) * sigma2 ** 0.5).contiguous()
    g = cn(T, NRE // 12, NR, 1)
    cov = sigma2 * (torch.eye(NR, dtype=torch.complex128, device="cuda") + 0.5 * g @ g.conj().transpose(2, 3))
    cov = ((cov + cov.conj().transpose(2, 3)) / 2).contiguous()

    def linear():
        sym, nv = phy.equalize(y, h, cov, "MMSE")
        return phy.demod_descramble(sym, nv, QM)
    variants = {name: (lambda name=name: phy.ml_detect(y, h, cov, QM, name)) for name in _lib.ML_ALGO}
    variants["equalize(MMSE) + demod_descramble"] = linear
    times = {k: [] for k in variants}
    ber = {}
    for k, fn in variants.items():
        for _ in range(args.warmup):
            out = fn()
        torch.cuda.synchronize()
        ber[k] = float(((out < 0).to(torch.int8) != bits).double().mean())   # sanity: the detectors detect
    for _ in range(args.steps):
        for k, fn in variants.items():
            times[k].append(ev(fn))
    res = {"shape": {"T": T, "nre": NRE, "Nr": NR, "NL": NL, "Qm": QM, "storage": "complex128",
                     "llr": "float64 (ML), float32 (linear)", "snr_dB": 25},
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps": args.steps,
           "timing": "HIP events around each call, variants interleaved within a step",
           "ms": {k: stats(v) for k, v in times.items()}, "raw_bit_error_rate": ber}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["ms"], indent=1))
    print(json.dumps(ber))


if __name__ == "__main__":
    main()
