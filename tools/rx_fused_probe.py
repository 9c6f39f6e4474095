"""Fused receive front end probe: BASELINE config 5's shape (32 TBs x 129 codeblocks, 256QAM, cfg
as bench.bench_config5 builds it), the unfused pair (ldpc5g_demod_descramble +
ldpc5g_sch_raterecover) against the fused kernel (ldpc5g_sch_demod_raterecover) in one process,
alternating, each step event-timed on its own: 3 warm-ups, 20 steps, min / median / max.  Both
paths get precomputed scrambling words.  Two precisions: complex128 symbols -> float64 rows (the
reference's) and complex64 -> float32 rows (perf mode).  The outputs are compared first.

    python tools/rx_fused_probe.py [--T 32] [--steps 20] [--warmup 3] [--out profiles/rx_fused/probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from python_5gtoolbox_amd import phy  # noqa: E402
from python_5gtoolbox_amd.sch import SchWorkspace, sch_config, sch_demod_raterecover_batch, \
    sch_raterecover_batch  # noqa: E402

HBM_GBS = 8000.0   # MI355X peak HBM bandwidth, as bench.py's rooflines


def ev_each(fn, n):
    """n calls of fn, each between its own pair of device events -> [ms]."""
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms, nbytes):
    med = statistics.median(ms)
    return {"min_ms": round(min(ms), 5), "median_ms": round(med, 5), "max_ms": round(max(ms), 5),
            "bytes": nbytes, "hbm_frac_at_median": round(nbytes / (med * 1e-3) / 1e9 / HBM_GBS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--snr", type=float, default=28.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rx_fused", "probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda", 0)
    T = args.T
    A, Qm, R, NL, rv, G = (bench.C5[k] for k in ("A", "Qm", "R", "NL", "rv", "G"))
    cfg = sch_config(A, Qm, R, NL, rv, A, G)
    nsym = G // Qm
    g = torch.Generator(device=dev)
    g.manual_seed(505)
    # symbols of random bits through the mapper + AWGN, as the bench's channel
    bits = torch.randint(0, 2, (T, G), dtype=torch.int8, device=dev, generator=g)
    cinit = torch.arange(T, device=dev, dtype=torch.int64) * 2 ** 15 + 7
    words = phy.prbs_words(cinit, G)
    sym = phy.scramble_modulate(bits, Qm, words=words)
    nvar = 10 ** (-args.snr / 10)
    noise = torch.complex(torch.randn(sym.shape, device=dev, generator=g),
                          torch.randn(sym.shape, device=dev, generator=g)) * (nvar / 2) ** 0.5
    y64 = (sym + noise).contiguous()
    nv = torch.full(sym.shape, nvar, dtype=torch.float32, device=dev)
    del bits, noise, sym
    res = {"workload": f"BASELINE config 5 shape: {T} TBs x {cfg.C} codeblocks, 256QAM, E {cfg.E_lo}/{cfg.E_hi} per "
                       f"codeblock, N {cfg.N}, SNR {args.snr} dB", "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "lines": {}}
    for name, cdt, dnt in (("reference_precision_c128_f64", torch.complex128, torch.float64),
                           ("perf_c64_f32", torch.complex64, torch.float32)):
        y = y64.to(cdt)
        llr = torch.empty((T, G), dtype=torch.float32, device=dev)
        ws_a, ws_b = SchWorkspace(cfg, T, dev), SchWorkspace(cfg, T, dev)

        def pair():
            phy.demod_descramble(y, nv, Qm, words=words, out=llr)
            return sch_raterecover_batch(llr, cfg, None, dnt, ws_a)

        def fused():
            return sch_demod_raterecover_batch(y, nv, Qm, cfg, words=words, dn_dtype=dnt, ws=ws_b)
        same = bool(torch.equal(pair(), fused()))
        for _ in range(args.warmup):
            pair(), fused()
        tp, tf = [], []
        for _ in range(args.steps):   # alternating, each step timed on its own
            tp += ev_each(pair, 1)
            tf += ev_each(fused, 1)
        t_demod = ev_each(lambda: phy.demod_descramble(y, nv, Qm, words=words, out=llr), args.steps)
        t_rr = ev_each(lambda: sch_raterecover_batch(llr, cfg, None, dnt, ws_a), args.steps)
        ys, es = y.element_size(), torch.empty((), dtype=dnt).element_size()
        b_in = T * (nsym * (ys + 4) + G // 8)             # symbols + noise variances + scrambling words
        b_out = T * cfg.C * cfg.N * es                     # the rate-recovered rows
        b_llr = T * G * 4                                  # the demodulated LLRs, written then read
        sp, sf = stats(tp, b_in + 2 * b_llr + b_out), stats(tf, b_in + b_out)
        spread = sp["max_ms"] - sp["min_ms"]
        res["lines"][name] = {
            "outputs_equal": same, "unfused_pair": sp, "fused": sf,
            "demod_descramble_alone": stats(t_demod, b_in + b_llr), "raterecover_alone": stats(t_rr, b_llr + b_out),
            "bytes_per_tb": {"unfused": (b_in + 2 * b_llr + b_out) // T, "fused": (b_in + b_out) // T},
            "median_gain_ms": round(sp["median_ms"] - sf["median_ms"], 5), "pair_min_max_spread_ms": round(spread, 5),
            # a gain: the fused median is below the pair's by more than the pair's own spread
            "fused_is_a_gain": bool(sp["median_ms"] - sf["median_ms"] > spread)}
        print(name, json.dumps(res["lines"][name]), flush=True)
        del y, llr, ws_a, ws_b
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
