"""Polar codec throughput and latency on the GPU -> profiles/polar/probe.json.

    python tools/polar_probe.py                      event-timed kernels at B = 4096 and B = 1 (needs a GPU)
    python tools/polar_probe.py --reference ROOT     times the reference's own decoder (py5gphy under ROOT) on one
                                                     core for the same shapes and merges it into the same file

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o polar -- python tools/polar_probe.py --once
    python tools/polar_probe.py --trace DIR          merges the polar kernels' rows of the trace statistics
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv \
        -d DIR -o polar -- python tools/polar_probe.py --once      (counters only, a run of its own)
    python tools/polar_probe.py --counters DIR       merges the counters, summed per kernel

(--once: one warm-up and one call of each kernel per shape at B = 4096.)

Shapes: DCI (K 64, E 216, N 256, L 8), UCI (K 211, E 1024, N 1024, L 8) and the same UCI at L 32 (two LLR layers
in the global workspace).  Inputs are noisy codewords at 3 dB, so the list is busy.  Each figure is the median of
REPS event-timed launches after WARM warm-up launches.
"""
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "polar", "probe.json")
SHAPES = [("DCI", 64, 216, 9, 1, 24, 8), ("UCI_L8", 211, 1024, 10, 0, 11, 8), ("UCI_L32", 211, 1024, 10, 0, 11, 32)]
B, WARM, REPS, SNR = 4096, 3, 10, 3.0


def _load():
    try:
        with open(OUT) as f:
            return json.load(f)
    except OSError:
        return {}


def _save(d):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
    print("wrote", os.path.relpath(OUT, ROOT))


def gpu():
    import torch

    from python_5gtoolbox_amd import polar

    def timed(fn):
        for _ in range(WARM):
            fn()
        ts = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts))

    res = _load()
    res["device"] = torch.cuda.get_device_name(0)
    res["method"] = f"median of {REPS} event-timed launches after {WARM} warm-ups; inputs at {SNR} dB"
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1)
    for name, K, E, nMax, iIL, crclen, L in SHAPES:
        p = polar.plan(K, E, nMax, iIL, crclen)
        row = dict(K=K, E=E, N=p.N, L=L, mode=p.mode_name)
        for nb in (B, 1):
            bits = torch.randint(0, 2, (nb, K), generator=gen, device="cuda:0", dtype=torch.int8)
            d = polar.encode(bits, p)
            f = polar.rate_match(d, p, 0)
            s2 = 10 ** (-SNR / 10)
            llr = 2 * ((1 - 2 * f.double()) + torch.randn(f.shape, generator=gen, device="cuda:0", dtype=torch.float64)
                       * s2 ** 0.5) / s2
            y = polar.rate_recover(llr, p, 0)
            us = dict(encode=timed(lambda: polar.encode(bits, p)), rate_match=timed(lambda: polar.rate_match(d, p, 0)),
                      rate_recover=timed(lambda: polar.rate_recover(llr, p, 0)),
                      decode=timed(lambda: polar.decode(y, p, "SCL", L)), decode_sc=timed(lambda: polar.decode(y, p, "SC")))
            _, st, _ = polar.decode(y, p, "SCL", L)
            row[f"B{nb}"] = dict(us=us, codewords_per_s={k: nb / (v * 1e-6) for k, v in us.items()},
                                 decoded_fraction=float(st.double().mean()))
        res[name] = row
        print(name, json.dumps(row[f"B{B}"]["us"]), "B=1:", json.dumps(row["B1"]["us"]))
    _save(res)


def once():
    import torch

    from python_5gtoolbox_amd import polar
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1)
    for name, K, E, nMax, iIL, crclen, L in SHAPES:
        p = polar.plan(K, E, nMax, iIL, crclen)
        bits = torch.randint(0, 2, (B, K), generator=gen, device="cuda:0", dtype=torch.int8)
        s2 = 10 ** (-SNR / 10)
        for _ in range(2):   # warm-up, then the call that counts
            f = polar.polar_tx(bits, p, E, 0)
            llr = 2 * ((1 - 2 * f.double()) + torch.randn(f.shape, generator=gen, device="cuda:0", dtype=torch.float64)
                       * s2 ** 0.5) / s2
            polar.polar_rx(llr, p, E, 0, "SCL", L)
        torch.cuda.synchronize()
    print("once: done")


def _csv(d, pattern):
    hits = sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True))
    assert hits, f"no {pattern} under {d}"
    with open(hits[0]) as f:
        return list(csv.DictReader(f))


def merge_trace(d):
    res = _load()
    rows = [r for r in _csv(d, "*kernel_stats.csv") if "polar_" in r.get("Name", "")]
    res["kernel_trace"] = dict(note="rocprofv3 --kernel-trace --stats of `polar_probe.py --once`: two calls per kernel and "
                                    "shape (three shapes, B = 4096), durations in ns", kernels=rows)
    _save(res)


def merge_counters(d):
    res = _load()
    tot = {}
    for r in _csv(d, "*counter_collection.csv"):
        m = re.search(r"polar_\w+_kernel", r["Kernel_Name"])
        if m:
            k = m.group(0)   # the decoder's three shapes are summed: the trace tells them apart only by time
            tot.setdefault(k, {}).setdefault(r["Counter_Name"], 0.0)
            tot[k][r["Counter_Name"]] += float(r["Counter_Value"])
    for c in tot.values():
        if c.get("SQ_LDS_IDX_ACTIVE"):
            c["bank_conflict_over_idx_active"] = round(c.get("SQ_LDS_BANK_CONFLICT", 0.0) / c["SQ_LDS_IDX_ACTIVE"], 4)
        if c.get("SQ_BUSY_CYCLES"):
            c["wave_cycles_over_busy_cycles"] = round(c.get("SQ_WAVE_CYCLES", 0.0) / c["SQ_BUSY_CYCLES"], 4)
    res.pop("not_measured", None)
    res["counters"] = dict(note="rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES SQ_BUSY_CYCLES of "
                                "`polar_probe.py --once`, a run of its own, summed over the calls of each kernel",
                           kernels=dict(sorted(tot.items())))
    _save(res)


def reference(root):
    sys.path.insert(0, root)
    os.chdir(root)
    from py5gphy.polar import nr_polar_decoder
    res = _load()
    ref = {}
    for name, K, E, nMax, iIL, crclen, L in SHAPES:
        N = 1 << (E - 1).bit_length() if E < 1024 else 1024
        rng = np.random.default_rng(3)
        ts = []
        for _ in range(3):
            llr = rng.normal(2.0, 2.0, N)   # the run time does not depend on the values
            t0 = time.perf_counter()
            nr_polar_decoder.nr_decode_polar("SCL", llr, E, K, L, nMax, iIL, crclen)
            ts.append(time.perf_counter() - t0)
        ref[name] = dict(seconds_per_codeword=float(np.median(ts)), N=N, L=L, note="rate-recovered input of N LLRs, one core")
        print(name, ref[name])
    res["reference_cpu"] = ref
    _save(res)


if __name__ == "__main__":
    if "--once" in sys.argv:
        once()
    elif "--trace" in sys.argv:
        merge_trace(sys.argv[sys.argv.index("--trace") + 1])
    elif "--counters" in sys.argv:
        merge_counters(sys.argv[sys.argv.index("--counters") + 1])
    elif "--reference" in sys.argv:
        reference(os.path.abspath(sys.argv[sys.argv.index("--reference") + 1]))
    else:
        gpu()
