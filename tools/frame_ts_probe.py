"""Per-workgroup phase timing of the float64 frame kernel (dev tool): run with
LDPC5G_LIB=build/alt/frame_ts.so (tools/ab/make_variants.py frame_ts), whose workgroups write 9
real-time clock stamps (100 MHz) and their HW_ID / XCC_ID registers into the first 88 bytes of
their ck row; the frame_ts_fused build adds two stamps inside BG1's fused start in the 16 bytes
behind.  Prints the split and writes it as JSON.

    LDPC5G_LIB=build/alt/frame_ts.so python tools/frame_ts_probe.py [B] [L] [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from python_5gtoolbox_amd import nr_ldpc_decode as D, nr_ldpc_encode as E  # noqa: E402

NAMES = ["prologue", "iteration 0 (peeled)", "iteration 1", "iteration 2", "iterations 3..L-1",
         "final: ext decisions", "final: syndrome + barrier", "ck store"]


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    dst = sys.argv[3] if len(sys.argv) > 3 else None
    Zc, K, NF = 384, 22 * 384, 68 * 384
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    ck = torch.randint(0, 2, (B, K), dtype=torch.int8, device="cuda", generator=g)
    dn = E.encode_ldpc_batch(ck, 1)
    sigma = 10 ** (3 / 20)   # -3 dB: every codeblock runs all L iterations
    llr = (2 * ((1 - 2 * dn.float()) + sigma * torch.randn(dn.shape, device="cuda", generator=g)) / sigma ** 2).double()
    out = (torch.empty((B, NF), dtype=torch.int8, device="cuda"), torch.empty((B,), dtype=torch.uint8, device="cuda"),
           torch.empty((B,), dtype=torch.int32, device="cuda"))
    for _ in range(3):
        D.nr_decode_ldpc_batch(llr, Zc, 1, L, "min-sum", 0.75, 0.0, "flooding", out=out)
    torch.cuda.synchronize()
    assert int(out[2].min()) == L, "a codeblock left the loop early: the split assumes L iterations"
    raw = out[0][:, :104].contiguous().cpu().numpy().view(np.uint64).astype(np.int64)   # [B, 13]
    ts = raw[:, :9]
    # the fused start's inner stamps (a build without them leaves decoded bits there)
    inner = raw[:, 11:13]
    fused = bool(((ts[:, 1] <= inner[:, 0]) & (inner[:, 0] <= inner[:, 1]) & (inner[:, 1] <= ts[:, 2])).all())
    cu = ((raw[:, 9] >> 8) & 0xff) | ((raw[:, 10] & 0xf) << 8)   # CU / SH / SE bits of HW_ID, XCC
    d = np.diff(ts, axis=1) * 10e-3   # us
    life = (ts[:, 8] - ts[:, 0]) * 10e-3
    span = (ts[:, 8].max() - ts[:, 0].min()) * 10e-3
    gaps = []
    for c in np.unique(cu):
        w = ts[cu == c]
        w = w[np.argsort(w[:, 0])]
        gaps.extend(((w[1:, 0] - w[:-1, 8]) * 10e-3).tolist())
    gaps = np.array(gaps) if gaps else np.zeros(1)
    res = {"B": B, "L": L, "workgroups": int(len(ts)), "cus_seen": int(len(np.unique(cu))), "launch_span_us": round(span, 2),
           "wg_life_us_mean": round(float(life.mean()), 3), "phases_us": {},
           "gap_between_wgs_on_a_cu_us": {"mean": round(float(gaps.mean()), 3), "median": round(float(np.median(gaps)), 3),
                                          "min": round(float(gaps.min()), 3), "max": round(float(gaps.max()), 3)}}
    print(f"frame kernel B={B} L={L}: {len(ts)} workgroups on {res['cus_seen']} CUs, launch span {span:.1f} us, "
          f"per-WG life mean {life.mean():.2f} us")
    for k, n in enumerate(NAMES):
        res["phases_us"][n] = {"mean": round(float(d[:, k].mean()), 3), "median": round(float(np.median(d[:, k])), 3),
                               "min": round(float(d[:, k].min()), 3), "max": round(float(d[:, k].max()), 3)}
        print(f"  {n:26s} mean {d[:, k].mean():8.2f} us  median {np.median(d[:, k]):8.2f}  min {d[:, k].min():8.2f}  max {d[:, k].max():8.2f}")
    print(f"  {'gap to the CU next WG':26s} mean {gaps.mean():8.2f} us  median {np.median(gaps):8.2f}  min {gaps.min():8.2f}  max {gaps.max():8.2f}")
    # BG1's fused start: "iteration 0 (peeled)" is iteration 0 with iteration 1's phase A, and
    # "iteration 1" its phase B alone, so the fixed-cost formula of the peeled iteration has no meaning
    res["fused_start"] = bool(d[:, 2].mean() < 0.75 * d[:, 3].mean())
    if fused:
        parts = np.stack([inner[:, 0] - ts[:, 1], inner[:, 1] - inner[:, 0], ts[:, 2] - inner[:, 1]], axis=1) * 10e-3
        res["fused_start_us"] = {}
        for k, n in enumerate(["pass + barrier", "iteration 0's column sums + barrier", "combine"]):
            res["fused_start_us"][n] = round(float(parts[:, k].mean()), 3)
            print(f"    fused start: {n:36s} mean {parts[:, k].mean():8.2f} us")
    elif not res["fused_start"]:
        steady = float(d[:, 3].mean())
        fixed = float(d[:, 0].mean() + (d[:, 1].mean() - 0.28 * steady) + d[:, 5].mean() + d[:, 6].mean() + d[:, 7].mean() + gaps.mean())
        res["fixed_cost_us"] = round(fixed, 3)
        res["fixed_cost_share_of_life_plus_gap"] = round(fixed / float(life.mean() + gaps.mean()), 4)
        print(f"  fixed cost (prologue + it0 - 0.28 steady + final + ck + gap) = {fixed:.2f} us = "
              f"{100 * res['fixed_cost_share_of_life_plus_gap']:.1f} % of life + gap")
    if dst:
        os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
        with open(dst, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
