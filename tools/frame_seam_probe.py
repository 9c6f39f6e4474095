"""Per-wave timing of the seam between two iterations of the float64 frame kernel (dev tool): run
with LDPC5G_LIB=build/alt/frame_seam_ts.so (tools/ab/make_variants.py frame_seam_ts), whose waves
write 8 real-time clock stamps (100 MHz) of iterations 4 and 5 into the first 768 bytes of their
workgroup's ck row, [wave][8] (the stamp points: make_variants.py).  Prints the split and writes
it as JSON.  Waves 0-5 are half 0, waves 6-11 half 1.

    LDPC5G_LIB=build/alt/frame_seam_ts.so python tools/frame_seam_probe.py [B] [L] [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from python_5gtoolbox_amd import nr_ldpc_decode as D, nr_ldpc_encode as E  # noqa: E402

SEG = ["phase A (cold start back -> last row)", "barrier + flag test", "lf / hand-offs + group 0 + barrier",
       "groups 1.. + barriers", "LQ update", "flag reset + closing barrier", "cold start (loads -> first edge ready)"]
NW, NS = 12, 8


def _st(x):
    return {"mean": round(float(x.mean()), 3), "median": round(float(np.median(x)), 3),
            "p10": round(float(np.percentile(x, 10)), 3), "p90": round(float(np.percentile(x, 90)), 3)}


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    dst = sys.argv[3] if len(sys.argv) > 3 else None
    assert L >= 6, "the stamps are taken in iterations 4 and 5"
    Zc, K, NF = 384, 22 * 384, 68 * 384
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    ck = torch.randint(0, 2, (B, K), dtype=torch.int8, device="cuda", generator=g)
    dn = E.encode_ldpc_batch(ck, 1)
    sigma = 10 ** (3 / 20)   # -3 dB: every codeblock runs all L iterations
    llr = (2 * ((1 - 2 * dn.float()) + sigma * torch.randn(dn.shape, device="cuda", generator=g)) / sigma ** 2).double()
    out = (torch.zeros((B, NF), dtype=torch.int8, device="cuda"), torch.empty((B,), dtype=torch.uint8, device="cuda"),
           torch.empty((B,), dtype=torch.int32, device="cuda"))
    for _ in range(3):
        D.nr_decode_ldpc_batch(llr, Zc, 1, L, "min-sum", 0.75, 0.0, "flooding", out=out)
    torch.cuda.synchronize()
    assert int(out[2].min()) == L, "a codeblock left the loop early: the split assumes L iterations"
    ts = out[0][:, :NW * NS * 8].contiguous().cpu().numpy().view(np.uint64).astype(np.int64).reshape(B, NW, NS)
    assert (ts > 0).all() and (np.diff(ts, axis=2) >= 0).all(), "not a frame_seam_ts library (no stamps)"
    us = 10e-3
    seg = np.diff(ts, axis=2) * us                      # [B, wave, 7] per wave
    # workgroup view: a point is passed when its last wave passes it
    wg = ts.max(axis=1)
    wseg = np.diff(wg, axis=1) * us
    res = {"B": B, "L": L, "iteration_us": _st((ts[:, :, 7] - ts[:, :, 0]).mean(axis=1) * us),
           "segments_us_per_wave_mean": {}, "segments_us_last_wave": {}, "per_wave": {}}
    print(f"frame seam B={B} L={L}: iteration (stamp 0 -> 7) {res['iteration_us']['mean']:.2f} us")
    for k, n in enumerate(SEG):
        res["segments_us_per_wave_mean"][n] = _st(seg[:, :, k].mean(axis=1))
        res["segments_us_last_wave"][n] = _st(wseg[:, k])
        print(f"  {k}->{k + 1} {n:40s} wave mean {seg[:, :, k].mean():7.3f} us   last wave to last wave {wseg[:, k].mean():7.3f}")
    seam = seg[:, :, 1] + seg[:, :, 4] + seg[:, :, 5] + seg[:, :, 6]
    res["seam_us_excl_group0_block"] = _st(seam.mean(axis=1))
    res["seam_plus_group0_block_us"] = _st((seam + seg[:, :, 2]).mean(axis=1))
    print(f"  seam (1->2, 4->7) {seam.mean():.3f} us; with 2->3 (lf issue, hand-offs, group 0 and its barrier) "
          f"{(seam + seg[:, :, 2]).mean():.3f} us")
    # arrival skew at phase A's barrier: each wave's stamp 1 behind its workgroup's first
    arr = (ts[:, :, 1] - ts[:, :, 1].min(axis=1, keepdims=True)) * us
    half = np.stack([ts[:, :6, 1].max(axis=1), ts[:, 6:, 1].max(axis=1)], axis=1)
    res["phaseA_end_skew_us"] = {"last_minus_first_wave": _st(arr.max(axis=1)),
                                 "half1_last_minus_half0_last": _st((half[:, 1] - half[:, 0]) * us),
                                 "per_wave_behind_first_mean": [round(float(v), 3) for v in arr.mean(axis=0)]}
    print(f"  phase A end: last wave - first wave {arr.max(axis=1).mean():.3f} us; half 1's last - half 0's last "
          f"{((half[:, 1] - half[:, 0]) * us).mean():+.3f} us")
    for w in range(NW):
        res["per_wave"][str(w)] = [round(float(v), 3) for v in seg[:, w, :].mean(axis=0)]
        print(f"    wave {w:2d} (half {w // 6}): " + " ".join(f"{v:7.3f}" for v in seg[:, w, :].mean(axis=0))
              + f"   behind first at A's end {arr[:, w].mean():.3f}")
    if dst:
        os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
        with open(dst, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
