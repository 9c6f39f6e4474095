"""OFDM low-PHY probe: ldpc5g_ofdm_demod / ldpc5g_ofdm_mod at T = 32 slots x Nr = 4 antennas for the
273-PRB carrier (nfft 4096) and the 24-PRB carrier (nfft 512), 30 kHz, carrier 3840 MHz, complex128
and complex64 storage, beside the same operation composed from torch on the same tensors (window
gather, phase scalar, torch.fft.fft(norm="ortho"), fftshift, ramp, slice; and the reverse).  Each
variant is event-timed on its own: warm-ups, then interleaved steps of every variant, each step
REPS calls back to back, min / median / max.  Then the whole sch_td_rx_batch call beside
sch_slot_rx_batch on the same slots already demodulated, in one interleaved loop: what the stage
adds to the chain.

    python tools/ofdm_probe.py [--T 32] [--steps 20] [--warmup 3] [--out profiles/ofdm/probe.json]

The LDS counters come from a separate, counters-only run under the profiler (one warm-up and one
call per variant):

    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d DIR -o ofdm -- \
        python tools/ofdm_probe.py --once
    python tools/ofdm_probe.py --counters DIR      # merges them into the json

Model number written beside the times: the bytes that must move (td read or written once, the
grid written or read once) over the time, as a fraction of the 6.29 TB/s copy ceiling.
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tp_probe import CE, HBM_COPY_GBS, NOISE_VAR, _find, load_json, pusch_config, save_json  # noqa: E402

REPS = 10
NR, SCS, MHZ = 4, 30, 3840
CARRIERS = ((273, 100), (24, 10))   # (PRBs, BW in MHz)


def merge_counters(counters_dir, out):
    res = load_json(out)
    tot = {}
    with open(_find(counters_dir, "*counter_collection.csv")) as f:
        for r in sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"])):
            m = re.search(r"ofdm_kernel<(.*?)>\(", r["Kernel_Name"])
            if m:
                k = "ofdm_kernel<" + re.sub(r"HIP_vector_type<(\w+), 2u>", r"\g<1>2", m.group(1)).strip() + ">"
                tot.setdefault(k, {}).setdefault(r["Counter_Name"], 0.0)
                tot[k][r["Counter_Name"]] += float(r["Counter_Value"])
    for c in tot.values():
        if c.get("SQ_LDS_IDX_ACTIVE"):
            c["bank_conflict_over_idx_active"] = round(c.get("SQ_LDS_BANK_CONFLICT", 0.0) / c["SQ_LDS_IDX_ACTIVE"], 4)
    res["lds_counters"] = {"note": "rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE of `ofdm_probe.py --once`, summed "
                                   "over the calls of each kernel <storage, demodulation, nfft>",
                           "kernels": dict(sorted(tot.items()))}
    save_json(out, res)


def torch_composition(torch, phy, prbs, dev, cdt):
    """(demod, mod) composed from torch ops, constants built once."""
    nfft, cps, S = phy.ofdm_params(SCS, prbs)
    cre, h, fs, hz = 12 * prbs, cps[1] // 2, nfft * SCS * 1000, MHZ * 10 ** 6
    lo = (nfft - cre) // 2
    starts = np.cumsum([0] + [c + nfft for c in cps[:-1]]) + np.array(cps)    # first useful sample of each symbol
    win = torch.tensor((starts - h)[:, None] + np.arange(nfft)[None], device=dev)
    ph = np.array([((hz * int(n)) % fs) / fs for n in starts])
    rot = torch.tensor(np.exp(2j * np.pi * ph)[:, None], device=dev).to(cdt)
    ramp = torch.tensor(np.exp(2j * np.pi * ((h * np.arange(nfft)) % nfft) / nfft), device=dev).to(cdt)
    back = np.concatenate([s * nfft + (np.arange(-c, nfft) % nfft) for s, c in enumerate(cps)])
    back = torch.tensor(back, device=dev)

    def demod(td):
        x = td[..., win] * rot
        f = torch.fft.fftshift(torch.fft.fft(x, norm="ortho"), dim=-1) * ramp
        return f[..., lo:lo + cre].reshape(td.shape[0], td.shape[1], 14 * cre)

    def mod(grid):
        a = torch.zeros(grid.shape[:2] + (14, nfft), dtype=grid.dtype, device=dev)
        a[..., lo:lo + cre] = grid.view(grid.shape[0], grid.shape[1], 14, cre)
        x = torch.fft.ifft(torch.fft.ifftshift(a, dim=-1), norm="ortho") * rot.conj()
        return x.flatten(-2)[..., back]
    return demod, mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--counters", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ofdm", "probe.json"))
    args = ap.parse_args()
    if args.counters:
        return merge_counters(args.counters, args.out)

    import torch
    from python_5gtoolbox_amd import phy, sch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda", 0)
    T = args.T

    def ev(fn, reps=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def stats(ms):
        return {"min_ms": round(min(ms), 5), "median_ms": round(statistics.median(ms), 5), "max_ms": round(max(ms), 5)}

    res = {} if args.once else load_json(args.out)
    res.update({"workload": f"T = {T} slots x Nr = {NR}, scs {SCS} kHz, carrier {MHZ} MHz, carriers {[c[0] for c in CARRIERS]} PRB, "
                            f"each step {REPS} calls back to back",
                "T": T, "Nr": NR, "steps": args.steps, "warmup": args.warmup, "reps_per_step": REPS,
                "device": torch.cuda.get_device_name(0), "hbm_copy_ceiling_GBs": HBM_COPY_GBS,
                "torch_yardstick": "window gather, phase scalar, torch.fft.fft(norm='ortho'), fftshift, ramp, slice (and the "
                                   "reverse) on the same tensors, constants built once",
                "stage": {}})
    gen = torch.Generator(device=dev)
    gen.manual_seed(4096)
    for cdt, pname in ((torch.complex128, "complex128"), (torch.complex64, "complex64")):
        rdt = torch.float64 if cdt == torch.complex128 else torch.float32
        variants, moved = {}, {}
        for prbs, _ in CARRIERS:
            nfft, _, S = phy.ofdm_params(SCS, prbs)
            W = 14 * 12 * prbs
            td = torch.complex(torch.randn((T, NR, S), dtype=rdt, device=dev, generator=gen),
                               torch.randn((T, NR, S), dtype=rdt, device=dev, generator=gen))
            grid = torch.complex(torch.randn((T, NR, W), dtype=rdt, device=dev, generator=gen),
                                 torch.randn((T, NR, W), dtype=rdt, device=dev, generator=gen))
            otd, ogrid = torch.empty_like(td), torch.empty_like(grid)
            t_demod, t_mod = torch_composition(torch, phy, prbs, dev, cdt)
            nbytes = (td.numel() + grid.numel()) * td.element_size()
            tol = 1e-10 if cdt == torch.complex128 else 1e-3
            assert float((phy.ofdm_demod(td, SCS, prbs, MHZ) - t_demod(td)).abs().max()) < tol
            assert float((phy.ofdm_mod(grid, SCS, prbs, MHZ) - t_mod(grid)).abs().max()) < tol
            for tag, ours, theirs in (
                    (f"nfft={nfft}/demod", lambda td=td, o=ogrid, p=prbs: phy.ofdm_demod(td, SCS, p, MHZ, out=o),
                     lambda td=td, f=t_demod: f(td)),
                    (f"nfft={nfft}/mod", lambda g=grid, o=otd, p=prbs: phy.ofdm_mod(g, SCS, p, MHZ, out=o),
                     lambda g=grid, f=t_mod: f(g))):
                variants[tag + "/ldpc5g_ofdm"] = ours
                moved[tag + "/ldpc5g_ofdm"] = nbytes
                if not args.once:
                    variants[tag + "/torch"] = theirs
                    moved[tag + "/torch"] = nbytes
        for _ in range(1 if args.once else args.warmup):
            for fn in variants.values():
                fn()
        if args.once:
            for fn in variants.values():
                fn()
            torch.cuda.synchronize()
            continue
        times = {k: [] for k in variants}
        for _ in range(args.steps):   # interleaved: every variant once per step
            for k, fn in variants.items():
                times[k].append(ev(fn, REPS))
        line = {}
        for k in variants:
            st = stats(times[k])
            line[k] = dict(st, bytes=moved[k], fraction_of_copy_ceiling_at_median=round(
                moved[k] / (st["median_ms"] * 1e-3) / (HBM_COPY_GBS * 1e9), 4))
        res["stage"][pname] = line
        for k, v in line.items():
            print(pname, k, json.dumps(v), flush=True)
        del variants
        torch.cuda.empty_cache()
    if args.once:
        return

    # ---- the chain: 270 PRB of the 273-PRB carrier, 1 x 4, from samples and from the grid
    prbs, bw = CARRIERS[0]
    cfg = pusch_config(0)
    carrier = {"scs": SCS, "BW": bw, "carrier_frequency_in_mhz": MHZ}
    re_idx = phy.slot_data_re_idx_device(cfg, dev)
    nre, Qm = re_idx.numel(), 2
    G = nre * Qm
    A = 19464
    scfg = sch.sch_config(A, Qm, 308, 1, 0, 0, G)
    tb = torch.randint(0, 2, (T, A), dtype=torch.int8, device=dev, generator=gen)
    cinit = torch.arange(T, device=dev, dtype=torch.int64) * 2 ** 15 + 7
    words = phy.prbs_words(cinit, G)
    slots = (torch.arange(T, device=dev, dtype=torch.int32) % 20).contiguous()
    x = phy.scramble_modulate(sch.sch_encode_batch(tb, scfg).contiguous(), Qm, words=words)
    tx = phy.ofdm_mod(phy.slot_map(x, slots, cfg, prbs, 1, re_idx=re_idx).to(torch.complex128), SCS, prbs, MHZ)
    rng = np.random.default_rng(273)
    H = torch.tensor((rng.standard_normal((T, NR, 1)) + 1j * rng.standard_normal((T, NR, 1))) / np.sqrt(2)).to(dev)
    rx = H @ tx
    rx += torch.complex(torch.randn(rx.shape, dtype=torch.float64, device=dev, generator=gen),
                        torch.randn(rx.shape, dtype=torch.float64, device=dev, generator=gen)) * (NOISE_VAR / 2) ** 0.5
    res["chain"] = {}
    for cdt, pname in ((torch.complex128, "complex128"), (torch.complex64, "complex64")):
        td = rx.to(cdt)
        grid = phy.ofdm_demod(td, SCS, prbs, MHZ)
        sched, dnt = ("flooding", torch.float64) if cdt == torch.complex128 else ("layered", torch.float32)
        ws = sch.SchWorkspace(scfg, T, dev)
        kw = dict(alpha=0.75, beta=0.0, schedule=sched, words=words, dn_dtype=dnt, ws=ws, re_idx=re_idx)

        def from_td():
            return sch.sch_td_rx_batch(td, slots, cfg, carrier, CE, "MMSE", Qm, scfg, 8, **kw)

        def from_grid():
            return sch.sch_slot_rx_batch(grid, slots, cfg, CE, "MMSE", Qm, scfg, 8, **kw)
        ok_td = float(from_td().tb_ok.float().mean())
        ok_grid = float(from_grid().tb_ok.float().mean())
        for _ in range(args.warmup):
            from_td(), from_grid()
        t_a, t_b = [], []
        for _ in range(args.steps):
            t_a.append(ev(from_td))
            t_b.append(ev(from_grid))
        res["chain"][pname] = {"shape": f"T = {T}, RBSize 270 of {prbs}, 1 x {NR}, QPSK, A = {A}, G = {G}, MMSE, min-sum L = 8, "
                                        f"noise variance {NOISE_VAR} per sample", "schedule": sched,
                               "tb_ok_rate_from_samples": ok_td, "tb_ok_rate_from_grid": ok_grid,
                               "sch_td_rx_batch": stats(t_a), "sch_slot_rx_batch_on_the_demodulated_grid": stats(t_b),
                               "median_difference_ms": round(statistics.median(t_a) - statistics.median(t_b), 5)}
        print(pname, "chain", json.dumps(res["chain"][pname]), flush=True)
        del ws
        torch.cuda.empty_cache()
    save_json(args.out, res)


if __name__ == "__main__":
    main()
