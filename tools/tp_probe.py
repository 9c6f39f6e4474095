"""Transform precoding probe: ldpc5g_transform_precode at T = 32 slots x 12 data symbols for RBSize
270, 100, 16 and 1 (M = 3240, 1200, 192, 12), complex128 and complex64 storage, forward and
inverse, beside rocFFT on the same tensors (torch.fft.fft / ifft with norm="ortho" on the
(T*12, M) view).  Each variant is event-timed on its own: warm-ups, then interleaved steps of every
variant, each step REPS calls back to back (one launch is a few microseconds: the step time over
REPS is the per-call time with the launch gaps the stream leaves), min / median / max.  Then, at
the chain's shape (RBSize 270 of 273, 1 x 4), ldpc5g_slot_rx_frontend_tp (its LS and extraction
launches, each alone and both together) and ldpc5g_slot_map_tp, each call event-timed on its own as
in tools/slot_probe.py, and the whole sch_pusch_tp_rx_batch call beside sch_slot_rx_batch on the
same allocation without transform precoding, in one interleaved loop.

    python tools/tp_probe.py [--T 32] [--steps 20] [--warmup 3] [--out profiles/tp/probe.json]

Per-kernel times and the LDS counters come from separate runs under the profiler (one warm-up and
one call per variant):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tp -- python tools/tp_probe.py --once
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d DIR2 -o tp -- \
        python tools/tp_probe.py --once --ours-only
    python tools/tp_probe.py --kernel-stats DIR --counters DIR2      # merges them into the json

Model number written beside the times: the bytes the transform must move (every element read once
and written once) over the time, as a fraction of the 6.29 TB/s copy ceiling.
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_COPY_GBS = 6290.0
NSYM = 12
RBS = (270, 100, 16, 1)
REPS = 10
CARRIER_PRB, NR, SCS = 273, 4, 30
CE = dict(algo="DFT_symmetric", scs=SCS, eRB=4, l_left_ns=1400, l_right_ns=1200)
NOISE_VAR = 1e-3


def pusch_config(trans_precode):
    """270 PRB of a 273-PRB carrier, symbols 2..13, DMRS on [2, 11]: ten data symbols."""
    return {"nTransPrecode": trans_precode, "num_of_layers": 1, "nNrOfAntennaPorts": 1, "PortIndexList": [1000], "nPMI": 0,
            "StartSymbolIndex": 2, "NrOfSymbols": 12, "ResAlloType1": {"RBStart": 0, "RBSize": 270}, "rnti": 1, "nNid": 7,
            "DMRS": {"dmrs_TypeA_Position": "pos2", "nSCID": 0, "DMRSConfigType": 1, "NrOfDMRSSymbols": 1,
                     "NumCDMGroupsWithoutData": 2, "DMRSAddPos": 1, "PUSCHMappintType": "A",
                     "transformPrecodingDisabled": {"NID0": 7, "NID1": 7},
                     "transformPrecodingEnabled": {"nPuschID": 77, "groupOrSequenceHopping": "groupHopping"}}}


def load_json(path):
    try:
        with open(path) as f:
            return json.load(f)
    except OSError:
        return {}


def save_json(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", path)


def _find(d, pattern):
    hits = sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True))
    assert hits, f"no {pattern} under {d}"
    return hits[0]


def _kernel_key(name):
    """'tp_dft_kernel<double2, false>' from the profiler's demangled name, None for other kernels."""
    m = re.search(r"(tp_dft(?:_single)?_kernel)<(.*?)>\(", name)
    if not m:
        return None
    return m.group(1) + "<" + re.sub(r"HIP_vector_type<(\w+), 2u>", r"\g<1>2", m.group(2)).strip() + ">"


def _length_of(key, grid):
    """The transform length of a dispatch of `--once` at the default T: the single-buffer kernel
    runs M = 3240, the one-block-per-workgroup kernel M = 1200, and the packed kernel's grid tells
    M = 192 from M = 12."""
    if key.startswith("tp_dft_single"):
        return 12 * RBS[0]
    if key.endswith("false>"):
        return 12 * RBS[1]
    return {NSYM * 32 // (768 // (12 * rb)) * 256: 12 * rb for rb in RBS[2:]}.get(int(grid), 0)


def merge_profiles(stats_dir, counters_dir, out):
    """Per (kernel, transform length) the kernel times of the trace run and the two LDS counters of
    the counters-only run (both `--once` at the default T); rocFFT's kernels by name from the
    trace's statistics."""
    res = load_json(out)
    if stats_dir:
        ours, theirs = {}, {}
        with open(_find(stats_dir, "*kernel_trace.csv")) as f:
            for r in sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"])):
                k = _kernel_key(r["Kernel_Name"])
                if k:
                    k = f"{k} M={_length_of(k, r['Grid_Size_X'])}"
                    ours.setdefault(k, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        with open(_find(stats_dir, "*kernel_stats.csv")) as f:
            for r in csv.DictReader(f):
                if r.get("Name", "").startswith("fft_"):
                    theirs[r["Name"][:110]] = {"calls": int(r["Calls"]), "average_ns": round(float(r["AverageNs"]), 1),
                                               "min_ns": int(float(r["MinNs"])), "max_ns": int(float(r["MaxNs"]))}
        res["kernel_trace"] = {
            "note": "rocprofv3 --kernel-trace --stats of `tp_probe.py --once` (one warm-up and one call per variant, "
                    "forward and inverse together); ours per (kernel, transform length)",
            "ldpc5g_transform_precode": {k: {"calls": len(v), "average_ns": round(sum(v) / len(v), 1), "min_ns": min(v),
                                             "max_ns": max(v)} for k, v in sorted(ours.items())},
            "rocfft": theirs}
    if counters_dir:
        tot = {}
        with open(_find(counters_dir, "*counter_collection.csv")) as f:
            for r in sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"])):
                k = _kernel_key(r["Kernel_Name"])
                if k:
                    k = f"{k} M={_length_of(k, r['Grid_Size'])}"
                    tot.setdefault(k, {}).setdefault(r["Counter_Name"], 0.0)
                    tot[k][r["Counter_Name"]] += float(r["Counter_Value"])
        for c in tot.values():
            if c.get("SQ_LDS_IDX_ACTIVE"):
                c["bank_conflict_over_idx_active"] = round(c.get("SQ_LDS_BANK_CONFLICT", 0.0) / c["SQ_LDS_IDX_ACTIVE"], 4)
        res["lds_counters"] = {"note": "rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE of `tp_probe.py --once "
                                       "--ours-only`, summed over the calls of each (kernel, transform length)",
                               "kernels": dict(sorted(tot.items()))}
    save_json(out, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--ours-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--counters", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tp", "probe.json"))
    args = ap.parse_args()
    if args.kernel_stats or args.counters:
        return merge_profiles(args.kernel_stats, args.counters, args.out)

    import torch
    from python_5gtoolbox_amd import _lib, phy, sch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda", 0)
    T = args.T
    lib = _lib.lib()

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

    rocfft = not args.ours_only
    if rocfft:
        try:
            torch.fft.fft(torch.zeros((2, 12), dtype=torch.complex128, device=dev), norm="ortho")
            torch.cuda.synchronize()
        except Exception as e:   # noqa: BLE001 - whatever the build raises, the yardstick is dropped and said so
            rocfft = False
            print("torch.fft is not usable in this build:", e)
    res = load_json(args.out) if not args.once else {}
    res.update({"workload": f"T = {T} slots x {NSYM} data symbols, RBSize {list(RBS)} (M = 12 RBSize), forward and inverse, "
                            f"each step {REPS} calls back to back",
                "T": T, "nsym": NSYM, "steps": args.steps, "warmup": args.warmup, "reps_per_step": REPS,
                "device": torch.cuda.get_device_name(0), "hbm_copy_ceiling_GBs": HBM_COPY_GBS,
                "rocfft_yardstick": "torch.fft.fft / ifft, norm='ortho', on the (T*nsym, M) view" if rocfft else
                                    "not usable in this torch build: dropped",
                "transform": {}})
    gen = torch.Generator(device=dev)
    gen.manual_seed(3240)
    for cdt, pname in ((torch.complex128, "complex128"), (torch.complex64, "complex64")):
        rdt = torch.float64 if cdt == torch.complex128 else torch.float32
        variants, moved = {}, {}
        for rb in RBS:
            M = 12 * rb
            x = torch.complex(torch.randn((T, NSYM * M), dtype=rdt, device=dev, generator=gen),
                              torch.randn((T, NSYM * M), dtype=rdt, device=dev, generator=gen))
            out = torch.empty_like(x)
            for inv in (0, 1):
                def ours(x=x, out=out, rb=rb, inv=inv):
                    rc = lib.ldpc5g_transform_precode(_lib.ptr(x), x.stride(0), _lib.ptr(out), out.stride(0),
                                                      _lib.F32 if cdt == torch.complex64 else _lib.F64, T, NSYM, rb, inv,
                                                      _lib.stream_ptr(dev))
                    assert rc == 0, rc

                def theirs(x=x, M=M, inv=inv):
                    v = x.view(T * NSYM, M)
                    return torch.fft.ifft(v, norm="ortho") if inv else torch.fft.fft(v, norm="ortho")
                tag = f"M={M}/{'inverse' if inv else 'forward'}"
                variants[tag + "/ldpc5g_transform_precode"] = ours
                moved[tag + "/ldpc5g_transform_precode"] = 2 * x.numel() * x.element_size()
                if rocfft:
                    variants[tag + "/rocfft"] = theirs
                    moved[tag + "/rocfft"] = 2 * x.numel() * x.element_size()
                    ours()
                    err = float((out.view(T * NSYM, M) - theirs()).abs().max())
                    assert err < (1e-10 if cdt == torch.complex128 else 1e-3), (tag, err)
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
        res["transform"][pname] = line
        for k, v in line.items():
            print(pname, k, json.dumps(v), flush=True)

    # ---- the low-PAPR front end and map at the chain's shape: the entry points themselves, one call per event pair
    cfg1, cfg0 = pusch_config(1), pusch_config(0)
    re_idx = torch.from_numpy(phy.pusch_tp_data_re_idx(cfg1)[0]).to(dev)
    assert torch.equal(re_idx, phy.slot_data_re_idx_device(cfg0, dev))
    nre, Qm = re_idx.numel(), 2
    RB, S, W = 270, 2, 14 * 12 * CARRIER_PRB
    syms = (ctypes.c_int32 * 4)(2, 11)
    slots = (torch.arange(T, device=dev, dtype=torch.int32) % 20).contiguous()
    spread = torch.complex(torch.randn((T, nre), dtype=torch.float32, device=dev, generator=gen),
                           torch.randn((T, nre), dtype=torch.float32, device=dev, generator=gen))
    grid_out = torch.zeros((T, 1, W), dtype=torch.complex64, device=dev)

    def raw_map():
        rc = lib.ldpc5g_slot_map_tp(_lib.ptr(spread), spread.stride(0), _lib.ptr(re_idx), nre, _lib.ptr(slots), T, W // 14,
                                    0, RB, 1, 0, None, S, syms, 77, 1, None, _lib.ptr(grid_out), grid_out.stride(0),
                                    _lib.stream_ptr(dev))
        assert rc == 0, rc
    res["calls"] = {"note": f"T = {T}, RBSize {RB} of {CARRIER_PRB}, Nr = {NR}, port 1000, DMRS symbols [2, 11], group "
                            "hopping; ldpc5g_slot_rx_frontend_tp and ldpc5g_slot_map_tp (one antenna, identity), "
                            "each call event-timed on its own, interleaved"}
    for cdt, pname in ((torch.complex128, "complex128"), (torch.complex64, "complex64")):
        rdt = torch.float64 if cdt == torch.complex128 else torch.float32
        grid = torch.complex(torch.randn((T, NR, W), dtype=rdt, device=dev, generator=gen),
                             torch.randn((T, NR, W), dtype=rdt, device=dev, generator=gen))
        h_ls = torch.empty((T, S, 3 * RB, NR, 1), dtype=cdt, device=dev)
        y = torch.empty((T, 14 * 12 * RB, NR), dtype=cdt, device=dev)

        def raw_fe(h, yy):
            rc = lib.ldpc5g_slot_rx_frontend_tp(
                _lib.ptr(grid), grid.stride(0), _lib.F32 if cdt == torch.complex64 else _lib.F64, _lib.ptr(slots), T,
                W // 14, 0, RB, NR, 0, S, syms, 77, 1, None, _lib.ptr(h) if h is not None else None, h_ls.stride(0),
                _lib.ptr(yy) if yy is not None else None, y.stride(0), _lib.stream_ptr(dev))
            assert rc == 0, rc
        variants = {"pusch_tp_frontend/h_ls_only": lambda: raw_fe(h_ls, None),
                    "pusch_tp_frontend/y_only": lambda: raw_fe(None, y),
                    "pusch_tp_frontend/both": lambda: raw_fe(h_ls, y)}
        if cdt == torch.complex64:
            variants["pusch_tp_map"] = raw_map
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
                times[k].append(ev(fn))
        res["calls"][pname] = {k: stats(v) for k, v in times.items()}
        print(pname, "calls", json.dumps(res["calls"][pname]), flush=True)
        del grid, h_ls, y
    if args.once:
        return

    # ---- the chain: RBSize 270, 1 x 4, with and without transform precoding
    G = nre * Qm
    A = 19464
    scfg = sch.sch_config(A, Qm, 308, 1, 0, 0, G)
    tb = torch.randint(0, 2, (T, A), dtype=torch.int8, device=dev, generator=gen)
    cinit = torch.arange(T, device=dev, dtype=torch.int64) * 2 ** 15 + 7
    words = phy.prbs_words(cinit, G)
    x = phy.scramble_modulate(sch.sch_encode_batch(tb, scfg).contiguous(), Qm, words=words)
    rng = np.random.default_rng(270)
    H = torch.tensor((rng.standard_normal((T, NR, 1)) + 1j * rng.standard_normal((T, NR, 1))) / np.sqrt(2)).to(dev)
    res["chain"] = {}
    for cdt, pname in ((torch.complex128, "complex128"), (torch.complex64, "complex64")):
        grids = {}
        for name, tx in (("tp", phy.pusch_tp_map(x, slots, cfg1, CARRIER_PRB, 1, re_idx=re_idx)),
                         ("plain", phy.slot_map(x, slots, cfg0, CARRIER_PRB, 1, re_idx=re_idx))):
            rx = H @ tx.to(torch.complex128)
            rx += torch.complex(torch.randn(rx.shape, dtype=torch.float64, device=dev, generator=gen),
                                torch.randn(rx.shape, dtype=torch.float64, device=dev, generator=gen)) * (NOISE_VAR / 2) ** 0.5
            grids[name] = rx.to(cdt)
        sched, dnt = ("flooding", torch.float64) if cdt == torch.complex128 else ("layered", torch.float32)
        ws = sch.SchWorkspace(scfg, T, dev)
        kw = dict(alpha=0.75, beta=0.0, schedule=sched, words=words, dn_dtype=dnt, ws=ws)

        def with_tp():
            return sch.sch_pusch_tp_rx_batch(grids["tp"], slots, cfg1, CE, "MMSE", Qm, scfg, 8, re_idx=re_idx, **kw)

        def without():
            return sch.sch_slot_rx_batch(grids["plain"], slots, cfg0, CE, "MMSE", Qm, scfg, 8, re_idx=re_idx, **kw)
        ok_tp = float(with_tp().tb_ok.float().mean())
        ok_plain = float(without().tb_ok.float().mean())
        for _ in range(args.warmup):
            with_tp(), without()
        t_a, t_b = [], []
        for _ in range(args.steps):
            t_a.append(ev(with_tp))
            t_b.append(ev(without))
        res["chain"][pname] = {"shape": f"T = {T}, RBSize 270 of {CARRIER_PRB}, 1 x {NR}, QPSK, A = {A}, G = {G}, MMSE, "
                                        f"min-sum L = 8, noise variance {NOISE_VAR}", "schedule": sched,
                               "tb_ok_rate_with_transform_precoding": ok_tp, "tb_ok_rate_without": ok_plain,
                               "sch_pusch_tp_rx_batch": stats(t_a), "sch_slot_rx_batch_without_transform_precoding": stats(t_b),
                               "median_difference_ms": round(statistics.median(t_a) - statistics.median(t_b), 5)}
        print(pname, "chain", json.dumps(res["chain"][pname]), flush=True)
        del grids, ws
        torch.cuda.empty_cache()
    save_json(args.out, res)


if __name__ == "__main__":
    main()
