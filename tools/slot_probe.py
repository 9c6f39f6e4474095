"""Slot front end probe: ldpc5g_slot_rx_frontend (its LS and extraction launches, each alone and
both together) and ldpc5g_slot_map at BASELINE config 5's slot shape (T = 32 slots, 273 PRB,
Nr = Nt = 4, DMRS symbols [2, 11], scs 30 kHz), complex128 and complex64 grids, each call
event-timed on its own: warm-ups, then interleaved steps of every variant, min / median / max.
Then the whole sch_slot_rx_batch call beside sch_ce_eq_rx_batch fed with precomputed y and H_LS, in
one interleaved loop.

    python tools/slot_probe.py [--T 32] [--steps 20] [--warmup 3] [--out profiles/slot/probe.json]

Event times of single launches include the launch itself; per-kernel times come from a separate run
under the profiler (one warm-up and one call per variant; counters, if wanted, go in yet another
run):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o slot -- python tools/slot_probe.py --once
    python tools/slot_probe.py --kernel-stats DIR/slot_kernel_stats.csv      # merges them into the json

Model numbers written beside the times: the bytes each kernel must move (LS: the twelve REs per
PRB of the S DMRS symbols of every antenna read, h_ls written; extraction: the allocation read and
written once; map: symbols and indices read, data and DMRS REs of every antenna written) and the
fraction of the 6.29 TB/s copy ceiling that bytes / time comes to.
"""
import argparse
import csv
import ctypes
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_COPY_GBS = 6290.0
PRB, NR, NT, SCS, SYM = 273, 4, 4, 30, [2, 11]
N = 3 * PRB
NOISE_VAR = 1e-4   # 40 dB: with the channel estimated from the DMRS, config 5's 256QAM blocks need more than
                   # the 30 dB at which tools/ce_probe.py decodes them with the channel known
CE = dict(algo="DFT_symmetric", scs=SCS, eRB=4, l_left_ns=1400, l_right_ns=1200)


def pdsch_config():
    """Symbols 1..13 of the slot, DMRS on [2, 11], two CDM groups: the 11 data symbols of config 5."""
    return {"num_of_layers": NT, "PortIndexList": [1000, 1001, 1002, 1003], "StartSymbolIndex": 1, "NrOfSymbols": 13,
            "ResAlloType1": {"RBStart": 0, "RBSize": PRB}, "rnti": 1, "nID": 7,
            "DMRS": {"DMRSReferencePoint": "CRB0", "nSCID": 0, "nNIDnSCID": 7, "DMRSConfigType": 1,
                     "NrOfDMRSSymbols": 1, "NumCDMGroupsWithoutData": 2, "DMRSAddPos": 1, "PDSCHMappintType": "A"}}


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


def kernel_bytes(T, es, nre):
    """Bytes each kernel must move at this shape (es: bytes per grid element)."""
    S = len(SYM)
    return {"slot_ls_kernel": T * S * (12 * PRB * NR + N * NR * NT) * es,
            "slot_extract_kernel": T * 14 * 12 * PRB * NR * es * 2,
            "slot_map_kernel": T * (nre * NT * 8 + nre * 4 + (nre + S * 12 * PRB) * NT * 8)}


def merge_kernel_stats(path, out):
    res = load_json(out)
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            m = re.search(r"(slot_\w+_kernel)<(.*?)>\(", r.get("Name", ""))
            if m:
                targs = m.group(2).replace("HIP_vector_type<", "").replace(", 2u>", "2").strip()
                rows[f"{m.group(1)}<{targs}>"] = {
                    "calls": int(r["Calls"]), "average_ns": round(float(r["AverageNs"]), 1),
                    "min_ns": int(float(r["MinNs"])), "max_ns": int(float(r["MaxNs"]))}
    T = res.get("T", 32)
    nre = res.get("nre", 11 * 12 * PRB)
    for key, row in rows.items():
        es = 16 if "double2" in key else 8
        b = kernel_bytes(T, es, nre)[key.split("<")[0]]
        row["bytes"] = b
        row["fraction_of_copy_ceiling_at_min"] = round(b / (row["min_ns"] * 1e-9) / (HBM_COPY_GBS * 1e9), 3)
    res["kernel_trace"] = {"note": "rocprofv3 --kernel-trace --stats of `slot_probe.py --once` (one warm-up and the "
                                   "calls of one pass per storage type)", "kernels": rows}
    save_json(out, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slot", "probe.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.kernel_stats, args.out)

    import torch
    import bench
    from python_5gtoolbox_amd import _lib, phy, sch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda", 0)
    T, S = args.T, len(SYM)
    cfg = pdsch_config()
    lib = _lib.lib()

    def ev(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def stats(ms):
        return {"min_ms": round(min(ms), 5), "median_ms": round(statistics.median(ms), 5), "max_ms": round(max(ms), 5)}

    # the transmitted slots: config 5's transport blocks mapped into the grid, then a channel
    A, Qm, Rate, nl, rv, G = (bench.C5[k] for k in ("A", "Qm", "R", "NL", "rv", "G"))
    re_idx = phy.slot_data_re_idx_device(cfg, dev)
    nre = re_idx.numel()
    assert nl == NT and G == nre * NT * Qm, (nl, G, nre)
    scfg = sch.sch_config(A, Qm, Rate, NT, rv, A, G)
    gen = torch.Generator(device=dev)
    gen.manual_seed(36036)
    tb = torch.randint(0, 2, (T, A), dtype=torch.int8, device=dev, generator=gen)
    cinit = torch.arange(T, device=dev, dtype=torch.int64) * 2 ** 15 + 7
    words = phy.prbs_words(cinit, G)
    slots = (torch.arange(T, device=dev, dtype=torch.int32) % 20).contiguous()
    x = phy.scramble_modulate(sch.sch_encode_batch(tb, scfg).contiguous(), Qm, words=words)
    tx = phy.slot_map(x, slots, cfg, PRB, NT, re_idx=re_idx)
    rng = np.random.default_rng(273)   # H = I + 0.2 CN(0, 1)-sized entries, flat per slot (as tools/eq_probe.py)
    H = np.eye(NR, NT)[None] + 0.2 * (rng.standard_normal((T, NR, NT)) + 1j * rng.standard_normal((T, NR, NT))) / np.sqrt(2)
    rx128 = torch.tensor(H).to(dev) @ tx.to(torch.complex128)
    rx128 += torch.complex(torch.randn(rx128.shape, dtype=torch.float64, device=dev, generator=gen),
                           torch.randn(rx128.shape, dtype=torch.float64, device=dev, generator=gen)) * (NOISE_VAR / 2) ** 0.5
    ports = (ctypes.c_int32 * 4)(0, 1, 2, 3)
    syms = (ctypes.c_int32 * 4)(*SYM)
    res = load_json(args.out) if not args.once else {}
    res.update({"workload": f"BASELINE config 5 slot shape: T = {T} slots x {PRB} PRB, Nr = Nt = 4, DMRS symbols {SYM}, "
                            f"two CDM groups, symbols 1..13 allocated, scs {SCS} kHz; chain: H = I + 0.2 CN(0, 1) flat per slot, "
                            f"noise variance {NOISE_VAR}",
                "T": T, "nre": nre, "steps": args.steps, "warmup": args.warmup,
                "device": torch.cuda.get_device_name(0), "hbm_copy_ceiling_GBs": HBM_COPY_GBS,
                "launches": {"slot_frontend": 2, "slot_frontend_one_output": 1, "slot_map": 1},
                "calls": {}, "chain": {}})
    grid_out = torch.zeros_like(tx)

    def raw_map():
        rc = lib.ldpc5g_slot_map(_lib.ptr(x), x.stride(0), _lib.ptr(re_idx), nre, _lib.ptr(slots), T, 12 * PRB, 0, PRB,
                                 NT, NT, None, S, syms, 7, 0, 2, _lib.ptr(grid_out), grid_out.stride(0),
                                 _lib.stream_ptr(dev))
        assert rc == 0, rc

    for pname, cdt in (("complex128", torch.complex128), ("complex64", torch.complex64)):
        grid = rx128.to(cdt)
        es = grid.element_size()
        h_ls = torch.empty((T, S, N, NR, NT), dtype=cdt, device=dev)
        y = torch.empty((T, 14 * 12 * PRB, NR), dtype=cdt, device=dev)

        def raw_fe(h, yy):
            rc = lib.ldpc5g_slot_rx_frontend(
                _lib.ptr(grid), grid.stride(0), _lib.F32 if cdt == torch.complex64 else _lib.F64, _lib.ptr(slots), T,
                12 * PRB, 0, PRB, NR, NT, ports, S, syms, 7, 0, 2, _lib.ptr(h) if h is not None else None,
                h_ls.stride(0), _lib.ptr(yy) if yy is not None else None, y.stride(0), _lib.stream_ptr(dev))
            assert rc == 0, rc
        variants = {"slot_rx_frontend/h_ls_only": lambda: raw_fe(h_ls, None),
                    "slot_rx_frontend/y_only": lambda: raw_fe(None, y),
                    "slot_rx_frontend/both": lambda: raw_fe(h_ls, y)}
        if cdt == torch.complex64:
            variants["slot_map"] = raw_map
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
        kb = kernel_bytes(T, es, nre)
        moved = {"slot_rx_frontend/h_ls_only": kb["slot_ls_kernel"], "slot_rx_frontend/y_only": kb["slot_extract_kernel"],
                 "slot_rx_frontend/both": kb["slot_ls_kernel"] + kb["slot_extract_kernel"], "slot_map": kb["slot_map_kernel"]}
        line = {}
        for k in variants:
            st = stats(times[k])
            line[k] = dict(st, bytes=moved[k], event_timed_fraction_of_copy_ceiling_at_median=round(
                moved[k] / (st["median_ms"] * 1e-3) / (HBM_COPY_GBS * 1e9), 3))
        res["calls"][pname] = line
        print(pname, json.dumps(line), flush=True)

        # the whole receiver from the grid beside the same receiver fed with precomputed y and H_LS
        sched, dnt = ("flooding", torch.float64) if cdt == torch.complex128 else ("layered", torch.float32)
        ws = sch.SchWorkspace(scfg, T, dev)
        kw = dict(alpha=0.75, beta=0.0, schedule=sched, words=words, dn_dtype=dnt, ws=ws)
        ce2 = dict(CE, sym_map=SYM, num_cdm_groups=2)

        def from_grid():
            return sch.sch_slot_rx_batch(grid, slots, cfg, CE, "MMSE", Qm, scfg, 8, re_idx=re_idx, **kw)

        def from_y_h_ls():
            return sch.sch_ce_eq_rx_batch(y, h_ls, ce2, "MMSE", re_idx, Qm, scfg, 8, **kw)
        raw_fe(h_ls, y)
        r = from_grid()
        ok = float(r.tb_ok.float().mean())
        same = bool(torch.equal(r.tbblk, from_y_h_ls().tbblk))
        for _ in range(args.warmup):
            from_grid(), from_y_h_ls()
        t_a, t_b = [], []
        for _ in range(args.steps):
            t_a.append(ev(from_grid))
            t_b.append(ev(from_y_h_ls))
        res["chain"][pname] = {"schedule": sched, "tb_ok_rate": ok, "tbblk_equal": same,
                               "sch_slot_rx_batch_from_the_grid": stats(t_a),
                               "sch_ce_eq_rx_batch_from_precomputed_y_and_h_ls": stats(t_b)}
        print(pname, "chain", json.dumps(res["chain"][pname]), flush=True)
        del grid, h_ls, y, ws
        torch.cuda.empty_cache()
    if not args.once:
        save_json(args.out, res)


if __name__ == "__main__":
    main()
