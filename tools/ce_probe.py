"""Channel-estimator probe: ldpc5g_channel_estimate at BASELINE config 5's slot shape (T = 32 slots,
273 PRB, Nr = Nt = 4, DMRS symbols [2, 11], D = 4, eRB = 4, windows 1400 / 1200 ns, scs 30 kHz),
the four algorithms, complex128 and complex64 storage, each call event-timed on its own: warm-ups,
then interleaved steps of every variant, min / median / max.  Then the chain
channel_estimate + equalize + sch_rx_batch beside sch_rx_batch alone, as tools/eq_probe.py does
for the equaliser.

    python tools/ce_probe.py [--T 32] [--steps 20] [--warmup 3] [--lib-b build/libldpc5g_ce_direct.so]
                             [--out profiles/ce/probe.json]

A/B of the forward DFT: --lib-b names a second build of the library with the direct O(M^2) sum,
    LDPC5G_EXTRA_FLAGS=-DLDPC5G_CE_MAX_RADIX=1 python -m python_5gtoolbox_amd.build \
        --csrc python_5gtoolbox_amd/csrc --out build/libldpc5g_ce_direct.so
It is loaded beside the product library (one decimation step by R <= 8), its h and cov are compared
with the product's, and its calls alternate with the product's in the same timed loop.

Per-kernel times come from a separate run under the profiler (one call per variant after one
warm-up; counters, if wanted, go in yet another run):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ce -- python tools/ce_probe.py --once
    python tools/ce_probe.py --kernel-stats DIR/ce_kernel_stats.csv      # merges them into the json

and the reference's own time for one such slot, on a machine that has a py5gphy checkout (CPU
only, one run per algorithm):

    python tools/ce_probe.py --cpu-ref <py5gphy root>                     # merges it into the json

Model numbers written beside the times: the expand launch's bytes (float64 H_est read, h and cov
written) against the 6.29 TB/s copy ceiling, and the tap kernel's float64 lane-ops (4 fused
multiply-adds per complex DFT term, 2 per DCT term, forward M^2 plus back (N + 1)(L_left + L_right)
terms per sequence) against the 78.6 T lane-op/s peak of DESIGN.md §4.6.
"""
import argparse
import csv
import ctypes
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_COPY_GBS = 6290.0
VALU_PEAK_TLANE = 256 * 4 * 32 * 2.4e9 / 1e12
PRB, NR, NT, D, ERB, SCS, SYM = 273, 4, 4, 4, 4, 30, [2, 11]
WIN = (1400, 1200)
NOISE_VAR = 1e-3   # 30 dB, on the DMRS estimate and on the data alike
N = PRB * 12 // D
ALGOS = ("DFT", "DCT", "DFT_symmetric", "DCT_symmetric")


def make_h_ls(T, seed=273):
    """Three paths per (nr, nt) with delays in 0..300 ns scaled to 0.2 rms on top of the identity, plus noise at 30 dB, complex64."""
    rng = np.random.default_rng(seed)
    f = np.arange(N) * D * SCS * 1000.0
    x = np.zeros((T, len(SYM), N, NR, NT), np.complex128)
    for _ in range(3):
        tau = rng.uniform(0, 300e-9, (T, 1, 1, NR, NT))
        amp = (rng.standard_normal((T, 1, 1, NR, NT)) + 1j * rng.standard_normal((T, 1, 1, NR, NT))) / np.sqrt(2)
        x += amp * np.exp(-2j * np.pi * tau * f[None, None, :, None, None])
    # H = I + 0.2 CN(0, 1)-sized entries (as tools/eq_probe.py): well conditioned for the chain
    x = 0.2 / np.sqrt(3) * x + np.eye(NR, NT)[None, None, None]
    x += (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) * np.sqrt(NOISE_VAR / 2)
    return x.astype(np.complex64)


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


def cpu_reference(root, out):
    sys.path.insert(0, root)
    from py5gphy.channel_estimate import dft_dct_CE, dft_dct_symmetric_CE
    H = make_h_ls(1)[0]
    RS = {"RE_distance": D, "scs": SCS, "RSSymMap": SYM, "NumCDMGroupsWithoutData": 2}
    CE = {"L_symm_left_in_ns": WIN[0], "L_symm_right_in_ns": WIN[1], "eRB": ERB, "freq_intp_method": "linear",
          "timing_intp_method": "linear"}
    times = {}
    for algo in ALGOS:
        fn = dft_dct_symmetric_CE.DFT_DCT_symmetric_channel_estimate if algo.endswith("_symmetric") else \
            dft_dct_CE.DFT_DCT_channel_estimate
        t0 = time.perf_counter()
        fn(H.copy(), RS, CE, algo[:3])
        times[algo] = round(time.perf_counter() - t0, 3)
        print(algo, times[algo], "s", flush=True)
    res = load_json(out)
    res["cpu_reference_seconds_per_slot"] = {"note": "py5gphy on one CPU core, one run per algorithm, one slot "
                                             f"({PRB} PRB, {NR}x{NT}, {SYM})", **times}
    save_json(out, res)


def merge_kernel_stats(path, out):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "ce_" in name:
                m = re.search(r"(ce_\w+)<(.*?)>\(", name)
                key = f"{m.group(1)}<{m.group(2).replace('HIP_vector_type<', '').replace(', 2u>', '2').replace(' ,', ',').strip()}>"
                rows[key] = {"calls": int(r["Calls"]), "average_ns": round(float(r["AverageNs"]), 1),
                             "min_ns": int(float(r["MinNs"])), "max_ns": int(float(r["MaxNs"]))}
    res = load_json(out)
    res["kernel_trace"] = {"note": "rocprofv3 --kernel-trace --stats of `ce_probe.py --once` (one warm-up and one "
                                   "call per algorithm and storage type)", "kernels": rows}
    save_json(out, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--lib-b", default=None)
    ap.add_argument("--cpu-ref", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce", "probe.json"))
    args = ap.parse_args()
    if args.cpu_ref:
        return cpu_reference(args.cpu_ref, args.out)
    if args.kernel_stats:
        return merge_kernel_stats(args.kernel_stats, args.out)

    import torch
    import bench
    from python_5gtoolbox_amd import _lib, phy
    from python_5gtoolbox_amd.sch import SchWorkspace, sch_config, sch_encode_batch, sch_rx_batch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda", 0)
    T = args.T
    S, ND, NE = len(SYM), N * D, NR * NT

    def ev(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def stats(ms):
        return {"min_ms": round(min(ms), 5), "median_ms": round(statistics.median(ms), 5), "max_ms": round(max(ms), 5)}

    h_ls64 = torch.tensor(make_h_ls(T)).to(dev)
    lib_a, lib_b = _lib.lib(), None
    if args.lib_b:
        lib_b = _lib.bind(ctypes.CDLL(os.path.abspath(args.lib_b)))

    def raw_ce(lib, h_ls, algo, h, cov):
        """ldpc5g_channel_estimate of `lib` (a ctypes handle) on the current stream."""
        eK, _, M = phy.ce_lengths(N, algo, ERB, D)
        Ll, Lr = phy.ce_window(algo, M, SCS, D, *WIN)
        sym = (ctypes.c_int32 * S)(*SYM)
        rc = lib.ldpc5g_channel_estimate(
            _lib.ptr(h_ls), h_ls.stride(0), _lib.F32 if h_ls.dtype == torch.complex64 else _lib.F64, T, S, N, NR, NT,
            D, sym, _lib.CE_ALGO[algo], eK, Ll, Lr, 2, 0, SCS, _lib.ptr(h), h.stride(0), _lib.ptr(cov),
            cov.stride(0), _lib.ptr(work), work.numel(), None, 0, None, None, None, None, None,
            _lib.stream_ptr(h_ls.device))
        assert rc == 0, rc
    work = torch.empty((int(_lib.lib().ldpc5g_ce_workspace_bytes(T, S, N, NR, NT, D)),), dtype=torch.uint8, device=dev)
    res = load_json(args.out) if not args.once else {}
    res.update({"workload": f"BASELINE config 5 slot shape: T = {T} slots x {PRB} PRB, Nr = Nt = 4, DMRS symbols {SYM}, "
                            f"D = {D}, eRB = {ERB}, windows {WIN} ns, scs {SCS} kHz",
                "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
                "hbm_copy_ceiling_GBs": HBM_COPY_GBS, "valu_peak_Tlane": round(VALU_PEAK_TLANE, 1),
                "forward_dft_ab_library": args.lib_b, "channel_estimate": {}, "chain": {}})
    for pname, cdt in (("complex128", torch.complex128), ("complex64", torch.complex64)):
        h_ls = h_ls64.to(cdt)
        es = h_ls.element_size()
        h = torch.empty((T, 14 * ND, NR, NT), dtype=cdt, device=dev)
        cov = torch.empty((T, 14 * PRB, NR, NR), dtype=cdt, device=dev)
        variants = {a: (lambda a=a: raw_ce(lib_a, h_ls, a, h, cov)) for a in ALGOS}
        same = {}
        if lib_b is not None and not args.once:
            h_b, cov_b = torch.empty_like(h), torch.empty_like(cov)
            for a in ("DFT", "DFT_symmetric"):
                variants[a + "/direct_sum"] = (lambda a=a: raw_ce(lib_b, h_ls, a, h_b, cov_b))
                variants[a](), variants[a + "/direct_sum"]()
                scale = float(h.abs().max())
                same[a] = {"bit_equal": bool(torch.equal(torch.view_as_real(h), torch.view_as_real(h_b)) and
                                             torch.equal(torch.view_as_real(cov), torch.view_as_real(cov_b))),
                           "max_abs_diff_h_over_max": float((h - h_b).abs().max()) / scale}
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
        line = {}
        for a in ALGOS:
            _, _, M = phy.ce_lengths(N, a, ERB, D)
            Ll, Lr = phy.ce_window(a, M, SCS, D, *WIN)
            per_term = 2 if a.startswith("DCT") else 4
            lane_ops = T * S * NE * per_term * (M * M + (N + 1) * (Ll + Lr))
            exp_bytes = T * (S * ND * NE * 16 + 14 * ND * NE * es + 14 * PRB * NR * NR * es)
            line[a] = dict(stats(times[a]), M=M, L_left=Ll, L_right=Lr, tap_kernel_f64_lane_ops=lane_ops,
                           expand_launch_bytes=exp_bytes)
        for k in times:
            if k not in line:
                line[k] = stats(times[k])
        if same:
            line["direct_sum_vs_product"] = same
        res["channel_estimate"][pname] = line
        print(pname, json.dumps(line), flush=True)
        # the chain at config 5: the 11 data symbols of the slot carry the transport block
        A, Qm, Rate, nl, rv, G = (bench.C5[k] for k in ("A", "Qm", "R", "NL", "rv", "G"))
        data_syms = [s for s in range(14) if s not in SYM][:11]
        re_idx = torch.cat([torch.arange(s * ND, (s + 1) * ND, dtype=torch.int32, device=dev) for s in data_syms])
        nre = re_idx.numel()
        assert nl == NT and G == nre * NT * Qm
        cfg = sch_config(A, Qm, Rate, NT, rv, A, G)
        gen = torch.Generator(device=dev)
        gen.manual_seed(36036)
        tb = torch.randint(0, 2, (T, A), dtype=torch.int8, device=dev, generator=gen)
        cinit = torch.arange(T, device=dev, dtype=torch.int64) * 2 ** 15 + 7
        words = phy.prbs_words(cinit, G)
        x = phy.scramble_modulate(sch_encode_batch(tb, cfg), Qm, words=words).to(torch.complex128)
        variants["DFT_symmetric"]()
        hd = h.to(torch.complex128)[:, re_idx.long()]
        sigma2 = NOISE_VAR
        noise = torch.complex(torch.randn((T, nre, NR), dtype=torch.float64, device=dev, generator=gen),
                              torch.randn((T, nre, NR), dtype=torch.float64, device=dev, generator=gen)) * (sigma2 / 2) ** 0.5
        y = torch.zeros((T, 14 * ND, NR), dtype=torch.complex128, device=dev)
        y[:, re_idx.long()] = (hd @ x.view(T, nre, NT, 1))[..., 0] + noise
        y = y.to(cdt)
        del hd, noise, x
        sched, dnt = ("flooding", torch.float64) if cdt == torch.complex128 else ("layered", torch.float32)
        ws = SchWorkspace(cfg, T, dev)
        sym, nv = phy.equalize(y, h, cov, "MMSE", re_idx)

        def rx():
            return sch_rx_batch(sym, nv, Qm, cfg, 8, "min-sum", 0.75, 0.0, sched, words=words, dn_dtype=dnt, ws=ws)

        def ce_eq_rx():
            variants["DFT_symmetric"]()
            phy.equalize(y, h, cov, "MMSE", re_idx, out=(sym, nv))
            return rx()
        ok = float(ce_eq_rx().tb_ok.float().mean())
        for _ in range(args.warmup):
            rx(), ce_eq_rx()
        t_rx, t_all = [], []
        for _ in range(max(args.steps // 2, 3)):
            t_rx.append(ev(rx))
            t_all.append(ev(ce_eq_rx))
        res["chain"][pname] = {"schedule": sched, "tb_ok_rate": ok, "sch_rx_batch_alone": stats(t_rx),
                               "channel_estimate_DFT_symmetric_then_equalize_MMSE_then_sch_rx_batch": stats(t_all)}
        print(pname, "chain", json.dumps(res["chain"][pname]), flush=True)
        del y, h, cov, sym, nv, ws
        torch.cuda.empty_cache()
    if not args.once:
        save_json(args.out, res)


if __name__ == "__main__":
    main()
