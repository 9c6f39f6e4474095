"""Equaliser probe: ldpc5g_equalize at BASELINE config 5's slot shape (nre = 36036 data REs,
Nr = NL = 4, T = 32 transport blocks, G = 8*4*36036 as bench.C5), MMSE and MMSE-IRC, complex128
and complex64 storage, each call event-timed on its own: warm-ups, then interleaved steps of every
variant, min / median / max.  Bytes moved (y, H, cov read; symbols and noise variances written)
over the median time are reported as a fraction of the measured HBM copy ceiling.  Then the
equaliser followed by sch_rx_batch (the whole receive chain from the resource grid), against
sch_rx_batch alone on the same equalised symbols.

A/B of the H load strategy: --lib-b names a second build of the library (the LDS-staged variant,
    LDPC5G_EXTRA_FLAGS=-DLDPC5G_EQ_STAGE_LDS=1 python -m python_5gtoolbox_amd.build \
        --csrc python_5gtoolbox_amd/csrc --out build/libldpc5g_eq_lds.so
); it is loaded beside the product library, its outputs are compared bit for bit, and its calls
alternate with the product's in the same timed loop.

    python tools/eq_probe.py [--T 32] [--steps 20] [--warmup 3] [--lib-b build/libldpc5g_eq_lds.so]
                             [--out profiles/eq/probe.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from python_5gtoolbox_amd import _lib, phy  # noqa: E402
from python_5gtoolbox_amd.sch import SchWorkspace, sch_config, sch_encode_batch, sch_rx_batch  # noqa: E402

HBM_COPY_GBS = 6290.0   # measured float4 copy ceiling of the MI355X (79 % of the 8 TB/s peak)
NRE, NR, NL = 36036, 4, 4


def ev(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms, nbytes=None):
    med = statistics.median(ms)
    out = {"min_ms": round(min(ms), 5), "median_ms": round(med, 5), "max_ms": round(max(ms), 5)}
    if nbytes is not None:
        out["bytes"] = nbytes
        out["GBs_at_median"] = round(nbytes / (med * 1e-3) / 1e9, 1)
        out["frac_of_hbm_copy_ceiling"] = round(nbytes / (med * 1e-3) / 1e9 / HBM_COPY_GBS, 4)
    return out


def raw_equalize(lib, y, h, cov, algo, sym, nv):
    """ldpc5g_equalize of `lib` (a ctypes handle) on the current stream, all REs."""
    T, R, Nr = y.shape
    rc = lib.ldpc5g_equalize(
        _lib.ptr(y), y.stride(0), _lib.ptr(h), h.stride(0), _lib.ptr(cov), cov.stride(0),
        _lib.F32 if y.dtype == torch.complex64 else _lib.F64, None, R, R, 12, T, Nr, h.shape[3],
        _lib.EQ_ALGO[algo], _lib.ptr(sym), sym.stride(0), _lib.ptr(nv), nv.stride(0), _lib.stream_ptr(y.device))
    assert rc == 0, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--snr", type=float, default=30.0)
    ap.add_argument("--lib-b", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eq", "probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda", 0)
    T = args.T
    A, Qm, Rate, nl, rv, G = (bench.C5[k] for k in ("A", "Qm", "R", "NL", "rv", "G"))
    assert nl == NL and G == NRE * NL * Qm
    cfg = sch_config(A, Qm, Rate, NL, rv, A, G)
    lib_a = _lib.lib()
    lib_b = None
    if args.lib_b:
        lib_b = _lib.bind(ctypes.CDLL(os.path.abspath(args.lib_b)))
    gen = torch.Generator(device=dev)
    gen.manual_seed(36036)

    def cn(*shape):
        return torch.complex(torch.randn(shape, dtype=torch.float64, device=dev, generator=gen),
                             torch.randn(shape, dtype=torch.float64, device=dev, generator=gen)) / 2 ** 0.5
    # a transport-block stream through a per-RE channel H = I + 0.2 N(0, 1) and AWGN
    tb = torch.randint(0, 2, (T, A), dtype=torch.int8, device=dev, generator=gen)
    cinit = torch.arange(T, device=dev, dtype=torch.int64) * 2 ** 15 + 7
    words = phy.prbs_words(cinit, G)
    x = phy.scramble_modulate(sch_encode_batch(tb, cfg), Qm, words=words).to(torch.complex128)
    h128 = torch.eye(NR, NL, dtype=torch.complex128, device=dev) + 0.2 * cn(T, NRE, NR, NL)
    sigma2 = 10 ** (-args.snr / 10)
    y128 = ((h128 @ x.view(T, NRE, NL, 1))[..., 0] + cn(T, NRE, NR) * sigma2 ** 0.5).contiguous()
    cov128 = (sigma2 * torch.eye(NR, dtype=torch.complex128, device=dev)).repeat(T, NRE // 12, 1, 1).contiguous()
    del x
    res = {"workload": f"BASELINE config 5 slot shape: T = {T} TBs x nre = {NRE} data REs, Nr = NL = 4, 256QAM, "
                       f"{cfg.C} codeblocks per TB, SNR {args.snr} dB, H = I + 0.2 CN(0, 1) per RE",
           "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "hbm_copy_ceiling_GBs": HBM_COPY_GBS, "load_ab_library": args.lib_b, "equalize": {}, "chain": {}}
    for pname, cdt in (("complex128", torch.complex128), ("complex64", torch.complex64)):
        y, h, cov = y128.to(cdt), h128.to(cdt), cov128.to(cdt)
        es = y.element_size()
        nbytes = T * (NRE * (NR + NR * NL) * es + (NRE // 12) * NR * NR * es + NRE * NL * (es + 4))
        sym = torch.empty((T, NRE * NL), dtype=cdt, device=dev)
        nv = torch.empty((T, NRE * NL), dtype=torch.float32, device=dev)
        sym_b, nv_b = torch.empty_like(sym), torch.empty_like(nv)
        variants = {}
        for algo in ("MMSE", "MMSE-IRC"):
            variants[f"{algo}/direct"] = (lambda a=algo: raw_equalize(lib_a, y, h, cov, a, sym, nv))
            if lib_b is not None:
                variants[f"{algo}/lds_staged"] = (lambda a=algo: raw_equalize(lib_b, y, h, cov, a, sym_b, nv_b))
        same = {}
        if lib_b is not None:
            for algo in ("MMSE", "MMSE-IRC"):
                variants[f"{algo}/direct"](), variants[f"{algo}/lds_staged"]()
                same[algo] = bool(torch.equal(torch.view_as_real(sym), torch.view_as_real(sym_b)) and
                                  torch.equal(nv, nv_b))
                assert same[algo], "the LDS-staged variant must give the same bits"
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        times = {k: [] for k in variants}
        for _ in range(args.steps):   # interleaved: every variant once per step
            for k, fn in variants.items():
                times[k].append(ev(fn))
        line = {k: stats(v, nbytes) for k, v in times.items()}
        line["lds_staged_equals_direct"] = same
        res["equalize"][pname] = line
        print(pname, json.dumps(line), flush=True)
        # the chain: equalise + sch_rx_batch against sch_rx_batch alone (this precision's decoder)
        sched, dnt, alpha = ("flooding", torch.float64, 0.75) if cdt == torch.complex128 else \
            ("layered", torch.float32, 0.75)
        ws = SchWorkspace(cfg, T, dev)

        def rx():
            return sch_rx_batch(sym, nv, Qm, cfg, 8, "min-sum", alpha, 0.0, sched, words=words, dn_dtype=dnt, ws=ws)

        def eq_rx():
            raw_equalize(lib_a, y, h, cov, "MMSE", sym, nv)
            return rx()
        ok = float(eq_rx().tb_ok.float().mean())
        for _ in range(args.warmup):
            rx(), eq_rx()
        t_rx, t_eq_rx = [], []
        for _ in range(max(args.steps // 2, 3)):
            t_rx.append(ev(rx))
            t_eq_rx.append(ev(eq_rx))
        res["chain"][pname] = {"schedule": sched, "tb_ok_rate": ok, "sch_rx_batch_alone": stats(t_rx),
                               "equalize_MMSE_then_sch_rx_batch": stats(t_eq_rx)}
        print(pname, "chain", json.dumps(res["chain"][pname]), flush=True)
        del y, h, cov, sym, nv, sym_b, nv_b, ws
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
