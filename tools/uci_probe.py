"""UCI-on-PUSCH kernel and chain times on the GPU -> profiles/uci/probe.json.

    python tools/uci_probe.py [--steps 30] [--warmup 5]

Shape: BASELINE config 5's slot with UCI: T = 32 slots, 273 PRB x 14 symbols, DMRS symbols [2, 11], 4 layers,
256QAM (MCS 27, TBS 1,081,512), 4-bit HARQ-ACK + 20-bit CSI part 1 + 40-bit CSI part 2, beta-offset indices 9 / 6 / 6.
Every variant is event-timed on its own: warm-ups, then interleaved steps of every variant (each variant once
per step), min / median / max over the steps.  The demultiplexer's bytes are what it must move (LLRs in once,
streams out once, the map once, the scrambling words once) over the median, as a fraction of the 6.29 TB/s copy
ceiling of DESIGN.md §4.7.  The receive chain is timed beside sch_rx_batch on a slot of the same allocation
without UCI (its own symbols, so both chains decode successfully and stop at the same iteration).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "uci", "probe.json")
COPY_CEILING = 6.29e12
T, RB, NL, QM, TBS, CR = 32, 273, 4, 8, 1081512, 948.0
DMRS = [2, 11]
CFG = {"ResAlloType1": {"RBStart": 0, "RBSize": RB}, "StartSymbolIndex": 0, "NrOfSymbols": 14,
       "DMRS": {"NumCDMGroupsWithoutData": 2}, "num_of_layers": NL, "UCIScaling": 1, "EnableULSCH": 1,
       "EnableACK": 1, "NumACKBits": 4, "I_HARQ_ACK_offset": 9, "EnableCSI1": 1, "NumCSI1Bits": 20, "I_CSI1offset": 6,
       "EnableCSI2": 1, "NumCSI2Bits": 40, "I_CSI2offset": 6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch

    from python_5gtoolbox_amd import phy, sch, uci
    assert torch.cuda.is_available(), "uci_probe needs a GPU"
    dev = "cuda:0"
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    G = uci.slot_bits(CFG, DMRS, QM)
    plain = sch.sch_config(TBS, QM, CR, NL, 0, 0, G)
    rm = uci.rm_info(CFG, DMRS, plain.C * plain.K, QM, CR, G)
    p = uci.plan(CFG, DMRS, rm, QM)
    cfg = sch.sch_config(TBS, QM, CR, NL, 0, 0, rm["G_ULSCH"])
    trblk = torch.randint(0, 2, (T, TBS), generator=gen, device=dev, dtype=torch.int8)
    bits = {n: torch.randint(0, 2, (T, A), generator=gen, device=dev, dtype=torch.int8)
            for n, A in (("ack", 4), ("csi1", 20), ("csi2", 40))}
    cinit = torch.arange(T, device=dev, dtype=torch.int32) * 2 ** 15 + 17
    words = phy.prbs_words(cinit, G)
    g_ul = sch.sch_encode_batch(trblk, cfg).clone()
    coded = {n: uci.encode(bits[n], p.lens[n], QM) for n in bits}
    g_seq = uci.mux(p, g_ul, coded["ack"], coded["csi1"], coded["csi2"])
    sym = sch.sch_uci_tx_batch(trblk, bits, p, cfg, QM, words=words)
    sym_plain = phy.scramble_modulate(sch.sch_encode_batch(trblk, plain).clone(), QM, words=words)
    noise = 0.002 ** 0.5
    for s in (sym, sym_plain):
        s += (torch.randn(s.shape, generator=gen, device=dev) + 1j * torch.randn(s.shape, generator=gen, device=dev)) * noise
    nv = torch.full(sym.shape, 2 * noise ** 2, dtype=torch.float32, device=dev)
    llr32 = phy.demod_descramble(sym, nv, QM)
    llr = {"float32": llr32, "float64": llr32.double()}
    ex = p.expand()
    idx = {n: torch.from_numpy(ex["inv"][n]).to(dev) for n in uci.STREAMS}
    sb_llr = (1.0 - 2.0 * uci.smallblock_encode(torch.randint(0, 2, (4096, 11), generator=gen, device=dev, dtype=torch.int8),
                                                64, 2).double()) + torch.randn((4096, 64), generator=gen, device=dev,
                                                                               dtype=torch.float64)
    ws_u, ws_p = sch.SchWorkspace(cfg, T, dev), sch.SchWorkspace(plain, T, dev)
    kw = dict(schedule="layered", alpha=0.75)

    variants = {
        "mux": lambda: uci.mux(p, g_ul, coded["ack"], coded["csi1"], coded["csi2"]),
        "scramble_modulate": lambda: uci.scramble_modulate(g_seq, QM, words=words),
        "smallblock_decode_4096xK11_E64": lambda: uci.smallblock_decode(sb_llr, 11, 2),
        "sch_uci_rx_batch": lambda: sch.sch_uci_rx_batch(sym, nv, QM, p, cfg, 8, words=words, ws=ws_u, **kw),
        "sch_rx_batch_no_uci": lambda: sch.sch_rx_batch(sym_plain, nv, QM, plain, 8, words=words, ws=ws_p, **kw),
    }
    st = uci.demux(p, llr32, words=words)
    variants["demod_no_descramble"] = lambda: phy.demod_descramble(sym, nv, QM)
    variants["sch_decode_batch_ulsch_stream"] = lambda: sch.sch_decode_batch(st.ulsch, cfg, 8, dn_dtype=torch.float32, ws=ws_u, **kw)
    variants["uci_decode_ack_4bit"] = lambda: uci.decode(st.ack, 4, p.lens["ack"], QM)
    variants["uci_decode_csi1_20bit_polar"] = lambda: uci.decode(st.csi1, 20, p.lens["csi1"], QM)
    variants["uci_decode_csi2_40bit_polar"] = lambda: uci.decode(st.csi2, 40, p.lens["csi2"], QM)
    for dt, x in llr.items():
        variants[f"demux_plain_{dt}"] = lambda x=x: uci.demux(p, x, erase_punctured=False)
        variants[f"demux_descramble_{dt}"] = lambda x=x: uci.demux(p, x, words=words)
        variants[f"index_select_{dt}"] = lambda x=x: [x.index_select(1, idx[n]) for n in uci.STREAMS]
    res_u, uci_out = variants["sch_uci_rx_batch"]()
    res_p = variants["sch_rx_batch_no_uci"]()
    ok = dict(tb_ok_uci=int(res_u.tb_ok.sum()), tb_ok_plain=int(res_p.tb_ok.sum()),
              uci_bits_ok=bool(all(torch.equal(uci_out[n], bits[n]) for n in bits)),
              crc_ok=bool(all(uci_out[n + "_crc_ok"].all() for n in ("csi1", "csi2"))),
              iters_uci=float(res_u.iters.float().mean()), iters_plain=float(res_p.iters.float().mean()))
    for dt, x in llr.items():   # the kernel against the composed gather it is compared with
        a, b = uci.demux(p, x, erase_punctured=False), variants[f"index_select_{dt}"]()
        assert all(torch.equal(u, v) for u, v in zip(a, b))

    times = {k: [] for k in variants}
    for step in range(args.warmup + args.steps):
        for k, fn in variants.items():   # interleaved: every variant once per step
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if step >= args.warmup:
                times[k].append(a.elapsed_time(b) * 1e3)
    us = {k: dict(min=float(np.min(v)), median=float(np.median(v)), max=float(np.max(v))) for k, v in times.items()}
    n_inv = p.n_inv
    moved = {}
    for dt, size in (("float32", 4), ("float64", 8)):
        for mode, extra in (("plain", 0), ("descramble", T * 4 * ((G + 31) // 32))):
            nbytes = T * G * size + T * n_inv * size + 4 * n_inv + extra
            med = us[f"demux_{mode}_{dt}"]["median"] * 1e-6
            moved[f"demux_{mode}_{dt}"] = dict(bytes=nbytes, bytes_per_s=nbytes / med, fraction_of_copy_ceiling=nbytes / med / COPY_CEILING,
                                               over_index_select=us[f"demux_{mode}_{dt}"]["median"] / us[f"index_select_{dt}"]["median"])
    out = dict(device=torch.cuda.get_device_name(0),
               method=f"{args.steps} interleaved event-timed steps after {args.warmup} warm-ups; microseconds",
               shape=dict(T=T, RBSize=RB, NL=NL, Qm=QM, TBS=TBS, Gtotal=G, rm=rm, n_inv=n_inv, ldpc="layered float32, L = 8, alpha 0.75"),
               us=us, demux=moved, checks=ok,
               chain_added_us=us["sch_uci_rx_batch"]["median"] - us["sch_rx_batch_no_uci"]["median"])
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))
    print("wrote", os.path.relpath(OUT, ROOT))


if __name__ == "__main__":
    main()
