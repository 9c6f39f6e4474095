"""Generate tests/golden/tp_golden_<case>.npz by running the REFERENCE (py5gphy) with
nTransPrecode = 1: its low-PAPR sequences, its hopping, its LS estimates, its transmit processing
and two whole receptions.  The reference never travels: only the inputs and its outputs below are
committed.

    cd <root of a py5gphy checkout> && python <this repository>/tests/golden/gen_tp_golden.py

(the working directory must be the reference's root: its LDPC tables and default configurations
load by relative path).  All grids are the 10 MHz / 30 kHz carrier's (24 PRB).

seq (tests/tp_ref.py SEQ_CASES): gen_lowPAPR_seq outputs, with gap = max |tp_ref - reference|
asserted <= 1e-8 (the reference evaluates pi q m (m+1) / N in floating point at large arguments);
and the table sequences of length 6, 12, 18, 24 for u in SHORT_U, which feed base_seq.
hop: the (u, v) that _gen_seq_with_transform_precoding hands to gen_lowPAPR_seq for HOP_IDS x the
three hopping modes x HOP_SLOTS x HOP_SYMS at a 20-PRB allocation, asserted equal to tp_ref.hop_uv.
LS cases (LS_CASES): pusch_dmrs_LS_est on a random complex64 grid.  Stored: grid, h_ls, slot, gap =
max |tp_ref - reference| / max |reference|, asserted <= 64 * 2^-23; the base sequences of the
RBSize-2 case come from the seq fixture's table sequences.
process / map cases (MAP_CASES): NrPUSCH.process on a zero grid.  Stored: the modulated symbols
(recomputed from nr_pusch_process's arguments with the reference's own scrambler and modulator),
nr_pusch_process's output, the transmit grid, the data-RE indices, slot, and the gaps of
tp_ref.process / tp_ref.tp_map, same cap.
End-to-end cases (E2E_CASES): NrPUSCH.process, a flat 1 x Nr channel and noise of standard
deviation 0.02 per component, then H_LS_est, NrChannelEstimation.channel_est (DFT_symmetric, eRB 4,
1400 / 1200 ns, timing-offset compensation on) and RX_process (MMSE; min-sum, alpha 0.8, beta 0.3,
L = 8).  Stored: the received grid, the transmitted block, the reference's status and tbblk, and the
transport-block geometry.  Asserted: status is true, tbblk equals the transmitted block.
"""
import json
import os
import sys
import time

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.getcwd())
import tp_ref  # noqa: E402

GAP_MAX = 64 * 2.0 ** -23
PRB = tp_ref.CARRIER_PRB


def save(name, **store):
    path = os.path.join(OUT, f"tp_golden_{name}.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    assert size <= 512 * 1024, (name, size)
    return size


def full_config(kw):
    """tp_ref's config on top of the reference's default PUSCH configuration."""
    with open("py5gphy/nr_default_config/default_pusch_config.json") as f:
        cfg = json.load(f)
    mine = tp_ref.pusch_config(**kw)
    cfg["DMRS"].update(mine.pop("DMRS"))
    cfg.update(mine)
    return cfg


def seq_cases():
    from py5gphy.common import lowPAPR_seq
    store, worst = {}, 0.0
    for name, (u, v, alpha, MZC) in tp_ref.SEQ_CASES.items():
        ref = lowPAPR_seq.gen_lowPAPR_seq(u, v, alpha, MZC)
        assert ref.shape == (MZC,) and ref.dtype == np.complex128
        gap = float(np.abs(tp_ref.low_papr_seq(u, v, alpha, MZC) - ref).max())
        assert gap <= 1e-8, (name, gap)
        worst = max(worst, gap)
        store[name], store[name + "_gap"] = ref, np.float64(gap)
    for MZC in tp_ref.SHORT_MZC:
        tab = np.stack([lowPAPR_seq.gen_lowPAPR_seq(u, 0, 0, MZC) for u in tp_ref.SHORT_U])
        assert np.allclose(np.abs(tab), 1.0)
        store[f"short{MZC}"] = tab
    print(f"seq: worst gap {worst:.2e}, {save('seq', **store)} bytes")
    return store


def hop_cases():
    from py5gphy.common import lowPAPR_seq
    from py5gphy.nr_pusch import nr_pusch_dmrs
    tab = np.zeros((len(tp_ref.HOP_IDS), 3, len(tp_ref.HOP_SLOTS), len(tp_ref.HOP_SYMS), 2), np.int16)
    seen = []
    real = lowPAPR_seq.gen_lowPAPR_seq

    def spy(u, v, alpha, MZC):
        seen.append((int(u), int(v)))
        return real(u, v, alpha, MZC)
    lowPAPR_seq.gen_lowPAPR_seq = spy
    try:
        for a, nid in enumerate(tp_ref.HOP_IDS):
            for b, mode in enumerate(tp_ref.HOPPING):
                for c, slot in enumerate(tp_ref.HOP_SLOTS):
                    for d, sym in enumerate(tp_ref.HOP_SYMS):
                        nr_pusch_dmrs._gen_seq_with_transform_precoding(nid, mode, 120, slot, sym)
                        tab[a, b, c, d] = seen[-1]
                        assert seen[-1] == tp_ref.hop_uv(nid, mode, 120, slot, sym), (nid, mode, slot, sym)
    finally:
        lowPAPR_seq.gen_lowPAPR_seq = real
    assert len(np.unique(tab[:, 1, ..., 0])) > 5 and set(np.unique(tab[:, 2, ..., 1])) == {0, 1}
    print("hop:", save("hop", table=tab), "bytes")


def ls_cases(rng, seq):
    from py5gphy.nr_pusch import nr_pusch_dmrs
    for name, (kw, Nr, slot) in tp_ref.LS_CASES.items():
        cfg = full_config(kw)
        grid = ((rng.standard_normal((Nr, 14 * 12 * PRB)) + 1j * rng.standard_normal((Nr, 14 * 12 * PRB)))
                / np.sqrt(2)).astype(np.complex64)
        H, info = nr_pusch_dmrs.pusch_dmrs_LS_est(grid.copy(), cfg, slot)
        assert H.dtype == np.complex64
        p = tp_ref.tp_params(cfg)
        base = None
        if kw["rb_size"] <= 4:   # the table sequence of u = nPuschID % 30, one row per DMRS symbol
            u = tp_ref.SHORT_U.index(p["npuschid"] % 30)
            base = np.tile(seq[f"short{6 * kw['rb_size']}"][u], (len(p["syms"]), 1))
        mine = tp_ref.ls_est(grid, cfg, slot, base)
        assert mine.shape == H.shape and info["RSSymMap"] == p["syms"]
        gap = float(np.abs(mine - H).max() / np.abs(H).max())
        assert gap <= GAP_MAX, (name, gap)
        size = save("L" + name, grid=grid, h_ls=H, slot=np.int32(slot), gap=np.float64(gap))
        print(f"L{name}: h_ls {H.shape} gap={gap:.2e} {size} bytes")


def carrier(num_ant, Nr):
    return {"frequency_range": "FR1", "carrier_frequency_in_mhz": 3840, "PCI": 1, "BW": 10, "scs": 30,
            "num_of_ant": num_ant, "Nr": Nr, "maxMIMO_layers": 1, "duplex_type": "TDD"}


def transmit(cfg, num_ant, slot):
    """(NrPUSCH, transmit grid, modulated symbols, nr_pusch_process's output) of one process call."""
    from py5gphy.common import nr_slot, nrModulation, nrPRBS
    from py5gphy.nr_pusch import nr_pusch, nr_pusch_process
    pu = nr_pusch.NrPUSCH(carrier(num_ant, num_ant), cfg)
    fd, usage = nr_slot.init_fd_slot(num_ant, PRB)
    seen = {}
    real = nr_pusch_process.nr_pusch_process

    def spy(g_seq, rnti, nID, Qm, *rest):
        out = real(g_seq, rnti, nID, Qm, *rest)
        seen.update(g=np.array(g_seq), rnti=rnti, nID=nID, Qm=Qm, out=np.array(out))
        return out
    nr_pusch_process.nr_pusch_process = spy
    try:
        fd, usage = pu.process(fd, usage, slot)
    finally:
        nr_pusch_process.nr_pusch_process = real
    g = seen["g"]
    assert g.min() >= 0   # no UCI placeholders
    scr = (g + nrPRBS.gen_nrPRBS(seen["rnti"] * 2 ** 15 + seen["nID"], g.size)) % 2
    sym = nrModulation.nrModulate(scr, {2: "QPSK", 4: "16QAM", 6: "64QAM", 8: "256QAM"}[seen["Qm"]])
    return pu, fd, np.asarray(sym, np.complex64), np.atleast_2d(seen["out"])


def map_cases():
    from py5gphy.nr_pusch import nr_pusch_precoding
    for name, (kw, num_ant, slot) in tp_ref.MAP_CASES.items():
        cfg = full_config(kw)
        pu, fd, sym, precoded = transmit(cfg, num_ant, slot)
        assert fd.dtype == np.complex64 and fd.shape == (num_ant, 14 * 12 * PRB)
        idx, _ = tp_ref.data_re_idx(cfg)
        assert sym.size == idx.size and precoded.shape == (num_ant, sym.size)
        pm = None if num_ant == 1 else nr_pusch_precoding.get_precoding_matrix(1, num_ant, kw["pmi"])
        mine = tp_ref.process(sym, kw["rb_size"], pm)
        gap_p = float(np.abs(mine - precoded).max() / np.abs(precoded).max())
        grid = tp_ref.tp_map(sym, cfg, slot, PRB, num_ant, pm)
        assert np.all((grid != 0) == (fd != 0)), name   # the same REs are written
        gap_g = float(np.abs(grid - fd).max() / np.abs(fd).max())
        assert gap_p <= GAP_MAX and gap_g <= GAP_MAX, (name, gap_p, gap_g)
        size = save(name, grid=fd, sym=sym, precoded=precoded.astype(np.complex64), re_idx=idx, slot=np.int32(slot),
                    gap_process=np.float64(gap_p), gap_grid=np.float64(gap_g),
                    precoding=np.zeros((0, 1), np.complex64) if pm is None else np.asarray(pm, np.complex64))
        print(f"{name}: nre={idx.size} gap process {gap_p:.2e} grid {gap_g:.2e} {size} bytes")


def e2e_cases(rng):
    from py5gphy.channel_estimate import nr_channel_estimation
    for name, c in tp_ref.E2E_CASES.items():
        cfg = full_config(c["cfg"])
        Nr, slot = c["Nr"], c["slot"]
        pu, fd, _, _ = transmit(cfg, 1, slot)
        H0 = (rng.standard_normal((Nr, 1)) + 1j * rng.standard_normal((Nr, 1))) / np.sqrt(2)
        H0 = H0 / np.abs(H0) * rng.uniform(0.8, 1.25, (Nr, 1))   # flat, gains in 0.8 .. 1.25
        rx = H0 @ fd.astype(np.complex128)
        rx = (rx + 0.02 * (rng.standard_normal(rx.shape) + 1j * rng.standard_normal(rx.shape))).astype(np.complex64)
        t0 = time.time()
        H_LS, info = pu.H_LS_est(rx, slot)
        CE_config = {"enable_TO_comp": True, "enable_FO_est": False, "enable_FO_comp": False,
                     "CE_algo": "DFT_symmetric", "L_symm_left_in_ns": 1400, "L_symm_right_in_ns": 1200, "eRB": 4}
        ce = nr_channel_estimation.NrChannelEstimation(H_LS, info, CE_config)
        H_result, cov_m = ce.channel_est()
        status, tbblk, _ = pu.RX_process(rx, slot, {"algo": "MMSE"}, H_result, cov_m,
                                         {"L": 8, "algo": "min-sum", "alpha": 0.8, "beta": 0.3}, ce)
        dt = time.time() - t0
        assert status, name
        A = pu.info["TBSize"]
        assert np.array_equal(np.asarray(tbblk)[:A], pu.trblk), name
        idx, _ = tp_ref.data_re_idx(cfg)
        meta = np.array([A, pu.info["Qm"], idx.size * pu.info["Qm"]], np.int64)
        size = save(name, grid=rx, trblk=np.asarray(pu.trblk, np.int8), status=np.bool_(status),
                    tbblk=np.asarray(tbblk, np.int8), meta=meta, coderate=np.float64(pu.info["coderateby1024"]))
        print(f"{name}: A={A} Qm={pu.info['Qm']} G={meta[2]} reference receive {dt:.1f} s {size} bytes")


def main():
    assert os.path.isdir("py5gphy"), "run from the root of a py5gphy checkout"
    rng = np.random.default_rng(20261020)
    np.random.seed(20261020)   # NrPUSCH.get_trblk draws from the global generator
    seq = seq_cases()
    hop_cases()
    ls_cases(rng, seq)
    map_cases()
    e2e_cases(rng)


if __name__ == "__main__":
    main()
