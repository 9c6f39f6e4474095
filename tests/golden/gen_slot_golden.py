"""Generate tests/golden/slot_golden_<case>.npz by running the REFERENCE (py5gphy): its LS
estimates, its usage maps and transmit grids, and two whole receptions.  The reference never
travels: only the inputs and its outputs below are committed.

    cd <root of a py5gphy checkout> && python <this repository>/tests/golden/gen_slot_golden.py

(the working directory must be the reference's root: its LDPC tables load by relative path).
All grids are the 10 MHz / 30 kHz carrier's (24 PRB), so a whole grid fits a fixture.

LS cases (tests/slot_ref.py LS_CASES): pdsch_dmrs_LS_est / pusch_dmrs_LS_est on a random complex64
grid (unit-variance entries, which stand for signal plus noise alike: the LS step is linear).
Stored: grid, h_ls as the reference returns it, slot, gap = max |slot_ref - reference| /
max |reference|, asserted <= 64 * 2^-23 (the reference multiplies in complex64).
Symbol lists: both get_DMRS_symlist tables for Ld 3..14 and DMRSAddPos 0..3 (slot_golden_symlists).
Map cases (MAP_CASES): Pdsch.process on a zero grid.  Stored: the transmit grid, the
layer-interleaved modulated symbols it mapped (recomputed from nr_pdsch_encode's arguments with the
reference's own scrambler and modulator), copy_Rx_pdsch_resource's usage map, the data-RE indices
read off that map, slot.  Asserted:
slot_ref's mapper equals the grid (exactly with identity precoding, within 4 NL 2^-23 max|grid|
with the matrix), slot_ref's usage map and extraction equal the reference's.
End-to-end cases (E2E_CASES): Pdsch.process, a flat Nr x NL channel, a 60 ns delay and noise of
standard deviation 0.03 per component, then H_LS_est, NrChannelEstimation.channel_est
(DFT_symmetric, eRB 4, 1400 / 1200 ns, timing-offset compensation on) and RX_process (min-sum,
alpha 0.8, beta 0.3, L = 8).  Stored: the received grid, the transmitted block, the reference's
status and tbblk, and the transport-block geometry.  Asserted: status is true, tbblk equals the
transmitted block.
"""
import os
import sys
import time

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.getcwd())
import slot_ref  # noqa: E402

GAP_MAX = 64 * 2.0 ** -23
PRB = slot_ref.CARRIER_PRB


def save(name, **store):
    path = os.path.join(OUT, f"slot_golden_{name}.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    assert size <= 512 * 1024, (name, size)
    return size


def ls_cases(rng):
    from py5gphy.nr_pdsch import nr_pdsch_dmrs
    from py5gphy.nr_pusch import nr_pusch_dmrs
    for name, (kind, kw, Nr, slot) in slot_ref.LS_CASES.items():
        cfg = slot_ref.make_config(kind, kw)
        grid = ((rng.standard_normal((Nr, 14 * 12 * PRB)) + 1j * rng.standard_normal((Nr, 14 * 12 * PRB)))
                / np.sqrt(2)).astype(np.complex64)
        fn = nr_pusch_dmrs.pusch_dmrs_LS_est if kind == "pusch" else nr_pdsch_dmrs.pdsch_dmrs_LS_est
        H, info = fn(grid.copy(), cfg, slot)
        assert H.dtype == np.complex64
        mine = slot_ref.ls_est(grid, cfg, slot)
        assert mine.shape == H.shape and info["RSSymMap"] == slot_ref.params(cfg)["syms"]
        gap = float(np.abs(mine - H).max() / np.abs(H).max())
        assert gap <= GAP_MAX, (name, gap)
        size = save("L" + name, grid=grid, h_ls=H, slot=np.int32(slot), gap=np.float64(gap))
        print(f"L{name}: h_ls {H.shape} gap={gap:.2e} {size} bytes")


def symlists():
    """Both get_DMRS_symlist tables for Ld 3..14 and DMRSAddPos 0..3, padded with -1."""
    from py5gphy.nr_pdsch import nr_pdsch_dmrs
    from py5gphy.nr_pusch import nr_pusch_dmrs
    tab = np.full((2, 12, 4, 4), -1, np.int8)
    for c, mod in enumerate((nr_pdsch_dmrs, nr_pusch_dmrs)):
        for Ld in range(3, 15):
            for ap in range(4):
                lst = mod.get_DMRS_symlist(Ld, ap)
                assert lst == slot_ref.symlist(Ld, ap, ("pdsch", "pusch")[c])
                tab[c, Ld - 3, ap, :len(lst)] = lst
    print("symlists:", save("symlists", table=tab), "bytes")


def carrier(num_ant, Nr, NL):
    return {"frequency_range": "FR1", "carrier_frequency_in_mhz": 3840, "PCI": 1, "BW": 10, "scs": 30,
            "num_of_ant": num_ant, "Nr": Nr, "maxMIMO_layers": NL, "duplex_type": "TDD"}


def transmit(cfg, num_ant, slot, NL):
    """(Pdsch, transmit grid, layer-interleaved modulated symbols) of one Pdsch.process call."""
    from py5gphy.common import nr_slot, nrModulation, nrPRBS
    from py5gphy.nr_pdsch import nr_pdsch, nr_pdsch_process
    pd = nr_pdsch.Pdsch(cfg, carrier(num_ant, num_ant, NL))
    fd, usage = nr_slot.init_fd_slot(num_ant, PRB)
    seen = {}
    real = nr_pdsch_process.nr_pdsch_encode

    def spy(g_seq, rnti, nID, Qm, num_of_layers, precoding_matrix, num_of_ant):
        seen.update(g=np.array(g_seq), rnti=rnti, nID=nID, Qm=Qm)
        return real(g_seq, rnti, nID, Qm, num_of_layers, precoding_matrix, num_of_ant)
    nr_pdsch_process.nr_pdsch_encode = spy
    try:
        fd, usage = pd.process(fd, usage, slot)
    finally:
        nr_pdsch_process.nr_pdsch_encode = real
    g = seen["g"]
    scr = (g + nrPRBS.gen_nrPRBS(seen["rnti"] * 2 ** 15 + seen["nID"], g.size)) % 2
    sym = nrModulation.nrModulate(scr, {2: "QPSK", 4: "16QAM", 6: "64QAM", 8: "256QAM"}[seen["Qm"]])
    return pd, fd, np.asarray(sym, np.complex64)


def map_cases():
    from py5gphy.nr_pdsch import nrpdsch_resource_mapping
    for name, (kw, num_ant, pm, slot) in slot_ref.MAP_CASES.items():
        cfg = slot_ref.pdsch_config(**kw, precoding=() if pm is None else pm)
        cfg["allocated_slots"] = [0]
        NL = cfg["num_of_layers"]
        pd, fd, sym = transmit(cfg, num_ant, slot, NL)
        assert fd.dtype == np.complex64
        res, usage = nrpdsch_resource_mapping.copy_Rx_pdsch_resource(fd, cfg)
        idx, my_usage = slot_ref.data_re_idx(cfg)
        assert np.array_equal(usage, my_usage) and sym.size == idx.size * NL
        p = slot_ref.params(cfg)
        y = slot_ref.extract(fd, cfg).reshape(14, 12 * p["rb_size"], num_ant)
        assert np.array_equal(y[p["start"]:p["start"] + p["nsym"]], res)
        mine = slot_ref.slot_map(sym, cfg, slot, PRB, num_ant, pm)
        if pm is None:
            assert np.all(mine == fd), name
        else:
            assert np.abs(mine - fd).max() <= 4 * NL * 2.0 ** -23 * np.abs(fd).max(), name
        m, re = np.nonzero(usage == 0)   # the data REs in the order RX_process visits them
        re_idx = ((m + p["start"]) * 12 * p["rb_size"] + re).astype(np.int32)
        assert np.array_equal(re_idx, idx)
        size = save(name, grid=fd, sym=sym, usage=usage, re_idx=re_idx, slot=np.int32(slot))
        print(f"{name}: NL={NL} nre={idx.size} {size} bytes")


def e2e_cases(rng):
    from py5gphy.channel_estimate import nr_channel_estimation
    for name, c in slot_ref.E2E_CASES.items():
        cfg = slot_ref.pdsch_config(**c["cfg"])
        NL, Nr, slot = cfg["num_of_layers"], c["Nr"], c["slot"]
        pd, fd, _ = transmit(cfg, NL, slot, NL)
        # a flat, well-conditioned channel: a unitary matrix times gains in 0.8 .. 1.25
        q, _ = np.linalg.qr(rng.standard_normal((Nr, Nr)) + 1j * rng.standard_normal((Nr, Nr)))
        H0 = (q * rng.uniform(0.8, 1.25, Nr))[:, :NL]
        k = np.tile(np.arange(12 * PRB), 14)
        rx = (H0 @ fd.astype(np.complex128)) * np.exp(-2j * np.pi * 60e-9 * k * 30e3)
        rx = (rx + 0.03 * (rng.standard_normal(rx.shape) + 1j * rng.standard_normal(rx.shape))).astype(np.complex64)
        t0 = time.time()
        H_LS, info = pd.H_LS_est(rx, slot)
        CE_config = {"enable_TO_comp": True, "enable_FO_est": False, "enable_FO_comp": False,
                     "CE_algo": "DFT_symmetric", "L_symm_left_in_ns": 1400, "L_symm_right_in_ns": 1200, "eRB": 4}
        ce = nr_channel_estimation.NrChannelEstimation(H_LS, info, CE_config)
        H_result, cov_m = ce.channel_est()
        status, tbblk, _ = pd.RX_process(rx, slot, {"algo": c["algo"]}, H_result, cov_m,
                                         {"L": 8, "algo": "min-sum", "alpha": 0.8, "beta": 0.3}, ce)
        dt = time.time() - t0
        assert status, name
        A = pd.info["TBSize"]
        assert np.array_equal(np.asarray(tbblk)[:A], pd.trblk), name
        idx, _ = slot_ref.data_re_idx(cfg)
        meta = np.array([A, pd.info["Qm"], pd.info["TBS_LBRM"], idx.size * NL * pd.info["Qm"]], np.int64)
        size = save(name, grid=rx, trblk=np.asarray(pd.trblk, np.int8), status=np.bool_(status),
                    tbblk=np.asarray(tbblk, np.int8), meta=meta, coderate=np.float64(pd.info["coderateby1024"]))
        print(f"{name}: A={A} Qm={pd.info['Qm']} G={meta[3]} reference receive {dt:.1f} s {size} bytes")


def main():
    assert os.path.isdir("py5gphy"), "run from the root of a py5gphy checkout"
    rng = np.random.default_rng(20261021)
    np.random.seed(20261021)   # Pdsch.get_trblk draws from the global generator
    symlists()
    ls_cases(rng)
    map_cases()
    e2e_cases(rng)


if __name__ == "__main__":
    main()
