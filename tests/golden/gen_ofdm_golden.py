"""Generate tests/golden/ofdm_golden_<case>.npz by running the REFERENCE's low-PHY (py5gphy/nr_lowphy):
Rx_low_phy and Tx_low_phy at six carriers, one Tx_low_phy call with Dm, and one whole reception
that starts from time-domain samples.  The reference never travels: only its outputs below (and the
inputs no formula gives) are committed.

    cd <root of a py5gphy checkout> && python <this repository>/tests/golden/gen_ofdm_golden.py

(the working directory must be the reference's root: its LDPC tables and default configurations
load by relative path).

Carrier cases (tests/ofdm_ref.py CASES): the inputs are ofdm_ref.case_inputs' exact-integer formula
(complex64), not stored.  Stored: Rx_low_phy's grid ("rx") and Tx_low_phy's samples ("tx"), for the
two 4096-point cases only symbols {0, 1, 7, 13} of each; gap_rx / gap_tx = max |ofdm_ref - reference|
/ max |reference| with the reference's antenna roll applied to ofdm_ref (fftshift without axes),
asserted <= 64 * 2^-23, and the same without the roll for information where Nr > 1.
DM: Tx_low_phy(fd, carrier, Dm=ofdm_ref.DM) at case A.  Stored: the samples and the fd_slot the call
left behind (it rotates the caller's array in place), with both gaps.
E2E: slot_ref.E2E_CASES["X2"] on the 24-PRB carrier (nfft 512): Pdsch.process, Tx_low_phy, a flat Nr x
num_ant channel and noise of standard deviation 0.02 per component in the time domain, Rx_low_phy,
H_LS_est, NrChannelEstimation.channel_est (DFT_symmetric, eRB 4, 1400 / 1200 ns, timing-offset
compensation on) and RX_process (MMSE-IRC; min-sum, alpha 0.8, beta 0.3, L = 8).  Stored: the
received TIME-DOMAIN slot, the transmitted block, the reference's status and tbblk, the
transport-block geometry.  Asserted: status is true, tbblk equals the transmitted block.
"""
import os
import sys
import time

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.getcwd())
import ofdm_ref  # noqa: E402
import slot_ref  # noqa: E402

GAP_MAX = 64 * 2.0 ** -23


def save(name, **store):
    path = os.path.join(OUT, f"ofdm_golden_{name}.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    assert size <= 512 * 1024, (name, size)
    return size


def carrier(scs, bw, n, mhz, NL=1):
    return {"frequency_range": "FR1", "carrier_frequency_in_mhz": mhz, "PCI": 1, "BW": bw, "scs": scs,
            "num_of_ant": n, "Nr": n, "maxMIMO_layers": NL, "duplex_type": "TDD"}


def relgap(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def carrier_cases():
    from py5gphy.common import nr_slot
    from py5gphy.nr_lowphy import rx_lowphy_process, tx_lowphy_process
    for name, (scs, bw, prbs, nr, mhz, syms) in ofdm_ref.CASES.items():
        assert nr_slot.get_carrier_prb_size(scs, bw) == prbs
        assert nr_slot.get_FFT_IFFT_size(prbs) == ofdm_ref.nfft_of(prbs)
        cc = carrier(scs, bw, nr, mhz)
        hz = int(mhz * 10 ** 6)
        td, fd = ofdm_ref.case_inputs(name)
        rx = rx_lowphy_process.Rx_low_phy(td.copy(), cc)
        tx = tx_lowphy_process.Tx_low_phy(fd.copy(), cc)
        assert rx.dtype == np.complex64 and tx.dtype == np.complex64
        my_rx, my_tx = ofdm_ref.demod(td, scs, prbs, hz), ofdm_ref.mod(fd, scs, prbs, hz)
        ig, it = ofdm_ref.sym_slices(name, "grid"), ofdm_ref.sym_slices(name, "td")
        assert relgap(ofdm_ref.roll(my_rx), rx) <= GAP_MAX and relgap(ofdm_ref.roll(my_tx), tx) <= GAP_MAX, name
        gr, gt = relgap(ofdm_ref.roll(my_rx)[:, ig], rx[:, ig]), relgap(ofdm_ref.roll(my_tx)[:, it], tx[:, it])   # what is stored
        nr_, nt_ = relgap(my_rx, rx), relgap(my_tx, tx)
        assert gr <= GAP_MAX and gt <= GAP_MAX, (name, gr, gt)
        size = save(name, rx=rx[:, ig], tx=tx[:, it], gap_rx=np.float64(gr), gap_tx=np.float64(gt),
                    noroll_rx=np.float64(nr_), noroll_tx=np.float64(nt_))
        print(f"{name}: nfft {ofdm_ref.nfft_of(prbs)} Nr {nr} gap rx {gr:.2e} tx {gt:.2e} "
              f"(without the roll {nr_:.2e} {nt_:.2e}) {size} bytes")


def dm_case():
    from py5gphy.nr_lowphy import tx_lowphy_process
    scs, bw, prbs, nr, mhz, _ = ofdm_ref.CASES[ofdm_ref.DM_CASE]
    _, fd = ofdm_ref.case_inputs(ofdm_ref.DM_CASE)
    mutated = fd.copy()
    tx = tx_lowphy_process.Tx_low_phy(mutated, carrier(scs, bw, nr, mhz), Dm=list(ofdm_ref.DM))
    assert not np.array_equal(mutated, fd), "Tx_low_phy with Dm rotates the caller's fd_slot in place"
    my_fd = ofdm_ref.dm_rotate(fd, scs, prbs, ofdm_ref.DM)
    my_tx = ofdm_ref.roll(ofdm_ref.mod(fd, scs, prbs, int(mhz * 10 ** 6), dm=ofdm_ref.DM))
    gf, gt = relgap(my_fd, mutated), relgap(my_tx, tx)
    assert gf <= GAP_MAX and gt <= GAP_MAX, (gf, gt)
    size = save("DM", tx=tx, fd=mutated, gap_fd=np.float64(gf), gap_tx=np.float64(gt))
    print(f"DM: gap fd {gf:.2e} tx {gt:.2e} {size} bytes")


def e2e_case(rng):
    from py5gphy.channel_estimate import nr_channel_estimation
    from py5gphy.common import nr_slot
    from py5gphy.nr_lowphy import rx_lowphy_process, tx_lowphy_process
    from py5gphy.nr_pdsch import nr_pdsch
    c = slot_ref.E2E_CASES["X2"]
    e = ofdm_ref.E2E
    cfg = slot_ref.pdsch_config(**c["cfg"])
    NL, Nr, slot = cfg["num_of_layers"], c["Nr"], c["slot"]
    assert Nr == e["Nr"] and nr_slot.get_carrier_prb_size(e["scs"], e["BW"]) == e["prbs"] == slot_ref.CARRIER_PRB
    cc = carrier(e["scs"], e["BW"], NL, 3840, NL)
    cc["Nr"] = Nr
    pd = nr_pdsch.Pdsch(cfg, cc)
    fd, usage = nr_slot.init_fd_slot(NL, e["prbs"])
    fd, usage = pd.process(fd, usage, slot)
    tx = tx_lowphy_process.Tx_low_phy(fd, cc)
    q, _ = np.linalg.qr(rng.standard_normal((Nr, Nr)) + 1j * rng.standard_normal((Nr, Nr)))
    H0 = (q * rng.uniform(0.8, 1.25, Nr))[:, :NL]
    rx = H0 @ tx.astype(np.complex128)
    rx = (rx + e["snr_sigma"] * (rng.standard_normal(rx.shape) + 1j * rng.standard_normal(rx.shape))).astype(np.complex64)
    t0 = time.time()
    rx_fd = rx_lowphy_process.Rx_low_phy(rx, cc)
    H_LS, info = pd.H_LS_est(rx_fd, slot)
    CE_config = {"enable_TO_comp": True, "enable_FO_est": False, "enable_FO_comp": False,
                 "CE_algo": "DFT_symmetric", "L_symm_left_in_ns": 1400, "L_symm_right_in_ns": 1200, "eRB": 4}
    ce = nr_channel_estimation.NrChannelEstimation(H_LS, info, CE_config)
    H_result, cov_m = ce.channel_est()
    status, tbblk, _ = pd.RX_process(rx_fd, slot, {"algo": c["algo"]}, H_result, cov_m,
                                     {"L": 8, "algo": "min-sum", "alpha": 0.8, "beta": 0.3}, ce)
    dt = time.time() - t0
    assert status
    A = pd.info["TBSize"]
    assert np.array_equal(np.asarray(tbblk)[:A], pd.trblk)
    idx, _ = slot_ref.data_re_idx(cfg)
    meta = np.array([A, pd.info["Qm"], pd.info["TBS_LBRM"], idx.size * NL * pd.info["Qm"]], np.int64)
    gap = relgap(ofdm_ref.roll(ofdm_ref.demod(rx, e["scs"], e["prbs"], 3840 * 10 ** 6)), rx_fd)
    assert gap <= GAP_MAX, gap
    size = save("E2E", td=rx, trblk=np.asarray(pd.trblk, np.int8), status=np.bool_(status),
                tbblk=np.asarray(tbblk, np.int8), meta=meta, coderate=np.float64(pd.info["coderateby1024"]),
                gap_rx=np.float64(gap))
    print(f"E2E: A={A} Qm={pd.info['Qm']} G={meta[3]} gap rx {gap:.2e} reference receive {dt:.1f} s {size} bytes")


def main():
    assert os.path.isdir("py5gphy"), "run from the root of a py5gphy checkout"
    rng = np.random.default_rng(20261022)
    np.random.seed(20261022)   # Pdsch.get_trblk draws from the global generator
    carrier_cases()
    dm_case()
    e2e_case(rng)


if __name__ == "__main__":
    main()
