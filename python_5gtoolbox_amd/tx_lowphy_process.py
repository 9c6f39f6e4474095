"""Drop-in for py5gphy/nr_lowphy/tx_lowphy_process.py on the GPU (ldpc5g_ofdm_mod, float64 arithmetic).

    Tx_low_phy(fd_slot, carrier_config, Dm=[]) -> td_slot (num_of_ant, 15*nfft) complex64

Two behaviours of the reference are reproduced here and only here (phy.ofdm_mod has neither): its
fft.ifftshift has no `axes`, so row r of the result is antenna (r - num_of_ant // 2) mod num_of_ant;
and with Dm it rotates the symbols of the caller's fd_slot in place.  channel_filter (FIR and
half-band filters designed by scipy.signal.remez) is not provided.
"""
import numpy as np

from . import _lib, nr_slot, phy


def Tx_low_phy(fd_slot, carrier_config, Dm=[]):
    """tx_lowphy_process.py:10-80"""
    scs, BW = carrier_config["scs"], carrier_config["BW"]
    num_of_ant = carrier_config["num_of_ant"]
    prbs = nr_slot.get_carrier_prb_size(scs, BW)
    nfft = phy.ofdm_params(scs, prbs)[0]
    assert fd_slot.ndim == 2 and fd_slot.shape[0] == num_of_ant, f"fd_slot {fd_slot.shape}: num_of_ant = {num_of_ant} rows"
    sc_size = fd_slot.shape[1] // 14
    if sc_size != 12 * prbs:
        raise NotImplementedError(f"fd_slot holds {sc_size} subcarriers per symbol, the carrier {12 * prbs}")
    t = _lib.require_gpu()
    if len(Dm) > 0:   # in place, in fd_slot's own dtype (:54-55)
        for sym in range(14):
            fd_slot[:, sc_size * sym:sc_size * (sym + 1)] *= np.exp(1j * 2 * np.pi * np.arange(sc_size) * scs * 1000 * Dm[sym])
    fd = np.asarray(fd_slot)[:, :14 * sc_size]
    fd = np.ascontiguousarray(fd if fd.dtype == np.complex64 else fd.astype(np.complex128))
    td = phy.ofdm_mod(t.from_numpy(fd[None]).cuda(), scs, prbs, carrier_config["carrier_frequency_in_mhz"])
    return np.roll(td[0].cpu().numpy(), num_of_ant // 2, axis=0).astype(np.complex64)


def channel_filter(td_waveform, carrier_config, sample_rate_in_hz):
    """tx_lowphy_process.py:82-153"""
    raise NotImplementedError("channel_filter: the FIR and half-band filters the reference designs with "
                              "scipy.signal.remez are not provided")
