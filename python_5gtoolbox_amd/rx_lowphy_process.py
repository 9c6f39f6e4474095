"""Drop-in for py5gphy/nr_lowphy/rx_lowphy_process.py on the GPU (ldpc5g_ofdm_demod, float64 arithmetic).

    Rx_low_phy(td_slot, carrier_config) -> fd_slot (Nr, 14*12*carrier_prbs) complex64

The reference's fft.fftshift has no `axes`, so it also shifts the antenna axis: row r of its result
is antenna (r - Nr // 2) mod Nr.  Rx_low_phy here reproduces that; phy.ofdm_demod, the batched
function underneath, never permutes antennas.  channel_filter and waveform_rx_processing (FIR and
half-band filters designed by scipy.signal.remez) are not provided.
"""
import numpy as np

from . import _lib, nr_slot, phy


def _carrier(carrier_config):
    scs, BW = carrier_config["scs"], carrier_config["BW"]
    prbs = nr_slot.get_carrier_prb_size(scs, BW)
    return scs, prbs, phy.ofdm_params(scs, prbs)[0]


def Rx_low_phy(td_slot, carrier_config):
    """rx_lowphy_process.py:35-98"""
    scs, prbs, nfft = _carrier(carrier_config)
    Nr = carrier_config["Nr"]
    td = np.asarray(td_slot)
    assert td.ndim == 2 and td.shape[0] == Nr and td.shape[1] >= 15 * nfft, \
        f"td_slot {td.shape}: (Nr = {Nr}, at least 15*{nfft} samples)"
    td = td[:, :15 * nfft]
    td = np.ascontiguousarray(td if td.dtype == np.complex64 else td.astype(np.complex128))
    t = _lib.require_gpu()
    grid = phy.ofdm_demod(t.from_numpy(td[None]).cuda(), scs, prbs, carrier_config["carrier_frequency_in_mhz"])
    return np.roll(grid[0].cpu().numpy(), Nr // 2, axis=0).astype(np.complex64)


def channel_filter(rx_waveform, carrier_config, sample_rate_in_hz):
    """rx_lowphy_process.py:100-164"""
    raise NotImplementedError("channel_filter: the FIR and half-band filters the reference designs with "
                              "scipy.signal.remez are not provided; filter and decimate to nfft*scs*1000 Hz first")


def waveform_rx_processing(rx_waveform, carrier_config, sample_rate_in_hz):
    """rx_lowphy_process.py:11-33"""
    raise NotImplementedError("waveform_rx_processing starts with channel_filter, which is not provided; pass the "
                              "filtered waveform's slots to phy.ofdm_demod (a (T, Nr, 15*nfft) view needs no copy)")
