"""Drop-in for py5gphy/common/nr_slot.py: the host-side carrier tables and slot initialisation the
reference's simulations read (no GPU work here)."""
import numpy as np

REusage_types = {0: 'empty',
                 10: 'SSB',
                 11: 'SSB-PRB-RSV',
                 15: 'CSI-RS',
                 16: 'CSI-RS-RSV',
                 20: 'CORESET',
                 21: 'PDCCH-DMRS',
                 22: 'PDCCH-DATA',
                 30: 'PDSCH-DMRS-RSV',
                 31: 'PDSCH-DMRS',
                 32: 'PDSCH-DATA',
                 40: 'SRS',
                 50: 'PUCCH-DATA',
                 51: 'PUCCH-DMRS',
                 60: 'PUSCH-DMRS-RSV',
                 61: 'PUSCH-DMRS',
                 62: 'PUSCH-DATA',
                 63: 'PUSCH-ULSCH',
                 64: 'PUSCH-HARQ-ACK',
                 65: 'PUSCH-HARQ-ACK-RSV',
                 66: 'PUSCH-CSI1',
                 67: 'PUSCH-CSI2',
                 }

# 38.101-1 Table 5.3.2-1: transmission bandwidth configuration N_RB, BW in MHz -> PRBs
_PRBS = {15: {5: 25, 10: 52, 15: 79, 20: 106, 25: 133, 30: 160, 35: 188, 40: 216, 45: 242, 50: 270},
         30: {5: 11, 10: 24, 15: 38, 20: 51, 25: 65, 30: 78, 35: 92, 40: 106, 45: 119, 50: 133,
              60: 162, 70: 189, 80: 217, 90: 245, 100: 273}}


def init_fd_slot(num_of_ant, carrier_prbsize):
    """(fd_slot_data, RE_usage_inslot): num_of_ant x (14*12*carrier_prbsize) zeros, complex64 and int8."""
    fd_slot_data = np.zeros((num_of_ant, 14 * 12 * carrier_prbsize), 'c8')
    RE_usage_inslot = np.zeros([num_of_ant, 14 * 12 * carrier_prbsize], 'i1')
    return fd_slot_data, RE_usage_inslot


def get_REusage_type(value):
    assert value in REusage_types
    return REusage_types[value]


def get_REusage_value(type):
    assert type in REusage_types.values()
    return next(k for k, v in REusage_types.items() if v == type)


def get_carrier_prb_size(scs, BW):
    """Carrier PRBs; as the reference, every scs other than 15 reads the 30 kHz column."""
    return _PRBS[15 if scs == 15 else 30][BW]


def get_FFT_IFFT_size(carrier_prb_size):
    """2 ** ceil(log2(12 * prbs / 0.85)): room for the channel filter's transition band."""
    return int(2 ** np.ceil(np.log2(carrier_prb_size * 12 / 0.85)))


def get_symbol_timing_offset(scs):
    """(seconds, samples) from the slot's start to each symbol's data part, at 30.72 MHz / 2048 points
    (scs 15) or 122.88 MHz / 4096 points (otherwise)."""
    if scs == 15:
        cps, n, rate = [160] + [144] * 6 + [160] + [144] * 6, 2048, 30.72 * 10 ** 6
    else:
        cps, n, rate = [352] + [288] * 13, 4096, 122.88 * 10 ** 6
    symbols_sample_offset_list = np.zeros(14)
    offset = 0
    for m in range(14):
        offset += cps[m]
        symbols_sample_offset_list[m] = offset
        offset += n
    return symbols_sample_offset_list / rate, symbols_sample_offset_list


def get_sample_rate_and_CP_size(scs, BW):
    """(sample rate in Hz, the 14 CP lengths in samples)."""
    fftsize = get_FFT_IFFT_size(get_carrier_prb_size(scs, BW))
    if scs == 15:
        CPs = np.array([160] + [144] * 6 + [160] + [144] * 6) * fftsize / 2048
    else:
        CPs = np.array([352] + [288] * 13) * fftsize / 4096
    return fftsize * scs * 1000, [int(x) for x in CPs]
