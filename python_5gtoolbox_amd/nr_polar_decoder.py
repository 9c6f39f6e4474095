"""Polar decoding — drop-in for py5gphy/polar/nr_polar_decoder.py:12-67.

nr_decode_polar runs one block through `ldpc5g_polar_decode` (SC, or the reference's CA-PC-SCL
variant; the optionB names are the same arithmetic and are accepted as aliases) and
returns the reference's (ck, status), `[-1], False` on failure."""
import numpy as np

from . import _lib, _polar_dropin as D, crc, polar


def nr_decode_polar(algo, LLRin, E, K, L, nMax, iIL, CRCLEN=24, padCRC=0, rnti=0):
    if algo not in polar.ALGOS:
        assert 0
    LLRin = np.asarray(LLRin, np.float64)
    if polar.ALGOS[algo] == polar.SC:
        assert [nMax, iIL] in [[9, 1], [10, 0]]
        p = polar.plan(K, E, nMax, iIL, D.crclen_of(K, nMax))
    else:
        assert [nMax, iIL, CRCLEN] in [[9, 1, 24], [10, 0, 6], [10, 0, 11]]
        p = polar.plan(K, E, nMax, iIL, CRCLEN, padCRC, rnti)
    assert LLRin.size == p.N
    ck, status, _ = polar.decode(D.dev(LLRin, np.float64, "polar_dec"), p, algo, L if polar.ALGOS[algo] else 1)
    if not int(_lib.to_host(status, "polar_dec_st")[0]):
        return [-1], False
    return _lib.to_host(ck, "polar_dec_ck")[0].astype("i1"), True


def for_test_5g_polar_encoder(K, E, nMax, iIL, snr_db=8, CRCLEN=24, padCRC=0, rnti=0):
    """K information bits, CRC attached here: -> (LLRin, encodedbits, blkandcrc), E = N expected."""
    from . import nr_polar_encoder
    inbits = np.random.randint(2, size=K)
    poly = {6: '6', 11: '11', 24: '24C'}[CRCLEN]
    if padCRC == 0:
        blkandcrc = crc.nr_crc_encode(inbits, poly)
    else:
        inbits = np.concatenate((np.ones(24, 'i1'), inbits))
        blkandcrc = crc.nr_crc_encode(inbits, poly, rnti)[24:]
    encodedbits = nr_polar_encoder.encode_polar(blkandcrc, E, nMax, iIL)
    fn = (1 - 2 * encodedbits) + np.random.normal(0, 10 ** (-snr_db / 20), encodedbits.size)
    return 2 * fn / 10 ** (-snr_db / 10), encodedbits, blkandcrc
