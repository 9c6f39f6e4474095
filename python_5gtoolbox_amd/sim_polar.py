"""Batched polar BLER simulation — the reference's scripts/internal/sim_polar_internal.py:10-68 with
every trial of a stopping-rule stage in one launch.

A test case is the reference's [K, N, nMax, iIL, CRCLEN, padCRC, rnti]: K information bits BEFORE the
CRC, E = N, no rate matching, BPSK over AWGN with sigma^2 = 10^(-snr/10) and LLR = 2 y / sigma^2, as
for_test_5g_polar_encoder does.  Blocks, noise and LLRs are drawn on the device from one seeded
generator per point; a block counts as failed unless the decoder reports success with the sent bits.
"""
import pickle

import numpy as np

from . import _lib, crc, polar

STAGES = ((200, 10), (400, 5), (800, 2), (2000, 0))   # stop at `count` trials with >= `errors` failures


def _crc_matrix(A, crclen, padCRC, rnti):
    """CRC bits of a block = bits @ M (mod 2) xor const: the CRC is linear in the block."""
    poly = {6: "6", 11: "11", 24: "24C"}[crclen]
    pad = 24 if padCRC else 0
    t = crc._pos_table(poly, pad + A).astype(np.int64)
    M = ((t[pad:, None] >> (crclen - 1 - np.arange(crclen))[None, :]) & 1).astype(np.float64)
    const = int(np.bitwise_xor.reduce(t[:pad])) if pad else 0
    const ^= (rnti & ((1 << crclen) - 1)) if padCRC else 0   # nr_polar_decoder.py:49-55 masks only with padCRC
    return M, np.array([(const >> (crclen - 1 - c)) & 1 for c in range(crclen)], np.int8)


def draw(testcase, snr_db, n, gen):
    """n blocks with CRC and their LLRs on gen's device: -> (plan, blk [n, K + CRCLEN] int8, llr [n, N] float64)."""
    t = _lib.require_gpu()
    A, N, nMax, iIL, crclen, padCRC, rnti = testcase
    p = polar.plan(A + crclen, N, nMax, iIL, crclen, padCRC, rnti)
    assert p.N == N, f"test case {testcase}: E = {N} gives N = {p.N}"
    M, const = _crc_matrix(A, crclen, padCRC, rnti)
    dev = gen.device
    bits = t.randint(0, 2, (n, A), generator=gen, device=dev, dtype=t.int8)
    par = (bits.to(t.float64) @ t.from_numpy(M).to(dev)).to(t.int64) & 1
    blk = t.cat((bits, (par ^ t.from_numpy(const.astype(np.int64)).to(dev)).to(t.int8)), dim=1)
    x = 1.0 - 2.0 * polar.encode(blk, p).to(t.float64)
    sigma2 = 10.0 ** (-snr_db / 10.0)
    y = x + t.randn((n, N), generator=gen, device=dev, dtype=t.float64) * sigma2 ** 0.5
    return p, blk, 2.0 * y / sigma2


def bler_fixed(testcase, algo, L, snr_db, n, seed=0, device=None):
    """(failures, n) over exactly n trials."""
    t = _lib.require_gpu()
    gen = t.Generator(device=device if device is not None else f"cuda:{t.cuda.current_device()}")
    gen.manual_seed(seed)
    return _run(testcase, algo, L, snr_db, n, gen), n


def _run(testcase, algo, L, snr_db, n, gen):
    p, blk, llr = draw(testcase, snr_db, n, gen)
    ck, st, _ = polar.decode(llr, p, algo, L)
    good = (st == 1) & (ck == blk).all(dim=1)
    return int(n - int(good.sum()))


def bler_point(testcase, algo, L, snr_db, seed=0, device=None):
    """(bler, trials) under the reference's stopping rule: 200 / 400 / 800 / 2000 trials with at least
    10 / 5 / 2 / 0 failures."""
    t = _lib.require_gpu()
    gen = t.Generator(device=device if device is not None else f"cuda:{t.cuda.current_device()}")
    gen.manual_seed(seed)
    done = failed = 0
    for count, errors in STAGES:
        failed += _run(testcase, algo, L, snr_db, count - done, gen)
        done = count
        if failed >= errors:
            break
    return failed / done, done


def run_polar_simulation(testcase_list, algo_list, L_list, snr_db_list, filename, seed=0):
    """The reference's sweep and pickle layout: [testcase_list, snr_db_list, [[[algo, L, testcase],
    [snr, bler], ...], ...]]."""
    results = []
    for testcase in testcase_list:
        for algo in algo_list:
            for L in ([1] if algo in ("SC", "SC_optionB") else L_list):
                row = [[algo, L, testcase]]
                for snr_db in snr_db_list:
                    bler, _ = bler_point(testcase, algo, L, snr_db, seed=seed)
                    seed += 1
                    row.append([snr_db, bler])
                results.append(row)
    with open(filename, "wb") as handle:
        pickle.dump([testcase_list, snr_db_list, results], handle, protocol=pickle.HIGHEST_PROTOCOL)
    return results
