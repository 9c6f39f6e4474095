"""Float64 numpy restatement of PUSCH transform precoding (python_5gtoolbox_amd/csrc/ldpc5g_tp.hip and
the low-PAPR DMRS source of ldpc5g_slot.hip):
the spreading DFT and its inverse (py5gphy/nr_pusch/nr_pusch_process.py:39-54, nr_pusch.py:170-194),
the low-PAPR sequence with the phase index reduced exactly in integers (common/lowPAPR_seq.py:5-41),
the group / sequence hopping (nr_pusch_dmrs.py:216-249), and the LS estimate and transmit map that
use them (nr_pusch_dmrs.py:66-101, 163-190).  It is the yardstick of the GPU tests; the generator
(tests/golden/gen_tp_golden.py) ties it to the reference's recorded outputs
(tests/golden/tp_golden_*.npz)."""
import glob
import os

import numpy as np

import slot_ref

CARRIER_PRB = slot_ref.CARRIER_PRB
HOPPING = ("neither", "groupHopping", "sequenceHopping")


def smooth235(n):
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


RB_SIZES = [n for n in range(1, 276) if smooth235(n)]   # the 53 allocations 2^a 3^b 5^c (38.211 6.3.1.4)


def pusch_config(rb_start, rb_size, port=1000, add_pos=0, hopping="neither", npuschid=77, num_ant=1, pmi=0,
                 mcs_index=5, mcs_table="256QAM", start=2, nsym=12):
    """A pusch_config with nTransPrecode = 1: slot_ref.pusch_config's keys (what the LS estimate reads)
    and the ones NrPUSCH.process / RX_process read on top (default_pusch_config.json supplies the
    rest in the generator)."""
    cfg = slot_ref.pusch_config(rb_start=rb_start, rb_size=rb_size, ports=[port], add_pos=add_pos, cdm=2,
                                start=start, nsym=nsym, num_ant=num_ant, pmi=pmi, trans_precode=1)
    cfg["DMRS"]["transformPrecodingEnabled"] = {"nPuschID": npuschid, "groupOrSequenceHopping": hopping}
    cfg.update(rnti=1, nNid=1, mcs_table=mcs_table, mcs_index=mcs_index, rv=[0], data_source=[], nTpPi2BPSK=0,
               period_in_slot=1, allocated_slots=[0])
    return cfg


# sequence cases: name -> (u, v, alpha, MZC); the short ones (tables in the reference) feed base_seq
SEQ_CASES = {
    "z30": (7, 0, 0.0, 30), "z36": (0, 0, 0.0, 36), "z72v0": (29, 0, 0.0, 72), "z72v1": (29, 1, 0.0, 72),
    "z120": (17, 1, 0.0, 120), "z1620": (13, 1, 0.0, 1620), "z96a": (4, 0, 2 * np.pi * 5 / 12, 96),
}
SHORT_U = (0, 13, 29)
SHORT_MZC = (6, 12, 18, 24)
# hopping table axes
HOP_IDS = (0, 29, 30, 77, 1007)
HOP_SLOTS = (0, 7, 19)
HOP_SYMS = (2, 5, 11)
# LS cases: name -> (config arguments, Nr, slot)
LS_CASES = {
    "R5": (dict(rb_start=3, rb_size=5, port=1001), 2, 3),                                   # M_ZC = 30, the closed form
    "R6": (dict(rb_start=0, rb_size=6), 2, 0),                                              # N_ZC = 31, smallest ZC
    "R16": (dict(rb_start=8, rb_size=16, add_pos=3, hopping="groupHopping"), 4, 19),        # 4 DMRS symbols, carrier edge
    "R20": (dict(rb_start=2, rb_size=20, port=1002, add_pos=1, hopping="sequenceHopping"), 1, 7),   # M_ZC = 120 >= 72
    "R2": (dict(rb_start=5, rb_size=2, npuschid=13), 2, 0),                                 # base_seq (u = 13)
}
# process / map cases: name -> (config arguments, num_ant, slot)
MAP_CASES = {
    "P5": (dict(rb_start=4, rb_size=5, add_pos=1, num_ant=1), 1, 2),
    "P18": (dict(rb_start=3, rb_size=18, add_pos=2, hopping="groupHopping", num_ant=2, pmi=4), 2, 9),
}
# end-to-end cases
E2E_CASES = {
    "E18": dict(cfg=dict(rb_start=3, rb_size=18, add_pos=1, hopping="groupHopping", mcs_index=5), Nr=2, slot=7),
    "E20": dict(cfg=dict(rb_start=2, rb_size=20, add_pos=1, hopping="sequenceHopping", mcs_index=9), Nr=2, slot=19),
}


def transform_precode(x, rb_size, inverse=False):
    """Every block of M = 12*rb_size along the last axis: np.fft in complex128, orthonormal."""
    M = 12 * rb_size
    x = np.asarray(x).astype(np.complex128)
    b = x.reshape(x.shape[:-1] + (x.shape[-1] // M, M))
    y = np.fft.ifft(b, axis=-1) * np.sqrt(M) if inverse else np.fft.fft(b, axis=-1) / np.sqrt(M)
    return y.reshape(x.shape)


def largest_prime_below(n):
    for p in range(n - 1, 1, -1):
        if all(p % d for d in range(2, int(p ** 0.5) + 1)):
            return p


def zc_q(NZC, u, v):
    """q = floor(qbar + 1/2) + v (-1)^floor(2 qbar), qbar = NZC (u + 1) / 31, in integers."""
    A = NZC * (u + 1)
    return (2 * A + 31) // 62 + v * (-1) ** ((2 * A) // 31)


def low_papr_seq(u, v, alpha, MZC):
    """gen_lowPAPR_seq for MZC = 30 and MZC >= 36 with the phase index reduced exactly."""
    assert MZC % 6 == 0 and MZC >= 30
    m = np.arange(MZC, dtype=np.int64)
    if MZC == 30:
        idx, den = ((u + 1) * (m + 1) * (m + 2)) % 62, 31
    else:
        den = largest_prime_below(MZC)
        n = m % den
        idx = (zc_q(den, u, v) * ((n * (n + 1)) % (2 * den))) % (2 * den)
    ph = np.pi * idx.astype(np.float64) / den
    return np.exp(1j * alpha * np.arange(MZC)) * (np.cos(ph) - 1j * np.sin(ph))


def hop_uv(npuschid, hopping, MZC, slot, sym):
    """(u, v) of _gen_seq_with_transform_precoding (nr_pusch_dmrs.py:216-249)."""
    fgh, v = 0, 0
    if hopping == "groupHopping":
        c = slot_ref.prbs(npuschid // 30, 8 * (14 * slot + sym) + 8)
        fgh = int(sum(int(c[8 * (14 * slot + sym) + i]) << i for i in range(8))) % 30
    elif hopping == "sequenceHopping" and MZC >= 72:
        v = int(slot_ref.prbs(npuschid, 14 * slot + sym + 1)[14 * slot + sym])
    return (fgh + npuschid) % 30, v


def tp_params(cfg):
    p = slot_ref.params(cfg)
    en = cfg["DMRS"]["transformPrecodingEnabled"]
    assert cfg["nTransPrecode"] == 1 and p["NL"] == 1 and p["cdm"] == 2
    return dict(p, npuschid=en["nPuschID"], hopping=en["groupOrSequenceHopping"], port=p["ports"][0])


def dmrs_seq(p, slot, sym, base_seq=None, m=0):
    if base_seq is not None:
        return np.asarray(base_seq, np.complex128)[m]
    MZC = 6 * p["rb_size"]
    u, v = hop_uv(p["npuschid"], p["hopping"], MZC, slot, sym)
    return low_papr_seq(u, v, 0.0, MZC)


def ls_est(grid, cfg, slot, base_seq=None):
    """H_LS (S, 3*rb_size, Nr, 1) complex128 of one slot grid (Nr, 14*carrier_re); base_seq (S, 6*rb_size)
    replaces the generated sequences."""
    p = tp_params(cfg)
    g = np.asarray(grid).astype(np.complex128)
    Nr, W = g.shape
    cre = W // 14
    out = np.zeros((len(p["syms"]), 3 * p["rb_size"], Nr, 1), np.complex128)
    d = (p["port"] // 2) % 2
    for m, sym in enumerate(p["syms"]):
        rc = dmrs_seq(p, slot, sym, base_seq, m).conj()
        a = sym * cre + 12 * p["rb_start"]
        for r in range(Nr):
            d0 = g[r, a + d:a + 12 * p["rb_size"]:4] * rc[0::2]
            d1 = g[r, a + d + 2:a + 12 * p["rb_size"]:4] * rc[1::2]
            out[m, :, r, 0] = ((d0 - d1) if p["port"] % 2 else (d0 + d1)) / (2 * slot_ref.scaling(p))
    return out


def data_re_idx(cfg):
    return slot_ref.data_re_idx(cfg)


def process(sym, rb_size, precoding=None):
    """nr_pusch_process after the modulator: the float64 DFT rounded to complex64, then the
    precoding product in float64 rounded once.  (num_ant, n) complex64."""
    y = transform_precode(np.asarray(sym, np.complex64), rb_size).astype(np.complex64)
    if precoding is None:
        return y[None]
    W = np.asarray(precoding, np.complex64).reshape(-1, 1).astype(np.complex128)
    return (W @ y[None].astype(np.complex128)).astype(np.complex64)


def tp_map(sym, cfg, slot, carrier_prb, num_ant, precoding=None, grid=None, base_seq=None):
    """The transmit grid (num_ant, 14*12*carrier_prb) complex64 from the MODULATED symbols: the DMRS
    as float32(scaling * r) and float32(+-scaling * r) on the port's comb, the data spread by
    `process`; the precoding product in float64, rounded once.  Only those REs are written."""
    p = tp_params(cfg)
    cre = 12 * carrier_prb
    g = np.zeros((num_ant, 14 * cre), np.complex64) if grid is None else grid
    W = np.eye(num_ant, 1) if precoding is None else np.asarray(precoding, np.complex64).reshape(-1, 1)[:num_ant]
    W = W.astype(np.complex128)

    def put(pos, x):
        g[:, pos] = (W @ x.astype(np.complex64)[None].astype(np.complex128)).astype(np.complex64)
    d = (p["port"] // 2) % 2
    sc = slot_ref.scaling(p)
    k = 4 * np.arange(3 * p["rb_size"])
    for m, s in enumerate(p["syms"]):
        r = dmrs_seq(p, slot, s, base_seq, m)
        a = s * cre + 12 * p["rb_start"]
        put(a + d + k, sc * r[0::2])
        put(a + d + 2 + k, sc * (1 - 2 * (p["port"] % 2)) * r[1::2])
    idx, _ = data_re_idx(cfg)
    n = 12 * p["rb_size"]
    pos = (idx // n) * cre + 12 * p["rb_start"] + idx % n
    put(pos, transform_precode(np.asarray(sym, np.complex64), p["rb_size"]))
    return g


def load_golden(gold_dir):
    out = {}
    for path in sorted(glob.glob(os.path.join(gold_dir, "tp_golden_*.npz"))):
        name = os.path.basename(path)[len("tp_golden_"):-4]
        with np.load(path) as d:
            out[name] = {k: d[k] for k in d.files}
    return out
