"""numpy restatement of UCI on PUSCH (TS 38.212 §5.3.3, §6.2.7; 38.211 §6.3.1.1), the yardstick of the
UCI tests: the small-block code, the §6.2.7 map built with per-RE flags, the separator in plain and
in descrambling mode, and the soft small-block decoder.  Checked against the recorded outputs of the
reference (tests/golden/uci_golden_*) by tests/test_uci_host.py; where the reference has no
counterpart (descrambling mode, erasure, soft decisions) this file is the definition.
"""
import json
import os

import numpy as np

ULSCH, ACK, CSI1, CSI2, NONE = 0, 1, 2, 3, 4
DATA, X, Y = 0, 1, 2
STREAMS = ("ulsch", "ack", "csi1", "csi2")

# TS 38.212 Table 5.3.3.3-1: bit k of ROWS[i] is M_{i,k}
ROWS = (0x403, 0x607, 0x749, 0x50d, 0x48f, 0x5d3, 0x755, 0x599, 0x69b, 0x65d, 0x6e5, 0x567, 0x7a9, 0x6ab, 0x4b1, 0x6f3,
        0x277, 0x139, 0x0fb, 0x061, 0x445, 0x60b, 0x591, 0x717, 0x3df, 0x4e3, 0x32d, 0x3af, 0x175, 0x1fd, 0x7ff, 0x001)

# name: RBSize, NrOfSymbols, StartSymbolIndex, DMRSAddPos, CDM groups, NL, mcs_index, OACK, OCSI1, OCSI2, options
CASES = {
    "A1": (2, 12, 2, 0, 2, 1, 5, 1, 0, 0, {}),
    "Q2": (2, 12, 2, 0, 2, 1, 1, 1, 0, 0, {}),
    "A2": (2, 12, 2, 1, 1, 1, 12, 2, 0, 0, {}),
    "A2C": (3, 14, 0, 1, 2, 2, 5, 2, 7, 0, {}),
    "SC5": (3, 14, 0, 1, 2, 1, 5, 2, 7, 0, {"UCIScaling": 0.5}),
    "A7": (3, 12, 2, 0, 2, 1, 5, 7, 0, 0, {}),
    "ALL": (4, 14, 0, 2, 2, 1, 12, 4, 11, 15, {}),
    "POL": (6, 14, 0, 1, 2, 2, 20, 12, 20, 40, {}),
    "BIG": (24, 14, 0, 1, 2, 1, 20, 20, 60, 400, {}),
    "U0a": (4, 14, 0, 1, 2, 1, 5, 2, 20, 0, {"EnableULSCH": 0}),
    "U0b": (4, 14, 0, 1, 2, 1, 5, 5, 20, 30, {"EnableULSCH": 0}),
}


def case_config(name):
    """The fields of pusch_config that the UCI code reads (no reference default file needed)."""
    RB, nsym, start, addpos, cdm, NL, mcs, oack, ocsi1, ocsi2, opt = CASES[name]
    cfg = {"ResAlloType1": {"RBStart": 0, "RBSize": RB}, "StartSymbolIndex": start, "NrOfSymbols": nsym,
           "DMRS": {"NumCDMGroupsWithoutData": cdm, "DMRSAddPos": addpos, "DMRSConfigType": 1, "NrOfDMRSSymbols": 1}, "num_of_layers": NL, "mcs_index": mcs,
           "mcs_table": "256QAM", "nTransPrecode": 0, "nTpPi2BPSK": 0, "UCIScaling": 1, "EnableULSCH": 1,
           "EnableACK": int(oack > 0), "NumACKBits": oack, "I_HARQ_ACK_offset": 9,
           "EnableCSI1": int(ocsi1 > 0), "NumCSI1Bits": ocsi1, "I_CSI1offset": 6,
           "EnableCSI2": int(ocsi2 > 0), "NumCSI2Bits": ocsi2, "I_CSI2offset": 6}
    cfg.update(opt)
    return cfg


def load_cases(gold_dir):
    """name -> dict(cfg, dmrs, Qm, coderateby1024, TBSize, ULSCH_size, Gtotal, rm, g_seq, ulsch, ack, csi1, csi2)."""
    with open(os.path.join(gold_dir, "uci_golden_cases.json")) as f:
        meta = json.load(f)
    d = np.load(os.path.join(gold_dir, "uci_golden_map.npz"))
    out = {}
    for name, m in meta["cases"].items():
        c = dict(m)
        c["cfg"] = case_config(name)
        for k in ("g_seq",) + STREAMS:
            c[k] = d[f"{name}_{k}"]
        out[name] = c
    return out


# ---------------------------------------------------------------------------- small-block code
def sb_N(K, Qm):
    return Qm if K == 1 else 3 * Qm if K == 2 else 32


def sb_kinds(K, Qm):
    """Kind (DATA / X / Y) of each of the N codeword positions."""
    N = sb_N(K, Qm)
    k = np.zeros(N, np.int8)
    if K == 1:
        k[1:2] = Y
        k[2:] = X
    elif K == 2:
        k[(np.arange(N) % Qm) >= 2] = X
    return k


def sb_encode(bits, Qm):
    """[T, K] 0/1 -> [T, N] int8 with the placeholders x = -1, y = -2 (§5.3.3)."""
    bits = np.atleast_2d(np.asarray(bits, np.int64))
    T, K = bits.shape
    N = sb_N(K, Qm)
    if K >= 3:
        M = np.array([[(r >> k) & 1 for k in range(K)] for r in ROWS])
        return ((bits @ M.T) & 1).astype(np.int8)
    out = np.zeros((T, N), np.int8)
    if K == 1:
        out[:, 0] = bits[:, 0]
        out[:, 1:2] = -2
        out[:, 2:] = -1
        return out
    c = np.stack([bits[:, 0], bits[:, 1], bits[:, 0] ^ bits[:, 1]], 1)
    nd = min(Qm, 2)
    for g in range(3):
        out[:, g * Qm + nd:(g + 1) * Qm] = -1
        for j in range(nd):
            out[:, g * Qm + j] = c[:, (nd * g + j) % 3]
    return out


def sb_encode_rm(bits, E, Qm):
    d = sb_encode(bits, Qm)
    return np.tile(d, (1, -(-E // d.shape[1])))[:, :E]


def sb_fold(llr, N):
    """Sum the repetitions of each of the N positions in ascending order, float64; unsent ones are 0."""
    llr = np.atleast_2d(np.asarray(llr, np.float64))
    f = np.zeros((llr.shape[0], N))
    for off in range(0, llr.shape[1], N):
        seg = llr[:, off:off + N]
        f[:, :seg.shape[1]] += seg
    return f


def sb_decode(llr, K, Qm):
    """Soft maximum-likelihood decision, ties to the smallest message read MSB first: [T, E] -> [T, K] int8."""
    N = sb_N(K, Qm)
    f = sb_fold(llr, N)
    T = f.shape[0]
    if K == 1:
        s = f[:, 0] + (f[:, 1] if Qm >= 2 else 0.0)
        return (s < 0).astype(np.int8)[:, None]
    if K == 2:
        nd = min(Qm, 2)
        S = np.zeros((T, 3))
        for g in range(3):          # ascending position within each of the three sums
            for j in range(nd):
                S[:, (nd * g + j) % 3] += f[:, g * Qm + j]
        msgs = np.array([[0, 0], [0, 1], [1, 0], [1, 1]])
        sg = 1 - 2 * np.stack([msgs[:, 0], msgs[:, 1], msgs[:, 0] ^ msgs[:, 1]], 1)
        return msgs[np.argmax(S @ sg.T, axis=1)].astype(np.int8)
    msgs = (np.arange(2 ** K)[:, None] >> (K - 1 - np.arange(K))) & 1          # message m, MSB first
    cw = 1.0 - 2.0 * sb_encode(msgs, Qm)
    return msgs[np.argmax(f @ cw.T, axis=1)].astype(np.int8)                   # argmax: first = smallest m


# ---------------------------------------------------------------------------- §6.2.7 map
def build_map(cfg, dmrs, rm, Qm, Gtotal):
    """-> dict(stream [G], index [G], kind [G], inv {name: t [len]}, punct {name: bool [len]}, lens).
    stream / index are the FINAL owner of g_seq position t (after step 5); inv maps each stream element to
    its position, and punct marks the elements that a 1-2 bit HARQ-ACK overwrites."""
    RB = cfg["ResAlloType1"]["RBSize"]
    start, nsym, NL = cfg["StartSymbolIndex"], cfg["NrOfSymbols"], cfg["num_of_layers"]
    dre = 6 if cfg["DMRS"]["NumCDMGroupsWithoutData"] == 1 else 0
    oack = cfg["EnableACK"] * cfg["NumACKBits"]
    ocsi1 = cfg["EnableCSI1"] * cfg["NumCSI1Bits"]
    ocsi2 = cfg["EnableCSI2"] * cfg["NumCSI2Bits"]
    q = NL * Qm
    M = RB * 12
    mul = [RB * dre if (start + L) in dmrs else M for L in range(nsym)]
    muci = [0 if (start + L) in dmrs else M for L in range(nsym)]
    assert Gtotal == sum(mul) * q
    uci_av = [np.arange(M) < muci[L] for L in range(nsym)]
    ul_av = [np.arange(M) < mul[L] for L in range(nsym)]
    rvd = [np.zeros(M, bool) for L in range(nsym)]
    owner = np.full((nsym, M), NONE, np.int8)
    first = np.zeros((nsym, M), np.int64)        # stream index of the RE's first bit
    over_s = np.full((nsym, M), NONE, np.int8)   # the stream that step 5 overwrites, and its first index
    over_first = np.zeros((nsym, M), np.int64)
    L1 = dmrs[0] + 1
    Lcsi = start + 1 if start in dmrs else start

    def spread(G, L, count_of, cand_of, full_of, take):
        n = 0
        while n < G:
            c = count_of(L)
            if c > 0:
                if G - n >= c * q:
                    d, m = 1, full_of(L)
                else:
                    d, m = (c * q) // (G - n), -(-(G - n) // q)
                cand = cand_of(L)
                take(L, cand[np.arange(m) * d], n)
                n += m * q
            L += 1

    if oack <= 2:
        def take1(L, ks, n):
            rvd[L][ks] = True
        spread(rm["Euci_ackrvd"], L1, lambda L: int(uci_av[L].sum()), lambda L: np.flatnonzero(ul_av[L]),
               lambda L: int(ul_av[L].sum()), take1)
    nrvd = [int(r.sum()) for r in rvd]

    def taker(s):
        def take(L, ks, n):
            owner[L][ks] = s
            first[L][ks] = n + np.arange(ks.size) * q
            uci_av[L][ks] = False
            ul_av[L][ks] = False
        return take

    if oack > 2:
        spread(rm["Euci_ack"], L1, lambda L: int(uci_av[L].sum()), lambda L: np.flatnonzero(uci_av[L]),
               lambda L: int(ul_av[L].sum()), taker(ACK))
    if ocsi1 > 0:
        L = Lcsi
        while int(uci_av[L].sum()) - nrvd[L] <= 0:
            L += 1
        spread(rm["Euci_CSI1"], L, lambda L: int(uci_av[L].sum()) - nrvd[L], lambda L: np.flatnonzero(uci_av[L] & ~rvd[L]),
               lambda L: int(uci_av[L].sum()) - nrvd[L], taker(CSI1))
    if ocsi2 > 0:
        L = Lcsi
        while int(uci_av[L].sum()) <= 0:
            L += 1
        spread(rm["Euci_CSI2"], L, lambda L: int(uci_av[L].sum()), lambda L: np.flatnonzero(uci_av[L]),
               lambda L: int(uci_av[L].sum()), taker(CSI2))
    n_ul = 0
    if cfg["EnableULSCH"] == 1:
        for L in range(nsym):
            ks = np.flatnonzero(ul_av[L])
            owner[L][ks] = ULSCH
            first[L][ks] = n_ul + np.arange(ks.size) * q
            n_ul += ks.size * q
    if oack in (1, 2):
        def take5(L, ks, n):
            over_s[L][ks] = owner[L][ks]
            over_first[L][ks] = first[L][ks]
            owner[L][ks] = ACK
            first[L][ks] = n + np.arange(ks.size) * q
        spread(rm["Euci_ack"], L1, lambda L: nrvd[L], lambda L: np.flatnonzero(rvd[L]), lambda L: nrvd[L], take5)
    # step 6: t runs over symbols, REs, then the NL * Qm bits of an RE
    st = np.concatenate([np.repeat(owner[L][:mul[L]], q) for L in range(nsym)])
    v = np.tile(np.arange(q), Gtotal // q)
    ix = np.concatenate([np.repeat(first[L][:mul[L]], q) for L in range(nsym)]) + v
    ovs = np.concatenate([np.repeat(over_s[L][:mul[L]], q) for L in range(nsym)])
    ovf = np.concatenate([np.repeat(over_first[L][:mul[L]], q) for L in range(nsym)]) + v
    ix[st == NONE] = 0
    lens = {"ulsch": n_ul, "ack": rm["Euci_ack"] if oack else 0, "csi1": rm["Euci_CSI1"] if ocsi1 else 0,
            "csi2": rm["Euci_CSI2"] if ocsi2 else 0}
    kind = np.zeros(Gtotal, np.int8)
    if oack in (1, 2):
        kk = sb_kinds(oack, Qm)
        a = st == ACK
        kind[a] = kk[ix[a] % kk.size]
    inv = {}
    for s, name in enumerate(STREAMS):
        t = np.full(lens[name], -1, np.int64)
        sel = np.flatnonzero(st == s)
        t[ix[sel]] = sel
        inv[name] = t
    punct = {name: np.zeros(lens[name], bool) for name in STREAMS}
    for s, name in enumerate(STREAMS):
        over = np.flatnonzero(ovs == s)
        inv[name][ovf[over]] = over
        punct[name][ovf[over]] = True
    for name in STREAMS:
        assert (inv[name] >= 0).all(), name
    return {"stream": st, "index": ix, "kind": kind, "inv": inv, "punct": punct, "lens": lens}


def mux(m, streams):
    """g_seq of data_control_multiplex from the four coded streams (dict name -> 1-D array)."""
    g = np.zeros(m["stream"].size, np.int8)
    for s, name in enumerate(STREAMS):
        sel = m["stream"] == s
        g[sel] = np.asarray(streams[name])[m["index"][sel]]
    return g


def prbs(cinit, n):
    """gen_nrPRBS: the Gold sequence of 38.211 §5.2.1."""
    x1 = np.zeros(1600 + n + 31, np.uint8)
    x2 = np.zeros(1600 + n + 31, np.uint8)
    x1[0] = 1
    for i in range(31):
        x2[i] = (cinit >> i) & 1
    for i in range(1600 + n):
        x1[i + 31] = x1[i + 3] ^ x1[i]
        x2[i + 31] = x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i]
    return (x1[1600:1600 + n] ^ x2[1600:1600 + n]).astype(np.int8)


def demux(m, llr, c=None, erase_punctured=False):
    """LLRs of one slot -> dict of the four streams.  c = None: the permutation of data_control_separate
    (input already descrambled).  c = PRBS bits: input in the scrambled domain; ordinary positions times
    1 - 2 c[t], a y position times 1 - 2 c[t - 1], an x position 0.  erase_punctured writes 0 where a
    1-2 bit HARQ-ACK overwrote the UL-SCH (or CSI part 2)."""
    llr = np.asarray(llr)
    out = {}
    for name in STREAMS:
        t = m["inv"][name]
        v = llr[t].copy()
        if c is not None:
            k = m["kind"][t] if name == "ack" else np.zeros(t.size, np.int8)
            cc = np.where(k == Y, c[np.maximum(t - 1, 0)], c[t])
            v = np.where(cc == 1, -v, v)
            v[k == X] = 0
        if erase_punctured:
            v[m["punct"][name]] = 0
        out[name] = v.astype(llr.dtype)
    return out


def scramble(g, c):
    """nr_pusch_process.py:14-25."""
    s = np.zeros(g.size, np.int8)
    for i in range(g.size):
        s[i] = 1 if g[i] == -1 else s[i - 1] if g[i] == -2 else (g[i] + c[i]) % 2
    return s
