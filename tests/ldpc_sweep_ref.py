"""Inputs of the all-lifting-sizes LDPC sweep (tests/test_gpu_ldpc_sweep.py), shared with the CPU
check that those inputs can tell a right decoder from a wrong one (tests/test_ldpc_sweep_inputs.py),
and the loader of the mid-size reference fixtures (tests/golden/decode_midzc_golden.npz).

One recipe throughout (sweep_input): a generator seeded from (bg, Zc, path tag), random information
bits, O.encode, BPSK + AWGN with one SNR per codeblock, LLR = 2y / sigma^2 cast to the path's dtype.
The SNRs are uniform over a per-base-graph range that straddles the waterfall of L = 8 normalised
min-sum at every lifting size, and stratified: row k of B draws from the k-th of B equal slices of
the range (rows then shuffled), so even a 5-codeblock launch has a codeblock from both ends.  An
input with a zeroed tail (the rate-matched variants) carries fewer transmitted bits, so its range is
moved up by the rate change, 10 log10(n / (n - zeroed)) dB, plus 0.5 dB."""
import os
import zlib

import numpy as np

from oracle import ldpc_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ZLIST = list(O.ZLIST)
PAIRS = [(bg, Zc) for bg in (1, 2) for Zc in ZLIST]
MID = [z for z in ZLIST if 96 < z < 384]
L, ALPHA, BETA = 8, 0.75, 0.0
SNR_RANGE = {1: (-3.0, 3.0), 2: (-6.0, 1.0)}     # dB
DIMS = {1: (22, 66, 68, 46), 2: (10, 50, 52, 42)}   # Kb, N / Zc, Nf / Zc, Mb


def pair_id(p):
    return "bg%d-z%d" % p


def wg_codeblocks(Zc, layered):
    """Codeblocks per workgroup (ldpc5g_common.h dec_G): 768 threads layered, 384 flooding."""
    return max((768 if layered else 384) // Zc, 1)


def batch_size(Zc, layered):
    """Full workgroups, then a last one that holds a single codeblock; at least 5 codeblocks."""
    return max(2 * wg_codeblocks(Zc, layered) + 1, 5)


def split_serves(bg, Zc):
    """Sizes the multi-workgroup float64 kernel takes at all (ldpc5g_dec_split.hip split_wanted)."""
    return Zc >= 64 and not (bg == 2 and Zc <= 64)


def f64_batch_size(bg, Zc):
    """A float64 flooding batch that the split kernel does not take.  split_wanted(bgn, B, Zc)
    accepts a launch when B * w1 <= maxwg or B * w2 <= maxwg, with wR = split_parts(bgn, Zc, R) =
    ceil(MB * ceil(Zc / 64) / (16 R)) workgroups per codeblock and maxwg = min(kSplitMaxWG,
    7/8 of the CUs) <= 224 on any device.  w2 <= w1, so B * w2 > 224, i.e. B >= 224 // w2 + 1,
    rules both out wherever the launch runs: 75 codeblocks at Zc 104 ... 128, 25 at 352 / 384."""
    B = batch_size(Zc, False)
    if split_serves(bg, Zc):
        w2 = -(-DIMS[bg][3] * -(-Zc // 64) // 32)
        B = max(B, 224 // w2 + 1)
    return B


def n_zeroed(Zc):
    """Extension columns zeroed in the rate-matched variants: differs with the lifting size, so
    the cut falls on different rows of the dead-row groups across the sweep."""
    return 5 + ZLIST.index(Zc) % 20


def row_groups(bg):
    """[(first row, end row)] of the decoders' barrier groups, restated from the base graph:
    consecutive base rows whose core columns (the Kb + 4 of degree > 1) are disjoint
    (ldpc5g_dec_body.h RowGroups).  The structure is the same at every lifting size."""
    g = O.graph(bg, 2)
    cols = [set(int(j) for j in g.bj[g.rs[i]:g.rs[i + 1]] if j < g.Kcore) for i in range(g.Mb)]
    starts, seen = [0], set(cols[0])
    for i in range(1, g.Mb):
        if seen & cols[i]:
            starts.append(i)
            seen = set()
        seen |= cols[i]
    return list(zip(starts, starts[1:] + [g.Mb]))


def dead_rows(bg, nzero):
    """Base rows whose degree-1 extension column (row i owns column Kb + i) is among the last
    nzero columns: the rows that rate_matched=True skips when those columns are +0.0."""
    Mb = DIMS[bg][3]
    return set(range(Mb - nzero, Mb))


def sweep_input(bg, Zc, tag, B, dtype, nzero=0, snr_range=None):
    """(ck (B, K) int8, llr (B, N) dtype) of the sweep recipe; nzero: trailing columns set to +0.0."""
    rng = np.random.default_rng([bg, Zc, zlib.crc32(tag.encode())])
    Kb = DIMS[bg][0]
    ck = rng.integers(0, 2, (B, Kb * Zc)).astype(np.int8)
    dn = O.encode(ck, bg)
    lo, hi = snr_range or SNR_RANGE[bg]
    if nzero and snr_range is None:   # fewer transmitted bits: the waterfall moves up with the rate
        up = 10 * np.log10(DIMS[bg][1] / (DIMS[bg][1] - nzero)) + 0.5
        lo, hi = lo + up, hi + up
    snr = lo + (hi - lo) * (rng.permutation(B) + rng.random(B)) / B
    snr = snr[:, None]
    llr = (2 * ((1 - 2 * dn) + rng.normal(size=dn.shape) * 10 ** (-snr / 20)) / 10 ** (-snr / 10)).astype(dtype)
    if nzero:
        llr[:, -nzero * Zc:] = 0.0
    return ck, llr


def oracle_decode(llr, bg, Zc, schedule, alpha=ALPHA, beta=BETA, iters=L):
    if schedule == "layered":
        return O.decode_layered(llr, Zc, bg, iters, alpha, beta)
    return O.decode_flooding(llr, Zc, bg, iters, alpha, beta, llr.dtype.type)


def load_midzc_cases(algo=None):
    """[dict(bg, Zc, algo, L, alpha, beta, nzero, llr float64[N], ck int8[Nf], status)]: the
    reference's nr_decode_ldpc on quarter-step LLRs (stored as int8 q, llr = q / 4) at the lifting
    sizes 104 ... 352 and BG2 Zc = 384 (tests/golden/gen_midzc_golden.py)."""
    d = np.load(os.path.join(GOLD, "decode_midzc_golden.npz"))
    out = []
    for i in range(d["bg"].size):
        bg, Zc = int(d["bg"][i]), int(d["Zc"][i])
        if algo is not None and str(d["algo"][i]) != algo:
            continue
        Nf = DIMS[bg][2] * Zc
        out.append(dict(bg=bg, Zc=Zc, algo=str(d["algo"][i]), L=int(d["L"][i]), alpha=float(d["alpha"][i]),
                        beta=float(d["beta"][i]), nzero=int(d["nzero"][i]),
                        llr=d["q"][d["q_off"][i]:d["q_off"][i + 1]].astype(np.float64) / 4,
                        ck=np.unpackbits(d["ck_bits"][d["ck_off"][i]:d["ck_off"][i + 1]])[:Nf].astype(np.int8),
                        status=bool(d["status"][i])))
    return out
