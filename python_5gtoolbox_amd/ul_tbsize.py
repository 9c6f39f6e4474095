"""PUSCH transport block size, modulation order and target code rate (TS 38.214 §6.1.4) — drop-in for
py5gphy/nr_pusch/ul_tbsize.py:6-69, on the host.  The MCS tables are those of 38.214 (Tables 6.1.4.1-1,
6.1.4.1-2, 5.1.3.1-2, 5.1.3.1-3), written as runs of target code rates per modulation order, and the TBS
table is Table 5.1.3.2-1.

    TBSize, Qm, coderateby1024 = gen_tbsize(pusch_config)
"""
import math


def _table(*runs):
    return [(Qm, R) for Qm, rates in runs for R in rates]


# mcs_table name (upper case) -> (entries, number of leading entries whose order is q = 1 or 2)
_MCS = {
    "MCSTABLE61411": (_table((1, (240, 314)), (2, (193, 251, 308, 379, 449, 526, 602, 679)),
                             (4, (340, 378, 434, 490, 553, 616, 658)),
                             (6, (466, 517, 567, 616, 666, 719, 772, 822, 873, 910, 948))), 2),
    "MCSTABLE61412": (_table((1, (60, 80, 100, 128, 156, 198)), (2, (120, 157, 193, 251, 308, 379, 449, 526, 602, 679)),
                             (4, (378, 434, 490, 553, 616, 658, 699, 772)), (6, (567, 616, 666, 772))), 6),
    "256QAM": (_table((2, (120, 193, 308, 449, 602)), (4, (378, 434, 490, 553, 616, 658)),
                      (6, (466, 517, 567, 616, 666, 719, 772, 822, 873)),
                      (8, (682.5, 711, 754, 797, 841, 885, 916.5, 948))), 0),
    "64QAMLOWSE": (_table((2, (30, 40, 50, 64, 78, 99, 120, 157, 193, 251, 308, 379, 449, 526, 602)),
                          (4, (340, 378, 434, 490, 553, 616)), (6, (438, 466, 517, 567, 616, 666, 719, 772))), 0),
}
_CASE_SENSITIVE = {"MCSTABLE61411": "MCStable61411", "MCSTABLE61412": "MCStable61412"}   # the reference's spelling


def _tbs_table():
    """Table 5.1.3.2-1: steps of 8 up to 192, 16 to 384, 24 to 576, 32 to 768, then the listed sizes."""
    t = list(range(24, 193, 8)) + list(range(208, 385, 16)) + list(range(408, 577, 24)) + list(range(608, 769, 32))
    return t + [808, 848, 888, 928, 984, 1032, 1064, 1128, 1160, 1192, 1224, 1256, 1288, 1320, 1352, 1416, 1480, 1544, 1608,
                1672, 1736, 1800, 1864, 1928, 2024, 2088, 2152, 2216, 2280, 2408, 2472, 2536, 2600, 2664, 2728, 2792, 2856,
                2976, 3104, 3240, 3368, 3496, 3624, 3752, 3824]


_TBS = _tbs_table()
assert len(_TBS) == 93


def _get_Qm_coderate(mcs_table, mcs_index, nTpPi2BPSK):
    """38.214 §6.1.4.1 (ul_tbsize.py:71-122)."""
    key = mcs_table.upper()
    if key not in _MCS or (key in _CASE_SENSITIVE and mcs_table != _CASE_SENSITIVE[key]):
        raise NameError("wrong mcs table")
    rows, nq = _MCS[key]
    assert 0 <= mcs_index < len(rows), f"mcs_index {mcs_index} outside table {mcs_table} (0..{len(rows) - 1})"
    Qm, R = rows[mcs_index]
    if mcs_index < nq:          # q = 1 with tp-pi2BPSK, otherwise 2; the rate is the table's divided by q
        q = 2 - nTpPi2BPSK
        Qm, R = Qm * q, int(R / q)
    return Qm, R


def _get_NprbDmrs(DMRS, NrOfSymbols):
    """DMRS resource elements per PRB with the CDM groups without data, single-symbol DMRS of a mapping
    type A allocation (ul_tbsize.py:124-168)."""
    ctype, groups = DMRS["DMRSConfigType"], DMRS["NumCDMGroupsWithoutData"]
    assert ctype in [1, 2]
    assert groups in ([1, 2] if ctype == 1 else [1, 2, 3])
    per_symbol = groups * (6 if ctype == 1 else 4)
    assert DMRS["NrOfDMRSSymbols"] in [1, 2]
    assert DMRS["NrOfDMRSSymbols"] == 1, "double-symbol DMRS is not supported"
    add = DMRS["DMRSAddPos"]
    assert add in [0, 1, 2, 3]
    nsym = 1 if NrOfSymbols <= 7 else min(add, 1) + 1 if NrOfSymbols <= 9 else min(add, 2) + 1 if NrOfSymbols <= 11 else add + 1
    return nsym * per_symbol


def gen_tbsize(pusch_config):
    """38.214 §6.1.4.2 with N_oh = 0: -> (TBSize, Qm, coderateby1024)."""
    NL = pusch_config['num_of_layers']
    nPRB = pusch_config['ResAlloType1']['RBSize']
    NrOfSymbols = pusch_config['NrOfSymbols']
    Qm, R = _get_Qm_coderate(pusch_config['mcs_table'], pusch_config['mcs_index'], pusch_config['nTpPi2BPSK'])
    NRE = min(156, 12 * NrOfSymbols - _get_NprbDmrs(pusch_config["DMRS"], NrOfSymbols)) * nPRB
    Ninfo = NRE * R / 1024 * Qm * NL
    if Ninfo <= 3824:
        n = max(3, math.floor(math.log2(Ninfo)) - 6)
        Nq = max(24, (2 ** n) * math.floor(Ninfo / (2 ** n)))
        return [v for v in _TBS if v >= Nq][0], Qm, R
    n = math.floor(math.log2(Ninfo - 24)) - 5
    x = (Ninfo - 24) / (2 ** n)
    whole = math.floor(x)
    Nq = max(3840, (2 ** n) * (whole + 1 if x - whole >= 0.5 else whole))      # ties of the round go up (38.214)
    C = math.ceil((Nq + 24) / 3816) if R <= 256 else math.ceil((Nq + 24) / 8424) if Nq > 8424 else 1
    return 8 * C * math.ceil((Nq + 24) / (8 * C)) - 24, Qm, R
