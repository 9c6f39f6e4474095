"""Drop-in for py5gphy/common/lowPAPR_seq.py: the low-PAPR sequences of 38.211 5.2.2 on the GPU
(ldpc5g_low_papr_seq: the phase index reduced exactly in integers, one sincospi per element).

    gen_lowPAPR_seq(u, v, alpha, MZC) -> (MZC,) complex128

M_ZC in {6, 12, 18, 24} are the phi tables of 38.211 5.2.2.2, which are not provided:
NotImplementedError.
"""
from . import phy


def gen_lowPAPR_seq(u, v, alpha, MZC):
    """lowPAPR_seq.py:5-41"""
    assert u in range(30)
    assert MZC % 6 == 0
    if 6 <= MZC <= 60:
        assert v == 0
    elif MZC >= 72:
        assert v in [0, 1]
    return phy.low_papr_seq(int(u), int(v), MZC, alpha)[0].cpu().numpy()
