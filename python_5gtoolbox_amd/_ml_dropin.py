"""Shared body of the per-resource-element ML drop-ins (ML.py, ML2.py, MMSE_ML.py,
opt_rank2_ML.py): one RE through phy.ml_detect, results as the reference returns them."""
import numpy as np

from . import _lib, phy


def detect(Y, H, cov, modtype, algo):
    """-> (s_est complex64 (NL,), noise_var float64 (NL,), de_hardbits int64 (NL*Qm,),
    LLR_a float64 (NL*Qm,))"""
    H = np.asarray(H)
    assert H.ndim == 2
    Nr, NL = H.shape
    Y = np.asarray(Y)
    cov = np.asarray(cov)
    assert Nr >= NL
    assert Nr == Y.size
    assert cov.ndim == 2 and Nr == cov.shape[0] and Nr == cov.shape[1]
    assert modtype in phy.MOD_ID, f"modtype {modtype!r}"
    t = _lib.require_gpu()

    def dev(a, shape):
        return t.from_numpy(np.array(a, dtype=np.complex128).reshape(shape)).cuda()
    llr, sym, nv, hb = phy.ml_detect(dev(Y, (1, 1, Nr)), dev(H, (1, 1, Nr, NL)), dev(cov, (1, 1, Nr, Nr)),
                                     phy.MOD_ID[modtype], algo, re_per_cov=1,
                                     want=("sym", "noise_var", "hardbits"))
    return (sym[0].cpu().numpy(), nv[0].cpu().numpy(), hb[0].cpu().numpy().astype(np.int64),
            llr[0].cpu().numpy())
