"""ctypes binding of libldpc5g.so (include/ldpc5g.h) plus device-buffer helpers.

PyTorch-ROCm is used only for device memory and the current HIP stream; no torch ops run on
the hot path.  There is no CPU fallback: if the library or a GPU is missing, calls raise.
"""
import collections
import ctypes
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LDPC5G_LIB") or os.path.join(HERE, "libldpc5g.so")

F64, F32 = 0, 1
FLOODING, LAYERED = 0, 1
LLR_FULL = 1
RATE_MATCHED = 2   # LDPC5G_RATE_MATCHED: rate-recovered rows, untransmitted columns +0.0
ALGO_MS, ALGO_BP, ALGO_BF = 0, 1, 2
EBGN, EZC, ESIZE, EHIP = -1, -2, -3, -4
EQ_ALGO = {"ZF": 0, "ZF-IRC": 1, "MMSE": 2, "MMSE-IRC": 3}   # LDPC5G_EQ_*: nr_channel_eq.py:15-26
# nr_channel_eq.py:27-46 names -> (LDPC5G_ML_* algo, irc)
ML_ALGO = {"ML-soft": (0, 0), "ML-IRC-soft": (0, 1), "ML-hard": (1, 0), "ML-IRC-hard": (1, 1),
           "ML2-soft": (2, 0), "ML2-IRC-soft": (2, 1), "MMSE-ML": (3, 0), "MMSE-ML-IRC": (3, 1),
           "opt-rank2-ML": (4, 0), "opt-rank2-ML-IRC": (4, 1)}
# CE_config["CE_algo"] (nr_channel_estimation.py:117-124) -> LDPC5G_CE_*
CE_ALGO = {"DFT": 0, "DCT": 1, "DFT_symmetric": 2, "DCT_symmetric": 3}

# every symbol include/ldpc5g.h declares: name -> (restype, argtypes)
_c = ctypes
OPTIONAL = {"ldpc5g_dec_blocks_per_cu", "ldpc5g_split_timeouts"}
SIGNATURES = {
    "ldpc5g_find_ils": (_c.c_int, [_c.c_int32]),
    "ldpc5g_dec_blocks_per_cu": (_c.c_int, [_c.c_int32, _c.c_int32, _c.c_int32]),
    "ldpc5g_encode": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_int32,
                                 _c.c_int64, _c.c_int64, _c.c_void_p]),
    "ldpc5g_decode_ms": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                    _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_double,
                                    _c.c_double, _c.c_int32, _c.c_int32, _c.c_int64, _c.c_int64,
                                    _c.c_void_p]),
    "ldpc5g_decode_ms_host": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                         _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                         _c.c_double, _c.c_double, _c.c_int32, _c.c_void_p]),
    "ldpc5g_encode_host": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_int32,
                                      _c.c_void_p]),
    "ldpc5g_decode_ms_mixed": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_int32,
                                          _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int32,
                                          _c.c_double, _c.c_double, _c.c_int32, _c.c_int32,
                                          _c.c_void_p]),
    "ldpc5g_mixed_plan": (_c.c_int64, [_c.c_void_p, _c.c_int32, _c.c_int32, _c.c_void_p, _c.c_int64]),
    "ldpc5g_decode_ms_mixed_plan": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int32,
                                               _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int32,
                                               _c.c_double, _c.c_double, _c.c_int32, _c.c_int32,
                                               _c.c_void_p]),
    "ldpc5g_decode_bf": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                    _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                    _c.c_int64, _c.c_int64, _c.c_void_p]),
    "ldpc5g_bp_scratch_elems": (_c.c_int64, [_c.c_int32, _c.c_int32, _c.c_int32]),
    "ldpc5g_decode_bp": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                    _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                    _c.c_int32, _c.c_int64, _c.c_int64, _c.c_void_p]),
    "ldpc5g_sparse_scratch_bytes": (_c.c_int64, [_c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                                 _c.c_int32]),
    "ldpc5g_decode_sparse": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32,
                                        _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_int32,
                                        _c.c_double, _c.c_double, _c.c_void_p, _c.c_int64,
                                        _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                        _c.c_void_p]),
    "ldpc5g_crc": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32,
                              _c.c_void_p, _c.c_void_p]),
    "ldpc5g_sch_config": (_c.c_int, [_c.c_int32, _c.c_int32, _c.c_double, _c.c_int32, _c.c_int32,
                                     _c.c_int64, _c.c_int64, _c.c_void_p]),
    "ldpc5g_sch_segment": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int32, _c.c_void_p,
                                      _c.c_void_p, _c.c_void_p]),
    "ldpc5g_sch_ratematch": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_void_p,
                                        _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "ldpc5g_sch_encode": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                     _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                     _c.c_void_p]),
    "ldpc5g_sch_raterecover": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_int64, _c.c_void_p,
                                          _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_int32,
                                          _c.c_void_p]),
    "ldpc5g_sch_tb_check": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int32,
                                       _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                       _c.c_void_p, _c.c_void_p]),
    "ldpc5g_sch_decode": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_int64, _c.c_void_p, _c.c_int32,
                                     _c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_void_p,
                                     _c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_double,
                                     _c.c_double, _c.c_int32, _c.c_void_p, _c.c_int64,
                                     _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "ldpc5g_sch_demod_raterecover": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_int64, _c.c_void_p,
                                                _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int32,
                                                _c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_void_p,
                                                _c.c_int32, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "ldpc5g_sch_rx_scratch_elems": (_c.c_int64, [_c.c_void_p, _c.c_int32, _c.c_int32]),
    "ldpc5g_sch_rx_decode": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_int64, _c.c_void_p,
                                        _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int32,
                                        _c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_void_p,
                                        _c.c_int32, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                        _c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_double,
                                        _c.c_double, _c.c_int32, _c.c_void_p, _c.c_int64,
                                        _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "ldpc5g_sch_multi_sizes": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_void_p]),
    "ldpc5g_sch_encode_multi": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64,
                                           _c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_void_p,
                                           _c.c_void_p, _c.c_void_p]),
    "ldpc5g_sch_raterecover_multi": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_int64, _c.c_void_p,
                                                _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_int32,
                                                _c.c_void_p]),
    "ldpc5g_sch_multi_plan": (_c.c_int64, [_c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_int64]),
    "ldpc5g_sch_raterecover_multi_plan": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int32,
                                                     _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int32,
                                                     _c.c_void_p]),
    "ldpc5g_sch_decode_multi": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_int64, _c.c_void_p,
                                           _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_int32,
                                           _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int32,
                                           _c.c_double, _c.c_double, _c.c_int32, _c.c_void_p,
                                           _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                           _c.c_void_p]),
    "ldpc5g_prbs": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_int64, _c.c_void_p, _c.c_int64,
                               _c.c_void_p]),
    "ldpc5g_scramble_modulate": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64,
                                            _c.c_int32, _c.c_int64, _c.c_int32, _c.c_void_p,
                                            _c.c_int64, _c.c_void_p]),
    "ldpc5g_demod_descramble": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_int64, _c.c_void_p,
                                           _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int32,
                                           _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int32,
                                           _c.c_int64, _c.c_void_p]),
    "ldpc5g_equalize": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                   _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int64, _c.c_int64,
                                   _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                   _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "ldpc5g_ml_detect": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                    _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int64, _c.c_int64,
                                    _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                    _c.c_int32, _c.c_int32, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                    _c.c_int32, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                    _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "ldpc5g_ce_workspace_bytes": (_c.c_int64, [_c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                               _c.c_int32, _c.c_int32]),
    "ldpc5g_channel_estimate": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32,
                                           _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                           _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_int32,
                                           _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                           _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64,
                                           _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64,
                                           _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                           _c.c_void_p, _c.c_void_p]),
    "ldpc5g_to_compensate": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int32,
                                        _c.c_void_p, _c.c_int32, _c.c_int64, _c.c_int64, _c.c_int32,
                                        _c.c_int32, _c.c_void_p]),
    "ldpc5g_slot_rx_frontend": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int32,
                                           _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                           _c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_int32, _c.c_int32,
                                           _c.c_int32, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64,
                                           _c.c_void_p]),
    "ldpc5g_slot_map": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                   _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                   _c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_int32,
                                   _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "ldpc5g_transform_precode": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int32,
                                            _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_void_p]),
    "ldpc5g_low_papr_seq": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_double, _c.c_int32,
                                       _c.c_void_p, _c.c_void_p]),
    "ldpc5g_slot_rx_frontend_tp": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int32,
                                              _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                              _c.c_int32, _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_void_p,
                                              _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "ldpc5g_slot_map_tp": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                      _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                      _c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_int32, _c.c_int32,
                                      _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "ldpc5g_ofdm_demod": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int64,
                                     _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                     _c.c_int64, _c.c_void_p]),
    "ldpc5g_ofdm_mod": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                   _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                   _c.c_int32, _c.c_int64, _c.c_void_p]),
    "ldpc5g_polar_plan": (_c.c_int64, [_c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                       _c.c_int32, _c.c_void_p, _c.c_int64]),
    "ldpc5g_polar_encode": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64,
                                       _c.c_int32, _c.c_void_p]),
    "ldpc5g_polar_rate_match": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                           _c.c_int64, _c.c_int32, _c.c_int32, _c.c_void_p]),
    "ldpc5g_polar_rate_recover": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                             _c.c_int64, _c.c_int32, _c.c_int32, _c.c_double, _c.c_int32,
                                             _c.c_void_p]),
    "ldpc5g_polar_decode": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64,
                                       _c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_void_p]),
    "ldpc5g_uci_rm_info": (_c.c_int, [_c.c_int32, _c.c_int32, _c.c_int32, _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_int32,
                                      _c.c_double, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32,
                                      _c.c_int32, _c.c_int32, _c.c_double, _c.c_int64, _c.c_void_p]),
    "ldpc5g_uci_map_plan": (_c.c_int64, [_c.c_int32, _c.c_int32, _c.c_int32, _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_int32,
                                         _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int64,
                                         _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int64]),
    "ldpc5g_uci_mux": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                  _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int32, _c.c_void_p]),
    "ldpc5g_uci_demux": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_int64, _c.c_void_p, _c.c_int64,
                                    _c.c_int32, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64,
                                    _c.c_void_p, _c.c_int64, _c.c_int32, _c.c_void_p]),
    "ldpc5g_uci_scramble_modulate": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int32, _c.c_int64,
                                                _c.c_int32, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "ldpc5g_smallblock_encode": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_void_p, _c.c_int64,
                                            _c.c_int32, _c.c_int32, _c.c_void_p]),
    "ldpc5g_smallblock_decode": (_c.c_int, [_c.c_void_p, _c.c_int32, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32,
                                            _c.c_void_p, _c.c_int64, _c.c_int32, _c.c_void_p]),
    "ldpc5g_pack_records": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int32, _c.c_int64,
                                       _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                       _c.c_void_p]),
    "ldpc5g_unpack_records": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int32, _c.c_int64,
                                         _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                         _c.c_int64, _c.c_void_p]),
    "ldpc5g_split_timeouts": (_c.c_int, [_c.c_void_p]),
    "ldpc5g_last_error": (_c.c_char_p, []),
    "ldpc5g_version": (_c.c_char_p, []),
}


class CbDesc(ctypes.Structure):
    """ldpc5g_cb_desc_t"""
    _fields_ = [("bgn", ctypes.c_int32), ("Zc", ctypes.c_int32),
                ("llr_off", ctypes.c_int64), ("ck_off", ctypes.c_int64)]


CRC_IDS = {"6": 0, "11": 1, "16": 2, "24A": 3, "24B": 4, "24C": 5}


class SchCfg(ctypes.Structure):
    """ldpc5g_sch_cfg_t"""
    _fields_ = [(n, ctypes.c_int32) for n in
                ("A", "B", "tb_crc_poly", "bgn", "C", "cbz", "Lcb", "F", "K", "K_apo", "Zc", "N",
                 "Ncb", "k0", "Qm", "NL", "rv", "E_lo", "E_hi", "c_switch")] + \
               [("G", ctypes.c_int64), ("E_total", ctypes.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class LdpcLibError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libldpc5g.so (raises LdpcLibError if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LdpcLibError(
                f"{LIB_PATH} is missing: build it with `python -m python_5gtoolbox_amd.build` "
                "(there is no CPU fallback for the LDPC hot path)")
        h = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if name in OPTIONAL and not hasattr(h, name):
                continue   # diagnostics absent from an older library (A/B builds)
            f = getattr(h, name)
            f.restype = res
            f.argtypes = args
        _lib = h
    return _lib


def check(rc):
    """Map a negative return code to the reference's error behaviour (AssertionError for
    argument errors, as its `assert` checks) or LdpcLibError for HIP failures."""
    if rc == 0:
        return
    msg = lib().ldpc5g_last_error().decode()
    if rc in (EBGN, EZC, ESIZE):
        raise AssertionError(msg)
    raise LdpcLibError(f"libldpc5g error {rc}: {msg}")


_torch = None


def torch():
    global _torch
    if _torch is None:
        import torch as t
        _torch = t
    return _torch


def require_gpu():
    t = torch()
    if not t.cuda.is_available():
        raise LdpcLibError("no ROCm GPU visible: the LDPC engine runs only on the GPU "
                           "(no CPU fallback)")
    return t


def stream_ptr(device=None):
    t = torch()
    return ctypes.c_void_p(t.cuda.current_stream(device).cuda_stream)


def ptr(tensor):
    return ctypes.c_void_p(tensor.data_ptr())


_tls = threading.local()
STAGING_MAX = int(os.environ.get("LDPC5G_STAGING_MAX", "32"))


def staging(key, make):
    """Per-thread cache of pinned-host / device buffers for the per-codeblock drop-ins (the
    reference's callers decode one codeblock per call, sim_ldpc_internal.py:51-58): a call then
    costs one pinned H2D copy, the launch and one D2H copy, with no allocation.  Bounded: at most
    STAGING_MAX entries per thread, least recently used evicted (a sweep over MCS / TBS / PRB
    configurations keeps only the recent ones; an evicted buffer is freed when its last user drops
    it — torch's allocators order the reuse after the stream work that used it)."""
    d = getattr(_tls, "bufs", None)
    if d is None:
        d = _tls.bufs = collections.OrderedDict()
    b = d.get(key)
    if b is None:
        b = d[key] = make()
        while len(d) > STAGING_MAX:
            d.popitem(last=False)
    else:
        d.move_to_end(key)
    return b


def staging_entries():
    """Number of cached staging entries of this thread."""
    return len(getattr(_tls, "bufs", ()))


def to_device(a, key):
    """numpy array -> device tensor through a per-thread cached pinned buffer (the drop-ins'
    host inputs; pageable copies measured milliseconds per call).  The device buffer is reused by
    the next call with the same key and shape: callers synchronise (to_host) before returning."""
    t = torch()
    a = np.ascontiguousarray(a)
    dev = t.cuda.current_device()
    tdt = t.from_numpy(a[:0] if a.ndim else a.reshape(1)[:0]).dtype

    def make():
        return (t.empty(a.shape, dtype=tdt, pin_memory=True), t.empty(a.shape, dtype=tdt, device=dev))
    hin, din = staging((key, "in", dev, a.shape, a.dtype.str), make)
    hin.numpy()[...] = a
    din.copy_(hin, non_blocking=True)
    return din


def to_host(x, key):
    """device tensor -> numpy copy through a per-thread cached pinned buffer; synchronises."""
    t = torch()
    dev = x.device.index if x.device.index is not None else t.cuda.current_device()
    hout = staging((key, "out", dev, tuple(x.shape), str(x.dtype)),
                   lambda: t.empty(tuple(x.shape), dtype=x.dtype, pin_memory=True))
    hout.copy_(x, non_blocking=True)
    t.cuda.current_stream().synchronize()
    return hout.numpy().copy()


def split_timeouts():
    """Codeblocks of the current device whose multi-workgroup float64 decode gave up waiting for
    its parts to be co-resident (status 0, iters -1; include/ldpc5g.h ldpc5g_split_timeouts)."""
    n = ctypes.c_uint32(0)
    check(lib().ldpc5g_split_timeouts(ctypes.byref(n)))
    return int(n.value)
