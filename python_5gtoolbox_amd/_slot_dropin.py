"""Shared body of the slot front end's drop-ins (nr_pdsch_dmrs.py, nr_pusch_dmrs.py,
nrpdsch_resource_mapping.py): one slot through phy.slot_frontend, results as the reference returns
them (numpy complex64)."""
import numpy as np

from . import _lib, phy


def _device_grid(fd_slot_data, slot):
    t = _lib.require_gpu()
    g = np.asarray(fd_slot_data)   # a complex128 grid keeps its precision on the way in, as in the reference
    g = np.ascontiguousarray(g, dtype=np.complex128 if g.dtype == np.complex128 else np.complex64)
    assert g.ndim == 2, "fd_slot_data: (Nr, 14 * carrier_RE_size)"
    return t.from_numpy(g[None]).cuda(), t.tensor([int(slot)], dtype=t.int32, device="cuda")


def ls_est(fd_slot_data, config, slot, kind):
    """(H_LS (S, 3*RBSize, Nr, NL) complex64, RS_info) of one slot."""
    p = phy._slot_params(config)   # the reference's asserts and refusals come first
    grid, slots = _device_grid(fd_slot_data, slot)
    (h_ls,) = phy.slot_frontend(grid, slots, config, want=("h_ls",))
    RS_info = {"type": kind, "RSSymMap": p["symlist"], "PortIndexList": list(config["PortIndexList"])[:p["NL"]],
               "RE_distance": 4, "NumCDMGroupsWithoutData": p["cdm"]}
    return h_ls[0].cpu().numpy().astype(np.complex64, copy=False), RS_info


def copy_resource(rx_fd_slot_data, config):
    """(pdsch_resource (NrOfSymbols, 12*RBSize, Nr) complex64, pdsch_RE_usage float64) of one slot."""
    p = phy._slot_params(config)
    _, usage = phy.slot_data_re_idx(config)
    grid, slots = _device_grid(rx_fd_slot_data, 0)
    (y,) = phy.slot_frontend(grid, slots, config, want=("y",))
    y = y[0].cpu().numpy().reshape(14, 12 * p["rb_size"], grid.shape[1])
    return np.ascontiguousarray(y[p["start"]:p["start"] + p["nsym"]], dtype=np.complex64), usage
