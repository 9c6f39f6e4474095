"""Mixed-(bgn, Zc) batched min-sum decode (ldpc5g_decode_ms_mixed) — the shape DLSCHDecode
(py5gphy/nr_pdsch/nr_dlsch_decode.py:62-91) and ULSCH_decoding produce once their per-codeblock
loop is batched: codeblocks of different lifting sizes decoded in at most two launches."""
import numpy as np

from . import _lib
from .ldpc_info import code_dims, find_iLS


def decode_mixed(items, L, alpha=1.0, beta=0.0, schedule="flooding", rate_matched=False):
    """items: list of (bgn, Zc, llr[N]) with float32 (or all float64) LLR rows.
    rate_matched: the rows come from rate recovery (LDPC5G_RATE_MATCHED: untransmitted extension
    columns +0.0 are detected and their null row updates skipped; same results).
    Returns (list of ck int8[Nf] arrays, status bool[B], iters int32[B]) in item order."""
    t = _lib.require_gpu()
    assert schedule in ("flooding", "layered")
    B = len(items)
    f64 = all(np.asarray(l).dtype == np.float64 for _, _, l in items) and schedule == "flooding"
    dt = np.float64 if f64 else np.float32
    desc = (_lib.CbDesc * max(B, 1))()
    lo = co = 0
    rows = []
    for k, (bgn, Zc, llr) in enumerate(items):
        assert bgn in [1, 2] and find_iLS(Zc) < 8
        K, N, Nf = code_dims(bgn, Zc)
        llr = np.asarray(llr, dt)
        assert llr.size == N
        desc[k].bgn, desc[k].Zc, desc[k].llr_off, desc[k].ck_off = bgn, Zc, lo, co
        rows.append((lo, co, Nf))
        lo += N
        co += Nf
    flat = np.concatenate([np.asarray(l, dt) for _, _, l in items]) if B else np.zeros(1, dt)
    x = t.from_numpy(flat).cuda()
    ck = t.empty(max(co, 1), dtype=t.int8, device=x.device)
    st = t.empty(max(B, 1), dtype=t.uint8, device=x.device)
    it = t.empty(max(B, 1), dtype=t.int32, device=x.device)
    _lib.call("ldpc5g_decode_ms_mixed", x.device, desc=desc, B=B, llr_base=x, llr_dtype=_lib.F64 if f64 else _lib.F32,
              ck_base=ck, status=st, iters=it, L=int(L), alpha=float(alpha), beta=float(beta),
              schedule=_lib.LAYERED if schedule == "layered" else _lib.FLOODING,
              flags=_lib.RATE_MATCHED if rate_matched else 0)
    ckh = ck.cpu().numpy()
    return ([ckh[c:c + n].copy() for _, c, n in rows], st.cpu().numpy()[:B].astype(bool),
            it.cpu().numpy()[:B])


class MixedBatch:
    """A device-resident mixed-(bgn, Zc) batch for repeated decoding (the bench's config 4):
    rows of several (bgn, Zc) groups concatenated in one flat LLR buffer, with the descriptor
    array (ldpc5g_cb_desc_t) built once.

    groups: list of (bgn, Zc, llr (n, N) device tensor), all float32 or all float64 (float64:
    flooding only, the reference's arithmetic).  flat: an existing flat buffer of that dtype
    holding exactly those rows back to back in group order (e.g. sch_raterecover_multi's output,
    whose row groups are views of it): used in place, nothing is copied."""

    def __init__(self, groups, flat=None):
        t = _lib.require_gpu()
        B = sum(g[2].shape[0] for g in groups)
        self.desc = (_lib.CbDesc * max(B, 1))()
        parts, lo, co, k = [], 0, 0, 0
        self.rows = []
        dt = groups[0][2].dtype
        self.dtype = _lib.dtype_id(dt, llr=True)
        for bgn, Zc, llr in groups:
            assert bgn in [1, 2] and find_iLS(Zc) < 8 and llr.dtype == dt
            K, N, Nf = code_dims(bgn, Zc)
            assert llr.dim() == 2 and llr.shape[1] == N
            for _ in range(llr.shape[0]):
                d = self.desc[k]
                d.bgn, d.Zc, d.llr_off, d.ck_off = bgn, Zc, lo, co
                self.rows.append((co, Nf))
                lo += N
                co += Nf
                k += 1
            parts.append(llr.reshape(-1))
        dev = groups[0][2].device
        if flat is not None:
            assert flat.dtype == dt and flat.is_contiguous() and flat.numel() >= lo
            self.llr = flat
        else:
            self.llr = t.cat(parts).contiguous()
        self.ck = t.empty(max(co, 1), dtype=t.int8, device=dev)
        self.status = t.empty(max(B, 1), dtype=t.uint8, device=dev)
        self.iters = t.empty(max(B, 1), dtype=t.int32, device=dev)
        self.B = B
        self._plans = {}

    def _plan(self, schedule):
        """Work list for `schedule`, built on the host once (pinned) and copied to the device
        once; later decodes only launch (ldpc5g_decode_ms_mixed_plan)."""
        p = self._plans.get(schedule)
        if p is None:
            t = _lib.torch()
            sc = _lib.LAYERED if schedule == "layered" else _lib.FLOODING
            n = _lib.call("ldpc5g_mixed_plan", desc=self.desc, B=self.B, schedule=sc, plan=None, plan_bytes=0)
            host = t.empty((max(n, 1),), dtype=t.uint8, pin_memory=True)
            _lib.call("ldpc5g_mixed_plan", desc=self.desc, B=self.B, schedule=sc, plan=host, plan_bytes=n)
            dev = host.to(self.llr.device, non_blocking=True)
            p = self._plans[schedule] = (host, dev)
        return p

    def decode(self, L, alpha=1.0, beta=0.0, schedule="layered", rate_matched=False):
        """<= 2 kernel launches on the current stream, asynchronous (no host synchronisation);
        returns the device buffers (ck flat, status (B,), iters (B,)).  rate_matched: see
        decode_mixed."""
        assert schedule != "layered" or self.dtype == _lib.F32, "the layered kernel is float32"
        host, dev = self._plan(schedule)
        _lib.call("ldpc5g_decode_ms_mixed_plan", self.llr.device, plan_dev=dev, plan_host=host, llr_base=self.llr,
                  llr_dtype=self.dtype, ck_base=self.ck, status=self.status, iters=self.iters, L=int(L),
                  alpha=float(alpha), beta=float(beta), schedule=_lib.LAYERED if schedule == "layered" else _lib.FLOODING,
                  flags=_lib.RATE_MATCHED if rate_matched else 0)
        return self.ck, self.status[:self.B], self.iters[:self.B]
