"""Per-month portfolio statistics on the padded [B, ld] layout of the weight recursion
(csrc/pfstats.hip; portfolio.pf_ts / PFML_best_hps.py:220-259 without a DataFrame)."""
from __future__ import annotations

import torch

from . import _native as nat

_P, _I, _L = nat.C.c_void_p, nat.C.c_int, nat.C.c_int64
nat.register_hip("pfml_pf_stats", [_P, _P, _P, _P, _P, _P, _L, _I, _P, _P])

STAT_COLUMNS = ("inv", "shorting", "turnover", "r", "tc")


def pf_stats(w: torch.Tensor, w_start: torch.Tensor, ret: torch.Tensor, lam: torch.Tensor,
             n_rows: torch.Tensor, wealth: torch.Tensor) -> torch.Tensor:
    """[B, 5] = (inv, shorting, turnover, r, tc) of every month.

    w, w_start, ret, lam: [B, ld] fp64; month t uses its first ``n_rows[t]`` columns, the rest
    is padding and never enters a sum.  wealth: [B].  Sums follow pandas ``groupby.sum``: a NaN
    term is skipped in that statistic only, a month without a finite term gives 0.  Device
    tensors go through one launch of ``pfml_pf_stats`` (one workgroup per month, a fixed
    reduction order: bitwise independent of B and of the month's position); CPU tensors take
    the fp64 torch path with the same NaN rule."""
    if w.dim() != 2 or not (w.shape == w_start.shape == ret.shape == lam.shape):
        raise ValueError("pf_stats: w, w_start, ret, lam must be [B, ld] of one shape")
    B, ld = w.shape
    if n_rows.shape != (B,) or wealth.shape != (B,):
        raise ValueError("pf_stats: n_rows and wealth must be [B]")
    ops = [w, w_start, ret, lam, wealth]
    if any(x.dtype != torch.float64 or x.device != w.device for x in ops):
        raise ValueError("pf_stats: fp64 tensors on one device expected")
    if nat.is_device(w):
        # rows at one common stride (a row slice of a wider [B, N] buffer is read in place)
        sd = w.stride(0) if B > 1 else ld
        if not all(x.stride(1) == 1 and (B == 1 or x.stride(0) == sd) for x in ops[:4]) \
                or sd < ld:
            w, w_start, ret, lam = (x.contiguous() for x in ops[:4])
            sd = ld
        n32 = n_rows.to(device=w.device, dtype=torch.int32).clamp(0, ld).contiguous()
        wl = wealth.contiguous()
        out = torch.empty((B, 5), dtype=torch.float64, device=w.device)
        nat.check(nat.hip_lib().pfml_pf_stats(w.data_ptr(), w_start.data_ptr(), ret.data_ptr(),
                                              lam.data_ptr(), n32.data_ptr(), wl.data_ptr(),
                                              sd, B, out.data_ptr(), nat.stream_of(w)),
                  "pfml_pf_stats")
        return out
    live = torch.arange(ld)[None, :] < n_rows.to(torch.int64).clamp(0, ld)[:, None]
    dw = w - w_start
    terms = torch.stack([w.abs(), w.clamp(max=0.0).abs(), dw.abs(), w * ret, lam * dw * dw], 1)
    keep = live[:, None, :] & ~torch.isnan(terms)
    out = torch.where(keep, terms, torch.zeros_like(terms)).sum(-1)
    out[:, 4] = wealth / 2.0 * out[:, 4]
    return out
