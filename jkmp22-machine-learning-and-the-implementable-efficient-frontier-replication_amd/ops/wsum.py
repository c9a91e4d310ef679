"""Expanding-window sums of the hyper-parameter grid (K14) in the canonical chunked order.

``WindowPlan`` is one rank's share of the canonical chunk layout (models/search.py
``rank_window_plan`` derives it from ``win_layout``; ``window_plan`` here checks it); the ops
run csrc/segsum.hip on device tensors and the same folds in torch on CPU tensors (the fp64
oracle of the chunk association).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as nat

MAX_SEGMENTS = 128      # csrc/segsum.hip WV_SEG: the segments a workgroup's LDS holds

nat.register_hip("pfml_wsum_chunk_totals", [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_void_p])
nat.register_hip("pfml_wsum_chunk_prefix", [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_int64, C.c_int, C.c_void_p])
nat.register_hip("pfml_wvec_chunk", [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p])
nat.register_hip("pfml_wsum_onepass", [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p])


@dataclass(frozen=True, eq=False)
class WindowPlan:
    """One rank's window segments and chunks (``window_plan`` checks every index once).

    Segment s sums the local month rows [st[s], sp[s]); the first ``skip`` segments (burn-in
    pieces) only feed the prefix, the other nYl = nseg - skip are this rank's hp-year blocks.
    Local chunk lc folds the segments [cs[lc], ce[lc]) into slot ``slot[lc]`` of this rank's
    totals.  In the gathered totals of every rank (``counts`` slots per rank, in rank order)
    burn-in piece k sits in slot sb[k] and year chunk c in slot sy[c]; year chunk c <= clast
    has the local segments [ys[c], ye[c]) (empty when another rank owns it).  All int32."""
    T: int                  # local months the segments index
    nseg: int
    skip: int
    nYl: int
    nlc: int                # local chunks
    C: int                  # canonical chunks per kind
    clast: int              # last year chunk this rank owns (-1: none)
    counts: tuple           # chunk-total slots per rank
    st: np.ndarray
    sp: np.ndarray
    cs: np.ndarray
    ce: np.ndarray
    slot: np.ndarray
    sb: np.ndarray
    sy: np.ndarray
    ys: np.ndarray
    ye: np.ndarray
    # this rank owns every chunk in canonical slot order, its year chunks' totals fold exactly
    # the segments their windows walk and the canonical walk visits the segments in index
    # order (world size one): what ``window_sums_onepass`` needs
    onepass: bool
    # device copies, views of ONE upload (None without a device or without segments); the
    # kernels take [cs | ce | slot] (3 x nlc) and [sb | sy | ys | ye] (4 x C) as one array each
    d_st: torch.Tensor | None = None
    d_sp: torch.Tensor | None = None
    d_cs_ce_slot: torch.Tensor | None = None
    d_sb_sy_ys_ye: torch.Tensor | None = None

    @property
    def nslot(self) -> int:
        return int(sum(self.counts))


def window_plan(*, T: int, skip: int, C: int, clast: int, counts, st, sp, cs, ce, slot, sb, sy,
                ys, ye, dev=None, who: str = "window plan") -> WindowPlan:
    """Check every index the window-sum kernels turn into an address, decide the one-pass
    eligibility and upload the index arrays (one pinned copy) when ``dev`` is a GPU."""
    st, sp, cs, ce, slot, sb, sy, ys, ye = (np.asarray(a, np.int32) for a in
                                            (st, sp, cs, ce, slot, sb, sy, ys, ye))
    nseg, nlc, nslot = len(st), len(cs), int(sum(counts))
    if nseg and (st.min() < 0 or sp.max() > T or (sp < st).any() or nseg > MAX_SEGMENTS):
        raise ValueError(f"{who}: window segments out of range (T={T}, nseg={nseg})")
    for a, b in ((cs, ce), (ys, ye)):
        if len(a) and (a.min() < 0 or b.max() > nseg or (b < a).any()):
            raise ValueError(f"{who}: chunk segment ranges out of range")
    for arr in (sb, sy):
        if len(arr) and (arr.min() < 0 or arr.max() >= nslot):
            raise ValueError(f"{who}: chunk total slots out of range")
    if len(slot) and (slot.min() < 0 or slot.max() >= nlc):
        raise ValueError(f"{who}: local chunk slots out of range")
    nYl = nseg - skip
    onepass = nlc == nslot and nlc == 2 * C and np.array_equal(slot, np.arange(nlc))
    if onepass:
        walk = ([s for k in range(C) for s in range(cs[sb[k]], ce[sb[k]])]
                + [s for c in range(clast + 1) for s in range(ys[c], ye[c])])
        own = sy[:clast + 1]
        onepass = (walk == list(range(nseg)) and np.array_equal(cs[own], ys[:clast + 1])
                   and np.array_equal(ce[own], ye[:clast + 1]))
    d = [None] * 4
    if nseg and dev is not None and dev.type == "cuda":
        d = nat.upload([st, sp, np.concatenate([cs, ce, slot]),
                        np.concatenate([sb, sy, ys, ye])], dev)
    return WindowPlan(T=int(T), nseg=nseg, skip=int(skip), nYl=nYl, nlc=nlc, C=int(C),
                      clast=int(clast), counts=tuple(int(c) for c in counts), st=st, sp=sp,
                      cs=cs, ce=ce, slot=slot, sb=sb, sy=sy, ys=ys, ye=ye, onepass=bool(onepass),
                      d_st=d[0], d_sp=d[1], d_cs_ce_slot=d[2], d_sb_sy_ys_ye=d[3])


def _fold_months(X: torch.Tensor, a: int, b: int) -> torch.Tensor:
    """CPU segment sum: left fold over months a .. b-1 of X [G, T, ...] (a fixed order, the
    same on every rank that holds these months)."""
    acc = torch.zeros_like(X[:, 0])
    for t in range(a, b):
        acc = acc + X[:, t]
    return acc


def chunk_totals(X: torch.Tensor, R: torch.Tensor, wp: WindowPlan):
    """Kernel A of the canonical chunked window sums (models/search.py): segment sums of this
    rank's segments and the totals of its chunks, chunk-major [nlc, G, P, P] / [nlc, G, P].
    Returns (totD, totR, bufs); ``bufs`` carries the segment sums to ``chunk_windows``."""
    G, T, P, _ = X.shape
    nlc, nseg, skip = wp.nlc, wp.nseg, wp.skip
    # matrix and vector totals of a chunk side by side in ONE row of one buffer (``bufs["tot"]``,
    # [nlc, G P P + G P]): the multi-rank path all-gathers them as one collective; totD / totR
    # are row-strided views and the kernels take that row stride
    GPP = G * P * P
    tot = torch.empty((nlc, GPP + G * P), dtype=X.dtype, device=X.device)
    totD = tot[:, :GPP].view(nlc, G, P, P)
    totR = tot[:, GPP:].view(nlc, G, P)
    out = torch.empty((G, wp.nYl, P, P), dtype=X.dtype, device=X.device)
    if nat.is_device(X):
        if X.dtype != torch.float64 or not X.is_contiguous():
            raise ValueError("chunk_totals: contiguous fp64 required")
        scratch = (torch.empty((G, skip, P, P), dtype=X.dtype, device=X.device) if skip
                   else None)
        lib = nat.hip_lib()
        s = nat.stream_of(X)
        nat.check(lib.pfml_wsum_chunk_totals(
            X.data_ptr(), P, T, G, nat.ptr(wp.d_st), nat.ptr(wp.d_sp), nseg, skip,
            out.data_ptr(), nat.ptr(scratch), nlc, nat.ptr(wp.d_cs_ce_slot), totD.data_ptr(),
            totD.stride(0), s), "pfml_wsum_chunk_totals")
        nat.check(lib.pfml_wvec_chunk(
            R.data_ptr(), P, T, G, nat.ptr(wp.d_st), nat.ptr(wp.d_sp), nseg, skip, 0, nlc,
            nat.ptr(wp.d_cs_ce_slot), wp.C, nat.ptr(wp.d_sb_sy_ys_ye), wp.clast,
            totR.data_ptr(), totR.stride(0), None, s), "pfml_wvec_chunk")
        return totD, totR, {"out": out, "scratch": scratch, "tot": tot}
    segD = [_fold_months(X, a, b) for a, b in zip(wp.st, wp.sp)]
    segR = [_fold_months(R, a, b) for a, b in zip(wp.st, wp.sp)]
    for lc in range(nlc):
        accD, accR = torch.zeros_like(X[:, 0]), torch.zeros_like(R[:, 0])
        for s in range(int(wp.cs[lc]), int(wp.ce[lc])):
            accD = accD + segD[s]
            accR = accR + segR[s]
        totD[lc], totR[lc] = accD, accR
    return totD, totR, {"out": out, "segD": segD, "segR": segR, "tot": tot}


def chunk_windows(X: torch.Tensor, R: torch.Tensor, wp: WindowPlan, totD: torch.Tensor,
                  totR: torch.Tensor, bufs: dict) -> tuple[torch.Tensor, torch.Tensor]:
    """Kernel B of the canonical chunked window sums: E = fold of the burn-in totals, then per
    year chunk the fold of its segments from the prefix P_c (``totD``/``totR``: every chunk's
    total, gathered, in the canonical slot order of ``wp``).  Returns (SD, Sr)."""
    G, T, P, _ = X.shape
    nseg, skip, clast, C = wp.nseg, wp.skip, wp.clast, wp.C
    out = bufs["out"]
    if totD.shape[0] != wp.nslot or totR.shape[0] != wp.nslot:
        # the slot map addresses the GATHERED totals of every rank (a local-only buffer here
        # would be read out of bounds by the device kernels)
        raise ValueError(f"chunk_windows: {totD.shape[0]} chunk totals, the canonical layout "
                         f"has {wp.nslot} slots (all-gather missing?)")
    Sr = torch.empty((G, wp.nYl, P), dtype=X.dtype, device=X.device)
    if nat.is_device(X):
        lib = nat.hip_lib()
        s = nat.stream_of(X)
        # (row-strided totals: each slot's G blocks contiguous, the slots totD.stride(0) apart)
        if totD.stride()[1:] != (P * P, P, 1) or totR.stride()[1:] != (P, 1):
            raise ValueError("chunk_windows: chunk totals must be row-strided [slot][g] blocks")
        nat.check(lib.pfml_wsum_chunk_prefix(
            P, G, nseg, skip, out.data_ptr(), nat.ptr(bufs["scratch"]), C,
            nat.ptr(wp.d_sb_sy_ys_ye), totD.data_ptr(), totD.stride(0), clast, s),
            "pfml_wsum_chunk_prefix")
        nat.check(lib.pfml_wvec_chunk(
            R.data_ptr(), P, T, G, nat.ptr(wp.d_st), nat.ptr(wp.d_sp), nseg, skip, 1, 0,
            nat.ptr(wp.d_cs_ce_slot), C, nat.ptr(wp.d_sb_sy_ys_ye), clast, totR.data_ptr(),
            totR.stride(0), Sr.data_ptr(), s), "pfml_wvec_chunk")
        return out, Sr
    segD, segR = bufs["segD"], bufs["segR"]
    pD, pR = torch.zeros_like(X[:, 0]), torch.zeros_like(R[:, 0])
    for k in range(C):
        pD = pD + totD[int(wp.sb[k])]
        pR = pR + totR[int(wp.sb[k])]
    for c in range(clast + 1):
        aD, aR = pD, pR
        for s in range(int(wp.ys[c]), int(wp.ye[c])):
            aD = aD + segD[s]
            aR = aR + segR[s]
            if s >= skip:
                out[:, s - skip] = aD
                Sr[:, s - skip] = aR
        if c < clast:
            pD = pD + totD[int(wp.sy[c])]
            pR = pR + totR[int(wp.sy[c])]
    return out, Sr


def window_sums_onepass(X: torch.Tensor, R: torch.Tensor, wp: WindowPlan):
    """The canonical chunked window sums of a rank that owns every chunk (world size one) in
    ONE launch (csrc/segsum.hip wsum_onepass_kernel): each month's upper triangle is read once
    and the windows are written once, with no segment sums or chunk totals in memory.  Bitwise
    ``chunk_windows(*chunk_totals(...))``.  Returns (SD [G, nYl, P, P], Sr [G, nYl, P])."""
    G, T, P, _ = X.shape
    if not nat.is_device(X) or not nat.is_device(R):
        raise ValueError("window_sums_onepass: device tensors required")
    if X.dtype != torch.float64 or not X.is_contiguous():
        raise ValueError("window_sums_onepass: contiguous fp64 required")
    if R.dtype != torch.float64 or not R.is_contiguous() or R.shape != (G, T, P):
        raise ValueError("window_sums_onepass: R must be a contiguous fp64 [G, T, P] tensor")
    if not wp.onepass or T != wp.T:
        # the kernel walks each element's months once, in canonical order
        raise ValueError("window_sums_onepass: this rank does not own every chunk of the "
                         "canonical layout (world size one required)")
    SD = torch.empty((G, wp.nYl, P, P), dtype=X.dtype, device=X.device)
    Sr = torch.empty((G, wp.nYl, P), dtype=X.dtype, device=X.device)
    if wp.nYl == 0 or wp.nseg == 0:
        return SD, Sr
    nat.check(nat.hip_lib().pfml_wsum_onepass(
        X.data_ptr(), R.data_ptr(), P, T, G, nat.ptr(wp.d_st), nat.ptr(wp.d_sp), wp.nseg,
        wp.skip, wp.nlc, nat.ptr(wp.d_cs_ce_slot), wp.C, nat.ptr(wp.d_sb_sy_ys_ye), wp.clast,
        SD.data_ptr(), Sr.data_ptr(), nat.stream_of(X)), "pfml_wsum_onepass")
    return SD, Sr
