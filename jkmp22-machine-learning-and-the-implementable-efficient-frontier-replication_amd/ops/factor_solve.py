"""Solves with "factor part plus diagonal" (csrc/factor_solve.hip):

    (X F_s X' + diag(d)) w = b,    F_s = fscale F

by ``w = u - D^-1 X M (X'u)`` with ``u = b / d``, ``G = X' D^-1 X``, ``M = (I + F_s G)^-1 F_s``.
No n x n matrix is formed and F is never inverted, so F may have zero rows.

* ``factor_prepare`` - M of every system s = (diagonal variant v, month t);
* ``factor_chain``   - A arms walk the B months side by side: each month's right-hand side is
  ``rhs + c * w_start``, the solution optionally normalised to sum 1, and the next w_start is
  the drift of ``portfolio._chain`` on the ``backtest_layout`` operands.

Device tensors within the kernels' limits (``max_k()`` factors, ``max_n()`` columns for the
chain) go through the HIP kernels; beyond a limit the launcher refuses with ValueError and the
public functions take the torch branch - the same formula batched over arms, which is also the
CPU path."""
from __future__ import annotations

import torch

from . import _native as nat

_P, _I, _L = nat.C.c_void_p, nat.C.c_int, nat.C.c_int64
nat.register_hip("pfml_factor_solve_max_n", [])
nat.register_hip("pfml_factor_solve_max_k", [])
nat.register_hip("pfml_factor_prepare", [_P, _L, _L, _P, _L, _P, _P, _P, _L, _P, _I, _I, _I, _I,
                                         _P, _P, _P])
nat.register_hip("pfml_factor_chain", [_P, _L, _L, _P, _L, _P, _P, _L, _P, _P, _P, _P, _P, _P,
                                       _P, _L, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P])

ST_ZERO_PIVOT, ST_NONFINITE = 1, 2


def max_n() -> int:
    return int(nat.hip_lib().pfml_factor_solve_max_n())


def max_k() -> int:
    return int(nat.hip_lib().pfml_factor_solve_max_k())


def _check_common(bX, ridx, d, n_rows):
    if bX.dim() != 2 or bX.dtype != torch.float64 or (bX.shape[1] > 1 and bX.stride(1) != 1):
        raise TypeError("factor_solve: bX must be a [R, K] fp64 table with unit inner stride")
    if ridx.dim() != 2 or ridx.dtype != torch.int64:
        raise TypeError("factor_solve: ridx must be [B, N] int64")
    B, N = ridx.shape
    if d.dim() != 3 or d.shape[1:] != (B, N) or d.dtype != torch.float64:
        raise TypeError("factor_solve: d must be [V, B, N] fp64")
    if n_rows.shape != (B,):
        raise TypeError("factor_solve: n_rows must be [B]")
    if bX.shape[0] < 1 or bX.shape[1] < 1 or N < 1:
        raise ValueError("factor_solve: empty loading table or zero columns")
    return B, N, int(bX.shape[1]), int(d.shape[0])


def _live(n_rows: torch.Tensor, N: int, dev) -> torch.Tensor:
    n = n_rows.to(device=dev, dtype=torch.int64).clamp(0, N)
    return torch.arange(N, device=dev)[None, :] < n[:, None]


def _gathered(bX, ridx, live):
    """X of every month [B, N, K], zero on padding rows (whose index is never followed)."""
    R = bX.shape[0]
    idx = torch.where(live, ridx, torch.zeros((), dtype=torch.int64, device=ridx.device))
    return bX[idx.clamp(0, R - 1)] * live[..., None].to(bX.dtype)


def _n32(n_rows, N, dev):
    return n_rows.to(device=dev, dtype=torch.int32).clamp(0, N).contiguous()


# ---------------------------------------------------------------------------------------------
def _launch_prepare(bX, ridx, F, fscale, d, n_rows):
    B, N, K, V = _check_common(bX, ridx, d, n_rows)
    if K > max_k():
        raise ValueError(f"pfml_factor_prepare takes at most {max_k()} factors, got {K}")
    dev = bX.device
    ridx_c, F_c, d_c = ridx.contiguous(), F.contiguous(), d.contiguous()
    fs = fscale.to(device=dev, dtype=torch.float64).contiguous()
    M = torch.empty((V, B, K, K), dtype=torch.float64, device=dev)
    status = torch.zeros((V, B), dtype=torch.int32, device=dev)
    if V and B:
        nat.check(nat.hip_lib().pfml_factor_prepare(
            bX.data_ptr(), bX.stride(0) if bX.shape[0] > 1 else K, bX.shape[0],
            ridx_c.data_ptr(), N, F_c.data_ptr(), fs.data_ptr(), d_c.data_ptr(), N,
            _n32(n_rows, N, dev).data_ptr(), V, B, N, K, M.data_ptr(), status.data_ptr(),
            nat.stream_of(bX)), "pfml_factor_prepare")
    return M, status


def _torch_prepare(bX, ridx, F, fscale, d, n_rows):
    B, N, K, V = _check_common(bX, ridx, d, n_rows)
    dev = bX.device
    live = _live(n_rows, N, dev)
    Xg = _gathered(bX, ridx, live)                                   # [B, N, K]
    one = torch.ones((), dtype=torch.float64, device=dev)
    XD = Xg[None] / torch.where(live[None], d, one)[..., None]      # [V, B, N, K]
    G = torch.matmul(Xg.transpose(1, 2)[None], XD)                   # [V, B, K, K]
    Fs = fscale.to(device=dev, dtype=torch.float64).view(V, 1, 1, 1) * F[None]
    Amat = torch.eye(K, dtype=torch.float64, device=dev) + torch.matmul(Fs, G)
    status = torch.zeros((V, B), dtype=torch.int32, device=dev)
    if V and B:
        finite = torch.isfinite(Amat).flatten(2).all(2) & torch.isfinite(Fs).flatten(2).all(2)
        eye = torch.eye(K, dtype=torch.float64, device=dev)
        safe = torch.where(finite[..., None, None], Amat, eye)
        M, info = torch.linalg.solve_ex(safe, Fs)
        M = torch.where(finite[..., None, None], M, torch.full_like(M, float("nan")))
        status = status + (info.to(torch.int32) > 0) * ST_ZERO_PIVOT
        status = status + (~torch.isfinite(M).flatten(2).all(2)).to(torch.int32) * ST_NONFINITE
    else:
        M = torch.empty((V, B, K, K), dtype=torch.float64, device=dev)
    return M, status


def factor_prepare(bX: torch.Tensor, ridx: torch.Tensor, F: torch.Tensor, fscale: torch.Tensor,
                   d: torch.Tensor, n_rows: torch.Tensor):
    """(M [V, B, K, K], status [V, B] int32) with ``M[v, t] = (I + F_s G)^-1 F_s``,
    ``F_s = fscale[v] F[t]``, ``G = X_t' diag(1 / d[v, t]) X_t``.

    bX: the loading table [R, K] (``S4Plan.bX``; any row stride, read in place); ridx [B, N]
    int64: month t's rows of bX in its first ``n_rows[t]`` entries (the rest is padding and is
    never followed); F [B, K, K]; fscale [V]; d [V, B, N].  ``I + F_s G`` is not symmetric:
    the device solves it by LU with partial pivoting in LDS.  status: bit 1 a zero pivot, bit
    2 a non-finite entry of G or M; it stays on the device for the caller's guard."""
    B, N = ridx.shape[-2:] if ridx.dim() == 2 else (0, 0)
    if F.dim() != 3 or F.shape[0] != B or F.shape[1] != F.shape[2] or \
            F.shape[1] != bX.shape[-1] or F.dtype != torch.float64:
        raise TypeError("factor_prepare: F must be [B, K, K] fp64")
    if nat.is_device(bX) and bX.shape[1] <= max_k():
        return _launch_prepare(bX, ridx, F, fscale, d, n_rows)
    return _torch_prepare(bX, ridx, F, fscale, d, n_rows)


# ---------------------------------------------------------------------------------------------
def _check_chain(bX, ridx, M, d, n_rows, rhs, c, varm, normalize, grow, nmap, hit, ws0):
    B, N, K, V = _check_common(bX, ridx, d, n_rows)
    if M.shape != (V, B, K, K) or M.dtype != torch.float64:
        raise TypeError("factor_chain: M must be [V, B, K, K] fp64")
    if rhs.dim() != 3 or rhs.shape[1:] != (B, N) or c.shape != rhs.shape or \
            rhs.dtype != torch.float64 or c.dtype != torch.float64:
        raise TypeError("factor_chain: rhs and c must be [A, B, N] fp64")
    A = int(rhs.shape[0])
    if grow.shape != (B, N) or hit.shape != (B, N) or nmap.shape != (B, N) or \
            nmap.dtype != torch.int64:
        raise TypeError("factor_chain: grow, hit [B, N] fp64 and nmap [B, N] int64 expected")
    if ws0.shape not in ((N,), (A, N)):
        raise TypeError("factor_chain: ws0 must be [N] or [A, N]")
    if len(varm) != A or len(normalize) != A:
        raise TypeError("factor_chain: one variant and one normalize flag per arm expected")
    if any(not 0 <= int(v) < V for v in varm):
        raise ValueError("factor_chain: an arm's variant is not a row of d")
    return A, B, N, K, V


def _launch_chain(bX, ridx, M, d, n_rows, rhs, c, varm, normalize, grow, nmap, hit, ws0):
    A, B, N, K, V = _check_chain(bX, ridx, M, d, n_rows, rhs, c, varm, normalize, grow, nmap,
                                 hit, ws0)
    if K > max_k() or N > max_n():
        raise ValueError(f"pfml_factor_chain takes at most {max_k()} factors and {max_n()} "
                         f"columns, got K = {K}, N = {N}")
    dev = bX.device
    f64 = dict(dtype=torch.float64, device=dev)
    Wst = torch.zeros((A, B, N), **f64)
    Wopt = torch.zeros((A, B, N), **f64)
    ws_end = torch.empty((A, N), **f64)
    if not A or not B:
        ws_end.copy_(ws0.expand(A, N))
        return Wst, Wopt, ws_end
    i32 = dict(dtype=torch.int32, device=dev)
    va = torch.as_tensor([int(v) for v in varm], **i32)
    nz = torch.as_tensor([int(bool(f)) for f in normalize], **i32)
    ws0_c = ws0.contiguous()
    keep = [x.contiguous() for x in (ridx, M, d, rhs, c, grow, nmap, hit)]
    ridx_c, M_c, d_c, rhs_c, c_c, grow_c, nmap_c, hit_c = keep
    nat.check(nat.hip_lib().pfml_factor_chain(
        bX.data_ptr(), bX.stride(0) if bX.shape[0] > 1 else K, bX.shape[0], ridx_c.data_ptr(),
        N, M_c.data_ptr(), d_c.data_ptr(), N, _n32(n_rows, N, dev).data_ptr(),
        rhs_c.data_ptr(), c_c.data_ptr(), grow_c.data_ptr(), nmap_c.data_ptr(),
        hit_c.data_ptr(), ws0_c.data_ptr(), N if ws0_c.dim() == 2 else 0, va.data_ptr(),
        nz.data_ptr(), A, B, N, K, Wst.data_ptr(), Wopt.data_ptr(), ws_end.data_ptr(),
        nat.stream_of(bX)), "pfml_factor_chain")
    return Wst, Wopt, ws_end


def _torch_chain(bX, ridx, M, d, n_rows, rhs, c, varm, normalize, grow, nmap, hit, ws0):
    A, B, N, K, V = _check_chain(bX, ridx, M, d, n_rows, rhs, c, varm, normalize, grow, nmap,
                                 hit, ws0)
    dev = bX.device
    f64 = dict(dtype=torch.float64, device=dev)
    Wst = torch.zeros((A, B, N), **f64)
    Wopt = torch.zeros((A, B, N), **f64)
    ws = ws0.expand(A, N)
    if not A:
        return Wst, Wopt, ws.contiguous()
    live = _live(n_rows, N, dev)
    va = torch.as_tensor([int(v) for v in varm], dtype=torch.int64, device=dev)
    nz = torch.as_tensor([bool(f) for f in normalize], device=dev)
    one, zero = torch.ones((), **f64), torch.zeros((), **f64)
    for t in range(B):
        lt = live[t]
        Xt = _gathered(bX, ridx[t:t + 1], live[t:t + 1])[0]           # [N, K]
        dt = torch.where(lt, d[va, t], one)                           # [A, N]
        Wst[:, t] = ws
        b = torch.where(c[:, t] != 0, rhs[:, t] + c[:, t] * ws, rhs[:, t])
        u = torch.where(lt, b / dt, zero)
        tau = u @ Xt                                                  # [A, K]
        s = torch.matmul(M[va, t], tau[..., None])[..., 0]            # [A, K]
        w = torch.where(lt, u - (s @ Xt.T) / dt, zero)
        w = torch.where(nz[:, None], w / w.sum(1, keepdim=True), w)
        Wopt[:, t] = w
        ws = (w * grow[t])[:, nmap[t].clamp(0, N - 1)] * hit[t]       # next month's w_start
    return Wst, Wopt, ws.contiguous()


def factor_chain(bX: torch.Tensor, ridx: torch.Tensor, M: torch.Tensor, d: torch.Tensor,
                 n_rows: torch.Tensor, rhs: torch.Tensor, c: torch.Tensor, varm, normalize,
                 grow: torch.Tensor, nmap: torch.Tensor, hit: torch.Tensor, ws0: torch.Tensor):
    """A arms walk the B months in order -> (Wst [A, B, N], Wopt [A, B, N], w_start after the
    last month [A, N]).  Arm a in month t, with v = varm[a] its diagonal variant and ws its
    w_start (``ws0`` [N] or [A, N] in the first month):

        b = rhs[a, t] + c[a, t] * ws        (c == 0: b = rhs, whatever ws holds)
        u = b / d[v, t];  w = u - (X_t (M[v, t] (X_t' u))) / d[v, t]
        normalize[a]:  w = w / sum(w)
        ws <- (w * grow[t])[nmap[t]] * hit[t]          (the drift of ``portfolio._chain``)

    over the month's first ``n_rows[t]`` columns; padding columns of Wopt are 0.  Device: ONE
    launch of ``pfml_factor_chain``, one workgroup per arm; every arm's output is bitwise
    independent of the other arms and of its position."""
    args = (bX, ridx, M, d, n_rows, rhs, c, varm, normalize, grow, nmap, hit, ws0)
    if nat.is_device(bX) and bX.shape[1] <= max_k() and ridx.shape[-1] <= max_n():
        return _launch_chain(*args)
    return _torch_chain(*args)
