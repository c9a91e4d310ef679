"""The two steps of Multiperiod-ML that the weight chain of models/portfolio.py cannot express
(csrc/multiperiod.hip), in the symbols of ops/linalg.py (a = Lambda^-1/2, m = diag(a) m_tilde
diag(1/a), W_t the wealth path, mu_hat_{t,h} the predicted return of month t at horizon h):

    b_tau   = (a_t o mu_hat_{t,tau+1}) / W_t                         tau = 0 .. K-1
    v_{K-1} = b_{K-1};  v_tau = b_tau + gbar (m_tilde_t v_{tau+1})    tau = K-2 .. 0;  V_t := v_0
    w_opt,t = a_t o (m_tilde_t (w_start,t / a_t + u V_t))
    w_start,t+1 = (w_opt,t * grow_t)[nmap_t] * hit_t                  (``portfolio._chain``)

* ``horizon_fold`` - V of every month, no arms (u enters linearly): one launch, one workgroup
  per month;
* ``mp_chain``     - A arms (one u each) walk the B months side by side: one launch per month
  enqueued by a host loop with no round trip, every row of m_tilde_t read once per launch.

The step is ``m w_start + offset``, not ``w_aim + m (w_start - w_aim)``: turning one into the
other would cost an (I - m) solve per month.  A month's live universe is its first ``n_rows[t]``
rows and columns; nothing beyond them is read from m_tilde, a, mu_hat and V, and padding
outputs of V and Wopt are 0.  Device tensors up to ``max_n()`` columns go through the HIP
kernels; CPU tensors and wider months take the torch branch - the plain loop of the formulas."""
from __future__ import annotations

import torch

from ..utils import work as _work
from . import _native as nat

_P, _I, _L, _D = nat.C.c_void_p, nat.C.c_int, nat.C.c_int64, nat.C.c_double
nat.register_hip("pfml_mp_max_n", [])
nat.register_hip("pfml_mp_max_arms", [_I])
nat.register_hip("pfml_mp_fold", [_P, _L, _L, _P, _P, _L, _P, _P, _L, _D, _I, _I, _I, _P, _P])
nat.register_hip("pfml_mp_chain", [_P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _L, _P, _L, _I, _I,
                                   _I, _P, _P, _L, _P, _P])


def max_n() -> int:
    return int(nat.hip_lib().pfml_mp_max_n())


def max_arms(N: int) -> int:
    return int(nat.hip_lib().pfml_mp_max_arms(int(N)))


def _f64(x, shape, what):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64:
        raise TypeError(f"multiperiod: {what} must be an fp64 tensor")
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"multiperiod: {what} must be {list(shape)}, got {list(x.shape)}")


def _check_m(mt, a, n_rows):
    if not isinstance(mt, torch.Tensor) or mt.dtype != torch.float64:
        raise TypeError("multiperiod: mt must be an fp64 tensor")
    if mt.dim() != 3 or mt.shape[1] != mt.shape[2]:
        raise ValueError(f"multiperiod: mt must be [B, N, N], got {list(mt.shape)}")
    B, N = int(mt.shape[0]), int(mt.shape[1])
    if N < 1:
        raise ValueError("multiperiod: zero columns")
    if N > 1 and mt.stride(2) != 1:
        raise ValueError("multiperiod: mt needs a unit inner stride (a strided view of rows)")
    _f64(a, (B, N), "a")
    if not isinstance(n_rows, torch.Tensor) or n_rows.dtype not in (torch.int32, torch.int64):
        raise TypeError("multiperiod: n_rows must be an int32 or int64 tensor")
    if tuple(n_rows.shape) != (B,):
        raise ValueError(f"multiperiod: n_rows must be [{B}]")
    return B, N


def _n32(n_rows, N, dev):
    return n_rows.to(device=dev, dtype=torch.int32).clamp(0, N).contiguous()


def _live(n_rows, N, dev):
    n = n_rows.to(device=dev, dtype=torch.int64).clamp(0, N)
    return torch.arange(N, device=dev)[None, :] < n[:, None]


def _strides(mt):
    B, N = mt.shape[:2]
    return (mt.stride(1) if N > 1 else N), (mt.stride(0) if B > 1 else max(mt.stride(1), N) * N)


# ---------------------------------------------------------------------------------------------
def horizon_fold(mt: torch.Tensor, a: torch.Tensor, mu_hat: torch.Tensor, wealth: torch.Tensor,
                 n_rows: torch.Tensor, gbar: float = 1.0) -> torch.Tensor:
    """V [B, N] of the B months: mt [B, N, N] (m_tilde; any row and month stride, read in
    place), a [B, N], mu_hat [K, B, N] (K >= 1 horizons), wealth [B], n_rows [B].  Device: ONE
    launch of ``mp_fold_kernel`` (a month's bits do not depend on B or on its place)."""
    B, N = _check_m(mt, a, n_rows)
    if not isinstance(mu_hat, torch.Tensor) or mu_hat.dtype != torch.float64:
        raise TypeError("multiperiod: mu_hat must be an fp64 tensor")
    if mu_hat.dim() != 3 or tuple(mu_hat.shape[1:]) != (B, N) or mu_hat.shape[0] < 1:
        raise ValueError(f"multiperiod: mu_hat must be [K >= 1, {B}, {N}], got "
                         f"{list(mu_hat.shape)}")
    _f64(wealth, (B,), "wealth")
    K, dev = int(mu_hat.shape[0]), mt.device
    gbar = float(gbar)
    if nat.is_device(mt) and N <= max_n():
        V = torch.empty((B, N), dtype=torch.float64, device=dev)
        if B:
            ldm, sm = _strides(mt)
            a_c, mu_c, w_c = a.contiguous(), mu_hat.contiguous(), wealth.contiguous()
            nr = _n32(n_rows, N, dev)
            _work.add("mp_fold_kernel", 2.0 * B * N * N * (K - 1) + 2.0 * B * N * K,
                      8.0 * B * (N * N * (K > 1) + N * (K + 2)))
            nat.check(nat.hip_lib().pfml_mp_fold(
                mt.data_ptr(), ldm, sm, a_c.data_ptr(), mu_c.data_ptr(), B * N, w_c.data_ptr(),
                nr.data_ptr(), N, gbar, K, B, N, V.data_ptr(), nat.stream_of(mt)),
                "pfml_mp_fold")
        return V
    live = _live(n_rows, N, dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    M = torch.where(live[:, :, None] & live[:, None, :], mt, zero)
    b = torch.where(live[None], (a[None] * mu_hat) / wealth[None, :, None], zero)
    v = b[K - 1]
    for tau in range(K - 2, -1, -1):
        v = torch.where(live, b[tau] + gbar * torch.matmul(M, v[..., None])[..., 0], zero)
    return v.contiguous()


# ---------------------------------------------------------------------------------------------
def mp_chain(mt: torch.Tensor, a: torch.Tensor, V: torch.Tensor, u, n_rows: torch.Tensor,
             grow: torch.Tensor, nmap: torch.Tensor, hit: torch.Tensor, ws0: torch.Tensor):
    """A arms walk the B months in order -> (Wst [A, B, N], Wopt [A, B, N], w_start after the
    last month [A, N]).  Arm k in month t, with ws its w_start (``ws0`` [N] or [A, N] first):

        w_opt = a_t o (m_tilde_t (ws / a_t + u[k] V_t))    on the month's n_rows[t] live rows
        ws <- (w_opt * grow[t])[nmap[t]] * hit[t]          (all N columns, ``portfolio._chain``)

    mt, a, n_rows as ``horizon_fold``; V [B, N] its output; u: A scales (sequence or tensor);
    grow, hit [B, N] fp64 and nmap [B, N] int64 with entries in [0, N).  Device: B + 1 launches
    of ``mp_month_kernel`` per chunk of at most ``max_arms(N)`` arms; arm k's bits depend
    neither on A nor on k's place."""
    B, N = _check_m(mt, a, n_rows)
    _f64(V, (B, N), "V")
    _f64(grow, (B, N), "grow")
    _f64(hit, (B, N), "hit")
    if not isinstance(nmap, torch.Tensor) or nmap.dtype != torch.int64:
        raise TypeError("multiperiod: nmap must be an int64 tensor")
    if tuple(nmap.shape) != (B, N):
        raise ValueError(f"multiperiod: nmap must be [{B}, {N}]")
    dev = mt.device
    f64 = dict(dtype=torch.float64, device=dev)
    uarm = torch.as_tensor(u, **f64).flatten().contiguous()
    A = int(uarm.shape[0])
    if not isinstance(ws0, torch.Tensor) or ws0.dtype != torch.float64:
        raise TypeError("multiperiod: ws0 must be an fp64 tensor")
    if tuple(ws0.shape) not in ((N,), (A, N)):
        raise ValueError(f"multiperiod: ws0 must be [{N}] or [{A}, {N}]")
    Wst = torch.zeros((A, B, N), **f64)
    Wopt = torch.zeros((A, B, N), **f64)
    if not A or not B:
        return Wst, Wopt, ws0.expand(A, N).contiguous()
    if nat.is_device(mt) and N <= max_n():
        lib = nat.hip_lib()
        cap = max_arms(N)
        if cap < 1:
            raise RuntimeError(f"pfml_mp_chain takes no arm at N = {N}")
        ws = torch.empty((A, N), **f64)
        ldm, sm = _strides(mt)
        keep = [x.contiguous() for x in (a, V, grow, nmap, hit, ws0)]
        a_c, V_c, grow_c, nmap_c, hit_c, ws0_c = keep
        nr = _n32(n_rows, N, dev)
        sws0 = N if ws0_c.dim() == 2 else 0
        for c0 in range(0, A, cap):
            Ac = min(cap, A - c0)
            _work.add("mp_month_kernel", B * (2.0 * N * N * Ac + 3.0 * N * Ac),
                      8.0 * B * (N * N + N * (6 + 3 * Ac)), calls=B + 1)
            nat.check(lib.pfml_mp_chain(
                mt.data_ptr(), ldm, sm, a_c.data_ptr(), V_c.data_ptr(),
                uarm.data_ptr() + 8 * c0, nr.data_ptr(), grow_c.data_ptr(), nmap_c.data_ptr(),
                hit_c.data_ptr(), N, ws0_c.data_ptr() + 8 * c0 * sws0, sws0, B, N, Ac,
                Wst[c0].data_ptr(), Wopt[c0].data_ptr(), B * N, ws[c0].data_ptr(),
                nat.stream_of(mt)), "pfml_mp_chain")
        return Wst, Wopt, ws
    live = _live(n_rows, N, dev)
    zero, one = torch.zeros((), **f64), torch.ones((), **f64)
    q = nmap.clamp(0, N - 1)
    ws = ws0.expand(A, N)
    for t in range(B):
        lt = live[t]
        Wst[:, t] = ws
        d = torch.where(lt, ws / torch.where(lt, a[t], one) + uarm[:, None] * V[t], zero)
        Mt = torch.where(lt[:, None] & lt[None, :], mt[t], zero)
        # one product per arm: an arm's bits do not depend on the other arms here either
        md = torch.stack([torch.mv(Mt, d[k]) for k in range(A)])
        wopt = torch.where(lt, a[t] * md, zero)
        Wopt[:, t] = wopt
        ws = (wopt * grow[t])[:, q[t]] * hit[t]                   # next month's w_start
    return Wst, Wopt, ws.contiguous()
