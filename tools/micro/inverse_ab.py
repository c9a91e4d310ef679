#!/usr/bin/env python3
"""Bitwise A/B of two builds of the SPD-inverse kernels (csrc/spd_inverse.hip: the 64-leaf
Gauss-Jordan, the one-launch 65..128-row node, the one-triangle recursive inverse) and of the
pivoted LU solve (csrc/lu_solve.hip).

    PFML_HIP_LIB=<lib A> python tools/micro/inverse_ab.py save A.json
    PFML_HIP_LIB=<lib B> python tools/micro/inverse_ab.py save B.json
    python tools/micro/inverse_ab.py cmp A.json B.json

``save`` inverts fixed-seed SPD batches (n = 490: nodes of 128 and 106 rows; n = 100: one
node; n = 64 and 37: a single leaf) with ``spd_inverse_sym`` and stores the results and the
launch times (the results as SHA-256 digests), then digests the m_func path built on them
(``mfunc_cases``: only calls that every tree since the one-triangle inverse has); ``cmp``
reports per case whether the digests match (bitwise equal).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pfml.ops.linalg as la  # noqa: E402

# (batches large enough that the GPU, not the Python launch path, sets the time)
CASES = [(192, 490), (2048, 100), (4096, 64), (4096, 37)]


def _spd(B, n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn(B, n, n + 32, generator=g, dtype=torch.float64, device=dev)
    A = X @ X.transpose(1, 2) / (n + 32) + 1e-3 * torch.eye(n, dtype=torch.float64, device=dev)
    return 0.5 * (A + A.transpose(1, 2))


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _m_tilde_inputs(tc):
    """The inputs of tests/test_gpu_pipeline.py::test_m_tilde_production_shape."""
    rng = np.random.default_rng(1)
    B, N, K, n = 2, 496, 25, 489
    X = rng.normal(size=(B, N, K))
    X[:, n:] = 0.0
    F = np.stack([np.cov(rng.normal(size=(K, 300))) * 21e-4 for _ in range(B)])
    iv = rng.uniform(0.01, 0.03, (B, N)) ** 2 * 21
    iv[:, n:] = 1.0
    S = np.einsum("bik,bkl,bjl->bij", X, F, X) + np.stack([np.diag(v) for v in iv])
    w = np.array([1e10, 3e9])
    lam = 0.2 / rng.uniform(1e7, 1e9, (B, N)) if tc else np.full((B, N), 1e-16)
    lam[:, n:] = 10.0 / w[:, None]
    mask = np.zeros((B, N))
    mask[:, :n] = 1.0
    t = lambda v: torch.tensor(v, dtype=torch.float64)                      # noqa: E731
    return (t(S), t(lam), t(w), t([0.003, 0.001]), 0.007, 10.0, 10), t(mask)


def mfunc_cases(dev):
    """Digests of the m_func path (ops/linalg.py): the two-sided inverse, the Denman-Beavers
    root, m_tilde at the production shape and the fused symmetric passes (csrc/s4.hip)."""
    out = {}

    def put(key, *ts):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in ts:
            h.update(t.contiguous().cpu().numpy().tobytes())
        out[key] = h.hexdigest()

    for B, n in ((3, 513), (3, 193)):
        put(f"spd_inverse_{B}x{n}", la.spd_inverse(_spd(B, n, dev, 200 + n)))
    for B, N, kw in ((2, 200, {}), (3, 160, {"exact_sym": True})):
        X = _rand(B, N + 40, N, seed=300 + N)
        S = X.transpose(1, 2) @ X / N
        S = S @ S + 1e-3 * torch.eye(N, dtype=torch.float64)
        Sd = (0.5 * (S + S.transpose(1, 2)) if kw else S).to(dev)
        st = torch.zeros(B, dtype=torch.int32, device=dev)
        ws = [torch.empty_like(Sd) for _ in range(4)]
        put(f"db_sqrt_{B}x{N}" + ("_exact_sym" if kw else ""),
            la._db_sqrt(Sd, la.DB_ITERS, la.DB_SCALED_ITERS, st, ws, **kw), st)
    for tc in (True, False):
        args, mask = _m_tilde_inputs(tc)
        for exact in (False, True):
            d = [x.to(dev) if isinstance(x, torch.Tensor) else x for x in args]
            if exact:              # (the flag promises an exactly symmetric Sigma)
                d[0] = 0.5 * (d[0] + d[0].transpose(1, 2))
            st = torch.zeros(2, dtype=torch.int32, device=dev)
            mt, a = la.m_tilde(*d, mask=mask.to(dev), status=st, sigma_exact_sym=exact)
            put(f"m_tilde_tc{int(tc)}_exact{int(exact)}", mt, a, st)
    for N, flat in ((37, False), (490, True)):
        B = 3
        X, Y = _rand(B, N, N, seed=1), _rand(B, N, N, seed=2)
        if flat:
            X, Y = X + X.transpose(1, 2), Y + Y.transpose(1, 2)
        kw = dict(svec=_rand(B, seed=3).abs() + 0.5, cvec=_rand(B, seed=4).abs() + 1.0,
                  a=_rand(B, N, seed=5).abs() + 0.1, mask=(_rand(B, N, seed=6) > -0.8).double())
        kd = {k: v.to(dev) for k, v in kw.items()}
        for mode in (0, 1, 2, 4):
            put(f"mf_sym_mode{mode}_{'flat' if flat else 'tiled'}_{N}",
                la.mf_sym(mode, X.to(dev), Y.to(dev), torch.empty_like(X).to(dev), d=1.5,
                          flat=flat, **kd))
    return out


def save(path):
    dev = torch.device("cuda", 0)
    out, times = {}, {}
    for k, (B, n) in enumerate(CASES):
        A = _spd(B, n, dev, k)
        X = torch.empty_like(A)
        st = torch.zeros(B, dtype=torch.int32, device=dev)
        la.spd_inverse_sym(X, st, src=A)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20
        e0.record()
        for _ in range(reps):
            la.spd_inverse_sym(X, st, src=A)
        e1.record()
        torch.cuda.synchronize()
        err = float((torch.bmm(X, A) - torch.eye(n, dtype=A.dtype, device=dev)).abs().max())
        out[f"{B}x{n}"] = hashlib.sha256(X.cpu().numpy().tobytes()).hexdigest()
        times[f"{B}x{n}"] = {"ms": round(e0.elapsed_time(e1) / reps, 4), "max_abs_XA_minus_I": err,
                             "status": int(st.sum())}
    # the pivoted LU solve of augmented [B | A] rows (csrc/lu_solve.hip, the S4 const^-1 Omega
    # form: one- and two-level), general A (partial pivoting active)
    for k, (B, n, m, two) in enumerate([(64, 490, 258, True), (64, 490, 258, False),
                                        (24, 137, 66, True)]):
        g = torch.Generator(device=dev).manual_seed(100 + k)
        Wz = m + n + (la.LU_PANEL_COLS if two else 0)
        M0 = torch.randn(B, n, Wz, generator=g, dtype=torch.float64, device=dev)
        M = M0.clone()
        st = torch.zeros(B, dtype=torch.int32, device=dev)
        z0 = m + n if two else None
        la.solve_augmented(M, n, m, a0=m, b0=0, status=st, z0=z0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            M.copy_(M0)
            la.solve_augmented(M, n, m, a0=m, b0=0, status=st, z0=z0)
        e1.record()
        torch.cuda.synchronize()
        X = M[:, :, :m]
        res = float((torch.bmm(M0[:, :, m:m + n], X) - M0[:, :, :m]).abs().max())
        key = f"lu{'2' if two else '1'}_{B}x{n}x{m}"
        out[key] = hashlib.sha256(X.contiguous().cpu().numpy().tobytes()).hexdigest()
        times[key] = {"ms_incl_copy": round(e0.elapsed_time(e1) / 10, 4), "max_abs_residual": res,
                      "status": int(st.sum())}
    out.update(mfunc_cases(dev))
    with open(path, "w") as f:
        json.dump(out, f)
    print(json.dumps({"lib": os.environ.get("PFML_HIP_LIB", "in-tree"), "cases": times}))


def cmp(pa, pb):
    with open(pa) as fa, open(pb) as fb:
        a, b = json.load(fa), json.load(fb)
    res = {k: a[k] == b[k] for k in a}
    print(json.dumps({"sha256_equal": res, "bitwise_equal": all(res.values())}))


if __name__ == "__main__":
    if sys.argv[1] == "save":
        save(sys.argv[2])
    else:
        cmp(sys.argv[2], sys.argv[3])
