#!/usr/bin/env python3
"""The device eigensolver alone (ops.linalg.eigh_psd, csrc/eigh_jacobi.hip): a batch of B
matrices x = (gamma / w) L^-1/2 Sigma L^-1/2 of the m_func shape (K = 25 factors plus specific
variance, 7 padded rows at N = 496) at wealth w; median wall seconds of ``--reps`` calls after
one warm-up, the device synchronised around each, and the sweeps the call took.

    python tools/bench_eigh.py --batch 32 --n 496 --wealth 1
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def m_func_x(B, N, wealth, seed=1, K=25, gamma=10.0):
    rng = np.random.default_rng(seed)
    n = N - max(1, N // 70)
    X = rng.normal(size=(B, N, K))
    X[:, n:] = 0.0
    F = np.stack([np.cov(rng.normal(size=(K, 300))) * 21e-4 for _ in range(B)])
    iv = rng.uniform(0.01, 0.03, (B, N)) ** 2 * 21
    iv[:, n:] = 1.0
    S = np.einsum("bik,bkl,bjl->bij", X, F, X) + np.stack([np.diag(v) for v in iv])
    lam = 0.2 / rng.uniform(1e7, 1e9, (B, N))
    lam[:, n:] = 10.0 / wealth
    a = 1.0 / np.sqrt(lam)
    x = (gamma / wealth) * S * a[:, :, None] * a[:, None, :]
    return 0.5 * (x + x.transpose(0, 2, 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n", type=int, default=496)
    ap.add_argument("--wealth", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from pfml.ops import linalg as la
    dev = torch.device("cuda", 0)
    x = torch.tensor(m_func_x(a.batch, a.n, a.wealth), device=dev)
    times, info = [], {}
    for rep in range(a.reps + 1):
        st = torch.zeros(a.batch, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        e, Vt = la.eigh_psd(x, status=st, info=info)
        torch.cuda.synchronize(dev)
        if rep:
            times.append(time.perf_counter() - t)
    lib = la.nat.hip_lib()
    resid = (torch.bmm(x, Vt.transpose(1, 2)) - Vt.transpose(1, 2) * e.unsqueeze(1)).abs().amax()
    out = {"metric": "eigh_psd wall seconds", "device": torch.cuda.get_device_name(dev),
           "batch": a.batch, "n": a.n, "wealth": a.wealth,
           "seconds_median": round(float(np.median(times)), 5),
           "seconds_all": [round(t, 5) for t in times], "sweeps": info["sweeps"],
           "block_rounds_per_sweep": lib.pfml_eigh_psd_rounds(a.n),
           "status_nonzero": int(st.sum().item()),
           "max_residual_over_norm": float(resid / e.abs().amax())}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
