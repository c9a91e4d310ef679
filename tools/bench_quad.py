#!/usr/bin/env python3
"""Validation-utility kernel (csrc/quadform.hip) in isolation, at the headline shapes:
12 validation months x 106 (g, year) cells for each p (n = 513 / 257 / 129 / 65), 101 lambdas.
Prints ms per launch and the achieved fp64 rate (symmetric half of D_t B counted).  The launch
plan is made and uploaded once, as in a grid step, and the launches are timed with device
events: host planning (about 2 ms per call of quadform_utilities) is not the kernel's time."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pfml.ops.ridge import quad_launch, quad_plan, upload  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    T, P, L, C = 120, 513, 101, 106
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(T, 64, P, generator=g, dtype=torch.float64, device=dev)
    D = X.transpose(1, 2) @ X / 64
    R = torch.randn(T, P, generator=g, dtype=torch.float64, device=dev)
    beta = torch.randn(C, L, P, generator=g, dtype=torch.float64, device=dev) * 0.01
    out = {}
    for n in (513, 257, 129, 65):
        jc = np.repeat(np.arange(C), 12)
        jm = (np.arange(C * 12) * 7) % T
        jn = np.full(C * 12, n)
        plan = quad_plan(P, L, P, jc, jm, jn)
        d_desc, d_tj = upload([plan["desc"], plan["tile_job"]], dev)
        obj = torch.empty((len(jc), L), dtype=torch.float64, device=dev)
        for _ in range(3):
            quad_launch(plan, d_desc, d_tj, D, R, beta, obj)
        torch.cuda.synchronize()
        reps = 20
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            quad_launch(plan, d_desc, d_tj, D, R, beta, obj)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        flops = len(jc) * (n * n + n * 64) * 101 * 2 / 2      # upper block triangle
        out[f"n{n}_ms"] = round(ms, 3)
        out[f"n{n}_tflops"] = round(flops / ms / 1e9, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
