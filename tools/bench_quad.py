#!/usr/bin/env python3
"""Validation-utility kernel (csrc/quadform.hip) in isolation, at the headline shapes:
12 validation months x 106 (g, year) cells for each p (n = 513 / 257 / 129 / 65), 101 lambdas.
Prints ms per launch and the achieved fp64 rate (symmetric half of D_t B counted).  The launch
plan is made and uploaded once, as in a grid step, and the launches are timed with device
events: host planning (about 2 ms per call of quadform_utilities) is not the kernel's time.

    --months M --cells C --sizes 513,65   the launch's shape (default 12 x 106, all four sizes;
                                          257+129+65: those three in one launch)
    --plans single,runs                   one arm per plan in the same call: single tiles, the
                                          run plan at ridge.QUAD_RUN_STEPS, or runs:N / months:K
                                          (a step target / a forced number of months per run);
                                          the arms must agree bitwise
    --ab OTHER_TREE [--rounds R]          A/B against another checkout built beside this one
                                          (the parent commit's, say): this script of either tree
                                          runs as a child process in turn, A B A B ..., and one
                                          JSON line holds every sample
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pfml.ops import ridge as rg  # noqa: E402


def plan_of(arm, P, L, jc, jm, jn):
    if arm == "single":
        return rg.quad_plan(P, L, P, jc, jm, jn)
    if not hasattr(rg, "QUAD_RUN_STEPS"):
        raise SystemExit(f"plan {arm}: this tree has no run plans")
    if arm == "runs":
        return rg.quad_plan(P, L, P, jc, jm, jn, run_steps=rg.QUAD_RUN_STEPS)
    kind, val = arm.split(":")
    kw = {"runs": "run_steps", "months": "run_months"}[kind]
    return rg.quad_plan(P, L, P, jc, jm, jn, **{kw: int(val)})


def tables_of(plan):
    return rg.quad_tables(plan) if hasattr(rg, "quad_tables") else plan["tile_job"]


def measure(args):
    dev = torch.device("cuda", 0)
    T, P, L, C, M = 120, 513, 101, args.cells, args.months
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(T, 64, P, generator=g, dtype=torch.float64, device=dev)
    D = X.transpose(1, 2) @ X / 64
    R = torch.randn(T, P, generator=g, dtype=torch.float64, device=dev)
    beta = torch.randn(C, L, P, generator=g, dtype=torch.float64, device=dev) * 0.01
    out = {}
    arms = args.plans.split(",")
    for size in args.sizes.split(","):
        ns = [int(v) for v in size.split("+")]     # a+b: C cells of each size in one launch
        n = size.replace("+", "_")
        jc = np.tile(np.repeat(np.arange(C), M), len(ns))
        jm = (np.arange(C * M * len(ns)) * 7) % T
        jn = np.repeat(np.array(ns), C * M)
        ref = None
        for arm in arms:
            plan = plan_of(arm, P, L, jc, jm, jn)
            d_desc, d_tj = rg.upload([plan["desc"], tables_of(plan)], dev)
            obj = torch.empty((len(jc), L), dtype=torch.float64, device=dev)
            for _ in range(3):
                rg.quad_launch(plan, d_desc, d_tj, D, R, beta, obj)
            torch.cuda.synchronize()
            reps = 20
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                rg.quad_launch(plan, d_desc, d_tj, D, R, beta, obj)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            flops = float(np.sum(jn * jn + jn * 64)) * 101 * 2 / 2    # upper block triangle
            tag = f"n{n}" if arms == ["single"] else f"n{n}_{arm}"
            out[f"{tag}_ms"] = round(ms, 4)
            out[f"{tag}_tflops"] = round(flops / ms / 1e9, 1)
            if plan.get("run_off") is not None:
                out[f"{tag}_nruns"] = len(plan["run_off"]) - 1
            if ref is None:
                ref = obj.clone()
            elif not torch.equal(ref, obj):
                raise SystemExit(f"n = {n}: plan {arm} differs from plan {arms[0]}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--months", type=int, default=12)
    ap.add_argument("--cells", type=int, default=106)
    ap.add_argument("--sizes", default="513,257,129,65")
    ap.add_argument("--plans", default="single")
    ap.add_argument("--ab", default=None, metavar="OTHER_TREE")
    ap.add_argument("--ab-plans", default="single", help="--plans of the other tree's runs")
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if args.ab is None:
        print(json.dumps(measure(args)))
        return
    shape = ["--months", str(args.months), "--cells", str(args.cells), "--sizes", args.sizes]
    arms = {"other": [os.path.join(os.path.abspath(args.ab), "tools", "bench_quad.py"), *shape,
                      "--plans", args.ab_plans],
            "this": [os.path.abspath(__file__), *shape, "--plans", args.plans]}
    env = {k: v for k, v in os.environ.items() if k != "PFML_HIP_LIB"}
    out = {"other": [], "this": []}
    for _ in range(args.rounds):
        for arm, cmd in arms.items():
            r = subprocess.run([sys.executable, *cmd], capture_output=True, text=True, env=env,
                               timeout=300)
            if r.returncode != 0:
                raise SystemExit(f"{arm}: exit {r.returncode}\n{r.stderr[-2000:]}")
            out[arm].append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
