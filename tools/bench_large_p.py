#!/usr/bin/env python3
"""Measurements of the grid search at p = 1024 and p = 2048 (n = p + 1 up to 2049).

    python tools/bench_large_p.py grid     [--grids default,p1024,p2048] [--steps 3]
    python tools/bench_large_p.py ab       [--reps 5]
    python tools/bench_large_p.py headline --parent DIR [--runs 3]

``grid``      the grid step (window sums, ridge grid, utilities, scores) on synthetic production
              windows (710 months, 53 hp years, 2 g, 101 lambda; bench.py's synthetic summands)
              as a replayed HIP graph, for the default p_vec, the default plus 1024, and the
              default plus 1024 and 2048: ms per step, solves/s, peak memory, and the per-kernel
              split of one eager step from event pairs (every launch group on its own, not
              overlapped: tridiagonalisation / tridiagonal solves / back-transform / repair /
              utilities; the band path's launch is one entry).
``ab``        the back-transform of cells with n > 1024: the blocked MFMA kernel against the
              generic one-reflector-at-a-time path at n = 1025 and 2049, L = 101, 1 and 106
              cells, the arms alternating within this process.
``headline``  bench.py's default-grid headline of this tree and of a built checkout of the
              parent commit (``--parent``), in alternating runs.

Each mode merges its section into ``--out`` (default profiles/r08_large_p.json).
"""
import argparse
import dataclasses
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = {"default": [], "p1024": [1024], "p2048": [1024, 2048]}


def _merge(path: str, key: str, val) -> None:
    doc = {}
    if os.path.exists(path):
        with open(path, encoding="utf-8") as f:
            doc = json.load(f)
    doc[key] = val
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", encoding="utf-8") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def _event_ms(fn, reps: int = 1) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def kernel_split(reals, cfg) -> dict:
    """One eager grid step's ridge / repair / utilities launches, group by group between event
    pairs on one stream (sums over the groups, ms)."""
    from pfml.models.search import _search_setup, window_sums
    from pfml.ops import ridge as rg
    dev = reals.denom.device
    G, T, P = reals.G, reals.denom.shape[1], reals.P
    months = np.asarray(reals.months, dtype=np.int64)
    su = _search_setup(months, np.asarray(cfg.hp_years), cfg.p_vec, G, T, 1, 0, dev,
                       np.asarray(cfg.l_vec, dtype=np.float64), np.arange(T, dtype=np.int64))
    SD, Sr = window_sums(reals, su.win)
    nYl = su.nYl
    SD, Sr = SD.reshape(G * nYl, P, P), Sr.reshape(G * nYl, P)
    D, R = reals.denom.reshape(G * T, P, P), reals.r_tilde.reshape(G * T, P).contiguous()
    lv = su.lvec
    L = int(lv.numel())
    plan = rg._utilities_plan(P, L, dev, su.cell_src, su.cell_n, su.cell_scale,
                              su.jc, su.jm, su.jn, split=True)
    beta = torch.empty((len(su.cell_n), L, P), dtype=torch.float64, device=dev)
    obj = torch.empty((len(su.jc), L), dtype=torch.float64, device=dev)
    out = {"band_launch": 0.0, "tridiagonalisation": 0.0, "tridiagonal_solves": 0.0,
           "back_transform": 0.0, "repair": 0.0, "utilities": 0.0, "groups": []}
    dv = plan["dv"]
    for gi, (cells, jobs, rp, qp) in enumerate(plan["groups"]):
        d_desc, d_q, d_tj, d_wg = dv[4 * gi: 4 * gi + 4]
        rec = {"n": sorted(set(int(v) for v in rp["desc"]["n"])), "cells": int(rp["nc"])}
        if rg.band_path(rp):
            rec["band_launch"] = _event_ms(
                lambda: rg.ridge_launch(rp, d_desc, SD, Sr, lv, beta, d_wgmap=d_wg))
            out["band_launch"] += rec["band_launch"]
        else:
            # one workspace for the full launch and the single phases that read its results
            work = torch.empty(rp["work"], dtype=torch.float64, device=dev)
            rg.ridge_launch(rp, d_desc, SD, Sr, lv, beta, d_wgmap=d_wg, work=work)
            for bit, name in ((1, "tridiagonalisation"), (2, "tridiagonal_solves"),
                              (4, "back_transform")):
                rec[name] = _event_ms(
                    lambda: rg.ridge_launch(rp, d_desc, SD, Sr, lv, beta, d_wgmap=d_wg,
                                            phases=bit, work=work))
                out[name] += rec[name]
            rg.ridge_launch(rp, d_desc, SD, Sr, lv, beta, d_wgmap=d_wg, work=work)  # betas for (utilities)
            rec["repair"] = _event_ms(lambda: rg.repair_launch(rp, d_desc, SD, Sr, lv, beta))
            out["repair"] += rec["repair"]
        rec["utilities"] = _event_ms(lambda: rg.quad_launch(qp, d_q, d_tj, D, R, beta, obj))
        out["utilities"] += rec["utilities"]
        out["groups"].append(rec)
    torch.cuda.synchronize()
    return out


def mode_grid(args) -> None:
    import bench
    from pfml.config import Config
    from pfml.parallel import dist as pdist
    dev = pdist.init("auto").device
    res = {}
    for name in args.grids.split(","):
        cfg = Config.default()
        p_vec = list(cfg.p_vec) + GRIDS[name]
        cfg = cfg.override([f"pf_ml.p_vec={json.dumps(p_vec)}"])
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        reals = bench.synthetic_reals(cfg, dev, n_months=args.months, n_stocks=args.stocks)
        torch.cuda.synchronize()
        setup_s = time.perf_counter() - t0
        box = {}

        def step():
            box["res"], box["scores"] = bench.one_step(reals, cfg)

        rep = bench.graphed(step, dev)
        ms = bench.timed(rep if rep is not None else step, args.steps, args.warmup, dev)
        n_solves = len(cfg.g_vec) * len(cfg.hp_years) * len(p_vec) * len(cfg.l_vec)
        from pfml.ops.ridge import coop_errors, repairs_done
        rec = {"p_vec": p_vec, "P": int(reals.P), "months": args.months, "steps": args.steps,
               "warmup": args.warmup, "hip_graph": rep is not None, "ms_per_step": round(ms, 3),
               "solves": n_solves, "solves_per_s": round(n_solves / (ms / 1e3), 1),
               "outputs_finite": bool(torch.isfinite(box["res"].obj).all().item()),
               "repairs": repairs_done(), "coop_timeouts": coop_errors(),
               "setup_s": round(setup_s, 2)}
        del rep
        rec["kernel_split_ms"] = kernel_split(reals, cfg)
        rec["peak_memory_gb"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
        print(json.dumps({name: rec}), flush=True)
        res[name] = rec
        _merge(args.out, "grid_step", {**_load(args.out).get("grid_step", {}), name: rec})
        del reals, box
    return res


def _load(path: str) -> dict:
    if os.path.exists(path):
        with open(path, encoding="utf-8") as f:
            return json.load(f)
    return {}


def mode_ab(args) -> None:
    from pfml.ops import ridge as rg
    dev = torch.device("cuda", 0)
    lv = torch.tensor([0.0] + list(np.exp(np.linspace(-10, 10, 100))), dtype=torch.float64,
                      device=dev)
    L = int(lv.numel())
    rows = []
    for n in (1025, 2049):
        S = 4
        X = torch.randn(S, n + 400, n, dtype=torch.float64, device=dev)
        SD = (X.transpose(1, 2) @ X).contiguous()
        del X
        Sr = torch.randn(S, n, dtype=torch.float64, device=dev)
        for ncells in (1, 106):
            src, nn, sc = np.arange(ncells) % S, np.full(ncells, n), np.full(ncells, 1e-3)
            plan = rg.ridge_plan(n, L, src, nn, sc)
            d_desc, = rg.upload([plan["desc"]], dev)
            beta = torch.empty((ncells, L, n), dtype=torch.float64, device=dev)
            work = torch.empty(plan["work"], dtype=torch.float64, device=dev)
            arms = {"blocked_mfma": dataclasses.replace(rg.switches(), bt_wy=True),
                    "generic": dataclasses.replace(rg.switches(), bt_wy=False)}

            def launch(k, phases=7):
                rg.ridge_launch(plan, d_desc, SD, Sr, lv, beta, sw=arms[k], phases=phases,
                                work=work)

            betas, ts, whole = {}, {k: [] for k in arms}, {}
            for k in arms:                            # whole launch, and the betas to compare
                launch(k)
                whole[k] = _event_ms(lambda: launch(k))
                betas[k] = beta.clone()
            for _ in range(args.reps):                # back-transform alone, arms alternating
                for k in arms:
                    ts[k].append(_event_ms(lambda: launch(k, phases=4)))
            dif = ((betas["blocked_mfma"] - betas["generic"]).norm(dim=-1)
                   / betas["generic"].norm(dim=-1)).max().item()
            rec = {"n": n, "cells": ncells, "L": L, "reps": args.reps,
                   "back_transform_ms": {k: round(float(np.median(v)), 3) for k, v in ts.items()},
                   "back_transform_ms_all": {k: [round(x, 3) for x in v] for k, v in ts.items()},
                   "whole_launch_ms": {k: round(v, 3) for k, v in whole.items()},
                   "max_rel_diff_of_betas": dif}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
        del SD, Sr
        torch.cuda.empty_cache()
    _merge(args.out, "back_transform_ab", rows)


def mode_headline(args) -> None:
    """bench.py --gpus 1 of the parent checkout and of this tree, alternating."""
    trees = {"parent": os.path.abspath(args.parent), "this": ROOT}
    runs = {k: [] for k in trees}
    for i in range(args.runs):
        for k, d in trees.items():
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps),
                   "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"bench.py failed in {d}:\n{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            ms = float(json.loads(line)["ms_per_step"])
            print(f"run {i} {k}: {ms} ms", flush=True)
            runs[k].append(ms)
    spread = {k: round(max(v) - min(v), 3) for k, v in runs.items()}
    med = {k: float(np.median(v)) for k, v in runs.items()}
    _merge(args.out, "default_grid_headline", {
        "command": f"bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup}",
        "ms_per_step": runs, "median_ms": med, "spread_ms": spread,
        "median_difference_ms": round(med["this"] - med["parent"], 3),
        "within_parent_spread": abs(med["this"] - med["parent"]) <= max(spread["parent"], 1e-9)})


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["grid", "ab", "headline"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_large_p.json"))
    ap.add_argument("--grids", default="default,p1024,p2048")
    ap.add_argument("--months", type=int, default=710)
    ap.add_argument("--stocks", type=int, default=500)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent", default="")
    args = ap.parse_args()
    {"grid": mode_grid, "ab": mode_ab, "headline": mode_headline}[args.mode](args)


if __name__ == "__main__":
    main()
