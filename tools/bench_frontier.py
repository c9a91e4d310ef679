#!/usr/bin/env python3
"""The efficient frontier (models/frontier.py) at production shape: the synthetic 500-stock
engine panel (``engine_inputs()`` defaults), the default p_vec / g_vec / l_vec, the 4 x 5
wealth x gamma grid of ``settings["ef"]``.

Timed:
  * the full frontier (the sum of its points' wall seconds, and the per-point seconds);
  * one point split into its phases (S4 plan re-aim, S4, grid search, selection, aims, chain,
    statistics; the device is synchronised at every mark), plus the host layouts that are
    built once (``make_s4_plan``, ``backtest_layout``);
  * the same points through a loop of the existing stages - ``Pipeline.run`` on
    pfml-input .. pfml-best-hps with the wealth file rewritten per point - in the same
    process, the two arms alternating point by point.  The stage arm gets the panel, the Barra
    arrays and the risk-free frame handed over in memory (it does not re-read the database per
    point), so what it pays per point is its S4 plan, the validation frame, the aim frames, the
    S9 plan, pf_ts and its CSV outputs; its file I/O seconds are reported separately.
Recorded per point: m_func repairs and every fallback counter (wealth = 1 included), the
relative difference of the two arms' pf_summary rows, the peak device memory allocated during
the point (the frontier arm alone: the counter is reset after the stage arm).

    python tools/bench_frontier.py --out profiles/r09_frontier.json

The wealth = 1 column alone, with the m_func repair's share of each point (the seconds inside
``linalg.m_func_reference``, device synchronised around each call) and the eigensolver's sweeps
per repair chunk - PFML_MFUNC_REPAIR_EIG=0 in the environment is the host-root arm:

    python tools/bench_frontier.py --set ef.wealth=[1.0] --loop-points 0 --repair-detail
"""
import argparse
import gc
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S4_S9 = ["pfml-input", "pfml-search-coef", "pfml-hp-reals", "pfml-aim", "pfml-hps",
         "pfml-best-hps"]
NUM = ["n", "inv", "shorting", "turnover_notional", "r", "sd", "sr_gross", "tc", "r_tc", "sr",
       "obj"]


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stocks", type=int, default=500)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--loop-points", type=int, default=-1,
                    help="points that also go through the stage loop (-1: all)")
    ap.add_argument("--set", action="append", default=[], help="dotted override key=value")
    ap.add_argument("--out", default="", help="write the JSON here as well")
    ap.add_argument("--repair-detail", action="store_true",
                    help="time the m_func repair calls and record the eigensolver's sweeps")
    a = ap.parse_args()
    from pfml.config import Config
    from pfml.data import io
    from pfml.data.synthetic import engine_inputs
    from pfml.models import frontier, portfolio
    from pfml.models import pfml_inputs as pin
    from pfml.pipeline import Pipeline
    from pfml.utils.dates import pfml_date_grids
    dev = torch.device(a.device)
    cuda = dev.type == "cuda"

    def sync():
        if cuda:
            torch.cuda.synchronize(dev)

    cfg = Config.default().override(a.set)
    cfg.run.compat_mode = False          # distinct RFF draw per g (no rff_w.csv), as bench.py
    cfg.run.plots = False
    t0 = time.perf_counter()
    chars, barra, wealth, rf = engine_inputs(n_stocks=a.stocks)
    data_s = time.perf_counter() - t0
    s = cfg.settings
    grids = pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                            s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                            s["pf"]["dates"]["split_years"])
    wv = [float(x) for x in s["ef"]["wealth"]]
    gv = [float(x) for x in s["ef"]["gamma_rel"]]
    npts = len(wv) * len(gv)
    nloop = npts if a.loop_points < 0 else min(a.loop_points, npts)

    # ---- one point, phase by phase (cold: with the once-only host layouts; then warm) ----
    def phases(ctx):
        marks, last = {}, [time.perf_counter()]

        def clock(name):
            sync()
            t = time.perf_counter()
            marks[name] = round(marks.get(name, 0.0) + t - last[0], 4)
            last[0] = t

        cfg_pt = frontier.point_config(cfg, 1e10, 10.0)
        sync()
        last[0] = time.perf_counter()
        frontier.run_point(cfg_pt, chars, barra, frontier.scaled_wealth(cfg, wealth, 1e10), rf,
                           dev, grids, ctx, clock=clock)
        return marks

    ctx: dict = {}
    cold = phases(ctx)
    warm = phases(ctx)
    warm = phases(ctx)
    once = {"make_s4_plan_s": round(cold["s4_plan"] - warm["s4_plan"], 4),
            "backtest_layout_s": cold.get("layout", 0.0)}
    del ctx
    print(json.dumps({"phases_s": warm, "host_layout_once_s": once}), flush=True)

    # ---- the two arms, alternating point by point --------------------------------------
    tmp = tempfile.mkdtemp(prefix="pfml_ef_bench_")
    points = []
    repair = {"s": 0.0, "calls": 0, "matrices": 0, "sweeps": []}
    if a.repair_detail:
        from pfml.ops import linalg as la
        inner, inner_eigh = la.m_func_reference, la._eigh_psd_device

        def timed_repair(sigma, *args, **kw):
            sync()
            t = time.perf_counter()
            r = inner(sigma, *args, **kw)
            sync()
            repair["s"] += time.perf_counter() - t
            repair["calls"] += 1
            repair["matrices"] += int(sigma.shape[0])
            return r

        def counted_eigh(*args, **kw):
            r = inner_eigh(*args, **kw)
            repair["sweeps"].append(int(r[3]))
            return r

        la.m_func_reference, la._eigh_psd_device = timed_repair, counted_eigh

    def stage_arm(W, gam):
        cfg_pt = frontier.point_config(cfg, W, gam)
        cfg_pt.run.data_dir = os.path.join(tmp, "data")
        cfg_pt.run.artifact_dir = os.path.join(tmp, "art")
        wealth_pt = frontier.scaled_wealth(cfg, wealth, W)
        sync()
        t = time.perf_counter()
        io0 = io.IO_SECONDS[0]
        io.write_csv(wealth_pt, cfg_pt.run.data_dir, "wealth_processed.csv")
        pipe = Pipeline(cfg_pt, device=a.device)
        pipe.state.update(chars=chars, barra=barra, wealth=wealth_pt, risk_free=rf, grids=grids)
        pipe.run(S4_S9)
        sync()
        return (time.perf_counter() - t, io.IO_SECONDS[0] - io0,
                pipe.state["pf_summary"].iloc[0])

    def on_point(row):
        k = len(points)
        rec = {"wealth_end": row["wealth_end"], "gamma_rel": row["gamma_rel"],
               "frontier_s": row["seconds"], "s4_repairs": row["s4_repairs"],
               "s4_fallbacks": json.loads(row["s4_fallbacks"]),
               "grid_recomputed_cells": row["grid_recomputed_cells"],
               "finite": bool(np.isfinite([row[c] for c in NUM]).all())}
        if a.repair_detail:
            rec.update(repair_s=round(repair["s"], 4),
                       repair_share=round(repair["s"] / max(row["seconds"], 1e-300), 3),
                       repair_calls=repair["calls"],
                       repair_matrices=repair["matrices"], eigh_sweeps=repair["sweeps"])
            repair.update(s=0.0, calls=0, matrices=0, sweeps=[])
        if cuda:
            rec["peak_device_bytes"] = int(torch.cuda.max_memory_allocated(dev))
            rec["allocated_after_bytes"] = int(torch.cuda.memory_allocated(dev))
        # (the stages repair every flagged m_func month in one batch: not run where that batch
        # is larger than the frontier's repair chunk, nor where the point itself failed)
        if k < nloop and rec["finite"] and row["s4_repairs"] <= frontier.REPAIR_CHUNK:
            dt, io_s, summ = stage_arm(row["wealth_end"], row["gamma_rel"])
            ref = np.asarray([summ[c] for c in NUM], float)
            got = np.asarray([row[c] for c in NUM], float)
            rec.update(stage_loop_s=round(dt, 4), stage_loop_io_s=round(io_s, 4),
                       max_rel_diff=float(np.max(np.abs(got - ref) /
                                                 np.maximum(np.abs(ref), 1e-300))))
        points.append(rec)
        print(json.dumps(rec), flush=True)
        gc.collect()                     # (the stage arm's frames and state, outside the clocks)
        if cuda:
            torch.cuda.reset_peak_memory_stats(dev)

    if cuda:
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
    frontier.efficient_frontier(cfg, chars, barra, wealth, rf, dev, on_point=on_point)
    shutil.rmtree(tmp, ignore_errors=True)

    per_point = np.asarray([p["frontier_s"] for p in points])
    frontier_wall = float(per_point.sum())
    both = [p for p in points if "stage_loop_s" in p]
    nloop = len(both)
    fr = np.asarray([p["frontier_s"] for p in both])
    st = np.asarray([p["stage_loop_s"] for p in both])
    clean = np.asarray([p["frontier_s"] for p in points if not p["s4_repairs"]])
    out = {
        "metric": "efficient frontier, wealth x gamma grid, wall-clock",
        "device": torch.cuda.get_device_name(dev) if cuda else "cpu",
        "stocks": a.stocks, "pfml_months": int(len(grids["m2"])),
        "oos_months": int(len(grids["oos"])), "p_vec": cfg.p_vec, "g_vec": cfg.g_vec,
        "n_lambda": int(len(cfg.l_vec)), "wealth": wv, "gamma_rel": gv, "points": npts,
        "data_s": round(data_s, 2),
        "frontier_s": round(frontier_wall, 3),
        "frontier_s_per_point_median": round(float(np.median(per_point)), 4),
        "frontier_s_per_point_median_no_repairs": (round(float(np.median(clean)), 4)
                                                   if len(clean) else None),
        "one_point_phases_s": warm, "host_layout_once_s": once,
        "stage_loop": {"points": nloop, "stage_loop_s": round(float(st.sum()), 3),
                       "frontier_s_same_points": round(float(fr.sum()), 3),
                       "stage_loop_io_s": round(float(sum(p["stage_loop_io_s"]
                                                          for p in both)), 3),
                       "skipped_points": len(points) - nloop,
                       "speedup": round(float(st.sum() / fr.sum()), 2) if nloop else None,
                       "max_rel_diff": max((p["max_rel_diff"] for p in both), default=None)},
        "repairs_per_point": [{"wealth_end": p["wealth_end"], "gamma_rel": p["gamma_rel"],
                               "s4_repairs": p["s4_repairs"], "s4_fallbacks": p["s4_fallbacks"],
                               "grid_recomputed_cells": p["grid_recomputed_cells"]}
                              for p in points],
        "all_points_finite": all(p["finite"] for p in points),
        "peak_device_bytes_point_1": points[0].get("peak_device_bytes"),
        "peak_device_bytes_point_last": points[-1].get("peak_device_bytes"),
        "allocated_after_point_1": points[0].get("allocated_after_bytes"),
        "allocated_after_point_last": points[-1].get("allocated_after_bytes"),
        "per_point": points,
    }
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
