#!/usr/bin/env python
"""Benchmark portfolios (models/benchmarks.py) at production shape: 500 stocks, the 516 OOS
months of the default date grid, for the default arms and for the reference's 27-arm Static-ML
grid (pf.hps.static).

The Portfolio-ML point (S4, grid search, layout) is computed once and handed to every run, so a
run is the part of the stage after ``frontier.point_inputs``.  Recorded, as medians of
``--reps`` runs (device synchronised at every mark):
  * seconds after the point, split into the Portfolio-ML backtest, the prediction model's
    summands, its grid search with mu_hat, prepare + chain, the guard, and the statistics with
    the frames;
  * the peak device memory of a run;
  * an A/B in this process, the arms alternating, on the run's own operands:
    ``factor_prepare`` + ``factor_chain`` against the dense route (Sigma by GEMM and
    ``torch.linalg.solve`` month by month), with each arm's spread (max - min) and the
    project's margin (gain >= 5 x the larger spread), the largest difference of the weights, and
    the time of ``factor_prepare`` alone.

    python tools/bench_benchmarks.py --out profiles/r23_benchmarks.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REFERENCE_GRID = ["bmk.static.k=[1,0.3333333333333333,0.2]", "bmk.static.u=[0.25,0.5,1]",
                  "bmk.static.g=[0,1,2]"]


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stocks", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--set", action="append", default=[], help="dotted override key=value")
    ap.add_argument("--end", default="2023-12-31", help="last month of the synthetic panel")
    ap.add_argument("--out", default="", help="write the JSON here as well")
    a = ap.parse_args()
    from pfml.config import Config
    from pfml.data import synthetic as syn
    from pfml.models import benchmarks, frontier
    from pfml.ops.factor_solve import factor_prepare
    from pfml.utils.dates import pfml_date_grids
    dev = torch.device(a.device)
    cuda = dev.type == "cuda"

    def sync():
        if cuda:
            torch.cuda.synchronize(dev)

    base = Config.default().override(a.set)
    base.run.compat_mode = False         # distinct RFF draw per g (no rff_w.csv), as bench.py
    base.run.plots = False
    chars, barra, wealth, rf = syn.engine_inputs(n_stocks=a.stocks, end=a.end)
    s = base.settings
    grids = pfml_date_grids(int(barra.months.min()), int(base.pf_set["lb_hor"]),
                            s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                            s["pf"]["dates"]["split_years"])
    sync()
    t0 = time.perf_counter()
    ctx: dict = {}
    pt = frontier.point_inputs(base, chars, barra, wealth, rf, dev, grids, ctx)
    sync()
    point_s = time.perf_counter() - t0
    layout = ctx["layout"]

    def handed(cfg_pt, chars_, barra_, wealth_pt, risk_free, device, grids_, ctx_, clock=None):
        ctx_["layout"] = layout
        return pt

    frontier.point_inputs = handed
    out = {"metric": "benchmark portfolios after the Portfolio-ML point, wall-clock",
           "device": torch.cuda.get_device_name(dev) if cuda else "cpu",
           "stocks": a.stocks, "N": int(layout["N"]), "oos_months": int(layout["B"]),
           "reps": a.reps, "point_inputs_s_cold": round(point_s, 3), "runs": {}}

    def one_run(cfg, keep=False):
        marks, last = {}, [0.0]

        def clock(name):
            sync()
            t = time.perf_counter()
            marks[name] = t - last[0]
            last[0] = t

        if cuda:
            torch.cuda.reset_peak_memory_stats(dev)
        sync()
        t_start = last[0] = time.perf_counter()
        res = benchmarks.benchmark_portfolios(cfg, chars, barra, wealth, rf, dev,
                                              keep_weights=keep, clock=clock)
        sync()
        t_end = time.perf_counter()
        marks["frames"] = t_end - last[0]
        marks["total"] = t_end - t_start
        marks["peak_bytes"] = int(torch.cuda.max_memory_allocated(dev)) if cuda else 0
        return res, marks

    def timed(fn):
        sync()
        t = time.perf_counter()
        r = fn()
        sync()
        return time.perf_counter() - t, r

    for label, extra in (("default", []), ("reference_grid", REFERENCE_GRID)):
        cfg = base.override(extra)
        cfg.run.compat_mode, cfg.run.plots = False, False
        one_run(cfg)                                              # warm-up
        runs = [one_run(cfg) for _ in range(a.reps)]
        bmk = runs[-1][0]["bmk"]
        keys = ("point", "summands", "prediction", "solve", "guard", "stats", "frames", "total")
        med = {k: float(np.median([m[k] for _, m in runs])) for k in keys}
        rec = {"rows": len(bmk), "sigma_arms": len(bmk) - 2,
               "after_point_inputs_s": round(med["total"], 4),
               "after_point_inputs_s_all": [round(m["total"], 4) for _, m in runs],
               "portfolio_ml_backtest_s": round(med["point"], 4),
               "summands_s": round(med["summands"], 4),
               "prediction_grid_s": round(med["prediction"], 4),
               "prepare_chain_s": round(med["solve"], 4), "guard_s": round(med["guard"], 4),
               "stats_frames_s": round(med["stats"] + med["frames"], 4),
               "peak_device_bytes": int(np.median([m["peak_bytes"] for _, m in runs])),
               "reasons": [r for r in bmk["reason"] if r],
               "table": bmk[["type", "r", "sd", "tc", "r_tc", "obj"]].round(6).to_dict("records")}
        del runs
        # ---- A/B: the factor-structured chain against the dense route, alternating --------
        mu_hat = torch.as_tensor(one_run(cfg, keep=True)[0]["mu_hat"], device=dev)
        ops = benchmarks.sigma_operands(cfg, pt["plan"], barra, layout, mu_hat, wealth)
        arms = list(range(len(ops["names"])))
        rec["split_ratio_max"] = float(ops["split_ratio"].max())

        def fast():
            return benchmarks._solve_arms(ops, arms, dev)

        def dense():
            return benchmarks._dense_arms(ops, arms, dev)

        def prepare():
            return factor_prepare(ops["bX"], ops["ridx"], ops["F"], ops["fscale"], ops["d"],
                                  ops["n_rows"])

        _, rf_ = timed(fast)
        _, rd_ = timed(dense)
        scale = float(rd_[1].abs().max())
        diff = float((rf_[1] - rd_[1]).abs().max())
        flagged = int(rf_[2].sum())
        del rf_, rd_
        tf, td, tp = [], [], []
        for _ in range(max(a.reps, 5)):
            tf.append(timed(fast)[0])
            td.append(timed(dense)[0])
            tp.append(timed(prepare)[0])
        gain = float(np.median(td) - np.median(tf))
        spread = max(max(tf) - min(tf), max(td) - min(td))
        rec["solve_ab"] = {
            "factor_ms": [round(1e3 * x, 3) for x in tf],
            "dense_ms": [round(1e3 * x, 3) for x in td],
            "factor_median_ms": round(1e3 * float(np.median(tf)), 3),
            "prepare_alone_median_ms": round(1e3 * float(np.median(tp)), 3),
            "prepare_systems": int(ops["d"].shape[0] * ops["d"].shape[1]),
            "dense_median_ms": round(1e3 * float(np.median(td)), 3),
            "gain_ms": round(1e3 * gain, 3), "larger_spread_ms": round(1e3 * spread, 3),
            "gain_over_spread": round(gain / max(spread, 1e-12), 2),
            "margin_5x_met": bool(gain >= 5.0 * spread),
            "speedup": round(float(np.median(td) / np.median(tf)), 2),
            "max_abs_weight_difference": diff, "max_abs_weight": scale,
            "flagged_systems_arms": flagged}
        out["runs"][label] = rec
        print(json.dumps({label: rec}), flush=True)
        del ops
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
