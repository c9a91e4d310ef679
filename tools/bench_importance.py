#!/usr/bin/env python
"""Feature-theme importance (models/importance.py) at production shape: 500 stocks, the 516 OOS
months of the default date grid, the 13 themes of the synthetic labels, D = 1 and D = 8 draws.

The benchmark point (S4, grid search, layout) is computed once and handed to every run, so a
run is exactly the part of the stage after the benchmark point.  Recorded, as medians of
``--reps`` runs (device synchronised at every mark):
  * seconds of the stage after the benchmark point, split into the arms' signals and aims
    (in total and per arm), the chain, and the statistics with the frames;
  * the peak device memory of a run;
  * an A/B in this process, the arms alternating: ``portfolio._chain_multi`` on the run's A
    aim vectors against A calls of ``portfolio._chain`` on the same operands, with each arm's
    spread (max - min) and the project's margin (gain >= 5 x the larger spread).

    python tools/bench_importance.py --out profiles/r15_importance.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stocks", type=int, default=500)
    ap.add_argument("--draws", default="1,8", help="comma list of D")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--set", action="append", default=[], help="dotted override key=value")
    ap.add_argument("--end", default="2023-12-31", help="last month of the synthetic panel")
    ap.add_argument("--out", default="", help="write the JSON here as well")
    a = ap.parse_args()
    from pfml.config import Config, get_features
    from pfml.data import synthetic as syn
    from pfml.models import frontier, importance, portfolio
    from pfml.utils.dates import pfml_date_grids
    dev = torch.device(a.device)
    cuda = dev.type == "cuda"

    def sync():
        if cuda:
            torch.cuda.synchronize(dev)

    cfg = Config.default().override(a.set)
    cfg.run.compat_mode = False          # distinct RFF draw per g (no rff_w.csv), as bench.py
    cfg.run.plots = False
    chars, barra, wealth, rf = syn.engine_inputs(n_stocks=a.stocks, end=a.end)
    feats = get_features()
    labels = pd.DataFrame({"characteristic": feats, "direction": 1,
                           "cluster": [syn._CLUSTERS[i % len(syn._CLUSTERS)]
                                       for i in range(len(feats))]})
    s = cfg.settings
    grids = pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                            s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                            s["pf"]["dates"]["split_years"])
    sync()
    t0 = time.perf_counter()
    ctx: dict = {}
    pt = frontier.point_inputs(cfg, chars, barra, wealth, rf, dev, grids, ctx)
    sync()
    point_s = time.perf_counter() - t0
    layout = ctx["layout"]

    def handed(cfg_pt, chars_, barra_, wealth_pt, risk_free, device, grids_, ctx_, clock=None):
        ctx_["layout"] = layout
        return pt

    frontier.point_inputs = handed
    out = {"metric": "feature-theme importance after the benchmark point, wall-clock",
           "device": torch.cuda.get_device_name(dev) if cuda else "cpu",
           "stocks": a.stocks, "N": int(layout["N"]), "oos_months": int(layout["B"]),
           "themes": len(importance.theme_columns(labels)), "reps": a.reps,
           "benchmark_point_s_cold": round(point_s, 3), "runs": {}}

    def one_run(D):
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
        res = importance.feature_importance(cfg, chars, barra, wealth, rf, labels, dev,
                                            n_draws=D, seed=1, keep_weights=False, clock=clock)
        sync()
        t_end = time.perf_counter()
        marks["frames"] = t_end - last[0]
        marks["after_benchmark"] = t_end - t_start - marks["benchmark"]
        marks["peak_bytes"] = int(torch.cuda.max_memory_allocated(dev)) if cuda else 0
        return res, marks

    for D in [int(x) for x in a.draws.split(",") if x.strip()]:
        one_run(D)                                            # warm-up
        runs = [one_run(D) for _ in range(a.reps)]
        fi = runs[-1][0]["fi"]
        A = len(fi)
        med = {k: float(np.median([m[k] for _, m in runs]))
               for k in ("aims", "chain", "stats", "frames", "after_benchmark")}
        rec = {"arms": A,
               "after_benchmark_s": round(med["after_benchmark"], 4),
               "after_benchmark_s_all": [round(m["after_benchmark"], 4) for _, m in runs],
               "signals_aims_s": round(med["aims"], 4),
               "signals_aims_ms_per_arm": round(1e3 * med["aims"] / max(A - 1, 1), 3),
               "chain_s": round(med["chain"], 4),
               "stats_frames_s": round(med["stats"] + med["frames"], 4),
               "peak_device_bytes": int(np.median([m["peak_bytes"] for _, m in runs])),
               "finite": bool(np.isfinite(fi["obj"].to_numpy(float)).all()),
               "obj_bm": float(fi["obj"].iloc[0]),
               "obj_drop_mean_by_theme": {
                   str(k): float(v) for k, v in
                   fi[fi["cluster"] != "bm"].groupby("cluster")["obj_drop"].mean().items()}}
        del runs
        # ---- A/B: one multi chain against A single chains, alternating ---------------------
        res, _ = (importance.feature_importance(cfg, chars, barra, wealth, rf, labels, dev,
                                                n_draws=D, seed=1, keep_weights=True), None)
        wa = torch.as_tensor(res["aims"], device=dev)
        del res
        mt_all, a_all = portfolio.layout_m(pt["res"], layout, dev)
        args = (layout["grow"], layout["nmap"], layout["hit"], layout["ws0"])

        def multi():
            return portfolio._chain_multi(mt_all, a_all, wa, *args)

        def singles():
            return [portfolio._chain(mt_all, a_all, wa[k], *args) for k in range(A)]

        def timed(fn):
            sync()
            t = time.perf_counter()
            r = fn()
            sync()
            return time.perf_counter() - t, r

        _, rm = timed(multi)
        _, rs = timed(singles)
        bitwise = all(torch.equal(rm[0][k], rs[k][0]) and torch.equal(rm[1][k], rs[k][1])
                      for k in range(A))
        del rm, rs
        tm, ts = [], []
        for _ in range(max(a.reps, 5)):
            tm.append(timed(multi)[0])
            ts.append(timed(singles)[0])
        gain = float(np.median(ts) - np.median(tm))
        spread = max(max(tm) - min(tm), max(ts) - min(ts))
        rec["chain_ab"] = {
            "multi_ms": [round(1e3 * x, 3) for x in tm],
            "singles_ms": [round(1e3 * x, 3) for x in ts],
            "multi_median_ms": round(1e3 * float(np.median(tm)), 3),
            "singles_median_ms": round(1e3 * float(np.median(ts)), 3),
            "gain_ms": round(1e3 * gain, 3), "larger_spread_ms": round(1e3 * spread, 3),
            "gain_over_spread": round(gain / max(spread, 1e-12), 2),
            "margin_5x_met": bool(gain >= 5.0 * spread),
            "speedup": round(float(np.median(ts) / np.median(tm)), 2),
            "columns_bitwise_equal": bool(bitwise)}
        out["runs"][f"D={D}"] = rec
        print(json.dumps({f"D={D}": rec}), flush=True)
        del wa
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
