#!/usr/bin/env python
"""Multiperiod-ML (models/multiperiod.py) at production shape: 500 stocks (N = 490), the 516 OOS
months of the default date grid, K = 12 horizons, A = 1 and A = 3 arms.

The Portfolio-ML point (S4, grid search, layout) is computed once and handed to every run, so a
run is the part of the stage after ``frontier.point_inputs``.  Recorded, as medians of
``--reps`` runs (device synchronised at every mark):
  * seconds after the point by phase: the Portfolio-ML backtest, the horizon targets with the
    summands, the K grid searches with mu_hat, fold + chain, the guard, statistics and frames;
  * an A/B in this process, the arms alternating, on the run's own operands: ``horizon_fold`` +
    ``mp_chain`` against the torch route (one ``baddbmm`` over the months per horizon, then the
    Python-loop chain with one matmul per month), each arm's spread (max - min), the project's
    margin (gain >= 5 x the larger spread) and the largest difference of the weights;
  * the fold alone: achieved bytes/s counting m_tilde once (B n^2 8 bytes) against the 6.3 TB/s
    the chip sustains, and its time at K = 2, 3, 6 (the cost of a further pass over m_tilde).

    python tools/bench_multiperiod.py --out profiles/r31_multiperiod.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SUSTAINED = 6.3e12


def torch_fold(mt, a, mu, wealth, gbar):
    b = (a[None] * mu) / wealth[None, :, None]
    v = b[-1]
    for tau in range(mu.shape[0] - 2, -1, -1):
        v = torch.baddbmm(b[tau][..., None], mt, v[..., None], alpha=gbar)[..., 0]
    return v


def torch_chain(mt, a, V, u, grow, nmap, hit, ws0):
    A, (B, N) = len(u), a.shape
    Wst = torch.zeros((A, B, N), dtype=a.dtype, device=a.device)
    Wopt = torch.zeros_like(Wst)
    ws = ws0.expand(A, N)
    for t in range(B):
        Wst[:, t] = ws
        wopt = a[t] * torch.matmul(ws / a[t] + u[:, None] * V[t], mt[t].T)
        Wopt[:, t] = wopt
        ws = (wopt * grow[t])[:, nmap[t]] * hit[t]
    return Wst, Wopt


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
    from pfml.models import frontier, multiperiod, portfolio
    from pfml.ops.multiperiod import horizon_fold, mp_chain
    from pfml.utils.dates import pfml_date_grids
    dev = torch.device(a.device)
    cuda = dev.type == "cuda"

    def sync():
        if cuda:
            torch.cuda.synchronize(dev)

    base = Config.default().override(a.set)
    base.run.compat_mode = False
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
        return dict(pt)

    frontier.point_inputs = handed
    out = {"metric": "Multiperiod-ML after the Portfolio-ML point, wall-clock",
           "device": torch.cuda.get_device_name(dev) if cuda else "cpu",
           "stocks": a.stocks, "N": int(layout["N"]), "oos_months": int(layout["B"]),
           "K": multiperiod.horizons(base), "reps": a.reps,
           "point_inputs_s_cold": round(point_s, 3), "runs": {}}

    def one_run(cfg, keep=False):
        marks, last = {}, [0.0]

        def clock(name):
            sync()
            t = time.perf_counter()
            marks[name] = t - last[0]
            last[0] = t

        sync()
        t_start = last[0] = time.perf_counter()
        res = multiperiod.multiperiod_portfolios(cfg, chars, barra, wealth, rf, dev,
                                                 keep_weights=keep, clock=clock)
        sync()
        t_end = time.perf_counter()
        marks["frames"] = t_end - last[0]
        marks["total"] = t_end - t_start
        return res, marks

    def timed(fn):
        sync()
        t = time.perf_counter()
        r = fn()
        sync()
        return time.perf_counter() - t, r

    for label, extra in (("A1", ["mp.u=[1]"]), ("A3", ["mp.u=[1,0.5,0.25]"])):
        cfg = base.override(extra)
        cfg.run.compat_mode, cfg.run.plots = False, False
        one_run(cfg)                                              # warm-up
        runs = [one_run(cfg) for _ in range(a.reps)]
        mp = runs[-1][0]["mp"]
        keys = ("point", "summands", "prediction", "solve", "guard", "stats", "frames", "total")
        med = {k: float(np.median([m[k] for _, m in runs])) for k in keys}
        rec = {"rows": len(mp), "after_point_inputs_s": round(med["total"], 4),
               "after_point_inputs_s_all": [round(m["total"], 4) for _, m in runs],
               "portfolio_ml_backtest_s": round(med["point"], 4),
               "targets_summands_s": round(med["summands"], 4),
               "prediction_grids_s": round(med["prediction"], 4),
               "fold_chain_s": round(med["solve"], 4), "guard_s": round(med["guard"], 4),
               "stats_frames_s": round(med["stats"] + med["frames"], 4),
               "reasons": [r for r in mp["reason"] if r],
               "table": mp[["type", "u", "r", "sd", "tc", "r_tc", "obj"]].round(6)
               .to_dict("records")}
        del runs
        # ---- A/B: the kernels against the torch route, alternating ------------------------
        res = one_run(cfg, keep=True)[0]
        f64 = dict(dtype=torch.float64, device=dev)
        mu_hat = torch.as_tensor(res["mu_hat"], **f64)
        mt, av = res["m"]
        wv = torch.as_tensor(portfolio._month_values(wealth, "wealth", layout["months"]), **f64)
        us = torch.as_tensor([u for _, u in multiperiod.mp_arms(cfg)], **f64)
        gbar = float(cfg.settings["mp"]["gbar"])
        n_rows, grow, nmap, hit, ws0 = (layout[k] for k in ("n_rows", "grow", "nmap", "hit",
                                                            "ws0"))
        live = layout["live"]
        full = bool((n_rows == layout["N"]).all())      # the torch route has no row mask
        zero = torch.zeros((), **f64)
        a_t = torch.where(live, av, torch.ones((), **f64))
        mt_t = torch.where(live[:, :, None] & live[:, None, :], mt, zero).contiguous()
        mu_t = torch.where(live[None], mu_hat, zero)

        def fast():
            V = horizon_fold(mt, av, mu_hat, wv, n_rows, gbar)
            return mp_chain(mt, av, V, us, n_rows, grow, nmap, hit, ws0)[:2]

        def slow():
            V = torch_fold(mt_t, a_t, mu_t, wv, gbar)
            return torch_chain(mt_t, a_t, V, us, grow, nmap, hit, ws0)

        def fold_only():
            return horizon_fold(mt, av, mu_hat, wv, n_rows, gbar)

        _, rf_ = timed(fast)
        _, rs_ = timed(slow)
        scale = float(rs_[1].abs().max())
        diff = float(torch.where(live[None], rf_[1] - rs_[1], zero).abs().max())
        del rf_, rs_
        tf, ts, tfo = [], [], []
        for _ in range(max(a.reps, 5)):
            tf.append(timed(fast)[0])
            ts.append(timed(slow)[0])
            tfo.append(timed(fold_only)[0])
        gain = float(np.median(ts) - np.median(tf))
        spread = max(max(tf) - min(tf), max(ts) - min(ts))
        nn = n_rows.to(torch.float64)
        m_bytes = float((nn * nn).sum()) * 8.0
        fo = float(np.median(tfo))
        rec["fold_chain_ab"] = {
            "kernels_ms": [round(1e3 * x, 3) for x in tf],
            "torch_ms": [round(1e3 * x, 3) for x in ts],
            "kernels_median_ms": round(1e3 * float(np.median(tf)), 3),
            "torch_median_ms": round(1e3 * float(np.median(ts)), 3),
            "gain_ms": round(1e3 * gain, 3), "larger_spread_ms": round(1e3 * spread, 3),
            "gain_over_spread": round(gain / max(spread, 1e-12), 2),
            "margin_5x_met": bool(gain >= 5.0 * spread),
            "speedup": round(float(np.median(ts) / np.median(tf)), 2),
            "max_abs_weight_difference": diff, "max_abs_weight": scale,
            "every_month_full_width": full}
        rec["fold_alone"] = {
            "ms": [round(1e3 * x, 3) for x in tfo], "median_ms": round(1e3 * fo, 3),
            "m_tilde_bytes_once": m_bytes,
            "achieved_bytes_per_s_m_once": m_bytes / fo,
            "floor_ms_at_sustained_hbm": round(1e3 * m_bytes / HBM_SUSTAINED, 4),
            "fraction_of_sustained_hbm": round(m_bytes / fo / HBM_SUSTAINED, 4)}
        # the same launch at fewer horizons: K - 1 passes over m_tilde; the slope per pass tells
        # whether the passes after the first are served by a cache or by HBM again
        by_k = {}
        for Kk in sorted({2, 3, 6, int(mu_hat.shape[0])}):
            if Kk > mu_hat.shape[0]:
                continue
            mu_k = mu_hat[:Kk].contiguous()
            horizon_fold(mt, av, mu_k, wv, n_rows, gbar)
            tk = [timed(lambda: horizon_fold(mt, av, mu_k, wv, n_rows, gbar))[0]
                  for _ in range(max(a.reps, 5))]
            by_k[str(Kk)] = round(1e3 * float(np.median(tk)), 3)
        rec["fold_alone"]["median_ms_by_K"] = by_k
        out["runs"][label] = rec
        print(json.dumps({label: rec}), flush=True)
        del res, mu_hat, mt_t
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
