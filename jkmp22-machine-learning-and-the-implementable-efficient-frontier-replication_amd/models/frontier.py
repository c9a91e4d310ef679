"""The implementable efficient frontier: Portfolio-ML re-estimated at every point of the
wealth x gamma grid (``settings["ef"]``).

m_func depends on both the wealth level and the risk aversion, so a frontier point is a full
S4 (PFML inputs) -> S5/S6 (grid search, scores) -> S7-S9 (aims, weight recursion, portfolio
statistics) run.  The reference never runs it (1-1.5 h of CPU per point); here a point stays
on the device from the panel to its per-month statistics (``portfolio.backtest_device``), and
the only host work that is repeated per point is the S4 layout.
"""
from __future__ import annotations

import copy
import dataclasses
import json
import os
import time

import numpy as np
import pandas as pd
import torch

from ..config import Config
from ..utils.dates import month_index, pfml_date_grids
from ..utils.log import COUNTERS, get_logger
from . import pfml_inputs as pin
from . import portfolio, search
from .risk import BarraCov

log = get_logger("frontier")

SUMMARY_COLUMNS = ["type", "n", "inv", "shorting", "turnover_notional", "r", "sd", "sr_gross",
                   "tc", "r_tc", "sr", "obj"]
DIAG_COLUMNS = ["s4_repairs", "s4_fallbacks", "grid_recomputed_cells", "seconds"]
EF_COLUMNS = ["wealth_end", "gamma_rel"] + SUMMARY_COLUMNS + DIAG_COLUMNS
PF_COLUMNS = ["wealth_end", "gamma_rel", "inv", "shorting", "turnover", "r", "tc", "eom_ret"]

# months per re-run of the m_func repair path (pfml_inputs.finish_inputs re-runs every flagged
# month as ONE batch; at wealth ~ 1 the device's Denman-Beavers convergence check flags every
# month - cond(x^2 + 4x) is beyond 1e16 there - and a one-batch reference-form repair of ~700
# months at N = 500 does not fit the batched-LU workspace)
REPAIR_CHUNK = 32

WORLD_ERROR = ("efficient_frontier runs at world size 1: start it in one process (spreading "
               "the points over GPUs needs a process group per rank)")


def point_config(cfg: Config, wealth_end: float, gamma_rel: float) -> Config:
    """cfg with pf_set.wealth / pf_set.gamma_rel of the frontier point."""
    c = copy.deepcopy(cfg)
    c.pf_set["wealth"] = wealth_end
    c.pf_set["gamma_rel"] = gamma_rel
    return c


def frame_end_wealth(cfg: Config, wealth: pd.DataFrame) -> float:
    """The wealth frame's value at split.test_end (the end wealth it was built from)."""
    end = int(month_index(cfg.settings["split"]["test_end"])[0])
    at = np.nonzero(month_index(wealth["eom"]) == end)[0]
    if len(at) == 0:
        raise ValueError("the wealth frame has no row at split.test_end")
    return float(wealth["wealth"].to_numpy(np.float64)[at[0]])


def scaled_wealth(cfg: Config, wealth: pd.DataFrame, wealth_end: float) -> pd.DataFrame:
    """The wealth path of a frontier point: the given frame with ``wealth`` multiplied by the
    single factor wealth_end / (the frame's value at split.test_end); mu_ld1 unchanged.
    ``prep.wealth_func`` is linear in its end wealth (cumprod(1 - tret) * wealth_end), so this
    equals wealth_func(wealth_end, ...) up to one rounding per month, and it is bitwise the
    frame itself when wealth_end is the frame's own end wealth (the factor is exactly 1.0)."""
    out = wealth.copy()
    out["wealth"] = wealth["wealth"].to_numpy(np.float64) * (
        float(wealth_end) / frame_end_wealth(cfg, wealth))
    return out


def _guard_inputs(cfg: Config, data: tuple, wealth_pt: pd.DataFrame, res, months, device) -> int:
    """The pfml-input stage's failure guard: months whose summands are not finite are
    recomputed, on the device then on the fp64 CPU path.  Returns the number of such months."""
    chars, barra, risk_free = data
    R = res.reals
    if cfg.run.fault_inject.startswith("pfml-input") and len(months):
        R.denom[:, 0, 0, 0] = float("nan")
        COUNTERS.add("fault_injected")
    bad = ~(torch.isfinite(R.denom).flatten(2).all(-1) & torch.isfinite(R.r_tilde).all(-1))
    bad_t = torch.nonzero(bad.any(0)).flatten().cpu().numpy()
    if len(bad_t) == 0:
        return 0
    log.warning(f"non-finite PFML inputs in {len(bad_t)} month(s): recomputing")
    COUNTERS.add("pfml_input.recomputed_months", len(bad_t))
    for dev in (torch.device(device), torch.device("cpu")):
        redo = pin.build_inputs(cfg, chars, barra, wealth_pt, risk_free, dev,
                                months=months[bad_t])
        ok = (torch.isfinite(redo.reals.denom).flatten(2).all(-1).all(0) &
              torch.isfinite(redo.reals.r_tilde).all(-1).all(0))
        if bool(ok.all()):
            idx = torch.as_tensor(bad_t, device=R.denom.device)
            R.denom[:, idx] = redo.reals.denom.to(R.denom.device)
            R.r_tilde[:, idx] = redo.reals.r_tilde.to(R.r_tilde.device)
            return len(bad_t)
    raise FloatingPointError(f"PFML inputs stay non-finite for months {months[bad_t]}")


def _guard_grid(cfg: Config, grid, reals) -> int:
    """The pfml-search-coef stage's failure guard (one process): cells whose coefficients are
    not finite after the device repair are re-solved on the fp64 CPU path.  Returns the number
    of recomputed cells."""
    if cfg.run.fault_inject.startswith("pfml-search-coef") and grid.beta.shape[1]:
        grid.beta[0, 0, -1, len(grid.l_vec) // 2, 0] = float("nan")
        COUNTERS.add("fault_injected")
    if grid.beta.is_cuda:
        from ..ops.ridge import coop_errors
        nto = coop_errors()
        if nto:
            COUNTERS.add("ridge.coop_timeouts", nto)
            log.warning(f"{nto} cell(s) of the cooperative band reduction timed out: their NaN "
                        "betas are recomputed")
    bad = search.nonfinite_cells(grid)
    if not bad:
        return 0
    log.warning(f"non-finite coefficients in {len(bad)} cell(s): recomputing on the CPU oracle")
    res = search.recompute_cells(grid, reals, bad)
    COUNTERS.add("pfml_search.recomputed_cells", res["recomputed"])
    if res["singular"]:
        COUNTERS.add("pfml_search.singular_cells", res["singular"])
        log.warning(f"{res['singular']} cell(s) singular even for pivoted LU: NaN kept")
    return int(res["recomputed"])


def repoint_s4_plan(plan: pin.S4Plan, cfg_pt: Config, wealth_pt: pd.DataFrame) -> pin.S4Plan:
    """An S4 plan made for one frontier point, re-aimed at another: the plan's host layout
    does not depend on the point apart from each month's wealth and the padding value of
    lambda (gamma / wealth, pfml_inputs.make_s4_plan), so those two tensors are swapped in and
    everything else - index tensors, the panel and Barra copies - is shared.  The operands are
    bitwise those of a fresh ``make_s4_plan`` for the point, hence so are the S4 summands."""
    gamma = float(cfg_pt.pf_set["gamma_rel"])
    wmap = dict(zip(month_index(wealth_pt["eom"]), wealth_pt["wealth"].to_numpy(np.float64)))
    batches = []
    for b in plan.batches:
        w = np.asarray([float(wmap[int(d)]) for d in b.months], np.float64)
        wt = torch.as_tensor(w, dtype=torch.float64, device=b.lam.device)
        pad = torch.as_tensor(gamma / w, dtype=torch.float64, device=b.lam.device)
        lam = torch.where(b.mask > 0, b.lam, pad[:, None].expand_as(b.lam)).contiguous()
        batches.append(dataclasses.replace(b, w=wt, lam=lam))
    return dataclasses.replace(plan, batches=batches)


def _finish_chunked(plan: pin.S4Plan, cfg: Config, out) -> int:
    """``pfml_inputs.finish_inputs`` with the flagged months repaired REPAIR_CHUNK at a time
    (the same per-month arithmetic: the repair is per matrix).  Returns the flagged count."""
    pend = out.pending
    if pend is None or pend["mstat"] is None:
        pin.finish_inputs(plan, cfg, out)
        return 0
    flags = pend["mstat"]
    bad = torch.nonzero(flags).flatten()
    nbad = int(bad.numel())
    if nbad <= REPAIR_CHUNK:
        pin.finish_inputs(plan, cfg, out)
        return nbad
    log.warning(f"S4: {nbad} of {len(plan.months)} month(s) on the m_func repair path, "
                f"repaired {REPAIR_CHUNK} at a time")
    if flags.is_cuda:
        torch.cuda.empty_cache()        # the repair's library workspaces are not torch's
    for c0 in range(0, nbad, REPAIR_CHUNK):
        part = torch.zeros_like(flags)
        part[bad[c0:c0 + REPAIR_CHUNK]] = 1
        out.pending = {"mstat": part, "keep_risk_tc": pend["keep_risk_tc"],
                       "nsing": pend["nsing"] if c0 == 0 else torch.zeros_like(pend["nsing"])}
        pin.finish_inputs(plan, cfg, out)
    return nbad


def run_point(cfg_pt: Config, chars: pd.DataFrame, barra: BarraCov, wealth_pt: pd.DataFrame,
              risk_free: pd.DataFrame, device, grids: dict, ctx: dict,
              keep_weights: bool = False, clock=None) -> dict:
    """One frontier point: S4 for all PFML months (m_tilde of the OOS months kept), the grid
    search, the device-resident backtest.  Returns the backtest result + diagnostics.  ``ctx``
    carries what does not depend on the point from one call to the next: the S4 plan (made by
    the first call, ``repoint_s4_plan`` for every point) and the backtest layout.
    ``clock(name)`` is called after each phase (tools/bench_frontier.py)."""
    c0 = COUNTERS.as_dict()
    pt = point_inputs(cfg_pt, chars, barra, wealth_pt, risk_free, device, grids, ctx, clock)
    bt = portfolio.backtest_device(cfg_pt, pt["grid"], pt["res"], ctx["layout"], wealth_pt,
                                   torch.device(device), keep_weights=keep_weights, clock=clock)
    bt["diag"] = point_diag(c0, pt)
    return bt


def point_inputs(cfg_pt: Config, chars: pd.DataFrame, barra: BarraCov, wealth_pt: pd.DataFrame,
                 risk_free: pd.DataFrame, device, grids: dict, ctx: dict, clock=None) -> dict:
    """Everything of a point in front of its backtest: the (re-aimed) S4 plan, S4 with the OOS
    months' m_tilde kept, the guarded grid search and the backtest layout (``ctx["layout"]``).
    Returns {"plan", "res", "grid", "ridge_rep", "ncell"}."""
    tick = clock or (lambda name: None)
    dev = torch.device(device)
    m2, oos = grids["m2"], grids["oos"]
    if ctx.get("plan") is None:
        ctx["plan"] = pin.make_s4_plan(cfg_pt, chars, barra, wealth_pt, risk_free, dev, m2)
    plan = repoint_s4_plan(ctx["plan"], cfg_pt, wealth_pt)
    tick("s4_plan")
    res = pin.run_plan(plan, cfg_pt, keep_m=oos, defer_checks=True)
    _finish_chunked(plan, cfg_pt, res)
    _guard_inputs(cfg_pt, (chars, barra, risk_free), wealth_pt, res, m2, dev)
    tick("s4")
    R = search.complete_local_reals(res.reals.r_tilde, res.reals.denom, m2, cfg_pt.hp_years)
    grid = search.grid_search(R, cfg_pt, gather=False)
    ridge_rep = 0
    if dev.type == "cuda":
        from ..ops.ridge import repairs_done
        ridge_rep = repairs_done()
    ncell = _guard_grid(cfg_pt, grid, R)
    grid = search.gather_grid(grid)
    tick("grid")
    if ctx.get("layout") is None:
        ctx["layout"] = portfolio.backtest_layout(cfg_pt, chars, wealth_pt, oos, m2, res.ids,
                                                  dev, n_pad=plan.N)
        tick("layout")
    return {"plan": plan, "res": res, "grid": grid, "ridge_rep": ridge_rep, "ncell": ncell}


def point_diag(c0: dict, pt: dict) -> dict:
    """The diagnostics columns of a point: the fallback counters it moved since ``c0``."""
    c1 = COUNTERS.as_dict()
    fb = {k: v - c0.get(k, 0) for k, v in c1.items() if v != c0.get(k, 0)}
    if pt["ridge_rep"]:
        fb["ridge.repairs"] = int(pt["ridge_rep"])
    return {"s4_repairs": int(fb.get("pfml_inputs.mfunc_repaired_months", 0)),
            "s4_fallbacks": json.dumps(fb, sort_keys=True),
            "grid_recomputed_cells": int(pt["ncell"])}


class _Checkpoint:
    """Finished points of a frontier run, appended to one JSON artifact (rewritten atomically
    after every point); a run with the same key continues at the first missing point."""

    def __init__(self, path: str | None, key: str):
        self.path, self.key, self.points = path, key, []
        if path and os.path.exists(path):
            try:
                with open(path, encoding="utf-8") as f:
                    doc = json.load(f)
                if doc.get("key") == key:
                    self.points = doc["points"]
            except (OSError, ValueError, KeyError):
                self.points = []

    def get(self, w: float, g: float):
        for p in self.points:
            if p["wealth_end"] == float(w) and p["gamma_rel"] == float(g):
                return p
        return None

    def add(self, w: float, g: float, row: dict, pf: pd.DataFrame) -> None:
        if not self.path:
            return
        rec = pf.copy()
        rec["eom_ret"] = pd.to_datetime(rec["eom_ret"]).dt.strftime("%Y-%m-%d")
        self.points.append({"wealth_end": float(w), "gamma_rel": float(g), "ef": row,
                            "pf": rec.to_dict(orient="list")})
        os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
        tmp = self.path + ".tmp"
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump({"key": self.key, "points": self.points}, f)
        os.replace(tmp, self.path)


def efficient_frontier(cfg: Config, chars: pd.DataFrame, barra: BarraCov, wealth: pd.DataFrame,
                       risk_free: pd.DataFrame, device, wealth_vec=None, gamma_vec=None,
                       keep_weights: bool = False, *, checkpoint: str | None = None,
                       checkpoint_key: str = "", on_point=None) -> dict:
    """Portfolio-ML at every (wealth, gamma) of the grid -> {"ef": one row per point, "pf": the
    per-point monthly series stacked, "chosen": {(W, gamma): {hp year: (g, p, l)}} of the
    points computed in this call} (plus {"weights": {(W, gamma): frame}} with
    ``keep_weights``).  The grids default to ``settings["ef"]``.

    Per point, one at a time: cfg with pf_set.wealth = W and pf_set.gamma_rel = gamma; the
    wealth path is ``scaled_wealth`` - the given frame times the single factor W / (its value
    at split.test_end), mu_ld1 unchanged, which equals prep.wealth_func(W, ...) up to rounding
    (wealth_func is linear in its end wealth) and is bitwise the given frame when W is the
    frame's own end wealth; then S4 for all PFML months with m_tilde of the OOS months kept,
    the grid search and ``portfolio.backtest_device``.  The point's device buffers are released
    before the next point: peak memory does not grow with the number of points.  The stages'
    failure guards apply (non-finite S4 months, grid cells, w_start); a point that still fails
    is reported with NaN statistics and a logged reason, the other points run on.

    ``ef`` columns: wealth_end, gamma_rel, the pf_summary columns (ddof = 1, annualised, quirk
    Q18), then s4_repairs (m_func months sent to the repair path), s4_fallbacks (JSON of every
    fallback counter the point moved, ridge repairs included), grid_recomputed_cells, seconds.

    ``checkpoint``: path of a JSON artifact of the finished points; an earlier run's points
    with the same ``checkpoint_key`` are reused and the run continues at the first missing one.
    ``on_point(row)`` is called after every computed point (tools/bench_frontier.py).
    One process only: under torch.distributed with more than one rank it raises."""
    from ..parallel.dist import env as dist_env
    if dist_env().world_size > 1:
        raise RuntimeError(WORLD_ERROR)
    ef_set = cfg.settings["ef"]
    wealth_vec = [float(x) for x in (ef_set["wealth"] if wealth_vec is None else wealth_vec)]
    gamma_vec = [float(x) for x in (ef_set["gamma_rel"] if gamma_vec is None else gamma_vec)]
    dev = torch.device(device)
    s = cfg.settings
    grids = pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                            s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                            s["pf"]["dates"]["split_years"])
    ck = _Checkpoint(checkpoint, checkpoint_key)
    ctx: dict = {}
    rows, pfs, weights, chosen = [], [], {}, {}
    for W in wealth_vec:
        for gam in gamma_vec:
            done = ck.get(W, gam)
            if done is not None and not keep_weights:
                log.info(f"point wealth={W:g} gamma={gam:g}: from the checkpoint")
                rows.append(done["ef"])
                pf = pd.DataFrame(done["pf"])
                pf["eom_ret"] = pd.to_datetime(pf["eom_ret"])
                pfs.append(pf)
                continue
            t0 = time.perf_counter()
            cfg_pt = point_config(cfg, W, gam)
            row = {"wealth_end": W, "gamma_rel": gam}
            try:
                wealth_pt = scaled_wealth(cfg, wealth, W)
                bt = run_point(cfg_pt, chars, barra, wealth_pt, risk_free, dev, grids, ctx,
                               keep_weights)
                pf = bt["pf"]
                chosen[(W, gam)] = bt["chosen"]
                row.update(portfolio.pf_summary(pf, gam).iloc[0].to_dict())
                row.update(bt["diag"])
                if keep_weights:
                    weights[(W, gam)] = bt["weights"]
                del bt
            except (FloatingPointError, np.linalg.LinAlgError, RuntimeError,
                    portfolio.NoRankedHyperParameters) as e:
                # numerical failures, and a repair that ran out of device memory; a wrong
                # setting, a device fault or any other runtime error ends the run
                if isinstance(e, RuntimeError) and not (
                        isinstance(e, torch.cuda.OutOfMemoryError) or "ALLOC_FAILED" in str(e)):
                    raise
                if dev.type == "cuda":
                    torch.cuda.empty_cache()
                log.warning(f"point wealth={W:g} gamma={gam:g} failed: {type(e).__name__}: {e}")
                pf = pd.DataFrame({c: [] for c in PF_COLUMNS[2:]})
                row.update({c: float("nan") for c in SUMMARY_COLUMNS + DIAG_COLUMNS})
                row.update(type="Portfolio-ML", n=0, s4_fallbacks=json.dumps(
                    {"failed": f"{type(e).__name__}: {e}"}))
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            row["seconds"] = round(time.perf_counter() - t0, 4)
            row = {k: (v.item() if isinstance(v, np.generic) else v) for k, v in row.items()}
            pf = pf.assign(wealth_end=W, gamma_rel=gam)[PF_COLUMNS]
            rows.append(row)
            pfs.append(pf)
            ck.add(W, gam, row, pf)
            if on_point is not None:
                on_point(row)
            log.info(f"point wealth={W:g} gamma={gam:g}: r_tc={row['r_tc']:.6g} "
                     f"sd={row['sd']:.6g} in {row['seconds']:.2f}s")
    out = {"ef": pd.DataFrame(rows, columns=EF_COLUMNS),
           "pf": pd.concat(pfs, ignore_index=True) if pfs else pd.DataFrame(columns=PF_COLUMNS),
           "chosen": chosen}
    if keep_weights:
        out["weights"] = weights
    return out


def plot_frontier(ef: pd.DataFrame, out_dir: str) -> list[str]:
    """plots/efficient_frontier.png: annualised sd on x, r_tc on y, one line per wealth in
    gamma order.  Skipped without matplotlib."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        log.info("matplotlib not available: plot skipped")
        return []
    os.makedirs(out_dir, exist_ok=True)
    fig, ax = plt.subplots(figsize=(6, 4))
    for W, sub in ef.groupby("wealth_end", sort=True):
        sub = sub.sort_values("gamma_rel")
        ax.plot(sub["sd"], sub["r_tc"], "o-", label=f"wealth {W:g}")
    ax.set_xlabel("volatility (annualised)")
    ax.set_ylabel("return net of TC (annualised)")
    ax.legend()
    f = os.path.join(out_dir, "efficient_frontier.png")
    fig.savefig(f, dpi=100)
    plt.close(fig)
    return [f]
