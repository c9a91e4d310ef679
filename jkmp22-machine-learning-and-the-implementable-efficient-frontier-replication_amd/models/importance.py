"""Economic feature importance of Portfolio-ML (Jensen, Kelly, Malamud & Pedersen, the
feature-theme figure): how much realised utility is lost when one theme (cluster) of
characteristics carries no information.

The counterfactual of an arm (theme, draw): within every OOS month the theme's characteristics
are permuted across the stocks of the month's signal universe, the random-feature signals are
rebuilt, and the aim portfolios and the weight recursion are re-run with the ESTIMATED
coefficients and the CHOSEN hyper-parameters of the unpermuted benchmark.  The characteristics
enter S4 only through the lag-0 signals of the OOS months (m_tilde, a, the vol scales, the
universes and the coefficients do not depend on them), so S4, the grid search and the
selection run once - exactly one frontier point at the configured wealth and gamma - and the
1 + C D portfolios (benchmark, C themes, D draws) differ only in their aim vectors: they share
every month's m_tilde, which ``portfolio._chain_multi`` reads once for all of them.
"""
from __future__ import annotations

import os

import numpy as np
import pandas as pd
import torch

from ..config import Config, get_features
from ..ops.panel import rff_features, standardize_signals
from ..ops.pfstats import STAT_COLUMNS, pf_stats
from ..utils.dates import month_end, pfml_date_grids
from ..utils.log import COUNTERS, get_logger
from . import frontier, portfolio
from . import pfml_inputs as pin
from .risk import BarraCov

log = get_logger("importance")

FI_COLUMNS = ["cluster", "draw", "n_features"] + frontier.SUMMARY_COLUMNS + ["obj_drop", "reason"]
FI_PF_COLUMNS = ["cluster", "draw", "inv", "shorting", "turnover", "r", "tc", "eom_ret"]
BM = "bm"

WORLD_ERROR = ("feature_importance runs at world size 1: start it in one process (the arms "
               "share one S4 run and one weight chain)")


def month_permutations(seed: int, draw: int, ns) -> list:
    """The permutations of one draw, one per OOS month in month order:
    ``np.random.default_rng([seed, draw]).permutation(n_t)``.  Drawn on the host, so the CPU
    and the device runs permute alike; one set per draw serves every theme (common random
    numbers)."""
    rng = np.random.default_rng([int(seed), int(draw)])
    return [rng.permutation(int(n)) for n in ns]


def theme_columns(labels: pd.DataFrame | None, clusters=None) -> list:
    """[(cluster name, [feature column positions])] in name order.  ``clusters``: None (every
    cluster of ``labels`` with a characteristic among get_features(); one without is skipped),
    a list of names of ``labels``, or {name: [characteristic names]} (kept as given, an empty
    theme included)."""
    feats = get_features()
    pos = {f: i for i, f in enumerate(feats)}
    if isinstance(clusters, dict):
        out = []
        for name in sorted(clusters):
            unknown = [c for c in clusters[name] if c not in pos]
            if unknown:
                raise KeyError(f"theme {name!r}: unknown characteristic(s) {unknown[:3]}")
            out.append((str(name), sorted(pos[c] for c in clusters[name])))
        return out
    if labels is None:
        raise ValueError("feature_importance needs the cluster labels or a dict of themes")
    names = sorted(set(labels["cluster"])) if clusters is None else sorted(clusters)
    out = []
    for name in names:
        members = labels.loc[labels["cluster"] == name, "characteristic"]
        cols = sorted(pos[c] for c in members if c in pos)
        if cols:
            out.append((str(name), cols))
        elif clusters is not None:
            raise KeyError(f"cluster {name!r} has no characteristic among the features")
    return out


class _OosSignals:
    """The lag-0 signal operands of the OOS months, gathered once from the S4 plan: the
    feature rows of every month's signal universe (``signal_rows[t]``, id order) side by side
    in one table, their vol scales, and the padded row index of ``standardize_signals``.
    ``aims`` rebuilds signals and aims for one arm from a permuted copy of the table."""

    def __init__(self, plan: pin.S4Plan, cfg: Config, layout: dict, meta: list,
                 coefs: torch.Tensor):
        dev = plan.feats.device
        self.plan, self.cfg, self.layout, self.meta, self.coefs = plan, cfg, layout, meta, coefs
        self.dev = dev
        B = len(meta)
        where = {}
        for kb, bt in enumerate(plan.batches):
            for bi, d in enumerate(bt.months):
                where[int(d)] = (kb, bi)
        rows, ns = [], []
        for t in range(B):
            kb, bi = where[int(plan.months[meta[t][1]])]
            bt = plan.batches[kb]
            n = int(bt.ns[bi])
            rows.append(bt.idx[bi, 0, :n])
            ns.append(n)
        self.ns = np.asarray(ns, np.int64)
        self.offs = np.concatenate([[0], np.cumsum(self.ns)]).astype(np.int64)
        R = int(self.offs[-1])
        self.R = R
        rows = torch.cat(rows) if rows else torch.zeros(0, dtype=torch.int64, device=dev)
        self.F0 = plan.feats.index_select(0, rows)                    # [R, k (even)]
        vol = pin._vol_device(plan)
        self.vol = torch.cat([vol.index_select(0, rows),
                              torch.ones(1, dtype=torch.float64, device=dev)])
        N = plan.N
        idx = np.full((B, 1, N), R, np.int64)                         # pad -> the zero row R
        for t in range(B):
            idx[t, 0, :ns[t]] = self.offs[t] + np.arange(ns[t])
        self.idx = torch.as_tensor(idx, device=dev)
        self.mask = torch.as_tensor((np.arange(N)[None, :] < self.ns[:, None]).astype(np.float64),
                                    device=dev)
        self.n_real = torch.as_tensor(self.ns, dtype=torch.int32, device=dev)
        # months by the W block of their chosen g (one block under quirk Q1)
        blocks: dict = {}
        for t, m in enumerate(meta):
            blocks.setdefault(m[0] if plan.Gc > 1 else 0, []).append(t)
        self.blocks = {g: np.asarray(ts, np.int64) for g, ts in blocks.items()}

    def source_rows(self, perms: list) -> torch.Tensor:
        """Table row whose theme columns row r takes: offs[t] + pi_t(i) for row i of month t."""
        if len(perms) != len(self.ns) or any(len(p) != n for p, n in zip(perms, self.ns)):
            raise ValueError("one permutation of n_t per OOS month expected")
        src = np.concatenate([self.offs[t] + np.asarray(p, np.int64)
                              for t, p in enumerate(perms)] + [np.zeros(0, np.int64)])
        return torch.as_tensor(src, device=self.dev)

    def aims(self, cols: list, src: torch.Tensor) -> torch.Tensor:
        """wa [B, N] of the arm whose feature columns ``cols`` come from table rows ``src``."""
        plan, P, Pp = self.plan, self.plan.P, self.plan.Pp
        Fp = self.F0.clone()
        if cols:
            ct = torch.as_tensor(np.asarray(cols, np.int64), device=self.dev)
            Fp[:, ct] = self.F0.index_select(0, src).index_select(1, ct)
        sig = [None] * len(self.meta)
        for g, ts in self.blocks.items():
            rff = rff_features(Fp, plan.Wd[g], self.cfg.run.precision, width=Pp, pad_rows=1)
            tt = torch.as_tensor(ts, device=self.dev)
            S = torch.empty((len(ts), 1, plan.N, Pp), dtype=torch.float64, device=self.dev)
            standardize_signals(rff, self.idx.index_select(0, tt), self.mask.index_select(0, tt),
                                self.vol, P=P, out=S, n_real=self.n_real.index_select(0, tt))
            del rff
            for k, t in enumerate(ts):
                sig[t] = S[k, 0, : int(self.ns[t]), :P]
        return portfolio.layout_aims(sig, self.coefs, [m[2] + 1 for m in self.meta],
                                     self.layout, self.dev)


def _chain_arms(mt_all, a_all, wa, layout: dict, to=None):
    """The recursion of all arms on the device of ``mt_all`` (``to``: move the result there)."""
    dev = mt_all.device
    args = (layout[k].to(dev) for k in ("grow", "nmap", "hit", "ws0"))
    Wst, Wopt, _ = portfolio._chain_multi(mt_all, a_all, wa.to(dev), *args)
    return (Wst, Wopt) if to is None else (Wst.to(to), Wopt.to(to))


def feature_importance(cfg: Config, chars: pd.DataFrame, barra: BarraCov, wealth: pd.DataFrame,
                       risk_free: pd.DataFrame, labels: pd.DataFrame | None, device,
                       n_draws: int | None = None, seed: int | None = None, clusters=None,
                       keep_weights: bool = False, clock=None) -> dict:
    """Realised utility of Portfolio-ML with each theme's characteristics permuted, against
    the unpermuted benchmark -> {"fi": one row per arm (bm first, then (cluster, draw) in
    cluster-name order), "pf": the arms' monthly series stacked, "chosen": {hp year: (g, p,
    l)} of the benchmark, "weights": {(cluster, draw): weights frame} with ``keep_weights``}.

    The benchmark is one frontier point at the configured pf_set.wealth / gamma_rel with the
    given wealth frame (``frontier.point_inputs``: S4 with the OOS months' m_tilde kept, the
    guarded grid search, ``select_hps``, ``backtest_layout``), and its arm reproduces
    ``portfolio.backtest_device`` bitwise.  Arm (theme, draw): in OOS month t stock i of the
    month's signal universe takes the theme's characteristics of stock pi_t(i) of the same
    month (``month_permutations(seed, draw, n)``; one set per draw for all themes) and keeps
    its other characteristics and its own vol scale; signals by ``rff_features`` with the W of
    the g chosen for the month and ``standardize_signals`` over the month's universe, aims with
    the benchmark's coefficient rows.  Arms are processed one at a time (one OOS signal block
    of scratch); ONE ``_chain_multi`` advances all of them, ``pf_stats`` runs on the
    [(A B), N] view and ``pf_summary`` per arm.

    Failure guard (as ``backtest_device``): arms whose live w_start is non-finite are
    recomputed on the CPU; an arm that stays non-finite is reported as a NaN row with a
    ``reason``, the other arms stand.  ``n_draws`` / ``seed`` / ``clusters`` default to
    ``settings["fi"]`` (seed: ``settings["seed_no"]``).  ``fi`` columns: cluster, draw,
    n_features, the pf_summary columns, obj_drop (the benchmark's obj minus the arm's; 0 for
    bm), reason.  ``clock(name)`` is called after each phase (tools/bench_importance.py).
    One process only."""
    from ..parallel.dist import env as dist_env
    if dist_env().world_size > 1:
        raise RuntimeError(WORLD_ERROR)
    tick = clock or (lambda name: None)
    fi_set = cfg.settings.get("fi", {})
    n_draws = int(fi_set.get("n_draws", 1) if n_draws is None else n_draws)
    if seed is None:
        seed = fi_set.get("seed")
    seed = int(cfg.settings["seed_no"] if seed is None else seed)
    clusters = fi_set.get("clusters") if clusters is None else clusters
    themes = theme_columns(labels, clusters)
    dev = torch.device(device)
    f64 = dict(dtype=torch.float64, device=dev)
    s = cfg.settings
    grids = pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                            s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                            s["pf"]["dates"]["split_years"])
    gamma = float(cfg.pf_set["gamma_rel"])

    # ---- the benchmark point: S4, grid search, selection - once ------------------------
    ctx: dict = {}
    pt = frontier.point_inputs(cfg, chars, barra, wealth, risk_free, dev, grids, ctx, clock)
    plan, res, grid, layout = pt["plan"], pt["res"], pt["grid"], ctx["layout"]
    meta, coefs, chosen = portfolio.chosen_coefs(cfg, grid, layout, dev)
    months, B, N = layout["months"], layout["B"], layout["N"]
    sig = [res.signal_t[m[0]][m[1]] for m in meta]
    nk = [m[2] + 1 for m in meta]
    arms = [(BM, 0, 0)]                                   # (cluster, draw, n_features)
    was = [portfolio.layout_aims(sig, coefs, nk, layout, dev)]
    mt_all, a_all = portfolio.layout_m(res, layout, dev)
    del sig, grid
    tick("benchmark")

    # ---- the arms' aims, one arm at a time ---------------------------------------------
    if themes and n_draws > 0:
        oos_sig = _OosSignals(plan, cfg, layout, meta, coefs)
        for draw in range(n_draws):
            src = oos_sig.source_rows(month_permutations(seed, draw, oos_sig.ns))
            for name, cols in themes:
                was.append(oos_sig.aims(cols, src))
                arms.append((name, draw, len(cols)))
        del oos_sig
    wa = torch.stack(was)                                  # [A, B, N]
    del was, res, plan, pt, ctx
    A = len(arms)
    tick("aims")

    # ---- one chain over all arms, the failure guard ------------------------------------
    live = layout["live"]
    Wst, Wopt = _chain_arms(mt_all, a_all, wa, layout)
    if cfg.run.fault_inject.startswith("pfml-fi") and B:
        Wst[A - 1, B // 2, 0] = float("nan")
        COUNTERS.add("fault_injected")
    reasons = [""] * A
    bad = torch.nonzero(~portfolio.finite_arms(Wst, live)).flatten()
    if bad.numel():
        names = [f"{arms[k][0]}/{arms[k][1]}" for k in bad.tolist()]
        log.warning(f"non-finite w_start in arm(s) {names}: recomputed on the CPU")
        COUNTERS.add("pfml_fi.recomputed_arms", int(bad.numel()))
        Wst_c, Wopt_c = _chain_arms(mt_all.cpu(), a_all.cpu(), wa[bad].cpu(), layout, to=dev)
        Wst[bad], Wopt[bad] = Wst_c, Wopt_c
        still = ~portfolio.finite_arms(Wst_c, live)
        for k in bad[still].tolist():
            reasons[k] = "w_start stays non-finite on the CPU recursion"
            log.warning(f"arm {arms[k][0]}/{arms[k][1]}: {reasons[k]}")
    # rows with a missing aim stay NaN like the reference's merge would leave them
    Wopt = torch.where(torch.isnan(wa), wa, Wopt)
    tick("chain")

    # ---- statistics on the [(A B), N] view, the frames ---------------------------------
    wvals = torch.as_tensor(portfolio._month_values(wealth, "wealth", months), **f64)
    stats = pf_stats(Wopt.view(A * B, N), Wst.view(A * B, N), layout["ret"].repeat(A, 1),
                     layout["lam"].repeat(A, 1), layout["n_rows"].repeat(A), wvals.repeat(A))
    stats_h = stats.cpu().numpy().reshape(A, B, len(STAT_COLUMNS))
    tick("stats")
    eom = month_end(months)
    eom_ret = eom if cfg.run.compat_mode else eom + pd.offsets.MonthEnd(1)    # quirk Q3
    rows, pfs, weights = [], [], {}
    nan_row = {c: float("nan") for c in frontier.SUMMARY_COLUMNS}
    for k, (name, draw, nf) in enumerate(arms):
        row = {"cluster": name, "draw": draw, "n_features": nf}
        if reasons[k]:
            row.update(nan_row, type="Portfolio-ML", n=0)
        else:
            pf = pd.DataFrame(stats_h[k], columns=list(STAT_COLUMNS))
            pf["eom_ret"] = eom_ret
            row.update(portfolio.pf_summary(pf, gamma).iloc[0].to_dict())
            pfs.append(pf.assign(cluster=name, draw=draw)[FI_PF_COLUMNS])
            if keep_weights:
                pl = layout["plan"]
                weights[(name, draw)] = pd.DataFrame({
                    "eom": month_end(pl["data"]["mi"].to_numpy()),
                    "mu_ld1": layout["mu"][pl["trow"]], "id": pl["ids"],
                    "tr_ld1": pl["data"]["tr_ld1"].to_numpy(np.float64),
                    "w_start": Wst[k][live].cpu().numpy(), "w": Wopt[k][live].cpu().numpy()})
        row["reason"] = reasons[k]
        rows.append({c: (v.item() if isinstance(v, np.generic) else v) for c, v in row.items()})
    fi = pd.DataFrame(rows, columns=[c for c in FI_COLUMNS if c != "obj_drop"])
    fi["obj_drop"] = float(fi["obj"].iloc[0]) - fi["obj"]
    fi = fi[FI_COLUMNS]
    out = {"fi": fi, "chosen": chosen, "stats": stats_h, "months": months,
           "pf": pd.concat(pfs, ignore_index=True) if pfs else pd.DataFrame(columns=FI_PF_COLUMNS)}
    if keep_weights:
        out["weights"] = weights
        out["aims"] = wa.cpu().numpy()                     # [A, B, N], the chain's layout
    return out


def plot_importance(fi: pd.DataFrame, out_dir: str) -> list[str]:
    """plots/feature_importance.png: one bar per theme, the mean obj_drop over its draws,
    sorted.  Skipped without matplotlib."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        log.info("matplotlib not available: plot skipped")
        return []
    os.makedirs(out_dir, exist_ok=True)
    drop = fi[fi["cluster"] != BM].groupby("cluster")["obj_drop"].mean().sort_values()
    fig, ax = plt.subplots(figsize=(6, max(2.0, 0.3 * len(drop) + 1.0)))
    ax.barh([str(c) for c in drop.index], drop.to_numpy(float))
    ax.set_xlabel("drop in realised utility (annualised)")
    f = os.path.join(out_dir, "feature_importance.png")
    fig.tight_layout()
    fig.savefig(f, dpi=100)
    plt.close(fig)
    return [f]
