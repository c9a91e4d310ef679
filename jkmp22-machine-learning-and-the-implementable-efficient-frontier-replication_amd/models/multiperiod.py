"""Multiperiod-ML (Jensen, Kelly, Malamud & Pedersen): the second dynamic portfolio of the
paper's comparison.  It predicts returns at the horizons 1 .. K and trades towards the closed
form of the multi-period problem with Portfolio-ML's trading-speed matrix m.  No reference
script.

With a = Lambda^-1/2, m = diag(a) m_tilde diag(1/a) (ops/linalg.py), W_t the wealth path and
mu_hat_{t,h} the predicted excess return of month t at horizon h, an OOS month is

    b_tau   = (a_t o mu_hat_{t,tau+1}) / W_t                          tau = 0 .. K-1
    v_{K-1} = b_{K-1};  v_tau = b_tau + gbar (m_tilde_t v_{tau+1})     tau = K-2 .. 0;  V_t := v_0
    w_opt,t = a_t o (m_tilde_t (w_start,t / a_t + u V_t))
    w_start,t+1 = drift of w_opt,t                                    (``portfolio._chain``)

which in w-space is w_t = m g w_{t-1} + sum_tau gbar^tau m^(tau+1) Lambda^-1 u mu_hat_{t,tau+1}
/ W_t: the first-order condition of the Bellman equation whose quadratic term is m_tilde's own
fixed point.  Everything but the two steps above is reuse: S4 keeps m_tilde and a of every OOS
month, ``benchmarks.prediction_reals`` builds the ridge summands of a return model (here one
per horizon on a shared Z'Z), and the grid search, the selection, ``layout_aims``,
``backtest_layout``, ``pf_stats`` and ``pf_summary`` run as they are.  The fold and the chain
are ops/multiperiod.py.

Arms: ``Multiperiod-ML`` (u = 1) and ``Multiperiod-ML(u)`` for every other u of
settings["mp"]["u"].  The (k, g) arms of pf.hps.m1 change Lambda and Sigma and with them
m_tilde itself - an m_func pass each - and are not built.
"""
from __future__ import annotations

import copy

import numpy as np
import pandas as pd
import torch

from ..config import Config
from ..ops.multiperiod import horizon_fold, mp_chain
from ..ops.pfstats import STAT_COLUMNS, pf_stats
from ..utils.dates import month_end, month_index, pfml_date_grids
from ..utils.log import COUNTERS, get_logger
from . import benchmarks, frontier, portfolio, search
from . import pfml_inputs as pin
from .risk import BarraCov

log = get_logger("multiperiod")

MP_COLUMNS = ["type", "u"] + frontier.SUMMARY_COLUMNS[1:] + ["reason"]
MP_PF_COLUMNS = ["type", "u", "inv", "shorting", "turnover", "r", "tc", "eom_ret"]
MP_HPS_COLUMNS = ["horizon"] + benchmarks.BMK_HPS_COLUMNS
NAN = float("nan")

WORLD_ERROR = ("multiperiod_portfolios runs at world size 1: start it in one process (the arms "
               "share one S4 plan and one weight chain)")


def horizons(cfg: Config) -> int:
    """K: settings["mp"]["K"], default pf.hps.m1.K."""
    K = cfg.settings.get("mp", {}).get("K")
    K = int(cfg.settings["pf"]["hps"]["m1"]["K"] if K is None else K)
    if K < 1:
        raise ValueError(f"mp.K must be at least 1, got {K}")
    return K


def mp_config(cfg: Config) -> Config:
    """cfg with the prediction models' grid in pf_ml, as ``benchmarks.bmk_config`` from
    settings["mp"]: l_vec (default settings["rff"]["l_vec"]), p_vec (default pf_ml's)."""
    m = cfg.settings.get("mp", {})
    c = copy.deepcopy(cfg)
    c.settings["bmk"] = {"l_vec": m.get("l_vec"), "p_vec": m.get("p_vec")}
    return benchmarks.bmk_config(c)


def mp_arms(cfg: Config) -> list:
    """[(name, u)]: (``Multiperiod-ML``, 1) first, then every other u of settings["mp"]["u"]."""
    us = [float(x) for x in cfg.settings.get("mp", {}).get("u", [1.0])]
    arms = [("Multiperiod-ML", 1.0)]
    for u in us:
        name = f"Multiperiod-ML({u:g})"
        if u != 1.0 and name not in [n for n, _ in arms]:
            arms.append((name, u))
    return arms


def horizon_targets(chars: pd.DataFrame, plan: pin.S4Plan, K: int) -> torch.Tensor:
    """Y [K, T, N] on the plan batches' rows: Y[h - 1, t, i] = ret_ld1 of the same id at month
    t + h - 1, looked up by (id, month) over all chars rows, valid or not; 0 where there is no
    such row or it is not finite (the reference's ``ret_impute: zero``).  Y[0] is the batches'
    own ``r`` wherever that is finite."""
    mi = month_index(chars["eom"])
    key = mi * 10_000_000 + chars["id"].to_numpy(np.int64)
    ret = chars["ret_ld1"].to_numpy(np.float64)
    if len(key) > 1 and not (key[1:] >= key[:-1]).all():
        o = np.argsort(key, kind="stable")
        key, ret = key[o], ret[o]
    T, N = len(plan.months), plan.N
    Y = np.zeros((K, T, N))
    hs = np.arange(K, dtype=np.int64)
    for t, ids in enumerate(plan.sig_ids):
        ids = np.asarray(ids, np.int64)
        if not len(ids) or not len(key):
            continue
        q = (int(plan.months[t]) + hs)[:, None] * 10_000_000 + ids[None, :]
        p = np.clip(np.searchsorted(key, q), 0, len(key) - 1)
        v = ret[p]
        Y[:, t, :len(ids)] = np.where((key[p] == q) & np.isfinite(v), v, 0.0)
    return torch.as_tensor(Y, dtype=torch.float64, device=plan.feats.device)


def _shift(x: torch.Tensor, s: int, dim: int) -> torch.Tensor:
    """x moved s positions towards later months along ``dim``, zeros in front."""
    if s == 0:
        return x
    T = x.shape[dim]
    out = torch.zeros_like(x)
    if s < T:
        out.narrow(dim, s, T - s).copy_(x.narrow(dim, 0, T - s))
    return out


def horizon_reals(r_h: torch.Tensor, D: torch.Tensor, h: int, m2: np.ndarray, hp_years):
    """The summands of horizon h's model as the grid search takes them: raw r_h [G, T, P] and
    the shared raw D [G, T, P, P] moved h - 1 months later, zeros in front."""
    return search.complete_local_reals(_shift(r_h, h - 1, 1), _shift(D, h - 1, 1), m2, hp_years)


def horizon_predictions(cfg_m: Config, plan: pin.S4Plan, grids: dict, layout: dict,
                        targets: torch.Tensor, device, clock=None):
    """mu_hat [K, B, N] of the layout's months (NaN: a row without a signal row) and the
    mp_hps.csv frame: one ridge model per horizon, searched and selected one at a time.

    No look-ahead: the pair (Z_s, y^(h)_s) is realised at s + h, so horizon h's summands are the
    raw ones moved h - 1 positions along the consecutive month grid - (r_h[t], D[t]) := (raw
    r_h[t - h + 1], raw D[t - h + 1]), zeros in front - and the window semantics of the grid
    search hold unchanged (horizon 1 is the benchmark stage's model)."""
    tick = clock or (lambda name: None)
    dev = torch.device(device)
    m2 = np.asarray(grids["m2"], np.int64)
    if not np.array_equal(np.asarray(plan.months, np.int64), m2) or \
            (len(m2) > 1 and not (np.diff(m2) == 1).all()):
        raise ValueError("horizon_predictions: the plan's months must be the consecutive PFML "
                         "month grid (the horizon shift moves summands by whole positions)")
    K = int(targets.shape[0])
    r, D, _, ny, z, rh = benchmarks.prediction_reals(plan, cfg_m, grids["oos"], targets=targets)
    del r
    yy = torch.empty((K, len(m2)), dtype=torch.float64, device=targets.device)
    b0 = 0
    for bt in plan.batches:
        sl = slice(b0, b0 + len(bt.months))
        ok = (torch.isfinite(bt.r) & (bt.mask > 0)).to(torch.float64)
        yy[:, sl] = (targets[:, sl] ** 2 * ok[None]).sum(2)
        b0 += len(bt.months)
    tick("summands")
    mu_hat, frames, chosen_all = [], [], []
    for h in range(1, K + 1):
        s = h - 1
        R = horizon_reals(rh[h - 1], D, h, m2, cfg_m.hp_years)
        grid = search.grid_search(R, cfg_m, gather=False)
        frontier._guard_grid(cfg_m, grid, R)
        grid = search.gather_grid(grid)
        meta, coefs, chosen = portfolio.chosen_coefs(cfg_m, grid, layout, dev)
        sig = [z[m[0] if plan.Gc > 1 else 0][m[1]] for m in meta]
        mu_hat.append(portfolio.layout_aims(sig, coefs, [m[2] + 1 for m in meta], layout, dev))
        hp = benchmarks._hps_frame(cfg_m, grid, chosen, _shift(yy[h - 1], s, 0),
                                   _shift(ny, s, 0))
        hp.insert(0, "horizon", h)
        frames.append(hp)
        chosen_all.append(chosen)
        del R, grid
    tick("prediction")
    return torch.stack(mu_hat), pd.concat(frames, ignore_index=True)[MP_HPS_COLUMNS], chosen_all


def multiperiod_portfolios(cfg: Config, chars: pd.DataFrame, barra: BarraCov,
                           wealth: pd.DataFrame, risk_free: pd.DataFrame, device,
                           keep_weights: bool = False, clock=None) -> dict:
    """The Multiperiod-ML table at the configured wealth and gamma -> {"mp": one row per
    portfolio (Portfolio-ML, Multiperiod-ML, the further Multiperiod-ML(u) arms), "pf": their
    monthly series stacked, "hps": the chosen hyper-parameters of every horizon's model,
    "chosen": {hp year: (g, p, l)} of Portfolio-ML}.

    Setup as ``benchmarks.benchmark_portfolios``: ``frontier.point_inputs`` once; the
    ``Portfolio-ML`` row is ``portfolio.backtest_device`` of that point, whose S4 result stays
    alive for its m_tilde and a (``portfolio.layout_m``).  ``horizon_targets`` ->
    ``horizon_predictions`` (a NaN mu_hat enters as 0, counted in ``pfml_mp.missing_mu``) ->
    ``horizon_fold`` once, no arms -> ONE ``mp_chain`` for all arms -> ``pf_stats`` on the
    [(A B), N] view, ``pf_summary`` per arm.

    Failure guard as the benchmarks stage: an arm with a non-finite live w_start is recomputed
    on the CPU; one that stays non-finite becomes a NaN row with its ``reason``, the others
    stand.  ``run.fault_inject = "pfml-mp"`` poisons the last arm.  One process only."""
    from ..parallel.dist import env as dist_env
    if dist_env().world_size > 1:
        raise RuntimeError(WORLD_ERROR)
    tick = clock or (lambda name: None)
    dev = torch.device(device)
    f64 = dict(dtype=torch.float64, device=dev)
    s = cfg.settings
    grids = pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                            s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                            s["pf"]["dates"]["split_years"])
    gamma = float(cfg.pf_set["gamma_rel"])
    cfg_m = mp_config(cfg)
    K = horizons(cfg)
    gbar = float(s.get("mp", {}).get("gbar", 1.0))
    arms = mp_arms(cfg)
    A = len(arms)

    # ---- the Portfolio-ML point ----------------------------------------------------------
    ctx: dict = {}
    pt = frontier.point_inputs(cfg, chars, barra, wealth, risk_free, dev, grids, ctx, clock)
    plan, layout, res = pt["plan"], ctx["layout"], pt["res"]
    months, B, N = layout["months"], layout["B"], layout["N"]
    bt = portfolio.backtest_device(cfg, pt["grid"], res, layout, wealth, dev,
                                   keep_weights=keep_weights)
    mt_all, a_all = portfolio.layout_m(res, layout, dev)         # views of res.m_keep
    del pt
    tick("point")

    # ---- one return model per horizon ----------------------------------------------------
    Y = horizon_targets(chars, plan, K)
    mu_hat, hps, chosen_mp = horizon_predictions(cfg_m, plan, grids, layout, Y, dev, clock)
    del Y
    missing = torch.isnan(mu_hat)
    n_missing = int(missing.sum())
    if n_missing:
        COUNTERS.add("pfml_mp.missing_mu", n_missing)
        log.warning(f"{n_missing} (horizon, row) pair(s) without a signal row: mu_hat taken as 0")
        mu_hat = torch.where(missing, torch.zeros((), **f64), mu_hat)

    # ---- the fold, one chain for all arms, the failure guard -----------------------------
    wvals = torch.as_tensor(portfolio._month_values(wealth, "wealth", months), **f64)
    live, n_rows = layout["live"], layout["n_rows"]
    us = [u for _, u in arms]
    chain_ops = (n_rows, layout["grow"], layout["nmap"], layout["hit"], layout["ws0"])

    def solve(idx: list, on):
        to = lambda x: x.to(on)                                            # noqa: E731
        mt, a = to(mt_all), to(a_all)
        V = horizon_fold(mt, a, to(mu_hat), to(wvals), to(n_rows), gbar)
        Wst, Wopt, _ = mp_chain(mt, a, V, [us[k] for k in idx], *(to(x) for x in chain_ops))
        return V, Wst, Wopt

    V, Wst, Wopt = solve(list(range(A)), dev)
    tick("solve")
    if cfg.run.fault_inject.startswith("pfml-mp") and B:
        Wst[A - 1, B // 2, 0] = NAN
        COUNTERS.add("fault_injected")
    reasons = [""] * A
    bad = torch.nonzero(~portfolio.finite_arms(Wst, live)).flatten()
    if bad.numel():
        names = [arms[k][0] for k in bad.tolist()]
        log.warning(f"non-finite w_start in arm(s) {names}: recomputed on the CPU")
        COUNTERS.add("pfml_mp.recomputed_arms", int(bad.numel()))
        _, Wst_c, Wopt_c = solve(bad.tolist(), torch.device("cpu"))
        Wst[bad], Wopt[bad] = Wst_c.to(dev), Wopt_c.to(dev)
        still = ~portfolio.finite_arms(Wst_c, live.cpu())
        for k in bad[still.to(bad.device)].tolist():
            reasons[k] = "w_start stays non-finite on the CPU weight chain"
            log.warning(f"arm {arms[k][0]}: {reasons[k]}")
    tick("guard")

    # ---- the statistics on the [(A B), N] view, the frames -------------------------------
    stats = pf_stats(Wopt.view(A * B, N), Wst.view(A * B, N), layout["ret"].repeat(A, 1),
                     layout["lam"].repeat(A, 1), n_rows.repeat(A), wvals.repeat(A))
    stats_h = stats.cpu().numpy().reshape(A, B, len(STAT_COLUMNS))
    tick("stats")
    eom = month_end(months)
    eom_ret = eom if cfg.run.compat_mode else eom + pd.offsets.MonthEnd(1)      # quirk Q3
    names = ["Portfolio-ML"] + [n for n, _ in arms]
    uu = [NAN] + us
    reasons = [""] + reasons
    rows, pfs, weights = [], [], {}
    nan_row = {c: NAN for c in frontier.SUMMARY_COLUMNS}
    for j, name in enumerate(names):
        row = {"type": name, "u": uu[j]}
        if reasons[j]:
            row.update({c: v for c, v in nan_row.items() if c != "type"}, n=0)
        else:
            if j == 0:
                pf = bt["pf"].copy()
            else:
                pf = pd.DataFrame(stats_h[j - 1], columns=list(STAT_COLUMNS))
                pf["eom_ret"] = eom_ret
            summ = portfolio.pf_summary(pf, gamma).iloc[0].to_dict()
            row.update({c: v for c, v in summ.items() if c != "type"})
            pfs.append(pf.assign(type=name, u=uu[j])[MP_PF_COLUMNS])
            if keep_weights:
                if j == 0:
                    weights[name] = bt["weights"]
                else:
                    pl = layout["plan"]
                    weights[name] = pd.DataFrame({
                        "eom": month_end(pl["data"]["mi"].to_numpy()), "id": pl["ids"],
                        "w_start": Wst[j - 1][live].cpu().numpy(),
                        "w": Wopt[j - 1][live].cpu().numpy()})
        row["reason"] = reasons[j]
        rows.append({c: (v.item() if isinstance(v, np.generic) else v) for c, v in row.items()})
    out = {"mp": pd.DataFrame(rows, columns=MP_COLUMNS), "hps": hps, "chosen": bt["chosen"],
           "chosen_mp": chosen_mp, "months": months, "missing_mu": n_missing, "K": K,
           "pf": pd.concat(pfs, ignore_index=True) if pfs else pd.DataFrame(columns=MP_PF_COLUMNS)}
    if keep_weights:
        out["weights"] = weights
        out["mu_hat"] = mu_hat.cpu().numpy()
        out["V"] = V.cpu().numpy()
        out["m"] = (mt_all, a_all)
    return out
