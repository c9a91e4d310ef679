"""The portfolios Portfolio-ML is compared against (Jensen, Kelly, Malamud & Pedersen, the
headline table and the frontier figure): Markowitz-ML, Static-ML (with its (k, u, g) arms),
minimum variance and 1/N, next to the Portfolio-ML point itself.  No reference script.

Two observations keep almost everything reuse:

* the return-prediction model is the existing grid search on other summands.  With Z_t the
  month's standardised random-feature block and y_t = ret_ld1, the ridge regression of y on Z
  over an expanding window is ``(mean Z'Z + l I) beta = mean Z'y``, and the validation
  "utility" ``r'beta - beta'D beta / 2`` with ``D = Z'Z``, ``r = Z'y`` equals
  ``-(SSE(beta) - y'y) / 2``: ranking by the expanding-mean score is ranking by validation
  squared error.  A ``PfmlReals`` of (Z'y, Z'Z) goes through ``search.grid_search``,
  ``frontier._guard_grid``, ``portfolio.select_hps`` / ``chosen_coefs`` and ``layout_aims``
  unchanged, quirks included; the aims that come out are mu_hat_t = Z_t beta;
* every benchmark that needs Sigma_t = X F X' + diag(ivol) needs only solves with "factor
  part plus diagonal" (ops/factor_solve.py): Markowitz ``gamma Sigma w = mu_hat``, Static-ML
  ``(gamma (Sigma + g diag(diag Sigma)) + W k Lambda) w = u mu_hat + W k Lambda w_start`` and
  minimum variance ``Sigma w ~ 1``.  Static-ML is sequential in its months through w_start,
  so the hot path is a chain; ONE ``factor_chain`` launch advances all Sigma-based arms.
"""
from __future__ import annotations

import copy
import itertools
import os

import numpy as np
import pandas as pd
import torch

from ..config import Config
from ..ops.factor_solve import factor_chain, factor_prepare
from ..ops.gemm import gemm_fused
from ..ops.panel import rff_features, standardize_signals
from ..ops.pfstats import STAT_COLUMNS, pf_stats
from ..utils.dates import month_end, pfml_date_grids
from ..utils.log import COUNTERS, get_logger
from . import frontier, portfolio, search
from . import pfml_inputs as pin
from .risk import BarraCov

log = get_logger("benchmarks")

BMK_COLUMNS = ["type", "k", "u", "g"] + frontier.SUMMARY_COLUMNS[1:] + ["reason"]
BMK_PF_COLUMNS = ["type", "k", "u", "g", "inv", "shorting", "turnover", "r", "tc", "eom_ret"]
BMK_HPS_COLUMNS = ["hp_year", "g", "p", "l", "lambda", "val_mse"]
NAN = float("nan")
# The factor-structured solve forms u = b / d before it corrects for the factor part, so it
# loses digits when a d_i is far below the factor part of its diagonal, however benign the
# explicit matrix is.  Measured (tests/test_factor_solve_cpu.py): about 4e-3 u ratio^2 of
# max|w| - 4e-11 at a ratio of 1e4, 2e-9 at 1e5.  Beyond 1e4, the largest decade that keeps
# 1e-10, a diagonal variant is "ill split" - a stock whose idiosyncratic variance is next to
# nothing - and its arms take the dense route instead.
SPLIT_RATIO_MAX = 1e4

WORLD_ERROR = ("benchmark_portfolios runs at world size 1: start it in one process (the arms "
               "share one S4 plan and one solve chain)")


def bmk_config(cfg: Config) -> Config:
    """cfg with the prediction model's grid in pf_ml: l_vec <- settings["bmk"]["l_vec"]
    (default settings["rff"]["l_vec"]), p_vec <- settings["bmk"]["p_vec"] (default pf_ml's).
    Every p must be within the S4 plan's p_max: the plan's W is reused."""
    b = cfg.settings.get("bmk", {})
    c = copy.deepcopy(cfg)
    l_vec = b.get("l_vec")
    p_vec = b.get("p_vec")
    c.settings["pf_ml"]["l_vec"] = list(cfg.settings["rff"]["l_vec"] if l_vec is None else l_vec)
    if p_vec is not None:
        c.settings["pf_ml"]["p_vec"] = [int(p) for p in p_vec]
    if max(c.p_vec) > cfg.p_max:
        raise ValueError(f"bmk.p_vec: every p must be <= p_max = {cfg.p_max}")
    return c


def static_arms(cfg: Config) -> list:
    """[(name, k, u, g)] of the Static-ML arms: (1, 1, 0) first as ``Static-ML``, then every
    other combination of settings["bmk"]["static"] as ``Static-ML(k,u,g)``."""
    st = cfg.settings.get("bmk", {}).get("static") or {}
    ks, us, gs = ([float(x) for x in st.get(n, [d])] for n, d in (("k", 1.0), ("u", 1.0),
                                                                  ("g", 0.0)))
    arms = [("Static-ML", 1.0, 1.0, 0.0)]
    for k, u, g in itertools.product(ks, us, gs):
        if (k, u, g) != (1.0, 1.0, 0.0):
            arms.append((f"Static-ML({k:g},{u:g},{g:g})", k, u, g))
    return arms


def prediction_reals(plan: pin.S4Plan, cfg: Config, keep: np.ndarray, targets=None):
    """The summands of the return-prediction model for every month of the plan and every g:
    (r [G, T, P] = Z'y, D [G, T, P, P] = Z'Z, yy [T] = y'y, ny [T] rows with a finite y, z:
    per distinct signal block, per month a [n_t, P] copy of Z_t for the months of ``keep``).

    Z_t: ``rff_features`` + ``standardize_signals`` at lag 0 over the month's signal universe
    with a vol table of ones (no 1 / vol row scale); y = ret_ld1 of the plan's batches.  A row
    with a non-finite y is dropped from both sums.  D by the symmetric-mode GEMM.

    ``targets`` [K, T, N] (``multiperiod.horizon_targets``: further regressands on the batches'
    rows): a sixth result r_h [K, G, T, P] = Z'y_h of every horizon, one [P x N] [N x K] product
    per month and g on the same Z (Z'Z is shared; the rows dropped for y are dropped for every
    y_h)."""
    dev = plan.feats.device
    f64 = dict(dtype=torch.float64, device=dev)
    G, Gc, P, Pp, N, T = plan.G, plan.Gc, plan.P, plan.Pp, plan.N, len(plan.months)
    ones = torch.ones(plan.feats.shape[0] + 1, **f64)
    rffs = [rff_features(plan.feats, plan.Wd[g], cfg.run.precision, width=Pp, pad_rows=1)
            for g in range(Gc)]
    r_out = torch.empty((G, T, P), **f64)
    d_out = torch.empty((G, T, P, P), **f64)
    yy = torch.empty(T, **f64)
    ny = torch.empty(T, **f64)
    z = [[None] * T for _ in range(Gc)]
    rh_out = None
    if targets is not None:
        if targets.dim() != 3 or tuple(targets.shape[1:]) != (T, N):
            raise ValueError(f"prediction_reals: targets must be [K, {T}, {N}]")
        Kh = int(targets.shape[0])
        rh_out = torch.empty((Kh, G, T, P), **f64)
    keep_set = set(int(m) for m in keep)
    b0 = 0
    for bt in plan.batches:
        B = len(bt.months)
        sl = slice(b0, b0 + B)
        ok = torch.isfinite(bt.r) & (bt.mask > 0)
        y = torch.where(ok, bt.r, torch.zeros((), **f64))
        yy[sl] = (y * y).sum(1)
        ny[sl] = ok.sum(1).to(torch.float64)
        idx0 = bt.idx[:, :1].contiguous()
        kept = [bi for bi, d in enumerate(bt.months) if int(d) in keep_set]
        for g in range(Gc):
            Z = torch.empty((B, 1, N, Pp), **f64)
            standardize_signals(rffs[g], idx0, bt.mask, ones, P=P, out=Z, n_real=bt.n_real)
            Zy = Z[:, 0] * ok[..., None].to(torch.float64)
            Dt = torch.empty((B, Pp, Pp), **f64)
            gemm_fused(Zy, Zy, Dt, trans_a=True, sym=True)
            d_out[g, sl] = Dt[:, :P, :P]
            r_out[g, sl] = (Zy * y[..., None]).sum(1)[:, :P]
            if targets is not None:
                Yt = targets[:, sl].to(**f64).permute(1, 2, 0).contiguous()      # [B, N, K]
                Rh = torch.empty((B, Pp, Kh), **f64)
                gemm_fused(Zy, Yt, Rh, trans_a=True)
                rh_out[:, g, sl] = Rh[:, :P].permute(2, 0, 1)
                del Yt, Rh
            for bi in kept:                     # copies: a view would pin the whole block
                z[g][b0 + bi] = Z[bi, 0, : int(bt.ns[bi]), :P].clone()
            del Z, Zy, Dt
        b0 += B
    for g in range(Gc, G):                                  # one signal block (quirk Q1)
        r_out[g], d_out[g] = r_out[0], d_out[0]
        if rh_out is not None:
            rh_out[:, g] = rh_out[:, 0]
    if rh_out is not None:
        return r_out, d_out, yy, ny, z, rh_out
    return r_out, d_out, yy, ny, z


def barra_rows(barra: BarraCov, layout: dict) -> np.ndarray:
    """[B, N] Barra row of every layout id in its month (pad -> the zero row behind the last).
    A layout id without a Barra row in its month is a KeyError, as in create_cov."""
    B, N = layout["B"], layout["N"]
    ridx = np.full((B, N), len(barra.ids), np.int64)
    for t, d in enumerate(layout["months"]):
        bp = barra.month_pos(int(d))
        o0, o1 = int(barra.offsets[bp]), int(barra.offsets[bp + 1])
        bids = np.asarray(barra.ids[o0:o1], np.int64)
        ids = np.asarray(layout["ids"][t], np.int64)
        pos = np.searchsorted(bids, ids)
        if len(ids) and (len(bids) == 0 or np.any(pos >= len(bids))
                         or np.any(bids[np.minimum(pos, len(bids) - 1)] != ids)):
            raise KeyError(f"month {int(d)}: ids missing from the Barra universe")
        ridx[t, :len(ids)] = o0 + pos
    return ridx


def _solve_arms(ops: dict, arms: list, dev):
    """factor_prepare + ONE factor_chain for the arms ``arms`` (indices) on ``dev``:
    (Wst, Wopt, bad [len(arms)] bool: the arm's variant has a flagged system)."""
    to = lambda x: x.to(dev)                                            # noqa: E731
    used = sorted({ops["varm"][a] for a in arms})
    vpos = {v: i for i, v in enumerate(used)}
    vi = torch.as_tensor(used, device=ops["d"].device)
    ai = torch.as_tensor(arms, device=ops["rhs"].device)
    bX, ridx, n_rows = to(ops["bX"]), to(ops["ridx"]), to(ops["n_rows"])
    d = to(ops["d"].index_select(0, vi))
    M, status = factor_prepare(bX, ridx, to(ops["F"]), to(ops["fscale"].index_select(0, vi)), d,
                               n_rows)
    varm = [vpos[ops["varm"][a]] for a in arms]
    Wst, Wopt, _ = factor_chain(bX, ridx, M, d, n_rows, to(ops["rhs"].index_select(0, ai)),
                                to(ops["c"].index_select(0, ai)), varm,
                                [ops["normalize"][a] for a in arms], to(ops["grow"]),
                                to(ops["nmap"]), to(ops["hit"]), to(ops["ws0"]))
    flagged = (status != 0).any(1)
    bad = flagged[torch.as_tensor(varm, device=flagged.device)] if arms else flagged[:0]
    return Wst, Wopt, bad


def _dense_arms(ops: dict, arms: list, dev):
    """The same arms by the dense route: every month's explicit matrix X F_s X' + diag(d) and
    ``torch.linalg.solve``, month by month with the drift -> (Wst, Wopt).  The guard's path for
    ill-split variants, and the other arm of tools/bench_benchmarks.py."""
    to = lambda x: x.to(dev)                                            # noqa: E731
    bX, ridx, F, fscale, d = (to(ops[k]) for k in ("bX", "ridx", "F", "fscale", "d"))
    rhs, c, grow, nmap, hit = (to(ops[k]) for k in ("rhs", "c", "grow", "nmap", "hit"))
    B, N = ridx.shape
    ns = ops["n_rows"].cpu().tolist()
    A = len(arms)
    f64 = dict(dtype=torch.float64, device=bX.device)
    Wst = torch.zeros((A, B, N), **f64)
    Wopt = torch.zeros((A, B, N), **f64)
    ws = to(ops["ws0"]).expand(A, N).clone()
    by_variant: dict = {}
    for j, a in enumerate(arms):
        by_variant.setdefault(ops["varm"][a], []).append(j)
    ai = torch.as_tensor(arms, device=bX.device)
    for t in range(B):
        n = int(ns[t])
        Wst[:, t] = ws
        X = bX[ridx[t, :n]]
        XFX = X @ F[t] @ X.T
        w = torch.zeros((A, N), **f64)
        for v, js in by_variant.items():
            jt = torch.as_tensor(js, device=bX.device)
            S = fscale[v] * XFX + torch.diag(d[v, t, :n])
            b = rhs[ai[jt], t, :n] + c[ai[jt], t, :n] * ws[jt, :n]
            w[jt, :n] = torch.linalg.solve(S, b.T).T
        for j, a in enumerate(arms):
            if ops["normalize"][a]:
                w[j] = w[j] / w[j].sum()
        Wopt[:, t] = w
        ws = (w * grow[t])[:, nmap[t]] * hit[t]
    return Wst, Wopt


def sigma_operands(cfg: Config, plan: pin.S4Plan, barra: BarraCov, layout: dict,
                   mu_hat: torch.Tensor, wealth: pd.DataFrame) -> dict:
    """The operands of the Sigma-based arms in the chain's padded [B, N] layout: arms in the
    order Markowitz-ML, the Static-ML arms (``static_arms``), Minimum variance; arms that share
    a diagonal share a ``factor_prepare`` system.  gamma = pf_set.gamma_rel, W_t the wealth
    path, Lambda the layout's lambda (1e-16 without transaction costs).  diag Sigma = sum_k
    (X F)_ik X_ik + ivol, from bX, bF and biv directly (the square of ``_vol_device``'s vol
    before its NaN fill)."""
    dev = mu_hat.device
    f64 = dict(dtype=torch.float64, device=dev)
    B, N = layout["B"], layout["N"]
    gamma, statics = float(cfg.pf_set["gamma_rel"]), static_arms(cfg)
    wvals = torch.as_tensor(portfolio._month_values(wealth, "wealth", layout["months"]), **f64)
    lam = layout["lam"] if bool(cfg.settings["Transaction_Costs"]) else \
        torch.where(layout["live"], torch.full((), 1e-16, **f64), torch.zeros((), **f64))
    Kp = plan.bF.shape[-1]
    bX = plan.bX[:, :Kp]
    ridx = torch.as_tensor(barra_rows(barra, layout), device=dev)
    fpos = torch.as_tensor(np.asarray([barra.month_pos(int(d)) for d in layout["months"]],
                                      np.int64), device=dev)
    F = plan.bF.index_select(0, fpos) if B else plan.bF[:0]
    live = layout["live"]
    one, zero = torch.ones((), **f64), torch.zeros((), **f64)
    iv = torch.where(live, plan.biv[ridx], one)
    Xg = bX[ridx]                                                       # [B, N, Kp]
    dsig = torch.where(live, (torch.matmul(Xg, F) * Xg).sum(-1) + iv, one)
    wl = torch.where(live, wvals[:, None] * lam, zero)                  # W_t Lambda_t
    names, kug, varm, normalize, rhs, c = [], [], [], [], [], []
    variants: dict = {}

    fdiag = (dsig - iv).abs()                                           # diag(X F X')

    def variant(key, fscale, diag):
        if key not in variants:
            ratio = torch.where(live, fscale * fdiag / diag, zero).max() if B else zero
            variants[key] = (len(variants), fscale, torch.where(live, diag, one), ratio)
        return variants[key][0]

    names.append("Markowitz-ML")
    kug.append((NAN, NAN, NAN))
    varm.append(variant(("mkw",), gamma, gamma * iv))
    normalize.append(False)
    rhs.append(mu_hat)
    c.append(torch.zeros((B, N), **f64))
    for name, k, u, g in statics:
        names.append(name)
        kug.append((k, u, g))
        varm.append(variant(("static", k, g), gamma, gamma * (iv + g * dsig) + k * wl))
        normalize.append(False)
        rhs.append(u * mu_hat)
        c.append(k * wl)
    names.append("Minimum variance")
    kug.append((NAN, NAN, NAN))
    varm.append(variant(("minvar",), 1.0, iv))
    normalize.append(True)
    rhs.append(torch.where(live, one, zero))
    c.append(torch.zeros((B, N), **f64))
    vs = sorted(variants.values(), key=lambda x: x[0])
    return dict(bX=bX, ridx=ridx, F=F, n_rows=layout["n_rows"], wvals=wvals,
                fscale=torch.as_tensor([v[1] for v in vs], **f64),
                split_ratio=torch.stack([v[3] for v in vs]),
                d=torch.stack([v[2] for v in vs]), rhs=torch.stack(rhs), c=torch.stack(c),
                varm=varm, normalize=normalize, grow=layout["grow"], nmap=layout["nmap"],
                hit=layout["hit"], ws0=layout["ws0"], names=names, kug=kug, diag_sigma=dsig)


def equal_weights(layout: dict):
    """1/N: w_t = 1 / n_t on the month's rows, w_start by the drift of ``portfolio._chain``."""
    live, B = layout["live"], layout["B"]
    n = layout["n_rows"].to(torch.float64).clamp(min=1.0)
    W = live.to(torch.float64) / n[:, None]
    Wst = torch.zeros_like(W)
    if B:
        Wst[0] = layout["ws0"]
    if B > 1:
        Wst[1:] = (W * layout["grow"])[:-1].gather(1, layout["nmap"][:-1]) * layout["hit"][:-1]
    return Wst, W


def _hps_frame(cfg_b: Config, grid, chosen: dict, yy, ny) -> pd.DataFrame:
    """bmk_hps.csv: the chosen (g, p, l) of every hp year the OOS months draw on, and the
    model's validation MSE: sum (yy_t - 2 obj_t) / sum n_t over the validation months up to the
    year's December (the expanding set the score ranks on)."""
    mpos = {int(m): i for i, m in enumerate(np.asarray(grid.all_months))}
    vm = np.asarray([mpos[int(m)] for m in grid.val_months], np.int64)
    yy_v, ny_v = yy.cpu().numpy()[vm], ny.cpu().numpy()[vm]
    rows = []
    for year, (g, p, l) in sorted(chosen.items()):
        sel = np.nonzero(np.asarray(grid.val_year) <= year)[0]
        obj = grid.obj[torch.as_tensor(sel, device=grid.obj.device), g,
                       cfg_b.p_vec.index(p), l].cpu().numpy()
        sse = float(np.sum(yy_v[sel] - 2.0 * obj))
        cnt = float(np.sum(ny_v[sel]))
        rows.append({"hp_year": int(year), "g": int(g), "p": int(p), "l": int(l),
                     "lambda": float(cfg_b.l_vec[l]), "val_mse": sse / cnt if cnt else NAN})
    return pd.DataFrame(rows, columns=BMK_HPS_COLUMNS)


def benchmark_portfolios(cfg: Config, chars: pd.DataFrame, barra: BarraCov, wealth: pd.DataFrame,
                         risk_free: pd.DataFrame, device, keep_weights: bool = False,
                         clock=None) -> dict:
    """The benchmark table at the configured wealth and gamma -> {"bmk": one row per portfolio
    (Portfolio-ML, Markowitz-ML, Static-ML, the further Static-ML(k,u,g) arms, Minimum
    variance, 1/N), "pf": their monthly series stacked, "hps": the prediction model's chosen
    hyper-parameters, "chosen": {hp year: (g, p, l)} of Portfolio-ML}.

    Setup as ``importance.feature_importance``: ``frontier.point_inputs`` once; its S4 plan,
    its ``backtest_layout`` and the Portfolio-ML point are reused, and the ``Portfolio-ML`` row
    is ``portfolio.backtest_device`` of that point.  The prediction model: ``prediction_reals``
    under ``bmk_config`` through the guarded grid search and the selection; mu_hat by
    ``layout_aims`` - a row without a signal row (NaN) enters the solves as 0 and is counted
    (``pfml_bmk.missing_mu``).  The Sigma-based arms: ``sigma_operands``, ``factor_prepare`` per
    distinct diagonal, ONE ``factor_chain``; 1/N in torch.  ``pf_stats`` on the [(A B), N]
    view, ``pf_summary`` per arm.  The backtest covers the OOS months; choosing among the
    Static-ML arms on validation years is not done - all arms are reported.

    A diagonal variant whose smallest entry is next to nothing against the factor part (a
    stock with almost no idiosyncratic variance; ``SPLIT_RATIO_MAX``) would lose its digits in
    u = b / d: its arms are solved densely instead (``_dense_arms``, counted in
    ``pfml_bmk.dense_arms``).  Failure guard as the importance stage: an arm with a non-finite
    live w_start (or a flagged ``factor_prepare`` system) is recomputed on the CPU; one that
    stays non-finite becomes a NaN row with its ``reason``, the others stand.  One process
    only."""
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
    cfg_b = bmk_config(cfg)

    # ---- the Portfolio-ML point ----------------------------------------------------------
    ctx: dict = {}
    pt = frontier.point_inputs(cfg, chars, barra, wealth, risk_free, dev, grids, ctx, clock)
    plan, layout = pt["plan"], ctx["layout"]
    months, B, N = layout["months"], layout["B"], layout["N"]
    bt = portfolio.backtest_device(cfg, pt["grid"], pt["res"], layout, wealth, dev,
                                   keep_weights=keep_weights)
    del pt
    tick("point")

    # ---- the return-prediction model -----------------------------------------------------
    r, D, yy, ny, z = prediction_reals(plan, cfg_b, grids["oos"])
    tick("summands")
    R = search.complete_local_reals(r, D, grids["m2"], cfg_b.hp_years)
    grid = search.grid_search(R, cfg_b, gather=False)
    frontier._guard_grid(cfg_b, grid, R)
    grid = search.gather_grid(grid)
    meta, coefs, chosen_b = portfolio.chosen_coefs(cfg_b, grid, layout, dev)
    sig = [z[m[0] if plan.Gc > 1 else 0][m[1]] for m in meta]
    mu_hat = portfolio.layout_aims(sig, coefs, [m[2] + 1 for m in meta], layout, dev)
    hps = _hps_frame(cfg_b, grid, chosen_b, yy, ny)
    del r, D, R, grid, z, sig
    missing = torch.isnan(mu_hat)
    n_missing = int(missing.sum())
    if n_missing:
        COUNTERS.add("pfml_bmk.missing_mu", n_missing)
        log.warning(f"{n_missing} row(s) without a signal row: mu_hat taken as 0")
        mu_hat = torch.where(missing, torch.zeros((), **f64), mu_hat)
    tick("prediction")

    # ---- the Sigma-based arms: prepare, one chain, the failure guard ---------------------
    ops = sigma_operands(cfg, plan, barra, layout, mu_hat, wealth)
    wvals = ops["wvals"]
    A = len(ops["names"])
    live = layout["live"]
    ratio = ops["split_ratio"].cpu().numpy()
    ill = {a for a in range(A) if not ratio[ops["varm"][a]] <= SPLIT_RATIO_MAX}
    if ill:
        log.warning(f"diagonal of arm(s) {[ops['names'][a] for a in sorted(ill)]} is next to "
                    f"nothing against the factor part (ratio up to {np.nanmax(ratio):.3g}): "
                    "dense solves")
        COUNTERS.add("pfml_bmk.dense_arms", len(ill))

    def solve(arms: list, on):
        """(Wst, Wopt, flagged) of ``arms``: the factor-structured chain, dense for ``ill``."""
        Ws = torch.zeros((len(arms), B, N), dtype=torch.float64, device=on)
        Wo = torch.zeros_like(Ws)
        fl = torch.zeros(len(arms), dtype=torch.bool, device=on)
        pos_f = [j for j, a in enumerate(arms) if a not in ill]
        pos_i = [j for j, a in enumerate(arms) if a in ill]
        if pos_f:
            jf = torch.as_tensor(pos_f, device=on)
            Ws[jf], Wo[jf], fl[jf] = _solve_arms(ops, [arms[j] for j in pos_f], on)
        if pos_i:
            ji = torch.as_tensor(pos_i, device=on)
            Ws[ji], Wo[ji] = _dense_arms(ops, [arms[j] for j in pos_i], on)
        return Ws, Wo, fl

    Wst, Wopt, flagged = solve(list(range(A)), dev)
    tick("solve")
    if cfg.run.fault_inject.startswith("pfml-bmk") and B:
        Wst[A - 1, B // 2, 0] = NAN
        COUNTERS.add("fault_injected")
    reasons = [""] * A
    bad = torch.nonzero(~portfolio.finite_arms(Wst, live) | flagged).flatten()
    if bad.numel():
        names = [ops["names"][k] for k in bad.tolist()]
        log.warning(f"non-finite w_start in arm(s) {names}: recomputed on the CPU")
        COUNTERS.add("pfml_bmk.recomputed_arms", int(bad.numel()))
        Wst_c, Wopt_c, flag_c = solve(bad.tolist(), torch.device("cpu"))
        Wst[bad], Wopt[bad] = Wst_c.to(dev), Wopt_c.to(dev)
        still = ~portfolio.finite_arms(Wst_c, live.cpu()) | flag_c
        for k in bad[still.to(bad.device)].tolist():
            reasons[k] = "w_start stays non-finite on the CPU solve chain"
            log.warning(f"arm {ops['names'][k]}: {reasons[k]}")
    tick("guard")

    # ---- 1/N, the statistics on the [(A B), N] view, the frames --------------------------
    Wst_n, Wopt_n = equal_weights(layout)
    Wst = torch.cat([Wst, Wst_n[None]])
    Wopt = torch.cat([Wopt, Wopt_n[None]])
    names = ["Portfolio-ML"] + ops["names"] + ["1/N"]
    kug = [(NAN, NAN, NAN)] + ops["kug"] + [(NAN, NAN, NAN)]
    reasons = [""] + reasons + [""]
    A1 = A + 1
    stats = pf_stats(Wopt.view(A1 * B, N), Wst.view(A1 * B, N), layout["ret"].repeat(A1, 1),
                     layout["lam"].repeat(A1, 1), layout["n_rows"].repeat(A1), wvals.repeat(A1))
    stats_h = stats.cpu().numpy().reshape(A1, B, len(STAT_COLUMNS))
    tick("stats")
    eom = month_end(months)
    eom_ret = eom if cfg.run.compat_mode else eom + pd.offsets.MonthEnd(1)      # quirk Q3
    rows, pfs, weights = [], [], {}
    nan_row = {c: NAN for c in frontier.SUMMARY_COLUMNS}
    for j, name in enumerate(names):
        row = {"type": name, "k": kug[j][0], "u": kug[j][1], "g": kug[j][2]}
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
            pfs.append(pf.assign(type=name, k=kug[j][0], u=kug[j][1], g=kug[j][2])[BMK_PF_COLUMNS])
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
    out = {"bmk": pd.DataFrame(rows, columns=BMK_COLUMNS), "hps": hps, "chosen": bt["chosen"],
           "chosen_bmk": chosen_b, "months": months, "missing_mu": n_missing,
           "pf": pd.concat(pfs, ignore_index=True) if pfs else pd.DataFrame(columns=BMK_PF_COLUMNS)}
    if keep_weights:
        out["weights"] = weights
        out["mu_hat"] = mu_hat.cpu().numpy()
    return out


def plot_benchmarks(bmk: pd.DataFrame, out_dir: str) -> list[str]:
    """plots/benchmarks.png: annualised sd against return net of TC, one marker per arm.
    Skipped without matplotlib."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        log.info("matplotlib not available: plot skipped")
        return []
    os.makedirs(out_dir, exist_ok=True)
    fig, ax = plt.subplots(figsize=(6, 4))
    for _, row in bmk[bmk["reason"] == ""].iterrows():
        ax.plot([row["sd"]], [row["r_tc"]], "o", label=str(row["type"]))
    ax.set_xlabel("volatility (annualised)")
    ax.set_ylabel("return net of TC (annualised)")
    ax.legend(fontsize=6)
    f = os.path.join(out_dir, "benchmarks.png")
    fig.tight_layout()
    fig.savefig(f, dpi=100)
    plt.close(fig)
    return [f]
