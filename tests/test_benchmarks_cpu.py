"""The benchmark portfolios on the CPU path (models/benchmarks.py): the prediction model's
summands against a pandas / numpy standardisation of the same panel, "selection = lowest
validation squared error" from the returned coefficients, mu_hat, every arm against an
independent oracle (``create_cov`` Sigma, ``np.linalg.solve``, a plain Python loop over the
months with the drift, ``pf_ts`` / ``pf_summary`` on frames) in compat and corrected mode, the
Portfolio-ML row, the frames, the stage registration and the failure isolation.

Inputs: the session's ``small_data`` panel with four OOS years and p_vec = [16, 32] (the
settings test_gpu_importance.py runs a point on), in a copy of its directory that also holds
an rff_w.csv for compat mode."""
import copy
import os
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

from pfml.config import Config, get_features
from pfml.data.io import CSV_COLUMNS
from pfml.models import benchmarks, frontier, portfolio, search
from pfml.models import pfml_inputs as pin
from pfml.models.risk import create_cov
from pfml.utils.dates import month_end, month_index, pfml_date_grids

STAT = ["inv", "shorting", "turnover", "r", "tc"]
NUM = [c for c in frontier.SUMMARY_COLUMNS if c != "type"]
TOL = dict(rtol=1e-10, atol=1e-12)          # the tolerance of the importance oracle
STATIC = ["bmk.static.k=[1,0.5]", "bmk.static.u=[1,0]", "bmk.static.g=[0,2]"]


def _grids(cfg, barra):
    s = cfg.settings
    return pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                           s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                           s["pf"]["dates"]["split_years"])


YEARS = ["pf.dates.start_year=2008", "pf.dates.end_yr=2012", "pf.dates.split_years=1",
         "pf_ml.p_vec=[16,32]"]


@pytest.fixture(scope="module")
def data(small_data, tmp_path_factory):
    from pfml.data import io
    from pfml.models.risk import BarraCov
    d = str(tmp_path_factory.mktemp("bmk_cpu") / "data")
    shutil.copytree(small_data.run.data_dir, d)
    cfg = small_data.override(YEARS + STATIC + [f"run.data_dir={d}"])
    rng = np.random.default_rng(5)
    pd.DataFrame(rng.standard_normal((len(get_features()), cfg.p_max // 2))).to_csv(
        f"{d}/rff_w.csv")
    return (cfg, io.read_processed_chars(d, get_features()),
            BarraCov.load(os.path.join(d, "Barra_Cov.npz")),
            pd.read_csv(os.path.join(d, "wealth_processed.csv"), parse_dates=["eom"]),
            io.read_risk_free(d))


def _cfg(data, compat):
    cfg = copy.deepcopy(data[0])
    cfg.run.compat_mode = compat
    return cfg


def _run(data, compat, cfg=None, **kw):
    _, chars, barra, wealth, rf = data
    return benchmarks.benchmark_portfolios(cfg or _cfg(data, compat), chars, barra, wealth, rf,
                                           "cpu", **kw)


@pytest.fixture(scope="module")
def runs(data):
    return {compat: _run(data, compat, keep_weights=True) for compat in (False, True)}


# ---------------------------------------------------------------------------------------------
# the prediction model
# ---------------------------------------------------------------------------------------------
def _z_oracle(chars, ids, month, W):
    """pandas / numpy: the standardised random-feature block of the month's universe (id
    order, internal column order [1, cos z1, sin z1, ...]) and its ret_ld1."""
    mi = month_index(chars["eom"])
    sub = chars[mi == int(month)].set_index("id").loc[list(ids)]
    zz = sub[get_features()].to_numpy(np.float64) @ W
    S = pd.DataFrame(np.ones((len(ids), 1 + 2 * W.shape[1])))
    S.iloc[:, 1::2] = np.cos(zz)
    S.iloc[:, 2::2] = np.sin(zz)
    dm = S - S.mean()
    dm[0] = S[0]                                        # the constant is not demeaned
    Z = dm / np.sqrt((dm ** 2).sum())
    return Z.to_numpy(np.float64), sub["ret_ld1"].to_numpy(np.float64)


@pytest.fixture(scope="module")
def model(data):
    """Per mode: the S4 plan, the summands and the grid of the prediction model (the stage's
    own calls, made here once), for the checks below."""
    out = {}
    _, chars, barra, wealth, rf = data
    for compat in (False, True):
        cfg = _cfg(data, compat)
        g = _grids(cfg, barra)
        plan = pin.make_s4_plan(cfg, chars, barra, wealth, rf, "cpu", g["m2"])
        cfg_b = benchmarks.bmk_config(cfg)
        r, D, yy, ny, z = benchmarks.prediction_reals(plan, cfg_b, g["oos"])
        R = search.complete_local_reals(r, D, g["m2"], cfg_b.hp_years)
        grid = search.grid_search(R, cfg_b)
        out[compat] = dict(cfg=cfg, cfg_b=cfg_b, plan=plan, r=r, D=D, yy=yy, ny=ny, z=z,
                           grid=grid, m2=g["m2"], oos=g["oos"])
    return out


@pytest.mark.parametrize("compat", [False, True])
def test_summands_against_pandas_standardisation(data, model, compat):
    m, chars = model[compat], data[1]
    plan = m["plan"]
    assert plan.Gc in (1, plan.G)
    T = len(m["m2"])
    for t in (0, T // 3, T - 1):
        for g in range(plan.G):
            gc = g if plan.Gc > 1 else 0
            Z, y = _z_oracle(chars, plan.sig_ids[t], m["m2"][t], plan.W[gc])
            ok = np.isfinite(y)
            Zk, yk = Z[ok], y[ok]
            assert np.allclose(m["D"][g, t].numpy(), Zk.T @ Zk, **TOL)
            assert np.allclose(m["r"][g, t].numpy(), Zk.T @ yk, **TOL)
        assert np.isclose(float(m["yy"][t]), float(yk @ yk), **TOL)
        assert float(m["ny"][t]) == ok.sum()


def test_nonfinite_return_is_dropped_from_both_sums(data, model):
    m = model[False]
    plan = copy.copy(m["plan"])
    bt = copy.copy(plan.batches[0])
    bt.r = bt.r.clone()
    bt.r[0, 1] = float("nan")
    plan.batches = [bt] + list(plan.batches[1:])
    r, D, yy, ny, _ = benchmarks.prediction_reals(plan, m["cfg_b"], m["oos"])
    Z, y = _z_oracle(data[1], plan.sig_ids[0], m["m2"][0], plan.W[0])
    keep = np.arange(len(y)) != 1
    assert np.allclose(D[0, 0].numpy(), Z[keep].T @ Z[keep], **TOL)
    assert np.allclose(r[0, 0].numpy(), Z[keep].T @ y[keep], **TOL)
    assert float(ny[0]) == keep.sum() and np.isclose(float(yy[0]), y[keep] @ y[keep], **TOL)


@pytest.mark.parametrize("compat", [False, True])
def test_utility_is_minus_half_sse_minus_yy(data, model, compat):
    """obj == -(SSE - yy) / 2 recomputed from the returned beta on sampled cells: ranking by
    the score is ranking by validation squared error."""
    m, chars = model[compat], data[1]
    grid, plan, cfg_b = m["grid"], m["plan"], m["cfg_b"]
    mpos = {int(d): i for i, d in enumerate(m["m2"])}
    years = list(np.asarray(grid.years_local))
    L = len(cfg_b.l_vec)
    nV = len(grid.val_months)
    checked = 0
    for v in (0, nV // 2, nV - 1):
        t = mpos[int(grid.val_months[v])]
        yi = years.index(int(grid.val_year[v]))
        for g in range(plan.G):
            Z, y = _z_oracle(chars, plan.sig_ids[t], m["m2"][t], plan.W[g if plan.Gc > 1 else 0])
            for pi, p in enumerate(cfg_b.p_vec):
                for l in (0, L // 2, L - 1):
                    beta = grid.beta[g, yi, pi, l, : p + 1].numpy()
                    if not np.isfinite(beta).all():
                        continue
                    e = y - Z[:, : p + 1] @ beta
                    want = -0.5 * (e @ e - y @ y)
                    got = float(grid.obj[v, g, pi, l])
                    assert abs(got - want) <= 1e-10 * float(y @ y), (v, g, p, l)
                    checked += 1
    assert checked >= 3 * plan.G * len(cfg_b.p_vec) * 2          # at most the l = 0 cells skipped


@pytest.mark.parametrize("compat", [False, True])
def test_mu_hat(data, model, runs, compat):
    m, out, chars = model[compat], runs[compat], data[1]
    grid, plan, cfg_b = m["grid"], m["plan"], m["cfg_b"]
    assert out["missing_mu"] == 0
    mpos = {int(d): i for i, d in enumerate(m["m2"])}
    years = list(np.asarray(grid.years_local))
    for tb, d in enumerate(out["months"]):
        oos_year = int(month_end(int(d) + 1).year[0])
        g, p, l = out["chosen_bmk"][oos_year - 1]
        t = mpos[int(d)]
        Z, _ = _z_oracle(chars, plan.sig_ids[t], d, plan.W[g if plan.Gc > 1 else 0])
        beta = grid.beta[g, years.index(oos_year), cfg_b.p_vec.index(p), l, : p + 1].numpy()
        n = len(plan.sig_ids[t])
        assert np.allclose(out["mu_hat"][tb, :n], Z[:, : p + 1] @ beta, **TOL)
        assert not out["mu_hat"][tb, n:].any()
    hps = out["hps"]
    assert list(hps.columns) == CSV_COLUMNS["bmk_hps.csv"]
    assert list(hps["hp_year"]) == sorted(out["chosen_bmk"])
    assert (hps["val_mse"] > 0).all()


@pytest.mark.parametrize("compat", [False, True])
def test_validation_mse_from_pandas(data, model, runs, compat):
    """val_mse of every chosen hp year recomputed from the pandas Z, y and the returned beta:
    the squared errors of the year's chosen (g, p, l), each validation month under the beta of
    its own hp year, pooled over the validation months of the hp years up to that year."""
    m, hps, chars = model[compat], runs[compat]["hps"], data[1]
    grid, plan, cfg_b = m["grid"], m["plan"], m["cfg_b"]
    mpos = {int(d): i for i, d in enumerate(m["m2"])}
    years = list(np.asarray(grid.years_local))
    first = int(np.min(grid.val_year))
    for _, row in hps.iterrows():
        year, g, p, l = int(row["hp_year"]), int(row["g"]), int(row["p"]), int(row["l"])
        assert float(row["lambda"]) == float(cfg_b.l_vec[l])
        sse, cnt, months = 0.0, 0, 0
        for v in range(len(grid.val_months)):
            if int(grid.val_year[v]) > year:
                continue
            t = mpos[int(grid.val_months[v])]
            Z, y = _z_oracle(chars, plan.sig_ids[t], m["m2"][t], plan.W[g if plan.Gc > 1 else 0])
            beta = grid.beta[g, years.index(int(grid.val_year[v])), cfg_b.p_vec.index(p), l,
                             : p + 1].numpy()
            ok = np.isfinite(y)
            e = y[ok] - Z[ok][:, : p + 1] @ beta
            sse, cnt, months = sse + float(e @ e), cnt + int(ok.sum()), months + 1
        assert months == 12 * (year - first + 1)
        assert np.isclose(float(row["val_mse"]), sse / cnt, **TOL), year


# ---------------------------------------------------------------------------------------------
# the arms
# ---------------------------------------------------------------------------------------------
def _arm_oracle(data, cfg, out, kind, k=1.0, u=1.0, g=0.0):
    """A plain loop over the OOS months: Sigma by ``create_cov``, ``np.linalg.solve``, the
    drift through the ids -> the weights frame (id, eom, w_start, w)."""
    _, chars, barra, wealth, _ = data
    gamma = float(cfg.pf_set["gamma_rel"])
    mi = month_index(chars["eom"])
    wmi = month_index(wealth["eom"])
    ws = None
    frames = []
    for tb, d in enumerate(out["months"]):
        sub = chars[(mi == int(d)) & chars["valid"].to_numpy()].sort_values("id")
        ids = sub["id"].to_numpy(np.int64)
        n = len(ids)
        wrow = wealth[wmi == int(d)].iloc[0]
        _, Sigma = create_cov(barra, int(d), ids)
        mu = out["mu_hat"][tb, :n]
        if ws is None:
            me = sub["me"].to_numpy(np.float64)
            start = me / me.sum()
        else:
            start = np.asarray([ws.get(int(i), 0.0) for i in ids])
        if kind == "markowitz":
            w = np.linalg.solve(gamma * Sigma, mu)
        elif kind == "static":
            WL = float(wrow["wealth"]) * k * np.diag(sub["lambda"].to_numpy(np.float64))
            S = Sigma + g * np.diag(np.diag(Sigma))
            w = np.linalg.solve(gamma * S + WL, u * mu + WL @ start)
        elif kind == "minvar":
            x = np.linalg.solve(Sigma, np.ones(n))
            w = x / x.sum()
        else:
            w = np.full(n, 1.0 / n)
        frames.append(pd.DataFrame({"id": ids, "eom": month_end(int(d))[0], "w_start": start,
                                    "w": w}))
        grown = w * (1.0 + sub["tr_ld1"].to_numpy(np.float64)) / (1.0 + float(wrow["mu_ld1"]))
        ws = dict(zip(ids.tolist(), grown.tolist()))
    return pd.concat(frames, ignore_index=True)


ARMS = [("Markowitz-ML", "markowitz", {}), ("Static-ML", "static", {}),
        ("Static-ML(1,1,2)", "static", dict(g=2.0)), ("Static-ML(0.5,1,0)", "static", dict(k=0.5)),
        ("Static-ML(0.5,0,2)", "static", dict(k=0.5, u=0.0, g=2.0)),
        ("Static-ML(1,0,0)", "static", dict(u=0.0)), ("Minimum variance", "minvar", {}),
        ("1/N", "equal", {})]


@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("name,kind,kw", ARMS)
def test_arm_against_the_independent_oracle(data, runs, compat, name, kind, kw):
    _, chars, _, wealth, _ = data
    cfg, out = _cfg(data, compat), runs[compat]
    ow = _arm_oracle(data, cfg, out, kind, **kw)
    got = out["weights"][name]
    assert np.array_equal(got["id"].to_numpy(), ow["id"].to_numpy())
    assert np.allclose(got["w"].to_numpy(), ow["w"].to_numpy(), **TOL)
    assert np.allclose(got["w_start"].to_numpy(), ow["w_start"].to_numpy(), **TOL)
    pf = portfolio.pf_ts(ow, chars, wealth, compat=compat)
    mine = out["pf"][out["pf"]["type"] == name]
    assert len(mine) == len(pf) == len(out["months"])
    assert list(pd.to_datetime(mine["eom_ret"])) == list(pd.to_datetime(pf["eom_ret"]))
    for c in STAT:
        assert np.allclose(mine[c].to_numpy(), pf[c].to_numpy(), **TOL), c
    summ = portfolio.pf_summary(pf, float(cfg.pf_set["gamma_rel"])).iloc[0]
    row = out["bmk"][out["bmk"]["type"] == name].iloc[0]
    assert np.allclose(row[NUM].to_numpy(float), summ[NUM].to_numpy(float), **TOL)
    if kind == "static":
        assert (row["k"], row["u"], row["g"]) == (kw.get("k", 1.0), kw.get("u", 1.0),
                                                  kw.get("g", 0.0))


def test_zero_u_only_decays_the_start_weights(data, runs):
    """u = 0, k > 0: w = (gamma Sigma + W k Lambda)^-1 W k Lambda w_start.  No signal enters
    (the oracle above matches with u mu_hat = 0), and with C = W k Lambda the map is a
    contraction in the C norm: C^1/2 w = (I + C^-1/2 gamma Sigma C^-1/2)^-1 C^1/2 w_start, so
    sum lambda w^2 < sum lambda w_start^2 in every month."""
    w = runs[False]["weights"]["Static-ML(1,0,0)"].merge(
        data[1][["id", "eom", "lambda"]], on=["id", "eom"], how="left")
    assert w["lambda"].notna().all() and np.isclose(w.groupby("eom")["w_start"].sum().iloc[0], 1.0)
    e = w.assign(a=w["lambda"] * w["w"] ** 2, b=w["lambda"] * w["w_start"] ** 2).groupby("eom")
    assert (e["a"].sum() < e["b"].sum()).all()


@pytest.mark.parametrize("compat", [False, True])
def test_portfolio_ml_row_is_backtest_device(data, runs, compat):
    _, chars, barra, wealth, rf = data
    cfg = _cfg(data, compat)
    bt = frontier.run_point(cfg, chars, barra, wealth, rf, "cpu", _grids(cfg, barra), {})
    out = runs[compat]
    mine = out["pf"][out["pf"]["type"] == "Portfolio-ML"]
    assert np.array_equal(mine[STAT].to_numpy(), bt["pf"][STAT].to_numpy())
    summ = portfolio.pf_summary(bt["pf"], float(cfg.pf_set["gamma_rel"])).iloc[0]
    assert np.array_equal(out["bmk"].loc[0, NUM].to_numpy(float), summ[NUM].to_numpy(float))
    assert out["chosen"] == bt["chosen"]


def test_ill_split_diagonals_take_the_dense_route(data, monkeypatch):
    """The small panel holds a stock whose idiosyncratic variance is ~1e-32: against the factor
    part that diagonal loses every digit of u = b / d, so the arms on gamma ivol and ivol alone
    (Markowitz-ML, Minimum variance) are solved densely; the Static-ML diagonals carry W Lambda
    and stay on the factor-structured chain.  Both routes are checked against the oracle above."""
    assert data[2].ivol.min() < 1e-20
    dense, chain = [], []
    real_d, real_s = benchmarks._dense_arms, benchmarks._solve_arms
    monkeypatch.setattr(benchmarks, "_dense_arms",
                        lambda ops, arms, dev: (dense.append([ops["names"][a] for a in arms]),
                                                real_d(ops, arms, dev))[1])
    monkeypatch.setattr(benchmarks, "_solve_arms",
                        lambda ops, arms, dev: (chain.append([ops["names"][a] for a in arms]),
                                                real_s(ops, arms, dev))[1])
    out = _run(data, False)
    assert dense == [["Markowitz-ML", "Minimum variance"]]
    assert len(chain) == 1 and len(chain[0]) == 8 and all(n.startswith("Static-ML")
                                                          for n in chain[0])
    assert (out["bmk"]["reason"] == "").all()


@pytest.fixture(scope="module")
def regular(tmp_path_factory):
    """The 40-stock engine panel of test_importance_cpu.py (three OOS years, p_vec = [8, 16]):
    no degenerate idiosyncratic variance, so every Sigma-based arm stays on the
    factor-structured chain.  (inputs, the corrected-mode run, the arms that went dense)."""
    from pfml.data.synthetic import engine_inputs
    d = str(tmp_path_factory.mktemp("bmk_regular"))
    cfg = Config.default().override(["pf_ml.p_vec=[8,16]", "pf.dates.start_year=2001",
                                     "pf.dates.end_yr=2004", "pf.dates.split_years=1",
                                     "split.test_end=2004-12-31", f"run.data_dir={d}"] + STATIC)
    cfg.run.compat_mode = False
    inputs = (cfg,) + engine_inputs(n_stocks=40, start="1993-01-31", end="2004-12-31")
    dense, real = [], benchmarks._dense_arms
    benchmarks._dense_arms = lambda ops, arms, dev: (dense.append(arms), real(ops, arms, dev))[1]
    try:
        out = _run(inputs, False, keep_weights=True)
    finally:
        benchmarks._dense_arms = real
    return inputs, out, dense


@pytest.mark.parametrize("name,kind,kw", ARMS)
def test_regular_panel_keeps_every_arm_on_the_chain(regular, name, kind, kw):
    """Markowitz-ML and the normalised Minimum variance included: nothing goes dense, and every
    arm meets the same oracle at the same tolerance."""
    inputs, out, dense = regular
    assert dense == [] and (out["bmk"]["reason"] == "").all()
    ow = _arm_oracle(inputs, inputs[0], out, kind, **kw)
    got = out["weights"][name]
    assert np.array_equal(got["id"].to_numpy(), ow["id"].to_numpy())
    assert np.allclose(got["w"].to_numpy(), ow["w"].to_numpy(), **TOL)
    assert np.allclose(got["w_start"].to_numpy(), ow["w_start"].to_numpy(), **TOL)
    pf = portfolio.pf_ts(ow, inputs[1], inputs[3], compat=False)
    mine = out["pf"][out["pf"]["type"] == name]
    for c in STAT:
        assert np.allclose(mine[c].to_numpy(), pf[c].to_numpy(), **TOL), c


def test_frames_columns_and_order(runs):
    for out in runs.values():
        bmk, pf = out["bmk"], out["pf"]
        assert list(bmk.columns) == CSV_COLUMNS["bmk.csv"] == benchmarks.BMK_COLUMNS
        assert list(pf.columns) == CSV_COLUMNS["bmk_pf.csv"] == benchmarks.BMK_PF_COLUMNS
        names = list(bmk["type"])
        assert names[:3] == ["Portfolio-ML", "Markowitz-ML", "Static-ML"]
        assert names[-2:] == ["Minimum variance", "1/N"]
        assert len(names) == 2 + 8 + 2 and len(set(names)) == len(names)    # 2 x 2 x 2 static arms
        assert (bmk["reason"] == "").all() and (bmk["n"] == len(out["months"])).all()
        assert list(pf["type"].drop_duplicates()) == names
        assert len(pf) == len(names) * len(out["months"])


def test_default_arms_and_config(data):
    cfg = Config.default()
    assert cfg.settings["bmk"] == {"l_vec": None, "p_vec": None,
                                   "static": {"k": [1.0], "u": [1.0], "g": [0.0]}}
    assert benchmarks.static_arms(cfg) == [("Static-ML", 1.0, 1.0, 0.0)]
    cb = benchmarks.bmk_config(cfg)
    assert list(cb.l_vec) == list(cfg.settings["rff"]["l_vec"]) and cb.p_vec == cfg.p_vec
    ref = cfg.override(["bmk.static.k=[1,0.3333333333333333,0.2]", "bmk.static.u=[0.25,0.5,1]",
                        "bmk.static.g=[0,1,2]"])
    assert len(benchmarks.static_arms(ref)) == 27
    with pytest.raises(ValueError, match="p_max"):
        benchmarks.bmk_config(cfg.override(["bmk.p_vec=[1024]"]))


def test_missing_barra_row_is_a_key_error(data):
    _, chars, barra, wealth, rf = data
    layout = {"B": 1, "N": 4, "months": np.asarray([int(barra.months[-1])]),
              "ids": [np.asarray([10 ** 6 + 7], np.int64)]}
    with pytest.raises(KeyError):
        benchmarks.barra_rows(barra, layout)


def test_stage_registration(data):
    from pfml.pipeline import _DEPS, _SIBLING_OF, ALL_STAGES, MAIN_STAGES, SIDE_STAGES, Pipeline
    assert "pfml-bmk" in SIDE_STAGES and "pfml-bmk" not in MAIN_STAGES
    assert _SIBLING_OF["pfml-bmk"] == "pfml-best-hps"
    cfg = data[0]
    pipe = Pipeline(cfg, device="cpu")
    key, keys = "", {}
    for st in [s for s in ALL_STAGES if s != "pfml-fi"]:        # the chain before this stage
        key = key + "|" + cfg.hash(*_DEPS.get(st, ())) + st
        keys[st] = key
    assert all(pipe._keys[st] == keys[st] for st in keys)
    assert pipe._keys["pfml-fi"] == keys["pfml-best-hps"] + "|" + cfg.hash(*_DEPS["pfml-fi"]) \
        + "pfml-fi"
    assert pipe._keys["pfml-bmk"] == keys["pfml-best-hps"] + "|" + \
        cfg.hash(*_DEPS["pfml-bmk"]) + "pfml-bmk"
    other = Pipeline(cfg.override(["bmk.static.g=[0,1]"]), device="cpu")
    assert other._keys["pfml-bmk"] != pipe._keys["pfml-bmk"]
    assert all(other._keys[st] == pipe._keys[st] for st in pipe._keys if st != "pfml-bmk")
    bare = copy.deepcopy(cfg)
    del bare.settings["bmk"]
    assert bare.hash() == cfg.hash()
    with pytest.raises(ValueError, match="unknown stage"):
        pipe.run(["pfml-nothing"])


def test_world_size_above_one_is_refused(data):
    from pfml.parallel import dist as pdist
    from pfml.pipeline import Pipeline
    old = pdist._ENV
    pdist.set_env(pdist.DistEnv(rank=0, world_size=2))
    try:
        with pytest.raises(RuntimeError, match="world size 1"):
            _run(data, False)
        pipe = Pipeline.__new__(Pipeline)
        pipe.env = pdist.DistEnv(rank=0, world_size=2)
        with pytest.raises(RuntimeError, match="world size 1"):
            pipe._pfml_bmk()
    finally:
        pdist.set_env(old)


def test_fault_injection_recomputes_the_arm(data, runs):
    """run.fault_inject = "pfml-bmk" poisons one w_start of the last chain arm: it is
    recomputed (here by the same CPU branch) and the frame is the clean run's."""
    from pfml.utils.log import COUNTERS
    cfg = _cfg(data, False)
    cfg.run.fault_inject = "pfml-bmk"
    n0 = COUNTERS.as_dict().get("pfml_bmk.recomputed_arms", 0)
    out = _run(data, False, cfg=cfg)
    assert COUNTERS.as_dict().get("pfml_bmk.recomputed_arms", 0) == n0 + 1
    assert (out["bmk"]["reason"] == "").all()
    got, ref = out["bmk"], runs[False]["bmk"]
    hit = (got["type"] == "Minimum variance").to_numpy()
    assert hit.sum() == 1 and list(got["type"]) == list(ref["type"])
    assert np.array_equal(got.loc[~hit, NUM].to_numpy(float), ref.loc[~hit, NUM].to_numpy(float))
    assert np.allclose(got.loc[hit, NUM].to_numpy(float), ref.loc[hit, NUM].to_numpy(float), **TOL)


def test_failing_arm_is_a_nan_row_and_the_rest_stands(data, runs):
    """A Static-ML arm with k = NaN stays non-finite on the CPU re-run: a NaN row with a
    reason; every other row unchanged."""
    cfg = _cfg(data, False).override(["bmk.static.k=[1,0.5,nan]"])
    out = _run(data, False, cfg=cfg)
    bmk, ref = out["bmk"], runs[False]["bmk"]
    failed = bmk[bmk["reason"] != ""]
    assert len(failed) == 4 and failed["type"].str.startswith("Static-ML(nan").all()
    assert (failed["n"] == 0).all() and failed["reason"].str.contains("non-finite").all()
    assert np.isnan(failed[NUM[1:]].to_numpy(float)).all()
    good = bmk[bmk["reason"] == ""].reset_index(drop=True)
    assert list(good["type"]) == list(ref["type"])
    assert np.array_equal(good[NUM].to_numpy(float), ref[NUM].to_numpy(float))
    assert set(out["pf"]["type"]) == set(ref["type"])
