"""Multiperiod-ML on the CPU path (models/multiperiod.py, the torch branch of
ops/multiperiod.py): the closed form against a direct solve of the stacked finite-horizon QP,
the fold and the chain against the longdouble references of tests/mp_oracle.py, the horizon
targets against a pandas merge, one horizon's ridge coefficients against pandas-accumulated
shifted sums, every arm against a longdouble dense month loop in w-space (explicit powers of m)
in compat and corrected mode, the Portfolio-ML row, the unchanged default ``prediction_reals``,
the stage registration and the failure isolation.

Stage inputs: the session's ``small_data`` panel as tests/test_benchmarks_cpu.py uses it, with
mp.K = 3 and a one-entry mp.p_vec."""
import copy
import os
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

import mp_oracle as mpo
from pfml.config import Config, get_features
from pfml.data.io import CSV_COLUMNS
from pfml.models import benchmarks, frontier, multiperiod, portfolio, search
from pfml.models import pfml_inputs as pin
from pfml.ops.multiperiod import horizon_fold, mp_chain
from pfml.utils.dates import month_end, month_index, pfml_date_grids

LD = np.longdouble
STAT = ["inv", "shorting", "turnover", "r", "tc"]
NUM = [c for c in frontier.SUMMARY_COLUMNS if c != "type"]
TOL = dict(rtol=1e-10, atol=1e-12)          # the benchmark tests' tolerances
YEARS = ["pf.dates.start_year=2008", "pf.dates.end_yr=2012", "pf.dates.split_years=1",
         "pf_ml.p_vec=[16,32]"]
MP = ["mp.K=3", "mp.p_vec=[16]", "mp.u=[1,0.5,0]", "mp.gbar=0.9"]


def _t(x):
    return torch.as_tensor(x)


def _fold(inp, gbar=1.0, mu=None):
    mu = inp["mu"] if mu is None else mu
    return horizon_fold(_t(inp["mt"]), _t(inp["a"]), _t(mu), _t(inp["wealth"]),
                        _t(inp["n_rows"]), gbar)


def _chain(inp, V, arms=None):
    arms = list(range(inp["A"])) if arms is None else arms
    return mp_chain(_t(inp["mt"]), _t(inp["a"]), V, _t(inp["u"][arms]), _t(inp["n_rows"]),
                    _t(inp["grow"]), _t(inp["nmap"]), _t(inp["hit"]), _t(inp["ws0"][arms]))


# ---------------------------------------------------------------------------------------------
# the kernels' formulas (torch branch)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(5, 0), (7, 3)])
def test_closed_form_is_the_stacked_qp(n, seed):
    """Deterministic growth (sigma_gr = 11'): m_tilde is the fixed point of (x + 2I - m)^-1, and
    in y = w / a the problem is max sum_t c_t'y_t - y_t'x y_t / 2 - |y_t - y_{t-1}|^2 / 2 with
    c_t = a o mu_t / W.  Its first-order conditions over T = 60 months - a block-tridiagonal
    system, solved directly - against fold + chain over the first two months, mu known for 12
    months and zero after: 1e-12 max|w| (measured 3e-16 max|w|)."""
    rng = np.random.default_rng(seed)
    T, K, W = 60, 12, 1e10
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    e = rng.uniform(0.5, 2.0, n)
    x = (Q * e) @ Q.T
    mt = (Q * (((e + 2.0) - np.sqrt((e + 2.0) ** 2 - 4.0)) / 2.0)) @ Q.T
    assert np.abs(mt - np.linalg.inv(x + 2.0 * np.eye(n) - mt)).max() < 1e-14
    a = 1e4 * rng.uniform(0.5, 2.0, n)
    mu = np.zeros((T + K, n))
    mu[:K] = 1e-2 * rng.standard_normal((K, n))
    w0 = 1e-2 * rng.standard_normal(n)
    big = np.zeros((T * n, T * n))
    rhs = np.zeros(T * n)
    for t in range(T):
        s = slice(t * n, (t + 1) * n)
        big[s, s] = x + (2.0 if t + 1 < T else 1.0) * np.eye(n)
        if t:
            big[s, (t - 1) * n: t * n] = big[(t - 1) * n: t * n, s] = -np.eye(n)
        rhs[s] = a * mu[t] / W
    rhs[:n] += w0 / a
    w_qp = np.linalg.solve(big, rhs).reshape(T, n) * a
    B = 2
    mu_hat = np.stack([mu[tau: tau + B] for tau in range(K)])           # [K, B, n]
    eye = np.tile(np.arange(n, dtype=np.int64), (B, 1))
    nr = torch.full((B,), n, dtype=torch.int32)
    mt_b, a_b = _t(np.stack([mt] * B)), _t(np.stack([a] * B))
    V = horizon_fold(mt_b, a_b, _t(mu_hat), torch.full((B,), W, dtype=torch.float64), nr, 1.0)
    _, Wopt, _ = mp_chain(mt_b, a_b, V, [1.0], nr, torch.ones(B, n, dtype=torch.float64),
                          _t(eye), torch.ones(B, n, dtype=torch.float64), _t(w0))
    err = np.abs(Wopt[0].numpy() - w_qp[:B]).max(1)
    print("closed form against the stacked QP:", err, "max|w| =", np.abs(w_qp[:B]).max())
    assert (err <= 1e-12 * np.abs(w_qp[:B]).max()).all()


def test_k1_and_gbar0_are_the_first_horizon():
    inp = mpo.mp_inputs(40, 4, 4, 1, seed=1)
    want = (_t(inp["a"]) * _t(inp["mu"][0])) / _t(inp["wealth"])[:, None]
    assert torch.equal(_fold(inp, mu=inp["mu"][:1]), want)
    assert torch.equal(_fold(inp, gbar=0.0), want)


@pytest.mark.parametrize("ragged", [False, True])
def test_torch_branch_within_the_oracle_bounds(ragged):
    inp = mpo.mp_inputs(40, 5, 4, 3, seed=2, ragged=ragged)
    V = _fold(inp, 0.8)
    mpo.check_fold(inp, V.numpy(), 0.8)
    out = _chain(inp, V)
    mpo.check_chain(inp, V.numpy(), *(o.numpy() for o in out))
    one = _chain(inp, V, arms=[2])
    for o, r in zip(one, out):
        assert torch.equal(o[0], r[2])


@pytest.mark.parametrize("h", [0, 1, 3])
def test_a_dropped_horizon_breaks_the_bound_in_every_month(h):
    inp = mpo.mp_inputs(40, 4, 4, 1, seed=3)
    mu = inp["mu"].copy()
    mu[h] = 0.0
    V = _fold(inp, mu=mu).numpy()
    for t in range(inp["B"]):
        with pytest.raises(AssertionError, match="over the bound"):
            mpo.check_fold(inp, V, 1.0, months=[t])


def test_shape_and_dtype_errors_are_raised_on_the_host():
    inp = mpo.mp_inputs(8, 2, 2, 2, seed=4)
    V = _fold(inp)
    with pytest.raises(TypeError):
        horizon_fold(_t(inp["mt"]).float(), _t(inp["a"]), _t(inp["mu"]), _t(inp["wealth"]),
                     _t(inp["n_rows"]))
    with pytest.raises(ValueError):
        horizon_fold(_t(inp["mt"]), _t(inp["a"]), _t(inp["mu"][:, :1]), _t(inp["wealth"]),
                     _t(inp["n_rows"]))
    with pytest.raises(ValueError):
        horizon_fold(_t(inp["mt"]), _t(inp["a"]), _t(inp["mu"][:0]), _t(inp["wealth"]),
                     _t(inp["n_rows"]))
    with pytest.raises(TypeError):
        horizon_fold(_t(inp["mt"]), _t(inp["a"]), _t(inp["mu"]), _t(inp["wealth"]),
                     _t(inp["n_rows"]).double())
    args = [_t(inp["mt"]), _t(inp["a"]), V, _t(inp["u"]), _t(inp["n_rows"]), _t(inp["grow"]),
            _t(inp["nmap"]), _t(inp["hit"]), _t(inp["ws0"])]
    for pos, bad, exc in ((6, _t(inp["nmap"]).int(), TypeError),
                          (8, _t(inp["ws0"][:, :4]), ValueError),
                          (2, V[:1], ValueError), (5, _t(inp["grow"]).float(), TypeError)):
        a2 = list(args)
        a2[pos] = bad
        with pytest.raises(exc):
            mp_chain(*a2)


# ---------------------------------------------------------------------------------------------
# the stage's inputs
# ---------------------------------------------------------------------------------------------
def _grids(cfg, barra):
    s = cfg.settings
    return pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                           s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                           s["pf"]["dates"]["split_years"])


@pytest.fixture(scope="module")
def data(small_data, tmp_path_factory):
    from pfml.data import io
    from pfml.models.risk import BarraCov
    d = str(tmp_path_factory.mktemp("mp_cpu") / "data")
    shutil.copytree(small_data.run.data_dir, d)
    cfg = small_data.override(YEARS + MP + [f"run.data_dir={d}"])
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
    return multiperiod.multiperiod_portfolios(cfg or _cfg(data, compat), chars, barra, wealth,
                                              rf, "cpu", **kw)


@pytest.fixture(scope="module")
def runs(data):
    return {compat: _run(data, compat, keep_weights=True) for compat in (False, True)}


@pytest.fixture(scope="module")
def model(data):
    """Corrected mode: the S4 plan, the horizon targets and the summands (the stage's calls)."""
    _, chars, barra, wealth, rf = data
    cfg = _cfg(data, False)
    g = _grids(cfg, barra)
    plan = pin.make_s4_plan(cfg, chars, barra, wealth, rf, "cpu", g["m2"])
    cfg_m = multiperiod.mp_config(cfg)
    Y = multiperiod.horizon_targets(chars, plan, 3)
    out = benchmarks.prediction_reals(plan, cfg_m, g["oos"], targets=Y)
    return dict(cfg=cfg, cfg_m=cfg_m, plan=plan, Y=Y, out=out, m2=g["m2"], oos=g["oos"])


def test_horizon_targets_against_a_pandas_merge(data, model):
    chars, plan, Y = data[1], model["plan"], model["Y"].numpy()
    assert Y.shape == (3, len(model["m2"]), plan.N)
    mi = month_index(chars["eom"])
    look = pd.DataFrame({"id": chars["id"].to_numpy(np.int64), "mi": mi,
                         "y": chars["ret_ld1"].to_numpy(np.float64)})
    T = len(model["m2"])
    for t in (0, T // 2, T - 2, T - 1):
        ids = np.asarray(plan.sig_ids[t], np.int64)
        for h in (1, 2, 3):
            left = pd.DataFrame({"id": ids, "mi": int(model["m2"][t]) + h - 1})
            y = left.merge(look, on=["id", "mi"], how="left")["y"].to_numpy()
            want = np.where(np.isfinite(y), y, 0.0)
            assert np.array_equal(Y[h - 1, t, :len(ids)], want), (t, h)
            assert not Y[h - 1, t, len(ids):].any()
    assert not Y[2, T - 1].any() and not Y[1, T - 1].any()      # beyond the panel's last month
    b0 = 0
    for bt in plan.batches:
        r = bt.r.numpy()
        ok = np.isfinite(r)
        assert np.array_equal(Y[0, b0:b0 + len(bt.months)][ok], r[ok])
        b0 += len(bt.months)


def test_default_prediction_reals_is_unchanged(model):
    """Without targets: five results, each torch.equal to the first five of the call with
    targets (whose code path the new argument must not touch)."""
    m = model
    base = benchmarks.prediction_reals(m["plan"], m["cfg_m"], m["oos"])
    assert len(base) == 5 and len(m["out"]) == 6
    for b, w in zip(base[:4], m["out"][:4]):
        assert torch.equal(b, w)
    for zb, zw in zip(base[4], m["out"][4]):
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(zb, zw))
    rh = m["out"][5]
    assert rh.shape == (3,) + tuple(base[0].shape)
    assert torch.allclose(rh[0], base[0], rtol=1e-12, atol=1e-15)


def _z_oracle(chars, ids, month, W):
    """As tests/test_benchmarks_cpu.py: the standardised random-feature block in pandas."""
    mi = month_index(chars["eom"])
    sub = chars[mi == int(month)].set_index("id").loc[list(ids)]
    zz = sub[get_features()].to_numpy(np.float64) @ W
    S = pd.DataFrame(np.ones((len(ids), 1 + 2 * W.shape[1])))
    S.iloc[:, 1::2] = np.cos(zz)
    S.iloc[:, 2::2] = np.sin(zz)
    dm = S - S.mean()
    dm[0] = S[0]
    Z = dm / np.sqrt((dm ** 2).sum())
    return Z.to_numpy(np.float64), sub["ret_ld1"].to_numpy(np.float64)


def test_horizon_three_coefficients_from_pandas_sums(data, model):
    """beta of the first hp year at horizon 3: the pair (Z_s, y_s^(3)) enters the window at
    position s + 2, so the window of months [0, stop) holds the pairs s < stop - 2; the mean
    still divides by the window's month count."""
    chars, m = data[1], model
    plan, cfg_m, m2 = m["plan"], m["cfg_m"], m["m2"]
    h, g = 3, 0
    R = multiperiod.horizon_reals(m["out"][5][h - 1], m["out"][1], h, m2, cfg_m.hp_years)
    assert not R.denom[:, :h - 1].any() and not R.r_tilde[:, :h - 1].any()
    grid = search.grid_search(R, cfg_m)
    sp = search.make_plan(m2, np.asarray(cfg_m.hp_years))
    stop = int(sp.seg_stop[0])
    mi = month_index(chars["eom"])
    look = pd.DataFrame({"id": chars["id"].to_numpy(np.int64), "mi": mi,
                         "y": chars["ret_ld1"].to_numpy(np.float64)})
    p = cfg_m.p_vec[0]
    SD, Sr = np.zeros((p + 1, p + 1)), np.zeros(p + 1)
    for s in range(stop - (h - 1)):
        ids = np.asarray(plan.sig_ids[s], np.int64)
        Z, y1 = _z_oracle(chars, ids, m2[s], plan.W[g])
        y3 = pd.DataFrame({"id": ids, "mi": int(m2[s]) + h - 1}).merge(
            look, on=["id", "mi"], how="left")["y"].fillna(0.0).to_numpy()
        ok = np.isfinite(y1)
        Zk = Z[ok][:, : p + 1]
        SD += Zk.T @ Zk
        Sr += Zk.T @ y3[ok]
    years = list(np.asarray(grid.years_local))
    yi = years.index(int(cfg_m.hp_years[0]))
    checked = 0
    for l, lam in enumerate(cfg_m.l_vec):
        if lam <= 0:
            continue
        want = np.linalg.solve(SD / stop + lam * np.eye(p + 1), Sr / stop)
        got = grid.beta[g, yi, 0, l, : p + 1].numpy()
        assert np.allclose(got, want, rtol=1e-9, atol=0.0), l
        checked += 1
    assert checked >= 3


def test_non_consecutive_months_are_refused(data, model):
    m = model
    plan = copy.copy(m["plan"])
    plan.months = np.asarray(plan.months).copy()
    plan.months[-1] += 1
    with pytest.raises(ValueError, match="consecutive"):
        multiperiod.horizon_predictions(m["cfg_m"], plan, {"m2": plan.months, "oos": m["oos"]},
                                        {}, m["Y"], "cpu")


# ---------------------------------------------------------------------------------------------
# the arms
# ---------------------------------------------------------------------------------------------
def _ld_matmul(A, B):
    out = np.zeros((A.shape[0], B.shape[1]), LD)
    for l in range(A.shape[1]):
        out += np.outer(A[:, l], B[l])
    return out


def _arm_oracle(data, cfg, out, u):
    """A longdouble month loop in w-space: m = diag(a) m_tilde diag(1/a), its powers formed
    explicitly, w = m w_start + sum_tau gbar^tau m^(tau+1) (a^2 o u mu_hat_{tau+1}) / W, the
    drift through the ids -> the weights frame (id, eom, w_start, w)."""
    _, chars, _, wealth, _ = data
    gbar = float(cfg.settings["mp"]["gbar"])
    mt_all, a_all = out["m"]
    mu_hat = out["mu_hat"]
    K = mu_hat.shape[0]
    mi = month_index(chars["eom"])
    wmi = month_index(wealth["eom"])
    ws, frames = None, []
    for tb, d in enumerate(out["months"]):
        sub = chars[(mi == int(d)) & chars["valid"].to_numpy()].sort_values("id")
        ids = sub["id"].to_numpy(np.int64)
        n = len(ids)
        wrow = wealth[wmi == int(d)].iloc[0]
        a = a_all[tb, :n].numpy().astype(LD)
        m = a[:, None] * mt_all[tb, :n, :n].numpy().astype(LD) / a[None, :]
        if ws is None:
            me = sub["me"].to_numpy(np.float64)
            start = me / me.sum()
        else:
            start = np.asarray([ws.get(int(i), 0.0) for i in ids])
        w = _ld_matmul(m, start.astype(LD)[:, None])[:, 0]
        mp = m.copy()
        for tau in range(K):
            c = a * a * LD(u) * mu_hat[tau, tb, :n].astype(LD) / LD(float(wrow["wealth"]))
            w = w + LD(gbar) ** tau * _ld_matmul(mp, c[:, None])[:, 0]
            mp = _ld_matmul(mp, m)
        w = w.astype(np.float64)
        frames.append(pd.DataFrame({"id": ids, "eom": month_end(int(d))[0], "w_start": start,
                                    "w": w}))
        grown = w * (1.0 + sub["tr_ld1"].to_numpy(np.float64)) / (1.0 + float(wrow["mu_ld1"]))
        ws = dict(zip(ids.tolist(), grown.tolist()))
    return pd.concat(frames, ignore_index=True)


ARMS = [("Multiperiod-ML", 1.0), ("Multiperiod-ML(0.5)", 0.5), ("Multiperiod-ML(0)", 0.0)]


@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("name,u", ARMS)
def test_arm_against_the_dense_longdouble_loop(data, runs, compat, name, u):
    _, chars, _, wealth, _ = data
    cfg, out = _cfg(data, compat), runs[compat]
    assert out["K"] == 3 and out["mu_hat"].shape[0] == 3
    ow = _arm_oracle(data, cfg, out, u)
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
    row = out["mp"][out["mp"]["type"] == name].iloc[0]
    assert np.allclose(row[NUM].to_numpy(float), summ[NUM].to_numpy(float), **TOL)
    assert row["u"] == u


@pytest.mark.parametrize("compat", [False, True])
def test_portfolio_ml_row_is_backtest_device(data, runs, compat):
    _, chars, barra, wealth, rf = data
    cfg = _cfg(data, compat)
    bt = frontier.run_point(cfg, chars, barra, wealth, rf, "cpu", _grids(cfg, barra), {})
    out = runs[compat]
    mine = out["pf"][out["pf"]["type"] == "Portfolio-ML"]
    assert np.array_equal(mine[STAT].to_numpy(), bt["pf"][STAT].to_numpy())
    summ = portfolio.pf_summary(bt["pf"], float(cfg.pf_set["gamma_rel"])).iloc[0]
    assert np.array_equal(out["mp"].loc[0, NUM].to_numpy(float), summ[NUM].to_numpy(float))
    assert out["chosen"] == bt["chosen"]


def test_frames_and_hps(runs):
    for out in runs.values():
        mp, pf, hps = out["mp"], out["pf"], out["hps"]
        assert list(mp.columns) == CSV_COLUMNS["mp.csv"] == multiperiod.MP_COLUMNS
        assert list(pf.columns) == CSV_COLUMNS["mp_pf.csv"] == multiperiod.MP_PF_COLUMNS
        assert list(hps.columns) == CSV_COLUMNS["mp_hps.csv"] == multiperiod.MP_HPS_COLUMNS
        names = list(mp["type"])
        assert names == ["Portfolio-ML"] + [n for n, _ in ARMS]
        assert (mp["reason"] == "").all() and (mp["n"] == len(out["months"])).all()
        assert list(pf["type"].drop_duplicates()) == names
        assert len(pf) == len(names) * len(out["months"])
        assert sorted(set(hps["horizon"])) == [1, 2, 3] and (hps["val_mse"] > 0).all()
        for h in (1, 2, 3):
            assert list(hps[hps["horizon"] == h]["hp_year"]) == sorted(out["chosen_mp"][h - 1])
        assert out["missing_mu"] == 0


def test_defaults_and_config():
    cfg = Config.default()
    assert cfg.settings["mp"] == {"K": None, "u": [1.0], "gbar": 1.0, "l_vec": None,
                                  "p_vec": None}
    assert multiperiod.horizons(cfg) == cfg.settings["pf"]["hps"]["m1"]["K"] == 12
    assert multiperiod.horizons(cfg.override(["mp.K=4"])) == 4
    assert multiperiod.mp_arms(cfg) == [("Multiperiod-ML", 1.0)]
    assert multiperiod.mp_arms(cfg.override(["mp.u=[0.25,0.5,1]"])) == [
        ("Multiperiod-ML", 1.0), ("Multiperiod-ML(0.25)", 0.25), ("Multiperiod-ML(0.5)", 0.5)]
    cm = multiperiod.mp_config(cfg)
    assert list(cm.l_vec) == list(cfg.settings["rff"]["l_vec"]) and cm.p_vec == cfg.p_vec
    with pytest.raises(ValueError, match="p_max"):
        multiperiod.mp_config(cfg.override(["mp.p_vec=[1024]"]))
    with pytest.raises(ValueError, match="mp.K"):
        multiperiod.horizons(cfg.override(["mp.K=0"]))


def test_stage_registration(data):
    from pfml.pipeline import _DEPS, _SIBLING_OF, ALL_STAGES, MAIN_STAGES, SIDE_STAGES, Pipeline
    assert SIDE_STAGES[-1] == "pfml-mp" and "pfml-mp" not in MAIN_STAGES + ALL_STAGES
    assert _SIBLING_OF["pfml-mp"] == "pfml-best-hps"
    assert set(_DEPS["pfml-mp"]) == (set(_DEPS["pfml-bmk"]) - {"bmk"}) | {"mp"}
    cfg = data[0]
    pipe = Pipeline(cfg, device="cpu")
    key, keys = "", {}
    for st in [s for s in ALL_STAGES if s != "pfml-fi"]:        # the chain before this stage
        key = key + "|" + cfg.hash(*_DEPS.get(st, ())) + st
        keys[st] = key
    assert all(pipe._keys[st] == keys[st] for st in keys)
    for st in ("pfml-fi", "pfml-bmk", "pfml-mp"):
        assert pipe._keys[st] == keys["pfml-best-hps"] + "|" + cfg.hash(*_DEPS[st]) + st
    other = Pipeline(cfg.override(["mp.u=[1,2]"]), device="cpu")
    assert other._keys["pfml-mp"] != pipe._keys["pfml-mp"]
    assert all(other._keys[st] == pipe._keys[st] for st in pipe._keys if st != "pfml-mp")
    bare = copy.deepcopy(cfg)
    del bare.settings["mp"]
    assert bare.hash() == cfg.hash()


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
            pipe._pfml_mp()
    finally:
        pdist.set_env(old)


def test_fault_injection_recomputes_the_arm(data, runs):
    """run.fault_inject = "pfml-mp" poisons one w_start of the last arm: it is recomputed (here
    by the same CPU branch) and the frame is the clean run's."""
    from pfml.utils.log import COUNTERS
    cfg = _cfg(data, False)
    cfg.run.fault_inject = "pfml-mp"
    n0 = COUNTERS.as_dict().get("pfml_mp.recomputed_arms", 0)
    out = _run(data, False, cfg=cfg)
    assert COUNTERS.as_dict().get("pfml_mp.recomputed_arms", 0) == n0 + 1
    assert (out["mp"]["reason"] == "").all()
    got, ref = out["mp"], runs[False]["mp"]
    assert list(got["type"]) == list(ref["type"])
    assert np.array_equal(got[NUM].to_numpy(float), ref[NUM].to_numpy(float))


def test_failing_arm_is_a_nan_row_and_the_rest_stands(data, runs):
    """An arm with u = NaN stays non-finite on the CPU re-run: a NaN row with a reason; every
    other row unchanged."""
    cfg = _cfg(data, False).override(["mp.u=[1,0.5,0,nan]"])
    out = _run(data, False, cfg=cfg)
    mp, ref = out["mp"], runs[False]["mp"]
    failed = mp[mp["reason"] != ""]
    assert list(failed["type"]) == ["Multiperiod-ML(nan)"]
    assert (failed["n"] == 0).all() and failed["reason"].str.contains("non-finite").all()
    assert np.isnan(failed[NUM[1:]].to_numpy(float)).all()
    good = mp[mp["reason"] == ""].reset_index(drop=True)
    assert list(good["type"]) == list(ref["type"])
    assert np.array_equal(good[NUM].to_numpy(float), ref[NUM].to_numpy(float))
    assert set(out["pf"]["type"]) == set(ref["type"])
