"""The efficient-frontier driver on the CPU path: a 2 x 2 frontier against the plain stage
functions run per point, the reused S4 plan, wealth = 1, resume, the world-size guard and the
torch path of ``pf_stats``."""
import copy

import numpy as np
import pandas as pd
import pytest
import torch

from pfml.config import Config
from pfml.data.io import CSV_COLUMNS
from pfml.models import frontier, portfolio, search
from pfml.models import pfml_inputs as pin
from pfml.utils.dates import month_end, pfml_date_grids

W_VEC, G_VEC = [1e10, 1.0], [10.0, 20.0]
STAT = ["inv", "shorting", "turnover", "r", "tc"]


def _grids(cfg, barra):
    s = cfg.settings
    return pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                           s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                           s["pf"]["dates"]["split_years"])


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """40-stock synthetic engine inputs; the small p_vec / years of models/pipeline_step.py
    extended by three OOS years (Dec 2001 .. Nov 2004).  Compat mode reads rff_w.csv."""
    from pfml.config import get_features
    from pfml.data.synthetic import engine_inputs
    d = str(tmp_path_factory.mktemp("ef_cpu"))
    cfg = Config.default().override(["pf_ml.p_vec=[8,16]", "pf.dates.start_year=2001",
                                     "pf.dates.end_yr=2004", "pf.dates.split_years=1",
                                     "split.test_end=2004-12-31", f"run.data_dir={d}"])
    rng = np.random.default_rng(5)
    pd.DataFrame(rng.standard_normal((len(get_features()), cfg.p_max // 2))).to_csv(
        f"{d}/rff_w.csv")
    return (cfg,) + engine_inputs(n_stocks=40, start="1993-01-31", end="2004-12-31")


def _cfg(data, compat):
    cfg = copy.deepcopy(data[0])
    cfg.run.compat_mode = compat
    return cfg


@pytest.fixture(scope="module")
def ef_corrected(data):
    _, chars, barra, wealth, rf = data
    return frontier.efficient_frontier(_cfg(data, False), chars, barra, wealth, rf, "cpu",
                                       wealth_vec=W_VEC, gamma_vec=G_VEC, keep_weights=True)


def _plain_point(cfg_pt, chars, barra, wealth_pt, rf):
    """The point through the existing functions, S4 with a fresh plan."""
    g = _grids(cfg_pt, barra)
    m2, oos = g["m2"], g["oos"]
    res = pin.build_inputs(cfg_pt, chars, barra, wealth_pt, rf, "cpu", months=m2, keep_m=oos)
    R = search.complete_local_reals(res.reals.r_tilde, res.reals.denom, m2, cfg_pt.hp_years)
    grid = search.grid_search(R, cfg_pt)
    val = search.validation_frame(grid, cfg_pt)
    years_b, beta_b = search.gather_beta(grid)
    aims = portfolio.aim_portfolios(cfg_pt, val, years_b, beta_b, m2, res.signal_t, res.ids, oos)
    hps = portfolio.hps_bundle(aims, val, res.rff_w)
    _, chosen, aim_df = portfolio.best_hps(hps, oos)
    w = portfolio.pfml_weights(cfg_pt, chars, barra, wealth_pt, rf, aim_df, oos, "cpu",
                               m_cache=res.m_keep, n_pad=pin.universe_npad(chars, m2))
    pf = portfolio.pf_ts(w, chars, wealth_pt, compat=cfg_pt.run.compat_mode)
    summ = portfolio.pf_summary(pf, float(cfg_pt.pf_set["gamma_rel"]))
    picks = {}
    for d in oos:
        a = hps[chosen[int(d)]["g"]]["aim_pfs_list"][int(d)]
        picks[int(month_end(int(d) + 1).year[0]) - 1] = (chosen[int(d)]["g"], a["p"], a["l"])
    return res, w, pf, summ, picks


def test_frontier_shape_columns_finite(ef_corrected):
    ef, pf = ef_corrected["ef"], ef_corrected["pf"]
    assert list(ef.columns) == CSV_COLUMNS["ef.csv"] == frontier.EF_COLUMNS
    assert list(pf.columns) == CSV_COLUMNS["ef_pf.csv"] == frontier.PF_COLUMNS
    assert len(ef) == 4
    assert [tuple(x) for x in ef[["wealth_end", "gamma_rel"]].to_numpy()] == \
        [(w, g) for w in W_VEC for g in G_VEC]
    assert len(pf) == 4 * 36 and (ef["n"] == 36).all()
    num = [c for c in ef.columns if c not in ("type", "s4_fallbacks")]
    assert np.isfinite(ef[num].to_numpy(float)).all()
    assert np.isfinite(pf[STAT].to_numpy(float)).all()
    # the overrides reached S4: the points differ
    assert ef["sd"].nunique() == 4 and ef["tc"].nunique() == 4


def test_wealth_one_finishes_finite(ef_corrected):
    ef = ef_corrected["ef"]
    one = ef[ef["wealth_end"] == 1.0]
    assert len(one) == 2
    assert np.isfinite(one[["r", "sd", "tc", "r_tc", "sr", "obj"]].to_numpy(float)).all()
    # TC ~ 0 at wealth 1
    assert (one["tc"].abs() < 1e-6).all()


@pytest.mark.parametrize("compat", [False, True])
def test_points_equal_plain_functions(data, ef_corrected, compat):
    _, chars, barra, wealth, rf = data
    cfg = _cfg(data, compat)
    pts = [(1e10, 10.0), (1.0, 20.0)] if not compat else [(1e9, 20.0)]
    if compat:
        out = frontier.efficient_frontier(cfg, chars, barra, wealth, rf, "cpu",
                                          wealth_vec=[1e9], gamma_vec=[20.0], keep_weights=True)
    else:
        out = ef_corrected
    for W, gam in pts:
        cfg_pt = frontier.point_config(cfg, W, gam)
        wealth_pt = frontier.scaled_wealth(cfg, wealth, W)
        _, w, pf, summ, picks = _plain_point(cfg_pt, chars, barra, wealth_pt, rf)
        assert out["chosen"][(W, gam)] == picks
        got_w = out["weights"][(W, gam)]
        assert got_w[["eom", "id"]].equals(w[["eom", "id"]])
        for c in ("mu_ld1", "tr_ld1", "w_start", "w"):
            assert np.allclose(got_w[c].to_numpy(), w[c].to_numpy(), rtol=1e-8, atol=1e-12,
                               equal_nan=True), c
        sel = out["pf"][(out["pf"]["wealth_end"] == W) & (out["pf"]["gamma_rel"] == gam)]
        assert list(pd.to_datetime(sel["eom_ret"])) == list(pd.to_datetime(pf["eom_ret"]))
        assert np.allclose(sel[STAT].to_numpy(), pf[STAT].to_numpy(), rtol=1e-8, atol=1e-12)
        row = out["ef"][(out["ef"]["wealth_end"] == W) & (out["ef"]["gamma_rel"] == gam)]
        num = [c for c in summ.columns if c != "type"]
        assert np.allclose(row[num].to_numpy(float), summ[num].to_numpy(float), rtol=1e-8,
                           atol=1e-12)


def test_scaled_wealth_is_the_frame_at_its_own_end_wealth(data):
    cfg, _, _, wealth, _ = data
    assert frontier.frame_end_wealth(cfg, wealth) == 1e10
    same = frontier.scaled_wealth(cfg, wealth, 1e10)
    assert np.array_equal(same["wealth"].to_numpy(), wealth["wealth"].to_numpy())
    assert same["mu_ld1"].equals(wealth["mu_ld1"])
    tenth = frontier.scaled_wealth(cfg, wealth, 1e9)
    assert np.allclose(tenth["wealth"].to_numpy(), wealth["wealth"].to_numpy() / 10, rtol=1e-15)


def test_reused_s4_plan_gives_bitwise_summands(data):
    """A plan made for one point and re-aimed at another feeds S4 the operands of a fresh
    plan for that point: lambda (padding included), wealth, and so the summands, bitwise."""
    _, chars, barra, wealth, rf = data
    cfg = _cfg(data, False)
    m2 = _grids(cfg, barra)["m2"]
    base = pin.make_s4_plan(frontier.point_config(cfg, 1e10, 10.0), chars, barra, wealth, rf,
                            "cpu", m2)
    cfg_pt = frontier.point_config(cfg, 1e9, 20.0)
    wealth_pt = frontier.scaled_wealth(cfg, wealth, 1e9)
    fresh = pin.make_s4_plan(cfg_pt, chars, barra, wealth_pt, rf, "cpu", m2)
    again = frontier.repoint_s4_plan(base, cfg_pt, wealth_pt)
    assert len(fresh.batches) == len(again.batches)
    for a, b in zip(fresh.batches, again.batches):
        assert torch.equal(a.lam, b.lam) and torch.equal(a.w, b.w)
        assert not torch.equal(a.lam, base.batches[0].lam[: a.lam.shape[0]])
    ra = pin.run_plan(fresh, cfg_pt).reals
    rb = pin.run_plan(again, cfg_pt).reals
    assert torch.equal(ra.denom, rb.denom) and torch.equal(ra.r_tilde, rb.r_tilde)


def test_world_size_above_one_is_refused(data):
    from pfml.parallel import dist as pdist
    _, chars, barra, wealth, rf = data
    old = pdist._ENV
    pdist.set_env(pdist.DistEnv(rank=0, world_size=2))
    try:
        with pytest.raises(RuntimeError, match="world size 1"):
            frontier.efficient_frontier(_cfg(data, False), chars, barra, wealth, rf, "cpu",
                                        wealth_vec=[1e10], gamma_vec=[10.0])
    finally:
        pdist.set_env(old)


def test_checkpoint_resumes_at_the_first_missing_point(data, ef_corrected, tmp_path,
                                                       monkeypatch):
    _, chars, barra, wealth, rf = data
    cfg = _cfg(data, False)
    ck = str(tmp_path / "points.json")
    real = frontier.run_point
    calls = []

    def failing(cfg_pt, *a, **k):
        if len(calls) == 1:
            raise KeyboardInterrupt("interrupted after point 1")
        calls.append((cfg_pt.pf_set["wealth"], cfg_pt.pf_set["gamma_rel"]))
        return real(cfg_pt, *a, **k)

    monkeypatch.setattr(frontier, "run_point", failing)
    kw = dict(wealth_vec=[1e10], gamma_vec=G_VEC, checkpoint=ck, checkpoint_key="k1")
    with pytest.raises(KeyboardInterrupt):
        frontier.efficient_frontier(cfg, chars, barra, wealth, rf, "cpu", **kw)
    assert calls == [(1e10, 10.0)]

    def counting(cfg_pt, *a, **k):
        calls.append((cfg_pt.pf_set["wealth"], cfg_pt.pf_set["gamma_rel"]))
        return real(cfg_pt, *a, **k)

    monkeypatch.setattr(frontier, "run_point", counting)
    out = frontier.efficient_frontier(cfg, chars, barra, wealth, rf, "cpu", **kw)
    assert calls == [(1e10, 10.0), (1e10, 20.0)]            # point 1 was not run again
    ref = ef_corrected["ef"][ef_corrected["ef"]["wealth_end"] == 1e10].reset_index(drop=True)
    num = [c for c in ref.columns if c not in ("type", "s4_fallbacks", "seconds")]
    assert np.array_equal(out["ef"][num].to_numpy(float), ref[num].to_numpy(float))
    rp = ef_corrected["pf"][ef_corrected["pf"]["wealth_end"] == 1e10].reset_index(drop=True)
    assert np.array_equal(out["pf"][STAT].to_numpy(), rp[STAT].to_numpy())
    assert list(pd.to_datetime(out["pf"]["eom_ret"])) == list(pd.to_datetime(rp["eom_ret"]))
    # another key (changed settings) does not reuse the points
    calls.clear()
    frontier.efficient_frontier(cfg, chars, barra, wealth, rf, "cpu", wealth_vec=[1e10],
                                gamma_vec=[10.0], checkpoint=ck, checkpoint_key="k2")
    assert calls == [(1e10, 10.0)]


def test_failing_point_is_reported_nan_and_the_rest_runs(data, monkeypatch):
    _, chars, barra, wealth, rf = data
    real = frontier.run_point

    def flaky(cfg_pt, *a, **k):
        if cfg_pt.pf_set["gamma_rel"] == 10.0:
            raise FloatingPointError("PFML inputs stay non-finite")
        return real(cfg_pt, *a, **k)

    monkeypatch.setattr(frontier, "run_point", flaky)
    out = frontier.efficient_frontier(_cfg(data, False), chars, barra, wealth, rf, "cpu",
                                      wealth_vec=[1e10], gamma_vec=G_VEC)
    ef = out["ef"]
    assert len(ef) == 2 and np.isnan(ef.loc[0, "r"]) and np.isfinite(ef.loc[1, "r"])
    assert "non-finite" in ef.loc[0, "s4_fallbacks"]
    assert set(out["pf"]["gamma_rel"]) == {20.0}


def test_stage_registration():
    from pfml.pipeline import _DEPS, ALL_STAGES, MAIN_STAGES
    assert ALL_STAGES[-1] == "pfml-ef" and "pfml-ef" not in MAIN_STAGES
    need = {"ef", "mu", "lb_hor"}
    for st in ("pfml-input", "pfml-search-coef", "pfml-hp-reals", "pfml-best-hps"):
        need |= set(_DEPS[st])
    assert need <= set(_DEPS["pfml-ef"])


def test_pf_stats_torch_path_follows_pandas_nan_rules():
    from pfml.ops.pfstats import pf_stats
    rng = np.random.default_rng(0)
    B, N = 4, 9
    w, ws, ret = (rng.standard_normal((B, N)) for _ in range(3))
    lam = rng.uniform(1e-9, 1e-8, (B, N))
    n_rows = np.array([9, 5, 0, 7])
    w[0, 2] = np.nan                       # a missing aim
    lam[0, 4] = np.nan                     # skipped in tc only
    ret[1, 1] = np.nan                     # skipped in r only
    w[3, :] = np.nan                       # no finite term at all
    w[1, 5:], ws[1, 5:], ret[1, 5:], lam[1, 5:] = np.nan, 1e300, 1e300, np.nan   # padding
    wealth = np.array([1e10, 2e10, 3e10, 4e10])
    got = pf_stats(*(torch.as_tensor(x) for x in (w, ws, ret, lam)),
                   torch.as_tensor(n_rows), torch.as_tensor(wealth)).numpy()
    eom = month_end(np.arange(B) + 2000 * 12)
    rows = [(b, j) for b in range(B) for j in range(n_rows[b])]
    bi, ji = (np.asarray(x, np.int64) for x in zip(*rows))
    weights = pd.DataFrame({"id": ji, "eom": eom[bi], "w": w[bi, ji], "w_start": ws[bi, ji]})
    chars = pd.DataFrame({"id": ji, "eom": eom[bi], "ret_ld1": ret[bi, ji],
                          "lambda": lam[bi, ji]})
    ref = portfolio.pf_ts(weights, chars, pd.DataFrame({"eom": eom, "wealth": wealth}))
    live = [0, 1, 3]
    assert np.allclose(got[live], ref[STAT].to_numpy(), rtol=1e-13, atol=0)
    assert np.array_equal(got[2], np.zeros(5))            # no row
    assert np.array_equal(got[3], np.zeros(5))            # all-NaN weights
    assert np.isfinite(got).all()
