"""Feature-theme importance on the CPU path: every arm against an independent oracle (a panel
whose theme columns are permuted with pandas, taken through the EXISTING stage functions with
the benchmark's validation frame and coefficients), the identity / empty-theme / seed rules,
the torch path of ``_chain_multi``, the stage registration and the failure isolation."""
import copy

import numpy as np
import pandas as pd
import pytest
import torch

import oracle as orc
from pfml.config import Config, get_features
from pfml.data.io import CSV_COLUMNS
from pfml.models import frontier, importance, portfolio, search
from pfml.models import pfml_inputs as pin
from pfml.utils.dates import month_end, month_index, pfml_date_grids

STAT = ["inv", "shorting", "turnover", "r", "tc"]
NUM = [c for c in frontier.SUMMARY_COLUMNS if c != "type"]
TOL = dict(rtol=1e-10, atol=1e-12)          # the fp64 CPU paths against the goldens
SEED = 11


def _grids(cfg, barra):
    s = cfg.settings
    return pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                           s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                           s["pf"]["dates"]["split_years"])


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The 40-stock inputs of test_frontier_cpu.py: three OOS years (Dec 2001 .. Nov 2004),
    p_vec = [8, 16]; compat mode reads rff_w.csv."""
    from pfml.data.synthetic import engine_inputs
    d = str(tmp_path_factory.mktemp("fi_cpu"))
    cfg = Config.default().override(["pf_ml.p_vec=[8,16]", "pf.dates.start_year=2001",
                                     "pf.dates.end_yr=2004", "pf.dates.split_years=1",
                                     "split.test_end=2004-12-31", f"run.data_dir={d}"])
    rng = np.random.default_rng(5)
    pd.DataFrame(rng.standard_normal((len(get_features()), cfg.p_max // 2))).to_csv(
        f"{d}/rff_w.csv")
    return (cfg,) + engine_inputs(n_stocks=40, start="1993-01-31", end="2004-12-31")


@pytest.fixture(scope="module")
def labels():
    """Three themes over the features (sizes 5, 40 and the rest) and a fourth cluster whose
    only member is not a feature (skipped)."""
    f = get_features()
    rows = [(c, 1, "value") for c in f[:5]] + [(c, -1, "momentum") for c in f[5:45]] + \
        [(c, 1, "quality") for c in f[45:]] + [("not_a_feature", 1, "zzz")]
    return pd.DataFrame(rows, columns=["characteristic", "direction", "cluster"])


def _cfg(data, compat):
    cfg = copy.deepcopy(data[0])
    cfg.run.compat_mode = compat
    return cfg


@pytest.fixture(scope="module")
def bench(data):
    """Per mode: the benchmark through the existing functions (``_plain_point`` of
    test_frontier_cpu.py), keeping what the arms' oracle reuses."""
    out = {}
    _, chars, barra, wealth, rf = data
    for compat in (False, True):
        cfg = _cfg(data, compat)
        g = _grids(cfg, barra)
        m2, oos = g["m2"], g["oos"]
        res = pin.build_inputs(cfg, chars, barra, wealth, rf, "cpu", months=m2, keep_m=oos)
        R = search.complete_local_reals(res.reals.r_tilde, res.reals.denom, m2, cfg.hp_years)
        grid = search.grid_search(R, cfg)
        val = search.validation_frame(grid, cfg)
        years_b, beta_b = search.gather_beta(grid)
        out[compat] = dict(cfg=cfg, m2=m2, oos=oos, res=res, val=val, years_b=years_b,
                           beta_b=beta_b, npad=pin.universe_npad(chars, m2))
        out[compat]["pf"], out[compat]["summ"] = _backtest(out[compat], data, res.signal_t,
                                                           res.ids, m2)
    return out


def _backtest(b, data, signal_t, signal_ids, signal_months):
    """aim_portfolios (the BENCHMARK's validation frame and betas) -> best_hps ->
    pfml_weights -> pf_ts / pf_summary, as ``_plain_point`` does."""
    _, chars, barra, wealth, rf = data
    cfg, oos = b["cfg"], b["oos"]
    aims = portfolio.aim_portfolios(cfg, b["val"], b["years_b"], b["beta_b"], signal_months,
                                    signal_t, signal_ids, oos)
    hps = portfolio.hps_bundle(aims, b["val"], b["res"].rff_w)
    _, _, aim_df = portfolio.best_hps(hps, oos)
    w = portfolio.pfml_weights(cfg, chars, barra, wealth, rf, aim_df, oos, "cpu",
                               m_cache=b["res"].m_keep, n_pad=b["npad"])
    pf = portfolio.pf_ts(w, chars, wealth, compat=cfg.run.compat_mode)
    return pf, portfolio.pf_summary(pf, float(cfg.pf_set["gamma_rel"]))


def _permuted_chars(chars, cols, oos, universes, perms):
    """pandas: in every OOS month, stock i of the month's universe (id order) takes the
    theme columns of stock pi(i) of the same month."""
    out = chars.copy()
    mi = month_index(out["eom"])
    vals = out[cols].to_numpy(np.float64, copy=True)
    ids = out["id"].to_numpy(np.int64)
    for d, uni, pi in zip(oos, universes, perms):
        at = np.nonzero(mi == int(d))[0]
        pos = {int(i): r for r, i in zip(at, ids[at])}
        rows = np.asarray([pos[int(i)] for i in uni], np.int64)
        vals[rows] = out[cols].to_numpy(np.float64)[rows[np.asarray(pi)]]
    out[cols] = vals
    return out


def _fi(data, labels, compat, **kw):
    _, chars, barra, wealth, rf = data
    kw.setdefault("seed", SEED)
    return importance.feature_importance(_cfg(data, compat), chars, barra, wealth, rf, labels,
                                         "cpu", **kw)


@pytest.fixture(scope="module")
def fi_runs(data, labels):
    return {compat: _fi(data, labels, compat, n_draws=2, keep_weights=True)
            for compat in (False, True)}


def _arm(out, cluster, draw):
    fi, pf = out["fi"], out["pf"]
    row = fi[(fi["cluster"] == cluster) & (fi["draw"] == draw)]
    assert len(row) == 1
    return row.iloc[0], pf[(pf["cluster"] == cluster) & (pf["draw"] == draw)]


def test_frames_shape_columns_order(fi_runs):
    for out in fi_runs.values():
        fi, pf = out["fi"], out["pf"]
        assert list(fi.columns) == CSV_COLUMNS["fi.csv"] == importance.FI_COLUMNS
        assert list(pf.columns) == CSV_COLUMNS["fi_pf.csv"] == importance.FI_PF_COLUMNS
        assert [tuple(x) for x in fi[["cluster", "draw", "n_features"]].to_numpy()] == \
            [("bm", 0, 0)] + [(c, d, n) for d in (0, 1)
                              for c, n in (("momentum", 40), ("quality", len(get_features()) - 45),
                                           ("value", 5))]
        assert len(pf) == 7 * 36 and (fi["n"] == 36).all()
        assert np.isfinite(fi[NUM + ["obj_drop"]].to_numpy(float)).all()
        assert fi["obj_drop"].iloc[0] == 0.0 and (fi["reason"] == "").all()
        assert np.array_equal(fi["obj_drop"].to_numpy(), fi["obj"].iloc[0] - fi["obj"].to_numpy())
        assert fi["obj"].nunique() == 7                       # every arm differs


@pytest.mark.parametrize("compat", [False, True])
def test_benchmark_row_is_the_plain_point(bench, fi_runs, compat):
    row, pf = _arm(fi_runs[compat], "bm", 0)
    ref_pf, summ = bench[compat]["pf"], bench[compat]["summ"]
    assert list(pd.to_datetime(pf["eom_ret"])) == list(pd.to_datetime(ref_pf["eom_ret"]))
    assert np.allclose(pf[STAT].to_numpy(), ref_pf[STAT].to_numpy(), **TOL)
    assert row["type"] == summ["type"].iloc[0]
    assert np.allclose(row[NUM].to_numpy(float), summ[NUM].to_numpy(float)[0], **TOL)


@pytest.mark.parametrize("compat,cluster", [(False, "momentum"), (True, "value")])
def test_arms_equal_the_independent_oracle(data, labels, bench, fi_runs, compat, cluster):
    """Two themes x two draws (momentum in corrected mode, where the two g have their own W;
    value in compat mode): permuted panel -> build_inputs' signal_t -> the existing functions."""
    _, chars, barra, wealth, rf = data
    b = bench[compat]
    oos = b["oos"]
    pos = np.searchsorted(b["m2"], oos)
    universes = [b["res"].ids[p] for p in pos]
    cols = list(labels.loc[labels["cluster"] == cluster, "characteristic"])
    for draw in (0, 1):
        perms = importance.month_permutations(SEED, draw, [len(u) for u in universes])
        cf = _permuted_chars(chars, cols, oos, universes, perms)
        res = pin.build_inputs(b["cfg"], cf, barra, wealth, rf, "cpu", months=oos)
        assert all(np.array_equal(x, y) for x, y in zip(res.ids, universes))
        ref_pf, summ = _backtest(b, data, res.signal_t, res.ids, oos)
        row, pf = _arm(fi_runs[compat], cluster, draw)
        assert list(pd.to_datetime(pf["eom_ret"])) == list(pd.to_datetime(ref_pf["eom_ret"]))
        err = np.abs(pf[STAT].to_numpy() - ref_pf[STAT].to_numpy())
        print(f"{cluster}/{draw} compat={compat}: max abs err of the monthly stats {err.max():.3e}")
        assert np.allclose(pf[STAT].to_numpy(), ref_pf[STAT].to_numpy(), **TOL)
        assert np.allclose(row[NUM].to_numpy(float), summ[NUM].to_numpy(float)[0], **TOL)
        bm = fi_runs[compat]["fi"].iloc[0]
        assert np.isclose(row["obj_drop"], bm["obj"] - summ["obj"].iloc[0], **TOL)


def test_identity_permutation_and_empty_theme_are_bitwise_bm(data, labels, monkeypatch):
    """The identity permutation goes through the whole counterfactual path (gather, RFF,
    standardisation, aims) and lands on the benchmark's bits; so does a theme without a
    column."""
    f = get_features()
    themes = {"empty": [], "some": f[5:45]}
    out = _fi(data, None, False, n_draws=1, clusters=themes, keep_weights=True)
    assert list(out["fi"]["cluster"]) == ["bm", "empty", "some"]
    assert list(out["fi"]["n_features"]) == [0, 0, 40]
    assert np.array_equal(out["aims"][1], out["aims"][0], equal_nan=True)
    assert np.array_equal(out["stats"][1], out["stats"][0])
    assert not np.array_equal(out["stats"][2], out["stats"][0])
    fi = out["fi"]
    assert fi.loc[1, NUM].to_numpy(float).tolist() == fi.loc[0, NUM].to_numpy(float).tolist()
    assert fi.loc[1, "obj_drop"] == 0.0
    # a real permutation moves the aims of every month with at least two stocks
    # (every month of this panel has)
    assert min(len(u) for u in out["weights"][("bm", 0)].groupby("eom")["id"].apply(list)) >= 2
    moved = (out["aims"][2] != out["aims"][0]).any(1)
    assert moved.all() and len(moved) == 36
    monkeypatch.setattr(importance, "month_permutations",
                        lambda seed, draw, ns: [np.arange(int(n)) for n in ns])
    ident = _fi(data, None, False, n_draws=1, clusters={"some": f[5:45]}, keep_weights=True)
    assert np.array_equal(ident["aims"][1], ident["aims"][0], equal_nan=True)
    assert np.array_equal(ident["stats"][1], ident["stats"][0])
    assert np.array_equal(ident["stats"][0], out["stats"][0])


def test_seed_and_draw_rules(data, labels, fi_runs):
    """The same seed reproduces the frame bitwise, another seed changes the arm and not bm;
    the bm row and a (theme, draw) arm do not depend on n_draws or on the other themes (on the
    CPU the batched matmul's bits may move with the number of arms, hence the CPU tolerance;
    the device chain is bitwise, tests/test_gpu_importance.py); month_permutations is the
    documented generator."""
    ref = fi_runs[False]
    one = _fi(data, labels, False, n_draws=1, clusters=["value"])
    assert list(one["fi"]["cluster"]) == ["bm", "value"]
    num = NUM + ["obj_drop"]
    again = _fi(data, labels, False, n_draws=1, clusters=["value"])
    assert np.array_equal(one["fi"][num].to_numpy(float), again["fi"][num].to_numpy(float))
    assert np.array_equal(one["pf"][STAT].to_numpy(), again["pf"][STAT].to_numpy())
    assert np.allclose(one["fi"].loc[0, num].to_numpy(float),
                       ref["fi"].loc[0, num].to_numpy(float), **TOL)
    same = ref["fi"][(ref["fi"]["cluster"] == "value") & (ref["fi"]["draw"] == 0)]
    assert np.allclose(one["fi"].loc[1, num].to_numpy(float), same[num].to_numpy(float)[0], **TOL)
    other = _fi(data, labels, False, n_draws=1, clusters=["value"], seed=SEED + 1)
    assert np.array_equal(other["fi"].loc[0, num].to_numpy(float),
                          one["fi"].loc[0, num].to_numpy(float))
    assert other["fi"].loc[1, "obj"] != one["fi"].loc[1, "obj"]
    p = importance.month_permutations(3, 2, [5, 1, 7])
    rng = np.random.default_rng([3, 2])
    assert all(np.array_equal(a, rng.permutation(n)) for a, n in zip(p, (5, 1, 7)))


@pytest.mark.parametrize("A", [1, 3, 17])
def test_chain_multi_torch_path_columns(A):
    """Column k of the batched-matmul path is ``_chain`` on wa[k]: the drift bitwise and every
    month within the derived 2 (N + 4) u bound of the longdouble step (oracle.check_chain);
    against the single chain's own output the months' bounds add up: B 2 (N + 4) u mag with
    mag = |wa| + |a| sum |M| |d| < 1 for these operands (|M| ~ 1 / (2 sqrt N), |d| < 0.1)."""
    N, B = 37, 4
    ops = orc.chain_inputs(N, B, seed=5)
    rng = np.random.default_rng(A)
    wa = np.concatenate([ops[2][None], 0.01 * rng.standard_normal((A - 1, B, N))], 0)
    t = [torch.as_tensor(x) for x in ops]
    Wst, Wopt, ws = portfolio._chain_multi(t[0], t[1], torch.as_tensor(wa), *t[3:])
    assert Wst.shape == (A, B, N) and Wopt.shape == (A, B, N) and ws.shape == (A, N)
    for k in range(A):
        ops_k = (ops[0], ops[1], wa[k]) + tuple(ops[3:])
        assert orc.check_chain(ops_k, Wst[k].numpy(), Wopt[k].numpy(), ws[k].numpy()) < 1.0
        s = portfolio._chain(t[0], t[1], torch.as_tensor(wa[k]), *t[3:])
        for got, ref in zip((Wst[k], Wopt[k], ws[k]), s):
            assert np.allclose(got.numpy(), ref.numpy(), rtol=0, atol=B * 2 * (N + 4) * orc.U)
    # a ws0 per portfolio
    ws0 = 0.01 * rng.standard_normal((A, N))
    W2 = portfolio._chain_multi(t[0], t[1], torch.as_tensor(wa), *t[3:6], torch.as_tensor(ws0))
    assert np.array_equal(W2[0][:, 0].numpy(), ws0)


def test_stage_registration(data):
    from pfml.pipeline import _DEPS, ALL_STAGES, MAIN_STAGES, Pipeline
    assert ALL_STAGES[-1] == "pfml-ef"
    assert "pfml-fi" in ALL_STAGES and "pfml-fi" not in MAIN_STAGES
    assert set(_DEPS["pfml-fi"]) == (set(_DEPS["pfml-ef"]) - {"ef"}) | {"fi"}
    cfg = data[0]
    pipe = Pipeline(cfg, device="cpu")
    old_stages = [s for s in ALL_STAGES if s != "pfml-fi"]
    key, keys = "", {}
    for st in old_stages:
        key = key + "|" + cfg.hash(*_DEPS.get(st, ())) + st
        keys[st] = key
    assert pipe._keys["pfml-ef"] == keys["pfml-ef"]
    assert all(pipe._keys[st] == keys[st] for st in old_stages)
    assert pipe._keys["pfml-fi"] == keys["pfml-best-hps"] + "|" + cfg.hash(*_DEPS["pfml-fi"]) \
        + "pfml-fi"
    # the new settings section moves pfml-fi's key and no other
    other = Pipeline(cfg.override(["fi.n_draws=3"]), device="cpu")
    assert other._keys["pfml-fi"] != pipe._keys["pfml-fi"]
    assert all(other._keys[st] == keys[st] for st in old_stages)
    bare = copy.deepcopy(cfg)
    del bare.settings["fi"]
    assert bare.hash() == cfg.hash()
    assert cfg.settings["fi"] == {"n_draws": 1, "seed": None, "clusters": None}


def test_world_size_above_one_is_refused(data, labels):
    from pfml.parallel import dist as pdist
    from pfml.pipeline import Pipeline
    old = pdist._ENV
    pdist.set_env(pdist.DistEnv(rank=0, world_size=2))
    try:
        with pytest.raises(RuntimeError, match="world size 1"):
            _fi(data, labels, False)
        pipe = Pipeline.__new__(Pipeline)
        pipe.env = pdist.DistEnv(rank=0, world_size=2)
        with pytest.raises(RuntimeError, match="world size 1"):
            pipe._pfml_fi()
    finally:
        pdist.set_env(old)


def test_fault_injection_recomputes_the_arm(data, labels):
    """run.fault_inject = "pfml-fi" poisons one w_start of the last arm after the chain: the
    arm is recomputed (here by the same CPU recursion) and the frame is the clean run's."""
    from pfml.utils.log import COUNTERS
    clean = _fi(data, labels, False, n_draws=1, clusters=["value"])
    _, chars, barra, wealth, rf = data
    cfg = _cfg(data, False)
    cfg.run.fault_inject = "pfml-fi"
    n0 = COUNTERS.as_dict().get("pfml_fi.recomputed_arms", 0)
    out = importance.feature_importance(cfg, chars, barra, wealth, rf, labels, "cpu", n_draws=1,
                                        seed=SEED, clusters=["value"])
    assert COUNTERS.as_dict().get("pfml_fi.recomputed_arms", 0) == n0 + 1
    num = NUM + ["obj_drop"]
    assert (out["fi"]["reason"] == "").all()
    assert np.array_equal(out["fi"].loc[0, num].to_numpy(float),
                          clean["fi"].loc[0, num].to_numpy(float))
    assert np.allclose(out["fi"].loc[1, num].to_numpy(float),
                       clean["fi"].loc[1, num].to_numpy(float), **TOL)


def test_failing_arm_is_a_nan_row_and_the_rest_stands(data, labels, fi_runs, monkeypatch):
    """Arm 2 (quality, draw 0) non-finite on the first chain and on its CPU re-run: a NaN row
    with a reason; every other row, and the monthly frame of the others, unchanged."""
    real = importance._chain_arms
    calls = []

    def poisoned(mt_all, a_all, wa, layout, to=None):
        Wst, Wopt = real(mt_all, a_all, wa, layout, to)
        k = 2 if not calls else 0                   # the re-run holds the bad arm alone
        calls.append(tuple(wa.shape))
        Wst[k, 3, 0] = float("nan")
        return Wst, Wopt

    monkeypatch.setattr(importance, "_chain_arms", poisoned)
    out = _fi(data, labels, False, n_draws=2)
    assert len(calls) == 2 and calls[0][0] == 7 and calls[1][0] == 1
    fi, ref = out["fi"], fi_runs[False]["fi"]
    assert list(fi["cluster"]) == list(ref["cluster"]) and fi.loc[2, "cluster"] == "quality"
    assert np.isnan(fi.loc[2, NUM[1:] + ["obj_drop"]].to_numpy(float)).all()
    assert fi.loc[2, "n"] == 0 and "non-finite" in fi.loc[2, "reason"]
    keep = [k for k in range(7) if k != 2]
    num = NUM + ["obj_drop"]
    assert np.array_equal(fi.loc[keep, num].to_numpy(float), ref.loc[keep, num].to_numpy(float))
    assert (fi.loc[keep, "reason"] == "").all()
    rp = fi_runs[False]["pf"]
    rp = rp[~((rp["cluster"] == "quality") & (rp["draw"] == 0))].reset_index(drop=True)
    assert np.array_equal(out["pf"][STAT].to_numpy(), rp[STAT].to_numpy())
    assert list(out["pf"]["cluster"]) == list(rp["cluster"])
