"""The benchmark portfolios on the device: ``benchmark_portfolios`` against the CPU run of the
same call (the tolerance test_gpu_importance.py applies to that comparison), the Portfolio-ML
row against ``portfolio.backtest_device``, and the ``pfml-bmk`` stage end to end through
``Pipeline.run``."""
import os
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

STAT = ["inv", "shorting", "turnover", "r", "tc"]
YEARS = ["pf.dates.start_year=2008", "pf.dates.end_yr=2012", "pf.dates.split_years=1",
         "pf_ml.p_vec=[16,32]"]
STATIC = ["bmk.static.k=[1,0.5]", "bmk.static.u=[1,0.5]", "bmk.static.g=[0,2]"]
TOL = dict(rtol=1e-8, atol=1e-12)      # device against CPU, as test_gpu_importance.py


def _load(cfg):
    from pfml.config import get_features
    from pfml.data import io
    from pfml.models.risk import BarraCov
    d = cfg.run.data_dir
    return (io.read_processed_chars(d, get_features()),
            BarraCov.load(os.path.join(d, "Barra_Cov.npz")),
            pd.read_csv(os.path.join(d, "wealth_processed.csv"), parse_dates=["eom"]),
            io.read_risk_free(d))


@pytest.fixture(scope="module")
def case(small_data):
    cfg = small_data.override(YEARS + STATIC)
    cfg.run.compat_mode = False
    return dict(cfg=cfg, data=_load(cfg))


@pytest.fixture(scope="module")
def device_run(case):
    from pfml.models import benchmarks
    return benchmarks.benchmark_portfolios(case["cfg"], *case["data"], torch.device("cuda", 0),
                                           keep_weights=True)


def test_device_matches_the_cpu_run(case, device_run):
    from pfml.models import benchmarks, frontier
    cpu = benchmarks.benchmark_portfolios(case["cfg"], *case["data"], "cpu", keep_weights=True)
    dev = device_run
    for c in ("type", "n", "reason"):
        assert list(dev["bmk"][c]) == list(cpu["bmk"][c]), c
    assert len(dev["bmk"]) == 2 + 8 + 2 and (dev["bmk"]["reason"] == "").all()
    assert dev["chosen"] == cpu["chosen"] and dev["chosen_bmk"] == cpu["chosen_bmk"]
    assert dev["missing_mu"] == cpu["missing_mu"] == 0
    print("max |device - cpu| of mu_hat:", float(np.abs(dev["mu_hat"] - cpu["mu_hat"]).max()))
    assert np.allclose(dev["mu_hat"], cpu["mu_hat"], **TOL)
    num = [c for c in frontier.SUMMARY_COLUMNS if c not in ("type", "n")]
    err = np.abs(dev["pf"][STAT].to_numpy() - cpu["pf"][STAT].to_numpy())
    print("max |device - cpu| of the monthly statistics:", float(err.max()))
    assert list(dev["pf"]["type"]) == list(cpu["pf"]["type"])
    assert np.allclose(dev["pf"][STAT].to_numpy(), cpu["pf"][STAT].to_numpy(), **TOL)
    assert np.allclose(dev["bmk"][num].to_numpy(float), cpu["bmk"][num].to_numpy(float), **TOL)
    assert np.allclose(dev["hps"]["val_mse"], cpu["hps"]["val_mse"], **TOL)
    for name, w in dev["weights"].items():
        ref = cpu["weights"][name]
        assert np.allclose(w["w"], ref["w"], equal_nan=True, **TOL), name
    assert dev["bmk"]["obj"].nunique() == len(dev["bmk"])


def test_regular_panel_runs_every_arm_on_the_kernels(gpu, tmp_path):
    """The 40-stock engine panel (no degenerate idiosyncratic variance): Markowitz-ML and the
    normalised Minimum variance go through factor_prepare + factor_chain on the device like the
    Static-ML arms - nothing takes the dense route - and match the CPU run of the same call."""
    from pfml.config import Config
    from pfml.data.synthetic import engine_inputs
    from pfml.models import benchmarks, frontier
    cfg = Config.default().override(["pf_ml.p_vec=[8,16]", "pf.dates.start_year=2001",
                                     "pf.dates.end_yr=2004", "pf.dates.split_years=1",
                                     "split.test_end=2004-12-31", f"run.data_dir={tmp_path}"]
                                    + STATIC)
    cfg.run.compat_mode = False
    inputs = engine_inputs(n_stocks=40, start="1993-01-31", end="2004-12-31")
    dense, chain = [], []
    real_d, real_s = benchmarks._dense_arms, benchmarks._solve_arms
    benchmarks._dense_arms = lambda ops, arms, dev: (dense.append(arms),
                                                     real_d(ops, arms, dev))[1]
    benchmarks._solve_arms = lambda ops, arms, dev: (chain.append((len(arms), str(dev))),
                                                     real_s(ops, arms, dev))[1]
    try:
        dev = benchmarks.benchmark_portfolios(cfg, *inputs, gpu, keep_weights=True)
    finally:
        benchmarks._dense_arms, benchmarks._solve_arms = real_d, real_s
    cpu = benchmarks.benchmark_portfolios(cfg, *inputs, "cpu", keep_weights=True)
    assert dense == [] and len(chain) == 1 and chain[0][0] == 10 and "cuda" in chain[0][1]
    assert (dev["bmk"]["reason"] == "").all()
    assert list(dev["bmk"]["type"]) == list(cpu["bmk"]["type"])
    assert dev["chosen_bmk"] == cpu["chosen_bmk"]
    num = [c for c in frontier.SUMMARY_COLUMNS if c not in ("type", "n")]
    assert np.allclose(dev["pf"][STAT].to_numpy(), cpu["pf"][STAT].to_numpy(), **TOL)
    assert np.allclose(dev["bmk"][num].to_numpy(float), cpu["bmk"][num].to_numpy(float), **TOL)
    for name in ("Markowitz-ML", "Minimum variance", "Static-ML"):
        assert np.allclose(dev["weights"][name]["w"], cpu["weights"][name]["w"], **TOL), name
    mv = dev["weights"]["Minimum variance"].groupby("eom")["w"].sum()
    assert np.allclose(mv.to_numpy(), 1.0, rtol=0, atol=1e-13)


def test_portfolio_ml_row_is_backtest_device(gpu, case, device_run):
    """The Portfolio-ML row is the point's own ``backtest_device`` (a second S4 run of the
    same point: the engine's device results are run-to-run bitwise)."""
    from pfml.models import frontier
    from pfml.utils.dates import pfml_date_grids
    cfg = case["cfg"]
    chars, barra, wealth, rf = case["data"]
    s = cfg.settings
    grids = pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                            s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                            s["pf"]["dates"]["split_years"])
    bt = frontier.run_point(cfg, chars, barra, wealth, rf, gpu, grids, {})
    mine = device_run["pf"][device_run["pf"]["type"] == "Portfolio-ML"]
    assert np.array_equal(mine[STAT].to_numpy(), bt["pf"][STAT].to_numpy())
    assert device_run["chosen"] == bt["chosen"]


def test_stage_end_to_end(gpu, small_data, device_run, tmp_path):
    from pfml.data.io import CSV_COLUMNS
    from pfml.pipeline import Pipeline
    d = str(tmp_path / "data_bmk")
    shutil.copytree(small_data.run.data_dir, d)
    cfg = small_data.override(YEARS + STATIC + ["run.plots=False", f"run.data_dir={d}",
                                                f"run.artifact_dir={tmp_path}/art"])
    cfg.run.compat_mode = False
    Pipeline(cfg, device=gpu.type).run(["pfml-bmk"])
    bmk = pd.read_csv(os.path.join(d, "bmk.csv"), keep_default_na=False,
                      na_values=["nan", "NaN"])
    pf = pd.read_csv(os.path.join(d, "bmk_pf.csv"), parse_dates=["eom_ret"])
    hps = pd.read_csv(os.path.join(d, "bmk_hps.csv"))
    assert list(bmk.columns) == CSV_COLUMNS["bmk.csv"]
    assert list(pf.columns) == CSV_COLUMNS["bmk_pf.csv"]
    assert list(hps.columns) == CSV_COLUMNS["bmk_hps.csv"]
    ref = device_run["bmk"]
    assert list(bmk["type"]) == list(ref["type"])
    assert len(pf) == len(bmk) * len(device_run["months"])
    num = ["r", "sd", "tc", "r_tc", "sr", "obj"]
    assert np.isfinite(bmk[num].to_numpy(float)).all()
    assert np.allclose(bmk[num].to_numpy(float), ref[num].to_numpy(float), **TOL)
    assert np.allclose(hps["val_mse"], device_run["hps"]["val_mse"], **TOL)
