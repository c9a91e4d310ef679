"""Feature-theme importance on the device: ``feature_importance`` against the CPU run of the
same call, the benchmark arm bitwise ``portfolio.backtest_device`` on the same grid and
inputs, and the ``pfml-fi`` stage end to end through ``Pipeline.run``."""
import os
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

STAT = ["inv", "shorting", "turnover", "r", "tc"]
# four OOS years on the session's small panel, and a p grid that keeps the CPU run of the same
# call at a fraction of a second; the selection picks both g over these years (two distinct W
# in corrected mode)
YEARS = ["pf.dates.start_year=2008", "pf.dates.end_yr=2012", "pf.dates.split_years=1",
         "pf_ml.p_vec=[16,32]"]
TOL = dict(rtol=1e-8, atol=1e-12)      # device against CPU, as test_gpu_frontier.py


def _load(cfg):
    from pfml.config import get_features
    from pfml.data import io
    from pfml.models.risk import BarraCov
    d = cfg.run.data_dir
    return (io.read_processed_chars(d, get_features()),
            BarraCov.load(os.path.join(d, "Barra_Cov.npz")),
            pd.read_csv(os.path.join(d, "wealth_processed.csv"), parse_dates=["eom"]),
            io.read_risk_free(d),
            pd.read_csv(os.path.join(d, "cluster_labels_processed.csv")))


def _grids(cfg, barra):
    from pfml.utils.dates import pfml_date_grids
    s = cfg.settings
    return pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                           s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                           s["pf"]["dates"]["split_years"])


@pytest.fixture(scope="module")
def case(small_data):
    """The small panel in corrected mode (the two g have their own W), its themes, and the
    benchmark point's S4 / grid / layout on the device, computed once."""
    from pfml.models import frontier, importance
    gpu = torch.device("cuda", 0)
    cfg = small_data.override(YEARS)
    cfg.run.compat_mode = False
    chars, barra, wealth, rf, labels = _load(cfg)
    themes = importance.theme_columns(labels)
    assert len(themes) >= 3
    pick = sorted([themes[0][0], themes[len(themes) // 2][0], themes[-1][0]])
    ctx = {}
    pt = frontier.point_inputs(cfg, chars, barra, wealth, rf, gpu, _grids(cfg, barra), ctx)
    return dict(cfg=cfg, data=(chars, barra, wealth, rf), labels=labels, themes=themes, pt=pt,
                layout=ctx["layout"], pick=pick)


@pytest.fixture(scope="module")
def device_run(case):
    """feature_importance on the device from the case's own point (point_inputs handed over,
    so the grid and the inputs are the very tensors backtest_device gets below)."""
    from pfml.models import frontier, importance
    gpu = torch.device("cuda", 0)

    def handed(cfg_pt, chars, barra, wealth_pt, risk_free, device, grids, ctx, clock=None):
        ctx["layout"] = case["layout"]
        return case["pt"]

    real = frontier.point_inputs
    frontier.point_inputs = handed
    try:
        return importance.feature_importance(case["cfg"], *case["data"], case["labels"], gpu,
                                             n_draws=2, seed=3, clusters=case["pick"],
                                             keep_weights=True)
    finally:
        frontier.point_inputs = real


def test_device_matches_the_cpu_run(case, device_run):
    from pfml.models import frontier, importance
    cpu = importance.feature_importance(case["cfg"], *case["data"], case["labels"], "cpu",
                                        n_draws=2, seed=3, clusters=case["pick"])
    dev = device_run
    A = 1 + 2 * len(case["pick"])
    assert len(dev["fi"]) == len(cpu["fi"]) == A
    for c in ("cluster", "draw", "n_features", "type", "n", "reason"):
        assert list(dev["fi"][c]) == list(cpu["fi"][c]), c
    assert dev["chosen"] == cpu["chosen"]
    assert len({g for g, _, _ in dev["chosen"].values()}) == 2        # both W blocks in play
    assert (dev["fi"]["reason"] == "").all()
    num = [c for c in frontier.SUMMARY_COLUMNS if c not in ("type", "n")]
    err = np.abs(dev["stats"] - cpu["stats"])
    print("max |device - cpu| of the monthly statistics:", float(err.max()))
    assert np.allclose(dev["stats"], cpu["stats"], **TOL)
    assert np.allclose(dev["fi"][num].to_numpy(float), cpu["fi"][num].to_numpy(float), **TOL)
    assert list(dev["pf"]["cluster"]) == list(cpu["pf"]["cluster"])
    assert np.allclose(dev["pf"][STAT].to_numpy(), cpu["pf"][STAT].to_numpy(), **TOL)
    # the arms are counterfactuals: every one differs from bm
    assert dev["fi"]["obj"].nunique() == A


def test_bm_arm_is_bitwise_backtest_device(gpu, case, device_run):
    """The multi chain's column 0 and the [(A B), N] statistics launch reproduce the single
    chain and the [B, N] launch: np.array_equal on the [B, 5] statistics, the weights too."""
    from pfml.models import portfolio
    chars, barra, wealth, rf = case["data"]
    bt = portfolio.backtest_device(case["cfg"], case["pt"]["grid"], case["pt"]["res"],
                                   case["layout"], wealth, gpu, keep_weights=True)
    assert not bt["recomputed"]
    assert np.array_equal(device_run["stats"][0], bt["stats"])
    assert device_run["chosen"] == bt["chosen"]
    w = device_run["weights"][("bm", 0)]
    for c in ("w_start", "w"):
        assert np.array_equal(w[c].to_numpy(), bt["weights"][c].to_numpy(), equal_nan=True), c
    bm = device_run["pf"][device_run["pf"]["cluster"] == "bm"]
    assert np.array_equal(bm[STAT].to_numpy(), bt["pf"][STAT].to_numpy())


def test_stage_end_to_end(gpu, small_data, case, device_run, tmp_path):
    """``Pipeline.run(["pfml-fi"])`` with every theme of the labels and one draw: both CSVs with
    the stated columns, one row per (cluster, draw) plus bm, finite, the monthly frame one
    block per arm; the rows of the three themes of ``device_run`` equal its draw 0 (common
    random numbers: a theme's draw does not depend on the other themes)."""
    from pfml.data.io import CSV_COLUMNS
    from pfml.pipeline import Pipeline
    d = str(tmp_path / "data_fi")
    shutil.copytree(small_data.run.data_dir, d)
    cfg = small_data.override(YEARS + ["fi.n_draws=1", "fi.seed=3", "run.plots=False",
                                       f"run.data_dir={d}", f"run.artifact_dir={tmp_path}/art"])
    cfg.run.compat_mode = False
    Pipeline(cfg, device=gpu.type).run(["pfml-fi"])
    fi = pd.read_csv(os.path.join(d, "fi.csv"), keep_default_na=False, na_values=["nan", "NaN"])
    pf = pd.read_csv(os.path.join(d, "fi_pf.csv"), parse_dates=["eom_ret"])
    assert list(fi.columns) == CSV_COLUMNS["fi.csv"]
    assert list(pf.columns) == CSV_COLUMNS["fi_pf.csv"]
    names = [t[0] for t in case["themes"]]
    assert [tuple(x) for x in fi[["cluster", "draw"]].to_numpy()] == \
        [("bm", 0)] + [(c, 0) for c in names]
    B = case["layout"]["B"]
    assert len(pf) == len(fi) * B and (fi["n"] == B).all()
    assert np.isfinite(fi[["r", "sd", "sr", "obj", "obj_drop"]].to_numpy(float)).all()
    assert fi["obj_drop"].iloc[0] == 0.0
    # the stage computed what the direct call computes (same seed, same draws; its own S4 run)
    ref = device_run["fi"]
    ref = ref[ref["draw"] == 0]
    got = fi[fi["cluster"].isin(list(ref["cluster"]))]
    assert list(got["cluster"]) == list(ref["cluster"]) == ["bm"] + case["pick"]
    num = ["r", "sd", "tc", "r_tc", "sr", "obj"]
    assert np.allclose(got[num].to_numpy(float), ref[num].to_numpy(float), **TOL)
