"""The efficient-frontier stage on the device: the per-month statistics kernel
(csrc/pfstats.hip) against ``portfolio.pf_ts``, its bitwise independence of the launch shape,
``portfolio.backtest_device`` against the frame-based stage functions, and the ``pfml-ef``
stage end to end against per-point runs of the existing S4-S9 stages."""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT = ["inv", "shorting", "turnover", "r", "tc"]
YEARS = ["pf.dates.start_year=1999", "pf.dates.end_yr=2012", "pf.dates.split_years=3"]
S4_S9 = ["pfml-input", "pfml-search-coef", "pfml-hp-reals", "pfml-aim", "pfml-hps",
         "pfml-best-hps"]


# ---------------------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(N: int, B: int):
    """Random months in the [B, N] layout and their statistics by ``portfolio.pf_ts`` (the
    reference's form: frames, merge, groupby.sum), computed once per (N, B).  Returns the
    dense arrays, n_rows, wealth, the reference [B, 5] (0 for months pf_ts has no row for),
    sum |terms| per statistic [B, 5] and the months that must give exactly 0."""
    from pfml.models.portfolio import pf_ts
    from pfml.utils.dates import month_end
    rng = np.random.default_rng(1000 * N + B)
    w, ws, ret = (rng.standard_normal((B, N)) * 0.05 for _ in range(3))
    lam = rng.uniform(1e-9, 1e-7, (B, N))
    wealth = rng.uniform(1e8, 1e11, B)
    if B == 1:
        n_rows = np.array([N])
    else:
        n_rows = np.array([N, 0, N // 2, min(1, N), N - 1, N, int(rng.integers(0, N + 1))])
    if N > 1:
        w[rng.random((B, N)) < 0.05] = np.nan              # missing aims
        lam[rng.random((B, N)) < 0.05] = np.nan
        ret[rng.random((B, N)) < 0.02] = np.nan
    zero = [b for b in range(B) if n_rows[b] == 0]
    if B > 1:
        w[5, :] = np.nan                                   # a month of missing aims only
        zero.append(5)
    eom = month_end(np.arange(B) + 2000 * 12)
    rows = [(b, j) for b in range(B) for j in range(n_rows[b])]
    bi, ji = (np.asarray(x, np.int64) for x in zip(*rows))
    weights = pd.DataFrame({"id": ji, "eom": eom[bi], "w": w[bi, ji], "w_start": ws[bi, ji]})
    chars = pd.DataFrame({"id": ji, "eom": eom[bi], "ret_ld1": ret[bi, ji],
                          "lambda": lam[bi, ji]})
    got = pf_ts(weights, chars, pd.DataFrame({"eom": eom, "wealth": wealth}))
    ref = np.zeros((B, 5))
    pos = {pd.Timestamp(e): b for b, e in enumerate(eom)}
    for _, r in got.iterrows():
        ref[pos[pd.Timestamp(r["eom_ret"])]] = r[STAT].to_numpy(float)
    dw = w - ws
    terms = np.stack([np.abs(w), np.abs(np.minimum(w, 0)), np.abs(dw), w * ret, lam * dw * dw], 1)
    live = np.arange(N)[None, :] < n_rows[:, None]
    mag = np.where(live[:, None, :] & ~np.isnan(terms), np.abs(terms), 0.0).sum(-1)
    mag[:, 4] *= wealth / 2
    return w, ws, ret, lam, n_rows, wealth, ref, mag, zero


def _padded(x, pad, fill, dev):
    """x [B, N] as the first N columns of a [B, N + pad] device buffer filled with ``fill``."""
    B, N = x.shape
    buf = torch.full((B, N + pad), fill, dtype=torch.float64, device=dev)
    buf[:, :N] = torch.as_tensor(x, device=dev)
    return buf


def _launch(case, pad, dev, order=None):
    """pf_stats on the case's months (``order``: a selection / permutation of them), with
    everything beyond n_rows overwritten by NaN (w, lam) and 1e300 (w_start, ret)."""
    from pfml.ops.pfstats import pf_stats
    w, ws, ret, lam, n_rows, wealth = case[:6]
    order = np.arange(len(n_rows)) if order is None else np.asarray(order)
    dead = np.arange(w.shape[1])[None, :] >= n_rows[order][:, None]
    ops = []
    for x, fill in ((w, np.nan), (ws, 1e300), (ret, 1e300), (lam, np.nan)):
        ops.append(_padded(np.where(dead, fill, x[order]), pad, fill, dev))
    return pf_stats(*ops, torch.as_tensor(n_rows[order], device=dev),
                    torch.as_tensor(wealth[order], device=dev))


@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 513])
def test_pf_stats_matches_pf_ts(gpu, N, pad, B):
    """|dev - ref| <= 2e-13 * sum |terms| per statistic: an fp64 sum of n <= 513 terms in any
    order is within n u sum |x| ~ 6e-14 sum |x| of the exact one (u = 1.1e-16), plus a few
    roundings per term; months without a finite term (or a row) give exactly 0.  ld = N + 3 is
    unaligned for every other month (the scalar-load path)."""
    case = _case(N, B)
    ref, mag, zero = case[6:]
    out = _launch(case, pad, gpu)
    assert out.shape == (B, 5)
    got = out.cpu().numpy()
    err = np.abs(got - ref)
    print("max err / bound:", float((err / np.maximum(2e-13 * mag, 1e-300)).max()))
    assert (err <= 2e-13 * mag).all()
    for b in zero:
        assert np.array_equal(got[b], np.zeros(5)), b


@pytest.mark.parametrize("pad", [0, 3])
def test_pf_stats_bitwise_independent_of_launch_shape(gpu, pad):
    """A month's five numbers do not depend on B, on the month's position in the launch, or
    on the alignment of its rows (16-byte loads or the scalar path)."""
    case = _case(257, 7)
    full = _launch(case, pad, gpu)
    perm = [3, 6, 0, 5, 2, 1, 4]
    moved = _launch(case, pad, gpu, perm)
    for k, b in enumerate(perm):
        assert torch.equal(moved[k], full[b]), b
    for b in range(7):
        assert torch.equal(_launch(case, pad, gpu, [b])[0], full[b]), b
    # the other alignment / leading dimension gives the same bits too
    assert torch.equal(_launch(case, 3 - pad, gpu), full)


def test_pf_stats_reads_row_slices_in_place(gpu):
    """Columns [0, n) of wider buffers (the chain's [B, N] outputs) go through at their own
    row stride; rows of different strides are made contiguous first."""
    from pfml.ops.pfstats import pf_stats
    case = _case(65, 7)
    full = _launch(case, 0, gpu)
    w, ws, ret, lam, n_rows, wealth = case[:6]
    wide = [_padded(x, 7, 1e300, gpu) for x in (w, ws, ret, lam)]
    nr, wl = torch.as_tensor(n_rows, device=gpu), torch.as_tensor(wealth, device=gpu)
    assert torch.equal(pf_stats(*(x[:, :65] for x in wide), nr, wl), full)
    mixed = [wide[0][:, :65], wide[1][:, :65].contiguous(), wide[2][:, :65], wide[3][:, :65]]
    assert torch.equal(pf_stats(*mixed, nr, wl), full)


# ---------------------------------------------------------------------------------------
# backtest_device against the stage functions
# ---------------------------------------------------------------------------------------
def _load(cfg):
    from pfml.config import get_features
    from pfml.data import io
    from pfml.models.risk import BarraCov
    d = cfg.run.data_dir
    return (io.read_processed_chars(d, get_features()),
            BarraCov.load(os.path.join(d, "Barra_Cov.npz")),
            pd.read_csv(os.path.join(d, "wealth_processed.csv"), parse_dates=["eom"]),
            io.read_risk_free(d))


def _grids(cfg, barra):
    from pfml.utils.dates import pfml_date_grids
    s = cfg.settings
    return pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                           s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                           s["pf"]["dates"]["split_years"])


@pytest.mark.parametrize("compat", [True, False])
def test_backtest_device_matches_stage_functions(gpu, small_data, compat):
    """One S4 + grid search on the device, then the frame path (validation_frame ->
    aim_portfolios -> hps_bundle -> best_hps -> pfml_weights -> pf_ts) against
    backtest_device: identical (g, p, l) per OOS year, weights and statistics to the
    tolerance test_full_pipeline_gpu uses between two paths of this pipeline."""
    from pfml.models import pfml_inputs as pin
    from pfml.models import portfolio, search
    from pfml.utils.dates import month_end
    cfg = small_data.override(YEARS)
    cfg.run.compat_mode = compat
    chars, barra, wealth, rf = _load(cfg)
    g = _grids(cfg, barra)
    m2, oos = g["m2"], g["oos"]
    res = pin.build_inputs(cfg, chars, barra, wealth, rf, gpu, months=m2, keep_m=oos)
    R = search.complete_local_reals(res.reals.r_tilde, res.reals.denom, m2, cfg.hp_years)
    grid = search.grid_search(R, cfg)
    npad = pin.universe_npad(chars, m2)
    # the existing path
    val = search.validation_frame(grid, cfg)
    years_b, beta_b = search.gather_beta(grid)
    aims = portfolio.aim_portfolios(cfg, val, years_b, beta_b, m2, res.signal_t, res.ids, oos)
    hps = portfolio.hps_bundle(aims, val, res.rff_w)
    _, chosen, aim_df = portfolio.best_hps(hps, oos)
    w = portfolio.pfml_weights(cfg, chars, barra, wealth, rf, aim_df, oos, gpu,
                               m_cache=res.m_keep, n_pad=npad)
    pf = portfolio.pf_ts(w, chars, wealth, compat=compat)
    picks = {}
    for d in oos:
        a = hps[chosen[int(d)]["g"]]["aim_pfs_list"][int(d)]
        picks[int(month_end(int(d) + 1).year[0]) - 1] = (chosen[int(d)]["g"], a["p"], a["l"])
    # the device-resident path
    layout = portfolio.backtest_layout(cfg, chars, wealth, oos, m2, res.ids, gpu, n_pad=npad)
    bt = portfolio.backtest_device(cfg, grid, res, layout, wealth, gpu, keep_weights=True)
    assert bt["chosen"] == picks
    assert not bt["recomputed"]
    got_w = bt["weights"]
    assert got_w[["eom", "id"]].equals(w[["eom", "id"]])
    for c in ("mu_ld1", "tr_ld1", "w_start", "w"):
        assert np.allclose(got_w[c].to_numpy(), w[c].to_numpy(), rtol=1e-8, atol=1e-12,
                           equal_nan=True), c
    assert list(pd.to_datetime(bt["pf"]["eom_ret"])) == list(pd.to_datetime(pf["eom_ret"]))
    assert bt["stats"].shape == (len(oos), 5)
    assert np.allclose(bt["stats"], pf[STAT].to_numpy(), rtol=1e-8, atol=1e-12)


# ---------------------------------------------------------------------------------------
# the stage, end to end
# ---------------------------------------------------------------------------------------
def test_frontier_stage_two_points_end_to_end(gpu, small_data, tmp_path):
    """The ``pfml-ef`` stage for point A = (the wealth frame's own end wealth, gamma 10) and
    point B = (a tenth of it, gamma 20) - A through ``python -m pfml pfml-ef`` in a child
    process, B through ``Pipeline.run`` in this one (a second child would only pay the start-up
    again) - against the existing S4-S9 stages run per point on a copy of the data directory
    whose wealth_processed.csv holds the point's scaled path, with pf_set.wealth /
    pf_set.gamma_rel overridden."""
    from pfml.data.io import CSV_COLUMNS
    from pfml.models import frontier
    from pfml.pipeline import Pipeline
    base = small_data.override(YEARS)
    wealth = pd.read_csv(os.path.join(base.run.data_dir, "wealth_processed.csv"),
                         parse_dates=["eom"])
    w_end = frontier.frame_end_wealth(base, wealth)
    points = [(w_end, 10.0), (w_end / 10.0, 20.0)]
    rows = []
    for k, (W, gam) in enumerate(points):
        d = str(tmp_path / f"data_ef{k}")
        shutil.copytree(base.run.data_dir, d)
        sets = [f"ef.wealth=[{W!r}]", f"ef.gamma_rel=[{gam!r}]", "run.plots=False"]
        if k == 0:
            env = dict(os.environ,
                       PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
            cmd = [sys.executable, "-m", "pfml", "pfml-ef", "--data-dir", d, "--artifact-dir",
                   str(tmp_path / "art_ef0"), "--device", gpu.type]
            for s in YEARS + sets + [
                    f"split.test_end={base.settings['split']['test_end'].date()}",
                    "pf_ml.p_vec=" + str(base.p_vec).replace(" ", ""),
                    f"run.compat_mode={base.run.compat_mode}"]:
                cmd += ["--set", s]
            r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        else:
            cfg = base.override(sets + [f"run.data_dir={d}",
                                        f"run.artifact_dir={tmp_path}/art_ef{k}"])
            Pipeline(cfg, device=gpu.type).run(["pfml-ef"])
        ef = pd.read_csv(os.path.join(d, "ef.csv"))
        ef_pf = pd.read_csv(os.path.join(d, "ef_pf.csv"), parse_dates=["eom_ret"])
        assert list(ef.columns) == CSV_COLUMNS["ef.csv"]
        assert list(ef_pf.columns) == CSV_COLUMNS["ef_pf.csv"]
        assert len(ef) == 1 and ef["gamma_rel"].iloc[0] == gam
        assert np.isclose(ef["wealth_end"].iloc[0], W, rtol=1e-15)
        assert np.isfinite(ef[["r", "sd", "sr", "obj"]].to_numpy(float)).all()
        # the existing stages at this point
        dk = str(tmp_path / f"data_pt{k}")
        shutil.copytree(base.run.data_dir, dk)
        frontier.scaled_wealth(base, wealth, W).to_csv(
            os.path.join(dk, "wealth_processed.csv"), index=False)
        cfg = base.override([f"run.data_dir={dk}", f"run.artifact_dir={tmp_path}/art_pt{k}",
                             f"pf_set.wealth={W!r}", f"pf_set.gamma_rel={gam!r}",
                             "run.plots=False"])
        Pipeline(cfg, device=gpu.type).run(S4_S9)
        summ = pd.read_csv(os.path.join(dk, "pf_summary.csv"))
        pf = pd.read_csv(os.path.join(dk, "pf.csv"), parse_dates=["eom_ret"])
        num = [c for c in summ.columns if c != "type"]
        assert ef["type"].iloc[0] == summ["type"].iloc[0]
        assert np.allclose(ef[num].to_numpy(float), summ[num].to_numpy(float), rtol=1e-8,
                           atol=1e-12), (W, gam)
        assert list(ef_pf["eom_ret"]) == list(pf["eom_ret"])
        assert (ef_pf["gamma_rel"] == gam).all()
        assert np.allclose(ef_pf[STAT].to_numpy(), pf[STAT].to_numpy(), rtol=1e-8, atol=1e-12)
        rows.append(ef.iloc[0])
    # the overrides reached S4
    assert rows[0]["sd"] != rows[1]["sd"] or rows[0]["tc"] != rows[1]["tc"]


def test_chunked_m_func_repair_matches_one_batch(gpu, monkeypatch):
    """At wealth = 1 the device's Denman-Beavers check may send months to the reference-form
    repair; the frontier repairs them REPAIR_CHUNK at a time.  With the chunk lowered to 8 and
    20 months flagged by hand on top of the device's own flags, the chunked repair gives the
    summands and m_tilde of pfml_inputs' one-batch repair (the repair is per matrix; its
    square-root iteration stops on a batch-wide criterion, hence a tolerance: 1e-8 relative,
    the tolerance between two paths of this pipeline)."""
    from pfml.config import Config
    from pfml.data.synthetic import engine_inputs
    from pfml.models import frontier
    from pfml.models import pfml_inputs as pin
    cfg = Config.default().override(["pf_ml.p_vec=[8,16]", "pf.dates.start_year=2001",
                                     "pf.dates.end_yr=2004", "pf.dates.split_years=1",
                                     "split.test_end=2004-12-31"])
    cfg.run.compat_mode = False
    chars, barra, wealth, rf = engine_inputs(n_stocks=40, start="1993-01-31", end="2004-12-31")
    cfg_pt = frontier.point_config(cfg, 1.0, 10.0)
    wealth_pt = frontier.scaled_wealth(cfg, wealth, 1.0)
    g = _grids(cfg, barra)
    m2, oos = g["m2"], g["oos"]
    plan = pin.make_s4_plan(cfg_pt, chars, barra, wealth_pt, rf, gpu, m2)
    ref = pin.run_plan(plan, cfg_pt, keep_m=oos)
    out = pin.run_plan(plan, cfg_pt, keep_m=oos, defer_checks=True)
    print("months flagged by the device at wealth = 1:",
          int(out.pending["mstat"].sum().item()), "of", len(m2))
    out.pending["mstat"][-20:] = 1                       # OOS months among them (m_keep)
    monkeypatch.setattr(frontier, "REPAIR_CHUNK", 8)
    n = frontier._finish_chunked(plan, cfg_pt, out)
    assert n >= 20 and out.pending is None
    for a, b in ((out.reals.denom, ref.reals.denom), (out.reals.r_tilde, ref.reals.r_tilde),
                 (out.m_keep["mt"], ref.m_keep["mt"]), (out.m_keep["a"], ref.m_keep["a"])):
        assert torch.isfinite(a).all()
        assert (a - b).abs().max().item() <= 1e-8 * b.abs().max().item()
