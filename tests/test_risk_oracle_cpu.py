"""The conditions that keep tests/test_gpu_risk_edges.py honest, checked without a GPU: the fp64
CPU branches of daily_ols / ewma_factor_cov / ewma_vol against the longdouble oracle on every
case the GPU tests use, the size of the tolerances that follow from them, the oracle's
minimum-norm construction against numpy's pinv, and the argument refusals of the ops.

Figures of the fp64 CPU paths on these cases (not kernel figures): OLS error 3e-16 to 5e-14 with
kappa_2 up to 1.8e4 at n = K + 1 and at most 270 at n = 2K; covariance F at most 7 u, cor at
most 4 u; volatility at most 10 u."""
import numpy as np
import pytest
import torch

import risk_oracle as ro
from risk_oracle import U

COV_CASES = [(K, obs) for K in ro.COV_KS for obs in ro.COV_OBS]
VOL_CASES = [(s, lam) for s in ro.VOL_STARTS for lam in ro.VOL_LAMS]


# ---------------------------------------------------------------------------------------------
# CPU branches against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", ro.OLS_KS)
def test_ols_cpu_branch_and_tolerances(K):
    ex = ro.ols_expect(K)
    ro.ols_check(ex, ex["cpu_coef"], ex["cpu_resid"], ex["cpu_status"], ex["cpu_nbad"], "cpu")
    ro.ols_self_consistent(ex["X"], ex["y"], ex["off"], ex["cpu_coef"], ex["cpu_resid"])
    for d, kind in enumerate(ex["kinds"]):
        if kind in (ro.CMP, ro.DUP, ro.ZERO):
            assert ex["kappa"][d] < 2e5, (d, ex["kappa"][d])
            assert ex["tol"][d] <= 1e-9, (d, ex["tol"][d])
            if ex["sizes"][d] >= 2 * K:
                assert ex["tol"][d] <= 1e-11, (d, ex["tol"][d])
        else:
            assert np.isnan(ex["tol"][d])


@pytest.mark.parametrize("K", ro.OLS_KS)
def test_ols_only_the_named_days_are_left_out(K):
    """Every day is compared except the 0-row day(s) (coef == 0 is asserted instead) and the
    under-determined 1-row and (K-1)-row days the builder names; the compared set holds every
    day size of the sweep and, from K = 2, both structured singular days."""
    c = ro.ols_case(K)
    kinds, sizes = c["kinds"], c["sizes"]
    checked = ro.ols_checked_days(c)
    named = [d for d, k in enumerate(kinds) if k == ro.UNDER]
    assert [sizes[d] for d in named] == [n for n in (1, K - 1) if 0 < n < K]
    assert len(checked) == len(kinds) - len(named) - kinds.count(ro.EMPTY)
    assert kinds.count(ro.EMPTY) == (2 if K == 1 else 1)
    want = {K + 1, 2 * K, 63, 64, 65, 127, 128, 129, 200, 513}
    assert want <= {sizes[d] for d in checked if kinds[d] == ro.CMP}
    assert kinds.count(ro.DUP) == kinds.count(ro.ZERO) == (1 if K >= 2 else 0)
    nd = min(12, K - 1)
    for d in checked:
        a, b = c["off"][d], c["off"][d + 1]
        assert set(np.unique(c["X"][a:b, :nd])) <= {0.0, 1.0}
        assert np.all(c["X"][a:b, :nd].sum(0) >= 1)            # every industry present
        assert nd == 0 or kinds[d] == ro.DUP or np.all(c["X"][a:b, :nd].sum(1) == 1)


@pytest.mark.parametrize("K", [k for k in ro.OLS_KS if k >= 2])
def test_minimum_norm_reference_equals_pinv(K):
    ex = ro.ols_expect(K)
    for d, sp in ex["special"].items():
        a, b = ex["off"][d], ex["off"][d + 1]
        Xd, yd = ex["X"][a:b], ex["y"][a:b]
        p = np.linalg.pinv(Xd.T @ Xd) @ (Xd.T @ yd)
        ref = ex["coef"][d].astype(np.float64)
        assert np.abs(p - ref).max() <= 1e-9 * np.abs(ref).max(), (d, sp)
        if sp[0] == ro.DUP:
            assert ref[sp[1]] == ref[sp[2]] != 0
        else:
            assert ref[sp[1]] == 0


@pytest.mark.parametrize("K,obs", COV_CASES)
def test_cov_cpu_branch_and_tolerances(K, obs):
    ex = ro.cov_expect(K, obs)
    assert ex["tol"].max() <= 1e-13
    assert list(ex["ends"]) == sorted({2, 5, 63, 64, 65, obs - 1, obs, obs + 1, obs + 70})
    ratio = ex["fr"].mean(0) / ex["fr"].std(0)
    assert np.all((ratio > 50) | (ratio < 0.5))
    assert K == 1 or ((ratio > 50).any() and (ratio < 0.5).any())


@pytest.mark.parametrize("start,lam", VOL_CASES)
def test_vol_cpu_branch_and_tolerances(start, lam):
    from pfml.ops.risk_kernels import ewma_vol
    ex = ro.vol_expect(start, lam)
    assert ex["tol"] <= 1e-13
    assert (len(ex["gs"]) - 1) % 4 != 0
    out = ewma_vol(torch.tensor(ex["x"]), ex["gs"], lam, start).numpy()
    assert ro.vol_err(out, ex["ref"]) <= ex["tol"]
    # the named groups: all-NaN for <= 1 valid row in the window, values elsewhere
    gs = ex["gs"]
    assert np.isnan(ex["ref"][gs[9]:gs[10]]).all()
    assert np.isnan(ex["x"][gs[10] + start - 1]) and np.isnan(ex["x"][gs[12] - 1])
    assert np.isfinite(ex["ref"][gs[8] + start:gs[9]]).all()


def test_one_day_window_is_nan_on_the_cpu_branch():
    from pfml.ops.risk_kernels import ewma_factor_cov
    c = ro.cov_case(2, 64)
    F, cor, var = ewma_factor_cov(torch.tensor(c["fr"]), [1], 64, c["w_cor"], c["w_var"],
                                  return_parts=True)
    assert torch.isnan(F).all() and torch.isnan(var).all()
    assert torch.equal(torch.diagonal(cor[0]), torch.ones(2, dtype=torch.float64))
    Fr, cr, vr = ro.cov_ref(c["fr"], [1], 64, c["w_cor"], c["w_var"], 21.0)
    assert np.isnan(Fr).all() and np.isnan(vr).all()


def test_empty_launches_cpu():
    from pfml.ops.risk_kernels import daily_ols, ewma_factor_cov, ewma_vol
    coef, resid, nbad = daily_ols(torch.zeros((0, 5)), torch.zeros(0), torch.zeros(1, dtype=torch.int64))
    assert coef.shape == (0, 5) and resid.shape == (0,) and nbad == 0
    assert coef.dtype == resid.dtype == torch.float64
    w = np.ones(8)
    for parts in (False, True):
        out = ewma_factor_cov(torch.zeros((10, 3), dtype=torch.float64), [], 8, w, w, return_parts=parts)
        for t in (out if parts else (out,)):
            assert t.shape == (0, 3, 3) and t.dtype == torch.float64
    v = ewma_vol(torch.zeros(0, dtype=torch.float64), np.zeros(1, np.int64), 0.97, 5)
    assert v.shape == (0,) and v.dtype == torch.float64


# ---------------------------------------------------------------------------------------------
# argument refusals (the same checks run before a device launch)
# ---------------------------------------------------------------------------------------------
def test_factor_cov_refuses_bad_ends_and_short_weights():
    from pfml.ops.risk_kernels import ewma_factor_cov
    fr = torch.zeros((20, 3), dtype=torch.float64)
    w = np.ones(8)
    ewma_factor_cov(fr, [0, 20], 8, w, w)                      # the limits themselves pass
    for ends in ([21], [5, -1], np.array([3, 2 ** 40])):
        with pytest.raises(ValueError):
            ewma_factor_cov(fr, ends, 8, w, w)
    with pytest.raises(ValueError):
        ewma_factor_cov(fr, [10], 8, w[:7], w)
    with pytest.raises(ValueError):
        ewma_factor_cov(fr, [10], 8, w, w[:7])
    ewma_factor_cov(fr, [10], 8, np.ones(9), np.ones(12))      # longer weights are accepted


@pytest.mark.parametrize("off", [[0, 5, 11], [0, 6, 5, 10], [-1, 5, 10], [1, 12], []])
def test_daily_ols_refuses_bad_offsets(off):
    from pfml.ops.risk_kernels import daily_ols
    X, y = torch.ones((10, 2), dtype=torch.float64), torch.ones(10, dtype=torch.float64)
    with pytest.raises(ValueError):
        daily_ols(X, y, torch.tensor(off, dtype=torch.int64))


def test_daily_ols_refuses_a_short_y_and_accepts_partial_cover():
    from pfml.ops.risk_kernels import daily_ols
    X = torch.tensor(np.random.default_rng(0).standard_normal((10, 2)))
    with pytest.raises(ValueError):
        daily_ols(X, torch.ones(9, dtype=torch.float64), torch.tensor([0, 10]))
    coef, _, _ = daily_ols(X, torch.ones(10, dtype=torch.float64), torch.tensor([2, 5, 5, 9]))
    assert coef.shape == (3, 2)


@pytest.mark.parametrize("as_tensor", [False, True])
@pytest.mark.parametrize("gs", [[0, 5, 11], [0, 6, 5, 10], [-1, 5, 10], []])
def test_ewma_vol_refuses_bad_groups(gs, as_tensor):
    from pfml.ops.risk_kernels import ewma_vol
    x = torch.ones(10, dtype=torch.float64)
    g = torch.tensor(gs, dtype=torch.int64) if as_tensor else np.array(gs, np.int64)
    with pytest.raises(ValueError):
        ewma_vol(x, g, 0.97, 3)


def test_ewma_vol_refuses_a_negative_start():
    from pfml.ops.risk_kernels import ewma_vol
    with pytest.raises(ValueError):
        ewma_vol(torch.ones(10, dtype=torch.float64), np.array([0, 10]), 0.97, -1)
