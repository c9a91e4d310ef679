"""p = 1024 and p = 2048 on the device: the ridge grid's tridiagonal path up to n = 2049, its
dense repair, the utilities, the window sums / grid search and S4 at P = 1025, each against the
fp64 CPU oracle of the same entry point."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand(*shape, seed=0, dev="cpu"):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dev)


def _spd_stack(S, P, n_obs=40, seed=0):
    X = _rand(S, n_obs, P, seed=seed)
    return X.transpose(1, 2) @ X


@functools.lru_cache(maxsize=None)
def _stack(P, n_obs):
    """(SD, Sr) of 2 window sums of ``n_obs`` observations, shared by the tests (read only)."""
    SD = _spd_stack(2, P, n_obs=n_obs, seed=801)
    return 0.5 * (SD + SD.transpose(1, 2)), _rand(2, P, seed=802)


def _lambdas(full_rank: bool) -> torch.Tensor:
    lam = np.exp(np.linspace(-10, 10, 8)) if full_rank else np.exp(np.linspace(-2, 10, 8))
    return torch.tensor([0.0] + list(lam), dtype=torch.float64)


def _ridge_rel(gpu, SD, Sr, src, nn, lv, ok=slice(None)):
    """max over (cell, lambda) of |device - oracle| / |oracle|; the output must hold no NaN."""
    from pfml.ops import ridge as rg
    src, nn = np.asarray(src), np.asarray(nn)
    sc = np.full(len(nn), 1e-3)
    ref = rg.ridge_grid(SD, Sr, src, nn, sc, lv)
    out = rg.ridge_grid(SD.to(gpu), Sr.to(gpu), src, nn, sc, lv.to(gpu)).cpu()
    assert not torch.isnan(out).any()
    for c, n in enumerate(nn):                       # padding columns [n, P) are zero
        assert not out[c, :, n:].any()
    return ((out[:, ok] - ref[:, ok]).norm(dim=-1) / ref[:, ok].norm(dim=-1)).max().item()


@pytest.mark.parametrize("n_obs", [3000, 800])
def test_ridge_large_n_matches_lu(gpu, n_obs):
    """1024 < n <= 2049 (p = 1024 .. 2048) vs the LU-solve oracle, full rank (n_obs = 3000,
    lambda = 0 included) and rank deficient (n_obs = 800 < n: lambda = 0 is singular, so it
    has no unique solution to compare and must only come back finite)."""
    from pfml.ops import ridge as rg
    assert rg.nat.hip_lib().pfml_ridge_nmax() == 2049
    SD, Sr = _stack(2049, n_obs)
    full = n_obs > 2049
    rel = _ridge_rel(gpu, SD, Sr, [0, 1, 0], [1025, 1500, 2049], _lambdas(full),
                     ok=slice(None) if full else slice(1, None))
    print(f"n_obs={n_obs} rel={rel:.3e}")
    assert rel < 1e-9, rel


def test_ridge_boundary_1024_1025(gpu):
    """n = 1024 (the n <= 1024 kernel instances) and n = 1025 (the large ones) in two launches
    from one P = 1025 stack."""
    SD, Sr = _stack(1025, 1500)
    for n in (1024, 1025):
        rel = _ridge_rel(gpu, SD, Sr, [0, 1], [n, n], _lambdas(True))
        print(f"n={n} rel={rel:.3e}")
        assert rel < 1e-9, (n, rel)


@pytest.mark.parametrize("n", [1040, 1041, 2048])
def test_ridge_ragged_sizes(gpu, n):
    """Sizes off the 64 k + 1 grid of p = 2^k: n a multiple of 16, one more, and 2048 (the last
    panel of 16 reflectors is ragged, the column sweep ends inside a 64-column block)."""
    SD, Sr = _stack(2049, 3000)
    rel = _ridge_rel(gpu, SD, Sr, [1], [n], _lambdas(True))
    print(f"n={n} rel={rel:.3e}")
    assert rel < 1e-9, (n, rel)


def test_ridge_placement_independent(gpu):
    """The n = 1025 cell's betas are bitwise the same alone and as the last of four cells, for
    L = 5 and L = 101 (the lambdas both share)."""
    from pfml.ops.ridge import ridge_grid
    SD, Sr = _stack(2049, 3000)
    SDd, Srd = SD.to(gpu), Sr.to(gpu)
    lv101 = torch.tensor([0.0] + list(np.exp(np.linspace(-10, 10, 100))), dtype=torch.float64)
    pick = [0, 10, 50, 75, 100]
    lv5 = lv101[pick]
    alone = ridge_grid(SDd, Srd, np.array([1]), np.array([1025]), np.array([1e-3]), lv5.to(gpu))
    assert torch.isfinite(alone).all()
    src, nn = np.array([0, 1, 0, 1]), np.array([2049, 1500, 1100, 1025])
    sc = np.full(4, 1e-3)
    four5 = ridge_grid(SDd, Srd, src, nn, sc, lv5.to(gpu))
    four101 = ridge_grid(SDd, Srd, src, nn, sc, lv101.to(gpu))
    assert torch.equal(four5[3], alone[0])
    assert torch.equal(four101[3, pick], alone[0])


def test_ridge_dense_repair_above_1024(gpu):
    """The dense device repair at n = 1100 / 1030: exactly the NaN-marked systems re-solved to
    the LU oracle, the others untouched."""
    from pfml.ops import ridge as rg
    P = 1100
    SD = _spd_stack(2, P, n_obs=1400, seed=803)
    Sr = _rand(2, P, seed=804)
    lv = torch.tensor([0.0] + list(np.exp(np.linspace(-6, 6, 11))), dtype=torch.float64)
    src, nn, sc = np.array([0, 1]), np.array([1100, 1030]), np.full(2, 1e-3)
    beta = rg.ridge_grid(SD.to(gpu), Sr.to(gpu), src, nn, sc, lv.to(gpu), repair=False)
    keep = beta.clone()
    marks = [(0, 0), (1, 5), (1, 11), (0, 3)]
    for c, l in marks:
        beta[c, l, :nn[c]] = float("nan")
    plan = rg.ridge_plan(P, len(lv), src, nn, sc)
    d_desc, = rg.upload([plan["desc"]], beta.device)
    cnt = rg.repair_launch(plan, d_desc, SD.to(gpu).contiguous(), Sr.to(gpu).contiguous(),
                           lv.to(gpu), beta)
    assert int(cnt.item()) == len(marks)
    ref = rg.ridge_grid(SD, Sr, src, nn, sc, lv)
    out = beta.cpu()
    for c, l in marks:
        rel = ((out[c, l] - ref[c, l]).norm() / ref[c, l].norm()).item()
        assert rel < 1e-9, (c, l, rel)
    untouched = torch.ones(beta.shape[:2], dtype=torch.bool)
    for c, l in marks:
        untouched[c, l] = False
    assert torch.equal(out[untouched], keep.cpu()[untouched])


def test_repair_scratch_bounded_above_1025():
    """The retained repair scratch never exceeds what nmax = 1025 takes (64 systems)."""
    from pfml.ops import ridge as rg
    lib = rg.nat.hip_lib()
    at1025 = int(lib.pfml_ridge_repair_work_doubles_cap(1025, 10 ** 6))
    assert at1025 == 64 * 1025 * 1026
    for nmax in (1026, 1100, 1500, 2049):
        w = int(lib.pfml_ridge_repair_work_doubles_cap(nmax, 10 ** 6))
        assert nmax * (nmax + 1) <= w <= at1025 and w % (nmax * (nmax + 1)) == 0
    assert int(lib.pfml_ridge_repair_work_doubles_cap(2049, 3)) == 3 * 2049 * 2050


def test_quadform_utilities_large_n(gpu):
    """Utilities at n = 1025 (17 row tiles, tail index split off), 1100 (18, no split) and
    2049 (32 + split), 3 validation months per cell, L = 101."""
    from pfml.ops.ridge import quadform_utilities
    T, P, L = 3, 2049, 101
    D = _spd_stack(T, P, n_obs=50, seed=805)
    R = _rand(T, P, seed=806)
    beta = _rand(3, L, P, seed=807)
    ns = [1025, 1100, 2049]
    jc = np.repeat(np.arange(3), T)
    jm = np.tile(np.arange(T), 3)
    jn = np.repeat(ns, T)
    for c, n in enumerate(ns):
        beta[c, :, n:] = 0.0
    ref = quadform_utilities(D, R, beta, jc, jm, jn)
    out = quadform_utilities(D.to(gpu), R.to(gpu), beta.to(gpu), jc, jm, jn).cpu()
    rel = ((out - ref).abs() / ref.abs().clamp_min(1e-12)).max().item()
    print(f"rel={rel:.3e}")
    assert rel < 1e-8, rel


def test_ridge_refuses_above_limit(gpu):
    """n = 2050 (p = 2049) on the device: a ValueError naming the limit and the p, raised by
    the plan, not a failed native call."""
    from pfml.ops.ridge import ridge_grid
    P = 2050
    SD = torch.zeros(1, P, P, dtype=torch.float64, device=gpu)
    Sr = torch.zeros(1, P, dtype=torch.float64, device=gpu)
    lv = torch.tensor([0.0, 1.0], dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError, match=r"p = 2049 .*2049.*p <= 2048"):
        ridge_grid(SD, Sr, np.array([0, 0]), np.array([65, 2050]), np.ones(2), lv)


@functools.lru_cache(maxsize=None)
def _reals_1025():
    """Synthetic reals as in test_grid_search_gpu_matches_cpu: G = 1, 69 months, P = 1025, 40
    observations per month (the first window, 45 months, holds 1800 > 1025: full rank)."""
    from pfml.utils.dates import mi_from_ym
    G, P = 1, 1025
    months = np.arange(mi_from_ym(2000, 3), mi_from_ym(2005, 11) + 1)
    T = len(months)
    X = _rand(G * T, 40, P, seed=811)
    D = (X.transpose(1, 2) @ X / 40).view(G, T, P, P)
    r = 0.1 * _rand(G, T, P, seed=812)
    return months, r, D


@pytest.mark.parametrize("p_vec", ["[16,1024]", "[16,600,1024]"])
def test_grid_search_p_1024_gpu_matches_cpu(gpu, p_vec):
    """Window sums, ridge grid (two, then three launch groups) and utilities at P = 1025."""
    from pfml.config import Config
    from pfml.models.search import PfmlReals, grid_search
    cfg = Config.default().override([f"pf_ml.p_vec={p_vec}",
                                     "pf_ml.l_vec=[0.0,0.0001,0.01,1.0,10.0,100.0]",
                                     "pf.dates.start_year=2004", "pf.dates.end_yr=2005"])
    months, r, D = _reals_1025()
    cpu = grid_search(PfmlReals(months, r, D), cfg)
    assert torch.isfinite(cpu.beta).all()
    dev = grid_search(PfmlReals(months, r.to(gpu), D.to(gpu)), cfg)
    rb = ((dev.beta.cpu() - cpu.beta).norm(dim=-1) / cpu.beta.norm(dim=-1)).max().item()
    ro = ((dev.obj.cpu() - cpu.obj).abs() / cpu.obj.abs().clamp_min(1e-12)).max().item()
    print(f"p_vec={p_vec} rb={rb:.3e} ro={ro:.3e}")
    assert rb < 1e-9, rb
    assert ro < 1e-8, ro


def test_pfml_inputs_p_1024_gpu_matches_cpu(gpu, small_data):
    """S4 (build_inputs) with p_max = 1024 (P = 1025) over 6 months vs the CPU path."""
    from pfml.config import get_features
    from pfml.data import io
    from pfml.models.pfml_inputs import build_inputs
    from pfml.models.risk import BarraCov
    from pfml.utils.dates import pfml_date_grids
    cfg = small_data.override(["pf_ml.p_vec=[8,1024]"])
    cfg.run.compat_mode = False          # W drawn for p_max / 2 = 512 (rff_w.csv holds 256)
    d = cfg.run.data_dir
    chars = io.read_processed_chars(d, get_features())
    barra = BarraCov.load(os.path.join(d, "Barra_Cov.npz"))
    wealth = pd.read_csv(os.path.join(d, "wealth_processed.csv"), parse_dates=["eom"])
    rf = io.read_risk_free(d)
    g = pfml_date_grids(int(barra.months.min()), 11, cfg.settings["split"]["test_end"], 1971, 10)
    months = g["m2"][:6]
    cpu = build_inputs(cfg, chars, barra, wealth, rf, "cpu", months=months)
    dev = build_inputs(cfg, chars, barra, wealth, rf, gpu, months=months)
    assert cpu.reals.denom.shape[-1] == 1025
    for a, b in [(dev.reals.r_tilde.cpu(), cpu.reals.r_tilde),
                 (dev.reals.denom.cpu(), cpu.reals.denom)]:
        err = (a - b).abs().max().item() / b.abs().max().item()
        print(f"err={err:.3e}")
        assert err < 1e-11, err
