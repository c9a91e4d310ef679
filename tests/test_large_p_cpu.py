"""p = 1024 and 2048 on the host side: the launch grouping rule of ridge_utilities and the
CPU oracle path, which has no size limit."""
import numpy as np
import torch


def _groups(ns):
    from pfml.ops.ridge import ridge_groups
    n = np.asarray(ns)
    return [sorted(n[g].tolist()) for g in ridge_groups(n)], ridge_groups(n)


def test_ridge_groups_default_grid_is_largest_and_rest():
    # [g][year][p] cell order, two years: every index once, the two groups of today
    n = np.tile([65, 129, 257, 513], 2)
    vals, idx = _groups(n)
    assert vals == [[513, 513], [65, 65, 129, 129, 257, 257]]
    assert np.array_equal(idx[0], np.nonzero(n == 513)[0])
    assert np.array_equal(idx[1], np.nonzero(n != 513)[0])


def test_ridge_groups_one_value_above_band():
    vals, _ = _groups([65, 513, 1025])
    assert vals == [[1025], [65, 513]]
    vals, _ = _groups([601, 1024])
    assert vals == [[1024], [601]]
    vals, _ = _groups([16, 600])
    assert vals == [[600], [16]]


def test_ridge_groups_band_cells_never_with_tridiagonal_cells():
    from pfml.ops.ridge import BAND_NMAX
    vals, idx = _groups([65, 513, 1025, 2049])
    assert vals == [[2049], [1025], [65, 513]]
    assert max(vals[2]) <= BAND_NMAX < min(vals[1])
    # every cell in exactly one group
    assert sorted(np.concatenate(idx).tolist()) == [0, 1, 2, 3]
    vals, _ = _groups([17, 601, 1025])
    assert vals == [[1025], [601], [17]]
    # two tridiagonal sizes and no band cell in the rest: still two groups
    vals, _ = _groups([601, 1025, 2049])
    assert vals == [[2049], [601, 1025]]


def test_cpu_grid_search_p_1024():
    """The CPU oracle path takes p = 1024 (n = 1025): it runs and every beta is finite."""
    from pfml.config import Config
    from pfml.models.search import PfmlReals, grid_search
    from pfml.utils.dates import mi_from_ym
    cfg = Config.default().override(["pf_ml.p_vec=[16,1024]", "pf_ml.l_vec=[0.0,0.01,1.0]",
                                     "pf.dates.start_year=2002", "pf.dates.end_yr=2002"])
    P = 1025
    months = np.arange(mi_from_ym(2000, 12), mi_from_ym(2002, 11) + 1)
    T = len(months)
    g = torch.Generator().manual_seed(5)
    X = torch.randn(T, 4, P, generator=g, dtype=torch.float64)
    D = (X.transpose(1, 2) @ X / 4 + 0.1 * torch.eye(P, dtype=torch.float64)).view(1, T, P, P)
    r = 0.1 * torch.randn(1, T, P, generator=g, dtype=torch.float64)
    res = grid_search(PfmlReals(months, r, D), cfg)
    assert res.beta.shape == (1, 1, 2, 3, P)
    assert torch.isfinite(res.beta).all()
    assert torch.isfinite(res.obj).all()
    assert bool(res.beta[0, 0, 1, :, 1024].abs().min() > 0)      # all 1025 rows are solved
