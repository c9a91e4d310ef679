"""The factor-structured solves on the CPU: the references of tests/factor_oracle.py against
each other, and the torch branch of pfml.ops.factor_solve (the CPU path, and the path beyond
the kernels' limits) against them with the bound the device test uses."""
import numpy as np
import pytest
import torch

import factor_oracle as fo

LD = fo.LD


def _t(x):
    return torch.as_tensor(x)


def _run(inp):
    from pfml.ops import factor_solve as fs
    M, status = fs.factor_prepare(_t(inp["X"]), _t(inp["ridx"]), _t(inp["F"]),
                                  _t(inp["fscale"]), _t(inp["d"]), _t(inp["n_rows"]))
    out = fs.factor_chain(_t(inp["X"]), _t(inp["ridx"]), M, _t(inp["d"]), _t(inp["n_rows"]),
                          _t(inp["rhs"]), _t(inp["c"]), inp["varm"], inp["normalize"],
                          _t(inp["grow"]), _t(inp["nmap"]), _t(inp["hit"]), _t(inp["ws0"]))
    return M, status, out


def test_refined_solve_is_the_explicit_longdouble_solve():
    """DenseSolver (fp64 LU of the explicit matrix, longdouble refinement through the factors)
    against Gaussian elimination on the explicit longdouble matrix, and the factored product
    against the explicit one."""
    inp = fo.factor_inputs(65, 12, 1, 4, seed=1)
    for v in range(4):
        X, Fs, d = fo.month_system(inp, v, 0)
        S = fo.explicit_matrix_ld(X, Fs, d)
        b = inp["rhs"][v, 0].astype(LD)
        w = fo.DenseSolver(X, Fs, d).solve(b)
        assert float(np.max(np.abs(S @ w - fo.ld_apply(X, Fs, d, w)))) <= \
            1e-17 * float(np.max(np.abs(b)))
        w2 = fo.ld_solve(S, b)
        assert float(np.max(np.abs(w - w2))) <= 1e-16 * float(np.max(np.abs(w2)))


@pytest.mark.parametrize("N,K,B,A,zero", [(1, 1, 1, 1, None), (2, 12, 5, 3, None),
                                          (65, 25, 5, 8, None), (130, 33, 2, 4, 3)])
def test_torch_branch_against_longdouble(N, K, B, A, zero):
    inp = fo.factor_inputs(N, K, B, A, seed=10 * N + K, zero_factor=zero)
    ref = fo.Reference(inp)
    M, status, (Wst, Wopt, ws_end) = _run(inp)
    assert not status.any()
    used = {(int(v), t) for v in inp["varm"] for t in range(B)}
    worst_m, orc_m = fo.check_m(ref, M.numpy(), used)
    worst_w, orc_w = fo.check_chain(ref, Wst.numpy(), Wopt.numpy())
    print(f"N={N} K={K}: M err/bound={worst_m:.3f} (oracle rel {orc_m:.2e})  "
          f"w err/bound={worst_w:.3f} (oracle rel {orc_w:.2e})")
    assert orc_m < 1e-13 and orc_w < 1e-13
    assert worst_m <= 1.0 and worst_w <= 1.0
    assert torch.equal(Wst[:, 0], _t(inp["ws0"]))
    for t in range(B):
        nxt = Wst[:, t + 1] if t + 1 < B else ws_end
        assert torch.equal(nxt, fo.drift(Wopt[:, t], _t(inp["grow"][t]), _t(inp["nmap"][t]),
                                         _t(inp["hit"][t])))


def test_torch_branch_f_zero_and_status():
    from pfml.ops import factor_solve as fs
    inp = fo.factor_inputs(17, 5, 2, 4, seed=3, f_zero=True)
    M, status, (Wst, Wopt, _) = _run(inp)
    assert not status.any() and not M.any()
    n = inp["n_rows"]
    for a in range(4):
        for t in range(2):
            if inp["normalize"][a]:
                continue
            b = inp["rhs"][a, t] + inp["c"][a, t] * Wst[a, t].numpy()
            assert np.array_equal(Wopt[a, t, :n[t]].numpy(),
                                  (b / inp["d"][inp["varm"][a], t])[:n[t]])
    # G = I, F = -I: I + F G = 0, a zero pivot; a NaN diagonal: non-finite
    X = torch.eye(2, dtype=torch.float64)
    ridx = torch.arange(2)[None]
    one = torch.ones((1, 1, 2), dtype=torch.float64)
    args = (X, ridx, -torch.eye(2, dtype=torch.float64)[None], torch.ones(1, dtype=torch.float64))
    _, st = fs.factor_prepare(*args, one, torch.tensor([2]))
    assert int(st[0, 0]) & fs.ST_ZERO_PIVOT
    _, st = fs.factor_prepare(*args, one * float("nan"), torch.tensor([2]))
    assert int(st[0, 0]) & fs.ST_NONFINITE


def test_empty_chain():
    inp = fo.factor_inputs(9, 3, 0, 3, seed=5)
    M, status, (Wst, Wopt, ws_end) = _run(inp)
    assert M.shape == (4, 0, 3, 3) and Wst.shape == (3, 0, 9) and Wopt.shape == (3, 0, 9)
    assert torch.equal(ws_end, _t(inp["ws0"]))


def _ratio_error(ratio, seeds=6):
    """Worst error, relative to max|w|, of the torch branch against the longdouble dense solve
    when one row's d is ``ratio`` times below the factor part of its diagonal (the Markowitz
    and the normalised minimum-variance arm of factor_inputs, N = 65, K = 12)."""
    worst = 0.0
    for seed in range(seeds):
        inp = fo.factor_inputs(65, 12, 1, 3, seed=40 + seed)
        for v in (0, 2):
            X, Fs, d = fo.month_system(inp, v, 0)
            inp["d"][v, 0, 7] = np.einsum("k,kl,l->", X[7], Fs, X[7]) / ratio
        M, status, (Wst, Wopt, _) = _run(inp)
        assert not status.any()
        for a in (0, 2):
            X, Fs, d = fo.month_system(inp, a, 0)
            assert np.linalg.cond(X @ Fs @ X.T + np.diag(d)) < 1e4      # the matrix stays benign
            w_ld = fo.DenseSolver(X, Fs, d).solve(inp["rhs"][a, 0].astype(LD))
            w_ld = w_ld / np.sum(w_ld) if inp["normalize"][a] else w_ld
            err = float(np.max(np.abs(Wopt[a, 0].numpy().astype(LD) - w_ld)))
            worst = max(worst, err / float(np.max(np.abs(w_ld))))
    return worst


def test_split_ratio_threshold_is_measured():
    """The Woodbury form divides by d first, so it loses digits when a d_i is far below the
    factor part of its diagonal although the explicit matrix is as well conditioned as ever.
    Measured here (and at N = 500, K = 25: smaller throughout): about 4e-3 u ratio^2 - 5e-15
    at 1e2, 5e-13 at 1e3, 4e-11 at 1e4, 2e-9 at 1e5, 3e-7 at 1e6.  benchmarks.SPLIT_RATIO_MAX
    is the largest decade that keeps the 1e-10 of the stage's oracle checks."""
    from pfml.models.benchmarks import SPLIT_RATIO_MAX
    at_max, above = _ratio_error(SPLIT_RATIO_MAX), _ratio_error(10.0 * SPLIT_RATIO_MAX)
    print(f"ratio {SPLIT_RATIO_MAX:g}: {at_max:.2e}; ratio {10 * SPLIT_RATIO_MAX:g}: {above:.2e}")
    assert _ratio_error(1e2) <= 1e-13
    assert at_max <= 1e-10 < above
