"""The factor-structured solve kernels (csrc/factor_solve.hip through pfml.ops.factor_solve):
factor_prepare's M against the longdouble (I + F_s G)^-1 F_s, every chain month against the
longdouble dense solve taken from the device's own w_start of that month, with the bound of
test_gpu_stage_kernels.py - at most 8 x the error of the same Woodbury formula evaluated
sequentially in fp64 numpy (tests/factor_oracle.py), plus a floor of (n + K) u max|w| - and the
bitwise properties: independence of the other arms and of the position, chain prefixes, the
drift expression, c = 0, F = 0, NaN isolation; the limits and the empty chain."""
import functools

import numpy as np
import pytest
import torch

import factor_oracle as fo

pytestmark = pytest.mark.gpu

NAN = float("nan")
GPU = torch.device("cuda", 0)


def _d(x):
    return torch.as_tensor(np.asarray(x)).to(GPU)


def _table(X):
    """X as a strided view inside a NaN-filled buffer."""
    R, K = X.shape
    buf = torch.full((R + 2, K + 5), NAN, dtype=torch.float64, device=GPU)
    buf[1:R + 1, 2:K + 2] = _d(X)
    view = buf[1:R + 1, 2:K + 2]
    assert view.stride(0) == K + 5 and (R == 1 or K == 1 or not view.is_contiguous())
    return view


def _prepare(inp, fn=None):
    from pfml.ops import factor_solve as fs
    fn = fn or fs.factor_prepare
    return fn(_table(inp["X"]), _d(inp["ridx"]), _d(inp["F"]), _d(inp["fscale"]), _d(inp["d"]),
              _d(inp["n_rows"]))


def _chain(inp, M, arms=None, months=None, ws0=None, rhs=None, fn=None):
    """The chain of the arms ``arms`` (default all) over the first ``months`` months."""
    from pfml.ops import factor_solve as fs
    fn = fn or fs.factor_chain
    a = np.arange(inp["A"]) if arms is None else np.asarray(arms)
    b = inp["B"] if months is None else months
    rhs = inp["rhs"] if rhs is None else rhs
    ws0 = inp["ws0"][a] if ws0 is None else ws0
    out = fn(_table(inp["X"]), _d(inp["ridx"][:b]), M[:, :b].contiguous(), _d(inp["d"][:, :b]),
             _d(inp["n_rows"][:b]), _d(rhs[a][:, :b]), _d(inp["c"][a][:, :b]),
             inp["varm"][a], inp["normalize"][a], _d(inp["grow"][:b]), _d(inp["nmap"][:b]),
             _d(inp["hit"][:b]), _d(ws0))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _case(N, K, B, A, zero=None, f_zero=False):
    """Inputs, shared references and the device's outputs of one shape (computed once)."""
    inp = fo.factor_inputs(N, K, B, A, seed=1000 * N + 10 * K + B, zero_factor=zero,
                           f_zero=f_zero)
    M, status = _prepare(inp)
    out = _chain(inp, M)
    return inp, fo.Reference(inp), M, status, out


SHAPES = [(1, 1, 1, 1), (2, 12, 5, 3), (63, 25, 5, 3), (64, 33, 1, 1), (65, 12, 5, 28),
          (513, 64, 5, 28), (1030, 25, 5, 3), (4096, 25, 1, 1), (4096, 64, 1, 3)]


@pytest.mark.parametrize("N,K,B,A", SHAPES)
def test_prepare_and_chain_against_longdouble(N, K, B, A):
    inp, ref, M, status, (Wst, Wopt, ws_end) = _case(N, K, B, A)
    assert status.shape == (inp["V"], B) and not status.any()
    used = {(int(v), t) for v in inp["varm"] for t in range(B)}
    worst_m, orc_m = fo.check_m(ref, M.cpu().numpy(), used)
    worst_w, orc_w = fo.check_chain(ref, Wst.cpu().numpy(), Wopt.cpu().numpy())
    print(f"N={N} K={K} B={B} A={A}: M err/bound={worst_m:.3f} (oracle rel {orc_m:.2e})  "
          f"w err/bound={worst_w:.3f} (oracle rel {orc_w:.2e})")
    assert orc_m < 1e-13 and orc_w < 1e-13          # the inputs keep the oracle formula accurate
    assert worst_m <= 1.0 and worst_w <= 1.0


@pytest.mark.parametrize("N,K,B,A", [(65, 12, 5, 28), (513, 64, 5, 28), (2, 12, 5, 3)])
def test_drift_is_the_torch_expression(N, K, B, A):
    inp, _, _, _, (Wst, Wopt, ws_end) = _case(N, K, B, A)
    assert torch.equal(Wst[:, 0], _d(inp["ws0"]))
    grow, nmap, hit = _d(inp["grow"]), _d(inp["nmap"]), _d(inp["hit"])
    for t in range(B):
        nxt = Wst[:, t + 1] if t + 1 < B else ws_end
        assert torch.equal(nxt, fo.drift(Wopt[:, t], grow[t], nmap[t], hit[t])), t


@pytest.mark.parametrize("N,K,B", [(65, 12, 5), (513, 64, 5)])
def test_arm_is_bitwise_whatever_the_launch(N, K, B):
    """An arm alone (A = 1), third of three, and among 28: the same bits."""
    inp, _, M, _, (Wst, Wopt, ws_end) = _case(N, K, B, 28)
    for arm in (5, 6, 27):
        for arms, pos in (([arm], 0), ([1, 9, arm], 2)):
            got = _chain(inp, M, arms=arms)
            for g, r in zip(got, (Wst, Wopt, ws_end)):
                assert torch.equal(g[pos], r[arm]), (arm, arms)


def test_prepare_system_is_bitwise_whatever_the_launch():
    """A system's M does not depend on the other months or variants of the launch."""
    from pfml.ops import factor_solve as fs
    inp, _, M, _, _ = _case(513, 64, 5, 28)
    X = _table(inp["X"])
    for v, t in ((0, 0), (3, 2), (2, 4)):
        Ms, st = fs.factor_prepare(X, _d(inp["ridx"][t:t + 1]), _d(inp["F"][t:t + 1]),
                                   _d(inp["fscale"][v:v + 1]), _d(inp["d"][v:v + 1, t:t + 1]),
                                   _d(inp["n_rows"][t:t + 1]))
        assert torch.equal(Ms[0, 0], M[v, t]) and not st.any()


@pytest.mark.parametrize("Bp", [1, 2, 4])
def test_chain_prefix_is_the_shorter_chain(Bp):
    inp, _, M, _, (Wst, Wopt, _) = _case(513, 64, 5, 28)
    got = _chain(inp, M, months=Bp)
    assert torch.equal(got[0], Wst[:, :Bp]) and torch.equal(got[1], Wopt[:, :Bp])
    if Bp < 5:
        assert torch.equal(got[2], Wst[:, Bp])


def test_zero_c_arms_ignore_ws0():
    inp, _, M, _, (_, Wopt, _) = _case(65, 12, 5, 28)
    free = np.nonzero(~inp["c"].any(axis=(1, 2)))[0]
    assert len(free) >= 10
    rng = np.random.default_rng(0)
    got = _chain(inp, M, ws0=rng.standard_normal(inp["ws0"].shape))
    assert torch.equal(got[1][free], Wopt[free])
    tied = np.nonzero(inp["c"].any(axis=(1, 2)))[0]
    assert not torch.equal(got[1][tied], Wopt[tied])


def test_f_zero_is_exactly_b_over_d():
    inp, _, M, status, (Wst, Wopt, _) = _case(65, 12, 5, 8, f_zero=True)
    assert not status.any() and not M.any()
    live = _d(np.arange(65)[None, :] < inp["n_rows"][:, None])
    zero = torch.zeros((), dtype=torch.float64, device=GPU)
    for a in range(8):
        if inp["normalize"][a]:
            continue
        b = _d(inp["rhs"][a]) + _d(inp["c"][a]) * Wst[a]
        want = torch.where(live, b / _d(inp["d"][inp["varm"][a]]), zero)
        assert torch.equal(Wopt[a], want), a


def test_zeroed_factor():
    """F with a zero row and column (an exposure-less factor): no inverse of F is needed."""
    inp, ref, M, status, (Wst, Wopt, _) = _case(130, 25, 5, 4, zero=7)
    assert not status.any()
    assert not M[:, :, :, 7].any()                     # a zero right-hand side stays zero
    worst_m, _ = fo.check_m(ref, M.cpu().numpy())
    worst_w, orc_w = fo.check_chain(ref, Wst.cpu().numpy(), Wopt.cpu().numpy())
    print(f"zeroed factor: M err/bound={worst_m:.3f} w err/bound={worst_w:.3f}")
    assert orc_w < 1e-13 and worst_m <= 1.0 and worst_w <= 1.0


@pytest.mark.parametrize("N,K,B,A", [(2, 12, 5, 3), (65, 12, 5, 28), (513, 64, 5, 28),
                                     (4096, 64, 1, 3)])
def test_normalize_sums_to_one(N, K, B, A):
    inp, _, _, _, (_, Wopt, _) = _case(N, K, B, A)
    w = Wopt.cpu().numpy()
    arms = np.nonzero(inp["normalize"])[0]
    assert len(arms)
    for a in arms:
        for t in range(B):
            n = int(inp["n_rows"][t])
            off = abs(float(np.sum(w[a, t, :n].astype(fo.LD)) - 1))
            print(f"N={N} arm {a} month {t} n={n}: |sum - 1| = {off:.3e} ({off / fo.U:.2f} u)")
            assert off <= n * fo.U


def test_nan_stays_in_its_arm():
    inp, _, M, _, (Wst, Wopt, ws_end) = _case(65, 12, 5, 28)
    rhs = inp["rhs"].copy()
    assert inp["c"][9].any() and inp["n_rows"][2] > 3   # a Static-ML arm; column 3 is live
    rhs[9, 2, 3] = NAN
    got = _chain(inp, M, rhs=rhs)
    others = [a for a in range(28) if a != 9]
    for g, r in zip(got, (Wst, Wopt, ws_end)):
        assert torch.equal(g[others], r[others])
    assert torch.equal(got[1][9, :2], Wopt[9, :2]) and torch.isnan(got[1][9, 2]).any()


def test_status_flags():
    from pfml.ops import factor_solve as fs
    X = torch.eye(2, dtype=torch.float64, device=GPU)
    ridx = torch.arange(2, device=GPU)[None]
    one = torch.ones((1, 1, 2), dtype=torch.float64, device=GPU)
    args = (X, ridx, -torch.eye(2, dtype=torch.float64, device=GPU)[None],
            torch.ones(1, dtype=torch.float64, device=GPU))
    n = torch.tensor([2])
    _, st = fs.factor_prepare(*args, one, n)           # G = I, F = -I: I + F G = 0
    assert int(st[0, 0]) & fs.ST_ZERO_PIVOT
    _, st = fs.factor_prepare(*args, one * NAN, n)
    assert int(st[0, 0]) & fs.ST_NONFINITE
    _, st = fs.factor_prepare(*args, 3.0 * one, n)
    assert int(st[0, 0]) == 0


def test_limits_refuse_and_torch_serves():
    from pfml.ops import factor_solve as fs
    assert fs.max_n() == 4096 and fs.max_k() == 64
    wide = fo.factor_inputs(4097, 3, 1, 1, seed=11)
    M, status = _prepare(wide)
    with pytest.raises(ValueError):
        _chain(wide, M, fn=fs._launch_chain)
    Wst, Wopt, _ = _chain(wide, M)
    worst, orc = fo.check_chain(fo.Reference(wide), Wst.cpu().numpy(), Wopt.cpu().numpy())
    print(f"N=4097 (torch branch): w err/bound={worst:.3f}")
    assert worst <= 1.0 and orc < 1e-13
    deep = fo.factor_inputs(300, 65, 2, 3, seed=12)
    with pytest.raises(ValueError):
        _prepare(deep, fn=fs._launch_prepare)
    M, status = _prepare(deep)
    assert not status.any()
    with pytest.raises(ValueError):
        _chain(deep, M, fn=fs._launch_chain)
    Wst, Wopt, _ = _chain(deep, M)
    ref = fo.Reference(deep)
    worst_m, _ = fo.check_m(ref, M.cpu().numpy(), {(int(v), t) for v in deep["varm"]
                                                   for t in range(2)})
    worst, orc = fo.check_chain(ref, Wst.cpu().numpy(), Wopt.cpu().numpy())
    print(f"K=65 (torch branch): M err/bound={worst_m:.3f} w err/bound={worst:.3f}")
    assert worst_m <= 1.0 and worst <= 1.0 and orc < 1e-13


def test_empty_chain():
    inp = fo.factor_inputs(9, 3, 0, 3, seed=5)
    M, status = _prepare(inp)
    Wst, Wopt, ws_end = _chain(inp, M)
    assert M.shape == (4, 0, 3, 3) and status.shape == (4, 0)
    assert Wst.shape == (3, 0, 9) and Wopt.shape == (3, 0, 9)
    assert torch.equal(ws_end, _d(inp["ws0"]))
