"""Risk kernels (csrc/risk.hip) against the longdouble oracle of tests/risk_oracle.py: every
factor width at which the 16 x 16 MFMA tiles, the rhs column or the LU / Jacobi loops change,
the chunk (64) and window edges, launch composition, stale outputs, empty launches and operand
layouts.  Inputs, references and tolerances are those tests/test_risk_oracle_cpu.py checks on
the CPU; nothing here widens them."""
import numpy as np
import pytest
import torch

import risk_oracle as ro
from risk_oracle import U

pytestmark = pytest.mark.gpu

COV_CASES = [(K, obs) for K in ro.COV_KS for obs in ro.COV_OBS]
VOL_CASES = [(s, lam) for s in ro.VOL_STARTS for lam in ro.VOL_LAMS]
SENTINEL = 7e300


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class _SentinelTorch:
    """``torch`` as pfml.ops.risk_kernels sees it, with every uninitialised floating buffer
    pre-filled with 7e300: an output element no kernel writes keeps that value."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _fill(t):
        return t.fill_(SENTINEL) if t.is_floating_point() else t

    def empty(self, *a, **k):
        return self._fill(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._fill(torch.empty_like(*a, **k))


@pytest.fixture
def sentinel(monkeypatch):
    from pfml.ops import risk_kernels as rk
    monkeypatch.setattr(rk, "torch", _SentinelTorch())
    probe = rk.torch.empty(3, dtype=torch.float64)
    assert (probe == SENTINEL).all()


def no_sentinel(*arrays):
    return all(not np.any(np.asarray(a) == SENTINEL) for a in arrays)


# ---------------------------------------------------------------------------------------------
# daily_ols
# ---------------------------------------------------------------------------------------------
def run_ols(gpu, X, y, off):
    from pfml.ops.risk_kernels import daily_ols
    X = X if isinstance(X, torch.Tensor) else torch.tensor(X, device=gpu)
    y = y if isinstance(y, torch.Tensor) else torch.tensor(y, device=gpu)
    coef, resid, nbad, st = daily_ols(X, y, torch.tensor(np.asarray(off, np.int64)),
                                      return_status=True)
    assert coef.device.type == resid.device.type == "cuda"
    return coef.cpu().numpy(), resid.cpu().numpy(), st.cpu().numpy(), nbad


_ols_batches = {}


def ols_batch(gpu, K):
    if K not in _ols_batches:
        ex = ro.ols_expect(K)
        _ols_batches[K] = run_ols(gpu, ex["X"], ex["y"], ex["off"])
    return _ols_batches[K]


@pytest.mark.parametrize("K", ro.OLS_KS)
def test_ols_against_oracle(gpu, K):
    """Compared days within tol_d with status 0; the duplicated-column and zero-column days
    within tol_d of the minimum-norm reference with status 2; the 0-row day exactly 0 with
    status 2; under-determined days finite; n_pinv the number of status-2 days; residuals are
    those of the stored coefficients."""
    ex = ro.ols_expect(K)
    coef, resid, st, nbad = ols_batch(gpu, K)
    worst = ro.ols_check(ex, coef, resid, st, nbad, "gpu")
    print(f"daily_ols K={K}: largest error / tol_d = {worst:.3g}")
    ro.ols_self_consistent(ex["X"], ex["y"], ex["off"], coef, resid)


@pytest.mark.parametrize("K", ro.OLS_KS)
def test_ols_day_alone_and_reversed_order_bitwise(gpu, K):
    ex = ro.ols_expect(K)
    X, y, off = ex["X"], ex["y"], ex["off"]
    coef, resid, st, _ = ols_batch(gpu, K)
    D = len(off) - 1
    for d in range(D):
        a, b = int(off[d]), int(off[d + 1])
        c1, r1, s1, n1 = run_ols(gpu, X[a:b], y[a:b], [0, b - a])
        assert same_bits(c1[0], coef[d]) and same_bits(r1, resid[a:b]), (K, d)
        assert s1[0] == st[d] and n1 == int(st[d] == 2), (K, d)
    order = list(range(D))[::-1]
    Xr = np.concatenate([X[off[d]:off[d + 1]] for d in order])
    yr = np.concatenate([y[off[d]:off[d + 1]] for d in order])
    offr = np.r_[0, np.cumsum([off[d + 1] - off[d] for d in order])]
    c2, r2, s2, _ = run_ols(gpu, Xr, yr, offr)
    assert same_bits(c2[::-1], coef) and np.array_equal(s2[::-1], st)
    for i, d in enumerate(order):
        assert same_bits(r2[offr[i]:offr[i + 1]], resid[off[d]:off[d + 1]]), (K, d)


@pytest.mark.parametrize("K", [1, 16, 31])
def test_ols_every_output_written(gpu, sentinel, K):
    ex = ro.ols_expect(K)
    coef, resid, st, _ = run_ols(gpu, ex["X"], ex["y"], ex["off"])
    assert no_sentinel(coef, resid)
    ref = ols_batch(gpu, K)
    assert same_bits(coef, ref[0]) and same_bits(resid, ref[1]) and np.array_equal(st, ref[2])


@pytest.mark.parametrize("K", [2, 17])
def test_ols_fp32_and_strided_operands(gpu, K):
    ex = ro.ols_expect(K)
    X32, y32, off = ex["X"].astype(np.float32), ex["y"].astype(np.float32), ex["off"]
    base = run_ols(gpu, X32.astype(np.float64), y32.astype(np.float64), off)
    got = run_ols(gpu, torch.tensor(X32, device=gpu), torch.tensor(y32, device=gpu), off)
    assert all(same_bits(g, b) for g, b in zip(got[:3], base[:3]))
    wide = np.full((X32.shape[0], 2 * K), 3.0)
    wide[:, ::2] = X32
    wy = np.full(2 * len(y32), 5.0)
    wy[::2] = y32
    Xv, yv = torch.tensor(wide, device=gpu)[:, ::2], torch.tensor(wy, device=gpu)[::2]
    assert not Xv.is_contiguous() and not yv.is_contiguous()
    got = run_ols(gpu, Xv, yv, off)
    assert all(same_bits(g, b) for g, b in zip(got[:3], base[:3]))


def test_ols_empty_launches(gpu):
    coef, resid, st, nbad = run_ols(gpu, np.zeros((0, 7)), np.zeros(0), [0])
    assert coef.shape == (0, 7) and resid.shape == (0,) and st.shape == (0,) and nbad == 0
    assert coef.dtype == resid.dtype == np.float64 and st.dtype == np.int32
    # days without rows only
    coef, resid, st, nbad = run_ols(gpu, np.zeros((0, 7)), np.zeros(0), [0, 0, 0])
    assert coef.shape == (2, 7) and np.all(coef == 0) and nbad == 2 and np.all(st == 2)


# ---------------------------------------------------------------------------------------------
# ewma_factor_cov
# ---------------------------------------------------------------------------------------------
def run_cov(gpu, ex, ends=None, fr=None, parts=True, sync=True):
    from pfml.ops.risk_kernels import ewma_factor_cov
    fr = torch.tensor(ex["fr"], device=gpu) if fr is None else fr
    out = ewma_factor_cov(fr, ex["ends"] if ends is None else ends, ex["obs"], ex["w_cor"],
                          ex["w_var"], scale=ex["scale"], return_parts=parts)
    out = out if parts else (out,)
    assert all(t.device.type == "cuda" and t.dtype == torch.float64 for t in out)
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("K,obs", COV_CASES)
def test_cov_against_oracle(gpu, K, obs):
    """F, cor and var of every window within panel_tol of the longdouble cov.wt.  F carries the
    same bits with and without ``return_parts``.  cor and var are symmetric to the bit (each
    entry and its mirror are the same products summed in the same order, in two tiles).  F is
    not symmetric by construction: ((sd_i cor) sd_j) scale and ((sd_j cor) sd_i) scale round
    differently, three roundings each of one exact product, so |F - F'| <= 8 u |F|.  The
    diagonal of cor is exactly 1."""
    ex = ro.cov_expect(K, obs)
    F, cor, var = run_cov(gpu, ex)
    worst = ro.cov_check(ex, F, cor, var, "gpu")
    print(f"ewma_factor_cov K={K} obs={obs}: largest error / tol = {worst:.3g}")
    (F1,) = run_cov(gpu, ex, parts=False)
    assert same_bits(F1, F)
    assert same_bits(cor, cor.transpose(0, 2, 1)) and same_bits(var, var.transpose(0, 2, 1))
    assert np.all(np.abs(F - F.transpose(0, 2, 1)) <= 8 * U * np.abs(F))
    assert np.all(np.diagonal(cor, axis1=1, axis2=2) == 1.0)


@pytest.mark.parametrize("K,obs", [(1, 64), (17, 64), (32, 300)])
def test_cov_month_alone_and_at_any_position_bitwise(gpu, K, obs):
    ex = ro.cov_expect(K, obs)
    fr = torch.tensor(ex["fr"], device=gpu)
    base = run_cov(gpu, ex, fr=fr)
    ends = ex["ends"]
    for b, e in enumerate(ends):
        one = run_cov(gpu, ex, ends=[int(e)], fr=fr)
        assert all(same_bits(o[0], f[b]) for o, f in zip(one, base)), (K, obs, int(e))
    perm = np.random.default_rng(5).permutation(len(ends))
    moved = run_cov(gpu, ex, ends=np.r_[ends[perm], ends[perm[:3]]], fr=fr)
    for m, f in zip(moved, base):
        assert same_bits(m[:len(ends)], f[perm]) and same_bits(m[len(ends):], f[perm[:3]])


def test_cov_one_day_window_is_nan_like_the_cpu_branch(gpu):
    """ends = 1: one weight, 1 - sum w^2 = 0, so cov.wt is 0 / 0: F and var NaN, cor NaN off the
    diagonal, on both branches; the neighbouring month is untouched."""
    from pfml.ops.risk_kernels import ewma_factor_cov
    ex = ro.cov_expect(17, 64)
    ends = [64, 1, 65]
    got = run_cov(gpu, ex, ends=ends)
    cpu = ewma_factor_cov(torch.tensor(ex["fr"]), ends, 64, ex["w_cor"], ex["w_var"],
                          return_parts=True)
    for g, c in zip(got, cpu):
        assert np.array_equal(np.isnan(g), np.isnan(c.numpy()))
    F, cor, var = got
    assert np.isnan(F[1]).all() and np.isnan(var[1]).all()
    assert np.all(np.diagonal(cor[1]) == 1.0)
    assert np.isnan(cor[1][~np.eye(17, dtype=bool)]).all()
    base = run_cov(gpu, ex)
    k64, k65 = list(ex["ends"]).index(64), list(ex["ends"]).index(65)
    assert all(same_bits(g[0], b[k64]) and same_bits(g[2], b[k65]) for g, b in zip(got, base))


@pytest.mark.parametrize("K,obs", [(2, 64), (25, 300)])
def test_cov_every_output_written(gpu, sentinel, K, obs):
    ex = ro.cov_expect(K, obs)
    got = run_cov(gpu, ex)
    assert no_sentinel(*got)
    (F,) = run_cov(gpu, ex, parts=False)
    assert no_sentinel(F) and same_bits(F, got[0])


def test_cov_fp32_and_strided_operands(gpu):
    ex = ro.cov_expect(17, 64)
    f32 = ex["fr"].astype(np.float32)
    base = run_cov(gpu, ex, fr=torch.tensor(f32.astype(np.float64), device=gpu))
    got = run_cov(gpu, ex, fr=torch.tensor(f32, device=gpu))
    assert all(same_bits(g, b) for g, b in zip(got, base))
    wide = np.full((f32.shape[0], 34), 3.0)
    wide[:, ::2] = f32
    view = torch.tensor(wide, device=gpu)[:, ::2]
    assert not view.is_contiguous()
    got = run_cov(gpu, ex, fr=view)
    assert all(same_bits(g, b) for g, b in zip(got, base))


@pytest.mark.parametrize("K", [5, 33])
def test_cov_empty_launch(gpu, K):
    ex = dict(ro.cov_case(2, 64), fr=np.zeros((134, K)))
    for parts in (False, True):
        out = run_cov(gpu, ex, ends=[], parts=parts)       # run_cov asserts device and dtype
        assert len(out) == (3 if parts else 1) and all(t.shape == (0, K, K) for t in out)


def test_cov_wider_than_the_kernel_takes_the_torch_branch(gpu):
    """K = 33 on the device: the torch branch, on the device, within panel_tol of the oracle
    (e_ref: the same branch on the CPU)."""
    from pfml.ops.risk_kernels import ewma_factor_cov
    rng = np.random.default_rng(733)
    c = dict(ro.cov_case(2, 64), fr=rng.standard_normal((134, 33)) * 0.01 + 0.001,
             ends=np.array([64, 134], np.int64), K=33)
    ref = ro.cov_ref(c["fr"], c["ends"], 64, c["w_cor"], c["w_var"], c["scale"])
    cpu = ewma_factor_cov(torch.tensor(c["fr"]), c["ends"], 64, c["w_cor"], c["w_var"],
                          return_parts=True)
    e_ref = ro.cov_errs(*(t.numpy() for t in cpu), ref)
    ex = dict(c, ref=ref, tol=np.vectorize(ro.panel_tol)(e_ref))
    assert ex["tol"].max() <= 1e-13
    ro.cov_check(ex, *run_cov(gpu, ex), "gpu torch branch")


# ---------------------------------------------------------------------------------------------
# ewma_vol
# ---------------------------------------------------------------------------------------------
def run_vol(gpu, x, gs, lam, start):
    from pfml.ops.risk_kernels import ewma_vol
    x = x if isinstance(x, torch.Tensor) else torch.tensor(x, device=gpu)
    out = ewma_vol(x, gs, lam, start)
    assert out.device.type == "cuda" and out.dtype == torch.float64
    return out.cpu().numpy()


@pytest.mark.parametrize("start,lam", VOL_CASES)
def test_vol_against_oracle(gpu, start, lam):
    ex = ro.vol_expect(start, lam)
    out = run_vol(gpu, ex["x"], ex["gs"], lam, start)
    err = ro.vol_err(out, ex["ref"])                       # asserts equal NaN masks
    print(f"ewma_vol start={start} lam={lam:.4f}: error {err / U:.1f} u, tol {ex['tol'] / U:.1f} u")
    assert err <= ex["tol"], (err, ex["tol"])
    dev = run_vol(gpu, ex["x"], torch.tensor(ex["gs"], device=gpu), lam, start)
    assert same_bits(dev, out)


@pytest.mark.parametrize("start,lam", VOL_CASES)
def test_vol_group_is_independent_of_its_wave(gpu, start, lam):
    """Each group alone, and as the p-th of four groups (wave p of the workgroup), carries the
    bits it has in the 13-group launch."""
    ex = ro.vol_expect(start, lam)
    x, gs = ex["x"], ex["gs"]
    base = run_vol(gpu, x, gs, lam, start)
    fill = x[gs[5]:gs[6]]
    for g in range(len(gs) - 1):
        xg = x[gs[g]:gs[g + 1]]
        want = base[gs[g]:gs[g + 1]]
        assert same_bits(run_vol(gpu, xg, [0, len(xg)], lam, start), want), (g, "alone")
        for p in range(4):
            parts = [fill] * p + [xg] + [fill] * (3 - p)
            o = np.r_[0, np.cumsum([len(q) for q in parts])]
            out = run_vol(gpu, np.concatenate(parts), o, lam, start)
            assert same_bits(out[o[p]:o[p + 1]], want), (g, p)


@pytest.mark.parametrize("start", ro.VOL_STARTS)
def test_vol_every_output_written(gpu, sentinel, start):
    ex = ro.vol_expect(start, ro.VOL_LAMS[0])
    out = run_vol(gpu, ex["x"], ex["gs"], ex["lam"], start)
    assert no_sentinel(out)
    assert np.array_equal(np.isnan(out), np.isnan(ex["ref"]))


def test_vol_fp32_and_strided_operands(gpu):
    ex = ro.vol_expect(65, 0.97)
    x32 = ex["x"].astype(np.float32)
    base = run_vol(gpu, x32.astype(np.float64), ex["gs"], 0.97, 65)
    assert same_bits(run_vol(gpu, torch.tensor(x32, device=gpu), ex["gs"], 0.97, 65), base)
    wide = np.full(2 * len(x32), 3.0)
    wide[::2] = x32
    view = torch.tensor(wide, device=gpu)[::2]
    assert not view.is_contiguous()
    assert same_bits(run_vol(gpu, view, ex["gs"], 0.97, 65), base)


def test_vol_empty_launches(gpu):
    out = run_vol(gpu, np.zeros(0), np.zeros(1, np.int64), 0.97, 5)
    assert out.shape == (0,)
    out = run_vol(gpu, np.zeros(0), np.zeros(4, np.int64), 0.97, 5)       # zero-length groups
    assert out.shape == (0,)
