"""The Multiperiod-ML kernels (csrc/multiperiod.hip through pfml.ops.multiperiod) against the
longdouble references of tests/mp_oracle.py at the widths where their loops change shape, their
bitwise properties (a month's V independent of the launch, an arm independent of the other
arms, chain prefixes, NaN isolation, padding, sentinels), the torch branch beyond the kernels'
width, and the ``pfml-mp`` stage on the device against its CPU run and end to end."""
import functools
import os
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

import mp_oracle as mpo

pytestmark = pytest.mark.gpu

NAN = float("nan")
KS = (1, 2, 3, 12)
STAT = ["inv", "shorting", "turnover", "r", "tc"]
YEARS = ["pf.dates.start_year=2008", "pf.dates.end_yr=2012", "pf.dates.split_years=1",
         "pf_ml.p_vec=[16,32]"]
MP = ["mp.K=3", "mp.p_vec=[16]", "mp.u=[1,0.5,0.25]"]
TOL = dict(rtol=1e-8, atol=1e-12)      # device against CPU, as test_gpu_benchmarks.py


def _d(x, gpu):
    return torch.as_tensor(x).to(gpu)


def _cap(N):
    from pfml.ops import multiperiod as mp
    return mp.max_arms(N)


@functools.lru_cache(maxsize=None)
def _inputs(N, B, K, A, ragged=True):
    return mpo.mp_inputs(N, B, K, A, seed=1000 * N + 10 * B + K, ragged=ragged)


def _fold(inp, gpu, K=None, gbar=1.0, months=None, strided=False, mu=None):
    from pfml.ops.multiperiod import horizon_fold
    sel = slice(None) if months is None else list(months)
    mt = _d(inp["mt"][sel], gpu)
    if strided:
        Bs, N = mt.shape[:2]
        buf = torch.full((Bs, N + 7, N + 9), NAN, dtype=torch.float64, device=gpu)
        buf[:, :N, :N] = mt
        mt = buf[:, :N, :N]
        assert not mt.is_contiguous() or N == 1
    mu = inp["mu"] if mu is None else mu
    V = horizon_fold(mt, _d(inp["a"][sel], gpu), _d(mu[:K, sel], gpu),
                     _d(inp["wealth"][sel], gpu), _d(inp["n_rows"][sel], gpu), gbar)
    torch.cuda.synchronize()
    return V


def _chain(inp, V, gpu, arms=None, B=None, ws0=None, strided=False):
    from pfml.ops.multiperiod import mp_chain
    arms = list(range(inp["A"])) if arms is None else list(arms)
    b = slice(0, inp["B"] if B is None else B)
    mt = _d(inp["mt"][b], gpu)
    if strided:
        Bs, N = mt.shape[:2]
        buf = torch.full((Bs, N + 7, N + 9), NAN, dtype=torch.float64, device=gpu)
        buf[:, :N, :N] = mt
        mt = buf[:, :N, :N]
    ws0 = inp["ws0"][arms] if ws0 is None else ws0
    out = mp_chain(mt, _d(inp["a"][b], gpu), V[b], _d(inp["u"][arms], gpu),
                   _d(inp["n_rows"][b], gpu), _d(inp["grow"][b], gpu), _d(inp["nmap"][b], gpu),
                   _d(inp["hit"][b], gpu), _d(ws0, gpu))
    torch.cuda.synchronize()
    return out


def _np(xs):
    return tuple(x.cpu().numpy() for x in xs)


# ---------------------------------------------------------------------------------------------
# the fold
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 127, 512, 513, 1030])
def test_fold_within_the_oracle_bound(gpu, N, B):
    """K = 1, 2, 3, 12 with n_rows out of {N, 0, 1, N - 5}: |V - V_ld| <= 8 x (error of the
    sequential-fp64 formula) + (n + K) u max|V_ld| in every month, padding 0."""
    inp = _inputs(N, B, 12, 1)
    assert B == 1 or set(inp["n_rows"].tolist()) == {N, 0, min(1, N), max(N - 5, 0)}
    for K in KS:
        sub = dict(inp, mu=inp["mu"][:K])
        V = _fold(inp, gpu, K=K).cpu().numpy()
        worst = mpo.check_fold(sub, V, 1.0)
        print(f"fold N={N} B={B} K={K}: worst error / bound = {worst:.3e}")
    V = _fold(inp, gpu, K=3, gbar=0.7).cpu().numpy()
    mpo.check_fold(dict(inp, mu=inp["mu"][:3]), V, 0.7)


def test_fold_at_the_kernel_width(gpu):
    inp = _inputs(4096, 1, 3, 3, ragged=False)
    V = _fold(inp, gpu).cpu().numpy()
    print("fold N=4096 K=3: worst error / bound =", mpo.check_fold(inp, V, 1.0))


@pytest.mark.parametrize("N", [65, 513])
def test_fold_strided_view_in_a_nan_buffer(gpu, N):
    inp = _inputs(N, 5, 12, 1)
    for K in (2, 12):
        V = _fold(inp, gpu, K=K)
        Vs = _fold(inp, gpu, K=K, strided=True)
        assert torch.isfinite(Vs).all() and torch.equal(V, Vs)


def test_fold_k1_and_gbar0_are_the_first_horizon(gpu):
    inp = _inputs(127, 5, 12, 1)
    a, W, n = _d(inp["a"], gpu), _d(inp["wealth"], gpu), inp["n_rows"]
    live = _d(np.arange(127)[None, :] < n[:, None], gpu)
    want = torch.where(live, (a * _d(inp["mu"][0], gpu)) / W[:, None],
                       torch.zeros((), dtype=torch.float64, device=gpu))
    assert torch.equal(_fold(inp, gpu, K=1), want)
    assert torch.equal(_fold(inp, gpu, K=12, gbar=0.0), want)


def test_month_bits_do_not_depend_on_the_launch(gpu):
    """A month's V alone (B = 1), in a reversed launch and in the full launch: torch.equal."""
    N, B = 513, 5
    inp = _inputs(N, B, 12, 1)
    full = _fold(inp, gpu, K=12)
    rev = _fold(inp, gpu, K=12, months=range(B - 1, -1, -1))
    assert torch.equal(rev.flip(0), full)
    for t in (0, 3, 4):
        assert torch.equal(_fold(inp, gpu, K=12, months=[t])[0], full[t])


def test_nan_mu_stays_in_its_month(gpu):
    N, B = 513, 5
    inp = _inputs(N, B, 12, 1)
    ref = _fold(inp, gpu, K=3)
    mu = inp["mu"].copy()
    mu[2, 4, 17] = np.nan
    got = _fold(inp, gpu, K=3, mu=mu)
    assert torch.equal(got[:4], ref[:4])
    assert torch.isnan(got[4]).any()


# ---------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 127, 512, 513, 1030])
def test_chain_within_the_oracle_bound_for_every_arm_count(gpu, N, B):
    """A = cap + 1 arms (two launch chains: the host chunks) checked month by month against the
    longdouble step from the device's own w_start; then A = 1, 3 and cap: every column
    torch.equal to its column of the cap + 1 run."""
    cap = _cap(N)
    assert cap == min(16, 8192 // N)
    inp = _inputs(N, B, 2, cap + 1)
    V = _fold(inp, gpu)
    ref = _chain(inp, V, gpu)
    worst = mpo.check_chain(inp, V.cpu().numpy(), *_np(ref))
    print(f"chain N={N} B={B} A={cap + 1}: worst error / bound = {worst:.3e}")
    for A in (1, 3, cap):
        got = _chain(inp, V, gpu, arms=range(A))
        for g, r in zip(got, ref):
            assert torch.equal(g, r[:A])


def test_chain_at_the_kernel_width(gpu):
    N = 4096
    assert _cap(N) == 2 and _cap(4097) == 0
    inp = _inputs(N, 1, 3, 3, ragged=False)
    V = _fold(inp, gpu)
    out = _chain(inp, V, gpu)
    print("chain N=4096 A=3: worst error / bound =",
          mpo.check_chain(inp, V.cpu().numpy(), *_np(out)))


def test_arm_bits_do_not_depend_on_A_or_position(gpu):
    N, B = 513, 5
    cap = _cap(N)
    inp = _inputs(N, B, 2, cap + 1)
    V = _fold(inp, gpu)
    ref = _chain(inp, V, gpu)
    k = 5
    two = _chain(inp, V, gpu, arms=[k, 0])
    order = [c for c in range(cap + 1) if c != k]
    order.insert(13, k)
    many = _chain(inp, V, gpu, arms=order)
    for t, s, r in zip(two, many, ref):
        assert torch.equal(t[0], r[k]) and torch.equal(s[13], r[k]) and torch.equal(t[1], r[0])


def test_chain_prefixes_and_broadcast_ws0(gpu):
    N, B = 65, 5
    inp = _inputs(N, B, 2, 17)
    V = _fold(inp, gpu)
    full = _chain(inp, V, gpu, arms=range(3))
    for Bp in (1, 2, 4):
        Wst, Wopt, ws = _chain(inp, V, gpu, arms=range(3), B=Bp)
        assert torch.equal(Wst, full[0][:, :Bp]) and torch.equal(Wopt, full[1][:, :Bp])
        assert torch.equal(ws, full[0][:, Bp])
    one = _chain(inp, V, gpu, arms=[0, 1], ws0=inp["ws0"][0])
    both = _chain(inp, V, gpu, arms=[0, 1], ws0=np.stack([inp["ws0"][0]] * 2))
    for a, b in zip(one, both):
        assert torch.equal(a, b)
    assert torch.equal(one[0][0], full[0][0])


@pytest.mark.parametrize("N", [65, 513])
def test_chain_strided_view_in_a_nan_buffer(gpu, N):
    inp = _inputs(N, 5, 2, _cap(N) + 1)
    V = _fold(inp, gpu)
    ref = _chain(inp, V, gpu, arms=range(3))
    got = _chain(inp, V, gpu, arms=range(3), strided=True)
    assert all(torch.isfinite(g).all() for g in got)
    for g, r in zip(got, ref):
        assert torch.equal(g, r)


def test_nan_ws0_stays_in_its_arm(gpu):
    N, B = 513, 5
    inp = _inputs(N, B, 2, _cap(N) + 1)
    V = _fold(inp, gpu)
    ref = _chain(inp, V, gpu)
    ws0 = inp["ws0"].copy()
    ws0[3, 17] = np.nan
    got = _chain(inp, V, gpu, ws0=ws0)
    keep = [k for k in range(inp["A"]) if k != 3]
    for g, r in zip(got, ref):
        assert torch.equal(g[keep], r[keep])
    assert torch.isnan(got[1][3, 0]).any()


def test_sentinel_outputs_are_overwritten(gpu):
    """The launchers called on outputs filled with 1e300: live entries are the wrappers'
    results, padding entries of V and w_opt are 0, w_start is written in all N columns."""
    from pfml.ops import _native as nat
    from pfml.ops import multiperiod as mp
    N, B, K, A = 127, 5, 3, 3
    inp = _inputs(N, B, 12, 1)
    arm = mpo.mp_inputs(N, B, 2, A, seed=9)
    inp = dict(inp, ws0=arm["ws0"], u=arm["u"], A=A)
    V_ref = _fold(inp, gpu, K=K)
    ref = _chain(inp, V_ref, gpu)
    lib = nat.hip_lib()
    mt, a, mu = _d(inp["mt"], gpu), _d(inp["a"], gpu), _d(inp["mu"][:K].copy(), gpu)
    W, nr = _d(inp["wealth"], gpu), _d(inp["n_rows"], gpu).to(torch.int32)
    full = lambda *s: torch.full(s, 1e300, dtype=torch.float64, device=gpu)   # noqa: E731
    V = full(B, N)
    st = nat.stream_of(mt)
    nat.check(lib.pfml_mp_fold(mt.data_ptr(), N, N * N, a.data_ptr(), mu.data_ptr(), B * N,
                               W.data_ptr(), nr.data_ptr(), N, 1.0, K, B, N, V.data_ptr(), st),
              "pfml_mp_fold")
    Wst, Wopt, ws = full(A, B, N), full(A, B, N), full(A, N)
    grow, nmap, hit = (_d(inp[k], gpu) for k in ("grow", "nmap", "hit"))
    ws0, u = _d(inp["ws0"], gpu), _d(inp["u"], gpu)
    nat.check(lib.pfml_mp_chain(mt.data_ptr(), N, N * N, a.data_ptr(), V.data_ptr(),
                                u.data_ptr(), nr.data_ptr(), grow.data_ptr(), nmap.data_ptr(),
                                hit.data_ptr(), N, ws0.data_ptr(), N, B, N, A, Wst.data_ptr(),
                                Wopt.data_ptr(), B * N, ws.data_ptr(), st), "pfml_mp_chain")
    torch.cuda.synchronize()
    assert torch.equal(V, V_ref)
    for g, r in zip((Wst, Wopt, ws), ref):
        assert torch.equal(g, r)
    assert mp.max_n() == 4096
    # the launchers refuse what is beyond them before any launch (hipErrorInvalidValue)
    p = V.data_ptr()
    assert lib.pfml_mp_fold(p, 4097, 4097 * 4097, p, p, 4097, p, p, 4097, 1.0, 2, 1, 4097, p,
                            st) == 1
    assert lib.pfml_mp_chain(p, N, N * N, p, p, p, p, p, p, p, N, p, 0, 1, N, _cap(N) + 1, p, p,
                             N, p, st) == 1


def test_empty_launches(gpu):
    from pfml.ops.multiperiod import horizon_fold, mp_chain
    N, A = 65, 3
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=gpu)     # noqa: E731
    V = horizon_fold(z(0, N, N), z(0, N), z(2, 0, N), z(0), z(0, dt=torch.int32))
    assert V.shape == (0, N)
    ws0 = torch.arange(A * N, dtype=torch.float64, device=gpu).view(A, N)
    Wst, Wopt, ws = mp_chain(z(0, N, N), z(0, N), V, [1.0, 0.5, 2.0], z(0, dt=torch.int32),
                             z(0, N), z(0, N, dt=torch.int64), z(0, N), ws0)
    assert Wst.shape == (A, 0, N) and Wopt.shape == (A, 0, N) and torch.equal(ws, ws0)
    assert torch.equal(mp_chain(z(0, N, N), z(0, N), V, [1.0], z(0, dt=torch.int32), z(0, N),
                                z(0, N, dt=torch.int64), z(0, N), ws0[0])[2], ws0[:1])


def test_above_the_kernel_width_takes_the_torch_branch(gpu):
    """N = 4097 on the device: the plain torch loop, inside the same bounds."""
    inp = _inputs(4097, 1, 2, 2, ragged=False)
    V = _fold(inp, gpu)
    mpo.check_fold(inp, V.cpu().numpy(), 1.0)
    out = _chain(inp, V, gpu)
    mpo.check_chain(inp, V.cpu().numpy(), *_np(out))


# ---------------------------------------------------------------------------------------------
# the stage
# ---------------------------------------------------------------------------------------------
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
    cfg = small_data.override(YEARS + MP)
    cfg.run.compat_mode = False
    return dict(cfg=cfg, data=_load(cfg))


@pytest.fixture(scope="module")
def device_run(case):
    from pfml.models import multiperiod
    return multiperiod.multiperiod_portfolios(case["cfg"], *case["data"],
                                              torch.device("cuda", 0), keep_weights=True)


def test_device_matches_the_cpu_run(case, device_run):
    from pfml.models import frontier, multiperiod
    cpu = multiperiod.multiperiod_portfolios(case["cfg"], *case["data"], "cpu",
                                             keep_weights=True)
    dev = device_run
    for c in ("type", "n", "reason"):
        assert list(dev["mp"][c]) == list(cpu["mp"][c]), c
    assert list(dev["mp"]["type"]) == ["Portfolio-ML", "Multiperiod-ML", "Multiperiod-ML(0.5)",
                                       "Multiperiod-ML(0.25)"]
    assert (dev["mp"]["reason"] == "").all()
    assert dev["chosen"] == cpu["chosen"] and dev["chosen_mp"] == cpu["chosen_mp"]
    assert dev["missing_mu"] == cpu["missing_mu"]
    print("max |device - cpu| of mu_hat:", float(np.abs(dev["mu_hat"] - cpu["mu_hat"]).max()))
    assert np.allclose(dev["mu_hat"], cpu["mu_hat"], **TOL)
    num = [c for c in frontier.SUMMARY_COLUMNS if c not in ("type", "n")]
    err = np.abs(dev["pf"][STAT].to_numpy() - cpu["pf"][STAT].to_numpy())
    print("max |device - cpu| of the monthly statistics:", float(err.max()))
    assert list(dev["pf"]["type"]) == list(cpu["pf"]["type"])
    assert np.allclose(dev["pf"][STAT].to_numpy(), cpu["pf"][STAT].to_numpy(), **TOL)
    assert np.allclose(dev["mp"][num].to_numpy(float), cpu["mp"][num].to_numpy(float), **TOL)
    assert np.allclose(dev["hps"]["val_mse"], cpu["hps"]["val_mse"], **TOL)
    for name, w in dev["weights"].items():
        assert np.allclose(w["w"], cpu["weights"][name]["w"], equal_nan=True, **TOL), name
    assert dev["mp"]["obj"].nunique() == len(dev["mp"])


def test_portfolio_ml_row_is_backtest_device(gpu, case, device_run):
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
    d = str(tmp_path / "data_mp")
    shutil.copytree(small_data.run.data_dir, d)
    cfg = small_data.override(YEARS + MP + ["run.plots=False", f"run.data_dir={d}",
                                            f"run.artifact_dir={tmp_path}/art"])
    cfg.run.compat_mode = False
    Pipeline(cfg, device=gpu.type).run(["pfml-mp"])
    mp = pd.read_csv(os.path.join(d, "mp.csv"), keep_default_na=False, na_values=["nan", "NaN"])
    pf = pd.read_csv(os.path.join(d, "mp_pf.csv"), parse_dates=["eom_ret"])
    hps = pd.read_csv(os.path.join(d, "mp_hps.csv"))
    assert list(mp.columns) == CSV_COLUMNS["mp.csv"]
    assert list(pf.columns) == CSV_COLUMNS["mp_pf.csv"]
    assert list(hps.columns) == CSV_COLUMNS["mp_hps.csv"]
    ref = device_run["mp"]
    assert list(mp["type"]) == list(ref["type"])
    assert len(pf) == len(mp) * len(device_run["months"])
    assert sorted(set(hps["horizon"])) == [1, 2, 3]
    num = ["r", "sd", "tc", "r_tc", "sr", "obj"]
    assert np.isfinite(mp[num].to_numpy(float)).all()
    assert np.allclose(mp[num].to_numpy(float), ref[num].to_numpy(float), **TOL)
    assert np.allclose(hps["val_mse"], device_run["hps"]["val_mse"], **TOL)
