"""The longdouble references of tests/test_gpu_stage_kernels.py (tests/oracle.py) checked against
the project's CPU paths - ``_chain`` on CPU tensors, the CPU branches of ``aim_portfolios``'
product, ``standardize_signals`` / ``signal_stats`` and ``validation_scores`` - so that the
references and the derived bounds are validated where no device exists."""
import numpy as np
import pytest
import torch

import oracle as orc
from oracle import U

CHAIN_NS = (1, 3, 4, 5, 63, 64, 65, 257, 511, 512, 513, 1030)


def _t(x):
    return None if x is None else torch.as_tensor(x)


def _chain_cpu(ops):
    from pfml.models.portfolio import _chain
    mt, a, wa, grow, nmap, hit, ws0 = (_t(x) for x in ops)
    return tuple(x.numpy() for x in _chain(mt, a, wa, grow, nmap, hit, ws0))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", CHAIN_NS)
def test_chain_reference_vs_cpu_chain(N, B):
    """The per-month checks (bitwise drift, one-step bound) hold for the CPU recursion."""
    ops = orc.chain_inputs(N, B, seed=100 * N + B)
    Wst, Wopt, ws = _chain_cpu(ops)
    assert np.abs(Wopt).max() < 0.1 and np.abs(Wst).max() < 0.1      # the chain does not grow
    assert orc.check_chain(ops, Wst, Wopt, ws) < 1.0


def test_chain_reference_vs_cpu_chain_lds_limit():
    """N = 4096 (the device kernel's LDS limit), B = 2."""
    ops = orc.chain_inputs(4096, 2, seed=4096)
    Wst, Wopt, ws = _chain_cpu(ops)
    assert np.abs(Wopt).max() < 0.1
    assert orc.check_chain(ops, Wst, Wopt, ws) < 1.0


@pytest.mark.parametrize("N", [3, 65, 513, 1030])
def test_chain_bound_is_sharp(N):
    """One dropped term M_ij d_j (what a wrong guard at one load would lose) breaks the
    one-step bound in every row, by orders of magnitude; so does a duplicated one (the same
    distance on the other side)."""
    mt, a, wa, grow, nmap, hit, ws0 = orc.chain_inputs(N, 1, seed=7 * N)
    ref, mag = orc.chain_step_ref(mt[0], a[0], wa[0], ws0)
    bound = orc.chain_step_bound(N, mag)
    for j in sorted({0, N // 2, N - 1, min(N - 1, 8 * 64), min(N - 1, 511)}):
        dropped, _ = orc.chain_step_ref(mt[0], a[0], wa[0], ws0, drop=j)
        over = np.abs(dropped - ref) / bound
        assert over.min() > 1.0, (j, float(over.min()))
        assert np.median(over) > 1e3, (j, float(np.median(over)))


def test_chain_check_rejects_wrong_outputs():
    """check_chain itself fails on a last-bits error of Wopt far below any tolerance one would
    tune by hand (1e-12 relative), and on a drift computed in another order."""
    ops = orc.chain_inputs(65, 3, seed=11)
    Wst, Wopt, ws = _chain_cpu(ops)
    bad = Wopt.copy()
    bad[2, np.abs(Wopt[2]).argmax()] *= 1 + 1e-12
    nmap, grow, hit = ops[4], ops[3], ops[5]
    ws_bad = (bad[2][nmap[2]] * grow[2][nmap[2]]) * hit[2]           # a consistent drift
    with pytest.raises(AssertionError, match="over the bound"):
        orc.check_chain(ops, Wst, bad, ws_bad)
    bad = Wst.copy()
    bad[1, 5] = np.nextafter(bad[1, 5], 1.0) if bad[1, 5] != 0 else 1e-300
    with pytest.raises(AssertionError):
        orc.check_chain(ops, bad, Wopt, ws)


def test_aim_reference_vs_cpu_product():
    """aim_ref against the CPU branch's product s[:, :nk] @ coef[:nk], within the bound."""
    rng = np.random.default_rng(5)
    for nrow, nk in ((1, 1), (3, 17), (5, 65), (50, 129), (513, 513)):
        s, c = rng.standard_normal((nrow, nk)), rng.standard_normal(nk)
        ref, mag = orc.aim_ref(s, c)
        got = (torch.as_tensor(s) @ torch.as_tensor(c)).numpy()
        assert np.all(np.abs(got - ref) <= 2.0 * (nk + 1) * U * mag)
        # a dropped last term is outside the bound
        short, _ = orc.aim_ref(s[:, :nk - 1], c[:nk - 1])
        assert np.all(np.abs(short - ref) > 2.0 * (nk + 1) * U * mag)


def _cpu_standardize(cs):
    from pfml.ops.panel import signal_stats, standardize_signals
    B, TH, N, P, Pw = cs["B"], cs["TH"], cs["N"], cs["P"], cs["Pw"]
    F, idx, mask, vol = _t(cs["F"]), _t(cs["idx"]), _t(cs["mask"]), _t(cs["vol"])
    out = standardize_signals(F, idx, mask, vol, P=P,
                              out=torch.empty((B, TH, N, Pw), dtype=torch.float64),
                              row_scale=_t(cs["row_scale"]))
    st = signal_stats(F, idx, mask, P, torch.empty((B, TH, 2, Pw), dtype=torch.float64))
    return out.numpy(), st.numpy()


def _two_pass_tol(cs, mean):
    """Bound of the CPU branch (raw mean, then centred squares; recursive summation at worst):
    the mean carries gamma_n max|x|, which enters relative to max|x - mean|; the norm and the
    element-wise operations add gamma_(n + 8)."""
    X = cs["F"][:, :cs["P"]][cs["idx"]]                      # [B, TH, N, P]
    live = cs["mask"].astype(bool)[:, None, :, None]
    ax = np.where(live, np.abs(X), 0.0).max(axis=2)
    dx = np.where(live, np.abs(X - mean[:, :, None].astype(np.float64)), 0.0).max(axis=2)
    n = cs["n_real"].reshape(-1, 1, 1)
    return float((2.0 * (n + 8) * U * (1.0 + ax / dx)).max())


@pytest.mark.parametrize("cs", orc.panel_cases(), ids=lambda c: "N{N}-P{P}-Pw{Pw}-B{B}x{TH}".format(**c))
def test_standardize_reference_vs_cpu_branch(cs):
    """standardize_ref against the CPU branches, and the sequential fp64 shifted-moment
    evaluation (the GPU tests' error yardstick) against standardize_ref."""
    case = orc.panel_case(**cs)
    _check_panel_refs(case)


@pytest.mark.parametrize("N", [40, 600])
def test_standardize_reference_offset_columns(N):
    case = orc.panel_case(N=N, P=33, Pw=34, B=2, TH=3, rs=True, k=77, offset=True)
    e_ref = _check_panel_refs(case)
    # the shifted moments are what keeps 1e6 + randn columns near 1e6 u: far below the raw
    # two-pass mean's n u 1e6
    assert e_ref < 64 * 1e6 * U


def _check_panel_refs(case):
    B, TH, N, P, Pw = case["B"], case["TH"], case["N"], case["P"], case["Pw"]
    ref, mean, scale = orc.standardize_ref(case["F"], case["idx"], case["n_real"], case["vol"],
                                           P, Pw, case["row_scale"])
    out, st = _cpu_standardize(case)
    tol = _two_pass_tol(case, mean)
    assert orc.col_err(out, ref) <= tol
    assert np.all(out[..., P:] == 0) and np.all(st[..., P:] == 0)
    # the stats imply the same block
    imp = orc.apply_stats_f64(case["F"], case["idx"], case["n_real"], case["vol"], P, Pw,
                              st[:, :, 0], st[:, :, 1], case["row_scale"])
    assert orc.col_err(imp, ref) <= tol
    # the yardstick: the kernels' formula, sequentially in fp64
    X = case["F"][:, :P][case["idx"]].reshape(B * TH, N, P)
    m64, s64 = orc.shifted_stats_f64(X, np.repeat(case["n_real"], TH))
    seq = orc.apply_stats_f64(case["F"], case["idx"], case["n_real"], case["vol"], P, Pw,
                              m64.reshape(B, TH, P), s64.reshape(B, TH, P), case["row_scale"])
    e_ref = orc.col_err(seq, ref)
    assert e_ref <= tol
    return e_ref


@pytest.mark.parametrize("P", [33, 65])
def test_excl_reference_vs_cpu_stats(P):
    """The longdouble statistics of 'U(d) minus the excluded rows' against the CPU
    signal_stats of the kept rows, and the fp64 difference form against both."""
    from pfml.ops.panel import signal_stats
    cs = orc.excl_case(P)
    F = cs["F"]
    for bt, rows in enumerate(cs["kept"]):
        n = len(rows)
        assert n == cs["n_real"][bt // cs["TH"]]
        mean, scale = orc.stats_ref(F[rows, :P])
        st = signal_stats(_t(np.nan_to_num(F)), _t(rows.reshape(1, 1, n)), torch.ones(1, n,
                          dtype=torch.float64), P, torch.empty((1, 1, 2, P), dtype=torch.float64))
        st = st.numpy()[0, 0]
        X = F[rows, :P]
        ref = (X - mean) * scale
        got = (X - st[0]) * st[1]
        ax, dx = np.abs(X).max(0), np.abs(X - mean.astype(np.float64)).max(0)
        tol = float((2.0 * (n + 8) * U * (1.0 + ax / dx)).max())
        assert orc.col_err(got, ref) <= tol
        d = cs["dpos"][bt]
        Xu = F[cs["urows"][d, :cs["un"][d]], :P][None]
        Xe = F[cs["erows"][bt], :P][None]
        m64, s64 = orc.shifted_stats_f64(Xu, [cs["un"][d]], np.nan_to_num(Xe), [cs["en"][bt]])
        # the difference form subtracts sums over U(d): its centred square sum carries the
        # rounding of sum_U (x - K)^2, i.e. a condition number sum_U (x - K)^2 / sum_kept
        # (x - mean)^2 (near 1 when few rows of many are excluded, as in the stage)
        su = ((Xu[0] - Xu[0, 0]) ** 2).sum(0)
        kappa = su / ((X - mean.astype(np.float64)) ** 2).sum(0)
        un = int(cs["un"][d])
        tol_d = float((2.0 * (un + 8) * U * (1.0 + ax / dx + 3.0 * kappa)).max())
        assert orc.col_err((X - m64[0]) * s64[0], ref) <= tol_d


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("shape", orc.SCORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scores_reference_vs_cpu_path(shape, compat):
    """cum_ref / dense_rank_ref against the CPU validation_scores at the production-like frames
    with NaN runs on chunk boundaries."""
    from pfml.models.search import validation_scores
    nV, G, nP, L, frame = shape
    obj = orc.scores_case(nV, G, nP, L, frame, compat)
    seq, k = orc.frame_rows(obj, frame, compat)
    ref = orc.cum_ref(seq)
    _, cum, rank = validation_scores(torch.as_tensor(obj), frame, compat)
    cum = cum.numpy().reshape(nV * k, -1)
    assert np.array_equal(np.isnan(cum), np.isnan(ref))
    assert np.isnan(ref[:, 4]).all() and np.isnan(ref[:25, 3]).all() and not np.isnan(ref[25, 3])
    fin = ~np.isnan(ref)
    assert np.all(np.abs(cum[fin] - ref[fin]) <= 1e-12 * np.abs(ref[fin]))
    rr = orc.dense_rank_ref(cum.reshape(nV, -1))
    assert np.array_equal(np.nan_to_num(rr, nan=-1.0),
                          np.nan_to_num(rank.numpy().reshape(nV, -1), nan=-1.0))
    # NaN rows repeat the previous mean in the reference by construction
    nanrow = np.isnan(seq)
    r, c = np.nonzero(nanrow[1:] & ~np.isnan(ref[:-1]))
    assert np.array_equal(ref[r + 1, c], ref[r, c])


def test_dense_rank_reference_small():
    v = np.array([[3.0, np.nan, 3.0, -np.inf, 0.0, -0.0, np.inf, 1.5]])
    assert np.array_equal(np.nan_to_num(orc.dense_rank_ref(v), nan=-1.0),
                          [[2.0, -1.0, 2.0, 5.0, 4.0, 4.0, 1.0, 3.0]])
