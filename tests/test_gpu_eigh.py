"""The device eigensolver (csrc/eigh_jacobi.hip, ``ops.linalg.eigh_psd``), the eigen form of
m_tilde_0 and the m_func repair that uses it.

Bounds of the decomposition, per matrix, against the input itself and LAPACK on the CPU
(u = 2^-53):  max|A V - V E| <= 4 N u |A|_2,  max|V'V - I| <= 15.726 N u,  sorted eigenvalues
within 5.832 N u |A|_2.  They come from the sequential numpy model of the same algorithm
(tests/jacobi_ref.py; profiles/r12_eigh_jacobi.md) - never from the kernel's own output: 4, 8
and 4 were set as multiples of the model's figures at N <= 128; at N = 496 the model measures
0.361, 5.242 and 1.944, the last two above a third of their bound, so those two are 3 x the
model's N = 496 value."""
import functools

import numpy as np
import pytest
import torch

import jacobi_ref as jr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RESID_MAX, ORTH_MAX, EIG_MAX = 4.0, 3 * 5.242, 3 * 1.944
SHAPES = [1, 2, 7, 16, 17, 40, 100, 129, 496, 576, 577]


@functools.lru_cache(maxsize=None)
def _batch(N: int):
    """The three spectra of one test batch [3, N, N] (wealth 1, wealth 1e10, a Gram matrix of
    rank N / 2) and LAPACK's ascending eigenvalues and eigenvectors, computed once per N."""
    A = torch.tensor(np.stack(jr.spectra(N)))
    e, V = torch.linalg.eigh(A)
    return A, e, V


def _check(A, e, Vt, ref_e):
    N = A.shape[-1]
    for b in range(A.shape[0]):
        nrm = max(ref_e[b].abs().max().item(), 1e-300)
        V = Vt[b].T
        resid = (A[b] @ V - V * e[b]).abs().max().item() / (N * U * nrm)
        orth = (V.T @ V - torch.eye(N, dtype=A.dtype)).abs().max().item() / (N * U)
        eig = (torch.sort(e[b]).values - ref_e[b]).abs().max().item() / (N * U * nrm)
        print(f"N = {N} matrix {b}: resid {resid:.3f} ({RESID_MAX})  orth {orth:.3f} "
              f"({ORTH_MAX:.3f})  eig {eig:.3f} ({EIG_MAX:.3f})")
        assert resid <= RESID_MAX and orth <= ORTH_MAX and eig <= EIG_MAX, (b, resid, orth, eig)


@pytest.mark.parametrize("N", SHAPES)
def test_eigh_psd_against_lapack(gpu, N):
    from pfml.ops import linalg as la
    A, ref_e, _ = _batch(N)
    Ad = A.to(gpu)
    st = torch.zeros(3, dtype=torch.int32, device=gpu)
    info = {}
    e, Vt = la.eigh_psd(Ad, status=st, info=info)
    assert 1 <= info["sweeps"] <= 30
    print("sweeps:", info["sweeps"], " LDS bytes:", la.nat.hip_lib().pfml_eigh_psd_lds_bytes(N))
    assert e.shape == (3, N) and Vt.shape == (3, N, N)
    assert st.tolist() == [0, 0, 0]
    assert torch.equal(Ad.cpu(), A)                                  # the input is not modified
    assert 0 < la.nat.hip_lib().pfml_eigh_psd_lds_bytes(N) <= 160 * 1024
    _check(A, e.cpu(), Vt.cpu(), ref_e)


def test_sort_orders_ascending(gpu):
    from pfml.ops.linalg import eigh_psd
    A, ref_e, _ = _batch(40)
    e, Vt = eigh_psd(A.to(gpu), sort=True)
    e, Vt = e.cpu(), Vt.cpu()
    assert bool((e[:, 1:] >= e[:, :-1]).all())
    _check(A, e, Vt, ref_e)
    # the pairing of value and vector survives the gather: the residual above; and the values
    # line up with LAPACK's without a sort
    nrm = ref_e.abs().amax(dim=1, keepdim=True)
    assert bool(((e - ref_e).abs() <= EIG_MAX * 40 * U * nrm).all())


@pytest.mark.parametrize("N", [40, 100])
def test_bitwise_independent_of_the_batch(gpu, N):
    """A matrix alone, first of 3 and last of 5 next to neighbours that need more sweeps gives
    the same bits (the matrix: a nearly diagonal one, done in a few sweeps; the neighbours: the
    production spectra, 11 to 14 sweeps in the numpy model)."""
    from pfml.ops import linalg as la
    A, _, _ = _batch(N)
    rng = np.random.default_rng(N)
    Q = rng.normal(size=(N, N)) * 1e-6
    quick = torch.tensor(np.diag(np.arange(1.0, N + 1)) + Q + Q.T).unsqueeze(0).to(gpu)
    slow = A[1:2].to(gpu)
    alone, three = {}, {}
    e1, V1 = la.eigh_psd(quick, info=alone)
    e3, V3 = la.eigh_psd(torch.cat([quick, slow, slow]), info=three)
    assert three["sweeps"] > alone["sweeps"]                # the neighbours did go on sweeping
    e5, V5 = la.eigh_psd(torch.cat([slow, A[0:1].to(gpu), slow, slow, quick]))
    assert torch.equal(e3[0], e1[0]) and torch.equal(V3[0], V1[0])
    assert torch.equal(e5[4], e1[0]) and torch.equal(V5[4], V1[0])
    assert torch.equal(e5[0], e3[1]) and torch.equal(V5[0], V3[1])


def test_nan_matrix_is_refused_and_costs_nothing(gpu):
    from pfml.ops import linalg as la
    A, ref_e, _ = _batch(40)
    two = torch.stack([A[0], A[1]]).to(gpu)
    i2, i3, i1 = {}, {}, {}
    e2, V2 = la.eigh_psd(two, info=i2)
    bad = A[2].clone()
    bad[5, 7] = bad[7, 5] = float("nan")
    st = torch.zeros(3, dtype=torch.int32, device=gpu)
    e3, V3 = la.eigh_psd(torch.stack([A[0], bad, A[1]]).to(gpu), status=st, info=i3)
    assert st.tolist() == [0, 1, 0]
    assert i3["sweeps"] <= i2["sweeps"]
    assert torch.equal(e3[0], e2[0]) and torch.equal(V3[0], V2[0])
    assert torch.equal(e3[2], e2[1]) and torch.equal(V3[2], V2[1])
    # nothing but refused matrices: no sweep at all
    st1 = torch.zeros(1, dtype=torch.int32, device=gpu)
    la.eigh_psd(bad.unsqueeze(0).to(gpu), status=st1, info=i1)
    assert st1.tolist() == [1] and i1["sweeps"] == 0


def test_max_sweeps_flags_unconverged(gpu):
    from pfml.ops import linalg as la
    A, _, _ = _batch(100)
    st = torch.zeros(3, dtype=torch.int32, device=gpu)
    info = {}
    la.eigh_psd(A.to(gpu), max_sweeps=2, status=st, info=info)
    assert st.tolist() == [1, 1, 1] and info["sweeps"] == 2


def test_too_wide_raises(gpu):
    from pfml.ops.linalg import eigh_psd
    with pytest.raises(ValueError):
        eigh_psd(torch.zeros(1, 1153, 1153, dtype=torch.float64, device=gpu))


# ---------------------------------------------------------------------------------------
# m_tilde_0 from the eigendecomposition
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [40, 129, 496])
def test_m_tilde0_eig(gpu, N):
    """Against V f(E) V' from LAPACK on the CPU: <= 1e-12 of the largest entry (the project's
    m_tilde tolerance, test_m_tilde_production_shape; CPU to CPU the numpy model is at 1.4e-14);
    m0 solves m0 (x + 2I) - m0^2 - I = 0 to 1e-11; exactly symmetric.

    f has an infinite slope at 0 (f(e) ~ 1 - sqrt(e)), so the reference takes LAPACK's
    eigenvalues that are zero to LAPACK's own accuracy, |e| <= N u |x|_2, as the zeros they
    stand for (only the rank N / 2 Gram matrix has any: its null space is exact by
    construction).  With LAPACK's +-1e-13 |x|_2 noise put through f instead, the reference
    itself is off by sqrt(noise): the printed 'raw' figure, 9.5e-8 / 1.6e-7 / 4.0e-7 at N = 40 /
    129 / 496 for that matrix (8e-15 / 3.4e-14 / 2.4e-13 against the reference used), and the
    same as the reference used for the two full-rank ones."""
    from pfml.ops.linalg import m_tilde0_eig
    x, ref_e, ref_V = _batch(N)

    def v_f_vt(ec):
        f = 2.0 / (ec + 2.0 + torch.sqrt(ec * ec + 4.0 * ec))
        return ref_V @ torch.diag_embed(f) @ ref_V.transpose(1, 2)

    raw = v_f_vt(ref_e.clamp_min(0.0))
    nrm = ref_e.abs().amax(dim=1, keepdim=True)
    ref = v_f_vt(torch.where(ref_e.abs() <= N * U * nrm, torch.zeros_like(ref_e),
                             ref_e).clamp_min(0.0))
    st = torch.zeros(3, dtype=torch.int32, device=gpu)
    xd = x.to(gpu)
    m0 = m_tilde0_eig(xd, st).cpu()
    assert st.tolist() == [0, 0, 0] and torch.equal(xd.cpu(), x)
    assert torch.equal(m0, m0.transpose(1, 2))
    I = torch.eye(N, dtype=torch.float64)
    for b in range(3):
        err = (m0[b] - ref[b]).abs().max().item() / ref[b].abs().max().item()
        quad = (m0[b] @ (x[b] + 2.0 * I) - m0[b] @ m0[b] - I).abs().max().item()
        err_raw = (m0[b] - raw[b]).abs().max().item() / raw[b].abs().max().item()
        print(f"N = {N} matrix {b}: vs eigh {err:.2e} (1e-12; raw {err_raw:.2e})  "
              f"quadratic {quad:.2e} (1e-11)")
        assert err <= 1e-12 and quad <= 1e-11, (b, err, quad)


# ---------------------------------------------------------------------------------------
# the m_func repair
# ---------------------------------------------------------------------------------------
def _repair_args(N, n, wealth, dev=None):
    S, lam, w, mask = jr.production_inputs(N, n, wealth)
    t = lambda v: torch.tensor(v, dtype=torch.float64)                      # noqa: E731
    args = [t(S), t(lam), t(w), t([0.003, 0.001]), 0.007, 10.0, 10]
    mask = t(mask)
    if dev is not None:
        args = [a.to(dev) if isinstance(a, torch.Tensor) else a for a in args]
        mask = mask.to(dev)
    return args, mask


@pytest.mark.parametrize("wealth", [(1.0, 1e10), (1e4, 1e6)])
@pytest.mark.parametrize("N,n", [(40, 37), (96, 90)])
def test_repair_on_device_matches_cpu(gpu, monkeypatch, N, n, wealth):
    """``m_func_reference`` on device tensors (eigen root) against the same call on CPU tensors
    (convergence-checked Denman-Beavers root): <= 1e-12 of the largest entry; the host square
    root is not reached, and the repaired matrices are counted."""
    from pfml.ops import linalg as la
    args, mask = _repair_args(N, n, wealth)
    ref = la.m_func_reference(*args, mask=mask)
    dargs, dmask = _repair_args(N, n, wealth, gpu)

    def no_host_root(*a, **k):
        raise AssertionError("host square root reached")

    monkeypatch.setattr(la, "sqrtm_spd", no_host_root)
    before = la.COUNTERS.as_dict()
    got = la.m_func_reference(*dargs, mask=dmask).cpu()
    after = la.COUNTERS.as_dict()
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    print(f"N = {N} wealth {wealth}: device vs CPU repair {err:.2e} (1e-12)")
    assert err <= 1e-12
    assert after.get("linalg.m_func_repair_eig", 0) - before.get("linalg.m_func_repair_eig", 0) == 2
    assert after.get("linalg.eigh_not_converged", 0) == before.get("linalg.eigh_not_converged", 0)


def test_wider_than_the_eigensolver_takes_the_host_root(gpu, monkeypatch):
    """``m_func_reference`` serves any width: beyond the eigensolver's largest N (1152; lowered
    to 32 here, under the test's N = 40) the device call takes the host square root, as it did
    before the eigensolver existed, and gives the CPU call's result to 1e-12."""
    from pfml.ops import linalg as la
    args, mask = _repair_args(40, 37, (1.0, 1e10))
    ref = la.m_func_reference(*args, mask=mask)
    dargs, dmask = _repair_args(40, 37, (1.0, 1e10), gpu)
    assert la.eigh_psd_max_n() == 1152
    calls = []
    host_root = la.sqrtm_spd

    def counted(S, *a, **k):
        calls.append(tuple(S.shape))
        return host_root(S, *a, **k)

    monkeypatch.setattr(la, "sqrtm_spd", counted)
    monkeypatch.setattr(la, "eigh_psd_max_n", lambda: 32)
    before = la.COUNTERS.as_dict()
    got = la.m_func_reference(*dargs, mask=dmask).cpu()
    after = la.COUNTERS.as_dict()
    assert calls == [(2, 40, 40)]
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    assert after.get("linalg.m_func_repair_host_wide", 0) \
        - before.get("linalg.m_func_repair_host_wide", 0) == 2
    assert after.get("linalg.m_func_repair_eig", 0) == before.get("linalg.m_func_repair_eig", 0)
    # the solver itself still refuses the width
    with pytest.raises(ValueError):
        la.eigh_psd(dargs[0])


def test_switch_restores_the_host_root(gpu, monkeypatch):
    from pfml.ops import linalg as la
    dargs, dmask = _repair_args(40, 37, (1.0, 1e10), gpu)

    class Reached(Exception):
        pass

    def host_root(*a, **k):
        raise Reached

    monkeypatch.setattr(la, "sqrtm_spd", host_root)
    monkeypatch.setattr(la, "MFUNC_REPAIR_EIG", False)
    with pytest.raises(Reached):
        la.m_func_reference(*dargs, mask=dmask)


# ---------------------------------------------------------------------------------------
# the frontier's chunked repair
# ---------------------------------------------------------------------------------------
def test_frontier_chunked_repair_takes_the_device_root(gpu, monkeypatch):
    """The small setup of test_chunked_m_func_repair_matches_one_batch (40 stocks, wealth 1,
    20 months flagged by hand): after ``_finish_chunked`` the summands and the kept m_tilde
    are finite and equal, to 1e-8 of the largest entry (the pipeline's path-to-path
    tolerance), those of a run with the host root; no month took the host root."""
    from pfml.config import Config
    from pfml.data.synthetic import engine_inputs
    from pfml.models import frontier
    from pfml.models import pfml_inputs as pin
    from pfml.ops import linalg as la
    from pfml.utils.dates import pfml_date_grids
    cfg = Config.default().override(["pf_ml.p_vec=[8,16]", "pf.dates.start_year=2001",
                                     "pf.dates.end_yr=2004", "pf.dates.split_years=1",
                                     "split.test_end=2004-12-31"])
    cfg.run.compat_mode = False
    chars, barra, wealth, rf = engine_inputs(n_stocks=40, start="1993-01-31", end="2004-12-31")
    cfg_pt = frontier.point_config(cfg, 1.0, 10.0)
    wealth_pt = frontier.scaled_wealth(cfg, wealth, 1.0)
    s = cfg.settings
    g = pfml_date_grids(int(barra.months.min()), int(cfg.pf_set["lb_hor"]),
                        s["split"]["test_end"], s["pf"]["dates"]["start_year"],
                        s["pf"]["dates"]["split_years"])
    m2, oos = g["m2"], g["oos"]
    plan = pin.make_s4_plan(cfg_pt, chars, barra, wealth_pt, rf, gpu, m2)
    monkeypatch.setattr(frontier, "REPAIR_CHUNK", 8)

    def finish(eig):
        monkeypatch.setattr(la, "MFUNC_REPAIR_EIG", eig)
        out = pin.run_plan(plan, cfg_pt, keep_m=oos, defer_checks=True)
        out.pending["mstat"][-20:] = 1
        before = la.COUNTERS.as_dict()
        # (at 40 stocks the hand-flagged months pass the device's own Denman-Beavers check, and
        # the finish's re-run would not send them to the repair: with the tail tolerance below
        # zero every month of the re-run is flagged there and takes m_func_reference)
        with monkeypatch.context() as mp:
            mp.setattr(la, "DB_TAIL_TOL", -1.0)
            n = frontier._finish_chunked(plan, cfg_pt, out)
        after = la.COUNTERS.as_dict()
        assert n >= 20 and out.pending is None
        return out, before, after

    dev, before, after = finish(True)
    assert after.get("linalg.m_func_repair_eig", 0) - before.get("linalg.m_func_repair_eig", 0) >= 20
    assert after.get("linalg.eigh_not_converged", 0) == before.get("linalg.eigh_not_converged", 0)
    host, _, _ = finish(False)
    for a, b in ((dev.reals.denom, host.reals.denom), (dev.reals.r_tilde, host.reals.r_tilde),
                 (dev.m_keep["mt"], host.m_keep["mt"]), (dev.m_keep["a"], host.m_keep["a"])):
        assert torch.isfinite(a).all()
        err = (a - b).abs().max().item() / b.abs().max().item()
        print(f"device root vs host root: {err:.2e} (1e-8)")
        assert err <= 1e-8
