"""Default utilities kernel (csrc/quadform.hip quadform_pipe_kernel: the pipelined loop for the
aligned tiles, the direct form's loop for every other tile) against the CPU oracle
``quadform_utilities``: loop-structure and L edge cases, poisoned padding, jobs per cell,
launch-composition independence and the production sizes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P, L, T = 200, 101, 13
# 0 - 3 main steps + tail split (1, 17, 33, 49); aligned without tail (64); one row tile of 4
# steps (65); two of 8 and 4 (129); three, 12 steps (193); the general path with masks (100, 130)
NS = [1, 17, 33, 49, 64, 65, 129, 193, 100, 130]


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.fixture(autouse=True)
def _default_form(monkeypatch):
    for k in ("PFML_QUAD_DIRECT", "PFML_QUAD_MM", "PFML_QUAD_XCD"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def data():
    """D (PSD, so the quadratic term dominates and no utility sits near zero), R, beta of one
    cell per n of NS, and the oracle's utilities of every (cell, month) - computed once."""
    from pfml.ops.ridge import quadform_utilities
    X = _rand(T, 64, P, seed=201)
    D = X.transpose(1, 2) @ X
    R = _rand(T, P, seed=202)
    beta = _rand(len(NS), L, P, seed=203)
    jc = np.repeat(np.arange(len(NS)), T)
    jm = np.tile(np.arange(T), len(NS))
    jn = np.repeat(np.array(NS), T)
    ref = quadform_utilities(D, R, beta, jc, jm, jn).reshape(len(NS), T, L)
    return D, R, beta, ref


def _rel(out, ref, floor):
    return ((out - ref).abs() / ref.abs().clamp_min(floor)).max().item()


def _run(gpu, D, R, beta, jc, jm, jn):
    from pfml.ops.ridge import quadform_utilities
    return quadform_utilities(D.to(gpu), R.to(gpu), beta.to(gpu), np.asarray(jc), np.asarray(jm),
                              np.asarray(jn)).cpu()


def test_loop_edges_mixed_launch(gpu, data):
    """Every n of NS in one launch, two months each."""
    D, R, beta, ref = data
    jc = np.repeat(np.arange(len(NS)), 2)
    jm = np.tile(np.array([3, 7]), len(NS))
    jn = np.repeat(np.array(NS), 2)
    out = _run(gpu, D, R, beta, jc, jm, jn)
    want = ref[jc, jm]
    rel = _rel(out, want, 1e-12)
    print("rel", rel)
    assert rel < 1e-11, rel


@pytest.mark.parametrize("ci", range(len(NS)), ids=[f"n{n}" for n in NS])
def test_composition_independence(gpu, data, monkeypatch, ci):
    """A job alone, inside a mixed launch and without the XCD tile order: bitwise equal."""
    D, R, beta, ref = data
    n = NS[ci]
    alone = _run(gpu, D, R, beta, [ci], [5], [n])
    rel = _rel(alone, ref[ci, 5][None], 1e-12)
    print("rel", rel)
    assert rel < 1e-11, rel
    jc = np.concatenate([np.repeat(np.arange(len(NS)), 3), [ci]])
    jm = np.concatenate([np.tile(np.array([0, 5, 9]), len(NS)), [11]])
    jn = np.array(NS)[jc]
    mixed = _run(gpu, D, R, beta, jc, jm, jn)
    assert torch.equal(mixed[3 * ci + 1], alone[0])
    monkeypatch.setenv("PFML_QUAD_XCD", "0")
    flat = _run(gpu, D, R, beta, jc, jm, jn)
    assert torch.equal(flat, mixed)


def test_pipelined_equals_direct_form(gpu, data, monkeypatch):
    """The pipelined loop adds the direct form's products in the direct form's order (the
    diagonal weight 1/2 is exact wherever it is applied): bitwise equal on every n of NS."""
    D, R, beta, _ = data
    jc = np.repeat(np.arange(len(NS)), 2)
    jm = np.tile(np.array([4, 10]), len(NS))
    jn = np.repeat(np.array(NS), 2)
    new = _run(gpu, D, R, beta, jc, jm, jn)
    monkeypatch.setenv("PFML_QUAD_DIRECT", "1")
    old = _run(gpu, D, R, beta, jc, jm, jn)
    assert torch.equal(new, old)


@pytest.mark.parametrize("Lx", [1, 16, 17, 101, 112])
def test_lambda_counts(gpu, data, Lx):
    from pfml.ops.ridge import quadform_utilities
    D, R, beta, _ = data
    b = _rand(3, Lx, P, seed=210 + Lx)
    jc, jm, jn = np.array([0, 1, 2, 0]), np.array([1, 2, 3, 4]), np.array([65, 129, 100, 65])
    want = quadform_utilities(D, R, b, jc, jm, jn)
    out = _run(gpu, D, R, b, jc, jm, jn)
    rel = _rel(out, want, 1e-12)
    print("rel", rel)
    assert rel < 1e-11, rel


def test_lambda_count_113_refused(gpu, data):
    D, R, _, _ = data
    b = _rand(1, 113, P, seed=330)
    with pytest.raises(RuntimeError, match="pfml_quadform failed with hipError 1"):
        _run(gpu, D, R, b, [0], [0], [65])


def test_poisoned_padding(gpu, data):
    """beta past each cell's n is NaN (ldB > n) and D past [:n, :n] holds the larger matrix's
    values: neither may reach a result."""
    D, R, beta, ref = data
    b = beta.clone()
    for ci, n in enumerate(NS):
        b[ci, :, n:] = float("nan")
    jc = np.repeat(np.arange(len(NS)), 2)
    jm = np.tile(np.array([2, 12]), len(NS))
    jn = np.repeat(np.array(NS), 2)
    out = _run(gpu, D, R, b, jc, jm, jn)
    assert torch.isfinite(out).all()
    rel = _rel(out, ref[jc, jm], 1e-12)
    print("rel", rel)
    assert rel < 1e-11, rel


def test_jobs_per_cell(gpu, data):
    """1, 2, 3, 12 and 13 jobs of a cell (odd jobs out included) and two n classes in one
    cell, in one launch."""
    from pfml.ops.ridge import quadform_utilities
    D, R, beta, ref = data
    c129, c65 = NS.index(129), NS.index(65)
    # cells of the launch: five beta blocks used at n = 129, a sixth at n = 65 and n = 129
    b = torch.stack([beta[c129], beta[c65], beta[c129].flip(0), beta[c65].flip(0),
                     beta[NS.index(193)], beta[NS.index(130)]])
    counts = [1, 2, 3, 12, 13]
    jc = np.concatenate([np.full(k, i) for i, k in enumerate(counts)] + [np.full(5, 5)])
    jm = np.concatenate([np.arange(k) for k in counts] + [np.array([0, 1, 2, 3, 4])])
    jn = np.concatenate([np.full(sum(counts), 129), np.array([65, 129, 65, 129, 129])])
    want = quadform_utilities(D, R, b, jc, jm, jn)
    out = _run(gpu, D, R, b, jc, jm, jn)
    rel = _rel(out, want, 1e-12)
    print("rel", rel)
    assert rel < 1e-11, rel
    # cell 0 is the n = 129 cell of the shared reference
    assert _rel(out[:1], ref[c129, 0][None], 1e-12) < 1e-11


def test_production_sizes(gpu):
    """One n = 513 job and one n = 257 job under the default form."""
    from pfml.ops.ridge import quadform_utilities
    Pp = 513
    X = _rand(2, 600, Pp, seed=98)
    D = X.transpose(1, 2) @ X / 600
    R = _rand(2, Pp, seed=99)
    beta = 0.1 * _rand(2, L, Pp, seed=100)
    jc, jm, jn = np.array([0, 1]), np.array([0, 1]), np.array([513, 257])
    want = quadform_utilities(D, R, beta, jc, jm, jn)
    out = _run(gpu, D, R, beta, jc, jm, jn)
    rel = _rel(out, want, 1e-9)
    print("rel", rel)
    assert rel < 1e-10, rel
