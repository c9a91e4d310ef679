"""Run form of the utilities kernel (csrc/quadform.hip quad_pipe_body: one workgroup walks a
run of tiles - one cell's one row tile over consecutive validation months - with the pipeline
kept full across the month boundary) and the host plan that cuts the runs (ops/ridge.py
``quad_plan(run_steps= / run_months=)``).  Every run plan must give bitwise the utilities of
the single-tile plan and of the direct form; the plan's own properties need no device."""
import numpy as np
import pytest
import torch

P, T = 130, 16
NCELL = [65, 129, 70]      # one row tile + tail index; two row tiles; not aligned (rest kernel)
MONTHS = [1, 2, 5, 12, 13]
RUN_MONTHS = [1, 2, 3, 12]
LS = [1, 17, 101, 112]


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.fixture(autouse=True)
def _default_form(monkeypatch):
    for k in ("PFML_QUAD_DIRECT", "PFML_QUAD_MM", "PFML_QUAD_XCD"):
        monkeypatch.delenv(k, raising=False)


def _inputs(L):
    """D, R and beta with NaN wherever no utility may look: D past the largest n, and past
    n = 65 in the months only the n = 65 cell uses (months 13 .. 15); beta past every cell's
    n (row stride P > n) and past its L rows (every other block of the beta array is NaN)."""
    X = _rand(T, 64, P, seed=501)
    D = X.transpose(1, 2) @ X
    D[:, 129:, :] = float("nan")
    D[:, :, 129:] = float("nan")
    D[13:, 65:, :] = float("nan")
    D[13:, :, 65:] = float("nan")
    R = _rand(T, P, seed=502)
    beta = torch.full((2 * len(NCELL), L, P), float("nan"), dtype=torch.float64)
    for ci, n in enumerate(NCELL):
        beta[2 * ci, :, :n] = _rand(L, n, seed=510 + ci)
    return D, R, beta


def _jobs(nm, seed):
    """nm months per cell in arbitrary, non-contiguous order - the n = 129 and n = 70 cells
    draw from months 0 .. 12 (at 12 and 13 months every month of theirs is shared), the
    n = 65 cell from all 16 - with the cells' jobs interleaved, and a permuted job_out."""
    rng = np.random.default_rng(seed)
    jc = np.concatenate([np.full(nm, 2 * ci) for ci in range(len(NCELL))])
    jm = np.concatenate([rng.permutation(T if ci == 0 else 13)[:nm]
                         for ci in range(len(NCELL))])
    mix = rng.permutation(len(jc))
    jc, jm = jc[mix], jm[mix]
    jn = np.array(NCELL)[jc // 2]
    return jc, jm, jn, rng.permutation(len(jc))


def _launch(gpu, dev, jc, jm, jn, job_out=None, sw=None, **plan_kw):
    """One utilities launch of a plan made with ``plan_kw``; rows no job writes keep -7.25."""
    from pfml.ops import ridge as rg
    D, R, beta = dev
    L = beta.shape[1]
    plan = rg.quad_plan(P, L, beta.shape[2], jc, jm, jn, job_out=job_out, sw=sw, **plan_kw)
    d_desc, d_tj = rg.upload([plan["desc"], rg.quad_tables(plan)], gpu)
    obj = torch.full((len(jc), L), -7.25, dtype=torch.float64, device=gpu)
    rg.quad_launch(plan, d_desc, d_tj, D, R, beta, obj, sw=sw)
    torch.cuda.synchronize()
    return obj.cpu(), plan


@pytest.mark.gpu
@pytest.mark.parametrize("L", LS)
def test_runs_equal_single_tiles_and_direct_form(gpu, L):
    """n = 65, 129 and 70 in one launch, 1 / 2 / 5 / 12 / 13 months per cell in arbitrary
    order, a permuted job_out, poisoned padding: runs forced to 1, 2, 3 and 12 months (a run
    that ends mid-cell, a run of one, month counts that are no multiple of the run length) and
    runs cut by a step target give bitwise the single-tile plan's and the direct form's
    utilities, and a cell's utilities are the same alone as inside the mixed launch."""
    from pfml.ops import ridge as rg
    D, R, beta = _inputs(L)
    dev = tuple(t.to(gpu) for t in (D, R, beta))
    for nm in MONTHS:
        jc, jm, jn, jout = _jobs(nm, seed=600 + nm)
        single, sp = _launch(gpu, dev, jc, jm, jn, job_out=jout)
        assert sp["run_off"] is None
        assert torch.isfinite(single).all(), nm
        want = rg.quadform_utilities(D, R, beta, jc, jm, jn)      # fp64 CPU formula
        rel = ((single[jout] - want).abs() / want.abs().clamp_min(1e-12)).max().item()
        print(f"L {L} months {nm}: rel {rel:.2e}")
        assert rel < 1e-11, (nm, rel)
        direct, _ = _launch(gpu, dev, jc, jm, jn, job_out=jout,
                            sw=rg.Switches(quad_direct=True))
        assert torch.equal(direct, single), nm
        plans = [dict(run_months=k) for k in RUN_MONTHS]
        plans += [dict(run_steps=8, slots=1), dict(run_steps=rg.QUAD_RUN_STEPS, slots=1)]
        for kw in plans:
            out, plan = _launch(gpu, dev, jc, jm, jn, job_out=jout, **kw)
            lens = np.diff(plan["run_off"])
            if "run_months" in kw:
                assert lens.max() == min(kw["run_months"], nm), (kw, lens)
            assert torch.equal(out, single), (nm, kw)
            direct, _ = _launch(gpu, dev, jc, jm, jn, job_out=jout,
                                sw=rg.Switches(quad_direct=True), **kw)
            assert torch.equal(direct, single), (nm, kw)
        # every cell alone, under runs, against its rows of the mixed launch
        for c in np.unique(jc):
            sel = jc == c
            alone, _ = _launch(gpu, dev, jc[sel], jm[sel], jn[sel], run_months=3)
            assert torch.equal(alone, single[jout[sel]]), (nm, int(c))


@pytest.mark.gpu
def test_runs_production_shape(gpu):
    """Two n = 513 cells x 12 months, L = 101: runs by the step target (several months per
    run, on all eight row tiles) and 12-month runs against the single-tile plan, bitwise, and
    against the fp64 torch formula."""
    from pfml.ops import ridge as rg
    Pp, L, M = 513, 101, 12
    X = _rand(M, 600, Pp, seed=98)
    D = X.transpose(1, 2) @ X / 600
    R = _rand(M, Pp, seed=99)
    beta = 0.1 * _rand(2, L, Pp, seed=100)
    jc = np.repeat(np.arange(2), M)
    jm = np.concatenate([np.arange(M), np.arange(M)[::-1]])
    jn = np.full(2 * M, Pp)
    want = rg.quadform_utilities(D, R, beta, jc, jm, jn)

    def launch(**kw):
        plan = rg.quad_plan(Pp, L, Pp, jc, jm, jn, **kw)
        d_desc, d_tj = rg.upload([plan["desc"], rg.quad_tables(plan)], gpu)
        obj = torch.empty((len(jc), L), dtype=torch.float64, device=gpu)
        rg.quad_launch(plan, d_desc, d_tj, D.to(gpu), R.to(gpu), beta.to(gpu), obj)
        torch.cuda.synchronize()
        return obj.cpu(), plan

    single, _ = launch()
    rel = ((single - want).abs() / want.abs().clamp_min(1e-9)).max().item()
    print("rel", rel)
    assert rel < 1e-10, rel
    out, plan = launch(run_steps=rg.QUAD_RUN_STEPS, slots=8)
    lens = np.diff(plan["run_off"])
    assert lens.min() >= 2 and len(lens) % 16 == 0, lens
    assert torch.equal(out, single)
    out, plan = launch(run_months=12)
    assert (np.diff(plan["run_off"]) == 12).all()
    assert torch.equal(out, single)


def _grid_jobs(sizes, cells, months, T=120):
    jc = np.repeat(np.arange(cells * len(sizes)), months)
    jm = (np.arange(len(jc)) * 7) % T
    jn = np.repeat(np.repeat(np.array(sizes), cells), months)
    return jc, jm, jn


@pytest.mark.parametrize("sizes,cells,slots", [
    ((513,), 106, 768), ((257, 129, 65), 106, 768), ((513,), 13, 768), ((257, 129, 65), 13, 96),
    ((129, 70, 65), 9, 8)])
def test_run_plan_properties(sizes, cells, slots):
    """The run plan of the benchmark's two utilities launches (106 cells x 12 months), of a
    one-in-eight shard of them and of a small launch with an unaligned cell: every (job, row
    tile) is in exactly one run; a run holds one cell and one row tile (so one n and one beta
    block); runs are in non-increasing length in every XCD's queue; no run of several tiles is
    longer than the launch's K steps per workgroup slot - a single tile cannot be cut, so a
    run of one may be, and at the benchmark's shapes none is."""
    from pfml.ops import ridge as rg
    Pp, L = 513, 101
    jc, jm, jn = _grid_jobs(sizes, cells, 12)
    plan = rg.quad_plan(Pp, L, Pp, jc, jm, jn, run_steps=rg.QUAD_RUN_STEPS, slots=slots)
    single = rg.quad_plan(Pp, L, Pp, jc, jm, jn)
    tj, ro = plan["tile_job"], plan["run_off"]
    assert ro[0] == 0 and ro[-1] == len(tj) == plan["ntiles"] and (np.diff(ro) >= 1).all()
    assert sorted(tj.tolist()) == sorted(single["tile_job"].tolist())
    assert len(np.unique(tj)) == len(tj) == plan["nslots"]
    assert np.array_equal(plan["desc"], single["desc"])
    job, rt = tj >> 5, tj & 31
    run_of = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
    first = ro[:-1][run_of]
    assert np.array_equal(jc[job], jc[job[first]]) and np.array_equal(rt, rt[first])
    assert np.array_equal(jn[job], jn[job[first]])
    steps = rg.quad_tile_steps(jn, job, rt)
    rlen = np.add.reduceat(steps, ro[:-1])
    per_slot = int(steps.sum()) // slots
    several = np.diff(ro) > 1
    assert (rlen[several] <= per_slot).all(), (rlen[several].max(), per_slot)
    assert (rlen[several] <= rg.QUAD_RUN_STEPS).all()
    if cells == 106:
        assert rlen.max() <= per_slot, (rlen.max(), per_slot)
        assert several.any()
    # unaligned tiles stay runs of one
    una = np.array([not rg.nat.hip_lib().pfml_quadform_aligned(int(n), L, Pp, Pp) for n in jn])
    assert (np.diff(ro)[np.unique(run_of[una[job]])] == 1).all()
    # the runs of the cells with affinity to one XCD (cell mod 8) form that XCD's queue
    _, dense = np.unique(jc, return_inverse=True)
    cell_x = dense[job[ro[:-1]]] % rg.NXCD
    for x in range(rg.NXCD):
        assert (np.diff(rlen[cell_x == x]) <= 0).all(), x


def test_run_plan_forced_months():
    """run_months = k: every (cell, row tile) is cut into runs of exactly k months, the last
    one taking what is left; k = 1 is a run table of single tiles."""
    from pfml.ops import ridge as rg
    jc, jm, jn = _grid_jobs((129, 65), 3, 13)
    for k in (1, 2, 3, 12, 20):
        plan = rg.quad_plan(129, 5, 129, jc, jm, jn, run_months=k)
        lens = np.diff(plan["run_off"])
        want = sorted(([k] * (13 // k) + ([13 % k] if 13 % k else [])) * 9 if k <= 13
                      else [13] * 9)
        assert sorted(lens.tolist()) == want, k
