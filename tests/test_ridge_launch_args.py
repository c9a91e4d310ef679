"""The ridge grid's launch arguments (csrc/ridge_desc.h RidgeLaunchArgs, ops/ridge.py
``LaunchArgs`` / ``launch_opts``): every option travels with its launch and none outlives it,
and the workspace, timing-buffer and sync-word sizes the library states once."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

ENV = ("PFML_COOP_SOLO", "PFML_COOP_SPIN_MAX", "PFML_BT_CLASSES", "PFML_RIDGE_BT_WY")


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    from pfml.ops import ridge as rg
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    rg.set_coop_spin_max(0)
    yield
    rg.set_coop_spin_max(0)


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def test_launch_opts_maps_every_arm(monkeypatch):
    from pfml.ops.ridge import LaunchArgs, Switches, launch_opts, switches
    base = launch_opts(Switches(), 0)
    assert base == {"spin_max": 0, "solo": True, "bt_wy": True, "bt_classes": True}
    assert set(base) <= {f[0] for f in LaunchArgs._fields_}
    arms = [("PFML_COOP_SOLO", "0", "solo", False), ("PFML_COOP_SPIN_MAX", "7", "spin_max", 7),
            ("PFML_BT_CLASSES", "0", "bt_classes", False),
            ("PFML_RIDGE_BT_WY", "0", "bt_wy", False)]
    for var, val, field, want in arms:
        with monkeypatch.context() as m:
            m.setenv(var, val)
            got = launch_opts(switches(), 0)
        assert got == {**base, field: want}, var
    # the fields land in the struct as given
    a = LaunchArgs(phases=7, **launch_opts(Switches(coop_solo=False, coop_spin_max=9), 0))
    assert (a.solo, a.bt_wy, a.bt_classes, a.spin_max, a.phases) == (False, True, True, 9, 7)
    assert a.timing is None and a.work is None


def test_set_coop_spin_max_wins_over_environment(monkeypatch):
    from pfml.ops import ridge as rg
    monkeypatch.setenv("PFML_COOP_SPIN_MAX", "7")
    assert rg.launch_opts(rg.switches())["spin_max"] == 7
    rg.set_coop_spin_max(3)
    assert rg.launch_opts(rg.switches())["spin_max"] == 3
    assert rg.launch_opts(rg.switches(), 5)["spin_max"] == 5      # (an explicit override)
    rg.set_coop_spin_max(0)
    assert rg.launch_opts(rg.switches())["spin_max"] == 7
    monkeypatch.delenv("PFML_COOP_SPIN_MAX")
    assert rg.launch_opts(rg.switches())["spin_max"] == 0


def test_library_sizes_match_the_mirrors():
    from pfml.ops import ridge as rg
    lib = rg.nat.hip_lib()
    assert lib.pfml_ridge_launch_args_size() == ctypes.sizeof(rg.LaunchArgs)
    assert lib.pfml_coop_sync_words() == 32 == rg.COOP_SYNC_WORDS
    assert [lib.pfml_ridge_timing_words(c) for c in (0, 1, 106)] == [16, 32, 106 * 16 + 16]


@pytest.mark.parametrize("L", [1, 101])
@pytest.mark.parametrize("n", [1, 16, 17, 528, 529, 1024, 1025, 2049])
def test_work_doubles_closed_form(n, L):
    """pfml_ridge_work_doubles against the closed form the layouts had before they were
    stated once (TriWork in ridge.hip, BandWork / CoopWork in ridge_band.h)."""
    from pfml.ops import ridge as rg
    npad, npan = (n + 15) // 16 * 16, (n + 15) // 16
    tri = n * n + 5 * n * L + 36 * n
    band = (npad * npad + 17 * n + n + 256 * npan + L * n + 15 + 17 * L * n
            + (32 * npad + 256 + 33 * 272))
    want = (max(tri, band) + 31) // 32 * 32
    assert rg.nat.hip_lib().pfml_ridge_work_doubles(n, L) == want


def _launch_setup(gpu, P, ncells, n_obs, seed):
    """(plan, d_desc, d_wgmap, SD, Sr, lv) of ``ncells`` cells of n = P on the device."""
    from pfml.ops import ridge as rg
    X = _rand(ncells, n_obs, P, seed=seed).to(gpu)
    SD = (X.transpose(1, 2) @ X).contiguous()
    Sr = _rand(ncells, P, seed=seed + 1).to(gpu)
    lv = torch.tensor(np.exp(np.linspace(-4, 2, 5)), dtype=torch.float64, device=gpu)
    plan = rg.ridge_plan(P, 5, np.arange(ncells), np.full(ncells, P),
                         np.full(ncells, 1.0 / n_obs), ncu=rg.num_cus(gpu))
    d_desc, d_wg = rg.upload([plan["desc"], plan["wgmap"]], gpu)
    return plan, d_desc, d_wg, SD, Sr, lv


@pytest.mark.gpu
def test_timing_is_per_launch(gpu):
    """Band path, n = 33 (two panels: the smallest shape with a look-ahead panel), two cells:
    a launch given a timing buffer fills it, the next launch without one leaves it alone, and
    the betas are the same bits."""
    from pfml.ops import ridge as rg
    plan, d_desc, d_wg, SD, Sr, lv = _launch_setup(gpu, 33, 2, 80, seed=501)
    assert rg.band_path(plan)
    buf = torch.zeros(rg.nat.hip_lib().pfml_ridge_timing_words(2), dtype=torch.int64, device=gpu)
    b1 = torch.empty((2, 5, 33), dtype=torch.float64, device=gpu)
    b2 = torch.empty_like(b1)
    rg.ridge_launch(plan, d_desc, SD, Sr, lv, b1, d_wgmap=d_wg, timing=buf)
    torch.cuda.synchronize()
    slots = buf.cpu()
    print("cell 0 slots:", slots[:8].tolist(), "solve:", slots[32:34].tolist())
    assert bool((slots[:8] != 0).all()), slots.tolist()
    buf.zero_()
    rg.ridge_launch(plan, d_desc, SD, Sr, lv, b2, d_wgmap=d_wg)
    torch.cuda.synchronize()
    assert not bool(buf.any())
    assert torch.isfinite(b1).all() and torch.equal(b1, b2)
    with pytest.raises(ValueError, match="timing must hold 48"):
        rg.ridge_launch(plan, d_desc, SD, Sr, lv, b2, d_wgmap=d_wg, timing=buf[:47])


@pytest.fixture(scope="module")
def tri_setup(gpu):
    return _launch_setup(gpu, 1025, 1, 1300, seed=511)


@pytest.mark.gpu
def test_bt_wy_is_per_launch(gpu, tri_setup):
    """Tridiagonal path, n = 1025 (the smallest size on the blocked back-transform), one cell:
    launches with bt_wy on, off, on in one process.  The first and third are the same bits;
    the generic form between them agrees to 1e-12 (recorded agreement of the forms: 2.4e-15)."""
    from pfml.ops import ridge as rg
    plan, d_desc, _, SD, Sr, lv = tri_setup
    assert not rg.band_path(plan)
    out = []
    for wy in (True, False, True):
        beta = torch.empty((1, 5, 1025), dtype=torch.float64, device=gpu)
        rg.ridge_launch(plan, d_desc, SD, Sr, lv, beta,
                        sw=dataclasses.replace(rg.Switches(), bt_wy=wy))
        out.append(beta)
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    assert torch.equal(out[0], out[2])
    rel = ((out[1] - out[0]).norm(dim=-1) / out[0].norm(dim=-1)).max().item()
    print("generic vs blocked back-transform, max relative difference:", rel)
    assert rel < 1e-12, rel
    assert not torch.equal(out[0], out[1]), "bt_wy=False did not reach the launch"


@pytest.mark.gpu
def test_partial_phases_need_the_work_of_a_full_launch(gpu, tri_setup):
    from pfml.ops import ridge as rg
    plan, d_desc, _, SD, Sr, lv = tri_setup
    beta = torch.full((1, 5, 1025), -7.25, dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError, match="work tensor of a preceding full launch"):
        rg.ridge_launch(plan, d_desc, SD, Sr, lv, beta, phases=4)
    small = torch.empty(plan["work"] - 1, dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError, match="work must hold"):
        rg.ridge_launch(plan, d_desc, SD, Sr, lv, beta, phases=4, work=small)
    torch.cuda.synchronize()
    assert bool((beta == -7.25).all()), "a refused launch queued something"
    # the back-transform alone, on the workspace of a full launch: the same betas
    work = torch.empty(plan["work"], dtype=torch.float64, device=gpu)
    full = torch.empty_like(beta)
    rg.ridge_launch(plan, d_desc, SD, Sr, lv, full, work=work)
    rg.ridge_launch(plan, d_desc, SD, Sr, lv, beta, phases=4, work=work)
    torch.cuda.synchronize()
    assert torch.equal(beta, full)
