"""The launch switches of the grid step (ops/ridge.py ``Switches``): parsing, the cached
utilities plan keyed on them, and the retired utilities forms refused by the library."""
import dataclasses

import numpy as np
import pytest
import torch

ENV = ("PFML_COOP_K", "PFML_COOP_SOLO", "PFML_COOP_SPIN_MAX", "PFML_BT_CLASSES",
       "PFML_RIDGE_BT_WY", "PFML_RIDGE_STREAMS", "PFML_QUAD_DIRECT", "PFML_QUAD_XCD",
       "PFML_QUAD_MM")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _spd_stack(S, P, n_obs, seed):
    X = _rand(S, n_obs, P, seed=seed)
    return X.transpose(1, 2) @ X / n_obs


def test_switches_defaults_and_other_arms(monkeypatch):
    from pfml.ops.ridge import Switches, switches
    base = switches()
    assert base == Switches()
    assert dataclasses.asdict(base) == {
        "coop_k": None, "coop_solo": True, "coop_spin_max": 0, "bt_classes": True,
        "bt_wy": True, "two_streams": True, "quad_direct": False, "quad_xcd": True}
    arms = [("PFML_COOP_K", "3", "coop_k", 3), ("PFML_COOP_SOLO", "0", "coop_solo", False),
            ("PFML_COOP_SPIN_MAX", "7", "coop_spin_max", 7),
            ("PFML_BT_CLASSES", "0", "bt_classes", False),
            ("PFML_RIDGE_BT_WY", "0", "bt_wy", False),
            ("PFML_RIDGE_STREAMS", "1", "two_streams", False),
            ("PFML_QUAD_DIRECT", "1", "quad_direct", True),
            ("PFML_QUAD_XCD", "0", "quad_xcd", False)]
    assert sorted(a[2] for a in arms) == sorted(f.name for f in dataclasses.fields(Switches))
    seen = {base}
    for var, val, field, want in arms:
        with monkeypatch.context() as m:
            m.setenv(var, val)
            sw = switches()
        assert dataclasses.asdict(sw) == {**dataclasses.asdict(base), field: want}, var
        # differing in one field: unequal, and a different hash (the plan cache's key)
        assert sw != base and hash(sw) != hash(base), var
        seen.add(sw)
    assert len(seen) == len(arms) + 1


def test_switches_odd_values_parse_as_before(monkeypatch):
    """The parent's readers: two streams unless PFML_RIDGE_STREAMS is set, non-empty and not
    "2" after stripping; an empty PFML_COOP_K is unset; an empty PFML_COOP_SPIN_MAX is 0."""
    from pfml.ops.ridge import switches
    for val, want in (("", True), ("1", False), ("2", True), (" 2 ", True)):
        monkeypatch.setenv("PFML_RIDGE_STREAMS", val)
        assert switches().two_streams is want, repr(val)
    monkeypatch.setenv("PFML_COOP_K", "")
    assert switches().coop_k is None
    monkeypatch.setenv("PFML_COOP_SPIN_MAX", "")
    assert switches().coop_spin_max == 0
    # any value but 0 is the direct form, as before
    monkeypatch.setenv("PFML_QUAD_DIRECT", "yes")
    assert switches().quad_direct is True


def test_retired_switches_raise(monkeypatch):
    from pfml.ops.ridge import Switches, switches
    monkeypatch.setenv("PFML_QUAD_MM", "1")
    assert switches() == Switches()
    monkeypatch.setenv("PFML_QUAD_MM", "2")
    with pytest.raises(ValueError, match="PFML_QUAD_MM=2.*retired"):
        switches()
    monkeypatch.delenv("PFML_QUAD_MM")
    monkeypatch.setenv("PFML_QUAD_DIRECT", "0")
    with pytest.raises(ValueError, match="PFML_QUAD_DIRECT=0.*retired"):
        switches()


@pytest.mark.gpu
def test_utilities_plan_follows_quad_xcd(gpu, monkeypatch):
    """Two grid searches in one process, the second with PFML_QUAD_XCD=0: the cached plan of
    the first must not be reused (its tile order is the other arm's); betas and utilities are
    bitwise the same either way.  Nine n = 129 cells (two row tiles each; cell mod 8 wraps)
    and one n = 65 cell, so the launch splits into two groups."""
    from pfml.ops import ridge as rg
    P, L = 129, 5
    SD = _spd_stack(2, P, n_obs=300, seed=401) * 300
    Sr = _rand(2, P, seed=402)
    lv = torch.tensor(np.exp(np.linspace(-4, 2, L)), dtype=torch.float64)
    nn = np.array([129] * 9 + [65])
    src = np.arange(len(nn)) % 2
    sc = np.full(len(nn), 1.0 / 300)
    D = _spd_stack(2, P, n_obs=200, seed=403)
    R = _rand(2, P, seed=404)
    jc = np.repeat(np.arange(len(nn)), 2)
    jm = np.tile(np.array([0, 1]), len(nn))
    jn = nn[jc]
    rb, ro = rg.ridge_utilities(SD, Sr, src, nn, sc, lv, D, R, jc, jm, jn)
    dev = [t.to(gpu) for t in (SD, Sr)], lv.to(gpu), [t.to(gpu) for t in (D, R)]

    def run():
        (a, b), l, (d, r) = dev
        beta, obj = rg.ridge_utilities(a, b, src, nn, sc, l, d, r, jc, jm, jn)
        torch.cuda.synchronize()
        return beta.cpu(), obj.cpu()

    rg._UTIL_PLANS.clear()
    b1, o1 = run()
    first = list(rg._UTIL_PLANS.values())
    assert len(first) == 1
    monkeypatch.setenv("PFML_QUAD_XCD", "0")
    b2, o2 = run()
    plans = list(rg._UTIL_PLANS.values())
    assert len(plans) == 2, "the second search reused the plan cached under the other switch"
    second = [p for p in plans if p is not first[0]][0]
    assert len(first[0]["groups"]) == len(second["groups"]) == 2
    tj = [[g[3]["tile_job"] for g in p["groups"]] for p in (first[0], second)]
    assert sorted(tj[0][0].tolist()) == sorted(tj[1][0].tolist())
    assert not np.array_equal(tj[0][0], tj[1][0])
    assert torch.equal(b1, b2) and torch.equal(o1, o2)
    rel = ((b1 - rb).norm(dim=-1) / rb.norm(dim=-1).clamp(min=1e-300)).max().item()
    assert rel < 1e-8, rel
    assert torch.allclose(o1, ro, rtol=1e-8, atol=1e-12 * ro.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_retired_quadform_forms_refused(gpu, form):
    """pfml_quadform's ``form`` 1 and 2 (the LDS-staged forms) are invalid values: nothing is
    queued, obj keeps its sentinel."""
    from pfml.ops import _native as nat, ridge as rg
    P, L = 65, 5
    D = _spd_stack(2, P, n_obs=100, seed=411).to(gpu)
    R = _rand(2, P, seed=412).to(gpu)
    beta = _rand(1, L, P, seed=413).to(gpu)
    plan = rg.quad_plan(P, L, P, np.array([0, 0]), np.array([0, 1]), np.array([65, 65]))
    d_desc, d_tj = rg.upload([plan["desc"], plan["tile_job"]], gpu)
    partial = torch.empty((plan["nslots"], L), dtype=torch.float64, device=gpu)
    obj = torch.full((2, L), -7.25, dtype=torch.float64, device=gpu)
    with pytest.raises(RuntimeError, match="pfml_quadform failed with hipError 1"):
        nat.check(nat.hip_lib().pfml_quadform(
            D.data_ptr(), P, R.data_ptr(), beta.data_ptr(), P, d_desc.data_ptr(), plan["nj"],
            d_tj.data_ptr(), plan["ntiles"], form, L, partial.data_ptr(), obj.data_ptr(),
            nat.stream_of(D)), "pfml_quadform")
    torch.cuda.synchronize()
    assert torch.equal(obj.cpu(), torch.full((2, L), -7.25, dtype=torch.float64))
