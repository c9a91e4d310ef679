"""Start-up copy of the band reduction (csrc/ridge_band_reduce.hip, "A = S * scale"): whole rows
per wave, batched loads, masks as selects, zero padding up to lda.  The copy is shared by the solo
and the general instance, so the oracle here is independent of both: ``ridge_grid`` on the CPU
tensors (torch's dense solves), at the project's bound rel < 1e-10.

Sizes: every kind of n the band path sees - below one block (2), a whole block (16: no panel), one
and two above it (17, 18: one panel of one and two rows), 31 / 32 / 34 (odd, a multiple of 16,
two panels), 257 (a production size) and 528 (the largest, m = 512).  Stacks with P = 528 (even
ldS) and P = 513 (odd ldS: the 8-byte loads of a row start at any 8-byte phase; n <= 513).  The two
cells take their sources as src = [1, 0], so a cell's source offset is non-zero."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [2, 16, 17, 18, 31, 32, 34, 257, 528]
SCALE = 1.5e-3
SRC = [1, 0]


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _stack(P, seed):
    """Two exactly symmetric SPD matrices (n_obs = 700 > P: full rank), right-hand sides and
    L = 5 lambdas including 0."""
    X = _rand(2, 700, P, seed=seed)
    SD = X.transpose(1, 2) @ X
    SD = 0.5 * (SD + SD.transpose(1, 2))
    Sr = _rand(2, P, seed=seed + 1)
    lv = torch.tensor([0.0] + list(np.exp(np.linspace(-10, 10, 4))), dtype=torch.float64)
    return SD, Sr, lv


@pytest.fixture(scope="module")
def stacks():
    """The stacks per P, built once and never modified."""
    return {528: _stack(528, 811), 513: _stack(513, 813)}


@pytest.fixture(scope="module")
def cpu_refs(stacks):
    """CPU ``ridge_grid`` betas per (P, n), computed once on first use and shared by the K cases."""
    cache = {}

    def get(P, n):
        if (P, n) not in cache:
            from pfml.ops import ridge as rg
            SD, Sr, lv = stacks[P]
            cache[(P, n)] = rg.ridge_grid(SD, Sr, np.asarray(SRC), np.asarray([n, n]),
                                          np.full(2, SCALE), lv)
        return cache[(P, n)]

    return get


@pytest.mark.parametrize("k", ["1", "2"])
@pytest.mark.parametrize("P, n", [(P, n) for P in (528, 513) for n in SIZES if n <= P])
def test_band_startup_against_cpu(gpu, stacks, cpu_refs, monkeypatch, P, n, k):
    from pfml.ops import ridge as rg
    SD, Sr, lv = stacks[P]
    monkeypatch.setenv("PFML_COOP_K", k)            # "1": the solo instance; "2": the general one
    monkeypatch.delenv("PFML_COOP_SOLO", raising=False)
    out = rg.ridge_grid(SD.to(gpu), Sr.to(gpu), np.asarray(SRC), np.asarray([n, n]),
                        np.full(2, SCALE), lv.to(gpu)).cpu()
    assert rg.coop_errors() == 0, (P, n, k)
    ref = cpu_refs(P, n)
    assert torch.isfinite(out).all(), (P, n, k)
    assert torch.equal(out[..., n:], torch.zeros_like(out[..., n:])), (P, n, k)
    rel = ((out - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
    print(f"P={P} n={n} K={k} rel={rel:.3e}")
    assert rel < 1e-10, (P, n, k, rel)


def _launch_with_work(rg, gpu, stack, n, work):
    """Two cells of size n queued through ``ridge_launch`` on the given workspace tensor."""
    SD, Sr, lv = stack
    P, L = SD.shape[-1], int(lv.numel())
    plan = rg.ridge_plan(P, L, np.asarray(SRC), np.asarray([n, n]), np.full(2, SCALE),
                         ncu=rg.num_cus(gpu))
    assert work.numel() >= plan["work"]
    d_desc, d_wg = rg.upload([plan["desc"], plan["wgmap"]], gpu)
    beta = torch.zeros((2, L, P), dtype=torch.float64, device=gpu)
    rg.reset_coop_sync()
    rg.ridge_launch(plan, d_desc, SD.to(gpu), Sr.to(gpu), lv.to(gpu), beta, d_wgmap=d_wg, work=work)
    out = beta.cpu()
    assert rg.coop_errors() == 0, n
    return out, plan["work"]


@pytest.mark.parametrize("k", ["1", "2"])
def test_band_startup_stale_workspace(gpu, stacks, monkeypatch, k):
    """Two n = 528 cells, then two n = 18 cells on the SAME workspace: the small cells' padding
    rows and columns (18 -> lda = 32) lie where the large cells left live numbers.  Their betas
    must equal, bitwise, those of the same cells on a fresh (zeroed) workspace under a fresh
    plan: the padding zeros are written by the copy, not inherited."""
    from pfml.ops import ridge as rg
    monkeypatch.setenv("PFML_COOP_K", k)
    monkeypatch.delenv("PFML_COOP_SOLO", raising=False)
    stack = stacks[528]
    L = int(stack[2].numel())
    words = rg.ridge_plan(528, L, np.asarray(SRC), np.asarray([528, 528]), np.full(2, SCALE),
                          ncu=rg.num_cus(gpu))["work"]
    fresh, _ = _launch_with_work(rg, gpu, stack, 18,
                                 torch.zeros(words, dtype=torch.float64, device=gpu))
    work = torch.zeros(words, dtype=torch.float64, device=gpu)
    big, used = _launch_with_work(rg, gpu, stack, 528, work)
    assert torch.isfinite(big).all() and used <= words
    assert bool((work[:32 * 32] != 0).any())          # the small cells' A region holds old data
    stale, _ = _launch_with_work(rg, gpu, stack, 18, work)
    assert torch.isfinite(stale).all()
    assert torch.equal(stale, fresh), float((stale - fresh).abs().max())
