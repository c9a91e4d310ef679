"""Solo instance of the cooperative band reduction (csrc/ridge_band.hip, band_coop_kernel<.., SOLO>):
the kernel a launch takes when every cell has one workgroup (K = 1).  It must give bitwise the
betas of the general kernel at K = 1 (PFML_COOP_SOLO=0) and at K = 2, whose arithmetic it shares."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P = 528          # the band path's largest n: m = 512, every LDS row of the panel in use


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.fixture(scope="module")
def stacks():
    """Two exactly symmetric SPD matrices (n_obs = 700 > P: full rank), right-hand sides and
    L = 5 lambdas, built once for every case (never modified)."""
    X = _rand(2, 700, P, seed=271)
    SD = X.transpose(1, 2) @ X
    SD = 0.5 * (SD + SD.transpose(1, 2))
    Sr = _rand(2, P, seed=272)
    lv = torch.tensor([0.0] + list(np.exp(np.linspace(-10, 10, 4))), dtype=torch.float64)
    return SD, Sr, lv


def _launch(rg, gpu, stacks, src, nn, monkeypatch, k, solo):
    SD, Sr, lv = stacks
    monkeypatch.setenv("PFML_COOP_K", k)
    if solo:
        monkeypatch.delenv("PFML_COOP_SOLO", raising=False)
    else:
        monkeypatch.setenv("PFML_COOP_SOLO", "0")
    sc = np.full(len(src), 1.5e-3)
    out = rg.ridge_grid(SD.to(gpu), Sr.to(gpu), np.asarray(src), np.asarray(nn), sc,
                        lv.to(gpu)).cpu()
    assert rg.coop_errors() == 0, (list(nn), k, solo)
    return out


# 17: one panel, no look-ahead; 33: a one-row look-ahead panel; 49, 100: ragged; 145: more block
# rows than waves; 65 / 257 / 513: the production sizes; 528: the largest (m = 512)
@pytest.mark.parametrize("n", [17, 33, 49, 65, 100, 145, 257, 513, 528])
def test_band_solo_bitwise_general_k1_and_k2(gpu, stacks, n, monkeypatch):
    from pfml.ops import ridge as rg
    SD, Sr, lv = stacks
    src, nn = [0, 1], [n, n]
    solo = _launch(rg, gpu, stacks, src, nn, monkeypatch, "1", True)     # nwg == ncells: solo
    gen1 = _launch(rg, gpu, stacks, src, nn, monkeypatch, "1", False)    # general kernel, K = 1
    gen2 = _launch(rg, gpu, stacks, src, nn, monkeypatch, "2", True)     # K = 2: general kernel
    assert torch.equal(solo, gen1), float((solo - gen1).abs().max())
    assert torch.equal(solo, gen2), float((solo - gen2).abs().max())
    ref = rg.ridge_grid(SD, Sr, np.asarray(src), np.asarray(nn), np.full(2, 1.5e-3), lv)
    rel = ((solo - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
    assert rel < 1e-10, (n, rel)


def test_band_solo_mixed_sizes_bitwise(gpu, stacks, monkeypatch):
    """Cells of different n in ONE all-K = 1 launch (the solo instance) give, cell by cell,
    bitwise the betas of each cell launched alone."""
    from pfml.ops import ridge as rg
    src, nn = [0, 1, 0, 1, 0], [513, 65, 257, 17, 100]
    mixed = _launch(rg, gpu, stacks, src, nn, monkeypatch, "1", True)
    for c in range(len(src)):
        one = _launch(rg, gpu, stacks, src[c:c + 1], nn[c:c + 1], monkeypatch, "1", True)
        assert torch.equal(one[0], mixed[c]), (c, nn[c])
