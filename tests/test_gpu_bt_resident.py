"""Back-transform with several workgroups per CU (csrc/ridge_band.hip, kernel 3): V_b goes
through a wave-private ONE-block LDS buffer, block after block, and the registers of a block
take the next panel's loads as soon as the block is consumed.  The tests pin what that form
could break: the size-class edges, a partial lambda chunk, a transpose buffer shared between
blocks or waves by mistake, a chunk's padding lanes leaking into live ones, and the zeroed
padding columns.  Every launch is checked against ops.ridge.ridge_grid on CPU tensors."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P = 528
# both sides of every instance edge (96 | 97, 192 | 193, 320 | 321), the smallest cell, the
# production sizes 65 and 513, and the band path's largest n
NN = np.array([17, 65, 96, 97, 192, 193, 320, 321, 513, 528])
SRC = np.arange(len(NN)) % 2
SC = np.full(len(NN), 1.5e-3)


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _spd_stack(S, n_obs, seed):
    X = _rand(S, n_obs, P, seed=seed)
    SD = X.transpose(1, 2) @ X
    return 0.5 * (SD + SD.transpose(1, 2))


@pytest.fixture(scope="module")
def full():
    """Full-rank stacks (n_obs = 700 > P), 101 lambdas and the CPU oracle of the mixed launch,
    computed once (never modified); the oracle of a shorter lambda list is a slice of it."""
    from pfml.ops import ridge as rg
    SD, Sr = _spd_stack(2, 700, 311), _rand(2, P, seed=312)
    lv = torch.tensor([0.0] + list(np.exp(np.linspace(-10, 10, 100))), dtype=torch.float64)
    return SD, Sr, lv, rg.ridge_grid(SD, Sr, SRC, NN, SC, lv)


@pytest.fixture(scope="module")
def mixed(gpu, full):
    """The mixed launch at L = 101 on the device (default switches), once."""
    from pfml.ops import ridge as rg
    SD, Sr, lv, _ = full
    out = rg.ridge_grid(SD.to(gpu), Sr.to(gpu), SRC, NN, SC, lv.to(gpu)).cpu()
    assert rg.coop_errors() == 0
    return out


def _rel(a, b):
    return ((a - b).norm(dim=-1) / b.norm(dim=-1).clamp(min=1e-300)).max().item()


# L = 5: one partial chunk; 17: a full chunk and a chunk of one lambda; 101: the production list
@pytest.mark.parametrize("L", [5, 17, 101])
def test_class_edges_against_oracle(gpu, full, L, monkeypatch):
    from pfml.ops import ridge as rg
    SD, Sr, lv, ref = full
    out = {}
    for v in ("0", "1"):
        monkeypatch.setenv("PFML_BT_CLASSES", v)
        out[v] = rg.ridge_grid(SD.to(gpu), Sr.to(gpu), SRC, NN, SC, lv[:L].to(gpu)).cpu()
        assert rg.coop_errors() == 0
        rel = _rel(out[v], ref[:, :L])
        print(f"L={L} classes={v} rel={rel:.3e}")
        assert rel < 1e-9, (L, v, rel)
        for c, n in enumerate(NN):
            assert not out[v][c, :, n:].any(), (L, v, n)
    rel = _rel(out["1"], out["0"])
    print(f"L={L} classes 1 vs 0 rel={rel:.3e}")
    assert rel < 1e-12, (L, rel)


def test_rank_deficient_with_lambda_zero(gpu):
    """Summands of rank 90 and lambda = 0 in the list: the band-domain repair runs before the
    back-transform.  Bound and lambda list of test_band_coop_matches_lu_and_bitwise_across_k's
    rank-deficient case; lambda = 0 is compared only where the system is regular (n <= 90)."""
    from pfml.ops import ridge as rg
    n_obs = 90
    SD, Sr = _spd_stack(2, n_obs, 313), _rand(2, P, seed=314)
    lv = torch.tensor([0.0] + list(np.exp(np.linspace(-2, 10, 40))), dtype=torch.float64)
    out = rg.ridge_grid(SD.to(gpu), Sr.to(gpu), SRC, NN, SC, lv.to(gpu)).cpu()
    assert rg.coop_errors() == 0
    ref = rg.ridge_grid(SD, Sr, SRC, NN, SC, lv)
    for c, n in enumerate(NN):
        ok = slice(1, None) if n_obs <= n else slice(None)
        rel = _rel(out[c, ok], ref[c, ok])
        print(f"n={n} rel={rel:.3e}")
        assert rel < 1e-10, (n, rel)
        assert not out[c, :, n:].any(), n


def test_cell_alone_bitwise(gpu, full, mixed):
    """The instance depends on a cell's n alone: every cell launched by itself gives the bits
    it has in the mixed launch."""
    from pfml.ops import ridge as rg
    SD, Sr, lv, _ = full
    dSD, dSr, dlv = SD.to(gpu), Sr.to(gpu), lv.to(gpu)
    for c in range(len(NN)):
        one = rg.ridge_grid(dSD, dSr, SRC[c:c + 1], NN[c:c + 1], SC[c:c + 1], dlv).cpu()
        assert torch.equal(one[0], mixed[c]), (int(NN[c]), float((one[0] - mixed[c]).abs().max()))


def test_lambda_permutation_bitwise(gpu, full, mixed):
    """The product's columns are independent: with the lambda list permuted (other chunks,
    other lanes, another lambda in the last, one-wide chunk) every lambda keeps its bits."""
    from pfml.ops import ridge as rg
    SD, Sr, lv, _ = full
    perm = torch.randperm(len(lv), generator=torch.Generator().manual_seed(315))
    out = rg.ridge_grid(SD.to(gpu), Sr.to(gpu), SRC, NN, SC, lv[perm].to(gpu)).cpu()
    assert torch.equal(out, mixed[:, perm]), float((out - mixed[:, perm]).abs().max())


def test_padding_columns_zeroed_other_rows_untouched(gpu, full, mixed):
    """beta_out pre-filled with a sentinel: the columns [n, ldo) of every lambda row of the
    launch's cells come back zero, the rows of cells outside the launch keep the sentinel."""
    from pfml.ops import ridge as rg
    SD, Sr, lv, _ = full
    L, nc, sentinel = 17, len(NN), -7.25
    plan = rg.ridge_plan(P, L, SRC, NN, SC, ncu=rg.num_cus(gpu))
    d_desc, d_wg = rg.upload([plan["desc"], plan["wgmap"]], gpu)
    beta = torch.full((nc + 2, L, P), sentinel, dtype=torch.float64, device=gpu)
    rg.reset_coop_sync()
    rg.ridge_launch(plan, d_desc, SD.to(gpu).contiguous(), Sr.to(gpu).contiguous(),
                    lv[:L].to(gpu).contiguous(), beta, True, d_wg)
    out = beta.cpu()
    assert rg.coop_errors() == 0
    for c, n in enumerate(NN):
        assert not out[c, :, n:].any(), n
        assert torch.equal(out[c, :, :n], mixed[c, :L, :n]), n
    assert bool((out[nc:] == sentinel).all())
