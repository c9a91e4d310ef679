"""The multi-portfolio weight chain (csrc/weights.hip weights_month_multi_kernel through
``portfolio._chain_multi``): every column bitwise the single chain ``portfolio._chain`` run on
that column's aims - at the widths where the single kernel's loops change shape, for every
number of portfolios up to and across the launch cap - plus the derived longdouble bound, the
strided m_tilde operand, per-portfolio and broadcast ws0, NaN isolation and the edge shapes.
Operands: tests/oracle.chain_inputs; the other portfolios' aims are further draws of the same
distribution."""
import functools

import numpy as np
import pytest
import torch

import oracle as orc

pytestmark = pytest.mark.gpu

NAN = float("nan")
A_MAX = 16


def _d(x, gpu):
    return torch.as_tensor(x).to(gpu)


def _cap(N):
    from pfml.ops import _native as nat
    from pfml.models import portfolio  # noqa: F401  (registers the signatures)
    return int(nat.hip_lib().pfml_weights_chain_multi_max_arms(int(N)))


def _aims(ops, A, seed):
    """[A, B, N] aims: column 0 the oracle's, the others fresh draws of its distribution."""
    wa = ops[2]
    rng = np.random.default_rng(seed)
    more = 0.01 * rng.standard_normal((A - 1,) + wa.shape)
    return np.concatenate([wa[None], more], 0)


@functools.lru_cache(maxsize=None)
def _case(N, B, A, per_ws0=False):
    """Operands on the host, and the A single chains on the device (computed once)."""
    from pfml.models.portfolio import _chain
    gpu = torch.device("cuda", 0)
    ops = orc.chain_inputs(N, B, seed=100 * N + B)
    wa = _aims(ops, A, seed=7 * N + B)
    rng = np.random.default_rng(3 * N + B)
    ws0 = np.concatenate([ops[6][None], 0.01 * rng.standard_normal((A - 1, N))], 0) \
        if per_ws0 else ops[6]
    mt, a, _, grow, nmap, hit, _ = (_d(x, gpu) for x in ops)
    single = []
    for k in range(A):
        w0 = _d(ws0[k] if per_ws0 else ws0, gpu)
        single.append(_chain(mt, a, _d(wa[k], gpu), grow, nmap, hit, w0))
    torch.cuda.synchronize()
    ref = tuple(torch.stack([s[i] for s in single]) for i in range(3))
    return ops, wa, ws0, ref


def _multi(ops, wa, ws0, gpu, strided=False):
    from pfml.models.portfolio import _chain_multi
    mt, a, _, grow, nmap, hit, _ = ops
    B, N = a.shape
    if strided:
        buf = torch.full((B, N + 7, N + 9), NAN, dtype=torch.float64, device=gpu)
        buf[:, :N, :N] = _d(mt, gpu)
        mt_d = buf[:, :N, :N]
        assert mt_d.stride(1) == N + 9 and not mt_d.is_contiguous()
    else:
        mt_d = _d(mt, gpu)
    out = _chain_multi(mt_d, _d(a, gpu), _d(wa, gpu), _d(grow, gpu), _d(nmap, gpu),
                       _d(hit, gpu), _d(ws0, gpu))
    torch.cuda.synchronize()
    return out


def _assert_bitwise(got, ref, cols=None):
    for name, g, r in zip(("Wst", "Wopt", "ws_out"), got, ref):
        r = r if cols is None else r[cols]
        assert g.shape == r.shape, name
        assert torch.equal(g, r), name


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [1, 4, 5, 63, 64, 65, 511, 512, 513, 1030])
def test_columns_bitwise_the_single_chain(gpu, N, B):
    """A = 1, 2, 14, 16 portfolios: Wst, Wopt and ws_out of every column torch.equal to
    ``_chain`` on that column (N = 1 .. 1030: partial first load, all eight loads, the second
    and third trip of the 512-column loop, the row guard at N % 4 != 0; at N = 1030 the cap is
    7, so A = 14 and 16 are chunked by the host)."""
    ops, wa, ws0, ref = _case(N, B, A_MAX)
    assert all(torch.isfinite(r).all() for r in ref)
    for A in (1, 2, 14, 16):
        _assert_bitwise(_multi(ops, wa[:A], ws0, gpu), ref, slice(0, A))


@pytest.mark.parametrize("N,B", [(65, 1), (513, 2), (1030, 2), (4096, 1)])
def test_launch_cap_and_host_chunks(gpu, N, B):
    """A = cap(N) is one launch chain, cap(N) + 1 two (the host chunks); N = 4096 (cap 2) with
    A = 3 is among them.  The cap is >= 16 at N <= 512 and >= 1 at N = 4096."""
    cap = _cap(N)
    assert cap >= 1 and _cap(512) >= 16 and _cap(100) >= 16 and _cap(4096) >= 1
    assert _cap(4097) == 0
    ops, wa, ws0, ref = _case(N, B, cap + 1)
    for A in (cap, cap + 1):
        _assert_bitwise(_multi(ops, wa[:A], ws0, gpu), ref, slice(0, A))
    if N == 4096:
        assert cap + 1 >= 3
        _assert_bitwise(_multi(ops, wa[:3], ws0, gpu), ref, slice(0, 3))


def test_launcher_refuses_above_the_cap(gpu):
    """The launcher itself answers hipErrorInvalidValue (1) for A above the cap and for
    N > WMAX, before any launch."""
    from pfml.ops import _native as nat
    lib = nat.hip_lib()
    N = 513
    cap = _cap(N)
    z = torch.zeros(8, dtype=torch.float64, device=gpu)
    p = z.data_ptr()
    st = nat.stream_of(z)
    assert lib.pfml_weights_chain_multi(p, N, N * N, p, p, N, p, p, p, N, p, 0, 1, N, cap + 1,
                                        p, p, N, p, st) == 1
    assert lib.pfml_weights_chain_multi(p, 4097, 4097 * 4097, p, p, 4097, p, p, p, 4097, p, 0,
                                        1, 4097, 1, p, p, 4097, p, st) == 1


def test_column_bits_do_not_depend_on_A_or_position(gpu):
    """The same aims as column 0 of A = 2 and as column 13 of A = 16."""
    N, B = 513, 5
    ops, wa, ws0, ref = _case(N, B, A_MAX)
    k = 5
    two = _multi(ops, wa[[k, 0]], ws0, gpu)
    order = [c for c in range(16) if c != k]
    order.insert(13, k)
    sixteen = _multi(ops, wa[order], ws0, gpu)
    for t, s, r in zip(two, sixteen, ref):
        assert torch.equal(t[0], s[13]) and torch.equal(t[0], r[k])


def test_every_column_within_the_derived_bound(gpu):
    """oracle.check_chain on every column at N = 513, A = 16: the drift bitwise and every
    month's w_opt within 2 (N + 4) u (|wa| + |a| sum |M| |d|) of the longdouble step."""
    N, B = 513, 5
    ops, wa, ws0, _ = _case(N, B, A_MAX)
    Wst, Wopt, ws = (x.cpu().numpy() for x in _multi(ops, wa, ws0, gpu))
    worst = 0.0
    for k in range(A_MAX):
        ops_k = (ops[0], ops[1], wa[k]) + tuple(ops[3:])
        worst = max(worst, orc.check_chain(ops_k, Wst[k], Wopt[k], ws[k]))
    print(f"multi chain N={N} A={A_MAX}: worst error / bound = {worst:.3e}")
    assert worst < 1.0


@pytest.mark.parametrize("N", [65, 513])
def test_strided_operand_and_per_portfolio_ws0(gpu, N):
    """m_tilde as a strided view inside a NaN-filled buffer (ldm > N) with a ws0 per portfolio,
    and with the broadcast ws0: finite, bitwise the single chains."""
    B, A = 3, 5
    ops, wa, ws0, ref = _case(N, B, A, True)
    assert ws0.shape == (A, N)
    got = _multi(ops, wa, ws0, gpu, strided=True)
    assert all(torch.isfinite(g).all() for g in got)
    _assert_bitwise(got, ref)
    assert torch.equal(got[0][:, 0], _d(ws0, gpu))
    ops_b, wa_b, ws0_b, ref_b = _case(N, B, A)
    assert ws0_b.shape == (N,)
    _assert_bitwise(_multi(ops_b, wa_b, ws0_b, gpu, strided=True), ref_b)


def test_nan_aims_stay_in_their_column(gpu):
    """NaN aims (a whole month of one portfolio, and one entry of another): every other column
    bitwise unchanged; the poisoned columns NaN from that month on."""
    N, B = 513, 5
    ops, wa, ws0, ref = _case(N, B, A_MAX)
    bad = wa.copy()
    bad[3, 1, :] = np.nan
    bad[9, 2, 17] = np.nan
    got = _multi(ops, bad, ws0, gpu)
    keep = [k for k in range(A_MAX) if k not in (3, 9)]
    _assert_bitwise(tuple(g[keep] for g in got), ref, keep)
    assert torch.isnan(got[1][3, 1]).all() and torch.isfinite(got[1][3, 0]).all()
    assert torch.isnan(got[1][9, 2]).any() and torch.isfinite(got[1][9, :2]).all()


def test_above_the_kernel_width_takes_the_torch_branch(gpu):
    """N = 4097: the batched-matmul branch on the device, each column equal to the CPU
    ``_chain`` to 1e-13 of the output's largest entry (the bound of the single chain's own
    torch-branch test: the library's summation order differs from the CPU's)."""
    from pfml.models.portfolio import _chain
    N, B, A = 4097, 2, 2
    ops = orc.chain_inputs(N, B, seed=N)
    wa = _aims(ops, A, seed=N + 1)
    got = [x.cpu().numpy() for x in _multi(ops, wa, ops[6], gpu)]
    for k in range(A):
        ops_k = (ops[0], ops[1], wa[k]) + tuple(ops[3:])
        ref = [x.numpy() for x in _chain(*(torch.as_tensor(x) for x in ops_k))]
        for g, r in zip(got, ref):
            gk, rk = np.atleast_2d(g[k]), np.atleast_2d(r)
            for m in range(len(rk)):
                assert np.abs(gk[m] - rk[m]).max() <= 1e-13 * np.abs(rk[m]).max()
    assert np.array_equal(got[0][:, 0], np.broadcast_to(ops[6], (A, N)))


def test_no_month_returns_ws0(gpu):
    N, A = 65, 3
    ops = orc.chain_inputs(N, 4, seed=77)
    empty = tuple(x[:0] for x in ops[:6]) + (ops[6],)
    wa = np.zeros((A, 0, N))
    Wst, Wopt, ws = _multi(empty, wa, ops[6], gpu)
    assert Wst.shape == (A, 0, N) and Wopt.shape == (A, 0, N)
    assert np.array_equal(ws.cpu().numpy(), np.broadcast_to(ops[6], (A, N)))
    ws0 = np.arange(A * N, dtype=np.float64).reshape(A, N)
    assert np.array_equal(_multi(empty, wa, ws0, gpu)[2].cpu().numpy(), ws0)
