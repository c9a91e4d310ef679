"""Kernel-level tests of csrc/weights.hip, csrc/panel.hip and csrc/scores.hip at the shapes where
their loops take a second trip, their guards cut a partial tile and their dispatch changes
form (production N ~ 500 / P = 512, the 3000-stock stress, the LDS limit), against the plain
longdouble references of tests/oracle.py (validated on the CPU in test_stage_kernel_refs.py).
Bounds are derived (dot-product bounds, or a multiple of the error of the same formula
evaluated sequentially in fp64), not tuned to the kernels' output."""
import numpy as np
import pytest
import torch

import oracle as orc
from oracle import LD, U

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -777.25                                   # sentinel of the gaps around an output block


def _d(x, gpu):
    return None if x is None else torch.as_tensor(x).to(gpu)


# ---------------------------------------------------------------------------------------
# 1. weight chain
# ---------------------------------------------------------------------------------------
def _chain_dev(ops, gpu, strided=False):
    """portfolio._chain on device operands; ``strided``: mt as the [:, :N, :N] view of a wider
    NaN-filled buffer and a through .contiguous() of a wider NaN-padded one, as S9 passes
    S4's m_keep."""
    from pfml.models.portfolio import _chain
    mt, a, wa, grow, nmap, hit, ws0 = ops
    B, N = wa.shape
    if strided:
        buf = torch.full((B, N + 7, N + 9), NAN, dtype=torch.float64, device=gpu)
        buf[:, :N, :N] = _d(mt, gpu)
        mt_d = buf[:, :N, :N]
        abuf = torch.full((B, N + 5), NAN, dtype=torch.float64, device=gpu)
        abuf[:, :N] = _d(a, gpu)
        a_d = abuf[:, :N].contiguous()
        assert mt_d.stride(1) == N + 9 and not mt_d.is_contiguous()
    else:
        mt_d, a_d = _d(mt, gpu), _d(a, gpu)
    out = _chain(mt_d, a_d, *(_d(x, gpu) for x in (wa, grow, nmap, hit, ws0)))
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def _chain_cpu(ops):
    from pfml.models.portfolio import _chain
    return tuple(x.numpy() for x in _chain(*(torch.as_tensor(x) for x in ops)))


@pytest.mark.parametrize("N,B", [(N, B) for N in (1, 3, 4, 5, 63, 64, 65, 257, 511, 512, 513, 1030)
                                 for B in (1, 5)] + [(4096, 2)])
def test_weight_chain_one_step_bound(gpu, N, B):
    """weights_month_kernel: Wst[0] == ws0 and the drift gather bitwise, every month's w_opt
    within 2 (N + 4) u (|wa| + |a| sum |M| |d|) of the longdouble step from the device's own
    w_start (N = 1 .. 4096: partial first load, all eight loads, a second and an eighth trip of
    the 512-column loop, row guard at N % 4 != 0)."""
    from pfml.ops import _native as nat
    assert nat.hip_lib().pfml_weights_chain_max_n() == 4096        # every N here: the kernel
    ops = orc.chain_inputs(N, B, seed=100 * N + B)
    Wst, Wopt, ws = _chain_dev(ops, gpu)
    assert np.isfinite(Wst).all() and np.isfinite(Wopt).all() and np.isfinite(ws).all()
    worst = orc.check_chain(ops, Wst, Wopt, ws)
    print(f"chain N={N} B={B}: worst error / bound = {worst:.3e}")


@pytest.mark.parametrize("N", [65, 513])
def test_weight_chain_strided_operand(gpu, N):
    """m_tilde as a strided view inside a NaN-filled wider buffer: finite outputs, bitwise the
    contiguous run (no read outside the view, row and batch strides honoured)."""
    ops = orc.chain_inputs(N, 3, seed=31 * N)
    ref = _chain_dev(ops, gpu)
    got = _chain_dev(ops, gpu, strided=True)
    for g, r in zip(got, ref):
        assert np.isfinite(g).all()
        assert np.array_equal(g, r)
    orc.check_chain(ops, *got)


def test_weight_chain_nan_aim_and_empty(gpu):
    """A NaN aim in one row of one month: the NaN masks of the device chain equal the CPU
    branch's; Bm = 0 returns ws0."""
    ops = list(orc.chain_inputs(65, 4, seed=77))
    ops[2] = ops[2].copy()
    ops[2][1, 7] = np.nan
    got, ref = _chain_dev(ops, gpu), _chain_cpu(ops)
    for g, r in zip(got, ref):
        assert np.array_equal(np.isnan(g), np.isnan(r))
    assert not np.isnan(got[1][0]).any() and np.isnan(got[1][1]).any()
    empty = [x[:0] for x in ops[:6]] + [ops[6]]
    Wst, Wopt, ws = _chain_dev(empty, gpu)
    assert Wst.shape == (0, 65) and Wopt.shape == (0, 65)
    assert np.array_equal(ws, ops[6])


def test_weight_chain_above_lds_limit_torch_branch(gpu):
    """N = 4097 > the kernel's LDS limit: the device torch branch, equal to the CPU branch to
    1e-13 of each output's largest entry (element-wise relative error is unbounded where the
    N-term sum cancels; the library GEMV's summation order differs from the CPU's)."""
    ops = orc.chain_inputs(4097, 2, seed=4097)
    got, ref = _chain_dev(ops, gpu), _chain_cpu(ops)
    for g, r in zip(got, ref):
        for m in range(len(np.atleast_2d(r))):
            gm, rm = np.atleast_2d(g)[m], np.atleast_2d(r)[m]
            assert np.abs(gm - rm).max() <= 1e-13 * np.abs(rm).max()
    assert np.array_equal(got[0][0], ops[6])


# ---------------------------------------------------------------------------------------
# 2. aim GEMV
# ---------------------------------------------------------------------------------------
AIM_NROW = (1, 3, 4, 5, 50, 513)
AIM_NK = (1, 17, 64, 65, 129, 513)


def _aim_jobs(gpu):
    """Every nrow x nk once.  Signal blocks: [:, :nk] views of NaN-filled [nrow, nk + 3 + j % 5]
    buffers; coef rows NaN beyond nk; output offsets with gaps of 1 .. 3."""
    rng = np.random.default_rng(17)
    pairs = [(r, k) for r in AIM_NROW for k in AIM_NK]
    sig_h, sig_d = [], []
    coefs = np.full((len(pairs), 520), np.nan)
    offs, o = [], 2
    for j, (nrow, nk) in enumerate(pairs):
        s = rng.standard_normal((nrow, nk))
        buf = torch.full((nrow, nk + 3 + j % 5), NAN, dtype=torch.float64, device=gpu)
        buf[:, :nk] = _d(s, gpu)
        sig_h.append(s)
        sig_d.append(buf[:, :nk])
        coefs[j, :nk] = rng.standard_normal(nk)
        offs.append(o)
        o += nrow + 1 + j % 3
    return pairs, sig_h, sig_d, coefs, np.asarray(offs, np.int64), o


def test_aim_gemv_mixed_launch(gpu):
    """aim_gemv_kernel through portfolio._aim_gemv: one launch mixing nrow 1 .. 513 with nk
    1 .. 513 (1 to 9 trips of the k loop, partial last trip, partial last 4-row workgroup):
    gaps untouched, every output within 2 (nk + 1) u sum |s c| of the longdouble dot product,
    and each job's bits independent of the launch it is in and of its position."""
    from pfml.models.portfolio import _aim_gemv
    pairs, sig_h, sig_d, coefs, offs, total = _aim_jobs(gpu)
    nk = [k for _, k in pairs]
    cd = _d(coefs, gpu)
    out = torch.full((total,), SENT, dtype=torch.float64, device=gpu)
    _aim_gemv(sig_d, cd, nk, offs, out)
    got = out.cpu().numpy()
    touched = np.zeros(total, bool)
    for j, (nrow, k) in enumerate(pairs):
        ref, mag = orc.aim_ref(sig_h[j], coefs[j, :k])
        g = got[offs[j]:offs[j] + nrow]
        assert np.all(np.abs(g.astype(LD) - ref) <= 2.0 * (k + 1) * U * mag), (nrow, k)
        touched[offs[j]:offs[j] + nrow] = True
    assert np.all(got[~touched] == SENT) and (~touched).sum() > len(pairs)
    # each job alone, and the whole list reversed: the same bits
    J = len(pairs)
    for j, (nrow, k) in enumerate(pairs):
        one = torch.full((nrow + 2,), SENT, dtype=torch.float64, device=gpu)
        _aim_gemv([sig_d[j]], cd[j:j + 1], [k], [1], one)
        one = one.cpu().numpy()
        assert one[0] == SENT and one[-1] == SENT
        assert np.array_equal(one[1:-1], got[offs[j]:offs[j] + nrow]), (nrow, k)
    rev = torch.full((total,), SENT, dtype=torch.float64, device=gpu)
    _aim_gemv(sig_d[::-1], cd.flip(0).contiguous(), nk[::-1], offs[::-1], rev)
    assert np.array_equal(rev.cpu().numpy(), got)
    assert J == 36


# ---------------------------------------------------------------------------------------
# 3. panel kernels
# ---------------------------------------------------------------------------------------
def _run_standardize(case, gpu):
    """standardize_signals into a column block of a wider sentinel-filled buffer and
    signal_stats likewise; returns (out, stats) as NumPy, sentinels checked."""
    from pfml.ops.panel import signal_stats, standardize_signals
    B, TH, N, P, Pw = case["B"], case["TH"], case["N"], case["P"], case["Pw"]
    F, idx, mask, vol = (_d(case[k], gpu) for k in ("F", "idx", "mask", "vol"))
    wide = torch.full((B, TH, N, Pw + 8), SENT, dtype=torch.float64, device=gpu)
    out = standardize_signals(F, idx, mask, vol, P=P, out=wide[..., 3:3 + Pw],
                              row_scale=_d(case["row_scale"], gpu))
    swide = torch.full((B, TH, 2, Pw + 5), SENT, dtype=torch.float64, device=gpu)
    st = signal_stats(F, idx, mask, P, swide[..., :Pw])
    torch.cuda.synchronize()
    w, sw = wide.cpu().numpy(), swide.cpu().numpy()
    assert np.all(w[..., :3] == SENT) and np.all(w[..., 3 + Pw:] == SENT)
    assert np.all(sw[..., Pw:] == SENT)
    return out.cpu().numpy(), st.cpu().numpy()


def _check_standardize(case, gpu):
    """-> (e_ref, kernel error of the write call, of the block implied by the stats call)."""
    B, TH, N, P, Pw = case["B"], case["TH"], case["N"], case["P"], case["Pw"]
    args = (case["F"], case["idx"], case["n_real"], case["vol"], P, Pw)
    ref, _, _ = orc.standardize_ref(*args, case["row_scale"])
    X = case["F"][:, :P][case["idx"]].reshape(B * TH, N, P)
    m64, s64 = orc.shifted_stats_f64(X, np.repeat(case["n_real"], TH))
    seq = orc.apply_stats_f64(*args, m64.reshape(B, TH, P), s64.reshape(B, TH, P),
                              case["row_scale"])
    e_ref = orc.col_err(seq, ref)
    tol = orc.panel_tol(e_ref)
    out, st = _run_standardize(case, gpu)
    assert not np.isnan(out).any() and not np.isnan(st).any()
    for b in range(B):                                     # pad rows, pad columns: zero
        assert np.all(out[b, :, case["n_real"][b]:] == 0)
    assert np.all(out[..., P:] == 0) and np.all(st[..., P:] == 0)
    assert np.all(st[:, :, 0, 0] == 0)                     # the constant is not demeaned
    err = orc.col_err(out, ref)
    imp = orc.apply_stats_f64(*args, st[:, :, 0], st[:, :, 1], case["row_scale"])
    err_st = orc.col_err(imp, ref)
    print(f"standardize N={N} P={P} Pw={Pw} B={B} TH={TH}: e_ref={e_ref:.3e} "
          f"kernel={err:.3e} stats={err_st:.3e} tol={tol:.3e}")
    assert err <= tol and err_st <= tol
    # same kernel, same sums: the stats call's (mean, scale) are bitwise the write call's,
    # so the block they imply (one rounding per operation, the kernel's order) is its output
    assert np.array_equal(imp, out)
    return e_ref, err, out


@pytest.mark.parametrize("cs", orc.panel_cases(),
                         ids=lambda c: "N{N}-P{P}-Pw{Pw}-B{B}x{TH}".format(**c))
def test_standardize_forms(gpu, cs):
    """standardize_reg_kernel (N <= 512: up to all 32 row slots, one to three 64-column strips,
    a last strip of one real or one pad column) and the two-pass standardize_kernel (N = 513,
    600) against the longdouble standardisation; n_real in {2, N - 5, N} differing per month.

    Tolerance max(8 e_ref, 64 u), e_ref the error of the same shifted-moment formula evaluated
    sequentially in fp64 (per case).  Measured on an MI355X over these 35 cases: largest e_ref
    1.04e-13 (N = 17, P = 129: a month of n_real = 2 whose two rows nearly coincide in one
    column), largest kernel error 1.04e-13 in the same case (the kernel's sums of two rows are
    the sequential ones).  The kernel error was at most e_ref in every case, and the stats call
    implied the write call's block bitwise in every case."""
    _check_standardize(orc.panel_case(**cs), gpu)


@pytest.mark.parametrize("N", [40, 600])
def test_standardize_offset_columns(gpu, N):
    """Columns 1e6 + randn and 1e-6 randn (why the kernels use shifted moments), both forms.

    Measured on an MI355X: e_ref = kernel error = 4.8e-10 (N = 40, register form) and 6.7e-10
    (N = 600, two-pass form): the rounding of the mean K + S1 / n near 1e6, about 1e6 u
    relative to the column's spread; raw moments would lose n times that."""
    _check_standardize(orc.panel_case(N=N, P=33, Pw=34, B=2, TH=3, rs=True, k=77, offset=True),
                       gpu)


def test_standardize_forms_agree_across_dispatch(gpu):
    """N = 513 built as the N = 512 case plus one pad row: the two-pass kernel and the
    register form see the same real rows and agree within the tolerance (both are within it
    of the reference)."""
    c512 = orc.panel_case(N=512, P=65, Pw=66, B=3, TH=2, rs=True, k=91)
    R = c512["F"].shape[0] - 1
    c513 = dict(c512, N=513)
    c513["idx"] = np.concatenate([c512["idx"], np.full((3, 2, 1), R, np.int64)], axis=2)
    c513["mask"] = np.concatenate([c512["mask"], np.zeros((3, 1))], axis=1)
    c513["row_scale"] = np.concatenate([c512["row_scale"], np.full((3, 1), 1.5)], axis=1)
    e_ref, _, o512 = _check_standardize(c512, gpu)
    e_ref2, _, o513 = _check_standardize(c513, gpu)
    assert e_ref == e_ref2
    assert np.all(o513[:, :, 512] == 0)
    assert orc.col_err(o513[:, :, :512], o512) <= orc.panel_tol(e_ref)


def _check_dsum(cs, dsum):
    """date_sums' (S1, S2, K) per date against longdouble sums: K bitwise the first row's
    value; S1, S2 within the any-order summation bound 2 (n + 2) u sum |term|."""
    F, P = cs["F"], cs["P"]
    for d, n in enumerate(cs["un"]):
        X = F[cs["urows"][d, :n], :P]
        assert np.array_equal(dsum[d, 2, :P], X[0])
        s1, s2, a1 = np.zeros(P, LD), np.zeros(P, LD), np.zeros(P, LD)
        for i in range(n):
            x = X[i].astype(LD) - X[0].astype(LD)
            s1 += x
            s2 += x * x
            a1 += np.abs(x)
        assert np.all(np.abs(dsum[d, 0, :P] - s1) <= 2.0 * (n + 2) * U * a1), (d, n)
        assert np.all(np.abs(dsum[d, 1, :P] - s2) <= 2.0 * (n + 2) * U * s2), (d, n)


@pytest.mark.parametrize("umax", [1, 16, 17, 128, 129, 300])
def test_date_sums_widths(gpu, umax):
    """date_sums_kernel at umax = un from one row to three trips of its 128-row loop."""
    from pfml.ops.panel import date_sums
    cs = orc.excl_case(33, umax=umax)
    dsum = date_sums(_d(cs["F"], gpu), _d(cs["urows"], gpu), _d(cs["un"], gpu), 33, 34)
    dsum = dsum.cpu().numpy()
    assert not np.isnan(dsum).any()
    _check_dsum(cs, dsum)


@pytest.mark.parametrize("P", [33, 65])
def test_date_sums_excl_stats(gpu, P):
    """date_sums + excl_stats against the longdouble statistics of 'U(d) minus the excluded
    rows': un 16 .. 600 (one to five trips of 128 rows), en 0 .. 40 (none to three trips of 16
    rows), the row that supplies K excluded, several tiles per date slot, TH = 3 tiles per
    n_real entry.  Compared through the standardised kept rows (x - mean) * scale, tolerance
    max(8 e_ref, 64 u) with e_ref from the same difference formula sequentially in fp64.

    Measured on an MI355X: P = 33 e_ref 3.01e-14, kernel 3.01e-14; P = 65 e_ref 3.43e-14,
    kernel 3.43e-14 (the columns offset by 1e3 set both)."""
    from pfml.ops.panel import date_sums, excl_stats
    cs = orc.excl_case(P)
    F, Pw, B, TH = cs["F"], cs["Pw"], cs["B"], cs["TH"]
    assert B == len(orc.EXCL_TILES)
    k_excluded = [bt for bt in range(B * TH)
                  if cs["urows"][cs["dpos"][bt], 0] in cs["erows"][bt, :cs["en"][bt]]]
    assert len(k_excluded) >= 3                            # tiles that exclude the K row
    Fd = _d(F, gpu)
    dsum = date_sums(Fd, _d(cs["urows"], gpu), _d(cs["un"], gpu), P, Pw)
    swide = torch.full((B, TH, 2, Pw + 3), SENT, dtype=torch.float64, device=gpu)
    st = excl_stats(Fd, _d(cs["erows"], gpu), _d(cs["en"], gpu), _d(cs["dpos"], gpu), dsum,
                    _d(cs["n_real"], gpu), P, swide[..., :Pw])
    torch.cuda.synchronize()
    assert np.all(swide.cpu().numpy()[..., Pw:] == SENT)
    _check_dsum(cs, dsum.cpu().numpy())
    st = st.cpu().numpy().reshape(B * TH, 2, Pw)
    assert not np.isnan(st).any()
    assert np.all(st[:, :, P:] == 0) and np.all(st[:, 0, 0] == 0)
    e_ref = err = 0.0
    for bt, rows in enumerate(cs["kept"]):
        X = F[rows, :P]
        mean, scale = orc.stats_ref(X)
        ref = (X - mean) * scale
        d = cs["dpos"][bt]
        Xu = F[cs["urows"][d, :cs["un"][d]], :P][None]
        Xe = np.nan_to_num(F[cs["erows"][bt], :P])[None]
        m64, s64 = orc.shifted_stats_f64(Xu, [cs["un"][d]], Xe, [cs["en"][bt]])
        e_ref = max(e_ref, orc.col_err((X - m64[0]) * s64[0], ref))
        err = max(err, orc.col_err((X - st[bt, 0, :P]) * st[bt, 1, :P], ref))
    print(f"excl_stats P={P}: e_ref={e_ref:.3e} kernel={err:.3e} tol={orc.panel_tol(e_ref):.3e}")
    assert err <= orc.panel_tol(e_ref)


# ---------------------------------------------------------------------------------------
# 4. validation scores
# ---------------------------------------------------------------------------------------
def _check_scores(obj, frame, compat, cum_d, rank_d):
    nV = obj.shape[0]
    seq, k = orc.frame_rows(obj, frame, compat)
    ref = orc.cum_ref(seq)
    cum = cum_d.cpu().numpy().reshape(nV * k, -1)
    rank = rank_d.cpu().numpy().reshape(nV, -1)
    assert np.array_equal(np.isnan(cum), np.isnan(ref))
    fin = ~np.isnan(ref)
    assert np.all(np.abs(cum[fin] - ref[fin]) <= 1e-12 * np.abs(ref[fin]))
    # a NaN row repeats the previous mean bit for bit
    r, c = np.nonzero(np.isnan(seq[1:]) & ~np.isnan(cum[:-1]))
    assert len(r) > 0 and np.array_equal(cum[r + 1, c], cum[r, c])
    # the sort, isolated from last-bit differences of the means: ranks of the device's cum
    rr = orc.dense_rank_ref(cum.reshape(nV, -1))
    assert np.array_equal(np.nan_to_num(rr, nan=-1.0), np.nan_to_num(rank, nan=-1.0))
    return cum, rank


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("shape", orc.SCORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scores_production_frames(gpu, shape, compat):
    """prefix_mean_kernel at chunk lengths 5 .. 20 (one to three trips of the 8-wide loop,
    clamped tail loads) with NaN runs that start, end and span whole chunks, an all-NaN column
    and exact ties; dense_rank_kernel on the result.  Against the sequential longdouble
    running mean (1e-12 relative; R u ~ 1.4e-13), the reference ranks of the device's own cum,
    and the CPU path's ranks."""
    from pfml.models.search import validation_scores
    nV, G, nP, L, frame = shape
    obj = orc.scores_case(nV, G, nP, L, frame, compat)
    _, cum_d, rank_d = validation_scores(_d(obj, gpu), frame, compat)
    _, rank = _check_scores(obj, frame, compat, cum_d, rank_d)
    _, _, rank_c = validation_scores(torch.as_tensor(obj), frame, compat)
    assert torch.equal(rank_d.cpu().nan_to_num(-1.0), rank_c.nan_to_num(-1.0))
    assert np.isnan(rank.reshape(nV, -1, nP * L)[:, :, 4]).all()       # all-NaN column: unranked


def test_scores_all_frames_bitwise_per_frame(gpu):
    """validation_scores_all at the first production-like shape: bitwise the per-frame calls."""
    from pfml.models.search import validation_scores, validation_scores_all
    nV, G, nP, L, frame = orc.SCORE_SHAPES[0]
    for compat in (True, False):
        obj = _d(orc.scores_case(nV, G, nP, L, frame, compat), gpu)
        allf = validation_scores_all(obj, compat)
        assert len(allf) == G
        for g in range(G):
            one = validation_scores(obj, g, compat)
            for a, b in zip(allf[g], one):
                assert a.shape == b.shape
                assert torch.equal(a.nan_to_num(-7.0), b.nan_to_num(-7.0))
                assert torch.equal(torch.isnan(a), torch.isnan(b))


@pytest.mark.parametrize("G,nP,L,frame,width", [(4, 4, 64, 3, 1024), (1, 1, 1, 0, 1),
                                                (5, 5, 41, 4, 1025)])
def test_dense_rank_widths(gpu, G, nP, L, frame, width):
    """k C = 1024 exactly (no padding keys in the sort), k C = 1, and k C = 1025 (above the
    kernel's width: the device torch path, without error)."""
    from pfml.models.search import validation_scores
    rng = np.random.default_rng(width)
    nV = 7
    obj = 1.0 + rng.standard_normal((nV, G, nP, L))
    if L > 1:
        obj[:, :, 0, 1] = obj[:, :, 0, 0]                   # exact ties
    obj[2, 0, 0, 0] = np.nan
    assert (frame + 1) * nP * L == width
    _, cum_d, rank_d = validation_scores(_d(obj, gpu), frame, True)
    seq, k = orc.frame_rows(obj, frame, True)
    ref = orc.cum_ref(seq)
    cum = cum_d.cpu().numpy().reshape(nV * k, -1)
    assert np.array_equal(np.isnan(cum), np.isnan(ref))
    fin = ~np.isnan(ref)
    assert np.all(np.abs(cum[fin] - ref[fin]) <= 1e-12 * np.abs(ref[fin]))
    rr = orc.dense_rank_ref(cum.reshape(nV, -1))
    assert np.array_equal(np.nan_to_num(rr, nan=-1.0),
                          np.nan_to_num(rank_d.cpu().numpy().reshape(nV, -1), nan=-1.0))
    _, _, rank_c = validation_scores(torch.as_tensor(obj), frame, True)
    assert torch.equal(rank_d.cpu().nan_to_num(-1.0), rank_c.nan_to_num(-1.0))
