"""References for the Multiperiod-ML kernels (pfml.ops.multiperiod): sequential
``np.longdouble`` code for the horizon fold and for one step of the offset weight chain, and
the fold's formula evaluated sequentially in fp64 numpy, whose error against the long-double
fold sets the scale of the device's bound (the convention of tests/factor_oracle.py).

    b_tau = (a o mu_{tau+1}) / W;  v_{K-1} = b_{K-1};  v_tau = b_tau + gbar (M v_{tau+1});  V = v_0
    w_opt = a o (M (w_start / a + u V))

Operands: M symmetric with its spectrum in (0, 1), a = 1e4 U(0.5, 2), W = 1e10, mu ~ 1e-2 N(0,
1); grow, nmap, hit and ws0 as tests/oracle.chain_inputs."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def ragged_rows(N, B):
    """n_rows of B months out of {N, 0, 1, N - 5} (clamped to [0, N]), N first."""
    pool = [N, 0, 1, max(N - 5, 0), N]
    return np.asarray([pool[t % len(pool)] for t in range(B)], np.int32)


def sym_contraction(N, rng):
    """A symmetric N x N matrix with eigenvalues U(0.05, 0.95); beyond N = 1100, where a QR
    costs seconds, a Wigner matrix around I / 2 (semicircle: spectrum in 0.5 -+ 0.2)."""
    if N > 1100:
        G = rng.standard_normal((N, N))
        return 0.5 * np.eye(N) + 0.1 * (G + G.T) / np.sqrt(2.0 * N)
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    M = (Q * rng.uniform(0.05, 0.95, N)) @ Q.T
    return 0.5 * (M + M.T)


def mp_inputs(N, B, K, A, seed, ragged=False):
    rng = np.random.default_rng(seed)
    mt = np.stack([sym_contraction(N, rng) for _ in range(B)]) if B else np.zeros((0, N, N))
    a = 1e4 * rng.uniform(0.5, 2.0, (B, N))
    mu = 1e-2 * rng.standard_normal((K, B, N))
    wealth = np.full(B, 1e10)
    n_rows = ragged_rows(N, B) if ragged else np.full(B, N, np.int32)
    grow = rng.uniform(0.9, 1.1, (B, N))
    nmap = rng.integers(0, N, (B, N), dtype=np.int64)
    hit = (rng.random((B, N)) >= 0.1).astype(np.float64)
    ws0 = 1e-2 * rng.standard_normal((A, N))
    u = np.asarray([1.0, 0.5, 0.25, 2.0, 0.0, -1.0, 3.0, 0.125] * ((A + 7) // 8))[:A]
    return dict(mt=mt, a=a, mu=mu, wealth=wealth, n_rows=n_rows, grow=grow, nmap=nmap, hit=hit,
                ws0=ws0, u=u, N=N, B=B, K=K, A=A)


def _seq_mv(M, v):
    """M v with the column loop sequential, in M's dtype; and sum_j |M_ij| |v_j|."""
    s = np.zeros(M.shape[0], M.dtype)
    g = np.zeros(M.shape[0], M.dtype)
    for j in range(M.shape[1]):
        t = M[:, j] * v[j]
        s += t
        g += np.abs(t)
    return s, g


def fold_month(M, a, mu, W, n, gbar, dtype=LD):
    """V of one month ([N], zero beyond n) from fp64 operands, every operation in ``dtype``."""
    N = len(a)
    K = mu.shape[0]
    Mn = np.ascontiguousarray(M[:n, :n]).astype(dtype)
    b = (a[:n].astype(dtype)[None] * mu[:, :n].astype(dtype)) / dtype(W)
    v = b[K - 1]
    g = dtype(gbar)
    for tau in range(K - 2, -1, -1):
        v = b[tau] + g * _seq_mv(Mn, v)[0]
    out = np.zeros(N, dtype)
    out[:n] = v
    return out


def fold_bound(V_ld, V_64, n, K):
    """8 x (error of the sequential-fp64 formula) + (n + K) u max|V_ld|, one number a month."""
    e_o = float(np.max(np.abs(V_64.astype(LD) - V_ld))) if len(V_ld) else 0.0
    scale = float(np.max(np.abs(V_ld))) if len(V_ld) else 0.0
    return 8.0 * e_o + (n + K) * U * scale


def check_fold(inp, V, gbar, months=None):
    """Device V [B, N] (numpy) against the longdouble fold -> worst error / bound; padding
    entries must be 0."""
    worst = 0.0
    for t in (range(inp["B"]) if months is None else months):
        n = int(inp["n_rows"][t])
        args = (inp["mt"][t], inp["a"][t], inp["mu"][:, t], inp["wealth"][t], n, gbar)
        v_ld, v_64 = fold_month(*args), fold_month(*args, dtype=np.float64)
        assert not np.any(V[t, n:]), f"month {t}: padding of V must be 0"
        if n == 0:
            continue
        err = float(np.max(np.abs(V[t, :n].astype(LD) - v_ld[:n])))
        bound = fold_bound(v_ld[:n], v_64[:n], n, inp["mu"].shape[0])
        assert err <= bound, f"month {t}: fold error {err:.3e} over the bound {bound:.3e}"
        worst = max(worst, err / bound)
    return worst


def chain_step_ref(M, a, V, u, ws, n):
    """One month of one arm in longdouble from fp64 operands: ref = a (M d), d = ws / a + u V
    on the n live rows, and the magnitude |a_i| sum_j |M_ij| (|ws_j / a_j| + |u V_j|) the
    rounding errors of d and of the dot product scale with."""
    Mn = np.ascontiguousarray(M[:n, :n]).astype(LD)
    al = a[:n].astype(LD)
    t1, t2 = ws[:n].astype(LD) / al, LD(u) * V[:n].astype(LD)
    s, _ = _seq_mv(Mn, t1 + t2)
    _, g = _seq_mv(Mn, np.abs(t1) + np.abs(t2))
    return al * s, np.abs(al) * g


def chain_step_bound(n, mag):
    """As tests/oracle.chain_step_bound: the dot product of n terms in any order, doubled; + 4
    for the division, the multiply and the add of d and the final multiply."""
    return 2.0 * (n + 4) * U * mag


def check_chain(inp, V, Wst, Wopt, ws_out, arms=None):
    """Every month of every arm from the outputs themselves (numpy; V the fold's fp64 output
    the chain was given), so no error compounds: Wst[:, 0] == ws0 and the drift bitwise, w_opt
    row-wise within the bound of the longdouble step, padding rows of w_opt 0.  Returns the
    largest error / bound."""
    B, N = inp["B"], inp["N"]
    ws0 = inp["ws0"]
    worst = 0.0
    for k in (range(Wst.shape[0]) if arms is None else arms):
        if B:
            assert np.array_equal(Wst[k, 0], ws0[k] if ws0.ndim == 2 else ws0), "Wst[0] != ws0"
        for t in range(B):
            nm, gr, ht = inp["nmap"][t], inp["grow"][t], inp["hit"][t]
            nxt = (Wopt[k, t][nm] * gr[nm]) * ht
            got = Wst[k, t + 1] if t + 1 < B else ws_out[k]
            assert np.array_equal(got, nxt), f"arm {k}: drift of month {t} not bitwise"
            n = int(inp["n_rows"][t])
            assert not np.any(Wopt[k, t, n:]), f"arm {k} month {t}: padding of w_opt must be 0"
            if n == 0:
                continue
            ref, mag = chain_step_ref(inp["mt"][t], inp["a"][t], V[t], inp["u"][k], Wst[k, t], n)
            err = np.abs(Wopt[k, t, :n].astype(LD) - ref)
            bound = chain_step_bound(n, mag)
            bad = np.nonzero(~(err <= bound))[0]
            assert len(bad) == 0, (f"arm {k} month {t}: {len(bad)} row(s) over the bound, first "
                                   f"{bad[0]}: err {float(err[bad[0]]):.3e} bound "
                                   f"{float(bound[bad[0]]):.3e}")
            worst = max(worst, float((err / np.where(bound > 0, bound, 1)).max()))
    return worst
