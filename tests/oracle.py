"""Straight-line fp64 NumPy oracle of one PFML month, in the reference's own operation order
(PFML_Input_Data.py:318-491; General_functions.py:919-963): explicit cumulative products,
np.linalg.solve, scipy.linalg.sqrtm.  Independent of the batched engine."""
import numpy as np
import scipy.linalg as sla


def m_func_ref(w, mu, rf, sigma_gam, gam, lam, iterations):
    n = len(lam)
    c = 1 + rf + mu
    mbar = np.full(n, c)
    sgr = (np.outer(mbar, mbar) + sigma_gam / gam) / c ** 2
    a = np.diag(lam ** -0.5)
    x = (1.0 / w) * a @ sigma_gam @ a
    y = np.diag(1 + np.diag(sgr))
    sh = x + 2 * np.eye(n)
    mt = 0.5 * (sh - np.real(sla.sqrtm(sh @ sh - 4 * np.eye(n))))
    for _ in range(iterations):
        mt = np.linalg.inv(x + y - mt * sgr)
    return a @ mt @ np.diag(lam ** 0.5)


def month_ref(S_win, gt_win, r, Sigma, lam, w, rf, mu, gamma, iterations=10):
    """S_win: [13, n, P] standardised signals for lags 0..12; gt_win: [13, n]."""
    n = Sigma.shape[0]
    m = m_func_ref(w, mu, rf, Sigma * gamma, gamma, lam, iterations)
    gtm = [m @ np.diag(gt_win[t]) for t in range(13)]
    agg = [np.eye(n)]
    agg_l1 = [np.eye(n)]
    for t in range(11):
        agg.append(agg[t] @ gtm[t])
        agg_l1.append(agg_l1[t] @ gtm[t + 1])
    om = sum(agg[t] @ S_win[t] for t in range(12))
    const = sum(agg[t] for t in range(12))
    om1 = sum(agg_l1[t] @ S_win[t + 1] for t in range(12))
    const1 = sum(agg_l1[t] for t in range(12))
    omega = np.linalg.solve(const, om)
    omega_l1 = np.linalg.solve(const1, om1)
    chg = omega - np.diag(gt_win[0]) @ omega_l1
    r_tilde = omega.T @ r
    risk = gamma * omega.T @ Sigma @ omega
    tc = w * chg.T @ np.diag(lam) @ chg
    return r_tilde, risk, tc, m


# ---------------------------------------------------------------------------------------
# Stage-kernel references (tests/test_gpu_stage_kernels.py, tests/test_stage_kernel_refs.py):
# plain NumPy in np.longdouble with sequential loops over the summed index (vectorised only
# over independent outputs).  None of them calls the code under test.
# ---------------------------------------------------------------------------------------
LD = np.longdouble
U = 2.0 ** -53                                  # unit roundoff of fp64


# ---- weight chain ---------------------------------------------------------------------
def chain_inputs(N, B, seed):
    """NumPy fp64 operands of a bounded weight chain: (mt, a, wa, grow, nmap, hit, ws0)."""
    rng = np.random.default_rng(seed)
    mt = rng.standard_normal((B, N, N)) / (2.0 * np.sqrt(N))
    a = rng.uniform(0.5, 1.5, (B, N))
    wa = 0.01 * rng.standard_normal((B, N))
    grow = rng.uniform(0.9, 1.1, (B, N))
    nmap = rng.integers(0, N, (B, N), dtype=np.int64)
    hit = (rng.random((B, N)) >= 0.1).astype(np.float64)
    ws0 = 0.01 * rng.standard_normal(N)
    return mt, a, wa, grow, nmap, hit, ws0


def chain_step_ref(M, a, wa, ws, drop=None, rows=512):
    """One month in longdouble from fp64 operands: ref = wa + a (M d), d = (ws - wa) / a, and
    the magnitude |wa| + |a| sum_j |M_ij| |d_j| the error bound scales with.  The j loop is
    sequential; ``drop``: leave term j = drop out (the sharpness check)."""
    N = len(a)
    d = (ws.astype(LD) - wa.astype(LD)) / a.astype(LD)
    acc, mag = np.zeros(N, LD), np.zeros(N, LD)
    for i0 in range(0, N, rows):
        Mt = np.ascontiguousarray(M[i0:i0 + rows].T).astype(LD)      # [j, rows]
        s, g = np.zeros(Mt.shape[1], LD), np.zeros(Mt.shape[1], LD)
        for j in range(N):
            if j == drop:
                continue
            t = Mt[j] * d[j]
            s += t
            g += np.abs(t)
        acc[i0:i0 + rows], mag[i0:i0 + rows] = s, g
    return wa.astype(LD) + a.astype(LD) * acc, np.abs(wa).astype(LD) + np.abs(a).astype(LD) * mag


def chain_step_bound(N, mag):
    """2 gamma_N-style bound of one month: the dot product of N terms in any summation order,
    doubled; + 4 for the division, the final multiply-add and a possible FMA contraction."""
    return 2.0 * (N + 4) * U * mag


def check_chain(ops, Wst, Wopt, ws_out):
    """Per-month checks of a chain's outputs (NumPy fp64 [B, N], [B, N], [N]) from those
    outputs themselves, so no error compounds.  Returns the largest error / bound ratio."""
    mt, a, wa, grow, nmap, hit, ws0 = ops
    B, N = wa.shape
    assert Wst.shape == (B, N) and Wopt.shape == (B, N) and ws_out.shape == (N,)
    assert np.array_equal(Wst[0], ws0), "Wst[0] != ws0"
    worst = 0.0
    for m in range(B):
        nxt = (Wopt[m][nmap[m]] * grow[m][nmap[m]]) * hit[m]
        got = Wst[m + 1] if m + 1 < B else ws_out
        assert np.array_equal(got, nxt), f"drift of month {m} not bitwise"
        ref, mag = chain_step_ref(mt[m], a[m], wa[m], Wst[m])
        err = np.abs(Wopt[m].astype(LD) - ref)
        bound = chain_step_bound(N, mag)
        bad = np.nonzero(~(err <= bound))[0]
        assert len(bad) == 0, (f"month {m}: {len(bad)} row(s) over the bound, first {bad[0]}: "
                               f"err {float(err[bad[0]]):.3e} bound {float(bound[bad[0]]):.3e}")
        worst = max(worst, float((err / bound).max()))
    return worst


# ---- aim GEMV -------------------------------------------------------------------------
def aim_ref(s, c):
    """Rows of s [nrow, nk] dot c [nk] in longdouble (sequential over k) and sum_k |s c|."""
    acc, mag = np.zeros(s.shape[0], LD), np.zeros(s.shape[0], LD)
    for k in range(s.shape[1]):
        t = s[:, k].astype(LD) * LD(c[k])
        acc += t
        mag += np.abs(t)
    return acc, mag


# ---- panel standardisation ------------------------------------------------------------
def standardize_ref(F, idx, n_real, vol, P, Pw, row_scale=None):
    """Longdouble standardisation of the gathered tiles: F [R+1, >= P], idx [B, TH, N],
    n_real [B], vol [R+1] -> (out [B, TH, N, Pw], mean [B, TH, P], scale [B, TH, P]): mean over
    the n real rows (0 for column 0), unit-L2 scale, division by vol[row], then the row scale;
    pad rows and pad columns zero."""
    B, TH, N = idx.shape
    X = F[:, :P].astype(LD)[idx]                                   # [B, TH, N, P]
    n = np.asarray(n_real).reshape(B, 1, 1)
    live = (np.arange(N).reshape(1, N) < np.asarray(n_real).reshape(B, 1))      # [B, N]
    s = np.zeros((B, TH, P), LD)
    for i in range(N):
        s += np.where(live[:, i].reshape(B, 1, 1), X[:, :, i], LD(0))
    mean = s / n.astype(LD)
    mean[..., 0] = 0
    q = np.zeros((B, TH, P), LD)
    for i in range(N):
        dlt = X[:, :, i] - mean
        q += np.where(live[:, i].reshape(B, 1, 1), dlt * dlt, LD(0))
    scale = 1 / np.sqrt(q)
    out = np.zeros((B, TH, N, Pw), LD)
    v = vol.astype(LD)[idx][..., None]
    out[..., :P] = np.where(live.reshape(B, 1, N, 1),
                            (X - mean[:, :, None]) * scale[:, :, None] / v, LD(0))
    if row_scale is not None:
        out *= row_scale.astype(LD).reshape(B, 1, N, 1)
    return out, mean, scale


def shifted_stats_f64(X, n_real, Xe=None, ne=None):
    """The kernels' shifted-moment formula evaluated sequentially in fp64: X [T, N, P] tile
    rows (tile t uses its first n_real[t]; K = row 0), optionally minus the excluded rows Xe
    [T, E, P] (first ne[t]); n = n_real - ne.  Returns (mean, scale) [T, P]."""
    T, N, P = X.shape
    K = X[:, 0].copy()
    s1, s2 = np.zeros((T, P)), np.zeros((T, P))
    nr = np.asarray(n_real).reshape(T, 1)
    for i in range(N):
        x = np.where(i < nr, X[:, i] - K, 0.0)
        s1 += x
        s2 += x * x
    n = nr.astype(np.float64)
    if Xe is not None:
        e1, e2 = np.zeros((T, P)), np.zeros((T, P))
        ner = np.asarray(ne).reshape(T, 1)
        for i in range(Xe.shape[1]):
            x = np.where(i < ner, Xe[:, i] - K, 0.0)
            e1 += x
            e2 += x * x
        s1, s2 = s1 - e1, s2 - e2
        n = n - ner
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = K + s1 / n
        scale = np.sqrt(1.0 / (s2 - s1 * s1 / n))
        tk = s1[:, 0] + n[:, 0] * K[:, 0]
        scale[:, 0] = np.sqrt(1.0 / (s2[:, 0] + 2.0 * K[:, 0] * tk - n[:, 0] * K[:, 0] * K[:, 0]))
    mean[:, 0] = 0.0
    return mean, scale


def apply_stats_f64(F, idx, n_real, vol, P, Pw, mean, scale, row_scale=None):
    """out = ((x - mean) * scale) / vol [* row_scale] in fp64, one rounding per operation in
    the kernels' order; pad rows / columns zero.  mean, scale: [B, TH, >= P]."""
    B, TH, N = idx.shape
    X = F[:, :P][idx]
    live = (np.arange(N).reshape(1, N) < np.asarray(n_real).reshape(B, 1)).reshape(B, 1, N, 1)
    out = np.zeros((B, TH, N, Pw))
    val = ((X - mean[:, :, None, :P]) * scale[:, :, None, :P]) / vol[idx][..., None]
    out[..., :P] = np.where(live, val, 0.0)
    if row_scale is not None:
        out = out * row_scale.reshape(B, 1, N, 1)
    return out


def col_err(got, ref):
    """Per-column error max_i |got - ref| / max_i |ref| over the row axis (-2), reduced to the
    largest column; a column whose reference is all zero must be exactly zero."""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    num = np.abs(got - ref).max(axis=-2)
    den = np.abs(ref).max(axis=-2)
    assert np.all(num[den == 0] == 0), "non-zero output where the reference is all zero"
    r = np.where(den > 0, num / np.where(den > 0, den, 1), 0)
    assert not np.isnan(r).any(), "NaN in a compared column"
    return float(r.max())


def panel_tol(e_ref):
    """Tolerance of a panel kernel given the error of the sequential fp64 evaluation of the
    same formula: x 8 for the 4- or 16-stream partial sums and FMA contraction, floor 64 u."""
    return max(8.0 * e_ref, 64.0 * U)


def stats_ref(X):
    """Longdouble (mean, scale) of the rows of X [n, P] (column 0 not demeaned)."""
    X = X.astype(LD)
    s = np.zeros(X.shape[1], LD)
    for i in range(X.shape[0]):
        s += X[i]
    mean = s / LD(X.shape[0])
    mean[0] = 0
    q = np.zeros(X.shape[1], LD)
    for i in range(X.shape[0]):
        q += (X[i] - mean) ** 2
    return mean, 1 / np.sqrt(q)


# ---- validation scores ----------------------------------------------------------------
def frame_rows(obj, frame_g, compat):
    """The frame's row sequence [nV * k, C] of obj [nV, G, nP, L] (months outer, g' inner)."""
    g0, g1 = (0, frame_g + 1) if compat else (frame_g, frame_g + 1)
    nV = obj.shape[0]
    return obj[:, g0:g1].reshape(nV * (g1 - g0), -1), g1 - g0


def cum_ref(seq):
    """Expanding mean of the non-NaN values per column, sequential over the rows with a running
    sum and count (longdouble); a NaN row copies the previous value; NaN until the first
    finite one.  seq [R, C] -> [R, C] longdouble."""
    R, C = seq.shape
    s, n = np.zeros(C, LD), np.zeros(C)
    out = np.full((R, C), np.nan, LD)
    for r in range(R):
        ok = ~np.isnan(seq[r])
        s = s + np.where(ok, seq[r], 0.0).astype(LD)
        n = n + ok
        new = np.where(n > 0, s / np.maximum(n, 1).astype(LD), LD(np.nan))
        out[r] = np.where(ok, new, out[r - 1] if r else LD(np.nan))
    return out


def dense_rank_ref(vals):
    """Dense descending rank over the finite values of each row of vals [nV, n] (NaN: NaN)."""
    out = np.full(vals.shape, np.nan)
    for v in range(vals.shape[0]):
        fin = ~np.isnan(vals[v])
        uq = np.unique(vals[v][fin])                       # ascending, -0 == +0
        out[v][fin] = len(uq) - np.searchsorted(uq, vals[v][fin])
    return out


# ---- shared case builders (the CPU self-checks and the GPU tests use the same inputs) ---
PANEL_NS = (16, 17, 40, 511, 512, 513, 600)     # 513, 600: the two-pass kernel (N > 512)
PANEL_PS = (1, 33, 64, 65, 129)
PANEL_BT = ((2, 13), (5, 2), (3, 1))


def panel_cases():
    """Every N x P once; Pw in {P, P + 1}, (B, TH) and the row scale cycle so that each N (and
    each kernel form) meets every value of them."""
    out = []
    for iN, N in enumerate(PANEL_NS):
        for iP, P in enumerate(PANEL_PS):
            k = iN * len(PANEL_PS) + iP
            B, TH = PANEL_BT[k % 3]
            out.append(dict(N=N, P=P, Pw=P + k % 2, B=B, TH=TH, rs=bool((k // 2) % 2), k=k))
    return out


def panel_case(N, P, Pw, B, TH, rs, k, offset=False, R=700):
    """Operands of one standardisation case.  F [R + 1, P + 2]: P real columns, two NaN columns
    behind them (never to be read), last row all zero (the pad row); n_real per month cycles
    through 2, N - 5, N; pad rows of idx point at the zero row.  ``offset``: columns with a
    large common offset (1e6 + randn) and tiny ones (1e-6 randn)."""
    rng = np.random.default_rng(1000 + k)
    F = np.full((R + 1, P + 2), np.nan)
    F[:R, :P] = rng.standard_normal((R, P))
    if offset:
        for c in range(1, P, 3):
            F[:R, c] += 1e6
        for c in range(2, P, 3):
            F[:R, c] *= 1e-6
    F[R, :P] = 0.0
    vol = rng.uniform(0.5, 2.0, R + 1)
    vol[R] = 1.0
    n_real = np.asarray([(2, N - 5, N)[(b + k) % 3] for b in range(B)], np.int32)
    idx = np.full((B, TH, N), R, np.int64)
    for b in range(B):
        for th in range(TH):
            idx[b, th, :n_real[b]] = rng.choice(R, n_real[b], replace=False)
    mask = (np.arange(N)[None, :] < n_real[:, None]).astype(np.float64)
    row_scale = rng.uniform(0.5, 2.0, (B, N)) if rs else None
    return dict(F=F, idx=idx, n_real=n_real, vol=vol, mask=mask, row_scale=row_scale,
                P=P, Pw=Pw, B=B, TH=TH, N=N)


# (un of the date, excluded rows) of the TH = 3 tiles of every month: the tiles of one month
# keep the same number of rows (n_real is per month); tiles repeating a date share its slot
EXCL_DATES = (1, 16, 17, 128, 129, 300, 600)
EXCL_TILES = (((16, 0), (17, 1), (17, 1)),
              ((128, 16), (129, 17), (128, 16)),
              ((128, 15), (129, 16), (129, 16)),
              ((300, 40), (300, 40), (300, 40)),
              ((600, 40), (600, 40), (600, 40)),
              ((600, 0), (600, 0), (600, 0)),
              ((300, 1), (300, 1), (300, 1)),
              ((129, 1), (128, 0), (129, 1)))


def excl_case(P, umax=600, seed=7, R=900):
    """Operands of date_sums + excl_stats: one date per un in EXCL_DATES (un <= umax), the
    tiles of EXCL_TILES whose dates exist.  Every tile's excluded set is drawn afresh; the
    first and every third tile with en > 0 exclude U(d)'s first row (the row that supplies K).
    ``kept``: per tile the panel rows of U(d) minus the excluded ones, in U(d)'s order."""
    rng = np.random.default_rng(seed + P)
    Pw = P + 1
    F = np.full((R + 1, P + 2), np.nan)                  # row R: all NaN, the pad slots' target
    F[:R, :P] = rng.standard_normal((R, P))
    F[:R, 1:P:4] += 1e3                                  # columns with a common offset
    dates = [u for u in EXCL_DATES if u <= umax]
    un = np.asarray(dates, np.int32)
    urows = np.full((len(dates), umax), R, np.int64)     # pad slots: never to be read
    for d, u in enumerate(dates):
        urows[d, :u] = rng.choice(R, u, replace=False)
    tiles = [t for t in EXCL_TILES if all(u in dates for u, _ in t)]
    B, TH = len(tiles), 3
    emax = 40
    erows = np.full((max(B, 1) * TH, emax), R, np.int64)
    en = np.zeros(B * TH, np.int32)
    dpos = np.zeros(B * TH, np.int32)
    n_real = np.zeros(B, np.int32)
    kept, k0 = [], 0
    for b, t in enumerate(tiles):
        for th, (u, e) in enumerate(t):
            bt, d = b * TH + th, dates.index(u)
            pos = rng.choice(u, e, replace=False)
            if e and k0 % 3 == 0 and 0 not in pos:
                pos[0] = 0
            k0 += 1 if e else 0
            erows[bt, :e] = urows[d, pos]
            en[bt], dpos[bt] = e, d
            kept.append(np.delete(urows[d, :u], pos))
            assert len(kept[-1]) >= 2
        n_real[b] = t[0][0] - t[0][1]
        assert all(u - e == n_real[b] for u, e in t)
    return dict(F=F, P=P, Pw=Pw, urows=urows, un=un, umax=umax, erows=erows, en=en, dpos=dpos,
                n_real=n_real, B=B, TH=TH, kept=kept)


SCORE_SHAPES = ((300, 2, 4, 101, 1), (700, 1, 4, 101, 0), (640, 2, 4, 101, 1))  # ..., frame


def scores_case(nV, G, nP, L, frame, compat, seed=3):
    """obj [nV, G, nP, L] = 1 + randn (means well away from zero: the relative bound then holds
    row by row) with NaN runs placed by the frame's own row numbering r = v * k + kk and its
    chunk length ceil(R / 64), each in a column of its own:
      c0 first row of a chunk; c1 last row of a chunk; c2 from mid-chunk across two whole
      chunks into the next; c3 the first 25 rows; c4 every row; c5 the last row of the frame;
      c6 a copy of c2 and c7 a copy of c3 (exact ties with NaN runs); c9 a copy of c8 (ties)."""
    rng = np.random.default_rng(seed + nV)
    obj = 1.0 + rng.standard_normal((nV, G, nP, L))
    g0, k = (0, frame + 1) if compat else (frame, 1)
    R = nV * k
    ch = (R + 63) // 64
    flat = obj.reshape(nV, G, nP * L)

    def put(rows, c):
        rows = np.asarray(rows)
        flat[rows // k, g0 + rows % k, c] = np.nan

    put([3 * ch], 0)
    put([4 * ch - 1], 1)
    put(np.arange(5 * ch + ch // 2, 8 * ch + 2), 2)
    put(np.arange(25), 3)
    put(np.arange(R), 4)
    put([R - 1], 5)
    flat[:, :, 6] = flat[:, :, 2]
    flat[:, :, 7] = flat[:, :, 3]
    flat[:, :, 9] = flat[:, :, 8]
    return obj
