"""Longdouble references, fixed-seed cases and tolerance rules for the Barra risk kernels
(csrc/risk.hip: daily_ols_kernel, ewma_factor_cov_kernel, ewma_vol_kernel).

The references use numpy longdouble only (no torch, no GPU).  The ``*_expect`` helpers add what
the tolerance rules need: the error of the op's own fp64 CPU branch against the reference, per
day / month / case, computed once and shared by the CPU and GPU tests, which therefore see the
same inputs and the same bounds.

Tolerances follow ``oracle.panel_tol``: 8 x the fp64 CPU path's error against longdouble (for
partial-sum order and FMA contraction), floor 64 u.  For the OLS the floor carries the
first-order sensitivity of the solve: 64 u max(1, kappa_2(X'X)).
"""
import functools

import numpy as np

from factor_oracle import LD, ld_matmul, ld_solve
from oracle import U, panel_tol

# ---------------------------------------------------------------------------------------------
# daily OLS
# ---------------------------------------------------------------------------------------------
OLS_KS = (1, 2, 15, 16, 17, 25, 31)
CMP, EMPTY, UNDER, DUP, ZERO = "compared", "empty", "under-determined", "dup-column", "zero-column"


def ols_case(K):
    """One launch for width K: compared days of n in {K+1, 2K, 63, 64, 65, 127, 128, 129, 200,
    513} rows with a 0-row day, a 1-row day, a (K-1)-row day, a duplicated-column day and a
    zero-column day between them (the last two for K >= 2).  The first min(12, K-1) columns are
    0/1 industry dummies and every industry has a member on every day of at least that many
    rows.  ``kinds[d]`` names what day d is; under-determined days (0 < n < K) are the only ones
    a test does not compare.  ``special[d]`` = (DUP, kept, copy) or (ZERO, column).

    The duplicate is a copy of column 0 in the last column.  Column 0's largest entry in X'X
    is its own diagonal (tied with the twin row), so an LU with partial pivoting takes row 0 in
    its first step and the twin row is exactly zero from then on: the blocked LAPACK LU of the
    CPU branch meets the exact zero pivot as the kernel's unblocked LU does, and e_ref on that
    day is the error of the pinv route.  (With twins further right a blocked LU updates the two
    rows in different orders and may solve through rounding noise instead.)"""
    rng = np.random.default_rng(7100 + K)
    nd = min(12, K - 1)
    plan = [(K + 1, CMP), (0, EMPTY), (2 * K, CMP), (1, None), (63, CMP), (64, CMP),
            (K - 1, None), (65, CMP), (127, CMP)]
    if K >= 2:
        plan.append((90, DUP))
    plan += [(128, CMP), (129, CMP)]
    if K >= 2:
        plan.append((70, ZERO))
    plan += [(200, CMP), (513, CMP)]
    sizes, kinds = [], []
    for n, kind in plan:
        if kind is None:
            kind = EMPTY if n == 0 else (UNDER if n < K else CMP)
        assert (kind == UNDER) == (0 < n < K) and (kind == EMPTY) == (n == 0)
        sizes.append(n)
        kinds.append(kind)
    off = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    R = int(off[-1])
    X = rng.standard_normal((R, K))
    y = rng.standard_normal(R) * 0.02
    special = {}
    for d, (n, kind) in enumerate(zip(sizes, kinds)):
        a = int(off[d])
        if nd:
            ind = rng.integers(0, nd, n)
            m = min(n, nd)
            ind[:m] = rng.permutation(nd)[:m]          # every industry present when n >= nd
            X[a:a + n, :nd] = ind[:, None] == np.arange(nd)[None, :]
        if kind == DUP:
            X[a:a + n, K - 1] = X[a:a + n, 0]
            special[d] = (DUP, 0, K - 1)
        elif kind == ZERO:
            X[a:a + n, K - 1] = 0.0
            special[d] = (ZERO, K - 1)
    return {"K": K, "X": X, "y": y, "off": off, "sizes": sizes, "kinds": kinds,
            "special": special}


def _ols_day_ref(Xd, yd):
    Xl, yl = Xd.astype(LD), yd.astype(LD)
    G = ld_matmul(Xl.T, Xl)
    b = ld_matmul(Xl.T, yl[:, None])[:, 0]
    return ld_solve(G, b), float(np.linalg.cond(G.astype(np.float64)))


def ols_ref(X, y, off, special=None):
    """Per day G = X'X, b = X'y, coef = ld_solve(G, b), resid = y - X coef in longdouble, and
    kappa_2(G) rounded to fp64.  A day in ``special`` is exactly singular by construction and
    gets the minimum-norm solution without an SVD: the zero column (or one of the two equal
    columns) is dropped, the reduced system solved, the zero column's coefficient is 0 and the
    kept duplicate's coefficient is split equally between the two equal columns; kappa is the
    reduced Gram matrix's.  A 0-row day has coef 0; a day with 0 < n < K is not referenced (NaN).
    Returns (coef [D, K], resid [R], kappa [D])."""
    special = special or {}
    D, K = len(off) - 1, X.shape[1]
    coef = np.full((D, K), np.nan, LD)
    resid = np.full(len(y), np.nan, LD)
    kappa = np.full(D, np.nan)
    for d in range(D):
        a, b = int(off[d]), int(off[d + 1])
        Xd, yd = X[a:b], y[a:b]
        if b == a:
            coef[d] = 0
            continue
        if d in special:
            sp = special[d]
            drop = sp[2] if sp[0] == DUP else sp[1]
            keep = [j for j in range(K) if j != drop]
            c, kappa[d] = _ols_day_ref(Xd[:, keep], yd)
            coef[d] = 0
            coef[d, keep] = c
            if sp[0] == DUP:
                coef[d, sp[1]] = coef[d, sp[2]] = c[keep.index(sp[1])] / 2
        elif b - a >= K:
            coef[d], kappa[d] = _ols_day_ref(Xd, yd)
        else:
            continue
        resid[a:b] = yd.astype(LD) - ld_matmul(Xd.astype(LD), coef[d][:, None])[:, 0]
    return coef, resid, kappa


def ols_day_err(coef_d, ref_d):
    """max |coef - ref| / max |ref| of one day."""
    return float(np.abs(coef_d.astype(LD) - ref_d).max() / np.abs(ref_d).max())


def ols_tol(e_ref_d, kappa_d):
    return max(8.0 * e_ref_d, 64.0 * U * max(1.0, kappa_d))


@functools.lru_cache(maxsize=None)
def ols_expect(K):
    """The case for width K, its longdouble reference, the CPU branch's result and per-day
    error, and tol_d.  Days without a reference (UNDER) have NaN tolerances."""
    import torch
    from pfml.ops.risk_kernels import daily_ols
    c = ols_case(K)
    coef, resid, kappa = ols_ref(c["X"], c["y"], c["off"], c["special"])
    got, got_r, nbad, st = daily_ols(torch.tensor(c["X"]), torch.tensor(c["y"]),
                                     torch.tensor(c["off"]), return_status=True)
    got, got_r = got.numpy(), got_r.numpy()
    D = len(c["sizes"])
    e_ref, tol = np.full(D, np.nan), np.full(D, np.nan)
    for d in ols_checked_days(c):
        e_ref[d] = ols_day_err(got[d], coef[d])
        tol[d] = ols_tol(e_ref[d], kappa[d])
    return dict(c, coef=coef, resid=resid, kappa=kappa, cpu_coef=got, cpu_resid=got_r,
                cpu_nbad=nbad, cpu_status=st.numpy(), e_ref=e_ref, tol=tol)


def ols_checked_days(c):
    """Days whose coefficients are compared with the reference: all but the empty and the
    named under-determined ones."""
    return [d for d, k in enumerate(c["kinds"]) if k in (CMP, DUP, ZERO)]


def ols_check(ex, coef, resid, status, nbad, what=""):
    """Assert an OLS result against ``ols_expect(K)``; returns the largest error / tol_d."""
    c = ex
    X, y, off, K = c["X"], c["y"], c["off"], c["K"]
    worst = 0.0
    for d, kind in enumerate(c["kinds"]):
        a, b = int(off[d]), int(off[d + 1])
        tag = f"{what} K={K} day {d} ({kind}, n={b - a})"
        if kind == EMPTY:
            assert np.all(coef[d] == 0) and status[d] == 2, tag
            continue
        if kind == UNDER:
            assert np.all(np.isfinite(coef[d])) and np.all(np.isfinite(resid[a:b])), tag
            continue
        assert status[d] == (0 if kind == CMP else 2), f"{tag}: status {status[d]}"
        ref, tol = c["coef"][d], c["tol"][d]
        err = ols_day_err(coef[d], ref)
        worst = max(worst, err / tol)
        assert err <= tol, f"{tag}: coef error {err:.3e} > tol {tol:.3e} (kappa {c['kappa'][d]:.3g})"
        cmax = float(np.abs(ref).max())
        rb = tol * np.abs(X[a:b]).sum(1) * cmax + 8 * U * np.abs(y[a:b])
        dr = np.abs(resid[a:b].astype(LD) - c["resid"][a:b]).astype(np.float64)
        assert np.all(dr <= rb), f"{tag}: residual error / bound {np.max(dr / rb):.3g}"
    assert nbad == int((np.asarray(status) == 2).sum()), what
    return worst


def ols_self_consistent(X, y, off, coef, resid):
    """resid == y - X coef_returned within K 4u (|X| |coef| + |y|), row by row: the stored
    coefficients are the ones the residual loop used."""
    K = X.shape[1]
    for d in range(len(off) - 1):
        a, b = int(off[d]), int(off[d + 1])
        if b == a:
            continue
        r = y[a:b].astype(LD) - ld_matmul(X[a:b].astype(LD), coef[d].astype(LD)[:, None])[:, 0]
        bound = K * 4 * U * (np.abs(X[a:b]) @ np.abs(coef[d]) + np.abs(y[a:b]))
        dr = np.abs(resid[a:b].astype(LD) - r).astype(np.float64)
        assert np.all(dr <= bound), (d, float(np.max(dr / np.maximum(bound, 1e-300))))


# ---------------------------------------------------------------------------------------------
# EWMA factor covariance
# ---------------------------------------------------------------------------------------------
COV_KS = (1, 2, 16, 17, 25, 32)
COV_OBS = (64, 300)


def cov_case(K, obs):
    """days = obs + 70 of factor returns whose columns alternate between mean / sd = 100 and
    0.1 (sd 0.01), so a kernel that lost the two-pass centring would show; window ends at the
    chunk (64) and window (obs) edges and at the last day."""
    rng = np.random.default_rng(7200 + 10 * K + (obs == 64))
    days = obs + 70
    ratio = np.where((np.arange(K) + (obs == 64)) % 2 == 0, 100.0, 0.1)
    sd = 0.01
    fr = rng.standard_normal((days, K)) * sd + ratio[None, :] * sd
    tr = np.arange(obs, 0, -1, dtype=np.float64)
    w_cor = (0.5 ** (1 / 90.0)) ** tr
    w_var = (0.5 ** (1 / 30.0)) ** tr
    ends = []
    for e in (2, 5, 63, 64, 65, obs - 1, obs, obs + 1, days):
        if e not in ends:
            ends.append(e)
    return {"K": K, "obs": obs, "days": days, "fr": fr, "w_cor": w_cor, "w_var": w_var,
            "ends": np.array(ends, np.int64), "scale": 21.0}


def _cov_wt_ld(Xw, w):
    wn = w / w.sum()
    mu = (wn[:, None] * Xw).sum(0)
    Xc = (Xw - mu[None, :]) * np.sqrt(wn)[:, None]
    return ld_matmul(Xc.T, Xc) / (LD(1) - (wn * wn).sum())


def cov_ref(fr, ends, obs, w_cor, w_var, scale, nan_cor=True):
    """R's cov.wt(center = TRUE, method = 'unbiased') as ``weighted_cov_torch`` writes it, in
    longdouble: F = sd cor sd * scale with cor from w_cor and sd from w_var.  Returns
    (F, cor, var), each [B, K, K]."""
    fr, wc, wv = np.asarray(fr).astype(LD), np.asarray(w_cor).astype(LD), np.asarray(w_var).astype(LD)
    K = fr.shape[1]
    F, cor, var = (np.zeros((len(ends), K, K), LD) for _ in range(3))
    for b, e in enumerate(ends):
        t = min(int(obs), int(e))
        Xw = fr[int(e) - t:int(e)]
        with np.errstate(invalid="ignore", divide="ignore"):
            cc = _cov_wt_ld(Xw, wc[obs - t:])
            v = _cov_wt_ld(Xw, wv[obs - t:])
            s = np.sqrt(np.diagonal(cc))
            den = np.outer(s, s)
            if nan_cor:
                c = cc / den
            else:
                c = np.where(den > 0, cc / np.where(den > 0, den, 1), 0)
            c[np.arange(K), np.arange(K)] = 1
            sv = np.sqrt(np.diagonal(v))
            F[b] = sv[:, None] * c * sv[None, :] * LD(scale)
        cor[b], var[b] = c, v
    return F, cor, var


def cov_errs(F, cor, var, ref):
    """Per month: (max |dF| / max |F_ref|, max |dcor|, max |dvar| / max |var_ref|)."""
    Fr, cr, vr = ref
    out = np.zeros((len(Fr), 3))
    for b in range(len(Fr)):
        out[b, 0] = np.abs(F[b].astype(LD) - Fr[b]).max() / np.abs(Fr[b]).max()
        out[b, 1] = np.abs(cor[b].astype(LD) - cr[b]).max()
        out[b, 2] = np.abs(var[b].astype(LD) - vr[b]).max() / np.abs(vr[b]).max()
    return out


@functools.lru_cache(maxsize=None)
def cov_expect(K, obs):
    """Case, longdouble reference, the CPU branch's per-month errors and the tolerances."""
    import torch
    from pfml.ops.risk_kernels import ewma_factor_cov
    c = cov_case(K, obs)
    ref = cov_ref(c["fr"], c["ends"], obs, c["w_cor"], c["w_var"], c["scale"])
    got = ewma_factor_cov(torch.tensor(c["fr"]), c["ends"], obs, c["w_cor"], c["w_var"],
                          scale=c["scale"], return_parts=True)
    e_ref = cov_errs(*(g.numpy() for g in got), ref)
    tol = np.vectorize(panel_tol)(e_ref)
    return dict(c, ref=ref, e_ref=e_ref, tol=tol)


def cov_check(ex, F, cor, var, what=""):
    """Assert a covariance result against ``cov_expect``; returns the largest error / tol."""
    err = cov_errs(F, cor, var, ex["ref"])
    assert not np.isnan(err).any(), what
    bad = err > ex["tol"]
    assert not bad.any(), (f"{what} K={ex['K']} obs={ex['obs']}: (month, F/cor/var) "
                           f"{np.argwhere(bad).tolist()} err {err[bad]} tol {ex['tol'][bad]}")
    return float((err / ex["tol"]).max())


# ---------------------------------------------------------------------------------------------
# EWMA volatility
# ---------------------------------------------------------------------------------------------
VOL_STARTS = (2, 63, 64, 65, 130)
VOL_LAMS = (0.5 ** (1 / 126), 0.97, 0.5)


def vol_case(start, lam):
    """13 groups (not a multiple of the 4 waves of a workgroup): lengths 0, 1, start, start + 1,
    start + 2, start + 64, start + 65 (a full last chunk), start + 66, start + 700, then a
    group with one valid observation in its start window, one with a NaN at position start - 1,
    one with a NaN in its last row, and start + 129 (two full chunks).  5 % NaN elsewhere; the
    first two rows of every ordinary group stay valid so its start window has a variance."""
    rng = np.random.default_rng(7300 + start + int(round(lam * 1000)))
    sizes = [0, 1, start, start + 1, start + 2, start + 64, start + 65, start + 66, start + 700,
             start + 66, start + 65, start + 66, start + 129]
    gs = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    x = rng.standard_normal(gs[-1]) * 0.02
    x[rng.random(gs[-1]) < 0.05] = np.nan
    for g, n in enumerate(sizes):
        if n >= 2:
            x[gs[g]:gs[g] + 2] = rng.standard_normal(2) * 0.02
    x[gs[9]:gs[9] + start] = np.nan                    # one valid observation in the window
    x[gs[9] + start // 2] = 0.01
    x[gs[10] + start - 1] = np.nan
    x[gs[12] - 1] = np.nan                             # last row of group 11
    return {"start": start, "lam": lam, "x": x, "gs": gs, "sizes": sizes}


def vol_ref(x, gs, lam, start):
    """The sequential recurrence of runtime/panel.cpp::pfml_ewma_vol in longdouble:
    var[start] = sum of the valid x^2 of the first ``start`` rows / (count - 1), then
    var[i] = lam var[i-1] + (1 - lam) x[i-1]^2, carried over a NaN x[i-1]; NaN before ``start``
    and for a group of <= start rows or <= 1 valid row in its window."""
    out = np.full(len(x), np.nan, LD)
    xl, lam = np.asarray(x).astype(LD), LD(lam)
    for g in range(len(gs) - 1):
        a, b = int(gs[g]), int(gs[g + 1])
        if b - a <= start:
            continue
        win = xl[a:a + start]
        ok = ~np.isnan(win)
        if ok.sum() <= 1:
            continue
        var = (win[ok] * win[ok]).sum() / LD(int(ok.sum()) - 1)
        out[a + start] = np.sqrt(var)
        for i in range(a + start + 1, b):
            xp = xl[i - 1]
            if not np.isnan(xp):
                var = lam * var + (LD(1) - lam) * xp * xp
            out[i] = np.sqrt(var)
    return out


def vol_err(out, ref):
    """Largest relative error over the non-NaN outputs; the NaN masks must be equal."""
    assert np.array_equal(np.isnan(out), np.isnan(ref)), "NaN masks differ"
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    return float((np.abs(out[ok].astype(LD) - ref[ok]) / np.abs(ref[ok])).max())


@functools.lru_cache(maxsize=None)
def vol_expect(start, lam):
    from pfml import runtime as rt
    c = vol_case(start, lam)
    ref = vol_ref(c["x"], c["gs"], lam, start)
    e_ref = vol_err(rt.ewma_vol(c["x"], c["gs"], lam, start), ref)
    return dict(c, ref=ref, e_ref=e_ref, tol=panel_tol(e_ref))
