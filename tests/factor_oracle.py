"""References for the factor-structured solves (pfml.ops.factor_solve): sequential
``np.longdouble`` code, and the same Woodbury formula evaluated sequentially in fp64 numpy whose
error against the long-double solve sets the scale of the device's bound.

The systems are ``(X F_s X' + diag(d)) w = b``.  Inputs follow the synthetic spectra of
BASELINE.md: loadings N(0, 1), F the sample covariance of N(0, 1) draws times 1e-4 * 21, ivol =
U(0.01, 0.03)^2 * 21, lambda = 0.2 / U(1e7, 1e9), wealth 1e10, gamma 10.
"""
import numpy as np
import torch

LD = np.longdouble
U = 2.0 ** -53
GAMMA, WEALTH = 10.0, 1e10
N_VARIANTS = 4


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def ragged_rows(N, B):
    """n_rows of B months: N first, then 1, then sizes in between, N again last."""
    pool = [N, 1, max(1, N // 2), max(1, N - 1), N]
    return np.asarray([pool[t % len(pool)] for t in range(B)], np.int32)


def factor_inputs(N, K, B, A, seed, zero_factor=None, f_zero=False):
    """One launch's operands as numpy arrays (dict).  Variants (rows of d, fscale):
    0 Markowitz (gamma Sigma), 1 Static-ML (gamma Sigma + W Lambda), 2 minimum variance (Sigma),
    3 Static-ML with the cov_add shrinkage g = 2.  Arm a uses variant a % 4: rhs = mu_hat (0, 1,
    3), c = W Lambda (1, 3) or 0, rhs = 1 with the normalize flag (2).  X is a table of N + 13
    rows that every month indexes through its own permutation.  ``zero_factor``: that factor's
    row and column of F are 0; ``f_zero``: F = 0."""
    rng = np.random.default_rng(seed)
    V = N_VARIANTS
    R = N + 13
    X = rng.standard_normal((R, K))
    F = np.empty((B, K, K))
    for t in range(B):
        Z = rng.standard_normal((max(3 * K, 60), K))
        F[t] = np.atleast_2d(np.cov(Z, rowvar=False)) * 1e-4 * 21
    if zero_factor is not None:
        F[:, zero_factor, :] = 0.0
        F[:, :, zero_factor] = 0.0
    if f_zero:
        F[:] = 0.0
    ridx = np.stack([rng.permutation(R)[:N] for _ in range(B)]).astype(np.int64) \
        if B else np.zeros((0, N), np.int64)
    n_rows = ragged_rows(N, B)
    ivol = rng.uniform(0.01, 0.03, (B, N)) ** 2 * 21
    lam = 0.2 / rng.uniform(1e7, 1e9, (B, N))
    wl = WEALTH * lam
    Xg = X[ridx]                                                      # [B, N, K]
    diag_sigma = np.einsum("bnk,bkl,bnl->bn", Xg, F, Xg) + ivol
    d = np.stack([GAMMA * ivol, GAMMA * ivol + wl, ivol,
                  GAMMA * (ivol + 2.0 * diag_sigma) + wl])
    fscale = np.asarray([GAMMA, GAMMA, 1.0, GAMMA])
    varm = np.arange(A) % V
    mu = 0.01 * rng.standard_normal((A, B, N))
    rhs = np.where((varm == 2)[:, None, None], 1.0, mu)
    c = np.where(np.isin(varm, (1, 3))[:, None, None], wl[None], 0.0)
    normalize = varm == 2
    grow = rng.uniform(0.9, 1.1, (B, N))
    nmap = rng.integers(0, N, (B, N), dtype=np.int64)
    hit = (rng.random((B, N)) >= 0.1).astype(np.float64)
    live = np.arange(N)[None, :] < n_rows[:, None]
    grow = np.where(live, grow, 1.0)
    ws0 = 0.01 * rng.standard_normal((A, N))
    return dict(X=X, ridx=ridx, F=F, fscale=fscale, d=d, n_rows=n_rows, rhs=rhs, c=c,
                varm=varm, normalize=normalize, grow=grow, nmap=nmap, hit=hit, ws0=ws0,
                N=N, K=K, B=B, A=A, V=V, R=R)


def month_system(inp, v, t):
    """(X [n, K], F_s [K, K], d [n]) of system (v, t), fp64."""
    n = int(inp["n_rows"][t])
    X = inp["X"][inp["ridx"][t, :n]]
    return X, inp["fscale"][v] * inp["F"][t], inp["d"][v, t, :n]


# ---------------------------------------------------------------------------------------------
# long double
# ---------------------------------------------------------------------------------------------
def ld_solve(A, Bm):
    """Gaussian elimination with partial pivoting in longdouble (small systems)."""
    A = np.array(A, LD)
    Bm = np.array(Bm, LD)
    one_d = Bm.ndim == 1
    if one_d:
        Bm = Bm[:, None]
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            Bm[[k, p]] = Bm[[p, k]]
        l = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= l[:, None] * A[k, k:][None, :]
        Bm[k + 1:] -= l[:, None] * Bm[k][None, :]
    for k in range(n - 1, -1, -1):
        Bm[k] = (Bm[k] - A[k, k + 1:] @ Bm[k + 1:]) / A[k, k]
    return Bm[:, 0] if one_d else Bm


def ld_gram(X, d):
    """G = X' diag(1/d) X, rows added one by one in longdouble."""
    K = X.shape[1]
    G = np.zeros((K, K), LD)
    Xl, dl = X.astype(LD), d.astype(LD)
    for i in range(X.shape[0]):
        G += np.outer(Xl[i], Xl[i] / dl[i])
    return G


def ld_matmul(Aa, Bb):
    out = np.zeros((Aa.shape[0], Bb.shape[1]), LD)
    for l in range(Aa.shape[1]):
        out += np.outer(Aa[:, l], Bb[l])
    return out


def m_ref(X, Fs, d):
    """(I + F_s G)^-1 F_s in longdouble."""
    K = X.shape[1]
    Fl = Fs.astype(LD)
    return ld_solve(np.eye(K, dtype=LD) + ld_matmul(Fl, ld_gram(X, d)), Fl)


def ld_apply(X, Fs, d, w):
    """(X F_s X' + diag(d)) w in longdouble, through the factors (no n x n product)."""
    Xl, wl = X.astype(LD), np.asarray(w, LD)
    tau = np.zeros(X.shape[1], LD)
    for i in range(X.shape[0]):
        tau += Xl[i] * wl[i]
    s = np.zeros(X.shape[1], LD)
    Fl = Fs.astype(LD)
    for l in range(X.shape[1]):
        s += Fl[:, l] * tau[l]
    out = d.astype(LD) * wl
    for k in range(X.shape[1]):
        out += Xl[:, k] * s[k]
    return out


def explicit_matrix_ld(X, Fs, d):
    """X F_s X' + diag(d) as a longdouble [n, n] matrix (small n only)."""
    Xl = X.astype(LD)
    return ld_matmul(ld_matmul(Xl, Fs.astype(LD)), Xl.T.copy()) + np.diag(d.astype(LD))


class DenseSolver:
    """Long-double solves of one system's explicit matrix ``X F_s X' + diag(d)``: the matrix
    is formed and LU-factored in fp64 once, every solve is then refined with longdouble
    residuals until the correction is below 1e-18 of the solution.  The residual applies the
    same matrix through its factors in longdouble (``ld_apply``; equal to the product with
    ``explicit_matrix_ld``, checked at small n in test_factor_solve_cpu.py)."""

    def __init__(self, X, Fs, d):
        self.X, self.Fs, self.d = X, Fs, d
        S = X @ Fs @ X.T + np.diag(d)
        self.lu = torch.linalg.lu_factor(torch.as_tensor(S))

    def _f64(self, r):
        rt = torch.as_tensor(np.asarray(r, np.float64))[:, None]
        return torch.linalg.lu_solve(*self.lu, rt)[:, 0].numpy()

    def solve(self, b, iters=8):
        b = np.asarray(b, LD)
        x = self._f64(b).astype(LD)
        for _ in range(iters):
            r = b - ld_apply(self.X, self.Fs, self.d, x)
            dx = self._f64(r).astype(LD)
            x = x + dx
            if float(np.max(np.abs(dx))) <= 1e-18 * float(np.max(np.abs(x))):
                return x
        raise AssertionError("iterative refinement did not converge")


# ---------------------------------------------------------------------------------------------
# the same Woodbury formula, sequential fp64 numpy
# ---------------------------------------------------------------------------------------------
def woodbury_m_f64(X, Fs, d):
    K = X.shape[1]
    G = np.zeros((K, K))
    for i in range(X.shape[0]):
        G += np.outer(X[i], X[i] / d[i])
    Amat = np.zeros((K, K))
    for l in range(K):
        Amat += np.outer(Fs[:, l], G[l])
    return np.linalg.solve(Amat + np.eye(K), Fs)


def woodbury_w_f64(X, M, d, b):
    u = b / d
    tau = np.zeros(X.shape[1])
    for i in range(X.shape[0]):
        tau += X[i] * u[i]
    s = np.zeros(X.shape[1])
    for l in range(X.shape[1]):
        s += M[:, l] * tau[l]
    acc = np.zeros(X.shape[0])
    for k in range(X.shape[1]):
        acc += X[:, k] * s[k]
    return u - acc / d


# ---------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------
class Reference:
    """The shared, read-only references of one set of inputs: per system the longdouble M, the
    fp64 oracle M and a DenseSolver, built on first use."""

    def __init__(self, inp):
        self.inp = inp
        self._m, self._mo, self._solver = {}, {}, {}

    def m(self, v, t):
        if (v, t) not in self._m:
            X, Fs, d = month_system(self.inp, v, t)
            self._m[v, t] = m_ref(X, Fs, d)
            self._mo[v, t] = woodbury_m_f64(X, Fs, d)
        return self._m[v, t], self._mo[v, t]

    def solver(self, v, t):
        if (v, t) not in self._solver:
            self._solver[v, t] = DenseSolver(*month_system(self.inp, v, t))
        return self._solver[v, t]


def check_m(ref, M, systems=None):
    """Device M [V, B, K, K] (numpy) against the longdouble M: error at most 8 x the fp64
    oracle's + (N + K) u max|M|.  Returns (worst error / bound, worst oracle relative error)."""
    inp = ref.inp
    worst, worst_o = 0.0, 0.0
    for v in range(inp["V"]):
        for t in range(inp["B"]):
            if systems is not None and (v, t) not in systems:
                continue
            m_ld, m_o = ref.m(v, t)
            scale = float(np.max(np.abs(m_ld)))
            e_o = float(np.max(np.abs(m_o.astype(LD) - m_ld)))
            e_d = float(np.max(np.abs(M[v, t].astype(LD) - m_ld)))
            bound = 8.0 * e_o + (int(inp["n_rows"][t]) + inp["K"]) * U * scale
            if scale > 0:
                worst_o = max(worst_o, e_o / scale)
            worst = max(worst, e_d / bound if bound > 0 else (0.0 if e_d == 0 else np.inf))
    return worst, worst_o


def check_chain(ref, Wst, Wopt, arms=None, months=None):
    """Every (arm, month) of a chain's outputs (numpy [A, B, N]) against the longdouble dense
    solve taken from the chain's own w_start of that month, so no error compounds: error at
    most 8 x that of the fp64 oracle formula + (n + K) u max|w|.  Returns (worst error /
    bound, worst oracle relative error)."""
    inp = ref.inp
    worst, worst_o = 0.0, 0.0
    for a in (range(inp["A"]) if arms is None else arms):
        v = int(inp["varm"][a])
        for t in (range(inp["B"]) if months is None else months):
            n = int(inp["n_rows"][t])
            X, Fs, d = month_system(inp, v, t)
            cc, rr = inp["c"][a, t, :n], inp["rhs"][a, t, :n]
            ws = Wst[a, t, :n]
            w_ld = ref.solver(v, t).solve(rr.astype(LD) + cc.astype(LD) * ws.astype(LD))
            w_o = woodbury_w_f64(X, ref.m(v, t)[1], d, np.where(cc != 0, rr + cc * ws, rr))
            if inp["normalize"][a]:
                w_ld = w_ld / np.sum(w_ld)
                w_o = w_o / np.sum(w_o)
            scale = float(np.max(np.abs(w_ld)))
            e_o = float(np.max(np.abs(w_o.astype(LD) - w_ld)))
            e_d = float(np.max(np.abs(Wopt[a, t, :n].astype(LD) - w_ld)))
            bound = 8.0 * e_o + (n + inp["K"]) * U * scale
            worst_o = max(worst_o, e_o / scale)
            worst = max(worst, e_d / bound)
            assert not np.any(Wopt[a, t, n:]), "padding columns of Wopt must stay 0"
    return worst, worst_o


def drift(Wopt_t, grow_t, nmap_t, hit_t):
    """The drift of portfolio._chain (torch or numpy operands)."""
    return (Wopt_t * grow_t)[..., nmap_t] * hit_t
