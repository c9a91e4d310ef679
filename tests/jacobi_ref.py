"""Sequential numpy model of the device eigensolver (csrc/eigh_jacobi.hip): the same one-sided
Jacobi - the same block tournament, the same inner ordering, the same rotation threshold -
one column pair at a time.  It is the model the GPU bounds of tests/test_gpu_eigh.py rest on
(its own figures: profiles/r12_eigh_jacobi.md), and it holds the input generators both test
files share.

    python tests/jacobi_ref.py 496            # figures of one size, the three spectra
    python tests/jacobi_ref.py --plain 128    # the same without the two additions
"""
import sys
import time

import numpy as np

U = 2.0 ** -53
W_SMALL_MAX_N, MAX_N = 576, 1152


def block_cols(N: int) -> int:
    return 8 if N <= W_SMALL_MAX_N else 4


def tournament(m: int, r: int, k: int) -> tuple[int, int]:
    """Pair k of round r of the round-robin over m (even) players, smaller index first."""
    if k == 0:
        p, q = r, m - 1
    else:
        p, q = (r + k) % (m - 1), (r - k + m - 1) % (m - 1)
    return (p, q) if p < q else (q, p)


def sweep_pairs(N: int, w: int | None = None):
    """Every column pair (p < q) of one sweep, in the device's order: block rounds, block pairs,
    inner rounds, waves.  (The device runs the pairs of an inner round at once: they are
    disjoint, so the sequential order inside it does not matter.)"""
    w = w or block_cols(N)
    nb = -(-N // w)
    nbe = nb + (nb & 1)
    m = 2 * w
    for rnd in range(nbe - 1):
        for k in range(nbe // 2):
            I, J = tournament(nbe, rnd, k)
            col = lambda l: I * w + l if l < w else J * w + l - w          # noqa: E731
            if rnd == 0:
                inner = [[tournament(m, ir, kk) for kk in range(w)] for ir in range(m - 1)]
            else:
                inner = [[(kk, w + (kk + ir) % w) for kk in range(w)] for ir in range(w)]
            for pairs in inner:
                for lp, lq in pairs:
                    p, q = col(lp), col(lq)
                    if p < N and q < N:
                        yield p, q


def jacobi_eigh(A: np.ndarray, max_sweeps: int = 30, w: int | None = None,
                plain: bool = False):
    """(e [N], Vt [N, N], sweeps, converged): rows of Vt are the eigenvectors of the symmetric
    PSD A, e_j = |g_j| with the sign of v_j . g_j.  ``plain``: without the kernel's two
    additions for singular matrices (the interchange and the negligible-column floor)."""
    N = A.shape[0]
    G = np.array(A, dtype=np.float64)
    Vt = np.eye(N)
    tol = N * U
    # (tol max_j |a_j|)^2: columns at or under it are negligible
    fl2 = -1.0 if plain else tol * tol * float((G * G).sum(1).max())
    order = list(sweep_pairs(N, w))
    assert len(order) == N * (N - 1) // 2 and len(set(order)) == len(order)
    sweeps, conv = 0, False
    while sweeps < max_sweeps and not conv:
        worst = 0.0
        for p, q in order:
            gp, gq = G[p], G[q]
            app, aqq, apq = gp @ gp, gq @ gq, gp @ gq
            if apq == 0.0 or app <= fl2 or aqq <= fl2:
                rel = 0.0
            else:
                rel = abs(apq) / (np.sqrt(app) * np.sqrt(aqq))
            if not rel <= worst:
                worst = rel
            if rel > tol:
                zeta = (aqq - app) / (2.0 * apq)
                with np.errstate(over="ignore"):
                    t = np.copysign(1.0, zeta) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                a, b = c * gp - s * gq, s * gp + c * gq
                va, vb = c * Vt[p] - s * Vt[q], s * Vt[p] + c * Vt[q]
                if not plain and aqq + t * apq > app - t * apq:     # the longer one first
                    a, b, va, vb = b, a, vb, va
                G[p], G[q], Vt[p], Vt[q] = a, b, va, vb
        sweeps += 1
        conv = bool(worst <= tol)
    e = np.sqrt((G * G).sum(1))
    e = np.where((Vt * G).sum(1) < 0.0, -e, e)
    return e, Vt, sweeps, conv


# ---------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------
def production_inputs(N: int, n: int, wealth, tc: bool = True, seed: int = 1, K: int = 25):
    """(sigma, lam, w, mask) of tests/test_gpu_pipeline.py::test_m_tilde_production_shape at
    width N with n real stocks (the rest padding), one matrix per entry of ``wealth``."""
    rng = np.random.default_rng(seed)
    w = np.atleast_1d(np.asarray(wealth, dtype=np.float64))
    B = len(w)
    K = min(K, max(n, 1))
    X = rng.normal(size=(B, N, K))
    X[:, n:] = 0.0
    F = np.stack([np.atleast_2d(np.cov(rng.normal(size=(K, 300)))) * 21e-4 for _ in range(B)])
    iv = rng.uniform(0.01, 0.03, (B, N)) ** 2 * 21
    iv[:, n:] = 1.0
    S = np.einsum("bik,bkl,bjl->bij", X, F, X) + np.stack([np.diag(v) for v in iv])
    lam = 0.2 / rng.uniform(1e7, 1e9, (B, N)) if tc else np.full((B, N), 1e-16)
    lam[:, n:] = 10.0 / w[:, None]
    mask = np.zeros((B, N))
    mask[:, :n] = 1.0
    return S, lam, w, mask


def real_rows(N: int) -> int:
    """Real stocks of a width-N month: N = 496 holds 489 (the production test's padding)."""
    return N if N < 4 else N - max(1, N // 70)


def production_x(N: int, wealth: float, tc: bool = True, seed: int = 1, gamma: float = 10.0):
    """x = (gamma / w) L^-1/2 Sigma L^-1/2 [N, N] of the production generator, exactly
    symmetric."""
    S, lam, w, _ = production_inputs(N, real_rows(N), [wealth], tc, seed)
    a = 1.0 / np.sqrt(lam[0])
    x = (gamma / w[0]) * S[0] * a[:, None] * a[None, :]
    return 0.5 * (x + x.T)


def gram_half_rank(N: int, seed: int = 2):
    """A random Gram matrix of rank N // 2: exact zero eigenvalues."""
    rng = np.random.default_rng(seed)
    Y = rng.normal(size=(N, N // 2))
    A = Y @ Y.T
    return 0.5 * (A + A.T)


def spectra(N: int):
    """The three matrices of one test batch."""
    return [production_x(N, 1.0), production_x(N, 1e10), gram_half_rank(N)]


def figures(A: np.ndarray, e: np.ndarray, Vt: np.ndarray) -> dict:
    """Residual and eigenvalue error in units of N u |A|_2, orthogonality in units of N u."""
    N = A.shape[0]
    ref = np.linalg.eigvalsh(A)
    nrm = max(np.abs(ref).max(), 1e-300)
    V = Vt.T
    return {"resid": float(np.abs(A @ V - V * e).max() / (N * U * nrm)),
            "orth": float(np.abs(V.T @ V - np.eye(N)).max() / (N * U)),
            "eig": float(np.abs(np.sort(e) - ref).max() / (N * U * nrm))}


if __name__ == "__main__":
    plain = "--plain" in sys.argv
    for N in [int(v) for v in sys.argv[1:] if v != "--plain"] or [1, 2, 7, 17, 40, 100]:
        for name, A in zip(("wealth 1", "wealth 1e10", "gram rank N/2"), spectra(N)):
            t0 = time.perf_counter()
            e, Vt, sweeps, conv = jacobi_eigh(A, max_sweeps=60 if plain else 30, plain=plain)
            f = figures(A, e, Vt)
            print(f"N = {N:4d}  {name:14s} sweeps {sweeps:2d} converged {conv}  "
                  f"resid {f['resid']:.3f}  orth {f['orth']:.3f}  eig {f['eig']:.3f}  "
                  f"({time.perf_counter() - t0:.1f} s)", flush=True)
