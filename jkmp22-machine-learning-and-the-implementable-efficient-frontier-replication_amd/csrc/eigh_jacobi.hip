// Batched symmetric eigensolver for positive semi-definite A [B, N, N] in fp64: one-sided
// (Hestenes) Jacobi, the device root of the m_func repair (ops/linalg.py eigh_psd).
//
// State: two [B, N, N] buffers G and Vt whose ROW j is column j of the mathematical G and V.
// G starts as A (symmetric: its rows are its columns), Vt as I.  A rotation of the column pair
// (p, q) makes g_p and g_q orthogonal and applies the same rotation to v_p, v_q, so G = A V
// throughout; at convergence the rows of G are mutually orthogonal, |e_j| = |g_j| and row j of
// Vt is the eigenvector.  Nothing is ever squared: cond(A) up to 1e16 is fine, where the
// inverse-based square root of A^2 + 4A is not.
//
// Ordering.  The columns are cut into blocks of W; the nbe blocks (nbe even: a phantom block
// beyond N when the count is odd) meet in the round-robin tournament
//
//     round r, pair 0:      (r, nbe - 1)
//     round r, pair k > 0:  ((r + k) mod (nbe - 1), (r - k) mod (nbe - 1))
//
// nbe - 1 rounds of nbe / 2 disjoint block pairs.  One launch per round, grid (pairs, B); the
// kernel boundaries are the only synchronisation between workgroups (no atomics, no cooperative
// launch).  A workgroup loads its pair's 2 W rows of G and Vt into LDS and runs the column
// pairs there, one pair per wave per inner round, a barrier between inner rounds:
//   * round 0 (``full``): the same tournament over the 2 W local columns - the pairs inside
//     each block and the cross pairs;
//   * other rounds: the W x W cross pairs only (inner round i pairs local column k of the first
//     block with column (k + i) mod W of the second).
// So every column pair is visited exactly once per sweep.  Columns >= N are skipped.
//
// A pair rotates only when |g_p . g_q| > tol |g_p| |g_q| (tol = N u); a pair under the
// threshold is not written, and a workgroup that rotated nothing stores nothing, so further
// sweeps leave a converged matrix bitwise unchanged.  Two additions keep a SINGULAR A within
// the sweep limit (its null-space columns only shrink by a constant factor per sweep, and the
// others cannot settle before they are gone; in the numpy model, tests/jacobi_ref.py, at rank
// N / 2: 32 sweeps at N = 128 plain against 14; at N = 496, 29 with the interchange alone and
// 19 with both):
//   * the longer of the two rotated columns is stored first (de Rijk's interchange);
//   * a column with |g| <= tol max_j |a_j| (<= N u |A|_2: zero to the accuracy the solver
//     claims) is left alone.  By the symmetry of A the component of any other g_p along its
//     v_q is v_q' A v_p = g_q . v_p, at most |g_q|, so the residual of the others moves by no
//     more than that floor.  (x of m_func at wealth 1 has cond 1e10: no such column.)
// Every dot product is lanes strided over the row and an xor butterfly: a fixed order, so a
// matrix's result does not depend on the batch around it.
//
// Each workgroup leaves the largest |g_p . g_q| / (|g_p| |g_q|) it met (before rotating) in
// its [B, pairs] slot, NaN-propagating; round 0 overwrites the slot, the later rounds of the
// sweep fold into it.  ``skip[b] != 0``: matrix b is left alone (converged, or refused for a
// non-finite entry - the kernel never iterates on such data).
#include "common.h"

namespace {

__device__ __forceinline__ double nan_max(double a, double b) {
  return (a != a) ? a : (!(b <= a) ? b : a);
}

// W: block columns (= waves per workgroup); NC: row capacity (N <= NC, a multiple of 64)
template <int W, int NC>
__global__ __launch_bounds__(64 * W) void eigh_round_kernel(
    double* __restrict__ G, double* __restrict__ Vt, int N, int nbe, int round, int full,
    const int* __restrict__ skip, const double* __restrict__ floor2, double tol,
    double* __restrict__ meas) {
  constexpr int M = 2 * W, R = NC / 64;
  __shared__ double sG[M * NC];
  __shared__ double sV[M * NC];
  __shared__ double red[W];
  __shared__ int anyrot;
  const int b = blockIdx.y, k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (skip[b]) return;
  const int m1 = nbe - 1;
  int I, J;
  if (k == 0) {
    I = round;
    J = m1;
  } else {
    I = (round + k) % m1;
    J = (round - k + m1) % m1;
  }
  if (I > J) {
    const int t = I;
    I = J;
    J = t;
  }
  // (only cross pairs with a phantom block: nothing to visit, the slot keeps its value)
  if (!full && J * W >= N) return;
  double* Gb = G + (int64_t)b * N * N;
  double* Vb = Vt + (int64_t)b * N * N;
  if (threadIdx.x == 0) anyrot = 0;
  for (int r = wave; r < M; r += W) {
    const int gr = r < W ? I * W + r : J * W + r - W;
    if (gr < N)
      for (int j = lane; j < N; j += 64) {
        sG[r * NC + j] = Gb[(int64_t)gr * N + j];
        sV[r * NC + j] = Vb[(int64_t)gr * N + j];
      }
  }
  __syncthreads();
  double wmax = 0.0;
  const double fl2 = floor2[b];
  const int nin = full ? M - 1 : W;
  for (int ir = 0; ir < nin; ++ir) {
    int lp, lq;
    if (!full) {
      lp = wave;
      lq = W + (wave + ir) % W;
    } else if (wave == 0) {
      lp = ir;
      lq = M - 1;
    } else {
      lp = (ir + wave) % (M - 1);
      lq = (ir - wave + M - 1) % (M - 1);
    }
    if (lp > lq) {
      const int t = lp;
      lp = lq;
      lq = t;
    }
    const int gp_row = lp < W ? I * W + lp : J * W + lp - W;
    const int gq_row = lq < W ? I * W + lq : J * W + lq - W;
    if (gp_row < N && gq_row < N) {
      double* pg = sG + lp * NC;
      double* qg = sG + lq * NC;
      double gp[R], gq[R];
      double app = 0.0, aqq = 0.0, apq = 0.0;
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int j = lane + 64 * i;
        const bool in = j < N;
        gp[i] = in ? pg[j] : 0.0;
        gq[i] = in ? qg[j] : 0.0;
        app += gp[i] * gp[i];
        aqq += gq[i] * gq[i];
        apq += gp[i] * gq[i];
      }
      app = wave_sum(app);
      aqq = wave_sum(aqq);
      apq = wave_sum(apq);
      // (a column at or under the floor is zero to working accuracy and left alone - a zero
      // column among them: no 0 / 0; a NaN fails every comparison and stays a NaN)
      const double rel = (apq == 0.0 || app <= fl2 || aqq <= fl2)
                             ? 0.0 : fabs(apq) / (sqrt(app) * sqrt(aqq));
      wmax = nan_max(wmax, rel);
      if (rel > tol) {
        const double zeta = (aqq - app) / (2.0 * apq);
        const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        // the longer rotated column goes first (de Rijk's interchange): columns of a singular
        // A sort towards the end, where the plain ordering needs 2-3 times the sweeps
        const bool swap = aqq + t * apq > app - t * apq;
        double* pv = sV + (swap ? lq : lp) * NC;
        double* qv = sV + (swap ? lp : lq) * NC;
        double* pw = swap ? qg : pg;
        double* qw = swap ? pg : qg;
        const double* pr = sV + lp * NC;
        const double* qr = sV + lq * NC;
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const int j = lane + 64 * i;
          if (j < N) {
            pw[j] = c * gp[i] - s * gq[i];
            qw[j] = s * gp[i] + c * gq[i];
            const double vp = pr[j], vq = qr[j];
            pv[j] = c * vp - s * vq;
            qv[j] = s * vp + c * vq;
          }
        }
        if (lane == 0) anyrot = 1;
      }
    }
    __syncthreads();
  }
  if (lane == 0) red[wave] = wmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = red[0];
#pragma unroll
    for (int i = 1; i < W; ++i) m = nan_max(m, red[i]);
    double* slot = meas + (int64_t)b * gridDim.x + k;
    *slot = full ? m : nan_max(*slot, m);
  }
  if (!anyrot) return;
  for (int r = wave; r < M; r += W) {
    const int gr = r < W ? I * W + r : J * W + r - W;
    if (gr < N)
      for (int j = lane; j < N; j += 64) {
        Gb[(int64_t)gr * N + j] = sG[r * NC + j];
        Vb[(int64_t)gr * N + j] = sV[r * NC + j];
      }
  }
}

// floor2[b] = (tol max_j |a_j|)^2 over the rows of A[b] (max_j |a_j| <= |A|_2): one workgroup
// per matrix, a wave per row (lanes strided, butterfly), then the waves' maxima in index order.
__global__ __launch_bounds__(256) void eigh_floor_kernel(const double* __restrict__ A, int N,
                                                         double tol, double* __restrict__ floor2) {
  __shared__ double red[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* Ab = A + (int64_t)b * N * N;
  double m = 0.0;
  for (int r = wave; r < N; r += 4) {
    double s = 0.0;
    for (int j = lane; j < N; j += 64) s += Ab[(int64_t)r * N + j] * Ab[(int64_t)r * N + j];
    m = nan_max(m, wave_sum(s));
  }
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) m = nan_max(m, red[i]);
    floor2[b] = tol * tol * m;
  }
}

// One wave per column j: e_j = |g_j| with the sign of v_j . g_j (a rounding-level negative
// eigenvalue of a PSD input comes back negative, not folded), and optionally
// f_j = 2 / (x + 2 + sqrt(x^2 + 4 x)), x = max(e_j, 0): the k-scale of m_tilde_0 = V f(E) V'.
// f has an infinite slope at 0 (f ~ 1 - sqrt(x)), so a column under the sweeps' floor - an
// eigenvalue that is zero to working accuracy - takes x = 0: f = 1, not 1 - sqrt(noise).
// The floor is relative to |A|_2 and f depends on the absolute e: f is V f(E) V''s scale only
// for cond(A) < 1 / (N u), or where the columns under the floor are exact zeros
// (ops/linalg.py m_tilde0_eig states the condition).
__global__ __launch_bounds__(256) void eigh_finish_kernel(
    const double* __restrict__ G, const double* __restrict__ Vt, int N,
    const double* __restrict__ floor2, double* __restrict__ e, double* __restrict__ f) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= N) return;
  const double* g = G + ((int64_t)b * N + j) * N;
  const double* v = Vt + ((int64_t)b * N + j) * N;
  double gg = 0.0, vg = 0.0;
  for (int i = lane; i < N; i += 64) {
    gg += g[i] * g[i];
    vg += v[i] * g[i];
  }
  gg = wave_sum(gg);
  vg = wave_sum(vg);
  if (lane == 0) {
    double ev = sqrt(gg);
    if (vg < 0.0) ev = -ev;
    e[(int64_t)b * N + j] = ev;
    if (f) {
      const double x = gg <= floor2[b] ? 0.0 : ev > 0.0 ? ev : (ev != ev ? ev : 0.0);
      f[(int64_t)b * N + j] = 2.0 / (x + 2.0 + sqrt(x * x + 4.0 * x));
    }
  }
}

constexpr int W_SMALL_MAX_N = 576, MAX_N = 1152;

int block_cols(int N) { return N <= W_SMALL_MAX_N ? 8 : 4; }

int row_cap(int N) { return N <= 128 ? 128 : N <= 256 ? 256 : N <= W_SMALL_MAX_N ? 576 : 1152; }

int even_blocks(int N) {
  const int w = block_cols(N), nb = (N + w - 1) / w;
  return nb + (nb & 1);
}

template <int W, int NC>
void launch_round(double* G, double* Vt, int B, int N, int round, const int* skip,
                  const double* floor2, double tol, double* meas, hipStream_t st) {
  const int nbe = even_blocks(N);
  hipLaunchKernelGGL((eigh_round_kernel<W, NC>), dim3(nbe / 2, B), dim3(64 * W), 0, st, G, Vt, N,
                     nbe, round, round == 0 ? 1 : 0, skip, floor2, tol, meas);
}

}  // namespace

// Largest N, block width, block rounds per sweep and block pairs per round of the instance
// that serves N (0 where N is not served).
extern "C" int pfml_eigh_psd_max_n() { return MAX_N; }
extern "C" int pfml_eigh_psd_block_cols(int N) { return N < 1 || N > MAX_N ? 0 : block_cols(N); }
extern "C" int pfml_eigh_psd_rounds(int N) { return N < 1 || N > MAX_N ? 0 : even_blocks(N) - 1; }
extern "C" int pfml_eigh_psd_pairs(int N) { return N < 1 || N > MAX_N ? 0 : even_blocks(N) / 2; }

// Static LDS of the round kernel's instance for N: 2 W rows of G and of Vt at the instance's
// row capacity, plus the reduction scratch (-1 where N is not served).
extern "C" int64_t pfml_eigh_psd_lds_bytes(int N) {
  if (N < 1 || N > MAX_N) return -1;
  const int w = block_cols(N);
  return (int64_t)2 * 2 * w * row_cap(N) * 8 + 8 * w + 4;
}

// floor2 [B] = (tol max_j |a_j|)^2 of A [B, N, N] (contiguous), the round kernel's
// negligible-column floor.
extern "C" hipError_t pfml_eigh_psd_floor(const double* A, int B, int N, double tol,
                                          double* floor2, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (N < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(eigh_floor_kernel, dim3(B), dim3(256), 0, st, A, N, tol, floor2);
  return hipGetLastError();
}

// One block round (0 <= round < pfml_eigh_psd_rounds(N)) of a sweep over G, Vt [B, N, N]
// (contiguous); skip [B] int32; floor2 [B]; meas [B, pfml_eigh_psd_pairs(N)] doubles.
extern "C" hipError_t pfml_eigh_psd_round(double* G, double* Vt, int B, int N, int round,
                                          const int* skip, const double* floor2, double tol,
                                          double* meas, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (N < 1 || N > MAX_N || round < 0 || round >= even_blocks(N) - 1 || B > 65535)
    return hipErrorInvalidValue;
  switch (row_cap(N)) {
    case 128: launch_round<8, 128>(G, Vt, B, N, round, skip, floor2, tol, meas, st); break;
    case 256: launch_round<8, 256>(G, Vt, B, N, round, skip, floor2, tol, meas, st); break;
    case 576: launch_round<8, 576>(G, Vt, B, N, round, skip, floor2, tol, meas, st); break;
    default: launch_round<4, 1152>(G, Vt, B, N, round, skip, floor2, tol, meas, st); break;
  }
  return hipGetLastError();
}

// e [B, N] signed eigenvalues from the converged G, Vt; floor2 [B] as in the rounds; f [B, N]
// (may be null): f(e) above.
extern "C" hipError_t pfml_eigh_psd_finish(const double* G, const double* Vt, int B, int N,
                                           const double* floor2, double* e, double* f,
                                           hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (N < 1 || B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(eigh_finish_kernel, dim3((N + 3) / 4, B), dim3(256), 0, st, G, Vt, N,
                     floor2, e, f);
  return hipGetLastError();
}
