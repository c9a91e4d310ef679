// Solves with "factor part plus diagonal" for the benchmark portfolios (models/benchmarks.py):
//
//   (X F_s X' + diag(d)) w = b        X [n, K] Barra loadings, F_s = fscale F [K, K], d > 0
//
// by the Woodbury form that never builds an n x n matrix:
//
//   u = b / d,  G = X' diag(1/d) X,  M = (I + F_s G)^-1 F_s,  w = u - D^-1 X M (X' u)
//
// It stays valid when F has zero rows (exposure-less factors): no inverse of F is taken.
//
// factor_prepare_kernel: one workgroup per system s = (variant v, month t) -> M[s] and a status.
// factor_chain_kernel:   one workgroup per arm walks the B months in order; arms are
//                        independent, no workgroup waits for another and there are no atomics.
//
// X is read through the month's padded row index into the loading table both times; D^-1 X is
// never stored.  Every reduction over the month's rows has one order: thread t adds its rows
// t, t + 256, ... in that order, then a wave butterfly, then the four waves in index order.  A
// workgroup reads only its own system's / arm's operands, so every output is bitwise
// independent of the other systems or arms of the launch and of its position among them.
#include "common.h"

namespace {

constexpr int FT = 256;          // threads per workgroup
constexpr int FW = FT / 64;      // waves per workgroup
constexpr int KMAX = 64;         // factors
constexpr int NMAX = 4096;       // rows of a month held in LDS by the chain
constexpr int KC = 8;            // columns per thread and pass in the row reductions

__device__ __forceinline__ double butterfly(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_xor(v, off, PFML_WAVE));
  return v;
}

__device__ __forceinline__ int64_t clamp_row(int64_t r, int64_t R) {
  return r < 0 ? 0 : (r >= R ? R - 1 : r);
}

// status bits
constexpr int ST_ZERO_PIVOT = 1;
constexpr int ST_NONFINITE = 2;

__global__ __launch_bounds__(FT) void factor_prepare_kernel(
    const double* __restrict__ X, int64_t ldx, int64_t R, const int64_t* __restrict__ ridx,
    int64_t ldr, const double* __restrict__ F, const double* __restrict__ fscale,
    const double* __restrict__ d, int64_t ldd, const int* __restrict__ n_rows, int B, int N,
    int K, double* __restrict__ M, int* __restrict__ status) {
  // g: G, later the right-hand side F_s and the solution; a: the partial sums of the G pass,
  // later I + F_s G and its LU factors.  Row stride K in both.
  __shared__ double lds[2 * KMAX * KMAX];
  double* g = lds;
  double* a = lds + KMAX * KMAX;
  double* part = a;                                   // [K][FW] during the G pass
  const int s = blockIdx.x, v = s / B, t = s - v * B;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n = min(max(n_rows[t], 0), N);
  const int64_t* ri = ridx + (int64_t)t * ldr;
  const double* dr = d + (int64_t)s * ldd;
  const double fs = fscale[v];
  const double* Ft = F + (int64_t)t * K * K;
  int bad = 0;

  // ---- G = X' diag(1/d) X, upper triangle row by row, then mirrored ----------------------
  for (int j = 0; j < K; ++j) {
    for (int k0 = (j / KC) * KC; k0 < K; k0 += KC) {
      double acc[KC];
#pragma unroll
      for (int c = 0; c < KC; ++c) acc[c] = 0.0;
      for (int i = tid; i < n; i += FT) {
        const double* xr = X + clamp_row(ri[i], R) * ldx;
        const double q = xr[j] / dr[i];
#pragma unroll
        for (int c = 0; c < KC; ++c)
          if (k0 + c < K) acc[c] = fma(q, xr[k0 + c], acc[c]);
      }
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const double r = butterfly(acc[c]);
        if (lane == 0 && k0 + c < K) part[(k0 + c) * FW + wid] = r;
      }
    }
    __syncthreads();
    if (tid >= j && tid < K) {
      double r = part[tid * FW];
#pragma unroll
      for (int w = 1; w < FW; ++w) r = __dadd_rn(r, part[tid * FW + w]);
      g[j * K + tid] = r;
      if (!isfinite(r)) bad |= ST_NONFINITE;
    }
    __syncthreads();
  }
  for (int idx = tid; idx < K * K; idx += FT) {
    const int j = idx / K, k = idx - j * K;
    if (k < j) g[idx] = g[k * K + j];
  }
  __syncthreads();

  // ---- a = I + F_s G, then g = F_s ---------------------------------------------------------
  for (int idx = tid; idx < K * K; idx += FT) {
    const int j = idx / K, k = idx - j * K;
    double acc = 0.0;
    for (int l = 0; l < K; ++l) acc = fma(__dmul_rn(fs, Ft[j * K + l]), g[l * K + k], acc);
    a[idx] = __dadd_rn(acc, j == k ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int idx = tid; idx < K * K; idx += FT) g[idx] = __dmul_rn(fs, Ft[idx]);
  __syncthreads();

  // ---- LU with partial pivoting on [a | g], every wave finds the same pivot ----------------
  for (int col = 0; col < K; ++col) {
    // a NaN candidate counts as the largest, so the order is total and the pick uniform
    double pv = -1.0;
    if (lane >= col && lane < K) {
      pv = fabs(a[lane * K + col]);
      if (isnan(pv)) pv = INFINITY;
    }
    int pi = lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(pv, off, PFML_WAVE);
      const int oi = __shfl_xor(pi, off, PFML_WAVE);
      if (ov > pv || (ov == pv && oi < pi)) { pv = ov; pi = oi; }
    }
    pi = __shfl(pi, 0, PFML_WAVE);
    if (pi < col || pi >= K) pi = col;
    const double piv = a[pi * K + col];
    if (piv == 0.0) bad |= ST_ZERO_PIVOT;
    __syncthreads();
    if (pi != col && tid < 2 * K) {
      double* m = tid < K ? a : g;
      const int c = tid < K ? tid : tid - K;
      const double x = m[col * K + c];
      m[col * K + c] = m[pi * K + c];
      m[pi * K + c] = x;
    }
    __syncthreads();
    const int below = K - col - 1;
    for (int idx = tid; idx < below * 2 * K; idx += FT) {
      const int r = col + 1 + idx / (2 * K), c2 = idx % (2 * K);
      const double l = a[r * K + col] / piv;
      if (c2 < K) {
        if (c2 > col) a[r * K + c2] = fma(-l, a[col * K + c2], a[r * K + c2]);
      } else {
        const int c = c2 - K;
        g[r * K + c] = fma(-l, g[col * K + c], g[r * K + c]);
      }
    }
    __syncthreads();
  }
  // ---- back substitution, all K right-hand sides side by side ------------------------------
  for (int col = K - 1; col >= 0; --col) {
    if (tid < K) g[col * K + tid] = g[col * K + tid] / a[col * K + col];
    __syncthreads();
    for (int idx = tid; idx < col * K; idx += FT) {
      const int r = idx / K, c = idx - r * K;
      g[idx] = fma(-a[r * K + col], g[col * K + c], g[idx]);
    }
    __syncthreads();
  }
  double* Ms = M + (int64_t)s * K * K;
  for (int idx = tid; idx < K * K; idx += FT) {
    const double r = g[idx];
    if (!isfinite(r)) bad |= ST_NONFINITE;
    Ms[idx] = r;
  }
  const int zero = __syncthreads_or(bad & ST_ZERO_PIVOT);
  const int nonf = __syncthreads_or(bad & ST_NONFINITE);
  if (tid == 0) status[s] = (zero ? ST_ZERO_PIVOT : 0) | (nonf ? ST_NONFINITE : 0);
}

__global__ __launch_bounds__(FT) void factor_chain_kernel(
    const double* __restrict__ X, int64_t ldx, int64_t R, const int64_t* __restrict__ ridx,
    int64_t ldr, const double* __restrict__ M, const double* __restrict__ d, int64_t ldd,
    const int* __restrict__ n_rows, const double* __restrict__ rhs, const double* __restrict__ cc,
    const double* __restrict__ grow, const int64_t* __restrict__ nmap,
    const double* __restrict__ hit, const double* __restrict__ ws0, int64_t sws0,
    const int* __restrict__ varm, const int* __restrict__ norm, int B, int N, int K,
    double* Wst, double* __restrict__ Wopt, double* ws_end) {
  __shared__ double wbuf[NMAX];                       // u, then w, of the month
  __shared__ double part[KMAX * FW];
  __shared__ double tau[KMAX];
  __shared__ double sv[KMAX];
  __shared__ double red[FW];
  const int arm = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int v = varm[arm];
  const bool normalize = norm[arm] != 0;
  double* wst_a = Wst + (int64_t)arm * B * N;
  double* wopt_a = Wopt + (int64_t)arm * B * N;
  const double* rhs_a = rhs + (int64_t)arm * B * N;
  const double* cc_a = cc + (int64_t)arm * B * N;
  // column i of every month belongs to thread i % 256: it writes w_start of month t + 1 and is
  // the only one to read it back
  for (int i = tid; i < N; i += FT) wst_a[i] = ws0[(int64_t)arm * sws0 + i];

  for (int t = 0; t < B; ++t) {
    const int n = min(max(n_rows[t], 0), N);
    const int64_t s = (int64_t)v * B + t;
    const int64_t* ri = ridx + (int64_t)t * ldr;
    const double* dr = d + s * ldd;
    const double* Ms = M + s * K * K;
    const double* wsr = wst_a + (int64_t)t * N;
    const double* rr = rhs_a + (int64_t)t * N;
    const double* cr = cc_a + (int64_t)t * N;

    // u = (rhs + c w_start) / d; a zero c keeps w_start out altogether
    for (int i = tid; i < N; i += FT) {
      double u = 0.0;
      if (i < n) {
        // product and sum rounded one by one, as the torch expression rounds them
#pragma clang fp contract(off)
        const double c = cr[i];
        const double cw = c * wsr[i];
        const double b = c != 0.0 ? rr[i] + cw : rr[i];
        u = b / dr[i];
      }
      wbuf[i] = u;
    }
    // tau = X' u
    for (int k0 = 0; k0 < K; k0 += KC) {
      double acc[KC];
#pragma unroll
      for (int c = 0; c < KC; ++c) acc[c] = 0.0;
      for (int i = tid; i < n; i += FT) {
        const double* xr = X + clamp_row(ri[i], R) * ldx;
        const double u = wbuf[i];
#pragma unroll
        for (int c = 0; c < KC; ++c)
          if (k0 + c < K) acc[c] = fma(xr[k0 + c], u, acc[c]);
      }
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const double r = butterfly(acc[c]);
        if (lane == 0 && k0 + c < K) part[(k0 + c) * FW + wid] = r;
      }
    }
    __syncthreads();
    if (tid < K) {
      double r = part[tid * FW];
#pragma unroll
      for (int w = 1; w < FW; ++w) r = __dadd_rn(r, part[tid * FW + w]);
      tau[tid] = r;
    }
    __syncthreads();
    // s = M tau
    if (tid < K) {
      double acc = 0.0;
      for (int l = 0; l < K; ++l) acc = fma(Ms[tid * K + l], tau[l], acc);
      sv[tid] = acc;
    }
    __syncthreads();
    // w = u - (X s) / d
    double wsum = 0.0;
    for (int i = tid; i < n; i += FT) {
      const double* xr = X + clamp_row(ri[i], R) * ldx;
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc = fma(xr[k], sv[k], acc);
      const double w = __dsub_rn(wbuf[i], acc / dr[i]);
      wbuf[i] = w;
      wsum = __dadd_rn(wsum, w);
    }
    if (normalize) {
      wsum = butterfly(wsum);
      if (lane == 0) red[wid] = wsum;
      __syncthreads();
      double tot = red[0];
#pragma unroll
      for (int w = 1; w < FW; ++w) tot = __dadd_rn(tot, red[w]);
      for (int i = tid; i < n; i += FT) wbuf[i] = wbuf[i] / tot;
    }
    double* wo = wopt_a + (int64_t)t * N;
    for (int i = tid; i < N; i += FT) wo[i] = wbuf[i];            // padding columns: 0
    __syncthreads();
    // drift: next w_start = (w grow)[nmap] hit, the torch expression of portfolio._chain
    double* dst = t + 1 < B ? wst_a + (int64_t)(t + 1) * N : ws_end + (int64_t)arm * N;
    const int64_t* nm = nmap + (int64_t)t * N;
    for (int i = tid; i < N; i += FT) {
      int64_t j = nm[i];
      j = j < 0 ? 0 : (j >= N ? N - 1 : j);
      dst[i] = __dmul_rn(__dmul_rn(wbuf[j], grow[(int64_t)t * N + j]), hit[(int64_t)t * N + i]);
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int pfml_factor_solve_max_n() { return NMAX; }
extern "C" int pfml_factor_solve_max_k() { return KMAX; }

// X: loading table, R rows of K doubles at row stride ldx; ridx [B, N] (row stride ldr) int64
// rows of X, month t reads its first n_rows[t] entries; F [B, K, K]; fscale [V]; d [V, B, N] at
// row stride ldd (system s = v B + t); M [V, B, K, K]; status [V, B] (1: zero pivot, 2:
// non-finite entry).
extern "C" hipError_t pfml_factor_prepare(const double* X, int64_t ldx, int64_t R,
                                          const int64_t* ridx, int64_t ldr, const double* F,
                                          const double* fscale, const double* d, int64_t ldd,
                                          const int* n_rows, int V, int B, int N, int K,
                                          double* M, int* status, hipStream_t st) {
  if (V <= 0 || B <= 0) return hipSuccess;
  if (K < 1 || K > KMAX || N < 1 || R < 1 || ldx < K || ldr < N || ldd < N)
    return hipErrorInvalidValue;
  if ((int64_t)V * B > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(factor_prepare_kernel, dim3(V * B), dim3(FT), 0, st, X, ldx, R, ridx, ldr,
                     F, fscale, d, ldd, n_rows, B, N, K, M, status);
  return hipGetLastError();
}

// rhs, c, Wst, Wopt: [A, B, N] contiguous; grow, hit [B, N] fp64 and nmap [B, N] int64
// contiguous; ws0 [A, N] (sws0 = N) or [N] for all arms (sws0 = 0); varm [A] the arm's variant
// (its rows of d and M), norm [A] its normalize flag; ws_end [A, N]: w_start after month B.
extern "C" hipError_t pfml_factor_chain(const double* X, int64_t ldx, int64_t R,
                                        const int64_t* ridx, int64_t ldr, const double* M,
                                        const double* d, int64_t ldd, const int* n_rows,
                                        const double* rhs, const double* c, const double* grow,
                                        const int64_t* nmap, const double* hit,
                                        const double* ws0, int64_t sws0, const int* varm,
                                        const int* norm, int A, int B, int N, int K, double* Wst,
                                        double* Wopt, double* ws_end, hipStream_t st) {
  if (A <= 0 || B <= 0) return hipSuccess;
  if (K < 1 || K > KMAX || N < 1 || N > NMAX || R < 1 || ldx < K || ldr < N || ldd < N)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(factor_chain_kernel, dim3(A), dim3(FT), 0, st, X, ldx, R, ridx, ldr, M, d,
                     ldd, n_rows, rhs, c, grow, nmap, hit, ws0, sws0, varm, norm, B, N, K, Wst,
                     Wopt, ws_end);
  return hipGetLastError();
}
