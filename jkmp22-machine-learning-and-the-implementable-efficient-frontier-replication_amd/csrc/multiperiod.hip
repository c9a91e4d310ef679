// Multiperiod-ML (models/multiperiod.py): the closed-form multi-period trade
//
//   b_tau   = (a_t o mu_hat_{t,tau+1}) / W_t                     tau = 0 .. K-1
//   v_{K-1} = b_{K-1};  v_tau = b_tau + gbar (m_tilde_t v_{tau+1})  tau = K-2 .. 0   V_t := v_0
//   w_opt,t = a_t o (m_tilde_t (w_start,t / a_t + u V_t))
//   w_start,t+1 = drift of w_opt,t        (grow / nmap / hit, as weights.hip)
//
// with the symbols of ops/linalg.py (a = Lambda^-1/2, m = diag(a) m_tilde diag(1/a)).  V_t does
// not depend on the arm (u enters linearly), so the horizon fold runs once per month with no
// arms (mp_fold_kernel, all months in parallel) and only the chain carries arms
// (mp_month_kernel, one launch per month).  A month's live universe is its first n_rows[t] rows
// and columns: nothing beyond them is read from m_tilde, a, mu_hat or V, and the outputs'
// padding is written 0.
#include "common.h"

namespace {

constexpr int FT = 1024;               // fold: 16 waves per month
constexpr int FW = FT / 64;
constexpr int MPMAX = 4096;            // N: the fold's two N-vectors take 64 KB of LDS there
constexpr int WT = 256;
constexpr int ROWS_WG = 4;             // chain: 4 waves x 1 row, as weights_month_multi_kernel
constexpr int MP_LDS_DOUBLES = 8192;   // chain: d image [A][N] per workgroup, 64 KB
constexpr int MP_ARMS_MAX = 16;
constexpr int DKU = 8;                 // arms whose gathers fly together (d phase)

__device__ __forceinline__ int live_rows(const int* __restrict__ n_rows, int t, int N) {
  const int n = n_rows[t];
  return n < 0 ? 0 : (n > N ? N : n);
}

// One workgroup per month.  m_tilde_t (n x n) is read K - 1 times (with hundreds of months in
// flight the later passes come from memory again, not from the XCD's L2: measured in the README's
// Multiperiod-ML section); v_{tau+1} and v_tau are a ping-pong of two N-vectors in LDS.  Per pass wave
// w takes rows w, w + 16, ...: lane l sums columns l, l + 64, ... in order (8 loads in flight, the
// separate multiply and add of weights_month_kernel), a fixed butterfly, lane 0 writes
// b_tau[row] + gbar * sum.  Every wave meets the same K barriers whatever n is (n = 0 too).  A
// month's bits depend on its own operands only: not on B, not on its place in the launch.
__global__ __launch_bounds__(FT) void mp_fold_kernel(
    const double* __restrict__ mt, int64_t ldm, int64_t sm, const double* __restrict__ a,
    const double* __restrict__ mu, int64_t sk, const double* __restrict__ wealth,
    const int* __restrict__ n_rows, int64_t sv, double gbar, int K, int N,
    double* __restrict__ V) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double vbuf[];          // [2][N]
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = live_rows(n_rows, t, N);
  const double* am = a + (int64_t)t * sv;
  const double* mum = mu + (int64_t)t * sv;
  const double Wt = wealth[t];
  const double* M = mt + (int64_t)t * sm;
  double* cur = vbuf;
  double* nxt = vbuf + N;
  for (int j = tid; j < n; j += FT) cur[j] = (am[j] * mum[(int64_t)(K - 1) * sk + j]) / Wt;
  __syncthreads();
  for (int tau = K - 2; tau >= 0; --tau) {
    const double* mut = mum + (int64_t)tau * sk;
    for (int i = w; i < n; i += FW) {
      const double* row = M + (int64_t)i * ldm;
      const double bi = (am[i] * mut[i]) / Wt;
      double s = 0.0;
      for (int j0 = 0; j0 < n; j0 += 8 * 64) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = j0 + 64 * u + lane;
          x[u] = (j < n) ? row[j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = j0 + 64 * u + lane;
          s += (j < n) ? x[u] * cur[j] : 0.0;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == 0) nxt[i] = bi + gbar * s;
    }
    __syncthreads();
    double* sw = cur;
    cur = nxt;
    nxt = sw;
  }
  double* out = V + (int64_t)t * sv;
  for (int j = tid; j < N; j += FT) out[j] = (j < n) ? cur[j] : 0.0;
}

// One launch per month m (m == B: only the w_start after the last month), the design of
// weights_month_multi_kernel: every workgroup rebuilds d_k = w_start,k / a + u_k V_m of the
// launch's A arms in LDS through the drift gather, a wave loads its row of m_tilde_m once into
// registers and walks the arms with one accumulator each, w_opt = a o (row sum).  Arm k's
// arithmetic is the same operations in the same order whatever A is and wherever k sits; a NaN
// in one arm meets only that arm's d and accumulator.  The drift covers all N columns (padding
// columns carry hit = 0), d and the row sums only the month's n live ones; padding rows of
// w_opt are written 0.
template <int NT>
__global__ __launch_bounds__(WT) void mp_month_kernel(
    const double* __restrict__ mt, int64_t ldm, int64_t sm, const double* __restrict__ a,
    const double* __restrict__ V, const double* __restrict__ uarm,
    const int* __restrict__ n_rows, const double* __restrict__ grow,
    const int64_t* __restrict__ nmap, const double* __restrict__ hit, int64_t sv,
    const double* __restrict__ ws0, int64_t sws0, int m, int B, int N, int A,
    double* __restrict__ Wst, double* __restrict__ Wopt, int64_t so,
    double* __restrict__ ws_out) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double dm[];            // [A][N]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const double* gp = grow + (int64_t)(m - 1) * sv;
  const int64_t* np_ = nmap + (int64_t)(m - 1) * sv;
  const double* hp = hit + (int64_t)(m - 1) * sv;
  const bool last = m == B;
  const int n = last ? 0 : live_rows(n_rows, m, N);
  const double* am = a + (int64_t)m * sv;
  const double* vm = V + (int64_t)m * sv;
  // this wave's row of m_tilde_m first: its loads fly while d is built
  const int i = blockIdx.x * ROWS_WG + w;
  const bool live = i < n;
  double x[8 * NT];
  if (live) {
    const double* row = mt + (int64_t)m * sm + (int64_t)i * ldm;
#pragma unroll
    for (int g = 0; g < NT; ++g) {
      if (g * 512 < n) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = g * 512 + 64 * u + lane;
          x[8 * g + u] = (j < n) ? row[j] : 0.0;
        }
      }
    }
  }
  for (int j = t; j < N; j += WT) {
    int64_t q = 0;
    double gq = 0.0, hj = 0.0;
    if (m > 0) {
      q = np_[j];
      q = q < 0 ? 0 : (q >= N ? N - 1 : q);      // a map entry off the month is never followed
      gq = gp[q];
      hj = hp[j];
    }
    const bool col = j < n;
    const double aj = col ? am[j] : 1.0;
    const double vj = col ? vm[j] : 0.0;
    for (int k0 = 0; k0 < A; k0 += DKU) {
      double wv[DKU];
#pragma unroll
      for (int u = 0; u < DKU; ++u) {
        const int k = k0 + u < A ? k0 + u : A - 1;
        wv[u] = m == 0 ? ws0[(int64_t)k * sws0 + j]
                       : Wopt[(int64_t)k * so + (int64_t)(m - 1) * sv + q];
      }
#pragma unroll
      for (int u = 0; u < DKU; ++u) {
        const int k = k0 + u;
        if (k < A) {
          const double ws = m == 0 ? wv[u] : (wv[u] * gq) * hj;
          if (last) {
            if (blockIdx.x == 0) ws_out[(int64_t)k * N + j] = ws;
          } else {
            if (blockIdx.x == 0) Wst[(int64_t)k * so + (int64_t)m * sv + j] = ws;
            if (col) dm[k * N + j] = ws / aj + uarm[k] * vj;
          }
        }
      }
    }
  }
  if (last) return;
  __syncthreads();
  if (!live) {
    if (i < N && lane == 0)
      for (int k = 0; k < A; ++k) Wopt[(int64_t)k * so + (int64_t)m * sv + i] = 0.0;
    return;
  }
  const double ai = am[i];
  // two arms per trip, each with its own accumulator and butterfly (independent chains)
  for (int k = 0; k < A; k += 2) {
    const bool two = k + 1 < A;
    const double* d0 = dm + k * N;
    const double* d1 = dm + (two ? k + 1 : k) * N;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int g = 0; g < NT; ++g) {
      if (g * 512 < n) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = g * 512 + 64 * u + lane;
          s0 += (j < n) ? x[8 * g + u] * d0[j] : 0.0;
          s1 += (j < n) ? x[8 * g + u] * d1[j] : 0.0;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s0 += __shfl_xor(s0, off, 64);
      s1 += __shfl_xor(s1, off, 64);
    }
    if (lane == 0) {
      const int64_t o = (int64_t)m * sv + i;
      Wopt[(int64_t)k * so + o] = ai * s0;
      if (two) Wopt[(int64_t)(k + 1) * so + o] = ai * s1;
    }
  }
}

}  // namespace

extern "C" int pfml_mp_max_n() { return MPMAX; }

// Arms one pfml_mp_chain call takes at width N (0: N is beyond the kernel).
extern "C" int pfml_mp_max_arms(int N) {
  if (N > MPMAX) return 0;
  if (N <= 0) return MP_ARMS_MAX;
  const int c = MP_LDS_DOUBLES / N;
  return c < MP_ARMS_MAX ? c : MP_ARMS_MAX;
}

// mt: [B, N, N] (row stride ldm, month stride sm); a [B, N], V out [B, N] (month stride sv); mu
// [K, B, N] (horizon stride sk, month stride sv); wealth [B]; n_rows [B] int32.  One launch.
extern "C" hipError_t pfml_mp_fold(const double* mt, int64_t ldm, int64_t sm, const double* a,
                                   const double* mu, int64_t sk, const double* wealth,
                                   const int* n_rows, int64_t sv, double gbar, int K, int B,
                                   int N, double* V, hipStream_t st) {
  if (B <= 0 || N <= 0) return hipSuccess;
  if (N > MPMAX || K < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mp_fold_kernel, dim3(B), dim3(FT), sizeof(double) * 2 * (size_t)N, st, mt,
                     ldm, sm, a, mu, sk, wealth, n_rows, sv, gbar, K, N, V);
  return hipGetLastError();
}

// mt, a, n_rows as above; V [B, N] (the fold's output); uarm [A] device doubles; grow, hit [B, N]
// doubles and nmap [B, N] int64 (entries in [0, N)); ws0 [A, N] (arm stride sws0) or one [N] for
// all (sws0 = 0); outputs Wst, Wopt [A, B, N] (arm stride so, month stride sv) and ws_out [A, N]
// contiguous.  A <= pfml_mp_max_arms(N); B + 1 launches on `st`, no host round trip.
extern "C" hipError_t pfml_mp_chain(const double* mt, int64_t ldm, int64_t sm, const double* a,
                                    const double* V, const double* uarm, const int* n_rows,
                                    const double* grow, const int64_t* nmap, const double* hit,
                                    int64_t sv, const double* ws0, int64_t sws0, int B, int N,
                                    int A, double* Wst, double* Wopt, int64_t so,
                                    double* ws_out, hipStream_t st) {
  if (N <= 0 || A <= 0) return hipSuccess;
  if (N > MPMAX || A > pfml_mp_max_arms(N)) return hipErrorInvalidValue;
  const int grid = (N + ROWS_WG - 1) / ROWS_WG;
  const size_t lds = sizeof(double) * (size_t)A * (size_t)N;
  const int trips = (N + 511) / 512;
  auto kern = trips <= 1 ? mp_month_kernel<1>
              : trips <= 2 ? mp_month_kernel<2>
              : trips <= 4 ? mp_month_kernel<4>
                           : mp_month_kernel<8>;
  for (int m = 0; m <= B; ++m)
    hipLaunchKernelGGL(kern, dim3(m == B ? 1 : grid), dim3(WT), m == B ? 0 : lds, st, mt, ldm,
                       sm, a, V, uarm, n_rows, grow, nmap, hit, sv, ws0, sws0, m, B, N, A, Wst,
                       Wopt, so, ws_out);
  return hipGetLastError();
}
