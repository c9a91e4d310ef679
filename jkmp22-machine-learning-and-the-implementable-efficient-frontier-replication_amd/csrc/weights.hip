// The sequential part of the PFML weight recursion (PFML_best_hps.py:168-218, eq. (17)):
//
//   for t:  d      = (w_start - w_aim_t) / a_t
//           w_opt  = w_aim_t + a_t o (m_tilde_t d)           (m_t = diag(a) m_tilde diag(1/a))
//           w_start(t+1)[r] = hit[r] ? w_opt[map[r]] * grow_t[map[r]] : 0
//
// Every month depends on the previous one; each month is one launch of ROWS_WG-row
// workgroups (all launched from the host loop below, no host round trip): every workgroup
// rebuilds the N-vector d of its month in LDS from the previous month's w_opt (drift gather),
// then computes its rows of m_tilde_t d with one wave per row (coalesced row reads, 8 loads per
// lane in flight, shuffle reduction).  m_tilde_t (N x N, the only large operand) is read once
// per month spread over N / ROWS_WG workgroups, so a month costs about one memory round trip:
// a single persistent workgroup was bound by one CU's bandwidth (39 ms for 360 months at
// N = 500), 16-row workgroups walking their rows one load pair at a time by latency (14 ms).
#include "common.h"

namespace {

constexpr int WT = 256;
constexpr int ROWS_WG = 4;             // 4 waves x 1 row
constexpr int WMAX = 4096;             // N held in LDS (32 KB); the multi-portfolio chain
                                       // below holds A * N <= 8192 doubles (64 KB, dynamic)

__global__ __launch_bounds__(WT) void weights_month_kernel(
    const double* __restrict__ mt, int64_t ldm, int64_t sm, const double* __restrict__ a,
    const double* __restrict__ wa, const double* __restrict__ grow,
    const int64_t* __restrict__ nmap, const double* __restrict__ hit, int64_t sv,
    const double* __restrict__ ws0, int m, int B, int N, double* __restrict__ Wst,
    double* __restrict__ Wopt, double* __restrict__ ws_out) {
  __shared__ double d[WMAX];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  // w_start of month m: ws0 (m == 0) or the drifted w_opt of month m - 1
  const double* wop = Wopt + (int64_t)(m - 1) * sv;
  const double* gp = grow + (int64_t)(m - 1) * sv;
  const int64_t* np_ = nmap + (int64_t)(m - 1) * sv;
  const double* hp = hit + (int64_t)(m - 1) * sv;
  const bool last = m == B;                       // final call: only w_start of month B
  const double* am = a + (int64_t)m * sv;
  const double* wam = wa + (int64_t)m * sv;
  for (int j = t; j < N; j += WT) {
    double ws;
    if (m == 0) {
      ws = ws0[j];
    } else {
      const int64_t q = np_[j];
      ws = (wop[q] * gp[q]) * hp[j];
    }
    if (last) {
      if (blockIdx.x == 0) ws_out[j] = ws;
    } else {
      if (blockIdx.x == 0) Wst[(int64_t)m * sv + j] = ws;
      d[j] = (ws - wam[j]) / am[j];
    }
  }
  if (last) return;
  __syncthreads();
  const double* M = mt + (int64_t)m * sm;
  const int i = blockIdx.x * ROWS_WG + w;
  if (i >= N) return;
  const double* row = M + (int64_t)i * ldm;
  double s = 0.0;
  for (int j0 = 0; j0 < N; j0 += 8 * 64) {
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 + 64 * u + lane;
      x[u] = (j < N) ? row[j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 + 64 * u + lane;
      s += (j < N) ? x[u] * d[j] : 0.0;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) Wopt[(int64_t)m * sv + i] = wam[i] + am[i] * s;
}

}  // namespace

extern "C" int pfml_weights_chain_max_n() { return WMAX; }

// mt: [B, N, N] (row stride ldm, batch stride sm); a, wa, grow, hit: [B, N] doubles and nmap
// [B, N] int64 (batch stride sv, entries in [0, N)); ws0 [N]; outputs Wst, Wopt [B, N] (stride
// sv) and ws_out [N] (the w_start of the month after the last).  B + 1 launches on `st`.
extern "C" hipError_t pfml_weights_chain(const double* mt, int64_t ldm, int64_t sm,
                                         const double* a, const double* wa, const double* grow,
                                         const int64_t* nmap, const double* hit, int64_t sv,
                                         const double* ws0, int B, int N, double* Wst,
                                         double* Wopt, double* ws_out, hipStream_t st) {
  if (N <= 0) return hipSuccess;
  if (N > WMAX) return hipErrorInvalidValue;
  const int grid = (N + ROWS_WG - 1) / ROWS_WG;
  for (int m = 0; m <= B; ++m)
    hipLaunchKernelGGL(weights_month_kernel, dim3(m == B ? 1 : grid), dim3(WT), 0, st, mt, ldm,
                       sm, a, wa, grow, nmap, hit, sv, ws0, m, B, N, Wst, Wopt, ws_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// The same recursion for A independent portfolios that share m_tilde, a, grow, nmap and hit and
// differ in their aims wa [A, B, N] (and optionally in ws0): the counterfactual portfolios of
// models/importance.py.  One launch per month as above; every wave still owns one row of
// m_tilde_t and loads it ONCE, into registers (8 * NT loads per lane in flight, NT = the
// 512-column trips of the single kernel), then walks the launch's portfolios: per portfolio
// one accumulator, fed in the single kernel's order from that portfolio's d vector in LDS.
// Per portfolio the arithmetic is weights_month_kernel's operation for operation - the same
// element-to-lane map, the same 8-load groups, the separate multiply and add of the dot
// product (contraction is switched off here: the single kernel compiles to v_mul + v_add), the
// same butterfly, the fused final multiply-add - so column k is bitwise the single chain run
// on wa[k], whatever A is and wherever k sits in the launch.  A NaN in one portfolio's aims
// meets only that portfolio's d and accumulator.  What differs from the single kernel is
// scheduling only: the row loads are issued in front of the d phase, a thread builds column j
// of every portfolio's d (drift map, grow, hit and a read once per column; the portfolios'
// gathers DKU = 8 at a time - one element after the other, A N / 256 dependent gathers per
// thread cost 35 us a month at A = 14), and the portfolio loop runs two independent
// accumulators per trip.
//
// LDS: d is [A][N] doubles, lane l of a wave reads d[k][j0 + 64 u + l] - consecutive doubles
// across the 64 lanes, conflict-free ds_read_b64.  Budget MULTI_LDS_DOUBLES = 8192 doubles
// (64 KB) per workgroup: two workgroups fit in a CU's 160 KB, and a launch takes only A * N
// doubles of it (dynamic), so small shapes keep their occupancy.  Portfolios per launch:
// min(MULTI_ARMS_MAX, 8192 / N) - 16 at N = 512, 2 at N = 4096; the host splits a larger A.
namespace {

constexpr int MULTI_LDS_DOUBLES = 8192;    // d image per workgroup: 64 KB, 2 workgroups / CU
constexpr int MULTI_ARMS_MAX = 64;         // bounds the serial portfolio loop of one launch
constexpr int DKU = 8;                     // portfolios whose gathers fly together (d phase)

template <int NT>
__global__ __launch_bounds__(WT) void weights_month_multi_kernel(
    const double* __restrict__ mt, int64_t ldm, int64_t sm, const double* __restrict__ a,
    const double* __restrict__ wa, int64_t swa, const double* __restrict__ grow,
    const int64_t* __restrict__ nmap, const double* __restrict__ hit, int64_t sv,
    const double* __restrict__ ws0, int64_t sws0, int m, int B, int N, int A,
    double* __restrict__ Wst, double* __restrict__ Wopt, int64_t so,
    double* __restrict__ ws_out) {
#pragma clang fp contract(off)
  extern __shared__ double dm[];                  // [A][N]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const double* gp = grow + (int64_t)(m - 1) * sv;
  const int64_t* np_ = nmap + (int64_t)(m - 1) * sv;
  const double* hp = hit + (int64_t)(m - 1) * sv;
  const bool last = m == B;
  const double* am = a + (int64_t)m * sv;
  // this wave's row of m_tilde_t first: its loads fly while d is built
  const int i = blockIdx.x * ROWS_WG + w;
  const bool live = !last && i < N;
  double x[8 * NT];
  if (live) {
    const double* row = mt + (int64_t)m * sm + (int64_t)i * ldm;
#pragma unroll
    for (int g = 0; g < NT; ++g) {
      if (g * 512 < N) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = g * 512 + 64 * u + lane;
          x[8 * g + u] = (j < N) ? row[j] : 0.0;
        }
      }
    }
  }
  // d of every portfolio: a thread owns column j of all of them (the drift map, grow, hit and
  // a are read once per column), the portfolios' loads DKU at a time
  for (int j = t; j < N; j += WT) {
    int64_t q = 0;
    double gq = 0.0, hj = 0.0;
    if (m > 0) {
      q = np_[j];
      gq = gp[q];
      hj = hp[j];
    }
    const double aj = last ? 1.0 : am[j];
    for (int k0 = 0; k0 < A; k0 += DKU) {
      double wv[DKU], av[DKU];
#pragma unroll
      for (int u = 0; u < DKU; ++u) {
        const int k = k0 + u < A ? k0 + u : A - 1;
        wv[u] = m == 0 ? ws0[(int64_t)k * sws0 + j]
                       : Wopt[(int64_t)k * so + (int64_t)(m - 1) * sv + q];
        av[u] = last ? 0.0 : wa[(int64_t)k * swa + (int64_t)m * sv + j];
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
            dm[k * N + j] = (ws - av[u]) / aj;
          }
        }
      }
    }
  }
  if (last) return;
  __syncthreads();
  if (!live) return;
  const double ai = am[i];
  // two portfolios per trip, each with its own accumulator and butterfly (independent chains)
  for (int k = 0; k < A; k += 2) {
    const bool two = k + 1 < A;
    const double* d0 = dm + k * N;
    const double* d1 = dm + (two ? k + 1 : k) * N;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int g = 0; g < NT; ++g) {
      if (g * 512 < N) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = g * 512 + 64 * u + lane;
          s0 += (j < N) ? x[8 * g + u] * d0[j] : 0.0;
          s1 += (j < N) ? x[8 * g + u] * d1[j] : 0.0;
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
      Wopt[(int64_t)k * so + o] = __builtin_fma(s0, ai, wa[(int64_t)k * swa + o]);
      if (two)
        Wopt[(int64_t)(k + 1) * so + o] =
            __builtin_fma(s1, ai, wa[(int64_t)(k + 1) * swa + o]);
    }
  }
}

}  // namespace

// Portfolios one pfml_weights_chain_multi call takes at width N (0: N is beyond the kernel).
extern "C" int pfml_weights_chain_multi_max_arms(int N) {
  if (N > WMAX) return 0;
  if (N <= 0) return MULTI_ARMS_MAX;
  const int c = MULTI_LDS_DOUBLES / N;
  return c < MULTI_ARMS_MAX ? c : MULTI_ARMS_MAX;
}

// pfml_weights_chain for A portfolios: mt, a, grow, nmap, hit as there (shared); wa [A, B, N]
// (portfolio stride swa, month stride sv); ws0 [A, N] (portfolio stride sws0) or one [N] for
// all (sws0 = 0); outputs Wst, Wopt [A, B, N] (portfolio stride so, month stride sv) and
// ws_out [A, N] contiguous.  A <= pfml_weights_chain_multi_max_arms(N); B + 1 launches.
extern "C" hipError_t pfml_weights_chain_multi(
    const double* mt, int64_t ldm, int64_t sm, const double* a, const double* wa, int64_t swa,
    const double* grow, const int64_t* nmap, const double* hit, int64_t sv, const double* ws0,
    int64_t sws0, int B, int N, int A, double* Wst, double* Wopt, int64_t so, double* ws_out,
    hipStream_t st) {
  if (N <= 0 || A <= 0) return hipSuccess;
  if (N > WMAX || A > pfml_weights_chain_multi_max_arms(N)) return hipErrorInvalidValue;
  const int grid = (N + ROWS_WG - 1) / ROWS_WG;
  const size_t lds = sizeof(double) * (size_t)A * (size_t)N;
  const int trips = (N + 511) / 512;
  auto kern = trips <= 1 ? weights_month_multi_kernel<1>
              : trips <= 2 ? weights_month_multi_kernel<2>
              : trips <= 4 ? weights_month_multi_kernel<4>
                           : weights_month_multi_kernel<8>;
  for (int m = 0; m <= B; ++m)
    hipLaunchKernelGGL(kern, dim3(m == B ? 1 : grid), dim3(WT), m == B ? 0 : lds, st, mt, ldm,
                       sm, a, wa, swa, grow, nmap, hit, sv, ws0, sws0, m, B, N, A, Wst, Wopt,
                       so, ws_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Aim portfolios (PFML_aim_fun.py:138-163, K18): w_aim = s_t beta for every OOS month in ONE
// launch instead of a per-month library GEMV from a Python loop.  Job j (one month): S_j =
// rows [0, nrow_j) of a row-major [*, ld_j] signal block at sptr_j (the S4 signal views, no
// copy), beta_j = coef row j (nk_j = p + 1 entries), out[off_j + r].  One wave per output row:
// lane l sums k = l, l + 64, ... in order, then a fixed butterfly - the same order for a row
// wherever its month sits in the launch (aims are bitwise independent of the sharding).
namespace {
struct AimJob {
  const double* s;
  int64_t ld;
  int64_t off;
  int nrow;
  int nk;
};

__global__ __launch_bounds__(256) void aim_gemv_kernel(const AimJob* __restrict__ jobs,
                                                       const double* __restrict__ coef,
                                                       int64_t ldc, double* __restrict__ out) {
  const AimJob jb = jobs[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= jb.nrow) return;
  const double* srow = jb.s + (int64_t)r * jb.ld;
  const double* c = coef + (int64_t)blockIdx.y * ldc;
  double acc = 0.0;
  for (int k = lane; k < jb.nk; k += 64) acc = fma(srow[k], c[k], acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) out[jb.off + r] = acc;
}
}  // namespace

extern "C" int pfml_aim_job_size() { return (int)sizeof(AimJob); }

// jobs: device AimJob[njobs]; coef: [njobs, ldc]; rows per job <= max_rows.
extern "C" hipError_t pfml_aim_gemv(const void* jobs, int njobs, int max_rows, const double* coef,
                                    int64_t ldc, double* out, hipStream_t st) {
  if (njobs <= 0 || max_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(aim_gemv_kernel, dim3((max_rows + 3) / 4, njobs), dim3(256), 0, st,
                     static_cast<const AimJob*>(jobs), coef, ldc, out);
  return hipGetLastError();
}
