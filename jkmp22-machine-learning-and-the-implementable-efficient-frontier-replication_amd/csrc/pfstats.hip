// Per-month portfolio statistics (PFML_best_hps.py:220-259, portfolio.pf_ts) on the padded
// [B, ld] layout of the weight recursion, one launch for every month:
//
//   inv = sum |w|            shorting = sum |min(w, 0)|       turnover = sum |w - w_start|
//   r   = sum w ret          tc = wealth / 2 * sum lam (w - w_start)^2
//
// Month t reads its first n_rows[t] columns only (the rest is padding and is never loaded).
// Every sum has pandas groupby.sum semantics: a NaN term is skipped in that statistic alone, a
// month with no finite term (or no row) gives 0.
//
// One workgroup per month.  Thread t owns the element pairs p = t, t + 256, ... (elements 2p,
// 2p + 1) and adds their terms in that order; then a wave butterfly, then the four waves in
// index order.  A pair is one 16-byte load per operand when the four row bases are 16-byte
// aligned, two 8-byte loads otherwise - the element-to-thread map and the order of every
// addition are the same on both paths (products and sums are individually rounded, never
// contracted), so a month's five numbers are bitwise the same whatever B, the month's position
// in the launch, ld or the alignment of the buffers.  No atomics.
#include "common.h"

namespace {

constexpr int PT = 256;
typedef double double2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void add_term(double& acc, double t) {
  acc = isnan(t) ? acc : __dadd_rn(acc, t);
}

__device__ __forceinline__ void pf_terms(double w, double ws, double r, double l,
                                         double (&acc)[5]) {
  const double dw = __dsub_rn(w, ws);
  add_term(acc[0], fabs(w));
  add_term(acc[1], w < 0.0 ? -w : 0.0);
  add_term(acc[2], fabs(dw));
  add_term(acc[3], __dmul_rn(w, r));
  add_term(acc[4], __dmul_rn(__dmul_rn(l, dw), dw));
}

__global__ __launch_bounds__(PT) void pf_stats_kernel(
    const double* __restrict__ w, const double* __restrict__ ws, const double* __restrict__ ret,
    const double* __restrict__ lam, const int* __restrict__ n_rows,
    const double* __restrict__ wealth, int64_t ld, double* __restrict__ out) {
  __shared__ double part[5][PT / 64];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int64_t n = min((int64_t)max(n_rows[b], 0), ld);
  const double* wr = w + (int64_t)b * ld;
  const double* sr = ws + (int64_t)b * ld;
  const double* rr = ret + (int64_t)b * ld;
  const double* lr = lam + (int64_t)b * ld;
  const bool vec = (((uintptr_t)wr | (uintptr_t)sr | (uintptr_t)rr | (uintptr_t)lr) & 15) == 0;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t npair = (n + 1) >> 1;
  for (int64_t p = t; p < npair; p += PT) {
    const int64_t e = 2 * p;
    if (e + 1 < n) {
      double2_t a, s, r, l;
      if (vec) {
        a = *reinterpret_cast<const double2_t*>(wr + e);
        s = *reinterpret_cast<const double2_t*>(sr + e);
        r = *reinterpret_cast<const double2_t*>(rr + e);
        l = *reinterpret_cast<const double2_t*>(lr + e);
      } else {
        a = double2_t{wr[e], wr[e + 1]};
        s = double2_t{sr[e], sr[e + 1]};
        r = double2_t{rr[e], rr[e + 1]};
        l = double2_t{lr[e], lr[e + 1]};
      }
      pf_terms(a.x, s.x, r.x, l.x, acc);
      pf_terms(a.y, s.y, r.y, l.y, acc);
    } else {
      pf_terms(wr[e], sr[e], rr[e], lr[e], acc);          // the odd last element
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_xor(v, off, PFML_WAVE));
    if (lane == 0) part[k][wid] = v;
  }
  __syncthreads();
  if (t < 5) {
    double v = part[t][0];
#pragma unroll
    for (int i = 1; i < PT / 64; ++i) v = __dadd_rn(v, part[t][i]);
    if (t == 4) v = __dmul_rn(wealth[b] / 2.0, v);
    out[(int64_t)b * 5 + t] = v;
  }
}

}  // namespace

// w, w_start, ret, lam: [B, ld] doubles (row stride ld); n_rows [B] int32 (clamped to
// [0, ld]); wealth [B]; out [B, 5] = (inv, shorting, turnover, r, tc).
extern "C" hipError_t pfml_pf_stats(const double* w, const double* w_start, const double* ret,
                                    const double* lam, const int* n_rows, const double* wealth,
                                    int64_t ld, int B, double* out, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (ld < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pf_stats_kernel, dim3(B), dim3(PT), 0, st, w, w_start, ret, lam, n_rows,
                     wealth, ld, out);
  return hipGetLastError();
}
