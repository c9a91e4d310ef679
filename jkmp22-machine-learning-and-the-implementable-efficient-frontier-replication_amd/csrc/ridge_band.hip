// Ridge hyper-parameter grid, eq. (26), band path:  beta_l = (Dbar + l I)^-1 rbar  for all l.
//
// Reference: PFML_Search_Coef.py:124-137 (np.linalg.solve per lambda).  The tridiagonal path
// (ridge.hip) factors Dbar = Q T Q^T with one Householder reflector at a time; every reflector
// needs a full mat-vec over the trailing matrix, i.e. ~n^3/3 doubles streamed per cell through
// ONE CU, and that stream (not the flops) bounds it.  This path reduces Dbar to BAND form
// instead (bandwidth BB = 16, the two-sided blocked Householder of the first stage of a
// two-stage symmetric eigensolver):
//
//     Dbar = Q B Q^T,   Q = Q_0 Q_1 ... Q_{np-1},   Q_p = I - V_p T_p V_p^T  (compact WY)
//
// per panel p (16 columns) the trailing matrix is read once for X = A22 V T and read+written
// once for the rank-32 update A22 -= V W^T + W V^T, both on v_mfma_f64_16x16x4 with V, W
// resident in LDS: 16x fewer passes over the trailing matrix than one pass per reflector.
// Then every lambda is an independent banded Cholesky solve (B + l I) y = Q^T rbar (one wave
// per lambda, register window with DPP broadcasts, O(n BB^2)), and beta = Q y is a blocked-WY back-transform
// (MFMA, Y chunk of 16 lambdas resident in registers).
//
//   kernel 1  band_coop_kernel               K workgroups per cell (1..16, chosen per launch by
//             (ridge_band_reduce.hip)        ops/ridge.py::coop_k), bitwise independent of K
//   kernel 2  ridge_band_solve_kernel        4 lambdas per wave (16-lane DPP rows)
//             (ridge_band_solve.hip)
//   kernel 3  ridge_band_backtransform_kernel one 512-thread workgroup per (cell, 16 lambdas),
//             (ridge_band_bt.hip)            two per CU
//
// A non-positive Cholesky pivot (Dbar + l I not numerically SPD, e.g. l = 0 on a singular
// Dbar) marks that lambda's y NaN; kernel 2b re-solves exactly those systems in the band
// domain by LU with partial pivoting (np.linalg.solve semantics) before the back-transform.
//
// This file sequences the three stages; ridge_band.h holds what they share (constants, the
// workspace and timing-buffer layouts, DPP helpers).
#include "ridge_band.h"

extern "C" int64_t pfml_ridge_band_work_doubles(int n, int L) { return band_work_doubles(n, L); }
extern "C" int pfml_ridge_band_nmax() { return BNMAX; }
extern "C" int pfml_coop_sync_words() { return COOP_SYNC; }
// long long words of a launch's timing buffer (RidgeLaunchArgs::timing)
extern "C" int64_t pfml_ridge_timing_words(int ncells) { return timing_words(ncells); }

hipError_t ridge_band_launch(const RidgeLaunchArgs& a, hipStream_t st) {
  const hipError_t e = band_reduce_launch(a, st);
  if (e != hipSuccess) return e;
  band_solve_launch(a, st);
  band_bt_launch(a, st);
  return hipGetLastError();
}

