// Band path of the ridge grid (ridge_band.hip): what its translation units share.  The
// constants, the one statement of the per-cell workspace and timing-buffer layouts, the DPP and
// Newton helpers, and the stage launchers that ridge_band.hip sequences:
//
//   ridge_band_reduce.hip  kernel 1   band_coop_kernel (+ the panel-QR micro-benchmark)
//   ridge_band_solve.hip   kernel 2   ridge_band_solve_kernel, 2b band_lu_flag / ridge_band_lu
//   ridge_band_bt.hip      kernel 3   ridge_band_backtransform_kernel
#pragma once
#include "common.h"
#include "ridge_desc.h"
#include <type_traits>

constexpr int BB = 16;              // bandwidth = panel width = MFMA tile
constexpr int LS = BB + 1;          // LDS row stride (bank spread for column-wise reads)
constexpr int BMP = 512;            // max panel rows m = n - r0  (n <= BNMAX)
constexpr int BNMAX = BMP + BB;     // 528 >= p_max + 1
constexpr int COOP_SYNC = 32;       // u32 words of sync state per cell (128 B); word 1: error

// Per-cell workspace layout (doubles).  A has room for the padded npad x npad matrix
// (npad = n rounded up to 16).  P: double* in the kernels (the regions' addresses); int64_t on
// the host (their offsets from the cell's base, for band_work_doubles).
__host__ __device__ __forceinline__ int band_npad(int n) { return (n + BB - 1) & ~(BB - 1); }

template <class P>
struct BandWorkT {
  P A, LB, z, T, Yt, Lf, F;
  __host__ __device__ BandWorkT(P w, int n, int L) {
    const int np = (n + BB - 1) / BB;
    const int npad = band_npad(n);
    A = w;                                   // working matrix (V_p / R_p stored below)
    LB = A + (int64_t)npad * npad;           // n x LS lower band: LB[r][s] = B[r][r-16+s]
    z = LB + (int64_t)n * LS;                // Q^T rbar
    T = z + n;                               // np x 16 x 16 compact-WY T_p
    Yt = T + (int64_t)np * BB * BB;          // L x n   solutions y_l, then beta_l
    // banded Cholesky factors: L x n x 16 sub-diagonal entries (one 128-byte line per row,
    // the base rounded up to 16 doubles: every row is written whole by one store
    // instruction), then L x n inverse diagonals
    Lf = w + ((((Yt - w) + (int64_t)L * n) + 15) & ~(int64_t)15);
    F = Lf + (int64_t)L * n * LS;            // cooperative hand-off scratch (CoopWork)
  }
};
typedef BandWorkT<double*> BandWork;

// hand-off scratch of one cell (BandWork's F region, the last of the workspace)
template <class P>
struct CoopWorkT {
  P Vg, Wg, Tg, Pg, Pzg, end;
  __host__ __device__ CoopWorkT(P f, int npad) {
    Vg = f;                                  // V_p rows 0..m-1 (published by the QR WG)
    Wg = Vg + (int64_t)npad * BB;            // W_p rows (every WG its X blocks)
    Tg = Wg + (int64_t)npad * BB;            // T_p
    Pg = Tg + BB * BB;                       // per block V_I' X_I  [33][256]
    Pzg = Pg + (BNMAX / BB) * BB * BB;       // per block V_I' z_I  [33][16]
    end = Pzg + (BNMAX / BB) * BB;
  }
};
typedef CoopWorkT<double*> CoopWork;

// Doubles of one cell's band workspace: the end of the layout above, plus what the rounding of
// the Lf base left unused of the 15 doubles allowed for it (the allowance does not depend on
// how n and L happen to round).
inline int64_t band_work_doubles(int n, int L) {
  const BandWorkT<int64_t> bw(0, n, L);
  const CoopWorkT<int64_t> cw(bw.F, band_npad(n));
  return cw.end + 15 - (bw.Lf - (bw.Yt + (int64_t)L * n));
}

// Timing buffer (RidgeLaunchArgs::timing, long long words): per cell TIM_WG phase slots for
// each of the workgroups w = 0 (the QR one) and 1 of its reduction; behind the cells', the
// solve kernel's slots (forward / backward cycles of its block 0).
constexpr int TIM_WG = 8;
__host__ __device__ __forceinline__ int64_t timing_cell_slot(int cell, int w) {
  return (int64_t)cell * (2 * TIM_WG) + w * TIM_WG;
}
__host__ __device__ __forceinline__ int64_t timing_solve_slot(int ncells) {
  return timing_cell_slot(ncells, 0);
}
inline int64_t timing_words(int ncells) { return timing_solve_slot(ncells) + 2 * TIM_WG; }

// The stages of one band launch, each queued on st (ridge_band.hip: ridge_band_launch runs
// them in this order).  The kernels report nothing; the reduce launcher returns the error of
// its memset of the sync words.
hipError_t band_reduce_launch(const RidgeLaunchArgs& a, hipStream_t st);
void band_solve_launch(const RidgeLaunchArgs& a, hipStream_t st);
void band_bt_launch(const RidgeLaunchArgs& a, hipStream_t st);
hipError_t ridge_band_launch(const RidgeLaunchArgs& a, hipStream_t st);
extern "C" int64_t pfml_ridge_band_work_doubles(int n, int L);
extern "C" int pfml_ridge_band_nmax();

// f(integral_constant<I>), ..., f(integral_constant<N - 1>): a loop whose index is a constant
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// DPP helpers (gfx950: row_newbcast broadcasts one lane of each 16-lane row).
// (row_newbcast reads a valid source lane for every lane, so "old" is never used)
template <int SEL>
__device__ __forceinline__ double row_bcast(double v) {   // lane SEL of each 16-lane row
  // one v_mov_b64_dpp (64-bit DPP supports row_newbcast on gfx90a+/gfx950)
  const long s = __builtin_bit_cast(long, v);
  const long r = __builtin_amdgcn_update_dpp(s, s, 0x150 + SEL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, r);
}

// w += bcast_SEL(src) * m  as ONE v_fmac_f64_dpp (row_newbcast on the DPP source).  The
// first use after `src` is written must follow a VALU write by 2 wait states: FIRST adds them.
template <int SEL, bool FIRST>
__device__ __forceinline__ void fmac_bcast(double& w, double src, double m) {
  if constexpr (FIRST)
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(w) : "v"(src), "v"(m), "i"(SEL));
  else
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(w) : "v"(src), "v"(m), "i"(SEL));
}

// w -= bcast_SEL(src) * m  (the DPP source negated by the instruction's neg modifier: no
// separate negation of src)
template <int SEL, bool FIRST>
__device__ __forceinline__ void fnmac_bcast(double& w, double src, double m) {
  if constexpr (FIRST)
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(w) : "v"(src), "v"(m), "i"(SEL));
  else
    asm volatile("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(w) : "v"(src), "v"(m), "i"(SEL));
}

// 1/sqrt(x) with ONE Newton step on v_rsq_f64 (~2^-46 relative: the banded Cholesky's pivots,
// far below the factorisation's own n eps backward error)
__device__ __forceinline__ double rsqrt1_f64(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  return y * fma(-0.5 * x * y, y, 1.5);
}

template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// 1/sqrt(x) to full fp64 accuracy: v_rsq_f64 refined by Newton steps, a short dependent
// chain in place of the IEEE sqrt and divide sequences on the banded Cholesky's pivot path.
// Measured on MI355X over x in 1e-30 .. 1e30 (tools/micro/rsq_acc.hip): the seed is good to
// ~2^-24 relative, two steps give <= 2 ulp of the IEEE 1/sqrt, a third step changes nothing
// (still 2 ulp), so two steps.
__device__ __forceinline__ double rsqrt_f64(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double h = 0.5 * x;
#pragma unroll
  for (int it = 0; it < 2; ++it) y = y * fma(-h * y, y, 1.5);
  return y;
}

// 1/x to full fp64 accuracy: v_rcp_f64 refined by Newton steps (e = 1 - x y, y += y e); two
// steps are correctly rounded on every measured x (rsq_acc.hip), as three were.
__device__ __forceinline__ double rcp_f64(double x) {
  double y = __builtin_amdgcn_rcp(x);
#pragma unroll
  for (int it = 0; it < 2; ++it) y = fma(y, fma(-x, y, 1.0), y);
  return y;
}

// (64-bit DPP supports only row_newbcast, so the butterfly levels are 32-bit DPP moves)
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_mov<0xB1>(v);      // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);      // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);     // row_half_mirror
  v += dpp_mov<0x140>(v);     // row_mirror
  return v;
}

// Sum of v over lanes {l, l^16, l^32, l^48} (the 4 row groups of a wave), with the gfx950
// VALU lane swaps instead of two ds_bpermute round trips.
__device__ __forceinline__ double rowgroup_sum(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  v = __hiloint2double((int)h16[0], (int)l16[0]) + __hiloint2double((int)h16[1], (int)l16[1]);
  const int lo2 = __double2loint(v), hi2 = __double2hiint(v);
  const auto l32 = __builtin_amdgcn_permlane32_swap(lo2, lo2, false, false);
  const auto h32 = __builtin_amdgcn_permlane32_swap(hi2, hi2, false, false);
  return __hiloint2double((int)h32[0], (int)l32[0]) + __hiloint2double((int)h32[1], (int)l32[1]);
}
