// Band path of the ridge grid, kernel 3: the blocked-WY back-transform beta = Q y and its
// launcher, one launch per size class of cells (overview: ridge_band.hip).
#include "ridge_band.h"

namespace {

constexpr int NTB = 512;            // back-transform kernel: 8 waves
constexpr int NWB = NTB / 64;
constexpr int LC = 16;              // lambdas per back-transform workgroup

// ---------------------------------------------------------------------------------------
// kernel 3: beta = Q y, blocked WY, one workgroup per (cell, chunk of LC = 16 lambdas).
//
// The chunk's Y (n x 16) lives in REGISTERS: wave w owns the 16-row blocks b = w + 8 q, one
// double4 per block in the MFMA C layout (row 16 b + g4 + 4 r, lambda c16) - which is also
// the B-operand layout of P = V^T Y, so Y never round-trips through LDS.  Per panel
// (backwards) each wave holds V_p of its blocks in A-operand order of the first product, in
// ONE register copy: the unit-lower-triangular mask is applied in place at the block's first
// use; the 8 partial P meet in LDS (ping-pong buffers: one barrier per panel) and every wave
// forms M = T P itself.  The second product, Y_b -= V_b M, takes the blocks one after the
// other: block q is written to the wave's private ONE-block LDS buffer, read back transposed
// and consumed, and its registers take the loads of panel p - 1 at once (in flight until that
// panel's first product reaches the block; T_p is loaded at the top of its panel and lands
// under the first product).
//
// Residency is what this form is built for (the kernel is bound by neither the MFMA pipe nor
// memory, but by the latency of its barrier, LDS round trips and L2 loads per panel): the
// register budget is held to BT_WPS = 4 waves per SIMD and the LDS is the partial-P ping-pong
// plus 2 176 B per wave, so the 8 x 5 instance (n <= 528: 122 VGPRs, 0 B scratch, 50 176 B
// LDS) runs TWO workgroups per CU.  A full per-wave V image (87 KB) and a second register
// copy of V (the prefetch issued before the first product) held it to one: 373 -> 297 us for
// the 742 workgroups of the production step's big cells.  Three per CU needs <= 80 VGPRs;
// Y and V alone are 80 of them with the 8 x 5 split (the compiler spills 164 B there).
// Block-to-wave map, partial sums, their order and the MFMA sequences are those of the
// earlier form: the betas are bit for bit the same.
// ---------------------------------------------------------------------------------------
// Row-block capacity per wave of the production shape (n <= BNMAX, 8 waves).  Cells of small n
// take narrower instances (NWT waves x NBT blocks, band_bt_launch): fewer waves idle
// (n = 65 has 5 row blocks) and their LDS shrinks with the instance; 4 x 5 (120 VGPRs,
// 25 088 B) runs four workgroups per CU, 4 x 3 (88, 25 088 B) five, 2 x 3 (88, 12 544 B) ten.
constexpr int NBW = (BNMAX / 16 + NWB - 1) / NWB;   // row blocks per wave

constexpr int BT_WPS = 4;           // waves per SIMD the register budget is held to (<= 128 VGPRs)

template <int NWT, int NBT>
__global__ __launch_bounds__(NWT * 64, BT_WPS) void ridge_band_backtransform_kernel(
    const RidgeCellDesc* __restrict__ cells, int cell0, int ncells, int L, double* __restrict__ work,
    double* __restrict__ beta_out, int64_t ldo, const unsigned* __restrict__ syncw) {
  __shared__ double red[2][NWT][BB * BB];
  __shared__ double Vw[NWT][BB][LS];              // wave-private one-block transpose buffers
  // (the chunks of a cell are adjacent in dispatch order, so they run together and share
  // the cell's V panels through the caches; an XCD-grouped order measured slower)
  const int nch = (L + LC - 1) / LC;
  if ((int)blockIdx.x >= ncells * nch) return;
  const int cell = cell0 + (int)blockIdx.x / nch, ch = blockIdx.x % nch;
  const RidgeCellDesc cd = cells[cell];
  const int n = cd.n;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;
  BandWork bw(work + cd.work, n, L);
  const double* __restrict__ A = bw.A;
  const int l0 = ch * LC;
  const bool lok = c16 < min(LC, L - l0);
  const int nb = (n + 15) >> 4;
  const double* __restrict__ yc = bw.Yt + (int64_t)(l0 + (lok ? c16 : 0)) * n;
  {   // padding columns [n, ldo) of this chunk's lambda rows are zero (no fill by the caller)
    const int lc = min(LC, L - l0), pad = (int)(ldo - n);
    double* __restrict__ o = beta_out + cd.out + (int64_t)l0 * ldo + n;
    for (int e = threadIdx.x; e < lc * pad; e += NWT * 64) o[(int64_t)(e / pad) * ldo + e % pad] = 0.0;
  }
  // a cell whose cooperative reduction timed out (its error word, CoopSync) gets NaN betas:
  // the grid search's non-finite-cell recovery then recomputes it (never silent garbage)
  const bool failed = syncw != nullptr && syncw[(int64_t)cell * COOP_SYNC + 1] != 0u;
  double4_t Y[NBT];
#pragma unroll
  for (int q = 0; q < NBT; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * (wid + NWT * q) + g4 + 4 * r;
      Y[q][r] = (lok && i < n) ? (failed ? __builtin_nan("") : yc[i]) : 0.0;
    }
  // vv[q][r] = V_p[16 b - r0 + 4 r + g4][c16] for the blocks b = wid + NWT q of panel p: the
  // only register copy of V (Y and vv are 80 of the instance's VGPRs)
  const int lda = band_npad(n);                   // A's leading dimension (padded)
  double vv[NBT][4];
  // Branch-free loads (the row clamped into the panel: dead blocks and rows past m read a
  // valid, cached element); the unit-lower-triangular mask is applied in place where the
  // block is first used, so a block's loads are waited for only there.
  auto fetch = [&](int p, int q) {
    const int k0 = p * BB, r0 = k0 + BB, m = n - r0;
    const double* Ap = A + (int64_t)r0 * lda + k0; // &V_p[0][0] (wave-uniform)
    const int b = wid + NWT * q;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * b - r0 + 4 * r + g4;
      const int ic = min(max(i, 0), m - 1);
      // (wave-uniform base + 32-bit lane byte offset: one address register per load)
      vv[q][r] = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(Ap) +
                                                  (unsigned)((ic * lda + c16) * 8));
    }
  };
  const int np = (n - 1) / BB;    // panels: k0 = 16 p with k0 + 16 < n
  if (np > 0) {
#pragma unroll
    for (int q = 0; q < NBT; ++q) fetch(np - 1, q);
  }
  for (int p = np - 1; p >= 0; --p) {
    double (*rp)[BB * BB] = red[p & 1];
    double tv[4];                                   // T_p: in flight under the first product
    {
      const double* Tp = bw.T + (int64_t)p * BB * BB;
#pragma unroll
      for (int r = 0; r < 4; ++r) tv[r] = Tp[c16 * BB + 4 * r + g4];
    }
    const int m = n - (p * BB + BB);
    // P_w = sum over live blocks of V_b^T Y_b
    double4_t Pp[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};   // two MFMA chains
#pragma unroll
    for (int q = 0; q < NBT; ++q) {
      const int b = wid + NWT * q;
      if (b > p && b < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * (b - p - 1) + 4 * r + g4;
          vv[q][r] = (i < m && i >= c16) ? (i == c16 ? 1.0 : vv[q][r]) : 0.0;
          Pp[r & 1] = mfma_f64_16x16x4(vv[q][r], Y[q][r], Pp[r & 1]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) rp[wid][(g4 + 4 * r) * BB + c16] = Pp[0][r] + Pp[1][r];
    __syncthreads();
    // M = T P (every wave)
    double4_t Mm = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double pv = 0.0;
#pragma unroll
      for (int w = 0; w < NWT; ++w) pv += rp[w][(4 * r + g4) * BB + c16];
      Mm = mfma_f64_16x16x4(tv[r], pv, Mm);
      __builtin_amdgcn_sched_barrier(0);            // one row group's partials in flight
    }
    // Y_b -= V_b M, block by block: V_b goes through the wave's one-block LDS buffer to the
    // A-operand order V_b[c16][4 r + g4] (the LDS queue of a wave is in order: the fences
    // only pin the compiler), and its registers take the next panel's loads at once
#pragma unroll
    for (int q = 0; q < NBT; ++q) {
      const int b = wid + NWT * q;
      if (b > p && b < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Vw[wid][4 * r + g4][c16] = vv[q][r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double vt[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) vt[r] = Vw[wid][c16][4 * r + g4];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = mfma_f64_16x16x4(vt[r], Mm[r], acc);
        Y[q] -= acc;
      }
      if (p > 0) fetch(p - 1, q);                   // in flight until the next first product
    }
  }
  if (lok) {
    double* __restrict__ out = beta_out + cd.out + (int64_t)(l0 + c16) * ldo;
    // (the row base is made opaque here: otherwise the 4 NBT row indices of the Y loads
    // above stay in registers across the whole panel loop for these stores)
    int i0 = 16 * wid + g4;
    asm volatile("" : "+v"(i0));
#pragma unroll
    for (int q = 0; q < NBT; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 16 * NWT * q + 4 * r;
        if (i < n) out[i] = Y[q][r];
      }
  }
}

// kernel 3 instances by cell size: (waves, row blocks per wave) with 16 NWT NBT >= n
template <int NWT, int NBT>
void bt_one(const RidgeLaunchArgs& a, int c0, int nc, hipStream_t st) {
  const int nch = (a.L + LC - 1) / LC;
  hipLaunchKernelGGL((ridge_band_backtransform_kernel<NWT, NBT>), dim3(nc * nch), dim3(NWT * 64),
                     0, st, a.cells, c0, nc, a.L, a.work, a.beta, a.ldo, a.syncw);
}

int bt_class(int n) { return n <= 96 ? 0 : (n <= 192 ? 1 : (n <= 320 ? 2 : 3)); }

}  // namespace

// kernel 3 over a launch's cells: one launch per run of consecutive cells of one instance
// class (the plan orders cells by size, ops/ridge.py ridge_plan, so a grid has one run per
// size class; n_host: the cells' n in plan order).  bt_classes off: the 8-wave form for all.
void band_bt_launch(const RidgeLaunchArgs& a, hipStream_t st) {
  if (!a.bt_classes) {
    bt_one<NWB, NBW>(a, 0, a.ncells, st);
    return;
  }
  int c0 = 0;
  while (c0 < a.ncells) {
    const int k = bt_class(a.n_host[c0]);
    int c1 = c0 + 1;
    while (c1 < a.ncells && bt_class(a.n_host[c1]) == k) ++c1;
    switch (k) {
      case 0: bt_one<2, 3>(a, c0, c1 - c0, st); break;
      case 1: bt_one<4, 3>(a, c0, c1 - c0, st); break;
      case 2: bt_one<4, 5>(a, c0, c1 - c0, st); break;
      default: bt_one<NWB, NBW>(a, c0, c1 - c0, st); break;
    }
    c0 = c1;
  }
}
