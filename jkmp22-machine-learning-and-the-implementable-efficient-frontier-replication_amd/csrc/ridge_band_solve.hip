// Band path of the ridge grid, kernels 2 and 2b: the banded Cholesky solve of every lambda, the
// pivoted banded LU repair of the lambdas it marks, and their launcher (overview:
// ridge_band.hip).
#include "ridge_band.h"

namespace {

// w[U + s] = LDS row at byte address `base` (s = 0 .. LS-1) in the lanes U, U+16, U+32, U+48
// (the pivot lane of each 16-lane row): 17 ds_read_b64 straight into the window registers
// under an exec mask set and restored INSIDE the one asm statement (no branch, and "+v": the
// other lanes keep their values, so no merge copies), and NO wait: the caller overlaps the
// loads with independent work and then calls lds_row_wait<U>, which waits for them and ties
// the same registers, so no read of w[U..U+16] can be scheduled between the two.  (Written in
// plain C++ the compiler issued the loads into temporaries, waited for them at once and merged
// them with 14 masked moves: the LDS latency sat on every step.)
// `pv` (the pivot, unchanged) is tied through the asm so that the rsq chain that consumes it
// is scheduled after the loads are issued.
template <int U>
__device__ __forceinline__ void lds_row_issue(double* w, unsigned base, double& pv) {
  static_assert(LS == 17, "17 loads");
  const unsigned long long mask = 0x0001000100010001ULL << U;
  unsigned long long saved;
  // ("memory": the stores into the staged rows are only read here)
  asm volatile(
      "s_mov_b64 %[sv], exec\n\t"
      "s_mov_b64 exec, %[mk]\n\t"
      "ds_read_b64 %[w0], %[a] offset:0\n\t"
      "ds_read_b64 %[w1], %[a] offset:8\n\t"
      "ds_read_b64 %[w2], %[a] offset:16\n\t"
      "ds_read_b64 %[w3], %[a] offset:24\n\t"
      "ds_read_b64 %[w4], %[a] offset:32\n\t"
      "ds_read_b64 %[w5], %[a] offset:40\n\t"
      "ds_read_b64 %[w6], %[a] offset:48\n\t"
      "ds_read_b64 %[w7], %[a] offset:56\n\t"
      "ds_read_b64 %[w8], %[a] offset:64\n\t"
      "ds_read_b64 %[w9], %[a] offset:72\n\t"
      "ds_read_b64 %[w10], %[a] offset:80\n\t"
      "ds_read_b64 %[w11], %[a] offset:88\n\t"
      "ds_read_b64 %[w12], %[a] offset:96\n\t"
      "ds_read_b64 %[w13], %[a] offset:104\n\t"
      "ds_read_b64 %[w14], %[a] offset:112\n\t"
      "ds_read_b64 %[w15], %[a] offset:120\n\t"
      "ds_read_b64 %[w16], %[a] offset:128\n\t"
      "s_mov_b64 exec, %[sv]"
      : [sv] "=&s"(saved), [pv] "+v"(pv), [w0] "+v"(w[U + 0]), [w1] "+v"(w[U + 1]), [w2] "+v"(w[U + 2]), [w3] "+v"(w[U + 3]), [w4] "+v"(w[U + 4]), [w5] "+v"(w[U + 5]), [w6] "+v"(w[U + 6]), [w7] "+v"(w[U + 7]), [w8] "+v"(w[U + 8]), [w9] "+v"(w[U + 9]), [w10] "+v"(w[U + 10]), [w11] "+v"(w[U + 11]), [w12] "+v"(w[U + 12]), [w13] "+v"(w[U + 13]), [w14] "+v"(w[U + 14]), [w15] "+v"(w[U + 15]), [w16] "+v"(w[U + 16])
      : [a] "v"(base), [mk] "s"(mask)
      : "memory");
}

// (`dep`, unchanged, ties the wait after the value the caller computes under the loads)
template <int U>
__device__ __forceinline__ void lds_row_wait(double* w, double& dep) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(dep), "+v"(w[U]), "+v"(w[U + 1]), "+v"(w[U + 2]), "+v"(w[U + 3]), "+v"(w[U + 4]),
                 "+v"(w[U + 5]), "+v"(w[U + 6]), "+v"(w[U + 7]), "+v"(w[U + 8]),
                 "+v"(w[U + 9]), "+v"(w[U + 10]), "+v"(w[U + 11]), "+v"(w[U + 12]),
                 "+v"(w[U + 13]), "+v"(w[U + 14]), "+v"(w[U + 15]), "+v"(w[U + 16]));
}

// ---------------------------------------------------------------------------------------
// kernel 2: banded Cholesky solves, 4 lambdas per wave (one 16-lane DPP row each).
//
// Lane p of a row holds the band row r (r = p mod 16) of the 16-row window j+1..j+16 (the
// retiring pivot lane takes row j+16 in the same step), columns j..j+16 in 17 registers
// (slot k <-> column j+k, shifted one slot per step).  Every cross-lane value is a
// row_newbcast DPP move, and 4 independent solves share each instruction.  The entering rows
// (the same for the workgroup's 16 lambdas) are staged in LDS one block ahead and read by the
// pivot lane straight into its window (exec-masked ds_reads in flight during the pivot's rsq
// chain; measured 543 / 860 us vs 593 / 928 us for the big / small cells of the headline step
// with a 17-register row prefetch and VALU moves).  Slots right of a row's diagonal hold
// garbage that is never read.
// ---------------------------------------------------------------------------------------
constexpr int NTS = 256;      // 4 waves x 4 rows = 16 lambdas per workgroup

// 168 VGPRs: 3 waves per SIMD (the entering rows come from LDS, not a register prefetch).
__global__ __launch_bounds__(NTS, 3) void ridge_band_solve_kernel(
    const RidgeCellDesc* __restrict__ cells, const double* __restrict__ lvec, int L,
    double* __restrict__ work, long long* __restrict__ tim, int ncells,
    int* __restrict__ lu_count) {
  const long long t_start = (long long)__builtin_amdgcn_s_memtime();
  // the repair list count of kernel 2b starts at zero (no separate fill launch)
  if (lu_count != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *lu_count = 0;
  const int nb = (L + 15) / 16;
  const int cell = blockIdx.x / nb;
  const RidgeCellDesc cd = cells[cell];
  const int n = cd.n;
  const int p = threadIdx.x & 15;
  const int l = (blockIdx.x % nb) * 16 + (threadIdx.x >> 4);
  const bool lv = l < L;
  const int lc = lv ? l : L - 1;                 // padding rows redo the last lambda
  BandWork bw(work + cd.work, n, L);
  const double lam = lvec[lc];
  double* Lrow = bw.Lf + (int64_t)lc * n * BB;   // row j: l_{j+1..j+16, j}
  double* Linv = bw.Lf + (int64_t)L * n * BB + (int64_t)lc * n;
  double* yl = bw.Yt + (int64_t)lc * n;
  const double* LB = bw.LB;                      // row-major band: LB[r][s] = B[r][r-16+s]
  const double* z = bw.z;

  // w: 32 slots; within a 16-step block at phase u, slot u + k <-> column j + k (k <= 16), so
  // the window never shifts inside a block (one 16-slot move per block).  Rows >= n are
  // identity rows, so every block is a full, branch-free 16 steps.  The band rows entering
  // during a block are the same for all 16 lambdas of the workgroup: they are staged in LDS one
  // block ahead (double buffer, one barrier per block) and each lane reads its row at the
  // block start, instead of a second 17-register prefetch per lane (occupancy: VGPRs).
  __shared__ double LBs[2][BB][LS];
  // LDS byte offset of LBs (the low word of its flat address)
  const unsigned lbs_base = (unsigned)reinterpret_cast<uintptr_t>(&LBs[0][0][0]);
  const int npad = (n + 15) & ~15;
  double w[2 * BB];
  auto stage_rows = [&](int r0s, int buf) {       // rows r0s .. r0s + 15 -> LBs[buf]
    for (int e = threadIdx.x; e < BB * LS; e += NTS) {
      const int r = r0s + e / LS, s = e % LS;
      LBs[buf][e / LS][s] = (r < n) ? LB[(int64_t)r * LS + s] : (s == BB ? 1.0 : 0.0);
    }
  };
  // the same in two halves: the global loads at a block's start into two registers per thread
  // (BB * LS = 272 <= 2 NTS), the LDS stores at its end, so the loads' latency is spent under
  // the block's 16 steps instead of in front of them
  static_assert(BB * LS <= 2 * NTS, "two staged doubles per thread");
  double st[2];
  auto load_rows = [&](int r0s) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = threadIdx.x + h * NTS;
      const int r = r0s + e / LS, s = e % LS;
      st[h] = (e < BB * LS && r < n) ? LB[(int64_t)r * LS + s] : (s == BB ? 1.0 : 0.0);
    }
  };
  auto store_rows = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = threadIdx.x + h * NTS;
      if (e < BB * LS) LBs[buf][e / LS][e % LS] = st[h];
    }
  };
  // window at j = 0: lane p holds row p, slot k <-> column k
#pragma unroll
  for (int k = 0; k < 2 * BB; ++k)
    w[k] = (k <= p && p < n) ? LB[(int64_t)p * LS + BB - p + k] + (k == p ? lam : 0.0)
                             : (k == p ? 1.0 : 0.0);
  double zr = (p < n) ? z[p] : 0.0;
  stage_rows(BB, 0);                               // block 0's entering rows 16..31
  double znx = (p + BB < n) ? z[p + BB] : 0.0;
  bool ok = true;
  __syncthreads();

  // every prologue load (window, z) done here: otherwise the compiler's wait for the first
  // in-loop use of zr is a vmcnt(0) at the top of EVERY block, which also drains the block's
  // own staging loads issued just before it
  __builtin_amdgcn_s_waitcnt(0x0F70);              // vmcnt(0)
  // One 16-step block.  CHECK (the last block only): rows >= n are identity rows and store
  // nothing.  Elsewhere the stores need no condition: a padding lane (lambda >= L) redoes
  // lambda L-1 bit for bit, so its stores repeat the same values; 1 / l_jj and y_j are kept by
  // the pivot lane and stored once per block (16 lanes, one line) instead of per step.
  auto fwd_block = [&](int j0, auto CHECK) {
    constexpr bool chk = decltype(CHECK)::value;
    const int sb = (j0 >> 4) & 1;
    // this block's entering row for lane p (row j0 + 16 + p, taken at step p), then the NEXT
    // block's rows to the other buffer
    const double lam_in = (j0 + BB + p < n) ? lam : 0.0;   // diagonal shift of the entering row
    load_rows(j0 + 2 * BB);                        // -> LBs[sb ^ 1] at the block's end
    const double znx2 = (j0 + 2 * BB + p < n) ? z[j0 + 2 * BB + p] : 0.0;
    double myinv = 0.0, myy = 0.0;
    static_for<0, 16>([&](auto U) {
      constexpr int u = decltype(U)::value;
      const int j = j0 + u;
      const bool pl = (p == u);                  // pivot lane: holds row j, takes row j+16
      double piv = row_bcast<u>(w[u]);
      const double zpiv = row_bcast<u>(zr);      // (read before the pivot lane's zr changes)
      // LDS reads straight into the pivot lane's window, in flight during the pivot's rsq chain
      lds_row_issue<u>(w, lbs_base + (unsigned)(sb * BB * LS + u * LS) * 8u, piv);
      ok = ok && (piv > 0.0);
      double inv = rsqrt1_f64(piv);
      lds_row_wait<u>(w, inv);
      const double yj = zpiv * inv;
      if (pl) {
        w[u + BB] += lam_in;
        zr = znx;
        myinv = inv;
        myy = yj;
      }
      const double lval = w[u] * inv;            // l_i, i = (p - u) mod 16, pivot lane: i = 16
      if (!chk || j < n) Lrow[(int64_t)j * BB + (pl ? BB - 1 : ((p - u) & 15) - 1)] = lval;
      zr -= lval * yj;
      static_for<1, LS>([&](auto K) {
        constexpr int k = decltype(K)::value;
        fnmac_bcast<(u + k) & 15, k == 1>(w[u + k], lval, lval);   // w -= l_k * l_i
      });
    });
    if (!chk || j0 + p < n) {
      Linv[j0 + p] = myinv;
      yl[j0 + p] = myy;
    }
#pragma unroll
    for (int s = 0; s < BB; ++s) w[s] = w[s + BB];
    znx = znx2;
    store_rows(sb ^ 1);
    __syncthreads();                               // next block's rows staged; this buffer free
  };
  for (int j0 = 0; j0 < npad - 16; j0 += 16) fwd_block(j0, std::false_type{});
  fwd_block(npad - 16, std::true_type{});
  // back substitution L^T x = y, x overwrites y.  Lane (j+i) mod 16 holds x_{j+i} (xr); every
  // lane also holds the last two x (x1 = x_{j+1}, x2 = x_{j+2}).  Step j only waits on
  //     x_j = ((y_j - P_j) - l_{j+2,j} x2 - l_{j+1,j} x1) / l_jj,
  // P_j = sum_{i=3..16} l_{j+i,j} x_{j+i} being reduced over the row two steps earlier (its x
  // are all known then), so the 16-lane sum is off the step-to-step chain (two fmas and a mul
  // on it instead of a product, four DPP add levels, a subtract and a mul).  The factor data of
  // a block's 16 steps come in two halves of 8, each loaded one half ahead.
  __syncthreads();
  const long long t_mid = (long long)__builtin_amdgcn_s_memtime();
  struct Half {
    double pl[8], iv[8], yv[8];
  };
  // step s of the block at jb: j = jb - s, u = j & 15 = 15 - s; lane p's factor entry
  // l_{j+i,j}, i = (p - u) & 15 (0 -> 16).  CHECK (the first block only): rows >= n are
  // identity rows (l = 0, 1 / l_jj = 1, y = 0).  Elsewhere every row is < n and the loads are
  // branch-free (a row < 0, prefetched past the end, is clamped and never used): with a branch
  // per load the compiler waited for ALL loads (the prefetch included) at the first use.
  auto load_half = [&](int jb, auto S0, auto CHECK, Half& h) {
    constexpr int s0 = decltype(S0)::value;
    static_for<0, 8>([&](auto V) {
      constexpr int v = decltype(V)::value;
      constexpr int u = 15 - s0 - v;
      const int j = jb - s0 - v;
      const int i = (p - u) & 15;
      if constexpr (decltype(CHECK)::value) {
        const bool in = j < n;
        h.pl[v] = in ? Lrow[(int64_t)j * BB + (i == 0 ? BB - 1 : i - 1)] : 0.0;
        h.iv[v] = in ? Linv[j] : 1.0;
        h.yv[v] = in ? yl[j] : 0.0;
      } else {
        const int jc = max(j, 0);
        h.pl[v] = Lrow[(int64_t)jc * BB + (i == 0 ? BB - 1 : i - 1)];
        h.iv[v] = Linv[jc];
        h.yv[v] = yl[jc];
      }
    });
  };
  double xr = 0.0, x1 = 0.0, x2 = 0.0;
  double Pq[2] = {0.0, 0.0}, L1q[2] = {0.0, 0.0}, L2q[2] = {0.0, 0.0};
  // the row of step s + 2 (phase u' = u - 2, factor entries pl): its P from xr before step s's
  // update, its two critical coefficients broadcast from lanes u' + 1, u' + 2
  auto prep = [&](auto UP, double pl) {
    constexpr int up = decltype(UP)::value & 15;
    const int i = (p - up) & 15;
    const double pm = (i == 1 || i == 2) ? 0.0 : pl;
    Pq[0] = Pq[1];
    L1q[0] = L1q[1];
    L2q[0] = L2q[1];
    Pq[1] = row16_sum(pm * xr);
    L1q[1] = row_bcast<(up + 1) & 15>(pl);
    L2q[1] = row_bcast<(up + 2) & 15>(pl);
  };
  auto step = [&](double yv, double iv) {
    const double t = fma(-L2q[0], x2, yv - Pq[0]);
    const double xj = fma(-L1q[0], x1, t) * iv;
    x2 = x1;
    x1 = xj;
    return xj;
  };
  auto store_half = [&](int jb, int s0) {   // lanes u of the half hold their x in xr
    const int j = jb - (15 - p);
    if (lv && j < n && 15 - p >= s0 && 15 - p < s0 + 8) yl[j] = ok ? xr : __builtin_nan("");
  };
  using I0 = std::integral_constant<int, 0>;
  using I8 = std::integral_constant<int, 8>;
  Half A, B;
  load_half(npad - 1, I0{}, std::true_type{}, A);
  // the first two rows' P, l (rows >= n: zero factor, so zero from xr = 0 anyway)
  {
    Pq[1] = 0.0;
    L1q[1] = row_bcast<0>(A.pl[0]);   // u = 15: lanes 0, 1
    L2q[1] = row_bcast<1>(A.pl[0]);
    Pq[0] = Pq[1]; L1q[0] = L1q[1]; L2q[0] = L2q[1];
    Pq[1] = 0.0;
    L1q[1] = row_bcast<15>(A.pl[1]);  // u = 14: lanes 15, 0
    L2q[1] = row_bcast<0>(A.pl[1]);
  }
  auto block = [&](int jb, auto FIRST) {
    load_half(jb, I8{}, FIRST, B);
    static_for<0, 8>([&](auto V) {
      constexpr int v = decltype(V)::value;
      constexpr int u = 15 - v;
      const double xj = step(A.yv[v], A.iv[v]);
      if constexpr (v + 2 < 8) prep(std::integral_constant<int, u - 2>{}, A.pl[v + 2]);
      else prep(std::integral_constant<int, u - 2>{}, B.pl[v - 6]);
      xr = (p == u) ? xj : xr;
    });
    store_half(jb, 0);
    load_half(jb - 16, I0{}, std::false_type{}, A);
    static_for<0, 8>([&](auto V) {
      constexpr int v = decltype(V)::value;
      constexpr int u = 7 - v;
      const double xj = step(B.yv[v], B.iv[v]);
      if constexpr (v + 2 < 8) prep(std::integral_constant<int, u - 2 + 16>{}, B.pl[v + 2]);
      else prep(std::integral_constant<int, u - 2 + 16>{}, A.pl[v - 6]);
      xr = (p == u) ? xj : xr;
    });
    store_half(jb, 8);
  };
  block(npad - 1, std::true_type{});
  for (int jb = npad - 17; jb >= 0; jb -= 16) block(jb, std::false_type{});
  if (tim != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {   // debug: wave 0 of block 0
    const long long t_end = (long long)__builtin_amdgcn_s_memtime();
    tim[timing_solve_slot(ncells) + 0] = t_mid - t_start;
    tim[timing_solve_slot(ncells) + 1] = t_end - t_mid;
  }
}

// ---------------------------------------------------------------------------------------
// kernel 2b: the lambdas whose banded Cholesky failed (Dbar + l I not numerically SPD: l = 0
// on a rank-deficient Dbar, PFML_Search_Coef.py:131-133 / General_functions.py:81) are
// re-solved IN THE BAND DOMAIN by LU with partial pivoting (the LAPACK dgbtf2 pivot order) on
// (B + l I) y = z, before the back-transform turns y into beta = Q y.  Q is orthogonal, so this
// is a backward-stable solve of (Dbar + l I) beta = rbar, the system np.linalg.solve sees, at
// O(n BB^2) per system instead of the O(n^3) dense pivoted LU it replaces.
//
//   band_lu_flag_kernel  one thread per (cell, lambda): a NaN-marked y appends it to a list
//   ridge_band_lu_kernel LU_WG one-wave workgroups walk the list.  Window of the 17 live rows
//                        (slot = row mod 17) x 33 columns (slot = column mod 33: with
//                        pivoting U has upper bandwidth 2 BB) in LDS; the pivot row goes to
//                        an LDS copy of U, then 16 x 32 lanes eliminate and the row 17 below
//                        enters the freed slot (its loads issued two steps ahead).  Back substitution from LDS, y written back.
//                        An exactly zero pivot (singular: the reference raises LinAlgError)
//                        leaves the NaN.
// ---------------------------------------------------------------------------------------
constexpr int LR = BB + 1;          // live rows of the pivoting window
constexpr int UW = 2 * BB + 1;      // U row width (upper bandwidth 2 BB after pivoting)
constexpr int LU_WG = 128;

__global__ __launch_bounds__(256) void band_lu_flag_kernel(const RidgeCellDesc* __restrict__ cells,
                                                           int ncells, int L,
                                                           double* __restrict__ work,
                                                           int* __restrict__ list,
                                                           int* __restrict__ count, int cap) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ncells * L) return;
  const int c = e / L, l = e % L;
  const RidgeCellDesc cd = cells[c];
  const BandWork bw(work + cd.work, cd.n, L);
  const double y0 = bw.Yt[(int64_t)l * cd.n];
  if (y0 != y0) {
    const int slot = atomicAdd(count, 1);
    if (slot < cap) list[slot] = e;
  }
}

__global__ __launch_bounds__(64) void ridge_band_lu_kernel(
    const RidgeCellDesc* __restrict__ cells, const double* __restrict__ lvec, int L,
    double* __restrict__ work, const int* __restrict__ list, const int* __restrict__ count,
    int cap) {
  __shared__ double Us[BNMAX][UW];    // U rows: Us[k][c] = U[k][k + c]
  __shared__ double ys[BNMAX];        // L^-1 z, then y
  __shared__ double W[LR][UW];        // live rows k..k+16, columns k..k+32 (both mod-indexed)
  __shared__ double Z[LR];
  const int total = min(*count, cap);
  const int lane = threadIdx.x;
  for (int q = blockIdx.x; q < total; q += gridDim.x) {
    const int e = list[q];
    const RidgeCellDesc cd = cells[e / L];
    const int l = e % L, n = cd.n;
    BandWork bw(work + cd.work, n, L);
    const double lam = lvec[l];
    const double* __restrict__ LB = bw.LB;
    // B(r, c) + lam delta_rc for |r - c| <= BB (symmetric band, lower half stored)
    auto band = [&](int r, int c) -> double {
      if (r >= n || c >= n || c < 0 || abs(r - c) > BB) return 0.0;
      const int hi = max(r, c), lo = min(r, c);
      return LB[(int64_t)hi * LS + lo - hi + BB] + (r == c ? lam : 0.0);
    };
    for (int x = lane; x < LR * UW; x += 64) W[x / UW][x % UW] = band(x / UW, x % UW);
    if (lane < LR) Z[lane] = lane < n ? bw.z[lane] : 0.0;
    __syncthreads();
    // entering rows prefetched two steps ahead (their global loads overlap two steps of
    // elimination instead of stalling each step): the k loop is unrolled by two with one
    // register pair per parity, loads are unconditional (clamped) and the masks are applied
    // where the values are used - a select right after a load, a load under a branch or a
    // register copy would each wait for the load at once
    auto fetch = [&](int k, double& ev, double& zv) {
      const int r = k + LR, c = k + 1 + lane;
      const int hi = max(r, c), lo = min(r, c);
      ev = LB[(int64_t)min(hi, n - 1) * LS + max(0, min(BB, lo - hi + BB))];
      zv = bw.z[min(r, n - 1)];
    };
    // one elimination step; false on an exactly zero / NaN pivot
    auto step = [&](int k, double& ev, double& zv) -> bool {
      const int ks = k % LR, kc = k % UW;
      // pivot: first max |W[k + i][k]|, i = 0..16 (idamax order)
      double a = (lane < LR && k + lane < n) ? fabs(W[(k + lane) % LR][kc]) : -1.0;
      int ia = lane;
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) {
        const double oa = __shfl_xor(a, off, 32);
        const int oi = __shfl_xor(ia, off, 32);
        if (oa > a || (oa == a && oi < ia)) { a = oa; ia = oi; }
      }
      const int ip = __shfl(ia, 0);
      if (ip != 0) {
        const int ps = (k + ip) % LR;
        if (lane < UW) {
          const double t0 = W[ks][lane];
          W[ks][lane] = W[ps][lane];
          W[ps][lane] = t0;
        }
        if (lane == 0) {
          const double t0 = Z[ks];
          Z[ks] = Z[ps];
          Z[ps] = t0;
        }
      }
      __syncthreads();
      const double piv = W[ks][kc];
      if (piv == 0.0 || piv != piv) return false;
      const double rp = 1.0 / piv;
      const double zk = Z[ks];
      if (lane < UW) Us[k][lane] = W[ks][(k + lane) % UW];
      if (lane == 0) ys[k] = zk;
      // eliminate rows k+1..k+16, columns k+1..k+32: lane -> column 1 + (lane & 31), rows
      // 1 + (lane >> 5) + 2 t
      const int c = 1 + (lane & 31);
      const double uc = W[ks][(k + c) % UW];
      double zm = 0.0;
      if (lane < BB && k + 1 + lane < n) zm = W[(k + 1 + lane) % LR][kc] * rp;
#pragma unroll
      for (int t = 0; t < BB / 2; ++t) {
        const int i = 1 + (lane >> 5) + 2 * t;
        if (k + i < n) {
          const int rs = (k + i) % LR;
          const double m = W[rs][kc] * rp;
          W[rs][(k + c) % UW] -= m * uc;
        }
      }
      if (lane < BB && k + 1 + lane < n) Z[(k + 1 + lane) % LR] -= zm * zk;
      __syncthreads();
      // row k + 17 enters the pivot row's slot (columns k+1 .. k+33); the other rows' column
      // k slot becomes column k + 33, zero for them
      const int r = k + LR, col = k + 1 + lane;
      if (lane < UW)
        W[ks][col % UW] = (r < n && col < n) ? ev + (r == col ? lam : 0.0) : 0.0;
      if (lane < BB) W[(k + 1 + lane) % LR][kc] = 0.0;
      if (lane == 0) Z[ks] = r < n ? zv : 0.0;
      fetch(k + 2, ev, zv);
      __syncthreads();
      return true;
    };
    double eA, zA, eB, zB;
    fetch(0, eA, zA);
    fetch(1, eB, zB);
    bool singular = false;
    for (int k = 0; k < n; k += 2) {
      if (!step(k, eA, zA)) { singular = true; break; }
      if (k + 1 < n && !step(k + 1, eB, zB)) { singular = true; break; }
    }
    if (!singular) {
      for (int k = n - 1; k >= 0; --k) {
        double s = (lane >= 1 && lane < UW && k + lane < n) ? Us[k][lane] * ys[k + lane] : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) ys[k] = (ys[k] - s) / Us[k][0];
        __syncthreads();
      }
      double* __restrict__ yl = bw.Yt + (int64_t)l * n;
      for (int j = lane; j < n; j += 64) yl[j] = ys[j];
    }
    __syncthreads();
  }
}

}  // namespace

void band_solve_launch(const RidgeLaunchArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(ridge_band_solve_kernel, dim3(a.ncells * ((a.L + 15) / 16)), dim3(NTS), 0,
                     st, a.cells, a.lvec, a.L, a.work, a.timing, a.ncells, a.lu_count);
  if (a.lu_count != nullptr) {   // non-SPD lambdas: pivoted banded LU (count zeroed by kernel 2)
    hipLaunchKernelGGL(band_lu_flag_kernel, dim3((a.ncells * a.L + 255) / 256), dim3(256), 0, st,
                       a.cells, a.ncells, a.L, a.work, a.lu_list, a.lu_count, a.lu_cap);
    hipLaunchKernelGGL(ridge_band_lu_kernel, dim3(LU_WG), dim3(64), 0, st, a.cells, a.lvec, a.L,
                       a.work, a.lu_list, a.lu_count, a.lu_cap);
  }
}
