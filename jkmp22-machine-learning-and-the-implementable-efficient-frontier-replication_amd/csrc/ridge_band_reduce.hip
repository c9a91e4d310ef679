// Band path of the ridge grid, kernel 1: reduction of each cell's Dbar to band form by the
// cooperative two-sided blocked Householder (overview: ridge_band.hip), its launcher, and the
// panel-QR micro-benchmark.
#include "ridge_band.h"

namespace {

constexpr int NTR = 512;            // reduce kernel: 8 waves
constexpr int NWR = NTR / 64;
constexpr int TBR = 4;              // trailing-update tiles per wave per pass

// ---------------------------------------------------------------------------------------
// kernel 1: band reduction of one cell.
// ---------------------------------------------------------------------------------------
// X = U^-1 for upper U given by columns (lane c16: uc[i] = U[i][c16]) and di[i] = 1 / U[i][i];
// x[i] = X[i][c16].  Only entries above the diagonal of uc are read.
__device__ __forceinline__ void triu_inv16(const double (&uc)[BB], const double (&di)[BB],
                                           double (&x)[BB], int c16) {
  // right-looking: row k of X is final once the rows below it are; its update of the rows
  // above is 16 independent accumulations (back-to-back FMAs, no dependent chain)
  double acc[BB];
#pragma unroll
  for (int i = 0; i < BB; ++i) acc[i] = 0.0;
  static_for<0, BB>([&](auto KK) {
    constexpr int k = BB - 1 - decltype(KK)::value;
    x[k] = ((c16 == k) ? 1.0 + acc[k] : acc[k]) * di[k];
    const double nxk = -x[k];
    static_for<0, k>([&](auto I) {
      constexpr int i = decltype(I)::value;
      fmac_bcast<k, true>(acc[i], uc[i], nxk);     // acc[i] -= U[i][k] X[k][c16]
    });
  });
}

// P1 + P2 + T of one panel, by one NTR-thread workgroup: the m x 16 panel below the band
// (columns r0.. of rows k0..k0+15 of the symmetric A) is QR-factored by Householder in
// registers; V (unit lower trapezoid) -> Vs, V and R -> A's panel columns, the compact-WY T
// (dlarft) -> Ts and Tglob.  Ends with a barrier.  `redf` needs 2 x 256 + 32 doubles.
// `n` is A's leading dimension.  `Pn`: the panel is read from this LDS image (Pn[i][c] = panel
// row i, column c; it may alias Vs) instead of A's mirror row.
// (A CholeskyQR2 form with Householder reconstruction measured 45-60 % slower per panel,
// profiles/r04_qr_bench_dpp.jsonl, and was removed.)
__device__ __forceinline__ void band_panel_hh(double* __restrict__ A, int n, int k0, int r0,
                                              int m, double (*Vs)[LS], double (*Gs)[LS],
                                              double* redf, double (*Ts)[LS], double* taus,
                                              double* __restrict__ Tglob, long long* tk,
                                              const double (*Pn)[LS]) {
  const int t = threadIdx.x, lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cq = t & 15, rg = t >> 4;
  const int c16 = lane & 15, g4 = lane >> 4;
  // ---- P1: thread (rg, cq) loads rows i = rg + 32 q (q < 16) of panel column cq straight
  //      into registers (row k0+cq of the symmetric A; all 16 loads in flight at once)
  double a[16];
  if (Pn != nullptr) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = rg + 32 * q;
      a[q] = (i < m) ? Pn[i][cq] : 0.0;
    }
  } else {
    const double* src = A + (int64_t)(k0 + cq) * n + r0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = rg + 32 * q;
      a[q] = (i < m) ? src[i] : 0.0;
    }
  }
  if (tk) tk[0] = (long long)__builtin_amdgcn_s_memtime();
  // ---- P2: Householder QR of the m x 16 panel in REGISTERS: column j reaches the 16 lanes
  //      of a row group by row_newbcast DPP, fused into the FMA that consumes it
  //      (v_fmac_f64_dpp); one barrier per column (cross-wave sums, ping-pong buffers).
  //      A finished column keeps its Householder vector UNSCALED below the diagonal (u = the
  //      column at its own step; v = scal u): its scal is applied once, when V is written, and
  //      the dlarft dots of later steps carry it as one factor - so every element costs two
  //      fp64 operations per step (its share of the dots and its update), not five.
  double tau_r[BB];
  double myscal = 0.0;                           // scal of this lane's column once finished
  static_for<0, BB>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const int par = j & 1;
    // (tk: per-column sub-phases of thread 0's wave, accumulated in tk[2..4]: own work before
    // the barrier, barrier wait, reductions + pivot chain + update after it)
    const long long tc0 = tk ? (long long)__builtin_amdgcn_s_memtime() : 0;
    double s1p[4] = {0.0, 0.0, 0.0, 0.0};
    // Only row group q = 0 (rows < 32) meets the diagonal; groups of four row groups at or
    // beyond m are all-zero and skipped (one wave-uniform branch per four).  Four partial
    // sums break the FMA chain.
#pragma unroll
    for (int q4 = 0; q4 < 16; q4 += 4) {
      if (q4 > 0 && 32 * q4 >= m) continue;
#pragma unroll
      for (int q = q4; q < q4 + 4; ++q) {
        const int i = rg + 32 * q;
        const double mq = (q > 0 || i > j) ? a[q] : 0.0;       // rows below the diagonal
        // (DPP source a[q]: only a[0] can have been written by a plain VALU op just before -
        // the diagonal fix-up of the last column; every other a[q] was last written by this
        // asm sequence >= 2 instructions earlier, so only q = 0 needs the 2 wait states)
        if (q == 0) fmac_bcast<j, true>(s1p[q & 3], a[q], mq);  // += x_j[i] a_cq[i]
        else fmac_bcast<j, false>(s1p[q & 3], a[q], mq);
      }
    }
    // sum over the wave's 4 row groups (lanes l, l^16, l^32, l^48): VALU lane swaps
    const double s1 = rowgroup_sum((s1p[0] + s1p[1]) + (s1p[2] + s1p[3]));
    if (lane < 16) redf[par * 256 + wid * 16 + lane] = s1;
    if (rg == j) redf[512 + par * 16 + cq] = a[0];       // row j (q = 0)
    long long tc1 = 0;
    if (tk) {
      tc1 = (long long)__builtin_amdgcn_s_memtime();
      tk[2] += tc1 - tc0;
    }
    __syncthreads();
    if (tk) {
      const long long tc2 = (long long)__builtin_amdgcn_s_memtime();
      tk[3] += tc2 - tc1;
      tk[5] = tc2;
    }
    // the wave partials summed as a depth-3 tree (not an 8-deep chain), and the column's
    // scalars below without a branch, so the dc sum overlaps the rsq / rcp chain instead of
    // following it (the compiler kept every instruction after a data-dependent branch behind it)
    static_assert(NWR == 8, "tree sum of 8 wave partials");
    double xs[NWR], ds[NWR];
#pragma unroll
    for (int w = 0; w < NWR; ++w) {
      xs[w] = redf[par * 256 + w * 16 + j];
      ds[w] = redf[par * 256 + w * 16 + cq];
    }
    const double xn2 = ((xs[0] + xs[1]) + (xs[2] + xs[3])) + ((xs[4] + xs[5]) + (xs[6] + xs[7]));
    const double dc = ((ds[0] + ds[1]) + (ds[2] + ds[3])) + ((ds[4] + ds[5]) + (ds[6] + ds[7]));
    const double alpha = redf[512 + par * 16 + j];
    const double vjc = redf[512 + par * 16 + cq];
    // beta = -sign(alpha) ||x||, tau = 1 + |alpha| / ||x||, 1 / (alpha - beta) =
    // sign(alpha) / (|alpha| + ||x||): one rsq and one rcp chain (Newton-refined) instead of
    // the IEEE sqrt and two divide sequences on the per-column critical path.  xn2 = 0 (nothing
    // below the diagonal): tau = 0, beta = alpha, scal = 0 (the chains run on a dummy 1).
    const bool zc = xn2 == 0.0;
    const double nrm2 = zc ? 1.0 : fma(alpha, alpha, xn2);
    const double rn = rsqrt_f64(nrm2);
    const double nrm = nrm2 * rn;
    const double beta = zc ? alpha : -copysign(nrm, alpha);
    const double tau = zc ? 0.0 : fma(fabs(alpha), rn, 1.0);
    const double scal = zc ? 0.0 : copysign(rcp_f64(fabs(alpha) + nrm), alpha);
    // v_j' a_cq = a_cq[j] + scal sum_{i > j} x_j[i] a_cq[i] = vjc + scal dc: for cq > j the
    // update coefficient wc = tau (...), for a finished column cq < j (unscaled u_cq, factor
    // myscal) the dlarft dot G[cq][j] = v_cq' v_j = myscal (...): G = V'V comes free
    const double gcj = vjc + scal * dc;
    const double wc = tau * gcj;
    if (t < j) Gs[t][j] = myscal * gcj;          // (t < 16: row group 0, cq = t)
    tau_r[j] = tau;
    const bool upd = cq > j, own = cq == j;
    if (own) myscal = scal;
    // columns cq > j: a[i] -= v_j[i] wc = scal x_j[i] wc below the diagonal, a[j] -= wc on
    // it; column j: beta on the diagonal, u = x below it (scaled later); cq < j: unchanged
    const double nsw = upd ? -(scal * wc) : 0.0;
#pragma unroll
    for (int q4 = 0; q4 < 16; q4 += 4) {
      if (q4 > 0 && 32 * q4 >= m) continue;
#pragma unroll
      for (int q = q4; q < q4 + 4; ++q) {
        const int i = rg + 32 * q;
        if (q == 0) {
          const double ns0 = (i > j) ? nsw : 0.0;
          fmac_bcast<j, true>(a[0], a[0], ns0);
          if (i == j) a[0] = upd ? a[0] - wc : (own ? beta : a[0]);
        } else {
          fmac_bcast<j, false>(a[q], a[q], nsw);
        }
      }
    }
    if (t == 0) taus[j] = tau;
    if (tk) tk[4] += (long long)__builtin_amdgcn_s_memtime() - tk[5];
  });
  // explicit V -> Vs (MFMA operand); V (strictly lower) and R (upper) -> A's panel columns
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = rg + 32 * q;
    const double v = a[q] * myscal;
    Vs[i][cq] = (i > cq) ? v : ((i == cq && i < m) ? 1.0 : 0.0);
    if (i < m) A[(int64_t)(r0 + i) * n + k0 + cq] = (i > cq) ? v : a[q];
  }
  __syncthreads();
  if (tk) tk[1] = (long long)__builtin_amdgcn_s_memtime();
  // ---- T of the compact WY form: T^-1 = diag(1 / tau) + striu(V'V) (Puglisi; Joffrain,
  //      Low, Quintana-Orti, van de Geijn, "Accumulating Householder transformations,
  //      revisited", 2006), inverted in registers by every wave (lane c16: column c16 of U,
  //      1 / U_kk = tau_k - a zero tau gives a zero row and column of T, as dlarft does)
  {
    double uc[BB], tc[BB];
#pragma unroll
    for (int i = 0; i < BB; ++i) uc[i] = (i < c16) ? Gs[i][c16] : 0.0;
    triu_inv16(uc, tau_r, tc, c16);
    if (wid == 0 && g4 == 0) {
#pragma unroll
      for (int i = 0; i < BB; ++i) Ts[i][c16] = tc[i];
    }
  }
  __syncthreads();
  if (t < BB * BB) Tglob[t] = Ts[t / BB][t % BB];
}

// ---------------------------------------------------------------------------------------
// kernel 1, cooperative form (the only form): K workgroups per cell in
// ONE launch, K chosen per cell by the host (ops/ridge.py::coop_k) so that a launch fills
// the chip whether it holds 106 big cells (one GPU) or 13 (one rank of eight).  The results
// are BITWISE independent of K: every value has one producer whose arithmetic does not
// depend on which workgroup runs it, and every cross-block sum runs over per-block partials in
// a fixed block order.  So a 1-GPU and an N-GPU grid search pick the same hyper-parameters
// (PFML_hp_reals.py:118-122 dense rank, PFML_best_hps.py:275 first rank).
//
// Work units are 16-row blocks of the trailing matrix A22, of which only the LOWER block
// triangle (diagonal tiles whole) is stored: the update writes no mirror tiles and the X phase
// reads column block I above its first row from row block I (dsytrd 'L' semantics: the
// input's upper triangle is never read).  Per panel p:
//
//   B  every WG   U = V_p T_p (LDS), X_I = A22 U for the blocks I it owns in the X phase (the
//                 QR WG the last x0(nI, K) blocks, a cost-model split; the others the rest
//                 round-robin), partials V_I' X_I and V_I' z_I per block
//   C  every WG   P = sum_I V_I' X_I and V'z in block order, M = T' P, z_I -= V_I T' V'z,
//                 W_I = X_I - V_I M / 2 for its X blocks
//   D  QR WG      look-ahead: the tiles (I, 0) of A22 ARE panel p+1; it applies update p to
//                 them in registers and factors panel p+1 (band_panel_hh) while
//      others     apply A22 -= V W' + W V' to their update blocks, tiles (I, J), 1 <= J <= I
//                 (tile (0, 0): the diagonal band block)
//
// With K = 1 the one workgroup runs D's update first, then the look-ahead panel: the same
// operations in the same order.  Hand-offs between the workgroups of a cell
// (cdna_hip_programming.md Guideline 16): every handed-off byte is stored write-through (sc1:
// 8- and 16-byte buffer stores through descriptors on the cell's workspace), every storing
// wave drains (s_waitcnt vmcnt(0)) before the workgroup barrier behind which one lane adds to
// the cell's arrival counter; consumers poll that counter relaxed and read the small payloads
// (V, T, W, partials, z) with sc1 loads; the matrix reads of the X phase follow one agent-scope
// acquire per panel.  Spins are bounded (spin_max polls, RidgeLaunchArgs::spin_max): a timeout
// sets the cell's error word, every later wait of the workgroup returns at once and the launch
// drains (never a hang); the back-transform then writes NaN betas for that cell, so the grid
// search's non-finite-cell recovery (models/search.py recompute_cells, the reference's
// np.linalg.solve per lambda) replaces them, and the host counts the timed-out cells from the
// error words of every launch (ops/ridge.py coop_errors: COUNTERS ridge.coop_timeouts).
// ---------------------------------------------------------------------------------------
typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr unsigned COOP_SPIN_MAX = 1u << 22;   // default poll bound (~1 s of s_sleep 1)

struct CoopSync {
  gu32* ctr;
  gu32* err;
  int K;
  unsigned epoch;
  unsigned spin_max;
  // Every thread of the workgroup calls it; returns with the cell's K workgroups past the
  // same point.  acquire: one agent-scope acquire behind the poll (plain loads of other
  // workgroups' matrix tiles follow).
  __device__ __forceinline__ void sync(bool acquire, int* err_s) {
    ++epoch;
    if (K == 1) {
      __syncthreads();
      return;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave: its sc1 stores are out
    __syncthreads();
    if (threadIdx.x == 0) {
      __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned target = (unsigned)K * epoch;
      unsigned spins = 0;
      bool bad = *err_s != 0;
      while (!bad && __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins >= spin_max) {
          bad = true;
          *err_s = 1;
          __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (acquire) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    __syncthreads();
  }
};

// One k-chunk (NV x 8 rows of A22 from k) of the X phase for the NQ blocks of a wave, the
// first NB of which lie entirely BELOW the chunk (their first row <= k) and the rest entirely
// above it.  Lane (c16, g4) takes the k pair kk, kk + 1 (kk = k + 8 v + 2 g4) into two MFMAs (the
// k order inside the 16 x 16 x 4 steps is permuted, the same for every block and every K):
// above a block the pair is ONE 16-byte load along row i of the lower triangle (the 16 lanes of
// a k-group read 16 rows: half the load instructions of one 8-byte load per k), below it two
// row loads (coalesced along the block's 16 columns).  No per-element branch: with one the
// compiler made both paths exec-masked and waited for each load's predecessor (WAW).
template <int NQ, int NB, int NV>
__device__ __forceinline__ void coop_x_chunk(const double* __restrict__ A, int lda, int r0, int m,
                                             int k, const int (&col)[NQ], int c16, int g4,
                                             const double (*__restrict__ Us)[LS],
                                             double4_t (&X)[4]) {
  typedef double d2v __attribute__((ext_vector_type(2)));   // 16-B aligned: one dwordx4 load
  double a0[NV][NQ], a1[NV][NQ], b0[NV], b1[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int kk = k + 8 * v + 2 * g4;
    static_for<0, NQ>([&](auto Q) {
      constexpr int q = decltype(Q)::value;
      if constexpr (q < NB) {
        a0[v][q] = A[(int64_t)(r0 + min(kk, m - 1)) * lda + r0 + col[q]];
        a1[v][q] = A[(int64_t)(r0 + min(kk + 1, m - 1)) * lda + r0 + col[q]];
      } else {
        const d2v x = *reinterpret_cast<const d2v*>(A + (int64_t)(r0 + col[q]) * lda + r0 + kk);
        a0[v][q] = x.x;
        a1[v][q] = x.y;
      }
    });
    // (rows >= m of U are zero, and Us has BB zero rows behind row BMP - 1: a chunk that
    // starts 16 mod 32 runs to k = BMP + 15 at m = BMP.  Clamped to row BMP - 1, a live row
    // there, n = 528 gave wrong betas.)
    b0[v] = Us[min(kk, BMP + BB - 1)][c16];
    b1[v] = Us[min(kk + 1, BMP + BB - 1)][c16];
  }
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      X[q] = mfma_f64_16x16x4(a0[v][q], b0[v], X[q]);
      X[q] = mfma_f64_16x16x4(a1[v][q], b1[v], X[q]);
    }
}

// X_I += A22[k][I cols] U[k][:] for the NQ blocks blk[] of this wave (increasing).  Only the
// LOWER triangle of A22 is kept (the update writes no mirror tiles): element (kk, i) of column
// block I is A[kk][i] for rows kk at or below the block's first row and A[i][kk] above it - the
// same value a mirrored copy held.  The first rows of a wave's blocks are equal mod 32 (its
// blocks are 8 K' apart), so 32-row chunks aligned to them (after a 16-row head when they are
// 16 mod 32) never straddle one: each chunk is one coop_x_chunk<NQ, NB> with NB uniform.
template <int NQ>
__device__ __forceinline__ void coop_x_accum(const double* __restrict__ A, int lda, int r0,
                                             int m, const int (&blk)[4], int c16, int g4,
                                             const double (*__restrict__ Us)[LS],
                                             double4_t (&X)[4]) {
  int col[NQ], top[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    col[q] = min(blk[q] * 16 + c16, m - 1);
    top[q] = blk[q] * 16;
  }
  auto chunk = [&](int k, auto NV) {
    int nb = 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) nb += (top[q] <= k) ? 1 : 0;
    static_for<0, NQ + 1>([&](auto B) {
      if (nb == decltype(B)::value)
        coop_x_chunk<NQ, decltype(B)::value, decltype(NV)::value>(A, lda, r0, m, k, col, c16,
                                                                 g4, Us, X);
    });
  };
  int k = 0;
  if (top[0] & 16) {
    chunk(0, std::integral_constant<int, 2>{});
    k = 16;
  }
  for (; k < m; k += 32) chunk(k, std::integral_constant<int, 4>{});
}

// Trailing-update rows of each wave at K = 1, per number of live row blocks nI: row I holds
// the tiles J = 1..I (row 0: the diagonal band tile), i.e. max(1, ceil(I / TBR)) chunks of TBR
// tiles, and the rows go to the waves longest-first, each to the least-loaded wave (LPT).  The
// fixed snake (w, 15 - w, 16 + w, 31 - w) balanced only nI = 32: as the panels advance, the
// rows >= nI it drops are the long ones of the low waves, and the K = 1 update waited up to 2x
// on its slowest wave (wave 0 idle ~14 % of a cell's cycles at the barrier after the update).
// Which wave updates a tile does not change its arithmetic: the same bits.
constexpr int UPD_RMAX = 8;
constexpr int UPD_NI = BNMAX / BB + 2;
struct UpdRows {
  signed char r[UPD_NI][NWR][UPD_RMAX];
};
constexpr UpdRows make_upd_rows() {
  UpdRows t{};
  for (int nI = 0; nI < UPD_NI; ++nI) {
    int load[NWR] = {}, cnt[NWR] = {};
    for (int w = 0; w < NWR; ++w)
      for (int k = 0; k < UPD_RMAX; ++k) t.r[nI][w][k] = -1;
    for (int I = nI - 1; I >= 0; --I) {
      const int c = I == 0 ? 1 : (I + TBR - 1) / TBR;
      int best = -1;
      for (int w = 0; w < NWR; ++w)
        if (cnt[w] < UPD_RMAX && (best < 0 || load[w] < load[best])) best = w;
      t.r[nI][best][cnt[best]++] = (signed char)I;
      load[best] += c;
    }
  }
  return t;
}
__constant__ UpdRows kUpdRows = make_upd_rows();

// SOLO: the instance of a launch whose every cell has K = 1 (band_reduce_launch: nwg ==
// ncells).  K is a compile-time 1, so the hand-off code (published V / T / W / partials,
// CoopSync polling) is gone, and since no other workgroup ever reads this cell's bytes the tile
// stores, the hand-off words and z use plain accesses: a plain store keeps the line in the XCD's
// L2 for the next panel's X phase and update, where a write-through (sc1) store drops it.  The
// arithmetic is the general kernel's K = 1 path: the same bits.  The sync words are still
// passed (zeroed by the cell's workgroup at entry, no memset before the launch): the
// back-transform reads the error word, which stays 0.  z's rows >= 16 live in the padding column
// of Vs between the start-up copy and the epilogue.
template <bool TIMED, bool SOLO>
__global__ __launch_bounds__(NTR) void band_coop_kernel(
    const double* __restrict__ SD, int64_t ldS, const double* __restrict__ Sr,
    const RidgeCellDesc* __restrict__ cells, int L, double* __restrict__ work,
    const int* __restrict__ wgmap, unsigned* __restrict__ syncw, long long* __restrict__ tim,
    unsigned spin_max) {
  __shared__ double Vs[BMP][LS];       // V_p (rows >= m zero); the QR WG: panel p+1, V_{p+1}
  __shared__ double Ws[BMP + BB][LS];  // U = V T, then W; BB rows of zeros behind (X phase)
  __shared__ double red[NWR][BB * BB]; // QR scratch, canonical sums, update transposes
  __shared__ double Ts[BB][LS];
  __shared__ double taus[BB];
  __shared__ double zts[BB];
  __shared__ int err_s;

  const int code = wgmap[blockIdx.x];
  const int cell = code >> 8;
  const int w = SOLO ? 0 : (code >> 4) & 15, K = SOLO ? 1 : (code & 15) + 1;
  constexpr int AUX = SOLO ? 0 : 16;             // sc1 (write-through) unless solo
  const RidgeCellDesc cd = cells[cell];
  const int n = cd.n;
  const int lda = band_npad(n), nb = lda / BB;
  const int npan = (n - 1) / BB;                 // panels: k0 = 16 p with k0 + 16 < n
  const int t_ = threadIdx.x, lane_ = t_ & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t_ >> 6);
  BandWork bw(work + cd.work, n, L);
  CoopWork cw(bw.F, lda);
  double* __restrict__ A = bw.A;
  CoopSync cs{(gu32*)(syncw + (int64_t)cell * COOP_SYNC),
              (gu32*)(syncw + (int64_t)cell * COOP_SYNC + 1), K, 0u, spin_max};
  const bool qwg = (w == 0);
  const int Ku = K > 1 ? K - 1 : 1;            // update workgroups: all but the QR one
  const int wu = K > 1 ? w - 1 : 0;            // (-1: the QR workgroup when K > 1)
  // 16-byte write-through stores of the matrix tiles through a buffer descriptor on A (a
  // masked store gets an offset past the range and is dropped by the range check)
  const unsigned abytes = (unsigned)lda * (unsigned)lda * 8u;
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc(A, 0, (int)abytes, 0x00020000);
  auto st2 = [&](unsigned off, bool ok, double x, double y) {
    const double2 v = make_double2(x, y);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsA,
                                           ok ? off : abytes, 0, AUX);
  };
  // the hand-off words (V, T, W, partials, z) through a descriptor on the cell's workspace:
  // write-through (sc1) 8-byte buffer stores and sc1 buffer loads (not atomics: a loop's loads
  // are all in flight before the first wait)
  const auto rsW = __builtin_amdgcn_make_buffer_rsrc(A, 0, 0x7ffffff0, 0x00020000);
  auto ldw = [&](const double* p) -> double {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
                                          rsW, (unsigned)((p - A) * 8), 0, AUX));
  };
  auto stw = [&](double* p, double v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rsW,
                                          (unsigned)((p - A) * 8), 0, AUX);
  };
  // (timed instances: the clock is read at entry, so slot 0 covers the start-up copy and panel
  // 0, and the last mark follows the band epilogue, which slot 7 covers)
  long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long tlast = 0;
  if (TIMED && threadIdx.x == 0) tlast = (long long)__builtin_amdgcn_s_memtime();
#define COOP_TMARK(ph)                                                   \
  if (TIMED && threadIdx.x == 0) {                                       \
    const long long now = (long long)__builtin_amdgcn_s_memtime();       \
    tacc[ph] += now - tlast;                                             \
    tlast = now;                                                         \
  }
  if (t_ == 0) err_s = 0;
  for (int e = t_; e < BB * LS; e += NTR) (&Ws[BMP][0])[e] = 0.0;   // (visible after the sync below)

  // ---- A = S * scale (the lower block triangle incl. the diagonal blocks, zero padding),
  //      z = r * scale: row blocks gb = w (mod K)
  //      A wave takes whole rows (rows wid and wid + 8 of each block: the row index is
  //      wave-uniform, no division), its lanes the row's column pairs in chunks of 64.  CPB
  //      (row, chunk) units form one batch: their 2 CPB 8-byte loads (ldS may be odd) are all
  //      issued, at clamped addresses, before the first is used; the i < n, j < n masks are
  //      selects behind the loads and a unit past the end is a dropped store.
  if constexpr (SOLO) {
    // (no memset before a solo launch: the cell's one workgroup zeroes its own sync words;
    // nothing adds to them, and the back-transform and the host read the error word as 0)
    if (t_ < COOP_SYNC) syncw[(int64_t)cell * COOP_SYNC + t_] = 0u;
  }
  {
    const double* S = SD + cd.src;
    const double sc = cd.scale;
    constexpr int CPB = 8;
    int b = 0, h = 0, c = 0;                       // block w + K b, row wid + 8 h, chunk c
    while (w + K * b < nb) {
      double x0[CPB], x1[CPB];
      int ri[CPB], jc[CPB];
      bool ok[CPB];
#pragma unroll
      for (int u = 0; u < CPB; ++u) {
        const int gb = w + K * b;
        const int i = 16 * gb + wid + 8 * h, jp = 64 * c + lane_;
        ri[u] = i;
        jc[u] = 2 * jp;
        ok[u] = gb < nb && jp < 8 * (gb + 1);      // column pairs through the diagonal block
        const double* srow = S + (int64_t)min(i, n - 1) * ldS;
        x0[u] = srow[min(2 * jp, n - 1)];
        x1[u] = srow[min(2 * jp + 1, n - 1)];
        if (++c >= (gb + 8) >> 3) {                // ceil(8 (gb + 1) / 64) chunks per row
          c = 0;
          if (++h == 2) {
            h = 0;
            ++b;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < CPB; ++u) {
        const int i = ri[u], j = jc[u];
        // (the loaded values pinned in registers here: without it the compiler sank the last
        // load under its mask's branch and waited for it alone)
        asm volatile("" : "+v"(x0[u]), "+v"(x1[u]));
        const double x = (i < n && j < n) ? x0[u] * sc : 0.0;
        const double y = (i < n && j + 1 < n) ? x1[u] * sc : 0.0;
        st2((unsigned)((i * lda + j) * 8), ok[u], x, y);
      }
    }
    if constexpr (SOLO) {
      // z of the rows >= 16 (the ones the panels update) lives in the padding column of Vs,
      // which no other code touches: global row g at Vs[g - 16][BB] (n <= BNMAX: g - 16 < BMP)
      for (int g = t_; g < n; g += NTR) {
        const double zv = Sr[cd.rsrc + g] * sc;
        if (g < BB) stw(bw.z + g, zv);
        else Vs[g - BB][BB] = zv;
      }
    } else {
      for (int gb = w; gb < nb; gb += K)
        if (t_ < BB && 16 * gb + t_ < n) stw(bw.z + 16 * gb + t_, Sr[cd.rsrc + 16 * gb + t_] * sc);
    }
  }
  cs.sync(true, &err_s);

  // ---- panel 0 (the QR workgroup): column block 0, rows 16.., then publish V_0, T_0
  auto publish_vt = [&](int mp) {
    for (int e = t_; e < mp * BB; e += NTR) stw(cw.Vg + e, Vs[e / BB][e % BB]);
    if (t_ < BB * BB) stw(cw.Tg + t_, Ts[t_ / BB][t_ % BB]);
  };
  if (npan > 0 && qwg) {
    const int m0 = n - BB;
    // (a thread's 16 loads, rows clamped, all in flight before the first LDS write)
    double v[BMP * BB / NTR];
#pragma unroll
    for (int u = 0; u < BMP * BB / NTR; ++u) {
      const int i = (t_ >> 4) + (NTR / BB) * u;
      v[u] = A[(int64_t)(BB + min(i, m0 - 1)) * lda + (t_ & 15)];
    }
#pragma unroll
    for (int u = 0; u < BMP * BB / NTR; ++u) {
      const int i = (t_ >> 4) + (NTR / BB) * u;
      Vs[i][t_ & 15] = (i < m0) ? v[u] : 0.0;
    }
    __syncthreads();
    band_panel_hh(A, lda, 0, BB, m0, Vs, Ws, &red[0][0], Ts, taus, bw.T, nullptr, Vs);
    if (K > 1) publish_vt(m0);
  }
  if (npan > 0) cs.sync(false, &err_s);
  COOP_TMARK(0)

  for (int p = 0; p < npan; ++p) {
    const int k0 = p * BB, r0 = k0 + BB, m = n - r0;
    const int nI = (m + 15) >> 4;
    int t = t_, lane = lane_;
    asm volatile("" : "+v"(t), "+v"(lane));
    const int c16 = lane & 15, g4 = lane >> 4;
    // ---- B: V_p, T_p (the other workgroups load the published copy), U = V T -> Ws
    if (!qwg) {
      double v[BMP * BB / NTR];
#pragma unroll
      for (int u = 0; u < BMP * BB / NTR; ++u) v[u] = ldw(cw.Vg + min(t + NTR * u, m * BB - 1));
      const double tv = ldw(cw.Tg + (t & (BB * BB - 1)));
#pragma unroll
      for (int u = 0; u < BMP * BB / NTR; ++u) {
        const int e = t + NTR * u, i = e / BB;
        Vs[i][e % BB] = (i < m) ? v[u] : 0.0;
      }
      if (t < BB * BB) Ts[t / BB][t % BB] = tv;
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < BMP / 16 / NWR; ++q) {
      const int i0 = (wid + NWR * q) * 16;
      double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; ++r) acc = mfma_f64_16x16x4(Vs[i0 + c16][4 * r + g4], Ts[4 * r + g4][c16], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) Ws[i0 + g4 + 4 * r][c16] = acc[r];
    }
    __syncthreads();
    COOP_TMARK(1)
    // X blocks of this workgroup.  The QR workgroup (w = 0) also factors the next panel and
    // the others also apply the update, so the X blocks are split to balance the two: w = 0
    // takes the last x0 blocks, the K - 1 others the rest round-robin, with x0 from a cost
    // model of one panel calibrated on the MI355X phase timings (tools/bench_ridge.py
    // --timing; cycles: X 197 per block per block row, update 174 per 16 x 16 tile, panel QR
    // 30000 + 550 per block row) - large panels (update-heavy) give w = 0 about half the X
    // blocks, small ones (QR-latency-bound) none.  Which workgroup computes a block does not
    // change its arithmetic, so the betas stay bitwise independent of K.
    int x0 = nI;
    if (K > 1) {
      const float fn = (float)nI;
      const float upd = 174.0f * fn * (fn + 1.0f) * 0.5f, xs = 197.0f * fn;
      const float qr = 30000.0f + 550.0f * fn;
      const float xq = (upd + xs * fn - (float)(K - 1) * qr) / ((float)K * xs);
      x0 = min(nI, max(0, (int)(xq + 0.5f)));
    }
    int blk[4];
    int nq = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = wid + NWR * q;
      blk[q] = qwg ? nI - x0 + k : (w - 1) + (K - 1) * k;
      nq += (qwg ? k < x0 : blk[q] < nI - x0) ? 1 : 0;
    }
    double4_t X[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) X[q] = double4_t{0.0, 0.0, 0.0, 0.0};
    switch (nq) {
      case 1: coop_x_accum<1>(A, lda, r0, m, blk, c16, g4, Ws, X); break;
      case 2: coop_x_accum<2>(A, lda, r0, m, blk, c16, g4, Ws, X); break;
      case 3: coop_x_accum<3>(A, lda, r0, m, blk, c16, g4, Ws, X); break;
      case 4: coop_x_accum<4>(A, lda, r0, m, blk, c16, g4, Ws, X); break;
      default: break;
    }
    // per-block partials V_I' X_I and V_I' z_I (z as column 0 of the B operand).  With one
    // workgroup per cell (K = 1) they stay on the CU: U is dead once every wave's X is done, so
    // they go to the LDS of Ws (32 blocks x 272 doubles = exactly its 512 x 17), and W later
    // straight to Ws - no global round trip of partials and W per panel.  (Same values, same
    // summation order: bitwise the same betas as K > 1.)
    double* const Pl = &Ws[0][0];
    if (K == 1) __syncthreads();                   // every wave's reads of U are done
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < nq) {
        const int i0 = 16 * blk[q];
        double4_t Pp = {0.0, 0.0, 0.0, 0.0}, Pz = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = i0 + 4 * r + g4;
          const double va = Vs[row][c16];
          Pp = mfma_f64_16x16x4(va, X[q][r], Pp);
          double zl;                                 // (solo: z's LDS copy, row r0 + . - 16)
          if constexpr (SOLO) zl = Vs[k0 + min(row, m - 1)][BB];
          else zl = ldw(bw.z + r0 + min(row, m - 1));
          const double zb = (c16 == 0 && row < m) ? zl : 0.0;
          Pz = mfma_f64_16x16x4(va, zb, Pz);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (K == 1) {
            Pl[blk[q] * (BB * BB + BB) + (g4 + 4 * r) * BB + c16] = Pp[r];
            if (c16 == 0) Pl[blk[q] * (BB * BB + BB) + BB * BB + g4 + 4 * r] = Pz[r];
          } else {
            stw(cw.Pg + (int64_t)blk[q] * (BB * BB) + (g4 + 4 * r) * BB + c16, Pp[r]);
            if (c16 == 0) stw(cw.Pzg + blk[q] * BB + g4 + 4 * r, Pz[r]);
          }
        }
      }
    }
    COOP_TMARK(2)
    cs.sync(false, &err_s);
    COOP_TMARK(3)
    // ---- C: canonical sums (block order), M = T' P, z and W of the X blocks
    if (t < BB * BB + BB) {
      // (all nI partials in flight, then summed in block order)
      const bool isP = t < BB * BB;
      constexpr int NB = BNMAX / BB;
      double v[NB];
      if (K == 1) {
#pragma unroll
        for (int I = 0; I < NB; ++I) v[I] = Pl[min(I, nI - 1) * (BB * BB + BB) + t];
      } else {
        const double* base = isP ? cw.Pg + t : cw.Pzg + (t - BB * BB);
        const int stride = isP ? BB * BB : BB;
#pragma unroll
        for (int I = 0; I < NB; ++I) v[I] = ldw(base + min(I, nI - 1) * stride);
      }
      double s = 0.0;
#pragma unroll
      for (int I = 0; I < NB; ++I) s = (I < nI) ? s + v[I] : s;
      if (isP) red[0][t] = s;
      else red[1][t - BB * BB] = s;
    }
    __syncthreads();
    if (t < BB) {
      // (solo: the LDS reads of eight terms at a time first, then their part of the chain in
      // the same order: two round trips, not one per term.  All 32 reads at once cost the solo
      // instance scratch, and any batched form cost the general one 8 B more of it.)
      double s = 0.0;
      if constexpr (!SOLO) {
        for (int a = 0; a <= t; ++a) s = fma(Ts[a][t], red[1][a], s);
      }
#pragma unroll
      for (int a0 = 0; SOLO && a0 < BB; a0 += 8) {
        double ta[8], ra[8];
#pragma unroll
        for (int a = 0; a < 8; ++a) {
          ta[a] = Ts[a0 + a][t];
          ra[a] = red[1][a0 + a];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < 8; ++a) s = (a0 + a <= t) ? fma(ta[a], ra[a], s) : s;
        __builtin_amdgcn_sched_barrier(0);
      }
      zts[t] = s;
    }
    double4_t Mm = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r)
      Mm = mfma_f64_16x16x4(Ts[4 * r + g4][c16], red[0][(4 * r + g4) * BB + c16], Mm);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < nq) {
        const int i0 = 16 * blk[q];
        if (lane < BB && i0 + lane < m) {
          const int i = i0 + lane;
          double s = 0.0;
#pragma unroll
          for (int c = 0; c < BB; ++c) s = fma(Vs[i][c], zts[c], s);
          if constexpr (SOLO) Vs[k0 + i][BB] = Vs[k0 + i][BB] - s;
          else stw(bw.z + r0 + i, ldw(bw.z + r0 + i) - s);
        }
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = mfma_f64_16x16x4(Vs[i0 + c16][4 * r + g4], Mm[r], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + g4 + 4 * r;
          const double wv = (i < m) ? X[q][r] - 0.5 * acc[r] : 0.0;
          if (K == 1) Ws[i][c16] = wv;               // (the partials were read before the
          else stw(cw.Wg + i * BB + c16, wv);        // barriers above)
        }
      }
    }
    COOP_TMARK(4)
    cs.sync(false, &err_s);
    COOP_TMARK(3)
    // ---- D: W -> Ws (K = 1: already there); update (update workgroups) / look-ahead panel
    //      p+1 (QR workgroup)
    if (K > 1) {
      double v[BMP * BB / NTR];
#pragma unroll
      for (int u = 0; u < BMP * BB / NTR; ++u) v[u] = ldw(cw.Wg + min(t + NTR * u, nI * BB * BB - 1));
#pragma unroll
      for (int u = 0; u < BMP * BB / NTR; ++u) {
        const int e = t + NTR * u;
        if (e < nI * BB * BB) Ws[e / BB][e % BB] = v[u];
      }
    }
    __syncthreads();
    auto update = [&]() {
      // rows I = first_u + pos Ku (pos: snake over the waves), tiles J = (I ? 1 : 0) .. I,
      // TBR tiles per chunk, next chunk's tiles loaded before this chunk's MFMAs (the
      // one-workgroup kernel's trailing loop; stores through the buffer descriptor)
      const int first_u = ((wu - (p + 1)) % Ku + Ku) % Ku;
      // this workgroup's rows first_u + u Ku (u < nu) go to its waves by the LPT table of nu
      // rows (kUpdRows: K = 1 exactly; K > 1 the costs ceil((first_u + u Ku) / TBR) grow
      // linearly in u as the table's do).  A row >= nI ends the wave's list.
      constexpr int RR = UPD_RMAX;
      const int nu = (first_u < nI) ? (nI - first_u + Ku - 1) / Ku : 0;
      auto row_of = [&](int rr) {
        const int r = (rr < UPD_RMAX) ? (int)kUpdRows.r[nu][wid][rr] : -1;
        return r < 0 ? nI : first_u + r * Ku;
      };
      double4_t nxt[TBR];
      auto fetch = [&](int I, int J0) {
#pragma unroll
        for (int u = 0; u < TBR; ++u) {
          const int J = J0 + u;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * I + g4 + 4 * r, jj = 16 * J + c16;
            nxt[u][r] = A[(int64_t)(r0 + min(i, m - 1)) * lda + r0 + min(jj, m - 1)];
          }
        }
      };
      int rr = 0, I = row_of(0);
      while (rr < RR && I >= nI) I = row_of(++rr);
      if (rr >= RR) I = nI;
      int J0 = (I == 0) ? 0 : 1;
      auto advance = [&]() {
        J0 += TBR;
        if (J0 > I) {
          do I = row_of(++rr);
          while (rr < RR && I >= nI);
          if (rr >= RR) I = nI;
          J0 = (I == 0) ? 0 : 1;
        }
      };
      fetch(I, J0);
      double* tw = &red[0][0] + wid * (BB * BB);
      double4_t acc[TBR];
#pragma unroll
      for (int u = 0; u < TBR; ++u) acc[u] = nxt[u];
#pragma unroll
      for (int u = 0; u < TBR; ++u) asm volatile("" ::"v"(acc[u]));
      int ci = I, cj = J0;
      advance();
      while (ci < nI) {
        fetch(I, J0);
        double aV[4], aW[4], bW[TBR][4], bV[TBR][4];
        const int ia = 16 * ci + c16;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          aV[s] = -Vs[ia][4 * s + g4];
          aW[s] = -Ws[ia][4 * s + g4];
        }
#pragma unroll
        for (int u = 0; u < TBR; ++u) {
          const int jb = 16 * min(cj + u, ci) + c16;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            bW[u][s] = Ws[jb][4 * s + g4];
            bV[u][s] = Vs[jb][4 * s + g4];
          }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int u = 0; u < TBR; ++u) acc[u] = mfma_f64_16x16x4(aV[s], bW[u][s], acc[u]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int u = 0; u < TBR; ++u) acc[u] = mfma_f64_16x16x4(aW[s], bV[u][s], acc[u]);
#pragma unroll
        for (int u = 0; u < TBR; ++u) {
          const int J = cj + u;
          const bool live = J <= ci;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = g4 + 4 * r;
            tw[row * BB + (c16 ^ (row & ~1))] = acc[u][r];
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          {
            const int pr = lane >> 3, pc = 2 * (lane & 7);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int row = pr + 8 * h;
              const double2 v = *reinterpret_cast<const double2*>(&tw[row * BB + (pc ^ (row & ~1))]);
              st2((unsigned)(((r0 + 16 * ci + row) * lda + r0 + 16 * J + pc) * 8), live, v.x, v.y);
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
#pragma unroll
        for (int u = 0; u < TBR; ++u) asm volatile("" ::"v"(acc[u]));
#pragma unroll
        for (int u = 0; u < TBR; ++u) acc[u] = nxt[u];
        ci = I;
        cj = J0;
        advance();
      }
    };
    // the old tiles (I, 0) of the look-ahead panel, loaded before the update's stores are
    // issued (a load behind write-through stores waits for them: one vmcnt counter)
    double4_t pt[4];
    auto lookahead_load = [&]() {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int I = 1 + wid + NWR * q;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          pt[q][r] = A[(int64_t)(r0 + min(16 * min(I, nI - 1) + g4 + 4 * r, m - 1)) * lda + r0 + c16];
      }
    };
    auto lookahead = [&]() {
      // panel p+1 = tiles (I, 0), I >= 1, of A22 after update p (computed here, never stored
      // by the update), into Vs rows 16 (I - 1) .., then its QR (V_{p+1} -> Vs, T -> Ts)
      const int m1 = m - BB;
      double bW0[4], bV0[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bW0[s] = Ws[c16][4 * s + g4];
        bV0[s] = Vs[c16][4 * s + g4];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int I = 1 + wid + NWR * q;
        if (I < nI) {
          double aV[4], aW[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            aV[s] = -Vs[16 * I + c16][4 * s + g4];
            aW[s] = -Ws[16 * I + c16][4 * s + g4];
          }
#pragma unroll
          for (int s = 0; s < 4; ++s) pt[q] = mfma_f64_16x16x4(aV[s], bW0[s], pt[q]);
#pragma unroll
          for (int s = 0; s < 4; ++s) pt[q] = mfma_f64_16x16x4(aW[s], bV0[s], pt[q]);
        }
      }
      __syncthreads();                             // every V_p / W_p read is done
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int I = 1 + wid + NWR * q;
        if (I < nI) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * I + g4 + 4 * r;     // A22 row; panel row i - 16
            Vs[i - BB][c16] = (i < m) ? pt[q][r] : 0.0;
          }
        }
      }
      for (int e = t + 16 * (nI - 1) * BB; e < BMP * BB; e += NTR) Vs[e / BB][e % BB] = 0.0;
      __syncthreads();
      band_panel_hh(A, lda, k0 + BB, r0 + BB, m1, Vs, Ws, &red[0][0], Ts, taus,
                    bw.T + (int64_t)(p + 1) * BB * BB, nullptr, Vs);
      if (K > 1) publish_vt(m1);
    };
    if (K == 1) {
      if (p + 1 < npan) lookahead_load();
      update();
      COOP_TMARK(5)
      __syncthreads();
      COOP_TMARK(3)                                  // (timing: wave 0 waiting for the update)
      if (p + 1 < npan) lookahead();
      COOP_TMARK(6)
    } else if (qwg) {
      if (p + 1 < npan) {
        lookahead_load();
        lookahead();
      }
      COOP_TMARK(6)
    } else {
      update();
      COOP_TMARK(5)
    }
    cs.sync(true, &err_s);
    COOP_TMARK(7)
  }
  // ---- row-major lower band (the QR workgroup: it wrote the R blocks itself)
  if (qwg) {
    for (int e = t_; e < n * LS; e += NTR) {
      const int r = e / LS, c = r - BB + e % LS;
      bw.LB[e] = (c >= 0) ? A[(int64_t)r * lda + c] : 0.0;
    }
  }
  if constexpr (SOLO) {
    // z's rows >= 16, final since their panel's phase C, leave the LDS once (the solve reads bw.z)
    for (int g = BB + t_; g < n; g += NTR) stw(bw.z + g, Vs[g - BB][BB]);
  }
  if (TIMED) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the epilogue's stores are out)
    COOP_TMARK(7)
    if (threadIdx.x == 0 && w < 2)
      for (int q = 0; q < TIM_WG; ++q) tim[timing_cell_slot(cell, w) + q] = tacc[q];
  }
#undef COOP_TMARK
}

}  // namespace

// nwg workgroups (wgmap: cell << 8 | w << 4 | K - 1).  A general launch zeroes the cells' sync
// words on the stream first (a memset node under graph capture); the solo instance zeroes them
// itself (each cell's one workgroup, at entry), so a solo launch is the kernel alone.
hipError_t band_reduce_launch(const RidgeLaunchArgs& a, hipStream_t st) {
  if (a.wgmap == nullptr || a.syncw == nullptr || a.nwg <= 0) return hipErrorInvalidValue;
  // nwg == ncells: every cell has K = 1, the solo instance (no hand-offs, plain stores)
  const bool solo = a.solo && a.nwg == a.ncells;
  if (!solo) {
    const hipError_t e =
        hipMemsetAsync(a.syncw, 0, (size_t)a.ncells * COOP_SYNC * sizeof(unsigned), st);
    if (e != hipSuccess) return e;
  }
  const unsigned spin_max = a.spin_max ? a.spin_max : COOP_SPIN_MAX;
#define COOP_LAUNCH(TIMED, SOLO)                                                             \
  hipLaunchKernelGGL((band_coop_kernel<TIMED, SOLO>), dim3(a.nwg), dim3(NTR), 0, st, a.SD,   \
                     a.ldS, a.Sr, a.cells, a.L, a.work, a.wgmap, a.syncw, a.timing, spin_max)
  if (a.timing != nullptr) {
    if (solo) COOP_LAUNCH(true, true);
    else COOP_LAUNCH(true, false);
  } else {
    if (solo) COOP_LAUNCH(false, true);
    else COOP_LAUNCH(false, false);
  }
#undef COOP_LAUNCH
  return hipSuccess;
}

namespace {
// Panel-QR micro-benchmark (tools/bench_qr.py): every workgroup factors its own m x 16 panel
// (row-major in P) `reps` times with band_panel_hh, the band reduction's hot serial step, from
// an LDS image of the panel as the cooperative kernel holds it.  Cycles per factorisation
// (thread 0's s_memtime) -> cyc[block * 8 + ...]: total, load, column loop (incl. V stores),
// G + T, and the column loop's own work / barrier wait / pivot chain + update; V -> Vout,
// T -> Tout; R / V as band_panel_hh stores them land in A's columns 0..15, rows 16.. (lda =
// m + 16).
__global__ __launch_bounds__(NTR) void band_qr_bench_kernel(const double* __restrict__ P, int m,
                                                            int reps,
                                                            double* __restrict__ Aout,
                                                            double* __restrict__ Vout,
                                                            double* __restrict__ Tout,
                                                            long long* __restrict__ cyc) {
  __shared__ double Vs[BMP][LS];
  __shared__ double Gs[BB][LS];
  __shared__ double red[NWR][BB * BB];
  __shared__ double Ts[BB][LS];
  __shared__ double taus[BB];
  const int t = threadIdx.x;
  const int lda = m + BB;
  const double* Pb = P + (int64_t)blockIdx.x * m * BB;
  double* Ab = Aout + (int64_t)blockIdx.x * lda * lda;
  long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int rep = 0; rep < reps; ++rep) {
    for (int e = t; e < BMP * BB; e += NTR) {
      const int i = e / BB, c = e % BB;
      Vs[i][c] = (i < m) ? Pb[e] : 0.0;
    }
    __syncthreads();
    long long tk[6] = {0, 0, 0, 0, 0, 0};
    const long long t0 = (long long)__builtin_amdgcn_s_memtime();
    band_panel_hh(Ab, lda, 0, BB, m, Vs, Gs, &red[0][0], Ts, taus,
                  Tout + (int64_t)blockIdx.x * BB * BB, t == 0 ? tk : nullptr, Vs);
    __syncthreads();
    const long long t1 = (long long)__builtin_amdgcn_s_memtime();
    acc[0] += t1 - t0;
    acc[1] += tk[0] - t0;
    acc[2] += tk[1] - tk[0];
    acc[3] += t1 - tk[1];
    acc[4] += tk[2];
    acc[5] += tk[3];
    acc[6] += tk[4];
  }
  for (int e = t; e < m * BB; e += NTR) Vout[(int64_t)blockIdx.x * m * BB + e] = Vs[e / BB][e % BB];
  if (t == 0)
    for (int q = 0; q < 8; ++q) cyc[(int64_t)blockIdx.x * 8 + q] = acc[q] / (reps > 0 ? reps : 1);
}
}  // namespace

extern "C" hipError_t pfml_band_qr_bench(const double* P, int m, int nblocks, int reps,
                                         double* Aout, double* Vout, double* Tout,
                                         long long* cyc, hipStream_t st) {
  if (m < 1 || m > BMP) return hipErrorInvalidValue;
  hipLaunchKernelGGL(band_qr_bench_kernel, dim3(nblocks), dim3(NTR), 0, st, P, m, reps, Aout,
                     Vout, Tout, cyc);
  return hipGetLastError();
}
