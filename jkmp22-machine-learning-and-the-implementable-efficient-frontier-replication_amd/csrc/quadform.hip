// Out-of-sample validation utilities (PFML_hp_reals.py:81-102):
//
//     obj[job, l] = r_t^T beta_l - 1/2 beta_l^T D_t beta_l
//
// for every (g, year, p) cell, every one of its 12 validation months t and all 101 lambdas.
// The reference evaluates 513,888 of these quadratic forms one at a time from Python.  Here a
// job = (cell, month); the kernel computes the GEMM  U = D_t[:n,:n] * B  (B = [beta_l], n x L)
// on fp64 MFMA (upper block triangle only: D_t is symmetric) and folds the two reductions
// into the epilogue, so U never leaves registers.
//
// Tail index: n = p + 1 with p a multiple of 64 (65 .. 513), so the last index would cost a
// 16-wide K step of its own in every row tile and a 64-row tile of its own.  When n - 1 is a
// multiple of BK the tiles cover indices 0 .. n-2 only (K loop included); column n-1 enters
// each row's U in the epilogue (one rank-1 term) and row n-1's own term
// b_{n-1} (r_{n-1} - D_{n-1,n-1} b_{n-1} / 2) is added by the reduce kernel: 1 / 5 fewer
// tile-steps at n = 65, 2 / 15 at 129, 5 / 45 at 257, 9 / 153 at 513.
//
// Tile: 64 rows of D x 112 lambda columns (L <= 112) of one job per 256-thread workgroup (3
// per CU); each wave owns 16 rows x 7 MFMA 16x16 accumulators.  Every workgroup writes a
// deterministic per-row-tile partial; a second tiny kernel sums the partials in a fixed order
// (bitwise reproducible, no float atomics).  The host lists the tiles
// (tile_job[tile] = job << 5 | row tile, ops/ridge.py quad_plan) longest-first, and by
// default cuts them into runs - one cell's one row tile over consecutive validation months,
// levelled to about 64 K steps - which one workgroup of the pipelined kernel walks back to
// back (run_off; quad_pipe_body below).
//
// D_t is symmetric:  b'Db = sum_I b_I'(D_II b_I + 2 sum_{K>I} D_IK b_K).  A row tile I only
// walks K >= I, with the diagonal block weighted 1/2, so  acc = U_I / 2  and half the flops
// and D bytes of the full product are spent.
//
// Forms (ops/ridge.py quad_launch picks one per launch):
//  * quadform_pipe_kernel (default): the direct-A form below with a software-pipelined K
//    loop for aligned tiles (main index count a multiple of 64: every production cell) -
//    no branch, clamp or select around a load, counted vmcnt / lgkmcnt waits only, two B
//    fragment register sets, no vector ALU work beside the 28 MFMAs of a step, an
//    epilogue whose loads go out in two batches, and the pipeline kept full from one tile of
//    a run to the next (pfml_quadform_runs; pfml_quadform: every tile a run of its own).
//    Tiles that are not aligned go to quadform_rest_kernel, the direct form's loop, one per
//    workgroup in a second launch.
//  * quadform_direct_kernel (PFML_QUAD_DIRECT=1): the direct-A form for every tile.
// The pipelined and the direct form add the same products in the same order (the diagonal
// block's weight 1/2 is a power of two wherever it is applied), so barring underflow they
// agree bitwise (they do on the benchmark's grid).
#include "common.h"
#include <cstdlib>
#include <type_traits>

namespace {

constexpr int BK = 16, NCOL = 112, NTILE = NCOL / 16, BM = 64, NT = 256, NW = NT / 64;
// Earlier variants measured slower and removed: 128-row tiles (6.76 vs 6.64 ms per step), a
// prefetch distance of 2 (1.20 vs 1.33 ms), profiles/r02_quad_pf_ab.json, and the forms that
// staged D as well as beta in LDS, one or two validation months per tile (superseded by the
// direct-A form, profiles/r06_experiments.md; two months per tile 5.90 vs 5.78 ms per step).

// indices the tiles cover (n, or n - 1 when the tail index is split off, see above)
__host__ __device__ __forceinline__ int quad_main(int n) {
  return (n > 1 && (n - 1) % 16 == 0) ? n - 1 : n;
}

struct JobDesc {
  int64_t d_off;     // offset of D_t (P x P, ld ldD)
  int64_t r_off;     // offset of r_t
  int64_t b_off;     // offset of beta block [L][ldB]
  int64_t o_off;     // offset of this job's L utilities in obj
  int n;             // p + 1
  int ptile0;        // first partial slot of this job
};

// Direct-A form.  A wave's D rows are private to it (16 rows per wave, the tile's four waves
// disjoint), so D needs no LDS staging at all: every lane loads its own MFMA A fragments
// straight from global memory into registers, two K steps ahead (a ring of three 4-double
// fragment sets), and only the beta K-tile - shared by the four waves - goes through LDS.
// That takes the D tile's ds_writes, its masking pass and its place in the per-step vmcnt
// wait out of every step; the D stream (from HBM) has two steps to land.
//   k assignment within a 16-deep step: MFMA slice s takes k = k0 + 4c + s for lane group
//   c = lane >> 4, so lane (r, c) reads D[row r][k0 + 4c .. k0 + 4c + 3] - four consecutive
//   doubles of its row per step - and beta's LDS image is read at the same k.
//   beta image: row l (16 doubles = 32 banks), element k at l * 16 + (k ^ g(l)),
//   g(l) = (m & 3) | ((m & 4) << 1), m = (l >> 1) & 7: the fragment reads (16 rows x 2 lane
//   groups per half-wave) hit all 64 banks, the staging writes 2-way at most.
// The k summation order is fixed by this layout alone (the same bits on every rank count).
__device__ __forceinline__ int qd_swz(int l) {
  const int m = (l >> 1) & 7;
  return (m & 3) | ((m & 4) << 1);
}

typedef double double2_t __attribute__((ext_vector_type(2)));

// Aligned tiles: the main index count is a multiple of the 64-row tile (every production
// cell: 64, 128, 256, 512), so every row of every row tile and every k of every K step is in
// range, and the byte offsets into one D_t and one beta block fit 32 bits.
__host__ __device__ __forceinline__ bool quad_aligned(int nfull, int L, int64_t ldD,
                                                      int64_t ldB) {
  return quad_main(nfull) % BM == 0 && nfull <= ldB && nfull <= ldD &&
         (int64_t)nfull * ldD * 8 < (int64_t(1) << 31) &&
         (int64_t)L * ldB * 8 < (int64_t(1) << 31);
}

// The direct form's loop, one tile per workgroup, in two kernels.  QD_ALL: every tile.
// QD_REST: exactly the tiles the pipelined kernel leaves (launched after it, and only when
// the host's plan holds such a tile).  A tile's arithmetic depends on its own job alone, so
// results do not depend on what else the launch holds.
enum { QD_ALL = 0, QD_REST = 2 };

template <int MODE>
__device__ __forceinline__ void quad_direct_body(
    double (*Bs)[NCOL * BK], const double* __restrict__ D, int64_t ldD,
    const double* __restrict__ R, const double* __restrict__ Bt, int64_t ldB,
    const JobDesc* __restrict__ jobs, const int* __restrict__ tile_job, int L,
    double* __restrict__ partial) {
  static_assert(NW * NCOL <= 2 * NCOL * BK, "cross-wave sums must fit in the beta buffers");
  double (*red)[NCOL] = reinterpret_cast<double (*)[NCOL]>(&Bs[0][0]);

  const int tile = blockIdx.x;
  const int tj = tile_job[tile];
  const int jm = tj >> 5, rt = tj & 31;
  const JobDesc jd = jobs[jm];
  const int i0 = rt * BM;
  const int nfull = jd.n;
  const int n = quad_main(nfull);
  const bool tail = n != nfull;
  const double* Dm = D + jd.d_off;
  const double* rm = R + jd.r_off;
  const double* bt = Bt + jd.b_off;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r = lane & 15, c = lane >> 4;
  const int swz = qd_swz(r);                      // g(16 q + r) = g(r)

  double4_t acc[NTILE];
#pragma unroll
  for (int q = 0; q < NTILE; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};

  // this lane's D row (clamped: rows past n feed accumulator rows the epilogue drops)
  const double* drow = Dm + (int64_t)min(i0 + w * 16 + r, n - 1) * ldD;
  double da[3][4];                                 // A fragments of steps s, s + 1, s + 2
  auto dload = [&](int slot, int k0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) da[slot][u] = drow[min(k0 + 4 * c + u, n - 1)];
  };
  constexpr int BQ = (NCOL * BK) / NT;             // 7 beta elements per thread per step
  double rb[BQ];
  auto bload = [&](int k0) {
#pragma unroll
    for (int q = 0; q < BQ; ++q) {
      const int e = t + q * NT, l = e / BK, k = e % BK;
      rb[q] = bt[(int64_t)min(l, L - 1) * ldB + min(k0 + k, n - 1)];
    }
  };
  auto bstore = [&](int buf, int k0) {
#pragma unroll
    for (int q = 0; q < BQ; ++q) {
      const int e = t + q * NT, l = e / BK, k = e % BK;
      Bs[buf][l * BK + (k ^ qd_swz(l))] = (l < L && k0 + k < n) ? rb[q] : 0.0;
    }
  };

  const int nst = (n - i0 + BK - 1) / BK;          // K steps of this row tile
  if constexpr (MODE == QD_REST) {
    if (quad_aligned(nfull, L, ldD, ldB)) return;    // the pipelined kernel's
  }
  bload(i0);
  dload(0, i0);
  if (nst > 1) dload(1, i0 + BK);
  bstore(0, i0);
  __syncthreads();
  // one K step; SLOT = st % 3 as a compile-time constant (the fragment ring stays in
  // registers: the step loop below is unrolled by three)
  auto step = [&](auto slot_c, int st) -> bool {
    constexpr int cur = decltype(slot_c)::value;
    const int k0 = i0 + st * BK;
    const int buf = st & 1;
    const bool more = st + 1 < nst;
    // beta of the next step first, then D two steps ahead: the end-of-step wait for beta
    // leaves the D loads in flight (vmcnt counts in issue order)
    if (more) bload(k0 + BK);
    if (st + 2 < nst) dload((cur + 2) % 3, k0 + 2 * BK);
    // the diagonal block (k < i0 + 64) weighted 1/2: acc = U / 2 (D_t is symmetric, see top)
    const double wd = (k0 < i0 + BM) ? 0.5 : 1.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + 4 * c + s;
      const double a = (k < n) ? wd * da[cur][s] : 0.0;
#pragma unroll
      for (int q = 0; q < NTILE; ++q) {
        const double b = Bs[buf][(q * 16 + r) * BK + ((4 * c + s) ^ swz)];
        acc[q] = mfma_f64_16x16x4(a, b, acc[q]);
      }
    }
    if (!more) return false;
    bstore(buf ^ 1, k0 + BK);
    __syncthreads();
    return true;
  };
  for (int st = 0;; st += 3) {
    if (!step(std::integral_constant<int, 0>{}, st)) break;
    if (!step(std::integral_constant<int, 1>{}, st + 1)) break;
    if (!step(std::integral_constant<int, 2>{}, st + 2)) break;
  }
  __syncthreads();                                 // red reuses Bs

  if (tail) {
#pragma unroll
    for (int q = 0; q < NTILE; ++q) {
      const int l = min(q * 16 + (lane & 15), L - 1);
      const double bt_l = bt[(int64_t)l * ldB + n];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int gi = min(i0 + w * 16 + PFML_F64_CROW(lane, rr), n - 1);
        acc[q][rr] = fma(Dm[(int64_t)gi * ldD + n], bt_l, acc[q][rr]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NTILE; ++q) {
    const int l = q * 16 + (lane & 15);
    double s = 0.0;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int gi = i0 + w * 16 + PFML_F64_CROW(lane, rr);
      if (gi < n && l < L) s += bt[(int64_t)l * ldB + gi] * (rm[gi] - acc[q][rr]);
    }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (lane < 16) red[w][l] = s;
  }
  __syncthreads();
  if (t < L) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < NW; ++q) s += red[q][t];
    partial[(int64_t)(jd.ptile0 + rt) * L + t] = s;
  }
}

// Pipelined form for aligned tiles.  A workgroup walks a *run* of tiles back to back: entries
// tile_job[run_off[b] .. run_off[b + 1]) of the launch's tile list, which the host fills with
// one cell's one row tile over consecutive validation months (ops/ridge.py quad_plan), or,
// without a run table (run_off == nullptr), the single tile tile_job[b] - a run of one, and
// exactly the one-tile-per-workgroup kernel this replaced.  The months of a run share the beta
// block, the K range, the tile shape and the epilogue's beta rows; only D_t, r_t and the
// partial slot change.  So the row tile, n, the beta base and every loop-invariant offset are
// set up once per run, the next month's D base is fetched a month ahead, and the pipeline
// never drains at a month boundary: the last two steps of month t load the first two D
// fragments of month t + 1, the last step stages beta's first K tile again (it wraps), and
// r_t and the tail column of D_t are requested at the head of the month's last four steps.  A
// boundary then costs the epilogue alone (two batches of L2-resident beta loads, the sums,
// two barriers), not a descriptor fetch, a cold D / beta fetch and a ring fill.  Every month has
// an accumulator set and a partial slot of its own, with the products added in the order of
// the one-tile kernel: results are bitwise the same whatever the runs are.
//
// K loop (nst is a multiple of 4, >= 4).  No clamp, select or branch sits around a load: D
// and beta come through one buffer resource each, a loop-invariant 32-bit offset per element
// in a VGPR and the step's k offset in an SGPR.  The D ring has four slots so that slot and
// LDS buffer are compile-time constants of a loop unrolled by four; D is loaded two steps
// ahead, after the next step's beta, so the counted wait for beta at the end of a step leaves
// it in flight.  The last four steps of a month are peeled: they alone look past the month's
// end (after a run's last month they load the last K tile again and beta's first, for
// nobody).  The B fragments of a k-slice sit in one of two register sets: slice s + 1 is read
// from LDS while slice s's MFMAs issue.  The diagonal block's weight 1/2 is applied to the
// accumulators once, after the block's four steps (exact: a power of two).  Every step stages
// and syncs, the last one included: with the last step's staging under a branch the compiler
// sinks its beta loads into that branch and waits for them there in full.
__device__ __forceinline__ void quad_pipe_body(
    double (*Bs)[NCOL * BK], const double* __restrict__ D, int64_t ldD,
    const double* __restrict__ R, const double* __restrict__ Bt, int64_t ldB,
    const JobDesc* __restrict__ jobs, const int* __restrict__ tile_job,
    const int* __restrict__ run_off, int L, double* __restrict__ partial) {
  static_assert(NW * NCOL <= NCOL * BK, "cross-wave sums must fit in one beta buffer");
  // the sums go through buffer 1: at a month boundary buffer 0 already holds the next
  // month's first beta tile
  double (*red)[NCOL] = reinterpret_cast<double (*)[NCOL]>(&Bs[1][0]);

  int first = blockIdx.x, last = first + 1;
  if (run_off) {
    first = run_off[blockIdx.x];
    last = run_off[blockIdx.x + 1];
  }
  if (first >= last) return;
  const int tj = tile_job[first];
  const int rt = tj & 31;
  JobDesc jd = jobs[tj >> 5];
  const int i0 = rt * BM;
  const int nfull = jd.n;
  const int n = quad_main(nfull);
  const bool tail = n != nfull;
  if (!quad_aligned(nfull, L, ldD, ldB) || i0 >= n) return;   // quadform_rest_kernel's
  const double* bt = Bt + jd.b_off;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r = lane & 15, c = lane >> 4;
  const int swz = qd_swz(r);                      // g(16 q + r) = g(r)
  constexpr int BQ = (NCOL * BK) / NT;             // 7 beta elements per thread per step

  const int dbytes = (int)(((int64_t)(nfull - 1) * ldD + nfull) * 8);
  const int bbytes = (int)(((int64_t)(L - 1) * ldB + nfull) * 8);
  auto d_rsrc = [&](int64_t d_off) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(D + d_off), 0, dbytes,
                                             0x00020000);
  };
  __amdgpu_buffer_rsrc_t rsD = d_rsrc(jd.d_off);
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(bt), 0, bbytes, 0x00020000);
  const int dvo = ((i0 + w * 16 + r) * (int)ldD + 4 * c) * 8;
  int bvo[BQ];
#pragma unroll
  for (int q = 0; q < BQ; ++q) bvo[q] = (min((t >> 4) + 16 * q, L - 1) * (int)ldB + (t & 15)) * 8;
  // LDS element of this thread's staged beta (row t / 16 + 16 q: same swizzle for every
  // q) and of its fragment of slice s (row 16 q + r); both + 256 q
  const int bso = (t >> 4) * BK + ((t & 15) ^ qd_swz(t >> 4));
  int fro[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) fro[s] = r * BK + ((4 * c + s) ^ swz);
  constexpr int S = BK * 8;                        // bytes of a K step along a row
  const int klast = (n - BK) * 8;                  // byte offset of the last K tile
  double fa[4][4], fr[BQ];
  auto fdload = [&](__amdgpu_buffer_rsrc_t rs, int slot, int kb) {
    const double2_t lo = __builtin_bit_cast(
        double2_t, __builtin_amdgcn_raw_buffer_load_b128(rs, dvo, kb, 0));
    const double2_t hi = __builtin_bit_cast(
        double2_t, __builtin_amdgcn_raw_buffer_load_b128(rs, dvo + 16, kb, 0));
    fa[slot][0] = lo[0]; fa[slot][1] = lo[1]; fa[slot][2] = hi[0]; fa[slot][3] = hi[1];
  };
  auto fbload = [&](int kb) {
#pragma unroll
    for (int q = 0; q < BQ; ++q)
      fr[q] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsB, bvo[q], kb, 0));
  };
  auto fbstore = [&](int buf) {
#pragma unroll
    for (int q = 0; q < BQ; ++q) Bs[buf][q * 256 + bso] = fr[q];
  };
  double4_t acc[NTILE];
  // one K step on D slot `cur`: beta of the next step (byte offset kbn) first, then D two
  // steps ahead (resource rs, byte offset kdn), then whatever else the caller has to request
  auto fstep = [&](auto slot_c, int kbn, __amdgpu_buffer_rsrc_t rs, int kdn, auto&& also) {
    constexpr int cur = decltype(slot_c)::value;
    constexpr int buf = cur & 1;
    fbload(kbn);
    fdload(rs, (cur + 2) & 3, kdn);
    also();
    double fb[2][NTILE];
#pragma unroll
    for (int q = 0; q < NTILE; ++q) fb[0][q] = Bs[buf][q * 256 + fro[0]];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s < 3) {
#pragma unroll
        for (int q = 0; q < NTILE; ++q) fb[(s + 1) & 1][q] = Bs[buf][q * 256 + fro[s + 1]];
      }
#pragma unroll
      for (int q = 0; q < NTILE; ++q) acc[q] = mfma_f64_16x16x4(fa[cur][s], fb[s & 1][q], acc[q]);
    }
    fbstore(buf ^ 1);
    __syncthreads();
  };
  auto nothing = [] {};
  const std::integral_constant<int, 0> s0{};
  const std::integral_constant<int, 1> s1{};
  const std::integral_constant<int, 2> s2{};
  const std::integral_constant<int, 3> s3{};
  const int tn = (tail ? n : n - 1) * 8;           // in range either way; used if tail

  const int kb0 = i0 * 8, kend = n * 8;
  fbload(kb0);
  fdload(rsD, 0, kb0);
  fdload(rsD, 1, kb0 + S);
  fbstore(0);
  __syncthreads();
  for (int m = first;; ++m) {
    // the next month of the run: its D base, and where the last two steps look ahead to
    const bool more = m + 1 < last;
    JobDesc jn = jd;
    if (more) jn = jobs[tile_job[m + 1] >> 5];
    const __amdgpu_buffer_rsrc_t rsN = d_rsrc(jn.d_off);
    const int nk0 = more ? kb0 : klast, nk1 = more ? kb0 + S : klast;
    const double* rm = R + jd.r_off;
#pragma unroll
    for (int q = 0; q < NTILE; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
    // The epilogue's ~20 loop-invariant load offsets are rebuilt every month from these two
    // (opaque to the compiler here): hoisted out of the month loop they would sit in VGPRs
    // through every K loop and push the kernel past three waves per SIMD.
    int er_ = r, eg_ = i0 + w * 16 + PFML_F64_CROW(lane, 0);
    asm volatile("" : "+v"(er_), "+v"(eg_));
    auto grow = [&](int rr) { return eg_ + PFML_F64_CROW(0, rr); };
    int kb = kb0;
    for (; kb < kend - 4 * S; kb += 4 * S) {
      fstep(s0, kb + S, rsD, kb + 2 * S, nothing);
      fstep(s1, kb + 2 * S, rsD, kb + 3 * S, nothing);
      fstep(s2, kb + 3 * S, rsD, kb + 4 * S, nothing);
      fstep(s3, kb + 4 * S, rsD, kb + 5 * S, nothing);
      if (kb == kb0) {
#pragma unroll
        for (int q = 0; q < NTILE; ++q) acc[q] *= 0.5;
      }
    }
    // The month's last four steps.  Every row is in range here, so the epilogue's loads are
    // unconditional: r_i and D[i][n] (this month's own, from HBM) go out here, two steps
    // before the month's last wait for beta, and beta_l[i], beta_l[n] in one batch after
    // the last step (under `if (gi < n && l < L)` each of the 28 products waited for its own
    // loads: 28 memory round trips in a row, more than the whole K loop of a 4-step tile).
    double er[4], td[4];
    fstep(s0, kb + S, rsD, kb + 2 * S, [&] {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        er[rr] = rm[grow(rr)];
        td[rr] = __builtin_bit_cast(
            double, __builtin_amdgcn_raw_buffer_load_b64(rsD, grow(rr) * (int)ldD * 8, tn, 0));
      }
    });
    fstep(s1, kb + 2 * S, rsD, kb + 3 * S, nothing);
    fstep(s2, kb + 3 * S, rsN, nk0, nothing);
    fstep(s3, kb0, rsN, nk1, nothing);
    if (kb == kb0) {
#pragma unroll
      for (int q = 0; q < NTILE; ++q) acc[q] *= 0.5;
    }
    // Tail column and sums.  Columns l >= L compute on row L - 1's beta; nobody reads them.
    // Two batches (4 + 3 column tiles): with the next month's first D fragments live, all
    // 35 beta operands at once do not fit beside the accumulators in 168 VGPRs.
    auto sums = [&](auto q0_c, auto q1_c) {
      constexpr int q0 = decltype(q0_c)::value, q1 = decltype(q1_c)::value;
      double eb[q1 - q0][4], tb[q1 - q0];
#pragma unroll
      for (int q = q0; q < q1; ++q) {
        const int lo = min(q * 16 + er_, L - 1) * (int)ldB * 8;
        tb[q - q0] =
            __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsB, lo, tn, 0));
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          eb[q - q0][rr] = __builtin_bit_cast(
              double, __builtin_amdgcn_raw_buffer_load_b64(rsB, lo + grow(rr) * 8, 0, 0));
      }
#pragma unroll
      for (int q = q0; q < q1; ++q) {
        double s = 0.0;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const double u = tail ? fma(td[rr], tb[q - q0], acc[q][rr]) : acc[q][rr];
          s += eb[q - q0][rr] * (er[rr] - u);          // u = U / 2
        }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (lane < 16) red[w][q * 16 + r] = s;
      }
    };
    sums(std::integral_constant<int, 0>{}, std::integral_constant<int, 4>{});
    sums(std::integral_constant<int, 4>{}, std::integral_constant<int, NTILE>{});
    __syncthreads();
    if (t < L) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < NW; ++q) s += red[q][t];
      partial[(int64_t)(jd.ptile0 + rt) * L + t] = s;
    }
    if (!more) break;
    __syncthreads();                               // step 0 stages beta over the sums
    jd = jn;
    rsD = rsN;
  }
}

__global__ __launch_bounds__(NT, 3) void quadform_direct_kernel(
    const double* __restrict__ D, int64_t ldD, const double* __restrict__ R,
    const double* __restrict__ Bt, int64_t ldB, const JobDesc* __restrict__ jobs,
    const int* __restrict__ tile_job, int L, double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double Bs[2][NCOL * BK];
  quad_direct_body<QD_ALL>(Bs, D, ldD, R, Bt, ldB, jobs, tile_job, L, partial);
}

// (4 waves per SIMD - 128 VGPRs, the epilogue batch spilling 7 doubles - measured no faster:
// profiles/r07_experiments.md)
__global__ __launch_bounds__(NT, 3) void quadform_pipe_kernel(
    const double* __restrict__ D, int64_t ldD, const double* __restrict__ R,
    const double* __restrict__ Bt, int64_t ldB, const JobDesc* __restrict__ jobs,
    const int* __restrict__ tile_job, const int* __restrict__ run_off, int L,
    double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double Bs[2][NCOL * BK];
  quad_pipe_body(Bs, D, ldD, R, Bt, ldB, jobs, tile_job, run_off, L, partial);
}

__global__ __launch_bounds__(NT, 3) void quadform_rest_kernel(
    const double* __restrict__ D, int64_t ldD, const double* __restrict__ R,
    const double* __restrict__ Bt, int64_t ldB, const JobDesc* __restrict__ jobs,
    const int* __restrict__ tile_job, int L, double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double Bs[2][NCOL * BK];
  quad_direct_body<QD_REST>(Bs, D, ldD, R, Bt, ldB, jobs, tile_job, L, partial);
}

__global__ void quadform_reduce_kernel(const double* __restrict__ partial,
                                       const JobDesc* __restrict__ jobs, int njobs, int L,
                                       const double* __restrict__ D, int64_t ldD,
                                       const double* __restrict__ R,
                                       const double* __restrict__ Bt, int64_t ldB,
                                       double* __restrict__ obj) {
  const int j = blockIdx.x;
  const int l = threadIdx.x;
  if (j >= njobs || l >= L) return;
  const JobDesc jd = jobs[j];
  const int n = quad_main(jd.n);
  const int nt = (n + BM - 1) / BM;
  double s = 0.0;
  for (int q = 0; q < nt; ++q) s += partial[(int64_t)(jd.ptile0 + q) * L + l];
  if (n != jd.n) {                              // the tail row's own term
    const double b = Bt[jd.b_off + (int64_t)l * ldB + n];
    s += b * (R[jd.r_off + n] - 0.5 * D[jd.d_off + (int64_t)n * ldD + n] * b);
  }
  obj[jd.o_off + l] = s;
}

}  // namespace

extern "C" int pfml_quadform_job_desc_size() { return (int)sizeof(JobDesc); }
extern "C" int pfml_quadform_rows_per_tile() { return BM; }
extern "C" int pfml_quadform_row_tiles(int n) { return (quad_main(n) + BM - 1) / BM; }
// whether the tiles of a job of n indices take the pipelined loop (the kernels' own test)
extern "C" int pfml_quadform_aligned(int n, int L, int64_t ldD, int64_t ldB) {
  return quad_aligned(n, L, ldD, ldB) ? 1 : 0;
}

// tile_job: one int32 per tile, job << 5 | row tile.  form: 3 = the direct-A form for every
// tile; 4 = the pipelined form, every job of the launch aligned (pfml_quadform_aligned); 5 =
// the pipelined form for the aligned jobs and the direct form's loop for the rest.  run_off:
// nullptr (every tile a workgroup of its own, nruns = ntiles), or nruns + 1 ascending offsets
// into tile_job, run_off[0] = 0 and run_off[nruns] = ntiles: the pipelined kernel's
// workgroup b walks tiles run_off[b] .. run_off[b + 1] - 1, which must be the same row tile
// of jobs with the same n and beta block (forms 4 and 5 only; the direct form's loop takes
// one tile per workgroup whatever the runs are).
static hipError_t quadform_launch(const double* D, int64_t ldD, const double* R,
                                  const double* Bt, int64_t ldB, const void* jobs, int njobs,
                                  const int* tile_job, int ntiles, const int* run_off,
                                  int nruns, int form, int L, double* partial, double* obj,
                                  hipStream_t st) {
  if (njobs <= 0) return hipSuccess;
  if (L > NCOL || form < 3 || form > 5) return hipErrorInvalidValue;
  if (run_off && (form < 4 || nruns <= 0 || nruns > ntiles)) return hipErrorInvalidValue;
  const JobDesc* jd = static_cast<const JobDesc*>(jobs);
  if (form >= 4) {
    hipLaunchKernelGGL(quadform_pipe_kernel, dim3(run_off ? nruns : ntiles), dim3(NT), 0, st, D,
                       ldD, R, Bt, ldB, jd, tile_job, run_off, L, partial);
    if (form == 5)
      hipLaunchKernelGGL(quadform_rest_kernel, dim3(ntiles), dim3(NT), 0, st, D, ldD, R, Bt,
                         ldB, jd, tile_job, L, partial);
  } else
    hipLaunchKernelGGL(quadform_direct_kernel, dim3(ntiles), dim3(NT), 0, st, D, ldD, R, Bt, ldB,
                       jd, tile_job, L, partial);
  hipLaunchKernelGGL(quadform_reduce_kernel, dim3(njobs), dim3(128), 0, st, partial, jd, njobs, L,
                     D, ldD, R, Bt, ldB, obj);
  return hipGetLastError();
}

// One tile per workgroup.  The `form` argument keeps the position and the values it had when
// 1 / 2 meant the retired LDS-staged forms (months per tile), so a library built before their
// removal still loads under PFML_HIP_LIB for an A/B against this one; 1 / 2 are refused here.
extern "C" hipError_t pfml_quadform(const double* D, int64_t ldD, const double* R,
                                    const double* Bt, int64_t ldB, const void* jobs, int njobs,
                                    const int* tile_job, int ntiles, int form, int L,
                                    double* partial, double* obj, hipStream_t st) {
  return quadform_launch(D, ldD, R, Bt, ldB, jobs, njobs, tile_job, ntiles, nullptr, ntiles,
                         form, L, partial, obj, st);
}

// The pipelined form over runs of tiles (form 4 or 5, run_off as above).
extern "C" hipError_t pfml_quadform_runs(const double* D, int64_t ldD, const double* R,
                                         const double* Bt, int64_t ldB, const void* jobs,
                                         int njobs, const int* tile_job, int ntiles,
                                         const int* run_off, int nruns, int form, int L,
                                         double* partial, double* obj, hipStream_t st) {
  if (!run_off) return hipErrorInvalidValue;
  return quadform_launch(D, ldD, R, Bt, ldB, jobs, njobs, tile_job, ntiles, run_off, nruns,
                         form, L, partial, obj, st);
}
