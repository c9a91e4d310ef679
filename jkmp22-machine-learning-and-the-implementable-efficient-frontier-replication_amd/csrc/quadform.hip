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
// (bitwise reproducible, no float atomics).  The host lists the tiles longest-first
// (tile_job[tile] = job << 5 | row tile, ops/ridge.py quad_plan).
//
// D_t is symmetric:  b'Db = sum_I b_I'(D_II b_I + 2 sum_{K>I} D_IK b_K).  A row tile I only
// walks K >= I, with the diagonal block weighted 1/2, so  acc = U_I / 2  and half the flops
// and D bytes of the full product are spent.
//
// Forms (ops/ridge.py quad_launch picks one per launch):
//  * quadform_pipe_kernel (default): the direct-A form below with a software-pipelined K
//    loop for aligned tiles (main index count a multiple of 64: every production cell) -
//    no branch, clamp or select around a load, counted vmcnt / lgkmcnt waits only, two B
//    fragment register sets, no vector ALU work beside the 28 MFMAs of a step, and an
//    epilogue whose loads go out in one batch.  Tiles that are not aligned go to
//    quadform_rest_kernel, the direct form's loop, in a second launch.
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

// One body, three kernels.  QD_ALL: the direct form's loop for every tile.  QD_PIPE: the
// pipelined loop for the aligned tiles of the launch, any other tile is left alone.
// QD_REST: the direct form's loop for exactly the tiles QD_PIPE leaves (launched after it,
// and only when the host's plan holds such a tile).  A tile's arithmetic depends on its own
// job alone, so results do not depend on what else the launch holds.
enum { QD_ALL = 0, QD_PIPE = 1, QD_REST = 2 };

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
  if constexpr (MODE != QD_ALL) {
    if (quad_aligned(nfull, L, ldD, ldB) != (MODE == QD_PIPE)) return;   // not this kernel's
  }
  if constexpr (MODE == QD_PIPE) {
    // Pipelined loop (nst is a multiple of 4, >= 4).  No clamp, select or branch sits around
    // a load: D and beta come through one buffer resource each, a loop-invariant 32-bit
    // offset per element in a VGPR and the step's k offset in an SGPR, clamped to the last
    // K tile - the two steps past the end load that tile again and nobody reads it.  The
    // D ring has four slots so that slot and LDS buffer are compile-time constants of a
    // loop unrolled by four; D is loaded two steps ahead, after the next step's beta, so
    // the counted wait for beta at the end of a step leaves it in flight.  The B fragments
    // of a k-slice sit in one of two register sets: slice s + 1 is read from LDS while
    // slice s's MFMAs issue.  The diagonal block's weight 1/2 is applied to the accumulators
    // once, after the block's four steps (exact: a power of two).
    const int dbytes = (int)(((int64_t)(nfull - 1) * ldD + nfull) * 8);
    const int bbytes = (int)(((int64_t)(L - 1) * ldB + nfull) * 8);
    const __amdgpu_buffer_rsrc_t rsD =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(Dm), 0, dbytes, 0x00020000);
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
    const int klast = (n - BK) * 8;                // byte offset of the last K tile
    double fa[4][4], fr[BQ];
    auto fdload = [&](int slot, int kb) {
      const double2_t lo = __builtin_bit_cast(
          double2_t, __builtin_amdgcn_raw_buffer_load_b128(rsD, dvo, kb, 0));
      const double2_t hi = __builtin_bit_cast(
          double2_t, __builtin_amdgcn_raw_buffer_load_b128(rsD, dvo + 16, kb, 0));
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
    auto fstep = [&](auto slot_c, int kb) {
      constexpr int cur = decltype(slot_c)::value;
      constexpr int buf = cur & 1;
      fbload(min(kb + BK * 8, klast));
      fdload((cur + 2) & 3, min(kb + 2 * BK * 8, klast));
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
    const int kb0 = i0 * 8, kend = n * 8;
    fbload(kb0);
    fdload(0, kb0);
    fdload(1, kb0 + BK * 8);
    fbstore(0);
    __syncthreads();
    // every step stages and syncs, the last one included (it stages the clamped tile for
    // nobody): with the last step's staging under a branch the compiler sinks its beta loads
    // into that branch and waits for them there in full, once per four steps
    for (int kb = kb0; kb < kend; kb += 4 * BK * 8) {
      fstep(std::integral_constant<int, 0>{}, kb);
      fstep(std::integral_constant<int, 1>{}, kb + BK * 8);
      fstep(std::integral_constant<int, 2>{}, kb + 2 * BK * 8);
      fstep(std::integral_constant<int, 3>{}, kb + 3 * BK * 8);
      if (kb == kb0) {
#pragma unroll
        for (int q = 0; q < NTILE; ++q) acc[q] *= 0.5;
      }
    }
    __syncthreads();                               // red reuses Bs
    // Tail column and epilogue as below, but every row is in range here, so all their
    // loads (r_i, beta_l[i], beta_l[n], D[i][n]) are issued unconditionally in one batch
    // (under `if (gi < n && l < L)` each of the 28 products waited for its own loads: 28
    // memory round trips in a row, more than the whole K loop of a 4-step tile).  Columns
    // l >= L compute on row L - 1's beta; nobody reads their sums.
    auto grow = [&](int rr) { return i0 + w * 16 + PFML_F64_CROW(lane, rr); };
    const int tn = (tail ? n : n - 1) * 8;         // in range either way; used if tail
    double er[4], td[4], eb[NTILE][4], tb[NTILE];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      er[rr] = rm[grow(rr)];
      td[rr] = __builtin_bit_cast(
          double, __builtin_amdgcn_raw_buffer_load_b64(rsD, grow(rr) * (int)ldD * 8, tn, 0));
    }
#pragma unroll
    for (int q = 0; q < NTILE; ++q) {
      const int lo = min(q * 16 + r, L - 1) * (int)ldB * 8;
      tb[q] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsB, lo, tn, 0));
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        eb[q][rr] = __builtin_bit_cast(
            double, __builtin_amdgcn_raw_buffer_load_b64(rsB, lo + grow(rr) * 8, 0, 0));
    }
#pragma unroll
    for (int q = 0; q < NTILE; ++q) {
      double s = 0.0;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const double u = tail ? fma(td[rr], tb[q], acc[q][rr]) : acc[q][rr];
        s += eb[q][rr] * (er[rr] - u);               // u = U / 2
      }
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lane < 16) red[w][q * 16 + r] = s;
    }
  } else {
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
  }
  __syncthreads();
  if (t < L) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < NW; ++q) s += red[q][t];
    partial[(int64_t)(jd.ptile0 + rt) * L + t] = s;
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
    const int* __restrict__ tile_job, int L, double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double Bs[2][NCOL * BK];
  quad_direct_body<QD_PIPE>(Bs, D, ldD, R, Bt, ldB, jobs, tile_job, L, partial);
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
// the pipelined form for the aligned jobs and the direct form's loop for the rest.  The
// argument keeps the position and the values it had when 1 / 2 meant the retired LDS-staged
// forms (months per tile), so a library built before their removal still loads under
// PFML_HIP_LIB for an A/B against this one; 1 / 2 are refused here.
extern "C" hipError_t pfml_quadform(const double* D, int64_t ldD, const double* R,
                                    const double* Bt, int64_t ldB, const void* jobs, int njobs,
                                    const int* tile_job, int ntiles, int form, int L,
                                    double* partial, double* obj, hipStream_t st) {
  if (njobs <= 0) return hipSuccess;
  if (L > NCOL || form < 3 || form > 5) return hipErrorInvalidValue;
  const JobDesc* jd = static_cast<const JobDesc*>(jobs);
  if (form >= 4) {
    hipLaunchKernelGGL(quadform_pipe_kernel, dim3(ntiles), dim3(NT), 0, st, D, ldD, R, Bt, ldB,
                       jd, tile_job, L, partial);
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
