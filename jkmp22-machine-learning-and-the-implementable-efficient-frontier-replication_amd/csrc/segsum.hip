// Expanding-window sums of the grid search over the month axis.
//
// The reference keeps running sums of r_tilde and denom, adding each hyper-parameter year's
// 12 new months (PFML_Search_Coef.py:68-121).  The engine sums the resident [G, T, P, P] /
// [G, T, P] month stacks per window segment (burn-in pieces, then one block per hp year) and
// folds the segments in ONE canonical chunked association (below), so every world size adds
// the same numbers in the same order.  A rank of a multi-rank run forms its windows with two
// kernels around an all-gather of chunk totals (pfml_wsum_chunk_totals, pfml_wsum_chunk_prefix,
// pfml_wvec_chunk); a one-rank run takes pfml_wsum_onepass, ONE launch that reads every
// month's upper triangle once and writes the mirrored windows once, bitwise the same.
#include "common.h"

namespace {

// Segment s's sums live in out[g][s - skip] for s >= skip and in scratch[g][s] for the
// leading `skip` segments (the burn-in pieces, needed only as a prefix): the output is the
// contiguous [G][nseg - skip] stack the ridge grid consumes, with no slicing copy.
__device__ __forceinline__ double* seg_slot(double* out, double* scratch, int g, int s, int nseg,
                                            int skip, int64_t PP) {
  return s < skip ? scratch + ((int64_t)g * skip + s) * PP
                  : out + ((int64_t)g * (nseg - skip) + (s - skip)) * PP;
}

// Segment sums of the symmetric month matrices X [G, T, P, P] into their seg_slot: the UPPER
// triangle only (half the bytes of a dense pass), one workgroup per (row, segment, g) for
// full-chip parallelism.  The chunk kernels below fold and mirror them.
__global__ __launch_bounds__(256) void wsum_upper_kernel(const double* __restrict__ X, int P,
                                                         int T, const int* __restrict__ seg_start,
                                                         const int* __restrict__ seg_stop,
                                                         int nseg, int skip,
                                                         double* __restrict__ out,
                                                         double* __restrict__ scratch) {
  const int i = blockIdx.x, s = blockIdx.y, g = blockIdx.z;
  const int a = seg_start[s], b = seg_stop[s];
  const int64_t PP = (int64_t)P * P;
  const double* src = X + (int64_t)g * T * PP + (int64_t)i * P;
  double* dst = seg_slot(out, scratch, g, s, nseg, skip, PP) + (int64_t)i * P;
  for (int j = i + threadIdx.x; j < P; j += 256) {
    // four independent chains: four month loads in flight per lane
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int tm = a;
    for (; tm + 4 <= b; tm += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] += src[(int64_t)(tm + u) * PP + j];
    }
    for (; tm < b; ++tm) acc[0] += src[(int64_t)tm * PP + j];
    dst[j] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  }
}

// Segment sums of the month VECTORS (r_tilde): a workgroup of RG row groups x COLS columns
// holds every segment's sums of its columns in LDS (at most WV_SEG segments).  Row group ry
// fills part[s][lc] for s = ry, ry + RG, ...: eight independent chains (eight months in
// flight per lane, the months past the segment's end masked to +0.0), folded pairwise.  src
// points at the thread's column of month 0 and E is the month pitch.  The ONE copy of this
// loop: the two-kernel path and the one-pass kernel are bitwise alike because both call it.
constexpr int WV_COLS = 64, WV_SEG = 128, WV_T = 1024, WV_RG = WV_T / WV_COLS;
template <int COLS, int RG>
__device__ __forceinline__ void wvec_segsums(const double* src, int64_t E, const int* seg_start,
                                             const int* seg_stop, int nseg, int ry, int lc,
                                             double (*part)[COLS]) {
  for (int s = ry; s < nseg; s += RG) {
    const int a = seg_start[s], b = seg_stop[s];
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int tm = a; tm < b; tm += 8) {          // eight months in flight
      double x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = (tm + u < b) ? src[(int64_t)(tm + u) * E] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += x[u];
    }
    part[s][lc] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------
// Canonical chunked expanding-window sums (bitwise the same on every world size).
//
// A running sum over the segments of ONE rank re-associates differently for every sharding
// (world 1: ((S0 + S1) + S2) + ..., world N: (S_k + ...) + prefix of the lower ranks), so
// the utilities of an N-rank run differed from the 1-rank run in the last bits (2e-10 rel.)
// and a near-tie rank could flip.  The sums therefore follow ONE fixed association,
// independent of the world size:
//   * the months are cut into 2C canonical chunks: C burn-in pieces and C groups of whole
//     hp-year blocks (search.win_layout; C = 8 covers world 1, 2, 4, 8);
//   * chunk total T = left fold of its segment sums from 0 (kernel A, on the chunk's owner);
//   * E = left fold of the C burn-in totals, P_0 = E, P_{c+1} = P_c + TY_c;
//   * the window of a year in chunk c = left fold of c's year segments starting from P_c
//     (kernel B).
// Ranks own whole chunks; the totals cross ranks by one all-gather (P x P per owned chunk)
// and kernel B reads them through a canonical slot map, so no reordering copy.  Totals are
// chunk-major: slot k, g at tot + k * tstride + g * (P P or E).
namespace {

__device__ __forceinline__ bool tile_upper(int I, int J, int i, int j, int r, int c, int P) {
  return i < P && j < P && (I != J || c >= r);
}

// tot slot[lc] (upper triangle) = left fold of segments [cs[lc], ce[lc]) from 0; one
// workgroup per (tile, g, chunk): the chunks are independent, so the launch has nlc times
// the workgroups of a per-tile loop over them (that form was latency-bound: 306 workgroups
// walking 61 segment tiles one after another, 127 us for 128 MB).  Same per-element order.
__global__ __launch_bounds__(256) void wsum_chunk_totals_kernel(
    int P, int nseg, int skip, const double* __restrict__ out, const double* __restrict__ scratch,
    int nlc, const int* __restrict__ cs, const int* __restrict__ ce, const int* __restrict__ slot,
    double* __restrict__ tot, int64_t tstride) {
  const int g = blockIdx.y, lc = blockIdx.z;
  int tile = blockIdx.x;
  const int nt = (P + 31) / 32;
  int I = 0;
  while (tile >= nt - I) { tile -= nt - I; ++I; }
  const int J = I + tile;
  const int64_t PP = (int64_t)P * P;
  const int t = threadIdx.x, c = t & 31, r0 = t >> 5;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const int s0 = cs[lc], s1 = ce[lc];
  // all of a segment's loads in flight before the adds; the next segment's issued first
  double nx[4];
  auto fetch = [&](int s) {
    const double* o = seg_slot(const_cast<double*>(out), const_cast<double*>(scratch), g, s,
                               nseg, skip, PP);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = min(I * 32 + r0 + 8 * q, P - 1), j = min(J * 32 + c, P - 1);
      nx[q] = o[(int64_t)i * P + j];
    }
  };
  if (s0 < s1) fetch(s0);
  for (int s = s0; s < s1; ++s) {
    double cur[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) cur[q] = nx[q];
    if (s + 1 < s1) fetch(s + 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = r0 + 8 * q, i = I * 32 + r, j = J * 32 + c;
      if (tile_upper(I, J, i, j, r, c, P)) acc[q] += cur[q];
    }
  }
  double* d = tot + (int64_t)slot[lc] * tstride + (int64_t)g * PP;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = r0 + 8 * q, i = I * 32 + r, j = J * 32 + c;
    if (tile_upper(I, J, i, j, r, c, P)) d[(int64_t)i * P + j] = acc[q];
  }
}

// windows: E = fold(tot[sb[k]]), P_0 = E; chunk c with local year segments [ys[c], ye[c]):
// acc = P_c, acc += seg s, out[s - skip] = acc (full, mirrored); P_{c+1} = P_c + tot[sy[c]].
// One workgroup per (tile, g, chunk ch <= clast): it forms P_ch itself by the same left fold
// (E, then + tot[sy[0]], ..., + tot[sy[ch - 1]]), so every chunk's windows run in parallel
// and the bits are those of the sequential walk.
__global__ __launch_bounds__(256) void wsum_chunk_prefix_kernel(
    int P, int nseg, int skip, double* __restrict__ out, double* __restrict__ scratch, int C,
    const int* __restrict__ sb, const int* __restrict__ sy, const int* __restrict__ ys,
    const int* __restrict__ ye, const double* __restrict__ tot, int64_t tstride, int clast) {
  __shared__ double Ts[32][33];
  const int g = blockIdx.y, ch = blockIdx.z;
  const int s0 = ys[ch], s1 = ye[ch];
  if (s0 >= s1) return;                         // no local windows in this chunk
  int tile = blockIdx.x;
  const int nt = (P + 31) / 32;
  int I = 0;
  while (tile >= nt - I) { tile -= nt - I; ++I; }
  const int J = I + tile;
  const int64_t PP = (int64_t)P * P;
  const int t = threadIdx.x, c = t & 31, r0 = t >> 5;
  const double* tg = tot + (int64_t)g * PP;     // slot k at tg + k * tstride
  // the first segment's tile is in flight during the prefix, each next one while the current
  // is added and written (clamped loads, masked on use; the same adds in the same order)
  double nx[4];
  auto fetch = [&](int s) {
    const double* o = seg_slot(out, scratch, g, s, nseg, skip, PP);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = min(I * 32 + r0 + 8 * q, P - 1), j = min(J * 32 + c, P - 1);
      nx[q] = o[(int64_t)i * P + j];
    }
  };
  fetch(s0);
  // the C + ch prefix tiles, loaded together, then added in the canonical order
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const int nk = C + ch;
  for (int k0 = 0; k0 < nk; k0 += 8) {
    double v[8][4];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = min(k0 + u, nk - 1);
      const double* o = tg + (int64_t)(k < C ? sb[k] : sy[k - C]) * tstride;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = min(I * 32 + r0 + 8 * q, P - 1), j = min(J * 32 + c, P - 1);
        v[u][q] = o[(int64_t)i * P + j];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (k0 + u < nk) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = r0 + 8 * q, i = I * 32 + r, j = J * 32 + c;
          if (tile_upper(I, J, i, j, r, c, P)) acc[q] += v[u][q];
        }
      }
    }
  }
  for (int s = s0; s < s1; ++s) {
    double cur[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) cur[q] = nx[q];
    if (s + 1 < s1) fetch(s + 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = r0 + 8 * q, i = I * 32 + r, j = J * 32 + c;
      const double v = tile_upper(I, J, i, j, r, c, P) ? cur[q] : 0.0;
      acc[q] += v;
      Ts[r][c] = acc[q];
    }
    __syncthreads();
    if (s >= skip) {
      double* w = seg_slot(out, scratch, g, s, nseg, skip, PP);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + 8 * q;
        const int i = I * 32 + r, j = J * 32 + c;
        if (i < P && j < P) w[(int64_t)i * P + j] = (I != J || c >= r) ? Ts[r][c] : Ts[c][r];
        const int i2 = J * 32 + r, j2 = I * 32 + c;
        if (I != J && i2 < P && j2 < P) w[(int64_t)i2 * P + j2] = Ts[c][r];
      }
    }
    __syncthreads();
  }
}

// vectors (r_tilde): mode 0 = chunk totals into tot[g][slot[lc]][E], mode 1 = windows into
// out[g][s - skip][E].  Workgroup (64 columns, g): its 16 row groups sum the segments into LDS
// (wvec_segsums), then one row group runs the folds in canonical order.
__global__ __launch_bounds__(WV_T) void wvec_chunk_kernel(
    const double* __restrict__ X, int64_t E, int T, const int* __restrict__ seg_start,
    const int* __restrict__ seg_stop, int nseg, int skip, int mode, int nlc,
    const int* __restrict__ cs, const int* __restrict__ ce, const int* __restrict__ slot, int C,
    const int* __restrict__ sb, const int* __restrict__ sy, const int* __restrict__ ys,
    const int* __restrict__ ye, int clast, double* __restrict__ tot, int64_t tstride,
    double* __restrict__ out) {
  __shared__ double part[WV_SEG][WV_COLS];
  const int lc = threadIdx.x % WV_COLS, ry = threadIdx.x / WV_COLS;
  const int g = blockIdx.y, col = blockIdx.x * WV_COLS + lc;
  const bool cv = col < E;
  const double* src = X + (int64_t)g * T * E + (cv ? col : 0);
  wvec_segsums<WV_COLS, WV_RG>(src, E, seg_start, seg_stop, nseg, ry, lc, part);
  __syncthreads();
  if (ry != 0 || !cv) return;
  double* tg = tot + (int64_t)g * E + col;     // slot k at tg + k * tstride
  if (mode == 0) {
    for (int k = 0; k < nlc; ++k) {
      double acc = 0.0;
      for (int s = cs[k]; s < ce[k]; ++s) acc += part[s][lc];
      tg[(int64_t)slot[k] * tstride] = acc;
    }
    return;
  }
  double pc = 0.0;
  for (int k = 0; k < C; ++k) pc += tg[(int64_t)sb[k] * tstride];
  double* o = out + (int64_t)g * (nseg - skip) * E + col;
  for (int ch = 0; ch <= clast; ++ch) {
    double acc = pc;
    for (int s = ys[ch]; s < ye[ch]; ++s) {
      acc += part[s][lc];
      if (s >= skip) o[(int64_t)(s - skip) * E] = acc;
    }
    if (ch < clast) pc += tg[(int64_t)sy[ch] * tstride];
  }
}

}  // namespace

// Kernel A for the matrices: segment sums (upper triangles) into the out / scratch slots,
// then the local chunk totals.  idx = [cs, ce, slot] (3 x nlc int32, device).
extern "C" hipError_t pfml_wsum_chunk_totals(const double* X, int P, int T, int G,
                                             const int* seg_start, const int* seg_stop, int nseg,
                                             int skip, double* out, double* scratch, int nlc,
                                             const int* idx, double* tot, int64_t tstride,
                                             hipStream_t st) {
  if (nseg <= 0 || P <= 0 || G <= 0) return hipSuccess;
  if (skip < 0 || skip > nseg || (skip > 0 && scratch == nullptr)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wsum_upper_kernel, dim3(P, nseg, G), dim3(256), 0, st, X, P, T, seg_start,
                     seg_stop, nseg, skip, out, scratch);
  if (nlc > 0) {
    const int nt = (P + 31) / 32;
    hipLaunchKernelGGL(wsum_chunk_totals_kernel, dim3(nt * (nt + 1) / 2, G, nlc), dim3(256), 0, st, P,
                       nseg, skip, out, scratch, nlc, idx, idx + nlc, idx + 2 * nlc, tot,
                       tstride);
  }
  return hipGetLastError();
}

// Kernel B for the matrices.  cidx = [sb, sy, ys, ye] (4 x C int32, device).
extern "C" hipError_t pfml_wsum_chunk_prefix(int P, int G, int nseg, int skip, double* out,
                                             double* scratch, int C, const int* cidx,
                                             const double* tot, int64_t tstride, int clast,
                                             hipStream_t st) {
  if (nseg <= 0 || P <= 0 || G <= 0 || clast < 0) return hipSuccess;
  const int nt = (P + 31) / 32;
  hipLaunchKernelGGL(wsum_chunk_prefix_kernel, dim3(nt * (nt + 1) / 2, G, clast + 1), dim3(256), 0, st, P,
                     nseg, skip, out, scratch, C, cidx, cidx + C, cidx + 2 * C, cidx + 3 * C, tot,
                     tstride, clast);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// One-pass form of the canonical chunked window sums for a rank that owns EVERY chunk (world
// size one): one launch reads each month's upper triangle once and writes the windows once.
// No segment sum, chunk total or prefix goes through memory; every element still follows the
// association of the kernels above exactly (wsum_upper_kernel's four chains per segment,
// chunk totals folded from 0, E, P_c and the windows as wsum_chunk_prefix_kernel; the vectors
// as wvec_chunk_kernel), so the bits are those of the two-kernel path.
//
// A rank that owns every chunk holds the segments of a chunk side by side and the year
// chunks' totals fold exactly the segments their windows walk (cs[sy[c]] == ys[c], ce[sy[c]]
// == ye[c], slot[k] == k: checked by the caller), so one thread can walk its elements' months
// in canonical order with three running values per element: the prefix P_c, the chunk total
// and the window.
//
// Workgroup (OP_T threads) = one OP_R x OP_C tile of the upper triangle of one g: a thread
// owns two neighbouring columns of one row (one 16-byte load per month, 8-byte aligned: the
// row pitch and the month pitch are odd multiples of 8 bytes when P is odd), a half wave
// reads OP_C * 8 contiguous bytes of a row, and twelve months are in flight per lane, loaded
// one batch ahead of the adds.  Tiles off the diagonal and off the ragged last column take
// the unmasked path; the others load element by element and only entries with j >= i.  A
// window's tile is written straight from the registers and, through LDS, transposed as rows
// of OP_R doubles (two LDS buffers: one barrier per window).  8 x 64 tiles: every workgroup
// is resident at once, three per CU at P = 513 (16 x 64 tiles with 512 threads left the CUs
// one or two workgroups each and the kernel waiting for the CUs with two).  The first
// ceil(P / OP_VC) workgroups of a g do the vectors.
namespace {
constexpr int OP_T = 256, OP_R = 8, OP_C = 64, OP_LD = OP_C + 2;
constexpr int OP_VC = 32, OP_VRG = OP_T / OP_VC;
static_assert(OP_T == OP_R * OP_C / 2, "one thread per column pair of the tile");
static_assert(2 * OP_R * OP_LD <= WV_SEG * OP_VC, "the tile buffers fit the vector job's LDS");

typedef double op_d2 __attribute__((ext_vector_type(2)));
struct __attribute__((aligned(8))) op_pair { double x, y; };   // 16 bytes, 8-byte aligned

template <bool FULL>
__device__ __forceinline__ op_d2 op_load(const double* p, bool v0, bool v1) {
  op_d2 r = {0.0, 0.0};
  if (FULL) {
    const op_pair q = *reinterpret_cast<const op_pair*>(p);
    r.x = q.x;
    r.y = q.y;
  } else {
    if (v0) r.x = p[0];
    if (v1) r.y = p[1];
  }
  return r;
}

template <bool FULL>
__device__ __forceinline__ void op_store(double* p, bool v0, bool v1, double x, double y) {
  if (FULL) {
    op_pair q = {x, y};
    *reinterpret_cast<op_pair*>(p) = q;
  } else {
    if (v0) p[0] = x;
    if (v1) p[1] = y;
  }
}

// The month stream of one thread: the next batch of up to twelve months of its two elements,
// loaded one batch ahead of the adds.  The segments are walked in index order (the caller has
// checked that this IS the canonical order on a rank that owns every chunk), so the batch in
// ``x`` is always the one the next op_segsum trip consumes; the loads of the batch after it
// are issued as soon as the adds have freed the registers, before the window is folded,
// transposed and stored: the memory pipe never drains at a segment boundary.
template <bool FULL>
struct OpStream {
  const double* Xg;                               // X[g] (uniform); off: the thread's (i, j)
  unsigned off;
  const int* seg_start;
  const int* seg_stop;
  int64_t PP;
  int nseg, ps, tm, b;
  bool v0, v1;
  op_d2 x[12];

  // advance to the next batch and load it: always twelve loads, the months past the end of
  // the segment clamped to its last month (cache hits, masked at the adds)
  __device__ __forceinline__ void next() {
    tm += 12;
    while (tm >= b && ps < nseg) {
      tm = seg_start[ps];
      b = seg_stop[ps];
      ++ps;
    }
    if (tm < b) {
#pragma unroll
      for (int m = 0; m < 12; ++m)
        x[m] = op_load<FULL>(Xg + (int64_t)min(tm + m, b - 1) * PP + off, v0, v1);
    }
  }

  // segment sum over months [a, b1): wsum_upper_kernel's order (chain u takes month a + 4 k +
  // u of the whole groups of four, the leftover months go to chain 0 in month order, then
  // (c0 + c1) + (c2 + c3)).  A chain is never -0.0 (it starts at +0.0), so the +0.0 of an
  // absent month leaves its bits alone.
  __device__ __forceinline__ op_d2 segsum(int a, int b1) {
    op_d2 c[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    for (int t0 = a; t0 < b1; t0 += 12) {
      if (t0 + 12 <= b1) {
#pragma unroll
        for (int m = 0; m < 12; ++m) c[m & 3] += x[m];
      } else {
        const int n = b1 - t0, n4 = n & ~3;       // months left, of them in whole groups
#pragma unroll
        for (int m = 0; m < 8; ++m) c[m & 3] += m < n4 ? x[m] : op_d2{0.0, 0.0};
#pragma unroll
        for (int m = 0; m < 11; ++m) c[0] += (m >= n4 && m < n) ? x[m] : op_d2{0.0, 0.0};
      }
      next();
    }
    return (c[0] + c[1]) + (c[2] + c[3]);
  }
};

template <bool FULL>
__device__ __forceinline__ void op_tile(const double* __restrict__ X, int P, int T, int g, int I,
                                        int J, const int* __restrict__ seg_start,
                                        const int* __restrict__ seg_stop, int nseg, int skip,
                                        const int* __restrict__ cs, const int* __restrict__ ce,
                                        int C, const int* __restrict__ sb,
                                        const int* __restrict__ ys, const int* __restrict__ ye,
                                        int clast, double* __restrict__ SD, double* Ts) {
  const int64_t PP = (int64_t)P * P;
  const int nwin = nseg - skip;
  const int t = threadIdx.x;
  const int r = t / (OP_C / 2), cp = (t % (OP_C / 2)) * 2;       // tile row, first column
  const int i = I * OP_R + r, j = J * OP_C + cp;
  const bool v0 = FULL || (i < P && j < P && j >= i);
  const bool v1 = FULL || (i < P && j + 1 < P && j + 1 >= i);
  // the transposed write: target row J OP_C + tc, target columns I OP_R + tr, tr + 1
  const int tc = t / (OP_R / 2), tr = (t % (OP_R / 2)) * 2;
  const int i2 = J * OP_C + tc, j2 = I * OP_R + tr;
  const bool w0 = FULL || (i2 < P && j2 < i2);
  const bool w1 = FULL || (i2 < P && j2 + 1 < i2);
  OpStream<FULL> ms;
  ms.Xg = X + (int64_t)g * T * PP;
  ms.off = FULL || (i < P && j < P) ? (unsigned)i * P + j : 0u;
  ms.seg_start = seg_start;
  ms.seg_stop = seg_stop;
  ms.PP = PP;
  ms.nseg = nseg;
  ms.ps = 0;
  ms.tm = -12;
  ms.b = 0;
  ms.v0 = v0;
  ms.v1 = v1;
#pragma unroll
  for (int m = 0; m < 12; ++m) ms.x[m] = op_d2{0.0, 0.0};
  ms.next();
  op_d2 pc = {0.0, 0.0};
  for (int k = 0; k < C; ++k) {                   // E: the burn-in totals in sb order
    const int q = sb[k];
    op_d2 tot = {0.0, 0.0};
    for (int s = cs[q]; s < ce[q]; ++s) tot += ms.segsum(seg_start[s], seg_stop[s]);
    pc += tot;
  }
  int nst = 0;                                    // windows stored so far: the LDS buffer
  for (int ch = 0; ch <= clast; ++ch) {
    op_d2 acc = pc, tot = {0.0, 0.0};
    for (int s = ys[ch]; s < ye[ch]; ++s) {
      const op_d2 v = ms.segsum(seg_start[s], seg_stop[s]);
      tot += v;
      acc += v;
      if (s < skip) continue;
      double* w = SD + ((int64_t)g * nwin + (s - skip)) * PP;
      op_store<FULL>(w + (int64_t)i * P + j, v0, v1, acc.x, acc.y);
      double* tb = Ts + (nst & 1) * (OP_R * OP_LD);
      ++nst;
      tb[r * OP_LD + cp] = acc.x;
      tb[r * OP_LD + cp + 1] = acc.y;
      __syncthreads();
      op_store<FULL>(w + (int64_t)i2 * P + j2, w0, w1, tb[tr * OP_LD + tc],
                     tb[(tr + 1) * OP_LD + tc]);
    }
    if (ch < clast) pc += tot;
  }
}

__global__ __launch_bounds__(OP_T) void wsum_onepass_kernel(
    const double* __restrict__ X, const double* __restrict__ R, int P, int T,
    const int* __restrict__ seg_start, const int* __restrict__ seg_stop, int nseg, int skip,
    const int* __restrict__ cs, const int* __restrict__ ce, int C, const int* __restrict__ sb,
    const int* __restrict__ ys, const int* __restrict__ ye, int clast, int nvb,
    double* __restrict__ SD, double* __restrict__ Sr) {
  __shared__ double smem[WV_SEG * OP_VC];
  const int g = blockIdx.y, nwin = nseg - skip;
  if ((int)blockIdx.x >= nvb) {
    // upper tiles, row by row: tile row I holds the tile columns I OP_R / OP_C .. ntc - 1
    // (consecutive workgroups, which the dispatcher deals over the XCDs; one run of
    // consecutive tiles per XCD was measured slower, profiles/r14_experiments.md)
    int tile = blockIdx.x - nvb;
    const int ntc = (P + OP_C - 1) / OP_C;
    int I = 0;
    while (tile >= ntc - I * OP_R / OP_C) { tile -= ntc - I * OP_R / OP_C; ++I; }
    const int J = I * OP_R / OP_C + tile;
    const bool full = I * OP_R + OP_R - 1 <= J * OP_C && J * OP_C + OP_C <= P;
    if (full)
      op_tile<true>(X, P, T, g, I, J, seg_start, seg_stop, nseg, skip, cs, ce, C, sb, ys, ye,
                    clast, SD, smem);
    else
      op_tile<false>(X, P, T, g, I, J, seg_start, seg_stop, nseg, skip, cs, ce, C, sb, ys, ye,
                     clast, SD, smem);
    return;
  }
  // the vectors: wvec_chunk_kernel's segment sums (OP_VRG row groups of OP_VC columns), then
  // its mode 0 and mode 1 folds with the totals kept in a register
  double (*part)[OP_VC] = reinterpret_cast<double (*)[OP_VC]>(smem);
  const int lc = threadIdx.x % OP_VC, ry = threadIdx.x / OP_VC;
  const int col = blockIdx.x * OP_VC + lc;
  const bool cv = col < P;
  const double* src = R + (int64_t)g * T * P + (cv ? col : 0);
  wvec_segsums<OP_VC, OP_VRG>(src, P, seg_start, seg_stop, nseg, ry, lc, part);
  __syncthreads();
  if (ry != 0 || !cv) return;
  double pc = 0.0;
  for (int k = 0; k < C; ++k) {
    const int q = sb[k];
    double tot = 0.0;
    for (int s = cs[q]; s < ce[q]; ++s) tot += part[s][lc];
    pc += tot;
  }
  double* o = Sr + (int64_t)g * nwin * P + col;
  for (int ch = 0; ch <= clast; ++ch) {
    double acc = pc, tot = 0.0;
    for (int s = ys[ch]; s < ye[ch]; ++s) {
      tot += part[s][lc];
      acc += part[s][lc];
      if (s >= skip) o[(int64_t)(s - skip) * P] = acc;
    }
    if (ch < clast) pc += tot;
  }
}

}  // namespace

// Matrices and vectors in one launch: SD [G, nseg - skip, P, P] (full, mirrored) and Sr [G,
// nseg - skip, P] from X [G, T, P, P] and R [G, T, P].  idx = [cs, ce, slot] (3 x nlc) and
// cidx = [sb, sy, ys, ye] (4 x C) as above; the caller has checked that this rank owns every
// chunk in canonical order (see the kernel's comment).
extern "C" hipError_t pfml_wsum_onepass(const double* X, const double* R, int P, int T, int G,
                                        const int* seg_start, const int* seg_stop, int nseg,
                                        int skip, int nlc, const int* idx, int C, const int* cidx,
                                        int clast, double* SD, double* Sr, hipStream_t st) {
  if (nseg <= 0 || P <= 0 || G <= 0 || clast < 0 || nseg - skip <= 0) return hipSuccess;
  if (nseg > WV_SEG || skip < 0 || T <= 0 || nlc != 2 * C || clast >= C || P > 65535)
    return hipErrorInvalidValue;
  const int ntr = (P + OP_R - 1) / OP_R, ntc = (P + OP_C - 1) / OP_C;
  int ntile = 0;
  for (int I = 0; I < ntr; ++I) ntile += ntc - I * OP_R / OP_C;
  const int nvb = (P + OP_VC - 1) / OP_VC;
  hipLaunchKernelGGL(wsum_onepass_kernel, dim3(nvb + ntile, G), dim3(OP_T), 0, st, X, R, P, T,
                     seg_start, seg_stop, nseg, skip, idx, idx + nlc, C, cidx, cidx + 2 * C,
                     cidx + 3 * C, clast, nvb, SD, Sr);
  return hipGetLastError();
}

// Vectors, both kernels (mode 0 / 1); idx and cidx as above.
extern "C" hipError_t pfml_wvec_chunk(const double* X, int64_t E, int T, int G,
                                      const int* seg_start, const int* seg_stop, int nseg,
                                      int skip, int mode, int nlc, const int* idx, int C,
                                      const int* cidx, int clast, double* tot, int64_t tstride,
                                      double* out, hipStream_t st) {
  if (nseg <= 0 || E <= 0 || G <= 0) return hipSuccess;
  if (nseg > WV_SEG || skip < 0) return hipErrorInvalidValue;
  if (mode == 1 && (clast < 0 || nseg - skip <= 0)) return hipSuccess;
  if (mode == 0 && nlc <= 0) return hipSuccess;
  hipLaunchKernelGGL(wvec_chunk_kernel, dim3((unsigned)((E + WV_COLS - 1) / WV_COLS), G),
                     dim3(WV_T), 0, st, X, E, T, seg_start, seg_stop, nseg, skip, mode, nlc, idx,
                     idx + nlc, idx + 2 * nlc, C, cidx, cidx + C, cidx + 2 * C, cidx + 3 * C,
                     clast, tot, tstride, out);
  return hipGetLastError();
}
