// Cell descriptor and launch arguments shared by the ridge-grid kernels (ridge.hip:
// tridiagonal path, ridge_band*.hip: band path).  RidgeCellDesc mirrors
// ops/ridge.py::CELL_DTYPE.
#pragma once
#include <stdint.h>

struct RidgeCellDesc {
  int64_t src;      // offset (doubles) of the running-sum matrix S_D for this cell
  int64_t rsrc;     // offset of the running-sum vector S_r
  int64_t work;     // offset of this cell's workspace
  int64_t out;      // offset of beta output [L][ldo]
  int n;            // p + 1
  double scale;     // 1 / T  (the reference divides both sums by n months)
};

// One launch of the ridge grid (pfml_ridge_grid): everything the launch reads, its options
// included - the library keeps no state between launches.  Layout mirrors
// ops/ridge.py::LaunchArgs (checked there against pfml_ridge_launch_args_size).
struct RidgeLaunchArgs {
  const double* SD;            // running-sum matrices, rows ldS apart
  int64_t ldS;
  const double* Sr;            // running-sum vectors
  const RidgeCellDesc* cells;  // device, ncells of them, the largest n first
  int ncells;
  int nmax;                    // largest n of the launch: picks the path and the instances
  const double* lvec;          // device, L lambdas
  int L;
  double* work;                // sum of pfml_ridge_work_doubles(n, L) over the cells
  double* beta;                // [.][L][ldo] at each cell's `out`
  int64_t ldo;
  // band path: the in-band pivoted-LU repair list (lu_count nullptr = no repair)
  int* lu_list;
  int* lu_count;
  int lu_cap;
  // band path: workgroup map of the cooperative reduction (cell << 8 | w << 4 | K - 1),
  // COOP_SYNC sync words per cell, and the cells' n in plan order (host)
  const int* wgmap;
  int nwg;
  unsigned* syncw;
  const int* n_host;
  // options
  long long* timing;           // band path: device cycle counters (pfml_ridge_timing_words); nullptr = off
  unsigned spin_max;           // band path: poll bound of the cooperative waits; 0 = the default
  int phases;                  // tridiagonal path: bit 0 tridiagonalisation, 1 solves, 2 back-transform; 7 = all
  bool solo;                   // band path: a launch whose cells all have K = 1 on the solo instance
  bool bt_wy;                  // tridiagonal path: n > 1024 cells on the blocked-WY back-transform
  bool bt_classes;             // band path: a back-transform instance per size class of n_host
};
