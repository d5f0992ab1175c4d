// The row kernels of the neighbour-list multi-move 2-opt + Or-opt search with a closing full descent
// (difusco_tsp_nbr_local_search_ragged): the rounds of or_opt_multi.hip, but in the NEIGHBOUR STAGE a row of either phase
// evaluates only its candidate columns - the 2-opt pairs of two_opt_multi.hip's neighbour sweeps, and the Or-opt candidates
// (v, i, j) one of whose two insertion edges (tour[j], a), (b, tour[j+1]) joins a city to one of its listed neighbours, in either
// direction.  A tour whose neighbour-stage round applied no Or-opt move either stops (closing = 0) or goes on in the FULL STAGE
// (closing = 1) with the rounds of or_opt_multi.hip until one of them applies no Or-opt move.  The rule is stated in
// include/difusco_hip.h and restated in numpy in tests/nbr_local_search_emulation.py; a 2-opt change is change64's
// (two_opt_common.h) and an Or-opt delta is or_delta's (or_opt_rows.h), bit for bit.
//
// Included by or_opt_multi.hip behind its select kernels.  The stage is part of a tour's phase word (Phase: kTwoOpt, kOrOpt in the
// neighbour stage, where a tour starts; kFullTwoOpt, kFullOrOpt in the full stage), which the select step alone writes
// (mls_select_tour<kSelectListed>: the switch to the full stage, the counters of the full stage in MlStage), so within a sweep
// every kernel reads the same word.  One sweep is four launches without closing and six with it:
//   nls_prep_kernel         tp / dlen of every running tour; in the neighbour stage also the reset of the rows (nbr_reset_row);
//   nls_row_value_kernel    neighbour stage only: nbr_row_value (nbr_rows.h, shared with two_opt_multi.hip) - the walk of the
//                           lists with the 2-opt pairs or, in the Or-opt phase, the Or-opt candidates: the lowest value of a row;
//   nls_row_col_kernel      neighbour stage only: nbr_row_col, the lowest code - j, Or-opt: v n + j - of that value;
//   nls_full_two_kernel     full stage, 2-opt phase only: row_best_tile (multi_move_common.h);
//   nls_full_or_kernel      full stage, Or-opt phase only: or_row_best_tile (or_opt_rows.h).  A kernel of its own, so that its
//                           register demand is not the 2-opt loop's;
//   mls_select_listed_kernel  (or_opt_multi.hip).
// The kernels of the stage or phase a tour is not in return on their first branch.  Pads (entries outside 0 .. n-1 or equal to the
// city) are tested before anything is indexed with them.
#pragma once

#include "nbr_rows.h"

namespace difusco {
namespace {

__device__ __forceinline__ bool nbr_stage(int phase) { return phase == kTwoOpt || phase == kOrOpt; }

__global__ void nls_prep_kernel(const double* __restrict__ points, const int* __restrict__ tours, const TourDesc* __restrict__ desc,
                                double2* __restrict__ tp, double* __restrict__ dlen, int* __restrict__ pos,
                                unsigned long long* __restrict__ rowkey, int* __restrict__ rowj, const MlTourState* __restrict__ ts) {
  const TourDesc d = desc[blockIdx.y];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int phase = ts[blockIdx.y].phase;
  if (k > d.n || phase == kDone) return;
  prep_entry(points + d.points, tours + d.closed, d.n, k, tp + d.closed, dlen + d.cols);
  if (k < d.n && nbr_stage(phase)) nbr_reset_row(d, tours, k, pos, rowkey, rowj);
}

__global__ __launch_bounds__(256) void nls_row_value_kernel(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                                            const TourDesc* __restrict__ desc, const double2* __restrict__ tp,
                                                            const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                                            unsigned long long* __restrict__ rowkey,
                                                            const MlTourState* __restrict__ ts) {
  const int phase = ts[blockIdx.y].phase;
  if (!nbr_stage(phase)) return;
  nbr_row_value(desc[blockIdx.y], phase == kOrOpt, tours, neighbors, tp, dlen, pos, K, rowkey);
}

__global__ __launch_bounds__(256) void nls_row_col_kernel(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                                          const TourDesc* __restrict__ desc, const double2* __restrict__ tp,
                                                          const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                                          const unsigned long long* __restrict__ rowkey, double* __restrict__ rowv,
                                                          int* __restrict__ rowj, const MlTourState* __restrict__ ts) {
  const int phase = ts[blockIdx.y].phase;
  if (!nbr_stage(phase)) return;
  nbr_row_col(desc[blockIdx.y], phase == kOrOpt, tours, neighbors, tp, dlen, pos, K, rowkey, rowv, rowj);
}

__global__ __launch_bounds__(256) void nls_full_two_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                           const TourDesc* __restrict__ desc, double* __restrict__ rowv,
                                                           int* __restrict__ rowj, const MlTourState* __restrict__ ts) {
  if (ts[blockIdx.y].phase != kFullTwoOpt) return;
  const TourDesc d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk_two) return;
  row_best_tile(tp + d.closed, dlen + d.cols, d.n, blockIdx.x * TI, rowv + d.cols, rowj + d.cols);
}

__global__ __launch_bounds__(256) void nls_full_or_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                          const TourDesc* __restrict__ desc, double* __restrict__ rowv,
                                                          int* __restrict__ rowj, const MlTourState* __restrict__ ts) {
  if (ts[blockIdx.y].phase != kFullOrOpt) return;
  const TourDesc d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk_or) return;
  or_row_best_tile(tp + d.closed, dlen + d.cols, d.n, blockIdx.x * TI, rowv + d.cols, rowj + d.cols);
}

}  // namespace
}  // namespace difusco
