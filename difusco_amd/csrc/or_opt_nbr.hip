// Neighbour-list multi-move 2-opt + Or-opt search with a closing full descent (difusco_tsp_nbr_local_search_ragged): the rounds
// of or_opt_multi.hip, but in the NEIGHBOUR STAGE a row of either phase evaluates only its candidate columns - the 2-opt pairs of
// two_opt_multi.hip's neighbour sweeps, and the Or-opt candidates (v, i, j) one of whose two insertion edges (tour[j], a),
// (b, tour[j+1]) joins a city to one of its listed neighbours, in either direction.  A tour whose neighbour-stage round applied no Or-opt move either stops
// (closing = 0) or goes on in the FULL STAGE (closing = 1) with the rounds of or_opt_multi.hip until one of them applies no
// Or-opt move.  The rule is stated in include/difusco_hip.h and restated in numpy in tests/nbr_local_search_emulation.py; a 2-opt
// change is change64's (two_opt_common.h) and an Or-opt delta is or_delta's (or_opt_rows.h), bit for bit.
//
// One sweep is four launches without closing and six with it; every tour carries a stage word and a phase word that are written
// by the selection kernel only, so within a sweep every kernel reads the same stage and phase:
//   nls_prep_kernel         tp / dlen of every running tour; in the neighbour stage also the reset of the rows (nbr_reset_row);
//   nls_row_value_kernel    neighbour stage only: nbr_row_value (nbr_rows.h, shared with two_opt_multi.hip) - the walk of the
//                           lists with the 2-opt pairs or, in the Or-opt phase, the Or-opt candidates: the lowest value of a row;
//   nls_row_col_kernel      neighbour stage only: nbr_row_col, the lowest code - j, Or-opt: v n + j - of that value;
//   nls_full_two_kernel     full stage, 2-opt phase only: row_best_tile (multi_move_common.h);
//   nls_full_or_kernel      full stage, Or-opt phase only: or_row_best_tile (or_opt_rows.h).  A kernel of its own, so that its
//                           register demand is not the 2-opt loop's;
//   nls_select_kernel       mls_select_kernel's body - select_disjoint, reverse_winners, or_opt_winners - plus the stage: the
//                           switch to the full stage, the counters of the full stage.
// The kernels of the stage or phase a tour is not in return on their first branch.  Pads (entries outside 0 .. n-1 or equal to the
// city) are tested before anything is indexed with them.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"
#include "multi_move_common.h"
#include "nbr_rows.h"
#include "or_opt_rows.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

enum Phase : int { kTwoOpt = 0, kOrOpt = 1, kDone = 2 };
enum Stage : int { kNbr = 0, kFullStage = 1 };

struct NlTourState {       // device-resident loop state of a tour, zero at the start of a call
  int stage, phase;
  int round, or_moved;     // round: zero-based; the Or-opt phase of this round (of this stage) has applied a move
  int full_rounds, pad;    // rounds run in the full stage
  long long sweeps, two_opt_sweeps, or_opt_sweeps, two_opt_moves, or_opt_moves;   // sweeps: in which the tour moved
  long long full_sweeps;   // those of them in the full stage
};

struct NlGroup {           // tours of the group, and how many of them are done (zero at the start of a call)
  int count, done;
};

struct NlState {
  int done;                // groups that have stopped
  int pad;
};

__global__ void nls_prep_kernel(const double* __restrict__ points, const int* __restrict__ tours, const TourDesc* __restrict__ desc,
                                double2* __restrict__ tp, double* __restrict__ dlen, int* __restrict__ pos,
                                unsigned long long* __restrict__ rowkey, int* __restrict__ rowj, const NlTourState* __restrict__ ts) {
  const TourDesc d = desc[blockIdx.y];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const NlTourState s = ts[blockIdx.y];
  if (k > d.n || s.phase == kDone) return;
  prep_entry(points + d.points, tours + d.closed, d.n, k, tp + d.closed, dlen + d.cols);
  if (k < d.n && s.stage == kNbr) nbr_reset_row(d, tours, k, pos, rowkey, rowj);
}

__global__ __launch_bounds__(256) void nls_row_value_kernel(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                                            const TourDesc* __restrict__ desc, const double2* __restrict__ tp,
                                                            const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                                            unsigned long long* __restrict__ rowkey,
                                                            const NlTourState* __restrict__ ts) {
  const NlTourState s = ts[blockIdx.y];
  if (s.stage != kNbr || s.phase == kDone) return;
  nbr_row_value(desc[blockIdx.y], s.phase == kOrOpt, tours, neighbors, tp, dlen, pos, K, rowkey);
}

__global__ __launch_bounds__(256) void nls_row_col_kernel(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                                          const TourDesc* __restrict__ desc, const double2* __restrict__ tp,
                                                          const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                                          const unsigned long long* __restrict__ rowkey, double* __restrict__ rowv,
                                                          int* __restrict__ rowj, const NlTourState* __restrict__ ts) {
  const NlTourState s = ts[blockIdx.y];
  if (s.stage != kNbr || s.phase == kDone) return;
  nbr_row_col(desc[blockIdx.y], s.phase == kOrOpt, tours, neighbors, tp, dlen, pos, K, rowkey, rowv, rowj);
}

__global__ __launch_bounds__(256) void nls_full_two_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                           const TourDesc* __restrict__ desc, double* __restrict__ rowv,
                                                           int* __restrict__ rowj, const NlTourState* __restrict__ ts) {
  const NlTourState s = ts[blockIdx.y];
  if (s.stage != kFullStage || s.phase != kTwoOpt) return;
  const TourDesc d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk_two) return;
  row_best_tile(tp + d.closed, dlen + d.cols, d.n, blockIdx.x * TI, rowv + d.cols, rowj + d.cols);
}

__global__ __launch_bounds__(256) void nls_full_or_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                          const TourDesc* __restrict__ desc, double* __restrict__ rowv,
                                                          int* __restrict__ rowj, const NlTourState* __restrict__ ts) {
  const NlTourState s = ts[blockIdx.y];
  if (s.stage != kFullStage || s.phase != kOrOpt) return;
  const TourDesc d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk_or) return;
  or_row_best_tile(tp + d.closed, dlen + d.cols, d.n, blockIdx.x * TI, rowv + d.cols, rowj + d.cols);
}

// thread 0 of a tour that is done: the last tour of its group to finish counts the group as stopped
__device__ __forceinline__ void report_done(NlGroup* g, NlState* st) {
  if (atomicAdd(&g->done, 1) == g->count - 1) atomicAdd(&st->done, 1);
}

// the select step of one tour (the block): the selection and the moves of mls_select_kernel, and the tour's stage, phase, round
// and counters
__global__ __launch_bounds__(kSelectThreads) void nls_select_kernel(
    int* __restrict__ tours, const TourDesc* __restrict__ desc, const double* __restrict__ rowv_all, const int* __restrict__ rowj_all,
    int* __restrict__ live_all, int* __restrict__ winners_all, unsigned long long* __restrict__ tabv_all, int* __restrict__ tabi_all,
    int2* __restrict__ marks_all, int2* __restrict__ cum_all, long long max_iterations, int max_rounds, int select_rounds,
    int closing, NlState* st, NlGroup* grp, NlTourState* ts) {
  const int t = blockIdx.x;
  const int phase = ts[t].phase;                                 // written by thread 0 of this block at its end only
  if (phase == kDone) return;
  const TourDesc d = desc[t];
  const int n = d.n;
  const int* rowj = rowj_all + d.cols;
  int* winners = winners_all + d.cols;
  __shared__ int nwin;
  const int total = select_disjoint(PhaseRange{rowj, n, phase == kOrOpt}, phase == kTwoOpt ? n - 2 : n - 1, n,
                                    rowv_all + d.cols, live_all + d.cols, winners, tabv_all + d.table, tabi_all + d.table,
                                    marks_all + d.closed, cum_all + d.closed, select_rounds, &nwin);
  NlTourState* s = ts + t;                                       // thread 0 alone writes it
  if (total == 0) {                                              // no proposal: the phase ends
    if (threadIdx.x == 0) {
      if (phase == kTwoOpt) {
        s->phase = kOrOpt;
        s->or_moved = 0;
      } else if (s->stage == kNbr && !s->or_moved && closing) {  // the neighbour stage ends: the round goes on with full phases
        s->stage = kFullStage;
        s->phase = kTwoOpt;
        s->full_rounds = 1;
      } else if (!s->or_moved || s->round + 1 >= max_rounds) {
        s->phase = kDone;
        report_done(grp + d.group, st);
      } else {
        s->phase = kTwoOpt;
        s->round += 1;
        if (s->stage == kFullStage) s->full_rounds += 1;
      }
    }
    return;
  }
  if (phase == kTwoOpt)
    reverse_winners(tours + d.closed, winners, rowj, total);
  else
    or_opt_winners(tours + d.closed, (int*)(cum_all + d.closed), winners, rowj, n, total);   // cum is free after the selection
  if (threadIdx.x == 0) {
    s->sweeps += 1;
    if (s->stage == kFullStage) s->full_sweeps += 1;
    if (phase == kTwoOpt) {
      s->two_opt_sweeps += 1;
      s->two_opt_moves += total;
    } else {
      s->or_opt_sweeps += 1;
      s->or_opt_moves += total;
      s->or_moved = 1;
    }
    if (s->sweeps >= max_iterations) {
      s->phase = kDone;
      report_done(grp + d.group, st);
    }
  }
}

struct NlLayout {          // byte offsets
  size_t desc, tp, dlen, pos, rowkey, rowv, rowj, live, winners, tabv, tabi, marks, cum, grp, ts, st, total;
  GroupTotals tot;
};

// checks the host arrays and lays the workspace out; `tab` (optional) receives the descriptors
int nls_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, int K, int closing, NlLayout* L,
               std::vector<TourDesc>* tab) {
  const int rc = walk_groups(who, groups, group_n, group_tours, true, K, closing, &L->tot, tab);
  if (rc != DIFUSCO_OK) return rc;
  const GroupTotals& t = L->tot;
  Sections s;
  L->desc = s.take(sizeof(TourDesc) * t.tours);
  L->tp = s.take(sizeof(double2) * t.closed);
  L->dlen = s.take(sizeof(double) * t.cols);
  L->pos = s.take(sizeof(int) * t.cols);
  L->rowkey = s.take(sizeof(unsigned long long) * t.cols);
  L->rowv = s.take(sizeof(double) * t.cols);
  L->rowj = s.take(sizeof(int) * t.cols);
  L->live = s.take(sizeof(int) * t.cols);
  L->winners = s.take(sizeof(int) * t.cols);
  L->tabv = s.take(sizeof(unsigned long long) * t.cells);
  L->tabi = s.take(sizeof(int) * t.cells);
  L->marks = s.take(sizeof(int2) * t.closed);
  L->cum = s.take(sizeof(int2) * t.closed);
  L->grp = s.take(sizeof(NlGroup) * groups);
  L->ts = s.take(sizeof(NlTourState) * t.tours);                 // ts .. st are cleared by one memset
  L->st = s.take(sizeof(NlState));
  L->total = s.off;
  return DIFUSCO_OK;
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_nbr_local_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int K,
                                                        int closing, size_t* bytes) {
  using namespace difusco;
  if (!bytes) return set_error(DIFUSCO_EINVAL, "nbr_local_search_ragged_workspace_bytes: bytes is null");
  NlLayout lay;
  const int rc = nls_layout("nbr_local_search_ragged_workspace_bytes", groups, group_n, group_tours, K, closing, &lay, nullptr);
  if (rc == DIFUSCO_OK) *bytes = lay.total;
  return rc;
}

int difusco_tsp_nbr_local_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                        int32_t* tours, const int32_t* neighbors, int K, int closing, int64_t max_iterations,
                                        int max_rounds, int select_rounds, void* workspace, size_t workspace_bytes,
                                        int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out, int32_t* rounds_out,
                                        int64_t* two_opt_moves_out, int64_t* or_opt_moves_out, int64_t* full_sweeps_out,
                                        int32_t* full_rounds_out, void* stream) {
  using namespace difusco;
  const char* who = "tsp_nbr_local_search_ragged";
  NlLayout lay;
  std::vector<TourDesc> tab;
  const int rc = nls_layout(who, groups, group_n, group_tours, K, closing, &lay, &tab);
  if (rc != DIFUSCO_OK) return rc;
  if (!neighbors) return set_error(DIFUSCO_EINVAL, "%s: neighbors is null", who);
  if (!points || !tours || !workspace || !two_opt_sweeps_out || !or_opt_sweeps_out || !rounds_out || !two_opt_moves_out ||
      !or_opt_moves_out || !full_sweeps_out || !full_rounds_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "%s: needs non-null device arrays, the seven host output arrays [groups] and "
                                     "max_iterations >= 0", who);
  if (max_rounds < 1) return set_error(DIFUSCO_EINVAL, "%s: max_rounds = %d, needs at least 1", who, max_rounds);
  if (select_rounds < 1) return set_error(DIFUSCO_EINVAL, "%s: select_rounds = %d, needs at least 1", who, select_rounds);
  if (workspace_bytes < lay.total)
    return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", who, workspace_bytes, lay.total);
  for (int g = 0; g < groups; ++g) {
    two_opt_sweeps_out[g] = or_opt_sweeps_out[g] = two_opt_moves_out[g] = or_opt_moves_out[g] = full_sweeps_out[g] = 0;
    rounds_out[g] = 1;                                           // every tour starts round 1
    full_rounds_out[g] = 0;
  }
  if (max_iterations == 0) return DIFUSCO_OK;                    // no sweep may move a tour: nothing is applied
  char* w = (char*)workspace;
  TourDesc* desc = (TourDesc*)(w + lay.desc);
  double2* tp = (double2*)(w + lay.tp);
  double* dlen = (double*)(w + lay.dlen);
  int* pos = (int*)(w + lay.pos);
  unsigned long long* rowkey = (unsigned long long*)(w + lay.rowkey);
  double* rowv = (double*)(w + lay.rowv);
  int* rowj = (int*)(w + lay.rowj);
  int* live = (int*)(w + lay.live);
  int* winners = (int*)(w + lay.winners);
  unsigned long long* tabv = (unsigned long long*)(w + lay.tabv);
  int* tabi = (int*)(w + lay.tabi);
  int2* marks = (int2*)(w + lay.marks);
  int2* cum = (int2*)(w + lay.cum);
  NlGroup* grp = (NlGroup*)(w + lay.grp);
  NlTourState* ts = (NlTourState*)(w + lay.ts);
  NlState* st = (NlState*)(w + lay.st);
  hipStream_t s = (hipStream_t)stream;
  const int T = lay.tot.tours;
  std::vector<NlGroup> gtab(groups);
  for (int g = 0; g < groups; ++g) gtab[g] = NlGroup{group_tours[g], 0};
  // the tables, once per call; the host vectors live until the synchronisation below
  hipError_t er = hipMemcpyAsync(desc, tab.data(), sizeof(TourDesc) * T, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemcpyAsync(grp, gtab.data(), sizeof(NlGroup) * groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(ts, 0, lay.total - lay.ts, s);       // ts .. st, the end of the workspace
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s setup: %s", who, hipGetErrorString(er));
  // A launch sequence either moves a tour (at most max_iterations) or ends one of its phases: two per round, and two more in
  // the round in which the tour goes on to the full stage.
  const long long ends = 2LL * max_rounds + 2;
  const long long limit = max_iterations > INT64_MAX - ends ? INT64_MAX : max_iterations + ends;
  const dim3 prep_grid((lay.tot.nmax + 1 + 255) / 256, T), best_grid(lay.tot.nblk_or, T);
  const dim3 walk_grid((unsigned)(((long long)lay.tot.nmax * K + 255) / 256), T);
  const Polled polled = poll_launches(limit, 4, groups, &st->done, s, [&] {
    hipLaunchKernelGGL(nls_prep_kernel, prep_grid, dim3(256), 0, s, points, tours, desc, tp, dlen, pos, rowkey, rowj, ts);
    hipLaunchKernelGGL(nls_row_value_kernel, walk_grid, dim3(256), 0, s, tours, neighbors, desc, tp, dlen, pos, K, rowkey, ts);
    hipLaunchKernelGGL(nls_row_col_kernel, walk_grid, dim3(256), 0, s, tours, neighbors, desc, tp, dlen, pos, K, rowkey, rowv, rowj,
                       ts);
    if (closing) {
      hipLaunchKernelGGL(nls_full_two_kernel, best_grid, dim3(256), 0, s, tp, dlen, desc, rowv, rowj, ts);
      hipLaunchKernelGGL(nls_full_or_kernel, best_grid, dim3(256), 0, s, tp, dlen, desc, rowv, rowj, ts);
    }
    hipLaunchKernelGGL(nls_select_kernel, dim3(T), dim3(kSelectThreads), 0, s, tours, desc, rowv, rowj, live, winners, tabv, tabi,
                       marks, cum, (long long)max_iterations, max_rounds, select_rounds, closing, st, grp, ts);
  });
  if (polled.status != hipSuccess) return set_error(DIFUSCO_EHIP, "%s state: %s", who, hipGetErrorString(polled.status));
  std::vector<NlTourState> states(T);
  er = hipMemcpyAsync(states.data(), ts, sizeof(NlTourState) * T, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s counters: %s", who, hipGetErrorString(er));
  for (int b = 0; b < T; ++b) {
    const int g = tab[b].group;
    const NlTourState& x = states[b];
    if (x.two_opt_sweeps > two_opt_sweeps_out[g]) two_opt_sweeps_out[g] = x.two_opt_sweeps;
    if (x.or_opt_sweeps > or_opt_sweeps_out[g]) or_opt_sweeps_out[g] = x.or_opt_sweeps;
    if (x.round + 1 > rounds_out[g]) rounds_out[g] = x.round + 1;
    two_opt_moves_out[g] += x.two_opt_moves;
    or_opt_moves_out[g] += x.or_opt_moves;
    if (x.full_sweeps > full_sweeps_out[g]) full_sweeps_out[g] = x.full_sweeps;
    if (x.full_rounds > full_rounds_out[g]) full_rounds_out[g] = x.full_rounds;
  }
  return DIFUSCO_OK;
}

}  // extern "C"
