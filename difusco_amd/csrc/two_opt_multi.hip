// The group-synchronised multi-move 2-opt, both entries.  Every sweep applies a set of improving 2-opt moves whose position
// ranges are pairwise disjoint, not the one best move; the tours of a group count their sweeps together and stop together.
//   difusco_tsp_multi_two_opt_ragged   every row of a sweep evaluates all its columns (FULL sweeps).  The rule is stated in
//                                      include/difusco_hip.h and restated in numpy in tests/multi_two_opt_emulation.py;
//   difusco_tsp_nbr_two_opt_ragged     a row evaluates only its CANDIDATE columns - the pairs (i, j) whose new head edge
//                                      (tour[i], tour[j]) or new tail edge (tour[i+1], tour[j+1]) joins a city to one of its
//                                      listed neighbours, in either direction (NEIGHBOUR sweeps, nbr_rows.h).  A tour whose
//                                      neighbour sweep has no proposal either stops (closing = 0) or goes on with full sweeps
//                                      (closing = 1) until one of them has no proposal.  tests/nbr_two_opt_emulation.py.
// The arithmetic of a change is best_tile's / change64's (two_opt_common.h), bit for bit.
//
// Every tour carries ONE state word - full sweeps (0), neighbour sweeps, stopped - that the selection kernel alone writes, so
// within a sweep every kernel reads the same state.  The plain entry starts every tour in full sweeps, which is the memset that
// clears the loop state; the neighbour entry sets the words to neighbour sweeps behind it.  One kernel set:
//   mt_prep_kernel        tp / dlen of every tour that is still running (prep_entry); in neighbour sweeps also the reset of the
//                         rows (nbr_reset_row);
//   mt_row_value_kernel   neighbour sweeps only: nbr_row_value, the lowest change of every row;
//   mt_row_col_kernel     neighbour sweeps only: nbr_row_col, the lowest column of that change;
//   mt_row_full_kernel    full sweeps only.  One block per (row tile of 16, tour), row_best_tile (multi_move_common.h): a thread
//                         keeps 4 columns of every 1024-column chunk in registers and 16 running bests (change, j), one per row of
//                         the tile, across all chunks; one block reduction per row ends the tile.  A tile's block walks all its
//                         column chunks, so a row's best is complete when the block writes it;
//   mt_select_kernel      one block of 1024 threads per tour: the selection rounds (select_disjoint), the reversals, the switch
//                         from neighbour to full sweeps, the group's stop test and the counters, all on the device.
// The kernels of the sweeps a tour is not in return on their first branch.  The plain entry launches prep, full rows and select;
// the neighbour entry launches all five (the full rows with closing only).  The host enqueues sweeps and polls a counter of
// stopped groups (poll_launches).
//
// The selection (multi_move_common.h, shared with or_opt_multi.hip) never does work proportional to the lengths of the ranges:
// it is O(n log n) per round.  The winners of all rounds are disjoint; a wave reverses one winner's stretch at a time.
//
// Workspace: mt_layout.  The plain entry's holds no pos / rowkey sections.  The neighbour entry's is up256(4 tours) bytes smaller
// than it was while a tour had a done word and a phase word: that is the one section the merged state word removes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"
#include "multi_move_common.h"
#include "nbr_rows.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

enum : int { kFullSweeps = 0, kNbrSweeps = 1, kStopped = 2 };   // a tour's state word

struct MtGroupState {      // device-resident loop state of a group, zero at the start of a call
  int arrived, flags;      // flags: what the tours have reported of this sweep; kGroupStopped stays
  long long sweeps, full_sweeps;
};

struct MtGroup {           // the tours of a group: desc[first .. first + count - 1]
  int first, count;
};

struct MtState {
  int done;                // groups that have stopped
  int pad;
};

constexpr int kMoved = 1, kMovedFull = 2, kRunning = 4;      // what a tour reports of a sweep
constexpr int kGroupStopped = 8;                             // set by the group's stop test, read by later launches only

__global__ void mt_prep_kernel(const double* __restrict__ points, const int* __restrict__ tours, const TourDesc* __restrict__ desc,
                               double2* __restrict__ tp, double* __restrict__ dlen, int* __restrict__ pos,
                               unsigned long long* __restrict__ rowkey, int* __restrict__ rowj, const int* __restrict__ tstate) {
  const TourDesc d = desc[blockIdx.y];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int state = tstate[blockIdx.y];
  if (k > d.n || state == kStopped) return;
  prep_entry(points + d.points, tours + d.closed, d.n, k, tp + d.closed, dlen + d.cols);
  if (k < d.n && state == kNbrSweeps) nbr_reset_row(d, tours, k, pos, rowkey, rowj);
}

__global__ __launch_bounds__(256) void mt_row_value_kernel(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                                           const TourDesc* __restrict__ desc, const double2* __restrict__ tp,
                                                           const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                                           unsigned long long* __restrict__ rowkey,
                                                           const int* __restrict__ tstate) {
  if (tstate[blockIdx.y] != kNbrSweeps) return;
  nbr_row_value(desc[blockIdx.y], false, tours, neighbors, tp, dlen, pos, K, rowkey);
}

__global__ __launch_bounds__(256) void mt_row_col_kernel(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                                         const TourDesc* __restrict__ desc, const double2* __restrict__ tp,
                                                         const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                                         const unsigned long long* __restrict__ rowkey, double* __restrict__ rowv,
                                                         int* __restrict__ rowj, const int* __restrict__ tstate) {
  if (tstate[blockIdx.y] != kNbrSweeps) return;
  nbr_row_col(desc[blockIdx.y], false, tours, neighbors, tp, dlen, pos, K, rowkey, rowv, rowj);
}

__global__ __launch_bounds__(256) void mt_row_full_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                          const TourDesc* __restrict__ desc, double* __restrict__ rowv,
                                                          int* __restrict__ rowj, const int* __restrict__ tstate) {
  const TourDesc d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk_two || tstate[blockIdx.y] != kFullSweeps) return;
  row_best_tile(tp + d.closed, dlen + d.cols, d.n, blockIdx.x * TI, rowv + d.cols, rowj + d.cols);
}

// thread 0 of a tour's block reports to its group; the last tour of the group to report does the group's stop test
__device__ __forceinline__ void report_to_group(MtGroupState* gs, MtGroup g, int flags, long long max_iterations, int* tstate,
                                                MtState* st) {
  if (flags) atomicOr(&gs->flags, flags);
  __threadfence();
  if (atomicAdd(&gs->arrived, 1) != g.count - 1) return;
  __threadfence();
  const int any = atomicExch(&gs->flags, 0);
  gs->arrived = 0;
  if (any & kMoved) gs->sweeps += 1;                             // a sweep counts if one of the group's tours moved,
  if (any & kMovedFull) gs->full_sweeps += 1;                    // and as a full sweep if one that moved was in full sweeps
  if (!(any & kRunning) || gs->sweeps >= max_iterations) {
    gs->flags = kGroupStopped;
    for (int b = g.first; b < g.first + g.count; ++b) tstate[b] = kStopped;
    atomicAdd(&st->done, 1);
  }
}

__global__ __launch_bounds__(kSelectThreads) void mt_select_kernel(
    int* __restrict__ tours, const TourDesc* __restrict__ desc, const MtGroup* __restrict__ grp, const double* __restrict__ rowv_all,
    int* __restrict__ rowj_all, int* __restrict__ live_all, int* __restrict__ winners_all, unsigned long long* __restrict__ tabv_all,
    int* __restrict__ tabi_all, int2* __restrict__ marks_all, int2* __restrict__ cum_all, long long max_iterations, int select_rounds,
    int closing, MtState* st, MtGroupState* gstate, int* tstate, long long* __restrict__ tmoves) {
  const int t = blockIdx.x;
  const TourDesc d = desc[t];
  MtGroupState* gs = gstate + d.group;
  if (gs->flags & kGroupStopped) return;                         // written by an earlier launch only
  const MtGroup G = grp[d.group];
  const int state = tstate[t];                                   // every thread reads it before thread 0 may write it below:
  if (state == kStopped) {                                       // select_disjoint has barriers
    if (threadIdx.x == 0) report_to_group(gs, G, 0, max_iterations, tstate, st);
    return;
  }
  const int n = d.n;
  __shared__ int nwin;
  const int total = select_disjoint(TwoOptRange{rowj_all + d.cols}, n - 2, n, rowv_all + d.cols, live_all + d.cols,
                                    winners_all + d.cols, tabv_all + d.table, tabi_all + d.table, marks_all + d.closed,
                                    cum_all + d.closed, select_rounds, &nwin);
  if (total == 0) {                                              // no proposal: on to the full sweeps, or done
    if (threadIdx.x == 0) {
      const bool go_on = state == kNbrSweeps && closing;
      tstate[t] = go_on ? kFullSweeps : kStopped;
      report_to_group(gs, G, go_on ? kRunning : 0, max_iterations, tstate, st);
    }
    return;
  }
  // apply: the winners' ranges are disjoint
  reverse_winners(tours + d.closed, winners_all + d.cols, rowj_all + d.cols, total);
  if (threadIdx.x == 0) {
    tmoves[t] += total;
    report_to_group(gs, G, kRunning | kMoved | (state == kFullSweeps ? kMovedFull : 0), max_iterations, tstate, st);
  }
}

// ---- the host side: one workspace description (mt_layout, MtPtrs) and one driver (mt_run) behind the two entries

struct MtLayout {          // byte offsets; pos and rowkey are empty without lists
  size_t desc, grp, tp, dlen, pos, rowkey, rowv, rowj, live, winners, tabv, tabi, marks, cum, gstate, tstate, tmoves, st, total;
  GroupTotals tot;
};

// checks the host arrays and lays the workspace out; `tab` (optional) receives the descriptors
int mt_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, bool lists, int K, int closing,
              MtLayout* L, std::vector<TourDesc>* tab) {
  const int rc = walk_groups(who, groups, group_n, group_tours, lists, K, closing, &L->tot, tab);
  if (rc != DIFUSCO_OK) return rc;
  const GroupTotals& t = L->tot;
  Sections s;
  L->desc = s.take(sizeof(TourDesc) * t.tours);
  L->grp = s.take(sizeof(MtGroup) * groups);
  L->tp = s.take(sizeof(double2) * t.closed);
  L->dlen = s.take(sizeof(double) * t.cols);
  L->pos = s.take(sizeof(int) * t.cols, lists);
  L->rowkey = s.take(sizeof(unsigned long long) * t.cols, lists);
  L->rowv = s.take(sizeof(double) * t.cols);
  L->rowj = s.take(sizeof(int) * t.cols);
  L->live = s.take(sizeof(int) * t.cols);
  L->winners = s.take(sizeof(int) * t.cols);
  L->tabv = s.take(sizeof(unsigned long long) * t.cells);
  L->tabi = s.take(sizeof(int) * t.cells);
  L->marks = s.take(sizeof(int2) * t.closed);
  L->cum = s.take(sizeof(int2) * t.closed);
  // gstate .. st are cleared by one memset.  The neighbour entry reserves the 32 bytes per group that its group record took
  // before the state words were merged, so that its size differs from the earlier one by the merged word alone.
  L->gstate = s.take((lists ? 32 : sizeof(MtGroupState)) * groups);
  L->tstate = s.take(sizeof(int) * t.tours);
  L->tmoves = s.take(sizeof(long long) * t.tours);
  L->st = s.take(sizeof(MtState));
  L->total = s.off;
  return DIFUSCO_OK;
}

int mt_workspace_bytes(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, bool lists, int K,
                       int closing, size_t* bytes) {
  if (!bytes) return set_error(DIFUSCO_EINVAL, "%s: bytes is null", who);
  MtLayout lay;
  const int rc = mt_layout(who, groups, group_n, group_tours, lists, K, closing, &lay, nullptr);
  if (rc == DIFUSCO_OK) *bytes = lay.total;
  return rc;
}

struct MtPtrs {            // the sections of a workspace; pos and rowkey are never read without lists
  TourDesc* desc;
  MtGroup* grp;
  double2* tp;
  double *dlen, *rowv;
  int *pos, *rowj, *live, *winners, *tabi, *tstate;
  unsigned long long *rowkey, *tabv;
  int2 *marks, *cum;
  MtGroupState* gstate;
  long long* tmoves;
  MtState* st;
  MtPtrs(void* workspace, const MtLayout& L) {
    char* w = (char*)workspace;
    desc = (TourDesc*)(w + L.desc), grp = (MtGroup*)(w + L.grp), tp = (double2*)(w + L.tp), dlen = (double*)(w + L.dlen);
    pos = (int*)(w + L.pos), rowkey = (unsigned long long*)(w + L.rowkey), rowv = (double*)(w + L.rowv), rowj = (int*)(w + L.rowj);
    live = (int*)(w + L.live), winners = (int*)(w + L.winners), tabv = (unsigned long long*)(w + L.tabv), tabi = (int*)(w + L.tabi);
    marks = (int2*)(w + L.marks), cum = (int2*)(w + L.cum), gstate = (MtGroupState*)(w + L.gstate), tstate = (int*)(w + L.tstate);
    tmoves = (long long*)(w + L.tmoves), st = (MtState*)(w + L.st);
  }
};

struct MtCall {            // a call of one of the two entries
  const char* who;         // the entry, in front of every message
  const char* outputs;     // how the entry's refusal names its host output arrays
  bool lists;              // the neighbour entry
  int groups;
  const int32_t *group_n, *group_tours;
  const double* points;
  int32_t* tours;
  const int32_t* neighbors;
  int K, closing;
  int64_t max_iterations;
  int select_rounds;
  void* workspace;
  size_t workspace_bytes;
  int64_t *sweeps_out, *full_sweeps_out, *moves_out;             // full_sweeps_out: the neighbour entry
  void* stream;
};

// The two entries.  Checks the arguments, sets the device state up, enqueues sweeps until every group has stopped, and reads the
// counters back.
int mt_run(const MtCall& c) {
  const int groups = c.groups;
  MtLayout lay;
  std::vector<TourDesc> tab;
  const int rc = mt_layout(c.who, groups, c.group_n, c.group_tours, c.lists, c.K, c.closing, &lay, &tab);
  if (rc != DIFUSCO_OK) return rc;
  if (c.lists && !c.neighbors) return set_error(DIFUSCO_EINVAL, "%s: neighbors is null", c.who);
  if (!c.points || !c.tours || !c.workspace || !c.sweeps_out || (c.lists && !c.full_sweeps_out) || !c.moves_out || c.max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "%s: needs non-null device arrays, host %s [groups] and max_iterations >= 0", c.who, c.outputs);
  if (c.select_rounds < 1) return set_error(DIFUSCO_EINVAL, "%s: select_rounds = %d, needs at least 1", c.who, c.select_rounds);
  if (c.workspace_bytes < lay.total)
    return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", c.who, c.workspace_bytes, lay.total);
  for (int g = 0; g < groups; ++g) {
    c.sweeps_out[g] = c.moves_out[g] = 0;
    if (c.lists) c.full_sweeps_out[g] = 0;
  }
  if (c.max_iterations == 0) return DIFUSCO_OK;                  // no sweep counts: nothing is applied
  const MtPtrs p(c.workspace, lay);
  hipStream_t s = (hipStream_t)c.stream;
  const int T = lay.tot.tours, K = c.K, closing = c.lists ? c.closing : 0;
  std::vector<MtGroup> gtab(groups);
  for (int g = 0, first = 0; g < groups; first += c.group_tours[g++]) gtab[g] = MtGroup{first, c.group_tours[g]};
  // the tables, once per call; the host vectors live until the synchronisation below
  hipError_t er = hipMemcpyAsync(p.desc, tab.data(), sizeof(TourDesc) * T, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemcpyAsync(p.grp, gtab.data(), sizeof(MtGroup) * groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(p.gstate, 0, lay.total - lay.gstate, s);   // every tour in full sweeps
  if (er == hipSuccess && c.lists) er = hipMemsetD32Async((hipDeviceptr_t)p.tstate, kNbrSweeps, T, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s setup: %s", c.who, hipGetErrorString(er));
  // A launch sequence is a counted sweep of a group or one in which none of its tours moved.  Full sweeps: the first of the
  // latter stops the group - at most max_iterations + 1 sequences.  With lists, in the first of the latter every running tour of
  // the group is without a proposal: it stops or moves to full sweeps, so from then on every running tour is in full sweeps, and
  // the second stops them all - at most max_iterations + 2.
  const int64_t ends = c.lists ? 2 : 1;
  const long long limit = c.max_iterations > INT64_MAX - ends ? INT64_MAX : c.max_iterations + ends;
  const dim3 prep_grid((lay.tot.nmax + 1 + 255) / 256, T), best_grid(lay.tot.nblk_two, T);
  const dim3 walk_grid((unsigned)(((long long)lay.tot.nmax * K + 255) / 256), T);
  const Polled polled = poll_launches(limit, 4, groups, &p.st->done, s, [&] {
    hipLaunchKernelGGL(mt_prep_kernel, prep_grid, dim3(256), 0, s, c.points, c.tours, p.desc, p.tp, p.dlen, p.pos, p.rowkey, p.rowj,
                       p.tstate);
    if (c.lists) {
      hipLaunchKernelGGL(mt_row_value_kernel, walk_grid, dim3(256), 0, s, c.tours, c.neighbors, p.desc, p.tp, p.dlen, p.pos, K,
                         p.rowkey, p.tstate);
      hipLaunchKernelGGL(mt_row_col_kernel, walk_grid, dim3(256), 0, s, c.tours, c.neighbors, p.desc, p.tp, p.dlen, p.pos, K,
                         p.rowkey, p.rowv, p.rowj, p.tstate);
    }
    if (!c.lists || closing)
      hipLaunchKernelGGL(mt_row_full_kernel, best_grid, dim3(256), 0, s, p.tp, p.dlen, p.desc, p.rowv, p.rowj, p.tstate);
    hipLaunchKernelGGL(mt_select_kernel, dim3(T), dim3(kSelectThreads), 0, s, c.tours, p.desc, p.grp, p.rowv, p.rowj, p.live,
                       p.winners, p.tabv, p.tabi, p.marks, p.cum, (long long)c.max_iterations, c.select_rounds, closing, p.st,
                       p.gstate, p.tstate, p.tmoves);
  });
  if (polled.status != hipSuccess) return set_error(DIFUSCO_EHIP, "%s state: %s", c.who, hipGetErrorString(polled.status));
  std::vector<MtGroupState> states(groups);
  std::vector<long long> moves(T);
  er = hipMemcpyAsync(states.data(), p.gstate, sizeof(MtGroupState) * groups, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipMemcpyAsync(moves.data(), p.tmoves, sizeof(long long) * T, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s counters: %s", c.who, hipGetErrorString(er));
  for (int g = 0; g < groups; ++g) {
    c.sweeps_out[g] = states[g].sweeps;
    if (c.lists) c.full_sweeps_out[g] = states[g].full_sweeps;
    for (int b = gtab[g].first; b < gtab[g].first + gtab[g].count; ++b) c.moves_out[g] += moves[b];
  }
  return DIFUSCO_OK;
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_multi_two_opt_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes) {
  return difusco::mt_workspace_bytes("multi_two_opt_ragged_workspace_bytes", groups, group_n, group_tours, false, 0, 0, bytes);
}

int difusco_tsp_multi_two_opt_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                     int32_t* tours, int64_t max_iterations, int select_rounds, void* workspace,
                                     size_t workspace_bytes, int64_t* sweeps_out, int64_t* moves_out, void* stream) {
  return difusco::mt_run({"tsp_multi_two_opt_ragged", "sweeps_out and moves_out", false, groups, group_n, group_tours, points, tours,
                          nullptr, 0, 0, max_iterations, select_rounds, workspace, workspace_bytes, sweeps_out, nullptr, moves_out,
                          stream});
}

int difusco_tsp_nbr_two_opt_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int K, int closing,
                                                   size_t* bytes) {
  return difusco::mt_workspace_bytes("nbr_two_opt_ragged_workspace_bytes", groups, group_n, group_tours, true, K, closing, bytes);
}

int difusco_tsp_nbr_two_opt_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                   int32_t* tours, const int32_t* neighbors, int K, int closing, int64_t max_iterations,
                                   int select_rounds, void* workspace, size_t workspace_bytes, int64_t* sweeps_out,
                                   int64_t* full_sweeps_out, int64_t* moves_out, void* stream) {
  return difusco::mt_run({"tsp_nbr_two_opt_ragged", "sweeps_out, full_sweeps_out and moves_out", true, groups, group_n, group_tours,
                          points, tours, neighbors, K, closing, max_iterations, select_rounds, workspace, workspace_bytes, sweeps_out,
                          full_sweeps_out, moves_out, stream});
}

}  // extern "C"
