// Multi-move 2-opt (difusco_tsp_multi_two_opt_ragged): every sweep applies a set of improving 2-opt moves whose position ranges
// are pairwise disjoint, not the one best move.  The rule is stated in include/difusco_hip.h and restated in numpy in
// tests/multi_two_opt_emulation.py; the arithmetic of a change is best_tile's (two_opt_common.h), bit for bit.
//
// One sweep is three launches:
//   multi_prep_kernel       tp / dlen of every tour that is still running (prep_entry);
//   multi_row_best_kernel   one block per (row tile of 16, tour), the loop of best_tile: a thread keeps 4 columns of every
//                           1024-column chunk in registers and 16 running bests (change, j), one per row of the tile, across all
//                           chunks; one block reduction per row ends the tile.  A tile's block walks all its column chunks, so a
//                           row's best is complete when the block writes it and nothing is combined between blocks;
//   multi_select_kernel     one block of 1024 threads per tour: the selection rounds, the reversals, the stop test and the
//                           counters, all on the device.  The host enqueues sweeps and polls a counter of stopped groups.
//
// The selection (multi_move_common.h, shared with or_opt_multi.hip) never does work proportional to the lengths of the ranges:
// it is O(n log n) per round.  The winners of all rounds are disjoint; a wave reverses one winner's stretch at a time.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"
#include "multi_move_common.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

struct MtTour {            // offsets in elements of the array they index
  int n, nblk, group, pad;
  long long points;        // the group's first coordinate in `points` (doubles)
  long long closed;        // the tour's first entry in tours, tp, marks and cum (n + 1 per tour)
  long long cols;          //                       in dlen, rowv, rowj, live and winners (n per tour)
  long long table;         //                       in tabv and tabi (levels (n + 1) per tour)
};

struct MtGroupState {      // device-resident loop state of a group, zero at the start of a call
  int stopped, arrived, moved, pad;
  long long sweeps;
};

struct MtState {
  int done;                // groups that have stopped
  int pad;
};

__global__ void multi_prep_kernel(const double* __restrict__ points, const int* __restrict__ tours,
                                  const MtTour* __restrict__ desc, double2* __restrict__ tp, double* __restrict__ dlen,
                                  const int* __restrict__ tdone) {
  const MtTour d = desc[blockIdx.y];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > d.n || tdone[blockIdx.y]) return;
  prep_entry(points + d.points, tours + d.closed, d.n, k, tp + d.closed, dlen + d.cols);
}

__global__ __launch_bounds__(256) void multi_row_best_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                             const MtTour* __restrict__ desc, double* __restrict__ rowv,
                                                             int* __restrict__ rowj, const int* __restrict__ tdone) {
  const MtTour d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk || tdone[blockIdx.y]) return;
  row_best_tile(tp + d.closed, dlen + d.cols, d.n, blockIdx.x * TI, rowv + d.cols, rowj + d.cols);
}

struct GroupRef {          // the tours of a group: desc[first .. first + count - 1]
  int first, count;
};

// thread 0 of a tour's block reports to its group; the last tour of the group to report does the group's stop test
__device__ __forceinline__ void report_to_group(MtGroupState* gs, GroupRef g, bool moved, long long max_iterations,
                                                int* tdone, MtState* st) {
  if (moved) atomicOr(&gs->moved, 1);
  __threadfence();
  if (atomicAdd(&gs->arrived, 1) != g.count - 1) return;
  __threadfence();
  const int any = atomicExch(&gs->moved, 0);
  gs->arrived = 0;
  if (any) gs->sweeps += 1;                                      // a sweep counts if one of the group's tours moved
  if (!any || gs->sweeps >= max_iterations) {
    gs->stopped = 1;
    for (int b = g.first; b < g.first + g.count; ++b) tdone[b] = 1;
    atomicAdd(&st->done, 1);
  }
}

__global__ __launch_bounds__(kSelectThreads) void multi_select_kernel(
    int* __restrict__ tours, const MtTour* __restrict__ desc, const GroupRef* __restrict__ grp, const double* __restrict__ rowv_all,
    int* __restrict__ rowj_all, int* __restrict__ live_all, int* __restrict__ winners_all, unsigned long long* __restrict__ tabv_all,
    int* __restrict__ tabi_all, int2* __restrict__ marks_all, int2* __restrict__ cum_all, long long max_iterations, int select_rounds,
    MtState* st, MtGroupState* gstate, int* tdone, long long* __restrict__ tmoves) {
  const int t = blockIdx.x;
  const MtTour d = desc[t];
  MtGroupState* gs = gstate + d.group;
  if (gs->stopped) return;                                       // written by an earlier launch only
  const GroupRef G = grp[d.group];
  if (tdone[t]) {
    if (threadIdx.x == 0) report_to_group(gs, G, false, max_iterations, tdone, st);
    return;
  }
  const int n = d.n;
  __shared__ int nwin;
  const int total = select_disjoint(TwoOptRange{rowj_all + d.cols}, n - 2, n, rowv_all + d.cols, live_all + d.cols,
                                    winners_all + d.cols, tabv_all + d.table, tabi_all + d.table, marks_all + d.closed,
                                    cum_all + d.closed, select_rounds, &nwin);
  if (total == 0) {                                              // no proposal: the tour is done
    if (threadIdx.x == 0) {
      tdone[t] = 1;
      report_to_group(gs, G, false, max_iterations, tdone, st);
    }
    return;
  }
  // apply: the winners' ranges are disjoint
  reverse_winners(tours + d.closed, winners_all + d.cols, rowj_all + d.cols, total);
  if (threadIdx.x == 0) {
    tmoves[t] += total;
    report_to_group(gs, G, true, max_iterations, tdone, st);
  }
}

struct MtLayout {          // byte offsets
  size_t desc, grp, tp, dlen, rowv, rowj, live, winners, tabv, tabi, marks, cum, gstate, tdone, tmoves, st, total;
  int tours, nmax, nblk_max;
};

// checks the host arrays and lays the workspace out; `tab` / `gtab` (optional) receive the tables
int multi_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, MtLayout* L,
                 std::vector<MtTour>* tab, std::vector<GroupRef>* gtab) {
  int T = 0;
  const int rc = check_groups(who, groups, group_n, group_tours, &T);
  if (rc != DIFUSCO_OK) return rc;
  size_t points = 0, closed = 0, cols = 0, cells = 0;
  int first = 0;
  L->nmax = L->nblk_max = 0;
  for (int g = 0; g < groups; ++g) {
    const int n = group_n[g], nblk = (n - 2 + TI - 1) / TI;       // rows 0 .. n - 3
    L->nmax = n > L->nmax ? n : L->nmax;
    L->nblk_max = nblk > L->nblk_max ? nblk : L->nblk_max;
    if (gtab) gtab->push_back(GroupRef{first, group_tours[g]});
    first += group_tours[g];
    for (int p = 0; p < group_tours[g]; ++p) {
      if (tab) tab->push_back(MtTour{n, nblk, g, 0, (long long)points, (long long)closed, (long long)cols, (long long)cells});
      closed += (size_t)n + 1;
      cols += (size_t)n;
      cells += (size_t)table_levels(n) * ((size_t)n + 1);
    }
    points += 2 * (size_t)n;
  }
  L->tours = (int)T;
  size_t off = 0;
  auto take = [&off](size_t bytes) {
    const size_t at = off;
    off += up256(bytes);
    return at;
  };
  L->desc = take(sizeof(MtTour) * T);
  L->grp = take(sizeof(GroupRef) * groups);
  L->tp = take(sizeof(double2) * closed);
  L->dlen = take(sizeof(double) * cols);
  L->rowv = take(sizeof(double) * cols);
  L->rowj = take(sizeof(int) * cols);
  L->live = take(sizeof(int) * cols);
  L->winners = take(sizeof(int) * cols);
  L->tabv = take(sizeof(unsigned long long) * cells);
  L->tabi = take(sizeof(int) * cells);
  L->marks = take(sizeof(int2) * closed);
  L->cum = take(sizeof(int2) * closed);
  L->gstate = take(sizeof(MtGroupState) * groups);               // gstate .. st are cleared by one memset
  L->tdone = take(sizeof(int) * T);
  L->tmoves = take(sizeof(long long) * T);
  L->st = take(sizeof(MtState));
  L->total = off;
  return DIFUSCO_OK;
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_multi_two_opt_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes) {
  using namespace difusco;
  if (!bytes) return set_error(DIFUSCO_EINVAL, "multi_two_opt_ragged_workspace_bytes: bytes is null");
  MtLayout lay;
  const int rc = multi_layout("multi_two_opt_ragged_workspace_bytes", groups, group_n, group_tours, &lay, nullptr, nullptr);
  if (rc == DIFUSCO_OK) *bytes = lay.total;
  return rc;
}

int difusco_tsp_multi_two_opt_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                     int32_t* tours, int64_t max_iterations, int select_rounds, void* workspace,
                                     size_t workspace_bytes, int64_t* sweeps_out, int64_t* moves_out, void* stream) {
  using namespace difusco;
  MtLayout lay;
  std::vector<MtTour> tab;
  std::vector<GroupRef> gtab;
  const int rc = multi_layout("tsp_multi_two_opt_ragged", groups, group_n, group_tours, &lay, &tab, &gtab);
  if (rc != DIFUSCO_OK) return rc;
  if (!points || !tours || !workspace || !sweeps_out || !moves_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_multi_two_opt_ragged: needs non-null device arrays, host sweeps_out and moves_out "
                                     "[groups] and max_iterations >= 0");
  if (select_rounds < 1)
    return set_error(DIFUSCO_EINVAL, "tsp_multi_two_opt_ragged: select_rounds = %d, needs at least 1", select_rounds);
  if (workspace_bytes < lay.total)
    return set_error(DIFUSCO_EINVAL, "tsp_multi_two_opt_ragged: workspace %zu < %zu bytes", workspace_bytes, lay.total);
  for (int g = 0; g < groups; ++g) sweeps_out[g] = moves_out[g] = 0;
  if (max_iterations == 0) return DIFUSCO_OK;                    // no sweep counts: nothing is applied
  char* w = (char*)workspace;
  MtTour* desc = (MtTour*)(w + lay.desc);
  GroupRef* grp = (GroupRef*)(w + lay.grp);
  double2* tp = (double2*)(w + lay.tp);
  double* dlen = (double*)(w + lay.dlen);
  double* rowv = (double*)(w + lay.rowv);
  int* rowj = (int*)(w + lay.rowj);
  int* live = (int*)(w + lay.live);
  int* winners = (int*)(w + lay.winners);
  unsigned long long* tabv = (unsigned long long*)(w + lay.tabv);
  int* tabi = (int*)(w + lay.tabi);
  int2* marks = (int2*)(w + lay.marks);
  int2* cum = (int2*)(w + lay.cum);
  MtGroupState* gstate = (MtGroupState*)(w + lay.gstate);
  int* tdone = (int*)(w + lay.tdone);
  long long* tmoves = (long long*)(w + lay.tmoves);
  MtState* st = (MtState*)(w + lay.st);
  hipStream_t s = (hipStream_t)stream;
  const int T = lay.tours;
  // the tables, once per call; the host vectors live until the synchronisation below
  hipError_t er = hipMemcpyAsync(desc, tab.data(), sizeof(MtTour) * T, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemcpyAsync(grp, gtab.data(), sizeof(GroupRef) * groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(gstate, 0, lay.total - lay.gstate, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "tsp_multi_two_opt_ragged setup: %s", hipGetErrorString(er));
  // a launch sequence is a counted sweep of a group or the one that finds it without a proposal: at most max_iterations + 1
  const long long limit = max_iterations < INT64_MAX ? max_iterations + 1 : INT64_MAX;
  MtState host{0, 0};
  const int poll = 4;
  const dim3 prep_grid((lay.nmax + 1 + 255) / 256, T), best_grid(lay.nblk_max, T);
  for (long long it = 0; it < limit; ++it) {
    hipLaunchKernelGGL(multi_prep_kernel, prep_grid, dim3(256), 0, s, points, tours, desc, tp, dlen, tdone);
    hipLaunchKernelGGL(multi_row_best_kernel, best_grid, dim3(256), 0, s, tp, dlen, desc, rowv, rowj, tdone);
    hipLaunchKernelGGL(multi_select_kernel, dim3(T), dim3(kSelectThreads), 0, s, tours, desc, grp, rowv, rowj, live, winners, tabv,
                       tabi, marks, cum, (long long)max_iterations, select_rounds, st, gstate, tdone, tmoves);
    if ((it + 1) % poll == 0 || it + 1 == limit) {
      er = hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s);
      if (er == hipSuccess) er = hipStreamSynchronize(s);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "multi_two_opt state: %s", hipGetErrorString(er));
      if (host.done >= groups) break;
    }
  }
  std::vector<MtGroupState> states(groups);
  std::vector<long long> moves(T);
  er = hipMemcpyAsync(states.data(), gstate, sizeof(MtGroupState) * groups, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipMemcpyAsync(moves.data(), tmoves, sizeof(long long) * T, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "tsp_multi_two_opt_ragged counters: %s", hipGetErrorString(er));
  for (int g = 0; g < groups; ++g) {
    sweeps_out[g] = states[g].sweeps;
    for (int b = gtab[g].first; b < gtab[g].first + gtab[g].count; ++b) moves_out[g] += moves[b];
  }
  return DIFUSCO_OK;
}

}  // extern "C"
