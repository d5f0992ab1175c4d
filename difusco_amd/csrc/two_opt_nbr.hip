// Neighbour-list multi-move 2-opt with a closing full descent (difusco_tsp_nbr_two_opt_ragged): the sweeps of two_opt_multi.hip,
// but a row evaluates only its CANDIDATE columns - the pairs (i, j) whose new head edge (tour[i], tour[j]) or new tail edge
// (tour[i+1], tour[j+1]) joins a city to one of its listed neighbours, in either direction.  A tour whose neighbour sweep has no
// proposal either stops (closing = 0) or goes on with full sweeps (closing = 1, row_best_tile: the rule of two_opt_multi.hip)
// until one of them has no proposal.  The rule is stated in include/difusco_hip.h and restated in numpy in
// tests/nbr_two_opt_emulation.py; the arithmetic of a change is change64's (two_opt_common.h), bit for bit.
//
// One sweep is five launches; every tour carries a phase word (0 = neighbour sweeps, 1 = full sweeps) that is written by the
// selection kernel only, so within a sweep every kernel reads the same phase:
//   nbr_prep_kernel         tp / dlen of every running tour; in the neighbour phase also pos[city] = its position, and the rows
//                           are reset: rowkey = no key, rowj = -1;
//   nbr_row_value_kernel    neighbour phase only.  One thread per (position p, list slot s) of a tour: a = tour[p], c = its
//                           s-th listed city, q = pos[c].  The head pair of the two cities is (min(p, q), max(p, q)); the tail
//                           pair is that of the positions with 0 read as n (position n is position 0), minus one each.  A pair's
//                           row is therefore not the thread's own, so the threads combine: a change below the threshold does a
//                           64-bit atomic min of its ordered bits on rowkey[i].  Changes that are not below the threshold are
//                           dropped at once: such a row does not propose;
//   nbr_row_col_kernel      the same walk again: a pair whose change equals rowkey[i] writes rowv[i] (every such thread writes the
//                           same bits) and does a 32-bit unsigned atomic min of j on rowj[i].  The row ends with its lowest
//                           (change, j) whatever the order of the threads; nobody waits for anybody;
//   nbr_row_full_kernel     full phase only: multi_row_best_kernel's body;
//   nbr_select_kernel       multi_select_kernel's body plus the phase switch: a tour without a proposal in the neighbour phase
//                           with closing = 1 moves to the full phase instead of stopping.
// The kernels of the phase a tour is not in return on their first branch.  Pads (entries outside 0 .. n-1 or equal to the city)
// are tested before anything is indexed with them.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"
#include "multi_move_common.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

struct NbTour {            // offsets in elements of the array they index
  int n, nblk, group, pad;
  long long points;        // the group's first coordinate in `points` (doubles)
  long long nbr;           // the group's first entry in `neighbors` (n K per group)
  long long closed;        // the tour's first entry in tours, tp, marks and cum (n + 1 per tour)
  long long cols;          //                       in dlen, pos, rowkey, rowv, rowj, live and winners (n per tour)
  long long table;         //                       in tabv and tabi (levels (n + 1) per tour)
};

struct NbGroupState {      // device-resident loop state of a group, zero at the start of a call
  int stopped, arrived, flags, pad;
  long long sweeps, full_sweeps;
};

struct NbState {
  int done;                // groups that have stopped
  int pad;
};

struct NbGroupRef {        // the tours of a group: desc[first .. first + count - 1]
  int first, count;
};

constexpr int kMoved = 1, kMovedFull = 2, kRunning = 4;      // what a tour reports of a sweep

__global__ void nbr_prep_kernel(const double* __restrict__ points, const int* __restrict__ tours, const NbTour* __restrict__ desc,
                                double2* __restrict__ tp, double* __restrict__ dlen, int* __restrict__ pos,
                                unsigned long long* __restrict__ rowkey, int* __restrict__ rowj, const int* __restrict__ tdone,
                                const int* __restrict__ tphase) {
  const NbTour d = desc[blockIdx.y];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > d.n || tdone[blockIdx.y]) return;
  prep_entry(points + d.points, tours + d.closed, d.n, k, tp + d.closed, dlen + d.cols);
  if (k < d.n && tphase[blockIdx.y] == 0) {
    pos[d.cols + tours[d.closed + k]] = k;                      // a tour is a permutation of 0 .. n-1 (the entry's convention)
    rowkey[d.cols + k] = kNoKey;
    rowj[d.cols + k] = -1;
  }
}

// the walk both row kernels share (nbr_pairs: multi_move_common.h): thread (p, s) of tour blockIdx.y
template <class F>
__device__ __forceinline__ void nbr_walk(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                         const NbTour* __restrict__ desc, const double2* __restrict__ tp,
                                         const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                         const int* __restrict__ tdone, const int* __restrict__ tphase, F f) {
  const NbTour d = desc[blockIdx.y];
  if (tdone[blockIdx.y] || tphase[blockIdx.y] != 0) return;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)d.n * K) return;
  const int p = (int)(e / K), s = (int)(e % K);
  const int a = tours[d.closed + p];
  const int c = neighbors[d.nbr + (long long)a * K + s];
  if (c < 0 || c >= d.n || c == a) return;                       // a pad: nothing is indexed with it
  nbr_pairs(tp + d.closed, dlen + d.cols, d.n, p, pos[d.cols + c], f);
}

__global__ __launch_bounds__(256) void nbr_row_value_kernel(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                                            const NbTour* __restrict__ desc, const double2* __restrict__ tp,
                                                            const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                                            unsigned long long* __restrict__ rowkey,
                                                            const int* __restrict__ tdone, const int* __restrict__ tphase) {
  unsigned long long* keys = rowkey + desc[blockIdx.y].cols;
  nbr_walk(tours, neighbors, desc, tp, dlen, pos, K, tdone, tphase, [keys](int i, int, double change) {
    if (change < kThreshold) atomicMin(&keys[i], ordered_bits(change));
  });
}

__global__ __launch_bounds__(256) void nbr_row_col_kernel(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                                          const NbTour* __restrict__ desc, const double2* __restrict__ tp,
                                                          const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                                          const unsigned long long* __restrict__ rowkey, double* __restrict__ rowv,
                                                          int* __restrict__ rowj, const int* __restrict__ tdone,
                                                          const int* __restrict__ tphase) {
  const long long cols = desc[blockIdx.y].cols;
  const unsigned long long* keys = rowkey + cols;
  double* vals = rowv + cols;
  unsigned* js = (unsigned*)(rowj + cols);                       // -1 is the highest unsigned: no column yet
  nbr_walk(tours, neighbors, desc, tp, dlen, pos, K, tdone, tphase, [keys, vals, js](int i, int j, double change) {
    if (change < kThreshold && ordered_bits(change) == keys[i]) {
      vals[i] = change;
      atomicMin(&js[i], (unsigned)j);
    }
  });
}

__global__ __launch_bounds__(256) void nbr_row_full_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                           const NbTour* __restrict__ desc, double* __restrict__ rowv,
                                                           int* __restrict__ rowj, const int* __restrict__ tdone,
                                                           const int* __restrict__ tphase) {
  const NbTour d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk || tdone[blockIdx.y] || tphase[blockIdx.y] != 1) return;
  row_best_tile(tp + d.closed, dlen + d.cols, d.n, blockIdx.x * TI, rowv + d.cols, rowj + d.cols);
}

// thread 0 of a tour's block reports to its group; the last tour of the group to report does the group's stop test
__device__ __forceinline__ void report_to_group(NbGroupState* gs, NbGroupRef g, int flags, long long max_iterations, int* tdone,
                                                NbState* st) {
  if (flags) atomicOr(&gs->flags, flags);
  __threadfence();
  if (atomicAdd(&gs->arrived, 1) != g.count - 1) return;
  __threadfence();
  const int any = atomicExch(&gs->flags, 0);
  gs->arrived = 0;
  if (any & kMoved) gs->sweeps += 1;                             // a sweep counts if one of the group's tours moved,
  if (any & kMovedFull) gs->full_sweeps += 1;                    // and as a full sweep if one that moved was in the full phase
  if (!(any & kRunning) || gs->sweeps >= max_iterations) {
    gs->stopped = 1;
    for (int b = g.first; b < g.first + g.count; ++b) tdone[b] = 1;
    atomicAdd(&st->done, 1);
  }
}

__global__ __launch_bounds__(kSelectThreads) void nbr_select_kernel(
    int* __restrict__ tours, const NbTour* __restrict__ desc, const NbGroupRef* __restrict__ grp, const double* __restrict__ rowv_all,
    int* __restrict__ rowj_all, int* __restrict__ live_all, int* __restrict__ winners_all, unsigned long long* __restrict__ tabv_all,
    int* __restrict__ tabi_all, int2* __restrict__ marks_all, int2* __restrict__ cum_all, long long max_iterations, int select_rounds,
    int closing, NbState* st, NbGroupState* gstate, int* tdone, int* tphase, long long* __restrict__ tmoves) {
  const int t = blockIdx.x;
  const NbTour d = desc[t];
  NbGroupState* gs = gstate + d.group;
  if (gs->stopped) return;                                       // written by an earlier launch only
  const NbGroupRef G = grp[d.group];
  if (tdone[t]) {
    if (threadIdx.x == 0) report_to_group(gs, G, 0, max_iterations, tdone, st);
    return;
  }
  const int n = d.n;
  const int phase = tphase[t];                                   // every thread reads it before thread 0 may write it below:
  __shared__ int nwin;                                           // select_disjoint has barriers
  const int total = select_disjoint(TwoOptRange{rowj_all + d.cols}, n - 2, n, rowv_all + d.cols, live_all + d.cols,
                                    winners_all + d.cols, tabv_all + d.table, tabi_all + d.table, marks_all + d.closed,
                                    cum_all + d.closed, select_rounds, &nwin);
  if (total == 0) {                                              // no proposal: on to the full sweeps, or done
    if (threadIdx.x == 0) {
      if (phase == 0 && closing) {
        tphase[t] = 1;
        report_to_group(gs, G, kRunning, max_iterations, tdone, st);
      } else {
        tdone[t] = 1;
        report_to_group(gs, G, 0, max_iterations, tdone, st);
      }
    }
    return;
  }
  // apply: the winners' ranges are disjoint
  reverse_winners(tours + d.closed, winners_all + d.cols, rowj_all + d.cols, total);
  if (threadIdx.x == 0) {
    tmoves[t] += total;
    report_to_group(gs, G, kRunning | kMoved | (phase ? kMovedFull : 0), max_iterations, tdone, st);
  }
}

struct NbLayout {          // byte offsets
  size_t desc, grp, tp, dlen, pos, rowkey, rowv, rowj, live, winners, tabv, tabi, marks, cum, gstate, tdone, tphase, tmoves, st, total;
  int tours, nmax, nblk_max;
};

// checks the host arrays and lays the workspace out; `tab` / `gtab` (optional) receive the tables
int nbr_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, int K, int closing, NbLayout* L,
               std::vector<NbTour>* tab, std::vector<NbGroupRef>* gtab) {
  int T = 0;
  const int rc = check_groups(who, groups, group_n, group_tours, &T);
  if (rc != DIFUSCO_OK) return rc;
  if (K < 1) return set_error(DIFUSCO_EINVAL, "%s: K = %d, needs at least 1", who, K);
  if (closing != 0 && closing != 1) return set_error(DIFUSCO_EINVAL, "%s: closing = %d, needs 0 or 1", who, closing);
  size_t points = 0, nbr = 0, closed = 0, cols = 0, cells = 0;
  int first = 0;
  L->nmax = L->nblk_max = 0;
  for (int g = 0; g < groups; ++g) {
    const int n = group_n[g], nblk = (n - 2 + TI - 1) / TI;       // rows 0 .. n - 3
    if ((long long)n * K > (long long)INT32_MAX * 256)
      return set_error(DIFUSCO_EINVAL, "%s: group %d has n K = %lld list entries, too many for one launch", who, g, (long long)n * K);
    L->nmax = n > L->nmax ? n : L->nmax;
    L->nblk_max = nblk > L->nblk_max ? nblk : L->nblk_max;
    if (gtab) gtab->push_back(NbGroupRef{first, group_tours[g]});
    first += group_tours[g];
    for (int p = 0; p < group_tours[g]; ++p) {
      if (tab)
        tab->push_back(NbTour{n, nblk, g, 0, (long long)points, (long long)nbr, (long long)closed, (long long)cols, (long long)cells});
      closed += (size_t)n + 1;
      cols += (size_t)n;
      cells += (size_t)table_levels(n) * ((size_t)n + 1);
    }
    points += 2 * (size_t)n;
    nbr += (size_t)n * (size_t)K;
  }
  L->tours = (int)T;
  size_t off = 0;
  auto take = [&off](size_t bytes) {
    const size_t at = off;
    off += up256(bytes);
    return at;
  };
  L->desc = take(sizeof(NbTour) * T);
  L->grp = take(sizeof(NbGroupRef) * groups);
  L->tp = take(sizeof(double2) * closed);
  L->dlen = take(sizeof(double) * cols);
  L->pos = take(sizeof(int) * cols);
  L->rowkey = take(sizeof(unsigned long long) * cols);
  L->rowv = take(sizeof(double) * cols);
  L->rowj = take(sizeof(int) * cols);
  L->live = take(sizeof(int) * cols);
  L->winners = take(sizeof(int) * cols);
  L->tabv = take(sizeof(unsigned long long) * cells);
  L->tabi = take(sizeof(int) * cells);
  L->marks = take(sizeof(int2) * closed);
  L->cum = take(sizeof(int2) * closed);
  L->gstate = take(sizeof(NbGroupState) * groups);               // gstate .. st are cleared by one memset
  L->tdone = take(sizeof(int) * T);
  L->tphase = take(sizeof(int) * T);
  L->tmoves = take(sizeof(long long) * T);
  L->st = take(sizeof(NbState));
  L->total = off;
  return DIFUSCO_OK;
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_nbr_two_opt_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int K, int closing,
                                                   size_t* bytes) {
  using namespace difusco;
  if (!bytes) return set_error(DIFUSCO_EINVAL, "nbr_two_opt_ragged_workspace_bytes: bytes is null");
  NbLayout lay;
  const int rc = nbr_layout("nbr_two_opt_ragged_workspace_bytes", groups, group_n, group_tours, K, closing, &lay, nullptr, nullptr);
  if (rc == DIFUSCO_OK) *bytes = lay.total;
  return rc;
}

int difusco_tsp_nbr_two_opt_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                   int32_t* tours, const int32_t* neighbors, int K, int closing, int64_t max_iterations,
                                   int select_rounds, void* workspace, size_t workspace_bytes, int64_t* sweeps_out,
                                   int64_t* full_sweeps_out, int64_t* moves_out, void* stream) {
  using namespace difusco;
  NbLayout lay;
  std::vector<NbTour> tab;
  std::vector<NbGroupRef> gtab;
  const int rc = nbr_layout("tsp_nbr_two_opt_ragged", groups, group_n, group_tours, K, closing, &lay, &tab, &gtab);
  if (rc != DIFUSCO_OK) return rc;
  if (!neighbors) return set_error(DIFUSCO_EINVAL, "tsp_nbr_two_opt_ragged: neighbors is null");
  if (!points || !tours || !workspace || !sweeps_out || !full_sweeps_out || !moves_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_nbr_two_opt_ragged: needs non-null device arrays, host sweeps_out, full_sweeps_out and "
                                     "moves_out [groups] and max_iterations >= 0");
  if (select_rounds < 1)
    return set_error(DIFUSCO_EINVAL, "tsp_nbr_two_opt_ragged: select_rounds = %d, needs at least 1", select_rounds);
  if (workspace_bytes < lay.total)
    return set_error(DIFUSCO_EINVAL, "tsp_nbr_two_opt_ragged: workspace %zu < %zu bytes", workspace_bytes, lay.total);
  for (int g = 0; g < groups; ++g) sweeps_out[g] = full_sweeps_out[g] = moves_out[g] = 0;
  if (max_iterations == 0) return DIFUSCO_OK;                    // no sweep counts: nothing is applied
  char* w = (char*)workspace;
  NbTour* desc = (NbTour*)(w + lay.desc);
  NbGroupRef* grp = (NbGroupRef*)(w + lay.grp);
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
  NbGroupState* gstate = (NbGroupState*)(w + lay.gstate);
  int* tdone = (int*)(w + lay.tdone);
  int* tphase = (int*)(w + lay.tphase);
  long long* tmoves = (long long*)(w + lay.tmoves);
  NbState* st = (NbState*)(w + lay.st);
  hipStream_t s = (hipStream_t)stream;
  const int T = lay.tours;
  // the tables, once per call; the host vectors live until the synchronisation below
  hipError_t er = hipMemcpyAsync(desc, tab.data(), sizeof(NbTour) * T, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemcpyAsync(grp, gtab.data(), sizeof(NbGroupRef) * groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(gstate, 0, lay.total - lay.gstate, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "tsp_nbr_two_opt_ragged setup: %s", hipGetErrorString(er));
  // A launch sequence is a counted sweep of a group or one in which none of its tours moved.  In the first of the latter every
  // running tour of the group is without a proposal: it stops or moves to the full phase, so from then on every running tour is
  // in the full phase, and the second stops them all.  At most max_iterations + 2 sequences.
  const long long limit = max_iterations < INT64_MAX - 1 ? max_iterations + 2 : INT64_MAX;
  NbState host{0, 0};
  const int poll = 4;
  const dim3 prep_grid((lay.nmax + 1 + 255) / 256, T), best_grid(lay.nblk_max, T);
  const dim3 walk_grid((unsigned)(((long long)lay.nmax * K + 255) / 256), T);
  for (long long it = 0; it < limit; ++it) {
    hipLaunchKernelGGL(nbr_prep_kernel, prep_grid, dim3(256), 0, s, points, tours, desc, tp, dlen, pos, rowkey, rowj, tdone, tphase);
    hipLaunchKernelGGL(nbr_row_value_kernel, walk_grid, dim3(256), 0, s, tours, neighbors, desc, tp, dlen, pos, K, rowkey, tdone,
                       tphase);
    hipLaunchKernelGGL(nbr_row_col_kernel, walk_grid, dim3(256), 0, s, tours, neighbors, desc, tp, dlen, pos, K, rowkey, rowv, rowj,
                       tdone, tphase);
    if (closing)
      hipLaunchKernelGGL(nbr_row_full_kernel, best_grid, dim3(256), 0, s, tp, dlen, desc, rowv, rowj, tdone, tphase);
    hipLaunchKernelGGL(nbr_select_kernel, dim3(T), dim3(kSelectThreads), 0, s, tours, desc, grp, rowv, rowj, live, winners, tabv,
                       tabi, marks, cum, (long long)max_iterations, select_rounds, closing, st, gstate, tdone, tphase, tmoves);
    if ((it + 1) % poll == 0 || it + 1 == limit) {
      er = hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s);
      if (er == hipSuccess) er = hipStreamSynchronize(s);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "nbr_two_opt state: %s", hipGetErrorString(er));
      if (host.done >= groups) break;
    }
  }
  std::vector<NbGroupState> states(groups);
  std::vector<long long> moves(T);
  er = hipMemcpyAsync(states.data(), gstate, sizeof(NbGroupState) * groups, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipMemcpyAsync(moves.data(), tmoves, sizeof(long long) * T, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "tsp_nbr_two_opt_ragged counters: %s", hipGetErrorString(er));
  for (int g = 0; g < groups; ++g) {
    sweeps_out[g] = states[g].sweeps;
    full_sweeps_out[g] = states[g].full_sweeps;
    for (int b = gtab[g].first; b < gtab[g].first + gtab[g].count; ++b) moves_out[g] += moves[b];
  }
  return DIFUSCO_OK;
}

}  // extern "C"
