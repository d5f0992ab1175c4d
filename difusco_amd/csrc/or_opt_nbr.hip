// Neighbour-list multi-move 2-opt + Or-opt search with a closing full descent (difusco_tsp_nbr_local_search_ragged): the rounds
// of or_opt_multi.hip, but in the NEIGHBOUR STAGE a row of either phase evaluates only its candidate columns - the 2-opt pairs of
// two_opt_nbr.hip, and the Or-opt candidates (v, i, j) one of whose two insertion edges (tour[j], a), (b, tour[j+1]) joins a city
// to one of its listed neighbours, in either direction.  A tour whose neighbour-stage round applied no Or-opt move either stops
// (closing = 0) or goes on in the FULL STAGE (closing = 1) with the rounds of or_opt_multi.hip until one of them applies no
// Or-opt move.  The rule is stated in include/difusco_hip.h and restated in numpy in tests/nbr_local_search_emulation.py; a 2-opt
// change is change64's (two_opt_common.h) and an Or-opt delta is or_delta's (or_opt_rows.h), bit for bit.
//
// One sweep is four launches without closing and six with it; every tour carries a stage word and a phase word that are written
// by the selection kernel only, so within a sweep every kernel reads the same stage and phase:
//   nls_prep_kernel         tp / dlen of every running tour; in the neighbour stage also pos[city] = its position, and the rows
//                           are reset: rowkey = no key, rowj = -1;
//   nls_row_value_kernel    neighbour stage only.  One thread per (position p, list slot s) of a tour: x = tour[p], y = its s-th
//                           listed city, q = pos[y].  2-opt phase: nbr_pairs (multi_move_common.h), the walk of two_opt_nbr.hip.
//                           Or-opt phase: or_nbr_candidates - each of the two cities takes the role of a segment end while the
//                           other is the anchor, up to 20 candidates per thread, the bounds tested before any point is read.  A
//                           value below the threshold does a 64-bit atomic min of its ordered bits on rowkey[i]; the others are
//                           dropped at once;
//   nls_row_col_kernel      the same walk again: a candidate whose value equals rowkey[i] writes rowv[i] (every such thread writes
//                           the same bits) and does a 32-bit unsigned atomic min of its code - j, Or-opt: v n + j - on rowj[i].
//                           The row ends with its lowest (value, code) whatever the order of the threads;
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
#include "or_opt_rows.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

enum Phase : int { kTwoOpt = 0, kOrOpt = 1, kDone = 2 };
enum Stage : int { kNbr = 0, kFullStage = 1 };

struct NlTour {            // offsets in elements of the array they index
  int n, nblk_two, nblk_or, group;
  long long points;        // the group's first coordinate in `points` (doubles)
  long long nbr;           // the group's first entry in `neighbors` (n K per group)
  long long closed;        // the tour's first entry in tours, tp, marks and cum (n + 1 per tour)
  long long cols;          //                       in dlen, pos, rowkey, rowv, rowj, live and winners (n per tour)
  long long table;         //                       in tabv and tabi (levels (n + 1) per tour)
};

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

__global__ void nls_prep_kernel(const double* __restrict__ points, const int* __restrict__ tours, const NlTour* __restrict__ desc,
                                double2* __restrict__ tp, double* __restrict__ dlen, int* __restrict__ pos,
                                unsigned long long* __restrict__ rowkey, int* __restrict__ rowj, const NlTourState* __restrict__ ts) {
  const NlTour d = desc[blockIdx.y];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const NlTourState s = ts[blockIdx.y];
  if (k > d.n || s.phase == kDone) return;
  prep_entry(points + d.points, tours + d.closed, d.n, k, tp + d.closed, dlen + d.cols);
  if (k < d.n && s.stage == kNbr) {
    pos[d.cols + tours[d.closed + k]] = k;                      // a tour is a permutation of 0 .. n-1 (the entry's convention)
    rowkey[d.cols + k] = kNoKey;
    rowj[d.cols + k] = -1;
  }
}

// The Or-opt candidates of (position p, listed city at position q): each of the two cities is the segment end, at position e, and
// the other the anchor.  As `a` (the end joined to tour[j]) the end gives j = the anchor's position; as `b` (the end joined to
// tour[j+1]) it gives j = the anchor's position minus 1, position 0 read as n.  The end is the segment's first city (i = e - 1)
// or its last (i = e - L), by variant and orientation.  f(i, v n + j, delta) is called for every valid candidate: 0 <= i <=
// n - 1 - L (hence 1 <= e <= n - 1: position 0 never moves), j outside [i, i + L]; 0 <= j <= n - 1 holds by construction.  The
// bounds are tested before or_candidate_delta reads a point.
template <class F>
__device__ __forceinline__ void or_nbr_candidates(const double2* __restrict__ P, const double* __restrict__ D, int n, int p, int q,
                                                  F f) {
#pragma unroll
  for (int role = 0; role < 2; ++role) {
    const int e = role ? q : p, anchor = role ? p : q;
    const int ja = anchor, jb = (anchor == 0 ? n : anchor) - 1;
#pragma unroll
    for (int v = 0; v < 5; ++v) {
      const int L = variant_len(v);
      const bool rev = variant_rev(v);
      const int ia = rev ? e - L : e - 1, ib = rev ? e - 1 : e - L;   // the end as a, as b
      if (ia >= 0 && ia <= n - 1 - L && (ja < ia || ja > ia + L)) f(ia, v * n + ja, or_candidate_delta(P, D, v, ia, ja));
      if (ib >= 0 && ib <= n - 1 - L && (jb < ib || jb > ib + L)) f(ib, v * n + jb, or_candidate_delta(P, D, v, ib, jb));
    }
  }
}

// the walk both row kernels share: thread (p, s) of tour blockIdx.y; f(row, code, value)
template <class F>
__device__ __forceinline__ void nls_walk(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                         const NlTour* __restrict__ desc, const double2* __restrict__ tp,
                                         const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                         const NlTourState* __restrict__ ts, F f) {
  const NlTourState s = ts[blockIdx.y];
  if (s.stage != kNbr || s.phase == kDone) return;
  const NlTour d = desc[blockIdx.y];
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)d.n * K) return;
  const int p = (int)(e / K), slot = (int)(e % K);
  const int x = tours[d.closed + p];
  const int y = neighbors[d.nbr + (long long)x * K + slot];
  if (y < 0 || y >= d.n || y == x) return;                       // a pad: nothing is indexed with it
  const int q = pos[d.cols + y];
  if (s.phase == kTwoOpt)
    nbr_pairs(tp + d.closed, dlen + d.cols, d.n, p, q, f);
  else
    or_nbr_candidates(tp + d.closed, dlen + d.cols, d.n, p, q, f);
}

__global__ __launch_bounds__(256) void nls_row_value_kernel(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                                            const NlTour* __restrict__ desc, const double2* __restrict__ tp,
                                                            const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                                            unsigned long long* __restrict__ rowkey,
                                                            const NlTourState* __restrict__ ts) {
  unsigned long long* keys = rowkey + desc[blockIdx.y].cols;
  nls_walk(tours, neighbors, desc, tp, dlen, pos, K, ts, [keys](int i, int, double value) {
    if (value < kThreshold) atomicMin(&keys[i], ordered_bits(value));
  });
}

__global__ __launch_bounds__(256) void nls_row_col_kernel(const int* __restrict__ tours, const int* __restrict__ neighbors,
                                                          const NlTour* __restrict__ desc, const double2* __restrict__ tp,
                                                          const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                                          const unsigned long long* __restrict__ rowkey, double* __restrict__ rowv,
                                                          int* __restrict__ rowj, const NlTourState* __restrict__ ts) {
  const long long cols = desc[blockIdx.y].cols;
  const unsigned long long* keys = rowkey + cols;
  double* vals = rowv + cols;
  unsigned* codes = (unsigned*)(rowj + cols);                    // -1 is the highest unsigned: no column yet; 5 n fits 32 bits
  nls_walk(tours, neighbors, desc, tp, dlen, pos, K, ts, [keys, vals, codes](int i, int code, double value) {
    if (value < kThreshold && ordered_bits(value) == keys[i]) {
      vals[i] = value;
      atomicMin(&codes[i], (unsigned)code);
    }
  });
}

__global__ __launch_bounds__(256) void nls_full_two_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                           const NlTour* __restrict__ desc, double* __restrict__ rowv,
                                                           int* __restrict__ rowj, const NlTourState* __restrict__ ts) {
  const NlTourState s = ts[blockIdx.y];
  if (s.stage != kFullStage || s.phase != kTwoOpt) return;
  const NlTour d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk_two) return;
  row_best_tile(tp + d.closed, dlen + d.cols, d.n, blockIdx.x * TI, rowv + d.cols, rowj + d.cols);
}

__global__ __launch_bounds__(256) void nls_full_or_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                          const NlTour* __restrict__ desc, double* __restrict__ rowv,
                                                          int* __restrict__ rowj, const NlTourState* __restrict__ ts) {
  const NlTourState s = ts[blockIdx.y];
  if (s.stage != kFullStage || s.phase != kOrOpt) return;
  const NlTour d = desc[blockIdx.y];
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
    int* __restrict__ tours, const NlTour* __restrict__ desc, const double* __restrict__ rowv_all, const int* __restrict__ rowj_all,
    int* __restrict__ live_all, int* __restrict__ winners_all, unsigned long long* __restrict__ tabv_all, int* __restrict__ tabi_all,
    int2* __restrict__ marks_all, int2* __restrict__ cum_all, long long max_iterations, int max_rounds, int select_rounds,
    int closing, NlState* st, NlGroup* grp, NlTourState* ts) {
  const int t = blockIdx.x;
  const int phase = ts[t].phase;                                 // written by thread 0 of this block at its end only
  if (phase == kDone) return;
  const NlTour d = desc[t];
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
  int tours, nmax, nblk_max;
};

// checks the host arrays and lays the workspace out; `tab` / `gtab` (optional) receive the tables
int nls_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, int K, int closing, NlLayout* L,
               std::vector<NlTour>* tab, std::vector<NlGroup>* gtab) {
  int T = 0;
  const int rc = check_groups(who, groups, group_n, group_tours, &T);
  if (rc != DIFUSCO_OK) return rc;
  if (K < 1) return set_error(DIFUSCO_EINVAL, "%s: K = %d, needs at least 1", who, K);
  if (closing != 0 && closing != 1) return set_error(DIFUSCO_EINVAL, "%s: closing = %d, needs 0 or 1", who, closing);
  size_t points = 0, nbr = 0, closed = 0, cols = 0, cells = 0;
  L->nmax = L->nblk_max = 0;
  for (int g = 0; g < groups; ++g) {
    const int n = group_n[g];
    const int nblk_two = (n - 2 + TI - 1) / TI, nblk_or = (n - 1 + TI - 1) / TI;   // rows 0 .. n - 3 and 0 .. n - 2
    if ((long long)n * K > (long long)INT32_MAX * 256)
      return set_error(DIFUSCO_EINVAL, "%s: group %d has n K = %lld list entries, too many for one launch", who, g, (long long)n * K);
    L->nmax = n > L->nmax ? n : L->nmax;
    L->nblk_max = nblk_or > L->nblk_max ? nblk_or : L->nblk_max;
    if (gtab) gtab->push_back(NlGroup{group_tours[g], 0});
    for (int p = 0; p < group_tours[g]; ++p) {
      if (tab)
        tab->push_back(NlTour{n, nblk_two, nblk_or, g, (long long)points, (long long)nbr, (long long)closed, (long long)cols,
                              (long long)cells});
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
  L->desc = take(sizeof(NlTour) * T);
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
  L->grp = take(sizeof(NlGroup) * groups);
  L->ts = take(sizeof(NlTourState) * T);                         // ts .. st are cleared by one memset
  L->st = take(sizeof(NlState));
  L->total = off;
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
  const int rc = nls_layout("nbr_local_search_ragged_workspace_bytes", groups, group_n, group_tours, K, closing, &lay, nullptr, nullptr);
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
  std::vector<NlTour> tab;
  std::vector<NlGroup> gtab;
  const int rc = nls_layout(who, groups, group_n, group_tours, K, closing, &lay, &tab, &gtab);
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
  NlTour* desc = (NlTour*)(w + lay.desc);
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
  const int T = lay.tours;
  // the tables, once per call; the host vectors live until the synchronisation below
  hipError_t er = hipMemcpyAsync(desc, tab.data(), sizeof(NlTour) * T, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemcpyAsync(grp, gtab.data(), sizeof(NlGroup) * groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(ts, 0, lay.total - lay.ts, s);       // ts .. st, the end of the workspace
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s setup: %s", who, hipGetErrorString(er));
  // A launch sequence either moves a tour (at most max_iterations) or ends one of its phases: two per round, and two more in
  // the round in which the tour goes on to the full stage.
  const long long ends = 2LL * max_rounds + 2;
  const long long limit = max_iterations > INT64_MAX - ends ? INT64_MAX : max_iterations + ends;
  NlState host{0, 0};
  const int poll = 4;
  const dim3 prep_grid((lay.nmax + 1 + 255) / 256, T), best_grid(lay.nblk_max, T);
  const dim3 walk_grid((unsigned)(((long long)lay.nmax * K + 255) / 256), T);
  for (long long it = 0; it < limit; ++it) {
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
    if ((it + 1) % poll == 0 || it + 1 == limit) {
      er = hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s);
      if (er == hipSuccess) er = hipStreamSynchronize(s);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s state: %s", who, hipGetErrorString(er));
      if (host.done >= groups) break;
    }
  }
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
