// Multi-move local search (difusco_tsp_multi_local_search_ragged): per tour, rounds of a multi-move 2-opt phase and a multi-move
// Or-opt phase.  A sweep of either phase applies a set of improving moves whose position ranges are pairwise disjoint.  The rule
// is stated in include/difusco_hip.h and restated in numpy in tests/multi_local_search_emulation.py; a 2-opt change is best_tile's
// (two_opt_common.h) and an Or-opt delta is or_opt_tile's (or_opt.hip), bit for bit.
//
// One sweep is three launches, whatever the phases of the tours:
//   mls_prep_kernel       tp / dlen of every tour that is still running (prep_entry);
//   mls_row_best_kernel   one block per (row tile of 16, tour), the loop of the tour's phase.  2-opt: row_best_tile
//                         (multi_move_common.h), the loop of two_opt_multi.hip.  Or-opt: or_row_best_tile (or_opt_rows.h), the
//                         loop of or_opt_tile -
//                         a thread keeps 4 columns of every 1024-column chunk in registers, walks the rows of the tile upwards and
//                         carries |P_j P_i+2|, |P_j P_i+3| (and the two from P_j+1) to the next row, two square roots per (i, j)
//                         for all five variants; the row-only terms are computed once per tile in LDS - with 16 running bests
//                         (delta, v n + j), one per row, across all chunks and one block reduction per row at the end.  A tile's
//                         block walks all its column chunks, so nothing is combined between blocks;
//   mls_select_kernel     one block of 1024 threads per tour: the selection rounds (select_disjoint, multi_move_common.h) on
//                         (key, range), the moves of the phase - a wave reverses one winner's stretch, or copies one winner's
//                         stretch to a buffer of the tour's own and writes it back shifted -, the switch of phase and round, the
//                         stop tests and the counters.  The last tour of a group to finish counts the group as stopped; the
//                         host enqueues sweeps and polls the counter of stopped groups.
// The iterated search (difusco_tsp_iterated_search_ragged) launches the same three and a fourth after them:
//   mls_keep_kick_kernel  one block of 1024 threads per tour whose descent has just ended: the length of the tour in one fixed
//                         association, the comparison with the tour's incumbent, the copy one way or the other, and either the
//                         next seeded kick (segment swaps read from the incumbent) with a reset of the descent state, or the end.
// The focused search (difusco_tsp_focused_search_ragged) launches the first two as they are and three of its own
// (or_opt_focused.h, included behind the kernels here): after a kick a tour's sweeps evaluate only candidates next to a marked edge.
// The guided search (difusco_tsp_guided_search_ragged) is either of the two with the keep / kick kernel's `kHeat` instantiation:
// the first cut of a draw is drawn by the heat of the incumbent's edges (or_opt_heat.h).  Both keep / kick kernels draw a kick
// with kick_draws here and apply it with kick_swaps (multi_move_common.h, which also holds what the window search of
// tsp_window_search.hip shares with this file: PhaseRange, or_opt_winners, tour_length).
// The listed search (difusco_tsp_nbr_local_search_ragged) is one descent whose rounds start in a neighbour stage: its row kernels
// (or_opt_nbr.h, included behind the select kernels here) replace the first two, and the select step is the one here with the
// switch of stage (mls_select_tour<kSelectListed>).
//
// The host side of all five entries is at the end of this file, once: mls_layout describes the workspace - the sections of the
// descent and, as the entry needs them, the list sections, the iterated state, the focus state and the heat tables - and builds
// the host tables (the walk over the groups and the launch loop with its poll are multi_move_common.h's, shared with
// two_opt_multi.hip),
// MlPtrs holds the sections as typed pointers, and mls_run(MlCall) checks the arguments, sets the state up, enqueues launch
// sequences under their bound, polls, reads the state back and reduces it to the outputs.  The entries fill an MlCall: its mode
// (one descent, one descent on neighbour lists, iterated, iterated with focused descents), whether the kicks are drawn by heat,
// the arguments and the outputs.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "common.h"
#include "kernels.h"
#include "multi_move_common.h"
#include "or_opt_rows.h"      // LMAX, or_delta, or_row_best_tile
#include "two_opt_common.h"

namespace difusco {
namespace {

// kKeep: the iterated search only.  kFullTwoOpt, kFullOrOpt: the listed search only - its tours start in the neighbour stage,
// where kTwoOpt and kOrOpt are the phases on neighbour rows, and go on in the full stage with these two
enum Phase : int { kTwoOpt = 0, kOrOpt = 1, kDone = 2, kKeep = 3, kFullTwoOpt = 4, kFullOrOpt = 5 };

struct MlTourState {       // device-resident loop state of a tour, zero at the start of a call
  int phase, round;        // round: zero-based
  int or_moved, pad;       // the Or-opt phase of this round has applied a move
  long long sweeps, two_opt_sweeps, or_opt_sweeps, two_opt_moves, or_opt_moves;   // sweeps: in which the tour moved
};

struct MlStage {           // what the listed search counts of a tour's full stage, behind the MlTourState records; zero at the start
  long long full_sweeps;   // sweeps in which the tour moved in the full stage
  int full_rounds, pad;    // rounds run in the full stage
};

struct MlGroup {           // tours of the group, and how many of them are done (zero at the start of a call)
  int count, done;
};

struct MlState {
  int done;                // groups that have stopped
  int pad;
};

__global__ void mls_prep_kernel(const double* __restrict__ points, const int* __restrict__ tours, const TourDesc* __restrict__ desc,
                                double2* __restrict__ tp, double* __restrict__ dlen, const MlTourState* __restrict__ ts) {
  const TourDesc d = desc[blockIdx.y];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > d.n || ts[blockIdx.y].phase == kDone) return;
  prep_entry(points + d.points, tours + d.closed, d.n, k, tp + d.closed, dlen + d.cols);
}

__global__ __launch_bounds__(256) void mls_row_best_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                           const TourDesc* __restrict__ desc, double* __restrict__ rowv,
                                                           int* __restrict__ rowj, const MlTourState* __restrict__ ts) {
  const TourDesc d = desc[blockIdx.y];
  const int phase = ts[blockIdx.y].phase;                        // uniform over the block
  if (phase == kDone || (int)blockIdx.x >= (phase == kTwoOpt ? d.nblk_two : d.nblk_or)) return;
  const int i0 = blockIdx.x * TI;
  if (phase == kTwoOpt)
    row_best_tile(tp + d.closed, dlen + d.cols, d.n, i0, rowv + d.cols, rowj + d.cols);
  else
    or_row_best_tile(tp + d.closed, dlen + d.cols, d.n, i0, rowv + d.cols, rowj + d.cols);
}

// thread 0 of a tour that is done: the last tour of its group to finish counts the group as stopped
__device__ __forceinline__ void report_done(MlGroup* g, MlState* st) {
  if (atomicAdd(&g->done, 1) == g->count - 1) atomicAdd(&st->done, 1);
}

enum SelectMode : int { kSelectPlain = 0, kSelectIterated = 1, kSelectListed = 2 };

// the select step of one tour (the block).  kSelectIterated: where the descent ends, the tour goes to the keep / kick step of the
// iterated search (mls_keep_kick_kernel) instead of being done.  kSelectListed: the tour starts in the neighbour stage; an Or-opt
// phase without a move there ends the stage, and with `closing` the round goes on with full phases, counted in stages[t].
// The other two modes read neither `closing` nor `stages`.
template <SelectMode kMode>
__device__ __forceinline__ void mls_select_tour(
    int* __restrict__ tours, const TourDesc* __restrict__ desc, const double* __restrict__ rowv_all, const int* __restrict__ rowj_all,
    int* __restrict__ live_all, int* __restrict__ winners_all, unsigned long long* __restrict__ tabv_all, int* __restrict__ tabi_all,
    int2* __restrict__ marks_all, int2* __restrict__ cum_all, long long max_iterations, int max_rounds, int select_rounds,
    MlState* st, MlGroup* grp, MlTourState* ts, int closing = 0, MlStage* stages = nullptr) {
  constexpr bool kListed = kMode == kSelectListed;
  const int t = blockIdx.x;
  const int word = ts[t].phase;                                  // written by thread 0 of this block at its end only
  if (word == kDone) return;
  const bool full = kListed && word >= kFullTwoOpt;              // the tour is in the full stage of the listed search
  const int phase = full ? word - kFullTwoOpt : word;            // kTwoOpt or kOrOpt, in either stage
  const TourDesc d = desc[t];
  const int n = d.n;
  const int* rowj = rowj_all + d.cols;
  int* winners = winners_all + d.cols;
  __shared__ int nwin;
  const int total = select_disjoint(PhaseRange{rowj, n, phase == kOrOpt}, phase == kTwoOpt ? n - 2 : n - 1, n,
                                    rowv_all + d.cols, live_all + d.cols, winners, tabv_all + d.table, tabi_all + d.table,
                                    marks_all + d.closed, cum_all + d.closed, select_rounds, &nwin);
  MlTourState* s = ts + t;                                       // thread 0 alone writes it
  if (total == 0) {                                              // no proposal: the phase ends
    if (threadIdx.x == 0) {
      if (phase == kTwoOpt) {
        s->phase = full ? kFullOrOpt : kOrOpt;
        s->or_moved = 0;
      } else if (kListed && !full && !s->or_moved && closing) {  // the neighbour stage ends: the round goes on with full phases
        s->phase = kFullTwoOpt;
        stages[t].full_rounds = 1;
      } else if (!s->or_moved || s->round + 1 >= max_rounds) {
        if constexpr (kMode == kSelectIterated) {
          s->phase = kKeep;
        } else {
          s->phase = kDone;
          report_done(grp + d.group, st);
        }
      } else {
        s->phase = full ? kFullTwoOpt : kTwoOpt;
        s->round += 1;
        if constexpr (kListed)
          if (full) stages[t].full_rounds += 1;
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
    if constexpr (kListed)
      if (full) stages[t].full_sweeps += 1;
    if (phase == kTwoOpt) {
      s->two_opt_sweeps += 1;
      s->two_opt_moves += total;
    } else {
      s->or_opt_sweeps += 1;
      s->or_opt_moves += total;
      s->or_moved = 1;
    }
    if (s->sweeps >= max_iterations) {
      if constexpr (kMode == kSelectIterated) {
        s->phase = kKeep;
      } else {
        s->phase = kDone;
        report_done(grp + d.group, st);
      }
    }
  }
}

__global__ __launch_bounds__(kSelectThreads) void mls_select_kernel(
    int* __restrict__ tours, const TourDesc* __restrict__ desc, const double* __restrict__ rowv_all, const int* __restrict__ rowj_all,
    int* __restrict__ live_all, int* __restrict__ winners_all, unsigned long long* __restrict__ tabv_all, int* __restrict__ tabi_all,
    int2* __restrict__ marks_all, int2* __restrict__ cum_all, long long max_iterations, int max_rounds, int select_rounds,
    MlState* st, MlGroup* grp, MlTourState* ts) {
  mls_select_tour<kSelectPlain>(tours, desc, rowv_all, rowj_all, live_all, winners_all, tabv_all, tabi_all, marks_all, cum_all,
                                max_iterations, max_rounds, select_rounds, st, grp, ts);
}

// the listed search (difusco_tsp_nbr_local_search_ragged): its row kernels are in or_opt_nbr.h
__global__ __launch_bounds__(kSelectThreads) void mls_select_listed_kernel(
    int* __restrict__ tours, const TourDesc* __restrict__ desc, const double* __restrict__ rowv_all, const int* __restrict__ rowj_all,
    int* __restrict__ live_all, int* __restrict__ winners_all, unsigned long long* __restrict__ tabv_all, int* __restrict__ tabi_all,
    int2* __restrict__ marks_all, int2* __restrict__ cum_all, long long max_iterations, int max_rounds, int select_rounds,
    int closing, MlState* st, MlGroup* grp, MlTourState* ts, MlStage* stages) {
  mls_select_tour<kSelectListed>(tours, desc, rowv_all, rowj_all, live_all, winners_all, tabv_all, tabi_all, marks_all, cum_all,
                                 max_iterations, max_rounds, select_rounds, st, grp, ts, closing, stages);
}

// ---- the iterated search (difusco_tsp_iterated_search_ragged): descents of the search above with seeded segment kicks between
// them.  The rule is stated in include/difusco_hip.h and restated in numpy in tests/tsp_iterated_search_emulation.py.

__global__ __launch_bounds__(kSelectThreads) void mls_select_iterated_kernel(
    int* __restrict__ tours, const TourDesc* __restrict__ desc, const double* __restrict__ rowv_all, const int* __restrict__ rowj_all,
    int* __restrict__ live_all, int* __restrict__ winners_all, unsigned long long* __restrict__ tabv_all, int* __restrict__ tabi_all,
    int2* __restrict__ marks_all, int2* __restrict__ cum_all, long long max_iterations, int max_rounds, int select_rounds,
    MlState* st, MlGroup* grp, MlTourState* ts) {
  mls_select_tour<kSelectIterated>(tours, desc, rowv_all, rowj_all, live_all, winners_all, tabv_all, tabi_all, marks_all, cum_all,
                                   max_iterations, max_rounds, select_rounds, st, grp, ts);
}

}  // namespace
}  // namespace difusco

#include "or_opt_nbr.h"       // the row kernels of the listed search
#include "or_opt_heat.h"      // the heat-biased draws of the guided search: its kernels stand here, between the select and the
                              // keep / kick kernels

namespace difusco {
namespace {

struct MlIter {            // device-resident state of a tour of the iterated search, zero at the start of a call
  int kick, have;          // kicks drawn so far; the tour has an incumbent
  int kept, improved;      // kicks whose descent ended not longer / strictly shorter than the incumbent
  long long swapped;       // segment pairs swapped over all kicks
  int max_round, pad;      // the highest zero-based round of any descent
  double first_length, length;   // of the first descent's result, of the incumbent
};

// Wave 0: the draws of kick `kick` of tour t, one lane per draw c < kick_size - two segment lengths l1, l2 of at most `span`
// cities and the first cut a (kHeat: by the running weights of the incumbent, heat_pick), so that the draw swaps [a, a + l1) and
// [a + l1, b), b = a + l1 + l2 - and the disjointness filter in rising c: a draw is kept unless it meets a kept draw before it.
template <bool kHeat>
__device__ __forceinline__ void kick_draws(const unsigned long long* __restrict__ seeds, const unsigned long long* __restrict__ offsets,
                                           int t, int kick, int kick_size, int span, int n, long long closed, HeatArgs<kHeat> hx,
                                           int* ka, int* kl1, int* kb, int* kkeep) {
  const int c = threadIdx.x;
  const unsigned lc = (unsigned)span < (unsigned)(n - 1) / 2 ? (unsigned)span : (unsigned)(n - 1) / 2;
  int a = 0, b = 0, l1 = 0, keep = 0;
  if (c < kick_size) {
    uint32_t w[4];
    Philox::run(seeds[t], offsets[t] + (unsigned long long)kick, (uint64_t)c, w);
    l1 = 1 + (int)(w[1] % lc);
    const int l2 = 1 + (int)(w[2] % lc);
    if constexpr (kHeat)
      a = heat_pick(hx.W + closed, n - l1 - l2, w[0], w[3]);
    else
      a = 1 + (int)(w[0] % (unsigned)(n - l1 - l2));
    b = a + l1 + l2;
    keep = 1;
  }
  for (int e = 0; e < kick_size; ++e) {                          // lane e's flag is final when e comes up
    const int ae = __shfl(a, e), be = __shfl(b, e), ke = __shfl(keep, e);
    if (c > e && ke && a < be && ae < b) keep = 0;
  }
  ka[c] = a, kl1[c] = l1, kb[c] = b, kkeep[c] = keep;
}

// One block per tour, a no-op unless the tour's descent has just ended (phase kKeep).  Keep: the length of the descended tour C
// against the incumbent I (`inc`, n + 1 entries of the tour's own); I <- C if it is not longer (or there is no incumbent yet),
// else C <- I.  Kick, if kicks remain: the draws of kick t, the disjointness filter in rising c by wave 0, the kept draws swap
// their two adjacent segments in C reading I - a wave per draw -, and the descent state is reset.  Else the tour is done; C = I.
// kHeat: `a` of a draw comes from the running weights of I (heat_prefix, heat_pick), computed behind the keep copy.
template <bool kHeat>
__global__ __launch_bounds__(kSelectThreads) void mls_keep_kick_kernel(
    const double* __restrict__ points, int* __restrict__ tours, int* __restrict__ inc_all, const TourDesc* __restrict__ desc,
    const unsigned long long* __restrict__ seeds, const unsigned long long* __restrict__ offsets, int kicks, int kick_size,
    int span, int no_descent, MlState* st, MlGroup* grp, MlTourState* ts, MlIter* iters, HeatArgs<kHeat> hx) {
  const int t = blockIdx.x;
  if (ts[t].phase != kKeep) return;                              // written by thread 0 of this block at its end only
  const TourDesc d = desc[t];
  const int n = d.n;
  int* tour = tours + d.closed;
  int* inc = inc_all + d.closed;
  MlIter* it = iters + t;                                        // thread 0 alone writes it, at the end
  __shared__ double part[kLenParts];
  __shared__ int ka[kMaxKickSize], kl1[kMaxKickSize], kb[kMaxKickSize], kkeep[kMaxKickSize];
  const int have = it->have, kick = it->kick;                    // read before the barriers of tour_length
  const double inc_len = it->length;
  const double len = tour_length(points + d.points, tour, n, part);
  const bool take = !have || len <= inc_len;                     // uniform over the block
  if (take)
    for (int k = threadIdx.x; k <= n; k += kSelectThreads) inc[k] = tour[k];
  else
    for (int k = threadIdx.x; k <= n; k += kSelectThreads) tour[k] = inc[k];
  const bool more = kick < kicks;
  int nkept = 0;
  if (more) {
    if constexpr (kHeat) {
      __syncthreads();                                           // the copy above is complete
      const MlHeatTour h = hx.tab[t];
      heat_prefix(inc, n, hx.row_ptr + h.rows, hx.col + h.edges, hx.q + h.heat, hx.W + d.closed, (unsigned long long*)part);
    }
    if (threadIdx.x < 64) kick_draws<kHeat>(seeds, offsets, t, kick, kick_size, span, n, d.closed, hx, ka, kl1, kb, kkeep);
    __syncthreads();                                             // and the copy above is complete
    kick_swaps(tour, inc, kick_size, ka, kl1, kb, kkeep);
  }
  if (threadIdx.x == 0) {
    if (more)
      for (int c = 0; c < kick_size; ++c) nkept += kkeep[c];
    MlTourState* s = ts + t;
    if (!have) {
      it->have = 1;
      it->first_length = len;
    } else if (take) {
      it->kept += 1;
      if (len < inc_len) it->improved += 1;
    }
    if (take) it->length = len;
    if (s->round > it->max_round) it->max_round = s->round;
    if (more) {
      it->kick = kick + 1;
      it->swapped += nkept;
      s->phase = no_descent ? kKeep : kTwoOpt;
      s->round = 0;
      s->or_moved = 0;
      s->sweeps = 0;
    } else {
      s->phase = kDone;
      report_done(grp + d.group, st);
    }
  }
}

}  // namespace
}  // namespace difusco

#include "or_opt_focused.h"   // the focused search: its kernels, which use the types and device functions above

// ---- the host side: one workspace description (mls_layout, MlPtrs) and one driver (mls_run) behind the five entries

namespace difusco {
namespace {

enum MlPart : unsigned { kIterPart = 1, kFocusPart = 2, kHeatPart = 4, kListPart = 8 };   // the optional parts of a workspace

struct MlLayout {          // byte offsets; the optional parts follow the descent's in this order, an absent one is empty
  size_t desc, tp, dlen, rowv, rowj, live, winners, tabv, tabi, marks, cum, grp, ts, st;
  size_t pos, rowkey;                            // kListPart: the sections of nbr_rows.h, in front of grp; and MlStage, in `ts`
  size_t inc, iters;                             // kIterPart: the incumbents and MlIter
  size_t smark, tmark, arows, acols, foc, full;  // kFocusPart
  size_t W, q, htab, hgrp, bad;                  // kHeatPart
  size_t total;
  GroupTotals tot;
  int emax;                                      // the most edges of a group
};

struct MlTables {          // the host tables of a call
  std::vector<TourDesc> tours;
  std::vector<MlGroup> groups;
  std::vector<MlHeatTour> heat_tours;            // kHeatPart: a group's first row_ptr / col entry, a tour's first heat entry
  std::vector<MlHeatGroup> heat_groups;
};

// checks the group arrays (K and closing with kListPart, group_edges with kHeatPart) and lays out the workspace of a call that
// needs `parts`; `tabs` (optional) receives the tables
int mls_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, unsigned parts, int K, int closing,
               const int32_t* group_edges, MlLayout* L, MlTables* tabs) {
  *L = MlLayout{};
  const bool lists = parts & kListPart;
  const int rc = walk_groups(who, groups, group_n, group_tours, lists, K, closing, &L->tot, tabs ? &tabs->tours : nullptr);
  if (rc != DIFUSCO_OK) return rc;
  const bool heat = parts & kHeatPart;
  if (heat && !group_edges) return set_error(DIFUSCO_EINVAL, "%s: group_edges is null", who);
  for (int g = 0; heat && g < groups; ++g)
    if (group_edges[g] < 0) return set_error(DIFUSCO_EINVAL, "%s: group %d has %d edges", who, g, (int)group_edges[g]);
  size_t rows = 0, edges = 0, heats = 0;         // the group table and the heat bookkeeping: a walk of its own
  for (int g = 0; g < groups; ++g) {
    const int n = group_n[g], E = heat ? group_edges[g] : 0;
    L->emax = E > L->emax ? E : L->emax;
    if (tabs) tabs->groups.push_back(MlGroup{group_tours[g], 0});
    if (tabs && heat) tabs->heat_groups.push_back(MlHeatGroup{n, E, (long long)rows, (long long)edges});
    for (int p = 0; p < group_tours[g]; ++p) {
      if (tabs && heat) tabs->heat_tours.push_back(MlHeatTour{(long long)rows, (long long)edges, (long long)heats, n, E});
      heats += (size_t)E;
    }
    rows += (size_t)n + 1;
    edges += (size_t)E;
  }
  const GroupTotals& t = L->tot;
  const size_t T = t.tours;
  Sections s;
  L->desc = s.take(sizeof(TourDesc) * T);
  L->tp = s.take(sizeof(double2) * t.closed);
  L->dlen = s.take(sizeof(double) * t.cols);
  L->rowv = s.take(sizeof(double) * t.cols);
  L->rowj = s.take(sizeof(int) * t.cols);
  L->live = s.take(sizeof(int) * t.cols);
  L->winners = s.take(sizeof(int) * t.cols);
  L->tabv = s.take(sizeof(unsigned long long) * t.cells);
  L->tabi = s.take(sizeof(int) * t.cells);
  L->marks = s.take(sizeof(int2) * t.closed);
  L->cum = s.take(sizeof(int2) * t.closed);
  L->pos = s.take(sizeof(int) * t.cols, lists);
  L->rowkey = s.take(sizeof(unsigned long long) * t.cols, lists);
  L->grp = s.take(sizeof(MlGroup) * groups);
  L->ts = s.take((sizeof(MlTourState) + (lists ? sizeof(MlStage) : 0)) * T);     // with lists T MlStage behind T MlTourState
  L->st = s.take(sizeof(MlState));
  const bool iter = parts & kIterPart, focus = parts & kFocusPart;
  L->inc = s.take(sizeof(int) * t.closed, iter);
  L->iters = s.take(sizeof(MlIter) * T, iter);
  L->smark = s.take(sizeof(int) * t.cols, focus);
  L->tmark = s.take(sizeof(int) * t.cols, focus);
  L->arows = s.take(sizeof(int) * t.cols, focus);
  L->acols = s.take(sizeof(int) * t.cols, focus);
  L->foc = s.take(sizeof(MlFocus) * T, focus);
  L->full = s.take(sizeof(MlTourState) * T, focus);
  L->W = s.take(sizeof(unsigned long long) * t.closed, heat);
  L->q = s.take(sizeof(unsigned short) * heats, heat);
  L->htab = s.take(sizeof(MlHeatTour) * T, heat);
  L->hgrp = s.take(sizeof(MlHeatGroup) * groups, heat);
  L->bad = s.take(sizeof(int), heat);
  L->total = s.off;
  return DIFUSCO_OK;
}

// the five `_workspace_bytes` entries
int mls_workspace_bytes(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, unsigned parts, int K,
                        int closing, const int32_t* group_edges, size_t* bytes) {
  if (!bytes) return set_error(DIFUSCO_EINVAL, "%s: bytes is null", who);
  MlLayout lay;
  const int rc = mls_layout(who, groups, group_n, group_tours, parts, K, closing, group_edges, &lay, nullptr);
  if (rc == DIFUSCO_OK) *bytes = lay.total;
  return rc;
}

struct MlPtrs {            // the sections of a workspace; those of a part the layout does not hold are never read
  TourDesc* desc;
  double2* tp;
  double *dlen, *rowv;
  int *rowj, *live, *winners;
  unsigned long long* tabv;
  int* tabi;
  int2 *marks, *cum;
  MlGroup* grp;
  MlTourState* ts;
  MlState* st;
  MlStage* stages;
  int* pos;
  unsigned long long* rowkey;
  int* inc;
  MlIter* iters;
  int *smark, *tmark, *arows, *acols;
  MlFocus* foc;
  MlTourState* full;
  unsigned long long* W;
  unsigned short* q;
  MlHeatTour* htab;
  MlHeatGroup* hgrp;
  int* bad;
  MlPtrs(void* workspace, const MlLayout& L) {
    char* w = (char*)workspace;
    desc = (TourDesc*)(w + L.desc), tp = (double2*)(w + L.tp), dlen = (double*)(w + L.dlen), rowv = (double*)(w + L.rowv);
    rowj = (int*)(w + L.rowj), live = (int*)(w + L.live), winners = (int*)(w + L.winners);
    tabv = (unsigned long long*)(w + L.tabv), tabi = (int*)(w + L.tabi), marks = (int2*)(w + L.marks), cum = (int2*)(w + L.cum);
    grp = (MlGroup*)(w + L.grp), ts = (MlTourState*)(w + L.ts), st = (MlState*)(w + L.st);
    stages = (MlStage*)(ts + L.tot.tours), pos = (int*)(w + L.pos), rowkey = (unsigned long long*)(w + L.rowkey);
    inc = (int*)(w + L.inc), iters = (MlIter*)(w + L.iters);
    smark = (int*)(w + L.smark), tmark = (int*)(w + L.tmark), arows = (int*)(w + L.arows), acols = (int*)(w + L.acols);
    foc = (MlFocus*)(w + L.foc), full = (MlTourState*)(w + L.full);
    W = (unsigned long long*)(w + L.W), q = (unsigned short*)(w + L.q), htab = (MlHeatTour*)(w + L.htab);
    hgrp = (MlHeatGroup*)(w + L.hgrp), bad = (int*)(w + L.bad);
  }
};

thread_local int g_host_syncs = 0;   // host synchronisations of this thread's last iterated call (difusco_tsp_search_host_syncs)

// one descent; descents and kicks; focused descents after kicks; one descent that starts on neighbour lists
enum MlMode : int { kPlain = 0, kIterFull = 1, kIterFocused = 2, kListed = 3 };

struct MlCall {            // a call of one of the five entries
  const char* who;         // the entry, in front of every message
  MlMode mode;
  bool heat;               // the kicks are drawn by heat (the guided entry)
  unsigned parts;          // what the entry's workspace holds: the guided entry reserves the focus part for both descents
  const char* tour_outputs;   // how the entry's refusal names its per-tour output arrays
  int groups;
  const int32_t *group_n, *group_tours;
  const double* points;
  int32_t* tours;
  const int32_t* neighbors;                      // kListed, with K and closing
  int K, closing;
  int64_t max_iterations;
  int max_rounds, select_rounds;
  int32_t kicks, kick_size, span;                // from here to `heat_values`: the iterated modes
  const uint64_t *tour_seeds, *tour_offsets;
  int32_t compact_select_max;                    // kIterFocused
  const int32_t *group_edges, *row_ptr, *col;    // heat
  const float* heat_values;
  void* workspace;
  size_t workspace_bytes;
  int64_t *two_opt_sweeps_out, *or_opt_sweeps_out;
  int32_t* rounds_out;
  int64_t *two_opt_moves_out, *or_opt_moves_out;
  int64_t* full_sweeps_out;                      // kListed: the two counters of the full stage, [groups]
  int32_t* full_rounds_out;
  int32_t *kicks_kept_out, *kicks_improved_out;  // the per-tour outputs: the iterated modes
  int64_t* segments_swapped_out;
  double *first_length_out, *final_length_out;
  int32_t* closing_sweeps_out;                   // kIterFocused; with heat and a full descent optional, written as 0
  int64_t* tour_sweeps_out;                      // optional, [tours]: the sweeps in which the tour moved (the window search)
  void* stream;
};

// the keep / kick step of every tour: the kernel of the descent, its instantiation of the draws
template <bool kHeat>
void mls_launch_keep_kick(const MlCall& c, const MlPtrs& p, int T, int no_descent, HeatArgs<kHeat> hx) {
  hipStream_t s = (hipStream_t)c.stream;
  const unsigned long long* seeds = (const unsigned long long*)c.tour_seeds;
  const unsigned long long* offsets = (const unsigned long long*)c.tour_offsets;
  if (c.mode == kIterFocused)
    hipLaunchKernelGGL(mls_keep_kick_focused_kernel<kHeat>, dim3(T), dim3(kSelectThreads), 0, s, c.points, c.tours, p.inc, p.desc,
                       seeds, offsets, (int)c.kicks, (int)c.kick_size, (int)c.span, no_descent, p.st, p.grp, p.ts, p.iters, p.full,
                       p.foc, p.marks, p.cum, p.smark, p.tmark, p.arows, p.acols, hx);
  else
    hipLaunchKernelGGL(mls_keep_kick_kernel<kHeat>, dim3(T), dim3(kSelectThreads), 0, s, c.points, c.tours, p.inc, p.desc, seeds,
                       offsets, (int)c.kicks, (int)c.kick_size, (int)c.span, no_descent, p.st, p.grp, p.ts, p.iters, hx);
}

// The five entries.  Checks the arguments, sets the device state up, enqueues launch sequences - a sweep of every tour that is
// still descending and, in the iterated modes, the keep / kick step - until every group has stopped, and reduces the tours'
// counters to the outputs.
int mls_run(const MlCall& c) {
  // plain: one descent, no keep / kick step - on full rows, or (listed) with a neighbour stage in front of them
  const bool listed = c.mode == kListed, plain = listed || c.mode == kPlain, focused = c.mode == kIterFocused;
  const int groups = c.groups;
  if (!plain) g_host_syncs = 0;
  MlLayout lay;
  MlTables tabs;
  const int rc = mls_layout(c.who, groups, c.group_n, c.group_tours, c.parts, c.K, c.closing, c.group_edges, &lay, &tabs);
  if (rc != DIFUSCO_OK) return rc;
  if (listed && !c.neighbors) return set_error(DIFUSCO_EINVAL, "%s: neighbors is null", c.who);
  if (!c.points || !c.tours || !c.workspace || !c.two_opt_sweeps_out || !c.or_opt_sweeps_out || !c.rounds_out ||
      !c.two_opt_moves_out || !c.or_opt_moves_out || (listed && (!c.full_sweeps_out || !c.full_rounds_out)) || c.max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "%s: needs non-null device arrays, the %s host output arrays [groups] and "
                                     "max_iterations >= 0", c.who, listed ? "seven" : "five");
  if (!plain && (!c.tour_seeds || !c.tour_offsets || !c.kicks_kept_out || !c.kicks_improved_out || !c.segments_swapped_out ||
                 !c.first_length_out || !c.final_length_out || (focused && !c.closing_sweeps_out)))
    return set_error(DIFUSCO_EINVAL, "%s: needs the device arrays tour_seeds / tour_offsets and %s", c.who, c.tour_outputs);
  if (c.max_rounds < 1) return set_error(DIFUSCO_EINVAL, "%s: max_rounds = %d, needs at least 1", c.who, c.max_rounds);
  if (c.select_rounds < 1) return set_error(DIFUSCO_EINVAL, "%s: select_rounds = %d, needs at least 1", c.who, c.select_rounds);
  if (!plain) {
    if (c.kicks < 0) return set_error(DIFUSCO_EINVAL, "%s: kicks = %d < 0", c.who, (int)c.kicks);
    if (c.kick_size < 1 || c.kick_size > kMaxKickSize)
      return set_error(DIFUSCO_EINVAL, "%s: kick_size = %d, needs 1 .. %d", c.who, (int)c.kick_size, kMaxKickSize);
    if (c.span < 1) return set_error(DIFUSCO_EINVAL, "%s: span = %d < 1", c.who, (int)c.span);
  }
  if (focused && (c.compact_select_max < 0 || c.compact_select_max > kCompactMax))
    return set_error(DIFUSCO_EINVAL, "%s: compact_select_max = %d, needs 0 .. %d", c.who, (int)c.compact_select_max, kCompactMax);
  if (c.workspace_bytes < lay.total)
    return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", c.who, c.workspace_bytes, lay.total);
  for (int g = 0; g < groups; ++g) {
    c.two_opt_sweeps_out[g] = c.or_opt_sweeps_out[g] = c.two_opt_moves_out[g] = c.or_opt_moves_out[g] = 0;
    c.rounds_out[g] = 1;                                         // every descent starts round 1
    if (listed) c.full_sweeps_out[g] = 0, c.full_rounds_out[g] = 0;
  }
  // no sweep may move a tour.  One descent: nothing is applied; the iterated modes: a call of keeps and kicks only
  const int no_descent = c.max_iterations == 0;
  if (plain && no_descent) return DIFUSCO_OK;
  const MlPtrs p(c.workspace, lay);
  const HeatArgs<true> hx{c.row_ptr, c.col, p.q, p.htab, p.W};
  hipStream_t s = (hipStream_t)c.stream;
  const int T = lay.tot.tours;
  std::vector<MlTourState> states(T);                            // zero; with no descent every tour starts at its keep step
  for (int b = 0; b < T; ++b) states[b].phase = no_descent ? kKeep : kTwoOpt;
  int bad = 0;
  // the tables, once per call; the host vectors live until the synchronisation below
  hipError_t er = hipMemcpyAsync(p.desc, tabs.tours.data(), sizeof(TourDesc) * T, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemcpyAsync(p.grp, tabs.groups.data(), sizeof(MlGroup) * groups, hipMemcpyHostToDevice, s);
  if (plain) {
    if (er == hipSuccess) er = hipMemsetAsync(p.ts, 0, lay.total - lay.ts, s);   // ts .. st, the end of this workspace
  } else {
    if (er == hipSuccess) er = hipMemsetAsync(p.st, 0, sizeof(MlState), s);
    if (er == hipSuccess) er = hipMemsetAsync(p.iters, 0, sizeof(MlIter) * T, s);
    if (er == hipSuccess) er = hipMemcpyAsync(p.ts, states.data(), sizeof(MlTourState) * T, hipMemcpyHostToDevice, s);
  }
  if (focused) {                                                 // every tour starts in its first, full descent
    if (er == hipSuccess) er = hipMemsetAsync(p.foc, 0, sizeof(MlFocus) * T, s);
    if (er == hipSuccess) er = hipMemcpyAsync(p.full, states.data(), sizeof(MlTourState) * T, hipMemcpyHostToDevice, s);
  }
  if (c.heat) {              // the graph tables and the check of the graphs, in front of the setup synchronisation
    if (er == hipSuccess) er = hipMemcpyAsync(p.htab, tabs.heat_tours.data(), sizeof(MlHeatTour) * T, hipMemcpyHostToDevice, s);
    if (er == hipSuccess)
      er = hipMemcpyAsync(p.hgrp, tabs.heat_groups.data(), sizeof(MlHeatGroup) * groups, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipMemsetAsync(p.bad, 0, sizeof(int), s);
    if (er == hipSuccess) {
      const long long longest = (long long)lay.tot.nmax + 1 > lay.emax ? (long long)lay.tot.nmax + 1 : lay.emax;
      hipLaunchKernelGGL(heat_graph_check_kernel, dim3((unsigned)((longest + 255) / 256), groups), dim3(256), 0, s, c.row_ptr, c.col,
                         p.hgrp, p.bad);
      er = hipMemcpyAsync(&bad, p.bad, sizeof(int), hipMemcpyDeviceToHost, s);
    }
  }
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (!plain) ++g_host_syncs;
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s setup: %s", c.who, hipGetErrorString(er));
  if (bad)
    return set_error(DIFUSCO_EINVAL, "%s: a group's graph is not a CSR over its cities (row_ptr[0] = 0, row_ptr rising to "
                                     "row_ptr[n] = edges, 0 <= col < n)", c.who);
  if (c.heat && lay.emax > 0)                                    // the q table of every tour, once per call, in stream order
    hipLaunchKernelGGL(heat_table_kernel, dim3((unsigned)(((long long)lay.emax + 255) / 256), T), dim3(256), 0, s, c.row_ptr, c.col,
                       c.heat_values, p.htab, p.q);
  // A launch sequence either moves a tour (at most max_iterations per descent), ends one of its phases (two per round) - in the
  // iterated modes the last of them runs the keep / kick step -, or, with no descent, is one keep / kick step: the bound per
  // descent.  Listed, two more end phases: those of the round in which the tour goes on to the full stage.  A tour runs its first
  // descent, one per kick and, focused, the closing one.
  const long long ends = 2LL * c.max_rounds + (listed ? 2 : 0);
  const long long per = no_descent ? 1 : (c.max_iterations > INT64_MAX - ends ? INT64_MAX : c.max_iterations + ends);
  const long long descents = plain ? 1 : (long long)c.kicks + (focused ? 2 : 1);
  const long long limit = per > INT64_MAX / descents ? INT64_MAX : per * descents;
  const int split = lay.tot.nmax;                                // blocks of the row part: the list holds at most n - 1 rows
  const dim3 prep_grid((lay.tot.nmax + 1 + 255) / 256, T), best_grid(lay.tot.nblk_or, T), focus_grid(split + lay.tot.nblk_or, T);
  const dim3 walk_grid((unsigned)(((long long)lay.tot.nmax * c.K + 255) / 256), T);   // listed: a thread per (position, list slot)
  const long long cap = (long long)c.max_iterations;
  const auto select_kernel = plain ? mls_select_kernel : mls_select_iterated_kernel;
  const Polled polled = poll_launches(limit, plain ? 4 : 8, groups, &p.st->done, s, [&] {
    if (listed) {            // the rows of the neighbour stage, with closing also those of the full stage, and the select step
      hipLaunchKernelGGL(nls_prep_kernel, prep_grid, dim3(256), 0, s, c.points, c.tours, p.desc, p.tp, p.dlen, p.pos, p.rowkey, p.rowj,
                         p.ts);
      hipLaunchKernelGGL(nls_row_value_kernel, walk_grid, dim3(256), 0, s, c.tours, c.neighbors, p.desc, p.tp, p.dlen, p.pos, c.K,
                         p.rowkey, p.ts);
      hipLaunchKernelGGL(nls_row_col_kernel, walk_grid, dim3(256), 0, s, c.tours, c.neighbors, p.desc, p.tp, p.dlen, p.pos, c.K,
                         p.rowkey, p.rowv, p.rowj, p.ts);
      if (c.closing) {
        hipLaunchKernelGGL(nls_full_two_kernel, best_grid, dim3(256), 0, s, p.tp, p.dlen, p.desc, p.rowv, p.rowj, p.ts);
        hipLaunchKernelGGL(nls_full_or_kernel, best_grid, dim3(256), 0, s, p.tp, p.dlen, p.desc, p.rowv, p.rowj, p.ts);
      }
      hipLaunchKernelGGL(mls_select_listed_kernel, dim3(T), dim3(kSelectThreads), 0, s, c.tours, p.desc, p.rowv, p.rowj, p.live,
                         p.winners, p.tabv, p.tabi, p.marks, p.cum, cap, c.max_rounds, c.select_rounds, c.closing, p.st, p.grp, p.ts,
                         p.stages);
    } else if (!no_descent) {
      hipLaunchKernelGGL(mls_prep_kernel, prep_grid, dim3(256), 0, s, c.points, c.tours, p.desc, p.tp, p.dlen, p.ts);
      // a focused tour reads kDone in `full`: the full sweep skips it, the focused one takes it
      hipLaunchKernelGGL(mls_row_best_kernel, best_grid, dim3(256), 0, s, p.tp, p.dlen, p.desc, p.rowv, p.rowj, focused ? p.full : p.ts);
      if (focused) {
        hipLaunchKernelGGL(mls_focused_row_best_kernel, focus_grid, dim3(256), 0, s, p.tp, p.dlen, p.desc, p.rowv, p.rowj, p.ts,
                           p.foc, p.arows, p.acols, p.marks, split);
        hipLaunchKernelGGL(mls_select_focused_kernel, dim3(T), dim3(kSelectThreads), 0, s, c.tours, p.desc, p.rowv, p.rowj, p.live,
                           p.winners, p.tabv, p.tabi, p.marks, p.cum, cap, c.max_rounds, c.select_rounds, (int)c.compact_select_max,
                           p.st, p.grp, p.ts, p.full, p.foc, p.smark, p.tmark, p.arows, p.acols);
      } else {
        hipLaunchKernelGGL(select_kernel, dim3(T), dim3(kSelectThreads), 0, s, c.tours,
                           p.desc, p.rowv, p.rowj, p.live, p.winners, p.tabv, p.tabi, p.marks, p.cum, cap, c.max_rounds,
                           c.select_rounds, p.st, p.grp, p.ts);
      }
    }
    if (!plain && c.heat) mls_launch_keep_kick<true>(c, p, T, no_descent, hx);
    if (!plain && !c.heat) mls_launch_keep_kick<false>(c, p, T, no_descent, HeatArgs<false>{});
  });
  if (!plain) g_host_syncs += polled.syncs;
  if (polled.status != hipSuccess) return set_error(DIFUSCO_EHIP, "%s state: %s", c.who, hipGetErrorString(polled.status));
  std::vector<MlIter> its(plain ? 0 : T);
  std::vector<MlFocus> focs(focused ? T : 0);
  std::vector<MlStage> stages(listed ? T : 0);
  er = hipMemcpyAsync(states.data(), p.ts, sizeof(MlTourState) * T, hipMemcpyDeviceToHost, s);
  if (listed && er == hipSuccess) er = hipMemcpyAsync(stages.data(), p.stages, sizeof(MlStage) * T, hipMemcpyDeviceToHost, s);
  if (!plain && er == hipSuccess) er = hipMemcpyAsync(its.data(), p.iters, sizeof(MlIter) * T, hipMemcpyDeviceToHost, s);
  if (focused && er == hipSuccess) er = hipMemcpyAsync(focs.data(), p.foc, sizeof(MlFocus) * T, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (!plain) ++g_host_syncs;
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s counters: %s", c.who, hipGetErrorString(er));
  for (int b = 0; b < T; ++b) {
    const int g = tabs.tours[b].group;
    const MlTourState& x = states[b];
    const int rounds = (plain ? x.round : its[b].max_round) + 1;
    if (x.two_opt_sweeps > c.two_opt_sweeps_out[g]) c.two_opt_sweeps_out[g] = x.two_opt_sweeps;
    if (x.or_opt_sweeps > c.or_opt_sweeps_out[g]) c.or_opt_sweeps_out[g] = x.or_opt_sweeps;
    if (rounds > c.rounds_out[g]) c.rounds_out[g] = rounds;
    c.two_opt_moves_out[g] += x.two_opt_moves;
    c.or_opt_moves_out[g] += x.or_opt_moves;
    if (c.tour_sweeps_out) c.tour_sweeps_out[b] = x.sweeps;
    if (listed && stages[b].full_sweeps > c.full_sweeps_out[g]) c.full_sweeps_out[g] = stages[b].full_sweeps;
    if (listed && stages[b].full_rounds > c.full_rounds_out[g]) c.full_rounds_out[g] = stages[b].full_rounds;
    if (plain) continue;
    c.kicks_kept_out[b] = its[b].kept;
    c.kicks_improved_out[b] = its[b].improved;
    c.segments_swapped_out[b] = its[b].swapped;
    c.first_length_out[b] = its[b].first_length;
    c.final_length_out[b] = its[b].length;
    if (c.closing_sweeps_out) c.closing_sweeps_out[b] = focused ? focs[b].closing_sweeps : 0;
  }
  return DIFUSCO_OK;
}

// the arguments the three iterated entries share, as they pass them
int mls_iterated_entry(const char* who, MlMode mode, bool heat, unsigned parts, const char* tour_outputs, int groups,
                       const int32_t* group_n, const int32_t* group_tours, const double* points, int32_t* tours,
                       int64_t max_iterations, int max_rounds, int select_rounds, int32_t kicks, int32_t kick_size, int32_t span,
                       const uint64_t* tour_seeds, const uint64_t* tour_offsets, int32_t compact_select_max,
                       const int32_t* group_edges, const int32_t* row_ptr, const int32_t* col, const float* heat_values,
                       void* workspace, size_t workspace_bytes, int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out,
                       int32_t* rounds_out, int64_t* two_opt_moves_out, int64_t* or_opt_moves_out, int32_t* kicks_kept_out,
                       int32_t* kicks_improved_out, int64_t* segments_swapped_out, double* first_length_out,
                       double* final_length_out, int32_t* closing_sweeps_out, void* stream) {
  MlCall c{};
  c.who = who, c.mode = mode, c.heat = heat, c.parts = parts, c.tour_outputs = tour_outputs;
  c.groups = groups, c.group_n = group_n, c.group_tours = group_tours, c.points = points, c.tours = tours;
  c.max_iterations = max_iterations, c.max_rounds = max_rounds, c.select_rounds = select_rounds;
  c.kicks = kicks, c.kick_size = kick_size, c.span = span, c.tour_seeds = tour_seeds, c.tour_offsets = tour_offsets;
  c.compact_select_max = compact_select_max;
  c.group_edges = group_edges, c.row_ptr = row_ptr, c.col = col, c.heat_values = heat_values;
  c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = stream;
  c.two_opt_sweeps_out = two_opt_sweeps_out, c.or_opt_sweeps_out = or_opt_sweeps_out, c.rounds_out = rounds_out;
  c.two_opt_moves_out = two_opt_moves_out, c.or_opt_moves_out = or_opt_moves_out;
  c.kicks_kept_out = kicks_kept_out, c.kicks_improved_out = kicks_improved_out, c.segments_swapped_out = segments_swapped_out;
  c.first_length_out = first_length_out, c.final_length_out = final_length_out, c.closing_sweeps_out = closing_sweeps_out;
  return mls_run(c);
}

}  // namespace

// the descent of difusco_tsp_multi_local_search_ragged for the window search (tsp_window_search.hip, declared in kernels.h): the
// messages name `who`, and tour_sweeps_out (HOST [tours], optional) receives the sweeps in which every tour moved
int mls_descent_workspace_bytes(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes) {
  return mls_workspace_bytes(who, groups, group_n, group_tours, 0, 0, 0, nullptr, bytes);
}

int mls_descent(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                int32_t* tours, int64_t max_iterations, int max_rounds, int select_rounds, void* workspace, size_t workspace_bytes,
                int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out, int32_t* rounds_out, int64_t* two_opt_moves_out,
                int64_t* or_opt_moves_out, int64_t* tour_sweeps_out, void* stream) {
  MlCall c{};
  c.who = who, c.mode = kPlain, c.parts = 0;
  c.groups = groups, c.group_n = group_n, c.group_tours = group_tours, c.points = points, c.tours = tours;
  c.max_iterations = max_iterations, c.max_rounds = max_rounds, c.select_rounds = select_rounds;
  c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = stream;
  c.two_opt_sweeps_out = two_opt_sweeps_out, c.or_opt_sweeps_out = or_opt_sweeps_out, c.rounds_out = rounds_out;
  c.two_opt_moves_out = two_opt_moves_out, c.or_opt_moves_out = or_opt_moves_out, c.tour_sweeps_out = tour_sweeps_out;
  return mls_run(c);
}

void tsp_search_set_host_syncs(int count) { g_host_syncs = count; }

}  // namespace difusco

extern "C" {

int difusco_tsp_multi_local_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours,
                                                          size_t* bytes) {
  return difusco::mls_workspace_bytes("multi_local_search_ragged_workspace_bytes", groups, group_n, group_tours, 0, 0, 0, nullptr, bytes);
}

int difusco_tsp_multi_local_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                          int32_t* tours, int64_t max_iterations, int max_rounds, int select_rounds, void* workspace,
                                          size_t workspace_bytes, int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out,
                                          int32_t* rounds_out, int64_t* two_opt_moves_out, int64_t* or_opt_moves_out, void* stream) {
  return difusco::mls_descent("tsp_multi_local_search_ragged", groups, group_n, group_tours, points, tours, max_iterations, max_rounds,
                              select_rounds, workspace, workspace_bytes, two_opt_sweeps_out, or_opt_sweeps_out, rounds_out,
                              two_opt_moves_out, or_opt_moves_out, nullptr, stream);
}

int difusco_tsp_nbr_local_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int K,
                                                        int closing, size_t* bytes) {
  using namespace difusco;
  return mls_workspace_bytes("nbr_local_search_ragged_workspace_bytes", groups, group_n, group_tours, kListPart, K, closing, nullptr,
                             bytes);
}

int difusco_tsp_nbr_local_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                        int32_t* tours, const int32_t* neighbors, int K, int closing, int64_t max_iterations,
                                        int max_rounds, int select_rounds, void* workspace, size_t workspace_bytes,
                                        int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out, int32_t* rounds_out,
                                        int64_t* two_opt_moves_out, int64_t* or_opt_moves_out, int64_t* full_sweeps_out,
                                        int32_t* full_rounds_out, void* stream) {
  using namespace difusco;
  MlCall c{};
  c.who = "tsp_nbr_local_search_ragged", c.mode = kListed, c.parts = kListPart;
  c.groups = groups, c.group_n = group_n, c.group_tours = group_tours, c.points = points, c.tours = tours;
  c.neighbors = neighbors, c.K = K, c.closing = closing;
  c.max_iterations = max_iterations, c.max_rounds = max_rounds, c.select_rounds = select_rounds;
  c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = stream;
  c.two_opt_sweeps_out = two_opt_sweeps_out, c.or_opt_sweeps_out = or_opt_sweeps_out, c.rounds_out = rounds_out;
  c.two_opt_moves_out = two_opt_moves_out, c.or_opt_moves_out = or_opt_moves_out;
  c.full_sweeps_out = full_sweeps_out, c.full_rounds_out = full_rounds_out;
  return mls_run(c);
}

int difusco_tsp_iterated_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours,
                                                       size_t* bytes) {
  using namespace difusco;
  return mls_workspace_bytes("tsp_iterated_search_ragged_workspace_bytes", groups, group_n, group_tours, kIterPart, 0, 0, nullptr, bytes);
}

int difusco_tsp_search_host_syncs(void) { return difusco::g_host_syncs; }

int difusco_tsp_focused_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours,
                                                      size_t* bytes) {
  using namespace difusco;
  return mls_workspace_bytes("tsp_focused_search_ragged_workspace_bytes", groups, group_n, group_tours, kIterPart | kFocusPart,
                             0, 0, nullptr, bytes);
}

int difusco_tsp_guided_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours,
                                                     const int32_t* group_edges, size_t* bytes) {
  using namespace difusco;
  return mls_workspace_bytes("tsp_guided_search_ragged_workspace_bytes", groups, group_n, group_tours,
                             kIterPart | kFocusPart | kHeatPart, 0, 0, group_edges, bytes);   // one size for both descents
}

int difusco_tsp_iterated_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                       int32_t* tours, int64_t max_iterations, int max_rounds, int select_rounds, int32_t kicks,
                                       int32_t kick_size, int32_t span, const uint64_t* tour_seeds, const uint64_t* tour_offsets,
                                       void* workspace, size_t workspace_bytes, int64_t* two_opt_sweeps_out,
                                       int64_t* or_opt_sweeps_out, int32_t* rounds_out, int64_t* two_opt_moves_out,
                                       int64_t* or_opt_moves_out, int32_t* kicks_kept_out, int32_t* kicks_improved_out,
                                       int64_t* segments_swapped_out, double* first_length_out, double* final_length_out,
                                       void* stream) {
  using namespace difusco;
  return mls_iterated_entry("tsp_iterated_search_ragged", kIterFull, false, kIterPart, "the five host output arrays [tours]", groups,
                            group_n, group_tours, points, tours, max_iterations, max_rounds, select_rounds, kicks, kick_size, span,
                            tour_seeds, tour_offsets, 0, nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes,
                            two_opt_sweeps_out, or_opt_sweeps_out, rounds_out, two_opt_moves_out, or_opt_moves_out, kicks_kept_out,
                            kicks_improved_out, segments_swapped_out, first_length_out, final_length_out, nullptr, stream);
}

int difusco_tsp_focused_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                      int32_t* tours, int64_t max_iterations, int max_rounds, int select_rounds, int32_t kicks,
                                      int32_t kick_size, int32_t span, const uint64_t* tour_seeds, const uint64_t* tour_offsets,
                                      int32_t compact_select_max, void* workspace, size_t workspace_bytes,
                                      int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out, int32_t* rounds_out,
                                      int64_t* two_opt_moves_out, int64_t* or_opt_moves_out, int32_t* kicks_kept_out,
                                      int32_t* kicks_improved_out, int64_t* segments_swapped_out, double* first_length_out,
                                      double* final_length_out, int32_t* closing_sweeps_out, void* stream) {
  using namespace difusco;
  return mls_iterated_entry("tsp_focused_search_ragged", kIterFocused, false, kIterPart | kFocusPart,
                            "the six host output arrays [tours]", groups, group_n, group_tours, points, tours, max_iterations,
                            max_rounds, select_rounds, kicks, kick_size, span, tour_seeds, tour_offsets, compact_select_max, nullptr,
                            nullptr, nullptr, nullptr, workspace, workspace_bytes, two_opt_sweeps_out, or_opt_sweeps_out, rounds_out,
                            two_opt_moves_out, or_opt_moves_out, kicks_kept_out, kicks_improved_out, segments_swapped_out,
                            first_length_out, final_length_out, closing_sweeps_out, stream);
}

// either of the two above with heat-drawn kicks; the workspace holds the focus part for both descents
int difusco_tsp_guided_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                     int32_t* tours, int64_t max_iterations, int max_rounds, int select_rounds, int32_t kicks,
                                     int32_t kick_size, int32_t span, const uint64_t* tour_seeds, const uint64_t* tour_offsets,
                                     int32_t compact_select_max, int32_t descent, const int32_t* group_edges,
                                     const int32_t* row_ptr, const int32_t* col, const float* heat, void* workspace,
                                     size_t workspace_bytes, int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out,
                                     int32_t* rounds_out, int64_t* two_opt_moves_out, int64_t* or_opt_moves_out,
                                     int32_t* kicks_kept_out, int32_t* kicks_improved_out, int64_t* segments_swapped_out,
                                     double* first_length_out, double* final_length_out, int32_t* closing_sweeps_out,
                                     void* stream) {
  using namespace difusco;
  if (descent != 0 && descent != 1)
    return set_error(DIFUSCO_EINVAL, "tsp_guided_search_ragged: descent = %d, needs 0 (full) or 1 (focused)", (int)descent);
  if (!group_edges || !row_ptr || !col || !heat)
    return set_error(DIFUSCO_EINVAL, "tsp_guided_search_ragged: needs group_edges and the device arrays row_ptr / col / heat");
  return mls_iterated_entry("tsp_guided_search_ragged", descent == 1 ? kIterFocused : kIterFull, true,
                            kIterPart | kFocusPart | kHeatPart,
                            "the host output arrays [tours] (closing_sweeps_out when the descent is focused)", groups, group_n,
                            group_tours, points, tours, max_iterations, max_rounds, select_rounds, kicks, kick_size, span, tour_seeds,
                            tour_offsets, compact_select_max, group_edges, row_ptr, col, heat, workspace, workspace_bytes,
                            two_opt_sweeps_out, or_opt_sweeps_out, rounds_out, two_opt_moves_out, or_opt_moves_out, kicks_kept_out,
                            kicks_improved_out, segments_swapped_out, first_length_out, final_length_out, closing_sweeps_out, stream);
}

}  // extern "C"
