// Local search of decoded tours: rounds of (2-opt phase, Or-opt phase) per group (difusco_tsp_local_search_ragged).
//
// The 2-opt phase is difusco_tsp_two_opt on the group's tours: the same prep entry, sweep (best_tile), argmin and reversal, from
// two_opt_common.h.  The Or-opt phase moves a segment of L = 1..3 cities, positions i+1 .. i+L of the closed tour (0 <= i <=
// n-1-L: positions 0 and n never move), between P_j and P_j+1 (0 <= j <= n-1, j outside [i, i+L]), forwards or reversed.
// Variant v of [(1, fwd), (2, fwd), (2, rev), (3, fwd), (3, rev)], (a, b) = (P_i+1, P_i+L) forwards and swapped when reversed:
//   add   = (|P_i P_i+L+1| + |P_j a|) + |b P_j+1|        float64, left to right, distances as dist2d
//   rem   = (d_i + d_i+L) + d_j
//   delta = add - rem
// A tour's best move is the lowest delta, ties to the lowest flat index (v n + i) n + j; it is applied if delta < -1e-6.  Every
// tour of a group applies its own best move per iteration; an iteration counts if a tour of the group moved; the phase ends after
// an iteration without a move or after max_iterations counted ones.  A round that applies no Or-opt move ends the group.
//
// One iteration is three launches, whatever the phases of the groups:
//   local_search_prep_kernel    tp / dlen of every tour of a running group (prep_entry);
//   local_search_best_kernel    one block per (row tile, tour): best_tile in the 2-opt phase, or_opt_tile in the Or-opt phase;
//   local_search_apply_kernel   one block per group: argmin per tour, the phase's stop test, the moves, the counters and the
//                               switch of phase, round and done flag - all on the device, the host polls a counter of stopped
//                               groups every few iterations.
// or_opt_tile: a thread keeps its columns (P_j, P_j+1, d_j) in registers, as in best_tile, and walks the rows i of the tile
// upwards.  Row i needs |P_j P_i+1|, |P_j P_i+2|, |P_j P_i+3| and the same three from P_j+1; row i + 1 needs two of each again, so
// only |P_j P_i+4| and |P_j+1 P_i+4| are new: two square roots per (i, j) for all five variants.  dist2d squares its
// differences, so |pq| and |qp| are the same bits and a carried value is the value the formula asks for.  The terms that
// depend on the row alone (|P_i P_i+L+1|, d_i + d_i+L) are computed once per tile into LDS.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"
#include "or_opt_move.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

struct LsTour {            // 40 bytes; offsets in elements of the array they index
  int n, nblk;
  long long points;        // the group's first coordinate in `points` (doubles)
  long long closed;        // the tour's first entry in tours, tp and stage (n + 1 per tour)
  long long cols;          //                       in dlen (n per tour)
  long long partial;       //                       in partial (nblk per tour)
};

struct LsGroup {           // the tours of a group: desc[first .. first + count - 1], all of n nodes and nblk partials
  int first, count, n, nblk;
  long long closed, partial;   // tour p of the group starts at closed + p (n + 1) and partial + p nblk
};

struct LsGroupState {      // device-resident loop state of a group, zero at the start of a call
  int phase, round;        // round: zero-based
  long long phase_iterations, two_opt_iterations, or_opt_iterations;
};

struct LsState {
  int done;                // groups that have stopped
  int pad;
};

__global__ void local_search_prep_kernel(const double* __restrict__ points, const int* __restrict__ tours,
                                         const LsTour* __restrict__ desc, double2* __restrict__ tp, double* __restrict__ dlen,
                                         const int* __restrict__ tphase) {
  const LsTour d = desc[blockIdx.y];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > d.n || tphase[blockIdx.y] == kDone) return;
  prep_entry(points + d.points, tours + d.closed, d.n, k, tp + d.closed, dlen + d.cols);
}

// one block of the Or-opt sweep: rows i0 .. i0 + TI - 1 of the tour (P = its tp, D = its dlen, n nodes) against every column;
// returns the block's best move in thread 0, flat index (v n + i) n + j.  Like best_tile it starts from (0.0, 0): a move is
// only applied below the threshold, so a tour without an improving candidate applies nothing.
__device__ __forceinline__ Best or_opt_tile(const double2* __restrict__ P, const double* __restrict__ D, int n, int i0) {
  __shared__ double2 pr[TI + LMAX + 1];    // P_i0 .. P_i0+TI+3, the index clipped to n
  __shared__ double closing[LMAX][TI];     // |P_i P_i+L+1|
  __shared__ double removed[LMAX][TI];     // d_i + d_i+L
  for (int t = threadIdx.x; t < TI + LMAX + 1; t += blockDim.x) pr[t] = P[i0 + t < n ? i0 + t : n];
  for (int t = threadIdx.x; t < LMAX * TI; t += blockDim.x) {
    const int r = t % TI, L = t / TI + 1, i = i0 + r;
    double c = 0.0, d = 0.0;
    if (i <= n - 1 - L) {
      const double2 p = P[i], q = P[i + L + 1];
      c = dist2d(p.x - q.x, p.y - q.y);
      d = __dadd_rn(D[i], D[i + L]);
    }
    closing[L - 1][r] = c;
    removed[L - 1][r] = d;
  }
  __syncthreads();
  Best best{0.0, 0};
  const int rows = (n - 1 - i0) < TI ? (n - 1 - i0) : TI;       // i <= n - 2: the last row of L = 1
  const long long nn = (long long)n * n;
  for (int jbase = 0; jbase < n; jbase += 256 * JPT) {
    double2 pj[JPT], pj1[JPT];
    double dj[JPT], e1[JPT], e2[JPT], e3[JPT], f1[JPT], f2[JPT], f3[JPT];   // e_k = |P_j P_i+k|, f_k = |P_j+1 P_i+k|
    int jj[JPT];
#pragma unroll
    for (int u = 0; u < JPT; ++u) {
      const int j = jbase + u * 256 + threadIdx.x, jc = j < n ? j : n - 1;
      jj[u] = j;
      pj[u] = P[jc];
      pj1[u] = P[jc + 1];
      dj[u] = D[jc];
      e1[u] = dist2d(pj[u].x - pr[1].x, pj[u].y - pr[1].y);
      e2[u] = dist2d(pj[u].x - pr[2].x, pj[u].y - pr[2].y);
      e3[u] = dist2d(pj[u].x - pr[3].x, pj[u].y - pr[3].y);
      f1[u] = dist2d(pj1[u].x - pr[1].x, pj1[u].y - pr[1].y);
      f2[u] = dist2d(pj1[u].x - pr[2].x, pj1[u].y - pr[2].y);
      f3[u] = dist2d(pj1[u].x - pr[3].x, pj1[u].y - pr[3].y);
    }
    for (int r = 0; r < rows; ++r) {
      const int i = i0 + r;
      const double c1 = closing[0][r], c2 = closing[1][r], c3 = closing[2][r];
      const double r1 = removed[0][r], r2 = removed[1][r], r3 = removed[2][r];
      const double2 next = pr[r + LMAX + 1];                    // P_i+4, for the row after this one
      const bool row2 = i <= n - 3, row3 = i <= n - 4;
#pragma unroll
      for (int u = 0; u < JPT; ++u) {
        const int j = jj[u];
        // delta = ((|P_i P_i+L+1| + |P_j a|) + |b P_j+1|) - ((d_i + d_i+L) + d_j), every operation rounded on its own
        const double rem1 = __dadd_rn(r1, dj[u]), rem2 = __dadd_rn(r2, dj[u]), rem3 = __dadd_rn(r3, dj[u]);
        const double d0 = __dsub_rn(__dadd_rn(__dadd_rn(c1, e1[u]), f1[u]), rem1);
        const double d1 = __dsub_rn(__dadd_rn(__dadd_rn(c2, e1[u]), f2[u]), rem2);
        const double d2 = __dsub_rn(__dadd_rn(__dadd_rn(c2, e2[u]), f1[u]), rem2);
        const double d3 = __dsub_rn(__dadd_rn(__dadd_rn(c3, e1[u]), f3[u]), rem3);
        const double d4 = __dsub_rn(__dadd_rn(__dadd_rn(c3, e3[u]), f1[u]), rem3);
        const bool in = j < n, left = j < i;
        const bool ok1 = in && (left || j > i + 1), ok2 = in && row2 && (left || j > i + 2), ok3 = in && row3 && (left || j > i + 3);
        // the lowest delta of the pair's variants, the lowest v on a tie (= the lowest flat index among them)
        double m = ok1 ? d0 : INFINITY;
        int v = 0;
        if (ok2 && d1 < m) m = d1, v = 1;
        if (ok2 && d2 < m) m = d2, v = 2;
        if (ok3 && d3 < m) m = d3, v = 3;
        if (ok3 && d4 < m) m = d4, v = 4;
        const long long idx = v * nn + (long long)i * n + j;
        if (better(m, idx, best)) best = Best{m, idx};
        e1[u] = e2[u];
        e2[u] = e3[u];
        e3[u] = dist2d(pj[u].x - next.x, pj[u].y - next.y);
        f1[u] = f2[u];
        f2[u] = f3[u];
        f3[u] = dist2d(pj1[u].x - next.x, pj1[u].y - next.y);
      }
    }
  }
  return block_best(best);
}

__global__ __launch_bounds__(256) void local_search_best_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                                const LsTour* __restrict__ desc, Best* __restrict__ partial,
                                                                const int* __restrict__ tphase) {
  const LsTour d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk) return;
  const int phase = tphase[blockIdx.y];                         // uniform over the block
  if (phase == kDone) return;
  const int i0 = blockIdx.x * TI;
  const Best r = phase == kTwoOpt ? best_tile(tp + d.closed, dlen + d.cols, d.n, i0) : or_opt_tile(tp + d.closed, dlen + d.cols, d.n, i0);
  if (threadIdx.x == 0) partial[d.partial + blockIdx.x] = r;
}

// One block per group: the step of its current phase.
//   2-opt:   two_opt_apply_kernel's step - the group's minimum decides, every tour reverses its best segment; the phase
//            ends on a minimum >= -1e-6 or after max_iterations moves of this phase, and the Or-opt phase follows;
//   Or-opt:  every tour applies its own best move if it is below the threshold; the phase ends after an iteration without a move
//            or after max_iterations counted ones (none with max_iterations = 0).  b = its counted iterations: b = 0 or the
//            last round ends the group, otherwise the next round starts with a 2-opt phase.
__global__ __launch_bounds__(256) void local_search_apply_kernel(int* __restrict__ tours, const LsGroup* __restrict__ grp,
                                                                 const Best* __restrict__ partial, long long max_iterations,
                                                                 int max_rounds, LsState* st, LsGroupState* __restrict__ gstate,
                                                                 int* __restrict__ tphase, Best* __restrict__ chosen,
                                                                 int* __restrict__ stage) {
  const int g = blockIdx.x;
  const int phase = gstate[g].phase;
  if (phase == kDone) return;
  __shared__ int moving;
  const LsGroup G = grp[g];
  for (int p = 0; p < G.count; ++p) {
    const Best r = tour_argmin(partial + G.partial + (long long)p * G.nblk, G.nblk);
    if (threadIdx.x == 0) chosen[G.first + p] = r;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double m = chosen[G.first].v;
    for (int b = G.first + 1; b < G.first + G.count; ++b) m = chosen[b].v < m ? chosen[b].v : m;
    moving = m < kThreshold;                                     // 2-opt: all tours move; Or-opt: at least one does
  }
  __syncthreads();
  if (moving) {
    for (int p = 0; p < G.count; ++p) {
      const Best c = chosen[G.first + p];
      int* tour = tours + G.closed + (long long)p * (G.n + 1);
      if (phase == kTwoOpt) {
        apply_move(tour, c.idx, G.n);                            // tsp_utils.py:40-42: every tour, whatever its own change
      } else if (c.v < kThreshold) {                             // uniform over the block
        apply_or_opt_move(tour, stage + G.closed + (long long)p * (G.n + 1), c.idx, G.n);
      }
    }
  }
  if (threadIdx.x != 0) return;
  LsGroupState s = gstate[g];
  bool phase_ends = !moving;
  if (moving) {
    s.phase_iterations += 1;
    (phase == kTwoOpt ? s.two_opt_iterations : s.or_opt_iterations) += 1;
    phase_ends = s.phase_iterations >= max_iterations;           // tsp_utils.py:46-47
  }
  if (phase_ends) {
    if (phase == kTwoOpt) {
      s.phase = max_iterations > 0 ? kOrOpt : kDone;             // an Or-opt phase of no iterations applies nothing: b = 0
    } else if (s.phase_iterations == 0 || s.round + 1 >= max_rounds) {
      s.phase = kDone;
    } else {
      s.phase = kTwoOpt;
      s.round += 1;
    }
    s.phase_iterations = 0;
    for (int b = G.first; b < G.first + G.count; ++b) tphase[b] = s.phase;
    if (s.phase == kDone) atomicAdd(&st->done, 1);
  }
  gstate[g] = s;
}

struct LsLayout {          // byte offsets
  size_t desc, grp, tp, dlen, partial, chosen, stage, gstate, tphase, st, total;
  int tours, nmax, nblk_max;
};

// checks the host arrays and lays the workspace out; `tab` / `gtab` (optional) receive the tables
int local_search_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, LsLayout* L,
                        std::vector<LsTour>* tab, std::vector<LsGroup>* gtab) {
  int T = 0;
  const int rc = check_groups(who, groups, group_n, group_tours, &T);
  if (rc != DIFUSCO_OK) return rc;
  size_t points = 0, closed = 0, cols = 0, nblks = 0;
  L->nmax = L->nblk_max = 0;
  for (int g = 0; g < groups; ++g) {
    const int n = group_n[g], nblk = (n + TI - 1) / TI;
    L->nmax = n > L->nmax ? n : L->nmax;
    L->nblk_max = nblk > L->nblk_max ? nblk : L->nblk_max;
    if (gtab) gtab->push_back(LsGroup{(int)(tab ? tab->size() : 0), group_tours[g], n, nblk, (long long)closed, (long long)nblks});
    for (int p = 0; p < group_tours[g]; ++p) {
      if (tab) tab->push_back(LsTour{n, nblk, (long long)points, (long long)closed, (long long)cols, (long long)nblks});
      closed += (size_t)n + 1;
      cols += (size_t)n;
      nblks += (size_t)nblk;
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
  L->desc = take(sizeof(LsTour) * T);
  L->grp = take(sizeof(LsGroup) * groups);
  L->tp = take(sizeof(double2) * closed);
  L->dlen = take(sizeof(double) * cols);
  L->partial = take(sizeof(Best) * nblks);
  L->chosen = take(sizeof(Best) * T);
  L->stage = take(sizeof(int) * closed);
  L->gstate = take(sizeof(LsGroupState) * groups);               // gstate .. st are cleared by one memset
  L->tphase = take(sizeof(int) * T);
  L->st = take(sizeof(LsState));
  L->total = off;
  return DIFUSCO_OK;
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_local_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes) {
  using namespace difusco;
  if (!bytes) return set_error(DIFUSCO_EINVAL, "local_search_ragged_workspace_bytes: bytes is null");
  LsLayout lay;
  const int rc = local_search_layout("local_search_ragged_workspace_bytes", groups, group_n, group_tours, &lay, nullptr, nullptr);
  if (rc == DIFUSCO_OK) *bytes = lay.total;
  return rc;
}

int difusco_tsp_local_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                    int32_t* tours, int64_t max_iterations, int max_rounds, void* workspace, size_t workspace_bytes,
                                    int64_t* two_opt_iterations_out, int64_t* or_opt_iterations_out, int32_t* rounds_out,
                                    void* stream) {
  using namespace difusco;
  LsLayout lay;
  std::vector<LsTour> tab;
  std::vector<LsGroup> gtab;
  const int rc = local_search_layout("tsp_local_search_ragged", groups, group_n, group_tours, &lay, &tab, &gtab);
  if (rc != DIFUSCO_OK) return rc;
  if (!points || !tours || !workspace || !two_opt_iterations_out || !or_opt_iterations_out || !rounds_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_local_search_ragged: needs non-null device arrays, host two_opt_iterations_out, "
                                     "or_opt_iterations_out and rounds_out [groups] and max_iterations >= 0");
  if (max_rounds < 1) return set_error(DIFUSCO_EINVAL, "tsp_local_search_ragged: max_rounds = %d, needs at least 1", max_rounds);
  if (workspace_bytes < lay.total)
    return set_error(DIFUSCO_EINVAL, "tsp_local_search_ragged: workspace %zu < %zu bytes", workspace_bytes, lay.total);
  char* w = (char*)workspace;
  LsTour* desc = (LsTour*)(w + lay.desc);
  LsGroup* grp = (LsGroup*)(w + lay.grp);
  double2* tp = (double2*)(w + lay.tp);
  double* dlen = (double*)(w + lay.dlen);
  Best* partial = (Best*)(w + lay.partial);
  Best* chosen = (Best*)(w + lay.chosen);
  int* stage = (int*)(w + lay.stage);
  LsGroupState* gstate = (LsGroupState*)(w + lay.gstate);
  int* tphase = (int*)(w + lay.tphase);
  LsState* st = (LsState*)(w + lay.st);
  hipStream_t s = (hipStream_t)stream;
  const int T = lay.tours;
  // the tables, once per call; the host vectors live until the synchronisation below
  hipError_t er = hipMemcpyAsync(desc, tab.data(), sizeof(LsTour) * T, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemcpyAsync(grp, gtab.data(), sizeof(LsGroup) * groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(gstate, 0, lay.total - lay.gstate, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "tsp_local_search_ragged setup: %s", hipGetErrorString(er));
  // A launch sequence either applies a counted iteration of a group's phase or ends that phase: a 2-opt phase takes at most
  // max(max_iterations, 1) + 1 of them, an Or-opt phase max_iterations + 1, a group max_rounds of each.
  const long long per_round = 2 * (max_iterations < (1LL << 60) ? max_iterations : (1LL << 60)) + 3;
  const long long limit = per_round > INT64_MAX / max_rounds ? INT64_MAX : per_round * max_rounds;
  LsState host{0, 0};
  const int poll = 8;
  const dim3 prep_grid((lay.nmax + 1 + 255) / 256, T), best_grid(lay.nblk_max, T);
  for (long long it = 0; it < limit; ++it) {
    hipLaunchKernelGGL(local_search_prep_kernel, prep_grid, dim3(256), 0, s, points, tours, desc, tp, dlen, tphase);
    hipLaunchKernelGGL(local_search_best_kernel, best_grid, dim3(256), 0, s, tp, dlen, desc, partial, tphase);
    hipLaunchKernelGGL(local_search_apply_kernel, dim3(groups), dim3(256), 0, s, tours, grp, partial, (long long)max_iterations,
                       max_rounds, st, gstate, tphase, chosen, stage);
    if ((it + 1) % poll == 0 || it + 1 == limit) {
      er = hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s);
      if (er == hipSuccess) er = hipStreamSynchronize(s);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "local_search state: %s", hipGetErrorString(er));
      if (host.done >= groups) break;
    }
  }
  std::vector<LsGroupState> states(groups);
  er = hipMemcpyAsync(states.data(), gstate, sizeof(LsGroupState) * groups, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "tsp_local_search_ragged counters: %s", hipGetErrorString(er));
  for (int g = 0; g < groups; ++g) {
    two_opt_iterations_out[g] = states[g].two_opt_iterations;
    or_opt_iterations_out[g] = states[g].or_opt_iterations;
    rounds_out[g] = states[g].round + 1;
  }
  return DIFUSCO_OK;
}

}  // extern "C"
