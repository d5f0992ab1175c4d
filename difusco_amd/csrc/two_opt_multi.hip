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
// Selection never does work proportional to the lengths of the ranges.  A key is (ordered bits of the change, row).  Per round:
//   1. a table of levels 0 .. kmax of n + 1 keys is cleared (kmax = the highest floor(log2(range length)) of a live proposal);
//   2. a proposal of range [i, j + 1), 2^k <= length < 2^(k+1), does its atomic mins at level k: at i and at j + 1 - 2^k.  The
//      two cells of 2^k positions cover the range exactly.  The change goes first (a 64-bit atomic min), then the row into the
//      cells that hold the proposal's own change (a 32-bit atomic min), so a cell ends with the lowest (change, row);
//   3. the levels are pushed down, kmax .. 1: cell (l-1, p) takes the minimum of itself, (l, p) and (l, p - 2^(l-1)).  Level 0 is
//      then, per position, the lowest key of the live proposals that cover it;
//   4. the same array is rebuilt upwards as a range-minimum table: (l, p) = min((l-1, p), (l-1, p + 2^(l-1)));
//   5. a proposal wins iff min((k, i), (k, j + 1 - 2^k)) is its own key: no live proposal that shares a position with it has a
//      lower one;
//   6. winners mark their first position and the one after their last in two 0/1 arrays; a prefix sum S (starts), E (ends) over
//      the positions follows.  A live proposal is dropped iff its first position lies in a winner's range (S[i] - E[i] > 0) or a
//      winner starts at one of its later positions (S[j] - S[i] > 0).
// That is O(n log n) per round.  The winners of all rounds are disjoint; a wave reverses one winner's stretch at a time.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

constexpr double kThreshold = -1e-6;       // the reference's 2-opt threshold (tsp_utils.py:39)
constexpr int kSelectThreads = 1024;
constexpr unsigned long long kNoKey = ~0ull;

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

__device__ __forceinline__ bool better_col(double v, int j, double bv, int bj) { return v < bv || (v == bv && j < bj); }

// one block of the row-best sweep: rows i0 .. i0 + TI - 1 of the tour (P = its tp, D = its dlen, n nodes) against all their
// columns, best_tile's loop; row i <= n - 3 gets its lowest change in rowv[i] and that change's lowest column in rowj[i], or
// rowj[i] = -1 if the lowest change is not below the threshold
__device__ __forceinline__ void row_best_tile(const double2* __restrict__ P, const double* __restrict__ D, int n, int i0,
                                              double* __restrict__ rowv, int* __restrict__ rowj) {
  __shared__ double2 pi[TI + 1];
  __shared__ double di[TI];
  __shared__ double redv[4][TI];
  __shared__ int redj[4][TI];
  for (int t = threadIdx.x; t <= TI; t += blockDim.x) pi[t] = P[i0 + t <= n ? i0 + t : n];
  for (int t = threadIdx.x; t < TI; t += blockDim.x) di[t] = D[i0 + t < n ? i0 + t : n - 1];
  __syncthreads();
  double bv[TI];
  int bj[TI];
#pragma unroll
  for (int r = 0; r < TI; ++r) bv[r] = 0.0, bj[r] = -1;
  for (int jbase = i0 + 2; jbase < n; jbase += 256 * JPT) {
    double2 pj[JPT], pj1[JPT];
    double dj[JPT];
    int jj[JPT];
#pragma unroll
    for (int u = 0; u < JPT; ++u) {
      const int j = jbase + u * 256 + threadIdx.x, jc = j < n ? j : n - 1;
      jj[u] = j;
      pj[u] = P[jc];
      pj1[u] = P[jc + 1];
      dj[u] = D[jc];
    }
#pragma unroll
    for (int r = 0; r < TI; ++r) {
      const int i = i0 + r;
      const double2 a = pi[r], a1 = pi[r + 1];
      const double d_i = di[r];
#pragma unroll
      for (int u = 0; u < JPT; ++u) {
        const int j = jj[u];
        const double x0 = a.x - pj[u].x, y0 = a.y - pj[u].y;
        const double x1 = a1.x - pj1[u].x, y1 = a1.y - pj1[u].y;
        // change = A_ij + A_i+1,j+1 - A_i,i+1 - A_j,j+1, evaluated left to right (tsp_utils.py:31), as in best_tile
        const double change = __dsub_rn(__dsub_rn(__dadd_rn(dist2d(x0, y0), dist2d(x1, y1)), d_i), dj[u]);
        // a thread meets its columns in rising order: the strict comparison keeps the lowest j of equal changes
        if (j < n && j >= i + 2 && change < bv[r]) bv[r] = change, bj[r] = j;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < TI; ++r) {
    double v = bv[r];
    int j = bj[r];
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_down(v, off);
      const int oj = __shfl_down(j, off);
      if (better_col(ov, oj, v, j)) v = ov, j = oj;
    }
    if (lane == 0) redv[wave][r] = v, redj[wave][r] = j;
  }
  __syncthreads();
  if (threadIdx.x < TI && i0 + (int)threadIdx.x <= n - 3) {
    const int r = threadIdx.x;
    double v = redv[0][r];
    int j = redj[0][r];
    for (int w = 1; w < 4; ++w)
      if (better_col(redv[w][r], redj[w][r], v, j)) v = redv[w][r], j = redj[w][r];
    rowv[i0 + r] = v;
    rowj[i0 + r] = v < kThreshold ? j : -1;
  }
}

__global__ __launch_bounds__(256) void multi_row_best_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                             const MtTour* __restrict__ desc, double* __restrict__ rowv,
                                                             int* __restrict__ rowj, const int* __restrict__ tdone) {
  const MtTour d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk || tdone[blockIdx.y]) return;
  row_best_tile(tp + d.closed, dlen + d.cols, d.n, blockIdx.x * TI, rowv + d.cols, rowj + d.cols);
}

// a double as an unsigned integer of the same order
__device__ __forceinline__ unsigned long long ordered_bits(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

__device__ __forceinline__ int floor_log2(int x) { return 31 - __clz(x); }

__device__ __forceinline__ bool key_less(unsigned long long v, int i, unsigned long long bv, int bi) {
  return v < bv || (v == bv && i < bi);
}

__device__ __forceinline__ int wave_sum(int x) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
  return x;
}

__device__ __forceinline__ int wave_max(int x) {
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_down(x, off);
    x = o > x ? o : x;
  }
  return x;
}

// the sum and the maximum (of values >= 0) over the block, in every thread
__device__ __forceinline__ void block_sum_max(int add, int mx, int* sum_out, int* max_out) {
  __shared__ int acc[2];
  if (threadIdx.x == 0) acc[0] = 0, acc[1] = 0;
  __syncthreads();
  add = wave_sum(add);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) {
    if (add) atomicAdd(&acc[0], add);
    if (mx) atomicMax(&acc[1], mx);
  }
  __syncthreads();
  *sum_out = acc[0];
  *max_out = acc[1];
  __syncthreads();
}

// cum[p] = the sums of marks[0 .. p], p = 0 .. n, over the block's threads: a thread sums a contiguous chunk, the chunk sums are
// scanned in LDS
__device__ __forceinline__ void block_prefix(const int2* __restrict__ marks, int2* __restrict__ cum, int n) {
  __shared__ int2 part[kSelectThreads];
  const int chunk = (n + 1 + kSelectThreads - 1) / kSelectThreads;
  const int lo = threadIdx.x * chunk, hi = lo + chunk < n + 1 ? lo + chunk : n + 1;
  int2 mine = make_int2(0, 0);
  for (int p = lo; p < hi; ++p) mine.x += marks[p].x, mine.y += marks[p].y;
  part[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < kSelectThreads; off <<= 1) {
    int2 o = make_int2(0, 0);
    if ((int)threadIdx.x >= off) o = part[threadIdx.x - off];
    __syncthreads();
    part[threadIdx.x].x += o.x;
    part[threadIdx.x].y += o.y;
    __syncthreads();
  }
  int2 run = make_int2(part[threadIdx.x].x - mine.x, part[threadIdx.x].y - mine.y);
  for (int p = lo; p < hi; ++p) {
    run.x += marks[p].x;
    run.y += marks[p].y;
    cum[p] = run;
  }
  __syncthreads();
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
  const int n = d.n, rows = n - 2, stride = n + 1, tid = threadIdx.x;
  const double* rowv = rowv_all + d.cols;
  const int* rowj = rowj_all + d.cols;
  int* live = live_all + d.cols;
  int* winners = winners_all + d.cols;
  unsigned long long* tabv = tabv_all + d.table;
  int* tabi = tabi_all + d.table;
  int2* marks = marks_all + d.closed;
  int2* cum = cum_all + d.closed;
  __shared__ int nwin;

  int cnt = 0, kmax = 0;
  for (int i = tid; i < rows; i += kSelectThreads) {
    const int j = rowj[i];
    live[i] = j >= 0;
    if (j >= 0) {
      cnt += 1;
      const int k = floor_log2(j + 1 - i);
      kmax = k > kmax ? k : kmax;
    }
  }
  for (int p = tid; p <= n; p += kSelectThreads) marks[p] = make_int2(0, 0);
  if (tid == 0) nwin = 0;
  int nlive;
  block_sum_max(cnt, kmax, &nlive, &kmax);
  if (nlive == 0) {                                              // no proposal: the tour is done
    if (tid == 0) {
      tdone[t] = 1;
      report_to_group(gs, G, false, max_iterations, tdone, st);
    }
    return;
  }

  for (int round = 0; round < select_rounds && nlive > 0; ++round) {
    const int cells = (kmax + 1) * stride;
    for (int c = tid; c < cells; c += kSelectThreads) tabv[c] = kNoKey, tabi[c] = INT_MAX;
    __syncthreads();
    for (int i = tid; i < rows; i += kSelectThreads)
      if (live[i]) {
        const int e = rowj[i] + 1, k = floor_log2(e - i);
        const unsigned long long key = ordered_bits(rowv[i]);
        atomicMin(&tabv[k * stride + i], key);
        atomicMin(&tabv[k * stride + e - (1 << k)], key);
      }
    __syncthreads();
    for (int i = tid; i < rows; i += kSelectThreads)
      if (live[i]) {
        const int e = rowj[i] + 1, k = floor_log2(e - i);
        const unsigned long long key = ordered_bits(rowv[i]);
        const int c0 = k * stride + i, c1 = k * stride + e - (1 << k);
        if (tabv[c0] == key) atomicMin(&tabi[c0], i);
        if (tabv[c1] == key) atomicMin(&tabi[c1], i);
      }
    __syncthreads();
    for (int l = kmax; l >= 1; --l) {                            // push down: level 0 becomes the cover minimum per position
      const int h = 1 << (l - 1);
      unsigned long long* lo_v = tabv + (l - 1) * stride;
      int* lo_i = tabi + (l - 1) * stride;
      const unsigned long long* hi_v = tabv + l * stride;
      const int* hi_i = tabi + l * stride;
      for (int p = tid; p < n; p += kSelectThreads) {
        unsigned long long v = lo_v[p];
        int i = lo_i[p];
        if (key_less(hi_v[p], hi_i[p], v, i)) v = hi_v[p], i = hi_i[p];
        if (p >= h && key_less(hi_v[p - h], hi_i[p - h], v, i)) v = hi_v[p - h], i = hi_i[p - h];
        lo_v[p] = v;
        lo_i[p] = i;
      }
      __syncthreads();
    }
    for (int l = 1; l <= kmax; ++l) {                            // and up again: the range-minimum table of level 0
      const int h = 1 << (l - 1);
      const unsigned long long* lo_v = tabv + (l - 1) * stride;
      const int* lo_i = tabi + (l - 1) * stride;
      unsigned long long* hi_v = tabv + l * stride;
      int* hi_i = tabi + l * stride;
      for (int p = tid; p + 2 * h <= n; p += kSelectThreads) {
        unsigned long long v = lo_v[p];
        int i = lo_i[p];
        if (key_less(lo_v[p + h], lo_i[p + h], v, i)) v = lo_v[p + h], i = lo_i[p + h];
        hi_v[p] = v;
        hi_i[p] = i;
      }
      __syncthreads();
    }
    int won = 0;
    for (int i = tid; i < rows; i += kSelectThreads)
      if (live[i]) {
        const int e = rowj[i] + 1, k = floor_log2(e - i);
        const int c0 = k * stride + i, c1 = k * stride + e - (1 << k);
        unsigned long long v = tabv[c0];
        int w = tabi[c0];
        if (key_less(tabv[c1], tabi[c1], v, w)) v = tabv[c1], w = tabi[c1];
        if (w == i && v == ordered_bits(rowv[i])) {              // no intersecting live proposal has a lower key
          live[i] = 0;
          marks[i].x = 1;
          marks[e].y = 1;
          winners[atomicAdd(&nwin, 1)] = i;
          won += 1;
        }
      }
    int dummy;
    block_sum_max(won, 0, &won, &dummy);
    nlive -= won;
    if (nlive == 0 || round + 1 == select_rounds) break;
    block_prefix(marks, cum, n);
    cnt = 0, kmax = 0;
    for (int i = tid; i < rows; i += kSelectThreads)
      if (live[i]) {
        const int j = rowj[i];
        if (cum[i].x - cum[i].y > 0 || cum[j].x - cum[i].x > 0) {  // it shares a position with a winner
          live[i] = 0;
        } else {
          cnt += 1;
          const int k = floor_log2(j + 1 - i);
          kmax = k > kmax ? k : kmax;
        }
      }
    block_sum_max(cnt, kmax, &nlive, &kmax);
  }
  __syncthreads();

  // apply: the winners' ranges are disjoint; a wave reverses tour[i+1 .. j] of one winner at a time
  int* tour = tours + d.closed;
  const int total = nwin, lane = tid & 63;
  for (int w = tid >> 6; w < total; w += kSelectThreads / 64) {
    const int i = winners[w], j = rowj[i], len = j - i;
    for (int s = lane; s < len / 2; s += 64) {
      const int x = i + 1 + s, y = j - s;
      const int tmp = tour[x];
      tour[x] = tour[y];
      tour[y] = tmp;
    }
  }
  if (tid == 0) {
    tmoves[t] += total;
    report_to_group(gs, G, true, max_iterations, tdone, st);
  }
}

struct MtLayout {          // byte offsets
  size_t desc, grp, tp, dlen, rowv, rowj, live, winners, tabv, tabi, marks, cum, gstate, tdone, tmoves, st, total;
  int tours, nmax, nblk_max;
};

constexpr int kMaxTours = 65535;                   // a grid dimension; the limits of difusco_tsp_two_opt_ragged
constexpr int kMaxNodes = 65535 * TI;

int table_levels(int n) {                          // floor(log2(n + 1)) + 1
  int l = 0;
  while ((2LL << l) <= (long long)n + 1) ++l;
  return l + 1;
}

// checks the host arrays and lays the workspace out; `tab` / `gtab` (optional) receive the tables
int multi_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, MtLayout* L,
                 std::vector<MtTour>* tab, std::vector<GroupRef>* gtab) {
  if (groups < 1) return set_error(DIFUSCO_EINVAL, "%s: groups = %d, needs at least 1", who, groups);
  if (!group_n || !group_tours) return set_error(DIFUSCO_EINVAL, "%s: group_n / group_tours is null", who);
  long long T = 0;
  for (int g = 0; g < groups; ++g) {
    if (group_n[g] < 4) return set_error(DIFUSCO_EINVAL, "%s: group %d has n = %d, needs n >= 4", who, g, group_n[g]);
    if (group_n[g] > kMaxNodes)
      return set_error(DIFUSCO_EINVAL, "%s: group %d has n = %d, at most %d nodes", who, g, group_n[g], kMaxNodes);
    if (group_tours[g] < 1) return set_error(DIFUSCO_EINVAL, "%s: group %d has %d tours, needs at least 1", who, g, group_tours[g]);
    T += group_tours[g];
    if (T > kMaxTours) return set_error(DIFUSCO_EINVAL, "%s: more than %d tours in one call", who, kMaxTours);
  }
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
