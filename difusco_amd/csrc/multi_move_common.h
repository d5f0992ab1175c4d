// What the multi-move searches share (two_opt_multi.hip, or_opt_multi.hip with its headers, tsp_window_search.hip; the Or-opt row
// loop is in or_opt_rows.h, the neighbour stage in nbr_rows.h): the row-best loop of the 2-opt, the selection of a set of
// proposals with pairwise disjoint position ranges and, at the end, the host side the group-wise entries share - the tour
// descriptor, the walk over the groups that fills it and the launch loop with its poll.  Every function is per translation unit
// (anonymous namespace), as in two_opt_common.h.
//
// Selection never does work proportional to the lengths of the ranges.  A proposal is a row i with a key (ordered bits of its
// value rowv[i], i) and a half-open position range [a, b), 0 <= a < b <= n.  Per round:
//   1. a table of levels 0 .. kmax of n + 1 keys is cleared (kmax = the highest floor(log2(range length)) of a live proposal);
//   2. a proposal of range [a, b), 2^k <= length < 2^(k+1), does its atomic mins at level k: at a and at b - 2^k.  The two cells
//      of 2^k positions cover the range exactly.  The value goes first (a 64-bit atomic min), then the row into the cells that
//      hold the proposal's own value (a 32-bit atomic min), so a cell ends with the lowest (value, row);
//   3. the levels are pushed down, kmax .. 1: cell (l-1, p) takes the minimum of itself, (l, p) and (l, p - 2^(l-1)).  Level 0 is
//      then, per position, the lowest key of the live proposals that cover it;
//   4. the same array is rebuilt upwards as a range-minimum table: (l, p) = min((l-1, p), (l-1, p + 2^(l-1)));
//   5. a proposal wins iff min((k, a), (k, b - 2^k)) is its own key: no live proposal that shares a position with it has a lower
//      one;
//   6. winners mark their first position and the one after their last in two 0/1 arrays; a prefix sum S (starts), E (ends) over
//      the positions follows.  A live proposal is dropped iff its first position lies in a winner's range (S[a] - E[a] > 0) or a
//      winner starts at one of its later positions (S[b-1] - S[a] > 0).
// That is O(n log n) per round.  The winners of all rounds are disjoint.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "two_opt_common.h"

namespace difusco {
namespace {

constexpr double kThreshold = -1e-6;       // the reference's 2-opt threshold (tsp_utils.py:39)
constexpr int kSelectThreads = 1024;
constexpr unsigned long long kNoKey = ~0ull;

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

// The selection of one tour by one block of kSelectThreads threads.  Rows 0 .. rows - 1; row i proposes iff range.proposes(i),
// with the value rowv[i] and the position range range(i, &a, &b) = [a, b), 0 <= a < b <= n.  live, winners: rows ints each;
// tabv, tabi: (floor(log2(n + 1)) + 1) levels of n + 1 cells; marks, cum: n + 1 entries.  Returns the number of winners (in
// every thread), their rows in winners[] in no particular order; 0 iff no row proposes.  *nwin: a word of LDS.
template <class Range>
__device__ __forceinline__ int select_disjoint(const Range range, int rows, int n, const double* __restrict__ rowv,
                                               int* __restrict__ live, int* __restrict__ winners,
                                               unsigned long long* __restrict__ tabv, int* __restrict__ tabi,
                                               int2* __restrict__ marks, int2* __restrict__ cum, int select_rounds, int* nwin) {
  const int stride = n + 1, tid = threadIdx.x;
  int cnt = 0, kmax = 0;
  for (int i = tid; i < rows; i += kSelectThreads) {
    const bool p = range.proposes(i);
    live[i] = p;
    if (p) {
      int a, b;
      range(i, &a, &b);
      cnt += 1;
      const int k = floor_log2(b - a);
      kmax = k > kmax ? k : kmax;
    }
  }
  for (int p = tid; p <= n; p += kSelectThreads) marks[p] = make_int2(0, 0);
  if (tid == 0) *nwin = 0;
  int nlive;
  block_sum_max(cnt, kmax, &nlive, &kmax);
  if (nlive == 0) return 0;

  for (int round = 0; round < select_rounds && nlive > 0; ++round) {
    const int cells = (kmax + 1) * stride;
    for (int c = tid; c < cells; c += kSelectThreads) tabv[c] = kNoKey, tabi[c] = INT_MAX;
    __syncthreads();
    for (int i = tid; i < rows; i += kSelectThreads)
      if (live[i]) {
        int a, e;
        range(i, &a, &e);
        const int k = floor_log2(e - a);
        const unsigned long long key = ordered_bits(rowv[i]);
        atomicMin(&tabv[k * stride + a], key);
        atomicMin(&tabv[k * stride + e - (1 << k)], key);
      }
    __syncthreads();
    for (int i = tid; i < rows; i += kSelectThreads)
      if (live[i]) {
        int a, e;
        range(i, &a, &e);
        const int k = floor_log2(e - a);
        const unsigned long long key = ordered_bits(rowv[i]);
        const int c0 = k * stride + a, c1 = k * stride + e - (1 << k);
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
        int a, e;
        range(i, &a, &e);
        const int k = floor_log2(e - a);
        const int c0 = k * stride + a, c1 = k * stride + e - (1 << k);
        unsigned long long v = tabv[c0];
        int w = tabi[c0];
        if (key_less(tabv[c1], tabi[c1], v, w)) v = tabv[c1], w = tabi[c1];
        if (w == i && v == ordered_bits(rowv[i])) {              // no intersecting live proposal has a lower key
          live[i] = 0;
          marks[a].x = 1;
          marks[e].y = 1;
          winners[atomicAdd(nwin, 1)] = i;
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
        int a, e;
        range(i, &a, &e);
        if (cum[a].x - cum[a].y > 0 || cum[e - 1].x - cum[a].x > 0) {  // it shares a position with a winner
          live[i] = 0;
        } else {
          cnt += 1;
          const int k = floor_log2(e - a);
          kmax = k > kmax ? k : kmax;
        }
      }
    block_sum_max(cnt, kmax, &nlive, &kmax);
  }
  __syncthreads();
  return *nwin;
}

// the range of a 2-opt proposal (i, rowj[i]): [i, rowj[i] + 1); rowj[i] < 0: the row does not propose
struct TwoOptRange {
  const int* __restrict__ rowj;
  __device__ __forceinline__ bool proposes(int i) const { return rowj[i] >= 0; }
  __device__ __forceinline__ void operator()(int i, int* a, int* b) const { *a = i, *b = rowj[i] + 1; }
};

// a wave reverses tour[i+1 .. j] of one winner at a time
__device__ __forceinline__ void reverse_winners(int* __restrict__ tour, const int* __restrict__ winners,
                                                const int* __restrict__ rowj, int total) {
  const int lane = threadIdx.x & 63;
  for (int w = threadIdx.x >> 6; w < total; w += kSelectThreads / 64) {
    const int i = winners[w], j = rowj[i], len = j - i;
    for (int s = lane; s < len / 2; s += 64) {
      const int x = i + 1 + s, y = j - s;
      const int tmp = tour[x];
      tour[x] = tour[y];
      tour[y] = tmp;
    }
  }
}

// ---- what the searches of or_opt_multi.hip and tsp_window_search.hip share beyond the selection: the Or-opt variants, the range
// of a proposal of either phase, the Or-opt apply, the fixed-association tour length and the segment swaps of a kick

__device__ __forceinline__ int variant_len(int v) { return (v + 3) >> 1; }      // 1, 2, 2, 3, 3
__device__ __forceinline__ bool variant_rev(int v) { return v == 2 || v == 4; }

// the range of a proposal of either phase.  2-opt (i, j = rowj[i]): [i, j + 1).  Or-opt (rowj[i] = v n + j): [min(i, j), hi + 1)
// with hi = j for j > i + L and i + L for j < i - from the first position of the lowest of the three edges the move touches to
// the first position of the highest.  One type for both, so that the selection is instantiated once.
struct PhaseRange {
  const int* __restrict__ rowj;
  int n;
  bool or_opt;
  __device__ __forceinline__ bool proposes(int i) const { return rowj[i] >= 0; }
  __device__ __forceinline__ void operator()(int i, int* a, int* b) const {
    const int c = rowj[i], j = or_opt ? c % n : c, L = or_opt ? variant_len(c / n) : 0;
    *a = j < i ? j : i;
    *b = (j < i ? i + L : j) + 1;
  }
};

// the Or-opt moves of the winners: the stretch between a segment and its insertion edge shifts by L places over the segment, so
// a wave copies the rewritten positions lo .. hi of one winner to `stage` (n + 1 entries of the tour's own), and after a barrier
// writes them back from there (apply_or_opt_move of or_opt.hip, a winner per wave).  The stretches are disjoint.
__device__ __forceinline__ void or_opt_winners(int* __restrict__ tour, int* __restrict__ stage, const int* __restrict__ winners,
                                               const int* __restrict__ rowj, int n, int total) {
  const int lane = threadIdx.x & 63;
  for (int w = threadIdx.x >> 6; w < total; w += kSelectThreads / 64) {
    const int i = winners[w], j = rowj[i] % n, L = variant_len(rowj[i] / n);
    const int lo = (j < i ? j : i) + 1, hi = j < i ? i + L : j;  // 1 <= lo <= hi <= n - 1
    for (int k = lo + lane; k <= hi; k += 64) stage[k] = tour[k];
  }
  __syncthreads();
  for (int w = threadIdx.x >> 6; w < total; w += kSelectThreads / 64) {
    const int i = winners[w], j = rowj[i] % n, v = rowj[i] / n, L = variant_len(v);
    const bool rev = variant_rev(v);
    const int lo = (j < i ? j : i) + 1, hi = j < i ? i + L : j;
    for (int k = lo + lane; k <= hi; k += 64) {
      int src;
      if (j > i) {                                               // tour[:i+1] + tour[i+L+1 : j+1] + seg + tour[j+1:]
        const int s = k - (j - L + 1);
        src = s < 0 ? k + L : (rev ? i + L - s : i + 1 + s);
      } else {                                                   // tour[:j+1] + seg + tour[j+1 : i+1] + tour[i+L+1:]
        const int s = k - (j + 1);
        src = s < L ? (rev ? i + L - s : i + 1 + s) : k - L;
      }
      tour[k] = stage[src];
    }
  }
}

constexpr int kMaxKickSize = 64;           // the draws of a kick: one wave decides which are kept
constexpr int kLenParts = kSelectThreads;  // strided partial sums of a tour length

// The length of the closed tour in the fixed association: thread r sums d_r, d_r+1024, .. in rising k from 0.0, then a halving
// tree over the 1024 partial sums (part[r] += part[r + h], h = 512 .. 1).  d_k is prep_entry's.  The result in every thread.
__device__ __forceinline__ double tour_length(const double* __restrict__ points, const int* __restrict__ tour, int n,
                                              double* part) {
  double acc = 0.0;
  for (int k = threadIdx.x; k < n; k += kLenParts) {
    const int c = tour[k], c1 = tour[k + 1];
    acc = __dadd_rn(acc, dist2d(points[2 * c] - points[2 * c1], points[2 * c + 1] - points[2 * c1 + 1]));
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int h = kLenParts / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] = __dadd_rn(part[threadIdx.x], part[threadIdx.x + h]);
    __syncthreads();
  }
  const double len = part[0];
  __syncthreads();
  return len;
}

// the kept draws swap their two adjacent segments in `tour` reading the incumbent `inc`, a wave per draw
__device__ __forceinline__ void kick_swaps(int* __restrict__ tour, const int* __restrict__ inc, int kick_size, const int* ka,
                                           const int* kl1, const int* kb, const int* kkeep) {
  const int lane = threadIdx.x & 63;
  for (int c = threadIdx.x >> 6; c < kick_size; c += kSelectThreads / 64) {
    if (!kkeep[c]) continue;
    const int a = ka[c], b = kb[c], l1 = kl1[c], l2 = b - a - l1;
    for (int k = a + lane; k < b; k += 64) tour[k] = inc[k < a + l2 ? k + l1 : k - l2];
  }
}

// ---- the host side the group-wise entries share (two_opt_multi.hip, or_opt_multi.hip)

int table_levels(int n) {                          // floor(log2(n + 1)) + 1
  int l = 0;
  while ((2LL << l) <= (long long)n + 1) ++l;
  return l + 1;
}

struct TourDesc {          // a tour of a call; offsets in elements of the array they index
  int n, nblk_two, nblk_or, group;   // row tiles of a full 2-opt sweep (rows 0 .. n - 3) and of a full Or-opt sweep (0 .. n - 2)
  long long points;        // the group's first coordinate in `points` (doubles, 2 n per group); a group's first entry in
                           // `neighbors` (n K per group) follows from it: (points >> 1) K, see nbr_walk (nbr_rows.h)
  long long closed;        // the tour's first entry in tours, tp, marks and cum (n + 1 per tour)
  long long cols;          //                       in dlen, rowv, rowj, live, winners, pos and rowkey (n per tour)
  long long table;         //                       in tabv and tabi (levels (n + 1) per tour)
};

struct GroupTotals {       // of a call: the tours, the largest group and its row tiles, the elements the sections hold
  int tours, nmax, nblk_two, nblk_or;
  size_t closed, cols, cells, points;
};

// Checks the group arrays of a _ragged entry and, with `lists`, K, closing and the launch limit of the n K list entries of a
// group; then walks the groups: `tot` receives the totals, `tab` (optional) the descriptor of every tour.
int walk_groups(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, bool lists, int K, int closing,
                GroupTotals* tot, std::vector<TourDesc>* tab) {
  *tot = GroupTotals{};
  const int rc = check_groups(who, groups, group_n, group_tours, &tot->tours);
  if (rc != DIFUSCO_OK) return rc;
  if (lists && K < 1) return set_error(DIFUSCO_EINVAL, "%s: K = %d, needs at least 1", who, K);
  if (lists && closing != 0 && closing != 1) return set_error(DIFUSCO_EINVAL, "%s: closing = %d, needs 0 or 1", who, closing);
  for (int g = 0; g < groups; ++g) {
    const int n = group_n[g];
    const int nblk_two = (n - 2 + TI - 1) / TI, nblk_or = (n - 1 + TI - 1) / TI;
    if (lists && (long long)n * K > (long long)INT32_MAX * 256)
      return set_error(DIFUSCO_EINVAL, "%s: group %d has n K = %lld list entries, too many for one launch", who, g, (long long)n * K);
    if (n > tot->nmax) tot->nmax = n, tot->nblk_two = nblk_two, tot->nblk_or = nblk_or;
    for (int p = 0; p < group_tours[g]; ++p) {
      if (tab)
        tab->push_back(TourDesc{n, nblk_two, nblk_or, g, (long long)tot->points, (long long)tot->closed, (long long)tot->cols,
                                (long long)tot->cells});
      tot->closed += (size_t)n + 1;
      tot->cols += (size_t)n;
      tot->cells += (size_t)table_levels(n) * ((size_t)n + 1);
    }
    tot->points += 2 * (size_t)n;
  }
  return DIFUSCO_OK;
}

struct Sections {          // hands out the sections of a workspace, each rounded up to 256 bytes; an absent one is empty
  size_t off = 0;
  size_t take(size_t bytes, bool present = true) {
    const size_t at = off;
    if (present) off += up256(bytes);
    return at;
  }
};

struct Polled {            // of poll_launches: the HIP status, the host synchronisations
  hipError_t status;
  int syncs;
};

// The launch loop of a search whose device state counts its stopped groups in the int at `stopped`: calls enqueue() - one launch
// sequence - up to `limit` times; every `poll`-th time, and at the last, copies the word back, synchronises and ends if every
// group has stopped.
template <class Enqueue>
Polled poll_launches(long long limit, int poll, int groups, const int* stopped, hipStream_t s, Enqueue enqueue) {
  Polled r{hipSuccess, 0};
  int done = 0;
  for (long long it = 0; it < limit; ++it) {
    enqueue();
    if ((it + 1) % poll == 0 || it + 1 == limit) {
      r.status = hipMemcpyAsync(&done, stopped, sizeof(int), hipMemcpyDeviceToHost, s);
      if (r.status == hipSuccess) r.status = hipStreamSynchronize(s);
      r.syncs += 1;
      if (r.status != hipSuccess || done >= groups) break;
    }
  }
  return r;
}

}  // namespace
}  // namespace difusco
