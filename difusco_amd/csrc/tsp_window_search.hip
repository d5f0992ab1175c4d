// Windowed iterated search (difusco_tsp_window_search_ragged): the iterated multi-move search of or_opt_multi.hip on the windows
// of a tour, one block per window, the whole search of a window - descents, kicks and keeps - inside ONE launch.  The rule is
// stated in include/difusco_hip.h and restated in numpy in tests/tsp_window_search_emulation.py.
//
// A window is the open path of the positions lo .. lo + m of a tour, m <= 1024.  Its end positions never move, so a window
// changes only edges of its own and the windows of a pass need nothing from one another: no block waits on a block.
//   win_search_kernel   one block of 1024 threads per (tour, window) of a pass.  LDS holds the state of the window for the whole
//                       launch: the coordinates by local index (gathered once from points[tour[lo + l]]), the candidate and the
//                       incumbent path as local indices, the edge lengths, and one region that is the position-ordered
//                       coordinates while a sweep evaluates and the row bests and selection lists after it.  A sweep: prep
//                       (tp, d), row bests - one row per G lanes, G = the power of two with G m <= 1024, columns strided over
//                       the lanes and combined by (value, column), the changes and deltas of row_best_tile / or_row_best_tile
//                       bit for bit -, selection, apply (reverse_winners, or_opt_winners).  The selection is step 2 of the
//                       multi-move 2-opt read literally, every live proposal against the list of live proposals: the tables of
//                       select_disjoint ((log2 m + 1) (m + 1) keys of 12 bytes, 135 KB at m = 1024) do not fit LDS, and near a
//                       local optimum a sweep has a handful of proposals.  The winners are the same set.
//   win_keep_kernel     one block per tour: the tour-level lengths of a tour and its candidate in the fixed association
//                       (tour_length, multi_move_common.h) and the keep; also the keep of the closing descent.
// The host uploads the window tables of the even and the odd passes once and enqueues 2 R launches without a synchronisation;
// the first and the closing descent are mls_descent (or_opt_multi.hip).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "common.h"
#include "kernels.h"
#include "multi_move_common.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

constexpr int kWinMax = 1024;              // the most cities between the ends of a window: its path has at most 1025 positions
constexpr int kWinMin = 16;
constexpr int kWinSkip = 8;                // a window of fewer cities is copied unchanged
constexpr int kWinMaxKicks = 1024;

struct WinDesc {           // a window of a pass
  int tour, lo, m, index;  // positions lo .. lo + m of the tour; index: w of the rule
};

struct WinTour {           // offsets in elements of the array they index
  int n, stride;           // stride: C of the rule, ceil(n / W) + 1
  long long points;        // the group's first coordinate in `points` (doubles)
  long long closed;        // the tour's first entry in tours and the candidates (n + 1 per tour)
};

struct WinStat {           // device-resident counters of a tour, zero at the start of a call
  int passes_kept, kicks_kept, kicks_improved, pad;
  long long swapped, sweeps, moves;
  double first_length, final_length;
};

// the region of LDS that is tp while a sweep evaluates and the row bests and lists after it
constexpr int kOffRowKey = 0;                                  // unsigned long long [1024]
constexpr int kOffRowJ = kOffRowKey + 8 * kWinMax;             // int [1024]
constexpr int kOffLive = kOffRowJ + 4 * kWinMax;               // int [1024]: (a, b, row) of the live proposals
constexpr int kOffWin = kOffLive + 4 * kWinMax;                // int [1024]: the rows of the winners
constexpr int kRegionBytes = kOffWin + 4 * kWinMax;            // 20480 >= 16 * 1025 (tp) and >= 8 * 1024 (length partials)
static_assert(kRegionBytes >= 16 * (kWinMax + 1), "tp fits the region");
static_assert(kOffRowJ >= 4 * (kWinMax + 1), "the Or-opt stage fits in front of rowj");

struct WinLds {
  double2 C[kWinMax + 1];  // coordinates by local index
  double D[kWinMax];       // d_k of the candidate path
  int path[kWinMax + 1];   // the candidate: local indices by position
  int inc[kWinMax + 1];    // the incumbent
  int pad[2];
  alignas(16) char region[kRegionBytes];
  int ka[kMaxKickSize], kl1[kMaxKickSize], kb[kMaxKickSize], kkeep[kMaxKickSize];
  int cnt[4];              // live proposals of a round, winners so far
  __device__ double2* tp() { return (double2*)region; }
  __device__ unsigned long long* rowkey() { return (unsigned long long*)(region + kOffRowKey); }
  __device__ int* rowj() { return (int*)(region + kOffRowJ); }
  __device__ int* live() { return (int*)(region + kOffLive); }
  __device__ int* winners() { return (int*)(region + kOffWin); }
  __device__ int* stage() { return (int*)region; }             // over rowkey, free after the selection
  __device__ double* part() { return (double*)region; }
};
static_assert(sizeof(WinLds) <= 64 * 1024, "a window's state fits 64 KB of LDS");

__device__ __forceinline__ int pack_range(int a, int b, int row) { return a | (b << 10) | (row << 21); }   // a, row < 1024; b <= 1024

// tp and d of the candidate path; ends behind a barrier
__device__ __forceinline__ void win_prep(WinLds& s, int m) {
  double2* tp = s.tp();
  for (int k = threadIdx.x; k <= m; k += kSelectThreads) tp[k] = s.C[s.path[k]];
  __syncthreads();
  for (int k = threadIdx.x; k < m; k += kSelectThreads) s.D[k] = dist2d(tp[k].x - tp[k + 1].x, tp[k].y - tp[k + 1].y);
  __syncthreads();
}

// the lowest of (v, c) over the G lanes of a row, in every lane
__device__ __forceinline__ void group_best(double& v, int& c, int G) {
  for (int off = G >> 1; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int oc = __shfl_xor(c, off);
    if (better_col(ov, oc, v, c)) v = ov, c = oc;
  }
}

// The row bests of one sweep into registers: lane `sub` of the G lanes of row i takes the columns sub, sub + G, ..  2-opt
// (row_best_tile): the lowest change of row i <= m - 3 and its lowest column.  Or-opt (or_row_best_tile): the lowest delta of row
// i <= m - 2 and the lowest v m + j of it.  *code < 0: the row does not propose.
__device__ __forceinline__ void win_row_best(WinLds& s, int m, bool or_opt, int i, int sub, int G, double* value, int* code) {
  const double2* P = s.tp();
  const double* D = s.D;
  const int n = m;
  double bv = 0.0;
  int bc = or_opt ? INT_MAX : -1;
  if (!or_opt) {
    if (i <= n - 3) {
      const double2 a = P[i], a1 = P[i + 1];
      const double d_i = D[i];
      int j = i + 2 + sub;
      for (; j < n; j += G) {
        const double2 pj = P[j], pj1 = P[j + 1];
        const double x0 = a.x - pj.x, y0 = a.y - pj.y;
        const double x1 = a1.x - pj1.x, y1 = a1.y - pj1.y;
        const double change = __dsub_rn(__dsub_rn(__dadd_rn(dist2d(x0, y0), dist2d(x1, y1)), d_i), D[j]);
        if (change < bv) bv = change, bc = j;                    // rising j: the strict comparison keeps the lowest j
      }
    }
    group_best(bv, bc, G);
    *value = bv;
    *code = bv < kThreshold ? bc : -1;
    return;
  }
  if (i <= n - 2) {
    const bool row2 = i <= n - 3, row3 = i <= n - 4;
    const double2 p0 = P[i], p1 = P[i + 1], p2 = P[i + 2 < n ? i + 2 : n], p3 = P[i + 3 < n ? i + 3 : n], p4 = P[i + 4 < n ? i + 4 : n];
    // |P_i P_i+L+1| and d_i + d_i+L, 0 where the row has no segment of L
    const double c1 = dist2d(p0.x - p2.x, p0.y - p2.y), r1 = __dadd_rn(D[i], D[i + 1]);
    const double c2 = row2 ? dist2d(p0.x - p3.x, p0.y - p3.y) : 0.0, r2 = row2 ? __dadd_rn(D[i], D[i + 2]) : 0.0;
    const double c3 = row3 ? dist2d(p0.x - p4.x, p0.y - p4.y) : 0.0, r3 = row3 ? __dadd_rn(D[i], D[i + 3]) : 0.0;
    for (int j = sub; j < n; j += G) {
      const double2 pj = P[j], pj1 = P[j + 1];
      const double dj = D[j];
      const double e1 = dist2d(pj.x - p1.x, pj.y - p1.y), e2 = dist2d(pj.x - p2.x, pj.y - p2.y), e3 = dist2d(pj.x - p3.x, pj.y - p3.y);
      const double f1 = dist2d(pj1.x - p1.x, pj1.y - p1.y), f2 = dist2d(pj1.x - p2.x, pj1.y - p2.y),
                   f3 = dist2d(pj1.x - p3.x, pj1.y - p3.y);
      // delta = ((|P_i P_i+L+1| + |P_j a|) + |b P_j+1|) - ((d_i + d_i+L) + d_j), every operation rounded on its own
      const double rem1 = __dadd_rn(r1, dj), rem2 = __dadd_rn(r2, dj), rem3 = __dadd_rn(r3, dj);
      const double d0 = __dsub_rn(__dadd_rn(__dadd_rn(c1, e1), f1), rem1);
      const double d1 = __dsub_rn(__dadd_rn(__dadd_rn(c2, e1), f2), rem2);
      const double d2 = __dsub_rn(__dadd_rn(__dadd_rn(c2, e2), f1), rem2);
      const double d3 = __dsub_rn(__dadd_rn(__dadd_rn(c3, e1), f3), rem3);
      const double d4 = __dsub_rn(__dadd_rn(__dadd_rn(c3, e3), f1), rem3);
      const bool left = j < i;
      const bool ok1 = left || j > i + 1, ok2 = row2 && (left || j > i + 2), ok3 = row3 && (left || j > i + 3);
      double mn = ok1 ? d0 : INFINITY;                           // the lowest delta of the pair's variants, the lowest v on a tie
      int v = 0;
      if (ok2 && d1 < mn) mn = d1, v = 1;
      if (ok2 && d2 < mn) mn = d2, v = 2;
      if (ok3 && d3 < mn) mn = d3, v = 3;
      if (ok3 && d4 < mn) mn = d4, v = 4;
      const int c = v * n + j;
      if (better_col(mn, c, bv, bc)) bv = mn, bc = c;
    }
  }
  group_best(bv, bc, G);
  *value = bv;
  *code = bv < kThreshold ? bc : -1;
}

// Step 2 of the multi-move 2-opt over the proposals in rowkey / rowj, one thread per row: per round a live proposal wins iff no
// other live proposal whose range meets its own has a lower key; the winners leave and every live proposal that meets a winner
// is dropped.  Returns the number of winners (in every thread), their rows in winners[].
__device__ __forceinline__ int win_select(WinLds& s, int rows, int m, bool or_opt, int select_rounds) {
  const int tid = threadIdx.x;
  const unsigned long long* rowkey = s.rowkey();
  int* live = s.live();
  int* winners = s.winners();
  const PhaseRange range{s.rowj(), m, or_opt};
  bool alive = tid < rows && range.proposes(tid);
  int a = 0, b = 0;
  unsigned long long key = 0;
  if (alive) {
    range(tid, &a, &b);
    key = rowkey[tid];
  }
  if (tid == 0) s.cnt[1] = 0;
  int base = 0;
  for (int round = 0; round < select_rounds; ++round) {
    if (tid == 0) s.cnt[0] = 0;
    __syncthreads();
    if (alive) live[atomicAdd(&s.cnt[0], 1)] = pack_range(a, b, tid);
    __syncthreads();
    const int nlive = s.cnt[0];                                  // uniform over the block
    if (nlive == 0) break;
    bool win = alive;
    for (int q = 0; win && q < nlive; ++q) {
      const int p = live[q], a2 = p & 1023, b2 = (p >> 10) & 2047, r2 = p >> 21;
      if (r2 != tid && a < b2 && a2 < b && key_less(rowkey[r2], r2, key, tid)) win = false;
    }
    if (win) {
      winners[atomicAdd(&s.cnt[1], 1)] = tid;
      alive = false;
    }
    __syncthreads();
    const int total = s.cnt[1];
    for (int q = base; alive && q < total; ++q) {                // it shares a position with a winner of this round
      int wa, wb;
      range(winners[q], &wa, &wb);
      if (a < wb && wa < b) alive = false;
    }
    base = total;
  }
  __syncthreads();
  return s.cnt[1];
}

// one sweep of the candidate path in the phase `or_opt`; returns the moves it applied (uniform over the block), 0: no proposal
__device__ __forceinline__ int win_sweep(WinLds& s, int m, bool or_opt, int select_rounds, int G, int shift) {
  win_prep(s, m);
  const int i = threadIdx.x >> shift, sub = threadIdx.x & (G - 1);
  double v;
  int code;
  win_row_best(s, m, or_opt, i, sub, G, &v, &code);
  __syncthreads();                                               // tp is read: the region becomes the row bests
  const int rows = or_opt ? m - 1 : m - 2;
  if (sub == 0 && i < rows) {
    s.rowkey()[i] = ordered_bits(v);
    s.rowj()[i] = code;
  }
  __syncthreads();
  const int total = win_select(s, rows, m, or_opt, select_rounds);
  if (total == 0) return 0;
  if (or_opt)
    or_opt_winners(s.path, s.stage(), s.winners(), s.rowj(), m, total);
  else
    reverse_winners(s.path, s.winners(), s.rowj(), total);
  __syncthreads();
  return total;
}

// the descent of difusco_tsp_multi_local_search_ragged on the candidate path: rounds of a 2-opt and an Or-opt phase
__device__ __forceinline__ void win_descent(WinLds& s, int m, long long max_iterations, int max_rounds, int select_rounds, int G,
                                            int shift, long long* sweeps, long long* moves) {
  long long total = 0;
  for (int round = 0; round < max_rounds && total < max_iterations; ++round) {
    bool or_moved = false;
    for (int phase = 0; phase < 2 && total < max_iterations; ++phase)
      while (total < max_iterations) {
        const int won = win_sweep(s, m, phase == 1, select_rounds, G, shift);
        if (won == 0) break;
        total += 1;
        *moves += won;
        or_moved |= phase == 1;
      }
    if (!or_moved) break;
  }
  *sweeps += total;
}

// the length of the candidate path in the fixed association of tour_length, n := m <= 1024: s_r = d_r, then the halving tree
__device__ __forceinline__ double win_length(WinLds& s, int m) {
  win_prep(s, m);
  double* part = s.part();
  const double d = (int)threadIdx.x < m ? __dadd_rn(0.0, s.D[threadIdx.x]) : 0.0;
  __syncthreads();                                               // D is computed from tp, which part overlies
  part[threadIdx.x] = d;
  __syncthreads();
  for (int h = kLenParts / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] = __dadd_rn(part[threadIdx.x], part[threadIdx.x + h]);
    __syncthreads();
  }
  const double len = part[0];
  __syncthreads();
  return len;
}

// wave 0: the draws of kick `kick` of a path of m edges (kick_draws of or_opt_multi.hip, uniform cuts, n := m)
__device__ __forceinline__ void win_kick_draws(WinLds& s, unsigned long long seed, unsigned long long offset, int kick_size,
                                               int span, int m) {
  const int c = threadIdx.x;
  const unsigned lc = (unsigned)span < (unsigned)(m - 1) / 2 ? (unsigned)span : (unsigned)(m - 1) / 2;
  int a = 0, b = 0, l1 = 0, keep = 0;
  if (c < kick_size) {
    uint32_t w[4];
    Philox::run(seed, offset, (uint64_t)c, w);
    l1 = 1 + (int)(w[1] % lc);
    const int l2 = 1 + (int)(w[2] % lc);
    a = 1 + (int)(w[0] % (unsigned)(m - l1 - l2));
    b = a + l1 + l2;
    keep = 1;
  }
  for (int e = 0; e < kick_size; ++e) {                          // lane e's flag is final when e comes up
    const int ae = __shfl(a, e), be = __shfl(b, e), ke = __shfl(keep, e);
    if (c > e && ke && a < be && ae < b) keep = 0;
  }
  s.ka[c] = a, s.kl1[c] = l1, s.kb[c] = b, s.kkeep[c] = keep;
}

// One block per window of pass `pass`.  Reads the tour, writes the positions lo .. lo + m - 1 of the candidate (and position n
// behind the last window): the neighbour writes the shared end, which never moves.
__global__ __launch_bounds__(kSelectThreads) void win_search_kernel(
    const double* __restrict__ points, const int* __restrict__ tours, int* __restrict__ cand, const WinDesc* __restrict__ desc,
    const WinTour* __restrict__ tab, const unsigned long long* __restrict__ seeds, const unsigned long long* __restrict__ offsets,
    WinStat* __restrict__ stats, int pass, int kicks, int kick_size, int span, long long max_iterations, int max_rounds,
    int select_rounds) {
  __shared__ WinLds s;
  const WinDesc w = desc[blockIdx.x];
  const WinTour t = tab[w.tour];
  const int m = w.m, tid = threadIdx.x;
  const int* src = tours + t.closed + w.lo;
  int* dst = cand + t.closed + w.lo;
  const int last = w.lo + m == t.n ? m : m - 1;                  // the last position this block writes
  if (m < kWinSkip) {
    for (int k = tid; k <= last; k += kSelectThreads) dst[k] = src[k];
    return;
  }
  const double* pts = points + t.points;
  for (int l = tid; l <= m; l += kSelectThreads) {
    const int c = src[l];
    s.C[l] = make_double2(pts[2 * c], pts[2 * c + 1]);
    s.path[l] = l;
  }
  __syncthreads();
  int G = 1, shift = 0;                                          // lanes per row: rows <= m - 1, so (m - 1) G <= 1024
  while (G < 64 && 2 * G * m <= kSelectThreads) G *= 2, shift += 1;
  long long sweeps = 0, moves = 0, swapped = 0;
  int kept = 0, improved = 0;
  win_descent(s, m, max_iterations, max_rounds, select_rounds, G, shift, &sweeps, &moves);
  double inc_len = win_length(s, m);
  for (int k = tid; k <= m; k += kSelectThreads) s.inc[k] = s.path[k];
  const unsigned long long seed = seeds[w.tour];
  const unsigned long long first = offsets[w.tour] + ((unsigned long long)pass * (unsigned long long)t.stride +
                                                      (unsigned long long)w.index) * (unsigned long long)kicks;
  for (int kick = 0; kick < kicks; ++kick) {
    if (tid < 64) win_kick_draws(s, seed, first + (unsigned long long)kick, kick_size, span, m);
    __syncthreads();                                             // and path == inc: the copy above or the one below is complete
    kick_swaps(s.path, s.inc, kick_size, s.ka, s.kl1, s.kb, s.kkeep);
    if (tid == 0)
      for (int c = 0; c < kick_size; ++c) swapped += s.kkeep[c];
    __syncthreads();
    win_descent(s, m, max_iterations, max_rounds, select_rounds, G, shift, &sweeps, &moves);
    const double len = win_length(s, m);
    const bool take = len <= inc_len;                            // uniform over the block
    if (take) {
      for (int k = tid; k <= m; k += kSelectThreads) s.inc[k] = s.path[k];
      kept += 1;
      improved += len < inc_len;
      inc_len = len;
    } else {
      for (int k = tid; k <= m; k += kSelectThreads) s.path[k] = s.inc[k];
    }
  }
  __syncthreads();
  for (int k = tid; k <= last; k += kSelectThreads) dst[k] = src[s.inc[k]];
  if (tid == 0) {
    WinStat* st = stats + w.tour;
    if (kept) atomicAdd(&st->kicks_kept, kept);
    if (improved) atomicAdd(&st->kicks_improved, improved);
    if (swapped) atomicAdd((unsigned long long*)&st->swapped, (unsigned long long)swapped);
    if (sweeps) atomicAdd((unsigned long long*)&st->sweeps, (unsigned long long)sweeps);
    if (moves) atomicAdd((unsigned long long*)&st->moves, (unsigned long long)moves);
  }
}

// One block per tour: X = `next` replaces T = `cur` iff len(X) <= len(T), the tour-level len; both arrays hold the kept tour
// afterwards.  first: len(T) is the tour's first_length; count: a kept X counts in passes_kept.
__global__ __launch_bounds__(kSelectThreads) void win_keep_kernel(const double* __restrict__ points, int* __restrict__ cur,
                                                                  int* __restrict__ next, const WinTour* __restrict__ tab,
                                                                  WinStat* __restrict__ stats, int first, int count) {
  __shared__ double part[kLenParts];
  const WinTour t = tab[blockIdx.x];
  int* T = cur + t.closed;
  int* X = next + t.closed;
  const double len_t = tour_length(points + t.points, T, t.n, part);
  const double len_x = tour_length(points + t.points, X, t.n, part);
  const bool take = len_x <= len_t;                              // uniform over the block
  if (take)
    for (int k = threadIdx.x; k <= t.n; k += kSelectThreads) T[k] = X[k];
  else
    for (int k = threadIdx.x; k <= t.n; k += kSelectThreads) X[k] = T[k];
  if (threadIdx.x == 0) {
    WinStat* st = stats + blockIdx.x;
    if (first) st->first_length = len_t;
    st->final_length = take ? len_x : len_t;
    if (count && take) st->passes_kept += 1;
  }
}

struct WinLayout {         // byte offsets behind the workspace of the descents
  size_t descent, cand, tab, stats, even, odd, total;
  int tours;
  long long closed;
};

struct WinTables {
  std::vector<WinTour> tours;
  std::vector<WinDesc> even, odd;
  std::vector<long long> searched_even, searched_odd;   // per tour: the windows of a pass that are searched
};

// the windows of a tour of n cities on a pass of offset o: the cuts {0, n} and every o + w W strictly between them
void win_windows(int tour, int n, int W, int o, std::vector<WinDesc>* out, long long* count, long long* searched) {
  int lo = 0, index = 0;
  for (long long cut = o > 0 ? o : W;; cut += W) {
    const int hi = cut < n ? (int)cut : n;
    if (out) out->push_back(WinDesc{tour, lo, hi - lo, index});
    *count += 1;
    *searched += hi - lo >= kWinSkip;
    index += 1;
    lo = hi;
    if (hi == n) break;
  }
}

constexpr const char* kWho = "tsp_window_search_ragged";

// the group arrays and `window` are checked; lays the workspace out and, with `tabs`, builds the tables
int win_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, int window, WinLayout* L,
               WinTables* tabs) {
  size_t descent = 0;
  const int rc = mls_descent_workspace_bytes(who, groups, group_n, group_tours, &descent);
  if (rc != DIFUSCO_OK) return rc;
  if (window < kWinMin || window > kWinMax)
    return set_error(DIFUSCO_EINVAL, "%s: window = %d, needs %d .. %d", who, window, kWinMin, kWinMax);
  long long T = 0, closed = 0, points = 0, even = 0, odd = 0;
  for (int g = 0; g < groups; ++g) {
    const int n = group_n[g];
    for (int p = 0; p < group_tours[g]; ++p, ++T) {
      long long se = 0, so = 0;
      win_windows((int)T, n, window, 0, tabs ? &tabs->even : nullptr, &even, &se);
      win_windows((int)T, n, window, window / 2, tabs ? &tabs->odd : nullptr, &odd, &so);
      if (tabs) {
        tabs->tours.push_back(WinTour{n, (n + window - 1) / window + 1, points, closed});
        tabs->searched_even.push_back(se), tabs->searched_odd.push_back(so);
      }
      closed += (long long)n + 1;
    }
    points += 2LL * n;
  }
  size_t off = up256(descent);
  auto take = [&off](size_t bytes) {
    const size_t at = off;
    off += up256(bytes);
    return at;
  };
  L->descent = descent;
  L->cand = take(sizeof(int) * (size_t)closed);
  L->tab = take(sizeof(WinTour) * (size_t)T);
  L->stats = take(sizeof(WinStat) * (size_t)T);
  L->even = take(sizeof(WinDesc) * (size_t)even);
  L->odd = take(sizeof(WinDesc) * (size_t)odd);
  L->total = off;
  L->tours = (int)T;
  L->closed = closed;
  return DIFUSCO_OK;
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_window_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int32_t window,
                                                     size_t* bytes) {
  using namespace difusco;
  const char* who = "tsp_window_search_ragged_workspace_bytes";
  if (!bytes) return set_error(DIFUSCO_EINVAL, "%s: bytes is null", who);
  WinLayout lay;
  const int rc = win_layout(who, groups, group_n, group_tours, window, &lay, nullptr);
  if (rc == DIFUSCO_OK) *bytes = lay.total;
  return rc;
}

int difusco_tsp_window_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                     int32_t* tours, int64_t max_iterations, int max_rounds, int select_rounds, int32_t kicks,
                                     int32_t kick_size, int32_t span, const uint64_t* tour_seeds, const uint64_t* tour_offsets,
                                     int32_t window, int32_t passes, void* workspace, size_t workspace_bytes,
                                     int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out, int32_t* rounds_out,
                                     int64_t* two_opt_moves_out, int64_t* or_opt_moves_out, int32_t* kicks_kept_out,
                                     int32_t* kicks_improved_out, int64_t* segments_swapped_out, double* first_length_out,
                                     double* final_length_out, int32_t* passes_kept_out, int32_t* windows_searched_out,
                                     int64_t* window_sweeps_out, int64_t* window_moves_out, int32_t* closing_sweeps_out,
                                     void* stream) {
  using namespace difusco;
  WinLayout lay;
  WinTables tabs;
  int rc = win_layout(kWho, groups, group_n, group_tours, window, &lay, &tabs);
  if (rc != DIFUSCO_OK) return rc;
  if (!points || !tours || !workspace || !two_opt_sweeps_out || !or_opt_sweeps_out || !rounds_out || !two_opt_moves_out ||
      !or_opt_moves_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "%s: needs non-null device arrays, the five host output arrays [groups] and "
                                     "max_iterations >= 0", kWho);
  if (!tour_seeds || !tour_offsets || !kicks_kept_out || !kicks_improved_out || !segments_swapped_out || !first_length_out ||
      !final_length_out || !passes_kept_out || !windows_searched_out || !window_sweeps_out || !window_moves_out ||
      !closing_sweeps_out)
    return set_error(DIFUSCO_EINVAL, "%s: needs the device arrays tour_seeds / tour_offsets and the ten host output arrays [tours]",
                     kWho);
  if (max_rounds < 1) return set_error(DIFUSCO_EINVAL, "%s: max_rounds = %d, needs at least 1", kWho, max_rounds);
  if (select_rounds < 1) return set_error(DIFUSCO_EINVAL, "%s: select_rounds = %d, needs at least 1", kWho, select_rounds);
  if (kicks < 0 || kicks > kWinMaxKicks)
    return set_error(DIFUSCO_EINVAL, "%s: kicks = %d, needs 0 .. %d", kWho, (int)kicks, kWinMaxKicks);
  if (kick_size < 1 || kick_size > kMaxKickSize)
    return set_error(DIFUSCO_EINVAL, "%s: kick_size = %d, needs 1 .. %d", kWho, (int)kick_size, kMaxKickSize);
  if (span < 1) return set_error(DIFUSCO_EINVAL, "%s: span = %d < 1", kWho, (int)span);
  if (passes < 1) return set_error(DIFUSCO_EINVAL, "%s: passes = %d, needs at least 1", kWho, (int)passes);
  const int T = lay.tours;
  for (int b = 0; b < T; ++b)                                    // R C max(K, 1) < 2^32: the streams of two copies cannot meet
    if ((unsigned long long)passes * (unsigned long long)tabs.tours[b].stride * (unsigned long long)(kicks > 1 ? kicks : 1) >= (1ull << 32))
      return set_error(DIFUSCO_EINVAL, "%s: passes = %d with %d windows and %d kicks each needs 2^32 or more Philox offsets per tour",
                       kWho, (int)passes, tabs.tours[b].stride, (int)kicks);
  if (workspace_bytes < lay.total)
    return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", kWho, workspace_bytes, lay.total);

  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* cand = (int*)(ws + lay.cand);
  WinTour* d_tab = (WinTour*)(ws + lay.tab);
  WinStat* d_stats = (WinStat*)(ws + lay.stats);
  WinDesc* d_desc[2] = {(WinDesc*)(ws + lay.even), (WinDesc*)(ws + lay.odd)};
  const std::vector<WinDesc>* h_desc[2] = {&tabs.even, &tabs.odd};
  // 1. the first descent
  rc = mls_descent(kWho, groups, group_n, group_tours, points, tours, max_iterations, max_rounds, select_rounds, workspace,
                   lay.descent, two_opt_sweeps_out, or_opt_sweeps_out, rounds_out, two_opt_moves_out, or_opt_moves_out, nullptr, s);
  if (rc != DIFUSCO_OK) return rc;
  // 2. the passes: the tables once, then two launches per pass and no synchronisation
  hipError_t er = hipMemcpyAsync(d_tab, tabs.tours.data(), sizeof(WinTour) * T, hipMemcpyHostToDevice, s);
  for (int par = 0; par < 2 && er == hipSuccess; ++par)
    er = hipMemcpyAsync(d_desc[par], h_desc[par]->data(), sizeof(WinDesc) * h_desc[par]->size(), hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(d_stats, 0, sizeof(WinStat) * T, s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s setup: %s", kWho, hipGetErrorString(er));
  const unsigned long long* seeds = (const unsigned long long*)tour_seeds;
  const unsigned long long* offsets = (const unsigned long long*)tour_offsets;
  for (int r = 0; r < passes; ++r) {
    const int par = r & 1;
    hipLaunchKernelGGL(win_search_kernel, dim3((unsigned)h_desc[par]->size()), dim3(kSelectThreads), 0, s, points, tours, cand,
                       d_desc[par], d_tab, seeds, offsets, d_stats, r, (int)kicks, (int)kick_size, (int)span,
                       (long long)max_iterations, max_rounds, select_rounds);
    hipLaunchKernelGGL(win_keep_kernel, dim3(T), dim3(kSelectThreads), 0, s, points, tours, cand, d_tab, d_stats, r == 0, 1);
  }
  // 3. the closing descent of T_R-1 (the candidates hold a copy of it), kept iff not longer
  std::vector<int64_t> two(groups), orr(groups), m2(groups), mo(groups), tour_sweeps(T, 0);
  std::vector<int32_t> rounds(groups);
  rc = mls_descent(kWho, groups, group_n, group_tours, points, tours, max_iterations, max_rounds, select_rounds, workspace,
                   lay.descent, two.data(), orr.data(), rounds.data(), m2.data(), mo.data(), tour_sweeps.data(), s);
  if (rc != DIFUSCO_OK) return rc;
  for (int g = 0; g < groups; ++g) {
    two_opt_sweeps_out[g] += two[g], or_opt_sweeps_out[g] += orr[g];
    two_opt_moves_out[g] += m2[g], or_opt_moves_out[g] += mo[g];
    if (rounds[g] > rounds_out[g]) rounds_out[g] = rounds[g];
  }
  hipLaunchKernelGGL(win_keep_kernel, dim3(T), dim3(kSelectThreads), 0, s, points, cand, tours, d_tab, d_stats, 0, 0);
  std::vector<WinStat> stats(T);
  er = hipMemcpyAsync(stats.data(), d_stats, sizeof(WinStat) * T, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s counters: %s", kWho, hipGetErrorString(er));
  for (int b = 0; b < T; ++b) {
    const WinStat& x = stats[b];
    kicks_kept_out[b] = x.kicks_kept;
    kicks_improved_out[b] = x.kicks_improved;
    segments_swapped_out[b] = x.swapped;
    first_length_out[b] = x.first_length;
    final_length_out[b] = x.final_length;
    passes_kept_out[b] = x.passes_kept;
    windows_searched_out[b] = (int32_t)(tabs.searched_even[b] * ((passes + 1) / 2) + tabs.searched_odd[b] * (passes / 2));
    window_sweeps_out[b] = x.sweeps;
    window_moves_out[b] = x.moves;
    closing_sweeps_out[b] = (int32_t)tour_sweeps[b];
  }
  return DIFUSCO_OK;
}

}  // extern "C"
