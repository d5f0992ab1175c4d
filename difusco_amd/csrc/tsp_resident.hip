// The two tour searches with one resident block per group: the single-move 2-opt (difusco_tsp_two_opt_resident) and the
// 2-opt + Or-opt local search (difusco_tsp_local_search_resident).  Each must equal its launched entry bit for bit.
//
// difusco_tsp_two_opt_resident - the rule of difusco_tsp_two_opt_ragged (two_opt.hip): per tour the (min, first flat index
// i n + j) over j >= i + 2 of change64 starting at (0.0, 0), the group's minimum against -1e-6, every tour of a group that goes
// on reverses tour[i+1 .. j] of its own best move.  The pieces are two_opt_common.h's: dist2d, change64, better, and for method 1
// change32, screen_eps, kScreenMinM / kScreenMaxM and the !(c32 > thr) rule with thr from the tour's m32 as two_opt.hip derives it.
//
// difusco_tsp_local_search_resident - the rule of difusco_tsp_local_search_ragged (or_opt.hip): rounds of (exact 2-opt phase,
// Or-opt phase), max_iterations per phase, the threshold -1e-6, flat-index ties, one evaluated (and possibly applied) 2-opt move
// at max_iterations = 0, the stop after a round with b = 0 or after max_rounds rounds.  The pieces are the shared ones: dist2d,
// change64, better and prep_entry (two_opt_common.h), apply_or_opt_move and the variants (or_opt_move.h); the Or-opt delta is
// evaluated in the operation order of or_opt_tile (or_opt.hip): add = (close + |P_j a|) + |b P_j+1|, rem = (d_i + d_i+L) + d_j,
// delta = add - rem, every operation rounded on its own.
//
// Why a block can run alone: every step of either rule is local to a group.  A block runs the steps of ITS group from the first
// sweep to the stop that ends it; the only word two blocks both touch is the count of stopped groups (an integer atomic).
//
// LDS of a block, S = the cell capacity of the launch (a cell is one entry of a closed tour: P (n + 1) cells per group; S is the
// call's largest group, a multiple of 4) and T = its largest number of tours (a multiple of 4):
//                                                                     2-opt kernel      local search
//   double2 [S]  tp      points in tour order                         16 B per cell     16
//   float4  [S]  q       (P_k, P_k+1) in float32                      16 (method 1)
//   double2 [S]  pts     the group's n points in city order (n < S)                     16
//   Best    [T]  chosen  the best move of every tour                  16 B per tour     16
//   double  [S]  dlen    |P_k - P_k+1|                                 8                 8
//   int     [S]  tour                                                  4                 4
//   float   [S]  d32     fl32(dlen)                                    4 (method 1)
//   int     [S]  stage   the stretch an Or-opt move shifts                               4
//   unsigned[T]  tkey    m32 of every tour as an ordered key           4 (method 1)
// = 48 S + 20 T bytes (28 S + 16 T with method 0) and 48 S + 16 T bytes.  A tour has at least 5 cells (n >= 4), so T <= S / 5
// rounded up to a multiple of 4 and a group of kMaxCells = 3072 cells needs at most 48 * 3072 + 20 * 616 = 159,776 B (the local
// search 157,312 B), plus 272 B of static LDS (the wave partials and two scalars): 160,048 of the CU's 163,840 B.  One limit for
// both entries and both methods.
//
// The two kernels keep their LDS current in different ways, and stay two kernels for it.  The 2-opt kernel: tp[k] is a copy of
// points[tour[k]], a reversal exchanges the copies together with the tour entries, and dlen, q and d32 are then recomputed from
// tp by the arithmetic of prep_entry / prep_screen_entry (two_opt.hip) on the same operands.  The local search: after a move of
// either kind the tour entries change first (the reversal, or apply_or_opt_move through `stage`), then tp and dlen of every cell
// are written again by prep_entry itself, with `pts` as its points, exactly as the launched prep kernel leaves them.  dlen is
// never updated incrementally in either.
//
// Work of a 2-opt sweep: the waves of the block form `teams` teams of whole waves (block waves / P, at least one wave), a team
// sweeps one tour per round, tours round r * teams + team; a leftover wave only keeps the barriers.  In a team a thread takes
// every (team size)-th pair of the row-major order of the triangle j >= i + 2, so every thread has the same number of pairs,
// give or take one.  The Or-opt sweep of a tour gives a wave of the team units of (64 columns j, a chunk of rows i): a lane keeps
// its column (P_j, P_j+1, d_j) and the six distances e_k = |P_j P_i+k|, f_k = |P_j+1 P_i+k|, k = 1..3, in registers and walks
// the rows upwards, so a pair (i, j) costs two new square roots for all five variants (dist2d squares its differences: a carried
// value is the same bits).  The terms of a row alone: lane l of the wave computes |P_i P_i+2|, |P_i P_i+3|, |P_i P_i+4| of row
// r0 + l for 64 rows at a time and the wave reads them lane by lane; d_i + d_i+L comes from dlen.  Both sides of the diagonal
// are covered: a column block spans all j.  No result depends on the split: better() is a strict order on (value, flat index)
// pairs, a NaN never wins and -0.0 never replaces +0.0.
//
// The state of a group lives in global memory between launches.  2-opt: the applied moves, the float64 pairs, the stop flag; a
// launch applies at most moves_per_launch moves.  Local search: phase, round, iterations of the phase, the two counters; a launch
// applies at most steps_per_launch steps (a 2-opt move of the group or a counted Or-opt iteration) and ends when it would apply
// one more - that sweep is repeated by the next launch - or when the group stops.
//
// Loop bounds: moves of a 2-opt launch <= moves_per_launch; steps of a local-search launch <= steps_per_launch, its sweeps
// <= 3 steps_per_launch + 3 (at most two sweeps without a move lie between two steps: the end of an Or-opt phase, then the end
// of a 2-opt phase; a third ends the group), rounds of a group <= max_rounds; rounds of a sweep <= tours of the group; 2-opt pairs
// of a thread <= pairs of the tour / team size + 1, its row search <= n turns per sweep; Or-opt units of a wave
// <= ceil(n / 64) * max(team waves / ceil(n / 64), 1) / team waves + 1, rows of a unit <= n - 1 in fills of 64; cells per thread
// of a copy, reversal or rebuild <= S / block size + 1, of an Or-opt shift <= n / block size + 1 per tour, tours one after the
// other; the cross-wave reduction <= 16 waves.  No spin waits, no block waits for another.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"
#include "or_opt_move.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

constexpr int up4(int x) { return (x + 3) & ~3; }

constexpr int kMaxCells = 3072;          // both _max_cells entries: see the LDS budget above
constexpr int kThreads = 1024;           // the largest block: 16 waves
constexpr int kMinThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kDefaultPerLaunch = 1024;  // moves_per_launch / steps_per_launch = 0
constexpr int kStaticLds = 16 * kWaves + 16;
constexpr int kMaxGroupTours = up4(kMaxCells / 5);

constexpr size_t two_opt_lds_bytes(bool screen, int S, int T) { return screen ? 48 * (size_t)S + 20 * (size_t)T : 28 * (size_t)S + 16 * (size_t)T; }
constexpr size_t local_search_lds_bytes(int S, int T) { return 48 * (size_t)S + 16 * (size_t)T; }
static_assert(two_opt_lds_bytes(true, kMaxCells, kMaxGroupTours) + kStaticLds <= 163840, "a group of kMaxCells cells must fit the LDS of a CU");
static_assert(local_search_lds_bytes(kMaxCells, kMaxGroupTours) + kStaticLds <= 163840, "a group of kMaxCells cells must fit the LDS of a CU");
static_assert(kMaxCells >= 2048 && kMaxCells % 4 == 0, "TSP-500 with 4 samples is 2004 cells");

struct ResGroup {          // 24 bytes; offsets in elements of the array they index
  int n, tours;
  long long points;        // the group's first coordinate in `points` (doubles)
  long long cells;         // its first tour entry in `tours`
};

// ---- what both kernels are made of ----------------------------------------------------------------------------------------

__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const Best o{__shfl_xor(b.v, off, 64), __shfl_xor(b.idx, off, 64)};
    if (better(o.v, o.idx, b)) b = o;
  }
  return b;
}

// The split of a tour's pairs over a team: the pairs (i, j), j >= i + 2, in row-major order (row i holds the n - 2 - i pairs
// (i, i + 2 + q)); a thread takes the pairs first, first + step, ... of that order, step = the team size.  Consecutive threads
// then read consecutive columns and, mostly, one row.  work is false for a thread of a team without a tour.
struct Split {
  int first, step;
  bool work;
};

// f(i, j) for every pair of the thread: <= pairs / team size + 1 calls; the row search runs <= n turns over the whole sweep
template <class F>
__device__ __forceinline__ void for_pairs(int n, const Split& s, F f) {
  int i = 0, q = s.first, len = n - 2;
  for (;;) {
    while (len > 0 && q >= len) {
      q -= len;
      ++i;
      --len;
    }
    if (len <= 0) break;
    f(i, i + 2 + q);
    q += s.step;
  }
}

// A thread's place in the teams of its block: wpt waves per team, tsize threads, `teams` teams; the thread is thread tt of wave
// wv of team `team`.  A leftover wave (team >= teams) only keeps the barriers: sp.work is false.  A sweep takes `rounds` rounds.
struct Team {
  int lane, wave, wpt, tsize, teams, team, wv, tt, rounds;
  Split sp;
};

// `wave` is the caller's: the Or-opt sweep needs it wave uniform
__device__ __forceinline__ Team make_team(int nw, int P, int tid, int wave) {
  const int wpt = nw / P > 1 ? nw / P : 1, tsize = wpt * 64, teams = nw / wpt, team = wave / wpt;
  const int wv = wave - team * wpt, tt = tid - team * tsize;
  const int rounds = (P + teams - 1) / teams;
  return Team{tid & 63, wave, wpt, tsize, teams, team, wv, tt, rounds, Split{tt, tsize, team < teams}};
}

// the best move of tour p from the bests of its team's threads (`work`: the thread belongs to that team), into chosen[p]
__device__ __forceinline__ void team_reduce(Best best, const Team& t, int p, bool work, Best* wred, Best* chosen) {
  best = wave_best(best);
  if (t.lane == 0) wred[t.wave] = best;
  __syncthreads();
  if (work && t.tt == 0) {                                     // the team's first thread: its waves' partials
    Best b = wred[t.wave];
    for (int w = 1; w < t.wpt; ++w)                            // <= 16 waves
      if (better(wred[t.wave + w].v, wred[t.wave + w].idx, b)) b = wred[t.wave + w];
    chosen[p] = b;
  }
  __syncthreads();
}

// the minimum over the group's tours, into *gmin; ends with a barrier
__device__ __forceinline__ void group_min(const Team& t, const Best* chosen, int P, double* gmin) {
  if (t.wave == 0) {
    double m = chosen[0].v;
    for (int p = t.lane; p < P; p += 64) m = chosen[p].v < m ? chosen[p].v : m;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(m, off, 64);
      m = o < m ? o : m;
    }
    if (t.lane == 0) *gmin = m;
  }
  __syncthreads();
}

// the exact 2-opt sweep of one tour (P = its tp, D = its dlen): the thread's best move; counted() once per pair
template <class F>
__device__ __forceinline__ Best sweep_exact(const double2* P, const double* D, int n, const Split& s, F counted) {
  Best best{0.0, 0};
  if (!s.work) return best;
  for_pairs(n, s, [&](int i, int j) {
    const double change = change64(P[i], P[i + 1], P[j], P[j + 1], D[i], D[j]);
    const long long idx = (long long)i * n + j;
    if (better(change, idx, best)) best = Best{change, idx};
    counted();
  });
  return best;
}

// every tour applies its own best move (apply_move of two_opt_common.h: tour[mi+1 .. mj] reversed, idx = mi * n + mj);
// kPoints: the points in tour order with it
template <bool kPoints>
__device__ __forceinline__ void reverse_moves(int* tour, double2* tp, const Best* chosen, int cells, int stride, int n) {
  for (int c = threadIdx.x, nt = blockDim.x; c < cells; c += nt) {      // <= S / block size + 1 turns
    const int p = c / stride, k = c - p * stride;
    const int idx = (int)chosen[p].idx;                        // < n * n <= kMaxCells^2
    const int mi = idx / n, mj = idx % n;
    const int len = mj - mi, t = k - (mi + 1);
    if (t >= 0 && t < len / 2) {
      const int x = p * stride + mi + 1 + t, y = p * stride + mj - t;
      const int tmp = tour[x];
      tour[x] = tour[y];
      tour[y] = tmp;
      if (kPoints) {
        const double2 tq = tp[x];
        tp[x] = tp[y];
        tp[y] = tq;
      }
    }
  }
}

// the tour entries of the group into LDS, each(c, city) per cell, and back
template <class F>
__device__ __forceinline__ void copy_in(int* tour, const int* gt, int cells, F each) {
  for (int c = threadIdx.x, nt = blockDim.x; c < cells; c += nt) {
    const int city = gt[c];
    tour[c] = city;
    each(c, city);
  }
}

__device__ __forceinline__ void copy_out(int* gt, const int* tour, int cells) {
  for (int c = threadIdx.x, nt = blockDim.x; c < cells; c += nt) gt[c] = tour[c];
}

// ---- the 2-opt kernel -----------------------------------------------------------------------------------------------------

struct TwoLds {
  double2* tp;
  float4* q;
  Best* chosen;
  double* dlen;
  int* tour;
  float* d32;
  unsigned* tkey;
};

template <bool kScreen>
__device__ __forceinline__ TwoLds two_carve(unsigned char* base, int S, int T) {
  TwoLds L;
  L.tp = (double2*)base;
  base += 16 * (size_t)S;
  L.q = (float4*)base;
  if (kScreen) base += 16 * (size_t)S;
  L.chosen = (Best*)base;
  base += 16 * (size_t)T;
  L.dlen = (double*)base;
  base += 8 * (size_t)S;
  L.tour = (int*)base;
  base += 4 * (size_t)S;
  L.d32 = (float*)base;
  if (kScreen) base += 4 * (size_t)S;
  L.tkey = (unsigned*)base;
  return L;
}

// dlen / q / d32 of cell c from tp: the arithmetic of prep_entry and prep_screen_entry on the same operands
template <bool kScreen>
__device__ __forceinline__ void edge_entry(const TwoLds& L, int c) {
  const double2 p = L.tp[c], p1 = L.tp[c + 1];
  const double d = dist2d(p.x - p1.x, p.y - p1.y);
  L.dlen[c] = d;
  if (kScreen) {
    L.q[c] = make_float4((float)p.x, (float)p.y, (float)p1.x, (float)p1.y);
    L.d32[c] = (float)d;
  }
}

// the edges of every tour of the group, and m32 of every tour back at the value of the no-op move; ends with a barrier
template <bool kScreen>
__device__ __forceinline__ void two_rebuild(const TwoLds& L, int cells, int stride, int P) {
  for (int c = threadIdx.x; c < cells; c += blockDim.x)        // <= S / block size + 1 turns
    if (c % stride != stride - 1) edge_entry<kScreen>(L, c);   // the closing entry of a tour starts no edge
  if (kScreen)
    for (int p = threadIdx.x; p < P; p += blockDim.x) L.tkey[p] = f32_key(0.0f);
  __syncthreads();
}

// the screen of one tour: min c32 over the thread's pairs (+inf without one)
__device__ __forceinline__ float sweep_screen(const TwoLds& L, int base, int n, const Split& s) {
  float m = INFINITY;
  if (!s.work) return m;
  const float4* Q = L.q + base;
  const float* D = L.d32 + base;
  for_pairs(n, s, [&](int i, int j) { m = fminf(m, change32(Q[i], D[i], Q[j], D[j])); });
  return m;
}

// the screened best move of one tour: float64 for the pairs with !(c32 > thr) only (screened_best_tile of two_opt.hip)
__device__ __forceinline__ Best sweep_screened(const TwoLds& L, int base, int n, const Split& s, float thr, unsigned long long& cnt) {
  Best best{0.0, 0};
  if (!s.work) return best;
  const double2* P = L.tp + base;
  const double* D64 = L.dlen + base;
  const float4* Q = L.q + base;
  const float* D = L.d32 + base;
  for_pairs(n, s, [&](int i, int j) {
    if (!(change32(Q[i], D[i], Q[j], D[j]) > thr)) {
      const double change = change64(P[i], P[i + 1], P[j], P[j + 1], D64[i], D64[j]);
      const long long idx = (long long)i * n + j;
      if (better(change, idx, best)) best = Best{change, idx};
      ++cnt;
    }
  });
  return best;
}

// One block per group.  Between launches the tours are in `tours`, the applied moves in iters[g], the float64 pairs in pairs[g]
// and the stop flag in done[g]; *stopped counts the stopped groups.
template <bool kScreen>
__global__ __launch_bounds__(kThreads) void two_opt_resident_kernel(int S, int T, const ResGroup* __restrict__ grp,
                                                                    const double* __restrict__ points, int* __restrict__ tours,
                                                                    long long max_iterations, int moves_per_launch,
                                                                    long long* __restrict__ iters_g,
                                                                    unsigned long long* __restrict__ pairs_g,
                                                                    int* __restrict__ done, int* stopped) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ Best wred[kWaves];
  __shared__ double gmin;
  __shared__ unsigned long long maxbits;
  const int g = blockIdx.x;
  if (done[g]) return;                                         // a stopped group's block returns at once
  const ResGroup G = grp[g];
  const int n = G.n, P = G.tours, stride = n + 1, cells = P * stride;
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
  const TwoLds L = two_carve<kScreen>(smem, S, T);
  const double* pts = points + G.points;

  copy_in(L.tour, tours + G.cells, cells, [&](int c, int city) { L.tp[c] = make_double2(pts[2 * city], pts[2 * city + 1]); });
  // the group's largest |coordinate| M (bits: non-negative doubles order like their bits, a NaN sorts above inf) decides, for
  // this group alone, whether the screen has a bound
  bool bounded = false;
  double eps = 0.0;
  if (kScreen) {
    if (tid == 0) maxbits = 0;
    __syncthreads();
    unsigned long long m = 0;
    for (int k = tid; k < 2 * n; k += nt) {
      const unsigned long long v = (unsigned long long)__double_as_longlong(fabs(pts[k]));
      m = v > m ? v : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(m, off, 64);
      m = o > m ? o : m;
    }
    if (lane == 0 && m) atomicMax(&maxbits, m);
  }
  __syncthreads();
  if (kScreen) {
    const double M = __longlong_as_double((long long)maxbits);
    bounded = M >= kScreenMinM && M <= kScreenMaxM;            // false for inf and NaN
    eps = screen_eps(M);
  }
  two_rebuild<kScreen>(L, cells, stride, P);
  const Team tm = make_team(nt >> 6, P, tid, tid >> 6);

  // The moves of this launch: at most moves_per_launch, at most what max_iterations leaves, at least one sweep (the reference
  // evaluates once even with max_iterations = 0, and a move it then applies reaches the cap: tsp_utils.py:46-47).
  const long long left = max_iterations - iters_g[g];
  const int lim = left < (long long)moves_per_launch ? (left > 1 ? (int)left : 1) : moves_per_launch;
  const bool capped = left <= (long long)lim;                  // lim applied moves reach max_iterations
  unsigned long long cnt = 0;
  bool stop = false;
  int mv = 0;
  for (;;) {                                                   // <= lim <= moves_per_launch turns
    for (int round = 0; round < tm.rounds; ++round) {          // <= tours of the group
      const int p = round * tm.teams + tm.team;
      Split s = tm.sp;
      s.work = tm.sp.work && p < P;
      const int base = p * stride;
      Best best{0.0, 0};
      if (kScreen && bounded) {                                // block uniform
        const float mine = sweep_screen(L, base, n, s);
        float m = mine;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off, 64));
        if (s.work && lane == 0) {                             // the minimum is order-independent, so m32 is deterministic
          const unsigned key = f32_key(m);
          if (key < L.tkey[p]) atomicMin(&L.tkey[p], key);
        }
        __syncthreads();
        if (s.work) {
          const float m32 = f32_unkey(L.tkey[p]);
          const double upper = fmin(0.0, (double)m32 + eps);   // U >= V*
          const float thr = __double2float_ru(upper + eps);
          if (!(mine > thr)) best = sweep_screened(L, base, n, s, thr, cnt);   // no pair of a skipped thread has !(c32 > thr)
        }
      } else {
        best = sweep_exact(L.tp + base, L.dlen + base, n, s, [&] { ++cnt; });
      }
      team_reduce(best, tm, p, s.work, wred, L.chosen);
    }
    group_min(tm, L.chosen, P, &gmin);
    if (!(gmin < -1e-6)) {                                     // tsp_utils.py:39,44
      stop = true;
      break;
    }
    reverse_moves<true>(L.tour, L.tp, L.chosen, cells, stride, n);
    __syncthreads();
    two_rebuild<kScreen>(L, cells, stride, P);
    if (++mv == lim) {
      stop = capped;
      break;
    }
  }
  copy_out(tours + grp[g].cells, L.tour, cells);               // read again: the offset need not stay live over the move loop
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if (lane == 0 && cnt) atomicAdd(&pairs_g[g], cnt);
  if (tid == 0) {
    iters_g[g] += mv;
    if (stop) {
      done[g] = 1;
      atomicAdd(stopped, 1);
    }
  }
}

// ---- the local search kernel ----------------------------------------------------------------------------------------------

struct ResState {          // the loop state of a group between launches, zero at the start of a call (LsGroupState of or_opt.hip)
  int phase, round;        // round: zero-based
  long long phase_iterations, two_opt_iterations, or_opt_iterations;
};

struct LsLds {
  double2* tp;
  double2* pts;
  Best* chosen;
  double* dlen;
  int* tour;
  int* stage;
};

__device__ __forceinline__ LsLds ls_carve(unsigned char* base, int S, int T) {
  LsLds L;
  L.tp = (double2*)base;
  base += 16 * (size_t)S;
  L.pts = (double2*)base;
  base += 16 * (size_t)S;
  L.chosen = (Best*)base;
  base += 16 * (size_t)T;
  L.dlen = (double*)base;
  base += 8 * (size_t)S;
  L.tour = (int*)base;
  base += 4 * (size_t)S;
  L.stage = (int*)base;
  return L;
}

// tp and dlen of every tour of the group from its tour entries: prep_entry with the LDS copy of the points; ends with a barrier
__device__ __forceinline__ void ls_rebuild(const LsLds& L, int cells, int stride) {
  for (int c = threadIdx.x; c < cells; c += blockDim.x) {      // <= S / block size + 1 turns
    const int p = c / stride, k = c - p * stride, base = p * stride;
    prep_entry((const double*)L.pts, L.tour + base, stride - 1, k, L.tp + base, L.dlen + base);
  }
  __syncthreads();
}

// lane `l` (wave uniform) of x
__device__ __forceinline__ double lane_value(double x, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), l), hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  return __hiloint2double(hi, lo);
}

// The Or-opt sweep of one tour (P = its tp, D = its dlen, n nodes) by a team of `wpt` whole waves, `wv` this wave's number in
// the team (wave uniform): the lane's best move, flat index (v n + i) n + j.  Like or_opt_tile it starts from (0.0, 0).
__device__ __forceinline__ Best sweep_or_opt(const double2* P, const double* D, int n, int wv, int wpt, int lane, bool work) {
  Best best{0.0, 0};
  if (!work) return best;
  const int colblocks = (n + 63) >> 6;
  const int rowchunks = wpt > colblocks ? wpt / colblocks : 1;
  const int rows = n - 1;                                        // i <= n - 2: the last row of L = 1
  const int rpc = (rows + rowchunks - 1) / rowchunks;
  const int units = colblocks * rowchunks;
  const long long nn = (long long)n * n;
  for (int u = wv; u < units; u += wpt) {                        // <= units / team waves + 1 turns
    const int cb = u % colblocks, rc = u / colblocks;
    const int rbeg = rc * rpc, rend = rbeg + rpc < rows ? rbeg + rpc : rows;
    if (rbeg >= rend) continue;
    const int j = cb * 64 + lane, jc = j < n ? j : n - 1;
    const bool in = j < n;
    const double2 pj = P[jc], pj1 = P[jc + 1];
    const double dj = D[jc];
    const double2 s1 = P[rbeg + 1 < n ? rbeg + 1 : n], s2 = P[rbeg + 2 < n ? rbeg + 2 : n], s3 = P[rbeg + 3 < n ? rbeg + 3 : n];
    double e1 = dist2d(pj.x - s1.x, pj.y - s1.y), e2 = dist2d(pj.x - s2.x, pj.y - s2.y), e3 = dist2d(pj.x - s3.x, pj.y - s3.y);
    double f1 = dist2d(pj1.x - s1.x, pj1.y - s1.y), f2 = dist2d(pj1.x - s2.x, pj1.y - s2.y), f3 = dist2d(pj1.x - s3.x, pj1.y - s3.y);
    for (int r0 = rbeg; r0 < rend; r0 += 64) {                   // <= rows / 64 + 1 fills
      // lane l: |P_i P_i+L+1| of row i = r0 + l, 0.0 where the row has no segment of L cities (closing of or_opt_tile)
      const int il = r0 + lane;
      double cl1 = 0.0, cl2 = 0.0, cl3 = 0.0;
      if (il <= n - 2) {
        const double2 p = P[il], q = P[il + 2];
        cl1 = dist2d(p.x - q.x, p.y - q.y);
      }
      if (il <= n - 3) {
        const double2 p = P[il], q = P[il + 3];
        cl2 = dist2d(p.x - q.x, p.y - q.y);
      }
      if (il <= n - 4) {
        const double2 p = P[il], q = P[il + 4];
        cl3 = dist2d(p.x - q.x, p.y - q.y);
      }
      const int rtop = r0 + 64 < rend ? r0 + 64 : rend;
      for (int i = r0; i < rtop; ++i) {                          // <= 64 rows
        const bool row2 = i <= n - 3, row3 = i <= n - 4;
        const double c1 = lane_value(cl1, i - r0), c2 = lane_value(cl2, i - r0), c3 = lane_value(cl3, i - r0);
        const double di = D[i];
        const double r1 = __dadd_rn(di, D[i + 1]);               // i + 1 <= n - 1
        const double r2 = row2 ? __dadd_rn(di, D[row2 ? i + 2 : i]) : 0.0;
        const double r3 = row3 ? __dadd_rn(di, D[row3 ? i + 3 : i]) : 0.0;
        const double2 next = P[i + 4 < n ? i + 4 : n];           // P_i+4, for the row after this one
        // delta = ((|P_i P_i+L+1| + |P_j a|) + |b P_j+1|) - ((d_i + d_i+L) + d_j), every operation rounded on its own
        const double rem1 = __dadd_rn(r1, dj), rem2 = __dadd_rn(r2, dj), rem3 = __dadd_rn(r3, dj);
        const double d0 = __dsub_rn(__dadd_rn(__dadd_rn(c1, e1), f1), rem1);
        const double d1 = __dsub_rn(__dadd_rn(__dadd_rn(c2, e1), f2), rem2);
        const double d2 = __dsub_rn(__dadd_rn(__dadd_rn(c2, e2), f1), rem2);
        const double d3 = __dsub_rn(__dadd_rn(__dadd_rn(c3, e1), f3), rem3);
        const double d4 = __dsub_rn(__dadd_rn(__dadd_rn(c3, e3), f1), rem3);
        const bool left = j < i;
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
        e1 = e2;
        e2 = e3;
        e3 = dist2d(pj.x - next.x, pj.y - next.y);
        f1 = f2;
        f2 = f3;
        f3 = dist2d(pj1.x - next.x, pj1.y - next.y);
      }
    }
  }
  return best;
}

// One block per group.  Between launches the tours are in `tours` and the loop state in state[g]; *stopped counts the stopped
// groups.
__global__ __launch_bounds__(kThreads) void local_search_resident_kernel(int S, int T, const ResGroup* __restrict__ grp,
                                                                         const double* __restrict__ points, int* __restrict__ tours,
                                                                         long long max_iterations, int max_rounds, int steps_per_launch,
                                                                         ResState* __restrict__ state, int* stopped) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ Best wred[kWaves];
  __shared__ double gmin;
  const int g = blockIdx.x;
  ResState s = state[g];
  if (s.phase == kDone) return;                                // a stopped group's block returns at once
  const ResGroup G = grp[g];
  const int n = G.n, P = G.tours, stride = n + 1, cells = P * stride;
  const int tid = threadIdx.x, nt = blockDim.x;
  const LsLds L = ls_carve(smem, S, T);
  const double* pts = points + G.points;
  int* gt = tours + G.cells;

  copy_in(L.tour, gt, cells, [](int, int) {});
  for (int k = tid; k < n; k += nt) L.pts[k] = make_double2(pts[2 * k], pts[2 * k + 1]);
  __syncthreads();
  ls_rebuild(L, cells, stride);
  const Team tm = make_team(nt >> 6, P, tid, __builtin_amdgcn_readfirstlane(tid >> 6));

  int steps = 0;
  for (;;) {                                                   // <= 3 steps_per_launch + 3 sweeps
    for (int round = 0; round < tm.rounds; ++round) {          // <= tours of the group
      const int p = round * tm.teams + tm.team;
      const bool work = tm.sp.work && p < P;
      const int base = p * stride;
      Best best;
      if (s.phase == kTwoOpt) {                                // block uniform
        Split sw = tm.sp;
        sw.work = work;
        best = sweep_exact(L.tp + base, L.dlen + base, n, sw, [] {});
      } else {
        best = sweep_or_opt(L.tp + base, L.dlen + base, n, tm.wv, tm.wpt, tm.lane, work);
      }
      team_reduce(best, tm, p, work, wred, L.chosen);
    }
    group_min(tm, L.chosen, P, &gmin);
    const bool moving = gmin < kThreshold;                     // 2-opt: all tours move; Or-opt: at least one does
    if (moving && steps == steps_per_launch) break;            // the next launch repeats this sweep and applies its moves
    if (moving) {
      if (s.phase == kTwoOpt) {
        reverse_moves<false>(L.tour, L.tp, L.chosen, cells, stride, n);
      } else {
        for (int p = 0; p < P; ++p) {                          // <= tours of the group, one barrier each
          const Best c = L.chosen[p];
          if (c.v < kThreshold) apply_or_opt_move(L.tour + p * stride, L.stage + p * stride, c.idx, n);   // uniform over the block
        }
      }
      __syncthreads();
      ls_rebuild(L, cells, stride);
      ++steps;
    }
    // the step of local_search_apply_kernel (or_opt.hip) on the group's state, the same in every thread
    bool phase_ends = !moving;
    if (moving) {
      s.phase_iterations += 1;
      (s.phase == kTwoOpt ? s.two_opt_iterations : s.or_opt_iterations) += 1;
      phase_ends = s.phase_iterations >= max_iterations;       // tsp_utils.py:46-47
    }
    if (phase_ends) {
      if (s.phase == kTwoOpt) {
        s.phase = max_iterations > 0 ? kOrOpt : kDone;         // an Or-opt phase of no iterations applies nothing: b = 0
      } else if (s.phase_iterations == 0 || s.round + 1 >= max_rounds) {
        s.phase = kDone;
      } else {
        s.phase = kTwoOpt;
        s.round += 1;
      }
      s.phase_iterations = 0;
    }
    if (s.phase == kDone) break;
  }
  copy_out(gt, L.tour, cells);
  if (tid == 0) {
    state[g] = s;
    if (s.phase == kDone) atomicAdd(stopped, 1);
  }
}

// ---- the host side: one plan, one workspace layout, one launch loop -------------------------------------------------------

struct ResPlan {
  std::vector<ResGroup> tab;       // the group table
  int S, T, threads;               // the launch's cell and tour capacity (multiples of 4) and its block size
};

// The walk over the groups of a call that check_groups has accepted (the entries run it first: its refusals come before the
// ones of their own arguments).  The sizes are host arrays: a group above the limit is refused here, before any GPU work.
int plan_resident(const char* who, const char* max_cells_entry_name, int groups, const int32_t* group_n, const int32_t* group_tours,
                  ResPlan* plan) {
  plan->tab.resize((size_t)groups);
  long long points_at = 0, cells_at = 0, most_pairs = 0;
  int S = 0, T = 0;
  for (int g = 0; g < groups; ++g) {
    const long long n = group_n[g], P = group_tours[g], cells = P * (n + 1);
    if (cells > kMaxCells)
      return set_error(DIFUSCO_EUNSUPPORTED, "%s: group %d has %lld cells (%d tours of %d + 1 entries), above the limit of %d "
                                             "cells per group (%s; tours unchanged)",
                       who, g, cells, (int)P, (int)n, kMaxCells, max_cells_entry_name);
    plan->tab[(size_t)g] = ResGroup{(int)n, (int)P, points_at, cells_at};
    points_at += 2 * n;
    cells_at += cells;
    S = (int)cells > S ? (int)cells : S;
    T = (int)P > T ? (int)P : T;
    const long long pairs = P * ((n - 1) * (n - 2) / 2);
    most_pairs = pairs > most_pairs ? pairs : most_pairs;
  }
  plan->S = up4(S), plan->T = up4(T);
  // a thread of the largest group gets about 4 pairs of a 2-opt sweep or more: whole waves, 256 .. 1024 threads
  const long long threads = ((most_pairs + 3) / 4 + 63) / 64 * 64;
  plan->threads = (int)(threads < kMinThreads ? kMinThreads : threads > kThreads ? kThreads : threads);
  return DIFUSCO_OK;
}

// the workspace: the group table, then the state between launches as one block that a single copy reads
struct ResCarve {
  size_t grp, state, state_bytes, total;
};

ResCarve res_carve(int groups, size_t state_bytes) {
  ResCarve c;
  c.grp = 0;
  c.state = up256(sizeof(ResGroup) * (size_t)groups);
  c.state_bytes = state_bytes;
  c.total = c.state + up256(state_bytes);
  return c;
}

constexpr size_t two_opt_state_bytes(int groups) { return 20 * (size_t)groups + 8; }                            // iters [G], pairs [G], done [G], stopped
constexpr size_t local_search_state_bytes(int groups) { return sizeof(ResState) * (size_t)groups + 8; }         // state [G], stopped

// The launches of a call: the table goes up, the state starts at zero, then at most `launches` times launch(), whose state is
// read after every launch: before another one it tells whether every group has stopped (the int at byte `stopped_at` of the
// state counts them), after the last one it is the result, left in `state`.  One synchronisation per launch, none inside a
// launch; *syncs counts them.
template <class Launch>
hipError_t run_resident(const ResPlan& plan, const ResCarve& c, void* workspace, long long launches, Launch launch, size_t stopped_at,
                        std::vector<long long>* state, int* syncs, const char** stage, hipStream_t s) {
  const int groups = (int)plan.tab.size();
  char* w = (char*)workspace;
  *stage = " setup";
  // plan.tab lives until the first synchronisation below
  hipError_t er = hipMemcpyAsync(w + c.grp, plan.tab.data(), sizeof(ResGroup) * (size_t)groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(w + c.state, 0, c.state_bytes, s);
  if (er != hipSuccess) return er;
  *stage = "";
  state->assign((c.state_bytes + 7) / 8, 0);
  for (long long l = 0; l < launches; ++l) {
    er = launch();
    if (er == hipSuccess) er = hipMemcpyAsync(state->data(), w + c.state, c.state_bytes, hipMemcpyDeviceToHost, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    *syncs += 1;
    if (er != hipSuccess) return er;
    if (*(const int*)((const char*)state->data() + stopped_at) >= groups) break;
  }
  return hipSuccess;
}

// one launch, one block per group; the first on a device raises the kernel's dynamic LDS limit to a group of kMaxCells cells
template <bool kScreen>
hipError_t launch_two_opt(const ResPlan& plan, hipStream_t s, const ResGroup* grp, const double* points, int* tours, long long max_iterations,
                          int per_launch, long long* iters, unsigned long long* pairs, int* done, int* stopped) {
  static std::atomic<unsigned long long> attr_devices{0};
  const hipError_t er = ensure_max_dynamic_lds(attr_devices, reinterpret_cast<const void*>(&two_opt_resident_kernel<kScreen>),
                                               (int)two_opt_lds_bytes(kScreen, kMaxCells, kMaxGroupTours));
  if (er != hipSuccess) return er;
  hipLaunchKernelGGL(two_opt_resident_kernel<kScreen>, dim3((unsigned)plan.tab.size()), dim3((unsigned)plan.threads),
                     two_opt_lds_bytes(kScreen, plan.S, plan.T), s, plan.S, plan.T, grp, points, tours, max_iterations, per_launch, iters,
                     pairs, done, stopped);
  return hipGetLastError();
}

hipError_t launch_local_search(const ResPlan& plan, hipStream_t s, const ResGroup* grp, const double* points, int* tours,
                               long long max_iterations, int max_rounds, int per_launch, ResState* state, int* stopped) {
  static std::atomic<unsigned long long> attr_devices{0};
  const hipError_t er = ensure_max_dynamic_lds(attr_devices, reinterpret_cast<const void*>(&local_search_resident_kernel),
                                               (int)local_search_lds_bytes(kMaxCells, kMaxGroupTours));
  if (er != hipSuccess) return er;
  hipLaunchKernelGGL(local_search_resident_kernel, dim3((unsigned)plan.tab.size()), dim3((unsigned)plan.threads),
                     local_search_lds_bytes(plan.S, plan.T), s, plan.S, plan.T, grp, points, tours, max_iterations, max_rounds, per_launch,
                     state, stopped);
  return hipGetLastError();
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_two_opt_resident_max_cells(void) { return difusco::kMaxCells; }

int difusco_tsp_two_opt_resident_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int method,
                                                 size_t* bytes) {
  using namespace difusco;
  const char* who = "two_opt_resident_workspace_bytes";
  if (!bytes) return set_error(DIFUSCO_EINVAL, "%s: bytes is null", who);
  int T = 0;
  const int rc = check_groups(who, groups, group_n, group_tours, &T);
  if (rc != DIFUSCO_OK) return rc;
  if (method != 0 && method != 1) return set_error(DIFUSCO_EINVAL, "%s: method %d (0 exact, 1 screened)", who, method);
  *bytes = res_carve(groups, two_opt_state_bytes(groups)).total;
  return DIFUSCO_OK;
}

int difusco_tsp_two_opt_resident(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                 int32_t* tours, int64_t max_iterations, int method, int32_t moves_per_launch, void* workspace,
                                 size_t workspace_bytes, int64_t* iterations_out, int64_t* exact_pairs_out,
                                 int32_t* host_syncs_out, void* stream) {
  using namespace difusco;
  const char* who = "tsp_two_opt_resident";
  int tours_of_call = 0;
  int rc = check_groups(who, groups, group_n, group_tours, &tours_of_call);
  if (rc != DIFUSCO_OK) return rc;
  if (method != 0 && method != 1) return set_error(DIFUSCO_EINVAL, "%s: method %d (0 exact, 1 screened)", who, method);
  if (!points || !tours || !workspace || !iterations_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "%s: needs non-null device arrays, a host iterations_out[groups] and max_iterations >= 0", who);
  if (moves_per_launch < 0) return set_error(DIFUSCO_EINVAL, "%s: moves_per_launch = %d < 0", who, (int)moves_per_launch);
  const ResCarve c = res_carve(groups, two_opt_state_bytes(groups));
  if (workspace_bytes < c.total) return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", who, workspace_bytes, c.total);
  ResPlan plan;
  rc = plan_resident(who, "difusco_tsp_two_opt_resident_max_cells", groups, group_n, group_tours, &plan);
  if (rc != DIFUSCO_OK) return rc;

  char* w = (char*)workspace;
  const ResGroup* d_grp = (const ResGroup*)(w + c.grp);
  long long* d_iters = (long long*)(w + c.state);
  unsigned long long* d_pairs = (unsigned long long*)(d_iters + groups);
  int* d_done = (int*)(d_pairs + groups);
  int* d_stopped = d_done + groups;
  hipStream_t s = (hipStream_t)stream;
  // the reference always evaluates (and may apply) once; at most max_iterations moves are applied (tsp_utils.py:20-47)
  const long long loops = max_iterations > 0 ? max_iterations : 1;
  const long long per = moves_per_launch > 0 ? moves_per_launch : kDefaultPerLaunch;
  const auto launch = [&] {
    return (method == 1 ? launch_two_opt<true> : launch_two_opt<false>)(plan, s, d_grp, points, (int*)tours, (long long)max_iterations,
                                                                        (int)per, d_iters, d_pairs, d_done, d_stopped);
  };
  std::vector<long long> state;
  const char* stage = "";
  int syncs = 0;
  const hipError_t er = run_resident(plan, c, workspace, (loops + per - 1) / per, launch, 20 * (size_t)groups, &state, &syncs, &stage, s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s%s: %s", who, stage, hipGetErrorString(er));
  unsigned long long pairs = 0;
  for (int g = 0; g < groups; ++g) {
    iterations_out[g] = (int64_t)state[(size_t)g];
    pairs += (unsigned long long)state[(size_t)groups + (size_t)g];
  }
  if (exact_pairs_out) *exact_pairs_out = (int64_t)pairs;
  if (host_syncs_out) *host_syncs_out = syncs;
  return DIFUSCO_OK;
}

int difusco_tsp_local_search_resident_max_cells(void) { return difusco::kMaxCells; }

int difusco_tsp_local_search_resident_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes) {
  using namespace difusco;
  const char* who = "local_search_resident_workspace_bytes";
  if (!bytes) return set_error(DIFUSCO_EINVAL, "%s: bytes is null", who);
  int T = 0;
  const int rc = check_groups(who, groups, group_n, group_tours, &T);
  if (rc != DIFUSCO_OK) return rc;
  *bytes = res_carve(groups, local_search_state_bytes(groups)).total;
  return DIFUSCO_OK;
}

int difusco_tsp_local_search_resident(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                      int32_t* tours, int64_t max_iterations, int max_rounds, int32_t steps_per_launch,
                                      void* workspace, size_t workspace_bytes, int64_t* two_opt_iterations_out,
                                      int64_t* or_opt_iterations_out, int32_t* rounds_out, int32_t* host_syncs_out, void* stream) {
  using namespace difusco;
  const char* who = "tsp_local_search_resident";
  int tours_of_call = 0;
  int rc = check_groups(who, groups, group_n, group_tours, &tours_of_call);
  if (rc != DIFUSCO_OK) return rc;
  if (!points || !tours || !workspace || !two_opt_iterations_out || !or_opt_iterations_out || !rounds_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "%s: needs non-null device arrays, host two_opt_iterations_out, or_opt_iterations_out and "
                                     "rounds_out [groups] and max_iterations >= 0", who);
  if (max_rounds < 1) return set_error(DIFUSCO_EINVAL, "%s: max_rounds = %d, needs at least 1", who, max_rounds);
  if (steps_per_launch < 0) return set_error(DIFUSCO_EINVAL, "%s: steps_per_launch = %d < 0", who, (int)steps_per_launch);
  const ResCarve c = res_carve(groups, local_search_state_bytes(groups));
  if (workspace_bytes < c.total) return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", who, workspace_bytes, c.total);
  ResPlan plan;
  rc = plan_resident(who, "difusco_tsp_local_search_resident_max_cells", groups, group_n, group_tours, &plan);
  if (rc != DIFUSCO_OK) return rc;

  char* w = (char*)workspace;
  const ResGroup* d_grp = (const ResGroup*)(w + c.grp);
  ResState* d_state = (ResState*)(w + c.state);
  int* d_stopped = (int*)(d_state + groups);
  hipStream_t s = (hipStream_t)stream;
  // A launch that does not stop its group applies `per` steps, and a group applies at most max(max_iterations, 1) steps per
  // phase, two phases per round: the launches of a call are bounded by the steps of its slowest group.
  const long long per = steps_per_launch > 0 ? steps_per_launch : kDefaultPerLaunch;
  const long long per_round = 2 * (max_iterations < (1LL << 60) ? (max_iterations > 0 ? max_iterations : 1) : (1LL << 60));
  const long long most_steps = per_round > INT64_MAX / max_rounds ? INT64_MAX : per_round * max_rounds;
  const auto launch = [&] {
    return launch_local_search(plan, s, d_grp, points, (int*)tours, (long long)max_iterations, max_rounds, (int)per, d_state, d_stopped);
  };
  std::vector<long long> raw;
  const char* stage = "";
  int syncs = 0;
  const hipError_t er = run_resident(plan, c, workspace, most_steps / per + 1, launch, sizeof(ResState) * (size_t)groups, &raw, &syncs,
                                     &stage, s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s%s: %s", who, stage, hipGetErrorString(er));
  const ResState* state = (const ResState*)raw.data();
  for (int g = 0; g < groups; ++g) {
    two_opt_iterations_out[g] = (int64_t)state[g].two_opt_iterations;
    or_opt_iterations_out[g] = (int64_t)state[g].or_opt_iterations;
    rounds_out[g] = state[g].round + 1;
  }
  if (host_syncs_out) *host_syncs_out = syncs;
  return DIFUSCO_OK;
}

}  // extern "C"
