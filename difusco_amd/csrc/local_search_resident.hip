// The 2-opt + Or-opt local search with one resident block per group (difusco_tsp_local_search_resident).  The rule is the one of
// difusco_tsp_local_search_ragged (or_opt.hip), which this entry must equal bit for bit: rounds of (exact 2-opt phase, Or-opt
// phase), max_iterations per phase, the threshold -1e-6, flat-index ties, one evaluated (and possibly applied) 2-opt move at
// max_iterations = 0, the stop after a round with b = 0 or after max_rounds rounds.  The pieces are the shared ones: dist2d,
// change64, better and prep_entry (two_opt_common.h), the team split of the 2-opt pairs (resident_team.h), apply_or_opt_move
// and the variants (or_opt_move.h); the Or-opt delta is evaluated in the operation order of or_opt_tile (or_opt.hip):
// add = (close + |P_j a|) + |b P_j+1|, rem = (d_i + d_i+L) + d_j, delta = add - rem, every operation rounded on its own.
//
// Why a block can run alone: every step of the rule is local to a group.  A block runs the steps of ITS group from the first
// sweep to the stop that ends it; the only word two blocks both touch is the count of stopped groups (an integer atomic).
//
// LDS of a block, S = the cell capacity of the launch (a cell is one entry of a closed tour: P (n + 1) cells per group; S is the
// call's largest group, a multiple of 4) and T = its largest number of tours (a multiple of 4):
//   double2 [S]  tp      points in tour order                                16 B per cell
//   double2 [S]  pts     the group's n points in city order (n < S)           16
//   Best    [T]  chosen  the best move of every tour                         16 B per tour
//   double  [S]  dlen    |P_k - P_k+1|                                        8
//   int     [S]  tour                                                         4
//   int     [S]  stage   the stretch an Or-opt move shifts                    4
// = 48 S + 16 T bytes.  A tour has at least 5 cells (n >= 4), so T <= S / 5 rounded up to a multiple of 4 and a group of
// kMaxCells = 3072 cells needs at most 48 * 3072 + 16 * 616 = 157,312 B, plus 272 B of static LDS (the wave partials and the
// group minimum): 157,584 of the CU's 163,840 B.  The limit is the one of the resident 2-opt.
//
// After a move of either kind the tour entries change first (the reversal of apply_move, or apply_or_opt_move through `stage`),
// then tp and dlen of every cell are written again by prep_entry itself, with `pts` as its points: tp[k] is a copy of
// points[tour[k]] and dlen[k] the distance of the two copies, exactly as the launched prep kernel leaves them.  dlen is never
// updated incrementally.
//
// The 2-opt sweep is the team scheme of two_opt_resident.hip: the waves of the block form `teams` teams of whole waves (block
// waves / P, at least one wave), a team sweeps one tour per round, a thread takes every (team size)-th pair of the triangle.
// The Or-opt sweep of a tour gives a wave of the team units of (64 columns j, a chunk of rows i): a lane keeps its column
// (P_j, P_j+1, d_j) and the six distances e_k = |P_j P_i+k|, f_k = |P_j+1 P_i+k|, k = 1..3, in registers and walks the rows
// upwards, so a pair (i, j) costs two new square roots for all five variants (dist2d squares its differences: a carried value is
// the same bits).  The terms of a row alone: lane l of the wave computes |P_i P_i+2|, |P_i P_i+3|, |P_i P_i+4| of row r0 + l
// for 64 rows at a time and the wave reads them lane by lane; d_i + d_i+L comes from dlen.  Both sides of the diagonal are
// covered: a column block spans all j.  The result does not depend on the split: better() is a strict order on (value, flat
// index) pairs, a NaN never wins and -0.0 never replaces +0.0.
//
// The state of a group (phase, round, iterations of the phase, the two counters) lives in global memory between launches; a
// launch applies at most steps_per_launch steps (a 2-opt move of the group or a counted Or-opt iteration) and ends when it
// would apply one more - that sweep is repeated by the next launch - or when the group stops.
//
// Loop bounds: steps of a launch <= steps_per_launch; sweeps of a launch <= 3 steps_per_launch + 3 (at most two sweeps without a
// move lie between two steps: the end of an Or-opt phase, then the end of a 2-opt phase; a third ends the group); rounds of a
// sweep <= tours of the group; 2-opt pairs of a thread <= pairs of the tour / team size + 1, its row search <= n turns per
// sweep; Or-opt units of a wave <= ceil(n / 64) * max(team waves / ceil(n / 64), 1) / team waves + 1, rows of a unit <= n - 1 in
// fills of 64; cells per thread of a copy, reversal or rebuild <= S / block size + 1, of an Or-opt shift <= n / block size + 1
// per tour, tours one after the other; the cross-wave reduction <= 16 waves; rounds of a group <= max_rounds.  No spin waits, no
// block waits for another.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"
#include "or_opt_move.h"
#include "resident_team.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

constexpr int kMaxCells = 3072;          // difusco_tsp_local_search_resident_max_cells: see the LDS budget above
constexpr int kThreads = 1024;           // the largest block: 16 waves
constexpr int kMinThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kDefaultStepsPerLaunch = 1024;
constexpr int kStaticLds = 16 * kWaves + 16;

constexpr size_t lds_bytes(int S, int T) { return 48 * (size_t)S + 16 * (size_t)T; }
static_assert(lds_bytes(kMaxCells, up4(kMaxCells / 5)) + kStaticLds <= 163840, "a group of kMaxCells cells must fit the LDS of a CU");
static_assert(kMaxCells >= 2048 && kMaxCells % 4 == 0, "TSP-500 with 4 samples is 2004 cells");

struct ResGroup {          // 24 bytes; offsets in elements of the array they index
  int n, tours;
  long long points;        // the group's first coordinate in `points` (doubles)
  long long cells;         // its first tour entry in `tours`
};

struct ResState {          // the loop state of a group between launches, zero at the start of a call (LsGroupState of or_opt.hip)
  int phase, round;        // round: zero-based
  long long phase_iterations, two_opt_iterations, or_opt_iterations;
};

struct Lds {
  double2* tp;
  double2* pts;
  Best* chosen;
  double* dlen;
  int* tour;
  int* stage;
};

__device__ __forceinline__ Lds carve(unsigned char* base, int S, int T) {
  Lds L;
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
__device__ __forceinline__ void rebuild(const Lds& L, int cells, int stride) {
  for (int c = threadIdx.x; c < cells; c += blockDim.x) {      // <= S / block size + 1 turns
    const int p = c / stride, k = c - p * stride, base = p * stride;
    prep_entry((const double*)L.pts, L.tour + base, stride - 1, k, L.tp + base, L.dlen + base);
  }
  __syncthreads();
}

// the exact 2-opt sweep of one tour (P = its tp, D = its dlen): the thread's best move (sweep_exact of two_opt_resident.hip)
__device__ __forceinline__ Best sweep_two_opt(const double2* P, const double* D, int n, const Split& s) {
  Best best{0.0, 0};
  if (!s.work) return best;
  for_pairs(n, s, [&](int i, int j) {
    const double change = change64(P[i], P[i + 1], P[j], P[j + 1], D[i], D[j]);
    const long long idx = (long long)i * n + j;
    if (better(change, idx, best)) best = Best{change, idx};
  });
  return best;
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
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, nw = nt >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Lds L = carve(smem, S, T);
  const double* pts = points + G.points;
  int* gt = tours + G.cells;

  for (int c = tid; c < cells; c += nt) L.tour[c] = gt[c];
  for (int k = tid; k < n; k += nt) L.pts[k] = make_double2(pts[2 * k], pts[2 * k + 1]);
  __syncthreads();
  rebuild(L, cells, stride);

  // teams of whole waves; a leftover wave (team >= teams) only keeps the barriers
  const int wpt = nw / P > 1 ? nw / P : 1, tsize = wpt * 64, teams = nw / wpt, team = wave / wpt;
  const int wv = wave - team * wpt, tt = tid - team * tsize;
  const int rounds = (P + teams - 1) / teams;
  const Split sp{tt, tsize, team < teams};

  int steps = 0;
  for (;;) {                                                   // <= 3 steps_per_launch + 3 sweeps
    for (int round = 0; round < rounds; ++round) {             // <= tours of the group
      const int p = round * teams + team;
      const bool work = sp.work && p < P;
      const int base = p * stride;
      Best best;
      if (s.phase == kTwoOpt) {                                // block uniform
        Split sw = sp;
        sw.work = work;
        best = sweep_two_opt(L.tp + base, L.dlen + base, n, sw);
      } else {
        best = sweep_or_opt(L.tp + base, L.dlen + base, n, wv, wpt, lane, work);
      }
      best = wave_best(best);
      if (lane == 0) wred[wave] = best;
      __syncthreads();
      if (work && tt == 0) {                                   // the team's first thread: its waves' partials
        Best b = wred[wave];
        for (int w = 1; w < wpt; ++w)                          // <= 16 waves
          if (better(wred[wave + w].v, wred[wave + w].idx, b)) b = wred[wave + w];
        L.chosen[p] = b;
      }
      __syncthreads();
    }
    if (wave == 0) {                                           // the minimum over the group's tours
      double m = L.chosen[0].v;
      for (int p = lane; p < P; p += 64) m = L.chosen[p].v < m ? L.chosen[p].v : m;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(m, off, 64);
        m = o < m ? o : m;
      }
      if (lane == 0) gmin = m;
    }
    __syncthreads();
    const bool moving = gmin < kThreshold;                     // 2-opt: all tours move; Or-opt: at least one does
    if (moving && steps == steps_per_launch) break;            // the next launch repeats this sweep and applies its moves
    if (moving) {
      if (s.phase == kTwoOpt) {
        // every tour applies its own best move (apply_move of two_opt_common.h: tour[mi+1 .. mj] reversed, idx = mi * n + mj)
        for (int c = tid; c < cells; c += nt) {
          const int p = c / stride, k = c - p * stride;
          const int idx = (int)L.chosen[p].idx;                // < n * n <= kMaxCells^2
          const int mi = idx / n, mj = idx % n;
          const int len = mj - mi, t = k - (mi + 1);
          if (t >= 0 && t < len / 2) {
            const int x = p * stride + mi + 1 + t, y = p * stride + mj - t;
            const int tmp = L.tour[x];
            L.tour[x] = L.tour[y];
            L.tour[y] = tmp;
          }
        }
      } else {
        for (int p = 0; p < P; ++p) {                          // <= tours of the group, one barrier each
          const Best c = L.chosen[p];
          if (c.v < kThreshold) apply_or_opt_move(L.tour + p * stride, L.stage + p * stride, c.idx, n);   // uniform over the block
        }
      }
      __syncthreads();
      rebuild(L, cells, stride);
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
  for (int c = tid; c < cells; c += nt) gt[c] = L.tour[c];
  if (tid == 0) {
    state[g] = s;
    if (s.phase == kDone) atomicAdd(stopped, 1);
  }
}

// the workspace: the group table, then the state between launches as one block that a single copy reads
struct ResCarve {
  size_t grp, state, state_bytes, total;
};

ResCarve res_carve(int groups) {
  ResCarve c;
  c.grp = 0;
  c.state = up256(sizeof(ResGroup) * (size_t)groups);
  c.state_bytes = sizeof(ResState) * (size_t)groups + 8;       // state [G], stopped
  c.total = c.state + up256(c.state_bytes);
  return c;
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_local_search_resident_max_cells(void) { return difusco::kMaxCells; }

int difusco_tsp_local_search_resident_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes) {
  using namespace difusco;
  const char* who = "local_search_resident_workspace_bytes";
  if (!bytes) return set_error(DIFUSCO_EINVAL, "%s: bytes is null", who);
  int T = 0;
  const int rc = check_groups(who, groups, group_n, group_tours, &T);
  if (rc != DIFUSCO_OK) return rc;
  *bytes = res_carve(groups).total;
  return DIFUSCO_OK;
}

int difusco_tsp_local_search_resident(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                      int32_t* tours, int64_t max_iterations, int max_rounds, int32_t steps_per_launch,
                                      void* workspace, size_t workspace_bytes, int64_t* two_opt_iterations_out,
                                      int64_t* or_opt_iterations_out, int32_t* rounds_out, int32_t* host_syncs_out, void* stream) {
  using namespace difusco;
  const char* who = "tsp_local_search_resident";
  int tours_of_call = 0;
  const int rc = check_groups(who, groups, group_n, group_tours, &tours_of_call);
  if (rc != DIFUSCO_OK) return rc;
  if (!points || !tours || !workspace || !two_opt_iterations_out || !or_opt_iterations_out || !rounds_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "%s: needs non-null device arrays, host two_opt_iterations_out, or_opt_iterations_out and "
                                     "rounds_out [groups] and max_iterations >= 0", who);
  if (max_rounds < 1) return set_error(DIFUSCO_EINVAL, "%s: max_rounds = %d, needs at least 1", who, max_rounds);
  if (steps_per_launch < 0) return set_error(DIFUSCO_EINVAL, "%s: steps_per_launch = %d < 0", who, (int)steps_per_launch);
  const ResCarve c = res_carve(groups);
  if (workspace_bytes < c.total) return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", who, workspace_bytes, c.total);
  // the sizes are host arrays: a group above the limit is refused here, before any GPU work
  std::vector<ResGroup> tab((size_t)groups);
  long long points_at = 0, cells_at = 0, most_pairs = 0;
  int S = 0, T = 0;
  for (int g = 0; g < groups; ++g) {
    const long long n = group_n[g], P = group_tours[g], cells = P * (n + 1);
    if (cells > kMaxCells)
      return set_error(DIFUSCO_EUNSUPPORTED, "%s: group %d has %lld cells (%d tours of %d + 1 entries), above the limit of %d "
                                             "cells per group (difusco_tsp_local_search_resident_max_cells; tours unchanged)",
                       who, g, cells, (int)P, (int)n, kMaxCells);
    tab[(size_t)g] = ResGroup{(int)n, (int)P, points_at, cells_at};
    points_at += 2 * n;
    cells_at += cells;
    S = (int)cells > S ? (int)cells : S;
    T = (int)P > T ? (int)P : T;
    const long long pairs = P * ((n - 1) * (n - 2) / 2);
    most_pairs = pairs > most_pairs ? pairs : most_pairs;
  }
  S = up4(S), T = up4(T);
  // a thread of the largest group gets about 4 pairs of a 2-opt sweep or more: whole waves, 256 .. 1024 threads
  long long threads = ((most_pairs + 3) / 4 + 63) / 64 * 64;
  threads = threads < kMinThreads ? kMinThreads : threads > kThreads ? kThreads : threads;

  char* w = (char*)workspace;
  ResGroup* d_grp = (ResGroup*)(w + c.grp);
  ResState* d_state = (ResState*)(w + c.state);
  int* d_stopped = (int*)(d_state + groups);
  hipStream_t s = (hipStream_t)stream;
  static std::atomic<unsigned long long> attr_devices{0};
  hipError_t er = ensure_max_dynamic_lds(attr_devices, reinterpret_cast<const void*>(&local_search_resident_kernel),
                                         (int)lds_bytes(kMaxCells, up4(kMaxCells / 5)));
  // `tab` lives until the first synchronisation below
  if (er == hipSuccess) er = hipMemcpyAsync(d_grp, tab.data(), sizeof(ResGroup) * (size_t)groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(w + c.state, 0, c.state_bytes, s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s setup: %s", who, hipGetErrorString(er));

  // A launch that does not stop its group applies `per` steps, and a group applies at most max(max_iterations, 1) steps per
  // phase, two phases per round: the launches of a call are bounded by the steps of its slowest group.
  const long long per = steps_per_launch > 0 ? steps_per_launch : kDefaultStepsPerLaunch;
  const long long per_round = 2 * (max_iterations < (1LL << 60) ? (max_iterations > 0 ? max_iterations : 1) : (1LL << 60));
  const long long most_steps = per_round > INT64_MAX / max_rounds ? INT64_MAX : per_round * max_rounds;
  const long long launches = most_steps / per + 1;
  std::vector<long long> raw((c.state_bytes + 7) / 8);
  const ResState* state = (const ResState*)raw.data();
  int syncs = 0;
  for (long long l = 0; l < launches; ++l) {
    // The state is read after every launch: before another one it tells whether every group has stopped, after the last one
    // it is the result.  One synchronisation per launch, none inside a launch.
    hipLaunchKernelGGL(local_search_resident_kernel, dim3((unsigned)groups), dim3((unsigned)threads), lds_bytes(S, T), s, S, T,
                       d_grp, points, (int*)tours, (long long)max_iterations, max_rounds, (int)per, d_state, d_stopped);
    er = hipGetLastError();
    if (er == hipSuccess) er = hipMemcpyAsync(raw.data(), w + c.state, c.state_bytes, hipMemcpyDeviceToHost, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    syncs += 1;
    if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s: %s", who, hipGetErrorString(er));
    if (*(const int*)(state + groups) >= groups) break;
  }
  for (int g = 0; g < groups; ++g) {
    two_opt_iterations_out[g] = (int64_t)state[g].two_opt_iterations;
    or_opt_iterations_out[g] = (int64_t)state[g].or_opt_iterations;
    rounds_out[g] = state[g].round + 1;
  }
  if (host_syncs_out) *host_syncs_out = syncs;
  return DIFUSCO_OK;
}

}  // extern "C"
