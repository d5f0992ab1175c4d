// The single-move 2-opt with one resident block per group (difusco_tsp_two_opt_resident).  The rule is the one of
// difusco_tsp_two_opt_ragged (two_opt.hip), which this entry must equal bit for bit: per tour the (min, first flat index i n + j)
// over j >= i + 2 of change64 starting at (0.0, 0), the group's minimum against -1e-6, every tour of a group that goes on
// reverses tour[i+1 .. j] of its own best move.  The pieces are two_opt_common.h's: dist2d, change64, better, and for method 1
// change32, screen_eps, kScreenMinM / kScreenMaxM and the !(c32 > thr) rule with thr from the tour's m32 as two_opt.hip derives it.
//
// Why a block can run alone: every step of the rule is local to a group.  A block runs the moves of ITS group from the first
// sweep to the stop test that ends it; the only words two blocks both touch are the count of stopped groups (an integer atomic).
//
// LDS of a block, S = the cell capacity of the launch (a cell is one entry of a closed tour: P (n + 1) cells per group; S is the
// call's largest group, a multiple of 4) and T = its largest number of tours (a multiple of 4):
//   double2 [S]  tp      points in tour order                                16 B per cell
//   float4  [S]  q       (P_k, P_k+1) in float32                (method 1)   16
//   Best    [T]  chosen  the best move of every tour                         16 B per tour
//   double  [S]  dlen    |P_k - P_k+1|                                        8
//   int     [S]  tour                                                         4
//   float   [S]  d32     fl32(dlen)                             (method 1)    4
//   unsigned[T]  tkey    m32 of every tour as an ordered key    (method 1)    4 B per tour
// = 48 S + 20 T bytes with method 1, 28 S + 16 T with method 0.  A tour has at least 5 cells (n >= 4), so T <= S / 5 rounded up
// to a multiple of 4 and a group of kMaxCells = 3072 cells needs at most 48 * 3072 + 20 * 616 = 159,776 B, plus 272 B of static
// LDS (the wave partials and two scalars): 160,048 of the CU's 163,840 B.  52.1 B per cell; the same limit for both methods.
//
// tp, dlen, q and d32 stay bit-equal to prep_entry / prep_screen_entry (two_opt.hip): tp[k] is a copy of points[tour[k]], and a
// reversal exchanges the copies together with the tour entries; dlen, q and d32 are then recomputed from tp by the arithmetic of
// those functions on the same operands.
//
// Work of a sweep: the waves of the block form `teams` teams of whole waves (block waves / P, at least one wave), a team sweeps
// one tour per round, tours round r * teams + team.  In a team a thread takes every (team size)-th pair of the row-major order
// of the triangle j >= i + 2, so every thread has the same number of pairs, give or take one.  The result does not depend on
// the split: better() is a strict order on (value, flat index) pairs, a NaN change never wins and -0.0 never replaces +0.0.
//
// Loop bounds: moves of a launch <= moves_per_launch; rounds of a move <= tours of the group; pairs of a thread <= pairs of the
// tour / team size + 1, its row search <= n turns per sweep; cells per thread of a copy, reversal or rebuild <= S / block size + 1; the cross-wave
// reduction <= 16 waves.  No spin waits, no block waits for another.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"
#include "resident_team.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

constexpr int kMaxCells = 3072;          // difusco_tsp_two_opt_resident_max_cells: see the LDS budget above
constexpr int kThreads = 1024;           // the largest block: 16 waves
constexpr int kMinThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kDefaultMovesPerLaunch = 1024;
constexpr int kStaticLds = 16 * kWaves + 16;

constexpr size_t lds_bytes(bool screen, int S, int T) { return screen ? 48 * (size_t)S + 20 * (size_t)T : 28 * (size_t)S + 16 * (size_t)T; }
static_assert(lds_bytes(true, kMaxCells, up4(kMaxCells / 5)) + kStaticLds <= 163840, "a group of kMaxCells cells must fit the LDS of a CU");
static_assert(kMaxCells >= 2048 && kMaxCells % 4 == 0, "TSP-500 with 4 samples is 2004 cells");

struct ResGroup {          // 24 bytes; offsets in elements of the array they index
  int n, tours;
  long long points;        // the group's first coordinate in `points` (doubles)
  long long cells;         // its first tour entry in `tours`
};

struct Lds {
  double2* tp;
  float4* q;
  Best* chosen;
  double* dlen;
  int* tour;
  float* d32;
  unsigned* tkey;
};

template <bool kScreen>
__device__ __forceinline__ Lds carve(unsigned char* base, int S, int T) {
  Lds L;
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
__device__ __forceinline__ void edge_entry(const Lds& L, int c) {
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
__device__ __forceinline__ void rebuild(const Lds& L, int cells, int stride, int P) {
  for (int c = threadIdx.x; c < cells; c += blockDim.x)        // <= S / block size + 1 turns
    if (c % stride != stride - 1) edge_entry<kScreen>(L, c);   // the closing entry of a tour starts no edge
  if (kScreen)
    for (int p = threadIdx.x; p < P; p += blockDim.x) L.tkey[p] = f32_key(0.0f);
  __syncthreads();
}

// the exact sweep of one tour (its arrays at `base`): the thread's best move; counts its pairs
__device__ __forceinline__ Best sweep_exact(const Lds& L, int base, int n, const Split& s, unsigned long long& cnt) {
  Best best{0.0, 0};
  if (!s.work) return best;
  const double2* P = L.tp + base;
  const double* D = L.dlen + base;
  for_pairs(n, s, [&](int i, int j) {
    const double change = change64(P[i], P[i + 1], P[j], P[j + 1], D[i], D[j]);
    const long long idx = (long long)i * n + j;
    if (better(change, idx, best)) best = Best{change, idx};
    ++cnt;
  });
  return best;
}

// the screen of one tour: min c32 over the thread's pairs (+inf without one)
__device__ __forceinline__ float sweep_screen(const Lds& L, int base, int n, const Split& s) {
  float m = INFINITY;
  if (!s.work) return m;
  const float4* Q = L.q + base;
  const float* D = L.d32 + base;
  for_pairs(n, s, [&](int i, int j) { m = fminf(m, change32(Q[i], D[i], Q[j], D[j])); });
  return m;
}

// the screened best move of one tour: float64 for the pairs with !(c32 > thr) only (screened_best_tile of two_opt.hip)
__device__ __forceinline__ Best sweep_screened(const Lds& L, int base, int n, const Split& s, float thr, unsigned long long& cnt) {
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
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const Lds L = carve<kScreen>(smem, S, T);
  const double* pts = points + G.points;

  for (int c = tid; c < cells; c += nt) {                      // tp as prep_entry writes it
    const int city = tours[G.cells + c];
    L.tour[c] = city;
    L.tp[c] = make_double2(pts[2 * city], pts[2 * city + 1]);
  }
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
  rebuild<kScreen>(L, cells, stride, P);

  // teams of whole waves; a leftover wave (team >= teams) only keeps the barriers
  const int wpt = nw / P > 1 ? nw / P : 1, tsize = wpt * 64, teams = nw / wpt, team = wave / wpt;
  const int tt = tid - team * tsize;
  const int rounds = (P + teams - 1) / teams;
  const Split sp{tt, tsize, team < teams};

  // The moves of this launch: at most moves_per_launch, at most what max_iterations leaves, at least one sweep (the reference
  // evaluates once even with max_iterations = 0, and a move it then applies reaches the cap: tsp_utils.py:46-47).
  const long long left = max_iterations - iters_g[g];
  const int lim = left < (long long)moves_per_launch ? (left > 1 ? (int)left : 1) : moves_per_launch;
  const bool capped = left <= (long long)lim;                  // lim applied moves reach max_iterations
  unsigned long long cnt = 0;
  bool stop = false;
  int mv = 0;
  for (;;) {                                                   // <= lim <= moves_per_launch turns
    for (int round = 0; round < rounds; ++round) {             // <= tours of the group
      const int p = round * teams + team;
      Split s = sp;
      s.work = sp.work && p < P;
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
        best = sweep_exact(L, base, n, s, cnt);
      }
      best = wave_best(best);
      if (lane == 0) wred[wave] = best;
      __syncthreads();
      if (team < teams && p < P && tt == 0) {                  // the team's first thread: its waves' partials
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
    if (!(gmin < -1e-6)) {                                     // tsp_utils.py:39,44
      stop = true;
      break;
    }
    // every tour applies its own best move (apply_move of two_opt_common.h: tour[mi+1 .. mj] reversed, idx = mi * n + mj),
    // the points in tour order with it
    for (int c = tid; c < cells; c += nt) {
      const int p = c / stride, k = c - p * stride;
      const int idx = (int)L.chosen[p].idx;                    // < n * n <= kMaxCells^2
      const int mi = idx / n, mj = idx % n;
      const int len = mj - mi, t = k - (mi + 1);
      if (t >= 0 && t < len / 2) {
        const int x = p * stride + mi + 1 + t, y = p * stride + mj - t;
        const int tmp = L.tour[x];
        L.tour[x] = L.tour[y];
        L.tour[y] = tmp;
        const double2 tq = L.tp[x];
        L.tp[x] = L.tp[y];
        L.tp[y] = tq;
      }
    }
    __syncthreads();
    rebuild<kScreen>(L, cells, stride, P);
    if (++mv == lim) {
      stop = capped;
      break;
    }
  }
  int* gt = tours + grp[g].cells;
  for (int c = tid; c < cells; c += nt) gt[c] = L.tour[c];
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

// the workspace: the group table, then the state between launches as one block that a single copy reads
struct ResCarve {
  size_t grp, state, state_bytes, total;
};

ResCarve res_carve(int groups) {
  ResCarve c;
  c.grp = 0;
  c.state = up256(sizeof(ResGroup) * (size_t)groups);
  c.state_bytes = 20 * (size_t)groups + 8;                     // iters [G], pairs [G], done [G], stopped
  c.total = c.state + up256(c.state_bytes);
  return c;
}

template <bool kScreen>
hipError_t launch_resident(int groups, int threads, int S, int T, const ResGroup* grp, const double* points, int32_t* tours,
                           long long max_iterations, int per_launch, long long* iters, unsigned long long* pairs, int* done,
                           int* stopped, hipStream_t s) {
  static std::atomic<unsigned long long> attr_devices{0};
  const hipError_t er = ensure_max_dynamic_lds(attr_devices, reinterpret_cast<const void*>(&two_opt_resident_kernel<kScreen>),
                                               (int)lds_bytes(kScreen, kMaxCells, up4(kMaxCells / 5)));
  if (er != hipSuccess) return er;
  hipLaunchKernelGGL(two_opt_resident_kernel<kScreen>, dim3((unsigned)groups), dim3((unsigned)threads), lds_bytes(kScreen, S, T), s,
                     S, T, grp, points, (int*)tours, max_iterations, per_launch, iters, pairs, done, stopped);
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
  *bytes = res_carve(groups).total;
  return DIFUSCO_OK;
}

int difusco_tsp_two_opt_resident(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                 int32_t* tours, int64_t max_iterations, int method, int32_t moves_per_launch, void* workspace,
                                 size_t workspace_bytes, int64_t* iterations_out, int64_t* exact_pairs_out,
                                 int32_t* host_syncs_out, void* stream) {
  using namespace difusco;
  const char* who = "tsp_two_opt_resident";
  int tours_of_call = 0;
  const int rc = check_groups(who, groups, group_n, group_tours, &tours_of_call);
  if (rc != DIFUSCO_OK) return rc;
  if (method != 0 && method != 1) return set_error(DIFUSCO_EINVAL, "%s: method %d (0 exact, 1 screened)", who, method);
  if (!points || !tours || !workspace || !iterations_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "%s: needs non-null device arrays, a host iterations_out[groups] and max_iterations >= 0", who);
  if (moves_per_launch < 0) return set_error(DIFUSCO_EINVAL, "%s: moves_per_launch = %d < 0", who, (int)moves_per_launch);
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
                                             "cells per group (difusco_tsp_two_opt_resident_max_cells; tours unchanged)",
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
  // a thread of the largest group gets about 4 pairs of a sweep or more: whole waves, 256 .. 1024 threads
  long long threads = ((most_pairs + 3) / 4 + 63) / 64 * 64;
  threads = threads < kMinThreads ? kMinThreads : threads > kThreads ? kThreads : threads;

  char* w = (char*)workspace;
  ResGroup* d_grp = (ResGroup*)(w + c.grp);
  long long* d_iters = (long long*)(w + c.state);
  unsigned long long* d_pairs = (unsigned long long*)(d_iters + groups);
  int* d_done = (int*)(d_pairs + groups);
  int* d_stopped = d_done + groups;
  hipStream_t s = (hipStream_t)stream;
  // `tab` lives until the first synchronisation below
  hipError_t er = hipMemcpyAsync(d_grp, tab.data(), sizeof(ResGroup) * (size_t)groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(w + c.state, 0, c.state_bytes, s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s setup: %s", who, hipGetErrorString(er));

  // the reference always evaluates (and may apply) once; at most max_iterations moves are applied (tsp_utils.py:20-47)
  const long long loops = max_iterations > 0 ? max_iterations : 1;
  const long long per = moves_per_launch > 0 ? moves_per_launch : kDefaultMovesPerLaunch;
  const long long launches = (loops + per - 1) / per;
  std::vector<long long> state((c.state_bytes + 7) / 8);
  int syncs = 0;
  for (long long l = 0; l < launches; ++l) {
    // The state is read after every launch: before another one it tells whether every group has stopped, after the last one
    // it is the result.  One synchronisation per launch, none inside a launch.
    er = method == 1 ? launch_resident<true>(groups, (int)threads, S, T, d_grp, points, tours, (long long)max_iterations, (int)per,
                                             d_iters, d_pairs, d_done, d_stopped, s)
                     : launch_resident<false>(groups, (int)threads, S, T, d_grp, points, tours, (long long)max_iterations, (int)per,
                                              d_iters, d_pairs, d_done, d_stopped, s);
    if (er == hipSuccess) er = hipMemcpyAsync(state.data(), w + c.state, c.state_bytes, hipMemcpyDeviceToHost, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    syncs += 1;
    if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s: %s", who, hipGetErrorString(er));
    if (((const int*)(state.data() + 2 * (size_t)groups))[groups] >= groups) break;
  }
  unsigned long long pairs = 0;
  for (int g = 0; g < groups; ++g) {
    iterations_out[g] = (int64_t)state[(size_t)g];
    pairs += (unsigned long long)state[(size_t)groups + (size_t)g];
  }
  if (exact_pairs_out) *exact_pairs_out = (int64_t)pairs;
  if (host_syncs_out) *host_syncs_out = syncs;
  return DIFUSCO_OK;
}

}  // extern "C"
