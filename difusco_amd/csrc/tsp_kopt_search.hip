// Heatmap-guided sampled k-opt search for TSP tours (difusco_tsp_kopt_search_ragged; the rule: include/difusco_hip.h, restated
// in python in tests/tsp_kopt_search_emulation.py).  Launched, not resident: per round two launches,
//
//   kopt_simulate_kernel   one THREAD per simulation, the grid spread over (tours x ceil(S / 256)): opens the incumbent at a drawn
//                          position and, up to D times, draws a new edge from the head of the open path among the promising
//                          candidate entries of the head's row (two passes over the row: the total, then the cumulative walk) and
//                          reverses the path prefix that closes it.  The path is never copied: with at most 10 cuts a position
//                          maps through them in O(i); the cuts of a thread live in its column of an LDS array.  It leaves its
//                          value, its i*, its begin position and, per step, the chosen entry, its mirror entry and the cut;
//   kopt_round_kernel      one BLOCK per tour: the best value of the round (ties to the lowest simulation, by a reduction
//                          that does not depend on arrival), the counts of all steps, and - if the best is above 1e-6 - the action
//                          as one gather through the cut map, the weights of the added edges, the length, the stall counter and
//                          the tour's stop word.
//
// In front of them, once per call: the graph check of the guided search (or_opt_heat.h), kopt_weight_kernel (w and C by (tour,
// entry); an entry that is no candidate holds w = -1, so a row scan needs no second look at the row) and kopt_init_kernel (the
// incumbent, its inverse, the row sums and the length).  Behind them kopt_finish_kernel writes the incumbent over the input tour
// unless it is longer.  All float64 arithmetic is + - * / sqrt, compiled without contraction.
#include <cmath>
#include <vector>

#include "common.h"
#include "multi_move_common.h"
#include "or_opt_heat.h"

namespace difusco {
namespace {

constexpr int kMaxSamples = 4096, kMaxDepth = 10, kSimThreads = 256;
constexpr double kImprove = 1e-6;

struct KoTour {            // a tour of a call; offsets in elements of the array they index
  int n, edges, group, pad;
  long long points;        // the group's first coordinate in `points`
  long long closed;        // the tour's first entry in tours, inc and nxt (n + 1 per tour)
  long long cols;          //                       in pos and sw (n per tour)
  long long rows, gedges;  // the group's first entry in row_ptr and in col
  long long heat;          // the tour's first entry in heat, w and C (E_g per tour)
  long long sim;           //                       in value, istar, nsteps and start (S per tour); x D in ent, mir and cut
};

struct KoState {           // the state of a tour
  double len, first_len;
  long long stall, depth_sum;
  int rounds, actions, stopped, reverted, city0, pad;
};

struct KoLayout {
  size_t tab, hgrp, st, done, bad, inc, nxt, pos, sw, w, C, value, istar, nsteps, start, ent, mir, cut, total;
  int tours, nmax, emax;
};

struct KoPtrs {
  KoTour* tab;
  MlHeatGroup* hgrp;
  KoState* st;
  int *done, *bad, *inc, *nxt, *pos;
  double *sw, *w;
  int* C;
  double* value;
  int *istar, *nsteps, *start, *ent, *mir, *cut;
  KoPtrs(void* workspace, const KoLayout& L) {
    char* p = (char*)workspace;
    tab = (KoTour*)(p + L.tab), hgrp = (MlHeatGroup*)(p + L.hgrp), st = (KoState*)(p + L.st);
    done = (int*)(p + L.done), bad = (int*)(p + L.bad), inc = (int*)(p + L.inc), nxt = (int*)(p + L.nxt), pos = (int*)(p + L.pos);
    sw = (double*)(p + L.sw), w = (double*)(p + L.w), C = (int*)(p + L.C), value = (double*)(p + L.value);
    istar = (int*)(p + L.istar), nsteps = (int*)(p + L.nsteps), start = (int*)(p + L.start);
    ent = (int*)(p + L.ent), mir = (int*)(p + L.mir), cut = (int*)(p + L.cut);
  }
};

// ---- device

__device__ __forceinline__ double city_dist(const double* __restrict__ P, int a, int b) {
  return dist2d(P[2 * a] - P[2 * b], P[2 * a + 1] - P[2 * b + 1]);
}

// the first entry of row u with column v, -1 if there is none: for u != v the candidate entry (u, v)
__device__ __forceinline__ int find_entry(const int* __restrict__ row_ptr, const int* __restrict__ col, int u, int v) {
  const int e1 = row_ptr[u + 1];
  for (int e = row_ptr[u]; e < e1; ++e)
    if (col[e] == v) return e;
  return -1;
}

// one thread per (entry, tour) of a checked graph: the row of the entry by bisection of row_ptr, then the entries in front of it
__global__ __launch_bounds__(256) void kopt_weight_kernel(const int* __restrict__ row_ptr_all, const int* __restrict__ col_all,
                                                          const float* __restrict__ heat_all, const KoTour* __restrict__ tab,
                                                          double* __restrict__ w_all, int* __restrict__ C_all) {
  const KoTour t = tab[blockIdx.y];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.edges) return;
  const int e = (int)i;
  const int* row_ptr = row_ptr_all + t.rows;
  const int* col = col_all + t.gedges;
  int lo = 0, hi = t.n;                                            // row_ptr[lo] <= e < row_ptr[hi]
  for (int step = 0; step < 32 && hi - lo > 1; ++step) {
    const int mid = (lo + hi) >> 1;
    if (row_ptr[mid] <= e)
      lo = mid;
    else
      hi = mid;
  }
  const int v = col[e];
  bool cand = v != lo;
  for (int f = row_ptr[lo]; f < e && cand; ++f) cand = col[f] != v;
  const float h = fminf(fmaxf(heat_all[t.heat + e], 0.0f), 1.0f);  // a NaN counts as 0
  w_all[t.heat + e] = cand ? 100.0 * (double)h : -1.0;
  C_all[t.heat + e] = 0;
}

// one block per tour: the incumbent and its inverse, the row sums, the length and the state
__global__ __launch_bounds__(kSelectThreads) void kopt_init_kernel(const double* __restrict__ points_all,
                                                                   const int* __restrict__ tours_all,
                                                                   const int* __restrict__ row_ptr_all,
                                                                   const KoTour* __restrict__ tab, int* __restrict__ inc_all,
                                                                   int* __restrict__ pos_all, double* __restrict__ sw_all,
                                                                   const double* __restrict__ w_all, KoState* __restrict__ st) {
  __shared__ double part[kLenParts];
  const KoTour t = tab[blockIdx.x];
  const int n = t.n;
  const int* tour = tours_all + t.closed;
  int* inc = inc_all + t.closed;
  int* pos = pos_all + t.cols;
  const int* row_ptr = row_ptr_all + t.rows;
  const double* w = w_all + t.heat;
  for (int k = threadIdx.x; k <= n; k += kSelectThreads) {
    const int c = tour[k];
    inc[k] = c;
    if (k < n) pos[c] = k;
  }
  for (int u = threadIdx.x; u < n; u += kSelectThreads) {
    double s = 0.0;
    const int e1 = row_ptr[u + 1];
    for (int e = row_ptr[u]; e < e1; ++e) {
      const double x = w[e];
      if (x >= 0.0) s = __dadd_rn(s, x);
    }
    sw_all[t.cols + u] = s;
  }
  const double len = tour_length(points_all + t.points, tour, n, part);
  if (threadIdx.x == 0) {
    KoState s{};
    s.len = s.first_len = len;
    s.city0 = tour[0];
    st[blockIdx.x] = s;
  }
}

// the position map of a simulation: cuts y_0 .. y_i-1 (reversals of the path prefix [0, y)), the begin position p
struct CutMap {
  const int* cuts;         // cuts[k * stride]
  int stride, p, n;
  // the original path position of current position x behind the first i reversals
  __device__ __forceinline__ int origin(int x, int i) const {
    for (int k = i - 1; k >= 0; --k) {
      const int y = cuts[k * stride];
      if (x < y) x = y - 1 - x;
    }
    return x;
  }
  // the position in the incumbent of current path position x
  __device__ __forceinline__ int tour_pos(int x, int i) const {
    const int q = p + 1 + origin(x, i);
    return q >= n ? q - n : q;
  }
  // the current path position of the city at position `at` of the incumbent
  __device__ __forceinline__ int path_pos(int at, int i) const {
    int x = at - p - 1;
    if (x < 0) x += n;
    for (int k = 0; k < i; ++k) {
      const int y = cuts[k * stride];
      if (x < y) x = y - 1 - x;
    }
    return x;
  }
};

// pot(e) of a candidate entry: w / avg + explore / sqrt(C + 1)
__device__ __forceinline__ double potential(double w, double avg, double ex, int count) {
  return __dadd_rn(__ddiv_rn(w, avg), __ddiv_rn(ex, sqrt((double)(count + 1))));
}

// one thread per simulation of round `round`; grid (ceil(S / 256), tours)
__global__ __launch_bounds__(kSimThreads) void kopt_simulate_kernel(
    const double* __restrict__ points_all, const int* __restrict__ row_ptr_all, const int* __restrict__ col_all,
    const KoTour* __restrict__ tab, const KoState* __restrict__ st, const int* __restrict__ inc_all,
    const int* __restrict__ pos_all, const double* __restrict__ w_all, const int* __restrict__ C_all,
    const double* __restrict__ sw_all, const unsigned long long* __restrict__ seeds,
    const unsigned long long* __restrict__ offsets, int S, int D, unsigned long long round, double ex,
    double* __restrict__ value, int* __restrict__ istar, int* __restrict__ nsteps, int* __restrict__ start, int* __restrict__ ent,
    int* __restrict__ mir, int* __restrict__ cut) {
  __shared__ int cuts[kMaxDepth][kSimThreads];
  const int b = blockIdx.y;
  if (st[b].stopped) return;
  const int s = blockIdx.x * kSimThreads + threadIdx.x;
  if (s >= S) return;
  const KoTour t = tab[b];
  const int n = t.n;
  const double* P = points_all + t.points;
  const int* row_ptr = row_ptr_all + t.rows;
  const int* col = col_all + t.gedges;
  const int* I = inc_all + t.closed;
  const int* pos = pos_all + t.cols;
  const double* w = w_all + t.heat;
  const int* C = C_all + t.heat;
  const double* sw = sw_all + t.cols;
  const unsigned long long seed = seeds[b], offset = offsets[b] + round;
  const long long sim = t.sim + s, steps = t.sim * D + s;

  uint32_t r[4];
  Philox::run(seed, offset, (uint64_t)(unsigned)s, r);
  const int p = (int)(r[0] % (unsigned)n);
  const CutMap map{&cuts[0][threadIdx.x], kSimThreads, p, n};
  const int a1 = I[p];
  int head = I[p + 1 == n ? 0 : p + 1];
  double gain = city_dist(P, a1, head), best = 0.0;
  int best_i = 0, taken = 0;
  const double nm1 = (double)(n - 1);
  for (int i = 1; i <= D; ++i) {
    if ((i & 3) == 0) Philox::run(seed, offset, ((uint64_t)(i >> 2) << 32) | (unsigned)s, r);
    const uint32_t word = (i & 3) == 0 ? r[0] : (i & 3) == 1 ? r[1] : (i & 3) == 2 ? r[2] : r[3];
    const double avg = __ddiv_rn(sw[head], nm1);
    if (!(avg > 0.0)) break;
    const int next = I[map.tour_pos(1, i - 1)];
    const int e0 = row_ptr[head], e1 = row_ptr[head + 1];
    double tot = 0.0;
    int last = -1;
    for (int e = e0; e < e1; ++e) {
      const double we = w[e];
      const int c = col[e];
      if (we < 0.0 || c == a1 || c == next) continue;
      const double pot = potential(we, avg, ex, C[e]);
      if (pot >= 1.0) tot = __dadd_rn(tot, pot), last = e;
    }
    if (last < 0) break;
    const int draw = (int)(word % 1000u);
    int cum = 0, chosen = last;
    for (int e = e0; e < last; ++e) {
      const double we = w[e];
      const int c = col[e];
      if (we < 0.0 || c == a1 || c == next) continue;
      const double pot = potential(we, avg, ex, C[e]);
      if (pot >= 1.0) {
        cum += (int)__ddiv_rn(__dmul_rn(1000.0, pot), tot);
        if (draw < cum) {
          chosen = e;
          break;
        }
      }
    }
    const int c = col[chosen];
    const int y = map.path_pos(pos[c], i - 1);                     // 2 <= y <= n - 2
    const int nb = I[map.tour_pos(y - 1, i - 1)];
    gain = __dadd_rn(__dsub_rn(gain, city_dist(P, head, c)), city_dist(P, c, nb));
    const double real = __dsub_rn(gain, city_dist(P, nb, a1));
    cuts[i - 1][threadIdx.x] = y;
    ent[steps + (long long)(i - 1) * S] = chosen;
    mir[steps + (long long)(i - 1) * S] = find_entry(row_ptr, col, c, head);
    cut[steps + (long long)(i - 1) * S] = y;
    taken = i;
    if (best_i == 0 || real > best) best = real, best_i = i;
    head = nb;
    if (real > kImprove) break;
  }
  value[sim] = best;
  istar[sim] = best_i;
  nsteps[sim] = taken;
  start[sim] = p;
}

__device__ __forceinline__ bool better_sim(double v, int s, double bv, int bs) { return v > bv || (v == bv && s < bs); }

// one block per tour: the end of a round
__global__ __launch_bounds__(kSelectThreads) void kopt_round_kernel(
    const double* __restrict__ points_all, const int* __restrict__ row_ptr_all, const int* __restrict__ col_all,
    const KoTour* __restrict__ tab, KoState* __restrict__ st, int* __restrict__ inc_all, int* __restrict__ nxt_all,
    int* __restrict__ pos_all, double* __restrict__ w_all, int* __restrict__ C_all, double* __restrict__ sw_all, int S, int D,
    long long patience, double beta, const double* __restrict__ value, const int* __restrict__ istar,
    const int* __restrict__ nsteps, const int* __restrict__ start, const int* __restrict__ ent, const int* __restrict__ mir,
    const int* __restrict__ cut, int* __restrict__ done) {
  __shared__ double part[kLenParts];
  __shared__ int who[kSelectThreads];
  __shared__ int ycut[kMaxDepth];
  __shared__ int eu[kMaxDepth + 1], ev[kMaxDepth + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (st[b].stopped) return;
  const KoTour t = tab[b];
  const int n = t.n;
  const int* row_ptr = row_ptr_all + t.rows;
  const int* col = col_all + t.gedges;
  int* I = inc_all + t.closed;
  int* nxt = nxt_all + t.closed;
  int* pos = pos_all + t.cols;
  double* w = w_all + t.heat;
  int* C = C_all + t.heat;
  double* sw = sw_all + t.cols;
  const long long steps = t.sim * D;

  // the best of the round: the largest value, ties to the lowest s; a simulation without a step has none
  double bv = 0.0;
  int bs = INT_MAX;
  for (int s = tid; s < S; s += kSelectThreads)
    if (istar[t.sim + s] > 0) {
      const double v = value[t.sim + s];
      if (bs == INT_MAX || v > bv) bv = v, bs = s;
    }
  part[tid] = bv, who[tid] = bs;
  __syncthreads();
  for (int h = kSelectThreads / 2; h > 0; h >>= 1) {
    if (tid < h && who[tid + h] != INT_MAX && (who[tid] == INT_MAX || better_sim(part[tid + h], who[tid + h], part[tid], who[tid])))
      part[tid] = part[tid + h], who[tid] = who[tid + h];
    __syncthreads();
  }
  bv = part[0], bs = who[0];
  __syncthreads();

  // the counts: every step taken by every simulation, the chosen entry and its mirror
  for (int x = tid; x < S * D; x += kSelectThreads) {
    const int k = x / S, s = x - k * S;
    if (k < nsteps[t.sim + s]) {
      atomicAdd(&C[ent[steps + x]], 1);
      const int m = mir[steps + x];
      if (m >= 0) atomicAdd(&C[m], 1);
    }
  }

  const bool apply = bs != INT_MAX && bv > kImprove;
  if (apply) {
    const int is = istar[t.sim + bs], p = start[t.sim + bs];
    if (tid < is) ycut[tid] = cut[steps + (long long)tid * S + bs];
    __syncthreads();
    const CutMap map{ycut, 1, p, n};
    if (tid == 0) {                                                // the added edges, from the incumbent as it still is
      int head = I[p + 1 == n ? 0 : p + 1];
      for (int k = 0; k < is; ++k) {
        eu[k] = head, ev[k] = col[ent[steps + (long long)k * S + bs]];
        head = I[map.tour_pos(ycut[k] - 1, k)];
      }
      eu[is] = head, ev[is] = I[p];
    }
    // path position x becomes tour position x, rotated so that the city at position 0 stays there
    const int z = map.path_pos(pos[st[b].city0], is);
    for (int k = tid; k < n; k += kSelectThreads) {
      const int x = z + k >= n ? z + k - n : z + k;
      nxt[k] = I[map.tour_pos(x, is)];
    }
    __syncthreads();
    for (int k = tid; k < n; k += kSelectThreads) {
      const int c = nxt[k];
      I[k] = c;
      pos[c] = k;
      if (k == 0) I[n] = c;
    }
    if (tid == 0) {                                                // the weights, sequentially in step order
      const double x = __ddiv_rn(bv, st[b].len);
      const double inc = __dmul_rn(beta, __dadd_rn(x, __dmul_rn(__dmul_rn(0.5, x), x)));
      for (int k = 0; k <= is; ++k)
        for (int o = 0; o < 2; ++o) {
          const int u = o ? ev[k] : eu[k], v = o ? eu[k] : ev[k];
          const int e = find_entry(row_ptr, col, u, v);
          if (e >= 0) w[e] = __dadd_rn(w[e], inc);
          sw[u] = __dadd_rn(sw[u], inc);
        }
    }
    __syncthreads();
    const double len = tour_length(points_all + t.points, I, n, part);
    if (tid == 0) {
      st[b].len = len;
      st[b].stall = 0;
      st[b].actions += 1;
      st[b].depth_sum += is;
      st[b].rounds += 1;
    }
  } else if (tid == 0) {
    const long long stall = st[b].stall + S;
    st[b].stall = stall;
    st[b].rounds += 1;
    if (stall >= patience * n) {
      st[b].stopped = 1;
      atomicAdd(done, 1);
    }
  }
}

// one block per tour: the incumbent over the input tour unless it is longer
__global__ __launch_bounds__(256) void kopt_finish_kernel(const KoTour* __restrict__ tab, KoState* __restrict__ st,
                                                          const int* __restrict__ inc_all, int* __restrict__ tours_all) {
  const KoTour t = tab[blockIdx.x];
  const bool longer = st[blockIdx.x].len > st[blockIdx.x].first_len;
  if (!longer)
    for (int k = threadIdx.x; k <= t.n; k += blockDim.x) tours_all[t.closed + k] = inc_all[t.closed + k];
  if (threadIdx.x == 0) st[blockIdx.x].reverted = longer;
}

// ---- host

int kopt_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, const int32_t* group_edges,
                int samples, int depth, KoLayout* lay, std::vector<KoTour>* tab, std::vector<MlHeatGroup>* hgrp) {
  *lay = KoLayout{};
  const int rc = check_groups(who, groups, group_n, group_tours, &lay->tours);
  if (rc != DIFUSCO_OK) return rc;
  if (!group_edges) return set_error(DIFUSCO_EINVAL, "%s: group_edges is null", who);
  if (samples < 1 || samples > kMaxSamples)
    return set_error(DIFUSCO_EINVAL, "%s: samples = %d, needs 1 .. %d", who, samples, kMaxSamples);
  if (depth < 1 || depth > kMaxDepth) return set_error(DIFUSCO_EINVAL, "%s: depth = %d, needs 1 .. %d", who, depth, kMaxDepth);
  size_t closed = 0, cols = 0, points = 0, rows = 0, gedges = 0, heat = 0, sim = 0;
  for (int g = 0; g < groups; ++g) {
    const int n = group_n[g], E = group_edges[g];
    if (E < 0) return set_error(DIFUSCO_EINVAL, "%s: group %d has %d edges", who, g, E);
    if (n > lay->nmax) lay->nmax = n;
    if (E > lay->emax) lay->emax = E;
    if (hgrp) hgrp->push_back(MlHeatGroup{n, E, (long long)rows, (long long)gedges});
    for (int p = 0; p < group_tours[g]; ++p) {
      if (tab)
        tab->push_back(KoTour{n, E, g, 0, (long long)points, (long long)closed, (long long)cols, (long long)rows, (long long)gedges,
                              (long long)heat, (long long)sim});
      closed += (size_t)n + 1, cols += (size_t)n, heat += (size_t)E, sim += (size_t)samples;
    }
    points += 2 * (size_t)n, rows += (size_t)n + 1, gedges += (size_t)E;
  }
  Sections sec;
  const size_t T = (size_t)lay->tours;
  lay->tab = sec.take(sizeof(KoTour) * T), lay->hgrp = sec.take(sizeof(MlHeatGroup) * (size_t)groups);
  lay->st = sec.take(sizeof(KoState) * T), lay->done = sec.take(sizeof(int)), lay->bad = sec.take(sizeof(int));
  lay->inc = sec.take(sizeof(int) * closed), lay->nxt = sec.take(sizeof(int) * closed), lay->pos = sec.take(sizeof(int) * cols);
  lay->sw = sec.take(sizeof(double) * cols), lay->w = sec.take(sizeof(double) * heat), lay->C = sec.take(sizeof(int) * heat);
  lay->value = sec.take(sizeof(double) * sim), lay->istar = sec.take(sizeof(int) * sim);
  lay->nsteps = sec.take(sizeof(int) * sim), lay->start = sec.take(sizeof(int) * sim);
  lay->ent = sec.take(sizeof(int) * sim * (size_t)depth), lay->mir = sec.take(sizeof(int) * sim * (size_t)depth);
  lay->cut = sec.take(sizeof(int) * sim * (size_t)depth);
  lay->total = sec.off;
  return DIFUSCO_OK;
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_kopt_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours,
                                                   const int32_t* group_edges, int32_t samples, int32_t depth, size_t* bytes) {
  using namespace difusco;
  const char* who = "tsp_kopt_search_ragged_workspace_bytes";
  if (!bytes) return set_error(DIFUSCO_EINVAL, "%s: bytes is null", who);
  KoLayout lay;
  const int rc = kopt_layout(who, groups, group_n, group_tours, group_edges, samples, depth, &lay, nullptr, nullptr);
  if (rc != DIFUSCO_OK) return rc;
  *bytes = lay.total;
  return DIFUSCO_OK;
}

int difusco_tsp_kopt_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                   int32_t* tours, const int32_t* group_edges, const int32_t* row_ptr, const int32_t* col,
                                   const float* heat, const uint64_t* tour_seeds, const uint64_t* tour_offsets, int32_t samples,
                                   int32_t depth, int32_t max_rounds, int32_t patience, double beta, const double* explore,
                                   void* workspace, size_t workspace_bytes, int32_t* rounds_out, int32_t* actions_out,
                                   int64_t* depth_sum_out, int32_t* reverted_out, double* first_length_out,
                                   double* final_length_out, void* stream) {
  using namespace difusco;
  const char* who = "tsp_kopt_search_ragged";
  tsp_search_set_host_syncs(0);
  KoLayout lay;
  std::vector<KoTour> tab;
  std::vector<MlHeatGroup> hgrp;
  const int rc = kopt_layout(who, groups, group_n, group_tours, group_edges, samples, depth, &lay, &tab, &hgrp);
  if (rc != DIFUSCO_OK) return rc;
  if (!points || !tours || !row_ptr || !col || !heat || !tour_seeds || !tour_offsets || !workspace)
    return set_error(DIFUSCO_EINVAL, "%s: needs the device arrays points / tours / row_ptr / col / heat / tour_seeds / tour_offsets "
                                     "and a workspace", who);
  if (!rounds_out || !actions_out || !depth_sum_out || !reverted_out || !first_length_out || !final_length_out)
    return set_error(DIFUSCO_EINVAL, "%s: needs the six host output arrays [tours]", who);
  if (max_rounds < 0) return set_error(DIFUSCO_EINVAL, "%s: max_rounds = %d < 0", who, (int)max_rounds);
  if (patience < 1) return set_error(DIFUSCO_EINVAL, "%s: patience = %d, needs at least 1", who, (int)patience);
  if (!(beta >= 0.0) || !std::isfinite(beta)) return set_error(DIFUSCO_EINVAL, "%s: beta = %g, needs a finite value >= 0", who, beta);
  if (max_rounds > 0 && !explore) return set_error(DIFUSCO_EINVAL, "%s: explore is null", who);
  for (int r = 0; r < max_rounds; ++r)
    if (!(explore[r] >= 0.0) || !std::isfinite(explore[r]))
      return set_error(DIFUSCO_EINVAL, "%s: explore[%d] = %g, needs a finite value >= 0", who, r, explore[r]);
  if (workspace_bytes < lay.total) return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", who, workspace_bytes, lay.total);

  const KoPtrs p(workspace, lay);
  hipStream_t s = (hipStream_t)stream;
  const int T = lay.tours, S = samples, D = depth;
  int bad = 0, syncs = 0;
  hipError_t er = hipMemcpyAsync(p.tab, tab.data(), sizeof(KoTour) * T, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemcpyAsync(p.hgrp, hgrp.data(), sizeof(MlHeatGroup) * groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(p.done, 0, sizeof(int), s);
  if (er == hipSuccess) er = hipMemsetAsync(p.bad, 0, sizeof(int), s);
  if (er == hipSuccess) {                                          // the check of the graphs, in front of the setup synchronisation
    const long long longest = (long long)lay.nmax + 1 > lay.emax ? (long long)lay.nmax + 1 : lay.emax;
    hipLaunchKernelGGL(heat_graph_check_kernel, dim3((unsigned)((longest + 255) / 256), groups), dim3(256), 0, s, row_ptr, col, p.hgrp,
                       p.bad);
    er = hipMemcpyAsync(&bad, p.bad, sizeof(int), hipMemcpyDeviceToHost, s);
  }
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  tsp_search_set_host_syncs(++syncs);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s setup: %s", who, hipGetErrorString(er));
  if (bad)
    return set_error(DIFUSCO_EINVAL, "%s: a group's graph is not a CSR over its cities (row_ptr[0] = 0, row_ptr rising to "
                                     "row_ptr[n] = edges, 0 <= col < n)", who);
  if (lay.emax > 0)
    hipLaunchKernelGGL(kopt_weight_kernel, dim3((unsigned)(((long long)lay.emax + 255) / 256), T), dim3(256), 0, s, row_ptr, col, heat,
                       p.tab, p.w, p.C);
  hipLaunchKernelGGL(kopt_init_kernel, dim3(T), dim3(kSelectThreads), 0, s, points, tours, row_ptr, p.tab, p.inc, p.pos, p.sw, p.w,
                     p.st);
  const unsigned long long* seeds = (const unsigned long long*)tour_seeds;
  const unsigned long long* offsets = (const unsigned long long*)tour_offsets;
  const dim3 sim_grid((S + kSimThreads - 1) / kSimThreads, T);
  long long round = 0;
  // a round of every tour that has not stopped: its simulations, then its end; the word counts the tours that stalled
  const Polled polled = poll_launches(max_rounds, 8, T, p.done, s, [&] {
    hipLaunchKernelGGL(kopt_simulate_kernel, sim_grid, dim3(kSimThreads), 0, s, points, row_ptr, col, p.tab, p.st, p.inc, p.pos, p.w,
                       p.C, p.sw, seeds, offsets, S, D, (unsigned long long)round, explore[round], p.value, p.istar, p.nsteps,
                       p.start, p.ent, p.mir, p.cut);
    hipLaunchKernelGGL(kopt_round_kernel, dim3(T), dim3(kSelectThreads), 0, s, points, row_ptr, col, p.tab, p.st, p.inc, p.nxt, p.pos,
                       p.w, p.C, p.sw, S, D, (long long)patience, beta, p.value, p.istar, p.nsteps, p.start, p.ent, p.mir, p.cut,
                       p.done);
    ++round;
  });
  syncs += polled.syncs;
  tsp_search_set_host_syncs(syncs);
  if (polled.status != hipSuccess) return set_error(DIFUSCO_EHIP, "%s state: %s", who, hipGetErrorString(polled.status));
  hipLaunchKernelGGL(kopt_finish_kernel, dim3(T), dim3(256), 0, s, p.tab, p.st, p.inc, tours);
  std::vector<KoState> states(T);
  er = hipMemcpyAsync(states.data(), p.st, sizeof(KoState) * T, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  tsp_search_set_host_syncs(++syncs);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s counters: %s", who, hipGetErrorString(er));
  for (int b = 0; b < T; ++b) {
    const KoState& x = states[b];
    rounds_out[b] = x.rounds;
    actions_out[b] = x.actions;
    depth_sum_out[b] = x.depth_sum;
    reverted_out[b] = x.reverted;
    first_length_out[b] = x.first_len;
    final_length_out[b] = x.reverted ? x.first_len : x.len;
  }
  return DIFUSCO_OK;
}

}  // extern "C"
