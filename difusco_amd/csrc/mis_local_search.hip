// (1,2)-swap local search for MIS solutions (difusco_mis_local_search; the rule is stated in include/difusco_hip.h and restated
// in numpy in tests/mis_local_search_emulation.py).  Not in the reference: its MIS path ends at the greedy decode.
//
// Works, like the decode, on the CSR of the whole call: the graphs of a batch are components, and every step below is local to
// a component.  rank = position in the stable descending sort of the scores (rocPRIM radix sort, as in mis_decode.hip).
//
// All per-round work is on the device.  A control block in the workspace holds the phase and the counters; every kernel reads
// the phase first and returns when it is not its own, so the host enqueues a fixed sequence of launches (a "group") and polls
// the control block once per group:
//   group  = CYCLES x cycle, then mis_ls_finish_kernel (copies the set out once the phase is DONE)
//   cycle  = SUBROUNDS x (insert round, insert advance), then one swap round:
//            tight, propose, conflict, apply, tight (the new set's states), swap advance
// The phases: INSERT (sub-rounds of the insertion phase until no free node is undecided), SWAP (ready for a round), DONE.
// A cycle whose insertion phase needs more than SUBROUNDS sub-rounds skips its swap round (still INSERT) and goes on in the
// next cycle.  Only the one-thread advance kernels write the phase, so it is constant inside every other launch.
//
// Determinism: every kernel reads what earlier launches wrote and writes arrays that no other wave of its launch reads, with
// two exceptions.  (a) An insert round reads the states of other nodes while they are being decided, as mis_round_kernel does:
// a stale read only delays a decision by a sub-round, the decisions themselves are those of the lexicographically first
// maximal independent set.  (b) The propose kernel marks, in mark[], the candidates of x adjacent to its first node and reads
// the marks back in the SAME wave; candidate sets of different x are disjoint, so no other wave touches those entries.
// The counters are integer atomic adds.
//
// difusco_mis_iterated_search (second half of this file) repeats that descent between seeded random kicks: the same kernels and
// phase word, two more phases, and a kick sequence after every IT_CYCLES cycles (restated in tests/mis_iterated_search_emulation.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "../../include/difusco_hip.h"
#include "common.h"
#include "kernels.h"

namespace difusco {
namespace {

constexpr int LS_INSERT = 0, LS_SWAP = 1, LS_DONE = 2;
constexpr int LS_KICK = 3, LS_FINAL = 4;   // the iterated search only (below): a kick is being applied; the incumbent is final
constexpr int LS_CYCLES = 4;         // swap rounds enqueued between two host polls
constexpr int LS_SUBROUNDS = 2;      // insertion sub-rounds enqueued in front of every swap round

struct LsCtrl {                      // device; the host reads it once per group
  int phase, bad, rounds, swaps, inserts, proposals, undecided, max_rounds;
  // the iterated search only: kicks asked for and applied, 1 once the first descent is the incumbent, the round cap of ONE
  // descent (max_rounds above is then rounds-so-far + cap), kick_size, 1 when the instance table is malformed
  int kicks, kicks_done, started, cap, kick_size, bad_table;
};

thread_local int g_host_syncs = 0;   // host synchronisations of this thread's last search call (difusco_mis_search_host_syncs)

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// the sort key of difusco_mis_decode (mis_sort_key, kernels.h) beside the index
__global__ void mis_ls_key_kernel(int n, const float* __restrict__ scores, unsigned* __restrict__ key, unsigned* __restrict__ idx) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  key[v] = mis_sort_key(__float_as_uint(scores[v]));
  idx[v] = (unsigned)v;
}

// rank from the sorted order; the working copy of the set (anything non-zero counts as chosen); no marks yet
__global__ void mis_ls_setup_kernel(int n, const unsigned* __restrict__ order, const int* __restrict__ solution,
                                    int* __restrict__ rank, int* __restrict__ sol, int* __restrict__ mark) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  rank[order[p]] = p;
  sol[p] = solution[p] != 0;
  mark[p] = -1;
}

// The checking pass: a chosen node with a chosen neighbour sets the flag.  One wavefront per node.
__global__ __launch_bounds__(256) void mis_ls_check_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const int* __restrict__ sol, LsCtrl* __restrict__ ctrl) {
  const int v = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (v >= n) return;
  if (!sol[v]) return;                                       // wave uniform
  int hit = 0;
  for (int e = rowptr[v] + lane; e < rowptr[v + 1]; e += 64) {
    const int u = col[e];
    hit |= u != v && sol[u] != 0;
  }
  if (__any(hit) && lane == 0) ctrl->bad = 1;
}

__global__ void mis_ls_start_kernel(LsCtrl* __restrict__ ctrl) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->phase = ctrl->bad ? LS_DONE : LS_INSERT;
}

// tight / owner / state of every node from the current set.  when: the phase it runs in; after_swaps: only in a round that
// proposed something (the second launch of a swap round: the states the next insertion phase starts from).
// state: 0 undecided (free), 1 in, 2 out.
__global__ __launch_bounds__(256) void mis_ls_tight_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const int* __restrict__ sol, int* __restrict__ tight,
                                                           int* __restrict__ owner, int* __restrict__ state,
                                                           const LsCtrl* __restrict__ ctrl, int when, int after_swaps) {
  const int v = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (v >= n) return;
  if (ctrl->phase != when || (after_swaps && ctrl->proposals == 0)) return;
  if (sol[v]) {                                              // wave uniform
    if (lane == 0) { tight[v] = -1; owner[v] = -1; state[v] = 1; }
    return;
  }
  int c = 0, o = -1;
  for (int e = rowptr[v] + lane; e < rowptr[v + 1]; e += 64) {
    const int u = col[e];
    if (u != v && sol[u]) { ++c; o = max(o, u); }
  }
  c = wave_sum(c);
  o = wave_max(o);
  if (lane == 0) { tight[v] = c; owner[v] = c == 1 ? o : -1; state[v] = c > 0 ? 2 : 0; }
}

// One sub-round of the insertion phase: the rule of mis_round_kernel on the free nodes (every other node is decided).
__global__ __launch_bounds__(256) void mis_ls_insert_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                            const int* __restrict__ rank, int* __restrict__ state,
                                                            int* __restrict__ sol, LsCtrl* __restrict__ ctrl) {
  const int v = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (v >= n) return;
  if (ctrl->phase != LS_INSERT) return;
  if (state[v] != 0) return;                                 // wave uniform
  const int rv = rank[v];
  int any_in = 0, any_open = 0;
  for (int e = rowptr[v] + lane; e < rowptr[v + 1]; e += 64) {
    const int u = col[e];
    if (u == v) continue;
    if (rank[u] < rv) {
      const int su = state[u];                               // a stale read only delays the decision by a sub-round
      any_in |= su == 1;
      any_open |= su == 0;
    }
  }
  any_in = __any(any_in);
  any_open = __any(any_open);
  if (lane == 0) {
    if (any_in) state[v] = 2;
    else if (!any_open) { state[v] = 1; sol[v] = 1; atomicAdd(&ctrl->inserts, 1); }
    else atomicAdd(&ctrl->undecided, 1);
  }
}

__global__ void mis_ls_insert_advance_kernel(LsCtrl* __restrict__ ctrl) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || ctrl->phase != LS_INSERT) return;
  if (ctrl->undecided == 0) ctrl->phase = ctrl->rounds < ctrl->max_rounds ? LS_SWAP : LS_DONE;
  ctrl->undecided = 0;
}

// The proposal of every x in the set: prop_u[x], prop_w[x], or -1.  v is in L(x) iff tight[v] == 1 && owner[v] == x.
// The first node is the pairable candidate of the smallest rank (pairable: fewer than |L(x)| - 1 members of L(x) among its
// neighbours); candidates are visited in rank order until one is pairable.  The second node is the member of the smallest rank
// above the first's that is not marked as a neighbour of the first.  mark[w] == u is only ever written for w in N(u), so a mark
// left by an earlier round still tells the truth.
__global__ __launch_bounds__(256) void mis_ls_propose_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const int* __restrict__ rank, const int* __restrict__ sol,
                                                             const int* __restrict__ tight, const int* __restrict__ owner,
                                                             int* __restrict__ mark, int* __restrict__ prop_u,
                                                             int* __restrict__ prop_w, LsCtrl* __restrict__ ctrl) {
  const int x = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (x >= n) return;
  if (ctrl->phase != LS_SWAP) return;
  if (!sol[x]) return;                                       // wave uniform
  const int b = rowptr[x], e = rowptr[x + 1];
  const unsigned long long none = ~0ull;
  int cnt = 0;
  for (int i = b + lane; i < e; i += 64) {
    const int v = col[i];
    cnt += v != x && tight[v] == 1 && owner[v] == x;
  }
  cnt = wave_sum(cnt);
  int pu = -1, pw = -1;
  long long last = -1;                                       // rank of the candidate visited last
  while (cnt >= 2) {
    unsigned long long best = none;
    for (int i = b + lane; i < e; i += 64) {
      const int v = col[i];
      if (v != x && tight[v] == 1 && owner[v] == x && rank[v] > last) {
        const unsigned long long key = ((unsigned long long)(unsigned)rank[v] << 32) | (unsigned)v;
        best = key < best ? key : best;
      }
    }
    best = wave_min64(best);
    if (best == none) break;                                 // every candidate visited, none pairable
    const int u = (int)(unsigned)(best & 0xffffffffu);
    last = (long long)(best >> 32);
    int c = 0;
    for (int j = rowptr[u] + lane; j < rowptr[u + 1]; j += 64) {
      const int w = col[j];
      if (w != u && w != x && tight[w] == 1 && owner[w] == x) {
        ++c;
        __hip_atomic_store(&mark[w], u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    c = wave_sum(c);
    if (c >= cnt - 1) continue;                              // adjacent to every other candidate
    __threadfence();                                         // this wave's marks are in memory before it reads them back
    unsigned long long second = none;
    for (int i = b + lane; i < e; i += 64) {
      const int v = col[i];
      if (v != x && v != u && tight[v] == 1 && owner[v] == x && rank[v] > last &&
          __hip_atomic_load(&mark[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != u) {
        const unsigned long long key = ((unsigned long long)(unsigned)rank[v] << 32) | (unsigned)v;
        second = key < second ? key : second;
      }
    }
    second = wave_min64(second);
    if (second != none) { pu = u; pw = (int)(unsigned)(second & 0xffffffffu); }
    break;                                                   // no second node (duplicate entries): no proposal
  }
  if (lane == 0) {
    prop_u[x] = pu;
    prop_w[x] = pw;
    if (pu >= 0) atomicAdd(&ctrl->proposals, 1);
  }
}

// win[x] = 1 iff x proposes and its key rank[u_x] is below the key of every conflicting proposal.  A neighbour b of u_x or w_x
// belongs to a proposal iff it is a candidate (of y = owner[b]) and one of y's two nodes.  win = 0 for every other node.
__global__ __launch_bounds__(256) void mis_ls_conflict_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              const int* __restrict__ rank, const int* __restrict__ tight,
                                                              const int* __restrict__ owner, const int* __restrict__ prop_u,
                                                              const int* __restrict__ prop_w, int* __restrict__ win,
                                                              const LsCtrl* __restrict__ ctrl) {
  const int x = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (x >= n) return;
  if (ctrl->phase != LS_SWAP || ctrl->proposals == 0) return;
  const int pu = tight[x] == -1 ? prop_u[x] : -1;            // tight == -1: x is in the set (prop_* are this round's)
  if (pu < 0) {                                              // wave uniform
    if (lane == 0) win[x] = 0;
    return;
  }
  const int key = rank[pu];
  int lose = 0;
  for (int s = 0; s < 2; ++s) {
    const int a = s == 0 ? pu : prop_w[x];
    for (int j = rowptr[a] + lane; j < rowptr[a + 1]; j += 64) {
      const int q = col[j];
      if (q == a || tight[q] != 1) continue;
      const int y = owner[q];
      if (y == x) continue;
      const int uy = prop_u[y];
      if (uy >= 0 && (uy == q || prop_w[y] == q)) lose |= rank[uy] < key;
    }
  }
  lose = __any(lose);
  if (lane == 0) win[x] = !lose;
}

// All winners at once: x leaves, u_x and w_x enter.  Membership is read from tight (the set before this round), never from
// sol, which this launch writes; the three entries a winner writes are written by no other thread.
__global__ void mis_ls_apply_kernel(int n, const int* __restrict__ tight, const int* __restrict__ win,
                                    const int* __restrict__ prop_u, const int* __restrict__ prop_w, int* __restrict__ sol,
                                    LsCtrl* __restrict__ ctrl) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n) return;
  if (ctrl->phase != LS_SWAP || ctrl->proposals == 0) return;
  if (tight[x] != -1 || !win[x]) return;
  sol[x] = 0;
  sol[prop_u[x]] = 1;
  sol[prop_w[x]] = 1;
  atomicAdd(&ctrl->swaps, 1);
}

__global__ void mis_ls_swap_advance_kernel(LsCtrl* __restrict__ ctrl) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || ctrl->phase != LS_SWAP) return;
  if (ctrl->proposals == 0) {
    ctrl->phase = LS_DONE;                                   // a round without a proposal ends the search, uncounted
  } else {
    ctrl->rounds += 1;
    ctrl->proposals = 0;
    ctrl->phase = LS_INSERT;
  }
}

__global__ void mis_ls_finish_kernel(int n, const int* __restrict__ sol, int* __restrict__ solution,
                                     const LsCtrl* __restrict__ ctrl) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  if (ctrl->phase != LS_DONE || ctrl->bad) return;
  solution[v] = sol[v];
}

// ---- the iterated search (difusco_mis_iterated_search): kicks between descents ----------------------------------------------
// After the cycles of a unit comes the kick sequence.  Its kernels run only when the descent has ended (phase DONE):
//   keep      one block per instance: |C_b| against |I_b|, then I_b <- C_b or C_b <- I_b (the first time: I <- the descent)
//   advance   DONE -> FINAL when every kick ran, else -> KICK
//   draw      w_v and the kicked test of every node          (KICK)
//   enter     the kicked nodes without a smaller kicked neighbour (KICK)
//   evict     members next to an entered node leave, the entered nodes go in (KICK)
//   tight     the states the next descent starts from        (KICK)
//   advance   KICK -> INSERT: the next descent, with its own round cap  Every kernel reads what earlier launches wrote; the only words two waves of
// one launch write are entered_flag[b], where every writer stores the same 1.

// The instance of node v: the last b with rows[b] <= v.  Stays inside the table whatever the table holds.
__device__ __forceinline__ int ls_instance_of(const int64_t* __restrict__ rows, int nb, int v) {
  int lo = 0, hi = nb;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (rows[mid] <= (int64_t)v) lo = mid; else hi = mid;
  }
  return lo;
}

// rows[0] = 0, rows[nb] = n, non-decreasing; anything else ends the call before a kernel walks an instance
__global__ void mis_it_table_kernel(int n, int nb, const int64_t* __restrict__ rows, LsCtrl* __restrict__ ctrl) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nb) return;
  const bool bad = i == nb ? rows[nb] != (int64_t)n : (rows[i] > rows[i + 1] || (i == 0 && rows[0] != 0));
  if (bad) { ctrl->bad_table = 1; ctrl->bad = 1; }
}

__global__ void mis_it_setup_kernel(int n, int nb, const int64_t* __restrict__ rows, int* __restrict__ inst,
                                    int* __restrict__ entered_flag, int* __restrict__ per) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) inst[v] = ls_instance_of(rows, nb, v);
  if (v < nb) {
    entered_flag[v] = 0;
    per[4 * v] = per[4 * v + 1] = per[4 * v + 2] = per[4 * v + 3] = 0;
  }
}

// per: entered, accepted, size_before, size_after of every instance
__global__ __launch_bounds__(256) void mis_it_keep_kernel(const int64_t* __restrict__ rows, int* __restrict__ sol,
                                                          int* __restrict__ inc, int* __restrict__ isize,
                                                          int* __restrict__ entered_flag, int* __restrict__ per,
                                                          const LsCtrl* __restrict__ ctrl) {
  if (ctrl->phase != LS_DONE || ctrl->bad) return;
  __shared__ int part[4];
  __shared__ int total;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = (int)rows[b], hi = (int)rows[b + 1];
  const int first = !ctrl->started;
  const int old = first ? 0 : isize[b];                      // read by every thread before thread 0 writes it
  int c = 0;
  for (int v = lo + (int)threadIdx.x; v < hi; v += 256) c += sol[v] != 0;
  c = wave_sum(c);
  if (lane == 0) part[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) total = part[0] + part[1] + part[2] + part[3];
  __syncthreads();
  const int cnt = total;
  const int keep = first || cnt >= old;
  for (int v = lo + (int)threadIdx.x; v < hi; v += 256) {
    if (keep) inc[v] = sol[v]; else sol[v] = inc[v];
  }
  if (threadIdx.x == 0) {
    if (first) per[4 * b + 2] = cnt;
    else if (entered_flag[b]) { per[4 * b] += 1; per[4 * b + 1] += keep; }
    entered_flag[b] = 0;
    if (keep) isize[b] = cnt;
    per[4 * b + 3] = keep ? cnt : old;
  }
}

__global__ void mis_it_keep_advance_kernel(LsCtrl* __restrict__ ctrl) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || ctrl->phase != LS_DONE || ctrl->bad) return;
  ctrl->started = 1;
  ctrl->phase = ctrl->kicks_done >= ctrl->kicks ? LS_FINAL : LS_KICK;
}

// kw[v] = w_v when v is kicked, -1 otherwise.  sol is the incumbent here (the keep kernel made it so).
__global__ void mis_it_draw_kernel(int n, const int64_t* __restrict__ rows, const uint64_t* __restrict__ seeds,
                                   const uint64_t* __restrict__ offsets, const int* __restrict__ inst,
                                   const int* __restrict__ isize, const int* __restrict__ sol, int* __restrict__ kw,
                                   const LsCtrl* __restrict__ ctrl) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  if (ctrl->phase != LS_KICK) return;
  int out = -1;
  if (!sol[v]) {
    const int b = inst[v];
    const int64_t lo = rows[b];
    uint32_t r[4];
    Philox::run(seeds[b], offsets[b] + (uint64_t)ctrl->kicks_done, (uint64_t)((int64_t)v - lo), r);
    const uint64_t w = r[0] >> 8;
    const uint64_t m = (uint64_t)(rows[b + 1] - lo - (int64_t)isize[b]);
    if (w * m < ((uint64_t)ctrl->kick_size << 24)) out = (int)w;     // exact: w < 2^24, m < 2^31, kick_size < 2^31
  }
  kw[v] = out;
}

// One wavefront per node.  ent[v] = 1 iff v is kicked and no kicked neighbour has a smaller (w, node).
__global__ __launch_bounds__(256) void mis_it_enter_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const int* __restrict__ kw, const int* __restrict__ inst,
                                                           int* __restrict__ ent, int* __restrict__ entered_flag,
                                                           const LsCtrl* __restrict__ ctrl) {
  const int v = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (v >= n) return;
  if (ctrl->phase != LS_KICK) return;
  const int wv = kw[v];
  if (wv < 0) {                                              // wave uniform
    if (lane == 0) ent[v] = 0;
    return;
  }
  const unsigned long long key = ((unsigned long long)(unsigned)wv << 32) | (unsigned)v;
  int lose = 0;
  for (int e = rowptr[v] + lane; e < rowptr[v + 1]; e += 64) {
    const int u = col[e];
    const int wu = kw[u];
    if (u != v && wu >= 0) lose |= (((unsigned long long)(unsigned)wu << 32) | (unsigned)u) < key;
  }
  lose = __any(lose);
  if (lane == 0) {
    ent[v] = !lose;
    if (!lose) __hip_atomic_store(&entered_flag[inst[v]], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One wavefront per node.  Every wave writes sol[v] of its own node only and reads ent[], which this launch does not write.
__global__ __launch_bounds__(256) void mis_it_evict_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const int* __restrict__ ent, int* __restrict__ sol,
                                                           const LsCtrl* __restrict__ ctrl) {
  const int v = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (v >= n) return;
  if (ctrl->phase != LS_KICK) return;
  if (ent[v]) {                                              // wave uniform
    if (lane == 0) sol[v] = 1;
    return;
  }
  if (!sol[v]) return;                                       // wave uniform
  int hit = 0;
  for (int e = rowptr[v] + lane; e < rowptr[v + 1]; e += 64) {
    const int u = col[e];
    hit |= u != v && ent[u] != 0;
  }
  if (__any(hit) && lane == 0) sol[v] = 0;
}

__global__ void mis_it_kick_advance_kernel(LsCtrl* __restrict__ ctrl) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || ctrl->phase != LS_KICK) return;
  ctrl->kicks_done += 1;
  const long long cap = (long long)ctrl->rounds + ctrl->cap;           // the descent that starts now has its own cap
  ctrl->max_rounds = cap > 0x7fffffffLL ? 0x7fffffff : (int)cap;
  ctrl->phase = LS_INSERT;
}

__global__ void mis_it_finish_kernel(int n, const int* __restrict__ sol, int* __restrict__ solution,
                                     const LsCtrl* __restrict__ ctrl) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  if (ctrl->phase != LS_FINAL || ctrl->bad) return;
  solution[v] = sol[v];
}

size_t up256(size_t x) { return (x + 255) / 256 * 256; }

struct LsCarve {
  unsigned *key_b, *idx_a, *idx_b;
  int *rank, *sol, *state, *tight, *owner, *mark, *prop_u, *prop_w, *win;
  LsCtrl* ctrl;
  void* temp;
  size_t temp_bytes, total;
};

hipError_t ls_carve(void* base, int n, LsCarve* c) {
  size_t t = 0;
  hipError_t er = rocprim::radix_sort_pairs_desc(nullptr, t, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr,
                                                 (unsigned*)nullptr, (size_t)n, 0, 32, 0, false);
  if (er != hipSuccess) return er;
  c->temp_bytes = t;
  size_t cur = 0;
  auto take = [&](size_t bytes) {
    size_t at = cur;
    cur += up256(bytes);
    return base ? (void*)((char*)base + at) : (void*)nullptr;
  };
  const size_t row = 4 * (size_t)n;
  c->key_b = (unsigned*)take(row);
  c->idx_a = (unsigned*)take(row);
  c->idx_b = (unsigned*)take(row);
  c->rank = (int*)take(row);
  c->sol = (int*)take(row);
  c->state = (int*)take(row);
  c->tight = (int*)take(row);
  c->owner = (int*)take(row);
  c->mark = (int*)take(row);
  c->prop_u = (int*)take(row);
  c->prop_w = (int*)take(row);
  c->win = (int*)take(row);
  c->ctrl = (LsCtrl*)take(sizeof(LsCtrl));
  c->temp = take(t);
  c->total = cur;
  return hipSuccess;
}

// What a search starts with: the control block, the ranks, the working copy of the set and the checking pass.
hipError_t ls_enqueue_begin(const LsCarve& c, int n, const int* rowptr, const int* col, const float* scores,
                            const int* solution, const LsCtrl& h, hipStream_t st) {
  const dim3 blk(256), g1((unsigned)((n + 255) / 256)), gw((unsigned)(((long long)n * 64 + 255) / 256));
  hipError_t er = hipMemcpyAsync(c.ctrl, &h, sizeof(h), hipMemcpyHostToDevice, st);
  if (er != hipSuccess) return er;
  unsigned* key_a = (unsigned*)c.prop_u;      // free until the first proposal, which comes after the sort
  hipLaunchKernelGGL(mis_ls_key_kernel, g1, blk, 0, st, n, scores, key_a, c.idx_a);
  size_t tb = c.temp_bytes;
  // descending by key; the sort is stable, so equal keys keep increasing index order (the order of difusco_mis_decode)
  er = rocprim::radix_sort_pairs_desc(c.temp, tb, key_a, c.key_b, c.idx_a, c.idx_b, (size_t)n, 0, 32, st, false);
  if (er != hipSuccess) return er;
  hipLaunchKernelGGL(mis_ls_setup_kernel, g1, blk, 0, st, n, c.idx_b, solution, c.rank, c.sol, c.mark);
  hipLaunchKernelGGL(mis_ls_check_kernel, gw, blk, 0, st, n, rowptr, col, c.sol, c.ctrl);
  return hipSuccess;
}

// One cycle: SUBROUNDS x (insert round, insert advance), then one swap round.
void ls_enqueue_cycle(const LsCarve& c, int n, const int* rowptr, const int* col, hipStream_t st) {
  const dim3 blk(256), g1((unsigned)((n + 255) / 256)), gw((unsigned)(((long long)n * 64 + 255) / 256)), one(1);
  for (int s = 0; s < LS_SUBROUNDS; ++s) {
    hipLaunchKernelGGL(mis_ls_insert_kernel, gw, blk, 0, st, n, rowptr, col, c.rank, c.state, c.sol, c.ctrl);
    hipLaunchKernelGGL(mis_ls_insert_advance_kernel, one, dim3(64), 0, st, c.ctrl);
  }
  hipLaunchKernelGGL(mis_ls_tight_kernel, gw, blk, 0, st, n, rowptr, col, c.sol, c.tight, c.owner, c.state, c.ctrl, LS_SWAP, 0);
  hipLaunchKernelGGL(mis_ls_propose_kernel, gw, blk, 0, st, n, rowptr, col, c.rank, c.sol, c.tight, c.owner, c.mark,
                     c.prop_u, c.prop_w, c.ctrl);
  hipLaunchKernelGGL(mis_ls_conflict_kernel, gw, blk, 0, st, n, rowptr, col, c.rank, c.tight, c.owner, c.prop_u, c.prop_w,
                     c.win, c.ctrl);
  hipLaunchKernelGGL(mis_ls_apply_kernel, g1, blk, 0, st, n, c.tight, c.win, c.prop_u, c.prop_w, c.sol, c.ctrl);
  hipLaunchKernelGGL(mis_ls_tight_kernel, gw, blk, 0, st, n, rowptr, col, c.sol, c.tight, c.owner, c.state, c.ctrl, LS_SWAP, 1);
  hipLaunchKernelGGL(mis_ls_swap_advance_kernel, one, dim3(64), 0, st, c.ctrl);
}

constexpr int IT_CYCLES = 2;         // cycles in front of every kick sequence (a descent after a kick is short)
constexpr int IT_UNITS = 8;          // (cycles, kick sequence) units enqueued between two host polls

struct ItCarve {                     // the workspace of the iterated search: the descent's, then its own arrays
  LsCarve ls;
  int *inc, *kw, *ent, *inst, *isize, *entered_flag, *per;
  size_t total;
};

hipError_t it_carve(void* base, int n, int nb, ItCarve* c) {
  hipError_t er = ls_carve(base, n, &c->ls);
  if (er != hipSuccess) return er;
  size_t cur = c->ls.total;
  auto take = [&](size_t bytes) {
    size_t at = cur;
    cur += up256(bytes);
    return base ? (int*)((char*)base + at) : (int*)nullptr;
  };
  const size_t row = 4 * (size_t)n, irow = 4 * (size_t)nb;
  c->inc = take(row);
  c->kw = take(row);
  c->ent = take(row);
  c->inst = take(row);
  c->isize = take(irow);
  c->entered_flag = take(irow);
  c->per = take(4 * irow);
  c->total = cur;
  return hipSuccess;
}

}  // namespace

// The start of difusco_mis_iterated_search up to its first round, for mis_resident_search.hip (declared in kernels.h): the
// same carve and the same launches, so both searches rank, copy and check alike.
hipError_t mis_search_prelude(void* workspace, int n, int nb, const int32_t* rowptr, const int32_t* col, const float* scores,
                              const int32_t* solution, const int64_t* rows, hipStream_t st, MisSearchPrelude* out) {
  ItCarve w;
  hipError_t er = it_carve(workspace, n, nb, &w);
  if (er != hipSuccess) return er;
  out->bytes = w.total;
  if (!workspace) return hipSuccess;
  // static: the asynchronous copy may read it after this function has returned.  DONE: no kernel of the launched search runs
  static const LsCtrl h = [] {
    LsCtrl c;
    std::memset(&c, 0, sizeof(c));
    c.phase = LS_DONE;
    return c;
  }();
  er = ls_enqueue_begin(w.ls, n, rowptr, col, scores, solution, h, st);
  if (er != hipSuccess) return er;
  hipLaunchKernelGGL(mis_it_table_kernel, dim3((unsigned)(nb / 256 + 1)), dim3(256), 0, st, n, nb, rows, w.ls.ctrl);
  hipLaunchKernelGGL(mis_it_setup_kernel, dim3((unsigned)(((n > nb ? n : nb) + 255) / 256)), dim3(256), 0, st, n, nb, rows, w.inst,
                     w.entered_flag, w.per);
  out->rank = w.ls.rank;
  out->sol = w.ls.sol;
  out->inc = w.inc;
  out->per = w.per;
  out->bad = &w.ls.ctrl->bad;
  out->bad_table = &w.ls.ctrl->bad_table;
  return hipSuccess;
}

void mis_search_set_host_syncs(int count) { g_host_syncs = count; }

}  // namespace difusco

extern "C" {

int difusco_mis_local_search_workspace_bytes(int n_nodes, int64_t n_edges, size_t* bytes) {
  using namespace difusco;
  if (!bytes || n_nodes < 1 || n_edges < 0) return set_error(DIFUSCO_EINVAL, "mis_local_search_workspace_bytes: bad arguments");
  LsCarve c;
  hipError_t er = ls_carve(nullptr, n_nodes, &c);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  *bytes = c.total;
  return DIFUSCO_OK;
}

int difusco_mis_local_search(int n_nodes, const int32_t* rowptr, const int32_t* col, const float* scores, int32_t* solution,
                             int32_t max_rounds, void* workspace, size_t workspace_bytes, int32_t counters[3], void* stream) {
  using namespace difusco;
  if (n_nodes < 1 || !rowptr || !col || !scores || !solution || !workspace || !counters)
    return set_error(DIFUSCO_EINVAL, "mis_local_search: null array or empty graph");
  if (max_rounds < 0) return set_error(DIFUSCO_EINVAL, "mis_local_search: max_rounds = %d < 0", (int)max_rounds);
  g_host_syncs = 0;
  LsCarve c;
  hipError_t er = ls_carve(workspace, n_nodes, &c);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  if (workspace_bytes < c.total)
    return set_error(DIFUSCO_EINVAL, "mis_local_search: workspace %zu < %zu bytes", workspace_bytes, c.total);
  hipStream_t st = (hipStream_t)stream;
  const int n = n_nodes;
  const dim3 blk(256);
  const dim3 g1((unsigned)((n + 255) / 256));                         // one thread per node
  const dim3 gw((unsigned)(((long long)n * 64 + 255) / 256));         // one wavefront per node
  const dim3 one(1);

  LsCtrl h;
  std::memset(&h, 0, sizeof(h));
  h.phase = LS_DONE;                                                   // until the start kernel has seen the check
  h.max_rounds = max_rounds;
  er = ls_enqueue_begin(c, n, rowptr, col, scores, solution, h, st);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "mis_local_search start: %s", hipGetErrorString(er));
  hipLaunchKernelGGL(mis_ls_start_kernel, one, dim3(64), 0, st, c.ctrl);
  hipLaunchKernelGGL(mis_ls_tight_kernel, gw, blk, 0, st, n, rowptr, col, c.sol, c.tight, c.owner, c.state, c.ctrl, LS_INSERT, 0);

  // every counted round applies a swap and every unfinished sub-round decides a node, so a correct input ends long before this
  const long long max_groups = 2LL * n + 8;
  for (long long group = 0;; ++group) {
    for (int cyc = 0; cyc < LS_CYCLES; ++cyc) ls_enqueue_cycle(c, n, rowptr, col, st);
    hipLaunchKernelGGL(mis_ls_finish_kernel, g1, blk, 0, st, n, c.sol, solution, c.ctrl);
    er = hipMemcpyAsync(&h, c.ctrl, sizeof(h), hipMemcpyDeviceToHost, st);
    if (er == hipSuccess) er = hipStreamSynchronize(st);                // the one host synchronisation of the group
    ++g_host_syncs;
    if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "mis_local_search rounds: %s", hipGetErrorString(er));
    if (h.bad) return set_error(DIFUSCO_EINVAL, "mis_local_search: the input set is not independent (solution unchanged)");
    if (h.phase == LS_DONE) break;
    if (group > max_groups) return set_error(DIFUSCO_EINVAL, "mis_local_search: no progress (adjacency not symmetric?)");
  }
  counters[0] = h.rounds;
  counters[1] = h.swaps;
  counters[2] = h.inserts;
  return DIFUSCO_OK;
}

int difusco_mis_search_host_syncs(void) { return difusco::g_host_syncs; }

int difusco_mis_iterated_search_workspace_bytes(int n_nodes, int64_t n_edges, int n_instances, size_t* bytes) {
  using namespace difusco;
  if (!bytes || n_nodes < 1 || n_edges < 0 || n_instances < 1)
    return set_error(DIFUSCO_EINVAL, "mis_iterated_search_workspace_bytes: bad arguments");
  ItCarve c;
  hipError_t er = it_carve(nullptr, n_nodes, n_instances, &c);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  *bytes = c.total;
  return DIFUSCO_OK;
}

int difusco_mis_iterated_search(int n_nodes, const int32_t* rowptr, const int32_t* col, const float* scores, int32_t* solution,
                                int n_instances, const int64_t* instance_rows, const uint64_t* instance_seeds,
                                const uint64_t* instance_offsets, int32_t kicks, int32_t kick_size, int32_t max_rounds,
                                void* workspace, size_t workspace_bytes, int32_t counters[3], int32_t* per_instance, void* stream) {
  using namespace difusco;
  g_host_syncs = 0;
  if (n_nodes < 1 || !rowptr || !col || !scores || !solution || !workspace || !counters || !instance_rows || !instance_seeds ||
      !instance_offsets)
    return set_error(DIFUSCO_EINVAL, "mis_iterated_search: null array or empty graph");
  if (n_instances < 1) return set_error(DIFUSCO_EINVAL, "mis_iterated_search: n_instances = %d < 1", n_instances);
  if (max_rounds < 0) return set_error(DIFUSCO_EINVAL, "mis_iterated_search: max_rounds = %d < 0", (int)max_rounds);
  if (kicks < 0) return set_error(DIFUSCO_EINVAL, "mis_iterated_search: kicks = %d < 0", (int)kicks);
  if (kick_size < 1) return set_error(DIFUSCO_EINVAL, "mis_iterated_search: kick_size = %d < 1", (int)kick_size);
  ItCarve w;
  hipError_t er = it_carve(workspace, n_nodes, n_instances, &w);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  if (workspace_bytes < w.total)
    return set_error(DIFUSCO_EINVAL, "mis_iterated_search: workspace %zu < %zu bytes", workspace_bytes, w.total);
  const LsCarve& c = w.ls;
  hipStream_t st = (hipStream_t)stream;
  const int n = n_nodes, nb = n_instances;
  const dim3 blk(256);
  const dim3 g1((unsigned)((n + 255) / 256));                         // one thread per node
  const dim3 gw((unsigned)(((long long)n * 64 + 255) / 256));         // one wavefront per node
  const dim3 gs((unsigned)(((n > nb ? n : nb) + 255) / 256));         // one thread per node and per instance
  const dim3 gt((unsigned)(nb / 256 + 1));                            // one thread per table entry
  const dim3 one(1);

  LsCtrl h;
  std::memset(&h, 0, sizeof(h));
  h.phase = LS_DONE;                                                   // until the start kernel has seen the checks
  h.max_rounds = h.cap = max_rounds;
  h.kicks = kicks;
  h.kick_size = kick_size;
  er = ls_enqueue_begin(c, n, rowptr, col, scores, solution, h, st);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "mis_iterated_search start: %s", hipGetErrorString(er));
  hipLaunchKernelGGL(mis_it_table_kernel, gt, blk, 0, st, n, nb, instance_rows, c.ctrl);
  hipLaunchKernelGGL(mis_it_setup_kernel, gs, blk, 0, st, n, nb, instance_rows, w.inst, w.entered_flag, w.per);
  hipLaunchKernelGGL(mis_ls_start_kernel, one, dim3(64), 0, st, c.ctrl);
  hipLaunchKernelGGL(mis_ls_tight_kernel, gw, blk, 0, st, n, rowptr, col, c.sol, c.tight, c.owner, c.state, c.ctrl, LS_INSERT, 0);

  std::vector<int32_t> per(4 * (size_t)nb);
  // every descent ends within 2 n + 8 groups (difusco_mis_local_search), and there are kicks + 1 of them
  const long long max_groups = (2LL * n + 8) * ((long long)kicks + 1);
  for (long long group = 0;; ++group) {
    for (int unit = 0; unit < IT_UNITS; ++unit) {
      for (int cyc = 0; cyc < IT_CYCLES; ++cyc) ls_enqueue_cycle(c, n, rowptr, col, st);
      hipLaunchKernelGGL(mis_it_keep_kernel, dim3((unsigned)nb), blk, 0, st, instance_rows, c.sol, w.inc, w.isize, w.entered_flag,
                         w.per, c.ctrl);
      hipLaunchKernelGGL(mis_it_keep_advance_kernel, one, dim3(64), 0, st, c.ctrl);
      if (kicks > 0) {
        hipLaunchKernelGGL(mis_it_draw_kernel, g1, blk, 0, st, n, instance_rows, instance_seeds, instance_offsets, w.inst,
                           w.isize, c.sol, w.kw, c.ctrl);
        hipLaunchKernelGGL(mis_it_enter_kernel, gw, blk, 0, st, n, rowptr, col, w.kw, w.inst, w.ent, w.entered_flag, c.ctrl);
        hipLaunchKernelGGL(mis_it_evict_kernel, gw, blk, 0, st, n, rowptr, col, w.ent, c.sol, c.ctrl);
        hipLaunchKernelGGL(mis_ls_tight_kernel, gw, blk, 0, st, n, rowptr, col, c.sol, c.tight, c.owner, c.state, c.ctrl,
                           LS_KICK, 0);                                // the states the next descent starts from
        hipLaunchKernelGGL(mis_it_kick_advance_kernel, one, dim3(64), 0, st, c.ctrl);
      }
    }
    hipLaunchKernelGGL(mis_it_finish_kernel, g1, blk, 0, st, n, c.sol, solution, c.ctrl);
    er = hipMemcpyAsync(&h, c.ctrl, sizeof(h), hipMemcpyDeviceToHost, st);
    if (er == hipSuccess) er = hipMemcpyAsync(per.data(), w.per, per.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (er == hipSuccess) er = hipStreamSynchronize(st);                // the one host synchronisation of the group
    ++g_host_syncs;
    if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "mis_iterated_search rounds: %s", hipGetErrorString(er));
    if (h.bad_table)
      return set_error(DIFUSCO_EINVAL, "mis_iterated_search: instance_rows must start at 0, end at n_nodes and not decrease "
                                       "(solution unchanged)");
    if (h.bad) return set_error(DIFUSCO_EINVAL, "mis_iterated_search: the input set is not independent (solution unchanged)");
    if (h.phase == LS_FINAL) break;
    if (group > max_groups) return set_error(DIFUSCO_EINVAL, "mis_iterated_search: no progress (adjacency not symmetric?)");
  }
  counters[0] = h.rounds;
  counters[1] = h.swaps;
  counters[2] = h.inserts;
  if (per_instance) std::memcpy(per_instance, per.data(), per.size() * sizeof(int32_t));
  return DIFUSCO_OK;
}

}  // extern "C"
