// The iterated (1,2)-swap search for MIS solutions with one resident block per instance (difusco_mis_resident_search).  The rule is
// the one of difusco_mis_iterated_search (include/difusco_hip.h), which this entry must equal bit for bit; the numpy restatement
// is tests/mis_iterated_search_emulation.py.  Nothing of the rule is restated here: every pass below is the kernel of the same
// name in mis_local_search.hip with the union's arrays replaced by the instance's arrays in LDS and node ids made local.
//
// Why a block can run alone: every step of the rule is local to an instance, and step t of a union is step t of each instance.
// A block therefore runs the descent, the kicks and the keep-or-restore of ITS instance start to finish; the only words two
// blocks both touch are the integer atomics of the call counters (add for swaps and inserts, max for the rounds of descent t).
//
// Prelude (mis_search_prelude, mis_local_search.hip): the launched search's own sort, rank scatter, working copy, independence
// check and table check.  Then one limit check, `launches` launches of the search kernel back to back and one finish kernel; the
// host synchronises once, after the copy-out.
//
// LDS of a block, S = the node capacity of the launch (the largest possible instance of the call, at most kMaxNodes):
//   int  [S]   rank, tight, osum, mark, kw (the draws), pu, pw (the proposals)
//   int  [S+4] rp: the instance's slice of rowptr (col stays in global memory: read-only, L2 resident)
//   u8   [S]   sol, inc (the incumbent), ent, win
// = 36 S + 16 bytes: 147,472 B at S = kMaxNodes = 4096, of the CU's 163,840.
//
// tight and owner are kept INCREMENTALLY (the launched search recomputes them per round): tight[v] is the number of entries of
// solution nodes' rows that name v, osum[v] the sum of those nodes' local ids - the owner when tight[v] == 1.  A node that enters
// or leaves the set walks its own row once and adds +-1 / +-id to its neighbours with LDS integer atomics (push); the launched
// search counts the entries of v's own row (pull).  On the symmetric adjacency both entries require these are the same numbers,
// duplicates counted per entry, self entries ignored.  The insertion state needs no array then: a node is undecided iff it is
// outside the set with tight == 0, and "out" iff tight > 0.
//
// Loop bounds: insertion sub-rounds <= n_b + 1 (every unfinished sub-round decides the undecided node of the smallest rank; the
// last one finds nothing undecided), swap rounds of a descent <= min(max_rounds, n_b) (a counted round applies a swap and a swap
// grows the set), the candidate walk of a proposal <= |L(x)| <= n_b, kicks of a launch <= kicks_per_launch.  No spin waits.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/difusco_hip.h"
#include "common.h"
#include "kernels.h"

namespace difusco {
namespace {

constexpr int kMaxNodes = 4096;          // difusco_mis_resident_max_nodes: 36 B of LDS per node
constexpr int kThreads = 1024;           // 16 waves: a wave per node, striding over the neighbour list
constexpr int kDefaultKicksPerLaunch = 256;
constexpr int kNone = INT_MAX;

struct ResCtrl {                         // device; copied out once, after the last launch
  int over, over_nodes;                  // the first instance above the limit (kNone: none) and its node count
  int rounds, swaps, inserts;
  int bad, bad_table;                    // the prelude's two flags, gathered by the finish kernel
};

__device__ __forceinline__ int wsum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wmin64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

struct Lds {                             // the arrays of one instance (see the layout above) and the block's scalars
  int *rank, *tight, *osum, *mark, *kw, *pu, *pw, *rp;
  uint8_t *sol, *inc, *ent, *win;
  int* slot;                             // [3] rotating sums of block_sum
  int* tally;                            // [2] swaps, inserts of this launch
  int turn;                              // block_sum calls so far, the same in every thread
  int n, lo;                             // nodes of the instance, its first node in the union
  const int* col;
};

// Sum of v over the block, and the barrier that ends a pass.  Call k adds into slot k % 3 and clears slot (k + 1) % 3, which was
// last read in call k - 2: every thread left that call before it passed the barrier of call k - 1.
__device__ __forceinline__ int block_sum(Lds& s, int v) {
  const int k = s.turn % 3;
  v = wsum(v);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s.slot[k], v);
  if (threadIdx.x == 0) s.slot[(k + 1) % 3] = 0;
  __syncthreads();
  s.turn += 1;
  return s.slot[k];
}

// local index of a neighbour entry, or -1 for a self entry and for an entry outside the instance (the caller guarantees there is
// none; it is never used as an index)
__device__ __forceinline__ int local_of(const Lds& s, int u, int v) {
  const unsigned l = (unsigned)(u - s.lo);
  return (l < (unsigned)s.n && (int)l != v) ? (int)l : -1;
}

// Node a enters (d = +1) or leaves (d = -1) the set: every entry of its row counts once at the neighbour it names.  Called by
// the whole wave; integer atomics, so the sums do not depend on the order of the waves.
__device__ __forceinline__ void push(Lds& s, int a, int d) {
  const int lane = threadIdx.x & 63;
  for (int i = s.rp[a] + lane; i < s.rp[a + 1]; i += 64) {
    const int l = local_of(s, s.col[i], a);
    if (l >= 0) {
      atomicAdd(&s.tight[l], d);
      atomicAdd(&s.osum[l], d * a);
    }
  }
}

// tight / osum of every node from the set in sol: zero, then every member pushes (once per launch)
__device__ void tight_from_scratch(Lds& s) {
  const int wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int v = threadIdx.x; v < s.n; v += blockDim.x) s.tight[v] = s.osum[v] = 0;
  __syncthreads();
  for (int v = wv; v < s.n; v += nw)
    if (s.sol[v]) push(s, v, 1);                               // wave uniform
  __syncthreads();
}

// mis_ls_insert_kernel; returns the undecided nodes of the sub-round.  Undecided: outside the set with tight == 0.  A neighbour
// read while it is being decided shows as in, as out (tight > 0: final, the set only grows here) or, stale, as undecided: a
// stale read only delays the decision by a sub-round.
__device__ int insert_pass(Lds& s) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const volatile uint8_t* sol = s.sol;                         // other waves decide while this one reads
  const volatile int* tight = s.tight;
  int undecided = 0;
  for (int v = wv; v < s.n; v += nw) {
    if (sol[v] || tight[v] != 0) continue;                     // wave uniform: one address for all lanes
    const int rv = s.rank[v];
    int any_in = 0, any_open = 0;
    for (int i = s.rp[v] + lane; i < s.rp[v + 1]; i += 64) {
      const int l = local_of(s, s.col[i], v);
      if (l >= 0 && s.rank[l] < rv) {
        const int in = sol[l];
        any_in |= in;
        any_open |= !in && tight[l] == 0;
      }
    }
    any_in = __any(any_in);
    any_open = __any(any_open);
    if (any_in) continue;                                      // out: the neighbour's push says so from now on
    if (any_open) { undecided = lane == 0; continue; }
    if (lane == 0) { s.sol[v] = 1; atomicAdd(&s.tally[1], 1); }
    push(s, v, 1);
  }
  return block_sum(s, undecided);
}

// mis_ls_propose_kernel; returns the proposals of the round.  v is in L(x) iff tight[v] == 1 && osum[v] == x.  The first two
// strides of x's row stay in registers for the three sweeps over it.
__device__ int propose_pass(Lds& s) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const unsigned long long none = ~0ull;
  int proposed = 0;
  for (int x = wv; x < s.n; x += nw) {
    if (!s.sol[x]) continue;                                   // wave uniform
    const int b = s.rp[x], e = s.rp[x + 1];
    const int r0 = b + lane < e ? local_of(s, s.col[b + lane], x) : -1;
    const int r1 = b + 64 + lane < e ? local_of(s, s.col[b + 64 + lane], x) : -1;
    const bool c0 = r0 >= 0 && s.tight[r0] == 1 && s.osum[r0] == x;      // tight / osum do not change during the pass
    const bool c1 = r1 >= 0 && s.tight[r1] == 1 && s.osum[r1] == x;
    int cnt = (int)c0 + (int)c1;
    for (int i = b + 128 + lane; i < e; i += 64) {
      const int v = local_of(s, s.col[i], x);
      cnt += v >= 0 && s.tight[v] == 1 && s.osum[v] == x;
    }
    cnt = wsum(cnt);
    int pu = -1, pw = -1;
    long long last = -1;                                       // rank of the candidate visited last
    while (cnt >= 2) {                                         // every turn visits a candidate of a larger rank: <= |L(x)| turns
      unsigned long long best = none;
      auto first = [&](int v) {
        if (s.rank[v] > last) {
          const unsigned long long key = ((unsigned long long)(unsigned)s.rank[v] << 32) | (unsigned)v;
          best = key < best ? key : best;
        }
      };
      if (c0) first(r0);
      if (c1) first(r1);
      for (int i = b + 128 + lane; i < e; i += 64) {
        const int v = local_of(s, s.col[i], x);
        if (v >= 0 && s.tight[v] == 1 && s.osum[v] == x) first(v);
      }
      best = wmin64(best);
      if (best == none) break;                                 // every candidate visited, none pairable
      const int u = (int)(unsigned)(best & 0xffffffffu);
      last = (long long)(best >> 32);
      int c = 0;
      for (int j = s.rp[u] + lane; j < s.rp[u + 1]; j += 64) {
        const int w = local_of(s, s.col[j], u);
        if (w >= 0 && w != x && s.tight[w] == 1 && s.osum[w] == x) {
          ++c;
          s.mark[w] = u;
        }
      }
      c = wsum(c);
      if (c >= cnt - 1) continue;                              // adjacent to every other candidate
      __threadfence_block();                                   // this wave's marks are in LDS before it reads them back
      unsigned long long second = none;
      auto other = [&](int v) {
        if (v != u && s.rank[v] > last && ((const volatile int*)s.mark)[v] != u) {
          const unsigned long long key = ((unsigned long long)(unsigned)s.rank[v] << 32) | (unsigned)v;
          second = key < second ? key : second;
        }
      };
      if (c0) other(r0);
      if (c1) other(r1);
      for (int i = b + 128 + lane; i < e; i += 64) {
        const int v = local_of(s, s.col[i], x);
        if (v >= 0 && s.tight[v] == 1 && s.osum[v] == x) other(v);
      }
      second = wmin64(second);
      if (second != none) { pu = u; pw = (int)(unsigned)(second & 0xffffffffu); }
      break;                                                   // no second node (duplicate entries): no proposal
    }
    if (lane == 0) {
      s.pu[x] = pu;
      s.pw[x] = pw;
      proposed += pu >= 0;
    }
  }
  return block_sum(s, proposed);
}

// mis_ls_conflict_kernel
__device__ void conflict_pass(Lds& s) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int x = wv; x < s.n; x += nw) {
    const int pu = s.sol[x] ? s.pu[x] : -1;                    // pu / pw of a member are this round's
    if (pu < 0) {                                              // wave uniform
      if (lane == 0) s.win[x] = 0;
      continue;
    }
    const int key = s.rank[pu];
    int lose = 0;
    for (int t = 0; t < 2; ++t) {
      const int a = t == 0 ? pu : s.pw[x];
      for (int j = s.rp[a] + lane; j < s.rp[a + 1]; j += 64) {
        const int q = local_of(s, s.col[j], a);
        if (q < 0 || s.tight[q] != 1) continue;
        const int y = s.osum[q];
        if (y == x || (unsigned)y >= (unsigned)s.n) continue;  // in range on a symmetric adjacency; never an index otherwise
        const int uy = s.pu[y];
        if (uy >= 0 && (uy == q || s.pw[y] == q)) lose |= s.rank[uy] < key;
      }
    }
    lose = __any(lose);
    if (lane == 0) s.win[x] = !lose;
  }
  __syncthreads();
}

// mis_ls_apply_kernel: win is 1 only for the members that won this round (the conflict pass wrote it for every node), so
// membership is never read from sol, which this pass writes.  The three nodes of a winner belong to no other winner.
__device__ void apply_pass(Lds& s) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int x = wv; x < s.n; x += nw) {
    if (!s.win[x]) continue;                                   // wave uniform
    const int u = s.pu[x], w = s.pw[x];
    if (lane == 0) {
      s.sol[x] = 0;
      s.sol[u] = 1;
      s.sol[w] = 1;
      atomicAdd(&s.tally[0], 1);
    }
    push(s, x, -1);
    push(s, u, 1);
    push(s, w, 1);
  }
  __syncthreads();
}

// THE DESCENT from the set in sol (tight / osum are its): one insertion phase, then rounds until one proposes nothing or `cap`
// rounds ran.  Returns the counted rounds.  The order of the steps is the launched search's (ls_enqueue_cycle behind the phase
// word), without its recomputations of tight.
__device__ int descent(Lds& s, int cap) {
  const int max_rounds = min(cap, s.n);
  int rounds = 0;
  for (;;) {                                                   // <= min(cap, n) + 1 turns
    for (int sub = 0; sub <= s.n; ++sub)                       // <= n + 1 sub-rounds
      if (insert_pass(s) == 0) break;
    if (rounds >= max_rounds) break;
    if (propose_pass(s) == 0) break;                           // a round without a proposal ends the descent, uncounted
    conflict_pass(s);
    apply_pass(s);
    ++rounds;
  }
  return rounds;
}

// mis_it_draw_kernel, mis_it_enter_kernel, mis_it_evict_kernel for kick t; sol is the incumbent.  Returns whether a node entered.
__device__ int kick(Lds& s, uint64_t seed, uint64_t offset, int t, int isize, int kick_size) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint64_t m = (uint64_t)((int64_t)s.n - (int64_t)isize);
  for (int v = threadIdx.x; v < s.n; v += blockDim.x) {
    int out = -1;
    if (!s.sol[v]) {
      uint32_t r[4];
      Philox::run(seed, offset + (uint64_t)t, (uint64_t)v, r);          // the index is the LOCAL node index
      const uint64_t w = r[0] >> 8;
      if (w * m < ((uint64_t)kick_size << 24)) out = (int)w;            // exact: w < 2^24, m < 2^31, kick_size < 2^31
    }
    s.kw[v] = out;
    s.ent[v] = 0;
  }
  __syncthreads();
  int entered = 0;
  for (int v = wv; v < s.n; v += nw) {
    const int wvv = s.kw[v];
    if (wvv < 0) continue;                                     // wave uniform
    const unsigned long long key = ((unsigned long long)(unsigned)wvv << 32) | (unsigned)v;
    int lose = 0;
    for (int i = s.rp[v] + lane; i < s.rp[v + 1]; i += 64) {
      const int u = local_of(s, s.col[i], v);
      if (u < 0) continue;
      const int wu = s.kw[u];
      if (wu >= 0) lose |= (((unsigned long long)(unsigned)wu << 32) | (unsigned)u) < key;
    }
    lose = __any(lose);
    if (lose) continue;
    if (lane == 0) { s.ent[v] = 1; s.sol[v] = 1; entered = 1; }
    push(s, v, 1);                                             // the members next to v now have tight > 0
  }
  entered = block_sum(s, entered);
  for (int v = wv; v < s.n; v += nw) {                         // evict: the members next to an entered node leave
    if (!s.sol[v] || s.ent[v] || s.tight[v] == 0) continue;    // wave uniform; tight of a member counts entered nodes only
    if (lane == 0) s.sol[v] = 0;
    push(s, v, -1);
  }
  __syncthreads();
  return entered != 0;
}

// C_b <- I_b: the nodes in which the two differ leave or enter, and push
__device__ void restore(Lds& s) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int v = wv; v < s.n; v += nw) {
    const int want = s.inc[v];
    if (s.sol[v] == want) continue;                            // wave uniform
    if (lane == 0) s.sol[v] = want;
    push(s, v, want ? 1 : -1);
  }
  __syncthreads();
}

__device__ int set_size(Lds& s) {
  int c = 0;
  for (int v = threadIdx.x; v < s.n; v += blockDim.x) c += s.sol[v] != 0;
  return block_sum(s, c);
}

__global__ void mis_res_setup_kernel(int nb, int kicks, int* __restrict__ kdone, int* __restrict__ isize,
                                     int* __restrict__ round_max, ResCtrl* __restrict__ rc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) { kdone[i] = -1; isize[i] = 0; }
  if (i <= kicks) round_max[i] = 0;
  if (i == 0) {
    rc->over = kNone;
    rc->over_nodes = rc->rounds = rc->swaps = rc->inserts = rc->bad = rc->bad_table = 0;
  }
}

// the first instance with more than `limit` nodes; reads the table only, whatever it holds
__global__ void mis_res_limit_kernel(int nb, int limit, const int64_t* __restrict__ rows, ResCtrl* __restrict__ rc) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < nb && rows[b + 1] - rows[b] > (int64_t)limit) atomicMin(&rc->over, b);
}

// One block per table row.  kdone[b]: kicks applied to instance b so far, -1 before its first descent.  Between launches the
// incumbent is in inc_g, its size in isize[b], the counters in per / rc / round_max.
__global__ __launch_bounds__(kThreads) void mis_res_search_kernel(
    int S, const int* __restrict__ rowptr, const int* __restrict__ col, const int* __restrict__ rank_g,
    const int* __restrict__ sol_g, int* __restrict__ inc_g, const int64_t* __restrict__ rows, const uint64_t* __restrict__ seeds,
    const uint64_t* __restrict__ offsets, int kicks, int kick_size, int cap, int kicks_per_launch, int* __restrict__ kdone,
    int* __restrict__ isize_g, int* __restrict__ per, int* __restrict__ round_max, ResCtrl* __restrict__ rc,
    const int* __restrict__ bad) {
  extern __shared__ int smem[];
  __shared__ int slot[3], tally[2];
  // nothing is written unless the set is independent, the table well formed and every instance within the limit
  if (*bad || rc->over != kNone) return;
  const int b = blockIdx.x;
  const int lo = (int)rows[b], n = (int)(rows[b + 1] - rows[b]);
  if (n == 0) return;                                          // an empty instance: per stays [0, 0, 0, 0]
  Lds s;
  s.rank = smem;
  s.tight = s.rank + S;
  s.osum = s.tight + S;
  s.mark = s.osum + S;
  s.kw = s.mark + S;
  s.pu = s.kw + S;
  s.pw = s.pu + S;
  s.rp = s.pw + S;
  s.sol = (uint8_t*)(s.rp + S + 4);
  s.inc = s.sol + S;
  s.ent = s.inc + S;
  s.win = s.ent + S;
  s.slot = slot;
  s.tally = tally;
  s.turn = 0;
  s.n = n;
  s.lo = lo;
  s.col = col;
  int done = kdone[b], isize = isize_g[b];                     // read by every thread long before thread 0 writes them
  const int* from = done < 0 ? sol_g : inc_g;
  for (int v = threadIdx.x; v < n; v += blockDim.x) {
    s.rank[v] = rank_g[lo + v];
    s.sol[v] = s.inc[v] = from[lo + v] != 0;
    s.mark[v] = -1;                                            // a mark is written in the pass that reads it: none to carry over
    s.rp[v] = rowptr[lo + v];
  }
  if (threadIdx.x == 0) {
    s.rp[n] = rowptr[lo + n];
    slot[0] = slot[1] = slot[2] = 0;
    tally[0] = tally[1] = 0;
  }
  __syncthreads();
  tight_from_scratch(s);
  int entered = 0, accepted = 0;
  if (done < 0) {                                              // step 1: the descent on the input set gives the incumbent
    const int r = descent(s, cap);
    if (threadIdx.x == 0) atomicMax(&round_max[0], r);
    isize = set_size(s);
    for (int v = threadIdx.x; v < n; v += blockDim.x) s.inc[v] = s.sol[v];
    if (threadIdx.x == 0) per[4 * b + 2] = isize;
    __syncthreads();
    done = 0;
  }
  const int end = min(kicks, done + kicks_per_launch);
  for (; done < end; ++done) {                                 // <= kicks_per_launch turns
    const int hit = kick(s, seeds[b], offsets[b], done, isize, kick_size);
    const int r = descent(s, cap);                             // also when nothing entered: a capped incumbent goes on descending
    if (threadIdx.x == 0) atomicMax(&round_max[done + 1], r);
    const int cnt = set_size(s);
    const int keep = cnt >= isize;
    if (keep) {                                                // the same in every thread
      for (int v = threadIdx.x; v < n; v += blockDim.x) s.inc[v] = s.sol[v];
      isize = cnt;
      __syncthreads();
    } else {
      restore(s);
    }
    entered += hit;
    accepted += hit && keep;
  }
  for (int v = threadIdx.x; v < n; v += blockDim.x) inc_g[lo + v] = s.inc[v];
  if (threadIdx.x == 0) {
    kdone[b] = done;
    isize_g[b] = isize;
    per[4 * b] += entered;
    per[4 * b + 1] += accepted;
    per[4 * b + 3] = isize;
    if (tally[0]) atomicAdd(&rc->swaps, tally[0]);
    if (tally[1]) atomicAdd(&rc->inserts, tally[1]);
  }
}

// solution <- the incumbents; rounds = the sum over the descents of the longest instance's rounds; the flags in one place
__global__ void mis_res_finish_kernel(int n, int kicks, const int* __restrict__ inc_g, int* __restrict__ solution,
                                      const int64_t* __restrict__ rows, const int* __restrict__ round_max,
                                      ResCtrl* __restrict__ rc, const int* __restrict__ bad, const int* __restrict__ bad_table) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const bool stop = *bad || rc->over != kNone;
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) {
      rc->bad = *bad;
      rc->bad_table = *bad_table;
      if (!*bad_table && rc->over != kNone) rc->over_nodes = (int)(rows[rc->over + 1] - rows[rc->over]);
    }
    if (!stop) {
      int sum = 0;
      for (int i = threadIdx.x; i <= kicks; i += blockDim.x) sum += round_max[i];
      if (sum) atomicAdd(&rc->rounds, sum);
    }
  }
  if (v < n && !stop) solution[v] = inc_g[v];
}

size_t up256(size_t x) { return (x + 255) / 256 * 256; }

struct ResCarve {                        // the launched search's workspace (the prelude's), then the state between launches
  int *kdone, *isize, *round_max;
  ResCtrl* rc;
  size_t total;
};

void res_carve(void* base, size_t prelude_bytes, int nb, int kicks, ResCarve* c) {
  size_t cur = up256(prelude_bytes);
  auto take = [&](size_t bytes) {
    size_t at = cur;
    cur += up256(bytes);
    return base ? (void*)((char*)base + at) : (void*)nullptr;
  };
  c->kdone = (int*)take(4 * (size_t)nb);
  c->isize = (int*)take(4 * (size_t)nb);
  c->round_max = (int*)take(4 * ((size_t)kicks + 1));
  c->rc = (ResCtrl*)take(sizeof(ResCtrl));
  c->total = cur;
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_mis_resident_max_nodes(void) { return difusco::kMaxNodes; }

int difusco_mis_resident_search_workspace_bytes(int n_nodes, int64_t n_edges, int n_instances, int32_t kicks, size_t* bytes) {
  using namespace difusco;
  if (!bytes || n_nodes < 1 || n_edges < 0 || n_instances < 1 || kicks < 0)
    return set_error(DIFUSCO_EINVAL, "mis_resident_search_workspace_bytes: bad arguments");
  MisSearchPrelude p;
  hipError_t er = mis_search_prelude(nullptr, n_nodes, n_instances, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &p);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  ResCarve c;
  res_carve(nullptr, p.bytes, n_instances, kicks, &c);
  *bytes = c.total;
  return DIFUSCO_OK;
}

int difusco_mis_resident_search(int n_nodes, const int32_t* rowptr, const int32_t* col, const float* scores, int32_t* solution,
                                int n_instances, const int64_t* instance_rows, const uint64_t* instance_seeds,
                                const uint64_t* instance_offsets, int32_t kicks, int32_t kick_size, int32_t max_rounds,
                                int32_t kicks_per_launch, void* workspace, size_t workspace_bytes, int32_t counters[3],
                                int32_t* per_instance, void* stream) {
  using namespace difusco;
  mis_search_set_host_syncs(0);
  if (n_nodes < 1 || !rowptr || !col || !scores || !solution || !workspace || !counters || !instance_rows || !instance_seeds ||
      !instance_offsets)
    return set_error(DIFUSCO_EINVAL, "mis_resident_search: null array or empty graph");
  if (n_instances < 1) return set_error(DIFUSCO_EINVAL, "mis_resident_search: n_instances = %d < 1", n_instances);
  if (max_rounds < 0) return set_error(DIFUSCO_EINVAL, "mis_resident_search: max_rounds = %d < 0", (int)max_rounds);
  if (kicks < 0) return set_error(DIFUSCO_EINVAL, "mis_resident_search: kicks = %d < 0", (int)kicks);
  if (kick_size < 1) return set_error(DIFUSCO_EINVAL, "mis_resident_search: kick_size = %d < 1", (int)kick_size);
  if (kicks_per_launch < 0)
    return set_error(DIFUSCO_EINVAL, "mis_resident_search: kicks_per_launch = %d < 0", (int)kicks_per_launch);
  const int n = n_nodes, nb = n_instances;
  MisSearchPrelude p;
  hipError_t er = mis_search_prelude(nullptr, n, nb, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &p);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  ResCarve c;
  res_carve(workspace, p.bytes, nb, kicks, &c);
  if (workspace_bytes < c.total)
    return set_error(DIFUSCO_EINVAL, "mis_resident_search: workspace %zu < %zu bytes", workspace_bytes, c.total);
  hipStream_t st = (hipStream_t)stream;
  const int S = ((n < kMaxNodes ? n : kMaxNodes) + 3) & ~3;             // no instance of the call is larger
  const size_t lds = 36 * (size_t)S + 16;
  static std::atomic<unsigned long long> attr_devices{0};
  er = ensure_max_dynamic_lds(attr_devices, reinterpret_cast<const void*>(&mis_res_search_kernel), 36 * kMaxNodes + 16);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "mis_resident_search: hipFuncSetAttribute: %s", hipGetErrorString(er));

  const int per_launch = kicks_per_launch > 0 ? kicks_per_launch : kDefaultKicksPerLaunch;
  const int launches = kicks == 0 ? 1 : (int)(((long long)kicks + per_launch - 1) / per_launch);
  const int most = nb > kicks + 1 ? nb : kicks + 1;
  hipLaunchKernelGGL(mis_res_setup_kernel, dim3((unsigned)(most / 256 + 1)), dim3(256), 0, st, nb, kicks, c.kdone, c.isize,
                     c.round_max, c.rc);
  er = mis_search_prelude(workspace, n, nb, rowptr, col, scores, solution, instance_rows, st, &p);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "mis_resident_search start: %s", hipGetErrorString(er));
  hipLaunchKernelGGL(mis_res_limit_kernel, dim3((unsigned)(nb / 256 + 1)), dim3(256), 0, st, nb, kMaxNodes, instance_rows, c.rc);
  for (int l = 0; l < launches; ++l)                                     // back to back: no poll between them
    hipLaunchKernelGGL(mis_res_search_kernel, dim3((unsigned)nb), dim3(kThreads), lds, st, S, rowptr, col, p.rank, p.sol, p.inc,
                       instance_rows, instance_seeds, instance_offsets, kicks, kick_size, max_rounds, per_launch, c.kdone,
                       c.isize, p.per, c.round_max, c.rc, p.bad);
  hipLaunchKernelGGL(mis_res_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, kicks, p.inc, solution,
                     instance_rows, c.round_max, c.rc, p.bad, p.bad_table);
  ResCtrl h;
  std::vector<int32_t> per(4 * (size_t)nb);
  er = hipMemcpyAsync(&h, c.rc, sizeof(h), hipMemcpyDeviceToHost, st);
  if (er == hipSuccess) er = hipMemcpyAsync(per.data(), p.per, per.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  if (er == hipSuccess) er = hipStreamSynchronize(st);                  // the one host synchronisation of the call
  mis_search_set_host_syncs(1);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "mis_resident_search: %s", hipGetErrorString(er));
  if (h.bad_table)
    return set_error(DIFUSCO_EINVAL, "mis_resident_search: instance_rows must start at 0, end at n_nodes and not decrease "
                                     "(solution unchanged)");
  if (h.over != kNone)
    return set_error(DIFUSCO_EUNSUPPORTED, "mis_resident_search: instance %d has %d nodes, above the limit of %d nodes per "
                                           "instance (difusco_mis_resident_max_nodes; solution unchanged)",
                     h.over, h.over_nodes, kMaxNodes);
  if (h.bad) return set_error(DIFUSCO_EINVAL, "mis_resident_search: the input set is not independent (solution unchanged)");
  counters[0] = h.rounds;
  counters[1] = h.swaps;
  counters[2] = h.inserts;
  if (per_instance) std::memcpy(per_instance, per.data(), per.size() * sizeof(int32_t));
  return DIFUSCO_OK;
}

}  // extern "C"
