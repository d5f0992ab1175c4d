// Heatmap -> tour: the greedy edge insertion that runs right after the sampling loop on every TSP sample
// (difusco/utils/tsp_utils.py:89-145 `merge_tours`, difusco/utils/cython_merge/cython_merge.pyx:19-104 `merge_cython`).
//
// The reference densifies the E-entry heatmap to N x N (A + A^T), divides by the N x N distance matrix and
// argsorts all N^2 entries on the host: 10^8 elements per TSP-10000 sample.  Only entries that are edges of the
// sparse graph (in either direction) are non-zero, and the walk over the sorted list ends after N-1 successful
// insertions, long before the zero entries - so the same tour comes out of the E candidate pairs alone:
//
//   device  1. key = min(i,j) * N + max(i,j) per directed edge; radix sort (rocPRIM) brings the two directions
//              of a pair together, pairs in flat-index order;
//           2. per pair: S = fl32(A_ij + A_ji) (the reference adds the two float32 matrices, tsp_utils.py:108-114),
//              score = double(S) / ||p_i - p_j||_2 in float64 (cython_merge.pyx:21,37), self loops set aside;
//           3. stable radix sort by score, descending (ties keep flat-index order);
//   host    4. greedy insertion over the sorted pairs with the reference's accept / reject decisions
//              (cython_merge.pyx:46-96), kept as path end points + node degrees, the closing edge, and the walk from node 0 that always takes the larger unvisited neighbour
//              (tsp_utils.py:134-141).
//
// `merge_iterations` reproduces the reference's count over its dense list: the self entries (score -inf, sorted
// first) + two entries per pair before the terminating one + 1.  If the candidate pairs with a positive score do
// not suffice for N-1 insertions the reference continues into its zero-valued entries, whose order is whatever
// numpy's unstable argsort leaves - not reproducible; this implementation then walks the zero block in flat-index
// order (a stable sort's order, as the CPU oracle does) and then the negative-score candidates, and reports
// completed = 0 so that callers (and tests) know the tour is outside the regime pinned to the reference.  In that
// regime merge_iterations counts the entries this implementation looked at, not the reference's.
//
// Non-finite scores rank as a stable ascending sort of -(A + A^T) / dist ranks them (numpy puts NaN last):
//   1. scores > 0 by decreasing score, +inf first (positive heat at distance 0, +inf heat);
//   2. the zero block: S == +-0 and every pair that is no edge, in flat-index order;
//   3. scores < 0 by decreasing score;
//   4. score -inf (negative heat at distance 0, -inf heat);
//   5. NaN of either sign (0/0, NaN heat, inf + -inf);
// equal scores, and the NaNs among themselves, in flat-index order.  pair_score_at states this once for every entry:
// it rewrites a candidate's NaN score to ONE sign-bit NaN pattern and marks the list positions that hold no candidate
// (non-heads of a run, self loops) with a second sign-bit NaN pattern and a `pair` value that is no pair.  Under
// rocPRIM's descending float order (sign-bit patterns are compared bit-inverted: -inf, then the sign-bit NaNs by
// increasing mantissa) the sorted list is blocks 1, 2 (its listed part), 3, 4, 5 and then, strictly after every
// candidate, the positions that are none.  completed = 1 exactly when all N-1 insertions came from block 1, and an
// entry of block 5 is never counted before a terminating entry of block 1.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <unordered_set>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "../../include/difusco_hip.h"
#include "kernels.h"

namespace difusco {
namespace {

__global__ void pair_key_kernel(const int* __restrict__ row, const int* __restrict__ col, long long n_edges, long long n,
                                unsigned long long* __restrict__ key, unsigned* __restrict__ val) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const long long i = row[e], j = col[e];
  const long long lo = i < j ? i : j, hi = i < j ? j : i;
  key[e] = (unsigned long long)(lo * n + hi);
  val[e] = (unsigned)e;
}

// How scores rank (header comment), stated once for the device kernels and the host walks.  A candidate's NaN score is
// stored as kScoreNaN; a list position that holds no candidate as kScoreNoPair with pair = kNoPair.  Both are sign-bit NaNs:
// radix_sort_pairs_desc puts them after -inf, and kScoreNaN (the smaller mantissa) strictly before kScoreNoPair.
constexpr unsigned long long kScoreNaN = 0xfff8000000000000ULL;
constexpr unsigned long long kScoreNoPair = 0xffffffffffffffffULL;
constexpr unsigned long long kNoPair = 0xffffffffffffffffULL;      // decodes to ids >= any n: refused by pair_nodes

__host__ __device__ __forceinline__ double score_from_bits(unsigned long long bits) {
  double v;
  memcpy(&v, &bits, sizeof(v));
  return v;
}
// block 1: the only entries the pinned walk (host loop and wave) inserts; false for NaN
__host__ __device__ __forceinline__ bool score_in_pinned_regime(double score) { return score > 0.0; }
// blocks 3-5: visited after the zero block, in list order (a listed entry of block 2 is found by the zero-block scan)
__host__ __device__ __forceinline__ bool score_after_zero_block(double score) { return score < 0.0 || score != score; }
// the node ids of a sorted-list entry; false for anything that is not a candidate pair of an n-node graph
__host__ __device__ __forceinline__ bool pair_nodes(unsigned long long pair, int n, int* i, int* j) {
  const unsigned long long a = pair >> 32, b = pair & 0xffffffffULL;
  *i = (int)a;
  *j = (int)b;
  return a < b && b < (unsigned long long)n;
}

// The score of position p of a pair-sorted edge list (one graph's, `n_edges` long).  The first position of a run of equal
// keys owns the pair: it sums the run's heat in float32 (a_ij first when both directions exist, like A + A^T evaluated at
// (i,j), i < j; float addition commutes, so (j,i) gets the same value) and emits score + packed (i,j).
// Everything else (non-heads, self loops) is no candidate: kScoreNoPair / kNoPair, strictly after every candidate in the
// sorted list, so that the first counters[0] sorted entries are exactly the candidates.  `key_mask` strips the graph index
// that the batched entry keeps above lo * n + hi (all ones for the single-graph entries).  Shared by pair_score_kernel and
// pair_score_batch_kernel: one statement of the arithmetic.
__device__ __forceinline__ void pair_score_at(const unsigned long long* __restrict__ key, const unsigned* __restrict__ val,
                                              const float* __restrict__ heat, const float* __restrict__ points, long long p,
                                              long long n_edges, long long n, unsigned long long key_mask,
                                              double* __restrict__ score, unsigned long long* __restrict__ pair,
                                              unsigned* __restrict__ counters) {   // [0] pairs, [1] self loops with S > 0
  const unsigned long long raw = key[p];
  const unsigned long long k = raw & key_mask;
  score[p] = score_from_bits(kScoreNoPair);
  pair[p] = kNoPair;
  if (p > 0 && key[p - 1] == raw) return;
  float s = heat[val[p]];
  long long q = p + 1;
  while (q < n_edges && key[q] == raw) {
    s += heat[val[q]];
    ++q;
  }
  const long long lo = (long long)(k / (unsigned long long)n), hi = (long long)(k % (unsigned long long)n);
  if (lo == hi) {
    // diagonal of A + A^T: A_ii + A_ii (tsp_utils.py:108-114); score -S/0 = -inf for S > 0 -> sorted first, skipped
    const float d = s + s;
    if (d > 0.0f) atomicAdd(&counters[1], 1u);
    return;
  }
  const double dx = (double)points[2 * lo] - (double)points[2 * hi];
  const double dy = (double)points[2 * lo + 1] - (double)points[2 * hi + 1];
  const double dist = sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));   // np.linalg.norm: no fused multiply-add
  const double sc = (double)s / dist;
  score[p] = sc != sc ? score_from_bits(kScoreNaN) : sc;
  pair[p] = ((unsigned long long)lo << 32) | (unsigned long long)hi;
  atomicAdd(&counters[0], 1u);
}

// One thread per position of the pair-sorted edge list of ONE graph and ONE sample.
__global__ void pair_score_kernel(const unsigned long long* __restrict__ key, const unsigned* __restrict__ val,
                                  const float* __restrict__ heat, const float* __restrict__ points, long long n_edges,
                                  long long n, double* __restrict__ score, unsigned long long* __restrict__ pair,
                                  unsigned* __restrict__ counters) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_edges) return;
  pair_score_at(key, val, heat, points, p, n_edges, n, ~0ULL, score, pair, counters);
}

struct Carve {
  unsigned long long *key_a, *key_b, *pair_a, *pair_b;
  unsigned *val_a, *val_b, *counters;
  double *score_a, *score_b;
  void* temp;
  size_t temp_bytes, total;
};

size_t up256(size_t x) { return (x + 255) / 256 * 256; }

hipError_t carve(void* base, long long E, Carve* c) {
  size_t t1 = 0, t2 = 0;
  hipError_t er = rocprim::radix_sort_pairs(nullptr, t1, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                            (unsigned*)nullptr, (unsigned*)nullptr, (size_t)E, 0, 64, 0, false);
  if (er != hipSuccess) return er;
  er = rocprim::radix_sort_pairs_desc(nullptr, t2, (double*)nullptr, (double*)nullptr, (unsigned long long*)nullptr,
                                      (unsigned long long*)nullptr, (size_t)E, 0, 64, 0, false);
  if (er != hipSuccess) return er;
  c->temp_bytes = t1 > t2 ? t1 : t2;
  size_t cur = 0;
  auto take = [&](size_t bytes) {
    size_t at = cur;
    cur += up256(bytes);
    return base ? (void*)((char*)base + at) : (void*)nullptr;
  };
  c->key_a = (unsigned long long*)take(8 * E);
  c->key_b = (unsigned long long*)take(8 * E);
  c->pair_a = (unsigned long long*)take(8 * E);
  c->pair_b = (unsigned long long*)take(8 * E);
  c->score_a = (double*)take(8 * E);
  c->score_b = (double*)take(8 * E);
  c->val_a = (unsigned*)take(4 * E);
  c->val_b = (unsigned*)take(4 * E);
  c->counters = (unsigned*)take(256);
  c->temp = take(c->temp_bytes);
  c->total = cur;
  return hipSuccess;
}

int merge_one_sample(const Carve& c, int n_nodes, long long E, const float* heat, const float* points, hipStream_t st,
                     int32_t* tour_out, int64_t* merge_iterations, int32_t* completed);

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_merge_workspace_bytes(int64_t n_edges, size_t* bytes) {
  if (!bytes || n_edges < 0) return difusco::set_error(DIFUSCO_EINVAL, "tsp_merge_workspace_bytes: bad arguments");
  difusco::Carve c;
  hipError_t er = difusco::carve(nullptr, n_edges > 0 ? n_edges : 1, &c);
  if (er != hipSuccess) return difusco::set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  *bytes = c.total;
  return DIFUSCO_OK;
}

// samples: heat [n_samples][n_edges], tour_out [n_samples][n_nodes + 1], merge_iterations / completed [n_samples] (optional).
// The pair keys depend on the graph only: one key sort serves every sample of the call.
static int merge_tours_impl(const char* who, int n_nodes, int64_t n_edges, const int32_t* row, const int32_t* col,
                            const float* heat, const float* points, int n_samples, void* workspace, size_t workspace_bytes,
                            int32_t* tour_out, int64_t* merge_iterations, int32_t* completed, void* stream) {
  using namespace difusco;
  if (n_nodes < 3 || n_edges <= 0 || n_samples < 1 || !row || !col || !heat || !points || !workspace || !tour_out)
    return set_error(DIFUSCO_EINVAL, "%s: needs n_nodes >= 3, n_edges > 0, n_samples >= 1 and non-null arrays", who);
  if (n_edges > 0xffffffffLL) return set_error(DIFUSCO_EINVAL, "%s: more than 2^32 edges in one graph", who);
  const long long E = n_edges, N = n_nodes;
  Carve c;
  hipError_t er = carve(workspace, E, &c);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  if (workspace_bytes < c.total)
    return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", who, workspace_bytes, c.total);
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((E + 255) / 256);
  int key_bits = 1;
  while (key_bits < 64 && (1ULL << key_bits) < (unsigned long long)(N * N)) ++key_bits;

  hipLaunchKernelGGL(pair_key_kernel, dim3(grid), dim3(256), 0, st, row, col, E, N, c.key_a, c.val_a);
  size_t tb = c.temp_bytes;
  er = rocprim::radix_sort_pairs(c.temp, tb, c.key_a, c.key_b, c.val_a, c.val_b, (size_t)E, 0, key_bits, st, false);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "radix_sort_pairs: %s", hipGetErrorString(er));
  for (int smp = 0; smp < n_samples; ++smp) {
    const int rc = merge_one_sample(c, n_nodes, E, heat + (long long)smp * E, points, st, tour_out + (long long)smp * (N + 1),
                                    merge_iterations ? merge_iterations + smp : nullptr, completed ? completed + smp : nullptr);
    if (rc != DIFUSCO_OK) return rc;
  }
  return DIFUSCO_OK;
}

int difusco_tsp_merge_tour(int n_nodes, int64_t n_edges, const int32_t* row, const int32_t* col, const float* heat,
                           const float* points, void* workspace, size_t workspace_bytes, int32_t* tour_out,
                           int64_t* merge_iterations, int32_t* completed, void* stream) {
  return merge_tours_impl("tsp_merge_tour", n_nodes, n_edges, row, col, heat, points, 1, workspace, workspace_bytes, tour_out,
                          merge_iterations, completed, stream);
}

int difusco_tsp_merge_tours(int n_nodes, int64_t n_edges, const int32_t* row, const int32_t* col, const float* heat,
                            const float* points, int n_samples, void* workspace, size_t workspace_bytes, int32_t* tours_out,
                            int64_t* merge_iterations, int32_t* completed, void* stream) {
  return merge_tours_impl("tsp_merge_tours", n_nodes, n_edges, row, col, heat, points, n_samples, workspace, workspace_bytes,
                          tours_out, merge_iterations, completed, stream);
}

}  // extern "C"

namespace difusco {
namespace {
// ---- host: greedy insertion (the accept / reject rule of cython_merge.pyx:26-104) ----------------------------
// The partial tour is a set of vertex-disjoint paths.  A candidate pair (i, j) is accepted iff both nodes still have a free
// side and they are not the two ends of one path (that would close a cycle early) - the same decisions as the reference's
// two union-find forests over route begins / ends, kept here as one array over path END POINTS: far_end[v] is the other
// end of the path v terminates (v itself while v is isolated; stale and never read once v is interior).
struct HostPaths {
  std::vector<int> far_end, degree, nb0, nb1;
  long long merge_count = 0;
  explicit HostPaths(int n_nodes) : far_end(n_nodes), degree(n_nodes, 0), nb0(n_nodes, -1), nb1(n_nodes, -1) {
    for (int v = 0; v < n_nodes; ++v) far_end[v] = v;
  }
  void link_nodes(int a, int b) {
    (nb0[a] < 0 ? nb0[a] : nb1[a]) = b;
    (nb0[b] < 0 ? nb0[b] : nb1[b]) = a;
  }
  bool try_insert(int i, int j) {
    if (degree[i] == 2 || degree[j] == 2 || far_end[i] == j) return false;
    const int tail_i = far_end[i], tail_j = far_end[j];   // the joined path runs tail_i .. i - j .. tail_j
    far_end[tail_i] = tail_j;
    far_end[tail_j] = tail_i;
    ++degree[i];
    ++degree[j];
    link_nodes(i, j);
    ++merge_count;
    return true;
  }
};

// Outside the pinned regime: `pairs` / `scores` are the `count` entries of the sample's sorted list from the position at
// which its positive scores ended.  The dense list continues with its zero block (all entries with S == 0: the pairs
// that are not edges of the sparse graph, and candidates whose heat sums to exactly 0), then the entries with
// S < 0 (Gaussian heat can be negative) by decreasing score.  The reference's order INSIDE the zero block is an
// accident of numpy's unstable argsort; here it is flat-index order (what a stable sort gives, and what
// oracle/tsp_decode_oracle.py does): pairs (a, b), a < b, lexicographic.  Only path end points can be joined, so
// the scan walks end points instead of all N^2 / 2 pairs.  Called by the per-sample host walk and by the batched entry.
// After the zero block come the listed entries that score_after_zero_block names, in list order: negative scores by
// decreasing score, -inf, NaN last.  Every entry is a candidate pair by construction (the callers pass at most the
// counters[0] candidates, which sort before every other position); one that does not decode to two nodes of the graph
// is refused, never used as an index.
int finish_outside_regime(HostPaths& s, int n_nodes, const unsigned long long* pairs, const double* scores, size_t count) {
  const long long N = n_nodes;
  int i, j;
  std::unordered_set<unsigned long long> later;
  for (size_t q = 0; q < count; ++q) {
    if (!pair_nodes(pairs[q], n_nodes, &i, &j))
      return set_error(DIFUSCO_EINVAL, "tsp_merge_tour: sorted entry %zu of the tail is no pair of a %d-node graph", q, n_nodes);
    if (score_after_zero_block(scores[q])) later.insert(pairs[q]);
  }
  for (int a = 0; a < n_nodes && s.merge_count < N - 1; ++a) {
    if (s.nb1[a] >= 0) continue;
    for (int b = a + 1; b < n_nodes && s.merge_count < N - 1; ++b) {
      if (s.nb1[b] >= 0) continue;
      if (!later.empty() && later.count(((unsigned long long)a << 32) | (unsigned long long)b)) continue;
      if (s.try_insert(a, b) && s.nb1[a] >= 0) break;
    }
  }
  for (size_t q = 0; q < count && s.merge_count < N - 1; ++q) {
    if (!score_after_zero_block(scores[q])) continue;
    pair_nodes(pairs[q], n_nodes, &i, &j);
    s.try_insert(i, j);
  }
  return DIFUSCO_OK;
}

// The closing edge of the Hamiltonian path and the walk from node 0 (tsp_utils.py:134-141).
int close_and_walk(HostPaths& s, int n_nodes, int32_t* tour_out) {
  if (s.merge_count != (long long)n_nodes - 1)
    return set_error(DIFUSCO_EINVAL, "tsp_merge_tour: could not assemble a Hamiltonian path");
  int open_end = 0;                                     // one end of the Hamiltonian path; far_end gives the other
  while (open_end < n_nodes && s.degree[open_end] == 2) ++open_end;
  s.link_nodes(s.far_end[open_end], open_end);
  // tsp_utils.py:134-141: walk from node 0, always to the larger-numbered neighbour that is not the previous node
  tour_out[0] = 0;
  int prev = -1, cur = 0;
  for (int step = 1; step <= n_nodes; ++step) {
    int a = s.nb0[cur], b = s.nb1[cur], nxt;
    if (prev < 0) nxt = a > b ? a : b;
    else if (a == prev && b == prev) nxt = a;            // (2-cycles cannot occur for N >= 3)
    else if (a == prev) nxt = b;
    else if (b == prev) nxt = a;
    else nxt = a > b ? a : b;
    tour_out[step] = nxt;
    prev = cur;
    cur = nxt;
  }
  return DIFUSCO_OK;
}

// steps 2-4 of the header comment for ONE sample; c.key_b / c.val_b hold the pair-sorted edge list of the graph
int merge_one_sample(const Carve& c, int n_nodes, long long E, const float* heat, const float* points, hipStream_t st,
                     int32_t* tour_out, int64_t* merge_iterations, int32_t* completed) {
  const long long N = n_nodes;
  const unsigned grid = (unsigned)((E + 255) / 256);
  size_t tb = c.temp_bytes;
  hipError_t er = hipMemsetAsync(c.counters, 0, 256, st);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "memset: %s", hipGetErrorString(er));
  hipLaunchKernelGGL(pair_score_kernel, dim3(grid), dim3(256), 0, st, c.key_b, c.val_b, heat, points, E, N, c.score_a,
                     c.pair_a, c.counters);
  tb = c.temp_bytes;
  er = rocprim::radix_sort_pairs_desc(c.temp, tb, c.score_a, c.score_b, c.pair_a, c.pair_b, (size_t)E, 0, 64, st, false);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "radix_sort_pairs_desc: %s", hipGetErrorString(er));
  unsigned counters[2] = {0, 0};
  er = hipMemcpyAsync(counters, c.counters, sizeof(counters), hipMemcpyDeviceToHost, st);
  if (er == hipSuccess) er = hipStreamSynchronize(st);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "counters: %s", hipGetErrorString(er));
  const size_t n_pairs = counters[0];
  std::vector<unsigned long long> pairs(n_pairs);
  std::vector<double> scores(n_pairs);
  if (n_pairs) {
    er = hipMemcpyAsync(pairs.data(), c.pair_b, 8 * n_pairs, hipMemcpyDeviceToHost, st);
    if (er == hipSuccess) er = hipMemcpyAsync(scores.data(), c.score_b, 8 * n_pairs, hipMemcpyDeviceToHost, st);
    if (er == hipSuccess) er = hipStreamSynchronize(st);
    if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "sorted pairs: %s", hipGetErrorString(er));
  }

  HostPaths paths(n_nodes);
  long long iterations = counters[1];   // the -inf self entries come first in the dense order
  int within = 0;
  size_t k = 0;
  for (; k < n_pairs && paths.merge_count < N - 1; ++k) {
    if (!score_in_pinned_regime(scores[k])) break;       // the pinned regime ends with the positive scores
    int i, j;
    if (!pair_nodes(pairs[k], n_nodes, &i, &j))
      return set_error(DIFUSCO_EINVAL, "tsp_merge_tour: sorted entry %zu is no pair of a %d-node graph", k, n_nodes);
    // dense order: (i,j) and (j,i) are adjacent with equal scores; the first one met does the insertion
    iterations += 1;
    paths.try_insert(i, j);
    if (paths.merge_count == N - 1) break;
    iterations += 1;
  }
  if (paths.merge_count == N - 1) within = 1;
  int rc = DIFUSCO_OK;
  if (paths.merge_count < N - 1) rc = finish_outside_regime(paths, n_nodes, pairs.data() + k, scores.data() + k, n_pairs - k);
  if (rc == DIFUSCO_OK) rc = close_and_walk(paths, n_nodes, tour_out);
  if (rc != DIFUSCO_OK) return rc;
  if (merge_iterations) *merge_iterations = iterations;
  if (completed) *completed = within;
  return DIFUSCO_OK;
}
}  // namespace
}  // namespace difusco

// ---- batched merge: G graphs of any sizes, P_g samples each, one launch sequence -------------------------------------
// (difusco_tsp_merge_batch).  The call-wide arrays hold the graphs' edge lists back to back (`total_edges`
// entries) and the samples' lists back to back in (graph, sample) order (`total_list` entries, the layout of `heat`).
//   1. pair_key_batch_kernel + one stable radix sort of (graph index << key_bits) | (lo * n_g + hi): inside a graph the
//      order of pair_key_kernel + radix_sort_pairs, shared by the graph's samples;
//   2. pair_score_batch_kernel: pair_score_at for every (graph, sample) in one launch;
//   3. one stable descending sort of all scores, one stable sort by sample index, one gather: every sample's list by
//      descending score, ties in flat-index order (what radix_sort_pairs_desc gives one sample);
//   4. merge_insert_kernel: one 64-lane wave per sample does the greedy insertion, the closing edge and the tour walk;
//   5. one copy returns records and tours; only samples whose positive scores ran out go through finish_outside_regime.
namespace difusco {
namespace {

constexpr int kMergeWave = 64;
constexpr int kMergeLdsBytes = 160 * 1024;                 // path state of a sample in LDS when 12 * n_g fits: one workgroup
constexpr int kMergeLdsNodes = kMergeLdsBytes / 12;        // may take the whole LDS of a CU; 13653 nodes
constexpr uint32_t kMergeKnownFlags = DIFUSCO_MERGE_STATE_GLOBAL;

struct MergeGraph {
  long long edge_off;     // first entry of the graph's edge list in the call-wide edge arrays
  int n, pad;
};

struct MergeSample {      // one per (graph, sample), in (graph, sample) order
  long long list_off;     // first entry of the sample's list in the call-wide list arrays (= its offset in heat)
  long long edge_off;     // first entry of its graph's pair-sorted edge list
  long long n_edges;
  long long node_off;     // nodes of the graphs before its graph (points)
  long long state_off;    // nodes of the samples before it (path state, 3 ints per node)
  long long tour_off;     // ints of the tours before its tour
  int n, graph;
};

struct MergeRecord {      // what the insert kernel leaves per sample; 32 bytes
  long long iterations;   // merge_iterations
  long long position;     // list position at which the walk ended (the terminating pair, or the first non-positive score)
  unsigned counters[2];   // [0] candidate pairs, [1] self loops with S > 0 (pair_score_at)
  int completed;
  int merge_count;        // insertions made
};

__device__ __forceinline__ int graph_of_edge(const MergeGraph* __restrict__ graphs, int n_graphs, long long e) {
  int lo = 0, hi = n_graphs - 1;                           // last graph with edge_off <= e
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (graphs[mid].edge_off <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int sample_of_entry(const MergeSample* __restrict__ samples, int n_samples, long long q) {
  int lo = 0, hi = n_samples - 1;                          // last sample with list_off <= q
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (samples[mid].list_off <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// pair_key_kernel for every graph of the call; row == nullptr: complete graphs, entry (i, j) at i * n_g + j
__global__ void pair_key_batch_kernel(const MergeGraph* __restrict__ graphs, int n_graphs, const int* __restrict__ row,
                                      const int* __restrict__ col, long long total_edges, int key_bits,
                                      unsigned long long* __restrict__ key, unsigned* __restrict__ val) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total_edges) return;
  const int g = graph_of_edge(graphs, n_graphs, e);
  const long long local = e - graphs[g].edge_off, n = graphs[g].n;
  const long long i = row ? (long long)row[e] : local / n, j = row ? (long long)col[e] : local % n;
  const long long lo = i < j ? i : j, hi = i < j ? j : i;
  const unsigned long long high = key_bits < 64 ? (unsigned long long)g << key_bits : 0ULL;
  key[e] = high | (unsigned long long)(lo * n + hi);
  val[e] = (unsigned)local;
}

__global__ void pair_score_batch_kernel(const MergeSample* __restrict__ samples, int n_samples,
                                        const unsigned long long* __restrict__ key, const unsigned* __restrict__ val,
                                        const float* __restrict__ heat, const float* __restrict__ points, long long total_list,
                                        unsigned long long key_mask, double* __restrict__ score,
                                        unsigned long long* __restrict__ pair, unsigned* __restrict__ index,
                                        MergeRecord* __restrict__ records) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total_list) return;
  const int s = sample_of_entry(samples, n_samples, q);
  const MergeSample d = samples[s];
  index[q] = (unsigned)q;
  pair_score_at(key + d.edge_off, val + d.edge_off, heat + d.list_off, points + 2 * d.node_off, q - d.list_off, d.n_edges,
                (long long)d.n, key_mask, score + d.list_off, pair + d.list_off, records[s].counters);
}

__global__ void entry_sample_kernel(const MergeSample* __restrict__ samples, int n_samples, const unsigned* __restrict__ index,
                                    long long total_list, unsigned* __restrict__ sample) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total_list) return;
  sample[r] = (unsigned)sample_of_entry(samples, n_samples, (long long)index[r]);
}

__global__ void gather_sorted_kernel(const unsigned* __restrict__ index, const double* __restrict__ score_in,
                                     const unsigned long long* __restrict__ pair_in, long long total_list,
                                     double* __restrict__ score_out, unsigned long long* __restrict__ pair_out) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total_list) return;
  const unsigned q = index[r];
  score_out[r] = score_in[q];
  pair_out[r] = pair_in[q];
}

// The greedy insertion of merge_one_sample for one sample, by one wave.  far / nb0 / nb1 [n]: the path state (LDS or
// workspace); a node has degree 2 iff nb1 >= 0.  Lane 0 alone changes the state, every lane reads it: the block-wide
// barriers around the writes (one wave per block) order the two.
__device__ __forceinline__ void merge_insert_wave(const MergeSample& d, const double* __restrict__ score,
                                                  const unsigned long long* __restrict__ pair, int* far, int* nb0, int* nb1,
                                                  int* saved, MergeRecord* __restrict__ rec,
                                                  int* __restrict__ tour) {
  const int lane = threadIdx.x, n = d.n;
  const long long E = d.n_edges;
  for (int v = lane; v < n; v += kMergeWave) {
    far[v] = v;
    nb0[v] = -1;
    nb1[v] = -1;
  }
  __syncthreads();
  int count = 0;
  bool complete = false;
  long long position = E;
  for (long long base = 0; base < E; base += kMergeWave) {
    const long long q = base + lane;
    const double sc = q < E ? score[q] : 0.0;
    const unsigned long long pr = q < E ? pair[q] : 0ULL;
    // the walk ends at the first score outside block 1 (NaN sorts last: it never cuts the positive scores short); lanes
    // [0, n_pos) hold candidate pairs - by construction, and a lane whose entry does not decode to two nodes of the graph
    // reads no state
    const unsigned long long not_pos = __ballot(!(q < E && score_in_pinned_regime(sc)));
    const int n_pos = not_pos ? __ffsll((unsigned long long)not_pos) - 1 : kMergeWave;
    int i, j;
    const bool is_pair = pair_nodes(pr, n, &i, &j);
    // degrees only grow: a pair with a full endpoint can never be accepted later
    unsigned long long alive = __ballot(lane < n_pos && is_pair && nb1[i] < 0 && nb1[j] < 0);
    while (alive) {
      const int l = __ffsll(alive) - 1;
      alive &= alive - 1;
      const int a = __shfl(i, l), b = __shfl(j, l);
      const int tail_a = far[a], tail_b = far[b];
      const bool accept = nb1[a] < 0 && nb1[b] < 0 && tail_a != b;     // try_insert of HostPaths
      __syncthreads();
      if (!accept) continue;
      if (lane == 0) {
        far[tail_a] = tail_b;
        far[tail_b] = tail_a;
        (nb0[a] < 0 ? nb0[a] : nb1[a]) = b;
        (nb0[b] < 0 ? nb0[b] : nb1[b]) = a;
      }
      __syncthreads();
      if (++count == n - 1) {
        complete = true;
        position = base + l;
        break;
      }
    }
    if (complete) break;
    if (n_pos < kMergeWave) {
      position = base + n_pos;
      break;
    }
  }
  if (complete) {
    int open_end = -1;                                    // close_and_walk: the first node of degree < 2
    for (int base = 0; base < n && open_end < 0; base += kMergeWave) {
      const int v = base + lane;
      const unsigned long long open = __ballot(v < n && nb1[v] < 0);
      if (open) open_end = base + __ffsll(open) - 1;
    }
    if (lane == 0) {
      const int a = far[open_end], b = open_end;
      (nb0[a] < 0 ? nb0[a] : nb1[a]) = b;
      (nb0[b] < 0 ? nb0[b] : nb1[b]) = a;
      tour[0] = 0;
      int prev = -1, cur = 0;
      for (int step = 1; step <= n; ++step) {
        const int x = nb0[cur], y = nb1[cur];
        int nxt;
        if (prev < 0) nxt = x > y ? x : y;
        else if (x == prev && y == prev) nxt = x;
        else if (x == prev) nxt = y;
        else if (y == prev) nxt = x;
        else nxt = x > y ? x : y;
        tour[step] = nxt;
        prev = cur;
        cur = nxt;
      }
    }
  } else if (saved != far) {                              // the host finishes this sample: leave the state in the workspace
    for (int v = lane; v < n; v += kMergeWave) {
      saved[v] = far[v];
      saved[n + v] = nb0[v];
      saved[2 * n + v] = nb1[v];
    }
  }
  if (lane == 0) {
    // the dense list: the self entries first, two entries per pair before the terminating one, + 1 when it completes
    rec->iterations = (long long)rec->counters[1] + 2 * position + (complete ? 1 : 0);
    rec->position = position;
    rec->completed = complete ? 1 : 0;
    rec->merge_count = count;
  }
}

__global__ __launch_bounds__(kMergeWave) void merge_insert_kernel(const MergeSample* __restrict__ samples,
                                                                  const double* __restrict__ score,
                                                                  const unsigned long long* __restrict__ pair,
                                                                  int* __restrict__ state, MergeRecord* __restrict__ records,
                                                                  int* __restrict__ tours, int lds_nodes) {
  extern __shared__ int merge_lds[];
  const MergeSample d = samples[blockIdx.x];
  int* saved = state + 3 * d.state_off;
  if (d.n <= lds_nodes)
    merge_insert_wave(d, score + d.list_off, pair + d.list_off, merge_lds, merge_lds + d.n, merge_lds + 2 * d.n, saved,
                      records + blockIdx.x, tours + d.tour_off);
  else
    merge_insert_wave(d, score + d.list_off, pair + d.list_off, saved, saved + d.n, saved + 2 * d.n, saved,
                      records + blockIdx.x, tours + d.tour_off);
}

struct BatchPlan {
  std::vector<MergeGraph> graphs;
  std::vector<MergeSample> samples;
  long long total_edges = 0, total_list = 0, total_state = 0, total_tour = 0;
  int key_bits = 1, graph_bits = 0, sample_bits = 0, lds_nodes_max = 0;
};

struct BatchCarve {
  unsigned long long *key_a, *key_b, *pair_a, *pair_b;
  unsigned *val_a, *val_b, *index_a, *index_b, *sample_a, *sample_b;
  double *score_a, *score_b;
  int* state;
  MergeGraph* graphs;
  MergeSample* samples;
  MergeRecord* records;   // followed by the tours: one region, one copy back
  int* tours;
  size_t result_bytes;
  void* temp;
  size_t temp_bytes, total;
};

int bits_for(unsigned long long count) {                   // bits that hold 0 .. count - 1
  int b = 0;
  while (b < 64 && (1ULL << b) < count) ++b;
  return b;
}

// the host checks of both entries: no device is touched
int plan_batch(const char* who, int graphs, const int32_t* graph_n, const int64_t* graph_edges, const int32_t* graph_samples,
               bool dense, BatchPlan* plan) {
  if (graphs < 1) return set_error(DIFUSCO_EINVAL, "%s: graphs = %d, needs at least one", who, graphs);
  if (!graph_n || !graph_edges || !graph_samples)
    return set_error(DIFUSCO_EINVAL, "%s: null graph_n / graph_edges / graph_samples table", who);
  unsigned long long max_keys = 1;
  long long nodes = 0;
  for (int g = 0; g < graphs; ++g) {
    const long long n = graph_n[g], E = graph_edges[g], P = graph_samples[g];
    if (n < 3) return set_error(DIFUSCO_EINVAL, "%s: graph %d has n = %lld, needs at least 3", who, g, n);
    if (E <= 0 || E > (1LL << 32))
      return set_error(DIFUSCO_EINVAL, "%s: graph %d has %lld edges, needs 1 .. 2^32", who, g, E);
    if (dense && E != n * n)
      return set_error(DIFUSCO_EINVAL, "%s: graph %d is complete (no row / col): %lld edges given, n^2 = %lld", who, g, E, n * n);
    if (P < 1) return set_error(DIFUSCO_EINVAL, "%s: graph %d has %lld samples, needs at least 1", who, g, P);
    plan->graphs.push_back(MergeGraph{plan->total_edges, (int)n, 0});
    for (long long s = 0; s < P; ++s) {
      plan->samples.push_back(MergeSample{plan->total_list, plan->total_edges, E, nodes, plan->total_state, plan->total_tour,
                                          (int)n, g});
      plan->total_list += E;
      plan->total_state += n;
      plan->total_tour += n + 1;
      if (plan->total_list > (1LL << 32))
        return set_error(DIFUSCO_EINVAL, "%s: more than 2^32 list entries (samples x edges) in one call", who);
      if (plan->samples.size() > (size_t)0x7fffffff) return set_error(DIFUSCO_EINVAL, "%s: more than 2^31 - 1 samples", who);
    }
    plan->total_edges += E;
    nodes += n;
    if ((unsigned long long)(n * n) > max_keys) max_keys = (unsigned long long)(n * n);
    if (n <= kMergeLdsNodes && n > plan->lds_nodes_max) plan->lds_nodes_max = (int)n;
  }
  plan->key_bits = bits_for(max_keys) < 1 ? 1 : bits_for(max_keys);
  plan->graph_bits = bits_for((unsigned long long)graphs);
  plan->sample_bits = bits_for((unsigned long long)plan->samples.size());
  if (plan->key_bits + plan->graph_bits > 64)
    return set_error(DIFUSCO_EINVAL, "%s: graph index and pair key need %d bits, 64 available", who,
                     plan->key_bits + plan->graph_bits);
  return DIFUSCO_OK;
}

// with_temp = false: the layout without the rocPRIM scratch (a lower bound that needs no device)
hipError_t carve_batch(void* base, const BatchPlan& plan, bool with_temp, BatchCarve* c) {
  const size_t Et = (size_t)plan.total_edges, Lt = (size_t)plan.total_list;
  c->temp_bytes = 0;
  if (with_temp) {
    size_t t1 = 0, t2 = 0, t3 = 0;
    hipError_t er = rocprim::radix_sort_pairs(nullptr, t1, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                              (unsigned*)nullptr, (unsigned*)nullptr, Et, 0, 64, 0, false);
    if (er != hipSuccess) return er;
    er = rocprim::radix_sort_pairs_desc(nullptr, t2, (double*)nullptr, (double*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr,
                                        Lt, 0, 64, 0, false);
    if (er != hipSuccess) return er;
    er = rocprim::radix_sort_pairs(nullptr, t3, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr,
                                   Lt, 0, 32, 0, false);
    if (er != hipSuccess) return er;
    c->temp_bytes = t1 > t2 ? t1 : t2;
    if (t3 > c->temp_bytes) c->temp_bytes = t3;
  }
  size_t cur = 0;
  auto take = [&](size_t bytes) {
    size_t at = cur;
    cur += up256(bytes);
    return base ? (void*)((char*)base + at) : (void*)nullptr;
  };
  c->key_a = (unsigned long long*)take(8 * Et);
  c->key_b = (unsigned long long*)take(8 * Et);
  c->val_a = (unsigned*)take(4 * Et);
  c->val_b = (unsigned*)take(4 * Et);
  c->score_a = (double*)take(8 * Lt);
  c->score_b = (double*)take(8 * Lt);
  c->pair_a = (unsigned long long*)take(8 * Lt);
  c->pair_b = (unsigned long long*)take(8 * Lt);
  c->index_a = (unsigned*)take(4 * Lt);
  c->index_b = (unsigned*)take(4 * Lt);
  c->sample_a = (unsigned*)take(4 * Lt);
  c->sample_b = (unsigned*)take(4 * Lt);
  c->state = (int*)take(12 * (size_t)plan.total_state);
  c->graphs = (MergeGraph*)take(sizeof(MergeGraph) * plan.graphs.size());
  c->samples = (MergeSample*)take(sizeof(MergeSample) * plan.samples.size());
  const size_t record_bytes = sizeof(MergeRecord) * plan.samples.size();
  c->result_bytes = record_bytes + 4 * (size_t)plan.total_tour;
  c->records = (MergeRecord*)take(c->result_bytes);
  c->tours = base ? (int*)((char*)c->records + record_bytes) : nullptr;
  c->temp = take(c->temp_bytes);
  c->total = cur;
  return hipSuccess;
}

unsigned blocks_of(long long items) { return (unsigned)((items + 255) / 256); }

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_merge_batch_workspace_bytes(int graphs, const int32_t* graph_n, const int64_t* graph_edges,
                                            const int32_t* graph_samples, size_t* bytes) {
  using namespace difusco;
  const char* who = "tsp_merge_batch_workspace_bytes";
  if (!bytes) return set_error(DIFUSCO_EINVAL, "%s: null bytes", who);
  BatchPlan plan;
  const int rc = plan_batch(who, graphs, graph_n, graph_edges, graph_samples, false, &plan);
  if (rc != DIFUSCO_OK) return rc;
  BatchCarve c;
  hipError_t er = carve_batch(nullptr, plan, true, &c);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  *bytes = c.total;
  return DIFUSCO_OK;
}

int difusco_tsp_merge_batch(int graphs, const int32_t* graph_n, const int64_t* graph_edges, const int32_t* graph_samples,
                            const int32_t* row, const int32_t* col, const float* heat, const float* points, uint32_t flags,
                            void* workspace, size_t workspace_bytes, int32_t* tours_out, int64_t* merge_iterations,
                            int32_t* completed, void* stream) {
  using namespace difusco;
  const char* who = "tsp_merge_batch";
  if (!heat || !points || !workspace || !tours_out)
    return set_error(DIFUSCO_EINVAL, "%s: needs non-null heat, points, workspace and tours_out", who);
  if ((row == nullptr) != (col == nullptr))
    return set_error(DIFUSCO_EINVAL, "%s: row and col are both given or both null (complete graphs)", who);
  if (flags & ~kMergeKnownFlags) return set_error(DIFUSCO_EINVAL, "%s: unknown flag bits 0x%x", who, flags & ~kMergeKnownFlags);
  BatchPlan plan;
  int rc = plan_batch(who, graphs, graph_n, graph_edges, graph_samples, row == nullptr, &plan);
  if (rc != DIFUSCO_OK) return rc;
  BatchCarve c;
  carve_batch(workspace, plan, false, &c);                // everything but the sort scratch: refused without a device
  if (workspace_bytes < c.total)
    return set_error(DIFUSCO_EINVAL, "%s: workspace %zu bytes is below the %zu bytes of its arrays alone", who, workspace_bytes,
                     c.total);
  hipError_t er = carve_batch(workspace, plan, true, &c);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  if (workspace_bytes < c.total)
    return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", who, workspace_bytes, c.total);

  hipStream_t st = (hipStream_t)stream;
  const int G = graphs, S = (int)plan.samples.size();
  const long long Et = plan.total_edges, Lt = plan.total_list;
  auto fail = [&](const char* what, hipError_t e) { return set_error(DIFUSCO_EHIP, "%s: %s: %s", who, what, hipGetErrorString(e)); };
  er = hipMemcpyAsync(c.graphs, plan.graphs.data(), sizeof(MergeGraph) * G, hipMemcpyHostToDevice, st);
  if (er == hipSuccess) er = hipMemcpyAsync(c.samples, plan.samples.data(), sizeof(MergeSample) * S, hipMemcpyHostToDevice, st);
  if (er == hipSuccess) er = hipMemsetAsync(c.records, 0, sizeof(MergeRecord) * S, st);
  if (er != hipSuccess) return fail("tables", er);

  // 1. pair keys of every graph, one stable sort
  hipLaunchKernelGGL(pair_key_batch_kernel, dim3(blocks_of(Et)), dim3(256), 0, st, c.graphs, G, row, col, Et, plan.key_bits,
                     c.key_a, c.val_a);
  size_t tb = c.temp_bytes;
  er = rocprim::radix_sort_pairs(c.temp, tb, c.key_a, c.key_b, c.val_a, c.val_b, (size_t)Et, 0,
                                 plan.key_bits + plan.graph_bits, st, false);
  if (er != hipSuccess) return fail("radix_sort_pairs (keys)", er);
  // 2. scores of every (graph, sample)
  const unsigned long long key_mask = plan.key_bits < 64 ? (1ULL << plan.key_bits) - 1 : ~0ULL;
  hipLaunchKernelGGL(pair_score_batch_kernel, dim3(blocks_of(Lt)), dim3(256), 0, st, c.samples, S, c.key_b, c.val_b, heat,
                     points, Lt, key_mask, c.score_a, c.pair_a, c.index_a, c.records);
  // 3. descending by score over the whole call, then stable by sample: every sample's list in radix_sort_pairs_desc order
  tb = c.temp_bytes;
  er = rocprim::radix_sort_pairs_desc(c.temp, tb, c.score_a, c.score_b, c.index_a, c.index_b, (size_t)Lt, 0, 64, st, false);
  if (er != hipSuccess) return fail("radix_sort_pairs_desc (scores)", er);
  const unsigned* order = c.index_b;
  if (S > 1) {
    hipLaunchKernelGGL(entry_sample_kernel, dim3(blocks_of(Lt)), dim3(256), 0, st, c.samples, S, c.index_b, Lt, c.sample_a);
    tb = c.temp_bytes;
    er = rocprim::radix_sort_pairs(c.temp, tb, c.sample_a, c.sample_b, c.index_b, c.index_a, (size_t)Lt, 0, plan.sample_bits, st,
                                   false);
    if (er != hipSuccess) return fail("radix_sort_pairs (samples)", er);
    order = c.index_a;
  }
  hipLaunchKernelGGL(gather_sorted_kernel, dim3(blocks_of(Lt)), dim3(256), 0, st, order, c.score_a, c.pair_a, Lt, c.score_b,
                     c.pair_b);
  // 4. one wave per sample
  const int lds_nodes = (flags & DIFUSCO_MERGE_STATE_GLOBAL) ? 0 : plan.lds_nodes_max;
  static std::atomic<unsigned long long> attr_devices{0};
  er = ensure_max_dynamic_lds(attr_devices, reinterpret_cast<const void*>(&merge_insert_kernel), kMergeLdsBytes);
  if (er != hipSuccess) return fail("hipFuncSetAttribute", er);
  hipLaunchKernelGGL(merge_insert_kernel, dim3((unsigned)S), dim3(kMergeWave), (size_t)12 * lds_nodes, st, c.samples, c.score_b,
                     c.pair_b, c.state, c.records, c.tours, lds_nodes);
  er = hipGetLastError();
  if (er != hipSuccess) return fail("launch", er);
  // 5. one copy back
  std::vector<unsigned char> result(c.result_bytes);
  er = hipMemcpyAsync(result.data(), c.records, c.result_bytes, hipMemcpyDeviceToHost, st);
  if (er == hipSuccess) er = hipStreamSynchronize(st);
  if (er != hipSuccess) return fail("results", er);
  const MergeRecord* recs = (const MergeRecord*)result.data();
  const int32_t* tours = (const int32_t*)(result.data() + sizeof(MergeRecord) * S);
  for (int s = 0; s < S; ++s) {
    const MergeSample& d = plan.samples[s];
    const MergeRecord& r = recs[s];
    int32_t* tour_out = tours_out + d.tour_off;
    if (merge_iterations) merge_iterations[s] = r.iterations;
    if (completed) completed[s] = r.completed;
    if (r.completed) {
      std::memcpy(tour_out, tours + d.tour_off, sizeof(int32_t) * (d.n + 1));
      continue;
    }
    // outside the pinned regime: the sample's state and the tail of its list come back, the host finishes it
    const size_t n = (size_t)d.n, n_pairs = r.counters[0], k = (size_t)r.position;
    const size_t tail = n_pairs > k ? n_pairs - k : 0;
    std::vector<int> state(3 * n);
    std::vector<unsigned long long> pairs(tail);
    std::vector<double> scores(tail);
    er = hipMemcpyAsync(state.data(), c.state + 3 * d.state_off, 12 * n, hipMemcpyDeviceToHost, st);
    if (er == hipSuccess && tail)
      er = hipMemcpyAsync(pairs.data(), c.pair_b + d.list_off + k, 8 * tail, hipMemcpyDeviceToHost, st);
    if (er == hipSuccess && tail)
      er = hipMemcpyAsync(scores.data(), c.score_b + d.list_off + k, 8 * tail, hipMemcpyDeviceToHost, st);
    if (er == hipSuccess) er = hipStreamSynchronize(st);
    if (er != hipSuccess) return fail("state of an unfinished sample", er);
    HostPaths paths(d.n);
    for (size_t v = 0; v < n; ++v) {
      paths.far_end[v] = state[v];
      paths.nb0[v] = state[n + v];
      paths.nb1[v] = state[2 * n + v];
      paths.degree[v] = (paths.nb0[v] >= 0) + (paths.nb1[v] >= 0);
    }
    paths.merge_count = r.merge_count;
    rc = finish_outside_regime(paths, d.n, pairs.data(), scores.data(), tail);
    if (rc == DIFUSCO_OK) rc = close_and_walk(paths, d.n, tour_out);
    if (rc != DIFUSCO_OK) return rc;
  }
  return DIFUSCO_OK;
}

}  // extern "C"
