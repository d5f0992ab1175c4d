// Heat-biased kicks (difusco_tsp_guided_search_ragged): the first cut of every draw of a kick falls on position p of the incumbent
// with a probability proportional to w_p = 65536 - (the quantised heat of the tour edge at p).  Included by or_opt_multi.hip in
// front of its keep / kick kernels: they are templates on `kHeat` and call heat_prefix, their draws (kick_draws) heat_pick,
// and its host side lays out the tables and launches the two kernels here (mls_layout, mls_run); the rule is stated in
// include/difusco_hip.h and restated in numpy in tests/tsp_heat_kick_emulation.py.  All of it is integer arithmetic.
//
//   heat_graph_check_kernel  once per call, before the search: row_ptr and col of every group are what the row scans rely on;
//   heat_table_kernel        once per call, behind the check: q by (tour, entry), duplicates resolved - entry e of row u holds the
//                            largest q(e') over the entries e' >= e of the row with the same column, so the FIRST entry of a
//                            pair holds q(u, v) and a scan may stop there;
//   heat_prefix              the block of a tour: w_k of every position of the incumbent (two row scans of the group's CSR, each
//                            up to its first match: k-NN rows list near cities first, where tour edges are), and W_0 .. W_n,
//                            their running sums, in the tour's own n + 1 words of the workspace;
//   heat_pick                one lane per draw: r = (w0 2^32 + w3) mod W_M and the position p with W_p <= r < W_p+1.
#pragma once

namespace difusco {
namespace {

struct MlHeatTour {        // offsets in elements: the group's first entry in row_ptr and in col, the tour's first in heat and
  long long rows, edges, heat;   // in the q table
  int n, count;            // the group's cities and edges
};

struct MlHeatGroup {       // a group's graph for the check
  int n, edges;
  long long rows, cols;    // its first entry in row_ptr and in col
};

template <bool kHeat>
struct HeatArgs {};        // the uniform kernels carry nothing

template <>
struct HeatArgs<true> {
  const int* row_ptr;
  const int* col;
  const unsigned short* q; // the q table, laid out as heat
  const MlHeatTour* tab;
  unsigned long long* W;   // n + 1 per tour, at the tour's `closed` offset
};

// q(e): float32 product, round to nearest even; a NaN counts as 0
__device__ __forceinline__ unsigned heat_q(float h) { return (unsigned)rintf(fminf(fmaxf(h, 0.0f), 1.0f) * 65535.0f); }

// q(u, v): the largest q(e) over the entries e of row u with col[e] == v, 0 if there is none - the table entry of the first
__device__ __forceinline__ unsigned heat_edge_q(const int* __restrict__ row_ptr, const int* __restrict__ col,
                                                const unsigned short* __restrict__ q, int u, int v) {
  const int e1 = row_ptr[u + 1];
  for (int e = row_ptr[u]; e < e1; ++e)
    if (col[e] == v) return q[e];
  return 0;
}

// one thread per (entry, tour) of a checked graph: the row of the entry by bisection of row_ptr, then the entries behind it
__global__ __launch_bounds__(256) void heat_table_kernel(const int* __restrict__ row_ptr_all, const int* __restrict__ col_all,
                                                         const float* __restrict__ heat_all, const MlHeatTour* __restrict__ tab,
                                                         unsigned short* __restrict__ q_all) {
  const MlHeatTour h = tab[blockIdx.y];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h.count) return;
  const int e = (int)i;
  const int* row_ptr = row_ptr_all + h.rows;
  const int* col = col_all + h.edges;
  const float* heat = heat_all + h.heat;
  int lo = 0, hi = h.n;                                          // row_ptr[lo] <= e < row_ptr[hi]
  for (int step = 0; step < 32 && hi - lo > 1; ++step) {
    const int mid = (lo + hi) >> 1;
    if (row_ptr[mid] <= e)
      lo = mid;
    else
      hi = mid;
  }
  const int e1 = row_ptr[lo + 1], v = col[e];
  unsigned q = heat_q(heat[e]);
  for (int f = e + 1; f < e1; ++f)
    if (col[f] == v) {
      const unsigned x = heat_q(heat[f]);
      q = x > q ? x : q;
    }
  q_all[h.heat + e] = (unsigned short)q;
}

// one thread per entry of the longest array of a group: row_ptr[0] = 0, row_ptr[n] = E, row_ptr rising, 0 <= col < n
__global__ __launch_bounds__(256) void heat_graph_check_kernel(const int* __restrict__ row_ptr, const int* __restrict__ col,
                                                               const MlHeatGroup* __restrict__ groups, int* __restrict__ bad) {
  const MlHeatGroup g = groups[blockIdx.y];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = true;
  if (i <= g.n) {
    const int r = row_ptr[g.rows + i];
    if (i == 0) ok = ok && r == 0;
    if (i == g.n) ok = ok && r == g.edges;
    if (i < g.n) ok = ok && r <= row_ptr[g.rows + i + 1];
    ok = ok && r >= 0 && r <= g.edges;
  }
  if (i < g.edges) {
    const int c = col[g.cols + i];
    ok = ok && c >= 0 && c < g.n;
  }
  if (!ok) *bad = 1;
}

// W_0 .. W_n of the incumbent `inc` (complete: the caller has passed a barrier behind its last write) into W.  Thread r takes the
// positions r ch .. r ch + ch - 1, ch = ceil(n / 1024): it leaves w_k in W[k + 1] and sums them, the 1024 sums are scanned in
// `part` (1024 words of LDS), and the thread turns its w_k into running sums.  Ends behind a barrier: every thread may read W.
__device__ __forceinline__ void heat_prefix(const int* __restrict__ inc, int n, const int* __restrict__ row_ptr,
                                            const int* __restrict__ col, const unsigned short* __restrict__ heat,
                                            unsigned long long* __restrict__ W, unsigned long long* part) {
  const int tid = threadIdx.x, ch = (n + kSelectThreads - 1) / kSelectThreads;
  const int k0 = tid * ch < n ? tid * ch : n, k1 = k0 + ch < n ? k0 + ch : n;      // tid ch < 2^20
  unsigned long long s = 0;
  for (int k = k0; k < k1; ++k) {
    const int u = inc[k], v = inc[k + 1];
    const unsigned a = heat_edge_q(row_ptr, col, heat, u, v), b = heat_edge_q(row_ptr, col, heat, v, u);
    const unsigned long long w = 65536u - (a > b ? a : b);
    W[k + 1] = w;
    s += w;
  }
  part[tid] = s;
  __syncthreads();
  for (int off = 1; off < kSelectThreads; off <<= 1) {
    const unsigned long long add = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  unsigned long long run = part[tid] - s;                                        // the sum of the chunks before this one
  if (tid == 0) W[0] = 0;
  for (int k = k0; k < k1; ++k) {
    run += W[k + 1];
    W[k + 1] = run;
  }
  __syncthreads();
}

// a of a draw: r = (w0 2^32 + w3) mod W_M, p with W_p <= r < W_p+1 (W_0 = 0 <= r < W_M, W rising strictly), a = p + 1
__device__ __forceinline__ int heat_pick(const unsigned long long* __restrict__ W, int M, uint32_t w0, uint32_t w3) {
  const unsigned long long r = (((unsigned long long)w0 << 32) | w3) % W[M];
  int lo = 0, hi = M;
  for (int step = 0; step < 32 && hi - lo > 1; ++step) {                         // W[lo] <= r < W[hi]
    const int mid = (lo + hi) >> 1;
    if (W[mid] <= r)
      lo = mid;
    else
      hi = mid;
  }
  return lo + 1;
}

}  // namespace
}  // namespace difusco
