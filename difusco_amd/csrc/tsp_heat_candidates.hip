// Candidate lists for the neighbour-list TSP searches drawn from the heatmaps (difusco_tsp_heat_candidates_ragged; the rule:
// include/difusco_hip.h, restated in numpy in tests/tsp_heat_candidates_emulation.py).  Every group carries the directed CSR
// candidate graph and the per-tour heat of the guided search; city a lists the K members b of C(a) - the cities its row names and
// the cities whose row names it - that come first by (S(a, b) descending, d2(a, b) ascending, b ascending), S the quantised heat
// of both orientations summed over the group's tours.  Launches, in stream order, with no synchronisation between them but the
// one that brings the flag of the graph check back:
//
//   heat_graph_check_kernel, heat_table_kernel   or_opt_heat.h: the graphs are CSR over their cities; q by (tour, entry), the
//                            first entry of a (row, column) pair holding q_t(row, column);
//   hc_entry_kernel          one thread per entry of a group: sq[e] = the sum over the group's tours of the table entry (so the
//                            first entry of a pair holds the sum of q_t), and the in-degree of col[e] grows by 1;
//   hc_scan_kernel           one block per group: the in-degrees become the row pointers of the transpose (exclusive scan);
//   hc_scatter_kernel        one thread per entry: its row into the transpose row of its column, at a slot an atomic hands out -
//                            the order inside a transpose row is arbitrary, the order of the lists is total and does not see it;
//   hc_select_kernel         one wave per city: lane l owns slots l, l + 64, .. of the city's dout + din gathered entries.  Pass 1
//                            leaves (S, b) of every slot in the workspace, b = -1 for the city itself, a repeated column and an
//                            incoming city the out-row already names; pass 2 runs K rounds of a wave-wide lexicographic maximum
//                            over the slots that are not taken yet.  A lane reads back only what it wrote itself.
//
// All arithmetic is integer but d2 = dx dx + dy dy, float64 with every operation rounded on its own (no contraction).
#include <vector>

#include "common.h"
#include "multi_move_common.h"
#include "or_opt_heat.h"

namespace difusco {
namespace {

constexpr int kMaxCandidates = 128, kWavesPerBlock = 4;

struct HcGroup {           // a group of a call; offsets in elements of the array they index
  int n, edges, tours, pad;
  long long points;        // the group's first coordinate in `points`
  long long rows;          // its first entry in row_ptr and in_ptr (n + 1 per group)
  long long cols;          //                 in col, sq and in_src (E per group); x 2 in slot_s and slot_b
  long long heat;          // its first tour's first entry in heat and q (P E per group)
  long long nodes;         // the cities before the group: x K in neighbors_out; its first entry in fill (n per group)
};

struct HcLayout {
  size_t hgrp, tab, grp, bad, counts, q, sq, in_ptr, fill, in_src, slot_s, slot_b, total;
  size_t rows, nodes, edges;   // the elements the zeroed sections hold: in_ptr (rows), fill (nodes)
  int tours, nmax, emax;
};

struct HcPtrs {
  MlHeatGroup* hgrp;
  MlHeatTour* tab;
  HcGroup* grp;
  int* bad;
  unsigned long long* counts;   // listed, pads per group
  unsigned short* q;
  unsigned* sq;
  int *in_ptr, *fill, *in_src;
  unsigned long long* slot_s;
  int* slot_b;
  HcPtrs(void* workspace, const HcLayout& L) {
    char* p = (char*)workspace;
    hgrp = (MlHeatGroup*)(p + L.hgrp), tab = (MlHeatTour*)(p + L.tab), grp = (HcGroup*)(p + L.grp), bad = (int*)(p + L.bad);
    counts = (unsigned long long*)(p + L.counts), q = (unsigned short*)(p + L.q), sq = (unsigned*)(p + L.sq);
    in_ptr = (int*)(p + L.in_ptr), fill = (int*)(p + L.fill), in_src = (int*)(p + L.in_src);
    slot_s = (unsigned long long*)(p + L.slot_s), slot_b = (int*)(p + L.slot_b);
  }
};

// ---- device

// the row of entry e of a checked CSR over n cities: row_ptr[row] <= e < row_ptr[row + 1]
__device__ __forceinline__ int row_of(const int* __restrict__ row_ptr, int n, int e) {
  int lo = 0, hi = n;
  for (int step = 0; step < 32 && hi - lo > 1; ++step) {
    const int mid = (lo + hi) >> 1;
    if (row_ptr[mid] <= e)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// one thread per entry of a group; grid (ceil(emax / 256), groups)
__global__ __launch_bounds__(256) void hc_entry_kernel(const int* __restrict__ col_all, const HcGroup* __restrict__ grp,
                                                       const unsigned short* __restrict__ q_all, unsigned* __restrict__ sq_all,
                                                       int* __restrict__ in_ptr_all) {
  const HcGroup g = grp[blockIdx.y];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.edges) return;
  const unsigned short* q = q_all + g.heat + i;
  unsigned s = 0;                                                  // at most 65535 tours of at most 65535 each
  for (int t = 0; t < g.tours; ++t) s += q[(long long)t * g.edges];
  sq_all[g.cols + i] = s;
  atomicAdd(&in_ptr_all[g.rows + col_all[g.cols + i]], 1);
}

// one block per group: in_ptr[0 .. n] from the in-degrees in in_ptr[0 .. n-1] (in_ptr[n] holds 0), in place.  A thread sums a
// contiguous chunk, the chunk sums are scanned in LDS.
__global__ __launch_bounds__(kSelectThreads) void hc_scan_kernel(const HcGroup* __restrict__ grp, int* __restrict__ in_ptr_all) {
  __shared__ int part[kSelectThreads];
  const HcGroup g = grp[blockIdx.x];
  int* in_ptr = in_ptr_all + g.rows;
  const int tid = threadIdx.x, cells = g.n + 1, chunk = (cells + kSelectThreads - 1) / kSelectThreads;
  const int lo = tid * chunk < cells ? tid * chunk : cells, hi = lo + chunk < cells ? lo + chunk : cells;
  int mine = 0;
  for (int p = lo; p < hi; ++p) mine += in_ptr[p];
  part[tid] = mine;
  __syncthreads();
  for (int off = 1; off < kSelectThreads; off <<= 1) {
    const int add = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int run = part[tid] - mine;
  for (int p = lo; p < hi; ++p) {
    const int d = in_ptr[p];
    in_ptr[p] = run;
    run += d;
  }
}

// one thread per entry of a group; grid (ceil(emax / 256), groups)
__global__ __launch_bounds__(256) void hc_scatter_kernel(const int* __restrict__ row_ptr_all, const int* __restrict__ col_all,
                                                         const HcGroup* __restrict__ grp, const int* __restrict__ in_ptr_all,
                                                         int* __restrict__ fill_all, int* __restrict__ in_src_all) {
  const HcGroup g = grp[blockIdx.y];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.edges) return;
  const int u = row_of(row_ptr_all + g.rows, g.n, (int)i), v = col_all[g.cols + i];
  const int at = atomicAdd(&fill_all[g.nodes + v], 1);             // at < the in-degree of v
  in_src_all[g.cols + in_ptr_all[g.rows + v] + at] = u;
}

// (S, d2, b) orders before (S', d2', b'); b < 0: no candidate
__device__ __forceinline__ bool lists_before(unsigned long long s, double d, int b, unsigned long long bs, double bd, int bb) {
  if (b < 0) return false;
  if (bb < 0) return true;
  return s > bs || (s == bs && (d < bd || (d == bd && b < bb)));
}

__device__ __forceinline__ double city_d2(const double* __restrict__ P, int a, int b) {
  const double dx = P[2 * a] - P[2 * b], dy = P[2 * a + 1] - P[2 * b + 1];
  return __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
}

// one wave per city; grid (ceil(nmax / kWavesPerBlock), groups)
__global__ __launch_bounds__(64 * kWavesPerBlock) void hc_select_kernel(
    const double* __restrict__ points_all, const int* __restrict__ row_ptr_all, const int* __restrict__ col_all,
    const HcGroup* __restrict__ grp, const unsigned* __restrict__ sq_all, const int* __restrict__ in_ptr_all,
    const int* __restrict__ in_src_all, unsigned long long* __restrict__ slot_s_all, int* __restrict__ slot_b_all, int K,
    int* __restrict__ neighbors_out, unsigned long long* __restrict__ counts) {
  const HcGroup g = grp[blockIdx.y];
  const int lane = threadIdx.x & 63, a = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (a >= g.n) return;                                            // the whole wave
  const double* P = points_all + g.points;
  const int* row_ptr = row_ptr_all + g.rows;
  const int* col = col_all + g.cols;
  const unsigned* sq = sq_all + g.cols;
  const int* in_ptr = in_ptr_all + g.rows;
  const int* in_src = in_src_all + g.cols;
  const int o0 = row_ptr[a], dout = row_ptr[a + 1] - o0, i0 = in_ptr[a], din = in_ptr[a + 1] - i0, total = dout + din;
  unsigned long long* slot_s = slot_s_all + 2 * g.cols + o0 + i0;  // the slots of the cities before: their out- and in-degrees
  int* slot_b = slot_b_all + 2 * g.cols + o0 + i0;

  // pass 1: the slots of this lane
  for (int x = lane; x < total; x += 64) {
    const bool out = x < dout;
    int b = out ? col[o0 + x] : in_src[i0 + x - dout];
    unsigned long long s = 0;
    bool keep = b != a;
    if (out) {
      for (int f = 0; f < x && keep; ++f) keep = col[o0 + f] != b;              // the first entry of the pair holds its sum
      s = sq[o0 + x];
    } else {
      for (int f = 0; f < dout && keep; ++f) keep = col[o0 + f] != b;           // the out-row names it already
      for (int f = dout; f < x && keep; ++f) keep = in_src[i0 + f - dout] != b; // an earlier incoming entry does
    }
    if (keep) {
      const int e1 = row_ptr[b + 1];
      for (int e = row_ptr[b]; e < e1; ++e)
        if (col[e] == a) {
          s += sq[e];
          break;
        }
    }
    slot_s[x] = s;
    slot_b[x] = keep ? b : -1;
  }

  // pass 2: K rounds of the wave's first candidate
  int listed = 0, pads = 0;
  int* out_row = neighbors_out + (g.nodes + a) * (long long)K;
  for (int k = 0; k < K; ++k) {
    unsigned long long bs = 0;
    double bd = 0.0;
    int bb = -1, bx = -1;
    for (int x = lane; x < total; x += 64) {
      const int b = slot_b[x];
      if (b < 0) continue;
      const unsigned long long s = slot_s[x];
      const double d = city_d2(P, a, b);
      if (lists_before(s, d, b, bs, bd, bb)) bs = s, bd = d, bb = b, bx = x;
    }
    unsigned long long ws = bs;
    double wd = bd;
    int wb = bb;
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long os = __shfl_xor(ws, off);
      const double od = __shfl_xor(wd, off);
      const int ob = __shfl_xor(wb, off);
      if (lists_before(os, od, ob, ws, wd, wb)) ws = os, wd = od, wb = ob;
    }
    if (wb >= 0 && wb == bb) slot_b[bx] = -1;                      // kept cities are distinct: one lane owns the winner
    if (lane == 0) out_row[k] = wb;
    if (wb < 0)
      pads += 1;
    else if (ws > 0)
      listed += 1;
  }
  if (lane == 0) {
    if (listed) atomicAdd(&counts[2 * blockIdx.y], (unsigned long long)listed);
    if (pads) atomicAdd(&counts[2 * blockIdx.y + 1], (unsigned long long)pads);
  }
}

// ---- host

// The size conditions of the guided search with one difference: a group needs n >= 1 (no tour is walked here).
int hc_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, const int32_t* group_edges, int K,
              HcLayout* lay, std::vector<HcGroup>* grp, std::vector<MlHeatGroup>* hgrp, std::vector<MlHeatTour>* tab) {
  *lay = HcLayout{};
  if (groups < 1) return set_error(DIFUSCO_EINVAL, "%s: groups = %d, needs at least 1", who, groups);
  if (!group_n || !group_tours || !group_edges) return set_error(DIFUSCO_EINVAL, "%s: group_n / group_tours / group_edges is null", who);
  if (K < 1 || K > kMaxCandidates) return set_error(DIFUSCO_EINVAL, "%s: K = %d, needs 1 .. %d", who, K, kMaxCandidates);
  size_t points = 0, rows = 0, cols = 0, heat = 0, nodes = 0;
  long long T = 0;
  for (int g = 0; g < groups; ++g) {
    const int n = group_n[g], P = group_tours[g], E = group_edges[g];
    if (n < 1) return set_error(DIFUSCO_EINVAL, "%s: group %d has n = %d, needs n >= 1", who, g, n);
    if (n > kMaxNodes) return set_error(DIFUSCO_EINVAL, "%s: group %d has n = %d, at most %d nodes", who, g, n, kMaxNodes);
    if (P < 1) return set_error(DIFUSCO_EINVAL, "%s: group %d has %d tours, needs at least 1", who, g, P);
    if (E < 0) return set_error(DIFUSCO_EINVAL, "%s: group %d has %d edges", who, g, E);
    T += P;
    if (T > kMaxTours) return set_error(DIFUSCO_EINVAL, "%s: more than %d tours in one call", who, kMaxTours);
    if (n > lay->nmax) lay->nmax = n;
    if (E > lay->emax) lay->emax = E;
    if (hgrp) hgrp->push_back(MlHeatGroup{n, E, (long long)rows, (long long)cols});
    if (grp) grp->push_back(HcGroup{n, E, P, 0, (long long)points, (long long)rows, (long long)cols, (long long)heat, (long long)nodes});
    for (int p = 0; p < P; ++p) {
      if (tab) tab->push_back(MlHeatTour{(long long)rows, (long long)cols, (long long)heat, n, E});
      heat += (size_t)E;
    }
    points += 2 * (size_t)n, rows += (size_t)n + 1, cols += (size_t)E, nodes += (size_t)n;
  }
  lay->tours = (int)T, lay->rows = rows, lay->nodes = nodes, lay->edges = cols;
  Sections sec;
  lay->hgrp = sec.take(sizeof(MlHeatGroup) * (size_t)groups), lay->tab = sec.take(sizeof(MlHeatTour) * (size_t)T);
  lay->grp = sec.take(sizeof(HcGroup) * (size_t)groups), lay->bad = sec.take(sizeof(int));
  lay->counts = sec.take(sizeof(unsigned long long) * 2 * (size_t)groups);
  lay->q = sec.take(sizeof(unsigned short) * heat), lay->sq = sec.take(sizeof(unsigned) * cols);
  lay->in_ptr = sec.take(sizeof(int) * rows), lay->fill = sec.take(sizeof(int) * nodes), lay->in_src = sec.take(sizeof(int) * cols);
  lay->slot_s = sec.take(sizeof(unsigned long long) * 2 * cols), lay->slot_b = sec.take(sizeof(int) * 2 * cols);
  lay->total = sec.off;
  return DIFUSCO_OK;
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_heat_candidates_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours,
                                                       const int32_t* group_edges, int32_t K, size_t* bytes) {
  using namespace difusco;
  const char* who = "tsp_heat_candidates_ragged_workspace_bytes";
  if (!bytes) return set_error(DIFUSCO_EINVAL, "%s: bytes is null", who);
  HcLayout lay;
  const int rc = hc_layout(who, groups, group_n, group_tours, group_edges, K, &lay, nullptr, nullptr, nullptr);
  if (rc != DIFUSCO_OK) return rc;
  *bytes = lay.total;
  return DIFUSCO_OK;
}

int difusco_tsp_heat_candidates_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const int32_t* group_edges,
                                       const double* points, const int32_t* row_ptr, const int32_t* col, const float* heat,
                                       int32_t K, int32_t* neighbors_out, void* workspace, size_t workspace_bytes,
                                       int64_t* listed_out, int64_t* pads_out, void* stream) {
  using namespace difusco;
  const char* who = "tsp_heat_candidates_ragged";
  HcLayout lay;
  std::vector<HcGroup> grp;
  std::vector<MlHeatGroup> hgrp;
  std::vector<MlHeatTour> tab;
  const int rc = hc_layout(who, groups, group_n, group_tours, group_edges, K, &lay, &grp, &hgrp, &tab);
  if (rc != DIFUSCO_OK) return rc;
  if (!points || !row_ptr || !col || !heat || !neighbors_out || !workspace)
    return set_error(DIFUSCO_EINVAL, "%s: needs the device arrays points / row_ptr / col / heat / neighbors_out and a workspace", who);
  if (!listed_out || !pads_out) return set_error(DIFUSCO_EINVAL, "%s: needs the two host output arrays [groups]", who);
  if (workspace_bytes < lay.total) return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", who, workspace_bytes, lay.total);

  const HcPtrs p(workspace, lay);
  hipStream_t s = (hipStream_t)stream;
  const int T = lay.tours;
  int bad = 0;
  hipError_t er = hipMemcpyAsync(p.hgrp, hgrp.data(), sizeof(MlHeatGroup) * groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemcpyAsync(p.tab, tab.data(), sizeof(MlHeatTour) * T, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemcpyAsync(p.grp, grp.data(), sizeof(HcGroup) * groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(p.bad, 0, sizeof(int), s);
  if (er == hipSuccess) er = hipMemsetAsync(p.counts, 0, sizeof(unsigned long long) * 2 * groups, s);
  if (er == hipSuccess) er = hipMemsetAsync(p.in_ptr, 0, sizeof(int) * lay.rows, s);
  if (er == hipSuccess) er = hipMemsetAsync(p.fill, 0, sizeof(int) * lay.nodes, s);
  if (er == hipSuccess) {                                          // the check of the graphs, in front of everything that walks them
    const long long longest = (long long)lay.nmax + 1 > lay.emax ? (long long)lay.nmax + 1 : lay.emax;
    hipLaunchKernelGGL(heat_graph_check_kernel, dim3((unsigned)((longest + 255) / 256), groups), dim3(256), 0, s, row_ptr, col, p.hgrp,
                       p.bad);
    er = hipMemcpyAsync(&bad, p.bad, sizeof(int), hipMemcpyDeviceToHost, s);
  }
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s setup: %s", who, hipGetErrorString(er));
  if (bad)
    return set_error(DIFUSCO_EINVAL, "%s: a group's graph is not a CSR over its cities (row_ptr[0] = 0, row_ptr rising to "
                                     "row_ptr[n] = edges, 0 <= col < n)", who);
  if (lay.emax > 0) {
    const dim3 per_entry((unsigned)(((long long)lay.emax + 255) / 256), groups);
    hipLaunchKernelGGL(heat_table_kernel, dim3(per_entry.x, T), dim3(256), 0, s, row_ptr, col, heat, p.tab, p.q);
    hipLaunchKernelGGL(hc_entry_kernel, per_entry, dim3(256), 0, s, col, p.grp, p.q, p.sq, p.in_ptr);
    hipLaunchKernelGGL(hc_scan_kernel, dim3(groups), dim3(kSelectThreads), 0, s, p.grp, p.in_ptr);
    hipLaunchKernelGGL(hc_scatter_kernel, per_entry, dim3(256), 0, s, row_ptr, col, p.grp, p.in_ptr, p.fill, p.in_src);
  }
  hipLaunchKernelGGL(hc_select_kernel, dim3((lay.nmax + kWavesPerBlock - 1) / kWavesPerBlock, groups), dim3(64 * kWavesPerBlock), 0, s,
                     points, row_ptr, col, p.grp, p.sq, p.in_ptr, p.in_src, p.slot_s, p.slot_b, (int)K, neighbors_out, p.counts);
  std::vector<unsigned long long> counts(2 * (size_t)groups);
  er = hipMemcpyAsync(counts.data(), p.counts, sizeof(unsigned long long) * counts.size(), hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er == hipSuccess) er = hipGetLastError();
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s: %s", who, hipGetErrorString(er));
  for (int g = 0; g < groups; ++g) listed_out[g] = (int64_t)counts[2 * g], pads_out[g] = (int64_t)counts[2 * g + 1];
  return DIFUSCO_OK;
}

}  // extern "C"
