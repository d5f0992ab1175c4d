// Graph preparation on the device: COO edge_index -> CSR over the centre node, with the optional Morton renumbering of the
// nodes - bit for bit the arrays of difusco_amd/graph.py `build_csr` (difusco_csr_from_coo_host + locality_node_order).
//
// Passes (all on the caller's stream; rocPRIM for the scans and the two stable radix sorts):
//   1. gb_init_kernel        flags, the bounding box and the per-node spans (S: own id on both halves)
//   2. gb_edge_check_kernel  range check of every edge (smallest bad edge id by atomicMin), and
//                            points: the span of every node - integer atomicMax on the two halves of S[centre];
//                            no points: the sort keys of pass 7 (inv is the identity)
//   3. gb_bbox_kernel        bounding box of the points in float64 (order-preserving integer atomics: exact, any order)
//   4. inclusive scan of S   both running extrema in one scan: high half max-scan of hi (= reach), low half max-scan
//                            of n-1-lo over the REVERSED node order (= n-1-back, reversed)
//   5. inclusive sum scan    of the cuts (computed on the fly from the scanned spans) = the block id of every node
//   6. gb_node_key_kernel    key = (block << 32) | morton, value = node id; stable radix sort on the bits in use;
//      gb_order_kernel       node_order, inv[order[i]] = i, "order is the identity" flag
//   7. gb_edge_key_kernel    key = inv[centre], value = edge id; stable radix sort on the bits n_nodes needs,
//                            written straight into row / perm
//   8. gb_finish_kernel      col = inv[col[perm]], "perm is the identity" flag, rowptr by a lower-bound search per
//                            node, and the endpoints of the first bad edge for the error text
// then ONE device-to-host copy (the 32-byte flag block) and a stream synchronise.
// An edge that failed the range check is never used as an index: passes 7 and 8 test again and substitute node 0 (the
// outputs are unspecified in that case; the call returns DIFUSCO_EINVAL).
// Compiled with -ffp-contract=off: the Morton arithmetic is numpy's float64 program (no multiply-add exists in it anyway).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/difusco_hip.h"
#include "kernels.h"

namespace difusco {
namespace {

constexpr unsigned GB_NO_BAD_EDGE = 0xFFFFFFFFu;
constexpr int GB_BLOCK = 256;
constexpr long long GB_MAX_BLOCKS = 4096;      // memory-bound passes: capped grid, grid-stride loops

struct GbFlags {                // device copy of what the host reads back (32 bytes)
  unsigned perm_differs;        // 1: perm is not the identity
  unsigned order_differs;       // 1: node_order is not the identity
  unsigned bad_edge;            // smallest edge id with an endpoint outside [0, n_nodes); GB_NO_BAD_EDGE: none
  unsigned pad;
  long long bad_row, bad_col;   // its endpoints
};

struct GbBox {                  // bounding box as order-preserving unsigned images of the float64 coordinates
  unsigned long long mn[2], mx[2];
};

__device__ __forceinline__ unsigned long long gb_ordered(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double gb_unordered(unsigned long long u) {
  const unsigned long long b = (u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u;
  return __longlong_as_double((long long)b);
}

__device__ __forceinline__ double gb_point(const void* points, int f64, long long i) {
  return f64 ? ((const double*)points)[i] : (double)((const float*)points)[i];
}

__device__ __forceinline__ bool gb_in_range(long long v, long long n) { return v >= 0 && v < n; }

// S[k]: high half = hi of node k, low half = n-1-lo of node n-1-k (little endian: word 2k is the low half)
__global__ __launch_bounds__(GB_BLOCK) void gb_init_kernel(long long n, int with_points, GbFlags* flags, GbBox* box,
                                                           unsigned long long* __restrict__ S) {
  const long long t0 = (long long)blockIdx.x * GB_BLOCK + threadIdx.x, stride = (long long)gridDim.x * GB_BLOCK;
  if (t0 == 0) {
    flags->perm_differs = 0;
    flags->order_differs = 0;
    flags->bad_edge = GB_NO_BAD_EDGE;
    flags->pad = 0;
    flags->bad_row = 0;
    flags->bad_col = 0;
    box->mn[0] = box->mn[1] = ~0ull;
    box->mx[0] = box->mx[1] = 0ull;
  }
  if (!with_points) return;
  for (long long k = t0; k < n; k += stride) S[k] = ((unsigned long long)k << 32) | (unsigned long long)k;
}

template <bool WITH_POINTS>
__global__ __launch_bounds__(GB_BLOCK) void gb_edge_check_kernel(long long n, long long E, const long long* __restrict__ ei,
                                                                 GbFlags* flags, unsigned* __restrict__ S32,
                                                                 unsigned* __restrict__ ekey, unsigned* __restrict__ eid) {
  const long long t0 = (long long)blockIdx.x * GB_BLOCK + threadIdx.x, stride = (long long)gridDim.x * GB_BLOCK;
  unsigned bad = GB_NO_BAD_EDGE;
  for (long long k = t0; k < E; k += stride) {
    const long long r = ei[k], c = ei[E + k];
    const bool ok = gb_in_range(r, n) && gb_in_range(c, n);
    if (!ok && bad == GB_NO_BAD_EDGE) bad = (unsigned)k;      // k grows along the loop: the first one is this thread's smallest
    if (WITH_POINTS) {
      if (ok) {
        // both halves only ever grow, so a stale plain read can only let a needless atomic through, never drop a needed one
        unsigned* hi = S32 + 2 * r + 1;
        unsigned* rlo = S32 + 2 * (n - 1 - r);
        const unsigned c_hi = (unsigned)c, c_rlo = (unsigned)(n - 1 - c);
        if (c_hi > __builtin_nontemporal_load(hi)) atomicMax(hi, c_hi);
        if (c_rlo > __builtin_nontemporal_load(rlo)) atomicMax(rlo, c_rlo);
      }
    } else {
      ekey[k] = ok ? (unsigned)r : 0u;
      eid[k] = (unsigned)k;
    }
  }
  if (bad != GB_NO_BAD_EDGE) atomicMin(&flags->bad_edge, bad);
}

__global__ __launch_bounds__(GB_BLOCK) void gb_bbox_kernel(long long n, const void* __restrict__ points, int f64, GbBox* box) {
  __shared__ unsigned long long sh[4][GB_BLOCK / 64];
  const long long t0 = (long long)blockIdx.x * GB_BLOCK + threadIdx.x, stride = (long long)gridDim.x * GB_BLOCK;
  unsigned long long mn0 = ~0ull, mn1 = ~0ull, mx0 = 0ull, mx1 = 0ull;
  for (long long i = t0; i < n; i += stride) {
    const unsigned long long x = gb_ordered(gb_point(points, f64, 2 * i)), y = gb_ordered(gb_point(points, f64, 2 * i + 1));
    mn0 = x < mn0 ? x : mn0;
    mx0 = x > mx0 ? x : mx0;
    mn1 = y < mn1 ? y : mn1;
    mx1 = y > mx1 ? y : mx1;
  }
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long o;
    o = __shfl_xor(mn0, off); mn0 = o < mn0 ? o : mn0;
    o = __shfl_xor(mx0, off); mx0 = o > mx0 ? o : mx0;
    o = __shfl_xor(mn1, off); mn1 = o < mn1 ? o : mn1;
    o = __shfl_xor(mx1, off); mx1 = o > mx1 ? o : mx1;
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[0][wave] = mn0; sh[1][wave] = mx0; sh[2][wave] = mn1; sh[3][wave] = mx1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < GB_BLOCK / 64; ++w) {
      mn0 = sh[0][w] < mn0 ? sh[0][w] : mn0;
      mx0 = sh[1][w] > mx0 ? sh[1][w] : mx0;
      mn1 = sh[2][w] < mn1 ? sh[2][w] : mn1;
      mx1 = sh[3][w] > mx1 ? sh[3][w] : mx1;
    }
    atomicMin(&box->mn[0], mn0);
    atomicMax(&box->mx[0], mx0);
    atomicMin(&box->mn[1], mn1);
    atomicMax(&box->mx[1], mx1);
  }
}

// the scan operator of pass 4: max on each 32-bit half
struct GbMaxHalves {
  __host__ __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const {
    const unsigned long long ah = a >> 32, bh = b >> 32, al = a & 0xFFFFFFFFull, bl = b & 0xFFFFFFFFull;
    return ((ah > bh ? ah : bh) << 32) | (al > bl ? al : bl);
  }
};

// cut[b] = 1: a block starts at node b (graph.py _id_blocks), from the scanned spans T
struct GbCut {
  const unsigned long long* T;
  long long n;
  __host__ __device__ unsigned operator()(long long b) const {
    if (b == 0) return 0u;
    const long long reach_prev = (long long)(T[b - 1] >> 32);
    const long long back = n - 1 - (long long)(T[n - 1 - b] & 0xFFFFFFFFull);
    return (reach_prev < b && back >= b) ? 1u : 0u;
  }
};

__device__ __forceinline__ unsigned long long gb_spread(unsigned long long v) {
  v = (v | (v << 8)) & 0x00FF00FFull;
  v = (v | (v << 4)) & 0x0F0F0F0Full;
  v = (v | (v << 2)) & 0x33333333ull;
  return (v | (v << 1)) & 0x55555555ull;
}

// graph.py _morton_keys, one axis: clip((p - mn) / max(mx - mn, 1e-30) * 65535.0, 0, 65535) truncated
__device__ __forceinline__ unsigned long long gb_quantise(double p, double mn, double mx) {
  const double span = fmax(mx - mn, 1e-30);
  double q = (p - mn) / span * 65535.0;
  q = fmin(fmax(q, 0.0), 65535.0);
  return (unsigned long long)q;
}

__global__ __launch_bounds__(GB_BLOCK) void gb_node_key_kernel(long long n, const void* __restrict__ points, int f64,
                                                               const GbBox* __restrict__ box, const unsigned* __restrict__ block,
                                                               unsigned long long* __restrict__ key, unsigned* __restrict__ id) {
  const long long t0 = (long long)blockIdx.x * GB_BLOCK + threadIdx.x, stride = (long long)gridDim.x * GB_BLOCK;
  const double mn0 = gb_unordered(box->mn[0]), mx0 = gb_unordered(box->mx[0]);
  const double mn1 = gb_unordered(box->mn[1]), mx1 = gb_unordered(box->mx[1]);
  for (long long i = t0; i < n; i += stride) {
    const unsigned long long qx = gb_quantise(gb_point(points, f64, 2 * i), mn0, mx0);
    const unsigned long long qy = gb_quantise(gb_point(points, f64, 2 * i + 1), mn1, mx1);
    key[i] = ((unsigned long long)block[i] << 32) | gb_spread(qx) | (gb_spread(qy) << 1);
    id[i] = (unsigned)i;
  }
}

__global__ __launch_bounds__(GB_BLOCK) void gb_order_kernel(long long n, const unsigned* __restrict__ order,
                                                            long long* __restrict__ node_order, unsigned* __restrict__ inv,
                                                            GbFlags* flags) {
  const long long t0 = (long long)blockIdx.x * GB_BLOCK + threadIdx.x, stride = (long long)gridDim.x * GB_BLOCK;
  bool differs = false;
  for (long long i = t0; i < n; i += stride) {
    const unsigned o = order[i];      // a permutation of 0..n-1 (the sorted values)
    node_order[i] = (long long)o;
    inv[o] = (unsigned)i;
    differs |= o != (unsigned)i;
  }
  if (__any(differs) && (threadIdx.x & 63) == 0) flags->order_differs = 1u;      // same value from every writer
}

__global__ __launch_bounds__(GB_BLOCK) void gb_edge_key_kernel(long long n, long long E, const long long* __restrict__ ei,
                                                               const unsigned* __restrict__ inv, unsigned* __restrict__ ekey,
                                                               unsigned* __restrict__ eid) {
  const long long t0 = (long long)blockIdx.x * GB_BLOCK + threadIdx.x, stride = (long long)gridDim.x * GB_BLOCK;
  for (long long k = t0; k < E; k += stride) {
    const long long r = ei[k], c = ei[E + k];
    ekey[k] = (gb_in_range(r, n) && gb_in_range(c, n)) ? inv[r] : 0u;
    eid[k] = (unsigned)k;
  }
}

// threads 0..E-1: one CSR slot each; threads 0..n: one rowptr entry each (first slot whose centre is >= v)
__global__ __launch_bounds__(GB_BLOCK) void gb_finish_kernel(long long n, long long E, const long long* __restrict__ ei,
                                                             const unsigned* __restrict__ inv, const int* __restrict__ row,
                                                             const int* __restrict__ perm, int* __restrict__ col,
                                                             int* __restrict__ rowptr, GbFlags* flags) {
  const long long t0 = (long long)blockIdx.x * GB_BLOCK + threadIdx.x, stride = (long long)gridDim.x * GB_BLOCK;
  if (t0 == 0) {
    const unsigned b = flags->bad_edge;      // final since pass 2
    if (b != GB_NO_BAD_EDGE) {
      flags->bad_row = ei[b];
      flags->bad_col = ei[E + b];
    }
  }
  bool differs = false;
  for (long long s = t0; s < E; s += stride) {
    const long long k = perm[s];             // a permutation of 0..E-1 (the sorted values)
    const long long c = ei[E + k];
    const unsigned cc = gb_in_range(c, n) ? (unsigned)c : 0u;
    col[s] = (int)(inv ? inv[cc] : cc);
    differs |= k != s;
  }
  if (__any(differs) && (threadIdx.x & 63) == 0) flags->perm_differs = 1u;
  for (long long v = t0; v <= n; v += stride) {
    long long lo = 0, hi = E;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if ((long long)row[mid] < v) lo = mid + 1;
      else hi = mid;
    }
    rowptr[v] = (int)lo;
  }
}

size_t gb_up256(size_t x) { return (x + 255) / 256 * 256; }

int gb_bits(long long values) {      // bits that hold every value of 0..values-1 (at least 1)
  int b = 1;
  while (b < 63 && (1ll << b) < values) ++b;
  return b;
}

unsigned gb_grid(long long work) {
  long long g = (work + GB_BLOCK - 1) / GB_BLOCK;
  return (unsigned)(g < 1 ? 1 : (g > GB_MAX_BLOCKS ? GB_MAX_BLOCKS : g));
}

// the rocPRIM calls, each usable as its own temporary-storage query (temp == nullptr)
hipError_t gb_scan_spans(void* temp, size_t& bytes, unsigned long long* S, unsigned long long* T, long long n, hipStream_t st) {
  return rocprim::inclusive_scan(temp, bytes, S, T, (size_t)n, GbMaxHalves(), st, false);
}
hipError_t gb_scan_cuts(void* temp, size_t& bytes, const unsigned long long* T, unsigned* block, long long n, hipStream_t st) {
  auto cuts = rocprim::make_transform_iterator(rocprim::make_counting_iterator<long long>(0), GbCut{T, n});
  return rocprim::inclusive_scan(temp, bytes, cuts, block, (size_t)n, rocprim::plus<unsigned>(), st, false);
}
hipError_t gb_sort_nodes(void* temp, size_t& bytes, unsigned long long* key_in, unsigned long long* key_out, unsigned* id_in,
                         unsigned* id_out, long long n, hipStream_t st) {
  return rocprim::radix_sort_pairs(temp, bytes, key_in, key_out, id_in, id_out, (size_t)n, 0u, (unsigned)(32 + gb_bits(n)), st,
                                   false);
}
hipError_t gb_sort_edges(void* temp, size_t& bytes, unsigned* key_in, unsigned* key_out, unsigned* id_in, unsigned* id_out,
                         long long n, long long E, hipStream_t st) {
  return rocprim::radix_sort_pairs(temp, bytes, key_in, key_out, id_in, id_out, (size_t)E, 0u, (unsigned)gb_bits(n), st, false);
}

struct GbCarve {
  GbFlags* flags;
  GbBox* box;
  unsigned long long *S, *T, *nkey_a, *nkey_b;
  unsigned *block, *nid_a, *nid_b, *inv, *ekey, *eid;
  void* temp;
  size_t temp_bytes, total;
};

// the largest temporary storage any rocPRIM call of a build asks for (the query reads the device's properties)
hipError_t gb_temp_bytes(long long n, long long E, bool with_points, size_t* bytes) {
  size_t t = 0, need = 0;
  hipError_t er = gb_sort_edges(nullptr, t, nullptr, nullptr, nullptr, nullptr, n, E, 0);
  if (er != hipSuccess) return er;
  need = t;
  if (with_points) {
    er = gb_scan_spans(nullptr, t, nullptr, nullptr, n, 0);
    if (er != hipSuccess) return er;
    need = t > need ? t : need;
    er = gb_scan_cuts(nullptr, t, nullptr, nullptr, n, 0);
    if (er != hipSuccess) return er;
    need = t > need ? t : need;
    er = gb_sort_nodes(nullptr, t, nullptr, nullptr, nullptr, nullptr, n, 0);
    if (er != hipSuccess) return er;
    need = t > need ? t : need;
  }
  *bytes = need;
  return hipSuccess;
}

// need: the rocPRIM temporary storage (gb_temp_bytes); 0 gives the size of the library's own arrays alone
void gb_carve(void* base, long long n, long long E, bool with_points, size_t need, GbCarve* c) {
  c->temp_bytes = need;
  size_t cur = 0;
  auto take = [&](size_t bytes) {
    size_t at = cur;
    cur += gb_up256(bytes);
    return base ? (void*)((char*)base + at) : (void*)nullptr;
  };
  const size_t nn = with_points ? (size_t)n : 0;
  c->flags = (GbFlags*)take(sizeof(GbFlags));
  c->box = (GbBox*)take(sizeof(GbBox));
  c->S = (unsigned long long*)take(8 * nn);
  c->T = (unsigned long long*)take(8 * nn);
  c->nkey_a = (unsigned long long*)take(8 * nn);
  c->nkey_b = (unsigned long long*)take(8 * nn);
  c->block = (unsigned*)take(4 * nn);
  c->nid_a = (unsigned*)take(4 * nn);
  c->nid_b = (unsigned*)take(4 * nn);
  c->inv = (unsigned*)take(4 * nn);
  c->ekey = (unsigned*)take(4 * (size_t)E);
  c->eid = (unsigned*)take(4 * (size_t)E);
  c->temp = take(need);
  c->total = cur;
}

int gb_sizes_ok(int64_t n_nodes, int64_t n_edges) {
  return !(n_edges < 0 || n_nodes < 0 || n_edges > INT32_MAX || n_nodes >= INT32_MAX);
}

// the host skips the renumbering without points, with one node or none, and without edges (graph.py build_csr)
bool gb_renumbers(int64_t n_nodes, int64_t n_edges, int with_points) { return with_points && n_nodes > 1 && n_edges > 0; }

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_graph_build_workspace_bytes(int64_t n_nodes, int64_t n_edges, int with_points, size_t* bytes) {
  using namespace difusco;
  if (!bytes) return set_error(DIFUSCO_EINVAL, "graph_build_workspace_bytes: null pointer");
  if (!gb_sizes_ok(n_nodes, n_edges))
    return set_error(DIFUSCO_EINVAL, "graph_build_workspace_bytes: sizes out of int32 range (n_nodes %lld, n_edges %lld)",
                     (long long)n_nodes, (long long)n_edges);
  const bool renumber = gb_renumbers(n_nodes, n_edges, with_points);
  size_t temp = 0;
  hipError_t er = gb_temp_bytes(n_nodes, n_edges, renumber, &temp);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  GbCarve c;
  gb_carve(nullptr, n_nodes, n_edges, renumber, temp, &c);
  *bytes = c.total;
  return DIFUSCO_OK;
}

int difusco_graph_build(int64_t n_nodes, int64_t n_edges, const int64_t* edge_index, const void* points, int points_f64,
                        int32_t* rowptr, int32_t* col, int32_t* row, int32_t* perm, int64_t* node_order, uint32_t* flags_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
  using namespace difusco;
  if (!gb_sizes_ok(n_nodes, n_edges))
    return set_error(DIFUSCO_EINVAL, "graph_build: sizes out of int32 range (n_nodes %lld, n_edges %lld)", (long long)n_nodes,
                     (long long)n_edges);
  if (!rowptr || !flags_out || !workspace) return set_error(DIFUSCO_EINVAL, "graph_build: null pointer (rowptr, flags_out, workspace)");
  if (n_edges > 0 && (!edge_index || !col || !row || !perm))
    return set_error(DIFUSCO_EINVAL, "graph_build: null pointer (edge_index, col, row, perm)");
  const bool with_points = gb_renumbers(n_nodes, n_edges, points != nullptr);
  if (with_points && !node_order) return set_error(DIFUSCO_EINVAL, "graph_build: null pointer (node_order, with points)");
  if (points_f64 != 0 && points_f64 != 1) return set_error(DIFUSCO_EINVAL, "graph_build: points_f64 must be 0 or 1");
  GbCarve c;
  gb_carve(workspace, n_nodes, n_edges, with_points, 0, &c);      // the library's own arrays: known without asking the device
  if (workspace_bytes < c.total)
    return set_error(DIFUSCO_EINVAL, "graph_build: workspace %zu < %zu bytes before the sort storage", workspace_bytes, c.total);
  size_t temp = 0;
  hipError_t er = gb_temp_bytes(n_nodes, n_edges, with_points, &temp);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "rocprim temp size: %s", hipGetErrorString(er));
  gb_carve(workspace, n_nodes, n_edges, with_points, temp, &c);
  if (workspace_bytes < c.total)
    return set_error(DIFUSCO_EINVAL, "graph_build: workspace %zu < %zu bytes", workspace_bytes, c.total);

  hipStream_t st = (hipStream_t)stream;
  const long long n = n_nodes, E = n_edges;
  const long long* ei = (const long long*)edge_index;
  hipLaunchKernelGGL(gb_init_kernel, dim3(gb_grid(with_points ? n : 1)), dim3(GB_BLOCK), 0, st, n, (int)with_points, c.flags,
                     c.box, c.S);
  size_t tb;
  if (E > 0) {
    if (with_points) {
      hipLaunchKernelGGL(gb_edge_check_kernel<true>, dim3(gb_grid(E)), dim3(GB_BLOCK), 0, st, n, E, ei, c.flags, (unsigned*)c.S,
                         c.ekey, c.eid);
      hipLaunchKernelGGL(gb_bbox_kernel, dim3(gb_grid(n)), dim3(GB_BLOCK), 0, st, n, points, points_f64, c.box);
      tb = c.temp_bytes;
      er = gb_scan_spans(c.temp, tb, c.S, c.T, n, st);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "graph_build span scan: %s", hipGetErrorString(er));
      tb = c.temp_bytes;
      er = gb_scan_cuts(c.temp, tb, c.T, c.block, n, st);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "graph_build block scan: %s", hipGetErrorString(er));
      hipLaunchKernelGGL(gb_node_key_kernel, dim3(gb_grid(n)), dim3(GB_BLOCK), 0, st, n, points, points_f64, c.box, c.block,
                         c.nkey_a, c.nid_a);
      tb = c.temp_bytes;
      er = gb_sort_nodes(c.temp, tb, c.nkey_a, c.nkey_b, c.nid_a, c.nid_b, n, st);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "graph_build node sort: %s", hipGetErrorString(er));
      hipLaunchKernelGGL(gb_order_kernel, dim3(gb_grid(n)), dim3(GB_BLOCK), 0, st, n, c.nid_b, (long long*)node_order, c.inv,
                         c.flags);
      hipLaunchKernelGGL(gb_edge_key_kernel, dim3(gb_grid(E)), dim3(GB_BLOCK), 0, st, n, E, ei, c.inv, c.ekey, c.eid);
    } else {
      hipLaunchKernelGGL(gb_edge_check_kernel<false>, dim3(gb_grid(E)), dim3(GB_BLOCK), 0, st, n, E, ei, c.flags,
                         (unsigned*)nullptr, c.ekey, c.eid);
    }
    tb = c.temp_bytes;
    er = gb_sort_edges(c.temp, tb, c.ekey, (unsigned*)row, c.eid, (unsigned*)perm, n, E, st);
    if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "graph_build edge sort: %s", hipGetErrorString(er));
  }
  const long long work = E > n + 1 ? E : n + 1;
  hipLaunchKernelGGL(gb_finish_kernel, dim3(gb_grid(work)), dim3(GB_BLOCK), 0, st, n, E, ei, with_points ? c.inv : (unsigned*)nullptr,
                     row, perm, col, rowptr, c.flags);
  GbFlags host;
  er = hipMemcpyAsync(&host, c.flags, sizeof(GbFlags), hipMemcpyDeviceToHost, st);
  if (er == hipSuccess) er = hipStreamSynchronize(st);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "graph_build: %s", hipGetErrorString(er));
  const bool bad = host.bad_edge != GB_NO_BAD_EDGE;
  flags_out[0] = (host.perm_differs ? 0u : DIFUSCO_GRAPH_PERM_IDENTITY) | ((with_points && host.order_differs) ? 0u : DIFUSCO_GRAPH_ORDER_IDENTITY) |
                 (bad ? DIFUSCO_GRAPH_BAD_EDGE : 0u);
  flags_out[1] = bad ? host.bad_edge : 0u;
  if (bad)
    return set_error(DIFUSCO_EINVAL, "edge %lld = (%lld,%lld) out of range [0,%lld)", (long long)host.bad_edge, host.bad_row,
                     host.bad_col, n);
  return DIFUSCO_OK;
}

}  // extern "C"
