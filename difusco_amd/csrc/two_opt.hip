// Batched 2-opt refinement of decoded tours (difusco/utils/tsp_utils.py:12-49 `batched_two_opt_torch`), SURVEY 8(f)-2.
//
// The reference materialises four N x N float64 distance matrices per iteration (A_ij, A_i+1,j+1, A_i,i+1, A_j,j+1),
// takes triu(diagonal=2) of their combination, and an argmin per tour; up to 1000-5000 iterations.  Here one
// iteration is three small launches with nothing N x N in memory:
//   two_opt_prep_kernel   P[k] = points[tour[k]] (tour order) and d[k] = |P[k] - P[k+1]|;
//   two_opt_best_kernel   every thread keeps P[j], P[j+1], d[j] of its columns in registers, a block sweeps a tile of
//                         rows i, change = ((A_ij + A_i+1,j+1) - d_i) - d_j in float64 in the reference's operation
//                         order, running (min, first flat index) per thread -> block -> partial[];
//   two_opt_apply_kernel  one block per group: argmin per tour over the partials (ties: lowest flat index = first occurrence,
//                         what torch.argmin returns on the flattened matrix); min over the group's tours decides (tsp_utils.py:
//                         33,39: one global `min_change < -1e-6` test, every tour applies its own best move);
//                         the segment tour[i+1 .. j] is reversed in place, the group's iteration counter advances.
// Invalid entries (j < i + 2) are zeros in the reference's matrix, so the minimum is never positive and the argmin of
// an all-non-improving matrix is flat index 0 = a no-op reversal: the running best starts at (0.0, 0).
// The host only polls the count of stopped groups every few iterations; a stopped group's launches return immediately.
// Every entry is one call of two_opt_run on groups of tours: one batch (difusco_tsp_two_opt: one group), groups of one n
// (_grouped) and groups of different n (_ragged).  The kernels are templates over where a block finds its tour's n, array bases
// and stop flag (UniformAddr, TableAddr); the per-block code is screen_tile, screened_best_tile here and best_tile, tour_argmin,
// apply_move in two_opt_common.h, which the local search of or_opt.hip uses as well.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

// ---- addressing: where a block finds its tour -----------------------------------------------------------------------------------
//
// Groups of different n (difusco_tsp_two_opt_ragged) run the launch sequence of the equal-size entries with every kernel reading
// its tour's n and array bases from a descriptor table instead of computing them from one n.  The table is built on the host from
// group_n / group_tours and written to the workspace once per call.  A block reads desc[its tour], an index that is uniform over
// the block, so the descriptor and every base derived from it stay in scalar registers and the row data of the screen still
// arrive by scalar loads.
// Grids: the call's maxima (nblk_max, [nchunk_max,] tours); a block beyond its own tour's nblk / nchunk returns at once.  With
// equal sizes the grids are exactly those of the grouped entries.  A flat work list with a search over a prefix array would
// launch no idle block, but every block would pay the search and equal sizes would no longer map to the grouped grid; an idle
// block costs a descriptor load and an exit.
struct RaggedTour {        // 64 bytes; offsets in elements of the array they index
  int group, n, nblk, nchunk;
  long long points;        // the group's first coordinate in `points` (doubles)
  long long tours;         // the tour's first entry in `tours` (n + 1 per tour)
  long long tp;            //                       in tp (n + 1 per tour)
  long long cols;          //                       in dlen, q and d32 (n per tour each: one offset serves the three)
  long long partial;       //                       in partial (nblk per tour)
  long long bmin;          //                       in bmin (nblk * nchunk per tour)
};

struct RaggedGroup {       // what the apply block and the max |coordinate| reduction of a group need
  int first, count;        // its tours: first .. first + count - 1, all of n nodes and nblk partials,
  int n, nblk;
  long long points;
  long long tours, partial;   // so tour p of the group starts at tours + p (n + 1) and partial + p nblk: no descriptor per tour
};

// Equal sizes: n and per_group travel in the kernel arguments, the bases follow from the tour's index b, and the stop flag is
// its group's, gdone[b / per_group] - one line shared by every block of a launch.
struct UniformAddr {
  static constexpr bool kTable = false;
  int n, per_group, nblk, nchunk;
  const int* gdone;
  __device__ __forceinline__ RaggedTour tour(int b) const {
    const int g = b / per_group;
    const long long row = (long long)b * n;
    return RaggedTour{g, n, nblk, nchunk, (long long)g * 2 * n, row + b, row + b, row, (long long)b * nblk, (long long)b * nblk * nchunk};
  }
  __device__ __forceinline__ RaggedGroup group(int g) const {
    const long long b0 = (long long)g * per_group;
    return RaggedGroup{g * per_group, per_group, n, nblk, (long long)g * 2 * n, b0 * (n + 1), b0 * nblk};
  }
  __device__ __forceinline__ bool stopped(int b) const { return gdone[b / per_group]; }
};

// Any sizes: the tables.  A group that stops also sets tdone of its tours: a block reads its tour's flag by its own index,
// alongside the descriptor and not after it.
struct TableAddr {
  static constexpr bool kTable = true;
  const RaggedTour* desc;
  const RaggedGroup* grp;
  int* tdone;
  __device__ __forceinline__ RaggedTour tour(int b) const { return desc[b]; }
  __device__ __forceinline__ RaggedGroup group(int g) const { return grp[g]; }
  __device__ __forceinline__ bool stopped(int b) const { return tdone[b]; }
};

// ---- the exact move -------------------------------------------------------------------------------------------------------------

template <class A>
__global__ void two_opt_prep_kernel(A a, const double* __restrict__ points, const int* __restrict__ tours,
                                    double2* __restrict__ tp, double* __restrict__ dlen) {
  const RaggedTour d = a.tour(blockIdx.y);
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > d.n || a.stopped(blockIdx.y)) return;
  prep_entry(points + d.points, tours + d.tours, d.n, k, tp + d.tp, dlen + d.cols);
}

template <class A>
__global__ __launch_bounds__(256) void two_opt_best_kernel(A a, const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                           Best* __restrict__ partial) {
  const RaggedTour d = a.tour(blockIdx.y);
  if constexpr (A::kTable)
    if ((int)blockIdx.x >= d.nblk) return;                     // beyond the tour's own tiles
  if (a.stopped(blockIdx.y)) return;
  const Best r = best_tile(tp + d.tp, dlen + d.cols, d.n, blockIdx.x * TI);
  if (threadIdx.x == 0) partial[d.partial + blockIdx.x] = r;
}

// Block g = group g: argmin per tour, the group's minimum decides, every tour applies its best move; a group that stops sets
// its flag (table form: and those of its tours) and counts itself in *stopped.
template <class A>
__global__ __launch_bounds__(256) void two_opt_apply_kernel(A a, int* __restrict__ tours, const Best* __restrict__ partial,
                                                            long long max_iterations, int* stopped, int* __restrict__ gdone,
                                                            long long* __restrict__ giters, Best* __restrict__ chosen) {
  const int g = blockIdx.x;
  if (gdone[g]) return;
  __shared__ double gmin;
  const RaggedGroup G = a.group(g);
  auto stop = [&]() {                                          // thread 0
    gdone[g] = 1;
    if constexpr (A::kTable)
      for (int b = G.first; b < G.first + G.count; ++b) a.tdone[b] = 1;
    atomicAdd(stopped, 1);
  };
  for (int p = 0; p < G.count; ++p) {
    const Best r = tour_argmin(partial + G.partial + (long long)p * G.nblk, G.nblk);
    if (threadIdx.x == 0) chosen[G.first + p] = r;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double m = chosen[G.first].v;
    for (int b = G.first + 1; b < G.first + G.count; ++b) m = chosen[b].v < m ? chosen[b].v : m;
    gmin = m;
  }
  __syncthreads();
  if (!(gmin < -1e-6)) {                                       // tsp_utils.py:39,44
    if (threadIdx.x == 0) stop();
    return;
  }
  for (int p = 0; p < G.count; ++p) apply_move(tours + G.tours + (long long)p * (G.n + 1), chosen[G.first + p].idx, G.n);
  if (threadIdx.x == 0) {
    giters[g] += 1;
    if (giters[g] >= max_iterations) stop();                   // tsp_utils.py:46-47
  }
}

// ---- screened 2-opt (difusco_tsp_two_opt_screened*, _ragged with method 1): the same (min, first flat index) as
// two_opt_best_kernel, with float64 only for the pairs a float32 evaluation of the same formula cannot rule out.
//
// One move is four launches:
//   two_opt_prep_screen_kernel    tp / dlen as above, plus float32 copies q[k] = (P[k], P[k+1]) and d32[k] = fl32(d[k]);
//   two_opt_screen_kernel         c32 of every pair in float32, nothing but a running minimum per thread -> bmin[tile][chunk]
//                                 per block and m32 = min c32 per tour (one atomic min of an order-preserving key);
//   two_opt_screened_best_kernel  U = min(0, m32 + eps) is an upper bound of the tour's exact best value V* = min(0, min c64):
//                                 the pair that attains m32 has c64 <= m32 + eps.  A pair is skipped only if c32 > thr, thr the
//                                 float32 at or above U + eps (rounded up), so c64 >= c32 - eps > U >= V*: a skipped pair is
//                                 strictly worse than the answer and cannot even tie.  Written as !(c32 > thr), so a NaN would
//                                 take the float64 path - a formal guard: within the range of M that has a bound no float32
//                                 intermediate is NaN, and a non-finite coordinate sends the whole call to the exact sweep.  A (tile, chunk) whose bmin > thr holds no survivor and is not revisited;
//                                 survivors are evaluated with the float64 sequence of two_opt_best_kernel and compared with
//                                 better().  On a random tour (half of all pairs improve) and on a decoded one alike the
//                                 survivors are the pairs within 2 eps of the minimum;
//   two_opt_apply_kernel          unchanged.
// Load balance: the screen runs on a (row tile, 1024-column chunk) grid over the triangle j >= i + 2, every block 16 x 1024
// pairs, blocks left of the triangle return at once.
//
// The bound |c32 - c64| <= eps(M) = 96 * 2^-24 * M for 2^-32 <= M <= 2^60, M = the largest |coordinate| of the instance.
// u = 2^-24 (float32 unit roundoff).  c = (|v0| + |v1|) - d_i - d_j in real arithmetic, v0 = P_i - P_j, v1 = P_i+1 - P_j+1.
//  (1) coordinates: x' = fl32(x), |x' - x| <= u M.
//  (2) subtract: dx' = fl32(x_a' - x_b') = (x_a' - x_b')(1 + t), |t| <= u, |x_a' - x_b'| <= 2 M (1 + u), so
//      |dx' - dx| <= 2 u M + 2 u M (1 + u) =: A <= 4.01 u M, and |v' - v| <= sqrt(2) A for v' = (dx', dy').
//  (3) multiply, add: s' = fl32(fl32(dx'^2) + fl32(dy'^2)) or, contracted, fl32(dx'^2 + fl32(dy'^2)) (either operand may be
//      the fused one).  Both terms are >= 0, so in every form s' = |v'|^2 (1 + h) with (1 - u)^2 <= 1 + h <= (1 + u)^2.
//  (4) sqrt: d' = sqrt(s')(1 + r), |r| <= 4 u: covers v_sqrt_f32 (1 ulp = at most 2 u relative) and a correctly rounded sqrt.
//      d' = |v'| (1 + e), |e| <= (1 + u)(1 + 4 u) - 1 <= 5.01 u.  With |v'| <= 2 sqrt(2) M + sqrt(2) A:
//      |d' - |v|| <= sqrt(2) A + 5.01 u (2 sqrt(2) M + sqrt(2) A) <= 19.9 u M              per distance, two of them: 39.8 u M.
//  (5) d_i, d_j: d32 = fl32(d), d <= 2 sqrt(2) M: 2.83 u M each                                                    5.7 u M.
//  (6) three additions (d0' + d1') - d_i' - d_j': all terms >= 0, so every intermediate is at most 4 sqrt(2) M (1 + 6 u) in
//      magnitude and each rounding adds at most u times that: 3 * 5.66 u M (1 + 6 u)                              17.0 u M.
//  Sum: 62.5 u M.  Not yet counted: the float64 roundings inside c64, tp, dlen and in forming U and thr (<= 40 * 2^-53 * 6 M),
//  and underflow - a float32 product, sum, conversion or sqrt input below 2^-126 may be flushed or rounded with an absolute
//  error <= 2^-126, which moves a distance by at most sqrt(3 * 2^-126) + 2^-63 < 2^-61 and c32 by < 2^-59.  For M >= 2^-32 the
//  slack (96 - 62.5) u M > 2^-52 covers both.  Overflow: the largest intermediate is s' <= 8 M^2 (1 + u)^4 < 2^124 for
//  M <= 2^60.  Outside 2^-32 <= M <= 2^60, or with a non-finite coordinate (M = inf / NaN), no bound is claimed:
//  difusco_tsp_two_opt_screen_bound says so and the call runs the exact sweep.
//  Nothing above depends on n: the bound is per pair, from M alone, so in a ragged call (difusco_tsp_two_opt_ragged) it holds
//  for every tour with the M of its own group, whatever the sizes of the other groups.
//  kScreenEpsPerM, kScreenMinM / kScreenMaxM, screen_eps, f32_key and change32 are in two_opt_common.h: the resident 2-opt
//  (tsp_resident.hip) screens with them as well.
constexpr int SCH = 256 * JPT;                     // columns per chunk of the screen

// gmax[g] = bits of the largest |coordinate| of group g (non-negative doubles order like their bits; a NaN sorts above inf)
template <class A>
__global__ void two_opt_maxabs_kernel(A a, const double* __restrict__ points, unsigned long long* __restrict__ gmax) {
  const RaggedGroup G = a.group(blockIdx.y);
  const double* pts = points + G.points;
  unsigned long long m = 0;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < 2 * G.n; k += gridDim.x * blockDim.x) {
    const unsigned long long v = (unsigned long long)__double_as_longlong(fabs(pts[k]));
    m = v > m ? v : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(gmax + blockIdx.y, m);
}

// prep_entry plus the float32 copies of the screen (pointers at the tour's own arrays)
__device__ __forceinline__ void prep_screen_entry(const double* __restrict__ points, const int* __restrict__ tour, int n, int k,
                                                  double2* __restrict__ tp, double* __restrict__ dlen, float4* __restrict__ q,
                                                  float* __restrict__ d32) {
  const int c = tour[k];
  const double2 p = make_double2(points[2 * c], points[2 * c + 1]);
  tp[k] = p;
  if (k < n) {
    const int c1 = tour[k + 1];
    const double2 p1 = make_double2(points[2 * c1], points[2 * c1 + 1]);
    const double d = dist2d(p.x - p1.x, p.y - p1.y);           // as prep_entry
    dlen[k] = d;
    q[k] = make_float4((float)p.x, (float)p.y, (float)p1.x, (float)p1.y);
    d32[k] = (float)d;
  }
}

template <class A>
__global__ void two_opt_prep_screen_kernel(A a, const double* __restrict__ points, const int* __restrict__ tours,
                                           double2* __restrict__ tp, double* __restrict__ dlen, float4* __restrict__ q,
                                           float* __restrict__ d32, unsigned* __restrict__ tmin) {
  const RaggedTour d = a.tour(blockIdx.y);
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > d.n || a.stopped(blockIdx.y)) return;
  if (k == 0) tmin[blockIdx.y] = f32_key(0.0f);                // m32 starts at the value of the no-op move
  prep_screen_entry(points + d.points, tours + d.tours, d.n, k, tp + d.tp, dlen + d.cols, q + d.cols, d32 + d.cols);
}

// the columns of a chunk: thread t holds columns jbase + u * 256 + t; a column past the tour gets d_j = -inf, which makes its
// c32 = +inf
__device__ __forceinline__ void load_columns32(const float4* __restrict__ Q, const float* __restrict__ D, int n, int jbase,
                                               float4 (&c)[JPT], float (&dj)[JPT], int (&jj)[JPT]) {
#pragma unroll
  for (int u = 0; u < JPT; ++u) {
    const int j = jbase + u * 256 + (int)threadIdx.x, jc = j < n ? j : n - 1;
    jj[u] = j;
    c[u] = Q[jc];
    dj[u] = j < n ? D[jc] : -INFINITY;
  }
}

// one block of the screen: min c32 over rows i0 .. i0 + TI - 1 and the chunk's columns of the tour (Q = its q, D = its d32,
// n nodes); the result is valid in thread 0.  Q and D must be block-uniform: the row data then arrive by scalar loads.
__device__ __forceinline__ float screen_tile(const float4* __restrict__ Q, const float* __restrict__ D, int n, int i0, int jbase) {
  float4 c[JPT];
  float dj[JPT];
  int jj[JPT];
  load_columns32(Q, D, n, jbase, c, dj, jj);
  float m = INFINITY;
  if (jbase >= i0 + TI + 1) {                                  // every pair of the block has j >= i + 2 (and i < n - 1)
#pragma unroll
    for (int r = 0; r < TI; ++r) {
      const float4 a = Q[i0 + r];                              // block-uniform: scalar loads
      const float d_i = D[i0 + r];
#pragma unroll
      for (int u = 0; u < JPT; ++u) m = fminf(m, change32(a, d_i, c[u], dj[u]));
    }
  } else {
#pragma unroll
    for (int r = 0; r < TI; ++r) {
      const int i = i0 + r, ic = i < n ? i : n - 1;            // a row past the tour has no j >= i + 2 with d_j > -inf
      const float4 a = Q[ic];
      const float d_i = D[ic];
#pragma unroll
      for (int u = 0; u < JPT; ++u) {
        const float v = change32(a, d_i, c[u], dj[u]);
        m = jj[u] >= i + 2 ? fminf(m, v) : m;
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off));
  __shared__ float wm[4];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  return fminf(fminf(wm[0], wm[1]), fminf(wm[2], wm[3]));
}

// thread 0 of a screen block: its minimum into bmin and into the tour's m32
__device__ __forceinline__ void screen_publish(float m, float* __restrict__ bmin_slot, unsigned* __restrict__ tmin_slot) {
  *bmin_slot = m;
  // the minimum is order-independent, so m32 is deterministic; the relaxed device-scope read only saves atomics
  const unsigned key = f32_key(m);
  if (key < __hip_atomic_load(tmin_slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(tmin_slot, key);
}

template <class A>
__global__ __launch_bounds__(256) void two_opt_screen_kernel(A a, const float4* __restrict__ q, const float* __restrict__ d32,
                                                             float* __restrict__ bmin, unsigned* __restrict__ tmin) {
  const RaggedTour d = a.tour(blockIdx.z);
  const int i0 = blockIdx.x * TI, jbase = blockIdx.y * SCH;
  if constexpr (A::kTable)
    if ((int)blockIdx.x >= d.nblk || (int)blockIdx.y >= d.nchunk) return;   // beyond the tour's own tiles
  if (jbase + SCH <= i0 + 2) return;                                       // the chunk lies left of the triangle
  if (a.stopped(blockIdx.z)) return;
  const float m = screen_tile(q + d.cols, d32 + d.cols, d.n, i0, jbase);
  if (threadIdx.x == 0) screen_publish(m, bmin + d.bmin + (long long)blockIdx.x * d.nchunk + blockIdx.y, tmin + blockIdx.z);
}

// one block of the screened best move: rows i0 .. i0 + TI - 1 of the tour (P, D64: tp, dlen; Q, D: q, d32; n nodes, nchunk
// chunks, bm = the bmin row of this tile); m32 = the tour's screen minimum, eps from its group's M.  The block's best move is
// written to *partial_slot and its float64 evaluations are added to *exact_pairs.
__device__ __forceinline__ void screened_best_tile(const double2* __restrict__ P, const double* __restrict__ D64,
                                                   const float4* __restrict__ Q, const float* __restrict__ D, int n, int nchunk,
                                                   int i0, const float* __restrict__ bm, float m32, double eps,
                                                   Best* __restrict__ partial_slot, unsigned long long* __restrict__ exact_pairs) {
  const double upper = fmin(0.0, (double)m32 + eps);                       // U >= V*
  const float thr = __double2float_ru(upper + eps);
  Best best{0.0, 0};
  unsigned cnt = 0;
  for (int chunk = (i0 + 2) / SCH; chunk < nchunk; ++chunk) {
    if (bm[chunk] > thr) continue;                            // no pair of this block's chunk can reach the answer
    float4 c[JPT];
    float dj[JPT];
    int jj[JPT];
    load_columns32(Q, D, n, chunk * SCH, c, dj, jj);
    for (int r = 0; r < TI; ++r) {
      const int i = i0 + r, ic = i < n ? i : n - 1;
      const float4 a = Q[ic];
      const float d_i = D[ic];
#pragma unroll
      for (int u = 0; u < JPT; ++u) {
        const int j = jj[u];
        if (j < n && j >= i + 2 && !(change32(a, d_i, c[u], dj[u]) > thr)) {
          // the float64 sequence of two_opt_best_kernel
          const double2 p0 = P[i], p1 = P[i + 1], pj = P[j], pj1 = P[j + 1];
          const double x0 = p0.x - pj.x, y0 = p0.y - pj.y;
          const double x1 = p1.x - pj1.x, y1 = p1.y - pj1.y;
          const double change = __dsub_rn(__dsub_rn(__dadd_rn(dist2d(x0, y0), dist2d(x1, y1)), D64[i]), D64[j]);
          const long long idx = (long long)i * n + j;
          if (better(change, idx, best)) best = Best{change, idx};
          ++cnt;
        }
      }
    }
  }
  __shared__ Best red[256];
  __shared__ unsigned cred[256];
  red[threadIdx.x] = best;
  cred[threadIdx.x] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      if (better(red[threadIdx.x + s].v, red[threadIdx.x + s].idx, red[threadIdx.x])) red[threadIdx.x] = red[threadIdx.x + s];
      cred[threadIdx.x] += cred[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *partial_slot = red[0];
    if (cred[0]) atomicAdd(exact_pairs, (unsigned long long)cred[0]);
  }
}

template <class A>
__global__ __launch_bounds__(256) void two_opt_screened_best_kernel(
    A a, const double2* __restrict__ tp, const double* __restrict__ dlen, const float4* __restrict__ q,
    const float* __restrict__ d32, const float* __restrict__ bmin, const unsigned* __restrict__ tmin,
    const double* __restrict__ gmax, Best* __restrict__ partial, unsigned long long* __restrict__ exact_pairs) {
  const RaggedTour d = a.tour(blockIdx.y);
  if constexpr (A::kTable)
    if ((int)blockIdx.x >= d.nblk) return;                     // beyond the tour's own tiles
  if (a.stopped(blockIdx.y)) return;
  screened_best_tile(tp + d.tp, dlen + d.cols, q + d.cols, d32 + d.cols, d.n, d.nchunk, blockIdx.x * TI,
                     bmin + d.bmin + (long long)blockIdx.x * d.nchunk, f32_unkey(tmin[blockIdx.y]), screen_eps(gmax[d.group]),
                     partial + d.partial + blockIdx.x, exact_pairs);
}

// ---- the host side: one layout, one driver --------------------------------------------------------------------------------------

struct TwoOptCall {        // what an entry asks for; the first block is all the layout needs
  const char* who;         // for the messages
  bool table;              // false: `groups` groups of per_group tours of n nodes (UniformAddr); true: group_n / group_tours (TableAddr)
  int method;              // 0 exact, 1 screened
  int groups, n, per_group;
  const int32_t *group_n, *group_tours;
  const double* points;
  int32_t* tours;
  int64_t max_iterations;
  void* workspace;
  size_t workspace_bytes;
  int64_t* iterations_out;   // host [groups]
  int64_t* exact_pairs_out;  // host, optional
  void* stream;
  int n_of(int g) const { return table ? group_n[g] : n; }
  int tours_of(int g) const { return table ? group_tours[g] : per_group; }
};

// Byte offsets.  The exact uniform entries' arrays first, in their order, so the screened entries run the exact sweep on the same
// workspace; desc, grp and tdone only in the table form, q .. counter only with method 1.
struct TwoOptLayout {
  size_t desc, grp, tp, dlen, partial, chosen, gdone, tdone, giters, stopped, q, d32, bmin, tmin, gmax, counter, total;
  int tours, nmax, nblk_max, nchunk_max;
  std::vector<RaggedTour> tab;     // the host tables (table form, on request)
  std::vector<RaggedGroup> gtab;
};

// lays the workspace of a call out (the group arrays are checked by then); with_tables: builds the tables as well
int two_opt_layout(const TwoOptCall& c, bool with_tables, TwoOptLayout* L) {
  size_t points = 0, closed = 0, cols = 0, nblks = 0, tiles = 0, T = 0;
  L->nmax = L->nblk_max = L->nchunk_max = 0;
  const int kinds = c.table ? c.groups : 1;                    // uniform: one kind of group, c.groups times
  for (int g = 0; g < kinds; ++g) {
    const int n = c.n_of(g), nblk = (n + TI - 1) / TI, nchunk = (n + SCH - 1) / SCH;
    const size_t count = c.table ? (size_t)c.group_tours[g] : (size_t)c.groups * c.per_group;
    L->nmax = n > L->nmax ? n : L->nmax;
    L->nblk_max = nblk > L->nblk_max ? nblk : L->nblk_max;
    L->nchunk_max = nchunk > L->nchunk_max ? nchunk : L->nchunk_max;
    if (c.table && with_tables) {
      L->gtab.push_back(RaggedGroup{(int)T, (int)count, n, nblk, (long long)points, (long long)closed, (long long)nblks});
      for (size_t p = 0; p < count; ++p)
        L->tab.push_back(RaggedTour{g, n, nblk, nchunk, (long long)points, (long long)(closed + p * (n + 1)),
                                    (long long)(closed + p * (n + 1)), (long long)(cols + p * n), (long long)(nblks + p * nblk),
                                    (long long)(tiles + p * nblk * nchunk)});
    }
    T += count;
    closed += count * ((size_t)n + 1);
    cols += count * n;
    nblks += count * nblk;
    tiles += count * nblk * nchunk;
    points += 2 * (size_t)n;
  }
  if (!c.table && c.method == 1 && (T > 65535 || L->nblk_max > 65535 || L->nchunk_max > 65535))
    return set_error(DIFUSCO_EINVAL, "two_opt_screened: at most 65535 tours per call and %d nodes", 65535 * TI);
  L->tours = (int)T;
  size_t off = 0;
  auto take = [&off](bool present, size_t bytes) {
    const size_t at = off;
    if (present) off += up256(bytes);
    return at;
  };
  L->desc = take(c.table, sizeof(RaggedTour) * T);
  L->grp = take(c.table, sizeof(RaggedGroup) * c.groups);
  L->tp = take(true, sizeof(double2) * closed);
  L->dlen = take(true, sizeof(double) * cols);
  L->partial = take(true, sizeof(Best) * nblks);
  L->chosen = take(true, sizeof(Best) * T);
  L->gdone = take(true, sizeof(int) * c.groups);               // gdone .. stopped are cleared by one memset
  L->tdone = take(c.table, sizeof(int) * T);
  L->giters = take(true, sizeof(long long) * c.groups);
  L->stopped = take(true, sizeof(int));                        // the number of groups that have stopped
  const bool screen = c.method == 1;
  L->q = take(screen, sizeof(float4) * cols);
  L->d32 = take(screen, sizeof(float) * cols);
  L->bmin = take(screen, sizeof(float) * tiles);
  L->tmin = take(screen, sizeof(unsigned) * T);
  L->gmax = take(screen, sizeof(double) * c.groups);           // gmax and counter are cleared by one memset
  L->counter = take(screen, sizeof(unsigned long long));
  L->total = off;
  return DIFUSCO_OK;
}

int two_opt_bytes(const TwoOptCall& c, size_t* bytes) {
  TwoOptLayout lay;
  const int rc = two_opt_layout(c, false, &lay);
  if (rc == DIFUSCO_OK) *bytes = lay.total;
  return rc;
}

struct TwoOptPtrs {        // (workspace, layout) as typed pointers
  RaggedTour* desc;
  RaggedGroup* grp;
  double2* tp;
  double* dlen;
  Best *partial, *chosen;
  int *gdone, *tdone;
  long long* giters;
  int* stopped;
  float4* q;
  float *d32, *bmin;
  unsigned* tmin;
  unsigned long long *gmax, *counter;
  TwoOptPtrs(void* workspace, const TwoOptLayout& L) {
    char* w = (char*)workspace;
    desc = (RaggedTour*)(w + L.desc), grp = (RaggedGroup*)(w + L.grp);
    tp = (double2*)(w + L.tp), dlen = (double*)(w + L.dlen);
    partial = (Best*)(w + L.partial), chosen = (Best*)(w + L.chosen);
    gdone = (int*)(w + L.gdone), tdone = (int*)(w + L.tdone);
    giters = (long long*)(w + L.giters), stopped = (int*)(w + L.stopped);
    q = (float4*)(w + L.q), d32 = (float*)(w + L.d32), bmin = (float*)(w + L.bmin), tmin = (unsigned*)(w + L.tmin);
    gmax = (unsigned long long*)(w + L.gmax), counter = (unsigned long long*)(w + L.counter);
  }
};

long long evaluations(long long iterations, long long max_iterations) {   // sweeps of the exact loop that did work
  return iterations < (max_iterations > 0 ? max_iterations : 1) ? iterations + 1 : iterations;
}

// the max |coordinate| pass of a screened call
template <class A>
void launch_maxabs(const A& a, const TwoOptCall& c, const TwoOptLayout& L, const TwoOptPtrs& p, hipStream_t s) {
  const int mblocks = (2 * L.nmax + 255) / 256 < 64 ? (2 * L.nmax + 255) / 256 : 64;
  hipLaunchKernelGGL(two_opt_maxabs_kernel<A>, dim3(mblocks, c.groups), dim3(256), 0, s, a, c.points, p.gmax);
}

// the launches of one move: prep, best or screen + screened best, apply
template <class A>
void launch_move(const A& a, bool screened, const TwoOptCall& c, const TwoOptLayout& L, const TwoOptPtrs& p, hipStream_t s) {
  const int T = L.tours;
  const dim3 prep_grid((L.nmax + 1 + 255) / 256, T), best_grid(L.nblk_max, T);
  if (screened) {
    hipLaunchKernelGGL(two_opt_prep_screen_kernel<A>, prep_grid, dim3(256), 0, s, a, c.points, (const int*)c.tours, p.tp, p.dlen,
                       p.q, p.d32, p.tmin);
    hipLaunchKernelGGL(two_opt_screen_kernel<A>, dim3(L.nblk_max, L.nchunk_max, T), dim3(256), 0, s, a, (const float4*)p.q,
                       (const float*)p.d32, p.bmin, p.tmin);
    hipLaunchKernelGGL(two_opt_screened_best_kernel<A>, best_grid, dim3(256), 0, s, a, (const double2*)p.tp, (const double*)p.dlen,
                       (const float4*)p.q, (const float*)p.d32, (const float*)p.bmin, (const unsigned*)p.tmin,
                       (const double*)p.gmax, p.partial, p.counter);
  } else {
    hipLaunchKernelGGL(two_opt_prep_kernel<A>, prep_grid, dim3(256), 0, s, a, c.points, (const int*)c.tours, p.tp, p.dlen);
    hipLaunchKernelGGL(two_opt_best_kernel<A>, best_grid, dim3(256), 0, s, a, (const double2*)p.tp, (const double*)p.dlen,
                       p.partial);
  }
  hipLaunchKernelGGL(two_opt_apply_kernel<A>, dim3(c.groups), dim3(256), 0, s, a, (int*)c.tours, (const Best*)p.partial,
                     (long long)c.max_iterations, p.stopped, p.gdone, p.giters, p.chosen);
}

// The driver of every entry (whose own argument checks have passed): layout, clearing, the tables (table form), the bound
// decision (method 1), the moves with a host poll every 8, the read-back.
int two_opt_run(const TwoOptCall& c) {
  TwoOptLayout L;
  const int rc = two_opt_layout(c, true, &L);
  if (rc != DIFUSCO_OK) return rc;
  if (c.workspace_bytes < L.total)
    return set_error(DIFUSCO_EINVAL, "%s: workspace %zu < %zu bytes", c.who, c.workspace_bytes, L.total);
  const TwoOptPtrs p(c.workspace, L);
  const UniformAddr ua{c.n, c.per_group, L.nblk_max, L.nchunk_max, p.gdone};
  const TableAddr ta{p.desc, p.grp, p.tdone};
  hipStream_t s = (hipStream_t)c.stream;
  const int groups = c.groups;
  hipError_t er = hipSuccess;
  if (c.table) {                                               // the tables, once per call; L holds them until the synchronisation below
    er = hipMemcpyAsync(p.desc, L.tab.data(), sizeof(RaggedTour) * L.tours, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(p.grp, L.gtab.data(), sizeof(RaggedGroup) * groups, hipMemcpyHostToDevice, s);
  }
  if (er == hipSuccess) er = hipMemsetAsync(p.gdone, 0, (char*)p.stopped + sizeof(int) - (char*)p.gdone, s);
  bool screened = c.method == 1;
  if (er == hipSuccess && screened) {                          // M per group decides, once per call, whether the screen has a bound
    er = hipMemsetAsync(p.gmax, 0, L.total - L.gmax, s);
    if (er == hipSuccess) {
      if (c.table) launch_maxabs(ta, c, L, p, s);
      else launch_maxabs(ua, c, L, p, s);
    }
    std::vector<double> maxabs(groups);
    if (er == hipSuccess) er = hipMemcpyAsync(maxabs.data(), p.gmax, sizeof(double) * groups, hipMemcpyDeviceToHost, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    for (int g = 0; er == hipSuccess && g < groups; ++g) {
      double eps = 0.0;
      screened = screened && difusco_tsp_two_opt_screen_bound(maxabs[g], &eps) == 1;   // one group without a bound: exact sweep
    }
  } else if (er == hipSuccess && c.table) {
    er = hipStreamSynchronize(s);
  }
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s setup: %s", c.who, hipGetErrorString(er));
  // the reference evaluates the moves once more after the last applied one and stops on `min_change >= -1e-6`;
  // at most max_iterations moves are applied (tsp_utils.py:20-47)
  const int poll = 8;
  const long long loops = c.max_iterations > 0 ? c.max_iterations : 1;   // the reference always evaluates (and may apply) once
  for (long long it = 0; it < loops; ++it) {
    if (c.table) launch_move(ta, screened, c, L, p, s);
    else launch_move(ua, screened, c, L, p, s);
    if ((it + 1) % poll == 0 || it + 1 == loops) {
      int stopped = 0;
      er = hipMemcpyAsync(&stopped, p.stopped, sizeof(int), hipMemcpyDeviceToHost, s);
      if (er == hipSuccess) er = hipStreamSynchronize(s);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s state: %s", c.who, hipGetErrorString(er));
      if (stopped >= groups) break;
    }
  }
  unsigned long long pairs = 0;
  er = hipMemcpyAsync(c.iterations_out, p.giters, sizeof(long long) * groups, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess && screened) er = hipMemcpyAsync(&pairs, p.counter, sizeof(pairs), hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "%s iterations: %s", c.who, hipGetErrorString(er));
  if (!c.exact_pairs_out) return DIFUSCO_OK;
  if (!screened)                                               // every pair of every sweep that did work, in float64
    for (int g = 0; g < groups; ++g)
      pairs += (unsigned long long)(evaluations(c.iterations_out[g], c.max_iterations) * c.tours_of(g) *
                                    ((long long)(c.n_of(g) - 1) * (c.n_of(g) - 2) / 2));
  *c.exact_pairs_out = (int64_t)pairs;
  return DIFUSCO_OK;
}

TwoOptCall uniform_call(const char* who, int method, int n, int groups, int per_group) {
  TwoOptCall c{};
  c.who = who, c.method = method, c.n = n, c.groups = groups, c.per_group = per_group;
  return c;
}

}  // namespace
}  // namespace difusco

extern "C" {

// one group of `batch` tours
int difusco_tsp_two_opt_workspace_bytes(int n_nodes, int batch, size_t* bytes) {
  using namespace difusco;
  if (!bytes || n_nodes < 4 || batch < 1) return set_error(DIFUSCO_EINVAL, "two_opt_workspace_bytes: bad arguments");
  return two_opt_bytes(uniform_call("two_opt_workspace_bytes", 0, n_nodes, 1, batch), bytes);
}

int difusco_tsp_two_opt(int n_nodes, int batch, const double* points, int32_t* tours, int64_t max_iterations,
                        void* workspace, size_t workspace_bytes, int64_t* iterations_out, void* stream) {
  using namespace difusco;
  if (n_nodes < 4 || batch < 1 || !points || !tours || !workspace || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt: needs n_nodes >= 4, batch >= 1 and non-null device arrays");
  int64_t iterations = 0;
  TwoOptCall c = uniform_call("tsp_two_opt", 0, n_nodes, 1, batch);
  c.points = points, c.tours = tours, c.max_iterations = max_iterations, c.workspace = workspace;
  c.workspace_bytes = workspace_bytes, c.iterations_out = &iterations, c.stream = stream;
  const int rc = two_opt_run(c);
  if (rc == DIFUSCO_OK && iterations_out) *iterations_out = iterations;
  return rc;
}

int difusco_tsp_two_opt_grouped_workspace_bytes(int n_nodes, int groups, int per_group, size_t* bytes) {
  using namespace difusco;
  if (!bytes || n_nodes < 4 || groups < 1 || per_group < 1 || (long long)groups * per_group > (1 << 30))
    return set_error(DIFUSCO_EINVAL, "two_opt_grouped_workspace_bytes: bad arguments");
  return two_opt_bytes(uniform_call("two_opt_grouped_workspace_bytes", 0, n_nodes, groups, per_group), bytes);
}

int difusco_tsp_two_opt_grouped(int n_nodes, int groups, int per_group, const double* points, int32_t* tours,
                                int64_t max_iterations, void* workspace, size_t workspace_bytes, int64_t* iterations_out,
                                void* stream) {
  using namespace difusco;
  if (n_nodes < 4 || groups < 1 || per_group < 1 || (long long)groups * per_group > (1 << 30) || !points || !tours ||
      !workspace || !iterations_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt_grouped: needs n_nodes >= 4, groups, per_group >= 1, non-null device arrays "
                                     "and a host iterations_out[groups]");
  TwoOptCall c = uniform_call("tsp_two_opt_grouped", 0, n_nodes, groups, per_group);
  c.points = points, c.tours = tours, c.max_iterations = max_iterations, c.workspace = workspace;
  c.workspace_bytes = workspace_bytes, c.iterations_out = iterations_out, c.stream = stream;
  return two_opt_run(c);
}

int difusco_tsp_two_opt_screen_bound(double max_abs_coord, double* eps) {
  using namespace difusco;
  if (!eps) return set_error(DIFUSCO_EINVAL, "two_opt_screen_bound: eps is null");
  *eps = 0.0;
  if (!(max_abs_coord >= kScreenMinM && max_abs_coord <= kScreenMaxM)) return 0;   // also inf and NaN
  *eps = screen_eps(max_abs_coord);
  return 1;
}

int difusco_tsp_two_opt_grouped_screened_workspace_bytes(int n_nodes, int groups, int per_group, size_t* bytes) {
  using namespace difusco;
  if (!bytes || n_nodes < 4 || groups < 1 || per_group < 1 || (long long)groups * per_group > (1 << 30))
    return set_error(DIFUSCO_EINVAL, "two_opt_grouped_screened_workspace_bytes: bad arguments");
  return two_opt_bytes(uniform_call("two_opt_grouped_screened_workspace_bytes", 1, n_nodes, groups, per_group), bytes);
}

int difusco_tsp_two_opt_grouped_screened(int n_nodes, int groups, int per_group, const double* points, int32_t* tours,
                                         int64_t max_iterations, void* workspace, size_t workspace_bytes,
                                         int64_t* iterations_out, int64_t* exact_pairs_out, void* stream) {
  using namespace difusco;
  if (n_nodes < 4 || groups < 1 || per_group < 1 || (long long)groups * per_group > (1 << 30) || !points || !tours ||
      !workspace || !iterations_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt_grouped_screened: needs n_nodes >= 4, groups, per_group >= 1, non-null device "
                                     "arrays and a host iterations_out[groups]");
  TwoOptCall c = uniform_call("tsp_two_opt_screened", 1, n_nodes, groups, per_group);
  c.points = points, c.tours = tours, c.max_iterations = max_iterations, c.workspace = workspace;
  c.workspace_bytes = workspace_bytes, c.iterations_out = iterations_out, c.exact_pairs_out = exact_pairs_out, c.stream = stream;
  return two_opt_run(c);
}

int difusco_tsp_two_opt_screened_workspace_bytes(int n_nodes, int batch, size_t* bytes) {
  using namespace difusco;
  if (!bytes || n_nodes < 4 || batch < 1) return set_error(DIFUSCO_EINVAL, "two_opt_screened_workspace_bytes: bad arguments");
  return two_opt_bytes(uniform_call("two_opt_screened_workspace_bytes", 1, n_nodes, 1, batch), bytes);
}

// one group of `batch` tours
int difusco_tsp_two_opt_screened(int n_nodes, int batch, const double* points, int32_t* tours, int64_t max_iterations,
                                 void* workspace, size_t workspace_bytes, int64_t* iterations_out, int64_t* exact_pairs_out,
                                 void* stream) {
  using namespace difusco;
  if (n_nodes < 4 || batch < 1 || !points || !tours || !workspace || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt_screened: needs n_nodes >= 4, batch >= 1 and non-null device arrays");
  int64_t iterations = 0;
  TwoOptCall c = uniform_call("tsp_two_opt_screened", 1, n_nodes, 1, batch);
  c.points = points, c.tours = tours, c.max_iterations = max_iterations, c.workspace = workspace;
  c.workspace_bytes = workspace_bytes, c.iterations_out = &iterations, c.exact_pairs_out = exact_pairs_out, c.stream = stream;
  const int rc = two_opt_run(c);
  if (rc == DIFUSCO_OK && iterations_out) *iterations_out = iterations;
  return rc;
}

int difusco_tsp_two_opt_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int method,
                                               size_t* bytes) {
  using namespace difusco;
  const char* who = "two_opt_ragged_workspace_bytes";
  if (!bytes) return set_error(DIFUSCO_EINVAL, "%s: bytes is null", who);
  int T = 0;
  const int rc = check_groups(who, groups, group_n, group_tours, &T);
  if (rc != DIFUSCO_OK) return rc;
  if (method != 0 && method != 1) return set_error(DIFUSCO_EINVAL, "%s: method %d (0 exact, 1 screened)", who, method);
  TwoOptCall c{};
  c.who = who, c.table = true, c.method = method, c.groups = groups, c.group_n = group_n, c.group_tours = group_tours;
  return two_opt_bytes(c, bytes);
}

int difusco_tsp_two_opt_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                               int32_t* tours, int64_t max_iterations, int method, void* workspace, size_t workspace_bytes,
                               int64_t* iterations_out, int64_t* exact_pairs_out, void* stream) {
  using namespace difusco;
  const char* who = "tsp_two_opt_ragged";
  int T = 0;
  const int rc = check_groups(who, groups, group_n, group_tours, &T);
  if (rc != DIFUSCO_OK) return rc;
  if (method != 0 && method != 1) return set_error(DIFUSCO_EINVAL, "%s: method %d (0 exact, 1 screened)", who, method);
  if (!points || !tours || !workspace || !iterations_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt_ragged: needs non-null device arrays, a host iterations_out[groups] and "
                                     "max_iterations >= 0");
  TwoOptCall c{};
  c.who = who, c.table = true, c.method = method, c.groups = groups, c.group_n = group_n, c.group_tours = group_tours;
  c.points = points, c.tours = tours, c.max_iterations = max_iterations, c.workspace = workspace;
  c.workspace_bytes = workspace_bytes, c.iterations_out = iterations_out, c.exact_pairs_out = exact_pairs_out, c.stream = stream;
  return two_opt_run(c);
}

}  // extern "C"
