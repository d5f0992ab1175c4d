// Batched 2-opt refinement of decoded tours (difusco/utils/tsp_utils.py:12-49 `batched_two_opt_torch`), SURVEY 8(f)-2.
//
// The reference materialises four N x N float64 distance matrices per iteration (A_ij, A_i+1,j+1, A_i,i+1, A_j,j+1),
// takes triu(diagonal=2) of their combination, and an argmin per tour; up to 1000-5000 iterations.  Here one
// iteration is three small launches with nothing N x N in memory:
//   two_opt_prep_kernel   P[k] = points[tour[k]] (tour order) and d[k] = |P[k] - P[k+1]|;
//   two_opt_best_kernel   every thread keeps P[j], P[j+1], d[j] of its columns in registers, a block sweeps a tile of
//                         rows i, change = ((A_ij + A_i+1,j+1) - d_i) - d_j in float64 in the reference's operation
//                         order, running (min, first flat index) per thread -> block -> partial[];
//   two_opt_apply_kernel  per tour: argmin over the partials (ties: lowest flat index = first occurrence, what
//                         torch.argmin returns on the flattened matrix); min over the batch decides (tsp_utils.py:
//                         33,39: one global `min_change < -1e-6` test, every tour applies its own best move);
//                         the segment tour[i+1 .. j] is reversed in place, the iteration counter advances.
// Invalid entries (j < i + 2) are zeros in the reference's matrix, so the minimum is never positive and the argmin of
// an all-non-improving matrix is flat index 0 = a no-op reversal: the running best starts at (0.0, 0).
// The host only polls a `done` flag every few iterations; once set, the remaining launches return immediately.
// Three shapes of a call share the per-block code (screen_tile, screened_best_tile here; best_tile, tour_argmin, apply_move in
// two_opt_common.h, which the local search of or_opt.hip uses as well): one
// batch (difusco_tsp_two_opt), groups of one n (_grouped) and groups of different n (_ragged, at the end of the namespace).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

struct TwoOptState {       // device-resident loop state
  int done;
  int pad;
  long long iterations;
};

// GROUPED (difusco_tsp_two_opt_grouped): tour b belongs to group b / per_group, which has points of its own
// (points + group * 2 n) and a done flag of its own (gdone[group]); otherwise one state for the whole batch.
template <bool GROUPED>
__global__ void two_opt_prep_kernel(const double* __restrict__ points, const int* __restrict__ tours, int n, int batch,
                                    double2* __restrict__ tp, double* __restrict__ dlen, const TwoOptState* st,
                                    const int* __restrict__ gdone, int per_group) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if constexpr (GROUPED) {
    if (gdone[b / per_group]) return;
    points += (long long)(b / per_group) * 2 * n;
  } else {
    if (st->done) return;
  }
  if (k > n) return;
  prep_entry(points, tours + (long long)b * (n + 1), n, k, tp + (long long)b * (n + 1), dlen + (long long)b * n);
}

template <bool GROUPED>
__global__ __launch_bounds__(256) void two_opt_best_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                           int n, Best* __restrict__ partial, const TwoOptState* st,
                                                           const int* __restrict__ gdone, int per_group) {
  const int b = blockIdx.y, i0 = blockIdx.x * TI;
  if constexpr (GROUPED) {
    if (gdone[b / per_group]) return;
  } else {
    if (st->done) return;
  }
  const Best r = best_tile(tp + (long long)b * (n + 1), dlen + (long long)b * n, n, i0);
  if (threadIdx.x == 0) partial[(long long)b * gridDim.x + blockIdx.x] = r;
}

__global__ __launch_bounds__(256) void two_opt_apply_kernel(int* __restrict__ tours, int n, int batch, int nblk,
                                                            const Best* __restrict__ partial, long long max_iterations,
                                                            TwoOptState* st, Best* __restrict__ chosen) {
  if (st->done) return;
  __shared__ double gmin;
  // per tour: argmin over its partials
  for (int b = 0; b < batch; ++b) {
    const Best r = tour_argmin(partial + (long long)b * nblk, nblk);
    if (threadIdx.x == 0) chosen[b] = r;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double m = chosen[0].v;
    for (int b = 1; b < batch; ++b) m = chosen[b].v < m ? chosen[b].v : m;
    gmin = m;
  }
  __syncthreads();
  if (!(gmin < -1e-6)) {                                  // tsp_utils.py:39,44
    if (threadIdx.x == 0) st->done = 1;
    return;
  }
  for (int b = 0; b < batch; ++b) apply_move(tours + (long long)b * (n + 1), chosen[b].idx, n);
  if (threadIdx.x == 0) {
    st->iterations += 1;
    if (st->iterations >= max_iterations) st->done = 1;   // tsp_utils.py:46-47
  }
}

// The apply step of difusco_tsp_two_opt_grouped: block g = group g, the steps of two_opt_apply_kernel over the group's own
// tours (argmin per tour, the group's minimum decides, every tour applies its best move); a group that stops sets its flag
// and counts itself in st->done (= number of stopped groups).
__global__ __launch_bounds__(256) void two_opt_apply_grouped_kernel(int* __restrict__ tours, int n, int per_group, int nblk,
                                                                    const Best* __restrict__ partial, long long max_iterations,
                                                                    TwoOptState* st, int* __restrict__ gdone,
                                                                    long long* __restrict__ giters, Best* __restrict__ chosen) {
  const int g = blockIdx.x;
  if (gdone[g]) return;
  __shared__ double gmin;
  const int b0 = g * per_group;
  for (int b = b0; b < b0 + per_group; ++b) {
    const Best r = tour_argmin(partial + (long long)b * nblk, nblk);
    if (threadIdx.x == 0) chosen[b] = r;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double m = chosen[b0].v;
    for (int b = b0 + 1; b < b0 + per_group; ++b) m = chosen[b].v < m ? chosen[b].v : m;
    gmin = m;
  }
  __syncthreads();
  if (!(gmin < -1e-6)) {
    if (threadIdx.x == 0) {
      gdone[g] = 1;
      atomicAdd(&st->done, 1);
    }
    return;
  }
  for (int b = b0; b < b0 + per_group; ++b) apply_move(tours + (long long)b * (n + 1), chosen[b].idx, n);
  if (threadIdx.x == 0) {
    giters[g] += 1;
    if (giters[g] >= max_iterations) {
      gdone[g] = 1;
      atomicAdd(&st->done, 1);
    }
  }
}

// the workspace of difusco_tsp_two_opt_grouped (byte offsets): the screened entries run on the same arrays and append their own
struct GroupedLayout {
  size_t tp, dlen, partial, chosen, gdone, giters, st, total;
};

GroupedLayout grouped_layout(int n, int groups, int per_group) {
  const size_t batch = (size_t)groups * per_group, nblk = (size_t)(n + TI - 1) / TI;
  GroupedLayout L;
  size_t off = 0;
  L.tp = off;
  off += up256(sizeof(double2) * batch * (n + 1));
  L.dlen = off;
  off += up256(sizeof(double) * batch * n);
  L.partial = off;
  off += up256(sizeof(Best) * batch * nblk);
  L.chosen = off;
  off += up256(sizeof(Best) * batch);
  L.gdone = off;
  off += up256(sizeof(int) * groups);
  L.giters = off;
  off += up256(sizeof(long long) * groups);
  L.st = off;                            // TwoOptState: st->done = number of groups that have stopped
  L.total = off + 256;
  return L;
}

// ---- screened 2-opt (difusco_tsp_two_opt_screened*): the same (min, first flat index) as two_opt_best_kernel, with float64 only
// for the pairs a float32 evaluation of the same formula cannot rule out.
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
//   two_opt_apply_grouped_kernel  unchanged.
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
constexpr double kScreenEpsPerM = 0x1.8p-18;       // 96 * 2^-24
constexpr double kScreenMinM = 0x1p-32, kScreenMaxM = 0x1p60;
constexpr int SCH = 256 * JPT;                     // columns per chunk of the screen

__host__ __device__ inline double screen_eps(double m) { return m * kScreenEpsPerM; }

// order-preserving key of a float32 (no NaN): a < b  <=>  key(a) < key(b)
__device__ __forceinline__ unsigned f32_key(float v) {
  const unsigned bits = __float_as_uint(v);
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ float f32_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ float dist32(float dx, float dy) { return __builtin_amdgcn_sqrtf(__builtin_fmaf(dx, dx, dy * dy)); }

// q = (P_i, P_i+1), c = (P_j, P_j+1)
__device__ __forceinline__ float change32(float4 q, float d_i, float4 c, float d_j) {
  const float d0 = dist32(q.x - c.x, q.y - c.y), d1 = dist32(q.z - c.z, q.w - c.w);
  return ((d0 + d1) - d_i) - d_j;
}

// gmax[g] = bits of the largest |coordinate| of group g (non-negative doubles order like their bits; a NaN sorts above inf)
__global__ void two_opt_maxabs_kernel(const double* __restrict__ points, int n2, unsigned long long* __restrict__ gmax) {
  const int g = blockIdx.y;
  unsigned long long m = 0;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n2; k += gridDim.x * blockDim.x) {
    const unsigned long long v = (unsigned long long)__double_as_longlong(fabs(points[(long long)g * n2 + k]));
    m = v > m ? v : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(gmax + g, m);
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

__global__ void two_opt_prep_screen_kernel(const double* __restrict__ points, const int* __restrict__ tours, int n,
                                           double2* __restrict__ tp, double* __restrict__ dlen, float4* __restrict__ q,
                                           float* __restrict__ d32, unsigned* __restrict__ tmin,
                                           const int* __restrict__ gdone, int per_group) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (gdone[b / per_group]) return;
  points += (long long)(b / per_group) * 2 * n;
  if (k > n) return;
  if (k == 0) tmin[b] = f32_key(0.0f);                         // m32 starts at the value of the no-op move
  const long long row = (long long)b * n;
  prep_screen_entry(points, tours + (long long)b * (n + 1), n, k, tp + (long long)b * (n + 1), dlen + row, q + row, d32 + row);
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

__global__ __launch_bounds__(256) void two_opt_screen_kernel(const float4* __restrict__ q, const float* __restrict__ d32, int n,
                                                             float* __restrict__ bmin, unsigned* __restrict__ tmin,
                                                             const int* __restrict__ gdone, int per_group) {
  const int b = blockIdx.z, i0 = blockIdx.x * TI, jbase = blockIdx.y * SCH;
  if (jbase + SCH <= i0 + 2) return;                           // the chunk lies left of the triangle
  if (gdone[b / per_group]) return;
  const float m = screen_tile(q + (long long)b * n, d32 + (long long)b * n, n, i0, jbase);
  if (threadIdx.x == 0) screen_publish(m, bmin + ((long long)b * gridDim.x + blockIdx.x) * gridDim.y + blockIdx.y, tmin + b);
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

__global__ __launch_bounds__(256) void two_opt_screened_best_kernel(
    const double2* __restrict__ tp, const double* __restrict__ dlen, const float4* __restrict__ q, const float* __restrict__ d32,
    int n, int nchunk, const float* __restrict__ bmin, const unsigned* __restrict__ tmin, const double* __restrict__ gmax,
    Best* __restrict__ partial, unsigned long long* __restrict__ exact_pairs, const int* __restrict__ gdone, int per_group) {
  const int b = blockIdx.y, i0 = blockIdx.x * TI, g = b / per_group;
  if (gdone[g]) return;
  const long long row = (long long)b * n;
  screened_best_tile(tp + (long long)b * (n + 1), dlen + row, q + row, d32 + row, n, nchunk, i0,
                     bmin + ((long long)b * gridDim.x + blockIdx.x) * nchunk, f32_unkey(tmin[b]), screen_eps(gmax[g]),
                     partial + (long long)b * gridDim.x + blockIdx.x, exact_pairs);
}

struct ScreenedLayout {    // the exact entries' layout first (the exact sweep runs on the same workspace), then the screen's arrays
  size_t q, d32, bmin, tmin, gmax, counter, total;
};

int screened_layout(int n, int groups, int per_group, ScreenedLayout* L) {
  const size_t base = grouped_layout(n, groups, per_group).total;
  const size_t batch = (size_t)groups * per_group, nblk = (size_t)(n + TI - 1) / TI, nchunk = (size_t)(n + SCH - 1) / SCH;
  if (batch > 65535 || nblk > 65535 || nchunk > 65535)
    return set_error(DIFUSCO_EINVAL, "two_opt_screened: at most 65535 tours per call and %d nodes", 65535 * TI);
  size_t off = up256(base);
  L->q = off;
  off += up256(sizeof(float4) * batch * n);
  L->d32 = off;
  off += up256(sizeof(float) * batch * n);
  L->bmin = off;
  off += up256(sizeof(float) * batch * nblk * nchunk);
  L->tmin = off;
  off += up256(sizeof(unsigned) * batch);
  L->gmax = off;
  off += up256(sizeof(double) * groups);
  L->counter = off;
  off += 256;
  L->total = off;
  return DIFUSCO_OK;
}

long long evaluations(long long iterations, long long max_iterations) {   // sweeps of the exact loop that did work
  return iterations < (max_iterations > 0 ? max_iterations : 1) ? iterations + 1 : iterations;
}

int two_opt_screened_run(int n, int groups, int per_group, const double* points, int32_t* tours, int64_t max_iterations,
                         void* workspace, size_t workspace_bytes, int64_t* iterations_out, int64_t* exact_pairs_out,
                         void* stream) {
  ScreenedLayout lay;
  const int rc = screened_layout(n, groups, per_group, &lay);
  if (rc != DIFUSCO_OK) return rc;
  if (workspace_bytes < lay.total)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt_screened: workspace %zu < %zu bytes", workspace_bytes, lay.total);
  const int nblk = (n + TI - 1) / TI, nchunk = (n + SCH - 1) / SCH, batch = groups * per_group;
  const GroupedLayout gl = grouped_layout(n, groups, per_group);      // the arrays of difusco_tsp_two_opt_grouped
  char* base = (char*)workspace;
  double2* tp = (double2*)(base + gl.tp);
  double* dlen = (double*)(base + gl.dlen);
  Best* partial = (Best*)(base + gl.partial);
  Best* chosen = (Best*)(base + gl.chosen);
  int* gdone = (int*)(base + gl.gdone);
  long long* giters = (long long*)(base + gl.giters);
  TwoOptState* st = (TwoOptState*)(base + gl.st);
  float4* q = (float4*)(base + lay.q);
  float* d32 = (float*)(base + lay.d32);
  float* bmin = (float*)(base + lay.bmin);
  unsigned* tmin = (unsigned*)(base + lay.tmin);
  unsigned long long* gmax = (unsigned long long*)(base + lay.gmax);
  unsigned long long* counter = (unsigned long long*)(base + lay.counter);
  hipStream_t s = (hipStream_t)stream;
  hipError_t er = hipMemsetAsync(gdone, 0, (char*)st + sizeof(TwoOptState) - (char*)gdone, s);
  if (er == hipSuccess) er = hipMemsetAsync(gmax, 0, lay.total - lay.gmax, s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "memset: %s", hipGetErrorString(er));
  // M per group decides, once per call, whether the screen has a bound
  const int mblocks = (2 * n + 255) / 256 < 64 ? (2 * n + 255) / 256 : 64;
  hipLaunchKernelGGL(two_opt_maxabs_kernel, dim3(mblocks, groups), dim3(256), 0, s, points, 2 * n, gmax);
  std::vector<double> maxabs(groups);
  er = hipMemcpyAsync(maxabs.data(), gmax, sizeof(double) * groups, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "two_opt_screened max |coordinate|: %s", hipGetErrorString(er));
  bool bounded = true;
  for (int g = 0; g < groups; ++g) {
    double eps = 0.0;
    bounded = bounded && difusco_tsp_two_opt_screen_bound(maxabs[g], &eps) == 1;
  }
  if (!bounded) {                                              // no bound: the exact sweep, every pair in float64
    const int rc2 = difusco_tsp_two_opt_grouped(n, groups, per_group, points, tours, max_iterations, workspace, workspace_bytes,
                                                iterations_out, stream);
    if (rc2 == DIFUSCO_OK && exact_pairs_out) {
      long long sweeps = 0;
      for (int g = 0; g < groups; ++g) sweeps += evaluations(iterations_out[g], max_iterations);
      *exact_pairs_out = sweeps * per_group * ((long long)(n - 1) * (n - 2) / 2);
    }
    return rc2;
  }
  TwoOptState host{0, 0, 0};
  const int poll = 8;
  const long long loops = max_iterations > 0 ? max_iterations : 1;   // as difusco_tsp_two_opt
  for (long long it = 0; it < loops; ++it) {
    hipLaunchKernelGGL(two_opt_prep_screen_kernel, dim3((n + 1 + 255) / 256, batch), dim3(256), 0, s, points, tours, n, tp, dlen,
                       q, d32, tmin, gdone, per_group);
    hipLaunchKernelGGL(two_opt_screen_kernel, dim3(nblk, nchunk, batch), dim3(256), 0, s, q, d32, n, bmin, tmin, gdone, per_group);
    hipLaunchKernelGGL(two_opt_screened_best_kernel, dim3(nblk, batch), dim3(256), 0, s, tp, dlen, q, d32, n, nchunk, bmin, tmin,
                       (const double*)gmax, partial, counter, gdone, per_group);
    hipLaunchKernelGGL(two_opt_apply_grouped_kernel, dim3(groups), dim3(256), 0, s, tours, n, per_group, nblk, partial,
                       (long long)max_iterations, st, gdone, giters, chosen);
    if ((it + 1) % poll == 0 || it + 1 == loops) {
      er = hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s);
      if (er == hipSuccess) er = hipStreamSynchronize(s);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "two_opt state: %s", hipGetErrorString(er));
      if (host.done >= groups) break;
    }
  }
  unsigned long long pairs = 0;
  er = hipMemcpyAsync(iterations_out, giters, sizeof(long long) * groups, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipMemcpyAsync(&pairs, counter, sizeof(pairs), hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "two_opt_screened iterations: %s", hipGetErrorString(er));
  if (exact_pairs_out) *exact_pairs_out = (int64_t)pairs;
  return DIFUSCO_OK;
}

// ---- ragged 2-opt (difusco_tsp_two_opt_ragged): groups of different n in one launch sequence ---------------------------------
//
// The same move as the grouped entries (prep, best or screen + screened best, apply with one block per group), with every
// kernel reading its tour's n and array bases from a descriptor table instead of computing them from one n.  The table is built
// on the host from group_n / group_tours and written to the workspace once per call.  A block reads desc[its tour], an index that
// is uniform over the block, so the descriptor and every base derived from it stay in scalar registers and the row data of the
// screen still arrive by scalar loads.
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
  int first, count;        // its tours: desc[first .. first + count - 1], all of n nodes and nblk partials,
  int n, nblk;
  long long points;
  long long tours, partial;   // so tour p of the group starts at tours + p (n + 1) and partial + p nblk: no descriptor per tour
};

__global__ void two_opt_prep_ragged_kernel(const double* __restrict__ points, const int* __restrict__ tours,
                                           const RaggedTour* __restrict__ desc, double2* __restrict__ tp, double* __restrict__ dlen,
                                           const int* __restrict__ tdone) {
  const RaggedTour d = desc[blockIdx.y];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > d.n || tdone[blockIdx.y]) return;
  prep_entry(points + d.points, tours + d.tours, d.n, k, tp + d.tp, dlen + d.cols);
}

__global__ __launch_bounds__(256) void two_opt_best_ragged_kernel(const double2* __restrict__ tp, const double* __restrict__ dlen,
                                                                  const RaggedTour* __restrict__ desc, Best* __restrict__ partial,
                                                                  const int* __restrict__ tdone) {
  const RaggedTour d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk || tdone[blockIdx.y]) return;
  const Best r = best_tile(tp + d.tp, dlen + d.cols, d.n, blockIdx.x * TI);
  if (threadIdx.x == 0) partial[d.partial + blockIdx.x] = r;
}

__global__ void two_opt_maxabs_ragged_kernel(const double* __restrict__ points, const RaggedGroup* __restrict__ grp,
                                             unsigned long long* __restrict__ gmax) {
  const RaggedGroup G = grp[blockIdx.y];
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

__global__ void two_opt_prep_screen_ragged_kernel(const double* __restrict__ points, const int* __restrict__ tours,
                                                  const RaggedTour* __restrict__ desc, double2* __restrict__ tp,
                                                  double* __restrict__ dlen, float4* __restrict__ q, float* __restrict__ d32,
                                                  unsigned* __restrict__ tmin, const int* __restrict__ tdone) {
  const RaggedTour d = desc[blockIdx.y];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > d.n || tdone[blockIdx.y]) return;
  if (k == 0) tmin[blockIdx.y] = f32_key(0.0f);
  prep_screen_entry(points + d.points, tours + d.tours, d.n, k, tp + d.tp, dlen + d.cols, q + d.cols, d32 + d.cols);
}

__global__ __launch_bounds__(256) void two_opt_screen_ragged_kernel(const float4* __restrict__ q, const float* __restrict__ d32,
                                                                    const RaggedTour* __restrict__ desc, float* __restrict__ bmin,
                                                                    unsigned* __restrict__ tmin, const int* __restrict__ tdone) {
  const RaggedTour d = desc[blockIdx.z];
  const int i0 = blockIdx.x * TI, jbase = blockIdx.y * SCH;
  if ((int)blockIdx.x >= d.nblk || (int)blockIdx.y >= d.nchunk) return;   // beyond the tour's own tiles
  if (jbase + SCH <= i0 + 2) return;                                       // the chunk lies left of the triangle
  if (tdone[blockIdx.z]) return;
  const float m = screen_tile(q + d.cols, d32 + d.cols, d.n, i0, jbase);
  if (threadIdx.x == 0) screen_publish(m, bmin + d.bmin + (long long)blockIdx.x * d.nchunk + blockIdx.y, tmin + blockIdx.z);
}

__global__ __launch_bounds__(256) void two_opt_screened_best_ragged_kernel(
    const double2* __restrict__ tp, const double* __restrict__ dlen, const float4* __restrict__ q, const float* __restrict__ d32,
    const RaggedTour* __restrict__ desc, const float* __restrict__ bmin, const unsigned* __restrict__ tmin,
    const double* __restrict__ gmax, Best* __restrict__ partial, unsigned long long* __restrict__ exact_pairs,
    const int* __restrict__ tdone) {
  const RaggedTour d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nblk || tdone[blockIdx.y]) return;
  screened_best_tile(tp + d.tp, dlen + d.cols, q + d.cols, d32 + d.cols, d.n, d.nchunk, blockIdx.x * TI,
                     bmin + d.bmin + (long long)blockIdx.x * d.nchunk, f32_unkey(tmin[blockIdx.y]), screen_eps(gmax[d.group]),
                     partial + d.partial + blockIdx.x, exact_pairs);
}

// two_opt_apply_grouped_kernel with the group's tours and their n from the tables.  A group that stops also sets tdone of its
// tours: the other kernels read their tour's flag by the block's own index, alongside the descriptor and not after it.
__global__ __launch_bounds__(256) void two_opt_apply_ragged_kernel(int* __restrict__ tours,
                                                                   const RaggedGroup* __restrict__ grp,
                                                                   const Best* __restrict__ partial, long long max_iterations,
                                                                   TwoOptState* st, int* __restrict__ gdone,
                                                                   int* __restrict__ tdone, long long* __restrict__ giters,
                                                                   Best* __restrict__ chosen) {
  const int g = blockIdx.x;
  if (gdone[g]) return;
  __shared__ double gmin;
  const RaggedGroup G = grp[g];
  auto stop = [&]() {                                          // thread 0
    gdone[g] = 1;
    for (int b = G.first; b < G.first + G.count; ++b) tdone[b] = 1;
    atomicAdd(&st->done, 1);
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
  if (!(gmin < -1e-6)) {
    if (threadIdx.x == 0) stop();
    return;
  }
  for (int p = 0; p < G.count; ++p) apply_move(tours + G.tours + (long long)p * (G.n + 1), chosen[G.first + p].idx, G.n);
  if (threadIdx.x == 0) {
    giters[g] += 1;
    if (giters[g] >= max_iterations) stop();
  }
}

struct RaggedLayout {      // byte offsets; the screen's arrays (q ..) only with method 1
  size_t desc, grp, tp, dlen, partial, chosen, gdone, tdone, giters, st, q, d32, bmin, tmin, gmax, counter, total;
  int tours, nmax, nblk_max, nchunk_max;
};

constexpr int kRaggedMaxTours = 65535;             // a grid dimension
constexpr int kRaggedMaxNodes = 65535 * TI;

// checks the host arrays and lays the workspace out; `tab` / `gtab` (optional) receive the tables
int ragged_layout(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, int method, RaggedLayout* L,
                  std::vector<RaggedTour>* tab, std::vector<RaggedGroup>* gtab) {
  if (groups < 1) return set_error(DIFUSCO_EINVAL, "%s: groups = %d, needs at least 1", who, groups);
  if (!group_n || !group_tours) return set_error(DIFUSCO_EINVAL, "%s: group_n / group_tours is null", who);
  if (method != 0 && method != 1) return set_error(DIFUSCO_EINVAL, "%s: method %d (0 exact, 1 screened)", who, method);
  long long T = 0;
  for (int g = 0; g < groups; ++g) {
    if (group_n[g] < 4) return set_error(DIFUSCO_EINVAL, "%s: group %d has n = %d, needs n >= 4", who, g, group_n[g]);
    if (group_n[g] > kRaggedMaxNodes)
      return set_error(DIFUSCO_EINVAL, "%s: group %d has n = %d, at most %d nodes", who, g, group_n[g], kRaggedMaxNodes);
    if (group_tours[g] < 1) return set_error(DIFUSCO_EINVAL, "%s: group %d has %d tours, needs at least 1", who, g, group_tours[g]);
    T += group_tours[g];
    if (T > kRaggedMaxTours) return set_error(DIFUSCO_EINVAL, "%s: more than %d tours in one call", who, kRaggedMaxTours);
  }
  if (tab) tab->clear();
  if (gtab) gtab->clear();
  size_t points = 0, closed = 0, cols = 0, nblks = 0, tiles = 0;
  L->nmax = L->nblk_max = L->nchunk_max = 0;
  for (int g = 0; g < groups; ++g) {
    const int n = group_n[g], nblk = (n + TI - 1) / TI, nchunk = (n + SCH - 1) / SCH;
    L->nmax = n > L->nmax ? n : L->nmax;
    L->nblk_max = nblk > L->nblk_max ? nblk : L->nblk_max;
    L->nchunk_max = nchunk > L->nchunk_max ? nchunk : L->nchunk_max;
    if (gtab)
      gtab->push_back(RaggedGroup{(int)(tab ? tab->size() : 0), group_tours[g], n, nblk, (long long)points, (long long)closed,
                                  (long long)nblks});
    for (int p = 0; p < group_tours[g]; ++p) {
      if (tab)
        tab->push_back(RaggedTour{g, n, nblk, nchunk, (long long)points, (long long)closed, (long long)closed, (long long)cols,
                                  (long long)nblks, (long long)tiles});
      closed += (size_t)n + 1;
      cols += (size_t)n;
      nblks += (size_t)nblk;
      tiles += (size_t)nblk * nchunk;
    }
    points += 2 * (size_t)n;
  }
  L->tours = (int)T;
  size_t off = 0;
  auto take = [&off](size_t bytes) {
    const size_t at = off;
    off += up256(bytes);
    return at;
  };
  L->desc = take(sizeof(RaggedTour) * T);
  L->grp = take(sizeof(RaggedGroup) * groups);
  L->tp = take(sizeof(double2) * closed);
  L->dlen = take(sizeof(double) * cols);
  L->partial = take(sizeof(Best) * nblks);
  L->chosen = take(sizeof(Best) * T);
  L->gdone = take(sizeof(int) * groups);                       // gdone .. st are cleared by one memset
  L->tdone = take(sizeof(int) * T);
  L->giters = take(sizeof(long long) * groups);
  L->st = take(sizeof(TwoOptState));
  L->q = L->d32 = L->bmin = L->tmin = L->gmax = L->counter = off;
  if (method == 1) {
    L->q = take(sizeof(float4) * cols);
    L->d32 = take(sizeof(float) * cols);
    L->bmin = take(sizeof(float) * tiles);
    L->tmin = take(sizeof(unsigned) * T);
    L->gmax = take(sizeof(double) * groups);
    L->counter = take(sizeof(unsigned long long));
  }
  L->total = off;
  return DIFUSCO_OK;
}

}  // namespace
}  // namespace difusco

extern "C" {

int difusco_tsp_two_opt_workspace_bytes(int n_nodes, int batch, size_t* bytes) {
  using namespace difusco;
  if (!bytes || n_nodes < 4 || batch < 1) return set_error(DIFUSCO_EINVAL, "two_opt_workspace_bytes: bad arguments");
  const size_t nblk = (size_t)(n_nodes + TI - 1) / TI;
  *bytes = up256(sizeof(double2) * (size_t)batch * (n_nodes + 1)) + up256(sizeof(double) * (size_t)batch * n_nodes) +
           up256(sizeof(Best) * (size_t)batch * nblk) + up256(sizeof(Best) * (size_t)batch) + 256;
  return DIFUSCO_OK;
}

int difusco_tsp_two_opt(int n_nodes, int batch, const double* points, int32_t* tours, int64_t max_iterations,
                        void* workspace, size_t workspace_bytes, int64_t* iterations_out, void* stream) {
  using namespace difusco;
  if (n_nodes < 4 || batch < 1 || !points || !tours || !workspace || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt: needs n_nodes >= 4, batch >= 1 and non-null device arrays");
  size_t need = 0;
  difusco_tsp_two_opt_workspace_bytes(n_nodes, batch, &need);
  if (workspace_bytes < need) return set_error(DIFUSCO_EINVAL, "tsp_two_opt: workspace %zu < %zu bytes", workspace_bytes, need);
  const int n = n_nodes, nblk = (n + TI - 1) / TI;
  char* w = (char*)workspace;
  double2* tp = (double2*)w;
  w += up256(sizeof(double2) * (size_t)batch * (n + 1));
  double* dlen = (double*)w;
  w += up256(sizeof(double) * (size_t)batch * n);
  Best* partial = (Best*)w;
  w += up256(sizeof(Best) * (size_t)batch * nblk);
  Best* chosen = (Best*)w;
  w += up256(sizeof(Best) * (size_t)batch);
  TwoOptState* st = (TwoOptState*)w;
  hipStream_t s = (hipStream_t)stream;
  hipError_t er = hipMemsetAsync(st, 0, sizeof(TwoOptState), s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "memset: %s", hipGetErrorString(er));
  TwoOptState host{0, 0, 0};
  // the reference evaluates the moves once more after the last applied one and stops on `min_change >= -1e-6`;
  // at most max_iterations moves are applied (tsp_utils.py:20-47)
  const int poll = 8;
  const long long loops = max_iterations > 0 ? max_iterations : 1;   // the reference always evaluates (and may apply) once
  for (long long it = 0; it < loops; ++it) {
    hipLaunchKernelGGL(two_opt_prep_kernel<false>, dim3((n + 1 + 255) / 256, batch), dim3(256), 0, s, points, tours, n, batch,
                       tp, dlen, st, (const int*)nullptr, batch);
    hipLaunchKernelGGL(two_opt_best_kernel<false>, dim3(nblk, batch), dim3(256), 0, s, tp, dlen, n, partial, st,
                       (const int*)nullptr, batch);
    hipLaunchKernelGGL(two_opt_apply_kernel, dim3(1), dim3(256), 0, s, tours, n, batch, nblk, partial,
                       (long long)max_iterations, st, chosen);
    if ((it + 1) % poll == 0 || it + 1 == loops) {
      er = hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s);
      if (er == hipSuccess) er = hipStreamSynchronize(s);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "two_opt state: %s", hipGetErrorString(er));
      if (host.done) break;
    }
  }
  er = hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "two_opt state: %s", hipGetErrorString(er));
  if (iterations_out) *iterations_out = host.iterations;
  return DIFUSCO_OK;
}

int difusco_tsp_two_opt_grouped_workspace_bytes(int n_nodes, int groups, int per_group, size_t* bytes) {
  using namespace difusco;
  if (!bytes || n_nodes < 4 || groups < 1 || per_group < 1 || (long long)groups * per_group > (1 << 30))
    return set_error(DIFUSCO_EINVAL, "two_opt_grouped_workspace_bytes: bad arguments");
  *bytes = grouped_layout(n_nodes, groups, per_group).total;
  return DIFUSCO_OK;
}

int difusco_tsp_two_opt_grouped(int n_nodes, int groups, int per_group, const double* points, int32_t* tours,
                                int64_t max_iterations, void* workspace, size_t workspace_bytes, int64_t* iterations_out,
                                void* stream) {
  using namespace difusco;
  if (n_nodes < 4 || groups < 1 || per_group < 1 || (long long)groups * per_group > (1 << 30) || !points || !tours ||
      !workspace || !iterations_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt_grouped: needs n_nodes >= 4, groups, per_group >= 1, non-null device arrays "
                                     "and a host iterations_out[groups]");
  size_t need = 0;
  difusco_tsp_two_opt_grouped_workspace_bytes(n_nodes, groups, per_group, &need);
  if (workspace_bytes < need)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt_grouped: workspace %zu < %zu bytes", workspace_bytes, need);
  const int n = n_nodes, nblk = (n + TI - 1) / TI, batch = groups * per_group;
  const GroupedLayout gl = grouped_layout(n, groups, per_group);
  char* w = (char*)workspace;
  double2* tp = (double2*)(w + gl.tp);
  double* dlen = (double*)(w + gl.dlen);
  Best* partial = (Best*)(w + gl.partial);
  Best* chosen = (Best*)(w + gl.chosen);
  int* gdone = (int*)(w + gl.gdone);
  long long* giters = (long long*)(w + gl.giters);
  TwoOptState* st = (TwoOptState*)(w + gl.st);
  hipStream_t s = (hipStream_t)stream;
  hipError_t er = hipMemsetAsync(gdone, 0, (char*)st + sizeof(TwoOptState) - (char*)gdone, s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "memset: %s", hipGetErrorString(er));
  TwoOptState host{0, 0, 0};
  const int poll = 8;
  const long long loops = max_iterations > 0 ? max_iterations : 1;   // as difusco_tsp_two_opt
  for (long long it = 0; it < loops; ++it) {
    hipLaunchKernelGGL(two_opt_prep_kernel<true>, dim3((n + 1 + 255) / 256, batch), dim3(256), 0, s, points, tours, n, batch,
                       tp, dlen, st, gdone, per_group);
    hipLaunchKernelGGL(two_opt_best_kernel<true>, dim3(nblk, batch), dim3(256), 0, s, tp, dlen, n, partial, st, gdone,
                       per_group);
    hipLaunchKernelGGL(two_opt_apply_grouped_kernel, dim3(groups), dim3(256), 0, s, tours, n, per_group, nblk, partial,
                       (long long)max_iterations, st, gdone, giters, chosen);
    if ((it + 1) % poll == 0 || it + 1 == loops) {
      er = hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s);
      if (er == hipSuccess) er = hipStreamSynchronize(s);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "two_opt state: %s", hipGetErrorString(er));
      if (host.done >= groups) break;
    }
  }
  er = hipMemcpyAsync(iterations_out, giters, sizeof(long long) * groups, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "two_opt_grouped iterations: %s", hipGetErrorString(er));
  return DIFUSCO_OK;
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
  ScreenedLayout lay;
  const int rc = screened_layout(n_nodes, groups, per_group, &lay);
  if (rc == DIFUSCO_OK) *bytes = lay.total;
  return rc;
}

int difusco_tsp_two_opt_grouped_screened(int n_nodes, int groups, int per_group, const double* points, int32_t* tours,
                                         int64_t max_iterations, void* workspace, size_t workspace_bytes,
                                         int64_t* iterations_out, int64_t* exact_pairs_out, void* stream) {
  using namespace difusco;
  if (n_nodes < 4 || groups < 1 || per_group < 1 || (long long)groups * per_group > (1 << 30) || !points || !tours ||
      !workspace || !iterations_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt_grouped_screened: needs n_nodes >= 4, groups, per_group >= 1, non-null device "
                                     "arrays and a host iterations_out[groups]");
  return two_opt_screened_run(n_nodes, groups, per_group, points, tours, max_iterations, workspace, workspace_bytes,
                              iterations_out, exact_pairs_out, stream);
}

int difusco_tsp_two_opt_screened_workspace_bytes(int n_nodes, int batch, size_t* bytes) {
  using namespace difusco;
  if (!bytes || n_nodes < 4 || batch < 1) return set_error(DIFUSCO_EINVAL, "two_opt_screened_workspace_bytes: bad arguments");
  return difusco_tsp_two_opt_grouped_screened_workspace_bytes(n_nodes, 1, batch, bytes);
}

// one group of `batch` tours: difusco_tsp_two_opt_grouped with groups = 1 is difusco_tsp_two_opt
int difusco_tsp_two_opt_screened(int n_nodes, int batch, const double* points, int32_t* tours, int64_t max_iterations,
                                 void* workspace, size_t workspace_bytes, int64_t* iterations_out, int64_t* exact_pairs_out,
                                 void* stream) {
  using namespace difusco;
  if (n_nodes < 4 || batch < 1 || !points || !tours || !workspace || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt_screened: needs n_nodes >= 4, batch >= 1 and non-null device arrays");
  int64_t iterations = 0;
  const int rc = two_opt_screened_run(n_nodes, 1, batch, points, tours, max_iterations, workspace, workspace_bytes, &iterations,
                                      exact_pairs_out, stream);
  if (rc == DIFUSCO_OK && iterations_out) *iterations_out = iterations;
  return rc;
}

int difusco_tsp_two_opt_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int method,
                                               size_t* bytes) {
  using namespace difusco;
  if (!bytes) return set_error(DIFUSCO_EINVAL, "two_opt_ragged_workspace_bytes: bytes is null");
  RaggedLayout lay;
  const int rc = ragged_layout("two_opt_ragged_workspace_bytes", groups, group_n, group_tours, method, &lay, nullptr, nullptr);
  if (rc == DIFUSCO_OK) *bytes = lay.total;
  return rc;
}

int difusco_tsp_two_opt_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                               int32_t* tours, int64_t max_iterations, int method, void* workspace, size_t workspace_bytes,
                               int64_t* iterations_out, int64_t* exact_pairs_out, void* stream) {
  using namespace difusco;
  RaggedLayout lay;
  std::vector<RaggedTour> tab;
  std::vector<RaggedGroup> gtab;
  const int rc = ragged_layout("tsp_two_opt_ragged", groups, group_n, group_tours, method, &lay, &tab, &gtab);
  if (rc != DIFUSCO_OK) return rc;
  if (!points || !tours || !workspace || !iterations_out || max_iterations < 0)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt_ragged: needs non-null device arrays, a host iterations_out[groups] and "
                                     "max_iterations >= 0");
  if (workspace_bytes < lay.total)
    return set_error(DIFUSCO_EINVAL, "tsp_two_opt_ragged: workspace %zu < %zu bytes", workspace_bytes, lay.total);
  char* w = (char*)workspace;
  RaggedTour* desc = (RaggedTour*)(w + lay.desc);
  RaggedGroup* grp = (RaggedGroup*)(w + lay.grp);
  double2* tp = (double2*)(w + lay.tp);
  double* dlen = (double*)(w + lay.dlen);
  Best* partial = (Best*)(w + lay.partial);
  Best* chosen = (Best*)(w + lay.chosen);
  int* gdone = (int*)(w + lay.gdone);
  int* tdone = (int*)(w + lay.tdone);
  long long* giters = (long long*)(w + lay.giters);
  TwoOptState* st = (TwoOptState*)(w + lay.st);
  float4* q = (float4*)(w + lay.q);
  float* d32 = (float*)(w + lay.d32);
  float* bmin = (float*)(w + lay.bmin);
  unsigned* tmin = (unsigned*)(w + lay.tmin);
  unsigned long long* gmax = (unsigned long long*)(w + lay.gmax);
  unsigned long long* counter = (unsigned long long*)(w + lay.counter);
  hipStream_t s = (hipStream_t)stream;
  const int T = lay.tours;
  // the tables, once per call; the host vectors live until the synchronisation below
  hipError_t er = hipMemcpyAsync(desc, tab.data(), sizeof(RaggedTour) * T, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemcpyAsync(grp, gtab.data(), sizeof(RaggedGroup) * groups, hipMemcpyHostToDevice, s);
  if (er == hipSuccess) er = hipMemsetAsync(gdone, 0, (char*)st + sizeof(TwoOptState) - (char*)gdone, s);
  if (er == hipSuccess && method == 1) er = hipMemsetAsync(gmax, 0, lay.total - lay.gmax, s);
  bool screened = method == 1;
  if (er == hipSuccess && screened) {                          // M per group decides, once per call, whether the screen has a bound
    const int mblocks = (2 * lay.nmax + 255) / 256 < 64 ? (2 * lay.nmax + 255) / 256 : 64;
    hipLaunchKernelGGL(two_opt_maxabs_ragged_kernel, dim3(mblocks, groups), dim3(256), 0, s, points, grp, gmax);
    std::vector<double> maxabs(groups);
    er = hipMemcpyAsync(maxabs.data(), gmax, sizeof(double) * groups, hipMemcpyDeviceToHost, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    for (int g = 0; er == hipSuccess && g < groups; ++g) {
      double eps = 0.0;
      screened = screened && difusco_tsp_two_opt_screen_bound(maxabs[g], &eps) == 1;   // one group without a bound: exact sweep
    }
  } else if (er == hipSuccess) {
    er = hipStreamSynchronize(s);
  }
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "tsp_two_opt_ragged setup: %s", hipGetErrorString(er));
  TwoOptState host{0, 0, 0};
  const int poll = 8;
  const long long loops = max_iterations > 0 ? max_iterations : 1;   // as difusco_tsp_two_opt
  const dim3 prep_grid((lay.nmax + 1 + 255) / 256, T), best_grid(lay.nblk_max, T);
  for (long long it = 0; it < loops; ++it) {
    if (screened) {
      hipLaunchKernelGGL(two_opt_prep_screen_ragged_kernel, prep_grid, dim3(256), 0, s, points, tours, desc, tp, dlen, q, d32, tmin,
                         tdone);
      hipLaunchKernelGGL(two_opt_screen_ragged_kernel, dim3(lay.nblk_max, lay.nchunk_max, T), dim3(256), 0, s, q, d32, desc, bmin,
                         tmin, tdone);
      hipLaunchKernelGGL(two_opt_screened_best_ragged_kernel, best_grid, dim3(256), 0, s, tp, dlen, q, d32, desc, bmin, tmin,
                         (const double*)gmax, partial, counter, tdone);
    } else {
      hipLaunchKernelGGL(two_opt_prep_ragged_kernel, prep_grid, dim3(256), 0, s, points, tours, desc, tp, dlen, tdone);
      hipLaunchKernelGGL(two_opt_best_ragged_kernel, best_grid, dim3(256), 0, s, tp, dlen, desc, partial, tdone);
    }
    hipLaunchKernelGGL(two_opt_apply_ragged_kernel, dim3(groups), dim3(256), 0, s, tours, grp, partial,
                       (long long)max_iterations, st, gdone, tdone, giters, chosen);
    if ((it + 1) % poll == 0 || it + 1 == loops) {
      er = hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s);
      if (er == hipSuccess) er = hipStreamSynchronize(s);
      if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "two_opt state: %s", hipGetErrorString(er));
      if (host.done >= groups) break;
    }
  }
  unsigned long long pairs = 0;
  er = hipMemcpyAsync(iterations_out, giters, sizeof(long long) * groups, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess && screened) er = hipMemcpyAsync(&pairs, counter, sizeof(pairs), hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return set_error(DIFUSCO_EHIP, "tsp_two_opt_ragged iterations: %s", hipGetErrorString(er));
  if (!screened)                                               // every pair of every sweep that did work, in float64
    for (int g = 0; g < groups; ++g)
      pairs += (unsigned long long)(evaluations(iterations_out[g], max_iterations) * group_tours[g] *
                                    ((long long)(group_n[g] - 1) * (group_n[g] - 2) / 2));
  if (exact_pairs_out) *exact_pairs_out = (int64_t)pairs;
  return DIFUSCO_OK;
}

}  // extern "C"
