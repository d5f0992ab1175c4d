// What the 2-opt entries (two_opt.hip), the resident searches (tsp_resident.hip) and the local search (or_opt.hip) share: the
// float64 distance and pair change, the float32 pair change of the screen and its bound, the (min, first flat
// index) reductions, the prep entry, one block of the exact 2-opt sweep and the segment reversal; and the check of the group
// arrays that every _ragged tour entry starts with.  Every function is
// per translation unit (anonymous namespace): the kernels that use them are compiled where they are launched.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/difusco_hip.h"
#include "kernels.h"

namespace difusco {
namespace {

// float64 distance exactly as torch evaluates sqrt(sum((p - q) ** 2, -1)): two products, one sum, no fused multiply-add
__device__ __forceinline__ double dist2d(double dx, double dy) { return sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy))); }

struct Best {
  double v;
  long long idx;
};

__device__ __forceinline__ bool better(double v, long long idx, const Best& b) { return v < b.v || (v == b.v && idx < b.idx); }

// entry k of one tour's tp / dlen (pointers at the tour's own arrays, `points` at its group's coordinates)
__device__ __forceinline__ void prep_entry(const double* __restrict__ points, const int* __restrict__ tour, int n, int k,
                                           double2* __restrict__ tp, double* __restrict__ dlen) {
  const int c = tour[k];
  const double2 p = make_double2(points[2 * c], points[2 * c + 1]);
  tp[k] = p;
  if (k < n) {
    const int c1 = tour[k + 1];
    const double dx = p.x - points[2 * c1], dy = p.y - points[2 * c1 + 1];
    dlen[k] = dist2d(dx, dy);                                   // A_i,i+1 (tsp_utils.py:28)
  }
}

// one pair's change A_ij + A_i+1,j+1 - A_i,i+1 - A_j,j+1, evaluated left to right (tsp_utils.py:31) as best_tile evaluates it:
// a = P_i, a1 = P_i+1, pj = P_j, pj1 = P_j+1, d_i and d_j their dlen
__device__ __forceinline__ double change64(double2 a, double2 a1, double2 pj, double2 pj1, double d_i, double d_j) {
  const double x0 = a.x - pj.x, y0 = a.y - pj.y;
  const double x1 = a1.x - pj1.x, y1 = a1.y - pj1.y;
  return __dsub_rn(__dsub_rn(__dadd_rn(dist2d(x0, y0), dist2d(x1, y1)), d_i), d_j);
}

// ---- the float32 screen of a pair (the bound is derived in two_opt.hip): |c32 - c64| <= eps(M) = 96 * 2^-24 * M for
// 2^-32 <= M <= 2^60, M = the largest |coordinate| of the instance; outside that range, or with a non-finite M, no bound.
constexpr double kScreenEpsPerM = 0x1.8p-18;       // 96 * 2^-24
constexpr double kScreenMinM = 0x1p-32, kScreenMaxM = 0x1p60;

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

constexpr int TI = 16;     // rows per block
constexpr int JPT = 4;     // columns per thread per sweep (256 threads x 4 = 1024 columns per sweep)

// (min, first flat index) over the 256 threads of a block; the result is valid in thread 0
__device__ __forceinline__ Best block_best(Best best) {
  __shared__ Best red[256];
  red[threadIdx.x] = best;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s && better(red[threadIdx.x + s].v, red[threadIdx.x + s].idx, red[threadIdx.x])) red[threadIdx.x] = red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// one block of the exact sweep: rows i0 .. i0 + TI - 1 of the tour (P = its tp, D = its dlen, n nodes) against all their columns;
// returns the block's best move in thread 0.  The flat index is i * n + j with the tour's own n.
__device__ __forceinline__ Best best_tile(const double2* __restrict__ P, const double* __restrict__ D, int n, int i0) {
  __shared__ double2 pi[TI + 1];
  __shared__ double di[TI];
  for (int t = threadIdx.x; t <= TI; t += blockDim.x)
    if (i0 + t <= n) pi[t] = P[i0 + t];
  for (int t = threadIdx.x; t < TI; t += blockDim.x)
    if (i0 + t < n) di[t] = D[i0 + t];
  __syncthreads();
  Best best{0.0, 0};
  const int rows = (n - i0) < TI ? (n - i0) : TI;
  // columns j >= i0 + 2 matter for this tile; sweep them in chunks of 256 * JPT
  for (int jbase = i0 + 2; jbase < n; jbase += 256 * JPT) {
    double2 pj[JPT], pj1[JPT];
    double dj[JPT];
    int jj[JPT];
#pragma unroll
    for (int u = 0; u < JPT; ++u) {
      const int j = jbase + u * 256 + threadIdx.x;
      jj[u] = j;
      if (j < n) {
        pj[u] = P[j];
        pj1[u] = P[j + 1];
        dj[u] = D[j];
      }
    }
    for (int r = 0; r < rows; ++r) {
      const int i = i0 + r;
      const double2 a = pi[r], a1 = pi[r + 1];
      const double d_i = di[r];
#pragma unroll
      for (int u = 0; u < JPT; ++u) {
        const int j = jj[u];
        if (j < n && j >= i + 2) {
          const double x0 = a.x - pj[u].x, y0 = a.y - pj[u].y;
          const double x1 = a1.x - pj1[u].x, y1 = a1.y - pj1[u].y;
          // change = A_ij + A_i+1,j+1 - A_i,i+1 - A_j,j+1, evaluated left to right (tsp_utils.py:31)
          const double change = __dsub_rn(__dsub_rn(__dadd_rn(dist2d(x0, y0), dist2d(x1, y1)), d_i), dj[u]);
          const long long idx = (long long)i * n + j;
          if (better(change, idx, best)) best = Best{change, idx};
        }
      }
    }
  }
  return block_best(best);                                      // min value, then lowest flat index
}

// the apply kernels' steps on one tour: argmin over its partials (valid in thread 0) ...
__device__ __forceinline__ Best tour_argmin(const Best* __restrict__ part, int nblk) {
  Best best{0.0, 0};
  for (int t = threadIdx.x; t < nblk; t += blockDim.x) {
    const Best c = part[t];
    if (better(c.v, c.idx, best)) best = c;
  }
  return block_best(best);
}

// ... and its best move: tour[mi+1 .. mj] reversed (tsp_utils.py:41), idx = mi * n + mj
__device__ __forceinline__ void apply_move(int* __restrict__ tour, long long idx, int n) {
  const int mi = (int)(idx / n), mj = (int)(idx % n);
  const int len = mj - mi;
  for (int t = threadIdx.x; t < len / 2; t += blockDim.x) {
    const int x = mi + 1 + t, y = mj - t;
    const int tmp = tour[x];
    tour[x] = tour[y];
    tour[y] = tmp;
  }
}

size_t up256(size_t x) { return (x + 255) / 256 * 256; }

constexpr int kMaxTours = 65535;                   // a grid dimension
constexpr int kMaxNodes = 65535 * TI;              // and as many row tiles

// the group arrays of a _ragged entry (`who` for the message): DIFUSCO_OK and the tours of the call, or the refusal
int check_groups(const char* who, int groups, const int32_t* group_n, const int32_t* group_tours, int* tours) {
  if (groups < 1) return set_error(DIFUSCO_EINVAL, "%s: groups = %d, needs at least 1", who, groups);
  if (!group_n || !group_tours) return set_error(DIFUSCO_EINVAL, "%s: group_n / group_tours is null", who);
  long long T = 0;
  for (int g = 0; g < groups; ++g) {
    if (group_n[g] < 4) return set_error(DIFUSCO_EINVAL, "%s: group %d has n = %d, needs n >= 4", who, g, group_n[g]);
    if (group_n[g] > kMaxNodes)
      return set_error(DIFUSCO_EINVAL, "%s: group %d has n = %d, at most %d nodes", who, g, group_n[g], kMaxNodes);
    if (group_tours[g] < 1) return set_error(DIFUSCO_EINVAL, "%s: group %d has %d tours, needs at least 1", who, g, group_tours[g]);
    T += group_tours[g];
    if (T > kMaxTours) return set_error(DIFUSCO_EINVAL, "%s: more than %d tours in one call", who, kMaxTours);
  }
  *tours = (int)T;
  return DIFUSCO_OK;
}

}  // namespace
}  // namespace difusco
