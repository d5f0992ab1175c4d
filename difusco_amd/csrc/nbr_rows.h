// The neighbour stage of the neighbour-list searches (two_opt_multi.hip, or_opt_nbr.h), once: a row of a sweep evaluates only
// its CANDIDATE columns - the moves one of whose new edges joins a city to one of its listed neighbours, in either direction.
//   nbr_reset_row   entry k of a tour in front of a sweep: pos[city] = its position, rowkey = no key, rowj = -1;
//   nbr_walk        thread (position p, list slot s) of a tour: x = tour[p], y = its s-th listed city, q = pos[y]; the 2-opt pairs
//                   (nbr_pairs) or the Or-opt candidates (or_nbr_candidates) of the two positions go to a visitor f(row, code,
//                   value).  A candidate's row is not the thread's own, so the threads combine, in two launches:
//   nbr_row_value   a value below the threshold does a 64-bit atomic min of its ordered bits on rowkey[row]; the others are
//                   dropped at once: such a row does not propose;
//   nbr_row_col     the same walk again: a candidate whose value equals rowkey[row] writes rowv[row] (every such thread writes
//                   the same bits) and does a 32-bit unsigned atomic min of its code - j, Or-opt: v n + j - on rowj[row].  The row
//                   ends with its lowest (value, code) whatever the order of the threads; nobody waits for anybody.
// The __global__ kernels stay in the files: they read their own state, return early for a tour that is not in its neighbour
// stage, and call these with the tour's descriptor.  Pads (list entries outside 0 .. n-1 or equal to the city) are tested before
// anything is indexed with them.  Every function is per translation unit (anonymous namespace), as in multi_move_common.h.
#pragma once
#include <hip/hip_runtime.h>

#include "multi_move_common.h"
#include "or_opt_rows.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

__device__ __forceinline__ void nbr_reset_row(const TourDesc& d, const int* __restrict__ tours, int k, int* __restrict__ pos,
                                              unsigned long long* __restrict__ rowkey, int* __restrict__ rowj) {
  pos[d.cols + tours[d.closed + k]] = k;                         // a tour is a permutation of 0 .. n-1 (the entries' convention)
  rowkey[d.cols + k] = kNoKey;
  rowj[d.cols + k] = -1;
}

// The up to two 2-opt pairs of (position p, listed city at position q) and their changes.  f(i, j, change) is called for every
// valid pair: 0 <= i, i + 2 <= j <= n - 1 (hence i <= n - 3).
template <class F>
__device__ __forceinline__ void nbr_pairs(const double2* __restrict__ P, const double* __restrict__ D, int n, int p, int q, F f) {
  {                                                              // head: tour[i] and tour[j] are the two cities
    const int i = p < q ? p : q, j = p < q ? q : p;
    if (j >= i + 2) f(i, j, change64(P[i], P[i + 1], P[j], P[j + 1], D[i], D[j]));
  }
  {                                                              // tail: tour[i+1] and tour[j+1]; position 0 is also position n
    const int pp = p == 0 ? n : p, qq = q == 0 ? n : q;
    const int i = (pp < qq ? pp : qq) - 1, j = (pp < qq ? qq : pp) - 1;      // 0 <= i, j <= n - 1
    if (j >= i + 2) f(i, j, change64(P[i], P[i + 1], P[j], P[j + 1], D[i], D[j]));
  }
}

// The Or-opt candidates of (position p, listed city at position q): each of the two cities is the segment end, at position e, and
// the other the anchor.  As `a` (the end joined to tour[j]) the end gives j = the anchor's position; as `b` (the end joined to
// tour[j+1]) it gives j = the anchor's position minus 1, position 0 read as n.  The end is the segment's first city (i = e - 1)
// or its last (i = e - L), by variant and orientation.  f(i, v n + j, delta) is called for every valid candidate: 0 <= i <=
// n - 1 - L (hence 1 <= e <= n - 1: position 0 never moves), j outside [i, i + L]; 0 <= j <= n - 1 holds by construction.  The
// bounds are tested before or_candidate_delta reads a point.
template <class F>
__device__ __forceinline__ void or_nbr_candidates(const double2* __restrict__ P, const double* __restrict__ D, int n, int p, int q,
                                                  F f) {
#pragma unroll
  for (int role = 0; role < 2; ++role) {
    const int e = role ? q : p, anchor = role ? p : q;
    const int ja = anchor, jb = (anchor == 0 ? n : anchor) - 1;
#pragma unroll
    for (int v = 0; v < 5; ++v) {
      const int L = variant_len(v);
      const bool rev = variant_rev(v);
      const int ia = rev ? e - L : e - 1, ib = rev ? e - 1 : e - L;   // the end as a, as b
      if (ia >= 0 && ia <= n - 1 - L && (ja < ia || ja > ia + L)) f(ia, v * n + ja, or_candidate_delta(P, D, v, ia, ja));
      if (ib >= 0 && ib <= n - 1 - L && (jb < ib || jb > ib + L)) f(ib, v * n + jb, or_candidate_delta(P, D, v, ib, jb));
    }
  }
}

// thread (p, s) of tour d, blockIdx.x * blockDim.x + threadIdx.x = p K + s; or_opt: the Or-opt candidates, else the 2-opt pairs
template <class F>
__device__ __forceinline__ void nbr_walk(const TourDesc& d, bool or_opt, const int* __restrict__ tours,
                                         const int* __restrict__ neighbors, const double2* __restrict__ tp,
                                         const double* __restrict__ dlen, const int* __restrict__ pos, int K, F f) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)d.n * K) return;
  const int p = (int)(e / K), slot = (int)(e % K);
  const int x = tours[d.closed + p];
  const int y = neighbors[(d.points >> 1) * K + (long long)x * K + slot];   // the group's lists start at (cities before it) K
  if (y < 0 || y >= d.n || y == x) return;                       // a pad: nothing is indexed with it
  const int q = pos[d.cols + y];
  if (or_opt)
    or_nbr_candidates(tp + d.closed, dlen + d.cols, d.n, p, q, f);
  else
    nbr_pairs(tp + d.closed, dlen + d.cols, d.n, p, q, f);
}

__device__ __forceinline__ void nbr_row_value(const TourDesc& d, bool or_opt, const int* __restrict__ tours,
                                              const int* __restrict__ neighbors, const double2* __restrict__ tp,
                                              const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                              unsigned long long* __restrict__ rowkey) {
  unsigned long long* keys = rowkey + d.cols;
  nbr_walk(d, or_opt, tours, neighbors, tp, dlen, pos, K, [keys](int i, int, double value) {
    if (value < kThreshold) atomicMin(&keys[i], ordered_bits(value));
  });
}

__device__ __forceinline__ void nbr_row_col(const TourDesc& d, bool or_opt, const int* __restrict__ tours,
                                            const int* __restrict__ neighbors, const double2* __restrict__ tp,
                                            const double* __restrict__ dlen, const int* __restrict__ pos, int K,
                                            const unsigned long long* __restrict__ rowkey, double* __restrict__ rowv,
                                            int* __restrict__ rowj) {
  const unsigned long long* keys = rowkey + d.cols;
  double* vals = rowv + d.cols;
  unsigned* codes = (unsigned*)(rowj + d.cols);                  // -1 is the highest unsigned: no column yet; 5 n fits 32 bits
  nbr_walk(d, or_opt, tours, neighbors, tp, dlen, pos, K, [keys, vals, codes](int i, int code, double value) {
    if (value < kThreshold && ordered_bits(value) == keys[i]) {
      vals[i] = value;
      atomicMin(&codes[i], (unsigned)code);
    }
  });
}

}  // namespace
}  // namespace difusco
