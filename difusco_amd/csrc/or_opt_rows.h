// What the Or-opt sweeps of the multi-move searches share (or_opt_multi.hip with or_opt_focused.h and or_opt_nbr.h): the delta of a
// candidate, in one place, the full row-best loop and the delta of a single candidate (v, i, j).  Every function is per translation
// unit (anonymous namespace), as in multi_move_common.h.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "multi_move_common.h"
#include "two_opt_common.h"

namespace difusco {
namespace {

constexpr int LMAX = 3;                    // longest segment

// delta = ((|P_i P_i+L+1| + |P_j a|) + |b P_j+1|) - ((d_i + d_i+L) + d_j), every operation rounded on its own: c = the closing
// edge, e = |P_j a|, f = |b P_j+1|, rem = or_removed(d_i + d_i+L, d_j), which the variants of one length share
__device__ __forceinline__ double or_removed(double r, double dj) { return __dadd_rn(r, dj); }
__device__ __forceinline__ double or_delta(double c, double e, double f, double rem) {
  return __dsub_rn(__dadd_rn(__dadd_rn(c, e), f), rem);
}

// the delta of the single candidate (v, i, j) of a tour (P = its tp, n + 1 entries; D = its dlen): 0 <= i <= n - 1 - L,
// 0 <= j <= n - 1, j outside [i, i + L] - the caller has tested that, so every index is at most n
__device__ __forceinline__ double or_candidate_delta(const double2* __restrict__ P, const double* __restrict__ D, int v, int i,
                                                     int j) {
  const int L = variant_len(v);
  const bool rev = variant_rev(v);
  const double2 p = P[i], q = P[i + L + 1], a = P[rev ? i + L : i + 1], b = P[rev ? i + 1 : i + L], pj = P[j], pj1 = P[j + 1];
  return or_delta(dist2d(p.x - q.x, p.y - q.y), dist2d(pj.x - a.x, pj.y - a.y), dist2d(pj1.x - b.x, pj1.y - b.y),
                  or_removed(__dadd_rn(D[i], D[i + L]), D[j]));
}

// one block of the Or-opt row-best sweep: rows i0 .. i0 + TI - 1 of the tour (P = its tp, D = its dlen, n nodes) against every
// column.  Row i <= n - 2 gets its lowest delta in rowv[i], ties to the lowest v and then the lowest j; rowj[i] = v n + j of
// that candidate, or -1 if the delta is not below the threshold.
__device__ __forceinline__ void or_row_best_tile(const double2* __restrict__ P, const double* __restrict__ D, int n, int i0,
                                                 double* __restrict__ rowv, int* __restrict__ rowj) {
  __shared__ double2 pr[TI + LMAX + 1];    // P_i0 .. P_i0+TI+3, the index clipped to n
  __shared__ double closing[LMAX][TI];     // |P_i P_i+L+1|
  __shared__ double removed[LMAX][TI];     // d_i + d_i+L
  __shared__ double redv[4][TI];
  __shared__ int redc[4][TI];
  for (int t = threadIdx.x; t < TI + LMAX + 1; t += blockDim.x) pr[t] = P[i0 + t < n ? i0 + t : n];
  for (int t = threadIdx.x; t < LMAX * TI; t += blockDim.x) {
    const int r = t % TI, L = t / TI + 1, i = i0 + r;
    double c = 0.0, d = 0.0;
    if (i <= n - 1 - L) {
      const double2 p = P[i], q = P[i + L + 1];
      c = dist2d(p.x - q.x, p.y - q.y);
      d = __dadd_rn(D[i], D[i + L]);
    }
    closing[L - 1][r] = c;
    removed[L - 1][r] = d;
  }
  __syncthreads();
  double bv[TI];
  int bc[TI];                              // v n + j: the order of (v, j)
#pragma unroll
  for (int r = 0; r < TI; ++r) bv[r] = 0.0, bc[r] = INT_MAX;
  for (int jbase = 0; jbase < n; jbase += 256 * JPT) {
    double2 pj[JPT], pj1[JPT];
    double dj[JPT], e1[JPT], e2[JPT], e3[JPT], f1[JPT], f2[JPT], f3[JPT];   // e_k = |P_j P_i+k|, f_k = |P_j+1 P_i+k|
    int jj[JPT];
#pragma unroll
    for (int u = 0; u < JPT; ++u) {
      const int j = jbase + u * 256 + threadIdx.x, jc = j < n ? j : n - 1;
      jj[u] = j;
      pj[u] = P[jc];
      pj1[u] = P[jc + 1];
      dj[u] = D[jc];
      e1[u] = dist2d(pj[u].x - pr[1].x, pj[u].y - pr[1].y);
      e2[u] = dist2d(pj[u].x - pr[2].x, pj[u].y - pr[2].y);
      e3[u] = dist2d(pj[u].x - pr[3].x, pj[u].y - pr[3].y);
      f1[u] = dist2d(pj1[u].x - pr[1].x, pj1[u].y - pr[1].y);
      f2[u] = dist2d(pj1[u].x - pr[2].x, pj1[u].y - pr[2].y);
      f3[u] = dist2d(pj1[u].x - pr[3].x, pj1[u].y - pr[3].y);
    }
#pragma unroll
    for (int r = 0; r < TI; ++r) {
      const int i = i0 + r;
      const double c1 = closing[0][r], c2 = closing[1][r], c3 = closing[2][r];
      const double r1 = removed[0][r], r2 = removed[1][r], r3 = removed[2][r];
      const double2 next = pr[r + LMAX + 1];                    // P_i+4, for the row after this one
      const bool row1 = i <= n - 2, row2 = i <= n - 3, row3 = i <= n - 4;
#pragma unroll
      for (int u = 0; u < JPT; ++u) {
        const int j = jj[u];
        const double rem1 = or_removed(r1, dj[u]), rem2 = or_removed(r2, dj[u]), rem3 = or_removed(r3, dj[u]);
        const double d0 = or_delta(c1, e1[u], f1[u], rem1);
        const double d1 = or_delta(c2, e1[u], f2[u], rem2);
        const double d2 = or_delta(c2, e2[u], f1[u], rem2);
        const double d3 = or_delta(c3, e1[u], f3[u], rem3);
        const double d4 = or_delta(c3, e3[u], f1[u], rem3);
        const bool in = j < n, left = j < i;
        const bool ok1 = in && row1 && (left || j > i + 1), ok2 = in && row2 && (left || j > i + 2),
                   ok3 = in && row3 && (left || j > i + 3);
        // the lowest delta of the pair's variants, the lowest v on a tie
        double m = ok1 ? d0 : INFINITY;
        int v = 0;
        if (ok2 && d1 < m) m = d1, v = 1;
        if (ok2 && d2 < m) m = d2, v = 2;
        if (ok3 && d3 < m) m = d3, v = 3;
        if (ok3 && d4 < m) m = d4, v = 4;
        const int code = v * n + j;
        if (better_col(m, code, bv[r], bc[r])) bv[r] = m, bc[r] = code;
        e1[u] = e2[u];
        e2[u] = e3[u];
        e3[u] = dist2d(pj[u].x - next.x, pj[u].y - next.y);
        f1[u] = f2[u];
        f2[u] = f3[u];
        f3[u] = dist2d(pj1[u].x - next.x, pj1[u].y - next.y);
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < TI; ++r) {
    double v = bv[r];
    int c = bc[r];
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_down(v, off);
      const int oc = __shfl_down(c, off);
      if (better_col(ov, oc, v, c)) v = ov, c = oc;
    }
    if (lane == 0) redv[wave][r] = v, redc[wave][r] = c;
  }
  __syncthreads();
  if (threadIdx.x < TI && i0 + (int)threadIdx.x <= n - 2) {
    const int r = threadIdx.x;
    double v = redv[0][r];
    int c = redc[0][r];
    for (int w = 1; w < 4; ++w)
      if (better_col(redv[w][r], redc[w][r], v, c)) v = redv[w][r], c = redc[w][r];
    rowv[i0 + r] = v;
    rowj[i0 + r] = v < kThreshold ? c : -1;                      // below the threshold c is the code of a candidate
  }
}

}  // namespace
}  // namespace difusco
