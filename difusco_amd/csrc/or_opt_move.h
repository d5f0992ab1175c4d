// What the launched local search (or_opt.hip) and the resident one (tsp_resident.hip) share beside two_opt_common.h: the
// Or-opt variants, the threshold, the phases of a group and the Or-opt move on one tour.  Per translation unit (anonymous
// namespace), like two_opt_common.h.
#pragma once
#include <hip/hip_runtime.h>

namespace difusco {
namespace {

constexpr int LMAX = 3;                    // longest segment
constexpr double kThreshold = -1e-6;       // the reference's 2-opt threshold (tsp_utils.py:39), for both moves

__device__ __forceinline__ int variant_len(int v) { return (v + 3) >> 1; }      // 1, 2, 2, 3, 3
__device__ __forceinline__ bool variant_rev(int v) { return v == 2 || v == 4; }

enum Phase : int { kTwoOpt = 0, kOrOpt = 1, kDone = 2 };

// the Or-opt move idx = (v n + i) n + j on one tour: the stretch between the segment and the insertion edge shifts by L places
// over the segment, so the affected positions are copied to `stage` (the tour's own n + 1 entries) and written back from there
__device__ __forceinline__ void apply_or_opt_move(int* __restrict__ tour, int* __restrict__ stage, long long idx, int n) {
  const long long nn = (long long)n * n;
  const int v = (int)(idx / nn), i = (int)(idx % nn / n), j = (int)(idx % n);
  const int L = variant_len(v);
  const bool rev = variant_rev(v);
  if (v > 4 || i + L > n - 1 || (j >= i && j <= i + L)) return;  // no candidate: nothing the sweep can return
  const int lo = (j < i ? j : i) + 1, hi = j < i ? i + L : j;    // 1 <= lo <= hi <= n - 1
  for (int k = lo + threadIdx.x; k <= hi; k += blockDim.x) stage[k] = tour[k];
  __syncthreads();
  for (int k = lo + threadIdx.x; k <= hi; k += blockDim.x) {
    int src;
    if (j > i) {                                                 // tour[:i+1] + tour[i+L+1 : j+1] + seg + tour[j+1:]
      const int s = k - (j - L + 1);
      src = s < 0 ? k + L : (rev ? i + L - s : i + 1 + s);
    } else {                                                     // tour[:j+1] + seg + tour[j+1 : i+1] + tour[i+L+1:]
      const int s = k - (j + 1);
      src = s < L ? (rev ? i + L - s : i + 1 + s) : k - L;
    }
    tour[k] = stage[src];
  }
}

}  // namespace
}  // namespace difusco
