// What the resident tour searches (two_opt_resident.hip, local_search_resident.hip) share beside two_opt_common.h: the wave
// reduction of a best move and the split of a tour's 2-opt pairs over a team of whole waves.  Per translation unit (anonymous
// namespace), like two_opt_common.h.
#pragma once
#include <hip/hip_runtime.h>

#include "two_opt_common.h"

namespace difusco {
namespace {

constexpr int up4(int x) { return (x + 3) & ~3; }

__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const Best o{__shfl_xor(b.v, off, 64), __shfl_xor(b.idx, off, 64)};
    if (better(o.v, o.idx, b)) b = o;
  }
  return b;
}

// The split of a tour's pairs over a team: the pairs (i, j), j >= i + 2, in row-major order (row i holds the n - 2 - i pairs
// (i, i + 2 + q)); a thread takes the pairs first, first + step, ... of that order, step = the team size.  Consecutive threads
// then read consecutive columns and, mostly, one row.  work is false for a thread of a team without a tour.
struct Split {
  int first, step;
  bool work;
};

// f(i, j) for every pair of the thread: <= pairs / team size + 1 calls; the row search runs <= n turns over the whole sweep
template <class F>
__device__ __forceinline__ void for_pairs(int n, const Split& s, F f) {
  int i = 0, q = s.first, len = n - 2;
  for (;;) {
    while (len > 0 && q >= len) {
      q -= len;
      ++i;
      --len;
    }
    if (len <= 0) break;
    f(i, i + 2 + q);
    q += s.step;
  }
}

}  // namespace
}  // namespace difusco
