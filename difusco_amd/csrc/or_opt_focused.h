// The focused search (difusco_tsp_focused_search_ragged): the iterated search of or_opt_multi.hip whose descents after a kick
// evaluate only candidates next to a marked edge.  Included by or_opt_multi.hip behind its kernels, whose types and device
// functions it uses (the kick itself is kick_draws / kick_swaps there), and in front of its host side, which lays out the focus
// state and launches the kernels here (mls_layout, mls_run); the rule is stated in include/difusco_hip.h and restated in numpy in
// tests/tsp_focused_search_emulation.py.
//
// A tour is in one of three modes: kFull (its first descent), kFocused (a descent after a kick) and kClosing (the full descent
// that closes the call).  A launch sequence is five launches, whatever the modes of the tours:
//   mls_prep_kernel               as it is;
//   mls_row_best_kernel           as it is, on a copy of the phase words in which a focused tour reads kDone: a no-op for it;
//   mls_focused_row_best_kernel   a no-op for a tour that is not focused.  Row part: a block takes one entry of the tour's list of
//                                 active rows against all columns (lists are short).  Column part: a block takes a tile of TI
//                                 consecutive rows against the list of active columns, and skips the rows that are in the row
//                                 list.  So every row's best is complete in one block.  The arithmetic is row_best_tile's and
//                                 or_row_best_tile's; the Or-opt form recomputes |P_j P_i+k| and |P_j+1 P_i+k| for every (i, j);
//   mls_select_focused_kernel     one block per tour.  Not focused: the select step of the iterated search.  Focused: the
//                                 selection - one proposal per thread in LDS if there are at most compact_select_max of them
//                                 (select_compact), else select_disjoint -, the marks S and T from the tour before the moves,
//                                 the moves, S := T at a switch of phase, and the two lists of the next sweep (focus_rebuild);
//   mls_keep_kick_focused_kernel  mls_keep_kick_kernel plus T, S and the lists after a kick, and the closing descent.
#pragma once

namespace difusco {
namespace {

constexpr int kCompactMax = 1024;          // proposals the compact selection holds: one per thread

enum FocusMode : int { kFull = 0, kFocused = 1, kClosing = 2 };

struct MlFocus {           // device-resident state of a tour of the focused search, zero at the start of a call
  int mode;
  int nrows, ncols;        // the lengths of the tour's lists of active rows / columns
  int closing_sweeps;      // sweeps in which the closing descent moved the tour
};

// the lowest delta of the Or-opt candidates (v, i, j), v = 0 .. 4, the lowest v on a tie, and v n + j: the inner step of
// or_row_best_tile with q_k = P_i+k, c_L = |P_i P_i+L+1| and r_L = d_i + d_i+L
__device__ __forceinline__ void or_pair_best(double2 q1, double2 q2, double2 q3, double c1, double c2, double c3, double r1,
                                             double r2, double r3, int i, int n, int j, double2 pj, double2 pj1, double dj,
                                             double* best, int* code) {
  const double e1 = dist2d(pj.x - q1.x, pj.y - q1.y), e2 = dist2d(pj.x - q2.x, pj.y - q2.y), e3 = dist2d(pj.x - q3.x, pj.y - q3.y);
  const double f1 = dist2d(pj1.x - q1.x, pj1.y - q1.y), f2 = dist2d(pj1.x - q2.x, pj1.y - q2.y),
               f3 = dist2d(pj1.x - q3.x, pj1.y - q3.y);
  const double rem1 = or_removed(r1, dj), rem2 = or_removed(r2, dj), rem3 = or_removed(r3, dj);
  const double d0 = or_delta(c1, e1, f1, rem1);
  const double d1 = or_delta(c2, e1, f2, rem2);
  const double d2 = or_delta(c2, e2, f1, rem2);
  const double d3 = or_delta(c3, e1, f3, rem3);
  const double d4 = or_delta(c3, e3, f1, rem3);
  const bool left = j < i;
  const bool ok1 = i <= n - 2 && (left || j > i + 1), ok2 = i <= n - 3 && (left || j > i + 2), ok3 = i <= n - 4 && (left || j > i + 3);
  double m = ok1 ? d0 : INFINITY;
  int v = 0;
  if (ok2 && d1 < m) m = d1, v = 1;
  if (ok2 && d2 < m) m = d2, v = 2;
  if (ok3 && d3 < m) m = d3, v = 3;
  if (ok3 && d4 < m) m = d4, v = 4;
  *best = m;
  *code = v * n + j;
}

// the row part of a sweep: the row i (<= n - 3, Or-opt: <= n - 2) of the list against all columns, by the whole block.  A thread
// keeps one running best (value, code); better_col orders them, so the order in which the columns are met does not matter.
template <bool kOr>
__device__ __forceinline__ void focused_row(const double2* __restrict__ P, const double* __restrict__ D, int n, int i,
                                            double* __restrict__ rowv, int* __restrict__ rowj) {
  __shared__ double redv[4];
  __shared__ int redc[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double bv = 0.0;
  int bc = INT_MAX;
  if constexpr (!kOr) {
    const double2 a = P[i], a1 = P[i + 1];
    const double d_i = D[i];
    for (int j = i + 2 + threadIdx.x; j < n; j += 256) {
      const double2 pj = P[j], pj1 = P[j + 1];
      const double change = __dsub_rn(__dsub_rn(__dadd_rn(dist2d(a.x - pj.x, a.y - pj.y), dist2d(a1.x - pj1.x, a1.y - pj1.y)), d_i), D[j]);
      if (better_col(change, j, bv, bc)) bv = change, bc = j;
    }
  } else {
    const double2 p = P[i], q1 = P[i + 1 < n ? i + 1 : n], q2 = P[i + 2 < n ? i + 2 : n], q3 = P[i + 3 < n ? i + 3 : n];
    double c[LMAX], rm[LMAX];                                  // |P_i P_i+L+1| and d_i + d_i+L
#pragma unroll
    for (int L = 1; L <= LMAX; ++L) {
      c[L - 1] = rm[L - 1] = 0.0;
      if (i <= n - 1 - L) {
        const double2 b = P[i + L + 1];
        c[L - 1] = dist2d(p.x - b.x, p.y - b.y);
        rm[L - 1] = __dadd_rn(D[i], D[i + L]);
      }
    }
    for (int j = threadIdx.x; j < n; j += 256) {
      double m;
      int code;
      or_pair_best(q1, q2, q3, c[0], c[1], c[2], rm[0], rm[1], rm[2], i, n, j, P[j], P[j + 1], D[j], &m, &code);
      if (better_col(m, code, bv, bc)) bv = m, bc = code;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_down(bv, off);
    const int oc = __shfl_down(bc, off);
    if (better_col(ov, oc, bv, bc)) bv = ov, bc = oc;
  }
  if (lane == 0) redv[wave] = bv, redc[wave] = bc;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (better_col(redv[w], redc[w], bv, bc)) bv = redv[w], bc = redc[w];
    rowv[i] = bv;
    rowj[i] = bv < kThreshold ? bc : -1;
  }
}

// the column part of a sweep: the rows i0 .. i0 + TI - 1 that are not in the row list (own[i].x == 0) against the columns
// acols[0 .. ncols) (2-opt: every one in 2 .. n - 1).  Thread (r, slot) takes row i0 + r and the list entries slot, slot + 16, ..;
// the 16 slots of a row are combined in LDS.
template <bool kOr>
__device__ __forceinline__ void focused_cols(const double2* __restrict__ P, const double* __restrict__ D, int n,
                                             const int* __restrict__ acols, int ncols, const int2* __restrict__ own, int i0,
                                             double* __restrict__ rowv, int* __restrict__ rowj) {
  constexpr int kSlots = 256 / TI;
  __shared__ double redv[kSlots][TI];
  __shared__ int redc[kSlots][TI];
  const int r = threadIdx.x % TI, slot = threadIdx.x / TI, i = i0 + r;
  const bool mine = i <= (kOr ? n - 2 : n - 3) && !own[i].x;
  double bv = 0.0;
  int bc = INT_MAX;
  if (mine) {
    if constexpr (!kOr) {
      const double2 a = P[i], a1 = P[i + 1];
      const double d_i = D[i];
      for (int e = slot; e < ncols; e += kSlots) {
        const int j = acols[e];
        const double2 pj = P[j], pj1 = P[j + 1];
        const double change = __dsub_rn(__dsub_rn(__dadd_rn(dist2d(a.x - pj.x, a.y - pj.y), dist2d(a1.x - pj1.x, a1.y - pj1.y)), d_i), D[j]);
        if (j >= i + 2 && better_col(change, j, bv, bc)) bv = change, bc = j;
      }
    } else {
      const double2 p = P[i], q1 = P[i + 1 < n ? i + 1 : n], q2 = P[i + 2 < n ? i + 2 : n], q3 = P[i + 3 < n ? i + 3 : n];
      double c[LMAX], rm[LMAX];
#pragma unroll
      for (int L = 1; L <= LMAX; ++L) {
        c[L - 1] = rm[L - 1] = 0.0;
        if (i <= n - 1 - L) {
          const double2 b = P[i + L + 1];
          c[L - 1] = dist2d(p.x - b.x, p.y - b.y);
          rm[L - 1] = __dadd_rn(D[i], D[i + L]);
        }
      }
      for (int e = slot; e < ncols; e += kSlots) {
        const int j = acols[e];
        double m;
        int code;
        or_pair_best(q1, q2, q3, c[0], c[1], c[2], rm[0], rm[1], rm[2], i, n, j, P[j], P[j + 1], D[j], &m, &code);
        if (better_col(m, code, bv, bc)) bv = m, bc = code;
      }
    }
  }
  redv[slot][r] = bv, redc[slot][r] = bc;
  __syncthreads();
  if (slot == 0 && mine) {
    for (int w = 1; w < kSlots; ++w)
      if (better_col(redv[w][r], redc[w][r], bv, bc)) bv = redv[w][r], bc = redc[w][r];
    rowv[i] = bv;
    rowj[i] = bv < kThreshold ? bc : -1;
  }
}

// blocks 0 .. split - 1 of a tour are its row part (one list entry each), the blocks behind them its column part (a tile each);
// the host fixes both counts from the largest n of the call, the list lengths live in `foc`, surplus blocks return at once
__global__ __launch_bounds__(256) void mls_focused_row_best_kernel(
    const double2* __restrict__ tp, const double* __restrict__ dlen, const TourDesc* __restrict__ desc, double* __restrict__ rowv,
    int* __restrict__ rowj, const MlTourState* __restrict__ ts, const MlFocus* __restrict__ foc, const int* __restrict__ arows,
    const int* __restrict__ acols, const int2* __restrict__ marks, int split) {
  const MlFocus f = foc[blockIdx.y];
  const int phase = ts[blockIdx.y].phase;                        // uniform over the block
  if (f.mode != kFocused || (phase != kTwoOpt && phase != kOrOpt)) return;
  const TourDesc d = desc[blockIdx.y];
  const double2* P = tp + d.closed;
  const double* D = dlen + d.cols;
  if ((int)blockIdx.x < split) {
    if ((int)blockIdx.x >= f.nrows) return;
    const int i = arows[d.cols + blockIdx.x];
    if (phase == kTwoOpt)
      focused_row<false>(P, D, d.n, i, rowv + d.cols, rowj + d.cols);
    else
      focused_row<true>(P, D, d.n, i, rowv + d.cols, rowj + d.cols);
  } else {
    const int tile = blockIdx.x - split;
    if (tile >= (phase == kTwoOpt ? d.nblk_two : d.nblk_or)) return;
    if (phase == kTwoOpt)
      focused_cols<false>(P, D, d.n, acols + d.cols, f.ncols, marks + d.closed, tile * TI, rowv + d.cols, rowj + d.cols);
    else
      focused_cols<true>(P, D, d.n, acols + d.cols, f.ncols, marks + d.closed, tile * TI, rowv + d.cols, rowj + d.cols);
  }
}

// The selection of one tour with at most kCompactMax proposals, one per thread: (key, a, b) in LDS.  Per round a proposal wins
// iff no live proposal whose range meets its own has a lower key; winners leave; live proposals that meet a winner are dropped
// - step 2 of the multi-move 2-opt, one proposal against all.  Returns the number of winners (in every thread), their rows in
// winners[] in no particular order.
template <class Range>
__device__ __forceinline__ int select_compact(const Range range, int rows, const double* __restrict__ rowv,
                                              int* __restrict__ winners, int select_rounds) {
  __shared__ unsigned long long ckey[kCompactMax];
  __shared__ int crow[kCompactMax], ca[kCompactMax], cb[kCompactMax], cstate[kCompactMax];   // state: 0 live, 1 won now, 2 gone
  __shared__ int cm, cw;
  const int tid = threadIdx.x;
  if (tid == 0) cm = 0, cw = 0;
  __syncthreads();
  for (int i = tid; i < rows; i += kSelectThreads)
    if (range.proposes(i)) {
      const int slot = atomicAdd(&cm, 1);                        // < kCompactMax: the caller has counted
      int a, b;
      range(i, &a, &b);
      ckey[slot] = ordered_bits(rowv[i]);
      crow[slot] = i, ca[slot] = a, cb[slot] = b, cstate[slot] = 0;
    }
  __syncthreads();
  const int m = cm;
  const bool mine = tid < m;
  const unsigned long long key = mine ? ckey[tid] : 0;
  const int row = mine ? crow[tid] : 0, a = mine ? ca[tid] : 0, b = mine ? cb[tid] : 0;
  for (int round = 0; round < select_rounds; ++round) {
    bool win = mine && cstate[tid] == 0;
    if (win)
      for (int q = 0; q < m; ++q)
        if (cstate[q] == 0 && ca[q] < b && a < cb[q] && key_less(ckey[q], crow[q], key, row)) {
          win = false;
          break;
        }
    __syncthreads();
    if (win) {
      cstate[tid] = 1;
      winners[atomicAdd(&cw, 1)] = row;
    }
    __syncthreads();
    bool drop = false;
    if (mine && cstate[tid] == 0)
      for (int q = 0; q < m; ++q)
        if (cstate[q] == 1 && ca[q] < b && a < cb[q]) {
          drop = true;
          break;
        }
    __syncthreads();
    if (win || drop) cstate[tid] = 2;
    if (__syncthreads_count(mine && cstate[tid] == 0) == 0) break;
  }
  __syncthreads();
  return cw;
}

// the lists of the next sweep of a focused tour from the tour as it stands: position k is active iff tour[k] and tour[k+1] are in
// S.  2-opt: the rows are the active positions <= n - 3, the columns the active positions >= 2.  Or-opt: the rows are the
// positions i <= n - 2 with an active position among i .. i+3 (clipped to n - 1), the columns the active positions.  marks[k] keeps
// (k is in the row list, k is in the column list); the lists are in rising order (block_prefix).
__device__ __forceinline__ void focus_rebuild(const int* __restrict__ tour, const int* __restrict__ smark, int n, bool or_opt,
                                              int2* __restrict__ marks, int2* __restrict__ cum, int* __restrict__ arows,
                                              int* __restrict__ acols, MlFocus* f) {
  for (int p = threadIdx.x; p <= n; p += kSelectThreads) {
    const bool act = p < n && smark[tour[p]] && smark[tour[p + 1]];
    bool ract = act;
    if (or_opt)
      for (int k = 1; k <= LMAX; ++k)
        if (p + k <= n - 1) ract = ract || (smark[tour[p + k]] && smark[tour[p + k + 1]]);
    const bool row = or_opt ? (ract && p <= n - 2) : (act && p <= n - 3);
    const bool col = or_opt ? act : (act && p >= 2);
    marks[p] = make_int2(row, col);
  }
  __syncthreads();
  block_prefix(marks, cum, n);
  for (int p = threadIdx.x; p < n; p += kSelectThreads) {
    const int2 m = marks[p], c = cum[p];
    if (m.x) arows[c.x - 1] = p;
    if (m.y) acols[c.y - 1] = p;
  }
  if (threadIdx.x == 0) f->nrows = cum[n].x, f->ncols = cum[n].y;
}

// `full`: the phase words mls_row_best_kernel reads - a tour's own while it is in a full descent, kDone while it is focused
__global__ __launch_bounds__(kSelectThreads) void mls_select_focused_kernel(
    int* __restrict__ tours, const TourDesc* __restrict__ desc, const double* __restrict__ rowv_all, const int* __restrict__ rowj_all,
    int* __restrict__ live_all, int* __restrict__ winners_all, unsigned long long* __restrict__ tabv_all, int* __restrict__ tabi_all,
    int2* __restrict__ marks_all, int2* __restrict__ cum_all, long long max_iterations, int max_rounds, int select_rounds,
    int compact_select_max, MlState* st, MlGroup* grp, MlTourState* ts, MlTourState* full, MlFocus* foc, int* __restrict__ smark_all,
    int* __restrict__ tmark_all, int* __restrict__ arows_all, int* __restrict__ acols_all) {
  const int t = blockIdx.x;
  if (foc[t].mode != kFocused) {                                 // written by thread 0 of the keep / kick step only
    mls_select_tour<kSelectIterated>(tours, desc, rowv_all, rowj_all, live_all, winners_all, tabv_all, tabi_all, marks_all, cum_all,
                                     max_iterations, max_rounds, select_rounds, st, grp, ts);
    if (threadIdx.x == 0) full[t].phase = ts[t].phase;
    return;
  }
  MlTourState* s = ts + t;                                       // thread 0 alone writes it, at the end
  const int phase = s->phase, round = s->round, or_moved = s->or_moved;
  const long long sweeps = s->sweeps;
  if (phase != kTwoOpt && phase != kOrOpt) return;
  const TourDesc d = desc[t];
  const int n = d.n, rows = phase == kTwoOpt ? n - 2 : n - 1;
  const bool or_opt = phase == kOrOpt;
  int* tour = tours + d.closed;
  const int* rowj = rowj_all + d.cols;
  int* winners = winners_all + d.cols;
  int* smark = smark_all + d.cols;
  int* tmark = tmark_all + d.cols;
  const PhaseRange range{rowj, n, or_opt};
  __shared__ int nwin;
  int cnt = 0, m, dummy;
  for (int i = threadIdx.x; i < rows; i += kSelectThreads) cnt += range.proposes(i);
  block_sum_max(cnt, 0, &m, &dummy);
  int total = 0;
  if (m > 0 && m <= compact_select_max)
    total = select_compact(range, rows, rowv_all + d.cols, winners, select_rounds);
  else if (m > 0)
    total = select_disjoint(range, rows, n, rowv_all + d.cols, live_all + d.cols, winners, tabv_all + d.table, tabi_all + d.table,
                            marks_all + d.closed, cum_all + d.closed, select_rounds, &nwin);
  int next = phase;
  if (total == 0) {                                              // no proposal: the phase ends, the next one begins with S := T
    if (phase == kTwoOpt)
      next = kOrOpt;
    else
      next = !or_moved || round + 1 >= max_rounds ? kKeep : kTwoOpt;
    if (next != kKeep)
      for (int c = threadIdx.x; c < n; c += kSelectThreads) smark[c] = tmark[c];
  } else {
    // S := the end cities of the removed edges of every proposal, T += those of the winners, from the tour before the moves
    for (int c = threadIdx.x; c < n; c += kSelectThreads) smark[c] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < rows; i += kSelectThreads)
      if (rowj[i] >= 0) {
        const int c = rowj[i], j = or_opt ? c % n : c, L = or_opt ? variant_len(c / n) : 0;
        smark[tour[i]] = 1, smark[tour[i + 1]] = 1, smark[tour[j]] = 1, smark[tour[j + 1]] = 1;
        if (or_opt) smark[tour[i + L]] = 1, smark[tour[i + L + 1]] = 1;
      }
    for (int w = threadIdx.x; w < total; w += kSelectThreads) {
      const int i = winners[w], c = rowj[i], j = or_opt ? c % n : c, L = or_opt ? variant_len(c / n) : 0;
      tmark[tour[i]] = 1, tmark[tour[i + 1]] = 1, tmark[tour[j]] = 1, tmark[tour[j + 1]] = 1;
      if (or_opt) tmark[tour[i + L]] = 1, tmark[tour[i + L + 1]] = 1;
    }
    __syncthreads();
    if (or_opt)
      or_opt_winners(tour, (int*)(cum_all + d.closed), winners, rowj, n, total);   // cum is free after the selection
    else
      reverse_winners(tour, winners, rowj, total);
    if (sweeps + 1 >= max_iterations) next = kKeep;
  }
  __syncthreads();
  if (next != kKeep)
    focus_rebuild(tour, smark, n, next == kOrOpt, marks_all + d.closed, cum_all + d.closed, arows_all + d.cols,
                  acols_all + d.cols, foc + t);
  if (threadIdx.x == 0) {
    s->phase = next;
    if (total == 0) {
      if (phase == kTwoOpt) s->or_moved = 0;
      if (next == kTwoOpt) s->round = round + 1;
    } else {
      s->sweeps = sweeps + 1;
      if (or_opt) {
        s->or_opt_sweeps += 1;
        s->or_opt_moves += total;
        s->or_moved = 1;
      } else {
        s->two_opt_sweeps += 1;
        s->two_opt_moves += total;
      }
    }
  }
}

// mls_keep_kick_kernel for the focused search.  After a kick: T := the cities the kicked tour holds at a-1, a, a+l2-1, a+l2, b-1
// and b of every kept draw, S := T, the lists of the first 2-opt sweep, and the tour is focused.  After the keep of the last
// kick (kicks > 0): the closing full descent of the incumbent starts; at its keep the tour is done.  kHeat: as there.
template <bool kHeat>
__global__ __launch_bounds__(kSelectThreads) void mls_keep_kick_focused_kernel(
    const double* __restrict__ points, int* __restrict__ tours, int* __restrict__ inc_all, const TourDesc* __restrict__ desc,
    const unsigned long long* __restrict__ seeds, const unsigned long long* __restrict__ offsets, int kicks, int kick_size,
    int span, int no_descent, MlState* st, MlGroup* grp, MlTourState* ts, MlIter* iters, MlTourState* full, MlFocus* foc,
    int2* __restrict__ marks_all, int2* __restrict__ cum_all, int* __restrict__ smark_all, int* __restrict__ tmark_all,
    int* __restrict__ arows_all, int* __restrict__ acols_all, HeatArgs<kHeat> hx) {
  const int t = blockIdx.x;
  if (ts[t].phase != kKeep) return;                              // written by thread 0 of this block at its end only
  const TourDesc d = desc[t];
  const int n = d.n;
  int* tour = tours + d.closed;
  int* inc = inc_all + d.closed;
  int* smark = smark_all + d.cols;
  int* tmark = tmark_all + d.cols;
  MlIter* it = iters + t;                                        // thread 0 alone writes it and foc[t], at the end
  __shared__ double part[kLenParts];
  __shared__ int ka[kMaxKickSize], kl1[kMaxKickSize], kb[kMaxKickSize], kkeep[kMaxKickSize];
  const int have = it->have, kick = it->kick;                    // read before the barriers of tour_length
  const bool closing = foc[t].mode == kClosing;
  const double inc_len = it->length;
  const double len = tour_length(points + d.points, tour, n, part);
  const bool take = !have || len <= inc_len;                     // uniform over the block
  if (take)
    for (int k = threadIdx.x; k <= n; k += kSelectThreads) inc[k] = tour[k];
  else
    for (int k = threadIdx.x; k <= n; k += kSelectThreads) tour[k] = inc[k];
  const bool more = !closing && kick < kicks;
  const bool close_next = !closing && !more && kicks > 0 && !no_descent;
  int nkept = 0;
  if (more) {
    if constexpr (kHeat) {
      __syncthreads();                                           // the copy above is complete
      const MlHeatTour h = hx.tab[t];
      heat_prefix(inc, n, hx.row_ptr + h.rows, hx.col + h.edges, hx.q + h.heat, hx.W + d.closed, (unsigned long long*)part);
    }
    if (threadIdx.x < 64) kick_draws<kHeat>(seeds, offsets, t, kick, kick_size, span, n, d.closed, hx, ka, kl1, kb, kkeep);
    for (int c = threadIdx.x; c < n; c += kSelectThreads) tmark[c] = 0;
    __syncthreads();                                             // and the copy above is complete
    kick_swaps(tour, inc, kick_size, ka, kl1, kb, kkeep);
    __syncthreads();
    if ((int)threadIdx.x < kick_size && kkeep[threadIdx.x]) {    // 1 <= a, b <= n
      const int a = ka[threadIdx.x], b = kb[threadIdx.x], l2 = b - a - kl1[threadIdx.x];
      tmark[tour[a - 1]] = 1, tmark[tour[a]] = 1, tmark[tour[a + l2 - 1]] = 1, tmark[tour[a + l2]] = 1;
      tmark[tour[b - 1]] = 1, tmark[tour[b]] = 1;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += kSelectThreads) smark[c] = tmark[c];
    __syncthreads();
    focus_rebuild(tour, smark, n, false, marks_all + d.closed, cum_all + d.closed, arows_all + d.cols, acols_all + d.cols, foc + t);
  }
  if (threadIdx.x == 0) {
    if (more)
      for (int c = 0; c < kick_size; ++c) nkept += kkeep[c];
    MlTourState* s = ts + t;
    MlFocus* f = foc + t;
    if (!have) {
      it->have = 1;
      it->first_length = len;
    } else if (take && !closing) {
      it->kept += 1;
      if (len < inc_len) it->improved += 1;
    }
    if (take) it->length = len;
    if (s->round > it->max_round) it->max_round = s->round;
    if (closing) f->closing_sweeps = (int)s->sweeps;
    if (more || close_next) {
      if (more) {
        it->kick = kick + 1;
        it->swapped += nkept;
      }
      s->phase = no_descent ? kKeep : kTwoOpt;
      s->round = 0;
      s->or_moved = 0;
      s->sweeps = 0;
      f->mode = more ? kFocused : kClosing;
      full[t].phase = more ? kDone : kTwoOpt;
    } else {
      s->phase = kDone;
      full[t].phase = kDone;
      report_done(grp + d.group, st);
    }
  }
}

}  // namespace
}  // namespace difusco
