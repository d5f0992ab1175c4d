// The host side of the group-wise multi-move entries (two_opt_multi.hip, or_opt_multi.hip) as a stand-alone
// program for a sanitizer run without a GPU: the layout, size and refusal paths over the sizes and refusals of
// tests/multi_move_entries_cases.py.  No call here reaches a HIP call - a refused call returns in front of the first one.
// Build the host side with the sanitizers and run it (gfx950 cross-compiles; the device code is not executed):
//
//   cd difusco_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       two_opt_multi.hip or_opt_multi.hip ../../scripts/multi_move_host_check.cpp -fsanitize=address,undefined \
//       -o /tmp/multi_move_host_check && /tmp/multi_move_host_check
//
// It prints one line per call: the return code and the bytes or the message.  The lines of a correct library are those of
// tests/golden/multi_move_entries.json (the sizes with the closed forms of tests/multi_move_entries_cases.py applied) and, for the
// entries of or_opt_multi.hip, of tests/golden/tsp_search_entries.json; the exit status is 1 if a call that must be refused is not,
// or the other way round.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/difusco_hip.h"

namespace difusco {
static thread_local char g_err[512] = "";
int set_error(int code, const char* fmt, ...) {                  // api.hip's, which this program does not link
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace difusco

static int failures = 0;

static void report(const char* what, int rc, bool want_ok, size_t bytes) {
  if ((rc == DIFUSCO_OK) != want_ok) ++failures;
  if (rc == DIFUSCO_OK)
    printf("%s: ok %zu\n", what, bytes);
  else
    printf("%s: %d %s\n", what, rc, difusco::g_err);
}

struct Shape {
  std::vector<int32_t> n, tours;
};

int main() {
  const std::vector<Shape> shapes = {{{4}, {1}}, {{16}, {1}}, {{17}, {2}}, {{18}, {3}}, {{1025}, {1}}, {{4, 1025}, {3, 1}},
                                     {{16, 17, 18}, {1, 2, 3}}, {{1025, 4, 17}, {2, 3, 1}}};
  char what[128];
  for (size_t k = 0; k < shapes.size(); ++k) {
    const Shape& s = shapes[k];
    const int G = (int)s.n.size();
    size_t bytes = 0;
    snprintf(what, sizeof(what), "size multi_two_opt shape%zu", k);
    report(what, difusco_tsp_multi_two_opt_ragged_workspace_bytes(G, s.n.data(), s.tours.data(), &bytes), true, bytes);
    snprintf(what, sizeof(what), "size multi_local_search shape%zu", k);
    report(what, difusco_tsp_multi_local_search_ragged_workspace_bytes(G, s.n.data(), s.tours.data(), &bytes), true, bytes);
    snprintf(what, sizeof(what), "size iterated_search shape%zu", k);
    report(what, difusco_tsp_iterated_search_ragged_workspace_bytes(G, s.n.data(), s.tours.data(), &bytes), true, bytes);
    snprintf(what, sizeof(what), "size focused_search shape%zu", k);
    report(what, difusco_tsp_focused_search_ragged_workspace_bytes(G, s.n.data(), s.tours.data(), &bytes), true, bytes);
    std::vector<int32_t> edges;
    for (int32_t n : s.n) edges.push_back(8 * n);
    snprintf(what, sizeof(what), "size guided_search shape%zu", k);
    report(what, difusco_tsp_guided_search_ragged_workspace_bytes(G, s.n.data(), s.tours.data(), edges.data(), &bytes), true, bytes);
    for (int K : {1, 8})
      for (int closing : {0, 1}) {
        snprintf(what, sizeof(what), "size nbr_two_opt K%d closing%d shape%zu", K, closing, k);
        report(what, difusco_tsp_nbr_two_opt_ragged_workspace_bytes(G, s.n.data(), s.tours.data(), K, closing, &bytes), true, bytes);
        snprintf(what, sizeof(what), "size nbr_local_search K%d closing%d shape%zu", K, closing, k);
        report(what, difusco_tsp_nbr_local_search_ragged_workspace_bytes(G, s.n.data(), s.tours.data(), K, closing, &bytes), true, bytes);
      }
  }
  // the refusals: every call departs from the valid one in the named arguments
  const int32_t n_ok[2] = {5, 9}, t_ok[2] = {2, 1}, n_bad[2] = {5, 3}, t_bad[2] = {0, 1}, n_big[2] = {5, 1 << 19};
  size_t bytes = 0, need_mt = 0, need_nb = 0, need_nl = 0, need_ml = 0;
  report("valid multi_local_search size", difusco_tsp_multi_local_search_ragged_workspace_bytes(2, n_ok, t_ok, &need_ml), true, need_ml);
  report("valid multi_two_opt size", difusco_tsp_multi_two_opt_ragged_workspace_bytes(2, n_ok, t_ok, &need_mt), true, need_mt);
  report("valid nbr_two_opt size", difusco_tsp_nbr_two_opt_ragged_workspace_bytes(2, n_ok, t_ok, 2, 1, &need_nb), true, need_nb);
  report("valid nbr_local_search size", difusco_tsp_nbr_local_search_ragged_workspace_bytes(2, n_ok, t_ok, 2, 1, &need_nl), true, need_nl);
  report("size groups_0", difusco_tsp_nbr_two_opt_ragged_workspace_bytes(0, nullptr, nullptr, 2, 1, &bytes), false, 0);
  report("size null_bytes", difusco_tsp_nbr_two_opt_ragged_workspace_bytes(2, n_ok, t_ok, 2, 1, nullptr), false, 0);
  report("size null_bytes plain", difusco_tsp_multi_two_opt_ragged_workspace_bytes(2, n_ok, t_ok, nullptr), false, 0);
  report("size n_3", difusco_tsp_nbr_local_search_ragged_workspace_bytes(2, n_bad, t_ok, 2, 1, &bytes), false, 0);
  report("size tours_0", difusco_tsp_multi_two_opt_ragged_workspace_bytes(2, n_ok, t_bad, &bytes), false, 0);
  report("size K_0", difusco_tsp_nbr_two_opt_ragged_workspace_bytes(2, n_ok, t_ok, 0, 1, &bytes), false, 0);
  report("size closing_2", difusco_tsp_nbr_local_search_ragged_workspace_bytes(2, n_ok, t_ok, 2, 2, &bytes), false, 0);
  report("size nK_too_many", difusco_tsp_nbr_two_opt_ragged_workspace_bytes(2, n_big, t_ok, INT32_MAX, 1, &bytes), false, 0);
  report("size nK_too_many nls", difusco_tsp_nbr_local_search_ragged_workspace_bytes(2, n_big, t_ok, INT32_MAX, 1, &bytes), false, 0);

  std::vector<double> points(64);
  std::vector<int32_t> tours(64), nbr(64), r32(4), f32(4);
  std::vector<char> ws(need_nb > need_nl ? need_nb : need_nl);            // the plain entries need less
  std::vector<int64_t> a(4), b(4), c(4), d(4), e(4);
  double* P = points.data();
  int32_t *T = tours.data(), *N = nbr.data();
  void* W = ws.data();
  // difusco_tsp_multi_two_opt_ragged
  report("multi_two_opt groups_0", difusco_tsp_multi_two_opt_ragged(0, n_ok, t_ok, P, T, 10, 4, W, need_mt, a.data(), b.data(), nullptr), false, 0);
  report("multi_two_opt null_group_n", difusco_tsp_multi_two_opt_ragged(2, nullptr, t_ok, P, T, 10, 4, W, need_mt, a.data(), b.data(), nullptr), false, 0);
  report("multi_two_opt n_3", difusco_tsp_multi_two_opt_ragged(2, n_bad, t_ok, P, T, 10, 4, W, need_mt, a.data(), b.data(), nullptr), false, 0);
  report("multi_two_opt null_points", difusco_tsp_multi_two_opt_ragged(2, n_ok, t_ok, nullptr, T, 10, 4, W, need_mt, a.data(), b.data(), nullptr), false, 0);
  report("multi_two_opt null_workspace", difusco_tsp_multi_two_opt_ragged(2, n_ok, t_ok, P, T, 10, 4, nullptr, need_mt, a.data(), b.data(), nullptr), false, 0);
  report("multi_two_opt null_moves_out", difusco_tsp_multi_two_opt_ragged(2, n_ok, t_ok, P, T, 10, 4, W, need_mt, a.data(), nullptr, nullptr), false, 0);
  report("multi_two_opt max_iterations_-1", difusco_tsp_multi_two_opt_ragged(2, n_ok, t_ok, P, T, -1, 0, W, need_mt, a.data(), b.data(), nullptr), false, 0);
  report("multi_two_opt select_rounds_0", difusco_tsp_multi_two_opt_ragged(2, n_ok, t_ok, P, T, 10, 0, W, need_mt - 1, a.data(), b.data(), nullptr), false, 0);
  report("multi_two_opt workspace_short", difusco_tsp_multi_two_opt_ragged(2, n_ok, t_ok, P, T, 10, 4, W, need_mt - 1, a.data(), b.data(), nullptr), false, 0);
  report("multi_two_opt max_iterations_0", difusco_tsp_multi_two_opt_ragged(2, n_ok, t_ok, P, T, 0, 4, W, need_mt, a.data(), b.data(), nullptr), true, 0);
  // difusco_tsp_nbr_two_opt_ragged
  report("nbr_two_opt tours_0", difusco_tsp_nbr_two_opt_ragged(2, n_ok, t_bad, P, T, N, 2, 1, 10, 4, W, need_nb, a.data(), b.data(), c.data(), nullptr), false, 0);
  report("nbr_two_opt K_0", difusco_tsp_nbr_two_opt_ragged(2, n_ok, t_ok, P, T, nullptr, 0, 1, 10, 4, W, need_nb, a.data(), b.data(), c.data(), nullptr), false, 0);
  report("nbr_two_opt closing_2", difusco_tsp_nbr_two_opt_ragged(2, n_ok, t_ok, P, T, N, 2, 2, -1, 4, W, need_nb, a.data(), b.data(), c.data(), nullptr), false, 0);
  report("nbr_two_opt null_neighbors", difusco_tsp_nbr_two_opt_ragged(2, n_ok, t_ok, P, T, nullptr, 2, 1, 10, 0, W, need_nb, a.data(), b.data(), c.data(), nullptr), false, 0);
  report("nbr_two_opt null_tours", difusco_tsp_nbr_two_opt_ragged(2, n_ok, t_ok, P, nullptr, N, 2, 1, 10, 4, W, need_nb, a.data(), b.data(), c.data(), nullptr), false, 0);
  report("nbr_two_opt null_full_sweeps_out", difusco_tsp_nbr_two_opt_ragged(2, n_ok, t_ok, P, T, N, 2, 1, 10, 4, W, need_nb, a.data(), nullptr, c.data(), nullptr), false, 0);
  report("nbr_two_opt select_rounds_0", difusco_tsp_nbr_two_opt_ragged(2, n_ok, t_ok, P, T, N, 2, 1, 10, 0, W, need_nb - 1, a.data(), b.data(), c.data(), nullptr), false, 0);
  report("nbr_two_opt workspace_short", difusco_tsp_nbr_two_opt_ragged(2, n_ok, t_ok, P, T, N, 2, 1, 10, 4, W, need_nb - 1, a.data(), b.data(), c.data(), nullptr), false, 0);
  report("nbr_two_opt max_iterations_0", difusco_tsp_nbr_two_opt_ragged(2, n_ok, t_ok, P, T, N, 2, 1, 0, 4, W, need_nb, a.data(), b.data(), c.data(), nullptr), true, 0);
  // difusco_tsp_nbr_local_search_ragged
  report("nbr_local_search n_3", difusco_tsp_nbr_local_search_ragged(2, n_bad, t_ok, P, T, N, 2, 1, 10, 2, 4, W, need_nl, a.data(), b.data(), r32.data(), c.data(), d.data(), e.data(), f32.data(), nullptr), false, 0);
  report("nbr_local_search K_0", difusco_tsp_nbr_local_search_ragged(2, n_ok, t_ok, P, T, nullptr, 0, 1, 10, 2, 4, W, need_nl, a.data(), b.data(), r32.data(), c.data(), d.data(), e.data(), f32.data(), nullptr), false, 0);
  report("nbr_local_search closing_2", difusco_tsp_nbr_local_search_ragged(2, n_ok, t_ok, P, T, N, 2, 2, 10, 2, 4, W, need_nl, a.data(), b.data(), r32.data(), c.data(), d.data(), e.data(), f32.data(), nullptr), false, 0);
  report("nbr_local_search null_neighbors", difusco_tsp_nbr_local_search_ragged(2, n_ok, t_ok, P, T, nullptr, 2, 1, 10, 0, 4, W, need_nl, a.data(), b.data(), r32.data(), c.data(), d.data(), e.data(), f32.data(), nullptr), false, 0);
  report("nbr_local_search null_full_rounds_out", difusco_tsp_nbr_local_search_ragged(2, n_ok, t_ok, P, T, N, 2, 1, 10, 2, 4, W, need_nl, a.data(), b.data(), r32.data(), c.data(), d.data(), e.data(), nullptr, nullptr), false, 0);
  report("nbr_local_search max_rounds_0", difusco_tsp_nbr_local_search_ragged(2, n_ok, t_ok, P, T, N, 2, 1, 10, 0, 0, W, need_nl, a.data(), b.data(), r32.data(), c.data(), d.data(), e.data(), f32.data(), nullptr), false, 0);
  report("nbr_local_search select_rounds_0", difusco_tsp_nbr_local_search_ragged(2, n_ok, t_ok, P, T, N, 2, 1, 10, 2, 0, W, need_nl - 1, a.data(), b.data(), r32.data(), c.data(), d.data(), e.data(), f32.data(), nullptr), false, 0);
  report("nbr_local_search workspace_short", difusco_tsp_nbr_local_search_ragged(2, n_ok, t_ok, P, T, N, 2, 1, 10, 2, 4, W, need_nl - 1, a.data(), b.data(), r32.data(), c.data(), d.data(), e.data(), f32.data(), nullptr), false, 0);
  report("nbr_local_search max_iterations_0", difusco_tsp_nbr_local_search_ragged(2, n_ok, t_ok, P, T, N, 2, 1, 0, 2, 4, W, need_nl, a.data(), b.data(), r32.data(), c.data(), d.data(), e.data(), f32.data(), nullptr), true, 0);
  // difusco_tsp_multi_local_search_ragged: the driver it shares with the listed entry
  report("multi_local_search n_3", difusco_tsp_multi_local_search_ragged(2, n_bad, t_ok, P, T, 10, 2, 4, W, need_ml, a.data(), b.data(), r32.data(), c.data(), d.data(), nullptr), false, 0);
  report("multi_local_search null_or_opt_moves_out", difusco_tsp_multi_local_search_ragged(2, n_ok, t_ok, P, T, 10, 2, 4, W, need_ml, a.data(), b.data(), r32.data(), c.data(), nullptr, nullptr), false, 0);
  report("multi_local_search max_rounds_0", difusco_tsp_multi_local_search_ragged(2, n_ok, t_ok, P, T, 10, 0, 0, W, need_ml, a.data(), b.data(), r32.data(), c.data(), d.data(), nullptr), false, 0);
  report("multi_local_search workspace_short", difusco_tsp_multi_local_search_ragged(2, n_ok, t_ok, P, T, 10, 2, 4, W, need_ml - 1, a.data(), b.data(), r32.data(), c.data(), d.data(), nullptr), false, 0);
  report("multi_local_search max_iterations_0", difusco_tsp_multi_local_search_ragged(2, n_ok, t_ok, P, T, 0, 2, 4, W, need_ml, a.data(), b.data(), r32.data(), c.data(), d.data(), nullptr), true, 0);
  printf("%d unexpected return codes\n", failures);
  return failures ? 1 : 0;
}
