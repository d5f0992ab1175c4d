// The host side of the two resident tour searches (tsp_resident.hip) as a stand-alone program for a sanitizer run without a GPU:
// the size and refusal paths over the sizes and refusals of tests/resident_entries_cases.py, the group above the limit included
// (the walk that builds the group table runs up to it).  No call here reaches a HIP call - a refused call returns in front of the
// first one.  Build the host side with the sanitizers and run it (gfx950 cross-compiles; the device code is not executed):
//
//   cd difusco_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tsp_resident.hip ../../scripts/resident_host_check.cpp -fsanitize=address,undefined \
//       -o /tmp/resident_host_check && /tmp/resident_host_check
//
// It prints one line per call: the return code and the bytes or the message.  The lines of a correct library are those of
// tests/golden/resident_entries.json; the exit status is 1 if a call that must be refused is not, or the other way round.
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
  std::vector<Shape> shapes = {{{4}, {1}}, {{4}, {2}}, {{5}, {2}}, {{7}, {1}}, {{33}, {3}}, {{65}, {1}}, {{4}, {20}}, {{43}, {5}},
                               {{4, 7, 33}, {20, 1, 3}}, {{33, 33}, {3, 2}}, {std::vector<int32_t>(11, 5), std::vector<int32_t>(11, 2)},
                               {std::vector<int32_t>(600, 8), std::vector<int32_t>(600, 1)}};
  char what[128];
  for (size_t k = 0; k < shapes.size(); ++k) {
    const Shape& s = shapes[k];
    const int G = (int)s.n.size();
    size_t bytes = 0;
    for (int method : {0, 1}) {
      snprintf(what, sizeof(what), "size two_opt method%d shape%zu", method, k);
      report(what, difusco_tsp_two_opt_resident_workspace_bytes(G, s.n.data(), s.tours.data(), method, &bytes), true, bytes);
    }
    snprintf(what, sizeof(what), "size local_search shape%zu", k);
    report(what, difusco_tsp_local_search_resident_workspace_bytes(G, s.n.data(), s.tours.data(), &bytes), true, bytes);
  }
  // the refusals: every call departs from the valid one in the named arguments
  const int M = difusco_tsp_two_opt_resident_max_cells();
  report("limits agree", M == difusco_tsp_local_search_resident_max_cells() ? DIFUSCO_OK : DIFUSCO_EINVAL, true, (size_t)M);
  const int32_t n_ok[2] = {5, 9}, t_ok[2] = {2, 1}, n_bad[2] = {5, 3}, t_bad[2] = {0, 1}, t_many[2] = {65535, 1};
  const int32_t n_over[2] = {5, M}, n_501[2] = {5, 500}, t_501[2] = {2, M / 501 + 1}, n_bad_over[2] = {3, M};
  size_t bytes = 0, need_two = 0, need_ls = 0;
  report("valid two_opt size", difusco_tsp_two_opt_resident_workspace_bytes(2, n_ok, t_ok, 0, &need_two), true, need_two);
  report("valid local_search size", difusco_tsp_local_search_resident_workspace_bytes(2, n_ok, t_ok, &need_ls), true, need_ls);
  report("size two_opt groups_0", difusco_tsp_two_opt_resident_workspace_bytes(0, nullptr, nullptr, 0, &bytes), false, 0);
  report("size two_opt n_3", difusco_tsp_two_opt_resident_workspace_bytes(2, n_bad, t_ok, 0, &bytes), false, 0);
  report("size two_opt tours_too_many", difusco_tsp_two_opt_resident_workspace_bytes(2, n_ok, t_many, 1, &bytes), false, 0);
  report("size two_opt null_bytes", difusco_tsp_two_opt_resident_workspace_bytes(2, n_ok, t_ok, 0, nullptr), false, 0);
  report("size two_opt method_2", difusco_tsp_two_opt_resident_workspace_bytes(2, n_ok, t_ok, 2, &bytes), false, 0);
  report("size two_opt order_n_3_method_2", difusco_tsp_two_opt_resident_workspace_bytes(2, n_bad, t_ok, 2, &bytes), false, 0);
  report("size local_search groups_0", difusco_tsp_local_search_resident_workspace_bytes(0, n_ok, t_ok, &bytes), false, 0);
  report("size local_search tours_0", difusco_tsp_local_search_resident_workspace_bytes(2, n_ok, t_bad, &bytes), false, 0);
  report("size local_search null_bytes", difusco_tsp_local_search_resident_workspace_bytes(2, n_ok, t_ok, nullptr), false, 0);
  report("size local_search null_bytes_groups_0", difusco_tsp_local_search_resident_workspace_bytes(0, nullptr, nullptr, nullptr), false, 0);

  std::vector<double> points(64);
  std::vector<int32_t> tours(64), r32(4);
  std::vector<char> ws(need_two > need_ls ? need_two : need_ls);
  std::vector<int64_t> a(4), b(4);
  int64_t pairs = 0;
  int32_t syncs = 0;
  double* P = points.data();
  int32_t* T = tours.data();
  void* W = ws.data();
  // difusco_tsp_two_opt_resident
  report("two_opt groups_0", difusco_tsp_two_opt_resident(0, n_ok, t_ok, P, T, 10, 0, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt null_group_n", difusco_tsp_two_opt_resident(2, nullptr, t_ok, P, T, 10, 0, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt n_3", difusco_tsp_two_opt_resident(2, n_bad, t_ok, P, T, 10, 0, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt tours_0", difusco_tsp_two_opt_resident(2, n_ok, t_bad, P, T, 10, 0, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt method_2", difusco_tsp_two_opt_resident(2, n_ok, t_ok, P, T, 10, 2, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt null_points", difusco_tsp_two_opt_resident(2, n_ok, t_ok, nullptr, T, 10, 0, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt null_tours", difusco_tsp_two_opt_resident(2, n_ok, t_ok, P, nullptr, 10, 1, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt null_workspace", difusco_tsp_two_opt_resident(2, n_ok, t_ok, P, T, 10, 0, 0, nullptr, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt null_iterations_out", difusco_tsp_two_opt_resident(2, n_ok, t_ok, P, T, 10, 0, 0, W, need_two, nullptr, nullptr, nullptr, nullptr), false, 0);
  report("two_opt max_iterations_-1", difusco_tsp_two_opt_resident(2, n_ok, t_ok, P, T, -1, 0, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt per_launch_-1", difusco_tsp_two_opt_resident(2, n_ok, t_ok, P, T, 10, 0, -1, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt workspace_short", difusco_tsp_two_opt_resident(2, n_ok, t_ok, P, T, 10, 0, 0, W, need_two - 1, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt max_cells_one_tour", difusco_tsp_two_opt_resident(2, n_over, t_ok, P, T, 10, 1, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt max_cells_tours_of_501", difusco_tsp_two_opt_resident(2, n_501, t_501, P, T, 10, 0, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt order_n_3_max_cells", difusco_tsp_two_opt_resident(2, n_bad_over, t_ok, P, T, 10, 0, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt order_method_max_cells", difusco_tsp_two_opt_resident(2, n_over, t_ok, P, T, 10, 2, 0, W, need_two, a.data(), &pairs, &syncs, nullptr), false, 0);
  report("two_opt order_workspace_max_cells", difusco_tsp_two_opt_resident(2, n_over, t_ok, P, T, 10, 0, 0, W, need_two - 1, a.data(), &pairs, &syncs, nullptr), false, 0);
  // difusco_tsp_local_search_resident
  report("local_search groups_0", difusco_tsp_local_search_resident(0, n_ok, t_ok, P, T, 10, 2, 0, W, need_ls, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search null_group_tours", difusco_tsp_local_search_resident(2, n_ok, nullptr, P, T, 10, 2, 0, W, need_ls, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search n_3", difusco_tsp_local_search_resident(2, n_bad, t_ok, P, T, 10, 2, 0, W, need_ls, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search null_points", difusco_tsp_local_search_resident(2, n_ok, t_ok, nullptr, T, 10, 2, 0, W, need_ls, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search null_workspace", difusco_tsp_local_search_resident(2, n_ok, t_ok, P, T, 10, 2, 0, nullptr, need_ls, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search null_two_opt_iterations_out", difusco_tsp_local_search_resident(2, n_ok, t_ok, P, T, 10, 2, 0, W, need_ls, nullptr, b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search null_or_opt_iterations_out", difusco_tsp_local_search_resident(2, n_ok, t_ok, P, T, 10, 2, 0, W, need_ls, a.data(), nullptr, r32.data(), &syncs, nullptr), false, 0);
  report("local_search null_rounds_out", difusco_tsp_local_search_resident(2, n_ok, t_ok, P, T, 10, 2, 0, W, need_ls, a.data(), b.data(), nullptr, nullptr, nullptr), false, 0);
  report("local_search max_iterations_-1", difusco_tsp_local_search_resident(2, n_ok, t_ok, P, T, -1, 0, 0, W, need_ls, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search order_max_rounds_per_launch", difusco_tsp_local_search_resident(2, n_ok, t_ok, P, T, 10, 0, -1, W, need_ls, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search order_per_launch_workspace", difusco_tsp_local_search_resident(2, n_ok, t_ok, P, T, 10, 2, -1, W, need_ls - 1, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search workspace_short", difusco_tsp_local_search_resident(2, n_ok, t_ok, P, T, 10, 2, 0, W, need_ls - 1, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search max_cells_one_tour", difusco_tsp_local_search_resident(2, n_over, t_ok, P, T, 10, 2, 0, W, need_ls, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search max_cells_tours_of_501", difusco_tsp_local_search_resident(2, n_501, t_501, P, T, 10, 2, 0, W, need_ls, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search order_max_rounds_max_cells", difusco_tsp_local_search_resident(2, n_over, t_ok, P, T, 10, 0, 0, W, need_ls, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  report("local_search order_workspace_max_cells", difusco_tsp_local_search_resident(2, n_over, t_ok, P, T, 10, 2, 0, W, need_ls - 1, a.data(), b.data(), r32.data(), &syncs, nullptr), false, 0);
  printf("%d unexpected return codes\n", failures);
  return failures ? 1 : 0;
}
