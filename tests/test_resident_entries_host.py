"""tests/golden/resident_entries.json is not self-referential: the tours and the iteration / round counters of every recorded run
equal what the numpy restatements of the two rules compute group by group on the fixture's inputs - the 2-opt oracle
(``oracle.tsp_decode_oracle.batched_two_opt``) and ``or_opt_emulation.local_search``, the ones the two resident GPU suites
compare with.  ``exact_pairs`` of the exact method is the formula of tests/test_gpu_two_opt_resident.py, of the screened method
at most that, and ``host_syncs`` the launch counts those suites derive from the counters.  The inputs are checked for what they
are there to exercise.  No GPU: the sizes and refusals of the library in the tree are compared with the recording here as well,
since every refusal comes before any GPU work."""
import functools
import json
import os

import numpy as np
import pytest

import resident_entries_cases as C


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "resident_entries.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replay(recorded):
    """The emulated result of (entry, call, cap, rounds): the per-launch settings and the two methods share one."""
    return functools.lru_cache(maxsize=None)(lambda entry, call, cap, rounds: C.emulated_run(recorded["inputs"], entry, call, cap, rounds))


def test_fixture_holds_every_run_and_case(recorded):
    assert sorted(recorded["runs"]) == sorted(C.run_name(*r) for r in C.RUNS)
    assert len(set(C.run_name(*r) for r in C.RUNS)) == len(C.RUNS)
    assert len(recorded["commit"]) == 40
    assert [(r["group_n"], r["group_tours"]) for r in recorded["workspace_bytes"]] == [(n, t) for n, t in C.SIZE_SHAPES]
    for entry in C.ENTRIES:
        assert list(recorded["refusals"][entry]) == [name for name, _ in C.REFUSALS[entry]]
        assert all(rc < 0 and text and unchanged for rc, text, unchanged in recorded["refusals"][entry].values())
        assert all(rc < 0 and text for rc, text in recorded["workspace_bytes_refusals"][entry].values())
        for name in ("max_cells_one_tour", "max_cells_tours_of_501"):
            rc, text, _ = recorded["refusals"][entry][name]
            assert rc == -4 and f"difusco_tsp_{entry}_resident_max_cells" in text and f"limit of {recorded['max_cells'][entry]} cells" in text


def test_inputs_are_what_the_cases_need(recorded):
    inputs = recorded["inputs"]
    assert set(inputs) == set(C.GROUPS)
    for name, (n, P) in C.GROUPS.items():
        pts, tours = np.array(inputs[name]["points_q16"]), np.array(inputs[name]["tours"])
        assert pts.shape == (n, 2) and tours.shape == (P, n + 1)
        assert all(sorted(t[:-1]) == list(range(n)) and t[0] == t[-1] == 0 for t in tours.tolist())
    from difusco_amd.decode import two_opt_screen_bound
    tiny = C.group_arrays(inputs, len(C.CALLS) - 1)
    assert two_opt_screen_bound(np.abs(tiny[0][0]).max()) is not None and two_opt_screen_bound(np.abs(tiny[1][0]).max()) is None
    # the block shapes the groups are named for: threads as the host derives them, waves per team, teams
    def teams(call):
        pairs = max(P * ((n - 1) * (n - 2) // 2) for n, P in (C.GROUPS[g] for g in call))
        threads = min(max(-(-(-(-pairs // 4)) // 64) * 64, 256), 1024)
        return threads, [(max(threads // 64 // P, 1), threads // 64 // max(threads // 64 // P, 1)) for _, P in (C.GROUPS[g] for g in call)]
    assert teams(("n4x20",)) == (256, [(1, 4)])                 # 20 tours on 4 teams: five rounds
    assert teams(("n43x5",)) == (1024, [(3, 5)])                # 16 waves, 5 teams of 3: one wave left over
    assert teams(("n4x20", "poly7", "n33x3"))[0] == 384


def test_the_polygon_never_moves(recorded):
    start = recorded["inputs"]["poly7"]["tours"]
    for run in C.RUNS:
        if "poly7" in C.CALLS[run[1]]:
            got, at = C.recorded_run(recorded, C.run_name(*run)), C.CALLS[run[1]].index("poly7")
            assert got["tours"][at] == start and all(got[k][at] == 0 for k in C.OUTPUTS[run[0]] if k != "rounds"), run


@pytest.mark.parametrize("run", C.RUNS, ids=[C.run_name(*r) for r in C.RUNS])
def test_recorded_run_matches_the_emulation(recorded, replay, run):
    entry, call, cap, per_launch, variant = run
    got = C.recorded_run(recorded, C.run_name(*run))
    want = replay(entry, call, cap, None if entry == "two_opt" else variant)
    assert set(got) == set(want) | {"host_syncs"} | ({"exact_pairs"} if entry == "two_opt" else set())
    for k in want:
        assert got[k] == want[k], k
    per = per_launch or C.DEFAULT_PER_LAUNCH
    if entry == "two_opt":
        from test_gpu_two_opt_resident import exact_formula, launches_of
        groups = C.group_arrays(recorded["inputs"], call)
        formula = exact_formula(groups, want["iterations"], cap)
        assert got["exact_pairs"] == formula if variant == "exact" else 0 <= got["exact_pairs"] <= formula
        assert got["host_syncs"] == max(launches_of(it, cap, per) for it in want["iterations"])
    else:
        from test_gpu_local_search_resident import launches_of
        assert got["host_syncs"] == launches_of(want["two_opt_iterations"], want["or_opt_iterations"], per)


def test_the_screened_method_counts_what_the_recording_says_and_less_than_the_exact_one(recorded):
    """``exact_pairs`` of method 1 has no formula: it is pinned by the recording alone.  What can be said without one: a group
    without a screen bound counts like the exact method, and somewhere the screen saves pairs."""
    saved = 0
    for entry, call, cap, per_launch, variant in C.RUNS:
        if entry == "two_opt" and variant == "screened":
            exact = recorded["runs"][C.run_name(entry, call, cap, per_launch, "exact")]["exact_pairs"]
            saved += exact - recorded["runs"][C.run_name(entry, call, cap, per_launch, "screened")]["exact_pairs"]
    assert saved > 0


def test_the_library_in_the_tree_reserves_and_refuses_as_recorded(recorded):
    from difusco_amd import _lib
    L = _lib.lib()
    assert C.max_cells(L) == recorded["max_cells"]
    assert C.workspace_sizes(L) == recorded["workspace_bytes"]
    assert C.size_refusals(L) == recorded["workspace_bytes_refusals"]
    assert C.refusals(L) == recorded["refusals"]
