"""tests/golden/two_opt_entries.json is not self-referential: the tours (or their hashes) and the iteration counts of every recorded
run equal what ``oracle.tsp_decode_oracle.batched_two_opt`` computes per group on the fixture's inputs.  No GPU.  The oracle holds
four N x N float64 matrices per tour, so the n = 1025 groups (cap 25) take most of the time here."""
import json
import os

import pytest

import two_opt_entries_cases as C
from oracle.tsp_decode_oracle import batched_two_opt


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "two_opt_entries.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def oracle(recorded):
    """(tours, iterations) of one group at one cap, computed once."""
    done = {}

    def get(n, g, scale, cap):
        if (n, g, scale, cap) not in done:
            pts, tours = C.group_arrays(recorded["inputs"], n, g, scale)
            out, it = batched_two_opt(pts, tours, max_iterations=cap)
            done[(n, g, scale, cap)] = (C.encode_tours(out), int(it))
        return done[(n, g, scale, cap)]
    return get


def test_fixture_holds_every_run(recorded):
    assert sorted(recorded["runs"]) == sorted(C.run_name(*r) for r in C.RUNS)


def test_one_group_starts_at_a_local_optimum(recorded, oracle):
    for n in C.SIZES:
        tours, it = oracle(n, 1, 1.0, 1000 if n < 1025 else C.BIG_CAP)
        assert it == 0 and tours == C.encode_tours(C.group_arrays(recorded["inputs"], n, 1)[1])
        assert any(oracle(n, g, 1.0, 3)[1] > 0 for g in (0, 2))                  # while another group goes on


@pytest.mark.parametrize("shape", list(C.SIZES) + ["mixed", C.SCALED])
def test_recorded_runs_match_the_oracle(recorded, oracle, shape):
    runs = [r for r in C.RUNS if r[1] == shape]
    assert runs
    for entry, _, cap in runs:
        got = recorded["runs"][C.run_name(entry, shape, cap)]
        want = [oracle(n, g, scale, C.cap_of(shape, cap)) for n, g, scale in C.groups_of(shape)]
        assert got["tours"] == [t for t, _ in want], (entry, cap)
        assert got["iterations"] == [it for _, it in want], (entry, cap)
        if entry in ("ragged_exact",) or shape == C.SCALED:
            assert got["exact_pairs"] == [C.exact_pairs_of_exact_run(shape, cap, got["iterations"])], (entry, cap)
