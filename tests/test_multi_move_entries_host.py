"""tests/golden/multi_move_entries.json is not self-referential: the tours and every counter array of every recorded run equal
what the numpy restatements of the three rules (``multi_two_opt_emulation``, ``nbr_two_opt_emulation``,
``nbr_local_search_emulation``) compute group by group on the fixture's inputs.  No GPU.  The inputs are also checked for what
they are there to exercise: the pads and the local optimum."""
import json
import os

import numpy as np
import pytest

import multi_move_entries_cases as C


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "multi_move_entries.json")) as f:
        return json.load(f)


def test_fixture_holds_every_run_and_case(recorded):
    assert sorted(recorded["runs"]) == sorted(C.run_name(*r) for r in C.RUNS)
    assert len(set(C.run_name(*r) for r in C.RUNS)) == len(C.RUNS)
    assert len(recorded["commit"]) == 40
    assert [(r["group_n"], r["group_tours"]) for r in recorded["workspace_bytes"]] == [(n, t) for n, t in C.SHAPES]
    for entry in C.ENTRIES:
        assert list(recorded["refusals"][entry]) == [name for name, _ in C.REFUSALS[entry]]
        assert all(rc < 0 and text for rc, text in recorded["refusals"][entry].values())
        assert all(rc < 0 and text for rc, text in recorded["workspace_bytes_refusals"][entry].values())


def test_inputs_are_what_the_cases_need(recorded):
    groups = C.group_arrays(recorded["inputs"], C.RUN_KS[-1])
    assert [(len(p), len(t)) for p, t, _ in groups] == [(4, 2), (7, 1), (33, 3)]
    for pts, tours, lists in groups:
        n = len(pts)
        assert np.array_equal(pts * 65536, np.round(pts * 65536))                # the 2^-16 grid
        assert all(sorted(t[:-1]) == list(range(n)) and t[0] == t[-1] == 0 for t in tours.tolist())
        assert lists.shape == (n, C.RUN_KS[-1])
    lists = groups[2][2]
    own = np.arange(33)[:, None]
    pads = (lists < 0) | (lists >= 33) | (lists == own)
    assert (lists == -1).all(1).sum() == 1 and (lists == 33).all(1).sum() == 1 and (lists == own).all(1).sum() == 1
    assert pads.all(1).sum() == 3 and not pads[~pads.all(1)].any()
    assert not any(((l < 0) | (l >= len(p)) | (l == np.arange(len(p))[:, None])).any() for p, _, l in groups[:2])


def test_the_polygon_group_never_moves(recorded):
    start = recorded["inputs"]["groups"][1]["tours"]
    for run in C.RUNS:
        got = recorded["runs"][C.run_name(*run)]
        assert got["tours"][1] == start, run
        assert all(got[k][1] == 0 for k in C.OUTPUTS[run[0]] if "sweeps" in k or "moves" in k), run


@pytest.mark.parametrize("run", C.RUNS, ids=[C.run_name(*r) for r in C.RUNS])
def test_recorded_run_matches_the_emulation(recorded, run):
    got = recorded["runs"][C.run_name(*run)]
    want = C.emulated_run(recorded["inputs"], *run)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
