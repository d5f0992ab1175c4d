"""The two resident tour searches (``difusco_tsp_two_opt_resident``, ``difusco_tsp_local_search_resident``) against recorded
behaviour (tests/golden/resident_entries.json, scripts/record_resident_entries.py): the limit, the bytes each ``_workspace_bytes``
reserves, the return code and message of every refusal, and on short runs the tours, every counter array, ``host_syncs`` and the
2-opt entry's ``exact_pairs``, all as exact values.  The two resident suites pin the rules; this pins what they leave open - the
sizes Python allocates by, the messages, the order of the checks, the launches of a call - for changes to the shared skeleton and
the host side."""
import json
import os

import pytest
import torch

import resident_entries_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "resident_entries.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def library():
    from difusco_amd import _lib
    return _lib.lib()


def test_max_cells_and_workspace_bytes(recorded, library):
    want = recorded["workspace_bytes"]
    assert len(want) == len(C.SIZE_SHAPES) and all(rc == 0 for row in want for rc, _ in (v for k, v in row.items() if not k.startswith("group_")))
    assert C.workspace_sizes(library) == want
    assert C.max_cells(library) == recorded["max_cells"]


def test_workspace_bytes_refusals(recorded, library):
    got = C.size_refusals(library)
    assert got == recorded["workspace_bytes_refusals"]
    assert all(rc < 0 for rows in got.values() for rc, _ in rows.values())


@pytest.mark.parametrize("entry", C.ENTRIES)
def test_refusals(recorded, library, entry):
    want = recorded["refusals"][entry]
    assert list(want) == [name for name, _ in C.REFUSALS[entry]]
    for name, change in C.REFUSALS[entry]:
        got = C.refused_call(library, entry, **change)
        assert got[0] < 0 and got[2] and got == want[name], name


@pytest.mark.parametrize("run", C.RUNS, ids=[C.run_name(*r) for r in C.RUNS])
def test_short_run(recorded, dev, run):
    want = C.recorded_run(recorded, C.run_name(*run))
    got = C.short_run(dev, recorded["inputs"], *run)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
