"""The four multi-move TSP search entries (``difusco_tsp_multi_local_search_ragged``, ``_iterated_``, ``_focused_`` and
``_guided_search_ragged``) against recorded behaviour (tests/golden/tsp_search_entries.json, scripts/record_tsp_search_entries.py):
the bytes each ``_workspace_bytes`` reserves, the return code and message of every refusal, and on short runs of every mode the
tours, every counter array and the host synchronisations, all as exact values.  The emulation suites pin the rule; this pins what
they leave open - the sizes Python allocates by, the messages, ``host_syncs`` as a number - for changes to the host side."""
import json
import os

import pytest
import torch

import tsp_search_entries_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "tsp_search_entries.json")) as f:
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


def test_workspace_bytes(recorded, library):
    assert C.workspace_sizes(library) == recorded["workspace_bytes"]


def test_workspace_bytes_refusals(recorded, library):
    got = C.size_refusals(library)
    assert got == recorded["workspace_bytes_refusals"]
    assert all(rc < 0 for rows in got.values() for rc, _ in rows.values())


def test_workspace_bytes_null_result(library):
    for entry in C.ENTRIES:
        args = (1, None, None) + ((None,) if entry == "guided_search" else ())
        assert getattr(library, f"difusco_tsp_{entry}_ragged_workspace_bytes")(*args, None) < 0
        assert "bytes is null" in library.difusco_last_error().decode()


@pytest.mark.parametrize("entry", C.ENTRIES)
def test_refusals(recorded, library, entry):
    want = recorded["refusals"][entry]
    assert list(want) == [name for name, _ in C.REFUSALS[entry]]
    for name, change in C.REFUSALS[entry]:
        got = C.refused_call(library, entry, **change)
        assert got[0] < 0 and got == want[name], name


@pytest.mark.parametrize("mode,kicks,cap", C.RUNS, ids=[C.run_name(*r) for r in C.RUNS])
def test_short_run(recorded, dev, mode, kicks, cap):
    want = recorded["runs"][C.run_name(mode, kicks, cap)]
    got = C.short_run(dev, recorded["inputs"], mode, kicks, cap)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
