"""The group-synchronised multi-move 2-opt entries (``difusco_tsp_multi_two_opt_ragged``, ``difusco_tsp_nbr_two_opt_ragged``) and
``difusco_tsp_nbr_local_search_ragged`` against recorded behaviour (tests/golden/multi_move_entries.json,
scripts/record_multi_move_entries.py): the bytes each ``_workspace_bytes`` reserves, the return code and message of every refusal,
and on short runs the tours and every counter array, all as exact values.  The emulation suites pin the rules; this pins what
they leave open - the sizes Python allocates by, the messages, the order of the checks - for changes to the host side.  The
figures that are not the recorded ones are written once each, in ``multi_move_entries_cases.merged_state_word_bytes`` and
``tour_descriptor_bytes``."""
import json
import os

import pytest
import torch

import multi_move_entries_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "multi_move_entries.json")) as f:
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
    want = C.expected_sizes(recorded["workspace_bytes"])
    assert len(want) == len(C.SHAPES) and all(rc == 0 for row in want for rc, _ in (v for k, v in row.items() if not k.startswith("group_")))
    assert C.workspace_sizes(library) == want


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
        assert got[0] < 0 and got == want[name], name


@pytest.mark.parametrize("run", C.RUNS, ids=[C.run_name(*r) for r in C.RUNS])
def test_short_run(recorded, dev, run):
    want = recorded["runs"][C.run_name(*run)]
    got = C.short_run(dev, recorded["inputs"], *run)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
