"""The six single-move 2-opt entries (``difusco_tsp_two_opt``, ``_grouped``, ``_screened``, ``_grouped_screened`` and ``_ragged``
with both methods) against recorded behaviour (tests/golden/two_opt_entries.json, scripts/record_two_opt_entries.py): the bytes each
``_workspace_bytes`` reserves, the return code and message of every refusal, and on short runs the tours, ``iterations_out`` and
``exact_pairs_out``, all as exact values.  The oracle tests pin the rule (tests/test_two_opt_entries_host.py does so for this
fixture); this pins what they leave open - the sizes Python allocates by, the messages, ``exact_pairs`` - for changes to the host
side, and states the relations between the entries from the test's own outputs."""
import json
import os

import pytest
import torch

import two_opt_entries_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "two_opt_entries.json")) as f:
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


@pytest.fixture(scope="module")
def run(recorded, dev):
    """Every run once per module: the relations below compare runs that test_short_run has made as well."""
    done = {}

    def get(entry, shape, cap, one_group=False):
        key = (entry, shape, cap, one_group)
        if key not in done:
            done[key] = C.short_run(dev, recorded["inputs"], entry, shape, cap, one_group=one_group)
        return done[key]
    return get


def test_workspace_bytes(recorded, library):
    assert C.workspace_sizes(library) == recorded["workspace_bytes"]


def test_plain_workspace_bytes_are_the_grouped_ones_of_one_group(library):
    for n in C.WS_N:
        for G, P in C.WS_GROUPS:
            plain = C.uniform_workspace_bytes(library, "two_opt", n, G * P)
            assert plain[0] == 0 and plain == C.uniform_workspace_bytes(library, "two_opt_grouped", n, 1, G * P), (n, G * P)


def test_workspace_bytes_refusals(recorded, library):
    got = C.size_refusals(library)
    assert got == recorded["workspace_bytes_refusals"]
    assert all(rc < 0 for rows in got.values() for rc, _ in rows.values())


@pytest.mark.parametrize("entry", list(C.REFUSALS))
def test_refusals(recorded, library, entry):
    want = recorded["refusals"][entry]
    assert list(want) == [name for name, _ in C.REFUSALS[entry]]
    for name, change in C.REFUSALS[entry]:
        got = C.refused_call(library, entry, **change)
        assert got[0] < 0 and got == want[name], name


@pytest.mark.parametrize("entry,shape,cap", C.RUNS, ids=[C.run_name(*r) for r in C.RUNS])
def test_short_run(recorded, run, entry, shape, cap):
    want = recorded["runs"][C.run_name(entry, shape, cap)]
    got = run(entry, shape, cap)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k


SHAPED = [(n, cap) for n in C.SIZES for cap in C.CAPS]


@pytest.mark.parametrize("shape,cap", SHAPED + [("mixed", cap) for cap in C.CAPS])
def test_screened_equals_exact(run, shape, cap):
    pairs = [("ragged_screened", "ragged_exact")] + ([] if shape == "mixed" else [("screened", "plain"), ("grouped_screened", "grouped")])
    for screened, exact in pairs:
        a, b = run(screened, shape, cap), run(exact, shape, cap)
        assert a["tours"] == b["tours"] and a["iterations"] == b["iterations"], screened


@pytest.mark.parametrize("shape,cap", SHAPED)
def test_ragged_at_equal_sizes_equals_grouped(run, shape, cap):
    for ragged, grouped in (("ragged_exact", "grouped"), ("ragged_screened", "grouped_screened")):
        a, b = run(ragged, shape, cap), run(grouped, shape, cap)
        assert a["tours"] == b["tours"] and a["iterations"] == b["iterations"], ragged
    assert run("ragged_screened", shape, cap)["exact_pairs"] == run("grouped_screened", shape, cap)["exact_pairs"]
    assert run("ragged_exact", shape, cap)["exact_pairs"] == [C.exact_pairs_of_exact_run(shape, cap, run("grouped", shape, cap)["iterations"])]


@pytest.mark.parametrize("shape,cap", SHAPED)
def test_plain_equals_grouped_with_one_group(run, shape, cap):
    a, b = run("plain", shape, cap), run("grouped", shape, cap, one_group=True)
    assert a["tours"] == b["tours"] and a["iterations"] == b["iterations"]


def test_no_screen_bound_takes_the_exact_sweep(run):
    """M = 2^70 in one group: the whole call evaluates every pair in float64 and says so in ``exact_pairs``."""
    got = run("grouped_screened", C.SCALED, 1000)
    assert got["exact_pairs"] == [C.exact_pairs_of_exact_run(C.SCALED, 1000, got["iterations"])]
