"""The Python wrappers of ``difusco_amd.decode`` and the local-search part of ``difusco_amd.pipeline`` against recorded behaviour
(tests/golden/decode_wrappers.json, scripts/record_decode_wrappers.py; the cases: tests/decode_wrapper_cases.py): every returned
array with dtype and shape, every scalar with its type, the key set of every stats dict and info record, on the smallest calls
at which the shared plumbing can go wrong - one group (no cut), two equal groups with different tours (the split), three
groups of different unsorted sizes and counts (the offsets) - all as exact values."""
import json
import os

import pytest
import torch

import decode_wrapper_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "decode_wrappers.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights():
    return C.pipeline_weights()


def test_the_fixture_holds_every_case(recorded):
    assert list(recorded["tsp"]) == [f"{family}/{form}" for family, form in C.TSP_RUNS]
    assert list(recorded["mis"]) == [f"{graph}/{how}" for graph, how in C.MIS_RUNS]
    assert list(recorded["pipeline"]) == [f"{setting}/{entry}" for setting, entry in C.PIPELINE_RUNS]
    assert max(recorded["inputs"]["seeds"]) >= 2 ** 63


@pytest.mark.parametrize("family,form", C.TSP_RUNS, ids=[f"{a}-{b}" for a, b in C.TSP_RUNS])
def test_tsp_wrapper(recorded, dev, family, form):
    assert C.tsp_run(dev, recorded["inputs"], family, form) == recorded["tsp"][f"{family}/{form}"]


def test_guided_shape_refusals(recorded, dev):
    got = {name: C.refusal(call) for name, call in C.tsp_gpu_refusal_calls(dev, recorded["inputs"]).items()}
    assert got == recorded["tsp_refusals"]
    assert all(kind == "ValueError" for kind, _ in got.values())


@pytest.mark.parametrize("graph,how", C.MIS_RUNS, ids=[f"{a}-{b}" for a, b in C.MIS_RUNS])
def test_mis_wrappers(recorded, dev, graph, how):
    want = recorded["mis"][f"{graph}/{how}"]
    got = C.mis_run(dev, recorded["inputs"], graph, how)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k


@pytest.mark.parametrize("setting,entry", C.PIPELINE_RUNS, ids=[f"{a}-{b}" for a, b in C.PIPELINE_RUNS])
def test_pipeline(recorded, dev, weights, setting, entry):
    assert C.pipeline_run(dev, recorded["inputs"], weights, setting, entry) == recorded["pipeline"][f"{setting}/{entry}"]
