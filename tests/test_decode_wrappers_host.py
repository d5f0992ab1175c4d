"""Every refusal that the wrappers of ``difusco_amd.decode`` raise from their arguments alone - all ``batched_*`` families as
``_torch``, ``_grouped`` and ``_ragged``, ``mis_local_search_np`` and ``mis_iterated_search_np`` - against the recorded exception
types and messages (tests/golden/decode_wrapper_refusals.json, scripts/record_decode_wrappers.py; the cases:
tests/decode_wrapper_cases.py).  No GPU: the library raises if it is reached, and so would an upload.

The shape errors of a guided call's ``heat`` / ``edge_index`` past the two list lengths are raised on uploaded arrays; they are
in tests/test_gpu_decode_wrappers.py."""
import json
import os

import pytest

import decode_wrapper_cases as C
from difusco_amd import _lib


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "decode_wrapper_refusals.json")) as f:
        return json.load(f)["refusals"]


def test_refusals_raise_what_was_recorded_before_any_library_call(recorded, monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    got = C.host_refusals()
    assert list(got) == list(recorded)
    wrong = {name: (got[name], recorded[name]) for name in recorded if got[name] != recorded[name]}
    assert not wrong


def test_the_recorded_refusals_are_refusals(recorded):
    assert len(recorded) > 250
    for name, (kind, text) in recorded.items():
        assert kind in ("ValueError", "DifuscoHipError") and text, name
        if name.endswith("/cpu"):
            assert kind == "DifuscoHipError" and "GPU only" in text and name.split("/")[0] in text, name
