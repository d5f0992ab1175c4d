#!/usr/bin/env python
"""Records tests/golden/resident_entries.json: what ``difusco_tsp_two_opt_resident`` and ``difusco_tsp_local_search_resident``
reserve, refuse and compute on a few tiny calls (the cases: tests/resident_entries_cases.py), as exact values, from the library
that is built in the tree or the one ``DIFUSCO_HIP_LIBRARY`` names.  tests/test_gpu_resident_entries.py compares a later library
with them, so record only from a commit whose behaviour is the intended one, and name it:

    python scripts/record_resident_entries.py --commit $(git rev-parse HEAD)

The inputs of the runs are written into the fixture (points on a 2^-16 grid: short and exact in JSON); a fixture that exists
keeps its inputs unless ``--new_inputs`` is given.  ``--host_only`` records the sizes and refusals alone (no GPU) and keeps the
runs of the fixture that exists.  tests/test_resident_entries_host.py checks every recorded run against the numpy restatements
of the rules, so a bad recording does not become the standard."""
import argparse
import json
import os
import sys

import numpy as np
import torch      # before the library: both then share one HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import resident_entries_cases as C  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", required=True, help="the commit the library was built from")
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "resident_entries.json"))
ap.add_argument("--new_inputs", action="store_true")
ap.add_argument("--host_only", action="store_true")
opts = ap.parse_args()


def make_inputs():
    rng = np.random.default_rng(20261021)
    inputs = {}
    for name, (n, P) in C.GROUPS.items():
        if name == "poly7":     # a convex polygon visited in order: no 2-opt or Or-opt move shortens it
            ang = np.sort(rng.choice(64, n, replace=False)) * (2 * np.pi / 64)
            q16 = np.round((0.5 + 0.45 * np.stack([np.cos(ang), np.sin(ang)], 1)) * 65536).astype(np.int64)
            tours = np.tile(np.concatenate([np.arange(n), [0]]), (P, 1))
        else:
            q16 = rng.choice(65536, (n, 2), replace=False)
            tours = np.stack([np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(P)])
        inputs[name] = {"points_q16": q16.tolist(), "tours": tours.tolist()}
        if name == "tiny33":
            inputs[name]["scale_log2"] = C.TINY_LOG2
    return inputs


old = None
if os.path.exists(opts.out):
    with open(opts.out) as f:
        old = json.load(f)
from difusco_amd import _lib  # noqa: E402

L = _lib.lib()
doc = {"commit": opts.commit, "inputs": make_inputs() if old is None or opts.new_inputs else old["inputs"],
       "max_cells": C.max_cells(L), "workspace_bytes": C.workspace_sizes(L), "workspace_bytes_refusals": C.size_refusals(L),
       "refusals": C.refusals(L)}
if opts.host_only:
    doc["tours"], doc["runs"] = (old["tours"], old["runs"]) if old else ([], {})
else:
    dev = torch.device("cuda:0")
    doc["tours"], doc["runs"] = C.pack_runs({C.run_name(*r): C.short_run(dev, doc["inputs"], *r) for r in C.RUNS})
os.makedirs(os.path.dirname(opts.out), exist_ok=True)
with open(opts.out, "w") as f:
    f.write(json.dumps(doc, separators=(",", ":")) + "\n")
print(f"{opts.out}: {os.path.getsize(opts.out)} bytes, {len(doc['runs'])} runs")
