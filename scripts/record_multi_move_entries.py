#!/usr/bin/env python
"""Records tests/golden/multi_move_entries.json: what ``difusco_tsp_multi_two_opt_ragged``, ``difusco_tsp_nbr_two_opt_ragged`` and
``difusco_tsp_nbr_local_search_ragged`` reserve, refuse and compute on a few tiny calls (the cases:
tests/multi_move_entries_cases.py), as exact values, from the library that is built in the tree.
tests/test_gpu_multi_move_entries.py compares a later library with them, so record only from a commit whose behaviour is the
intended one, and name it:

    python scripts/record_multi_move_entries.py --commit $(git rev-parse HEAD)

The inputs of the runs are written into the fixture (points on a 2^-16 grid: short and exact in JSON); a fixture that exists
keeps its inputs unless ``--new_inputs`` is given.  ``--host_only`` records the sizes and refusals alone (no GPU) and keeps the
runs of the fixture that exists.  tests/test_multi_move_entries_host.py checks every recorded run against the numpy restatements
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

import multi_move_entries_cases as C  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", required=True, help="the commit the library was built from")
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "multi_move_entries.json"))
ap.add_argument("--new_inputs", action="store_true")
ap.add_argument("--host_only", action="store_true")
opts = ap.parse_args()

PAD_ROWS = ((5, "minus_one"), (11, "n"), (20, "self"))      # rows of the n = 33 group's lists that hold pads only


def make_inputs():
    """The three groups of scripts/record_tsp_search_entries.py (same recipe, same seed) with the K nearest other cities."""
    rng = np.random.default_rng(20261019)
    K = C.RUN_KS[-1]
    groups = []
    for n, P in ((4, 2), (7, 1), (33, 3)):
        if n == 7:      # a convex polygon visited in order: no 2-opt or Or-opt move shortens it
            ang = np.sort(rng.choice(64, n, replace=False)) * (2 * np.pi / 64)
            pts = np.round((0.5 + 0.45 * np.stack([np.cos(ang), np.sin(ang)], 1)) * 65536) / 65536
            tours = np.tile(np.concatenate([np.arange(n), [0]]), (P, 1))
        else:
            pts = rng.choice(65536, (n, 2), replace=False) / 65536
            tours = np.stack([np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(P)])
        d = np.linalg.norm(pts[:, None] - pts[None], axis=2)
        np.fill_diagonal(d, np.inf)
        nbr = np.argsort(d, axis=1, kind="stable")[:, :K]          # by rising distance
        if n == 33:     # pads: nothing may be indexed with them
            for row, kind in PAD_ROWS:
                nbr[row] = {"minus_one": -1, "n": n, "self": row}[kind]
        groups.append({"points_q16": np.round(pts * 65536).astype(np.int64).tolist(), "tours": tours.tolist(), "neighbors": nbr.tolist()})
    return {"groups": groups}


old = None
if os.path.exists(opts.out):
    with open(opts.out) as f:
        old = json.load(f)
from difusco_amd import _lib  # noqa: E402

L = _lib.lib()
doc = {"commit": opts.commit, "inputs": make_inputs() if old is None or opts.new_inputs else old["inputs"],
       "workspace_bytes": C.workspace_sizes(L), "workspace_bytes_refusals": C.size_refusals(L), "refusals": C.refusals(L)}
if opts.host_only:
    doc["runs"] = old["runs"] if old else {}
else:
    dev = torch.device("cuda:0")
    doc["runs"] = {C.run_name(*r): C.short_run(dev, doc["inputs"], *r) for r in C.RUNS}
os.makedirs(os.path.dirname(opts.out), exist_ok=True)
with open(opts.out, "w") as f:
    f.write(json.dumps(doc, separators=(",", ":")) + "\n")
print(f"{opts.out}: {os.path.getsize(opts.out)} bytes, {len(doc['runs'])} runs")
