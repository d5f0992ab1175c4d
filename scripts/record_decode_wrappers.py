#!/usr/bin/env python
"""Records tests/golden/decode_wrappers.json and tests/golden/decode_wrapper_refusals.json: what the Python wrappers of
``difusco_amd.decode`` and the local-search part of ``difusco_amd.pipeline`` return and refuse on a few tiny calls (the cases:
tests/decode_wrapper_cases.py), as exact values with their types.  tests/test_gpu_decode_wrappers.py and
tests/test_decode_wrappers_host.py compare a later host side with them, so record only from a commit whose behaviour is the
intended one, and name it:

    python scripts/record_decode_wrappers.py --commit $(git rev-parse HEAD)

Needs a GPU, also for the refusals: some of them are raised only after an upload in the commit they are recorded from.  While
they are recorded every function of the library raises, so a refusal that reaches one is seen.  Every GPU case runs twice and
nothing is written unless both runs agree.  The inputs are written into the fixture (points on a 2^-16 grid, heat and scores
as integers over 256: short and exact in JSON); a fixture that exists keeps its inputs unless ``--new_inputs`` is given."""
import argparse
import json
import os
import sys

import numpy as np
import torch      # before the library: both then share one HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import decode_wrapper_cases as C  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", required=True, help="the commit the wrappers are recorded from")
ap.add_argument("--out_dir", default=os.path.join(ROOT, "tests", "golden"))
ap.add_argument("--new_inputs", action="store_true")
opts = ap.parse_args()


def make_inputs():
    rng = np.random.default_rng(20261019)
    tsp = {}
    for name, n, P in (("a4", 4, 3), ("b40", 40, 1), ("c17", 17, 3), ("d17", 17, 2)):
        pts = rng.choice(65536, (n, 2), replace=False) / 65536
        tours = []
        while len(tours) < P:                                        # P different closed tours from city 0
            t = [0] + (rng.permutation(n - 1) + 1).tolist() + [0]
            if t not in tours:
                tours.append(t)
        d = np.linalg.norm(pts[:, None] - pts[None], axis=2)
        np.fill_diagonal(d, np.inf)
        K = min(4, n - 1)
        row, col = np.repeat(np.arange(n), K), np.argsort(d, axis=1, kind="stable")[:, :K].reshape(-1)
        order = rng.permutation(n * K)                               # an edge list that is not sorted by row
        tsp[name] = {"points": pts.tolist(), "tours": tours, "edge_index": [row[order].tolist(), col[order].tolist()],
                     "sparse_heat": rng.integers(0, C.HEAT_GRID + 1, (P, n * K)).tolist(),
                     "dense_heat": rng.integers(0, C.HEAT_GRID + 1, (P, n, n)).tolist()}

    def graph(n, p):
        upper = np.triu(rng.random((n, n)) < p, 1)
        row, col = np.nonzero(upper | upper.T)
        scores = rng.integers(0, C.HEAT_GRID + 1, n)
        sol = np.zeros(n, dtype=np.int64)                            # the greedy set by falling score, then rising id
        for v in np.argsort(-scores, kind="stable"):
            if not sol[col[row == v]].any():
                sol[v] = 1
        return row, col, scores, sol
    r30, c30, s30, sol30 = graph(30, 0.15)
    r12, c12, s12, sol12 = graph(12, 0.3)
    mis = {"g30": {"scores": s30.tolist(), "edge_index": [r30.tolist(), c30.tolist()], "solution": sol30.tolist()},
           "empty": {"scores": rng.integers(0, C.HEAT_GRID + 1, 5).tolist(), "edge_index": [[], []], "solution": [0] * 5},
           "two": {"scores": s30.tolist() + s12.tolist(), "edge_index": [r30.tolist() + (r12 + 30).tolist(), c30.tolist() + (c12 + 30).tolist()],
                   "solution": sol30.tolist() + sol12.tolist(), "instance_rows": [0, 30, 42]}}
    seeds = [int(x) for x in rng.integers(0, 2 ** 63, 6)]
    seeds[1] += 2 ** 63                                              # the 64-bit mask
    return {"tsp": tsp, "mis": mis, "seeds": seeds, "offsets": [(1 << 62) + (p << 32) + 7 * p for p in range(6)],
            "pipeline_points": (rng.choice(65536, (2, C.PIPELINE_N, 2), replace=False) / 65536).tolist()}


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def load(name):
    path = os.path.join(opts.out_dir, name)
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


def save(name, doc):
    path = os.path.join(opts.out_dir, name)
    with open(path, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")) + "\n")
    print(f"{path}: {os.path.getsize(path)} bytes")


from difusco_amd import _lib  # noqa: E402

real = _lib.lib
_lib.lib = lambda: NoLibrary()
try:
    refused = C.host_refusals()
finally:
    _lib.lib = real
bad = {k: v for k, v in refused.items() if v[0] in ("no exception", "AssertionError")}
if bad:
    sys.exit(f"not refused before the library: {bad}")

old = load("decode_wrappers.json")
inputs = make_inputs() if old is None or opts.new_inputs else old["inputs"]
dev = torch.device("cuda:0")
first, second = C.gpu_results(dev, inputs), C.gpu_results(dev, inputs)
if first != second:
    diff = [f"{part}/{name}" for part in first for name in first[part] if first[part][name] != second[part][name]]
    sys.exit(f"two runs of the same cases differ, nothing written: {diff}")
os.makedirs(opts.out_dir, exist_ok=True)
save("decode_wrapper_refusals.json", {"commit": opts.commit, "refusals": refused})
save("decode_wrappers.json", dict({"commit": opts.commit, "inputs": inputs}, **first))
