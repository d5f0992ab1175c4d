#!/usr/bin/env python
"""Generates tests/golden/tsp_merge_zoo.npz with the REFERENCE's own decode - ``merge_tours`` calling ``merge_cython`` compiled
from the reference's .pyx into a temporary directory, exactly as make_golden_decode.py loads them (nothing of the reference is
copied into the repo) - on the cases ``FIXTURE_PAIRS`` of tests/tsp_merge_cases.py: coincident cities, NaN and infinite heat.
The reference sorts with numpy's default, unstable argsort, so only cases whose result cannot depend on the order of equal keys
are recorded (``tsp_merge_cases.recorded_case`` asserts it).  Runs in the build container only.  One file, per case the arrays
``<case>__points`` (float32), ``__edge_index`` (int32), ``__heat`` (float32), ``__tour`` (int32), ``__iterations`` (int64),
``__negative_key_entries`` (int64: entries of the reference's dense list with a key < 0) and ``__completed``; written with a
fixed member date, so a rerun gives the same bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden_decode import load_reference, save_npz_fixed  # noqa: E402


def main():
    import tsp_merge_cases as Z
    tu = load_reference()
    arrays = {"provenance": np.array("reference: tsp_utils.merge_tours + cython_merge.merge_cython (pyx compiled here) on "
                                     "tests/tsp_merge_cases.FIXTURE_PAIRS")}
    for pair in Z.FIXTURE_PAIRS:
        c = Z.recorded_case(*pair)
        name = Z.case_id(pair)
        pts, ei, heat = c["points"], c["edge_index"], c["heat"]
        n = pts.shape[0]
        with np.errstate(all="ignore"):
            tours, it = tu.merge_tours(heat.copy(), pts.copy(), ei.copy(), sparse_graph=True, parallel_sampling=1)
            a = np.zeros((n, n), dtype=np.float32)
            np.add.at(a, (ei[0], ei[1]), heat)
            p64 = pts.astype(np.float64)
            key = -(a + a.T).astype(np.float64) / np.linalg.norm(p64[:, None] - p64, axis=-1)
        neg = int((key < 0).sum())
        arrays[f"{name}__points"] = pts
        arrays[f"{name}__edge_index"] = ei.astype(np.int32)
        arrays[f"{name}__heat"] = heat
        arrays[f"{name}__tour"] = np.asarray(tours[0], dtype=np.int32)
        arrays[f"{name}__iterations"] = np.int64(it)
        arrays[f"{name}__negative_key_entries"] = np.int64(neg)
        arrays[f"{name}__completed"] = np.bool_(it <= neg)
        print(name, "n", n, "E", ei.shape[1], "merge_iterations", int(it), "negative-key entries", neg, "completed", bool(it <= neg),
              "oracle", c["want"][1:], "same tour" if list(map(int, tours[0])) == c["want"][0] else "TOUR DIFFERS")
    save_npz_fixed(os.path.join(HERE, "tsp_merge_zoo.npz"), arrays)


if __name__ == "__main__":
    main()
