#!/usr/bin/env python
"""The CPU table of DESIGN 5.2o: sweeps and end length of the neighbour-list multi-move 2-opt (tests/nbr_two_opt_emulation.py)
by the list length K, without and with the closing full descent, beside the multi-move 2-opt (tests/multi_two_opt_emulation.py).
Uniform points from ``np.random.default_rng(n)``; nearest-neighbour or random-permutation start; lists = the K nearest other
cities; ``select_rounds`` = 4.  No GPU.  Prints one JSON line per row; arguments: the indices of the rows to compute (default:
all)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multi_two_opt_emulation as E  # noqa: E402
import nbr_two_opt_emulation as NB  # noqa: E402

ROWS = [(1000, "nearest"), (1000, "random"), (3000, "nearest")]
KS = [5, 8, 16]
for n, kind in [ROWS[int(a)] for a in sys.argv[1:]] or ROWS:
    rng = np.random.default_rng(n)
    pts = rng.random((n, 2))
    start = E.nearest_neighbour_tour(pts) if kind == "nearest" else np.concatenate([[0], rng.permutation(n - 1) + 1, [0]])
    row = {"n": n, "start": kind, "start_length": E.tour_length(pts, start)}
    t, sweeps, moves = E.multi_two_opt(pts, start[None], 10 ** 6, 4)
    row["multi2opt"] = {"sweeps": sweeps, "moves": moves, "length": E.tour_length(pts, t[0])}
    lists = NB.knn_lists(pts, max(KS))
    for K in KS:
        for closing in (False, True):
            t, sweeps, full, moves = NB.nbr_two_opt(pts, start[None], lists[:, :K], closing, 10 ** 6, 4)
            row[f"K={K}" + (" closing" if closing else "")] = {"neighbour_sweeps": sweeps - full, "full_sweeps": full, "moves": moves,
                                                              "length": E.tour_length(pts, t[0])}
    print(json.dumps(row), flush=True)
