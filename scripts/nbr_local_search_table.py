#!/usr/bin/env python
"""The CPU table of DESIGN 5.2p: sweeps by stage and kind, moves, rounds and end length of the neighbour-list multi-move 2-opt +
Or-opt search (tests/nbr_local_search_emulation.py) by the list length K, without and with the closing full stage, beside the
multi-move local search (tests/multi_local_search_emulation.py).  Uniform points from ``np.random.default_rng(n)``;
nearest-neighbour or random-permutation start; lists = the K nearest other cities; ``select_rounds`` = 4, ``max_rounds`` = 16.
No GPU.  Prints one JSON line per row; arguments: the indices of the rows to compute (default: all)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multi_local_search_emulation as M  # noqa: E402
import multi_two_opt_emulation as E  # noqa: E402
import nbr_local_search_emulation as NL  # noqa: E402

ROWS = [(1000, "nearest"), (1000, "random"), (3000, "nearest")]
KS = [5, 8, 16]
for n, kind in [ROWS[int(a)] for a in sys.argv[1:]] or ROWS:
    rng = np.random.default_rng(n)
    pts = rng.random((n, 2))
    start = E.nearest_neighbour_tour(pts) if kind == "nearest" else np.concatenate([[0], rng.permutation(n - 1) + 1, [0]])
    row = {"n": n, "start": kind, "start_length": E.tour_length(pts, start)}
    t, c = M.search_tour(pts, start, 10 ** 6, 16, 4)
    row["multi2opt+oropt"] = {"two_opt_sweeps": c["two_opt_sweeps"], "or_opt_sweeps": c["or_opt_sweeps"], "rounds": c["rounds"],
                              "moves": c["two_opt_moves"] + c["or_opt_moves"], "length": E.tour_length(pts, t)}
    lists = NL.knn_lists(pts, max(KS))
    for K in KS:
        for closing in (False, True):
            log = []
            t, c = NL.search_tour(pts, start, lists[:, :K], closing, 10 ** 6, 16, 4, log=log)
            count = lambda stage, kind_: sum(1 for e in log if e[:2] == (stage, kind_))
            row[f"K={K}" + (" closing" if closing else "")] = {
                "nbr_two_opt_sweeps": count("nbr", "2opt"), "nbr_or_opt_sweeps": count("nbr", "oropt"),
                "full_two_opt_sweeps": count("full", "2opt"), "full_or_opt_sweeps": count("full", "oropt"),
                "rounds": c["rounds"], "full_rounds": c["full_rounds"], "moves": c["two_opt_moves"] + c["or_opt_moves"],
                "length": E.tour_length(pts, t)}
    print(json.dumps(row), flush=True)
