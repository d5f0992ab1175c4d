#!/usr/bin/env python
"""The CPU table of DESIGN 5.2f: sweeps, moves, rounds and end length of the multi-move local search
(tests/multi_local_search_emulation.py, S = 4) beside the multi-move 2-opt alone (tests/multi_two_opt_emulation.py) and the exact
2-opt + Or-opt search (tests/or_opt_emulation.py, one move per sweep).  Uniform points from ``np.random.default_rng(n)``;
nearest-neighbour or random-permutation start.  No GPU.  Prints one JSON line per row; arguments: the indices of the rows to
compute (default: all).  The exact search is not run at n = 3000 (one O(n^2) sweep per move)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multi_local_search_emulation as E  # noqa: E402
import multi_two_opt_emulation as M  # noqa: E402
import or_opt_emulation as O  # noqa: E402

ROWS = [(300, "nearest", True), (1000, "nearest", True), (1000, "random", True), (3000, "nearest", False)]
S = 4
for n, kind, exact in [ROWS[int(a)] for a in sys.argv[1:]] or ROWS:
    rng = np.random.default_rng(n)
    pts = rng.random((n, 2))
    start = M.nearest_neighbour_tour(pts) if kind == "nearest" else np.concatenate([[0], rng.permutation(n - 1) + 1, [0]])
    row = {"n": n, "start": kind, "select_rounds": S, "start_length": M.tour_length(pts, start)}
    if exact:
        moves = []
        t, two, orr, rounds = O.local_search(pts, start[None], 10 ** 6, 16, moves=moves)
        row["2opt+oropt"] = {"two_opt_moves": int(two), "or_opt_iterations": int(orr), "or_opt_moves": len(moves), "rounds": rounds,
                             "length": M.tour_length(pts, t[0])}
    t, sweeps, moves = M.multi_two_opt(pts, start[None], 10 ** 6, S)
    row["multi2opt"] = {"sweeps": sweeps, "moves": moves, "length": M.tour_length(pts, t[0])}
    phases = []
    t, c = E.search_tour(pts, start, 10 ** 6, 16, S, phases=phases)
    row["multi2opt+oropt"] = dict(c, phases=phases, length=M.tour_length(pts, t))
    print(json.dumps(row), flush=True)
