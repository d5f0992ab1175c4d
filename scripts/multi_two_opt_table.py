#!/usr/bin/env python
"""The CPU table of DESIGN 5.2e: sweeps and end length of the multi-move 2-opt (tests/multi_two_opt_emulation.py) by the number
of selection rounds S, beside the reference rule (one best move per sweep, ``oracle.tsp_decode_oracle.batched_two_opt``).
Uniform points from ``np.random.default_rng(n)``; nearest-neighbour or random-permutation start.  No GPU.  Prints one JSON line
per row; arguments: the indices of the rows to compute (default: all)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multi_two_opt_emulation as E  # noqa: E402
from oracle.tsp_decode_oracle import batched_two_opt  # noqa: E402

ROWS = [(1000, "nearest"), (1000, "random"), (3000, "nearest")]
ROUNDS = [1, 2, 4, 8, 10 ** 6]
for n, kind in [ROWS[int(a)] for a in sys.argv[1:]] or ROWS:
    rng = np.random.default_rng(n)
    pts = rng.random((n, 2))
    start = E.nearest_neighbour_tour(pts) if kind == "nearest" else np.concatenate([[0], rng.permutation(n - 1) + 1, [0]])
    row = {"n": n, "start": kind, "start_length": E.tour_length(pts, start)}
    ref, its = batched_two_opt(pts, start[None], 10 ** 6)
    row["reference"] = {"sweeps": int(its), "moves": int(its), "length": E.tour_length(pts, ref[0])}
    for S in ROUNDS:
        t, sweeps, moves = E.multi_two_opt(pts, start[None], 10 ** 6, S)
        row["unbounded" if S == 10 ** 6 else f"S={S}"] = {"sweeps": sweeps, "moves": moves, "length": E.tour_length(pts, t[0])}
    print(json.dumps(row), flush=True)
