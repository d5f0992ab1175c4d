"""CPU restatement of the iterated MIS swap search (``difusco_mis_iterated_search``; the rule is stated in include/difusco_hip.h)
in numpy and adjacency sets, on top of the restatement of the descent (tests/mis_local_search_emulation.py) and the host Philox
(tests/philox_reference.py).  TEST INFRASTRUCTURE ONLY.

    descent        ``local_search`` exactly: one insertion phase, then swap rounds until a round proposes nothing or
                   ``max_rounds`` rounds ran; ranks fixed from the scores
    incumbent I    the descent of the input set
    kick t         draw     node v of instance b, local index r: w_v = word 0 of Philox4x32-10(seeds[b], offsets[b] + t, r) >> 8
                   kicked   v outside I and w_v * m_b < kick_size * 2^24 (m_b: nodes of b outside I), in exact integers
                   entered  a kicked v no kicked neighbour u of which has (w_u, u) < (w_v, v)
                   evict    C = I minus the members adjacent to an entered node, plus the entered nodes
                   descend  the descent on C
                   keep     per instance: I_b <- C_b iff |C_b| >= |I_b|

``draw(b, t, n_b)`` (optional) replaces the Philox draw of instance b at kick t by an integer array [n_b] of 24-bit values: the
hook of the hand cases."""
import numpy as np

import mis_local_search_emulation as M
import philox_reference as P

TWO_24 = 1 << 24


def philox_draw(seeds, offsets):
    def draw(b, t, n_b):
        off = (int(offsets[b]) + t) % (1 << 64)
        return (P.words(int(seeds[b]), off, n_b)[:, 0].astype(np.int64) >> 8) if n_b else np.zeros(0, dtype=np.int64)
    return draw


def is_kicked(w, m, kick_size):
    """The exact-integer test of one node outside the incumbent (python ints: no rounding, no wrap)."""
    return int(w) * int(m) < int(kick_size) * TWO_24


def entered_nodes(adj, kicked):
    """``kicked``: {v: w_v}.  -> the sorted list of the kicked nodes that enter."""
    return sorted(v for v, w in kicked.items() if not any(u in kicked and (kicked[u], u) < (w, v) for u in adj[v]))


def iterated_search(n, edge_index, scores, solution, instance_rows=None, seeds=None, offsets=None, kicks=0, kick_size=4,
                    max_rounds=None, draw=None):
    """-> (solution int array [n], (rounds, swaps, inserts), per_instance int array [B, 4] = entered, accepted, size_before,
    size_after).  ``max_rounds=None``: unbounded descents."""
    adj = edge_index if isinstance(edge_index, list) else M.adjacency(n, edge_index)
    rows = [0, n] if instance_rows is None else [int(v) for v in instance_rows]
    B = len(rows) - 1
    assert B >= 1 and rows[0] == 0 and rows[-1] == n and all(a <= b for a, b in zip(rows, rows[1:])), "malformed instance table"
    assert kicks >= 0 and kick_size >= 1
    seeds = [0] * B if seeds is None else list(seeds)
    offsets = [0] * B if offsets is None else list(offsets)
    assert len(seeds) == len(offsets) == B
    draw = philox_draw(seeds, offsets) if draw is None else draw
    inc, rounds, swaps, inserts = M.local_search(n, adj, scores, solution, max_rounds)
    per = np.zeros((B, 4), dtype=np.int64)
    per[:, 2] = [int(inc[rows[b]:rows[b + 1]].sum()) for b in range(B)]
    for t in range(kicks):
        kicked = {}
        for b in range(B):
            lo, hi = rows[b], rows[b + 1]
            m = (hi - lo) - int(inc[lo:hi].sum())
            w = np.asarray(draw(b, t, hi - lo)).reshape(-1)
            assert len(w) == hi - lo and all(0 <= int(x) < TWO_24 for x in w)
            kicked.update({v: int(w[v - lo]) for v in range(lo, hi) if not inc[v] and is_kicked(w[v - lo], m, kick_size)})
        ent = entered_nodes(adj, kicked)
        cand = inc.copy()
        for v in ent:
            for u in adj[v]:
                cand[u] = 0
        for v in ent:
            cand[v] = 1
        cand, r, s, i = M.local_search(n, adj, scores, cand, max_rounds)
        rounds, swaps, inserts = rounds + r, swaps + s, inserts + i
        for b in range(B):
            lo, hi = rows[b], rows[b + 1]
            keep = int(cand[lo:hi].sum()) >= int(inc[lo:hi].sum())
            if any(lo <= v < hi for v in ent):
                per[b, 0] += 1
                per[b, 1] += keep
            if keep:
                inc[lo:hi] = cand[lo:hi]
    per[:, 3] = [int(inc[rows[b]:rows[b + 1]].sum()) for b in range(B)]
    return inc, (rounds, swaps, inserts), per
