"""CPU restatement of the (1,2)-swap local search for MIS solutions (difusco_amd/csrc/mis_local_search.hip,
``difusco_mis_local_search``; the rule is stated in include/difusco_hip.h) in numpy and adjacency sets.  TEST INFRASTRUCTURE ONLY.

``rank[v]`` is the position of ``v`` in the stable descending sort of the scores (equal scores keep index order; a smaller rank is
a higher priority).  On the current set S, ``tight[v]`` counts the neighbours ``u != v`` of ``v`` in S; a node outside S is *free*
with ``tight == 0`` and a *candidate* of its one solution neighbour with ``tight == 1``; ``L(x)`` is the set of candidates of x.

    insertion phase   the lexicographically first maximal independent set, by rank, of the subgraph the free nodes induce goes in
    round             every x in S proposes the pair (u, w) of L(x), u and w not adjacent, rank[u] < rank[w], smallest in
                      (rank[u], rank[w]); two proposals conflict iff a node of one is adjacent to a node of the other; x is applied
                      iff rank[u_x] < rank[u_y] for every conflicting y; all winners at once (x out, u_x and w_x in); insertion phase

One insertion phase, then rounds until a round proposes nothing (it is not counted) or ``max_rounds`` rounds ran."""
import numpy as np


def adjacency(n, edge_index):
    """Neighbour sets of the symmetric adjacency ``edge_index`` [2, E]; self loops are dropped, duplicates collapse."""
    adj = [set() for _ in range(n)]
    ei = np.asarray(edge_index).reshape(2, -1)
    for a, b in zip(ei[0].tolist(), ei[1].tolist()):
        if a != b:
            adj[a].add(b)
            adj[b].add(a)
    return adj


def ranks(scores):
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    order = np.argsort(-s, kind="stable")
    rank = np.empty(len(s), dtype=np.int64)
    rank[order] = np.arange(len(s))
    return rank


def tightness(adj, sol):
    return np.array([sum(int(sol[u]) for u in adj[v]) for v in range(len(adj))], dtype=np.int64)


def insertion_phase(adj, rank, sol):
    """Inserts, in rank order, every free node none of whose neighbours is in the set by then.  Returns the number inserted."""
    tight = tightness(adj, sol)
    free = [v for v in np.argsort(rank).tolist() if not sol[v] and tight[v] == 0]
    added = 0
    for v in free:
        if not any(sol[u] for u in adj[v]):
            sol[v] = 1
            added += 1
    return added


def proposals(adj, rank, sol):
    """{x: (u, w)}: the minimal pair of every x in S that has one."""
    tight = tightness(adj, sol)
    cand = {}
    for v in range(len(adj)):
        if not sol[v] and tight[v] == 1:
            x = next(u for u in adj[v] if sol[u])
            cand.setdefault(x, []).append(v)
    out = {}
    for x, L in cand.items():
        L.sort(key=lambda v: rank[v])
        pair = next(((u, w) for i, u in enumerate(L) for w in L[i + 1:] if w not in adj[u]), None)
        if pair is not None:
            out[x] = pair
    return out


def winners(adj, rank, props):
    proposer = {v: x for x, pair in props.items() for v in pair}
    win = []
    for x, pair in props.items():
        rivals = {proposer[b] for a in pair for b in adj[a] if b in proposer} - {x}
        if all(rank[pair[0]] < rank[props[y][0]] for y in rivals):
            win.append(x)
    return win


def local_search(n, edge_index, scores, solution, max_rounds=None):
    """-> (solution int array [n], rounds, swaps, inserts).  ``max_rounds=None``: unbounded."""
    adj = edge_index if isinstance(edge_index, list) else adjacency(n, edge_index)
    rank = ranks(scores)
    sol = np.array(solution, dtype=np.int64).reshape(-1).copy()
    assert len(sol) == n == len(rank)
    assert not any(sol[v] and sol[u] for v in range(n) for u in adj[v]), "the start set is not independent"
    rounds = swaps = 0
    inserts = insertion_phase(adj, rank, sol)
    while max_rounds is None or rounds < max_rounds:
        props = proposals(adj, rank, sol)
        if not props:
            break
        win = winners(adj, rank, props)
        assert win
        for x in win:
            sol[x] = 0
        for x in win:
            sol[props[x][0]] = sol[props[x][1]] = 1
        rounds += 1
        swaps += len(win)
        inserts += insertion_phase(adj, rank, sol)
    return sol, rounds, swaps, inserts


# ---- properties the tests assert ---------------------------------------------------------------------------------------------
def is_independent(adj, sol):
    return not any(sol[v] and sol[u] for v in range(len(adj)) for u in adj[v])


def is_maximal(adj, sol):
    return all(sol[v] or any(sol[u] for u in adj[v]) for v in range(len(adj)))


def remaining_swaps(adj, sol):
    """Brute force over all x in S and all u, w outside it: the (1,2)-swaps the set still admits."""
    n = len(adj)
    out = []
    for x in range(n):
        if not sol[x]:
            continue
        ok = [v for v in adj[x] if not sol[v] and all(not sol[t] or t == x for t in adj[v])]
        out += [(x, u, w) for u in ok for w in ok if u < w and w not in adj[u]]
    return out
