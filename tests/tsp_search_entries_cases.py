"""The cases of tests/golden/tsp_search_entries.json: what the four multi-move TSP search entries (``difusco_tsp_multi_local_search_ragged``,
``_iterated_``, ``_focused_`` and ``_guided_search_ragged``) reserve, refuse and compute on a handful of tiny calls.
scripts/record_tsp_search_entries.py records them, tests/test_gpu_tsp_search_entries.py replays them; both call the functions here, so
the fixture and the test cannot drift apart.  Nothing here draws a random number: the inputs of the runs are in the fixture."""
import ctypes

import numpy as np

ENTRIES = ("multi_local_search", "iterated_search", "focused_search", "guided_search")
KEYS = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")
GUIDED_K = 8                                # the second guided size is recorded with group_edges = K n

# (group_n, group_tours): the minimum, around the 16-row tile, past one 1024-column chunk, mixes of two and three groups
SHAPES = [([4], [1]), ([16], [1]), ([17], [2]), ([18], [3]), ([1025], [1]), ([4, 1025], [3, 1]), ([16, 17, 18], [1, 2, 3]),
          ([1025, 4, 17], [2, 3, 1])]


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def workspace_bytes(L, entry, group_n, group_tours, group_edges=None):
    """[return code, bytes] of the entry's ``_workspace_bytes``."""
    n, t, out = _i32(group_n), _i32(group_tours), ctypes.c_size_t(0)
    fn = getattr(L, f"difusco_tsp_{entry}_ragged_workspace_bytes")
    if entry == "guided_search":
        e = _i32(group_edges)
        return [fn(len(n), n.ctypes.data, t.ctypes.data, e.ctypes.data, ctypes.byref(out)), int(out.value)]
    return [fn(len(n), n.ctypes.data, t.ctypes.data, ctypes.byref(out)), int(out.value)]


def workspace_sizes(L):
    rows = []
    for group_n, group_tours in SHAPES:
        row = {"group_n": group_n, "group_tours": group_tours}
        for entry in ENTRIES[:3]:
            row[entry] = workspace_bytes(L, entry, group_n, group_tours)
        row["guided_search_no_edges"] = workspace_bytes(L, "guided_search", group_n, group_tours, [0] * len(group_n))
        row["guided_search_knn_edges"] = workspace_bytes(L, "guided_search", group_n, group_tours, [GUIDED_K * n for n in group_n])
        rows.append(row)
    return rows


# the valid call every refusal departs from in one argument
VALID = dict(groups=2, group_n=[5, 9], group_tours=[2, 1], max_iterations=10, max_rounds=2, select_rounds=4, kicks=1, kick_size=4,
             span=8, compact_select_max=1024, descent=1, group_edges=[20, 36], null_output=None, workspace_short=0)
COMMON = [("groups_0", dict(groups=0)), ("n_3", dict(group_n=[5, 3])), ("tours_0", dict(group_tours=[0, 1])),
          ("max_rounds_0", dict(max_rounds=0)), ("select_rounds_0", dict(select_rounds=0))]
KICKS = [("kicks_-1", dict(kicks=-1)), ("kick_size_0", dict(kick_size=0)), ("kick_size_65", dict(kick_size=65)),
         ("span_0", dict(span=0))]
COMPACT = [("compact_select_max_-1", dict(compact_select_max=-1)), ("compact_select_max_1025", dict(compact_select_max=1025))]
LAST = [("null_group_output", dict(null_output="or_opt_moves")), ("workspace_one_byte_short", dict(workspace_short=1))]
REFUSALS = {
    "multi_local_search": COMMON + LAST,
    "iterated_search": COMMON + KICKS + [("null_tour_output", dict(null_output="final_length"))] + LAST,
    "focused_search": COMMON + KICKS + COMPACT + [("null_tour_output", dict(null_output="closing_sweeps"))] + LAST,
    "guided_search": COMMON + KICKS + COMPACT + [("descent_2", dict(descent=2)), ("group_edges_-1", dict(group_edges=[20, -1])),
                                                 ("null_tour_output", dict(null_output="closing_sweeps"))] + LAST,
}


def refused_call(L, entry, **change):
    """The entry on VALID with ``change``; every array is a host array of the right length, which a refused call never reads.
    Returns [return code, the text of ``difusco_last_error``]."""
    a = dict(VALID, **change)
    group_n, group_tours, group_edges = _i32(a["group_n"]), _i32(a["group_tours"]), _i32(a["group_edges"])
    G = len(group_n)
    T, cells = int(np.maximum(group_tours, 0).sum()), int((np.maximum(group_n, 0) + 1) @ np.maximum(group_tours, 0))
    points, tours = np.zeros(2 * int(np.maximum(group_n, 0).sum()) + 2), np.zeros(cells + 1, dtype=np.int32)
    seeds, offsets = np.zeros(T + 1, dtype=np.uint64), np.zeros(T + 1, dtype=np.uint64)
    row_ptr, col, heat = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int32), np.zeros(256, dtype=np.float32)
    rc, need = workspace_bytes(L, entry, VALID["group_n"], VALID["group_tours"], VALID["group_edges"])
    assert rc == 0
    ws = np.zeros(need, dtype=np.uint8)
    out = {k: np.zeros(G + 1, dtype=np.int32 if k == "rounds" else np.int64) for k in KEYS}
    per = {"kicks_kept": np.zeros(T + 1, dtype=np.int32), "kicks_improved": np.zeros(T + 1, dtype=np.int32),
           "segments_swapped": np.zeros(T + 1, dtype=np.int64), "first_length": np.zeros(T + 1), "final_length": np.zeros(T + 1),
           "closing_sweeps": np.zeros(T + 1, dtype=np.int32)}
    ptr = lambda name, arr: None if a["null_output"] == name else arr.ctypes.data
    head = (a["groups"], group_n.ctypes.data, group_tours.ctypes.data, points.ctypes.data, tours.ctypes.data, a["max_iterations"],
            a["max_rounds"], a["select_rounds"])
    kick = (a["kicks"], a["kick_size"], a["span"], seeds.ctypes.data, offsets.ctypes.data)
    tail = (ws.ctypes.data, need - a["workspace_short"]) + tuple(ptr(k, out[k]) for k in KEYS)
    tail_per = tuple(ptr(k, per[k]) for k in ("kicks_kept", "kicks_improved", "segments_swapped", "first_length", "final_length"))
    closing = (ptr("closing_sweeps", per["closing_sweeps"]),)
    fn = getattr(L, f"difusco_tsp_{entry}_ragged")
    if entry == "multi_local_search":
        rc = fn(*head, *tail, None)
    elif entry == "iterated_search":
        rc = fn(*head, *kick, *tail, *tail_per, None)
    elif entry == "focused_search":
        rc = fn(*head, *kick, a["compact_select_max"], *tail, *tail_per, *closing, None)
    else:
        rc = fn(*head, *kick, a["compact_select_max"], a["descent"], group_edges.ctypes.data, row_ptr.ctypes.data, col.ctypes.data,
                heat.ctypes.data, *tail, *tail_per, *closing, None)
    return [int(rc), L.difusco_last_error().decode()]


def size_refusals(L):
    """The refusals of the four ``_workspace_bytes`` entries."""
    rows = {}
    for entry in ENTRIES:
        cases = [("groups_0", [], [], []), ("n_3", [5, 3], [2, 1], [20, 36]), ("tours_0", [5, 9], [0, 1], [20, 36])]
        if entry == "guided_search":
            cases.append(("group_edges_-1", [5, 9], [2, 1], [20, -1]))
        rows[entry] = {name: [workspace_bytes(L, entry, *args)[0], L.difusco_last_error().decode()] for name, *args in cases}
    return rows


def refusals(L):
    return {entry: {name: refused_call(L, entry, **change) for name, change in REFUSALS[entry]} for entry in ENTRIES}


# ---- the short runs: three groups (n = 4, 7, 33) in one call; the middle one is a convex polygon in order, a local optimum

MODES = [("plain", {}), ("iterated_full", dict(descent="full")), ("iterated_focused", dict(descent="focused")),
         ("guided_full", dict(descent="full", kick_bias="heat")), ("guided_focused", dict(descent="focused", kick_bias="heat"))]
RUNS = [(mode, kicks, cap) for mode, _ in MODES for kicks in ((None,) if mode == "plain" else (0, 3)) for cap in (0, 1000)]


def run_name(mode, kicks, cap):
    return f"{mode}_cap{cap}" if kicks is None else f"{mode}_kicks{kicks}_cap{cap}"


def short_run(dev, inputs, mode, kicks, cap):
    """One call on the fixture's inputs; every result as plain lists (float64 lengths as their hex strings)."""
    from difusco_amd import _lib
    from difusco_amd.decode import batched_iterated_search_ragged, batched_multi_local_search_ragged
    pts = [np.array(g["points"], dtype=np.float64) for g in inputs["groups"]]
    starts = [np.array(g["tours"], dtype=np.int64) for g in inputs["groups"]]
    common = dict(device=dev, max_rounds=inputs["max_rounds"], select_rounds=inputs["select_rounds"])
    L = _lib.lib()
    if mode == "plain":
        # the plain entry leaves the count of the thread's last iterated call alone: a call of keeps only comes first
        batched_iterated_search_ragged(pts, starts, 0, kicks=0, stats={}, **common)
        tours, stats = batched_multi_local_search_ragged(pts, starts, cap, **common)
        res = {"host_syncs_of_the_iterated_call_before": int(L.difusco_tsp_search_host_syncs())}
    else:
        kw = dict(dict(MODES)[mode])
        if kw.get("kick_bias") == "heat":
            kw["heat"] = [np.array(g["heat"], dtype=np.float32) for g in inputs["groups"]]
            kw["edge_index"] = [np.stack([np.repeat(np.arange(len(g["row_ptr"]) - 1), np.diff(g["row_ptr"])), g["col"]]).astype(np.int64)
                                for g in inputs["groups"]]
        per = {}
        tours, stats = batched_iterated_search_ragged(pts, starts, cap, kicks=kicks, kick_size=inputs["kick_size"], span=inputs["span"],
                                                      seeds=inputs["seeds"], offsets=inputs["offsets"], stats=per, **common, **kw)
        res = {k: ([float(x).hex() for x in v] if k.endswith("length") else np.asarray(v).tolist()) for k, v in sorted(per.items())}
    res["tours"] = [t.tolist() for t in tours]
    res.update({k: np.asarray(stats[k]).tolist() for k in KEYS})
    return res
