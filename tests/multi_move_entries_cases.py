"""The cases of tests/golden/multi_move_entries.json: what the group-synchronised multi-move 2-opt entries
(``difusco_tsp_multi_two_opt_ragged``, ``difusco_tsp_nbr_two_opt_ragged``) and the neighbour-list 2-opt + Or-opt search
(``difusco_tsp_nbr_local_search_ragged``) reserve, refuse and compute on a handful of tiny calls.
scripts/record_multi_move_entries.py records them, tests/test_gpu_multi_move_entries.py replays them and
tests/test_multi_move_entries_host.py checks the recorded runs against the numpy restatements; all three call the functions
here, so the fixture and the tests cannot drift apart.  Nothing here draws a random number: the inputs of the runs are in the
fixture."""
import ctypes

import numpy as np

from tsp_search_entries_cases import SHAPES

ENTRIES = ("multi_two_opt", "nbr_two_opt", "nbr_local_search")
LISTED = ENTRIES[1:]                          # the entries that take neighbour lists: K and closing
SIZE_KS, CLOSINGS = (1, 8), (0, 1)
OUTPUTS = {"multi_two_opt": ("sweeps", "moves"), "nbr_two_opt": ("sweeps", "full_sweeps", "moves"),
           "nbr_local_search": ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves", "full_sweeps",
                                "full_rounds")}
I32_OUTPUTS = ("rounds", "full_rounds")


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


# ---- workspace bytes

def workspace_bytes(L, entry, group_n, group_tours, K=1, closing=0, null_bytes=False):
    """[return code, bytes] of the entry's ``_workspace_bytes``."""
    n, t, out = _i32(group_n), _i32(group_tours), ctypes.c_size_t(0)
    fn = getattr(L, f"difusco_tsp_{entry}_ragged_workspace_bytes")
    args = (len(n), n.ctypes.data, t.ctypes.data) + ((K, closing) if entry in LISTED else ())
    return [fn(*args, None if null_bytes else ctypes.byref(out)), int(out.value)]


def workspace_sizes(L):
    rows = []
    for group_n, group_tours in SHAPES:
        row = {"group_n": group_n, "group_tours": group_tours, "multi_two_opt": workspace_bytes(L, "multi_two_opt", group_n, group_tours)}
        for entry in LISTED:
            for K in SIZE_KS:
                for closing in CLOSINGS:
                    row[f"{entry}_K{K}_closing{closing}"] = workspace_bytes(L, entry, group_n, group_tours, K, closing)
        rows.append(row)
    return rows


def merged_state_word_bytes(tours):
    """What ``difusco_tsp_nbr_two_opt_ragged_workspace_bytes`` returns less than the recorded library: that one kept a done word
    and a phase word per tour, two sections of ``4 * tours`` bytes rounded up to 256; the merged state word is one of them."""
    return 256 * -(-4 * tours // 256)


def _up256(nbytes):
    return 256 * -(-nbytes // 256)


def tour_descriptor_bytes(tours):
    """What the three entries return MORE than the recorded library (never more than 0) for their section of tour descriptors:
    the recorded descriptor held the offset of the group's lists, 56 bytes; the offset now follows from the group's offset in
    ``points`` and the descriptor is 48 bytes.  Zero for every shape of ``SHAPES``: 1 .. 6 tours fit 256 bytes either way."""
    return _up256(48 * tours) - _up256(56 * tours)


def expected_sizes(recorded_rows):
    """The recorded sizes as a library with the merged state word and the 48-byte descriptor returns them.  The state of
    ``nbr_local_search`` is split into two records of 56 and 16 bytes per tour that share the section the 72-byte record had:
    no change."""
    rows = []
    for rec in recorded_rows:
        row, tours = dict(rec), sum(rec["group_tours"])
        for key in rec:
            if key.startswith("group_"):
                continue
            change = tour_descriptor_bytes(tours)
            if key.startswith("nbr_two_opt_"):
                change -= merged_state_word_bytes(tours)
            row[key] = [rec[key][0], rec[key][1] + change]
        rows.append(row)
    return rows


SIZE_REFUSALS = [("groups_0", dict(group_n=[], group_tours=[])), ("n_3", dict(group_n=[5, 3])), ("tours_0", dict(group_tours=[0, 1])),
                 ("null_bytes", dict(null_bytes=True)), ("K_0", dict(K=0)), ("closing_2", dict(closing=2)),
                 ("nK_too_many", dict(group_n=[5, 1 << 19], K=(1 << 31) - 1)),
                 ("order_null_bytes_groups_0", dict(group_n=[], group_tours=[], null_bytes=True)),
                 ("order_n_3_K_0", dict(group_n=[5, 3], K=0)), ("order_K_0_closing_2", dict(K=0, closing=2))]


def size_refusals(L):
    """The refusals of the three ``_workspace_bytes`` entries; the plain entry takes neither K nor closing."""
    rows = {}
    for entry in ENTRIES:
        rows[entry] = {}
        for name, change in SIZE_REFUSALS:
            if entry not in LISTED and ("K" in change or "closing" in change):
                continue
            a = dict(dict(group_n=[5, 9], group_tours=[2, 1], K=2, closing=1), **change)
            rows[entry][name] = [workspace_bytes(L, entry, **a)[0], L.difusco_last_error().decode()]
    return rows


# ---- refusals: the valid call every refusal departs from in one argument (the `order_` cases in two)

VALID = dict(groups=2, group_n=[5, 9], group_tours=[2, 1], K=2, closing=1, max_iterations=10, max_rounds=2, select_rounds=4,
             null=None, workspace_short=0)
_GROUPS = [("groups_0", dict(groups=0)), ("null_group_n", dict(null="group_n")), ("n_3", dict(group_n=[5, 3])),
           ("tours_0", dict(group_tours=[0, 1]))]
_LISTS = [("K_0", dict(K=0)), ("closing_2", dict(closing=2)), ("null_neighbors", dict(null="neighbors"))]
_DEVICE = [("null_points", dict(null="points")), ("null_tours", dict(null="tours")), ("null_workspace", dict(null="workspace"))]
_CAP = [("max_iterations_-1", dict(max_iterations=-1))]
_SELECT = [("select_rounds_0", dict(select_rounds=0))]
_SHORT = [("workspace_one_byte_short", dict(workspace_short=1))]


def _null_outputs(entry):
    return [(f"null_{k}_out", dict(null=k)) for k in OUTPUTS[entry]]


REFUSALS = {
    "multi_two_opt": _GROUPS + _DEVICE + _null_outputs("multi_two_opt") + _CAP + _SELECT + _SHORT +
                     [("order_max_iterations_select_rounds", dict(max_iterations=-1, select_rounds=0)),
                      ("order_select_rounds_workspace", dict(select_rounds=0, workspace_short=1))],
    "nbr_two_opt": _GROUPS + _LISTS + _DEVICE + _null_outputs("nbr_two_opt") + _CAP + _SELECT + _SHORT +
                   [("order_K_neighbors", dict(K=0, null="neighbors")), ("order_closing_max_iterations", dict(closing=2, max_iterations=-1)),
                    ("order_neighbors_select_rounds", dict(null="neighbors", select_rounds=0)),
                    ("order_select_rounds_workspace", dict(select_rounds=0, workspace_short=1))],
    "nbr_local_search": _GROUPS + _LISTS + _DEVICE + _null_outputs("nbr_local_search") + _CAP + [("max_rounds_0", dict(max_rounds=0))] +
                        _SELECT + _SHORT +
                        [("order_K_neighbors", dict(K=0, null="neighbors")), ("order_closing_max_iterations", dict(closing=2, max_iterations=-1)),
                         ("order_neighbors_max_rounds", dict(null="neighbors", max_rounds=0)),
                         ("order_max_rounds_select_rounds", dict(max_rounds=0, select_rounds=0)),
                         ("order_select_rounds_workspace", dict(select_rounds=0, workspace_short=1))],
}


def refused_call(L, entry, **change):
    """The entry on VALID with ``change``; every array is a host array of VALID's size, which a refused call never reads.
    Returns [return code, the text of ``difusco_last_error``]."""
    a = dict(VALID, **change)
    rc, need = workspace_bytes(L, entry, VALID["group_n"], VALID["group_tours"], VALID["K"], VALID["closing"])
    assert rc == 0
    arrays = {"group_n": _i32(a["group_n"]), "group_tours": _i32(a["group_tours"]), "points": np.zeros(64),
              "tours": np.zeros(64, dtype=np.int32), "neighbors": np.zeros(64, dtype=np.int32), "workspace": np.zeros(need, dtype=np.uint8)}
    arrays.update({k: np.zeros(4, dtype=np.int32 if k in I32_OUTPUTS else np.int64) for k in OUTPUTS[entry]})
    ptr = lambda name: None if a["null"] == name else arrays[name].ctypes.data
    head = (a["groups"], ptr("group_n"), ptr("group_tours"), ptr("points"), ptr("tours"))
    lists = (ptr("neighbors"), a["K"], a["closing"]) if entry in LISTED else ()
    caps = (a["max_iterations"],) + ((a["max_rounds"],) if entry == "nbr_local_search" else ()) + (a["select_rounds"],)
    tail = (ptr("workspace"), need - a["workspace_short"]) + tuple(ptr(k) for k in OUTPUTS[entry])
    rc = getattr(L, f"difusco_tsp_{entry}_ragged")(*head, *lists, *caps, *tail, None)
    text = L.difusco_last_error().decode()
    if entry == "nbr_two_opt":      # its figure differs from the recorded library's by merged_state_word_bytes: workspace_sizes pins it
        text = text.replace(str(need - 1), "<bytes - 1>").replace(str(need), "<bytes>")
    return [int(rc), text]


def refusals(L):
    return {entry: {name: refused_call(L, entry, **change) for name, change in REFUSALS[entry]} for entry in ENTRIES}


# ---- the short runs: three groups (n = 4, 7, 33) in one call; the middle one is a convex polygon in order, a local optimum of
# both move kinds.  The lists of the fixture hold RUN_KS[-1] columns; a run with fewer takes the first ones.

RUN_KS = (1, 3)
CAPS = (0, 1, 2, 1000)                        # 2 with closing: the cap falls between the two phases
ROUNDS = (1, 16)
RUNS = [("multi_two_opt", None, None, cap, None, 4) for cap in CAPS] + [("multi_two_opt", None, None, 1000, None, 1)] + \
       [("nbr_two_opt", K, closing, cap, None, 4) for K in RUN_KS for closing in CLOSINGS for cap in CAPS] + \
       [("nbr_two_opt", 3, 1, 1000, None, 1)] + \
       [("nbr_local_search", K, closing, cap, rounds, 4) for K in RUN_KS for closing in CLOSINGS for cap in CAPS for rounds in ROUNDS] + \
       [("nbr_local_search", 3, 1, 1000, 16, 1)]


def run_name(entry, K, closing, cap, rounds, select_rounds):
    lists = "" if K is None else f"_K{K}_closing{closing}"
    return f"{entry}{lists}_cap{cap}" + ("" if rounds is None else f"_rounds{rounds}") + f"_select{select_rounds}"


def group_arrays(inputs, K=None):
    """(points float64 [n, 2], tours int64 [P, n + 1], lists int32 [n, K] or None) of every group; the points are stored as
    integers on a 2^-16 grid."""
    return [(np.array(g["points_q16"], dtype=np.float64) / 65536.0, np.array(g["tours"], dtype=np.int64),
             None if K is None else np.ascontiguousarray(np.array(g["neighbors"], dtype=np.int32)[:, :K])) for g in inputs["groups"]]


def short_run(dev, inputs, entry, K, closing, cap, rounds, select_rounds):
    """One call on the fixture's inputs: the tours and every counter array as plain lists."""
    from difusco_amd import decode
    groups = group_arrays(inputs, K)
    pts, starts = [g[0] for g in groups], [g[1] for g in groups]
    lists = {} if K is None else dict(neighbors=[g[2] for g in groups], closing=bool(closing))
    if entry == "nbr_local_search":
        tours, stats = decode.batched_nbr_local_search_ragged(pts, starts, cap, device=dev, max_rounds=rounds, select_rounds=select_rounds,
                                                              **lists)
    else:
        fn = decode.batched_multi_two_opt_ragged if entry == "multi_two_opt" else decode.batched_nbr_two_opt_ragged
        stats = {}
        tours, stats["sweeps"] = fn(pts, starts, cap, device=dev, select_rounds=select_rounds, stats=stats, **lists)
    return dict({"tours": [t.tolist() for t in tours]}, **{k: np.asarray(stats[k]).tolist() for k in OUTPUTS[entry]})


def emulated_run(inputs, entry, K, closing, cap, rounds, select_rounds):
    """What ``short_run`` returns, from the numpy restatements of the three rules, group by group."""
    import multi_two_opt_emulation as M2
    import nbr_local_search_emulation as NL
    import nbr_two_opt_emulation as N2
    res = {"tours": []}
    res.update({k: [] for k in OUTPUTS[entry]})
    for pts, starts, lists in group_arrays(inputs, K):
        if entry == "multi_two_opt":
            tours, *counters = M2.multi_two_opt(pts, starts, cap, select_rounds)
            counters = dict(zip(OUTPUTS[entry], counters))
        elif entry == "nbr_two_opt":
            tours, *counters = N2.nbr_two_opt(pts, starts, lists, bool(closing), cap, select_rounds)
            counters = dict(zip(OUTPUTS[entry], counters))
        else:
            tours, counters = NL.nbr_local_search(pts, starts, lists, bool(closing), cap, rounds, select_rounds)
        res["tours"].append(np.asarray(tours).tolist())
        for k in OUTPUTS[entry]:
            res[k].append(int(counters[k]))
    return res
