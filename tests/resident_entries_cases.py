"""The cases of tests/golden/resident_entries.json: what the two resident tour searches (``difusco_tsp_two_opt_resident``,
``difusco_tsp_local_search_resident``: one GPU block per group) and their ``_workspace_bytes`` / ``_max_cells`` reserve, refuse
and compute on a handful of tiny calls.  scripts/record_resident_entries.py records them, tests/test_gpu_resident_entries.py
replays them and tests/test_resident_entries_host.py checks the recorded runs against the numpy restatements; all three call the
functions here, so the fixture and the tests cannot drift apart.  Nothing here draws a random number: the inputs of the runs are
in the fixture."""
import ctypes

import numpy as np

ENTRIES = ("two_opt", "local_search")
METHODS = ("exact", "screened")               # of the 2-opt entry: its codes 0 and 1
OUTPUTS = {"two_opt": ("iterations",), "local_search": ("two_opt_iterations", "or_opt_iterations", "rounds")}
I32_OUTPUTS = ("rounds",)
DEFAULT_PER_LAUNCH = 1024                     # what per-launch = 0 stands for in both entries

# (n, tours) of the groups of the fixture, by name.  A block has 256 .. 1024 threads in whole waves, a quarter of the largest
# group's 2-opt pairs, and its waves form block waves / tours teams of whole waves:
#   n4x20  256 threads, 4 teams of one wave for 20 tours: five rounds per sweep
#   n43x5  1024 threads, 16 waves, 3 per team, 5 teams: wave 15 is left over and only keeps the barriers
#   n65    a second block of 64 Or-opt columns
#   poly7  a convex polygon visited in order: it stops at once
#   tiny33 the points of another n = 33 group times 2^-40: every |coordinate| is below the least M with a screen bound
GROUPS = {"n4x1": (4, 1), "n4x2": (4, 2), "n5": (5, 2), "poly7": (7, 1), "n33x3": (33, 3), "n65": (65, 1), "n4x20": (4, 20),
          "n43x5": (43, 5), "tiny33": (33, 2)}
TINY_LOG2 = -40
# the calls: every group alone, one call whose S (cells) and T (tours) come from different groups, and the group without a
# screen bound beside a bounded one
CALLS = [(name,) for name in GROUPS if name != "tiny33"] + [("n4x20", "poly7", "n33x3"), ("n33x3", "tiny33")]
SHAPES = [([GROUPS[g][0] for g in call], [GROUPS[g][1] for g in call]) for call in CALLS]
# the sizes depend on the number of groups alone: two calls of many groups beside the shapes of the runs
SIZE_SHAPES = SHAPES + [([5] * 11, [2] * 11), ([8] * 600, [1] * 600)]


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


# ---- workspace bytes and the limit

def workspace_bytes(L, entry, group_n, group_tours, method=0, null_bytes=False):
    """[return code, bytes] of the entry's ``_workspace_bytes``; only the 2-opt one takes a method."""
    n, t, out = _i32(group_n), _i32(group_tours), ctypes.c_size_t(0)
    fn = getattr(L, f"difusco_tsp_{entry}_resident_workspace_bytes")
    args = (len(n), n.ctypes.data, t.ctypes.data) + ((method,) if entry == "two_opt" else ())
    return [fn(*args, None if null_bytes else ctypes.byref(out)), int(out.value)]


def max_cells(L):
    return {entry: int(getattr(L, f"difusco_tsp_{entry}_resident_max_cells")()) for entry in ENTRIES}


def workspace_sizes(L):
    return [{"group_n": n, "group_tours": t, "two_opt_method0": workspace_bytes(L, "two_opt", n, t, 0),
             "two_opt_method1": workspace_bytes(L, "two_opt", n, t, 1), "local_search": workspace_bytes(L, "local_search", n, t)}
            for n, t in SIZE_SHAPES]


SIZE_REFUSALS = [("groups_0", dict(group_n=[], group_tours=[])), ("n_3", dict(group_n=[5, 3])), ("tours_0", dict(group_tours=[0, 1])),
                 ("tours_too_many", dict(group_tours=[65535, 1])), ("null_bytes", dict(null_bytes=True)), ("method_2", dict(method=2)),
                 ("order_null_bytes_groups_0", dict(group_n=[], group_tours=[], null_bytes=True)),
                 ("order_n_3_method_2", dict(group_n=[5, 3], method=2))]


def size_refusals(L):
    rows = {}
    for entry in ENTRIES:
        rows[entry] = {}
        for name, change in SIZE_REFUSALS:
            if entry != "two_opt" and "method" in change:
                continue
            a = dict(dict(group_n=[5, 9], group_tours=[2, 1]), **change)
            rows[entry][name] = [workspace_bytes(L, entry, **a)[0], L.difusco_last_error().decode()]
    return rows


# ---- refusals: the valid call every refusal departs from in one argument (the `order_` cases in two).  `over` puts one cell
# more than the limit into group 1: as one tour of max_cells cities, and as tours of 501 entries.

VALID = dict(groups=2, group_n=[5, 9], group_tours=[2, 1], method=0, max_iterations=10, max_rounds=2, per_launch=0, null=None,
             workspace_short=0, over=None)
_GROUPS = [("groups_0", dict(groups=0)), ("null_group_n", dict(null="group_n")), ("null_group_tours", dict(null="group_tours")),
           ("n_3", dict(group_n=[5, 3])), ("tours_0", dict(group_tours=[0, 1]))]
_DEVICE = [("null_points", dict(null="points")), ("null_tours", dict(null="tours")), ("null_workspace", dict(null="workspace"))]
_TAIL = [("max_iterations_-1", dict(max_iterations=-1)), ("per_launch_-1", dict(per_launch=-1)),
         ("workspace_one_byte_short", dict(workspace_short=1)), ("max_cells_one_tour", dict(over="one_tour")),
         ("max_cells_tours_of_501", dict(over="tours_of_501")), ("order_n_3_max_cells", dict(group_n=[3, 9], over="one_tour")),
         ("order_null_points_per_launch", dict(null="points", per_launch=-1)),
         ("order_per_launch_workspace", dict(per_launch=-1, workspace_short=1)),
         ("order_workspace_max_cells", dict(workspace_short=1, over="one_tour"))]


def _null_outputs(entry):
    return [(f"null_{k}_out", dict(null=k)) for k in OUTPUTS[entry]]


REFUSALS = {
    "two_opt": _GROUPS + [("method_2", dict(method=2)), ("method_-1", dict(method=-1))] + _DEVICE + _null_outputs("two_opt") + _TAIL +
               [("order_tours_0_method", dict(group_tours=[0, 1], method=2)), ("order_method_null_points", dict(method=2, null="points")),
                ("order_method_max_cells", dict(method=2, over="one_tour"))],
    "local_search": _GROUPS + _DEVICE + _null_outputs("local_search") + [("max_rounds_0", dict(max_rounds=0))] + _TAIL +
                    [("order_max_iterations_max_rounds", dict(max_iterations=-1, max_rounds=0)),
                     ("order_max_rounds_per_launch", dict(max_rounds=0, per_launch=-1)),
                     ("order_max_rounds_max_cells", dict(max_rounds=0, over="one_tour"))],
}


def refused_call(L, entry, **change):
    """The entry on VALID with ``change``; every array is a host array of VALID's size, which a refused call never reads.
    Returns [return code, the text of ``difusco_last_error``, whether the tours array is unchanged]."""
    a = dict(VALID, **change)
    rc, need = workspace_bytes(L, entry, VALID["group_n"], VALID["group_tours"])
    assert rc == 0
    group_n, group_tours = list(a["group_n"]), list(a["group_tours"])
    m = max_cells(L)[entry]
    if a["over"] == "one_tour":
        group_n[1], group_tours[1] = m, 1                      # m + 1 cells
    elif a["over"] == "tours_of_501":
        group_n[1], group_tours[1] = 500, m // 501 + 1
    arrays = {"group_n": _i32(group_n), "group_tours": _i32(group_tours), "points": np.zeros(64),
              "tours": np.arange(64, dtype=np.int32), "workspace": np.zeros(need, dtype=np.uint8)}
    arrays.update({k: np.zeros(4, dtype=np.int32 if k in I32_OUTPUTS else np.int64) for k in OUTPUTS[entry]})
    before = arrays["tours"].tobytes()
    ptr = lambda name: None if a["null"] == name else arrays[name].ctypes.data_as(ctypes.c_void_p)
    head = (a["groups"], ptr("group_n"), ptr("group_tours"), ptr("points"), ptr("tours"), a["max_iterations"])
    caps = (a["method"],) if entry == "two_opt" else (a["max_rounds"],)
    outs = tuple(ptr(k) for k in OUTPUTS[entry]) + ((ctypes.byref(ctypes.c_int64()),) if entry == "two_opt" else ())
    rc = getattr(L, f"difusco_tsp_{entry}_resident")(*head, *caps, a["per_launch"], ptr("workspace"), need - a["workspace_short"],
                                                      *outs, ctypes.byref(ctypes.c_int32()), None)
    return [int(rc), L.difusco_last_error().decode(), arrays["tours"].tobytes() == before]


def refusals(L):
    return {entry: {name: refused_call(L, entry, **change) for name, change in REFUSALS[entry]} for entry in ENTRIES}


# ---- the short runs

CAPS = (0, 1, 3, 1000)
PER_LAUNCH = (0, 1, 2)
ROUNDS = (1, 16)
# (entry, call, max_iterations, per-launch, method of the 2-opt entry or max_rounds of the local search)
RUNS = [("two_opt", c, cap, per, m) for c in range(len(CALLS)) for cap in CAPS for per in PER_LAUNCH for m in METHODS] + \
       [("local_search", c, cap, per, r) for c in range(len(CALLS) - 1) for cap in CAPS for per in PER_LAUNCH for r in ROUNDS]


def run_name(entry, call, cap, per_launch, variant):
    return f"{entry}_{'+'.join(CALLS[call])}_cap{cap}_per{per_launch}_" + (variant if entry == "two_opt" else f"rounds{variant}")


def group_arrays(inputs, call):
    """[(points float64 [n, 2], tours int64 [P, n + 1])] of a call's groups; the points are stored as integers on a 2^-16 grid,
    with a power of two to scale them by where there is one."""
    return [(np.array(inputs[g]["points_q16"], dtype=np.float64) / 65536.0 * 2.0 ** inputs[g].get("scale_log2", 0),
             np.array(inputs[g]["tours"], dtype=np.int64)) for g in CALLS[call]]


def short_run(dev, inputs, entry, call, cap, per_launch, variant):
    """One call on the fixture's inputs: the tours and every counter as plain lists."""
    from difusco_amd import decode
    groups = group_arrays(inputs, call)
    pts, starts, stats = [p for p, _ in groups], [t for _, t in groups], {}
    if entry == "two_opt":
        tours, its = decode.batched_two_opt_ragged(pts, starts, max_iterations=cap, device=dev, method=variant, mode="resident",
                                                   moves_per_launch=per_launch, stats=stats)
        res = {"iterations": np.asarray(its).tolist(), "exact_pairs": int(stats["exact_pairs"])}
    else:
        tours, two = decode.batched_local_search_ragged(pts, starts, max_iterations=cap, device=dev, max_rounds=variant, mode="resident",
                                                        steps_per_launch=per_launch, stats=stats)
        res = {"two_opt_iterations": np.asarray(two).tolist(), "or_opt_iterations": np.asarray(stats["or_opt_iterations"]).tolist(),
               "rounds": np.asarray(stats["rounds"]).tolist()}
    return dict(res, tours=[np.asarray(t).tolist() for t in tours], host_syncs=int(stats["host_syncs"]))


def pack_runs(runs):
    """The fixture's form of the runs: most runs of a call end with the same tours (the per-launch settings and the two methods
    do not change them), so the fixture holds every distinct list of tours once and a run holds its index.
    Returns (tours, runs)."""
    tours, index, packed = [], {}, {}
    for name, run in runs.items():
        key = repr(run["tours"])
        if key not in index:
            index[key] = len(tours)
            tours.append(run["tours"])
        packed[name] = dict(run, tours=index[key])
    return tours, packed


def recorded_run(recorded, name):
    """A run of the fixture as ``short_run`` returns it."""
    run = recorded["runs"][name]
    return dict(run, tours=recorded["tours"][run["tours"]])


def emulated_run(inputs, entry, call, cap, rounds=None):
    """The tours and the iteration / round counters of ``short_run`` from the numpy restatements of the two rules, group by
    group: ``oracle.tsp_decode_oracle.batched_two_opt`` and ``or_opt_emulation.local_search``."""
    import or_opt_emulation as E
    from oracle import tsp_decode_oracle as D
    res = {"tours": []}
    res.update({k: [] for k in OUTPUTS[entry]})
    for pts, starts in group_arrays(inputs, call):
        if entry == "two_opt":
            tours, *counters = D.batched_two_opt(pts, starts, max_iterations=cap)
        else:
            tours, *counters = E.local_search(pts, starts, max_iterations=cap, max_rounds=rounds)
        res["tours"].append(np.asarray(tours).tolist())
        for k, v in zip(OUTPUTS[entry], counters):
            res[k].append(int(v))
    return res
