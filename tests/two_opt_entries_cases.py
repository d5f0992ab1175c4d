"""The cases of tests/golden/two_opt_entries.json: what the six single-move 2-opt entries (``difusco_tsp_two_opt``, ``_grouped``,
``_screened``, ``_grouped_screened`` and ``_ragged`` with method 0 and 1) reserve, refuse and compute on a handful of tiny calls.
scripts/record_two_opt_entries.py records them, tests/test_gpu_two_opt_entries.py replays them and tests/test_two_opt_entries_host.py
checks the recorded runs against the oracle; all three call the functions here, so the fixture and the tests cannot drift apart.
Nothing here draws a random number: the inputs of the runs are in the fixture."""
import ctypes
import hashlib

import numpy as np

from tsp_search_entries_cases import SHAPES

UNIFORM = ("two_opt", "two_opt_screened", "two_opt_grouped", "two_opt_grouped_screened")
I64P = ctypes.POINTER(ctypes.c_int64)


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


# ---- workspace bytes: n around the 16-row tile and the 1024-column chunk, one tour, one group, three groups

WS_N = (4, 16, 17, 1024, 1025)
WS_GROUPS = ((1, 1), (1, 3), (3, 2))


def uniform_workspace_bytes(L, entry, n, *counts):
    """[return code, bytes] of a uniform entry's ``_workspace_bytes``: counts = (batch,) or (groups, per_group)."""
    out = ctypes.c_size_t(0)
    return [getattr(L, f"difusco_tsp_{entry}_workspace_bytes")(n, *counts, ctypes.byref(out)), int(out.value)]


def ragged_workspace_bytes(L, group_n, group_tours, method, entry="two_opt"):
    n, t, out = _i32(group_n), _i32(group_tours), ctypes.c_size_t(0)
    fn = getattr(L, f"difusco_tsp_{entry}_ragged_workspace_bytes")
    args = (len(n), n.ctypes.data, t.ctypes.data) + ((method,) if entry == "two_opt" else ())
    return [fn(*args, ctypes.byref(out)), int(out.value)]


def workspace_sizes(L):
    """Five of the six figures; the plain entry's is the grouped (n, 1, batch) one and is compared with that, not recorded."""
    uniform = []
    for n in WS_N:
        for G, P in WS_GROUPS:
            uniform.append({"n": n, "groups": G, "per_group": P,
                            "two_opt_screened": uniform_workspace_bytes(L, "two_opt_screened", n, G * P),
                            "two_opt_grouped": uniform_workspace_bytes(L, "two_opt_grouped", n, G, P),
                            "two_opt_grouped_screened": uniform_workspace_bytes(L, "two_opt_grouped_screened", n, G, P)})
    ragged = [{"group_n": group_n, "group_tours": group_tours, "method_0": ragged_workspace_bytes(L, group_n, group_tours, 0),
               "method_1": ragged_workspace_bytes(L, group_n, group_tours, 1)} for group_n, group_tours in SHAPES]
    return {"uniform": uniform, "ragged": ragged}


# ---- refusals: one bad argument against one valid tiny call

VALID = dict(n=5, batch=2, groups=2, per_group=2, group_n=[5, 9], group_tours=[2, 1], method=0, max_iterations=10, null=None,
             workspace_short=0)
_ARRAYS = [("null_points", dict(null="points")), ("null_tours", dict(null="tours")), ("null_workspace", dict(null="workspace")),
           ("max_iterations_-1", dict(max_iterations=-1))]
_SHORT = [("workspace_one_byte_short", dict(workspace_short=1))]
_NULL_ITS = [("null_iterations_out", dict(null="iterations_out"))]
REFUSALS = {
    "two_opt": [("n_3", dict(n=3)), ("batch_0", dict(batch=0))] + _ARRAYS + _SHORT,
    "two_opt_screened": [("n_3", dict(n=3)), ("batch_0", dict(batch=0))] + _ARRAYS + _SHORT + [("batch_65536", dict(batch=65536))],
    "two_opt_grouped": [("n_3", dict(n=3)), ("groups_0", dict(groups=0)), ("per_group_0", dict(per_group=0))] + _ARRAYS + _NULL_ITS +
                       _SHORT,
    "two_opt_grouped_screened": [("n_3", dict(n=3)), ("groups_0", dict(groups=0)), ("per_group_0", dict(per_group=0))] + _ARRAYS +
                                _NULL_ITS + _SHORT + [("batch_65536", dict(per_group=32768))],
    "two_opt_ragged": [("groups_0", dict(groups=0)), ("null_group_n", dict(null="group_n")), ("n_3", dict(group_n=[5, 3])),
                       ("n_65535x16+1", dict(group_n=[5, 65535 * 16 + 1])), ("tours_0", dict(group_tours=[0, 1])),
                       ("tours_65536", dict(group_tours=[65535, 1])), ("method_2", dict(method=2))] + _NULL_ITS + _SHORT,
    # the group-array check these two share with the entries above
    "local_search_ragged": [("groups_0", dict(groups=0)), ("n_3", dict(group_n=[5, 3])), ("tours_0", dict(group_tours=[0, 1]))],
    "multi_two_opt_ragged": [("groups_0", dict(groups=0)), ("n_3", dict(group_n=[5, 3])), ("tours_0", dict(group_tours=[0, 1]))],
}


def refused_call(L, entry, **change):
    """The entry on VALID with ``change``; every array is a host array of VALID's size, which a refused call never reads.
    Returns [return code, the text of ``difusco_last_error``]."""
    a = dict(VALID, **change)
    ragged = entry.endswith("_ragged")
    if ragged:
        rc, need = ragged_workspace_bytes(L, VALID["group_n"], VALID["group_tours"], VALID["method"], entry[:-len("_ragged")])
    else:
        valid_counts = (VALID["groups"], VALID["per_group"]) if "grouped" in entry else (VALID["batch"],)
        rc, need = uniform_workspace_bytes(L, entry, VALID["n"], *valid_counts)
    assert rc == 0
    group_n, group_tours = _i32(a["group_n"]), _i32(a["group_tours"])
    arrays = {"points": np.zeros(64), "tours": np.zeros(64, dtype=np.int32), "workspace": np.zeros(need, dtype=np.uint8),
              "iterations_out": np.zeros(4, dtype=np.int64), "group_n": group_n, "group_tours": group_tours}
    ptr = lambda name: None if a["null"] == name else arrays[name].ctypes.data_as(I64P if name == "iterations_out" else ctypes.c_void_p)
    pairs, spare, rounds = ctypes.c_int64(), np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int32)
    body = (ptr("points"), ptr("tours"), a["max_iterations"])
    ws = (ptr("workspace"), need - a["workspace_short"])
    fn = getattr(L, f"difusco_tsp_{entry}")
    if entry == "two_opt_ragged":
        rc = fn(a["groups"], ptr("group_n"), ptr("group_tours"), *body, a["method"], *ws, ptr("iterations_out"), ctypes.byref(pairs), None)
    elif entry == "local_search_ragged":
        rc = fn(a["groups"], ptr("group_n"), ptr("group_tours"), *body, 2, *ws, ptr("iterations_out"), spare.ctypes.data,
                rounds.ctypes.data, None)
    elif entry == "multi_two_opt_ragged":
        rc = fn(a["groups"], ptr("group_n"), ptr("group_tours"), *body, 4, *ws, ptr("iterations_out"), spare.ctypes.data, None)
    else:
        counts = (a["groups"], a["per_group"]) if "grouped" in entry else (a["batch"],)
        tail = (ctypes.byref(pairs),) if "screened" in entry else ()
        rc = fn(a["n"], *counts, *body, *ws, ptr("iterations_out"), *tail, None)
    text = L.difusco_last_error().decode()
    if entry == "two_opt":      # its figure is compared with the grouped entry's and not recorded: named in the message as well
        text = text.replace(str(need - 1), "<bytes - 1>").replace(str(need), "<bytes>")
    return [int(rc), text]


def refusals(L):
    return {entry: {name: refused_call(L, entry, **change) for name, change in cases} for entry, cases in REFUSALS.items()}


def size_refusals(L):
    """The group-array refusals of the three ``_ragged_workspace_bytes`` that share the check."""
    cases = [("groups_0", [], []), ("n_3", [5, 3], [2, 1]), ("tours_0", [5, 9], [0, 1])]
    return {entry: {name: [ragged_workspace_bytes(L, gn, gt, 0, entry)[0], L.difusco_last_error().decode()] for name, gn, gt in cases}
            for entry in ("two_opt", "local_search", "multi_two_opt")}


# ---- the short runs: three groups of two tours at each of three sizes; group 1 of every size is a convex polygon visited in
# order, a local optimum, so it stops at the first apply while the others go on

SIZES = (4, 17, 1025)
GROUPS, PER_GROUP = 3, 2
CAPS = (0, 3, 1000)
BIG_CAP = 25                                 # what the cap 1000 becomes in a call with n = 1025 (the oracle's cost on the CPU)
ENTRIES = ("plain", "screened", "grouped", "grouped_screened", "ragged_exact", "ragged_screened")
SCALED = "17_scaled"                         # group 0 of n = 17 times 2^70: M = 2^70 has no screen bound, the exact fallback runs
RUNS = [(entry, n, cap) for entry in ENTRIES for n in SIZES for cap in CAPS] + \
       [(entry, "mixed", cap) for entry in ENTRIES[4:] for cap in CAPS] + [("grouped_screened", SCALED, 1000)]


def run_name(entry, shape, cap):
    return f"{entry}_{'n' if isinstance(shape, int) else ''}{shape}_cap{cap}"


def groups_of(shape):
    """(n, group, scale) of every group of a run, in call order."""
    if shape == "mixed":                     # all nine groups, the sizes interleaved
        return [(n, g, 1.0) for g in range(GROUPS) for n in SIZES]
    if shape == SCALED:
        return [(17, 0, 2.0 ** 70), (17, 1, 1.0), (17, 2, 1.0)]
    return [(shape, g, 1.0) for g in range(GROUPS)]


def cap_of(shape, cap):
    return BIG_CAP if cap == 1000 and shape in (1025, "mixed") else cap


def group_arrays(inputs, n, g, scale=1.0):
    """(points float64 [n, 2], tours int64 [PER_GROUP, n + 1]) of one group; the points are stored as integers on a 2^-16 grid."""
    grp = inputs["groups"][str(n)][g]
    return np.array(grp["points_q16"], dtype=np.float64) / 65536.0 * scale, np.array(grp["tours"], dtype=np.int64)


def encode_tours(tours):
    """Tours as lists; above 64 nodes as the SHA-256 of their int32 bytes."""
    tours = np.asarray(tours)
    if tours.shape[1] - 1 <= 64:
        return tours.tolist()
    return [hashlib.sha256(np.ascontiguousarray(t, dtype=np.int32).tobytes()).hexdigest() for t in tours]


def evaluations(iterations, cap):
    """Sweeps of the exact loop that did work: one more than the moves unless the cap ended the run."""
    return iterations + 1 if iterations < max(cap, 1) else iterations


def exact_pairs_of_exact_run(shape, cap, iterations):
    """``exact_pairs`` of a run that evaluates every pair in float64."""
    return sum(evaluations(int(it), cap_of(shape, cap)) * PER_GROUP * ((n - 1) * (n - 2) // 2)
               for (n, _, _), it in zip(groups_of(shape), iterations))


def short_run(dev, inputs, entry, shape, cap, one_group=False):
    """One run on the fixture's inputs: {"tours": per group, "iterations": per group, "exact_pairs": per call that reports it}.
    The plain and screened entries take one group per call.  ``one_group``: the grouped entry called as (n, 1, batch) per group."""
    from difusco_amd.decode import batched_two_opt_grouped, batched_two_opt_ragged, batched_two_opt_torch
    groups = [group_arrays(inputs, *k) for k in groups_of(shape)]
    kw = dict(max_iterations=cap_of(shape, cap), device=dev, method="screened" if entry.endswith("screened") else "exact")
    calls = []
    if entry in ("plain", "screened"):
        for pts, trs in groups:
            stats = {}
            tours, it = batched_two_opt_torch(pts, trs, stats=stats, **kw)
            calls.append(([tours], [it], stats))
    elif one_group:
        for pts, trs in groups:
            stats = {}
            tours, its = batched_two_opt_grouped(pts[None], trs, stats=stats, **kw)
            calls.append(([tours], its.tolist(), stats))
    elif entry.startswith("grouped"):
        stats = {}
        tours, its = batched_two_opt_grouped(np.stack([p for p, _ in groups]), np.concatenate([t for _, t in groups]), stats=stats, **kw)
        calls.append((np.split(tours, len(groups)), its.tolist(), stats))
    else:
        stats = {}
        tours, its = batched_two_opt_ragged([p for p, _ in groups], [t for _, t in groups], stats=stats, **kw)
        calls.append((tours, its.tolist(), stats))
    return {"tours": [encode_tours(t) for tours, _, _ in calls for t in tours],
            "iterations": [int(it) for _, its, _ in calls for it in its],
            "exact_pairs": [int(stats["exact_pairs"]) for _, _, stats in calls if "exact_pairs" in stats]}
