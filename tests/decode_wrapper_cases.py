"""The cases of tests/golden/decode_wrappers.json and decode_wrapper_refusals.json: what the Python wrappers of ``difusco_amd.decode``
(every ``batched_*`` family as ``_torch``, ``_grouped`` and ``_ragged``, the three MIS functions) and the local-search part of
``difusco_amd.pipeline`` return, record and refuse on a handful of tiny calls.  scripts/record_decode_wrappers.py records them,
tests/test_decode_wrappers_host.py and tests/test_gpu_decode_wrappers.py replay them; all three call the functions here, so the
fixtures and the tests cannot drift apart.  Nothing here draws a random number: every input is in the fixture.

The emulation suites pin the search rules and the batch == solo suites pin one wrapper against another; this pins what they
leave open for a change of the host side - dtypes, key sets, group order, the offsets a flat result is cut at, the text of every
refusal."""
import numpy as np
import torch

FORMS = ("torch4", "torch17", "grouped", "ragged")
RAGGED = ("a4", "b40", "c17")                 # group_n = [4, 40, 17] with group_tours = [3, 1, 2]: unsorted, all different
RAGGED_TOURS = (3, 1, 2)
KICKS = dict(kicks=2, kick_size=2, span=8)
HEAT_GRID, CAP = 256, 50


# ---- recording: every value with its type


def encode(x):
    """A returned value as JSON that keeps what a caller can tell apart: arrays with dtype and shape, scalars with the name of
    their Python (or numpy) type, the keys of every dict."""
    if isinstance(x, np.ndarray):
        return {"array": x.tolist(), "dtype": str(x.dtype), "shape": list(x.shape)}
    if isinstance(x, dict):
        return {"dict": {k: encode(v) for k, v in x.items()}}
    if isinstance(x, (list, tuple)):
        kinds = {type(v) for v in x}
        if len(kinds) == 1 and kinds <= {int, float, str, bool}:
            return {type(x).__name__: list(x), "of": kinds.pop().__name__}
        return {type(x).__name__: [encode(v) for v in x]}
    if isinstance(x, np.generic):
        return {type(x).__name__: x.item()}
    assert x is None or isinstance(x, (int, float, str, bool)), type(x)
    return {type(x).__name__: x}


# ---- the TSP wrappers


def _group(inputs, name, P):
    g = inputs["tsp"][name]
    return np.array(g["points"], dtype=np.float64), np.array(g["tours"][:P], dtype=np.int64)


def form_groups(form):
    """(suffix of the wrapper, [(group name, tours)]) of a form's case."""
    return {"torch4": ("torch", [("a4", 1)]), "torch17": ("torch", [("c17", 3)]), "grouped": ("grouped", [("c17", 2), ("d17", 2)]),
            "ragged": ("ragged", list(zip(RAGGED, RAGGED_TOURS)))}[form]


def form_args(inputs, form):
    """(suffix, points, tours) as the form's wrappers take them."""
    suffix, groups = form_groups(form)
    pts, trs = zip(*(_group(inputs, name, P) for name, P in groups))
    if suffix == "torch":
        return suffix, pts[0], trs[0]
    if suffix == "grouped":
        return suffix, np.stack(pts), np.concatenate(trs, axis=0)
    return suffix, list(pts), list(trs)


def heat_args(inputs, form, kind, dev):
    """``heat`` / ``edge_index`` of a guided call.  ``sparse``: numpy, the edge list NOT sorted by row; ``dense``: device tensors;
    ``pad``: sparse, and the first group has no edge at all."""
    suffix, groups = form_groups(form)
    heat, ei = [], []
    for i, (name, P) in enumerate(groups):
        g = inputs["tsp"][name]
        if kind == "dense":
            heat.append(torch.tensor(g["dense_heat"][:P], dtype=torch.float32, device=dev) / HEAT_GRID)
        elif kind == "pad" and i == 0:
            heat.append(np.zeros((P, 0), dtype=np.float32))
            ei.append(np.zeros((2, 0), dtype=np.int64))
        else:
            heat.append(np.array(g["sparse_heat"][:P], dtype=np.float32) / HEAT_GRID)
            ei.append(np.array(g["edge_index"], dtype=np.int64))
    if kind == "dense":
        return dict(heat=heat[0] if suffix == "torch" else heat, edge_index=None)
    return dict(heat=heat[0] if suffix == "torch" else heat, edge_index=ei[0] if suffix == "torch" else ei)


def philox(inputs, form):
    T = sum(P for _, P in form_groups(form)[1])
    return dict(seeds=inputs["seeds"][:T], offsets=inputs["offsets"][:T])


# family -> (stem of the wrapper, takes stats=, the keyword arguments given (inputs, form, dev))
FAMILIES = {
    "two_opt_exact": ("two_opt", True, lambda i, f, d: dict(method="exact")),
    "two_opt_screened": ("two_opt", True, lambda i, f, d: dict(method="screened")),
    "local_search": ("local_search", True, lambda i, f, d: {}),
    "multi_two_opt": ("multi_two_opt", True, lambda i, f, d: {}),
    "multi_local_search": ("multi_local_search", False, lambda i, f, d: {}),
    "iterated_full": ("iterated_search", True, lambda i, f, d: dict(KICKS, descent="full", **philox(i, f))),
    "iterated_focused": ("iterated_search", True, lambda i, f, d: dict(KICKS, descent="focused", **philox(i, f))),
    "iterated_heat_sparse": ("iterated_search", True,
                             lambda i, f, d: dict(KICKS, kick_bias="heat", **philox(i, f), **heat_args(i, f, "sparse", d))),
    "iterated_heat_dense": ("iterated_search", True,
                            lambda i, f, d: dict(KICKS, kick_bias="heat", **philox(i, f), **heat_args(i, f, "dense", d))),
    "iterated_heat_pad": ("iterated_search", True,
                          lambda i, f, d: dict(KICKS, kick_bias="heat", **philox(i, f), **heat_args(i, f, "pad", d))),
    "window": ("window_search", True, lambda i, f, d: dict(window=16, passes=2, kicks=1, kick_size=2, span=8, **philox(i, f))),
}
TSP_RUNS = [(family, form) for family in FAMILIES for form in FORMS]


def tsp_run(dev, inputs, family, form):
    """One wrapper call; what it returned and what it left in ``stats``, encoded."""
    from difusco_amd import decode
    stem, takes_stats, kwargs = FAMILIES[family]
    suffix, points, tours = form_args(inputs, form)
    kw = kwargs(inputs, form, dev)
    stats = {}
    if takes_stats:
        kw["stats"] = stats
    before = np.array(tours[0] if suffix == "ragged" else tours, copy=True)
    ret = getattr(decode, f"batched_{stem}_{suffix}")(points, tours, CAP, dev, **kw)
    assert np.array_equal(before, tours[0] if suffix == "ragged" else tours), "the caller's tours were written"
    return {"returned": encode(ret), "stats": encode(stats)}


def tsp_gpu_refusal_calls(dev, inputs):
    """The shape errors of the guided call that need the heat on the device before they can be raised."""
    from difusco_amd.decode import batched_iterated_search_ragged
    _, points, tours = form_args(inputs, "ragged")
    good = heat_args(inputs, "ragged", "sparse", dev)
    dense = heat_args(inputs, "ragged", "dense", dev)

    def call(heat, edge_index):
        return lambda: batched_iterated_search_ragged(points, tours, CAP, dev, kicks=1, kick_bias="heat", heat=heat, edge_index=edge_index)

    def swap(seq, g, v):
        return [v if i == g else x for i, x in enumerate(seq)]
    ei1 = good["edge_index"][1]
    return {
        "dense_numel": call(swap(dense["heat"], 2, dense["heat"][2][:, :-1]), None),
        "edge_index_1d": call(good["heat"], swap(good["edge_index"], 1, ei1[0])),
        "sparse_numel": call(swap(good["heat"], 1, good["heat"][1][:, :-1]), good["edge_index"]),
        "city_outside": call(good["heat"], swap(good["edge_index"], 1, ei1 + 40 * (np.arange(ei1.shape[1]) == 5))),
        "city_negative": call(good["heat"], swap(good["edge_index"], 1, ei1 - 41 * (np.arange(ei1.shape[1]) == 5))),
    }


# ---- the MIS wrappers


MIS_GRAPHS = ("g30", "empty", "two")
MIS_RUNS = [(graph, how) for graph in MIS_GRAPHS for how in ("numpy", "tensor")]


def mis_run(dev, inputs, graph, how):
    """The three MIS wrappers on one graph.  ``numpy``: the solution as a numpy array and the graph as its edge list;
    ``tensor``: the solution as a device tensor, which the call must leave as it was, and the graph as a built ``CsrGraph``."""
    from difusco_amd.decode import mis_decode_np, mis_iterated_search_np, mis_local_search_np
    from difusco_amd.graph import build_csr
    g = inputs["mis"][graph]
    n = len(g["scores"])
    scores = np.array(g["scores"], dtype=np.float32) / HEAT_GRID
    ei = np.array(g["edge_index"], dtype=np.int64).reshape(2, -1)
    start = np.array(g["solution"], dtype=np.int64)
    if how == "tensor":
        where = dict(graph=build_csr(torch.from_numpy(ei), n, dev), device=dev)
        scores = torch.from_numpy(scores).to(dev)
        sol = torch.from_numpy(start).to(dev)
    else:
        where = dict(edge_index=ei, device=dev)
        sol = start.copy()
    rows = g.get("instance_rows")
    B = 1 if rows is None else len(rows) - 1
    out = {}
    stats = {}
    out["decode"] = {"returned": encode(mis_decode_np(scores, stats=stats, **where)), "stats": encode(stats)}
    stats = {}
    out["local_search"] = {"returned": encode(mis_local_search_np(scores, sol, max_rounds=CAP, stats=stats, **where)),
                           "stats": encode(stats)}
    stats = {}
    ret = mis_iterated_search_np(scores, sol, instance_rows=rows, seeds=inputs["seeds"][:B], offsets=inputs["offsets"][:B], kicks=2,
                                 kick_size=2, max_rounds=CAP, stats=stats, **where)
    out["iterated_search"] = {"returned": encode(ret), "stats": encode(stats)}
    assert np.array_equal(start, sol.cpu().numpy() if how == "tensor" else sol), "the caller's solution was written"
    return out


# ---- the pipeline


PIPELINE_N, PIPELINE_P, PIPELINE_STEPS = 24, 2, 2
_MULTI = dict(local_search="multi2opt+oropt")
_KICKED = dict(_MULTI, local_search_kicks=2, local_search_kick_size=2, local_search_kick_span=8)
# setting -> (sparse_factor, keyword arguments)
PIPELINE_SETTINGS = {
    "2opt": (-1, dict(local_search="2opt")),
    "2opt+oropt": (-1, dict(local_search="2opt+oropt")),
    "multi2opt": (-1, dict(local_search="multi2opt")),
    "multi2opt+oropt": (-1, _MULTI),
    "kicks": (-1, _KICKED),
    "kicks_focused": (-1, dict(_KICKED, local_search_descent="focused")),
    "kicks_heat_dense": (-1, dict(_KICKED, local_search_kick_bias="heat")),
    "kicks_heat_sparse": (8, dict(_KICKED, local_search_kick_bias="heat")),
    "window": (-1, dict(_MULTI, local_search_window=16, local_search_passes=2, local_search_kicks=1, local_search_kick_size=2,
                        local_search_kick_span=8)),
}
PIPELINE_ENTRIES = ("solo", "batch", "mixed")
PIPELINE_RUNS = [(setting, entry) for setting in PIPELINE_SETTINGS for entry in PIPELINE_ENTRIES]


def pipeline_weights():
    from difusco_amd.synthetic import random_state_dict
    return random_state_dict(64, 2, 2, seed=0)


def pipeline_run(dev, inputs, weights, setting, entry):
    """``solve_tsp`` (``solo``), ``solve_tsp_batch`` on a [2, 24, 2] array (``batch``) or on a list of sizes [24, 12] (``mixed``):
    the whole returned value, encoded."""
    from difusco_amd import TSPModel
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    sparse_factor, kw = PIPELINE_SETTINGS[setting]
    args = dict(diffusion_type="categorical", inference_schedule="cosine", inference_diffusion_steps=PIPELINE_STEPS,
                sparse_factor=sparse_factor, hidden_dim=64, n_layers=2)
    pts = np.array(inputs["pipeline_points"], dtype=np.float64)
    kw = dict(kw, parallel_sampling=PIPELINE_P, sequential_sampling=2, two_opt_iterations=CAP)
    if entry == "solo":
        model = TSPModel(args, weights, device=dev, seed=21)
        return encode(solve_tsp(model, pts[0], sparse_factor, generator=torch.Generator().manual_seed(0), **kw))
    model = TSPModel(args, weights, device=dev, seed=0)
    points = pts if entry == "batch" else [pts[0], pts[1][:PIPELINE_N // 2]]
    return encode(solve_tsp_batch(model, points, sparse_factor, seeds=[21, 22],
                                  generators=[torch.Generator().manual_seed(b) for b in range(2)], **kw))


def gpu_results(dev, inputs):
    """Every GPU case by name."""
    weights = pipeline_weights()
    doc = {"tsp": {f"{family}/{form}": tsp_run(dev, inputs, family, form) for family, form in TSP_RUNS},
           "tsp_refusals": {name: refusal(call) for name, call in tsp_gpu_refusal_calls(dev, inputs).items()},
           "mis": {f"{graph}/{how}": mis_run(dev, inputs, graph, how) for graph, how in MIS_RUNS},
           "pipeline": {f"{setting}/{entry}": pipeline_run(dev, inputs, weights, setting, entry) for setting, entry in PIPELINE_RUNS}}
    return doc


# ---- the refusals that need no device


def refusal(call):
    """[type name, message] of what ``call`` raises."""
    try:
        call()
    except Exception as e:  # noqa: BLE001 - the type is what is recorded
        return [type(e).__name__, str(e)]
    return ["no exception", ""]


_ITER = [("max_iterations_-1", dict(max_iterations=-1)), ("max_iterations_1.5", dict(max_iterations=1.5))]
_ROUNDS = [("max_rounds_0", dict(max_rounds=0)), ("max_rounds_1.5", dict(max_rounds=1.5))]
_SELECT = [("select_rounds_0", dict(select_rounds=0)), ("select_rounds_1.5", dict(select_rounds=1.5))]
_KICK = [("kick_size_0", dict(kick_size=0)), ("kick_size_65", dict(kick_size=65)), ("span_0", dict(span=0)),
         ("span_2^31", dict(span=2 ** 31)), ("seeds_short", dict(seeds=[1])), ("seeds_long", dict(seeds=[1] * 9)),
         ("offsets_short", dict(offsets=[1])), ("offsets_long", dict(offsets=[1] * 9))]
# family -> (the keyword arguments of a valid call, [(name, the one argument that is wrong)])
HOST_VALUES = {
    "two_opt": ({}, [("method", dict(method="fast"))]),
    "local_search": ({}, _ITER + _ROUNDS),
    "multi_two_opt": ({}, _ITER + _SELECT),
    "multi_local_search": ({}, _ITER + _ROUNDS + _SELECT),
    "iterated_search": (dict(kicks=1), _ITER + _ROUNDS + _SELECT + _KICK + [
        ("kicks_-1", dict(kicks=-1)), ("kicks_2^31", dict(kicks=2 ** 31)), ("descent", dict(descent="fast")),
        ("kick_bias", dict(kick_bias="cold")), ("compact_select_max_-1", dict(compact_select_max=-1)),
        ("compact_select_max_1025", dict(compact_select_max=1025)), ("heat_without_bias", dict(heat=[])),
        ("edge_index_without_bias", dict(edge_index=[])), ("bias_without_heat", dict(kick_bias="heat")),
        ("heat_count", dict(kick_bias="heat", heat=[None] * 5)),
        ("edge_index_count", dict(kick_bias="heat", heat="per group", edge_index=[None] * 5)),
        ("edge_index_none", dict(kick_bias="heat", heat="per group", edge_index="none per group"))]),
    "window_search": (dict(window=16, kicks=1), _ITER + _ROUNDS + _SELECT + _KICK + [
        ("kicks_-1", dict(kicks=-1)), ("kicks_1025", dict(kicks=1025)), ("window_15", dict(window=15)),
        ("window_1025", dict(window=1025)), ("passes_0", dict(passes=0)), ("passes_2^31", dict(passes=2 ** 31)),
        ("philox_2^32", dict(passes=2 ** 30, kicks=2))]),
}


def _host_tsp_calls():
    from difusco_amd import decode
    pts = (np.arange(40, dtype=np.float64).reshape(20, 2) * 7 % 31) / 31
    tour = np.stack([np.concatenate([np.arange(20), [0]])] * 2)          # two tours each: one seed is never enough
    forms = {"torch": (pts, tour, 1), "grouped": (np.stack([pts, pts]), np.concatenate([tour, tour]), 2),
             "ragged": ([pts, pts[:9]], [tour, tour[:, :10]], 2)}
    calls = {}
    for family, (valid, values) in HOST_VALUES.items():
        for suffix, (p, t, G) in forms.items():
            fn = getattr(decode, f"batched_{family}_{suffix}")

            def add(name, points, tours, fn=fn, family=family, suffix=suffix, **kw):
                for k in ("heat", "edge_index"):        # one placeholder per group of the form
                    if isinstance(kw.get(k), str):
                        kw[k] = None if suffix == "torch" else [None] * G
                    elif kw.get(k) is not None and suffix == "torch":
                        kw[k] = kw[k][0] if kw[k] else np.zeros(0)
                calls[f"{family}_{suffix}/{name}"] = lambda: fn(points, tours, **kw)
            add("cpu", p, t, **dict(valid, device="cpu"))
            for name, bad in values:
                if suffix == "torch" and name in ("heat_count", "edge_index_count", "edge_index_none"):
                    continue                            # one instance: the wrapper makes the lists itself
                add(name, p, t, **dict(valid, **bad))
            if suffix == "torch":
                add("tour_width", p, t[:, :-1], **valid)
            if suffix == "grouped":
                add("points_2d", pts, t, **valid)
                add("tours_width", p, t[:, :-1], **valid)
                add("tours_rows", p, t[:3], **valid)
            if suffix == "ragged":
                add("no_groups", [], [], **valid)
                add("lists_differ", p, t[:1], **valid)
                if family != "two_opt":                 # the library refuses these two for the plain 2-opt
                    add("n_3", [pts, pts[:3]], [tour, np.array([[0, 1, 2, 0]] * 2)], **valid)
                add("P_0", p, [tour, np.zeros((0, 10), dtype=np.int64)], **valid)
                add("row_width", p, [tour, tour[:, :11]], **valid)
                add("points_1d", [pts, pts[:9].reshape(-1)], t, **valid)
    return calls


def _host_mis_calls():
    from difusco_amd.decode import mis_iterated_search_np, mis_local_search_np
    scores, sol = np.linspace(0, 1, 6, dtype=np.float32), np.zeros(6, dtype=np.int64)
    ei = np.array([[0, 1], [1, 0]], dtype=np.int64)
    calls = {}

    def local(solution=sol, **kw):
        return lambda: mis_local_search_np(scores, solution, edge_index=ei, **kw)

    def iterated(solution=sol, kicks=1, **kw):
        return lambda: mis_iterated_search_np(scores, solution, edge_index=ei, kicks=kicks, **kw)
    for name, make in (("mis_local_search_np", local), ("mis_iterated_search_np", iterated)):
        calls[f"{name}/cpu"] = make(device="cpu")
        calls[f"{name}/max_rounds_-1"] = make(max_rounds=-1)
        calls[f"{name}/max_rounds_1.5"] = make(max_rounds=1.5)
        calls[f"{name}/solution_short"] = make(solution=sol[:5])
        calls[f"{name}/solution_long"] = make(solution=np.zeros(7, dtype=np.int64))
    calls.update({"mis_iterated_search_np/kicks_-1": iterated(kicks=-1), "mis_iterated_search_np/kick_size_0": iterated(kick_size=0),
                  "mis_iterated_search_np/instance_rows_one": iterated(instance_rows=[0]),
                  "mis_iterated_search_np/instance_rows_none": iterated(instance_rows=[]),
                  "mis_iterated_search_np/seeds_short": iterated(instance_rows=[0, 2, 6], seeds=[1]),
                  "mis_iterated_search_np/seeds_long": iterated(seeds=[1, 2]),
                  "mis_iterated_search_np/offsets_short": iterated(instance_rows=[0, 2, 6], offsets=[1]),
                  "mis_iterated_search_np/offsets_long": iterated(offsets=[1, 2])})
    return calls


def host_refusals():
    """name -> [type name, message] of every refusal that a wrapper raises from its arguments alone."""
    return {name: refusal(call) for name, call in {**_host_tsp_calls(), **_host_mis_calls()}.items()}
