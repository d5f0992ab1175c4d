"""The inference flow of ``TSPModel.test_step`` (``difusco/pl_tsp_model.py:153-256``) and ``MISModel.test_step``
(``difusco/pl_mis_model.py:142-209``) without Lightning, every stage on the GPU path of this package: k-NN graph ->
``sequential_sampling`` rounds of ``parallel_sampling`` noise samples through the denoising loop -> heatmap -> greedy
tour merge -> batched 2-opt -> best tour.  ``solve_tsp`` / ``solve_mis`` take one instance per call, like the reference (its
test batch size is 1); ``solve_tsp_batch`` / ``solve_mis_batch`` solve many instances per pass with the same per-instance
answers (one sampling loop over their union, per-instance statistics and random streams, grouped 2-opt; TSP instances of
different sizes as a list: ragged k-NN and ragged 2-opt).  In both the
parallel samples form the batch of the denoise steps (disjoint union, ``duplicate_edge_index``), the sequential rounds
repeat the whole loop with fresh noise and stack the results (``pl_tsp_model.py:185,238,240``).

This is host-side orchestration only - each stage is one of the drop-in entry points (``graph.knn_edge_index_gpu``,
``TSPModel.sample``, ``decode.merge_tours``, ``decode.batched_two_opt_torch``) and can be used on its own."""
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import decode
from .decode import (TSP_KICK_SIZE, TSP_KICK_SPAN, TSP_KOPT_DEPTH, TSP_KOPT_SAMPLES, check_local_search, check_tsp_kopt, check_tsp_candidates, check_tsp_candidate_source, check_merge_method, check_tsp_descent, check_tsp_kick_bias,
                     check_tsp_kicks, check_tsp_local_search_mode, check_tsp_window, check_two_opt_method, check_two_opt_mode, merge_tours,
                     merge_tours_batch)
from .graph import knn_edge_index_gpu


def tour_length(points: np.ndarray, tour) -> float:
    """``TSPEvaluator.evaluate`` (``utils/tsp_utils.py:148-156``) without the N x N distance matrix."""
    t = np.asarray(tour)
    return float(np.linalg.norm(points[t[:-1]] - points[t[1:]], axis=1).sum())


def _ticker(timings, dev):
    def tick(name, t0):
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0
    return tick


def solve_tsp(model, points: np.ndarray, sparse_factor: int, parallel_sampling: int = 1, two_opt_iterations: int = 1000,
              generator: Optional[torch.Generator] = None, timings: Optional[Dict[str, float]] = None,
              sequential_sampling: int = 1, *, graphed: bool = False, two_opt_method: str = "exact",
              local_search: str = "2opt", local_search_kicks: int = 0, local_search_kick_size: int = TSP_KICK_SIZE,
              local_search_kick_span: int = TSP_KICK_SPAN, local_search_descent: str = "full",
              local_search_kick_bias: str = "uniform", local_search_window: int = 0, local_search_passes: int = 1,
              two_opt_mode: str = "launches", local_search_candidates: int = 0, local_search_closing: bool = True,
              local_search_mode: str = "launches", kopt_rounds: int = 0, kopt_samples: int = TSP_KOPT_SAMPLES,
              kopt_depth: int = TSP_KOPT_DEPTH, local_search_candidate_source: str = "knn"):
    """points: float64/float32 [N,2] of ONE instance.  ``sparse_factor`` > 0: k-NN graph (the sparse models);
    <= 0: dense mode (``pl_tsp_model.py:158-160``, TSP-50/100).  Returns (best_tour list, best_cost, all_costs, info):
    ``all_costs`` has ``parallel_sampling * sequential_sampling`` entries in the reference's stacking order, info holds
    merge_iterations / 2-opt moves of the LAST round - the quantities the reference logs (``pl_tsp_model.py:244-251``).
    ``graphed=True``: every sampling loop runs as one replay of a captured HIP graph (``TSPModel.sample``), same results.
    ``two_opt_method``: "exact" or "screened" (``decode.batched_two_opt_torch``), same results.  ``local_search``: "2opt"
    (default) or "2opt+oropt" (``decode.batched_local_search_torch`` with ``max_iterations=two_opt_iterations``: never a longer
    tour; info gains ``or_opt_iterations`` and ``local_search_rounds`` of the last round; exact sweep only) or "multi2opt"
    (``decode.batched_multi_two_opt_torch``: every sweep applies all disjoint improving moves it selects, another 2-opt optimum;
    ``two_opt_iterations`` of info is the sweep count and info gains ``two_opt_moves``, both of the last round; exact sweep only)
    or "multi2opt+oropt" (``decode.batched_multi_local_search_torch`` with ``max_iterations=two_opt_iterations``: rounds of
    multi-move 2-opt and multi-move Or-opt sweeps, never a longer tour than "multi2opt"; ``two_opt_iterations`` of info is the
    2-opt sweep count, info gains ``two_opt_moves``, ``or_opt_iterations`` (the Or-opt sweeps), ``or_opt_moves`` and
    ``local_search_rounds``, all of the last round; exact sweep only).  ``local_search_kicks`` > 0 (only with
    "multi2opt+oropt", else ``ValueError``): that search iterated with that many seeded kicks of up to
    ``local_search_kick_size`` segment swaps within ``local_search_kick_span`` cities (``decode.batched_iterated_search_torch``;
    never a longer tour); copy p of sequential round r is its own tour, keyed by the model's seed at the Philox offset
    ``2^62 + (r P + p) 2^32``; info gains ``local_search_kicks_improved`` of the last round (a list, one per copy).  0 is the
    plain search.  ``local_search_descent``: "full" (default) or "focused" (only with ``local_search_kicks`` > 0, else
    ``ValueError``): the descents after the kicks evaluate only the candidates next to a touched edge and one full descent
    closes the search (``descent="focused"`` of ``decode.batched_iterated_search_torch``); info gains
    ``local_search_closing_sweeps`` of the last round (a list, one per copy).  ``local_search_kick_bias``: "uniform" (default)
    or "heat" (only with ``local_search_kicks`` > 0, else ``ValueError``): the first cut of every draw of a kick falls on a tour
    edge with a probability that rises as the heat of that edge falls (``kick_bias="heat"`` of
    ``decode.batched_iterated_search_torch``); copy p reads its own heatmap of its sequential round, the tensor the merge
    received, still on the device; info gains ``local_search_kick_bias`` ("heat"; the uniform records stay as they were).
    ``local_search_window`` = W > 0 (only with "multi2opt+oropt", a full descent and uniform kicks, else ``ValueError``; 0, the
    default, changes nothing): the windowed iterated search (``decode.batched_window_search_torch``) with
    ``local_search_passes`` passes over windows of W positions and ``local_search_kicks`` kicks (>= 0) per window and pass, of
    ``local_search_kick_size`` and ``local_search_kick_span``; the copies are keyed as above; info gains
    ``local_search_window``, ``local_search_passes`` and, of the last round, one per copy, ``local_search_kicks_improved``,
    ``local_search_passes_kept`` and ``local_search_closing_sweeps``.  ``two_opt_mode``: "launches" (default) or "resident"
    (only with ``local_search="2opt"``, else ``ValueError``): the 2-opt runs with one GPU block for the instance
    (``mode="resident"`` of ``decode.batched_two_opt_torch``), same results with either ``two_opt_method``; the
    ``parallel_sampling`` tours must fit its limit, there is no fallback.  ``local_search_candidates`` = K > 0 (only with
    "multi2opt", no kicks, no window, not "resident", else ``ValueError``; 0, the default, changes nothing): the neighbour-list
    multi-move 2-opt (``decode.batched_nbr_two_opt_torch``): sweeps over the K listed neighbours of every city, then, with
    ``local_search_closing`` (default), full sweeps until one finds nothing.  With ``sparse_factor`` > 0 and K <=
    ``sparse_factor`` - 1 the lists are the first K non-self neighbours of the instance's own ``edge_index``, else the K nearest
    cities of a k-NN call of their own.  info gains ``local_search_candidates``, ``local_search_closing`` and
    ``two_opt_full_sweeps`` (of the last round).  ``local_search="nbr2opt+oropt"`` (needs ``local_search_candidates`` = K >= 1,
    K = 0 is a ``ValueError``; accepts ``local_search_closing``; no kicks, no window, not "resident"): the 2-opt + Or-opt search
    of "multi2opt+oropt" on the same lists (``decode.batched_nbr_local_search_torch``), closed by full rounds with
    ``local_search_closing``.  It is a name of its own, not "multi2opt+oropt" with K > 0: that combination stays refused, as the
    host tests of the neighbour-list 2-opt pin.  info holds what "multi2opt+oropt" gives, ``local_search_candidates``,
    ``local_search_closing``, ``local_search_full_sweeps`` and ``local_search_full_rounds``.  ``local_search_mode``: "launches"
    (default) or "resident" (only with ``local_search="2opt+oropt"``, else ``ValueError``): that search runs with one GPU block
    for the instance (``mode="resident"`` of ``decode.batched_local_search_torch``), same tours and info; the
    ``parallel_sampling`` tours must fit its limit, there is no fallback.  ``kopt_rounds`` = R > 0 (0, the default, changes
    nothing: results and info are what they are without the option): after the chosen local search, and before the best tour is
    picked, every tour runs up to R rounds of the heatmap-guided sampled k-opt search (``decode.batched_kopt_search_torch``) with
    ``kopt_samples`` simulations per round and moves of up to ``kopt_depth`` new edges, on its own heatmap of its sequential
    round (the tensor the merge received) - never a longer tour.  Copy p of sequential round r is keyed by the model's seed at
    the Philox offset ``3 * 2^61 + (r P + p) 2^32``, which no kick offset of the same tour reaches.  info gains ``kopt_rounds``,
    ``kopt_samples``, ``kopt_depth`` and, of the last round, one per copy, ``kopt_rounds_run`` and ``kopt_actions``.
    ``local_search_candidate_source``: "knn" (default: every result and info is what it is without the option) or "heat" (needs
    ``local_search_candidates`` = K >= 1, else ``ValueError``): the neighbour lists of "multi2opt" with K > 0 and of
    "nbr2opt+oropt" are ranked by heat, not distance (``decode.tsp_heat_candidate_lists``), from the round's own heatmaps and
    graph - the dense heatmaps in dense mode - so every sequential round builds its own lists; info gains
    ``local_search_candidate_source`` ("heat") and ``local_search_heat_listed``, the share of the last round's list slots that
    hold a city with a score above 0."""
    kopt = check_tsp_kopt(kopt_rounds, kopt_samples, kopt_depth)
    check_two_opt_method(two_opt_method)
    check_local_search(local_search, two_opt_method)
    two_opt_mode = check_two_opt_mode(local_search, two_opt_mode)
    ls_mode = check_tsp_local_search_mode(local_search, local_search_mode)
    kicks, kick_size, kick_span = check_tsp_kicks(local_search, local_search_kicks, local_search_kick_size, local_search_kick_span)
    descent = check_tsp_descent(local_search_descent, kicks)
    kick_bias = check_tsp_kick_bias(local_search_kick_bias, kicks)
    window, passes = check_tsp_window(local_search, local_search_window, local_search_passes, kicks, descent, kick_bias)
    nbr = (check_tsp_candidates(local_search, local_search_candidates, kicks, window, two_opt_mode), bool(local_search_closing))
    nbr += (check_tsp_candidate_source(local_search_candidate_source, nbr[0]),)
    search = (local_search, (two_opt_method, two_opt_mode, ls_mode), window, passes, kicks, kick_size, kick_span, descent, kick_bias, nbr)
    dev = model.device
    pts64 = np.ascontiguousarray(points, dtype=np.float64)
    n = pts64.shape[0]
    sparse = sparse_factor is not None and sparse_factor > 0
    tick = _ticker(timings, dev)

    t0 = time.perf_counter()
    edge_index = knn_edge_index_gpu(pts64, sparse_factor, device=dev) if sparse else None    # tsp_graph_dataset.py:53-62
    tick("knn", t0)
    # the reference's np_points are the float32 coordinates of the batch (graph_data.x / points tensor); merge, 2-opt
    # (after .astype("float64")) and the cost evaluation all start from these rounded values (pl_tsp_model.py:159,172,233,240)
    pts32 = torch.from_numpy(pts64.astype(np.float32)).to(dev)
    np_points = pts32.cpu().numpy()
    np_points64 = np_points.astype(np.float64)
    if sparse:
        pts_rep = pts32.repeat(parallel_sampling, 1)                                        # :178-183
        ei_rep = model.duplicate_edge_index(edge_index, n, dev, copies=parallel_sampling) if parallel_sampling > 1 else edge_index
    else:
        pts_rep, ei_rep = pts32.reshape(1, n, 2).repeat(parallel_sampling, 1, 1), None

    stacked, merged_costs = [], []
    merge_iterations, ns = 0.0, 0
    ls_stats, kick_stats, kopt_stats = {}, {}, {}
    for r in range(sequential_sampling):                                                    # :185
        t0 = time.perf_counter()
        heat = model.sample(pts_rep, ei_rep, generator=generator, graphed=graphed)          # :186-222, on the device
        tick("sampling", t0)
        t0 = time.perf_counter()
        tours, merge_iterations = merge_tours(heat, pts32, edge_index, sparse_graph=sparse,  # :226-230
                                              parallel_sampling=parallel_sampling, device=dev)
        tick("merge", t0)
        t0 = time.perf_counter()
        solved, ns, ls_stats = _local_search("torch", search, np_points64, np.asarray(tours, dtype=np.int64), two_opt_iterations, dev,
                                             [_kick_key(model.seed)] * parallel_sampling, _kick_offsets(r, parallel_sampling),
                                             heat, edge_index, kick_stats)
        if kopt[0] > 0:
            solved = _kopt_stage("torch", kopt, np_points64, solved, dev, [_kick_key(model.seed)] * parallel_sampling,
                                 _kopt_offsets(r, parallel_sampling), heat, edge_index, kopt_stats)
        tick("two_opt", t0)
        stacked.append(solved)
        merged_costs += [tour_length(np_points64, t) for t in tours]
    solved = np.concatenate(stacked, axis=0)                                                # :238
    costs = [tour_length(np_points64, t) for t in solved]                                   # :240-246
    best = int(np.argmin(costs))
    info = {"merge_iterations": merge_iterations, "two_opt_iterations": ns, "merged_costs": merged_costs}
    info.update(_local_search_info(search, ls_stats, kick_stats, 0, parallel_sampling, 0))
    info.update(_kopt_info(kopt, kopt_stats, 0, parallel_sampling))
    return solved[best].tolist(), costs[best], costs, info


def solve_mis(model, n_nodes: int, edge_index, parallel_sampling: int = 1, generator: Optional[torch.Generator] = None,
              timings: Optional[Dict[str, float]] = None, sequential_sampling: int = 1, *, graphed: bool = False,
              local_search: str = "none", local_search_rounds: int = 1000, stats: Optional[dict] = None,
              local_search_kicks: int = 0, local_search_kick_size: int = 4, local_search_mode: str = "launches"):
    """``MISModel.test_step`` (``difusco/pl_mis_model.py:142-206``): ``sequential_sampling`` rounds of
    ``parallel_sampling`` noise samples of ONE graph through the denoising loop (disjoint union), greedy decode of every
    sample, best = largest set.  ``edge_index``: int64 [2,E] in the dataset's layout (both directions + self loops).
    Returns (best 0/1 array, best size, sizes).  Upstream re-duplicates ``edge_index`` inside the sequential loop
    (``pl_mis_model.py:168-169``), which breaks ``parallel > 1 and sequential > 1`` there; here the duplication happens
    once, which is what that combination means.  ``graphed=True``: every sampling loop is one graph replay
    (``MISModel.sample``), same results.  ``local_search``: "none" (default) or "swap": every decode is followed by one
    ``decode.mis_local_search_np`` call on the same graph (all P copies at once, at most ``local_search_rounds`` rounds): never
    a smaller set.  ``stats`` (a dict) then receives ``decoded_sizes`` (the greedy sizes in the order of ``sizes``) and the
    call counters ``rounds``, ``swaps``, ``inserts`` summed over the sequential rounds.  ``local_search_kicks`` > 0 (only with
    "swap", else ``ValueError``): the search is iterated with that many seeded kicks of about ``local_search_kick_size`` nodes
    (``decode.mis_iterated_search_np``); copy p of sequential round r is its own instance of the call, keyed by the model's
    seed at Philox offset ``2^62 + (r P + p) 2^32``.  ``stats`` then also receives ``swap_sizes`` (the sizes after
    the first descent), ``kicks_entered`` and ``kicks_accepted``, in the order of ``sizes``.  0 is the plain swap search.
    ``local_search_mode``: "launches" (default) or "resident" (only with "swap", else ``ValueError``): the search, with any
    number of kicks >= 0, runs as ``decode.mis_iterated_search_np(mode="resident")``, one GPU block per copy, on the same
    instance rows, seeds and offsets; results and ``stats`` are those of "launches"."""
    from .decode import (check_mis_kicks, check_mis_local_search, check_mis_search_mode, mis_decode_np, mis_iterated_search_np,
                         mis_local_search_np)
    check_mis_local_search(local_search)
    kicks, kick_size = check_mis_kicks(local_search, local_search_kicks, local_search_kick_size)
    mode = check_mis_search_mode(local_search, local_search_mode)
    kick_stats = {"swap_sizes": [], "kicks_entered": [], "kicks_accepted": []}
    dev = model.device
    ei = edge_index if isinstance(edge_index, torch.Tensor) else torch.from_numpy(np.asarray(edge_index))
    ei = ei.to(dev)
    tick = _ticker(timings, dev)
    ei_rep = model.duplicate_edge_index(ei, n_nodes, dev, copies=parallel_sampling) if parallel_sampling > 1 else ei   # pl_mis_model.py:168-169
    graph = model.prepare_graph(ei_rep, n_nodes * parallel_sampling)
    sols, decoded, counters = [], [], {"rounds": 0, "swaps": 0, "inserts": 0}
    for r in range(sequential_sampling):                                                          # :156
        t0 = time.perf_counter()
        scores = model.sample(n_nodes * parallel_sampling, ei_rep, generator=generator, graphed=graphed)   # :157-192
        tick("sampling", t0)
        t0 = time.perf_counter()
        sol = mis_decode_np(scores, graph=graph, device=dev)                                      # :195-198
        tick("decode", t0)
        if local_search == "swap":
            t0 = time.perf_counter()
            decoded += sol.reshape(parallel_sampling, n_nodes).sum(axis=1).tolist()
            call = {}
            if kicks > 0 or mode == "resident":
                P = parallel_sampling
                sol = mis_iterated_search_np(scores, sol, graph=graph, device=dev, max_rounds=local_search_rounds, stats=call,
                                             kicks=kicks, kick_size=kick_size, instance_rows=[n_nodes * p for p in range(P + 1)],
                                             seeds=[model.seed] * P, offsets=_kick_offsets(r, P), mode=mode)
                _kick_stats(kick_stats, call, 0, P)
            else:
                sol = mis_local_search_np(scores, sol, graph=graph, device=dev, max_rounds=local_search_rounds, stats=call)
            for k in counters:
                counters[k] += call[k]
            tick("local_search", t0)
        sols.append(sol.reshape(parallel_sampling, n_nodes))
    sol = np.concatenate(sols, axis=0)
    sizes = sol.sum(axis=1)
    best = int(np.argmax(sizes))
    if local_search == "swap" and stats is not None:
        stats.update(decoded_sizes=decoded, **counters, **(kick_stats if kicks > 0 else {}))
    return sol[best], int(sizes[best]), sizes.tolist()


def _kick_offsets(r: int, P: int):
    """Philox offsets of the kick streams of the P copies of sequential round ``r``: copy p of the round is the (r P + p)-th
    copy of its instance and owns the 2^32 offsets from ``2^62 + (r P + p) 2^32``; the sampling draws at small step counters
    under the same key, so the streams cannot meet."""
    from .decode import MIS_KICK_OFFSET
    return [MIS_KICK_OFFSET + ((r * P + p) << 32) for p in range(P)]


def _kick_key(seed) -> int:
    """A sampling seed as the Philox key of a kick stream: the way ``sample_batch`` resolves it."""
    return int(seed) & (2 ** 63 - 1)


TSP_KOPT_OFFSET = 3 << 61       # first Philox offset of the k-opt streams: 2^61 above the first kick offset (2^62)


def _kopt_offsets(r: int, P: int):
    """Philox offsets of the k-opt streams of the P copies of sequential round ``r``: copy p owns the 2^32 offsets from
    ``3 * 2^61 + (r P + p) 2^32`` (round t of the search draws at + t).  The kick offsets of the same copy lie in
    ``2^62 + (r P + p) 2^32 + [0, 2^32)`` (``_kick_offsets``), 2^61 below: the two cannot meet for fewer than 2^29 copies."""
    return [TSP_KOPT_OFFSET + ((r * P + p) << 32) for p in range(P)]


def _kopt_stage(form: str, kopt: tuple, points, tours, dev, seeds, offsets, heat, edge_index, kopt_stats):
    """The sampled k-opt search of one round on the tours the local search returned, through the ``decode.batched_kopt_search_*``
    wrapper of ``form``; ``kopt``: the checked (rounds, samples, depth), rounds > 0.  ``kopt_stats`` receives the per-tour
    arrays."""
    rounds, samples, depth = kopt
    return getattr(decode, f"batched_kopt_search_{form}")(points, tours, heat=heat, edge_index=edge_index, samples=samples,
                                                          depth=depth, rounds=rounds, seeds=seeds, offsets=offsets,
                                                          stats=kopt_stats, device=dev)


def _kopt_info(kopt: tuple, kopt_stats: dict, first: int, P: int) -> dict:
    """What info gains from the k-opt stage of the last round (nothing when it is off)."""
    if kopt[0] == 0:
        return {}
    cut = lambda k: [int(v) for v in kopt_stats[k][first:first + P]]
    return dict(kopt_rounds=kopt[0], kopt_samples=kopt[1], kopt_depth=kopt[2], kopt_rounds_run=cut("rounds"),
                kopt_actions=cut("actions"))


def _local_search(form: str, search: tuple, points, tours, two_opt_iterations, dev, seeds, offsets, heat, edge_index, kick_stats):
    """The local search of one round on the merged tours, through the ``decode.batched_*`` wrapper of ``form`` ("torch",
    "grouped" or "ragged") that ``search`` - the checked (local_search, (two_opt_method, two_opt_mode, local_search_mode), window, passes, kicks, kick_size,
    kick_span, descent, kick_bias) - selects.  ``seeds`` / ``offsets``: the Philox key and first offset of every tour, read by
    the kicked searches, as ``heat`` / ``edge_index`` (the round's heatmaps and their graphs) are by heat-biased kicks;
    ``kick_stats`` receives their per-tour arrays.  Returns (tours, iterations, the search's own statistics)."""
    local_search, (two_opt_method, two_opt_mode, ls_mode), window, passes, kicks, kick_size, kick_span, descent, kick_bias, nbr = search
    run = lambda stem, **kw: getattr(decode, f"batched_{stem}_{form}")(points, tours, max_iterations=two_opt_iterations, device=dev, **kw)
    ls_stats = {}
    lists = lambda: _candidate_lists(form, points, edge_index, nbr[0], nbr[2], heat, dev)
    if local_search == "2opt":
        solved, iterations = run("two_opt", method=two_opt_method,                              # pl_tsp_model.py:233-236
                                 **(dict(mode="resident") if two_opt_mode == "resident" else {}))
    elif local_search == "multi2opt" and nbr[0] > 0:
        neighbors, heat_stats = lists()
        solved, iterations = run("nbr_two_opt", candidates=nbr[0], closing=nbr[1], stats=ls_stats, neighbors=neighbors)
        ls_stats.update(heat_stats)
    elif local_search == "multi2opt":
        solved, iterations = run("multi_two_opt", stats=ls_stats)
    elif local_search == "2opt+oropt":
        solved, iterations = run("local_search", stats=ls_stats, **(dict(mode="resident") if ls_mode == "resident" else {}))
    elif local_search == "nbr2opt+oropt":
        neighbors, heat_stats = lists()
        solved, ls_stats = run("nbr_local_search", candidates=nbr[0], closing=nbr[1], neighbors=neighbors)
        ls_stats = dict(ls_stats, **heat_stats)
        iterations = ls_stats["two_opt_sweeps"]
    else:
        kicked = dict(kicks=kicks, kick_size=kick_size, span=kick_span, seeds=seeds, offsets=offsets, stats=kick_stats)
        if window > 0:
            solved, ls_stats = run("window_search", window=window, passes=passes, **kicked)
        elif kicks > 0:
            solved, ls_stats = run("iterated_search", descent=descent, **kicked,
                                   **(dict(kick_bias="heat", heat=heat, edge_index=edge_index) if kick_bias == "heat" else {}))
        else:
            solved, ls_stats = run("multi_local_search")
        iterations = ls_stats["two_opt_sweeps"]
    return solved, iterations, ls_stats


def _candidate_lists(form: str, points, edge_index, K: int, source: str = "knn", heat=None, dev=None):
    """(the neighbour lists of the K-candidate searches, what the statistics of the search gain).  ``source="knn"``: from the
    instances' own k-NN graphs (``edge_index`` of the form: one [2, n k] tensor, or one per instance with local node ids) where
    they hold K other cities per node; else None, and the search builds the lists with a k-NN call of its own.
    ``source="heat"``: ``decode.tsp_heat_candidate_lists`` on ``heat`` - the round's heatmaps, one [P, E] or dense [P, n, n] per
    instance - and the same graphs, one library call; the statistics gain ``heat_listed``, per instance the share of its n K
    list slots that hold a city with a score above 0."""
    if source == "heat":
        st = {}
        # a sparse heatmap comes flat, the P samples of an instance one after the other: [P E] -> [P, E]
        rows = lambda h, e: h if e is None else h.reshape(-1, e.shape[1])
        if form == "torch":
            lists = decode.tsp_heat_candidate_lists(np.asarray(points), rows(heat, edge_index), edge_index, K, device=dev, stats=st)
            return lists, dict(heat_listed=np.array([st["listed"] / (len(points) * K)]))
        eis = None if edge_index is None else list(edge_index)
        heats = [rows(h, None if eis is None else eis[g]) for g, h in enumerate(heat)]
        lists = decode.tsp_heat_candidate_lists([np.asarray(p) for p in points], heats, eis, K, device=dev, stats=st)
        return lists, dict(heat_listed=st["listed"] / np.array([len(p) * K for p in points], dtype=np.float64))
    if edge_index is None:
        return None, {}
    eis = [edge_index] if form == "torch" else list(edge_index)
    sizes = [len(points)] if form == "torch" else [len(p) for p in points]
    if any(e.shape[1] // n - 1 < K for e, n in zip(eis, sizes)):
        return None, {}
    lists = decode.tsp_candidate_lists(eis, sizes, K)
    return (lists[0] if form == "torch" else lists), {}


def _local_search_info(search: tuple, ls_stats: dict, kick_stats: dict, first: int, P: int, g: int) -> dict:
    """What info gains from the local search of the last round: the statistics of group ``g`` of the call (``solve_tsp``: 0,
    its scalars are ints already) and the per-copy arrays of its copies first .. first + P - 1."""
    local_search, _, window, passes, kicks, _, _, descent, kick_bias, nbr = search
    at = lambda k: int(np.reshape(ls_stats[k], -1)[g])
    cut = lambda k: [int(v) for v in kick_stats[k][first:first + P]]
    if local_search == "2opt":
        return {}
    heat_lists = dict(local_search_candidate_source="heat", local_search_heat_listed=float(np.reshape(ls_stats["heat_listed"], -1)[g])) \
        if nbr[2] == "heat" else {}
    if local_search == "multi2opt" and nbr[0] > 0:
        return dict(two_opt_moves=at("moves"), local_search_candidates=nbr[0], local_search_closing=nbr[1],
                    two_opt_full_sweeps=at("full_sweeps"), **heat_lists)
    if local_search == "multi2opt":
        return dict(two_opt_moves=at("moves"))
    if local_search == "2opt+oropt":
        return dict(or_opt_iterations=at("or_opt_iterations"), local_search_rounds=at("rounds"))
    info = dict(two_opt_moves=at("two_opt_moves"), or_opt_iterations=at("or_opt_sweeps"), or_opt_moves=at("or_opt_moves"),
                local_search_rounds=at("rounds"))
    if local_search == "nbr2opt+oropt":
        info.update(local_search_candidates=nbr[0], local_search_closing=nbr[1], local_search_full_sweeps=at("full_sweeps"),
                    local_search_full_rounds=at("full_rounds"), **heat_lists)
    elif window > 0:
        info.update(local_search_window=window, local_search_passes=passes, local_search_kicks_improved=cut("kicks_improved"),
                    local_search_passes_kept=cut("passes_kept"), local_search_closing_sweeps=cut("closing_sweeps"))
    elif kicks > 0:
        info.update(local_search_kicks_improved=cut("kicks_improved"))
        if kick_bias == "heat":
            info.update(local_search_kick_bias="heat")
        if descent == "focused":
            info.update(local_search_closing_sweeps=cut("closing_sweeps"))
    return info


def _kick_stats(out: dict, call: dict, first: int, P: int):
    for k, src in (("swap_sizes", "size_before"), ("kicks_entered", "entered"), ("kicks_accepted", "accepted")):
        out[k] += call[src][first:first + P]


def _chunks(B: int, per_call: Optional[int]):
    if per_call is not None and int(per_call) < 1:
        raise ValueError("instances_per_call must be >= 1")
    step = B if per_call is None else int(per_call)
    return [(s, min(B, s + step)) for s in range(0, B, step)]


def _per_instance(v, B: int, name: str):
    if v is None:
        return None
    v = list(v)
    if len(v) != B:
        raise ValueError(f"{name}: {len(v)} entries for {B} instances")
    return v


def _round_offset(model, step_offset: Optional[int], r: int) -> Optional[int]:
    """First Philox offset of sequential round ``r`` of a call that starts at ``step_offset`` (None: the engine's counter)."""
    return None if step_offset is None else int(step_offset) + r * int(model.args.inference_diffusion_steps)


def solve_tsp_batch(model, points, sparse_factor: int, parallel_sampling: int = 1, sequential_sampling: int = 1,
                    two_opt_iterations: int = 1000, seeds: Optional[Sequence[int]] = None,
                    generators: Optional[Sequence[torch.Generator]] = None, timings: Optional[Dict[str, float]] = None,
                    instances_per_call: Optional[int] = None, step_offset: Optional[int] = None,
                    heatmaps: Optional[list] = None, *, two_opt_method: str = "exact",
                    merge_method: str = "loop", local_search: str = "2opt", local_search_kicks: int = 0,
                    local_search_kick_size: int = TSP_KICK_SIZE, local_search_kick_span: int = TSP_KICK_SPAN,
                    local_search_descent: str = "full", local_search_kick_bias: str = "uniform", local_search_window: int = 0,
                    local_search_passes: int = 1, two_opt_mode: str = "launches", local_search_candidates: int = 0,
                    local_search_closing: bool = True, local_search_mode: str = "launches", kopt_rounds: int = 0,
                    kopt_samples: int = TSP_KOPT_SAMPLES, kopt_depth: int = TSP_KOPT_DEPTH,
                    local_search_candidate_source: str = "knn") -> List[tuple]:
    """``solve_tsp`` of B instances: ``points`` [B, N, 2], or a sequence of B arrays [n_b, 2] of any sizes (one ragged k-NN
    sequence, one sampling loop, per-instance merges and one ragged 2-opt per chunk: ``_solve_tsp_list``).  Returns the list of what ``solve_tsp`` returns for
    every instance, run with ``seed = seeds[b]`` (default: the model's) and ``generator = generators[b]``.  Up to
    ``instances_per_call`` instances (default: all) share one k-NN launch sequence, one sampling loop over their union
    (``TSPModel.sample_batch``) and one grouped 2-opt; the merge runs per instance.  The step offsets come from the engine's
    call counter, as in ``solve_tsp``: with a fresh engine the first group of instances matches solo calls on fresh engines.
    ``step_offset``: every group of ``instances_per_call`` instances starts its steps at this offset instead (sequential round r
    at ``step_offset + r * inference_diffusion_steps``): ``step_offset=0`` draws what solo calls on fresh engines draw, whatever
    ran on this engine before.  ``heatmaps``: a list to which one entry per instance is appended - the host copies (numpy) of
    its ``sequential_sampling`` heatmaps, each shaped like ``TSPModel.sample``'s output (what ``test_step`` saves with
    ``--save_numpy_heatmap``); None (default) copies nothing.  ``two_opt_method``: as ``solve_tsp``.  ``merge_method``:
    ``"loop"`` (default) merges instance by instance (``decode.merge_tours``), ``"batched"`` merges the chunk in one library
    call (``decode.merge_tours_batch``): the same tours and counters.  ``local_search``: as ``solve_tsp``, per instance.
    ``local_search_kicks``, ``local_search_kick_size``, ``local_search_kick_span``: as ``solve_tsp``; every one of the P copies of
    an instance is its own tour, keyed by the instance's seed, so an instance gets what its solo call gets.
    ``local_search_descent``, ``local_search_kick_bias``: as ``solve_tsp``; "heat" passes every instance's own heatmaps of the
    round (the tensors the merge received, on the device) and its own graph.  ``local_search_window``,
    ``local_search_passes``: as ``solve_tsp``; an instance gets what its solo call gets.  ``two_opt_mode``: as ``solve_tsp``,
    one GPU block per instance, for arrays and sequences of instances alike.  ``local_search_candidates``,
    ``local_search_closing``: as ``solve_tsp``, per instance, for arrays and sequences alike.  ``local_search_mode``: as
    ``solve_tsp``, one GPU block per instance, for arrays and sequences of instances alike.  ``kopt_rounds``,
    ``kopt_samples``, ``kopt_depth``: as ``solve_tsp``; every copy of an instance is its own tour on its own heatmap, keyed by
    the instance's seed, so an instance gets what its solo call gets.  ``local_search_candidate_source``: as ``solve_tsp``, per
    instance, from its own heatmaps and graph, one library call per chunk and round."""
    kopt = check_tsp_kopt(kopt_rounds, kopt_samples, kopt_depth)
    check_two_opt_method(two_opt_method)
    check_merge_method(merge_method)
    check_local_search(local_search, two_opt_method)
    two_opt_mode = check_two_opt_mode(local_search, two_opt_mode)
    ls_mode = check_tsp_local_search_mode(local_search, local_search_mode)
    kicks, kick_size, kick_span = check_tsp_kicks(local_search, local_search_kicks, local_search_kick_size, local_search_kick_span)
    descent = check_tsp_descent(local_search_descent, kicks)
    kick_bias = check_tsp_kick_bias(local_search_kick_bias, kicks)
    window, passes = check_tsp_window(local_search, local_search_window, local_search_passes, kicks, descent, kick_bias)
    nbr = (check_tsp_candidates(local_search, local_search_candidates, kicks, window, two_opt_mode), bool(local_search_closing))
    nbr += (check_tsp_candidate_source(local_search_candidate_source, nbr[0]),)
    search = (local_search, (two_opt_method, two_opt_mode, ls_mode), window, passes, kicks, kick_size, kick_span, descent, kick_bias, nbr)
    if not isinstance(points, (np.ndarray, torch.Tensor)):      # a sequence of instances; one array keeps the equal-size path
        return _solve_tsp_list(model, points, sparse_factor, int(parallel_sampling), sequential_sampling, two_opt_iterations,
                               seeds, generators, timings, instances_per_call, step_offset, heatmaps, merge_method, search, kopt)
    pts_all = np.ascontiguousarray(points, dtype=np.float64)
    if pts_all.ndim != 3 or pts_all.shape[2] != 2 or pts_all.shape[0] < 1:
        raise ValueError("points must be [B, N, 2] with B >= 1")
    B, n = pts_all.shape[0], pts_all.shape[1]
    seeds, generators = _per_instance(seeds, B, "seeds"), _per_instance(generators, B, "generators")
    dev = model.device
    sparse = sparse_factor is not None and sparse_factor > 0
    P = int(parallel_sampling)
    tick = _ticker(timings, dev)
    results = []
    for c0, c1 in _chunks(B, instances_per_call):
        G = c1 - c0
        t0 = time.perf_counter()
        if sparse:
            ei_all = knn_edge_index_gpu(pts_all[c0:c1].reshape(-1, 2), sparse_factor, device=dev, graphs=G)
            E = n * sparse_factor
            eis = [ei_all[:, g * E:(g + 1) * E] - g * n for g in range(G)]
        tick("knn", t0)
        pts32 = torch.from_numpy(pts_all[c0:c1].astype(np.float32)).to(dev)           # [G, n, 2], as solve_tsp
        np_points64 = pts32.cpu().numpy().astype(np.float64)
        if sparse:
            pts_rep = [pts32[g].repeat(P, 1) for g in range(G)]
            ei_rep = [model.duplicate_edge_index(eis[g], n, dev, copies=P) if P > 1 else eis[g] for g in range(G)]
        else:
            pts_rep, ei_rep = [pts32[g].reshape(1, n, 2).repeat(P, 1, 1) for g in range(G)], None
        seeds_c = None if seeds is None else seeds[c0:c1]
        gens_c = None if generators is None else generators[c0:c1]
        stacked = [[] for _ in range(G)]
        merged_costs = [[] for _ in range(G)]
        heat_out = [[] for _ in range(G)]
        merge_its = [0.0] * G
        ns = np.zeros(G, dtype=np.int64)
        ls_stats, kick_stats, kopt_stats = {}, {}, {}
        # the Philox keys of the chunk's instances, resolved the way sample_batch resolves them
        keys = [_kick_key(v) for v in ([model.seed] * G if seeds is None else seeds_c)]
        for r in range(sequential_sampling):
            t0 = time.perf_counter()
            heats = model.sample_batch(pts_rep, ei_rep, seeds=seeds_c, generators=gens_c,
                                       step_offset=_round_offset(model, step_offset, r))
            if heatmaps is not None:
                for g in range(G):
                    heat_out[g].append(heats[g].cpu().numpy())
            tick("sampling", t0)
            t0 = time.perf_counter()
            tours = []
            if merge_method == "batched":
                for g, (tg, it) in enumerate(merge_tours_batch(heats, pts32, eis if sparse else None, sparse_graph=sparse,
                                                               parallel_sampling=P, device=dev)):
                    merge_its[g] = it
                    tours.append(tg)
            else:
                for g in range(G):
                    tg, merge_its[g] = merge_tours(heats[g], pts32[g], eis[g] if sparse else None, sparse_graph=sparse,
                                                   parallel_sampling=P, device=dev)
                    tours.append(tg)
            tick("merge", t0)
            t0 = time.perf_counter()
            solved, ns, ls_stats = _local_search("grouped", search, np_points64, np.asarray(tours, dtype=np.int64).reshape(G * P, n + 1),
                                                 two_opt_iterations, dev, [k for k in keys for _ in range(P)], _kick_offsets(r, P) * G,
                                                 heats, eis if sparse else None, kick_stats)
            if kopt[0] > 0:
                solved = _kopt_stage("grouped", kopt, np_points64, solved, dev, [k for k in keys for _ in range(P)],
                                     _kopt_offsets(r, P) * G, heats, eis if sparse else None, kopt_stats)
            tick("two_opt", t0)
            for g in range(G):
                stacked[g].append(solved[g * P:(g + 1) * P])
                merged_costs[g] += [tour_length(np_points64[g], t) for t in tours[g]]
        for g in range(G):
            sol = np.concatenate(stacked[g], axis=0)
            costs = [tour_length(np_points64[g], t) for t in sol]
            best = int(np.argmin(costs))
            info = {"merge_iterations": merge_its[g], "two_opt_iterations": int(ns[g]), "merged_costs": merged_costs[g]}
            info.update(_local_search_info(search, ls_stats, kick_stats, g * P, P, g))
            info.update(_kopt_info(kopt, kopt_stats, g * P, P))
            results.append((sol[best].tolist(), costs[best], costs, info))
        if heatmaps is not None:
            heatmaps.extend(heat_out)
    return results


def _solve_tsp_list(model, points, sparse_factor, P, sequential_sampling, two_opt_iterations, seeds, generators, timings,
                    instances_per_call, step_offset, heatmaps, merge_method, search, kopt=(0, 0, 0)) -> List[tuple]:
    """``solve_tsp_batch`` for a sequence of instances [n_b, 2] of any sizes; ``search``: its checked local-search settings, as
    ``_local_search`` takes them; ``kopt``: the checked (rounds, samples, depth) of the k-opt stage.  Every argument is checked
    before any library call."""
    pts_list = [np.ascontiguousarray(p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p, dtype=np.float64)
                for p in points]
    B = len(pts_list)
    if B < 1:
        raise ValueError("points must hold at least one instance")
    sparse = sparse_factor is not None and sparse_factor > 0
    for b, p in enumerate(pts_list):
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"points[{b}] must be [n, 2], got {list(p.shape)}")
        if p.shape[0] < 4:
            raise ValueError(f"points[{b}] has {p.shape[0]} nodes, a tour needs at least 4")
        if sparse and p.shape[0] < sparse_factor:
            raise ValueError(f"points[{b}] has {p.shape[0]} nodes, fewer than sparse_factor = {sparse_factor}")
    seeds, generators = _per_instance(seeds, B, "seeds"), _per_instance(generators, B, "generators")
    dev = model.device
    tick = _ticker(timings, dev)
    results = []
    for c0, c1 in _chunks(B, instances_per_call):
        G = c1 - c0
        ns = [p.shape[0] for p in pts_list[c0:c1]]
        t0 = time.perf_counter()
        if sparse:
            ei_all = knn_edge_index_gpu(np.concatenate(pts_list[c0:c1]), sparse_factor, device=dev, sizes=ns)
            e_off = np.concatenate([[0], np.cumsum([n * sparse_factor for n in ns])])
            n_off = np.concatenate([[0], np.cumsum(ns)])
            eis = [ei_all[:, e_off[g]:e_off[g + 1]] - int(n_off[g]) for g in range(G)]
        tick("knn", t0)
        pts32 = [torch.from_numpy(p.astype(np.float32)).to(dev) for p in pts_list[c0:c1]]     # as solve_tsp
        np_points64 = [p.cpu().numpy().astype(np.float64) for p in pts32]
        if sparse:
            pts_rep = [pts32[g].repeat(P, 1) for g in range(G)]
            ei_rep = [model.duplicate_edge_index(eis[g], ns[g], dev, copies=P) if P > 1 else eis[g] for g in range(G)]
        else:
            pts_rep, ei_rep = [pts32[g].reshape(1, ns[g], 2).repeat(P, 1, 1) for g in range(G)], None
        seeds_c = None if seeds is None else seeds[c0:c1]
        gens_c = None if generators is None else generators[c0:c1]
        stacked = [[] for _ in range(G)]
        merged_costs = [[] for _ in range(G)]
        heat_out = [[] for _ in range(G)]
        merge_its = [0.0] * G
        its = np.zeros(G, dtype=np.int64)
        ls_stats, kick_stats, kopt_stats = {}, {}, {}
        keys = [_kick_key(v) for v in ([model.seed] * G if seeds is None else seeds_c)]
        for r in range(sequential_sampling):
            t0 = time.perf_counter()
            heats = model.sample_batch(pts_rep, ei_rep, seeds=seeds_c, generators=gens_c,
                                       step_offset=_round_offset(model, step_offset, r))
            if heatmaps is not None:
                for g in range(G):
                    heat_out[g].append(heats[g].cpu().numpy())
            tick("sampling", t0)
            t0 = time.perf_counter()
            tours = []
            if merge_method == "batched":
                for g, (tg, it) in enumerate(merge_tours_batch(heats, pts32, eis if sparse else None, sparse_graph=sparse,
                                                               parallel_sampling=P, device=dev)):
                    merge_its[g] = it
                    tours.append(tg)
            else:
                for g in range(G):
                    tg, merge_its[g] = merge_tours(heats[g], pts32[g], eis[g] if sparse else None, sparse_graph=sparse,
                                                   parallel_sampling=P, device=dev)
                    tours.append(tg)
            tick("merge", t0)
            t0 = time.perf_counter()
            solved, its, ls_stats = _local_search("ragged", search, np_points64, [np.asarray(t, dtype=np.int64) for t in tours],
                                                  two_opt_iterations, dev, [k for k in keys for _ in range(P)], _kick_offsets(r, P) * G,
                                                  heats, eis if sparse else None, kick_stats)
            if kopt[0] > 0:
                solved = _kopt_stage("ragged", kopt, np_points64, solved, dev, [k for k in keys for _ in range(P)],
                                     _kopt_offsets(r, P) * G, heats, eis if sparse else None, kopt_stats)
            tick("two_opt", t0)
            for g in range(G):
                stacked[g].append(solved[g])
                merged_costs[g] += [tour_length(np_points64[g], t) for t in tours[g]]
        for g in range(G):
            sol = np.concatenate(stacked[g], axis=0)
            costs = [tour_length(np_points64[g], t) for t in sol]
            best = int(np.argmin(costs))
            info = {"merge_iterations": merge_its[g], "two_opt_iterations": int(its[g]), "merged_costs": merged_costs[g]}
            info.update(_local_search_info(search, ls_stats, kick_stats, g * P, P, g))
            info.update(_kopt_info(kopt, kopt_stats, g * P, P))
            results.append((sol[best].tolist(), costs[best], costs, info))
        if heatmaps is not None:
            heatmaps.extend(heat_out)
    return results


def solve_mis_batch(model, instances, parallel_sampling: int = 1, sequential_sampling: int = 1,
                    seeds: Optional[Sequence[int]] = None, generators: Optional[Sequence[torch.Generator]] = None,
                    timings: Optional[Dict[str, float]] = None, instances_per_call: Optional[int] = None,
                    step_offset: Optional[int] = None, *, local_search: str = "none", local_search_rounds: int = 1000,
                    stats: Optional[list] = None, local_search_kicks: int = 0, local_search_kick_size: int = 4,
                    local_search_mode: str = "launches") -> List[tuple]:
    """``solve_mis`` of B graphs: ``instances`` = [(n_nodes, edge_index), ...].  Returns the list of what ``solve_mis`` returns
    for every graph (run with ``seed = seeds[b]``, ``generator = generators[b]``).  Up to ``instances_per_call`` graphs share
    one sampling loop over their union (``MISModel.sample_batch``) and one greedy decode of the union (``mis_decode_np``: the
    decode never crosses a component, so every graph gets its own decode).  ``step_offset``: as in ``solve_tsp_batch``.
    ``local_search``, ``local_search_rounds``: as ``solve_mis``; one ``decode.mis_local_search_np`` call per decode on the
    union of the chunk (the search never crosses a component and round r of the union is round r of every graph, so every graph
    gets its solo answer).  ``stats``: a list to which one dict per instance is appended (only with "swap"): ``decoded_sizes``
    of the instance, and the counters ``rounds``, ``swaps``, ``inserts`` of its CHUNK's calls summed over the sequential rounds.
    ``local_search_kicks``, ``local_search_kick_size``: as ``solve_mis``; every one of the P copies of an instance is its own
    row of the call's instance table, keyed by the instance's sampling seed (``seeds[b]`` as ``sample_batch`` resolves it) at
    offset ``2^62 + (r P + p) 2^32``, so the records do not depend on the chunking; the per-instance dicts then also hold
    ``swap_sizes``, ``kicks_entered`` and ``kicks_accepted``.  ``local_search_mode``: as ``solve_mis``."""
    from .decode import (check_mis_kicks, check_mis_local_search, check_mis_search_mode, mis_decode_np, mis_iterated_search_np,
                         mis_local_search_np)
    from .graph import build_csr
    check_mis_local_search(local_search)
    kicks, kick_size = check_mis_kicks(local_search, local_search_kicks, local_search_kick_size)
    mode = check_mis_search_mode(local_search, local_search_mode)
    instances = list(instances)
    B = len(instances)
    if B < 1:
        raise ValueError("solve_mis_batch needs at least one instance")
    seeds, generators = _per_instance(seeds, B, "seeds"), _per_instance(generators, B, "generators")
    dev = model.device
    P = int(parallel_sampling)
    tick = _ticker(timings, dev)
    results = []
    for c0, c1 in _chunks(B, instances_per_call):
        ns = [int(instances[b][0]) for b in range(c0, c1)]
        eis = []
        for b in range(c0, c1):
            ei = instances[b][1]
            ei = (ei if isinstance(ei, torch.Tensor) else torch.from_numpy(np.asarray(ei))).to(dev)
            eis.append(model.duplicate_edge_index(ei, ns[b - c0], dev, copies=P) if P > 1 else ei)
        off = np.concatenate([[0], np.cumsum([n * P for n in ns])])
        union = torch.cat([e + int(off[g]) for g, e in enumerate(eis)], dim=1)
        graph = build_csr(union, int(off[-1]), dev, method=getattr(model, "graph_build", "host"))
        sols = [[] for _ in ns]
        decoded = [[] for _ in ns]
        counters = {"rounds": 0, "swaps": 0, "inserts": 0}
        kick_stats = [{"swap_sizes": [], "kicks_entered": [], "kicks_accepted": []} for _ in ns]
        # the Philox keys of the chunk's instances, resolved the way sample_batch resolves them
        keys = [int(v) & (2 ** 63 - 1) for v in ([model.seed] * len(ns) if seeds is None else seeds[c0:c1])]
        for r in range(sequential_sampling):
            t0 = time.perf_counter()
            scores = model.sample_batch([n * P for n in ns], eis, seeds=None if seeds is None else seeds[c0:c1],
                                        generators=None if generators is None else generators[c0:c1],
                                        step_offset=_round_offset(model, step_offset, r))
            tick("sampling", t0)
            t0 = time.perf_counter()
            sol = mis_decode_np(torch.cat(scores), graph=graph, device=dev)
            if local_search == "swap":
                tick("decode", t0)
                t0 = time.perf_counter()
                for g, n in enumerate(ns):
                    decoded[g] += sol[off[g]:off[g + 1]].reshape(P, n).sum(axis=1).tolist()
                call = {}
                if kicks > 0 or mode == "resident":
                    sol = mis_iterated_search_np(
                        torch.cat(scores), sol, graph=graph, device=dev, max_rounds=local_search_rounds, stats=call, kicks=kicks,
                        kick_size=kick_size, instance_rows=[int(off[g]) + n * p for g, n in enumerate(ns) for p in range(P)] + [int(off[-1])],
                        seeds=[k for k in keys for _ in range(P)], offsets=_kick_offsets(r, P) * len(ns), mode=mode)
                    for g in range(len(ns)):
                        _kick_stats(kick_stats[g], call, g * P, P)
                else:
                    sol = mis_local_search_np(torch.cat(scores), sol, graph=graph, device=dev, max_rounds=local_search_rounds,
                                              stats=call)
                for k in counters:
                    counters[k] += call[k]
            for g, n in enumerate(ns):
                sols[g].append(sol[off[g]:off[g + 1]].reshape(P, n))
            tick("local_search" if local_search == "swap" else "decode", t0)
        for g in range(len(ns)):
            sol = np.concatenate(sols[g], axis=0)
            sizes = sol.sum(axis=1)
            best = int(np.argmax(sizes))
            results.append((sol[best], int(sizes[best]), sizes.tolist()))
            if local_search == "swap" and stats is not None:
                stats.append(dict(decoded_sizes=decoded[g], **counters, **(kick_stats[g] if kicks > 0 else {})))
    return results
