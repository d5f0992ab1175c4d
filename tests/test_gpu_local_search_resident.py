"""The resident 2-opt + Or-opt search on the GPU (``mode="resident"``: ``difusco_tsp_local_search_resident``, one block per group,
tours in LDS through both phases and all rounds): the tours and the three counters of ``or_opt_emulation.local_search`` bit for
bit; the caps, ties and degenerate geometry, per-instance semantics, the state across launches and ``host_syncs``, the limit,
non-finite input, the wrappers, the solvers and the runner.

Sizes.  The kernel has no tile.  Its 2-opt sweep splits the pairs of a tour over a team of whole waves; its Or-opt sweep gives a
wave blocks of 64 columns and chunks of rows, filled 64 rows at a time: n = 63, 64, 65 lie around one column block and one fill,
200 takes four column blocks and several fills per chunk when P = 3 leaves a team few waves, n = 4 has no L = 3 candidate and
n = 5 one row of them, P = 20 at n = 8 is more tours than waves."""
import functools

import numpy as np
import pytest
import torch

import or_opt_emulation as E
from test_gpu_evaluate import _argv, _ckpt, _model_args, _write_tsp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def group(n, P, s=0):
    """P start tours over the points of ``instance(n, s)``: the tours of ``instance(n, s), instance(n, s + 1), ...``."""
    return E.instance(n, s)[0], np.stack([E.instance(n, s + p)[1] for p in range(P)])


@functools.lru_cache(maxsize=None)
def emulated(n, P, cap=1000, rounds=16, s=0):
    return E.local_search(*group(n, P, s), max_iterations=cap, max_rounds=rounds)


def resident(dev, groups, cap=1000, rounds=16, mode="resident", **kw):
    """(tours, two_opt_iterations, or_opt_iterations, rounds, host_syncs) of one call on the groups."""
    from difusco_amd.decode import batched_local_search_ragged
    stats = {}
    tours, two = batched_local_search_ragged([p for p, _ in groups], [t for _, t in groups], max_iterations=cap, device=dev,
                                             max_rounds=rounds, stats=stats, **(dict(mode=mode, **kw) if mode == "resident" else {}))
    return (tours, [int(v) for v in two], [int(v) for v in stats["or_opt_iterations"]], [int(v) for v in stats["rounds"]],
            stats.get("host_syncs"))


def launched(dev, groups, cap=1000, rounds=16):
    return resident(dev, groups, cap, rounds, mode="launches")


def same_tours(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def launches_of(two, orr, per_launch=1024):
    """A launch ends when it would apply one step more than ``per_launch``: the slowest group decides, one launch at least."""
    steps = max(a + b for a, b in zip(two, orr))
    return max(1, -(-steps // per_launch))


def equals_emulation(got, want_list):
    tours, two, orr, rounds, syncs = got
    assert two == [w[1] for w in want_list] and orr == [w[2] for w in want_list] and rounds == [w[3] for w in want_list]
    assert same_tours(tours, [w[0] for w in want_list])
    assert syncs == launches_of(two, orr)


# ---- 1. sizes and group shapes against the emulation -------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("n", [4, 5, 6, 8, 33, 63, 64, 65, 200])
def test_sizes_and_group_shapes_equal_the_emulation(dev, n, P):
    want = emulated(n, P)
    equals_emulation(resident(dev, [group(n, P)]), [want])
    assert want[1] > 0 or n <= 5                                 # a random tour moves
    assert want[2] > 0 or n <= 33                                # and from 63 cities on the Or-opt phase finds work after 2-opt


def test_more_tours_than_waves(dev):
    want = emulated(8, 20)
    assert want[1] > 0
    equals_emulation(resident(dev, [group(8, 20)]), [want])


# ---- 2. the caps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,rounds", [(5, 16), (1000, 1), (0, 16), (1, 2)])
def test_the_caps_equal_the_emulation(dev, cap, rounds):
    shapes = [(8, 2), (33, 3), (64, 1)]
    want = [emulated(n, P, cap, rounds) for n, P in shapes]
    equals_emulation(resident(dev, [group(n, P) for n, P in shapes], cap, rounds), want)
    if cap == 0:                                                 # one evaluated 2-opt move, no Or-opt phase, one round
        assert [w[1:] for w in want[1:]] == [(1, 0, 1)] * 2
    if (cap, rounds) == (1, 2):
        assert want[1][1:] == (2, 2, 2)
    if (cap, rounds) == (5, 16):
        assert want[1][3] > 2 and want[1][1] > 5                 # several rounds, each phase capped on its own


# ---- 3. ties and degenerate geometry -------------------------------------------------------------------------------------------
def degenerate_groups():
    lattice = np.stack(np.meshgrid(np.arange(6), np.arange(6), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
    dup = E.instance(15, 3)[0]
    pts30, tours30 = group(30, 2, 5)
    return [(lattice, group(36, 3, 1)[1]),                                       # exact ties: the first flat index wins
            (np.full((8, 2), 0.375), group(8, 2, 2)[1]),                         # all cities coincident
            (np.concatenate([dup, dup]), tours30),                               # pairs of duplicate cities
            (pts30 * 2.0 ** -20, tours30),                                       # few changes reach 1e-6
            (pts30 + 1e6, tours30)]                                              # the coordinates lose 20 bits


def test_ties_and_degenerate_geometry_equal_the_emulation(dev):
    groups = degenerate_groups()
    want = [E.local_search(p, t) for p, t in groups]
    assert want[0][1] > 0 and want[0][2] > 0 and want[2][1] > 0 and want[4][1] > 0
    assert want[1][1:] == (0, 0, 1) and np.array_equal(want[1][0], groups[1][1])
    equals_emulation(resident(dev, groups), want)
    for g, grp in enumerate(groups):                             # and every group alone
        equals_emulation(resident(dev, [grp]), [want[g]])


# ---- 4. independence -------------------------------------------------------------------------------------------------------------
def test_a_group_gets_its_own_answer_in_any_call(dev):
    shapes = [(4, 3), (5, 2), (9, 1), (17, 4), (33, 2), (64, 1), (65, 5), (100, 2), (130, 7), (12, 40), (50, 20)]
    groups = [group(n, P, 9) for n, P in shapes]
    cap, rounds = 30, 3
    tours, two, orr, rnd, syncs = resident(dev, groups, cap, rounds)
    assert sum(two) > 0 and sum(orr) > 0
    again = resident(dev, groups, cap, rounds)
    assert again[1:] == (two, orr, rnd, syncs) and same_tours(again[0], tours)
    back = resident(dev, groups[::-1], cap, rounds)
    assert back[1:] == (two[::-1], orr[::-1], rnd[::-1], syncs) and same_tours(back[0], tours[::-1])
    for g, grp in enumerate(groups):
        t, a, b, r, _ = resident(dev, [grp], cap, rounds)
        assert (a, b, r) == ([two[g]], [orr[g]], [rnd[g]]) and np.array_equal(t[0], tours[g]), g
    ref = launched(dev, groups, cap, rounds)
    assert ref[1:4] == (two, orr, rnd) and same_tours(ref[0], tours)


def test_six_hundred_groups_equal_their_solo_calls(dev):
    groups = [group(12, 1, g) for g in range(600)]
    tours, two, orr, rnd, syncs = resident(dev, groups)
    assert sum(two) > 600 and sum(orr) > 0 and syncs == 1
    for g, grp in enumerate(groups):
        t, a, b, r, _ = resident(dev, [grp])
        assert (a, b, r) == ([two[g]], [orr[g]], [rnd[g]]) and np.array_equal(t[0], tours[g]), g
    for g in range(0, 600, 50):
        want = emulated(12, 1, s=g)
        assert (two[g], orr[g], rnd[g]) == want[1:] and np.array_equal(tours[g], want[0])


def test_a_finished_group_next_to_a_working_one(dev):
    done = emulated(33, 3)
    finished = (group(33, 3)[0], done[0])
    again = E.local_search(*finished)
    assert again[1:] == (0, 0, 1) and np.array_equal(again[0], done[0])
    groups = [finished, group(64, 1), finished]
    equals_emulation(resident(dev, groups), [again, emulated(64, 1), again])
    got = resident(dev, groups, steps_per_launch=3)              # the finished groups stop in the first launch, the other goes on
    assert got[4] == launches_of(*got[1:3], 3) > 1 and same_tours(got[0], [again[0], emulated(64, 1)[0], again[0]])


# ---- 5. the state across launches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,rounds", [(1000, 16), (4, 3)])
def test_the_state_survives_launches_and_every_launch_costs_one_synchronisation(dev, cap, rounds):
    groups = [group(33, 3), group(8, 2), group(50, 1)]
    want = [emulated(n, P, cap, rounds) for n, P in ((33, 3), (8, 2), (50, 1))]
    tours, two, orr, rnd, syncs = resident(dev, groups, cap, rounds)
    equals_emulation((tours, two, orr, rnd, syncs), want)
    assert max(a + b for a, b in zip(two, orr)) > 7
    for per_launch in (1, 7):
        got = resident(dev, groups, cap, rounds, steps_per_launch=per_launch)
        assert got[1:4] == (two, orr, rnd) and same_tours(got[0], tours), per_launch
        assert got[4] == launches_of(two, orr, per_launch) > 1, per_launch


def test_the_default_costs_one_synchronisation_per_1024_steps(dev):
    want = emulated(50, 1)
    tours, two, orr, rnd, syncs = resident(dev, [group(50, 1)])
    equals_emulation((tours, two, orr, rnd, syncs), [want])
    steps = two[0] + orr[0]
    assert steps > 30 and syncs == max(1, -(-steps // 1024))
    assert syncs == 1 or steps > 1024


# ---- 6. the limit ----------------------------------------------------------------------------------------------------------------
def test_the_largest_group_runs_and_one_city_more_is_refused(dev):
    from difusco_amd import _lib
    from difusco_amd.decode import batched_local_search_torch, local_search_resident_max_cells
    m = local_search_resident_max_cells()
    n = m - 1
    pts, tour = E.instance(n + 1, 7)
    inside = pts[:n], np.concatenate([[0], 1 + np.random.default_rng(7).permutation(n - 1), [0]])[None]
    ref = launched(dev, [inside], 3, 2)
    assert ref[1:4] == ([6], [6], [2])
    got = resident(dev, [inside], 3, 2)
    assert got[1:4] == ref[1:4] and same_tours(got[0], ref[0]) and got[4] == 1
    with pytest.raises(_lib.DifuscoHipError) as e:
        batched_local_search_torch(pts, tour[None], max_iterations=3, device=dev, max_rounds=2, mode="resident")
    assert "group 0 " in str(e.value) and f"{m + 1} cells" in str(e.value) and f"limit of {m} cells" in str(e.value)
    with pytest.raises(_lib.DifuscoHipError, match="group 1 "):
        resident(dev, [group(9, 2), (pts, tour[None])], 3, 2)


# ---- 7. non-finite input -----------------------------------------------------------------------------------------------------------
def test_an_infinite_coordinate_beside_a_normal_group(dev):
    pts, tours = group(40, 2, 6)
    pts = pts.copy()
    pts[7, 0] = np.inf
    normal = group(33, 1)
    for cap, rounds in ((5, 2), (60, 16)):
        got = resident(dev, [(pts, tours), normal], cap, rounds)                 # the call returns
        for t in got[0][0]:
            assert t[0] == t[-1] and sorted(t[:-1]) == list(range(40))
        solo = resident(dev, [normal], cap, rounds)
        assert (got[1][1], got[2][1], got[3][1]) == (solo[1][0], solo[2][0], solo[3][0]) and np.array_equal(got[0][1], solo[0][0])
        ref = launched(dev, [(pts, tours), normal], cap, rounds)
        assert got[1:4] == ref[1:4] and same_tours(got[0], ref[0]), (cap, rounds)


# ---- 8. wrappers, solvers, runner --------------------------------------------------------------------------------------------------
def test_the_three_wrappers_equal_their_launched_mode(dev):
    from difusco_amd.decode import batched_local_search_grouped, batched_local_search_ragged, batched_local_search_torch
    G, n, P = 3, 40, 2
    pts = np.stack([group(n, P, 20 + g)[0] for g in range(G)])
    tours = np.concatenate([group(n, P, 20 + g)[1] for g in range(G)])
    ragged = [group(17, 2), group(64, 1), group(33, 3)]
    for per_launch in (0, 5):
        kw = dict(max_iterations=50, device=dev, max_rounds=4)
        res = dict(mode="resident", steps_per_launch=per_launch)
        plain, stats = {}, {}
        a, ia = batched_local_search_torch(pts[0], tours[:P], stats=plain, **kw)
        b, ib = batched_local_search_torch(pts[0], tours[:P], stats=stats, **kw, **res)
        assert isinstance(ib, int) and ib == ia > 0 and np.array_equal(a, b) and b.dtype == np.int64
        assert set(stats) == set(plain) | {"host_syncs"} == {"or_opt_iterations", "rounds", "host_syncs"}
        assert {k: stats[k] for k in plain} == plain and isinstance(stats["host_syncs"], int)
        want = E.local_search(pts[0], tours[:P], 50, 4)
        assert np.array_equal(b, want[0]) and (ib, stats["or_opt_iterations"], stats["rounds"]) == want[1:]
        a, ia = batched_local_search_grouped(pts, tours, stats=plain, **kw)
        b, ib = batched_local_search_grouped(pts, tours, stats=stats, **kw, **res)
        assert np.array_equal(ia, ib) and ib.dtype == np.int64 and np.array_equal(a, b) and b.shape == tours.shape
        assert all(np.array_equal(stats[k], plain[k]) and stats[k].dtype == plain[k].dtype for k in plain)
        a, ia = batched_local_search_ragged([p for p, _ in ragged], [t for _, t in ragged], stats=plain, **kw)
        b, ib = batched_local_search_ragged([p for p, _ in ragged], [t for _, t in ragged], stats=stats, **kw, **res)
        assert np.array_equal(ia, ib) and same_tours(a, b) and all(np.array_equal(stats[k], plain[k]) for k in plain)


def test_the_solvers_return_the_launched_results(dev):
    from difusco_amd import TSPModel
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    from difusco_amd.synthetic import random_state_dict
    sd = random_state_dict(64, 2, 2, seed=0)
    B, n, P = 3, 50, 2
    rng = np.random.default_rng(12)
    pts = rng.random((B, n, 2))
    mixed = [rng.random((k, 2)) for k in (20, 33, 47, 60)]
    seeds = [21, 22, 23, 24]
    model = lambda seed: TSPModel(_model_args(sparse_factor=-1, hidden_dim=64, n_layers=2), sd, device=dev, seed=seed)
    gens = lambda k: [torch.Generator().manual_seed(b) for b in range(k)]
    kw = dict(parallel_sampling=P, two_opt_iterations=100, local_search="2opt+oropt")
    res = dict(local_search_mode="resident")
    base = solve_tsp(model(5), pts[0], -1, generator=torch.Generator().manual_seed(0), **kw)
    assert base == solve_tsp(model(5), pts[0], -1, generator=torch.Generator().manual_seed(0), **kw, **res)
    assert base == solve_tsp(model(5), pts[0], -1, generator=torch.Generator().manual_seed(0), **kw, local_search_mode="launches")
    assert base[3]["two_opt_iterations"] > 0 and base[3]["local_search_rounds"] >= 1 and "or_opt_iterations" in base[3]
    base = solve_tsp_batch(model(0), pts, -1, seeds=seeds[:B], generators=gens(B), **kw)
    assert base == solve_tsp_batch(model(0), pts, -1, seeds=seeds[:B], generators=gens(B), **kw, **res)
    base = solve_tsp_batch(model(0), mixed, -1, seeds=seeds, generators=gens(4), **kw)
    assert base == solve_tsp_batch(model(0), mixed, -1, seeds=seeds, generators=gens(4), **kw, **res)
    assert [len(r[0]) - 1 for r in base] == [20, 33, 47, 60] and sum(r[3]["or_opt_iterations"] for r in base) > 0


def test_evaluate_gives_the_launched_records_plus_one_key(dev, tmp_path):
    from difusco_amd import evaluate as EV
    split = _write_tsp(tmp_path / "tsp.txt", [50] * 4, seed=1)
    ckpt, _ = _ckpt(tmp_path / "last.ckpt", 64, 2)
    argv = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--two_opt_iterations", "100", "--do_valid_only", "--validation_examples", "4",
                 "--parallel_sampling", "2", "--local_search", "2opt+oropt")
    plain_lines, plain = EV.run(argv)
    lines, recs = EV.run(argv + ["--tsp_local_search_mode", "resident"])
    assert len(recs) == len(plain) == 4 and sum(r["2opt_iterations"] for r in plain) > 0
    assert "tsp_local_search_mode" not in plain_lines[0] and lines[0]["tsp_local_search_mode"] == "resident"
    assert {k: v for k, v in lines[0].items() if k != "tsp_local_search_mode"}.keys() == plain_lines[0].keys()
    for r, p in zip(recs, plain):
        assert "tsp_local_search_mode" not in p and r["tsp_local_search_mode"] == "resident"
        assert {k: v for k, v in r.items() if k != "tsp_local_search_mode"} == p
    again_lines, again = EV.run(argv + ["--tsp_local_search_mode", "launches"])
    assert plain == again and list(again_lines[0]) == list(plain_lines[0])
