"""The resident 2-opt on the GPU (``mode="resident"``: ``difusco_tsp_two_opt_resident``, one block per group, tours in LDS): the
tours and iteration counts of ``oracle.tsp_decode_oracle.batched_two_opt`` and of the launched ``batched_two_opt_ragged`` bit for
bit, with both methods; the stop rule, ties, groups without a screen bound, per-instance semantics, the limit, the state across
launches, ``exact_pairs`` and ``host_syncs``, the refusals, the wrappers, the solvers and the runner.

Sizes.  The kernel has no tile: a block is 256 .. 1024 threads in whole waves (a quarter of the largest group's pairs), its waves
form teams of 64 k threads (block waves / P), and a thread of a team takes every (team size)-th pair of the row-major triangle
j >= i + 2, skipping the rows shorter than its step.  The widths are therefore the team sizes: beside the sizes every case takes
(4, 5, 17, 63, 64, 65, 257) the list has 193 (a row one pair longer than the 192-thread teams of P = 5), 513 and 1025 (rows around
half of and all of a 1024-thread team; with P = 2, twice a 512-thread team)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import tsp_decode_oracle as D
from test_gpu_evaluate import _argv, _ckpt, _model_args, _write_tsp

pytestmark = pytest.mark.gpu

METHODS = ("exact", "screened")
BIG_CAP = 25                                  # what the cap 1000 becomes from n = 193 on (the oracle's cost on the CPU)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def grid_points(rng, n):
    return rng.integers(0, 65536, size=(n, 2)).astype(np.float64) / 65536.0


def random_tours(rng, n, P):
    return np.stack([np.concatenate([[0], 1 + rng.permutation(n - 1), [0]]) for _ in range(P)])


@functools.lru_cache(maxsize=None)
def random_group(n, P, seed=0):
    rng = np.random.default_rng(1000 * n + 10 * P + seed)
    return grid_points(rng, n), random_tours(rng, n, P)


@functools.lru_cache(maxsize=None)
def oracle_of(n, P, cap, seed=0):
    pts, tours = random_group(n, P, seed)
    return D.batched_two_opt(pts, tours, max_iterations=cap)


def evaluations(iterations, cap):
    """Sweeps that did work: one more than the moves unless the cap ended the run (tests/two_opt_entries_cases.py)."""
    return iterations + 1 if iterations < max(cap, 1) else iterations


def exact_formula(groups, its, cap):
    """``exact_pairs_of_exact_run`` of tests/two_opt_entries_cases.py for groups of any (n, P)."""
    return sum(evaluations(int(it), cap) * t.shape[0] * ((len(p) - 1) * (len(p) - 2) // 2) for (p, t), it in zip(groups, its))


def resident(dev, groups, cap, method, **kw):
    from difusco_amd.decode import batched_two_opt_ragged
    stats = {}
    tours, its = batched_two_opt_ragged([p for p, _ in groups], [t for _, t in groups], max_iterations=cap, device=dev, method=method,
                                        mode="resident", stats=stats, **kw)
    return tours, [int(v) for v in its], stats


def launched(dev, groups, cap, method="exact"):
    from difusco_amd.decode import batched_two_opt_ragged
    stats = {}
    tours, its = batched_two_opt_ragged([p for p, _ in groups], [t for _, t in groups], max_iterations=cap, device=dev, method=method,
                                        stats=stats)
    return tours, [int(v) for v in its], stats


def same_tours(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. sizes and group shapes against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("n", [4, 5, 17, 63, 64, 65, 193, 257])
def test_sizes_and_group_shapes_equal_the_oracle(dev, n, P):
    group = random_group(n, P)
    moved = 0
    for cap in (0, 1, 3, 1000):
        cap = BIG_CAP if cap == 1000 and n >= 193 else cap
        ref, ref_it = oracle_of(n, P, cap)
        for method in METHODS:
            tours, its, stats = resident(dev, [group], cap, method)
            assert its == [ref_it] and np.array_equal(tours[0], ref), (cap, method)
            assert stats["host_syncs"] == 1
        moved += ref_it
    assert moved > 0 or n == 4                # a random tour moves; of the three tours of 4 cities two are optimal


@pytest.mark.parametrize("n,P", [(513, 1), (1025, 1), (1025, 2)])
def test_the_widths_above_a_team_equal_the_oracle(dev, n, P):
    group = random_group(n, P)
    ref, ref_it = oracle_of(n, P, 3)
    assert ref_it == 3
    for method in METHODS:
        tours, its, _ = resident(dev, [group], 3, method)
        assert its == [3] and np.array_equal(tours[0], ref), method


# ---- 2. the stop rule ---------------------------------------------------------------------------------------------------------
def polygon(n, P):
    a = 2 * np.pi * np.arange(n) / n
    pts = np.round((0.5 + 0.4 * np.stack([np.cos(a), np.sin(a)], axis=1)) * 65536) / 65536
    return pts, np.tile(np.concatenate([np.arange(n), [0]]), (P, 1))


def optimal_beside_random():
    """Two tours over one point set.  Tour 0 visits a convex polygon in order, one of whose corners is a cluster of 12 cities
    within 2^-28 of each other, taken in a random order: no move of it reaches -1e-6, but its best one is negative.  Tour 1 is
    random."""
    rng = np.random.default_rng(5)
    poly = polygon(12, 1)[0]
    cluster = poly[-1] + rng.integers(-64, 65, size=(12, 2)) * 2.0 ** -34
    pts = np.concatenate([poly[:-1], cluster])
    n = len(pts)
    return pts, np.stack([np.concatenate([np.arange(11), 11 + rng.permutation(12), [0]]), np.concatenate([[0], 1 + rng.permutation(n - 1), [0]])])


def test_a_finished_group_stops_alone_and_an_optimal_tour_still_applies_its_best_move(dev):
    poly = polygon(24, 2)
    assert D.batched_two_opt(*poly)[1] == 0
    pair = optimal_beside_random()
    assert D.batched_two_opt(pair[0], pair[1][:1])[1] == 0       # alone, tour 0 is finished
    groups = [random_group(33, 2), poly, pair, random_group(17, 1)]
    for cap in (2, 1000):
        want = [D.batched_two_opt(p, t, max_iterations=cap) for p, t in groups]
        assert want[1][1] == 0 and want[0][1] > 0 and want[2][1] > 0
        for method in METHODS:
            tours, its, _ = resident(dev, groups, cap, method)
            assert its == [it for _, it in want] and same_tours(tours, [t for t, _ in want]), (cap, method)
    # while its group runs, tour 0 applies its own best move, which does not improve it by 1e-6: after one move it differs
    after_one, _ = D.batched_two_opt(*pair, max_iterations=1)
    assert not np.array_equal(after_one[0], pair[1][0])
    for method in METHODS:
        tours, its, _ = resident(dev, [pair], 1, method)
        assert its == [1] and np.array_equal(tours[0], after_one)


# ---- 3. ties and degenerate geometry -------------------------------------------------------------------------------------------
def test_ties_on_integer_grids_coincident_and_duplicate_cities(dev):
    rng = np.random.default_rng(3)
    groups = []
    for side in (4, 6):                                          # exact ties: the first flat index wins
        xy = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
        groups.append((xy, random_tours(rng, side * side, 3)))
    groups.append((np.full((8, 2), 0.375), random_tours(rng, 8, 2)))                      # all cities coincident
    dup = grid_points(rng, 15)
    groups.append((np.concatenate([dup, dup]), random_tours(rng, 30, 2)))                 # pairs of duplicate cities
    want = [D.batched_two_opt(p, t) for p, t in groups]
    assert want[2][1] == 0 and np.array_equal(want[2][0], groups[2][1]) and want[0][1] > 0 and want[3][1] > 0
    for method in METHODS:
        tours, its, _ = resident(dev, groups, 1000, method)
        assert its == [it for _, it in want] and same_tours(tours, [t for t, _ in want]), method
        for g, grp in enumerate(groups):                         # and every group alone
            t, it, _ = resident(dev, [grp], 1000, method)
            assert it == [want[g][1]] and np.array_equal(t[0], want[g][0]), (method, g)


def test_a_zero_change_reversal_of_a_finished_tour_is_not_a_move(dev):
    """tests/golden/two_opt_zero_change_reversal.npz: 4 decoded tours over 200 cities (float32 coordinates).  Tour 1 finishes
    three moves before its group; from then on its best move is the no-op at flat index 0, because the reversal of the whole tour,
    pair (0, n - 1), changes it by ((a + b) - b) - a = 0.0 exactly when the two products of a distance are added without a fused
    multiply-add.  With one it is -6.9e-18 and the tour comes back reversed.
    Provenance of the file (no reference code): group 56 of the n = 200, P = 4, G = 64 case of scripts/bench_two_opt_resident.py -
    ``points``: ``difusco_amd.synthetic.tsp_instance(200, 10, seed=4056)`` as float64 of their float32 values; ``tours``: what
    ``decode.merge_tours_batch`` decoded from that script's synthetic heatmap; ``tours_out`` / ``iterations``:
    ``oracle.tsp_decode_oracle.batched_two_opt`` on them (numpy), which this test recomputes."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "two_opt_zero_change_reversal.npz"))
    ref, ref_it = D.batched_two_opt(z["points"], z["tours"])
    assert ref_it == int(z["iterations"]) == 42 and np.array_equal(ref, z["tours_out"])
    for method in METHODS:
        tours, its, _ = resident(dev, [(z["points"], z["tours"].astype(np.int64))], 1000, method)
        assert its == [42] and np.array_equal(tours[0], ref), method


# ---- 4. no screen bound --------------------------------------------------------------------------------------------------------
def test_groups_without_a_bound_take_the_exact_sweep_for_themselves_only(dev):
    from difusco_amd.decode import two_opt_screen_bound
    big, small = random_group(30, 2, seed=1), random_group(21, 1, seed=2)
    scaled = [(big[0] * 2.0 ** 70, big[1]), (small[0] * 2.0 ** -40, small[1])]
    assert all(two_opt_screen_bound(np.abs(p).max()) is None for p, _ in scaled)
    plain = [random_group(64, 2, seed=3), random_group(100, 1, seed=4)]
    groups = [plain[0], scaled[0], plain[1], scaled[1]]
    cap = 1000
    want = [D.batched_two_opt(p, t, max_iterations=cap) for p, t in groups]
    assert want[0][1] > 0 and want[1][1] > 0 and want[2][1] > 0 and want[3][1] == 0      # at 2^-40 no change reaches -1e-6
    total = {}
    for method in METHODS:
        tours, its, stats = resident(dev, groups, cap, method)
        assert its == [it for _, it in want] and same_tours(tours, [t for t, _ in want]), method
        total[method] = stats["exact_pairs"]
    assert total["exact"] == exact_formula(groups, [it for _, it in want], cap)
    # the scaled groups' share is the formula, the others' is what they count alone, far below theirs
    _, its_s, st_s = resident(dev, scaled, cap, "screened")
    _, its_p, st_p = resident(dev, plain, cap, "screened")
    assert st_s["exact_pairs"] == exact_formula(scaled, its_s, cap)
    assert st_p["exact_pairs"] < exact_formula(plain, its_p, cap)
    assert total["screened"] == st_s["exact_pairs"] + st_p["exact_pairs"] < total["exact"]


def test_an_infinite_coordinate_equals_the_launched_entry(dev):
    pts, tours = random_group(40, 2, seed=6)
    pts = pts.copy()
    pts[7, 0] = np.inf
    groups = [random_group(33, 1), (pts, tours), random_group(20, 2)]
    for cap in (5, 60):
        ref, ref_its, _ = launched(dev, groups, cap)
        for method in METHODS:
            tours_r, its, stats = resident(dev, groups, cap, method)
            assert its == ref_its and same_tours(tours_r, ref), (cap, method)
        assert stats["exact_pairs"] < exact_formula(groups, its, cap)             # screened: the other groups keep their screen


# ---- 5. per-instance semantics ---------------------------------------------------------------------------------------------------
def test_a_group_gets_its_own_answer_in_any_call(dev):
    shapes = [(4, 3), (9, 1), (17, 4), (33, 2), (64, 1), (65, 5), (100, 2), (130, 7), (257, 1), (12, 40), (50, 20)]
    groups = [random_group(n, P, seed=9) for n, P in shapes]
    cap = 30
    for method in METHODS:
        tours, its, stats = resident(dev, groups, cap, method)
        assert sum(its) > 0
        again = resident(dev, groups, cap, method)
        assert again[1] == its and same_tours(again[0], tours) and again[2] == stats
        back = resident(dev, groups[::-1], cap, method)
        assert back[1] == its[::-1] and same_tours(back[0], tours[::-1]) and back[2]["exact_pairs"] == stats["exact_pairs"]
        for g, grp in enumerate(groups):
            t, it, _ = resident(dev, [grp], cap, method)
            assert it == [its[g]] and np.array_equal(t[0], tours[g]), (method, g)
    ref, ref_its, _ = launched(dev, groups, cap)
    assert ref_its == its and same_tours(ref, tours)


# ---- 6. more groups than CUs -----------------------------------------------------------------------------------------------------
def test_six_hundred_groups_equal_the_launched_entry(dev):
    rng = np.random.default_rng(6)
    groups = []
    for g in range(600):
        n = 8 + g % 5
        groups.append((grid_points(rng, n), random_tours(rng, n, 1 + g % 2)))
    ref, ref_its, _ = launched(dev, groups, 1000)
    assert sum(ref_its) > 600
    for method in METHODS:
        tours, its, stats = resident(dev, groups, 1000, method)
        assert its == ref_its and same_tours(tours, ref), method
        assert stats["host_syncs"] == 1


# ---- 7. the limit ------------------------------------------------------------------------------------------------------------------
def raw_call(dev, group_n, group_tours, pts, tours, cap, method=0, moves_per_launch=0, workspace_short=0, null=None, groups=None):
    """``difusco_tsp_two_opt_resident`` on device buffers: (return code, text, the tours buffer afterwards as numpy)."""
    from difusco_amd import _lib
    L = _lib.lib()
    gn, gt = np.ascontiguousarray(group_n, dtype=np.int32), np.ascontiguousarray(group_tours, dtype=np.int32)
    nbytes = ctypes.c_size_t()
    ok_n, ok_t = np.array([5], dtype=np.int32), np.array([1], dtype=np.int32)          # the size does not depend on the shapes
    assert L.difusco_tsp_two_opt_resident_workspace_bytes(max(len(gn), 1), np.resize(ok_n, max(len(gn), 1)).ctypes.data,
                                                          np.resize(ok_t, max(len(gn), 1)).ctypes.data, 0, ctypes.byref(nbytes)) == 0
    d_pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64).reshape(-1)).to(dev)
    d_tours = torch.from_numpy(np.ascontiguousarray(tours, dtype=np.int32).reshape(-1)).to(dev)
    ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
    its = np.zeros(max(len(gn), 1), dtype=np.int64)
    ptr = lambda name, t: None if null == name else ctypes.c_void_p(t.data_ptr())
    rc = L.difusco_tsp_two_opt_resident(len(gn) if groups is None else groups, None if null == "group_n" else gn.ctypes.data,
                                        None if null == "group_tours" else gt.ctypes.data, ptr("points", d_pts), ptr("tours", d_tours),
                                        cap, method, moves_per_launch, ptr("workspace", ws), nbytes.value - workspace_short,
                                        None if null == "iterations_out" else its.ctypes.data, None, None,
                                        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    return int(rc), L.difusco_last_error().decode(), d_tours.cpu().numpy()


def test_the_largest_group_runs_and_one_city_more_is_refused(dev):
    from difusco_amd import _lib
    from difusco_amd.decode import batched_two_opt_torch, two_opt_resident_max_cells
    m = two_opt_resident_max_cells()
    rng = np.random.default_rng(7)
    n = m - 1
    pts, tours = grid_points(rng, n + 1), random_tours(rng, n, 1)
    ref, ref_its, _ = launched(dev, [(pts[:n], tours)], 3)
    assert ref_its == [3]
    for method in METHODS:
        t, its, _ = resident(dev, [(pts[:n], tours)], 3, method)
        assert its == [3] and np.array_equal(t[0], ref[0]), method
    over = random_tours(rng, n + 1, 1)
    for method in (0, 1):
        rc, text, after = raw_call(dev, [n + 1], [1], pts, over, 3, method)
        assert rc == -4 and np.array_equal(after, over.reshape(-1))
        assert "group 0 " in text and f"{m + 1} cells" in text and f"limit of {m} cells" in text
    small = random_group(9, 2)
    both_pts, both_tours = np.concatenate([small[0], pts]), np.concatenate([small[1].reshape(-1), over.reshape(-1)])
    rc, text, after = raw_call(dev, [9, n + 1], [2, 1], both_pts, both_tours, 3)
    assert rc == -4 and np.array_equal(after, both_tours)          # refused whole: the small group did not run either
    assert "group 1 " in text and f"{m + 1} cells" in text and f"limit of {m} cells" in text
    with pytest.raises(_lib.DifuscoHipError, match="above the limit"):
        batched_two_opt_torch(pts, over, max_iterations=3, device=dev, mode="resident")
    with pytest.raises(_lib.DifuscoHipError, match="group 1 "):
        resident(dev, [small, (pts, over)], 3, "screened")


# ---- 8. / 9. state across launches, no poll in the move loop -----------------------------------------------------------------
def launches_of(iterations, cap, per_launch):
    """Launches the host enqueues before every group has stopped: a run that stops on the test does so in the sweep after its
    last move; a capped one in the launch of its last move."""
    return iterations // per_launch + 1 if iterations < max(cap, 1) else -(-max(cap, 1) // per_launch)


@pytest.mark.parametrize("n,cap", [(100, 40), (12, 1000)])
def test_the_state_survives_launches_and_every_launch_costs_one_synchronisation(dev, n, cap):
    group = random_group(n, 1, seed=8)
    ref, ref_it = D.batched_two_opt(*group, max_iterations=cap)
    assert ref_it == 40 if n == 100 else 0 < ref_it < cap
    for method in METHODS:
        pairs = set()
        for per_launch in (1, 3, 0):
            tours, its, stats = resident(dev, [group], cap, method, moves_per_launch=per_launch)
            assert its == [ref_it] and np.array_equal(tours[0], ref), (method, per_launch)
            if per_launch == 0:
                assert stats["host_syncs"] <= 2
            assert stats["host_syncs"] == launches_of(ref_it, cap, per_launch or 1024), (method, per_launch)
            pairs.add(stats["exact_pairs"])
        assert len(pairs) == 1                                   # no sweep runs twice, none is lost


def test_two_groups_that_stop_in_different_launches(dev):
    groups = [random_group(12, 1, seed=8), random_group(100, 1, seed=8), polygon(16, 1)]
    ref, ref_its, _ = launched(dev, groups, 40)
    for method in METHODS:
        tours, its, stats = resident(dev, groups, 40, method, moves_per_launch=7)
        assert its == ref_its and same_tours(tours, ref) and ref_its[2] == 0 < ref_its[0] < ref_its[1] == 40
        assert stats["host_syncs"] == 6                          # ceil(40 / 7): the slowest group's


def test_no_poll_in_the_move_loop(dev):
    group = random_group(100, 1, seed=8)
    syncs = []
    for cap in (3, 1000):
        ref, ref_it = D.batched_two_opt(*group, max_iterations=cap)
        assert ref_it == 3 if cap == 3 else ref_it >= 30
        for method in METHODS:
            tours, its, stats = resident(dev, [group], cap, method)
            assert its == [ref_it] and np.array_equal(tours[0], ref)
            syncs.append(stats["host_syncs"])
    assert len(set(syncs)) == 1 and syncs[0] <= 2


# ---- 10. exact_pairs -----------------------------------------------------------------------------------------------------------
def test_exact_pairs_is_the_formula_and_the_screen_cuts_it(dev):
    groups = [random_group(100, 1, seed=4), random_group(33, 3), polygon(24, 2)]
    for cap in (0, 5, 1000):
        t0, its0, st0 = resident(dev, groups, cap, "exact")
        assert st0["exact_pairs"] == exact_formula(groups, its0, cap)
        t1, its1, st1 = resident(dev, groups, cap, "screened")
        assert its1 == its0 and same_tours(t1, t0) and 0 < st1["exact_pairs"] <= st0["exact_pairs"]
    one = [random_group(100, 1, seed=4)]
    t0, its0, st0 = resident(dev, one, 1000, "exact")
    t1, its1, st1 = resident(dev, one, 1000, "screened")
    assert its0 == its1 and its0[0] > 0 and same_tours(t0, t1)
    print(f"n = 100: {its0[0]} moves, {st1['exact_pairs']} of {st0['exact_pairs']} pairs in float64")
    assert st1["exact_pairs"] < st0["exact_pairs"]


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_device_buffer_unchanged(dev):
    (p0, t0), (p1, t1) = random_group(5, 2), random_group(9, 1)
    pts, tours = np.concatenate([p0, p1]), np.concatenate([t0.reshape(-1), t1.reshape(-1)])
    who = "tsp_two_opt_resident"
    arrays = f"{who}: needs non-null device arrays, a host iterations_out[groups] and max_iterations >= 0"
    for change, text in (
            (dict(groups=0), f"{who}: groups = 0, needs at least 1"),
            (dict(null="group_n"), f"{who}: group_n / group_tours is null"),
            (dict(group_n=[5, 3]), f"{who}: group 1 has n = 3, needs n >= 4"),
            (dict(group_n=[5, 65535 * 16 + 1]), f"{who}: group 1 has n = {65535 * 16 + 1}, at most {65535 * 16} nodes"),
            (dict(group_tours=[0, 1]), f"{who}: group 0 has 0 tours, needs at least 1"),
            (dict(group_tours=[65535, 1]), f"{who}: more than 65535 tours in one call"),
            (dict(method=2), f"{who}: method 2 (0 exact, 1 screened)"),
            (dict(null="points"), arrays), (dict(null="tours"), arrays), (dict(null="workspace"), arrays),
            (dict(null="iterations_out"), arrays), (dict(cap=-1), arrays),
            (dict(moves_per_launch=-1), f"{who}: moves_per_launch = -1 < 0"),
            (dict(workspace_short=1), f"{who}: workspace 511 < 512 bytes")):
        kw = dict(dict(group_n=[5, 9], group_tours=[2, 1], pts=pts, tours=tours, cap=10), **change)
        rc, got, after = raw_call(dev, **kw)
        assert rc == -1 and got == text, change
        assert np.array_equal(after, tours), change
    rc, _, after = raw_call(dev, [5, 9], [2, 1], pts, tours, 10)                      # and the valid call runs
    want = np.concatenate([D.batched_two_opt(p0, t0, 10)[0].reshape(-1), D.batched_two_opt(p1, t1, 10)[0].reshape(-1)])
    assert rc == 0 and np.array_equal(after, want)


# ---- 12. wrappers and solvers --------------------------------------------------------------------------------------------------
def test_the_three_wrappers_equal_their_launched_mode(dev):
    from difusco_amd.decode import batched_two_opt_grouped, batched_two_opt_ragged, batched_two_opt_torch
    rng = np.random.default_rng(12)
    G, n, P = 3, 40, 2
    pts = np.stack([grid_points(rng, n) for _ in range(G)])
    tours = np.concatenate([random_tours(rng, n, P) for _ in range(G)])
    ragged = [random_group(17, 2), random_group(64, 1), random_group(33, 3)]
    for method in METHODS:
        for per_launch in (0, 5):
            kw = dict(max_iterations=50, device=dev, method=method)
            res = dict(mode="resident", moves_per_launch=per_launch)
            stats = {}
            a, ia = batched_two_opt_torch(pts[0], tours[:P], **kw)
            b, ib = batched_two_opt_torch(pts[0], tours[:P], stats=stats, **kw, **res)
            assert isinstance(ib, int) and ib == ia > 0 and np.array_equal(a, b) and b.dtype == np.int64
            assert set(stats) == {"exact_pairs", "host_syncs"}
            a, ia = batched_two_opt_grouped(pts, tours, **kw)
            b, ib = batched_two_opt_grouped(pts, tours, stats=stats, **kw, **res)
            assert np.array_equal(ia, ib) and ib.dtype == np.int64 and np.array_equal(a, b) and b.shape == tours.shape
            a, ia = batched_two_opt_ragged([p for p, _ in ragged], [t for _, t in ragged], **kw)
            b, ib = batched_two_opt_ragged([p for p, _ in ragged], [t for _, t in ragged], stats=stats, **kw, **res)
            assert np.array_equal(ia, ib) and same_tours(a, b)


def test_the_solvers_return_the_defaults_results(dev):
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
    kw = dict(parallel_sampling=P, two_opt_iterations=100)
    for extra in (dict(), dict(two_opt_method="screened")):
        res = dict(extra, two_opt_mode="resident")
        base = solve_tsp(model(5), pts[0], -1, generator=torch.Generator().manual_seed(0), **kw, **extra)
        assert base == solve_tsp(model(5), pts[0], -1, generator=torch.Generator().manual_seed(0), **kw, **res)
        assert base[3]["two_opt_iterations"] > 0
        base = solve_tsp_batch(model(0), pts, -1, seeds=seeds[:B], generators=gens(B), **kw, **extra)
        assert base == solve_tsp_batch(model(0), pts, -1, seeds=seeds[:B], generators=gens(B), **kw, **res)
        base = solve_tsp_batch(model(0), mixed, -1, seeds=seeds, generators=gens(4), **kw, **extra)
        assert base == solve_tsp_batch(model(0), mixed, -1, seeds=seeds, generators=gens(4), **kw, **res)
        assert [len(r[0]) - 1 for r in base] == [20, 33, 47, 60] and sum(r[3]["two_opt_iterations"] for r in base) > 0


def test_evaluate_gives_the_defaults_records_plus_one_key(dev, tmp_path):
    from difusco_amd import evaluate as EV
    split = _write_tsp(tmp_path / "tsp.txt", [50] * 4, seed=1)
    ckpt, _ = _ckpt(tmp_path / "last.ckpt", 64, 2)
    argv = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--two_opt_iterations", "100", "--do_valid_only", "--validation_examples", "4",
                 "--parallel_sampling", "2")
    plain_lines, plain = EV.run(argv)
    lines, recs = EV.run(argv + ["--two_opt_mode", "resident"])
    assert len(recs) == len(plain) == 4 and sum(r["2opt_iterations"] for r in plain) > 0
    assert list(lines[0]) == list(plain_lines[0]) + ["two_opt_mode"] and lines[0]["two_opt_mode"] == "resident"
    for r, p in zip(recs, plain):
        assert list(r) == list(p) + ["two_opt_mode"] and r["two_opt_mode"] == "resident"
        assert {k: v for k, v in r.items() if k != "two_opt_mode"} == p
    assert plain == EV.run(argv + ["--two_opt_mode", "launches"])[1]
