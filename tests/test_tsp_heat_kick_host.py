"""The heat-biased kicks of the iterated TSP search on the host: the numpy restatement of the rule
(tests/tsp_heat_kick_emulation.py) held to the rule's own statements - the range of a draw, the corners of the quantisation, the
cases of q(u, v), the concentration of the draws on cold edges, the 64-bit running weights - and the argument checks of the
Python layers and the runner that need no GPU, so that the GPU tests compare against a reference that is itself pinned."""
import types
from fractions import Fraction

import numpy as np
import pytest

import multi_local_search_emulation as E
import tsp_heat_kick_emulation as H
import tsp_iterated_search_emulation as T
from difusco_amd.decode import (TSP_KICK_BIASES, batched_iterated_search_grouped, batched_iterated_search_ragged,
                                batched_iterated_search_torch, check_tsp_kick_bias)
from philox_reference import philox4x32_10


def instance(n, s):
    rng = np.random.default_rng(100 * n + s)
    return rng.random((n, 2)), np.concatenate([[0], rng.permutation(n - 1) + 1, [0]])


def is_closed_permutation(tour, n, first):
    t = np.asarray(tour)
    return len(t) == n + 1 and t[0] == t[-1] == first and sorted(t[:-1].tolist()) == list(range(n))


def tour_graph(tour):
    """One edge per row: city tour[k] -> tour[k + 1]; ``order[k]`` = the entry of position k."""
    t = np.asarray(tour)
    n = len(t) - 1
    col = np.empty(n, dtype=np.int32)
    col[t[:-1]] = t[1:]
    return np.arange(n + 1, dtype=np.int32), col, t[:-1]


@pytest.mark.parametrize("n", [4, 5, 8, 64])
def test_draw_range(n):
    pts, start = instance(n, 3)
    rp, col = H.knn_csr(pts, 8)
    heat = np.random.default_rng(n).random(len(col)).astype(np.float32)
    W = H.prefix(H.position_weights(start, H.edge_table(rp, col, heat)))
    assert len(W) == n + 1 and all(1 <= b - a <= 65536 for a, b in zip(W, W[1:]))
    seen = set()
    for seed in range(6):
        for t in range(4):
            for a, l1, l2 in H.heat_kick_draws(seed, 11, t, n, 16, 30, W):
                assert 1 <= a and l1 >= 1 and l2 >= 1 and a + l1 + l2 <= n
                seen.add((a, l1, l2))
    if n == 4:                                                   # Lc = 1 and M = 2
        assert seen == {(1, 1, 1), (2, 1, 1)}


def exact_q(h):
    """q of one finite float32 heat by exact arithmetic: the float32 product rounded once, then to the nearest even integer."""
    c = min(max(Fraction(float(np.float32(h))), Fraction(0)), Fraction(1))
    prod = np.float32(float(c * 65535))                          # the exact product fits a double: one rounding to float32
    return round(Fraction(float(prod)))                          # python rounds halves to even


def test_quantisation_corners():
    q = H.quantise(np.array([-1.0, 2.0, np.nan, 0.0, 1.0, 0.5, 1.5 / 65535, -np.inf, np.inf], dtype=np.float32))
    assert q.dtype == np.uint32
    assert q[:5].tolist() == [0, 65535, 0, 0, 65535] and q[7:].tolist() == [0, 65535]
    assert q[5] == 32768 == exact_q(0.5)                         # 32767.5 is a tie: to the even 32768
    assert q[6] == exact_q(1.5 / 65535) and q[6] in (1, 2)
    rng = np.random.default_rng(5)
    h = rng.random(2000).astype(np.float32)
    assert H.quantise(h).tolist() == [exact_q(x) for x in h]
    ties = ((np.arange(0, 65535, 257) + 0.5) / 65535).astype(np.float32)
    assert H.quantise(ties).tolist() == [exact_q(x) for x in ties]


def test_edge_q_cases():
    # row 0: 0->1 twice (0.25, 0.75) and 0->0; row 1: empty; row 2: 2->3; row 3: 3->2 and 3->0
    rp = np.array([0, 3, 3, 4, 6], dtype=np.int32)
    col = np.array([1, 1, 0, 3, 2, 0], dtype=np.int32)
    heat = np.array([0.25, 0.75, 1.0, 0.5, 0.125, 1.0], dtype=np.float32)
    table = H.edge_table(rp, col, heat)
    q = H.quantise(heat)
    assert table[(0, 1)] == q[1] > q[0]                          # duplicates: the largest
    w = H.position_weights([0, 1, 2, 3, 0], table)
    assert w[0] == 65536 - q[1]                                  # one direction only: 0->1, no 1->0
    assert w[1] == 65536                                         # 1-2 is in neither row
    assert w[2] == 65536 - max(q[3], q[4]) == 65536 - q[3]       # both directions: the larger
    assert w[3] == 1                                             # 3->0 has heat 1.0
    assert H.prefix(w) == [0, w[0], w[0] + w[1], w[0] + w[1] + w[2], sum(w)]


CONC_SEED, CONC_OFFSET = 3, 0


def concentration_case():
    """n = 64, span 3, a fixed tour whose edges all have heat 1.0 except those at positions 20 and 40 (heat 0)."""
    n = 64
    pts, tour = instance(n, 4)
    rp, col, order = tour_graph(tour)
    heat = np.ones(n, dtype=np.float32)
    heat[order[[20, 40]]] = 0.0
    return pts, tour, rp, col, heat


def test_concentration():
    pts, tour, rp, col, heat = concentration_case()
    n = 64
    w = H.position_weights(tour, H.edge_table(rp, col, heat))
    assert [k for k in range(n) if w[k] != 1] == [20, 40] and w[20] == w[40] == 65536
    W = H.prefix(w)
    assert W[-1] == 131134                                       # a draw misses with probability at most 62 / 131134
    draws = H.heat_kick_draws(CONC_SEED, CONC_OFFSET, 0, n, 16, 3, W)
    assert {a for a, _, _ in draws} <= {21, 41} and len(draws) == 16
    uniform = T.kick_draws(CONC_SEED, CONC_OFFSET, 0, n, 16, 3)
    assert not {a for a, _, _ in uniform} <= {21, 41}
    assert [d[1:] for d in draws] == [d[1:] for d in uniform]    # l1 and l2 are the uniform rule's
    _, kept = T.apply_kick(tour, draws)
    _, kept_uniform = T.apply_kick(tour, uniform)
    assert 1 <= sum(kept) <= 2 < sum(kept_uniform)


def test_64_bit_prefix():
    n = 70001
    tour = np.concatenate([np.arange(n), [0]])
    rp, col, _ = tour_graph(tour)
    W = H.prefix(H.position_weights(tour, H.edge_table(rp, col, np.zeros(n, dtype=np.float32))))
    assert W[-1] == n * 65536 and W[n - 60] > 2 ** 32
    Lc = 30
    for t in range(2):
        got = H.heat_kick_draws(9, 5, t, n, 16, Lc, W)
        for c, (a, l1, l2) in enumerate(got):
            w0, w1, w2, w3 = (int(x) for x in philox4x32_10(9, 5 + t, c))
            assert (l1, l2) == (1 + w1 % Lc, 1 + w2 % Lc)
            M = n - l1 - l2
            assert a == 1 + (((w0 << 32) | w3) % (M * 65536)) // 65536
    assert any(a * 65536 > 2 ** 32 for a, _, _ in got)           # a draw lands above the 32-bit range


@pytest.mark.parametrize("descent", ["full", "focused"])
def test_tour_properties(descent):
    n = 200
    pts, start = instance(n, 1)
    rp, col = H.knn_csr(pts, 8)
    first = T.tour_length(pts, E.search_tour(pts, start)[0])
    for seed in range(3):
        heat = np.random.default_rng(seed).random(len(col)).astype(np.float32)
        log = []
        out, c, per = H.search_tour(pts, start, rp, col, heat, seed, 2, kicks=4, kick_size=8, span=16, descent=descent,
                                    draws_log=log)
        assert is_closed_permutation(out, n, start[0])
        assert per["final_length"] <= per["first_length"] == first
        assert per["final_length"] == T.tour_length(pts, out)
        assert len(log) == 4 and all(1 <= a and a + l1 + l2 <= n for d in log for a, l1, l2 in d)
        assert ("closing_sweeps" in per) == (descent == "focused")
    # kicks = 0 is the multi-move search whatever the heat
    want, wc = E.search_tour(pts, start)
    got, gc, gp = H.search_tour(pts, start, rp, col, heat, 1, 2, kicks=0, descent=descent)
    assert np.array_equal(got, want) and gc == wc and gp["kicks_kept"] == 0


def test_python_layers_refuse_before_any_library_call():
    assert TSP_KICK_BIASES == ("uniform", "heat")
    assert check_tsp_kick_bias("uniform") == "uniform" and check_tsp_kick_bias("heat", 3) == "heat"
    with pytest.raises(ValueError, match="kick_bias"):
        check_tsp_kick_bias("cold")
    with pytest.raises(ValueError, match="local_search_kicks > 0"):
        check_tsp_kick_bias("heat", 0)
    pts, start = instance(8, 1)
    heat, ei = np.zeros((1, 8), dtype=np.float32), np.stack([np.arange(8), (np.arange(8) + 1) % 8])
    with pytest.raises(ValueError, match="needs heat"):
        batched_iterated_search_torch(pts, start[None], kicks=1, kick_bias="heat")
    with pytest.raises(ValueError, match="only with kick_bias='heat'"):
        batched_iterated_search_torch(pts, start[None], kicks=1, heat=heat, edge_index=ei)
    with pytest.raises(ValueError, match="kick_bias"):
        batched_iterated_search_torch(pts, start[None], kicks=1, kick_bias="warm", heat=heat, edge_index=ei)
    with pytest.raises(ValueError, match="needs heat"):
        batched_iterated_search_grouped(pts[None], start[None], kicks=1, kick_bias="heat")
    with pytest.raises(ValueError, match="only with kick_bias='heat'"):
        batched_iterated_search_ragged([pts], [start[None]], kicks=1, heat=[heat], edge_index=[ei])


def test_pipeline_and_runner_refuse_the_bias_without_kicks():
    from difusco_amd import evaluate
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    model = types.SimpleNamespace(device="cpu", seed=0)
    pts = np.random.default_rng(0).random((8, 2))
    for fn, p in ((solve_tsp, pts), (solve_tsp_batch, pts[None]), (solve_tsp_batch, [pts])):
        with pytest.raises(ValueError, match="local_search_kicks > 0"):
            fn(model, p, 4, local_search="multi2opt+oropt", local_search_kick_bias="heat")
        with pytest.raises(ValueError, match="kick_bias"):
            fn(model, p, 4, local_search="multi2opt+oropt", local_search_kicks=2, local_search_kick_bias="cold")
    base = ["--task", "tsp", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."]
    kicked = ["--local_search", "multi2opt+oropt", "--tsp_local_search_kicks", "3"]
    assert evaluate.parse_args(base)[0].tsp_local_search_kick_bias == "uniform"
    assert evaluate.parse_args(base + kicked + ["--tsp_local_search_kick_bias", "heat"])[0].tsp_local_search_kick_bias == "heat"
    assert evaluate.parse_args(base + ["--tsp_local_search_kick_bias", "uniform"])[0].tsp_local_search_kicks == 0
    for bad in (["--tsp_local_search_kick_bias", "heat"],
                ["--local_search", "multi2opt+oropt", "--tsp_local_search_kicks", "0", "--tsp_local_search_kick_bias", "heat"],
                kicked + ["--tsp_local_search_kick_bias", "cold"]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(base + bad)
    with pytest.raises(SystemExit):
        evaluate.parse_args(["--task", "mis"] + base[2:] + ["--tsp_local_search_kick_bias", "heat"])
