"""The restatement of the sampled k-opt search (tests/tsp_kopt_search_emulation.py) against what the rule promises, on the CPU:
every applied action is the explicit sequence of prefix reversals, the tour stays a permutation closed on its first city, the
length falls by the action's value, a depth-1 search finds nothing on a 2-opt optimum, dead rows end a simulation, the Philox
word layout by hand - and the inputs of the GPU test make the emulation move, so that the device comparison proves something."""
import numpy as np
import pytest

import tsp_kopt_search_cases as C
import tsp_kopt_search_emulation as K
from oracle import tsp_decode_oracle as O
from philox_reference import philox4x32_10
from tsp_iterated_search_emulation import tour_length

MULTI_ROUND = [name for name, (_, kw) in C.cases().items() if kw["max_rounds"] > 0]


@pytest.mark.parametrize("name", ["ladder-n7", "ladder-n65", "S65-D2", "corners", "begin-at-n-1"])
def test_an_action_is_its_prefix_reversals(name):
    groups, _ = C.cases()[name]
    want, logs = C.expected(name)
    tours = [t for pts, starts, *_ in groups for t in starts]
    points = [pts for pts, starts, *_ in groups for _ in starts]
    assert sum(len(log) for log in logs) > 0
    for pts, start, log in zip(points, tours, logs):
        n = len(start) - 1
        for r, s, value, istar, p, before, steps, after, len_before, len_after in log:
            assert value > 1e-6 and 1 <= istar == len(steps)
            path = [before[(p + 1 + x) % n] for x in range(n)]
            for e, b, c, y, _ in steps:
                assert path[0] == b and path[y] == c and 2 <= y <= n - 2
                path[:y] = path[:y][::-1]
            z = path.index(int(start[0]))
            assert after == path[z:] + path[:z]
            assert sorted(after) == list(range(n)) and after[0] == start[0]
            assert len_before == tour_length(pts, before + before[:1]) and len_after == tour_length(pts, after + after[:1])
            assert abs((len_before - len_after) - value) <= 1e-9


@pytest.mark.parametrize("name", sorted(C.cases()))
def test_results_are_closed_permutations_and_never_longer(name):
    groups, kw = C.cases()[name]
    want, _ = C.expected(name)
    for (pts, starts, *_), (tours, per) in zip(groups, want):
        for start, t, b in zip(starts, tours, range(len(starts))):
            n = len(start) - 1
            assert sorted(t[:-1].tolist()) == list(range(n)) and t[0] == t[-1] == start[0]
            assert per["first_length"][b] == tour_length(pts, start) and per["final_length"][b] == tour_length(pts, t)
            assert per["final_length"][b] <= per["first_length"][b] and per["reverted"][b] == 0
            assert per["rounds"][b] <= kw["max_rounds"] and per["actions"][b] <= per["depth_sum"][b] <= kw["depth"] * per["actions"][b]
            if kw["max_rounds"] == 0:
                assert np.array_equal(t, start)


@pytest.mark.parametrize("name", MULTI_ROUND)
def test_the_gpu_inputs_make_the_emulation_move(name):
    """At least one action on at least one tour of every multi-round case: otherwise the device comparison proves nothing."""
    want, _ = C.expected(name)
    assert sum(sum(per["actions"]) for _, per in want) >= 1


def test_the_stall_case_stops_one_tour_and_runs_another_on():
    _, kw = C.cases()["stall"]
    want, _ = C.expected("stall")
    rounds = [r for _, per in want for r in per["rounds"]]
    assert min(rounds) < kw["max_rounds"] and max(rounds) == kw["max_rounds"]
    assert rounds[0] < kw["max_rounds"] and rounds[-1] < kw["max_rounds"]       # the tours of 5 and of 7 cities


def test_begin_position_n_minus_1_is_applied():
    _, logs = C.expected("begin-at-n-1")
    assert any(a[4] == 6 for a in logs[0])


def test_depth_one_finds_nothing_on_a_two_opt_optimum():
    """A depth-1 action removes two tour edges and adds the two that reconnect the tour: a 2-opt move."""
    for n in (12, 40):
        pts, starts, rp, col, heat, seeds, offsets = C.group(n, 3)
        done, _ = O.batched_two_opt(pts, starts, 10000)
        full = np.arange(0, n * n + 1, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), n)     # every pair is a candidate
        for t, s in zip(done, seeds):
            out, per = K.search_tour(pts, t, *full, np.ones(n * n, np.float32), s, 0, samples=256, depth=1, max_rounds=4,
                                     patience=1000)
            assert per["actions"] == 0 and per["rounds"] == 4 and np.array_equal(out, t)
        moved = K.search_tour(pts, starts[1], *full, np.ones(n * n, np.float32), seeds[0], 0, samples=256, depth=1, max_rounds=4)
        assert moved[1]["actions"] > 0                            # the same search does move a random tour, which is no optimum


def _one_simulation(n, rp, col, heat, depth=3):
    pts = np.random.default_rng(n).random((n, 2))
    tour = np.concatenate([np.arange(n), [0]])
    st = K.State(pts, tour, rp, col, heat)
    words = K.round_words(3, 0, 0, 8, depth)
    return [K.simulate(st, s, words, depth, 1.0) for s in range(8)], st


def test_dead_rows_end_a_simulation():
    n = 9
    rp, col = np.arange(0, n * n + 1, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), n)
    for h in (np.zeros(n * n, np.float32), np.full(n * n, np.nan, np.float32), np.full(n * n, -3.0, np.float32)):
        sims, st = _one_simulation(n, rp, col, h)
        assert all(x == 0.0 for x in st.sw)
        assert all(v is None and i == 0 and steps == [] for v, i, steps in sims)
    sims, _ = _one_simulation(n, np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))   # degree 0 everywhere
    assert all(v is None and steps == [] for v, _, steps in sims)
    live, _ = _one_simulation(n, rp, col, np.ones(n * n, np.float32))
    assert all(len(steps) >= 1 for _, _, steps in live)
    # one dead row: a simulation whose head reaches city 4 ends there, with the steps it has
    h = np.ones((n, n), np.float32)
    h[4] = 0.0
    sims, st = _one_simulation(n, rp, col, h.reshape(-1), depth=10)
    assert st.sw[4] == 0.0
    heads = [b for _, _, steps in sims for _, b, _, _, _ in steps]
    assert heads and 4 not in heads


def test_candidates_skip_self_entries_and_later_duplicates():
    rp, col = np.array([0, 5, 5, 7]), np.array([0, 1, 2, 1, 2, 2, 0])
    assert K.candidates(rp, col) == [[1, 2], [], [6]]
    st = K.State(np.random.default_rng(0).random((3, 2)), [0, 1, 2, 0], rp, col,
                 np.array([9, 0.5, np.nan, 0.25, 7, 1, -1], np.float32))
    assert st.w == {1: 50.0, 2: 0.0, 6: 0.0} and st.sw == [50.0, 0.0, 0.0]
    assert K.clamp_weight(np.float32(2.5)) == 100.0 and K.clamp_weight(np.float32(np.nan)) == 0.0


def test_word_layout_by_hand():
    """Step i of simulation s in round r: word i mod 4 of the call with index ((i div 4) << 32) | s at offset + r mod 2^64."""
    seed, offset, r, S, s = 0x123456789ABCDEF, (1 << 64) - 2, 5, 77, 41
    words = K.round_words(seed, offset, r, S, 10)
    assert len(words) == 3
    for i, (call, word) in {0: (0, 0), 3: (0, 3), 4: (1, 0), 8: (2, 0)}.items():
        by_hand = philox4x32_10(seed, 3, (call << 32) | s)        # (2^64 - 2 + 5) mod 2^64 = 3
        assert K.step_word(words, i, s) == int(by_hand[word])
    assert K.step_word(words, 4, s) != K.step_word(words, 0, s)
