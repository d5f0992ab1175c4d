"""The zoo of the TSP merge decode (tests/tsp_merge_cases.py), pinned on the CPU: the structures and heat classes are what the module
promises; every reference tour is a tour; the completed flags are the asserted ones, with both regimes present among the non-finite
cases; the cases DISCRIMINATE - a reference that ranks NaN first or into the zero block, or that drops -inf scores, gives another
tour or flag - so the GPU test can fail; and the oracle reproduces the reference's own recorded results
(tests/golden/tsp_merge_zoo.npz).  No GPU."""
import os

import numpy as np
import pytest

import tsp_merge_cases as Z

ZOO_FILE = os.path.join(os.path.dirname(__file__), "golden", "tsp_merge_zoo.npz")


def zoo_fixture(name, z=None):
    """-> (points float32, edge_index int64, heat float32, tour list, iterations int, completed bool) of one recorded case."""
    z = np.load(ZOO_FILE) if z is None else z
    return (z[f"{name}__points"], z[f"{name}__edge_index"].astype(np.int64), z[f"{name}__heat"], z[f"{name}__tour"].tolist(),
            int(z[f"{name}__iterations"]), bool(z[f"{name}__completed"]))


def test_the_structures_are_what_the_zoo_promises():
    assert {Z.STRUCTURES[s][0].shape[0] for s in Z.STRUCTURES} == set(Z.SIZES) == {5, 8, 33, 64, 65, 129}
    lengths = {s: len(Z.directed_edges(s)[0]) for s in Z.STRUCTURES}
    assert lengths["knn_5_full"] == 20 and lengths["knn_8_full"] == 56 and lengths["all_8_k8"] == 64      # inside one 64-lane block
    assert sorted({v % 64 for v in lengths.values()}) == [0, 1, 8, 20, 32, 56]                # block-aligned and mid-block ends
    assert max(lengths.values()) == 129 * 128
    for s, (pts, ei) in Z.STRUCTURES.items():
        n = pts.shape[0]
        assert pts.dtype == np.float64 and (ei is None or (ei.dtype == np.int64 and 0 <= ei.min() and ei.max() == n - 1)), s
        if ei is not None:                             # self loops, and both directions of most pairs, as in every k-NN list
            loops = int((ei[0] == ei[1]).sum())
            flat = set((ei[0] * n + ei[1]).tolist())
            both = sum((j * n + i) in flat for i, j in zip(ei[0].tolist(), ei[1].tolist()) if i != j)
            assert loops >= n - 8 and both > 0.5 * (ei.shape[1] - loops), s
    for s in Z.STRUCTURES:
        if s.endswith("_perm"):
            a, b = Z.STRUCTURES[s[:-5]][1], Z.STRUCTURES[s][1]
            assert not np.array_equal(a, b) and sorted(map(tuple, a.T.tolist())) == sorted(map(tuple, b.T.tolist()))
    groups = lambda s: sorted(tuple(g) for g in _coincident_groups(Z.points32(s)))          # noqa: E731
    assert groups("pair_33_full") == groups("pair_33_k8") == groups("pair_33_dense") == [(4, 17)]
    assert groups("trio_33_full") == groups("trio_33_k8_perm") == [Z.TRIO, Z.TRIO_PAIR] == [(3, 7, 20), (11, 30)]
    assert groups("all_8_full") == groups("all_8_k8") == [tuple(range(8))]
    assert groups("cast_65_full") == groups("cast_65_k8") == [(9, 40)]
    assert _coincident_groups(Z.STRUCTURES["cast_65_full"][0]) == []                          # distinct before the float32 cast
    assert all(groups(s) == [] for s in Z.PLAIN) and set(Z.PLAIN) | set(Z.COINCIDENT) == set(Z.STRUCTURES)
    for s in Z.COINCIDENT:                             # coincident cities are each other's nearest neighbours: every such pair is a candidate
        n = Z.STRUCTURES[s][0].shape[0]
        row, col = Z.directed_edges(s)
        listed = set((row * n + col).tolist())
        assert all(a * n + b in listed or b * n + a in listed for g in groups(s) for a in g for b in g if a != b), s


def _coincident_groups(pts):
    seen = {}
    for v, p in enumerate(map(tuple, pts.tolist())):
        seen.setdefault(p, []).append(v)
    return [tuple(g) for g in seen.values() if len(g) > 1]


def test_the_heat_classes_are_what_the_zoo_promises():
    tiny = np.finfo(np.float32).tiny
    for s in ("trio_33_k8", "pair_33_full_perm", "cast_65_k8", "all_8_k8"):
        co = Z.coincident_edges(s)
        base = Z.make_heat("base", s)
        assert base.dtype == np.float32 and co.any() and np.all(base >= np.float32(1e-3)) and np.all(np.isfinite(base))
        assert np.all(Z.make_heat("coincident_positive", s)[co] > 0)
        for kind, want_sign in (("coincident_zero", False), ("coincident_negative_zero", True)):
            h = Z.make_heat(kind, s)
            assert np.all(h[co] == 0) and np.all(np.signbit(h[co]) == want_sign) and np.all(h[~co] > 0)
        assert np.all(Z.make_heat("coincident_negative", s)[co] < 0) and np.all(Z.make_heat("coincident_negative", s)[~co] > 0)
        g = Z.make_heat("gaussian_negative", s)
        assert np.all(g[co] < 0) and np.all(np.isfinite(g))
    for s in ("knn_33_k8", "knn_129_k8_perm", "dense_33", "pair_33_k8"):
        row, col = Z.directed_edges(s)
        n = Z.STRUCTURES[s][0].shape[0]
        where = lambda mask: list(zip(row[mask].tolist(), col[mask].tolist()))                # noqa: E731
        h = Z.make_heat("nan_edges", s)
        nan = where(np.isnan(h))
        assert len(nan) == 5 and all(i != j for i, j in nan) and not any((j, i) in nan for i, j in nan)   # one direction only
        back = [np.flatnonzero((row == j) & (col == i)) for i, j in nan]
        assert len(back[0]) == 1 and np.isfinite(h[back[0][0]])                               # a NaN edge whose reverse is listed
        assert len(set(h[np.isnan(h)].view(np.uint32).tolist())) == 4 and np.signbit(h[np.isnan(h)]).sum() == 2
        h = Z.make_heat("inf_edges", s)
        assert np.isposinf(h).sum() == 3 and np.isneginf(h).sum() == 3 and not np.isnan(h).any()
        assert len({(min(i, j), max(i, j)) for i, j in where(np.isinf(h))}) == 6
        h = Z.make_heat("inf_opposed", s)
        (i, j), (k, l) = where(np.isposinf(h))[0], where(np.isneginf(h))[0]
        assert np.isinf(h).sum() == 2 and (i, j) == (l, k) and i != j
        assert Z.analyse(Z.points32(s), Z.STRUCTURES[s][1], h)["nan_scores"] == 1             # inf + -inf
        z = Z.make_heat("negative_zero_edges", s)
        assert 0.2 < np.mean(z == 0) < 0.4 and np.all(np.signbit(z[z == 0])) and np.all(z[z != 0] > 0)
        g = Z.make_heat("gaussian_negative", s)
        assert 0.25 < np.mean(g < 0) < 0.42
        sub = Z.make_heat("subnormal", s)
        assert np.all(sub > 0) and np.all(sub < tiny)
        o = Z.make_heat("overflowing_sum", s)
        assert np.all(np.isfinite(o)) and Z.analyse(Z.points32(s), Z.STRUCTURES[s][1], o)["pinf_scores"] > 10
        assert np.isnan(Z.make_heat("all_nan", s)).all()
    assert {k for _, k in Z.PAIRS} == set(Z.HEAT_CLASSES) and {s for s, _ in Z.PAIRS} == set(Z.STRUCTURES)
    assert len(set(Z.PAIRS)) == len(Z.PAIRS) and set(Z.FIXTURE_PAIRS) <= set(Z.PAIRS)
    # the score classes the rule names, over the cases: +inf, 0/0, -inf from coincident cities and from the heat itself
    for (s, k), field in {("pair_33_k8", "coincident_positive"): "pinf_scores", ("pair_33_k8", "coincident_zero"): "nan_scores",
                          ("pair_33_k8", "coincident_negative_zero"): "nan_scores", ("pair_33_k8", "coincident_negative"): "ninf_scores",
                          ("knn_33_k8", "inf_edges"): "ninf_scores", ("knn_33_k8", "nan_edges"): "nan_scores"}.items():
        assert Z.case(s, k)["info"][field] >= 1, (s, k)
    assert Z.case("trio_33_k8", "coincident_zero")["info"]["nan_scores"] == 4                 # 3 pairs of the trio + the pair
    assert Z.case("all_8_k8", "coincident_negative")["info"]["ninf_scores"] == 28


@pytest.mark.parametrize("pair", Z.PAIRS, ids=Z.case_id)
def test_reference_gives_a_tour_and_the_asserted_flag(pair):
    c = Z.case(*pair)                                  # the second walk of ``analyse`` agrees with the oracle's, or case() raises
    tour, iterations, completed = c["want"]
    n = c["points"].shape[0]
    assert c["points"].dtype == np.float32 and c["heat"].dtype == np.float32
    assert len(tour) == n + 1 and tour[0] == tour[-1] == 0 and sorted(tour[:-1]) == list(range(n))
    assert 1 <= iterations <= n * n
    assert completed == Z.expected_completed(*pair)


def test_both_regimes_hold_non_finite_entries():
    done = {p: Z.case(*p)["want"][2] for p in Z.PAIRS}
    non_finite = ("coincident_positive", "coincident_zero", "coincident_negative_zero", "coincident_negative", "nan_edges", "inf_edges",
                  "inf_opposed")
    for k in non_finite:
        assert {done[p] for p in Z.PAIRS if p[1] == k} == {True, False}, k
    for n in (33, 65):                                 # K = n - 1: completed for every class but the all-NaN one
        assert all(ok == (k != "all_nan") for (s, k), ok in done.items() if s in (f"knn_{n}_full", f"pair_{n}_full"))
    assert not any(done[("trio_33_k8", k)] for k in ("coincident_zero", "coincident_negative", "inf_edges", "gaussian_negative"))
    assert done[("all_8_full", "coincident_positive")] and done[("all_8_k8", "coincident_positive")]
    assert not done[("all_8_full", "coincident_zero")] and not done[("all_8_k8", "coincident_zero")]
    assert not any(ok for (s, k), ok in done.items() if k == "all_nan")
    # merge_iterations can be held against the reference on many cases of either kind
    pinned = [p for p in Z.PAIRS if done[p] and Z.case(*p)["info"]["tie_free"]]
    assert len(pinned) > 50 and {k for _, k in pinned} >= set(non_finite) - {"inf_edges"}


def _differs(pair, **wrong):
    c = Z.case(*pair)
    got = Z.reference(c["points"], c["edge_index"], c["heat"], **wrong)[0]
    return (got[0], got[2]) != (c["want"][0], c["want"][2])


def test_the_cases_tell_a_wrong_nan_rank_from_the_rule():
    """Every case with a NaN score, under the two wrong ranks.  Which cases change is printed; that some do, among the K = n - 1 and
    among the K = 8 structures, is asserted: a decode that puts NaN first, or treats it as a zero, fails the GPU test."""
    with_nan = [p for p in Z.PAIRS if Z.case(*p)["info"]["nan_scores"] and p[1] != "all_nan"]
    assert len(with_nan) > 60
    for rank in ("first", "zero"):
        hit = [p for p in with_nan if _differs(p, nan_rank=rank)]
        print(rank, len(hit), "of", len(with_nan), [Z.case_id(p) for p in hit])
        assert any(s.endswith(("_full", "_full_perm")) for s, _ in hit), rank
        assert any("_k8" in s and not s.startswith("all_8") for s, _ in hit), rank
        for kind in ("coincident_zero", "coincident_negative_zero", "nan_edges", "inf_opposed"):      # 0/0, NaN heat, inf + -inf
            assert any(k == kind for _, k in hit), (rank, kind)


def test_the_cases_tell_dropped_negative_infinities_from_the_rule():
    with_ninf = [p for p in Z.PAIRS if Z.case(*p)["info"]["ninf_scores"]]
    assert len(with_ninf) > 40
    hit = [p for p in with_ninf if _differs(p, ninf_absent=True)]
    print(len(hit), "of", len(with_ninf), [Z.case_id(p) for p in hit])
    assert hit and {"coincident_negative", "inf_edges"} <= {k for _, k in hit}


def test_the_zoo_file_holds_the_recorded_cases():
    z = np.load(ZOO_FILE)
    fields = ("points", "edge_index", "heat", "tour", "iterations", "negative_key_entries", "completed")
    assert sorted(z.files) == sorted(["provenance"] + [f"{Z.case_id(p)}__{f}" for p in Z.FIXTURE_PAIRS for f in fields])
    kinds = {k for _, k in Z.FIXTURE_PAIRS}
    assert {"coincident_positive", "coincident_zero", "coincident_negative", "nan_edges", "inf_edges", "inf_opposed"} <= kinds
    assert all(s.endswith(("_full", "_full_perm")) and not s.startswith(("trio", "all_8")) for s, _ in Z.FIXTURE_PAIRS)


@pytest.mark.parametrize("pair", Z.FIXTURE_PAIRS, ids=Z.case_id)
def test_oracle_reproduces_the_recorded_reference(pair):
    """The reference's own merge_tours + merge_cython ran on exactly the case's arrays; the oracle (through ``reference``) gives its
    tour, its iteration count and its flag."""
    c = Z.recorded_case(*pair)                         # asserts that the result cannot depend on the unstable argsort
    pts, ei, heat, tour, iterations, completed = zoo_fixture(Z.case_id(pair))
    assert pts.dtype == np.float32 and np.array_equal(pts, c["points"]) and np.array_equal(ei, c["edge_index"])
    assert np.array_equal(heat.view(np.uint32), c["heat"].view(np.uint32))
    assert completed and c["want"] == (tour, iterations, completed)
    assert Z.reference(pts, ei, heat)[0] == (tour, iterations, completed)
