"""The reference of the MIS decode zoo (tests/mis_decode_cases.py), pinned on the CPU: it equals the project's oracle on every zoo
case and the reference's own recorded outputs (tests/golden/mis_decode_*.npz, the zoo file included); its sets are independent and
maximal; ``levels`` gives the chain lengths that can be worked out by hand; NaN scores rank last; the two zeros are one value.
No GPU."""
import glob
import os

import numpy as np
import pytest

import mis_decode_cases as Z
from oracle import tsp_decode_oracle as D

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ZOO_FILE = os.path.join(GOLDEN, "mis_decode_zoo.npz")
SOLO = sorted(p for p in glob.glob(os.path.join(GOLDEN, "mis_decode_*.npz")) if p != ZOO_FILE)
SMALL = [p for p in Z.PAIRS if p != Z.BIG]


def zoo_fixture(name, z=None):
    """-> (n, edge_index int64, predictions float32, solution int) of one case of tests/golden/mis_decode_zoo.npz."""
    z = np.load(ZOO_FILE) if z is None else z
    pred = z[f"{name}__predictions"]
    return len(pred), z[f"{name}__edge_index"].astype(np.int64), pred, z[f"{name}__solution"].astype(int)


def test_the_pairs_are_what_the_zoo_promises():
    assert len(set(Z.PAIRS)) == len(Z.PAIRS) and Z.BIG in Z.PAIRS
    assert {s for s, _ in Z.PAIRS} == set(Z.STRUCTURES) and {k for _, k in Z.PAIRS} == set(Z.SCORE_CLASSES)
    assert [s for s, _ in Z.PAIRS if Z.STRUCTURES[s][0] > 5000] == ["sparse_300000"]
    for name, (n, ei) in Z.STRUCTURES.items():
        assert ei.dtype == np.int64 and ei.shape[0] == 2 and (ei.size == 0 or (0 <= ei.min() and ei.max() < n)), name
        pairs = lambda e: e[:, np.lexsort((e[1], e[0]))]                 # noqa: E731
        assert np.array_equal(pairs(ei), pairs(ei[::-1])), name          # symmetric, as a multiset
    for d in Z.STAR_DEGREES:                                             # the hub's list in both orders
        for o, want in (("inc", list(range(1, d + 1))), ("dec", list(range(d, 0, -1)))):
            rowptr, col = Z.rows_of(Z.STRUCTURES[f"star_{d}_{o}"][1], d + 1)
            assert col[rowptr[0]:rowptr[1]].tolist() == want
    deg = lambda s: np.bincount(Z.STRUCTURES[s][1][0], minlength=Z.STRUCTURES[s][0])      # noqa: E731
    assert (deg("isolated_33") == 0).sum() == 33 and deg("edgeless_7").sum() == 0
    assert deg("duplicates").tolist() == (2 * deg("loops_all") - 2).tolist()
    rowptr, col = Z.rows_of(Z.STRUCTURES["loops_only"][1], 12)
    assert [col[rowptr[v]:rowptr[v + 1]].tolist() for v in (8, 9, 10, 11)] == [[8], [], [10], [11]]
    sizes = [n for n, _ in Z.UNION_40]
    assert len(sizes) == 40 and set(sizes) <= set(range(1, 10)) and sizes[19:22] == [1, 1, 1] and {1, 9} <= set(sizes)
    for n in Z.SORT_SIZES[:-1]:
        assert 3.5 < deg(f"sparse_{n}").mean() <= 4.0


def test_the_score_classes_are_what_the_zoo_promises():
    n = 4097
    s = {k: Z.make_scores(k, n, seed=3) for k in Z.SCORE_CLASSES}
    assert all(v.dtype == np.float32 and v.shape == (n,) for k, v in s.items() if k != "float64_collapsing")
    assert len(np.unique(s["distinct"])) == n and len(np.unique(s["denormal"])) == n
    tiny = np.finfo(np.float32).tiny
    assert np.all(np.abs(s["denormal"]) < tiny) and np.all(s["denormal"] != 0) and (s["denormal"] < 0).any() and (s["denormal"] > 0).any()
    assert np.all(np.diff(s["increasing_id"]) > 0) and np.all(np.diff(s["decreasing_id"]) < 0)
    assert s["alternating_id"][::2].min() > s["alternating_id"][1::2].max()
    z = s["mixed_zero_signs"]
    assert np.all(z == 0) and np.signbit(z[:12]).tolist() == [False] * 3 + [True] * 3 + [False] * 3 + [True] * 3
    assert set(np.unique(s["two_level"])) == {0.0, 1.0} and set(np.unique(s["sixteen_levels"])) == {k / 16 for k in range(17)}
    want = set()
    for b in (np.float32(0.5), np.float32(1.0), tiny):
        up = dn = b
        want.add(float(b))
        for _ in range(2):
            up, dn = np.nextafter(up, np.float32(2)), np.nextafter(dn, np.float32(0))
            want |= {float(up), float(dn)}
    assert {float(x) for x in s["one_ulp"]} == want and len(want) == 15
    assert -0.7 <= s["gaussian_range"].min() < 0 and 1 < s["gaussian_range"].max() <= 1.6
    assert np.isposinf(s["infinities"]).sum() > 1 and np.isneginf(s["infinities"]).sum() > 1
    nan = np.isnan(s["with_nan"])
    assert nan.sum() == round(0.05 * n) and set(s["with_nan"][nan].view(np.uint32)) == set(Z.NANS.view(np.uint32))
    assert np.signbit(s["with_nan"][nan]).any() and not np.signbit(s["with_nan"][nan]).all()
    c = s["float64_collapsing"]
    assert c.dtype == np.float64 and len(np.unique(c)) == n and len(np.unique(c.astype(np.float32))) == 8
    assert np.isnan(Z.make_scores("with_nan", 1)).all()


def test_the_visiting_order_on_the_special_values():
    a = np.array([0, -0.0, np.nan, -np.inf, 1, np.inf, -1], dtype=np.float32)
    assert Z.visiting_order(a).tolist() == [5, 4, 0, 1, 6, 3, 2]
    a = np.concatenate([Z.NANS, np.array([-np.inf, 0.0], dtype=np.float32)])
    assert Z.visiting_order(a).tolist() == [5, 4, 0, 1, 2, 3]            # every NaN after -inf, by id among themselves


@pytest.mark.parametrize("pair", SMALL, ids=Z.case_id)
def test_reference_equals_the_oracle_and_is_a_maximal_independent_set(pair):
    c = Z.case(*pair)
    n, ei, want = c["n"], c["edge_index"], c["want"]
    assert want.shape == (n,) and set(np.unique(want)) <= {0, 1}
    assert np.array_equal(want, D.mis_decode(np.asarray(c["scores"]).astype(np.float32), ei, n))
    assert Z.is_independent(n, ei, want) and Z.is_maximal(n, ei, want)
    assert 1 <= c["lmax"] <= n


def test_reference_on_the_big_case():
    c = Z.case(*Z.BIG)
    assert np.array_equal(c["want"], D.mis_decode(c["scores"], c["edge_index"], c["n"]))
    assert Z.is_independent(c["n"], c["edge_index"], c["want"]) and Z.is_maximal(c["n"], c["edge_index"], c["want"])


@pytest.mark.parametrize("path", SOLO, ids=[os.path.basename(p)[11:-4] for p in SOLO])
def test_reference_equals_the_recorded_solutions(path):
    z = np.load(path)
    n = len(z["predictions"])
    assert len(SOLO) == 3
    assert np.array_equal(Z.reference(z["predictions"], z["edge_index"], n), z["solution"].astype(int))


@pytest.mark.parametrize("name", Z.FIXTURE_STRUCTURES)
def test_reference_equals_the_recorded_zoo_solutions(name):
    n, ei, pred, sol = zoo_fixture(name)
    c = Z.case(name, "distinct")
    assert n == c["n"] and np.array_equal(ei, c["edge_index"]) and np.array_equal(pred.view(np.uint32), c["scores"].view(np.uint32))
    assert np.array_equal(Z.reference(pred, ei, n), sol) and np.array_equal(c["want"], sol)


def test_the_zoo_file_holds_every_structure_up_to_4097_nodes():
    z = np.load(ZOO_FILE)
    assert sorted(z.files) == sorted(["provenance"] + [f"{s}__{k}" for s in Z.FIXTURE_STRUCTURES
                                                     for k in ("edge_index", "predictions", "solution")])
    assert set(Z.STRUCTURES) - set(Z.FIXTURE_STRUCTURES) == {"sparse_300000"}
    assert {"edgeless_7", "one_node", "one_node_loop", "loops_only", "duplicates"} <= set(Z.FIXTURE_STRUCTURES)
    assert zoo_fixture("edgeless_7", z)[3].tolist() == [1] * 7


def test_levels():
    for n in (5, 257, 1000):
        ei = Z.STRUCTURES[f"path_{n}"][1]
        # monotone scores, in either direction, make every node wait for its predecessor: the chain is the whole path
        assert Z.levels(Z.make_scores("increasing_id", n), ei, n) == n
        assert Z.levels(Z.make_scores("decreasing_id", n), ei, n) == n
        assert Z.levels(Z.make_scores("all_zero", n), ei, n) == n
        assert Z.levels(Z.make_scores("alternating_id", n), ei, n) == 2
    for k in Z.SCORE_CLASSES:
        assert Z.levels(Z.make_scores(k, 70, seed=1), Z.STRUCTURES["k_70"][1], 70) == 70
        assert Z.levels(Z.make_scores(k, 7, seed=1), Z.STRUCTURES["edgeless_7"][1], 7) == 1
    assert Z.levels(np.zeros(1, np.float32), Z.STRUCTURES["one_node_loop"][1], 1) == 1
    assert Z.levels(np.zeros(12, np.float32), Z.STRUCTURES["loops_only"][1], 12) == 8
    assert [Z.round_bound(x) for x in (1, 4, 5, 70, 1000)] == [4, 4, 8, 72, 1000]
    for d, pos, kind in Z.STAR_PLACEMENTS:
        n, ei, scores = Z.star_placement(d, pos, kind)
        assert Z.levels(scores, ei, n) == (3 if kind == "in" else 5)     # .. leaf, hub, the other leaves


@pytest.mark.parametrize("d,pos,kind", Z.STAR_PLACEMENTS)
def test_star_placement(d, pos, kind):
    n, ei, scores = Z.star_placement(d, pos, kind)
    rowptr, col = Z.rows_of(ei, n)
    assert rowptr[1] - rowptr[0] == d and col[rowptr[0] + pos] == pos + 1
    want = Z.reference(scores, ei, n)
    assert want[0] == 0 and want[1:d + 1].tolist() == [1] * d           # the hub is OUT only because of the leaf at ``pos``
    blind = np.concatenate([ei[:, :pos], ei[:, pos + 1:d], ei[:, d:d + pos], ei[:, d + pos + 1:]], axis=1)
    assert blind.shape[1] == ei.shape[1] - 2 and Z.reference(scores, blind, n)[0] == 1
    assert {(63, 0), (63, 62), (64, 63), (65, 64), (128, 63), (129, 128), (300, 64), (300, 299)} <= {(d, p) for d, p, _ in Z.STAR_PLACEMENTS}


def test_no_nan_node_is_taken_while_a_non_nan_neighbour_could_be():
    seen = 0
    for pair in [p for p in SMALL if p[1] == "with_nan"]:
        c = Z.case(*pair)
        n, ei, s, want = c["n"], c["edge_index"], c["scores"], c["want"]
        nan = np.isnan(s)
        # the NaN-free nodes are decided among themselves: the set restricted to them is the decode of their induced graph
        keep = ~nan[ei[0]] & ~nan[ei[1]]
        clean = Z.reference(np.where(nan, -np.inf, s), ei[:, keep], n)
        assert np.array_equal(want[~nan], clean[~nan]), pair
        assert Z.is_maximal(n, ei[:, keep], np.where(nan, 1, clean)), pair
        a, b = ei
        assert not np.any((want[a] == 1) & nan[a] & (want[b] == 1) & (a != b)), pair      # and no NaN node beside a taken one
        seen += int(nan.sum())
    assert seen > 400                                  # NaN nodes met in all (5 % of the two 4 k graphs alone)


def test_mixed_zero_signs_equals_all_zero():
    pairs = [p for p in SMALL if p[1] == "mixed_zero_signs"]
    assert len(pairs) >= 10
    for s, _ in pairs:
        n, ei = Z.STRUCTURES[s]
        assert np.array_equal(Z.case(s, "mixed_zero_signs")["want"], Z.reference(np.zeros(n, np.float32), ei, n)), s
        assert Z.case(s, "mixed_zero_signs")["lmax"] == Z.levels(np.zeros(n, np.float32), ei, n)


def test_float64_scores_are_ranked_after_the_cast():
    for s, k in [p for p in SMALL if p[1] == "float64_collapsing"]:
        c = Z.case(s, k)
        n, ei, x = c["n"], c["edge_index"], c["scores"]
        assert np.array_equal(c["want"], Z.reference(x.astype(np.float32), ei, n))
        order64 = np.argsort(-x, kind="stable")
        assert not np.array_equal(order64, Z.visiting_order(x))          # float64 ranks them otherwise
