"""The TSP merge decode on the zoo of tests/tsp_merge_cases.py, on a real GPU: coincident cities and NaN, infinite, signed-zero,
subnormal and overflowing heat.  The per-graph entry with its host walk (``decode.merge_tours``) and the batched entry with the path
state in LDS and in the workspace (``difusco_tsp_merge_batch``, ``auto`` / ``global``) must all return exactly the reference's tour
and completed flag - the reference ranks NaN last, -inf before it, and never reads an entry that is not a pair - and one
``merge_iterations``, the reference's where the sample completed and no two distinct pairs tie.  Every case has n <= 129."""
import numpy as np
import pytest
import torch

import tsp_merge_cases as Z
from test_gpu_merge_batch import STATES, _existing, _raw
from test_tsp_merge_cases_host import zoo_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _three_entries(dev, pts, ei, heat):
    """[(tours, iterations, completed)] of the per-graph entry and of the batched entry in both states, one graph, heat [P, E]."""
    graph = [(pts, ei, np.asarray(heat, dtype=np.float32).reshape(len(heat), -1))]
    return [_existing(dev, pts, ei, graph[0][2])] + [_raw(dev, graph, state)[0] for state in STATES]


@pytest.mark.parametrize("pair", Z.PAIRS, ids=Z.case_id)
def test_every_entry_gives_the_reference(dev, pair):
    c = Z.case(*pair)
    tour, iterations, completed = c["want"]
    got = _three_entries(dev, c["points"], c["edge_index"], c["heat"][None])
    print("merge_iterations: per-graph", got[0][1], "auto", got[1][1], "global", got[2][1], "reference", iterations,
          "completed", completed, "tie_free", c["info"]["tie_free"])
    for tours, its, done in got:
        assert done == [completed]
        assert tours == [tour]
        assert its == got[0][1]
    if completed and c["info"]["tie_free"]:
        assert got[0][1] == [iterations]


@pytest.mark.parametrize("pair", Z.FIXTURE_PAIRS, ids=Z.case_id)
def test_recorded_reference_cases(dev, pair):
    """The reference's own results.  The recorded cases complete with a terminating run of one pair, and every run before it is
    visited whole, so the two-entries-per-pair count is the reference's count here even where +inf scores tie."""
    pts, ei, heat, tour, iterations, completed = zoo_fixture(Z.case_id(pair))
    for got in _three_entries(dev, pts, ei, heat[None]):
        assert got == ([tour], [iterations], [completed])


ISOLATION = ("knn_5_full", "knn_33_k8", "pair_33_k8_perm", "knn_65_full", "trio_33_k8", "knn_129_k8")
SAMPLE_KINDS = ("base", "all_nan", "inf_edges")


def test_samples_of_one_call_do_not_touch_each_other(dev):
    """The batched entry sorts the scores of all samples of a call together: NaN, +inf and -inf of one sample rank among the
    ordinary scores of the others before the samples are separated again.  Every sample must get what it gets alone, and the
    ordinary samples what they get from a call without an adversarial sample."""
    graphs = [(Z.points32(s), Z.STRUCTURES[s][1], np.stack([Z.case(s, k)["heat"] for k in SAMPLE_KINDS])) for s in ISOLATION]
    assert len({g[0].shape[0] for g in graphs}) == 4 and all((s, k) in Z.PAIRS for s in ISOLATION for k in SAMPLE_KINDS)
    ordinary = [(p, e, h[:1]) for p, e, h in graphs]
    for state in STATES:
        got = _raw(dev, graphs, state)
        clean = _raw(dev, ordinary, state)
        for s, (pts, ei, heat), (tours, its, done), (c_tours, c_its, c_done) in zip(ISOLATION, graphs, got, clean):
            for k, kind in enumerate(SAMPLE_KINDS):
                alone = _raw(dev, [(pts, ei, heat[k:k + 1])], state)[0]
                assert ([tours[k]], [its[k]], [done[k]]) == alone, (s, kind)
                want = Z.case(s, kind)["want"]
                assert (tours[k], done[k]) == (want[0], want[2]), (s, kind)
            assert (tours[:1], its[:1], done[:1]) == (c_tours, c_its, c_done), s
        flags = [ok for _, _, done in got for ok in done]
        assert any(flags) and not all(flags)


def test_dense_form_with_a_coincident_pair(dev):
    """``merge_tours_batch(..., edge_indices=None)``: complete graphs without index arrays, zero heat (and -0.0, and negative heat)
    on the coincident pair of one of them - 0/0 and -inf among n^2 entries, the diagonal included."""
    from difusco_amd.decode import merge_tours_batch
    cases = [Z.case("pair_33_dense", "coincident_zero"), Z.case("dense_33", "nan_edges"), Z.case("pair_33_dense", "coincident_negative"),
             Z.case("pair_33_dense", "coincident_negative_zero")]
    assert all(c["edge_index"] is None for c in cases)
    heats = [c["heat"].reshape(1, 33, 33) for c in cases]
    for state in STATES:
        res = merge_tours_batch(heats, [c["points"] for c in cases], None, sparse_graph=False, parallel_sampling=1, device=dev,
                                return_completed=True, state=state)
        for c, (tours, it, done) in zip(cases, res):
            assert (tours, done) == ([c["want"][0]], [c["want"][2]])
            assert c["want"][2] and c["info"]["tie_free"] and it == float(c["want"][1])


def test_an_adversarial_call_repeats_bitwise(dev):
    graphs = [(Z.points32(s), Z.STRUCTURES[s][1], np.stack([Z.case(s, k)["heat"] for k in kinds]))
              for s, kinds in (("trio_33_k8", ("coincident_zero", "coincident_negative", "all_nan", "inf_opposed")),
                               ("all_8_k8", ("coincident_negative", "nan_edges", "coincident_positive", "inf_edges")),
                               ("knn_65_k8_perm", ("nan_edges", "inf_edges", "gaussian_negative", "overflowing_sum")))]
    for state in STATES:
        first = _raw(dev, graphs, state)
        assert _raw(dev, graphs, state) == first
        for (pts, ei, heat), got in zip(graphs, first):
            assert _existing(dev, pts, ei, heat) == got
