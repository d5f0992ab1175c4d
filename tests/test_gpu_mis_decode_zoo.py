"""The greedy MIS decode on the GPU (``difusco_mis_decode``) against the sequential reference of tests/mis_decode_cases.py (pinned by
tests/test_mis_decode_host.py) on adversarial scores and graph structures: exact ties in masses, both zeros, one-ulp steps,
subnormals, infinities and NaN; paths, stars around the lane stride with the one neighbour that matters at a chosen list position,
complete graphs, isolated nodes, self loops, duplicate entries, one node, no entry at all, a union of small graphs, and sizes across
the switch of the radix sort.  Every comparison is exact equality of the whole 0/1 array; the round count is held to the bound that
follows from the kernel's code, ``rounds % 4 == 0`` and ``4 <= rounds <= 4 * ceil(Lmax / 4)``."""
import ctypes

import numpy as np
import pytest
import torch

import mis_decode_cases as Z
from test_mis_decode_host import SMALL, zoo_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _decode(dev, scores, lmax=None, **graph):
    """One call; the set comes back with its round count checked against the bound of ``lmax`` (when given)."""
    from difusco_amd.decode import mis_decode_np
    stats = {}
    sol = mis_decode_np(scores, device=dev, stats=stats, **graph)
    assert sol.dtype == int and set(np.unique(sol)) <= {0, 1}
    rounds = stats["rounds"]
    assert rounds % 4 == 0 and rounds >= 4
    if lmax is not None:
        assert rounds <= Z.round_bound(lmax), (rounds, lmax)
    return sol


@pytest.mark.parametrize("pair", SMALL, ids=Z.case_id)
def test_zoo_case_equals_reference(dev, pair):
    c = Z.case(*pair)
    got = _decode(dev, c["scores"], c["lmax"], edge_index=c["edge_index"])
    assert got.shape == (c["n"],) and np.array_equal(got, c["want"])


def test_big_case_equals_reference_twice(dev):
    """300 000 nodes on 17 score values: the multi-pass sort has to be stable under massive ties, call after call."""
    c = Z.case(*Z.BIG)
    first = _decode(dev, c["scores"], c["lmax"], edge_index=c["edge_index"])
    again = _decode(dev, c["scores"], c["lmax"], edge_index=c["edge_index"])
    assert np.array_equal(first, c["want"]) and np.array_equal(again, first)


@pytest.mark.parametrize("name", Z.FIXTURE_STRUCTURES)
def test_recorded_zoo_solution(dev, name):
    """The reference's own output on every structure (tests/golden/mis_decode_zoo.npz), not only our restatement of it."""
    n, ei, pred, sol = zoo_fixture(name)
    assert np.array_equal(_decode(dev, pred, edge_index=ei), sol)


@pytest.mark.parametrize("d,pos,kind", Z.STAR_PLACEMENTS)
def test_star_placement(dev, d, pos, kind):
    """The hub is OUT only because of entry ``pos`` of its list: lane 0, the last lane, the first and last lane of later strides."""
    n, ei, scores = Z.star_placement(d, pos, kind)
    want = Z.reference(scores, ei, n)
    assert want[0] == 0
    assert np.array_equal(_decode(dev, scores, Z.levels(scores, ei, n), edge_index=ei), want)


def test_the_long_path_walks_every_poll(dev):
    c = Z.case("path_1000", "increasing_id")
    assert c["lmax"] == 1000 and Z.round_bound(c["lmax"]) == 1000       # up to 250 polls of the undecided counter
    assert np.array_equal(_decode(dev, c["scores"], 1000, edge_index=c["edge_index"]), c["want"])
    assert c["want"].tolist() == [0, 1] * 500


FORMS = [("loops_all", "two_level"), ("sparse_4097", "with_nan"), ("edgeless_7", "all_zero")]


@pytest.mark.parametrize("pair", FORMS, ids=Z.case_id)
def test_entry_forms_agree(dev, pair):
    import scipy.sparse
    from difusco_amd.graph import build_csr
    c = Z.case(*pair)
    n, ei, s, want = c["n"], c["edge_index"], c["scores"], c["want"]
    adj = scipy.sparse.coo_matrix((np.ones(ei.shape[1], dtype=np.int64), (ei[0], ei[1])), shape=(n, n))
    graphs = {"host": dict(edge_index=ei), "device": dict(edge_index=ei, graph_build="device"),
              "tensor": dict(edge_index=torch.from_numpy(ei).to(dev), graph_build="device"),
              "graph": dict(graph=build_csr(torch.from_numpy(ei), n, dev)), "scipy": dict(adj_matrix=adj)}
    wide = np.stack([s, s[::-1]], axis=1)                                # [N, 2]: its first column is a strided [N, 1] view
    wide_t = torch.from_numpy(wide.copy()).to(dev)
    with np.errstate(invalid="ignore"):                                  # widening a signalling NaN raises the flag
        s64 = s.astype(np.float64)
    forms = {"float32": s, "float64": s64, "device tensor": torch.from_numpy(s).to(dev),
             "numpy [N, 1] view": wide[:, :1], "tensor [N, 1] view": wide_t[:, :1]}
    assert not wide[:, :1].flags["C_CONTIGUOUS"] or n == 1
    assert n == 1 or not wide_t[:, :1].is_contiguous()
    for gname, g in graphs.items():
        for fname, f in forms.items():
            assert np.array_equal(_decode(dev, f, c["lmax"], **g), want), (gname, fname)


def test_float64_scores_tie_by_id_after_the_cast(dev):
    c = Z.case("sparse_4095", "float64_collapsing")
    assert c["scores"].dtype == np.float64
    got = _decode(dev, c["scores"], c["lmax"], edge_index=c["edge_index"])
    assert np.array_equal(got, c["want"])
    assert np.array_equal(got, _decode(dev, c["scores"].astype(np.float32), c["lmax"], edge_index=c["edge_index"]))


def _solo_calls(dev, members, scores, off):
    return np.concatenate([_decode(dev, scores[off[g]:off[g + 1]], edge_index=ei) for g, (_, ei) in enumerate(members)])


@pytest.mark.parametrize("kind", ["two_level", "with_nan", "all_zero"])
def test_union_of_40_equals_solo_calls(dev, kind):
    c = Z.case("union_40", kind)
    n, ei, off = Z.union_of(Z.UNION_40)
    assert n == c["n"] and np.array_equal(ei, c["edge_index"])
    got = _decode(dev, c["scores"], c["lmax"], edge_index=ei)
    assert np.array_equal(got, c["want"]) and np.array_equal(got, _solo_calls(dev, Z.UNION_40, c["scores"], off))


def test_union_of_different_structures_equals_solo_calls(dev):
    members = [Z.STRUCTURES[s] for s in ("star_129_dec", "edgeless_7", "k_70", "loops_only", "one_node", "path_257")]
    n, ei, off = Z.union_of(members)
    for kind in ("two_level", "with_nan", "mixed_zero_signs"):
        scores = Z.make_scores(kind, n, seed=11)
        got = _decode(dev, scores, Z.levels(scores, ei, n), edge_index=ei)
        assert np.array_equal(got, Z.reference(scores, ei, n)), kind
        assert np.array_equal(got, _solo_calls(dev, members, scores, off)), kind


def test_argument_checks(dev):
    from difusco_amd import _lib
    from difusco_amd.graph import build_csr
    L = _lib.lib()
    c = Z.case("loops_all", "two_level")
    n = c["n"]
    g = build_csr(torch.from_numpy(c["edge_index"]), n, dev)
    d_sc = torch.from_numpy(c["scores"]).to(dev)
    d_sol = torch.full((n,), -7, dtype=torch.int32, device=dev)
    nbytes = ctypes.c_size_t()
    _lib.check(L.difusco_mis_decode_workspace_bytes(n, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    rounds = ctypes.c_int32(-1)
    args = [n, ctypes.c_void_p(g.rowptr.data_ptr()), ctypes.c_void_p(g.col.data_ptr()), ctypes.c_void_p(d_sc.data_ptr()),
            ctypes.c_void_p(d_sol.data_ptr()), ctypes.c_void_p(ws.data_ptr()), nbytes.value, ctypes.byref(rounds),
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)]
    short = list(args)
    short[6] = nbytes.value - 1                                          # one byte short: refused, both sizes named
    assert L.difusco_mis_decode(*short) == -1                            # DIFUSCO_EINVAL
    msg = L.difusco_last_error().decode()
    assert "workspace" in msg and str(nbytes.value - 1) in msg and str(nbytes.value) in msg
    for i, v in ((0, 0), (3, None), (1, None), (2, None), (4, None), (5, None)):      # n_nodes = 0, null scores, null others
        broken = list(args)
        broken[i] = v
        assert L.difusco_mis_decode(*broken) == -1, i
    assert rounds.value == -1 and d_sol.cpu().tolist() == [-7] * n      # nothing ran
    assert L.difusco_mis_decode_workspace_bytes(0, ctypes.byref(nbytes)) == -1
    assert L.difusco_mis_decode(*args) == 0 and rounds.value >= 4       # the same arguments, unbroken
    assert np.array_equal(d_sol.cpu().numpy(), c["want"])
    args[7] = None                                                       # rounds_out is optional
    assert L.difusco_mis_decode(*args) == 0
