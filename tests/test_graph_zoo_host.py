"""Host-side guard of tests/graph_zoo.py (no GPU): the zoo reaches every case of the neighbour-aggregation protocol, its graphs
are what the CSR builder makes of them, and the inputs of the layer tests are SENSITIVE enough - on the float64 reference alone -
that a kernel which loses one edge of a hub cannot pass tests/test_gpu_graph_structure.py."""
import numpy as np
import pytest
import torch

from tests import graph_zoo as Z


def test_zoo_reaches_every_protocol_case():
    reached = set()
    for name, deg in Z.ZOO.items():
        cases = Z.classify(deg)
        assert cases <= set(Z.ALL_CASES), (name, cases - set(Z.ALL_CASES))
        reached |= cases
    assert reached == set(Z.ALL_CASES), sorted(set(Z.ALL_CASES) - reached)


def test_classify_on_hand_checked_sequences():
    assert Z.classify([32]) == {"whole_tile/full", "start_row0", "end_row31", "empty_last", "E%32==0"}
    # E = 40: row 0 fills tile 0 and owns the first edge of the partial tile 1 (part0), row 1 sits inside it, row 2 owns its last edge
    c = Z.classify([35, 2, 3])
    assert {"whole_tile/full", "part0/partial", "direct/partial", "part1/partial", "start_row0", "empty_last"} <= c
    assert "start_group_boundary" not in c and "start_group_row7" not in c      # starts at rows 0, 3 and 5
    assert Z.classify([7, 1, 8]) >= {"start_group_row7", "start_group_boundary", "E<32"}      # starts at 0, 7, 8
    assert "tile_all_starts" in Z.classify([1] * 32) and "tile_all_starts" not in Z.classify([2] + [1] * 30)
    assert "spans_9_tiles" in Z.classify([1, 257]) and "spans_9_tiles" not in Z.classify([256])      # tiles 0..8 / 0..7
    assert Z.classify([0] * 5) == {"empty_first", "empty_last"}
    assert "E%256==0" in Z.classify([256]) and "E%32==0" not in Z.classify([256])


@pytest.mark.parametrize("name", list(Z.ZOO))
def test_from_degrees_round_trips_through_the_csr_builder(name):
    from difusco_amd import graph
    deg, ei = Z.zoo_graph(name)
    n, E = len(deg), int(sum(deg))
    assert ei.dtype == np.int64 and ei.shape == (2, E) and n >= max(deg)
    assert Z.classify(deg) == Z.classify(Z.ZOO[name])
    rowptr, col, row, perm, ident = graph.csr_from_coo_host(ei, n)
    assert np.array_equal(rowptr, Z.rowptr_of(deg))
    assert ident and np.array_equal(perm, np.arange(E)) and np.array_equal(col, ei[1]) and np.array_equal(row, ei[0])
    for i in np.flatnonzero(np.asarray(deg) > 0)[:50]:      # self first, neighbours distinct
        nb = col[rowptr[i]:rowptr[i + 1]]
        assert nb[0] == i and len(set(nb.tolist())) == len(nb)
    if E > 1:      # the caller's order shuffled: perm maps CSR slot -> caller index
        sh = np.random.default_rng(E).permutation(E)
        rowptr2, col2, row2, perm2, ident2 = graph.csr_from_coo_host(ei[:, sh], n)
        assert np.array_equal(rowptr2, rowptr) and np.array_equal(row2, row)
        assert np.array_equal(np.sort(perm2), np.arange(E))
        assert np.array_equal(ei[1][sh][perm2], col2) and np.array_equal(ei[0][sh][perm2], row2)
        assert ident2 == bool(np.array_equal(perm2, np.arange(E)))


def test_empty_row_insertion_keeps_every_csr_slot():
    for name in ("straddle", "hub_empties", "ones_95"):
        deg, ei = Z.zoo_graph(name)
        deg2, where = Z.with_empty_rows(deg)
        assert [deg2[w] for w in where] == deg and sum(deg2) == sum(deg) and len(deg2) > len(deg) + 5
        assert deg2[0] == 0 and deg2[-1] == 0
        assert np.array_equal(Z.rowptr_of(deg2)[where], Z.rowptr_of(deg)[:-1])


def _d32(inp, ei, agg, hub):
    t64 = Z.layer_reference(inp, ei, agg, 0, torch.float64)[1]
    t32 = Z.layer_reference(inp, ei, agg, 0, torch.float32)[1]
    return (t32.double() - t64)[hub].abs().max().item(), (t32.double() - t64).abs().max().item()


@pytest.mark.parametrize("name", Z.HUBS)
def test_sensitivity_of_the_marker_inputs(name):
    """Dropping ANY single edge of the hub from the float64 reference moves the hub's h row by more than SENSITIVITY x the bound
    that the GPU test asserts (project bound or 4 x d32, whichever is larger): in the phase whose block holds the edge, for sum,
    mean and max."""
    deg, ei = Z.zoo_graph(name)
    hub = Z.hub_of(deg)
    covered = np.zeros(deg[hub], dtype=bool)
    for phase in range(Z.n_phases(deg[hub])):
        lo, hi = Z.phase_block(deg[hub], phase)
        covered[lo:hi] = True
        inp = Z.layer_inputs(ei, len(deg), seed=Z.input_seed(), kind="marker", phase=phase)
        for agg in ("sum", "mean", "max"):
            change = Z.hub_drop_sensitivity(inp, ei, agg)[lo:hi].min().item()
            d32_hub, d32 = _d32(inp, ei, agg, hub)
            print(f"{name} marker phase {phase} {agg}: min change of the hub row {change:.2e}; d32 {d32:.2e} (hub row {d32_hub:.2e})")
            for engine, project in Z.H_BOUND.items():
                if engine == "fp16x1" and agg != "sum":
                    continue
                factor = Z.SENSITIVITY_BF16X3_BIG_HUBS if (engine == "bf16x3" and name != "hub256") else Z.SENSITIVITY
                assert change > factor * Z.calibrated(project, d32), (engine, agg, phase, change, d32)
    assert covered.all()
    # the shortcut of hub_drop_sensitivity against the full reference with the slot left out
    a = int(Z.rowptr_of(deg)[hub])
    full = Z.layer_reference(inp, ei, "max", 0)[1][hub]
    k = deg[hub] - 1
    direct = (Z.layer_reference(inp, ei, "max", 0, drop=a + k)[1][hub] - full).abs().max().item()
    assert abs(direct - Z.hub_drop_sensitivity(inp, ei, "max")[k].item()) < 1e-12


@pytest.mark.parametrize("name", ["hub_first", "hub_middle", "hub_last"])
def test_sensitivity_of_the_random_inputs_on_the_big_hubs(name):
    """Random inputs, sum: every single edge of a degree-1000 hub moves the row by > 100 x the bound of the default engine's kernel
    (fp16x3) and of the unfused kernel.  Mean does NOT reach it on these inputs (one edge of 1000 moves the row by 1.2e-3 .. 1.4e-3:
    60 x the unfused bound, 4 x the fp16x3 one; printed below): the marker inputs, whose hub has a zero U row so that LayerNorm
    removes the 1 / degree, carry mean (test above), and max, where a random edge usually owns no feature at all."""
    deg, ei = Z.zoo_graph(name)
    hub = Z.hub_of(deg)
    inp = Z.layer_inputs(ei, len(deg), seed=Z.input_seed(), kind="random")
    for agg, engines in (("sum", ("fp16x3", "unfused", "fp16x1")), ("mean", ())):
        change = Z.hub_drop_sensitivity(inp, ei, agg).min().item()
        d32_hub, d32 = _d32(inp, ei, agg, hub)
        print(f"{name} random {agg}: min change of the hub row {change:.2e}; d32 {d32:.2e} (hub row {d32_hub:.2e})")
        for engine in engines:
            assert change > Z.SENSITIVITY * Z.calibrated(Z.H_BOUND[engine], d32), (engine, agg, change, d32)
