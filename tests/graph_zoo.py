"""A zoo of graphs defined by DEGREE SEQUENCES, for the neighbour-aggregation protocol of the fused edge layer, and the float64
reference of one layer on them (a helper module like tests/fp16x1_emulation.py: no conftest, nothing collected from it).

The protocol (csrc/edge_layer_kernel.h "Neighbour sum", csrc/edge_layer.hip node_finalize_kernel): the CSR edge list is cut
into 32-edge tiles; inside a tile the edges of one centre node form a segment.  The kernel writes the first segment of a tile to
part[tile][0], the last one to part[tile][1] (to part[tile][0] when the tile holds a single segment) and the segments strictly
inside to direct[node]; node_finalize re-derives from rowptr alone where the pieces of a node are.  Where a row starts and ends
relative to the tiles decides every branch of both kernels, and a degree sequence in node order fixes exactly that: row i
occupies the CSR slots [cumsum(deg)[i-1], cumsum(deg)[i]).  ``classify`` restates node_finalize's arithmetic in numpy and names
the cases a sequence reaches; tests/test_graph_zoo_host.py asserts that the zoo reaches all of ``ALL_CASES``.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

TILE = 32

PLACES = ("whole_tile", "part0", "part1", "direct")
ALL_CASES = tuple(f"{p}/{k}" for p in PLACES for k in ("full", "partial")) + (
    "start_row0", "end_row31",                  # a segment that starts on tile row 0 / ends on tile row 31
    "start_group_boundary", "start_group_row7",  # a segment start on row 8, 16 or 24 of a tile / on row 7 of an 8-row group
    "tile_all_starts",                          # a full tile whose 31 inner rows all start a segment (32 nodes in one tile)
    "spans_9_tiles",                            # a node whose row touches >= 9 tiles (more than one workgroup of tiles)
    "empty_first", "empty_last", "empty_middle",
    "E%256==0", "E%32==0", "E<32")              # (E%32==0: a multiple of 32 that is not one of 256)


def padded(deg):
    """The degree sequence with empty rows appended so that every row can have ``deg`` DISTINCT neighbours (n >= max(deg))."""
    deg = [int(d) for d in deg]
    return deg + [0] * max(0, max(deg, default=0) - len(deg))


def from_degrees(deg, seed):
    """int64 [2, E]: rows in node order, row i = deg[i] distinct neighbours, itself first (ei[0] = centre node, ei[1] = neighbour);
    the node count is len(padded(deg))."""
    deg = padded(deg)
    n = len(deg)
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i, d in enumerate(deg):
        if d == 0:
            continue
        others = rng.choice(n - 1, size=d - 1, replace=False) if d > 1 else np.empty(0, dtype=np.int64)
        others = others + (others >= i)
        rows.append(np.full(d, i, dtype=np.int64))
        cols.append(np.concatenate([[i], others]).astype(np.int64))
    if not rows:
        return np.zeros((2, 0), dtype=np.int64)
    return np.stack([np.concatenate(rows), np.concatenate(cols)])


def rowptr_of(deg):
    return np.concatenate([[0], np.cumsum(np.asarray(deg, dtype=np.int64))])


def node_cases(rowptr, i, n_edges):
    """The protocol cases of row i - node_finalize_kernel's loop over the tiles of the row, case names instead of loads."""
    a, b = int(rowptr[i]), int(rowptr[i + 1])
    out = set()
    if b <= a:
        return out
    t0, t1 = a >> 5, (b - 1) >> 5
    for t in range(t0, t1 + 1):
        first = TILE * t
        last = min(first + TILE - 1, n_edges - 1)
        kind = "full" if last - first + 1 == TILE else "partial"
        if a <= first:
            place = "whole_tile" if b > last else "part0"      # (a single-segment tile writes part[tile][0] only)
        elif b > last:
            place = "part1"
        else:
            place = "direct"
        out.add(f"{place}/{kind}")
    if a % TILE == 0:
        out.add("start_row0")
    elif a % 8 == 0:
        out.add("start_group_boundary")
    if a % 8 == 7:
        out.add("start_group_row7")
    if b % TILE == 0:
        out.add("end_row31")
    if t1 - t0 + 1 >= 9:
        out.add("spans_9_tiles")
    return out


def classify(deg):
    """The set of protocol cases the (padded) degree sequence reaches."""
    deg = np.asarray(padded(deg), dtype=np.int64)
    rowptr = rowptr_of(deg)
    E = int(rowptr[-1])
    out = set()
    for i in range(len(deg)):
        out |= node_cases(rowptr, i, E)
    starts = np.zeros(E + 1, dtype=bool)
    starts[rowptr[:-1][deg > 0]] = True
    for t in range(E // TILE):
        if starts[TILE * t + 1:TILE * t + TILE].all():
            out.add("tile_all_starts")
    nz = np.flatnonzero(deg > 0)
    if len(deg) and deg[0] == 0:
        out.add("empty_first")
    if len(deg) and deg[-1] == 0:
        out.add("empty_last")
    if len(nz) and (deg[nz[0]:nz[-1] + 1] == 0).any():
        out.add("empty_middle")
    if E > 0 and E % 256 == 0:
        out.add("E%256==0")
    elif E > 0 and E % TILE == 0:
        out.add("E%32==0")
    if 0 < E < TILE:
        out.add("E<32")
    return out


def _zipf():
    rng = np.random.default_rng(20240607)
    d = np.minimum(rng.zipf(1.6, 400), 400)
    d[rng.random(400) < 0.15] = 0
    return [int(x) for x in d]


# name -> degree sequence (as written; from_degrees / classify pad it).  Remove none without tests/test_graph_zoo_host.py passing.
ZOO = {
    "ones_96": [1] * 96,
    "ones_95": [1] * 95,
    "aligned32_x16": [32] * 16,
    "aligned32_x8": [32] * 8,
    "groups_of_8": [8] * 37,
    "straddle": [16, 32, 16, 5, 40, 31, 1, 1, 31, 33, 63, 1, 1, 63, 9, 7, 7, 1, 24],
    "hub_first": [1000] + [1, 2, 3] * 100,
    "hub_middle": [1, 2, 3] * 50 + [1000] + [3, 2, 1] * 50 + [0] * 690,
    "hub_last": [2] * 1023 + [1021],                      # the hub ends in the partial last tile
    "hub_empties": [0, 0, 3, 700] + [0] * 40 + [1, 0, 2, 0, 0, 5] * 20 + [0] * 602,
    "tiny_1": [1, 0],
    "tiny_31": [31] + [0] * 31,
    "tiny_33": [20, 13] + [0] * 40,
    "zipf": _zipf(),
    "hub256": [3] * 40 + [256] + [2] * 300,               # one feature of the row maximum per hub edge (marker inputs)
    "no_edges": [0] * 40,
}
HUBS = ("hub256", "hub_first", "hub_middle", "hub_last", "hub_empties")      # the graphs that also run the marker inputs


def zoo_graph(name):
    """-> (padded degree list, edge_index int64 [2, E] numpy); the seed is a function of the name alone."""
    deg = padded(ZOO[name])
    return deg, from_degrees(deg, seed=sum(map(ord, name)))


def hub_of(deg):
    return int(np.argmax(np.asarray(deg)))


def with_empty_rows(deg):
    """-> (new degree list, old node -> new node): empty rows inserted before, between and after the rows of ``deg``; every edge
    keeps its CSR slot."""
    new, where = [0, 0], []
    for i, d in enumerate(deg):
        where.append(len(new))
        new.append(int(d))
        if i % 3 == 0:
            new.append(0)
        if i % 7 == 0:
            new += [0, 0]
    new += [0, 0, 0]
    return new, np.asarray(where, dtype=np.int64)


# ---- one layer: inputs and the plain torch reference ------------------------------------------------------------------------------
H = 256


def input_seed(hidden=H):
    """The seed of layer_inputs in the GPU module and in the host test's sensitivity conditions: the same inputs in both."""
    return 7 + hidden


def n_phases(deg_hub):
    return max(1, math.ceil(deg_hub / 256))


def phase_block(deg_hub, phase):
    """The hub edges [lo, hi) that carry the large marker in ``phase``: 256-edge blocks, the last one moved back so that it is
    full too (every feature then has one large marker in every phase); the blocks of all phases cover every edge."""
    lo = min(256 * phase, max(deg_hub - 256, 0))
    return lo, min(lo + 256, deg_hub)


def layer_inputs(ei, n, seed, kind="random", phase=0, hidden=H):
    """fp32 inputs of one layer on the graph ``ei`` (row-ordered).  ``random``: the inputs of test_gpu_parity.py::
    test_edge_layer_fused.  ``marker``: A, B rows and C e + b_C bounded by 0.3 in magnitude, so |e'| <= 0.9 and every gate lies in
    [0.29, 0.71]; V rows uniform in +-1; for the k-th edge of the hub (the row of largest degree) the V row of its neighbour gets
    +32 on feature (37 k) mod hidden - and +128 instead for the edges of the 256-edge block ``phase`` (phase_block),
    128 * 0.29 > 32 * 0.71 - so every edge of that block owns one feature of the hub's row maximum and dominates one feature of its sum.  The hub's U row is
    zero: LayerNorm then removes the 1 / degree of "mean" (up to its epsilon) and "mean" is as sensitive to one lost edge as "sum"."""
    g = torch.Generator().manual_seed(seed)
    E = ei.shape[1]
    Hd = hidden
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1      # noqa: E731
    d = dict(kind=kind, n=n, E=E, H=Hd)
    if kind == "random":
        d["node4"] = torch.randn(n, 4 * Hd, generator=g)
        d["e"] = torch.randn(E, Hd, generator=g) * 2.0
        d["h"] = torch.randn(n, Hd, generator=g)
        d["Wc"] = u(Hd, Hd) / 16 + torch.arange(Hd).float()[:, None] * 1e-4
        d["Wo"] = u(Hd, Hd) / 16 + torch.arange(Hd).float()[None, :] * 1e-4
        d["bc"], d["bo"] = torch.randn(Hd, generator=g) * 0.1, torch.randn(Hd, generator=g) * 0.1
    elif kind == "marker":
        node4 = torch.cat([u(n, Hd), u(n, Hd), u(n, Hd) * 0.3, u(n, Hd) * 0.3], dim=1)      # U | V | A | B
        deg = np.bincount(ei[0], minlength=n)
        hub = hub_of(deg)
        a = int(deg[:hub].sum())
        k = np.arange(int(deg[hub]))
        nb = torch.from_numpy(ei[1][a:a + len(k)]).long()
        lo, hi = phase_block(len(k), phase)
        amp = torch.where(torch.from_numpy((k >= lo) & (k < hi)), 128.0, 32.0)
        node4[nb, Hd + torch.from_numpy((37 * k) % Hd).long()] += amp
        node4[hub, :Hd] = 0.0
        d["node4"] = node4
        d["e"] = u(E, Hd)
        d["h"] = torch.randn(n, Hd, generator=g)
        d["Wc"] = u(Hd, Hd) * (0.25 / Hd)           # |C e| <= 0.25
        d["Wo"] = u(Hd, Hd) / 16 + torch.arange(Hd).float()[None, :] * 1e-4
        d["bc"], d["bo"] = u(Hd) * 0.05, torch.randn(Hd, generator=g) * 0.1      # |C e + b_C| <= 0.3
    else:
        raise ValueError(kind)
    d["prm"] = [1 + 0.1 * torch.randn(Hd, generator=g) if i % 2 == 0 else 0.1 * torch.randn(Hd, generator=g) for i in range(6)]
    d["tb"] = torch.randn(Hd, generator=g)
    # C e + b_C as an fp32 INPUT, for the unfused kernel (which starts behind GEMM 1)
    d["ce"] = (d["e"].double() @ d["Wc"].double().t() + d["bc"].double()).float()
    return d


AGGS = ("sum", "mean", "max")


def layer_reference_all(inp, ei, dtype=torch.float64, gemm=None, from_ce=False, drop=None, aggs=AGGS, toes=(0, 1)):
    """One layer in plain torch at ``dtype`` - the arithmetic written out in test_edge_layer_fused, oracle.segment_aggregate for the
    aggregation - for every (aggregation, time_on_edge) asked for: {(agg, toe): (e_out, h_out, act)}; act = SiLU(LN_o(..)) is what
    the unfused kernel leaves in place of C e.  gemm(x, w) replaces the two products (fp16x1 emulation); from_ce: start from the
    fp32 input C e + b_C (unfused kernel); drop: a CSR slot left out of the AGGREGATION only (the sensitivity conditions)."""
    from oracle import difusco_oracle as O
    n, Hd = inp["n"], inp["H"]
    c = lambda t: t.to(dtype)      # noqa: E731
    node4, e, h, tb = c(inp["node4"]), c(inp["e"]), c(inp["h"]), c(inp["tb"])
    prm = [c(t) for t in inp["prm"]]
    rowt, colt = torch.from_numpy(ei[0]).long(), torch.from_numpy(ei[1]).long()
    Uh, Vh, Ah, Bh = node4[:, :Hd], node4[:, Hd:2 * Hd], node4[:, 2 * Hd:3 * Hd], node4[:, 3 * Hd:]
    mm = gemm if gemm is not None else (lambda x, w: x @ c(w).t())
    ce = c(inp["ce"]) if from_ce else c(mm(e, inp["Wc"])) + c(inp["bc"])
    e1 = Ah[colt] + Bh[rowt] + ce
    msg = torch.sigmoid(e1) * Vh[colt]
    rows = rowt
    if drop is not None:
        keep = torch.ones(len(rowt), dtype=torch.bool)
        keep[drop] = False
        msg, rows = msg[keep], rowt[keep]
    hn = {a: F.relu(F.layer_norm(Uh + O.segment_aggregate(msg, rows, n, a), (Hd,), prm[0], prm[1], 1e-5)) for a in aggs}
    en0 = F.relu(F.layer_norm(e1, (Hd,), prm[2], prm[3], 1e-5))
    out = {}
    for toe in toes:
        en = en0 + tb if toe else en0
        act = F.silu(F.layer_norm(en, (Hd,), prm[4], prm[5], 1e-5))
        e_out = e + c(mm(act, inp["Wo"])) + c(inp["bo"])
        for a in aggs:
            out[(a, toe)] = (e_out, h + (hn[a] if toe else hn[a] + tb), act)
    return out


def layer_reference(inp, ei, aggregation, time_on_edge, dtype=torch.float64, **kw):
    return layer_reference_all(inp, ei, dtype, aggs=(aggregation,), toes=(time_on_edge,), **kw)[(aggregation, time_on_edge)]


def hub_drop_sensitivity(inp, ei, aggregation, edges=None):
    """For each hub edge k (all, or ``edges``): L_inf change of the hub's float64 h row when edge k is left out of the aggregation.
    Only the hub's row is evaluated (same formulas as layer_reference)."""
    Hd = inp["H"]
    deg = np.bincount(ei[0], minlength=inp["n"])
    hub = hub_of(deg)
    a, dg = int(deg[:hub].sum()), int(deg[hub])
    node4 = inp["node4"].double()
    col = torch.from_numpy(ei[1][a:a + dg]).long()
    e1 = node4[col, 2 * Hd:3 * Hd] + node4[hub, 3 * Hd:] + (inp["e"][a:a + dg].double() @ inp["Wc"].double().t() + inp["bc"].double())
    msg = torch.sigmoid(e1) * node4[col, Hd:2 * Hd]                    # [deg, H]
    if aggregation == "max":
        top = torch.topk(msg, 2, dim=0).values
        full = top[0]
        without = torch.where(msg == top[0], top[1].expand_as(msg), top[0].expand_as(msg))
    else:
        full = msg.sum(0)
        without = full - msg
        if aggregation == "mean":
            full, without = full / dg, without / (dg - 1)
    w, b = inp["prm"][0].double(), inp["prm"][1].double()
    f = lambda x: F.relu(F.layer_norm(node4[hub, :Hd] + x, (Hd,), w, b, 1e-5))      # noqa: E731
    change = (f(without) - f(full)).abs().max(dim=1).values
    return change if edges is None else change[edges]


# ---- the bounds of the layer tests (tests/test_gpu_graph_structure.py) and what the sensitivity conditions are held against ---------
# h bounds that the suite already asserts for one layer: test_gpu_parity.py::test_edge_layer_fused (10 x tol, |e| ~ 10),
# ::test_edge_gate_aggregate (2e-5), test_gpu_fp16x1.py::test_edge_layer_fused_fp16x1 (h 3e-5 against the emulated products)
H_BOUND = {"fp16x3": 3e-4, "bf16x3": 1e-3, "unfused": 2e-5, "fp16x1": 3e-5}
E_BOUND = {"fp16x3": 3e-4, "bf16x3": 1e-3, "unfused": 2e-5, "fp16x1": 5e-4}
SENSITIVITY = 100.0      # one lost hub edge must move the hub's float64 h row by more than this many bounds
# bf16x3 (not the default engine) carries the widest bound, 1e-3.  On hub256 the marker inputs reach 100 x that as well; on the
# degree-700 / -1000 hubs one edge of 1000 moves the row by 5.4e-2 or more, i.e. by 54 bounds at least: held to 50 there.
SENSITIVITY_BF16X3_BIG_HUBS = 50.0


def calibrated(project_bound, d32):
    """The round-6 rule (test_gpu_round6.py::test_default_engine_on_trained_like_weights): against float64 a kernel may sit at the
    project's bound or at 4 x the distance of a plain fp32 evaluation of the same layer from the float64 value."""
    return max(project_bound, 4.0 * d32)


def uses_calibrated_bound(deg, kind):
    """Marker inputs have another magnitude than the inputs the project bounds were set on, and the hubs sum up to 1000 terms."""
    return kind == "marker" or max(deg) >= 256
