"""Normalisation inputs whose MEAN dwarfs their SPREAD (a helper module like tests/graph_zoo.py: no conftest, nothing collected
from it).

Every other adversarial parameter set of the suite multiplies weights by a common factor, bends LayerNorm gains or makes entries
heavy-tailed; the ratio |mean| / sigma that a normalisation sees stays that of the random init, about 1.  ``offset_params`` adds a
constant c to ONE bias vector, which moves the mean of what a GroupNorm group / a LayerNorm row sees by a multiple of c and leaves
the spread alone.  A one-pass variance  E[x^2] - E[x]^2  loses about 2 log2(|mean| / sigma) bits; a two-pass or a pivoted one
does not.

The module holds (1) the parameter sets, (2) the inputs and the references (fp32 oracle, the same network in float64) of the
shapes that tests/test_gpu_offset_statistics.py runs, computed once per case and shared with tests/test_offset_statistics_host.py,
(3) numpy emulations of how the head's GroupNorm sums can be formed from the last layer's e - one-pass fp32 sums per 32-edge tile
(the arithmetic the fused last layer had before it subtracted a pivot), the pivoted fp32 sums it forms now, plain double sums -
and (4) the head evaluated in fp32 from given statistics.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import difusco_oracle as O

CLASS_TOL = 1e-5          # the default engine's class (tests/test_gpu_round6.py)
ORACLE_CAP = 1e-4         # a case stays in the list only while the fp32 oracle itself is this close to float64
MIN_RATIO = 40.0          # max |mean| / sigma over the 32 head groups that a case which reaches the head must show
OFFSETS = (16.0, 64.0, 256.0)      # (1024 breaks ORACLE_CAP on last_out_bias: 1.5e-4 - not in the list)
DEAD_GROUP = 5            # channels 40..47

TSP_KINDS = ("last_out_bias", "edge_embed_bias", "abc_bias", "node_embed_bias", "dead_group")
MIS_KINDS = ("last_time_bias", "node_embed_bias")
# the kinds whose offset arrives in the features the head normalises (abc_bias is removed by LN_e; on TSP node_embed_bias
# offsets h, which reaches e only through A h + B h and LN_e)
REACHES_HEAD = {"tsp": ("last_out_bias", "edge_embed_bias", "dead_group"), "mis": ("last_time_bias", "node_embed_bias")}

T_STEP, T_TARGET = 500, 469


def offset_params(p, kind, c, n_layers):
    """A copy of the oracle parameter dict ``p`` with the constant ``c`` added to one bias vector (``dead_group``: GroupNorm
    group 5 of the edge features made constant at c over the whole call)."""
    q = {k: v.clone() for k, v in p.items()}
    L = n_layers
    c = float(c)
    if kind == "last_out_bias":          # shifts only the final e: the TSP head statistics alone
        q[f"per_layer_out.{L - 1}.2.bias"] += c
    elif kind == "edge_embed_bias":      # rides the residual stream of e through every layer: C e on offset operands, LN_e, the head
        q["edge_embed.bias"] += c
    elif kind == "abc_bias":             # rows of e' = A h[j] + B h[i] + C e: mean 3c, spread ~1 - the LayerNorms
        for l in range(L):
            for m in "ABC":
                q[f"layers.{l}.{m}.bias"] += c
    elif kind == "node_embed_bias":      # offset node rows: the node linears, LN_h (MIS: the head as well)
        q["node_embed.bias"] += c
    elif kind == "last_time_bias":       # MIS: shifts the final h
        q[f"time_embed_layers.{L - 1}.1.bias"] += c
    elif kind == "dead_group":           # e[:, 40:48] == c exactly in every layer: the true variance of group 5 is 0
        ch = slice(8 * DEAD_GROUP, 8 * DEAD_GROUP + 8)
        q["edge_embed.weight"][ch] = 0.0
        q["edge_embed.bias"][ch] = c
        for l in range(L):
            q[f"per_layer_out.{l}.2.weight"][ch] = 0.0
            q[f"per_layer_out.{l}.2.bias"][ch] = 0.0
    else:
        raise ValueError(kind)
    return q


# ---- the shapes of the GPU tests ---------------------------------------------------------------------------------------------------
# name -> (task, hidden, layers, graph).  tsp60: 600 edges = 19 tiles, the last one 24 of 32; tsp150: 3,000 edges = 94 tiles (more
# than one workgroup of tiles per statistics block); h64 / h128: the row-major kernels at VEC 1 and 2; dense: 2 samples of 196
# rows, segments that are not tile aligned; mis: statistics over node rows.
SHAPES = {
    "tsp60": ("tsp", 256, 2, ("knn", 60, 10)),
    "tsp150": ("tsp", 256, 2, ("knn", 150, 20)),
    "tsp60_h64": ("tsp", 64, 3, ("knn", 60, 10)),
    "tsp60_h128": ("tsp", 128, 3, ("knn", 60, 10)),
    "dense": ("tsp", 256, 2, ("dense", 2, 14)),
    "mis": ("mis", 256, 2, ("er", 120, 0.12)),
}
# (seed 77 with one output channel and Gaussian x_t gives last_out_bias / c = 16 a ratio of 37, short of MIN_RATIO: 78 gives 42)
PARAM_SEED = {"categorical": 77, "gaussian": 78}

# Cases at which the fp32 ORACLE ITSELF leaves ORACLE_CAP (measured, fp32 oracle vs float64): removed from the list, not tolerated.
#   abc_bias, c = 256: 1.1e-4 (tsp60), 1.9e-4 (H = 64, H = 128) - the LayerNorm inputs have mean 768;
#   dead_group, c = 256: 2.0e-4 - the oracle's own fp32 GroupNorm leaves noise on the constant group, amplified by 1 / sqrt(eps);
#   dense, c = 64 / 256: 7.6e-4 / 1.7e-2 - the oracle's fp32 GroupNorm on a [B, H, V, V] tensor (c = 16: 4.9e-5, kept).
def offsets_for(shape, kind):
    if kind in ("abc_bias", "dead_group"):
        return OFFSETS[:2]
    if shape == "dense":
        return OFFSETS[:1]
    return OFFSETS


def _grid(shape, kinds, diffusions=("categorical",)):
    return [(shape, df, k, c) for df in diffusions for k in kinds for c in offsets_for(shape, k)]


# (shape, diffusion, kind, c) of every case that a GPU test runs; the host test checks each of them
GRID_TSP60 = _grid("tsp60", TSP_KINDS, ("categorical", "gaussian"))
GRID_TSP150 = _grid("tsp150", ("last_out_bias", "edge_embed_bias"))
GRID_NARROW = _grid("tsp60_h64", ("last_out_bias", "abc_bias")) + _grid("tsp60_h128", ("last_out_bias", "abc_bias"))
GRID_DENSE = _grid("dense", ("last_out_bias",))
GRID_MIS = _grid("mis", MIS_KINDS)
GRID_ALL = GRID_TSP60 + GRID_TSP150 + GRID_NARROW + GRID_DENSE + GRID_MIS


def case_id(case):
    shape, df, kind, c = case
    return f"{shape}-{df}-{kind}-{int(c)}"


@functools.lru_cache(maxsize=None)
def inputs(shape, diffusion="categorical"):
    """-> dict(points, ei, xt, u): CPU tensors; points / ei None where the shape has none.  Gaussian: real-valued x_t, no draw."""
    task, _, _, graph = SHAPES[shape]
    g = torch.Generator().manual_seed(17)
    d = dict(points=None, ei=None, u=None)
    if graph[0] == "knn":
        pts, ei = O.tsp_instance(graph[1], graph[2], seed=6)
        d["points"], d["ei"] = torch.from_numpy(pts), torch.from_numpy(ei)
        n_var = (ei.shape[1],)
    elif graph[0] == "dense":
        B, V = graph[1], graph[2]
        d["points"] = torch.rand(B, V, 2, generator=g)
        n_var = (B, V, V)
    else:
        d["ei"] = torch.from_numpy(O.er_mis_instance(graph[1], graph[2], seed=5))
        n_var = (graph[1],)
    x = torch.randn(n_var, generator=g)
    if diffusion == "categorical":
        d["xt"] = (x > 0).float()
        d["u"] = torch.rand(n_var, generator=g)
    else:
        d["xt"] = x
    return d


@functools.lru_cache(maxsize=None)
def params(shape, kind, c, diffusion="categorical"):
    _, H, L, _ = SHAPES[shape]
    base = O.init_params(H, L, 2 if diffusion == "categorical" else 1, seed=PARAM_SEED[diffusion])
    return base if kind is None else offset_params(base, kind, c, L)


def _dense_as_sparse(points, xt):
    """Sample b of a dense call is the complete graph on its V nodes, self loops included, row-major (i, j) (oracle.encoder_dense)."""
    B, V, _ = points.shape
    i, j = torch.meshgrid(torch.arange(V), torch.arange(V), indexing="ij")
    ei = torch.stack([i.reshape(-1), j.reshape(-1)])
    return [(points[b], xt[b].reshape(-1), ei) for b in range(B)]


@functools.lru_cache(maxsize=None)
def reference(shape, kind, c, diffusion="categorical"):
    """One denoising step of the case by the fp32 oracle and the network output in float64.  -> dict(x, out, prob, truth, feat):
    x the step's result, out the network output [rows, C] (dense: [B, V, V, C]), prob the posterior probability (categorical), truth
    the float64 network output in the shape of out, feat the fp32 oracle's features that the head normalises (None for dense).
    Shared by every test of the case: treat as read-only."""
    task, H, L, graph = SHAPES[shape]
    p = params(shape, kind, c, diffusion)
    d = inputs(shape, diffusion)
    tvec = torch.tensor([float(T_STEP)])
    r = dict(prob=None, feat=None)
    if task == "mis":
        r["x"], r["out"], r["prob"] = O.mis_categorical_denoise_step(p, O.CategoricalTables(), d["xt"], T_STEP, d["ei"], T_TARGET,
                                                                     uniform=d["u"], return_aux=True)
        r["truth"] = O.encoder_sparse_f64(p, None, d["xt"], tvec, d["ei"], node_feature_only=True)
        r["feat"] = O.encoder_sparse_node(p, d["xt"], tvec, d["ei"], return_features=True)[1]
        return r
    ei = d["ei"]      # None: dense
    if diffusion == "categorical":
        r["x"], out, r["prob"] = O.tsp_categorical_denoise_step(p, O.CategoricalTables(), d["points"], d["xt"], T_STEP, ei, T_TARGET,
                                                                uniform=d["u"], return_aux=True)
    else:
        r["x"], out = O.tsp_gaussian_denoise_step(p, O.GaussianTables(), d["points"], d["xt"], T_STEP, ei, T_TARGET, return_aux=True)[:2]
        out = out.reshape(-1, 1)
    if ei is None:
        r["out"] = out.permute(0, 2, 3, 1).contiguous()      # [B, C, V, V] -> [B, V, V, C]
        r["truth"] = torch.stack([O.encoder_sparse_f64(p, pts_b, xt_b, tvec, ei_b) for pts_b, xt_b, ei_b in
                                  _dense_as_sparse(d["points"], d["xt"])]).reshape(r["out"].shape)
    else:
        r["out"] = out
        r["truth"] = O.encoder_sparse_f64(p, d["points"], d["xt"], tvec, ei).reshape(out.shape)
        r["feat"] = O.encoder_sparse_edge(p, d["points"], d["xt"], tvec, ei, return_features=True)[2]
    return r


def distances(got, ref):
    """(HIP vs fp32 oracle, fp32 oracle vs float64, HIP vs float64), L_inf; ``got`` in any shape with the elements of ref['out']."""
    out, truth = ref["out"], ref["truth"]
    got = got.reshape(out.shape)
    return ((got - out).abs().max().item(), (out.double() - truth).abs().max().item(), (got.double() - truth).abs().max().item())


# ---- group statistics of a feature matrix [R, H] -----------------------------------------------------------------------------------
def group_moments_f64(feat):
    """Per GroupNorm group (H / 32 adjacent channels x all rows): (mean, biased variance) in float64, two-pass."""
    R, H = feat.shape
    x = feat.double().reshape(R, 32, H // 32).permute(1, 0, 2).reshape(32, -1)
    mean = x.mean(1)
    return mean.numpy(), ((x - mean[:, None]) ** 2).mean(1).numpy()


def mean_over_sigma(feat):
    """max over the 32 groups of |mean| / sigma (inf for a group of zero spread and non-zero mean)."""
    mean, var = group_moments_f64(feat)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(mean) / np.sqrt(var)
    return float(np.nanmax(r))


def _tiles(feat):
    """fp32 [E, 256] -> (x [T, 32 rows, 32 groups, 2 halves, 4], valid rows per tile [T]); pad rows hold 0 and are masked below."""
    E, H = feat.shape
    assert H == 256
    T = (E + 31) // 32
    x = np.zeros((T * 32, H), dtype=np.float32)
    x[:E] = feat.numpy()
    rows = np.minimum(32, E - 32 * np.arange(T)).astype(np.int64)
    return x.reshape(T, 32, 32, 2, 4), rows


def _wave_sum(v):
    """fp32 [T, 32 rows, 32 groups, 2 halves]: the per-lane partials of a tile summed as the fused kernel's epilogue does - a lane
    adds the 16 partials of rows 0..15 / 16..31 of one half one after the other, then two pairwise adds (rows, then halves)."""
    f = np.float32
    acc = np.zeros(v.shape[:1] + (2,) + v.shape[2:], dtype=f)      # [T, 2 row blocks, 32, 2]
    vb = v.reshape(v.shape[0], 2, 16, 32, 2)
    for k in range(16):
        acc = (acc + vb[:, :, k]).astype(f)
    tot = (acc[:, 0] + acc[:, 1]).astype(f)                        # lanes xor 16
    return (tot[..., 0] + tot[..., 1]).astype(f)                   # lanes xor 32


def _lane(x):
    """fp32 [..., 4]: (v0 + v1) + (v2 + v3) and the same of the squares, every operation rounded to fp32."""
    f = np.float32
    s = ((x[..., 0] + x[..., 1]).astype(f) + (x[..., 2] + x[..., 3]).astype(f)).astype(f)
    q = (x * x).astype(f)
    q = ((q[..., 0] + q[..., 1]).astype(f) + (q[..., 2] + q[..., 3]).astype(f)).astype(f)
    return s, q


def _moments(S, Q, n):
    mean = S / n
    return mean, np.maximum(Q / n - mean * mean, 0.0)


def moments_fp32_tile_sums(feat):
    """ONE-PASS fp32 sums per 32-edge tile (sum and sum of squares of the 256 values of a group), the tiles added in double,
    var = Q / n - mean^2 in double: the arithmetic of the fused last layer before it subtracted a pivot."""
    x, rows = _tiles(feat)
    s, q = _lane(x)
    mask = (np.arange(32)[None, :] < rows[:, None])[:, :, None, None]
    S = _wave_sum(np.where(mask, s, np.float32(0))).astype(np.float64).sum(0)
    Q = _wave_sum(np.where(mask, q, np.float32(0))).astype(np.float64).sum(0)
    return _moments(S, Q, 8.0 * feat.shape[0])


def moments_pivoted_tile_sums(feat):
    """What the fused last layer forms now: per tile and group the pivot p = the group's first channel on the tile's first edge,
    fp32 sums of d = x - p and of d^2 in the same order as above, recombined in double per tile
    (sum x = sum d + n p, sum x^2 = sum d^2 + 2 p sum d + n p^2 with n = 8 x the tile's valid rows), the tiles added in double."""
    x, rows = _tiles(feat)
    p = x[:, 0, :, 0, 0]                                            # [T, 32]
    d = (x - p[:, None, :, None, None]).astype(np.float32)
    s, q = _lane(d)
    mask = (np.arange(32)[None, :] < rows[:, None])[:, :, None, None]
    sd = _wave_sum(np.where(mask, s, np.float32(0))).astype(np.float64)
    qd = _wave_sum(np.where(mask, q, np.float32(0))).astype(np.float64)
    n = 8.0 * rows[:, None].astype(np.float64)
    pd = p.astype(np.float64)
    S = (sd + n * pd).sum(0)
    Q = (qd + 2.0 * pd * sd + n * pd * pd).sum(0)
    return _moments(S, Q, 8.0 * feat.shape[0])


def moments_double_sums(feat):
    """One-pass sums in double from the first element (gn_partial_kernel, gn_partial_tiled_kernel), var = Q / n - mean^2."""
    R, H = feat.shape
    x = feat.double().reshape(R, 32, H // 32).permute(1, 0, 2).reshape(32, -1).numpy()
    return _moments(x.sum(1), (x * x).sum(1), float(x.shape[1]))


def head_from_stats(p, feat, mean, var):
    """The head on fp32 features with GIVEN group statistics, in fp32 as the head kernels evaluate it: mean and
    rstd = 1 / sqrt(var + 1e-5) are rounded to fp32, then (x - mean) rstd gamma + beta, ReLU and the 1 x 1 convolution.
    -> [R, C] fp32."""
    R, H = feat.shape
    cpg = H // 32
    m = torch.from_numpy(np.asarray(mean, dtype=np.float64)).float().repeat_interleave(cpg)
    rstd = torch.from_numpy(1.0 / np.sqrt(np.asarray(var, dtype=np.float64) + 1e-5)).float().repeat_interleave(cpg)
    x = (feat.float() - m) * rstd * p["out.0.weight"] + p["out.0.bias"]
    return F.linear(F.relu(x), p["out.2.weight"].reshape(-1, H), p["out.2.bias"])
