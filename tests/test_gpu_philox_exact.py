"""The on-device random draws, bit for bit against a host Philox (tests/philox_reference.py, DESIGN.md "The random stream as a
contract").

Philox is an integer function, so nothing here has a tolerance except the float32 Box-Muller of (b), whose bound is derived:

(a) the uniform of the stand-alone categorical posterior kernel, with probabilities placed within one step of 2^-24 of the draw
    they are compared with (``u < p``, not ``u <= p``);
(b) the normal of the stand-alone Gaussian posterior kernel within the error of ``logf`` / ``sqrtf`` / ``cosf``;
(c) whole steps: a step that draws on the device returns the bits of the same step with the host numbers injected in caller
    order - through every head kernel (fused tiled, folds off, unfused at H = 64 / 128 / 256, dense segments, MIS node rows), both
    bindings and the prepared state;
(d) per-instance streams: instance b of a union draws ``(seeds[b], row - instance_rows[b])``, empty instances are skipped;
(e) the device offset shift carries into the high counter word;
(f) which offset every step of ``sample()`` / ``sample(graphed=True)`` / ``sample_batch()`` uses, as an absolute fact.

The injected path is what the golden fixtures and the oracle are compared with, so these equalities tie the default path to
them."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import philox_reference as P
from difusco_amd import _lib
from difusco_amd.graph import build_csr, build_union_csr, complete_graph_batch
from difusco_amd.schedules import CategoricalDiffusion, GaussianDiffusion, InferenceSchedule
from difusco_amd.synthetic import er_mis_edge_index, random_state_dict, tsp_instance

pytestmark = pytest.mark.gpu

# the third Random123 known-answer vector of philox4x32-10, read as (seed, offset): both high words set
KAT_SEED, KAT_OFFSET = 0x299f31d0a4093822, 0x0370734413198a2e
PAIRS = [(11, 0), (KAT_SEED, KAT_OFFSET)]
PAIR63 = ((1 << 63) - 59, (1 << 63) - 2)      # the widest key and offset both bindings carry (offset + 1 still fits)
STEP = 2.0 ** -24
N_ALONE = (1 << 16) + 37                      # stand-alone kernels: 257 blocks of 256, the last one partial


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _same(a, b, what=""):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and a.dtype == b.dtype, what
        assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} values differ, first at " \
                                  f"{(a != b).reshape(-1).nonzero()[:8].reshape(-1).tolist()}"


# ---- the two stand-alone kernels -------------------------------------------------------------------------------------------
def _device_normal(dev, n, seed, offset):
    """z[i] = philox_normal(seed, offset, i), fp32 on the device: x_s = a (x_t - b eps) + d z with a = d = 1, b = 0, x_t = 0
    (0 + 1 * z is exact)."""
    post = np.array([1, 0, 0, 1, 1, 0, 0, 0], dtype=np.float32)
    zero = torch.zeros(n, device=dev)
    out = torch.empty(n, device=dev)
    _lib.check(_lib.lib().difusco_gaussian_posterior(_p(zero), _p(zero), _fp(post), _lib.RAND_PHILOX, None, seed, offset,
                                                     _p(out), n, _stream()))
    torch.cuda.synchronize()
    return out


def _device_bernoulli(dev, logits, seed, offset):
    """(bits, prob) of the stand-alone categorical posterior with post = {0, 0, 1, 1, draw} and x_t = 0: prob = softmax(l)[1]."""
    n = logits.shape[0]
    post = np.array([0, 0, 1, 1, 1, 0, 0, 0], dtype=np.float32)
    lg = torch.from_numpy(logits).to(dev).contiguous()
    xt = torch.zeros(n, device=dev)
    out, prob = torch.empty(n, device=dev), torch.empty(n, device=dev)
    _lib.check(_lib.lib().difusco_categorical_posterior(_p(lg), _p(xt), _fp(post), _lib.RAND_PHILOX, None, seed, offset,
                                                        _p(out), _p(prob), n, _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), prob.cpu().numpy()


def _logits_at(u):
    """fp32 logits [n, 2] whose softmax puts p1 within about one step of 2^-24 of u."""
    q = np.clip(u.astype(np.float64), 1e-12, 1 - 1e-12)
    return np.stack([np.log1p(-q), np.log(q)], axis=1).astype(np.float32)


EDGE_PATTERNS = {"0": 0, "1": 1, "2^23 - 1": (1 << 23) - 1, "2^23 + 1": (1 << 23) + 1, "2^24 - 1": (1 << 24) - 1}


@pytest.mark.parametrize("seed,offset", [(11, 0), (11, 1), (KAT_SEED, KAT_OFFSET), (KAT_SEED, KAT_OFFSET + 1),
                                         (11, (1 << 32) - 1), (11, 1 << 32), (KAT_SEED, (1 << 32) - 1), (KAT_SEED, 1 << 32)])
def test_uniform_of_the_standalone_kernel_is_sharp_at_the_tie(dev, seed, offset):
    """Element i compares u = (w0 >> 8) 2^-24 of Philox(seed, offset, i) with its probability by ``u < p``.  The logits are chosen
    so that p lands within a step or two of 2^-24 of u itself: a draw from another word, other bits, another counter layout, or
    ``u <= p`` changes bits.  The edge patterns of u (0, 1, 2^23 +- 1, 2^24 - 1 in units of 2^-24) are looked for in the first
    2^20 indices of the stream; when one lies beyond the 2^16 + 37 elements, a second call reaches it."""
    wide = P.words(seed, offset, 1 << 20)[:, 0] >> np.uint32(8)
    found = {name: int(np.flatnonzero(wide == v)[0]) for name, v in EDGE_PATTERNS.items() if (wide == v).any()}
    print(f"stream ({seed:#x}, {offset:#x}): edge patterns found at {found}, not found in 2^20 indices: "
          f"{[k for k in EDGE_PATTERNS if k not in found]}")
    sizes = [N_ALONE] + ([max(found.values()) + 1] if found and max(found.values()) >= N_ALONE else [])
    np.testing.assert_array_equal(P.uniform(seed, offset, N_ALONE), (wide[:N_ALONE].astype(np.float64) * STEP).astype(np.float32))
    for n in sizes:
        u = (wide[:n].astype(np.float64) * STEP).astype(np.float32)
        out, prob = _device_bernoulli(dev, _logits_at(u), seed, offset)
        want = (u < np.clip(prob, 0.0, 1.0)).astype(np.float32)
        ones, near, ties = float((out == 1).mean()), float((np.abs(prob.astype(np.float64) - u) <= 2 * STEP).mean()), \
            int((prob == u).sum())
        print(f"  n {n}: out == 1 on {100 * ones:.1f} %, |prob - u| <= 2 steps on {100 * near:.2f} %, exact ties {ties}, "
              f"max |prob - u| {np.abs(prob.astype(np.float64) - u).max() / STEP:.2f} steps")
        np.testing.assert_array_equal(out, want)
        # not vacuous: both outcomes are frequent, the probabilities hug the draws, and exact ties (where < and <= part) occur
        assert ones >= 0.10 and 1 - ones >= 0.10
        assert near >= 0.95
        assert ties >= 1
        assert set(np.unique(out).tolist()) == {0.0, 1.0}


K_COS = K_LOG = 2.0      # ulp bounds of cosf / logf: no accuracy table ships with the toolchain here, so 2 ulp each is ASSUMED
R_MAX = math.sqrt(2 * 24 * math.log(2))      # the largest radius: u1 = 2^-24


def _normal_bound(z_ref):
    return R_MAX * K_COS * STEP + np.abs(z_ref) * (K_LOG / 2 + 1) * 2.0 ** -23


@pytest.mark.parametrize("seed,offset", PAIRS + [(11, 1), (KAT_SEED, (1 << 32) - 1), (KAT_SEED, 1 << 32)])
def test_normal_of_the_standalone_kernel_within_the_derived_bound(dev, seed, offset):
    """z_dev = fl(fl(sqrt(fl(-2 logf(u1)))) * cosf(arg)) against the float64 value z = r c, r = sqrt(-2 ln u1), c = cos(arg), on
    the SAME inputs (u1 exact in fp32; arg the one fp32 product float32(2 pi) * u2, restated in numpy float32).

    Bound.  logf(u1) = ln(u1) (1 + e_l), |e_l| <= k_log 2^-23 (k_log ulp, one ulp being at most 2^-23 relative); the product
    with -2 is exact; sqrtf rounds correctly: r_dev = r (1 + e_l)^(1/2) (1 + e_s), |e_s| <= 2^-24.  cosf(arg) = c + e_c with
    |e_c| <= k_cos 2^-24 (k_cos ulp of a value of magnitude at most 1).  The final product rounds once, |e_p| <= 2^-24.  To first
    order z_dev - z = z (e_l / 2 + e_s + e_p) + r e_c, so with r <= R = sqrt(2 * 24 ln 2) (u1 >= 2^-24)

        |z_dev - z| <= R k_cos 2^-24 + |z| (k_log / 2 + 1) 2^-23.

    k_cos = k_log = 2: the installed toolchain carries no accuracy table of the device math library, so 2 ulp each is an
    assumption (stated in DESIGN.md), not a measured value.  Observed on MI355X (printed below, recorded in DESIGN.md 5h): max
    error 4.40e-7 = 7.4 steps of 2^-24, at most 0.36 of the bound.

    The test checks itself: with the roles of the two words exchanged the reference is far outside the bound almost everywhere."""
    n = N_ALONE
    w = P.words(seed, offset, n)
    z_ref = P.normal_from_words(w[:, 0], w[:, 1])
    np.testing.assert_array_equal(z_ref, P.normal(seed, offset, n))
    z_dev = _device_normal(dev, n, seed, offset).cpu().numpy().astype(np.float64)
    assert np.isfinite(z_dev).all()
    err, bound = np.abs(z_dev - z_ref), _normal_bound(z_ref)
    worst = int(np.argmax(err / bound))
    print(f"stream ({seed:#x}, {offset:#x}): max |z_dev - z_ref| {err.max():.3e} ({err.max() / STEP:.2f} steps of 2^-24), "
          f"max error / bound {(err / bound).max():.3f} at element {worst} (z {z_ref[worst]:+.4f})")
    assert (err <= bound).all(), f"{int((err > bound).sum())} elements over the bound, worst ratio {(err / bound).max():.2f}"
    swapped = P.normal_from_words(w[:, 1], w[:, 0])
    far = np.abs(z_dev - swapped) > 100 * bound
    print(f"  words exchanged: {100 * far.mean():.2f} % of the elements are more than 100 bounds away")
    assert far.mean() > 0.9


# ---- whole steps -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(hidden, channels):
    return random_state_dict(hidden, 2, channels, seed=3)


@functools.lru_cache(maxsize=None)
def _post(diffusion):
    post = np.zeros(8, dtype=np.float32)
    if diffusion == _lib.CATEGORICAL:
        post[:4] = CategoricalDiffusion(T=1000, schedule="linear").posterior_constants(500, 450)
        post[4] = 1.0
    else:
        post[:5] = GaussianDiffusion(T=1000, schedule="linear").posterior_constants(500, 450, None)      # DDPM: draws a normal
    assert post[4] == 1.0
    return post


# name -> (hidden, precision, fused, flags)
ENGINES = {
    "fused-fp16x3": (256, "fp16x3", True, 0),
    "fused-fp16x3-folds-off": (256, "fp16x3", True, _lib.FLAG_NO_L0_FOLD | _lib.FLAG_NO_TAIL_FOLD),
    "fused-bf16x3": (256, "bf16x3", True, 0),
    "fused-bf16x3-folds-off": (256, "bf16x3", True, _lib.FLAG_NO_L0_FOLD | _lib.FLAG_NO_TAIL_FOLD),
    "unfused-h64": (64, "fp32", False, 0),
    "unfused-h128": (128, "fp32", False, 0),
    "unfused-h256": (256, "fp32", False, 0),
}
DIFFUSIONS = {"categorical": _lib.CATEGORICAL, "gaussian-ddpm": _lib.GAUSSIAN}


def _engine(dev, name, diffusion, backend="ctypes"):
    from difusco_amd.engine import DenoiseEngine
    hidden, precision, fused, flags = ENGINES[name]
    return DenoiseEngine(_weights(hidden, 2 if diffusion == _lib.CATEGORICAL else 1), device=dev, precision=precision,
                         fused=fused, backend=backend, flags=flags)


def _xt(rows, diffusion, dev, seed=5):
    x = torch.randn(rows, generator=torch.Generator().manual_seed(seed))
    return ((x > 0).float() if diffusion == _lib.CATEGORICAL else x).to(dev)


def _host_draws(dev, diffusion, rows, seed, offset, instances=None):
    """What the step keyed (seed, offset) must draw for caller rows 0 .. rows-1, as a device tensor: the host uniforms, or - the
    fp32 Box-Muller not being an integer function - the normals of the stand-alone kernel, which (b) holds to the host."""
    if instances is None:
        inst_rows, seeds = [0, rows], [seed]
    else:
        inst_rows, seeds = [int(v) for v in instances[0]], [int(v) for v in instances[1]]
        assert inst_rows[-1] == rows
    if diffusion == _lib.CATEGORICAL:
        return torch.from_numpy(P.instance_uniform(inst_rows, seeds, offset)).to(dev)
    parts = [_device_normal(dev, b1 - b0, s, offset) for b0, b1, s in zip(inst_rows, inst_rows[1:], seeds) if b1 > b0]
    return torch.cat(parts)


def _tables(dev, inst_rows, seeds):
    return (torch.as_tensor(np.asarray(inst_rows, dtype=np.int64)).to(dev), torch.tensor(seeds, dtype=torch.int64).to(dev))


def _assert_device_draws_equal_injected(eng, g, task, diffusion, xt, points, seed, offset, dev, prepared=None, instances=None,
                                        offset_shift=None, drawn_offset=None, what=""):
    """The step with on-device draws returns the bits of the step with the host numbers of (seed, ``drawn_offset``) injected,
    on x_t+1, the network output and the probability; and the draw is live: the step one offset later differs."""
    rows = xt.numel()
    kw = dict(points=points, xt_is_binary=diffusion == _lib.CATEGORICAL, want_pred=True, want_prob=True, prepared=prepared)
    tables = None if instances is None else _tables(dev, *instances)
    post = _post(diffusion)
    got = eng.step(g, task, diffusion, xt, 500.0, post, seed=seed, offset=offset, instances=tables, offset_shift=offset_shift, **kw)
    rand = _host_draws(dev, diffusion, rows, seed, offset if drawn_offset is None else drawn_offset, instances)
    assert rand.numel() == rows and rand.dtype == torch.float32
    want = eng.step(g, task, diffusion, xt, 500.0, post, rand=rand, seed=seed, offset=offset, instances=tables, **kw)
    for a, b, name in zip(got, want, ("xt_next", "pred", "prob")):
        _same(a, b, f"{what} (seed {seed:#x}, offset {offset:#x}) {name}")
    assert got[1] is not None and (got[2] is not None) == (diffusion == _lib.CATEGORICAL)
    later = eng.step(g, task, diffusion, xt, 500.0, post, seed=seed, offset=offset + 1, instances=tables,
                     offset_shift=offset_shift, **kw)
    assert not torch.equal(later[0], got[0]), f"{what}: the step does not depend on its offset"
    _same(later[1], got[1], f"{what} pred at the next offset")
    return got


def _tsp(dev, n, k, seed=4):
    p, ei = tsp_instance(n, k, seed=seed)
    pts, ei = torch.from_numpy(p), torch.from_numpy(ei)
    g = build_csr(ei, n, dev, points=pts)
    return g, pts.to(dev), ei.to(dev)


@pytest.mark.parametrize("n,k", [(37, 7), (150, 12)])
@pytest.mark.parametrize("diffusion", list(DIFFUSIONS))
@pytest.mark.parametrize("engine", list(ENGINES))
def test_tsp_step_draws_the_host_numbers(dev, engine, diffusion, n, k):
    """Sparse TSP: E = 259 is one padded 256-edge block plus 3 with a partial last 32-edge tile; the Morton node order makes
    ``perm`` a real permutation, so a draw keyed by the CSR slot instead of the caller row changes bits."""
    D = DIFFUSIONS[diffusion]
    g, pts, ei = _tsp(dev, n, k)
    assert g.n_edges == n * k
    if n == 37:
        assert g.perm is not None and not torch.equal(g.perm.cpu(), torch.arange(g.n_edges, dtype=torch.int32))
    eng = _engine(dev, engine, D)
    for seed, offset in PAIRS:
        _assert_device_draws_equal_injected(eng, g, _lib.TASK_TSP, D, _xt(g.n_edges, D, dev), pts, seed, offset, dev,
                                            what=f"{engine} {diffusion} N {n}")


@pytest.mark.parametrize("diffusion", list(DIFFUSIONS))
@pytest.mark.parametrize("engine", ["fused-fp16x3", "unfused-h256"])
def test_dense_batch_step_draws_the_host_numbers(dev, engine, diffusion):
    """Dense mode, B = 2 samples of V = 20: one statistic segment per sample (the ``seg_ptr`` route of both head kernels), rows
    b V V + i V + j in caller order."""
    D = DIFFUSIONS[diffusion]
    B, V = 2, 20
    g = complete_graph_batch(B, V, dev)
    assert g.n_segments == B and g.n_edges == B * V * V
    pts = torch.rand(B * V, 2, generator=torch.Generator().manual_seed(8)).to(dev)
    eng = _engine(dev, engine, D)
    for seed, offset in PAIRS:
        _assert_device_draws_equal_injected(eng, g, _lib.TASK_TSP, D, _xt(g.n_edges, D, dev), pts, seed, offset, dev,
                                            what=f"dense {engine} {diffusion}")


def _mis(dev, n, seed=6, p=0.12):
    ei = torch.from_numpy(er_mis_edge_index(n, p, seed=seed))
    return build_csr(ei, n, dev), ei.to(dev)


@pytest.mark.parametrize("diffusion", list(DIFFUSIONS))
@pytest.mark.parametrize("engine", ["fused-fp16x3", "unfused-h64"])
def test_mis_step_draws_the_host_numbers(dev, engine, diffusion):
    """MIS on an Erdos-Renyi graph (90 nodes, p = 0.12): node rows in caller order."""
    D = DIFFUSIONS[diffusion]
    g, _ = _mis(dev, 90)
    eng = _engine(dev, engine, D)
    for seed, offset in PAIRS:
        _assert_device_draws_equal_injected(eng, g, _lib.TASK_MIS, D, _xt(90, D, dev), None, seed, offset, dev,
                                            what=f"MIS {engine} {diffusion}")


@pytest.mark.parametrize("diffusion", list(DIFFUSIONS))
def test_step_through_the_custom_op_carries_63_bit_seed_and_offset(dev, diffusion):
    """The ``torch.ops.difusco`` binding passes seed and offset as signed 64-bit ints: the widest values must arrive whole."""
    D = DIFFUSIONS[diffusion]
    g, pts, _ = _tsp(dev, 37, 7)
    eng = _engine(dev, "fused-fp16x3", D, backend="torch")
    twin = _engine(dev, "fused-fp16x3", D, backend="ctypes")
    for seed, offset in PAIRS + [PAIR63]:
        got = _assert_device_draws_equal_injected(eng, g, _lib.TASK_TSP, D, _xt(g.n_edges, D, dev), pts, seed, offset, dev,
                                                  what=f"torch op {diffusion}")
        other = twin.step(g, _lib.TASK_TSP, D, _xt(g.n_edges, D, dev), 500.0, _post(D), points=pts,
                          xt_is_binary=D == _lib.CATEGORICAL, seed=seed, offset=offset, want_pred=True, want_prob=True)
        for a, b in zip(got, other):
            _same(a, b, "torch op against ctypes")


@pytest.mark.parametrize("diffusion", list(DIFFUSIONS))
def test_prepared_step_draws_the_host_numbers(dev, diffusion):
    D = DIFFUSIONS[diffusion]
    g, pts, _ = _tsp(dev, 37, 7)
    eng = _engine(dev, "fused-fp16x3", D)
    prepared = eng.prepare(g, pts)
    assert prepared is not None
    eng.prepare_times([500])
    for seed, offset in PAIRS:
        _assert_device_draws_equal_injected(eng, g, _lib.TASK_TSP, D, _xt(g.n_edges, D, dev), pts, seed, offset, dev,
                                            prepared=prepared, what=f"prepared {diffusion}")


# ---- per-instance streams --------------------------------------------------------------------------------------------------
INSTANCE_SEEDS = [KAT_SEED, (1 << 62) + 5, (0x7fffffff << 32) | 7]


def _tsp_union(dev, sizes, k=7):
    inst = [tsp_instance(n, k, seed=20 + i) for i, n in enumerate(sizes)]
    pts = [torch.from_numpy(p) for p, _ in inst]
    eis = [torch.from_numpy(e) for _, e in inst]
    g, _, rows = build_union_csr(eis, list(sizes), dev, points=torch.cat(pts))
    solo = [(build_csr(e, n, dev, points=p), p.to(dev)) for p, e, n in zip(pts, eis, sizes)]
    return g, torch.cat(pts).to(dev), [int(v) for v in rows], solo


def _mis_union(dev, sizes):
    eis = [torch.from_numpy(er_mis_edge_index(n, 0.12, seed=30 + i)) for i, n in enumerate(sizes)]
    g, _, rows = build_union_csr(eis, list(sizes), dev, task_rows="nodes")
    return g, None, [int(v) for v in rows], [(build_csr(e, n, dev), None) for e, n in zip(eis, sizes)]


@pytest.mark.parametrize("diffusion", list(DIFFUSIONS))
@pytest.mark.parametrize("task,engine", [("tsp", "fused-fp16x3"), ("tsp", "unfused-h64"), ("mis", "fused-fp16x3"),
                                         ("mis", "unfused-h64")])
def test_instances_of_a_union_draw_their_own_streams(dev, task, engine, diffusion):
    """Three instances with distinct keys: the union step equals the step injected with the concatenated host streams
    (instance b: key seeds[b], elements 0 .. rows_b - 1), and every instance's slice of x_t+1 equals its SOLO step fed
    ``uniform(seeds[b], offset, rows_b)``.  TSP 37 / 20 / 50 with K = 7 puts the boundaries at rows 259 and 399, both strictly
    inside a 32-row tile.  (The solo comparison is on x_t+1: logits of a union and a solo call agree to rounding only, their
    GroupNorm sums are taken in another order - test_gpu_batch_solve.py.)"""
    D = DIFFUSIONS[diffusion]
    if task == "tsp":
        g, pts, rows, solo = _tsp_union(dev, [37, 20, 50])
        assert rows == [0, 259, 399, 749] and all(r % 32 for r in rows[1:-1])
        tk = _lib.TASK_TSP
    else:
        g, pts, rows, solo = _mis_union(dev, [90, 41, 61])
        assert all(r % 32 for r in rows[1:-1])
        tk = _lib.TASK_MIS
    assert g.n_segments == 3
    eng = _engine(dev, engine, D)
    xt = _xt(rows[-1], D, dev)
    for offset in (0, KAT_OFFSET):
        got = _assert_device_draws_equal_injected(eng, g, tk, D, xt, pts, 99, offset, dev, instances=(rows, INSTANCE_SEEDS),
                                                  what=f"union {task} {engine} {diffusion}")
        if D == _lib.GAUSSIAN:
            # x_t+1 of a Gaussian step carries the prediction's rounding, so the solo comparison exposes the draw itself instead:
            # x_s = 0 + 1 * z (post = {1, 0, 0, 1, DDPM}, x_t = 0) of the union is each instance's stand-alone stream, exactly
            expose = np.array([1, 0, 0, 1, 1, 0, 0, 0], dtype=np.float32)
            z = eng.step(g, tk, D, torch.zeros(rows[-1], device=dev), 500.0, expose, points=pts, seed=99, offset=offset,
                         instances=_tables(dev, rows, INSTANCE_SEEDS))[0]
            _same(z, _host_draws(dev, D, rows[-1], 99, offset, (rows, INSTANCE_SEEDS)), "exposed normals of the union")
        for b, (gs, ps) in enumerate(solo):
            sl = slice(rows[b], rows[b + 1])
            rand = _host_draws(dev, D, rows[b + 1] - rows[b], INSTANCE_SEEDS[b], offset)
            if D == _lib.CATEGORICAL:
                alone = eng.step(gs, tk, D, xt[sl], 500.0, _post(D), points=ps, xt_is_binary=True, rand=rand)
                _same(got[0][sl], alone[0], f"instance {b} against its solo step")
            else:
                alone = eng.step(gs, tk, D, torch.zeros(rows[b + 1] - rows[b], device=dev), 500.0, expose, points=ps,
                                 seed=INSTANCE_SEEDS[b], offset=offset)
                _same(z[sl], alone[0], f"exposed normals of instance {b} against its solo step")
                _same(alone[0], rand, f"exposed normals of instance {b} against the stand-alone kernel")


@pytest.mark.parametrize("diffusion", list(DIFFUSIONS))
def test_an_empty_instance_between_two_others_is_skipped(dev, diffusion):
    """instance_rows = [0, 259, 259, 609]: no row belongs to the middle instance; rows 259.. draw the THIRD key from element 0.
    The Python layer accepts such tables (the C entry does), so the equality is what is asserted."""
    D = DIFFUSIONS[diffusion]
    g, pts, rows, _ = _tsp_union(dev, [37, 50])
    assert rows == [0, 259, 609]
    eng = _engine(dev, "fused-fp16x3", D)
    xt = _xt(609, D, dev)
    with_empty = ([0, 259, 259, 609], INSTANCE_SEEDS)
    got = _assert_device_draws_equal_injected(eng, g, _lib.TASK_TSP, D, xt, pts, 99, KAT_OFFSET, dev, instances=with_empty,
                                              what=f"empty middle instance {diffusion}")
    two = eng.step(g, _lib.TASK_TSP, D, xt, 500.0, _post(D), points=pts, xt_is_binary=D == _lib.CATEGORICAL, seed=99,
                   offset=KAT_OFFSET, instances=_tables(dev, rows, [INSTANCE_SEEDS[0], INSTANCE_SEEDS[2]]))
    _same(got[0], two[0], "the empty instance changes nothing")
    for lead in ([0, 0, 259, 609], [0, 259, 609, 609]):      # empty at the start / at the end
        seeds = [INSTANCE_SEEDS[1]] + [INSTANCE_SEEDS[0], INSTANCE_SEEDS[2]] if lead[1] == 0 else \
            [INSTANCE_SEEDS[0], INSTANCE_SEEDS[2], INSTANCE_SEEDS[1]]
        other = _assert_device_draws_equal_injected(eng, g, _lib.TASK_TSP, D, xt, pts, 99, KAT_OFFSET, dev,
                                                    instances=(lead, seeds), what=f"empty instance {lead}")
        _same(other[0], two[0], f"the empty instance of {lead} changes nothing")


@pytest.mark.parametrize("diffusion", list(DIFFUSIONS))
def test_one_instance_draws_the_stream_of_its_seed(dev, diffusion):
    D = DIFFUSIONS[diffusion]
    g, pts, _ = _tsp(dev, 37, 7)
    eng = _engine(dev, "fused-fp16x3", D)
    xt = _xt(259, D, dev)
    got = _assert_device_draws_equal_injected(eng, g, _lib.TASK_TSP, D, xt, pts, 99, KAT_OFFSET, dev,
                                              instances=([0, 259], [KAT_SEED]), what=f"one instance {diffusion}")
    plain = eng.step(g, _lib.TASK_TSP, D, xt, 500.0, _post(D), points=pts, xt_is_binary=D == _lib.CATEGORICAL, seed=KAT_SEED,
                     offset=KAT_OFFSET)
    _same(got[0], plain[0], "one instance against the call's own seed")


# ---- the device offset shift -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["ctypes", "torch"])
@pytest.mark.parametrize("diffusion", list(DIFFUSIONS))
def test_offset_shift_carries_into_the_high_word(dev, diffusion, backend):
    """offset 2^32 - 3 with a device shift of 5 draws the host stream of offset 2^32 + 2 (a sum taken in 32 bits would draw
    offset 2); the known-answer offset with shift 1 draws offset + 1."""
    D = DIFFUSIONS[diffusion]
    g, pts, _ = _tsp(dev, 37, 7)
    eng = _engine(dev, "fused-fp16x3", D, backend=backend)
    xt = _xt(259, D, dev)
    for seed, offset, shift in [(11, (1 << 32) - 3, 5), (KAT_SEED, (1 << 32) - 3, 5), (KAT_SEED, KAT_OFFSET, 1)]:
        sh = torch.tensor([shift], dtype=torch.int64, device=dev)
        _assert_device_draws_equal_injected(eng, g, _lib.TASK_TSP, D, xt, pts, seed, offset, dev, offset_shift=sh,
                                            drawn_offset=offset + shift, what=f"shift {shift} {diffusion} {backend}")


# ---- the offsets of the sampling loops -------------------------------------------------------------------------------------
STEPS = 6
LOOP_SEED = KAT_SEED


def _loop_args(hidden, sparse_factor):
    return dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=sparse_factor,
                n_layers=2, hidden_dim=hidden, inference_diffusion_steps=STEPS, inference_schedule="cosine")


LOOP_MODELS = {"unfused-h64": dict(hidden=64, precision="fp32", fused=False), "fused-h256": dict(hidden=256)}


def _loop_model(cls, dev, name, seed=LOOP_SEED, sparse_factor=7):
    kw = dict(LOOP_MODELS[name])
    hidden = kw.pop("hidden")
    return cls(_loop_args(hidden, sparse_factor), _weights(hidden, 2), device=dev, seed=seed, **kw)


def _hand_loop(step, x0, draws, first_offset):
    """The loop of ``sample()`` written out: step k injects ``draws(first_offset + k)`` at the schedule's own (t, target_t); the
    final map of the categorical loop follows."""
    sched = InferenceSchedule(inference_schedule="cosine", T=1000, inference_T=STEPS)
    xt = (x0 > 0).float()
    for k in range(STEPS):
        t1, t2 = sched(k)
        xt = step(xt, np.array([t1]).astype(int), np.array([t2]).astype(int), draws(first_offset + k))
    return xt + 1e-6


def _tsp_points(dev, n=37, k=7, seed=4):
    p, ei = tsp_instance(n, k, seed=seed)
    return torch.from_numpy(p).to(dev), torch.from_numpy(ei).to(dev)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
@pytest.mark.parametrize("name", list(LOOP_MODELS))
def test_tsp_sample_uses_offsets_0_1_2_and_continues(dev, name, graphed):
    """A fresh model: call c of ``sample()`` draws step k at offset 6 c + k of the model's seed - the eager loop, and the
    captured one on its capture call and its first two replays."""
    from difusco_amd import TSPModel
    m, twin = _loop_model(TSPModel, dev, name), _loop_model(TSPModel, dev, name, seed=1)      # (the twin's own seed is never used)
    pts, ei = _tsp_points(dev)
    E = ei.shape[1]
    x0 = torch.randn(E, generator=torch.Generator().manual_seed(2)).to(dev)
    step = lambda xt, t1, t2, u: twin.categorical_denoise_step(pts, xt, t1, dev, ei, target_t=t2, uniform=u)
    draws = lambda off: torch.from_numpy(P.uniform(LOOP_SEED, off, E)).to(dev)
    outs = []
    for call in range(3 if graphed else 2):
        got = m.sample(pts, ei, xt0=x0, graphed=graphed)
        _same(got, _hand_loop(step, x0, draws, STEPS * call), f"{name} sample() call {call}")
        outs.append(got)
    assert not torch.equal(outs[0], outs[1])
    if graphed:
        assert m.graph_captures == 1 and m.graph_replays == 2


def test_mis_sample_uses_offsets_0_1_2_and_continues(dev):
    from difusco_amd import MISModel
    m, twin = (_loop_model(MISModel, dev, "unfused-h64", seed=s, sparse_factor=-1) for s in (LOOP_SEED, 1))
    n = 90
    ei = torch.from_numpy(er_mis_edge_index(n, 0.12, seed=6)).to(dev)
    x0 = torch.randn(n, generator=torch.Generator().manual_seed(2)).to(dev)
    step = lambda xt, t1, t2, u: twin.categorical_denoise_step(xt, t1, dev, ei, target_t=t2, uniform=u)
    draws = lambda off: torch.from_numpy(P.uniform(LOOP_SEED, off, n)).to(dev)
    a = m.sample(n, ei, xt0=x0)
    _same(a, _hand_loop(step, x0, draws, 0), "MIS sample() call 0")
    b = m.sample(n, ei, xt0=x0)
    _same(b, _hand_loop(step, x0, draws, STEPS), "MIS sample() call 1")
    assert not torch.equal(a, b)


@pytest.mark.parametrize("name", list(LOOP_MODELS))
def test_sample_batch_uses_per_instance_streams_at_the_loop_offsets(dev, name):
    """``sample_batch`` on a fresh model (offsets = the call counter = 0 ..) and again with ``step_offset=0`` after the counter
    moved: both equal the written-out loop over the union that injects ``instance_uniform(rows, seeds, k)`` at step k."""
    from difusco_amd import TSPModel
    sizes = [37, 20, 50]
    m, twin = _loop_model(TSPModel, dev, name, seed=77), _loop_model(TSPModel, dev, name, seed=1)
    inst = [tsp_instance(n, 7, seed=20 + i) for i, n in enumerate(sizes)]
    pts = [torch.from_numpy(p).to(dev) for p, _ in inst]
    eis = [torch.from_numpy(e).to(dev) for _, e in inst]
    x0 = [torch.randn(e.shape[1], generator=torch.Generator().manual_seed(40 + b)).to(dev) for b, e in enumerate(eis)]
    g, _, rows = build_union_csr(eis, sizes, dev, points=torch.cat([p.cpu() for p in pts]))
    rows = [int(v) for v in rows]
    tables = twin._instance_tables(rows, INSTANCE_SEEDS)
    union_pts = torch.cat(pts)
    step = lambda xt, t1, t2, u: twin._categorical(g, _lib.TASK_TSP, union_pts, xt, t1, t2, u, False, instances=tables)
    draws = lambda off: torch.from_numpy(P.instance_uniform(rows, INSTANCE_SEEDS, off)).to(dev)
    want = _hand_loop(step, torch.cat(x0), draws, 0)
    first = m.sample_batch(pts, eis, seeds=INSTANCE_SEEDS, xt0=x0)
    again = m.sample_batch(pts, eis, seeds=INSTANCE_SEEDS, xt0=x0, step_offset=0)
    later = m.sample_batch(pts, eis, seeds=INSTANCE_SEEDS, xt0=x0)      # the counter: offsets 12 ..
    assert m.model.calls == 3 * STEPS
    for b in range(3):
        _same(first[b], want[rows[b]:rows[b + 1]], f"{name} sample_batch instance {b}")
        _same(again[b], want[rows[b]:rows[b + 1]], f"{name} sample_batch(step_offset=0) instance {b}")
    _same(torch.cat(later), _hand_loop(step, torch.cat(x0), draws, 2 * STEPS), f"{name} third sample_batch call")
    assert not torch.equal(torch.cat(later), want)
