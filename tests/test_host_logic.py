"""CPU-only tests of the host side: C-ABI library loads and exports what include/*.h declares, the
host CSR helper, weight packing, and the product's schedule / posterior constants against the oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from difusco_amd import _lib, graph, schedules, weights
from oracle import difusco_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "difusco_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    prof = re.search(r"#ifdef DIFUSCO_PROFILING(.*?)#endif", hdr, flags=re.S)
    prof_names = set(re.findall(r"\b(difusco_[a-z0-9_]+)\s*\(", prof.group(1)))
    hdr = hdr.replace(prof.group(0), "")
    names = set(re.findall(r"\b(difusco_[a-z0-9_]+)\s*\(", hdr))
    assert {"difusco_denoise_step", "difusco_linear_rows", "difusco_edge_gate_aggregate",
            "difusco_csr_from_coo_host", "difusco_weights_layout", "difusco_workspace_bytes"} <= names
    L = _lib.lib()
    for n in sorted(names):
        assert hasattr(L, n), f"{n} declared in include/difusco_hip.h but not exported"
    assert L.difusco_abi_version() == _lib.ABI_VERSION
    # the profiling knobs (process-wide state, timing-only kernel variants) live in libdifusco_hip_prof.so only
    assert prof_names == {"difusco_debug_set", "difusco_debug_set_ptr", "difusco_lab_gemm1", "difusco_lab_gemm1_nopk", "difusco_lab_reread_pass"}
    for n in prof_names:
        assert not hasattr(L, n), f"{n} must not be exported by the production library"


def test_profiling_library_loads():
    """libdifusco_hip_prof.so (timing-only kernel variants, stage-loop laboratory) must at least LOAD: an unresolved kernel stub
    only shows at dlopen time (round 4: an inline-asm "v" constraint made clang drop a whole kernel-template instantiation on
    the host pass without a diagnostic)."""
    from difusco_amd.build import PROF_LIB_PATH
    if not os.path.exists(PROF_LIB_PATH):
        pytest.skip("profiling library not built (python -m difusco_amd.build --prof)")
    P = ctypes.CDLL(PROF_LIB_PATH)
    for n in ("difusco_debug_set", "difusco_debug_set_ptr", "difusco_lab_gemm1", "difusco_denoise_step"):
        assert hasattr(P, n)


def test_step_args_abi_is_checked():
    a = _lib.StepArgs()
    a.struct_size = 8          # wrong on purpose
    a.abi_version = _lib.ABI_VERSION
    rc = _lib.lib().difusco_denoise_step(ctypes.byref(a))
    assert rc == -1 and b"ABI mismatch" in _lib.lib().difusco_last_error()
    with pytest.raises(_lib.DifuscoHipError):
        _lib.check(rc)


def test_rejects_unsupported_shapes():
    assert _lib.lib().difusco_weights_layout(100, 2, 2, None, 0, None) == -1
    assert _lib.lib().difusco_workspace_bytes(100, 2, 10, 10, 1) == 0


def test_csr_tsp_layout_is_identity():
    _, ei = O.tsp_instance(50, 7, seed=1)
    rowptr, col, row, perm, ident = graph.csr_from_coo_host(ei, 50)
    assert ident
    np.testing.assert_array_equal(rowptr, np.arange(51) * 7)
    np.testing.assert_array_equal(col, ei[1])
    np.testing.assert_array_equal(row, ei[0])
    np.testing.assert_array_equal(perm, np.arange(350))


def test_csr_unsorted_mis_and_empty_rows():
    ei = O.er_mis_instance(40, 0.2, seed=2)
    ei = ei[:, ei[0] != 7]              # node 7 gets no edges at all, not even its self loop
    rowptr, col, row, perm, ident = graph.csr_from_coo_host(ei, 40)
    assert not ident
    assert rowptr[7] == rowptr[8]
    assert (np.diff(row) >= 0).all()
    np.testing.assert_array_equal(ei[0][perm], row)
    np.testing.assert_array_equal(ei[1][perm], col)
    for i in range(40):                 # stable: caller order preserved inside a row
        assert (np.diff(perm[rowptr[i]:rowptr[i + 1]]) > 0).all()
    counts = np.bincount(ei[0], minlength=40)
    np.testing.assert_array_equal(np.diff(rowptr), counts)


def test_csr_rejects_out_of_range():
    ei = np.array([[0, 1, 5], [1, 0, 0]], dtype=np.int64)
    with pytest.raises(_lib.DifuscoHipError):
        graph.csr_from_coo_host(ei, 3)


def test_csr_empty_graph():
    rowptr, col, row, perm, ident = graph.csr_from_coo_host(np.zeros((2, 0), dtype=np.int64), 4)
    assert ident and (rowptr == 0).all() and col.shape == (0,)


@pytest.mark.parametrize("H,L,C", [(64, 2, 2), (256, 12, 2), (128, 3, 1)])
def test_weight_packing_roundtrip(H, L, C):
    p = O.init_params(H, L, C, seed=3)
    state = {"model." + k: v for k, v in p.items()}     # Lightning prefix must be accepted
    assert weights.infer_config(state) == (H, L, C)
    blob = weights.pack_state_dict(state)
    off, total = _lib.weights_layout(H, L, C)
    assert blob.numel() == total and all(o % 64 == 0 for o in off)
    assert sorted(off) == off

    def view(idx, shape):
        n = int(np.prod(shape))
        return blob[off[idx]: off[idx] + n].reshape(shape)

    for i, name in enumerate(_lib.W_GLOBAL):
        if not name.startswith("@"):
            torch.testing.assert_close(view(i, p[name].reshape(-1).shape), p[name].reshape(-1), rtol=0, atol=0)
    for l in range(L):
        base = len(_lib.W_GLOBAL) + l * len(_lib.W_LAYER)
        n4 = view(base + 0, (4 * H, H))
        for q, m in enumerate("UVAB"):
            torch.testing.assert_close(n4[q * H:(q + 1) * H], p[f"layers.{l}.{m}.weight"], rtol=0, atol=0)
        torch.testing.assert_close(view(base + 12, (H, H)), p[f"per_layer_out.{l}.2.weight"], rtol=0, atol=0)
    # constant tables are the very expressions of the reference forward pass
    half = H // 2
    torch.testing.assert_close(view(12, (half,)),
                               torch.exp(-np.log(10000) * torch.arange(half, dtype=torch.float32) / half), rtol=0, atol=0)
    torch.testing.assert_close(view(13, (half,)), O._dim_t(half), rtol=0, atol=0)
    torch.testing.assert_close(view(14, (H,)), O._dim_t(H), rtol=0, atol=0)


def test_schedules_match_oracle_and_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "schedules.npz"))
    for kind in ("linear", "cosine"):
        c, g = schedules.CategoricalDiffusion(1000, kind), schedules.GaussianDiffusion(1000, kind)
        np.testing.assert_array_equal(c.Q_bar, z[f"Q_bar_{kind}"])
        np.testing.assert_array_equal(g.alphabar, z[f"alphabar_{kind}"])
        for S in (50, 7, 1000):
            s = schedules.InferenceSchedule(kind, T=1000, inference_T=S)
            np.testing.assert_array_equal(np.array([s(i) for i in range(S)]), z[f"sched_{kind}_{S}"])
    with pytest.raises(ValueError):
        schedules.InferenceSchedule("nope")(0)


def _emulate_categorical_kernel(post, logits, xt):
    """fp32 arithmetic of categorical_step() in graph_kernels.hip (softmax over 2 + c0*p0 + c1*p1)."""
    l = logits.astype(np.float32)
    m = np.maximum(l[:, 0], l[:, 1])
    e0, e1 = np.exp(l[:, 0] - m, dtype=np.float32), np.exp(l[:, 1] - m, dtype=np.float32)
    den = e0 + e1
    p0, p1 = e0 / den, e1 / den
    b = (xt > 0.5).astype(int)
    return (post[b] * p0).astype(np.float32) + (post[2 + b] * p1).astype(np.float32)


def test_categorical_posterior_constants_reproduce_reference_formula(golden_dir):
    """The 4-scalar closed form must equal the reference's matmul/one-hot formulation; checked against
    the golden probabilities recorded from the reference itself."""
    z = np.load(os.path.join(golden_dir, "posteriors.npz"))
    diff = schedules.CategoricalDiffusion(1000, "linear")
    for i in range(6):
        t, tt = (int(v) for v in z[f"cat{i}_t"])
        tt = t - 1 if tt < 0 else tt
        post = diff.posterior_constants(t, tt)
        x0 = z[f"cat{i}_x0"].reshape(-1, 2)
        xt = z[f"cat{i}_xt"].reshape(-1)
        b = (xt > 0.5).astype(int)
        prob = (post[b] * x0[:, 0]).astype(np.float32) + (post[2 + b] * x0[:, 1]).astype(np.float32)
        ref = z[f"cat{i}_prob"].reshape(-1) if f"cat{i}_prob" in z.files else z[f"cat{i}_out"].reshape(-1)
        np.testing.assert_allclose(prob, ref, rtol=0, atol=6e-8)
        # and through a softmax like the kernel does
        logits = np.log(x0)
        np.testing.assert_allclose(_emulate_categorical_kernel(post, logits, xt), ref, rtol=0, atol=3e-7)


def test_gaussian_posterior_constants(golden_dir):
    z = np.load(os.path.join(golden_dir, "posteriors.npz"))
    diff = schedules.GaussianDiffusion(1000, "linear")
    for i in range(5):
        t, tt = (int(v) for v in z[f"gau{i}_t"])
        trick = "ddim" if int(z[f"gau{i}_trick"]) else None
        a, b, c, d, branch = diff.posterior_constants(t, tt, trick)
        pred, xt = z[f"gau{i}_pred"], z[f"gau{i}_xt"]
        base = a * (xt - b * pred)
        if branch == 0:
            out = base + c * pred
        else:
            out = base + d * z[f"gau{i}_noise"]
        np.testing.assert_allclose(out.astype(np.float32), z[f"gau{i}_out"], rtol=0, atol=2e-7)
    with pytest.raises(ValueError):
        diff.posterior_constants(10, 5, "bogus")


def test_complete_graph_batch_matches_dense_flattening():
    g = graph.complete_graph_batch(2, 3, "cpu")
    assert g.n_nodes == 6 and g.n_edges == 18 and g.n_segments == 2
    np.testing.assert_array_equal(g.rowptr.numpy(), np.arange(7) * 3)
    np.testing.assert_array_equal(g.col.numpy(), [0, 1, 2] * 3 + [3, 4, 5] * 3)
    np.testing.assert_array_equal(g.seg_ptr.numpy(), [0, 9, 18])


def test_engine_refuses_cpu_device():
    from difusco_amd.engine import DenoiseEngine
    with pytest.raises(_lib.DifuscoHipError):
        DenoiseEngine(O.init_params(64, 1, 2, 0), device="cpu")


def _emulated_split_gemm(x, w, n_planes):
    """CPU emulation of linear_rows_split_kernel's arithmetic: operands decomposed into bf16 planes
    (RNE), every bf16 x bf16 product exact, accumulation in fp32 (here fp64 of exactly representable
    products - an upper bound on the kernel's accuracy, the kernel adds fp32 accumulation rounding)."""
    def planes(t):
        out, rest = [], t.clone()
        for _ in range(n_planes):
            p = rest.to(torch.bfloat16).float()
            rest = rest - p
            out.append(p.double())
        return out
    xp, wp = planes(x), planes(w)
    pairs = [(0, 0), (0, 1), (1, 0)] if n_planes == 2 else [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]
    return sum(xp[a] @ wp[b].t() for a, b in pairs)


def test_split_precision_error_model():
    """bf16x3 (2 planes / 3 products) vs bf16x6 (3 planes / 6 products) against fp64: documents why
    bf16x6 is 'fp32-class' (dropped terms <= 2^-24) while bf16x3 sits near 2^-17 per product."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(512, 256, generator=g)
    w = (torch.rand(256, 256, generator=g) * 2 - 1) / 16
    ref = x.double() @ w.double().t()
    scale = ref.abs().max().item()
    e3 = (_emulated_split_gemm(x, w, 2) - ref).abs().max().item() / scale
    e6 = (_emulated_split_gemm(x, w, 3) - ref).abs().max().item() / scale
    e32 = ((x @ w.t()).double() - ref).abs().max().item() / scale
    assert e6 < 2e-7 and e6 <= e32 * 2       # at least as good as an fp32 GEMM
    assert 1e-7 < e3 < 2e-5


def _emulated_fp16x3_gemm(x, w, scaled):
    """fp64 emulation of the fp16x3 path: two fp16 planes per operand, products hi*hi + hi*lo + lo*hi.  scaled: the
    power-of-two operand scaling of the product path (weights per matrix, x per row: weights.pow2_scale)."""
    def planes(t):
        hi = t.to(torch.float16)
        lo = (t - hi.float()).to(torch.float16)
        return hi.double(), lo.double()
    sw = weights.pow2_scale(w.abs().amax().reshape(1, 1)) if scaled else torch.ones(1, 1)
    sx = weights.pow2_scale(x.abs().amax(dim=1, keepdim=True)) if scaled else torch.ones(x.shape[0], 1)
    (xh, xl), (wh, wl) = planes(x * sx), planes(w * sw)
    acc = xh @ wh.t() + xh @ wl.t() + xl @ wh.t()
    return acc / (sx.double() * sw.double())


@pytest.mark.parametrize("wexp", [5, 0, -6, -10, -13, -20])
@pytest.mark.parametrize("xexp", [8, 0, -8])
def test_fp16x3_error_model_is_scale_invariant(wexp, xexp):
    """The two-plane fp16 split keeps ~22 significand bits only while the low plane is a NORMAL fp16 number: unscaled,
    |w| <= 2^-4 (the default initialisation!) already has a subnormal low plane and the error grows as the operands
    shrink (an absolute 2^-25 floor per element).  With the power-of-two pre-scaling of weights.split_planes / the
    kernels the relative error is the same at every operand scale, and at fp32-GEMM level."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(256, 256, generator=g) * 2.0 ** xexp
    w = (torch.rand(256, 256, generator=g) * 2 - 1) * 2.0 ** wexp
    ref = x.double() @ w.double().t()
    scale = ref.abs().max().item()
    e_scaled = (_emulated_fp16x3_gemm(x, w, True) - ref).abs().max().item() / scale
    e_fp32 = ((x @ w.t()).double() - ref).abs().max().item() / scale
    assert e_scaled < 3e-7, e_scaled                 # observed 4-9e-8 at every scale
    assert e_scaled < 2 * e_fp32 + 1e-7
    if max(abs(wexp), abs(xexp)) < 12 and wexp + xexp > -20:     # (the unscaled split overflows / flushes beyond)
        e_raw = (_emulated_fp16x3_gemm(x, w, False) - ref).abs().max().item() / scale
        if wexp <= -10 or xexp <= -8:
            assert e_raw > 20 * e_scaled, (e_raw, e_scaled)      # what round 2 shipped: not scale invariant


def test_split_planes_layout_and_exactness():
    g = torch.Generator().manual_seed(1)
    for wscale, per_row in [(1.0, False), (2.0 ** -11, False), (2.0 ** 7, True)]:
        w = torch.randn(64, 64, generator=g) * wscale
        if per_row:
            w = w * (2.0 ** torch.arange(-32, 32).float())[:, None]       # rows 2^64 apart in magnitude
        flat = weights.split_planes(w, per_row=per_row)
        assert flat.dtype == torch.float32 and flat.numel() == 5 * 64 * 64 // 2 + 64
        inv_scale = weights.plane_scale_inv(flat, 64, 64)
        raw = flat[: 5 * 64 * 64 // 2].view(torch.int16).reshape(5, 64 // 16, 64, 4, 4)   # [plane][slab][row][pos group][4]
        inv = [0, 2, 1, 3]                                                 # the permutation is an involution
        nat = raw[:, :, :, inv, :].permute(0, 2, 1, 3, 4).reshape(5, 64, 64)   # back to [plane][row][k]
        bf = nat[:3].view(torch.bfloat16).float()
        fp = nat[3:].view(torch.float16).float()
        assert (bf.sum(0) - w).abs().max().item() <= 2 ** -23 * w.abs().max().item()     # 24 bits recovered
        assert torch.equal(bf[0], w.to(torch.bfloat16).float())
        # fp16 planes: those of the scaled matrix, scale a power of two, largest scaled magnitude in [2^14, 2^15)
        ws = w / inv_scale[:, None]
        assert torch.equal(torch.frexp(inv_scale)[0], torch.full((64,), 0.5))
        top = ws.abs().amax(dim=1) if per_row else ws.abs().amax().expand(64)
        assert ((top >= 2.0 ** 14) & (top < 2.0 ** 15)).all()
        assert torch.equal(fp[0], ws.to(torch.float16).float())
        grp = w.abs().amax(dim=1, keepdim=True) if per_row else w.abs().max()
        assert ((fp.sum(0) * inv_scale[:, None] - w).abs() <= 2.0 ** -21 * w.abs() + 2.0 ** -38 * grp).all()   # 22 bits


def test_fused_scales_record():
    g = torch.Generator().manual_seed(2)
    wc, wo = torch.randn(256, 256, generator=g) * 1e-3, torch.randn(256, 256, generator=g) * 30
    for gmax, bmax in [(1.0, 0.0), (1e-4, 1e-5), (37.0, 5.0)]:
        go, bo = torch.rand(256, generator=g) * gmax, (torch.rand(256, generator=g) - 0.5) * 2 * bmax
        rec = weights.fused_scales(wc, wo, go, bo)
        # {log2(e) 2^-kc, 2^-(ko+ka) / log2(e), log2(e), 2^-ka} (include/difusco_hip.h, ABI 11: the fused kernel's log2(e) domain)
        c = np.float32(weights.LOG2E)
        inv_c_c, inv_o_a_c, gmul, s_den = (np.float32(v) for v in rec[:4])
        assert gmul == c
        inv_c = float(inv_c_c / c)
        assert inv_c == 2.0 ** round(np.log2(inv_c)) and 2.0 ** 14 <= wc.abs().max().item() / inv_c < 2.0 ** 15
        sa = 1.0 / float(s_den)
        assert sa == 2.0 ** round(np.log2(sa))
        bound = max(16 * go.abs().max().item() + bo.abs().max().item(), 0.2785) * float(c)
        assert 2.0 ** 14 <= bound * sa < 2.0 ** 15          # |a| log2(e) 2^ka stays below the fp16 maximum
        inv_o = float(inv_o_a_c) * sa * float(c)
        assert abs(inv_o / 2.0 ** round(np.log2(inv_o)) - 1.0) < 2e-7 and 2.0 ** 14 <= wo.abs().max().item() / inv_o < 2.0 ** 15.001
        assert (rec[4:] == 0).all()


def test_knn_generator_matches_sklearn_fixture(golden_dir):
    """The host-side k-NN generator (difusco_amd/synthetic.py, used for synthetic inputs and as the checker of the
    GPU k-NN kernel) against sklearn KDTree outputs (tests/golden/make_golden_knn.py)."""
    import glob
    from difusco_amd.synthetic import knn_edge_index
    paths = sorted(glob.glob(os.path.join(golden_dir, "knn_*.npz")))
    assert len(paths) >= 4
    for p in paths:
        z = np.load(p)
        k = int(z["k"])
        ei = knn_edge_index(z["points"], k)
        n = z["points"].shape[0]
        assert np.array_equal(ei[0], np.repeat(np.arange(n), k))
        assert np.array_equal(ei[1].reshape(n, k), z["idx_knn"])


def test_mcts_heatmap_text_matches_reference(golden_dir, tmp_path):
    """difusco_amd.formats against the text the reference's convert_numpy_to_txt.py produced (make_golden_formats.py)."""
    import glob
    from difusco_amd import formats
    paths = sorted(glob.glob(os.path.join(golden_dir, "mcts_text_*.npz")))
    assert len(paths) >= 2
    for p in paths:
        z = np.load(p)
        n, prob = int(z["num_nodes"]), float(z["expected_valid_prob"])
        text = formats.mcts_heatmap_text(z["heat"], z["points"], n, prob)
        assert text == bytes(z["text"]).decode()
        out = formats.write_mcts_heatmap(z["heat"], z["points"], n, str(tmp_path), 0, expected_valid_prob=prob, use_gpu=False)
        assert out.endswith(f"heatmap/tsp{n}/heatmaptsp{n}_0.txt") and open(out).read() == text
    hp, pp = formats.save_numpy_heatmap(z["heat"], z["points"], str(tmp_path), 3)
    assert hp.endswith("numpy_heatmap/test-heatmap-3.npy") and np.array_equal(np.load(hp), z["heat"])
    ei = np.array([[0, 1, 2], [1, 2, 0]])
    d = formats.densify(np.array([0.5, 0.25, 1.0]), ei, 3)
    assert d[0, 1] == 0.5 and d[2, 0] == 1.0 and d.sum() == 1.75


def test_step_argument_validation_without_gpu():
    """difusco_denoise_step validates its argument block before any HIP call: every malformed block comes back as
    DIFUSCO_EINVAL with a message (the reference raises Python exceptions; the binding turns codes into exceptions)."""
    import ctypes
    from difusco_amd import _lib
    L = _lib.lib()

    def make(**kw):
        a = _lib.StepArgs()
        a.struct_size, a.abi_version = ctypes.sizeof(_lib.StepArgs), _lib.ABI_VERSION
        a.hidden, a.n_layers, a.out_channels, a.task = 256, 12, 2, _lib.TASK_TSP
        a.diffusion, a.n_nodes, a.n_edges, a.n_segments = _lib.CATEGORICAL, 10, 20, 1
        for name in ("weights", "rowptr", "col", "xt", "xt_out", "workspace", "points"):
            setattr(a, name, 0x1000)            # never dereferenced: validation fails first
        a.precision = _lib.PRECISIONS["fp16x3"]
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def expect_einval(a, fragment):
        rc = L.difusco_denoise_step(ctypes.byref(a))
        assert rc < 0, fragment
        assert fragment in L.difusco_last_error().decode(), L.difusco_last_error().decode()

    assert L.difusco_denoise_step(None) < 0
    expect_einval(make(struct_size=8), "ABI mismatch")
    expect_einval(make(abi_version=_lib.ABI_VERSION - 1), "ABI mismatch")
    expect_einval(make(hidden=100), "hidden must be")
    expect_einval(make(n_layers=0), "n_layers")
    expect_einval(make(task=7), "unknown task")
    expect_einval(make(out_channels=1), "out_channels")
    expect_einval(make(n_nodes=0), "n_nodes")
    expect_einval(make(xt=None), "null device pointer")
    expect_einval(make(points=None), "TSP needs points")
    expect_einval(make(n_segments=3), "seg_ptr required")
    expect_einval(make(gn_phase=3), "gn_phase")
    expect_einval(make(gn_phase=1), "gn_sums")
    expect_einval(make(aggregation=3), "unknown aggregation")
    expect_einval(make(aggregation=-1), "unknown aggregation")
    with pytest.raises(_lib.DifuscoHipError):
        _lib.check(L.difusco_denoise_step(ctypes.byref(make(hidden=100))))


def test_decode_entry_points_reject_bad_arguments_without_gpu():
    import ctypes
    from difusco_amd import _lib
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    it, ok = ctypes.c_int64(), ctypes.c_int32()
    p = ctypes.c_void_p(0x1000)
    assert L.difusco_tsp_merge_tour(2, 10, p, p, p, p, p, 1 << 20, p, ctypes.byref(it), ctypes.byref(ok), None) < 0
    assert "n_nodes >= 3" in L.difusco_last_error().decode()
    assert L.difusco_tsp_merge_tour(10, 10, p, None, p, p, p, 1 << 20, p, ctypes.byref(it), ctypes.byref(ok), None) < 0
    assert L.difusco_tsp_merge_tours(10, 10, p, p, p, p, 0, p, 1 << 20, p, None, None, None) < 0      # no samples
    assert "n_samples" in L.difusco_last_error().decode()
    assert L.difusco_tsp_two_opt_workspace_bytes(3, 1, ctypes.byref(nbytes)) < 0
    assert L.difusco_tsp_two_opt(3, 1, p, p, 10, p, 1 << 20, ctypes.byref(it), None) < 0
    assert L.difusco_tsp_two_opt_workspace_bytes(1000, 4, ctypes.byref(nbytes)) == 0 and nbytes.value > 4 * 1001 * 16
    assert L.difusco_tsp_two_opt(1000, 4, p, p, 10, p, 16, ctypes.byref(it), None) < 0          # workspace too small
    assert L.difusco_knn_graph_workspace_bytes(10, 11, ctypes.byref(nbytes)) < 0                  # k > n
    assert L.difusco_knn_graph_workspace_bytes(10, 0, ctypes.byref(nbytes)) < 0
    assert L.difusco_knn_graph_workspace_bytes(5000, 2000, ctypes.byref(nbytes)) < 0              # k > 1024
    assert L.difusco_knn_graph_workspace_bytes(20000, 50, ctypes.byref(nbytes)) == 0 and nbytes.value == 1024 * 20000 * 8
    assert L.difusco_knn_graph(10, 11, p, 0, p, p, None, 0, None) < 0
    assert L.difusco_mis_decode(0, p, p, p, p, p, 1 << 20, None, None) < 0
    assert L.difusco_mis_decode_workspace_bytes(0, ctypes.byref(nbytes)) < 0


# ------------------------------------------------------------------------------------------------
# locality node order (graph.locality_node_order) and the graph cache key
# ------------------------------------------------------------------------------------------------
def test_locality_node_order_is_a_per_graph_permutation():
    """Morton renumbering: a permutation that never mixes the graphs of a disjoint-union batch; the CSR built on the
    renumbered graph describes the same edges, and ``perm`` still maps CSR slots to the caller's edge ids."""
    import torch
    from difusco_amd import graph, synthetic
    n, k, G = 60, 7, 3
    pts, ei = synthetic.tsp_batch(n, k, range(G))
    g = graph.build_csr(ei, n * G, "cpu", points=pts)
    assert g.node_order is not None
    order = g.node_order.numpy()
    assert np.array_equal(np.sort(order), np.arange(n * G))
    assert np.array_equal(order.reshape(G, n) // n, np.repeat(np.arange(G)[:, None], n, axis=1))
    inv = np.empty(n * G, dtype=np.int64)
    inv[order] = np.arange(n * G)
    e, perm = ei.numpy(), g.perm.numpy()
    assert np.array_equal(inv[e[0][perm]], g.row.numpy()) and np.array_equal(inv[e[1][perm]], g.col.numpy())
    assert np.array_equal(np.sort(perm), np.arange(e.shape[1]))
    rp = g.rowptr.numpy()
    assert np.all(np.diff(rp) == k) and np.all(np.diff(g.row.numpy()) >= 0)
    # spatial neighbours are close in the new numbering: fewer distinct neighbour ids per window of edges
    g0 = graph.build_csr(ei, n * G, "cpu")
    win = lambda c: np.mean([len(np.unique(c[i:i + 64])) for i in range(0, c.shape[0], 64)])
    assert win(g.col.numpy()) < win(g0.col.numpy())
    # one connected blob (every node reaches across the id range): one block
    ring = np.stack([np.arange(10), (np.arange(10) + 5) % 10])
    assert graph._id_blocks(*graph.csr_from_coo_host(ring, 10)[:2], 10).max() == 0


def test_prepare_graph_under_inference_mode():
    """tensors created under torch.inference_mode() have no version counter (Lightning's default for
    trainer.test); the graph cache key must not touch ``_version`` for them."""
    import torch
    from difusco_amd.models import COMetaModel
    from difusco_amd import graph
    m = COMetaModel.__new__(COMetaModel)
    m._graph_cache, m.device, m.reorder_nodes = {}, "cpu", True
    with torch.inference_mode():
        ei = torch.tensor([[0, 0, 1, 1, 2, 2], [0, 1, 1, 2, 2, 0]])
        pts = torch.rand(3, 2)
        g1 = m.prepare_graph(ei, 3, points=pts)
        g2 = m.prepare_graph(ei, 3, points=pts)
    assert g1 is g2 and isinstance(g1, graph.CsrGraph) and g1.n_edges == 6


def test_binary_input_detection_on_host():
    """models.COMetaModel._xt_is_binary: {0,1} -> table path; other values whose truncation is 0/1 -> general path;
    anything else raises like F.one_hot(xt.long(), num_classes=2) upstream (pl_meta_model.py:122-123)."""
    import torch
    from difusco_amd.models import COMetaModel
    m = COMetaModel.__new__(COMetaModel)
    m._binary_out = None
    assert m._xt_is_binary(torch.tensor([0.0, 1.0, 1.0, 0.0])) is True
    assert m._xt_is_binary(torch.tensor([0, 1, 1])) is True
    assert m._xt_is_binary(torch.tensor([0.3, 0.7, 1.2, 0.0])) is False
    assert m._xt_is_binary(torch.tensor([-0.5, 1.99])) is False
    for bad in ([2.0, 0.0], [-1.0, 1.0], [0.0, float("nan")]):
        with pytest.raises(ValueError):
            m._xt_is_binary(torch.tensor(bad))
    # a tensor remembered as our own Bernoulli output is trusted without a look - until it is modified in place
    out = torch.tensor([0.0, 1.0])
    m._binary_out = (out, out._version)
    assert m._xt_is_binary(out) is True
    out.add_(0.25)
    assert m._xt_is_binary(out) is False
    # under torch.inference_mode() (Lightning's default for trainer.test) the output has no version counter;
    # the held reference + storage identity is then the key, so the 50-step loop still never syncs to look at x_t
    with torch.inference_mode():
        out_i = torch.tensor([1.0, 0.0, 1.0])
        m._binary_out = (out_i, None)
        seen = []
        orig_all = torch.Tensor.all
        try:
            torch.Tensor.all = lambda self, *a, **k: (seen.append(1), orig_all(self, *a, **k))[1]
            assert m._xt_is_binary(out_i) is True
            assert not seen, "the known-binary fast path must not inspect the tensor"
            # an in-place edit of an inference tensor is invisible to that key; strict_binary_check=True looks
            m.strict_binary_check = True
            out_i_bad = torch.tensor([0.5, 0.0, 1.0])
            m._binary_out = (out_i_bad, None)
            assert m._xt_is_binary(out_i_bad) is False and seen
            m.strict_binary_check = False
            assert m._xt_is_binary(torch.tensor([1.0, 0.0, 1.0])) is True and seen     # a different tensor is looked at
        finally:
            torch.Tensor.all = orig_all


# ------------------------------------------------------------------------------------------------
# torch.library registration of the step (csrc/torch_ops.cpp; north_star "PyTorch-ROCm custom ops")
# ------------------------------------------------------------------------------------------------
def test_torch_ops_registered_and_host_ops_match_the_c_abi():
    import torch
    from difusco_amd import _lib, graph, torch_ops
    ops = torch_ops.load()
    assert ops.abi_version() == _lib.ABI_VERSION
    for name in ("prepare_graph", "weights_layout", "workspace_bytes", "denoise_step_categorical", "denoise_step_gaussian"):
        assert hasattr(ops, name), name
    schema = str(ops.denoise_step_categorical.default._schema)
    assert schema.startswith("difusco::denoise_step_categorical(Tensor weights, Tensor rowptr, Tensor col, Tensor? perm")
    assert "-> (Tensor, Tensor, Tensor)" in schema
    # host ops against the ctypes binding of the same C functions
    ei = O_er = torch.from_numpy(__import__("oracle.difusco_oracle", fromlist=["x"]).er_mis_instance(40, 0.2, seed=3))
    rowptr, col, row, perm, ident = ops.prepare_graph(ei, 40)
    r2, c2, w2, p2, i2 = graph.csr_from_coo_host(ei.numpy(), 40)
    assert np.array_equal(rowptr.numpy(), r2) and np.array_equal(col.numpy(), c2) and np.array_equal(row.numpy(), w2)
    assert np.array_equal(perm.numpy(), p2) and ident == i2
    off, tot = _lib.weights_layout(256, 12, 2)
    lay = ops.weights_layout(256, 12, 2)
    assert lay[:-1].tolist() == off and int(lay[-1]) == tot
    assert ops.workspace_bytes(256, 12, 1000, 100000, 1) == _lib.lib().difusco_workspace_bytes(256, 12, 1000, 100000, 1)
    with pytest.raises(RuntimeError):          # CPU tensors are refused by the step ops (no CPU kernel is registered)
        z = torch.zeros(4)
        ops.denoise_step_categorical(z, z.int(), z.int(), None, None, None, None, z, 1.0, [0.0] * 5, None, 0, 0, z,
                                     [64, 2, 2, 0, 3, 0, 1, 0, 0], False, False, None)      # (a valid 9-entry cfg: only the device is wrong)


def test_mcts_text_from_sparse_heatmap_matches_reference(golden_dir, tmp_path):
    """(f)-4 from the E-entry heatmap of a k-NN model (N=1000, K=50): the streamed text equals the reference
    converter's output on the densified matrix, for several block sizes (nothing N x N is allocated)."""
    from difusco_amd import formats
    z = np.load(os.path.join(golden_dir, "mcts_sparse_text_n1000_k50.npz"))
    n, prob = int(z["num_nodes"]), float(z["expected_valid_prob"])
    ref_text = bytes(z["text"]).decode()
    assert ref_text.count("-0.000000") > 0          # the reference's signed zeros (both orientations negative) are covered
    path = formats.write_mcts_heatmap(z["heat"], z["points"], n, str(tmp_path), 0, expected_valid_prob=prob,
                                      edge_index=z["edge_index"], use_gpu=False)
    assert path.endswith(f"heatmap/tsp{n}/heatmaptsp{n}_0.txt") and open(path).read() == ref_text
    rows_a = list(formats.mcts_heatmap_rows(z["heat"], z["edge_index"], z["points"], n, prob, block_rows=37))
    rows_b = list(formats.mcts_heatmap_rows(z["heat"], z["edge_index"], z["points"], n, prob, block_rows=1000))
    assert all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(rows_a, rows_b)) and len(rows_a) == n
    # shuffled entry order, torch tensors
    import torch
    perm = np.random.default_rng(0).permutation(z["heat"].shape[0])
    path2 = formats.write_mcts_heatmap(torch.from_numpy(z["heat"][perm]), torch.from_numpy(z["points"]), n, str(tmp_path), 1,
                                       expected_valid_prob=prob, edge_index=torch.from_numpy(z["edge_index"][:, perm].astype(np.int64)),
                                       use_gpu=False)
    assert open(path2).read() == ref_text
    # the host program runs ONLY when asked for: the default (use_gpu=None) is the GPU kernels and raises on a GPU-less host
    # instead of silently taking 31 s at N = 10^4
    if not torch.cuda.is_available():
        from difusco_amd import _lib
        with pytest.raises(_lib.DifuscoHipError):
            formats.write_mcts_heatmap(z["heat"], z["points"], n, str(tmp_path), 2, expected_valid_prob=prob,
                                       edge_index=z["edge_index"])
    # no positive entry at all: IndexError like the reference's valid_values[-k] on an empty array, also for k = 0
    far = np.array([[0.0, 0.0], [3.0, 0.0], [0.0, 3.0], [3.0, 3.0]], np.float32)      # all distances > 1: the prior is negative
    diag = np.array([[0, 1, 2, 3], [0, 1, 2, 3]])                                       # ... except on the diagonal (+0.01)
    for pr in (0.5, 0.0):
        with pytest.raises(IndexError):
            list(formats.mcts_heatmap_rows(np.full(4, -5.0, np.float32), diag, far, 4, pr))


def test_row_sum_program_is_numpys_own_order():
    """csrc/formats.hip sums an output row of the MCTS heatmap in the order numpy's float32 add.reduce uses (8192-element
    ufunc-buffer chunks, pairwise summation inside, eight interleaved accumulators per <=128-element block): the host twin of
    that program against np.sum itself, on lengths around every boundary of the scheme."""
    rng = np.random.default_rng(5)
    out = ctypes.c_float()
    for n in [1, 5, 7, 8, 9, 63, 128, 129, 130, 255, 256, 257, 1000, 1001, 4099, 8191, 8192, 8193, 8200, 10000, 16384, 20011, 38000]:
        for trial in range(3):
            a = (rng.random(n) ** 3 * 10.0 ** rng.integers(-3, 3)).astype(np.float32)
            if trial == 2:
                a[rng.random(n) < 0.9] = 0.0                                   # mostly zeros, like a thresholded row
            _lib.check(_lib.lib().difusco_host_rowsum_f32(a.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(out)))
            want = a.reshape(1, n).sum(axis=1, keepdims=True)[0, 0]
            assert np.float32(out.value) == want, (n, trial, out.value, want)


def test_mcts_k_zero_selects_the_smallest_positive_value():
    """int(N*N*prob) == 0 -> the reference's valid_values[-0] is valid_values[0], the SMALLEST positive value
    (every other positive entry is kept); the product used to raise instead."""
    from difusco_amd import formats
    rng = np.random.default_rng(3)
    n = 6
    pts = rng.random((n, 2)).astype(np.float32)
    heat = (rng.random((n, n)) ** 2).astype(np.float32)
    rows = np.stack(list(formats.mcts_heatmap_rows(*formats.sparsify(heat), pts, n, expected_valid_prob=0.01)))     # int(36*0.01) = 0
    # the reference's statements on the dense matrix
    d = np.linalg.norm(pts[:, None, :] - pts[None, :, :], axis=-1)
    adj = heat + 0.01 * (1.0 - d)
    vals = np.sort(adj[adj > 0.0])
    thr = vals[-0]
    assert thr == vals[0]
    top3 = np.argsort(adj, axis=1)[:, -3:]
    mask = adj > thr
    mask[np.arange(n)[:, None], top3] = True
    adj = adj * mask
    adj[adj != 0.0] += 1e-2
    adj = adj + adj.T
    adj = adj / adj.sum(axis=1, keepdims=True)
    assert np.array_equal(rows, adj)


def test_bench_profile_lookups_are_keyed_by_the_run():
    """bench.py's roofline extras come from committed profiles keyed by the exact run (workload : edges : variant): a run that
    was never profiled reports None - never another workload's counters - and the power-limited matrix rate is only quoted
    for the precision it was measured with."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(os.path.dirname(os.path.dirname(__file__)), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    t = bench.pmc_traffic_bytes("edge_layer_fused_kernel<FFp16>", "tsp1000", 800000, "fused-fp16x3")
    assert t is not None and t["bytes_per_launch"] > 1.5e9 and "levels" in t
    assert bench.pmc_traffic_bytes("edge_layer_fused_kernel<FFp16>", "tsp1000", 800001, "fused-fp16x3") is None
    assert bench.pmc_pipe_busy("tsp1000", 800001, "fused-fp16x3", 0.72e-3) is None
    p = bench.pmc_pipe_busy("tsp1000", 800000, "fused-fp16x3", 0.72e-3)
    assert p is not None and 0.2 < p["value"] < 0.5
    pl = bench.power_limited_mfma(830.0, "fp16x3")
    assert pl is not None and 0.4 < pl["frac_of_nominal_peak"] < 0.55 and abs(pl["frac_issued_of_power_limited"] - 830.0 / pl["gemm_only_TFLOPs_issued"]) < 1e-12
    assert pl["power_cap_W"] == 1400.0 and pl["power_W"] >= 1390.0
    assert bench.power_limited_mfma(830.0, "bf16x3") is None


def test_bench_stdout_line_is_compact():
    """the driver could not parse a 20.8 KB bench line.  The stdout line is `compact_record(full)`: the contract's
    fields + roofline + cpu_baseline + one line per workload, < 4 KB, valid JSON - checked on round 4's full 20.8 KB record."""
    import importlib.util
    import json
    root = os.path.dirname(os.path.dirname(__file__))
    spec = importlib.util.spec_from_file_location("bench_module2", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    full = json.load(open(os.path.join(root, "profiles", "r04", "bench_default.json")))
    assert len(json.dumps(full)) > 20000
    full["power"] = {"power_W_median": 1351.0, "power_W_max": 1402.0, "sclk_MHz_median": 1893.0, "samples": 41, "J_per_graph_step": 1.61,
                     "source": "hwmon power1_average + freq1_input, sampled inside the timed loops"}
    line = json.dumps(bench.compact_record(full, "/x/bench_full.json"), separators=(",", ":"))
    assert len(line) < 4096, len(line)
    rec = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "workloads", "repeats", "parity_linf", "ranks_seen", "power"):
        assert key in rec, key
    assert rec["value"] == full["value"] and rec["ms_per_step"] == full["ms_per_step"]
    r = rec["roofline"]
    assert r["bound"] == "mfma" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4 and r["traffic"]["bytes_per_launch"] > 1e9
    assert set(rec["workloads"]) == {"tsp500", "tsp10000", "mis", "tsp50dense"}
    assert rec["cpu_baseline"]["kind"] == "port" and rec["cpu_baseline"]["cores"] >= 1 and rec["cpu_baseline"]["value"] > 0
    assert rec["full_record"] == "bench_full.json"


def test_bench_dump_outputs_caps_the_total_with_a_fixed_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 .npy per array, shape kept while the array fits its share of the cap; a larger array is
    replaced by the same seeded sample of its elements in every run."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(__file__))
    spec = importlib.util.spec_from_file_location("bench_module4", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 4 * 1000)
    small = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    big = torch.arange(5000, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    a_small, a_big = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert a_small.dtype == np.float32 and np.array_equal(a_small, small.float().numpy())
    assert a_big.dtype == np.float32 and a_big.shape == (1000,) and np.all(np.diff(a_big) > 0)     # sorted distinct elements
    assert np.array_equal(a_big, np.load(tmp_path / "b" / "big.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 2 * 4 * 1000 + 2 * 256


def test_node4_fused_vectors():
    """ABI 11: bias / column scales with which the node linear writes the A | B rows in the fused kernel's log2(e) domain."""
    H = 64
    st = synthetic_state = __import__("difusco_amd.synthetic", fromlist=["x"]).random_state_dict(H, 2, 2, seed=5)
    w4 = torch.cat([st[f"layers.1.{m}.weight"] for m in "UVAB"], dim=0)
    planes = weights.split_planes(w4, per_row=True)
    bias, scale = weights.node4_fused_vectors(st, 1, H, planes)
    c = np.float32(weights.LOG2E)
    assert bias.shape == (4 * H,) and scale.shape == (8 * H,)
    assert torch.equal(bias[:H], st["layers.1.U.bias"]) and torch.equal(bias[H:2 * H], st["layers.1.V.bias"])
    assert torch.equal(bias[2 * H:3 * H], (st["layers.1.A.bias"] + st["layers.1.C.bias"]) * c)
    assert torch.equal(bias[3 * H:], st["layers.1.B.bias"] * c)
    w_inv = weights.plane_scale_inv(planes, 4 * H, H)
    assert torch.equal(scale[:2 * H], w_inv[:2 * H]) and torch.equal(scale[2 * H:4 * H], w_inv[2 * H:] * c)
    assert (scale[4 * H:6 * H] == 1).all() and (scale[6 * H:] == c).all()
    # and the packed blob holds them where the layout says
    blob = weights.pack_state_dict(st)
    off, _ = _lib.weights_layout(H, 2, 2)
    base = len(_lib.W_GLOBAL) + 1 * len(_lib.W_LAYER)
    ib, isc = base + _lib.W_LAYER.index("@node4.fused_bias"), base + _lib.W_LAYER.index("@node4.fused_scale")
    assert torch.equal(blob[off[ib]: off[ib] + 4 * H], bias) and torch.equal(blob[off[isc]: off[isc] + 8 * H], scale)


def test_bench_power_sampler_reads_hwmon_files(tmp_path):
    """bench.py's live power / clock sampler: hwmon-style files (microwatts, hertz) read by a background thread between start() and
    stop(); the summary carries medians and joules per graph-step; with no readable source it reports zero samples instead of failing."""
    import importlib.util
    import time
    root = os.path.dirname(os.path.dirname(__file__))
    spec = importlib.util.spec_from_file_location("bench_module3", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    s = bench.PowerSampler(torch.device("cpu"), period=0.002)
    (tmp_path / "power1_input").write_text("1300000000\n")
    (tmp_path / "freq1_input").write_text("1850000000\n")
    s.power_file, s.freq_file, s.source = str(tmp_path / "power1_input"), str(tmp_path / "freq1_input"), "hwmon power1_input + freq1_input"
    s.start()
    time.sleep(0.05)
    s.stop()
    out = s.summary(seconds_per_step=9.0e-3, graphs=8)
    assert out["samples"] >= 5 and out["power_W_median"] == 1300.0 and out["sclk_MHz_median"] == 1850.0
    assert abs(out["J_per_graph_step"] - 1300.0 * 9.0e-3 / 8) < 1e-9
    empty = bench.PowerSampler(torch.device("cpu"))
    empty.power_file, empty.samples = None, [(None, None)]
    assert empty.summary(1.0, 1)["samples"] == 0
