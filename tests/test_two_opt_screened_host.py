"""Screened 2-opt without a GPU: the host bound function, the proven margin held against a numpy restatement of the float32
screen on adversarial inputs, the skip rule's answer against the oracle's, and the argument checks of every new entry."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

import two_opt_screen_emulation as S
from difusco_amd import _lib
from difusco_amd.decode import batched_two_opt_grouped, batched_two_opt_torch, two_opt_screen_bound


# ---- the bound function ------------------------------------------------------------------------------------------------------
def test_screen_bound_is_positive_finite_and_scales():
    eps = {m: two_opt_screen_bound(m) for m in (1e-3, 1.0, 1e3)}
    for m, e in eps.items():
        assert e is not None and math.isfinite(e) and e > 0.0, m
    assert eps[1e-3] < eps[1.0] < eps[1e3]
    assert eps[1e3] == pytest.approx(1e3 * eps[1.0], rel=1e-12) and eps[1e-3] == pytest.approx(1e-3 * eps[1.0], rel=1e-12)
    assert eps[1.0] < 1e-5                       # a screen with a margin near the stop test's 1e-6, not a vacuous one


@pytest.mark.parametrize("m", [float("inf"), float("nan"), 1e30, 1e300, 1e-30, 0.0, -1.0])
def test_screen_bound_reports_no_bound(m):
    assert two_opt_screen_bound(m) is None


def test_screen_bound_c_entry():
    L = _lib.lib()
    eps = ctypes.c_double(-1.0)
    assert L.difusco_tsp_two_opt_screen_bound(1.0, ctypes.byref(eps)) == 1 and eps.value == two_opt_screen_bound(1.0)
    assert L.difusco_tsp_two_opt_screen_bound(float("inf"), ctypes.byref(eps)) == 0 and eps.value == 0.0
    assert L.difusco_tsp_two_opt_screen_bound(1.0, None) < 0
    assert L.difusco_abi_version() == 13


# ---- the bound against the float32 program -----------------------------------------------------------------------------------
N = 160


def _nn_tour(pts):
    """A decoded-like start: the nearest-neighbour tour from node 0."""
    n = len(pts)
    left = np.ones(n, dtype=bool)
    tour = [0]
    left[0] = False
    while len(tour) < n:
        d = ((pts - pts[tour[-1]]) ** 2).sum(-1)
        d[~left] = np.inf
        tour.append(int(d.argmin()))
        left[tour[-1]] = False
    return np.array(tour + [0])


def _point_sets():
    rng = np.random.default_rng(11)
    uniform = rng.random((N, 2))
    centres = rng.random((5, 2))
    clustered = centres[rng.integers(0, 5, N)] + 1e-3 * rng.standard_normal((N, 2))
    dup = uniform.copy()
    dup[N // 2:] = dup[:N // 2]                                     # every point twice
    collinear = np.stack([np.sort(rng.random(N)), np.full(N, 0.25)], axis=1)
    collinear[::7, 0] = collinear[3, 0]                             # and repeated abscissae
    grid = np.round(rng.random((N, 2)) * 4096) / 4096               # 2^-12 grid
    coarse = np.round(rng.random((N, 2)) * 8) / 8                   # many exact ties and duplicates
    return {"uniform": uniform, "clustered": clustered, "duplicates": dup, "collinear": collinear, "grid_2^-12": grid,
            "grid_1/8": coarse, "scaled_1e-3": uniform * 1e-3, "scaled_1e4": uniform * 1e4, "offset_1000": uniform + 1000.0}


def _cases():
    rng = np.random.default_rng(3)
    for name, pts in _point_sets().items():
        yield name + "/random", pts, np.concatenate([[0], 1 + rng.permutation(N - 1), [0]])
        yield name + "/decoded", pts, _nn_tour(pts)


CASES = list(_cases())


@pytest.mark.parametrize("name,pts,tour", CASES, ids=[c[0] for c in CASES])
def test_restated_change_matrix_picks_the_oracles_move(name, pts, tour):
    """The helper's c64 / (min, first flat index) against oracle.tsp_decode_oracle itself: one step of ``batched_two_opt``
    applies exactly the move the restated matrix selects (or none, under the oracle's stop test)."""
    from oracle import tsp_decode_oracle as D
    best, flat = S.oracle_best(S.c64_matrix(pts, tour))
    want = np.array(tour, dtype=np.int64)
    if best < -1e-6:
        i, j = divmod(flat, N)
        want[i + 1:j + 1] = want[i + 1:j + 1][::-1].copy()
    got, moves = D.batched_two_opt(pts, np.asarray(tour)[None, :], max_iterations=1)
    assert moves == int(best < -1e-6) and np.array_equal(got[0], want)


@pytest.mark.parametrize("name,pts,tour", CASES, ids=[c[0] for c in CASES])
def test_float32_change_stays_within_the_bound(name, pts, tour):
    eps = two_opt_screen_bound(np.abs(pts).max())
    assert eps is not None
    c64 = S.c64_matrix(pts, tour)
    valid = S.valid_mask(N)
    worst = 0.0
    for contracted in (True, False):
        for ulps in (-2, 0, 2):                                     # a square root off by up to 2 ulps either way
            c32 = S.c32_matrix(pts, tour, contracted=contracted, sqrt_ulps=ulps)
            assert np.isfinite(c32[valid]).all()
            worst = max(worst, float(np.abs(c32.astype(np.float64) - c64)[valid].max()))
    print(f"{name}: max |c32 - c64| = {worst:.3e}, eps = {eps:.3e} (ratio {worst / eps:.3f})")
    assert worst <= eps


@pytest.mark.parametrize("name,pts,tour", CASES, ids=[c[0] for c in CASES])
def test_screen_rule_yields_the_oracle_move(name, pts, tour):
    eps = two_opt_screen_bound(np.abs(pts).max())
    c64 = S.c64_matrix(pts, tour)
    valid = S.valid_mask(N)
    want = S.oracle_best(c64)
    for contracted in (True, False):
        for ulps in (-1, 0, 1):
            c32 = S.c32_matrix(pts, tour, contracted=contracted, sqrt_ulps=ulps)
            got, exact_pairs, upper, survive = S.screened_best(c32, c64, eps)
            assert got == want, (name, contracted, ulps)
            # the kernel's float32 comparison skips no pair that "skip only if c32 - eps > T" would keep, T = U, and U is
            # an upper bound of the answer
            skipped = valid & ~survive
            assert (c32[skipped].astype(np.float64) - eps > upper).all() and upper >= want[0]
            if contracted and ulps == 0:
                print(f"{name}: {exact_pairs} of {int(valid.sum())} pairs take the float64 path")


# ---- arguments -----------------------------------------------------------------------------------------------------------------
def test_unknown_method_raises_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    pts = np.random.default_rng(0).random((20, 2))
    with pytest.raises(ValueError, match="bogus"):
        batched_two_opt_torch(pts, np.zeros((1, 21), np.int64), method="bogus")
    with pytest.raises(ValueError, match="bogus"):
        batched_two_opt_grouped(pts[None], np.zeros((1, 21), np.int64), method="bogus")
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    model = types.SimpleNamespace(device=torch.device("cpu"))
    with pytest.raises(ValueError, match="bogus"):
        solve_tsp(model, pts, 5, two_opt_method="bogus")
    with pytest.raises(ValueError, match="bogus"):
        solve_tsp_batch(model, pts[None], 5, two_opt_method="bogus")


def test_screened_method_has_no_cpu_fallback():
    pts = np.random.default_rng(0).random((20, 2))
    with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
        batched_two_opt_torch(pts, np.zeros((1, 21), np.int64), device="cpu", method="screened")
    with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
        batched_two_opt_grouped(pts[None], np.zeros((1, 21), np.int64), device="cpu", method="screened")


def test_screened_entries_reject_bad_arguments_without_gpu():
    """The checks of tests/test_host_logic.py (plain entry) and tests/test_batch_host.py (grouped entry) on the new entries."""
    L = _lib.lib()
    nbytes, exact = ctypes.c_size_t(), ctypes.c_size_t()
    it, pairs = ctypes.c_int64(), ctypes.c_int64()
    p = ctypes.c_void_p(0x1000)
    assert L.difusco_tsp_two_opt_screened_workspace_bytes(3, 1, ctypes.byref(nbytes)) < 0
    assert L.difusco_tsp_two_opt_screened(3, 1, p, p, 10, p, 1 << 20, ctypes.byref(it), ctypes.byref(pairs), None) < 0
    assert L.difusco_tsp_two_opt_screened_workspace_bytes(1000, 4, ctypes.byref(nbytes)) == 0
    assert L.difusco_tsp_two_opt_workspace_bytes(1000, 4, ctypes.byref(exact)) == 0
    assert nbytes.value > exact.value > 4 * 1001 * 16              # the exact sweep's arrays and the screen's
    assert L.difusco_tsp_two_opt_screened(1000, 4, p, p, 10, p, 16, ctypes.byref(it), None, None) < 0   # workspace too small
    assert "workspace" in L.difusco_last_error().decode()
    assert L.difusco_tsp_two_opt_screened(1000, 4, None, p, 10, p, nbytes.value, ctypes.byref(it), None, None) < 0
    assert L.difusco_tsp_two_opt_screened(1000, 4, p, p, -1, p, nbytes.value, ctypes.byref(it), None, None) < 0

    nb = ctypes.c_size_t()
    assert L.difusco_tsp_two_opt_grouped_screened_workspace_bytes(3, 2, 2, ctypes.byref(nb)) == -1
    assert L.difusco_tsp_two_opt_grouped_screened_workspace_bytes(10, 0, 2, ctypes.byref(nb)) == -1
    assert L.difusco_tsp_two_opt_grouped_screened_workspace_bytes(10, 2, 0, ctypes.byref(nb)) == -1
    assert L.difusco_tsp_two_opt_grouped_screened_workspace_bytes(10, 2, 3, None) == -1
    assert L.difusco_tsp_two_opt_grouped_screened_workspace_bytes(10, 2, 3, ctypes.byref(nb)) == 0 and nb.value > 0
    its = (ctypes.c_int64 * 2)()
    assert L.difusco_tsp_two_opt_grouped_screened(10, 2, 3, p, p, 5, p, 0, its, None, None) == -1      # workspace too small
    assert "workspace" in L.difusco_last_error().decode()
    assert L.difusco_tsp_two_opt_grouped_screened(10, 2, 3, p, p, 5, p, nb.value, None, None, None) == -1   # no iterations_out
    assert L.difusco_tsp_two_opt_grouped_screened(10, 2, 3, p, p, -1, p, nb.value, its, None, None) == -1
    assert L.difusco_abi_version() == 13


def test_evaluate_accepts_two_opt_method():
    from difusco_amd import evaluate as E
    base = ["--task", "tsp", "--storage_path", "/data", "--do_test", "--ckpt_path", "last.ckpt"]
    args, ignored = E.parse_args(base + ["--two_opt_method", "screened", "--two_opt_iterations", "5000"])
    assert args.two_opt_method == "screened" and args.two_opt_iterations == 5000 and ignored == []
    args, ignored = E.parse_args(base)
    assert args.two_opt_method == "exact" and ignored == []
    assert "two_opt_method" not in E.TRAINING_ONLY
    with pytest.raises(SystemExit):
        E.parse_args(base + ["--two_opt_method", "bogus"])
