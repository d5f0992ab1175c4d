"""What the resident 2-opt (``difusco_tsp_two_opt_resident``, one GPU block per group) decides without a GPU: the three symbols,
the limit, the workspace size and its refusals, the refusals of the entry before any GPU work (the group above the limit
included: the sizes are host arrays), ``check_two_opt_mode``, the ``two_opt_mode`` of the solvers and the runner's
``--two_opt_mode``."""
import ctypes

import numpy as np
import pytest

I64P = ctypes.POINTER(ctypes.c_int64)


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def workspace_bytes(L, group_n, group_tours, method):
    n, t, out = _i32(group_n), _i32(group_tours), ctypes.c_size_t(0)
    rc = L.difusco_tsp_two_opt_resident_workspace_bytes(len(n), n.ctypes.data if len(n) else None, t.ctypes.data if len(t) else None,
                                                        method, ctypes.byref(out))
    return rc, int(out.value)


def test_the_three_symbols_exist_and_the_limit_is_a_constant_of_at_least_2048_cells():
    from difusco_amd import _lib, decode
    L = _lib.lib()
    for name in ("difusco_tsp_two_opt_resident_max_cells", "difusco_tsp_two_opt_resident_workspace_bytes", "difusco_tsp_two_opt_resident"):
        assert hasattr(L, name), name
    m = L.difusco_tsp_two_opt_resident_max_cells()
    assert m >= 2048 and m == L.difusco_tsp_two_opt_resident_max_cells() == decode.two_opt_resident_max_cells()
    assert 4 * (500 + 1) <= m                                   # TSP-500 with --parallel_sampling 4


def test_workspace_bytes_succeeds_on_valid_sizes_and_refuses_the_rest_with_the_shared_texts():
    from difusco_amd import _lib
    L = _lib.lib()
    for group_n, group_tours in (([5], [1]), ([5, 9], [2, 1]), ([500] * 64, [4] * 64), ([4], [600])):
        for method in (0, 1):
            rc, nbytes = workspace_bytes(L, group_n, group_tours, method)
            assert rc == 0 and nbytes >= 20 * len(group_n), (group_n, method)
    # a group above the limit has a workspace size all the same: the entry refuses it, with the text that names it
    assert workspace_bytes(L, [L.difusco_tsp_two_opt_resident_max_cells()], [1], 0)[0] == 0
    who = "two_opt_resident_workspace_bytes"
    for group_n, group_tours, method, text in (
            ([], [], 0, f"{who}: groups = 0, needs at least 1"),
            ([5, 3], [2, 1], 0, f"{who}: group 1 has n = 3, needs n >= 4"),
            ([5, 65535 * 16 + 1], [2, 1], 0, f"{who}: group 1 has n = {65535 * 16 + 1}, at most {65535 * 16} nodes"),
            ([5, 9], [0, 1], 1, f"{who}: group 0 has 0 tours, needs at least 1"),
            ([5, 9], [65535, 1], 1, f"{who}: more than 65535 tours in one call"),
            ([5, 9], [2, 1], 2, f"{who}: method 2 (0 exact, 1 screened)")):
        assert workspace_bytes(L, group_n, group_tours, method)[0] == -1, text
        assert L.difusco_last_error().decode() == text
    n, t = _i32([5]), _i32([1])
    assert L.difusco_tsp_two_opt_resident_workspace_bytes(1, n.ctypes.data, t.ctypes.data, 0, None) == -1
    assert L.difusco_last_error().decode() == f"{who}: bytes is null"
    assert L.difusco_tsp_two_opt_resident_workspace_bytes(1, None, t.ctypes.data, 0, ctypes.byref(ctypes.c_size_t())) == -1
    assert L.difusco_last_error().decode() == f"{who}: group_n / group_tours is null"


def refused_call(L, group_n=(5, 9), group_tours=(2, 1), method=0, max_iterations=10, moves_per_launch=0, null=None, short=0,
                 groups=None):
    """The entry on a tiny valid call with one thing changed; every array is a host array, which a refused call never reads.
    Returns (return code, text, the tours array as bytes before and after)."""
    rc, need = workspace_bytes(L, [5, 9], [2, 1], 0)
    assert rc == 0
    gn, gt = _i32(group_n), _i32(group_tours)
    arrays = {"points": np.zeros(64), "tours": np.arange(64, dtype=np.int32), "workspace": np.zeros(need, dtype=np.uint8),
              "iterations_out": np.zeros(4, dtype=np.int64), "group_n": gn, "group_tours": gt}
    before = arrays["tours"].tobytes()
    ptr = lambda name: None if null == name else arrays[name].ctypes.data_as(I64P if name == "iterations_out" else ctypes.c_void_p)
    pairs, syncs = ctypes.c_int64(), ctypes.c_int32()
    rc = L.difusco_tsp_two_opt_resident(len(gn) if groups is None else groups, ptr("group_n"), ptr("group_tours"), ptr("points"),
                                        ptr("tours"), max_iterations, method, moves_per_launch, ptr("workspace"), need - short,
                                        ptr("iterations_out"), ctypes.byref(pairs), ctypes.byref(syncs), None)
    return int(rc), L.difusco_last_error().decode(), before, arrays["tours"].tobytes()


def test_every_refusal_comes_before_any_gpu_work_with_its_text():
    from difusco_amd import _lib
    L = _lib.lib()
    who = "tsp_two_opt_resident"
    need = workspace_bytes(L, [5, 9], [2, 1], 0)[1]
    arrays = f"{who}: needs non-null device arrays, a host iterations_out[groups] and max_iterations >= 0"
    for change, text in (
            (dict(groups=0), f"{who}: groups = 0, needs at least 1"),
            (dict(null="group_n"), f"{who}: group_n / group_tours is null"),
            (dict(null="group_tours"), f"{who}: group_n / group_tours is null"),
            (dict(group_n=[5, 3]), f"{who}: group 1 has n = 3, needs n >= 4"),
            (dict(group_n=[5, 65535 * 16 + 1]), f"{who}: group 1 has n = {65535 * 16 + 1}, at most {65535 * 16} nodes"),
            (dict(group_tours=[0, 1]), f"{who}: group 0 has 0 tours, needs at least 1"),
            (dict(group_tours=[65535, 1]), f"{who}: more than 65535 tours in one call"),
            (dict(method=2), f"{who}: method 2 (0 exact, 1 screened)"),
            (dict(method=-1), f"{who}: method -1 (0 exact, 1 screened)"),
            (dict(null="points"), arrays), (dict(null="tours"), arrays), (dict(null="workspace"), arrays),
            (dict(null="iterations_out"), arrays), (dict(max_iterations=-1), arrays),
            (dict(moves_per_launch=-1), f"{who}: moves_per_launch = -1 < 0"),
            (dict(short=1), f"{who}: workspace {need - 1} < {need} bytes")):
        rc, got, before, after = refused_call(L, **change)
        assert rc == -1 and got == text, change
        assert before == after, change


def test_a_group_above_the_limit_is_refused_on_the_host_and_named():
    from difusco_amd import _lib
    L = _lib.lib()
    m = L.difusco_tsp_two_opt_resident_max_cells()
    rc, text, before, after = refused_call(L, group_n=[m], group_tours=[1])          # m + 1 cells
    assert rc == -4 and before == after
    assert "group 0 " in text and f"{m + 1} cells" in text and f"limit of {m} cells" in text
    rc, text, before, after = refused_call(L, group_n=[5, 500], group_tours=[2, m // 501 + 1])
    assert rc == -4 and before == after
    assert "group 1 " in text and f"{(m // 501 + 1) * 501} cells" in text and f"limit of {m} cells" in text
    # the check of the group arrays comes first: its text, not the limit's
    rc, text, _, _ = refused_call(L, group_n=[m, 3], group_tours=[1, 1])
    assert rc == -1 and "group 1 has n = 3" in text


def test_check_two_opt_mode_handles_its_combinations():
    from difusco_amd import decode, pipeline
    assert decode.TWO_OPT_MODES == ("launches", "resident")
    assert decode.TWO_OPT_METHODS == ("exact", "screened")
    assert decode.check_two_opt_mode("2opt", "resident") == "resident"
    for search in decode.LOCAL_SEARCHES:
        assert decode.check_two_opt_mode(search, "launches") == "launches"
        if search != "2opt":
            with pytest.raises(ValueError, match="needs local_search='2opt'"):
                decode.check_two_opt_mode(search, "resident")
    for mode in ("persistent", "", None):
        with pytest.raises(ValueError, match="one of"):
            decode.check_two_opt_mode("2opt", mode)
    pts = np.zeros((8, 2))
    # before any GPU work: there is no model to touch
    with pytest.raises(ValueError, match="needs local_search='2opt'"):
        pipeline.solve_tsp(None, pts, -1, local_search="2opt+oropt", two_opt_mode="resident")
    with pytest.raises(ValueError, match="needs local_search='2opt'"):
        pipeline.solve_tsp_batch(None, pts[None], -1, local_search="multi2opt", two_opt_mode="resident")
    with pytest.raises(ValueError, match="needs local_search='2opt'"):
        pipeline.solve_tsp_batch(None, [pts, pts[:5]], -1, local_search="multi2opt+oropt", two_opt_mode="resident")
    with pytest.raises(ValueError, match="one of"):
        pipeline.solve_tsp(None, pts, -1, two_opt_mode="blocks")
    with pytest.raises(ValueError, match="one of"):
        pipeline.solve_tsp_batch(None, pts[None], -1, two_opt_mode="blocks")


def test_the_wrappers_check_the_mode_before_any_gpu_work():
    from difusco_amd import decode
    pts, tour = np.zeros((5, 2)), np.array([[0, 1, 2, 3, 4, 0]])
    for fn, args in ((decode.batched_two_opt_torch, (pts, tour)), (decode.batched_two_opt_grouped, (pts[None], tour)),
                     (decode.batched_two_opt_ragged, ([pts], [tour]))):
        with pytest.raises(ValueError, match="one of"):
            fn(*args, device="cuda:0", mode="blocks")
        with pytest.raises(decode._lib.DifuscoHipError, match="GPU only"):
            fn(*args, device="cpu", mode="resident")


def test_evaluate_accepts_the_flag_and_refuses_it_with_mis_and_another_search(capsys):
    from difusco_amd import evaluate as EV
    base = ["--storage_path", "x", "--do_test", "--ckpt_path", "c"]
    tsp = base + ["--task", "tsp"]
    args, _ = EV.parse_args(tsp)
    assert args.two_opt_mode == "launches"
    args, _ = EV.parse_args(tsp + ["--two_opt_mode", "resident"])
    assert (args.two_opt_mode, args.local_search, args.two_opt_method) == ("resident", "2opt", "exact")
    args, _ = EV.parse_args(tsp + ["--two_opt_mode", "resident", "--two_opt_method", "screened", "--local_search", "2opt"])
    assert (args.two_opt_mode, args.two_opt_method) == ("resident", "screened")
    args, _ = EV.parse_args(base + ["--task", "mis", "--two_opt_mode", "launches"])
    assert args.two_opt_mode == "launches"
    with pytest.raises(SystemExit) as e:
        EV.parse_args(base + ["--task", "mis", "--two_opt_mode", "resident"])
    assert e.value.code == 2 and "--task tsp" in capsys.readouterr().err
    for search in ("2opt+oropt", "multi2opt", "multi2opt+oropt"):
        with pytest.raises(SystemExit) as e:
            EV.parse_args(tsp + ["--two_opt_mode", "resident", "--local_search", search])
        assert e.value.code == 2 and "--local_search 2opt" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        EV.parse_args(tsp + ["--two_opt_mode", "blocks"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err


def test_the_default_record_keys_are_unchanged_and_the_mode_adds_one():
    """``tsp_record`` is what every record starts as; ``solve_split`` adds ``two_opt_mode`` only in the resident mode (the GPU test
    runs the runner both ways and compares the header lines as well)."""
    import inspect

    from difusco_amd import evaluate as EV

    class Ex:
        source, points, tour = ("f", 0), np.array([[0., 0.], [1., 0.], [1., 1.], [0., 1.]]), [0, 1, 2, 3, 0]
    info = {"merge_iterations": 3.0, "two_opt_iterations": 2, "merged_costs": [4.0]}
    rec = EV.tsp_record("val", 0, Ex, 7, ([0, 1, 2, 3, 0], 4.0, [4.0], info))
    assert list(rec) == ["split", "index", "source", "n_nodes", "gt_cost", "solved_cost", "all_costs", "merged_costs", "2opt_iterations",
                         "merge_iterations", "seed", "tour"]
    assert inspect.signature(EV.solve_split).parameters["two_opt_mode"].default == "launches"
