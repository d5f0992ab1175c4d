"""What the resident 2-opt + Or-opt search (``difusco_tsp_local_search_resident``, one GPU block per group) decides without a
GPU: the three symbols, the limit, the workspace size and its refusals, the refusals of the entry before any GPU work (the group
above the limit included: the sizes are host arrays), ``check_tsp_local_search_mode``, the ``local_search_mode`` of the solvers,
the old ``check_two_opt_mode`` refusals and the runner's ``--tsp_local_search_mode``."""
import ctypes

import numpy as np
import pytest

I64P = ctypes.POINTER(ctypes.c_int64)
I32P = ctypes.POINTER(ctypes.c_int32)
WHO = "tsp_local_search_resident"


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def workspace_bytes(L, group_n, group_tours):
    n, t, out = _i32(group_n), _i32(group_tours), ctypes.c_size_t(0)
    rc = L.difusco_tsp_local_search_resident_workspace_bytes(len(n), n.ctypes.data if len(n) else None,
                                                             t.ctypes.data if len(t) else None, ctypes.byref(out))
    return rc, int(out.value)


def test_the_three_symbols_exist_and_the_limit_is_a_constant_of_at_least_2048_cells():
    from difusco_amd import _lib, decode
    L = _lib.lib()
    for name in ("difusco_tsp_local_search_resident_max_cells", "difusco_tsp_local_search_resident_workspace_bytes",
                 "difusco_tsp_local_search_resident"):
        assert hasattr(L, name), name
    m = L.difusco_tsp_local_search_resident_max_cells()
    assert m >= 2048 and m == L.difusco_tsp_local_search_resident_max_cells() == decode.local_search_resident_max_cells()
    assert 4 * (500 + 1) <= m                                   # TSP-500 with --parallel_sampling 4


def test_workspace_bytes_is_monotone_in_groups_and_refuses_the_rest_with_the_shared_texts():
    from difusco_amd import _lib
    L = _lib.lib()
    sizes = []
    for groups in (1, 2, 7, 8, 9, 64, 512, 600, 4096):
        rc, nbytes = workspace_bytes(L, [5 + g % 3 for g in range(groups)], [1 + g % 2 for g in range(groups)])
        assert rc == 0 and nbytes >= 32 * groups + 8, groups                      # the state of every group and the shared count
        sizes.append(nbytes)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # the size depends on the number of groups alone, and a group above the limit has one all the same: the entry refuses it
    assert workspace_bytes(L, [500] * 64, [4] * 64)[1] == sizes[5]
    assert workspace_bytes(L, [L.difusco_tsp_local_search_resident_max_cells()], [1])[0] == 0
    who = "local_search_resident_workspace_bytes"
    for group_n, group_tours, text in (
            ([], [], f"{who}: groups = 0, needs at least 1"),
            ([5, 3], [2, 1], f"{who}: group 1 has n = 3, needs n >= 4"),
            ([5, 65535 * 16 + 1], [2, 1], f"{who}: group 1 has n = {65535 * 16 + 1}, at most {65535 * 16} nodes"),
            ([5, 9], [0, 1], f"{who}: group 0 has 0 tours, needs at least 1"),
            ([5, 9], [65535, 1], f"{who}: more than 65535 tours in one call")):
        assert workspace_bytes(L, group_n, group_tours)[0] == -1, text
        assert L.difusco_last_error().decode() == text
    n, t = _i32([5]), _i32([1])
    assert L.difusco_tsp_local_search_resident_workspace_bytes(1, n.ctypes.data, t.ctypes.data, None) == -1
    assert L.difusco_last_error().decode() == f"{who}: bytes is null"
    assert L.difusco_tsp_local_search_resident_workspace_bytes(1, None, t.ctypes.data, ctypes.byref(ctypes.c_size_t())) == -1
    assert L.difusco_last_error().decode() == f"{who}: group_n / group_tours is null"


OUTS = ("two_opt_iterations_out", "or_opt_iterations_out", "rounds_out")


def refused_call(L, group_n=(5, 9), group_tours=(2, 1), max_iterations=10, max_rounds=16, steps_per_launch=0, null=None, short=0,
                 groups=None):
    """The entry on a tiny valid call with one thing changed; every array is a host array, which a refused call never reads.
    Returns (return code, text, the tours array as bytes before and after)."""
    rc, need = workspace_bytes(L, [5, 9], [2, 1])
    assert rc == 0
    gn, gt = _i32(group_n), _i32(group_tours)
    arrays = {"points": np.zeros(64), "tours": np.arange(64, dtype=np.int32), "workspace": np.zeros(need, dtype=np.uint8),
              "two_opt_iterations_out": np.zeros(4, dtype=np.int64), "or_opt_iterations_out": np.zeros(4, dtype=np.int64),
              "rounds_out": np.zeros(4, dtype=np.int32), "group_n": gn, "group_tours": gt}
    before = arrays["tours"].tobytes()
    ptr = lambda name: None if null == name else arrays[name].ctypes.data_as(ctypes.c_void_p)
    syncs = ctypes.c_int32()
    rc = L.difusco_tsp_local_search_resident(len(gn) if groups is None else groups, ptr("group_n"), ptr("group_tours"), ptr("points"),
                                             ptr("tours"), max_iterations, max_rounds, steps_per_launch, ptr("workspace"),
                                             need - short, *(ptr(k) for k in OUTS), ctypes.byref(syncs), None)
    return int(rc), L.difusco_last_error().decode(), before, arrays["tours"].tobytes()


def test_every_refusal_comes_before_any_gpu_work_with_its_text():
    from difusco_amd import _lib
    L = _lib.lib()
    need = workspace_bytes(L, [5, 9], [2, 1])[1]
    arrays = (f"{WHO}: needs non-null device arrays, host two_opt_iterations_out, or_opt_iterations_out and rounds_out [groups] "
              "and max_iterations >= 0")
    for change, text in (
            (dict(groups=0), f"{WHO}: groups = 0, needs at least 1"),
            (dict(null="group_n"), f"{WHO}: group_n / group_tours is null"),
            (dict(null="group_tours"), f"{WHO}: group_n / group_tours is null"),
            (dict(group_n=[5, 3]), f"{WHO}: group 1 has n = 3, needs n >= 4"),
            (dict(group_n=[5, 65535 * 16 + 1]), f"{WHO}: group 1 has n = {65535 * 16 + 1}, at most {65535 * 16} nodes"),
            (dict(group_tours=[0, 1]), f"{WHO}: group 0 has 0 tours, needs at least 1"),
            (dict(group_tours=[65535, 1]), f"{WHO}: more than 65535 tours in one call"),
            (dict(null="points"), arrays), (dict(null="tours"), arrays), (dict(null="workspace"), arrays),
            (dict(null="two_opt_iterations_out"), arrays), (dict(null="or_opt_iterations_out"), arrays),
            (dict(null="rounds_out"), arrays), (dict(max_iterations=-1), arrays),
            (dict(max_rounds=0), f"{WHO}: max_rounds = 0, needs at least 1"),
            (dict(max_rounds=-3), f"{WHO}: max_rounds = -3, needs at least 1"),
            (dict(steps_per_launch=-1), f"{WHO}: steps_per_launch = -1 < 0"),
            (dict(short=1), f"{WHO}: workspace {need - 1} < {need} bytes")):
        rc, got, before, after = refused_call(L, **change)
        assert rc == -1 and got == text, change
        assert before == after, change


def test_a_group_above_the_limit_is_refused_on_the_host_and_named():
    from difusco_amd import _lib
    L = _lib.lib()
    m = L.difusco_tsp_local_search_resident_max_cells()
    rc, text, before, after = refused_call(L, group_n=[m], group_tours=[1])          # m + 1 cells
    assert rc == -4 and before == after
    assert "group 0 " in text and f"{m + 1} cells" in text and f"limit of {m} cells" in text
    rc, text, before, after = refused_call(L, group_n=[5, 500], group_tours=[2, m // 501 + 1])
    assert rc == -4 and before == after
    assert "group 1 " in text and f"{(m // 501 + 1) * 501} cells" in text and f"limit of {m} cells" in text
    # the check of the group arrays comes first: its text, not the limit's
    rc, text, _, _ = refused_call(L, group_n=[m, 3], group_tours=[1, 1])
    assert rc == -1 and "group 1 has n = 3" in text


def test_check_tsp_local_search_mode_gives_every_combination_its_answer():
    from difusco_amd import decode, pipeline
    assert decode.TSP_LOCAL_SEARCH_MODES == ("launches", "resident")
    assert decode.check_tsp_local_search_mode("2opt+oropt", "resident") == "resident"
    for search in decode.LOCAL_SEARCHES:
        assert decode.check_tsp_local_search_mode(search, "launches") == "launches"
        if search != "2opt+oropt":
            with pytest.raises(ValueError) as e:
                decode.check_tsp_local_search_mode(search, "resident")
            assert "'resident'" in str(e.value) and repr(search) in str(e.value) and "needs local_search='2opt+oropt'" in str(e.value)
    for mode in ("persistent", "", None):
        with pytest.raises(ValueError) as e:
            decode.check_tsp_local_search_mode("2opt+oropt", mode)
        assert "one of" in str(e.value) and repr(mode) in str(e.value)
    pts = np.zeros((8, 2))
    # before any GPU work: there is no model to touch
    with pytest.raises(ValueError, match="needs local_search='2opt\\+oropt'"):
        pipeline.solve_tsp(None, pts, -1, local_search_mode="resident")
    with pytest.raises(ValueError, match="needs local_search='2opt\\+oropt'"):
        pipeline.solve_tsp_batch(None, pts[None], -1, local_search="multi2opt+oropt", local_search_mode="resident")
    with pytest.raises(ValueError, match="needs local_search='2opt\\+oropt'"):
        pipeline.solve_tsp_batch(None, [pts, pts[:5]], -1, local_search="2opt", local_search_mode="resident")
    with pytest.raises(ValueError, match="one of"):
        pipeline.solve_tsp(None, pts, -1, local_search="2opt+oropt", local_search_mode="blocks")
    with pytest.raises(ValueError, match="one of"):
        pipeline.solve_tsp_batch(None, pts[None], -1, local_search="2opt+oropt", local_search_mode="blocks")
    # both resident modes at once: the 2-opt one has no form for this search, whatever the other says
    with pytest.raises(ValueError, match="needs local_search='2opt'"):
        pipeline.solve_tsp(None, pts, -1, local_search="2opt+oropt", two_opt_mode="resident", local_search_mode="resident")
    with pytest.raises(ValueError, match="needs local_search='2opt'"):
        pipeline.solve_tsp_batch(None, [pts], -1, local_search="2opt+oropt", two_opt_mode="resident", local_search_mode="resident")


def test_the_old_check_two_opt_mode_refusals_still_hold():
    from difusco_amd import decode
    assert decode.check_tsp_local_search_mode("2opt", "launches") == "launches"          # the new check exists beside the old one
    assert decode.check_two_opt_mode("2opt", "resident") == "resident"
    for search in decode.LOCAL_SEARCHES:
        assert decode.check_two_opt_mode(search, "launches") == "launches"
        if search != "2opt":
            with pytest.raises(ValueError, match="needs local_search='2opt'"):
                decode.check_two_opt_mode(search, "resident")


def test_the_wrappers_check_the_mode_before_any_gpu_work():
    from difusco_amd import decode
    pts, tour = np.zeros((5, 2)), np.array([[0, 1, 2, 3, 4, 0]])
    for fn, args in ((decode.batched_local_search_torch, (pts, tour)), (decode.batched_local_search_grouped, (pts[None], tour)),
                     (decode.batched_local_search_ragged, ([pts], [tour]))):
        with pytest.raises(ValueError, match="one of"):
            fn(*args, device="cuda:0", mode="blocks")
        with pytest.raises(decode._lib.DifuscoHipError, match="GPU only"):
            fn(*args, device="cpu", mode="resident", steps_per_launch=3)


def test_evaluate_accepts_the_flag_and_refuses_it_with_mis_and_the_other_searches(capsys):
    from difusco_amd import evaluate as EV
    base = ["--storage_path", "x", "--do_test", "--ckpt_path", "c"]
    tsp = base + ["--task", "tsp"]
    args, _ = EV.parse_args(tsp)
    assert args.tsp_local_search_mode == "launches"
    args, _ = EV.parse_args(tsp + ["--local_search", "2opt+oropt", "--tsp_local_search_mode", "resident"])
    assert (args.tsp_local_search_mode, args.local_search, args.two_opt_mode) == ("resident", "2opt+oropt", "launches")
    args, _ = EV.parse_args(base + ["--task", "mis", "--tsp_local_search_mode", "launches"])
    assert args.tsp_local_search_mode == "launches"
    with pytest.raises(SystemExit) as e:
        EV.parse_args(base + ["--task", "mis", "--local_search", "2opt+oropt", "--tsp_local_search_mode", "resident"])
    assert e.value.code == 2 and "--task tsp" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        EV.parse_args(tsp + ["--tsp_local_search_mode", "resident"])                      # the default search is 2opt
    assert e.value.code == 2 and "--local_search 2opt+oropt" in capsys.readouterr().err
    for search in ("2opt", "multi2opt", "multi2opt+oropt"):
        with pytest.raises(SystemExit) as e:
            EV.parse_args(tsp + ["--tsp_local_search_mode", "resident", "--local_search", search])
        assert e.value.code == 2 and "--local_search 2opt+oropt" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        EV.parse_args(tsp + ["--local_search", "2opt+oropt", "--tsp_local_search_mode", "blocks"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err
    import inspect
    assert inspect.signature(EV.solve_split).parameters["tsp_local_search_mode"].default == "launches"
