"""The argument checks of the resident MIS search (``difusco_mis_resident_search``, one GPU block per instance) that need no GPU:
the limit, the workspace size, the refusals of the library entry before any GPU work, ``check_mis_search_mode``, the
``local_search_mode`` of the solvers and the runner's ``--mis_local_search_mode``."""
import ctypes

import numpy as np
import pytest


def test_the_limit_is_a_constant_of_at_least_2048_nodes():
    from difusco_amd import _lib
    L = _lib.lib()
    assert L.difusco_mis_resident_max_nodes() >= 2048
    assert L.difusco_mis_resident_max_nodes() == L.difusco_mis_resident_max_nodes()


def test_workspace_bytes_checks_its_arguments_and_grows_with_kicks():
    from difusco_amd import _lib
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    #           n  edges B kicks
    for bad in ((0, 0, 1, 3), (5, -1, 1, 3), (5, 8, 0, 3), (5, 8, -1, 3), (5, 8, 1, -1)):
        assert L.difusco_mis_resident_search_workspace_bytes(*bad, ctypes.byref(nbytes)) == -1, bad
    assert L.difusco_mis_resident_search_workspace_bytes(5, 8, 2, 3, None) == -1
    sizes = []
    for kicks in (0, 100, 10_000):
        assert L.difusco_mis_resident_search_workspace_bytes(5, 8, 2, kicks, ctypes.byref(nbytes)) == 0
        sizes.append(nbytes.value)
    assert sizes[0] < sizes[1] < sizes[2] and sizes[2] >= 4 * 10_001                 # an int32 per descent
    launched = ctypes.c_size_t()
    for n, edges, B, kicks in ((5, 8, 2, 0), (5, 8, 2, 50), (64, 400, 4, 1000)):
        assert L.difusco_mis_iterated_search_workspace_bytes(n, edges, B, ctypes.byref(launched)) == 0
        assert L.difusco_mis_resident_search_workspace_bytes(n, edges, B, kicks, ctypes.byref(nbytes)) == 0
        assert nbytes.value >= launched.value


def test_library_argument_checks_come_before_any_gpu_work():
    from difusco_amd import _lib
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    assert L.difusco_mis_resident_search_workspace_bytes(5, 8, 2, 3, ctypes.byref(nbytes)) == 0
    p = ctypes.c_void_p(0x1000)
    counters = (ctypes.c_int32 * 3)()
    #     n  rowptr col scores sol B rows seeds offsets kicks kick_size max_rounds kicks_per_launch ws bytes counters per stream
    ok = [5, p, p, p, p, 2, p, p, p, 3, 4, 10, 0, p, 1 << 20, counters, None, None]
    for i, v in ((0, 0), (1, None), (2, None), (3, None), (4, None), (5, 0), (6, None), (7, None), (8, None), (13, None),
                 (15, None), (14, nbytes.value - 1)):
        bad = list(ok)
        bad[i] = v
        assert L.difusco_mis_resident_search(*bad) == -1, i
    for i, word in ((9, b"kicks"), (10, b"kick_size"), (11, b"max_rounds"), (12, b"kicks_per_launch")):
        bad = list(ok)
        bad[i] = -1 if i != 10 else 0
        assert L.difusco_mis_resident_search(*bad) == -1 and word in L.difusco_last_error(), i


def test_the_resident_mode_needs_the_swap_search():
    from difusco_amd import decode, pipeline
    assert decode.MIS_SEARCH_MODES == ("launches", "resident")
    assert decode.check_mis_search_mode("swap", "resident") == "resident"
    assert decode.check_mis_search_mode("none", "launches") == "launches"
    with pytest.raises(ValueError, match="swap"):
        decode.check_mis_search_mode("none", "resident")
    for mode in ("persistent", "", None):
        with pytest.raises(ValueError, match="one of"):
            decode.check_mis_search_mode("swap", mode)
    none = np.zeros((2, 0), dtype=np.int64)
    # before any GPU work: there is no model to touch
    with pytest.raises(ValueError, match="swap"):
        pipeline.solve_mis(None, 3, none, local_search_mode="resident")
    with pytest.raises(ValueError, match="swap"):
        pipeline.solve_mis_batch(None, [(3, none)], local_search="none", local_search_mode="resident")
    with pytest.raises(ValueError, match="one of"):
        pipeline.solve_mis(None, 3, none, local_search="swap", local_search_mode="blocks")


def test_the_search_entry_checks_mode_and_kicks_per_launch_on_the_host():
    from difusco_amd.decode import mis_iterated_search_np
    from test_mis_local_search_host import sym
    sc, ei = np.array([.5, .9, .4], dtype=np.float32), sym(3, [(0, 1), (1, 2)])
    with pytest.raises(ValueError, match="one of"):
        mis_iterated_search_np(sc, [0, 1, 0], edge_index=ei, kicks=1, device="cuda:0", mode="blocks")
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="kicks_per_launch"):
            mis_iterated_search_np(sc, [0, 1, 0], edge_index=ei, kicks=1, device="cuda:0", mode="resident", kicks_per_launch=bad)


def test_evaluate_refuses_the_mode_without_swap_with_tsp_and_unknown(capsys):
    from difusco_amd import evaluate as EV
    base = ["--storage_path", "x", "--do_test", "--ckpt_path", "c"]
    mis = base + ["--task", "mis"]
    args, _ = EV.parse_args(mis)
    assert args.mis_local_search_mode == "launches"
    args, _ = EV.parse_args(mis + ["--mis_local_search", "swap", "--mis_local_search_mode", "resident"])
    assert (args.mis_local_search_mode, args.mis_local_search_kicks) == ("resident", 0)       # kicks = 0 is allowed
    args, _ = EV.parse_args(mis + ["--mis_local_search_mode", "launches"])
    assert args.mis_local_search_mode == "launches"
    with pytest.raises(SystemExit) as e:
        EV.parse_args(mis + ["--mis_local_search_mode", "resident"])
    assert e.value.code == 2 and "--mis_local_search swap" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        EV.parse_args(base + ["--task", "tsp", "--mis_local_search_mode", "resident"])
    assert e.value.code == 2 and "--task mis" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        EV.parse_args(mis + ["--mis_local_search", "swap", "--mis_local_search_mode", "blocks"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err
