"""CPU tests of graphed sampling: the C entry point with a device-side Philox offset shift (difusco_denoise_step_shifted) is
declared, exported and validates its argument block before any GPU work; the step ops carry the trailing offset_shift
argument; the sampling entry points and the pipeline take a keyword-only ``graphed`` that defaults to False."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from difusco_amd import _lib
from tests import test_batch_host as BH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_shifted_step():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "difusco_hip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+difusco_denoise_step_shifted\s*\(([^)]*)\)\s*;", hdr)
    assert decl is not None
    assert re.sub(r"\s+", " ", decl.group(1)).strip() == "const difusco_step_args* args, const uint64_t* offset_shift"
    assert not re.search(r"#ifdef DIFUSCO_PROFILING[^#]*difusco_denoise_step_shifted", hdr)      # production symbol
    assert hasattr(_lib.lib(), "difusco_denoise_step_shifted")
    assert _lib.ABI_VERSION == 13 and _lib.lib().difusco_abi_version() == 13      # additive: no ABI bump


@pytest.mark.parametrize("bad", [dict(n_instances=0), dict(n_instances=-1), dict(instance_rows=None),
                                 dict(instance_seeds=None), dict(rand_mode=4)])
def test_shifted_step_validates_before_gpu_work(bad):
    L = _lib.lib()
    rc = L.difusco_denoise_step_shifted(ctypes.byref(BH._args(**bad)), ctypes.c_void_p(0x4000))   # never dereferenced
    assert rc == -1        # DIFUSCO_EINVAL
    msg = L.difusco_last_error().decode()
    assert "PHILOX_INSTANCES" in msg or "unknown rand_mode" in msg, msg


def test_shifted_step_refuses_a_null_block_and_an_abi_mismatch():
    L = _lib.lib()
    assert L.difusco_denoise_step_shifted(None, ctypes.c_void_p(0x4000)) == -1
    a = BH._args()
    a.abi_version = 12
    assert L.difusco_denoise_step_shifted(ctypes.byref(a), ctypes.c_void_p(0x4000)) == -1
    assert "ABI mismatch" in L.difusco_last_error().decode()


def _ops():
    from difusco_amd import torch_ops
    return torch_ops.load()


@pytest.mark.parametrize("name", ["denoise_step_categorical", "denoise_step_gaussian"])
def test_step_schema_ends_with_offset_shift(name):
    schema = str(getattr(_ops(), name).default._schema)
    assert schema.endswith("Tensor? instance_seeds=None, Tensor? offset_shift=None) -> (Tensor, Tensor, Tensor)"), schema


def test_step_op_has_no_cpu_kernel():
    """The step ops accept the trailing offset_shift positionally but have no CPU kernel (every step input must live on the GPU).
    The shim's own offset_shift checks (dtype, one element, device) need a GPU step: tests/test_gpu_graphed_sampling.py."""
    ops = _ops()
    f = torch.zeros(16)
    i = torch.zeros(5, dtype=torch.int32)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ops.denoise_step_categorical(f, i, i, None, None, None, f, f, 1.0, [0.0] * 5, None, 0, 0, f,
                                     [256, 12, 2, 0, 3, 0, 1, 0, 0], False, False, None, None, None, None, None, None,
                                     torch.zeros(1, dtype=torch.int64))


def _kw_only_false(fn, name="graphed"):
    p = inspect.signature(fn).parameters[name]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_sampling_entry_points_take_keyword_only_graphed():
    from difusco_amd import models, pipeline
    for fn in (models.TSPModel.sample, models.MISModel.sample, pipeline.solve_tsp, pipeline.solve_mis):
        _kw_only_false(fn)
    # the positional prefix of each is unchanged
    assert list(inspect.signature(models.TSPModel.sample).parameters)[:5] == ["self", "points", "edge_index", "xt0", "generator"]
    assert list(inspect.signature(models.MISModel.sample).parameters)[:5] == ["self", "n_nodes", "edge_index", "xt0", "generator"]


def test_engine_step_takes_offset_shift():
    from difusco_amd.engine import DenoiseEngine
    p = inspect.signature(DenoiseEngine.step).parameters["offset_shift"]
    assert p.default is None
