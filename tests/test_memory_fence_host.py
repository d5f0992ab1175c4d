"""tests/memory_fence.py on CPU tensors: the layout of a fenced buffer, what ``check`` reports and what ``unchanged`` sees."""
import numpy as np
import pytest
import torch

import memory_fence as MF

CPU = torch.device("cpu")


@pytest.mark.parametrize("guard", [MF.GUARD_BYTES, 512, 100])
@pytest.mark.parametrize("shape,dtype", [((33,), torch.float32), ((7, 3), torch.int64), ((1,), torch.uint8), ((1001,), torch.uint8),
                                         ((5,), torch.float64), ((0,), torch.int32), ((3, 0), torch.float32)])
def test_layout_alignment_and_odd_sizes(shape, dtype, guard):
    f = MF.Fence(CPU, guard_bytes=guard)
    t = f.alloc(shape, dtype)
    b = f.buffers[-1]
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and b.nbytes == n
    assert b.backing.dtype == torch.uint8 and b.backing.numel() == b.lead + n + guard
    assert b.lead % 512 == 0 and b.lead >= guard                      # the payload starts a multiple of 512 bytes from the base,
    assert t.data_ptr() - b.backing.data_ptr() == b.lead or n == 0    # behind a lead guard of at least the guard size,
    assert b.guards[0].numel() == b.lead and b.guards[1].numel() == guard      # and the tail guard starts right behind it:
    if n:
        assert t.reshape(-1).view(torch.uint8).data_ptr() + n == b.backing[b.lead + n:].data_ptr()
    f.check("untouched")
    t.copy_(torch.ones(shape).to(dtype))                               # writing the whole payload touches no guard
    f.check("payload written")


def test_alloc_bytes_and_names():
    f = MF.Fence(CPU, guard_bytes=512)
    t = f.alloc_bytes(1001, name="scratch")
    assert t.dtype == torch.uint8 and t.shape == (1001,) and f.buffers[0].name == "scratch" and f.nbytes == 1001
    assert f.buffer_of(t) is f.buffers[0] and f.buffer_of(t.reshape(-1)) is f.buffers[0] and f.buffer_of(torch.zeros(3)) is None


def test_guards_are_seeded_random_bytes():
    a, b = MF.Fence(CPU, guard_bytes=4096, seed=5), MF.Fence(CPU, guard_bytes=4096, seed=5)
    a.alloc_bytes(10), b.alloc_bytes(10)
    assert torch.equal(a.buffers[0].backing, b.buffers[0].backing)     # the seed decides them
    c = MF.Fence(CPU, guard_bytes=4096, seed=6)
    c.alloc_bytes(10)
    assert not torch.equal(a.buffers[0].backing, c.buffers[0].backing)
    for g in a.buffers[0].guards:                                      # no constant: every byte value occurs, none dominates
        counts = torch.bincount(g.long(), minlength=256)
        assert int(counts.max()) < 64 and int((counts > 0).sum()) > 250
    a.alloc_bytes(10)
    assert not torch.equal(a.buffers[0].backing, a.buffers[1].backing)  # and the next buffer draws fresh ones


@pytest.mark.parametrize("n", [40, 1001, 0])
def test_check_reports_the_offsets_of_changed_guard_bytes(n):
    f = MF.Fence(CPU, guard_bytes=512)
    t = f.alloc_bytes(n, name="victim")
    b = f.buffers[0]
    f.check("untouched")
    b.backing[b.lead + n] ^= 0x01                                      # the first byte past the payload
    with pytest.raises(MF.FenceError) as exc:
        f.check("one past")
    assert "one past" in str(exc.value) and f"victim ({n} bytes): 1 guard bytes changed, first at +0" in str(exc.value)
    assert f.changed_offsets(t) == ([], [0]) if n else True
    b.backing[b.lead + n] ^= 0x01
    f.check("restored")
    b.backing[b.lead - 1] ^= 0x80                                      # the last byte before it
    with pytest.raises(MF.FenceError) as exc:
        f.check("one before")
    assert f"victim ({n} bytes): 1 guard bytes changed, first at -1" in str(exc.value)
    b.backing[b.lead + n + 511] ^= 0xFF                                # + the last byte of the tail guard, + the first of the lead
    b.backing[0] ^= 0x10
    with pytest.raises(MF.FenceError) as exc:
        f.check("three")
    assert "3 guard bytes changed, first at -512, -1, +511" in str(exc.value)


def test_check_names_every_buffer_that_was_hit():
    f = MF.Fence(CPU, guard_bytes=512)
    f.alloc((3,), torch.float32, name="a"), f.alloc((3,), torch.float32, name="b"), f.alloc((3,), torch.float32, name="c")
    for k in (0, 2):
        b = f.buffers[k]
        b.backing[b.lead + b.nbytes + 4:b.lead + b.nbytes + 8] ^= 0xFF
    with pytest.raises(MF.FenceError) as exc:
        f.check("two of three")
    text = str(exc.value)
    assert "a (12 bytes): 4 guard bytes changed, first at +4, +5, +6, +7" in text and "c (12 bytes)" in text and "b (12 bytes)" not in text


def test_a_stray_zero_minus_one_or_nan_does_not_match_its_guard():
    """A constant guard would hide the store of that constant.  Of 64 float slots behind the payload, every one differs from 0.0,
    from the all-ones pattern and from the canonical NaN."""
    f = MF.Fence(CPU, guard_bytes=512, seed=1)
    f.alloc((4,), torch.float32)
    tail = f.buffers[0].guards[1][:256].view(torch.int32)
    for pattern in (0, -1, 0x7fc00000):
        assert not bool((tail == pattern).any())


def test_unchanged_compares_bytes():
    f = MF.Fence(CPU, guard_bytes=512)
    x = f.alloc((6,), torch.float32)
    x.copy_(torch.tensor([1.0, float("nan"), -0.0, 0.0, float("inf"), -3.5]))
    snap = f.snapshot(x)
    assert f.unchanged(x, snap)                                        # a NaN payload equals itself (== would say no)
    x[2] = 0.0                                                         # -0.0 -> +0.0: == would say yes
    assert not f.unchanged(x, snap)
    x[2] = -0.0
    assert f.unchanged(x, snap)
    x.view(torch.int32)[1] ^= 1                                        # one bit of the NaN's payload
    assert not f.unchanged(x, snap)
    x.view(torch.int32)[1] ^= 1
    x.view(torch.int32)[5] ^= 1 << 31                                  # one sign bit
    assert not f.unchanged(x, snap)
    empty = torch.empty(0, dtype=torch.int32).expand(0)               # no bytes: always unchanged, whatever its strides
    assert f.unchanged(empty, f.snapshot(empty)) and f.unchanged(torch.zeros(3, 0), f.snapshot(torch.zeros(3, 0)))
    y = f.alloc((2, 3), torch.int64)
    snap = f.snapshot(y)
    assert f.unchanged(y)                                              # (without a snapshot: against the last one taken of y)
    y[1, 2] += 1
    assert not f.unchanged(y, snap) and not f.unchanged(y) and snap.dtype == torch.uint8 and snap.numel() == 48
    f.snapshot(y)
    assert f.unchanged(y) and not f.unchanged(y, snap) and not f.unchanged(x)


def test_put_copies_and_fences():
    f = MF.Fence(CPU, guard_bytes=512)
    src = torch.arange(10, dtype=torch.float64).reshape(2, 5).t()      # not contiguous
    t = f.put(src, name="pts")
    assert torch.equal(t, src) and t.is_contiguous() and f.buffers[0].name == "pts"
    f.check("put")


def test_allocation_patch_leaves_cpu_allocations_alone(monkeypatch):
    """``fence_allocations`` on a machine without a GPU: every ``torch.empty`` / ``torch.zeros`` call is a CPU allocation and goes to
    the original untouched, in every call form the wrappers use."""
    f = MF.Fence(CPU, guard_bytes=512)
    empty, zeros = torch.empty, torch.zeros
    made = MF.fence_allocations(monkeypatch, f)
    assert torch.empty is not empty and torch.zeros is not zeros
    for t in (torch.empty(5), torch.empty((2, 3), dtype=torch.int32), torch.empty(2, 3, dtype=torch.float64, device="cpu"),
              torch.zeros(7, dtype=torch.uint8, device=CPU), torch.zeros((2, 2)), torch.empty(0, dtype=torch.uint8),
              torch.empty(4, pin_memory=False), torch.zeros(3, out=empty(3))):
        assert t.device.type == "cpu" and f.buffer_of(t) is None
    assert torch.zeros(4, 2).shape == (4, 2) and not bool(torch.zeros(4, 2).any())
    assert made == [] and f.buffers == []
    monkeypatch.undo()
    assert torch.empty is empty and torch.zeros is zeros


def test_upload_patch_leaves_cpu_uploads_alone(monkeypatch):
    from difusco_amd import decode
    f = MF.Fence(CPU, guard_bytes=512)
    orig = decode._dev
    records = MF.fence_uploads(monkeypatch, f)
    t = decode._dev(np.arange(6).reshape(2, 3), torch.float32, CPU)
    assert t.dtype == torch.float32 and t.shape == (2, 3) and torch.equal(t, orig(np.arange(6).reshape(2, 3), torch.float32, CPU))
    assert records == [] and f.buffers == []
    monkeypatch.undo()
    assert decode._dev is orig
