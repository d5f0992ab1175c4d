"""Fenced device buffers for the GPU entries (a helper module like tests/workspace_poison.py: no conftest, nothing collected).

Every GPU entry of the library writes into buffers that the Python layer allocates with ``torch.empty`` / ``torch.zeros`` or uploads
with ``decode._dev``.  The caching allocator rounds every block up to 512 bytes and packs blocks into large segments, so a store
past the end of an output, or past the bytes a ``_workspace_bytes`` function declared, lands in allocator slack or in a neighbouring
live tensor: no fault, and no wrong result in the test that made the call.  ``Fence`` hands out buffers whose neighbours are known:

    [ lead guard | payload | tail guard ]      one ``uint8`` backing allocation per buffer

The payload starts a multiple of 512 bytes (the allocator's alignment; the library's ``Carver`` assumes 256) from the base of the
backing allocation; the tail guard starts at the byte right after the payload, whatever the payload's size; both guards (and the
payload, until the caller fills it) hold seeded random bytes, so that a stray store of 0, of -1 or of NaN does not match its guard.
The default guard of 256 KiB is one 256-edge workgroup of H = 256 floats, the largest unit any kernel of the library writes per
workgroup: an index that is one tile off still lands in a guard.  ``Fence.check`` raises when a guard byte changed and names the
buffer, the number of changed bytes and their first offsets relative to the payload (``-k``: k bytes before its start, ``+k``: k
bytes past its end).  ``snapshot`` / ``unchanged`` compare the bytes of an input before and after a call.

Three hooks put the fence under the wrappers (all through ``monkeypatch``: undone when the test ends):

``fence_allocations``  ``torch.empty`` / ``torch.zeros`` with the fence's device return fenced buffers: the step's outputs and
                       ``gn_sums``, the buffers of ``engine.prepare`` / ``gen_table`` / ``prepare_times``, the ``edge_index`` of
                       ``knn_edge_index_gpu`` and every ``_workspace`` of ``decode.py``, ``graph.py`` and ``engine.py`` - each with
                       exactly the bytes its size function declared;
``fence_uploads``      ``decode._dev``, the one upload path of the decode, search and MIS wrappers: uploads land in fenced buffers
                       and their host copy is kept for the unchanged check;
``fresh_engine_workspace``  ``DenoiseEngine._workspace`` caches one buffer per stream: the cache is cleared so that the next call
                       allocates it, under the patch, at exactly ``difusco_workspace_bytes(...)``.

What a fence cannot see.  Only ``backend="ctypes"`` is in reach: the torch custom ops (csrc/torch_ops.cpp) allocate their outputs
in C++, where no Python hook applies.  And an overrun from one carved piece of a workspace into the next piece of the SAME
workspace stays inside the payload: tests/test_gpu_workspace_contents.py (results do not depend on what the scratch held) is
what covers that."""
import sys

import numpy as np
import torch

GUARD_BYTES = 256 << 10      # one 256-edge workgroup x 256 floats
ALIGN = 512                  # the caching allocator's block alignment
KEEP_INITIAL = 1 << 20       # payloads up to this size keep a copy of their first contents (``Fence.untouched``)


class FenceError(AssertionError):
    pass


def _bytes_of(t):
    """The bytes of a contiguous tensor as a flat ``uint8`` view (NaN payloads and -0.0 compare as what they are)."""
    assert t.is_contiguous()
    if t.numel() == 0:           # (an empty tensor may carry a stride of 0, which ``view`` refuses)
        return torch.empty(0, dtype=torch.uint8, device=t.device)
    return t.reshape(-1).view(torch.uint8)


def snapshot(t):
    """A copy of the bytes of ``t``."""
    return _bytes_of(t).clone()


def unchanged(t, snap):
    """Does ``t`` hold exactly the bytes of ``snap``?  Compared as ``uint8``: a NaN equals itself, -0.0 is not +0.0."""
    now = _bytes_of(t)
    return now.numel() == snap.numel() and bool(torch.equal(now, snap.to(now.device)))


class _Buffer:
    def __init__(self, name, backing, lead, nbytes, guards, tensor):
        self.name, self.backing, self.lead, self.nbytes, self.guards, self.tensor = name, backing, lead, nbytes, guards, tensor
        self.initial = None      # the random bytes the payload started with (payloads of at most KEEP_INITIAL bytes)
        self.host = None         # fence_uploads: the bytes that were uploaded
        self.label = None        # fence_uploads: who uploaded it

    def changed(self):
        """Offsets (relative to the payload: negative before its start, >= 0 past its end) of the guard bytes that changed."""
        lead_now, tail_now = self.backing[:self.lead], self.backing[self.lead + self.nbytes:]
        if torch.equal(lead_now, self.guards[0]) and torch.equal(tail_now, self.guards[1]):
            return [], []
        before = (lead_now != self.guards[0]).nonzero().reshape(-1) - self.lead
        after = (tail_now != self.guards[1]).nonzero().reshape(-1)
        return before.cpu().tolist(), after.cpu().tolist()


class Fence:
    def __init__(self, device, guard_bytes=GUARD_BYTES, seed=20240917):
        self.device = torch.device(device)
        self.guard_bytes = int(guard_bytes)
        assert self.guard_bytes > 0
        self.lead = (self.guard_bytes + ALIGN - 1) // ALIGN * ALIGN
        self.rng = np.random.default_rng(seed)
        self.buffers = []
        self._snaps = []
        self._empty = torch.empty          # the allocator itself, whatever is patched over ``torch.empty`` later

    # ---- allocation ------------------------------------------------------------------------------------------------------------
    def alloc_bytes(self, n, name=None):
        return self.alloc((int(n),), torch.uint8, name)

    def alloc(self, shape, dtype, name=None):
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        item = self._empty(0, dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        total = self.lead + nbytes + self.guard_bytes
        host = torch.from_numpy(self.rng.integers(0, 256, total, dtype=np.uint8))
        backing = self._empty(total, dtype=torch.uint8, device=self.device)
        backing.copy_(host)
        guards = (backing[:self.lead].clone(), backing[self.lead + nbytes:].clone())
        tensor = backing[self.lead:self.lead + nbytes].view(dtype).reshape(shape)
        if name is None:
            name = f"buffer {len(self.buffers)} ({str(dtype).replace('torch.', '')}{list(shape)})"
        self.buffers.append(_Buffer(name, backing, self.lead, nbytes, guards, tensor))
        if nbytes <= KEEP_INITIAL:
            self.buffers[-1].initial = backing[self.lead:self.lead + nbytes].clone()
        return tensor

    def untouched(self, t):
        """Does the payload of ``t`` still hold the random bytes it was handed out with?  (Payloads of at most KEEP_INITIAL bytes.)"""
        b = self.buffer_of(t)
        return bool(torch.equal(b.backing[b.lead:b.lead + b.nbytes], b.initial))

    def put(self, t, name=None):
        """A fenced copy of ``t`` (any device) on the fence's device."""
        t = t.detach().contiguous()
        out = self.alloc(t.shape, t.dtype, name)
        out.copy_(t)
        return out

    def buffer_of(self, t):
        for b in self.buffers:
            if b.tensor is t or (b.nbytes and b.tensor.data_ptr() == t.data_ptr() and b.tensor.numel() == t.numel()):
                return b
        return None

    @property
    def nbytes(self):
        return sum(b.nbytes for b in self.buffers)

    # ---- inputs ------------------------------------------------------------------------------------------------------------------
    def snapshot(self, t):
        """Remember the bytes of ``t`` as they are now (and return them)."""
        snap = snapshot(t)
        self._snaps = [(u, s) for u, s in self._snaps if u is not t] + [(t, snap)]
        return snap

    def unchanged(self, t, snap=None):
        """Are the bytes of ``t`` those of ``snap`` (default: of the last ``snapshot(t)``)?"""
        if snap is None:
            (snap,) = [s for u, s in self._snaps if u is t]
        return unchanged(t, snap)

    # ---- the check ----------------------------------------------------------------------------------------------------------------
    def check(self, what=""):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        found = []
        for b in self.buffers:
            before, after = b.changed()
            if before or after:
                offs = [f"{o}" for o in before[:16]] + [f"+{o}" for o in after[:16]]
                found.append(f"{b.name} ({b.nbytes} bytes): {len(before) + len(after)} guard bytes changed, first at {', '.join(offs)}")
        if found:
            raise FenceError(f"{what}: stores outside a buffer\n  " + "\n  ".join(found))

    def changed_offsets(self, t):
        """(offsets before the payload, offsets past it) of the guard bytes of ``t``'s buffer that changed."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return self.buffer_of(t).changed()


# ---- the hooks ---------------------------------------------------------------------------------------------------------------------
def _is_fenced_device(fence, device):
    if device is None or fence.device.type != "cuda":
        return False
    device = torch.device(device)
    if device.type != "cuda":
        return False
    index = torch.cuda.current_device() if device.index is None else device.index
    return index == (0 if fence.device.index is None else fence.device.index)


def fence_allocations(monkeypatch, fence):
    """``torch.empty`` / ``torch.zeros`` with ``device=`` the fence's CUDA device return ``fence.alloc(...)`` (zeroed for ``zeros``);
    every other call - CPU tensors, no device, ``out=`` or another layout - goes to the original untouched.  -> the list the fenced
    tensors are appended to."""
    made = []
    plain = {"dtype", "device", "requires_grad"}

    def patched(orig, zero):
        def fn(*size, **kw):
            if not _is_fenced_device(fence, kw.get("device")) or set(kw) - plain or kw.get("requires_grad"):
                return orig(*size, **kw)
            shape = size[0] if len(size) == 1 and not isinstance(size[0], (int, np.integer)) else size
            dtype = kw.get("dtype") or torch.get_default_dtype()
            t = fence.alloc(tuple(shape), dtype)
            if zero:
                t.zero_()
            made.append(t)
            return t
        return fn
    monkeypatch.setattr(torch, "empty", patched(torch.empty, False))
    monkeypatch.setattr(torch, "zeros", patched(torch.zeros, True))
    return made


def fence_uploads(monkeypatch, fence):
    """``decode._dev(x, dtype, device)`` uploads into a fenced buffer; the buffer's record keeps the uploaded bytes (``host``) and
    who uploaded it (``label``: ``<function of decode.py>:<dtype>#<k>``, k counting that function's uploads of that dtype within
    one test).  -> the list of those records."""
    from difusco_amd import decode
    records, seen = [], {}

    def _dev(x, dtype, device):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if not _is_fenced_device(fence, device):
            return x.to(device=device, dtype=dtype).contiguous()
        code = sys._getframe(1).f_code
        who = f"{getattr(code, 'co_qualname', code.co_name)}:{str(dtype).replace('torch.', '')}"
        seen[who] = seen.get(who, -1) + 1
        host = x.detach().to(device="cpu", dtype=dtype).contiguous()
        t = fence.put(host, name=f"upload {who}#{seen[who]} {list(host.shape)}")
        rec = fence.buffers[-1]
        rec.host, rec.label = _bytes_of(host).clone(), f"{who}#{seen[who]}"
        records.append(rec)
        return t
    monkeypatch.setattr(decode, "_dev", _dev)
    return records


def fresh_engine_workspace(eng):
    """Forget the cached step workspaces of a ``DenoiseEngine``: the next call allocates one of exactly the declared size."""
    eng._ws.clear()
