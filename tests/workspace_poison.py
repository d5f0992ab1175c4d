"""Chosen scratch contents for the GPU entries (a helper module like tests/graph_zoo.py: no conftest, nothing collected from it).

Every GPU entry of the library works in caller-provided scratch, which the Python layer allocates with ``torch.empty``: in
production those bytes are whatever the caching allocator last held there.  ``Arena`` is one device buffer that stands in for
that memory and whose contents the test chooses before a call:

``zeros``    every byte 0;
``ones``     every byte 0xFF: NaN as a float, -1 as an int, the largest value as an unsigned counter;
``random``   bytes of a seeded numpy generator;
``residue``  no refill: what the calls before left there (the tests run a different, larger case of the same entry first).

``patch_decode`` / ``patch_graph`` hand ``arena[:nbytes]`` to every call of ``difusco_amd.decode`` / ``graph`` + ``formats``
(refilled before EACH call, so a later call of one run never sees an earlier call's residue unless the fill is ``residue``);
``give_to_engine`` makes the arena the step workspace of a ``DenoiseEngine`` on the current stream.  ``Arena.check_used`` is the
proof that the poison was in play: the calls were counted, and the bytes the last call was handed differ from their fill."""
import ctypes

import numpy as np
import torch

FILLS = ("zeros", "ones", "random", "residue")
POISONS = FILLS[1:]


class Arena:
    def __init__(self, dev, nbytes, seed=20240611):
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        self.seed = seed
        self._pattern = None
        self.how = "zeros"
        self.calls = []          # bytes handed out since the last set()

    @property
    def nbytes(self):
        return self.buf.numel()

    def pattern(self):
        """The random bytes, generated once on the host from the seed and kept on the device."""
        if self._pattern is None:
            host = np.random.default_rng(self.seed).integers(0, 256, self.nbytes, dtype=np.uint8)
            self._pattern = torch.from_numpy(host).to(self.buf.device)
        return self._pattern

    def _refill(self, nbytes):
        if self.how == "zeros":
            self.buf[:nbytes].zero_()
        elif self.how == "ones":
            self.buf[:nbytes].fill_(0xFF)
        elif self.how == "random":
            self.buf[:nbytes].copy_(self.pattern()[:nbytes])
        elif self.how != "residue":
            raise ValueError(self.how)

    def set(self, how, whole=True):
        """Choose the fill of the calls that follow; ``whole``: write it over the whole arena now (not for ``residue``)."""
        if how not in FILLS:
            raise ValueError(how)
        self.how = how
        self.calls = []
        if whole:
            self._refill(self.nbytes)

    def take(self, nbytes):
        """The workspace of one call: the first ``nbytes`` bytes, refilled."""
        assert nbytes <= self.nbytes, f"the arena holds {self.nbytes} bytes, the call needs {nbytes}"
        self.calls.append(int(nbytes))
        if nbytes == 0:      # what torch.empty(0) is to the library: no buffer at all
            return torch.empty(0, dtype=torch.uint8, device=self.buf.device)
        self._refill(nbytes)
        return self.buf[:nbytes]

    def still_filled(self, nbytes):
        """Do the first ``nbytes`` bytes hold exactly what the fill wrote?  (Not defined for ``residue``.)"""
        got = self.buf[:nbytes]
        if self.how == "zeros":
            return not bool(got.any())
        if self.how == "ones":
            return bool((got == 0xFF).all())
        if self.how == "random":
            return torch.equal(got, self.pattern()[:nbytes])
        raise ValueError("residue has no fill to compare with")

    def check_used(self, calls=None, at_least=1, written=True):
        """The poison was in play: ``calls`` workspaces were handed out (or ``at_least``), and where the last one had bytes and the
        fill is ``ones`` or ``random``, the call wrote some of them (a call may well write nothing but zeros, and ``residue`` has
        no fill to compare with).  ``written=False``: the call is known to return before it touches the device, which is shown."""
        torch.cuda.synchronize(self.buf.device)
        if calls is not None:
            assert len(self.calls) == calls, (len(self.calls), calls)
        assert len(self.calls) >= at_least, self.calls
        last = self.calls[-1]
        if last > 0 and self.how in ("ones", "random"):
            assert self.still_filled(last) != written, \
                f"{last} bytes of workspace, {self.how} fill: the call {'did not write' if written else 'wrote'} them"


def patch_decode(monkeypatch, arena):
    """Every ``decode._workspace`` call (all the decode, search and MIS wrappers) gets the arena."""
    from difusco_amd import _lib, decode

    def _workspace(size_fn, *sizes, device):
        nbytes = ctypes.c_size_t()
        _lib.check(size_fn(*sizes, ctypes.byref(nbytes)))
        assert torch.device(device) == arena.buf.device
        return arena.take(nbytes.value), nbytes.value
    monkeypatch.setattr(decode, "_workspace", _workspace)


def patch_graph(monkeypatch, arena):
    """Every ``graph._workspace`` call (the device graph build, the k-NN graph, the MCTS heat map) gets the arena."""
    from difusco_amd import graph

    def _workspace(nbytes, device):
        assert torch.device(device) == arena.buf.device
        return arena.take(nbytes)
    monkeypatch.setattr(graph, "_workspace", _workspace)


def give_to_engine(eng, arena, stream=None):
    """The arena as the step workspace of ``eng`` on ``stream`` (default: the current one): ``eng._workspace`` keeps one buffer per
    stream and reuses any that is large enough."""
    key = (torch.cuda.current_stream(eng.device) if stream is None else stream).cuda_stream
    eng._ws[key] = arena.buf
    return key
