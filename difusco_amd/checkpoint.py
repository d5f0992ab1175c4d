"""Checkpoints of the reference for the evaluation runner (``evaluate.py``): a Lightning ``.ckpt`` as ``trainer.fit`` writes it
(``{"state_dict": {"model.…": …}, "optimizer_states": …, ...}``; ``COMetaModel.model`` is the ``GNNEncoder``) or a file that
holds the bare ``GNNEncoder`` state dict."""
import pickle
import re

import torch

from .weights import infer_config, strip_prefix


class CheckpointError(ValueError):
    """A checkpoint that cannot be evaluated with the given arguments, or that would need full unpickling."""


def load_checkpoint(path: str, allow_unsafe: bool = False) -> dict:
    """-> the ``GNNEncoder`` state dict (CPU tensors, keys without Lightning's ``model.`` prefix).  Loaded with
    ``torch.load(..., map_location="cpu", weights_only=True)``; a file that needs full unpickling (Python objects beside the
    tensors) is refused with the global that stopped it, unless ``allow_unsafe`` - for trusted files only: full unpickling can
    run arbitrary code."""
    try:
        obj = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as exc:
        if not allow_unsafe:
            m = re.search(r"GLOBAL (\S+) was not an allowed global", str(exc))
            what = f"it holds the global {m.group(1)}" if m else str(exc).strip().splitlines()[0]
            raise CheckpointError(f"{path}: needs full unpickling ({what}); refused - pass --unsafe_checkpoint_load "
                                  "only for a file you trust") from None
        obj = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(obj, dict) and isinstance(obj.get("state_dict"), dict):
        obj = obj["state_dict"]
    if not isinstance(obj, dict) or not obj or not all(isinstance(v, torch.Tensor) for v in obj.values()):
        raise CheckpointError(f"{path}: neither a Lightning checkpoint nor a state dict of tensors")
    state = strip_prefix(obj)
    if "node_embed.weight" not in state or "out.2.weight" not in state:
        raise CheckpointError(f"{path}: no GNNEncoder weights (node_embed.weight / out.2.weight missing)")
    return state


def check_config(state: dict, hidden_dim: int, n_layers: int, diffusion_type: str):
    """``weights.infer_config`` of the checkpoint against ``--hidden_dim``, ``--n_layers`` and the output channels of
    ``--diffusion_type`` (categorical 2, gaussian 1): one ``CheckpointError`` naming both values of every mismatch (the
    reference fails later, inside ``load_state_dict``).  Returns (hidden, n_layers, out_channels)."""
    hidden, layers, out = infer_config(state)
    want_out = {"categorical": 2, "gaussian": 1}.get(diffusion_type)
    bad = []
    if hidden != int(hidden_dim):
        bad.append(f"hidden size {hidden} in the checkpoint, --hidden_dim {hidden_dim}")
    if layers != int(n_layers):
        bad.append(f"{layers} layers in the checkpoint, --n_layers {n_layers}")
    if want_out is not None and out != want_out:
        bad.append(f"{out} output channels in the checkpoint, --diffusion_type {diffusion_type} needs {want_out}")
    if bad:
        raise CheckpointError("the checkpoint does not match the arguments: " + "; ".join(bad))
    return hidden, layers, out
