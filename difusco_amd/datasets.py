"""Readers of the reference's test splits (``difusco/co_datasets``), for the evaluation runner (``evaluate.py``).

* ``read_tsp_split(path)``: the text format of ``TSPGraphDataset`` (``tsp_graph_dataset.py:20-36``), one instance per line:
  ``x1 y1 x2 y2 ... output t1 t2 ... t1`` with a closed, 1-based tour.  Each line gives what ``get_example`` returns - float64
  points [N, 2] (every coordinate is ``float(token)``) and the 0-based closed tour, int64 [N + 1] - and its source
  ``(path, line number)``.  Lines may hold different N.
* ``read_mis_split(pattern, label_dir=None)``: the ``.gpickle`` files of ``MISDataset`` (``mis_dataset.py:23-50``) in
  ``glob.glob(pattern)`` order, so index i is the reference's ``real_batch_idx`` on the same filesystem.  The files are
  unpickled through an allow-list (networkx graph classes, builtin containers, numpy scalars and dtypes); networkx is
  imported here only, and only when a graph is read.

Generators of new data stay out of scope."""
import glob
import os
import pickle
from typing import List, NamedTuple, Optional, Tuple

import numpy as np


class TSPExample(NamedTuple):
    points: np.ndarray            # float64 [N, 2]
    tour: np.ndarray              # int64 [N + 1], 0-based, closed
    source: Tuple[str, int]       # (path, 1-based line number)


class MISExample(NamedTuple):
    n_nodes: int
    labels: np.ndarray            # int64 [n]
    edge_index: np.ndarray        # int64 [2, 2|E| + n]: the edges, their reversed copy, the self loops
    source: Tuple[str, int]       # (path, 0): one graph per file


class SplitFormatError(ValueError):
    """A line or file of a split that the reference's reader could not turn into an instance."""


def parse_tsp_line(line: str, where: str = "<line>"):
    """One line of a TSP split -> (points float64 [N, 2], closed tour int64 [N + 1]), tokenised as ``get_example`` does:
    ``strip``, split on ``" output "``, split on ``" "``.  ``where`` names the line in errors."""
    parts = line.strip().split(" output ")
    if len(parts) != 2:
        raise SplitFormatError(f"{where}: expected '<coordinates> output <tour>', found {len(parts) - 1} ' output ' separators")
    coords, tour_tok = parts[0].split(" "), parts[1].split(" ")
    if len(coords) < 2 or len(coords) % 2:
        raise SplitFormatError(f"{where}: {len(coords)} coordinate tokens, need an even number >= 2")
    try:
        points = np.array([float(t) for t in coords], dtype=np.float64).reshape(-1, 2)
    except ValueError as exc:
        raise SplitFormatError(f"{where}: bad coordinate ({exc})") from None
    try:
        tour = np.array([int(t) for t in tour_tok], dtype=np.int64) - 1
    except ValueError as exc:
        raise SplitFormatError(f"{where}: bad tour index ({exc})") from None
    n = points.shape[0]
    if tour.shape[0] != n + 1 or tour[0] != tour[-1]:
        raise SplitFormatError(f"{where}: the tour must visit the {n} points and return to its start "
                               f"({tour.shape[0]} indices, need {n + 1} with the first repeated last)")
    if tour.min() < 0 or tour.max() >= n:
        raise SplitFormatError(f"{where}: tour index outside 1..{n}")
    return points, tour


def read_tsp_split(path: str, limit: Optional[int] = None) -> List[TSPExample]:
    """Every line of the TSP split at ``path`` (the first ``limit`` lines when given; see the module docstring).  A malformed
    line raises ``SplitFormatError`` naming the file and its 1-based line number."""
    with open(path) as f:
        lines = f.read().splitlines()
    out = []
    for i, line in enumerate(lines[:limit]):
        points, tour = parse_tsp_line(line, where=f"{path}:{i + 1}")
        out.append(TSPExample(points, tour, (path, i + 1)))
    return out


# ---- MIS -----------------------------------------------------------------------------------------------------------------
_BUILTINS = {"set", "frozenset", "dict", "list", "tuple", "int", "float", "complex", "bool", "str", "bytes", "bytearray",
             "object"}
_ALLOWED = {("copyreg", "_reconstructor"), ("collections", "OrderedDict"), ("collections", "defaultdict"),
            ("numpy", "dtype"), ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar")}


class _GraphUnpickler(pickle.Unpickler):
    """Resolves only networkx graph classes (and their views) under ``networkx.classes``, builtin containers and numpy
    scalar / dtype reconstruction; any other global is refused with its name."""

    def find_class(self, module, name):
        if (module == "builtins" and name in _BUILTINS) or (module, name) in _ALLOWED:
            return super().find_class(module, name)
        if module.startswith("networkx.classes.") and not name.startswith("_"):
            obj = super().find_class(module, name)
            if isinstance(obj, type):
                return obj
        raise pickle.UnpicklingError(f"global '{module}.{name}' is not allowed in a graph file")


def load_gpickle(path: str):
    """A networkx graph from ``path`` (``nx.write_gpickle`` / ``pickle.dump`` of a graph) through the allow-list."""
    import networkx  # noqa: F401  (the graph classes resolve through it)
    with open(path, "rb") as f:
        try:
            graph = _GraphUnpickler(f).load()
        except pickle.UnpicklingError as exc:
            raise SplitFormatError(f"{path}: {exc}") from None
    if not hasattr(graph, "number_of_nodes") or not hasattr(graph, "edges"):
        raise SplitFormatError(f"{path}: holds a {type(graph).__name__}, not a networkx graph")
    return graph


def mis_example(graph, path: str, label_dir: Optional[str] = None):
    """``MISDataset.get_example`` (``mis_dataset.py:23-50``) of an already loaded graph -> (n_nodes, labels, edge_index)."""
    n = int(graph.number_of_nodes())
    if label_dir is None:
        labels = [v for _, v in graph.nodes(data="label")]
        labels = np.array(labels, dtype=np.int64) if labels and labels[0] is not None else np.zeros(n, dtype=np.int64)
    else:
        label_file = os.path.join(label_dir, os.path.basename(path).replace(".gpickle", "_unweighted.result"))
        with open(label_file) as f:
            labels = np.array([int(v) for v in f.read().splitlines()], dtype=np.int64)
        if labels.shape[0] != n:
            raise SplitFormatError(f"{label_file}: {labels.shape[0]} labels for {n} nodes")
    edges = np.array(list(graph.edges), dtype=np.int64).reshape(-1, 2)
    edges = np.concatenate([edges, edges[:, ::-1]], axis=0)
    loops = np.arange(n, dtype=np.int64).reshape(-1, 1).repeat(2, axis=1)
    edge_index = np.ascontiguousarray(np.concatenate([edges, loops], axis=0).T)
    if edge_index.size and (edge_index.min() < 0 or edge_index.max() >= n):
        raise SplitFormatError(f"{path}: node ids must be 0..{n - 1}")
    return n, labels, edge_index


def read_mis_split(pattern: str, label_dir: Optional[str] = None, limit: Optional[int] = None) -> List[MISExample]:
    """Every graph matched by ``pattern`` (the first ``limit`` when given), in ``glob.glob`` order (see the module
    docstring).  Labels come from the ``label`` node attribute (zeros when it is absent) or, with ``label_dir``, from
    ``<name>_unweighted.result``."""
    out = []
    for path in glob.glob(pattern)[:limit]:
        n, labels, edge_index = mis_example(load_gpickle(path), path, label_dir)
        out.append(MISExample(n, labels, edge_index, (path, 0)))
    return out
