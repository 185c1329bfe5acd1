"""The 2-D picture of an embedding: exact t-SNE of rows of the engine's table, on the GPU.

Nothing in the reference does this: its users hand ``Z.npy`` to scikit-learn.  Here the hot path is HIP (csrc/tsne.h): the
all-pairs squared distances on the matrix cores, the perplexity search, the joint probabilities, and per iteration one
pass over ``P [n, n]`` for the force sums and one small update kernel.  The formulas are scikit-learn's
``TSNE(method="exact")`` -- ``_binary_search_perplexity``, ``_joint_probabilities``, ``_kl_divergence``,
``_gradient_descent`` -- so a layout minimises the exact objective; every sum runs in an order that depends on ``n``
alone, so a fit is reproducible bit for bit.

What stays torch plumbing: the initial layout (``ContentPCA`` to two components), the column mean the distances are
centred with (the existing column-sum kernel), the host's look at KL and gradient norm every 50 iterations, and
``neighbour_agreement``.

Past 65 536 points ``P [n, n]`` does not fit: ``NeighbourTSNE`` (csrc/tsne_nn.h) keeps ``P`` on every point's
``k = 3 * perplexity`` nearest neighbours -- scikit-learn's ``_joint_probabilities_nn`` -- found by a fused distance +
selection kernel on the matrix cores (``KNeighbours``), and keeps the repulsion EXACT: all pairs of ``Y`` through LDS, no
tree.  The sparsity of ``P`` is its only approximation.  The union of the neighbour pairs is sorted into CSR by torch.

There is no CPU fallback: without the library or a GPU, ``fit`` raises ``ClaneHipError``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch

from . import _hip

CHECK_EVERY = 50                    # scikit-learn's n_iter_check: the host reads KL and |g| this often
MIN_POINTS = 4
MAX_POINTS = _hip.TSNE_MAX_POINTS   # P [n, n] fp32 would pass 16 GiB
INIT_STD = 1e-4                     # scikit-learn's init="pca": the first column's standard deviation
SECTION_KEYS = ("perplexity", "max_points", "max_iter", "seed", "labels", "baseline")
SECTION_DEFAULTS = {"perplexity": 30.0, "max_points": 20000, "max_iter": 1000, "seed": 0, "labels": None,
                    "baseline": False}
METHODS = ("exact", "neighbours")
NEIGHBOUR_KEYS = ("method", "neighbours")       # in check_section's result only when the section gives them
NN_MAX_POINTS = _hip.TSNE_NN_MAX_POINTS          # method "neighbours": nothing is n x n
MAX_NEIGHBOURS = _hip.KNN_MAX_K


# ---- the config section -------------------------------------------------------------------------------------------------
def check_section(section, world_size: int = 1) -> dict:
    """The validated ``layout`` section of a config, every key filled in.  Before any graph is read."""
    if world_size > 1:
        raise NotImplementedError("layout: the 2-D layout runs on ONE GPU only (WORLD_SIZE > 1): several GPUs are out of "
                                  "scope")
    if section is None:
        section = {}                                 # `layout:` with nothing under it: every default
    if not isinstance(section, dict):
        raise ValueError(f"layout: expected a mapping of {list(SECTION_KEYS)}, got {section!r}")
    unknown = sorted(set(section) - set(SECTION_KEYS) - set(NEIGHBOUR_KEYS))
    if unknown:
        raise ValueError(f"layout: unknown keys {unknown}; known: {list(SECTION_KEYS + NEIGHBOUR_KEYS)}")
    out = {**SECTION_DEFAULTS, **section}
    method = out.get("method", "exact")
    if method not in METHODS:
        raise ValueError(f"layout: method must be one of {list(METHODS)}, got {method!r}")
    if "neighbours" in out and method != "neighbours":
        raise ValueError(f"layout: neighbours = {out['neighbours']!r} needs method: neighbours (method {method!r} keeps "
                         f"all of P)")
    cap = NN_MAX_POINTS if method == "neighbours" else MAX_POINTS
    p = out["perplexity"]
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not math.isfinite(p) or p <= 0:
        raise ValueError(f"layout: perplexity must be a positive number, got {p!r}")
    out["perplexity"] = float(p)
    for key, least in (("max_points", MIN_POINTS), ("max_iter", 1), ("seed", 0)):
        v = out[key]
        if isinstance(v, bool) or not isinstance(v, int) or v < least:
            raise ValueError(f"layout: {key} must be an integer >= {least}, got {v!r}")
    if out["max_points"] > cap:
        raise ValueError(f"layout: max_points = {out['max_points']} exceeds {cap} " + (
            "(method: neighbours)" if method == "neighbours" else "(P would pass 16 GiB)"))
    if out["perplexity"] >= out["max_points"]:
        raise ValueError(f"layout: perplexity = {out['perplexity']:g} must be below max_points = {out['max_points']}")
    if method == "neighbours":
        check_neighbours(out.get("neighbours"), out["perplexity"], "layout")
    if out["labels"] is not None and (not isinstance(out["labels"], str) or not out["labels"]):
        raise ValueError(f"layout: labels must be the path of a file of id<TAB>class lines, got {out['labels']!r}")
    if not isinstance(out["baseline"], bool):
        raise ValueError(f"layout: baseline must be true or false, got {out['baseline']!r}")
    return out


def check_neighbours(neighbours, perplexity: float, who: str, n: Optional[int] = None) -> Optional[int]:
    """The neighbours per point of the method "neighbours": the given count, or (None) scikit-learn's
    ``floor(3 * perplexity)``, at most ``n - 1`` once ``n`` is known (None: returned as None).  Arithmetic only."""
    most = MAX_NEIGHBOURS if n is None else min(MAX_NEIGHBOURS, n - 1)
    if neighbours is None:
        if int(3.0 * perplexity) > MAX_NEIGHBOURS:
            raise ValueError(f"{who}: perplexity = {perplexity:g} asks for {int(3.0 * perplexity)} neighbours per point, "
                             f"more than {MAX_NEIGHBOURS}: perplexity up to {MAX_NEIGHBOURS // 3} (or give neighbours)")
        if n is None:
            return None
        k = min(n - 1, int(3.0 * perplexity))
        if not perplexity < k:
            raise ValueError(f"{who}: perplexity = {perplexity:g} must be below the {k} neighbours of n = {n} points")
        return k
    if isinstance(neighbours, bool) or not isinstance(neighbours, int):
        raise ValueError(f"{who}: neighbours must be an integer, got {neighbours!r}")
    if not perplexity < neighbours <= most:
        raise ValueError(f"{who}: neighbours = {neighbours} must be above perplexity = {perplexity:g} and at most {most}"
                         + ("" if n is None or most == MAX_NEIGHBOURS else f" (n - 1 of n = {n} points)"))
    return neighbours


def resolve_labels(section: dict, data_root) -> Optional[Path]:
    """The file of the section's ``labels`` (relative to ``data_root``), which must exist; None without the key."""
    if section.get("labels") is None:
        return None
    path = Path(section["labels"])
    if not path.is_absolute():
        path = Path(data_root) / path
    if not path.is_file():
        raise ValueError(f"layout: labels: {str(path)!r} is missing")
    return path


def sample_vertices(n_vertices: int, max_points: int, seed: int = 0):
    """``(vertex indices, sampled)``: all of them, or -- with more than ``max_points`` -- the first ``max_points`` of a
    torch permutation seeded with ``seed``, sorted."""
    if n_vertices <= max_points:
        return torch.arange(n_vertices), False
    perm = torch.randperm(n_vertices, generator=torch.Generator().manual_seed(int(seed)))
    return torch.sort(perm[:max_points]).values, True


def neighbour_agreement(Y, labels, k: int = 5) -> float:
    """The share of the ``k`` nearest 2-D neighbours (Euclidean, the point itself excluded) that carry the point's own
    class, averaged over the points.  Torch plumbing, on ``Y``'s device, 4096 rows of distances at a time."""
    Y = torch.as_tensor(Y).to(torch.float64)
    y = torch.as_tensor(labels, device=Y.device).reshape(-1)
    n = int(Y.shape[0])
    if Y.dim() != 2 or y.numel() != n:
        raise ValueError(f"neighbour_agreement: Y must be [n, dims] with one label per point, got {tuple(Y.shape)} and "
                         f"{y.numel()} labels")
    if not 1 <= k < n:
        raise ValueError(f"neighbour_agreement: k must be in [1, n - 1 = {n - 1}], got {k}")
    same = 0
    for a in range(0, n, 4096):
        d = torch.cdist(Y[a:a + 4096], Y)
        d[torch.arange(d.shape[0]), torch.arange(a, a + d.shape[0])] = math.inf
        idx = d.topk(k, dim=1, largest=False).indices
        same += int((y[idx] == y[a:a + 4096, None]).sum())
    return same / (n * k)


REPORT_KEYS = ("n", "sampled", "perplexity", "iterations", "kl", "kl_init", "grad_norm", "kl_trace")
NN_REPORT_KEYS = ("method", "neighbours", "nnz")


def write_results(output_root, vertex_ids, tables: dict) -> dict:
    """What the CLI writes from ``Graph.layout``'s returns, ``tables = {"Z": (Y, vertices, info)[, "X": ...]}``:
    ``layout.tsv`` (``layout_X.tsv`` for the baseline) with one ``id<TAB>x<TAB>y[<TAB>class]`` line per laid-out vertex in
    the order of ``vertices``, and ``layout.json``: REPORT_KEYS of "Z" (with labels also ``neighbour_agreement``), the
    same of "X" under ``"baseline"``.  Returns the report."""
    import json
    output_root = Path(output_root)
    report = {}
    for name, (Y, vertices, info) in tables.items():
        classes = info.get("classes")
        with open(output_root / ("layout.tsv" if name == "Z" else f"layout_{name}.tsv"), "w") as io:
            for i, v in enumerate(vertices.tolist()):
                tail = "" if classes is None else f"\t{'' if classes[i] is None else classes[i]}"
                io.write(f"{vertex_ids[v]}\t{float(Y[i, 0])!r}\t{float(Y[i, 1])!r}{tail}\n")
        entry = {key: info[key] for key in REPORT_KEYS}
        entry.update({key: info[key] for key in NN_REPORT_KEYS if key in info})      # method "neighbours" only
        if "neighbour_agreement" in info:
            entry["neighbour_agreement"] = info["neighbour_agreement"]
        if name == "Z":
            report.update(entry)
        else:
            report["baseline"] = entry
    with open(output_root / "layout.json", "w") as io:
        json.dump(report, io, indent=1)
        io.write("\n")
    return report


# ---- the fit --------------------------------------------------------------------------------------------------------------
def column_mean(k, d: int, Z, rows) -> torch.Tensor:
    """The column mean of the listed rows (a row outside the table counts as zeros), float32 on the device: the
    fixed-order column sums in double, divided by n, rounded once."""
    n = int(rows.numel())
    sums = torch.empty(d, dtype=torch.float64, device=Z.device)
    ws = torch.empty(k.column_sums_ws_len(n, d), dtype=torch.float64, device=Z.device)
    k.column_sums(Z, d, rows, ws, sums)
    return (sums / n).to(torch.float32)


@dataclass
class TSNEFit:
    Y: torch.Tensor             # [n, 2] float32, on the device
    kl: float                   # KL(P || Q) of the layout the last iteration started from (scikit-learn's kl_divergence_)
    iterations: int
    grad_norm: float            # |g| of the last iteration
    beta: torch.Tensor          # [n] float32, on the device: the precision of every point's conditional distribution
    kl_init: float              # KL of the initial layout
    kl_trace: List[float] = field(default_factory=list)     # one value per CHECK_EVERY iterations


class TSNE:
    """Exact t-SNE to two dimensions of rows of a table of ``engine``: scikit-learn's ``TSNE(method="exact")`` with its
    defaults -- ``exaggeration_iters`` iterations at ``early_exaggeration`` and momentum 0.5, the rest at 1 and 0.8 (gains
    and velocity start afresh there, as in scikit-learn's two ``_gradient_descent`` calls); every 50 iterations the host
    reads KL and the gradient norm and stops on ``min_grad_norm`` or ``n_iter_without_progress``."""

    def __init__(self, engine, perplexity: float = 30.0, early_exaggeration: float = 12.0, exaggeration_iters: int = 250,
                 max_iter: int = 1000, learning_rate="auto", min_grad_norm: float = 1e-7,
                 n_iter_without_progress: int = 300):
        from .train import require_one_gpu
        try:
            require_one_gpu(engine)
        except NotImplementedError:
            raise NotImplementedError(
                f"t-SNE runs on ONE GPU only: a fit reads arbitrary rows of the table, which this engine "
                f"divides over {engine.world} ranks (exchange={engine.exchange!r}); several GPUs are out of scope") from None
        if not (isinstance(perplexity, (int, float)) and math.isfinite(perplexity) and perplexity > 0):
            raise ValueError(f"TSNE: perplexity must be a positive number, got {perplexity!r}")
        if not early_exaggeration >= 1.0:
            raise ValueError(f"TSNE: early_exaggeration must be at least 1, got {early_exaggeration!r}")
        if int(max_iter) < 1 or int(exaggeration_iters) < 0:
            raise ValueError("TSNE: max_iter >= 1 and exaggeration_iters >= 0")
        if learning_rate != "auto" and not float(learning_rate) > 0:
            raise ValueError(f"TSNE: learning_rate must be 'auto' or a positive number, got {learning_rate!r}")
        self.eng, self.k = engine, engine.k
        self.perplexity, self.early_exaggeration = float(perplexity), float(early_exaggeration)
        self.exaggeration_iters, self.max_iter = int(exaggeration_iters), int(max_iter)
        self.learning_rate = learning_rate
        self.min_grad_norm, self.n_iter_without_progress = float(min_grad_norm), int(n_iter_without_progress)

    def table_and_rows(self, vertices, table: str = "Z"):
        """(table, int32 rows) for vertex indices: the current embeddings ("Z") or the content embeddings ("X")."""
        from .classify import table_and_rows
        return table_and_rows(self.eng, vertices, table)

    # ---- checks: arithmetic, before any allocation ----------------------------------------------------------------------
    def check_points(self, n: int) -> None:
        if n < MIN_POINTS:
            raise ValueError(f"TSNE: a layout needs at least {MIN_POINTS} points, got n = {n}")
        if n > MAX_POINTS:
            raise ValueError(f"TSNE: n = {n} exceeds {MAX_POINTS} points: P [n, n] would pass 16 GiB; lay out a sample "
                             f"(Graph.layout(max_points=...))")
        if self.perplexity >= n:
            raise ValueError(f"TSNE: perplexity = {self.perplexity:g} must be below n = {n}")

    @staticmethod
    def workspace_bytes(n: int) -> int:
        """P and everything else a fit keeps on the device, in bytes."""
        tiles = -(-n // 64)
        return 4 * n * n + 4 * n * (6 + 4 * 2 + 2) + 8 * (tiles * (tiles + 1) // 2 + 8)

    def _check_memory(self, n: int, dev) -> None:
        free, _ = torch.cuda.mem_get_info(dev)
        free += torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)     # torch re-uses what it caches
        if self.workspace_bytes(n) > free:
            fits = int(math.isqrt(max(0, free - (64 << 20)) // 4))
            raise _hip.ClaneHipError(f"TSNE: P [n, n] and the workspace of n = {n} points need "
                                     f"{self.workspace_bytes(n)} bytes, the GPU has {free} free: about {fits} points "
                                     f"would fit (Graph.layout(max_points=...))")

    def learning_rate_for(self, n: int) -> float:
        if self.learning_rate == "auto":
            return max(n / self.early_exaggeration / 4.0, 50.0)
        return float(self.learning_rate)

    # ---- pieces ---------------------------------------------------------------------------------------------------------
    def column_mean(self, Z, rows) -> torch.Tensor:
        """The column mean of the listed rows (a row outside the table counts as zeros), float32 on the device: the
        fixed-order column sums in double, divided by n, rounded once."""
        return column_mean(self.k, int(self.eng.d), Z, rows)

    def joint_probabilities(self, Z, rows):
        """``(P [n, n], beta [n], sum p ln p)``: distances, the perplexity search and the symmetrisation, in place in one
        ``[n, n]`` matrix."""
        n, dev = int(rows.numel()), Z.device
        P = torch.empty(n, n, dtype=torch.float32, device=dev)
        sq = torch.empty(n, dtype=torch.float32, device=dev)
        beta = torch.empty(n, dtype=torch.float32, device=dev)
        self.k.tsne_sqdist(Z, int(self.eng.d), rows, self.column_mean(Z, rows), sq, P)
        self.k.tsne_affinities(P, self.perplexity, beta)
        partials = torch.empty(self.k.tsne_symmetrize_ws_len(n), dtype=torch.float64, device=dev)
        self.k.tsne_symmetrize(P, partials)
        plogp = float(np.cumsum(partials.cpu().numpy())[-1])       # the tile pairs in order, in float64
        return P, beta, plogp

    def pca_init(self, Z, rows) -> torch.Tensor:
        """scikit-learn's ``init="pca"``: the first two principal components of the listed rows, scaled so that the first
        column's standard deviation is 1e-4."""
        from .reduce import ContentPCA
        n, d, dev = int(rows.numel()), int(self.eng.d), Z.device
        pca = ContentPCA(2)
        pca._check_fit_shape(n, d)
        step = pca._rows_per_block(d, Z.dtype)
        pca._fit_blocks(pca._table_blocks(Z, rows, step), n, d, Z.dtype, dev, step)
        out = torch.empty(n, 2, dtype=Z.dtype, device=dev)
        pca._transform_blocks(pca._table_blocks(Z, rows, step), n, d, Z.dtype, dev, out)
        Y = out.to(torch.float32)
        std = float(Y[:, 0].double().std(unbiased=False))
        if not std > 0:
            raise ValueError("TSNE: the listed rows have no variance: there is nothing to lay out")
        return (Y.double() / std * INIT_STD).to(torch.float32).contiguous()

    # ---- fit ------------------------------------------------------------------------------------------------------------
    def fit(self, Z: torch.Tensor, rows: torch.Tensor, init: Optional[torch.Tensor] = None, seed: int = 0) -> TSNEFit:
        """Lay out the rows ``rows`` (int32 table rows) of ``Z``.  ``init``: a ``[n, 2]`` tensor used as it is; None: the
        PCA initialisation, which is deterministic -- ``seed`` is accepted for the day an initialisation draws numbers
        and changes nothing today."""
        n = int(rows.numel())
        self.check_points(n)
        if init is not None and tuple(init.shape) != (n, 2):
            raise ValueError(f"TSNE: init must be [{n}, 2], got {tuple(init.shape)}")
        dev = Z.device
        k = self.k
        with torch.cuda.device(dev):
            self._check_memory(n, dev)
            Y = self.pca_init(Z, rows) if init is None else init.to(dev, torch.float32).contiguous().clone()
            P, beta, plogp = self.joint_probabilities(Z, rows)
            return self._descend(Y, beta, plogp, lambda Y, F, kl: k.tsne_forces(P, Y, F, kl=kl))

    def _descend(self, Y, beta, plogp: float, forces, **more) -> TSNEFit:
        """The two-phase gradient descent from ``Y``, under the caller's ``torch.cuda.device``; ``forces(Y, F, kl)`` fills
        the force sums ``F [n, 6]`` of a layout.  ``more``: the further fields of a ``NeighbourTSNEFit``."""
        n, dev, k = int(Y.shape[0]), Y.device, self.k
        Y_next = torch.empty_like(Y)
        V, G = torch.empty_like(Y), torch.empty_like(Y)
        F = torch.empty(n, 6, dtype=torch.float32, device=dev)
        stats = torch.zeros(4, dtype=torch.float64, device=dev)
        stats_init = None
        lr = self.learning_rate_for(n)
        switch = min(self.exaggeration_iters, self.max_iter)
        phases = ((switch, self.early_exaggeration, 0.5, max(self.exaggeration_iters, 1)),
                  (self.max_iter, 1.0, 0.8, self.n_iter_without_progress))
        it, trace, stopped = 0, [], False
        for end, alpha, momentum, patience in phases:
            if it >= end or stopped:
                continue
            V.zero_()
            G.fill_(1.0)
            best, best_it = math.inf, it
            while it < end:
                check = (it + 1) % CHECK_EVERY == 0
                forces(Y, F, check or it == end - 1 or it == 0)
                k.tsne_step(F, Y, alpha, momentum, lr, plogp, V, G, Y_next, stats)
                Y, Y_next = Y_next, Y
                if it == 0:
                    stats_init = stats.clone()
                it += 1
                if check:                                  # the one look of the host per CHECK_EVERY iterations
                    kl, gnorm = stats[:2].tolist()
                    trace.append(kl)
                    if kl < best:
                        best, best_it = kl, it - 1
                    elif it - 1 - best_it > patience:
                        stopped = end == self.max_iter
                        break
                    if gnorm <= self.min_grad_norm:
                        stopped = end == self.max_iter
                        break
        kl, gnorm = stats[:2].tolist()
        return (NeighbourTSNEFit if more else TSNEFit)(Y=Y, kl=kl, iterations=it, grad_norm=gnorm, beta=beta,
                                                       kl_init=float(stats_init[0]), kl_trace=trace, **more)


# ---- past the dense cap: P on the nearest neighbours, the repulsion exact ---------------------------------------------------
@dataclass
class NeighbourTSNEFit(TSNEFit):
    neighbours: int = 0         # k: the neighbours per point P was built on
    nnz: int = 0                # stored entries of the joint P (both directions of every pair)


@dataclass
class SparseJoint:
    """The joint probabilities on the union of the neighbour pairs, CSR on the device: no diagonal, no floor, columns
    ascending in each row, ``P[i, j]`` and ``P[j, i]`` the same bits."""
    rowptr: torch.Tensor        # [n + 1] int64
    cols: torch.Tensor          # [nnz] int32
    val: torch.Tensor           # [nnz] float32

    @property
    def n(self) -> int:
        return int(self.rowptr.numel()) - 1

    @property
    def nnz(self) -> int:
        return int(self.val.numel())


KNN_BLOCKS = 1024               # workgroups a search aims at: four per compute unit


def knn_query_tile(k: int) -> int:
    """Queries whose lists a workgroup of knn_sqdist keeps in LDS (csrc/tsne_nn.h, knn_tile_mi)."""
    return 128 if k <= 40 else 64 if k <= 96 else 32


def knn_slabs(n: int, k: int) -> int:
    """Slabs of candidate tiles a search of ``n`` rows is cut into when nobody says: enough for KNN_BLOCKS workgroups,
    at most one per tile of 128 candidates.  The result of a search does not depend on it."""
    q_tiles, tiles = -(-n // knn_query_tile(k)), -(-n // 128)
    return max(1, min(tiles, -(-KNN_BLOCKS // q_tiles)))


class KNeighbours:
    """The ``k`` nearest listed rows of every listed row of a table of ``engine`` by squared Euclidean distance
    (csrc/tsne_nn.h, knn_sqdist): the distances of exact t-SNE -- centred by the listed rows' column mean, a row outside
    the table counts as zeros -- with the selection fused in, so the ``n x n`` distances never exist."""

    def __init__(self, engine):
        from .train import require_one_gpu
        try:
            require_one_gpu(engine)
        except NotImplementedError:
            raise NotImplementedError(
                f"the neighbour search runs on ONE GPU only: it reads arbitrary rows of the table, which this engine "
                f"divides over {engine.world} ranks (exchange={engine.exchange!r}); several GPUs are out of scope") from None
        self.eng, self.k = engine, engine.k

    @staticmethod
    def check(n: int, k: int) -> None:
        if isinstance(k, bool) or int(k) != k or not 1 <= k <= MAX_NEIGHBOURS:
            raise ValueError(f"KNeighbours: k must be an integer in [1, {MAX_NEIGHBOURS}], got {k!r}")
        if not 2 <= n <= NN_MAX_POINTS:
            raise ValueError(f"KNeighbours: a search needs 2 to {NN_MAX_POINTS} rows, got n = {n}")

    def search(self, Z, rows, k: int, n_slabs: Optional[int] = None):
        """``(ids [n, k] int32, sqdist [n, k] float32)`` on the device: for every row of ``rows`` (int32 table rows) the
        positions in ``rows`` of its ``k`` nearest other rows, distance ascending, ties by position; ``-1`` and ``inf``
        past the ``n - 1`` other rows.  ``n_slabs``: how the candidates are cut (None: ``knn_slabs``); never the result."""
        n = int(rows.numel())
        self.check(n, k)
        k = int(k)
        n_slabs = knn_slabs(n, k) if n_slabs is None else int(n_slabs)
        if n_slabs < 1:
            raise ValueError(f"KNeighbours: n_slabs must be at least 1, got {n_slabs}")
        dev, f32 = Z.device, torch.float32
        with torch.cuda.device(dev):
            ids = torch.empty(n, k, dtype=torch.int32, device=dev)
            sqdist = torch.empty(n, k, dtype=f32, device=dev)
            cand_i = cand_d = None
            if n_slabs > 1:
                cand_i = torch.empty(n * n_slabs * k, dtype=torch.int32, device=dev)
                cand_d = torch.empty(n * n_slabs * k, dtype=f32, device=dev)
            self.k.knn_sqdist(Z, int(self.eng.d), rows, column_mean(self.k, int(self.eng.d), Z, rows),
                              torch.empty(n, dtype=f32, device=dev), ids, sqdist, n_slabs, cand_i, cand_d)
        return ids, sqdist


def sparse_joint(ids, p) -> SparseJoint:
    """``p_ij = (c_ij + c_ji) / 2n`` over the union of the neighbour pairs, from the conditionals ``p [n, k]`` of the
    neighbours ``ids [n, k]`` (-1: none); an absent conditional counts as 0.  Torch plumbing, sort-based: every
    conditional is filed under its own pair and under the mirrored one, the (at most two) entries of a pair are added by
    ONE fp32 add -- which commutes, so both directions get the same bits -- and divided; nothing is accumulated."""
    n, k = int(ids.shape[0]), int(ids.shape[1])
    dev = ids.device
    i = torch.arange(n, dtype=torch.int64, device=dev).repeat_interleave(k)
    j = ids.reshape(-1).to(torch.int64)
    keep = j >= 0
    i, j, c = i[keep], j[keep], p.reshape(-1)[keep]
    key = torch.cat(((i * n + j) * 2, (j * n + i) * 2 + 1))        # pair << 1 | mirrored: unique
    del i, j, keep
    key, order = torch.sort(key)
    c = torch.cat((c, c))[order]
    del order
    pair = key >> 1
    del key
    first = torch.ones(pair.numel(), dtype=torch.bool, device=dev)
    first[1:] = pair[1:] != pair[:-1]
    start = first.nonzero().reshape(-1)
    del first
    pair = pair[start]
    two = torch.zeros(start.numel(), dtype=torch.bool, device=dev)
    two[:-1] = start[1:] - start[:-1] == 2
    two[-1:] = c.numel() - start[-1:] == 2
    b = torch.where(two, c[(start + 1).clamp_(max=c.numel() - 1)], torch.zeros((), dtype=c.dtype, device=dev))
    val = (c[start] + b) / torch.full((), 2 * n, dtype=torch.float32, device=dev)      # a tensor: a true division
    r = torch.div(pair, n, rounding_mode="floor")
    cols = (pair - r * n).to(torch.int32)
    rowptr = torch.searchsorted(r, torch.arange(n + 1, dtype=torch.int64, device=dev))
    return SparseJoint(rowptr=rowptr.contiguous(), cols=cols.contiguous(), val=val.contiguous())


class NeighbourTSNE(TSNE):
    """t-SNE to two dimensions with ``P`` kept on every point's ``neighbours`` nearest neighbours (None: scikit-learn's
    ``floor(3 * perplexity)``, at most ``n - 1``) and the repulsion exact -- up to 2^20 points.  The descent, its checks
    and its record are ``TSNE``'s; the objective is scikit-learn's ``barnes_hut`` one (``_joint_probabilities_nn``: no
    floor under ``P``) without the tree."""

    def __init__(self, engine, *args, neighbours: Optional[int] = None, **kwargs):
        super().__init__(engine, *args, **kwargs)
        check_neighbours(neighbours, self.perplexity, "NeighbourTSNE")
        self.neighbours = neighbours

    def neighbours_for(self, n: int) -> int:
        return check_neighbours(self.neighbours, self.perplexity, "NeighbourTSNE", n)

    # ---- checks: arithmetic, before any allocation ----------------------------------------------------------------------
    def check_points(self, n: int) -> None:
        if n < MIN_POINTS:
            raise ValueError(f"NeighbourTSNE: a layout needs at least {MIN_POINTS} points, got n = {n}")
        if n > NN_MAX_POINTS:
            raise ValueError(f"NeighbourTSNE: n = {n} exceeds {NN_MAX_POINTS} points; lay out a sample "
                             f"(Graph.layout(max_points=...))")
        if self.perplexity >= n:
            raise ValueError(f"NeighbourTSNE: perplexity = {self.perplexity:g} must be below n = {n}")
        self.neighbours_for(n)

    def workspace_bytes(self, n: int, k: Optional[int] = None) -> int:
        """What a fit keeps on the device at its peak, in bytes: the lists of the search (ids, distances, conditionals,
        per slab the candidates), the sort that builds the joint P (keys, order, values and their sorted copies, the CSR:
        128 bytes per directed neighbour at most) and the arrays of the descent."""
        k = self.neighbours_for(n) if k is None else k
        slabs = knn_slabs(n, k)
        return n * k * (12 + 128 + (8 * slabs if slabs > 1 else 0)) + 4 * n * (6 + 4 * 2 + 2 + 1) + 8 * (n + 1 + 8)

    def _check_memory(self, n: int, dev) -> None:
        free, _ = torch.cuda.mem_get_info(dev)
        free += torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)     # torch re-uses what it caches
        if self.workspace_bytes(n) > free:
            k = self.neighbours_for(n)
            fits = max(0, free - (64 << 20)) // (self.workspace_bytes(n, k) // n + 1)
            raise _hip.ClaneHipError(f"NeighbourTSNE: the {k} neighbours and the workspace of n = {n} points need "
                                     f"{self.workspace_bytes(n)} bytes, the GPU has {free} free: about {fits} points "
                                     f"would fit (Graph.layout(max_points=...))")

    # ---- pieces ---------------------------------------------------------------------------------------------------------
    def joint_probabilities(self, Z, rows):
        """``(P: SparseJoint, beta [n], sum p ln p)``: the neighbour search, the perplexity search over each row's
        neighbours and the symmetrisation over the union of the pairs."""
        n, dev = int(rows.numel()), Z.device
        kk = self.neighbours_for(n)
        ids, sqdist = KNeighbours(self.eng).search(Z, rows, kk)
        beta = torch.empty(n, dtype=torch.float32, device=dev)
        p = torch.empty_like(sqdist)
        self.k.tsne_nn_affinities(sqdist, ids, self.perplexity, p, beta)
        del sqdist
        P = sparse_joint(ids, p)
        del ids, p
        row_plogp = torch.empty(n, dtype=torch.float64, device=dev)
        self.k.tsne_nn_plogp(P.rowptr, P.val, row_plogp)
        plogp = float(np.cumsum(row_plogp.cpu().numpy())[-1])      # the rows in order, in float64
        return P, beta, plogp

    # ---- fit ------------------------------------------------------------------------------------------------------------
    def fit(self, Z: torch.Tensor, rows: torch.Tensor, init: Optional[torch.Tensor] = None,
            seed: int = 0) -> NeighbourTSNEFit:
        """As ``TSNE.fit``; the record also says ``neighbours`` and ``nnz``."""
        n = int(rows.numel())
        self.check_points(n)
        if init is not None and tuple(init.shape) != (n, 2):
            raise ValueError(f"NeighbourTSNE: init must be [{n}, 2], got {tuple(init.shape)}")
        dev = Z.device
        k = self.k
        with torch.cuda.device(dev):
            self._check_memory(n, dev)
            Y = self.pca_init(Z, rows) if init is None else init.to(dev, torch.float32).contiguous().clone()
            P, beta, plogp = self.joint_probabilities(Z, rows)

            def forces(Y, F, kl):
                k.tsne_nn_attract(P.rowptr, P.cols, P.val, Y, F, kl=kl)
                k.tsne_repulse(Y, F)
            return self._descend(Y, beta, plogp, forces, neighbours=self.neighbours_for(n), nnz=P.nnz)
