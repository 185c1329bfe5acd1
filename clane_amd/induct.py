"""Embedding NEW vertices against a finished graph (``NewVertexEmbedder`` / ``Graph.embed_new`` / the config's
``new_vertices`` section).  No reference counterpart as a function, but it is the reference's own loop: a vertex ``u`` that
was not in ``V`` has content ``x_u`` and out-edges to EXISTING vertices only, and nothing reads ``u``.  ``Graph.build_P``
(graph.py:118-128) followed by the update (embedder.py:84-92), restricted to row ``u`` with the table held fixed, is the
per-row fixed point

    z  <-  x_u + gamma * sum_v softmax_v(score(z, z_v)) z_v ,    v in nbrs(u),   z^0 = x_u

iterated with the reference's ``Tolerence`` per row (csrc/new_rows.h: one launch, every row stops on its own).  The
existing rows do not move, so a classifier, clustering or ranker fitted on the old ``Z`` stays valid, and the result can
be handed to ``LabelProbe`` weights, ``KMeans`` centres or ``LinkRanker`` as any other row.

FROZEN: in reference cosine mode the global Frobenius denominators (similarity.py:37) are those of the EXISTING graph --
the new edges are not counted in.  If the existing rows are at their fixed point and nobody links to ``u``,
``Embedder.iterate()`` on the augmented graph converges to the same ``z_u`` in ``per_edge`` mode and for the bilinear
score; in reference mode up to the change of the global denominator.

Neighbours are vertex indices in ``[0, V)`` (mapped through ``eng.pos`` to table rows); anything else is a ValueError, so
edges between new vertices are impossible by construction.  A repeated neighbour counts once: the reference coalesces
duplicate edges.  One GPU only.
"""
from __future__ import annotations

import json
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from .train import require_one_gpu

SUPPORTED = "CosineSimilarity and AsymmertricSimilarity"
SECTION_KEYS = ("root", "max_rounds", "weights")


def _round_up(n: int, m: int) -> int:
    return -(-n // m) * m


@dataclass
class NewRows:
    """What ``NewVertexEmbedder.embed`` returns; tensors on the engine's device (``Graph.embed_new``: on the host)."""
    Z: torch.Tensor                     # [m, d], the table dtype
    rounds: torch.Tensor                # int32 [m]: rounds run, 0 for a vertex without neighbours (it keeps x)
    delta: torch.Tensor                 # [m], accumulate dtype: the last round's sum |z_new - z|
    converged: torch.Tensor             # bool [m]: rounds < max_rounds
    rowptr: torch.Tensor                # int64 [m + 1]: the coalesced neighbour lists P refers to
    cols: torch.Tensor                  # int64: their vertex indices, ascending within a row
    P: Optional[torch.Tensor] = None    # soft-max weights that produced Z, in (rowptr, cols) order

    def cpu(self) -> "NewRows":
        return NewRows(*[None if t is None else t.cpu() for t in
                         (self.Z, self.rounds, self.delta, self.converged, self.rowptr, self.cols, self.P)])


def normalize_neighbours(neighbours, m: int) -> Tuple[np.ndarray, np.ndarray]:
    """(rowptr int64 [m + 1], cols int64) of the new vertices' neighbour lists.  ``neighbours`` is a ``tuple`` of two
    arrays / tensors ``(rowptr, colidx)``, or a sequence of ``m`` collections of vertex indices (anything else than such
    a tuple is read as the latter).  Ranges of the indices are checked by ``NewVertexEmbedder.embed``, which knows V."""
    if isinstance(neighbours, tuple) and len(neighbours) == 2 and all(
            isinstance(a, (np.ndarray, torch.Tensor)) for a in neighbours):
        rowptr = np.asarray(torch.as_tensor(neighbours[0]).cpu().numpy())
        cols = np.asarray(torch.as_tensor(neighbours[1]).cpu().numpy())
        if rowptr.ndim != 1 or cols.ndim != 1 or rowptr.dtype.kind not in "iu" or (cols.size and cols.dtype.kind not in "iu"):
            raise ValueError("neighbours: (rowptr, colidx) must be two 1-D integer arrays")
        if rowptr.size != m + 1:
            raise ValueError(f"neighbours: rowptr needs m + 1 = {m + 1} entries, got {rowptr.size}")
        rowptr = rowptr.astype(np.int64)
        if rowptr[0] != 0 or (np.diff(rowptr) < 0).any() or rowptr[-1] != cols.size:
            raise ValueError("neighbours: rowptr must start at 0, never decrease and end at len(colidx)")
        return rowptr, cols.astype(np.int64)
    try:
        lists = list(neighbours)
    except TypeError:
        raise ValueError("neighbours: a sequence of per-vertex index collections or a (rowptr, colidx) tuple") from None
    if len(lists) != m:
        raise ValueError(f"neighbours: one collection per new vertex: expected {m}, got {len(lists)}")
    rowptr = np.zeros(m + 1, dtype=np.int64)
    parts = []
    for i, nb in enumerate(lists):
        a = np.asarray(torch.as_tensor(nb).cpu().numpy() if isinstance(nb, torch.Tensor) else list(nb))
        if a.size and a.dtype.kind not in "iu":
            raise ValueError(f"neighbours[{i}]: vertex indices must be integers")
        if a.ndim > 1:
            raise ValueError(f"neighbours[{i}]: a flat collection of vertex indices")
        parts.append(a.astype(np.int64).reshape(-1))
        rowptr[i + 1] = rowptr[i] + parts[-1].size
    cols = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return rowptr, cols.astype(np.int64)


class NewVertexEmbedder:
    def __init__(self, engine, similarity):
        from .similarity import AsymmertricSimilarity, CosineSimilarity
        try:
            require_one_gpu(engine)
        except NotImplementedError:
            raise NotImplementedError(
                f"embedding new vertices runs on ONE GPU only: a new row reads arbitrary rows of Z, which this engine "
                f"divides over {engine.world} ranks (exchange={engine.exchange!r}); several GPUs and column divisions are "
                f"out of scope") from None
        if isinstance(similarity, AsymmertricSimilarity):
            self.bilinear = True
            n_dim = similarity.Phi_src.in_features
            if n_dim != engine.d_full or similarity.Phi_dst.in_features != engine.d_full:
                raise ValueError(f"AsymmertricSimilarity(n_dim={n_dim}) does not fit embeddings of dimension "
                                 f"{engine.d_full}")
        elif isinstance(similarity, CosineSimilarity):
            self.bilinear = False
        else:
            raise NotImplementedError(
                f"new vertices are embedded with {SUPPORTED}; a plug-in similarity ({type(similarity).__name__}) has no "
                f"kernel to iterate a row with")
        self.eng, self.k, self.sim = engine, engine.k, similarity
        self._Y = None              # the M-projection of the table; NOT eng._Y: a prepared LinkRanker stays valid
        self._ready = False

    def prepare(self) -> None:
        """Bring what the scores are computed from up to date with the engine's CURRENT table (and the module's current
        weights), as ``LinkRanker.prepare`` does: K0 where nobody has left the norms behind and the degree-weighted sums
        of the EXISTING graph for the cosine; for the bilinear score S = Z M^T, M = Phi_src.weight^T Phi_dst.weight, so
        that (Phi_src z) . (Phi_dst z_v) = z . S_v for an iterate z that is in no table."""
        eng, k = self.eng, self.k
        Z = eng.Zcur
        self.sums2 = self.sq = self.S = None
        if self.bilinear:
            d, acc = eng.d, eng.acc_dtype
            Ws = self.sim.Phi_src.weight.detach().to(eng.device, torch.float64)
            Wd = self.sim.Phi_dst.weight.detach().to(eng.device, torch.float64)
            W = torch.zeros(2 * d, d, dtype=acc, device=eng.device)   # project_rows wants [2d, d]: M on zeros
            W[:d] = (Ws.t() @ Wd).to(acc)
            eng._sync_quiet_rows()
            if self._Y is None:
                self._Y = torch.empty(Z.shape[0], _round_up(2 * d, 8), dtype=acc, device=eng.device)
            k.project_rows(Z, d, W, self._Y)
            self.S = self._Y[:, :d]
            self.mode = _hip.SCORE_RAW_DOT
        else:
            self.mode = _hip.SCORE_MODES[eng.cosine_mode]
            if not eng.sq_ok[eng.cur]:                  # nobody has left this table's norms behind: K0
                for b in eng.blocks:
                    k.row_sqnorm(eng._zrows(Z, b), eng.d, eng.sq_pp[eng.cur][eng._rows(b)])
                eng.sq_ok[eng.cur] = True
            sq = eng.sq_pp[eng.cur]                     # one GPU: every table row is an own row, in table order
            if eng.cosine_mode == "reference":
                k.degree_weighted_sums(sq, eng.rowptr, eng.indeg, eng.part.n_local, eng.ws, eng.sums2)
                self.sums2 = eng.sums2
            else:
                self.sq = sq
        self._ready = True

    def _coalesce(self, rowptr, cols, m: int):
        """The neighbour lists on the device, every row sorted by vertex index with repeats removed (the reference
        coalesces duplicate edges): (rowptr int64 [m + 1], cols int64)."""
        eng = self.eng
        rowptr = torch.as_tensor(rowptr, dtype=torch.int64, device=eng.device).reshape(-1)
        cols = torch.as_tensor(cols, dtype=torch.int64, device=eng.device).reshape(-1)
        if rowptr.numel() != m + 1:
            raise ValueError(f"embed: rowptr needs m + 1 = {m + 1} entries, got {rowptr.numel()}")
        deg = rowptr[1:] - rowptr[:-1]
        if int(rowptr[0]) != 0 or (m and int(deg.min()) < 0) or int(rowptr[-1]) != cols.numel():
            raise ValueError("embed: rowptr must start at 0, never decrease and end at len(cols)")
        if cols.numel() and (int(cols.min()) < 0 or int(cols.max()) >= eng.V):
            raise ValueError(f"embed: a neighbour must be an existing vertex, an index in [0, {eng.V}); new vertices "
                             f"cannot link to each other")
        src = torch.repeat_interleave(torch.arange(m, device=eng.device), deg)
        key = torch.unique(src * eng.V + cols)          # sorted: by row, then by vertex index
        counts = torch.zeros(m, dtype=torch.int64, device=eng.device)
        counts.index_add_(0, key // eng.V, torch.ones_like(key))
        out = torch.zeros(m + 1, dtype=torch.int64, device=eng.device)
        out[1:] = torch.cumsum(counts, 0)
        return out, key % eng.V

    def embed(self, X_new, rowptr, cols, gamma: float, tolerence: int = 10, max_rounds: int = 64,
              weights: bool = False, refresh: bool = True) -> NewRows:
        """Embeddings of ``m`` new vertices with content ``X_new [m, d]`` and out-neighbours ``cols[rowptr[i] :
        rowptr[i + 1]]`` (vertex indices of the existing graph).  ``refresh=False``: the caller knows that neither the
        table nor the weights moved since the last call.  Everything stays on the device."""
        eng = self.eng
        X_new = torch.as_tensor(X_new)
        if X_new.dim() != 2 or X_new.shape[1] != eng.d:
            raise ValueError(f"embed: X_new must be [m, {eng.d}], got {tuple(X_new.shape)}")
        if int(tolerence) < 1 or int(max_rounds) < 1:
            raise ValueError("embed: tolerence and max_rounds must be at least 1")
        m = int(X_new.shape[0])
        rowptr, cols = self._coalesce(rowptr, cols, m)
        if refresh or not self._ready:
            self.prepare()
        dev, acc = eng.device, eng.acc_dtype
        Xd = torch.zeros(m, eng.ld, dtype=eng.dtype, device=dev)
        Xd[:, :eng.d] = X_new.to(dev, eng.dtype)
        colidx = eng.pos[cols].to(torch.int32) if cols.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
        Z_out = torch.zeros(m, eng.ld, dtype=eng.dtype, device=dev)
        rounds = torch.zeros(m, dtype=torch.int32, device=dev)
        delta = torch.zeros(m, dtype=acc, device=dev)
        P = torch.zeros(max(int(cols.numel()), 1), dtype=acc, device=dev) if weights else None
        if m:
            self.k.embed_rows(rowptr, colidx.contiguous(), Xd, eng.Zcur, int(eng.Zcur.shape[0]), eng.d, self.mode,
                              self.sums2, self.sq, self.S, float(gamma), int(tolerence), int(max_rounds), Z_out, rounds,
                              delta, P)
        return NewRows(Z=Z_out[:, :eng.d], rounds=rounds, delta=delta, converged=rounds < int(max_rounds),
                       rowptr=rowptr, cols=cols, P=None if P is None else P[:cols.numel()])


# ---- the config's `new_vertices` section (CLI) ------------------------------------------------------------------------
def check_section(section, world_size: int = 1) -> dict:
    """The validated ``new_vertices`` section of a config: ``{"root", "max_rounds", "weights"}``.  Before any graph is
    read."""
    if world_size > 1:
        raise NotImplementedError(
            "new_vertices: embedding new vertices runs on ONE GPU only (WORLD_SIZE > 1): several GPUs and column "
            "divisions are out of scope")
    if not isinstance(section, dict):
        raise ValueError("new_vertices: expected a mapping with the key `root`")
    unknown = sorted(set(section) - set(SECTION_KEYS))
    if unknown:
        raise ValueError(f"new_vertices: unknown keys {unknown}; known: {list(SECTION_KEYS)}")
    if not section.get("root") or not isinstance(section["root"], str):
        raise ValueError("new_vertices: `root` (a directory with V, E and C.npy / C.pt) is required")
    max_rounds = section.get("max_rounds", 64)
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, int) or max_rounds < 1:
        raise ValueError(f"new_vertices: max_rounds must be a positive integer, got {max_rounds!r}")
    weights = section.get("weights", False)
    if not isinstance(weights, bool):
        raise ValueError(f"new_vertices: weights must be true or false, got {weights!r}")
    return {"root": section["root"], "max_rounds": max_rounds, "weights": weights}


def read_arrivals(root: Path, vertex_ids: Sequence[str], d: Optional[int]):
    """(new ids, X_new [m, d] tensor, rowptr, cols) of the directory ``root``: ``V`` (one new id per line), ``E``
    (``new_id<TAB>existing_id`` lines) and ``C.npy`` / ``C.pt`` (content, one row per line of ``V``; required -- there is
    no N(0, 1) fallback here; ``d`` None: the caller checks the width once it knows the graph's).  Every violation is a ValueError / FileNotFoundError that names the file."""
    root = Path(root)
    if not root.is_dir():
        raise FileNotFoundError(f"new_vertices: root {str(root)!r} is not a directory")
    if not (root / "V").exists():
        raise FileNotFoundError(f"new_vertices: {str(root / 'V')!r} is missing")
    with open(root / "V", "r") as io:
        new_ids = [l.strip("\r") for l in io.read().split("\n") if l.strip()]
    existing = {}
    for i, vid in enumerate(vertex_ids):
        existing.setdefault(str(vid), i)
    new_index = {}
    for i, vid in enumerate(new_ids):
        if vid in existing:
            raise ValueError(f"new_vertices: V line {i + 1}: {vid!r} already exists in the graph")
        if vid in new_index:
            raise ValueError(f"new_vertices: V line {i + 1}: {vid!r} is listed twice")
        new_index[vid] = i
    m = len(new_ids)
    if (root / "C.npy").exists():
        X = torch.from_numpy(np.load(root / "C.npy"))
    elif (root / "C.pt").exists():
        X = torch.as_tensor(torch.load(root / "C.pt"))
    else:
        raise FileNotFoundError(f"new_vertices: neither C.npy nor C.pt in {str(root)!r}: new vertices need their content")
    if X.dim() != 2 or X.shape[0] != m or (d is not None and X.shape[1] != d):
        raise ValueError(f"new_vertices: content must be [{m}, {'d' if d is None else d}] (one row per line of V), got "
                         f"{tuple(X.shape)}")
    lists = [[] for _ in range(m)]
    if (root / "E").exists():
        with open(root / "E", "r") as io:
            for n, line in enumerate(io.read().split("\n")):
                if not line.strip():
                    continue
                parts = line.strip("\r").split("\t")
                if len(parts) != 2:
                    raise ValueError(f"new_vertices: E line {n + 1}: expected 'new_id\\texisting_id', got {line!r}")
                if parts[0] not in new_index:
                    raise ValueError(f"new_vertices: E line {n + 1}: source {parts[0]!r} is not a new vertex")
                if parts[1] not in existing:
                    raise ValueError(f"new_vertices: E line {n + 1}: destination {parts[1]!r} is not an existing vertex")
                lists[new_index[parts[0]]].append(existing[parts[1]])
    rowptr, cols = normalize_neighbours(lists, m)
    return new_ids, X, rowptr, cols


def write_results(out_root: Path, new_ids: Sequence[str], vertex_ids: Sequence[str], res: NewRows, similarity,
                  max_rounds: int, weights: bool) -> dict:
    """``Z_new.npy`` (rows in the order of the arrivals' ``V``), ``new_vertices.json`` and, with ``weights``,
    ``P_new.tsv`` (``new_id<TAB>existing_id<TAB>weight``) under ``out_root``; returns the JSON's content."""
    out_root = Path(out_root)
    res = res.cpu()
    Z = res.Z.float() if res.Z.dtype == torch.bfloat16 else res.Z
    np.save(out_root / "Z_new.npy", Z.numpy())
    rounds = res.rounds.numpy()
    hist = np.bincount(rounds, minlength=1)
    deg = np.diff(res.rowptr.numpy())
    report = {"new_vertices": int(len(new_ids)), "edges": int(res.cols.numel()), "max_rounds": int(max_rounds),
              "rounds_histogram": {str(r): int(c) for r, c in enumerate(hist) if c},
              "not_converged": int((~res.converged).sum()), "without_neighbours": int((deg == 0).sum()),
              "similarity": type(similarity).__name__}
    with open(out_root / "new_vertices.json", "w") as io:
        json.dump(report, io, indent=1)
    if weights:
        src = np.repeat(np.arange(len(new_ids)), deg)
        with open(out_root / "P_new.tsv", "w") as io:
            for s, c, p in zip(src.tolist(), res.cols.tolist(), res.P.double().tolist()):
                io.write("%s\t%s\t%.9g\n" % (new_ids[s], vertex_ids[c], p))
    return report
