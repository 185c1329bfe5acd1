"""Link prediction on a SweepEngine: which links a vertex is most likely to have (``LinkRanker.top_k``) and how probable a
given pair is (``score_pairs`` / ``probabilities``), with the model's own score -- the bilinear
``(Phi_src z_u) . (Phi_dst z_v)`` of ``AsymmertricSimilarity`` (its sigmoid is the probability the module was trained on,
embedder.py:276) or the cosine of ``CosineSimilarity`` in the engine's ``cosine_mode``.  No reference counterpart: the
reference stops at ``Z.npy``.

The scores of a batch of query vertices against ALL vertices are one dense contraction on the matrix cores with the
top-k selection fused in (csrc/link_rank.h): the ``Q x V`` score matrix never exists, and nothing crosses PCIe but the
answer.  How good the model is on held-out edges is the same contraction with the selection replaced by counting
(csrc/link_eval.h): ``LinkRanker.rank_pairs`` gives every pair's exact filtered rank among all vertices, ``evaluate``
the MRR, Hits@K, mean rank and AUC from it; ``hold_out_edges`` makes the held-out set.  Everything works on TABLE ROWS of ``eng.Zcur`` (``eng.pos`` maps vertex -> table row); ids go in and come out
as vertex indices.  One GPU only: a query reads arbitrary rows of the table.
"""
from __future__ import annotations

import shutil
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip, plan
from .train import require_one_gpu, sorted_adjacency

SUPPORTED = "CosineSimilarity and AsymmertricSimilarity"


class LinkRanker:
    def __init__(self, engine, similarity_measure):
        from .similarity import AsymmertricSimilarity, CosineSimilarity
        try:
            require_one_gpu(engine)
        except NotImplementedError:
            raise NotImplementedError(
                f"ranking links runs on ONE GPU only: a query scores against every row of Z, which this engine divides "
                f"over {engine.world} ranks (exchange={engine.exchange!r}); several GPUs are out of scope") from None
        if isinstance(similarity_measure, AsymmertricSimilarity):
            self.bilinear = True
            n_dim = similarity_measure.Phi_src.in_features
            if n_dim != engine.d_full or similarity_measure.Phi_dst.in_features != engine.d_full:
                raise ValueError(f"AsymmertricSimilarity(n_dim={n_dim}) does not fit embeddings of dimension "
                                 f"{engine.d_full}")
        elif isinstance(similarity_measure, CosineSimilarity):
            self.bilinear = False
        else:
            raise NotImplementedError(
                f"link prediction scores with {SUPPORTED}; a plug-in similarity "
                f"({type(similarity_measure).__name__}) has no kernel to score all pairs with")
        self.eng, self.k, self.sim = engine, engine.k, similarity_measure
        self.rows = int(engine.Zcur.shape[0])
        # table row -> vertex, -1 on the padding rows: the id a candidate is reported with, and what breaks ties
        self.label = torch.full((self.rows,), -1, dtype=torch.int32, device=engine.device)
        self.label[engine.pos] = torch.arange(engine.V, dtype=torch.int32, device=engine.device)
        self.query_tile = 64 if engine.acc_dtype == torch.float64 else plan.RANK_QUERY_TILE
        self._ready = False

    # ---- the tables the kernels read ---------------------------------------------------------------------------
    def prepare(self) -> None:
        """Bring what the scores are computed from up to date with the engine's CURRENT embeddings (and the module's
        current weights): the projected table for the bilinear score, the rows' norms / the degree-weighted sums for the
        cosine.  ``top_k`` and ``score_pairs`` call it first unless told ``refresh=False`` (a caller that knows that
        neither the embeddings nor the weights have moved since the last call saves the projection)."""
        eng, k = self.eng, self.k
        Z = eng.Zcur
        self.sums2 = self.sq = None
        if self.bilinear:
            from .bilinear import project_table
            self.S, self.N = project_table(eng, self.sim.stacked_weight(eng.acc_dtype, eng.device))
            self.mode = _hip.SCORE_RAW_DOT
        else:
            self.S = self.N = Z
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

    def _vertices(self, v, what: str) -> torch.Tensor:
        v = torch.as_tensor(v, dtype=torch.int64, device=self.eng.device).reshape(-1)
        if v.numel() and (int(v.min()) < 0 or int(v.max()) >= self.eng.V):
            raise ValueError(f"{what}: vertex indices must be in [0, {self.eng.V})")
        return v

    # ---- the two questions -------------------------------------------------------------------------------------
    def top_k(self, k: int, sources=None, exclude_existing: bool = True, batch: int = 4096,
              refresh: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """(ids [Q, k] int64 vertex indices, scores [Q, k]) on the device: for every source vertex (None: all, in
        vertex order) the k vertices it scores highest against, best first, ties by vertex index; itself never, its
        existing out-neighbours unless ``exclude_existing`` is off.  Places beyond the eligible vertices hold -1 / -inf."""
        if not 1 <= int(k) <= _hip.RANK_MAX_K:
            raise ValueError(f"top_k: k must be in [1, {_hip.RANK_MAX_K}], got {k}")
        if batch < 1:
            raise ValueError("top_k: batch must be at least 1")
        k, eng, kern = int(k), self.eng, self.k
        if refresh or not self._ready:
            self.prepare()
        src = torch.arange(eng.V, device=eng.device) if sources is None else self._vertices(sources, "top_k")
        q_rows = eng.pos[src].to(torch.int32)
        Q = q_rows.numel()
        rowptr = colidx = None
        if exclude_existing:
            rowptr, colidx, _ = sorted_adjacency(eng)
        ids = torch.empty(Q, k, dtype=torch.int32, device=eng.device)
        scores = torch.empty(Q, k, dtype=eng.acc_dtype, device=eng.device)
        for a in range(0, Q, batch):
            b = min(a + batch, Q)
            n_slabs = plan.rank_slabs(b - a, self.rows, self.query_tile)
            cand_s = torch.empty((b - a) * n_slabs * k, dtype=eng.acc_dtype, device=eng.device)
            cand_i = torch.empty((b - a) * n_slabs * k, dtype=torch.int32, device=eng.device)
            kern.rank_scores(self.S, self.N, self.rows, eng.d, q_rows[a:b].contiguous(), self.mode, self.sums2, self.sq,
                             self.label, rowptr, colidx, True, k, n_slabs, cand_s, cand_i)
            kern.rank_merge(cand_s, cand_i, n_slabs, k, scores[a:b], ids[a:b])
        return ids.long(), scores

    def score_pairs(self, src, dst, refresh: bool = True) -> torch.Tensor:
        """score(src[i], dst[i]) for vertex indices, on the device, in the accumulate dtype."""
        eng = self.eng
        s, t = self._vertices(src, "score_pairs"), self._vertices(dst, "score_pairs")
        if s.numel() != t.numel():
            raise ValueError("score_pairs: src and dst must have one entry per pair")
        if refresh or not self._ready:
            self.prepare()
        out = torch.empty(s.numel(), dtype=eng.acc_dtype, device=eng.device)
        self.k.pair_score(self.S, self.N, self.rows, eng.d, eng.pos[s].to(torch.int32).contiguous(),
                          eng.pos[t].to(torch.int32).contiguous(), self.mode, self.sums2, self.sq, out)
        return out

    def probabilities(self, src, dst, refresh: bool = True) -> torch.Tensor:
        """sigmoid(score): the link probability AsymmertricSimilarity is trained to give (embedder.py:276)."""
        return torch.sigmoid(self.score_pairs(src, dst, refresh))

    # ---- how good is the model: ranks of held-out pairs ----------------------------------------------------------
    def rank_pairs(self, src, dst, filter_existing: bool = True, batch: int = 4096, refresh: bool = True):
        """(greater, equal_lower, equal_higher, eligible, score) on the device for the pairs (src[i], dst[i]) of vertex
        indices: among all vertices eligible as a candidate for src[i] -- not src[i] itself, not dst[i], and with
        ``filter_existing`` none of src[i]'s existing out-neighbours (the filtered setting) -- how many score above
        dst[i], how many score exactly the same with a smaller / larger vertex index, and how many there are (int64);
        ``score`` is score(src[i], dst[i]) in the accumulate dtype, bit for bit what ``top_k`` reports for that pair.
        ``1 + greater + equal_lower`` is dst[i]'s place in ``top_k``'s order.  dst[i] itself is never filtered: an edge
        that is still in the graph is ranked among the non-edges."""
        if batch < 1:
            raise ValueError("rank_pairs: batch must be at least 1")
        eng, kern = self.eng, self.k
        s, t = self._vertices(src, "rank_pairs"), self._vertices(dst, "rank_pairs")
        if s.numel() != t.numel():
            raise ValueError("rank_pairs: src and dst must have one entry per pair")
        if refresh or not self._ready:
            self.prepare()
        q_rows, t_rows = eng.pos[s].to(torch.int32), eng.pos[t].to(torch.int32)
        B = q_rows.numel()
        rowptr = colidx = None
        if filter_existing:
            rowptr, colidx, _ = sorted_adjacency(eng)
        counts = torch.empty(B, 4, dtype=torch.int64, device=eng.device)
        score = torch.empty(B, dtype=eng.acc_dtype, device=eng.device)
        for a in range(0, B, batch):
            b = min(a + batch, B)
            n_slabs = plan.rank_slabs(b - a, self.rows, self.query_tile)
            per_slab = torch.empty(b - a, n_slabs, 4, dtype=torch.int32, device=eng.device)
            kern.rank_count(self.S, self.N, self.rows, eng.d, q_rows[a:b].contiguous(), t_rows[a:b].contiguous(),
                            self.mode, self.sums2, self.sq, self.label, rowptr, colidx, True, n_slabs, score[a:b], per_slab)
            total = per_slab.sum(1, dtype=torch.int64)                  # integers: the same for every n_slabs
            counts[a:b] = torch.where(per_slab[:, 0, :] < 0, torch.full_like(total, -1), total)
        return counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3], score

    def evaluate(self, src, dst, hits: Sequence[int] = (1, 3, 10), filter_existing: bool = True) -> "LinkMetrics":
        """MRR, mean rank, Hits@K and AUC of the held-out pairs (src[i], dst[i]) under the exact filtered ranks of
        ``rank_pairs``."""
        greater, lower, higher, eligible, _ = self.rank_pairs(src, dst, filter_existing)
        return link_metrics(greater, lower, higher, eligible, hits)


@dataclass
class LinkMetrics:
    """What ``LinkRanker.evaluate`` reports.  rank = 1 + greater + equal / 2: ties count half, so a model that scores
    everything the same does not get rank 1."""
    pairs: int                  # pairs that were ranked
    skipped: int                # pairs without a rank (counts of -1)
    mrr: float                  # mean of 1 / rank
    mean_rank: float
    hits: Dict[int, float]      # K -> share of the pairs with rank <= K
    auc: float                  # mean share of the eligible candidates the target beats (ties half), pairs with eligible > 0

    def as_dict(self) -> dict:
        return {"pairs": self.pairs, "skipped": self.skipped, "mrr": self.mrr, "mean_rank": self.mean_rank,
                "hits": {str(k): v for k, v in self.hits.items()}, "auc": self.auc}


def link_metrics(greater, equal_lower, equal_higher, eligible, hits: Sequence[int] = (1, 3, 10)) -> LinkMetrics:
    """The metrics from the counts of ``rank_pairs`` (integer tensors, wherever they live: the arithmetic runs there, in
    float64).  No ranked pair: the means are nan."""
    hits = [int(k) for k in hits]
    if any(k < 1 for k in hits):
        raise ValueError("link_metrics: hits must be positive ranks")
    greater = torch.as_tensor(greater)
    ranked = greater >= 0
    g = greater[ranked].double()
    equal = (torch.as_tensor(equal_lower)[ranked] + torch.as_tensor(equal_higher)[ranked]).double()
    el = torch.as_tensor(eligible)[ranked].double()
    rank = 1.0 + g + equal / 2.0
    nan = torch.full((), float("nan"), dtype=torch.float64, device=greater.device)
    mean = lambda x: x.mean() if x.numel() else nan      # noqa: E731
    some = el > 0
    values = torch.stack([mean(1.0 / rank), mean(rank), mean(((el - g - equal / 2.0) / el)[some])]
                         + [mean((rank <= k).double()) for k in hits]).tolist()       # one trip to the host
    return LinkMetrics(pairs=int(g.numel()), skipped=int(greater.numel() - g.numel()), mrr=values[0], mean_rank=values[1],
                       hits=dict(zip(hits, values[3:])), auc=values[2])


# ---- held-out pairs: the file the CLI reads, and the tool that makes one ------------------------------------------
def read_link_pairs(path: Path, vertex_ids: Sequence[str]):
    """(src, dst) lists of vertex indices of the ``src<TAB>dst`` lines of ``path`` (empty lines skipped); an id resolves as
    in the ``E`` file (first occurrence in ``V``), an unknown one is a ValueError naming it."""
    first = {}
    for i, vid in enumerate(vertex_ids):
        first.setdefault(str(vid), i)
    src, dst = [], []
    with open(path, "r") as io:
        for n, line in enumerate(io.read().split("\n")):
            if not line.strip():
                continue
            parts = line.strip("\r").split("\t")
            if len(parts) != 2:
                raise ValueError(f"link_evaluation pairs line {n + 1}: expected 'src\\tdst', got {line!r}")
            for vid in parts:
                if vid not in first:
                    raise ValueError(f"link_evaluation pairs: {vid!r} is not in list")
            src.append(first[parts[0]])
            dst.append(first[parts[1]])
    return src, dst


def split_edges(src: Sequence, dst: Sequence, fraction: float, seed: int) -> np.ndarray:
    """bool [E]: which edges (src[i], dst[i]) to hold out -- a seeded Bernoulli(fraction) draw per DISTINCT edge (the copies
    of a repeated edge go together, so no held-out pair is still in the graph), except that a vertex never loses its last
    out-edge (a row without out-edges stops being updated at all): of a vertex whose every edge was drawn, the first one
    in the list stays."""
    if not 0.0 <= float(fraction) < 1.0:
        raise ValueError("hold_out_edges: fraction must be in [0, 1)")
    edge_of, src_of_edge = {}, []
    which = np.empty(len(src), dtype=np.int64)
    for i, e in enumerate(zip(src, dst)):
        j = edge_of.setdefault(e, len(edge_of))
        if j == len(src_of_edge):
            src_of_edge.append(e[0])
        which[i] = j
    held = np.random.default_rng(seed).random(len(edge_of)) < float(fraction)
    kept_some = set()
    for j, u in enumerate(src_of_edge):
        if not held[j]:
            kept_some.add(u)
    for j, u in enumerate(src_of_edge):                 # first distinct edge of a vertex that would lose them all
        if u not in kept_some:
            held[j] = False
            kept_some.add(u)
    return held[which] if len(src) else np.zeros(0, dtype=bool)


def hold_out_edges(data_root: Path, out_root: Path, fraction: float, seed: int = 0) -> Tuple[int, int]:
    """Write to ``out_root`` a copy of the graph in ``data_root`` (``V``, ``C.npy`` / ``C.pt``) whose ``E`` lacks the edges
    ``split_edges`` draws, and those as ``held_out.tsv`` (the ``pairs`` file of the config's ``link_evaluation`` section).
    Returns (edges kept, edges held out).  Host only."""
    data_root, out_root = Path(data_root), Path(out_root)
    with open(data_root / "E", "r") as io:
        lines = [l for l in io.read().split("\n") if l.strip()]
    pairs = []
    for n, line in enumerate(lines):
        parts = line.split("\t")
        if len(parts) != 2:
            raise ValueError(f"E line {n + 1}: expected 'src\\tdst', got {line!r}")
        pairs.append(parts)
    held = split_edges([p[0] for p in pairs], [p[1] for p in pairs], fraction, seed)
    out_root.mkdir(parents=True, exist_ok=True)
    for name in ("V", "C.npy", "C.pt"):
        if (data_root / name).exists():
            shutil.copyfile(data_root / name, out_root / name)
    for name, take in (("E", ~held), ("held_out.tsv", held)):
        with open(out_root / name, "w") as io:
            io.write("".join(line + "\n" for line, t in zip(lines, take) if t))
    return int((~held).sum()), int(held.sum())


# ---- links.tsv (CLI --predict_links) ----------------------------------------------------------------------------
def read_link_sources(path: Path, vertex_ids: Sequence[str]):
    """Vertex indices of the ids in ``path`` (one per line, in the file's order); an id resolves as in the ``E`` file (first
    occurrence in ``V``), an unknown one is a ValueError naming it."""
    first = {}
    for i, vid in enumerate(vertex_ids):
        first.setdefault(str(vid), i)
    out = []
    with open(path, "r") as io:
        for line in io.read().split("\n"):
            vid = line.strip()
            if not vid:
                continue
            if vid not in first:
                raise ValueError(f"--link_sources: {vid!r} is not in list")
            out.append(first[vid])
    return out


def write_links_tsv(path: Path, vertex_ids: Sequence[str], sources: Optional[Sequence[int]], ids: torch.Tensor,
                    scores: torch.Tensor) -> int:
    """One line ``src_id<TAB>dst_id<TAB>score`` per ranked candidate: sources in the order given (None: vertex order),
    candidates in rank order, ids as in the ``V`` file, scores ``%.9g``; unfilled places (id -1) are omitted.  Returns the
    number of lines."""
    ids, scores = ids.cpu().tolist(), scores.cpu().double().tolist()
    n = 0
    with open(path, "w") as io:
        for i, (row_ids, row_scores) in enumerate(zip(ids, scores)):
            src = vertex_ids[i if sources is None else int(sources[i])]
            for v, s in zip(row_ids, row_scores):
                if v < 0:
                    continue
                io.write("%s\t%s\t%.9g\n" % (src, vertex_ids[v], s))
                n += 1
    return n
