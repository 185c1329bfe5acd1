"""Training the bilinear similarity (AsymmertricSimilarity) on a SweepEngine -- the reference's
``IterativeEmbedder.update_similarity_measure`` (clane/embedder.py:249-289) as five kernel calls per step and no host
decision: gathered MFMA projection, loss + mask + d loss / d s, MFMA gradient, Adam (which skips itself when no pair
took part in the loss, the reference's ``continue``).  The host reads one scalar per epoch.

``SimilarityTrainer`` holds the optimizer state on the device; ``PairSampler`` draws an epoch's batches with torch ops
on the device from a seeded generator.  Both work on TABLE ROWS of ``eng.Zcur`` (the engine relabels vertices:
``eng.pos`` maps vertex -> table row); callers that think in vertex ids translate with ``rows_of_vertices``.
One GPU only: the pairs of a batch read arbitrary rows, which a row division does not hold and a column division holds
in slices.
"""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import torch


def require_one_gpu(eng) -> None:
    if eng.world > 1 or eng.columns or eng.halo:
        raise NotImplementedError(
            f"training the similarity runs on ONE GPU only: a batch's pairs read arbitrary rows of Z, which this engine "
            f"divides over {eng.world} ranks (exchange={eng.exchange!r}); several GPUs are out of scope")


def rows_of_vertices(eng, vertices) -> torch.Tensor:
    """int32 table rows of ``eng.Zcur`` for vertex ids (any integer tensor / sequence)."""
    v = torch.as_tensor(vertices, dtype=torch.int64, device=eng.device)
    return eng.pos[v].to(torch.int32)


def sorted_adjacency(eng):
    """(rowptr int64 [R + 1], colidx int32, R): the adjacency in TABLE-ROW numbering with every row sorted by column --
    what ``clane_pair_labels`` and the exclusion of ``clane_rank_scores_*`` search.  The engine's own CSR keeps the edges
    of its class rows in (class of the column, column) order, so the adjacency is sorted once more; built once per
    engine and shared by ``PairSampler`` and ``LinkRanker`` (the graph of an engine never changes)."""
    cached = getattr(eng, "_sorted_adjacency", None)
    if cached is not None:
        return cached
    dev = eng.device
    R = eng.part.padded_vertices
    own = torch.from_numpy(eng.part.local_positions()).to(dev)
    deg = (eng.rowptr[1:] - eng.rowptr[:-1])[:eng.part.n_local]
    src = torch.repeat_interleave(own[:deg.numel()], deg)
    key = torch.sort(src * R + eng.colidx[:eng.E_loc].long()).values
    counts = torch.zeros(R, dtype=torch.int64, device=dev)
    counts.index_add_(0, src, torch.ones_like(src))
    rowptr = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(counts, 0)
    colidx = (key % R).to(torch.int32) if key.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
    eng._sorted_adjacency = (rowptr, colidx, R)
    return eng._sorted_adjacency


class SimilarityTrainer:
    """W = cat(Phi_src.weight, Phi_dst.weight) [2d, d], Adam's m and v, the step counter and the epoch-loss accumulator
    on the device, with the buffers of one batch of up to ``batch_size`` pairs (``SweepEngine.similarity_trainer``)."""

    def __init__(self, eng, W0: torch.Tensor, lr: float, batch_size: int):
        require_one_gpu(eng)
        d = eng.d
        if tuple(W0.shape) != (2 * d, d):
            raise ValueError(f"similarity_trainer: W0 must be [2d, d] = [{2 * d}, {d}], got {tuple(W0.shape)}")
        if batch_size < 1:
            raise ValueError("similarity_trainer: batch_size must be at least 1")
        self.eng, self.k, self.d, self.lr, self.batch_size = eng, eng.k, d, float(lr), int(batch_size)
        dev, acc = eng.device, eng.acc_dtype
        self.W = W0.detach().to(dev, acc).contiguous().clone()
        self.m, self.v, self.dW = (torch.zeros_like(self.W) for _ in range(3))
        self.state = torch.zeros(2, dtype=torch.float64, device=dev)       # steps taken, sum of the epoch's step losses
        self.stats = torch.zeros(2, dtype=torch.float64, device=dev)       # the step's sum of masked losses, M
        self.A = torch.empty(batch_size, d, dtype=acc, device=dev)
        self.Bm = torch.empty(batch_size, d, dtype=acc, device=dev)
        self.g = torch.empty(batch_size, dtype=acc, device=dev)
        self.mask = torch.empty(batch_size, dtype=torch.uint8, device=dev)
        self.ws = torch.zeros(self.k.reduce_ws_len(), dtype=torch.float64, device=dev)
        self.grad_ws = torch.empty(self.k.pair_grad_ws_len(batch_size, d), dtype=acc, device=dev)

    def step(self, src_rows: torch.Tensor, dst_rows: torch.Tensor, linked: torch.Tensor, u: torch.Tensor) -> None:
        """One optimizer step on a batch: int32 table rows, uint8 labels, uniforms in the accumulate dtype.  Nothing
        comes back to the host."""
        B, d, k = src_rows.numel(), self.d, self.k
        if not 1 <= B <= self.batch_size:
            raise ValueError(f"step: a batch holds 1..{self.batch_size} pairs, got {B}")
        Z = self.eng.Zcur
        A, Bm, g, mask = self.A[:B], self.Bm[:B], self.g[:B], self.mask[:B]
        k.pair_project(Z, d, src_rows, dst_rows, self.W, A, Bm)
        k.pair_loss(A, Bm, d, linked, u, g, mask, self.ws, self.stats)
        k.pair_grad(Z, d, src_rows, dst_rows, A, Bm, g, self.stats, self.grad_ws, self.dW)
        k.adam_step(self.W, self.m, self.v, self.dW, self.lr, self.stats, self.state)

    def epoch_loss(self) -> float:
        """Sum of the step losses since the last call (skipped steps add nothing); clears the accumulator."""
        total = float(self.state[1].item())
        self.state[1:2].zero_()
        return total

    def steps_taken(self) -> int:
        return int(self.state[0].item())

    def weights(self) -> torch.Tensor:
        """The current [2d, d] weights (a copy, on the device)."""
        return self.W.clone()


class PairSampler:
    """An epoch = a random permutation of the vertices cut into ``V // batch_size`` batches (the DataLoader's
    ``shuffle=True, drop_last=True``, embedder.py:251-258); ``dst`` uniform over the vertices; the label says whether
    (src, dst) is an edge -- the evident intent of graph.py:96-100 (upstream tests a DIFFERENT random vertex than the one
    it returns).  ``positive_fraction`` > 0 replaces that share of ``dst`` by a uniformly drawn
    out-neighbour of ``src`` (rows without out-edges keep their random ``dst``).  Everything is drawn with torch ops on the
    engine's device from ``generator``: same seed, same batches."""

    def __init__(self, engine, batch_size: int, generator: torch.Generator, positive_fraction: float = 0.0):
        require_one_gpu(engine)
        if not 1 <= batch_size <= engine.V:
            raise ValueError(f"PairSampler: batch_size must be in [1, {engine.V}], got {batch_size}")
        if not 0.0 <= positive_fraction <= 1.0:
            raise ValueError("PairSampler: positive_fraction must be in [0, 1]")
        self.eng, self.batch_size, self.gen, self.positive_fraction = engine, int(batch_size), generator, float(positive_fraction)
        self.n_batches = engine.V // self.batch_size
        self.rowptr, self.colidx, self.nrows = sorted_adjacency(engine)

    def _rand(self, n: int) -> torch.Tensor:
        return torch.rand(n, generator=self.gen, device=self.gen.device, dtype=torch.float64).to(self.eng.device)

    def epoch(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]:
        """Yields (src_rows, dst_rows, linked, u) per batch; the whole epoch is drawn and labelled at once."""
        eng, V, n = self.eng, self.eng.V, self.n_batches * self.batch_size
        perm = torch.randperm(V, generator=self.gen, device=self.gen.device).to(eng.device)[:n]
        dst_v = torch.clamp((self._rand(n) * V).long(), max=V - 1)
        src = eng.pos[perm]
        dst = eng.pos[dst_v]
        if self.positive_fraction > 0.0:
            take = self._rand(n) < self.positive_fraction
            pick = self._rand(n)
            a, b = self.rowptr[src], self.rowptr[src + 1]
            has = take & (b > a)
            e = torch.minimum(a + (pick * (b - a).double()).long(), torch.clamp(b - 1, min=0))
            dst = torch.where(has, self.colidx[torch.clamp(e, max=self.colidx.numel() - 1)].long(), dst)
        u = self._rand(n).to(eng.acc_dtype)
        src, dst = src.to(torch.int32).contiguous(), dst.to(torch.int32).contiguous()
        linked = torch.empty(n, dtype=torch.uint8, device=eng.device)
        eng.k.pair_labels(self.rowptr, self.colidx, self.nrows, src, dst, linked)
        B = self.batch_size
        for i in range(self.n_batches):
            s = slice(i * B, (i + 1) * B)
            yield src[s], dst[s], linked[s], u[s]
