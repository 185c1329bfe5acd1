"""Node clustering on a SweepEngine: k-means on the embeddings, every restart advancing at once on the card, scored by
NMI, ARI and purity against labels where there are any -- the experiment the attributed-network-embedding literature runs
beside link prediction and node classification, and the one a graph without labels or held-out edges allows.

One Lloyd iteration is two kernels of csrc/kmeans.h: the assignment is a dense contraction on the matrix cores with the
arg-min over ALL centres fused in (the n x K distances never exist), the update one gather of the rows sorted by
assigned centre, summed in a fixed order.  The restarts are the kernels' R dimension.  What remains for torch is
plumbing: a stable sort of the assignments, a bincount, the stop test and the D^2 sampling of k-means++.

Everything works on TABLE ROWS of the engine's tables (``eng.pos`` maps vertex -> table row).  One GPU only: a fit reads
arbitrary rows of the table.

The initial centres are k-means++ from a seeded torch generator per restart, NOT scikit-learn's random stream: inertia,
NMI and ARI are defined as scikit-learn defines them, the partitions found are those of this module's seeds.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _hip
from .classify import table_and_rows
from .train import require_one_gpu


# ---- metrics: host side -----------------------------------------------------------------------------------------
def contingency(y: torch.Tensor, assign: torch.Tensor, C: int, k: int) -> torch.Tensor:
    """int64 [R, C, k] from y [n] and assign [n, R] (or [C, k] from assign [n]): cont[r, c, j] = rows of class c in
    cluster j of restart r -- one integer bincount."""
    single = assign.dim() == 1
    a = (assign[:, None] if single else assign).long()
    R = a.shape[1]
    key = (torch.arange(R, device=a.device)[None, :] * C + y.long().to(a.device)[:, None]) * k + a
    cont = torch.bincount(key.reshape(-1), minlength=R * C * k).view(R, C, k)
    return cont[0] if single else cont


def clustering_scores(cont: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(nmi, ari, purity) of contingency counts [..., C, k], float64, as scikit-learn's ``normalized_mutual_info_score``
    (arithmetic-mean normalisation, natural logarithm, 0 log 0 = 0) and ``adjusted_rand_score`` give them; purity = the
    share of rows in their cluster's largest class.  A table with one class and one cluster scores nmi 1 and ari 1, and so
    does every table in which no pair of rows is split by one partition and joined by the other."""
    c = cont.double()
    N = c.sum((-2, -1))
    a, b = c.sum(-1), c.sum(-2)                              # class sizes [..., C], cluster sizes [..., k]
    Ns = N.clamp(min=1.0)
    outer = a[..., :, None] * b[..., None, :]
    term = torch.where(c > 0, c / Ns[..., None, None] * (torch.log(c.clamp(min=1.0)) + torch.log(Ns)[..., None, None]
                                                          - torch.log(outer.clamp(min=1.0))), torch.zeros_like(c))
    mi = term.sum((-2, -1)).clamp(min=0.0)

    def entropy(m):
        p = m / Ns[..., None]
        return -torch.where(m > 0, p * torch.log(p.clamp(min=1e-300)), torch.zeros_like(p)).sum(-1)
    ha, hb = entropy(a), entropy(b)
    one_each = ((a > 0).sum(-1) == 1) & ((b > 0).sum(-1) == 1)
    norm = (0.5 * (ha + hb)).clamp(min=torch.finfo(torch.float64).eps)
    nmi = torch.where(one_each, torch.ones_like(mi), (mi / norm).clamp(max=1.0))     # I <= min(H): rounding alone exceeds 1
    # pair counts: tp pairs joined by both partitions, fp / fn joined by one only, tn by neither
    sq = (c * c).sum((-2, -1))
    tp = sq - N
    fp = (b * b).sum(-1) - sq
    fn = (a * a).sum(-1) - sq
    tn = N * N - fp - fn - sq
    denom = (tp + fn) * (fn + tn) + (tp + fp) * (fp + tn)
    agree = (fp == 0) & (fn == 0)
    ari = torch.where(agree, torch.ones_like(tp), 2.0 * (tp * tn - fn * fp) / torch.where(agree, torch.ones_like(denom), denom))
    purity = c.amax(-2).sum(-1) / Ns
    return nmi, ari, purity


# ---- the fit ----------------------------------------------------------------------------------------------------
@dataclass
class KMeansFit:
    centres: torch.Tensor       # [R, k, d], accumulate dtype, on the device
    assign: torch.Tensor        # [n, R] int32: the nearest of ``centres``, ties to the lowest index
    inertia: torch.Tensor       # [R] float64: sum of the squared distances to the assigned centre
    iterations: torch.Tensor    # [R] int64: centre updates until restart r's assignments stopped changing
    converged: torch.Tensor     # [R] bool: the last update changed no assignment
    empty: torch.Tensor         # [R] int64: centres that own no row at the end
    best_restart: int           # lowest inertia, ties to the lowest index


class KMeans:
    """Lloyd's k-means on rows of a table of ``engine``, ``restarts`` runs at once: assign every row to its nearest centre
    (squared Euclidean distance, ties to the lowest centre), move every centre to the mean of its rows (a centre without
    rows stays where it is: no relocation), until no assignment of any restart changes or ``max_iter`` updates were made.
    A restart that has converged is not frozen: at a fixed point an iteration reproduces its own bits."""

    def __init__(self, engine, max_iter: int = 300):
        try:
            require_one_gpu(engine)
        except NotImplementedError:
            raise NotImplementedError(
                f"k-means runs on ONE GPU only: a fit reads arbitrary rows of the table, which this engine "
                f"divides over {engine.world} ranks (exchange={engine.exchange!r}); several GPUs are out of scope") from None
        if max_iter < 0:
            raise ValueError("KMeans: max_iter >= 0")
        self.eng, self.k = engine, engine.k
        self.max_iter = int(max_iter)
        self.passes = {"assign": 0, "update": 0}    # kernel calls of the last fit(), the seeding's included
        self.last_fit: Optional[KMeansFit] = None   # what the last evaluate() found

    def table_and_rows(self, vertices, table: str = "Z"):
        """(table, int32 rows) for vertex indices: the current embeddings ("Z") or the content embeddings ("X")."""
        return table_and_rows(self.eng, vertices, table)

    # ---- pieces -------------------------------------------------------------------------------------------------
    def _gathered(self, Z, rows, acc):
        """Z[rows, :d] in the accumulate dtype, a zero row for an index outside the table (a handful of rows: torch)."""
        r = rows.long()
        inside = (r >= 0) & (r < Z.shape[0])
        return Z[r.clamp(0, Z.shape[0] - 1), :self.eng.d].to(acc) * inside[:, None].to(acc)

    def _csq(self, centres):
        R, K, d = centres.shape
        csq = torch.empty(R * K, dtype=centres.dtype, device=centres.device)
        self.k.row_sqnorm(centres.view(R * K, d), d, csq)
        return csq.view(R, K)

    def _assign(self, Z, rows, centres, csq, assign, best):
        self.k.kmeans_assign(Z, self.eng.d, rows, centres, csq, assign, best)
        self.passes["assign"] += 1

    def seed_centres(self, Z, rows, zsq, k: int, restarts: int, seed: int):
        """k-means++ per restart, ([R, k, d] centres, int64 [R, k] positions in ``rows``): the first centre is a row drawn
        from a CPU generator seeded ``seed + r``; each further one is drawn with probability proportional to the squared
        distance to the nearest centre so far, by inverse CDF (a float64 cumsum, searchsorted of a uniform from the same
        generator), so a row at distance 0 -- a row already drawn among them -- is never drawn.  One kmeans_assign call
        with the R newest centres (K = 1 per restart) updates the running minimum.  Where every row coincides with a
        centre the draw is uniform.  NOT scikit-learn's stream."""
        dev, acc = Z.device, _hip.acc_dtype(Z.dtype)
        n, R = rows.numel(), int(restarts)
        gens = [torch.Generator().manual_seed(int(seed) + r) for r in range(R)]
        picks = torch.empty(R, k, dtype=torch.int64)
        picks[:, 0] = torch.stack([torch.randint(n, (1,), generator=g)[0] for g in gens])
        centres = torch.empty(R, k, self.eng.d, dtype=acc, device=dev)
        centres[:, 0] = self._gathered(Z, rows[picks[:, 0].to(dev)], acc)
        mind = torch.full((R, n), float("inf"), dtype=torch.float64, device=dev)
        assign = torch.empty(n, R, dtype=torch.int32, device=dev)
        best = torch.empty(n, R, dtype=acc, device=dev)
        lanes = torch.arange(R, device=dev)
        for j in range(1, k):
            newest = centres[:, j - 1:j].contiguous()
            self._assign(Z, rows, newest, self._csq(newest), assign, best)
            mind = torch.minimum(mind, (zsq[None, :] + best.T.double()).clamp(min=0.0))
            mind[lanes[:, None], picks[:, :j].to(dev)] = 0.0          # a drawn row is at distance 0 from its own copy
            for r, g in enumerate(gens):                              # restart by restart: the same scan whatever R is
                cdf = mind[r].clone().cumsum(0)
                total = float(cdf[-1])
                u = float(torch.rand(1, generator=g, dtype=torch.float64))
                fallback = int(torch.randint(n, (1,), generator=g))
                if total > 0.0:
                    target = torch.tensor([min(u * total, float(torch.nextafter(cdf[-1], cdf[-1] * 0)))],
                                          dtype=torch.float64, device=dev)
                    picks[r, j] = min(int(torch.searchsorted(cdf, target, right=True)), n - 1)
                else:
                    picks[r, j] = fallback
            centres[:, j] = self._gathered(Z, rows[picks[:, j].to(dev)], acc)
        return centres, picks

    # ---- the batched fit ----------------------------------------------------------------------------------------
    def fit(self, Z: torch.Tensor, rows: torch.Tensor, k: int, restarts: int = 10, seed: int = 0,
            init: Optional[torch.Tensor] = None) -> KMeansFit:
        """Cluster the rows ``rows`` (int32 table rows of ``Z``) into ``k`` clusters, ``restarts`` times: from the centres
        ``init`` ([R, k, d]) or from k-means++ seeded ``seed + r``."""
        eng, kern = self.eng, self.k
        dev, d = Z.device, eng.d
        acc = _hip.acc_dtype(Z.dtype)
        rows = rows.to(dev, torch.int32).contiguous()
        n, k = int(rows.numel()), int(k)
        if n < 1 or k < 1:
            raise ValueError(f"fit: at least one row and one cluster, got n = {n}, k = {k}")
        self.passes = {"assign": 0, "update": 0}
        sq = torch.empty(Z.shape[0], dtype=acc, device=dev)
        kern.row_sqnorm(Z, d, sq)
        r64 = rows.long()
        inside = (r64 >= 0) & (r64 < Z.shape[0])
        zsq = sq[r64.clamp(0, Z.shape[0] - 1)].double() * inside.double()
        if init is None:
            if restarts < 1:
                raise ValueError("fit: restarts >= 1")
            centres, _ = self.seed_centres(Z, rows, zsq, k, restarts, seed)
        else:
            if init.dim() != 3 or init.shape[1] != k or init.shape[2] != d:
                raise ValueError(f"fit: init must be [R, k = {k}, d = {d}], got {tuple(init.shape)}")
            centres = init.to(dev, acc).contiguous().clone()
        R = int(centres.shape[0])
        csq = self._csq(centres)
        centres_new, csq_new = torch.empty_like(centres), torch.empty_like(csq)
        ws = torch.empty(kern.kmeans_update_ws_len(n, R, k, d), dtype=acc, device=dev)
        assign = torch.empty(n, R, dtype=torch.int32, device=dev)
        best = torch.empty(n, R, dtype=acc, device=dev)
        offset = (torch.arange(R, device=dev) * k)[:, None]
        zero = torch.zeros(1, dtype=torch.int64, device=dev)

        self._assign(Z, rows, centres, csq, assign, best)
        changed = torch.ones(R, dtype=torch.bool, device=dev)
        last_change = torch.zeros(R, dtype=torch.int64, device=dev)
        done = 0
        while done < self.max_iter:
            key = (assign.T.long() + offset).reshape(-1)                # restart-major: restart r's keys in [r k, (r + 1) k)
            perm = torch.sort(key, stable=True).indices
            order = rows[perm % n].contiguous()
            seg = torch.cat([zero, torch.bincount(key, minlength=R * k).cumsum(0)])
            kern.kmeans_update(Z, d, order, seg, centres, ws, centres_new, csq_new)
            self.passes["update"] += 1
            centres, centres_new, csq, csq_new = centres_new, centres, csq_new, csq
            previous = assign.clone()
            self._assign(Z, rows, centres, csq, assign, best)
            changed = (assign != previous).any(0)                       # integer compare on the device
            last_change = torch.where(changed, torch.full_like(last_change, done + 1), last_change)
            done += 1
            if not bool(changed.any()):                                 # the one host read of the iteration
                break
        dist = (zsq[None, :] + best.T.double()).clamp(min=0.0)            # [R, n]
        inertia = torch.stack([dist[r].clone().sum() for r in range(R)])         # restart by restart: the same sum whatever R is
        counts = torch.bincount((assign.T.long() + offset).reshape(-1), minlength=R * k).view(R, k)
        iterations = torch.minimum(last_change + 1, torch.full_like(last_change, done))
        return KMeansFit(centres=centres, assign=assign, inertia=inertia, iterations=iterations, converged=~changed,
                         empty=(counts == 0).sum(1), best_restart=int(torch.argmin(inertia)))

    # ---- the experiment -----------------------------------------------------------------------------------------
    def evaluate(self, vertices, k: Optional[int] = None, y=None, n_classes: Optional[int] = None, restarts: int = 10,
                 seed: int = 0, table: str = "Z") -> dict:
        """Cluster the vertices' rows of ``table`` into ``k`` clusters (default: the number of classes of ``y``) and, with
        classes ``y`` in [0, n_classes), score every restart against them.  The best restart is the one of lowest
        inertia -- chosen without the labels."""
        if k is None and y is None:
            raise ValueError("evaluate: give k, the number of clusters, or the classes y it defaults to")
        Z, rows = self.table_and_rows(vertices, table)
        n = rows.numel()
        C = None
        if y is not None:
            y = torch.as_tensor(y, dtype=torch.int64).reshape(-1)
            if y.numel() != n:
                raise ValueError("evaluate: one class per clustered vertex")
            C = int(n_classes) if n_classes is not None else int(y.max()) + 1
            if n and (int(y.min()) < 0 or int(y.max()) >= C):
                raise ValueError(f"evaluate: classes must be in [0, {C})")
        k = int(k) if k is not None else C
        fit = self.fit(Z, rows, k, restarts=restarts, seed=seed)
        b = fit.best_restart
        out = {
            "table": table, "clustered": n, "clusters": k, "restarts": int(restarts), "seed": int(seed),
            "inertia": float(fit.inertia[b]), "iterations": int(fit.iterations[b]), "converged": bool(fit.converged[b]),
            "empty": int(fit.empty[b]), "best_restart": b,
            "sizes": torch.bincount(fit.assign[:, b].long(), minlength=k).tolist(),
        }
        if y is not None:
            nmi, ari, purity = clustering_scores(contingency(y.to(Z.device), fit.assign, C, k))
            out.update({"nmi": float(nmi[b]), "ari": float(ari[b]), "purity": float(purity[b]),
                        "per_restart": {"inertia": fit.inertia.tolist(), "nmi": nmi.tolist(), "ari": ari.tolist(),
                                        "iterations": fit.iterations.tolist()}})
        self.last_fit = fit
        return out
