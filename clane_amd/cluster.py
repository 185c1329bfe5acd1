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

Without labels a clustering is scored by its silhouette (``Silhouette``: the n x K sums of distances of
csrc/silhouette.h on the matrix cores, the n x n distances never exist), Calinski-Harabasz and Davies-Bouldin, and
``select_clusters`` keeps the number of clusters with the highest mean silhouette -- inertia falls as k grows and can
do neither.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

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


# ---- scores without labels ----------------------------------------------------------------------------------------
# The silhouette of a partition, from the n x K sums of distances of csrc/silhouette.h (the n x n distances never exist),
# and the two centre-based indices.  All three as scikit-learn defines them (silhouette_samples, calinski_harabasz_score,
# davies_bouldin_score), in float64; cluster ids that own no row are left out of all of them.
SILHOUETTE_METRICS = ("euclidean", "cosine")
SILHOUETTE_SUMS_BYTES = 1 << 27     # the default block of positions keeps the sums S [block, K] within this


def dense_partition(part) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ids, inverse) of any integer partition: the sorted distinct values and each row's index among them."""
    part = torch.as_tensor(part)
    if part.dtype.is_floating_point or part.dtype == torch.bool or part.dim() != 1:
        raise ValueError(f"a partition is one integer per row, got {part.dtype} {tuple(part.shape)}")
    ids, inv = torch.unique(part.long(), sorted=True, return_inverse=True)
    return ids, inv


def silhouette_finish(S: torch.Tensor, own: torch.Tensor, sizes: torch.Tensor) -> torch.Tensor:
    """Per-row silhouette (float64) from S [m, K] (float64: S[i, c] = the sum of row i's distances to the members of
    cluster c, its own term 0), the rows' clusters ``own`` [m] and the cluster sizes [K]: a = S[i, own] / (n_own - 1),
    b = the minimum over the OTHER NON-EMPTY clusters of S[i, c] / n_c, s = (b - a) / max(a, b); s = 0 for a row alone in
    its cluster and where max(a, b) = 0."""
    cnt = sizes.to(S.device).double()
    own = own.to(S.device).long()
    n_own = cnt[own]
    a = S.gather(1, own[:, None])[:, 0] / (n_own - 1.0).clamp(min=1.0)
    means = torch.where(cnt[None, :] > 0, S / cnt.clamp(min=1.0)[None, :], torch.full_like(S, float("inf")))
    b = means.scatter(1, own[:, None], float("inf")).min(1).values
    m = torch.maximum(a, b)
    ok = (n_own > 1) & (m > 0)
    return torch.where(ok, (b - a) / torch.where(ok, m, torch.ones_like(m)), torch.zeros_like(m))


def silhouette_reference(X, part, metric: str = "euclidean") -> torch.Tensor:
    """The definition, restated in float64 on the host: the per-row silhouette of the rows of ``X`` [n, d] under the
    integer partition ``part`` [n], with every pairwise distance formed -- ``euclidean``: sqrt(sum_k (x_ik - x_jk)^2);
    ``cosine``: max(0, 1 - x_i . x_j / (|x_i| |x_j|)), a zero row at distance 1 from every other row.  O(n^2 d): for tests."""
    if metric not in SILHOUETTE_METRICS:
        raise ValueError(f"silhouette_reference: metric must be one of {SILHOUETTE_METRICS}, got {metric!r}")
    X = torch.as_tensor(X).detach().cpu().double()
    ids, own = dense_partition(torch.as_tensor(part).cpu())
    n, K = int(X.shape[0]), int(ids.numel())
    if own.numel() != n:
        raise ValueError("silhouette_reference: one cluster per row")
    if K < 2:
        raise ValueError("silhouette_reference: the silhouette needs at least two non-empty clusters")
    if metric == "cosine":
        nr = (X * X).sum(1).sqrt()
        r = torch.where(nr > 0, 1.0 / nr.clamp(min=1e-300), torch.zeros_like(nr))
    member = torch.nn.functional.one_hot(own, K).double()
    S = torch.empty(n, K, dtype=torch.float64)
    for a in range(0, n, 256):
        x = X[a:a + 256]
        if metric == "euclidean":
            D = ((x[:, None, :] - X[None, :, :]) ** 2).sum(-1).sqrt()
        else:
            D = (1.0 - (x @ X.T) * r[a:a + 256, None] * r[None, :]).clamp(min=0.0)
        i = torch.arange(x.shape[0])
        D[i, a + i] = 0.0
        S[a:a + 256] = D @ member
    return silhouette_finish(S, own, member.sum(0).long())


def calinski_harabasz(centres: torch.Tensor, sizes: torch.Tensor, sq_dist: torch.Tensor) -> float:
    """scikit-learn's calinski_harabasz_score in float64 from the clusters' means ``centres`` [K, d], their sizes [K]
    and the rows' SQUARED distances to their own cluster's mean [n]: (between / (k - 1)) / (within / (n - k)) over the k
    non-empty clusters, 1.0 where within = 0."""
    w = sizes.double()
    live = w > 0
    c, w = centres.double()[live.to(centres.device)].to(w.device), w[live]
    k, n = int(w.numel()), float(w.sum())
    if k < 2 or n <= k:
        raise ValueError(f"calinski_harabasz: needs 2 <= non-empty clusters < rows, got {k} clusters of {int(n)} rows")
    mean = (w[:, None] * c).sum(0) / n
    between = float((w * ((c - mean) ** 2).sum(1)).sum())
    within = float(sq_dist.double().sum())
    return 1.0 if within == 0.0 else between * (n - k) / (within * (k - 1.0))


def davies_bouldin(centres: torch.Tensor, sizes: torch.Tensor, dist: torch.Tensor, assign: torch.Tensor) -> float:
    """scikit-learn's davies_bouldin_score in float64 from the clusters' means ``centres`` [K, d], their sizes [K], the
    rows' distances (NOT squared) to their own cluster's mean [n] and the rows' clusters [n]: the mean over the non-empty
    clusters of max_{c' != c} (s_c + s_c') / |mu_c - mu_c'|, s_c the mean distance of c's rows to its mean; coincident
    means do not count, and the score is 0 where every s_c or every distance between means is 0."""
    w = sizes.to(dist.device).double()
    live = torch.nonzero(w > 0)[:, 0]
    if live.numel() < 2:
        raise ValueError(f"davies_bouldin: needs at least two non-empty clusters, got {int(live.numel())}")
    c = centres.to(dist.device).double()[live]
    dist, assign = dist.double(), assign.to(dist.device).long()
    zero = torch.zeros((), dtype=torch.float64, device=dist.device)
    intra = torch.stack([torch.where(assign == j, dist, zero).sum() for j in live.tolist()]) / w[live]
    cd = ((c[:, None, :] - c[None, :, :]) ** 2).sum(-1).sqrt()
    if bool((intra.abs() <= 1e-8).all()) or bool((cd.abs() <= 1e-8).all()):      # numpy's allclose(x, 0)
        return 0.0
    cd = torch.where(cd == 0, torch.full_like(cd, float("inf")), cd)
    return float(((intra[:, None] + intra[None, :]) / cd).max(1).values.mean())


@dataclass
class SilhouetteResult:
    samples: torch.Tensor               # [n] float64, in the order of ``rows``, on the device
    sizes: torch.Tensor                 # [K] int64
    per_cluster: torch.Tensor           # [K] float64: the mean of a cluster's rows, NaN for an empty cluster
    mean: float
    sums: Optional[torch.Tensor] = None  # [n, K] float64 in the order of ``rows``, with ``keep_sums``


class Silhouette:
    """The exact silhouette of a partition of rows of a table of ``engine``: one norms call and, per block of
    ``block_rows`` positions (default: what keeps the sums within 128 MiB; rounded up to the kernel's 128-row tile), one
    sums call of csrc/silhouette.h and the finish in float64 torch on the device.  The result does not depend on the block
    size, bit for bit."""

    def __init__(self, engine, metric: str = "euclidean", block_rows: Optional[int] = None):
        try:
            require_one_gpu(engine)
        except NotImplementedError:
            raise NotImplementedError(
                f"the silhouette runs on ONE GPU only: it reads arbitrary rows of the table, which this engine divides "
                f"over {engine.world} ranks (exchange={engine.exchange!r}); several GPUs are out of scope") from None
        if metric not in SILHOUETTE_METRICS:
            raise ValueError(f"Silhouette: metric must be one of {SILHOUETTE_METRICS}, got {metric!r}")
        if block_rows is not None and (isinstance(block_rows, bool) or int(block_rows) != block_rows or int(block_rows) < 1):
            raise ValueError(f"Silhouette: block_rows must be a positive integer, got {block_rows!r}")
        self.eng, self.k, self.metric = engine, engine.k, metric
        self.block_rows = None if block_rows is None else int(block_rows)
        self.passes = {"norms": 0, "sums": 0}       # kernel calls of the last samples()

    def table_and_rows(self, vertices, table: str = "Z"):
        """(table, int32 rows) for vertex indices: the current embeddings ("Z") or the content embeddings ("X")."""
        return table_and_rows(self.eng, vertices, table)

    def column_mean(self, Z, rows) -> torch.Tensor:
        """The column mean of the listed rows (float64 [d]) through the library's deterministic column sums."""
        d, n = self.eng.d, int(rows.numel())
        ws = torch.empty(max(1, self.k.column_sums_ws_len(n, d)), dtype=torch.float64, device=Z.device)
        sums = torch.empty(d, dtype=torch.float64, device=Z.device)
        self.k.column_sums(Z, d, rows, ws, sums)
        return sums / n

    def samples(self, Z: torch.Tensor, rows: torch.Tensor, part: torch.Tensor, k: Optional[int] = None,
                mu: Optional[torch.Tensor] = None, keep_sums: bool = False) -> SilhouetteResult:
        """Score the rows ``rows`` (int32 table rows of ``Z``) under the partition ``part`` (one cluster in [0, k) per
        row; ``k`` defaults to the largest + 1; ids without rows are empty clusters and are left out).  ``mu``: the shift
        subtracted from every row for ``euclidean`` (default: the rows' column mean -- distances do not depend on it, the
        rounding of the Gram trick does); ``cosine`` takes the rows as they are."""
        dev, d, kern = Z.device, self.eng.d, self.k
        acc = _hip.acc_dtype(Z.dtype)
        rows = rows.to(dev, torch.int32).contiguous()
        part = torch.as_tensor(part)
        if part.dtype.is_floating_point or part.dtype == torch.bool:
            raise ValueError(f"samples: the partition must be integers, got {part.dtype}")
        part = part.to(dev, torch.int64).reshape(-1)
        n = int(rows.numel())
        if part.numel() != n:
            raise ValueError(f"samples: one cluster per row, got {part.numel()} for {n} rows")
        if n < 2:
            raise ValueError("samples: the silhouette needs at least two rows")
        lo, hi = int(part.min()), int(part.max())
        K = int(k) if k is not None else hi + 1
        if lo < 0 or hi >= K:
            raise ValueError(f"samples: clusters must be in [0, {K}), got [{lo}, {hi}]")
        sizes = torch.bincount(part, minlength=K)
        if int((sizes > 0).sum()) < 2:
            raise ValueError("samples: the silhouette needs at least two non-empty clusters")
        perm = torch.sort(part, stable=True).indices
        order, own = rows[perm].contiguous(), part[perm]
        seg = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), sizes.cumsum(0)])
        if self.metric == "cosine":
            if mu is not None:
                raise ValueError("samples: mu belongs to the euclidean metric; a shift changes cosine distances")
            shift = torch.zeros(d, dtype=acc, device=dev)
        else:
            shift = (self.column_mean(Z, rows) if mu is None else torch.as_tensor(mu).reshape(-1)).to(dev, acc).contiguous()
            if shift.numel() != d:
                raise ValueError(f"samples: mu needs d = {d} entries")
        self.passes = {"norms": 0, "sums": 0}
        nrm = torch.empty(n, dtype=acc, device=dev)
        kern.silhouette_norms(Z, d, order, shift, self.metric, nrm)
        self.passes["norms"] += 1
        block = self.block_rows if self.block_rows is not None else max(1, SILHOUETTE_SUMS_BYTES // (8 * K))
        block = min(-(-block // 128) * 128, -(-n // 128) * 128)
        S = torch.empty(min(block, n), K, dtype=torch.float64, device=dev)
        s_sorted = torch.empty(n, dtype=torch.float64, device=dev)
        kept = torch.empty(n, K, dtype=torch.float64, device=dev) if keep_sums else None
        for p0 in range(0, n, block):
            p1 = min(n, p0 + block)
            kern.silhouette_sums(Z, d, order, seg, shift, nrm, self.metric, p0, p1, S)
            self.passes["sums"] += 1
            s_sorted[p0:p1] = silhouette_finish(S[:p1 - p0], own[p0:p1], sizes)
            if kept is not None:
                kept[perm[p0:p1]] = S[:p1 - p0]
        s = torch.empty_like(s_sorted)
        s[perm] = s_sorted
        bounds = seg.tolist()
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        per = torch.stack([s_sorted[bounds[c]:bounds[c + 1]].sum() / (bounds[c + 1] - bounds[c])
                           if bounds[c + 1] > bounds[c] else nan for c in range(K)])    # cluster by cluster: a fixed order
        return SilhouetteResult(samples=s, sizes=sizes, per_cluster=per, mean=float(s_sorted.sum() / n), sums=kept)


# ---- choosing k ---------------------------------------------------------------------------------------------------
SELECTION_FIELDS = ("clusters", "inertia", "silhouette", "calinski_harabasz", "davies_bouldin", "empty")


def check_cluster_counts(k, what: str = "cluster") -> Tuple[List[int], bool]:
    """(the list of cluster counts, whether ``k`` was a sequence): one integer >= 1, or a non-empty sequence of distinct
    integers >= 2 (every candidate is scored by its silhouette, which needs two clusters)."""
    def integer(v):
        return not isinstance(v, bool) and isinstance(v, int)
    if isinstance(k, torch.Tensor):
        k = k.tolist()
    if isinstance(k, (list, tuple, range)):
        ks = list(k)
        if not ks or not all(integer(v) and v >= 2 for v in ks) or len(set(ks)) != len(ks):
            raise ValueError(f"{what}: a list of cluster counts needs distinct integers >= 2, got {k!r}")
        return ks, True
    if not integer(k) or k < 1:
        raise ValueError(f"{what}: the number of clusters must be an integer >= 1 or a list of them, got {k!r}")
    return [k], False


def select_clusters(ks: Sequence[int], run: Callable[[int], dict]) -> dict:
    """Fit and score every candidate (``run(k)``: the result of one scored clustering, with ``silhouette`` -- None where
    the fit left fewer than two non-empty clusters) and return the result of the one with the highest mean silhouette,
    ties to the smaller ``k``, with ``selection = {criterion, candidates, chosen}`` added."""
    results = [run(int(k)) for k in ks]
    best = None
    for i, r in enumerate(results):
        if r.get("silhouette") is None:
            continue
        if best is None or r["silhouette"] > results[best]["silhouette"] or \
                (r["silhouette"] == results[best]["silhouette"] and r["clusters"] < results[best]["clusters"]):
            best = i
    if best is None:
        raise ValueError("cluster: no candidate left two non-empty clusters to score")
    out = dict(results[best])
    out["selection"] = {"criterion": "silhouette",
                        "candidates": [{f: r.get(f) for f in SELECTION_FIELDS} for r in results],
                        "chosen": int(results[best]["clusters"])}
    return out


def score_fit(km: KMeans, sil: Silhouette, Z: torch.Tensor, rows: torch.Tensor, fit: KMeansFit,
              pick: Optional[torch.Tensor] = None) -> dict:
    """``silhouette`` (mean, over the positions ``pick`` of ``rows`` when given), ``silhouette_per_cluster``,
    ``calinski_harabasz`` and ``davies_bouldin`` (over all rows) of the best restart of ``fit``.  The two indices are
    taken about the MEANS of the final assignment (one kmeans_update call), which are the fit's centres once it has
    converged; the silhouette is None where fewer than two clusters own a row."""
    dev, d, kern = Z.device, km.eng.d, km.k
    acc = _hip.acc_dtype(Z.dtype)
    rows = rows.to(dev, torch.int32).contiguous()
    n, b = int(rows.numel()), fit.best_restart
    assign = fit.assign[:, b].long()
    K = int(fit.centres.shape[1])
    sizes = torch.bincount(assign, minlength=K)
    if int((sizes > 0).sum()) < 2:
        return {"silhouette": None, "silhouette_per_cluster": None, "calinski_harabasz": None, "davies_bouldin": None}
    perm = torch.sort(assign, stable=True).indices
    seg = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), sizes.cumsum(0)])
    old = fit.centres[b:b + 1].contiguous()
    means, msq = torch.empty_like(old), torch.empty(1, K, dtype=acc, device=dev)
    ws = torch.empty(kern.kmeans_update_ws_len(n, 1, K, d), dtype=acc, device=dev)
    kern.kmeans_update(Z, d, rows[perm].contiguous(), seg, old, ws, means, msq)
    means = means[0].double()
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    for a in range(0, n, 1 << 16):                              # O(n d) plumbing: the rows' distances to their own mean
        diff = km._gathered(Z, rows[a:a + (1 << 16)], acc).double() - means[assign[a:a + (1 << 16)]]
        d2[a:a + (1 << 16)] = (diff * diff).sum(1)
    if pick is None:
        res = sil.samples(Z, rows, assign, k=K)
    else:
        pick = pick.to(dev)
        sub = assign[pick]
        res = sil.samples(Z, rows[pick], sub, k=K) if int((torch.bincount(sub, minlength=K) > 0).sum()) >= 2 else None
    per = None if res is None else [None if v != v else v for v in res.per_cluster.tolist()]
    return {"silhouette": None if res is None else res.mean, "silhouette_per_cluster": per,
            "calinski_harabasz": calinski_harabasz(means, sizes, d2) if n > int((sizes > 0).sum()) else None,
            "davies_bouldin": davies_bouldin(means, sizes, d2.sqrt(), assign)}


def check_section(section) -> dict:
    """The ``node_clustering`` section's keys for scoring without labels, validated before any work: ``silhouette`` (true /
    false), ``silhouette_metric`` (euclidean / cosine), ``silhouette_points`` (an integer >= 2 or null: score at most so
    many sampled vertices) and ``clusters`` (an integer, or a list of them: the count of highest mean silhouette is kept;
    a list implies ``silhouette``).  Returns the keyword arguments they add to ``Graph.cluster``."""
    kw = {}
    listed = False
    if isinstance(section.get("clusters"), (list, tuple)):      # a single count is read as it always was
        _, listed = check_cluster_counts(section["clusters"], "node_clustering: clusters")
    if "silhouette" in section and not isinstance(section["silhouette"], bool):
        raise ValueError(f"node_clustering: silhouette must be true or false, got {section['silhouette']!r}")
    on = bool(section.get("silhouette", False)) or listed
    if "silhouette_metric" in section and section["silhouette_metric"] not in SILHOUETTE_METRICS:
        raise ValueError(f"node_clustering: silhouette_metric must be one of {list(SILHOUETTE_METRICS)}, got "
                         f"{section['silhouette_metric']!r}")
    if "silhouette_points" in section:
        p = section["silhouette_points"]
        if p is not None and (isinstance(p, bool) or not isinstance(p, int) or p < 2):
            raise ValueError(f"node_clustering: silhouette_points must be an integer >= 2 or null, got {p!r}")
    for key in ("silhouette_metric", "silhouette_points"):
        if key in section and not on:
            raise ValueError(f"node_clustering: {key} belongs to silhouette: true (or a list of clusters)")
        if key in section:
            kw[key] = section[key]
    if on:
        kw["silhouette"] = True
    return kw
