"""Node classification on a SweepEngine: the experiment the reference publishes (README.md:51-73) -- a multi-class
logistic regression on the embeddings for train shares of 10 % ... 90 % and several random splits per share, micro and
macro F1 -- with every fit of the table advancing at once on the card.

The fits differ only in which rows train them.  Their weights are stacked (``W_all [F * Cp, d]``, ``Cp`` = the classes
rounded up to a power of two), so one pass over the labelled rows is one dense contraction on the matrix cores with the
soft-max, the loss, its gradient w.r.t. the logits and the arg-max fused in (csrc/label_probe.h), and the weights'
gradient is the transposed contraction: ``Z`` is read once per pass instead of once per fit.  What remains for torch is
a batched L-BFGS on the ``[F, Cp (d + 1)]`` parameters, the split masks and the integer confusion counts.

Everything works on TABLE ROWS of the engine's tables (``eng.pos`` maps vertex -> table row).  One GPU only: a probe
reads arbitrary rows of the table.

Two things differ from ``tools/evaluate_f1.py`` on purpose: the splits are a seeded torch permutation, not scikit-learn's
``train_test_split`` stream, and the optimiser is this module's L-BFGS, not scipy's -- the objective, its minimum and
the F1 definitions are the same.

Multi-label data (a SET of classes per vertex: BlogCatalog, Flickr, PPI, Wikipedia POS) is opt-in: ``multilabel=True``
switches to DeepWalk's protocol -- one-vs-rest logistic regressions on the same stacked weights with the sigmoid epilogue
of csrc/multilabel_probe.h, and for a test vertex with k true classes the k classes of highest score.  Class sets travel
as 64-bit masks in int64 tensors (bit c: class c), predictions too.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from .train import require_one_gpu

DEFAULT_RATIOS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
G_BUDGET_BYTES = 8 << 30            # the [n, Fg * Cp] soft-max gradient of one group of fits


# ---- labels, splits, metrics: host side -------------------------------------------------------------------------
def read_labels(path: Path, vertex_ids: Sequence[str], multilabel: bool = False):
    """(vertices, y, classes) of the ``id<TAB>class`` lines of ``path`` (empty lines skipped): any subset of the vertices
    in any order; an id resolves as in the ``E`` file (first occurrence in ``V``).  An unknown or repeated id and a
    malformed line are a ValueError naming the line.  Classes are indexed in sorted order.

    ``multilabel=True``: a repeated id ADDS a class to the vertex (a repeated (id, class) pair is a ValueError naming
    the line); the return is (vertices, masks, classes) with the vertices in order of first appearance and ``masks`` one
    Python int per vertex, bit c set for class c.  More than 64 classes are a ValueError."""
    first = {}
    for i, vid in enumerate(vertex_ids):
        first.setdefault(str(vid), i)
    vertices, names, seen = [], [], {}
    with open(path, "r") as io:
        for n, line in enumerate(io.read().split("\n")):
            if not line.strip():
                continue
            parts = line.strip("\r").split("\t")
            if len(parts) != 2:
                raise ValueError(f"labels line {n + 1}: expected 'id\\tclass', got {line!r}")
            vid, name = parts
            if vid not in first:
                raise ValueError(f"labels line {n + 1}: {vid!r} is not in list")
            if multilabel:
                if (vid, name) in seen:
                    raise ValueError(f"labels line {n + 1}: {vid!r} was given class {name!r} on line "
                                     f"{seen[(vid, name)]} already")
                seen[(vid, name)] = n + 1
            else:
                if vid in seen:
                    raise ValueError(f"labels line {n + 1}: {vid!r} was labelled on line {seen[vid]} already")
                seen[vid] = n + 1
            vertices.append(first[vid])
            names.append(name)
    classes = sorted(set(names))
    index = {c: i for i, c in enumerate(classes)}
    if not multilabel:
        return vertices, [index[c] for c in names], classes
    if len(classes) > _hip.PROBE_MAX_CLASSES:
        raise ValueError(f"labels: {len(classes)} classes; the multi-label probe handles at most {_hip.PROBE_MAX_CLASSES}")
    masks = {}                                              # dicts keep the order of first appearance
    for v, name in zip(vertices, names):
        masks[v] = masks.get(v, 0) | (1 << index[name])
    return list(masks), list(masks.values()), classes


def index_classes(labels: Sequence) -> Tuple[List[int], list]:
    """(y, classes): arbitrary class names indexed in sorted order."""
    classes = sorted(set(labels))
    index = {c: i for i, c in enumerate(classes)}
    return [index[c] for c in labels], classes


def train_count(n: int, ratio: float) -> int:
    """Rows that train at share ``ratio`` of ``n`` labelled rows: round(ratio n), half up, at least 1, at most n - 1."""
    return min(n - 1, max(1, int(math.floor(ratio * n + 0.5))))


def make_splits(n: int, ratios: Sequence[float], runs: int, seed: int) -> Tuple[torch.Tensor, List[Tuple[float, int]]]:
    """(split uint8 [n, F] on the CPU, [(ratio, run)] per fit), F = len(ratios) * runs, ratio-major.  Run r permutes the n
    labelled rows with a CPU generator seeded ``seed + r`` (the same permutation for every ratio, as a fixed
    ``random_state`` gives in the tool); the first ``train_count`` rows of the permutation train, the rest test.  NOT
    scikit-learn's split stream."""
    if n < 2:
        raise ValueError(f"a split needs at least 2 labelled vertices, got {n}")
    if runs < 1 or not len(ratios) or any(not 0.0 < float(r) < 1.0 for r in ratios):
        raise ValueError("ratios must lie in (0, 1) and runs be at least 1")
    perms = [torch.randperm(n, generator=torch.Generator().manual_seed(int(seed) + r)) for r in range(runs)]
    split = torch.zeros(n, len(ratios) * runs, dtype=torch.uint8)
    fits = []
    for a, ratio in enumerate(ratios):
        for r in range(runs):
            split[perms[r][:train_count(n, float(ratio))], a * runs + r] = 1
            fits.append((float(ratio), r))
    return split, fits


def f1_from_confusion(conf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(micro, macro) F1 of confusion counts [..., C, C] (conf[t, p]: rows of true class t predicted p), as scikit-learn's
    ``f1_score`` gives for single-label data: micro = accuracy; macro = the mean of the per-class F1 over the classes
    that occur in the truth or in the predictions, a class without a true positive counting 0.  float64."""
    conf = conf.double()
    tp = torch.diagonal(conf, dim1=-2, dim2=-1)
    truth, predicted = conf.sum(-1), conf.sum(-2)
    denom = truth + predicted                               # 2 tp + fp + fn
    f1 = torch.where(denom > 0, 2.0 * tp / denom.clamp(min=1.0), torch.zeros_like(denom))
    present = (denom > 0).double()
    macro = (f1 * present).sum(-1) / present.sum(-1).clamp(min=1.0)
    micro = tp.sum(-1) / conf.sum((-2, -1)).clamp(min=1.0)
    return micro, macro


def confusion_counts(y: torch.Tensor, pred: torch.Tensor, test: torch.Tensor, C: int) -> torch.Tensor:
    """int64 [F, C, C] from y [n], pred [n, F] and the test mask [n, F]: one integer bincount of y C + pred per fit."""
    F = pred.shape[1]
    key = (torch.arange(F, device=pred.device)[None, :] * C + y.long()[:, None]) * C + pred.long()
    return torch.bincount(key[test], minlength=F * C * C).view(F, C, C)


# ---- multi-label: class sets as 64-bit masks -----------------------------------------------------------------------
def label_masks(sets_or_masks, C: int) -> torch.Tensor:
    """int64 [n] on the CPU, bit c of entry i set where row i has class c (the uint64 pattern: class 63 is the sign bit).
    ``sets_or_masks``: an integer tensor of masks, or per row a collection of class indices in [0, C) or an int mask."""
    if not 1 <= int(C) <= _hip.PROBE_MAX_CLASSES:
        raise ValueError(f"the multi-label probe handles 1..{_hip.PROBE_MAX_CLASSES} classes (C > 64 is out of scope), "
                         f"got {C}")
    if isinstance(sets_or_masks, torch.Tensor):
        if sets_or_masks.dtype.is_floating_point or sets_or_masks.dtype == torch.bool:
            raise ValueError("label_masks: a tensor must hold integer masks")
        out = sets_or_masks.detach().cpu().to(torch.int64).reshape(-1).clone()
    else:
        values = []
        for i, item in enumerate(sets_or_masks):
            if isinstance(item, int):
                m = item
            else:
                m = 0
                for c in item:
                    c = int(c)
                    if not 0 <= c < C:
                        raise ValueError(f"label_masks: row {i}: class {c} is not in [0, {C})")
                    m |= 1 << c
            if not 0 <= m < (1 << 64):
                raise ValueError(f"label_masks: row {i}: {m} is no 64-bit mask")
            values.append(m - (1 << 64) if m >= (1 << 63) else m)
        out = torch.tensor(values, dtype=torch.int64)
    if C < 64 and out.numel() and bool(((out >> C) != 0).any()):
        raise ValueError(f"label_masks: a mask has a bit at or above C = {C}")
    return out


def mask_bits(masks: torch.Tensor, C: int) -> torch.Tensor:
    """bool [..., C]: bit c of every mask."""
    return ((masks.unsqueeze(-1) >> torch.arange(C, device=masks.device)) & 1).bool()


def column_states(masks: torch.Tensor, split: torch.Tensor, C: int) -> torch.Tensor:
    """int8 [F, C] from masks [n] and split [n, F]: 0 a column to fit; -1 where no training row of the fit has the class
    (or nothing trains the fit); +1 where every training row has it."""
    trains = (split != 0).double()
    pos = trains.T @ mask_bits(masks, C).double()                       # [F, C]: counts, exact in float64
    n_train = trains.sum(0)[:, None]
    state = torch.zeros(pos.shape, dtype=torch.int8, device=pos.device)
    state[pos == n_train] = 1
    state[pos == 0] = -1                                                # also n_train == 0
    return state


def multilabel_counts(masks: torch.Tensor, pred: torch.Tensor, test: torch.Tensor, C: int) -> torch.Tensor:
    """int64 [F, C, 3] = (tp, fp, fn) per fit and class over the fit's test rows, from masks [n], pred [n, F] (masks)
    and the test mask [n, F], by integer bit operations."""
    y, p = masks.to(pred.device)[:, None], pred
    keep = torch.where(test, torch.full_like(p, -1), torch.zeros_like(p))        # all bits / none
    count = lambda m: mask_bits(m & keep, C).to(torch.int64).sum(0)     # noqa: E731
    return torch.stack([count(y & p), count(~y & p), count(y & ~p)], dim=-1)


def f1_from_counts(counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(micro, macro) F1 of (tp, fp, fn) counts [..., C, 3], as scikit-learn's ``f1_score`` gives on indicator matrices
    with ``zero_division=0``: micro = 2 sum TP / (2 sum TP + sum FP + sum FN); macro = the mean over ALL C classes of
    2 TP / (2 TP + FP + FN), a class with an empty denominator counting 0.  float64."""
    c = counts.double()
    num, den = 2.0 * c[..., 0], 2.0 * c[..., 0] + c[..., 1] + c[..., 2]
    f1 = torch.where(den > 0, num / den.clamp(min=1.0), torch.zeros_like(den))
    sden = den.sum(-1)
    micro = torch.where(sden > 0, num.sum(-1) / sden.clamp(min=1.0), torch.zeros_like(sden))
    return micro, f1.mean(-1)


# ---- tables (shared with cluster.KMeans) --------------------------------------------------------------------------
def table_and_rows(eng, vertices, table: str = "Z"):
    """(table, int32 rows) for vertex indices: the current embeddings ("Z") or the content embeddings ("X")."""
    v = torch.as_tensor(vertices, dtype=torch.int64, device=eng.device).reshape(-1)
    if v.numel() and (int(v.min()) < 0 or int(v.max()) >= eng.V):
        raise ValueError(f"vertex indices must be in [0, {eng.V})")
    if table == "Z":
        return eng.Zcur, eng.pos[v].to(torch.int32).contiguous()
    if table == "X":
        xrow = getattr(eng, "_x_row_of_vertex", None)
        if xrow is None:                      # X_loc is in local-row order: vertex -> local row, once per engine
            verts = torch.from_numpy(eng.local.vertex).to(eng.device).long()
            ok = verts >= 0
            xrow = torch.full((eng.V,), -1, dtype=torch.int64, device=eng.device)
            xrow[verts[ok]] = torch.arange(verts.numel(), device=eng.device)[ok]
            eng._x_row_of_vertex = xrow
        return eng.X_loc, xrow[v].to(torch.int32).contiguous()
    raise ValueError(f"table must be 'Z' or 'X', got {table!r}")


# ---- cross-validation: host side --------------------------------------------------------------------------------
def fold_assignment(n: int, folds: int, seed: int) -> torch.Tensor:
    """int64 [n] on the CPU: the fold of every labelled row -- the row at position p of one CPU permutation seeded
    ``seed`` is in fold p mod folds."""
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))
    fold = torch.empty(n, dtype=torch.int64)
    fold[perm] = torch.arange(n) % int(folds)
    return fold


def choose_l2(table: Sequence[dict]) -> float:
    """The l2 of the row of lowest ``log_loss``, ties to the larger l2; rows without a used fit (NaN) never."""
    best = None
    for row in table:
        if not row["fits_used"] or math.isnan(row["log_loss"]):
            continue
        if best is None or row["log_loss"] < best["log_loss"] or \
                (row["log_loss"] == best["log_loss"] and row["l2"] > best["l2"]):
            best = row
    if best is None:
        raise ValueError("cross-validation: every fit was skipped (no fold trains on two classes)")
    return float(best["l2"])


def calibration_error(prob: torch.Tensor, correct: torch.Tensor, held: torch.Tensor, bins: int = 10) -> torch.Tensor:
    """float64 [F]: the expected calibration error per fit over its held-out rows -- ``bins`` equal-width bins of the
    top-1 probability prob [n, F]; sum over the bins of (rows in the bin / held-out rows) |accuracy - mean probability|."""
    p = prob.double()
    b = (p * bins).floor().long().clamp(0, bins - 1)
    F = p.shape[1]
    key = (torch.arange(F, device=p.device)[None, :] * bins + b)[held]
    count = torch.bincount(key, minlength=F * bins).double()
    conf = torch.bincount(key, weights=p[held], minlength=F * bins)
    hits = torch.bincount(key, weights=correct.double()[held], minlength=F * bins)
    gap = (hits - conf).abs().view(F, bins).sum(1)                      # n_b |acc_b - conf_b| = |hits_b - conf sum_b|
    return gap / count.view(F, bins).sum(1).clamp(min=1.0)


@dataclass
class Prediction:
    classes: torch.Tensor       # [n, F, top] int32: the classes of highest probability, best first; -1: none left
    probs: torch.Tensor         # [n, F, top], accumulate dtype: their probabilities; 0 where the class is -1
    proba: Optional[torch.Tensor] = None        # [n, F, C]: every class's probability, on request


@dataclass
class CrossValidation:
    rows: List[dict]            # per l2: {l2, log_loss, accuracy | micro_f1, ece (soft-max), fits_used}
    l2: float                   # the chosen value
    folds: int
    seed: int
    fold: torch.Tensor          # [n] int64, CPU: the fold of every labelled row
    split: torch.Tensor         # [n, folds * len(grid)] uint8, CPU: fit g * folds + k trains on the rows outside fold k
    l2_per_fit: torch.Tensor    # [F] float64
    fit: "ProbeFit"
    log_loss: torch.Tensor      # [F] float64: held-out, per held-out row
    score: torch.Tensor         # [F] float64: held-out accuracy / micro-F1
    ece: Optional[torch.Tensor]

    def table(self) -> dict:
        """What a LabelModel keeps and the CLI writes."""
        return {"folds": self.folds, "seed": self.seed, "l2": self.l2, "rows": [dict(r) for r in self.rows]}


# ---- the fit ----------------------------------------------------------------------------------------------------
@dataclass
class ProbeFit:
    W: torch.Tensor             # [F, C, d], accumulate dtype, on the device
    b: torch.Tensor             # [F, C]
    objective: torch.Tensor     # [F] float64: J_f at (W, b)
    grad_max: torch.Tensor      # [F] float64: max |grad J_f| there
    iterations: torch.Tensor    # [F] int64: accepted steps
    converged: torch.Tensor     # [F] bool: grad_max <= gtol
    skipped: torch.Tensor       # [F] bool: fewer than 2 classes among the training rows -- not fitted
    pred: torch.Tensor          # [n, F] int32: arg-max class of EVERY row under fit f
    n_train: torch.Tensor       # [F] int64
    constant: Optional[torch.Tensor] = None     # fit_multilabel: [F] int64, the constant (not fitted) class columns;
    #                                             pred then holds int64 masks, bit c = class c predicted


class LabelProbe:
    """F soft-max regressions on rows of a table of ``engine``, minimising per fit

        J_f = (1 / n_f) [ sum_{i trains f} CE_i + (l2 / 2) ||W_f||^2 ],   bias unpenalised

    (scikit-learn's ``LogisticRegression(C=1 / l2)`` up to the factor 1 / n_f) with a batched L-BFGS: memory ``memory``,
    Armijo backtracking by halving, every fit with its own step, history and convergence flag; a fit is done when
    ``max |grad J_f| <= gtol`` or after ``max_iter`` accepted steps, and done fits are frozen.  If the soft-max gradient
    ``G [n, F Cp]`` would exceed ``g_budget_bytes`` the kernel passes run in groups of fits; the optimiser's state is one
    tensor for all fits either way, and the kernels give a fit the same bits whatever shares its call, so the grouping
    changes no result."""

    C1 = 1e-4               # Armijo
    MAX_HALVINGS = 40

    def __init__(self, engine, l2: float = 1.0, gtol: float = 1e-4, max_iter: int = 2000, memory: int = 10,
                 g_budget_bytes: int = G_BUDGET_BYTES):
        try:
            require_one_gpu(engine)
        except NotImplementedError:
            raise NotImplementedError(
                f"the label probe runs on ONE GPU only: a fit reads arbitrary rows of the table, which this engine "
                f"divides over {engine.world} ranks (exchange={engine.exchange!r}); several GPUs are out of scope") from None
        if l2 < 0 or gtol <= 0 or max_iter < 0 or memory < 1 or g_budget_bytes < 1:
            raise ValueError("LabelProbe: l2 >= 0, gtol > 0, max_iter >= 0, memory >= 1, g_budget_bytes >= 1")
        self.eng, self.k = engine, engine.k
        self.l2, self.gtol, self.max_iter, self.memory = float(l2), float(gtol), int(max_iter), int(memory)
        self.g_budget_bytes = int(g_budget_bytes)
        self.passes = {"forward": 0, "grad": 0}     # kernel calls of the last fit()

    # ---- tables -------------------------------------------------------------------------------------------------
    def table_and_rows(self, vertices, table: str = "Z"):
        """(table, int32 rows) for vertex indices: the current embeddings ("Z") or the content embeddings ("X")."""
        return table_and_rows(self.eng, vertices, table)

    def groups(self, n: int, F: int, Cp: int, acc: torch.dtype) -> List[Tuple[int, int]]:
        per = max(1, self.g_budget_bytes // max(1, n * Cp * torch.empty(0, dtype=acc).element_size()))
        return [(a, min(a + per, F)) for a in range(0, F, per)]

    # ---- the batched fit ----------------------------------------------------------------------------------------
    def fit(self, Z: torch.Tensor, rows: torch.Tensor, y: torch.Tensor, split: torch.Tensor, C: int,
            l2=None) -> ProbeFit:
        """Fit every column of ``split`` (uint8 [n, F]) on the rows ``rows`` (int32 table rows of ``Z``) with classes
        ``y`` (integers in [0, C)).  ``l2``: None -- the constructor's value for every fit -- or one value per fit
        (a sequence or tensor [F])."""
        eng, k = self.eng, self.k
        dev, d = Z.device, eng.d
        acc = _hip.acc_dtype(Z.dtype)
        Cp = _hip.probe_padded_classes(C)
        n, F = int(rows.numel()), int(split.shape[1])
        if split.dtype != torch.uint8 or split.dim() != 2 or split.shape[0] != n or y.numel() != n or F < 1:
            raise ValueError("fit: split must be uint8 [n, F] and y hold one class per row")
        rows = rows.to(dev, torch.int32).contiguous()
        y = y.to(dev, torch.int32).contiguous()
        if n and (int(y.min()) < 0 or int(y.max()) >= C):
            raise ValueError(f"fit: classes must be in [0, {C})")
        split = split.to(dev).contiguous()
        pred = torch.zeros(n, F, dtype=torch.int32, device=dev)
        trains = split != 0
        n_train = trains.sum(0)
        onehot = torch.zeros(n, C, dtype=torch.float64, device=dev)
        onehot[torch.arange(n, device=dev), y.long()] = 1.0
        classes_seen = ((trains.double().T @ onehot) > 0).sum(1)        # [F]: classes among a fit's training rows
        skipped = classes_seen < 2

        def forward(a, b, Wg, bg, loss_ws, loss, G, want_pred):
            k.probe_forward(Z, d, rows, y, split[:, a:b], Wg, bg, b - a, C, loss_ws, loss,
                            G=G, pred=pred[:, a:b] if want_pred else None)

        x, J, gmax, iterations = self._minimise(Z, rows, F, Cp, skipped, n_train, forward, l2)
        nw = Cp * d
        W = x[:, :nw].view(F, Cp, d)[:, :C].to(acc).contiguous()
        b = x[:, nw:][:, :C].to(acc).contiguous()
        return ProbeFit(W=W, b=b, objective=J, grad_max=gmax, iterations=iterations,
                        converged=~skipped & (gmax <= self.gtol), skipped=skipped, pred=pred, n_train=n_train)

    def fit_multilabel(self, Z: torch.Tensor, rows: torch.Tensor, masks: torch.Tensor, split: torch.Tensor, C: int,
                       predict: str = "top_k", l2=None) -> ProbeFit:
        """One-vs-rest: every column of ``split`` fits one binary logistic regression per class on the rows ``rows``,
        whose class sets are ``masks`` (int64 [n], bit c: class c -- ``label_masks``).  The objective is ``J_f`` with the
        sum of the fitted columns' binary cross-entropies in place of the soft-max cross-entropy; it is separable over
        the classes, so its minimiser is ``OneVsRestClassifier(LogisticRegression(C=1 / l2))``'s on the fitted columns.
        A column whose class no / every training row of the fit has is constant: not fitted, weights 0, predicted never
        / always, and counted in ``constant``.  A fit without a fitted column is ``skipped``.  ``pred`` holds int64 masks
        of EVERY row: ``predict="top_k"`` gives a row with k true classes the k classes of highest logit (ties to the
        lowest class; a constant-positive column first, a constant-negative one never), ``"threshold"`` the classes of
        logit > 0.  ``l2`` as in ``fit``."""
        if predict not in ("top_k", "threshold"):
            raise ValueError(f"predict must be 'top_k' or 'threshold', got {predict!r}")
        if not 1 <= int(C) <= _hip.PROBE_MAX_CLASSES:
            raise ValueError(f"the multi-label probe handles 1..{_hip.PROBE_MAX_CLASSES} classes (C > 64 is out of "
                             f"scope), got {C}")
        eng, k = self.eng, self.k
        dev, d = Z.device, eng.d
        acc = _hip.acc_dtype(Z.dtype)
        Cp = _hip.ovr_padded_classes(C)
        n, F = int(rows.numel()), int(split.shape[1]) if split.dim() == 2 else 0
        if split.dtype != torch.uint8 or split.dim() != 2 or split.shape[0] != n or masks.numel() != n or F < 1:
            raise ValueError("fit_multilabel: split must be uint8 [n, F] and masks hold one class set per row")
        if masks.dtype != torch.int64:
            raise ValueError("fit_multilabel: masks must be int64 (label_masks)")
        rows = rows.to(dev, torch.int32).contiguous()
        masks = masks.to(dev).reshape(-1).contiguous()
        if C < 64 and n and bool(((masks >> C) != 0).any()):
            raise ValueError(f"fit_multilabel: a mask has a bit at or above C = {C}")
        split = split.to(dev).contiguous()
        pred = torch.zeros(n, F, dtype=torch.int64, device=dev)
        n_train = (split != 0).sum(0)
        states = column_states(masks, split, C)                         # [F, C]
        col_state = torch.zeros(F, Cp, dtype=torch.int8, device=dev)    # pad columns: ignored by the kernel
        col_state[:, :C] = states
        col_state = col_state.reshape(-1)
        constant = (states != 0).sum(1)
        skipped = constant == C
        max_labels = int(mask_bits(masks, C).sum(1).max()) if n else 0
        top_k = predict == "top_k"

        def forward(a, b, Wg, bg, loss_ws, loss, G, want_pred):
            k.probe_forward_ovr(Z, d, rows, masks, split[:, a:b], Wg, bg, col_state[a * Cp:b * Cp], b - a, C, max_labels,
                                loss_ws, loss, G=G, pred=pred[:, a:b] if want_pred else None, top_k=top_k)

        x, J, gmax, iterations = self._minimise(Z, rows, F, Cp, skipped, n_train, forward, l2)
        nw = Cp * d
        W = x[:, :nw].view(F, Cp, d)[:, :C].to(acc).contiguous()
        b = x[:, nw:][:, :C].to(acc).contiguous()
        return ProbeFit(W=W, b=b, objective=J, grad_max=gmax, iterations=iterations,
                        converged=~skipped & (gmax <= self.gtol), skipped=skipped, pred=pred, n_train=n_train,
                        constant=constant)

    @staticmethod
    def per_fit_l2(l2, F: int) -> torch.Tensor:
        """float64 [F] on the CPU from a sequence or tensor of F values, each >= 0."""
        t = torch.as_tensor(l2, dtype=torch.float64).detach().cpu().reshape(-1)
        if t.numel() != F or not bool(torch.isfinite(t).all()) or bool((t < 0).any()):
            raise ValueError(f"l2 must hold one finite value >= 0 per fit ({F}), got {t.tolist()}")
        return t

    def _minimise(self, Z, rows, F: int, Cp: int, skipped, n_train, forward, l2=None):
        """The batched L-BFGS both probes share: (x [F, Cp (d + 1)], J, grad_max, iterations), then one last pass that
        writes the predictions.  ``forward(a, b, Wg, bg, loss_ws, loss, G, want_pred)`` makes the forward kernel call for
        the fits [a, b) of one group: the losses into ``loss`` [b - a], d loss / d logits into ``G`` unless it is None,
        the predictions where ``want_pred``.  ``l2``: None (``self.l2`` for every fit) or one value per fit."""
        eng, k = self.eng, self.k
        dev, d = Z.device, eng.d
        l2_f = None if l2 is None else self.per_fit_l2(l2, F).to(dev)
        acc = _hip.acc_dtype(Z.dtype)
        n = int(rows.numel())
        groups = self.groups(n, F, Cp, acc)
        Fg = max(b - a for a, b in groups)
        G = torch.empty(n * Fg * Cp, dtype=acc, device=dev)
        loss_ws = torch.empty(k.probe_loss_ws_len(n, Fg), dtype=torch.float64, device=dev)
        grad_ws = torch.empty(k.probe_grad_ws_len(n, Fg * Cp, d), dtype=acc, device=dev)
        dW = torch.empty(Fg * Cp * d, dtype=acc, device=dev)
        db = torch.empty(Fg * Cp, dtype=acc, device=dev)
        self.passes = {"forward": 0, "grad": 0}
        nw, P = Cp * d, Cp * (d + 1)

        n_f = n_train.clamp(min=1).double()

        def evaluate(x, want_grad, which=None, want_pred=False):
            """(J [F], grad [F, P] or None) at x for the fits of the groups that hold a fit of the mask ``which``."""
            loss = torch.zeros(F, dtype=torch.float64, device=dev)
            g = torch.zeros(F, P, dtype=torch.float64, device=dev) if want_grad else None
            need = None if which is None else which.tolist()
            for a, b in groups:
                if need is not None and not any(need[a:b]):
                    continue
                Wg = x[a:b, :nw].reshape((b - a) * Cp, d).to(acc).contiguous()
                bg = x[a:b, nw:].reshape(-1).to(acc).contiguous()
                forward(a, b, Wg, bg, loss_ws, loss[a:b], G if want_grad else None, want_pred)
                self.passes["forward"] += 1
                if want_grad:
                    Kg = (b - a) * Cp
                    k.probe_grad(Z, d, rows, G, grad_ws, dW[:Kg * d], db[:Kg])
                    self.passes["grad"] += 1
                    g[a:b, :nw] = dW[:Kg * d].view(b - a, nw).double()
                    g[a:b, nw:] = db[:Kg].view(b - a, Cp).double()
            Wm = x[:, :nw]
            if l2_f is None:
                J = (loss + 0.5 * self.l2 * (Wm * Wm).sum(1)) / n_f
            else:
                J = (loss + (0.5 * l2_f) * (Wm * Wm).sum(1)) / n_f
            if want_grad:
                g[:, :nw] += self.l2 * Wm if l2_f is None else l2_f[:, None] * Wm
                g /= n_f[:, None]
            return J, g

        eps = torch.finfo(acc).eps
        x = torch.zeros(F, P, dtype=torch.float64, device=dev)
        J, g = evaluate(x, True, ~skipped)
        gmax = g.abs().amax(1)
        done = skipped | (gmax <= self.gtol)
        iterations = torch.zeros(F, dtype=torch.int64, device=dev)
        m = self.memory
        S = torch.zeros(m, F, P, dtype=torch.float64, device=dev)
        Y = torch.zeros(m, F, P, dtype=torch.float64, device=dev)
        rho = torch.zeros(m, F, dtype=torch.float64, device=dev)
        gamma = torch.ones(F, dtype=torch.float64, device=dev)
        has_hist = torch.zeros(F, dtype=torch.bool, device=dev)
        head = count = 0

        for _ in range(self.max_iter):
            if bool(done.all()):
                break
            # the two-loop recursion, every fit with its own pairs (a slot a fit did not fill has rho = 0)
            q = g.clone()
            alphas = []
            slots = [(head - 1 - j) % m for j in range(count)]          # newest first
            for i in slots:
                a_i = rho[i] * (S[i] * q).sum(1)
                q -= a_i[:, None] * Y[i]
                alphas.append(a_i)
            r = q * gamma[:, None]
            for i, a_i in zip(reversed(slots), reversed(alphas)):
                b_i = rho[i] * (Y[i] * r).sum(1)
                r += S[i] * (a_i - b_i)[:, None]
            direction = -r
            gd = (g * direction).sum(1)
            uphill = ~(gd < 0)
            direction = torch.where(uphill[:, None], -g, direction)
            gd = torch.where(uphill, -(g * g).sum(1), gd)
            t = torch.where(has_hist, torch.ones_like(gd), (1.0 / g.abs().sum(1).clamp(min=1e-300)).clamp(max=1.0))

            searching = ~done
            x_new, J_new, g_new = x.clone(), J.clone(), g.clone()
            late = torch.zeros_like(done)
            slack = 8.0 * eps * J.abs()
            for trial in range(self.MAX_HALVINGS):
                xt = torch.where(searching[:, None], x + t[:, None] * direction, x)
                Jt, gt = evaluate(xt, trial == 0, searching)            # the first trial is usually taken: its gradient too
                ok = searching & (Jt <= J + self.C1 * t * gd + slack)
                x_new = torch.where(ok[:, None], xt, x_new)
                J_new = torch.where(ok, Jt, J_new)
                if trial == 0:
                    g_new = torch.where(ok[:, None], gt, g_new)
                else:
                    late |= ok
                searching = searching & ~ok
                t = torch.where(searching, 0.5 * t, t)
                if not bool(searching.any()):
                    break
            failed = searching
            if bool(late.any()):
                _, g2 = evaluate(x_new, True, late)
                g_new = torch.where(late[:, None], g2, g_new)
            moved = ~done & ~failed

            s, yv = x_new - x, g_new - g
            sy, yy = (s * yv).sum(1), (yv * yv).sum(1)
            valid = moved & (sy > 1e-10 * yy) & (yy > 0)
            S[head] = torch.where(valid[:, None], s, torch.zeros_like(s))
            Y[head] = torch.where(valid[:, None], yv, torch.zeros_like(yv))
            rho[head] = torch.where(valid, 1.0 / sy.clamp(min=1e-300), torch.zeros_like(sy))
            gamma = torch.where(valid, sy / yy.clamp(min=1e-300), gamma)
            head, count = (head + 1) % m, min(count + 1, m)
            has_hist = has_hist | valid
            # a fit whose search failed: once more from steepest descent, then it stops where it is
            retry = failed & has_hist
            rho[:, retry] = 0.0
            gamma = torch.where(retry, torch.ones_like(gamma), gamma)
            has_hist = has_hist & ~retry
            x, J, g = x_new, J_new, g_new
            iterations += moved.long()
            gmax = g.abs().amax(1)
            done = done | (gmax <= self.gtol) | (failed & ~retry) | (iterations >= self.max_iter)

        evaluate(x, False, None, want_pred=True)
        return x, J, gmax, iterations

    # ---- applying fitted weights --------------------------------------------------------------------------------
    @staticmethod
    def stacked(W: torch.Tensor, b: torch.Tensor, C: int, Cp: int, acc: torch.dtype, dev):
        """(W_all [F * Cp, d], b_all [F * Cp]) in the kernels' layout from W [F, C, d] (or [C, d]) and b [F, C] (or [C]):
        fit f's class c in row f * Cp + c, zero rows for the pad classes."""
        W = W.reshape(-1, C, W.shape[-1]) if W.dim() != 3 else W
        F, d = int(W.shape[0]), int(W.shape[2])
        b = b.reshape(F, -1)
        if W.shape[1] != C or tuple(b.shape) != (F, C):
            raise ValueError(f"weights must be W [F, C, d] and b [F, C] with C = {C}, got {tuple(W.shape)}, {tuple(b.shape)}")
        W_all = torch.zeros(F, Cp, d, dtype=acc, device=dev)
        b_all = torch.zeros(F, Cp, dtype=acc, device=dev)
        W_all[:, :C] = W.to(dev, acc)
        b_all[:, :C] = b.to(dev, acc)
        return W_all.view(F * Cp, d), b_all.view(-1)

    def predict(self, Z: torch.Tensor, rows: torch.Tensor, W: torch.Tensor, b: torch.Tensor, C: int, top: int = 1,
                proba: bool = False, multilabel: bool = False, col_state=None) -> "Prediction":
        """Apply F models (W [F, C, d], b [F, C]; one model may come as [C, d], [C]) to the rows ``rows`` (int32 table
        rows of ``Z``): per (row, model) the ``top`` classes of highest probability, best first, and their probabilities
        -- soft-max over the C classes, or (``multilabel``) one sigmoid per class with ``col_state`` (int8 [F, C] or [C];
        None: every column fitted) giving a constant column probability 0 / 1.  Ties go to the lowest class; where fewer
        than ``top`` classes can be chosen the rest is -1 / 0.  One kernel pass (csrc/label_predict.h)."""
        top = int(top)
        if not 1 <= top <= _hip.PREDICT_MAX_TOP:
            raise ValueError(f"predict: top must be in 1..{_hip.PREDICT_MAX_TOP}, got {top}")
        dev, acc = Z.device, _hip.acc_dtype(Z.dtype)
        C = int(C)
        Cp = _hip.ovr_padded_classes(C) if multilabel else _hip.probe_padded_classes(C)
        W_all, b_all = self.stacked(W, b, C, Cp, acc, dev)
        d, F = int(W_all.shape[1]), int(W_all.shape[0]) // Cp
        if Z.dim() != 2 or Z.shape[1] < d:
            raise ValueError(f"predict: the table has rows of {tuple(Z.shape)[1:]} elements, the weights need d = {d}")
        rows = rows.to(dev, torch.int32).contiguous()
        n = int(rows.numel())
        state = None
        if multilabel:
            state = torch.zeros(F, Cp, dtype=torch.int8, device=dev)
            if col_state is not None:
                cs = torch.as_tensor(col_state).to(dev, torch.int8).reshape(-1, C)
                if cs.shape[0] != F:
                    raise ValueError(f"predict: col_state must be [F, C] = [{F}, {C}], got {tuple(cs.shape)}")
                state[:, :C] = cs
            state = state.view(-1)
        classes = torch.empty(n, F, top, dtype=torch.int32, device=dev)
        probs = torch.empty(n, F, top, dtype=acc, device=dev)
        full = torch.empty(n, F, C, dtype=acc, device=dev) if proba else None
        self.k.probe_predict(Z, d, rows, W_all, b_all, F, C, classes, probs, proba=full, sigmoid=bool(multilabel),
                             col_state=state)
        return Prediction(classes=classes, probs=probs, proba=full)

    # ---- choosing l2 --------------------------------------------------------------------------------------------
    def cross_validate(self, Z: torch.Tensor, rows: torch.Tensor, y_or_masks: torch.Tensor, C: int, l2_grid,
                       folds: int = 5, seed: int = 0, multilabel: bool = False) -> "CrossValidation":
        """``folds``-fold cross-validation of every l2 of ``l2_grid`` on the labelled rows, all ``folds * len(l2_grid)``
        fits as ONE batched fit (fit g * folds + k: grid value g without fold k).  Folds: one CPU permutation seeded
        ``seed`` (``make_splits``' generator convention), the row at position p of it in fold p mod folds.  Per fit the
        held-out log-loss -- the forward kernel on the complement split at the final weights, over the held-out rows --
        the held-out accuracy (multi-label: micro-F1 of the top-k prediction) and, soft-max only, the expected
        calibration error over 10 equal-width bins of the held-out top-1 probability.  The chosen l2 has the lowest mean
        held-out log-loss over the fits that were not skipped, ties to the larger l2."""
        grid = [float(v) for v in l2_grid]
        folds, C = int(folds), int(C)
        n = int(rows.numel())
        if not grid or any(not (v >= 0 and math.isfinite(v)) for v in grid) or len(set(grid)) != len(grid):
            raise ValueError(f"cross_validate: l2_grid must hold distinct finite values >= 0, got {list(l2_grid)}")
        if not 2 <= folds <= n:
            raise ValueError(f"cross_validate: folds must be in 2..{n} (the labelled rows), got {folds}")
        dev, acc = Z.device, _hip.acc_dtype(Z.dtype)
        fold = fold_assignment(n, folds, seed)
        Fn = folds * len(grid)
        split = (fold[:, None] != torch.arange(folds)[None, :]).to(torch.uint8).repeat(1, len(grid)).contiguous()
        l2_f = torch.tensor(grid, dtype=torch.float64).repeat_interleave(folds)
        rows = rows.to(dev, torch.int32).contiguous()
        held = (split == 0).to(dev)
        comp = held.to(torch.uint8).contiguous()
        n_held = held.sum(0).double()
        loss = torch.zeros(Fn, dtype=torch.float64, device=dev)
        loss_ws = torch.empty(self.k.probe_loss_ws_len(n, Fn), dtype=torch.float64, device=dev)
        ece = None
        if multilabel:
            masks = y_or_masks.to(dev).reshape(-1).contiguous()
            fit = self.fit_multilabel(Z, rows, masks, split, C, predict="top_k", l2=l2_f)
            Cp = _hip.ovr_padded_classes(C)
            W_all, b_all = self.stacked(fit.W, fit.b, C, Cp, acc, dev)
            state = torch.zeros(Fn, Cp, dtype=torch.int8, device=dev)
            state[:, :C] = column_states(masks, split.to(dev), C)
            max_labels = int(mask_bits(masks, C).sum(1).max()) if n else 0
            self.k.probe_forward_ovr(Z, self.eng.d, rows, masks, comp, W_all, b_all, state.view(-1), Fn, C, max_labels,
                                     loss_ws, loss)
            score, _ = f1_from_counts(multilabel_counts(masks, fit.pred, held, C))
        else:
            y = y_or_masks.to(dev, torch.int32).reshape(-1).contiguous()
            fit = self.fit(Z, rows, y, split, C, l2=l2_f)
            Cp = _hip.probe_padded_classes(C)
            W_all, b_all = self.stacked(fit.W, fit.b, C, Cp, acc, dev)
            self.k.probe_forward(Z, self.eng.d, rows, y, comp, W_all, b_all, Fn, C, loss_ws, loss)
            hit = (fit.pred == y[:, None]) & held
            score = hit.sum(0).double() / n_held.clamp(min=1.0)
            top1 = self.predict(Z, rows, fit.W, fit.b, C, top=1)
            ece = calibration_error(top1.probs[:, :, 0], top1.classes[:, :, 0] == y[:, None], held)
        log_loss = loss / n_held.clamp(min=1.0)
        used = ~fit.skipped
        table = []
        for g, v in enumerate(grid):
            sl = slice(g * folds, (g + 1) * folds)
            u = used[sl]
            m = int(u.sum())
            mean = lambda t: float(t[sl][u].double().mean()) if m else float("nan")     # noqa: E731
            row = {"l2": v, "log_loss": mean(log_loss), "micro_f1" if multilabel else "accuracy": mean(score)}
            if ece is not None:
                row["ece"] = mean(ece)
            row["fits_used"] = m
            table.append(row)
        return CrossValidation(rows=table, l2=choose_l2(table), folds=folds, seed=int(seed), fold=fold, split=split,
                               l2_per_fit=l2_f, fit=fit, log_loss=log_loss, score=score, ece=ece)

    def train(self, vertices, y, n_classes: int, l2=1.0, folds: int = 5, seed: int = 0, table: str = "Z",
              multilabel: bool = False, class_names: Optional[Sequence] = None) -> "LabelModel":
        """A kept classifier from the labelled vertices (``evaluate``'s forms of ``y``): a list of ``l2`` is chosen among
        by ``cross_validate``; then ONE fit on all labelled rows at the (chosen) value."""
        Z, rows = self.table_and_rows(vertices, table)
        n, C = int(rows.numel()), int(n_classes)
        if multilabel:
            y = label_masks(y, C)
        else:
            y = torch.as_tensor(y, dtype=torch.int64).reshape(-1)
        if y.numel() != n:
            raise ValueError("train: one class (set) per labelled vertex")
        names = [str(c) for c in range(C)] if class_names is None else [str(c) for c in class_names]
        if len(names) != C:
            raise ValueError(f"train: {len(names)} class names for {C} classes")
        cv = None
        if isinstance(l2, (list, tuple)) or (isinstance(l2, torch.Tensor) and l2.dim() > 0):
            cv = self.cross_validate(Z, rows, y, C, l2, folds=folds, seed=seed, multilabel=multilabel)
            value = cv.l2
        else:
            value = float(l2)
        ones = torch.ones(n, 1, dtype=torch.uint8)
        if multilabel:
            fit = self.fit_multilabel(Z, rows, y, ones, C, l2=[value])
            state = column_states(y.to(Z.device), ones.to(Z.device), C)[0].cpu().numpy()
        else:
            fit = self.fit(Z, rows, y, ones, C, l2=[value])
            state = None
        if bool(fit.skipped[0]):
            raise ValueError("train: the labelled vertices hold fewer than 2 classes" if not multilabel else
                             "train: every class is held by no or by every labelled vertex")
        return LabelModel(W=fit.W[0].cpu().numpy(), b=fit.b[0].cpu().numpy(), class_names=names,
                          multilabel=bool(multilabel), l2=value, col_state=state, d=int(fit.W.shape[2]), table=table,
                          n_train=n, objective=float(fit.objective[0]), iterations=int(fit.iterations[0]),
                          converged=bool(fit.converged[0]), cv=None if cv is None else cv.table())

    # ---- the experiment -----------------------------------------------------------------------------------------
    def evaluate(self, vertices, y, n_classes: Optional[int] = None, ratios: Sequence[float] = DEFAULT_RATIOS,
                 runs: int = 10, seed: int = 0, table: str = "Z", multilabel: bool = False,
                 predict: str = "top_k") -> dict:
        """The README's table for the labelled vertices (vertex indices, classes in [0, n_classes)): per ratio the mean
        micro / macro F1 on the test rows over the runs whose training rows hold at least 2 classes.

        ``multilabel=True``: ``y`` holds a class SET per vertex (``label_masks``' forms), the fits are one-vs-rest
        (``fit_multilabel``), F1 is scikit-learn's on indicator matrices, a run is used unless it has no fitted column,
        and the result also carries ``"multilabel"``, ``"predict"`` and ``"constant_columns"``."""
        Z, rows = self.table_and_rows(vertices, table)
        n = rows.numel()
        if multilabel:
            if n_classes is None:
                raise ValueError("evaluate: multilabel needs n_classes")
            C = int(n_classes)
            y = label_masks(y, C)
            if y.numel() != n:
                raise ValueError("evaluate: one class set per labelled vertex")
            split, fits = make_splits(n, ratios, runs, seed)
            fit = self.fit_multilabel(Z, rows, y, split, C, predict=predict)
            micro, macro = f1_from_counts(multilabel_counts(y.to(Z.device), fit.pred, split.to(Z.device) == 0, C))
        else:
            y = torch.as_tensor(y, dtype=torch.int64).reshape(-1)
            C = int(n_classes) if n_classes is not None else int(y.max()) + 1
            if y.numel() != n:
                raise ValueError("evaluate: one class per labelled vertex")
            split, fits = make_splits(n, ratios, runs, seed)
            fit = self.fit(Z, rows, y, split, C)
            split_d = split.to(Z.device)
            conf = confusion_counts(y.to(Z.device), fit.pred, split_d == 0, C)
            micro, macro = f1_from_confusion(conf)
        used = (~fit.skipped).double()
        per_ratio = lambda v: (v * used).view(len(ratios), runs).sum(1)     # noqa: E731
        n_used = per_ratio(torch.ones_like(used))
        mean = lambda v: (per_ratio(v) / n_used.clamp(min=1.0)).tolist()    # noqa: E731
        micro_r, macro_r, n_used = mean(micro), mean(macro), n_used.tolist()
        nan = float("nan")
        out = {
            "table": table, "labelled": n, "classes": C, "l2": self.l2, "seed": int(seed), "runs": int(runs),
            "rows": [{"ratio": float(r), "micro_f1": micro_r[i] if n_used[i] else nan,
                      "macro_f1": macro_r[i] if n_used[i] else nan, "runs_used": int(n_used[i])}
                     for i, r in enumerate(ratios)],
            "fits": {"ratio": [f[0] for f in fits], "run": [f[1] for f in fits],
                     "iterations": fit.iterations.tolist(), "converged": fit.converged.tolist(),
                     "objective": fit.objective.tolist(), "skipped": fit.skipped.tolist(),
                     "micro_f1": micro.tolist(), "macro_f1": macro.tolist()},
            "skipped_fits": int(fit.skipped.sum()),
        }
        if multilabel:
            out["fits"]["constant_columns"] = fit.constant.tolist()
            out.update(multilabel=True, predict=predict, constant_columns=int(fit.constant.sum()))
        return out


# ---- a kept classifier ------------------------------------------------------------------------------------------
MODEL_KEYS = ("W", "b", "class_names", "multilabel", "l2", "col_state", "d", "table", "n_train", "objective",
              "iterations", "converged", "cv")


@dataclass
class LabelModel:
    """One fitted classifier, on the host: what ``LabelProbe.train`` returns, a file keeps and ``predict_*`` apply."""
    W: np.ndarray               # [C, d], the accumulate dtype of the table it was fitted on
    b: np.ndarray               # [C]
    class_names: List[str]
    multilabel: bool
    l2: float
    col_state: Optional[np.ndarray]     # multi-label: int8 [C], -1 / +1 a class no / every labelled vertex has
    d: int
    table: str
    n_train: int
    objective: float
    iterations: int
    converged: bool
    cv: Optional[dict] = None   # CrossValidation.table(), or None where l2 was given

    def __post_init__(self):
        self.check("LabelModel")

    def check(self, what: str):
        W, b, C = np.asarray(self.W), np.asarray(self.b), len(self.class_names)
        if W.ndim != 2 or W.shape[1] != int(self.d) or b.shape != (W.shape[0],) or W.dtype != b.dtype \
                or W.dtype not in (np.float32, np.float64):
            raise ValueError(f"{what}: W {W.shape} {W.dtype} and b {b.shape} {b.dtype} are no [C, d = {self.d}] weights "
                             f"with their [C] biases")
        if C != W.shape[0]:
            raise ValueError(f"{what}: {C} class names for the {W.shape[0]} classes of W")
        if self.multilabel != (self.col_state is not None) or \
                (self.col_state is not None and np.asarray(self.col_state).shape != (C,)):
            raise ValueError(f"{what}: a multi-label model, and only it, carries col_state [C = {C}]")
        if self.table not in ("Z", "X"):
            raise ValueError(f"{what}: table must be 'Z' or 'X', got {self.table!r}")

    @property
    def C(self) -> int:
        return len(self.class_names)

    def save(self, path) -> Path:
        """One ``.npz`` of MODEL_KEYS, read with numpy alone (no pickle: the names are a string array, cv is JSON)."""
        path = Path(path)
        state = np.zeros(0, dtype=np.int8) if self.col_state is None else np.asarray(self.col_state, dtype=np.int8)
        with open(path, "wb") as io:
            np.savez(io, W=self.W, b=self.b, class_names=np.array(self.class_names, dtype=np.str_),
                     multilabel=np.bool_(self.multilabel), l2=np.float64(self.l2), col_state=state, d=np.int64(self.d),
                     table=np.str_(self.table), n_train=np.int64(self.n_train), objective=np.float64(self.objective),
                     iterations=np.int64(self.iterations), converged=np.bool_(self.converged),
                     cv=np.str_(json.dumps(self.cv)))
        return path

    @classmethod
    def load(cls, path, d: Optional[int] = None) -> "LabelModel":
        """The model of ``save``; ``d``: the width it must have.  A file that is no such archive, a shape that does not
        fit and a class-name count other than W's are a ValueError."""
        name = os.fspath(path)
        try:
            with np.load(name) as z:
                missing = [key for key in MODEL_KEYS if key not in z.files]
                if missing:
                    raise ValueError(f"LabelModel.load: {name!r} lacks {missing}")
                multilabel = bool(z["multilabel"])
                fields = dict(W=np.array(z["W"]), b=np.array(z["b"]), class_names=[str(c) for c in z["class_names"].reshape(-1)],
                              multilabel=multilabel, l2=float(z["l2"]),
                              col_state=np.array(z["col_state"], dtype=np.int8) if multilabel else None, d=int(z["d"]),
                              table=str(z["table"]), n_train=int(z["n_train"]), objective=float(z["objective"]),
                              iterations=int(z["iterations"]), converged=bool(z["converged"]), cv=json.loads(str(z["cv"])))
        except ValueError:
            raise
        except Exception as e:                              # a truncated or foreign file: zipfile / numpy errors
            raise ValueError(f"LabelModel.load: {name!r} is no label model: {type(e).__name__}: {e}") from None
        try:
            model = cls(**fields)
        except ValueError as e:
            raise ValueError(str(e).replace("LabelModel:", f"LabelModel.load: {name!r}:", 1)) from None
        if d is not None and int(d) != model.d:
            raise ValueError(f"LabelModel.load: {name!r} holds a model for d = {model.d}, not {int(d)}")
        return model

    # ---- applying it ------------------------------------------------------------------------------------------------
    def _apply(self, engine, Z, rows, top: int, proba: bool):
        if Z.dim() != 2 or int(Z.shape[1]) < self.d or int(engine.d) != self.d:
            raise ValueError(f"the model was fitted for d = {self.d}; the engine has d = {engine.d} and the table rows of "
                             f"{tuple(Z.shape)[1:]}")
        out = LabelProbe(engine).predict(Z, rows, torch.from_numpy(np.ascontiguousarray(self.W)),
                                         torch.from_numpy(np.ascontiguousarray(self.b)), self.C, top=top, proba=proba,
                                         multilabel=self.multilabel, col_state=self.col_state)
        res = (out.classes[:, 0].cpu().numpy(), out.probs[:, 0].cpu().numpy())
        return res + (out.proba[:, 0].cpu().numpy(),) if proba else res

    def predict_table(self, engine, vertices=None, table: str = "Z", top: int = 3, proba: bool = False):
        """(classes [m, top] int32, probs [m, top][, proba [m, C]]) on the host for the vertices (default: all, in vertex
        order) from the engine's table "Z" or "X"."""
        if vertices is None:
            vertices = torch.arange(engine.V)
        Z, rows = table_and_rows(engine, vertices, table)
        return self._apply(engine, Z, rows, top, proba)

    def predict_rows(self, engine, M: torch.Tensor, top: int = 3, proba: bool = False):
        """The same for the rows of ``M`` [m, d], a device tensor of the table's dtype (``NewVertexEmbedder.embed``'s
        ``Z`` of new vertices, say), read with identity rows."""
        if not isinstance(M, torch.Tensor) or M.dim() != 2 or M.dtype not in (torch.float32, torch.float64, torch.bfloat16):
            raise ValueError("predict_rows: M must be a [m, d] tensor of dtype float32, float64 or bfloat16")
        rows = torch.arange(M.shape[0], dtype=torch.int32, device=M.device)
        return self._apply(engine, M, rows, top, proba)


# ---- the CLI section `label_prediction` -------------------------------------------------------------------------------
SECTION_KEYS = ("labels", "l2", "folds", "seed", "top", "multilabel", "scope", "load")


def check_section(section, data_root, world_size: int = 1) -> dict:
    """The validated ``label_prediction`` section of a config, file paths resolved against ``data_root``: ``{"labels",
    "load" (Paths or None), "l2" (a float or a list), "folds", "seed", "top", "multilabel", "scope"}``.  Before any graph
    is read."""
    if world_size > 1:
        raise NotImplementedError(
            "label_prediction: fitting and applying a label model runs on ONE GPU only (WORLD_SIZE > 1): several GPUs "
            "are out of scope")
    if not isinstance(section, dict):
        raise ValueError("label_prediction: expected a mapping with the key `labels` or `load`")
    unknown = sorted(set(section) - set(SECTION_KEYS))
    if unknown:
        raise ValueError(f"label_prediction: unknown keys {unknown}; known: {list(SECTION_KEYS)}")
    files = {}
    for key in ("labels", "load"):
        value = section.get(key)
        if value is not None and (not isinstance(value, str) or not value):
            raise ValueError(f"label_prediction: {key} must be a file name, got {value!r}")
        files[key] = None if value is None else (Path(value) if Path(value).is_absolute() else Path(data_root) / value)
    if (files["labels"] is None) == (files["load"] is None):
        raise ValueError("label_prediction: give exactly one of `labels` (fit a model) and `load` (apply a saved one)")
    fitting_only = sorted(set(section) & {"l2", "folds", "seed", "multilabel"})
    if files["load"] is not None and fitting_only:
        raise ValueError(f"label_prediction: {fitting_only} only steer a fit and have no effect on a loaded model (it "
                         f"carries its own l2 and multilabel): leave them out with `load`")
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v >= 0   # noqa: E731
    l2 = section.get("l2", 1.0)
    if isinstance(l2, list):
        if not l2 or not all(number(v) for v in l2) or len({float(v) for v in l2}) != len(l2):
            raise ValueError(f"label_prediction: l2 must be a number >= 0 or a list of distinct ones, got {l2!r}")
        l2 = [float(v) for v in l2]
    elif number(l2):
        l2 = float(l2)
    else:
        raise ValueError(f"label_prediction: l2 must be a number >= 0 or a list of distinct ones, got {l2!r}")
    whole = lambda v: isinstance(v, int) and not isinstance(v, bool)    # noqa: E731
    folds = section.get("folds", 5)
    if not whole(folds) or folds < 2:
        raise ValueError(f"label_prediction: folds must be an integer >= 2, got {folds!r}")
    if "folds" in section and not isinstance(l2, list):
        raise ValueError("label_prediction: folds is given but l2 is no list: nothing is cross-validated")
    seed = section.get("seed", 0)
    if not whole(seed):
        raise ValueError(f"label_prediction: seed must be an integer, got {seed!r}")
    top = section.get("top", 3)
    if not whole(top) or not 1 <= top <= _hip.PREDICT_MAX_TOP:
        raise ValueError(f"label_prediction: top must be an integer in 1..{_hip.PREDICT_MAX_TOP}, got {top!r}")
    multilabel = section.get("multilabel", False)
    if not isinstance(multilabel, bool):
        raise ValueError(f"label_prediction: multilabel must be true or false, got {multilabel!r}")
    scope = section.get("scope", "unlabelled")
    if scope not in ("unlabelled", "all"):
        raise ValueError(f"label_prediction: scope must be 'unlabelled' or 'all', got {scope!r}")
    for key, path in files.items():
        if path is not None and not path.is_file():
            raise FileNotFoundError(f"label_prediction: the {key} file {str(path)!r} is missing")
    return {"labels": files["labels"], "load": files["load"], "l2": l2, "folds": folds, "seed": seed, "top": top,
            "multilabel": multilabel, "scope": scope}


def write_predictions_tsv(path, ids: Sequence[str], class_names: Sequence[str], classes: np.ndarray,
                          probs: np.ndarray) -> int:
    """``id<TAB>class<TAB>prob[<TAB>class<TAB>prob]...`` per row, class NAMES best first, probabilities as ``repr`` of
    the float; slots without a class (-1) are left out.  Returns the number of lines."""
    with open(path, "w") as io:
        for vid, cs, ps in zip(ids, classes.tolist(), probs.tolist()):
            io.write("\t".join([str(vid)] + [f"{class_names[c]}\t{float(q)!r}" for c, q in zip(cs, ps) if c >= 0]) + "\n")
    return len(ids)


def run_section(cfg: dict, graph, output_root, say=print) -> Tuple["LabelModel", dict]:
    """What the CLI does for a checked ``label_prediction`` section after ``Z.npy``: fit (or load) the model, write
    ``label_model.npz`` (fitted models only), ``predicted_labels.tsv`` and return (model, the report that becomes
    ``label_prediction.json`` -- the caller adds the arrivals' count and writes it)."""
    output_root = Path(output_root)
    predicted = np.ones(len(graph), dtype=bool)
    if cfg["load"] is not None:
        model = LabelModel.load(cfg["load"], d=graph.d)
        source = "loaded"
    else:
        labelled, y, names = read_labels(cfg["labels"], graph.vertex_ids, multilabel=cfg["multilabel"])
        model = LabelProbe(graph.engine()).train(labelled, y, len(names), l2=cfg["l2"], folds=cfg["folds"],
                                                 seed=cfg["seed"], multilabel=cfg["multilabel"], class_names=names)
        model.save(output_root / "label_model.npz")
        if cfg["scope"] == "unlabelled":
            predicted[labelled] = False
        source = "fitted"
    vertices = np.flatnonzero(predicted)
    if len(vertices):
        _, classes, probs = graph.predict_labels(model, vertices, top=cfg["top"])
    else:
        classes, probs = np.zeros((0, cfg["top"]), np.int32), np.zeros((0, cfg["top"]), np.float32)
    write_predictions_tsv(output_root / "predicted_labels.tsv", [graph.vertex_ids[v] for v in vertices],
                          model.class_names, classes, probs)
    hist = np.histogram(probs[:, 0].astype(np.float64), bins=10, range=(0.0, 1.0))[0] if len(vertices) else np.zeros(10)
    report = {"model": source, "labelled": int(model.n_train), "predicted": int(len(vertices)), "scope": cfg["scope"],
              "class_names": list(model.class_names), "multilabel": bool(model.multilabel), "l2": float(model.l2),
              "cv": model.cv, "iterations": int(model.iterations), "converged": bool(model.converged),
              "objective": float(model.objective), "top": cfg["top"],
              "top1_probability_histogram": [int(c) for c in hist]}
    return model, report


def write_report(output_root, report: dict) -> Path:
    out = Path(output_root) / "label_prediction.json"
    with open(out, "w") as io:
        json.dump(report, io, indent=1)
        io.write("\n")
    return out
