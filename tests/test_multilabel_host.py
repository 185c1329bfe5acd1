"""Multi-label node classification, the parts that need no GPU: the label file, class sets as masks, the constant-column
rule, (tp, fp, fn) counts and F1 from hand-worked tables, probe_forward_ovr of csrc/multilabel_probe.h restated in torch,
and the host logic driven by it -- the one-vs-rest fit against a per-class torch.optim.LBFGS, constant columns, skipped
fits, grouping, top-k prediction, the refusals, the ABI's argument checks and the CLI section's validation.  Every fit
test prints its figures before it asserts: run with -s to see them."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.classify import (LabelProbe, column_states, f1_from_counts, label_masks, make_splits, mask_bits,
                                multilabel_counts, read_labels)
from clane_amd.engine import SweepEngine
from clane_amd.partition import HostCSR

from .oracle_kernels import OracleKernels
from .test_classify_host import ProbeOracleKernels

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = [f"clane_probe_forward_ovr_{s}" for s in ("f32", "f64", "bf16")]


class MultilabelOracleKernels(ProbeOracleKernels):
    """probe_forward_ovr of csrc/multilabel_probe.h in torch (the same formulas, no attempt at the same rounding), on top
    of the probe_forward / probe_grad restatements of the classify host test (an OracleKernels subclass)."""

    def probe_forward_ovr(self, Z, d, rows, ymask, split, W, bias, col_state, F, C_, max_labels, loss_ws, loss, G=None,
                          pred=None, top_k=True):
        n, Cp = rows.numel(), _hip.ovr_padded_classes(C_)
        assert 0 <= max_labels <= C_
        Zg = self._gathered(Z, d, rows, W.dtype)
        y = mask_bits(ymask, C_)
        want = y.sum(1)
        assert n == 0 or int(want.max()) <= max_labels
        for f in range(F):                                  # fit by fit: a fit gets the same bits whatever shares the call
            logits = Zg @ W[f * Cp:f * Cp + C_].T + bias[f * Cp:f * Cp + C_]
            state = col_state[f * Cp:f * Cp + C_]
            live = (split[:, f] != 0)[:, None] & (state == 0)[None, :]
            yf = y.to(logits.dtype)
            term = torch.nn.functional.softplus(logits) - yf * logits
            loss[f] = (term * live).double().sum()
            if G is not None:
                Gm = G[:n * F * Cp].view(n, F * Cp)
                Gm[:, f * Cp:(f + 1) * Cp] = 0.0
                Gm[:, f * Cp:f * Cp + C_] = (torch.sigmoid(logits) - yf) * live
            if pred is not None:
                inf = torch.full_like(logits, float("inf"))
                val = torch.where(state[None, :] == 0, logits, torch.where(state[None, :] < 0, -inf, inf))
                if top_k:
                    order = torch.sort(val.nan_to_num(nan=float("-inf")), dim=1, descending=True, stable=True).indices
                    rank = torch.empty_like(order)
                    rank.scatter_(1, order, torch.arange(C_).expand(n, C_).contiguous())
                    sel = (rank < want[:, None]) & (val > float("-inf"))
                else:
                    sel = val > 0
                pred[:, f] = (sel.to(torch.int64) << torch.arange(C_)).sum(1)


def _engine(X, kernels=None):
    V = X.shape[0]
    csr = HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + 1) % V).astype(np.int32))
    eng = SweepEngine(csr, X, "cpu", kernels or MultilabelOracleKernels())
    eng.set_Z(X)
    return eng


def _planted(n, d, Cn, sep, seed):
    """Rows with 1-3 classes (skewed frequencies), each the sum of its classes' directions times sep plus noise."""
    rng = np.random.default_rng(seed)
    freq = 1.0 / (1.0 + np.arange(Cn)) ** 1.5
    freq /= freq.sum()
    dirs = rng.standard_normal((Cn, d))
    Y = np.zeros((n, Cn))
    for i in range(n):
        Y[i, rng.choice(Cn, size=min(Cn, int(rng.integers(1, 4))), replace=False, p=freq)] = 1.0
    X = Y @ dirs * sep + rng.standard_normal((n, d))
    masks = label_masks([np.flatnonzero(r).tolist() for r in Y], Cn)
    return torch.from_numpy(X), masks, torch.from_numpy(Y)


# ---- the label file ---------------------------------------------------------------------------------------------
def test_read_labels_multilabel(tmp_path):
    vertex_ids = ["a", "b", "c", "a", "d"]
    (tmp_path / "Y").write_text("c\tzebra\n\nb\tant\nc\tant\r\nd\tzebra\nb\tmole\n")
    v, masks, names = read_labels(tmp_path / "Y", vertex_ids, multilabel=True)
    assert names == ["ant", "mole", "zebra"]                     # sorted order
    assert v == [2, 1, 4]                                        # first appearance
    assert masks == [0b101, 0b011, 0b100]
    with pytest.raises(ValueError, match=r"line 4: 'c' was labelled on line 1"):      # the default is single-label
        read_labels(tmp_path / "Y", vertex_ids)
    (tmp_path / "pair").write_text("c\tx\nb\ty\n\nc\ty\nc\tx\n")
    with pytest.raises(ValueError, match=r"line 5: 'c' was given class 'x' on line 1"):
        read_labels(tmp_path / "pair", vertex_ids, multilabel=True)
    (tmp_path / "unknown").write_text("c\tx\nzz\ty\n")
    with pytest.raises(ValueError, match=r"line 2: 'zz'"):
        read_labels(tmp_path / "unknown", vertex_ids, multilabel=True)
    (tmp_path / "many").write_text("".join(f"a\tk{i}\n" for i in range(65)))
    with pytest.raises(ValueError, match="65 classes"):
        read_labels(tmp_path / "many", vertex_ids, multilabel=True)
    (tmp_path / "full").write_text("".join(f"a\tk{i:02d}\n" for i in range(64)))
    v, masks, names = read_labels(tmp_path / "full", vertex_ids, multilabel=True)
    assert v == [0] and masks == [(1 << 64) - 1] and len(names) == 64


def test_label_masks_forms():
    m = label_masks([{0, 2}, [], (1,), 5], 3)
    assert m.dtype == torch.int64 and m.tolist() == [5, 0, 2, 5]
    assert torch.equal(label_masks(m, 3), m)
    top = label_masks([[63], list(range(64))], 64)
    assert top.tolist() == [-(1 << 63), -1]                      # the uint64 pattern in an int64
    assert mask_bits(top, 64).sum(1).tolist() == [1, 64] and bool(mask_bits(top, 64)[0, 63])
    for bad, C_, text in (([[3]], 3, "class 3"), ([8], 3, "at or above"), ([[0]], 65, "C > 64"), ([[0]], 0, "classes")):
        with pytest.raises(ValueError, match=text):
            label_masks(bad, C_)


def test_column_states_on_a_hand_made_split():
    #                 classes      fit 0  fit 1  fit 2
    masks = label_masks([[0, 1],    # 1     1      0
                         [0],       # 1     0      0
                         [0, 2],    # 1     1      0
                         [1],       # 0     1      0
                         [2]], 4)   # 0     0      0
    split = torch.tensor([[1, 1, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 0]], dtype=torch.uint8)
    s = column_states(masks, split, 4)
    assert s.dtype == torch.int8 and s.tolist() == [[1, 0, 0, -1],      # class 0 on every training row, 3 on none
                                                    [0, 0, 0, -1],
                                                    [-1, -1, -1, -1]]   # nothing trains fit 2


# ---- metrics ----------------------------------------------------------------------------------------------------
def test_counts_and_f1_of_a_hand_worked_table():
    # 5 rows, 4 classes; class 3 is in no truth and no prediction
    truth = [[0, 1], [0], [1, 2], [2], [0, 2]]
    pred0 = [[0, 1], [1], [1], [0, 2], [0, 2]]
    pred1 = [[], [0], [2, 1], [2], [1]]
    masks = label_masks(truth, 4)
    pred = torch.stack([label_masks(pred0, 4), label_masks(pred1, 4)], 1)
    test = torch.tensor([[1, 1], [1, 1], [1, 0], [1, 1], [1, 1]], dtype=torch.bool)
    counts = multilabel_counts(masks, pred, test, 4)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (2, 4, 3)
    # fit 0, per class (tp, fp, fn): class 0: truth rows 0 1 4, predicted rows 0 3 4
    assert counts[0].tolist() == [[2, 1, 1], [2, 1, 0], [2, 0, 1], [0, 0, 0]]
    # fit 1 without row 2: class 0: truth 0 1 4, predicted 1; class 1: truth 0, predicted 4; class 2: truth 3 4, predicted 3
    assert counts[1].tolist() == [[1, 0, 2], [0, 1, 1], [1, 0, 1], [0, 0, 0]]
    micro, macro = f1_from_counts(counts)                               # a leading fit dimension
    assert float(micro[0]) == pytest.approx(2 * 6 / (2 * 6 + 2 + 2), abs=1e-15)
    assert float(macro[0]) == pytest.approx((4 / 6 + 4 / 5 + 4 / 5 + 0.0) / 4, abs=1e-15)     # the empty class counts 0
    assert float(micro[1]) == pytest.approx(2 * 2 / (2 * 2 + 1 + 4), abs=1e-15)
    assert float(macro[1]) == pytest.approx((2 / 4 + 0.0 + 2 / 3 + 0.0) / 4, abs=1e-15)
    one_micro, one_macro = f1_from_counts(counts[1])                    # and without one
    assert float(one_micro) == float(micro[1]) and float(one_macro) == float(macro[1])
    empty = torch.zeros(3, 3, dtype=torch.int64)                        # all classes empty
    assert [float(v) for v in f1_from_counts(empty)] == [0.0, 0.0]


def test_f1_against_scikit_learn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(0)
    for case in range(30):
        n, Cn = int(rng.integers(1, 80)), int(rng.integers(2, 9))       # one column would be read as a binary target
        Y, P = rng.random((n, Cn)) < 0.3, rng.random((n, Cn)) < 0.3
        masks = label_masks([np.flatnonzero(r).tolist() for r in Y], Cn)
        pred = label_masks([np.flatnonzero(r).tolist() for r in P], Cn)[:, None]
        counts = multilabel_counts(masks, pred, torch.ones(n, 1, dtype=torch.bool), Cn)
        micro, macro = f1_from_counts(counts)
        assert float(micro[0]) == pytest.approx(metrics.f1_score(Y, P, average="micro", zero_division=0), abs=1e-12), case
        assert float(macro[0]) == pytest.approx(metrics.f1_score(Y, P, average="macro", zero_division=0), abs=1e-12), case


# ---- the fit ----------------------------------------------------------------------------------------------------
def _reference_column(X, y, train, l2):
    """One binary logistic regression by torch.optim.LBFGS(strong_wolfe) in float64: (w, b, the summed loss + penalty)."""
    Xt, yt = X[train], y[train]
    w = torch.zeros(X.shape[1], dtype=torch.float64, requires_grad=True)
    b = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.LBFGS([w, b], max_iter=2000, tolerance_grad=1e-11, tolerance_change=0, history_size=20,
                            line_search_fn="strong_wolfe")

    def objective():
        bce = torch.nn.functional.binary_cross_entropy_with_logits(Xt @ w + b, yt, reduction="sum")
        return (bce + 0.5 * l2 * (w * w).sum()) / Xt.shape[0]

    def closure():
        opt.zero_grad()
        J = objective()
        J.backward()
        return J
    opt.step(closure)
    return w.detach(), b.detach(), float(objective().detach())


@pytest.mark.parametrize("shape", [(300, 5, 3), (600, 16, 7)], ids=str)
def test_fit_is_separable_and_matches_a_per_class_lbfgs(shape):
    n, d, Cn = shape
    X, masks, Y = _planted(n, d, Cn, 1.0, seed=n)
    eng = _engine(X)
    rows = eng.pos[torch.arange(n)].to(torch.int32)
    split, _ = make_splits(n, (0.1, 0.5, 0.9), 2, seed=3)
    F = split.shape[1]
    probe = LabelProbe(eng, l2=1.0, gtol=1e-8)
    fit = probe.fit_multilabel(eng.Zcur, rows, masks, split, Cn)
    states = column_states(masks, split, Cn)
    print(f"fit {shape}: iterations {fit.iterations.tolist()} constant {fit.constant.tolist()} passes {probe.passes}")
    assert bool(fit.converged.all()) and not bool(fit.skipped.any())
    assert fit.pred.dtype == torch.int64 and tuple(fit.pred.shape) == (n, F) and tuple(fit.W.shape) == (F, Cn, d)
    assert torch.equal(fit.constant, (states != 0).sum(1))
    # separable: J_f = the sum of the C single-column problems' objectives
    single = torch.zeros(F, dtype=torch.float64)
    for c in range(Cn):
        one = probe.fit_multilabel(eng.Zcur, rows, (masks >> c) & 1, split, 1)
        assert torch.equal(one.skipped, states[:, c] != 0)
        single += torch.where(one.skipped, torch.zeros_like(one.objective), one.objective)
    gap = (fit.objective - single).abs() / fit.objective
    print(f"  max |J - sum of single-column J| / J = {float(gap.max()):.2e}")
    assert float(gap.max()) <= 1e-9
    for f in range(F):
        train = split[:, f].bool()
        J, logits = 0.0, torch.zeros(n, Cn, dtype=torch.float64)
        for c in range(Cn):
            if int(states[f, c]) != 0:
                assert float(fit.W[f, c].abs().max()) == 0.0 and float(fit.b[f, c]) == 0.0
                logits[:, c] = float("inf") * int(states[f, c])
                continue
            w, b, Jc = _reference_column(X, Y[:, c], train, 1.0)
            J += Jc
            logits[:, c] = X @ w + b
            assert float((fit.W[f, c] - w).abs().max()) < 1e-4 and abs(float(fit.b[f, c] - b)) < 1e-4
        assert abs(float(fit.objective[f]) - J) <= 1e-9 * J
        # top-k of the reference's logits where the k-th and (k + 1)-th are clearly apart
        k_i = Y.sum(1).long()
        ranked = logits.sort(1, descending=True)
        kth = ranked.values.gather(1, (k_i - 1).clamp(min=0)[:, None])[:, 0]
        nxt = ranked.values.gather(1, k_i.clamp(max=Cn - 1)[:, None])[:, 0]
        clear = (k_i == Cn) | ((kth - nxt) >= 1e-2) | (kth == nxt)
        clear &= ~((kth == nxt) & (k_i < Cn) & torch.isfinite(kth))
        want = (torch.arange(Cn)[None, :] < k_i[:, None])
        sel = torch.zeros(n, Cn, dtype=torch.bool).scatter_(1, ranked.indices, want) & (logits > float("-inf"))
        expected = (sel.to(torch.int64) << torch.arange(Cn)).sum(1)
        assert int(clear.sum()) >= 0.95 * n
        assert torch.equal(fit.pred[clear, f], expected[clear])


def _constant_case():
    n, d = 40, 4
    X = torch.from_numpy(np.random.default_rng(5).standard_normal((n, d)))
    sets = [[0] if i % 2 else [0, 1] for i in range(n)]                 # class 0 everywhere, class 1 on even rows
    for i in range(30, 40):
        sets[i] = [1, 2] if i % 2 else [2]                              # class 2 only on the last ten rows
    split = torch.zeros(n, 3, dtype=torch.uint8)
    split[:20, 0] = 1               # fit 0: class 0 on every training row, class 2 on none, class 1 fitted
    split[10:, 1] = 1               # fit 1: everything fitted
    split[1:20:2, 2] = 1            # fit 2: odd rows among the first twenty: {0} alone -- no fitted column
    return X, label_masks(sets, 3), split


def test_constant_columns_are_counted_carry_no_weights_and_are_predicted_never_or_always():
    X, masks, split = _constant_case()
    eng = _engine(X)
    rows = eng.pos[torch.arange(40)].to(torch.int32)
    for predict in ("top_k", "threshold"):
        fit = LabelProbe(eng, gtol=1e-8).fit_multilabel(eng.Zcur, rows, masks, split, 3, predict=predict)
        assert fit.constant.tolist() == [2, 0, 3] and fit.skipped.tolist() == [False, False, True]
        assert fit.converged.tolist() == [True, True, False] and fit.iterations.tolist()[2] == 0
        assert float(fit.W[0, 0].abs().max()) == 0.0 and float(fit.W[0, 2].abs().max()) == 0.0
        assert float(fit.b[0, [0, 2]].abs().max()) == 0.0 and float(fit.W[0, 1].abs().max()) > 0.0
        assert float(fit.W[2].abs().max()) == 0.0 and float(fit.objective[2]) == 0.0
        bits = mask_bits(fit.pred, 3)                                   # [n, F, C]
        assert not bool(bits[:, 0, 2].any())                            # never, although rows 30.. have class 2
        if predict == "threshold":
            assert bool(bits[:, 0, 0].all()) and bool(bits[:, 2, 0].all()) and not bool(bits[:, 2, 1:].any())
        else:
            assert bool(bits[:, 0, 0].all())                            # every row has k >= 1: the +inf column first
            k_i = mask_bits(masks, 3).sum(1)
            assert bool((bits[:, 0].sum(1) <= k_i).all()) and bool((bits[:, 1].sum(1) == k_i).all())
            assert torch.equal(bits[:, 2].sum(1), torch.ones(40, dtype=torch.int64))      # one +inf column, two -inf
    out = LabelProbe(eng).evaluate(list(range(40)), [[0] if i % 2 else [0, 1] for i in range(40)], 2, ratios=(0.5,),
                                   runs=2, seed=0, multilabel=True)
    assert out["multilabel"] is True and out["predict"] == "top_k" and out["constant_columns"] == 2      # class 0, twice
    assert out["fits"]["constant_columns"] == [1, 1] and out["skipped_fits"] == 0 and out["rows"][0]["runs_used"] == 2


def test_grouping_by_a_small_budget_changes_no_result():
    n, d, Cn = 120, 6, 5
    X, masks, _ = _planted(n, d, Cn, 1.0, seed=1)
    eng = _engine(X)
    rows = eng.pos[torch.arange(n)].to(torch.int32)
    split, _ = make_splits(n, (0.2, 0.5, 0.8), 2, seed=5)
    probe = LabelProbe(eng, gtol=1e-8)
    fit = probe.fit_multilabel(eng.Zcur, rows, masks, split, Cn)
    one_pass = dict(probe.passes)
    small = LabelProbe(eng, gtol=1e-8, g_budget_bytes=n * 8 * 8)        # one fit's G at a time
    assert len(small.groups(n, 6, 8, torch.float64)) == 6
    again = small.fit_multilabel(eng.Zcur, rows, masks, split, Cn)
    for name in ("W", "b", "objective", "iterations", "pred", "grad_max", "constant", "skipped"):
        assert torch.equal(getattr(fit, name), getattr(again, name)), name
    assert small.passes["forward"] > one_pass["forward"]


def test_one_label_per_row_top_k_is_the_arg_max_lowest_class_on_ties():
    n, d, Cn = 90, 4, 4
    rng = np.random.default_rng(2)
    y = torch.from_numpy(rng.integers(0, Cn, n))
    X = torch.from_numpy(rng.standard_normal((Cn, d)))[y] + torch.from_numpy(rng.standard_normal((n, d)))
    eng = _engine(X)
    rows = eng.pos[torch.arange(n)].to(torch.int32)
    split, _ = make_splits(n, (0.5,), 2, seed=0)
    masks = label_masks([[int(c)] for c in y], Cn)
    fit = LabelProbe(eng, gtol=1e-8).fit_multilabel(eng.Zcur, rows, masks, split, Cn)
    for f in range(2):
        logits = X @ fit.W[f].T + fit.b[f]
        assert torch.equal(fit.pred[:, f], torch.ones(n, dtype=torch.int64) << logits.argmax(1))
    # no step: every weight 0, every logit 0 -- all classes tie, the lowest wins
    tied = LabelProbe(eng, max_iter=0).fit_multilabel(eng.Zcur, rows, masks, split, Cn)
    assert float(tied.W.abs().max()) == 0.0 and bool((tied.pred == 1).all())


def test_single_label_fit_is_what_a_direct_call_sequence_gives():
    """The soft-max fit after its L-BFGS loop became a driver shared with fit_multilabel: the kernel calls it makes and
    the objective it reports are those of the calls made by hand."""
    n, d, Cn = 60, 5, 3
    rng = np.random.default_rng(4)
    y = torch.from_numpy(rng.integers(0, Cn, n))
    X = torch.from_numpy(rng.standard_normal((Cn, d)))[y] + torch.from_numpy(rng.standard_normal((n, d)))
    eng = _engine(X)
    k = eng.k
    rows = eng.pos[torch.arange(n)].to(torch.int32)
    split, _ = make_splits(n, (0.3, 0.7), 2, seed=1)
    F, Cp = 4, 4
    n_f = split.sum(0).double()
    start = LabelProbe(eng, max_iter=0)
    fit0 = start.fit(eng.Zcur, rows, y, split, Cn)
    assert start.passes == {"forward": 2, "grad": 1}                    # loss and gradient at 0, then the predictions
    assert float((fit0.objective - np.log(Cn)).abs().max()) < 1e-12 and bool((fit0.pred == 0).all())
    probe = LabelProbe(eng, l2=0.5, gtol=1e-8)
    fit = probe.fit(eng.Zcur, rows, y, split, Cn)
    assert bool(fit.converged.all()) and probe.passes["forward"] > probe.passes["grad"] >= int(fit.iterations.max()) + 1
    W = torch.zeros(F * Cp, d, dtype=torch.float64)
    b = torch.zeros(F * Cp, dtype=torch.float64)
    W.view(F, Cp, d)[:, :Cn], b.view(F, Cp)[:, :Cn] = fit.W, fit.b
    loss, G = torch.zeros(F, dtype=torch.float64), torch.zeros(n * F * Cp, dtype=torch.float64)
    pred = torch.zeros(n, F, dtype=torch.int32)
    k.probe_forward(eng.Zcur, d, rows, y.to(torch.int32), split, W, b, F, Cn, torch.zeros(1, dtype=torch.float64), loss,
                    G=G, pred=pred)
    dW, db = torch.zeros(F * Cp * d, dtype=torch.float64), torch.zeros(F * Cp, dtype=torch.float64)
    k.probe_grad(eng.Zcur, d, rows, G, torch.zeros(1, dtype=torch.float64), dW, db)
    J = (loss + 0.5 * 0.5 * (W * W).view(F, -1).sum(1)) / n_f
    g = torch.cat([(dW.view(F, Cp * d) + 0.5 * W.view(F, -1)), db.view(F, Cp)], 1) / n_f[:, None]
    assert torch.equal(J, fit.objective) and torch.equal(g.abs().amax(1), fit.grad_max) and torch.equal(pred, fit.pred)
    assert fit.constant is None


# ---- refusals ---------------------------------------------------------------------------------------------------
def test_refusals():
    X, masks, split = _constant_case()
    eng = _engine(X)
    rows = eng.pos[torch.arange(40)].to(torch.int32)
    probe = LabelProbe(eng)
    with pytest.raises(ValueError, match="C > 64"):
        probe.fit_multilabel(eng.Zcur, rows, masks, split, 65)
    with pytest.raises(ValueError, match="'top_k' or 'threshold'"):
        probe.fit_multilabel(eng.Zcur, rows, masks, split, 3, predict="best")
    with pytest.raises(ValueError, match="at or above C = 2"):
        probe.fit_multilabel(eng.Zcur, rows, masks, split, 2)
    with pytest.raises(ValueError, match="int64"):
        probe.fit_multilabel(eng.Zcur, rows, masks.to(torch.int32), split, 3)
    with pytest.raises(ValueError, match="multilabel needs n_classes"):
        probe.evaluate(list(range(40)), [[0]] * 40, multilabel=True)
    with pytest.raises(ValueError, match="classes"):
        _hip.ovr_padded_classes(65)
    assert [_hip.ovr_padded_classes(c) for c in (1, 2, 3, 17, 64)] == [1, 2, 4, 32, 64]
    # a backend without the kernel says so: no fall-back
    with pytest.raises(NotImplementedError, match="OracleKernels has no probe_forward_ovr"):
        OracleKernels().probe_forward_ovr(None, 1, None, None, None, None, None, None, 1, 2, 1, None, None)
    plain = _engine(X, ProbeOracleKernels())
    with pytest.raises(NotImplementedError, match="ProbeOracleKernels has no probe_forward_ovr"):
        LabelProbe(plain).fit_multilabel(plain.Zcur, rows, masks, split, 3)
    eng.world = 2                                                       # several ranks
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        LabelProbe(eng)
    eng.world, eng.columns = 1, True                                    # a column division
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        LabelProbe(eng)


# ---- the ABI ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    text = (ROOT / "include" / "clane_hip.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", header)
        assert decl and name in _hip.SIGNATURES, name
        assert len(_hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == 22, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define CLANE_ABI_VERSION 5\b", header) and lib.clane_abi_version() == 5
    assert "clane_probe_forward_ovr_*" in text.split("#define CLANE_OK")[0]      # the version comment lists the addition
    assert re.search(r"#define CLANE_PROBE_PRED_TOPK 4\b", header) and _hip.PROBE_PRED_TOPK == 4
    assert callable(_hip.HipKernels.probe_forward_ovr)


def test_argument_validation_reaches_last_error():
    lib = _hip.load_library()                   # refused on the host before any launch: safe without a GPU
    p = C.cast((C.c_float * 64)(), C.c_void_p)

    def fwd(fn=lib.clane_probe_forward_ovr_f32, d=4, ldz=4, n=2, ld_split=3, F=3, Cn=3, max_labels=3, flags=0, G=None,
            ws=p, loss=p, pred=None, ld_pred=3, Z=p, state=p, ymask=p):
        return fn(Z, 8, d, ldz, p, ymask, n, p, ld_split, p, p, state, F, Cn, max_labels, flags, G, ws, loss, pred, ld_pred,
                  None)

    for bad, text in ((dict(d=0), b"bad shape"), (dict(ldz=3), b"bad shape"), (dict(n=-1), b"bad shape"),
                      (dict(Cn=0, max_labels=0), b"C must be"), (dict(Cn=65), b"C must be"),
                      (dict(max_labels=4), b"max_labels"), (dict(max_labels=-1), b"max_labels"),
                      (dict(F=0), b"number of fits"), (dict(ld_split=2), b"ld_split"), (dict(flags=8), b"unknown flags"),
                      (dict(flags=1), b"needs G"), (dict(flags=2), b"needs pred"), (dict(flags=6), b"needs pred"),
                      (dict(flags=2, pred=p, ld_pred=2), b"ld_pred"), (dict(ws=None), b"null loss"),
                      (dict(Z=None), b"null pointer"), (dict(state=None), b"null pointer"),
                      (dict(ymask=None), b"null pointer")):
        assert fwd(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"probe_forward_ovr" in lib.clane_last_error()
    assert fwd(fn=lib.clane_probe_forward_ovr_bf16, Cn=70) == -1 and fwd(fn=lib.clane_probe_forward_ovr_f64, d=-1) == -1


# ---- the CLI section --------------------------------------------------------------------------------------------
CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


@pytest.mark.parametrize("section, text", [("  multilabel: true\n  predict: best\n", "predict must be"),
                                           ("  multilabel: 1\n", "multilabel must be true or false"),
                                           ("  multilabel: \"yes\"\n", "multilabel must be true or false"),
                                           ("  predict: threshold\n", "belongs to multilabel")])
def test_cli_section_is_validated_before_the_graph_is_loaded(monkeypatch, tmp_path, section, text):
    import clane_amd.__main__ as M

    def touched(*a, **k):
        raise AssertionError("the run went on to load the graph")
    monkeypatch.setattr(M, "_distributed_setup", touched)
    monkeypatch.setattr(M, "Graph", touched)
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG + "\nnode_classification:\n  labels: Y\n" + section)
    args = M.get_parser().parse_args(["--data_root", str(tmp_path), "--output_root", str(tmp_path / "o"),
                                      "--config_file", str(cfg)])
    with pytest.raises(ValueError, match=text):
        M.embedding(args)
