"""Label prediction on the GPU: clane_probe_predict_* (csrc/label_predict.h) against float64 within the probe's a-priori
bound, exact on integer data, bit for bit consistent with the two fit kernels, reproducible, and the layers above it --
LabelProbe.train with cross-validation against a per-fit torch.optim.LBFGS on the CPU, Graph.fit_labels /
predict_labels and predict_rows on new vertices.  Every test prints its figures before it asserts: run with -s."""
import functools

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.classify import LabelProbe, fold_assignment
from clane_amd.embedder import Embedder
from clane_amd.graph import Graph
from clane_amd.similarity import CosineSimilarity

from . import label_predict_cases as L
from .conftest import GOLDEN, load_golden, write_data_root
from .test_gpu_classify import FIT_SEEDS, FIT_SHAPES, _objective, _planted, _ring_engine

pytestmark = pytest.mark.gpu

EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}      # unit roundoff of the accumulate type


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


def _run(k, dev, case, n, d, C, F, top, sigmoid, proba=True, fits=None):
    """The kernel on a case's operands (``fits``: only these fits of the stack) -> (classes, probs, proba) on the CPU."""
    Cp = case["Cp"]
    sel = list(range(F)) if fits is None else list(fits)
    W = case["W"].view(F, Cp, d)[sel].reshape(len(sel) * Cp, d).contiguous().to(dev)
    bias = case["bias"].view(F, Cp)[sel].reshape(-1).contiguous().to(dev)
    state = case["state"].view(F, Cp)[sel].reshape(-1).contiguous().to(dev)
    Z = case["table"].to(dev)[:, :d]                                    # leading dimension d + 3
    acc = case["acc"]
    cls = torch.full((n, len(sel), top), -7, dtype=torch.int32, device=dev)
    pr = torch.full((n, len(sel), top), float("nan"), dtype=acc, device=dev)
    full = torch.full((n, len(sel), C), float("nan"), dtype=acc, device=dev) if proba else None
    k.probe_predict(Z, d, case["rows"].to(dev), W, bias, len(sel), C, cls, pr, proba=full, sigmoid=sigmoid,
                    col_state=state if sigmoid else None)
    torch.cuda.synchronize()
    return cls.cpu(), pr.cpu(), None if full is None else full.cpu()


@pytest.mark.parametrize("shape", L.KERNEL_CASES, ids=str)
def test_against_float64(k, dev, shape):
    n, d, C, F, top, dtype, sigmoid, seed = shape
    case = L.kernel_case(*shape)
    cls, pr, full = _run(k, dev, case, n, d, C, F, top, sigmoid)
    logits, b, val, p64 = L.reference64(case, n, d, C, F, sigmoid)
    eps = EPS[case["acc"]]
    tol = 2.0 * b.amax(2, keepdim=True) + 8.0 * eps                     # the probe's: test_forward_against_float64
    err = (full.double() - p64).abs()
    named = cls.long().clamp(min=0)
    err_top = torch.where(cls >= 0, (pr.double() - torch.gather(p64, 2, named)).abs(), pr.double().abs())
    clear = L.clear_rows(val, b, top)
    left_out = int((~clear).sum())
    print(f"predict {shape}: max |proba - p64| / bound = {float((err / tol).max()):.3f}, top_prob "
          f"{float((err_top / tol).max()):.3f}; left out of the class comparison {left_out} of {n * F}")
    assert left_out <= 0.01 * n * F                                     # from the reference alone
    assert bool((err <= tol).all()) and bool((err_top <= tol).all())
    want = torch.stack([L.select_top(val[:, f], p64[:, f], top)[0] for f in range(F)], 1)
    assert torch.equal(cls[clear], want[clear])
    assert bool(((cls >= -1) & (cls < C)).all())
    if not sigmoid:                                                     # finite logits: min(top, C) classes, then the fill
        assert bool((cls[:, :, :min(top, C)] >= 0).all()) and bool((cls[:, :, C:] == -1).all())
        assert bool((pr[:, :, C:] == 0).all())


@pytest.mark.parametrize("shape", L.KERNEL_CASES, ids=str)
def test_integer_data_is_exact(k, dev, shape):
    n, d, C, F, top, dtype, sigmoid, seed = shape
    case = L.kernel_case(*shape, integer=True)
    cls, pr, full = _run(k, dev, case, n, d, C, F, top, sigmoid)
    logits, b, val, p64 = L.reference64(case, n, d, C, F, sigmoid)      # exact: small integers
    want = torch.stack([L.select_top(val[:, f], p64[:, f], top)[0] for f in range(F)], 1)
    ties = int((torch.sort(val, dim=2).values.diff(dim=2) == 0).any(2).sum())
    print(f"integer {shape}: rows x fits with tied values {ties} of {n * F}")
    assert torch.equal(cls, want)                                       # every row and fit, ties to the lowest class
    if n > 1 and not sigmoid:                                           # the zero row: every logit is the bias, so the
        bias = case["bias"].view(F, case["Cp"])[:, :C]                  # kernel's probabilities are the bias's soft-max
        assert torch.equal(logits[1], bias.double())
        tol = 2.0 * b[1].amax(1, keepdim=True) + 8.0 * EPS[case["acc"]]     # test_against_float64's
        assert bool(((full[1].double() - torch.softmax(bias.double(), 1)).abs() <= tol).all())
        assert torch.equal(cls[1], torch.stack([L.select_top(bias[f:f + 1], bias[f:f + 1], top)[0][0] for f in range(F)]))
    assert bool((pr[cls < 0] == 0).all())


def _probe_inputs(dev, n, F, C, g):
    y = torch.randint(0, C, (n,), generator=g).to(torch.int32).to(dev)
    return y, torch.ones(n, F, dtype=torch.uint8, device=dev)


@pytest.mark.parametrize("shape", [s for s in L.KERNEL_CASES if not s[6]], ids=str)
def test_consistent_with_the_softmax_fit_kernel(k, dev, shape):
    n, d, C, F, top, dtype, _, seed = shape
    case = L.kernel_case(*shape)
    cls, pr, full = _run(k, dev, case, n, d, C, F, top, False)
    Cp, acc = case["Cp"], case["acc"]
    y, split = _probe_inputs(dev, n, F, C, torch.Generator().manual_seed(5))
    G = torch.full((n * F * Cp,), float("nan"), dtype=acc, device=dev)
    loss = torch.zeros(F, dtype=torch.float64, device=dev)
    ws = torch.zeros(k.probe_loss_ws_len(n, F), dtype=torch.float64, device=dev)
    pred = torch.full((n, F), -7, dtype=torch.int32, device=dev)
    k.probe_forward(case["table"].to(dev)[:, :d], d, case["rows"].to(dev), y, split, case["W"].to(dev), case["bias"].to(dev),
                    F, C, ws, loss, G=G, pred=pred)
    torch.cuda.synchronize()
    onehot = torch.nn.functional.one_hot(y.long().cpu(), C).to(acc)[:, None, :]
    assert torch.equal(full - onehot, G.view(n, F, Cp)[:, :, :C].cpu())          # bit for bit
    assert torch.equal(cls[:, :, 0], pred.cpu())


@pytest.mark.parametrize("shape", [s for s in L.KERNEL_CASES if s[6]], ids=str)
def test_consistent_with_the_one_vs_rest_fit_kernel(k, dev, shape):
    n, d, C, F, top, dtype, _, seed = shape
    case = L.kernel_case(*shape)
    cls, pr, full = _run(k, dev, case, n, d, C, F, top, True)
    Cp, acc = case["Cp"], case["acc"]
    g = torch.Generator().manual_seed(6)
    bits = torch.rand(n, C, generator=g) < 0.3
    ymask = (bits.to(torch.int64) << torch.arange(C)).sum(1).to(dev)
    split = torch.ones(n, F, dtype=torch.uint8, device=dev)
    G = torch.full((n * F * Cp,), float("nan"), dtype=acc, device=dev)
    loss = torch.zeros(F, dtype=torch.float64, device=dev)
    ws = torch.zeros(k.probe_loss_ws_len(n, F), dtype=torch.float64, device=dev)
    k.probe_forward_ovr(case["table"].to(dev)[:, :d], d, case["rows"].to(dev), ymask, split, case["W"].to(dev),
                        case["bias"].to(dev), case["state"].to(dev), F, C, C, ws, loss, G=G)
    torch.cuda.synchronize()
    state = case["state"].view(F, Cp)[:, :C]
    live = (state == 0)[None].expand(n, F, C)
    Gc = G.view(n, F, Cp)[:, :, :C].cpu()
    assert torch.equal((full - bits.to(acc)[:, None, :])[live], Gc[live])        # bit for bit on the fitted columns
    assert bool((full[(state < 0)[None].expand(n, F, C)] == 0).all())
    assert bool((full[(state > 0)[None].expand(n, F, C)] == 1).all())


def test_reproducible_and_independent_of_the_other_fits(k, dev):
    for shape in (L.KERNEL_CASES[2], L.KERNEL_CASES[9]):                # F = 19: soft-max f32 (Cp = 8), sigmoid bf16
        n, d, C, F, top, dtype, sigmoid, seed = shape
        case = L.kernel_case(*shape)
        a = _run(k, dev, case, n, d, C, F, top, sigmoid)
        b = _run(k, dev, case, n, d, C, F, top, sigmoid)
        assert all(torch.equal(u, v) for u, v in zip(a, b))             # two calls: the same bits
        for f in (0, 7, 16, 18):                                        # 16: the first fit of the second column tile
            alone = _run(k, dev, case, n, d, C, F, top, sigmoid, fits=[f])
            assert all(torch.equal(u[:, f:f + 1], v) for u, v in zip(a, alone)), f
        lean = _run(k, dev, case, n, d, C, F, top, sigmoid, proba=False)
        assert torch.equal(lean[0], a[0]) and torch.equal(lean[1], a[1]) and lean[2] is None


# ---- the layers above -------------------------------------------------------------------------------------------------
CV_GRID, CV_FOLDS, CV_GTOL = [0.01, 1.0, 100.0], 3, 1e-4


@functools.lru_cache(maxsize=None)
def _cv_reference(shape):
    """Per l2: the mean held-out log-loss and the objective gap test_fit_float32_and_bfloat16_reach_the_minimum allows a
    float32 fit at ``CV_GTOL`` (its formula, from the reference's weights), averaged over the folds -- one
    torch.optim.LBFGS fit per (l2, fold) on the CPU in float64, the folds of ``fold_assignment``."""
    n, d, Cn, sep = shape
    X, y = _planted(n, d, Cn, sep, FIT_SEEDS[shape])
    fold = fold_assignment(n, CV_FOLDS, seed=0)
    eps = EPS[torch.float32]
    out = []
    for l2 in CV_GRID:
        losses, gaps = [], []
        for f in range(CV_FOLDS):
            train = fold != f
            Xt, yt = X[train], y[train]
            n_f = int(train.sum())
            W = torch.zeros(Cn, d, dtype=torch.float64, requires_grad=True)
            b = torch.zeros(Cn, dtype=torch.float64, requires_grad=True)
            opt = torch.optim.LBFGS([W, b], max_iter=2000, tolerance_grad=1e-10, tolerance_change=0, history_size=20,
                                    line_search_fn="strong_wolfe")

            def closure():
                opt.zero_grad()
                J = _objective(Xt, yt, W, b, l2)
                J.backward()
                return J
            opt.step(closure)
            with torch.no_grad():
                losses.append(float(torch.nn.functional.cross_entropy(X[~train] @ W.T + b, y[~train])))
                bmax = (2 * d * eps * (Xt.abs() @ W.abs().T + b.abs())).amax(1)
                logits = Xt @ W.T + b
                terms = torch.logsumexp(logits, 1) - logits[torch.arange(n_f), yt]
                forward_bound = float((2 * bmax).sum() + n * eps * terms.abs().sum()) / n_f
                gaps.append(CV_GTOL ** 2 * Cn * (d + 1) * n_f / (2 * l2) + forward_bound)
        out.append((sum(losses) / len(losses), sum(gaps) / len(gaps)))
    return X, y, out


@pytest.mark.parametrize("shape", FIT_SHAPES[:2], ids=str)
def test_train_with_cross_validation_against_a_per_fit_lbfgs(dev, shape):
    """float32, gtol and the allowed gap as in test_fit_float32_and_bfloat16_reach_the_minimum of tests/test_gpu_classify.py:
    J - J_ref <= gtol^2 C (d + 1) n_f / (2 l2) + the forward kernel's bound, here with the fit's own l2 and required of
    the mean held-out log-loss per l2 in both directions."""
    n, d, Cn, _ = shape
    X, y, ref = _cv_reference(shape)
    with torch.cuda.device(dev):
        eng = _ring_engine(X, torch.float32, dev)
        model = LabelProbe(eng, gtol=CV_GTOL).train(list(range(n)), y, Cn, l2=CV_GRID, folds=CV_FOLDS, seed=0)
    got = [r["log_loss"] for r in model.cv["rows"]]
    for l2, a, (b, gap) in zip(CV_GRID, got, ref):
        print(f"cv {shape} l2 = {l2}: held-out log-loss {a:.9f}, reference {b:.9f}, |difference| / allowed "
              f"{abs(a - b) / gap:.3f}")
    best = min(range(len(CV_GRID)), key=lambda i: (ref[i][0], -CV_GRID[i]))
    assert model.l2 == CV_GRID[best] == model.cv["l2"]
    assert all(abs(a - b) <= gap for a, (b, gap) in zip(got, ref))
    assert model.converged and all(r["fits_used"] == CV_FOLDS and 0.0 <= r["ece"] <= 1.0 for r in model.cv["rows"])
    assert model.W.dtype == np.float32 and model.W.shape == (Cn, d) and model.n_train == n


def _karate_graph(tmp_path):
    kar = load_golden("g2_karate_csr.npz")
    X = np.random.default_rng(0).standard_normal((34, 4)).astype(np.float32)
    root = write_data_root(tmp_path / "karate", kar["vertex_ids"], kar["edge_src"], kar["edge_dst"], X)
    lines = (GOLDEN / "g2_karate_Y.tsv").read_text().splitlines()
    (root / "Y").write_text("\n".join(lines[::2]) + "\n")
    return Graph(root, embedding_dim=4), root, len(lines[::2])


def test_graph_fit_predict_and_new_vertices(dev, tmp_path):
    g, root, labelled = _karate_graph(tmp_path)
    Embedder(g, CosineSimilarity(), dev, tolerence=3, verbose=False).iterate()
    model = g.fit_labels(root / "Y", l2=[0.1, 1.0, 10.0], folds=3, seed=1)
    assert model.n_train == labelled and model.d == 4 and model.converged and model.l2 in (0.1, 1.0, 10.0)
    v, classes, probs, proba = g.predict_labels(model, top=3, proba=True)
    C = len(model.class_names)
    assert v.tolist() == list(range(34)) and classes.shape == probs.shape == (34, 3) and proba.shape == (34, C)
    assert bool((probs[:, :-1] >= probs[:, 1:]).all()) and np.allclose(proba.sum(1), 1.0, atol=1e-5)
    assert bool((classes[:, :min(3, C)] >= 0).all()) and bool((classes[:, C:] == -1).all())
    rows = np.arange(34)
    assert np.array_equal(proba[rows, classes[:, 0]], probs[:, 0]) and np.array_equal(proba.argmax(1), classes[:, 0])
    # predict_rows on a gathered copy of the rows equals predict_table on the table
    eng = g.engine()
    some = [33, 0, 7, 7, 12]
    a = model.predict_table(eng, some, top=2, proba=True)
    b = model.predict_rows(eng, eng.get_Z()[some].to(eng.Zcur.dtype).to(eng.device).contiguous(), top=2, proba=True)
    assert all(np.array_equal(u, w) for u, w in zip(a, b))
    # arrivals: embed them, then the same model on their rows
    Xn = np.random.default_rng(1).standard_normal((3, 4)).astype(np.float32)
    res = g.embed_new(CosineSimilarity(), Xn, [[3, 9], [0], []], gamma=0.76, tolerence=3)
    cn, pn = model.predict_rows(eng, res.Z.to(eng.device, eng.Zcur.dtype).contiguous(), top=1)
    assert cn.shape == (3, 1) and bool((cn >= 0).all()) and bool(((pn > 0) & (pn <= 1)).all())
    Z_all = torch.cat([eng.get_Z().cpu().double(), res.Z.double()])
    want = (Z_all[34:] @ torch.from_numpy(model.W).double().T + torch.from_numpy(model.b).double()).softmax(1)
    assert np.allclose(pn[:, 0], want.amax(1).numpy(), atol=1e-5)
    with pytest.raises(ValueError, match="top must be in 1..8"):
        g.predict_labels(model, top=9)
