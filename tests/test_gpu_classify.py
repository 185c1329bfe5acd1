"""Node classification on the GPU: clane_probe_forward_* / clane_probe_grad_* (csrc/label_probe.h) against float64 within
a-priori bounds, bit-reproducibility, exactness on integer data, the batched L-BFGS of classify.LabelProbe against a per-fit
torch.optim.LBFGS on the CPU, and the surface (Graph.evaluate_labels).  Every test prints its figures (error / bound,
L-BFGS steps, J - J_ref) before it asserts: run with -s to see them."""
import functools

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.classify import LabelProbe, confusion_counts, f1_from_confusion, make_splits
from clane_amd.embedder import Embedder
from clane_amd.engine import SweepEngine
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR
from clane_amd.similarity import CosineSimilarity

pytestmark = pytest.mark.gpu

EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}      # unit roundoff of the accumulate type
DTYPES = [torch.float32, torch.bfloat16, torch.float64]
# every d, C, F and n of the issue's lists at least once; (129, 16, 7, 19) and (129, 256, 16, 19): K = 152 / 304 cross
# the 128-column tile
FORWARD_SHAPES = [(1, 1, 2, 1), (127, 5, 3, 3), (129, 16, 7, 19), (5000, 130, 17, 3), (5000, 256, 64, 3),
                  (129, 256, 16, 19), (127, 130, 2, 19), (5000, 16, 7, 1)]
GRAD_SHAPES = [(1, 8, 1), (2047, 152, 5), (2049, 8, 16), (10000, 152, 130), (2049, 152, 256), (10000, 8, 256)]
FIT_SHAPES = [(600, 16, 7, 0.6), (300, 5, 3, 0.8), (1000, 130, 17, 0.25)]
FIT_RATIOS = (0.1, 0.5, 0.9)
# The prediction check leaves out the test rows whose REFERENCE top-two margin is below 1e-2 and requires them to be at
# most 1 % of a fit's test rows -- a property of the data and of the float64 CPU reference alone.  With 30 test rows
# that means none, so the planted data's seed is picked per shape, from the reference's margins only, such that the
# condition holds (left out per fit: 1 / 540, 1 / 300, 0 / 60; 2 / 270, 0 / 150, 0 / 30; 8 / 900, 4 / 500, 0 / 100).
FIT_SEEDS = {FIT_SHAPES[0]: 0, FIT_SHAPES[1]: 2, FIT_SHAPES[2]: 8}


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


def _padded(values, dtype, dev, pad=3):
    buf = torch.zeros(values.shape[0], values.shape[1] + pad, dtype=dtype, device=dev)
    buf[:, :values.shape[1]] = values.to(dtype).to(dev)
    return buf[:, :values.shape[1]]                     # leading dimension d + pad


def _forward_case(n, d, Cn, F, dtype, dev, integers=False):
    gen = torch.Generator().manual_seed(1000 * n + 10 * d + Cn + F)
    acc = _hip.acc_dtype(dtype)
    Cp = _hip.probe_padded_classes(Cn)
    table_rows = max(3, n // 2)                         # rows repeat
    if integers:
        Zv = torch.randint(-2, 3, (table_rows, d), generator=gen).double()
        W = torch.randint(-1, 2, (F * Cp, d), generator=gen).double()
        bias = torch.randint(-1, 2, (F * Cp,), generator=gen).double()
    else:
        Zv = torch.randn(table_rows, d, generator=gen, dtype=torch.float64)
        W = torch.randn(F * Cp, d, generator=gen, dtype=torch.float64) / max(1.0, d ** 0.5) * 2.0
        bias = torch.randn(F * Cp, generator=gen, dtype=torch.float64)
    Z = _padded(Zv, dtype, dev)
    rows = torch.randint(0, table_rows, (n,), generator=gen).to(torch.int32)
    rows[n // 2] = table_rows                           # one index past the table: a zero row
    y = torch.randint(0, Cn, (n,), generator=gen).to(torch.int32)
    split = (torch.rand(n, F + 2, generator=gen) < 0.5).to(torch.uint8)
    if F > 1:
        split[:, F - 1] = 0                             # a fit that nothing trains
    return dict(Z=Z, rows=rows.to(dev), y=y.to(dev), split=split.to(dev)[:, :F], W=W.to(acc).to(dev),
                bias=bias.to(acc).to(dev), n=n, d=d, C=Cn, Cp=Cp, F=F, acc=acc, table_rows=table_rows)


def _run_forward(k, c, dev):
    n, F, Cp = c["n"], c["F"], c["Cp"]
    G = torch.full((n * F * Cp,), float("nan"), dtype=c["acc"], device=dev)
    loss = torch.full((F,), float("nan"), dtype=torch.float64, device=dev)
    ws = torch.zeros(k.probe_loss_ws_len(n, F), dtype=torch.float64, device=dev)
    pred = torch.full((n, F + 1), -7, dtype=torch.int32, device=dev)
    k.probe_forward(c["Z"], c["d"], c["rows"], c["y"], c["split"], c["W"], c["bias"], F, c["C"], ws, loss, G=G,
                    pred=pred[:, :F])
    torch.cuda.synchronize()
    return G.view(n, F, Cp), loss, pred


def _forward64(c):
    """float64 logits [n, F, C] of the values the kernel reads, and the bound b per logit."""
    n, F, Cp, Cn, d = c["n"], c["F"], c["Cp"], c["C"], c["d"]
    Z = c["Z"].double()
    r = c["rows"].long()
    inside = r < c["table_rows"]
    Zg = Z[r.clamp(max=c["table_rows"] - 1)] * inside[:, None]
    W, bias = c["W"].double(), c["bias"].double()
    logits = (Zg @ W.T + bias).view(n, F, Cp)[:, :, :Cn]
    eps = EPS[c["acc"]]
    b = (2 * d * eps * (Zg.abs() @ W.abs().T + bias.abs())).view(n, F, Cp)[:, :, :Cn]
    return logits, b, eps


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", FORWARD_SHAPES, ids=str)
def test_forward_against_float64(k, dev, dtype, shape):
    n, d, Cn, F = shape
    c = _forward_case(n, d, Cn, F, dtype, dev)
    G, loss, pred = _run_forward(k, c, dev)
    logits, b, eps = _forward64(c)
    bmax = b.amax(2)                                                    # [n, F]
    train = (c["split"] != 0)
    yl = c["y"].long()
    G64 = torch.softmax(logits, 2)
    G64[torch.arange(n, device=dev), :, yl] -= 1.0
    G64 = G64 * train[:, :, None]
    err = (G[:, :, :Cn].double() - G64).abs()
    tol = 2 * bmax[:, :, None] + 8 * eps
    print(f"forward {shape} {dtype}: max |G - G64| / bound = {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())
    assert bool((G[:, :, Cn:] == 0).all())                              # pad columns
    if F > 1:                                                           # the fit without training rows
        assert bool((G[:, F - 1] == 0).all()) and float(loss[F - 1]) == 0.0
    terms = (torch.logsumexp(logits, 2) - logits[torch.arange(n, device=dev), :, yl]) * train
    loss_tol = (2 * bmax * train).sum(0) + n * eps * terms.abs().sum(0)
    loss_err = (loss - terms.sum(0)).abs()
    print(f"forward {shape} {dtype}: max loss error / bound = {float((loss_err / loss_tol.clamp(min=1e-300)).max()):.3f}")
    assert bool((loss_err <= loss_tol).all())
    top2 = logits.topk(2, 2).values
    clear = (top2[:, :, 0] - top2[:, :, 1]) > 2 * bmax
    assert bool(clear.any())
    assert torch.equal(pred[:, :F][clear].long(), logits.argmax(2)[clear])
    assert bool((pred[:, F] == -7).all())                               # nothing written past the F columns
    assert bool(((pred[:, :F] >= 0) & (pred[:, :F] < Cn)).all())        # every row, training or not
    G2, loss2, pred2 = _run_forward(k, c, dev)
    assert torch.equal(G, G2) and torch.equal(loss, loss2) and torch.equal(pred, pred2)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(129, 5, 3, 19), (127, 16, 17, 3), (200, 4, 64, 2)], ids=str)
def test_forward_ties_go_to_the_lowest_class(k, dev, dtype, shape):
    n, d, Cn, F = shape
    c = _forward_case(n, d, Cn, F, dtype, dev, integers=True)           # integer logits: exact in every dtype, many ties
    G, loss, pred = _run_forward(k, c, dev)
    logits, _, _ = _forward64(c)
    top = logits.amax(2, keepdim=True)
    idx = torch.arange(Cn, device=dev).expand_as(logits)
    lowest = torch.where(logits == top, idx, torch.full_like(idx, Cn)).amin(2)
    assert int(((logits == top).sum(2) > 1).sum()) > n // 4             # the case does hold ties
    assert torch.equal(pred[:, :F].long(), lowest)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=str)
def test_grad_against_float64(k, dev, dtype, shape):
    n, K, d = shape
    gen = torch.Generator().manual_seed(n + K + d)
    acc = _hip.acc_dtype(dtype)
    table_rows = max(3, n // 2)
    Z = _padded(torch.randn(table_rows, d, generator=gen, dtype=torch.float64), dtype, dev)
    rows = torch.randint(0, table_rows, (n,), generator=gen).to(torch.int32)
    rows[n // 2] = table_rows
    rows = rows.to(dev)
    G = torch.randn(n, K, generator=gen, dtype=torch.float64).to(acc).to(dev)

    def run():
        ws = torch.full((k.probe_grad_ws_len(n, K, d),), float("nan"), dtype=acc, device=dev)
        dW = torch.full((K * d,), float("nan"), dtype=acc, device=dev)
        db = torch.full((K,), float("nan"), dtype=acc, device=dev)
        k.probe_grad(Z, d, rows, G.view(-1), ws, dW, db)
        torch.cuda.synchronize()
        return dW.view(K, d), db
    dW, db = run()
    Zg = Z.double()[rows.long().clamp(max=table_rows - 1)] * (rows.long() < table_rows)[:, None]
    G64 = G.double()
    eps = EPS[acc]
    tol_w = 2 * n * eps * (G64.abs().T @ Zg.abs())
    tol_b = 2 * n * eps * G64.abs().sum(0)
    err_w, err_b = (dW.double() - G64.T @ Zg).abs(), (db.double() - G64.sum(0)).abs()
    print(f"grad {shape} {dtype}: max error / bound dW {float((err_w / tol_w.clamp(min=1e-300)).max()):.3f} "
          f"db {float((err_b / tol_b.clamp(min=1e-300)).max()):.3f}")
    assert bool((err_w <= tol_w).all()) and bool((err_b <= tol_b).all())
    dW2, db2 = run()
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(10000, 152, 130), (2049, 8, 5)], ids=str)
def test_grad_is_exact_on_integer_data(k, dev, dtype, shape):
    n, K, d = shape                                     # |G| <= 3, |Z| <= 4: every sum below 12 n < 2^24
    gen = torch.Generator().manual_seed(7)
    acc = _hip.acc_dtype(dtype)
    table_rows = n // 3
    Zi = torch.randint(-4, 5, (table_rows, d), generator=gen)
    Gi = torch.randint(-3, 4, (n, K), generator=gen)
    rows = torch.randint(0, table_rows, (n,), generator=gen)
    Z = _padded(Zi.double(), dtype, dev)
    ws = torch.empty(k.probe_grad_ws_len(n, K, d), dtype=acc, device=dev)
    dW = torch.empty(K * d, dtype=acc, device=dev)
    db = torch.empty(K, dtype=acc, device=dev)
    k.probe_grad(Z, d, rows.to(torch.int32).to(dev), Gi.to(acc).to(dev).view(-1), ws, dW, db)
    want = Gi.T @ Zi[rows]
    assert torch.equal(dW.view(K, d).cpu().long(), want) and torch.equal(db.cpu().long(), Gi.sum(0))
    assert torch.equal(dW.view(K, d).cpu().double(), want.double())     # integers, not values near them


# ---- the fit ----------------------------------------------------------------------------------------------------
def _planted(n, d, Cn, sep, seed=0):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, Cn, n)
    y[:Cn] = np.arange(Cn)
    X = rng.standard_normal((Cn, d))[y] * sep + rng.standard_normal((n, d))
    return torch.from_numpy(X), torch.from_numpy(y)


def _objective(X, y, W, b, l2):
    return (torch.nn.functional.cross_entropy(X @ W.T + b, y, reduction="sum") + 0.5 * l2 * (W * W).sum()) / X.shape[0]


@functools.lru_cache(maxsize=None)
def _reference(shape, rounded):
    """Per fit (W, b, J) by torch.optim.LBFGS(strong_wolfe) on the CPU in float64; ``rounded``: on the bf16-rounded table.
    Computed once per shape and shared."""
    n, d, Cn, sep = shape
    X, y = _planted(n, d, Cn, sep, FIT_SEEDS[shape])
    if rounded:
        X = X.to(torch.bfloat16).double()
    split, _ = make_splits(n, FIT_RATIOS, 1, seed=0)
    out = []
    for f in range(split.shape[1]):
        Xt, yt = X[split[:, f].bool()], y[split[:, f].bool()]
        W = torch.zeros(Cn, d, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(Cn, dtype=torch.float64, requires_grad=True)
        opt = torch.optim.LBFGS([W, b], max_iter=2000, tolerance_grad=1e-10, tolerance_change=0, history_size=20,
                                line_search_fn="strong_wolfe")

        def closure():
            opt.zero_grad()
            J = _objective(Xt, yt, W, b, 1.0)
            J.backward()
            return J
        opt.step(closure)
        out.append((W.detach(), b.detach(), float(_objective(Xt, yt, W, b, 1.0).detach())))
    return X, y, split, out


def _ring_engine(X, dtype, dev):
    V = X.shape[0]
    csr = HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + 1) % V).astype(np.int32))
    return SweepEngine(csr, X.to(dtype), dev)


def _host_f1(y, pred, Cn):
    f1, hit = [], 0
    for c in range(Cn):
        tp = int(((y == c) & (pred == c)).sum())
        fp = int(((y != c) & (pred == c)).sum())
        fn = int(((y == c) & (pred != c)).sum())
        hit += tp
        if tp + fp + fn:
            f1.append(2 * tp / (2 * tp + fp + fn))
    return hit / len(y), sum(f1) / len(f1)


@pytest.mark.parametrize("shape", FIT_SHAPES, ids=str)
def test_fit_float64_against_an_independent_lbfgs(dev, shape):
    n, d, Cn, _ = shape
    X, y, split, ref = _reference(shape, False)
    with torch.cuda.device(dev):
        eng = _ring_engine(X, torch.float64, dev)
        probe = LabelProbe(eng, l2=1.0, gtol=1e-8)
        rows = eng.pos[torch.arange(n, device=dev)].to(torch.int32)
        fit = probe.fit(eng.Zcur, rows, y, split, Cn)
    print(f"fit {shape}: iterations {fit.iterations.tolist()} passes {probe.passes}")
    assert bool(fit.converged.all())
    test = split == 0
    conf = confusion_counts(y.to(dev), fit.pred, test.to(dev), Cn)
    micro, macro = f1_from_confusion(conf)
    for f, (W, b, J) in enumerate(ref):
        assert abs(float(fit.objective[f]) - J) <= 1e-9 * J
        assert float((fit.W[f].cpu() - W).abs().max()) <= 1e-4
        bf = fit.b[f].cpu()
        assert float(((bf - bf.mean()) - (b - b.mean())).abs().max()) <= 1e-4
        logits = X @ W.T + b
        top2 = logits.topk(2, 1).values
        clear = ((top2[:, 0] - top2[:, 1]) >= 1e-2) & test[:, f]
        assert int((test[:, f] & ~clear).sum()) <= 0.01 * int(test[:, f].sum())
        pred = fit.pred[:, f].cpu().long()
        assert torch.equal(pred[clear], logits.argmax(1)[clear])
        mi, ma = _host_f1(y[test[:, f]].numpy(), pred[test[:, f]].numpy(), Cn)
        assert float(micro[f]) == pytest.approx(mi, abs=1e-12) and float(macro[f]) == pytest.approx(ma, abs=1e-12)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("shape", FIT_SHAPES, ids=str)
def test_fit_float32_and_bfloat16_reach_the_minimum(dev, dtype, shape):
    n, d, Cn, _ = shape
    gtol, l2 = 1e-4, 1.0
    X, y, split, ref = _reference(shape, dtype == torch.bfloat16)
    with torch.cuda.device(dev):
        eng = _ring_engine(X, dtype, dev)
        probe = LabelProbe(eng, l2=l2, gtol=gtol)
        rows = eng.pos[torch.arange(n, device=dev)].to(torch.int32)
        fit = probe.fit(eng.Zcur, rows, y, split, Cn)
    print(f"fit {shape} {dtype}: iterations {fit.iterations.tolist()} grad_max {fit.grad_max.tolist()}")
    assert bool(fit.converged.all())
    eps = EPS[torch.float32]
    for f, (_, _, J) in enumerate(ref):
        train = split[:, f].bool()
        n_f = int(train.sum())
        Wf, bf = fit.W[f].cpu().double(), fit.b[f].cpu().double()
        Xt = X[train]
        bmax = (2 * d * eps * (Xt.abs() @ Wf.abs().T + bf.abs())).amax(1)
        logits = Xt @ Wf.T + bf
        terms = torch.logsumexp(logits, 1) - logits[torch.arange(n_f), y[train]]
        forward_bound = float((2 * bmax).sum() + n * eps * terms.abs().sum()) / n_f
        excess = float(fit.objective[f]) - J
        bound = gtol ** 2 * Cn * (d + 1) * n_f / (2 * l2) + forward_bound
        print(f"  fit {f}: J - J_ref = {excess:.3e}, bound {bound:.3e}")
        assert excess <= bound


# ---- end to end -------------------------------------------------------------------------------------------------
def _two_blocks(V=120, d=8, seed=0):
    rng = np.random.default_rng(seed)
    block = np.arange(V) % 2
    src, dst = [], []
    for u in range(V):
        same = np.flatnonzero(block == block[u])
        for v in set(rng.choice(same, 5).tolist()) - {u}:
            src.append(u)
            dst.append(v)
        src.append(u)
        dst.append((u + 1) % V)                             # a few links across
    order = np.lexsort((dst, src))
    src, dst = np.asarray(src)[order], np.asarray(dst)[order]
    keep = np.ones(len(src), dtype=bool)
    keep[1:] = (src[1:] != src[:-1]) | (dst[1:] != dst[:-1])
    src, dst = src[keep], dst[keep]
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=V), out=rowptr[1:])
    X = torch.from_numpy((rng.standard_normal((V, d)) + 0.4 * (2 * block[:, None] - 1)).astype(np.float32))
    return HostCSR(V, rowptr, dst.astype(np.int32)), X, block


def test_evaluate_labels_end_to_end(dev):
    csr, X, block = _two_blocks()
    g = Graph.from_csr(csr, X)
    Embedder(g, CosineSimilarity(), dev, tolerence=3, verbose=False).iterate()
    kw = dict(ratios=(0.2, 0.5, 0.8), runs=3, seed=2)
    names = ["even" if b == 0 else "odd" for b in block]
    outZ = g.evaluate_labels(names, **kw)
    assert outZ["class_names"] == ["even", "odd"] and outZ["labelled"] == 120 and all(outZ["fits"]["converged"])
    # the same table from a probe on an engine loaded with the embeddings that left the first one
    with torch.cuda.device(dev):
        other = SweepEngine(csr, g.engine().get_Z(), dev)
        direct = LabelProbe(other).evaluate(list(range(120)), block.tolist(), 2, **kw)
        assert direct["rows"] == outZ["rows"] and direct["fits"] == outZ["fits"]
        outX = g.evaluate_labels(names, table="X", **kw)
        assert outX["rows"] != outZ["rows"] and outX["fits"]["objective"] != outZ["fits"]["objective"]
        # a budget of one fit's G per kernel call: nine groups, no bit changes
        small = LabelProbe(g.engine(), g_budget_bytes=120 * 2 * 4)
        assert len(small.groups(120, 9, 2, torch.float32)) == 9
        grouped = small.evaluate(list(range(120)), block.tolist(), 2, **kw)
        assert grouped["rows"] == outZ["rows"] and grouped["fits"] == outZ["fits"]
    assert all(0.0 <= r["macro_f1"] <= 1.0 and 0.0 <= r["micro_f1"] <= 1.0 and r["runs_used"] == 3 for r in outZ["rows"])
