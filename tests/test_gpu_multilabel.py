"""Multi-label node classification on the GPU: clane_probe_forward_ovr_* (csrc/multilabel_probe.h) against float64 within
a-priori bounds, exact label masks on integer data in both prediction modes, bit-reproducibility, the one-vs-rest fit of
classify.LabelProbe against a per-class torch.optim.LBFGS on the CPU, and the surface (Graph.evaluate_labels, the CLI
section).  Every test prints its figures (error / bound, L-BFGS steps, J - J_ref) before it asserts: run with -s."""
import functools
import json

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.classify import LabelProbe, label_masks, make_splits, mask_bits
from clane_amd.embedder import Embedder
from clane_amd.engine import SweepEngine
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR
from clane_amd.similarity import CosineSimilarity

from .conftest import write_data_root

pytestmark = pytest.mark.gpu

EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}      # unit roundoff of the accumulate type
DTYPES = [torch.float32, torch.bfloat16, torch.float64]
# every Cp from 1 to 64; K = F Cp below (1, 12, 10), at (128: 300 x 17 -> 32 x 5 = 160 crosses, 64 x 3 = 192 crosses,
# 70 x 2 = 140 crosses) and across the 64-column wave and the 128-column tile; partial row tiles; d off the k-slice
FORWARD_SHAPES = [(1, 1, 1, 1), (127, 5, 3, 3), (129, 16, 7, 19), (300, 130, 17, 5), (300, 256, 33, 3), (129, 16, 64, 3),
                  (5000, 130, 2, 70)]
BIG_LOGITS = (300, 130, 17, 5)                                     # this case's W is scaled: |logit| about 100
EXACT_SHAPES = [(129, 16, 7, 19), (127, 5, 64, 3), (300, 8, 17, 5)]
FIT_SHAPES = [(300, 5, 3, 0.8), (600, 16, 7, 0.6), (1000, 130, 17, 0.25)]
FIT_RATIOS = (0.1, 0.5, 0.9)
FIT_RUNS = 2
FIT_SEEDS = {FIT_SHAPES[0]: 3, FIT_SHAPES[1]: 0, FIT_SHAPES[2]: 1}


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


def _case(n, d, Cn, F, dtype, dev, integers=False, scale=1.0):
    gen = torch.Generator().manual_seed(1000 * n + 10 * d + Cn + F)
    acc = _hip.acc_dtype(dtype)
    Cp = _hip.ovr_padded_classes(Cn)
    table_rows = max(3, n // 2)                         # rows repeat
    if integers:
        Zv = torch.randint(-2, 3, (table_rows, d), generator=gen).double()
        W = torch.randint(-1, 2, (F, Cp, d), generator=gen).double()
        bias = torch.randint(-1, 2, (F, Cp), generator=gen).double()
        if Cn >= 3:                                     # equal columns inside one 16-column tile ...
            W[:, 2], bias[:, 2] = W[:, 1], bias[:, 1]
        if Cn >= 41:                                    # ... and in different tiles of a Cp = 64 fit
            W[:, 40], bias[:, 40] = W[:, 3], bias[:, 3]
            W[:, 17], bias[:, 17] = W[:, 1], bias[:, 1]
    else:
        Zv = torch.randn(table_rows, d, generator=gen, dtype=torch.float64)
        W = torch.randn(F, Cp, d, generator=gen, dtype=torch.float64) / max(1.0, d ** 0.5) * 2.0 * scale
        bias = torch.randn(F, Cp, generator=gen, dtype=torch.float64)
    Z = _padded(Zv, dtype, dev)
    rows = torch.randint(0, table_rows, (n,), generator=gen).to(torch.int32)
    rows[n // 2] = table_rows                           # one index past the table: a zero row
    # k_i runs from 0 to C: row i has i % (C + 1) classes, drawn at random
    order = torch.rand(n, Cn, generator=gen).argsort(1)
    Y = torch.zeros(n, Cn, dtype=torch.bool)
    Y.scatter_(1, order, (torch.arange(Cn)[None, :] < (torch.arange(n) % (Cn + 1))[:, None]))
    ymask = (Y.to(torch.int64) << torch.arange(Cn)).sum(1)
    split = (torch.rand(n, F + 2, generator=gen) < 0.5).to(torch.uint8)
    if F > 1:
        split[:, F - 1] = 0                             # a fit that nothing trains
    state = torch.zeros(F, Cp, dtype=torch.int8)
    draw = torch.rand(F, Cn, generator=gen)
    state[:, :Cn][draw < 0.2] = 1                       # about a tenth of the columns constant-positive,
    state[:, :Cn][draw < 0.1] = -1                      # a tenth constant-negative
    state[:, Cn:] = 1                                   # pad columns: ignored whatever the entry says
    if Cn >= 2:
        state[0, 0], state[0, 1] = 1, -1
    return dict(Z=Z, rows=rows.to(dev), ymask=ymask.to(dev), Y=Y.to(dev), split=split.to(dev)[:, :F],
                W=W.view(F * Cp, d).to(acc).to(dev), bias=bias.view(-1).to(acc).to(dev), state=state.view(-1).to(dev),
                n=n, d=d, C=Cn, Cp=Cp, F=F, acc=acc, table_rows=table_rows)


def _run(k, c, dev, top_k=True, max_labels=None):
    n, F, Cp = c["n"], c["F"], c["Cp"]
    G = torch.full((n * F * Cp,), float("nan"), dtype=c["acc"], device=dev)
    loss = torch.full((F,), float("nan"), dtype=torch.float64, device=dev)
    ws = torch.zeros(k.probe_loss_ws_len(n, F), dtype=torch.float64, device=dev)
    pred = torch.full((n, F + 1), -7, dtype=torch.int64, device=dev)
    k.probe_forward_ovr(c["Z"], c["d"], c["rows"], c["ymask"], c["split"], c["W"], c["bias"], c["state"], F, c["C"],
                        c["C"] if max_labels is None else max_labels, ws, loss, G=G, pred=pred[:, :F], top_k=top_k)
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
    b = (2 * d * eps * (Zg.abs() @ W.abs().T) + eps * bias.abs()).view(n, F, Cp)[:, :, :Cn]
    return logits, b, eps


def _expected_masks(logits, state, Y, top_k):
    """int64 [n, F] from float64 logits [n, F, C], the states [F, C] and the truth [n, C], on the logits' device."""
    n, F, Cn = logits.shape
    inf = torch.full_like(logits, float("inf"))
    val = torch.where(state[None] == 0, logits, torch.where(state[None] < 0, -inf, inf))
    if top_k:
        order = torch.sort(val, dim=2, descending=True, stable=True).indices       # ties: the lowest class first
        first = torch.arange(Cn, device=logits.device)[None, None, :] < Y.sum(1)[:, None, None]
        sel = torch.zeros_like(first.expand(n, F, Cn)).scatter(2, order, first.expand(n, F, Cn)) & (val > -inf)
    else:
        sel = val > 0
    return (sel.to(torch.int64) << torch.arange(Cn, device=logits.device)).sum(2)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", FORWARD_SHAPES, ids=str)
def test_forward_against_float64(k, dev, dtype, shape):
    n, d, Cn, F = shape
    c = _case(n, d, Cn, F, dtype, dev, scale=25.0 if shape == BIG_LOGITS else 1.0)
    G, loss, pred = _run(k, c, dev)
    logits, b, eps = _forward64(c)
    if shape == BIG_LOGITS:
        print(f"forward {shape} {dtype}: max |logit| = {float(logits.abs().max()):.1f}")
        assert float(logits.max()) > 80 and float(logits.min()) < -80
    assert bool(torch.isfinite(G).all()) and bool(torch.isfinite(loss).all())      # neither branch overflows
    state = c["state"].view(F, c["Cp"])[:, :Cn]
    live = (c["split"] != 0)[:, :, None] & (state == 0)[None]
    y = c["Y"][:, None, :].double()
    G64 = (torch.sigmoid(logits) - y) * live
    err = (G[:, :, :Cn].double() - G64).abs()
    tol = b / 2 + 8 * eps
    print(f"forward {shape} {dtype}: max |G - G64| / bound = {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())
    assert bool((G[:, :, Cn:] == 0).all())                              # pad columns: exactly 0
    assert bool((G[:, :, :Cn][~live] == 0).all())                       # constant columns, rows that do not train
    terms = (torch.nn.functional.softplus(logits) - y * logits) * live
    loss_tol = (2 * b * live).sum((0, 2)) + n * Cn * eps * terms.abs().sum((0, 2))
    loss_err = (loss - terms.sum((0, 2))).abs()
    print(f"forward {shape} {dtype}: max loss error / bound = {float((loss_err / loss_tol.clamp(min=1e-300)).max()):.3f}")
    assert bool((loss_err <= loss_tol).all())
    fitted = (live.sum((0, 2)) > 0)
    assert bool((loss[~fitted] == 0).all())                             # no live entry: no loss (the untrained fit)
    if F > 1:
        assert float(loss[F - 1]) == 0.0 and bool((G[:, F - 1] == 0).all())
    assert bool((pred[:, F] == -7).all())                               # nothing written past the F columns
    # masks where every gap between a value and the k-th largest exceeds the bound
    val = torch.where(state[None] == 0, logits, torch.where(state[None] < 0, -torch.inf, torch.inf).double())
    ranked = val.sort(2, descending=True).values
    k_i = c["Y"].sum(1)
    kth = ranked.gather(2, (k_i - 1).clamp(min=0)[:, None, None].expand(n, F, 1))[:, :, 0]
    nxt = ranked.gather(2, k_i.clamp(max=Cn - 1)[:, None, None].expand(n, F, 1))[:, :, 0]
    clear = (k_i[:, None] == 0) | (k_i[:, None] == Cn) | (kth - nxt > 2 * b.amax(2)) | ((kth == nxt) & torch.isinf(kth))
    want = _expected_masks(logits, state, c["Y"], True)
    assert bool(clear.any()) and torch.equal(pred[:, :F][clear], want[clear])
    assert bool(((pred[:, :F] >> Cn) == 0).all() if Cn < 64 else True)  # no bit at or above C


@pytest.mark.parametrize("top_k", [True, False], ids=["top_k", "threshold"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=str)
def test_label_masks_are_exact_on_integer_data(k, dev, dtype, shape, top_k):
    n, d, Cn, F = shape
    c = _case(n, d, Cn, F, dtype, dev, integers=True)                   # integer logits: exact in every dtype
    _, _, pred = _run(k, c, dev, top_k=top_k)
    logits, _, _ = _forward64(c)
    state = c["state"].view(F, c["Cp"])[:, :Cn]
    want = _expected_masks(logits.cpu(), state.cpu(), c["Y"].cpu(), top_k)         # float64 on the CPU
    got = pred[:, :F].cpu()
    k_i = c["Y"].sum(1).cpu()
    bits = mask_bits(got, Cn)
    ties = int((logits[:, :, 1] == logits[:, :, 2]).sum()) if Cn >= 3 else 0
    print(f"masks {shape} {dtype} top_k={top_k}: zero logits {int((logits == 0).sum())}, tied pairs {ties}, "
          f"k_i 0..{int(k_i.max())}, rows short of k_i {int((bits.sum(2) < k_i[:, None]).sum())}")
    assert int((logits == 0).sum()) > 0 and ties >= n * F                  # the duplicated columns tie on every row
    assert int(k_i.min()) == 0 and int(k_i.max()) == Cn
    assert torch.equal(got, want)
    assert bool((pred[:, F] == -7).all())
    st = state.cpu()
    assert not bool(bits[:, st == -1].any())                            # a constant-negative column: never
    if top_k:
        assert bool((bits.sum(2) <= k_i[:, None]).all()) and bool((got[k_i == 0] == 0).all())
        assert bool(bits[k_i >= 1, 0, 0].all())                         # fit 0's class 0 is +1: the first place
        assert bool((bits[k_i == Cn, 0].sum(1) < Cn).all())             # fit 0 has a -1 column: fewer than k_i bits
    else:
        assert torch.equal(bits, ((logits.cpu() > 0) & (st == 0)[None]) | (st == 1)[None])     # logit 0: not predicted


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(300, 16, 7, 5), (129, 40, 33, 5)], ids=str)
def test_bits_do_not_depend_on_the_call(k, dev, dtype, shape):
    n, d, Cn, F = shape
    c = _case(n, d, Cn, F, dtype, dev)                                  # random, non-integer data
    c["split"] = c["split"].clone()
    c["split"][:, F - 1] = c["split"][:, 0] ^ 1
    Cp = c["Cp"]
    G, loss, pred = _run(k, c, dev)
    G2, loss2, pred2 = _run(k, c, dev)
    assert torch.equal(G, G2) and torch.equal(loss, loss2) and torch.equal(pred, pred2)
    assert bool((loss > 0).all())

    def pick(fits):
        idx = torch.tensor(fits, device=dev)
        wide = torch.zeros(n, len(fits) + 2, dtype=torch.uint8, device=dev)
        wide[:, :len(fits)] = c["split"][:, idx]
        return dict(c, F=len(fits), split=wide[:, :len(fits)], W=c["W"].view(F, Cp, d)[idx].reshape(-1, d).contiguous(),
                    bias=c["bias"].view(F, Cp)[idx].reshape(-1).contiguous(),
                    state=c["state"].view(F, Cp)[idx].reshape(-1).contiguous())
    for f in range(F):                                                  # fit f alone
        Ga, la, pa = _run(k, pick([f]), dev)
        assert torch.equal(Ga[:, 0], G[:, f]) and torch.equal(la[0], loss[f]) and torch.equal(pa[:, 0], pred[:, f]), f
    order = [3, 4, 0, 1, 2]                                             # and at another position, beside other fits
    Gb, lb, pb = _run(k, pick(order), dev)
    for pos, f in enumerate(order):
        assert torch.equal(Gb[:, pos], G[:, f]) and torch.equal(lb[pos], loss[f]) and torch.equal(pb[:, pos], pred[:, f])


# ---- the fit ----------------------------------------------------------------------------------------------------
def _planted(n, d, Cn, sep):
    """1-3 classes per row (mostly 1: 85 / 12 / 3 %), class c drawn with weight (c + 1)^-2 (^-3 for up to 4 classes) -- the last classes are rare
    enough to be absent from a 10 % training share; a row is the sum of its classes' directions times sep plus noise.
    The seed is picked per shape, from the labels and the splits alone, such that a 10 % fit does miss a class."""
    rng = np.random.default_rng(FIT_SEEDS[(n, d, Cn, sep)])
    freq = 1.0 / (1.0 + np.arange(Cn)) ** (3 if Cn <= 4 else 2)
    freq /= freq.sum()
    dirs = rng.standard_normal((Cn, d))
    Y = np.zeros((n, Cn))
    for i in range(n):
        Y[i, rng.choice(Cn, size=int(rng.choice(3, p=(0.85, 0.12, 0.03))) + 1, replace=False, p=freq)] = 1.0
    X = Y @ dirs * sep + rng.standard_normal((n, d))
    return torch.from_numpy(X), torch.from_numpy(Y)


def _column_objective(Xt, yt, w, b, l2):
    bce = torch.nn.functional.binary_cross_entropy_with_logits(Xt @ w + b, yt, reduction="sum")
    return (bce + 0.5 * l2 * (w * w).sum()) / Xt.shape[0]


@functools.lru_cache(maxsize=None)
def _reference(shape, rounded):
    """Per fit (W [C, d], b [C], state [C], J) by one torch.optim.LBFGS(strong_wolfe) per fitted class on the CPU in
    float64; ``rounded``: on the bf16-rounded table.  Computed once per shape and shared."""
    n, d, Cn, sep = shape
    X, Y = _planted(n, d, Cn, sep)
    if rounded:
        X = X.to(torch.bfloat16).double()
    split, _ = make_splits(n, FIT_RATIOS, FIT_RUNS, seed=0)
    out = []
    for f in range(split.shape[1]):
        train = split[:, f].bool()
        Xt = X[train]
        W, b = torch.zeros(Cn, d, dtype=torch.float64), torch.zeros(Cn, dtype=torch.float64)
        state, J = torch.zeros(Cn, dtype=torch.int8), 0.0
        for cl in range(Cn):
            yt = Y[train, cl]
            if float(yt.sum()) in (0.0, float(yt.numel())):
                state[cl] = -1 if float(yt.sum()) == 0.0 else 1
                continue
            w = torch.zeros(d, dtype=torch.float64, requires_grad=True)
            b0 = torch.zeros(1, dtype=torch.float64, requires_grad=True)
            opt = torch.optim.LBFGS([w, b0], max_iter=2000, tolerance_grad=1e-10, tolerance_change=0, history_size=20,
                                    line_search_fn="strong_wolfe")

            def closure():
                opt.zero_grad()
                Jc = _column_objective(Xt, yt, w, b0, 1.0)
                Jc.backward()
                return Jc
            opt.step(closure)
            W[cl], b[cl] = w.detach(), b0.detach()[0]
            J += float(_column_objective(Xt, yt, w, b0, 1.0).detach())
        out.append((W, b, state, J))
    return X, Y, split, out


def _ring_engine(X, dtype, dev):
    V = X.shape[0]
    csr = HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + 1) % V).astype(np.int32))
    return SweepEngine(csr, X.to(dtype), dev)


def _masks(Y):
    return label_masks([np.flatnonzero(r).tolist() for r in Y.numpy()], Y.shape[1])


def test_the_planted_data_has_constant_columns():
    for shape in FIT_SHAPES:                                            # a property of the data alone
        _, Y = _planted(*shape)
        split, _ = make_splits(shape[0], FIT_RATIOS, FIT_RUNS, seed=0)
        absent = [bool((Y[split[:, f].bool()].sum(0) == 0).any()) for f in range(FIT_RUNS)]       # the 10 % fits
        print(f"planted {shape}: a class absent from training in runs {absent}")
        assert any(absent)


@pytest.mark.parametrize("shape", FIT_SHAPES, ids=str)
def test_fit_float64_against_an_independent_per_class_lbfgs(dev, shape):
    n, d, Cn, _ = shape
    X, Y, split, ref = _reference(shape, False)
    with torch.cuda.device(dev):
        eng = _ring_engine(X, torch.float64, dev)
        probe = LabelProbe(eng, l2=1.0, gtol=1e-8)
        rows = eng.pos[torch.arange(n, device=dev)].to(torch.int32)
        fit = probe.fit_multilabel(eng.Zcur, rows, _masks(Y), split, Cn)
    print(f"fit {shape}: iterations {fit.iterations.tolist()} constant {fit.constant.tolist()} passes {probe.passes}")
    assert bool(fit.converged.all()) and not bool(fit.skipped.any())
    eps = EPS[torch.float64]
    k_i = Y.sum(1).long()
    for f, (W, b, state, J) in enumerate(ref):
        assert int(fit.constant[f]) == int((state != 0).sum())
        Wf, bf = fit.W[f].cpu(), fit.b[f].cpu()
        print(f"  fit {f}: |J - J_ref| / J = {abs(float(fit.objective[f]) - J) / J:.2e}, "
              f"max |W - W_ref| = {float((Wf - W).abs().max()):.2e}")
        assert abs(float(fit.objective[f]) - J) <= 1e-9 * J
        assert float((Wf - W).abs().max()) <= 1e-4 and float((bf - b).abs().max()) <= 1e-4
        assert float(Wf[state != 0].abs().max() if bool((state != 0).any()) else 0.0) == 0.0
        # rows whose k-th and (k + 1)-th reference values are further apart than the forward bound plus what weights
        # that agree to 1e-4 (asserted above) can move a logit by: 1e-4 (|x|_1 + 1), twice
        logits = X @ W.T + b
        val = torch.where(state[None] == 0, logits, torch.where(state[None] < 0, -torch.inf, torch.inf).double())
        ranked = val.sort(1, descending=True).values
        kth = ranked.gather(1, (k_i - 1)[:, None])[:, 0]
        nxt = ranked.gather(1, k_i.clamp(max=Cn - 1)[:, None])[:, 0]
        bound = 2 * d * eps * (X.abs() @ W.abs().T).amax(1) + eps * b.abs().max()
        clear = (k_i == Cn) | (kth - nxt > 2 * bound + 2e-4 * (X.abs().sum(1) + 1))
        want = _expected_masks(logits[:, None, :], state[None], Y.bool(), True)[:, 0]
        print(f"  fit {f}: rows compared {int(clear.sum())} / {n}")
        assert int(clear.sum()) >= n // 2
        assert torch.equal(fit.pred[:, f].cpu()[clear], want[clear])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("shape", FIT_SHAPES, ids=str)
def test_fit_float32_and_bfloat16_reach_the_minimum(dev, dtype, shape):
    n, d, Cn, _ = shape
    gtol, l2 = 1e-4, 1.0
    X, Y, split, ref = _reference(shape, dtype == torch.bfloat16)
    with torch.cuda.device(dev):
        eng = _ring_engine(X, dtype, dev)
        probe = LabelProbe(eng, l2=l2, gtol=gtol)
        rows = eng.pos[torch.arange(n, device=dev)].to(torch.int32)
        fit = probe.fit_multilabel(eng.Zcur, rows, _masks(Y), split, Cn)
    print(f"fit {shape} {dtype}: iterations {fit.iterations.tolist()} grad_max {fit.grad_max.tolist()}")
    assert bool(fit.converged.all())
    eps = EPS[torch.float32]
    for f, (_, _, state, J) in enumerate(ref):                          # J_ref: the float64 CPU loop's
        train = split[:, f].bool()
        n_f = int(train.sum())
        Wf, bf = fit.W[f].cpu().double(), fit.b[f].cpu().double()
        Xt, Yt = X[train], Y[train]
        fitted = (state == 0)[None, :].double()
        b_logit = 2 * d * eps * (Xt.abs() @ Wf.abs().T) + eps * bf.abs()
        logits = Xt @ Wf.T + bf
        terms = (torch.nn.functional.softplus(logits) - Yt * logits) * fitted
        forward_bound = float((2 * b_logit * fitted).sum() + n * Cn * eps * terms.abs().sum()) / n_f
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
    return HostCSR(V, rowptr, dst.astype(np.int32)), X, block, src, dst


def _sets(block):
    """even / odd from the block, "third" on every third vertex, "rare" on two vertices."""
    return [(["even"] if b == 0 else ["odd"]) + (["third"] if i % 3 == 0 else []) + (["rare"] if i in (5, 77) else [])
            for i, b in enumerate(block)]


def test_evaluate_labels_multilabel_end_to_end(dev):
    csr, X, block, _, _ = _two_blocks()
    g = Graph.from_csr(csr, X)
    Embedder(g, CosineSimilarity(), dev, tolerence=3, verbose=False).iterate()
    kw = dict(ratios=(0.2, 0.5, 0.8), runs=3, seed=2)
    sets = _sets(block)
    out = g.evaluate_labels(sets, multilabel=True, **kw)
    assert out["class_names"] == ["even", "odd", "rare", "third"] and out["labelled"] == 120 and out["classes"] == 4
    assert out["multilabel"] is True and out["predict"] == "top_k" and all(out["fits"]["converged"])
    assert out["constant_columns"] == sum(out["fits"]["constant_columns"]) >= 1         # "rare" misses a 20 % share
    names = out["class_names"]
    indexed = [[names.index(c) for c in s] for s in sets]
    with torch.cuda.device(dev):
        other = SweepEngine(csr, g.engine().get_Z(), dev)
        direct = LabelProbe(other).evaluate(list(range(120)), indexed, 4, multilabel=True, **kw)
        assert direct["rows"] == out["rows"] and direct["fits"] == out["fits"]
        small = LabelProbe(g.engine(), g_budget_bytes=120 * 4 * 4)      # one fit's G per kernel call
        assert len(small.groups(120, 9, 4, torch.float32)) == 9
        grouped = small.evaluate(list(range(120)), indexed, 4, multilabel=True, **kw)
        assert grouped["rows"] == out["rows"] and grouped["fits"] == out["fits"]
        thr = g.evaluate_labels((list(range(120)), sets), multilabel=True, predict="threshold", **kw)
    assert thr["predict"] == "threshold" and thr["fits"]["objective"] == out["fits"]["objective"]
    print("multilabel rows:", out["rows"])
    assert all(0.0 <= r["macro_f1"] <= r["micro_f1"] <= 1.0 and r["runs_used"] == 3 for r in out["rows"])
    assert out["rows"][-1]["micro_f1"] > 0.6                            # the blocks are planted: far above chance


def test_cli_section_writes_the_multilabel_keys(dev, tmp_path):
    from clane_amd.__main__ import embedding, get_parser
    csr, X, block, src, dst = _two_blocks()
    ids = np.asarray([f"v{i}" for i in range(120)])
    root = write_data_root(tmp_path / "data", ids, ids[src], ids[dst], X.numpy())
    (root / "Y").write_text("".join(f"v{i}\t{c}\n" for i, s in enumerate(_sets(block)) for c in s))
    config = ("graph:\n  embedding_dim: 8\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
              "embedder:\n  gamma: 0.76\n  tolerence: 3\n\nnode_classification:\n  labels: Y\n  ratios: [0.3, 0.7]\n"
              "  runs: 2\n  seed: 4\n")
    cfg = tmp_path / "config.yaml"

    def run(extra, out):
        cfg.write_text(config + extra)
        embedding(get_parser().parse_args(["--data_root", str(root), "--config_file", str(cfg), "--gpu",
                                           "--output_root", str(tmp_path / out)]))
    run("  multilabel: true\n  predict: threshold\n  baseline: true\n", "multi")
    got = json.loads((tmp_path / "multi" / "label_metrics.json").read_text())
    assert set(got) == {"labels", "labelled", "class_names", "ratios", "runs", "seed", "l2", "tables", "multilabel",
                        "predict", "constant_columns"}
    assert got["multilabel"] is True and got["predict"] == "threshold" and set(got["constant_columns"]) == {"Z", "X"}
    assert got["class_names"] == ["even", "odd", "rare", "third"] and got["labelled"] == 120
    assert all(len(t["rows"]) == 2 and len(t["fits"]["constant_columns"]) == 4 for t in got["tables"].values())
    with pytest.raises(ValueError, match=r"line 2: 'v0' was labelled on line 1"):      # single-label: as before
        run("", "single")
