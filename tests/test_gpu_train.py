"""Training the bilinear similarity on the card (csrc/pair_train.h): each kernel against fp64 with bounds derived from
the operation counts, the reference's own training run (fixture g14) replayed in fp64 and teacher-forced in fp32 / bf16,
and AlternatingEmbedder end to end on a planted two-block graph."""
import math

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.embedder import AlternatingEmbedder, Embedder
from clane_amd.engine import SweepEngine
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR
from clane_amd.similarity import AsymmertricSimilarity
from clane_amd.train import rows_of_vertices

from .conftest import load_golden, write_data_root

pytestmark = pytest.mark.gpu

GOLD = "g14_karate_asym_train.npz"
EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
CHUNK = 2048                              # pairs per workgroup of the gradient kernel (clane_pair_grad_ws_len)
DTYPES = [torch.float32, torch.bfloat16, torch.float64]


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


def _table(rows, d, dtype, dev, gen, pad=3):
    """A [rows, d + pad] table whose first d columns are random (the padded leading dimension of the general case)."""
    Zc = torch.randn(rows, d, generator=gen, dtype=torch.float64).to(dtype)
    buf = torch.zeros(rows, d + pad, dtype=dtype, device=dev)
    buf[:, :d] = Zc.to(dev)
    return buf, Zc.to(dev).double()


def _pairs(B, rows, dev, gen):
    src = torch.randint(0, rows, (B,), generator=gen, dtype=torch.int32)
    dst = torch.randint(0, rows, (B,), generator=gen, dtype=torch.int32)
    if B >= 4:                            # repeated and out-of-order indices
        src[1], dst[2], src[B - 1] = src[0], src[0], rows - 1
    return src.to(dev), dst.to(dev)


# ---- 1. pair_project ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_project_against_fp64(dev, k, dtype):
    """|A - A64| <= 2 d eps (|Z| |W|^T) elementwise, as test_project_rows_against_fp64: a k-ordered fma chain of d terms
    in the accumulate type (bf16 rows are exact in f32); a second call gives the same bits."""
    acc = _hip.acc_dtype(dtype)
    gen = torch.Generator().manual_seed(11)
    for d in (1, 5, 16, 130, 256):
        rows = 5000
        Z, Z64 = _table(rows, d, dtype, dev, gen)
        W = (torch.randn(2 * d, d, generator=gen, dtype=torch.float64) / d ** 0.5).to(acc).to(dev).contiguous()
        W64 = W.double()
        for B in (1, 4, 1000, 100_003):
            src, dst = _pairs(B, rows, dev, gen)
            A = torch.full((B, d), float("nan"), dtype=acc, device=dev)
            Bm = torch.full((B, d), float("nan"), dtype=acc, device=dev)
            k.pair_project(Z, d, src, dst, W, A, Bm)
            A1, B1 = A.clone(), Bm.clone()
            k.pair_project(Z, d, src, dst, W, A, Bm)
            assert torch.equal(A1, A) and torch.equal(B1, Bm), (dtype, d, B)
            for got, idx, Ws in ((A1, src, W64[:d]), (B1, dst, W64[d:])):
                zz = Z64[idx.long()]
                want = zz @ Ws.T
                bound = 2 * d * EPS[acc] * (zz.abs() @ Ws.abs().T) + 1e-300
                err = (got.double() - want).abs()
                assert bool((err <= bound).all()), (dtype, d, B, float((err / bound).max()))


# ---- 2. pair_loss ---------------------------------------------------------------------------------------------------
def _loss_reference(A64, B64, linked, u64, mask=None):
    s = (A64 * B64).sum(1)
    p, q = torch.sigmoid(s), torch.sigmoid(-s)
    lk = linked.bool()
    mk = (lk ^ (u64 < p)) if mask is None else mask.bool()
    loss = -torch.log(torch.where(lk, p, q) + 1e-10)
    g = torch.where(lk, -p * q / (p + 1e-10), p * q / (q + 1e-10))
    return s, p, q, mk, loss, torch.where(mk, g, torch.zeros_like(g))


def _score_error(A64, B64, d, eps):
    """Bound on |s - s64| for s accumulated in the accumulate type from the given A, Bm: products and a chain of d
    adds (each lane sums d / 16 terms, then 4 butterfly adds): at most d roundings per term, doubled for safety."""
    return 2 * d * eps * (A64.abs() * B64.abs()).sum(1)


@pytest.mark.parametrize("acc", [torch.float32, torch.float64])
def test_pair_loss_against_fp64(dev, k, acc):
    """mask equals the fp64 mask except where |u - p64| is within the forward error of p (|dp/ds| <= 1/4 times the error
    of s, plus 8 eps for exp, add and divide); such pairs are at most 0.1 % of a case.  g and stats against fp64 with the
    kernel's own mask: |dg/ds| <= 0.3 and |dloss/ds| <= 1 propagate the error of s, 16 eps cover the five to six
    roundings of the closed forms.  Scores reach |s| = 40, where 1 - p would be 0 in fp32."""
    eps = EPS[acc]
    gen = torch.Generator().manual_seed(23)
    ws = torch.zeros(k.reduce_ws_len(), dtype=torch.float64, device=dev)
    for d, B in ((1, 1), (5, 4), (16, 1000), (130, 4099), (256, 100_003)):
        A = torch.randn(B, d, generator=gen, dtype=torch.float64).to(acc).to(dev)
        Bm = (torch.randn(B, d, generator=gen, dtype=torch.float64) / d ** 0.5).to(acc).to(dev)
        if B >= 1000:                     # a band of large scores of both signs: s = +-10 .. +-40
            n = 200
            scale = torch.linspace(10, 40, n, dtype=torch.float64) * torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0)
            A[:n] = 0
            Bm[:n] = 0
            A[:n, 0] = scale.to(acc).to(dev)
            Bm[:n, 0] = 1
        linked = (torch.rand(B, generator=gen) < 0.5).to(torch.uint8).to(dev)
        u = torch.rand(B, generator=gen, dtype=torch.float64).to(acc).to(dev)
        g = torch.full((B,), float("nan"), dtype=acc, device=dev)
        mask = torch.full((B,), 7, dtype=torch.uint8, device=dev)
        stats = torch.zeros(2, dtype=torch.float64, device=dev)
        k.pair_loss(A, Bm, d, linked, u, g, mask, ws, stats)
        g1, m1, s1 = g.clone(), mask.clone(), stats.clone()
        k.pair_loss(A, Bm, d, linked, u, g, mask, ws, stats)
        assert torch.equal(g1, g) and torch.equal(m1, mask) and torch.equal(s1, stats), (acc, d, B)
        A64, B64, u64 = A.double(), Bm.double(), u.double()
        ds = _score_error(A64, B64, d, eps)
        s, p, q, mk64, _, _ = _loss_reference(A64, B64, linked, u64)
        dp = 0.25 * ds + 8 * eps
        near = (u64 - p).abs() <= dp
        differs = mk64 != m1.bool()
        print(f"pair_loss {acc} d={d} B={B}: near={int(near.sum())} differs={int(differs.sum())} |s|max={float(s.abs().max()):.1f}")
        assert int(near.sum()) <= max(1, B // 1000) if B >= 1000 else True, (acc, d, B, int(near.sum()))
        assert not bool((differs & ~near).any()), (acc, d, B)
        _, p, q, _, loss, g64 = _loss_reference(A64, B64, linked, u64, mask=m1)
        dg = 0.3 * ds + 16 * eps * g64.abs() + 1e-300
        errg = (g1.double() - g64).abs()
        assert bool((errg <= dg).all()), (acc, d, B, float((errg / dg).max()))
        assert float(s1[1]) == float(m1.sum())
        want0 = float(loss[m1.bool()].sum())
        bound0 = float((ds + 16 * eps * (loss.abs() + 1))[m1.bool()].sum()) + 1e-300
        print(f"   stats0 {float(s1[0]):.9g} want {want0:.9g} bound {bound0:.3g}")
        assert abs(float(s1[0]) - want0) <= bound0, (acc, d, B)


# ---- 3. pair_grad ---------------------------------------------------------------------------------------------------
def _autograd_dW(Z64, src, dst, W64, linked, mask):
    """torch.autograd of the reference's expression (embedder.py:276-283) in fp64 with the given mask."""
    d = W64.shape[1]
    W = W64.clone().requires_grad_(True)
    prob = ((Z64[src.long()] @ W[:d].T) * (Z64[dst.long()] @ W[d:].T)).sum(1).sigmoid()
    loss = prob.where(linked.bool(), 1 - prob).add(1e-10).log().neg()
    loss.masked_select(mask.bool()).mean().backward()
    return W.grad.detach()


def _grad_bound(Z64, src, dst, W64, A64, B64, g64, M, B, d, eps, rows_sel):
    """Elementwise bound for rows `rows_sel` of both halves of dW.  Per term g_k Bm[k,o] Z[src_k,i] / M the kernel rounds
    the product g_k Bm (1), each accumulation step of its chunk and of the sum over the chunks (at most n_k in all) and
    the division by M (1): at most n_k + 2 roundings, bounded here by c (n_k + d) eps with c = 2.  On top come the errors
    the operands arrive with: A and Bm from pair_project (2 d eps |Z| |W|^T), and g from pair_loss (0.3 times the error
    of s -- its own accumulation plus what A and Bm carry into it -- plus 16 eps |g|)."""
    zs, zd = Z64[src.long()].abs(), Z64[dst.long()].abs()
    dA = 2 * d * eps * (zs @ W64[:d].abs().T)
    dB = 2 * d * eps * (zd @ W64[d:].abs().T)
    ds = 2 * d * eps * (A64.abs() * B64.abs()).sum(1) + (dA * B64.abs() + A64.abs() * dB).sum(1)
    dg = torch.where(g64 != 0, 0.3 * ds + 16 * eps * g64.abs(), torch.zeros_like(ds))
    c = 2 * (B + d) * eps
    out = []
    for P64, dP, zz in ((B64, dB, zs), (A64, dA, zd)):
        Ps, dPs = P64[:, rows_sel].abs(), dP[:, rows_sel]
        per = (c * g64.abs()[:, None] * Ps + dg[:, None] * Ps + g64.abs()[:, None] * dPs)
        out.append(per.T @ zz / max(M, 1))
    return torch.cat(out, 0) + 1e-300


def _closed_form(Z64, src, dst, A64, B64, g64, M, rows_sel):
    top = (g64[:, None] * B64[:, rows_sel]).T @ Z64[src.long()] / max(M, 1)
    bot = (g64[:, None] * A64[:, rows_sel]).T @ Z64[dst.long()] / max(M, 1)
    return torch.cat([top, bot], 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_grad_against_fp64(dev, k, dtype):
    """project -> loss -> grad on the card against torch.autograd in fp64 of the reference's expression with the same
    pairs and the kernel's mask; bound: see _grad_bound (c = 2).  B = 4, one chunk - 1 / exactly / + 1, and 262 144 pairs at
    d = 256 (sampled rows of dW against the closed form, which the small cases check against autograd); M = 0; the
    same bits on a second call."""
    acc = _hip.acc_dtype(dtype)
    eps = EPS[acc]
    gen = torch.Generator().manual_seed(31)
    ws = torch.zeros(k.reduce_ws_len(), dtype=torch.float64, device=dev)
    for d, B in ((5, 4), (16, CHUNK - 1), (130, CHUNK), (16, CHUNK + 1), (256, 262_144)):
        rows = 20_000
        Z, Z64 = _table(rows, d, dtype, dev, gen)
        W = (torch.randn(2 * d, d, generator=gen, dtype=torch.float64) / d ** 0.75).to(acc).to(dev).contiguous()
        W64 = W.double()
        src, dst = _pairs(B, rows, dev, gen)
        linked = (torch.rand(B, generator=gen) < 0.5).to(torch.uint8).to(dev)
        u = torch.rand(B, generator=gen, dtype=torch.float64).to(acc).to(dev)
        A = torch.empty(B, d, dtype=acc, device=dev)
        Bm = torch.empty(B, d, dtype=acc, device=dev)
        g = torch.empty(B, dtype=acc, device=dev)
        mask = torch.empty(B, dtype=torch.uint8, device=dev)
        stats = torch.zeros(2, dtype=torch.float64, device=dev)
        gws = torch.full((k.pair_grad_ws_len(B, d),), float("nan"), dtype=acc, device=dev)
        dW = torch.full((2 * d, d), float("nan"), dtype=acc, device=dev)
        k.pair_project(Z, d, src, dst, W, A, Bm)
        k.pair_loss(A, Bm, d, linked, u, g, mask, ws, stats)
        k.pair_grad(Z, d, src, dst, A, Bm, g, stats, gws, dW)
        first = dW.clone()
        k.pair_grad(Z, d, src, dst, A, Bm, g, stats, gws, dW)
        assert torch.equal(first, dW), (dtype, d, B)
        M = int(stats[1])
        assert M > 0
        A64 = Z64[src.long()] @ W64[:d].T
        B64 = Z64[dst.long()] @ W64[d:].T
        _, _, _, _, _, g64 = _loss_reference(A64, B64, linked, u.double(), mask=mask)
        sel = torch.arange(d, device=dev) if B <= CHUNK + 1 else torch.tensor([0, 1, 63, 64, 127, 128, 200, 255], device=dev)
        want = _closed_form(Z64, src, dst, A64, B64, g64, M, sel)
        if B <= CHUNK + 1:
            auto = _autograd_dW(Z64, src, dst, W64, linked, mask)
            assert float((auto - want).abs().max()) <= 1e-12 * max(1.0, float(auto.abs().max())), (dtype, d, B)
            want = auto
        bound = _grad_bound(Z64, src, dst, W64, A64, B64, g64, M, B, d, eps, sel)
        got = torch.cat([first[:d][sel], first[d:][sel]], 0).double()
        err = (got - want).abs()
        print(f"pair_grad {dtype} d={d} B={B} M={M}: max err {float(err.max()):.3e} max err/bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (dtype, d, B, float((err / bound).max()))
        # M = 0: nobody takes part (unlinked pairs whose trial fails) -- dW is exactly zero
        zero_l = torch.zeros(B, dtype=torch.uint8, device=dev)
        one_u = torch.ones(B, dtype=acc, device=dev)
        k.pair_loss(A, Bm, d, zero_l, one_u, g, mask, ws, stats)
        k.pair_grad(Z, d, src, dst, A, Bm, g, stats, gws, dW)
        assert float(stats[1]) == 0 and not bool(dW.any()) and not bool(mask.any()), (dtype, d, B)


# ---- 4. adam_step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [torch.float32, torch.float64])
def test_adam_step_against_torch(dev, k, acc):
    """50 steps with random gradients, every seventh skipped (stats[1] = 0), against torch.optim.Adam on the CPU in the
    same dtype.  fp64: 1e-12 relative.  fp32: one step is about a dozen roundings (lerp 2, v 3, sqrt, divide, add, multiply,
    divide, add), each worth at most one ulp of an update of size ~lr, and contraction into fma may move each; the
    states m, v carry theirs forward with weights 0.9 / 0.999.  Bound: 16 ulp of lr per step taken, accumulated."""
    n, lr = 2 * 37 * 37, 1e-2
    gen = torch.Generator().manual_seed(41)
    W0 = torch.randn(n, generator=gen, dtype=torch.float64).to(acc)
    ref = torch.nn.Parameter(W0.clone())
    opt = torch.optim.Adam([ref], lr=lr)
    W, m, v = W0.clone().to(dev), torch.zeros(n, dtype=acc, device=dev), torch.zeros(n, dtype=acc, device=dev)
    state = torch.zeros(2, dtype=torch.float64, device=dev)
    taken, loss_sum = 0, 0.0
    for step in range(50):
        grad = (torch.randn(n, generator=gen, dtype=torch.float64) * 10 ** float(torch.randint(-3, 2, (1,), generator=gen))).to(acc)
        skip = step % 7 == 3
        stats = torch.tensor([0.0, 0.0] if skip else [3.0 * (step + 1), 4.0], dtype=torch.float64, device=dev)
        before = (W.clone(), m.clone(), v.clone(), state.clone())
        k.adam_step(W, m, v, grad.to(dev), lr, stats, state)
        if skip:
            assert all(torch.equal(a, b) for a, b in zip(before, (W, m, v, state)))
            continue
        taken += 1
        loss_sum += 3.0 * (step + 1) / 4.0
        ref.grad = grad.clone()
        opt.step()
        err = float((W.cpu().double() - ref.detach().double()).abs().max())
        bound = 1e-12 * float(ref.detach().abs().max()) if acc == torch.float64 else 16 * EPS[acc] * lr * taken + 2 * EPS[acc] * float(ref.detach().abs().max())
        assert err <= bound, (acc, step, err, bound)
    print(f"adam {acc}: final max|W - W_torch| = {err:.3e} (bound {bound:.3e})")
    assert float(state[0]) == taken and abs(float(state[1]) - loss_sum) < 1e-9


# ---- 5 / 6. the reference's training run ------------------------------------------------------------------------
def _karate(tmp_path, gold, dtype):
    kk = load_golden("g2_karate_csr.npz")
    X = gold["X"].astype(np.float64 if dtype == "float64" else np.float32)
    root = write_data_root(tmp_path / "karate_train", kk["vertex_ids"], kk["edge_src"], kk["edge_dst"], X)
    return Graph(root, embedding_dim=int(X.shape[1]), dtype=dtype)


def _replay(gold):
    return [(gold["src"][i], gold["dst"][i], gold["linked"][i], gold["trial"][i]) for i in range(len(gold["src"]))]


def _teacher_forced(eng, gold, i):
    """dW of step i of the fixture from the recorded fp64 weights before that step (a fresh trainer: one step)."""
    tr = eng.similarity_trainer(torch.from_numpy(gold["W_before"][i]), float(gold["lr"]), int(gold["batch_size"]))
    tr.step(rows_of_vertices(eng, gold["src"][i]), rows_of_vertices(eng, gold["dst"][i]),
            torch.from_numpy(gold["linked"][i]).to(eng.device),
            (1.0 - torch.from_numpy(gold["trial"][i]).to(eng.device, eng.acc_dtype)))
    return tr


def test_golden_replay_f64(dev, tmp_path):
    """The whole recorded run in fp64: per-step dW, epoch losses and final W within 1e-9 of the reference's fp64 run."""
    gold = load_golden(GOLD)
    g = _karate(tmp_path, gold, "float64")
    d = 16
    sim = AsymmertricSimilarity(d).double()
    with torch.no_grad():
        sim.Phi_src.weight.copy_(torch.from_numpy(gold["W0"][:d]))
        sim.Phi_dst.weight.copy_(torch.from_numpy(gold["W0"][d:]))
    emb = Embedder(g, sim, torch.device("cuda"), lr=float(gold["lr"]), batch_size=int(gold["batch_size"]), verbose=False)
    losses = emb.update_similarity_measure(int(gold["epochs"]), replay=_replay(gold))
    print("losses", losses, "want", gold["losses_f64"].tolist())
    np.testing.assert_allclose(losses, gold["losses_f64"], rtol=1e-9, atol=1e-9)
    W = torch.cat([sim.Phi_src.weight, sim.Phi_dst.weight], 0).detach().numpy()
    assert np.abs(W - gold["W_final_f64"]).max() < 1e-9
    eng = g.engine()
    worst = 0.0
    for i in range(len(gold["src"])):
        tr = _teacher_forced(eng, gold, i)
        worst = max(worst, float((tr.dW.cpu().numpy() - gold["dW_f64"][i]).__abs__().max()))
    print(f"g14 fp64: max per-step |dW - dW_ref| = {worst:.3e}")
    assert worst < 1e-9


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_golden_teacher_forced_f32_bf16(dev, tmp_path, dtype):
    """Per step from the recorded fp64 weights: max|dW - dW_f64| <= max(derived bound of the gradient test, 4 x the
    reference's own fp32 error stored in the fixture).  bf16: Z is rounded to bf16 on both sides of the comparison."""
    gold = load_golden(GOLD)
    g = _karate(tmp_path, gold, dtype)
    eng = g.engine()
    d, B, eps = 16, int(gold["batch_size"]), EPS[torch.float32]
    yard = 4 * float(gold["grad_err_ref_f32"])
    Xr = torch.from_numpy(gold["X"])
    Z64 = (Xr.bfloat16() if dtype == "bfloat16" else Xr).double()
    worst = 0.0
    for i in range(len(gold["src"])):
        tr = _teacher_forced(eng, gold, i)
        got = tr.dW.cpu().double()
        src, dst = torch.from_numpy(gold["src"][i]), torch.from_numpy(gold["dst"][i])
        linked, mask = torch.from_numpy(gold["linked"][i]), torch.from_numpy(gold["linked"][i] ^ gold["trial"][i])
        assert torch.equal(tr.mask.cpu(), mask.to(torch.uint8)), i
        W64 = torch.from_numpy(gold["W_before"][i]).float().double()       # the weights as the card holds them
        if dtype == "float32":
            want = torch.from_numpy(gold["dW_f64"][i])
        else:
            want = _autograd_dW(Z64, src, dst, torch.from_numpy(gold["W_before"][i]), linked, mask) if mask.any() \
                else torch.zeros(2 * d, d, dtype=torch.float64)
        A64, B64 = Z64[src] @ W64[:d].T, Z64[dst] @ W64[d:].T
        _, _, _, _, _, g64 = _loss_reference(A64, B64, linked, torch.zeros(B, dtype=torch.float64), mask=mask)
        M = int(mask.sum())
        bound = _grad_bound(Z64, src, dst, W64, A64, B64, g64, M, B, d, eps, torch.arange(d))
        # rounding the fp64 weights to the card's fp32 moves dW by at most |d dW / d W| eps |W|: inside the yardstick
        err = (got - want).abs()
        worst = max(worst, float(err.max()))
        assert bool((err <= torch.clamp(bound, min=yard)).all()), (dtype, i, float(err.max()), yard, float(bound.max()))
    print(f"g14 {dtype}: max per-step |dW - dW_f64| = {worst:.3e}; 4 x grad_err_ref_f32 = {yard:.3e}")


# ---- 7. end to end ------------------------------------------------------------------------------------------------
def planted_two_blocks(V=4096, d=32, p_in=0.012, p_out=0.0005, held_out=4096, seed=0):
    """A two-block stochastic block model with block-dependent content (+-mu plus noise); `held_out` of its edges are
    kept out of the graph for the ranking test, with as many non-edges."""
    rng = np.random.default_rng(seed)
    block = np.arange(V) % 2
    same = block[:, None] == block[None, :]
    adj = rng.random((V, V)) < np.where(same, p_in, p_out)
    np.fill_diagonal(adj, False)
    es, ed = np.nonzero(adj)
    hold = rng.choice(es.size, size=held_out, replace=False)
    keep = np.ones(es.size, dtype=bool)
    keep[hold] = False
    neg = []
    while len(neg) < held_out:
        a, b = rng.integers(V, size=2)
        if a != b and not adj[a, b]:
            neg.append((a, b))
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(es[keep], minlength=V), out=rowptr[1:])
    csr = HostCSR(V, rowptr, ed[keep].astype(np.int32))
    mu = rng.standard_normal(d) / math.sqrt(d) * 2.0
    X = (np.where(block[:, None] == 0, 1.0, -1.0) * mu + 0.5 * rng.standard_normal((V, d))).astype(np.float32)
    return csr, torch.from_numpy(X), (es[hold], ed[hold]), tuple(np.array(neg).T)


def auc(pos, neg):
    """Share of (edge, non-edge) pairs that the score ranks the right way round."""
    order = torch.cat([pos, neg]).argsort()
    ranks = torch.empty_like(order, dtype=torch.float64)
    ranks[order] = torch.arange(1, order.numel() + 1, dtype=torch.float64)
    return float((ranks[:pos.numel()].sum() - pos.numel() * (pos.numel() + 1) / 2) / (pos.numel() * neg.numel()))


def run_alternating(device, kernels=None, seed=5):
    csr, X, pos, neg = planted_two_blocks()
    g = Graph.from_csr(csr, X)
    if kernels is not None:
        g._attach_engine(SweepEngine(g.csr, g.X, "cpu", kernels))
    torch.manual_seed(1)
    sim = AsymmertricSimilarity(X.shape[1])
    W0 = sim.stacked_weight(torch.float64, "cpu").clone()
    emb = AlternatingEmbedder(g, sim, device, gamma=0.5, tolerence=1, tolerence_Z=3, tolerence_P=2, epoch=3,
                              batch_size=64, lr=1e-2, seed=seed, positive_fraction=0.5, verbose=False, max_rounds=2)
    emb.iterate()
    Z = g.Z.double()
    W = sim.stacked_weight(torch.float64, "cpu")
    d = X.shape[1]

    def score(Wm, pairs):
        s, t = (torch.from_numpy(np.asarray(p)) for p in pairs)
        return ((Z[s] @ Wm[:d].T) * (Z[t] @ Wm[d:].T)).sum(1)
    return emb, W, g.Z, auc(score(W, pos), score(W, neg)), auc(score(W0, pos), score(W0, neg))


def test_alternating_embedder_end_to_end(dev):
    """The mean training loss of the last epoch is below that of the first; on 4096 held-out edges against 4096 non-edges
    the trained score ranks edges above non-edges more often than the untrained Xavier weights; two runs with one seed
    give the same bits."""
    emb, W, Z, auc_trained, auc_xavier = run_alternating(torch.device("cuda"))
    first, last = emb.train_losses[0][0][0], emb.train_losses[-1][-1][-1]
    print(f"end to end: loss first epoch {first:.4f} last epoch {last:.4f}; AUC trained {auc_trained:.4f} "
          f"xavier {auc_xavier:.4f}; rounds {len(emb.train_losses)} sweeps {emb.sweep_counts}")
    assert last < first
    assert auc_trained > auc_xavier
    _, W2, Z2, _, _ = run_alternating(torch.device("cuda"))
    assert torch.equal(W, W2) and torch.equal(Z, Z2)
