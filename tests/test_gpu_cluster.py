"""Node clustering on the GPU: clane_kmeans_assign_* / clane_kmeans_update_* (csrc/kmeans.h) against float64 within
a-priori bounds, the tie rule and exactness on integer data, bit-reproducibility, the Lloyd loop of cluster.KMeans against
an independent float64 loop on the CPU, restarts, and the surface (Graph.cluster, the CLI section).  Every test prints its
figures (error / bound, margins, iterations) before it asserts: run with -s to see them.

Bound of one value csq_j - 2 z . c_j in the accumulate type (unit roundoff eps): b = 2 d eps (2 |z| . |c_j| + |csq_j|), the
dot's d-term bound on the absolute values, doubled."""
import functools
import json

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.cluster import KMeans
from clane_amd.embedder import Embedder
from clane_amd.engine import SweepEngine
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR
from clane_amd.similarity import CosineSimilarity

from .conftest import GOLDEN, load_golden, write_data_root

pytestmark = pytest.mark.gpu

EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}      # unit roundoff of the accumulate type
DTYPES = [torch.float32, torch.bfloat16, torch.float64]
ASSIGN_SHAPES = [(1, 1, 1, 1), (127, 5, 3, 3), (129, 16, 7, 2), (5000, 130, 17, 3), (300, 256, 129, 2), (129, 256, 300, 1),
                 (5000, 16, 1, 1)]                                  # (n, d, K, R)
UPDATE_SHAPES = [(1, 1, 1), (2, 5, 5), (3, 17, 130), (1, 4, 256)]  # (R, K, d)
SEGMENT_SIZES = [2049, 10000, 0, 2047, 1, 2]                       # around the 2048-row chunk, empty, and tiny
LOOP_CASES = [((300, 5, 3, 3.0), 0), ((300, 5, 3, 3.0), 1), ((300, 5, 3, 3.0), 2), ((600, 16, 7, 2.0), 1),
              ((600, 16, 7, 2.0), 2), ((1000, 130, 17, 1.0), 0), ((1000, 130, 17, 1.0), 1), ((1000, 130, 17, 1.0), 2)]


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


def _gathered64(Z, rows, table_rows):
    r = rows.long()
    return Z.double()[r.clamp(max=table_rows - 1)] * (r < table_rows)[:, None]


# ---- assignment -------------------------------------------------------------------------------------------------
def _assign_case(n, d, K, R, dtype, dev, integers=False):
    gen = torch.Generator().manual_seed(1000 * n + 10 * d + K + R)
    acc = _hip.acc_dtype(dtype)
    table_rows = max(3, n // 2)                         # rows repeat
    if integers:
        Zv = torch.randint(-2, 3, (table_rows, d), generator=gen).double()
        centres = torch.randint(-1, 2, (R, K, d), generator=gen).double()
        if K > 131:
            centres[:, 131] = centres[:, 3]             # the same centre in two column tiles ...
        if K > 7:
            centres[:, 7] = centres[:, 3]               # ... and twice in one
    else:
        Zv = torch.randn(table_rows, d, generator=gen, dtype=torch.float64)
        centres = torch.randn(R, K, d, generator=gen, dtype=torch.float64)
    Z = _padded(Zv, dtype, dev)
    rows = torch.randint(0, table_rows, (n,), generator=gen).to(torch.int32)
    rows[n // 2] = table_rows                           # one index past the table: a zero row
    centres = centres.to(acc).to(dev)
    csq = (centres.double() ** 2).sum(2).to(acc)
    return dict(Z=Z, rows=rows.to(dev), centres=centres, csq=csq, n=n, d=d, K=K, R=R, acc=acc, table_rows=table_rows)


def _run_assign(k, c, dev):
    assign = torch.full((c["n"], c["R"] + 1), -7, dtype=torch.int32, device=dev)
    best = torch.full((c["n"], c["R"] + 2), float("nan"), dtype=c["acc"], device=dev)
    k.kmeans_assign(c["Z"], c["d"], c["rows"], c["centres"], c["csq"], assign[:, :c["R"]], best[:, :c["R"]])
    torch.cuda.synchronize()
    return assign, best


def _values64(c):
    """float64 values [n, R, K] of what the kernel reads, and the bound b per value."""
    Zg = _gathered64(c["Z"], c["rows"], c["table_rows"])
    c64, q64 = c["centres"].double(), c["csq"].double()
    val = q64[None] - 2.0 * torch.einsum("nd,rkd->nrk", Zg, c64)
    b = 2 * c["d"] * EPS[c["acc"]] * (2.0 * torch.einsum("nd,rkd->nrk", Zg.abs(), c64.abs()) + q64.abs()[None])
    return val, b


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", ASSIGN_SHAPES, ids=str)
def test_assign_against_float64(k, dev, dtype, shape):
    n, d, K, R = shape
    c = _assign_case(n, d, K, R, dtype, dev)
    assign, best = _run_assign(k, c, dev)
    val, b = _values64(c)
    bmax = b.amax(2)
    low = val.amin(2)
    got = assign[:, :R].long()
    assert bool(((got >= 0) & (got < K)).all())
    err = (best[:, :R].double() - low).abs()
    chosen = val.gather(2, got[:, :, None])[:, :, 0]
    b_chosen = b.gather(2, got[:, :, None])[:, :, 0]
    print(f"assign {shape} {dtype}: max |best - min64| / (2 max b) = {float((err / (2 * bmax)).max()):.3f}, "
          f"max (chosen - min64) / (2 b) = {float(((chosen - low) / (2 * b_chosen)).max()):.3f}")
    assert bool((err <= 2 * bmax).all())
    assert bool((chosen - low <= 2 * b_chosen).all())
    if K > 1:
        top2 = val.topk(2, 2, largest=False).values
        clear = (top2[:, :, 1] - top2[:, :, 0]) > 2 * bmax
    else:
        clear = torch.ones_like(low, dtype=torch.bool)
    print(f"assign {shape} {dtype}: {int(clear.sum())} of {clear.numel()} rows have a margin above 2 b")
    assert bool(clear.any())
    assert torch.equal(got[clear], val.argmin(2)[clear])
    assert bool((assign[:, R] == -7).all()) and bool(torch.isnan(best[:, R:]).all())     # nothing written past column R
    assign2, best2 = _run_assign(k, c, dev)
    assert torch.equal(assign, assign2) and torch.equal(best[:, :R], best2[:, :R])


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(300, 4, 140, 2), (129, 5, 7, 3), (200, 3, 129, 1)], ids=str)
def test_assign_ties_go_to_the_lowest_centre(k, dev, dtype, shape):
    n, d, K, R = shape
    c = _assign_case(n, d, K, R, dtype, dev, integers=True)             # integer values: exact in every dtype, many ties
    if K > 131:
        assert torch.equal(c["centres"][:, 131], c["centres"][:, 3]) and torch.equal(c["centres"][:, 7], c["centres"][:, 3])
    assign, best = _run_assign(k, c, dev)
    val, _ = _values64(c)
    low = val.amin(2, keepdim=True)
    idx = torch.arange(K, device=dev).expand_as(val)
    lowest = torch.where(val == low, idx, torch.full_like(idx, K)).amin(2)
    tied = ((val == low).sum(2) > 1)
    print(f"ties {shape} {dtype}: {int(tied.sum())} of {tied.numel()} (row, restart) pairs tie at the minimum")
    assert int(tied.any(1).sum()) > n // 4                              # the case does hold ties
    assert torch.equal(assign[:, :R].long(), lowest)
    assert torch.equal(best[:, :R].double(), low[:, :, 0])


# ---- update -----------------------------------------------------------------------------------------------------
def _update_case(R, K, d, dtype, dev, integers=False):
    gen = torch.Generator().manual_seed(100 * R + 10 * K + d)
    acc = _hip.acc_dtype(dtype)
    start = UPDATE_SHAPES.index((R, K, d))
    sizes = [[SEGMENT_SIZES[(start + r + j) % len(SEGMENT_SIZES)] for j in range(K)] for r in range(R)]
    n = max(sum(s) for s in sizes)
    for s in sizes:
        s[-1] += n - sum(s)                             # every restart lists n rows
    table_rows = 1000
    if integers:
        Zv = torch.randint(-4, 5, (table_rows, d), generator=gen).double()
    else:
        Zv = torch.randn(table_rows, d, generator=gen, dtype=torch.float64)
    Z = _padded(Zv, dtype, dev, pad=8)                  # d = 256: 16-byte packs; the others element by element
    order = torch.randint(0, table_rows, (R * n,), generator=gen).to(torch.int32)
    order[n // 2] = table_rows                          # one index past the table: a zero row that counts
    seg = torch.tensor([0] + [x for s in sizes for x in s], dtype=torch.int64).cumsum(0)
    old = torch.randn(R, K, d, generator=gen, dtype=torch.float64).to(acc)
    return dict(Z=Z, order=order.to(dev), seg=seg.to(dev), old=old.to(dev), sizes=sizes, n=n, R=R, K=K, d=d, acc=acc,
                table_rows=table_rows)


def _run_update(k, c, dev):
    R, K, d = c["R"], c["K"], c["d"]
    ws = torch.full((k.kmeans_update_ws_len(c["n"], R, K, d),), float("nan"), dtype=c["acc"], device=dev)
    new = torch.full((R, K, d), float("nan"), dtype=c["acc"], device=dev)
    csq = torch.full((R, K), float("nan"), dtype=c["acc"], device=dev)
    k.kmeans_update(c["Z"], d, c["order"], c["seg"], c["old"], ws, new, csq)
    torch.cuda.synchronize()
    return new, csq


def _segments64(c):
    """Per segment: (float64 sum, float64 sum of |z|, count)."""
    Zg = _gathered64(c["Z"], c["order"], c["table_rows"])
    seg = c["seg"].tolist()
    out = []
    for s in range(c["R"] * c["K"]):
        part = Zg[seg[s]:seg[s + 1]]
        out.append((part.sum(0), part.abs().sum(0), seg[s + 1] - seg[s]))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", UPDATE_SHAPES, ids=str)
def test_update_against_float64(k, dev, dtype, shape):
    R, K, d = shape
    c = _update_case(R, K, d, dtype, dev)
    new, csq = _run_update(k, c, dev)
    eps = EPS[c["acc"]]
    worst = 0.0
    for s, (total, total_abs, count) in enumerate(_segments64(c)):
        got = new.view(R * K, d)[s]
        if count == 0:
            assert torch.equal(got, c["old"].view(R * K, d)[s])         # the old centre's bits
            continue
        tol = 2 * count * eps * (total_abs / count)
        err = (got.double() - total / count).abs()
        worst = max(worst, float((err / tol.clamp(min=1e-300)).max()))
        assert bool((err <= tol).all()), (s, count)
    sq64 = (new.double() ** 2).sum(2)
    sq_err = (csq.double() - sq64).abs()
    print(f"update {shape} {dtype}: segments {c['sizes']}, max error / bound {worst:.3f}, "
          f"csq {float((sq_err / (2 * d * eps * sq64).clamp(min=1e-300)).max()):.3f}")
    assert bool((sq_err <= 2 * d * eps * sq64).all())                   # d squares and d - 1 additions, doubled
    new2, csq2 = _run_update(k, c, dev)
    assert torch.equal(new, new2) and torch.equal(csq, csq2)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", UPDATE_SHAPES, ids=str)
def test_update_is_exact_on_integer_data(k, dev, dtype, shape):
    R, K, d = shape                                     # |Z| <= 4: every sum below 4 * 33000 < 2^24
    c = _update_case(R, K, d, dtype, dev, integers=True)
    new, _ = _run_update(k, c, dev)
    for s, (total, _, count) in enumerate(_segments64(c)):
        if count:
            want = total.cpu().to(c["acc"]) / count     # one IEEE division of the exact sum, made on the host
            assert torch.equal(new.view(R * K, d)[s].cpu(), want), (s, count)


# ---- the loop ---------------------------------------------------------------------------------------------------
def _planted(n, d, Cn, sep, seed=0):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, Cn, n)
    y[:Cn] = np.arange(Cn)
    X = rng.standard_normal((Cn, d))[y] * sep + rng.standard_normal((n, d))
    return torch.from_numpy(X), torch.from_numpy(y)


@functools.lru_cache(maxsize=None)
def _reference(shape, seed, rounded):
    """An independent Lloyd loop on the CPU in float64 from the rows randperm(n, seed)[:K]; ``rounded``: on the
    bf16-rounded table.  Returns (X, init, assign, centres, updates, converged, smallest top-two margin of the whole
    trajectory, largest bound b of the trajectory for the f32 accumulators).  Computed once per case and shared."""
    n, d, K, sep = shape
    X, _ = _planted(n, d, K, sep, seed)
    if rounded:
        X = X.to(torch.bfloat16).double()
    init = X[torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:K]].clone()
    centres, margin, bound = init.clone(), float("inf"), 0.0

    def nearest(c):
        nonlocal margin, bound
        csq = (c * c).sum(1)
        val = csq[None, :] - 2.0 * X @ c.T
        top2 = val.topk(2, 1, largest=False).values
        margin = min(margin, float((top2[:, 1] - top2[:, 0]).min()))
        bound = max(bound, float((2 * d * EPS[torch.float32] * (2.0 * X.abs() @ c.abs().T + csq[None, :])).max()))
        return val.argmin(1)
    assign = nearest(centres)
    updates, converged = 0, False
    while updates < 300:
        for j in range(K):
            mine = assign == j
            if bool(mine.any()):
                centres[j] = X[mine].sum(0) / int(mine.sum())
        new = nearest(centres)
        updates += 1
        if torch.equal(new, assign):
            converged = True
            break
        assign = new
    return X, init, assign, centres, updates, converged, margin, bound


def _ring_engine(X, dtype, dev):
    V = X.shape[0]
    csr = HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + 1) % V).astype(np.int32))
    return SweepEngine(csr, X.to(dtype), dev)


def _fit(X, dtype, dev, K, **kw):
    with torch.cuda.device(dev):
        eng = _ring_engine(X, dtype, dev)
        rows = eng.pos[torch.arange(X.shape[0], device=dev)].to(torch.int32)
        km = KMeans(eng, max_iter=kw.pop("max_iter", 300))
        return km.fit(eng.Zcur, rows, K, **kw), km


@pytest.mark.parametrize("case", LOOP_CASES, ids=str)
def test_loop_float64_follows_an_independent_lloyd(dev, case):
    shape, seed = case
    n, d, K, _ = shape
    X, init, assign, centres, updates, converged, margin, _ = _reference(shape, seed, False)
    print(f"loop {case}: reference {updates} updates, converged {converged}, smallest top-two margin {margin:.3e}, "
          f"sizes {torch.bincount(assign, minlength=K).tolist()}")
    assert converged and margin > 1e-6                  # a property of the reference alone
    fit, _ = _fit(X, torch.float64, dev, K, init=init[None])
    assert torch.equal(fit.assign[:, 0].cpu().long(), assign)
    assert int(fit.iterations[0]) == updates and bool(fit.converged[0]) and int(fit.empty[0]) == 0
    assert float((fit.centres[0].cpu() - centres).abs().max()) <= 1e-12
    inertia = float(((X - centres[assign]) ** 2).sum())
    print(f"loop {case}: inertia {float(fit.inertia[0])!r} reference {inertia!r}")
    assert abs(float(fit.inertia[0]) - inertia) <= 1e-12 * inertia


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("case", LOOP_CASES, ids=str)
def test_loop_float32_and_bfloat16_reach_a_fixed_point(dev, dtype, case):
    shape, seed = case
    n, d, K, _ = shape
    X, init, ref_assign, _, _, _, margin, ref_bound = _reference(shape, seed, dtype == torch.bfloat16)
    fit, _ = _fit(X, dtype, dev, K, init=init[None])
    eps = EPS[torch.float32]
    assign = fit.assign[:, 0].cpu().long()
    c64 = fit.centres[0].cpu().double()
    print(f"loop {case} {dtype}: {int(fit.iterations[0])} updates, converged {bool(fit.converged[0])}")
    assert bool(fit.converged[0])
    for j in range(K):                                  # every centre is the mean of its rows
        mine = X[assign == j]
        if mine.shape[0]:
            tol = 2 * mine.shape[0] * eps * mine.abs().mean(0)
            assert bool(((c64[j] - mine.mean(0)).abs() <= tol).all()), j
    csq = (c64 * c64).sum(1)
    val = csq[None, :] - 2.0 * X @ c64.T
    b = 2 * d * eps * (2.0 * X.abs() @ c64.abs().T + csq[None, :])
    chosen, b_chosen = val.gather(1, assign[:, None])[:, 0], b.gather(1, assign[:, None])[:, 0]
    print(f"  max (chosen - nearest) / (2 b) = {float(((chosen - val.amin(1)) / (2 * b_chosen)).max()):.3f}")
    assert bool((chosen - val.amin(1) <= 2 * b_chosen).all())
    inertia = float(((X - c64[assign]) ** 2).sum())
    print(f"  inertia {float(fit.inertia[0])!r}, float64 of its own assignment {inertia!r}, bound {n * float(b.max()):.3e}")
    assert abs(float(fit.inertia[0]) - inertia) <= n * float(b.max())
    if shape == (300, 5, 3, 3.0):
        print(f"  reference margin {margin:.3e}, 4 b = {4 * ref_bound:.3e}")
        assert margin > 4 * ref_bound                   # from the reference alone: the trajectories cannot part
        assert torch.equal(assign, ref_assign)


def test_restarts_and_idempotence(dev):
    n, d, K = 600, 16, 7
    X, _ = _planted(n, d, K, 2.0, 1)
    for dtype in (torch.float32, torch.float64):
        with torch.cuda.device(dev):
            eng = _ring_engine(X, dtype, dev)
            rows = eng.pos[torch.arange(n, device=dev)].to(torch.int32)
            km = KMeans(eng)
            fit = km.fit(eng.Zcur, rows, K, restarts=4, seed=3)
            print(f"restarts {dtype}: iterations {fit.iterations.tolist()} inertia {fit.inertia.tolist()} passes {km.passes}")
            assert bool(fit.converged.all())
            assert fit.best_restart == int(torch.argmin(fit.inertia))
            assert len(set(fit.iterations.tolist())) > 1 or int(fit.iterations.max()) > 1
            for r in range(4):                          # restart r is the one-restart fit seeded seed + r, bit for bit
                one = KMeans(eng).fit(eng.Zcur, rows, K, restarts=1, seed=3 + r)
                assert torch.equal(one.assign[:, 0], fit.assign[:, r]) and torch.equal(one.centres[0], fit.centres[r])
                assert torch.equal(one.inertia[0], fit.inertia[r]) and torch.equal(one.iterations[0], fit.iterations[r])
            # beyond convergence nothing moves: a fit started from the fixed point makes one update and changes no bit
            again = KMeans(eng, max_iter=5).fit(eng.Zcur, rows, K, init=fit.centres)
            assert again.iterations.tolist() == [1] * 4 and bool(again.converged.all())
            assert torch.equal(again.centres, fit.centres) and torch.equal(again.assign, fit.assign)
            assert torch.equal(again.inertia, fit.inertia)
            zsq = (eng.Zcur[rows.long(), :d].double() ** 2).sum(1)
            _, picks = km.seed_centres(eng.Zcur, rows, zsq, 40, 4, seed=3)
            assert all(len(set(p)) == 40 for p in picks.tolist())       # no drawn initial centre repeats a row


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


def test_cluster_end_to_end(dev):
    csr, X, block = _two_blocks()
    g = Graph.from_csr(csr, X)
    Embedder(g, CosineSimilarity(), dev, tolerence=3, verbose=False).iterate()
    names = ["even" if b == 0 else "odd" for b in block]
    outZ = g.cluster(labels=names, restarts=3, seed=2)
    print(f"end to end: nmi {outZ['nmi']:.3f} ari {outZ['ari']:.3f} purity {outZ['purity']:.3f} sizes {outZ['sizes']}")
    assert outZ["class_names"] == ["even", "odd"] and outZ["clusters"] == 2 and outZ["clustered"] == 120
    assert 0.0 <= outZ["nmi"] <= 1.0 and 0.0 <= outZ["ari"] <= 1.0 and 0.0 <= outZ["purity"] <= 1.0
    with torch.cuda.device(dev):
        other = SweepEngine(csr, g.engine().get_Z(), dev)
        direct = KMeans(other).evaluate(list(range(120)), y=block.tolist(), n_classes=2, restarts=3, seed=2)
        assert direct == {key: v for key, v in outZ.items() if key != "class_names"}
        outX = g.cluster(labels=names, restarts=3, seed=2, table="X")
        assert outX["inertia"] != outZ["inertia"] and outX["table"] == "X"
        plain = g.cluster(k=3, return_assignments=True)
        assert "nmi" not in plain and plain["clusters"] == 3 and len(plain["assignments"]) == 120
        assert plain["vertices"] == list(range(120)) and sum(plain["sizes"]) == 120
        with pytest.raises(ValueError, match="give k"):
            g.cluster()


CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


def test_cli_section_writes_cluster_metrics(dev, tmp_path, capsys):
    import clane_amd.__main__ as M
    kar = load_golden("g2_karate_csr.npz")
    X = np.random.default_rng(0).standard_normal((34, 4)).astype(np.float32)
    root = write_data_root(tmp_path / "karate", kar["vertex_ids"], kar["edge_src"], kar["edge_dst"], X)
    (root / "Y").write_text((GOLDEN / "g2_karate_Y.tsv").read_text())

    def run(text, out):
        cfg = tmp_path / f"{out}.yaml"
        cfg.write_text(text)
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg), "--gpu"]))
        return capsys.readouterr().out.replace(str(tmp_path / out), "O").splitlines()
    base = run(CONFIG, "plain")
    assert (tmp_path / "plain" / "Z.npy").exists()
    assert not (tmp_path / "plain" / "cluster_metrics.json").exists() and not (tmp_path / "plain" / "clusters.tsv").exists()
    lines = run(CONFIG + "\nnode_clustering:\n  labels: Y\n  restarts: 4\n  seed: 1\n  baseline: true\n  assignments: true\n",
                "clu")
    assert lines[:len(base)] == base and len(lines) == len(base) + 1    # the same stdout, and one line more
    assert np.array_equal(np.load(tmp_path / "plain" / "Z.npy"), np.load(tmp_path / "clu" / "Z.npy"))
    got = json.loads((tmp_path / "clu" / "cluster_metrics.json").read_text())
    assert set(got["tables"]) == {"Z", "X"} and got["clustered"] == 34 and got["clusters"] == len(got["class_names"]) >= 2
    for t in got["tables"].values():
        assert 0.0 <= t["nmi"] <= 1.0 and 0.0 < t["purity"] <= 1.0 and sum(t["sizes"]) == 34 and len(t["per_restart"]["nmi"]) == 4
    rows = (tmp_path / "clu" / "clusters.tsv").read_text().splitlines()
    assert len(rows) == 34 and all(0 <= int(r.split("\t")[1]) < got["clusters"] for r in rows)
    run(CONFIG + "\nnode_clustering:\n  clusters: 3\n", "k_only")       # no labels: nothing to score against
    only = json.loads((tmp_path / "k_only" / "cluster_metrics.json").read_text())
    assert set(only["tables"]) == {"Z"} and "nmi" not in only["tables"]["Z"] and only["class_names"] is None
    assert not (tmp_path / "k_only" / "clusters.tsv").exists()
