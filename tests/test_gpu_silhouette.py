"""The silhouette on the card (csrc/silhouette.h, cluster.Silhouette): the n x K sums of distances to the bit on integer
data, within a bound derived beforehand on float data, the two properties the header promises (identical rows at distance
exactly 0; sums in an order that is a function of the segments alone), and the surface above it."""
import functools
import json
import types

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.cluster import Silhouette, silhouette_reference
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR

from .conftest import GOLDEN, load_golden, write_data_root
from .silhouette_cases import SHAPES, SIZES, cosine64, euclidean64, finish, gathered, partition, sums_of, table_case

pytestmark = pytest.mark.gpu

EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}      # unit roundoff of the accumulate type
DTYPES = [torch.float32, torch.bfloat16, torch.float64]
METRICS = ["euclidean", "cosine"]


def _dev():
    return _hip.require_gpu("cuda:0")


def _padded(values, dtype, dev, pad=3):
    buf = torch.zeros(values.shape[0], values.shape[1] + pad, dtype=dtype, device=dev)
    buf[:, :values.shape[1]] = values.to(dtype).to(dev)
    return buf[:, :values.shape[1]]                     # leading dimension d + pad


def _scorer(d, metric="euclidean", block_rows=None):
    """A Silhouette over any table of width d: it asks its engine for the kernels, the width and the one-GPU rule only."""
    eng = types.SimpleNamespace(k=_hip.kernels(), d=d, world=1, columns=None, halo=None, exchange=None)
    return Silhouette(eng, metric=metric, block_rows=block_rows)


def _shifted(Z, rows, mu, acc):
    """float64 [n, d]: a = Z[rows] - mu as the operand loaders form it -- ONE subtraction in the accumulate type."""
    return (gathered(Z.cpu().to(acc), rows.cpu()).to(acc) - mu.cpu().to(acc)).double()


# ---- integer data: exact --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _integer_run(shape, dtype):
    n, d, K = shape
    dev = _dev()
    acc = _hip.acc_dtype(dtype)
    Zv, rows, mu = table_case(shape, integers=True)
    part = partition(shape)
    with torch.cuda.device(dev):
        Z = _padded(Zv, dtype, dev)
        res = _scorer(d).samples(Z, rows.to(dev), part.to(dev), k=K, mu=mu, keep_sums=True)
        torch.cuda.synchronize()
    A = _shifted(Z, rows, mu, acc).numpy()              # integers: exact in every dtype
    D2 = ((A[:, None, :] - A[None, :, :]) ** 2).sum(-1)
    assert float(D2.max()) < 2 ** 24 and np.array_equal(D2, np.rint(D2))        # exact in fp32
    return dict(res=res, A=A, D2=D2, part=part.numpy(), S=res.sums.cpu().numpy(), s=res.samples.cpu().numpy())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_sums_are_exact_on_integer_data(shape, dtype):
    r = _integer_run(shape, dtype)
    n, d, K = shape
    if dtype == torch.float64:
        # the distances are correctly rounded doubles; their sum is not exact: one roundoff per addition of a cluster
        dist = np.sqrt(r["D2"])
        want = sums_of(dist, r["part"], K)
        bound = max(SIZES[shape]) * EPS[torch.float64] * want
        print(f"{shape} f64: max |S - float64| / bound = {np.max(np.abs(r['S'] - want) / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(np.abs(r["S"] - want) <= bound)
    else:
        # squared distances exact in fp32, a correctly rounded fp32 square root, and double sums of at most 2^10 fp32
        # values within a factor 2^6 of each other: exact in ANY order -- so equal to the bit
        dist = np.sqrt(r["D2"].astype(np.float32)).astype(np.float64)
        want = sums_of(dist, r["part"], K)
        print(f"{shape} {dtype}: S differs from numpy in {int((r['S'] != want).sum())} of {want.size} places")
        assert np.array_equal(r["S"], want)
    want_s = finish(r["S"], r["part"])                  # the float64 finish of the very sums the kernel left
    print(f"{shape} {dtype}: max |s - finish(S)| = {np.abs(r['s'] - want_s).max():.2e}")
    assert np.abs(r["s"] - want_s).max() <= 1e-15
    res = r["res"]
    assert res.sizes.tolist() == SIZES[shape]
    per = res.per_cluster.cpu().numpy()
    for c in range(K):
        rows_c = r["s"][r["part"] == c]
        assert (np.isnan(per[c]) and rows_c.size == 0) or abs(per[c] - rows_c.mean()) <= 1e-14
    assert abs(res.mean - r["s"].mean()) <= 1e-14


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_integer_data_against_scikit_learn(shape, dtype):
    """One roundoff per distance (the fp32 square root; everything before it and the sums after it are exact): relative
    2^-24 on a and on b, so at most 4 * 2^-24 on s = (b - a) / max(a, b) with |s| <= 1 -- asserted whatever is observed."""
    metrics = pytest.importorskip("sklearn.metrics")
    r = _integer_run(shape, dtype)
    want = metrics.silhouette_samples(r["A"], r["part"], metric="euclidean")
    err = np.abs(r["s"] - want).max()
    print(f"{shape} {dtype}: max |s - sklearn| = {err / 2.0 ** -24:.3f} * 2^-24")
    assert err <= 4 * 2.0 ** -24


# ---- float data: within the a-priori bound ----------------------------------------------------------------------------
def _pair_bound(A, D, d, eps, metric):
    """Per pair, what rounding can do to a distance, from the formats alone.
    euclidean: the Gram form sq_i + sq_j - 2 dot is off by at most 2 (d + 2) eps (|a_i| + |a_j|)^2 (d-term fp32 chains of
    the three dots, the addition and the fma); a square root turns an error e of D^2 into at most min(sqrt(e), e / D) and
    adds its own eps D.
    cosine: the dot is off by (d + 2) eps |a_i| |a_j|, each r = 1 / sqrt(sq) by ((d + 2) / 2 + 2) eps relatively, the two
    products and the subtraction by eps each; |cos| <= 1: (2 d + 12) eps in all."""
    if metric == "cosine":
        return np.full_like(D, (2 * d + 12) * eps)
    nr = np.sqrt((A * A).sum(1))
    e = 2 * (d + 2) * eps * (nr[:, None] + nr[None, :]) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.minimum(np.sqrt(e), np.where(D > 0, e / D, np.inf)) + eps * D


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_float_data_against_the_reference(shape, dtype, metric):
    n, d, K = shape
    dev = _dev()
    acc = _hip.acc_dtype(dtype)
    Zv, rows, mu = table_case(shape, integers=False)
    part = partition(shape)
    with torch.cuda.device(dev):
        Z = _padded(Zv, dtype, dev)
        kw = dict(mu=mu) if metric == "euclidean" else {}
        res = _scorer(d, metric).samples(Z, rows.to(dev), part.to(dev), k=K, keep_sums=True, **kw)
        torch.cuda.synchronize()
    A = _shifted(Z, rows, mu if metric == "euclidean" else torch.zeros(d), acc).numpy()
    D = euclidean64(A) if metric == "euclidean" else cosine64(A)
    p = part.numpy()
    S_ref = sums_of(D, p, K)
    B = sums_of(_pair_bound(A, D, d, EPS[acc], metric), p, K) + max(SIZES[shape]) * 2.0 ** -53 * S_ref
    S = res.sums.cpu().numpy()
    ratio = np.abs(S - S_ref) / np.maximum(B, 1e-300)
    print(f"{shape} {dtype} {metric}: max |S - float64| / bound = {ratio.max():.4f}")
    assert np.all(np.abs(S - S_ref) <= B)
    # s = (b - a) / max(a, b): an error of a and of b moves it by at most (|da| + |db|) / max(a, b)
    cnt = np.bincount(p, minlength=K).astype(np.float64)
    own = cnt[p]
    a = S_ref[np.arange(n), p] / np.maximum(own - 1, 1)
    da = B[np.arange(n), p] / np.maximum(own - 1, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        means = np.where(cnt > 0, S_ref / cnt, np.inf)
        dmeans = np.where(cnt > 0, B / cnt, 0.0)
    means[np.arange(n), p] = np.inf
    b, db = means.min(1), dmeans.max(1)
    bound_s = np.where(own > 1, 1.01 * (da + db) / np.maximum(np.maximum(a, b) - da - db, 1e-300), 0.0) + 1e-15
    want = silhouette_reference(torch.from_numpy(A), part, metric).numpy()
    got = res.samples.cpu().numpy()
    print(f"{shape} {dtype} {metric}: max |s - reference| / bound = {(np.abs(got - want) / bound_s).max():.4f}, "
          f"max |s - reference| = {np.abs(got - want).max():.2e}")
    assert np.all(np.abs(got - want) <= bound_s)


# ---- the two properties -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_rows_of_the_same_bits_are_at_distance_zero(dtype):
    """Float data; cluster 0 is 130 positions (two column tiles) that all hold the bits of ONE row -- through the same
    table row and through a second table row of the same bits.  A Gram-trick distance with the squared norm from another
    chain leaves ~sqrt(d eps) |a| between them; here it is exactly 0, so the sums do not see where a copy sits."""
    dev = _dev()
    d, copies, others = 37, 130, 150
    gen = torch.Generator().manual_seed(4)
    Zv = torch.randn(others + 2, d, generator=gen, dtype=torch.float64) * 3 + 1
    Zv[1] = Zv[0]                                           # table rows 0 and 1: the same bits
    rows = torch.cat([torch.arange(2).repeat(copies // 2), 2 + torch.arange(others)]).to(torch.int32)
    part = torch.cat([torch.zeros(copies, dtype=torch.int64), 1 + torch.arange(others) % 2])
    perm = torch.randperm(copies + others, generator=gen)
    rows, part = rows[perm], part[perm]
    mu = Zv.mean(0)                                         # not an integer shift: a = z - mu is rounded
    with torch.cuda.device(dev):
        Z = _padded(Zv, dtype, dev)
        res = _scorer(d).samples(Z, rows.to(dev), part.to(dev), k=3, mu=mu, keep_sums=True)
        torch.cuda.synchronize()
    S, s = res.sums.cpu(), res.samples.cpu()
    inside = part == 0
    assert bool((S[inside, 0] == 0.0).all())                # every copy is at distance exactly 0 from every other
    assert bool((s[inside] == 1.0).all())                   # a = 0 < b
    assert bool((S[inside] == S[inside][0]).all())          # the copies see the other clusters alike, to the bit
    # a row outside sees 130 times ONE distance: the sum of 130 equal fp32 (fp64: one rounding per addition) values
    one = S[~inside, 0] / copies
    acc = _hip.acc_dtype(dtype)
    A = _shifted(Z, rows, mu, acc).numpy()
    want = euclidean64(A)[~inside.numpy()][:, np.flatnonzero(inside.numpy())[0]]
    assert np.all(np.abs(one.numpy() - want) <= _pair_bound(A, euclidean64(A), d, EPS[acc], "euclidean")
                  [~inside.numpy()][:, np.flatnonzero(inside.numpy())[0]] + copies * 2.0 ** -53 * want)
    if acc == torch.float32:
        assert bool((one.float().double() == one).all())    # 130 x is exact in double for an fp32 x


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_blocks_and_calls_give_the_same_bits(dtype, metric):
    shape = (600, 17, 6)
    n, d, K = shape
    dev = _dev()
    Zv, rows, mu = table_case(shape, integers=False)
    part = partition(shape)
    with torch.cuda.device(dev):
        Z = _padded(Zv, dtype, dev)
        runs = []
        for block in (None, 128, 256, n, 128):
            sc = _scorer(d, metric, block_rows=block)
            res = sc.samples(Z, rows.to(dev), part.to(dev), k=K, keep_sums=True)
            runs.append((res.sums.cpu(), res.samples.cpu(), res.per_cluster.cpu(), res.mean, dict(sc.passes)))
        torch.cuda.synchronize()
    assert [r[4]["sums"] for r in runs] == [1, 5, 3, 1, 5] and all(r[4]["norms"] == 1 for r in runs)
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1])
        assert torch.equal(r[2].nan_to_num(7.0), runs[0][2].nan_to_num(7.0))       # an empty cluster's mean is NaN
        assert r[3] == runs[0][3]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_cluster_ids_and_row_order_do_not_matter(dtype):
    """Integer data, where every sum is exact (fp64: the sums of a cluster are taken in the order of the rows, so the
    comparison allows their roundoff): renaming the clusters permutes the columns of S and leaves s alone; reordering the
    rows reorders s with them."""
    shape = (300, 130, 17)
    n, d, K = shape
    base = _integer_run(shape, dtype)
    dev = _dev()
    Zv, rows, mu = table_case(shape, integers=True)
    part = partition(shape)
    gen = torch.Generator().manual_seed(9)
    rename, shuffle = torch.randperm(K, generator=gen), torch.randperm(n, generator=gen)
    with torch.cuda.device(dev):
        Z = _padded(Zv, dtype, dev)
        renamed = _scorer(d).samples(Z, rows.to(dev), rename[part].to(dev), k=K, mu=mu, keep_sums=True)
        moved = _scorer(d).samples(Z, rows[shuffle].to(dev), part[shuffle].to(dev), k=K, mu=mu, keep_sums=True)
        torch.cuda.synchronize()
    tol = 0.0 if dtype != torch.float64 else max(SIZES[shape]) * 2.0 ** -53
    S, s = torch.from_numpy(base["S"]), torch.from_numpy(base["s"])

    def same(x, y):
        return bool(((x - y).abs() <= tol * y.abs()).all())
    assert same(renamed.sums.cpu()[:, rename], S) and renamed.sizes.cpu()[rename].tolist() == SIZES[shape]
    assert same(moved.sums.cpu(), S[shuffle])
    assert bool(((renamed.samples.cpu() - s).abs() <= 4 * tol).all())
    assert bool(((moved.samples.cpu() - s[shuffle]).abs() <= 4 * tol).all())


def test_refusals():
    dev = _dev()
    with torch.cuda.device(dev):
        Z = torch.zeros(8, 4, device=dev)
        rows = torch.arange(6, dtype=torch.int32, device=dev)
        sc = _scorer(4)
        with pytest.raises(ValueError, match="two non-empty"):
            sc.samples(Z, rows, torch.zeros(6, dtype=torch.int64))
        with pytest.raises(ValueError, match="one cluster per row"):
            sc.samples(Z, rows, torch.zeros(5, dtype=torch.int64))
        with pytest.raises(ValueError, match=r"clusters must be in \[0, 2\)"):
            sc.samples(Z, rows, torch.tensor([0, 1, 2, 0, 1, 2]), k=2)
        with pytest.raises(ValueError, match="integers"):
            sc.samples(Z, rows, torch.tensor([0.0, 1, 1, 0, 1, 1]))
        with pytest.raises(ValueError, match="belongs to the euclidean"):
            _scorer(4, "cosine").samples(Z, rows, torch.tensor([0, 1, 1, 0, 1, 1]), mu=torch.zeros(4))
    with pytest.raises(ValueError, match="metric"):
        _scorer(4, "manhattan")
    with pytest.raises(ValueError, match="block_rows"):
        _scorer(4, block_rows=0)
    several = types.SimpleNamespace(k=None, d=4, world=2, columns=None, halo=None, exchange="ring")
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        Silhouette(several)


# ---- the surface ----------------------------------------------------------------------------------------------------
def _ring(V):
    return HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + 1) % V).astype(np.int32))


def test_a_list_of_cluster_counts_finds_three_blobs():
    rng = np.random.default_rng(3)
    centres = np.array([[6.0] + [0.0] * 7, [0.0, 6.0] + [0.0] * 6, [0.0, 0.0, 6.0] + [0.0] * 5])
    truth = np.arange(300) % 3
    X = torch.from_numpy((centres[truth] + 0.5 * rng.standard_normal((300, 8))).astype(np.float32))
    g = Graph.from_csr(_ring(300), X)
    out = g.cluster(k=[2, 3, 4, 5], restarts=4, seed=1, table="X", return_assignments=True)
    sel = out["selection"]
    print("candidates:", [(c["clusters"], round(c["silhouette"], 4)) for c in sel["candidates"]])
    assert sel["chosen"] == 3 and out["clusters"] == 3 and sel["criterion"] == "silhouette"
    assert [c["clusters"] for c in sel["candidates"]] == [2, 3, 4, 5]
    assert sorted(out["sizes"]) == [100, 100, 100] and len(out["assignments"]) == 300
    inertia = [c["inertia"] for c in sel["candidates"]]
    assert inertia == sorted(inertia, reverse=True)                 # inertia only falls: it cannot choose
    # the chosen entry is the scored fit of k = 3 alone, and its scores are scikit-learn's on the same partition
    alone = g.cluster(k=3, restarts=4, seed=1, table="X", silhouette=True, return_assignments=True)
    assert alone == {key: v for key, v in out.items() if key != "selection"}
    plain = g.cluster(k=3, restarts=4, seed=1, table="X", return_assignments=True)
    assert plain == {key: v for key, v in alone.items() if key in plain} and "silhouette" not in plain
    metrics = pytest.importorskip("sklearn.metrics")
    a = np.asarray(out["assignments"])
    Xd = X.double().numpy()
    assert abs(out["silhouette"] - metrics.silhouette_score(Xd, a)) <= 1e-5
    assert abs(out["calinski_harabasz"] / metrics.calinski_harabasz_score(Xd, a) - 1) <= 1e-5
    assert abs(out["davies_bouldin"] - metrics.davies_bouldin_score(Xd, a)) <= 1e-5
    assert len(out["silhouette_per_cluster"]) == 3 and out["silhouette_scored"] == 300
    # a sample: the same vertices for every candidate, seeded
    sampled = g.cluster(k=[2, 3], restarts=2, seed=1, table="X", silhouette_points=100)
    assert sampled["silhouette_scored"] == 100 and sampled["clusters"] == 3
    direct = g.silhouette(partition=a, table="X")
    assert direct["n"] == 300 and not direct["sampled"] and direct["sizes"] == out["sizes"]
    assert direct["mean"] == out["silhouette"] and direct["per_cluster"] == out["silhouette_per_cluster"]
    part = g.silhouette(partition=a, table="X", max_points=120, seed=5)
    assert part["n"] == 120 and part["sampled"] and sum(part["sizes"]) == 120 and part["mean"] > 0.5
    with pytest.raises(ValueError, match="one of the two"):
        g.silhouette()
    with pytest.raises(ValueError, match="one cluster per vertex"):
        g.silhouette(partition=a[:10])


def test_silhouette_of_the_true_classes_on_karate(tmp_path):
    from clane_amd.classify import read_labels
    kar = load_golden("g2_karate_csr.npz")
    X = np.random.default_rng(0).standard_normal((34, 4)).astype(np.float32)
    root = write_data_root(tmp_path / "karate", kar["vertex_ids"], kar["edge_src"], kar["edge_dst"], X)
    g = Graph(data_root=root, embedding_dim=4)
    vertices, y, names = read_labels(GOLDEN / "g2_karate_Y.tsv", g.vertex_ids)
    for metric in METRICS:
        out = g.silhouette(labels=GOLDEN / "g2_karate_Y.tsv", metric=metric)
        assert out["clusters"] == [str(c) for c in names] and out["n"] == len(vertices) and not out["sampled"]
        assert out["metric"] == metric and out["table"] == "Z"
        assert out["sizes"] == np.bincount(np.asarray(y), minlength=len(names)).tolist() and -1.0 <= out["mean"] <= 1.0
        Z = g.engine().get_Z()[torch.as_tensor(vertices, dtype=torch.int64), :4]
        want = silhouette_reference(Z, torch.as_tensor(y), metric)
        print(f"karate {metric}: mean silhouette of the true classes {out['mean']:.4f}")
        assert abs(out["mean"] - float(want.mean())) <= 1e-5
    with pytest.raises(ValueError, match="one class per labelled vertex"):
        g.silhouette(labels=([0, 1, 2], ["a", "b"]))


CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")
TODAY = {"inertia", "iterations", "converged", "empty", "best_restart", "sizes"}     # a table's keys without labels


def test_cli_section_writes_the_selection(tmp_path, capsys):
    import clane_amd.__main__ as M
    _dev()
    kar = load_golden("g2_karate_csr.npz")
    X = np.random.default_rng(0).standard_normal((34, 4)).astype(np.float32)
    root = write_data_root(tmp_path / "karate", kar["vertex_ids"], kar["edge_src"], kar["edge_dst"], X)

    def run(section, out):
        cfg = tmp_path / f"{out}.yaml"
        cfg.write_text(CONFIG + section)
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg), "--gpu"]))
        capsys.readouterr()
        return json.loads((tmp_path / out / "cluster_metrics.json").read_text())
    got = run("\nnode_clustering:\n  clusters: [2, 3, 4]\n  restarts: 3\n  assignments: true\n  silhouette_metric: cosine\n",
              "listed")
    t = got["tables"]["Z"]
    sel = t["selection"]
    assert [c["clusters"] for c in sel["candidates"]] == [2, 3, 4] and sel["criterion"] == "silhouette"
    best = max(sel["candidates"], key=lambda c: (c["silhouette"], -c["clusters"]))
    assert sel["chosen"] == best["clusters"] == got["clusters"] and t["silhouette"] == best["silhouette"]
    assert set(t) == TODAY | {"selection", "silhouette", "silhouette_per_cluster", "calinski_harabasz", "davies_bouldin",
                              "silhouette_metric", "silhouette_scored"}
    assert t["silhouette_metric"] == "cosine" and len(t["sizes"]) == sel["chosen"]
    rows = (tmp_path / "listed" / "clusters.tsv").read_text().splitlines()
    assert len(rows) == 34 and {int(r.split("\t")[1]) for r in rows} <= set(range(sel["chosen"]))
    # without the new keys: today's keys only
    plain = run("\nnode_clustering:\n  clusters: 3\n  restarts: 3\n", "plain")
    assert set(plain) == {"labels", "clustered", "class_names", "clusters", "restarts", "seed", "tables"}
    assert set(plain["tables"]) == {"Z"} and set(plain["tables"]["Z"]) == TODAY
