"""Node clustering, the parts that need no GPU: NMI / ARI / purity against hand-computed answers (and scikit-learn where
it is installed), the contingency counts, the two kernels of csrc/kmeans.h restated in torch as a KernelBackend subclass
and the host logic driven by it -- seeding, the Lloyd loop against a plain loop, the refusals -- the ABI's new symbols
and their argument checks, and the validation of the CLI section."""
import ctypes as C
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.engine import SweepEngine
from clane_amd.partition import HostCSR

from .oracle_kernels import OracleKernels

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ([f"clane_kmeans_{w}_{s}" for w in ("assign", "update") for s in ("f32", "f64", "bf16")]
               + ["clane_kmeans_update_ws_len"])


class KMeansOracleKernels(OracleKernels):
    """kmeans_assign / kmeans_update of csrc/kmeans.h in torch (the same formulas, no attempt at the same rounding)."""

    def __init__(self):
        super().__init__()
        self.assign_calls = []

    @staticmethod
    def _gathered(Z, d, rows, dtype):
        r = rows.long()
        inside = (r >= 0) & (r < Z.shape[0])
        return Z[r.clamp(0, Z.shape[0] - 1), :d].to(dtype) * inside[:, None].to(dtype)

    def kmeans_assign(self, Z, d, rows, centres, csq, assign, best):
        self.assign_calls.append(centres.clone())
        Zg = self._gathered(Z, d, rows, centres.dtype)
        for r in range(centres.shape[0]):                   # restart by restart: a restart's bits do not depend on the others
            val = csq[r][None, :] - 2.0 * (Zg @ centres[r].T)
            low = val.amin(1)
            best[:, r] = low
            assign[:, r] = (val == low[:, None]).int().argmax(1).to(torch.int32)     # the first of the minima

    def kmeans_update_ws_len(self, n, R, K, d):
        return 1

    def kmeans_update(self, Z, d, order, seg, centres_old, ws, centres_new, csq_new):
        R, K, _ = centres_old.shape
        for s in range(R * K):
            a, b = int(seg[s]), int(seg[s + 1])
            r, j = divmod(s, K)
            if b > a:
                centres_new[r, j] = self._gathered(Z, d, order[a:b], centres_old.dtype).sum(0) / (b - a)
            else:
                centres_new[r, j] = centres_old[r, j]
        csq_new.copy_((centres_new * centres_new).sum(2))


def _engine(X, kernels=None):
    V = X.shape[0]
    csr = HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + 1) % V).astype(np.int32))
    return SweepEngine(csr, X, "cpu", kernels if kernels is not None else KMeansOracleKernels())


def _planted(n, d, C_, sep, seed):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C_, n)
    y[:C_] = np.arange(C_)
    X = rng.standard_normal((C_, d))[y] * sep + rng.standard_normal((n, d))
    return torch.from_numpy(X), torch.from_numpy(y)


# ---- metrics ----------------------------------------------------------------------------------------------------
def test_scores_of_identical_and_relabelled_partitions():
    from clane_amd.cluster import clustering_scores
    same = torch.tensor([[3, 0, 0], [0, 4, 0], [0, 0, 2]])
    relabelled = same[:, [2, 0, 1]]
    for table in (same, relabelled):
        nmi, ari, purity = clustering_scores(table)
        assert float(nmi) == pytest.approx(1.0, abs=1e-15) and float(ari) == 1.0 and float(purity) == 1.0
    nmi, ari, purity = clustering_scores(torch.stack([same, relabelled]))      # batched over a leading restart dimension
    assert nmi.shape == (2,) and ari.tolist() == [1.0, 1.0] and purity.tolist() == [1.0, 1.0]


def test_scores_of_an_independent_table():
    """nij = ai bj / N: the mutual information is 0.  The ARI of the finite table [[m, m], [m, m]] is not exactly 0 but
    (s - e) / (max - e) with s = 2 m (m - 1) joined pairs, max = 2 m (2 m - 1) and e = max^2 / C(4 m, 2), which is
    -1 / (2 (2 m - 1)): -1/6 at m = 2, and 0 in the limit."""
    from clane_amd.cluster import clustering_scores
    for m in (2, 5, 500_000):
        nmi, ari, purity = clustering_scores(torch.full((2, 2), m))
        assert abs(float(nmi)) <= 1e-15 and float(purity) == 0.5
        assert float(ari) == pytest.approx(-1.0 / (2 * (2 * m - 1)), rel=1e-9)
    assert abs(float(ari)) < 1e-6


def test_scores_of_a_worked_table():
    from clane_amd.cluster import clustering_scores
    table = [[5, 1, 0],
             [1, 4, 1],
             [0, 2, 6]]
    # classes 6, 6, 8; clusters 6, 7, 7; N = 20
    N, a, b = 20, (6, 6, 8), (6, 7, 7)
    mi = sum(table[i][j] / N * math.log(N * table[i][j] / (a[i] * b[j])) for i in range(3) for j in range(3) if table[i][j])
    h_classes = -sum(x / N * math.log(x / N) for x in a)
    h_clusters = -sum(x / N * math.log(x / N) for x in b)
    assert mi == pytest.approx(0.47569593939500193, abs=1e-15)
    assert h_classes == pytest.approx(1.0888999753452238, abs=1e-15) and h_clusters == pytest.approx(1.0960673284468554, abs=1e-15)
    # pairs joined in a cell: C(5,2) + C(4,2) + C(6,2) + C(2,2) = 10 + 6 + 15 + 1 = 32; by class 15 + 15 + 28 = 58; by
    # cluster 15 + 21 + 21 = 57; expected 58 * 57 / C(20, 2) = 3306 / 190
    expected = 58 * 57 / 190
    want_ari = (32 - expected) / ((58 + 57) / 2 - expected)
    nmi, ari, purity = clustering_scores(torch.tensor(table))
    assert float(nmi) == pytest.approx(0.4354261398506209, abs=1e-14)
    assert float(nmi) == pytest.approx(mi / ((h_classes + h_clusters) / 2), abs=1e-14)
    assert float(ari) == pytest.approx(0.3640897755610973, abs=1e-14) and float(ari) == pytest.approx(want_ari, abs=1e-14)
    assert float(purity) == (5 + 4 + 6) / 20


def test_scores_of_degenerate_tables():
    from clane_amd.cluster import clustering_scores
    one = torch.zeros(3, 3, dtype=torch.int64)
    one[1, 2] = 7                                           # one class, one cluster (the others empty)
    single = torch.tensor([[1]])
    split = torch.tensor([[2, 3], [0, 0]])                  # one class cut into two clusters
    merged = torch.tensor([[2], [3]])                       # two classes in one cluster
    nmi, ari, purity = clustering_scores(one)
    assert (float(nmi), float(ari), float(purity)) == (1.0, 1.0, 1.0)
    nmi, ari, purity = clustering_scores(single)
    assert (float(nmi), float(ari), float(purity)) == (1.0, 1.0, 1.0)
    nmi, ari, purity = clustering_scores(split)
    assert (float(nmi), float(ari), float(purity)) == (0.0, 0.0, 1.0)
    nmi, ari, purity = clustering_scores(merged)
    assert (float(nmi), float(ari), float(purity)) == (0.0, 0.0, 0.6)


def test_scores_against_scikit_learn():
    metrics = pytest.importorskip("sklearn.metrics")
    from clane_amd.cluster import clustering_scores, contingency
    rng = np.random.default_rng(0)
    for case in range(50):
        n, Cn, k = int(rng.integers(1, 200)), int(rng.integers(1, 8)), int(rng.integers(1, 8))
        y, a = rng.integers(0, Cn, n), rng.integers(0, k, n)
        nmi, ari, _ = clustering_scores(contingency(torch.from_numpy(y), torch.from_numpy(a), Cn, k))
        assert float(nmi) == pytest.approx(metrics.normalized_mutual_info_score(y, a), abs=1e-12), case
        assert float(ari) == pytest.approx(metrics.adjusted_rand_score(y, a), abs=1e-12), case


def test_contingency_against_a_loop():
    from clane_amd.cluster import contingency
    gen = torch.Generator().manual_seed(0)
    n, Cn, k, R = 97, 4, 5, 3
    y = torch.randint(0, Cn, (n,), generator=gen)
    assign = torch.randint(0, k, (n, R), generator=gen).to(torch.int32)
    want = torch.zeros(R, Cn, k, dtype=torch.int64)
    for i in range(n):
        for r in range(R):
            want[r, y[i], assign[i, r]] += 1
    got = contingency(y, assign, Cn, k)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert torch.equal(contingency(y, assign[:, 1], Cn, k), want[1])
    assert int(got.sum()) == n * R


# ---- the loop on the test double --------------------------------------------------------------------------------
def test_first_centre_of_a_restart_depends_on_its_seed_alone():
    from clane_amd.cluster import KMeans
    X, _ = _planted(80, 4, 3, 2.0, seed=0)
    eng = _engine(X)
    rows = eng.pos[torch.arange(80)].to(torch.int32)

    def first_centres(restarts, seed):
        eng.k.assign_calls.clear()
        KMeans(eng, max_iter=0).fit(eng.Zcur, rows, 3, restarts=restarts, seed=seed)
        return eng.k.assign_calls[0][:, 0]                  # the seeding's first call: the R first centres, K = 1
    a, b, c = first_centres(4, 5), first_centres(2, 6), first_centres(1, 8)
    assert a.shape == (4, 4)
    assert torch.equal(a[1:3], b) and torch.equal(a[3:4], c)                  # restart r of seed s = restart 0 of s + r
    for r in range(4):
        want = int(torch.randint(80, (1,), generator=torch.Generator().manual_seed(5 + r)))
        assert torch.equal(a[r], X[want])
    # and so does everything that follows: a restart's fit is the one-restart fit of its seed
    km = KMeans(eng)
    fit4 = km.fit(eng.Zcur, rows, 3, restarts=4, seed=5)
    assert km.passes["assign"] >= 3 and km.passes["update"] >= 1
    for r in range(4):
        one = KMeans(eng).fit(eng.Zcur, rows, 3, restarts=1, seed=5 + r)
        assert torch.equal(one.assign[:, 0], fit4.assign[:, r]) and torch.equal(one.centres[0], fit4.centres[r])
        assert float(one.inertia[0]) == float(fit4.inertia[r]) and int(one.iterations[0]) == int(fit4.iterations[r])
    assert fit4.best_restart == int(torch.argmin(fit4.inertia))


def test_seeding_never_repeats_a_row_and_spreads_over_the_clusters():
    from clane_amd.cluster import KMeans
    X, _ = _planted(60, 3, 4, 6.0, seed=1)
    eng = _engine(X)
    rows = eng.pos[torch.arange(60)].to(torch.int32)
    km = KMeans(eng)
    zsq = (X * X).sum(1)
    centres, picks = km.seed_centres(eng.Zcur, rows, zsq, 12, 5, seed=3)
    assert tuple(centres.shape) == (5, 12, 3) and tuple(picks.shape) == (5, 12)
    for r in range(5):
        assert len(set(picks[r].tolist())) == 12
        assert torch.equal(centres[r], X[picks[r]])
    # more centres than distinct rows: the draw falls back to a uniform one instead of failing
    same = _engine(torch.ones(6, 2, dtype=torch.float64))
    fit = KMeans(same).fit(same.Zcur, same.pos[torch.arange(6)].to(torch.int32), 3, restarts=2, seed=0)
    assert fit.empty.tolist() == [2, 2] and bool(fit.converged.all()) and fit.inertia.tolist() == [0.0, 0.0]


def _lloyd(X, init, max_iter=300):
    """A plain Lloyd loop in float64: (assignments, centres, updates made, converged)."""
    centres = init.clone()
    nearest = lambda c: ((X[:, None, :] - c[None, :, :]) ** 2).sum(2).argmin(1)     # noqa: E731
    assign = nearest(centres)
    for it in range(1, max_iter + 1):
        for j in range(centres.shape[0]):
            if bool((assign == j).any()):
                centres[j] = X[assign == j].mean(0)
        new = nearest(centres)
        if torch.equal(new, assign):
            return assign, centres, it, True
        assign = new
    return assign, centres, max_iter, False


def test_fit_follows_a_plain_lloyd_loop():
    from clane_amd.cluster import KMeans
    n, d, k = 300, 5, 3
    X, _ = _planted(n, d, k, 3.0, seed=0)
    eng = _engine(X)
    rows = eng.pos[torch.arange(n)].to(torch.int32)
    init = torch.stack([X[torch.randperm(n, generator=torch.Generator().manual_seed(s))[:k]] for s in (0, 1)])
    fit = KMeans(eng).fit(eng.Zcur, rows, k, init=init)
    for r in range(2):
        assign, centres, updates, converged = _lloyd(X, init[r])
        assert converged and bool(fit.converged[r]) and int(fit.iterations[r]) == updates
        assert torch.equal(fit.assign[:, r].long(), assign)
        assert float((fit.centres[r] - centres).abs().max()) <= 1e-12
        inertia = float(((X - centres[assign]) ** 2).sum())
        assert float(fit.inertia[r]) == pytest.approx(inertia, rel=1e-12)
    assert fit.empty.tolist() == [0, 0]
    # max_iter cuts the loop short and says so
    short = KMeans(eng, max_iter=1).fit(eng.Zcur, rows, k, init=init)
    assert short.iterations.tolist() == [1, 1] and not bool(short.converged.any())
    # an empty cluster keeps its centre and is counted
    far = init.clone()
    far[0, 2] = 1e6
    lonely = KMeans(eng).fit(eng.Zcur, rows, k, init=far)
    assert lonely.empty.tolist() == [1, 0] and torch.equal(lonely.centres[0, 2], far[0, 2])


def test_evaluate_and_refusals():
    from clane_amd.cluster import KMeans
    n, d, Cn = 90, 4, 3
    X, y = _planted(n, d, Cn, 8.0, seed=2)
    eng = _engine(X)
    km = KMeans(eng)
    verts = list(range(0, n, 2))
    out = km.evaluate(verts, y=y[verts].tolist(), restarts=3, seed=1)
    assert set(out) == {"table", "clustered", "clusters", "restarts", "seed", "inertia", "iterations", "converged", "empty",
                        "best_restart", "sizes", "nmi", "ari", "purity", "per_restart"}
    assert out["clustered"] == 45 and out["clusters"] == Cn and sum(out["sizes"]) == 45 and out["converged"]
    assert set(out["per_restart"]) == {"inertia", "nmi", "ari", "iterations"}
    assert out["inertia"] == min(out["per_restart"]["inertia"])
    assert out["nmi"] == pytest.approx(1.0, abs=1e-12) and out["ari"] == 1.0 and out["purity"] == 1.0     # far apart
    plain = km.evaluate(verts, k=4, restarts=2)
    assert "nmi" not in plain and plain["clusters"] == 4 and len(plain["sizes"]) == 4
    with pytest.raises(ValueError, match="give k"):
        km.evaluate(verts)
    with pytest.raises(ValueError, match="one class per clustered vertex"):
        km.evaluate(verts, y=[0, 1])
    with pytest.raises(ValueError, match=r"init must be \[R, k = 3, d = 4\]"):
        km.fit(eng.Zcur, eng.pos[:5].to(torch.int32), 3, init=torch.zeros(2, 3, 5))
    with pytest.raises(NotImplementedError, match="OracleKernels has no kmeans_assign"):
        KMeans(_engine(X, OracleKernels())).evaluate(verts, k=2)
    eng.world = 2
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        KMeans(eng)


# ---- the ABI ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "clane_hip.h").read_text(), flags=re.S)
    lib = _hip.load_library()
    assert len(NEW_SYMBOLS) == 7
    for name in NEW_SYMBOLS:
        decl = re.search(rf"\b(?:int|int64_t) {name}\s*\(([^;]*)\);", header)
        assert decl and name in _hip.SIGNATURES, name
        assert len(_hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
        assert getattr(lib, name) is not None
    assert re.search(r"#define CLANE_ABI_VERSION 5\b", header) and lib.clane_abi_version() == 5
    # two chunk sums of d elements per window of 2048 positions of the sorted list of R n rows
    assert lib.clane_kmeans_update_ws_len(1, 1, 1, 1) == 2 and lib.clane_kmeans_update_ws_len(2048, 1, 9, 5) == 10
    assert lib.clane_kmeans_update_ws_len(2049, 3, 9, 16) == 2 * 4 * 16
    for name in ("kmeans_assign", "kmeans_update", "kmeans_update_ws_len"):
        assert callable(getattr(_hip.HipKernels, name))


def test_argument_validation_reaches_last_error():
    lib = _hip.load_library()                   # refused on the host before any launch: safe without a GPU
    p = C.cast((C.c_float * 64)(), C.c_void_p)

    def assign(fn=lib.clane_kmeans_assign_f32, d=4, ldz=4, n=2, R=2, K=3, out=p, best=p, ld_assign=2, ld_best=2, Z=p):
        return fn(Z, 8, d, ldz, p, n, p, p, R, K, out, ld_assign, best, ld_best, None)
    for bad, text in ((dict(d=0), b"bad shape"), (dict(ldz=3), b"bad shape"), (dict(n=-1), b"bad shape"),
                      (dict(K=0), b"K must be"), (dict(R=0), b"R must be"), (dict(R=65536), b"R must be"),
                      (dict(ld_assign=1), b"ld_assign"), (dict(ld_best=1), b"ld_best"), (dict(out=None), b"null output"),
                      (dict(best=None), b"null output"), (dict(Z=None), b"null pointer")):
        assert assign(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"kmeans_assign" in lib.clane_last_error()
    assert assign(fn=lib.clane_kmeans_assign_bf16, K=-1) == -1 and assign(fn=lib.clane_kmeans_assign_f64, d=-1) == -1

    def update(fn=lib.clane_kmeans_update_f32, d=4, ldz=4, n=2, R=2, K=3, ws=p, new=p, csq=p, seg=p, order=p):
        return fn(p, 8, d, ldz, order, seg, n, R, K, p, ws, new, csq, None)
    for bad, text in ((dict(d=0), b"bad shape"), (dict(ldz=2), b"bad shape"), (dict(n=-1), b"bad shape"),
                      (dict(K=0), b"K must be"), (dict(R=0), b"R must be"), (dict(R=1 << 20, K=1 << 20), b"too many centres"),
                      (dict(ws=None), b"null workspace"), (dict(new=None), b"null workspace"),
                      (dict(csq=None), b"null workspace"), (dict(seg=None), b"null pointer"),
                      (dict(order=None), b"null pointer")):
        assert update(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"kmeans_update" in lib.clane_last_error()
    assert update(fn=lib.clane_kmeans_update_bf16, K=-2) == -1 and update(fn=lib.clane_kmeans_update_f64, d=0) == -1


# ---- the CLI section --------------------------------------------------------------------------------------------
CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


def test_node_clustering_is_refused_on_several_gpus_before_the_graph_is_loaded(monkeypatch, tmp_path):
    import clane_amd.__main__ as M
    monkeypatch.setenv("WORLD_SIZE", "2")

    def touched(*a, **k):
        raise AssertionError("the run went on to set up devices")
    monkeypatch.setattr(M, "_distributed_setup", touched)
    monkeypatch.setattr(M, "Graph", touched)
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG + "\nnode_clustering:\n  clusters: 3\n")
    args = M.get_parser().parse_args(["--data_root", str(tmp_path), "--output_root", str(tmp_path / "o"),
                                      "--config_file", str(cfg)])
    with pytest.raises(NotImplementedError, match="node_clustering runs on one GPU"):
        M.embedding(args)
    monkeypatch.setenv("WORLD_SIZE", "1")
    for section in ("node_clustering:\n  restarts: 3\n", "node_clustering: 7\n"):
        cfg.write_text(CONFIG + "\n" + section)
        with pytest.raises(ValueError, match="node_clustering"):        # neither labels nor clusters
            M.embedding(args)
    for section in ("node_clustering:\n  clusters: 3\n", "node_clustering:\n  labels: Y\n"):
        cfg.write_text(CONFIG + "\n" + section)
        with pytest.raises(AssertionError, match="went on"):            # a valid section passes the validation
            M.embedding(args)
    assert set(vars(M.get_parser().parse_args([]))) == {                # no new flag
        "command", "data_root", "output_root", "config_file", "save_history", "num_workers", "init_Z", "exchange",
        "train_similarity", "predict_links", "link_sources", "gpu"}


def test_a_config_without_the_section_never_imports_the_module(tmp_path, monkeypatch, capsys):
    import clane_amd.__main__ as M
    from clane_amd.graph import Graph
    from .conftest import GOLDEN, load_golden, write_data_root
    k = load_golden("g2_karate_csr.npz")
    X = np.random.default_rng(0).standard_normal((34, 4)).astype(np.float32)
    root = write_data_root(tmp_path / "karate", k["vertex_ids"], k["edge_src"], k["edge_dst"], X)
    (root / "Y").write_text((GOLDEN / "g2_karate_Y.tsv").read_text())

    def cpu_engine(self, device=None, cosine_mode="reference", **kw):
        if self._engine is None:
            self._attach_engine(SweepEngine(self.csr, self.X, "cpu", KMeansOracleKernels(), cosine_mode=cosine_mode))
        return self._engine
    monkeypatch.setattr(Graph, "engine", cpu_engine)

    def run(cfg_text, out):
        cfg = tmp_path / f"{out}.yaml"
        cfg.write_text(cfg_text)
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg)]))
        return capsys.readouterr().out
    monkeypatch.delitem(sys.modules, "clane_amd.cluster", raising=False)
    plain = run(CONFIG, "plain")
    assert "clane_amd.cluster" not in sys.modules
    assert not (tmp_path / "plain" / "cluster_metrics.json").exists() and not (tmp_path / "plain" / "clusters.tsv").exists()
    # the section, on the test double: the same Z, the same lines before its own
    import json
    with_section = run(CONFIG + "\nnode_clustering:\n  labels: Y\n  restarts: 3\n  seed: 1\n  baseline: true\n"
                                "  assignments: true\n", "clu")
    assert "clane_amd.cluster" in sys.modules
    assert np.array_equal(np.load(tmp_path / "plain" / "Z.npy"), np.load(tmp_path / "clu" / "Z.npy"))
    strip = lambda text, out: text.replace(str(tmp_path / out), "O")     # noqa: E731
    lines, base = strip(with_section, "clu").splitlines(), strip(plain, "plain").splitlines()
    assert lines[:len(base)] == base and len(lines) == len(base) + 1 and "34 vertices into" in lines[-1]
    got = json.loads((tmp_path / "clu" / "cluster_metrics.json").read_text())
    assert set(got) == {"labels", "clustered", "class_names", "clusters", "restarts", "seed", "tables"}
    assert got["clustered"] == 34 and got["restarts"] == 3 and got["seed"] == 1 and got["clusters"] == len(got["class_names"])
    assert set(got["tables"]) == {"Z", "X"}
    for t in got["tables"].values():
        assert set(t) == {"inertia", "iterations", "converged", "empty", "best_restart", "sizes", "nmi", "ari", "purity",
                          "per_restart"}
        assert 0.0 <= t["nmi"] <= 1.0 and -1.0 <= t["ari"] <= 1.0 and 0.0 < t["purity"] <= 1.0 and sum(t["sizes"]) == 34
    rows = (tmp_path / "clu" / "clusters.tsv").read_text().splitlines()
    assert len(rows) == 34 and all(len(r.split("\t")) == 2 for r in rows)
    ids = [str(i) for i in k["vertex_ids"]]
    assert sorted(r.split("\t")[0] for r in rows) == sorted(ids)
