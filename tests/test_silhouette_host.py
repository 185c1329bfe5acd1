"""Scoring a clustering without labels, the host side: the float64 restatement of the silhouette and the two
centre-based indices against scikit-learn, the selection of k, the new keys of the node_clustering section and the ABI's
new entries.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.cluster import (calinski_harabasz, check_cluster_counts, check_section, davies_bouldin, dense_partition,
                               select_clusters, silhouette_finish, silhouette_reference)

from .silhouette_cases import SHAPES, cosine64, euclidean64, finish, partition, sums_of

ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-12
NEW_SYMBOLS = [f"clane_silhouette_{what}_{s}" for what in ("norms", "sums") for s in ("f32", "f64", "bf16")]


def _dyadic(n, d, seed):
    """Rows on a grid of eighths: sums of squares and dots are exact in float64, so scikit-learn's Gram-trick distances
    carry no cancellation error of their own -- duplicated rows included."""
    return np.random.default_rng(seed).integers(-16, 17, (n, d)).astype(np.float64) / 8.0


def _cases():
    X = _dyadic(40, 3, 0)
    yield "plain", X, np.arange(40) % 3
    yield "singleton", X, np.r_[np.zeros(20, int), np.ones(19, int), [2]]
    yield "an empty id", X, np.where(np.arange(40) % 3 == 1, 5, np.arange(40) % 3)     # ids 0, 2, 5: 1, 3, 4 own nothing
    D = X.copy()
    D[7], D[30], D[31] = D[3], D[3], D[8]                                              # copies within and across clusters
    yield "duplicated points", D, np.arange(40) % 4
    yield "every row of a cluster the same", np.r_[np.tile(X[:1], (5, 1)), X[5:]], np.r_[np.zeros(5, int), 1 + np.arange(35) % 2]
    Z = X.copy()
    Z[4] = 0.0
    Z[9] = 0.0                                                                         # zero rows: cosine distance 1
    yield "zero rows", Z, np.arange(40) % 3
    yield "gaussian", np.random.default_rng(5).standard_normal((60, 7)), np.arange(60) % 5


CASES = list(_cases())


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_against_scikit_learn(case, metric):
    metrics = pytest.importorskip("sklearn.metrics")
    _, X, part = case
    want = metrics.silhouette_samples(X, part, metric=metric)
    got = silhouette_reference(torch.from_numpy(X), torch.from_numpy(part), metric).numpy()
    print(f"max |s - sklearn| = {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= TOL
    # and the numpy restatement the GPU tests use says the same
    ids, own = dense_partition(torch.from_numpy(part))
    D = euclidean64(X) if metric == "euclidean" else cosine64(X)
    mine = finish(sums_of(D, own.numpy(), ids.numel()), own.numpy())
    assert np.abs(mine - want).max() <= TOL


def test_finish_handles_singletons_empty_clusters_and_zero_distances():
    S = torch.tensor([[0.0, 4.0, 0.0], [2.0, 6.0, 0.0], [2.0, 3.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]],
                     dtype=torch.float64)
    own = torch.tensor([0, 0, 0, 1, 0])
    sizes = torch.tensor([4, 1, 0])                                 # cluster 2 owns nothing: never the nearest
    s = silhouette_finish(S, own, sizes)
    a, b = [0.0, 2 / 3, 2 / 3], [4.0, 6.0, 3.0]
    want = [(b[i] - a[i]) / max(a[i], b[i]) for i in range(3)] + [0.0, 0.0]    # a singleton; a = b = 0
    assert torch.allclose(s, torch.tensor(want, dtype=torch.float64), rtol=0, atol=1e-15)
    assert np.allclose(finish(S.numpy(), own.numpy()), want, rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="two non-empty"):
        silhouette_reference(torch.zeros(4, 2), torch.tensor([3, 3, 3, 3]))
    with pytest.raises(ValueError, match="metric"):
        silhouette_reference(torch.zeros(4, 2), torch.tensor([0, 1, 0, 1]), "manhattan")
    with pytest.raises(ValueError, match="one integer per row"):
        dense_partition(torch.tensor([0.5, 1.0]))


def _centre_inputs(X, part, K):
    X, part = torch.from_numpy(X), torch.from_numpy(part)
    sizes = torch.bincount(part, minlength=K)
    centres = torch.full((K, X.shape[1]), 123.0, dtype=torch.float64)       # an empty centre holds anything: it is left out
    for c in range(K):
        if sizes[c]:
            centres[c] = X[part == c].mean(0)
    d2 = ((X - centres[part]) ** 2).sum(1)
    return centres, sizes, d2, part


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_centre_indices_against_scikit_learn(case):
    metrics = pytest.importorskip("sklearn.metrics")
    _, X, part = case
    centres, sizes, d2, p = _centre_inputs(X, part, int(part.max()) + 2)    # one more id than used: empty as well
    ch, db = calinski_harabasz(centres, sizes, d2), davies_bouldin(centres, sizes, d2.sqrt(), p)
    want_ch, want_db = metrics.calinski_harabasz_score(X, part), metrics.davies_bouldin_score(X, part)
    print(f"CH {ch:.12g} vs {want_ch:.12g}; DB {db:.12g} vs {want_db:.12g}")
    assert abs(ch - want_ch) <= TOL * max(1.0, abs(want_ch)) and abs(db - want_db) <= TOL * max(1.0, abs(want_db))


def test_centre_indices_of_degenerate_partitions():
    X = np.r_[np.zeros((3, 2)), np.ones((3, 2))]
    part = np.r_[np.zeros(3, int), np.ones(3, int)]
    centres, sizes, d2, p = _centre_inputs(X, part, 2)
    assert calinski_harabasz(centres, sizes, d2) == 1.0                     # no dispersion within: scikit-learn's 1.0
    assert davies_bouldin(centres, sizes, d2.sqrt(), p) == 0.0
    with pytest.raises(ValueError, match="non-empty"):
        calinski_harabasz(centres, torch.tensor([6, 0]), d2)
    with pytest.raises(ValueError, match="non-empty"):
        davies_bouldin(centres, torch.tensor([6, 0]), d2.sqrt(), torch.zeros(6, dtype=torch.int64))


# ---- choosing k ---------------------------------------------------------------------------------------------------
def _stub(scores, calls):
    def run(k):
        calls.append(k)
        return {"clusters": k, "inertia": 100.0 / k, "silhouette": scores[k], "calinski_harabasz": 10.0 * k,
                "davies_bouldin": 1.0 / k, "empty": 0, "sizes": [1] * k, "assignments": [k]}
    return run


def test_selection_takes_the_highest_silhouette_and_ties_go_to_the_smaller_k():
    calls = []
    out = select_clusters([2, 3, 4, 5], _stub({2: 0.3, 3: 0.7, 4: 0.5, 5: 0.1}, calls))
    assert calls == [2, 3, 4, 5]                                    # every candidate is fitted, in the order given
    assert out["clusters"] == 3 and out["assignments"] == [3] and out["selection"]["chosen"] == 3
    assert out["selection"]["criterion"] == "silhouette"
    assert [c["clusters"] for c in out["selection"]["candidates"]] == [2, 3, 4, 5]
    assert all(set(c) == {"clusters", "inertia", "silhouette", "calinski_harabasz", "davies_bouldin", "empty"}
               for c in out["selection"]["candidates"])
    assert out["selection"]["candidates"][2] == {"clusters": 4, "inertia": 25.0, "silhouette": 0.5,
                                                 "calinski_harabasz": 40.0, "davies_bouldin": 0.25, "empty": 0}
    # inertia falls with k and never decides; a tie goes to the smaller k whatever the order of the list
    assert select_clusters([5, 4, 2], _stub({2: 0.5, 4: 0.5, 5: 0.5}, []))["clusters"] == 2
    assert select_clusters([4, 2, 3], _stub({2: 0.1, 3: 0.6, 4: 0.6}, []))["clusters"] == 3
    # a candidate that could not be scored is listed and never chosen
    out = select_clusters([2, 3], _stub({2: None, 3: -0.2}, []))
    assert out["clusters"] == 3 and out["selection"]["candidates"][0]["silhouette"] is None
    with pytest.raises(ValueError, match="no candidate"):
        select_clusters([2, 3], _stub({2: None, 3: None}, []))


def test_cluster_counts():
    assert check_cluster_counts(3) == ([3], False) and check_cluster_counts(1) == ([1], False)
    assert check_cluster_counts([2, 5, 3]) == ([2, 5, 3], True) and check_cluster_counts(range(2, 5)) == ([2, 3, 4], True)
    for bad in ([], [2, 2], [1, 2], [2, 3.0], [True, 2], "3", 0, True, 2.0):
        with pytest.raises(ValueError, match="cluster"):
            check_cluster_counts(bad)


# ---- the section ----------------------------------------------------------------------------------------------------
def test_section_keys():
    assert check_section({"clusters": 3}) == {} and check_section({"labels": "Y", "restarts": 3}) == {}
    assert check_section({"clusters": 3, "silhouette": False}) == {}
    assert check_section({"clusters": 3, "silhouette": True}) == {"silhouette": True}
    assert check_section({"clusters": [2, 3, 4]}) == {"silhouette": True}             # a list implies the scoring
    assert check_section({"labels": "Y", "silhouette": True, "silhouette_metric": "cosine", "silhouette_points": None}) \
        == {"silhouette": True, "silhouette_metric": "cosine", "silhouette_points": None}
    assert check_section({"clusters": [2, 3], "silhouette_points": 500}) == {"silhouette": True, "silhouette_points": 500}
    for bad, text in (({"clusters": 3, "silhouette": 1}, "true or false"), ({"clusters": 3, "silhouette": "yes"}, "true or false"),
                      ({"clusters": 3, "silhouette": True, "silhouette_metric": "l1"}, "silhouette_metric"),
                      ({"clusters": 3, "silhouette": True, "silhouette_metric": 2}, "silhouette_metric"),
                      ({"clusters": 3, "silhouette": True, "silhouette_points": 1}, "silhouette_points"),
                      ({"clusters": 3, "silhouette": True, "silhouette_points": 2.5}, "silhouette_points"),
                      ({"clusters": 3, "silhouette": True, "silhouette_points": True}, "silhouette_points"),
                      ({"clusters": 3, "silhouette": True, "silhouette_points": "all"}, "silhouette_points"),
                      ({"clusters": 3, "silhouette_metric": "cosine"}, "belongs to silhouette"),
                      ({"clusters": 3, "silhouette": False, "silhouette_points": 100}, "belongs to silhouette"),
                      ({"clusters": []}, "distinct integers"), ({"clusters": [2, 2]}, "distinct integers"),
                      ({"clusters": [1, 2]}, "distinct integers"), ({"clusters": [2, "3"]}, "distinct integers"),
                      ({"clusters": [2, 3.5]}, "distinct integers")):
        with pytest.raises(ValueError, match=text):
            check_section(bad)


CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


def test_wrong_types_are_refused_before_the_graph_is_loaded(monkeypatch, tmp_path):
    import clane_amd.__main__ as M

    def touched(*a, **k):
        raise AssertionError("the run went on to set up devices")
    monkeypatch.setattr(M, "_distributed_setup", touched)
    monkeypatch.setattr(M, "Graph", touched)
    cfg = tmp_path / "config.yaml"
    args = M.get_parser().parse_args(["--data_root", str(tmp_path), "--output_root", str(tmp_path / "o"),
                                      "--config_file", str(cfg)])
    for section, text in (("  clusters: 3\n  silhouette: 2\n", "true or false"),
                          ("  clusters: 3\n  silhouette: true\n  silhouette_metric: manhattan\n", "silhouette_metric"),
                          ("  clusters: 3\n  silhouette: true\n  silhouette_points: many\n", "silhouette_points"),
                          ("  clusters: [2, two]\n", "distinct integers"), ("  clusters: []\n", "distinct integers"),
                          ("  clusters: 3\n  silhouette_points: 100\n", "belongs to silhouette")):
        cfg.write_text(CONFIG + "\nnode_clustering:\n" + section)
        with pytest.raises(ValueError, match=text):
            M.embedding(args)
    for section in ("  clusters: [2, 3, 4]\n", "  labels: Y\n  silhouette: true\n  silhouette_metric: cosine\n",
                    "  clusters: 4\n  silhouette: true\n  silhouette_points: null\n"):
        cfg.write_text(CONFIG + "\nnode_clustering:\n" + section)
        with pytest.raises(AssertionError, match="went on"):            # a valid section passes the validation
            M.embedding(args)
    monkeypatch.setenv("WORLD_SIZE", "2")
    cfg.write_text(CONFIG + "\nnode_clustering:\n  clusters: [2, 3]\n")
    with pytest.raises(NotImplementedError, match="node_clustering runs on one GPU"):
        M.embedding(args)


# ---- the ABI ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "clane_hip.h").read_text(), flags=re.S)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", header)
        assert decl and name in _hip.SIGNATURES, name
        assert len(_hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
        assert getattr(lib, name) is not None
    assert re.search(r"#define CLANE_ABI_VERSION 5\b", header) and lib.clane_abi_version() == 5      # additions only
    assert re.search(r"#define CLANE_SILHOUETTE_EUCLIDEAN 0\b", header) and re.search(r"#define CLANE_SILHOUETTE_COSINE 1\b", header)
    assert _hip.SILHOUETTE_METRICS == {"euclidean": 0, "cosine": 1}
    for name in ("silhouette_norms", "silhouette_sums"):
        assert callable(getattr(_hip.HipKernels, name)) and callable(getattr(_hip.KernelBackend, name))
    assert "clane_silhouette_" in (ROOT / "INTEGRATION.md").read_text()


def test_argument_validation_reaches_last_error():
    lib = _hip.load_library()                   # refused on the host before any launch: safe without a GPU
    p = C.cast((C.c_double * 64)(), C.c_void_p)

    def norms(fn=lib.clane_silhouette_norms_f32, d=4, ldz=4, n=2, metric=0, Z=p, order=p, mu=p, nrm=p, rows=8):
        return fn(Z, rows, d, ldz, order, n, mu, metric, nrm, None)
    for bad, text in ((dict(d=0), b"bad shape"), (dict(ldz=3), b"bad shape"), (dict(n=-1), b"bad shape"),
                      (dict(rows=-1), b"bad shape"), (dict(metric=2), b"unknown metric"), (dict(metric=-1), b"unknown metric"),
                      (dict(Z=None), b"null pointer"), (dict(order=None), b"null pointer"), (dict(mu=None), b"null pointer"),
                      (dict(nrm=None), b"null pointer")):
        assert norms(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"silhouette_norms" in lib.clane_last_error()
    assert norms(fn=lib.clane_silhouette_norms_bf16, d=-1) == -1 and norms(fn=lib.clane_silhouette_norms_f64, metric=7) == -1
    assert norms(n=0, Z=None, order=None) == 0                       # nothing to do is not an error

    def sums(fn=lib.clane_silhouette_sums_f32, d=4, ldz=4, n=6, K=2, metric=0, p0=0, p1=6, Z=p, order=p, seg=p, mu=p,
             nrm=p, S=p):
        return fn(Z, 8, d, ldz, order, n, seg, K, mu, nrm, metric, p0, p1, S, None)
    for bad, text in ((dict(d=0), b"bad shape"), (dict(ldz=2), b"bad shape"), (dict(n=-1), b"bad shape"),
                      (dict(metric=5), b"unknown metric"), (dict(K=0), b"K must be"), (dict(p0=-1), b"positions"),
                      (dict(p0=4, p1=3), b"positions"), (dict(p1=7), b"positions"), (dict(Z=None), b"null pointer"),
                      (dict(order=None), b"null pointer"), (dict(seg=None), b"null pointer"), (dict(mu=None), b"null pointer"),
                      (dict(nrm=None), b"null pointer"), (dict(S=None), b"null pointer"),
                      (dict(K=1 << 30, n=1 << 20, p1=1 << 20), b"too many")):
        assert sums(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"silhouette_sums" in lib.clane_last_error()
    assert sums(fn=lib.clane_silhouette_sums_bf16, K=-3) == -1 and sums(fn=lib.clane_silhouette_sums_f64, d=0) == -1
    assert sums(p0=3, p1=3, S=None) == 0                             # an empty block of positions


def test_shapes_cover_the_tile():
    sizes = {s for shape in SHAPES for s in np.bincount(partition(shape).numpy(), minlength=shape[2]).tolist()}
    assert {0, 1, 127, 128, 129, 257} <= sizes
