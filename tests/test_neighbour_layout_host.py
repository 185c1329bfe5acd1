"""The neighbour-sparse 2-D layout without a GPU: the restatement of tests/neighbour_layout_cases.py pinned to
tests/layout_cases.py (with every other point a neighbour it IS exact t-SNE) and to scikit-learn's
``_joint_probabilities_nn`` (where it is installed), the `layout:` section's two new keys, ``Graph.layout``'s argument
refusals and the additions to the C ABI."""
import numpy as np
import pytest
import torch

from clane_amd import _hip, layout
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR

from . import layout_cases as LC
from . import neighbour_layout_cases as NC


def centred_sqdist(X):
    X = X.astype(np.float64)
    return LC.sqdist(X - X.mean(0))[0]


# ---- the checker against the exact restatement and scikit-learn -----------------------------------------------------------
def test_with_every_other_point_a_neighbour_it_is_exact_tsne():
    n, perplexity = 40, 10.0
    D = centred_sqdist(LC.gaussian(n, 8, seed=3))
    ids, sq = NC.knn(D, n - 1)
    assert (np.sort(ids, 1) == np.array([np.delete(np.arange(n), i) for i in range(n)])).all()
    assert (np.diff(sq, axis=1) >= 0).all()
    p, beta = NC.perplexity_search(sq, ids, perplexity)
    Pc, beta_full = LC.perplexity_search(D, perplexity)
    C, mask = NC.scatter(ids, p)
    assert mask.sum() == n * (n - 1) and not mask.diagonal().any()
    assert np.array_equal(beta, beta_full)
    assert np.abs(C - Pc).max() <= 1e-14
    P, union = NC.joint(ids, p)
    full = LC.joint(Pc)
    above = full > LC.EPS
    assert above.sum() > n and np.abs(P - full)[above].max() <= 1e-15
    assert np.array_equal(P, P.T) and not P.diagonal().any() and (union == ~np.eye(n, dtype=bool)).all()


def test_knn_order_is_total_and_the_tail_is_marked():
    D = np.array([[0.0, 2.0, 1.0, 2.0], [2.0, 0.0, 2.0, 2.0], [1.0, 2.0, 0.0, 5.0], [2.0, 2.0, 5.0, 0.0]])
    ids, sq = NC.knn(D, 5)
    assert ids.tolist() == [[2, 1, 3, -1, -1], [0, 2, 3, -1, -1], [0, 1, 3, -1, -1], [0, 1, 2, -1, -1]]
    assert sq[0].tolist() == [1.0, 2.0, 2.0, np.inf, np.inf]
    p, beta = NC.perplexity_search(sq, ids, 2.0)
    assert not p[ids < 0].any() and np.allclose(p.sum(1), 1.0) and np.isfinite(beta).all()


SKLEARN_REL = 3.32e-6       # measured: max |P - P_sklearn| / max P_sklearn at n = 300, perplexity 30, k = 90


def test_restated_sparse_joint_is_scikit_learns():
    """scikit-learn searches in float32 and divides by P.sum() where the restatement divides by 2n: 4x what was measured."""
    t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.sparse import csr_matrix
    n, k, perplexity = 300, 90, 30.0
    D = centred_sqdist(LC.gaussian(n, 16, seed=1))
    ids, sq = NC.knn(D, k)
    p, _ = NC.perplexity_search(sq, ids, perplexity)
    P, union = NC.joint(ids, p)
    dist = csr_matrix((sq.astype(np.float32).ravel(), ids.ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
    P_sk = t_sne._joint_probabilities_nn(dist, perplexity, 0).toarray()
    rel = np.abs(P - P_sk).max() / P_sk.max()
    print(f"sparse joint P: max |restatement - scikit-learn| / max P = {rel:.3g} (allowed {4 * SKLEARN_REL:.3g}); "
          f"{int(union.sum())} entries")
    assert rel <= 4 * SKLEARN_REL
    assert not P_sk[~union].any() and not P[~union].any() and (P[union] > 0).all()


# ---- the config section --------------------------------------------------------------------------------------------------------
def test_section_takes_the_two_keys_and_returns_them_only_when_given():
    assert layout.check_section({}) == layout.SECTION_DEFAULTS and set(layout.SECTION_DEFAULTS) == set(layout.SECTION_KEYS)
    assert layout.check_section({"method": "exact"}) == {**layout.SECTION_DEFAULTS, "method": "exact"}
    got = layout.check_section({"method": "neighbours"})
    assert got == {**layout.SECTION_DEFAULTS, "method": "neighbours"} and "neighbours" not in got
    got = layout.check_section({"method": "neighbours", "neighbours": 45, "max_points": 1 << 20, "perplexity": 12})
    assert got == {**layout.SECTION_DEFAULTS, "method": "neighbours", "neighbours": 45, "max_points": 1 << 20,
                   "perplexity": 12.0}
    assert layout.check_section({"method": "neighbours", "neighbours": 192, "perplexity": 64})["neighbours"] == 192


@pytest.mark.parametrize("section,match", [
    ({"method": "barnes_hut"}, r"method must be one of \['exact', 'neighbours'\]"),
    ({"method": 1}, "method must be one of"),
    ({"neighbours": 90}, "neighbours = 90 needs method: neighbours"),
    ({"method": "exact", "neighbours": 90}, "neighbours = 90 needs method: neighbours"),
    ({"max_points": 65537}, r"max_points = 65537 exceeds 65536 \(P would pass 16 GiB\)"),
    ({"method": "exact", "max_points": 65537}, r"max_points = 65537 exceeds 65536 \(P would pass 16 GiB\)"),
    ({"method": "neighbours", "max_points": (1 << 20) + 1}, "max_points = 1048577 exceeds 1048576"),
    ({"method": "neighbours", "neighbours": 193}, "neighbours = 193 must be above perplexity = 30 and at most 192"),
    ({"method": "neighbours", "neighbours": 30}, "neighbours = 30 must be above perplexity = 30"),
    ({"method": "neighbours", "neighbours": 20}, "neighbours = 20 must be above perplexity = 30"),
    ({"method": "neighbours", "neighbours": 90.0}, "neighbours must be an integer"),
    ({"method": "neighbours", "neighbours": True}, "neighbours must be an integer"),
    ({"method": "neighbours", "perplexity": 65}, "perplexity = 65 asks for 195 neighbours per point, more than 192"),
    ({"method": "neighbours", "perplexty": 3}, r"unknown keys \['perplexty'\]"),
])
def test_section_refuses(section, match):
    with pytest.raises(ValueError, match=match):
        layout.check_section(section)


CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


@pytest.mark.parametrize("extra,match", [
    ("\nlayout:\n  method: tree\n", "layout: method must be one of"),
    ("\nlayout:\n  neighbours: 40\n", "layout: neighbours = 40 needs method: neighbours"),
    ("\nlayout:\n  method: neighbours\n  neighbours: 500\n", "layout: neighbours = 500 must be above"),
    ("\nlayout:\n  max_points: 65537\n", "layout: max_points = 65537 exceeds 65536"),
])
def test_cli_checks_the_new_keys_before_the_graph_is_read(tmp_path, monkeypatch, extra, match):
    """The data root does not exist: an error of the section's own is proof that it came first."""
    import clane_amd.__main__ as M
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG + extra)
    with pytest.raises(ValueError, match=match):
        M.embedding(M.get_parser().parse_args(["--data_root", str(tmp_path / "none"), "--output_root",
                                               str(tmp_path / "out"), "--config_file", str(cfg)]))


# ---- arithmetic of the classes ---------------------------------------------------------------------------------------------------
class Engine:                                    # what the constructors look at
    world, columns, halo, exchange, k, d = 1, False, False, "none", None, 16


def test_neighbour_counts_limits_and_workspace():
    t = layout.NeighbourTSNE(Engine())
    assert t.neighbours is None and t.neighbours_for(300) == 90 and t.neighbours_for(50) == 49
    assert layout.NeighbourTSNE(Engine(), perplexity=5).neighbours_for(300) == 15
    assert layout.NeighbourTSNE(Engine(), neighbours=120).neighbours_for(300) == 120
    t.check_points(1 << 20)
    t.check_points(65537)
    for n, match in ((3, "at least 4 points"), (30, "must be below n = 30"), ((1 << 20) + 1, "exceeds 1048576 points"),
                     (31, "perplexity = 30 must be below the 30 neighbours of n = 31")):
        with pytest.raises(ValueError, match=match):
            t.check_points(n)
    with pytest.raises(ValueError, match=r"neighbours = 120 must be above .* at most 99 \(n - 1 of n = 100 points\)"):
        layout.NeighbourTSNE(Engine(), neighbours=120).check_points(100)
    for bad, match in ((193, "at most 192"), (30, "must be above perplexity = 30"), (45.0, "must be an integer")):
        with pytest.raises(ValueError, match=match):
            layout.NeighbourTSNE(Engine(), neighbours=bad)
    with pytest.raises(ValueError, match="perplexity up to 64"):
        layout.NeighbourTSNE(Engine(), perplexity=70)
    # nothing is n x n: a million points take gigabytes, not the terabytes of P [n, n]
    assert t.workspace_bytes(1 << 20) < 16 << 30 < layout.TSNE.workspace_bytes(65536)
    assert t.workspace_bytes(65536) > 65536 * 90 * (4 + 4 + 4 + 2 * 8)       # the lists and the CSR at the least
    assert layout.knn_query_tile(40) == 128 and layout.knn_query_tile(41) == 64 and layout.knn_query_tile(96) == 64
    assert layout.knn_query_tile(97) == 32 and layout.knn_query_tile(192) == 32
    assert layout.knn_slabs(1 << 18, 90) == 1 and layout.knn_slabs(257, 7) == 3 and layout.knn_slabs(5, 4) == 1

    class Divided(Engine):
        world, exchange = 2, "halo"
    with pytest.raises(NotImplementedError, match="t-SNE runs on ONE GPU only.*2 ranks"):
        layout.NeighbourTSNE(Divided())
    with pytest.raises(NotImplementedError, match="neighbour search runs on ONE GPU only.*2 ranks"):
        layout.KNeighbours(Divided())
    for n, k, match in ((300, 0, "k must be an integer in"), (300, 193, "k must be an integer in"), (1, 3, "2 to 1048576 rows")):
        with pytest.raises(ValueError, match=match):
            layout.KNeighbours.check(n, k)


def test_graph_refuses_bad_arguments_on_the_host():
    """Before the engine is asked for: none of these needs a GPU."""
    V = 40
    csr = HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + 1) % V).astype(np.int32))
    g = Graph.from_csr(csr, torch.from_numpy(LC.gaussian(V, 8)))
    with pytest.raises(ValueError, match=r"layout: method must be one of \['exact', 'neighbours'\], got 'barnes_hut'"):
        g.layout(method="barnes_hut")
    with pytest.raises(ValueError, match="layout: neighbours = 12 needs method=\"neighbours\""):
        g.layout(neighbours=12)
    with pytest.raises(ValueError, match="layout: neighbours = 12 needs method"):
        g.layout(method="exact", neighbours=12)
    with pytest.raises(ValueError, match="max_points must be an integer >= 4"):
        g.layout(method="neighbours", max_points=3)
    with pytest.raises(ValueError, match="k must be an integer in"):
        g.neighbours(0)
    with pytest.raises(ValueError, match="k must be an integer in"):
        g.neighbours(193)
    assert g._engine is None


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("clane_knn_sqdist_f32", "clane_knn_sqdist_bf16", "clane_tsne_nn_affinities_f32", "clane_tsne_nn_plogp_f32",
               "clane_tsne_nn_attract_f32", "clane_tsne_repulse_f32")


def test_abi_additions_keep_the_version():
    assert _hip.ABI_VERSION == 5 and _hip.KNN_MAX_K == 192 and _hip.TSNE_NN_MAX_POINTS == 1 << 20
    assert _hip.TSNE_MAX_POINTS == 65536
    lib = _hip.load_library()
    assert lib.clane_abi_version() == 5
    for name in NEW_SYMBOLS:
        assert name in _hip.SIGNATURES and getattr(lib, name) is not None
    for name in ("knn_sqdist", "tsne_nn_affinities", "tsne_nn_plogp", "tsne_nn_attract", "tsne_repulse"):
        assert callable(getattr(_hip.KernelBackend, name))
    # invalid arguments are rejected on the host before any launch: safe without a GPU
    rc = lib.clane_knn_sqdist_f32(None, 8, 4, 4, None, 8, None, None, 193, 1, None, None, None, None, None)
    assert rc == -1 and b"k must be in [1, 192], got 193" in lib.clane_last_error()
    rc = lib.clane_knn_sqdist_f32(None, 8, 4, 4, None, (1 << 20) + 1, None, None, 8, 1, None, None, None, None, None)
    assert rc == -1 and b"bad shape" in lib.clane_last_error()
    rc = lib.clane_knn_sqdist_bf16(None, 8, 4, 4, None, 8, None, None, 8, 0, None, None, None, None, None)
    assert rc == -1 and b"n_slabs" in lib.clane_last_error()
    rc = lib.clane_knn_sqdist_f32(None, 8, 4, 4, None, 8, None, None, 8, 1, None, None, None, None, None)
    assert rc == -1 and b"null pointer" in lib.clane_last_error()
    rc = lib.clane_tsne_nn_affinities_f32(None, None, 300, 90, 90.0, None, None, None)
    assert rc == -1 and b"perplexity 90 is not in (0, k = 90)" in lib.clane_last_error()
    rc = lib.clane_tsne_nn_affinities_f32(None, None, 300, 193, 30.0, None, None, None)
    assert rc == -1 and b"k must be in" in lib.clane_last_error()
    rc = lib.clane_tsne_nn_plogp_f32(None, None, 0, 0, None, None)
    assert rc == -1 and b"bad shape" in lib.clane_last_error()
    rc = lib.clane_tsne_nn_attract_f32(None, None, None, None, 8, 4, 2, None, None)
    assert rc == -1 and b"unknown flags 2" in lib.clane_last_error()
    rc = lib.clane_tsne_repulse_f32(None, (1 << 20) + 1, None, None)
    assert rc == -1 and b"n must be in [1, 1048576]" in lib.clane_last_error()
    rc = lib.clane_tsne_repulse_f32(None, 8, None, None)
    assert rc == -1 and b"null pointer" in lib.clane_last_error()
