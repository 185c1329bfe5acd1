"""The 2-D layout without a GPU: the float64 restatement of tests/layout_cases.py pinned to scikit-learn (where it is
installed), the `layout:` section's validation, the vertex sampling and neighbour_agreement on a hand-made case."""
import numpy as np
import pytest
import torch

from clane_amd import layout

from . import layout_cases as LC


# ---- the checker against scikit-learn --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pinned():
    X = LC.gaussian(300, 16, seed=1)
    D, _ = LC.sqdist(X.astype(np.float64) - X.astype(np.float64).mean(0))
    D32 = np.ascontiguousarray(D, dtype=np.float32)
    return D32, LC.joint_probabilities(D32, 30.0)


def test_restated_joint_probabilities_are_scikit_learns(pinned):
    t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    D32, P = pinned
    P_sk = squareform(t_sne._joint_probabilities(D32, 30.0, 0))
    err = np.abs(P - P_sk)[~np.eye(300, dtype=bool)].max()
    print(f"joint P: max |restatement - scikit-learn| = {err:.3g}, largest entry {P_sk.max():.3g}")
    assert err <= 1e-8
    assert np.array_equal(P, P.T) and not P.diagonal().any()


@pytest.mark.parametrize("scale", [1e-4, 10.0])
def test_restated_kl_and_gradient_are_scikit_learns(pinned, scale):
    t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    _, P = pinned
    Y = LC.layout_at(300, scale).astype(np.float64)
    kl_sk, g_sk = t_sne._kl_divergence(Y.ravel().copy(), squareform(P, checks=False), 1.0, 300, 2)
    kl, g, _ = LC.objective(P, Y, alpha=1.0)
    print(f"scale {scale:g}: KL {kl:.12g} vs {kl_sk:.12g}; max |g - g_sk| / max |g_sk| = "
          f"{np.abs(g.ravel() - g_sk).max() / np.abs(g_sk).max():.3g}")
    assert abs(kl - kl_sk) <= 1e-10 * abs(kl_sk)
    assert np.abs(g.ravel() - g_sk).max() <= 1e-10 * np.abs(g_sk).max()


def test_restated_update_is_scikit_learns_rule():
    g = np.array([[1.0, -2.0], [0.5, 0.0], [-1.0, 3.0]])
    V = np.array([[-1.0, -1.0], [0.0, 1.0], [-2.0, 0.0]])
    G = np.array([[1.0, 1.0], [0.011, 2.0], [0.012, 1.0]])
    Y = np.zeros((3, 2))
    Yn, Vn, Gn = LC.update(g, Y, V, G, momentum=0.5, lr=10.0)
    # v g < 0 grows the gain by 0.2; anything else (v g = 0 included) shrinks it to 0.8 of itself, floored at 0.01
    assert np.allclose(Gn, [[1.2, 0.8], [0.01, 1.6], [0.01, 0.8]])
    assert np.allclose(Vn, 0.5 * V - 10.0 * Gn * g) and np.allclose(Yn, Vn)


def test_degenerate_search_gives_the_uniform_row():
    D = np.ones((7, 7)) * 3.0
    np.fill_diagonal(D, 0.0)
    for dtype in (np.float64, np.float32):
        Pc, beta = LC.perplexity_search(D, 3.0, dtype)
        assert np.allclose(Pc[~np.eye(7, dtype=bool)], 1.0 / 6.0) and np.isfinite(beta).all()


# ---- the config section --------------------------------------------------------------------------------------------------------
def test_section_defaults_and_values():
    assert layout.check_section({}) == layout.SECTION_DEFAULTS == layout.check_section(None)
    got = layout.check_section({"perplexity": 5, "max_points": 100, "max_iter": 250, "seed": 3, "labels": "Y",
                                "baseline": True})
    assert got == {"perplexity": 5.0, "max_points": 100, "max_iter": 250, "seed": 3, "labels": "Y", "baseline": True}
    assert isinstance(got["perplexity"], float)


@pytest.mark.parametrize("section,match", [
    ([1, 2], "expected a mapping"),
    ("yes", "expected a mapping"),
    ({"perplexty": 30}, r"unknown keys \['perplexty'\]"),
    ({"perplexity": 0}, "perplexity must be a positive number"),
    ({"perplexity": -1.5}, "perplexity must be a positive number"),
    ({"perplexity": "30"}, "perplexity must be a positive number"),
    ({"perplexity": True}, "perplexity must be a positive number"),
    ({"perplexity": float("nan")}, "perplexity must be a positive number"),
    ({"max_points": 3}, "max_points must be an integer >= 4"),
    ({"max_points": 2.5}, "max_points must be an integer"),
    ({"max_points": True}, "max_points must be an integer"),
    ({"max_points": 65537}, "exceeds 65536"),
    ({"perplexity": 30, "max_points": 30}, "must be below max_points"),
    ({"max_iter": 0}, "max_iter must be an integer >= 1"),
    ({"max_iter": "1000"}, "max_iter must be an integer"),
    ({"seed": -1}, "seed must be an integer >= 0"),
    ({"seed": 1.0}, "seed must be an integer"),
    ({"labels": 7}, "labels must be the path"),
    ({"labels": ""}, "labels must be the path"),
    ({"baseline": "true"}, "baseline must be true or false"),
    ({"baseline": 1}, "baseline must be true or false"),
])
def test_section_refuses(section, match):
    with pytest.raises(ValueError, match=match):
        layout.check_section(section)


def test_section_refuses_several_gpus():
    with pytest.raises(NotImplementedError, match="ONE GPU only"):
        layout.check_section({}, world_size=2)


def test_missing_labels_file_is_named(tmp_path):
    assert layout.resolve_labels(layout.check_section({}), tmp_path) is None
    (tmp_path / "Y").write_text("a\t0\n")
    assert layout.resolve_labels(layout.check_section({"labels": "Y"}), tmp_path) == tmp_path / "Y"
    with pytest.raises(ValueError, match=r"layout: labels: .*nowhere' is missing"):
        layout.resolve_labels(layout.check_section({"labels": "nowhere"}), tmp_path)


CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


def run_cli(tmp_path, extra, monkeypatch, root="no_such_data_root"):
    import clane_amd.__main__ as M
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG + extra)
    M.embedding(M.get_parser().parse_args(["--data_root", str(tmp_path / root), "--output_root", str(tmp_path / "out"),
                                           "--config_file", str(cfg)]))


@pytest.mark.parametrize("extra,error,match", [
    ("\nlayout:\n  perplexty: 30\n", ValueError, "layout: unknown keys"),
    ("\nlayout:\n  perplexity: -3\n", ValueError, "layout: perplexity"),
    ("\nlayout:\n  max_points: many\n", ValueError, "layout: max_points"),
    ("\nlayout: 7\n", ValueError, "layout: expected a mapping"),
    ("\nlayout:\n  labels: Y\n", ValueError, "layout: labels: .* is missing"),
])
def test_cli_checks_the_section_before_the_graph_is_read(tmp_path, monkeypatch, extra, error, match):
    """The data root does not exist: an error of the section's own is proof that it came first."""
    with pytest.raises(error, match=match):
        run_cli(tmp_path, extra, monkeypatch)


def test_cli_refuses_the_section_on_several_gpus(tmp_path, monkeypatch):
    import clane_amd.__main__ as M
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG + "\nlayout:\n  perplexity: 5\n")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="layout: .* ONE GPU only"):
        M.embedding(M.get_parser().parse_args(["--data_root", str(tmp_path / "none"), "--output_root",
                                               str(tmp_path / "out"), "--config_file", str(cfg)]))


def test_cli_without_the_section_takes_the_old_path(tmp_path, monkeypatch):
    """No `layout:` key: the run goes on to read the graph, and fails there on the missing data root as it always did."""
    with pytest.raises(Exception) as without:
        run_cli(tmp_path, "", monkeypatch)
    assert "layout" not in str(without.value)


# ---- sampling ------------------------------------------------------------------------------------------------------------------
def test_sampling_is_seeded_sorted_and_reproducible():
    everyone, sampled = layout.sample_vertices(50, 50)
    assert not sampled and torch.equal(everyone, torch.arange(50))
    a, sampled = layout.sample_vertices(1000, 100, seed=3)
    b, _ = layout.sample_vertices(1000, 100, seed=3)
    c, _ = layout.sample_vertices(1000, 100, seed=4)
    assert sampled and torch.equal(a, b) and not torch.equal(a, c)
    assert a.numel() == 100 and len(set(a.tolist())) == 100 and torch.equal(a, torch.sort(a).values)
    assert int(a.min()) >= 0 and int(a.max()) < 1000
    expect = torch.sort(torch.randperm(1000, generator=torch.Generator().manual_seed(3))[:100]).values
    assert torch.equal(a, expect)


# ---- neighbour_agreement -------------------------------------------------------------------------------------------------------
def test_neighbour_agreement_on_a_hand_made_case():
    # two tight groups of three far apart, and one point of class 1 sitting inside group 0
    Y = torch.tensor([[0.0, 0.0], [0.1, 0.0], [0.0, 0.1], [10.0, 10.0], [10.1, 10.0], [10.0, 10.1], [0.05, 0.05]])
    y = torch.tensor([0, 0, 0, 1, 1, 1, 1])
    # k = 2: points 0..2 have the intruder as one of two neighbours (1/2 each); 3..5 agree fully; the intruder 0
    assert layout.neighbour_agreement(Y, y, k=2) == pytest.approx((3 * 0.5 + 3 * 1.0 + 0.0) / 7)
    assert layout.neighbour_agreement(Y[:6], y[:6], k=2) == 1.0
    assert layout.neighbour_agreement(Y, y, k=2) == pytest.approx(LC.neighbour_agreement(Y.numpy(), y.numpy(), k=2))
    with pytest.raises(ValueError, match="k must be in"):
        layout.neighbour_agreement(Y, y, k=7)
    with pytest.raises(ValueError, match="one label per point"):
        layout.neighbour_agreement(Y, y[:3])


def test_learning_rate_auto_and_the_arithmetic_refusals():
    class Engine:                                    # what TSNE's constructor looks at
        world, columns, halo, exchange, k, d = 1, False, False, "none", None, 16
    t = layout.TSNE(Engine(), perplexity=30.0)
    assert t.learning_rate_for(300) == 50.0 and t.learning_rate_for(48000) == 1000.0
    assert layout.TSNE(Engine(), learning_rate=200).learning_rate_for(48000) == 200.0
    for n, match in ((3, "at least 4 points"), (30, "must be below n = 30"), (65537, "exceeds 65536")):
        with pytest.raises(ValueError, match=match):
            t.check_points(n)
    t.check_points(65536)
    assert layout.TSNE.workspace_bytes(65536) > 16 << 30

    class Divided(Engine):
        world, exchange = 2, "halo"
    with pytest.raises(NotImplementedError, match="t-SNE runs on ONE GPU only.*2 ranks"):
        layout.TSNE(Divided())
    for bad in ({"perplexity": 0}, {"perplexity": "30"}, {"early_exaggeration": 0.5}, {"max_iter": 0},
                {"learning_rate": -1.0}):
        with pytest.raises(ValueError):
            layout.TSNE(Engine(), **bad)
