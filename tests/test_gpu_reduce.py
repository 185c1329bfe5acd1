"""Content reduction on the GPU (clane_amd/reduce.py, csrc/content_pca.h): the three calls through the C ABI -- exact on
integer data, bit for bit the existing dense kernels on float data, within a derived bound of float64 -- and the surface
above them (ContentPCA, Graph.reduce_content / project, the CLI's content_reduction section).  Fixtures, references and
checks: tests/reduce_cases.py; tests/test_reduce_host.py runs the same exact checks through a plain-torch double."""
import json

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR
from clane_amd.reduce import NPZ_KEYS, ContentPCA
from clane_amd.similarity import CosineSimilarity

from . import reduce_cases as RC
from .conftest import write_data_root

pytestmark = pytest.mark.gpu
ids = RC.case_id


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


# ---- exact, on integer data ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", RC.DTYPES, ids=ids)
@pytest.mark.parametrize("d", RC.INT_D)
@pytest.mark.parametrize("n", RC.INT_N)
def test_sums_and_gram_on_integer_data(dev, k, dtype, n, d):
    """sums and G == the int64 reference (mu NULL, an integer vector, the true integer mean); G == G^T; NaN pad columns,
    a shuffled row list with a repeat and an index past the table."""
    RC.check_int_sums(k, dev, dtype, n, d)
    RC.check_int_gram(k, dev, dtype, n, d)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=ids)
@pytest.mark.parametrize("d", RC.INT_D)
@pytest.mark.parametrize("n", RC.INT_N)
def test_projection_on_integer_data(dev, k, dtype, n, d):
    """Y == the int64 reference for W in {-1, 0, 1}, m in {1, 5, 130}; an absent row's Y is zeros."""
    for m in RC.INT_M:
        RC.check_int_affine(k, dev, dtype, n, d, m)


def test_unaligned_table_gives_the_aligned_bits(dev, k):
    """Column sums from a table whose rows are not 16-byte aligned (the element-wise layout) == the packed layout's."""
    for dtype in RC.DTYPES:
        X = (torch.randn(2300, 130, generator=RC.gen(3), dtype=RC.F64) * 3).to(dtype)
        rows = torch.randperm(2300, generator=RC.gen(4)).to(torch.int32).to(dev)
        vec = _hip.VEC_ELEMS[dtype]
        aligned = torch.zeros(2300, 130 + (-130) % vec, dtype=dtype, device=dev)
        aligned[:, :130] = X.to(dev)
        odd = RC.place(X, dtype, dev, pad=1)                  # ld = 131: no row but the first starts a pack
        assert aligned.stride(0) % vec == 0 and odd.stride(0) % vec != 0
        a, b = RC.run_sums(k, aligned[:, :130], 130, rows), RC.run_sums(k, odd, 130, rows)
        assert torch.equal(a, b) and not bool(torch.isnan(a).any())


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=ids)
@pytest.mark.parametrize("data", ["int", "float"])
def test_streaming_in_blocks_of_2048_rows_gives_the_one_call_bits(dev, k, dtype, data):
    RC.check_streaming(k, dev, dtype, 130, data)


# ---- exact, on random float data: the dense-bits contract ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", RC.DTYPES, ids=ids)
@pytest.mark.parametrize("d", [130, 257])
def test_gram_has_the_bits_of_probe_grad(dev, k, dtype, d):
    RC.check_gram_is_probe_grad(k, dev, dtype, d)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=ids)
@pytest.mark.parametrize("d,m", [(130, 5), (130, 130), (257, 130), (5, 10)])
def test_affine_projection_has_the_bits_of_project_rows(dev, k, dtype, d, m):
    RC.check_affine_is_project_rows(k, dev, dtype, d, m)


# ---- against float64, with the derived bound ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", RC.DTYPES, ids=ids)
def test_gram_and_fit_within_the_derived_bound_of_float64(dev, k, dtype):
    """|G - G64| <= (2048 + chunks + 2) u |Xc|^T |Xc| element-wise; explained variances within ||bound||_F / (n - 1)
    (Weyl); each of the five planted components within 2 ||bound||_F / gap_j of numpy's eigh of the float64 Gram
    (Davis-Kahan).  bf16: the reference is taken on the rounded input.  Observed on an MI355X: see DESIGN 6.14."""
    RC.check_gram_bound(k, dev, dtype)
    X = RC.planted_matrix(dtype)
    pca = ContentPCA(5).fit(X)
    RC.check_fit_bounds(pca, X, dtype)
    assert pca.n_samples_ == 700 and pca.components_.shape == (5, 130) and pca.components_.dtype == np.float64
    assert np.all(np.diff(pca.explained_variance_) <= 0)
    assert np.allclose(pca.explained_variance_ratio_, pca.explained_variance_ / pca.total_variance_)
    top = np.abs(pca.components_).argmax(1)
    assert (pca.components_[np.arange(5), top] > 0).all()                        # the sign rule
    assert np.allclose(pca.mean_, X.double().mean(0).numpy(), atol=3 * 2.0 ** -24 * 8)


def test_whitened_columns_have_unit_sample_variance_in_fp64(dev, k):
    X = RC.planted_matrix(RC.F64)
    pca = ContentPCA(5, whiten=True).fit(X)
    Y = pca.transform(X)
    assert Y.dtype == RC.F64 and not Y.is_cuda and tuple(Y.shape) == (700, 5)
    _, bound = RC.gram_bound(X, pca.mean_, RC.F64)
    lam = pca.explained_variance_ * (X.shape[0] - 1)
    var = Y.numpy().var(axis=0, ddof=1)
    err = np.abs(var - 1.0)
    print("whiten fp64: |var - 1| =", err, "bound =", float(torch.linalg.norm(bound)) / lam)
    assert (err <= float(torch.linalg.norm(bound)) / lam).all()


def test_whiten_on_a_rank_deficient_matrix_names_the_rank(dev):
    X = torch.zeros(40, 6, dtype=RC.F64)
    X[:, 0] = torch.arange(40.0)
    X[:, 1] = torch.arange(40.0) % 7
    with pytest.raises(ValueError, match=r"numerical rank 2 of d = 6"):
        ContentPCA(3, whiten=True).fit(X)
    assert ContentPCA(3).fit(X).explained_variance_[2] == 0.0


# ---- surface -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", RC.DTYPES, ids=ids)
def test_fit_transform_blocks_and_devices_give_the_same_bits(dev, dtype, tmp_path):
    X = (torch.randn(4300, 130, generator=RC.gen(51), dtype=RC.F64) * 2 + 1).to(dtype)
    one = ContentPCA(7)
    Y = one.fit_transform(X)
    assert Y.dtype == dtype and not Y.is_cuda and tuple(Y.shape) == (4300, 7)
    two = ContentPCA(7).fit(X)
    assert torch.equal(two.transform(X), Y)
    streamed = ContentPCA(7, block_rows=2048)
    assert torch.equal(streamed.fit_transform(X), Y)                             # three blocks == one block
    on_card = ContentPCA(7)
    Yd = on_card.fit_transform(X.to(dev))
    assert Yd.is_cuda and torch.equal(Yd.cpu(), Y)
    for other in (two, streamed, on_card):
        for name in ("components_", "mean_", "explained_variance_", "explained_variance_ratio_"):
            assert np.array_equal(getattr(other, name), getattr(one, name)), name
    back = ContentPCA.load(one.save(tmp_path / "pca.npz"))
    with np.load(tmp_path / "pca.npz") as z:
        assert sorted(z.files) == sorted(NPZ_KEYS)
    for name in ("components_", "mean_", "explained_variance_", "explained_variance_ratio_", "total_variance_",
                 "n_samples_", "dim", "center", "whiten"):
        assert np.array_equal(getattr(back, name), getattr(one, name)), name
    assert torch.equal(back.transform(X), Y)
    flat = ContentPCA(7, center=False).fit(X)
    assert not flat.mean_.any() and flat.explained_variance_[0] > one.explained_variance_[0]


def small_graph(V=700, seed=0, max_deg=12):
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, max_deg + 1, size=V)
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    colidx = np.concatenate([np.sort(rng.choice(V, size=g, replace=False)) for g in deg] + [np.empty(0, int)])
    return HostCSR(V, rowptr, colidx.astype(np.int32))


def iterate(g, dev):
    from clane_amd.embedder import Embedder
    Embedder(graph=g, similarity_measure=CosineSimilarity(), device=dev, gamma=0.76, tolerence=3, verbose=False).iterate()
    return g.Z


def test_reduce_content_then_iterate_is_a_graph_on_the_reduced_content(dev):
    csr, X = small_graph(), RC.planted_matrix(RC.F32)
    g = Graph.from_csr(csr, X.clone())
    pca = g.reduce_content(8)
    assert g.content_transform is pca and g.d == 8 and tuple(g.X.shape) == (700, 8) and g.X.dtype == RC.F32
    assert torch.equal(g.X, ContentPCA(8).fit_transform(X))
    Z = iterate(g, dev)
    fresh = Graph.from_csr(csr, g.X.clone())
    assert torch.equal(Z, iterate(fresh, dev)) and tuple(Z.shape) == (700, 8)
    with pytest.raises(RuntimeError, match="engine exists already"):
        g.reduce_content(4)


def test_project_reads_the_table_and_changes_nothing(dev):
    from clane_amd.links import LinkRanker
    g = Graph.from_csr(small_graph(seed=1), RC.planted_matrix(RC.F32)[:, :24].contiguous())
    iterate(g, dev)
    eng = g.engine()
    ranker = LinkRanker(eng, CosineSimilarity())
    ids0, sc0 = ranker.top_k(5)
    Z0 = eng.get_Z()
    Y, pca = g.project(2)
    assert tuple(Y.shape) == (700, 2) and not Y.is_cuda and pca.dim == 2
    assert torch.equal(Y, ContentPCA(2).fit_transform(g.Z))
    some = [5, 699, 0, 5]
    Ys, _ = g.project(3, vertices=some, whiten=False)
    assert torch.equal(Ys, ContentPCA(3).fit_transform(g.Z[some]))
    Yx, _ = g.project(2, table="X")
    assert torch.equal(Yx, ContentPCA(2).fit_transform(g.X))
    assert torch.equal(eng.get_Z(), Z0)
    ids1, sc1 = ranker.top_k(5, refresh=False)
    assert torch.equal(ids1, ids0) and torch.equal(sc1, sc0)


CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


def test_cli_reduces_the_content_and_the_arrivals(dev, tmp_path):
    import clane_amd.__main__ as M
    from .conftest import load_golden
    from .new_vertex_cases import write_arrivals
    gold = load_golden("g2_karate_csr.npz")
    rng = np.random.default_rng(0)
    C = (rng.standard_normal((34, 12)) * np.linspace(3, 0.5, 12) + 2).astype(np.float32)
    root = write_data_root(tmp_path / "karate", gold["vertex_ids"], gold["edge_src"], gold["edge_dst"], C)
    vids = [str(v) for v in gold["vertex_ids"]]
    new_ids, lists = ["new-b", "new-a", "new-c"], [[3, 9], [0], []]
    Xn = (rng.standard_normal((3, 12)) + 2).astype(np.float32)
    write_arrivals(root / "arrivals", V="\n".join(new_ids) + "\n",
                   E="".join(f"{new_ids[i]}\t{vids[v]}\n" for i in range(3) for v in lists[i]), C_=Xn)

    def run(extra, out):
        cfg = tmp_path / f"{out}.yaml"
        cfg.write_text(CONFIG + extra)
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg), "--gpu"]))
        return tmp_path / out
    out = run("\ncontent_reduction:\n  dim: 4\n\nnew_vertices:\n  root: arrivals\n", "fit")
    Z = np.load(out / "Z.npy")
    assert Z.shape == (34, 4)
    pca = ContentPCA.load(out / "content_projection.npz")
    with np.load(out / "content_projection.npz") as z:
        assert sorted(z.files) == sorted(NPZ_KEYS)
    rep = json.loads((out / "content_reduction.json").read_text())
    assert set(rep) == {"input_width", "output_width", "n", "explained_variance_ratio", "explained_variance_ratio_sum",
                        "center", "whiten", "source"}
    assert (rep["input_width"], rep["output_width"], rep["n"], rep["source"]) == (12, 4, 34, "fit")
    assert rep["center"] is True and rep["whiten"] is False and len(rep["explained_variance_ratio"]) == 4
    assert abs(sum(rep["explained_variance_ratio"]) - rep["explained_variance_ratio_sum"]) < 1e-12
    # Z_new.npy == Graph.embed_new on hand-transformed arrivals, against the reduced graph
    g = Graph(data_root=root, embedding_dim=4)
    g.X = pca.transform(g.X)
    g.d = 4
    g.set_Z(torch.from_numpy(Z))
    res = g.embed_new(CosineSimilarity(), pca.transform(torch.from_numpy(Xn)), lists, gamma=0.76, tolerence=3)
    assert np.array_equal(np.load(out / "Z_new.npy"), res.Z.numpy())
    # the reduced content is what a fit on C gives, and loading the written transform reproduces the run
    assert torch.equal(g.X, ContentPCA(4).fit_transform(torch.from_numpy(C)))
    (root / "saved.npz").write_bytes((out / "content_projection.npz").read_bytes())
    again = run("\ncontent_reduction:\n  load: saved.npz\n\nnew_vertices:\n  root: arrivals\n", "load")
    assert (again / "Z.npy").read_bytes() == (out / "Z.npy").read_bytes()
    assert (again / "Z_new.npy").read_bytes() == (out / "Z_new.npy").read_bytes()
    assert json.loads((again / "content_reduction.json").read_text())["source"] == "load"
    plain = run("", "plain")
    assert np.load(plain / "Z.npy").shape == (34, 12) and not (plain / "content_reduction.json").exists()
    with pytest.raises(ValueError, match=r"exceeds min\(d, n - 1\)"):
        run("\ncontent_reduction:\n  dim: 13\n", "toowide")
