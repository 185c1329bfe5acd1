"""Sparse content reduction on the GPU (clane_amd/sparse.py, ContentPCA.fit_sparse, csrc/sparse_rows.h): the CSR product and
the row sums through the C ABI -- exact on integer data, bit for bit the header's summation order, within the derived bound
of float64 -- the randomized fit against exact dense PCA and its float64 restatement, and the surface above them
(Graph.reduce_sparse_content, the CLI's ``sparse:`` key).  Fixtures, references and checks: tests/sparse_cases.py;
tests/test_sparse_reduce_host.py runs the same checks through a plain-torch double."""
import json

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.graph import Graph
from clane_amd.reduce import ContentPCA
from clane_amd.similarity import CosineSimilarity
from clane_amd.sparse import SparseRows

from . import sparse_cases as SC
from .conftest import write_data_root

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


# ---- exact, on integer data ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", SC.INT_L)
def test_spmm_on_integer_data(dev, k, l):
    """Rows of 0, 1, 64, 65, SEG, SEG + 1 and 3 SEG + 5 non-zeros among 67; without an epilogue, with s, with a and s; NaN
    behind B's l columns, a sentinel behind out's; a column index D - 1."""
    SC.check_int_spmm(k, dev, SC.int_matrix(), l)


@pytest.mark.parametrize("l", (4, 132, 512))
def test_spmm_on_one_row(dev, k, l):
    SC.check_int_spmm(k, dev, SC.one_row_matrix(), l)


def test_row_sums_on_integer_data(dev, k):
    SC.check_int_row_sums(k, dev, SC.int_matrix())
    SC.check_int_row_sums(k, dev, SC.one_row_matrix())


def test_transpose_is_numpys_and_spmm_on_it_is_exact(dev, k):
    SC.check_transpose(k, dev)


# ---- the fixed order -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", (20, 132, 512))
def test_two_calls_sub_matrices_and_the_float64_bound(dev, k, l):
    SC.check_fixed_bits(k, dev, l)


@pytest.mark.parametrize("l", (20, 100, 256, 512))
def test_spmm_has_the_bits_of_the_written_order(dev, k, l):
    """Every instance (4, 2 and 1 sub-waves, two packs per lane) against the header's order restated in numpy, on rows of
    SEG + 1 and 2 SEG + 70 non-zeros among short ones; and on the device-made transpose."""
    SC.check_order_bits(k, dev, l)
    SC.check_order_bits(k, dev, l, transposed=lambda S: S.transposed())


# ---- the fit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", SC.FIT_DIMS)
def test_fit_against_exact_pca_and_the_float64_restatement(dev, dim):
    """At least 0.999 of the exact top-dim variance; orthonormal to 1e-6; explained variances within EV_REL_BOUND of the
    float64 restatement with the same Omega."""
    SC.check_fit_against_exact(dev, dim)


def test_seeds(dev):
    SC.check_seeds(dev)


def test_uncentred_whitened_and_rank_deficient_fits(dev):
    SC.check_uncentred(dev)
    SC.check_whiten(dev)
    SC.check_rank_deficient(dev)


def test_transform_is_the_dense_transform_and_survives_a_file(dev, tmp_path):
    SC.check_transform_and_files(dev, tmp_path, dense_transform=lambda pca, X: pca.transform(X))


# ---- surface -----------------------------------------------------------------------------------------------------------------
def small_graph(V, seed=0, max_deg=12):
    from clane_amd.partition import HostCSR
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


def test_reduce_sparse_content_then_iterate_runs_at_the_reduced_width(dev):
    S = SC.bag_of_words()
    csr = small_graph(S.shape[0])
    g = Graph.from_csr(csr, torch.zeros(S.shape[0], 4))
    pca = g.reduce_sparse_content(S, 8)
    assert g.content_transform is pca and g.d == 8 and tuple(g.X.shape) == (S.shape[0], 8) and not g.X.is_cuda
    assert torch.equal(g.X, ContentPCA(8).fit_transform_sparse(S.to(dev)).cpu())
    assert pca.report(S.shape[1])["method"] == "randomized" and pca.report(S.shape[1])["nnz"] == S.nnz
    Z = iterate(g, dev)
    fresh = Graph.from_csr(csr, g.X.clone())
    assert tuple(Z.shape) == (S.shape[0], 8) and torch.equal(Z, iterate(fresh, dev))
    with pytest.raises(RuntimeError, match="engine exists already"):
        g.reduce_sparse_content(S, 4)


CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


def test_cli_reduces_sparse_content(dev, tmp_path):
    import clane_amd.__main__ as M
    from .conftest import load_golden
    gold = load_golden("g2_karate_csr.npz")
    rng = np.random.default_rng(0)
    C = np.where(rng.random((34, 40)) < 0.25, rng.integers(1, 5, size=(34, 40)), 0).astype(np.float32)
    root = write_data_root(tmp_path / "karate", gold["vertex_ids"], gold["edge_src"], gold["edge_dst"])
    S = SparseRows.from_dense(C)
    S.save_npz(root / "C.npz")

    def run(extra, out):
        cfg = tmp_path / f"{out}.yaml"
        cfg.write_text(CONFIG + extra)
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg), "--gpu"]))
        return tmp_path / out
    out = run("\ncontent_reduction:\n  dim: 4\n  sparse: C.npz\n  oversample: 8\n  seed: 3\n", "fit")
    assert np.load(out / "Z.npy").shape == (34, 4)
    rep = json.loads((out / "content_reduction.json").read_text())
    assert set(rep) == {"input_width", "output_width", "n", "explained_variance_ratio", "explained_variance_ratio_sum",
                        "center", "whiten", "source", "method", "nnz", "oversample", "power_iterations", "seed"}
    assert (rep["input_width"], rep["output_width"], rep["n"], rep["source"]) == (40, 4, 34, "fit")
    assert (rep["method"], rep["nnz"], rep["oversample"], rep["power_iterations"], rep["seed"]) == \
        ("randomized", S.nnz, 8, 4, 3)
    pca = ContentPCA.load(out / "content_projection.npz")
    want = ContentPCA(4).fit_sparse(S.to(dev), oversample=8, seed=3)
    assert np.array_equal(pca.components_, want.components_)
    (root / "saved.npz").write_bytes((out / "content_projection.npz").read_bytes())
    again = run("\ncontent_reduction:\n  load: saved.npz\n  sparse: C.npz\n", "load")
    assert (again / "Z.npy").read_bytes() == (out / "Z.npy").read_bytes()
    assert json.loads((again / "content_reduction.json").read_text())["source"] == "load"
