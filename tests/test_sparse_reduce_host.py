"""The sparse content reduction without a GPU: the plain-torch double of the CSR calls (sparse_cases.TorchSparse) through
the checks tests/test_gpu_sparse_reduce.py runs on the kernels, the mutations each check has to catch, SparseRows'
validation, and the errors the CLI raises before a graph is loaded."""
import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd import reduce as R
from clane_amd.sparse import SEGMENT, SparseRows, segment_items

from . import sparse_cases as SC
from .conftest import write_data_root

CPU = torch.device("cpu")
CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


@pytest.fixture
def on_host(monkeypatch):
    """ContentPCA's device calls served by the double, on the host."""
    monkeypatch.setattr(_hip, "kernels", lambda: SC.TorchSparse(ordered=False))
    monkeypatch.setattr(_hip, "require_gpu", lambda device=None: CPU)


# ---- the double through the kernels' checks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("l", SC.INT_L)
def test_double_spmm_on_integer_data(l):
    SC.check_int_spmm(SC.TorchSparse(), CPU, SC.int_matrix(), l)


def test_double_on_one_row_and_row_sums():
    SC.check_int_spmm(SC.TorchSparse(), CPU, SC.one_row_matrix(), 20)
    SC.check_int_row_sums(SC.TorchSparse(), CPU, SC.int_matrix())
    SC.check_int_row_sums(SC.TorchSparse(), CPU, SC.one_row_matrix())


def test_double_transpose_and_fixed_order():
    SC.check_transpose(SC.TorchSparse(), CPU)
    SC.check_fixed_bits(SC.TorchSparse(), CPU, l=20)
    SC.check_order_bits(SC.TorchSparse(), CPU, 20)
    SC.check_order_bits(SC.TorchSparse(), CPU, 20, transposed=lambda S: S.transposed())


def test_int_fixture_is_what_it_says():
    S = SC.int_matrix()
    lens = np.diff(S.rowptr.numpy())
    assert S.shape == (67, SC.INT_D) and set(SC.SPECIAL_LENGTHS) <= set(lens.tolist())
    assert int(S.col.max()) == SC.INT_D - 1 and SC.SEG == SEGMENT == 2048
    long_rows, seg_ptr, item_long = segment_items(S.rowptr)
    assert sorted(lens[long_rows.numpy()].tolist()) == [SC.SEG + 1, 3 * SC.SEG + 5]
    assert seg_ptr.tolist() in ([0, 2, 6], [0, 4, 6]) and item_long.numel() == 6
    assert 4 * (3 * SC.SEG + 5) + 4 < 2 ** 24
    x = SC.short_mantissa(np.random.default_rng(0).standard_normal(1000))
    prod = x[:500].astype(np.float64) * x[500:].astype(np.float64)
    assert np.array_equal(prod, (x[:500] * x[500:]).astype(np.float64)), "12-bit numbers: products exact in float32"


# ---- mutations -----------------------------------------------------------------------------------------------------------------
def test_mutation_a_dropped_segment():
    with pytest.raises(AssertionError, match="csr_spmm"):
        SC.check_int_spmm(SC.TorchSparse(mutation="drop_segment"), CPU, SC.int_matrix(), 20)
    with pytest.raises(AssertionError, match="csr_row_sums"):
        SC.check_int_row_sums(SC.TorchSparse(mutation="drop_segment"), CPU, SC.int_matrix())
    SC.check_int_spmm(SC.TorchSparse(mutation="drop_segment"), CPU, SC.one_row_matrix(), 20)     # no long row: unchanged


def test_mutation_the_epilogue_skipped():
    with pytest.raises(AssertionError, match=r"'csr_spmm', 's'"):
        SC.check_int_spmm(SC.TorchSparse(mutation="no_epilogue"), CPU, SC.one_row_matrix(), 20)


def test_mutation_a_ignored():
    """`a` read as ones: S^T Q would lose its centring mu (1^T Q)."""
    with pytest.raises(AssertionError, match=r"'csr_spmm', 'a_s'"):
        SC.check_int_spmm(SC.TorchSparse(mutation="ignore_a"), CPU, SC.int_matrix(), 4)
    with pytest.raises(AssertionError, match="on the transpose"):
        SC.check_transpose(SC.TorchSparse(mutation="ignore_a"), CPU)


def test_mutation_a_transposed_row_out_of_order():
    SC.check_order_bits(SC.TorchSparse(), CPU, 132, transposed=lambda S: S.transposed())
    with pytest.raises(AssertionError, match="leaves the written order"):
        SC.check_order_bits(SC.TorchSparse(), CPU, 132, transposed=SC.swapped_transpose)
    with pytest.raises(AssertionError, match="ascending order"):
        SC.check_transpose(SC.TorchSparse(), CPU, transposed=SC.swapped_transpose)


# ---- the fit, on the double ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", SC.FIT_DIMS)
def test_double_fit_against_exact_pca_and_the_restatement(on_host, dim):
    SC.check_fit_against_exact(CPU, dim)


def test_double_fit_seeds_centre_whiten_rank(on_host, tmp_path):
    SC.check_seeds(CPU)
    SC.check_uncentred(CPU)
    SC.check_whiten(CPU)
    SC.check_rank_deficient(CPU)
    SC.check_transform_and_files(CPU, tmp_path)


def test_restatement_reaches_the_exact_variance():
    Xc, ev = SC.exact_pca()
    for dim in SC.FIT_DIMS:
        C, _ = SC.restated_fit(dim)
        captured = float(((Xc @ C.T) ** 2).sum() / (Xc.shape[0] - 1))
        assert captured >= SC.CAPTURE * float(ev[:dim].sum()), dim


def test_fit_errors_come_before_any_launch(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_hip, "require_gpu", touched)
    monkeypatch.setattr(_hip, "kernels", touched)
    S = SC.rank_five_matrix()
    with pytest.raises(ValueError, match="expected a SparseRows"):
        R.ContentPCA(2).fit_sparse(S.to_dense())
    with pytest.raises(ValueError, match="exceeds min"):
        R.ContentPCA(61).fit_sparse(S)
    with pytest.raises(ValueError, match="dim \\+ oversample = 520 exceeds 512"):
        R.ContentPCA(8).fit_sparse(S, oversample=512)
    with pytest.raises(ValueError, match="power_iterations must be"):
        R.ContentPCA(8).fit_sparse(S, power_iterations=-1)
    with pytest.raises(ValueError, match="fit or load"):
        R.ContentPCA(8).transform_sparse(S)


def test_no_gpu_is_an_error_not_a_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_hip.ClaneHipError, match="no CPU fallback"):
        R.ContentPCA(2).fit_sparse(SC.rank_five_matrix())
    for name in ("csr_spmm_segment", "csr_spmm_ws_len", "csr_spmm", "csr_row_sums"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(_hip.KernelBackend, name)(object(), *([None] * {"csr_spmm_segment": 0, "csr_spmm_ws_len": 3,
                                                                     "csr_spmm": 4, "csr_row_sums": 2}[name]))


# ---- SparseRows ------------------------------------------------------------------------------------------------------------------
def test_sparse_rows_round_trip_sorts_and_sums(tmp_path):
    X = np.zeros((4, 6), dtype=np.float32)
    X[0, [1, 4]], X[2, [0, 5]], X[3, 3] = (2, 3), (1, -1), 7
    S = SparseRows.from_dense(X)
    assert S.shape == (4, 6) and S.nnz == 5 and S.rowptr.tolist() == [0, 2, 2, 4, 5]
    assert S.rowptr.dtype == torch.int64 and S.col.dtype == torch.int32 and S.val.dtype == torch.float32
    assert np.array_equal(S.to_dense().numpy(), X)
    back = SparseRows.load_npz(S.save_npz(tmp_path / "C.npz"))
    assert np.array_equal(back.to_dense().numpy(), X)
    with np.load(tmp_path / "C.npz", allow_pickle=False) as z:
        assert sorted(z.files) == ["data", "format", "indices", "indptr", "shape"]
    # unsorted, with a duplicate: sorted by column, the duplicate summed
    messy = SparseRows([0, 3, 3, 5, 6], [4, 1, 4, 5, 0, 3], [1.0, 2.0, 2.0, -1.0, 1.0, 7.0], (4, 6))
    assert messy.col.tolist() == [1, 4, 0, 5, 3] and np.array_equal(messy.to_dense().numpy(), X)
    T = S.transposed()
    assert T.shape == (6, 4) and np.array_equal(T.to_dense().numpy(), X.T)
    assert np.array_equal(S.rows(2, 4).to_dense().numpy(), X[2:4])
    assert np.array_equal(S.rows(2, 4).transposed().to_dense().numpy(), X[2:4].T)


def test_sparse_rows_validation(tmp_path):
    good = dict(data=np.ones(3, np.float32), indices=np.array([0, 2, 1], np.int32), indptr=np.array([0, 2, 3], np.int64),
                shape=np.array([2, 3]), format=np.asarray(b"csr"))

    def load(**change):
        np.savez(tmp_path / "m.npz", **{**good, **change})
        return SparseRows.load_npz(tmp_path / "m.npz")
    assert load().shape == (2, 3)
    assert load(format=np.asarray("csr")).nnz == 3
    for change, text in ((dict(format=np.asarray(b"csc")), "only 'csr'"),
                         (dict(indptr=np.array([0, 3, 2], np.int64)), "nnz|monotone"),
                         (dict(indptr=np.array([0, 4, 3], np.int64)), "monotone"),
                         (dict(indices=np.array([0, 3, 1], np.int32)), r"outside \[0, 3\)"),
                         (dict(indices=np.array([0, -1, 1], np.int32)), r"outside \[0, 3\)"),
                         (dict(data=np.array([1, np.inf, 1], np.float32)), "non-finite"),
                         (dict(data=np.array([1, np.nan, 1], np.float32)), "non-finite"),
                         (dict(shape=np.array([2, 1 << 31])), "below 2\\^31"),
                         (dict(shape=np.array([1 << 31, 3])), "below 2\\^31")):
        with pytest.raises(ValueError, match=text):
            load(**change)
    np.savez(tmp_path / "short.npz", data=good["data"])
    with pytest.raises(ValueError, match="lacks"):
        SparseRows.load_npz(tmp_path / "short.npz")


# ---- surface -----------------------------------------------------------------------------------------------------------------------
def test_section_keys():
    assert R.check_section({"dim": 8}) == {"dim": 8, "load": None, "center": True, "whiten": False}
    got = R.check_section({"dim": 8, "sparse": "C.npz"})
    assert got == {"dim": 8, "load": None, "center": True, "whiten": False, "sparse": "C.npz", "oversample": 16,
                   "power_iterations": 4, "seed": 0}
    assert R.check_section({"dim": 8, "sparse": "C.npz", "oversample": 4, "power_iterations": 0, "seed": 9})["seed"] == 9
    for section, text in (({"dim": 8, "oversample": 4}, r"\['oversample'\] belong to `sparse`"),
                          ({"dim": 8, "seed": 1, "power_iterations": 2}, ".*belong to `sparse`"),
                          ({"dim": 8, "sparse": 5}, "sparse must be the path"),
                          ({"dim": 8, "sparse": "C.npz", "oversample": -1}, "oversample must be a non-negative"),
                          ({"dim": 8, "sparse": "C.npz", "seed": True}, "seed must be a non-negative"),
                          ({"dim": 500, "sparse": "C.npz"}, r"dim \+ oversample = 516 exceeds 512"),
                          ({"dim": 8, "sparse": "C.npz", "dims": 1}, r"unknown keys \['dims'\]")):
        with pytest.raises(ValueError, match="content_reduction: " + text):
            R.check_section(section)
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        R.check_section({"dim": 8, "sparse": "C.npz"}, world_size=2)


def _args(M, root, out, cfg):
    return M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(out), "--config_file", str(cfg)])


def test_cli_checks_the_sparse_file_before_the_graph_is_loaded(monkeypatch, tmp_path):
    import clane_amd.__main__ as M

    def touched(*a, **k):
        raise AssertionError("the run went on to load the graph")
    monkeypatch.setattr(M, "_distributed_setup", touched)
    monkeypatch.setattr(M, "Graph", touched)
    root = write_data_root(tmp_path / "g", ["a", "b", "c"], ["a", "b"], ["b", "c"])
    cfg = tmp_path / "config.yaml"
    X = np.arange(12, dtype=np.float32).reshape(3, 4)

    def run(body, exc, text):
        cfg.write_text(CONFIG + "\ncontent_reduction:\n" + body)
        with pytest.raises(exc, match=text):
            M.embedding(_args(M, root, tmp_path / "o", cfg))
    run("  dim: 2\n  sparse: C.npz\n", ValueError, "sparse: .*C.npz.* is missing")
    run("  dim: 2\n  oversample: 3\n", ValueError, "belong to `sparse`")
    SparseRows.from_dense(X[:2]).save_npz(root / "C.npz")
    run("  dim: 2\n  sparse: C.npz\n", ValueError, "holds 2 rows, V lists 3 vertices")
    np.savez(root / "C.npz", data=np.ones(1, np.float32), indices=np.array([9], np.int32), indptr=np.array([0, 1, 1, 1]),
             shape=np.array([3, 4]), format=np.asarray(b"csr"))
    run("  dim: 2\n  sparse: C.npz\n", ValueError, r"sparse: .*outside \[0, 4\)")
    np.savez(root / "C.npz", data=np.ones(1, np.float32), indices=np.array([1], np.int32), indptr=np.array([0, 1, 1, 1, 1]),
             shape=np.array([4, 3]), format=np.asarray(b"csc"))
    run("  dim: 2\n  sparse: C.npz\n", ValueError, "only 'csr'")
    SparseRows.from_dense(X).save_npz(root / "C.npz")
    np.save(root / "C.npy", X)
    run("  dim: 2\n  sparse: C.npz\n", ValueError, r"also holds \['C.npy'\].*ambiguous")
    (root / "C.npy").unlink()
    run("  dim: 2\n  sparse: C.npz\n  load: gone.npz\n", ValueError, "is missing")
    monkeypatch.setenv("WORLD_SIZE", "2")
    run("  dim: 2\n  sparse: C.npz\n", NotImplementedError, "ONE GPU")


def test_reduce_sparse_content_guards():
    from clane_amd.graph import Graph
    from clane_amd.partition import HostCSR
    csr = HostCSR(3, np.array([0, 1, 2, 2], dtype=np.int64), np.array([1, 2], dtype=np.int32))
    S = SparseRows.from_dense(np.eye(3, 6, dtype=np.float32))
    g = Graph.from_csr(csr, torch.zeros(3, 6))
    with pytest.raises(ValueError, match="4 rows, the graph 3 vertices"):
        g.reduce_sparse_content(SparseRows.from_dense(np.eye(4, 6, dtype=np.float32)), 2)
    with pytest.raises(ValueError, match="expected a SparseRows"):
        g.reduce_sparse_content(np.eye(3, 6), 2)
    with pytest.raises(ValueError, match="exceeds min"):
        g.reduce_sparse_content(S, 5)
    g._engine = object()
    with pytest.raises(RuntimeError, match="engine exists already"):
        g.reduce_sparse_content(S, 2)
    g._engine = None
    g.set_Z(torch.ones(3, 6))
    with pytest.raises(RuntimeError, match="embeddings were set"):
        g.reduce_sparse_content(S, 2)


def test_abi_rejects_bad_shapes_before_any_launch():
    lib = _hip.load_library()
    p = 1 << 12
    assert lib.clane_csr_spmm_segment() == SEGMENT
    assert lib.clane_csr_spmm_ws_len(10, 100, 8) == 8 and lib.clane_csr_spmm_ws_len(10, 10 * SEGMENT + 5, 8) == 160
    assert lib.clane_csr_spmm_f32(p, p, p, 4, 9, p, 5, 6, 6, None, None, None, None, None, 0, 0, None, 0, p, 8, None) == -1
    assert b"csr_spmm: bad shape" in lib.clane_last_error()                      # l = 6 is no multiple of 4
    assert lib.clane_csr_spmm_f32(p, p, p, 4, 9, p, 5, 8, 516, None, None, None, None, None, 0, 0, None, 0, p, 8, None) == -1
    assert b"csr_spmm: bad shape" in lib.clane_last_error()                      # l > 512
    assert lib.clane_csr_spmm_f32(p, p, p, 4, 9, p, 5, 8, 8, None, None, p, p, p, 1, 2, p, 16, p, 8, None) == -1
    assert b"cannot belong" in lib.clane_last_error()                            # 2 segments in 9 non-zeros
    assert lib.clane_csr_spmm_f32(p, p, p, 4, 9, p + 4, 5, 8, 8, None, None, None, None, None, 0, 0, None, 0, p, 8, None) == -1
    assert b"16-byte aligned" in lib.clane_last_error()
    assert lib.clane_csr_spmm_f32(p, p, p, 4, 3 * SEGMENT, p, 5, 8, 8, None, None, p, p, p, 1, 3, p, 16, p, 8, None) == -1
    assert b"workspace needs 24" in lib.clane_last_error()
    assert lib.clane_csr_row_sums_f32(p, p, -1, 9, None, None, None, 0, 0, None, 0, p, None) == -1
    assert b"csr_row_sums: bad shape" in lib.clane_last_error()
    assert lib.clane_csr_row_sums_f32(p, p, 4, 9, None, None, None, 0, 0, None, 0, None, None) == -1
    assert b"null pointer" in lib.clane_last_error()
    assert _hip.CSR_MAX_L == 512
