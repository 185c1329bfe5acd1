"""Content reduction without a GPU: the config section, the error paths that come before any launch, the file format, the
sign rule -- and a plain-torch double of the three calls (tests/reduce_cases.py: TorchPca) run through the exact checks
the HIP kernels get in tests/test_gpu_reduce.py, with four mutations that each fail the check they should."""
import json

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd import reduce as R

from . import reduce_cases as RC
from .conftest import write_data_root

ids = RC.case_id
CPU = torch.device("cpu")
CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


# ---- the double passes the exact checks -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", RC.DTYPES, ids=ids)
@pytest.mark.parametrize("d", RC.INT_D)
@pytest.mark.parametrize("n", RC.INT_N)
def test_double_sums_and_gram_on_integer_data(dtype, n, d):
    RC.check_int_sums(RC.TorchPca(), CPU, dtype, n, d)
    RC.check_int_gram(RC.TorchPca(), CPU, dtype, n, d)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=ids)
@pytest.mark.parametrize("d", RC.INT_D)
@pytest.mark.parametrize("n", RC.INT_N)
def test_double_projection_on_integer_data(dtype, n, d):
    for m in RC.INT_M:
        RC.check_int_affine(RC.TorchPca(), CPU, dtype, n, d, m)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=ids)
@pytest.mark.parametrize("data", ["int", "float"])
def test_double_streams_to_the_one_call_bits(dtype, data):
    RC.check_streaming(RC.TorchPca(), CPU, dtype, 130, data)


def test_int_fixture_is_what_it_says():
    for n in RC.INT_N:
        X, rows, mu = RC.int_case(n, 130, "true")
        ok = RC.present_mask(rows, X.shape[0])
        assert int(X.abs().max()) <= 2 and int(mu.abs().max()) <= 1
        assert torch.equal(X[rows[ok].long()].sum(0), mu * int(ok.sum()))          # the mean is the integer vector
        if n >= 3:
            assert int(rows[0]) == int(rows[1]) and int(rows[2]) >= X.shape[0] and int((~ok).sum()) == 1
        _, G, Xc = RC.int_reference(X, rows, mu)
        assert int(G.abs().max()) < 2 ** 24 and int(Xc[~ok].abs().sum()) == 0
    assert bool(torch.isnan(RC.place(X, RC.F32, CPU).as_strided((X.shape[0], 133), (133, 1))[:, 130:]).all())


# ---- mutations --------------------------------------------------------------------------------------------------------------
def test_mutation_a_dropped_chunk():
    k = RC.TorchPca("drop_chunk")
    for n in (2049, 4300):
        with pytest.raises(AssertionError, match="column sums"):
            RC.check_int_sums(k, CPU, RC.F32, n, 130)
        with pytest.raises(AssertionError, match="gram"):
            RC.check_int_gram(k, CPU, RC.F32, n, 130)
    RC.check_int_sums(k, CPU, RC.F32, 130, 130)                  # one chunk: nothing to drop
    RC.check_int_gram(k, CPU, RC.F32, 130, 130)
    RC.check_int_affine(k, CPU, RC.F32, 4300, 130, 5)


def test_mutation_the_mirror_tile_not_written():
    k = RC.TorchPca("no_mirror")
    for d in (130, 257):
        with pytest.raises(AssertionError, match="not symmetric"):
            RC.check_int_gram(k, CPU, RC.F64, 130, d)
    RC.check_int_gram(k, CPU, RC.F64, 130, 2)                    # one tile: it is its own mirror
    RC.check_int_sums(k, CPU, RC.F64, 130, 257)
    RC.check_int_affine(k, CPU, RC.F64, 130, 257, 5)


def test_mutation_mu_subtracted_from_one_operand():
    k = RC.TorchPca("mu_one_operand")
    with pytest.raises(AssertionError, match="'integer'"):
        RC.check_int_gram(k, CPU, RC.BF16, 130, 130)
    X, rows, _ = RC.int_case(130, 130, "none")                   # without mu there is nothing to forget
    _, want, _ = RC.int_reference(X, rows, None)
    assert torch.equal(RC.run_gram(k, RC.place(X, RC.BF16, CPU), 130, rows, None), want.float())
    RC.check_int_sums(k, CPU, RC.BF16, 130, 130)
    RC.check_int_affine(k, CPU, RC.BF16, 130, 130, 5)


def test_mutation_a_pad_column_read(monkeypatch):
    k = RC.TorchPca("read_pad")
    with pytest.raises(AssertionError, match="column sums"):
        RC.check_int_sums(k, CPU, RC.F32, 130, 130)
    with pytest.raises(AssertionError, match="(?i)gram"):
        RC.check_int_gram(k, CPU, RC.F32, 130, 130)
    with pytest.raises(AssertionError, match="project_affine"):
        RC.check_int_affine(k, CPU, RC.F32, 130, 130, 5)
    monkeypatch.setattr(RC, "PAD", 0)                            # no pad column: nothing to read
    RC.check_int_sums(k, CPU, RC.F32, 130, 130)
    RC.check_int_gram(k, CPU, RC.F32, 130, 130)


def test_derived_bound_holds_for_chunked_fp32_sums_on_the_host():
    """The fixture and the bound, with numpy's fp32 products in 2048-row chunks standing in for the kernel."""
    X = RC.planted_matrix(RC.F32)
    mean = X.double().mean(0).float()
    G64, bound = RC.gram_bound(X, mean.double(), RC.F32)
    Xc = X - mean
    G = sum((Xc[a:a + RC.CHUNK].T @ Xc[a:a + RC.CHUNK]) for a in range(0, X.shape[0], RC.CHUNK))
    assert float(((G.double() - G64).abs() / bound).max()) < 1.0
    lam, comp, gaps = RC.reference_axes(G64, 5)
    assert np.allclose(lam[:5] / (X.shape[0] - 1), RC.PLANTED, rtol=0.25)
    assert (2 * float(torch.linalg.norm(bound)) / gaps < 0.1).all()              # non-vacuous


# ---- host logic of reduce.py ------------------------------------------------------------------------------------------------
def test_sign_rule_on_a_hand_made_matrix():
    comp = np.array([[0.1, -0.9, 0.3], [-0.5, 0.5, 0.2], [0.5, -0.5, -0.2], [0.0, 0.0, -1.0]])
    got = R.fix_signs(comp)
    assert np.array_equal(got[0], -comp[0])                      # the largest entry was negative
    assert np.array_equal(got[1], -comp[1])                      # a tie of magnitudes: the lowest index decides
    assert np.array_equal(got[2], comp[2])
    assert np.array_equal(got[3], [0.0, 0.0, 1.0])
    assert np.array_equal(comp[0], [0.1, -0.9, 0.3])             # the input is not written


def test_principal_axes_of_a_diagonal_gram():
    G = torch.diag(torch.tensor([2.0, 8.0, -1e-9, 4.0]))
    comp, var, total, rank = R.principal_axes(G, n=5, dim=3)
    assert np.allclose(var, [2.0, 1.0, 0.5]) and np.isclose(total, 3.5) and rank == 3          # descending, / (n - 1), clamped at 0
    assert np.allclose(np.abs(comp), np.eye(4)[[1, 3, 0]]) and (comp.sum(1) > 0).all()


def test_block_rows_rule():
    for d, dtype in ((1433, RC.F32), (1024, RC.BF16), (8, RC.F64), (32768, RC.F64)):
        rows = R.default_block_rows(d, dtype)
        elt, acc = torch.empty(0, dtype=dtype).element_size(), torch.empty(0, dtype=_hip.acc_dtype(dtype)).element_size()
        assert rows % R.CHUNK_ROWS == 0 and R.CHUNK_ROWS <= rows <= R.CHUNK_ROWS * R.MAX_CHUNKS
        if rows > R.CHUNK_ROWS:
            assert rows * d * elt + rows // R.CHUNK_ROWS * d * d * acc <= R.BLOCK_BYTE_BUDGET
    for bad in (0, 1000, 2049, -2048):
        with pytest.raises(ValueError, match="multiple of 2048"):
            R.ContentPCA(2, block_rows=bad)


def test_errors_come_before_any_launch(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("a device or the library was asked for")
    monkeypatch.setattr(_hip, "require_gpu", touched)
    monkeypatch.setattr(_hip, "kernels", touched)
    for dim in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="dim must be a positive integer"):
            R.ContentPCA(dim)
    X = torch.zeros(10, 4)
    with pytest.raises(ValueError, match=r"exceeds min\(d, n - 1\) = 4"):
        R.ContentPCA(5).fit(X)
    with pytest.raises(ValueError, match=r"exceeds min\(d, n - 1\) = 2"):
        R.ContentPCA(3).fit(X[:3])
    with pytest.raises(ValueError, match="at least 2 rows"):
        R.ContentPCA(1).fit(X[:1])
    for bad in (torch.zeros(4), torch.zeros(2, 3, 4)):
        with pytest.raises(ValueError, match="2-D"):
            R.ContentPCA(1).fit(bad)
    with pytest.raises(TypeError, match="float32, float64 and bfloat16"):
        R.ContentPCA(1).fit(torch.zeros(4, 4, dtype=torch.float16))
    with pytest.raises(ValueError, match="fit or load"):
        R.ContentPCA(1).transform(X)
    with pytest.raises(ValueError, match="nothing is fitted"):
        R.ContentPCA(1).save("unused.npz")


def test_no_gpu_is_an_error_not_a_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_hip.ClaneHipError, match="no CPU fallback"):
        R.ContentPCA(2).fit(torch.randn(10, 4))


def hand_made_pca(whiten=False):
    pca = R.ContentPCA(2, center=True, whiten=whiten)
    pca.components_ = np.array([[0.6, 0.8, 0.0], [0.0, 0.0, 1.0]])
    pca.mean_ = np.array([1.0, 2.0, 3.0])
    pca.explained_variance_ = np.array([4.0, 1.0])
    pca.explained_variance_ratio_ = np.array([0.8, 0.2])
    pca.total_variance_, pca.n_samples_, pca.fitted_from = 5.0, 9, "fit"
    return pca


def test_npz_format_round_trips(tmp_path):
    pca = hand_made_pca(whiten=True)
    path = pca.save(tmp_path / "pca.npz")
    with np.load(path) as z:
        assert sorted(z.files) == sorted(R.NPZ_KEYS)
        assert z["components"].dtype == np.float64 and z["components"].shape == (2, 3) and int(z["dim"]) == 2
        assert bool(z["center"]) and bool(z["whiten"]) and int(z["n_samples"]) == 9
    back = R.ContentPCA.load(path)
    for name in ("components_", "mean_", "explained_variance_", "explained_variance_ratio_"):
        assert np.array_equal(getattr(back, name), getattr(pca, name)), name
    assert (back.dim, back.center, back.whiten, back.total_variance_, back.n_samples_) == (2, True, True, 5.0, 9)
    assert back.fitted_from == "load"
    rep = back.report(3)
    assert set(rep) == {"input_width", "output_width", "n", "explained_variance_ratio", "explained_variance_ratio_sum",
                        "center", "whiten", "source"}
    assert rep["source"] == "load" and rep["input_width"] == 3 and rep["output_width"] == 2
    assert json.loads(json.dumps(rep)) == rep
    np.savez(tmp_path / "short.npz", components=pca.components_)
    with pytest.raises(ValueError, match="lacks"):
        R.ContentPCA.load(tmp_path / "short.npz")


def test_section_checking(tmp_path):
    ok = R.check_section({"dim": 8})
    assert ok == {"dim": 8, "load": None, "center": True, "whiten": False}
    assert R.check_section({"load": "pca.npz", "whiten": True})["dim"] is None
    for section, text in (({"dim": 8, "dims": 2}, r"unknown keys \['dims'\]"), ({}, "`dim`.*is required unless `load`"),
                          ({"dim": 0}, "dim must be a positive integer"), ({"dim": "8"}, "dim must be a positive integer"),
                          ({"dim": True}, "dim must be a positive integer"), ({"dim": 2, "center": 1}, "center must be true"),
                          ({"dim": 2, "whiten": "no"}, "whiten must be true"), ({"dim": 2, "load": 5}, "load must be"),
                          ([8], "expected a mapping")):
        with pytest.raises(ValueError, match="content_reduction: " + text):
            R.check_section(section)
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        R.check_section({"dim": 8}, world_size=2)
    with pytest.raises(ValueError, match="load: .*nowhere.npz.* is missing"):
        R.resolve_load(R.check_section({"load": "nowhere.npz"}), tmp_path)
    (tmp_path / "there.npz").write_bytes(b"")
    assert R.resolve_load(R.check_section({"load": "there.npz"}), tmp_path) == tmp_path / "there.npz"
    assert R.resolve_load(R.check_section({"dim": 3}), tmp_path) is None


def _args(M, root, out, cfg):
    return M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(out), "--config_file", str(cfg)])


def test_cli_checks_the_section_before_the_graph_is_loaded(monkeypatch, tmp_path):
    import clane_amd.__main__ as M

    def touched(*a, **k):
        raise AssertionError("the run went on to load the graph")
    monkeypatch.setattr(M, "_distributed_setup", touched)
    monkeypatch.setattr(M, "Graph", touched)
    cfg = tmp_path / "config.yaml"
    for body, exc, text in (("  dim: 0\n", ValueError, "positive integer"), ("  dim: 4\n  scale: true\n", ValueError, "unknown keys"),
                            ("  load: gone.npz\n", ValueError, "is missing"), ("  center: true\n", ValueError, "is required")):
        cfg.write_text(CONFIG + "\ncontent_reduction:\n" + body)
        with pytest.raises(exc, match=text):
            M.embedding(_args(M, tmp_path, tmp_path / "o", cfg))
    monkeypatch.setenv("WORLD_SIZE", "2")
    cfg.write_text(CONFIG + "\ncontent_reduction:\n  dim: 2\n")
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        M.embedding(_args(M, tmp_path, tmp_path / "o", cfg))
    assert "content_reduction" not in vars(M.get_parser().parse_args([]))        # a section, no new flag


def test_cli_arrivals_must_have_the_original_width(monkeypatch, tmp_path):
    import clane_amd.__main__ as M
    from clane_amd.graph import Graph
    from .new_vertex_cases import write_arrivals

    def touched(*a, **k):
        raise AssertionError("the content was reduced before the arrivals' width was checked")
    monkeypatch.setattr(Graph, "reduce_content", touched)
    root = write_data_root(tmp_path / "g", ["a", "b", "c"], ["a", "b"], ["b", "c"], np.zeros((3, 6), dtype=np.float32))
    write_arrivals(root / "arrivals", C_=np.zeros((2, 4), dtype=np.float32))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG + "\ncontent_reduction:\n  dim: 4\n\nnew_vertices:\n  root: arrivals\n")
    with pytest.raises(ValueError, match=r"ORIGINAL width 6 .*reduced to 4.* got \(2, 4\)"):
        M.embedding(_args(M, root, tmp_path / "o", cfg))


def test_reduce_content_is_refused_once_an_engine_exists():
    from clane_amd.graph import Graph
    from clane_amd.partition import HostCSR
    csr = HostCSR(3, np.array([0, 1, 2, 2], dtype=np.int64), np.array([1, 2], dtype=np.int32))
    g = Graph.from_csr(csr, torch.zeros(3, 6))
    g._engine = object()
    with pytest.raises(RuntimeError, match="engine exists already"):
        g.reduce_content(2)
    g._engine = None
    g.set_Z(torch.ones(3, 6))
    with pytest.raises(RuntimeError, match="embeddings were set"):
        g.reduce_content(2)


def test_abi_rejects_bad_shapes_before_any_launch():
    lib = _hip.load_library()
    p = 1 << 12
    assert lib.clane_column_sums_f32(p, 4, 0, 4, p, 4, 0, p, p, None) == -1 and b"column_sums: bad shape" in lib.clane_last_error()
    assert lib.clane_column_sums_f64(p, 4, 4, 4, p, 4, 2, p, p, None) == -1 and b"unknown flags" in lib.clane_last_error()
    assert lib.clane_gram_bf16(p, 4, 8, 4, p, 4, None, 0, p, p, None) == -1 and b"gram: bad shape" in lib.clane_last_error()
    assert lib.clane_gram_f32(p, 4, 4, 4, p, 4, None, 0, None, p, None) == -1 and b"null workspace" in lib.clane_last_error()
    assert lib.clane_project_affine_f32(p, 4, 4, 4, p, 4, None, p, 3, p, 2, None) == -1
    assert b"project_affine: bad shape" in lib.clane_last_error()
    assert lib.clane_project_affine_f64(p, 4, 4, 4, p, 4, None, None, 3, p, 3, None) == -1
    assert b"null pointer" in lib.clane_last_error()
    assert lib.clane_gram_ws_len(4300, 130) == 3 * 130 * 130 and lib.clane_column_sums_ws_len(2048, 7) == 7
    assert lib.clane_gram_ws_len(0, 5) == 25
    assert _hip.PCA_ACCUMULATE == 1
