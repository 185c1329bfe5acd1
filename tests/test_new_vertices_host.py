"""New vertices against a finished table, without a GPU: the checks of tests/new_vertex_cases.py through
``NewVertexEmbedder`` on a CPU double of the kernel, the checks' own self-checks (mutations that each check must catch),
neighbour normalisation, the config section and the files of the CLI, and the C ABI's host-side argument checks."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from clane_amd import _hip, induct
from clane_amd.induct import NewVertexEmbedder, normalize_neighbours
from clane_amd.similarity import CosineSimilarity

from . import engine_exact_cases as X
from . import new_vertex_cases as N
from .conftest import load_golden, write_data_root
from .exact_cases import BF16, F32, F64
from .oracle_kernels import OracleKernels

ROOT = Path(__file__).resolve().parent.parent


# ---- the CPU double -----------------------------------------------------------------------------------------------------
class InductOracleKernels(OracleKernels):
    """tests/oracle_kernels.py plus the two calls NewVertexEmbedder makes, in plain torch in the accumulate dtype."""

    def project_rows(self, Z, d, W, Y):
        Y[:, :2 * d] = Z[:, :d].to(W.dtype) @ W.T

    def embed_rows(self, rowptr, colidx, X_new, Z, table_rows, d, mode, sums2, sq, S, gamma, tolerence, max_rounds,
                   Z_out, rounds, delta, P_out=None, flags=0):
        acc = delta.dtype
        rp = rowptr.cpu().numpy()
        Zf = Z[:table_rows, :d].to(acc)
        for r in range(X_new.shape[0]):
            a, b = int(rp[r]), int(rp[r + 1])
            x = X_new[r, :d].to(acc)
            z, n, dl, left, best = x.clone(), 0, torch.zeros((), dtype=acc), tolerence, float("inf")
            if b > a:
                cols = colidx[a:b].long()
                Nb = Zf[cols]
                while True:
                    if S is not None:
                        s = S[cols, :d] @ z
                    else:
                        s = Nb @ z
                        if mode == _hip.SCORE_REFERENCE:
                            s = s / (sums2[0].to(acc).sqrt() * sums2[1].to(acc).sqrt())
                        elif mode == _hip.SCORE_PER_EDGE:
                            s = s / (z.pow(2).sum().sqrt() * sq[cols].sqrt())
                    p = torch.softmax(s, 0)
                    zn = x + gamma * (p @ Nb)
                    dl = (zn - z).abs().sum()
                    z, n = zn, n + 1
                    if best > float(dl):
                        left, best = tolerence, float(dl)
                    else:
                        left -= 1
                    if left == 0 or n >= max_rounds or float(dl) == 0.0:
                        break
                if P_out is not None:
                    P_out[a:b] = p
            Z_out[r, :d] = z.to(Z_out.dtype)
            Z_out[r, d:] = 0
            rounds[r] = n
            delta[r] = dl


K = InductOracleKernels()
HOST_CASES = [(F32, 24), (F32, 130), (F64, 24), (F64, 300), (BF16, 3), (BF16, 130)]


@pytest.mark.parametrize("score", N.SCORES)
@pytest.mark.parametrize("case", HOST_CASES, ids=N.case_id)
def test_rounds_against_float64(case, score):
    for n in (1, 2, 6):
        N.check_rounds(K, "cpu", case, score, n)


@pytest.mark.parametrize("score", ("reference", "per_edge"))
@pytest.mark.parametrize("case", [(F32, 24), (F64, 130), (BF16, 3)], ids=N.case_id)
def test_integer_data_is_exact(case, score):
    N.check_integers(K, "cpu", case, score)


@pytest.mark.parametrize("score", N.SCORES)
def test_position_in_the_batch_changes_no_bit(score):
    N.check_position(K, "cpu", (F32, 24), score)


@pytest.mark.parametrize("score", N.SCORES)
def test_degree_one_and_no_neighbours(score):
    N.check_degree_one_and_none(K, "cpu", (F32, 24), score)


@pytest.mark.parametrize("score", N.SCORES)
@pytest.mark.parametrize("case", [(F32, 24), (F64, 24), (BF16, 24)], ids=N.case_id)
def test_every_row_stops_at_its_fixed_point(case, score):
    N.check_stopping(K, "cpu", case, score)


# ---- the checks catch what they should -----------------------------------------------------------------------------------
SHUFFLED = dict(chunks=3, overlap_chunks=False, hot_rows_first=False, shuffle=True, seed=X.SEED)


def _on_shuffled_engine(mutate=None):
    def embed_fn(kernels, dev, t, score, **kw):
        eng = N.make_engine(kernels, dev, t, "reference" if score == "bilinear" else score, **SHUFFLED)
        assert not bool((eng.pos == torch.arange(eng.V)).all())
        if mutate is not None:
            mutate(eng)
        return N.embed(kernels, dev, t, score, eng=eng, **kw)
    return embed_fn


def test_mutation_identity_pos_is_caught():
    N.check_rounds(K, "cpu", (F32, 24), "per_edge", 2, embed_fn=_on_shuffled_engine())

    def identity(eng):
        eng.pos = torch.arange(eng.V)
    with pytest.raises(AssertionError):
        N.check_rounds(K, "cpu", (F32, 24), "per_edge", 2, embed_fn=_on_shuffled_engine(identity))
    N.check_degree_one_and_none(K, "cpu", (F32, 24), "per_edge", embed_fn=_on_shuffled_engine(identity))   # unrelated: still fine


def _after_a_sweep(stale):
    """embed on an engine that has swept once; the restatement reads its get_Z().  `stale`: the norms of the table
    before the sweep are passed off as current."""
    state = {}

    def embed_fn(kernels, dev, t, score, **kw):
        eng = N.make_engine(kernels, dev, t, "reference" if score == "bilinear" else score)
        eng.build_P()                                   # any P moves the table
        before = eng.sq_pp[eng.cur].clone()
        eng.sweep(N.GAMMA)
        assert not eng.sq_ok[eng.cur]
        if stale:
            eng.sq_pp[eng.cur].copy_(before)
            eng.sq_ok[eng.cur] = True
        state["Z"] = eng.get_Z().double()
        return N.embed(kernels, dev, t, score, eng=eng, **kw)
    return embed_fn, state


@pytest.mark.parametrize("stale", (False, True))
def test_mutation_stale_norms_are_caught(stale):
    t = N.table(F32, 24)
    for score, caught in (("per_edge", stale), ("bilinear", False)):          # the bilinear score reads no norms
        embed_fn, state = _after_a_sweep(stale)
        res = embed_fn(K, "cpu", t, score, gamma=N.GAMMA, tolerence=3, max_rounds=2, weights=True)
        _, rowptr, cols, _ = N.batch()
        z = t.X_new.double()
        for _ in range(2):
            z, P = N.restated_round(t, score, rowptr, cols, z, Zt=state["Z"])
        ok = N.O.rel_l2(res.Z.double(), z) <= N.Z_BOUND[F32] and float((res.P.double() - P).abs().max()) <= N.P_BOUND
        assert ok != caught, (score, stale)


def test_mutation_new_edges_in_the_denominator_are_caught():
    t = N.table(F64, 24)
    N.check_rounds(K, "cpu", (F64, 24), "reference", 2)
    _, rowptr, cols, _ = N.batch()
    sq = t.Z.double().pow(2).sum(1)
    csr = N.table_csr()
    outdeg, indeg = np.diff(csr.rowptr), np.bincount(csr.colidx, minlength=N.V) + np.bincount(cols, minlength=N.V)
    # what build_P on the augmented graph would divide by (similarity.py:37), with z = x for the new rows
    a = float((torch.from_numpy(outdeg).double() * sq).sum() + (torch.from_numpy(np.diff(rowptr)).double()
                                                                 * t.X_new.double().pow(2).sum(1)).sum())
    b = float((torch.from_numpy(indeg).double() * sq).sum())
    with pytest.raises(AssertionError):
        N.check_rounds(K, "cpu", (F64, 24), "reference", 2, denom=(a * b) ** 0.5)


def test_mutation_repeated_neighbour_counted_twice_is_caught():
    class Twice(NewVertexEmbedder):
        def _coalesce(self, rowptr, cols, m):
            eng = self.eng
            rowptr = torch.as_tensor(rowptr, dtype=torch.int64)
            src = torch.repeat_interleave(torch.arange(m), rowptr[1:] - rowptr[:-1])
            key = torch.sort(src * eng.V + torch.as_tensor(cols, dtype=torch.int64)).values
            return rowptr, key % eng.V

    def embed_fn(kernels, dev, t, score, **kw):
        eng = N.make_engine(kernels, dev, t, score)
        lists = N.batch()[0]
        rp, cols = normalize_neighbours(lists, N.M)
        return Twice(eng, CosineSimilarity(mode=score)).embed(t.X_new, rp, cols, **kw).cpu()
    with pytest.raises(AssertionError):
        N.check_rounds(K, "cpu", (F32, 24), "per_edge", 1, embed_fn=embed_fn)


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_neighbour_normalisation():
    rp, cols = normalize_neighbours([[3, 1], (), np.array([2]), torch.tensor([5, 5])], 4)
    assert rp.tolist() == [0, 2, 2, 3, 5] and cols.tolist() == [3, 1, 2, 5, 5] and rp.dtype == cols.dtype == np.int64
    rp, cols = normalize_neighbours((np.array([0, 1, 3]), torch.tensor([4, 0, 2])), 2)
    assert rp.tolist() == [0, 1, 3] and cols.tolist() == [4, 0, 2]
    assert normalize_neighbours([], 0)[0].tolist() == [0]
    for bad, m in (([[1]], 2), ((np.array([0, 1]), np.array([1])), 2), ((np.array([1, 1]), np.array([1])), 1),
                   ((np.array([0, 2]), np.array([1])), 1), ((np.array([0, 2, 1]), np.array([1])), 2),
                   ([[0.5]], 1), ([[[1]]], 1), (7, 1), ((np.array([0.0, 1.0]), np.array([1])), 1)):
        with pytest.raises(ValueError, match="neighbours"):
            normalize_neighbours(bad, m)


def test_embedder_refuses_what_it_cannot_do():
    t = N.table(F32, 24)
    eng = N.make_engine(K, "cpu", t)
    emb = NewVertexEmbedder(eng, CosineSimilarity())
    with pytest.raises(ValueError, match="existing vertex"):
        emb.embed(t.X_new[:1], [0, 1], [N.V], gamma=0.5)
    with pytest.raises(ValueError, match="existing vertex"):
        emb.embed(t.X_new[:1], [0, 1], [-1], gamma=0.5)
    with pytest.raises(ValueError, match="X_new"):
        emb.embed(t.X_new[:1, :5], [0, 0], [], gamma=0.5)
    with pytest.raises(ValueError, match="rowptr"):
        emb.embed(t.X_new[:2], [0, 1], [3], gamma=0.5)
    with pytest.raises(ValueError, match="at least 1"):
        emb.embed(t.X_new[:1], [0, 1], [3], gamma=0.5, tolerence=0)
    with pytest.raises(NotImplementedError, match="plug-in"):
        NewVertexEmbedder(eng, lambda a, b: (a * b).sum(1))
    with pytest.raises(ValueError, match="does not fit"):
        NewVertexEmbedder(eng, N.table(F32, 130).sim)
    empty = emb.embed(t.X_new[:0], [0], [], gamma=0.5, weights=True)
    assert empty.Z.shape == (0, 24) and empty.P.numel() == 0
    with pytest.raises(NotImplementedError, match="has no embed_rows"):
        NewVertexEmbedder(N.make_engine(OracleKernels(), "cpu", t), CosineSimilarity()).embed(t.X_new[:1], [0, 1], [3], 0.5)

    class Divided:
        world, columns, halo, exchange = 2, False, True, "halo"
    with pytest.raises(NotImplementedError, match="several GPUs and column divisions are out of scope"):
        NewVertexEmbedder(Divided(), CosineSimilarity())


def test_the_projection_has_a_buffer_of_its_own():
    t = N.table(F32, 24)
    eng = N.make_engine(K, "cpu", t)
    emb = NewVertexEmbedder(eng, t.sim)
    eng._Y = sentinel = torch.full((eng.Zcur.shape[0], 48), 7.0)
    emb.prepare()
    assert eng._Y is sentinel and bool((sentinel == 7.0).all()) and emb._Y is not sentinel      # a LinkRanker's table


# ---- the config section and the files of the CLI --------------------------------------------------------------------------
CONFIG = N.CONFIG


def test_section_validation():
    assert induct.check_section({"root": "a"}) == {"root": "a", "max_rounds": 64, "weights": False}
    assert induct.check_section({"root": "a", "max_rounds": 3, "weights": True})["max_rounds"] == 3
    for bad in (7, {}, {"root": ""}, {"root": 3}, {"root": "a", "rounds": 3}, {"root": "a", "max_rounds": 0},
                {"root": "a", "max_rounds": True}, {"root": "a", "max_rounds": 2.5}, {"root": "a", "weights": "yes"}):
        with pytest.raises(ValueError, match="new_vertices"):
            induct.check_section(bad)
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        induct.check_section({"root": "a"}, world_size=2)


def test_new_vertices_are_refused_on_several_gpus_before_the_graph_is_loaded(monkeypatch, tmp_path):
    import clane_amd.__main__ as M
    monkeypatch.setenv("WORLD_SIZE", "2")

    def touched(*a, **k):
        raise AssertionError("the run went on to set up devices")
    monkeypatch.setattr(M, "_distributed_setup", touched)
    monkeypatch.setattr(M, "Graph", touched)
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG + "\nnew_vertices:\n  root: arrivals\n")
    args = M.get_parser().parse_args(["--data_root", str(tmp_path), "--output_root", str(tmp_path / "o"),
                                      "--config_file", str(cfg)])
    with pytest.raises(NotImplementedError, match="new_vertices: embedding new vertices runs on ONE GPU"):
        M.embedding(args)
    monkeypatch.setenv("WORLD_SIZE", "1")
    cfg.write_text(CONFIG + "\nnew_vertices:\n  max_rounds: 3\n")
    with pytest.raises(ValueError, match="root"):
        M.embedding(args)
    cfg.write_text(CONFIG + "\nnew_vertices:\n  root: arrivals\n")
    (tmp_path / "V").write_text("a\nb\n")
    with pytest.raises(FileNotFoundError, match="arrivals"):             # a missing root: before the graph is read
        M.embedding(args)
    assert set(vars(M.get_parser().parse_args([]))) == {                # no new flag
        "command", "data_root", "output_root", "config_file", "save_history", "num_workers", "init_Z", "exchange",
        "train_similarity", "predict_links", "link_sources", "gpu"}


def test_every_file_error_of_the_arrivals(tmp_path):
    ids = ["a", "b", "c"]
    root = tmp_path / "arrivals"
    new_ids, Xn, rp, cols = induct.read_arrivals(N.write_arrivals(root), ids, 4)
    assert new_ids == ["n0", "n1"] and rp.tolist() == [0, 1, 3] and cols.tolist() == [0, 1, 0] and Xn.shape == (2, 4)
    assert induct.read_arrivals(N.write_arrivals(root, pt=True), ids, None)[1].shape == (2, 4)
    assert induct.read_arrivals(N.write_arrivals(root, E=None), ids, 4)[2].tolist() == [0, 0, 0]      # no E: no neighbours
    with pytest.raises(FileNotFoundError, match="not a directory"):
        induct.read_arrivals(tmp_path / "nowhere", ids, 4)
    with pytest.raises(FileNotFoundError, match="V"):
        induct.read_arrivals(N.write_arrivals(root, V=None), ids, 4)
    with pytest.raises(ValueError, match="'b' already exists"):
        induct.read_arrivals(N.write_arrivals(root, V="n0\nb\n"), ids, 4)
    with pytest.raises(ValueError, match="listed twice"):
        induct.read_arrivals(N.write_arrivals(root, V="n0\nn0\n"), ids, 4)
    with pytest.raises(ValueError, match="source 'a' is not a new vertex"):
        induct.read_arrivals(N.write_arrivals(root, E="a\tb\n"), ids, 4)
    with pytest.raises(ValueError, match="destination 'n1' is not an existing vertex"):
        induct.read_arrivals(N.write_arrivals(root, E="n0\tn1\n"), ids, 4)
    with pytest.raises(ValueError, match="destination 'zz' is not an existing vertex"):
        induct.read_arrivals(N.write_arrivals(root, E="n0\tzz\n"), ids, 4)
    with pytest.raises(ValueError, match="E line 2: expected"):
        induct.read_arrivals(N.write_arrivals(root, E="n0\ta\nn0 a\n"), ids, 4)
    with pytest.raises(FileNotFoundError, match="need their content"):
        induct.read_arrivals(N.write_arrivals(root, C_=None), ids, 4)
    with pytest.raises(ValueError, match=r"content must be \[2, 4\]"):
        induct.read_arrivals(N.write_arrivals(root, C_=np.zeros((2, 5), dtype=np.float32)), ids, 4)
    with pytest.raises(ValueError, match="content must be"):
        induct.read_arrivals(N.write_arrivals(root, C_=np.zeros((3, 4), dtype=np.float32)), ids, None)
    with pytest.raises(ValueError, match="content must be"):
        induct.read_arrivals(N.write_arrivals(root, C_=np.zeros(8, dtype=np.float32)), ids, 4)


def test_cli_end_to_end_on_the_double(tmp_path, monkeypatch):
    N.run_cli_case(tmp_path, monkeypatch, K)


def test_cli_shape_error_names_the_content(tmp_path, monkeypatch):
    import clane_amd.__main__ as M
    k = load_golden("g2_karate_csr.npz")
    Xc = np.zeros((34, 4), dtype=np.float32)
    root = write_data_root(tmp_path / "karate", k["vertex_ids"], k["edge_src"], k["edge_dst"], Xc)
    N.write_arrivals(root / "arrivals", E="", C_=np.zeros((2, 5), dtype=np.float32))

    def touched(*a, **kw):
        raise AssertionError("went on to embed")
    monkeypatch.setattr(M.Embedder, "iterate", touched)
    cfg = tmp_path / "c.yaml"
    cfg.write_text(CONFIG + "\nnew_vertices:\n  root: arrivals\n")
    with pytest.raises(ValueError, match=r"content must be \[2, 4\]"):      # known once the graph is: before any sweep
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / "o"),
                                               "--config_file", str(cfg)]))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_at_abi_5():
    text = (ROOT / "include" / "clane_hip.h").read_text()
    assert re.search(r"#define CLANE_ABI_VERSION 5\b", text) and _hip.ABI_VERSION == 5
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for suffix in ("f32", "f64", "bf16"):
        assert re.search(rf"\bint clane_embed_rows_{suffix}\s*\(", code)
        assert f"clane_embed_rows_{suffix}" in _hip.SIGNATURES
    assert "graph.py:118-128" in text and "embedder.py:84-92" in text


def test_argument_validation_reaches_last_error():
    lib = _hip.load_library()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    good = dict(rowptr=p, colidx=p, m=2, X=p, ldx=8, Z=p, rows=4, ldz=8, d=8, mode=1, sums2=p, sq=p, S=None, lds=0,
                gamma=0.5, tol=10, max_rounds=8, flags=0, out=p, ldo=8, rounds=p, delta=p, P=None)

    def call(fn=lib.clane_embed_rows_f32, **change):
        a = dict(good, **change)
        return fn(*[a[n] for n in good], None)
    for change, text in ((dict(m=-1), b"m = -1"), (dict(rows=-3), b"table_rows"), (dict(d=0), b"d = 0"),
                         (dict(ldx=7), b"ldx"), (dict(ldz=4), b"ldz"), (dict(ldo=3), b"ldo"), (dict(mode=7), b"unknown mode 7"),
                         (dict(S=p, lds=8), b"S (the projected table) goes with mode RAW_DOT"),
                         (dict(mode=2), b"mode RAW_DOT needs S"), (dict(mode=2, S=p, lds=4), b"lds"),
                         (dict(mode=0, sums2=None), b"sums2"), (dict(sq=None), b"sq"), (dict(tol=0), b"tolerence = 0"),
                         (dict(max_rounds=0), b"max_rounds = 0"), (dict(flags=64), b"flags"), (dict(out=None), b"Z_out"),
                         (dict(rounds=None), b"rounds"), (dict(delta=None), b"delta"), (dict(rowptr=None), b"rowptr"),
                         (dict(X=None), b"X_new"), (dict(Z=None), b"Z"), (dict(d=5000, ldx=5000, ldz=5000, ldo=5000), b"d = 5000")):
        assert call(**change) == -1, change
        assert text in lib.clane_last_error() and b"embed_rows" in lib.clane_last_error(), (change, lib.clane_last_error())
    assert call(m=0, rowptr=None, X=None) == 0                                   # nothing to do
    assert call(fn=lib.clane_embed_rows_f64, d=0) == -1 and call(fn=lib.clane_embed_rows_bf16, tol=-1) == -1
