"""The bilinear similarity (AsymmertricSimilarity) through Graph.build_P / Embedder / SweepEngine.build_P_bilinear, on
the CPU: a torch fp64 restatement pinned to a fixture made by the real reference (g13), the host logic driven by
substitute kernels, and the argument checks of the new C-ABI entries (no GPU needed for any of them)."""
import ctypes as C
import math
import threading

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.embedder import Embedder
from clane_amd.engine import SweepEngine
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR
from clane_amd.similarity import AsymmertricSimilarity
from clane_amd.xcd import xcd_class
from oracle import clane_oracle as O

from .conftest import load_golden, write_data_root
from .oracle_kernels import OracleKernels, item_stats
from .thread_comm import ThreadWorld

GOLD = "g13_karate_asym_d16.npz"


# ---- the restatement ---------------------------------------------------------------------------
def bilinear_P(rowptr, colidx, Z, Phi_src, Phi_dst):
    """Row softmax of s(u, v) = (Phi_src z_u) . (Phi_dst z_v) over the CSR edges (u: the row, v: the neighbour),
    in fp64 (similarity.py:54-57 + graph.py:118-128)."""
    Z, Ws, Wd = (torch.as_tensor(t).double() for t in (Z, Phi_src, Phi_dst))
    rows = torch.from_numpy(np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)))
    cols = torch.from_numpy(np.asarray(colidx, dtype=np.int64))
    scores = ((Z @ Ws.T)[rows] * (Z @ Wd.T)[cols]).sum(1)
    return O.segment_softmax(rowptr, scores)


def bilinear_iterate(rowptr, colidx, X, Phi_src, Phi_dst, gamma, tol):
    """Embedder.iterate (embedder.py:56-108) with the bilinear P rebuilt from Z every round, in fp64."""
    X = torch.as_tensor(X).double()
    Z, counts, best_outer, t_outer = X.clone(), [], math.inf, tol
    while True:
        prev = Z.clone()
        P = bilinear_P(rowptr, colidx, Z, Phi_src, Phi_dst)
        Ps = O.as_sparse(rowptr, colidx, P)
        best, t, n = math.inf, tol, 0
        while True:
            Z, amount = O.sweep(rowptr, colidx, P, X, Z, gamma, Ps)
            n += 1
            if best > amount:
                best, t = amount, tol
            else:
                t -= 1
            if t == 0:
                break
        counts.append(n)
        amount = (Z - prev).abs().sum()
        if best_outer > amount:
            best_outer, t_outer = amount, tol
        else:
            t_outer -= 1
        if t_outer == 0:
            return Z, counts


# ---- substitute kernels with the three new calls ---------------------------------------------------
class BilinearOracleKernels(OracleKernels):
    def project_rows(self, Z, d, W, Y):
        Y[:, :2 * d] = Z[:, :d].to(W.dtype) @ W.T

    def edge_score_pair(self, rowptr, colidx, nrows, row0, S, N, d, scores, long_threshold=0, long_rows=None,
                        fuse_softmax=False):
        rp = rowptr[:nrows + 1].cpu().numpy()
        if rp[-1] == rp[0]:
            return
        rows = torch.from_numpy(np.repeat(np.arange(nrows), np.diff(rp))) + row0
        cols = colidx[rp[0]:rp[-1]].long()
        scores[rp[0]:rp[-1]] = (S[rows, :d] * N[cols, :d]).sum(1)
        if fuse_softmax:
            for r in range(nrows):
                if rp[r + 1] > rp[r]:
                    scores[rp[r]:rp[r + 1]] = torch.softmax(scores[rp[r]:rp[r + 1]], 0)

    def edge_score_class_pair(self, rowptr, colidx, item_e0, item_len, item_slot, item_row, items_per_block,
                              class_rows, slot_ptr, row0, S, N, d, scores, stats=None, fuse_softmax=False,
                              n_slots=None, row_parts=1):
        assert n_slots is None or n_slots == int(slot_ptr[-1])
        e0, ln, rw = (t.cpu().numpy() for t in (item_e0, item_len, item_row))
        assert 4 <= items_per_block <= 64 and e0.size % items_per_block == 0 and e0.size // items_per_block % 8 == 0
        listed = set(class_rows.tolist())
        for k in range(e0.size):
            if ln[k] == 0:
                continue
            a, b = int(e0[k]), int(e0[k]) + int(ln[k])
            cols = colidx[a:b].long()
            assert bool((xcd_class(cols) == (k // items_per_block) % 8).all()) and int(rw[k]) in listed
            scores[a:b] = (S[row0 + int(rw[k]), :d].unsqueeze(0) * N[cols, :d]).sum(1)
            if fuse_softmax and stats is not None:
                item_stats(stats, int(item_slot[k]), scores[a:b])
        if fuse_softmax:
            rp = rowptr.cpu().numpy()
            for r in class_rows.tolist():
                scores[rp[r]:rp[r + 1]] = torch.softmax(scores[rp[r]:rp[r + 1]], 0)


def _sim(gold, dtype=torch.float32):
    sim = AsymmertricSimilarity(int(gold["X"].shape[1]))
    with torch.no_grad():
        sim.Phi_src.weight.copy_(torch.from_numpy(gold["Phi_src"]))
        sim.Phi_dst.weight.copy_(torch.from_numpy(gold["Phi_dst"]))
    return sim.to(dtype)


def _graph(tmp_path, gold, **engine_kw):
    k = load_golden("g2_karate_csr.npz")
    root = write_data_root(tmp_path / "karate_asym", k["vertex_ids"], k["edge_src"], k["edge_dst"], gold["X"])
    g = Graph(root, embedding_dim=int(gold["X"].shape[1]))
    eng = SweepEngine(g.csr, g.X, "cpu", BilinearOracleKernels(), **engine_kw)
    g._attach_engine(eng)
    return g


def _forbid_forward(sim):
    def forward(*a, **k):
        raise AssertionError("the bilinear path must not call the module's forward")
    sim.forward = forward
    return sim


# ---- the restatement against the real reference -------------------------------------------------
def test_restatement_reproduces_the_reference_golden():
    gold = load_golden(GOLD)
    idx = gold["A_indices"]
    rowptr, colidx = O.build_csr(34, idx[0], idx[1])
    P = bilinear_P(rowptr, colidx, gold["X"], gold["Phi_src"], gold["Phi_dst"])
    np.testing.assert_allclose(P.numpy(), gold["P_values"], rtol=1e-5, atol=1e-7)
    # the sides are not interchangeable: the CSR row is the source (Phi_src), the neighbour the destination (Phi_dst)
    swapped = bilinear_P(rowptr, colidx, gold["X"], gold["Phi_dst"], gold["Phi_src"])
    assert not np.allclose(swapped.numpy(), gold["P_values"], rtol=1e-3, atol=1e-5)
    Z, counts = bilinear_iterate(rowptr, colidx, gold["X"], gold["Phi_src"], gold["Phi_dst"], float(gold["gamma"]),
                                 int(gold["tolerence"]))
    assert O.rel_l2(Z, torch.from_numpy(gold["Z_final"])) < 1e-5
    # sweep counts depend on last-ulp noise near the fixed point: bounded, never pinned
    assert abs(counts[0] - int(gold["sweep_counts"][0])) <= 3


# ---- host logic with substitute kernels ----------------------------------------------------------------
def test_graph_build_P_matches_reference_without_forward(tmp_path):
    gold = load_golden(GOLD)
    g = _graph(tmp_path, gold)
    sim = _forbid_forward(_sim(gold))
    P = g.build_P(sim)
    assert P.is_coalesced() and P.shape == (34, 34)
    np.testing.assert_array_equal(P.indices().numpy(), gold["A_indices"])
    np.testing.assert_allclose(P.values().numpy(), gold["P_values"], rtol=1e-5, atol=1e-7)
    assert g._engine.P_valid


def test_embedder_iterate_matches_reference(tmp_path):
    gold = load_golden(GOLD)
    g = _graph(tmp_path, gold)
    sim = _forbid_forward(_sim(gold))
    emb = Embedder(g, sim, torch.device("cpu"), gamma=float(gold["gamma"]), tolerence=int(gold["tolerence"]),
                   verbose=False)
    emb.iterate()
    assert O.rel_l2(g.Z, torch.from_numpy(gold["Z_final"])) < 1e-5
    assert emb.tolerences["global"].value == 0 and emb.tolerences["propagation"].value == 0
    assert abs(emb.sweep_counts[0] - int(gold["sweep_counts"][0])) <= 3
    assert len(emb.sweep_counts) >= int(gold["tolerence"])


def test_embedder_does_not_take_P_through_the_host(tmp_path, monkeypatch):
    gold = load_golden(GOLD)
    g = _graph(tmp_path, gold)
    monkeypatch.setattr(Graph, "_gather_P", lambda *a, **k: pytest.fail("P went through the host"))
    emb = Embedder(g, _sim(gold), torch.device("cpu"), gamma=float(gold["gamma"]), tolerence=2, verbose=False)
    emb.propagate()
    assert g._engine.P_valid and emb.sweep_counts[0] >= 2


def test_changed_weights_give_a_new_P(tmp_path):
    gold = load_golden(GOLD)
    g = _graph(tmp_path, gold)
    sim = _sim(gold)
    first = g.build_P(sim).values().clone()
    with torch.no_grad():
        sim.Phi_dst.weight.mul_(-2.0)
    second = g.build_P(sim).values()
    assert not torch.allclose(first, second)
    idx = gold["A_indices"]
    rowptr, colidx = O.build_csr(34, idx[0], idx[1])
    want = bilinear_P(rowptr, colidx, gold["X"], gold["Phi_src"], -2.0 * gold["Phi_dst"])
    np.testing.assert_allclose(second.numpy(), want.numpy(), rtol=1e-5, atol=1e-7)


def test_dimension_mismatch_raises(tmp_path):
    gold = load_golden(GOLD)
    g = _graph(tmp_path, gold)
    with pytest.raises(ValueError, match="n_dim=8"):
        g.build_P(AsymmertricSimilarity(8))
    emb = Embedder(g, AsymmertricSimilarity(32), torch.device("cpu"), verbose=False)
    with pytest.raises(ValueError, match="n_dim=32"):
        emb.propagate()


def test_column_division_is_refused():
    gold = load_golden(GOLD)
    idx = gold["A_indices"]
    rowptr, colidx = O.build_csr(34, idx[0], idx[1])
    comm = ThreadWorld(1).comm(0)
    comm.force = True                       # a one-rank group that keeps the division it is given
    eng = SweepEngine(HostCSR(34, rowptr, colidx), torch.from_numpy(gold["X"]), "cpu", BilinearOracleKernels(),
                      comm=comm, exchange="columns")
    assert eng.columns
    W = _sim(gold).stacked_weight(torch.float32, "cpu")
    with pytest.raises(NotImplementedError, match="exchange='halo'"):
        eng.build_P_bilinear(W)


def _skewed_csr(V, seed):
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 9, V)
    deg[rng.integers(V)] = V                                     # one hub that points at everybody
    deg[rng.integers(V)] = 0
    cols = [np.sort(rng.choice(V, size=k, replace=False)) for k in deg]
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    return HostCSR(V, rowptr, np.concatenate(cols + [np.empty(0, int)]).astype(np.int32))


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", ["halo", "allgather", "allgather_all"])
@pytest.mark.parametrize("class_threshold", [None, 3])
def test_row_divisions_match_one_rank(world, mode, class_threshold):
    V, d = 90, 12
    csr = _skewed_csr(V, seed=world * 7 + len(mode))
    rng = np.random.default_rng(1)
    X = torch.from_numpy(rng.standard_normal((V, d)).astype(np.float32))
    W = torch.from_numpy(rng.standard_normal((2 * d, d)).astype(np.float32)) / math.sqrt(d)
    want = bilinear_P(csr.rowptr, csr.colidx, X, W[:d], W[d:])
    one = SweepEngine(csr, X, "cpu", BilinearOracleKernels(), class_threshold=class_threshold, class_chunk=64)
    one.build_P_bilinear(W)
    P_one = one.P_global()
    np.testing.assert_allclose(P_one.numpy(), want.numpy(), rtol=1e-5, atol=1e-7)

    shared, results, errors = ThreadWorld(world), [None] * world, []

    def run(rank):
        try:
            eng = SweepEngine(csr, X, "cpu", BilinearOracleKernels(), comm=shared.comm(rank), chunks=2, exchange=mode,
                              seed=world, class_threshold=class_threshold, class_chunk=64)
            eng.build_P_bilinear(W)
            P_mine = torch.zeros(csr.num_edges)
            P_mine[torch.from_numpy(eng.local.edge_origin)] = eng.P[:eng.E_loc]
            owned = torch.zeros(csr.num_edges, dtype=torch.bool)
            owned[torch.from_numpy(eng.local.edge_origin)] = True
            results[rank] = (P_mine, owned)
        except Exception as exc:
            errors.append((rank, exc))
            shared.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    covered = torch.zeros(csr.num_edges, dtype=torch.int32)
    for P_mine, owned in results:
        assert torch.allclose(P_mine[owned], P_one[owned], rtol=1e-6, atol=1e-8)
        covered += owned.int()
    assert bool((covered == 1).all())                  # every row's P is made by exactly one rank


def test_backend_contract_is_optional():
    kern = OracleKernels()                   # the existing double still instantiates without the new calls
    for call in (lambda: kern.project_rows(None, 1, None, None),
                 lambda: kern.edge_score_pair(None, None, 0, 0, None, None, 1, None),
                 lambda: kern.edge_score_class_pair(None, None, None, None, None, None, 4, None, None, 0, None, None, 1,
                                                    None)):
        with pytest.raises(NotImplementedError):
            call()
    eng = SweepEngine(_skewed_csr(20, 0), torch.zeros(20, 4), "cpu", kern)
    with pytest.raises(NotImplementedError, match="project_rows"):
        eng.build_P_bilinear(torch.zeros(8, 4))


# ---- the C ABI's host-side checks (no launch) --------------------------------------------------------
def test_abi_argument_checks_without_a_gpu():
    lib = _hip.load_library()
    assert lib.clane_abi_version() == 5
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.clane_project_rows_f32(p, 4, 8, 4, p, p, 16, None) == -1          # ldz < d
    assert b"project_rows" in lib.clane_last_error()
    assert lib.clane_project_rows_f64(p, 4, 8, 8, p, p, 15, None) == -1          # ldy < 2d
    assert lib.clane_project_rows_bf16(p, 4, 0, 8, p, p, 16, None) == -1         # d < 1
    assert lib.clane_project_rows_f32(None, 4, 8, 8, p, p, 16, None) == -1       # null Z
    assert b"null pointer" in lib.clane_last_error()
    assert lib.clane_project_rows_f32(None, 0, 8, 8, None, None, 16, None) == 0  # nothing to do
    assert lib.clane_edge_score_pair_f32(p, p, 4, 0, p, 4, p, 4, 8, p, 1, 0, None, 0, None) == -1   # lds < d
    assert b"edge_score_pair" in lib.clane_last_error()
    assert lib.clane_edge_score_pair_f64(p, p, 4, 0, p, 8, None, 8, 8, p, 1, 0, None, 0, None) == -1
    assert lib.clane_edge_score_pair_f32(p, p, 4, 0, p, 8, p, 8, 8, p, 1, 0, None, 2, None) == -1   # n_long, no list
    assert lib.clane_edge_score_class_pair_f32(p, p, p, p, p, p, 1, 2, p, p, 1, 0, p, 8, p, 8, 8, p, 1, p,
                                               None) == -1                      # items_per_block < 4
    assert b"edge_score_class_pair" in lib.clane_last_error()
    assert lib.clane_edge_score_class_pair_f64(None, p, p, p, p, p, 1, 8, None, None, 1, 0, p, 8, p, 8, 8, p, 1,
                                               None, None) == -1                # fused softmax without its arrays
