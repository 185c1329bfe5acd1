"""Training the bilinear similarity, on the CPU: the five kernel calls restated in torch as a KernelBackend subclass, the
host logic (Embedder.update_similarity_measure, PairSampler, AlternatingEmbedder, the CLI flag) driven by it, and the
reference's own training run (fixture g14, made by tools/make_train_golden.py) replayed in fp64."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.embedder import AlternatingEmbedder, Embedder, IterativeEmbedder
from clane_amd.engine import SweepEngine
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR
from clane_amd.similarity import AsymmertricSimilarity, CosineSimilarity
from clane_amd.train import PairSampler, rows_of_vertices

from .conftest import load_golden, write_data_root
from .oracle_kernels import OracleKernels
from .test_bilinear_host import BilinearOracleKernels, _skewed_csr
from .thread_comm import ThreadWorld

GOLD = "g14_karate_asym_train.npz"
ROOT = Path(__file__).resolve().parent.parent


class TrainOracleKernels(BilinearOracleKernels):
    """The training calls of csrc/pair_train.h in torch (the same formulas, no attempt at the same rounding)."""

    def pair_project(self, Z, d, src, dst, W, A, Bm):
        Zs = Z[:, :d].to(W.dtype)
        A[:src.numel()] = Zs[src.long()] @ W[:d].T
        Bm[:src.numel()] = Zs[dst.long()] @ W[d:].T

    def pair_loss(self, A, Bm, d, linked, u, g, mask, ws, stats):
        s = (A * Bm).sum(1)
        p, q = torch.sigmoid(s), torch.sigmoid(-s)
        lk = linked.bool()
        mk = lk ^ (u < p)
        loss = -torch.log(torch.where(lk, p, q) + 1e-10)
        gk = torch.where(lk, -p * q / (p + 1e-10), p * q / (q + 1e-10))
        g.copy_(torch.where(mk, gk, torch.zeros_like(gk)))
        mask.copy_(mk.to(torch.uint8))
        stats[0] = float(loss[mk].double().sum())
        stats[1] = float(mk.sum())

    def pair_grad_ws_len(self, B, d):
        return 1

    def pair_grad(self, Z, d, src, dst, A, Bm, g, stats, ws, dW):
        M = float(stats[1])
        Zs = Z[:, :d].to(A.dtype)
        if M == 0:
            dW.zero_()
            return
        dW[:d] = (g[:, None] * Bm).T @ Zs[src.long()] / M
        dW[d:] = (g[:, None] * A).T @ Zs[dst.long()] / M

    def adam_step(self, W, m, v, dW, lr, stats, state):
        if float(stats[1]) == 0:
            return
        t = float(state[0]) + 1
        m.add_((dW - m) * 0.1)
        v.mul_(0.999).add_(dW * dW * 0.001)
        denom = v.sqrt() / math.sqrt(1 - 0.999 ** t) + 1e-8
        W.add_(m / denom * (-lr / (1 - 0.9 ** t)))
        state[0] += 1
        state[1] += float(stats[0]) / float(stats[1])

    def pair_labels(self, rowptr, colidx, nrows, src, dst, linked):
        rp, ci = rowptr.tolist(), colidx.tolist()
        for k, (s, t) in enumerate(zip(src.tolist(), dst.tolist())):
            linked[k] = int(0 <= s < nrows and t in ci[rp[s]:rp[s + 1]])


def _karate(tmp_path, gold, dtype=torch.float64, **engine_kw):
    k = load_golden("g2_karate_csr.npz")
    X = gold["X"].astype(np.float64 if dtype == torch.float64 else np.float32)
    root = write_data_root(tmp_path / "karate_train", k["vertex_ids"], k["edge_src"], k["edge_dst"], X)
    g = Graph(root, embedding_dim=int(X.shape[1]))
    g._attach_engine(SweepEngine(g.csr, g.X, "cpu", TrainOracleKernels(), **engine_kw))
    return g


def _sim(W0, dtype=torch.float64):
    d = W0.shape[1]
    sim = AsymmertricSimilarity(d).to(dtype)
    with torch.no_grad():
        sim.Phi_src.weight.copy_(torch.as_tensor(W0[:d]))
        sim.Phi_dst.weight.copy_(torch.as_tensor(W0[d:]))
    return sim


def _replay(gold):
    return [(gold["src"][i], gold["dst"][i], gold["linked"][i], gold["trial"][i]) for i in range(len(gold["src"]))]


# ---- the reference's run, replayed ----------------------------------------------------------------------------
@pytest.mark.parametrize("class_threshold", [None, 3])
def test_replay_reproduces_the_reference_in_fp64(tmp_path, class_threshold):
    gold = load_golden(GOLD)
    g = _karate(tmp_path, gold, class_threshold=class_threshold, class_chunk=64)
    sim = _sim(gold["W0"])
    emb = Embedder(g, sim, torch.device("cpu"), lr=float(gold["lr"]), batch_size=int(gold["batch_size"]), verbose=False)
    losses = emb.update_similarity_measure(int(gold["epochs"]), replay=_replay(gold))
    np.testing.assert_allclose(losses, gold["losses_f64"], rtol=1e-9)
    W = torch.cat([sim.Phi_src.weight, sim.Phi_dst.weight], 0).detach().numpy()
    assert np.abs(W - gold["W_final_f64"]).max() < 1e-9
    # the fixture holds a step the reference skipped (no pair in the loss): it was not counted
    skipped = int((np.abs(gold["dW_f64"]).reshape(len(gold["src"]), -1).max(1) == 0).sum())
    assert skipped >= 1 and emb.last_trainer.steps_taken() == len(gold["src"]) - skipped


def test_fixture_is_self_consistent():
    gold = load_golden(GOLD)
    n = len(gold["src"])
    assert n == int(gold["epochs"]) * (34 // int(gold["batch_size"])) and gold["W_before"].shape == (n, 32, 16)
    assert np.array_equal(gold["W_before"][0], gold["W0"].astype(np.float64))
    k = load_golden("g2_karate_csr.npz")
    edges = set(zip(k["edge_src"].tolist(), k["edge_dst"].tolist()))
    ids = [int(v) for v in k["vertex_ids"]]
    pos = sum(int(l) for l in gold["linked"].ravel())
    assert 0 <= pos <= gold["linked"].size and len(edges) > 0 and len(ids) == 34
    assert 0 < float(gold["grad_err_ref_f32"]) < 1e-4


# ---- a step that no pair takes part in ------------------------------------------------------------------------
def test_step_without_masked_pairs_changes_nothing(tmp_path):
    gold = load_golden(GOLD)
    g = _karate(tmp_path, gold)
    eng = g._engine
    tr = eng.similarity_trainer(torch.from_numpy(gold["W0"]), 1e-2, 4)
    src = rows_of_vertices(eng, [0, 1, 2, 3])
    dst = rows_of_vertices(eng, [4, 5, 6, 7])
    ones = torch.ones(4, dtype=torch.float64)
    tr.step(src, dst, torch.zeros(4, dtype=torch.uint8), ones)             # unlinked, trial fails: mask empty
    assert tr.steps_taken() == 0 and tr.epoch_loss() == 0.0
    assert torch.equal(tr.weights(), torch.from_numpy(gold["W0"]).double())
    assert not tr.m.any() and not tr.v.any()
    tr.step(src, dst, torch.ones(4, dtype=torch.uint8), ones)              # linked, trial fails: all four count
    assert tr.steps_taken() == 1 and tr.epoch_loss() > 0 and not torch.equal(tr.weights(), tr.W * 0 + torch.from_numpy(gold["W0"]))
    assert tr.epoch_loss() == 0.0                                           # reading clears the accumulator


# ---- sampler ----------------------------------------------------------------------------------------------------
def _engine(V=90, d=6, seed=2, **kw):
    csr = _skewed_csr(V, seed)
    X = torch.from_numpy(np.random.default_rng(seed).standard_normal((V, d)))
    return csr, SweepEngine(csr, X, "cpu", TrainOracleKernels(), **kw)


def _vertex_of_row(eng):
    inv = torch.full((eng.part.padded_vertices,), -1, dtype=torch.int64)
    inv[eng.pos] = torch.arange(eng.V)
    return inv


@pytest.mark.parametrize("class_threshold", [None, 3])
def test_sampler_batches_labels_and_determinism(class_threshold):
    csr, eng = _engine(class_threshold=class_threshold, class_chunk=64)
    dense = np.zeros((90, 90), dtype=bool)
    dense[np.repeat(np.arange(90), np.diff(csr.rowptr)), csr.colidx] = True
    inv = _vertex_of_row(eng)

    def draw(seed, frac):
        s = PairSampler(eng, 7, torch.Generator().manual_seed(seed), positive_fraction=frac)
        return [[t.clone() for t in b] for b in s.epoch()], s

    a, s = draw(3, 0.0)
    assert len(a) == 90 // 7 == s.n_batches and all(b[0].numel() == 7 for b in a)          # drop_last
    srcs = torch.cat([inv[b[0].long()] for b in a])
    assert len(set(srcs.tolist())) == srcs.numel() and srcs.min() >= 0                   # a permutation's prefix
    for src, dst, linked, u in a:
        assert src.dtype == torch.int32 and linked.dtype == torch.uint8 and u.dtype == eng.acc_dtype
        assert bool(((u >= 0) & (u <= 1)).all())
        want = dense[inv[src.long()].numpy(), inv[dst.long()].numpy()]
        assert np.array_equal(linked.numpy().astype(bool), want)
    b, _ = draw(3, 0.0)
    assert all(torch.equal(x, y) for ba, bb in zip(a, b) for x, y in zip(ba, bb))        # same seed, same batches
    c, _ = draw(4, 0.0)
    assert any(not torch.equal(x, y) for ba, bc in zip(a, c) for x, y in zip(ba, bc))
    e1 = [[t.clone() for t in bt] for bt in s.epoch()]                                    # next epoch: new draw
    assert any(not torch.equal(x[0], y[0]) for x, y in zip(a, e1))
    # positive_fraction = 1: every source with an out-edge gets a neighbour, labels stay right
    p, _ = draw(5, 1.0)
    deg = np.diff(csr.rowptr)
    n_pos = 0
    for src, dst, linked, u in p:
        sv, dv = inv[src.long()].numpy(), inv[dst.long()].numpy()
        assert np.array_equal(linked.numpy().astype(bool), dense[sv, dv])
        assert bool(linked.numpy().astype(bool)[deg[sv] > 0].all())
        n_pos += int(linked.sum())
    assert n_pos > 0
    h, _ = draw(6, 0.5)
    share = np.mean([float(bt[2].float().mean()) for bt in h])
    assert 0.2 < share < 0.8


# ---- what is refused ------------------------------------------------------------------------------------------
def test_refusals(tmp_path):
    gold = load_golden(GOLD)
    g = _karate(tmp_path, gold)
    with pytest.raises(TypeError, match="AsymmertricSimilarity"):
        Embedder(g, CosineSimilarity(), torch.device("cpu"), verbose=False).update_similarity_measure(1)
    with pytest.raises(TypeError, match="AsymmertricSimilarity"):
        AlternatingEmbedder(g, CosineSimilarity(), torch.device("cpu"))
    with pytest.raises(NotImplementedError):
        IterativeEmbedder()                                                # the stub stays a stub
    g.dispense_pair = True
    with pytest.raises(NotImplementedError):
        g[0]                                                               # the sampler does not go through __getitem__
    csr = _skewed_csr(40, 1)
    X = torch.zeros(40, 4)
    shared = ThreadWorld(1)
    comm = shared.comm(0)
    comm.force = True
    eng = SweepEngine(csr, X, "cpu", TrainOracleKernels(), comm=comm, exchange="columns")
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        eng.similarity_trainer(torch.zeros(2 * eng.d, eng.d), 1e-2, 4)
    eng1 = SweepEngine(csr, X, "cpu", TrainOracleKernels())
    eng1.world = 2                                                          # what a rank of a 2-GPU run would see
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        PairSampler(eng1, 4, torch.Generator().manual_seed(0))
    with pytest.raises(NotImplementedError, match="OracleKernels has no pair_"):   # a backend without the optional calls
        SweepEngine(csr, X, "cpu", OracleKernels()).similarity_trainer(torch.zeros(8, 4), 1e-2, 4)


def test_backend_without_training_calls_says_so():
    kern = OracleKernels()
    for call in (lambda: kern.pair_project(None, 1, None, None, None, None, None),
                 lambda: kern.pair_loss(None, None, 1, None, None, None, None, None, None),
                 lambda: kern.pair_grad_ws_len(1, 1),
                 lambda: kern.pair_grad(None, 1, None, None, None, None, None, None, None, None),
                 lambda: kern.adam_step(None, None, None, None, 0.1, None, None),
                 lambda: kern.pair_labels(None, None, 0, None, None, None)):
        with pytest.raises(NotImplementedError):
            call()


# ---- AlternatingEmbedder's stopping rules -----------------------------------------------------------------------
def test_alternating_embedder_stopping_rules(tmp_path, monkeypatch):
    gold = load_golden(GOLD)
    g = _karate(tmp_path, gold)
    emb = AlternatingEmbedder(g, _sim(gold["W0"]), torch.device("cpu"), tolerence=2, tolerence_Z=3, tolerence_P=2,
                              epoch=2, lr=1e-2, verbose=False, max_rounds=5)
    script = iter([[9.0, 5.0], [9.0, 4.0], [9.0, 4.0], [1.0, 4.5],            # round 1: min at call 2, then two misses
                   [3.0, 3.0], [3.0, 3.5], [3.0, 3.2]] + [[7.0, 7.0]] * 40)   # round 2: min at call 1, two misses
    asked = []

    def scripted(epochs=None, sampler=None, replay=None):
        asked.append(epochs)
        return next(script)
    monkeypatch.setattr(emb, "update_similarity_measure", scripted)
    emb.iterate()
    assert emb.train_losses[0] == [[9.0, 5.0], [9.0, 4.0], [9.0, 4.0], [1.0, 4.5]]
    assert emb.train_losses[1] == [[3.0, 3.0], [3.0, 3.5], [3.0, 3.2]]
    assert set(asked) == {2}
    assert len(emb.sweep_counts) == len(emb.outer_deltas) == len(emb.train_losses) <= 5
    assert all(c >= 3 for c in emb.sweep_counts)                               # tolerence_Z sweeps at the very least
    assert emb.tolerences["global"].value == 0 or len(emb.outer_deltas) == 5
    # frozen weights: round 2 moves Z less than round 1 did, later rounds bring no new minimum for `tolerence` rounds
    assert emb.outer_deltas[1] < emb.outer_deltas[0]


def test_alternating_embedder_trains_and_propagates(tmp_path):
    gold = load_golden(GOLD)
    g = _karate(tmp_path, gold)
    sim = _sim(gold["W0"])
    emb = AlternatingEmbedder(g, sim, torch.device("cpu"), tolerence=1, tolerence_Z=2, tolerence_P=1, epoch=2,
                              batch_size=4, lr=1e-2, seed=3, positive_fraction=0.5, verbose=False, max_rounds=2)
    emb.iterate()
    W = torch.cat([sim.Phi_src.weight, sim.Phi_dst.weight], 0).detach()
    assert not torch.allclose(W, torch.from_numpy(gold["W0"]).double())       # the module got the trained weights
    assert len(emb.train_losses) >= 1 and all(len(l) == 2 and np.isfinite(l).all() for l in emb.train_losses[0])
    assert g._engine.P_valid and not torch.allclose(g.Z, g.X)


# ---- ABI surface and CLI --------------------------------------------------------------------------------------------
NEW_SYMBOLS = ([f"clane_pair_project_{s}" for s in ("f32", "f64", "bf16")] + [f"clane_pair_grad_{s}" for s in ("f32", "f64", "bf16")]
               + [f"clane_pair_loss_{s}" for s in ("f32", "f64")] + [f"clane_adam_step_{s}" for s in ("f32", "f64")]
               + ["clane_pair_grad_ws_len", "clane_pair_labels"])


def test_training_symbols_are_declared_bound_and_checked():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "clane_hip.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _hip.SIGNATURES, name
    lib = _hip.load_library()
    assert lib.clane_pair_grad_ws_len(1, 16) == 2 * 16 * 16
    assert lib.clane_pair_grad_ws_len(2048, 16) == 2 * 16 * 16 and lib.clane_pair_grad_ws_len(2049, 16) == 4 * 16 * 16
    import ctypes as C
    p = C.cast((C.c_float * 64)(), C.c_void_p)
    assert lib.clane_pair_project_f32(p, 4, 8, 4, p, p, 2, p, p, p, None) == -1            # ldz < d
    assert b"pair_project" in lib.clane_last_error()
    assert lib.clane_pair_project_f32(None, 4, 8, 8, None, None, 0, None, None, None, None) == 0   # no pairs
    assert lib.clane_pair_loss_f64(p, p, 2, 0, p, p, p, p, p, p, None) == -1               # d < 1
    assert lib.clane_pair_grad_bf16(p, 4, 8, 8, p, p, 2, p, p, p, None, p, p, None) == -1  # no stats
    assert lib.clane_adam_step_f32(p, p, p, p, 4, 0.1, None, p, None) == -1
    assert lib.clane_pair_labels(None, p, 4, p, p, 2, p, None) == -1
    assert b"null pointer" in lib.clane_last_error()


def test_cli_flag_selects_the_alternating_embedder(monkeypatch, tmp_path):
    import clane_amd.__main__ as M
    args = M.get_parser().parse_args(["--train_similarity", "--config_file", "c.yaml"])
    assert args.train_similarity is True
    assert M.get_parser().parse_args(["--config_file", "c.yaml"]).train_similarity is False
    gold = load_golden(GOLD)
    k = load_golden("g2_karate_csr.npz")
    root = write_data_root(tmp_path / "cli", k["vertex_ids"], k["edge_src"], k["edge_dst"], gold["X"][:, :2].copy())
    cfg = tmp_path / "config2.yaml"          # the keys of the reference's tests/config2.yaml
    cfg.write_text("graph:\n  embedding_dim: 2\nsimilarity:\n  method: \"AsymmertricSimilarity\"\n  kwargs:\n    n_dim: 2\n"
                   "embedder:\n  gamma: 0.76\n  lr: 0.1\n  tolerence: 1\n  tolerence_Z: 1\n  tolerence_P: 1\n  epoch: 2\n"
                   "  batch_size: 4\n")
    real_engine = Graph.engine

    def cpu_engine(self, device=None, **kw):
        if self._engine is None:
            self._attach_engine(SweepEngine(self.csr, self.X, "cpu", TrainOracleKernels()))
        return self._engine
    monkeypatch.setattr(Graph, "engine", cpu_engine)
    out = tmp_path / "out"
    common = ["--data_root", str(root), "--output_root", str(out), "--config_file", str(cfg)]
    with pytest.raises(NotImplementedError):                                   # without the flag: as before
        M.embedding(M.get_parser().parse_args(common))
    M.embedding(M.get_parser().parse_args(common + ["--train_similarity"]))
    Z = np.load(out / "Z.npy")
    assert Z.shape == (34, 2) and np.isfinite(Z).all()
    assert real_engine is not Graph.engine
