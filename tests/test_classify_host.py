"""Node classification, the parts that need no GPU: the two kernels of csrc/label_probe.h restated in torch as a
KernelBackend subclass, and the host logic driven by it -- splits, the skipped-fit rule, the label file, F1 from
hand-made confusion counts, the grouping of fits, the batched L-BFGS against torch.optim.LBFGS, the CLI section."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.classify import (LabelProbe, confusion_counts, f1_from_confusion, make_splits, read_labels,
                                train_count)
from clane_amd.engine import SweepEngine
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR

from .conftest import GOLDEN, load_golden, write_data_root
from .oracle_kernels import OracleKernels

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ([f"clane_probe_{w}_{s}" for w in ("forward", "grad") for s in ("f32", "f64", "bf16")]
               + ["clane_probe_loss_ws_len", "clane_probe_grad_ws_len"])


class ProbeOracleKernels(OracleKernels):
    """probe_forward / probe_grad of csrc/label_probe.h in torch (the same formulas, no attempt at the same rounding)."""

    def probe_loss_ws_len(self, n, F):
        return 1

    def probe_grad_ws_len(self, n, K, d):
        return 1

    @staticmethod
    def _gathered(Z, d, rows, dtype):
        r = rows.long()
        inside = (r >= 0) & (r < Z.shape[0])
        return Z[r.clamp(0, Z.shape[0] - 1), :d].to(dtype) * inside[:, None].to(dtype)

    def probe_forward(self, Z, d, rows, y, split, W, bias, F, C, loss_ws, loss, G=None, pred=None):
        # fit by fit: like the kernel, a fit gets the same bits whatever else shares the call
        n, Cp = rows.numel(), _hip.probe_padded_classes(C)
        Zg, yl = self._gathered(Z, d, rows, W.dtype), y.long()
        for f in range(F):
            logits = Zg @ W[f * Cp:f * Cp + C].T + bias[f * Cp:f * Cp + C]
            train = split[:, f] != 0
            ce = torch.logsumexp(logits, 1) - logits[torch.arange(n), yl]
            loss[f] = (ce * train).double().sum()
            if G is not None:
                g = torch.softmax(logits, 1)
                g[torch.arange(n), yl] -= 1.0
                Gm = G[:n * F * Cp].view(n, F * Cp)
                Gm[:, f * Cp:(f + 1) * Cp] = 0.0
                Gm[:, f * Cp:f * Cp + C] = g * train[:, None]
            if pred is not None:
                pred[:, f] = logits.argmax(1).to(torch.int32)       # distinct logits: no ties to break here

    def probe_grad(self, Z, d, rows, G, ws, dW, db):
        n, K = rows.numel(), db.numel()
        Gm, Zg = G[:n * K].view(n, K), None
        Zg = self._gathered(Z, d, rows, Gm.dtype)
        out = dW.view(K, d)
        for o in range(K):                                           # row by row, for the same reason
            out[o] = (Gm[:, o:o + 1] * Zg).sum(0)
            db[o] = Gm[:, o].sum()


def _engine(V=40, d=6, dtype=torch.float64, seed=0):
    rng = np.random.default_rng(seed)
    rowptr = np.arange(V + 1, dtype=np.int64)
    colidx = ((np.arange(V) + 1) % V).astype(np.int32)
    X = torch.from_numpy(rng.standard_normal((V, d))).to(dtype)
    return SweepEngine(HostCSR(V, rowptr, colidx), X, "cpu", ProbeOracleKernels()), X


def _planted(n, d, C, sep, seed):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, n)
    y[:C] = np.arange(C)
    X = rng.standard_normal((C, d))[y] * sep + rng.standard_normal((n, d))
    return torch.from_numpy(X), torch.from_numpy(y)


# ---- the ABI ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "clane_hip.h").read_text(), flags=re.S)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        decl = re.search(rf"\b(?:int|int64_t) {name}\s*\(([^;]*)\);", header)
        assert decl and name in _hip.SIGNATURES, name
        assert len(_hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
        assert getattr(lib, name) is not None
    assert re.search(r"#define CLANE_ABI_VERSION 5\b", header) and lib.clane_abi_version() == 5
    assert lib.clane_probe_loss_ws_len(1, 3) == 3 and lib.clane_probe_loss_ws_len(129, 90) == 180
    assert lib.clane_probe_grad_ws_len(2048, 8, 5) == 48 and lib.clane_probe_grad_ws_len(2049, 152, 16) == 2 * 152 * 17
    assert [_hip.probe_padded_classes(c) for c in (2, 3, 7, 16, 17, 64)] == [2, 4, 8, 16, 32, 64]
    for bad in (1, 65):
        with pytest.raises(ValueError, match="classes"):
            _hip.probe_padded_classes(bad)


def test_argument_validation_reaches_last_error():
    lib = _hip.load_library()                   # refused on the host before any launch: safe without a GPU
    p = C.cast((C.c_float * 64)(), C.c_void_p)

    def fwd(fn=lib.clane_probe_forward_f32, d=4, ldz=4, n=2, ld_split=3, F=3, Cn=3, flags=0, G=None, ws=p, loss=p, pred=None,
            ld_pred=3, Z=p):
        return fn(Z, 8, d, ldz, p, p, n, p, ld_split, p, p, F, Cn, flags, G, ws, loss, pred, ld_pred, None)

    for bad, text in ((dict(d=0), b"bad shape"), (dict(ldz=3), b"bad shape"), (dict(n=-1), b"bad shape"),
                      (dict(Cn=1), b"C must be"), (dict(Cn=65), b"C must be"), (dict(F=0), b"number of fits"),
                      (dict(ld_split=2), b"ld_split"), (dict(flags=4), b"unknown flags"), (dict(flags=1), b"needs G"),
                      (dict(flags=2), b"needs pred"), (dict(flags=2, pred=p, ld_pred=2), b"ld_pred"),
                      (dict(ws=None), b"null loss"), (dict(Z=None), b"null pointer")):
        assert fwd(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"probe_forward" in lib.clane_last_error()
    assert fwd(fn=lib.clane_probe_forward_bf16, Cn=70) == -1 and fwd(fn=lib.clane_probe_forward_f64, d=-1) == -1

    def grad(fn=lib.clane_probe_grad_f32, d=4, ldz=4, n=2, K=8, G=p, ws=p):
        return fn(p, 8, d, ldz, p, n, G, K, ws, p, p, None)
    for bad, text in ((dict(d=0), b"bad shape"), (dict(K=0), b"bad shape"), (dict(ldz=2), b"bad shape"),
                      (dict(ws=None), b"null workspace"), (dict(G=None), b"null pointer"),
                      (dict(n=65536 * 2048), b"too many")):
        assert grad(**bad) == -1 and text in lib.clane_last_error(), bad
    assert grad(fn=lib.clane_probe_grad_f64, K=-2) == -1 and grad(fn=lib.clane_probe_grad_bf16, n=-1) == -1


def test_backend_without_the_probe_says_so():
    with pytest.raises(NotImplementedError, match="OracleKernels has no probe_forward"):
        OracleKernels().probe_forward(None, 1, None, None, None, None, None, 1, 2, None, None)
    with pytest.raises(NotImplementedError, match="OracleKernels has no probe_grad"):
        OracleKernels().probe_grad(None, 1, None, None, None, None, None)


# ---- splits -----------------------------------------------------------------------------------------------------
def test_split_sizes_and_seeding():
    assert [train_count(34, r) for r in (0.1, 0.5, 0.9)] == [3, 17, 31]
    assert train_count(5, 0.5) == 3 and train_count(3, 0.01) == 1 and train_count(3, 0.99) == 2 and train_count(2, 0.9) == 1
    split, fits = make_splits(34, (0.1, 0.5, 0.9), 4, seed=3)
    assert split.dtype == torch.uint8 and tuple(split.shape) == (34, 12)
    assert fits == [(r, k) for r in (0.1, 0.5, 0.9) for k in range(4)]
    assert split.sum(0).tolist() == [3] * 4 + [17] * 4 + [31] * 4
    again, _ = make_splits(34, (0.1, 0.5, 0.9), 4, seed=3)
    assert torch.equal(split, again)
    other, _ = make_splits(34, (0.1, 0.5, 0.9), 4, seed=4)
    assert not torch.equal(split, other)
    assert torch.equal(other[:, 0], split[:, 1])                    # run r of seed s is run r - 1 of seed s + 1
    assert not torch.equal(split[:, 0], split[:, 1])                # runs differ
    assert bool((split[:, 0] <= split[:, 4]).all() and (split[:, 4] <= split[:, 8]).all())     # one permutation per run
    assert bool(((split == 0).sum(0) >= 1).all())                   # a test row always remains
    with pytest.raises(ValueError, match="at least 2"):
        make_splits(1, (0.5,), 1, 0)
    with pytest.raises(ValueError, match="ratios"):
        make_splits(10, (1.0,), 1, 0)


def test_read_labels(tmp_path):
    vertex_ids = ["a", "b", "c", "a", "d"]
    (tmp_path / "Y").write_text("c\tzebra\n\nb\tant\nd\tzebra\n")
    assert read_labels(tmp_path / "Y", vertex_ids) == ([2, 1, 4], [1, 0, 1], ["ant", "zebra"])
    (tmp_path / "unknown").write_text("c\tx\nzz\ty\n")
    with pytest.raises(ValueError, match=r"line 2: 'zz'"):
        read_labels(tmp_path / "unknown", vertex_ids)
    (tmp_path / "twice").write_text("c\tx\nb\ty\n\nc\ty\n")
    with pytest.raises(ValueError, match=r"line 4: 'c' was labelled on line 1"):
        read_labels(tmp_path / "twice", vertex_ids)
    (tmp_path / "short").write_text("c\n")
    with pytest.raises(ValueError, match="line 1"):
        read_labels(tmp_path / "short", vertex_ids)
    k = load_golden("g2_karate_csr.npz")
    v, y, names = read_labels(GOLDEN / "g2_karate_Y.tsv", [str(i) for i in k["vertex_ids"]])
    assert len(v) == 34 and sorted(v) == list(range(34)) and len(names) == max(y) + 1 >= 2


# ---- metrics ----------------------------------------------------------------------------------------------------
def test_f1_from_hand_made_confusion_counts():
    # truth rows, prediction columns.  Class 2 is never predicted, class 3 never true, class 4 absent altogether.
    conf = torch.tensor([[5, 1, 0, 0, 0],
                         [2, 3, 0, 1, 0],
                         [1, 1, 0, 0, 0],
                         [0, 0, 0, 0, 0],
                         [0, 0, 0, 0, 0]])
    micro, macro = f1_from_confusion(conf)
    f0 = 2 * 5 / (2 * 5 + 3 + 1)            # tp 5, fp 3 (column 0), fn 1
    f1 = 2 * 3 / (2 * 3 + 2 + 3)            # tp 3, fp 2, fn 3
    assert float(micro) == pytest.approx(8 / 14, abs=1e-15)
    assert float(macro) == pytest.approx((f0 + f1 + 0.0 + 0.0) / 4, abs=1e-15)      # classes 2 and 3 count 0, class 4 does not count
    perfect = torch.diag(torch.tensor([3, 0, 4]))
    micro, macro = f1_from_confusion(torch.stack([perfect, perfect.flip(0)]))
    assert micro.tolist() == [1.0, 0.0] and macro.tolist() == [1.0, 0.0]
    # the counts themselves
    y = torch.tensor([0, 1, 1, 2])
    pred = torch.tensor([[0, 1], [1, 1], [0, 2], [2, 2]], dtype=torch.int32)
    test = torch.tensor([[1, 0], [1, 1], [1, 1], [0, 1]], dtype=torch.bool)
    conf = confusion_counts(y, pred, test, 3)
    assert conf[0].tolist() == [[1, 0, 0], [1, 1, 0], [0, 0, 0]] and conf[1].tolist() == [[0, 0, 0], [0, 1, 1], [0, 0, 1]]


# ---- the fit ----------------------------------------------------------------------------------------------------
def _reference_fit(X, y, train, C, l2):
    """One fit by torch.optim.LBFGS(strong_wolfe) in float64 on the same objective."""
    Xt, yt = X[train], y[train]
    n_f, d = Xt.shape
    W = torch.zeros(C, d, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.LBFGS([W, b], max_iter=2000, tolerance_grad=1e-10, tolerance_change=0, history_size=20,
                            line_search_fn="strong_wolfe")

    def objective():
        return (torch.nn.functional.cross_entropy(Xt @ W.T + b, yt, reduction="sum") + 0.5 * l2 * (W * W).sum()) / n_f

    def closure():
        opt.zero_grad()
        J = objective()
        J.backward()
        return J
    opt.step(closure)
    return W.detach(), b.detach(), float(objective().detach())


def test_batched_fit_matches_a_per_fit_lbfgs_and_grouping_changes_nothing():
    n, d, Cn = 120, 6, 5
    X, y = _planted(n, d, Cn, 1.0, seed=1)
    eng, _ = _engine(V=n, d=d)
    eng.set_Z(X)
    rows = eng.pos[torch.arange(n)].to(torch.int32)
    split, _ = make_splits(n, (0.2, 0.5, 0.8), 2, seed=5)
    probe = LabelProbe(eng, l2=1.0, gtol=1e-8)
    fit = probe.fit(eng.Zcur, rows, y, split, Cn)
    assert bool(fit.converged.all()) and not bool(fit.skipped.any()) and int(fit.iterations.max()) < 400
    assert tuple(fit.W.shape) == (6, Cn, d) and tuple(fit.b.shape) == (6, Cn) and tuple(fit.pred.shape) == (n, 6)
    for f in range(6):
        W, b, J = _reference_fit(X, y.long(), split[:, f].bool(), Cn, 1.0)
        assert abs(float(fit.objective[f]) - J) <= 1e-9 * J
        assert float((fit.W[f] - W).abs().max()) < 1e-4
        assert float(((fit.b[f] - fit.b[f].mean()) - (b - b.mean())).abs().max()) < 1e-4
        logits = X @ W.T + b
        top2 = logits.topk(2, 1).values
        clear = (top2[:, 0] - top2[:, 1]) >= 1e-2
        assert torch.equal(fit.pred[clear, f].long(), logits.argmax(1)[clear])
    one_pass = dict(probe.passes)
    # a budget that holds one fit's G at a time: six groups, the same bits
    small = LabelProbe(eng, l2=1.0, gtol=1e-8, g_budget_bytes=n * 8 * 8)
    assert len(small.groups(n, 6, 8, torch.float64)) == 6
    again = small.fit(eng.Zcur, rows, y, split, Cn)
    for name in ("W", "b", "objective", "iterations", "pred", "grad_max"):
        assert torch.equal(getattr(fit, name), getattr(again, name)), name
    assert small.passes["forward"] > one_pass["forward"]


def test_a_fit_without_two_training_classes_is_skipped_and_counted():
    n, d = 30, 4
    X, _ = _planted(n, d, 2, 1.0, seed=2)
    y = torch.zeros(n, dtype=torch.int64)
    y[-3:] = 1                                              # class 1 only on three vertices
    eng, _ = _engine(V=n, d=d)
    eng.set_Z(X)
    probe = LabelProbe(eng)
    rows = eng.pos[torch.arange(n)].to(torch.int32)
    split = torch.zeros(n, 2, dtype=torch.uint8)
    split[:10, 0] = 1                                       # fit 0 trains on class 0 alone
    split[20:, 1] = 1
    fit = probe.fit(eng.Zcur, rows, y, split, 2)
    assert fit.skipped.tolist() == [True, False] and fit.converged.tolist() == [False, True]
    assert fit.iterations.tolist()[0] == 0 and float(fit.W[0].abs().max()) == 0.0
    out = probe.evaluate(list(range(n)), y.tolist(), 2, ratios=(0.1, 0.5), runs=6, seed=0)
    skipped = out["fits"]["skipped"]
    assert out["skipped_fits"] == sum(skipped) >= 1         # 3 training rows of 30 rarely meet class 1
    for i, row in enumerate(out["rows"]):
        used = [not s for s in skipped[i * 6:(i + 1) * 6]]
        assert row["runs_used"] == sum(used)
        micro = [m for m, u in zip(out["fits"]["micro_f1"][i * 6:(i + 1) * 6], used) if u]
        assert row["micro_f1"] == pytest.approx(sum(micro) / len(micro), abs=1e-12)


def test_evaluate_on_both_tables_and_refusals():
    n, d, Cn = 60, 5, 3
    X, y = _planted(n, d, Cn, 1.5, seed=3)
    eng, X0 = _engine(V=n, d=d)                             # content embeddings: noise; embeddings: planted
    eng.set_Z(X)
    probe = LabelProbe(eng)
    verts = list(range(0, n, 2))                            # a subset, and not every vertex
    outZ = probe.evaluate(verts, y[verts].tolist(), Cn, ratios=(0.5,), runs=3, seed=1, table="Z")
    outX = probe.evaluate(verts, y[verts].tolist(), Cn, ratios=(0.5,), runs=3, seed=1, table="X")
    assert outZ["labelled"] == 30 and outZ["rows"][0]["runs_used"] == 3 and all(outZ["fits"]["converged"])
    assert outZ["rows"][0]["micro_f1"] > outX["rows"][0]["micro_f1"]
    Zt, rows = probe.table_and_rows(verts, "X")
    assert torch.equal(Zt[rows.long(), :d], X0[verts])
    with pytest.raises(ValueError, match="'Z' or 'X'"):
        probe.table_and_rows(verts, "Q")
    with pytest.raises(ValueError, match=r"vertex indices must be in \[0, 60\)"):
        probe.table_and_rows([60])
    with pytest.raises(ValueError, match="classes must be in"):
        probe.fit(eng.Zcur, rows, torch.full((30,), 3), torch.ones(30, 1, dtype=torch.uint8), 3)
    eng.world = 2
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        LabelProbe(eng)


# ---- the surface ------------------------------------------------------------------------------------------------
def _karate_root(tmp_path):
    k = load_golden("g2_karate_csr.npz")
    X = np.random.default_rng(0).standard_normal((34, 4)).astype(np.float32)
    root = write_data_root(tmp_path / "karate", k["vertex_ids"], k["edge_src"], k["edge_dst"], X)
    (root / "Y").write_text((GOLDEN / "g2_karate_Y.tsv").read_text())
    return root


CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


def _cpu_engine(monkeypatch):
    def cpu_engine(self, device=None, cosine_mode="reference", **kw):
        if self._engine is None:
            self._attach_engine(SweepEngine(self.csr, self.X, "cpu", ProbeOracleKernels(), cosine_mode=cosine_mode))
        return self._engine
    monkeypatch.setattr(Graph, "engine", cpu_engine)


def test_cli_section_writes_label_metrics(tmp_path, monkeypatch):
    import clane_amd.__main__ as M
    root = _karate_root(tmp_path)
    _cpu_engine(monkeypatch)
    plain, with_cls = tmp_path / "plain.yaml", tmp_path / "cls.yaml"
    plain.write_text(CONFIG)
    with_cls.write_text(CONFIG + "\nnode_classification:\n  labels: Y\n  ratios: [0.3, 0.7]\n  runs: 2\n  seed: 4\n"
                                 "  l2: 0.5\n  baseline: true\n")

    def run(cfg, out):
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg)]))
    run(plain, "plain")
    assert (tmp_path / "plain" / "Z.npy").exists() and not (tmp_path / "plain" / "label_metrics.json").exists()
    run(with_cls, "cls")
    assert np.array_equal(np.load(tmp_path / "plain" / "Z.npy"), np.load(tmp_path / "cls" / "Z.npy"))
    got = json.loads((tmp_path / "cls" / "label_metrics.json").read_text())
    assert set(got) == {"labels", "labelled", "class_names", "ratios", "runs", "seed", "l2", "tables"}
    assert got["labelled"] == 34 and got["ratios"] == [0.3, 0.7] and got["runs"] == 2 and got["seed"] == 4 and got["l2"] == 0.5
    assert set(got["tables"]) == {"Z", "X"} and len(got["class_names"]) >= 2
    for t in got["tables"].values():
        assert set(t) == {"rows", "fits", "skipped_fits"} and len(t["rows"]) == 2
        assert set(t["rows"][0]) == {"ratio", "micro_f1", "macro_f1", "runs_used"}
        assert set(t["fits"]) == {"ratio", "run", "iterations", "converged", "objective", "skipped", "micro_f1", "macro_f1"}
        assert all(len(v) == 4 for v in t["fits"].values())
        assert all(0.0 <= r["macro_f1"] <= r["micro_f1"] + 1e-12 <= 1.0 + 1e-12 for r in t["rows"])
    with_cls.write_text(CONFIG + "\nnode_classification:\n  labels: Y\n  runs: 1\n  ratios: [0.5]\n")      # no baseline
    run(with_cls, "z_only")
    assert set(json.loads((tmp_path / "z_only" / "label_metrics.json").read_text())["tables"]) == {"Z"}
    # the same through the Graph method, from (vertices, classes) with names of any sortable kind
    g = Graph(root, embedding_dim=4)
    v, y, names = read_labels(root / "Y", g.vertex_ids)
    a = g.evaluate_labels(root / "Y", ratios=(0.5,), runs=2, seed=1)
    b = g.evaluate_labels((v, [names[c] for c in y]), ratios=(0.5,), runs=2, seed=1)
    assert a == b and a["class_names"] == names and a["table"] == "Z"


def test_node_classification_is_refused_on_several_gpus_before_the_graph_is_loaded(monkeypatch, tmp_path):
    import clane_amd.__main__ as M
    monkeypatch.setenv("WORLD_SIZE", "2")

    def touched(*a, **k):
        raise AssertionError("the run went on to set up devices")
    monkeypatch.setattr(M, "_distributed_setup", touched)
    monkeypatch.setattr(M, "Graph", touched)
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG + "\nnode_classification:\n  labels: Y\n")
    args = M.get_parser().parse_args(["--data_root", str(tmp_path), "--output_root", str(tmp_path / "o"),
                                      "--config_file", str(cfg)])
    with pytest.raises(NotImplementedError, match="one GPU"):
        M.embedding(args)
    monkeypatch.setenv("WORLD_SIZE", "1")
    cfg.write_text(CONFIG + "\nnode_classification:\n  runs: 3\n")
    with pytest.raises(ValueError, match="node_classification"):       # a section without its label file
        M.embedding(args)
    assert set(vars(M.get_parser().parse_args([]))) == {                # no new flag
        "command", "data_root", "output_root", "config_file", "save_history", "num_workers", "init_Z", "exchange",
        "train_similarity", "predict_links", "link_sources", "gpu"}
