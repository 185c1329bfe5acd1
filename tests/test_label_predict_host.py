"""Label prediction, the parts that need no GPU: the ABI of csrc/label_predict.h, and the host logic -- per-fit l2,
cross-validation, the kept model and its file, the selection rule, the CLI section -- driven through a torch double of
probe_predict on top of the existing kernel doubles (tests/label_predict_cases.py)."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from clane_amd import _hip, classify
from clane_amd.classify import LabelModel, LabelProbe, choose_l2, fold_assignment, label_masks
from clane_amd.engine import SweepEngine
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR

from . import new_vertex_cases as N
from .conftest import GOLDEN, load_golden, write_data_root
from .label_predict_cases import PredictOracleKernels, planted, select_top
from .oracle_kernels import OracleKernels

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = [f"clane_probe_predict_{s}" for s in ("f32", "f64", "bf16")]


def _engine(X):
    V = X.shape[0]
    csr = HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + 1) % V).astype(np.int32))
    eng = SweepEngine(csr, X, "cpu", PredictOracleKernels())
    eng.set_Z(X)
    return eng


def _rows(eng, n):
    return eng.pos[torch.arange(n)].to(torch.int32)


# ---- the ABI ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "clane_hip.h").read_text(), flags=re.S)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", header)
        assert decl and name in _hip.SIGNATURES, name
        assert len(_hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == 17, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define CLANE_ABI_VERSION 5\b", header) and lib.clane_abi_version() == 5
    for define, value in (("CLANE_PREDICT_SIGMOID", _hip.PREDICT_SIGMOID), ("CLANE_PREDICT_WRITE_PROBA", _hip.PREDICT_WRITE_PROBA),
                          ("CLANE_PREDICT_MAX_TOP", _hip.PREDICT_MAX_TOP)):
        assert re.search(rf"#define {define} {value}\b", header), define


def test_argument_validation_reaches_last_error():
    lib = _hip.load_library()                   # refused on the host before any launch: safe without a GPU
    p = C.cast((C.c_float * 64)(), C.c_void_p)

    def call(fn=lib.clane_probe_predict_f32, d=4, ldz=4, n=2, F=3, Cn=3, top=3, flags=0, Z=p, rows=p, W=p, bias=p,
             state=None, cls=p, prob=p, proba=None):
        return fn(Z, 8, d, ldz, rows, n, W, bias, state, F, Cn, top, flags, cls, prob, proba, None)

    for bad, text in ((dict(d=0), b"bad shape"), (dict(ldz=3), b"bad shape"), (dict(n=-1), b"bad shape"),
                      (dict(Cn=1), b"C must be"), (dict(Cn=65), b"C must be"), (dict(Cn=0, flags=1, state=p), b"C must be"),
                      (dict(top=0), b"top_m"), (dict(top=9), b"top_m"), (dict(F=0), b"number of fits"),
                      (dict(flags=4), b"unknown flags"), (dict(flags=1), b"needs col_state"),
                      (dict(flags=2), b"needs proba"), (dict(Z=None), b"null pointer"), (dict(rows=None), b"null pointer"),
                      (dict(W=None), b"null pointer"), (dict(bias=None), b"null pointer"), (dict(cls=None), b"null pointer"),
                      (dict(prob=None), b"null pointer")):
        assert call(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"probe_predict" in lib.clane_last_error()
    assert call(fn=lib.clane_probe_predict_bf16, Cn=70) == -1 and call(fn=lib.clane_probe_predict_f64, d=-1) == -1


def test_backend_without_the_call_says_so():
    with pytest.raises(NotImplementedError, match="OracleKernels has no probe_predict"):
        OracleKernels().probe_predict(None, 1, None, None, None, 1, 2, None, None)


# ---- per-fit l2 ---------------------------------------------------------------------------------------------------
def test_per_fit_l2_is_three_single_fits_and_none_is_the_scalar():
    n, d, Cn = 90, 5, 4
    X, y = planted(n, d, Cn, 1.0, seed=1)
    eng = _engine(X)
    rows = _rows(eng, n)
    split = torch.ones(n, 3, dtype=torch.uint8)
    split[::3, 0] = 0
    split[1::3, 1] = 0
    values = [0.05, 1.0, 20.0]
    probe = LabelProbe(eng, l2=1.0, gtol=1e-7)
    batched = probe.fit(eng.Zcur, rows, y, split, Cn, l2=values)
    names = ("W", "b", "objective", "iterations", "pred", "grad_max")
    for f, v in enumerate(values):
        alone = probe.fit(eng.Zcur, rows, y, split[:, f:f + 1].contiguous(), Cn, l2=[v])
        scalar = LabelProbe(eng, l2=v, gtol=1e-7).fit(eng.Zcur, rows, y, split[:, f:f + 1].contiguous(), Cn)
        for name in names:
            assert torch.equal(getattr(batched, name)[..., f:f + 1] if name == "pred" else getattr(batched, name)[f:f + 1],
                               getattr(alone, name)), (name, f)
            assert torch.equal(getattr(alone, name), getattr(scalar, name)), (name, f)
    assert float(batched.W[0].abs().max()) > float(batched.W[2].abs().max())       # more penalty, smaller weights
    today = probe.fit(eng.Zcur, rows, y, split, Cn)
    same = probe.fit(eng.Zcur, rows, y, split, Cn, l2=None)
    ones = probe.fit(eng.Zcur, rows, y, split, Cn, l2=torch.ones(3))
    for name in names:
        assert torch.equal(getattr(today, name), getattr(same, name)) and torch.equal(getattr(today, name), getattr(ones, name))
    masks = label_masks([[int(c)] + ([0] if i % 4 == 0 else []) for i, c in enumerate(y)], Cn)
    a = probe.fit_multilabel(eng.Zcur, rows, masks, split, Cn, l2=values)
    b = probe.fit_multilabel(eng.Zcur, rows, masks, split[:, 2:3].contiguous(), Cn, l2=[values[2]])
    assert torch.equal(a.W[2:3], b.W) and torch.equal(a.pred[:, 2:3], b.pred)
    for bad in ([1.0, 2.0], [1.0, -1.0, 2.0], [1.0, float("nan"), 2.0]):
        with pytest.raises(ValueError, match="one finite value >= 0 per fit"):
            probe.fit(eng.Zcur, rows, y, split, Cn, l2=bad)


# ---- cross-validation -----------------------------------------------------------------------------------------------
def test_folds_partition_the_rows_and_every_row_is_held_out_once_per_l2():
    n, folds, grid = 53, 4, [0.1, 1.0, 10.0]
    fold = fold_assignment(n, folds, seed=3)
    assert sorted(np.bincount(fold.numpy(), minlength=folds).tolist()) == [13, 13, 13, 14]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))          # make_splits' generator convention
    assert torch.equal(fold[perm], torch.arange(n) % folds)
    assert not torch.equal(fold, fold_assignment(n, folds, seed=4))
    X, y = planted(n, 4, 3, 1.5, seed=2)
    eng = _engine(X)
    cv = LabelProbe(eng, gtol=1e-6).cross_validate(eng.Zcur, _rows(eng, n), y, 3, grid, folds=folds, seed=3)
    assert tuple(cv.split.shape) == (n, folds * len(grid)) and torch.equal(cv.fold, fold)
    held = cv.split == 0
    for g in range(len(grid)):
        assert torch.equal(held[:, g * folds:(g + 1) * folds].sum(1), torch.ones(n, dtype=torch.int64))
        assert torch.equal(held[:, g * folds:(g + 1) * folds], fold[:, None] == torch.arange(folds)[None, :])
    assert cv.l2_per_fit.tolist() == [v for v in grid for _ in range(folds)]
    assert [r["l2"] for r in cv.rows] == grid and all(r["fits_used"] == folds for r in cv.rows)
    assert all(set(r) == {"l2", "log_loss", "accuracy", "ece", "fits_used"} for r in cv.rows)
    with pytest.raises(ValueError, match="folds must be in"):
        LabelProbe(eng).cross_validate(eng.Zcur, _rows(eng, n), y, 3, grid, folds=1)
    with pytest.raises(ValueError, match="distinct finite values"):
        LabelProbe(eng).cross_validate(eng.Zcur, _rows(eng, n), y, 3, [1.0, 1.0])


def test_held_out_log_loss_accuracy_and_ece_equal_a_float64_recomputation():
    n, d, Cn, folds, grid = 80, 5, 4, 3, [0.3, 3.0]
    X, y = planted(n, d, Cn, 1.0, seed=5)
    eng = _engine(X)
    cv = LabelProbe(eng, gtol=1e-7).cross_validate(eng.Zcur, _rows(eng, n), y, Cn, grid, folds=folds, seed=1)
    for f in range(folds * len(grid)):
        held = cv.split[:, f] == 0
        logits = X[held] @ cv.fit.W[f].double().T + cv.fit.b[f].double()
        logp = torch.log_softmax(logits, 1)
        want = float(-logp[torch.arange(int(held.sum())), y[held]].mean())
        assert float(cv.log_loss[f]) == pytest.approx(want, rel=1e-12)
        hit = logits.argmax(1) == y[held]
        assert float(cv.score[f]) == pytest.approx(float(hit.double().mean()), abs=1e-12)
        conf = torch.softmax(logits, 1).amax(1)
        b = (conf * 10).floor().long().clamp(max=9)
        ece = sum(abs(float(hit[b == k].double().sum()) - float(conf[b == k].sum())) for k in range(10)) / int(held.sum())
        assert float(cv.ece[f]) == pytest.approx(ece, abs=1e-12)
    for g, row in enumerate(cv.rows):
        assert row["log_loss"] == pytest.approx(float(cv.log_loss[g * folds:(g + 1) * folds].mean()), rel=1e-12)
    # multi-label: the sigmoid loss over the fitted columns of the held-out rows, micro-F1 from pred
    masks = label_masks([[int(c)] + ([(int(c) + 1) % Cn] if i % 3 == 0 else []) for i, c in enumerate(y)], Cn)
    cvm = LabelProbe(eng, gtol=1e-7).cross_validate(eng.Zcur, _rows(eng, n), masks, Cn, grid, folds=folds, seed=1,
                                                    multilabel=True)
    assert cvm.ece is None and all(set(r) == {"l2", "log_loss", "micro_f1", "fits_used"} for r in cvm.rows)
    Y = classify.mask_bits(masks, Cn).double()
    for f in range(folds * len(grid)):
        held = cvm.split[:, f] == 0
        logits = X[held] @ cvm.fit.W[f].double().T + cvm.fit.b[f].double()
        term = torch.nn.functional.softplus(logits) - Y[held] * logits
        assert float(cvm.log_loss[f]) == pytest.approx(float(term.sum() / int(held.sum())), rel=1e-12)


def test_noisy_labels_choose_a_larger_l2_than_clean_separable_data():
    n, d, Cn, grid = 150, 6, 3, [0.01, 1.0, 100.0]
    chosen = {}
    for name, sep, noise in (("clean", 4.0, 0.0), ("noisy", 0.7, 0.6)):
        X, y = planted(n, d, Cn, sep, seed=11, noise=noise)
        eng = _engine(X)
        cv = LabelProbe(eng, gtol=1e-6).cross_validate(eng.Zcur, _rows(eng, n), y, Cn, grid, folds=3, seed=0)
        chosen[name] = cv.l2
        assert cv.l2 == choose_l2(cv.rows) and cv.table()["l2"] == cv.l2
    assert chosen["noisy"] > chosen["clean"], chosen


def test_the_tie_rule_and_skipped_rows():
    row = lambda l2, ll, used=3: {"l2": l2, "log_loss": ll, "accuracy": 0.5, "fits_used": used}     # noqa: E731
    assert choose_l2([row(0.1, 0.5), row(1.0, 0.5), row(10.0, 0.7)]) == 1.0           # ties: the larger l2
    assert choose_l2([row(10.0, 0.5), row(1.0, 0.5), row(0.1, 0.5)]) == 10.0          # whatever the order
    assert choose_l2([row(0.1, 0.4), row(1.0, 0.5)]) == 0.1
    assert choose_l2([row(0.1, float("nan"), 0), row(1.0, 0.9)]) == 1.0               # a row without a used fit: never
    with pytest.raises(ValueError, match="every fit was skipped"):
        choose_l2([row(0.1, float("nan"), 0)])


# ---- the kept model -------------------------------------------------------------------------------------------------
def _trained(multilabel=False, l2=(0.1, 1.0)):
    n, d, Cn = 60, 4, 3
    X, y = planted(n, d, Cn, 2.0, seed=7)
    eng = _engine(X)
    labels = [[int(c)] + ([2] if i % 5 == 0 else []) for i, c in enumerate(y[:40])] if multilabel else y[:40].tolist()
    model = LabelProbe(eng, gtol=1e-6).train(list(range(40)), labels, Cn, l2=list(l2), folds=3, seed=2,
                                             multilabel=multilabel, class_names=["ant", "bee", "cat"])
    return eng, X, y, model


def test_train_returns_a_model_and_save_load_keeps_its_bits(tmp_path):
    for multilabel in (False, True):
        eng, X, y, model = _trained(multilabel)
        assert model.W.shape == (3, 4) and model.b.shape == (3,) and model.d == 4 and model.n_train == 40
        assert model.l2 in (0.1, 1.0) and model.cv["l2"] == model.l2 and len(model.cv["rows"]) == 2 and model.converged
        assert (model.col_state is not None) == multilabel and model.table == "Z"
        back = LabelModel.load(model.save(tmp_path / "m.npz"), d=4)
        for name in ("W", "b"):
            assert getattr(back, name).dtype == getattr(model, name).dtype
            assert getattr(back, name).tobytes() == getattr(model, name).tobytes()
        for name in ("class_names", "multilabel", "l2", "d", "table", "n_train", "objective", "iterations", "converged", "cv"):
            assert getattr(back, name) == getattr(model, name), name
        assert (back.col_state is None) if not multilabel else np.array_equal(back.col_state, model.col_state)
        a = model.predict_table(eng, top=2, proba=True)
        b = back.predict_table(eng, top=2, proba=True)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
        with np.load(tmp_path / "m.npz") as z:             # numpy alone, nothing pickled
            assert set(z.files) == set(classify.MODEL_KEYS)
    one = LabelProbe(eng).train(list(range(40)), y[:40].tolist(), 3, l2=0.5)
    assert one.cv is None and one.l2 == 0.5 and one.class_names == ["0", "1", "2"]


def test_load_refuses_a_wrong_d_a_truncated_file_and_a_name_count_mismatch(tmp_path):
    _, _, _, model = _trained()
    path = model.save(tmp_path / "m.npz")
    with pytest.raises(ValueError, match="d = 4, not 5"):
        LabelModel.load(path, d=5)
    data = path.read_bytes()
    (tmp_path / "cut.npz").write_bytes(data[:len(data) // 2])
    with pytest.raises(ValueError, match="is no label model"):
        LabelModel.load(tmp_path / "cut.npz")
    with np.load(path) as z:
        fields = {k: z[k] for k in z.files}
    np.savez(tmp_path / "names.npz", **{**fields, "class_names": np.array(["ant", "bee"])})
    with pytest.raises(ValueError, match="2 class names for the 3 classes"):
        LabelModel.load(tmp_path / "names.npz")
    np.savez(tmp_path / "width.npz", **{**fields, "d": np.int64(6)})
    with pytest.raises(ValueError, match=r"no \[C, d = 6\] weights"):
        LabelModel.load(tmp_path / "width.npz")
    np.savez(tmp_path / "lacks.npz", **{k: v for k, v in fields.items() if k != "b"})
    with pytest.raises(ValueError, match=r"lacks \['b'\]"):
        LabelModel.load(tmp_path / "lacks.npz")


# ---- the selection rule -----------------------------------------------------------------------------------------------
def test_selection_rule_in_the_double_and_through_predict():
    val = torch.tensor([[1.0, 3.0, 3.0], [2.0, float("nan"), 2.0], [float("-inf"), 0.0, float("nan")]], dtype=torch.float64)
    cls, pr = select_top(val, torch.full_like(val, 0.25), 5)
    assert cls.tolist() == [[1, 2, 0, -1, -1], [0, 2, -1, -1, -1], [1, -1, -1, -1, -1]]      # ties low; NaN, -inf never
    assert pr.tolist() == [[0.25, 0.25, 0.25, 0, 0], [0.25, 0.25, 0, 0, 0], [0.25, 0, 0, 0, 0]]
    # through LabelProbe.predict: integer logits, so ties are exact
    X = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [2.0, 2.0]], dtype=torch.float64)
    eng = _engine(X)
    probe, rows = LabelProbe(eng), _rows(eng, 4)
    W = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]], dtype=torch.float64)        # class 2 repeats class 0
    b = torch.zeros(3, dtype=torch.float64)
    out = probe.predict(eng.Zcur, rows, W, b, 3, top=5, proba=True)
    assert tuple(out.classes.shape) == (4, 1, 5) and out.classes.dtype == torch.int32
    assert out.classes[:, 0].tolist() == [[0, 2, 1, -1, -1], [1, 0, 2, -1, -1], [0, 1, 2, -1, -1], [0, 1, 2, -1, -1]]
    assert torch.equal(out.probs[:, 0, 3:], torch.zeros(4, 2, dtype=torch.float64))
    assert torch.allclose(out.proba[:, 0].sum(1), torch.ones(4, dtype=torch.float64))
    assert torch.equal(out.probs[2, 0, :3], torch.full((3,), 1.0 / 3.0, dtype=torch.float64))
    assert bool((out.probs[:, 0, :2] >= out.probs[:, 0, 1:3]).all())
    # sigmoid mode: a constant-positive column is first with p exactly 1, a constant-negative one is never named and has
    # p exactly 0 -- the slots it leaves are the fill at the end
    out = probe.predict(eng.Zcur, rows, W, b, 3, top=3, proba=True, multilabel=True, col_state=[0, -1, 1])
    assert out.classes[:, 0].tolist() == [[2, 0, -1]] * 4
    assert torch.equal(out.probs[:, 0, 0], torch.ones(4, dtype=torch.float64)) and float(out.probs[:, 0, 2].abs().max()) == 0.0
    assert torch.equal(out.proba[:, 0, 1], torch.zeros(4, dtype=torch.float64))
    assert torch.equal(out.proba[:, 0, 2], torch.ones(4, dtype=torch.float64))
    assert torch.equal(out.proba[:, 0, 0], torch.sigmoid(X[:, 0]))
    # NaN is never chosen
    Wn = W.clone()
    Wn[1, 1] = float("nan")
    out = probe.predict(eng.Zcur, rows, Wn, b, 3, top=3, multilabel=True)
    assert out.classes[:, 0].tolist() == [[0, 2, -1]] * 4
    # several models at once, and one model given as [C, d]
    both = probe.predict(eng.Zcur, rows, torch.stack([W, -W]), torch.stack([b, b]), 3, top=1)
    assert both.classes[:, :, 0].tolist() == [[0, 1], [1, 0], [0, 0], [0, 0]]
    for bad in (0, 9):
        with pytest.raises(ValueError, match="top must be in 1..8"):
            probe.predict(eng.Zcur, rows, W, b, 3, top=bad)
    with pytest.raises(ValueError, match="the weights need d = 3"):
        probe.predict(eng.Zcur, rows, torch.zeros(3, 3, dtype=torch.float64), b, 3)


def test_predict_rows_reads_a_matrix_with_identity_rows_and_graph_methods(tmp_path):
    eng, X, y, model = _trained()
    verts = [5, 59, 0, 41]
    a = model.predict_table(eng, verts, top=2, proba=True)
    b = model.predict_rows(eng, X[verts].contiguous(), top=2, proba=True)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and a[0].shape == (4, 2) and a[2].shape == (4, 3)
    assert float((a[0][:, 0] == y[verts].numpy()).mean()) >= 0.75           # well separated data
    with pytest.raises(ValueError, match="fitted for d = 4"):
        model.predict_rows(eng, torch.zeros(2, 3, dtype=torch.float64))
    eng.world = 2
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        model.predict_table(eng)


# ---- the CLI ----------------------------------------------------------------------------------------------------------
CONFIG = N.CONFIG


def _karate(tmp_path, monkeypatch):
    import clane_amd.__main__ as M
    k = load_golden("g2_karate_csr.npz")
    rng = np.random.default_rng(0)
    Xc = rng.standard_normal((34, 4)).astype(np.float32)
    root = write_data_root(tmp_path / "karate", k["vertex_ids"], k["edge_src"], k["edge_dst"], Xc)
    ids = [str(v) for v in k["vertex_ids"]]
    lines = (GOLDEN / "g2_karate_Y.tsv").read_text().splitlines()
    (root / "Y").write_text("\n".join(lines[::2]) + "\n")                  # every other vertex is labelled
    new_ids = ["new-b", "new-a", "new-c"]
    N.write_arrivals(root / "arrivals", V="\n".join(new_ids) + "\n", E=f"new-b\t{ids[3]}\nnew-a\t{ids[0]}\n",
                     C_=rng.standard_normal((3, 4)).astype(np.float32))
    kernels = PredictOracleKernels()

    def cpu_engine(self, device=None, cosine_mode="reference", **kw):
        if self._engine is None:
            self._attach_engine(SweepEngine(self.csr, self.X, "cpu", kernels, cosine_mode=cosine_mode))
        if self._dirty:
            self._engine.set_Z(self._Z_host)
            self._dirty = False
        return self._engine
    monkeypatch.setattr(Graph, "engine", cpu_engine)

    def run(section, out):
        cfg = tmp_path / f"{out}.yaml"
        cfg.write_text(CONFIG + section)
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg)]))
        return tmp_path / out
    return root, ids, len(lines[::2]), new_ids, run


def _parse(path):
    rows = [line.split("\t") for line in path.read_text().splitlines()]
    return [(r[0], r[1::2], [float(v) for v in r[2::2]]) for r in rows]


def test_cli_writes_the_three_files_and_load_reproduces_them(tmp_path, monkeypatch):
    root, ids, labelled, new_ids, run = _karate(tmp_path, monkeypatch)
    plain = run("", "plain")
    out = run("\nlabel_prediction:\n  labels: Y\n  l2: [0.01, 0.1, 1, 10]\n  folds: 3\n  seed: 1\n", "pred")
    assert sorted(p.name for p in plain.iterdir()) == ["Z.npy"]           # without the section: what it wrote before
    assert sorted(p.name for p in out.iterdir()) == ["Z.npy", "label_model.npz", "label_prediction.json",
                                                     "predicted_labels.tsv"]
    assert (plain / "Z.npy").read_bytes() == (out / "Z.npy").read_bytes()
    rows = _parse(out / "predicted_labels.tsv")
    labelled_ids = {line.split("\t")[0] for line in (root / "Y").read_text().splitlines()}
    assert len(rows) == 34 - labelled and [r[0] for r in rows] == [i for i in ids if i not in labelled_ids]
    report = json.loads((out / "label_prediction.json").read_text())
    names = report["class_names"]
    for _, classes, probs in rows:
        assert len(classes) == len(probs) == min(3, len(names)) and set(classes) <= set(names)
        assert all(a >= b for a, b in zip(probs, probs[1:])) and sum(probs) <= 1.0 + 1e-6
    assert report["model"] == "fitted" and report["labelled"] == labelled and report["predicted"] == 34 - labelled
    assert report["l2"] in (0.01, 0.1, 1.0, 10.0) and report["cv"]["l2"] == report["l2"] and report["cv"]["folds"] == 3
    assert [r["l2"] for r in report["cv"]["rows"]] == [0.01, 0.1, 1.0, 10.0] and not report["multilabel"]
    assert sum(report["top1_probability_histogram"]) == 34 - labelled and len(report["top1_probability_histogram"]) == 10
    assert isinstance(report["iterations"], int) and isinstance(report["converged"], bool) and report["objective"] > 0
    # the repr of the float: the text reads back to the same bits
    model = LabelModel.load(out / "label_model.npz")
    assert model.W.dtype == np.float32 and all(np.float32(v) == v for _, _, probs in rows for v in probs)
    # load: the same predictions byte for byte from the saved model, and no model written again
    everyone = run("\nlabel_prediction:\n  labels: Y\n  l2: [0.01, 0.1, 1, 10]\n  folds: 3\n  seed: 1\n  scope: all\n", "all")
    assert (everyone / "label_model.npz").read_bytes() == (out / "label_model.npz").read_bytes()
    (root / "saved.npz").write_bytes((out / "label_model.npz").read_bytes())
    again = run("\nlabel_prediction:\n  load: saved.npz\n", "loaded")
    assert not (again / "label_model.npz").exists()
    assert json.loads((again / "label_prediction.json").read_text())["model"] == "loaded"
    assert len(_parse(again / "predicted_labels.tsv")) == 34
    assert (again / "predicted_labels.tsv").read_bytes() == (everyone / "predicted_labels.tsv").read_bytes()
    (root / "only").mkdir()
    unl = [i for i in ids if i not in labelled_ids]
    g = Graph(root, embedding_dim=4)
    g.set_Z(torch.from_numpy(np.load(out / "Z.npy")))
    v, classes, probs = g.predict_labels(model, [ids.index(i) for i in unl], top=3)
    classify.write_predictions_tsv(root / "only" / "p.tsv", unl, model.class_names, classes, probs)
    assert (root / "only" / "p.tsv").read_bytes() == (out / "predicted_labels.tsv").read_bytes()
    wide = LabelModel(**{**vars(model), "W": np.zeros((len(model.class_names), 6), np.float32), "d": 6})
    with pytest.raises(ValueError, match="fitted for d = 6, this graph has d = 4"):
        g.predict_labels(wide)
    fitted = g.fit_labels(root / "Y", l2=[0.01, 0.1, 1, 10], folds=3, seed=1)      # the Graph methods: the CLI's model
    assert fitted.W.tobytes() == model.W.tobytes() and fitted.cv == model.cv and fitted.class_names == model.class_names


def test_cli_predicts_the_arrivals_in_their_order(tmp_path, monkeypatch):
    root, ids, labelled, new_ids, run = _karate(tmp_path, monkeypatch)
    out = run("\nnew_vertices:\n  root: arrivals\n\nlabel_prediction:\n  labels: Y\n  top: 2\n  multilabel: true\n", "new")
    rows = _parse(out / "predicted_labels_new.tsv")
    assert [r[0] for r in rows] == new_ids
    report = json.loads((out / "label_prediction.json").read_text())
    assert report["predicted_new"] == 3 and report["multilabel"] and report["cv"] is None and report["l2"] == 1.0
    model = LabelModel.load(out / "label_model.npz")
    eng = _engine(torch.from_numpy(np.load(out / "Z.npy")))
    classes, probs = model.predict_rows(eng, torch.from_numpy(np.load(out / "Z_new.npy")), top=2)
    assert [[model.class_names[c] for c in cs if c >= 0] for cs in classes.tolist()] == [r[1] for r in rows]


@pytest.mark.parametrize("section,error,text", [
    ("  labels: Y\n  depth: 3\n", ValueError, "unknown keys"),
    ("  labels: 3\n", ValueError, "labels must be a file name"),
    ("  labels: Y\n  top: 0\n", ValueError, "top must be an integer in 1..8"),
    ("  labels: Y\n  top: 9\n", ValueError, "top must be an integer in 1..8"),
    ("  labels: Y\n  l2: [1, 2]\n  folds: 1\n", ValueError, "folds must be an integer >= 2"),
    ("  labels: Y\n  folds: 3\n", ValueError, "folds is given but l2 is no list"),
    ("  labels: Y\n  l2: -1\n", ValueError, "l2 must be a number"),
    ("  labels: Y\n  l2: [1, 1]\n", ValueError, "l2 must be a number"),
    ("  labels: Y\n  multilabel: 1\n", ValueError, "multilabel must be true or false"),
    ("  labels: Y\n  scope: some\n", ValueError, "scope must be"),
    ("  labels: Y\n  seed: x\n", ValueError, "seed must be an integer"),
    ("  labels: nowhere\n", FileNotFoundError, "labels file"),
    ("  load: nowhere.npz\n", FileNotFoundError, "load file"),
    ("  top: 3\n", ValueError, "exactly one of"),
    ("  labels: Y\n  load: m.npz\n", ValueError, "exactly one of"),
    ("  load: m.npz\n  multilabel: true\n", ValueError, "have no effect on a loaded model"),
    ("  load: m.npz\n  l2: 2\n", ValueError, "have no effect on a loaded model"),
])
def test_cli_section_is_validated_before_the_graph_is_loaded(monkeypatch, tmp_path, section, error, text):
    import clane_amd.__main__ as M

    def touched(*a, **k):
        raise AssertionError("the run went on to set up devices")
    monkeypatch.setattr(M, "_distributed_setup", touched)
    monkeypatch.setattr(M, "Graph", touched)
    (tmp_path / "Y").write_text("a\tx\n")
    (tmp_path / "m.npz").write_bytes(b"")
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG + "\nlabel_prediction:\n" + section)
    args = M.get_parser().parse_args(["--data_root", str(tmp_path), "--output_root", str(tmp_path / "o"),
                                      "--config_file", str(cfg)])
    with pytest.raises(error, match=text):
        M.embedding(args)
    monkeypatch.setenv("WORLD_SIZE", "2")
    cfg.write_text(CONFIG + "\nlabel_prediction:\n  labels: Y\n")
    with pytest.raises(NotImplementedError, match="label_prediction: .* ONE GPU"):
        M.embedding(args)
    assert set(vars(M.get_parser().parse_args([]))) == {                # no new flag
        "command", "data_root", "output_root", "config_file", "save_history", "num_workers", "init_Z", "exchange",
        "train_similarity", "predict_links", "link_sources", "gpu"}
