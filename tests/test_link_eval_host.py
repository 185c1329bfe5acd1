"""Held-out link evaluation, the parts that need no GPU: the new entry points' declarations and host-side argument checks,
the refusals of the surface, the metrics' arithmetic on hand-made counts, the config section's refusal on several GPUs
and the hold-out split."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.links import LinkMetrics, hold_out_edges, link_metrics, read_link_pairs, split_edges

from .conftest import load_golden, write_data_root

ROOT = Path(__file__).resolve().parent.parent

NEW_SYMBOLS = [f"clane_rank_count_{s}" for s in ("f32", "f64", "bf16")]


def test_new_symbols_are_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "clane_hip.h").read_text(), flags=re.S)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", header)
        assert decl, name
        assert name in _hip.SIGNATURES, name
        restype, argtypes = _hip.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(decl.group(1).split(",")) == 20, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define CLANE_ABI_VERSION 5\b", header) and _hip.ABI_VERSION == 5
    assert lib.clane_abi_version() == 5


def test_argument_validation_reaches_last_error():
    # refused on the host before any launch: safe without a GPU
    lib = _hip.load_library()
    p = C.cast((C.c_float * 64)(), C.c_void_p)

    def count(fn=lib.clane_rank_count_f32, d=8, lds=8, ldn=8, mode=2, sums2=None, sq=None, rp=None, ci=None, n_slabs=1, S=p,
              t_rows=p, counts=p, B=2, rows=4):
        return fn(S, lds, p, ldn, rows, d, p, t_rows, B, mode, sums2, sq, None, rp, ci, 1, n_slabs, p, counts, None)

    for bad, text in ((dict(n_slabs=0), b"n_slabs"), (dict(n_slabs=-3), b"n_slabs"), (dict(d=0), b"bad shape"),
                      (dict(lds=7), b"bad shape"), (dict(ldn=7), b"bad shape"), (dict(B=-1), b"bad shape"),
                      (dict(rows=-1), b"bad shape"), (dict(mode=9), b"unknown mode"), (dict(mode=0), b"needs sums2"),
                      (dict(mode=1), b"needs sq"), (dict(rp=p), b"excl_rowptr and excl_colidx"),
                      (dict(ci=p), b"excl_rowptr and excl_colidx"), (dict(S=None), b"null pointer"),
                      (dict(t_rows=None), b"null pointer"), (dict(counts=None), b"null pointer")):
        assert count(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"rank_count" in lib.clane_last_error()
    assert count(B=0, S=None, t_rows=None, counts=None) == 0           # no pairs: nothing to do, no launch
    assert count(fn=lib.clane_rank_count_bf16, mode=1) == -1 and b"rank_count" in lib.clane_last_error()
    assert count(fn=lib.clane_rank_count_f64, n_slabs=0) == -1 and b"rank_count" in lib.clane_last_error()


def test_backend_without_rank_count_says_so():
    from .oracle_kernels import OracleKernels
    with pytest.raises(NotImplementedError, match="OracleKernels has no rank_count"):
        OracleKernels().rank_count(None, None, 0, 1, None, None, 2, None, None, None, None, None, True, 1, None, None)


def test_rank_pairs_checks_its_arguments_then_needs_the_kernel():
    from clane_amd.engine import SweepEngine
    from clane_amd.links import LinkRanker
    from clane_amd.partition import HostCSR
    from clane_amd.similarity import CosineSimilarity
    from .oracle_kernels import OracleKernels
    csr = HostCSR(6, np.array([0, 1, 2, 3, 4, 5, 6], dtype=np.int64), np.array([1, 2, 3, 4, 5, 0], dtype=np.int32))
    eng = SweepEngine(csr, torch.zeros(6, 4), "cpu", OracleKernels())
    ranker = LinkRanker(eng, CosineSimilarity())
    with pytest.raises(ValueError, match="one entry per pair"):
        ranker.rank_pairs([0, 1], [2])
    with pytest.raises(ValueError, match=r"vertex indices must be in \[0, 6\)"):
        ranker.rank_pairs([0, 6], [1, 2])
    with pytest.raises(ValueError, match=r"vertex indices must be in \[0, 6\)"):
        ranker.evaluate([0], [-1])
    with pytest.raises(ValueError, match="batch must be"):
        ranker.rank_pairs([0], [1], batch=0)
    with pytest.raises(NotImplementedError, match="OracleKernels has no rank_count"):
        ranker.rank_pairs([0, 1], [2, 3])
    with pytest.raises(NotImplementedError, match="OracleKernels has no rank_count"):
        ranker.evaluate([0, 1], [2, 3])


def test_link_metrics_arithmetic():
    # pair 0: alone at the top; pair 1: two above, a tie on each side -> rank 1 + 2 + 2 / 2 = 4;
    # pair 2: one tie -> the half rank 1.5; pair 3: no rank; pair 4: nothing eligible (rank 1, left out of the AUC)
    greater = torch.tensor([0, 2, 0, -1, 0])
    lower = torch.tensor([0, 1, 1, -1, 0])
    higher = torch.tensor([0, 1, 0, -1, 0])
    eligible = torch.tensor([9, 10, 4, -1, 0])
    m = link_metrics(greater, lower, higher, eligible, hits=(1, 2, 4))
    assert isinstance(m, LinkMetrics) and m.pairs == 4 and m.skipped == 1
    assert m.mean_rank == pytest.approx((1 + 4 + 1.5 + 1) / 4, abs=1e-15)
    assert m.mrr == pytest.approx((1 + 1 / 4 + 1 / 1.5 + 1) / 4, abs=1e-15)
    assert m.hits == {1: pytest.approx(2 / 4), 2: pytest.approx(3 / 4), 4: pytest.approx(1.0)}
    assert m.auc == pytest.approx(((9 - 0) / 9 + (10 - 2 - 1) / 10 + (4 - 0.5) / 4) / 3, abs=1e-15)
    d = m.as_dict()
    assert set(d) == {"pairs", "skipped", "mrr", "mean_rank", "hits", "auc"} and set(d["hits"]) == {"1", "2", "4"}
    assert d["hits"]["2"] == m.hits[2] and d["pairs"] == 4
    # a model that scores everything the same: every rank is the middle one, the AUC a half
    n = 11
    flat = link_metrics(torch.zeros(3, dtype=torch.int64), torch.tensor([0, 5, 10]), torch.tensor([10, 5, 0]),
                        torch.full((3,), 10))
    assert flat.mean_rank == (n + 1) / 2 and flat.auc == 0.5 and flat.hits[1] == 0.0
    nothing = link_metrics(torch.tensor([-1]), torch.tensor([-1]), torch.tensor([-1]), torch.tensor([-1]))
    assert nothing.pairs == 0 and nothing.skipped == 1 and nothing.mrr != nothing.mrr        # nan
    with pytest.raises(ValueError, match="hits"):
        link_metrics(greater, lower, higher, eligible, hits=(0,))


def test_link_evaluation_is_refused_on_several_gpus_before_the_graph_is_loaded(monkeypatch, tmp_path):
    import clane_amd.__main__ as M
    monkeypatch.setenv("WORLD_SIZE", "2")

    def touched(*a, **k):
        raise AssertionError("the run went on to set up devices")
    monkeypatch.setattr(M, "_distributed_setup", touched)
    monkeypatch.setattr(M, "Graph", touched)
    cfg = tmp_path / "config.yaml"
    cfg.write_text("graph:\n  embedding_dim: 8\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
                   "embedder:\n  gamma: 0.76\n  tolerence: 3\n\nlink_evaluation:\n  pairs: held_out.tsv\n")
    args = M.get_parser().parse_args(["--data_root", str(tmp_path), "--output_root", str(tmp_path / "o"),
                                      "--config_file", str(cfg)])
    with pytest.raises(NotImplementedError, match="one GPU"):
        M.embedding(args)
    monkeypatch.setenv("WORLD_SIZE", "1")
    cfg.write_text(cfg.read_text().replace("  pairs: held_out.tsv\n", "  hits: [1]\n"))
    with pytest.raises(ValueError, match="link_evaluation"):           # a section without its pairs file
        M.embedding(args)


def test_parser_has_exactly_the_destinations_it_had():
    import clane_amd.__main__ as M
    plain = vars(M.get_parser().parse_args([]))
    assert set(plain) == {"command", "data_root", "output_root", "config_file", "save_history", "num_workers", "init_Z",
                          "exchange", "train_similarity", "predict_links", "link_sources", "gpu"}


def test_read_link_pairs(tmp_path):
    vertex_ids = ["a", "b", "c", "a"]
    (tmp_path / "p.tsv").write_text("c\ta\n\nb\tb\n")
    assert read_link_pairs(tmp_path / "p.tsv", vertex_ids) == ([2, 1], [0, 1])        # first occurrence, file order
    (tmp_path / "bad.tsv").write_text("c\ta\nb\tzz\n")
    with pytest.raises(ValueError, match="'zz'"):
        read_link_pairs(tmp_path / "bad.tsv", vertex_ids)
    (tmp_path / "short.tsv").write_text("c\n")
    with pytest.raises(ValueError, match="line 1"):
        read_link_pairs(tmp_path / "short.tsv", vertex_ids)


def test_hold_out_edges_on_karate(tmp_path):
    kc = load_golden("g2_karate_csr.npz")
    X = np.random.default_rng(0).standard_normal((34, 4)).astype(np.float32)
    root = write_data_root(tmp_path / "karate", kc["vertex_ids"], kc["edge_src"], kc["edge_dst"], X)
    original = sorted((root / "E").read_text().splitlines())

    def read(folder, name):
        return (folder / name).read_text().splitlines()

    kept_n, held_n = hold_out_edges(root, tmp_path / "a", fraction=0.3, seed=7)
    kept, held = read(tmp_path / "a", "E"), read(tmp_path / "a", "held_out.tsv")
    assert (kept_n, held_n) == (len(kept), len(held)) and held_n > 0
    assert sorted(kept + held) == original                             # the original edge multiset ...
    assert not set(kept) & set(held)                                   # ... in two disjoint parts
    sources = {line.split("\t")[0] for line in original}
    assert {line.split("\t")[0] for line in kept} == sources           # whoever had out-edges keeps at least one
    assert (tmp_path / "a" / "V").read_bytes() == (root / "V").read_bytes()
    assert (tmp_path / "a" / "C.npy").read_bytes() == (root / "C.npy").read_bytes()
    hold_out_edges(root, tmp_path / "b", fraction=0.3, seed=7)         # the same seed: the same files
    assert read(tmp_path / "b", "E") == kept and read(tmp_path / "b", "held_out.tsv") == held
    hold_out_edges(root, tmp_path / "c", fraction=0.3, seed=8)
    assert read(tmp_path / "c", "held_out.tsv") != held
    assert hold_out_edges(root, tmp_path / "z", fraction=0.0, seed=7) == (len(original), 0)
    assert sorted(read(tmp_path / "z", "E")) == original and read(tmp_path / "z", "held_out.tsv") == []
    # nearly everything drawn: still one out-edge per source, and the copies of a repeated edge go together
    held_mask = split_edges(["u", "u", "v", "u"], ["v", "w", "u", "v"], fraction=0.999, seed=1)
    assert held_mask.tolist() == [False, True, False, False]
    with pytest.raises(ValueError, match="fraction"):
        split_edges(["u"], ["v"], fraction=1.0, seed=0)
    # the tool is the same function behind a command line
    import subprocess
    import sys
    subprocess.run([sys.executable, str(ROOT / "tools" / "hold_out_edges.py"), str(root), str(tmp_path / "t"),
                    "--fraction", "0.3", "--seed", "7"], check=True, capture_output=True)
    assert read(tmp_path / "t", "E") == kept and read(tmp_path / "t", "held_out.tsv") == held
