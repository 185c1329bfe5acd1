"""Link prediction, the parts that need no GPU: the CLI flags, the refusal on several GPUs, the links.tsv format, the
host-side argument checks of the three new entry-point families and the slab rule of plan.py."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from clane_amd import _hip, plan
from clane_amd.links import read_link_sources, write_links_tsv

ROOT = Path(__file__).resolve().parent.parent

NEW_SYMBOLS = ([f"clane_rank_scores_{s}" for s in ("f32", "f64", "bf16")] + [f"clane_rank_merge_{s}" for s in ("f32", "f64")]
               + [f"clane_pair_score_{s}" for s in ("f32", "f64", "bf16")])


def test_parser_accepts_the_new_flags_and_leaves_the_old_ones_alone():
    import clane_amd.__main__ as M
    old = ["--data_root", "d", "--output_root", "o", "--config_file", "c.yaml", "--save_history", "--train_similarity"]
    plain = vars(M.get_parser().parse_args(old))
    assert plain.pop("predict_links") is None and plain.pop("link_sources") is None
    with_flags = vars(M.get_parser().parse_args(old + ["--predict_links", "7", "--link_sources", "s.txt"]))
    assert with_flags.pop("predict_links") == 7 and with_flags.pop("link_sources") == Path("s.txt")
    assert with_flags == plain                          # every other flag parses as before
    assert set(plain) == {"command", "data_root", "output_root", "config_file", "save_history", "num_workers", "init_Z",
                          "exchange", "train_similarity", "gpu"}


def test_predict_links_is_refused_on_several_gpus_before_any_work(monkeypatch, tmp_path):
    import clane_amd.__main__ as M
    monkeypatch.setenv("WORLD_SIZE", "2")

    def touched(*a, **k):
        raise AssertionError("the run went on to set up devices")
    monkeypatch.setattr(M, "_distributed_setup", touched)
    args = M.get_parser().parse_args(["--data_root", str(tmp_path), "--output_root", str(tmp_path / "o"),
                                      "--config_file", str(tmp_path / "missing.yaml"), "--predict_links", "3"])
    with pytest.raises(NotImplementedError, match="one GPU"):
        M.embedding(args)
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(ValueError, match="--predict_links"):           # sources without the flag they restrict
        M.embedding(M.get_parser().parse_args(["--config_file", str(tmp_path / "missing.yaml"), "--link_sources", "s"]))


def test_links_tsv_format(tmp_path):
    vertex_ids = ["a", "b", "c", "d"]
    ids = torch.tensor([[2, 1, -1], [0, -1, -1], [-1, -1, -1]])
    scores = torch.tensor([[0.5, 1.0 / 3.0, float("-inf")], [-2.0 ** -22, float("-inf"), float("-inf")],
                           [float("-inf")] * 3], dtype=torch.float32)
    n = write_links_tsv(tmp_path / "links.tsv", vertex_ids, None, ids, scores)
    text = (tmp_path / "links.tsv").read_text()
    assert n == 3 and text == "a\tc\t0.5\na\tb\t%.9g\nb\ta\t%.9g\n" % (float(scores[0, 1]), float(scores[1, 0]))
    assert "0.333333343" in text                                       # %.9g of the fp32 value: it round-trips
    n = write_links_tsv(tmp_path / "some.tsv", vertex_ids, [3, 1, 0], ids, scores)
    assert (tmp_path / "some.tsv").read_text().split("\n")[:3] == ["d\tc\t0.5", "d\tb\t0.333333343", "b\ta\t-2.38418579e-07"]
    (tmp_path / "src.txt").write_text("c\n\na\n")
    assert read_link_sources(tmp_path / "src.txt", vertex_ids + ["a"]) == [2, 0]       # first occurrence, file order
    (tmp_path / "bad.txt").write_text("c\nzz\n")
    with pytest.raises(ValueError, match="'zz'"):
        read_link_sources(tmp_path / "bad.txt", vertex_ids)


def test_new_symbols_are_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "clane_hip.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _hip.SIGNATURES, name
    assert "#define CLANE_RANK_MAX_K 32" in header and _hip.RANK_MAX_K == 32
    assert re.search(r"#define CLANE_ABI_VERSION 5\b", header) and _hip.ABI_VERSION == 5


def test_argument_validation_reaches_last_error():
    # refused on the host before any launch: safe without a GPU
    lib = _hip.load_library()
    p = C.cast((C.c_float * 64)(), C.c_void_p)

    def rank(d=8, lds=8, ldn=8, mode=2, sums2=None, sq=None, rp=None, ci=None, k=5, n_slabs=1, S=p, Q=2):
        return lib.clane_rank_scores_f32(S, lds, p, ldn, 4, d, p, Q, mode, sums2, sq, None, rp, ci, 1, k, n_slabs, p, p, None)

    for bad, text in ((dict(k=0), b"k must be"), (dict(k=33), b"k must be"), (dict(n_slabs=0), b"n_slabs"),
                      (dict(d=0), b"bad shape"), (dict(lds=7), b"bad shape"), (dict(mode=9), b"unknown mode"),
                      (dict(mode=0), b"needs sums2"), (dict(mode=1), b"needs sq"), (dict(rp=p), b"excl_rowptr and excl_colidx"),
                      (dict(ci=p), b"excl_rowptr and excl_colidx"), (dict(S=None), b"null pointer")):
        assert rank(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"rank_scores" in lib.clane_last_error()
    assert rank(Q=0, S=None) == 0                                      # no queries: nothing to do
    assert lib.clane_rank_scores_bf16(p, 8, p, 8, 4, 8, p, 2, 2, None, None, None, None, None, 0, 40, 1, p, p, None) == -1
    assert lib.clane_rank_scores_f64(p, 8, p, 8, 4, 8, p, 2, 2, None, None, None, None, None, 0, 4, -1, p, p, None) == -1

    assert lib.clane_rank_merge_f32(p, p, 2, 1, 0, p, p, None) == -1 and b"rank_merge: k must be" in lib.clane_last_error()
    assert lib.clane_rank_merge_f64(p, p, 2, 0, 4, p, p, None) == -1 and b"n_slabs" in lib.clane_last_error()
    assert lib.clane_rank_merge_f32(p, None, 2, 1, 4, p, p, None) == -1 and b"null pointer" in lib.clane_last_error()
    assert lib.clane_rank_merge_f32(None, None, 0, 1, 4, None, None, None) == 0

    def pair(fn=lib.clane_pair_score_f32, d=8, lds=8, mode=2, sums2=None, sq=None, out=p, B=2):
        return fn(p, lds, p, 8, 4, d, p, p, B, mode, sums2, sq, out, None)

    for bad, text in ((dict(d=0), b"bad shape"), (dict(lds=3), b"bad shape"), (dict(mode=5), b"unknown mode"),
                      (dict(mode=0), b"needs sums2"), (dict(mode=1), b"needs sq"), (dict(out=None), b"null pointer"),
                      (dict(B=-1), b"bad shape")):
        assert pair(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"pair_score" in lib.clane_last_error()
    assert pair(B=0, out=None) == 0
    assert pair(fn=lib.clane_pair_score_bf16, mode=1) == -1 and pair(fn=lib.clane_pair_score_f64, d=-2) == -1


def test_backend_without_link_calls_says_so():
    from .oracle_kernels import OracleKernels
    kern = OracleKernels()
    for call in (lambda: kern.rank_scores(None, None, 0, 1, None, 2, None, None, None, None, None, True, 1, 1, None, None),
                 lambda: kern.rank_merge(None, None, 1, 1, None, None),
                 lambda: kern.pair_score(None, None, 0, 1, None, None, 2, None, None, None)):
        with pytest.raises(NotImplementedError, match="OracleKernels has no"):
            call()


def test_slab_rule():
    """ceil(Q / tile) * n_slabs covers 4 workgroups per CU (256 CUs) while the table has the tiles for it."""
    assert plan.rank_slabs(128, 2_000_000) == 1024                     # one query tile: 1024 slabs of ~15 tiles
    assert plan.rank_slabs(4096, 2_000_000) == 32                      # 32 query tiles x 32 slabs
    assert plan.rank_slabs(4096, 2_000_000, query_tile=64) == 16       # fp64: 64 queries per workgroup
    assert plan.rank_slabs(128, 200_000) == 1024 and plan.rank_slabs(129, 200_000) == 512
    assert plan.rank_slabs(34, 34) == 1 and plan.rank_slabs(7, 300) == 3           # never more slabs than candidate tiles
    assert plan.rank_slabs(1_000_000, 2_000_000) == 1 and plan.rank_slabs(0, 0) == 1
    for Q, rows in ((1, 1), (128, 129), (500, 70_000), (4096, 200_000)):
        n = plan.rank_slabs(Q, rows)
        tiles = -(-rows // plan.RANK_CANDIDATE_TILE)
        assert 1 <= n <= max(1, tiles)
        assert n == tiles or -(-Q // plan.RANK_QUERY_TILE) * n >= plan.RANK_WORKGROUPS_PER_CU * plan.COMPUTE_UNITS


def test_refusals_of_the_ranker():
    import numpy as np
    from clane_amd.engine import SweepEngine
    from clane_amd.links import LinkRanker
    from clane_amd.partition import HostCSR
    from clane_amd.similarity import AsymmertricSimilarity, CosineSimilarity
    from .oracle_kernels import OracleKernels
    csr = HostCSR(6, np.array([0, 1, 2, 3, 4, 5, 6], dtype=np.int64), np.array([1, 2, 3, 4, 5, 0], dtype=np.int32))
    eng = SweepEngine(csr, torch.zeros(6, 4), "cpu", OracleKernels())
    with pytest.raises(NotImplementedError, match="CosineSimilarity and AsymmertricSimilarity"):
        LinkRanker(eng, lambda a, b: a)
    with pytest.raises(ValueError, match="n_dim=3"):
        LinkRanker(eng, AsymmertricSimilarity(3))
    ranker = LinkRanker(eng, CosineSimilarity())
    assert ranker.label.tolist()[:0] == [] and sorted(v for v in ranker.label.tolist() if v >= 0) == list(range(6))
    with pytest.raises(ValueError, match="k must be"):
        ranker.top_k(0)
    with pytest.raises(NotImplementedError, match="OracleKernels has no rank_scores"):
        ranker.top_k(2)
    eng.world = 2                                                       # what a rank of a 2-GPU run would see
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        LinkRanker(eng, CosineSimilarity())
