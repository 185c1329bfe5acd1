"""Held-out link evaluation on the card (csrc/link_eval.h, clane_amd/links.py): the counting kernel exactly on integer
data (every dot below 2^24, so the four counts and the target's score must EQUAL int64 torch's masks and sums),
independent of the slab count on float data, the identity with top_k's order (1 + greater + equal_lower is the target's
place in the list, its score the list's, bit for bit), brackets against fp64 with the project's elementwise bound, and
the surface (LinkRanker.rank_pairs / evaluate, Graph.evaluate_links, the CLI's link_evaluation section) on the karate
golden."""
import functools
import itertools
import json

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.embedder import Embedder
from clane_amd.graph import Graph
from clane_amd.links import LinkRanker
from clane_amd.similarity import AsymmertricSimilarity, CosineSimilarity

from .conftest import load_golden, write_data_root

pytestmark = pytest.mark.gpu

EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}      # unit roundoff of the accumulate type
DTYPES = [torch.float32, torch.bfloat16, torch.float64]
MODES = [_hip.SCORE_RAW_DOT, _hip.SCORE_PER_EDGE, _hip.SCORE_REFERENCE]
NEG_INF = float("-inf")
TOPK = 32


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


def _padded(values, dtype, dev, pad=3):
    """[rows, d + pad] device table holding ``values`` (a CPU tensor) in its first d columns."""
    buf = torch.zeros(values.shape[0], values.shape[1] + pad, dtype=dtype, device=dev)
    buf[:, :values.shape[1]] = values.to(dtype).to(dev)
    return buf


def _random_csr(rows, gen, density=0.15):
    """A CSR over table rows with sorted, unique rows; about every third row holds itself."""
    m = torch.rand(rows, rows, generator=gen) < density
    idx = torch.arange(rows)
    m[idx, idx] = idx % 3 == 0
    rowptr = torch.zeros(rows + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(m.sum(1), 0)
    colidx = m.nonzero()[:, 1].to(torch.int32)
    if colidx.numel() == 0:
        colidx = torch.zeros(1, dtype=torch.int32)
    return m, rowptr, colidx


def _labels(rows, gen):
    """A random permutation as labels, about one row in seven not a candidate (-1)."""
    lab = torch.randperm(rows, generator=gen).to(torch.int32)
    if rows > 1:
        lab[torch.rand(rows, generator=gen) < 1 / 7] = -1
    return lab


def _in_table(q, t, rows, label):
    """bool [B]: the pair has a rank (both rows inside the table, the target a candidate row)."""
    inside = (q >= 0) & (q < rows) & (t >= 0) & (t < rows)
    if label is not None:
        inside &= label[t.clamp(0, rows - 1).long()] >= 0
    return inside


def _eligible(q, t, rows, label, excl, exclude_self):
    """[B, rows] bool on the CPU: is candidate v counted for pair i (pairs without a rank: whatever)."""
    B = q.numel()
    qc, tc = q.clamp(0, rows - 1).long(), t.clamp(0, rows - 1).long()
    ok = torch.ones(B, rows, dtype=torch.bool) if label is None else (label >= 0)[None, :].expand(B, rows).clone()
    if excl is not None:
        ok &= ~excl[qc]
    if exclude_self:
        ok[torch.arange(B), qc] = False
    ok[torch.arange(B), tc] = False                                   # the target never is a candidate
    return ok


def _count(k, dev, S, N, rows, d, q, t, mode, sums2, sq, label, rowptr, colidx, exclude_self, n_slabs):
    """(counts int64 [B, 4] summed over the slabs, target_score [B]) as the caller of the ABI forms them."""
    acc = _hip.acc_dtype(S.dtype)
    B = q.numel()
    ts = torch.full((B,), 7.0, dtype=acc, device=dev)
    per_slab = torch.full((B, n_slabs, 4), 7, dtype=torch.int32, device=dev)
    k.rank_count(S, N, rows, d, q, t, mode, sums2, sq, label, rowptr, colidx, exclude_self, n_slabs, ts, per_slab)
    none = per_slab[:, 0, 0] < 0
    assert bool((per_slab[none] == -1).all())                         # no rank: -1 in all four counts of EVERY slab
    assert bool((per_slab[~none] >= 0).all())
    total = per_slab.sum(1, dtype=torch.int64)
    total[none] = -1
    return total, ts


# ---- (a) exact: integer data -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 5, 16, 130])
@pytest.mark.parametrize("dtype", DTYPES)
def test_count_is_exact_on_integer_data(dev, k, dtype, d):
    """Entries in [-3, 3]: |dot| <= 9 * 130 < 2^24, exact in f32 (and bf16 holds the entries exactly), so the slab-summed
    counts and target_score must EQUAL int64 torch's.  Candidate rows are duplicated (the targets' rows among them), so
    ties fall on both sides of a target's label; the pairs hold a repeated pair, target == query, a target inside the
    query's exclusion row (still ranked), a target with label -1 and an index outside the table (no rank); table_rows
    crosses a tile edge (129) and leaves a partial tile (300); n_slabs = 7 is more than the small tables have tiles."""
    acc = _hip.acc_dtype(dtype)
    gen = torch.Generator().manual_seed(2000 + d)
    for rows in (1, 129, 300):
        Si = torch.randint(-3, 4, (rows, d), generator=gen)
        Ni = torch.randint(-3, 4, (rows, d), generator=gen)
        if rows > 1:                          # duplicated candidate rows: equal scores under different labels
            dup = torch.randint(0, rows, (rows // 3,), generator=gen)
            Ni[dup] = Ni[torch.randint(0, rows, (rows // 3,), generator=gen)]
            Ni[rows - 1] = Ni[0]
        S, N = _padded(Si, dtype, dev), _padded(Ni, dtype, dev)
        label = _labels(rows, gen)
        excl, rowptr, colidx = _random_csr(rows, gen)
        for B in (1, 7, 130):
            q = torch.randint(0, rows, (B,), generator=gen, dtype=torch.int32)
            t = torch.randint(0, rows, (B,), generator=gen, dtype=torch.int32)
            if B >= 7 and rows > 1:
                q[1], t[1] = q[0], t[0]                               # a repeated pair
                t[2] = q[2]                                           # target == query
                edge = excl.nonzero()[int(torch.randint(0, int(excl.sum()), (1,), generator=gen))]
                q[3], t[3] = int(edge[0]), int(edge[1])               # a target inside the query's exclusion row
                holes = (label < 0).nonzero()[:, 0]
                if holes.numel():
                    t[4] = int(holes[0])                              # a target with label -1 (when labels are given)
                t[5] = rows                                           # outside the table
                q[6] = -1
            if B == 130:
                t[64:] = t[7]                                         # many pairs on one target: its duplicates tie
            qc, tc = q.clamp(0, rows - 1).long(), t.clamp(0, rows - 1).long()
            score = Si[qc] @ Ni.T                                     # int64, exact
            tscore = score[torch.arange(B), tc]
            q_d, t_d = q.to(dev), t.to(dev)
            for with_label, with_csr, exclude_self in itertools.product((True, False), (True, False), (True, False)):
                lab = label if with_label else None
                ranked = _in_table(q, t, rows, lab)
                ok = _eligible(q, t, rows, lab, excl if with_csr else None, exclude_self)
                key = (label if with_label else torch.arange(rows, dtype=torch.int32)).long()
                gt = ok & (score > tscore[:, None])
                eq = ok & (score == tscore[:, None])
                lower = key[None, :] < key[tc][:, None]
                want = torch.stack([gt.sum(1), (eq & lower).sum(1), (eq & ~lower).sum(1), ok.sum(1)], 1)
                want[~ranked] = -1
                want_s = torch.where(ranked, tscore.double(), torch.full((B,), NEG_INF, dtype=torch.float64)).to(acc)
                for n_slabs in (1, 3, 7):
                    got, got_s = _count(k, dev, S, N, rows, d, q_d, t_d, _hip.SCORE_RAW_DOT, None, None,
                                        lab.to(dev) if with_label else None, rowptr.to(dev) if with_csr else None,
                                        colidx.to(dev) if with_csr else None, exclude_self, n_slabs)
                    where = (f"rows={rows} B={B} n_slabs={n_slabs} label={with_label} csr={with_csr} "
                             f"exclude_self={exclude_self}")
                    assert torch.equal(got.cpu(), want), where
                    assert torch.equal(got_s.cpu(), want_s), where
            if B >= 7 and rows > 1:                                   # what the special pairs are there for
                assert not bool(_in_table(q, t, rows, None)[5:7].any()) and bool(_in_table(q, t, rows, None)[:5].all())
                assert bool(excl[q[3].long(), t[3].long()])


# ---- (b) independent of the launch shape -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_count_does_not_depend_on_the_slab_count(dev, k, dtype):
    gen = torch.Generator().manual_seed(22)
    rows, d, B = 1000, 130, 200
    Z = _padded(torch.randn(rows, d, generator=gen, dtype=torch.float64), dtype, dev)
    q = torch.randint(0, rows, (B,), generator=gen, dtype=torch.int32).to(dev)
    t = torch.randint(0, rows, (B,), generator=gen, dtype=torch.int32).to(dev)
    sq = (Z[:, :d].double() ** 2).sum(1).to(_hip.acc_dtype(dtype))
    _, rowptr, colidx = _random_csr(rows, gen, density=0.02)
    args = (k, dev, Z, Z, rows, d, q, t, _hip.SCORE_PER_EDGE, None, sq, None, rowptr.to(dev), colidx.to(dev), True)
    first = _count(*args, 1)
    assert bool((first[0] >= 0).all()) and bool((first[0][:, 0] > 0).any())
    for n_slabs in (1, 2, 8):
        again = _count(*args, n_slabs)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]), n_slabs


# ---- (c), (d): float data, shared case -----------------------------------------------------------------------------
def _scale64(mode, sq64, sums2, rows_a, rows_b):
    """fp64 factor of score = dot * scale for [len(rows_a), len(rows_b)] pairs of table rows (0 for a zero norm)."""
    if mode == _hip.SCORE_RAW_DOT:
        return torch.ones(len(rows_a), len(rows_b), dtype=torch.float64)
    if mode == _hip.SCORE_REFERENCE:
        return torch.full((len(rows_a), len(rows_b)), 1.0 / float(torch.sqrt(sums2[0] * sums2[1])), dtype=torch.float64)
    den = torch.sqrt(sq64[rows_a])[:, None] * torch.sqrt(sq64[rows_b])[None, :]
    return torch.where(den > 0, 1.0 / den.clamp_min(1e-300), torch.zeros_like(den))


@functools.lru_cache(maxsize=2)
def _float_case(dtype, d, mode):
    """The inputs of test_rank_against_fp64 (2000 rows, 130 queries, labels with holes, an exclusion CSR, a zero row),
    built once for (c) and (d) and left unchanged: CPU tensors, the fp64 scores and their elementwise bound."""
    acc = _hip.acc_dtype(dtype)
    eps = EPS[acc]
    gen = torch.Generator().manual_seed(300 + d)
    rows, Q = 2000, 130
    Sv = torch.randn(rows, d, generator=gen, dtype=torch.float64).to(dtype)
    Nv = torch.randn(rows, d, generator=gen, dtype=torch.float64).to(dtype)
    Nv[17] = 0                                                        # a zero row: PER_EDGE scores it 0
    S64, N64 = Sv.double(), Nv.double()
    sq = (N64 ** 2).sum(1).to(acc)                                    # an input like any other: taken as stored
    sq64 = sq.double()
    sums2 = torch.tensor([float(sq64.sum()) * 3.0, float(sq64.sum()) * 0.7], dtype=torch.float64)
    label = torch.randperm(rows, generator=gen).to(torch.int32)      # a permutation with holes; row 17 stays a candidate
    holes = torch.rand(rows, generator=gen) < 1 / 7
    holes[17] = False
    label[holes] = -1
    excl, rowptr, colidx = _random_csr(rows, gen, density=0.03)
    q_rows = torch.randint(0, rows, (Q,), generator=gen, dtype=torch.int32)
    q_rows[1], q_rows[2] = q_rows[0], 17
    ql = q_rows.long()
    scale = _scale64(mode, sq64, sums2, ql, torch.arange(rows))
    s64 = (S64[ql] @ N64.T) * scale
    bound = 2 * d * eps * (S64[ql].abs() @ N64.abs().T) * scale
    if mode != _hip.SCORE_RAW_DOT:
        bound = bound + 8 * eps * s64.abs()
    ok = (label >= 0)[None, :].expand(Q, rows).clone() & ~excl[ql]
    ok[torch.arange(Q), ql] = False                                   # eligible for the QUERY (exclude_self on)
    return dict(rows=rows, Q=Q, d=d, mode=mode, Sv=Sv, Nv=Nv, sq=sq, sums2=sums2, label=label, rowptr=rowptr,
                colidx=colidx, q_rows=q_rows, s64=s64, bound=bound, ok=ok, gen_seed=900 + d)


def _random_eligible(ok, n, gen):
    """[Q, n] table rows, each eligible for its query, drawn uniformly."""
    return torch.multinomial(ok.double(), n, replacement=False, generator=gen)


def _on_device(c, dtype, dev):
    return dict(S=_padded(c["Sv"], dtype, dev), N=_padded(c["Nv"], dtype, dev), sq=c["sq"].to(dev),
                sums2=c["sums2"].to(dev), label=c["label"].to(dev), rowptr=c["rowptr"].to(dev), colidx=c["colidx"].to(dev))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [5, 128, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_count_places_the_target_where_top_k_does(dev, k, dtype, d, mode):
    """The identity the feature rests on.  rank_scores + rank_merge with k = 32 for 130 queries; targets: per query the
    entries at places 1, 7 and 32 of its own list, and three random eligible rows.  A target at place p of the list:
    1 + greater + equal_lower == p and target_score has the bits of the list's score at p.  A target not in the list:
    greater + equal_lower >= 32.  Every pair is checked."""
    c = _float_case(dtype, d, mode)
    acc = _hip.acc_dtype(dtype)
    rows, Q = c["rows"], c["Q"]
    D = _on_device(c, dtype, dev)
    n_slabs = 5
    cs = torch.empty(Q * n_slabs * TOPK, dtype=acc, device=dev)
    ci = torch.empty(Q * n_slabs * TOPK, dtype=torch.int32, device=dev)
    top_s = torch.empty(Q, TOPK, dtype=acc, device=dev)
    top_i = torch.empty(Q, TOPK, dtype=torch.int32, device=dev)
    q_d = c["q_rows"].to(dev)
    k.rank_scores(D["S"], D["N"], rows, d, q_d, mode, D["sums2"], D["sq"], D["label"], D["rowptr"], D["colidx"], True,
                  TOPK, n_slabs, cs, ci)
    k.rank_merge(cs, ci, n_slabs, TOPK, top_s, top_i)
    top_i, top_s = top_i.cpu().long(), top_s.cpu()
    assert bool((top_i >= 0).all())                                   # 32 eligible candidates everywhere
    row_of_label = torch.full((rows,), -1, dtype=torch.int64)
    row_of_label[c["label"][c["label"] >= 0].long()] = torch.nonzero(c["label"] >= 0)[:, 0]
    top_rows = row_of_label[top_i]                                    # [Q, 32] table rows
    picked = top_rows[:, [0, 6, 31]]
    extra = _random_eligible(c["ok"], 3, torch.Generator().manual_seed(c["gen_seed"]))
    targets = torch.cat([picked, extra], 1)                           # [Q, 6]
    q = c["q_rows"][:, None].expand(Q, 6).reshape(-1).contiguous()
    t = targets.reshape(-1).to(torch.int32)
    got, got_s = _count(k, dev, D["S"], D["N"], rows, d, q.to(dev), t.to(dev), mode, D["sums2"], D["sq"], D["label"],
                        D["rowptr"], D["colidx"], True, 3)
    got, got_s = got.cpu().reshape(Q, 6, 4), got_s.cpu().reshape(Q, 6)
    assert bool((got >= 0).all())
    before = got[:, :, 0] + got[:, :, 1]
    hit = top_rows[:, None, :] == targets[:, :, None]                 # [Q, 6, 32]
    in_list = hit.any(2)
    place = hit.double().argmax(2) + 1
    assert bool(in_list[:, :3].all()) and bool((place[:, :3] == torch.tensor([1, 7, 32])).all())
    assert bool((1 + before == place)[in_list].all())
    list_score = torch.gather(top_s, 1, place - 1)
    bits = torch.int64 if acc == torch.float64 else torch.int32
    assert torch.equal(got_s[in_list].view(bits), list_score[in_list].view(bits))
    assert bool((before >= TOPK)[~in_list].all())
    assert in_list.numel() == Q * 6 and int(in_list.sum()) + int((~in_list).sum()) == Q * 6      # no pair left out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [5, 128, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_count_against_fp64(dev, k, dtype, d, mode):
    """With s64 the fp64 score of the stored inputs and b the elementwise bound of test_rank_against_fp64
    (2 d eps |S| . |N| scale, plus 8 eps |s64| in the scaled modes), for every pair (q, t):
    #{eligible w : s64_w - b_w > s64_t + b_t} <= greater, greater + equal <= #{eligible w : s64_w + b_w >= s64_t - b_t},
    eligible equals the mask's count exactly, |target_score - s64_t| <= b_t; the zero row scores exactly 0 as a target
    in PER_EDGE."""
    c = _float_case(dtype, d, mode)
    rows, Q = c["rows"], c["Q"]
    D = _on_device(c, dtype, dev)
    per = 4
    targets = _random_eligible(c["ok"], per, torch.Generator().manual_seed(c["gen_seed"] + 1))
    targets[3:, per - 1] = 17                                         # the zero row as a target (a candidate row: label >= 0)
    assert int(c["label"][17]) >= 0
    q = c["q_rows"][:, None].expand(Q, per).reshape(-1).contiguous()
    t = targets.reshape(-1).to(torch.int32)
    got, got_s = _count(k, dev, D["S"], D["N"], rows, d, q.to(dev), t.to(dev), mode, D["sums2"], D["sq"], D["label"],
                        D["rowptr"], D["colidx"], True, 5)
    got, got_s = got.cpu().reshape(Q, per, 4), got_s.cpu().double().reshape(Q, per)
    s64, b = c["s64"], c["bound"]
    st, bt = torch.gather(s64, 1, targets), torch.gather(b, 1, targets)          # [Q, per]
    ok = c["ok"][:, None, :].expand(Q, per, rows).clone()
    ok.scatter_(2, targets[:, :, None], False)                        # the target never is a candidate
    low = (ok & ((s64 - b)[:, None, :] > (st + bt)[:, :, None])).sum(2)
    high = (ok & ((s64 + b)[:, None, :] >= (st - bt)[:, :, None])).sum(2)
    greater, equal, eligible = got[:, :, 0], got[:, :, 1] + got[:, :, 2], got[:, :, 3]
    assert bool((got >= 0).all())
    assert bool((low <= greater).all()), int((low - greater).max())
    assert bool((greater + equal <= high).all()), int((greater + equal - high).max())
    assert torch.equal(eligible, ok.sum(2))
    assert bool(((got_s - st).abs() <= bt).all()), float(((got_s - st).abs() - bt).max())
    if mode == _hip.SCORE_PER_EDGE:
        assert bool((got_s[targets == 17] == 0).all())


# ---- (e) through the surface: karate ------------------------------------------------------------------------------
def _karate_graph(tmp_path, d=16, seed=5):
    kc = load_golden("g2_karate_csr.npz")
    X = np.random.default_rng(seed).standard_normal((34, d)).astype(np.float32)
    root = write_data_root(tmp_path / "karate_eval", kc["vertex_ids"], kc["edge_src"], kc["edge_dst"], X)
    g = Graph(root, embedding_dim=d)
    adj = torch.zeros(34, 34, dtype=torch.bool)
    adj[torch.from_numpy(np.repeat(np.arange(34), g.csr.outdeg())), torch.from_numpy(g.csr.colidx.astype(np.int64))] = True
    return g, adj


def _karate_pairs(adj):
    """The 78 edges of the golden in both directions (78 x 2 directed pairs, each ranked against the non-edges of its
    source) and 100 random pairs."""
    edges = adj.nonzero()
    assert edges.shape[0] == 78
    gen = torch.Generator().manual_seed(12)
    src = torch.cat([edges[:, 0], edges[:, 1], torch.randint(0, 34, (100,), generator=gen)])
    dst = torch.cat([edges[:, 1], edges[:, 0], torch.randint(0, 34, (100,), generator=gen)])
    return src, dst


def _host_metrics(greater, lower, higher, eligible, hits):
    """The issue's formulas, on the host in plain Python floats."""
    rows = [(g, lo + hi, e) for g, lo, hi, e in zip(greater.tolist(), lower.tolist(), higher.tolist(), eligible.tolist())
            if g >= 0]
    rank = [1 + g + eq / 2 for g, eq, _ in rows]
    auc = [(e - g - eq / 2) / e for g, eq, e in rows if e > 0]
    return {"pairs": len(rows), "skipped": len(greater) - len(rows), "mrr": sum(1 / r for r in rank) / len(rank),
            "mean_rank": sum(rank) / len(rank), "hits": {str(K): sum(r <= K for r in rank) / len(rank) for K in hits},
            "auc": sum(auc) / len(auc)}


def _check_karate(g, sim, eng, adj, s64, bound):
    src, dst = _karate_pairs(adj)
    B = src.numel()
    ranker = LinkRanker(eng, sim)
    greater, lower, higher, eligible, score = ranker.rank_pairs(src, dst)
    assert all(x.is_cuda and x.dtype == torch.int64 for x in (greater, lower, higher, eligible)) and score.is_cuda
    greater, lower, higher, eligible, score = (x.cpu() for x in (greater, lower, higher, eligible, score))
    assert bool((greater >= 0).all())
    # the fp64 brackets of test_count_against_fp64
    ok = (~adj & ~torch.eye(34, dtype=torch.bool))[src].clone()
    ok[torch.arange(B), dst] = False
    st, bt = s64[src, dst], bound[src, dst]
    low = (ok & ((s64 - bound)[src] > (st + bt)[:, None])).sum(1)
    high = (ok & ((s64 + bound)[src] >= (st - bt)[:, None])).sum(1)
    assert bool((low <= greater).all()) and bool((greater + lower + higher <= high).all())
    assert torch.equal(eligible, ok.sum(1))
    assert bool(((score.double() - st).abs() <= bt).all())
    # unfiltered: the existing out-neighbours are candidates too
    _, _, _, eligible_all, score_all = ranker.rank_pairs(src, dst, filter_existing=False, batch=100, refresh=False)
    ok_all = (~torch.eye(34, dtype=torch.bool))[src].clone()
    ok_all[torch.arange(B), dst] = False
    assert torch.equal(eligible_all.cpu(), ok_all.sum(1)) and torch.equal(score_all.cpu(), score)
    # the metrics: Graph.evaluate_links against the same formulas on the host
    hits = (1, 3, 10)
    got = g.evaluate_links(sim, src, dst, hits=hits)
    want = _host_metrics(greater, lower, higher, eligible, hits)
    assert got["pairs"] == want["pairs"] == B and got["skipped"] == want["skipped"] == 0
    assert set(got["hits"]) == {"1", "3", "10"}
    for name in ("mrr", "mean_rank", "auc"):
        assert abs(got[name] - want[name]) <= 1e-12, name
    for K in got["hits"]:
        assert abs(got["hits"][K] - want["hits"][K]) <= 1e-12
    assert ranker.evaluate(src, dst, hits).as_dict() == got
    # consistent with predict_links: a non-edge target sits at place 1 + greater + equal_lower of its source's list, an
    # edge target (absent from the list) would be inserted behind exactly greater + equal_lower of its entries
    ids, scores = g.predict_links(sim, k=TOPK)
    for i in range(B):
        u, v = int(src[i]), int(dst[i])
        row_ids, row_s = ids[u].tolist(), scores[u].tolist()
        ts = float(score[i])
        ahead = sum(1 for w, s in zip(row_ids, row_s) if w >= 0 and w != v and (s > ts or (s == ts and w < v)))
        assert ahead == int(greater[i] + lower[i]), (u, v)
        if v in row_ids:
            p = row_ids.index(v)
            assert p == ahead and row_s[p] == ts
        else:                                                         # an edge, a self pair, or behind a full list
            assert bool(adj[u, v]) or u == v or ahead >= TOPK


@pytest.mark.parametrize("mode", ["reference", "per_edge"])
def test_evaluate_links_cosine_on_karate(tmp_path, dev, mode):
    g, adj = _karate_graph(tmp_path)
    sim = CosineSimilarity(mode=mode)
    Embedder(g, sim, dev, tolerence=3, verbose=False).iterate()
    Z = g.Z.double()
    d, eps = Z.shape[1], EPS[torch.float32]
    sq = (Z ** 2).sum(1)
    if mode == "per_edge":
        scale = 1.0 / (torch.sqrt(sq)[:, None] * torch.sqrt(sq)[None, :])
    else:
        outdeg = torch.from_numpy(g.csr.outdeg().astype(np.float64))
        indeg = torch.from_numpy(g.csr.indeg().astype(np.float64))
        scale = torch.full((34, 34), 1.0 / float(torch.sqrt((outdeg * sq).sum() * (indeg * sq).sum())), dtype=torch.float64)
    s64 = (Z @ Z.T) * scale
    # the bound of test_predict_links_cosine_on_karate
    bound = (2 * d * eps * (Z.abs() @ Z.abs().T) * scale + 8 * eps * s64.abs() + (d + 2) * eps * s64.abs())
    _check_karate(g, sim, g.engine(cosine_mode=mode), adj, s64, bound)


def test_evaluate_links_bilinear_on_karate(tmp_path, dev):
    g, adj = _karate_graph(tmp_path)
    torch.manual_seed(4)
    sim = AsymmertricSimilarity(16)
    Embedder(g, sim, dev, tolerence=3, verbose=False).iterate()
    Z = g.Z.double()
    sim64 = AsymmertricSimilarity(16).double()
    sim64.load_state_dict({n: p.double() for n, p in sim.state_dict().items()})
    with torch.no_grad():
        s64 = sim64(Z[:, None, :].expand(34, 34, 16), Z[None, :, :].expand(34, 34, 16))
        A64, B64 = sim64.Phi_src(Z), sim64.Phi_dst(Z)
        Aabs = Z.abs() @ sim64.Phi_src.weight.abs().T
        Babs = Z.abs() @ sim64.Phi_dst.weight.abs().T
    d, eps = 16, EPS[torch.float32]
    # the bound of test_predict_links_bilinear_on_karate
    bound = 2 * d * eps * (A64.abs() @ B64.abs().T) + 2 * d * eps * (Aabs @ B64.abs().T + A64.abs() @ Babs.T) * (1 + 2 * d * eps)
    _check_karate(g, sim, g.engine(), adj, s64, bound)
    with pytest.raises(NotImplementedError, match="evaluate_links scores with CosineSimilarity and AsymmertricSimilarity"):
        g.evaluate_links(lambda a, b: (a * b).sum(-1), [0], [1])
    with pytest.raises(ValueError, match="one entry per pair"):
        LinkRanker(g.engine(), sim).rank_pairs([0, 1], [2])


# ---- (f) CLI ----------------------------------------------------------------------------------------------------------
def test_cli_writes_link_metrics(tmp_path, karate_root):
    from clane_amd.__main__ import embedding, get_parser
    kc = load_golden("g2_karate_csr.npz")
    np.save(karate_root / "C.npy", np.random.default_rng(3).standard_normal((34, 8)).astype(np.float32))
    base = ("graph:\n  embedding_dim: 8\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
            "embedder:\n  gamma: 0.76\n  tolerence: 3\n")
    ids = [str(v) for v in kc["vertex_ids"]]
    lines = [f"{ids[3]}\t{ids[9]}", f"{ids[0]}\t{ids[33]}", f"{ids[20]}\t{ids[4]}", f"{ids[5]}\t{ids[5]}", f"{ids[33]}\t{ids[0]}"]
    (karate_root / "held_out.tsv").write_text("\n".join(lines) + "\n")
    plain, with_eval = tmp_path / "plain.yaml", tmp_path / "eval.yaml"
    plain.write_text(base)
    with_eval.write_text(base + "\nlink_evaluation:\n  pairs: held_out.tsv\n  hits: [1, 5]\n  filter_existing: false\n")

    def run(cfg, out):
        embedding(get_parser().parse_args(["--data_root", str(karate_root), "--config_file", str(cfg), "--gpu",
                                           "--output_root", str(tmp_path / out)]))
    run(plain, "plain")
    assert not (tmp_path / "plain" / "link_metrics.json").exists()
    run(with_eval, "eval")
    assert (tmp_path / "plain" / "Z.npy").read_bytes() == (tmp_path / "eval" / "Z.npy").read_bytes()
    got = json.loads((tmp_path / "eval" / "link_metrics.json").read_text())
    assert set(got) == {"pairs", "skipped", "mrr", "mean_rank", "hits", "auc", "similarity", "filtered"}
    assert got["pairs"] + got["skipped"] == len(lines) and got["pairs"] == len(lines)
    assert set(got["hits"]) == {"1", "5"} and got["similarity"] == "CosineSimilarity" and got["filtered"] is False
    assert 0.0 < got["mrr"] <= 1.0 and 1.0 <= got["mean_rank"] <= 33.0 and 0.0 <= got["auc"] <= 1.0
    assert got["hits"]["1"] <= got["hits"]["5"]
    # the defaults: hits 1, 3, 10 and the filtered setting, from an absolute path
    with_eval.write_text(base + f"\nlink_evaluation:\n  pairs: {karate_root / 'held_out.tsv'}\n")
    run(with_eval, "defaults")
    got = json.loads((tmp_path / "defaults" / "link_metrics.json").read_text())
    assert set(got["hits"]) == {"1", "3", "10"} and got["filtered"] is True and got["pairs"] == len(lines)
    (karate_root / "held_out.tsv").write_text(f"{ids[1]}\t{ids[2]}\n{ids[1]}\tno-such-vertex\n")
    with pytest.raises(ValueError, match="no-such-vertex"):
        run(with_eval, "bad")
