"""Link prediction on the card (csrc/link_rank.h, clane_amd/links.py): the fused score + top-k kernel and its merge
exactly on integer data (every dot below 2^24: exact in every accumulate type, so ids AND scores must be equal),
independent of the slab count on float data, against fp64 with the project's elementwise bound in the three score modes,
the pair scores likewise, and the surface (LinkRanker, Graph.predict_links, the CLI) on the karate golden."""
import itertools

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


def _random_csr(rows, gen, density=0.15, with_self=True):
    """A CSR over table rows with sorted, unique rows; about every third row holds itself."""
    m = torch.rand(rows, rows, generator=gen) < density
    idx = torch.arange(rows)
    m[idx, idx] = (idx % 3 == 0) if with_self else False
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


def _eligible(q_rows, label, excl, exclude_self):
    """[Q, rows] bool on the CPU: may candidate v be returned for query i."""
    rows = label.numel()
    ok = (label >= 0)[None, :].expand(q_rows.numel(), rows).clone()
    if excl is not None:
        ok &= ~excl[q_rows.long()]
    if exclude_self:
        ok[torch.arange(q_rows.numel()), q_rows.long()] = False
    return ok


def _rank(k, dev, S, N, rows, d, q_rows, mode, sums2, sq, label, rowptr, colidx, exclude_self, topk, n_slabs):
    acc = _hip.acc_dtype(S.dtype)
    Q = q_rows.numel()
    cs = torch.full((Q * n_slabs * topk,), 7.0, dtype=acc, device=dev)
    ci = torch.full((Q * n_slabs * topk,), 7, dtype=torch.int32, device=dev)
    out_s = torch.full((Q, topk), 7.0, dtype=acc, device=dev)
    out_i = torch.full((Q, topk), 7, dtype=torch.int32, device=dev)
    k.rank_scores(S, N, rows, d, q_rows, mode, sums2, sq, label, rowptr, colidx, exclude_self, topk, n_slabs, cs, ci)
    k.rank_merge(cs, ci, n_slabs, topk, out_s, out_i)
    return out_i, out_s


# ---- (a) exact: integer data -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 5, 16, 130])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rank_is_exact_on_integer_data(dev, k, dtype, d):
    """Entries in [-3, 3]: |dot| <= 9 * 130 < 2^24, exact in f32 (and bf16 holds the entries exactly), so out_id and
    out_score must EQUAL int64 torch's mask + stable sort by (-score, label), the -1 / -inf tail included.  Rows are
    duplicated so every query has ties; labels are a permutation with holes; the exclusion CSR holds some queries
    themselves; table_rows crosses a tile edge (129) and leaves a partial tile (300); n_slabs = 7 is more than the small
    tables have tiles."""
    acc = _hip.acc_dtype(dtype)
    gen = torch.Generator().manual_seed(1000 + d)
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
        label_d, rowptr_d, colidx_d = label.to(dev), rowptr.to(dev), colidx.to(dev)
        for Q in (1, 7, 130):
            q_rows = torch.randint(0, rows, (Q,), generator=gen, dtype=torch.int32)
            if Q >= 7:                        # a repeated and an out-of-order query row
                q_rows[1], q_rows[2], q_rows[3] = q_rows[0], rows - 1, 0
            score = Si[q_rows.long()] @ Ni.T                                    # int64, exact
            for exclude_self in (False, True):
                ok = _eligible(q_rows, label, excl, exclude_self)
                key = torch.where(ok, -score * 1024 + label.long()[None, :], torch.full_like(score, 1 << 40))
                order = torch.sort(key, dim=1, stable=True).indices             # (-score, label): labels are unique
                for topk, n_slabs in itertools.product((1, 5, 32), (1, 3, 7)):
                    take = order[:, :topk]
                    if take.shape[1] < topk:
                        take = torch.cat([take, take[:, :1].expand(Q, topk - take.shape[1])], 1)
                    valid = torch.gather(ok, 1, take) & (torch.arange(topk)[None, :] < ok.sum(1, keepdim=True))
                    want_i = torch.where(valid, label.long()[take], torch.full_like(take, -1)).to(torch.int32)
                    want_s = torch.where(valid, torch.gather(score, 1, take).double(),
                                         torch.full(take.shape, NEG_INF, dtype=torch.float64)).to(acc)
                    got_i, got_s = _rank(k, dev, S, N, rows, d, q_rows.to(dev), _hip.SCORE_RAW_DOT, None, None, label_d,
                                         rowptr_d, colidx_d, exclude_self, topk, n_slabs)
                    where = f"rows={rows} Q={Q} k={topk} n_slabs={n_slabs} exclude_self={exclude_self}"
                    assert torch.equal(got_i.cpu(), want_i), where
                    assert torch.equal(got_s.cpu(), want_s), where
                    if rows == 1 and exclude_self:
                        assert bool((got_i == -1).all()) and bool((got_s == NEG_INF).all())


def test_rank_without_label_and_exclusion_reports_rows(dev, k):
    """label = NULL reports the table row itself; excl_* = NULL skips nothing."""
    gen = torch.Generator().manual_seed(5)
    rows, d, Q, topk = 200, 7, 9, 4
    Ni = torch.randint(-3, 4, (rows, d), generator=gen)
    N = _padded(Ni, torch.float32, dev)
    q_rows = torch.randint(0, rows, (Q,), generator=gen, dtype=torch.int32)
    score = Ni[q_rows.long()] @ Ni.T
    key = -score * 1024 + torch.arange(rows)[None, :]
    take = torch.sort(key, dim=1, stable=True).indices[:, :topk]
    got_i, got_s = _rank(k, dev, N, N, rows, d, q_rows.to(dev), _hip.SCORE_RAW_DOT, None, None, None, None, None, False,
                         topk, 2)
    assert torch.equal(got_i.cpu().long(), take)
    assert torch.equal(got_s.cpu(), torch.gather(score, 1, take).float())


# ---- (b) independent of the launch shape -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rank_does_not_depend_on_the_slab_count(dev, k, dtype):
    gen = torch.Generator().manual_seed(21)
    rows, d, Q, topk = 1000, 130, 200, 10
    Z = _padded(torch.randn(rows, d, generator=gen, dtype=torch.float64), dtype, dev)
    q_rows = torch.randint(0, rows, (Q,), generator=gen, dtype=torch.int32).to(dev)
    sq = (Z[:, :d].double() ** 2).sum(1).to(_hip.acc_dtype(dtype))
    _, rowptr, colidx = _random_csr(rows, gen, density=0.02)
    args = (k, dev, Z, Z, rows, d, q_rows, _hip.SCORE_PER_EDGE, None, sq, None, rowptr.to(dev), colidx.to(dev), True, topk)
    first = _rank(*args, 1)
    assert bool((first[0] >= 0).all())
    for n_slabs in (1, 2, 8):
        again = _rank(*args, n_slabs)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]), n_slabs


# ---- (c) against fp64 --------------------------------------------------------------------------------------------
def _scale64(mode, sq64, sums2, rows_a, rows_b):
    """fp64 factor of score = dot * scale for [len(rows_a), len(rows_b)] pairs of table rows (0 for a zero norm)."""
    if mode == _hip.SCORE_RAW_DOT:
        return torch.ones(len(rows_a), len(rows_b), dtype=torch.float64)
    if mode == _hip.SCORE_REFERENCE:
        return torch.full((len(rows_a), len(rows_b)), 1.0 / float(torch.sqrt(sums2[0] * sums2[1])), dtype=torch.float64)
    den = torch.sqrt(sq64[rows_a])[:, None] * torch.sqrt(sq64[rows_b])[None, :]
    return torch.where(den > 0, 1.0 / den.clamp_min(1e-300), torch.zeros_like(den))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [5, 128, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rank_against_fp64(dev, k, dtype, d, mode):
    """With s64 the fp64 score of the stored inputs: |score - s64| <= 2 d eps (|S_q| . |N_v|) * scale, the bound of a
    k-ordered chain of d products in the accumulate type (as test_project_rows_against_fp64), plus 8 eps |s64| for the
    square roots, the reciprocal and the two multiplies of the scaled modes.  Checked: order, eligibility, uniqueness,
    every returned score, and optimality -- no eligible candidate left out beats the k-th returned by more than the two
    bounds involved."""
    acc = _hip.acc_dtype(dtype)
    eps = EPS[acc]
    gen = torch.Generator().manual_seed(300 + d)
    rows, Q, topk = 2000, 130, 10
    Sv = torch.randn(rows, d, generator=gen, dtype=torch.float64).to(dtype)
    Nv = torch.randn(rows, d, generator=gen, dtype=torch.float64).to(dtype)
    Nv[17] = 0                                                        # a zero row: PER_EDGE scores it 0
    S, N = _padded(Sv, dtype, dev), _padded(Nv, dtype, dev)
    S64, N64 = Sv.double(), Nv.double()
    sq = (N64 ** 2).sum(1).to(acc)                                    # an input like any other: taken as stored
    sq64 = sq.double()
    sums2 = torch.tensor([float(sq64.sum()) * 3.0, float(sq64.sum()) * 0.7], dtype=torch.float64)
    label = _labels(rows, gen)
    excl, rowptr, colidx = _random_csr(rows, gen, density=0.03)
    q_rows = torch.randint(0, rows, (Q,), generator=gen, dtype=torch.int32)
    q_rows[1], q_rows[2] = q_rows[0], 17
    got_i, got_s = _rank(k, dev, S, N, rows, d, q_rows.to(dev), mode, sums2.to(dev), sq.to(dev), label.to(dev),
                         rowptr.to(dev), colidx.to(dev), True, topk, 5)
    got_i, got_s = got_i.cpu().long(), got_s.cpu().double()

    ql = q_rows.long()
    scale = _scale64(mode, sq64, sums2, ql, torch.arange(rows))
    s64 = (S64[ql] @ N64.T) * scale
    bound = 2 * d * eps * (S64[ql].abs() @ N64.abs().T) * scale
    if mode != _hip.SCORE_RAW_DOT:
        bound = bound + 8 * eps * s64.abs()
    ok = _eligible(q_rows, label, excl, True)
    row_of_label = torch.full((rows,), -1, dtype=torch.int64)
    row_of_label[label[label >= 0].long()] = torch.nonzero(label >= 0)[:, 0]
    assert bool((ok.sum(1) >= topk).all()) and bool((got_i >= 0).all())
    v = row_of_label[got_i]                                           # [Q, k] table rows returned
    assert bool((v >= 0).all())
    # order: non-increasing scores, labels ascending among bitwise-equal scores
    assert bool((got_s[:, 1:] <= got_s[:, :-1]).all())
    tie = got_s[:, 1:] == got_s[:, :-1]
    assert bool((got_i[:, 1:][tie] > got_i[:, :-1][tie]).all())
    # eligibility and uniqueness
    assert bool(torch.gather(ok, 1, v).all())
    assert all(len(set(r)) == topk for r in got_i.tolist())
    # every returned score
    err = (got_s - torch.gather(s64, 1, v)).abs()
    lim = torch.gather(bound, 1, v)
    assert bool((err <= lim).all()), float((err / lim.clamp_min(1e-300)).max())
    # optimality
    returned = torch.zeros_like(ok)
    returned.scatter_(1, v, True)
    kth = v[:, -1:]
    slack = torch.gather(s64, 1, kth) + torch.gather(bound, 1, kth) + bound
    left = ok & ~returned
    assert bool((s64[left] <= slack[left]).all())
    if mode == _hip.SCORE_PER_EDGE:                                  # the zero row scores exactly 0 wherever it shows
        assert bool((got_s[v == 17] == 0).all())


# ---- (d) pair scores ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_score_against_fp64(dev, k, dtype, mode):
    """The bound of (c) for explicit pairs (a butterfly of d products: the same 2 d eps form), on the one-element-per-lane
    path (odd leading dimension) and the 16-byte path; an index outside the table reads as a zero row, a zero-norm row
    scores 0 in PER_EDGE; two calls give the same bits."""
    acc = _hip.acc_dtype(dtype)
    eps = EPS[acc]
    gen = torch.Generator().manual_seed(77)
    rows = 500
    for d, pad in ((5, 3), (130, 3), (128, 0), (40, 8)):
        Sv = torch.randn(rows, d, generator=gen, dtype=torch.float64).to(dtype)
        Nv = torch.randn(rows, d, generator=gen, dtype=torch.float64).to(dtype)
        Nv[3] = 0
        S, N = _padded(Sv, dtype, dev, pad), _padded(Nv, dtype, dev, pad)
        S64, N64 = Sv.double(), Nv.double()
        S64z, N64z = torch.cat([S64, torch.zeros(1, d, dtype=torch.float64)]), torch.cat([N64, torch.zeros(1, d, dtype=torch.float64)])
        sq = torch.cat([(S64 ** 2).sum(1)[:250], (N64 ** 2).sum(1)[250:]]).to(acc)
        sq[3] = 0
        sq64z = torch.cat([sq.double(), torch.zeros(1, dtype=torch.float64)])
        sums2 = torch.tensor([float(sq.double().sum()), 11.0], dtype=torch.float64)
        for B in (1, 4, 1000, 100_003):
            src = torch.randint(0, rows, (B,), generator=gen, dtype=torch.int32)
            dst = torch.randint(0, rows, (B,), generator=gen, dtype=torch.int32)
            if B >= 4:
                src[0], dst[1], src[2], dst[2], dst[3] = -1, rows, rows + 5, -7, 3
            out = torch.full((B,), 7.0, dtype=acc, device=dev)
            k.pair_score(S, N, rows, d, src.to(dev), dst.to(dev), mode, sums2.to(dev), sq.to(dev), out)
            out2 = torch.full((B,), 9.0, dtype=acc, device=dev)
            k.pair_score(S, N, rows, d, src.to(dev), dst.to(dev), mode, sums2.to(dev), sq.to(dev), out2)
            assert torch.equal(out, out2)
            s, t = src.long(), dst.long()
            s[(s < 0) | (s >= rows)] = rows                           # the appended zero row
            t[(t < 0) | (t >= rows)] = rows
            a, b = S64z[s], N64z[t]
            if mode == _hip.SCORE_RAW_DOT:
                scale = torch.ones(B, dtype=torch.float64)
            elif mode == _hip.SCORE_REFERENCE:
                scale = torch.full((B,), 1.0 / float(torch.sqrt(sums2[0] * sums2[1])), dtype=torch.float64)
            else:
                den = torch.sqrt(sq64z[s]) * torch.sqrt(sq64z[t])
                scale = torch.where(den > 0, 1.0 / den.clamp_min(1e-300), torch.zeros_like(den))
            s64 = (a * b).sum(1) * scale
            bound = 2 * d * eps * (a.abs() * b.abs()).sum(1) * scale
            if mode != _hip.SCORE_RAW_DOT:
                bound = bound + 8 * eps * s64.abs()
            err = (out.cpu().double() - s64).abs()
            assert bool((err <= bound).all()), (d, B, float((err - bound).max()))
            if B >= 4:
                assert bool((out[:3] == 0).all())                     # out-of-range indices: zero rows
                if mode == _hip.SCORE_PER_EDGE:
                    assert float(out[3]) == 0.0                       # a zero-norm row


# ---- (e) through the surface: karate ------------------------------------------------------------------------------
def _karate_graph(tmp_path, d=16, seed=5):
    kc = load_golden("g2_karate_csr.npz")
    X = np.random.default_rng(seed).standard_normal((34, d)).astype(np.float32)
    root = write_data_root(tmp_path / "karate_links", kc["vertex_ids"], kc["edge_src"], kc["edge_dst"], X)
    g = Graph(root, embedding_dim=d)
    adj = torch.zeros(34, 34, dtype=torch.bool)
    adj[torch.from_numpy(np.repeat(np.arange(34), g.csr.outdeg())), torch.from_numpy(g.csr.colidx.astype(np.int64))] = True
    return g, adj


def _check_surface(ids, scores, s64, bound, ok, topk):
    """The properties of (c) for host results in vertex numbering (label = vertex index)."""
    scores = scores.double()
    assert ids.dtype == torch.int64 and tuple(ids.shape) == tuple(scores.shape) == (s64.shape[0], topk)
    assert bool((ids >= 0).all()) and bool((ok.sum(1) >= topk).all())
    assert bool((scores[:, 1:] <= scores[:, :-1]).all())
    tie = scores[:, 1:] == scores[:, :-1]
    assert bool((ids[:, 1:][tie] > ids[:, :-1][tie]).all())
    assert bool(torch.gather(ok, 1, ids).all())
    assert all(len(set(r)) == topk for r in ids.tolist())
    assert bool(((scores - torch.gather(s64, 1, ids)).abs() <= torch.gather(bound, 1, ids)).all())
    returned = torch.zeros_like(ok)
    returned.scatter_(1, ids, True)
    kth = ids[:, -1:]
    slack = torch.gather(s64, 1, kth) + torch.gather(bound, 1, kth) + bound
    left = ok & ~returned
    assert bool((s64[left] <= slack[left]).all())


@pytest.mark.parametrize("mode", ["reference", "per_edge"])
def test_predict_links_cosine_on_karate(tmp_path, dev, mode):
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
    # the norms the kernel divides by are themselves fp32 sums of d squares (K0), the sums of 34 of them in double:
    # (d + 2) eps relative on each of the two factors under the root -- on top of the bound of (c)
    bound = (2 * d * eps * (Z.abs() @ Z.abs().T) * scale + 8 * eps * s64.abs() + (d + 2) * eps * s64.abs())
    eye = torch.eye(34, dtype=torch.bool)
    ids, scores = g.predict_links(sim, k=5)
    assert not ids.is_cuda and not scores.is_cuda
    _check_surface(ids, scores, s64, bound, ~adj & ~eye, 5)
    assert not bool(torch.gather(adj | eye, 1, ids).any())           # no existing edge, no self pair
    ids_all, scores_all = g.predict_links(sim, k=5, exclude_existing=False)
    _check_surface(ids_all, scores_all, s64, bound, ~eye, 5)
    assert bool(torch.gather(adj, 1, ids_all).any())                 # ... and with them allowed, some edge ranks
    some, _ = g.predict_links(sim, k=5, sources=[33, 0, 33])
    assert torch.equal(some, ids[[33, 0, 33]])


def test_predict_links_bilinear_on_karate(tmp_path, dev):
    g, adj = _karate_graph(tmp_path)
    torch.manual_seed(4)
    sim = AsymmertricSimilarity(16)
    Embedder(g, sim, dev, tolerence=3, verbose=False).iterate()
    Z = g.Z.double()
    sim64 = AsymmertricSimilarity(16).double()
    sim64.load_state_dict({n: p.double() for n, p in sim.state_dict().items()})
    with torch.no_grad():
        s64 = sim64(Z[:, None, :].expand(34, 34, 16), Z[None, :, :].expand(34, 34, 16))     # forward on all pairs
        A64, B64 = sim64.Phi_src(Z), sim64.Phi_dst(Z)
        Aabs = Z.abs() @ sim64.Phi_src.weight.abs().T
        Babs = Z.abs() @ sim64.Phi_dst.weight.abs().T
    d, eps = 16, EPS[torch.float32]
    # two chained fp32 contractions: each projected entry carries 2 d eps |z| . |w|, the dot another 2 d eps
    bound = 2 * d * eps * (A64.abs() @ B64.abs().T) + 2 * d * eps * (Aabs @ B64.abs().T + A64.abs() @ Babs.T) * (1 + 2 * d * eps)
    eye = torch.eye(34, dtype=torch.bool)
    ids, scores = g.predict_links(sim, k=5)
    _check_surface(ids, scores, s64, bound, ~adj & ~eye, 5)
    assert not bool(torch.gather(adj | eye, 1, ids).any())
    ids_all, _ = g.predict_links(sim, k=5, exclude_existing=False)
    assert bool(torch.gather(adj, 1, ids_all).any())
    # explicit pairs
    gen = torch.Generator().manual_seed(9)
    src, dst = torch.randint(0, 34, (100,), generator=gen), torch.randint(0, 34, (100,), generator=gen)
    ranker = LinkRanker(g.engine(), sim)
    got = ranker.score_pairs(src, dst)
    assert got.is_cuda and bool(((got.cpu().double() - s64[src, dst]).abs() <= bound[src, dst]).all())
    prob = ranker.probabilities(src, dst).cpu().double()
    assert bool(((prob - torch.sigmoid(s64[src, dst])).abs() <= bound[src, dst] + 4 * eps).all())
    with pytest.raises(NotImplementedError, match="CosineSimilarity and AsymmertricSimilarity"):
        g.predict_links(lambda a, b: (a * b).sum(-1))
    with pytest.raises(ValueError, match="k must be"):
        g.predict_links(sim, k=33)


def test_pair_scores_cosine_on_karate(tmp_path, dev):
    g, _ = _karate_graph(tmp_path)
    sim = CosineSimilarity(mode="per_edge")
    Embedder(g, sim, dev, tolerence=3, verbose=False).iterate()
    Z = g.Z.double()
    gen = torch.Generator().manual_seed(10)
    src, dst = torch.randint(0, 34, (100,), generator=gen), torch.randint(0, 34, (100,), generator=gen)
    got = LinkRanker(g.engine(cosine_mode="per_edge"), sim).score_pairs(src, dst).cpu().double()
    want = torch.nn.functional.cosine_similarity(Z[src], Z[dst], dim=1)
    assert bool(((got - want).abs() <= (2 * 16 + 8 + 18) * EPS[torch.float32]).all())


# ---- (f) CLI ----------------------------------------------------------------------------------------------------------
def test_cli_writes_links_tsv(tmp_path, karate_root):
    from clane_amd.__main__ import embedding, get_parser
    kc = load_golden("g2_karate_csr.npz")
    np.save(karate_root / "C.npy", np.random.default_rng(3).standard_normal((34, 8)).astype(np.float32))
    cfg = tmp_path / "config.yaml"
    cfg.write_text("graph:\n  embedding_dim: 8\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
                   "embedder:\n  gamma: 0.76\n  tolerence: 3\n")
    common = ["--data_root", str(karate_root), "--config_file", str(cfg), "--gpu"]
    embedding(get_parser().parse_args(common + ["--output_root", str(tmp_path / "plain")]))
    assert not (tmp_path / "plain" / "links.tsv").exists()
    embedding(get_parser().parse_args(common + ["--output_root", str(tmp_path / "links"), "--predict_links", "3"]))
    assert np.array_equal(np.load(tmp_path / "plain" / "Z.npy"), np.load(tmp_path / "links" / "Z.npy"))
    ids = [str(v) for v in kc["vertex_ids"]]
    edges = set(zip((str(s) for s in kc["edge_src"]), (str(t) for t in kc["edge_dst"])))
    lines = (tmp_path / "links" / "links.tsv").read_text().splitlines()
    assert len(lines) == 34 * 3
    rows = [l.split("\t") for l in lines]
    assert all(len(r) == 3 for r in rows)
    assert [r[0] for r in rows] == [v for v in ids for _ in range(3)]            # sources in vertex order
    assert all(r[1] in ids and r[0] != r[1] and (r[0], r[1]) not in edges for r in rows)
    scores = [float(r[2]) for r in rows]
    assert all(r[2] == "%.9g" % s for r, s in zip(rows, scores))
    assert all(scores[i] >= scores[i + 1] for i in range(len(rows) - 1) if rows[i][0] == rows[i + 1][0])
    pick = tmp_path / "sources.txt"
    pick.write_text(f"{ids[20]}\n{ids[4]}\n")
    embedding(get_parser().parse_args(common + ["--output_root", str(tmp_path / "two"), "--predict_links", "3",
                                               "--link_sources", str(pick)]))
    two = [l.split("\t") for l in (tmp_path / "two" / "links.tsv").read_text().splitlines()]
    assert [r[0] for r in two] == [ids[20]] * 3 + [ids[4]] * 3
    assert two == rows[60:63] + rows[12:15]
    pick.write_text(f"{ids[1]}\nno-such-vertex\n")
    with pytest.raises(ValueError, match="no-such-vertex"):
        embedding(get_parser().parse_args(common + ["--output_root", str(tmp_path / "bad"), "--predict_links", "3",
                                                   "--link_sources", str(pick)]))
