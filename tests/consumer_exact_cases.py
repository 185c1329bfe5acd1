"""Exact link, probe and k-means results through the Python layer that turns VERTEX numbering into TABLE-ROW numbering,
under every launch plan of tests/engine_exact_cases.py -- helpers of tests/test_gpu_consumer_exact.py (the HIP kernels)
and tests/test_consumer_exact_host.py (the same checks through the CPU test double, plus mutation self-checks).

engine_exact_cases pins the sweeps of every plan to the bit; what READS the engine's tables -- ``LinkRanker`` (links.py),
``sorted_adjacency`` / ``PairSampler`` / ``rows_of_vertices`` (train.py), ``project_table`` (bilinear.py) and
``table_and_rows`` (classify.py: LabelProbe and KMeans) -- had only ever met the default plan of a toy graph: one block,
no padding rows, no class rows, no rotated tables.  Here every one of them runs on the engines ``make_engine`` builds
for ``PLAN_RUNS`` (three blocks with 702 table rows for 700 vertices, shuffled layouts, class rows in (class, column)
edge order, column tiles, contiguous tables) and on the split graph, each plan's route assertion kept.

A. ``ConsumerCase``: Z has exactly q entries of +-1 per row, q the largest power of 4 <= d, so a row's norm^2 is q and
the per-edge factor 1 / sqrt(q) a power of two; one vertex with out-edges holds a zero row; every tenth vertex copies the
row of a vertex V / 2 + 3 further on (score ties whose order by vertex index is not the order of the table rows); W is
an integer matrix in {-1, 0, 1}, thinned until every partial sum of the projection (max |Z| |W|^T) and of a pair's dot
(max sum |A| |B| over the bounds of the projection) is below 2^24 -- asserted in the case builder -- so whatever order
a kernel adds in, fp32 accumulation included, every score is an exact integer (times a power of two per edge; times ONE
factor rounded once in the reference mode: the documented A(1 / sqrt(sums2[0] sums2[1])) formed in double from exact
integer sums reproduces bit for bit on the card, so that mode is held to torch.equal as well).  ``Reference`` restates every result in int64 / float64 torch in vertex
numbering only: it never sees ``pos`` or anything else of an engine.  Every comparison is torch.equal or ==.

B. ``check_current_table``: the table that is current.  Rankers made before any sweep, build_P, sweep, snapshot (the
third table), sweep, a launch taken back, the snapshot distance (which leaves norms behind), one more sweep (into the
third table, which only the launch taken back had written), set_Z with other data -- after each step every consumer result must be torch.equal to the same call on a FRESH engine of the same settings loaded with
``set_Z(eng.get_Z())``: the same layout, kernels and table bits, so a difference means the wrong table, stale norms or a
stale projection was read.

The consumers that merged later -- the silhouette, ContentPCA on a table, the k-NN search, t-SNE, LabelProbe.predict, the
Gaussian mixture and the kept label and mixture models -- live in tests/consumer_later_cases.py: A.8 holds them to a
LAYOUT-FREE result (a plain [V, d] tensor no engine made, rows = the vertex list itself) under the plans that change what
a consumer sees, and ``run_current_table`` compares them with the fresh engine after every step of B as well, through
objects and models made before any sweep and through new ones (on the HIP kernels: the CPU double has none of theirs).

Nothing here has a tolerance."""
import functools
import math

import numpy as np
import torch

from clane_amd import _hip, plan
from clane_amd import bilinear as bilinear_mod
from clane_amd import train as train_mod
from clane_amd.classify import LabelProbe, label_masks, make_splits, table_and_rows
from clane_amd.cluster import KMeans
from clane_amd.links import LinkRanker, link_metrics
from clane_amd.similarity import AsymmertricSimilarity, CosineSimilarity

from . import engine_exact_cases as X
from . import exact_cases as E
from .exact_cases import BF16, F32, F64

KS = (1, 10, 32)
MODES = ("bilinear", "per_edge", "reference")
SPLIT_RUNS = [(c, "defaults") for c in X.SPLIT_CASES]


def largest_power_of_4(d):
    q = 1
    while q * 4 <= d:
        q *= 4
    return q


# ---- A: the case ----------------------------------------------------------------------------------------------------------
class ConsumerCase:
    """Z, X, W of one (dtype, d) over graph(gname); host tensors in float64 holding integers, nobody writes to them.
    Asserted from the data: every |Z| |W_src|^T and |Z| |W_dst|^T entry (a bound on every partial sum of the projection
    and on |S|, |N|) and every pair's sum of those bounds' products (a bound on every partial sum of a bilinear dot) is
    below 2^24 = EXACT_LIMIT; a cosine dot's partial sums are within q <= 256."""
    FAR = 3                                                # a copy's source is V / 2 + FAR vertices further on

    def __init__(self, dtype, d, gname="ragged"):
        g = X.graph(gname)
        V = X.n_vertices(g)
        base = X.engine_case(dtype, d, gname)
        rng = np.random.default_rng(3500 + d)
        self.dtype, self.d, self.gname, self.acc = dtype, d, gname, _hip.acc_dtype(dtype)
        self.X, self.P = base.X, base.P                      # what make_engine wants besides Z0
        self.q = q = largest_power_of_4(d)
        Z = np.zeros((V, d), dtype=np.int64)
        cols = np.argsort(rng.random((V, d)), axis=1)[:, :q]
        np.put_along_axis(Z, cols, rng.choice(np.array([-1, 1]), size=(V, q)), axis=1)
        self.copies = np.arange(0, V, 10)
        self.copy_of = (self.copies + V // 2 + self.FAR) % V
        assert (self.copy_of % 10 != 0).all()               # no copy of a copy
        Z[self.copies] = Z[self.copy_of]
        self.zero_vertex = int(np.nonzero((g.deg > 0) & (np.arange(V) % 10 == 7))[0][0])    # neither a copy nor a source
        Z[self.zero_vertex] = 0
        assert ((Z != 0).sum(1) == np.where(np.arange(V) == self.zero_vertex, 0, q)).all()
        self.Z0 = torch.from_numpy(Z).double()
        keep = 1.0
        while True:
            W = rng.integers(-1, 2, size=(2 * d, d)) * (rng.random((2 * d, d)) < keep)
            absS = np.abs(Z).astype(np.float64) @ np.abs(W[:d]).T.astype(np.float64)
            absN = np.abs(Z).astype(np.float64) @ np.abs(W[d:]).T.astype(np.float64)
            self.project_bound = float(max(absS.max(), absN.max()))
            self.pair_bound = float((absS @ absN.T).max())
            if max(self.project_bound, self.pair_bound) < E.EXACT_LIMIT:
                break
            keep /= 2                                        # thin W
        assert self.project_bound < E.EXACT_LIMIT and self.pair_bound < E.EXACT_LIMIT and q <= 256 and (W != 0).any()
        self.W_density = keep
        self.W = torch.from_numpy(W).double()
        assert self.Z0.to(dtype).double().equal(self.Z0) and self.W.to(self.acc).double().equal(self.W)
        # queries: the full-row hubs (fewer than k eligible candidates), the zero row, copies and their sources, repeats
        hubs = np.argsort(g.deg, kind="stable")[-3:][::-1]
        some = rng.integers(0, V, 24)
        self.sources = torch.from_numpy(np.concatenate([hubs, [self.zero_vertex], self.copies[:3], self.copy_of[:3], some,
                                                        hubs[:1], some[:5]]).astype(np.int64))
        n = 260
        src = np.concatenate([rng.integers(0, V, n), np.repeat(hubs, 4), [self.zero_vertex] * 4])
        dst = np.concatenate([rng.integers(0, V, n), rng.integers(0, V, 12), rng.integers(0, V, 4)])
        edges = rng.integers(0, g.E, 40)                                        # pairs that are edges of the graph
        row_of_edge = np.repeat(np.arange(V), g.deg)
        src, dst = np.concatenate([src, row_of_edge[edges]]), np.concatenate([dst, g.sorted_colidx[edges].astype(np.int64)])
        ok = src != dst
        self.pair_src, self.pair_dst = torch.from_numpy(src[ok]), torch.from_numpy(dst[ok])
        assert int((~ok).sum()) < 10

    def similarity(self, mode):
        if mode != "bilinear":
            return CosineSimilarity(mode=mode)
        sim = AsymmertricSimilarity(self.d).to(torch.float64)
        with torch.no_grad():
            sim.Phi_src.weight.copy_(self.W[:self.d])
            sim.Phi_dst.weight.copy_(self.W[self.d:])
        return sim


@functools.lru_cache(maxsize=None)
def consumer_case(dtype, d, gname="ragged"):
    return ConsumerCase(dtype, d, gname)


class Reference:
    """Every expected result of a ConsumerCase in int64 / float64 torch, VERTEX numbering only."""

    def __init__(self, c):
        g = X.graph(c.gname)
        self.V = V = X.n_vertices(g)
        self.c, self.deg = c, torch.from_numpy(g.deg.astype(np.int64))
        self.row_of_edge = torch.from_numpy(np.repeat(np.arange(V), g.deg))
        self.col_of_edge = torch.from_numpy(g.sorted_colidx.astype(np.int64))
        self.adj = torch.zeros(V, V, dtype=torch.bool)
        self.adj[self.row_of_edge, self.col_of_edge] = True
        Zi, Wi, d = c.Z0.long(), c.W.long(), c.d
        self.S, self.N = Zi @ Wi[:d].T, Zi @ Wi[d:].T
        assert int(self.S.abs().max()) <= c.project_bound and int(self.N.abs().max()) <= c.project_bound
        dots = Zi @ Zi.T
        sq = (Zi * Zi).sum(1)
        assert bool(((sq == c.q) | (sq == 0)).all()) and int((sq == 0).sum()) == 1
        # per edge: 1 / sqrt(q) is a power of two (q a power of 4), 0 for the zero row -- the products are exact
        rn = torch.where(sq > 0, 1.0 / sq.double().sqrt(), torch.zeros(V, dtype=F64))
        assert bool((torch.frexp(rn[sq > 0])[0] == 0.5).all())
        # reference mode: the documented factor A(1 / sqrt(sums2[0] sums2[1])), sums2 = the out- / in-degree weighted
        # sums of the norms^2 (exact integers), formed in double and cast to A; then ONE multiply in A
        indeg = torch.bincount(self.col_of_edge, minlength=V)
        s0, s1 = int((self.deg * sq).sum()), int((indeg * sq).sum())
        assert 0 < s0 < 2 ** 53 and 0 < s1 < 2 ** 53
        self.sums2 = (s0, s1)
        factor = torch.tensor(1.0 / math.sqrt(float(s0) * float(s1)), dtype=F64).to(c.acc)
        self.scores = {"bilinear": (self.S @ self.N.T).double().to(c.acc),
                       "per_edge": (dots.double() * rn[:, None] * rn[None, :]).to(c.acc),
                       "reference": dots.double().to(c.acc) * factor}
        assert float(self.scores["bilinear"].abs().max()) <= c.pair_bound
        assert self.scores["per_edge"].double().equal(dots.double() * rn[:, None] * rn[None, :])
        self._orders = {}

    def eligible(self, exclude):
        out = ~torch.eye(self.V, dtype=torch.bool)
        return out & ~self.adj if exclude else out

    def order(self, mode, exclude):
        """(ids int64 [V, 32], scores [V, 32]) of every source: the mask (self, existing out-neighbours), a stable sort by
        (-score, vertex index), -1 / -inf beyond the eligible vertices."""
        key = (mode, bool(exclude))
        if key not in self._orders:
            sc, ok = self.scores[mode], self.eligible(exclude)
            inf = torch.full_like(sc, float("inf"))
            idx = torch.sort(torch.where(ok, -sc, inf), dim=1, stable=True).indices[:, :max(KS)]
            there = ok.gather(1, idx)
            self._orders[key] = (torch.where(there, idx, torch.full_like(idx, -1)),
                                 torch.where(there, sc.gather(1, idx), -inf.gather(1, idx)))
        return self._orders[key]

    def n_eligible(self, exclude):
        return self.eligible(exclude).sum(1)

    def counts(self, mode, src, dst, filtered):
        """(greater, equal_lower, equal_higher, eligible, score) by brute force over all vertices."""
        sc = self.scores[mode]
        rows, target = sc[src], sc[src, dst]
        v = torch.arange(self.V)[None, :]
        ok = (v != src[:, None]) & (v != dst[:, None])
        if filtered:
            ok &= ~self.adj[src]
        greater = (ok & (rows > target[:, None])).sum(1)
        same = ok & (rows == target[:, None])
        lower, higher = (same & (v < dst[:, None])).sum(1), (same & (v > dst[:, None])).sum(1)
        # V - 1 - excluded: the target, and in the filtered setting the source's out-neighbours other than itself / it
        excluded = torch.ones_like(src)
        if filtered:
            excluded = excluded + (self.adj[src] & (v != src[:, None]) & (v != dst[:, None])).sum(1)
        assert torch.equal(ok.sum(1), self.V - 1 - excluded)
        return greater, lower, higher, ok.sum(1), target


@functools.lru_cache(maxsize=3)
def reference(dtype, d, gname="ragged"):
    return Reference(consumer_case(dtype, d, gname))


# ---- hooks: where a mutation self-check reaches in ----------------------------------------------------------------------------
class Hooks:
    """What tests/test_consumer_exact_host.py overrides to make the project wrong in one named way."""

    def after_engine(self, eng):
        pass

    def after_ranker(self, ranker):
        pass

    def after_sweep(self, eng):
        pass


# ---- where a vertex sits: for messages ----------------------------------------------------------------------------------------
class Where:
    def __init__(self, eng, gname):
        self.g = X.graph(gname)
        self.pos = eng.pos.cpu()
        self.rows = int(eng.part.padded_vertices)
        self.inv = torch.full((self.rows,), -1, dtype=torch.int64)
        self.inv[self.pos] = torch.arange(eng.V)
        self.block = X.block_of_vertex(eng)

    def of(self, vertices, limit=6):
        """[(vertex, table row, degree, block)] of the first few of `vertices`."""
        vs = torch.as_tensor(vertices).reshape(-1).tolist()[:limit]
        return [(v, int(self.pos[v]), int(self.g.deg[v]), int(self.block[v])) for v in vs]


def _rows_that_differ(got, want):
    bad = got != want
    return (bad.reshape(bad.shape[0], -1).any(1)).nonzero().flatten()


# ---- A.1 - A.4 ------------------------------------------------------------------------------------------------------------------
def check_tables(checks, eng, c, w):
    V, d = eng.V, c.d
    everyone = torch.arange(V)
    repeats = torch.cat([c.sources, c.sources.flip(0)])
    for table, want in (("Z", c.Z0), ("X", c.X)):
        for what, vs in (("all", everyone), ("repeats", repeats)):
            T, rows = table_and_rows(eng, vs, table)
            got = T[rows.long(), :d].cpu().double()
            bad = _rows_that_differ(got, want[vs])
            checks.record(f"A1 table {table} {what}", bad.numel() == 0 and rows.dtype == torch.int32,
                          "(vertex, table row, degree, block)", w.of(vs[bad]))
        for bad_v in ([-1], [V], [0, V + 5]):
            try:
                table_and_rows(eng, bad_v, table)
                raised = False
            except ValueError:
                raised = True
            checks.record(f"A1 table {table} refuses {bad_v}", raised)
    rows = train_mod.rows_of_vertices(eng, repeats)
    checks.record("A1 rows_of_vertices", torch.equal(eng.Zcur[rows.long(), :d].cpu().double(), c.Z0[repeats]),
                  w.of(repeats))


def check_adjacency(checks, eng, c, w, ref):
    rowptr, colidx, R = train_mod.sorted_adjacency(eng)
    rowptr, colidx = rowptr.cpu(), colidx.cpu().long()
    n_edges = int(rowptr[-1])
    checks.record("A2 adjacency R", R == eng.part.padded_vertices and rowptr.numel() == R + 1 and n_edges == ref.row_of_edge.numel(),
                  R, eng.part.padded_vertices, n_edges)
    deg = rowptr[1:] - rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(R), deg)
    col = colidx[:n_edges]
    inside = bool(((col >= 0) & (col < R)).all())
    pads = (w.inv < 0).nonzero().flatten()
    checks.record("A2 adjacency padding rows are empty", bool((deg[pads] == 0).all()), pads.tolist())
    ok = False
    wrong = []
    if inside and bool((w.inv[row] >= 0).all()) and bool((w.inv[col] >= 0).all()):
        # as sets: (vertex, neighbour) of every edge, sorted, against the graph's own sorted rows
        got = torch.sort(w.inv[row] * eng.V + w.inv[col]).values
        want = ref.row_of_edge * eng.V + ref.col_of_edge
        ok = got.numel() == want.numel() and torch.equal(got, want)
        if not ok and got.numel() == want.numel():
            wrong = w.of(torch.unique(want[got != want] // eng.V))
    checks.record("A2 adjacency rows are the graph's", ok, "(vertex, table row, degree, block)", wrong)
    step = col[1:] - col[:-1]
    unsorted = torch.unique(row[1:][(row[1:] == row[:-1]) & (step <= 0)])
    checks.record("A2 adjacency rows strictly increasing", unsorted.numel() == 0, "(vertex, table row, degree, block)",
                  w.of(w.inv[unsorted].clamp(min=0)))


def check_sampler(checks, eng, c, w, ref):
    B = 64
    for fraction in (0.0, 1.0):
        gen = torch.Generator().manual_seed(5 + int(fraction))
        sampler = train_mod.PairSampler(eng, B, gen, positive_fraction=fraction)
        batches = list(sampler.epoch())
        src, dst, linked = (torch.cat([b[i] for b in batches]).cpu() for i in range(3))
        sv, dv = w.inv[src.long()], w.inv[dst.long()]
        real = bool((sv >= 0).all()) and bool((dv >= 0).all())
        checks.record(f"A3 sampler f={fraction:g} rows of real vertices", real and src.numel() == eng.V // B * B)
        if not real:
            continue
        want = ref.adj[sv, dv]
        bad = (linked.bool() != want).nonzero().flatten()
        checks.record(f"A3 sampler f={fraction:g} linked", bad.numel() == 0, "(vertex, table row, degree, block) of src",
                      w.of(sv[bad]))
        if fraction == 1.0:
            has = ref.deg[sv] > 0
            missed = (has & ~linked.bool()).nonzero().flatten()
            checks.record("A3 sampler f=1 every src with out-edges is linked", missed.numel() == 0 and bool(has.any()),
                          w.of(sv[missed]))


def check_projection(checks, eng, c, w, ref):
    S, N = bilinear_mod.project_table(eng, c.W)
    S, N = S.cpu().double(), N.cpu().double()
    for name, got, want in (("S", S, ref.S.double()), ("N", N, ref.N.double())):
        bad = _rows_that_differ(got[w.pos], want)
        checks.record(f"A4 projection {name}", bad.numel() == 0, "(vertex, table row, degree, block)", w.of(bad))
    pads = (w.inv < 0).nonzero().flatten()
    checks.record("A4 projection padding rows are zero", bool((S[pads] == 0).all()) and bool((N[pads] == 0).all()), pads.tolist())


# ---- A.5 / A.6 --------------------------------------------------------------------------------------------------------------------
def slab_batches(ranker, c, V):
    """(sources, batch) of ONE top_k call that takes several batches and at least two different n_slabs
    (plan.rank_slabs): on the 700-vertex graph the query list, repeated until a batch of it has more query tiles than a
    fifth of the 1024 workgroups the plan asks for, and a short remainder; on the 4300-vertex graph every vertex in
    batches of 4096."""
    if V > 4096:
        sources, batch, Q = None, 4096, V
    else:
        batch = ranker.query_tile * 205
        Q = batch + 7
        sources = c.sources.repeat(-(-Q // c.sources.numel()))[:Q]
    slabs = {plan.rank_slabs(min(batch, Q - a), ranker.rows, ranker.query_tile) for a in range(0, Q, batch)}
    assert len(slabs) >= 2 and Q > batch, (slabs, Q, batch)
    return sources, batch


def _judge_top(checks, name, w, srcs, got, want, k):
    (ids, scores), (wi, ws) = got, want
    ids, scores = ids.cpu(), scores.cpu()
    wi, ws = wi[srcs][:, :k], ws[srcs][:, :k]
    bad = _rows_that_differ(ids, wi)
    checks.record(f"{name} ids", bad.numel() == 0, "(source vertex, table row, degree, block)", w.of(srcs[bad]),
                  "got / want of the first", ids[bad[:1]].tolist(), wi[bad[:1]].tolist())
    bad = _rows_that_differ(scores, ws)
    checks.record(f"{name} scores", bad.numel() == 0 and scores.dtype == ws.dtype,
                  "(source vertex, table row, degree, block)", w.of(srcs[bad]))


def check_ranker(checks, eng, c, w, ref, mode, hooks):
    V = eng.V
    if mode != "bilinear":
        eng.set_cosine_mode(mode)
    ranker = LinkRanker(eng, c.similarity(mode))
    hooks.after_ranker(ranker)
    everyone = torch.arange(V)
    tag = f"A5 {mode}" if mode == "bilinear" else f"A6 {mode}"
    kept = {}
    for exclude in (True, False):
        want = ref.order(mode, exclude)
        ex = "excl=on" if exclude else "excl=off"
        short = (ref.n_eligible(exclude) < max(KS)).nonzero().flatten()         # the full-row hubs
        for k in KS:
            got = ranker.top_k(k, exclude_existing=exclude, batch=V // 3 + 67)  # 700 sources: batches of 300, 300, 100
            _judge_top(checks, f"{tag} top_k k={k} {ex} all", w, everyone, got, want, k)
            if k == max(KS):
                kept[exclude] = (got[0].cpu(), got[1].cpu())
                tails_ok = torch.equal(kept[exclude][0][short], want[0][short]) and \
                    torch.equal(kept[exclude][1][short], want[1][short])
                checks.record(f"{tag} tail of the short rows {ex}", tails_ok and (short.numel() > 0 or not exclude),
                              "(source vertex, table row, degree, block)", w.of(short))
            got = ranker.top_k(k, sources=c.sources, exclude_existing=exclude)
            _judge_top(checks, f"{tag} top_k k={k} {ex} listed", w, c.sources, got, want, k)
    sources, batch = slab_batches(ranker, c, V)
    got = ranker.top_k(10, sources=sources, batch=batch)
    _judge_top(checks, f"{tag} top_k k=10 excl=on several n_slabs", w, everyone if sources is None else sources, got,
               ref.order(mode, True), 10)

    src, dst = c.pair_src, c.pair_dst
    got = ranker.score_pairs(src, dst).cpu()
    bad = (got != ref.scores[mode][src, dst]).nonzero().flatten()
    checks.record(f"{tag} score_pairs", bad.numel() == 0, "(source vertex, table row, degree, block)", w.of(src[bad]))
    for filtered in (True, False):
        fl = "filter=on" if filtered else "filter=off"
        want = ref.counts(mode, src, dst, filtered)
        got = [t.cpu() for t in ranker.rank_pairs(src, dst, filter_existing=filtered, batch=150)]
        for name, g_, w_ in zip(("greater", "equal_lower", "equal_higher", "eligible", "score"), got, want):
            bad = (g_ != w_).nonzero().flatten()
            checks.record(f"{tag} rank_pairs {name} {fl}", bad.numel() == 0 and g_.dtype == w_.dtype,
                          "(source vertex, table row, degree, block)", w.of(src[bad]), "targets", w.of(dst[bad]),
                          "got / want", g_[bad[:4]].tolist(), w_[bad[:4]].tolist())
        metrics = ranker.evaluate(src, dst, hits=(1, 3, 10), filter_existing=filtered)
        on_dev = [t.to(eng.device) for t in want[:4]]                         # the arithmetic runs where the counts live
        checks.record(f"{tag} evaluate {fl}", metrics == link_metrics(*on_dev, hits=(1, 3, 10)), metrics)
    # a target inside the top 32 (the reference's): its place and its score are top_k's
    for exclude in (True, False):
        ids, scores = ref.order(mode, exclude)[0], kept[exclude][1]
        places = torch.tensor([0, 1, 9, 31])
        s_ = c.sources[(ids[c.sources][:, places] >= 0).all(1)]
        src2, dst2 = s_.repeat_interleave(places.numel()), ids[s_][:, places].reshape(-1)
        greater, lower, _, _, score = (t.cpu() for t in ranker.rank_pairs(src2, dst2, filter_existing=exclude))
        ex = "excl=on" if exclude else "excl=off"
        bad = (1 + greater + lower != places.repeat(s_.numel()) + 1).nonzero().flatten()
        checks.record(f"{tag} place in top_k {ex}", bad.numel() == 0 and s_.numel() > 0, w.of(src2[bad]), w.of(dst2[bad]))
        checks.record(f"{tag} rank_pairs score is top_k's {ex}", torch.equal(score, scores[s_][:, places].reshape(-1)))


def run_consumers(kernels, dev, case, settings, route, tag, gname="ragged", hooks=None):
    """One engine under one plan, the table loaded with set_Z: the `Checks` of A.1 - A.6."""
    hooks = hooks or Hooks()
    c, ref, checks = consumer_case(*case, gname), reference(*case, gname), X.Checks(tag)
    with X.device_ctx(dev):
        eng = X.make_engine(kernels, dev, c, **settings)
        route(eng, dev)
        hooks.after_engine(eng)
        w = Where(eng, gname)
        check_tables(checks, eng, c, w)
        check_adjacency(checks, eng, c, w, ref)
        check_sampler(checks, eng, c, w, ref)
        check_projection(checks, eng, c, w, ref)
        for mode in MODES:
            check_ranker(checks, eng, c, w, ref, mode, hooks)
    return checks


def check_plan(kernels, dev, case, plan_name):
    settings, route = X.PLANS[plan_name]
    run_consumers(kernels, dev, case, settings, route, X.plan_id((case, plan_name))).assert_none_failed()


def check_split(kernels, dev, case, plan_name):
    settings, route = X.SPLIT_PLANS[plan_name]
    run_consumers(kernels, dev, case, settings, route, f"split graph {X.case_id(case)}-{plan_name}",
                  gname="split").assert_none_failed()


# ---- A.7: plan independence on float data -----------------------------------------------------------------------------------
class FloatCase:
    """Random normal tables at (dtype, d) over graph(): what make_engine wants, and labels for the fits."""

    def __init__(self, dtype, d, seed=0):
        g = X.graph()
        V = X.n_vertices(g)
        gen = torch.Generator().manual_seed(7700 + d + seed)
        self.dtype, self.d, self.gname, self.acc = dtype, d, "ragged", _hip.acc_dtype(dtype)
        self.X = torch.randn(V, d, generator=gen, dtype=F64)
        self.Z0 = torch.randn(V, d, generator=gen, dtype=F64)
        self.Z1 = torch.randn(V, d, generator=gen, dtype=F64)            # "other data" of check B
        self.P = X.engine_case(dtype, d).P
        self.K, self.C = 7, 5
        self.y = torch.randint(0, self.C, (V,), generator=gen)
        sets = [sorted(set(torch.randint(0, self.C, (int(n),), generator=gen).tolist()))
                for n in torch.randint(1, 4, (V,), generator=gen)]
        self.masks = label_masks(sets, self.C)
        self.split, _ = make_splits(V, (0.5,), 3, seed=1)
        self.init = torch.randn(2, self.K, d, generator=gen, dtype=F64)
        self.W = torch.randn(2 * d, d, generator=gen, dtype=F64) / math.sqrt(d)


@functools.lru_cache(maxsize=None)
def float_case(dtype, d, seed=0):
    return FloatCase(dtype, d, seed)


def float_fits(kernels, dev, case, plan_name):
    """name -> CPU tensor: KMeans, LabelProbe.fit and fit_multilabel over all 700 vertices under one plan."""
    c = float_case(*case)
    settings, route = X.PLANS[plan_name]
    out = {}
    with X.device_ctx(dev):
        eng = X.make_engine(kernels, dev, c, **settings)
        route(eng, dev)
        Z, rows = table_and_rows(eng, torch.arange(eng.V))
        fit = KMeans(eng, max_iter=5).fit(Z, rows, c.K, restarts=3, seed=2)
        out.update({"kmeans assign": fit.assign, "kmeans centres": fit.centres, "kmeans inertia": fit.inertia})
        probe = LabelProbe(eng, max_iter=20)
        fit = probe.fit(Z, rows, c.y, c.split, c.C)
        out.update({"probe W": fit.W, "probe b": fit.b, "probe objective": fit.objective, "probe pred": fit.pred})
        fit = probe.fit_multilabel(Z, rows, c.masks, c.split, c.C)
        out.update({"multilabel W": fit.W, "multilabel b": fit.b, "multilabel objective": fit.objective,
                    "multilabel pred": fit.pred})
        return {name: t.detach().cpu().clone() for name, t in out.items()}


_baselines = {}


def check_plan_independence(kernels, dev, case, plan_name):
    key = (str(dev), case)
    if key not in _baselines:
        _baselines[key] = float_fits(kernels, dev, case, "defaults")
    base, checks = _baselines[key], X.Checks(f"A7 {X.plan_id((case, plan_name))}")
    for name, got in float_fits(kernels, dev, case, plan_name).items():
        checks.record(f"A7 {name}", torch.equal(got, base[name]),
                      "rows that differ", _rows_that_differ(got, base[name])[:8].tolist() if got.dim() else None)
    checks.assert_none_failed()


# ---- B: the table that is current ---------------------------------------------------------------------------------------------
CURRENT_RUNS = ([("sequence", p, m) for p in X.SEQUENCE_PLANS for m in ("reference", "per_edge")]
                + [(t, "chunks3_class", m) for t in ("f32", "bf16") for m in ("reference", "per_edge")])
STEPS = ("sweep 1", "snapshot + sweep 2", "a launch taken back", "the snapshot distance", "sweep 3", "set_Z")


def current_id(run):
    return "-".join(run)


def _bilinear(W):
    d = W.shape[1]
    sim = AsymmertricSimilarity(d).to(torch.float64)
    with torch.no_grad():
        sim.Phi_src.weight.copy_(W[:d])
        sim.Phi_dst.weight.copy_(W[d:])
    return sim


def _rankers(eng, W, hooks):
    out = {"cosine": LinkRanker(eng, CosineSimilarity(mode=eng.cosine_mode)), "bilinear": LinkRanker(eng, _bilinear(W))}
    for r in out.values():
        hooks.after_ranker(r)
    return out


def _ranker_results(ranker, sources, src, dst):
    out = {}
    out["top_k ids"], out["top_k scores"] = ranker.top_k(10, sources=sources, batch=17)
    out["top_k all ids"], out["top_k all scores"] = ranker.top_k(32, exclude_existing=False, batch=300)
    for name, t in zip(("greater", "equal_lower", "equal_higher", "eligible", "score"), ranker.rank_pairs(src, dst, batch=150)):
        out[f"rank_pairs {name}"] = t
    out["score_pairs"] = ranker.score_pairs(src, dst)
    return {k: v.cpu().clone() for k, v in out.items()}


def _other_results(eng, W, init, K):
    out = {}
    S, N = bilinear_mod.project_table(eng, W)
    out["project_table S"], out["project_table N"] = S[eng.pos].cpu().clone(), N[eng.pos].cpu().clone()
    T, rows = table_and_rows(eng, torch.arange(eng.V))
    out["table_and_rows"] = T[rows.long(), :eng.d].cpu().clone()
    fit = KMeans(eng, max_iter=5).fit(T, rows, K, init=init)
    out["kmeans assign"], out["kmeans centres"], out["kmeans inertia"] = (t.cpu().clone() for t in
                                                                          (fit.assign, fit.centres, fit.inertia))
    return out


def run_current_table(kernels, dev, run, hooks=None, later=None):
    """The `Checks` of B for run = (data, plan, cosine mode): data "sequence" is the fp64 sequence_case (exact: the
    gathered table is also held to SequenceCase.Z), "f32" / "bf16" random float data at d = 64.  ``later``: whether the
    consumers of tests/consumer_later_cases.py are compared as well (None: on the HIP kernels; the CPU double has none of
    their kernels).  ``checks.cur_seen`` lists ``eng.cur`` at every comparison."""
    from . import consumer_later_cases as CL
    hooks = hooks or Hooks()
    later = torch.device(dev).type == "cuda" if later is None else later
    data, plan_name, mode = run
    checks = X.Checks(f"current table {current_id(run)}")
    exact = data == "sequence"
    c = X.sequence_case() if exact else float_case({"f32": F32, "bf16": BF16}[data], 64, seed=1)
    fc = float_case(F64, c.d, seed=2) if exact else c                     # W, init, other data
    settings = dict(X.SEQUENCE_PLANS[plan_name] if exact else X.PLANS[plan_name][0], cosine_mode=mode)
    cc = consumer_case(F32, 64)                                           # its query and pair lists: vertices of graph()
    sources, src, dst = cc.sources, cc.pair_src, cc.pair_dst
    W = fc.W
    init = fc.init
    with X.device_ctx(dev):
        eng = X.make_engine(kernels, dev, c, **settings)
        assert len(eng.blocks) == 3 and eng.cosine_mode == mode
        hooks.after_engine(eng)
        old = _rankers(eng, W, hooks)                                     # before any sweep
        old_later = CL.Later(eng, c.dtype, c.d) if later else None        # objects and kept models, before any sweep
        checks.cur_seen = []

        def compare(step, expect=None):
            checks.cur_seen.append(eng.cur)
            fresh = X.make_engine(kernels, dev, c, **settings)
            fresh.set_Z(eng.get_Z())
            if later:
                want_later = old_later.results(fresh)
                for age, objs in (("old", old_later.old), ("new", None)):
                    CL.record_all(checks, f"B after {step}: {age}", old_later.results(eng, objs), want_later)
            want = {f"{n} ranker {k}": v for n, r in _rankers(fresh, W, Hooks()).items()
                    for k, v in _ranker_results(r, sources, src, dst).items()}
            want_other = _other_results(fresh, W, init, fc.K)
            for age, rankers in (("old", old), ("new", _rankers(eng, W, hooks))):
                for n, r in rankers.items():
                    for k, v in _ranker_results(r, sources, src, dst).items():
                        checks.record(f"B after {step}: {age} {n} ranker {k}", torch.equal(v, want[f"{n} ranker {k}"]),
                                      "rows that differ", _rows_that_differ(v, want[f"{n} ranker {k}"])[:6].tolist())
            got = _other_results(eng, W, init, fc.K)
            for k, v in got.items():
                checks.record(f"B after {step}: {k}", torch.equal(v, want_other[k]),
                              "vertices that differ", _rows_that_differ(v, want_other[k])[:6].tolist() if v.dim() else None)
            if expect is not None:
                checks.record(f"B after {step}: table_and_rows gathers the exact table",
                              torch.equal(got["table_and_rows"], expect),
                              _rows_that_differ(got["table_and_rows"], expect)[:6].tolist())

        eng.build_P()                                                     # leaves the norms of table 0 behind
        if exact:
            X.load_P(eng, c.P)                                            # ... and the exact P of the sequence back in
        eng.sweep(X.GAMMA)
        hooks.after_sweep(eng)
        compare(STEPS[0], c.Z[1] if exact else None)
        eng.snapshot()                                                    # the third table
        eng.sweep(X.GAMMA)
        hooks.after_sweep(eng)
        compare(STEPS[1], c.Z[2] if exact else None)
        eng.sweep_launch(X.GAMMA)
        eng.discard_launch()
        compare(STEPS[2], c.Z[2] if exact else None)
        eng.distance_from_snapshot()                                      # leaves norms behind in sq_pp
        compare(STEPS[3], c.Z[2] if exact else None)
        eng.sweep(X.GAMMA)                                                # into the third table: the one the launch taken
        hooks.after_sweep(eng)                                            # back wrote, now the current one
        assert eng.cur == 2
        compare(STEPS[4], c.Z[3] if exact else None)
        other = fc.Z1 if not exact else fc.Z1.round()
        eng.set_Z(other.to(c.dtype))
        compare(STEPS[5], other.to(c.dtype).double() if exact else None)
    return checks


def check_current_table(kernels, dev, run):
    checks = run_current_table(kernels, dev, run)
    checks.assert_none_failed()
    if torch.device(dev).type == "cuda":                                  # the later consumers were compared as well
        for step in STEPS:
            for what in ("old silhouette-euclidean samples", "new pca Y", "old mixture resp", "new predict-softmax proba",
                         "old label-model proba", "new mixture-model proba") + (("old knn7 ids",) * (run[0] != "sequence")):
                assert f"B after {step}: {what}" in checks.names, (step, what)
        assert ("B after sweep 1: new knn7 ids" in checks.names) == (run[0] != "sequence")
