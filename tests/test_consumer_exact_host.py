"""The exact consumer checks of tests/consumer_exact_cases.py, without a GPU: every case builder's range assertions, every
check of tests/test_gpu_consumer_exact.py (A.1 - A.6 and B) through a CPU test double with the same torch.equal / ==
comparisons -- which proves the fixtures exact and the reference right before a HIP kernel meets them -- and mutation
self-checks: the PROJECT made wrong in one named way (the vertex -> table-row map, the sort of the adjacency, the labels
of the padding rows, a stale norm flag, a projection of the wrong table) must fail the checks it targets, under the
plans where it matters, and no unrelated one.

The double extends the existing ones (training, k-means, the two probes) with the four link kernels in plain torch:
``rank_scores`` / ``rank_merge`` / ``rank_count`` / ``pair_score`` follow the order rule of include/clane_hip.h (score
descending, ties by LABEL ascending; label < 0 never is a candidate), its zero-row rule (a row outside the table, or of
norm 0 per edge, scores 0) and its slab ranges, and search the exclusion CSR the way the kernels do -- by bisection, so
that an unsorted row is missed here as it would be there.  ``pair_labels`` bisects as well.

A.7 (plan independence of the dense kernels' bits) is a statement about the HIP kernels; here it only runs to prove that
its fixtures build.  So is A.8 (tests/consumer_later_cases.py): here its fixtures' teeth are asserted on the engines the
double builds -- the vertex list, the permutation of the listed rows, the padding rows, the leading dimension, the
three tables B passes through -- with no kernel of the later consumers involved."""
import pytest
import torch

from clane_amd import _hip
from clane_amd import bilinear as bilinear_mod
from clane_amd import links as links_mod
from clane_amd import train as train_mod
from clane_amd.plan import _round_up

from . import consumer_exact_cases as CX
from . import consumer_later_cases as CL
from . import engine_exact_cases as X
from .exact_cases import F32, F64
from .test_cluster_host import KMeansOracleKernels
from .test_multilabel_host import MultilabelOracleKernels
from .test_train_host import TrainOracleKernels

DEV = "cpu"
TILE = 128                                                   # CLANE_RANK candidate rows per tile (kRankBN)


def _bisect_has(rowptr, colidx, r, want):
    """bool per (row r[i], wanted column want[i]): rank_excluded / pair_labels_kernel's binary search, which trusts the
    row to be sorted."""
    n = colidx.numel()
    lo, end = rowptr[r].clone(), rowptr[r + 1]
    hi = end.clone()
    while bool((lo < hi).any()):
        live = lo < hi
        mid = lo + (hi - lo) // 2
        below = live & (colidx[mid.clamp(max=n - 1)].long() < want)
        lo = torch.where(below, mid + 1, lo)
        hi = torch.where(live & ~below, mid, hi)
    return (lo < end) & (colidx[lo.clamp(max=n - 1)].long() == want)


class ConsumerOracleKernels(TrainOracleKernels, KMeansOracleKernels, MultilabelOracleKernels):
    """Every optional call of KernelBackend: the existing doubles' and the link kernels of csrc/link_rank.h /
    csrc/link_eval.h (the same formulas and order rules, no attempt at the MFMA's rounding: on the integer data of
    consumer_exact_cases every order of additions gives the same bits)."""

    def pair_labels(self, rowptr, colidx, nrows, src, dst, linked):
        s, t = src.long(), dst.long()
        inside = (s >= 0) & (s < nrows)
        linked.copy_((inside & _bisect_has(rowptr, colidx, s.clamp(0, nrows - 1), t)).to(torch.uint8))

    # ---- the link kernels -------------------------------------------------------------------------------------------------
    @staticmethod
    def _score_rows(S, N, table_rows, d, q, mode, sums2, sq):
        """[len(q), table_rows] scores in the accumulate dtype: (dot * query factor) * candidate factor."""
        acc = _hip.acc_dtype(S.dtype)
        dots = S[q.clamp(0, table_rows - 1), :d].to(acc) @ N[:table_rows, :d].to(acc).T
        if mode == _hip.SCORE_REFERENCE:
            return dots * (1.0 / (sums2[0] * sums2[1]).sqrt()).to(acc)
        if mode == _hip.SCORE_PER_EDGE:
            x = sq[:table_rows]
            rn = torch.where(x > 0, (1.0 / x.double().sqrt()).to(acc), torch.zeros_like(x))
            return (dots * rn[q.clamp(0, table_rows - 1)][:, None]) * rn[None, :]
        return dots

    @staticmethod
    def _excluded(rowptr, colidx, q, table_rows):
        """bool [len(q), table_rows]: candidate v is found in row q of the exclusion CSR -- by bisection where a row is not
        sorted (the cached dense form is the same thing where all are)."""
        dense = getattr(rowptr, "_consumer_dense", None)
        if dense is None:
            E = int(rowptr[-1])
            deg = rowptr[1:] - rowptr[:-1]
            row = torch.repeat_interleave(torch.arange(deg.numel()), deg)
            col = colidx[:E].long()
            if bool(((row[1:] != row[:-1]) | (col[1:] > col[:-1])).all()):
                dense = torch.zeros(deg.numel(), table_rows, dtype=torch.bool)
                dense[row, col] = True
            else:
                dense = False
            rowptr._consumer_dense = dense
        if dense is not False:
            return dense[q]
        Q = q.numel()
        r = q.repeat_interleave(table_rows)
        return _bisect_has(rowptr, colidx, r, torch.arange(table_rows).repeat(Q)).view(Q, table_rows)

    def _eligible(self, q, table_rows, label, excl_rowptr, excl_colidx, exclude_self):
        rows = torch.arange(table_rows)
        lab = rows if label is None else label[:table_rows].long()
        inside = (q >= 0) & (q < table_rows)
        qc = q.clamp(0, table_rows - 1)
        ok = (lab >= 0)[None, :] & inside[:, None]
        if exclude_self:
            ok = ok & (rows[None, :] != qc[:, None])
        if excl_rowptr is not None:
            ok = ok & ~self._excluded(excl_rowptr, excl_colidx, qc, table_rows)
        return ok, lab

    @staticmethod
    def _slabs(table_rows, n_slabs):
        tiles = -(-table_rows // TILE)
        per = -(-max(tiles, 1) // n_slabs)
        for s in range(n_slabs):
            t0 = min(s * per, tiles)
            yield s, t0 * TILE, min(min(t0 + per, tiles) * TILE, table_rows)

    def rank_scores(self, S, N, table_rows, d, q_rows, mode, sums2, sq, label, excl_rowptr, excl_colidx, exclude_self, k,
                    n_slabs, cand_score, cand_id):
        uq, back = torch.unique(q_rows.long(), return_inverse=True)       # a query's candidates do not depend on its place
        sc = self._score_rows(S, N, table_rows, d, uq, mode, sums2, sq)
        ok, lab = self._eligible(uq, table_rows, label, excl_rowptr, excl_colidx, exclude_self)
        by_label = torch.sort(lab, stable=True).indices                   # ties: by label ascending
        U = uq.numel()
        cs = torch.full((U, n_slabs, k), float("-inf"), dtype=sc.dtype)
        ci = torch.full((U, n_slabs, k), -1, dtype=torch.int32)
        for s, a, b in self._slabs(table_rows, n_slabs):
            cols = by_label[(by_label >= a) & (by_label < b)]
            if cols.numel() == 0:
                continue
            okc, scc = ok[:, cols], sc[:, cols]
            idx = torch.sort(torch.where(okc, -scc, torch.full_like(scc, float("inf"))), dim=1, stable=True).indices[:, :k]
            there = okc.gather(1, idx)
            n = idx.shape[1]
            cs[:, s, :n] = torch.where(there, scc.gather(1, idx), torch.full_like(scc[:, :n], float("-inf")))
            ci[:, s, :n] = torch.where(there, lab[cols][idx], torch.full_like(idx, -1)).to(torch.int32)
        n = q_rows.numel() * n_slabs * k
        cand_score[:n] = cs[back].reshape(-1)
        cand_id[:n] = ci[back].reshape(-1)

    def rank_merge(self, cand_score, cand_id, n_slabs, k, out_score, out_id):
        Q = out_id.numel() // k
        cs, ci = cand_score[:Q * n_slabs * k].view(Q, n_slabs * k), cand_id[:Q * n_slabs * k].view(Q, n_slabs * k)
        first = torch.sort(ci, dim=1, stable=True).indices                # by label, then stably by score
        cs, ci = cs.gather(1, first), ci.gather(1, first)
        order = torch.sort(torch.where(ci >= 0, -cs, torch.full_like(cs, float("inf"))), dim=1, stable=True).indices[:, :k]
        out_score.view(Q, k).copy_(cs.gather(1, order))
        out_id.view(Q, k).copy_(ci.gather(1, order))

    def pair_score(self, S, N, table_rows, d, src, dst, mode, sums2, sq, out):
        acc = _hip.acc_dtype(S.dtype)
        s, t = src.long(), dst.long()
        ok = (s >= 0) & (s < table_rows) & (t >= 0) & (t < table_rows)
        s, t = s.clamp(0, table_rows - 1), t.clamp(0, table_rows - 1)
        dot = (S[s, :d].to(acc) * N[t, :d].to(acc)).sum(1) * ok.to(acc)
        f, h = torch.ones((), dtype=acc), torch.ones((), dtype=acc)
        if mode == _hip.SCORE_REFERENCE:
            f = (1.0 / (sums2[0] * sums2[1]).sqrt()).to(acc)
        if mode == _hip.SCORE_PER_EDGE:
            x = sq[:table_rows]
            rn = torch.where(x > 0, (1.0 / x.double().sqrt()).to(acc), torch.zeros_like(x))
            f, h = rn[s] * ok.to(acc), rn[t] * ok.to(acc)
        out[:s.numel()] = (dot * f) * h

    def rank_count(self, S, N, table_rows, d, q_rows, t_rows, mode, sums2, sq, label, excl_rowptr, excl_colidx,
                   exclude_self, n_slabs, target_score, counts):
        q, t = q_rows.long(), t_rows.long()
        B = q.numel()
        sc = self._score_rows(S, N, table_rows, d, q, mode, sums2, sq)
        ok, lab = self._eligible(q, table_rows, label, excl_rowptr, excl_colidx, exclude_self)
        inside_t = (t >= 0) & (t < table_rows)
        tc = t.clamp(0, table_rows - 1)
        valid = (q >= 0) & (q < table_rows) & inside_t & (lab[tc] >= 0)
        ok = ok & (torch.arange(table_rows)[None, :] != tc[:, None])      # the target never is a candidate
        target = sc[torch.arange(B), tc]
        out = counts.view(B, n_slabs, 4)
        for s, a, b in self._slabs(table_rows, n_slabs):
            okc, scc, labc = ok[:, a:b], sc[:, a:b], lab[a:b]
            same = okc & (scc == target[:, None])
            out[:, s, 0] = (okc & (scc > target[:, None])).sum(1)
            out[:, s, 1] = (same & (labc[None, :] < lab[tc][:, None])).sum(1)
            out[:, s, 2] = (same & (labc[None, :] > lab[tc][:, None])).sum(1)
            out[:, s, 3] = okc.sum(1)
        out[~valid] = -1
        target_score[:B] = torch.where(valid, target, torch.full_like(target, float("-inf")))


@pytest.fixture(scope="module")
def k():
    return ConsumerOracleKernels()


# ---- the fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.ENGINE_CASES, ids=X.case_id)
def test_consumer_case_is_exact_and_has_what_the_checks_need(case):
    """Building the case asserts the range conditions (below 2^24 for every partial sum of the projection and of a pair's
    dot).  Here, what makes the checks bite: ties that table-row order would break the other way, a zero row with
    out-edges, sources with fewer than 32 eligible candidates, pairs that are edges."""
    c, ref = CX.consumer_case(*case), CX.reference(*case)
    g = X.graph()
    assert c.q == {3: 1, 13: 4, 16: 16, 32: 16, 64: 64, 70: 64, 128: 64, 130: 64, 256: 256, 300: 256, 520: 256}[c.d]
    assert max(c.project_bound, c.pair_bound) < X.E.EXACT_LIMIT and g.deg[c.zero_vertex] > 0
    assert c.Z0[c.copies].equal(c.Z0[c.copy_of]) and not bool(c.Z0[c.zero_vertex].any())
    for mode in CX.MODES:
        sc = ref.scores[mode]
        assert sc.dtype == c.acc and bool(torch.isfinite(sc).all())
        assert bool((sc[:, c.copies] == sc[:, c.copy_of]).all())                 # the planted ties
        ids, scores = ref.order(mode, True)
        tied = (scores[:, 1:] == scores[:, :-1]) & (ids[:, 1:] >= 0)
        assert int(tied.sum()) > 100 and bool((ids[:, 1:][tied] > ids[:, :-1][tied]).all())
    assert bool((ref.scores["per_edge"][c.zero_vertex] == 0).all())
    assert int((ref.n_eligible(True) < 32).sum()) >= 1 and int(ref.n_eligible(True).min()) == 0
    assert int(ref.adj[c.pair_src, c.pair_dst].sum()) >= 30
    if c.d >= 64:                                           # the reference factor is no power of two: one real rounding
        assert ref.scores["reference"].double().ne(ref.scores["per_edge"].double()).any()


@pytest.mark.parametrize("case", X.SPLIT_CASES, ids=X.case_id)
def test_split_consumer_case_is_exact(case):
    c = CX.consumer_case(*case, "split")
    assert max(c.project_bound, c.pair_bound) < X.E.EXACT_LIMIT and c.q in (16, 64)


def test_several_n_slabs_occur_in_one_call(k):
    """The long query list of `slab_batches` (its own assertion) on both graphs and both query-tile widths."""
    for case, gname in (((F32, 64), "ragged"), ((F64, 16), "ragged"), ((F32, 64), "split"), ((F64, 16), "split")):
        c = CX.consumer_case(*case, gname)
        eng = X.make_engine(k, DEV, c)
        sources, batch = CX.slab_batches(links_mod.LinkRanker(eng, c.similarity("per_edge")), c, eng.V)
        assert (sources is None) == (gname == "split")


# ---- the checks on the double --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", X.PLAN_RUNS, ids=X.plan_id)
def test_consumers_under_every_plan_on_the_double(k, run):
    CX.check_plan(k, DEV, *run)


@pytest.mark.parametrize("run", CX.SPLIT_RUNS, ids=X.plan_id)
def test_consumers_on_the_split_graph_on_the_double(k, run):
    CX.check_split(k, DEV, *run)


@pytest.mark.parametrize("run", CX.CURRENT_RUNS, ids=CX.current_id)
def test_current_table_on_the_double(k, run):
    CX.check_current_table(k, DEV, run)


def test_plan_independence_fixtures_build(k):
    """A.7 is a statement about the HIP kernels' bits; on the double it only has to run (the double's matmuls promise no
    order): the fits come out finite and of the expected shapes under two plans."""
    case = (F64, 64)
    for plan in ("defaults", "chunks3_class"):
        fits = CX.float_fits(k, DEV, case, plan)
        assert len(fits) == 11 and all(bool(torch.isfinite(t.double()).all()) for t in fits.values())
        assert fits["kmeans assign"].shape == (700, 3) and fits["probe pred"].shape == (700, 3)


# ---- mutation self-checks ----------------------------------------------------------------------------------------------------
CASE = (F32, 128)
GROUPS = ("A1", "A2", "A3", "A4", "A5", "A6")


def _run(k, plan, hooks=None, case=CASE):
    settings, route = X.PLANS[plan]
    return CX.run_consumers(k, DEV, case, settings, route, plan, hooks=hooks)


def _groups(names):
    return {n.split()[0] for n in names}


def test_unmutated_run_passes_and_every_comparison_is_made(k):
    checks = _run(k, "chunks3_class")
    assert checks.failed == [] and _groups(checks.names) == set(GROUPS)
    assert len(checks.names) == len(set(checks.names)) > 150
    for mode in CX.MODES:
        for what in ("top_k k=32 excl=on all ids", "tail of the short rows excl=on", "rank_pairs eligible filter=on",
                     "evaluate filter=off", "score_pairs", "place in top_k excl=on", "top_k k=10 excl=on several n_slabs ids"):
            assert any(n.endswith(f"{mode} {what}") for n in checks.names), (mode, what)


class PosIsIdentity(CX.Hooks):
    def after_engine(self, eng):
        eng.pos = torch.arange(eng.V, device=eng.device)


def test_mutation_a_pos_replaced_by_the_identity(k):
    """Every consumer then reads the rows of other vertices: something of every part of A fails under a shuffled plan
    (the X table has its own map and stays right); where the layout keeps the vertex order, pos IS the identity."""
    for plan in ("chunks3_in_order", "chunks3_class"):
        checks = _run(k, plan, PosIsIdentity())
        failed = checks.failed_names()
        assert _groups(failed) == set(GROUPS), (plan, _groups(failed))
        assert "A1 table Z all" in failed and "A1 table X all" not in failed
        name, _, where = next(f for f in checks.failed if f[0] == "A1 table Z all")[:3]
        assert len(where[0]) == 4 and where[0][1] == where[0][0]             # (vertex, the row it was looked up at, ...)
    assert _run(k, "chunks3_vertex_order", PosIsIdentity()).failed == []


def _engine_order_adjacency(eng):
    """train.sorted_adjacency without its sort: the engine's own edge order."""
    cached = getattr(eng, "_unsorted_adjacency", None)
    if cached is not None:
        return cached
    dev, R = eng.device, eng.part.padded_vertices
    own = torch.from_numpy(eng.part.local_positions()).to(dev)
    deg = (eng.rowptr[1:] - eng.rowptr[:-1])[:eng.part.n_local]
    src = torch.repeat_interleave(own[:deg.numel()], deg)
    order = torch.sort(src, stable=True).indices
    counts = torch.zeros(R, dtype=torch.int64, device=dev)
    counts.index_add_(0, src, torch.ones_like(src))
    rowptr = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(counts, 0)
    eng._unsorted_adjacency = (rowptr, eng.colidx[:eng.E_loc][order].contiguous(), R)
    return eng._unsorted_adjacency


def test_mutation_b_adjacency_left_in_the_engines_edge_order(k, monkeypatch):
    """The class pass keeps its rows in (class, column) order: a bisection misses their columns.  The sort check of A.2,
    the labels of A.3 and what excludes existing edges in A.5 / A.6 fail under a class plan -- nothing that does not
    search the adjacency -- and nothing at all where no row is a class row."""
    monkeypatch.setattr(train_mod, "sorted_adjacency", _engine_order_adjacency)
    monkeypatch.setattr(links_mod, "sorted_adjacency", _engine_order_adjacency)
    for plan in ("class_chunk64", "chunks3_class"):
        checks = _run(k, plan)
        failed = checks.failed_names()
        assert "A2 adjacency rows strictly increasing" in failed and "A2 adjacency rows are the graph's" not in failed
        assert any(n.startswith("A3 sampler f=1") for n in failed)
        for mode, group in zip(CX.MODES, ("A5", "A6", "A6")):
            assert f"{group} {mode} top_k k=32 excl=on all ids" in failed
            assert f"{group} {mode} rank_pairs eligible filter=on" in failed
        assert _groups(failed) == {"A2", "A3", "A5", "A6"}
        assert not any("excl=off" in n or "filter=off" in n or "score_pairs" in n for n in failed), failed
        where = next(f for f in checks.failed if f[0] == "A2 adjacency rows strictly increasing")[2]
        assert all(degree > 32 for _, _, degree, _ in where)                # the message names class rows
    assert _run(k, "row_pass_only").failed == []


class PadsAreLabelled(CX.Hooks):
    def after_ranker(self, ranker):
        pads = (ranker.label < 0).nonzero().flatten()
        ranker.label[pads] = (ranker.eng.V + torch.arange(pads.numel(), device=pads.device)).to(torch.int32)


def test_mutation_c_padding_rows_become_candidates(k):
    """A padding row is a zero row: it scores 0, is counted as eligible and fills the tail of a source that has fewer than
    k real candidates.  Only where the table has padding rows: the three-block plans (702 rows for 700 vertices)."""
    for plan in ("chunks3_overlap", "chunks3_in_order", "chunks3_vertex_order", "chunks3_class"):
        failed = _run(k, plan, PadsAreLabelled()).failed_names()
        assert _groups(failed) == {"A5", "A6"}
        for mode, group in zip(CX.MODES, ("A5", "A6", "A6")):
            for filtered in ("on", "off"):
                assert f"{group} {mode} rank_pairs eligible filter={filtered}" in failed
            assert f"{group} {mode} tail of the short rows excl=on" in failed
        assert not any("score_pairs" in n for n in failed)
    for plan in ("defaults", "class_chunk64", "tiles2_class"):
        assert _run(k, plan, PadsAreLabelled()).failed == []


class NormsFlaggedAfterSweep(CX.Hooks):
    def after_sweep(self, eng):
        eng.sq_ok[eng.cur] = True


@pytest.mark.parametrize("mode", ["reference", "per_edge"])
def test_mutation_d_norms_flagged_valid_right_after_a_sweep(k, mode):
    """prepare() then trusts norms nobody computed for the table the sweep wrote: the cosine comparisons fail from the
    first sweep on (zeros for a table never normed, then the norms of an older table), nothing bilinear and no table read
    does; right after l1_between has left the right norms behind and after set_Z (which clears the flags) the cosine is
    right."""
    checks = CX.run_current_table(k, DEV, ("sequence", "chunks3_class", mode), NormsFlaggedAfterSweep())
    failed = checks.failed_names()
    assert failed and all("cosine ranker" in n for n in failed), failed
    for step in CX.STEPS[:3] + CX.STEPS[4:5]:
        assert f"B after {step}: old cosine ranker top_k scores" in failed
        assert f"B after {step}: new cosine ranker score_pairs" in failed
    assert not any(CX.STEPS[3] in n or CX.STEPS[5] in n for n in failed)


def _project_first_table(eng, W):
    """bilinear.project_table reading Zbuf[0] in place of Zcur."""
    d = eng.d
    W = W.detach().to(eng.device, eng.acc_dtype).contiguous()
    Z = eng.Zbuf[0]
    if eng._Y is None:
        eng._Y = torch.empty(Z.shape[0], _round_up(2 * d, _hip.VEC_ELEMS[eng.acc_dtype]), dtype=eng.acc_dtype,
                             device=eng.device)
    eng.k.project_rows(Z, d, W, eng._Y)
    return eng._Y[:, :d], eng._Y[:, d:2 * d]


def test_mutation_e_projection_of_the_first_table(k, monkeypatch):
    """Right while table 0 is current (a fresh engine, after the sweep that returns to it, after set_Z), wrong while table 1
    or the third table is: the bilinear comparisons and project_table's own fail there, nothing else."""
    real = bilinear_mod.project_table
    calls = []

    def patched(eng, W):
        calls.append(eng.cur)
        return _project_first_table(eng, W) if getattr(eng, "_mutated", False) else real(eng, W)

    class Mark(CX.Hooks):
        def after_engine(self, eng):
            eng._mutated = True

    monkeypatch.setattr(bilinear_mod, "project_table", patched)
    checks = CX.run_current_table(k, DEV, ("f32", "chunks3_class", "per_edge"), Mark())
    failed = checks.failed_names()
    assert failed and all("bilinear ranker" in n or "project_table" in n for n in failed), failed
    for step in (CX.STEPS[0], CX.STEPS[4]):                                # table 1, then table 2 is current; else table 0
        assert f"B after {step}: project_table S" in failed and f"B after {step}: old bilinear ranker top_k scores" in failed
    assert not any(CX.STEPS[i] in n for n in failed for i in (1, 2, 3, 5)) and set(calls) == {0, 1, 2}


def test_unmutated_current_table_makes_every_comparison(k):
    checks = CX.run_current_table(k, DEV, ("sequence", "chunks3_tiles2", "per_edge"))
    assert checks.failed == [] and len(checks.names) == len(set(checks.names))
    for step in CX.STEPS:
        for what in ("old cosine ranker top_k ids", "new bilinear ranker rank_pairs score", "project_table N",
                     "table_and_rows", "kmeans inertia", "table_and_rows gathers the exact table"):
            assert f"B after {step}: {what}" in checks.names


# ---- the later consumers' fixtures (A.8, B) ------------------------------------------------------------------------------------
def test_later_vertex_list_is_neither_sorted_nor_everyone():
    L = CL.vertex_list()
    V = X.n_vertices(X.graph())
    assert L.numel() == CL.N_LISTED < V and L.unique().numel() == L.numel() and L.dtype == torch.int64
    assert int(L.min()) == 0 and int(L.max()) == V - 1 and set(CL.EDGE_VERTICES) <= set(L.tolist())
    ups = int((L[1:] > L[:-1]).sum())
    assert L.numel() // 3 < ups < 2 * L.numel() // 3                      # neither ascending nor descending
    for case in [c for c, _ in CL.LATER_RUNS] + [(F64, 32)]:
        c = CL.later_case(*case)
        assert c.part.numel() == c.Y0.shape[0] == c.resp0.shape[1] == L.numel() and torch.equal(c.vertices, L)
        assert bool((c.resp0.sum(2) - 1).abs().max() < 1e-12) and c.has_distances == (case[0] != F64)


def _edge_vertices(eng):
    """The real vertices on both sides of every block edge, in table-row order."""
    lv, out = eng.local.vertex, []
    for b in eng.blocks[1:]:
        lo, hi = b.local_start - 1, b.local_start
        while lv[lo] < 0:
            lo -= 1
        while lv[hi] < 0:
            hi += 1
        out += [int(lv[lo]), int(lv[hi])]
    return out


@pytest.mark.parametrize("run", CL.LATER_RUNS, ids=X.plan_id)
def test_later_fixture_has_teeth_under_plan(k, run):
    """What each plan of A.8 changes for a consumer.  The permutation: every plan but chunks3_vertex_order (whose pos is the
    identity) -- defaults, contiguous_tables and the tile plans through hot_rows_first.  Padding rows: the three-block
    plans.  A leading dimension wider than d: NOT the tile plans as such (a tile is a column range of one table; ld == d
    at d = 128, 64, 300), only PADDED_CASES."""
    case, plan = run
    L = CL.later_case(*case)
    settings, route = X.PLANS[plan]
    eng = X.make_engine(k, DEV, L.base, **settings)
    route(eng, DEV)
    V, pos, listed = eng.V, eng.pos.cpu(), L.vertices
    rows = pos[listed]
    T, got = CX.table_and_rows(eng, listed)
    assert torch.equal(got.long(), rows) and T is eng.Zcur
    steps = rows[1:] - rows[:-1]
    assert bool((steps > 0).any()) and bool((steps < 0).any())             # the listed rows are not monotone
    if plan in CL.IN_VERTEX_ORDER:
        assert torch.equal(rows, listed)
    else:
        assert int((rows != listed).sum()) > listed.numel() // 2
        in_row_order = listed[torch.sort(rows).indices]                    # the list is not in table-row order either
        assert int((in_row_order != listed).sum()) > listed.numel() // 2
    pads = int((eng.local.vertex < 0).sum())
    if plan in CL.THREE_BLOCK_PLANS:
        assert eng.Zcur.shape[0] == eng.X_loc.shape[0] == V + pads == 702 and pads == 2
        assert set(_edge_vertices(eng)) <= set(listed.tolist())
        blocks = X.block_of_vertex(eng)[listed.numpy()]
        assert set(blocks.tolist()) == {0, 1, 2}
    else:
        assert eng.Zcur.shape[0] == V and pads == 0
    assert eng.Zcur.stride() == (eng.ld, 1) and eng.X_loc.stride() == (eng.ld, 1)
    if case in CL.PADDED_CASES:
        assert eng.ld > eng.d and len(eng.tiles) == 2
    else:
        assert eng.ld == eng.d                                              # tiles or not
    # X_loc is in local-row order, which on one GPU is the table-row order: pos-mapped rows ARE its right rows
    TX, xrows = CX.table_and_rows(eng, listed, "X")
    assert TX is eng.X_loc and torch.equal(xrows.long(), rows)
    assert torch.equal(TX[xrows.long(), :eng.d].double(), L.base.X[listed].to(L.dtype).double())


def test_edge_vertices_cover_the_plans_of_b(k):
    """The three-block engines of B (the sequence plans; chunks3_class is covered above): the list holds both neighbours
    of their block edges too."""
    listed = set(CL.vertex_list().tolist())
    for plan, settings in X.SEQUENCE_PLANS.items():
        eng = X.make_engine(k, DEV, X.sequence_case(), **settings)
        assert len(eng.blocks) == 3 and set(_edge_vertices(eng)) <= listed, plan


@pytest.mark.parametrize("run", [CX.CURRENT_RUNS[0], CX.CURRENT_RUNS[-1]], ids=CX.current_id)
def test_current_table_passes_through_all_three_tables(k, run):
    checks = CX.run_current_table(k, DEV, run)
    assert checks.failed == [] and len(checks.cur_seen) == len(CX.STEPS) and set(checks.cur_seen) == {0, 1, 2}
    assert not any("knn7" in n or "mixture" in n for n in checks.names)    # the later consumers: HIP kernels only
