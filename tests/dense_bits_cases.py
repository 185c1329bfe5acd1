"""Float-data cases that hold every dense (MFMA) kernel to ONE order of the k terms -- helpers of
tests/test_gpu_dense_bits.py (the HIP kernels) and tests/test_dense_bits_host.py (the fixtures' and the expectation
functions' self-checks).

csrc/mfma_tile.h promises that the order in which the k terms of a dot are accumulated "is a fixed permutation, identical
for every element, every kernel and every call", whatever tile, slab or lane a (row, column) pair falls in.  Then every
dense kernel forms a (row, column) dot with the bits project_rows forms for the same operands, and what a kernel derives
from its dots (top-k lists, rank counts, arg-max classes, label masks, nearest centres, gradients summed over chunks)
can be computed on the CPU from project_rows' output alone -- `anchor_dots` -- and compared with torch.equal.  The data
are random non-integer floats: a dot's bits do depend on the order (test_dense_bits_host.py asserts how often), so a
kernel whose order differs from mfma_slice's, or between two tiles, or whose tie rule leans on integer data tying
exactly, fails.  project_rows itself is pinned against float64 (A1, the only tolerance) and by position invariance (A2).

Layout of a relation: `expect_*` computes on the CPU, from dots, what the kernel must return; `assert_*` compares a
kernel's outputs with it; `check_*(k, dev, ...)` builds the fixture, runs the kernel and the anchor and calls assert_*.
The host file feeds assert_* with dots summed in two different orders on the CPU: each must raise.

Planted exact ties (the positions of the integer-data tie tests): table row 5 is also row 133 and row 290, centre 3 also
7 and 131, class 1 of every probe fit also class 2 and, where Cp = 64, class 17, and class 3 also class 40.  On float
data such a tie survives only if the bits do not depend on the position.

Sibling: tests/distance_bits_cases.py holds relations 9..13 (silhouette_norms, silhouette_sums, tsne_sqdist, knn_sqdist,
probe_predict) to the same anchor, with this module's fixtures.
"""
import functools

import torch

from clane_amd import _hip

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DTYPES = [F32, BF16, F64]
UNIT = {F32: 2.0 ** -24, F64: 2.0 ** -53}                  # unit roundoff of the accumulate type
ROWS = 300                                                 # table rows: 3 row tiles of 128, 5 of 64
DUP_ROWS = (5, 133, 290)                                   # one row, three tiles
DUP_CENTRES = (3, 7, 131)
DENSE_D = (5, 17, 130)                                     # a partial slice; one slice + 1; 8 slices + 2
RANK_D = (1,) + DENSE_D                                    # d = 1: the anchor and the ranking kernels only
LIST_N = (300, 2100)                                       # 2100: more than one 2048-row chunk
CHUNK = 2048                                               # kGradChunk
SAME_ROW_AT = (0, 1, 15, 16, 31, 32, 63, 64, 127, 128, 129, 299)
RANK_Q, RANK_K, RANK_SLABS, ROLL = 130, (1, 10, 32), (1, 3), 77
TARGETS = 6                                                # rank_count: targets per query
KMEANS_R, KMEANS_K = 2, (7, 140)
PROBE_SHAPES = ((7, 19), (33, 3), (64, 3))                 # (C, F): K = 152 / 192 / 192 columns, Cp = 8 / 64 / 64
GRAD_CF = (7, 19)                                          # probe_grad: K = 152 rows of dW, two 128-row tiles
GRAD_M = 64.0


def case_id(v):
    return _hip._SUFFIX[v] if isinstance(v, torch.dtype) else str(v)


# ---- fixtures: host tensors, seeded, never written to ------------------------------------------------------------------
def randn(seed, shape, dtype, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(dtype)


def randint(seed, lo, hi, shape):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def table(seed, d, dtype):
    """[ROWS, d] Gaussian values rounded to `dtype`; rows 133 and 290 repeat row 5."""
    Z = randn(seed, (ROWS, d), dtype)
    for r in DUP_ROWS[1:]:
        Z[r] = Z[DUP_ROWS[0]]
    return Z


def place(Z, dev):
    """A host matrix on the device with a padded leading dimension (d + 3)."""
    buf = torch.zeros(Z.shape[0], Z.shape[1] + 3, dtype=Z.dtype, device=dev)
    buf[:, :Z.shape[1]] = Z.to(dev)
    return buf[:, :Z.shape[1]]


@functools.lru_cache(maxsize=None)
def row_list(seed, n):
    """n table rows; outside the table (-1 and ROWS + 5) are one index in 37 of each kind and the places on both sides of
    the 64- and the 128-row tile edge; the three equal rows stand at both ends and in between."""
    idx = randint(seed, 0, ROWS, (n,))
    idx[5::37] = -1
    idx[11::37] = ROWS + 5
    if n > 128:
        idx[[63, 128]] = -1
        idx[[64, 127]] = ROWS + 5
    for pos, r in zip((0, n * 13 // 30, n - 1), DUP_ROWS):
        idx[pos] = r
    return idx.to(torch.int32)


def inside(idx, rows=ROWS):
    return (idx >= 0) & (idx < rows)


def gather(M, idx):
    """M[idx] with zero rows where idx is outside [0, rows(M)) -- how every kernel reads a listed row."""
    out = M[idx.long().clamp(0, M.shape[0] - 1)].clone()
    out[~inside(idx, M.shape[0])] = 0
    return out


def first_index_where(mask, dim):
    """Lowest index along `dim` at which mask holds (the size of `dim` where it never does)."""
    n = mask.shape[dim]
    shape = [1] * mask.dim()
    shape[dim] = n
    return torch.where(mask, torch.arange(n).view(shape), torch.tensor(n)).amin(dim)


# ---- the anchor ----------------------------------------------------------------------------------------------------------
def anchor_dots(k, A_rows, B_rows, dev, shift=0):
    """[nA, nB] dots of every A row with every B row in the accumulate dtype, by project_rows alone.  A is the table
    operand (its dtype picks the instance), B the W operand in the accumulate dtype; project_rows computes exactly 2 d'
    columns, so B goes in chunks of 2 d' rows, the last one zero-padded.  `shift` zero rows in front of B move every
    column to another place of the chunking (and of the tiles)."""
    nA, dp = A_rows.shape
    acc = _hip.acc_dtype(A_rows.dtype)
    assert B_rows.dtype == acc and B_rows.shape[1] == dp and dp >= 1
    A = place(A_rows, dev)
    B = torch.cat([torch.zeros(shift, dp, dtype=acc), B_rows]).to(dev)
    out = []
    for c0 in range(0, B.shape[0], 2 * dp):
        chunk = B[c0:c0 + 2 * dp]
        W = torch.zeros(2 * dp, dp, dtype=acc, device=dev)
        W[:chunk.shape[0]] = chunk
        Y = torch.full((nA, 2 * dp), float("nan"), dtype=acc, device=dev)
        k.project_rows(A, dp, W, Y)
        out.append(Y[:, :chunk.shape[0]].cpu())
    Y = torch.cat(out, dim=1)[:, shift:]
    assert not bool(torch.isnan(Y).any())
    return Y


def anchor_case(d, dtype):
    acc = _hip.acc_dtype(dtype)
    return table(1, d, dtype), randn(2, (2 * d, d), acc, 0.3)


def check_anchor_fp64(k, dev, dtype, d):
    """(A1) |Y - Y64| <= 2 d u |Z| |W|^T elementwise: gamma_d of any summation order (Higham, Accuracy and Stability of
    Numerical Algorithms, section 3.1: gamma_d = d u / (1 - d u) < 2 d u for d u < 1/2).  The only tolerance."""
    Z, W = anchor_case(d, dtype)
    Y = anchor_dots(k, Z, W, dev)
    Z64, W64 = Z.double(), W.double()
    err = (Y.double() - Z64 @ W64.T).abs()
    bound = 2 * d * UNIT[W.dtype] * (Z64.abs() @ W64.abs().T)
    print(f"anchor {case_id(dtype)} d={d}: max error / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    return Y


def check_anchor_positions(k, dev, dtype, d):
    """(A2) a row's bits do not depend on its place among the rows, a column's not on its place among the columns, and
    not on how anchor_dots cuts B into chunks."""
    Z, W = anchor_case(d, dtype)
    Y = anchor_dots(k, Z, W, dev)
    lst = torch.arange(ROWS)
    lst[list(SAME_ROW_AT)] = 7
    Y1 = anchor_dots(k, Z[lst], W, dev)
    for p in SAME_ROW_AT:
        assert torch.equal(Y1[p], Y[7]), (case_id(dtype), d, "row position", p)
    assert torch.equal(Y1, Y[lst])
    assert torch.equal(Y[DUP_ROWS[1]], Y[DUP_ROWS[0]]) and torch.equal(Y[DUP_ROWS[2]], Y[DUP_ROWS[0]])
    perm = torch.randperm(2 * d, generator=torch.Generator().manual_seed(3))
    assert torch.equal(anchor_dots(k, Z, W[perm], dev), Y[:, perm]), (case_id(dtype), d, "column position")
    assert torch.equal(anchor_dots(k, Z, W, dev, shift=3), Y), (case_id(dtype), d, "shifted chunking")


# ---- 1. pair_project -------------------------------------------------------------------------------------------------------
def expect_pair_project(anchor, src, dst, d):
    return gather(anchor[:, :d], src), gather(anchor[:, d:], dst)


def assert_pair_project(A, Bm, anchor, src, dst, d):
    wantA, wantB = expect_pair_project(anchor, src, dst, d)
    assert torch.equal(A, wantA), ("pair_project A", int((A != wantA).sum()))
    assert torch.equal(Bm, wantB), ("pair_project Bm", int((Bm != wantB).sum()))


def check_pair_project(k, dev, dtype, d, B=300):
    Z, W = anchor_case(d, dtype)
    src, dst = row_list(3, B), row_list(4, B)
    A, Bm = (torch.full((B, d), float("nan"), dtype=W.dtype, device=dev) for _ in range(2))
    k.pair_project(place(Z, dev), d, src.to(dev), dst.to(dev), W.to(dev), A, Bm)
    assert_pair_project(A.cpu(), Bm.cpu(), anchor_dots(k, Z, W, dev), src, dst, d)


# ---- 2. / 3. the ranking kernels -----------------------------------------------------------------------------------------
class RankCase:
    """S, N [ROWS, d] of `dtype`; label a permutation with holes; an exclusion CSR of 0..8 sorted columns per row; Q
    query rows, some outside the table.  rolled(s): the same problem with every table row moved s places down."""

    def __init__(self, d, dtype):
        self.d, self.dtype = d, dtype
        self.S, self.N = table(31, d, dtype), table(32, d, dtype).clone()
        # the equal rows, half as long again: they reach the top-k lists of more queries (at d = 1, of any at all)
        self.N[list(DUP_ROWS)] = (self.N[DUP_ROWS[0]].double() * (1.5 if d > 1 else 3.0)).to(dtype)
        g = torch.Generator().manual_seed(33)
        self.label = torch.randperm(ROWS, generator=g).to(torch.int32)
        self.label[4::41] = -1
        deg = randint(34, 0, 9, (ROWS,))
        self.excl = torch.zeros(ROWS, ROWS, dtype=torch.bool)          # excl[q, v]: v is a column of row q
        for r in range(ROWS):
            self.excl[r, torch.randperm(ROWS, generator=g)[:int(deg[r])]] = True
        self.q_rows = row_list(36, RANK_Q)

    def csr(self):
        rowptr = torch.zeros(ROWS + 1, dtype=torch.int64)
        rowptr[1:] = self.excl.sum(1).cumsum(0)
        return rowptr, self.excl.nonzero()[:, 1].to(torch.int32)        # row-major nonzero: sorted columns per row

    def eligible(self, q_rows=None):
        """[Q, ROWS]: candidate v counts for query q -- a label, not q itself, not excluded; no query: nothing."""
        q = (self.q_rows if q_rows is None else q_rows).long()
        ok = inside(q)
        qc = q.clamp(0, ROWS - 1)
        el = (self.label >= 0)[None, :] & ~self.excl[qc] & (torch.arange(ROWS)[None, :] != qc[:, None])
        return el & ok[:, None]

    def rolled(self, s):
        other = object.__new__(RankCase)
        other.d, other.dtype = self.d, self.dtype
        other.S, other.N, other.label = self.S.roll(s, 0), self.N.roll(s, 0), self.label.roll(s, 0)
        other.excl = self.excl.roll((s, s), (0, 1))
        q = self.q_rows.long()
        other.q_rows = torch.where(inside(q), (q + s) % ROWS, q).to(torch.int32)
        return other


@functools.lru_cache(maxsize=None)
def rank_case(d, dtype):
    return RankCase(d, dtype)


def expect_topk(scores, eligible, label, kk):
    """([Q, kk] scores, [Q, kk] labels) of the eligible candidates in the order (score descending, label ascending);
    unused places -inf / -1."""
    by_label = torch.argsort(label.long(), stable=True)
    s = torch.where(eligible, scores, torch.full_like(scores, float("-inf")))[:, by_label]
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :kk]       # stable: label order among equals
    cand = by_label[order]
    used = eligible.gather(1, cand)
    out_s = torch.where(used, scores.gather(1, cand), torch.full_like(scores[:, :kk], float("-inf")))
    out_i = torch.where(used, label[cand], torch.tensor(-1, dtype=label.dtype))
    return out_s, out_i


def assert_topk(got_score, got_id, scores, eligible, label, kk, tag=""):
    want_s, want_i = expect_topk(scores, eligible, label, kk)
    assert torch.equal(got_id, want_i), ("top-k ids", tag, (got_id != want_i).any(1).nonzero().flatten()[:8].tolist())
    assert torch.equal(got_score, want_s), ("top-k scores", tag, int((got_score != want_s).sum()))


def expect_counts(scores, eligible, label, pair_q, t_rows):
    """(target_score [B], counts [B, 4] = greater, equal_lower, equal_higher, eligible) of pair (query pair_q[b] of the
    score matrix, target row t_rows[b]); the target itself never is a candidate.  A pair whose query has no eligible row
    at all (no such query) or whose target is outside the table or unlabelled has no rank: -inf and four -1."""
    t, V = t_rows.long(), scores.shape[1]
    ranked = inside(t, V) & eligible[pair_q].any(1)
    tc = t.clamp(0, V - 1)
    ranked &= label[tc] >= 0
    s, el = scores[pair_q], eligible[pair_q].clone()
    el[torch.arange(t.numel()), tc] = False
    thr = s.gather(1, tc[:, None])
    tl = label[tc][:, None]
    eq = el & (s == thr)
    counts = torch.stack([(el & (s > thr)).sum(1), (eq & (label[None, :] < tl)).sum(1),
                          (eq & (label[None, :] > tl)).sum(1), el.sum(1)], dim=1).to(torch.int32)
    counts[~ranked] = -1
    return torch.where(ranked, thr[:, 0], torch.full_like(thr[:, 0], float("-inf"))), counts


def assert_counts(got_target, got_counts, scores, eligible, label, pair_q, t_rows):
    """got_counts [B, n_slabs, 4]: summed over the slabs; a pair without a rank has -1 in every slab."""
    want_t, want_c = expect_counts(scores, eligible, label, pair_q, t_rows)
    assert torch.equal(got_target, want_t), ("rank_count target_score", int((got_target != want_t).sum()))
    ranked = want_c[:, 0] >= 0
    assert bool((got_counts[~ranked] == -1).all()), "rank_count: a pair without a rank"
    got = got_counts[ranked].sum(1)
    assert torch.equal(got, want_c[ranked]), ("rank_count counts", (got != want_c[ranked]).any(1).nonzero().flatten()[:8])


_RANK_SCORES = {}


def rank_anchor(k, dev, d, dtype):
    """The anchor's [Q, ROWS] scores of rank_case(d, dtype), computed once: queries are the A operand, N the B operand,
    as rank_scores_kernel and rank_count_kernel stage them."""
    if (d, dtype) not in _RANK_SCORES:
        c = rank_case(d, dtype)
        _RANK_SCORES[d, dtype] = anchor_dots(k, gather(c.S, c.q_rows), c.N.to(_hip.acc_dtype(dtype)), dev)
    return _RANK_SCORES[d, dtype]


def run_top_k(k, dev, c, kk, n_slabs):
    acc = _hip.acc_dtype(c.dtype)
    Q = c.q_rows.numel()
    rowptr, colidx = c.csr()
    cs = torch.full((Q * n_slabs * kk,), float("nan"), dtype=acc, device=dev)
    ci = torch.full((Q * n_slabs * kk,), -7, dtype=torch.int32, device=dev)
    k.rank_scores(place(c.S, dev), place(c.N, dev), ROWS, c.d, c.q_rows.to(dev), _hip.SCORE_RAW_DOT, None, None,
                  c.label.to(dev), rowptr.to(dev), colidx.to(dev), True, kk, n_slabs, cs, ci)
    os_ = torch.full((Q, kk), float("nan"), dtype=acc, device=dev)
    oi = torch.full((Q, kk), -7, dtype=torch.int32, device=dev)
    k.rank_merge(cs, ci, n_slabs, kk, os_, oi)
    return os_.cpu(), oi.cpu()


def duplicate_runs(ids, label):
    """How many lists hold two or more of the three equal rows (by their labels)."""
    dup = torch.isin(ids, label[list(DUP_ROWS)])
    return int((dup.sum(1) >= 2).sum())


def check_rank_scores(k, dev, dtype, d):
    """rank_scores + rank_merge in SCORE_RAW_DOT (the score IS the accumulator) for every k and slab count, and the same
    lists after the table rows moved by ROLL: 130 queries cross the 128-query tile of f32 / bf16 (MI = 4) and the
    64-query tile of f64 (MI = 2)."""
    c = rank_case(d, dtype)
    scores, el = rank_anchor(k, dev, d, dtype), c.eligible()
    _, ids32 = expect_topk(scores, el, c.label, 32)
    assert bool((ids32[inside(c.q_rows)] >= 0).all()) and bool((ids32[~inside(c.q_rows)] == -1).all())
    assert duplicate_runs(ids32, c.label) >= 1, "the equal rows meet in no list: nothing tests the tie rule"
    moved = c.rolled(ROLL)
    assert torch.equal(moved.eligible(), el.roll(ROLL, 1))
    for kk in RANK_K:
        for n_slabs in RANK_SLABS:
            assert_topk(*run_top_k(k, dev, c, kk, n_slabs), scores, el, c.label, kk, (kk, n_slabs))
            assert_topk(*run_top_k(k, dev, moved, kk, n_slabs), scores, el, c.label, kk, (kk, n_slabs, "rolled"))


def count_targets(c, scores, el):
    """TARGETS rows per query: those at places 1, 7 and 32 of its expected list and three seeded eligible rows, one of
    them an equal row for every tenth query.  A query outside the table gets rows 0..5 (it has no rank anyway)."""
    _, ids32 = expect_topk(scores, el, c.label, 32)
    row_of_label = torch.full((ROWS,), -1, dtype=torch.int64)
    row_of_label[c.label[c.label >= 0].long()] = (c.label >= 0).nonzero().flatten()
    g = torch.Generator().manual_seed(38)
    t_rows = torch.arange(TARGETS).repeat(RANK_Q, 1)
    for q in range(RANK_Q):
        if not bool(el[q].any()):
            continue
        listed = row_of_label[ids32[q, [0, 6, 31]].long()]
        pool = el[q].nonzero().flatten()
        extra = pool[torch.randperm(pool.numel(), generator=g)[:3]]
        dup = DUP_ROWS[(q // 10) % 3]
        if q % 10 == 0 and bool(el[q, dup]):
            extra[0] = dup
        t_rows[q] = torch.cat([listed, extra])
    return t_rows.flatten().to(torch.int32)


def check_rank_count(k, dev, dtype, d):
    c = rank_case(d, dtype)
    acc = _hip.acc_dtype(dtype)
    scores, el = rank_anchor(k, dev, d, dtype), c.eligible()
    t_rows = count_targets(c, scores, el)
    pair_q = torch.arange(RANK_Q).repeat_interleave(TARGETS)
    _, want = expect_counts(scores, el, c.label, pair_q, t_rows)
    assert int((want[:, 0] < 0).sum()) >= TARGETS * 6 and int((want[:, 1] > 0).sum()) >= 1 and int((want[:, 2] > 0).sum()) >= 1
    rowptr, colidx = c.csr()
    B = t_rows.numel()
    for n_slabs in RANK_SLABS:
        ts = torch.full((B,), float("nan"), dtype=acc, device=dev)
        counts = torch.full((B * n_slabs * 4,), -7, dtype=torch.int32, device=dev)
        k.rank_count(place(c.S, dev), place(c.N, dev), ROWS, d, c.q_rows[pair_q].contiguous().to(dev), t_rows.to(dev),
                     _hip.SCORE_RAW_DOT, None, None, c.label.to(dev), rowptr.to(dev), colidx.to(dev), True, n_slabs, ts,
                     counts)
        assert_counts(ts.cpu(), counts.cpu().view(B, n_slabs, 4), scores, el, c.label, pair_q, t_rows)


# ---- 4. kmeans_assign ------------------------------------------------------------------------------------------------------
def kmeans_case(d, dtype, K):
    """centres [R, K, d] with centre 3 repeated at 7 and 131 (K = 7: at 6), csq random -- not the norms, so that nothing
    hides -- and lowest at the repeated centre, which then is the nearest of many rows."""
    acc = _hip.acc_dtype(dtype)
    centres = randn(43, (KMEANS_R, K, d), acc)
    csq = randn(44, (KMEANS_R, K), acc).abs() + 1
    csq[:, DUP_CENTRES[0]] = 0.5
    copies = [j for j in DUP_CENTRES[1:] if j < K] or [K - 1]
    for j in copies:
        centres[:, j], csq[:, j] = centres[:, DUP_CENTRES[0]], csq[:, DUP_CENTRES[0]]
    return centres, csq, copies


def expect_kmeans(dots, csq):
    """dots [R, n, K] -> (assign [n, R], best [n, R]): best = min_j (csq[r, j] - 2 dot) in the accumulate dtype (2 x is
    exact, so a fused multiply-subtract rounds the same once), assign the lowest j that attains it."""
    val = csq[:, None, :] - 2 * dots
    best = val.amin(2)
    assign = first_index_where(val == best[:, :, None], 2)
    return assign.T.to(torch.int32).contiguous(), best.T.contiguous()


def assert_kmeans(assign, best, dots, csq):
    want_a, want_b = expect_kmeans(dots, csq)
    assert torch.equal(best, want_b), ("kmeans best", int((best != want_b).sum()))
    assert torch.equal(assign, want_a), ("kmeans assign", (assign != want_a).any(1).nonzero().flatten()[:8].tolist())


def check_kmeans(k, dev, dtype, d, K, n=300):
    Z = table(41, d, dtype)
    rows = row_list(42, n)
    centres, csq, copies = kmeans_case(d, dtype, K)
    assign = torch.full((n, KMEANS_R), -7, dtype=torch.int32, device=dev)
    best = torch.full((n, KMEANS_R), float("nan"), dtype=csq.dtype, device=dev)
    k.kmeans_assign(place(Z, dev), d, rows.to(dev), centres.to(dev), csq.to(dev), assign, best)
    dots = torch.stack([anchor_dots(k, gather(Z, rows), centres[r], dev) for r in range(KMEANS_R)])
    assign, best = assign.cpu(), best.cpu()
    assert_kmeans(assign, best, dots, csq)
    want_a, _ = expect_kmeans(dots, csq)
    assert int((want_a == DUP_CENTRES[0]).sum()) >= 1 and not bool(torch.isin(assign, torch.tensor(copies)).any())


# ---- 5. / 6. the probes' forward passes ------------------------------------------------------------------------------------
def probe_weights(seed, d, acc, Cp, F):
    """W [F, Cp, d], bias [F, Cp] with class 1 repeated at 2 and (Cp = 64) 17, class 3 at 40: one 16-column tile and
    three."""
    W, bias = randn(seed, (F, Cp, d), acc, 0.3), randn(seed + 1, (F, Cp), acc, 0.3)
    for a, b in ((1, 2), (3, 40), (1, 17)):
        if b < Cp:
            W[:, b], bias[:, b] = W[:, a], bias[:, a]
    return W, bias


def softmax_case(d, dtype, C, F, n=300):
    acc, Cp = _hip.acc_dtype(dtype), _hip.probe_padded_classes(C)
    W, bias = probe_weights(14, d, acc, Cp, F)
    return dict(Z=table(11, d, dtype), rows=row_list(12, n), y=randint(16, 0, C, (n,)).to(torch.int32),
                split=randint(13, 0, 2, (n, F)).to(torch.uint8), W=W, bias=bias, d=d, C=C, Cp=Cp, F=F, n=n, acc=acc)


def logits_of(dots, bias):
    """[n, F, Cp]: ONE add in the accumulate dtype, as both probes form a logit."""
    F, Cp = bias.shape
    return dots.view(dots.shape[0], F, Cp) + bias[None]


def expect_pred(dots, bias, C):
    """[n, F]: the lowest class attaining max_c (dot + bias) over the C real classes."""
    l = logits_of(dots, bias)[:, :, :C]
    return first_index_where(l == l.amax(2, keepdim=True), 2).to(torch.int32)


def assert_pred(pred, dots, bias, C):
    want = expect_pred(dots, bias, C)
    assert torch.equal(pred, want), ("probe_forward pred", (pred != want).any(1).nonzero().flatten()[:8].tolist())


def run_softmax(k, dev, c, fits=None, order=None):
    """(G [n, F', Cp], loss [F'], pred [n, F']) of the fits `fits` (default all) with the rows in `order`."""
    fits = list(range(c["F"])) if fits is None else fits
    order = torch.arange(c["n"]) if order is None else order
    n, Cp, Fn = c["n"], c["Cp"], len(fits)
    W, bias = c["W"][fits].reshape(Fn * Cp, c["d"]).contiguous(), c["bias"][fits].reshape(-1).contiguous()
    G = torch.full((n * Fn * Cp,), float("nan"), dtype=c["acc"], device=dev)
    loss = torch.full((Fn,), float("nan"), dtype=torch.float64, device=dev)
    ws = torch.zeros(k.probe_loss_ws_len(n, Fn), dtype=torch.float64, device=dev)
    pred = torch.full((n, Fn), -7, dtype=torch.int32, device=dev)
    k.probe_forward(place(c["Z"], dev), c["d"], c["rows"][order].contiguous().to(dev), c["y"][order].contiguous().to(dev),
                    c["split"][order][:, fits].contiguous().to(dev), W.to(dev), bias.to(dev), Fn, c["C"], ws, loss,
                    G=G, pred=pred)
    return G.cpu().view(n, Fn, Cp), loss.cpu(), pred.cpu()


def check_probe_forward(k, dev, dtype, d, C, F):
    c = softmax_case(d, dtype, C, F)
    G, loss, pred = run_softmax(k, dev, c)
    dots = anchor_dots(k, gather(c["Z"], c["rows"]), c["W"].view(F * c["Cp"], d), dev)
    assert_pred(pred, dots, c["bias"], C)
    l = logits_of(dots, c["bias"])[:, :, :C]
    assert int(((l == l.amax(2, keepdim=True)).sum(2) >= 2).sum()) >= 1, "no row's maximum is a repeated class"
    assert bool(torch.isfinite(G).all()) and bool((loss > 0).all())
    # fit position: a fit alone, and the stack reversed -- what classify.py relies on when it groups fits
    for f in range(F):
        Ga, la, pa = run_softmax(k, dev, c, fits=[f])
        assert torch.equal(Ga[:, 0], G[:, f]) and torch.equal(la[0], loss[f]) and torch.equal(pa[:, 0], pred[:, f]), f
    back = list(range(F))[::-1]
    Gb, lb, pb = run_softmax(k, dev, c, fits=back)
    assert torch.equal(Gb, G[:, back]) and torch.equal(lb, loss[back]) and torch.equal(pb, pred[:, back])
    # row position (the loss is not compared: the order of its row tiles legitimately changes)
    perm = torch.randperm(c["n"], generator=torch.Generator().manual_seed(5))
    Gp, _, pp = run_softmax(k, dev, c, order=perm)
    assert torch.equal(Gp, G[perm]) and torch.equal(pp, pred[perm])


def ovr_case(d, dtype, C, F, n=300):
    acc, Cp = _hip.acc_dtype(dtype), _hip.ovr_padded_classes(C)
    W, bias = probe_weights(18, d, acc, Cp, F)
    Y = randint(20, 0, 4, (n, C)) == 0                                              # a quarter of the classes per row
    x = randint(21, 0, 8, (F, Cp))                                                  # an eighth of the columns -1, an eighth +1
    state = ((x == 1).long() - (x == 0).long()).to(torch.int8)
    for a, b in ((1, 2), (3, 40), (1, 17)):                                         # the repeated classes stay fitted
        state[:, a] = 0
        if b < Cp:
            state[:, b] = 0
    return dict(Z=table(11, d, dtype), rows=row_list(12, n), Y=Y, ymask=(Y.long() << torch.arange(C)).sum(1),
                split=randint(13, 0, 2, (n, F)).to(torch.uint8), W=W, bias=bias, state=state, d=d, C=C, Cp=Cp, F=F, n=n,
                acc=acc)


def expect_masks(dots, bias, state, Y, C, top_k):
    """int64 [n, F] label masks from logits = dots + bias, by the expectation of tests/test_gpu_multilabel.py (imported,
    not copied): top-k by (value descending, class ascending) with k_i = the row's number of true classes, or value > 0."""
    from .test_gpu_multilabel import _expected_masks
    return _expected_masks(logits_of(dots, bias)[:, :, :C].double(), state[:, :C], Y, top_k)     # widening: exact


def assert_masks(pred, dots, bias, state, Y, C, top_k):
    want = expect_masks(dots, bias, state, Y, C, top_k)
    assert torch.equal(pred, want), ("probe_forward_ovr pred", top_k, (pred != want).any(1).nonzero().flatten()[:8].tolist())


def run_ovr(k, dev, c, top_k, order=None):
    order = torch.arange(c["n"]) if order is None else order
    n, Cp, F, C = c["n"], c["Cp"], c["F"], c["C"]
    G = torch.full((n * F * Cp,), float("nan"), dtype=c["acc"], device=dev)
    loss = torch.full((F,), float("nan"), dtype=torch.float64, device=dev)
    ws = torch.zeros(k.probe_loss_ws_len(n, F), dtype=torch.float64, device=dev)
    pred = torch.full((n, F), -7, dtype=torch.int64, device=dev)
    k.probe_forward_ovr(place(c["Z"], dev), c["d"], c["rows"][order].contiguous().to(dev), c["ymask"][order].contiguous().to(dev),
                        c["split"][order].contiguous().to(dev), c["W"].view(F * Cp, c["d"]).to(dev),
                        c["bias"].view(-1).to(dev), c["state"].view(-1).to(dev), F, C, int(c["Y"].sum(1).max()), ws, loss,
                        G=G, pred=pred, top_k=top_k)
    return G.cpu().view(n, F, Cp), loss.cpu(), pred.cpu()


def check_probe_ovr(k, dev, dtype, d, C, F):
    c = ovr_case(d, dtype, C, F)
    dots = anchor_dots(k, gather(c["Z"], c["rows"]), c["W"].view(F * c["Cp"], d), dev)
    perm = torch.randperm(c["n"], generator=torch.Generator().manual_seed(5))
    for top_k in (True, False):
        G, loss, pred = run_ovr(k, dev, c, top_k)
        assert_masks(pred, dots, c["bias"], c["state"], c["Y"], C, top_k)
        assert bool(torch.isfinite(G).all()) and bool(torch.isfinite(loss).all())
        Gp, _, pp = run_ovr(k, dev, c, top_k, order=perm)
        assert torch.equal(Gp, G[perm]) and torch.equal(pp, pred[perm])


# ---- 7. / 8. the gradient kernels --------------------------------------------------------------------------------------------
def chunks(n):
    return [(a, min(a + CHUNK, n)) for a in range(0, n, CHUNK)]


def widen(Z):
    """The table as the gradient kernels stage it: in the accumulate dtype (bf16 -> f32 is exact)."""
    return Z.to(_hip.acc_dtype(Z.dtype))


def transposed_dots(k, dev, Aop, Zg):
    """Per 2048-row chunk of the contraction index: anchor_dots(Aop_chunk^T, Zg_chunk^T) -- [nO, d] dots whose k runs over
    the chunk's rows.  The A operand is what the kernel stages as A (accumulate dtype: the f32 / f64 instance)."""
    return [anchor_dots(k, Aop[a:b].T.contiguous(), Zg[a:b].T.contiguous(), dev) for a, b in chunks(Aop.shape[0])]


def sum_in_order(parts):
    s = torch.zeros_like(parts[0])
    for p in parts:
        s = s + p
    return s


def expect_probe_grad(chunk_dots, G):
    """dW = the chunks' dots added in chunk order; db: per chunk the sequential sum of the even rows plus that of the odd
    rows (Db[0] + Db[1] of probe_grad_kernel), the chunks added in order.  All in the accumulate dtype."""
    parts = []
    for a, b in chunks(G.shape[0]):
        even, odd = torch.zeros_like(G[0]), torch.zeros_like(G[0])
        for i in range(a, b, 2):
            even = even + G[i]
        for i in range(a + 1, b, 2):
            odd = odd + G[i]
        parts.append(even + odd)
    return sum_in_order(chunk_dots), sum_in_order(parts)


def assert_probe_grad(dW, db, chunk_dots, G):
    want_W, want_b = expect_probe_grad(chunk_dots, G)
    assert torch.equal(dW, want_W), ("probe_grad dW", int((dW != want_W).sum()))
    assert torch.equal(db, want_b), ("probe_grad db", int((db != want_b).sum()))


def check_probe_grad(k, dev, dtype, d, n):
    acc = _hip.acc_dtype(dtype)
    K = GRAD_CF[1] * _hip.probe_padded_classes(GRAD_CF[0])
    Z, rows = table(11, d, dtype), row_list(12, n)
    G = randn(17, (n, K), acc, 0.5)
    ws = torch.full((k.probe_grad_ws_len(n, K, d),), float("nan"), dtype=acc, device=dev)
    dW = torch.full((K, d), float("nan"), dtype=acc, device=dev)
    db = torch.full((K,), float("nan"), dtype=acc, device=dev)
    k.probe_grad(place(Z, dev), d, rows.to(dev), G.to(dev).view(-1), ws, dW.view(-1), db)
    assert_probe_grad(dW.cpu(), db.cpu(), transposed_dots(k, dev, G, gather(widen(Z), rows)), G)


def expect_pair_grad(top_dots, bottom_dots, M=GRAD_M):
    return torch.cat([sum_in_order(top_dots), sum_in_order(bottom_dots)]) / M


def assert_pair_grad(dW, top_dots, bottom_dots):
    want = expect_pair_grad(top_dots, bottom_dots)
    d = want.shape[1]
    assert torch.equal(dW[:d], want[:d]), ("pair_grad dW, rows of Phi_src", int((dW[:d] != want[:d]).sum()))
    assert torch.equal(dW[d:], want[d:]), ("pair_grad dW, rows of Phi_dst", int((dW[d:] != want[d:]).sum()))


def check_pair_grad(k, dev, dtype, d, B):
    acc = _hip.acc_dtype(dtype)
    Z, src, dst = table(1, d, dtype), row_list(5, B), row_list(6, B)
    PA, PB, g = randn(7, (B, d), acc), randn(8, (B, d), acc), randn(9, (B,), acc, 0.5)
    ws = torch.full((k.pair_grad_ws_len(B, d),), float("nan"), dtype=acc, device=dev)
    dW = torch.full((2 * d, d), float("nan"), dtype=acc, device=dev)
    k.pair_grad(place(Z, dev), d, src.to(dev), dst.to(dev), PA.to(dev).view(-1), PB.to(dev).view(-1), g.to(dev),
                torch.tensor([0.0, GRAD_M], dtype=torch.float64, device=dev), ws, dW.view(-1))
    Zw = widen(Z)
    # the A operand the kernel forms: g_k times the projected row, one rounding in the accumulate dtype
    top = transposed_dots(k, dev, g[:, None] * PB, gather(Zw, src))
    bottom = transposed_dots(k, dev, g[:, None] * PA, gather(Zw, dst))
    assert_pair_grad(dW.cpu(), top, bottom)


# ---- two summation orders on the CPU (the host file's mutation and order-sensitivity checks) ----------------------------------
def slice_order(d):
    """The k of mfma_slice's documented steps in sequence: k = 16 s + 4 g + kk, slices outermost, then kk, then g."""
    ks = [16 * s + 4 * g + kk for s in range(-(-d // 16)) for kk in range(4) for g in range(4)]
    return [x for x in ks if x < d]


def cpu_dots(A, B, order):
    """[nA, nB] dots in the accumulate dtype of B, the k terms added one at a time in `order` (a multiply, then an add:
    two roundings -- a model of AN order, not of the matrix cores)."""
    A = A.to(B.dtype)
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=B.dtype)
    for kk in order:
        acc = acc + A[:, kk, None] * B[None, :, kk]
    return acc


def ascending(A, B):
    return cpu_dots(A, B, range(A.shape[1]))


def descending(A, B):
    return cpu_dots(A, B, range(A.shape[1] - 1, -1, -1))
