"""Row-softmax cases with an exact answer -- helpers of tests/test_gpu_softmax_exact.py (the HIP kernels) and
tests/test_softmax_exact_host.py (the same checks through the CPU test double, plus the fixtures' self-checks).

The recipe: every vertex v has a level s_v and the table row z_v = s_v * a + b, with a and b 0/1 patterns on disjoint
coordinates spread over the whole width (a: the even coordinates, b: the odd ones).  Then z_r . z_c = s_r s_c |a| + |b|,
and with s in {-30, 0, 30} (or {30, 60}, or {30, 60, 120} with a few -30 / 0: all exact in bf16) the scores of a row
lie on levels at least 900 apart -- or are all equal (s_r = 0).  exp(level - max) is exactly 1 on the top level and
exactly 0 below it (exp(-900) underflows in fp32 and in fp64), so every partial sum is a small integer, every rescale
factor exp(run_m - new_m) is exactly 0 or 1,
and the soft-maxed row must be 1 / c, rounded once in the accumulate type, on the c edges of its top level and 0.0
everywhere else -- whatever the chunking, the wave slices, the slot order or row_parts.  The scores themselves are integer
dots below 2^24, which tests/exact_cases.py proves exact through CLANE_SCORE_RAW_DOT.  Expectations are COUNTED from the
int64 dots; no softmax routine is involved.  In fp32 1/c != 1/(c - 1) for every c the graphs hold, so one lost or
double-counted top-level edge always moves a bit.

Every check takes the kernel object and the device: HipKernels on the card, the oracle-backed double on the host.
Nothing in the exact checks has a tolerance.

The one real-valued check (`check_real_*`): integer scores in [-40, 40], so the dots stay exact and only exp, sum and
divide can err; every edge is compared with the correctly rounded fp64 value of the true softmax (50-digit decimal
arithmetic over the at most 81 distinct scores of a row) by its own relative error.  The bound is 4 x the worst
element-wise relative error of torch.softmax, run on the CPU in the accumulate type on these same scores (both graphs,
every REAL_CASES / REAL_PAIR_CASES width, sorted and class order, degrees 1 to 5000; `torch_softmax_worst_error` below
re-measures it; the worst rows are the 2049- and 5000-edge hubs, the 700-row graph alone gives 2.4 and 5.1):
    fp32: 4.15 eps (eps = 2^-23)  ->  bound 16.6 eps          fp64: 27.5 eps (eps = 2^-52)  ->  bound 110 eps
(the chunked evaluation adds one rescale multiply and one more fold per level to what torch does).
"""
import contextlib
import decimal
import functools
import math

import numpy as np
import torch

from clane_amd import _hip
from clane_amd.partition import HostCSR
from clane_amd.xcd import class_items, xcd_class

from . import exact_cases as E
from .exact_cases import BF16, F32, F64, SENTINEL, case_id, place, to_dev
from .test_gpu_parity import ragged_csr

TORCH_SOFTMAX_WORST_EPS = {F32: 4.15, F64: 27.5}         # measured, in units of torch.finfo(dtype).eps
REAL_BOUND_EPS = {t: 4 * v for t, v in TORCH_SOFTMAX_WORST_EPS.items()}
EPS = {F32: torch.finfo(F32).eps, F64: torch.finfo(F64).eps}

LEVEL_GAP = 900                                          # exp(-900) == 0 in fp32 and fp64 (the fp64 cut-off is about -745)
BIG_V, BIG_HUBS = 6000, (1025, 2049, 5000)               # a wave of the 16-wave kernels takes a 2nd / 3rd / 5th chunk
GRAPHS = ("small", "big")
ASSIGNMENTS = ("thirds", "last", "middle", "random")
ROW_PARTS = (1, 2, 7, 64, 255)
ROW_BLOCK = (5, 300)                                     # row0, rows: holds hubs of both graphs
# one d per lane layout (exact_cases.LAYOUT_CASES) on the 700-row graph; a cut of them on the 6000-row one
BIG_CASES = [(F32, 128, True), (F32, 300, True), (BF16, 64, True), (BF16, 520, True), (F64, 16, True), (F64, 130, True),
             (F32, 13, False), (BF16, 70, False), (F64, 3, False)]
CLASS_CASES = [(F32, 128, True), (F32, 300, True), (BF16, 256, True), (F64, 32, True), (F32, 13, False), (BF16, 3, False)]
PAIR_CASES = [(F32, 64), (F32, 300), (F32, 13), (F64, 32), (F64, 130), (F64, 3)]     # lds = ldn = 2d: d = 13 / 3 unaligned
REAL_CASES = [(F32, 128, True), (F32, 300, True), (BF16, 64, True), (F64, 32, True), (F32, 13, False)]
REAL_PAIR_CASES = [(F32, 64), (F32, 13), (F64, 64), (F64, 13)]
# clane_segment_softmax_*: (min_degree, max_degree, the rows listed)
SEGMENT_SETTINGS = {
    "defaults": (0, 0, None), "min1": (1, 0, None), "min64": (64, 0, None),
    "max64_long_listed": (0, 64, "above_max"), "min1_max64_long_listed": (1, 64, "above_max"),
    "min64_max128_long_listed": (64, 128, "above_max"),
    "max64_longest_row_not_listed": (0, 64, "above_max_but_longest"),
    "max_equals_min": (64, 64, "above_max"), "max_below_min": (64, 48, "above_max"),
}


# ---- the graphs ----------------------------------------------------------------------------------------------------
class Rows:
    """A CSR with sorted rows (`sorted_colidx`) and the same with the rows above exact_cases.CLASS_DEGREE edges in class
    order (`colidx`, what the class routes need)."""

    def __init__(self, rowptr, sorted_colidx):
        self.V = rowptr.size - 1
        self.rowptr, self.sorted_colidx = rowptr, sorted_colidx
        self.deg = np.diff(rowptr)
        self.E = int(rowptr[-1])
        self.class_rows = np.nonzero(self.deg > E.CLASS_DEGREE)[0]
        colidx = sorted_colidx.copy()
        for r in self.class_rows:
            a, b = rowptr[r], rowptr[r + 1]
            c = colidx[a:b]
            colidx[a:b] = c[np.lexsort((c, xcd_class(c)))]
        self.colidx = colidx
        self.row_of_edge = np.repeat(np.arange(self.V), self.deg)
        self.longest = int(np.argmax(self.deg))

    def columns(self, order):
        return self.sorted_colidx if order == "sorted" else self.colidx

    @functools.lru_cache(maxsize=None)
    def items(self, chunk):
        return class_items(self.rowptr, self.colidx, self.class_rows, chunk, 8)

    def rows_above(self, degree):
        return np.nonzero(self.deg > degree)[0].astype(np.int32)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "small":                                  # exact_cases.graph(): 700 rows, degrees 0, 1, 63 ... 650, 700
        g = E.graph()
        rows = Rows(g.rowptr, g.sorted_colidx)
        assert np.array_equal(rows.colidx, g.colidx)
        return rows
    csr = ragged_csr(BIG_V, seed=23, max_deg=12, hubs=BIG_HUBS)
    rows = Rows(csr.rowptr, csr.colidx)
    assert set(BIG_HUBS) <= set(rows.deg.tolist()) and (rows.deg == 0).sum() > 500 and rows.class_rows.size == 3
    return rows


# ---- the levels and the tables -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def levels(gname, assignment):
    """s_v by vertex id.  Columns are sorted inside a row (inside a class segment of a class row), so the vertex id
    places the maximum:
      thirds -- 30 / 60 / 120 by thirds of the id range, ascending: a row with s_r > 0 meets a new maximum region by
                region.  In a symmetric form a row's own level is always on its top level, and the hubs have low ids, so
                the rows above 48 edges are set by hand, by falling degree: as their id says / -30, and their first
                column with them (the few columns of that level have low ids: the maximum arrives in the first chunk
                and never again) / 0 (all equal);
      last   -- 60 on the last column of the longest hub alone, 30 elsewhere: the hub's single maximum is the last edge
                of its last chunk, the rows without that column are all equal;
      middle -- 60 only on the 64 columns of one middle chunk of the longest hub;
      random -- seeded -30 / 0 / 30: ties spread over all waves and slots."""
    g = graph(gname)
    hub = g.sorted_colidx[g.rowptr[g.longest]:g.rowptr[g.longest + 1]]
    if assignment == "thirds":
        s = 30 << (np.arange(g.V) * 3 // g.V)
        by_degree = g.rows_above(48)[np.argsort(-g.deg[g.rows_above(48)], kind="stable")]
        s[g.sorted_colidx[g.rowptr[by_degree[1::3]]]] = -30
        s[by_degree[1::3]], s[by_degree[2::3]] = -30, 0
    elif assignment == "last":
        s = np.full(g.V, 30)
        s[hub[-1]] = 60
    elif assignment == "middle":
        s = np.full(g.V, 30)
        m = hub.size // 64 // 2
        s[hub[64 * m:64 * m + 64]] = 60
    else:
        s = np.random.default_rng(41).integers(-1, 2, size=g.V) * 30
    return s.astype(np.int64)


@functools.lru_cache(maxsize=None)
def row_levels(gname):
    """The pair kernels' source table carries levels of its own, independent of the neighbour table's."""
    return np.random.default_rng(43).integers(-1, 2, size=graph(gname).V).astype(np.int64) * 30


def level_table(s, d):
    """[V, d] int64: s_v on the even coordinates (a), 1 on the odd ones (b)."""
    a = (np.arange(d) % 2 == 0).astype(np.int64)
    return s[:, None] * a[None, :] + (1 - a)[None, :]


def int_dots(g, colidx, S, N):
    """int64 dot of S[row] and N[col] for every edge."""
    out = np.empty(g.E, dtype=np.int64)
    step = max(1, (1 << 22) // S.shape[1])
    for a in range(0, g.E, step):
        out[a:a + step] = (S[g.row_of_edge[a:a + step]] * N[colidx[a:a + step]]).sum(1)
    return out


def count_expectation(g, dots, acc):
    """From the int64 scores of every edge, by counting: (expected softmax in `acc`, top-level mask, row maximum per
    edge).  Asserts the range condition: inside a row every score is the maximum or at least LEVEL_GAP below it, and
    everything stays an exact integer of the accumulate type."""
    assert int(np.abs(dots).max()) < (1 << 24)
    full = g.deg > 0
    rowmax = np.zeros(g.V, dtype=np.int64)
    rowmax[full] = np.maximum.reduceat(dots, g.rowptr[:-1][full])
    edge_max = rowmax[g.row_of_edge]
    top = dots == edge_max
    assert bool((edge_max[~top] - dots[~top] >= LEVEL_GAP).all())
    count = np.bincount(g.row_of_edge[top], minlength=g.V)
    assert bool((count[full] >= 1).all())
    want = torch.ones(g.E, dtype=acc) / torch.from_numpy(count[g.row_of_edge]).to(acc)        # rounded once
    want[torch.from_numpy(~top)] = 0.0
    return want, top, edge_max


class Levelled:
    """Tables, int64 scores and counted expectations of one (graph, assignment, d); `pair`: two tables, the source one
    with row_levels().  Host data; nobody writes to it."""

    def __init__(self, gname, assignment, d, pair=False):
        self.g, self.d = graph(gname), d
        self.N = level_table(levels(gname, assignment), d)
        self.S = level_table(row_levels(gname), d) if pair else self.N
        bound = int(np.abs(self.S).max()) * int(np.abs(self.N).max()) * ((d + 1) // 2) + d // 2
        assert bound < (1 << 24), (gname, assignment, d)                 # the range condition: 900 |a| + |b| and above
        self._cache = {}

    def table(self):
        return torch.from_numpy(self.N).double()

    def pair_table(self):
        return torch.from_numpy(np.concatenate([self.S, self.N], axis=1)).double()

    def dots(self, order):
        if order not in self._cache:
            self._cache[order] = int_dots(self.g, self.g.columns(order), self.S, self.N)
        return self._cache[order]

    def want(self, order, acc):
        if (order, acc) not in self._cache:
            self._cache[order, acc] = count_expectation(self.g, self.dots(order), acc)[0]
        return self._cache[order, acc]


@functools.lru_cache(maxsize=32)
def levelled(gname, assignment, d, pair=False):
    return Levelled(gname, assignment, d, pair)


# ---- comparing ---------------------------------------------------------------------------------------------------------
def check_edges(g, got, want, owned, tag, elsewhere=None):
    """The owned edges equal `want` bit for bit; the others hold `elsewhere` (default: the sentinel)."""
    got = got.cpu()[:g.E]
    own = torch.from_numpy(owned)
    wrong = np.unique(g.row_of_edge[((got != want) & own).numpy()])
    assert wrong.size == 0, (tag, "rows that differ (row, degree)", [(int(r), int(g.deg[r])) for r in wrong[:8]])
    other = torch.full_like(got, SENTINEL) if elsewhere is None else elsewhere
    assert torch.equal(got[~own], other[~own]), (tag, "an edge of a row the call does not own was written")


def slot_stats(g, it, dots, acc):
    """Counted {max, sum of exp} per slot: the slot's top level and how many of its edges sit on it."""
    n_slots = int(it["slot_ptr"][-1])
    want = torch.full((n_slots, 2), float("nan"), dtype=acc)
    for e0, ln, slot in zip(it["e0"], it["len"], it["slot"]):
        if ln > 0:
            part = dots[e0:e0 + ln]
            want[slot, 0], want[slot, 1] = float(part.max()), float((part == part.max()).sum())
    assert not bool(torch.isnan(want).any())
    return want


# ---- the fused routes --------------------------------------------------------------------------------------------------
def _row_calls(g, dev, acc, want, score, tag, check=check_edges):
    """The launches of one fused K1 entry point over sorted rows: every row by one (sub-)wave; the rows above 48 edges
    listed as long rows; a row block with row0 > 0, without and with its long rows listed.  Returns the first result."""
    rp, ci = to_dev(g.rowptr, dev), to_dev(g.sorted_colidx, dev)
    fresh = lambda: torch.full((g.E,), SENTINEL, dtype=acc, device=dev)  # noqa: E731
    everything = np.ones(g.E, dtype=bool)
    long_rows = g.rows_above(48)
    whole = fresh()
    score(rp, ci, g.V, 0, whole)
    check(g, whole, want, everything, tag + " whole")
    s = fresh()
    score(rp, ci, g.V, 0, s, 48, to_dev(long_rows, dev))
    check(g, s, want, everything, tag + " long rows listed")
    r0, n = ROW_BLOCK
    block = (g.row_of_edge >= r0) & (g.row_of_edge < r0 + n)
    s = fresh()
    score(rp[r0:], ci, n, r0, s)
    check(g, s, want, block, tag + " row block")
    inside = long_rows[(long_rows >= r0) & (long_rows < r0 + n)] - r0
    assert inside.size >= 2
    s = fresh()
    score(rp[r0:], ci, n, r0, s, 48, to_dev(inside.astype(np.int32), dev))
    check(g, s, want, block, tag + " row block, long rows listed")
    return whole


def _class_calls(g, dev, acc, want, want_stats, chunk, score_class, tag, parts=ROW_PARTS, check=check_edges):
    it = g.items(chunk)
    n_slots = int(it["slot_ptr"][-1])
    args = (to_dev(g.rowptr, dev), to_dev(g.colidx, dev), *(to_dev(it[key], dev) for key in ("e0", "len", "slot", "row")),
            8, to_dev(g.class_rows.astype(np.int32), dev), to_dev(it["slot_ptr"], dev), 0)
    listed = np.isin(g.row_of_edge, g.class_rows)
    for p in parts:
        scores = torch.full((g.E,), SENTINEL, dtype=acc, device=dev)
        stats = torch.full((2 * n_slots,), float("nan"), dtype=acc, device=dev)
        score_class(args, scores, stats, n_slots, p)
        check(g, scores, want, listed, f"{tag} chunk {chunk} row_parts {p}")
        if want_stats is not None:
            assert torch.equal(stats.cpu().view(-1, 2), want_stats), (tag, chunk, p, "stats")


def check_fused_rows(k, dev, gname, assignment, case):
    """edge_score with CLANE_SCORE_FUSE_SOFTMAX in RAW_DOT mode."""
    dtype, d, pad = case
    g, acc, L = graph(gname), _hip.acc_dtype(dtype), levelled(gname, assignment, d)
    Zd = place(L.table(), dtype, dev, pad)
    _row_calls(g, dev, acc, L.want("sorted", acc),
               lambda rp, ci, n, r0, s, T=0, lr=None: k.edge_score(rp, ci, n, r0, Zd, d, _hip.SCORE_RAW_DOT, None, None, s,
                                                                   T, lr, fuse_softmax=True),
               f"{gname} {assignment} {case_id(case)} edge_score")


def check_fused_class(k, dev, gname, assignment, case, chunk):
    """edge_score_class with CLANE_SCORE_FUSE_SOFTMAX: scores, untouched rows and the per-slot stats, for every
    row_parts."""
    dtype, d, pad = case
    g, acc, L = graph(gname), _hip.acc_dtype(dtype), levelled(gname, assignment, d)
    Zd = place(L.table(), dtype, dev, pad)
    _class_calls(g, dev, acc, L.want("class", acc), slot_stats(g, g.items(chunk), L.dots("class"), acc), chunk,
                 lambda a, s, st, ns, p: k.edge_score_class(*a, Zd, d, _hip.SCORE_RAW_DOT, None, None, s, st,
                                                            fuse_softmax=True, n_slots=ns, row_parts=p),
                 f"{gname} {assignment} {case_id(case)} edge_score_class")


def check_fused_pair(k, dev, gname, assignment, dtype, d):
    """edge_score_pair and edge_score_class_pair with the fused softmax (S = Y, N = Y + d, lds = ldn = 2d)."""
    g, L = graph(gname), levelled(gname, assignment, d, True)
    Yd = L.pair_table().to(dtype).to(dev)
    S, N = Yd[:, :d], Yd[:, d:]
    tag = f"{gname} {assignment} {_hip._SUFFIX[dtype]}-d{d}"
    _row_calls(g, dev, dtype, L.want("sorted", dtype),
               lambda rp, ci, n, r0, s, T=0, lr=None: k.edge_score_pair(rp, ci, n, r0, S, N, d, s, T, lr, fuse_softmax=True),
               tag + " edge_score_pair")
    for chunk in (64, 256):
        _class_calls(g, dev, dtype, L.want("class", dtype), slot_stats(g, g.items(chunk), L.dots("class"), dtype), chunk,
                     lambda a, s, st, ns, p: k.edge_score_class_pair(*a, S, N, d, s, st, fuse_softmax=True, n_slots=ns,
                                                                     row_parts=p),
                     tag + " edge_score_class_pair", parts=(1, 7))


# ---- K2 ------------------------------------------------------------------------------------------------------------------
def segment_owned_rows(g, min_degree, max_degree, listed):
    """The contract of include/clane_hip.h, restated: which rows a clane_segment_softmax_* call normalises."""
    one_wave = not (0 < max_degree <= min_degree)
    owned = (g.deg > min_degree) & ((max_degree == 0) | (g.deg <= max_degree)) & one_wave
    if listed is not None:
        owned[listed] |= g.deg[listed] > min_degree
    return owned


def segment_rows_listed(g, max_degree, which):
    if which is None:
        return None
    rows = g.rows_above(max_degree)
    return rows if which == "above_max" else rows[rows != g.longest]


def check_segment_softmax(k, dev, gname, assignment, dtype, setting):
    """segment_softmax on levelled values written directly (s_r s_c: |a| = 1, |b| = 0): the rows the call owns are the
    counted expectation, every other row -- an empty one has no edge -- keeps its raw values, and so does the tail of
    the buffer."""
    g = graph(gname)
    s = levels(gname, assignment)
    dots = s[g.row_of_edge] * s[g.sorted_colidx]
    want = count_expectation(g, dots, dtype)[0]
    raw = torch.from_numpy(dots).to(dtype)
    min_degree, max_degree, which = SEGMENT_SETTINGS[setting]
    listed = segment_rows_listed(g, max_degree, which)
    owned = segment_owned_rows(g, min_degree, max_degree, listed)[g.row_of_edge]
    if setting == "max64_longest_row_not_listed":
        assert not owned[g.row_of_edge == g.longest].any() and owned.sum() > g.E // 2
    if setting in ("max_equals_min", "max_below_min"):
        assert not owned[g.deg[g.row_of_edge] <= 64].any() and owned.any()
    vals = torch.cat([raw, torch.full((64,), SENTINEL, dtype=dtype)]).to(dev)
    k.segment_softmax(to_dev(g.rowptr, dev), g.V, vals, min_degree, max_degree, None if listed is None else to_dev(listed, dev))
    tag = f"{gname} {assignment} {_hip._SUFFIX[dtype]} segment_softmax {setting}"
    check_edges(g, vals, want, owned, tag, elsewhere=raw)
    assert bool((vals.cpu()[g.E:] == SENTINEL).all()), (tag, "written past the last edge")


def check_column_split_route(k, dev, gname, assignment, case):
    """RAW_DOT scores (long rows listed), edge_score_finalize -- a no-op in RAW_DOT mode --, then segment_softmax with
    the rows above 64 edges listed: the fused result, bit for bit, and the counted expectation."""
    dtype, d, pad = case
    g, acc, L = graph(gname), _hip.acc_dtype(dtype), levelled(gname, assignment, d)
    Zd = place(L.table(), dtype, dev, pad)
    rp, ci = to_dev(g.rowptr, dev), to_dev(g.sorted_colidx, dev)
    fused = torch.full((g.E,), SENTINEL, dtype=acc, device=dev)
    k.edge_score(rp, ci, g.V, 0, Zd, d, _hip.SCORE_RAW_DOT, None, None, fused, fuse_softmax=True)
    split = torch.full((g.E,), SENTINEL, dtype=acc, device=dev)
    k.edge_score(rp, ci, g.V, 0, Zd, d, _hip.SCORE_RAW_DOT, None, None, split, 48, to_dev(g.rows_above(48), dev))
    assert torch.equal(split.cpu(), torch.from_numpy(L.dots("sorted")).to(acc))
    k.edge_score_finalize(rp, ci, g.V, 0, _hip.SCORE_RAW_DOT, None, None, split)
    k.segment_softmax(rp, g.V, split, 0, 64, to_dev(g.rows_above(64), dev))
    tag = f"{gname} {assignment} {case_id(case)} column-split route"
    check_edges(g, split, L.want("sorted", acc), np.ones(g.E, dtype=bool), tag)
    assert torch.equal(split.cpu(), fused.cpu()), tag


# ---- the engine ------------------------------------------------------------------------------------------------------------
ENGINE_SETTINGS = {"long": {"class_threshold": 0, "long_threshold": 64}, "class": {"class_threshold": 32, "class_chunk": 64}}


def check_engine_bilinear(kernels, dev, gname, assignment, dtype, route, d=40):
    """SweepEngine.build_P_bilinear(W) with the integer X of the recipe and W = two stacked identities (A = Bm = X):
    P_global() is the counted expectation, and the engine took the route the setting is there for."""
    from clane_amd.engine import SweepEngine
    g, L = graph(gname), levelled(gname, assignment, d)
    X = L.table().to(dtype)
    W = torch.cat([torch.eye(d, dtype=torch.float64)] * 2).to(dtype)
    with torch.cuda.device(dev) if torch.device(dev).type == "cuda" else contextlib.nullcontext():
        eng = SweepEngine(HostCSR(g.V, g.rowptr, g.sorted_colidx), X, dev, kernels, **ENGINE_SETTINGS[route])
        if route == "long":
            assert any(lr is not None and lr.numel() > 0 for lr in eng.k1_long_rows)
            assert not any(c is not None for c in eng.class_rows)
        else:
            assert eng.class_k1 and any(c is not None for c in eng.class_rows)
        eng.build_P_bilinear(W)
        got, want = eng.P_global(), L.want("sorted", dtype)
    wrong = np.unique(g.row_of_edge[(got != want).numpy()])
    assert wrong.size == 0, (gname, assignment, dtype, route, [(int(r), int(g.deg[r])) for r in wrong[:8]])


# ---- the real-valued, element-wise check -----------------------------------------------------------------------------------
def real_table(V, d, seed):
    """Integer rows whose dots lie in [-32, 36]: p, q in [-4, 4] on the first and the last coordinate, ones on up to
    four coordinates in between."""
    rng = np.random.default_rng(seed)
    Z = np.zeros((V, d), dtype=np.int64)
    Z[:, 0], Z[:, d - 1] = rng.integers(-4, 5, size=V), rng.integers(-4, 5, size=V)
    Z[:, np.unique(np.linspace(1, d - 2, min(4, d - 2)).astype(int))] = 1
    return Z


@functools.lru_cache(maxsize=None)
def _exp_table():
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        return [decimal.Decimal(-j).exp() for j in range(81)]


def true_softmax(g, dots):
    """Correctly rounded fp64 softmax of integer scores in [-40, 40], row by row, in 50-digit arithmetic."""
    assert int(dots.min()) >= -40 and int(dots.max()) <= 40
    T = _exp_table()
    out = np.zeros(g.E, dtype=np.float64)
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        for r in np.nonzero(g.deg)[0]:
            x = dots[g.rowptr[r]:g.rowptr[r + 1]]
            below = int(x.max()) - x
            cnt = np.bincount(below, minlength=81)
            den = sum(int(cnt[j]) * T[j] for j in np.nonzero(cnt)[0])
            lut = np.zeros(81)
            for j in np.nonzero(cnt)[0]:
                lut[j] = float(T[j] / den)
            out[g.rowptr[r]:g.rowptr[r + 1]] = lut[below]
    return out


class RealCase:
    def __init__(self, gname, d, pair=False):
        self.g = g = graph(gname)
        self.N = real_table(g.V, d, 50 + d)
        self.S = real_table(g.V, d, 51 + d) if pair else self.N
        self.dots = {o: int_dots(g, g.columns(o), self.S, self.N) for o in ("sorted", "class")}
        self.ref = {o: true_softmax(g, x) for o, x in self.dots.items()}


@functools.lru_cache(maxsize=16)
def real_case(gname, d, pair=False):
    return RealCase(gname, d, pair)


def worst_relative_error(got, ref):
    got = got.double().numpy()
    return float((np.abs(got - ref) / ref).max())


def torch_softmax_worst_error(acc, g, dots, ref):
    """Worst element-wise relative error of torch.softmax on the CPU in `acc`, in units of eps."""
    worst = 0.0
    x = torch.from_numpy(dots).to(acc)
    for r in np.nonzero(g.deg)[0]:
        a, b = g.rowptr[r], g.rowptr[r + 1]
        worst = max(worst, worst_relative_error(torch.softmax(x[a:b], 0), ref[a:b]))
    return worst / EPS[acc]


def check_real(g, got, ref, owned, tag, elsewhere=None):
    """Every owned edge within REAL_BOUND_EPS of the true softmax, relatively; every owned row's sum within deg * eps
    of 1 (summed exactly); the other edges untouched."""
    acc = got.dtype
    got = got.cpu()[:g.E]
    own = torch.from_numpy(owned)
    err = np.where(owned, np.abs(got.double().numpy() - ref) / ref, 0.0)
    worst = int(np.argmax(err))
    assert err[worst] <= REAL_BOUND_EPS[acc] * EPS[acc], (
        tag, "relative error in eps", err[worst] / EPS[acc], "row, degree", int(g.row_of_edge[worst]),
        int(g.deg[g.row_of_edge[worst]]))
    values = got.double().tolist()
    for r in np.unique(g.row_of_edge[owned]):
        total = math.fsum(values[g.rowptr[r]:g.rowptr[r + 1]])
        assert abs(total - 1.0) <= int(g.deg[r]) * EPS[acc], (tag, "row sum", int(r), int(g.deg[r]), total)
    other = torch.full_like(got, SENTINEL) if elsewhere is None else elsewhere
    assert torch.equal(got[~own], other[~own]), (tag, "an edge of a row the call does not own was written")


def check_real_rows(k, dev, gname, case):
    """Families row and long: edge_score fused, whole rows by one (sub-)wave and long rows listed at 48."""
    dtype, d, pad = case
    g, acc, c = graph(gname), _hip.acc_dtype(dtype), real_case(gname, d)
    Zd = place(torch.from_numpy(c.N).double(), dtype, dev, pad)
    _row_calls(g, dev, acc, c.ref["sorted"],
               lambda rp, ci, n, r0, s, T=0, lr=None: k.edge_score(rp, ci, n, r0, Zd, d, _hip.SCORE_RAW_DOT, None, None, s,
                                                                   T, lr, fuse_softmax=True),
               f"{gname} {case_id(case)} edge_score", check=check_real)


def check_real_class(k, dev, gname, case):
    """Family class + rescale: chunk 64 and 256, row_parts 1 and 7."""
    dtype, d, pad = case
    g, acc, c = graph(gname), _hip.acc_dtype(dtype), real_case(gname, d)
    Zd = place(torch.from_numpy(c.N).double(), dtype, dev, pad)
    for chunk in (64, 256):
        _class_calls(g, dev, acc, c.ref["class"], None, chunk,
                     lambda a, s, st, ns, p: k.edge_score_class(*a, Zd, d, _hip.SCORE_RAW_DOT, None, None, s, st,
                                                                fuse_softmax=True, n_slots=ns, row_parts=p),
                     f"{gname} {case_id(case)} edge_score_class", parts=(1, 7), check=check_real)


def check_real_segment_softmax(k, dev, gname, dtype):
    """Family segment_softmax: the scores written directly; the defaults, and the rows above 64 edges listed."""
    g, c = graph(gname), real_case(gname, 13)
    raw = torch.from_numpy(c.dots["sorted"]).to(dtype)
    for min_degree, max_degree, which in ((0, 0, None), (0, 64, "above_max"), (1, 64, "above_max")):
        listed = segment_rows_listed(g, max_degree, which)
        owned = segment_owned_rows(g, min_degree, max_degree, listed)[g.row_of_edge]
        vals = raw.clone().to(dev)
        k.segment_softmax(to_dev(g.rowptr, dev), g.V, vals, min_degree, max_degree,
                          None if listed is None else to_dev(listed, dev))
        check_real(g, vals, c.ref["sorted"], owned, f"{gname} {dtype} segment_softmax {min_degree} {max_degree}", elsewhere=raw)


def check_real_pair(k, dev, gname, dtype, d):
    """Family pair: edge_score_pair (whole, long rows listed, row blocks) and edge_score_class_pair."""
    g, c = graph(gname), real_case(gname, d, True)
    Yd = torch.from_numpy(np.concatenate([c.S, c.N], axis=1)).to(dtype).to(dev)
    S, N = Yd[:, :d], Yd[:, d:]
    tag = f"{gname} {_hip._SUFFIX[dtype]}-d{d}"
    _row_calls(g, dev, dtype, c.ref["sorted"],
               lambda rp, ci, n, r0, s, T=0, lr=None: k.edge_score_pair(rp, ci, n, r0, S, N, d, s, T, lr, fuse_softmax=True),
               tag + " edge_score_pair", check=check_real)
    _class_calls(g, dev, dtype, c.ref["class"], None, 64,
                 lambda a, s, st, ns, p: k.edge_score_class_pair(*a, S, N, d, s, st, fuse_softmax=True, n_slots=ns,
                                                                 row_parts=p),
                 tag + " edge_score_class_pair", parts=(1, 7), check=check_real)
