"""Integer-data cases whose every intermediate is exactly representable -- helpers of tests/test_gpu_exact.py (the HIP
kernels) and tests/test_exact_host.py (the same checks through the CPU test double, plus the fixtures' self-checks).

The recipe: Z_old entries are non-zero integers in [-4, 4] (a dropped edge always changes something), X integers in
[-8, 8], P[e] = m/4 with m in 1..8, gamma = 0.5; for projections and gradients W, A, Bm are integers in [-3, 3], g in
[-2, 2] and M = stats[1] a power of two.  Every partial sum of a sweep is then a multiple of 1/8 bounded by
0.5 * sum|P z| + 8; as long as that bound times 8 stays below 2^24 no fp32 (let alone fp64) accumulator ever rounds, so
summation order, FMA contraction and tiling cannot move a bit: a kernel must be torch.equal to the fp64 oracle's result
rounded ONCE, round-to-nearest-even, to the storage dtype (Elem<bf16_t>::from_acc and Tensor.to(torch.bfloat16) both
are).  The expected L1 delta is the sum over the STORED values (the kernels' shared epilogue, finish_pack, uses them),
exact as well.  `K3Case` asserts the range condition for every case it builds.

Every check takes the kernel object and the device: HipKernels on the card, the oracle-backed double on the host.
Nothing here has a tolerance.
"""
import functools

import numpy as np
import torch

from clane_amd import _hip
from clane_amd.xcd import class_items, xcd_class
from oracle import clane_oracle as O

from .test_gpu_parity import padded, ragged_csr

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
GAMMA = 0.5
V = 700
HUBS = (1, 63, 64, 65, 127, 128, 129, 300, 650, 700)      # the edges of the 64-aligned wave slices, full-width hubs
CLASS_DEGREE = 100                                         # rows above it take the class routes
EXACT_LIMIT = float(1 << 24)                               # integers an fp32 accumulator holds exactly

# (dtype, d, padded): one d per lane layout pick_layout / dispatch_layout (csrc/clane_abi.hip) can choose -- 16-byte
# packs over 8 / 16 / 32 / 64 lanes, then one that needs a second pass over the 64 lanes -- and the one-element-per-lane
# layouts (4 / 16 / 64 lanes) through an odd, unpadded leading dimension.
LAYOUT_CASES = ([(F32, d, True) for d in (32, 64, 128, 300)] + [(BF16, d, True) for d in (64, 128, 256, 520)]
                + [(F64, d, True) for d in (16, 32, 64, 130)]
                + [(t, d, False) for t in (F32, BF16, F64) for d in (3, 13, 70)])
K1_CASES = LAYOUT_CASES + [(t, 1433, True) for t in (F32, BF16, F64)]          # |dot| <= 16 * 1433
# clane_spmm_update_*: the flags x thresholds of the row pass, the 4- and 16-wave long rows, split hubs, class chunks
ROUTES = ("row_t0", "row_t0_sinks", "row_t48_long4", "row_t48_sinks_long16", "split64", "split128",
          "class64", "class64_beyond", "class256", "class256_beyond")
BEYOND_ROW_CASES = [(F32, 128, True)]       # where CLANE_SPMM_TABLE_BEYOND_CACHE selects another row-pass instance
SENTINEL = float((1 << 20) + 0.5)           # no score of these cases: they are integers below 2^15


def case_id(case):
    dtype, d, pad = case
    return f"{_hip._SUFFIX[dtype]}-d{d}-{'padded' if pad else 'scalar'}"


# ---- the recipe ----------------------------------------------------------------------------------------------------
def nonzero_ints(rng, shape, hi):
    return torch.from_numpy(rng.integers(1, hi + 1, size=shape) * rng.choice(np.array([-1, 1]), size=shape)).double()


def ints(rng, shape, hi):
    return torch.from_numpy(rng.integers(-hi, hi + 1, size=shape)).double()


def leading_dimension(dtype, d, pad):
    if pad:
        return -(-d // _hip.VEC_ELEMS[dtype]) * _hip.VEC_ELEMS[dtype]
    return d if d % 2 else d + 1                      # odd: never the 16-byte path, whatever the dtype


def place(t, dtype, dev, pad):
    """[rows, d] host values -> [rows, ld] device table of `dtype` with zero pad columns."""
    return padded(t, dtype, dev, leading_dimension(dtype, t.shape[1], pad))


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- the graph -----------------------------------------------------------------------------------------------------
class ExactGraph:
    """ragged_csr(700, hubs = HUBS): empty rows, ragged rows, hubs.  `colidx` has the rows above CLASS_DEGREE edges in
    class order (what the class routes need; the others take any order), `sorted_colidx` is the sorted original."""

    def __init__(self):
        csr = ragged_csr(V, seed=17, hubs=HUBS)
        self.rowptr, self.sorted_colidx = csr.rowptr, csr.colidx
        self.deg = np.diff(csr.rowptr)
        self.E = int(csr.num_edges)
        self.class_rows = np.nonzero(self.deg > CLASS_DEGREE)[0]
        colidx = csr.colidx.copy()
        for r in self.class_rows:
            a, b = csr.rowptr[r], csr.rowptr[r + 1]
            c = colidx[a:b]
            colidx[a:b] = c[np.lexsort((c, xcd_class(c)))]
        self.colidx = colidx
        self.row_of_edge = np.repeat(np.arange(V), self.deg)
        self.sink = torch.from_numpy(self.deg == 0)
        assert self.deg.max() == V and (self.deg == 0).sum() > 50 and self.class_rows.size >= 6
        # further destinations of finished rows, as tests/test_gpu_parity.py::test_spmm_mirror_packs_send_buffer lays
        # them out: 0..3 places per row with edges, 8..12 for a tenth, the long rows at least one; two buffers
        rng = np.random.default_rng(0)
        copies = np.where(self.deg > 0, rng.integers(0, 4, V), 0)
        many = (rng.random(V) < 0.1) & (self.deg > 0)
        copies[many] = rng.integers(8, 13, int(many.sum()))
        copies[self.deg > 48] = np.maximum(copies[self.deg > 48], 1)
        self.rows_of_slot = rng.permutation(np.repeat(np.arange(V), copies))
        order = np.argsort(self.rows_of_slot, kind="stable").astype(np.int32)
        self.mirror_row_ptr = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(copies, out=self.mirror_row_ptr[1:])
        self.mirror_place = (((order % 2) << _hip.MIRROR_ROW_BITS) | (order // 2)).astype(np.int32)

    @functools.lru_cache(maxsize=None)
    def items(self, chunk):
        return class_items(self.rowptr, self.colidx, self.class_rows, chunk, 8)

    @functools.lru_cache(maxsize=None)
    def segments(self, seg):
        rows = np.nonzero(self.deg > seg)[0].astype(np.int32)
        nseg = -(-self.deg[rows] // seg)
        seg_ptr = np.zeros(rows.size + 1, dtype=np.int64)
        np.cumsum(nseg, out=seg_ptr[1:])
        return rows, seg_ptr, np.repeat(np.arange(rows.size, dtype=np.int32), nseg)


@functools.lru_cache(maxsize=None)
def graph():
    return ExactGraph()


# ---- K3 ------------------------------------------------------------------------------------------------------------
class K3Case:
    """Inputs and exact expectations of one sweep over graph() at (dtype, d).  Host tensors; nobody writes to them."""

    def __init__(self, dtype, d, pad):
        g = graph()
        rng = np.random.default_rng(1000 + d)
        self.dtype, self.d, self.pad, self.acc = dtype, d, pad, _hip.acc_dtype(dtype)
        self.Zold = nonzero_ints(rng, (V, d), 4)
        self.X = ints(rng, (V, d), 8)
        self.P = torch.from_numpy(rng.integers(1, 9, size=g.E)).double() / 4
        # the condition for exactness: every partial sum is a multiple of 1/8 within this bound, a row's L1 delta
        # (summed in the accumulate type) a multiple of 1/8 within d * (bound + 4)
        self.bound = float((GAMMA * torch.sparse.mm(O.as_sparse(g.rowptr, g.colidx, self.P), self.Zold.abs()) + 8).max())
        assert self.bound * 8 < EXACT_LIMIT and d * (self.bound + 4) * 8 < EXACT_LIMIT, (dtype, d, self.bound)
        ref, _ = O.sweep(g.rowptr, g.colidx, self.P, self.X, self.Zold, GAMMA)
        assert float((ref * 8 - (ref * 8).round()).abs().max()) == 0 and float(ref.abs().max()) <= self.bound
        self.ref64 = ref
        self.expect = ref.to(dtype)                                   # rounded once, to nearest even
        assert self.Zold.to(dtype).double().equal(self.Zold) and self.X.to(dtype).double().equal(self.X)
        self.row_delta = (self.expect.double() - self.Zold).abs().sum(1)          # of the stored values
        self.delta = float(self.row_delta.sum())
        assert float(self.row_delta[g.sink].sum()) == 0 and self.expect[g.sink].double().equal(self.Zold[g.sink])

    def undetected_single_edge_drops(self, limit=600):
        """Of the first `limit` edges of the longest row: how many could vanish from the sum without changing the
        expected row in the storage dtype."""
        g = graph()
        r = int(np.argmax(g.deg))
        a = int(g.rowptr[r])
        n = min(int(g.deg[r]), limit)
        cols = torch.from_numpy(g.colidx[a:a + n].astype(np.int64))
        without = self.ref64[r].unsqueeze(0) - GAMMA * self.P[a:a + n].unsqueeze(1) * self.Zold[cols]
        changed = (without.to(self.dtype) != self.expect[r].unsqueeze(0)).any(1)
        return n, int((~changed).sum())


@functools.lru_cache(maxsize=None)
def k3_case(dtype, d, pad):
    return K3Case(dtype, d, pad)


def routes_of(case):
    return ROUTES + (("row_t0_beyond",) if case in BEYOND_ROW_CASES else ())


def check_k3_route(k, dev, case, route):
    """One whole sweep by `route` (its listed rows by the long / split / class kernel, the rest by the row pass), every
    call with the mirror on: table, pad columns, sinks, mirror buffers and the reduced delta, all exact."""
    g, c = graph(), k3_case(*case)
    d, dtype, acc, tag = c.d, c.dtype, c.acc, f"{case_id(case)} {route}"
    rp, ci, P = to_dev(g.rowptr, dev), to_dev(g.colidx, dev), c.P.to(acc).to(dev)
    Xd, Zo = place(c.X, dtype, dev, c.pad), place(c.Zold, dtype, dev, c.pad)
    ld = Zo.shape[1]
    sinks_untouched = "sinks" in route or route.startswith(("split", "class"))
    Zn = torch.full_like(Zo, float("nan"))
    Zn[:, d:] = 0
    if sinks_untouched:                              # the caller's side of CLANE_SPMM_SINKS_UNTOUCHED
        Zn[g.sink.to(dev)] = Zo[g.sink.to(dev)]
    buf = torch.full((2, (g.rows_of_slot.size + 1) // 2, ld), 7.0, dtype=dtype, device=dev)
    mir = k.make_mirror(to_dev(g.mirror_row_ptr, dev), to_dev(g.mirror_place, dev), [buf[0], buf[1]])
    beyond = route.endswith("beyond")
    n_main = k.spmm_partials_len(V, 0)

    def partials_for(n_listed):
        return torch.full((n_main + n_listed,), float("nan"), dtype=torch.float64, device=dev)

    if route.startswith("row"):
        T = 48 if "t48" in route else 0
        rows = np.nonzero(g.deg > T)[0].astype(np.int32) if T else np.empty(0, np.int32)
        partials = partials_for(rows.size)
        if rows.size:
            k.spmm_update_long(rp, ci, P, to_dev(rows, dev), 4 if route.endswith("long4") else 16, 0, Zo, Xd, GAMMA, Zn,
                               d, partials[n_main:], mirror=mir)
    elif route.startswith("split"):
        T = int(route[5:])
        rows, seg_ptr, seg_row = g.segments(T)
        partials = partials_for(rows.size)
        slab = torch.full((k.spmm_split_slab_len(int(seg_ptr[-1]), d),), float("nan"), dtype=acc, device=dev)
        k.spmm_update_split(rp, ci, P, to_dev(rows, dev), to_dev(seg_ptr, dev), to_dev(seg_row, dev), T, 0, Zo, Xd,
                            GAMMA, Zn, d, slab, partials[n_main:], mirror=mir)
    else:
        T, it = CLASS_DEGREE, g.items(int(route[5:].split("_")[0]))
        partials = partials_for(g.class_rows.size)
        slab = torch.full((k.spmm_class_slab_len(int(it["slot_ptr"][-1]), d),), float("nan"), dtype=acc, device=dev)
        k.spmm_update_class(ci, P, to_dev(it["e0"], dev), to_dev(it["len"], dev), to_dev(it["slot"], dev), 8,
                            to_dev(g.class_rows.astype(np.int32), dev), to_dev(it["slot_ptr"], dev), 0, Zo, Xd, GAMMA,
                            Zn, d, slab, partials[n_main:], mirror=mir, beyond_cache=beyond)
    k.spmm_update(rp, ci, P, V, 0, Zo, Xd, GAMMA, Zn, d, T, partials, sinks_untouched=sinks_untouched, mirror=mir,
                  beyond_cache=beyond and route.startswith("row"))
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    k.reduce_partials(partials, partials.numel(), torch.zeros(k.reduce_ws_len(), dtype=torch.float64, device=dev), out)

    got = Zn.cpu()
    wrong = (got[:, :d] != c.expect).any(1).nonzero().flatten().tolist()
    assert torch.equal(got[:, :d], c.expect), (tag, "rows that differ (degree)", [(r, int(g.deg[r])) for r in wrong[:8]])
    assert ld == d or float(got[:, d:].abs().sum()) == 0.0, (tag, "pad columns")
    assert torch.equal(got[g.sink, :d], c.Zold[g.sink].to(dtype)), (tag, "sinks")
    slots = torch.arange(g.rows_of_slot.size)
    assert torch.equal(buf.cpu()[slots % 2, slots // 2][:, :d], c.expect[torch.from_numpy(g.rows_of_slot)]), (tag, "mirror")
    assert float(out) == c.delta, (tag, "delta", float(out), c.delta)


def check_k3_row_block(k, dev, case, r0=150, n=200):
    """A rank's row block: local rowptr / X / Z_new, global columns, row0 = r0."""
    g, c = graph(), k3_case(*case)
    d = c.d
    Zn = torch.full_like(place(c.X[r0:r0 + n], c.dtype, dev, c.pad), float("nan"))
    Zn[:, d:] = 0
    partials = torch.full((k.spmm_partials_len(n, 0),), float("nan"), dtype=torch.float64, device=dev)
    k.spmm_update(to_dev(g.rowptr, dev)[r0:], to_dev(g.colidx, dev), c.P.to(c.acc).to(dev), n, r0,
                  place(c.Zold, c.dtype, dev, c.pad), place(c.X[r0:r0 + n], c.dtype, dev, c.pad), GAMMA, Zn, d, 0, partials)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    k.reduce_partials(partials, partials.numel(), torch.zeros(k.reduce_ws_len(), dtype=torch.float64, device=dev), out)
    assert torch.equal(Zn.cpu()[:, :d], c.expect[r0:r0 + n]), case_id(case)
    assert Zn.shape[1] == d or float(Zn[:, d:].abs().sum()) == 0.0
    assert float(out) == float(c.row_delta[r0:r0 + n].sum()), case_id(case)


# ---- K1 ------------------------------------------------------------------------------------------------------------
def _int_dots(S, N):
    """int64 dot of S[row] and N[col] for every edge of graph()."""
    g = graph()
    rows, cols = torch.from_numpy(g.row_of_edge), torch.from_numpy(g.colidx.astype(np.int64))
    out = torch.empty(g.E, dtype=torch.int64)
    for a in range(0, g.E, 2048):
        out[a:a + 2048] = (S[rows[a:a + 2048]] * N[cols[a:a + 2048]]).sum(1)
    assert int(out.abs().max()) < (1 << 15)
    return out


def _check_scores(got, want, owned, tag):
    got, owned = got.cpu(), torch.from_numpy(owned)
    assert torch.equal(got[owned], want[owned]), (tag, int((got[owned] != want[owned]).sum()))
    assert bool((got[~owned] == SENTINEL).all()), (tag, "an edge of a row the call does not own was written")


def _k1_calls(g, dev, acc, want, score, score_class, tag):
    """The launches of one K1 entry point: every row by one (sub-)wave; the rows above 48 edges listed as long rows;
    a row block with row0 > 0; the class rows over their items."""
    rp, ci = to_dev(g.rowptr, dev), to_dev(g.colidx, dev)
    fresh = lambda: torch.full((g.E,), SENTINEL, dtype=acc, device=dev)  # noqa: E731
    everything = np.ones(g.E, dtype=bool)
    s = fresh()
    score(rp, ci, V, 0, s)
    _check_scores(s, want, everything, tag + " whole")
    s = fresh()
    score(rp, ci, V, 0, s, 48, to_dev(np.nonzero(g.deg > 48)[0].astype(np.int32), dev))
    _check_scores(s, want, everything, tag + " long rows listed")
    r0, n = 150, 200
    s = fresh()
    score(rp[r0:], ci, n, r0, s)
    _check_scores(s, want, (g.row_of_edge >= r0) & (g.row_of_edge < r0 + n), tag + " row block")
    it = g.items(64)
    s = fresh()
    score_class(rp, ci, *(to_dev(it[key], dev) for key in ("e0", "len", "slot", "row")), 8,
                to_dev(g.class_rows.astype(np.int32), dev), to_dev(it["slot_ptr"], dev), 0, s)
    _check_scores(s, want, np.isin(g.row_of_edge, g.class_rows), tag + " class rows")


def check_k1(k, dev, case):
    """CLANE_SCORE_RAW_DOT through clane_edge_score_* and clane_edge_score_class_*: every score is the int64 dot."""
    dtype, d, pad = case
    g, acc = graph(), _hip.acc_dtype(dtype)
    Z = nonzero_ints(np.random.default_rng(2000 + d), (V, d), 4)
    Zd = place(Z, dtype, dev, pad)
    want = _int_dots(Z.long(), Z.long()).to(acc)
    _k1_calls(g, dev, acc, want,
              lambda rp, ci, n, r0, s, T=0, lr=None: k.edge_score(rp, ci, n, r0, Zd, d, _hip.SCORE_RAW_DOT, None, None, s, T, lr),
              lambda *a: k.edge_score_class(*a[:-1], Zd, d, _hip.SCORE_RAW_DOT, None, None, a[-1]),
              case_id(case) + " edge_score")


def check_k1_pair(k, dev, case):
    """The two-table K1 (S = Y, N = Y + d, lds = ldn = 2d) over an integer Y."""
    dtype, d, _ = case
    g = graph()
    Y = ints(np.random.default_rng(3000 + d), (V, 2 * d), 4)
    Yd = Y.to(dtype).to(dev)
    S, N = Yd[:, :d], Yd[:, d:]
    want = _int_dots(Y[:, :d].long(), Y[:, d:].long()).to(dtype)
    _k1_calls(g, dev, dtype, want,
              lambda rp, ci, n, r0, s, T=0, lr=None: k.edge_score_pair(rp, ci, n, r0, S, N, d, s, T, lr),
              lambda *a: k.edge_score_class_pair(*a[:-1], S, N, d, a[-1]),
              case_id(case) + " edge_score_pair")


def check_row_parts(k, dev, dtype, d, compare_stats=True):
    """CLANE_SCORE_ROW_PARTS(n): n workgroups share a listed row's rescale pass; scores and stats do not depend on n."""
    from clane_amd import synth
    g, acc = graph(), _hip.acc_dtype(dtype)
    Zd = place(synth.gaussian_X(V, d, seed=5).double(), dtype, dev, True)
    sq = torch.empty(V, dtype=acc, device=dev)
    k.row_sqnorm(Zd, d, sq)
    it = g.items(64)
    n_slots = int(it["slot_ptr"][-1])
    args = (to_dev(g.rowptr, dev), to_dev(g.colidx, dev), *(to_dev(it[key], dev) for key in ("e0", "len", "slot", "row")),
            8, to_dev(g.class_rows.astype(np.int32), dev), to_dev(it["slot_ptr"], dev), 0, Zd, d, _hip.SCORE_PER_EDGE,
            None, sq)
    runs = {}
    for parts in (1, 2, 7, 64, 255):
        scores = torch.full((g.E,), SENTINEL, dtype=acc, device=dev)
        stats = torch.full((2 * n_slots,), -1.0, dtype=acc, device=dev)
        k.edge_score_class(*args, scores, stats, fuse_softmax=True, n_slots=n_slots, row_parts=parts)
        runs[parts] = (scores.cpu(), stats.cpu())
    listed = torch.from_numpy(np.isin(g.row_of_edge, g.class_rows))
    first = runs[1][0]
    assert bool((first[~listed] == SENTINEL).all()) and bool(((first[listed] > 0) & (first[listed] <= 1)).all())
    for parts, (scores, stats) in runs.items():
        assert torch.equal(scores, first), parts
        if compare_stats:
            assert torch.equal(stats, runs[1][1]) and not bool((stats == -1.0).all()), parts


# ---- the other stage kernels -----------------------------------------------------------------------------------------
def check_stage_kernels(k, dev, case):
    """row_sqnorm, degree_weighted_sums, l1_distance (with the norms it leaves behind) on integer tables."""
    dtype, d, pad = case
    g, acc = graph(), _hip.acc_dtype(dtype)
    rng = np.random.default_rng(4000 + d)
    A, B = nonzero_ints(rng, (V, d), 4), ints(rng, (V, d), 8)
    Ad, Bd = place(A, dtype, dev, pad), place(B, dtype, dev, pad)
    want_sq = A.long().pow(2).sum(1)
    sq = torch.full((V,), float("nan"), dtype=acc, device=dev)
    k.row_sqnorm(Ad, d, sq)
    assert torch.equal(sq.cpu(), want_sq.to(acc)), case_id(case)
    indeg = np.bincount(g.colidx, minlength=V).astype(np.int32)
    ws = torch.zeros(k.reduce_ws_len(), dtype=torch.float64, device=dev)
    sums2 = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    k.degree_weighted_sums(sq, to_dev(g.rowptr, dev), to_dev(indeg, dev), V, ws, sums2)
    want2 = [int((torch.from_numpy(w).long() * want_sq).sum()) for w in (g.deg, indeg)]
    assert sums2.cpu().tolist() == [float(want2[0]), float(want2[1])], case_id(case)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    sq_l1 = torch.full((V,), float("nan"), dtype=acc, device=dev)
    k.l1_distance(Ad, Bd, d, ws, out, sq_a=sq_l1)
    assert float(out) == float((A - B).abs().sum()), case_id(case)
    assert torch.equal(sq_l1, sq), case_id(case)
    out2 = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    k.l1_distance(Ad, Bd, d, ws, out2)
    assert float(out2) == float(out)


def check_gather_rows(k, dev, case):
    """dst[i] = src[idx[i]] bit for bit for n in 0, 1, 63, 64, 65, 5000; rows beyond n keep their sentinel."""
    dtype, d, pad = case
    rng = np.random.default_rng(5000 + d)
    src_h = nonzero_ints(rng, (V, d), 4)
    src = place(src_h, dtype, dev, pad)
    for n in (0, 1, 63, 64, 65, 5000):
        idx = rng.integers(0, V, size=n)
        if n:
            idx[0], idx[-1] = 0, V - 1                                          # the first and the last table row
        if n > 8:
            idx[1], idx[-2], idx[5] = V - 1, 0, idx[3]                          # ... again, and a repeat next door
        dst = torch.full((n + 3, src.shape[1]), 9.0, dtype=dtype, device=dev)
        k.gather_rows(src, to_dev(idx.astype(np.int32), dev), d, dst)
        got = dst.cpu()
        assert torch.equal(got[:n, :d], src_h[torch.from_numpy(idx)].to(dtype)), (case_id(case), n)
        assert bool((got[n:] == 9.0).all()), (case_id(case), n, "rows beyond n")


# ---- projections and the gradient --------------------------------------------------------------------------------------
PROJECT_ROWS = (1, 127, 128, 129, 300)
PROJECT_D = (1, 5, 17, 65, 130)            # 2d = 130 / 260 crosses one / two 128-wide tiles
GRAD_B = (1, 15, 16, 17, 2047, 2048, 2049, 4097)       # the 16-pair staging slice and the 2048-pair chunk, -1 / 0 / +1
GRAD_D = (5, 17, 130)
GRAD_M = 64.0


def check_projections(k, dev, dtype, d):
    """project_rows and pair_project == the int64 matmul, outputs pre-filled with NaN."""
    acc = _hip.acc_dtype(dtype)
    rng = np.random.default_rng(6000 + d)
    W = ints(rng, (2 * d, d), 3)
    Wd = W.to(acc).to(dev)
    for rows in PROJECT_ROWS:
        Z = nonzero_ints(rng, (rows, d), 4)
        Zd = place(Z, dtype, dev, True)
        want = (Z.long() @ W.long().T).to(acc)
        Y = torch.full((rows, 2 * d), float("nan"), dtype=acc, device=dev)
        k.project_rows(Zd, d, Wd, Y)
        assert torch.equal(Y.cpu(), want), (dtype, d, rows, "project_rows")
        src, dst = rng.integers(0, rows, size=rows), rng.integers(0, rows, size=rows)
        A, Bm = (torch.full((rows, d), float("nan"), dtype=acc, device=dev) for _ in range(2))
        k.pair_project(Zd, d, to_dev(src.astype(np.int32), dev), to_dev(dst.astype(np.int32), dev), Wd, A, Bm)
        assert torch.equal(A.cpu(), want[torch.from_numpy(src), :d]), (dtype, d, rows, "pair_project A")
        assert torch.equal(Bm.cpu(), want[torch.from_numpy(dst), d:]), (dtype, d, rows, "pair_project Bm")


def _grad_inputs(rng, R, B, d):
    Z = nonzero_ints(rng, (R, d), 4)
    src, dst = rng.integers(0, R, size=B), rng.integers(0, R, size=B)
    return Z, src, dst, ints(rng, (B, d), 3), ints(rng, (B, d), 3), ints(rng, (B,), 2)


def _grad_expect(Zs, Zt, A, Bm, g, acc):
    """dW * M in int64: rows [0, d) = sum_k g_k Bm[k]^T z_src[k], rows [d, 2d) = sum_k g_k A[k]^T z_dst[k]."""
    gl = g.long().unsqueeze(1)
    top, bottom = (gl * Bm.long()).T @ Zs.long(), (gl * A.long()).T @ Zt.long()
    want = torch.cat([top, bottom])
    assert int(want.abs().max()) < (1 << 24)
    return (want.double() / GRAD_M).to(acc)


def _run_grad(k, dev, dtype, d, Zd, src, dst, A, Bm, g, M):
    acc = _hip.acc_dtype(dtype)
    B = src.size
    ws = torch.full((k.pair_grad_ws_len(B, d),), float("nan"), dtype=acc, device=dev)
    dW = torch.full((2 * d, d), float("nan"), dtype=acc, device=dev)
    k.pair_grad(Zd, d, to_dev(src.astype(np.int32), dev), to_dev(dst.astype(np.int32), dev), A.to(acc).to(dev),
                Bm.to(acc).to(dev), g.to(acc).to(dev), torch.tensor([0.0, M], dtype=torch.float64, device=dev), ws, dW)
    return dW.cpu()


def check_pair_grad(k, dev, dtype, d):
    """pair_grad fed integer A, Bm, g and stats = [0, 64]: dW == the int64 contraction / 64; M = 0: dW == 0."""
    acc = _hip.acc_dtype(dtype)
    rng = np.random.default_rng(7000 + d)
    for B in GRAD_B:
        Z, src, dst, A, Bm, g = _grad_inputs(rng, 200, B, d)
        Zd = place(Z, dtype, dev, True)
        got = _run_grad(k, dev, dtype, d, Zd, src, dst, A, Bm, g, GRAD_M)
        want = _grad_expect(Z[torch.from_numpy(src)], Z[torch.from_numpy(dst)], A, Bm, g, acc)
        assert torch.equal(got, want), (dtype, d, B)
    assert torch.equal(_run_grad(k, dev, dtype, d, Zd, src, dst, A, Bm, g, 0.0), torch.zeros(2 * d, d, dtype=acc)), (dtype, d)


def check_out_of_range_pairs(k, dev, dtype, d, R=40, B=300):
    """A pair row outside [0, table_rows) is read as a zero row.  The table is rows [1, R + 1) of a buffer whose rows 0
    and R + 1 are NaN and the bad indices are -1 and R only: a lost guard reads memory the test owns and shows as NaN."""
    acc = _hip.acc_dtype(dtype)
    rng = np.random.default_rng(8000 + d)
    Z, src, dst, A, Bm, g = _grad_inputs(rng, R, B, d)
    src[::7], src[3::11], dst[1::5], dst[2::13] = -1, R, R, -1
    big = place(torch.cat([torch.zeros(1, d, dtype=torch.float64), Z, torch.zeros(1, d, dtype=torch.float64)]), dtype, dev, True)
    big[0, :d] = float("nan")
    big[R + 1, :d] = float("nan")
    view = big[1:R + 1]
    assert view.shape[0] == R and view.data_ptr() == big.data_ptr() + big.stride(0) * big.element_size()

    def rows_or_zero(idx):
        ok = torch.from_numpy((idx >= 0) & (idx < R))
        return Z[torch.from_numpy(np.clip(idx, 0, R - 1))] * ok.unsqueeze(1)

    Zs, Zt = rows_or_zero(src), rows_or_zero(dst)
    W = ints(rng, (2 * d, d), 3)
    PA, PB = (torch.full((B, d), float("nan"), dtype=acc, device=dev) for _ in range(2))
    k.pair_project(view, d, to_dev(src.astype(np.int32), dev), to_dev(dst.astype(np.int32), dev), W.to(acc).to(dev), PA, PB)
    assert torch.equal(PA.cpu(), (Zs.long() @ W[:d].long().T).to(acc)), (dtype, d, "pair_project A")
    assert torch.equal(PB.cpu(), (Zt.long() @ W[d:].long().T).to(acc)), (dtype, d, "pair_project Bm")
    bad_s, bad_t = torch.from_numpy((src < 0) | (src >= R)), torch.from_numpy((dst < 0) | (dst >= R))
    assert int(bad_s.sum()) > 20 and int(bad_t.sum()) > 20
    assert float(PA.cpu()[bad_s].abs().sum()) == 0.0 and float(PB.cpu()[bad_t].abs().sum()) == 0.0
    got = _run_grad(k, dev, dtype, d, view, src, dst, A, Bm, g, GRAD_M)
    assert torch.equal(got, _grad_expect(Zs, Zt, A, Bm, g, acc)), (dtype, d, "pair_grad")


# ---- pair_labels -----------------------------------------------------------------------------------------------------
def label_pairs(B):
    """(src, dst, expected linked) of B pairs over graph()'s sorted CSR: for every row its first and last column, the
    first column of the next non-empty row and the last of the previous one, a destination below its first and above
    its last column; src = -1 and src = nrows; then seeded random pairs up to B.  Expected by a numpy set lookup."""
    g = graph()
    rp, ci = g.rowptr, g.sorted_colidx
    full = np.nonzero(g.deg > 0)[0]
    nxt = {int(r): int(n) for r, n in zip(full[:-1], full[1:])}
    prv = {int(n): int(r) for r, n in zip(full[:-1], full[1:])}
    src, dst = [], []
    for r in range(V):
        wanted = [0, V - 1, V // 2]
        if g.deg[r]:
            first, last = int(ci[rp[r]]), int(ci[rp[r + 1] - 1])
            wanted += [first, last, first - 1, last + 1]
        for other, at in ((nxt.get(r), 0), (prv.get(r), -1)):        # what sits just outside [rowptr[r], rowptr[r+1])
            if other is not None:
                wanted.append(int(ci[rp[other]:rp[other + 1]][at]))
        nearest = full[np.searchsorted(full, r)] if r <= full[-1] else full[-1]     # degree-0 rows: a neighbour's edge
        wanted.append(int(ci[rp[nearest]]))
        src += [r] * len(wanted)
        dst += wanted
    for bad in (-1, V):
        src += [bad] * 4
        dst += [0, int(ci[0]), int(ci[-1]), V - 1]
    rng = np.random.default_rng(9)
    n_random = max(0, B - len(src))
    src = np.concatenate([np.array(src), rng.integers(-1, V + 1, size=n_random)])[:B].astype(np.int32)
    dst = np.concatenate([np.array(dst), rng.integers(-1, V + 1, size=n_random)])[:B].astype(np.int32)
    edges = g.row_of_edge.astype(np.int64) * (V + 2) + ci
    inside = (src >= 0) & (src < V)
    linked = (inside & np.isin(src.astype(np.int64) * (V + 2) + dst, edges) & (dst >= 0)).astype(np.uint8)
    return src, dst, linked


def check_pair_labels(k, dev, B):
    g = graph()
    src, dst, want = label_pairs(B)
    assert B < 6000 or (want.sum() > 800 and (want == 0).sum() > 3000)
    linked = torch.full((B,), 7, dtype=torch.uint8, device=dev)
    k.pair_labels(to_dev(g.rowptr, dev), to_dev(g.sorted_colidx, dev), V, to_dev(src, dev), to_dev(dst, dev), linked)
    got = linked.cpu().numpy()
    assert np.array_equal(got, want), (B, np.nonzero(got != want)[0][:8], src[got != want][:8], dst[got != want][:8])


def check_pair_labels_small(k, dev):
    """B = 0, B = 1 and a table without rows (real one-element buffers)."""
    g = graph()
    rp, ci = to_dev(g.rowptr, dev), to_dev(g.sorted_colidx, dev)
    r = int(np.argmax(g.deg > 0))
    linked = torch.full((3,), 7, dtype=torch.uint8, device=dev)
    none = torch.zeros(0, dtype=torch.int32, device=dev)
    k.pair_labels(rp, ci, V, none, none, linked)
    assert linked.tolist() == [7, 7, 7]
    for col, want in ((int(g.sorted_colidx[g.rowptr[r]]), 1), (V, 0)):
        k.pair_labels(rp, ci, V, torch.tensor([r], dtype=torch.int32, device=dev),
                      torch.tensor([col], dtype=torch.int32, device=dev), linked)
        assert linked.tolist() == [want, 7, 7]
    linked.fill_(7)
    k.pair_labels(torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), 0,
                  torch.tensor([0, -1, 5], dtype=torch.int32, device=dev),
                  torch.tensor([0, 0, 0], dtype=torch.int32, device=dev), linked)
    assert linked.tolist() == [0, 0, 0]
