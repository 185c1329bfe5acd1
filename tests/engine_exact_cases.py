"""Exact integer-data sweeps through SweepEngine's OWN launch plan -- helpers of tests/test_gpu_engine_exact.py (the HIP
kernels) and tests/test_engine_exact_host.py (the same checks through the CPU test double, plus the fixtures' and the
checks' self-checks).

tests/exact_cases.py pins every kernel to the bit, but with row lists, class items, segments and mirrors that the TEST
builds.  Here the engine builds them: the vertex permutation, the row bins, the partial offsets of every bin and column
tile, the class items of the relabelled CSR, the halo send lists and mirrors, the quiet-row sync, the three-table
rotation and l1_between.  The recipe is exact_cases': Z0 non-zero integers in [-4, 4], X integers in [-8, 8], P[e] = m/4
with m in 1..8 (over the SORTED edge order: the engine does its own class ordering), gamma = 0.5 -- every partial sum is
a multiple of 1/8 below 2^24, so whatever order the engine's plan adds things in, get_Z() must be torch.equal to the
fp64 oracle's sweep rounded once to the storage dtype and the returned delta == the sum over the stored values.
`SequenceCase` does the same for three consecutive fp64 sweeps (its quantum shrinks by 2^-13 per sweep; the budget is
asserted from the data).

Every check takes the kernel object and the device: HipKernels on the card, the oracle-backed double on the host.  A
check collects its named comparisons in a `Checks` and asserts that none failed; every comparison is torch.equal or ==.
Nothing here has a tolerance.

`OWNED_PLANS` puts the class rows of the one-GPU plans through the owned pass (spmm_owned_kernel: fp32 only, hence a
list of its own), down to the configuration the engine chooses by itself for a table beyond the Infinity Cache.

Combinations the engine refuses by design, hence not run: column tiles under any division (engine.py,
_choose_division: ``T = self._pick_tiles(csr, X.dtype) if not divided else 1`` -- a division ignores ``column_tiles``;
_build_plan: "column tiles and mirrored launches do not combine").
"""
import contextlib
import functools
import threading

import numpy as np
import torch

import clane_amd.engine as engine_module
from clane_amd import _hip, xcd
from clane_amd.engine import SPLIT_EDGES, SweepEngine
from clane_amd.partition import HostCSR
from clane_amd.plan import lanes_per_row
from oracle import clane_oracle as O

from . import exact_cases as E
from .exact_cases import BF16, F32, F64, GAMMA
from .test_gpu_parity import ragged_csr
from .thread_comm import ThreadWorld

# the padded layouts of exact_cases.LAYOUT_CASES (the engine always pads ld: the odd strides stay with exact_cases)
ENGINE_CASES = [(t, d) for t, d, pad in E.LAYOUT_CASES if pad]
ONE_PER_DTYPE = [(F32, 128), (BF16, 128), (F64, 64)]
SPLIT_CASES = [(F32, 64), (BF16, 64), (F64, 16)]           # the range condition on the split graph: d <= 64
SEED = 11                                                  # of the shuffled layouts


def case_id(case):
    return f"{_hip._SUFFIX[case[0]]}-d{case[1]}"


# ---- the graphs ------------------------------------------------------------------------------------------------------
class SplitGraph:
    """4300 vertices: rows 3 and 10 point at EVERY vertex (more than SPLIT_EDGES edges: the segmented route), rows of
    300 and 129 edges, a ragged remainder of at most 12 edges and empty rows."""
    V = 4300

    def __init__(self):
        csr = ragged_csr(self.V, seed=23, max_deg=12, hubs=(self.V, self.V, 300, 129))
        self.rowptr, self.sorted_colidx = csr.rowptr, csr.colidx
        self.deg = np.diff(csr.rowptr)
        self.E = int(csr.num_edges)
        self.sink = torch.from_numpy(self.deg == 0)
        assert (self.deg > SPLIT_EDGES).sum() == 2 and self.deg.max() == self.V and (self.deg == 0).sum() > 500


@functools.lru_cache(maxsize=None)
def graph(name="ragged"):
    return E.graph() if name == "ragged" else SplitGraph()


def n_vertices(g):
    return int(g.deg.size)


# ---- the cases -------------------------------------------------------------------------------------------------------
class EngineCase:
    """Inputs and exact expectations of ONE sweep at (dtype, d) over graph(gname), P in the sorted edge order.  Host
    tensors; nobody writes to them."""

    def __init__(self, dtype, d, gname="ragged"):
        g = graph(gname)
        V = n_vertices(g)
        rng = np.random.default_rng(1500 + d)
        self.dtype, self.d, self.gname, self.acc = dtype, d, gname, _hip.acc_dtype(dtype)
        self.Z0 = E.nonzero_ints(rng, (V, d), 4)
        self.X = E.ints(rng, (V, d), 8)
        self.P = torch.from_numpy(rng.integers(1, 9, size=g.E)).double() / 4
        self.Ps = O.as_sparse(g.rowptr, g.sorted_colidx, self.P)
        # the condition for exactness, as exact_cases.K3Case states it: every partial sum is a multiple of 1/8 within
        # this bound, a row's L1 delta (summed in the accumulate type) a multiple of 1/8 within d * (bound + 4)
        self.bound = float((GAMMA * torch.sparse.mm(self.Ps, self.Z0.abs()) + 8).max())
        assert self.bound * 8 < E.EXACT_LIMIT and d * (self.bound + 4) * 8 < E.EXACT_LIMIT, (dtype, d, self.bound)
        ref, _ = O.sweep(g.rowptr, g.sorted_colidx, self.P, self.X, self.Z0, GAMMA, self.Ps)
        assert float((ref * 8 - (ref * 8).round()).abs().max()) == 0 and float(ref.abs().max()) <= self.bound
        self.ref64 = ref
        self.expect = ref.to(dtype)                                   # rounded once, to nearest even
        assert self.Z0.to(dtype).double().equal(self.Z0) and self.X.to(dtype).double().equal(self.X)
        self.diff = (self.expect.double() - self.Z0).abs()            # of the stored values
        self.row_delta = self.diff.sum(1)
        self.delta = float(self.row_delta.sum())
        assert self.delta * 8 < float(1 << 53)                        # the fp64 reductions of the partials
        assert float(self.row_delta[g.sink].sum()) == 0 and self.expect[g.sink].double().equal(self.Z0[g.sink])

    def undetected_single_edge_drops(self, limit=600):
        """exact_cases.K3Case's self-check for the sorted P order: of the first `limit` edges of the longest row, how
        many could vanish from the sum without changing the expected row in the storage dtype."""
        g = graph(self.gname)
        r = int(np.argmax(g.deg))
        a = int(g.rowptr[r])
        n = min(int(g.deg[r]), limit)
        cols = torch.from_numpy(g.sorted_colidx[a:a + n].astype(np.int64))
        without = self.ref64[r].unsqueeze(0) - GAMMA * self.P[a:a + n].unsqueeze(1) * self.Z0[cols]
        changed = (without.to(self.dtype) != self.expect[r].unsqueeze(0)).any(1)
        return n, int((~changed).sum())


@functools.lru_cache(maxsize=None)
def engine_case(dtype, d, gname="ragged"):
    return EngineCase(dtype, d, gname)


SEQUENCE_SWEEPS = 3


class SequenceCase:
    """Three consecutive fp64 sweeps over graph(), all exact.  P[e] = m * 2^-(q_r + 2) with m in 1..4 and
    q_r = ceil(log2(deg_r)): a row of P sums to at most 1, so values stay within 16, and with gamma = 1/2 the quantum
    after s sweeps is 2^-13s (q_r <= 10 on this graph).  The budget -- 2^53 quanta against the bound on every partial
    sum, the row delta and the global delta, and every expected value a multiple of the quantum -- is asserted here
    from the data."""

    def __init__(self, d=32):
        g = graph()
        V = n_vertices(g)
        rng = np.random.default_rng(2500 + d)
        self.dtype, self.d, self.gname, self.acc = F64, d, "ragged", F64
        self.Z0 = E.nonzero_ints(rng, (V, d), 4)
        self.X = E.ints(rng, (V, d), 8)
        q = np.ceil(np.log2(np.maximum(g.deg, 1))).astype(np.int64)
        assert (2.0 ** q >= g.deg).all() and int(q.max()) == 10
        m = rng.integers(1, 5, size=g.E)
        self.P = torch.from_numpy(m * 2.0 ** -(q[g.row_of_edge] + 2))
        self.Ps = O.as_sparse(g.rowptr, g.sorted_colidx, self.P)
        assert float(torch.sparse.mm(self.Ps, torch.ones(V, 1, dtype=F64)).max()) <= 1.0
        limit = float(1 << 53)
        self.Z, self.deltas = [self.Z0], []
        for s in range(1, SEQUENCE_SWEEPS + 1):
            old = self.Z[-1]
            quantum = 2.0 ** (-13 * s)
            new, _ = O.sweep(g.rowptr, g.sorted_colidx, self.P, self.X, old, GAMMA, self.Ps)
            # every partial sum of a row, in any order, with or without gamma applied yet (sum P z has twice the
            # quantum and at most twice the bound: the same bits)
            bound = float((GAMMA * torch.sparse.mm(self.Ps, old.abs()) + self.X.abs()).max())
            assert bound < limit * quantum and float(new.abs().max()) <= bound < 16, (s, bound)
            assert d * (bound + float(old.abs().max())) < limit * quantum, s             # a row's L1 delta
            scaled = new * 2.0 ** (13 * s)
            assert bool((scaled == scaled.round()).all()), s                             # multiples of the quantum
            delta = float((new - old).abs().sum())
            assert delta < limit * quantum, s                                            # the global delta
            assert new[g.sink].equal(self.Z0[g.sink])
            self.Z.append(new)
            self.deltas.append(delta)
        self.distance = float((self.Z[2] - self.Z0).abs().sum())                         # snapshot -> after two sweeps
        assert self.distance < limit * 2.0 ** -26


@functools.lru_cache(maxsize=None)
def sequence_case(d=32):
    return SequenceCase(d)


# ---- the engine ------------------------------------------------------------------------------------------------------
def device_ctx(dev):
    return torch.cuda.device(dev) if torch.device(dev).type == "cuda" else contextlib.nullcontext()


def load_P(eng, P_sorted):
    """The inverse of SweepEngine.P_global(): P in the global (row, col)-sorted edge order into the engine's own.
    After set_Z, which clears the flag."""
    eng.P[:eng.E_loc] = P_sorted[torch.from_numpy(eng.local.edge_origin)].to(eng.acc_dtype).to(eng.device)
    eng.P_valid = True


def make_engine(kernels, dev, c, comm=None, **settings):
    g = graph(c.gname)
    eng = SweepEngine(HostCSR(n_vertices(g), g.rowptr, g.sorted_colidx), c.X.to(c.dtype), dev, kernels, comm=comm,
                      **settings)
    eng.set_Z(c.Z0.to(c.dtype))
    load_P(eng, c.P)
    return eng


def block_of_vertex(eng):
    """int [V]: the launch block of this engine that finishes each vertex' row, -1 for another rank's."""
    out = np.full(eng.V, -1, dtype=np.int64)
    for i, b in enumerate(eng.blocks):
        verts = eng.local.vertex[b.local_start:b.local_start + b.nrows]
        out[verts[verts >= 0]] = i
    return out


def block_partials(eng):
    """Sum of the delta partials the latest sweep left for each launch block (all column tiles) -- for messages."""
    n = eng.partial_off[-1]
    parts = eng.partials.cpu().view(len(eng.tiles), n)
    return [float(parts[:, eng.partial_off[i]:eng.partial_off[i + 1]].sum()) for i in range(len(eng.blocks))]


class Checks:
    """The named exact comparisons of one run.  `failed`: [(name, detail)]."""

    def __init__(self, tag):
        self.tag, self.failed, self.names = tag, [], []

    def record(self, name, ok, *detail):
        self.names.append(name)
        if not ok:
            self.failed.append((name,) + detail)

    def failed_names(self):
        return [f[0] for f in self.failed]

    def assert_none_failed(self):
        assert self.failed == [], (self.tag, self.failed)


def differing_rows(g, got, want, blocks):
    """The rows of `got` that differ from `want`: (vertex, degree, block) -- block = (rank, block) under a division."""
    wrong = (got != want).any(1).nonzero().flatten().tolist()
    return [(r, int(g.deg[r]), blocks[r]) for r in wrong[:8]]


def judge_table(checks, g, name, got, want, Z0, dtype, blocks):
    checks.record(name, torch.equal(got, want), "rows that differ (vertex, degree, block)",
                  differing_rows(g, got, want, blocks))
    checks.record(name + " sinks", torch.equal(got[g.sink], Z0[g.sink].to(dtype)), "sinks moved")


def judge_delta(checks, name, got, want, eng_blocks=None):
    """`eng_blocks`: [(block, partials found, partials expected)] of the blocks whose share of the delta differs."""
    checks.record(name, got == want, got, want, got - want, "blocks whose partials differ (block, got, want)", eng_blocks)


def expected_block_deltas(eng, c):
    """What each launch block of this engine owes the delta: its own rows, its own columns."""
    share = c.diff[:, eng.col0:eng.col1].sum(1)
    out = []
    for b in eng.blocks:
        verts = eng.local.vertex[b.local_start:b.local_start + b.nrows]
        out.append(float(share[torch.from_numpy(verts[verts >= 0])].sum()))
    return out


def wrong_blocks(eng, c):
    return [(i, a, b) for i, (a, b) in enumerate(zip(block_partials(eng), expected_block_deltas(eng, c))) if a != b]


def pads_are_zero(eng):
    return bool((eng.Zcur[:, eng.d:] == 0).all())


def one_sweep(eng, c):
    """snapshot(), one sweep, and everything check A reads off the engine afterwards."""
    eng.snapshot()
    delta = eng.sweep(GAMMA)
    out = dict(delta=delta, wrong_blocks=wrong_blocks(eng, c), pads=pads_are_zero(eng),
               distance=eng.distance_from_snapshot(), Z=eng.get_Z(), blocks=block_of_vertex(eng))
    return out


def judge_one_sweep(checks, c, out, blocks=None):
    g = graph(c.gname)
    judge_table(checks, g, "Z", out["Z"], c.expect, c.Z0, c.dtype, out["blocks"] if blocks is None else blocks)
    checks.record("pad columns", out["pads"])
    judge_delta(checks, "delta", out["delta"], c.delta, out["wrong_blocks"])
    judge_delta(checks, "snapshot distance", out["distance"], c.delta)


# ---- A: one-GPU plans --------------------------------------------------------------------------------------------------
def _none(lists):
    return all(x is None for x in lists)


def _some(lists):
    return any(x is not None for x in lists)


def _route_defaults(eng, dev):
    # 700 x ld fits every cache: the defaults always give the class pass the hubs, one block, one tile
    assert _some(eng.class_rows) and _none(eng.split_rows) and len(eng.blocks) == 1 and len(eng.tiles) == 1


def _route_row_pass(eng, dev):
    assert _none(eng.mid_rows) and _none(eng.hub_rows) and _none(eng.split_rows) and _none(eng.class_rows)
    assert eng.long_threshold == 0 and eng.class_threshold == 0


def _route_bins(eng, dev):
    assert eng.mid_rows[0] is not None and eng.hub_rows[0] is not None and _none(eng.class_rows) and _none(eng.split_rows)
    assert (eng.long_threshold, eng.hub_threshold) == (48, 128)


def _route_class(chunk, phases=1):
    def route(eng, dev):
        assert eng.class_rows[0] is not None and (eng.class_threshold, eng.class_chunk) == (32, chunk)
        assert _none(eng.mid_rows) and _none(eng.hub_rows) and _none(eng.split_rows)      # the class rows are all long rows
        assert eng.class_phases == phases and eng.phase_threshold == (128 if phases > 1 else 0)
    return route


def _route_chunked(overlap, shuffled=True):
    def route(eng, dev):
        assert bool((eng.pos.cpu() == torch.arange(eng.V)).all()) != shuffled              # vertex order kept, or not
        assert len(eng.blocks) == 3 and sum(b.nrows for b in eng.blocks) == eng.part.padded_vertices > eng.V   # a pad row
        assert not eng.hot_rows_first
        if torch.device(dev).type == "cuda":
            assert (eng.side_streams is not None) == overlap
    return route


def _route_tiles(T, with_class):
    def route(eng, dev):
        assert len(eng.tiles) == T and eng.tiles[0][0] == 0 and eng.tiles[-1][1] == eng.d
        assert _some(eng.class_rows) == with_class
        assert eng.partials.numel() == T * eng.partial_off[-1]
    return route


def _route_contiguous(eng, dev):
    # two Z tables + X, the third Z table comes with the snapshot; or the driver had no such range
    assert eng.table_alloc == "contiguous" and (len(eng._own_tables) == 3 or eng.table_alloc_note is not None)


CLASS_ON = dict(class_threshold=32, class_chunk=64)
PLANS = {
    "defaults": (dict(), _route_defaults),
    "row_pass_only": (dict(class_threshold=0, long_threshold=0), _route_row_pass),
    "bins_4_and_16_waves": (dict(class_threshold=0, long_threshold=48, hub_threshold=128), _route_bins),
    "class_chunk64": (dict(class_threshold=32, class_chunk=64, class_phases=1), _route_class(64)),
    "class_chunk256": (dict(class_threshold=32, class_chunk=256, class_phases=1), _route_class(256)),
    "class_phases2": (dict(CLASS_ON, class_phases=2, phase_threshold=128), _route_class(64, 2)),
    "class_phases4": (dict(CLASS_ON, class_phases=4, phase_threshold=128), _route_class(64, 4)),
    "chunks3_overlap": (dict(chunks=3, overlap_chunks=True, hot_rows_first=False, shuffle=True, seed=SEED),
                        _route_chunked(True)),
    "chunks3_in_order": (dict(chunks=3, overlap_chunks=False, hot_rows_first=False, shuffle=True, seed=SEED),
                         _route_chunked(False)),
    "chunks3_vertex_order": (dict(chunks=3, hot_rows_first=False), _route_chunked(True, shuffled=False)),
    "chunks3_class": (dict(CLASS_ON, chunks=3, hot_rows_first=False, shuffle=True, seed=SEED + 1), _route_chunked(True)),
    "tiles2": (dict(column_tiles=2, class_threshold=0), _route_tiles(2, False)),
    "tiles2_class": (dict(CLASS_ON, column_tiles=2), _route_tiles(2, True)),
    "tiles3": (dict(column_tiles=3, class_threshold=0), _route_tiles(3, False)),
    "tiles3_class": (dict(CLASS_ON, column_tiles=3), _route_tiles(3, True)),
    "contiguous_tables": (dict(table_alloc="contiguous"), _route_contiguous),
}
EVERY_CASE_PLANS = ("defaults", "row_pass_only", "bins_4_and_16_waves", "class_chunk64", "class_chunk256")
OTHER_PLANS = tuple(p for p in PLANS if p not in EVERY_CASE_PLANS)
TILE_PLANS = tuple(p for p in PLANS if p.startswith("tiles"))
# (case, plan): the first five plans on every case, the rest on one case per dtype; fp32 d = 300 under tiles (75 packs:
# 38 + 37 in two tiles, 25 each in three)
PLAN_RUNS = ([(c, p) for c in ENGINE_CASES for p in EVERY_CASE_PLANS] + [(c, p) for c in ONE_PER_DTYPE for p in OTHER_PLANS]
             + [((F32, 300), p) for p in TILE_PLANS])


def plan_id(run):
    return f"{case_id(run[0])}-{run[1]}"


def run_plan(kernels, dev, c, settings, route, tag, constructing=contextlib.nullcontext):
    """One engine, one sweep: the `Checks` of check A.  `constructing`: a context for the engine's construction."""
    checks = Checks(tag)
    with device_ctx(dev):
        with constructing():
            eng = make_engine(kernels, dev, c, **settings)
        route(eng, dev)
        judge_one_sweep(checks, c, one_sweep(eng, c))
    return checks


def check_plan(kernels, dev, case, plan):
    settings, route = PLANS[plan]
    run_plan(kernels, dev, engine_case(*case), settings, route, plan_id((case, plan))).assert_none_failed()


# ---- A': the owned class pass (csrc/spmm_update.h spmm_owned_kernel) under the engine's plans ------------------------
# Apart from PLANS / PLAN_RUNS, which tests/consumer_exact_cases.py and OTHER_PLANS also run at bf16 and fp64, where the
# owned pass has no instance.  Judged like every plan of A.  8 groups with 8 LDS sums each: the 103 rows above 32 edges
# need up to 3 batches per group; the 700-edge row is 6 virtual rows of at most 128 edges (4 sums per batch could not
# hold it: xcd.owned_plan refuses).
OWN = dict(class_owned=True, owned_groups=8, owned_block_threads=256, owned_row_edges=128, owned_max_edges=4096)
OWNED_SUMS = 8
CHUNKS3_GROUPS = 3              # some 35 class rows per block of 234: 3 groups of 8 sums need 2 batches in every block


def own(*base, width=128, **more):
    """OWN, the LDS of OWNED_SUMS sums of rows (or column tiles) of `width` fp32 elements, and what the plan adds."""
    out = dict(OWN, owned_lds_bytes=OWNED_SUMS * 16 * lanes_per_row(width, F32))
    for b in base:
        out.update(b)
    out.update(more)
    return out


@contextlib.contextmanager
def no_infinity_cache():
    """While an engine is constructed: its planning sees an Infinity Cache of no bytes, so every table is beyond it.
    Put back on the way out; the engine keeps what it chose."""
    kept = engine_module.INFINITY_CACHE_BYTES
    engine_module.INFINITY_CACHE_BYTES = 0
    try:
        yield
    finally:
        engine_module.INFINITY_CACHE_BYTES = kept


def plan_field(plan, name):
    """A field of a block's owned plan: xcd.owned_plan's dict on the double, _hip.OwnedPlan on the card."""
    if isinstance(plan, dict):
        return plan[name]
    return plan.arrays[name].cpu().numpy() if name in plan.arrays else getattr(plan, name)


def batches_per_group(plan):
    return np.diff(plan_field(plan, "grp_bat_ptr"))


def _route_owned(blocks=1, n_rest=0, batches=2, hot=True, tiles=1, steps=None, more=None):
    """EVERY block has an owned plan, with `n_rest` class rows beside it on chunk + combine; some group
    takes its rows in at least `batches` batches; the vertex order is the engine's own (`hot`) or a shuffled one."""
    def route(eng, dev):
        assert eng.class_owned and len(eng.blocks) == blocks and all(o is not None for o in eng.owned_rows)
        plans = [o[0] for o in eng.owned_rows]
        for _, rest, n in eng.owned_rows:
            assert (rest is not None) == (n > 0) and n == n_rest
        assert max(int(batches_per_group(p).max()) for p in plans) >= batches
        assert all(plan_field(p, "n_groups") == eng.owned_groups for p in plans) and len(eng.tiles) == tiles
        assert eng.hot_rows_first == hot and not bool((eng.pos.cpu() == torch.arange(eng.V)).all())
        if steps is not None:
            assert [plan_field(p, "n_steps") for p in plans] == steps
        if more is not None:
            more(eng, plans)
    return route


def _owned_class(eng, plans):
    assert plan_field(plans[0], "row_id").size == 103 and int(batches_per_group(plans[0]).max()) == 3
    nv = np.diff(plan_field(plans[0], "row_vptr"))
    assert sorted(nv[nv > 1].tolist()) == [2, 3, 6, 6]                # the rows of 129, 300, 650 and 700 edges


def _owned_phases2(eng, plans):
    assert (eng.class_phases, eng.phase_threshold) == (2, 128)


def _owned_chunk256(eng, plans):
    assert (eng.class_threshold, eng.class_chunk, eng.owned_chunk) == (32, 256, 256)


def _owned_whole_rows(eng, plans):
    # one sum per row, and a (row, class) segment of more than one piece
    assert bool((np.diff(plan_field(plans[0], "row_vptr")) == 1).all()) and eng.owned_chunk == 64
    assert 64 < int(plan_field(plans[0], "seg_len").max()) <= 128


def _owned_rest(eng, plans):
    assert plan_field(plans[0], "row_id").size == 99 and eng.class_rows[0][0].numel() == 103


def _owned_chunks3(overlap):
    def more(eng, plans):
        assert [b.row0 for b in eng.blocks] == [0, 234, 468]              # Zold + (row0 + r) * ldz, Znew + r * ldo
        assert sum(b.nrows for b in eng.blocks) == eng.part.padded_vertices > eng.V
        assert all(int(batches_per_group(p).max()) > 1 for p in plans)    # in every block
        if eng.device.type == "cuda":
            assert (eng.side_streams is not None) == overlap
    return more


def _owned_contiguous(eng, plans):
    _route_contiguous(eng, eng.device)


def _owned_tiles(widths, lanes):
    def more(eng, plans):
        assert [c1 - c0 for c0, c1 in eng.tiles] == widths and eng.tiles[-1][1] == eng.d == 300
        assert lanes_per_row(max(widths), F32) == lanes and eng.owned_batch_vrows == OWNED_SUMS
    return more


def _route_owned_defaults(eng, dev):
    """No setting at all: the engine chose the owned pass by itself, with the shipped constants and its own vertex
    order; the two rows above OWNED_MAX_EDGES stay on chunk + combine."""
    assert eng.beyond_cache and eng.class_affinity and eng.owned_possible and eng.class_owned == xcd.OWNED_DEFAULT is True
    assert eng.hot_rows_first and not bool((eng.pos.cpu() == torch.arange(eng.V)).all())
    assert (eng.owned_groups, eng.owned_block_threads, eng._lds_bytes, eng.owned_row_edges, eng.owned_max_edges,
            eng.owned_loads) == (xcd.OWNED_GROUPS, xcd.OWNED_BLOCK_THREADS, xcd.OWNED_LDS_BYTES, xcd.OWNED_ROW_EDGES,
                                 xcd.OWNED_MAX_EDGES, xcd.OWNED_LOADS) == (256, 1024, 152 * 1024, 1024, 512, 12)
    assert len(eng.blocks) == 1 and len(eng.tiles) == 1 and len(eng.owned_rows) == 1
    plan, rest, n_rest = eng.owned_rows[0]
    assert rest is not None and n_rest == 2 and plan_field(plan, "n_groups") == 256
    assert plan_field(plan, "row_id").size + n_rest == eng.class_rows[0][0].numel() == 7         # above 64 edges


_CHUNKS3 = dict(CLASS_ON, chunks=3, hot_rows_first=False, shuffle=True, seed=SEED + 1, owned_groups=CHUNKS3_GROUPS)
OWNED_DEFAULTS = "owned_defaults_beyond_cache"
OWNED_PLANS = {
    "owned_class": (own(CLASS_ON, class_phases=1), _route_owned(batches=3, steps=[8], more=_owned_class)),
    "owned_phases2": (own(CLASS_ON, class_phases=2, phase_threshold=128), _route_owned(steps=[16], more=_owned_phases2)),
    "owned_chunk256": (own(class_threshold=32, class_chunk=256), _route_owned(more=_owned_chunk256)),
    "owned_whole_rows": (own(CLASS_ON, class_phases=1, owned_row_edges=1024),
                         _route_owned(batches=3, steps=[8], more=_owned_whole_rows)),
    "owned_rest": (own(CLASS_ON, owned_max_edges=128), _route_owned(n_rest=4, more=_owned_rest)),
    "owned_chunks3": (own(_CHUNKS3, overlap_chunks=True), _route_owned(blocks=3, hot=False, more=_owned_chunks3(True))),
    "owned_chunks3_in_order": (own(_CHUNKS3, overlap_chunks=False),
                               _route_owned(blocks=3, hot=False, more=_owned_chunks3(False))),
    "owned_contiguous": (own(CLASS_ON, table_alloc="contiguous"), _route_owned(more=_owned_contiguous)),
    "owned_tiles2": (own(CLASS_ON, width=152, column_tiles=2), _route_owned(tiles=2, more=_owned_tiles([152, 148], 64))),
    "owned_tiles3": (own(CLASS_ON, width=100, column_tiles=3),
                     _route_owned(tiles=3, more=_owned_tiles([100, 100, 100], 32))),
    OWNED_DEFAULTS: (dict(), _route_owned_defaults),
}
OWNED_RUNS = [(((F32, 300) if p.startswith("owned_tiles") else (F32, 128)), p) for p in OWNED_PLANS]


def run_owned_plan(kernels, dev, case, plan, tag=None):
    """run_plan for OWNED_PLANS; the one plan without settings is constructed as if no cache could hold the table."""
    settings, route = OWNED_PLANS[plan]
    tag = plan_id((case, plan)) if tag is None else tag
    constructing = no_infinity_cache if plan == OWNED_DEFAULTS else contextlib.nullcontext
    return run_plan(kernels, dev, engine_case(*case), settings, route, tag, constructing)


def check_owned_plan(kernels, dev, case, plan):
    run_owned_plan(kernels, dev, case, plan).assert_none_failed()


# ---- B: the split route --------------------------------------------------------------------------------------------------
def _route_split(eng, dev):
    assert eng.split_rows[0] is not None and eng.split_rows[0][0].numel() == 2 and _none(eng.class_rows)
    assert eng.segment_edges < SplitGraph.V                      # more than one segment per row, a ragged last one


def _route_split_hubs_to_class(eng, dev):
    assert _none(eng.split_rows) and eng.class_rows[0] is not None


SPLIT_PLANS = {"split": (dict(class_threshold=0), _route_split), "defaults": (dict(), _route_split_hubs_to_class)}


def check_split(kernels, dev, case, plan):
    settings, route = SPLIT_PLANS[plan]
    c = engine_case(case[0], case[1], "split")
    run_plan(kernels, dev, c, settings, route, f"split graph {case_id(case)}-{plan}").assert_none_failed()


# ---- ranks as threads ------------------------------------------------------------------------------------------------
MAX_RANKS = 8


def run_ranks(world, fn, dev):
    """fn(rank, comm) on `world` ranks, threads of this process over tests/thread_comm.ThreadWorld (all on `dev`); a
    rank that fails releases the others.  Returns the ranks' results."""
    assert 1 < world <= MAX_RANKS
    shared, results, errors = ThreadWorld(world), [None] * world, []

    def run(rank):
        try:
            with device_ctx(dev):
                results[rank] = fn(rank, shared.comm(rank))
        except threading.BrokenBarrierError as exc:                # released by the rank that failed
            errors.append((rank, exc))
        except Exception as exc:                                    # surface the failure, release the others
            errors.insert(0, (rank, exc))
            shared.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    assert not any(t.is_alive() for t in threads), "a rank did not finish"
    return results


def owners(results):
    """[V] of (rank, block): who finishes each vertex' row (the first rank that owns it: under the column division
    every rank owns every row)."""
    V = results[0]["blocks"].size
    out = [None] * V
    for rank, res in enumerate(results):
        for v in np.nonzero(res["blocks"] >= 0)[0]:
            if out[v] is None:
                out[v] = (rank, int(res["blocks"][v]))
    return out


# ---- C: divisions ----------------------------------------------------------------------------------------------------
# (dtype, d, exchange, world, fused_pack, class pass)
_DIVISIONS_PER_DTYPE = [("columns", 3, True, False), ("halo", 4, True, False), ("halo", 3, False, False),
                        ("halo_p2p", 3, True, False), ("allgather", 4, True, False), ("allgather_all", 2, True, False)]
DIVISION_RUNS = ([(t, d, *rest) for t, d in ONE_PER_DTYPE for rest in _DIVISIONS_PER_DTYPE]
                 + [(F32, 6, "columns", 4, True, False),            # two packs over four ranks: two hold no columns
                    (F32, 132, "columns", 2, True, False),          # 33 packs: slices of 32 and 16 lanes per row
                    (F32, 100, "columns", 2, True, False)]          # a ragged last pack
                 + [(F32, 64, x, 8, True, False) for x in ("columns", "halo", "halo_p2p", "allgather", "allgather_all")]
                 + [(BF16, 64, "halo", 8, False, False), (F64, 64, "allgather", 8, True, False)]
                 + [(F32, 128, "halo", 3, True, True), (BF16, 128, "halo", 4, False, True),            # the class pass on
                    (BF16, 128, "columns", 3, True, True), (F64, 64, "allgather", 3, True, True),
                    (F32, 128, "halo_p2p", 4, True, True)])


def division_id(run):
    dtype, d, exchange, world, fused, with_class = run
    return (f"{_hip._SUFFIX[dtype]}-d{d}-{exchange}-w{world}" + ("" if fused else "-unfused")
            + ("-class" if with_class else ""))


def division_settings(exchange, fused, with_class):
    return dict(dict(CLASS_ON) if with_class else {}, exchange=exchange, chunks=3, seed=SEED, fused_pack=fused)


def assert_division(eng, exchange, world, fused, with_class=False):
    assert eng.world == world and eng.exchange == exchange
    assert any(m is not None for m in eng.mirrors) == (fused and exchange == "halo")
    assert eng.p2p == (exchange == "halo_p2p") and eng.columns == (exchange == "columns") and len(eng.tiles) == 1
    assert len(eng.blocks) >= 3
    if with_class and eng.d > 0:
        assert _some(eng.class_rows) and eng.class_threshold == 32


def judge_ranks(checks, c, results, judge):
    where = owners(results)
    for rank, out in enumerate(results):
        sub = Checks(f"rank {rank}")
        judge(sub, c, out, where)
        for f in sub.failed:
            checks.record(f[0], False, f"rank {rank}", *f[1:])
        for name in sub.names:
            if name not in sub.failed_names():
                checks.record(name, True)


def run_division(kernels, dev, c, exchange, world, fused, with_class, tag):
    def rank_fn(rank, comm):
        eng = make_engine(kernels, dev, c, comm=comm, **division_settings(exchange, fused, with_class))
        assert_division(eng, exchange, world, fused, with_class)
        return one_sweep(eng, c)

    checks = Checks(tag)
    results = run_ranks(world, rank_fn, dev)
    judge_ranks(checks, c, results, judge_one_sweep)
    return checks


def check_division(kernels, dev, run):
    dtype, d, exchange, world, fused, with_class = run
    c = engine_case(dtype, d)
    run_division(kernels, dev, c, exchange, world, fused, with_class, division_id(run)).assert_none_failed()


# ---- D: consecutive sweeps -------------------------------------------------------------------------------------------
SEQUENCE_PLANS = {"chunks3_class": dict(CLASS_ON, chunks=3, hot_rows_first=False, shuffle=True, seed=SEED),
                  "chunks3_tiles2": dict(chunks=3, column_tiles=2, class_threshold=0, shuffle=True, seed=SEED)}
SEQUENCE_DIVISIONS = [("halo", 3, True), ("halo", 3, False), ("halo_p2p", 3, True), ("allgather", 3, True),
                      ("columns", 3, True)]


def sequence(eng, c):
    """snapshot, sweep, sweep, distance, a launch taken back, a third sweep."""
    out = dict(blocks=block_of_vertex(eng), Z=[], delta=[], pads=[])

    def swept(delta):
        out["delta"].append(delta)
        out["pads"].append(pads_are_zero(eng))
        out["Z"].append(eng.get_Z())

    eng.snapshot()
    swept(eng.sweep(GAMMA))
    swept(eng.sweep(GAMMA))
    out["distance"] = eng.distance_from_snapshot()
    eng.sweep_launch(GAMMA)
    eng.discard_launch()
    out["after_discard"] = eng.get_Z()
    swept(eng.sweep(GAMMA))
    out["distance3"] = eng.distance_from_snapshot()
    return out


def judge_sequence(checks, c, out, blocks=None):
    g = graph()
    blocks = out["blocks"] if blocks is None else blocks
    for s in range(SEQUENCE_SWEEPS):
        judge_table(checks, g, f"Z after sweep {s + 1}", out["Z"][s], c.Z[s + 1], c.Z0, F64, blocks)
        checks.record(f"pad columns after sweep {s + 1}", out["pads"][s])
        judge_delta(checks, f"delta of sweep {s + 1}", out["delta"][s], c.deltas[s])
        if s == 1:
            judge_delta(checks, "snapshot distance after sweep 2", out["distance"], c.distance)
            checks.record("Z after the discarded launch", torch.equal(out["after_discard"], c.Z[2]),
                          differing_rows(g, out["after_discard"], c.Z[2], blocks))
    judge_delta(checks, "snapshot distance after sweep 3", out["distance3"], float((c.Z[3] - c.Z0).abs().sum()))


def run_sequence(kernels, dev, settings, tag):
    c, checks = sequence_case(), Checks(tag)
    with device_ctx(dev):
        eng = make_engine(kernels, dev, c, **settings)
        assert len(eng.blocks) == 3 and (len(eng.tiles) == 2) == ("column_tiles" in settings)
        assert _some(eng.class_rows) == (settings.get("class_threshold") == 32)
        judge_sequence(checks, c, sequence(eng, c))
    return checks


def run_sequence_division(kernels, dev, exchange, world, fused, tag):
    c, checks = sequence_case(), Checks(tag)

    def rank_fn(rank, comm):
        eng = make_engine(kernels, dev, c, comm=comm, **division_settings(exchange, fused, False))
        assert_division(eng, exchange, world, fused)
        return sequence(eng, c)

    judge_ranks(checks, c, run_ranks(world, rank_fn, dev), judge_sequence)
    return checks


def check_sequence(kernels, dev, plan):
    run_sequence(kernels, dev, SEQUENCE_PLANS[plan], f"sequence {plan}").assert_none_failed()


def check_sequence_division(kernels, dev, exchange, world, fused):
    run_sequence_division(kernels, dev, exchange, world, fused,
                          f"sequence {exchange}-w{world}{'' if fused else '-unfused'}").assert_none_failed()
