"""The exact engine-level sweeps of tests/engine_exact_cases.py, without a GPU: every case builder's range assertion,
the single-dropped-edge sensitivity for the sorted P order, every check of tests/test_gpu_engine_exact.py run through
the CPU test double with the same torch.equal / == comparisons -- which proves the fixtures exact and the expectations
right before SweepEngine ever drives a HIP kernel against them -- and mutation self-checks: a wrapping double that is
wrong in one named way must fail the named comparison and no other (a moved table element also moves the snapshot
distance, which is read off the same table: the two are named together).  The double is the one with the owned class
pass (tests/owned_oracle_kernels.py): the OWNED_PLANS run through it, and their mutations edit the plan it is handed or
what it leaves behind."""
import dataclasses
import functools
import inspect
import threading

import numpy as np
import pytest
import torch

from . import engine_exact_cases as X
from .exact_cases import BF16, F32, F64
from .owned_oracle_kernels import OracleKernels          # the plain double plus spmm_update_owned

DEV = "cpu"


@pytest.fixture(scope="module")
def k():
    return OracleKernels()


# ---- the fixtures ----------------------------------------------------------------------------------------------------
def test_split_graph_reaches_the_split_route_and_nothing_else_does():
    g, s = X.graph(), X.graph("split")
    assert g.deg.max() <= X.SPLIT_EDGES < s.deg.max() == s.V
    assert sorted(s.deg[s.deg > 12].tolist()) == [129, 300, s.V, s.V]
    for r in range(s.V):                                      # sorted, unique rows: what HostCSR promises
        assert (np.diff(s.sorted_colidx[s.rowptr[r]:s.rowptr[r + 1]]) > 0).all()


@pytest.mark.parametrize("case", X.ENGINE_CASES + [(F32, 6), (F32, 100), (F32, 132), (BF16, 64), (F64, 64)], ids=X.case_id)
def test_engine_case_is_exact_and_notices_every_dropped_edge(case):
    """Building the case asserts the range condition.  exact_cases.K3Case's sensitivity restated for P in the sorted
    edge order: for d >= 16 no single edge of the longest row (700 edges, the first 600 tried) may vanish without
    changing the expected storage-dtype row."""
    c = X.engine_case(*case)
    assert c.bound * 8 < X.E.EXACT_LIMIT
    tried, undetected = c.undetected_single_edge_drops()
    assert tried == 600
    if c.d >= 16:
        assert undetected == 0, (X.case_id(case), undetected)


@pytest.mark.parametrize("case", X.SPLIT_CASES, ids=X.case_id)
def test_split_case_is_exact_and_notices_every_dropped_edge(case):
    c = X.engine_case(case[0], case[1], "split")
    assert c.bound * 8 < X.E.EXACT_LIMIT and c.d * (c.bound + 4) * 8 < X.E.EXACT_LIMIT
    tried, undetected = c.undetected_single_edge_drops()
    assert (tried, undetected) == (600, 0)


def test_sequence_case_stays_within_its_bit_budget():
    """SequenceCase asserts 2^53 quanta against its bounds sweep by sweep; here, the figures: after three sweeps the
    largest value needs fewer than 44 bits, the total delta fewer than 49, and the third sweep still moves most rows."""
    c = X.sequence_case()
    assert float(c.Z[3].abs().max()) * 2.0 ** 39 < 2.0 ** 44 and c.deltas[2] * 2.0 ** 39 < 2.0 ** 49
    assert c.deltas[0] > c.deltas[1] > c.deltas[2] > 0 and c.distance != c.deltas[0] + c.deltas[1]
    moved = (c.Z[3] != c.Z[2]).any(1)
    sink = X.graph().sink                       # a row that reads only sinks is at its fixed point after one sweep
    assert int(moved[~sink].sum()) > 400 and not bool(moved[sink].any())


def test_load_P_is_the_inverse_of_P_global(k):
    c = X.engine_case(F32, 128)
    eng = X.make_engine(k, DEV, c, **X.PLANS["chunks3_class"][0])
    assert not np.array_equal(eng.local.edge_origin, np.arange(eng.E_loc)) and torch.equal(eng.P_global(), c.P.float())

    def rank_fn(rank, comm):
        eng = X.make_engine(k, DEV, c, comm=comm, **X.division_settings("halo", True, True))
        return eng.P_global(), eng.local.edge_origin

    E_all = X.graph().E
    seen = torch.zeros(E_all)
    for P, origin in X.run_ranks(3, rank_fn, DEV):
        full, own = torch.zeros(E_all), torch.zeros(E_all, dtype=torch.bool)
        full[:P.numel()] = P
        own[torch.from_numpy(origin)] = True
        assert torch.equal(full[own], c.P.float()[own]) and float(full[~own].abs().sum()) == 0
        seen += own
    assert bool((seen == 1).all())                            # every edge on exactly one rank


# ---- the checks on the double ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", X.PLAN_RUNS, ids=X.plan_id)
def test_one_gpu_plans_on_the_double(k, run):
    X.check_plan(k, DEV, *run)


@pytest.mark.parametrize("run", X.OWNED_RUNS, ids=X.plan_id)
def test_owned_plans_on_the_double(k, run):
    X.check_owned_plan(k, DEV, *run)


def test_owned_plans_cover_what_they_are_there_for(k):
    """What no route can see from one engine: between them the plans run 8, 16 and 32 steps, pieces of 64 and 256, sums
    of 512 bytes and 1 KiB, segments of one edge, and launch blocks whose first row is not row 0."""
    seen = dict(steps=set(), chunk=set(), lanes=set(), row0=set(), shortest=10 ** 9)
    for case, plan in X.OWNED_RUNS:
        with X.no_infinity_cache() if plan == X.OWNED_DEFAULTS else X.contextlib.nullcontext():
            eng = X.make_engine(k, DEV, X.engine_case(*case), **X.OWNED_PLANS[plan][0])
        for b, o in zip(eng.blocks, eng.owned_rows):
            seen["steps"].add(o[0]["n_steps"])
            seen["chunk"].add(o[0]["chunk"])
            seen["row0"].add(b.row0)
            seen["shortest"] = min(seen["shortest"], int(o[0]["seg_len"].min()))
        seen["lanes"].add(X.lanes_per_row(max(c1 - c0 for c0, c1 in eng.tiles), F32))
    assert seen == dict(steps={8, 16, 32}, chunk={64, 256}, lanes={32, 64}, row0={0, 234, 468}, shortest=1)


@pytest.mark.parametrize("plan", list(X.SPLIT_PLANS))
@pytest.mark.parametrize("case", X.SPLIT_CASES, ids=X.case_id)
def test_split_route_on_the_double(k, case, plan):
    X.check_split(k, DEV, case, plan)


@pytest.mark.parametrize("run", X.DIVISION_RUNS, ids=X.division_id)
def test_divisions_on_the_double(k, run):
    X.check_division(k, DEV, run)


@pytest.mark.parametrize("plan", list(X.SEQUENCE_PLANS))
def test_consecutive_sweeps_on_the_double(k, plan):
    X.check_sequence(k, DEV, plan)


@pytest.mark.parametrize("exchange,world,fused", X.SEQUENCE_DIVISIONS)
def test_consecutive_sweeps_under_a_division_on_the_double(k, exchange, world, fused):
    X.check_sequence_division(k, DEV, exchange, world, fused)


def test_run_ranks_reports_the_rank_that_failed_first():
    def rank_fn(rank, comm):
        if rank == 1:
            raise ValueError("rank 1 is wrong")
        comm.all_gather_object(rank)

    with pytest.raises(AssertionError, match="rank 1 is wrong") as info:
        X.run_ranks(3, rank_fn, DEV)
    assert info.value.args[0][0][0] == 1


# ---- mutation self-checks ------------------------------------------------------------------------------------------------
class Mutant(OracleKernels):
    """The double, wrong in one way."""

    def __init__(self, what):
        self.what, self.calls, self.tls = what, 0, threading.local()

    def spmm_update(self, rowptr, colidx, P, nrows, row0, Z_old, X_, gamma, Z_new, d, long_threshold, partials, **kw):
        super().spmm_update(rowptr, colidx, P, nrows, row0, Z_old, X_, gamma, Z_new, d, long_threshold, partials, **kw)
        self.tls.Z_old = Z_old
        if self.what == "partial_left_out" and self.calls == 0:        # one row's |new - old| never reaches the delta
            deg = np.diff(rowptr[:nrows + 1].numpy())
            r = int(np.nonzero((deg > 0) & ((deg <= long_threshold) | (long_threshold == 0)))[0][5])
            partials[0] -= float((Z_new[r, :d].double() - Z_old[row0 + r, :d].double()).abs().sum())
            self.calls += 1

    def spmm_update_class(self, colidx, P, item_e0, item_len, item_slot, items_per_block, class_rows, slot_ptr, row0,
                          Z_old, X_, gamma, Z_new, d, slab, partials, **kw):
        super().spmm_update_class(colidx, P, item_e0, item_len, item_slot, items_per_block, class_rows, slot_ptr, row0,
                                  Z_old, X_, gamma, Z_new, d, slab, partials, **kw)
        if self.what == "class_element_moved":                         # by one quantum of the recipe
            Z_new[int(class_rows[1]), d - 1] += 0.125

    def spmm_update_owned(self, colidx, P, plan, block_threads, row0, Z_old, X_, gamma, Z_new, d, partials, **kw):
        """The owned pass, wrong in one way: through the plan it is handed, or through what it leaves behind."""
        S, chunk = plan["n_steps"], plan["chunk"]
        if self.what == "owned_partials_from_slot_0":                  # not after the chunk + combine rows' slots
            plan = dict(plan, row_part=plan["row_part"] - plan["row_part"].min())
        if self.what == "owned_last_piece_dropped":                    # of every segment of several pieces
            ln = plan["seg_len"]
            plan = dict(plan, seg_len=np.where(ln > chunk, (ln - 1) // chunk * chunk, ln).astype(np.int32))
        if self.what == "owned_last_virtual_row_left_out":             # its segments never run: the sum stays zero
            seg_bat = (np.searchsorted(plan["bat_seg_ptr"], np.arange(plan["seg_len"].size), side="right") - 1) // S
            last = plan["row_vptr"][1:][np.diff(plan["row_vptr"]) > 1] - 1
            keep = ~np.isin(plan["bat_vrow_ptr"][seg_bat] + plan["seg_vrow"], last)
            kept_before = np.concatenate([[0], np.cumsum(keep)])
            plan = dict(plan, bat_seg_ptr=kept_before[plan["bat_seg_ptr"]].astype(np.int32),
                        **{name: plan[name][keep] for name in ("seg_e0", "seg_len", "seg_vrow")})
        super().spmm_update_owned(colidx, P, plan, block_threads, row0, Z_old, X_, gamma, Z_new, d, partials, **kw)
        rows = torch.from_numpy(plan["row_id"].astype(np.int64))
        if self.what == "owned_old_row_without_row0":                  # |new - Z_old[r]| instead of |new - Z_old[row0 + r]|
            partials[torch.from_numpy(plan["row_part"].astype(np.int64))] = \
                (Z_new[rows, :d].double() - Z_old[rows, :d].double()).abs().sum(1)
        if self.what == "owned_last_batch_not_stored":                 # of the first group that has several
            gb = plan["grp_bat_ptr"]
            b = int(gb[1:][np.diff(gb) > 1][0]) - 1
            skipped = rows[plan["bat_row_ptr"][b]:plan["bat_row_ptr"][b + 1]]
            Z_new[skipped, :d] = Z_old[row0 + skipped, :d]

    def gather_rows(self, src, idx, d, dst):
        if self.what == "halo_rows_one_sweep_late":                    # the rows as they were BEFORE this sweep
            src = self.tls.Z_old
        super().gather_rows(src, idx, d, dst)

    def l1_distance(self, A, B, d, ws, out, sq_a=None):
        super().l1_distance(A, B, d, ws, out, sq_a=sq_a)
        self.calls += 1
        if self.what == "l1_skips_a_block" and self.calls == 2:
            out[0] = 0.0


ONE_SWEEP_NAMES = ["Z", "Z sinks", "pad columns", "delta", "snapshot distance"]


def _plan(kernels, case, plan):
    settings, route = X.PLANS[plan]
    return X.run_plan(kernels, DEV, X.engine_case(*case), settings, route, plan)


def test_unmutated_wrapper_passes_and_every_comparison_is_made():
    checks = _plan(Mutant(None), (F32, 128), "chunks3_class")
    assert checks.names == ONE_SWEEP_NAMES and checks.failed == []


def test_mutation_a_rows_partial_left_out_of_the_delta():
    checks = _plan(Mutant("partial_left_out"), (F32, 128), "row_pass_only")
    assert checks.names == ONE_SWEEP_NAMES and checks.failed_names() == ["delta"]
    (name, got, want, off, _, blocks), = checks.failed
    assert off < 0 and blocks == [(0, got, want)]                  # the message names the block that is short


def test_mutation_one_element_of_a_class_row_moved_by_a_quantum():
    """The table is wrong, the returned delta (made of the kernels' partials) is not.  The snapshot distance is read
    off the same table, so it moves by the same quantum: it cannot pass, and is named next to Z."""
    checks = _plan(Mutant("class_element_moved"), (F32, 128), "class_chunk64")
    assert checks.names == ONE_SWEEP_NAMES and checks.failed_names() == ["Z", "snapshot distance"]
    name, _, rows = checks.failed[0]
    g = X.graph()
    assert len(rows) == 1 and rows[0][1] == int(g.deg[rows[0][0]]) > 32 and rows[0][2] == 0
    assert abs(checks.failed[1][3]) == 0.125


def test_mutation_halo_rows_handed_over_one_sweep_late():
    """Unfused halo (gather_rows packs the send buffer) fed the rows of the table the sweep READ: every single-sweep
    comparison still passes (a rank's read-outs cover its own rows), the second consecutive sweep does not."""
    mutant = Mutant("halo_rows_one_sweep_late")
    single = X.run_division(mutant, DEV, X.engine_case(F64, 64), "halo", 3, False, False, "late halo, one sweep")
    assert single.failed == [] and set(single.names) == set(ONE_SWEEP_NAMES)
    failed = X.run_sequence_division(mutant, DEV, "halo", 3, False, "late halo, sequence").failed_names()
    assert failed[0] == "Z after sweep 2" and "delta of sweep 2" in failed
    assert not any(name.endswith("sweep 1") for name in failed)
    X.run_sequence_division(Mutant(None), DEV, "halo", 3, False, "wrapper alone").assert_none_failed()


def test_mutation_l1_distance_skips_a_block():
    checks = _plan(Mutant("l1_skips_a_block"), (F32, 128), "chunks3_in_order")
    assert checks.names == ONE_SWEEP_NAMES and checks.failed_names() == ["snapshot distance"]
    sequence = X.run_sequence(Mutant("l1_skips_a_block"), DEV, X.SEQUENCE_PLANS["chunks3_class"], "l1 skips a block")
    assert sequence.failed_names() == ["snapshot distance after sweep 2"]


# ---- every delta slot is written by exactly one launch -----------------------------------------------------------------
class SlotRecorder(OracleKernels):
    """The double with every K3 call of a sweep replaced by a note of the block's first row and the delta slots the
    call is to write: from the storage offset of its `partials` view on, the row pass' grid length, one per listed
    row, or the plan's row_part.  (What the calls compute is the other tests' matter.)"""

    def __init__(self):
        self.writes = []                                               # (method, row0, slots of eng.partials)

    def bind(self, method, *args, **kwargs):
        if not method.startswith("spmm_update"):
            return super().bind(method, *args, **kwargs)
        a = inspect.signature(getattr(self, method)).bind(*args, **kwargs).arguments
        if method == "spmm_update":
            slots = np.arange(self.spmm_partials_len(a["nrows"], 0))
        elif method == "spmm_update_owned":
            slots = np.asarray(a["plan"]["row_part"], dtype=np.int64)
        else:
            slots = np.arange(next(a[n] for n in ("long_rows", "split_rows", "class_rows") if n in a).numel())
        write = (method, a["row0"], a["partials"].storage_offset() + slots)
        return lambda: self.writes.append(write)


def delta_slot_faults(eng, writes):
    """What is wrong with the slots the K3 calls of ONE sweep wrote; [] when they are pairwise disjoint, cover every
    column tile's [0, partial_off[-1]) exactly and stay inside their block's [partial_off[i], partial_off[i + 1])."""
    off, faults = eng.partial_off, []
    block = {b.row0: i for i, b in enumerate(eng.blocks)}
    for method, row0, slots in writes:
        i, within = block[row0], slots % off[-1]
        if slots.size and not (off[i] <= within.min() and within.max() < off[i + 1]):
            faults.append(f"{method} of block {i} leaves [{off[i]}, {off[i + 1]}): {within.min()}..{within.max()}")
    every = np.concatenate([slots for _, _, slots in writes])
    if np.unique(every).size != every.size:
        faults.append(f"{every.size - np.unique(every).size} slots are written twice")
    if not np.array_equal(np.sort(every), np.arange(len(eng.tiles) * off[-1])):
        faults.append(f"{np.unique(every).size} of {len(eng.tiles) * off[-1]} slots are written")
    return faults


@functools.lru_cache(maxsize=None)
def _slot_engine(run, before_sweep=None):
    """The engine of one (case, plan) over a SlotRecorder after one sweep, and the recorder's writes.  Made once per
    run; nobody sweeps it again."""
    kind, case, plan = run
    settings = {"plan": X.PLANS, "owned": X.OWNED_PLANS, "split": X.SPLIT_PLANS}[kind][plan][0]
    c = X.engine_case(case[0], case[1], "split" if kind == "split" else "ragged")
    rec = SlotRecorder()
    with X.no_infinity_cache() if plan == X.OWNED_DEFAULTS else X.contextlib.nullcontext():
        eng = X.make_engine(rec, DEV, c, **settings)
    if before_sweep is not None:
        before_sweep(eng)
    eng.sweep(X.GAMMA)
    return eng, rec.writes


# every plan once: the one-GPU plans on the first case they are run at, the owned plans, the split plans
SLOT_RUNS = ([("plan", next(c for c, q in X.PLAN_RUNS if q == p and (not p.startswith("tiles") or c[1] == 300)), p)
              for p in X.PLANS] + [("owned", c, p) for c, p in X.OWNED_RUNS]
             + [("split", X.SPLIT_CASES[0], p) for p in X.SPLIT_PLANS])


@pytest.mark.parametrize("run", SLOT_RUNS, ids=lambda run: f"{run[0]}-{X.plan_id(run[1:])}")
def test_every_delta_slot_is_written_by_exactly_one_launch(run):
    """The layout of a block's delta partials (blocks.PartialLayout) against what the launches do with it: two
    launches sharing slots, or a slot nobody writes, change the delta by a few rows' worth -- nothing a convergence
    loop would notice."""
    eng, writes = _slot_engine(run)
    methods = {m for m, _, _ in writes}
    assert "spmm_update" in methods and len(writes) >= len(eng.blocks) * len(eng.tiles)
    assert ("spmm_update_owned" in methods) == (run[0] == "owned")
    assert delta_slot_faults(eng, writes) == []


def test_slot_runs_reach_every_bin_and_division():
    """Between them: every K3 kernel, both widths of the long-row kernel in one block, several blocks, several
    tiles, owned rows with and without rows beside them."""
    seen = dict(methods=set(), blocks=set(), tiles=set(), owned=set(), both_long=False)
    for run in SLOT_RUNS:
        eng, writes = _slot_engine(run)
        seen["methods"] |= {m for m, _, _ in writes}
        seen["blocks"].add(len(eng.blocks))
        seen["tiles"].add(len(eng.tiles))
        seen["owned"] |= {o.rest is not None for o in eng.owned_rows if o is not None}
        seen["both_long"] |= any(r.mid is not None and r.hub is not None for r in eng.block_rows)
    assert seen == dict(methods={"spmm_update", "spmm_update_long", "spmm_update_split", "spmm_update_class",
                                 "spmm_update_owned"}, blocks={1, 3}, tiles={1, 2, 3}, owned={False, True}, both_long=True)


def test_mutation_layout_puts_the_16_wave_rows_on_the_4_wave_rows_slots():
    """A PartialLayout whose `hub` start is its `mid` start: the slot check names it, and of the exact comparisons
    the delta -- the 4-wave launch overwrites what the 16-wave rows left -- and nothing else."""
    def mutate(eng):
        for r in eng.block_rows:
            r.partials = dataclasses.replace(r.partials, hub=r.partials.mid)

    run = ("plan", (F32, 128), "bins_4_and_16_waves")
    eng, writes = _slot_engine(run, mutate)
    faults = delta_slot_faults(eng, writes)
    n_hub, n = eng.hub_rows[0].numel(), eng.partial_off[-1]
    assert 0 < n_hub <= eng.mid_rows[0].numel()
    assert faults == [f"{n_hub} slots are written twice", f"{n - n_hub} of {n} slots are written"]
    assert delta_slot_faults(*_slot_engine(run)) == []

    def route(eng, dev):
        X.PLANS[run[2]][1](eng, dev)
        mutate(eng)
    checks = X.run_plan(OracleKernels(), DEV, X.engine_case(*run[1]), X.PLANS[run[2]][0], route, "hub on mid")
    assert checks.names == ONE_SWEEP_NAMES and checks.failed_names() == ["delta"]
    assert checks.failed[0][3] < 0 and checks.failed[0][5][0][0] == 0          # short, and block 0 is named


# ---- mutation self-checks of the owned plans ---------------------------------------------------------------------------
def _owned(kernels, plan):
    case = next(c for c, p in X.OWNED_RUNS if p == plan)
    return X.run_owned_plan(kernels, DEV, case, plan)


@pytest.mark.parametrize("plan", ["owned_class", "owned_whole_rows", "owned_rest", "owned_chunks3", X.OWNED_DEFAULTS])
def test_unmutated_wrapper_passes_the_owned_plans_and_every_comparison_is_made(plan):
    checks = _owned(Mutant(None), plan)
    assert checks.names == ONE_SWEEP_NAMES and checks.failed == []


def test_mutation_owned_old_row_read_without_row0():
    """Only the delta can tell: the table is right.  Block 0 (row0 = 0) is right too, and the message says so."""
    checks = _owned(Mutant("owned_old_row_without_row0"), "owned_chunks3")
    assert checks.names == ONE_SWEEP_NAMES and checks.failed_names() == ["delta"]
    (name, got, want, off, _, blocks), = checks.failed
    assert [b[0] for b in blocks] == [1, 2]
    assert _owned(Mutant("owned_old_row_without_row0"), "owned_class").failed == []         # one block: nothing to see


def test_mutation_owned_partials_written_from_slot_0():
    """The four rows on chunk + combine write slots 0..3 after the owned launch did: four owned rows' partials are
    lost, and the last four slots are never written."""
    checks = _owned(Mutant("owned_partials_from_slot_0"), "owned_rest")
    assert checks.names == ONE_SWEEP_NAMES and checks.failed_names() == ["delta"]
    assert checks.failed[0][5][0][0] == 0 and checks.failed[0][3] != 0
    assert _owned(Mutant("owned_partials_from_slot_0"), "owned_class").failed == []     # no rows beside it: slot 0 is right


def _rows_of_the_failed_table(checks):
    name, _, rows = checks.failed[0]
    assert name == "Z" and rows
    return rows


def test_mutation_owned_last_virtual_row_left_out():
    checks = _owned(Mutant("owned_last_virtual_row_left_out"), "owned_class")
    assert checks.names == ONE_SWEEP_NAMES and checks.failed_names() == ["Z", "delta", "snapshot distance"]
    rows = _rows_of_the_failed_table(checks)
    assert sorted(deg for _, deg, _ in rows) == [129, 300, 650, 700] and all(deg > 128 for _, deg, _ in rows)
    assert _owned(Mutant("owned_last_virtual_row_left_out"), "owned_whole_rows").failed == []   # no virtual rows there


def test_mutation_owned_last_piece_of_a_segment_dropped():
    checks = _owned(Mutant("owned_last_piece_dropped"), "owned_whole_rows")
    assert checks.names == ONE_SWEEP_NAMES and checks.failed_names() == ["Z", "delta", "snapshot distance"]
    assert sorted(deg for _, deg, _ in _rows_of_the_failed_table(checks)) == [650, 700]     # segments of some 87 edges
    assert _owned(Mutant("owned_last_piece_dropped"), "owned_class").failed == []           # virtual rows: one piece each


def test_mutation_owned_last_batch_of_a_group_not_stored():
    """Its rows keep their old values; their partials were computed from the new ones, so the delta is right."""
    checks = _owned(Mutant("owned_last_batch_not_stored"), "owned_class")
    assert checks.names == ONE_SWEEP_NAMES and checks.failed_names() == ["Z", "snapshot distance"]
    rows = _rows_of_the_failed_table(checks)
    assert 1 <= len(rows) <= X.OWNED_SUMS and all(deg > 32 and block == 0 for _, deg, block in rows)
