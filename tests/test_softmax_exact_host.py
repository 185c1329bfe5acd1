"""The exact softmax cases of tests/softmax_cases.py, without a GPU: the range condition of every fixture, the row kinds
the assignments are there for, plain-torch mutants of a chunked softmax (each must move an expected bit wherever its fault
can occur -- the fixtures are sensitive before a kernel is ever compared with them), and every check of
tests/test_gpu_softmax_exact.py run through the CPU test double with the same assertions."""
import numpy as np
import pytest
import torch

from . import exact_cases as E
from . import softmax_cases as S
from .test_exact_host import ExactOracleKernels

DEV = "cpu"
ids = E.case_id


@pytest.fixture(scope="module")
def k():
    return ExactOracleKernels()


# ---- the fixtures ------------------------------------------------------------------------------------------------------
def test_exp_is_exact_where_the_recipe_needs_it():
    for dtype in (S.F32, S.F64):
        x = torch.tensor([0.0, -float(S.LEVEL_GAP), -float("inf")], dtype=dtype)
        assert torch.exp(x).tolist() == [1.0, 0.0, 0.0]
    c = torch.arange(2, 100_001, dtype=S.F32)
    assert bool((1 / c != 1 / (c - 1)).all())                 # one lost or double-counted top-level edge moves a bit


def test_graphs_have_the_rows_the_routes_need():
    small, big = S.graph("small"), S.graph("big")
    assert small.V == E.V and set(E.HUBS) <= set(small.deg.tolist()) and small.class_rows.size >= 6
    assert big.V == S.BIG_V and sorted(big.deg[big.class_rows].tolist()) == list(S.BIG_HUBS)
    for g in (small, big):
        assert (g.deg == 0).sum() > 50 and g.rows_above(48).size >= 3
        r0, n = S.ROW_BLOCK
        assert g.deg[r0:r0 + n].max() == g.deg.max() and g.deg[:r0].max() > 0 and g.deg[r0 + n:].max() > 0
        for r in g.class_rows:                                 # sorted rows; class rows sorted by (class, column)
            assert (np.diff(g.sorted_colidx[g.rowptr[r]:g.rowptr[r + 1]]) > 0).all()
    # 16 waves over the hubs: slices of 2, 3 and 5 chunks of 64 edges
    assert [-(-(-(-h // 16)) // 64) for h in S.BIG_HUBS] == [2, 3, 5]


@pytest.mark.parametrize("gname", S.GRAPHS)
def test_range_condition_of_every_table(gname):
    """Building a case asserts 14400 |a| + |b| < 2^24; counting asserts that inside a row every score is the maximum or at
    least 900 below it.  Every d the card's tests use, single and pair."""
    widths = {c[1] for c in E.LAYOUT_CASES + S.BIG_CASES + S.CLASS_CASES} | {40}
    for a in S.ASSIGNMENTS:
        for d in sorted(widths):
            L = S.Levelled(gname, a, d)
            if d in (3, 40, 1433 if gname == "small" else 520):
                S.count_expectation(L.g, L.dots("sorted"), S.F32)
        for _, d in S.PAIR_CASES:
            L = S.Levelled(gname, a, d, True)
            S.count_expectation(L.g, L.dots("class"), S.F32)
        for t in (L.table(), L.pair_table()):
            assert t.to(S.BF16).double().equal(t)              # the levels are exact in bf16


def _kinds(g, top):
    kinds = set()
    for r in np.nonzero(g.deg > 64)[0]:
        t = top[g.rowptr[r]:g.rowptr[r + 1]]
        if t.all():
            kinds.add("all_equal")
        else:
            first, last = np.nonzero(t)[0][[0, -1]]
            if last < 64:
                kinds.add("maximum_first")                     # in the first chunk and nowhere after it
            if first >= t.size - 1 - (t.size - 1) % 64 or (first >= 64 and last == t.size - 1):
                kinds.add("maximum_last")                      # only in the last chunk / arrives late and stays to the end
            if t.sum() == 1:
                kinds.add("single_maximum")
    return kinds


@pytest.mark.parametrize("gname", S.GRAPHS)
def test_every_row_kind_is_present(gname):
    g = S.graph(gname)
    a, b = g.rowptr[g.longest], g.rowptr[g.longest + 1]
    tops = {}
    for name in S.ASSIGNMENTS:
        L = S.levelled(gname, name, 3)
        tops[name] = S.count_expectation(g, L.dots("sorted"), S.F32)[1]
    assert {"all_equal", "maximum_first", "maximum_last"} <= _kinds(g, tops["thirds"])
    assert {"all_equal", "single_maximum", "maximum_last"} <= _kinds(g, tops["last"])
    hub = tops["last"][a:b]
    assert hub.sum() == 1 and hub[-1]                           # the single maximum is the last edge of the last chunk
    hub = np.nonzero(tops["middle"][a:b])[0]
    m = (b - a) // 64 // 2
    assert hub.size == 64 and hub[0] == 64 * m and hub[-1] == 64 * m + 63 and 0 < m < (b - a) // 64
    s_hub = S.levels(gname, "random")[g.longest]
    if s_hub != 0:                                              # ties in every 64-edge chunk of the hub: all waves, all slots
        hub = tops["random"][a:b]
        assert all(hub[i:i + 64].any() for i in range(0, b - a, 64))
    assert (S.levels(gname, "random") == 0).sum() > g.V // 4


# ---- mutants of a chunked softmax ---------------------------------------------------------------------------------------
def _online(x, mutant=None):
    """{max, sum of exp} of x over 64-element chunks, as score_edge_range keeps them.  Returns (max, sum, whether the
    mutant's fault could occur)."""
    run_m, run_s, fault = torch.tensor(-float("inf"), dtype=x.dtype), torch.zeros((), dtype=x.dtype), False
    drop = int(np.nonzero((x == x.max()).numpy())[0][-1])
    for a in range(0, x.numel(), 64):
        v = x[a:a + 64]
        new_m = torch.maximum(run_m, v.max())
        ex = torch.exp(v - new_m)
        if mutant == "drops_a_top_element" and a <= drop < a + 64:
            ex[drop - a] = 0
            fault = True
        if mutant == "skips_the_rescale":
            fault = fault or bool(run_s > 0) and bool(new_m > run_m)
            run_s = run_s + ex.sum()
        else:
            run_s = run_s * torch.exp(run_m - new_m) + ex.sum()
        run_m = new_m
    return run_m, run_s, fault


def chunked_softmax(x, mutant=None):
    """One wave over the row's chunks, or (mutant "adds_slices_unscaled" and its sound twin "slices") 16 wave slices
    whose {max, sum} are combined afterwards; "normalises_twice" soft-maxes the result again."""
    if mutant in ("slices", "adds_slices_unscaled"):
        seg = -(-(-(-x.numel() // 16)) // 64) * 64
        parts = [_online(x[a:a + seg])[:2] for a in range(0, x.numel(), seg)]
        m = torch.stack([p[0] for p in parts]).max()
        fault = any(bool(pm < m) and bool(ps > 0) for pm, ps in parts)
        if mutant == "slices":
            total = sum(ps * torch.exp(pm - m) for pm, ps in parts)
        else:
            total = sum(ps for _, ps in parts)
    else:
        m, total, fault = _online(x, mutant)
    p = torch.exp(x - m) / total
    if mutant == "normalises_twice":
        p, fault = torch.exp(p - p.max()) / torch.exp(p - p.max()).sum(), True
    return p, fault


MUTANTS = ("drops_a_top_element", "skips_the_rescale", "adds_slices_unscaled", "normalises_twice")
# where a mutant's fault must be able to occur: a maximum that arrives after the first chunk / that a slice lacks
FAULT_MUST_OCCUR = {"drops_a_top_element": S.ASSIGNMENTS, "normalises_twice": S.ASSIGNMENTS,
                    "skips_the_rescale": ("thirds", "last", "middle"), "adds_slices_unscaled": ("thirds", "last", "middle")}


@pytest.mark.parametrize("dtype", [S.F32, S.F64])
@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("gname", S.GRAPHS)
def test_mutants_of_a_chunked_softmax_move_a_bit(gname, assignment, dtype):
    """The sound chunked evaluations give the counted expectation bit for bit; every mutant differs from it on every row
    where its fault occurs (normalising twice: on the assignment -- an all-equal row is its own fixed point), and the
    fault does occur on the assignments built for it."""
    g = S.graph(gname)
    L = S.levelled(gname, assignment, 3)
    dots, want = torch.from_numpy(L.dots("sorted")).to(dtype), L.want("sorted", dtype)
    rows = np.nonzero(g.deg > (0 if gname == "small" else 12))[0]
    occurred = dict.fromkeys(MUTANTS, 0)
    noticed = dict.fromkeys(MUTANTS, 0)
    for r in rows:
        a, b = g.rowptr[r], g.rowptr[r + 1]
        for sound in (None, "slices"):
            assert torch.equal(chunked_softmax(dots[a:b], sound)[0], want[a:b]), (r, sound)
        for mutant in MUTANTS:
            got, fault = chunked_softmax(dots[a:b], mutant)
            differs = not torch.equal(got, want[a:b])
            assert fault or not differs, (mutant, r)
            if mutant != "normalises_twice":
                assert differs == fault, (mutant, int(r), int(g.deg[r]))
            occurred[mutant] += fault
            noticed[mutant] += differs
    for mutant in MUTANTS:
        assert noticed[mutant] > 0 or not occurred[mutant], mutant
        if assignment in FAULT_MUST_OCCUR[mutant]:
            assert noticed[mutant] > 0, mutant


# ---- every check of the card's file, through the double -------------------------------------------------------------------
@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("case", E.LAYOUT_CASES, ids=ids)
def test_fused_rows_on_the_double(k, case, assignment):
    S.check_fused_rows(k, DEV, "small", assignment, case)


@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("case", [(S.F32, 128, True), (S.BF16, 70, False)], ids=ids)
def test_fused_rows_of_the_big_graph_on_the_double(k, case, assignment):
    S.check_fused_rows(k, DEV, "big", assignment, case)
    S.check_column_split_route(k, DEV, "big", assignment, case)


@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("case", S.CLASS_CASES, ids=ids)
def test_fused_class_rows_on_the_double(k, case, assignment):
    for chunk in (64, 256):
        S.check_fused_class(k, DEV, "small", assignment, case, chunk)
    if case[1] == 128:
        S.check_fused_class(k, DEV, "big", assignment, case, 64)
    S.check_column_split_route(k, DEV, "small", assignment, case)


@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("dtype,d", [(S.F32, 64), (S.F64, 3)])
def test_fused_pair_on_the_double(k, dtype, d, assignment):
    S.check_fused_pair(k, DEV, "small", assignment, dtype, d)
    if d == 3:
        S.check_fused_pair(k, DEV, "big", assignment, dtype, d)


@pytest.mark.parametrize("setting", sorted(S.SEGMENT_SETTINGS))
@pytest.mark.parametrize("dtype", [S.F32, S.F64])
def test_segment_softmax_settings_on_the_double(k, dtype, setting):
    for assignment in S.ASSIGNMENTS:
        S.check_segment_softmax(k, DEV, "small", assignment, dtype, setting)
    S.check_segment_softmax(k, DEV, "big", "thirds", dtype, setting)


def test_the_double_rejects_long_rows_without_max_degree(k):
    g = S.graph("small")
    with pytest.raises(ValueError):
        k.segment_softmax(torch.from_numpy(g.rowptr), g.V, torch.zeros(g.E), 0, 0, torch.from_numpy(g.rows_above(64)))


@pytest.mark.parametrize("route", sorted(S.ENGINE_SETTINGS))
@pytest.mark.parametrize("dtype", [S.F32, S.F64])
def test_engine_bilinear_on_the_double(k, dtype, route):
    for assignment in S.ASSIGNMENTS:
        S.check_engine_bilinear(k, DEV, "small", assignment, dtype, route)
    S.check_engine_bilinear(k, DEV, "big", "last", dtype, route)


# ---- the real-valued check ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [S.F32, S.F64])
def test_torch_softmax_itself_meets_the_bound(dtype):
    """The bound is 4 x the recorded worst error of torch.softmax over all the real-valued scores; re-measured on the
    scores that set the record, torch must at least pass what the kernels are asked (the figure is printed)."""
    worst = 0.0
    for gname, d, pair in (("big", 64, False), ("big", 32, False), ("small", 64, True)):
        c = S.real_case(gname, d, pair)
        assert -40 <= int(c.dots["sorted"].min()) and int(c.dots["sorted"].max()) <= 40
        assert len(np.unique(c.dots["sorted"])) > 40
        for order in ("sorted", "class"):
            worst = max(worst, S.torch_softmax_worst_error(dtype, c.g, c.dots[order], c.ref[order]))
    print(f"torch.softmax {dtype}: worst element-wise relative error {worst:.2f} eps")
    assert worst <= S.REAL_BOUND_EPS[dtype]
    assert S.REAL_BOUND_EPS[dtype] == 4 * S.TORCH_SOFTMAX_WORST_EPS[dtype]


def test_true_softmax_is_a_softmax():
    c = S.real_case("small", 13)
    g, ref = c.g, c.ref["sorted"]
    x = torch.from_numpy(c.dots["sorted"]).double()
    for r in np.nonzero(g.deg)[0][::7]:
        a, b = g.rowptr[r], g.rowptr[r + 1]
        assert np.allclose(ref[a:b], torch.softmax(x[a:b], 0).numpy(), rtol=1e-14, atol=0)


@pytest.mark.parametrize("case", S.REAL_CASES, ids=ids)
def test_real_valued_rows_and_class_rows_on_the_double(k, case):
    S.check_real_rows(k, DEV, "small", case)
    S.check_real_class(k, DEV, "small", case)


@pytest.mark.parametrize("dtype", [S.F32, S.F64])
def test_real_valued_segment_softmax_and_pair_on_the_double(k, dtype):
    for gname in S.GRAPHS:
        S.check_real_segment_softmax(k, DEV, gname, dtype)
    S.check_real_pair(k, DEV, "small", dtype, 13)
    S.check_real_rows(k, DEV, "big", (dtype, 32, True))
