"""The exact integer-data cases of tests/exact_cases.py, without a GPU: every case builder's exactness-range assertion,
the mutation self-check (a single dropped edge of the longest row must change the expected tensor in the storage dtype),
and every check of tests/test_gpu_exact.py run through the CPU test double with the same torch.equal assertions --
which proves the fixtures exact and the expectations right before a kernel is ever compared with them."""
import numpy as np
import pytest
import torch

from . import exact_cases as E
from .test_train_host import TrainOracleKernels


class ExactOracleKernels(TrainOracleKernels):
    """The double's pair_project / pair_grad index the table directly; the ABI reads a row outside [0, table_rows) as a
    zero row (include/clane_hip.h).  Restated here so that the out-of-range case has a host run as well."""

    @staticmethod
    def _rows(Z, d, idx, dtype):
        ok = (idx >= 0) & (idx < Z.shape[0])
        return Z[idx.long().clamp(0, Z.shape[0] - 1), :d].to(dtype) * ok.unsqueeze(1)

    def pair_project(self, Z, d, src, dst, W, A, Bm):
        A[:src.numel()] = self._rows(Z, d, src, W.dtype) @ W[:d].T
        Bm[:src.numel()] = self._rows(Z, d, dst, W.dtype) @ W[d:].T

    def pair_grad(self, Z, d, src, dst, A, Bm, g, stats, ws, dW):
        M = float(stats[1])
        if M == 0:
            dW.zero_()
            return
        dW[:d] = (g[:, None] * Bm).T @ self._rows(Z, d, src, A.dtype) / M
        dW[d:] = (g[:, None] * A).T @ self._rows(Z, d, dst, A.dtype) / M


@pytest.fixture(scope="module")
def k():
    return ExactOracleKernels()


DEV = "cpu"
ids = E.case_id


def test_graph_has_the_rows_the_routes_need():
    g = E.graph()
    assert set(E.HUBS) <= set(g.deg.tolist()) and (g.deg == 0).sum() > 50
    for seg in (64, 128):
        rows, seg_ptr, seg_row = g.segments(seg)
        assert rows.size >= 4 and int(seg_ptr[-1]) == seg_row.size > rows.size
    assert (g.deg > 48).sum() > (g.deg > E.CLASS_DEGREE).sum() >= 6
    for r in range(E.V):                                      # sorted, unique rows: what pair_labels searches
        assert (np.diff(g.sorted_colidx[g.rowptr[r]:g.rowptr[r + 1]]) > 0).all()


@pytest.mark.parametrize("case", E.LAYOUT_CASES, ids=ids)
def test_k3_case_is_exact_and_notices_every_dropped_edge(case):
    """Building the case asserts the range condition (bound * 8 < 2^24, row delta as well).  For d >= 16 no single edge
    of the longest row (700 edges, the first 600 tried) may vanish without changing the expected storage-dtype row; at
    d < 16 a bf16 rounding can hide one, so the self-check is not required there."""
    c = E.k3_case(*case)
    assert c.bound * 8 < E.EXACT_LIMIT
    tried, undetected = c.undetected_single_edge_drops()
    assert tried == 600
    if c.d >= 16:
        assert undetected == 0, (ids(case), undetected)


@pytest.mark.parametrize("degree", [65, 600, 5000])
@pytest.mark.parametrize("dtype,d", [(E.BF16, 16), (E.BF16, 128), (E.F32, 128)])
def test_recipe_stays_exact_and_sensitive_up_to_degree_5000(dtype, d, degree):
    """The recipe beyond this graph: one row of `degree` edges -- the range condition holds and no single dropped edge
    (of up to 600) hides under the storage rounding."""
    rng = np.random.default_rng(degree + d)
    Z = E.nonzero_ints(rng, (degree, d), 4)
    x = E.ints(rng, (d,), 8)
    P = torch.from_numpy(rng.integers(1, 9, size=degree)).double() / 4
    assert float((E.GAMMA * (P.unsqueeze(1) * Z.abs()).sum(0) + 8).max()) * 8 < E.EXACT_LIMIT
    full = x + E.GAMMA * (P.unsqueeze(1) * Z).sum(0)
    n = min(degree, 600)
    without = full.unsqueeze(0) - E.GAMMA * P[:n].unsqueeze(1) * Z[:n]
    assert bool((without.to(dtype) != full.to(dtype).unsqueeze(0)).any(1).all())


@pytest.mark.parametrize("case", E.LAYOUT_CASES, ids=ids)
def test_k3_routes_on_the_double(k, case):
    """Every case through one route of each kind of descriptor (the double walks rows in Python and has one code path
    for all flags); three cases, one per dtype, through every route."""
    every = case in [(E.F32, 128, True), (E.BF16, 128, True), (E.F64, 13, False)]
    for route in E.routes_of(case) if every else ("row_t0", "row_t48_sinks_long16", "split128", "class64_beyond"):
        E.check_k3_route(k, DEV, case, route)


@pytest.mark.parametrize("case", [(E.F32, 64, True), (E.BF16, 64, True), (E.F64, 64, True), (E.BF16, 13, False)], ids=ids)
def test_k3_row_block_on_the_double(k, case):
    E.check_k3_row_block(k, DEV, case)


@pytest.mark.parametrize("case", E.K1_CASES, ids=ids)
def test_k1_on_the_double(k, case):
    E.check_k1(k, DEV, case)
    if case[0] != E.BF16:
        E.check_k1_pair(k, DEV, case)


@pytest.mark.parametrize("case", E.LAYOUT_CASES, ids=ids)
def test_stage_kernels_and_gather_on_the_double(k, case):
    E.check_stage_kernels(k, DEV, case)
    E.check_gather_rows(k, DEV, case)


@pytest.mark.parametrize("dtype", [E.F32, E.BF16, E.F64])
@pytest.mark.parametrize("d", E.PROJECT_D)
def test_projections_on_the_double(k, dtype, d):
    E.check_projections(k, DEV, dtype, d)


@pytest.mark.parametrize("dtype", [E.F32, E.BF16, E.F64])
@pytest.mark.parametrize("d", E.GRAD_D)
def test_pair_grad_and_out_of_range_rows_on_the_double(k, dtype, d):
    E.check_pair_grad(k, DEV, dtype, d)
    E.check_out_of_range_pairs(k, DEV, dtype, d)


def test_pair_labels_on_the_double(k):
    """The structured pairs of every row (the random fill is the card's: the double searches in Python)."""
    E.check_pair_labels(k, DEV, 8000)
    E.check_pair_labels_small(k, DEV)
    src, dst, want = E.label_pairs(600_000)
    assert src.size == 600_000 and 5000 < int(want.sum()) < 100_000
    s8, d8, w8 = E.label_pairs(8000)
    assert np.array_equal(src[:6000], s8[:6000]) and np.array_equal(want[:6000], w8[:6000])


def test_row_parts_on_the_double(k):
    E.check_row_parts(k, DEV, E.F32, 100, compare_stats=False)      # the double keeps no per-slot stats
