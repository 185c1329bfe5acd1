"""Bit-exact parity of every kernel instance on integer data (tests/exact_cases.py): all intermediates are exactly
representable, so summation order, FMA contraction, tiling and the bf16 store cannot move a bit and a kernel must be
torch.equal to the fp64 / int64 result rounded once to the storage dtype.  A dropped edge, a lost segment lane, a read
one element past a row show as a wrong bit -- in bf16 as in fp32 and fp64.  No tolerance anywhere in this file.

tests/test_exact_host.py proves on the CPU that the fixtures are exact and that one dropped edge always shows."""
import pytest
import torch

from clane_amd import _hip

from . import exact_cases as E

pytestmark = pytest.mark.gpu
ids = E.case_id
DTYPES = [E.F32, E.BF16, E.F64]


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


# ---- K3: every route, every lane layout ----------------------------------------------------------------------------------
@pytest.mark.parametrize("route", E.ROUTES)
@pytest.mark.parametrize("case", E.LAYOUT_CASES, ids=ids)
def test_spmm_routes_exact(dev, k, case, route):
    """spmm_update (long_threshold 0 / 48, sinks untouched or copied), spmm_update_long (4 / 16 waves),
    spmm_update_split (64 / 128 edges per segment), spmm_update_class (chunk 64 / 256, with and without
    CLANE_SPMM_TABLE_BEYOND_CACHE), each finishing its rows into one Z_new with the mirror on: the table, the pad
    columns, the sinks, both mirror buffers and the reduced delta."""
    E.check_k3_route(k, dev, case, route)


@pytest.mark.parametrize("case", E.BEYOND_ROW_CASES, ids=ids)
def test_spmm_row_pass_beyond_cache_instance_exact(dev, k, case):
    """CLANE_SPMM_TABLE_BEYOND_CACHE on the row pass, where it selects another instance (fp32, d = 128)."""
    E.check_k3_route(k, dev, case, "row_t0_beyond")


@pytest.mark.parametrize("case", [(E.F32, 64, True), (E.BF16, 64, True), (E.F64, 64, True), (E.BF16, 13, False)], ids=ids)
def test_spmm_row_block_with_row0_exact(dev, k, case):
    E.check_k3_row_block(k, dev, case)


# ---- K1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.K1_CASES, ids=ids)
def test_edge_score_raw_dot_exact(dev, k, case):
    """edge_score (whole-wave and sub-row rows, listed long rows, a row block) and edge_score_class: every score is the
    int64 dot, every edge the call does not own keeps the sentinel."""
    E.check_k1(k, dev, case)


@pytest.mark.parametrize("case", [c for c in E.K1_CASES if c[0] != E.BF16], ids=ids)
def test_edge_score_pair_exact(dev, k, case):
    E.check_k1_pair(k, dev, case)


@pytest.mark.parametrize("dtype,d", [(E.F32, 256), (E.F32, 100), (E.F64, 64), (E.BF16, 128)])
def test_score_row_parts_change_no_bit(dev, k, dtype, d):
    E.check_row_parts(k, dev, dtype, d)


# ---- the other stage kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.K1_CASES, ids=ids)
def test_sqnorm_degree_sums_l1_exact(dev, k, case):
    E.check_stage_kernels(k, dev, case)


@pytest.mark.parametrize("case", E.LAYOUT_CASES, ids=ids)
def test_gather_rows_exact(dev, k, case):
    E.check_gather_rows(k, dev, case)


# ---- projections, gradient, labels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", E.PROJECT_D)
def test_projections_exact(dev, k, dtype, d):
    E.check_projections(k, dev, dtype, d)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", E.GRAD_D)
def test_pair_grad_exact(dev, k, dtype, d):
    E.check_pair_grad(k, dev, dtype, d)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", E.GRAD_D)
def test_pair_rows_outside_the_table_read_as_zero(dev, k, dtype, d):
    E.check_out_of_range_pairs(k, dev, dtype, d)


def test_pair_labels_against_a_set_lookup(dev, k):
    """600 000 pairs: more than the 2048 workgroups of 256 the launch is capped at, so the grid-stride loop takes a
    second trip."""
    E.check_pair_labels(k, dev, 600_000)


def test_pair_labels_empty_batches_and_tables(dev, k):
    E.check_pair_labels_small(k, dev)
