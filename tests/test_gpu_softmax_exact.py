"""Bit-exact softmax through every K1 / K2 route, the exp included (tests/softmax_cases.py): scores on levels at least 900
apart make exp(score - max) exactly 1 or 0, every partial sum a small integer and every rescale factor 0 or 1, so a row
must leave as 1 / c on the c edges of its top level and 0.0 elsewhere -- whatever the chunking, the wave slices, the slot
order or row_parts.  A maximum that arrives in a later chunk, wave, slot or part, a dropped or double-counted edge, a row
normalised twice or a row the call does not own being written all show as a wrong bit.  No tolerance in the exact tests;
the real-valued ones at the end compare every edge with the true softmax by its own relative error.

tests/test_softmax_exact_host.py proves on the CPU that the fixtures are exact and that the faults above always show."""
import pytest
import torch

from clane_amd import _hip

from . import exact_cases as E
from . import softmax_cases as S

pytestmark = pytest.mark.gpu
ids = E.case_id
ACC = [S.F32, S.F64]


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


# ---- edge_score, fused ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("case", E.LAYOUT_CASES, ids=ids)
def test_fused_rows_exact(dev, k, case, assignment):
    """Whole rows by one (sub-)wave, long rows listed at threshold 48, a row block with row0 > 0 (and its long rows
    listed): one d per lane layout, padded and odd leading dimensions, f32 / bf16 / f64."""
    S.check_fused_rows(k, dev, "small", assignment, case)


@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("case", S.BIG_CASES, ids=ids)
def test_fused_rows_of_the_6000_row_graph_exact(dev, k, case, assignment):
    """Hubs of 1025, 2049 and 5000 edges: a wave of the 16-wave kernel takes a second, third and fifth chunk, a one-wave
    row 79."""
    S.check_fused_rows(k, dev, "big", assignment, case)


# ---- edge_score_class, fused ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("chunk", [64, 256])
@pytest.mark.parametrize("gname", S.GRAPHS)
@pytest.mark.parametrize("case", S.CLASS_CASES, ids=ids)
def test_fused_class_rows_exact(dev, k, case, gname, chunk, assignment):
    """row_parts 1, 2, 7, 64, 255: the scores, the rows that are not listed, and every slot's {max, sum}."""
    S.check_fused_class(k, dev, gname, assignment, case, chunk)


# ---- the pair instances ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("gname", S.GRAPHS)
@pytest.mark.parametrize("dtype,d", S.PAIR_CASES)
def test_fused_pair_exact(dev, k, dtype, d, gname, assignment):
    S.check_fused_pair(k, dev, gname, assignment, dtype, d)


# ---- segment_softmax ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("setting", sorted(S.SEGMENT_SETTINGS))
@pytest.mark.parametrize("gname", S.GRAPHS)
@pytest.mark.parametrize("dtype", ACC)
def test_segment_softmax_settings_exact(dev, k, dtype, gname, setting, assignment):
    """The defaults, min_degree 0 / 1 / 64, max_degree with the long rows listed, with the longest row NOT listed (it
    stays untouched), max_degree <= min_degree, empty rows; rows the call does not own keep their values."""
    S.check_segment_softmax(k, dev, gname, assignment, dtype, setting)


@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("gname", S.GRAPHS)
@pytest.mark.parametrize("case", S.BIG_CASES, ids=ids)
def test_column_split_route_equals_the_fused_one(dev, k, case, gname, assignment):
    S.check_column_split_route(k, dev, gname, assignment, case)


# ---- the engine ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("assignment", S.ASSIGNMENTS)
@pytest.mark.parametrize("route", sorted(S.ENGINE_SETTINGS))
@pytest.mark.parametrize("gname", S.GRAPHS)
@pytest.mark.parametrize("dtype", ACC)
def test_engine_build_P_bilinear_exact(dev, k, dtype, gname, route, assignment):
    S.check_engine_bilinear(k, dev, gname, assignment, dtype, route)


# ---- real values, element-wise ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", S.GRAPHS)
@pytest.mark.parametrize("case", S.REAL_CASES, ids=ids)
def test_real_valued_rows_and_long_rows(dev, k, case, gname):
    """Integer scores in [-40, 40]: every edge within REAL_BOUND_EPS (4 x torch.softmax's own worst error, 16.6 eps in
    fp32 and 110 eps in fp64) of the true softmax, every row sum within deg * eps of 1."""
    S.check_real_rows(k, dev, gname, case)


@pytest.mark.parametrize("gname", S.GRAPHS)
@pytest.mark.parametrize("case", S.REAL_CASES, ids=ids)
def test_real_valued_class_rows(dev, k, case, gname):
    S.check_real_class(k, dev, gname, case)


@pytest.mark.parametrize("gname", S.GRAPHS)
@pytest.mark.parametrize("dtype", ACC)
def test_real_valued_segment_softmax(dev, k, dtype, gname):
    S.check_real_segment_softmax(k, dev, gname, dtype)


@pytest.mark.parametrize("gname", S.GRAPHS)
@pytest.mark.parametrize("dtype,d", S.REAL_PAIR_CASES)
def test_real_valued_pair(dev, k, dtype, d, gname):
    S.check_real_pair(k, dev, gname, dtype, d)
