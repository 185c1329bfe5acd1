"""Bit-exact sweeps through SweepEngine's own launch plan on integer data (tests/engine_exact_cases.py): the engine
builds the vertex permutation, the row bins, the partial offsets, the column tiles, the class items, the halo send lists
and mirrors, and drives the HIP kernels with them; get_Z() must be torch.equal to the fp64 oracle's sweep rounded once
to the storage dtype, the returned delta and the snapshot distance == the sum over the stored values -- on one GPU under
every plan, through the split route, under every division (ranks as threads on this card) and over three consecutive
sweeps with a launch taken back in between.  A row's partial dropped or counted twice, a tile's partials at the wrong
offset, a counted pad row, a bf16 row rounded twice on its way through a send buffer, a row delivered a sweep late show
as a wrong bit.  No tolerance anywhere in this file.

tests/test_engine_exact_host.py proves on the CPU that the fixtures are exact and that such mistakes show."""
import pytest

from clane_amd import _hip

from . import engine_exact_cases as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


@pytest.mark.parametrize("run", X.PLAN_RUNS, ids=X.plan_id)
def test_one_gpu_plan_exact(dev, k, run):
    """One sweep under one plan: the table, the sinks, the pad columns, the returned delta, the snapshot distance, and
    the route the plan is there for."""
    X.check_plan(k, dev, *run)


@pytest.mark.parametrize("run", X.OWNED_RUNS, ids=X.plan_id)
def test_owned_plan_exact(dev, k, run):
    """The same five comparisons with the class rows summed by spmm_owned_kernel: under the engine's own vertex order,
    class rows from 33 edges, pieces of 256, whole and virtual rows, rows beside it on chunk + combine, three launch
    blocks (row0 > 0) on side streams or in order, contiguous tables, column tiles of 152 / 148 and of 100 elements,
    and the configuration the engine chooses by itself for a table beyond the Infinity Cache."""
    X.check_owned_plan(k, dev, *run)


@pytest.mark.parametrize("plan", list(X.SPLIT_PLANS))
@pytest.mark.parametrize("case", X.SPLIT_CASES, ids=X.case_id)
def test_split_route_exact(dev, k, case, plan):
    """Two rows of 4300 edges: the segmented route with the class pass off, the class pass with the defaults."""
    X.check_split(k, dev, case, plan)


@pytest.mark.parametrize("run", X.DIVISION_RUNS, ids=X.division_id)
def test_division_exact(dev, k, run):
    """Every rank's get_Z() is the expectation and every rank's delta the global one."""
    X.check_division(k, dev, run)


@pytest.mark.parametrize("plan", list(X.SEQUENCE_PLANS))
def test_consecutive_sweeps_exact(dev, k, plan):
    """snapshot, two sweeps, the distance, a launch taken back, a third sweep: fp64, d = 32, everything exact."""
    X.check_sequence(k, dev, plan)


@pytest.mark.parametrize("exchange,world,fused", X.SEQUENCE_DIVISIONS)
def test_consecutive_sweeps_under_a_division_exact(dev, k, exchange, world, fused):
    X.check_sequence_division(k, dev, exchange, world, fused)
