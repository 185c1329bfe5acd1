"""Exact link, probe and k-means results through the layer that turns vertex numbering into table-row numbering
(tests/consumer_exact_cases.py), on the HIP kernels, under every one-GPU launch plan of tests/engine_exact_cases.py: the
engine builds the permutation, the padding rows, the class rows' edge order, the column tiles and rotates its tables;
``table_and_rows``, ``sorted_adjacency``, ``PairSampler``, ``project_table`` and ``LinkRanker`` (bilinear, cosine per edge,
cosine reference) must give what an int64 / float64 reference in vertex numbering gives -- ids, scores, the -1 / -inf
tails, the four counts of every ranked pair, the metrics -- and, on float data, the dense kernels the same bits under
every plan and the consumers the same bits as on a fresh engine after every step that changes which table is current.
No tolerance anywhere in this file.

The consumers that merged later (tests/consumer_later_cases.py) -- the silhouette, ContentPCA on a table, the k-NN search,
both t-SNE fits, LabelProbe.predict, the Gaussian mixture and the two kept models -- are held to the same relations: A.8,
every output under the plans that change what a consumer sees equals the LAYOUT-FREE result on a plain contiguous [V, d]
tensor no engine made, rows = the vertex list itself (the k-NN and t-SNE have no float64 instance and are left out of
that case); B, after every step the same consumers, through objects and models made before any sweep and through new
ones, equal those of a fresh engine; and one self-check feeds every consumer the list not mapped through ``pos``, the
table before the last sweep and, for ``table="X"``, the Z table, each of which must compare UNEQUAL.

tests/test_consumer_exact_host.py proves on the CPU that the fixtures are exact and that a wrong row map, an unsorted
adjacency, labelled padding rows, a stale norm flag and a projection of the wrong table show; for the later consumers,
that the plans permute the listed rows, pad the table and (PADDED_CASES) widen the leading dimension."""
import pytest

from clane_amd import _hip

from . import consumer_exact_cases as CX
from . import consumer_later_cases as CL
from . import engine_exact_cases as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


@pytest.mark.parametrize("run", X.PLAN_RUNS, ids=X.plan_id)
def test_consumers_exact_under_plan(dev, k, run):
    """A.1 - A.6 on the 700-vertex graph under one plan, and the route the plan is there for."""
    CX.check_plan(k, dev, *run)


@pytest.mark.parametrize("run", CX.SPLIT_RUNS, ids=X.plan_id)
def test_consumers_exact_on_the_split_graph(dev, k, run):
    """A.1 - A.6 on 4300 vertices: 34 candidate tiles, two rows that point at every vertex."""
    CX.check_split(k, dev, *run)


@pytest.mark.parametrize("plan", list(X.PLANS))
@pytest.mark.parametrize("case", X.ONE_PER_DTYPE, ids=X.case_id)
def test_fits_do_not_depend_on_the_plan(dev, k, case, plan):
    """A.7: k-means, the label probe and the one-vs-rest probe on random normal data give the defaults plan's bits."""
    CX.check_plan_independence(k, dev, case, plan)


@pytest.mark.parametrize("run", CX.CURRENT_RUNS, ids=CX.current_id)
def test_consumers_read_the_current_table(dev, k, run):
    """B: after every step of sweep / snapshot / a launch taken back / the snapshot distance / set_Z, rankers old and new,
    project_table, table_and_rows and a k-means fit equal those of a fresh engine holding the same table; so do the k-NN
    (float32 / bfloat16), the silhouette, fit_table + transform_table, LabelProbe.predict, a three-iteration mixture fit
    and the kept models' predictions, through objects made before any sweep and through new ones."""
    CX.check_current_table(k, dev, run)


@pytest.mark.parametrize("run", CL.LATER_RUNS, ids=X.plan_id)
def test_later_consumers_do_not_depend_on_the_layout(dev, k, run):
    """A.8: k-NN (k = 7; k = 192 in three slabs), silhouette (euclidean, cosine), fit_table + transform_table, both t-SNE
    fits, LabelProbe.predict (soft-max, sigmoid), the mixture fit and the kept label and mixture models give the bits of a
    plain [V, d] table read with the vertex list itself; under chunks3_overlap the silhouette, k-NN, PCA and mixture also
    on table="X".  float64: no k-NN and no t-SNE (the distance kernels have float32 and bfloat16 instances only)."""
    CL.check_layout_independence(k, dev, *run)


def test_wrong_inputs_fail_the_layout_comparison(dev, k):
    """Under chunks3_overlap: the list not mapped through pos (Z and X), the Z table where X was asked for and the table
    before the last sweep make every data output of every consumer differ from the layout-free result; pos-mapped rows
    into X_loc are the RIGHT rows on one GPU (X_loc is in table-row order) and compare equal."""
    CL.check_wrong_inputs(k, dev)
