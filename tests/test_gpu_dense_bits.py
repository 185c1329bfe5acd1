"""Every dense (MFMA) kernel against ONE order of the k terms, on random float data (tests/dense_bits_cases.py).

csrc/mfma_tile.h fixes the order in which the k terms of a dot are accumulated -- "identical for every element, every
kernel and every call" -- and the equal-bits promises of link_rank.h, link_eval.h, label_probe.h, multilabel_probe.h and
kmeans.h, "the grouping changes no result" of classify.py and "bit for bit what top_k reports" of links.py all rest on
it.  So project_rows' output (`anchor_dots`) is an EXACT reference for every other dense kernel: its dots, and what it
selects from them, are computed on the CPU from the anchor and compared with torch.equal on every element -- no "clear"
mask, no window.  The integer-data tests cannot see a changed order (integer sums are order-free) and the float64-bound
tests allow one; these see one inside a build, between two kernels, two tiles or two positions of a list.

The anchor is pinned by (A1) a derived float64 bound -- the only tolerance in this file -- and (A2) position invariance.
tests/test_dense_bits_host.py proves on the CPU that the expectations are right and that each relation fails when the
dots come from another order."""
import pytest

from clane_amd import _hip

from . import dense_bits_cases as D

pytestmark = pytest.mark.gpu
ids = D.case_id


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


# ---- the anchor ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=ids)
@pytest.mark.parametrize("d", D.RANK_D)
def test_anchor_against_float64(dev, k, dtype, d):
    """(A1) |Y - Y64| <= 2 d u |Z| |W|^T elementwise."""
    D.check_anchor_fp64(k, dev, dtype, d)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=ids)
@pytest.mark.parametrize("d", D.RANK_D)
def test_anchor_bits_do_not_depend_on_the_position(dev, k, dtype, d):
    """(A2) one source row at 12 places of the row tiles, the 2d columns permuted, B chunked from another offset."""
    D.check_anchor_positions(k, dev, dtype, d)


# ---- the kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=ids)
@pytest.mark.parametrize("d", D.DENSE_D)
def test_pair_project_has_the_anchors_bits(dev, k, dtype, d):
    """(1) A == anchor[src, :d], Bm == anchor[dst, d:] -- Bm's columns at other tile places than in project_rows."""
    D.check_pair_project(k, dev, dtype, d)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=ids)
@pytest.mark.parametrize("d", D.RANK_D)
def test_top_k_lists_follow_from_the_anchor(dev, k, dtype, d):
    """(2) rank_scores + rank_merge, raw dot, k in 1 / 10 / 32, 1 and 3 slabs, and again with the table rolled by 77:
    the whole [Q, k] lists of scores and ids, the equal rows in label order."""
    D.check_rank_scores(k, dev, dtype, d)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=ids)
@pytest.mark.parametrize("d", D.RANK_D)
def test_rank_counts_follow_from_the_anchor(dev, k, dtype, d):
    """(3) rank_count, raw dot, 6 targets per query, 1 and 3 slabs: target_score has the anchor's bits, the four counts
    are the CPU's counts over the anchor's scores."""
    D.check_rank_count(k, dev, dtype, d)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=ids)
@pytest.mark.parametrize("d", D.DENSE_D)
@pytest.mark.parametrize("K", D.KMEANS_K)
def test_kmeans_assign_follows_from_the_anchor(dev, k, dtype, d, K):
    """(4) best == min_j (csq - 2 anchor), assign the lowest index attaining it, for every row; never a copy of centre 3."""
    D.check_kmeans(k, dev, dtype, d, K)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=ids)
@pytest.mark.parametrize("d", D.DENSE_D)
@pytest.mark.parametrize("CF", D.PROBE_SHAPES, ids=str)
def test_probe_forward_follows_from_the_anchor(dev, k, dtype, d, CF):
    """(5) pred is the lowest class attaining max (anchor + bias) on every row; G, loss and pred of a fit do not depend on
    its place in the stack, G and pred of a row not on its place in the list."""
    D.check_probe_forward(k, dev, dtype, d, *CF)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=ids)
@pytest.mark.parametrize("d", D.DENSE_D)
@pytest.mark.parametrize("CF", D.PROBE_SHAPES, ids=str)
def test_probe_forward_ovr_follows_from_the_anchor(dev, k, dtype, d, CF):
    """(6) the label masks of every row, top-k and threshold, from logits = anchor + bias; row position as in (5)."""
    D.check_probe_ovr(k, dev, dtype, d, *CF)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=ids)
@pytest.mark.parametrize("d", D.DENSE_D)
@pytest.mark.parametrize("n", D.LIST_N)
def test_probe_grad_is_the_anchor_per_chunk(dev, k, dtype, d, n):
    """(7) dW == the 2048-row chunks' anchor dots added in chunk order; db == the documented even / odd row sums."""
    D.check_probe_grad(k, dev, dtype, d, n)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=ids)
@pytest.mark.parametrize("d", D.DENSE_D)
@pytest.mark.parametrize("B", D.LIST_N)
def test_pair_grad_is_the_anchor_per_chunk(dev, k, dtype, d, B):
    """(8) dW == (the chunks' anchor dots of (g Bm)^T / (g A)^T with the gathered rows, added in order) / 64, both halves."""
    D.check_pair_grad(k, dev, dtype, d, B)
