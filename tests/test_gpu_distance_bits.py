"""The distance kernels and probe_predict against the anchor, on random float data (tests/distance_bits_cases.py):
relations 9..13 of the dense-bits suite (tests/test_gpu_dense_bits.py holds the anchor itself and relations 1..8).

silhouette_norms and silhouette_sums (silhouette.h), tsne_sqnorm + tsne_sqdist (tsne.h), knn_sqdist + its merge
(tsne_nn.h, the three query tiles) and probe_predict (label_predict.h) all contract through mfma_tile.h, so
project_rows' dots of the same operands -- a = z - mu formed on the CPU, through the accumulate type's instance -- are
an EXACT reference for them too.  What each kernel adds on top of the dots is restated on the CPU and compared with
torch.equal on every element: the mirrored triangle, the clamp at zero after ONE rounding, the correctly rounded square
root and reciprocal, the documented double-precision order of a silhouette sum, the sorted lists with ties by position,
the eight knock-out rounds with ties by class.  The table holds equal rows and rows one unit in the last place apart,
for which the clamp and the ties are decided by single bits.  No tolerance: the anchor's stays the only one.

tests/test_distance_bits_host.py proves on the CPU that the expectations are right and that each relation fails when the
dots come from another order."""
import pytest

from clane_amd import _hip

from . import distance_bits_cases as X

pytestmark = pytest.mark.gpu
ids = X.case_id


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


@pytest.mark.parametrize("dtype", X.DTYPES, ids=ids)
@pytest.mark.parametrize("d", X.DENSE_D)
@pytest.mark.parametrize("metric", X.METRICS)
@pytest.mark.parametrize("mu", X.MU_KINDS)
def test_silhouette_norms_are_the_anchors_diagonal(dev, k, dtype, d, metric, mu):
    """(9) euclidean: nrm == diag(anchor); cosine: 1 / sqrt of it in two correctly rounded steps, 0 for a zero row."""
    X.check_norms(k, dev, dtype, d, metric, mu)


@pytest.mark.parametrize("dtype", X.DTYPES, ids=ids)
@pytest.mark.parametrize("d", X.DENSE_D)
@pytest.mark.parametrize("metric", X.METRICS)
@pytest.mark.parametrize("mu", X.MU_KINDS)
def test_silhouette_sums_follow_from_the_anchor(dev, k, dtype, d, metric, mu):
    """(10) S [300, 5] == the distances from the anchor's dots added in the documented order, for clusters of 1, 0, 63, 65
    and 171 positions; cosine: one of the two roundings of the last step, the same for the whole call (printed); the call
    for [37, 205) gives rows 37..204 of the call for [0, 300)."""
    X.check_sums(k, dev, dtype, d, metric, mu)


@pytest.mark.parametrize("dtype", X.FLOAT_DTYPES, ids=ids)
@pytest.mark.parametrize("d", X.DENSE_D)
@pytest.mark.parametrize("n", X.TSNE_N)
@pytest.mark.parametrize("mu", X.MU_KINDS)
def test_tsne_sqdist_follows_from_the_anchor(dev, k, dtype, d, n, mu):
    """(11) sq == the fmaf chain in ascending k; D == max((sq_i + sq_j) - 2 anchor, 0) with one rounding, 0 on the
    diagonal, bit-equal to its transpose; prints how many off-diagonal pairs the clamp catches."""
    X.check_sqdist(k, dev, dtype, d, n, mu)


@pytest.mark.parametrize("dtype", X.FLOAT_DTYPES, ids=ids)
@pytest.mark.parametrize("d", X.DENSE_D)
@pytest.mark.parametrize("mu", X.MU_KINDS)
def test_knn_lists_follow_from_the_anchor(dev, k, dtype, d, mu):
    """(12) k in 7 / 90 / 192 (the 128-, 64- and 32-query tile), 1 and 3 slabs: ids and sqdist are the k nearest of
    relation 11's D in the order (distance, position), the whole [300, k] lists."""
    X.check_knn(k, dev, dtype, d, mu)


@pytest.mark.parametrize("dtype", X.FLOAT_DTYPES, ids=ids)
def test_knn_lists_of_five_rows_end_in_fills(dev, k, dtype):
    """(12) n = 5, k = 7: four neighbours, then -1 / +inf."""
    X.check_knn(k, dev, dtype, 17, "random", n=5, ks=(7,))


@pytest.mark.parametrize("dtype", X.DTYPES, ids=ids)
@pytest.mark.parametrize("d", X.DENSE_D)
@pytest.mark.parametrize("CF", X.PROBE_SHAPES, ids=str)
@pytest.mark.parametrize("link", ["soft-max", "sigmoid"])
def test_probe_predict_follows_from_the_anchor(dev, k, dtype, d, CF, link):
    """(13) top_m in 1 / 3 / 8: top_class is the classes by (anchor + bias descending, class ascending), a NaN, a -inf and
    a col_state -1 column never, -1 where they run out; top_prob is proba at top_class bit for bit, 0 at a fill."""
    X.check_predict(k, dev, dtype, d, *CF, link == "sigmoid")
