"""The checker of the neighbour-sparse 2-D layout (clane_amd/layout.py NeighbourTSNE, csrc/tsne_nn.h): a float64
restatement in plain numpy of what differs from exact t-SNE -- the brute-force k nearest neighbours under the kernels'
total order, the perplexity search over a row's k distances, the joint probabilities on the union of the neighbour pairs
-- with a ``dtype`` argument for the float32 emulation the measured tolerances come from.  Everything after P is
tests/layout_cases.py's own: a sparse P is held here as a dense [n, n] matrix whose absent entries are exact zeros, which
add nothing to the attraction sums, to KL or to the bounds, while the repulsion runs over all pairs as it does there.
tests/test_neighbour_layout_host.py pins this file to layout_cases.py and to scikit-learn; tests/test_gpu_neighbour_layout.py
holds the kernels to it."""
import numpy as np

from . import layout_cases as LC

U = LC.U
forces, objective, update, trajectory, fit = LC.forces, LC.objective, LC.update, LC.trajectory, LC.fit


# ---- neighbours --------------------------------------------------------------------------------------------------------
def knn(D, k):
    """(ids [n, k] int32, sqdist [n, k]) of a full matrix of squared distances: per row the k nearest OTHER positions,
    distance ascending, ties by position ascending; -1 and inf past the n - 1 others."""
    D = np.asarray(D)
    n = D.shape[0]
    ids = np.full((n, k), -1, np.int32)
    sq = np.full((n, k), np.inf, D.dtype)
    for i in range(n):
        others = np.delete(np.arange(n), i)
        take = others[np.argsort(D[i, others], kind="stable")][:k]      # stable: equal distances stay in position order
        ids[i, :take.size], sq[i, :take.size] = take, D[i, take]
    return ids, sq


# ---- the perplexity search over the neighbours ----------------------------------------------------------------------------
def _shifted(sqd, ok, dtype):
    sqd = np.asarray(sqd, dtype)
    return np.where(ok, sqd - np.where(ok, sqd, np.inf).min(1)[:, None], dtype(0)).astype(dtype)


def conditional_at(sqd, ids, beta, dtype=np.float64):
    """p_{j|i} over the neighbours at the GIVEN beta, 0 where ids < 0."""
    ok = np.asarray(ids) >= 0
    dd = _shifted(sqd, ok, dtype)
    e = np.where(ok, np.exp(-np.asarray(beta, dtype)[:, None] * dd), dtype(0)).astype(dtype)
    return e / e.sum(1, dtype=dtype)[:, None]


def perplexity_search(sqd, ids, perplexity, dtype=np.float64):
    """layout_cases.perplexity_search over each row's k distances: (conditional p [n, k], beta)."""
    ok = np.asarray(ids) >= 0
    dd = _shifted(sqd, ok, dtype)
    n = dd.shape[0]
    beta = np.ones(n, dtype)
    lo, hi = np.full(n, -np.inf, dtype), np.full(n, np.inf, dtype)
    target = np.log(float(perplexity))
    active = np.ones(n, bool)
    half, two = dtype(0.5), dtype(2.0)
    for step in range(LC.SEARCH_STEPS):
        rows = np.flatnonzero(active)
        if rows.size == 0:
            break
        e = np.where(ok[rows], np.exp(-beta[rows, None] * dd[rows]), dtype(0)).astype(dtype)
        sp = e.sum(1, dtype=dtype).astype(np.float64)
        sdp = (dd[rows] * e).sum(1, dtype=dtype).astype(np.float64)
        diff = np.log(sp) + beta[rows].astype(np.float64) * sdp / sp - target
        found = np.abs(diff) <= LC.SEARCH_TOL
        active[rows[found]] = False
        if step == LC.SEARCH_STEPS - 1:
            break
        up, down = rows[~found & (diff > 0)], rows[~found & ~(diff > 0)]
        lo[up] = beta[up]
        beta[up] = np.where(np.isinf(hi[up]), beta[up] * two, (beta[up] + hi[up]) * half)
        hi[down] = beta[down]
        beta[down] = np.where(np.isinf(lo[down]), beta[down] * half, (beta[down] + lo[down]) * half)
    return conditional_at(sqd, ids, beta, dtype), beta


def conditional_bound(sqd, ids, beta):
    """layout_cases.conditional_bound restricted to the neighbours: the row's sum has k terms, not n."""
    ok = np.asarray(ids) >= 0
    arg = np.asarray(beta, np.float64)[:, None] * _shifted(sqd, ok, np.float64)
    k = ok.shape[1]
    return conditional_at(sqd, ids, beta) * U * (2.0 * np.abs(arg) + 3.0 + (k + 2)) + 1e-37


# ---- the joint probabilities on the union of the neighbour pairs ------------------------------------------------------------
def scatter(ids, values, dtype=np.float64):
    """The dense [n, n] matrix with values[i, r] at (i, ids[i, r]); (matrix, the mask of the places that were set)."""
    ids = np.asarray(ids)
    n = ids.shape[0]
    M, mask = np.zeros((n, n), dtype), np.zeros((n, n), bool)
    i, r = np.nonzero(ids >= 0)
    M[i, ids[i, r]] = np.asarray(values, dtype)[i, r]
    mask[i, ids[i, r]] = True
    return M, mask


def joint(ids, p, dtype=np.float64):
    """(P dense [n, n], union mask): p_ij = (c_ij + c_ji) / 2n where either is a neighbour of the other, an absent
    conditional counting as 0; no floor, no diagonal."""
    C, mask = scatter(ids, p, dtype)
    n = C.shape[0]
    return ((C + C.T) / dtype(2 * n)).astype(dtype), mask | mask.T


def csr_dense(rowptr, cols, val, dtype=np.float64):
    """A CSR as the dense matrix and the mask of its stored places."""
    rowptr, cols = np.asarray(rowptr), np.asarray(cols)
    n = rowptr.size - 1
    M, mask = np.zeros((n, n), dtype), np.zeros((n, n), bool)
    r = np.repeat(np.arange(n), np.diff(rowptr))
    M[r, cols] = np.asarray(val, dtype)
    mask[r, cols] = True
    return M, mask
