"""Cases and float64 restatements shared by the silhouette tests (test_silhouette_host.py, test_gpu_silhouette.py):
what csrc/silhouette.h is asked to compute, written down once more in numpy, independently of clane_amd.cluster."""
import numpy as np
import torch

# (n, d, K).  The last shape is this file's own: the one in which the sizes 257, 128 and 129 meet in one partition.
SHAPES = [(5, 1, 2), (127, 5, 3), (129, 16, 7), (300, 130, 17), (600, 17, 6)]

# cluster sizes around the 128-position tile: 0 (an empty id), 1 (a singleton), 127, 128, 129, 257
SIZES = {
    (5, 1, 2): [4, 1],
    (127, 5, 3): [126, 0, 1],
    (129, 16, 7): [127, 0, 1, 1, 0, 0, 0],
    (300, 130, 17): [257, 0, 1] + [3] * 14,
    (600, 17, 6): [257, 128, 129, 0, 1, 85],
}
assert all(sum(SIZES[s]) == s[0] and len(SIZES[s]) == s[2] for s in SHAPES)


def partition(shape, seed=0):
    """int64 [n]: a partition with SIZES[shape], the clusters scattered over the rows."""
    n = shape[0]
    part = np.repeat(np.arange(shape[2]), SIZES[shape])
    return torch.from_numpy(part[np.random.default_rng(1000 + seed + n).permutation(n)].astype(np.int64))


def table_case(shape, integers, seed=0):
    """(values [table_rows, d] float64, rows int32 [n], mu float64 [d]): a table of n // 2 rows, so ``rows`` repeat, and
    one index past the table (a zero row).  ``integers``: entries in -2..2 and an integer mu."""
    n, d, _ = shape
    gen = torch.Generator().manual_seed(77 * n + d + seed)
    table_rows = max(3, n // 2)
    if integers:
        Zv = torch.randint(-2, 3, (table_rows, d), generator=gen).double()
        mu = torch.randint(-1, 2, (d,), generator=gen).double()
    else:
        Zv = torch.randn(table_rows, d, generator=gen, dtype=torch.float64) + 0.5
        mu = torch.full((d,), 0.5, dtype=torch.float64)
    rows = torch.randint(0, table_rows, (n,), generator=gen).to(torch.int32)
    rows[n // 2] = table_rows
    return Zv, rows, mu


def gathered(values, rows):
    """float64 [n, d]: values[rows], a zero row for an index outside the table."""
    r = rows.long()
    inside = (r >= 0) & (r < values.shape[0])
    return values.double()[r.clamp(0, values.shape[0] - 1)] * inside[:, None]


def sums_of(D, part, K):
    """S [n, K] float64 from distances D [n, n] (numpy): S[i, c] = sum of D[i, j] over the rows j of cluster c, j != i."""
    D = np.array(D, dtype=np.float64)
    np.fill_diagonal(D, 0.0)
    member = np.zeros((D.shape[0], K))
    member[np.arange(D.shape[0]), np.asarray(part)] = 1.0
    return D @ member


def finish(S, part):
    """The per-row silhouette from the sums, in numpy float64 -- the definition: a = S[i, own] / (n_own - 1), b = min over
    the other non-empty clusters of S[i, c] / n_c, s = (b - a) / max(a, b); 0 for a singleton and where max(a, b) = 0."""
    S, part = np.asarray(S, dtype=np.float64), np.asarray(part)
    n, K = S.shape
    cnt = np.bincount(part, minlength=K).astype(np.float64)
    s = np.zeros(n)
    for i in range(n):
        own = part[i]
        if cnt[own] <= 1:
            continue
        a = S[i, own] / (cnt[own] - 1.0)
        b = min(S[i, c] / cnt[c] for c in range(K) if c != own and cnt[c] > 0)
        if max(a, b) > 0:
            s[i] = (b - a) / max(a, b)
    return s


def euclidean64(A):
    """All pairwise distances of the rows of A (numpy float64) by differences."""
    A = np.asarray(A, dtype=np.float64)
    return np.sqrt(((A[:, None, :] - A[None, :, :]) ** 2).sum(-1))


def cosine64(A):
    A = np.asarray(A, dtype=np.float64)
    nr = np.sqrt((A * A).sum(1))
    r = np.where(nr > 0, 1.0 / np.where(nr > 0, nr, 1.0), 0.0)
    return np.maximum(0.0, 1.0 - (A @ A.T) * r[:, None] * r[None, :])
