"""The checker of the 2-D layout (clane_amd/layout.py, csrc/tsne.h): a float64 restatement of exact t-SNE in plain numpy
-- squared distances, the perplexity search, the joint probabilities, the force sums, KL and gradient, scikit-learn's
update -- with the error bounds the GPU tests hold the kernels to, and a float32 emulation of the search and of a short
trajectory from which the two tolerances that cannot be derived are measured.  tests/test_layout_host.py pins this file
to scikit-learn; tests/test_gpu_layout.py holds the kernels to it."""
import numpy as np

U = 2.0 ** -24                      # unit round-off of float32
EPS = 2.220446e-16                  # scikit-learn's MACHINE_EPSILON, as the kernels spell it
EPS32 = float(np.float32(EPS))
SEARCH_STEPS, SEARCH_TOL = 100, 1e-5


# ---- data --------------------------------------------------------------------------------------------------------------
def gaussian(n, d, seed=0, scale=1.0, offset=0.0):
    return (np.random.default_rng(seed).standard_normal((n, d)) * scale + offset).astype(np.float32)


def blobs(n=300, d=16, classes=3, seed=0, spread=10.0):
    """``classes`` Gaussian blobs, centres ``spread * N(0, I)``, unit noise; (X float32, labels int64), classes in turn."""
    rng = np.random.default_rng(seed)
    centres = spread * rng.standard_normal((classes, d))
    y = np.arange(n) % classes
    return (centres[y] + rng.standard_normal((n, d))).astype(np.float32), y.astype(np.int64)


def layout_at(n, scale, seed=0):
    return (np.random.default_rng(100 + seed).standard_normal((n, 2)) * scale).astype(np.float32)


# ---- squared distances -------------------------------------------------------------------------------------------------
def centred(values, mu):
    """a = z - mu as the kernel forms it: ONE float32 subtraction of float32 values; returned as float64."""
    return (np.asarray(values, np.float32) - np.asarray(mu, np.float32)[None, :]).astype(np.float64)


def sqdist(a):
    """(D, bound): float64 squared distances of the rows of ``a`` (0 on the diagonal) and the float32 kernel's bound
    (d + 4) u (|a_i|^2 + |a_j|^2 + 2 sum_k |a_ik a_jk|): d roundings in each norm and in the dot, 4 for forming D."""
    a = np.asarray(a, np.float64)
    sq = (a * a).sum(1)
    D = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (a @ a.T), 0.0)
    np.fill_diagonal(D, 0.0)
    bound = (a.shape[1] + 4) * U * (sq[:, None] + sq[None, :] + 2.0 * (np.abs(a) @ np.abs(a).T))
    return D, bound


# ---- the perplexity search ---------------------------------------------------------------------------------------------
def perplexity_search(D, perplexity, dtype=np.float64):
    """scikit-learn's _binary_search_perplexity on the rows of D shifted by their minimum: (conditional P, beta).  With
    ``dtype=np.float32`` every element-wise operation and both sums run in float32 -- the emulation of the kernel, whose
    entropy is formed in double from the two sums, as here."""
    D = np.asarray(D, dtype)
    n = D.shape[0]
    off = ~np.eye(n, dtype=bool)
    dd = np.where(off, D - np.where(off, D, np.inf).min(1)[:, None], dtype(0)).astype(dtype)
    beta = np.ones(n, dtype)
    lo, hi = np.full(n, -np.inf, dtype), np.full(n, np.inf, dtype)
    target = np.log(float(perplexity))
    active = np.ones(n, bool)
    half, two = dtype(0.5), dtype(2.0)
    for step in range(SEARCH_STEPS):
        rows = np.flatnonzero(active)
        if rows.size == 0:
            break
        e = np.where(off[rows], np.exp(-beta[rows, None] * dd[rows]), dtype(0)).astype(dtype)
        sp = e.sum(1, dtype=dtype).astype(np.float64)
        sdp = (dd[rows] * e).sum(1, dtype=dtype).astype(np.float64)
        diff = np.log(sp) + beta[rows].astype(np.float64) * sdp / sp - target
        found = np.abs(diff) <= SEARCH_TOL
        active[rows[found]] = False
        if step == SEARCH_STEPS - 1:
            break
        up, down = rows[~found & (diff > 0)], rows[~found & ~(diff > 0)]
        lo[up] = beta[up]
        beta[up] = np.where(np.isinf(hi[up]), beta[up] * two, (beta[up] + hi[up]) * half)
        hi[down] = beta[down]
        beta[down] = np.where(np.isinf(lo[down]), beta[down] * half, (beta[down] + lo[down]) * half)
    return conditional_at(D, beta, dtype), beta


def conditional_at(D, beta, dtype=np.float64):
    """p_{j|i} = exp(-beta_i (D_ij - min_j D_ij)) / sum at the GIVEN beta, 0 on the diagonal."""
    D = np.asarray(D, dtype)
    off = ~np.eye(D.shape[0], dtype=bool)
    dd = np.where(off, D - np.where(off, D, np.inf).min(1)[:, None], dtype(0)).astype(dtype)
    e = np.where(off, np.exp(-np.asarray(beta, dtype)[:, None] * dd), dtype(0)).astype(dtype)
    return e / e.sum(1, dtype=dtype)[:, None]


def conditional_bound(D, beta):
    """What a float32 row may differ by from conditional_at(D, beta) in float64, element-wise: the argument beta (D - min)
    carries two roundings (2 |arg| u in the exponential), the exponential and the division three more, the row's sum at
    most n + 2 (as the row-sum check); 1e-37 covers results flushed below the normal range."""
    D = np.asarray(D, np.float64)
    n = D.shape[0]
    off = ~np.eye(n, dtype=bool)
    arg = np.asarray(beta, np.float64)[:, None] * (D - np.where(off, D, np.inf).min(1)[:, None])
    return conditional_at(D, beta) * U * (2.0 * np.abs(arg) + 3.0 + (n + 2)) + 1e-37


def row_entropy(Pc):
    """H_i = -sum_j p ln p of every row, float64."""
    p = np.asarray(Pc, np.float64)
    return -(p * np.log(np.where(p > 0, p, 1.0))).sum(1)


def joint(Pc):
    """scikit-learn's _joint_probabilities from the conditionals: max((p_{j|i} + p_{i|j}) / 2n, eps), 0 on the diagonal."""
    Pc = np.asarray(Pc, np.float64)
    P = np.maximum((Pc + Pc.T) / (2.0 * Pc.shape[0]), EPS)
    np.fill_diagonal(P, 0.0)
    return P


def joint_probabilities(D, perplexity):
    return joint(perplexity_search(D, perplexity)[0])


def plogp(P):
    p = np.asarray(P, np.float64)
    return float((p * np.log(np.where(p > 0, p, 1.0))).sum())


# ---- one iteration -----------------------------------------------------------------------------------------------------
def forces(P, Y, dtype=np.float64):
    """The four sums of an iteration and, in float64, the sums of their terms' absolute values:
    {"attr" [n, 2], "rep" [n, 2], "s" [n], "l" [n], "abs_attr", "abs_rep", "abs_l"}."""
    P, Y = np.asarray(P, dtype), np.asarray(Y, dtype)
    n = Y.shape[0]
    diff = Y[:, None, :] - Y[None, :, :]                          # [i, j, c] = y_i - y_j
    d2 = (diff * diff).sum(2, dtype=dtype)
    q = (dtype(1) / (dtype(1) + d2)).astype(dtype)
    pq, qq, lt = P * q, q * q, P * np.log1p(d2)
    out = {"attr": (pq[:, :, None] * diff).sum(1, dtype=dtype), "rep": (qq[:, :, None] * diff).sum(1, dtype=dtype),
           "s": np.where(np.eye(n, dtype=bool), dtype(0), q).sum(1, dtype=dtype), "l": lt.sum(1, dtype=dtype)}
    if dtype is np.float64:
        out.update(abs_attr=(pq[:, :, None] * np.abs(diff)).sum(1), abs_rep=(qq[:, :, None] * np.abs(diff)).sum(1),
                   abs_l=np.abs(lt).sum(1))
    return out


def objective(P, Y, alpha=1.0, plogp_value=None, dtype=np.float64):
    """(KL of the un-exaggerated P, gradient [n, 2] at exaggeration alpha, S): KL = sum p ln p + sum l_i + ln S,
    g_i = 4 (alpha attr_i - rep_i / S)."""
    f = forces(P, Y, dtype)
    S = f["s"].sum(dtype=np.float64)
    kl = (plogp(P) if plogp_value is None else plogp_value) + float(f["l"].sum(dtype=np.float64)) + np.log(S)
    g = 4.0 * (alpha * f["attr"].astype(np.float64) - f["rep"].astype(np.float64) / S)
    return kl, g, S


def update(g, Y, V, G, momentum, lr, dtype=np.float64):
    """scikit-learn's _gradient_descent step: (Y_next, V_next, G_next)."""
    g, Y, V, G = (np.asarray(x, dtype) for x in (g, Y, V, G))
    G = np.maximum(np.where(V * g < 0, G + dtype(0.2), G * dtype(0.8)), dtype(0.01)).astype(dtype)
    V = (dtype(momentum) * V - dtype(lr) * G * g).astype(dtype)
    return (Y + V).astype(dtype), V, G


def trajectory(P, Y0, iters, alpha, momentum, lr, dtype=np.float64):
    """Y after ``iters`` iterations from Y0 with zero velocity and unit gains; with ``dtype=np.float32`` the emulation:
    P, Y, the force sums, the gradient and the update all in float32."""
    P = np.asarray(P, dtype)
    Y = np.asarray(Y0, dtype)
    V, G = np.zeros_like(Y), np.ones_like(Y)
    for _ in range(iters):
        _, g, _ = objective(P, Y, alpha, plogp_value=0.0, dtype=dtype)
        Y, V, G = update(g.astype(dtype), Y, V, G, momentum, lr, dtype)
    return Y


def fit(P, Y0, max_iter=500, early_exaggeration=12.0, exaggeration_iters=250, lr=None):
    """The whole descent in float64, without the early stops: Y after max_iter iterations."""
    n = Y0.shape[0]
    lr = max(n / early_exaggeration / 4.0, 50.0) if lr is None else lr
    first = min(exaggeration_iters, max_iter)
    Y = trajectory(P, Y0, first, early_exaggeration, 0.5, lr)
    return trajectory(P, Y, max_iter - first, 1.0, 0.8, lr)


def neighbour_agreement(Y, labels, k=5):
    Y, labels = np.asarray(Y, np.float64), np.asarray(labels)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d, np.inf)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((labels[idx] == labels[:, None]).mean())


def pca_init(X):
    """scikit-learn's init="pca" in float64: two components, the first column's standard deviation 1e-4."""
    Xc = np.asarray(X, np.float64)
    Xc = Xc - Xc.mean(0)
    _, _, Vt = np.linalg.svd(Xc, full_matrices=False)
    Y = Xc @ Vt[:2].T
    return Y / Y[:, 0].std() * 1e-4
