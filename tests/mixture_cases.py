"""Shared cases of the Gaussian-mixture tests: the two kernels of csrc/mixture.h restated in torch as a KernelBackend
subclass (the CPU double), a float64 reference EM in numpy, and the planted data."""
import math

import numpy as np
import torch

from clane_amd import _hip
from clane_amd.engine import SweepEngine
from clane_amd.partition import HostCSR

from .test_cluster_host import KMeansOracleKernels

# (n, d, K, sep, seed)
SHAPES = ((600, 5, 4, 3.0, 0), (1000, 16, 7, 3.0, 1), (300, 3, 2, 4.0, 2))
EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.bfloat16: 2.0 ** -24}    # unit round-off of the accumulate type


def planted(n, d, K, sep, seed):
    """(X float64 [n, d], y int64 [n], means, sigma): draws in this order -- y uniform in K with the first K rows one per
    class, the component means standard_normal((K, d)) * sep, per-component per-dimension sigma uniform in [0.5, 1.5], the
    noise."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, K, n)
    y[:K] = np.arange(K)
    means = rng.standard_normal((K, d)) * sep
    sigma = rng.uniform(0.5, 1.5, (K, d))
    X = means[y] + sigma[y] * rng.standard_normal((n, d))
    return X, y, means, sigma


def padded(K):
    return 1 << (int(K) - 1).bit_length()


class MixtureOracleKernels(KMeansOracleKernels):
    """mixture_estep / mixture_mstep of csrc/mixture.h in torch (the same formulas, no attempt at the same rounding), and
    the column sums the centring needs.  A restart's bits do not depend on the other restarts of a call."""

    def __init__(self):
        super().__init__()
        self.estep_calls = []                       # (R, resp written, assign written)

    def column_sums_ws_len(self, n, d):
        return 1

    def column_sums(self, Z, d, rows, ws, sums, accumulate=False):
        s = self._gathered(Z, d, rows, torch.float64).sum(0)
        sums.copy_(sums + s if accumulate else s)

    def _phi(self, Z, d, rows, mean, dtype):
        xc = self._gathered(Z, d, rows, dtype) - mean
        return torch.cat([xc * xc, xc], 1)

    def mixture_ll_ws_len(self, n, R):
        return 1

    def mixture_estep(self, Z, d, rows, mean, Wm, cst, R, K, ll_ws, ll, resp=None, assign=None):
        self.estep_calls.append((R, resp is not None, assign is not None))
        Kp, n = padded(K), rows.numel()
        assert tuple(Wm.shape) == (R * Kp, 2 * d) and cst.numel() == R * Kp and mean.numel() == d
        phi = self._phi(Z, d, rows, mean, Wm.dtype)
        out = None if resp is None else resp.view(-1)[:n * R * Kp].view(n, R * Kp)
        for r in range(R):                                  # restart by restart
            l = phi @ Wm[r * Kp:r * Kp + K].T + cst[r * Kp:r * Kp + K]
            mx = l.amax(1)
            e = torch.exp(l - mx[:, None])
            se = e.sum(1)
            ll[r] = (mx + torch.log(se)).double().clone().sum()
            if out is not None:
                out[:, r * Kp:(r + 1) * Kp] = 0
                out[:, r * Kp:r * Kp + K] = e / se[:, None]
            if assign is not None:
                assign[:, r] = (l == mx[:, None]).int().argmax(1).to(torch.int32)      # the first of the maxima

    def mixture_mstep_ws_len(self, n, K, d):
        return 1

    def mixture_mstep(self, Z, d, rows, mean, resp, ws, S, nk):
        n, K = rows.numel(), nk.numel()
        phi = self._phi(Z, d, rows, mean, S.dtype)
        r = resp.view(-1)[:n * K].view(n, K)
        for c in range(K):                                  # column by column: a column's sums do not depend on the others
            S.view(K, 2 * d)[c] = r[:, c] @ phi
            nk[c] = r[:, c].clone().sum()


def cpu_engine(X, kernels=None):
    V = X.shape[0]
    csr = HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + 1) % V).astype(np.int32))
    return SweepEngine(csr, X, "cpu", kernels if kernels is not None else MixtureOracleKernels())


# ---- the float64 reference ------------------------------------------------------------------------------------------
def log_prob(X, weights, means, variances):
    """[n, K] float64: log pi_k + log N(x_i | mu_k, diag var_k), by scikit-learn's expansion."""
    d = X.shape[1]
    a = 1.0 / variances
    quad = (means * means * a).sum(1) - 2.0 * X @ (means * a).T + (X * X) @ a.T
    return -0.5 * (d * math.log(2.0 * math.pi) + quad) - 0.5 * np.log(variances).sum(1) + np.log(weights)


def e_step(X, weights, means, variances):
    """(lse [n], resp [n, K]) in float64."""
    l = log_prob(X, weights, means, variances)
    mx = l.max(1)
    lse = mx + np.log(np.exp(l - mx[:, None]).sum(1))
    return lse, np.exp(l - lse[:, None])


def m_step(X, resp, reg_covar):
    nk = resp.sum(0) + 10.0 * np.finfo(np.float64).eps
    means = resp.T @ X / nk[:, None]
    variances = np.maximum(resp.T @ (X * X) / nk[:, None] - means * means, 0.0) + reg_covar
    return nk / nk.sum(), means, variances


def reference_em(X, resp0=None, params0=None, reg_covar=1e-6, tol=1e-3, max_iter=100, reverse=False):
    """EM in float64 numpy on rows centred by their mean, from initial responsibilities (through the M-step) or initial
    parameters (means in X's coordinates), in scikit-learn's order; ``reverse`` sums the rows backwards.  Returns a dict:
    weights, means (X's coordinates), centred_means, variances, lower_bounds (one per iteration), n_iter, converged,
    log_likelihood (mean per row under the final parameters), resp, assign, bic, aic, mean."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    if reverse:
        X = X[::-1].copy()
        resp0 = None if resp0 is None else np.asarray(resp0)[::-1].copy()
    m = X.mean(0)
    Xc = X - m
    if params0 is not None:
        w, mu, var = (np.asarray(p, dtype=np.float64) for p in params0)
        mu = mu - m
    else:
        w, mu, var = m_step(Xc, np.asarray(resp0, dtype=np.float64), reg_covar)
    K = w.shape[0]
    lbs, lb, converged = [], -np.inf, False
    for _ in range(max_iter):
        prev = lb
        lse, resp = e_step(Xc, w, mu, var)
        w, mu, var = m_step(Xc, resp, reg_covar)
        lb = lse.sum() / n
        lbs.append(lb)
        if abs(lb - prev) < tol:
            converged = True
            break
    lse, resp = e_step(Xc, w, mu, var)
    if reverse:
        resp = resp[::-1].copy()
    ll = lse.sum() / n
    p = 2 * K * d + K - 1
    return {"weights": w, "means": mu + m, "centred_means": mu, "variances": var, "lower_bounds": lbs, "n_iter": len(lbs),
            "converged": converged, "log_likelihood": ll, "resp": resp, "assign": resp.argmax(1),
            "bic": -2.0 * ll * n + p * math.log(n), "aic": -2.0 * ll * n + 2.0 * p, "mean": m}


def score(X, weights, means, variances):
    """The mean log-likelihood per row of X under the parameters (means in X's coordinates), float64."""
    return e_step(np.asarray(X, dtype=np.float64), weights, means, variances)[0].mean()


def one_hot(y, K):
    r = np.zeros((len(y), K))
    r[np.arange(len(y)), y] = 1.0
    return r


def noisy_start(y, K, seed):
    """Initial responsibilities: the planted partition with a fifth of the rows moved to a random component -- a start EM
    has work to do from."""
    rng = np.random.default_rng(1000 + seed)
    y0 = y.copy()
    move = rng.random(len(y)) < 0.2
    y0[move] = rng.integers(0, K, int(move.sum()))
    y0[:K] = np.arange(K)
    return one_hot(y0, K)


def acc_of(dtype):
    return _hip.acc_dtype(dtype)
