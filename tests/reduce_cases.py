"""Fixtures, references and checks of the content reduction (clane_amd/reduce.py, csrc/content_pca.h) -- helpers of
tests/test_gpu_reduce.py (the HIP kernels) and tests/test_reduce_host.py (a plain-torch double of the three calls, run
through the same exact checks, and its mutations).

A check takes the kernel object `k` (``column_sums`` / ``gram`` / ``project_affine`` and their ``*_ws_len``) and the
device the operands go to, so one text serves the GPU and the double.

Integer data: entries in {-2 .. 2}, mu in {-1, 0, 1}^d, W in {-1, 0, 1}: every partial sum is an integer below 2^24
(9 * 4300 for the Gram), exact in all three dtypes, so the int64 reference is compared with torch.equal.  The table has a
padded leading dimension with NaN in the pad columns, the row list is shuffled with one repeat and one index past the
table.
"""
import functools

import numpy as np
import torch

from clane_amd import _hip

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DTYPES = [F32, BF16, F64]
UNIT = {F32: 2.0 ** -24, F64: 2.0 ** -53}                  # unit roundoff of the accumulate type
CHUNK = 2048                                               # kGradChunk
TILE = 128
INT_N = (1, 130, 2049, 4300)        # one row; a partial chunk; one row into the second chunk; three chunks
INT_D = (2, 130, 257)               # less than a pack; a partial second tile; three tiles per side
INT_M = (1, 5, 130)
MU_KINDS = ("none", "integer", "true")
PAD = 3
SAME_ROW_AT = (0, 1, 15, 16, 31, 32, 63, 64, 127, 128, 129, 299)


def case_id(v):
    return _hip._SUFFIX[v] if isinstance(v, torch.dtype) else str(v)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randint(seed, lo, hi, shape):
    return torch.randint(lo, hi, shape, generator=gen(seed), dtype=torch.int64)


# ---- integer fixture -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def int_case(n, d, mu_kind):
    """(X int64 [R, d], rows int32 [n], mu int64 [d] or None): R = max(n, 4) + 2 table rows; rows is a shuffle of table
    rows with rows[1] = rows[0] (a repeat) and rows[2] past the table where n >= 3.  mu_kind "true": the listed rows are
    built in pairs (x, 2 m - x) around m in {-1, 0, 1}^d -- their mean IS m, an integer vector."""
    R = max(n, 4) + 2
    rows = torch.randperm(R, generator=gen(100 + n))[:n].clone()
    if n >= 3:
        rows[1] = rows[0]
        rows[2] = R + 7
    X = randint(7 * n + d, -2, 3, (R, d))
    mu = None
    if mu_kind != "none":
        mu = randint(11 * n + d, -1, 2, (d,))
    if mu_kind == "true":
        present = [i for i in range(n) if 0 <= int(rows[i]) < R]
        X[rows[present]] = mu                                   # the repeat, an odd one out: the mean itself
        free = [i for i in present if i > 2] if n >= 3 else []
        off = randint(13 * n + d, -1, 2, (len(free) // 2, d))
        for j in range(len(free) // 2):
            X[rows[free[2 * j]]] = mu + off[j]
            X[rows[free[2 * j + 1]]] = mu - off[j]
    return X, rows.to(torch.int32), mu


def present_mask(rows, R):
    return (rows >= 0) & (rows < R)


def int_reference(X, rows, mu):
    """(sums [d], G [d, d], centred rows [n, d]) in int64: absent rows add nothing."""
    ok = present_mask(rows, X.shape[0])
    Xg = X[rows.long().clamp(0, X.shape[0] - 1)] * ok[:, None]
    Xc = (Xg - (0 if mu is None else mu)) * ok[:, None]
    return Xg.sum(0), Xc.T @ Xc, Xc


def place(X, dtype, dev, pad=None):
    """An exact integer (or any float) matrix as a `dtype` table on `dev` with `pad` (PAD) NaN columns behind the d real
    ones."""
    pad = PAD if pad is None else pad
    buf = torch.full((X.shape[0], X.shape[1] + pad), float("nan"), dtype=dtype, device=dev)
    buf[:, :X.shape[1]] = X.to(dtype).to(dev)
    return buf[:, :X.shape[1]]


def run_sums(k, Z, d, rows, accumulate=False, sums=None):
    n = rows.numel()
    ws = torch.full((k.column_sums_ws_len(n, d),), float("nan"), dtype=F64, device=Z.device)
    if sums is None:
        sums = torch.full((d,), float("nan"), dtype=F64, device=Z.device)
    k.column_sums(Z, d, rows, ws, sums, accumulate=accumulate)
    return sums


def run_gram(k, Z, d, rows, mu, accumulate=False, G=None):
    acc = _hip.acc_dtype(Z.dtype)
    n = rows.numel()
    ws = torch.full((k.gram_ws_len(n, d),), float("nan"), dtype=acc, device=Z.device)
    if G is None:
        G = torch.full((d, d), float("nan"), dtype=acc, device=Z.device)
    k.gram(Z, d, rows, None if mu is None else mu.to(acc).to(Z.device), ws, G, accumulate=accumulate)
    return G


def run_affine(k, Z, d, rows, mu, W, ldy_pad=2):
    acc = _hip.acc_dtype(Z.dtype)
    n, m = rows.numel(), W.shape[0]
    Y = torch.full((n, m + ldy_pad), 77.0, dtype=Z.dtype, device=Z.device)
    k.project_affine(Z, d, rows, None if mu is None else mu.to(acc).to(Z.device), W.to(acc).to(Z.device), Y[:, :m])
    assert bool((Y[:, m:] == 77.0).all()), "project_affine wrote behind its m columns"
    return Y[:, :m]


def check_int_sums(k, dev, dtype, n, d):
    X, rows, _ = int_case(n, d, "none")
    want, _, _ = int_reference(X, rows, None)
    got = run_sums(k, place(X, dtype, dev), d, rows.to(dev)).cpu()
    assert torch.equal(got, want.double()), ("column sums", n, d)
    Xt, rows_t, m = int_case(n, d, "true")
    got = run_sums(k, place(Xt, dtype, dev), d, rows_t.to(dev)).cpu()
    count = int(present_mask(rows_t, Xt.shape[0]).sum())
    assert torch.equal(got, (m * count).double()), ("column sums of the paired rows", n, d)


def check_int_gram(k, dev, dtype, n, d):
    acc = _hip.acc_dtype(dtype)
    for kind in MU_KINDS:
        X, rows, mu = int_case(n, d, kind)
        _, want, _ = int_reference(X, rows, mu)
        G = run_gram(k, place(X, dtype, dev), d, rows.to(dev), mu).cpu()
        assert torch.equal(G, G.T), ("the Gram is not symmetric", kind, n, d)
        assert torch.equal(G, want.to(acc)), ("gram", kind, n, d, int((G != want.to(acc)).sum()))
        assert torch.equal(want, want.T)


def check_int_affine(k, dev, dtype, n, d, m):
    for kind in MU_KINDS:
        X, rows, mu = int_case(n, d, kind)
        _, _, Xc = int_reference(X, rows, mu)
        W = randint(17 * m + d, -1, 2, (m, d))
        Y = run_affine(k, place(X, dtype, dev), d, rows.to(dev), mu, W).cpu()
        want = (Xc @ W.T).to(_hip.acc_dtype(dtype)).to(dtype)      # exact in the accumulate type, rounded once
        assert torch.equal(Y, want), ("project_affine", kind, n, d, m)
        absent = ~present_mask(rows, X.shape[0])
        assert bool((Y[absent] == 0).all())


def check_streaming(k, dev, dtype, d, data="int", n=4300):
    """ACCUMULATE over blocks of 2048 rows == one call, bit for bit, sums and Gram: on the integer case (where both are
    the int64 reference too) and on float data, where the order of the chunks shows."""
    acc = _hip.acc_dtype(dtype)
    if data == "int":
        X, rows, mu = int_case(n, d, "integer")
    else:
        X = (torch.randn(n + 2, d, generator=gen(5), dtype=F64) * 1.5 + 0.7).to(dtype)
        rows = torch.randperm(n + 2, generator=gen(6))[:n].to(torch.int32)
        rows[2] = n + 9
        mu = torch.randn(d, generator=gen(8), dtype=F64).to(acc)
    Z, r = place(X, dtype, dev), rows.to(dev)
    one_s, one_G = run_sums(k, Z, d, r), run_gram(k, Z, d, r, mu)
    s = G = None
    for a in range(0, n, CHUNK):
        s = run_sums(k, Z, d, r[a:a + CHUNK], accumulate=a > 0, sums=s)
        G = run_gram(k, Z, d, r[a:a + CHUNK], mu, accumulate=a > 0, G=G)
    assert torch.equal(s.cpu(), one_s.cpu()), "streamed column sums"
    assert torch.equal(G.cpu(), one_G.cpu()), "streamed Gram"
    assert not bool(torch.isnan(one_G).any()) and torch.equal(one_G.cpu(), one_G.cpu().T)
    if data == "int":
        want_s, want_G, _ = int_reference(X, rows, mu)
        assert torch.equal(s.cpu(), want_s.double()) and torch.equal(G.cpu(), want_G.to(acc))


# ---- the plain-torch double of the three calls -----------------------------------------------------------------------------
class TorchPca:
    """What csrc/content_pca.h computes, in torch on any device: chunks of 2048 rows added in chunk order, ACCUMULATE,
    only the upper tile pairs computed and mirrored, absent rows skipped, columns [0, d) alone read.  `mutation` breaks
    one of these on purpose (tests/test_reduce_host.py)."""

    def __init__(self, mutation=None):
        assert mutation in (None, "drop_chunk", "no_mirror", "mu_one_operand", "read_pad")
        self.mutation = mutation

    def column_sums_ws_len(self, n, d):
        return max(1, -(-n // CHUNK)) * d

    def gram_ws_len(self, n, d):
        return max(1, -(-n // CHUNK)) * d * d

    def _rows(self, Z, d, rows, acc):
        """(the listed rows' columns [0, d) in `acc`, which of them are present)."""
        ok = (rows >= 0) & (rows < Z.shape[0])
        at = rows.long().clamp(0, Z.shape[0] - 1)
        Xg = Z[at, :d].to(acc)
        if self.mutation == "read_pad" and Z.stride(0) > d:     # the pad column behind a row leaks into its last real one
            Xg[:, d - 1] += torch.as_strided(Z, (Z.shape[0], d + 1), (Z.stride(0), 1))[at, d].to(acc)
        return Xg, ok

    def column_sums(self, Z, d, rows, ws, sums, accumulate=False):
        Xg, ok = self._rows(Z, d, rows, F64)
        s = sums.clone() if accumulate else torch.zeros_like(sums)
        chunks = list(range(0, rows.numel(), CHUNK))
        for a in (chunks[:-1] if self.mutation == "drop_chunk" and len(chunks) > 1 else chunks):
            part = torch.zeros(d, dtype=F64, device=Z.device)
            for t in range(16):                             # thread t: rows t, t + 16, .. -- then the threads in order
                sel = Xg[a:a + CHUNK][t::16][ok[a:a + CHUNK][t::16]]
                part = part + sel.sum(0) if t else sel.sum(0)
            s = s + part
        sums.copy_(s)

    def gram(self, Z, d, rows, mu, ws, G, accumulate=False):
        acc = _hip.acc_dtype(Z.dtype)
        Xg, ok = self._rows(Z, d, rows, acc)
        Xc = Xg - mu if mu is not None else Xg
        Xc = torch.where(ok[:, None], Xc, torch.zeros_like(Xc))
        left = torch.where(ok[:, None], Xg, torch.zeros_like(Xg)) if self.mutation == "mu_one_operand" else Xc
        tile = torch.arange(d, device=Z.device) // TILE
        upper = tile[:, None] <= tile[None, :]
        s = G.clone() if accumulate else torch.zeros_like(G)
        chunks = list(range(0, rows.numel(), CHUNK))
        for a in (chunks[:-1] if self.mutation == "drop_chunk" and len(chunks) > 1 else chunks):
            s = s + left[a:a + CHUNK].T @ Xc[a:a + CHUNK]
        if self.mutation == "no_mirror":
            G.copy_(torch.where(upper, s, G))
        else:
            G.copy_(torch.where(upper, s, s.T))

    def project_affine(self, Z, d, rows, mu, W, Y):
        acc = _hip.acc_dtype(Z.dtype)
        Xg, ok = self._rows(Z, d, rows, acc)
        Xc = Xg - mu if mu is not None else Xg
        Xc = torch.where(ok[:, None], Xc, torch.zeros_like(Xc))
        Y[:rows.numel(), :W.shape[0]] = (Xc @ W.T).to(Y.dtype)


# ---- random float data: the dense-bits contract ------------------------------------------------------------------------------
FLOAT_N, FLOAT_R = 4300, 600


@functools.lru_cache(maxsize=None)
def float_case(d, dtype):
    """(X [FLOAT_R, d] in dtype, rows int32 [FLOAT_N] with absent entries, mu [d] in the accumulate dtype)."""
    acc = _hip.acc_dtype(dtype)
    X = (torch.randn(FLOAT_R, d, generator=gen(21), dtype=F64) + 0.4).to(dtype)
    rows = randint(22, 0, FLOAT_R, (FLOAT_N,))
    rows[5::37] = -1
    rows[11::37] = FLOAT_R + 5
    mu = (torch.randn(d, generator=gen(23), dtype=F64) * 0.5 + 0.4).to(acc)
    return X, rows.to(torch.int32), mu


def centred_table(X, mu):
    """widen(X) - mu: one subtraction per element in the accumulate dtype, on the host."""
    return X.to(mu.dtype) - mu


def check_gram_is_probe_grad(k, dev, dtype, d):
    """clane_gram_*(X, mu) == clane_probe_grad_* with G = the centred rows, the table = the centred table, K = d."""
    acc = _hip.acc_dtype(dtype)
    X, rows, mu = float_case(d, dtype)
    n = rows.numel()
    G = run_gram(k, place(X, dtype, dev), d, rows.to(dev), mu).cpu()
    Xc = centred_table(X, mu)
    ok = present_mask(rows, FLOAT_R)
    G_in = torch.where(ok[:, None], Xc[rows.long().clamp(0, FLOAT_R - 1)], torch.zeros(1, dtype=acc))
    ws = torch.full((k.probe_grad_ws_len(n, d, d),), float("nan"), dtype=acc, device=dev)
    dW = torch.full((d, d), float("nan"), dtype=acc, device=dev)
    db = torch.full((d,), float("nan"), dtype=acc, device=dev)
    k.probe_grad(place(Xc, acc, dev), d, rows.to(dev), G_in.contiguous().to(dev).view(-1), ws, dW.view(-1), db)
    assert not bool(torch.isnan(G).any())
    assert torch.equal(G, dW.cpu()), ("gram != probe_grad", d, int((G != dW.cpu()).sum()))
    assert torch.equal(G, G.T)
    assert torch.equal(run_gram(k, place(X, dtype, dev), d, rows.to(dev), mu).cpu(), G), "two calls differ"


def check_affine_is_project_rows(k, dev, dtype, d, m):
    """clane_project_affine_*(X, mu, W) == clane_project_rows_* on the pre-centred table (bf16: the f32 instance on the
    widened centred table, rounded once to bf16); two calls agree; a row's Y does not depend on its place in rows."""
    acc = _hip.acc_dtype(dtype)
    assert m <= 2 * d
    X, _, mu = float_case(d, dtype)
    rows = randint(31, 0, FLOAT_R, (300,))
    rows[5::37] = -1
    rows[11::37] = FLOAT_R + 5
    rows[list(SAME_ROW_AT)] = 17
    rows = rows.to(torch.int32)
    W = (torch.randn(m, d, generator=gen(32), dtype=F64) * 0.3).to(acc)
    Y = run_affine(k, place(X, dtype, dev), d, rows.to(dev), mu, W).cpu()
    W2 = torch.zeros(2 * d, d, dtype=acc)
    W2[:m] = W
    Y2 = torch.full((FLOAT_R, 2 * d), float("nan"), dtype=acc, device=dev)
    k.project_rows(place(centred_table(X, mu), acc, dev), d, W2.to(dev), Y2)
    ok = present_mask(rows, FLOAT_R)
    want = torch.where(ok[:, None], Y2.cpu()[rows.long().clamp(0, FLOAT_R - 1), :m], torch.zeros(1, dtype=acc)).to(dtype)
    assert torch.equal(Y, want), ("project_affine != project_rows", d, m, int((Y != want).sum()))
    assert torch.equal(run_affine(k, place(X, dtype, dev), d, rows.to(dev), mu, W).cpu(), Y), "two calls differ"
    first = Y[SAME_ROW_AT[0]]
    for p in SAME_ROW_AT:
        assert torch.equal(Y[p], first), ("a row's Y depends on its place", p)


# ---- against float64: the derived bound ------------------------------------------------------------------------------------
PLANTED = (16.0, 12.0, 9.0, 6.0, 4.0)


@functools.lru_cache(maxsize=None)
def planted_matrix(dtype, n=700, d=130):
    """[n, d]: five planted variances over a unit floor, rotated by a random orthogonal matrix, every column offset by 3;
    rounded to dtype."""
    g = gen(41)
    scale = torch.ones(d, dtype=F64)
    scale[:len(PLANTED)] = torch.tensor(PLANTED, dtype=F64).sqrt()
    Q, _ = torch.linalg.qr(torch.randn(d, d, generator=g, dtype=F64))
    return ((torch.randn(n, d, generator=g, dtype=F64) * scale) @ Q + 3.0).to(dtype)


def gram_bound(X, mean, dtype):
    """(G64, bound): the float64 Gram of X (as rounded to its dtype) about `mean`, and the element-wise bound
    (2048 + chunks + 2) u |Xc|^T |Xc| of a chunked sum in the accumulate type."""
    n = X.shape[0]
    Xc = X.double() - torch.as_tensor(mean, dtype=F64)
    chunks = -(-n // CHUNK)
    u = UNIT[_hip.acc_dtype(dtype)]
    return Xc.T @ Xc, (CHUNK + chunks + 2) * u * (Xc.abs().T @ Xc.abs())


def reference_axes(G64, dim):
    """numpy's eigh of the float64 Gram: (eigenvalues descending [d], components [dim, d] under the sign rule,
    gap_j = the distance of eigenvalue j to the nearest other one)."""
    from clane_amd.reduce import fix_signs
    lam, vec = np.linalg.eigh(G64.numpy())
    lam, vec = lam[::-1].copy(), vec[:, ::-1].copy()
    gaps = np.array([np.min(np.abs(np.delete(lam, j) - lam[j])) for j in range(dim)])
    return lam, fix_signs(vec[:, :dim].T), gaps


def check_gram_bound(k, dev, dtype, report=print):
    """The kernels' column sums and Gram of the planted matrix against float64; returns the worst fraction of the bound."""
    acc = _hip.acc_dtype(dtype)
    X = planted_matrix(dtype)
    n, d = X.shape
    Z, rows = place(X, dtype, dev), torch.arange(n, dtype=torch.int32, device=dev)
    sums = run_sums(k, Z, d, rows).cpu()
    exact = X.double().sum(0)
    assert float((sums - exact).abs().max()) <= n * 2.0 ** -53 * float(X.double().abs().sum(0).max()), "column sums"
    mean = (sums / n).to(acc)
    G = run_gram(k, Z, d, rows, mean).cpu().double()
    G64, bound = gram_bound(X, mean.double(), dtype)
    frac = float(((G - G64).abs() / bound).max())
    report(f"gram {case_id(dtype)}: max |G - G64| / bound = {frac:.4g}")
    assert frac <= 1.0
    return frac


def check_fit_bounds(pca, X, dtype, report=print):
    """A fitted ContentPCA(5) of the planted matrix: explained variances within ||bound||_F / (n - 1) (Weyl), each
    component within 2 ||bound||_F / gap_j of the reference's (Davis-Kahan)."""
    n = X.shape[0]
    G64, bound = gram_bound(X, pca.mean_, dtype)
    bF = float(torch.linalg.norm(bound))
    lam, comp, gaps = reference_axes(G64, pca.dim)
    ev_err = np.abs(pca.explained_variance_ - lam[:pca.dim] / (n - 1)).max()
    report(f"fit {case_id(dtype)}: |ev - ev64| max = {ev_err:.4g}, bound = {bF / (n - 1):.4g}")
    assert ev_err <= bF / (n - 1)
    for j in range(pca.dim):
        err = float(np.linalg.norm(pca.components_[j] - comp[j]))
        report(f"fit {case_id(dtype)}: component {j}: error {err:.4g}, bound {2 * bF / gaps[j]:.4g}")
        assert 2 * bF / gaps[j] < 0.5, "a vacuous bound"
        assert err <= 2 * bF / gaps[j]
    assert abs(pca.total_variance_ - float(torch.diagonal(G64).sum()) / (n - 1)) <= bF / (n - 1) * X.shape[1] ** 0.5
    return bF
