"""Fixtures, references and checks of the sparse content reduction (clane_amd/sparse.py, ContentPCA.fit_sparse,
csrc/sparse_rows.h) -- helpers of tests/test_gpu_sparse_reduce.py (the HIP kernels) and tests/test_sparse_reduce_host.py
(a plain-torch double of the calls, run through the same checks, and its mutations).

A check takes the kernel object `k` (``csr_spmm`` / ``csr_row_sums`` / ``csr_spmm_segment`` and the dense calls of
reduce_cases.TorchPca) and the device the operands go to, so one text serves the GPU and the double.

Integer data: values and B in {-2 .. 2}, a and s in {-2 .. 2}: every sum is an integer below 4 * (3 SEG + 5) + 4 < 2^24,
exact in float32, so the int64 reference is compared with torch.equal.

Order data: float32 numbers of 12 significant bits.  The product of two is exact in float32, so one fmaf(v, b, acc) is the
float32 sum ``acc + v * b`` that numpy forms, and `ordered_spmm` restates the header's summation order bit for bit.
"""
import functools

import numpy as np
import torch

from clane_amd.reduce import ContentPCA, fix_signs
from clane_amd.sparse import SEGMENT, SparseRows

from . import reduce_cases as RC

F32, F64 = torch.float32, torch.float64
SEG = SEGMENT
U = 2.0 ** -24
INT_L = (4, 20, 64, 132, 256, 512)
EPILOGUES = ("none", "s", "a_s")
PAD = 4                                     # columns behind l in B (NaN) and in out (a sentinel)
SENTINEL = 77.0
SPECIAL_LENGTHS = (0, 1, 64, 65, SEG, SEG + 1, 3 * SEG + 5)
INT_ROWS, INT_D = 67, 3 * SEG + 64

# explained variances of the device fit against the float64 restatement with the same Omega, relative: 8 x the larger of
# the fp32 numpy emulation's 6.1e-7 and the device's measured value (see test_gpu_sparse_reduce.py)
EV_EMULATED = 6.1e-7
EV_DEVICE_MEASURED = 1.79e-6             # MI355X, the largest of dim = 8, 16, 32 (1.60e-6, 1.79e-6, 1.21e-6)
EV_REL_BOUND = 8 * max(EV_EMULATED, EV_DEVICE_MEASURED)
CAPTURE = 0.999
FIT_DIMS = (8, 16, 32)


def rng(seed):
    return np.random.default_rng(seed)


# ---- matrices ------------------------------------------------------------------------------------------------------------
def rows_matrix(lengths, D, seed, values, last_column_in=None):
    """SparseRows with the given row lengths, columns drawn without replacement (ascending), values by ``values(rng, k)``;
    row ``last_column_in`` holds column D - 1."""
    g = rng(seed)
    rowptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=rowptr[1:])
    cols, vals = [], []
    for i, k in enumerate(lengths):
        c = np.sort(g.choice(D, size=k, replace=False)) if k else np.empty(0, np.int64)
        if i == last_column_in and k:
            c[-1] = D - 1
        cols.append(c)
        vals.append(values(g, k))
    col = np.concatenate(cols).astype(np.int32)
    return SparseRows(rowptr, col, np.concatenate(vals).astype(np.float32), (len(lengths), D))


def int_values(g, k):
    return g.choice(np.array([-2, -1, 1, 2], dtype=np.float32), size=k)


def short_mantissa(x):
    """float32 numbers cut to 12 significant bits."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return (x.view(np.int32) & np.int32(-4096)).view(np.float32)


def order_values(g, k):
    return short_mantissa(g.standard_normal(k) * 3 + 0.5)


def _lengths(seed):
    g = rng(seed)
    lengths = list(g.integers(0, 41, size=INT_ROWS))
    for at, k in zip(g.choice(INT_ROWS, size=len(SPECIAL_LENGTHS), replace=False), SPECIAL_LENGTHS):
        lengths[int(at)] = k
    return [int(x) for x in lengths]


@functools.lru_cache(maxsize=None)
def int_matrix():
    lengths = _lengths(1)
    return rows_matrix(lengths, INT_D, 2, int_values, last_column_in=lengths.index(3 * SEG + 5))


@functools.lru_cache(maxsize=None)
def one_row_matrix():
    return rows_matrix([70], 300, 3, int_values, last_column_in=0)


@functools.lru_cache(maxsize=None)
def order_matrix():
    """Float data of 12-bit numbers: short rows, one row of SEG + 1 and one of 2 SEG + 70 non-zeros."""
    g = rng(4)
    lengths = [int(x) for x in g.integers(0, 90, size=40)]
    lengths[7], lengths[22], lengths[31] = SEG + 1, 2 * SEG + 70, 0
    return rows_matrix(lengths, 2 * SEG + 200, 5, order_values, last_column_in=22)


def numpy_csr(S):
    return S.rowptr.cpu().numpy(), S.col.cpu().numpy(), S.val.cpu().numpy()


def numpy_transpose(S):
    """(rowptr, col, val) of the transpose by a stable argsort of the columns: ascending original rows in every row."""
    rowptr, col, val = numpy_csr(S)
    n, D = S.shape
    row = np.repeat(np.arange(n, dtype=np.int32), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    t_rowptr = np.zeros(D + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=D), out=t_rowptr[1:])
    return t_rowptr, row[order], val[order]


def swapped_transpose(S):
    """``S.transposed()`` with the second and third entry of its longest row exchanged: the same matrix, another order
    ((p0 + p2) + p1 instead of (p0 + p1) + p2)."""
    T = S.transposed()
    lens = (T.rowptr[1:] - T.rowptr[:-1])
    assert int(lens.max()) >= 3
    e = int(T.rowptr[int(lens.argmax())]) + 1
    col, val = T.col.clone(), T.val.clone()
    col[[e, e + 1]] = T.col[[e + 1, e]]
    val[[e, e + 1]] = T.val[[e + 1, e]]
    return SparseRows(T.rowptr, col, val, T.shape, _trusted=True)


# ---- references ------------------------------------------------------------------------------------------------------------
def segment_sum(colr, valr, B, l):
    """Steps 1 and 2 of the header's order on one segment, in numpy float32."""
    epw = 4 if l <= 64 else 2 if l <= 128 else 1
    subs = []
    for sub in range(epw):
        acc = np.zeros(l, dtype=np.float32)
        for j in range(sub, len(colr), epw):
            acc = acc + valr[j] * B[colr[j]]
        subs.append(acc)
    if epw == 4:
        return (subs[0] + subs[2]) + (subs[1] + subs[3])
    return subs[0] + subs[1] if epw == 2 else subs[0]


def ordered_spmm(rowptr, col, val, B, l, a=None, s=None, drop_segment=False):
    """The header's order on float32 numpy arrays (B [D, l]); exact where v * b is (see the module text)."""
    n = len(rowptr) - 1
    out = np.zeros((n, l), dtype=np.float32)
    for r in range(n):
        e0, e1 = int(rowptr[r]), int(rowptr[r + 1])
        starts = list(range(e0, e1, SEG)) or [e0]
        if drop_segment and len(starts) > 1:
            starts = starts[:-1]
        total = None
        for b0 in starts:
            part = segment_sum(col[b0:min(b0 + SEG, e1)], val[b0:min(b0 + SEG, e1)], B, l)
            total = part if total is None else total + part
        if s is not None:
            ar = np.float32(1.0) if a is None else a[r]
            total = total - ar * s[:l]                         # a * s exact on the test data: one rounding, as fmaf
        out[r] = total
    return out


def int_reference(S, B, a, s):
    """int64: S B - a s^T."""
    out = S.to_dense(torch.int64).cpu() @ B
    if s is not None:
        out = out - (torch.ones(S.shape[0], dtype=torch.int64) if a is None else a)[:, None] * s[None, :]
    return out


def place_B(B, dev, pad=PAD):
    buf = torch.full((B.shape[0], B.shape[1] + pad), float("nan"), dtype=F32, device=dev)
    buf[:, :B.shape[1]] = B.to(F32).to(dev)
    return buf[:, :B.shape[1]]


def run_spmm(k, S, B, l, a=None, s=None, dev=None):
    """csr_spmm into a padded output whose sentinel columns must survive; B with NaN behind its l columns."""
    dev = S.device if dev is None else dev
    buf = torch.full((S.shape[0], l + PAD), SENTINEL, dtype=F32, device=dev)
    k.csr_spmm(S, place_B(B, dev), l, buf[:, :l], a=None if a is None else a.to(F32).to(dev),
               s=None if s is None else s.to(F32).to(dev))
    assert bool((buf[:, l:] == SENTINEL).all()), "csr_spmm wrote behind its l columns"
    return buf[:, :l].cpu()


def epilogue_operands(kind, n, l, seed):
    if kind == "none":
        return None, None
    s = RC.randint(seed, -2, 3, (l,))
    return (RC.randint(seed + 1, -2, 3, (n,)) if kind == "a_s" else None), s


# ---- checks: exact integers --------------------------------------------------------------------------------------------
def check_int_spmm(k, dev, S, l):
    assert k.csr_spmm_segment() == SEG
    n, D = S.shape
    B = RC.randint(31 * l + n, -2, 3, (D, l))
    Sd = S.to(dev)
    for kind in EPILOGUES:
        a, s = epilogue_operands(kind, n, l, 7 * l + 3)
        got = run_spmm(k, Sd, B, l, a, s)
        want = int_reference(S, B, a, s)
        assert torch.equal(got, want.to(F32)), ("csr_spmm", kind, n, l, int((got != want.to(F32)).sum()))


def check_int_row_sums(k, dev, S):
    Sd = S.to(dev)
    sums = torch.full((S.shape[0],), float("nan"), dtype=F64, device=dev)
    k.csr_row_sums(Sd, sums)
    want = S.to_dense(torch.int64).sum(1)
    assert torch.equal(sums.cpu(), want.double()), "csr_row_sums"


def check_transpose(k, dev, transposed=lambda S: S.transposed(), l=20):
    """transposed() is numpy's stable transpose; SpMM on it is the int64 reference of S^T B."""
    S = int_matrix()
    T = transposed(S.to(dev))
    t_rowptr, t_col, t_val = numpy_transpose(S)
    assert T.shape == (S.shape[1], S.shape[0])
    assert np.array_equal(T.rowptr.cpu().numpy(), t_rowptr) and np.array_equal(T.col.cpu().numpy(), t_col), \
        "the transpose's rows do not list the original rows in ascending order"
    assert np.array_equal(T.val.cpu().numpy(), t_val)
    B = RC.randint(41, -2, 3, (S.shape[0], l))
    a, s = RC.randint(42, -2, 3, (S.shape[1],)), RC.randint(43, -2, 3, (l,))
    got = run_spmm(k, T, B, l, a, s)
    want = S.to_dense(torch.int64).cpu().T @ B - a[:, None] * s[None, :]
    assert torch.equal(got, want.to(F32)), "csr_spmm on the transpose"


# ---- checks: the fixed order ---------------------------------------------------------------------------------------------
def order_operands(S, l, seed):
    g = rng(seed)
    B = short_mantissa(g.standard_normal((S.shape[1], l)))
    a = short_mantissa(g.standard_normal(S.shape[0]) + 1)
    s = short_mantissa(g.standard_normal(l))
    return B, a, s


def check_order_bits(k, dev, l, S=None, transposed=None):
    """csr_spmm has the bits of the header's order restated in numpy: on the order matrix, or (``transposed``) on the
    transpose that function makes of it, against numpy's stable transpose."""
    S = order_matrix() if S is None else S
    if transposed is None:
        M, csr = S.to(dev), numpy_csr(S)
    else:
        M, csr = transposed(S.to(dev)), numpy_transpose(S)
    B, a, s = order_operands(M, l, 50 + l)
    got = run_spmm(k, M, torch.from_numpy(B), l, torch.from_numpy(a), torch.from_numpy(s))
    want = torch.from_numpy(ordered_spmm(*csr, B, l, a, s))
    assert torch.equal(got, want), ("csr_spmm leaves the written order", l, int((got != want).sum()))


def check_fixed_bits(k, dev, l=132):
    """Two calls agree; rows [a, b) as a matrix of their own (and re-based, in a call of their own) give the full call's
    bits; within (nnz_r + 2) u (sum |val| |B| + |a| |s|) of float64."""
    S = order_matrix()
    g = rng(60)
    n, D = S.shape
    B = torch.from_numpy(g.standard_normal((D, l)).astype(np.float32))
    a = torch.from_numpy(g.standard_normal(n).astype(np.float32))
    s = torch.from_numpy(g.standard_normal(l).astype(np.float32))
    Sd = S.to(dev)
    full = run_spmm(k, Sd, B, l, a, s)
    assert not bool(torch.isnan(full).any())
    assert torch.equal(run_spmm(k, Sd, B, l, a, s), full), "two calls differ"
    for lo, hi in ((5, 9), (20, 24), (0, n), (22, 23)):
        part = run_spmm(k, Sd.rows(lo, hi), B, l, a[lo:hi], s)
        assert torch.equal(part, full[lo:hi]), ("rows as a sub-matrix differ", lo, hi)
    rowptr, col, val = numpy_csr(S)
    lo, hi = 20, 24                                            # the same rows re-based in arrays of their own
    own = SparseRows(rowptr[lo:hi + 1] - rowptr[lo], col[rowptr[lo]:rowptr[hi]], val[rowptr[lo]:rowptr[hi]], (hi - lo, D))
    assert torch.equal(run_spmm(k, own.to(dev), B, l, a[lo:hi], s), full[lo:hi]), "a re-based sub-matrix differs"
    dense = S.to_dense(F64).cpu()
    exact = dense @ B.double() - a.double()[:, None] * s.double()[None, :]
    mag = dense.abs() @ B.double().abs() + a.double().abs()[:, None] * s.double().abs()[None, :]
    nnz_r = torch.from_numpy(np.diff(rowptr)).double()[:, None]
    frac = float(((full.double() - exact).abs() / ((nnz_r + 2) * U * mag).clamp(min=1e-300)).max())
    print(f"csr_spmm l={l}: max |out - out64| / bound = {frac:.4g}")
    assert frac <= 1.0
    return frac


# ---- the plain-torch double ------------------------------------------------------------------------------------------------
class TorchSparse(RC.TorchPca):
    """What csrc/sparse_rows.h computes, on any device.  ``ordered``: the header's summation order restated (slow: small
    matrices); else one float32 index_add per product (the fit).  `mutation` breaks one thing on purpose."""

    def __init__(self, ordered=True, mutation=None):
        super().__init__()
        assert mutation in (None, "drop_segment", "no_epilogue", "ignore_a")
        self.ordered, self.sparse_mutation = ordered, mutation

    def csr_spmm_segment(self):
        return SEG

    def csr_spmm_ws_len(self, n_rows, nnz, l):
        return max(1, 2 * (nnz // SEG)) * l

    def csr_spmm(self, S, B, l, out, a=None, s=None, ws=None):
        n = S.shape[0]
        if self.sparse_mutation == "no_epilogue":
            s = None
        if self.sparse_mutation == "ignore_a":
            a = None
        rowptr = (S.rowptr - S.rowptr[0]).cpu()
        e0 = int(S.rowptr[0])
        col, val = S.col[e0:e0 + int(rowptr[-1])].cpu(), S.val[e0:e0 + int(rowptr[-1])].cpu()
        Bl = B[:, :l].cpu()
        if self.ordered:
            res = torch.from_numpy(ordered_spmm(rowptr.numpy(), col.numpy(), val.numpy(), Bl.contiguous().numpy(), l,
                                                None if a is None else a.cpu().numpy(),
                                                None if s is None else s.cpu().numpy(),
                                                drop_segment=self.sparse_mutation == "drop_segment"))
        else:
            row = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
            res = torch.zeros(n, l, dtype=F32).index_add_(0, row, val[:, None] * Bl[col.long()])
            if s is not None:
                res = res - (torch.ones(n) if a is None else a.cpu())[:, None] * s.cpu()[None, :l]
        out[:n, :l] = res.to(out.device)

    def csr_row_sums(self, S, sums, ws=None):
        rowptr = (S.rowptr - S.rowptr[0]).cpu().numpy()
        e0 = int(S.rowptr[0])
        val = S.val[e0:e0 + int(rowptr[-1])].cpu().double().numpy()
        res = np.zeros(S.shape[0])
        for r in range(S.shape[0]):
            starts = list(range(int(rowptr[r]), int(rowptr[r + 1]), SEG))
            if self.sparse_mutation == "drop_segment" and len(starts) > 1:
                starts = starts[:-1]
            for b0 in starts:
                res[r] += val[b0:min(b0 + SEG, int(rowptr[r + 1]))].sum()
        sums.copy_(torch.from_numpy(res).to(sums.device))


# ---- the fit -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bag_of_words(n=3000, D=700, topics=12, nnz_row=40, seed=0, noise=0.15):
    """A synthetic bag of words: every row draws about ``nnz_row`` words from one of ``topics`` Zipf distributions (each
    over its own permutation of the vocabulary) mixed with a global one; the counts are the values."""
    g = rng(seed)
    base = 1.0 / np.arange(1, D + 1) ** 1.1
    perms = [g.permutation(D) for _ in range(topics)]
    glob = base / base.sum()
    lengths, cols, vals = [], [], []
    for _ in range(n):
        t = g.integers(topics)
        p = (1 - noise) * base[np.argsort(perms[t])] / base.sum() + noise * glob
        words = g.choice(D, size=max(1, g.poisson(nnz_row)), p=p / p.sum())
        u, c = np.unique(words, return_counts=True)
        lengths.append(len(u))
        cols.append(u)
        vals.append(c.astype(np.float32))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=rowptr[1:])
    return SparseRows(rowptr, np.concatenate(cols), np.concatenate(vals), (n, D))


@functools.lru_cache(maxsize=None)
def exact_pca(center=True):
    """(Xc float64 [n, D], eigenvalues / (n - 1) descending) of the densified bag of words."""
    X = bag_of_words().to_dense(F64).numpy()
    Xc = X - X.mean(0) if center else X
    sig = np.linalg.svd(Xc, compute_uv=False)
    return Xc, sig ** 2 / (X.shape[0] - 1)


def omega(D, l, seed):
    """The fit's own draw: N(0, 1) float32 from a CPU generator."""
    return torch.randn(D, l, generator=torch.Generator().manual_seed(seed), dtype=F32).double().numpy()


def orth64(Y):
    lam, V = np.linalg.eigh(Y.T @ Y)
    keep = lam > lam.max() * 1e-12
    return Y @ (V[:, keep] / np.sqrt(lam[keep]))


@functools.lru_cache(maxsize=None)
def restated_fit(dim, oversample=16, power_iterations=4, seed=0, center=True):
    """The algorithm of ContentPCA.fit_sparse in float64 numpy on the dense matrix, with the same Omega: (components,
    explained variances)."""
    X = bag_of_words().to_dense(F64).numpy()
    n, D = X.shape
    mu = X.mean(0) if center else np.zeros(D)
    Xc = X - mu
    Q = orth64(orth64(Xc @ omega(D, min(dim + oversample, D, n), seed)))
    for _ in range(power_iterations):
        Z = orth64(orth64(Xc.T @ Q))
        Q = orth64(orth64(Xc @ Z))
    _, sig, Vt = np.linalg.svd((Xc.T @ Q).T, full_matrices=False)
    return fix_signs(Vt[:dim]), sig[:dim] ** 2 / (n - 1)


def fit(dev, dim, **kw):
    fit_kw = {key: kw.pop(key) for key in ("oversample", "power_iterations", "seed") if key in kw}
    return ContentPCA(dim, **kw).fit_sparse(bag_of_words().to(dev), **fit_kw)


def check_fit_against_exact(dev, dim, report=print):
    """The variance the fitted components capture is at least CAPTURE of the exact top-dim variance; the components are
    orthonormal to 1e-6; the explained variances are within EV_REL_BOUND (relative) of the float64 restatement's."""
    pca = fit(dev, dim)
    Xc, ev = exact_pca()
    n = Xc.shape[0]
    C = pca.components_
    assert C.shape == (dim, Xc.shape[1]) and pca.n_samples_ == n
    ortho = float(np.abs(C @ C.T - np.eye(dim)).max())
    captured = float(((Xc @ C.T) ** 2).sum() / (n - 1))
    ratio = captured / float(ev[:dim].sum())
    _, ev64 = restated_fit(dim)
    rel = float(np.max(np.abs(pca.explained_variance_ - ev64) / ev64))
    report(f"fit_sparse dim={dim}: captured / exact = {ratio:.6f}, orthonormal to {ortho:.3g}, "
           f"explained variance vs the float64 restatement: {rel:.3g} (bound {EV_REL_BOUND:.3g})")
    assert ortho <= 1e-6
    assert ratio >= CAPTURE
    assert rel <= EV_REL_BOUND
    total = float((Xc ** 2).sum() / (n - 1))
    assert abs(pca.total_variance_ - total) <= 1e-6 * total
    assert np.allclose(pca.explained_variance_ratio_, pca.explained_variance_ / pca.total_variance_)
    assert np.allclose(pca.mean_, bag_of_words().to_dense(F64).numpy().mean(0), atol=2 * U * 8)
    return rel


def check_seeds(dev, dim=8):
    one, two, other = fit(dev, dim), fit(dev, dim), fit(dev, dim, seed=1)
    for name in ("components_", "mean_", "explained_variance_", "explained_variance_ratio_"):
        assert np.array_equal(getattr(one, name), getattr(two, name)), ("the same seed, other bits", name)
    assert not np.array_equal(one.components_, other.components_), "another seed, the same bits"
    assert np.array_equal(one.mean_, other.mean_)


def check_uncentred(dev, dim=8):
    pca = fit(dev, dim, center=False)
    X, ev = exact_pca(center=False)
    assert not pca.mean_.any()
    captured = float(((X @ pca.components_.T) ** 2).sum() / (X.shape[0] - 1))
    assert captured >= CAPTURE * float(ev[:dim].sum())
    _, ev64 = restated_fit(dim, center=False)
    assert float(np.max(np.abs(pca.explained_variance_ - ev64) / ev64)) <= EV_REL_BOUND


def check_whiten(dev, dim=8):
    """Column j's sample variance is |Xc v_j|^2 / sigma_j^2, sigma_j = |Q^T Xc v_j| <= |Xc v_j|: 1 plus what of Xc v_j
    the sketch Q misses.  The float64 restatement gives that excess; the device's denominator is within EV_REL_BOUND of
    the restatement's and its numerator, a float32 sum of about 45 terms per entry, within 2 * 48 u: 4 EV_REL_BOUND."""
    S = bag_of_words().to(dev)
    pca = ContentPCA(dim, whiten=True)
    Y = pca.fit_transform_sparse(S).cpu().double()
    var = Y.var(0, unbiased=True).numpy()
    Xc, _ = exact_pca()
    C64, ev64 = restated_fit(dim)
    want = ((Xc @ C64.T) ** 2).sum(0) / (Xc.shape[0] - 1) / ev64
    print(f"whiten: column variances - 1 in [{(var - 1).min():.3g}, {(var - 1).max():.3g}], the restatement's "
          f"[{(want - 1).min():.3g}, {(want - 1).max():.3g}]")
    assert (want >= 1 - 1e-12).all() and (want - 1).max() <= 1 - CAPTURE
    assert np.abs(var - want).max() <= 4 * EV_REL_BOUND, (var, want)
    plain = ContentPCA(dim).fit_sparse(S)
    assert np.array_equal(plain.components_, pca.components_)
    Yp = plain.transform_sparse(S).cpu().double() / torch.from_numpy(np.sqrt(plain.explained_variance_))
    X = bag_of_words().to_dense(F64)
    W, mu = torch.from_numpy(plain.components_), torch.from_numpy(plain.mean_)
    mag = ((X.abs() + mu.abs()) @ W.abs().T) / torch.from_numpy(np.sqrt(plain.explained_variance_))
    nnz_r = torch.from_numpy(np.diff(bag_of_words().rowptr.numpy())).double()[:, None]
    assert bool(((Y - Yp).abs() <= 2 * (nnz_r + 5) * U * mag).all()), "whitening is not folded into W"


@functools.lru_cache(maxsize=None)
def rank_five_matrix(n=400, D=60):
    g = rng(9)
    basis = g.integers(0, 4, size=(5, D)).astype(np.float32)
    X = g.integers(1, 6, size=(n, 1)).astype(np.float32) * basis[g.integers(0, 5, size=n)]
    return SparseRows.from_dense(X)


def check_rank_deficient(dev):
    import pytest
    S = rank_five_matrix().to(dev)
    pca = ContentPCA(4).fit_sparse(S)
    X = rank_five_matrix().to_dense(F64).numpy()
    Xc = X - X.mean(0)
    ev = np.linalg.svd(Xc, compute_uv=False) ** 2 / (X.shape[0] - 1)
    captured = float(((Xc @ pca.components_.T) ** 2).sum() / (X.shape[0] - 1))
    assert captured >= CAPTURE * float(ev[:4].sum())
    with pytest.raises(ValueError, match=r"numerical rank [0-9]+ of D = 60"):
        ContentPCA(8).fit_sparse(S)


def check_transform_and_files(dev, tmp_path, dense_transform=None):
    """transform_sparse(S) against the float64 value within the two float32 sums' bound (the sparse product's
    (nnz_r + 2) u, the dense projection's (D + 2) u, on |W| (|x| + |mu|)) -- and, with ``dense_transform`` (the GPU:
    ContentPCA.transform), against it within the sum of the two; save / load reproduces the output's bits."""
    S = bag_of_words()
    pca = fit(dev, 16)
    Y = pca.transform_sparse(S.to(dev))
    assert Y.dtype == F32 and tuple(Y.shape) == (S.shape[0], 16)
    X = S.to_dense(F64).cpu()
    W, mu = torch.from_numpy(pca.components_), torch.from_numpy(pca.mean_)
    exact = (X - mu) @ W.T
    mag = (X.abs() + mu.abs()) @ W.abs().T
    nnz_r = torch.from_numpy(np.diff(S.rowptr.numpy())).double()[:, None]
    W32 = 2 * U * (X.abs() + mu.abs()) @ W.abs().T              # W and W mu rounded to float32
    sparse_bound = (nnz_r + 3) * U * mag + W32
    assert bool(((Y.cpu().double() - exact).abs() <= sparse_bound).all())
    if dense_transform is not None:
        Yd = dense_transform(pca, S.to_dense(F32))
        dense_bound = (S.shape[1] + 3) * U * mag + W32
        assert bool(((Y.cpu().double() - Yd.cpu().double()).abs() <= sparse_bound + dense_bound).all())
    half = pca.transform_sparse(S.to(dev), dtype=torch.bfloat16)
    assert half.dtype == torch.bfloat16 and torch.equal(half.cpu(), Y.cpu().to(torch.bfloat16))
    back = ContentPCA.load(pca.save(tmp_path / "sparse_pca.npz"))
    assert torch.equal(back.transform_sparse(S.to(dev)).cpu(), Y.cpu())
    assert back.report(S.shape[1])["source"] == "load"
    assert torch.equal(ContentPCA(16).fit_transform_sparse(S.to(dev)).cpu(), Y.cpu())
