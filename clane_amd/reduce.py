"""Content reduction -- PCA of a wide ``[n, d]`` matrix (the bag-of-words ``C.npy`` of an attributed network) on the GPU.

Nothing in the reference does this: its users run a host PCA before the graph is loaded.  Here the three passes over the
data are HIP kernels (csrc/content_pca.h): deterministic column sums, the centred Gram ``Xc^T Xc`` on the matrix cores and
the affine projection ``W (x - mu)``.  The ``d x d`` eigen-problem in between is plumbing: ``torch.linalg.eigh`` in
float64 on the host.

Every sum runs in a fixed order, and a matrix that is streamed in blocks gives the bits of one call: a fit is
reproducible bit for bit, whatever ``block_rows``.

Sparse content (a bag of words as CSR, sparse.SparseRows) never becomes dense: ``fit_sparse`` is the randomized range
finder with power iterations (Halko, Martinsson, Tropp 2011), its products the CSR kernels of csrc/sparse_rows.h, the
centring a rank-one epilogue of those products, the ``l x l`` eigen-problems and the final SVD float64 on the host.

There is no CPU fallback: without the library or a GPU, ``fit`` and ``transform`` raise ``ClaneHipError``.
"""
from __future__ import annotations

import contextlib
import os
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _hip

CHUNK_ROWS = 2048                   # kGradChunk: the rows of one partial sum
BLOCK_BYTE_BUDGET = 1 << 30         # a block of X on the device plus the Gram's workspace for it
MAX_CHUNKS = 65535                  # chunks of one launch

SECTION_KEYS = ("dim", "center", "whiten", "load", "sparse", "oversample", "power_iterations", "seed")
SPARSE_DEFAULTS = {"oversample": 16, "power_iterations": 4, "seed": 0}
MAX_SKETCH = 512                    # CLANE_CSR_MAX_L: dim + oversample
RANK_TOL = 1e-6                     # eigenvalues (squared singular values) below RANK_TOL * the largest are dropped: fp32
                                    # sums of up to n terms leave noise of about that size in a Gram
NPZ_KEYS = ("components", "mean", "explained_variance", "explained_variance_ratio", "total_variance", "n_samples",
            "dim", "center", "whiten")


def default_block_rows(d: int, dtype: torch.dtype) -> int:
    """Rows per block: the largest multiple of 2048 for which the block (``rows * d`` elements of ``dtype``) and the
    Gram's workspace for it (``rows / 2048 * d * d`` elements of the accumulate dtype) stay under BLOCK_BYTE_BUDGET
    together -- at least 2048, at most what one launch takes."""
    elt = torch.empty(0, dtype=dtype).element_size()
    acc = torch.empty(0, dtype=_hip.acc_dtype(dtype)).element_size()
    per_chunk = CHUNK_ROWS * d * elt + d * d * acc
    return CHUNK_ROWS * int(min(MAX_CHUNKS, max(1, BLOCK_BYTE_BUDGET // per_chunk)))


def fix_signs(components: np.ndarray) -> np.ndarray:
    """Each row's entry of largest magnitude (the lowest index on a tie) made positive."""
    comp = np.array(components, dtype=np.float64, copy=True)
    for j in range(comp.shape[0]):
        i = int(np.argmax(np.abs(comp[j])))           # numpy: the first of equal maxima
        if comp[j, i] < 0:
            comp[j] = -comp[j]
    return comp


def principal_axes(G: torch.Tensor, n: int, dim: int):
    """(components [dim, d], explained variance [dim], total variance, numerical rank) of the Gram ``G`` of ``n`` centred
    rows, float64 on the host: eigenvalues descending, clamped at 0, divided by ``n - 1``; signs by ``fix_signs``; the
    rank counts the eigenvalues that stay positive."""
    lam, vec = torch.linalg.eigh(G.detach().to("cpu", torch.float64))
    lam = torch.flip(lam, [0]).clamp(min=0.0)
    vec = torch.flip(vec, [1])
    comp = fix_signs(vec[:, :dim].T.contiguous().numpy())
    var = lam.numpy() / (n - 1)
    return comp, var[:dim].copy(), float(var.sum()), int((var > 0).sum())


def check_section(section, world_size: int = 1) -> dict:
    """The validated ``content_reduction`` section of a config: ``{"dim", "center", "whiten", "load"}``.  Before any
    graph is read."""
    if world_size > 1:
        raise NotImplementedError(
            "content_reduction: reducing the content runs on ONE GPU only (WORLD_SIZE > 1): several GPUs are out of scope")
    if not isinstance(section, dict):
        raise ValueError("content_reduction: expected a mapping with the key `dim` (or `load`)")
    unknown = sorted(set(section) - set(SECTION_KEYS))
    if unknown:
        raise ValueError(f"content_reduction: unknown keys {unknown}; known: {list(SECTION_KEYS)}")
    load = section.get("load")
    if load is not None and (not isinstance(load, str) or not load):
        raise ValueError(f"content_reduction: load must be the path of a saved transform, got {load!r}")
    dim = section.get("dim")
    if dim is None and load is None:
        raise ValueError("content_reduction: `dim`, the reduced width, is required unless `load` is given")
    if dim is not None and (isinstance(dim, bool) or not isinstance(dim, int) or dim < 1):
        raise ValueError(f"content_reduction: dim must be a positive integer, got {dim!r}")
    out = {"dim": dim, "load": load}
    for key in ("center", "whiten"):
        val = section.get(key, key == "center")
        if not isinstance(val, bool):
            raise ValueError(f"content_reduction: {key} must be true or false, got {val!r}")
        out[key] = val
    sparse = section.get("sparse")
    if sparse is None:
        extra = sorted(set(section) & set(SPARSE_DEFAULTS))
        if extra:
            raise ValueError(f"content_reduction: {extra} belong to `sparse` (the randomized fit of a CSR content file)")
        return out
    if not isinstance(sparse, str) or not sparse:
        raise ValueError(f"content_reduction: sparse must be the path of a CSR .npz file, got {sparse!r}")
    out["sparse"] = sparse
    for key, default in SPARSE_DEFAULTS.items():
        val = section.get(key, default)
        if isinstance(val, bool) or not isinstance(val, int) or val < 0:
            raise ValueError(f"content_reduction: {key} must be a non-negative integer, got {val!r}")
        out[key] = val
    if dim is not None and dim + out["oversample"] > MAX_SKETCH:
        raise ValueError(f"content_reduction: dim + oversample = {dim + out['oversample']} exceeds {MAX_SKETCH}")
    return out


def resolve_sparse(section: dict, data_root: Path):
    """The validated ``SparseRows`` of the section's ``sparse`` file (relative to ``data_root``); None without the key.
    A data root that also holds ``C.npy`` or ``C.pt`` is ambiguous: an error."""
    if section.get("sparse") is None:
        return None
    from .sparse import SparseRows
    path = Path(section["sparse"])
    if not path.is_absolute():
        path = Path(data_root) / path
    if not path.is_file():
        raise ValueError(f"content_reduction: sparse: {str(path)!r} is missing")
    dense = [name for name in ("C.npy", "C.pt") if (Path(data_root) / name).exists()]
    if dense:
        raise ValueError(f"content_reduction: sparse: {str(data_root)!r} also holds {dense}: which content is meant is "
                         f"ambiguous")
    try:
        return SparseRows.load_npz(path)
    except ValueError as e:
        raise ValueError(f"content_reduction: sparse: {e}") from None


def resolve_load(section: dict, data_root: Path) -> Optional[Path]:
    """The file of the section's ``load`` (relative to ``data_root``), which must exist; None without ``load``."""
    if section.get("load") is None:
        return None
    path = Path(section["load"])
    if not path.is_absolute():
        path = Path(data_root) / path
    if not path.is_file():
        raise ValueError(f"content_reduction: load: {str(path)!r} is missing")
    return path


class ContentPCA:
    """PCA of the rows of a matrix, the passes over the data on the GPU.

    ``fit(X)`` takes a host or device ``[n, d]`` tensor (float32, float64, bfloat16), ``block_rows`` rows at a time
    (default: ``default_block_rows``; a multiple of 2048 -- any such value gives the same bits): pass 1 the column sums
    (double), ``mean_ = sums / n`` rounded to the accumulate dtype; pass 2 the Gram of the centred rows.  Kept after a
    fit, as float64 numpy arrays: ``components_ [dim, d]`` (rows of unit norm, the entry of largest magnitude
    positive), ``mean_ [d]`` (zeros with ``center=False``), ``explained_variance_`` (eigenvalue / (n - 1)),
    ``explained_variance_ratio_``, and ``total_variance_``, ``n_samples_``.

    ``transform(X)`` returns ``(X - mean_) components_^T`` -- every column divided by the square root of its variance
    under ``whiten`` -- in ``X``'s dtype on ``X``'s device, rounded once."""

    def __init__(self, dim: int, center: bool = True, whiten: bool = False, block_rows: Optional[int] = None,
                 device=None):
        if isinstance(dim, bool) or int(dim) != dim or int(dim) < 1:
            raise ValueError(f"ContentPCA: dim must be a positive integer, got {dim!r}")
        if block_rows is not None and (int(block_rows) < CHUNK_ROWS or int(block_rows) % CHUNK_ROWS
                                       or int(block_rows) > CHUNK_ROWS * MAX_CHUNKS):
            raise ValueError(f"ContentPCA: block_rows must be a multiple of {CHUNK_ROWS} (the rows of one partial sum: "
                             f"only then does a streamed matrix give the bits of one call), at most "
                             f"{CHUNK_ROWS * MAX_CHUNKS}; got {block_rows!r}")
        self.dim, self.center, self.whiten = int(dim), bool(center), bool(whiten)
        self.block_rows = None if block_rows is None else int(block_rows)
        self.device = device
        self.fitted_from = None                      # "fit" or "load"
        self.components_ = self.mean_ = self.explained_variance_ = self.explained_variance_ratio_ = None
        self.total_variance_ = self.n_samples_ = None
        self.sparse_fit_ = None                      # {"nnz", "oversample", "power_iterations", "seed"} of a sparse run

    # ---- checks: before any launch --------------------------------------------------------------------------------
    def _check_fit_shape(self, n: int, d: int):
        if n < 2:
            raise ValueError(f"ContentPCA: a fit needs at least 2 rows, got n = {n}")
        if self.dim > min(d, n - 1):
            raise ValueError(f"ContentPCA: dim = {self.dim} exceeds min(d, n - 1) = {min(d, n - 1)} (d = {d}, n = {n})")

    @staticmethod
    def _check_matrix(X, what: str) -> torch.Tensor:
        X = torch.as_tensor(X)
        if X.dim() != 2:
            raise ValueError(f"ContentPCA.{what}: X must be a 2-D [n, d] matrix, got shape {tuple(X.shape)}")
        _hip.acc_dtype(X.dtype)                      # TypeError for anything but fp32 / fp64 / bf16
        return X

    def _rows_per_block(self, d: int, dtype) -> int:
        return self.block_rows if self.block_rows is not None else default_block_rows(d, dtype)

    # ---- the data, a block at a time ------------------------------------------------------------------------------
    def _matrix_blocks(self, X: torch.Tensor, dev):
        """A callable that yields (table, rows) per block of ``X``: the block on the device with rows 0 .. b - 1.  A host
        matrix is uploaded block by block on every pass; one that fits a single block is uploaded once."""
        n, d = X.shape
        step = self._rows_per_block(d, X.dtype)
        ar = torch.arange(min(step, n), dtype=torch.int32, device=dev)
        if X.stride(1) != 1:
            X = X.contiguous()
        whole = X.to(dev) if n <= step else None

        def blocks():
            for a in range(0, n, step):
                b = min(a + step, n)
                yield (whole if whole is not None else X[a:b].to(dev, non_blocking=False)), ar[:b - a]
        return blocks

    @staticmethod
    def _table_blocks(table: torch.Tensor, rows: torch.Tensor, step: int):
        def blocks():
            for a in range(0, rows.numel(), step):
                yield table, rows[a:a + step]
        return blocks

    # ---- fit ------------------------------------------------------------------------------------------------------
    def _fit_blocks(self, blocks, n: int, d: int, dtype, dev, step: int):
        k = _hip.kernels()
        acc = _hip.acc_dtype(dtype)
        with torch.cuda.device(dev):
            mu = None
            if self.center:
                sums = torch.zeros(d, dtype=torch.float64, device=dev)
                ws = torch.empty(k.column_sums_ws_len(min(step, n), d), dtype=torch.float64, device=dev)
                for i, (table, rows) in enumerate(blocks()):
                    k.column_sums(table, d, rows, ws, sums, accumulate=i > 0)
                mean = (sums.cpu() / n).to(acc)                  # rounded to the accumulate dtype: what the Gram subtracts
                mu = mean.to(dev)
            else:
                mean = torch.zeros(d, dtype=acc)
            G = torch.zeros(d, d, dtype=acc, device=dev)
            ws = torch.empty(k.gram_ws_len(min(step, n), d), dtype=acc, device=dev)
            for i, (table, rows) in enumerate(blocks()):
                k.gram(table, d, rows, mu, ws, G, accumulate=i > 0)
            G_host = G.cpu()
        comp, var, total, rank = principal_axes(G_host, n, self.dim)
        if self.whiten and (var <= 0).any():
            raise ValueError(f"ContentPCA: whiten needs a positive variance in every kept component; component "
                             f"{int(np.argmax(var <= 0))} of {self.dim} has none (numerical rank {rank} of d = {d})")
        self.components_, self.mean_ = comp, mean.double().numpy()
        self.explained_variance_ = var
        self.explained_variance_ratio_ = var / total if total > 0 else np.zeros_like(var)
        self.total_variance_, self.n_samples_ = total, int(n)
        self.fitted_from = "fit"
        return self

    def fit(self, X) -> "ContentPCA":
        X = self._check_matrix(X, "fit")
        n, d = int(X.shape[0]), int(X.shape[1])
        self._check_fit_shape(n, d)
        dev = X.device if X.is_cuda else _hip.require_gpu(self.device)
        return self._fit_blocks(self._matrix_blocks(X, dev), n, d, X.dtype, dev, self._rows_per_block(d, X.dtype))

    def fit_table(self, engine, table: str = "Z", vertices=None) -> "ContentPCA":
        """Fit on the rows of ``vertices`` (default: all) in the engine's current embeddings ("Z") or content ("X"),
        where they lie: nothing is copied."""
        tab, rows = self._engine_rows(engine, table, vertices)
        n, d = int(rows.numel()), int(engine.d)
        self._check_fit_shape(n, d)
        step = self._rows_per_block(d, tab.dtype)
        return self._fit_blocks(self._table_blocks(tab, rows, step), n, d, tab.dtype, engine.device, step)

    @staticmethod
    def _engine_rows(engine, table, vertices):
        from .classify import table_and_rows
        from .train import require_one_gpu
        try:
            require_one_gpu(engine)
        except NotImplementedError:
            raise NotImplementedError(
                f"ContentPCA reads arbitrary rows of the table, which this engine divides over {engine.world} ranks "
                f"(exchange={engine.exchange!r}); several GPUs are out of scope") from None
        if vertices is None:
            vertices = torch.arange(engine.V)
        return table_and_rows(engine, vertices, table)

    # ---- sparse content: the randomized fit ------------------------------------------------------------------------------
    @staticmethod
    def _on(dev):
        return torch.cuda.device(dev) if torch.device(dev).type == "cuda" else contextlib.nullcontext()

    def _orthonormalise(self, k, Y: torch.Tensor, rows: torch.Tensor, what: str) -> torch.Tensor:
        """``Y W^T`` with ``W = Lambda^{-1/2} V^T`` from the float64 ``eigh`` of ``Y^T Y``: orthonormal columns where the
        eigenvalue is above RANK_TOL of the largest, zero columns behind them."""
        m, lp = int(Y.shape[0]), int(Y.shape[1])
        step = default_block_rows(lp, Y.dtype)
        G = torch.zeros(lp, lp, dtype=Y.dtype, device=Y.device)
        ws = torch.empty(k.gram_ws_len(min(step, m), lp), dtype=Y.dtype, device=Y.device)
        for i, a in enumerate(range(0, m, step)):
            k.gram(Y, lp, rows[a:a + step], None, ws, G, accumulate=i > 0)
        lam, vec = torch.linalg.eigh(G.cpu().double())
        lam, vec = torch.flip(lam, [0]), torch.flip(vec, [1])
        keep = lam > RANK_TOL * float(lam[0]) if float(lam[0]) > 0 else torch.zeros_like(lam, dtype=torch.bool)
        r = int(keep.sum())
        if r == 0:
            raise ValueError(f"ContentPCA: the content has no variance left in {what} (numerical rank 0)")
        W = torch.zeros(lp, lp, dtype=torch.float64)
        W[:r] = (vec[:, :r] / lam[:r].sqrt()).T
        Q = torch.empty_like(Y)
        Wd = W.to(Y.dtype).to(Y.device)
        for a in range(0, m, step):
            k.project_affine(Y, lp, rows[a:a + step], None, Wd, Q[a:a + step])
        return Q

    def fit_sparse(self, S, oversample: int = 16, power_iterations: int = 4, seed: int = 0) -> "ContentPCA":
        """Fit on a ``sparse.SparseRows`` [n, D] without densifying it: the randomized range finder with
        ``power_iterations`` rounds on a sketch of ``l = min(dim + oversample, D, n)`` columns, Omega drawn N(0, 1) from
        a CPU generator seeded with ``seed``.  The same seed gives the same bits."""
        from .sparse import SparseRows
        if not isinstance(S, SparseRows):
            raise ValueError(f"ContentPCA.fit_sparse: expected a SparseRows, got {type(S).__name__}")
        for name, v in (("oversample", oversample), ("power_iterations", power_iterations), ("seed", seed)):
            if isinstance(v, bool) or int(v) != v or int(v) < 0:
                raise ValueError(f"ContentPCA.fit_sparse: {name} must be a non-negative integer, got {v!r}")
        n, D = S.shape
        self._check_fit_shape(n, D)
        if self.dim + int(oversample) > MAX_SKETCH:
            raise ValueError(f"ContentPCA.fit_sparse: dim + oversample = {self.dim + int(oversample)} exceeds {MAX_SKETCH}")
        dev = S.device if S.device.type == "cuda" else _hip.require_gpu(self.device)
        k = _hip.kernels()
        l = min(self.dim + int(oversample), D, n)
        lp = -(-l // 4) * 4
        f32, f64 = torch.float32, torch.float64
        with self._on(dev):
            S = S if S.device == dev else S.to(dev)
            St = S.transposed()
            rows_n = torch.arange(n, dtype=torch.int32, device=dev)
            rows_D = torch.arange(D, dtype=torch.int32, device=dev)
            if self.center:
                sums = torch.empty(D, dtype=f64, device=dev)
                k.csr_row_sums(St, sums)
                mean = (sums.cpu() / n).to(f32)                      # rounded to float32: what the products subtract
            else:
                mean = torch.zeros(D, dtype=f32)
            mu64 = mean.double()
            mu = mean.to(dev) if self.center else None
            total = (S.sum_squares() - n * float(mu64 @ mu64)) / (n - 1)
            Omega = torch.zeros(D, lp, dtype=f32)
            Omega[:, :l] = torch.randn(D, l, generator=torch.Generator().manual_seed(int(seed)), dtype=f32)

            def times_S(Z_host_or_dev):                               # S Z - 1 (mu^T Z), Z [D, lp]
                Zd = Z_host_or_dev.to(dev)
                s = (mu64 @ Z_host_or_dev.cpu().double()).to(f32).to(dev) if self.center else None
                Y = torch.empty(n, lp, dtype=f32, device=dev)
                k.csr_spmm(S, Zd, lp, Y, a=None, s=s)
                return Y

            def times_St(Q):                                          # S^T Q - mu (1^T Q), Q [n, lp]
                s = None
                if self.center:
                    cs = torch.empty(lp, dtype=f64, device=dev)
                    cws = torch.empty(k.column_sums_ws_len(n, lp), dtype=f64, device=dev)
                    k.column_sums(Q, lp, rows_n, cws, cs)
                    s = cs.to(f32)
                Z = torch.empty(D, lp, dtype=f32, device=dev)
                k.csr_spmm(St, Q, lp, Z, a=mu, s=s)
                return Z

            Q = self._orthonormalise(k, self._orthonormalise(k, times_S(Omega), rows_n, "S Omega"), rows_n, "S Omega")
            for _ in range(int(power_iterations)):
                Z = times_St(Q)
                Z = self._orthonormalise(k, self._orthonormalise(k, Z, rows_D, "S^T Q"), rows_D, "S^T Q")
                Q = times_S(Z)
                Q = self._orthonormalise(k, self._orthonormalise(k, Q, rows_n, "S Z"), rows_n, "S Z")
            B = times_St(Q).cpu()
        _, sig, Vt = np.linalg.svd(B.double().numpy().T, full_matrices=False)
        lam = sig ** 2
        rank = int((lam > RANK_TOL * lam[0]).sum()) if lam[0] > 0 else 0
        if rank < self.dim:
            raise ValueError(f"ContentPCA: dim = {self.dim} needs a positive variance in every kept component; component "
                             f"{rank} of {self.dim} has none (numerical rank {rank} of D = {D})")
        var = lam[:self.dim] / (n - 1)
        self.components_, self.mean_ = fix_signs(Vt[:self.dim]), mu64.numpy().copy()
        self.explained_variance_ = var.copy()
        self.explained_variance_ratio_ = var / total if total > 0 else np.zeros_like(var)
        self.total_variance_, self.n_samples_ = float(total), int(n)
        self.fitted_from = "fit"
        return self

    def transform_sparse(self, S, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """``(S - 1 mean_^T) components_^T`` (whitened under ``whiten``) for a ``SparseRows``: one CSR product, summed in
        float32 and rounded once to ``dtype``; on ``S``'s device."""
        from .sparse import SparseRows
        if not isinstance(S, SparseRows):
            raise ValueError(f"ContentPCA.transform_sparse: expected a SparseRows, got {type(S).__name__}")
        if self.components_ is None:
            raise ValueError("ContentPCA: fit or load a transform first")
        _hip.acc_dtype(dtype)
        n, D = S.shape
        if D != self.components_.shape[1]:
            raise ValueError(f"ContentPCA.transform_sparse: the transform was fitted on {self.components_.shape[1]} "
                             f"columns, S has {D}")
        if self.dim > MAX_SKETCH:
            raise ValueError(f"ContentPCA.transform_sparse: dim = {self.dim} exceeds {MAX_SKETCH}")
        home = S.device
        if n == 0:
            return torch.empty(0, self.dim, dtype=dtype, device=home)
        dev = home if home.type == "cuda" else _hip.require_gpu(self.device)
        W = torch.from_numpy(np.ascontiguousarray(self.components_, dtype=np.float64))
        if self.whiten:
            var = torch.from_numpy(np.ascontiguousarray(self.explained_variance_, dtype=np.float64))
            if bool((var <= 0).any()):
                raise ValueError("ContentPCA: whiten needs a positive variance in every kept component")
            W = W / var.sqrt()[:, None]
        mp = -(-self.dim // 4) * 4
        Wt = torch.zeros(D, mp, dtype=torch.float32)
        Wt[:, :self.dim] = W.T.to(torch.float32)
        s = None
        if self.center:
            s = torch.zeros(mp, dtype=torch.float32)
            s[:self.dim] = (Wt[:, :self.dim].double().T @ torch.from_numpy(self.mean_)).to(torch.float32)
        k = _hip.kernels()
        with self._on(dev):
            Sd = S if home == dev else S.to(dev)
            out = torch.empty(n, mp, dtype=torch.float32, device=dev)
            k.csr_spmm(Sd, Wt.to(dev), mp, out, a=None, s=None if s is None else s.to(dev))
            Y = out[:, :self.dim].to(dtype).contiguous()
        return Y if home == dev else Y.to(home)

    def fit_transform_sparse(self, S, oversample: int = 16, power_iterations: int = 4, seed: int = 0,
                             dtype: torch.dtype = torch.float32) -> torch.Tensor:
        return self.fit_sparse(S, oversample=oversample, power_iterations=power_iterations,
                               seed=seed).transform_sparse(S, dtype=dtype)

    # ---- transform ------------------------------------------------------------------------------------------------
    def _weights(self, dtype, dev):
        if self.components_ is None:
            raise ValueError("ContentPCA: fit or load a transform first")
        acc = _hip.acc_dtype(dtype)
        W = torch.from_numpy(np.ascontiguousarray(self.components_, dtype=np.float64))
        if self.whiten:
            var = torch.from_numpy(np.ascontiguousarray(self.explained_variance_, dtype=np.float64))
            if bool((var <= 0).any()):
                raise ValueError("ContentPCA: whiten needs a positive variance in every kept component")
            W = W / var.sqrt()[:, None]
        mu = torch.from_numpy(np.ascontiguousarray(self.mean_, dtype=np.float64)).to(acc).to(dev) if self.center else None
        return W.to(acc).contiguous().to(dev), mu

    def _transform_blocks(self, blocks, n: int, d: int, dtype, dev, out: torch.Tensor):
        if d != self.components_.shape[1]:
            raise ValueError(f"ContentPCA.transform: the transform was fitted on {self.components_.shape[1]} columns, "
                             f"X has {d}")
        k = _hip.kernels()
        with torch.cuda.device(dev):
            W, mu = self._weights(dtype, dev)
            a = 0
            for table, rows in blocks():
                b = a + rows.numel()
                if out.is_cuda:
                    k.project_affine(table, d, rows, mu, W, out[a:b])
                else:
                    Y = torch.empty(rows.numel(), self.dim, dtype=dtype, device=dev)
                    k.project_affine(table, d, rows, mu, W, Y)
                    out[a:b] = Y.cpu()
                a = b
        return out

    def transform(self, X) -> torch.Tensor:
        X = self._check_matrix(X, "transform")
        if self.components_ is None:
            raise ValueError("ContentPCA: fit or load a transform first")
        n, d = int(X.shape[0]), int(X.shape[1])
        dev = X.device if X.is_cuda else _hip.require_gpu(self.device)
        out = torch.empty(n, self.dim, dtype=X.dtype, device=dev if X.is_cuda else "cpu")
        if n == 0:
            return out
        return self._transform_blocks(self._matrix_blocks(X, dev), n, d, X.dtype, dev, out)

    def fit_transform(self, X) -> torch.Tensor:
        return self.fit(X).transform(X)

    def transform_table(self, engine, table: str = "Z", vertices=None) -> torch.Tensor:
        """``[len(vertices), dim]`` on the device, in vertex order and the table's dtype."""
        tab, rows = self._engine_rows(engine, table, vertices)
        n, d = int(rows.numel()), int(engine.d)
        out = torch.empty(n, self.dim, dtype=tab.dtype, device=engine.device)
        if n == 0:
            return out
        step = self._rows_per_block(d, tab.dtype)
        return self._transform_blocks(self._table_blocks(tab, rows, step), n, d, tab.dtype, engine.device, out)

    # ---- files ----------------------------------------------------------------------------------------------------
    def save(self, path) -> Path:
        """An ``.npz`` of NPZ_KEYS: the arrays and the flags."""
        if self.components_ is None:
            raise ValueError("ContentPCA.save: nothing is fitted")
        path = Path(path)
        with open(path, "wb") as io:
            np.savez(io, components=self.components_, mean=self.mean_, explained_variance=self.explained_variance_,
                     explained_variance_ratio=self.explained_variance_ratio_,
                     total_variance=np.float64(self.total_variance_), n_samples=np.int64(self.n_samples_),
                     dim=np.int64(self.dim), center=np.bool_(self.center), whiten=np.bool_(self.whiten))
        return path

    @classmethod
    def load(cls, path, block_rows: Optional[int] = None, device=None) -> "ContentPCA":
        with np.load(os.fspath(path)) as z:
            missing = [key for key in NPZ_KEYS if key not in z.files]
            if missing:
                raise ValueError(f"ContentPCA.load: {os.fspath(path)!r} lacks {missing}")
            pca = cls(int(z["dim"]), center=bool(z["center"]), whiten=bool(z["whiten"]), block_rows=block_rows,
                      device=device)
            pca.components_ = np.array(z["components"], dtype=np.float64)
            pca.mean_ = np.array(z["mean"], dtype=np.float64)
            pca.explained_variance_ = np.array(z["explained_variance"], dtype=np.float64)
            pca.explained_variance_ratio_ = np.array(z["explained_variance_ratio"], dtype=np.float64)
            pca.total_variance_, pca.n_samples_ = float(z["total_variance"]), int(z["n_samples"])
        if pca.components_.ndim != 2 or pca.components_.shape[0] != pca.dim or pca.mean_.shape != pca.components_.shape[1:]:
            raise ValueError(f"ContentPCA.load: {os.fspath(path)!r} holds components {pca.components_.shape} and a mean "
                             f"{pca.mean_.shape} for dim = {pca.dim}")
        pca.fitted_from = "load"
        return pca

    def report(self, in_width: int) -> dict:
        """What the CLI writes as ``content_reduction.json``."""
        ratios = [float(r) for r in self.explained_variance_ratio_]
        out = {"input_width": int(in_width), "output_width": self.dim, "n": int(self.n_samples_),
               "explained_variance_ratio": ratios, "explained_variance_ratio_sum": float(sum(ratios)),
               "center": self.center, "whiten": self.whiten, "source": self.fitted_from}
        if self.sparse_fit_ is not None:                     # set by Graph.reduce_sparse_content
            out.update(method="randomized", **self.sparse_fit_)
        return out
