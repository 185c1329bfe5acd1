"""Content reduction -- PCA of a wide ``[n, d]`` matrix (the bag-of-words ``C.npy`` of an attributed network) on the GPU.

Nothing in the reference does this: its users run a host PCA before the graph is loaded.  Here the three passes over the
data are HIP kernels (csrc/content_pca.h): deterministic column sums, the centred Gram ``Xc^T Xc`` on the matrix cores and
the affine projection ``W (x - mu)``.  The ``d x d`` eigen-problem in between is plumbing: ``torch.linalg.eigh`` in
float64 on the host.

Every sum runs in a fixed order, and a matrix that is streamed in blocks gives the bits of one call: a fit is
reproducible bit for bit, whatever ``block_rows``.

There is no CPU fallback: without the library or a GPU, ``fit`` and ``transform`` raise ``ClaneHipError``.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _hip

CHUNK_ROWS = 2048                   # kGradChunk: the rows of one partial sum
BLOCK_BYTE_BUDGET = 1 << 30         # a block of X on the device plus the Gram's workspace for it
MAX_CHUNKS = 65535                  # chunks of one launch

SECTION_KEYS = ("dim", "center", "whiten", "load")
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
    return out


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
        return {"input_width": int(in_width), "output_width": self.dim, "n": int(self.n_samples_),
                "explained_variance_ratio": ratios, "explained_variance_ratio_sum": float(sum(ratios)),
                "center": self.center, "whiten": self.whiten, "source": self.fitted_from}
