"""Sparse content -- a validated CSR matrix of float32 values, what ``ContentPCA.fit_sparse`` and the kernels of
csrc/sparse_rows.h take.

A bag of words is read from the layout ``scipy.sparse.save_npz`` writes (keys ``data``, ``indices``, ``indptr``,
``shape``, ``format``) with numpy alone: the package does not depend on scipy.  Everything is checked on the host before
anything reaches the device -- the kernels trust the column indices.
"""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np
import torch

SEGMENT = 2048                      # CLANE_CSR_SEGMENT: the non-zeros of one work item of a long row
INDEX_LIMIT = 1 << 31
NPZ_KEYS = ("data", "indices", "indptr", "shape", "format")


def segment_items(rowptr: torch.Tensor, segment: int = SEGMENT):
    """(long_rows int32, seg_ptr int64, item_long int32) of a CSR's rows of more than ``segment`` non-zeros: the rows
    ascending, the prefix sums of their segment counts, and for every segment the index of its row in ``long_rows``."""
    lens = rowptr[1:] - rowptr[:-1]
    long_rows = torch.nonzero(lens > segment).flatten()
    nseg = (lens[long_rows] + (segment - 1)) // segment
    seg_ptr = torch.zeros(long_rows.numel() + 1, dtype=torch.int64, device=rowptr.device)
    seg_ptr[1:] = torch.cumsum(nseg, 0)
    item_long = torch.repeat_interleave(torch.arange(long_rows.numel(), dtype=torch.int32, device=rowptr.device), nseg)
    return long_rows.to(torch.int32), seg_ptr, item_long.contiguous()


class SparseRows:
    """CSR: ``rowptr`` int64 [n + 1], ``col`` int32 [nnz], ``val`` float32 [nnz], ``shape`` (n, D).  Inside a row the
    columns ascend and are unique (duplicates are summed on construction).  Raises ``ValueError`` for a non-monotone
    ``rowptr``, a column outside ``[0, D)``, a non-finite value, or ``n`` / ``D`` of 2^31 or more."""

    def __init__(self, rowptr, col, val, shape, _trusted: bool = False):
        if _trusted:
            self.rowptr, self.col, self.val, self.shape = rowptr, col, val, (int(shape[0]), int(shape[1]))
        else:
            self.rowptr, self.col, self.val, self.shape = self._validated(rowptr, col, val, shape)
        self._segments = None

    # ---- checks -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _validated(rowptr, col, val, shape):
        shape = tuple(int(x) for x in np.asarray(shape).reshape(-1))
        if len(shape) != 2 or min(shape) < 0:
            raise ValueError(f"SparseRows: shape must be (n, D), got {shape}")
        n, D = shape
        if n >= INDEX_LIMIT or D >= INDEX_LIMIT:
            raise ValueError(f"SparseRows: n = {n} and D = {D} must be below 2^31")
        rowptr = np.ascontiguousarray(np.asarray(rowptr).reshape(-1))
        col = np.ascontiguousarray(np.asarray(col).reshape(-1))
        val = np.asarray(val).reshape(-1)
        if rowptr.dtype.kind not in "iu" or col.dtype.kind not in "iu":
            raise ValueError("SparseRows: indptr and indices must be integers")
        if val.dtype.kind not in "fiu":
            raise ValueError(f"SparseRows: values must be real numbers, got {val.dtype}")
        rowptr = rowptr.astype(np.int64)
        if rowptr.shape[0] != n + 1 or rowptr[0] != 0 or int(rowptr[-1]) != col.shape[0] or val.shape[0] != col.shape[0]:
            raise ValueError(f"SparseRows: indptr must hold n + 1 = {n + 1} entries from 0 to nnz = {col.shape[0]}, "
                             f"and data one value per index")
        if (np.diff(rowptr) < 0).any():
            raise ValueError("SparseRows: indptr is not monotone")
        if col.shape[0] and (int(col.min()) < 0 or int(col.max()) >= D):
            raise ValueError(f"SparseRows: indices holds columns outside [0, {D})")
        val = val.astype(np.float32)
        if not np.isfinite(val).all():
            raise ValueError("SparseRows: data holds non-finite values")
        col = col.astype(np.int64)
        row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
        key = row * max(D, 1) + col
        if key.shape[0] and (np.diff(key) <= 0).any():            # unsorted or duplicated: sort (stable), sum duplicates
            order = np.argsort(key, kind="stable")
            key, val = key[order], val[order]
            first = np.ones(key.shape[0], dtype=bool)
            first[1:] = key[1:] != key[:-1]
            start = np.flatnonzero(first)
            val = np.add.reduceat(val.astype(np.float64), start).astype(np.float32)
            if not np.isfinite(val).all():
                raise ValueError("SparseRows: summing duplicate entries overflowed float32")
            key = key[start]
            row, col = key // max(D, 1), key % max(D, 1)
            rowptr = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(np.bincount(row, minlength=n), out=rowptr[1:])
        return (torch.from_numpy(rowptr), torch.from_numpy(col.astype(np.int32)), torch.from_numpy(val), (n, D))

    # ---- shape ------------------------------------------------------------------------------------------------------
    @property
    def nnz(self) -> int:
        return int(self.col.numel())

    @property
    def device(self):
        return self.val.device

    def __len__(self) -> int:
        return self.shape[0]

    # ---- files ------------------------------------------------------------------------------------------------------
    @classmethod
    def load_npz(cls, path) -> "SparseRows":
        """Read what ``scipy.sparse.save_npz`` writes for a CSR matrix (numpy alone, ``allow_pickle=False``)."""
        with np.load(os.fspath(path), allow_pickle=False) as z:
            missing = [key for key in NPZ_KEYS if key not in z.files]
            if missing:
                raise ValueError(f"SparseRows.load_npz: {os.fspath(path)!r} lacks {missing}")
            fmt = z["format"]
            fmt = fmt.item() if fmt.shape == () else fmt
            fmt = fmt.decode() if isinstance(fmt, bytes) else str(fmt)
            if fmt != "csr":
                raise ValueError(f"SparseRows.load_npz: {os.fspath(path)!r} holds format {fmt!r}; only 'csr' is read")
            return cls(z["indptr"], z["indices"], z["data"], z["shape"])

    def save_npz(self, path) -> Path:
        path = Path(path)
        with open(path, "wb") as io:
            np.savez(io, data=self.val.cpu().numpy(), indices=self.col.cpu().numpy(), indptr=self.rowptr.cpu().numpy(),
                     shape=np.asarray(self.shape, dtype=np.int64), format=np.asarray(b"csr"))
        return path

    @classmethod
    def from_dense(cls, X) -> "SparseRows":
        X = np.asarray(torch.as_tensor(X).cpu() if isinstance(X, torch.Tensor) else X)
        if X.ndim != 2:
            raise ValueError(f"SparseRows.from_dense: expected a 2-D matrix, got shape {X.shape}")
        r, c = np.nonzero(X)
        rowptr = np.zeros(X.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(r, minlength=X.shape[0]), out=rowptr[1:])
        return cls(rowptr, c, X[r, c], X.shape)

    def to_dense(self, dtype=torch.float32) -> torch.Tensor:
        n, D = self.shape
        out = torch.zeros(n, D, dtype=dtype, device=self.device)
        rowptr = self.rowptr - self.rowptr[0]
        row = torch.repeat_interleave(torch.arange(n, device=self.device), rowptr[1:] - rowptr[:-1])
        e0 = int(self.rowptr[0])
        sl = slice(e0, e0 + row.numel())
        out[row, self.col[sl].long()] = self.val[sl].to(dtype)
        return out

    # ---- device -----------------------------------------------------------------------------------------------------
    def to(self, device) -> "SparseRows":
        return SparseRows(self.rowptr.to(device), self.col.to(device), self.val.to(device), self.shape, _trusted=True)

    def segments(self):
        """The long rows' segment list (``segment_items``), made once where the matrix lies."""
        if self._segments is None:
            self._segments = segment_items(self.rowptr, SEGMENT)
        return self._segments

    def rows(self, a: int, b: int) -> "SparseRows":
        """Rows [a, b) as a matrix of its own that shares ``col`` / ``val``: only the row pointers are sliced."""
        if not 0 <= a <= b <= self.shape[0]:
            raise ValueError(f"SparseRows.rows: [{a}, {b}) is not a range of {self.shape[0]} rows")
        return SparseRows(self.rowptr[a:b + 1], self.col, self.val, (b - a, self.shape[1]), _trusted=True)

    def transposed(self) -> "SparseRows":
        """The transpose, built where the matrix lies: a STABLE sort of the column keys, so every row of the transpose
        lists the original rows in ascending order."""
        n, D = self.shape
        dev = self.device
        rowptr = self.rowptr - self.rowptr[0]
        e0 = int(self.rowptr[0])
        nnz = int(rowptr[-1])
        col, val = self.col[e0:e0 + nnz], self.val[e0:e0 + nnz]
        row = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev), rowptr[1:] - rowptr[:-1])
        order = torch.sort(col, stable=True).indices
        t_rowptr = torch.zeros(D + 1, dtype=torch.int64, device=dev)
        if nnz:
            t_rowptr[1:] = torch.cumsum(torch.bincount(col.long(), minlength=D), 0)
        return SparseRows(t_rowptr, row[order].contiguous(), val[order].contiguous(), (D, n), _trusted=True)

    def sum_squares(self) -> float:
        """The sum of the squared values, float64."""
        return float((self.val.double() ** 2).sum())
