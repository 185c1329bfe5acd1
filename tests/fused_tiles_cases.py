"""Shared by tests/test_fused_tiles_host.py and tests/test_gpu_fused_tiles.py: one graph of 3072 rows that holds every row
shape the K3 passes treat differently, integer and Gaussian data over it with references computed once, and the engine
that routes the rows to the row pass, the owned pass and chunk + combine.  Nobody writes to what this module returns."""
import functools

import numpy as np
import torch

from clane_amd.engine import SweepEngine
from clane_amd.partition import HostCSR
from oracle import clane_oracle as O

from .engine_exact_cases import load_P

V = 3072
CHUNK = 64                          # class_chunk and the owned pieces
OWNED_MAX = 512                     # rows of 65..512 edges are owned, rows above go through chunk + combine
PHASE_THRESHOLD = 1024              # the 5 000-edge row is phased: 2 phases x 8 classes
HEAVY = 5000
# the degrees the issue names, by the pass that takes them
ROW_PASS = [0, 1, 3, 4, 5, 63, 64]
OWNED = [65, 200, 512]
CHUNKED = [513, 900, HEAVY]
# (d, tile_cols): two tiles of 128, three tiles, a last tile of 72 columns, and a ragged last pack (70 columns, 2 pads)
WIDTHS = [(256, 128), (384, 128), (200, 128), (198, 128)]


@functools.lru_cache(maxsize=None)
def graph():
    """(rowptr, colidx) int64.  The first rows carry the named degrees, 60 more class rows of 65..700 edges follow, then
    2 000 rows of 0..64 edges; the rest are sinks.  The heavy row draws its columns with replacement (5 000 > V)."""
    rng = np.random.default_rng(16)
    named = ROW_PASS + OWNED + CHUNKED
    rows = []
    for r in range(V):
        if r < len(named):
            n = named[r]
        elif r < len(named) + 60:
            n = int(rng.integers(65, 701))
        elif r < len(named) + 60 + 2000:
            n = int(rng.integers(0, 65))
        else:
            n = 0
        cols = rng.integers(0, V, n) if n > V else rng.choice(V, n, replace=False)
        rows.append(np.sort(cols))
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum([c.size for c in rows], out=rowptr[1:])
    return rowptr, np.concatenate(rows).astype(np.int64)


def csr():
    rowptr, colidx = graph()
    return HostCSR(V, rowptr, colidx.astype(np.int32))


@functools.lru_cache(maxsize=None)
def integer_case(d, sweeps=1):
    """X, Z0 in -2..2, P in 1..2 (sorted edge order), gamma = 1: after `sweeps` sweeps every value stays an integer that
    fp32 holds exactly for one sweep (|z| <= 2 + 5 000 x 4).  float32 X, Z0, P and the int64 reference with its delta."""
    rowptr, colidx = graph()
    rng = np.random.default_rng(300 + d)
    X = rng.integers(-2, 3, (V, d))
    Z0 = rng.integers(-2, 3, (V, d))
    P = rng.integers(1, 3, colidx.size)
    Z1 = Z0.copy()
    for r in range(V):
        a, b = rowptr[r], rowptr[r + 1]
        if b > a:
            Z1[r] = X[r] + (P[a:b, None] * Z0[colidx[a:b]]).sum(0)
    delta = int(np.abs(Z1 - Z0).sum())
    f = lambda a: torch.from_numpy(a.astype(np.float32))       # noqa: E731
    return f(X), f(Z0), f(P), f(Z1), delta


@functools.lru_cache(maxsize=None)
def gaussian_case(d, gamma=0.7):
    """Gaussian X, Z0, positive P with rows summing to one; the oracle's sweep in double."""
    rowptr, colidx = graph()
    g = torch.Generator().manual_seed(400 + d)
    X, Z0 = torch.randn(V, d, generator=g), torch.randn(V, d, generator=g)
    P = torch.rand(colidx.size, generator=g) + 0.1
    deg = np.diff(rowptr)
    P = P / torch.from_numpy(np.repeat(np.add.reduceat(P.numpy(), rowptr[:-1][deg > 0]), deg[deg > 0]))
    Z1, delta = O.sweep(rowptr, colidx, P.double(), X.double(), Z0.double(), gamma)
    return X, Z0, P, Z1, float(delta), gamma


def tiles_for(d, tile_cols):
    """column_tiles that makes SweepEngine cut d into tiles of tile_cols columns where it can (its cuts are even): the
    engine-level runs use the cuts the engine makes, the backend-level ones cut by hand."""
    return -(-d // tile_cols)


def make_engine(kernels, dev, d, tiles, X, Z0, P, **more):
    """Rows up to 64 edges by the row pass, 65..512 owned, above by chunk + combine (the heavy row in 2 phases)."""
    kw = dict(class_threshold=64, class_chunk=CHUNK, class_phases=2, phase_threshold=PHASE_THRESHOLD, column_tiles=tiles,
              hot_rows_first=False, class_owned=True, owned_max_edges=OWNED_MAX, owned_row_edges=256, owned_groups=8,
              owned_lds_bytes=16 * 1024, owned_block_threads=256)
    kw.update(more)
    eng = SweepEngine(csr(), X, dev, kernels, **kw)
    eng.set_Z(Z0)
    load_P(eng, P)
    return eng


def tile_cuts(d, tile_cols):
    return [(c, min(d, c + tile_cols)) for c in range(0, d, tile_cols)]
