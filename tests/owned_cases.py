"""Shared by tests/test_owned_plan_host.py and tests/test_owned_class_pass_gpu.py: one small graph that holds every row
shape the owned class pass (csrc/spmm_update.h spmm_owned_kernel, xcd.owned_plan) treats differently, integer and
Gaussian data over it with references computed once, and the engine settings that force each path.  Nobody writes to
what this module returns."""
import functools

import numpy as np
import torch

from clane_amd.engine import SweepEngine
from clane_amd.partition import HostCSR
from clane_amd.xcd import xcd_class
from oracle import clane_oracle as O

from .engine_exact_cases import load_P

V = 1536
CHUNK = 64                      # class_chunk and the owned pieces
ROW_EDGES = 128                 # owned_row_edges: rows above it are summed as virtual rows
WIDTHS = [(128, 1), (256, 2), (136, 1)]        # (d, column tiles): 512-byte rows, two tiles of them, ragged 1-KiB rows

# degrees of the first rows, by what they are there for
ALL_CLASSES = [65, 100, 150, 200, 257, 300]     # rows of 65..300 edges touching all 8 classes
EMPTY_CLASS_ROW, EMPTY_CLASS = 6, 3             # 120 edges, none into class 3
EXACT = {7: 96, 8: 97, 9: 160, 10: 161, 12: ROW_EDGES, 13: ROW_EDGES + 1}     # H and H + 1 for H = 96 and 160; one / two virtual rows
ONE_CLASS_ROW, ONE_CLASS = 11, 5                # 150 edges of one class: a segment of several pieces
N_CLASS_ROWS = 44                               # rows 14..43: 65..160 edges, more rows than a small batch holds
N_SHORT = 700                                   # rows 44..743: 1..64 edges; the rest are sinks

# engine settings: (owned_max_edges, class_phases, phase_threshold)
SETTINGS = {"H96": (96, None, 512),             # rows of 65..96 edges owned, 97 and up by chunk + combine
            "H160": (160, None, 512),           # rows up to 160 owned, among them virtual rows and the one-class row
            "all_phased": (4096, 2, 200)}       # every class row owned; rows above 200 edges in 2 phases = 16 steps


@functools.lru_cache(maxsize=None)
def graph():
    """(rowptr, colidx) int64, rows sorted and unique.  Table positions are vertex ids (hot_rows_first=False)."""
    rng = np.random.default_rng(7)
    cls = xcd_class(np.arange(V))
    rows = []
    for r in range(V):
        if r < len(ALL_CLASSES):
            cols = rng.choice(V, ALL_CLASSES[r], replace=False)
            assert np.unique(cls[cols]).size == 8
        elif r == EMPTY_CLASS_ROW:
            cols = rng.choice(np.nonzero(cls != EMPTY_CLASS)[0], 120, replace=False)
        elif r in EXACT:
            cols = rng.choice(V, EXACT[r], replace=False)
        elif r == ONE_CLASS_ROW:
            cols = rng.choice(np.nonzero(cls == ONE_CLASS)[0], 150, replace=False)
        elif r < N_CLASS_ROWS:
            cols = rng.choice(V, int(rng.integers(65, 161)), replace=False)
        elif r < N_CLASS_ROWS + N_SHORT:
            cols = rng.choice(V, 64 if r == N_CLASS_ROWS else int(rng.integers(1, 65)), replace=False)
        else:
            cols = np.empty(0, dtype=np.int64)
        rows.append(np.sort(cols))
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum([c.size for c in rows], out=rowptr[1:])
    return rowptr, np.concatenate(rows).astype(np.int64)


def csr():
    rowptr, colidx = graph()
    return HostCSR(V, rowptr, colidx.astype(np.int32))


@functools.lru_cache(maxsize=None)
def integer_case(d):
    """X, Z0 in -4..4, P in 1..3 (sorted edge order), gamma = 1: every sum is an integer below 2^13.  Returns float32
    X, Z0, P and the int64 reference of one sweep with its delta."""
    rowptr, colidx = graph()
    rng = np.random.default_rng(100 + d)
    X = rng.integers(-4, 5, (V, d))
    Z0 = rng.integers(-4, 5, (V, d))
    P = rng.integers(1, 4, colidx.size)
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
    g = torch.Generator().manual_seed(200 + d)
    X, Z0 = torch.randn(V, d, generator=g), torch.randn(V, d, generator=g)
    P = torch.rand(colidx.size, generator=g) + 0.1
    deg = np.diff(rowptr)
    P = P / torch.from_numpy(np.repeat(np.add.reduceat(P.numpy(), rowptr[:-1][deg > 0]), deg[deg > 0]))
    Z1, delta = O.sweep(rowptr, colidx, P.double(), X.double(), Z0.double(), gamma)
    return X, Z0, P, Z1, float(delta), gamma


BATCH_VROWS = 4                 # LDS sums per batch: every group of 8 then needs several batches


def sum_bytes(d, tiles):
    """One LDS sum: a whole row of the lane layout, 32 or 64 lanes of 16 bytes."""
    return 512 if d // tiles <= 128 else 1024


def make_engine(kernels, dev, d, tiles, setting, X, Z0, P, class_owned=True, **more):
    H, phases, pt = SETTINGS[setting]
    kw = dict(class_threshold=64, class_chunk=CHUNK, class_phases=phases, phase_threshold=pt, column_tiles=tiles,
              hot_rows_first=False, class_owned=class_owned, owned_max_edges=H, owned_row_edges=ROW_EDGES,
              owned_groups=8, owned_lds_bytes=BATCH_VROWS * sum_bytes(d, tiles), owned_block_threads=256)
    kw.update(more)
    eng = SweepEngine(csr(), X, dev, kernels, **kw)
    assert torch.equal(eng.pos.cpu(), torch.arange(V))          # the classes graph() chose its columns by
    eng.set_Z(Z0)
    load_P(eng, P)
    return eng
