"""One weight per row instead of one per edge (SweepEngine(uniform_weights=...), the spmm_update*_rw calls) -- helpers of
tests/test_gpu_uniform_weights.py (the HIP kernels) and tests/test_uniform_weights_host.py (the engine's logic through
the CPU double below).

The graph: 1 300 vertices; the first 320 rows have out-degrees 0, 1, 3, 4, 5, 31, 32, 33, 64, 65, 200, 513, 600 and 1 100
(each twice) among a ragged remainder of at most 12 edges, the rest are rows without edges.  `SETTINGS` lowers the
engine's thresholds so that one sweep runs the row pass (rows of at most 32 edges), the owned pass (33 .. 550 edges: whole
rows up to 128 edges, virtual rows above) and chunk + combine (600 and 1 100 edges).  Data are Gaussian: nothing here is
compared with a reference, only the per-row-weight run with the per-edge run of the SAME engine, bit for bit -- Z_new,
every delta partial, the delta.
"""
import functools

import numpy as np
import torch

from clane_amd.engine import SweepEngine
from clane_amd.partition import HostCSR
from clane_amd.plan import lanes_per_row

from .fused_tiles_oracle_kernels import OracleKernels as _TilesDouble

V = 1300
ROWS_WITH_EDGES = 320
DEGREES = (0, 1, 3, 4, 5, 31, 32, 33, 64, 65, 200, 513, 600, 1100)
GAMMA = 0.7
# (d, column tiles): a sub-wave per row at 66 columns (17 packs: 32 lanes), a wave per row at 130 (33 packs), 128 columns
# untiled and 256 in two tiles of 128
WIDTHS = [(66, 1), (128, 1), (130, 1), (256, 2)]
OWNED_SUMS = 12


def settings(d, tiles, chunks=1, **more):
    width = d // tiles
    out = dict(class_threshold=32, class_chunk=64, class_phases=1, class_owned=True, owned_groups=8,
               owned_block_threads=256, owned_row_edges=128, owned_max_edges=550,
               owned_lds_bytes=OWNED_SUMS * 16 * lanes_per_row(width, torch.float32), column_tiles=tiles)
    if chunks > 1:
        out.update(chunks=chunks)
    out.update(more)
    return out


@functools.lru_cache(maxsize=None)
def graph():
    """(rowptr, colidx, deg): columns distinct and sorted within a row."""
    rng = np.random.default_rng(77)
    deg = np.zeros(V, dtype=np.int64)
    deg[:ROWS_WITH_EDGES] = rng.integers(0, 13, size=ROWS_WITH_EDGES)
    where = rng.permutation(ROWS_WITH_EDGES)[:2 * len(DEGREES)]
    deg[where] = np.tile(np.array(DEGREES), 2)
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    colidx = np.concatenate([np.sort(rng.choice(V, size=int(k), replace=False)) for k in deg]).astype(np.int32)
    assert set(DEGREES) <= set(deg.tolist())
    return rowptr, colidx, deg


@functools.lru_cache(maxsize=None)
def tables(d):
    g = torch.Generator().manual_seed(500 + d)
    return torch.randn(V, d, generator=g), torch.randn(V, d, generator=g)         # X, Z0


def row_of_edge():
    return np.repeat(np.arange(V), graph()[2])


def P_one_over_deg():
    """What build_P leaves in reference mode at scale: 1 / deg on every edge, in the sorted edge order."""
    deg = graph()[2]
    return torch.from_numpy((np.float32(1.0) / deg[row_of_edge()].astype(np.float32)))


def P_any_float_per_row(seed=5):
    """One arbitrary float per row (negative ones, a zero row, a subnormal, a huge one): uniform all the same."""
    w = torch.randn(V, generator=torch.Generator().manual_seed(seed))
    rows = np.nonzero(graph()[2] > 0)[0]
    w[rows[0]], w[rows[1]], w[rows[2]] = 0.0, 1e-41, 3e30
    return w[torch.from_numpy(row_of_edge())]


def one_ulp_off(P, row=None):
    """P with one edge (the last of the longest row, or of `row`) moved by one unit in the last place."""
    rowptr, _, deg = graph()
    r = int(np.argmax(deg)) if row is None else row
    out = P.clone()
    e = int(rowptr[r + 1]) - 1
    out[e] = torch.nextafter(out[e], torch.tensor(float("inf")))
    assert out[e] != P[e]
    return out


def load_P(eng, P_sorted):
    """P in the sorted edge order into the engine's own; P_valid last, as everything that writes P sets it."""
    eng.P[:eng.E_loc] = P_sorted[torch.from_numpy(eng.local.edge_origin)].to(eng.acc_dtype).to(eng.device)
    eng.P_valid = True


def make_engine(kernels, dev, d, tiles, P_sorted, uniform_weights="auto", beyond=None, **more):
    rowptr, colidx, _ = graph()
    X, Z0 = tables(d)
    eng = SweepEngine(HostCSR(V, rowptr, colidx), X, dev, kernels, uniform_weights=uniform_weights,
                      **settings(d, tiles, **more))
    if beyond is not None:
        eng.beyond_cache = bool(beyond)            # the cache hint of every K3 call (plans are bound at the first sweep)
    eng.set_Z(Z0)
    load_P(eng, P_sorted)
    return eng


def assert_every_pass_runs(eng):
    """The row pass, the owned pass with whole and virtual rows, chunk + combine beside it -- in every launch block when
    there is one, in some block when there are three."""
    owned = [r.owned for r in eng.block_rows if r.owned is not None]
    assert owned and any(o.rest is not None for o in owned) and eng.long_threshold == 32
    assert all(x is None for x in eng.mid_rows + eng.hub_rows + eng.split_rows)


def sweep_from_start(eng, d, P_sorted, mode):
    """One sweep from (Z0, P) under `mode`: (Z_new, every delta partial, the delta, the calls the sweep bound)."""
    eng.set_uniform_weights(mode)
    eng.set_Z(tables(d)[1])
    load_P(eng, P_sorted)
    bound = []
    bind = eng._bind

    def recording(method, *a, **kw):
        bound.append(method)
        return bind(method, *a, **kw)

    eng._bind = recording
    eng._plans = {}
    try:
        delta = eng.sweep(GAMMA)
    finally:
        del eng._bind
    return eng.Zcur.clone(), eng.partials.clone(), delta, bound


def k3_calls(bound):
    return sorted({m for m in bound if m.startswith("spmm_update")})


def rw_calls(tiles, fused=True):
    t = "_tiles" if tiles > 1 and fused else ""
    return sorted([f"spmm_update{t}_rw", f"spmm_update_class{t}_rw", f"spmm_update_owned{t}_rw"])


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


def numpy_row_weights(P_engine_order, rowptr):
    """The mirror of row_weight_kernel: (w, mixed) from P in the ENGINE's edge order and its rowptr, bit patterns compared."""
    P = np.ascontiguousarray(P_engine_order)
    bits = P.view(np.uint32 if P.dtype == np.float32 else np.uint64)
    n = rowptr.size - 1
    w = np.zeros(n, dtype=P.dtype)
    mixed = 0
    for r in range(n):
        a, b = int(rowptr[r]), int(rowptr[r + 1])
        if b > a:
            w[r] = P[a]
            mixed |= int((bits[a:b] != bits[a]).any())
    return w, mixed


# ---- the CPU double ----------------------------------------------------------------------------------------------------
class UniformOracleKernels(_TilesDouble):
    """tests/fused_tiles_oracle_kernels.py with row_weight and the *_rw calls.  A *_rw call checks what the engine hands
    it -- the weights row_weight last wrote, cut at the block's first row, of a P whose rows were uniform -- and then makes
    the per-edge call on the P those weights were taken from: what include/clane_hip.h says the *_rw calls compute."""

    def __init__(self):
        super().__init__()
        self.scans = 0

    def has_row_weight(self, dtype):
        return dtype == torch.float32

    def row_weight(self, rowptr, P, nrows, w, mixed):
        got, m = numpy_row_weights(P.numpy(), rowptr.numpy()[:nrows + 1])
        w[:nrows] = torch.from_numpy(got)
        mixed[0] = m
        self.scans += 1
        self._seen = (w, P, m)

    def _P_of(self, row_weight):
        w, P, mixed = self._seen
        assert mixed == 0, "a *_rw call on a P with a mixed row"
        off = (row_weight.data_ptr() - w.data_ptr()) // w.element_size()
        assert 0 <= off < max(w.numel(), 1) and row_weight.numel() == w.numel() - off, "not the engine's row weights"
        return P

    def spmm_update_rw(self, rowptr, colidx, row_weight, *a, **kw):
        return self.spmm_update(rowptr, colidx, self._P_of(row_weight), *a, **kw)

    def spmm_update_tiles_rw(self, rowptr, colidx, row_weight, *a, **kw):
        return self.spmm_update_tiles(rowptr, colidx, self._P_of(row_weight), *a, **kw)

    def spmm_update_class_rw(self, colidx, row_weight, item_e0, item_len, item_slot, item_row, *a, **kw):
        assert item_row.numel() == item_e0.numel()
        return self.spmm_update_class(colidx, self._P_of(row_weight), item_e0, item_len, item_slot, *a, **kw)

    def spmm_update_class_tiles_rw(self, colidx, row_weight, item_e0, item_len, item_slot, item_row, *a, **kw):
        assert item_row.numel() == item_e0.numel()
        return self.spmm_update_class_tiles(colidx, self._P_of(row_weight), item_e0, item_len, item_slot, *a, **kw)

    def spmm_update_owned_rw(self, colidx, row_weight, *a, **kw):
        return self.spmm_update_owned(colidx, self._P_of(row_weight), *a, **kw)

    def spmm_update_owned_tiles_rw(self, colidx, row_weight, *a, **kw):
        return self.spmm_update_owned_tiles(colidx, self._P_of(row_weight), *a, **kw)


def segment_rows_by_search(plan):
    """Every owned segment's row, the slow way: the batch of the segment, the row of that batch whose virtual rows hold
    the segment's.  What _hip.OwnedPlan.seg_row must equal."""
    S = int(plan["n_steps"])
    bs, bv, br = plan["bat_seg_ptr"], plan["bat_vrow_ptr"], plan["bat_row_ptr"]
    out = np.zeros(plan["seg_e0"].size, dtype=np.int32)
    for b in range(bv.size - 1):
        for k in range(int(bs[b * S]), int(bs[(b + 1) * S])):
            v = int(bv[b]) + int(plan["seg_vrow"][k])
            j = next(j for j in range(int(br[b]), int(br[b + 1]))
                     if int(plan["row_vptr"][j]) <= v < int(plan["row_vptr"][j + 1]))
            out[k] = plan["row_id"][j]
    return out

