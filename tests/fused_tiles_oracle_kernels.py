"""The CPU test double with the fused column-tile calls (``spmm_update_tiles`` / ``_class_tiles`` / ``_owned_tiles``):
each loops over the per-tile method of tests/owned_oracle_kernels.py on views of the whole tables, which is what
include/clane_hip.h says the fused launches compute.  It also records the name of every call an engine binds, so a
test can read a sweep's plan.  Like its bases it is only ever handed to an engine by a test."""
import torch

from clane_amd.plan import lanes_per_row

from .owned_oracle_kernels import OracleKernels as _Base


class OracleKernels(_Base):
    def __init__(self):
        super().__init__()
        self.bound = []                 # method names, in the order SweepEngine._build_plan bound them

    def bind(self, method, *args, **kwargs):
        self.bound.append(method)
        return super().bind(method, *args, **kwargs)

    def has_spmm_tiles(self, dtype, d, tile_cols):
        if dtype != torch.float32 or not 0 < tile_cols <= d or tile_cols % 4:
            return False
        last = d - (-(-d // tile_cols) - 1) * tile_cols
        return lanes_per_row(last, dtype) == lanes_per_row(tile_cols, dtype)

    @staticmethod
    def _cuts(d, tile_cols):
        return [(c, min(d, c + tile_cols)) for c in range(0, d, tile_cols)]

    def spmm_update_tiles(self, rowptr, colidx, P, nrows, row0, Z_old, X, gamma, Z_new, d, tile_cols, long_threshold,
                          partials, partials_stride, sinks_untouched=False, beyond_cache=False):
        assert self.has_spmm_tiles(Z_old.dtype, d, tile_cols)
        for t, (c0, c1) in enumerate(self._cuts(d, tile_cols)):
            self.spmm_update(rowptr, colidx, P, nrows, row0, Z_old[:, c0:c1], X[:, c0:c1], gamma, Z_new[:, c0:c1], c1 - c0,
                             long_threshold, partials[t * partials_stride:], sinks_untouched=sinks_untouched,
                             beyond_cache=beyond_cache)

    def spmm_update_class_tiles(self, colidx, P, item_e0, item_len, item_slot, items_per_block, class_rows, slot_ptr,
                                n_slots, row0, Z_old, X, gamma, Z_new, d, tile_cols, slab, partials, partials_stride,
                                beyond_cache=False):
        assert self.has_spmm_tiles(Z_old.dtype, d, tile_cols) and n_slots == int(slot_ptr[-1])
        per_tile = self.spmm_class_slab_len(n_slots, tile_cols)
        cuts = self._cuts(d, tile_cols)
        assert slab.numel() >= len(cuts) * per_tile, "the slab holds every tile's chunk sums at the same time"
        for t, (c0, c1) in enumerate(cuts):
            self.spmm_update_class(colidx, P, item_e0, item_len, item_slot, items_per_block, class_rows, slot_ptr, row0,
                                   Z_old[:, c0:c1], X[:, c0:c1], gamma, Z_new[:, c0:c1], c1 - c0,
                                   slab[t * per_tile:(t + 1) * per_tile], partials[t * partials_stride:],
                                   beyond_cache=beyond_cache)

    def spmm_update_owned_tiles(self, colidx, P, plan, block_threads, row0, Z_old, X, gamma, Z_new, d, tile_cols, partials,
                                partials_stride, beyond_cache=False, loads=0, ahead=False):
        assert self.has_spmm_tiles(Z_old.dtype, d, tile_cols)
        for t, (c0, c1) in enumerate(self._cuts(d, tile_cols)):
            self.spmm_update_owned(colidx, P, plan, block_threads, row0, Z_old[:, c0:c1], X[:, c0:c1], gamma,
                                   Z_new[:, c0:c1], c1 - c0, partials[t * partials_stride:], beyond_cache=beyond_cache,
                                   loads=loads)
