"""The fused column-tile launches of a SweepEngine (csrc/spmm_update.h, the *_tiles_kernel forms): every tile of a pass
in one launch.  ``has_spmm_tiles`` / ``spmm_update_tiles`` / ``spmm_update_class_tiles`` / ``spmm_update_owned_tiles`` are
the kernel backend's optional calls (``KernelBackend`` gives them a body that says no): a backend without them keeps one
launch per tile.  The owned pass's fused launch is owned.bind_launch_tiles."""
from __future__ import annotations


def backend_has(eng, tile_cols: int) -> bool:
    """Whether the backend runs this engine's tables in tiles of `tile_cols` columns with one launch per pass."""
    return bool(eng.k.has_spmm_tiles(eng.dtype, eng.d, tile_cols))


def bind_row(eng, rowptr, nrows: int, row0: int, Zold, Xb, gamma: float, Zn, tile_cols: int, partials, stride: int):
    """The row pass of one block over ALL column tiles (whole tables; tile t's partials at t x stride)."""
    return eng._bind("spmm_update_tiles", rowptr, eng.colidx, eng.P, nrows, row0, Zold, Xb, gamma, Zn, eng.d, tile_cols,
                     eng.long_threshold, partials, stride, sinks_untouched=True, beyond_cache=eng.beyond_cache)


def bind_class(eng, items, row0: int, Zold, Xb, gamma: float, Zn, tile_cols: int, slab, partials, stride: int):
    """Chunk + combine over `items` (a ClassItems) of one block for ALL column tiles: two launches."""
    return eng._bind("spmm_update_class_tiles", eng.colidx, eng.P, items.e0, items.len, items.slot, items.items_per_block,
                     items.rows, items.slot_ptr, int(items.slot_ptr[-1]), row0, Zold, Xb, gamma, Zn, eng.d, tile_cols,
                     slab, partials, stride, beyond_cache=eng.beyond_cache)
