"""The tables one K3 call of a SweepEngine is bound on, and the binders of the passes that have a fused form
(csrc/spmm_update.h, the *_tiles_kernel forms: every column tile of a pass in one launch).  A call is bound either on one
tile's cut of the tables or -- fused -- on the whole tables for all tiles; the fused call is the per-tile call under the
name ``*_tiles``, with `tile_cols` after `d` and the partials' tile stride after the partials, so each pass has ONE
binder and `Tables` says which form it binds.  ``has_spmm_tiles`` / ``spmm_update_tiles`` / ``spmm_update_class_tiles`` /
``spmm_update_owned_tiles`` are the kernel backend's optional calls (``KernelBackend`` gives them a body that says no):
a backend without them keeps one launch per tile.  The owned pass's binder is owned.bind_launch.
Every binder takes `w`: None binds the per-edge call on the engine's P; the rows' weights (the engine found every row of P
uniform, SweepEngine.uniform_weights) bind the call of the same name with ``_rw`` on them instead -- bit for bit the same."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any


@dataclass(frozen=True)
class Tables:
    """One column tile's views of a block's tables (`tile`: whose partials the call gets); or, fused, the whole tables
    for all tiles, with `cols` = (tile_cols,) and `strides` = (between the tiles' partials,): what the fused call takes
    after `d` and after the partials."""
    Zold: Any
    X: Any
    Znew: Any
    d: int
    tile: int = 0
    cols: tuple = ()
    strides: tuple = ()

    @property
    def fused(self) -> bool:
        return bool(self.cols)

    def method(self, per_tile: str, w=None) -> str:
        return per_tile + ("_tiles" if self.fused else "") + ("_rw" if w is not None else "")

    def mirrored(self, mirror) -> dict:
        """The `mirror` argument of a per-tile call; the fused calls have none (mirrored engines have no tiles)."""
        assert not (self.fused and mirror is not None)
        return {} if self.fused else {"mirror": mirror}


def backend_has(eng, tile_cols: int) -> bool:
    """Whether the backend runs this engine's tables in tiles of `tile_cols` columns with one launch per pass."""
    return bool(eng.k.has_spmm_tiles(eng.dtype, eng.d, tile_cols))


def bind_row(eng, rowptr, nrows: int, row0: int, v: Tables, gamma: float, partials, mirror=None, w=None):
    """The row pass of one block on `v`; `w`: the weights of rowptr's rows."""
    assert w is None or mirror is None
    return eng._bind(v.method("spmm_update", w), rowptr, eng.colidx, eng.P if w is None else w, nrows, row0, v.Zold, v.X,
                     gamma, v.Znew, v.d, *v.cols, eng.long_threshold, partials, *v.strides, sinks_untouched=True,
                     **({} if w is not None else v.mirrored(mirror)), beyond_cache=eng.beyond_cache)


def bind_class(eng, items, row0: int, v: Tables, gamma: float, slab, partials, mirror=None, w=None):
    """Chunk + combine over `items` (a ClassItems) of one block on `v`: two launches.  The fused call also takes the
    slots of a tile, whose chunk sums all lie in the slab at the same time.  `w`: the weights of the block's rows."""
    assert w is None or mirror is None
    n_slots = (int(items.slot_ptr[-1]),) if v.fused else ()
    item_row = () if w is None else (items.row,)
    return eng._bind(v.method("spmm_update_class", w), eng.colidx, eng.P if w is None else w, items.e0, items.len,
                     items.slot, *item_row, items.items_per_block, items.rows, items.slot_ptr, *n_slots, row0, v.Zold, v.X,
                     gamma, v.Znew, v.d, *v.cols, slab, partials, *v.strides,
                     **({} if w is not None else v.mirrored(mirror)), beyond_cache=eng.beyond_cache)
