"""The owned class pass of a SweepEngine (csrc/spmm_update.h spmm_owned_kernel; the reference's loop is
embedder.py:84-92 for every row alike): which engines can take it, one block's plan, the bound launch.
``has_spmm_owned`` / ``make_owned_plan`` / ``spmm_update_owned`` are the kernel backend's optional calls
(``KernelBackend`` gives them a body that says no): a backend without them keeps every class row on chunk + combine."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import xcd
from .blocks import ClassItems, OwnedRows, PartialLayout


def possible(eng) -> bool:
    """One GPU, no mirrored launches, a class pass at all, and an instance for every column tile's width."""
    widths = [c1 - c0 for c0, c1 in eng.tiles]
    return bool(eng.world == 1 and not eng._forced and eng.class_threshold > 0 and eng.d > 0
                and all(eng.k.has_spmm_owned(eng.dtype, w) for w in widths))


def plan_block(eng, layout: PartialLayout, rows_c: np.ndarray, rows_abs: np.ndarray, segments,
               phased: dict) -> Optional[OwnedRows]:
    """One block's class rows divided between the owned pass (at most owned_max_edges edges) and chunk + combine: the
    plan on the device, the class items of the rows above or None, the number of rows above; None without owned rows.
    `layout` says which of the block's delta partials the owned rows get."""
    dev = eng.device
    sizes, seg_len, seg_e0 = segments
    NS = seg_len.size // max(1, sizes.size)
    own = sizes <= eng.owned_max_edges
    if not own.any():
        return None
    n_rest = int((~own).sum())
    pick = lambda a, m: a.reshape(sizes.size, NS)[m].reshape(-1)       # noqa: E731
    plan = xcd.owned_plan(sizes[own], pick(seg_len, own), pick(seg_e0, own), rows_c[own],
                          layout.owned_slots(n_rest, int(own.sum())), row_edges=eng.owned_row_edges,
                          groups=eng.owned_groups, batch_vrows=eng.owned_batch_vrows)
    eng.owned_balance = plan["group_step_edges"]
    rest = None
    if n_rest:
        keep = ~own
        items = xcd.class_items(eng.local.rowptr, eng.local.colidx, rows_abs[keep], eng.class_chunk, None,
                                row_ids=rows_c[keep], segments=(sizes[keep], pick(seg_len, keep), pick(seg_e0, keep)),
                                **phased)
        rest = ClassItems.upload(items, rows_c[keep], dev)
    return OwnedRows(eng.k.make_owned_plan(plan, eng.owned_chunk, dev), rest, n_rest)


def bind_launch(eng, plan, row0: int, v, gamma: float, partials, w=None):
    """The owned launch of one block on `v` (a fused.Tables: one column tile, or all of them in one launch), bound like
    every other call of a sweep's plan.  `ahead=True` where the engine has the epilogue's look-ahead on -- only backends
    that declare ``owned_epilogue_ahead`` are ever asked for it.  `w`: the weights of the block's rows (fused.py)."""
    ahead = {"ahead": True} if getattr(eng, "owned_ahead", False) else {}
    return eng._bind(v.method("spmm_update_owned", w), eng.colidx, eng.P if w is None else w, plan,
                     eng.owned_block_threads, row0, v.Zold, v.X, gamma, v.Znew, v.d, *v.cols, partials, *v.strides,
                     beyond_cache=eng.beyond_cache, loads=eng.owned_loads, **ahead)
