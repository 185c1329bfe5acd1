"""XCD affinity -- host side of the class-affine row kernels (csrc/spmm_update.h, csrc/edge_score.h).

MI355X has 8 XCDs with a private 4 MiB L2 each and deals the workgroups of a launch to them round-robin (workgroup w
runs on XCD (w + c) % 8 with c fixed within a launch; tools/xcc_map.hip, clane_xcc_ids).  When any workgroup may gather any row of Z, all eight L2s cache the same few
thousand hottest rows.  The class-affine kernels keep every gathered row on ONE XCD instead: each table row gets a
class 0..7 (`xcd_class`), the edges of a long row are sorted by (class of the column, column) -- `partition.localize`,
`halo.build_halo_layout` -- and cut into work items of one class (`class_items`), laid out so that the items of
class b run on the workgroups 8 j + b.  No counterpart in the reference (its loop is embedder.py:84-92 for every row
alike); measurements in profiles/r02_gather_rows_ceiling.md and r02_class_threshold_sweep.md.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

XCD_CLASSES = 8          # MI355X: 8 XCDs, one private L2 each


def xcd_class(position):
    """XCD class (0..7) of the table row at `position` (numpy array, torch tensor or int): an xor-fold of the
    position's 3-bit groups.  Two things matter.  (1) NOT position % 8: that pins three low address bits of every
    row an XCD gathers, and only part of its L2's channels / sets get used -- measured on the pure gather
    (profiles/r02_gather_rows_ceiling.md): 128-byte rows 13.4 TB/s with % 8, 19.4 TB/s with this; 256-byte rows
    17.1 -> 19.5; 1-KiB rows the same.  (2) Heat must be dealt evenly whatever the layout: 8 consecutive rows go to 8
    different classes, so the hottest rows of every sorted run of a table (hot-rows-first Z, but also each
    (chunk, source rank) list of a halo table) are spread over all XCDs.  ((position / 8) % 8 is as fast on the
    hot-first layout and 40 % slower on a halo table, whose runs each start with their 8 hottest rows.)"""
    p = position
    return (p ^ (p >> 3) ^ (p >> 6) ^ (p >> 9)) & (XCD_CLASSES - 1)


def xcd_subclass(position, row_degree, class_threshold: int, phase_threshold: int = 0, phases: int = 1):
    """Sort key of an edge inside its row, ahead of the column: 0 for rows of at most `class_threshold` edges (plain
    column order); the XCD class of the column for class rows; `phase * 8 + class` for HEAVY rows (more than
    `phase_threshold` edges, `phases` > 1), where phase = (column / 64) % phases.  Works on numpy arrays and torch
    tensors alike (`position` and `row_degree` of equal shape)."""
    cls = xcd_class(position)
    if phases > 1 and phase_threshold > 0:
        cls = cls + XCD_CLASSES * (((position >> 6) % phases) * (row_degree > phase_threshold))
    return cls * (row_degree > class_threshold)


# Rows above CLASS_THRESHOLD edges are gathered XCD-affine (csrc/spmm_update.h, spmm_class_chunk_kernel): their edges
# are sorted by (class of the column, column) -- xcd_class above --, cut into chunks of at most CLASS_CHUNK edges
# of one class, and the chunks of class b run on the workgroups 8 j + b = XCD b, so each XCD's 4 MiB L2 caches its own
# eighth of the hot rows instead of all eight caching the same ones.  Costs one partial sum (d accumulators, written +
# read once) per chunk, which is why short rows stay with the row kernels.  Threshold by rows per wave-instruction,
# 0 = off; measured (profiles/r02_class_threshold_sweep.md), sweep ms without -> with: config 3 (1-KiB rows)
# 5.36 -> 4.36 at 64; its column slices: 512-B rows 2.55 -> 1.99 at 64, 256-B rows 1.26 -> 1.04 at 128..256, 128-B rows
# 0.716 -> 0.632 at 256; config 4's shape (bf16, 256-B rows) 8.24 -> 7.44 at 256; config 2 (Z fits the Infinity Cache)
# 0.257 -> 0.249.  build_P scores these rows over the same chunks (class_k1: 5.7 -> 4.7 ms at config 3).
CLASS_THRESHOLD_BY_ROWS_PER_WAVE = {1: 64, 2: 64, 4: 256, 8: 256}
CLASS_CHUNK = 256
# HEAVY class rows are additionally PHASED in time: the rows of a class are split into sub-classes ((column / 64) %
# phases: every sub-class gets the same mix of hot and cold rows) and all chunks of sub-class 0 are scheduled before
# those of sub-class 1, ... -- at any moment an XCD's hot working set is 1/phases of its class.  At 1-KiB rows the 4096
# hottest rows of a class ARE the 4 MiB L2; halving / quartering that working set lifts the pure gather from 14.3 to
# 15.5 / 16.7 TB/s (profiles/r02_gather_rows_ceiling.md).  Every phase multiplies a row's pieces and partial sums,
# hence heavy rows only (above PHASE_THRESHOLD edges).  Measured (profiles/r02_class_threshold_sweep.md): config 3
# 4.31 -> 4.01 ms with 4 phases (build_P 4.72 -> 4.44); its 512-byte column slice 1.98 -> 1.91 with 2; narrower rows
# lose (their hot rows already fit).
PHASES_BY_ROWS_PER_WAVE = {1: 4, 2: 2, 4: 1, 8: 1}
# A one-GPU sweep cut into column tiles (engine._pick_tiles) plans for the TILE's row width, but build_P's K1 still reads
# whole rows over the same edge order.  0 = by the tile's width (the table above); 4 is the measured better choice at
# config 3 (two tiles of 512 bytes under 1-KiB rows: build_P 3.81 -> 3.65-3.67 ms, sweep 3.66-3.67 -> 3.65-3.66,
# profiles/r05_tiles_phases_ab.jsonl) -- switch it together with a re-take of the PMC passes: class_phases is part of
# kernel_config(), profiles/traffic.json's entry was measured with two.
PHASES_UNDER_COLUMN_TILES = 0
PHASE_THRESHOLD = 512
CLASS_ITEMS_PIECE_EDGES = 1 << 28
# Chunks per workgroup, at most.  Round 2 found 16 / 32 / 64 alike on config 3 and took 32; measured again in round 3
# across shapes (profiles/r03_items_per_block.md): 16 is within 1 % of the best everywhere and ahead of 32 where a
# launch holds fewer chunks -- config 2 (108 k chunks) 0.141 -> 0.107 ms for the class pass, config 3 2.355 -> 2.29 ms.
CLASS_ITEMS_PER_BLOCK = 16



def row_pieces(rowptr: np.ndarray, max_edges: int):
    """Consecutive row ranges [a, b) covering all rows, each with at most ``max_edges`` edges (a single row with more
    is a piece of its own)."""
    n = rowptr.size - 1
    a = 0
    while a < n:
        b = int(np.searchsorted(rowptr, rowptr[a] + max_edges, side="right")) - 1
        b = min(max(b, a + 1), n)
        yield a, b
        a = b


def class_items(rowptr: np.ndarray, colidx: np.ndarray, rows: np.ndarray, chunk: int, items_per_block: Optional[int],
                row_ids: Optional[np.ndarray] = None, colidx_dev: Optional[torch.Tensor] = None,
                phase_threshold: int = 0, phases: int = 1, mega_segment_edges: int = 0, mega_min_edges: int = 0,
                segments=None) -> dict:
    """Work items of the XCD-affine pass over `rows` (absolute local row ids whose edges are sorted by
    (xcd_class(column), column)): every class segment of a row is cut into chunks of at most `chunk` edges.
    Slots -- where the partial sums go -- are numbered row by row, class by class, chunk by chunk, so a row's slots
    are contiguous (`slot_ptr`) and summed in that order.  Items are laid out for the kernel: blocks of
    `items_per_block` items of ONE class, block j of class b at block index 8 j + b, padded with empty items
    (len 0, slot -1).  With `phases` > 1 the rows above `phase_threshold` edges are cut by (phase, class) -- their
    edges sorted by xcd_subclass -- and their blocks come first, phase by phase (each phase a whole number of
    8-block rounds, so block index % 8 stays the class), then the blocks of the other rows.  Inside a class the items go row
    by row, except those of mega rows (`mega_segment_edges`), which come first ordered by their first column.  Returns int64 e0, int32 len, int32 slot, int32 row (flat, whole blocks; row = `row_ids` of the
    item's row, default `rows` itself), int64 slot_ptr [rows + 1] and the items_per_block used (None on entry: chosen
    by `items_per_block_for` from the item count, once the O(E) counting pass has it -- the layout itself is cheap).
    `segments`: what `row_segments` returns for these rows, for a caller that has it already."""
    n = rows.size
    NS = XCD_CLASSES * max(1, phases)                       # sub-classes per row (phase-major)
    sizes, seg_len, seg_e0 = segments if segments is not None else \
        row_segments(rowptr, colidx, rows, colidx_dev, phase_threshold, phases)
    nchunk = -(-seg_len // chunk)
    tot = int(nchunk.sum())
    if items_per_block is None:
        items_per_block = items_per_block_for(tot)
    seg_of = np.repeat(np.arange(n * NS), nchunk)
    within = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(nchunk) - nchunk, nchunk)
    e0 = seg_e0[seg_of] + within * chunk
    ln = np.minimum(chunk, seg_len[seg_of] - within * chunk)
    slot_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nchunk.reshape(n, NS).sum(1), out=slot_ptr[1:])
    item_cls = (seg_of % NS) % XCD_CLASSES
    heavy = sizes > phase_threshold if (phases > 1 and phase_threshold > 0) else np.zeros(n, dtype=bool)
    # rows whose average (phase, class) segment exceeds `mega_segment_edges` edges (0 = none): see the item order below
    # and that read at least `mega_min_edges` table rows (the engine passes a quarter of the table: two such rows
    # share much of what they gather; 256 hubs that each read 3.6 % of a 33M-row table do not, and lost 4 % by column)
    mega = ((sizes > mega_segment_edges * XCD_CLASSES * np.where(heavy, max(1, phases), 1)) & (sizes >= mega_min_edges)) \
        if mega_segment_edges > 0 else np.zeros(n, dtype=bool)
    # launch groups, in order: the heavy rows' items phase by phase, then everybody else's
    item_group = np.where(heavy[seg_of // NS], (seg_of % NS) // XCD_CLASSES, max(1, phases))
    ids = (rows if row_ids is None else row_ids).astype(np.int32)
    item_row = ids[seg_of // NS]
    pieces = []
    for g in range(max(1, phases) + 1):
        in_group = item_group == g
        if not in_group.any():
            continue
        per_class = [np.nonzero(in_group & (item_cls == c))[0] for c in range(XCD_CLASSES)]
        if mega.any():
            # MEGA rows -- one (phase, class) segment of the row alone is more than an L2 holds -- come first in their
            # class, their items in the order of their first column instead of row by row: chunks of DIFFERENT mega rows
            # that gather the same stretch of the table then run next to each other and share it through the L2 (ten rows
            # that read all 2M vertices: class pass 3.03 -> 1.68 ms).  Row by row, such a row has left the L2 long
            # before the next one comes by; for rows whose segments fit (config 3's 70k-edge hub: 2.2 MB) row order is
            # the better one (2.35 vs 2.41 ms).  Slots, and with them the order of every sum, stay row-major.
            ordered = []
            for pc in per_class:
                is_mega = mega[seg_of[pc] // NS]
                first = pc[is_mega]
                ordered.append(np.concatenate([first[np.argsort(colidx[e0[first]], kind="stable")], pc[~is_mega]]))
            per_class = ordered
        nblk = max(-(-len(pc) // items_per_block) for pc in per_class)
        flat = XCD_CLASSES * nblk * items_per_block
        g_e0 = np.zeros(flat, dtype=np.int64)
        g_len = np.zeros(flat, dtype=np.int32)
        g_slot = np.full(flat, -1, dtype=np.int32)
        g_row = np.zeros(flat, dtype=np.int32)
        for c, pc in enumerate(per_class):
            t = np.arange(len(pc))
            where = (t // items_per_block) * (XCD_CLASSES * items_per_block) + c * items_per_block + t % items_per_block
            g_e0[where], g_len[where], g_slot[where], g_row[where] = e0[pc], ln[pc], pc, item_row[pc]
        pieces.append((g_e0, g_len, g_slot, g_row))
    if not pieces:                                          # no edges at all: one round of empty blocks
        flat = XCD_CLASSES * items_per_block
        pieces.append((np.zeros(flat, dtype=np.int64), np.zeros(flat, dtype=np.int32),
                       np.full(flat, -1, dtype=np.int32), np.zeros(flat, dtype=np.int32)))
    out_e0, out_len, out_slot, out_row = (np.concatenate([p[i] for p in pieces]) for i in range(4))
    return {"e0": out_e0, "len": out_len, "slot": out_slot, "row": out_row, "slot_ptr": slot_ptr,
            "items_per_block": int(items_per_block)}


def row_segments(rowptr: np.ndarray, colidx: np.ndarray, rows: np.ndarray, colidx_dev: Optional[torch.Tensor] = None,
                 phase_threshold: int = 0, phases: int = 1):
    """The (phase, class) segments of `rows` (absolute local row ids whose edges are sorted by
    (xcd_subclass(column), column); AssertionError otherwise): the rows' edge counts [n], the segments' lengths and
    first edges [n * NS], NS = 8 * phases, row-major then phase-major.  One O(E) counting pass, on the card when
    `colidx_dev` is there."""
    n = rows.size
    NS = XCD_CLASSES * max(1, phases)                       # sub-classes per row (phase-major)
    sizes = (rowptr[rows + 1] - rowptr[rows]).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    if colidx_dev is not None and colidx_dev.is_cuda:        # the O(E) part on the card (40M edges: 0.3 s on the host)
        dev = colidx_dev.device
        seg_len = np.empty(n * NS, dtype=np.int64)
        unsorted = False
        bounds = np.concatenate([[0], np.cumsum(sizes)])
        for a, b in row_pieces(bounds, CLASS_ITEMS_PIECE_EDGES):    # pieces bound the scratch memory on the card
            if bounds[b] == bounds[a]:
                seg_len[a * NS:b * NS] = 0
                continue
            sizes_t = torch.from_numpy(sizes[a:b]).to(dev)
            rid = torch.repeat_interleave(torch.arange(b - a, device=dev), sizes_t)
            idx = (torch.from_numpy(rowptr[rows[a:b]] - (start[a:b] - bounds[a])).to(dev)[rid]
                   + torch.arange(int(bounds[b] - bounds[a]), device=dev))
            sub = xcd_subclass(colidx_dev[idx].long(), sizes_t[rid], 0, phase_threshold, phases)
            key = rid * NS + sub
            unsorted = unsorted or (bool((key[1:] < key[:-1]).any()) if key.numel() > 1 else False)
            seg_len[a * NS:b * NS] = torch.bincount(key, minlength=(b - a) * NS).cpu().numpy()
    else:
        idx = np.repeat(rowptr[rows] - start, sizes) + np.arange(int(sizes.sum()), dtype=np.int64)
        rid = np.repeat(np.arange(n, dtype=np.int64), sizes)
        sub = xcd_subclass(colidx[idx].astype(np.int64), sizes[rid], 0, phase_threshold, phases)
        unsorted = idx.size > 1 and bool((np.diff(rid * NS + sub) < 0).any())
        seg_len = np.bincount(rid * NS + sub, minlength=n * NS)
    if unsorted:
        raise AssertionError("class rows must have their edges sorted by (xcd_subclass(column), column)")
    seg_e0 = np.repeat(rowptr[rows], NS) + (np.cumsum(seg_len) - seg_len - np.repeat(start, NS))
    return sizes, seg_len.astype(np.int64), seg_e0


def items_per_block_for(n_items: int) -> int:
    """Chunks per workgroup of the class kernels: CLASS_ITEMS_PER_BLOCK when there are plenty, fewer (down to one per
    wave) when a launch holds few chunks -- a launch wants >= ~4096 workgroups to fill 256 CUs (a rank's quarter of
    the halo split at 8 GPUs holds 21k chunks: 650 workgroups of 32 ran at a third of the rate of 2 600 of 8)."""
    return int(min(CLASS_ITEMS_PER_BLOCK, max(4, 4 * -(-n_items // (4 * 4096)))))


# ---- owned class rows: the plan of spmm_owned_kernel (csrc/spmm_update.h) -------------------------------------------
# Class rows of at most OWNED_MAX_EDGES edges are summed by row-owning workgroups instead of chunk + combine: a
# workgroup keeps the sums of its rows in LDS and walks the rows' (phase, class) segments step by step, so nothing goes
# through a slab.  Measured on R-MAT 2M / 40M / d = 256 in two column tiles, one engine, variants alternating
# (profiles/r06_owned_class_pass.md; sweep ms, chunk + combine 3.623):
#  * what decides is how many BATCHES a group needs and how far the groups drift apart: 512 groups of 768 threads with
#    72 KiB each (two batches, 3 % step spread) 3.79; 256 groups of 1024 threads with 144 KiB (two batches, 2 %) 3.62;
#  * all class rows up to 4096 edges are 92 k sums of 512 bytes = 47 MB, more than the 40 MB of LDS on the card: two
#    batches at best, and 16 steps (the rows above PHASE_THRESHOLD are phased).  The 74.7 k rows up to 512 edges fit ONE
#    batch of 152 KiB per CU and have 8 steps, dealt to 0.4 % per step: 3.56;
#  * 16 waves per CU leave registers for 12 row loads in flight per wave: 3.52 (8: 3.55 at two batches; 6: 3.56 / 3.62).
# Rows above OWNED_ROW_EDGES edges would be cut into virtual rows (several waves per row and step): none at 512.
OWNED_MAX_EDGES = 512
OWNED_ROW_EDGES = 1024
OWNED_GROUPS = 256               # one workgroup per CU ...
OWNED_BLOCK_THREADS = 1024       # ... of 16 waves
OWNED_LDS_BYTES = 152 * 1024     # its sums: 304 rows of 512 bytes
OWNED_LOADS = 12                 # row loads in flight per wave (CLANE_OWNED_LOADS), 0 = as the chunk kernel
# SweepEngine(class_owned=None): on where it was measured to pay -- XCD-affine class rows of a table far beyond the
# Infinity Cache (engine.beyond_cache), where the kernel has an instance.  A cache-resident table (config 2) or evenly
# spread reads keep chunk + combine: not measured to gain, so not switched.
OWNED_DEFAULT = True
# SweepEngine(fused_tiles=None): the passes that run ALL column tiles in one launch (spmm_update*_tiles: "row", "class",
# "owned") instead of one launch per tile, and SweepEngine(owned_ahead=None): whether the owned epilogue requests the next
# rows' x / z_old ahead.  Bit for bit the per-tile plan; each piece is on where its own pass's time fell by more than
# the box's spread (profiles/r16_fused_tiles.md), else off.
FUSED_TILES_DEFAULT = ("row", "class", "owned")
# SweepEngine(uniform_weights=None) for a table far beyond the Infinity Cache (every other engine: False).  False = every
# K3 call reads one weight per edge; "auto" = where build_P left every row of P with one float on all of its edges
# (reference mode on a graph of tens of millions of edges: 1 / deg), the row, class and owned passes read one weight per
# row instead (spmm_update*_rw, bit for bit the same).  Config 3: 3.490 -> 3.439 ms per sweep against the parent commit,
# for 0.20 ms more per build_P.  Config 2 (4M edges, a cache-resident table) has a mixed P: the look at its rows would cost
# 0.21 ms per build_P -- one of its sweeps -- and gain nothing (profiles/r21_uniform_weights.md).
UNIFORM_WEIGHTS_DEFAULT = "auto"
OWNED_EPILOGUE_AHEAD = True


def owned_plan(sizes: np.ndarray, seg_len: np.ndarray, seg_e0: np.ndarray, row_ids: np.ndarray, row_parts: np.ndarray,
               *, row_edges: int, groups: int, batch_vrows: int) -> Optional[dict]:
    """Plan of the owned pass over n rows given by `row_segments` (sizes [n], seg_len / seg_e0 [n * NS]); `row_ids`:
    the rows relative to the launch's first row, `row_parts`: their slots in the delta partials.

    STEPS are the (phase, class) keys that hold any edge, in increasing order.  A row of more than `row_edges` edges is
    cut into VIRTUAL rows of at most that many, evenly over the keys: virtual row j of nv takes the edges
    [j L / nv, (j + 1) L / nv) of every segment of L edges.  Rows (with all their virtual rows) are dealt to `groups`
    groups, heaviest first, each to the group whose cumulative edges stay lowest against the fair share at every step
    (lowest index on a tie): the groups then change step at about the same time.  A
    group takes its rows, in the order dealt, in consecutive BATCHES of at most `batch_vrows` virtual rows.  Returns
    the flat arrays of clane_owned_plan_t (include/clane_hip.h) plus `group_step_edges` [groups, steps] for whoever
    wants to look at the balance; None without rows.  The order in which a row's edges are summed -- (virtual row,
    step, piece) -- does not depend on `groups` or `batch_vrows`."""
    n = int(sizes.size)
    if n == 0:
        return None
    if groups < 1 or row_edges < 64:
        raise ValueError("owned_plan: groups must be >= 1 and row_edges >= 64")
    NS = seg_len.size // n
    seg_len = seg_len.reshape(n, NS).astype(np.int64)
    seg_e0 = seg_e0.reshape(n, NS).astype(np.int64)
    keys = np.nonzero(seg_len.sum(0) > 0)[0]
    if keys.size == 0:
        keys = np.zeros(1, dtype=np.int64)
    S = int(keys.size)
    seg_len, seg_e0 = seg_len[:, keys], seg_e0[:, keys]
    # virtual rows: as few as keep every one of them within row_edges (the bound: a share of L edges is <= ceil(L / nv))
    nv = np.maximum(1, -(-sizes // row_edges)).astype(np.int64)
    while True:
        over = (-(-seg_len // nv[:, None])).sum(1) > row_edges
        if not over.any():
            break
        nv[over] += 1
    if int(nv.max()) > batch_vrows:
        raise ValueError(f"owned_plan: a row of {int(nv.max())} virtual rows does not fit a batch of {batch_vrows}")
    # The deal: heaviest row first, to the group that stays furthest below its share at EVERY step.  What costs hit rate
    # is drift -- a group that is ahead or behind in edges when the others change step -- so a group's load is its
    # cumulative edges after each step over that step's fair share, and a row goes where the largest of them ends lowest.
    row_cum = np.cumsum(seg_len, 1).astype(np.float64)
    share = np.maximum(row_cum.sum(0) / groups, 1.0)
    row_cum /= share
    cum = np.zeros((groups, S))
    group_of = np.empty(n, dtype=np.int64)
    dealt = np.argsort(-sizes, kind="stable")
    for i in dealt.tolist():
        g = int((cum + row_cum[i]).max(1).argmin())
        group_of[i] = g
        cum[g] += row_cum[i]
    order = dealt[np.argsort(group_of[dealt], kind="stable")]         # by group, inside a group as dealt
    g_sorted, nv_sorted = group_of[order], nv[order]
    bat_of_row = np.empty(n, dtype=np.int64)
    b, used, g_prev = -1, 0, -1
    for j, (g, k) in enumerate(zip(g_sorted.tolist(), nv_sorted.tolist())):
        if g != g_prev or used + k > batch_vrows:
            b, used, g_prev = b + 1, 0, g
        used += k
        bat_of_row[j] = b
    B = b + 1
    bat_row_ptr = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(np.bincount(bat_of_row, minlength=B), out=bat_row_ptr[1:])
    row_vptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nv_sorted, out=row_vptr[1:])
    bat_vrow_ptr = row_vptr[bat_row_ptr]
    bat_group = g_sorted[bat_row_ptr[:-1]]
    grp_bat_ptr = np.zeros(groups + 1, dtype=np.int64)
    np.cumsum(np.bincount(bat_group, minlength=groups), out=grp_bat_ptr[1:])
    # the virtual rows' shares of every step, in the new order
    nvirt = int(row_vptr[-1])
    v_row = np.repeat(np.arange(n), nv_sorted)                         # position of the row in `order`
    v_j = np.arange(nvirt) - row_vptr[v_row]
    L, E0, NV = seg_len[order][v_row], seg_e0[order][v_row], nv_sorted[v_row][:, None]
    lo = (v_j[:, None] * L) // NV
    hi = ((v_j[:, None] + 1) * L) // NV
    v_len, v_e0 = hi - lo, E0 + lo
    v_idx, s_idx = np.nonzero(v_len > 0)
    v_bat = bat_of_row[v_row]
    key = v_bat[v_idx] * S + s_idx
    by = np.lexsort((v_idx, key))                                      # (batch, step), then virtual row
    v_idx, s_idx, key = v_idx[by], s_idx[by], key[by]
    bat_seg_ptr = np.zeros(B * S + 1, dtype=np.int64)
    np.cumsum(np.bincount(key, minlength=B * S), out=bat_seg_ptr[1:])
    group_step = np.zeros((groups, S), dtype=np.int64)
    np.add.at(group_step, (g_sorted[v_row][v_idx], s_idx), v_len[v_idx, s_idx])
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)            # noqa: E731
    return {"grp_bat_ptr": i32(grp_bat_ptr), "bat_vrow_ptr": i32(bat_vrow_ptr), "bat_row_ptr": i32(bat_row_ptr),
            "bat_seg_ptr": i32(bat_seg_ptr), "seg_e0": np.ascontiguousarray(v_e0[v_idx, s_idx], dtype=np.int64),
            "seg_len": i32(v_len[v_idx, s_idx]), "seg_vrow": i32(v_idx - bat_vrow_ptr[v_bat[v_idx]]),
            "row_id": i32(row_ids[order]), "row_part": i32(row_parts[order]), "row_vptr": i32(row_vptr),
            "n_groups": int(groups), "n_steps": S, "max_batch_vrows": int(np.diff(bat_vrow_ptr).max()),
            "steps": keys.astype(np.int64), "group_step_edges": group_step}
