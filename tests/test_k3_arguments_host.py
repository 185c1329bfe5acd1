"""The error contract of the eight K3 entry points of the C ABI: what a rejected call returns and what it leaves in
clane_last_error, and which calls return CLANE_OK before any launch (zero rows, zero groups).

Every call below returns before a launch, so no GPU is needed.  The calls are made through ctypes with one small HOST
buffer standing in for every pointer; they run in a child process that sees no GPU, so that a call which a later
change lets through by mistake ends in a launch error there and not in a kernel reading host addresses.

EXPECTED was recorded from the library of the commit before the launchers were merged into one per pass
(spmm_update_impl, spmm_update_class_impl, spmm_update_owned_impl in csrc/clane_abi.hip): the texts, their prefixes,
the return codes and which check reports first are the contract the launchers keep."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

TABLES = [("Z_old", "B"), ("ldz", 8), ("X", "B"), ("ldx", 8), ("gamma", 0.5), ("Z_new", "B2"), ("ldo", 8), ("d", 8)]
TAIL = [("delta_partials", "B"), ("stream", None)]
CLASS_ITEMS = [("colidx", "B"), ("P", "B"), ("item_e0", "B"), ("item_len", "B"), ("item_slot", "B"), ("n_blocks", 1),
               ("items_per_block", 4), ("class_rows", "B"), ("slot_ptr", "B"), ("n_rows", 1)]
OWNED_HEAD = [("colidx", "B"), ("P", "B"), ("plan", {}), ("block_threads", 256), ("row0", 0)]
# argument order and a default that passes every check, per entry point (include/clane_hip.h)
ARGS = {
    "update": [("rowptr", "B"), ("colidx", "B"), ("P", "B"), ("nrows", 1), ("row0", 0)] + TABLES
    + [("long_threshold", 0), ("flags", 0), ("mirror", None)] + TAIL,
    "update_long": [("rowptr", "B"), ("colidx", "B"), ("P", "B"), ("long_rows", "B"), ("n_long", 1), ("waves_per_row", 16),
                    ("row0", 0)] + TABLES + [("mirror", None)] + TAIL,
    "update_split": [("rowptr", "B"), ("colidx", "B"), ("P", "B"), ("split_rows", "B"), ("seg_ptr", "B"), ("seg_row", "B"),
                     ("n_split", 1), ("n_segments", 1), ("edges_per_segment", 64), ("row0", 0)] + TABLES
    + [("slab", "B"), ("mirror", None)] + TAIL,
    "update_class": CLASS_ITEMS + [("row0", 0)] + TABLES + [("flags", 0), ("slab", "B"), ("mirror", None)] + TAIL,
    "update_owned": OWNED_HEAD + TABLES + [("flags", 0)] + TAIL,
    "update_tiles": [("rowptr", "B"), ("colidx", "B"), ("P", "B"), ("nrows", 1), ("row0", 0)] + TABLES
    + [("tile_cols", 8), ("long_threshold", 0), ("flags", 0), ("delta_partials", "B"), ("partials_tile_stride", 1),
       ("stream", None)],
    "update_class_tiles": CLASS_ITEMS + [("n_slots", 1), ("row0", 0)] + TABLES
    + [("tile_cols", 8), ("flags", 0), ("slab", "B"), ("delta_partials", "B"), ("partials_tile_stride", 1),
       ("stream", None)],
    "update_owned_tiles": OWNED_HEAD + TABLES
    + [("tile_cols", 8), ("flags", 0), ("delta_partials", "B"), ("partials_tile_stride", 1), ("stream", None)],
}
PLAN = dict(n_groups=1, n_steps=1, chunk=64, max_batch_vrows=1)
WIDE = dict(ldz=128, ldx=128, ldo=128, d=128)                  # a width the owned pass has an instance for
TWO_TILES = dict(ldz=256, ldx=256, ldo=256, d=256, tile_cols=128)
HALF_MIRROR = ("mirror", "B", None, "B", 8, 1)                 # row_ptr, slot, bufs, ld, aligned16: no slot

# (entry point, dtype suffix, what differs from the defaults)
CASES = [
    # -- the row pass, per tile ---------------------------------------------------------------------------------------
    ("update", "f32", dict(ldz=7)),
    ("update", "f32", dict(Z_new="B")),
    ("update", "f32", dict(colidx=None)),
    ("update", "f32", dict(delta_partials=None)),
    ("update", "f32", dict(nrows=-1)),
    ("update", "f32", dict(long_threshold=-1)),
    ("update", "f32", dict(mirror=HALF_MIRROR)),
    ("update", "f32", dict(mirror=("mirror", "B", "B", "B", 7, 1))),
    ("update", "f32", dict(nrows=0, rowptr=None, Z_new="B")),                   # CLANE_OK: zero rows
    ("update", "f32", dict(nrows=0, ldo=7)),                                    # ... but only of a well-formed call
    ("update", "f32", dict(nrows=-1, ldz=7, Z_new="B", delta_partials=None)),   # several fail: the shape reports
    ("update", "f32", dict(mirror=HALF_MIRROR, ldx=7, long_threshold=-1)),      # the mirror before the tables
    ("update", "bf16", dict(ldx=7)),
    ("update", "bf16", dict(Z_new="B")),
    ("update", "f64", dict(d=0)),
    # -- long rows ----------------------------------------------------------------------------------------------------
    ("update_long", "f32", dict(ldo=7)),
    ("update_long", "f32", dict(Z_new="B")),
    ("update_long", "f32", dict(long_rows=None)),
    ("update_long", "f32", dict(delta_partials=None)),
    ("update_long", "f32", dict(n_long=-1)),
    ("update_long", "f32", dict(waves_per_row=5)),
    ("update_long", "f32", dict(mirror=HALF_MIRROR)),
    ("update_long", "f32", dict(n_long=0, waves_per_row=5, Z_new="B")),         # CLANE_OK: zero rows
    ("update_long", "f32", dict(waves_per_row=5, Z_new="B")),                   # the alias before the waves
    ("update_long", "f64", dict(waves_per_row=5)),
    ("update_long", "f64", dict(ldz=7)),
    # -- split rows ---------------------------------------------------------------------------------------------------
    ("update_split", "f32", dict(ldx=7)),
    ("update_split", "f32", dict(Z_new="B")),
    ("update_split", "f32", dict(seg_ptr=None)),
    ("update_split", "f32", dict(slab=None)),
    ("update_split", "f32", dict(n_split=-1)),
    ("update_split", "f32", dict(n_segments=0)),
    ("update_split", "f32", dict(edges_per_segment=63)),
    ("update_split", "f32", dict(slab="ODD")),
    ("update_split", "f32", dict(mirror=HALF_MIRROR, edges_per_segment=63)),    # the mirror before the shape
    ("update_split", "f32", dict(n_split=0, n_segments=0, slab="ODD")),         # CLANE_OK: zero rows
    ("update_split", "bf16", dict(edges_per_segment=63)),
    ("update_split", "bf16", dict(slab="ODD")),
    # -- the class pass, per tile -------------------------------------------------------------------------------------
    ("update_class", "f32", dict(ldz=7)),
    ("update_class", "f32", dict(Z_new="B")),
    ("update_class", "f32", dict(item_slot=None)),
    ("update_class", "f32", dict(n_blocks=-1)),
    ("update_class", "f32", dict(n_rows=-1)),
    ("update_class", "f32", dict(items_per_block=3)),
    ("update_class", "f32", dict(items_per_block=65)),
    ("update_class", "f32", dict(slab="ODD")),
    ("update_class", "f32", dict(mirror=HALF_MIRROR, n_blocks=-1)),
    ("update_class", "f32", dict(n_rows=0, slab="ODD", Z_new="B")),             # CLANE_OK: zero rows
    ("update_class", "f32", dict(n_rows=0, items_per_block=3)),
    ("update_class", "f32", dict(items_per_block=3, ldz=7, slab="ODD")),
    ("update_class", "f64", dict(items_per_block=65)),
    ("update_class", "bf16", dict(slab="ODD")),
    # -- the owned class pass, per tile -------------------------------------------------------------------------------
    ("update_owned", "f32", dict(WIDE, plan=None)),
    ("update_owned", "f32", dict(WIDE, plan=dict(n_groups=-1))),
    ("update_owned", "f32", dict(WIDE, plan=dict(n_steps=0))),
    ("update_owned", "f32", dict(WIDE, plan=dict(n_steps=65))),
    ("update_owned", "f32", dict(WIDE, plan=dict(chunk=32))),
    ("update_owned", "f32", dict(WIDE, block_threads=96)),
    ("update_owned", "f32", dict(WIDE, block_threads=2048)),
    ("update_owned", "f32", dict(WIDE, ldz=127)),
    ("update_owned", "f32", dict(WIDE, plan=dict(max_batch_vrows=-1))),
    ("update_owned", "f32", dict(WIDE, plan=dict(seg_len=None))),
    ("update_owned", "f32", dict(WIDE, Z_new="B")),
    ("update_owned", "f32", dict()),                                            # d = 8: no instance
    ("update_owned", "f32", dict(WIDE, Z_old="ODD")),                           # no 16-byte packs: no instance
    ("update_owned", "f32", dict(WIDE, plan=dict(max_batch_vrows=400))),
    ("update_owned", "f32", dict(WIDE, flags=5 << 8)),
    ("update_owned", "f32", dict(ldz=256, ldx=256, ldo=256, d=256, flags=6 << 8)),   # 6 loads: two rows per instruction only
    ("update_owned", "f32", dict(WIDE, plan=dict(n_groups=0, seg_len=None), Z_new="B")),   # CLANE_OK: zero groups
    ("update_owned", "f32", dict(WIDE, plan=dict(n_groups=0, chunk=32))),
    ("update_owned", "f32", dict(WIDE, plan=dict(n_steps=0, chunk=32), block_threads=96)),
    # -- the row pass, every tile in one launch -----------------------------------------------------------------------
    ("update_tiles", "f32", dict(ldz=136, ldx=136, ldo=136, d=136, tile_cols=128)),   # a last tile with another layout
    ("update_tiles", "f32", dict(tile_cols=16)),
    ("update_tiles", "f32", dict(tile_cols=0)),
    ("update_tiles", "f32", dict(ldz=16, ldx=16, ldo=16, d=16, tile_cols=6)),
    ("update_tiles", "f32", dict(TWO_TILES, partials_tile_stride=0)),
    ("update_tiles", "f32", dict(TWO_TILES, ldo=255)),
    ("update_tiles", "f32", dict(TWO_TILES, Z_new="B")),
    ("update_tiles", "f32", dict(TWO_TILES, P=None)),
    ("update_tiles", "f32", dict(TWO_TILES, delta_partials=None)),
    ("update_tiles", "f32", dict(TWO_TILES, nrows=-1)),
    ("update_tiles", "f32", dict(TWO_TILES, long_threshold=-1)),
    ("update_tiles", "f32", dict(TWO_TILES, X="ODD")),
    ("update_tiles", "f32", dict(TWO_TILES, nrows=0, rowptr=None)),             # CLANE_OK: zero rows
    ("update_tiles", "f32", dict(TWO_TILES, nrows=0, partials_tile_stride=0)),
    ("update_tiles", "f32", dict(TWO_TILES, nrows=-1, tile_cols=512, ldz=7)),
    # -- the class pass, every tile in one launch ---------------------------------------------------------------------
    ("update_class_tiles", "f32", dict(ldz=136, ldx=136, ldo=136, d=136, tile_cols=128)),
    ("update_class_tiles", "f32", dict(tile_cols=16)),
    ("update_class_tiles", "f32", dict(TWO_TILES, partials_tile_stride=0)),
    ("update_class_tiles", "f32", dict(TWO_TILES, ldx=255)),
    ("update_class_tiles", "f32", dict(TWO_TILES, Z_new="B")),
    ("update_class_tiles", "f32", dict(TWO_TILES, class_rows=None)),
    ("update_class_tiles", "f32", dict(TWO_TILES, n_blocks=-1)),
    ("update_class_tiles", "f32", dict(TWO_TILES, n_slots=-1)),
    ("update_class_tiles", "f32", dict(TWO_TILES, n_blocks=2**31 - 4)),
    ("update_class_tiles", "f32", dict(TWO_TILES, n_blocks=2**30)),
    ("update_class_tiles", "f32", dict(TWO_TILES, items_per_block=3)),
    ("update_class_tiles", "f32", dict(TWO_TILES, items_per_block=65)),
    ("update_class_tiles", "f32", dict(TWO_TILES, slab="ODD")),
    ("update_class_tiles", "f32", dict(TWO_TILES, Z_old="ODD")),
    ("update_class_tiles", "f32", dict(TWO_TILES, n_rows=0, slab="ODD")),       # CLANE_OK: zero rows
    ("update_class_tiles", "f32", dict(TWO_TILES, n_rows=0, items_per_block=3)),
    ("update_class_tiles", "f32", dict(TWO_TILES, items_per_block=3, tile_cols=512)),
    # -- the owned class pass, every tile in one launch: the plan's own faults report as spmm_update_owned -------------
    ("update_owned_tiles", "f32", dict(ldz=136, ldx=136, ldo=136, d=136, tile_cols=128)),
    ("update_owned_tiles", "f32", dict(TWO_TILES, tile_cols=512)),
    ("update_owned_tiles", "f32", dict(TWO_TILES, partials_tile_stride=-1)),
    ("update_owned_tiles", "f32", dict(TWO_TILES, d=0)),
    ("update_owned_tiles", "f32", dict(TWO_TILES, plan=None)),
    ("update_owned_tiles", "f32", dict(TWO_TILES, plan=dict(n_steps=0))),
    ("update_owned_tiles", "f32", dict(TWO_TILES, plan=dict(chunk=32))),
    ("update_owned_tiles", "f32", dict(TWO_TILES, block_threads=96)),
    ("update_owned_tiles", "f32", dict(TWO_TILES, ldz=255)),
    ("update_owned_tiles", "f32", dict(TWO_TILES, Z_new="B")),
    ("update_owned_tiles", "f32", dict(TWO_TILES, plan=dict(row_vptr=None))),
    ("update_owned_tiles", "f32", dict(ldz=64, ldx=64, ldo=64, d=64, tile_cols=32)),   # tiles too narrow: no instance
    ("update_owned_tiles", "f32", dict(TWO_TILES, plan=dict(max_batch_vrows=400))),
    ("update_owned_tiles", "f32", dict(TWO_TILES, flags=5 << 8)),
    ("update_owned_tiles", "f32", dict(TWO_TILES, plan=dict(n_groups=0), colidx=None)),    # CLANE_OK: zero groups
    ("update_owned_tiles", "f32", dict(TWO_TILES, tile_cols=512, plan=None)),
]

BAD, OK = -1, 0
TILES_TEXT = "tile_cols must be a multiple of the 16-byte pack in (0, d] whose last tile keeps the lane layout"
# (return code, clane_last_error) of every case, in the order of CASES; the text of a CLANE_OK is not part of the contract
EXPECTED = [
    (BAD, "spmm_update: leading dimension < d"),
    (BAD, "spmm_update: Z_new must not alias Z_old (Jacobi sweep)"),
    (BAD, "spmm_update: null pointer"),
    (BAD, "spmm_update: null delta_partials"),
    (BAD, "spmm_update: bad shape nrows=-1 row0=0 d=8"),
    (BAD, "spmm_update: negative long_threshold"),
    (BAD, "spmm_update: incomplete mirror descriptor"),
    (BAD, "spmm_update: incomplete mirror descriptor"),
    (OK, None),
    (BAD, "spmm_update: leading dimension < d"),
    (BAD, "spmm_update: bad shape nrows=-1 row0=0 d=8"),
    (BAD, "spmm_update: incomplete mirror descriptor"),
    (BAD, "spmm_update: leading dimension < d"),
    (BAD, "spmm_update: Z_new must not alias Z_old (Jacobi sweep)"),
    (BAD, "spmm_update: bad shape nrows=1 row0=0 d=0"),
    (BAD, "spmm_update_long: leading dimension < d"),
    (BAD, "spmm_update_long: Z_new must not alias Z_old"),
    (BAD, "spmm_update_long: null pointer"),
    (BAD, "spmm_update_long: null pointer"),
    (BAD, "spmm_update_long: bad shape"),
    (BAD, "spmm_update_long: waves_per_row must be 4 or 16"),
    (BAD, "spmm_update_long: incomplete mirror descriptor"),
    (OK, None),
    (BAD, "spmm_update_long: Z_new must not alias Z_old"),
    (BAD, "spmm_update_long: waves_per_row must be 4 or 16"),
    (BAD, "spmm_update_long: leading dimension < d"),
    (BAD, "spmm_update_split: leading dimension < d"),
    (BAD, "spmm_update_split: Z_new must not alias Z_old"),
    (BAD, "spmm_update_split: null pointer"),
    (BAD, "spmm_update_split: null pointer"),
    (BAD, "spmm_update_split: bad shape (edges_per_segment must be a positive multiple of 64)"),
    (BAD, "spmm_update_split: bad shape (edges_per_segment must be a positive multiple of 64)"),
    (BAD, "spmm_update_split: bad shape (edges_per_segment must be a positive multiple of 64)"),
    (BAD, "spmm_update_split: slab must be 16-byte aligned"),
    (BAD, "spmm_update_split: incomplete mirror descriptor"),
    (OK, None),
    (BAD, "spmm_update_split: bad shape (edges_per_segment must be a positive multiple of 64)"),
    (BAD, "spmm_update_split: slab must be 16-byte aligned"),
    (BAD, "spmm_update_class: leading dimension < d"),
    (BAD, "spmm_update_class: Z_new must not alias Z_old"),
    (BAD, "spmm_update_class: null pointer"),
    (BAD, "spmm_update_class: bad shape"),
    (BAD, "spmm_update_class: bad shape"),
    (BAD, "spmm_update_class: items_per_block must be in [4, 64]"),
    (BAD, "spmm_update_class: items_per_block must be in [4, 64]"),
    (BAD, "spmm_update_class: slab must be 16-byte aligned"),
    (BAD, "spmm_update_class: incomplete mirror descriptor"),
    (OK, None),
    (BAD, "spmm_update_class: items_per_block must be in [4, 64]"),
    (BAD, "spmm_update_class: items_per_block must be in [4, 64]"),
    (BAD, "spmm_update_class: items_per_block must be in [4, 64]"),
    (BAD, "spmm_update_class: slab must be 16-byte aligned"),
    (BAD, "spmm_update_owned: null plan"),
    (BAD, "spmm_update_owned: bad shape"),
    (BAD, "spmm_update_owned: n_steps must be in [1, 64]"),
    (BAD, "spmm_update_owned: n_steps must be in [1, 64]"),
    (BAD, "spmm_update_owned: chunk must be a positive multiple of 64"),
    (BAD, "spmm_update_owned: block_threads must be a multiple of 64 in [64, 1024]"),
    (BAD, "spmm_update_owned: block_threads must be a multiple of 64 in [64, 1024]"),
    (BAD, "spmm_update_owned: leading dimension < d"),
    (BAD, "spmm_update_owned: negative max_batch_vrows"),
    (BAD, "spmm_update_owned: null pointer"),
    (BAD, "spmm_update_owned: Z_new must not alias Z_old"),
    (BAD, "spmm_update_owned: no instance for d=8 with these operands (16-byte packs, 17..64 packs per row)"),
    (BAD, "spmm_update_owned: no instance for d=128 with these operands (16-byte packs, 17..64 packs per row)"),
    (BAD, "spmm_update_owned: 400 virtual rows per batch need 204800 bytes of LDS"),
    (BAD, "spmm_update_owned: no instance with 5 row loads in flight"),
    (BAD, "spmm_update_owned: no instance with 6 row loads in flight"),
    (OK, None),
    (BAD, "spmm_update_owned: chunk must be a positive multiple of 64"),
    (BAD, "spmm_update_owned: n_steps must be in [1, 64]"),
    (BAD, "spmm_update_tiles: " + TILES_TEXT + " (d=136 tile_cols=128)"),
    (BAD, "spmm_update_tiles: " + TILES_TEXT + " (d=8 tile_cols=16)"),
    (BAD, "spmm_update_tiles: " + TILES_TEXT + " (d=8 tile_cols=0)"),
    (BAD, "spmm_update_tiles: " + TILES_TEXT + " (d=16 tile_cols=6)"),
    (BAD, "spmm_update_tiles: the tiles' partials overlap"),
    (BAD, "spmm_update_tiles: leading dimension < d"),
    (BAD, "spmm_update_tiles: Z_new must not alias Z_old (Jacobi sweep)"),
    (BAD, "spmm_update_tiles: null pointer"),
    (BAD, "spmm_update_tiles: null delta_partials"),
    (BAD, "spmm_update_tiles: bad shape nrows=-1 row0=0 d=256"),
    (BAD, "spmm_update_tiles: negative long_threshold"),
    (BAD, "spmm_update_tiles: the tables must allow 16-byte packs"),
    (OK, None),
    (BAD, "spmm_update_tiles: the tiles' partials overlap"),
    (BAD, "spmm_update_tiles: bad shape nrows=-1 row0=0 d=256"),
    (BAD, "spmm_update_class_tiles: " + TILES_TEXT + " (d=136 tile_cols=128)"),
    (BAD, "spmm_update_class_tiles: " + TILES_TEXT + " (d=8 tile_cols=16)"),
    (BAD, "spmm_update_class_tiles: the tiles' partials overlap"),
    (BAD, "spmm_update_class_tiles: leading dimension < d"),
    (BAD, "spmm_update_class_tiles: Z_new must not alias Z_old"),
    (BAD, "spmm_update_class_tiles: null pointer"),
    (BAD, "spmm_update_class_tiles: bad shape"),
    (BAD, "spmm_update_class_tiles: bad shape"),
    (BAD, "spmm_update_class_tiles: bad shape"),
    (BAD, "spmm_update_class_tiles: grid too large"),
    (BAD, "spmm_update_class_tiles: items_per_block must be in [4, 64]"),
    (BAD, "spmm_update_class_tiles: items_per_block must be in [4, 64]"),
    (BAD, "spmm_update_class_tiles: slab must be 16-byte aligned"),
    (BAD, "spmm_update_class_tiles: the tables must allow 16-byte packs"),
    (OK, None),
    (BAD, "spmm_update_class_tiles: items_per_block must be in [4, 64]"),
    (BAD, "spmm_update_class_tiles: " + TILES_TEXT + " (d=256 tile_cols=512)"),
    (BAD, "spmm_update_owned_tiles: " + TILES_TEXT + ", the partials' stride >= 0 (d=136 tile_cols=128)"),
    (BAD, "spmm_update_owned_tiles: " + TILES_TEXT + ", the partials' stride >= 0 (d=256 tile_cols=512)"),
    (BAD, "spmm_update_owned_tiles: " + TILES_TEXT + ", the partials' stride >= 0 (d=256 tile_cols=128)"),
    (BAD, "spmm_update_owned_tiles: " + TILES_TEXT + ", the partials' stride >= 0 (d=0 tile_cols=128)"),
    (BAD, "spmm_update_owned: null plan"),
    (BAD, "spmm_update_owned: n_steps must be in [1, 64]"),
    (BAD, "spmm_update_owned: chunk must be a positive multiple of 64"),
    (BAD, "spmm_update_owned: block_threads must be a multiple of 64 in [64, 1024]"),
    (BAD, "spmm_update_owned: leading dimension < d"),
    (BAD, "spmm_update_owned: Z_new must not alias Z_old"),
    (BAD, "spmm_update_owned: null pointer"),
    (BAD, "spmm_update_owned: no instance for d=32 with these operands (16-byte packs, 17..64 packs per row)"),
    (BAD, "spmm_update_owned: 400 virtual rows per batch need 204800 bytes of LDS"),
    (BAD, "spmm_update_owned: no instance with 5 row loads in flight"),
    (OK, None),
    (BAD, "spmm_update_owned_tiles: " + TILES_TEXT + ", the partials' stride >= 0 (d=256 tile_cols=512)"),
]


def _run_cases():
    """In the child process: make every call, print [[rc, text], ...] as JSON."""
    sys.path.insert(0, str(ROOT))
    from clane_amd import _hip
    lib = _hip.load_library()
    raw = C.create_string_buffer(8192 + 16)
    base = (C.addressof(raw) + 15) & ~15
    keep = []

    def pointer(v):
        return {"B": base, "B2": base + 4096, "ODD": base + 8, None: None}[v]

    def marshal(name, v):
        if name == "plan" and v is not None:
            arrays = [pointer(v.get(k, "B")) for k in _hip.OWNED_PLAN_ARRAYS]
            keep.append(_hip._OwnedPlanStruct(*arrays, *[v.get(k, PLAN[k]) for k in PLAN]))
            return C.addressof(keep[-1])
        if isinstance(v, tuple) and v[0] == "mirror":
            keep.append(_hip._MirrorStruct(pointer(v[1]), pointer(v[2]), pointer(v[3]), v[4], v[5]))
            return C.addressof(keep[-1])
        return pointer(v) if v is None or isinstance(v, str) else v

    out = []
    for entry, suffix, changes in CASES:
        assert set(changes) <= {n for n, _ in ARGS[entry]}, (entry, changes)
        values = [marshal(n, changes.get(n, default)) for n, default in ARGS[entry]]
        rc = getattr(lib, f"clane_spmm_{entry}_{suffix}")(*values)
        out.append([rc, lib.clane_last_error().decode()])
    print("K3CASES " + json.dumps(out))


@pytest.fixture(scope="module")
def observed():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    run = subprocess.run([sys.executable, "-c", "from tests.test_k3_arguments_host import _run_cases; _run_cases()"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    line, = [l for l in run.stdout.splitlines() if l.startswith("K3CASES ")]
    return [tuple(r) for r in json.loads(line[len("K3CASES "):])]


def test_every_entry_point_and_dtype_is_covered():
    assert {e for e, _, _ in CASES} == set(ARGS) and len(ARGS) == 8
    assert {(e, s) for e, s, _ in CASES if s != "f32"} >= {("update", "bf16"), ("update", "f64"), ("update_long", "f64"),
                                                         ("update_split", "bf16"), ("update_class", "f64"),
                                                         ("update_class", "bf16")}
    assert len(EXPECTED) == len(CASES)


def test_rejected_calls_keep_their_code_and_text(observed):
    assert len(observed) == len(CASES)
    wrong = [(case, got, want) for case, got, want in zip(CASES, observed, EXPECTED)
             if got[0] != want[0] or (want[0] != OK and got[1] != want[1])]
    assert not wrong, wrong


def test_no_case_reaches_a_launch():
    """CLANE_ERR_LAUNCH (-2) would mean a call got past its checks; the early CLANE_OK cases are the zero-count ones."""
    assert all(rc in (BAD, OK) for rc, _ in EXPECTED)
    early = [c for c, (rc, _) in zip(CASES, EXPECTED) if rc == OK]
    assert len(early) >= 8 and all(
        0 in (ch.get("nrows"), ch.get("n_long"), ch.get("n_split"), ch.get("n_rows"), (ch.get("plan") or {}).get("n_groups"))
        for _, _, ch in early)
