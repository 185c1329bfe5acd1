"""SweepEngine's fused column-tile plan without a GPU, through the CPU double of tests/fused_tiles_oracle_kernels.py: one
call per pass instead of one per tile, the same results as the per-tile plan, and the engines that must keep the
per-tile plan (non-uniform tiles, bf16, mirrored launches, a backend without the calls)."""
import collections

import numpy as np
import pytest
import torch

from clane_amd import xcd
from clane_amd.engine import SweepEngine

from . import fused_tiles_cases as F
from .engine_exact_cases import load_P
from .fused_tiles_oracle_kernels import OracleKernels
from .owned_oracle_kernels import OracleKernels as NoTilesKernels

DEV = "cpu"
D, T = 256, 2


def engine(fused, d=D, tiles=T, k=None, case=F.integer_case, **more):
    X, Z0, P = case(d)[:3]
    return F.make_engine(k if k is not None else OracleKernels(), DEV, d, tiles, X, Z0, P, fused_tiles=fused, **more)


def bound_calls(eng):
    """Names of the K3 calls of one sweep's plan, counted."""
    eng.k.bound.clear()
    eng._plans = {}
    eng.sweep(1.0)
    return collections.Counter(n for n in eng.k.bound if n.startswith("spmm_"))


def test_the_default_is_what_xcd_says_and_switches_per_pass():
    eng = engine(None)
    assert eng.fused_possible and eng.fused_tiles == frozenset(xcd.FUSED_TILES_DEFAULT)
    assert engine(True).fused_tiles == {"row", "class", "owned"} and engine(False).fused_tiles == frozenset()
    assert engine(("row",)).fused_tiles == {"row"}
    with pytest.raises(ValueError):
        engine(("rows",))
    assert "fused_tiles" not in engine(False).kernel_config()
    assert engine(True).kernel_config()["fused_tiles"] == ["class", "owned", "row"]
    assert engine(("owned",)).kernel_config()["fused_tiles"] == ["owned"]


@pytest.mark.parametrize("d,tiles", [(256, 2), (384, 3)])
def test_the_fused_plan_holds_one_call_per_pass(d, tiles):
    per_tile, fused = bound_calls(engine(False, d, tiles)), bound_calls(engine(True, d, tiles))
    assert per_tile == {"spmm_update": tiles, "spmm_update_owned": tiles, "spmm_update_class": tiles}
    assert fused == {"spmm_update_tiles": 1, "spmm_update_owned_tiles": 1, "spmm_update_class_tiles": 1}
    mixed = bound_calls(engine(("row", "owned"), d, tiles))
    assert mixed == {"spmm_update_tiles": 1, "spmm_update_owned_tiles": 1, "spmm_update_class": tiles}


def test_event_marks_keep_their_order():
    eng = engine(True)
    per_block, _ = eng._build_plan(0, 1, 0, 1.0)
    marks = [s[2] for s in per_block[0] if s[0] == "event"]
    assert marks == [0, 4, 1, 2, 3]
    kinds = [s[0] for s in per_block[0]]
    assert kinds[kinds.index("event") + 1] == "call" and kinds[-1] == "event"       # class pass after 0, row pass before 3


@pytest.mark.parametrize("d,tiles,chunks", [(256, 2, 1), (384, 3, 1), (200, 2, 1), (256, 2, 3)])
def test_integer_sweep_is_exact_and_equal_to_the_per_tile_plan(d, tiles, chunks):
    more = dict(chunks=chunks) if chunks > 1 else {}
    _, _, _, Z1, delta = F.integer_case(d)
    on, off = engine(True, d, tiles, **more), engine(False, d, tiles, **more)
    assert on.fused_tiles and not off.fused_tiles and len(on.blocks) == chunks
    assert on.sweep(1.0) == off.sweep(1.0) == delta
    assert torch.equal(on.get_Z(), Z1) and torch.equal(on.Zcur, off.Zcur)
    assert torch.equal(on.partials, off.partials)                   # every delta partial where the per-tile plan puts it
    assert bool((on.Zcur[:, d:] == 0).all())


def test_three_gaussian_sweeps_equal_the_per_tile_plan():
    X, Z0, P, _, _, gamma = F.gaussian_case(D)
    on, off = (F.make_engine(OracleKernels(), DEV, D, T, X, Z0, P, fused_tiles=f) for f in (True, False))
    for _ in range(3):
        assert on.sweep(gamma) == off.sweep(gamma)
    assert torch.equal(on.Zcur, off.Zcur)


def test_set_fused_tiles_replans_one_engine():
    eng = engine(False)
    assert bound_calls(eng)["spmm_update"] == T
    eng.set_fused_tiles(True)
    assert bound_calls(eng) == {"spmm_update_tiles": 1, "spmm_update_owned_tiles": 1, "spmm_update_class_tiles": 1}
    eng.set_fused_tiles(("class",))
    assert bound_calls(eng) == {"spmm_update": T, "spmm_update_owned": T, "spmm_update_class_tiles": 1}
    eng.set_fused_tiles(False)
    assert bound_calls(eng)["spmm_update"] == T and not eng.fused_tiles


def test_the_slab_holds_every_tiles_chunk_sums():
    on = engine(True)
    need = T * on.k.spmm_class_slab_len(max(on.class_slots), on.d_plan)
    assert all(s.numel() >= need for s in on.slabs)
    assert all(s.numel() < need for s in engine(False, k=NoTilesKernels()).slabs)     # nobody pays without the calls


def test_engines_the_fused_calls_do_not_apply_to_keep_the_per_tile_plan():
    X, Z0, P = F.integer_case(300)[:3]
    ragged = F.make_engine(OracleKernels(), DEV, 300, 2, X, Z0, P, fused_tiles=True)     # 38 + 37 packs: 152 / 148 columns
    assert [c1 - c0 for c0, c1 in ragged.tiles] == [152, 148]
    assert not ragged.fused_possible and not ragged.fused_tiles
    assert bound_calls(ragged)["spmm_update"] == 2
    X, Z0, P = F.integer_case(D)[:3]
    bf16 = SweepEngine(F.csr(), X.bfloat16(), DEV, OracleKernels(), column_tiles=2, class_threshold=64,
                       hot_rows_first=False, fused_tiles=True)
    assert len(bf16.tiles) == 2 and not bf16.fused_possible and not bf16.fused_tiles
    bf16.set_Z(Z0.bfloat16())
    load_P(bf16, P)
    assert bound_calls(bf16)["spmm_update"] == 2 and "spmm_update_tiles" not in bf16.k.bound
    one_tile = engine(True, tiles=1)
    assert not one_tile.fused_possible and bound_calls(one_tile)["spmm_update"] == 1
    no_calls = engine(True, k=NoTilesKernels())
    assert not no_calls.fused_possible and not no_calls.fused_tiles
    no_calls.set_fused_tiles(True)                                                  # never raises: stays per tile
    assert not no_calls.fused_tiles and no_calls.sweep(1.0) == F.integer_case(D)[4]


def test_mirrored_engines_keep_the_per_tile_plan():
    """Mirrors come with a row division, which has no column tiles: whatever is asked, nothing is fused."""
    from .engine_exact_cases import run_ranks
    X, Z0, P = F.integer_case(128)[:3]

    def rank(_, comm):
        eng = SweepEngine(F.csr(), X, DEV, OracleKernels(), comm=comm, exchange="halo", class_threshold=64,
                          fused_tiles=True)
        return eng.fused_possible, bool(eng.fused_tiles), any(m is not None for m in eng.mirrors)
    results = run_ranks(2, rank, DEV)
    assert all(r == (False, False, True) for r in results)


def test_ragged_last_tile_cuts():
    k = OracleKernels()
    assert k.has_spmm_tiles(torch.float32, 200, 128) and k.has_spmm_tiles(torch.float32, 198, 128)
    assert not k.has_spmm_tiles(torch.float32, 136, 128)            # a last tile of 8 columns: 8 lanes per row, not 32
    assert not k.has_spmm_tiles(torch.float32, 256, 126) and not k.has_spmm_tiles(torch.bfloat16, 256, 128)
    assert F.tile_cuts(200, 128) == [(0, 128), (128, 200)]
    assert np.array_equal(np.diff(F.graph()[0])[:13], F.ROW_PASS + F.OWNED + F.CHUNKED)
