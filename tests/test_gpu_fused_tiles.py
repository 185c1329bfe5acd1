"""Every column tile of a K3 pass in one launch (clane_spmm_update_tiles_f32 / _class_tiles_f32 / _owned_tiles_f32) against
the per-tile launches on the same inputs, on the graph of tests/fused_tiles_cases.py: out-degrees 0, 1, 3, 4, 5, 63, 64
(row pass), 65, 200, 512 (owned), 513, 900 (chunk + combine beside the owned rows), one row of 5 000 edges (phased, many
slots).  Widths: two tiles of 128 columns, three tiles, d = 200 in tiles of 128 (a last tile of 72 columns) and d = 198
(a ragged last pack: the pad columns stay zero).  Both values of the cache hint, one launch block and three (row0 > 0),
a chunk-block count that is no multiple of 8, the owned epilogue with and without its look-ahead.  Everything is
compared with torch.equal: Z_new, every delta partial where the per-tile call puts it, the reduced delta; integer data is
also checked exactly against the CPU reference.  tests/test_fused_tiles_host.py runs the engine-level cases through the
CPU double first."""
import functools

import pytest
import torch

from clane_amd import _hip

from . import fused_tiles_cases as F

pytestmark = pytest.mark.gpu
PAD = 5                             # the tiles' partials are PAD slots apart beyond their length: a dropped stride shows


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


@functools.lru_cache(maxsize=None)
def engine_for(d, chunks, gaussian):
    """A per-tile engine that only lends its structure (CSR on the device, row lists, class items, owned plan, partial
    layout) and its tables to the backend-level calls below."""
    case = F.gaussian_case(d) if gaussian else F.integer_case(d)
    more = dict(chunks=chunks) if chunks > 1 else {}
    return F.make_engine(_hip.kernels(), "cuda:0", d, 2, case[0], case[1], case[2], fused_tiles=False, **more)


def padded_items(items, extra_blocks=3):
    """The class items with `extra_blocks` empty item blocks appended: a block count that is no multiple of 8."""
    n = extra_blocks * items.items_per_block
    dev = items.e0.device
    return items._replace(e0=torch.cat([items.e0, torch.zeros(n, dtype=torch.int64, device=dev)]),
                          len=torch.cat([items.len, torch.zeros(n, dtype=torch.int32, device=dev)]),
                          slot=torch.cat([items.slot, torch.full((n,), -1, dtype=torch.int32, device=dev)]))


def run_passes(k, eng, d, tile_cols, gamma, beyond, fused, ahead=False, mutate=None):
    """The row pass, the owned pass and chunk + combine of every block of `eng`, per tile or fused, into a fresh table
    and fresh partials laid out [tile][block layout] with tiles L + PAD apart.  `mutate` breaks the PER-TILE side the way a
    fused kernel could be wrong: "stride" puts every tile's partials where tile 0's are, "offset" lets every tile read X
    at tile 0's columns."""
    cuts = F.tile_cuts(d, tile_cols)
    L = eng.partial_off[-1]
    stride = L + PAD
    Zold, Zn = eng.Zcur, torch.zeros_like(eng.Zcur)
    partials = torch.full((len(cuts) * stride,), -1.0, dtype=torch.float64, device=eng.device)
    slab = torch.zeros(len(cuts) * max(s.numel() for s in eng.slabs) + 64, dtype=torch.float32, device=eng.device)
    for i, (b, rows) in enumerate(zip(eng.blocks, eng.block_rows)):
        rp, Xb, Znb = eng.rowptr[b.local_start:], eng.X_loc[eng._rows(b)], eng._zrows(Zn, b)
        po, lay = eng.partial_off[i], rows.partials
        rest = padded_items(rows.owned.rest) if rows.owned is not None and rows.owned.rest is not None else None
        if fused:
            at = lambda start: partials[po + start:]                                              # noqa: E731
            k.spmm_update_tiles(rp, eng.colidx, eng.P, b.nrows, b.row0, Zold, Xb, gamma, Znb, d, tile_cols,
                                eng.long_threshold, at(lay.main), stride, sinks_untouched=True, beyond_cache=beyond)
            if rows.owned is not None:
                k.spmm_update_owned_tiles(eng.colidx, eng.P, rows.owned.plan, eng.owned_block_threads, b.row0, Zold, Xb,
                                          gamma, Znb, d, tile_cols, at(lay.klass), stride, beyond_cache=beyond,
                                          loads=eng.owned_loads, ahead=ahead)
            if rest is not None:
                k.spmm_update_class_tiles(eng.colidx, eng.P, rest.e0, rest.len, rest.slot, rest.items_per_block,
                                          rest.rows, rest.slot_ptr, int(rest.slot_ptr[-1]), b.row0, Zold, Xb, gamma, Znb,
                                          d, tile_cols, slab, at(lay.klass), stride, beyond_cache=beyond)
            continue
        for t, (c0, c1) in enumerate(cuts):
            cut = lambda M: M[:, c0:c1]                                                           # noqa: E731
            xcut = (lambda M: M[:, :c1 - c0]) if mutate == "offset" else cut
            at = lambda start: partials[(0 if mutate == "stride" else t * stride) + po + start:]  # noqa: E731
            k.spmm_update(rp, eng.colidx, eng.P, b.nrows, b.row0, cut(Zold), xcut(Xb), gamma, cut(Znb), c1 - c0,
                          eng.long_threshold, at(lay.main), sinks_untouched=True, beyond_cache=beyond)
            if rows.owned is not None:
                k.spmm_update_owned(eng.colidx, eng.P, rows.owned.plan, eng.owned_block_threads, b.row0, cut(Zold),
                                    xcut(Xb), gamma, cut(Znb), c1 - c0, at(lay.klass), beyond_cache=beyond,
                                    loads=eng.owned_loads, ahead=ahead)
            if rest is not None:
                k.spmm_update_class(eng.colidx, eng.P, rest.e0, rest.len, rest.slot, rest.items_per_block, rest.rows,
                                    rest.slot_ptr, b.row0, cut(Zold), xcut(Xb), gamma, cut(Znb), c1 - c0, slab, at(lay.klass),
                                    beyond_cache=beyond)
    delta = torch.zeros(1, dtype=torch.float64, device=eng.device)
    k.reduce_partials(partials.clamp_min(0.0), partials.numel(), eng.ws, delta)
    torch.cuda.synchronize()
    return Zn, partials, delta


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("gaussian", [False, True], ids=["integers", "gaussian"])
@pytest.mark.parametrize("chunks", [1, 3], ids=["one_block", "three_blocks"])
@pytest.mark.parametrize("d,tile_cols", F.WIDTHS)
def test_fused_calls_equal_the_per_tile_calls(k, dev, d, tile_cols, chunks, gaussian):
    eng = engine_for(d, chunks, gaussian)
    gamma = 0.7 if gaussian else 1.0
    assert len(eng.blocks) == chunks and (chunks == 1 or all(b.row0 > 0 for b in eng.blocks[1:]))
    rows = eng.block_rows[0]
    assert rows.owned is not None and rows.owned.rest is not None
    blocks = padded_items(rows.owned.rest).e0.numel() // rows.owned.rest.items_per_block
    assert blocks % 8 == 3 and k.has_spmm_tiles(torch.float32, d, tile_cols)
    for beyond in (False, True):
        want = run_passes(k, eng, d, tile_cols, gamma, beyond, fused=False)
        assert same(run_passes(k, eng, d, tile_cols, gamma, beyond, fused=True), want), beyond
        assert same(run_passes(k, eng, d, tile_cols, gamma, beyond, fused=True, ahead=True), want), beyond
        assert same(run_passes(k, eng, d, tile_cols, gamma, beyond, fused=False, ahead=True), want), beyond
    Zn, partials, _ = want
    assert bool((Zn[:, d:] == 0).all())                                     # the pad columns of a ragged last pack
    L = eng.partial_off[-1]
    gaps = partials.view(-1, L + PAD)[:, L:]
    assert bool((gaps == -1.0).all())                                       # nothing between the tiles' partials


@pytest.mark.parametrize("d,tile_cols", F.WIDTHS)
def test_integer_rows_are_exact_against_the_cpu_reference(k, dev, d, tile_cols):
    """The rows the three passes own (everything here: no 4- or 16-wave rows at class_threshold = 64), both forms."""
    eng = engine_for(d, 1, False)
    assert all(x is None for x in eng.mid_rows + eng.hub_rows + eng.split_rows)
    X, Z0, P, Z1, delta = F.integer_case(d)
    deg_pos = (torch.from_numpy(F.graph()[0]).diff() > 0)
    for fused in (False, True):
        Zn, _, got = run_passes(k, eng, d, tile_cols, 1.0, True, fused=fused, ahead=fused)
        assert torch.equal(Zn[:F.V, :d].cpu()[deg_pos], Z1[deg_pos]) and float(got) == delta


@pytest.mark.parametrize("mutate", ["stride", "offset"])
def test_the_comparison_fails_when_a_tile_loses_its_stride_or_its_offset(k, dev, mutate):
    """Self-check: a per-tile side that drops what the fused kernels must apply per tile is told apart."""
    eng = engine_for(256, 1, True)
    want = run_passes(k, eng, 256, 128, 0.7, True, fused=True)
    assert same(run_passes(k, eng, 256, 128, 0.7, True, fused=False), want)
    broken = run_passes(k, eng, 256, 128, 0.7, True, fused=False, mutate=mutate)
    assert not torch.equal(broken[1], want[1])
    assert torch.equal(broken[0], want[0]) == (mutate == "stride")


def test_padded_chunk_grid_keeps_every_tiles_blocks_on_their_xcd(k, dev):
    """The chunk grid is tiles x (blocks rounded up to 8): block 8 j + b of EVERY tile lands on the XCD of block b.
    Without the padding (11 blocks per tile) tile 1's blocks land three XCDs further."""
    n_blocks, tiles = 11, 3
    for per_tile, kept in ((16, True), (n_blocks, False)):
        ids = k.xcc_ids(tiles * per_tile, 256, dev).cpu()
        agree = all(bool((ids[t * per_tile:t * per_tile + n_blocks] == ids[:n_blocks]).all()) for t in range(tiles))
        assert agree == kept


def test_bad_tilings_are_refused_before_any_launch(k, dev):
    eng = engine_for(256, 1, False)
    b, rows = eng.blocks[0], eng.block_rows[0]
    Zn = torch.full_like(eng.Zcur, 7.0)
    L = eng.partial_off[-1]
    partials = torch.zeros(2 * L, dtype=torch.float64, device=eng.device)
    args = lambda d, tc, p, s: (eng.rowptr, eng.colidx, eng.P, b.nrows, 0, eng.Zcur, eng.X_loc, 1.0, Zn, d, tc,   # noqa: E731
                                eng.long_threshold, p, s)
    for d, tc, p, s in ((256, 126, partials, L), (136, 128, partials, L), (256, 128, partials, 3), (256, 128, partials[:L], L)):
        with pytest.raises(ValueError):
            k.spmm_update_tiles(*args(d, tc, p, s))
    with pytest.raises(_hip.ClaneHipError):                                # the library's own check of the same rule
        k._check(k.lib.clane_spmm_update_tiles_f32(
            eng.rowptr.data_ptr(), eng.colidx.data_ptr(), eng.P.data_ptr(), b.nrows, 0, eng.Zcur.data_ptr(), eng.ld,
            eng.X_loc.data_ptr(), eng.ld, 1.0, Zn.data_ptr(), eng.ld, 136, 128, eng.long_threshold, 0,
            partials.data_ptr(), L, None), "clane_spmm_update_tiles")
    torch.cuda.synchronize()
    assert bool((Zn == 7.0).all())                                         # nothing ran


@pytest.mark.parametrize("d,tiles,chunks", [(256, 2, 1), (384, 3, 1), (256, 2, 3)])
def test_engine_sweeps_are_bitwise_equal_with_fused_tiles_on_and_off(k, dev, d, tiles, chunks):
    X, Z0, P, _, _, gamma = F.gaussian_case(d)
    more = dict(chunks=chunks) if chunks > 1 else {}
    on = F.make_engine(k, dev, d, tiles, X, Z0, P, fused_tiles=True, owned_ahead=True, **more)
    off = F.make_engine(k, dev, d, tiles, X, Z0, P, fused_tiles=False, owned_ahead=False, **more)
    assert on.fused_tiles == {"row", "class", "owned"} and on.owned_ahead and not off.fused_tiles
    for _ in range(3):
        assert on.sweep(gamma) == off.sweep(gamma)
    assert torch.equal(on.Zcur, off.Zcur) and torch.equal(on.partials, off.partials)
    off.set_fused_tiles(("row", "class"), ahead=True)                       # the same engine switched between sweeps
    assert off.sweep(gamma) == on.sweep(gamma) and torch.equal(on.Zcur, off.Zcur)


@pytest.mark.parametrize("d,tiles", [(256, 2), (200, 2)])
def test_engine_integer_sweep_is_exact_with_fused_tiles(k, dev, d, tiles):
    X, Z0, P, Z1, delta = F.integer_case(d)
    eng = F.make_engine(k, dev, d, tiles, X, Z0, P, fused_tiles=True, owned_ahead=True)
    assert eng.fused_tiles and eng.sweep(1.0) == delta
    assert torch.equal(eng.get_Z(), Z1) and bool((eng.Zcur[:, d:] == 0).all())
