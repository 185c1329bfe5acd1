"""One weight per row instead of one per edge on the card: the spmm_update*_rw kernels (csrc/spmm_update.h, UNIFORM) and
row_weight_kernel (csrc/build_p.h) against the per-edge kernels on the same engine, on the graph of
tests/uniform_weight_cases.py -- out-degrees 0, 1, 3, 4, 5, 31, 32 (row pass), 33, 64, 65 (owned, whole rows), 200, 513
(owned, virtual rows), 600, 1 100 (chunk + combine) -- at d = 66 (a sub-wave per row), 128, 130 and 256 in two tiles of
128 (fused and per tile), both values of the cache hint, one launch block and three.  Everything is torch.equal: Z_new,
every delta partial, the delta.  tests/test_uniform_weights_host.py runs the engine's side through the CPU double."""
import numpy as np
import pytest
import torch

from clane_amd import _hip

from . import uniform_weight_cases as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


def engine(k, dev, P, d=256, tiles=2, mode="auto", **more):
    return U.make_engine(k, dev, d, tiles, P, mode, **more)


@pytest.mark.parametrize("chunks", [1, 3], ids=["one_block", "three_blocks"])
@pytest.mark.parametrize("beyond", [False, True], ids=["cached", "beyond_cache"])
@pytest.mark.parametrize("d,tiles,fused", [(d, t, True) for d, t in U.WIDTHS] + [(256, 2, False)])
def test_per_row_weights_change_no_bit(k, dev, d, tiles, fused, beyond, chunks):
    for P in (U.P_one_over_deg(), U.P_any_float_per_row()):
        eng = engine(k, dev, P, d, tiles, beyond=beyond, chunks=chunks, fused_tiles=fused)
        U.assert_every_pass_runs(eng)
        assert len(eng.blocks) == chunks and eng.beyond_cache == beyond and bool(eng.fused_tiles) == (fused and tiles > 1)
        on = U.sweep_from_start(eng, d, P, True)
        assert eng._uniform is True and U.k3_calls(on[3]) == U.rw_calls(tiles, fused)
        auto = U.sweep_from_start(eng, d, P, "auto")
        assert eng._uniform is True and U.k3_calls(auto[3]) == U.rw_calls(tiles, fused)
        off = U.sweep_from_start(eng, d, P, False)
        assert not any(m.endswith("_rw") for m in off[3]) and len(U.k3_calls(off[3])) == 3
        assert U.same(on, off) and U.same(auto, off)
        assert float(on[2]) > 0 and bool((on[0][:, d:] == 0).all())
        for _ in range(2):                                                   # and over consecutive sweeps
            eng.sweep(U.GAMMA)
        got = (eng.Zcur.clone(), eng.partials.clone())
        eng.set_uniform_weights(True)
        eng.set_Z(U.tables(d)[1])
        U.load_P(eng, P)
        for _ in range(3):
            eng.sweep(U.GAMMA)
        assert eng._uniform is True and torch.equal(eng.Zcur, got[0]) and torch.equal(eng.partials, got[1])


@pytest.mark.parametrize("acc", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_row_weights_equal_the_numpy_mirror(k, dev, acc):
    rowptr, _, deg = U.graph()
    rp = torch.from_numpy(rowptr).to(dev)
    for P, mixed in ((U.P_one_over_deg(), 0), (U.P_any_float_per_row(), 0), (U.one_ulp_off(U.P_one_over_deg()), 1),
                     (U.one_ulp_off(U.P_any_float_per_row(), int(np.nonzero(deg == 3)[0][0])), 1)):
        P = P.to(acc)
        w = torch.full((U.V,), 7.0, dtype=acc, device=dev)
        flag = torch.full((1,), 5, dtype=torch.int32, device=dev)
        k.row_weight(rp, P.to(dev), U.V, w, flag)
        want, m = U.numpy_row_weights(P.numpy(), rowptr)
        assert m == mixed == int(flag.item())
        bits = np.uint32 if acc == torch.float32 else np.uint64
        assert np.array_equal(w.cpu().numpy().view(bits), want.view(bits))
    zero = torch.zeros(1, dtype=acc, device=dev)
    w = torch.full((U.V,), 7.0, dtype=acc, device=dev)
    flag = torch.full((1,), 5, dtype=torch.int32, device=dev)
    k.row_weight(torch.zeros(U.V + 1, dtype=torch.int64, device=dev), zero, U.V, w, flag)     # no edges at all
    assert int(flag.item()) == 0 and bool((w == 0).all())


def test_rows_of_thousands_of_edges_beside_short_and_empty_ones(k, dev):
    """One workgroup's rows of 9 000, 5 000, 2 049 ... 1 and 0 edges: uniform, and one ulp off on the last edge of one of
    them (many trips of a wave's loop over a row, and a tail that is no multiple of 64)."""
    deg = np.array([3, 5000, 0, 2049, 2048, 70, 9000] + [1] * 40)
    rowptr = np.zeros(deg.size + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    base = torch.randn(deg.size, generator=torch.Generator().manual_seed(9))[torch.from_numpy(np.repeat(np.arange(deg.size), deg))]
    rp = torch.from_numpy(rowptr).to(dev)
    for off_row in (None, 1, 3, 4, 6):
        P = base.clone()
        if off_row is not None:
            e = int(rowptr[off_row + 1]) - 1
            P[e] = torch.nextafter(P[e], torch.tensor(float("inf")))
        w = torch.full((deg.size,), 7.0, device=dev)
        flag = torch.full((1,), 5, dtype=torch.int32, device=dev)
        k.row_weight(rp, P.to(dev), deg.size, w, flag)
        want, m = U.numpy_row_weights(P.numpy(), rowptr)
        assert m == int(off_row is not None) == int(flag.item()), off_row
        assert np.array_equal(w.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_one_ulp_on_one_edge_takes_the_per_edge_calls(k, dev):
    P = U.one_ulp_off(U.P_one_over_deg())
    eng = engine(k, dev, P)
    run = U.sweep_from_start(eng, 256, P, "auto")
    assert eng._uniform is False and not any(m.endswith("_rw") for m in run[3])
    with pytest.raises(ValueError, match="different weights"):
        U.sweep_from_start(eng, 256, P, True)
    assert U.same(run, U.sweep_from_start(eng, 256, P, False))


def test_a_mixed_P_after_a_uniform_one_is_per_edge_again(k, dev):
    P, Q = U.P_one_over_deg(), U.one_ulp_off(U.P_any_float_per_row())
    eng = engine(k, dev, P)
    eng.sweep(U.GAMMA)
    assert eng._uniform is True
    want = U.sweep_from_start(engine(k, dev, Q, mode=False), 256, Q, False)
    got = U.sweep_from_start(eng, 256, Q, "auto")
    assert eng._uniform is False and not any(m.endswith("_rw") for m in got[3]) and U.same(got, want)


def test_the_comparison_fails_on_a_neighbours_weight_and_on_stale_weights(k, dev):
    """Self-checks: a kernel that took row r + 1's weight for row r, and an engine that kept the weights of the P before
    this one, are both told apart by the comparisons above."""
    P = U.P_any_float_per_row()
    eng = engine(k, dev, P)
    want = U.sweep_from_start(eng, 256, P, False)
    assert U.same(U.sweep_from_start(eng, 256, P, "auto"), want)
    eng.set_Z(U.tables(256)[1])
    U.load_P(eng, P)
    assert eng._resolve_uniform() is True                                    # the rows are looked at here, not again below
    eng.row_w.copy_(torch.roll(eng.row_w, -1))                               # every row reads its neighbour's weight
    eng.sweep(U.GAMMA)
    assert eng._uniform is True and not torch.equal(eng.Zcur, want[0]) and not torch.equal(eng.partials, want[1])
    Q = U.P_any_float_per_row(seed=6)
    want = U.sweep_from_start(eng, 256, Q, False)
    eng.set_uniform_weights("auto")
    eng.set_Z(U.tables(256)[1])
    U.load_P(eng, P)                                                         # row_w: P's
    eng.sweep(U.GAMMA)
    assert eng._uniform is True
    eng.set_Z(U.tables(256)[1])
    eng.P[:eng.E_loc] = Q[torch.from_numpy(eng.local.edge_origin)].to(eng.device)    # ... Q written, and nobody told:
    eng._P_valid = True                                                      # the flag set behind the property's back
    eng._uniform = True
    eng.sweep(U.GAMMA)
    assert not torch.equal(eng.Zcur, want[0])


def test_misuse_is_refused_before_any_launch(k, dev):
    eng = engine(k, dev, U.P_one_over_deg(), d=128, tiles=1)
    assert eng._resolve_uniform() is True
    b = eng.blocks[0]
    Zn = torch.full_like(eng.Zcur, 7.0)
    short = eng.row_w[:b.nrows - 1]
    with pytest.raises(ValueError, match="row_weight holds"):
        k.spmm_update_rw(eng.rowptr, eng.colidx, short, b.nrows, 0, eng.Zcur, eng.X_loc, 1.0, Zn, 128, eng.long_threshold,
                         eng.partials)
    with pytest.raises(_hip.ClaneHipError, match="item_row"):                # the library's own check
        it = eng.block_rows[0].owned.rest
        k._check(k.lib.clane_spmm_update_class_rw_f32(
            eng.colidx.data_ptr(), eng.row_w.data_ptr(), it.e0.data_ptr(), it.len.data_ptr(), it.slot.data_ptr(), None,
            it.e0.numel() // it.items_per_block, it.items_per_block, it.rows.data_ptr(), it.slot_ptr.data_ptr(),
            it.rows.numel(), 0, eng.Zcur.data_ptr(), eng.ld, eng.X_loc.data_ptr(), eng.ld, 1.0, Zn.data_ptr(), eng.ld, 128, 0,
            eng.slabs[0].data_ptr(), eng.partials.data_ptr(), None), "clane_spmm_update_class_rw")
    torch.cuda.synchronize()
    assert bool((Zn == 7.0).all())                                           # nothing ran
