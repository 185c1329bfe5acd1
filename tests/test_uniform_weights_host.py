"""SweepEngine(uniform_weights=...) through the CPU double of tests/uniform_weight_cases.py: when the rows of P are looked
at, when the answer is read, which calls a sweep binds, what switches it back to the per-edge calls -- and the pieces that
need no kernel: the numpy mirror of the detection, an owned plan's seg_row, the binding of the new entry points."""
import numpy as np
import pytest
import torch

from clane_amd import _hip, xcd
from clane_amd.engine import SweepEngine
from clane_amd.partition import HostCSR

from . import uniform_weight_cases as U
from .engine_exact_cases import no_infinity_cache
from .oracle_kernels import OracleKernels as PlainDouble

CPU = "cpu"


def engine(P=None, mode="auto", d=256, tiles=2, kernels=None, **more):
    k = U.UniformOracleKernels() if kernels is None else kernels
    return U.make_engine(k, CPU, d, tiles, U.P_one_over_deg() if P is None else P, mode, **more), k


def test_default_looks_at_the_rows_and_off_costs_nothing():
    assert xcd.UNIFORM_WEIGHTS_DEFAULT == "auto"
    eng, k = engine(mode=None)                             # a table that fits the Infinity Cache: off
    assert not eng.beyond_cache and eng.uniform_weights is False and eng.uniform_possible
    eng.sweep(U.GAMMA)
    assert k.scans == 0 and "uniform_weights" not in eng.kernel_config()
    with no_infinity_cache():                              # ... and one far beyond it: looked at
        eng, k = engine(mode=None)
    assert eng.beyond_cache and eng.uniform_weights == "auto"
    eng.sweep(U.GAMMA)
    assert k.scans == 1 and eng.kernel_config()["uniform_weights"] is True
    eng, k = engine(mode=False)
    eng.sweep(U.GAMMA)
    assert k.scans == 0 and not any(m.endswith("_rw") for m in k.bound) and "uniform_weights" not in eng.kernel_config()


@pytest.mark.parametrize("d,tiles", U.WIDTHS)
@pytest.mark.parametrize("chunks", [1, 3])
def test_uniform_rows_bind_the_rw_calls_on_the_engines_own_weights(d, tiles, chunks):
    for P in (U.P_one_over_deg(), U.P_any_float_per_row()):
        eng, _ = engine(P, d=d, tiles=tiles, chunks=chunks)
        U.assert_every_pass_runs(eng)
        assert len(eng.blocks) == chunks
        on = U.sweep_from_start(eng, d, P, True)
        auto = U.sweep_from_start(eng, d, P, "auto")
        assert eng.kernel_config()["uniform_weights"] is True
        off = U.sweep_from_start(eng, d, P, False)
        assert "uniform_weights" not in eng.kernel_config()
        assert U.k3_calls(on[3]) == U.k3_calls(auto[3]) == U.rw_calls(tiles)
        assert not any(m.endswith("_rw") for m in off[3]) and len(U.k3_calls(off[3])) == 3
        assert U.same(on, off) and U.same(auto, off)


def test_one_ulp_on_one_edge_is_found():
    P = U.one_ulp_off(U.P_one_over_deg())
    eng, k = engine(P)
    assert eng._uniform is None and k.scans == 0           # nothing is launched or read until a sweep asks
    run = U.sweep_from_start(eng, 256, P, "auto")
    assert eng._uniform is False and not any(m.endswith("_rw") for m in run[3])
    with pytest.raises(ValueError, match="different weights"):
        U.sweep_from_start(eng, 256, P, True)
    for row in np.nonzero(U.graph()[2] > 1)[0][:3]:        # whichever pass owns the row
        eng2, _ = engine(U.one_ulp_off(U.P_one_over_deg(), int(row)))
        eng2.sweep(U.GAMMA)
        assert eng2._uniform is False


def test_row_weights_equal_the_numpy_mirror():
    for P, mixed in ((U.P_any_float_per_row(), 0), (U.one_ulp_off(U.P_any_float_per_row()), 1)):
        eng, _ = engine(P)
        assert eng._resolve_uniform() == (mixed == 0)
        w, m = U.numpy_row_weights(eng.P[:eng.E_loc].numpy(), eng.rowptr.numpy())
        assert m == mixed == int(eng._w_mixed) and np.array_equal(w.view(np.uint32), eng.row_w.numpy().view(np.uint32))
        assert bool((eng.row_w[torch.from_numpy(np.diff(eng.local.rowptr) == 0)] == 0).all())


def test_a_new_P_is_looked_at_again_and_the_answer_read_once():
    P = U.P_one_over_deg()
    eng, k = engine(P)
    for _ in range(3):
        eng.sweep(U.GAMMA)
    assert eng._uniform is True and k.scans == 1
    U.load_P(eng, U.one_ulp_off(P))                        # what a plug-in similarity does: write P, set P_valid
    assert eng._uniform is None and k.scans == 1           # forgotten, not yet looked at again
    k.bound.clear()
    eng.sweep(U.GAMMA)
    assert eng._uniform is False and k.bound and not any(m.endswith("_rw") for m in k.bound)
    U.load_P(eng, P)
    k.bound.clear()
    eng.sweep(U.GAMMA)
    assert eng._uniform is True and not k.bound            # the plan of the first sweeps, kept under its key


def test_build_P_looks_at_its_rows():
    eng, k = engine()
    eng.set_Z(U.tables(256)[1])
    assert not eng.P_valid and eng._uniform is None
    eng.build_P()
    assert eng.P_valid and k.scans == 0
    assert "uniform_weights" not in eng.kernel_config() and k.scans == 1     # kernel_config() asks when no sweep has
    eng.sweep(U.GAMMA)
    assert eng._uniform is False and k.scans == 1                           # 1 300 vertices: the scores are far from 1e-9


def test_engines_that_cannot_take_it_keep_the_per_edge_calls():
    rowptr, colidx, _ = U.graph()
    X = U.tables(128)[0]
    lacking = SweepEngine(HostCSR(U.V, rowptr, colidx), X, CPU, PlainDouble(), uniform_weights="auto")
    assert lacking.uniform_weights is False and not lacking.uniform_possible
    bf16 = SweepEngine(HostCSR(U.V, rowptr, colidx), X.bfloat16(), CPU, U.UniformOracleKernels(), uniform_weights="auto")
    assert bf16.uniform_weights is False
    with pytest.raises(ValueError, match="uniform_weights=True"):
        SweepEngine(HostCSR(U.V, rowptr, colidx), X.double(), CPU, U.UniformOracleKernels(), uniform_weights=True)
    with pytest.raises(ValueError, match="uniform_weights must be"):
        SweepEngine(HostCSR(U.V, rowptr, colidx), X, CPU, U.UniformOracleKernels(), uniform_weights="yes")


def test_long_rows_keep_their_per_edge_call():
    eng, k = engine(d=130, tiles=1, class_threshold=0, class_owned=False, long_threshold=48, hub_threshold=128)
    assert eng.mid_rows[0] is not None and eng.hub_rows[0] is not None
    eng.sweep(U.GAMMA)
    assert eng._uniform is True and U.k3_calls(k.bound) == ["spmm_update_long", "spmm_update_rw"]


def test_seg_row_of_an_owned_plan():
    eng, _ = engine()
    plans = [r.owned.plan for r in eng.block_rows if r.owned is not None]
    assert plans
    for plan in plans:
        on_device = _hip.OwnedPlan(plan, plan["chunk"], CPU)
        want = U.segment_rows_by_search(plan)
        assert want.size > 50 and np.array_equal(on_device.seg_row.numpy(), want)
        assert int(want.max()) <= on_device.max_row


def test_the_new_entry_points_validate_before_any_launch():
    lib = _hip.load_library()
    rc = lib.clane_row_weight_f32(None, None, 4, None, None, None)
    assert rc == -1 and b"null mixed" in lib.clane_last_error()
    rc = lib.clane_spmm_update_rw_f32(None, None, None, 4, 0, None, 8, None, 8, 0.5, None, 8, 8, 0, 0, None, None)
    assert rc == -1 and b"delta_partials" in lib.clane_last_error()
