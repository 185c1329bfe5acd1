"""The owned class pass without a GPU: the planner (xcd.owned_plan) checked array by array on the graph of
tests/owned_cases.py, and SweepEngine driving it through the CPU double (tests/owned_oracle_kernels.py)."""
import numpy as np
import pytest
import torch

from clane_amd import xcd

from . import owned_cases as C
from .owned_oracle_kernels import OracleKernels

DEV = "cpu"


@pytest.fixture(scope="module")
def k():
    return OracleKernels()


def engine(k, setting, d=128, tiles=1, **more):
    X, Z0, P, _, _ = C.integer_case(d)
    return C.make_engine(k, DEV, d, tiles, setting, X, Z0, P, **more)


def plan_of(eng):
    (plan, rest, n_rest), = [o for o in eng.owned_rows if o is not None]
    return plan, rest, n_rest


def segments_of(plan):
    """[(group, batch, step, e0, len, virtual row in the plan's numbering)] in launch order."""
    S, out = plan["n_steps"], []
    for g in range(plan["n_groups"]):
        for b in range(plan["grp_bat_ptr"][g], plan["grp_bat_ptr"][g + 1]):
            for s in range(S):
                for i in range(plan["bat_seg_ptr"][b * S + s], plan["bat_seg_ptr"][b * S + s + 1]):
                    out.append((g, b, s, int(plan["seg_e0"][i]), int(plan["seg_len"][i]),
                                int(plan["bat_vrow_ptr"][b] + plan["seg_vrow"][i])))
    return out


@pytest.mark.parametrize("setting", list(C.SETTINGS))
def test_rows_up_to_H_are_owned_once_and_rows_above_never(k, setting):
    eng = engine(k, setting)
    H = C.SETTINGS[setting][0]
    deg = np.diff(eng.local.rowptr)
    plan, rest, n_rest = plan_of(eng)
    owned = np.sort(plan["row_id"])
    assert np.array_equal(owned, np.nonzero((deg > 64) & (deg <= H))[0]) and np.unique(owned).size == owned.size
    above = np.nonzero(deg > H)[0]
    assert n_rest == above.size and (rest is None) == (above.size == 0)
    if rest is not None:
        assert np.array_equal(rest[0].numpy(), above)
    # the delta partials of the class rows: the rows above H first, then one slot per owned row
    assert np.array_equal(np.sort(plan["row_part"]), n_rest + np.arange(owned.size))
    for h in (H, H + 1):
        if h in C.EXACT.values():
            r = next(r for r, n in C.EXACT.items() if n == h)
            assert (r in owned) == (h <= H)


@pytest.mark.parametrize("setting", list(C.SETTINGS))
def test_segments_tile_every_row_in_subclass_order(k, setting):
    eng = engine(k, setting)
    plan, _, _ = plan_of(eng)
    rowptr, colidx = eng.local.rowptr, eng.local.colidx
    deg = np.diff(rowptr)
    v_row = np.repeat(np.arange(plan["row_id"].size), np.diff(plan["row_vptr"]))      # virtual row -> row (plan order)
    by_row = {}
    for g, b, s, e0, ln, v in segments_of(plan):
        by_row.setdefault(int(plan["row_id"][v_row[v]]), []).append((v, s, e0, ln))
    assert sorted(by_row) == sorted(plan["row_id"].tolist())
    for r, segs in by_row.items():
        covered = np.zeros(deg[r], dtype=int)
        for v, s, e0, ln in segs:
            covered[e0 - rowptr[r]:e0 - rowptr[r] + ln] += 1
            cols = colidx[e0:e0 + ln].astype(np.int64)
            key = xcd.xcd_subclass(cols, np.full(ln, deg[r]), 64, eng.phase_threshold, eng.class_phases)
            assert (key == plan["steps"][s]).all()                         # one (phase, class) key per segment: its step
        assert (covered == 1).all(), r                                     # no gap, no overlap
        # inside a virtual row the steps ascend with the edges; a row's virtual rows split every step in order
        for v in {v for v, *_ in segs}:
            mine = sorted((s, e0) for vv, s, e0, _ in segs if vv == v)
            assert [e for _, e in mine] == sorted(e for _, e in mine)
        for s in {s for _, s, *_ in segs}:
            mine = sorted((v, e0, ln) for v, ss, e0, ln in segs if ss == s)
            assert all(a[1] + a[2] == b[1] for a, b in zip(mine, mine[1:]))
    if setting != "H96":
        one = [ln for v, s, e0, ln in by_row[C.ONE_CLASS_ROW]]
        assert max(one) > C.CHUNK                                          # a segment of several pieces
    empty = {int(plan["steps"][s]) % 8 for _, s, *_ in by_row.get(C.EMPTY_CLASS_ROW, [])}
    assert C.EMPTY_CLASS not in empty and (setting == "H96" or len(empty) == 7)


@pytest.mark.parametrize("groups", [8, 16, 24])
def test_virtual_rows_groups_and_batches(k, groups):
    eng = engine(k, "all_phased", owned_groups=groups)
    plan, rest, _ = plan_of(eng)
    assert rest is None and plan["n_steps"] == 16 and plan["n_groups"] == groups
    deg = np.diff(eng.local.rowptr)
    nv = np.diff(plan["row_vptr"])
    d_owned = deg[plan["row_id"]]
    assert (nv[d_owned <= C.ROW_EDGES] == 1).all() and (nv[d_owned > C.ROW_EDGES] >= 2).all()
    assert nv[plan["row_id"] == 12] == 1 and nv[plan["row_id"] == 13] == 2          # 128 and 129 edges
    # no virtual row above owned_row_edges, and as few as that allows up to the rounding of the even cut
    per_v = np.zeros(plan["row_vptr"][-1], dtype=int)
    for g, b, s, e0, ln, v in segments_of(plan):
        per_v[v] += ln
    assert per_v.max() <= C.ROW_EDGES and (nv <= -(-d_owned // C.ROW_EDGES) + 1).all()
    # batches: whole rows, at most BATCH_VROWS virtual rows, consecutive in their group, every group served
    assert plan["max_batch_vrows"] == np.diff(plan["bat_vrow_ptr"]).max() <= C.BATCH_VROWS
    assert np.array_equal(plan["row_vptr"][plan["bat_row_ptr"]], plan["bat_vrow_ptr"])
    assert plan["grp_bat_ptr"][0] == 0 and plan["grp_bat_ptr"][-1] == plan["bat_vrow_ptr"].size - 1
    per_group = np.diff(plan["grp_bat_ptr"])
    assert (per_group >= 1).all() and (groups > 8 or per_group.max() > 1)           # more rows than one batch holds
    # the deal: every edge once; after every step no group is further from the mean than the heaviest row
    cum = np.cumsum(plan["group_step_edges"], 1)
    assert cum[:, -1].sum() == d_owned.sum() and (np.abs(cum - cum.mean(0)).max(0) <= d_owned.max()).all()
    assert eng.kernel_config()["class_owned"]["groups"] == groups
    assert eng.kernel_names()["split"].startswith("spmm_owned_kernel")


def test_engines_that_cannot_take_the_owned_pass_keep_chunk_and_combine(k):
    X, Z0, P, _, _ = C.integer_case(128)
    for more in (dict(X=X.double(), Z0=Z0.double()), dict(X=X.bfloat16(), Z0=Z0.bfloat16())):
        from .oracle_kernels import OracleKernels as Plain          # a backend without the call at all
        eng = C.make_engine(Plain(), DEV, 128, 1, "H160", more["X"], more["Z0"], P)
        assert not eng.class_owned and all(o is None for o in eng.owned_rows)
        assert "class_owned" not in eng.kernel_config()
    default = C.make_engine(k, DEV, 128, 1, "H160", X, Z0, P, class_owned=None)
    assert default.owned_possible and not default.beyond_cache and not default.class_owned     # a cache-resident table
    default.beyond_cache = True
    default._choose_owned(None, 160, C.ROW_EDGES, 8, 2048, 256, None)
    assert default.class_owned == xcd.OWNED_DEFAULT


@pytest.mark.parametrize("d,tiles", C.WIDTHS)
@pytest.mark.parametrize("setting", list(C.SETTINGS))
def test_owned_sweep_on_the_double_is_exact_on_integer_data(k, setting, d, tiles):
    X, Z0, P, Z1, delta = C.integer_case(d)
    got = {}
    for owned in (True, False):
        eng = C.make_engine(k, DEV, d, tiles, setting, X, Z0, P, class_owned=owned)
        assert eng.class_owned == owned
        dl = eng.sweep(1.0)
        assert dl == delta and torch.equal(eng.get_Z(), Z1)
        got[owned] = eng.get_Z()
    assert torch.equal(got[True], got[False])


@pytest.mark.parametrize("d,tiles", C.WIDTHS)
def test_owned_sweep_on_the_double_agrees_on_gaussian_data(k, d, tiles):
    X, Z0, P, Z1, delta, gamma = C.gaussian_case(d)
    out = {}
    for owned in (True, False):
        eng = C.make_engine(k, DEV, d, tiles, "all_phased", X, Z0, P, class_owned=owned)
        out[owned] = (eng.sweep(gamma), eng.get_Z().double())
    (d1, za), (d0, zb) = out[True], out[False]
    assert float((za - zb).norm() / zb.norm()) < 1e-6 and d1 == pytest.approx(d0, rel=1e-6)
    assert float((za - Z1).norm() / Z1.norm()) < 2e-6 and d1 == pytest.approx(delta, rel=1e-5)


# ---- every case of tests/test_owned_class_pass_gpu.py, first on the double ---------------------------------------------
def test_sum_bytes_follow_the_lane_layout():
    assert [C.lanes(d, t) for d, t in C.WIDTHS] == [32, 32, 64, 32, 64, 64, 64]
    assert [C.sum_bytes(d, t) for d, t in C.WIDTHS] == [512, 512, 1024, 512, 1024, 1024, 1024]
    assert [-(-d // 4) for d, _ in C.WIDTHS[3:]] == [17, 33, 64, 64] and [d % 4 for d, _ in C.WIDTHS[3:]] == [2, 2, 2, 0]


@pytest.mark.parametrize("run", C.LOAD_RUNS, ids=C.load_id)
def test_every_load_count_on_the_double(k, run):
    C.check_loads(k, DEV, *run)


def test_the_double_refuses_the_load_counts_the_kernel_refuses(k):
    for d, loads in ((128, 7), (136, 6), (130, 6), (128, 4)):
        eng = engine(k, "H160", d, owned_loads=loads)
        with pytest.raises(AssertionError, match="no instance"):
            eng.sweep(1.0)


@pytest.mark.parametrize("d,tiles", C.WIDTHS)
def test_bits_do_not_depend_on_the_launch_settings_on_the_double(k, d, tiles):
    C.check_independence(k, DEV, d, tiles)


@pytest.mark.parametrize("d,threads,row_edges", C.STEPS64_RUNS)
def test_sixty_four_steps_on_the_double(k, d, threads, row_edges):
    C.check_steps64(k, DEV, d, threads, row_edges)


@pytest.mark.parametrize("d", [128, 254])
def test_shipped_constants_on_the_double(k, d):
    C.check_shipped_constants(k, DEV, d)


@pytest.mark.parametrize("d", [128, 136])
def test_batches_above_64_kib_on_the_double(k, d):
    C.check_lds_grant_grows(k, DEV, d)


@pytest.mark.parametrize("d,tiles", [(128, 1), (256, 2), (130, 1)])
def test_set_owned_replans_between_sweeps_on_the_double(k, d, tiles):
    C.check_set_owned(k, DEV, d, tiles)
