"""Shared by tests/test_owned_plan_host.py and tests/test_owned_class_pass_gpu.py: one small graph that holds every row
shape the owned class pass (csrc/spmm_update.h spmm_owned_kernel, xcd.owned_plan) treats differently, integer and
Gaussian data over it with references computed once, and the engine settings that force each path.  Nobody writes to
what this module returns."""
import functools

import numpy as np
import pytest
import torch

from clane_amd import xcd
from clane_amd.engine import SweepEngine
from clane_amd.partition import HostCSR
from clane_amd.plan import column_slice, lanes_per_row
from clane_amd.xcd import xcd_class
from oracle import clane_oracle as O

from .engine_exact_cases import load_P, plan_field

V = 1536
CHUNK = 64                      # class_chunk and the owned pieces
ROW_EDGES = 128                 # owned_row_edges: rows above it are summed as virtual rows
# (d, column tiles): 512-byte rows, two tiles of them, ragged 1-KiB rows; 17 packs with a ragged last one, the first
# 64-lane width with a ragged pack, a ragged pack in lane 63, 64 full packs in one tile
WIDTHS = [(128, 1), (256, 2), (136, 1), (66, 1), (130, 1), (254, 1), (256, 1)]

# degrees of the first rows, by what they are there for
ALL_CLASSES = [65, 100, 150, 200, 257, 300]     # rows of 65..300 edges touching all 8 classes
EMPTY_CLASS_ROW, EMPTY_CLASS = 6, 3             # 120 edges, none into class 3
EXACT = {7: 96, 8: 97, 9: 160, 10: 161, 12: ROW_EDGES, 13: ROW_EDGES + 1}     # H and H + 1 for H = 96 and 160; one / two virtual rows
ONE_CLASS_ROW, ONE_CLASS = 11, 5                # 150 edges of one class: a segment of several pieces
N_CLASS_ROWS = 44                               # rows 14..43: 65..160 edges, more rows than a small batch holds
N_SHORT = 700                                   # rows 44..743: 1..64 edges; the rest are sinks

# engine settings: (owned_max_edges, class_phases, phase_threshold)
SETTINGS = {"H96": (96, None, 512),             # rows of 65..96 edges owned, 97 and up by chunk + combine
            "H160": (160, None, 512),           # rows up to 160 owned, among them virtual rows and the one-class row
            "all_phased": (4096, 2, 200)}       # every class row owned; rows above 200 edges in 2 phases = 16 steps
# kOwnedMaxSteps: every class row in 8 phases x 8 classes, segments as short as one edge (not among the SETTINGS that
# every test sweeps)
STEPS64 = "steps64"
ALL_SETTINGS = dict(SETTINGS, steps64=(4096, 8, 64))


@functools.lru_cache(maxsize=None)
def graph():
    """(rowptr, colidx) int64, rows sorted and unique.  Table positions are vertex ids (hot_rows_first=False)."""
    rng = np.random.default_rng(7)
    cls = xcd_class(np.arange(V))
    rows = []
    for r in range(V):
        if r < len(ALL_CLASSES):
            cols = rng.choice(V, ALL_CLASSES[r], replace=False)
            assert np.unique(cls[cols]).size == 8
        elif r == EMPTY_CLASS_ROW:
            cols = rng.choice(np.nonzero(cls != EMPTY_CLASS)[0], 120, replace=False)
        elif r in EXACT:
            cols = rng.choice(V, EXACT[r], replace=False)
        elif r == ONE_CLASS_ROW:
            cols = rng.choice(np.nonzero(cls == ONE_CLASS)[0], 150, replace=False)
        elif r < N_CLASS_ROWS:
            cols = rng.choice(V, int(rng.integers(65, 161)), replace=False)
        elif r < N_CLASS_ROWS + N_SHORT:
            cols = rng.choice(V, 64 if r == N_CLASS_ROWS else int(rng.integers(1, 65)), replace=False)
        else:
            cols = np.empty(0, dtype=np.int64)
        rows.append(np.sort(cols))
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum([c.size for c in rows], out=rowptr[1:])
    return rowptr, np.concatenate(rows).astype(np.int64)


def csr():
    rowptr, colidx = graph()
    return HostCSR(V, rowptr, colidx.astype(np.int32))


@functools.lru_cache(maxsize=None)
def integer_case(d):
    """X, Z0 in -4..4, P in 1..3 (sorted edge order), gamma = 1: every sum is an integer below 2^13.  Returns float32
    X, Z0, P and the int64 reference of one sweep with its delta."""
    rowptr, colidx = graph()
    rng = np.random.default_rng(100 + d)
    X = rng.integers(-4, 5, (V, d))
    Z0 = rng.integers(-4, 5, (V, d))
    P = rng.integers(1, 4, colidx.size)
    Z1 = Z0.copy()
    for r in range(V):
        a, b = rowptr[r], rowptr[r + 1]
        if b > a:
            Z1[r] = X[r] + (P[a:b, None] * Z0[colidx[a:b]]).sum(0)
    delta = int(np.abs(Z1 - Z0).sum())
    f = lambda a: torch.from_numpy(a.astype(np.float32))       # noqa: E731
    return f(X), f(Z0), f(P), f(Z1), delta


@functools.lru_cache(maxsize=None)
def gaussian_case(d, gamma=0.7):
    """Gaussian X, Z0, positive P with rows summing to one; the oracle's sweep in double."""
    rowptr, colidx = graph()
    g = torch.Generator().manual_seed(200 + d)
    X, Z0 = torch.randn(V, d, generator=g), torch.randn(V, d, generator=g)
    P = torch.rand(colidx.size, generator=g) + 0.1
    deg = np.diff(rowptr)
    P = P / torch.from_numpy(np.repeat(np.add.reduceat(P.numpy(), rowptr[:-1][deg > 0]), deg[deg > 0]))
    Z1, delta = O.sweep(rowptr, colidx, P.double(), X.double(), Z0.double(), gamma)
    return X, Z0, P, Z1, float(delta), gamma


BATCH_VROWS = 4                 # LDS sums per batch: every group of 8 then needs several batches


def lanes(d, tiles=1):
    """Lanes per row of the widest column tile (the first)."""
    c0, c1 = column_slice(d, torch.float32, tiles, 0)
    return lanes_per_row(c1 - c0, torch.float32)


def sum_bytes(d, tiles=1):
    """One LDS sum: a whole row of the lane layout, 32 or 64 lanes of 16 bytes."""
    return 16 * lanes(d, tiles)


def loads_of(d, tiles=1):
    """The row loads in flight per wave that have a kernel instance at this width (csrc/clane_abi.hip); 0 = the chunk
    kernel's choice, which is 6 beyond the caches and 8 within them at 32 lanes per row, 8 at 64."""
    return (0, 6, 8, 12) if lanes(d, tiles) == 32 else (0, 8, 12)


def load_cases(d, tiles=1):
    """(owned_loads, beyond_cache): every instance of the width, asked for by number and chosen by the cache hint."""
    return [(0, False), (0, True)] + [(u, False) for u in loads_of(d, tiles) if u]


def make_engine(kernels, dev, d, tiles, setting, X, Z0, P, class_owned=True, **more):
    H, phases, pt = ALL_SETTINGS[setting]
    kw = dict(class_threshold=64, class_chunk=CHUNK, class_phases=phases, phase_threshold=pt, column_tiles=tiles,
              hot_rows_first=False, class_owned=class_owned, owned_max_edges=H, owned_row_edges=ROW_EDGES,
              owned_groups=8, owned_lds_bytes=BATCH_VROWS * sum_bytes(d, tiles), owned_block_threads=256)
    kw.update(more)
    eng = SweepEngine(csr(), X, dev, kernels, **kw)
    assert torch.equal(eng.pos.cpu(), torch.arange(V))          # the classes graph() chose its columns by
    eng.set_Z(Z0)
    load_P(eng, P)
    return eng


# ---- checks shared by the card and the double: `kernels` is HipKernels or tests/owned_oracle_kernels.OracleKernels ----
def the_plan(eng):
    (plan, rest, n_rest), = [o for o in eng.owned_rows if o is not None]
    return plan


def check_integer_sweep(eng, d):
    """One sweep of integer data: the delta, the table and the pad columns, all exact."""
    _, _, _, Z1, delta = integer_case(d)
    assert eng.sweep(1.0) == delta
    assert torch.equal(eng.get_Z(), Z1)
    assert eng.Zcur.shape[1] >= d and bool((eng.Zcur[:, d:] == 0).all())


def integer_engine(kernels, dev, d, tiles, setting, **more):
    X, Z0, P, _, _ = integer_case(d)
    return make_engine(kernels, dev, d, tiles, setting, X, Z0, P, **more)


# (setting, d, column tiles, owned_loads, beyond_cache): every instance at every width under every setting
LOAD_RUNS = [(s, d, tiles, u, beyond) for s in SETTINGS for d, tiles in WIDTHS for u, beyond in load_cases(d, tiles)]


def load_id(run):
    setting, d, tiles, u, beyond = run
    return f"{setting}-d{d}x{tiles}-lanes{lanes(d, tiles)}-U{u}" + ("-beyond" if beyond else "")


def check_loads(kernels, dev, setting, d, tiles, loads, beyond):
    """`loads` row loads in flight (0: by the cache hint `beyond`) -- one kernel instance each."""
    eng = integer_engine(kernels, dev, d, tiles, setting, owned_loads=loads)
    assert eng.class_owned and eng.owned_loads == loads in loads_of(d, tiles)
    eng.beyond_cache = beyond
    check_integer_sweep(eng, d)


def independence_variants(d, tiles):
    """Settings that must not change a bit: groups x batch size x cache hint as before; every load count, by number and
    by the hint; a one-wave workgroup and the largest one."""
    sb = sum_bytes(d, tiles)
    out = [dict(owned_groups=g, owned_lds_bytes=v * sb, owned_block_threads=512 if g == 16 else 256, hint=h)
           for g in (8, 16, 24) for v in (BATCH_VROWS, 16) for h in (False, True)]
    out += [dict(owned_loads=u, hint=h) for u, h in load_cases(d, tiles)]
    out += [dict(owned_block_threads=t, owned_loads=u) for t, u in ((64, 12), (64, 0), (1024, 8))]
    return out


def check_independence(kernels, dev, d, tiles):
    X, Z0, P, _, _, gamma = gaussian_case(d)
    seen = None
    for variant in independence_variants(d, tiles):
        variant = dict(variant)
        hint = variant.pop("hint", False)
        eng = make_engine(kernels, dev, d, tiles, "all_phased", X, Z0, P, **variant)
        eng.beyond_cache = hint
        out = (eng.sweep(gamma), eng.Zcur.clone())
        if seen is None:
            seen = out
        assert out[0] == seen[0] and torch.equal(out[1], seen[1]), (variant, hint)


# (d, owned_block_threads, owned_row_edges) of the 64-step runs: a one-wave workgroup (s_cnt zeroed by threads 0..63,
# all of them), the usual one and the largest; virtual rows of at most 64 edges, the smallest allowed
STEPS64_RUNS = [(d, t, ROW_EDGES) for d in (128, 130) for t in (64, 256, 1024)] + [(128, 256, 64), (130, 64, 64)]


def check_steps64(kernels, dev, d, block_threads, row_edges):
    """n_steps = kOwnedMaxSteps.  The LDS is sized from the plan's largest row: planned once with room for any row,
    then with that many sums per batch."""
    roomy = integer_engine(kernels, dev, d, 1, STEPS64, owned_row_edges=row_edges, owned_lds_bytes=128 * sum_bytes(d))
    largest = int(np.diff(plan_field(the_plan(roomy), "row_vptr")).max())
    assert largest > (1 if row_edges >= ROW_EDGES else 4)
    eng = integer_engine(kernels, dev, d, 1, STEPS64, owned_row_edges=row_edges, owned_block_threads=block_threads,
                         owned_lds_bytes=max(largest, BATCH_VROWS) * sum_bytes(d))
    plan = the_plan(eng)
    assert plan_field(plan, "n_steps") == 64 and int(plan_field(plan, "seg_len").min()) == 1
    assert plan_field(plan, "max_batch_vrows") >= largest and int(np.diff(plan_field(plan, "grp_bat_ptr")).max()) > 1
    check_integer_sweep(eng, d)


def check_shipped_constants(kernels, dev, d):
    """256 groups of 1024 threads, 152 KiB, rows up to 512 edges whole, 12 loads: 44 class rows, so 212 groups have no
    batch at all."""
    eng = integer_engine(kernels, dev, d, 1, "all_phased", owned_groups=xcd.OWNED_GROUPS,
                         owned_block_threads=xcd.OWNED_BLOCK_THREADS, owned_lds_bytes=xcd.OWNED_LDS_BYTES,
                         owned_row_edges=xcd.OWNED_ROW_EDGES, owned_max_edges=xcd.OWNED_MAX_EDGES)
    assert eng.owned_loads == xcd.OWNED_LOADS == 12
    per_group = np.diff(plan_field(the_plan(eng), "grp_bat_ptr"))
    assert per_group.size == 256 and int((per_group == 0).sum()) == 212 and int(per_group.max()) == 1
    check_integer_sweep(eng, d)


def check_lds_grant_grows(kernels, dev, d):
    """One group takes the 400 rows above 32 edges: first in batches just above the 64 KiB a workgroup gets without
    asking, then in batches of the shipped 152 KiB -- the kernel instance asks twice, for more the second time."""
    sb, asked = sum_bytes(d), []
    for lds in (68 * 1024, xcd.OWNED_LDS_BYTES):
        eng = integer_engine(kernels, dev, d, 1, "all_phased", class_threshold=32, owned_groups=1, owned_lds_bytes=lds,
                             owned_block_threads=1024)
        plan = the_plan(eng)
        assert plan_field(plan, "row_id").size > 300 and int(np.diff(plan_field(plan, "grp_bat_ptr")).max()) > 1
        asked.append(int(plan_field(plan, "max_batch_vrows")) * sb)
        assert lds - 3 * sb < asked[-1] <= lds and asked[-1] > 64 * 1024
        check_integer_sweep(eng, d)
    assert asked[1] > asked[0] and asked[1] > 150 * 1024


def check_set_owned(kernels, dev, d=128, tiles=1):
    """One engine through owned -> off -> owned with other settings -> owned up to 96 edges; at every stage the sweep's
    delta and table are bitwise those of a fresh engine built with the stage's settings and the same table."""
    X, Z0, P, _, _, gamma = gaussian_case(d)
    sb = sum_bytes(d, tiles)
    eng = make_engine(kernels, dev, d, tiles, "all_phased", X, Z0, P)
    replanned = dict(owned_groups=16, owned_lds_bytes=16 * sb, owned_block_threads=512, owned_loads=8)
    stages = [(None, dict()),
              (lambda: eng.set_owned(False), dict(class_owned=False)),
              (lambda: eng.set_owned(True, groups=16, lds_bytes=16 * sb, block_threads=512, loads=8), replanned),
              (lambda: eng.set_owned(True, max_edges=96), dict(replanned, owned_max_edges=96))]
    for i, (switch, settings) in enumerate(stages):
        if switch is not None:
            switch()
        Zin = eng.get_Z()
        fresh = make_engine(kernels, dev, d, tiles, "all_phased", X, Zin, P, **settings)
        assert eng.class_owned == fresh.class_owned == settings.get("class_owned", True)
        for name in ("owned_groups", "owned_block_threads", "owned_loads", "owned_max_edges", "owned_batch_vrows"):
            assert not eng.class_owned or getattr(eng, name) == getattr(fresh, name), (i, name)
        plans = [[None if o is None else o[2] for o in e.owned_rows] for e in (eng, fresh)]     # rows beside the owned ones
        assert plans[0] == plans[1] and (plans[0][0] is not None) == eng.class_owned
        assert (i == 3) == bool(plans[0][0])                                   # rows beside the owned ones: the last stage
        assert eng.sweep(gamma) == fresh.sweep(gamma), i
        assert torch.equal(eng.get_Z(), fresh.get_Z()) and torch.equal(eng.Zcur, fresh.Zcur), i
    with pytest.raises(TypeError):
        eng.set_owned(True, lanes=32)
    no_pass = SweepEngine(csr(), X.bfloat16(), dev, kernels, class_threshold=64, hot_rows_first=False)
    assert not no_pass.owned_possible and not no_pass.class_owned
    no_pass.set_owned(False)
    with pytest.raises(ValueError):
        no_pass.set_owned(True)
