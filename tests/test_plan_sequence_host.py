"""The ordered steps of SweepEngine._build_plan, engine by engine, through a recording subclass of the fused-tiles CPU
double: the event marks, the bound method names with the width, partials region and mirror of every call, the
exchange steps.  An in-order stream makes the order part of the speed, and the class and split passes of one block share
a slab, so the interleaving owned(t), class(t), split(t) per tile and the place of the fused calls are pinned here.

EXPECTED was recorded from the commit before _build_plan spelled its passes through one helper: the plan is the
contract that helper keeps.

A step is (kind, method, width, region, mirrored): `width` is d for a call on one tile (a cut view) and (d, tile_cols)
for a fused call on the whole tables; `region` is (tile, start) -- the call's partials begin `start` slots into its
block's share of that tile's partials (blocks.PartialLayout), None for a call without partials."""
import inspect

import pytest

from clane_amd.engine import SweepEngine

from . import fused_tiles_cases as F
from .engine_exact_cases import load_P, run_ranks
from .fused_tiles_oracle_kernels import OracleKernels

DEV = "cpu"


class Bound:
    """What RecordingKernels.bind returns: the call itself, and what it was bound from."""

    def __init__(self, fn, method, arguments):
        self.fn, self.method, self.arguments = fn, method, arguments

    def __call__(self):
        return self.fn()


class RecordingKernels(OracleKernels):
    def bind(self, method, *args, **kwargs):
        named = inspect.signature(getattr(self, method)).bind(*args, **kwargs).arguments
        return Bound(super().bind(method, *args, **kwargs), method, named)


def describe(eng, plan):
    """The plan of one sweep as a list of blocks, each a list of steps, and the final reduction."""
    per_block, final = plan
    stride, item = eng.partial_off[-1], eng.partials.element_size()
    out = []
    for i, steps in enumerate(per_block):
        block = []
        for step in steps:
            if step[0] == "event":
                assert step[1] == i
                block.append(("event", step[2]))
            elif step[0] == "call":
                a = step[1].arguments
                width = (a["d"], a["tile_cols"]) if "tile_cols" in a else a.get("d")
                region = None
                if "partials" in a:
                    off = (a["partials"].data_ptr() - eng.partials.data_ptr()) // item
                    region = (off // stride, off % stride - eng.partial_off[i]) if stride else (0, off)
                block.append(("call", step[1].method, width, region, a.get("mirror") is not None))
            else:
                block.append((step[0],))
        out.append(block)
    return out, ("call", final.method)


def fused_engine(fused, d=256, tiles=2, **more):
    X, Z0, P = F.integer_case(d)[:3]
    return F.make_engine(RecordingKernels(), DEV, d, tiles, X, Z0, P, fused_tiles=fused, **more)


def bf16_engine():
    X, Z0, P = F.integer_case(256)[:3]
    eng = SweepEngine(F.csr(), X.bfloat16(), DEV, RecordingKernels(), column_tiles=2, class_threshold=64,
                      hot_rows_first=False, fused_tiles=True)
    eng.set_Z(Z0.bfloat16())
    load_P(eng, P)
    return eng


def halo_plans():
    """A two-rank halo engine: row division, mirrored launches, the packed exchange."""
    X = F.integer_case(128)[0]

    def rank(_, comm):
        eng = SweepEngine(F.csr(), X, DEV, RecordingKernels(), comm=comm, exchange="halo", class_threshold=64,
                          fused_tiles=True)
        assert any(m is not None for m in eng.mirrors)
        return describe(eng, eng._build_plan(0, 1, 0, 1.0))
    return run_ranks(2, rank, DEV)


FORMS = {"per_tile": False, "fused": True, "row_owned": ("row", "owned"), "class": ("class",)}
ENGINES = {"one_tile": lambda: fused_engine(True, tiles=1)}
for _d, _t in ((256, 2), (384, 3)):
    for _name, _form in FORMS.items():
        ENGINES[f"{_t}_tiles_{_name}"] = lambda d=_d, t=_t, form=_form: fused_engine(form, d, t)
ENGINES.update({
    "3_blocks_per_tile": lambda: fused_engine(False, chunks=3),
    "3_blocks_fused": lambda: fused_engine(True, chunks=3),
    "owned_off_per_tile": lambda: fused_engine(False, class_owned=False),
    "owned_off_fused": lambda: fused_engine(True, class_owned=False),
    # no class pass: the rows above 64 edges go to the 4-wave, 16-wave and split launches of every tile
    "no_class_pass_2_tiles": lambda: fused_engine(True, class_threshold=0, class_owned=False, hub_threshold=300),
    "bf16_2_tiles": bf16_engine,
})

EXPECTED = {'one_tile': [[('event', 0),
               ('call', 'spmm_update_owned', 256, (0, 96), False),
               ('call', 'spmm_update_class', 256, (0, 96), False),
               ('event', 4),
               ('event', 1),
               ('event', 2),
               ('call', 'spmm_update', 256, (0, 0), False),
               ('event', 3)]],
 '2_tiles_per_tile': [[('event', 0),
                       ('call', 'spmm_update_owned', 128, (0, 96), False),
                       ('call', 'spmm_update_class', 128, (0, 96), False),
                       ('call', 'spmm_update_owned', 128, (1, 96), False),
                       ('call', 'spmm_update_class', 128, (1, 96), False),
                       ('event', 4),
                       ('event', 1),
                       ('event', 2),
                       ('call', 'spmm_update', 128, (0, 0), False),
                       ('call', 'spmm_update', 128, (1, 0), False),
                       ('event', 3)]],
 '2_tiles_fused': [[('event', 0),
                    ('call', 'spmm_update_owned_tiles', (256, 128), (0, 96), False),
                    ('call', 'spmm_update_class_tiles', (256, 128), (0, 96), False),
                    ('event', 4),
                    ('event', 1),
                    ('event', 2),
                    ('call', 'spmm_update_tiles', (256, 128), (0, 0), False),
                    ('event', 3)]],
 '2_tiles_row_owned': [[('event', 0),
                        ('call', 'spmm_update_owned_tiles', (256, 128), (0, 96), False),
                        ('call', 'spmm_update_class', 128, (0, 96), False),
                        ('call', 'spmm_update_class', 128, (1, 96), False),
                        ('event', 4),
                        ('event', 1),
                        ('event', 2),
                        ('call', 'spmm_update_tiles', (256, 128), (0, 0), False),
                        ('event', 3)]],
 '2_tiles_class': [[('event', 0),
                    ('call', 'spmm_update_class_tiles', (256, 128), (0, 96), False),
                    ('call', 'spmm_update_owned', 128, (0, 96), False),
                    ('call', 'spmm_update_owned', 128, (1, 96), False),
                    ('event', 4),
                    ('event', 1),
                    ('event', 2),
                    ('call', 'spmm_update', 128, (0, 0), False),
                    ('call', 'spmm_update', 128, (1, 0), False),
                    ('event', 3)]],
 '3_tiles_per_tile': [[('event', 0),
                       ('call', 'spmm_update_owned', 128, (0, 96), False),
                       ('call', 'spmm_update_class', 128, (0, 96), False),
                       ('call', 'spmm_update_owned', 128, (1, 96), False),
                       ('call', 'spmm_update_class', 128, (1, 96), False),
                       ('call', 'spmm_update_owned', 128, (2, 96), False),
                       ('call', 'spmm_update_class', 128, (2, 96), False),
                       ('event', 4),
                       ('event', 1),
                       ('event', 2),
                       ('call', 'spmm_update', 128, (0, 0), False),
                       ('call', 'spmm_update', 128, (1, 0), False),
                       ('call', 'spmm_update', 128, (2, 0), False),
                       ('event', 3)]],
 '3_tiles_fused': [[('event', 0),
                    ('call', 'spmm_update_owned_tiles', (384, 128), (0, 96), False),
                    ('call', 'spmm_update_class_tiles', (384, 128), (0, 96), False),
                    ('event', 4),
                    ('event', 1),
                    ('event', 2),
                    ('call', 'spmm_update_tiles', (384, 128), (0, 0), False),
                    ('event', 3)]],
 '3_tiles_row_owned': [[('event', 0),
                        ('call', 'spmm_update_owned_tiles', (384, 128), (0, 96), False),
                        ('call', 'spmm_update_class', 128, (0, 96), False),
                        ('call', 'spmm_update_class', 128, (1, 96), False),
                        ('call', 'spmm_update_class', 128, (2, 96), False),
                        ('event', 4),
                        ('event', 1),
                        ('event', 2),
                        ('call', 'spmm_update_tiles', (384, 128), (0, 0), False),
                        ('event', 3)]],
 '3_tiles_class': [[('event', 0),
                    ('call', 'spmm_update_class_tiles', (384, 128), (0, 96), False),
                    ('call', 'spmm_update_owned', 128, (0, 96), False),
                    ('call', 'spmm_update_owned', 128, (1, 96), False),
                    ('call', 'spmm_update_owned', 128, (2, 96), False),
                    ('event', 4),
                    ('event', 1),
                    ('event', 2),
                    ('call', 'spmm_update', 128, (0, 0), False),
                    ('call', 'spmm_update', 128, (1, 0), False),
                    ('call', 'spmm_update', 128, (2, 0), False),
                    ('event', 3)]],
 '3_blocks_per_tile': [[('event', 0),
                        ('call', 'spmm_update_owned', 128, (0, 32), False),
                        ('call', 'spmm_update_class', 128, (0, 32), False),
                        ('call', 'spmm_update_owned', 128, (1, 32), False),
                        ('call', 'spmm_update_class', 128, (1, 32), False),
                        ('event', 4),
                        ('event', 1),
                        ('event', 2),
                        ('call', 'spmm_update', 128, (0, 0), False),
                        ('call', 'spmm_update', 128, (1, 0), False),
                        ('event', 3)],
                       [('event', 0),
                        ('event', 4),
                        ('event', 1),
                        ('event', 2),
                        ('call', 'spmm_update', 128, (0, 0), False),
                        ('call', 'spmm_update', 128, (1, 0), False),
                        ('event', 3)],
                       [('event', 0),
                        ('event', 4),
                        ('event', 1),
                        ('event', 2),
                        ('call', 'spmm_update', 128, (0, 0), False),
                        ('call', 'spmm_update', 128, (1, 0), False),
                        ('event', 3)]],
 '3_blocks_fused': [[('event', 0),
                     ('call', 'spmm_update_owned_tiles', (256, 128), (0, 32), False),
                     ('call', 'spmm_update_class_tiles', (256, 128), (0, 32), False),
                     ('event', 4),
                     ('event', 1),
                     ('event', 2),
                     ('call', 'spmm_update_tiles', (256, 128), (0, 0), False),
                     ('event', 3)],
                    [('event', 0),
                     ('event', 4),
                     ('event', 1),
                     ('event', 2),
                     ('call', 'spmm_update_tiles', (256, 128), (0, 0), False),
                     ('event', 3)],
                    [('event', 0),
                     ('event', 4),
                     ('event', 1),
                     ('event', 2),
                     ('call', 'spmm_update_tiles', (256, 128), (0, 0), False),
                     ('event', 3)]],
 'owned_off_per_tile': [[('event', 0),
                         ('call', 'spmm_update_class', 128, (0, 96), False),
                         ('call', 'spmm_update_class', 128, (1, 96), False),
                         ('event', 4),
                         ('event', 1),
                         ('event', 2),
                         ('call', 'spmm_update', 128, (0, 0), False),
                         ('call', 'spmm_update', 128, (1, 0), False),
                         ('event', 3)]],
 'owned_off_fused': [[('event', 0),
                      ('call', 'spmm_update_class_tiles', (256, 128), (0, 96), False),
                      ('event', 4),
                      ('event', 1),
                      ('event', 2),
                      ('call', 'spmm_update_tiles', (256, 128), (0, 0), False),
                      ('event', 3)]],
 'no_class_pass_2_tiles': [[('event', 0),
                            ('call', 'spmm_update_split', 128, (0, 156), False),
                            ('call', 'spmm_update_split', 128, (1, 156), False),
                            ('event', 4),
                            ('call', 'spmm_update_long', 128, (0, 110), False),
                            ('call', 'spmm_update_long', 128, (1, 110), False),
                            ('event', 1),
                            ('call', 'spmm_update_long', 128, (0, 96), False),
                            ('call', 'spmm_update_long', 128, (1, 96), False),
                            ('event', 2),
                            ('call', 'spmm_update_tiles', (256, 128), (0, 0), False),
                            ('event', 3)]],
 'bf16_2_tiles': [[('event', 0),
                   ('call', 'spmm_update_class', 128, (0, 96), False),
                   ('call', 'spmm_update_class', 128, (1, 96), False),
                   ('event', 4),
                   ('event', 1),
                   ('event', 2),
                   ('call', 'spmm_update', 128, (0, 0), False),
                   ('call', 'spmm_update', 128, (1, 0), False),
                   ('event', 3)]]}
# per rank, per block
EXPECTED_HALO = [[[('event', 0),
   ('call', 'spmm_update_class', 128, (0, 12), True),
   ('event', 4),
   ('event', 1),
   ('event', 2),
   ('call', 'spmm_update', 128, (0, 0), True),
   ('event', 3),
   ('alltoall',)],
  [('event', 0),
   ('call', 'spmm_update_class', 128, (0, 12), True),
   ('event', 4),
   ('event', 1),
   ('event', 2),
   ('call', 'spmm_update', 128, (0, 0), True),
   ('event', 3),
   ('alltoall',)],
  [('event', 0),
   ('call', 'spmm_update_class', 128, (0, 12), True),
   ('event', 4),
   ('event', 1),
   ('event', 2),
   ('call', 'spmm_update', 128, (0, 0), True),
   ('event', 3),
   ('alltoall',)],
  [('event', 0),
   ('call', 'spmm_update_class', 128, (0, 12), True),
   ('event', 4),
   ('event', 1),
   ('event', 2),
   ('call', 'spmm_update', 128, (0, 0), True),
   ('event', 3),
   ('alltoall',)]],
 [[('event', 0),
   ('call', 'spmm_update_class', 128, (0, 12), True),
   ('event', 4),
   ('event', 1),
   ('event', 2),
   ('call', 'spmm_update', 128, (0, 0), True),
   ('event', 3),
   ('alltoall',)],
  [('event', 0),
   ('call', 'spmm_update_class', 128, (0, 12), True),
   ('event', 4),
   ('event', 1),
   ('event', 2),
   ('call', 'spmm_update', 128, (0, 0), True),
   ('event', 3),
   ('alltoall',)],
  [('event', 0),
   ('call', 'spmm_update_class', 128, (0, 12), True),
   ('event', 4),
   ('event', 1),
   ('event', 2),
   ('call', 'spmm_update', 128, (0, 0), True),
   ('event', 3),
   ('alltoall',)],
  [('event', 0),
   ('call', 'spmm_update_class', 128, (0, 12), True),
   ('event', 4),
   ('event', 1),
   ('event', 2),
   ('call', 'spmm_update', 128, (0, 0), True),
   ('event', 3),
   ('alltoall',)]]]


def plan_of(name):
    eng = ENGINES[name]()
    return describe(eng, eng._build_plan(0, 1, 0, 1.0))


@pytest.mark.parametrize("name", list(ENGINES))
def test_the_plan_keeps_its_steps(name):
    blocks, final = plan_of(name)
    assert final == ("call", "reduce_partials")
    assert blocks == EXPECTED[name]


def test_the_halo_plan_keeps_its_steps():
    plans = halo_plans()
    assert [final for _, final in plans] == [("call", "reduce_partials")] * 2
    assert [blocks for blocks, _ in plans] == EXPECTED_HALO
    assert any(step[0] == "call" and step[4] for blocks in EXPECTED_HALO for b in blocks for step in b)      # mirrored


def test_the_cases_cover_what_they_are_there_for():
    calls = lambda name: [s[1] for b in EXPECTED[name] for s in b if s[0] == "call"]         # noqa: E731
    assert len(EXPECTED["3_blocks_fused"]) == 3 and len(EXPECTED["one_tile"]) == 1
    assert calls("2_tiles_per_tile")[:4] == ["spmm_update_owned", "spmm_update_class"] * 2   # owned(t), class(t) per tile
    assert calls("3_tiles_class")[:4] == ["spmm_update_class_tiles"] + ["spmm_update_owned"] * 3
    assert "spmm_update_owned" not in calls("owned_off_per_tile") and "spmm_update_class" in calls("owned_off_per_tile")
    assert {"spmm_update_long", "spmm_update_split"} <= set(calls("no_class_pass_2_tiles"))
    assert not any(n.endswith("_tiles") for n in calls("bf16_2_tiles") + calls("one_tile"))
