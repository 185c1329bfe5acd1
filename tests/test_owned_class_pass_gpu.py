"""spmm_owned_kernel on the GPU, driven by SweepEngine over the graph of tests/owned_cases.py: rows of 65..300 edges over
all 8 classes, a row with an empty class, rows of exactly H and H + 1 edges, a segment of several pieces, rows cut into
virtual rows, more rows than a batch holds, rows of <= 64 edges and sinks beside them.  Widths: 512-byte rows, two
column tiles of them, ragged 1-KiB rows (d = 136: the c0 < d mask), a ragged last pack at 32 lanes (66) and at 64 (130:
the narrowest 64-lane width; 254: the ragged pack in lane 63), 64 full packs (256).  Every kernel instance -- 6, 8 and
12 row loads in flight at 32 lanes per row, 8 and 12 at 64 --, the step limit, workgroups of one wave and of sixteen,
the shipped launch configuration, batches beyond the default LDS limit and SweepEngine.set_owned.
tests/test_owned_plan_host.py runs every case here through the CPU double first."""
import pytest
import torch

from clane_amd import _hip
from clane_amd.embedder import Embedder
from clane_amd.graph import Graph
from clane_amd.similarity import CosineSimilarity

from . import owned_cases as C

pytestmark = pytest.mark.gpu
TOL = 2e-6                      # tests/test_gpu_parity.py: rel-L2 of an fp32 sweep against the oracle
DELTA_RTOL = 1e-5               # and its delta


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("d,tiles", C.WIDTHS)
@pytest.mark.parametrize("setting", list(C.SETTINGS))
def test_integer_data_is_exact(k, dev, setting, d, tiles):
    X, Z0, P, Z1, delta = C.integer_case(d)
    eng = C.make_engine(k, dev, d, tiles, setting, X, Z0, P)
    assert eng.class_owned and any(o is not None for o in eng.owned_rows)
    plan = next(o for o in eng.owned_rows if o is not None)[0]
    if setting != "H96":                # (H96 owns a dozen rows) some group takes its rows in several batches
        assert int(plan.arrays["grp_bat_ptr"].diff().max()) > 1
    assert eng.sweep(1.0) == delta
    assert torch.equal(eng.get_Z(), Z1)
    assert bool((eng.Zcur[:, d:] == 0).all())                           # the pad columns of a ragged last pack


@pytest.mark.parametrize("run", C.LOAD_RUNS, ids=C.load_id)
def test_integer_data_is_exact_at_every_load_count(k, dev, run):
    """spmm_owned_kernel<4, 32, 6 | 8 | 12> and <4, 64, 8 | 12>: asked for by number, and with 0 chosen by the cache
    hint (6 beyond the caches, else 8, at 32 lanes; 8 at 64).  accumulate_chunk walks a piece 12, 16 or 24 edges per trip
    at 32 lanes and 8 or 12 at 64, masked by the piece's length."""
    C.check_loads(k, dev, *run)


@pytest.mark.parametrize("d,tiles", C.WIDTHS)
@pytest.mark.parametrize("setting", ["H160", "all_phased"])
def test_gaussian_data_against_the_oracle(k, dev, setting, d, tiles):
    X, Z0, P, Z1, delta, gamma = C.gaussian_case(d)
    eng = C.make_engine(k, dev, d, tiles, setting, X, Z0, P)
    twin = C.make_engine(k, dev, d, tiles, setting, X, Z0, P)
    got, again = eng.sweep(gamma), twin.sweep(gamma)
    assert rel(eng.get_Z(), Z1) < TOL and got == pytest.approx(delta, rel=DELTA_RTOL)
    assert got == again and torch.equal(eng.Zcur, twin.Zcur)            # two launches: bitwise equal
    second = eng.sweep(gamma), twin.sweep(gamma)                        # and the next sweep, read from what the first wrote
    assert second[0] == second[1] and torch.equal(eng.Zcur, twin.Zcur)


@pytest.mark.parametrize("d,tiles", C.WIDTHS)
def test_bits_do_not_depend_on_groups_batches_workgroup_or_cache_hint(k, dev, d, tiles):
    """Nor on the row loads in flight: within a (virtual row, step, piece) the fma order is the edge order whatever U.
    The variants: owned_cases.independence_variants -- the earlier groups x batch x hint loop, every load count, a
    one-wave workgroup, 1024 threads."""
    C.check_independence(k, dev, d, tiles)


@pytest.mark.parametrize("d,threads,row_edges", C.STEPS64_RUNS)
def test_sixty_four_steps_are_exact(k, dev, d, threads, row_edges):
    """n_steps = 64 = kOwnedMaxSteps (8 phases x 8 classes, segments of one edge), with workgroups of 64, 256 and 1024
    threads and with virtual rows of at most 64 edges."""
    C.check_steps64(k, dev, d, threads, row_edges)


@pytest.mark.parametrize("d", [128, 254])
def test_shipped_constants_are_exact_with_most_groups_idle(k, dev, d):
    C.check_shipped_constants(k, dev, d)


@pytest.mark.parametrize("d", [128, 136], ids=["lanes32", "lanes64"])
def test_the_lds_grant_grows_to_152_kib(k, dev, d):
    """68 KiB, then 152 KiB of dynamic LDS for one kernel instance: the function attribute is raised twice."""
    C.check_lds_grant_grows(k, dev, d)


@pytest.mark.parametrize("d,tiles", [(128, 1), (256, 2), (130, 1)])
def test_set_owned_replans_between_sweeps(k, dev, d, tiles):
    C.check_set_owned(k, dev, d, tiles)


def test_large_batches_take_the_lds_above_the_default_limit(k, dev):
    """128 sums of 1 KiB: 128 KiB of dynamic LDS, granted through the function attribute."""
    X, Z0, P, Z1, delta = C.integer_case(136)
    eng = C.make_engine(k, dev, 136, 1, "all_phased", X, Z0, P, owned_groups=1, owned_lds_bytes=128 * 1024,
                        owned_block_threads=1024)
    plan = next(o for o in eng.owned_rows if o is not None)[0]
    assert plan.max_batch_vrows * 1024 > 64 * 1024
    assert eng.sweep(1.0) == delta and torch.equal(eng.get_Z(), Z1)


def test_bad_arguments_are_refused_before_any_launch(k, dev):
    X, Z0, P, _, _ = C.integer_case(128)
    eng = C.make_engine(k, dev, 128, 1, "H160", X, Z0, P)
    plan = next(o for o in eng.owned_rows if o is not None)[0]
    Zn = torch.zeros_like(eng.Zcur)
    args = (eng.colidx, eng.P, plan, 256, 0, eng.Zcur, eng.X_loc, 1.0, Zn, 128, eng.partials)
    for bad, err in ((dict(block_threads=100), _hip.ClaneHipError), (dict(d=512), (_hip.ClaneHipError, ValueError)),
                     (dict(partials=eng.partials[:1]), ValueError)):
        a = list(args)
        for name, v in bad.items():
            a[{"block_threads": 3, "d": 9, "partials": 10}[name]] = v
        with pytest.raises(err):
            k.spmm_update_owned(*a)
    with pytest.raises(_hip.ClaneHipError):                           # no instance for narrow rows
        k.spmm_update_owned(eng.colidx, eng.P, plan, 256, 0, eng.Zcur[:, :32], eng.X_loc[:, :32], 1.0, Zn[:, :32], 32,
                            eng.partials)


def test_load_counts_without_an_instance_are_refused_before_any_launch(k, dev):
    """7 or 4 loads at any width, 6 at the 64-lane widths (tests/owned_oracle_kernels.py asserts the same set)."""
    for d, loads in ((128, 7), (128, 4), (136, 6), (130, 6)):
        X, Z0, P, _, _ = C.integer_case(d)
        eng = C.make_engine(k, dev, d, 1, "H160", X, Z0, P)
        Zn = torch.full_like(eng.Zcur, 7.0)
        with pytest.raises(_hip.ClaneHipError, match=f"no instance with {loads} row loads in flight"):
            k.spmm_update_owned(eng.colidx, eng.P, C.the_plan(eng), 256, 0, eng.Zcur, eng.X_loc, 1.0, Zn, d, eng.partials,
                                loads=loads)
        assert bool((Zn == 7.0).all())                                 # nothing ran


def test_propagate_matches_the_chunk_and_combine_run(dev):
    """Embedder.propagate over the same graph, 12 sweeps: sweep count and final delta as without the owned pass.
    The data keep the 12th delta a number the tolerance can be asked of: with zero-mean X every row averages its
    neighbours away and the 12th delta (0.02 over 196 608 elements, 1e-7 each) is the rounding of the stored values, of
    which two summation orders share no digit.  X = N(3, 1) and gamma = 0.95 leave a common component that decays by
    gamma x (the share of non-sink columns, 0.48) per sweep: the 12th delta is some tens, against ~1e-4 of rounding."""
    X = C.gaussian_case(128)[0] + 3.0
    runs = {}
    for owned in (True, False):
        g = Graph.from_csr(C.csr(), X.clone())
        eng = g.engine(dev, class_threshold=64, class_chunk=C.CHUNK, class_owned=owned, owned_max_edges=160,
                       owned_row_edges=C.ROW_EDGES, owned_groups=8, owned_lds_bytes=2048, owned_block_threads=256)
        assert eng.class_owned == owned
        deltas, sweep = [], eng.sweep
        eng.sweep = lambda gamma: deltas.append(sweep(gamma)) or deltas[-1]
        emb = Embedder(g, CosineSimilarity(), torch.device(dev), gamma=0.95, tolerence=12, verbose=False, max_sweeps=12,
                       lagged_check=False)
        emb.propagate()
        assert emb.sweep_counts[-1] == len(deltas)
        runs[owned] = (len(deltas), deltas[-1], eng.get_Z())
        print(f"class_owned={owned}: {len(deltas)} sweeps, deltas {deltas[0]:.6g} .. {deltas[-1]:.9g}")
    (n1, d1, z1), (n0, d0, z0) = runs[True], runs[False]
    assert n1 == n0 == 12 and d1 == pytest.approx(d0, rel=DELTA_RTOL) and rel(z1, z0) < TOL
