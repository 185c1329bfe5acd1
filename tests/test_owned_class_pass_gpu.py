"""spmm_owned_kernel on the GPU, driven by SweepEngine over the graph of tests/owned_cases.py: rows of 65..300 edges over
all 8 classes, a row with an empty class, rows of exactly H and H + 1 edges, a segment of several pieces, rows cut into
virtual rows, more rows than a batch holds, rows of <= 64 edges and sinks beside them.  Widths: 512-byte rows, two
column tiles of them, ragged 1-KiB rows (d = 136: the c0 < d mask)."""
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
    X, Z0, P, _, _, gamma = C.gaussian_case(d)
    seen = None
    for groups in (8, 16, 24):
        for vrows in (C.BATCH_VROWS, 16):
            for hint in (False, True):
                eng = C.make_engine(k, dev, d, tiles, "all_phased", X, Z0, P, owned_groups=groups,
                                    owned_lds_bytes=vrows * C.sum_bytes(d, tiles),
                                    owned_block_threads=512 if groups == 16 else 256)
                eng.beyond_cache = hint
                out = (eng.sweep(gamma), eng.Zcur.clone())
                if seen is None:
                    seen = out
                assert out[0] == seen[0] and torch.equal(out[1], seen[1]), (groups, vrows, hint)


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
