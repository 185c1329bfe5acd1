"""The 2-D layout on the GPU (clane_amd/layout.py, csrc/tsne.h): every kernel against the float64 restatement of
tests/layout_cases.py within a bound that is derived there or measured here on the CPU from a float32 emulation, the bit
promises (symmetry, reproducibility), and the surface above the kernels (TSNE, Graph.layout, the CLI's `layout:`
section).  Observed fractions of the bounds on an MI355X: DESIGN 6.16."""
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

from clane_amd import _hip, layout
from clane_amd.engine import SweepEngine
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR

from . import layout_cases as LC
from .conftest import write_data_root

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
U = LC.U


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


def column_mean(k, table, d, rows):
    n = rows.numel()
    sums = torch.empty(d, dtype=torch.float64, device=table.device)
    ws = torch.empty(k.column_sums_ws_len(n, d), dtype=torch.float64, device=table.device)
    k.column_sums(table, d, rows, ws, sums)
    return (sums / n).to(F32)


def run_sqdist(k, table, d, rows):
    n = rows.numel()
    mu = column_mean(k, table, d, rows)
    D = torch.full((n, n), float("nan"), dtype=F32, device=table.device)
    k.tsne_sqdist(table, d, rows, mu, torch.empty(n, dtype=F32, device=table.device), D)
    return D, mu


def listed_values(table, d, rows):
    """The float32 values of the listed rows as the kernel reads them: zeros for an index outside the table."""
    r = rows.long().cpu()
    inside = (r >= 0) & (r < table.shape[0])
    vals = table[:, :d].float().cpu()[r.clamp(0, table.shape[0] - 1)]
    return (vals * inside[:, None]).numpy()


def padded_table(X, dtype, dev, pad=7):
    """X in a wider table whose pad columns are NaN: they are never to be read."""
    t = torch.full((X.shape[0], X.shape[1] + pad), float("nan"), dtype=dtype, device=dev)
    t[:, :X.shape[1]] = torch.as_tensor(X).to(dtype).to(dev)
    return t[:, :X.shape[1]]


def joint_on_gpu(k, dev, n, d, perplexity, seed, dtype=F32):
    """(D, conditional P, beta, joint P, partials) of n Gaussian points, every stage's output kept."""
    table = padded_table(LC.gaussian(n, d, seed=seed), dtype, dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    D, _ = run_sqdist(k, table, d, rows)
    Pc, beta = D.clone(), torch.empty(n, dtype=F32, device=dev)
    k.tsne_affinities(Pc, perplexity, beta)
    P = Pc.clone()
    partials = torch.empty(k.tsne_symmetrize_ws_len(n), dtype=torch.float64, device=dev)
    k.tsne_symmetrize(P, partials)
    return D, Pc, beta, P, partials


# ---- 5. squared distances -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=str)
def test_sqdist_within_the_bound_of_float64(dev, k, dtype):
    """n = 257 rows (three row tiles, two of them partial pairs), d = 33 (two k slices and one column), a shuffled subset
    of a 400-row table with one index outside it."""
    n, d = 257, 33
    table = padded_table(LC.gaussian(400, d, seed=11, scale=2.0, offset=0.5), dtype, dev)
    rows = torch.randperm(400, generator=torch.Generator().manual_seed(5))[:n].to(torch.int32)
    rows[100] = 405
    rows = rows.to(dev)
    D, mu = run_sqdist(k, table, d, rows)
    D64, bound = LC.sqdist(LC.centred(listed_values(table, d, rows), mu.cpu().numpy()))
    got = D.cpu().numpy().astype(np.float64)
    frac = (np.abs(got - D64) / bound)[~np.eye(n, dtype=bool)].max()
    print(f"sqdist {dtype}: worst |D - D64| / bound = {frac:.3f}")
    assert np.isfinite(got).all() and frac <= 1.0
    assert not D.diagonal().any()
    assert torch.equal(D, D.T)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=str)
def test_sqdist_of_a_table_with_a_common_offset(dev, k, dtype):
    """Every column moved by 1000 -- on values for which the move is exact in the table's type -- gives the same D within
    the bound: the centring happens before anything is multiplied."""
    n, d = 257, 33
    ints = torch.randint(-3, 4, (n, d), generator=torch.Generator().manual_seed(6)).double()
    base = (ints * 4.0 if dtype is BF16 else (ints + torch.rand(n, d, generator=torch.Generator().manual_seed(7),
                                                              dtype=torch.float64)).mul(1024).round() / 1024)
    assert torch.equal((base + 1000.0).to(dtype).double(), base + 1000.0) and torch.equal(base.to(dtype).double(), base)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(8)).to(torch.int32).to(dev)
    out = {}
    for name, X in (("plain", base), ("offset", base + 1000.0)):
        table = padded_table(X, dtype, dev)
        D, mu = run_sqdist(k, table, d, rows)
        D64, bound = LC.sqdist(LC.centred(listed_values(table, d, rows), mu.cpu().numpy()))
        got = D.cpu().numpy().astype(np.float64)
        assert (np.abs(got - D64) <= bound).all() and torch.equal(D, D.T) and not D.diagonal().any()
        out[name] = (got, bound)
    diff = np.abs(out["plain"][0] - out["offset"][0])
    both = out["plain"][1] + out["offset"][1]
    off = ~np.eye(n, dtype=bool)
    print(f"offset {dtype}: worst |D - D_offset| / (bound + bound_offset) = {(diff[off] / both[off]).max():.3f}")
    assert (diff <= both).all()


# ---- 6. affinities and the joint probabilities -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,perplexity", [(300, 30.0), (300, 5.0), (130, 40.0)])
def test_affinities_and_joint_probabilities(dev, k, n, perplexity):
    D, Pc, beta, P, partials = joint_on_gpu(k, dev, n, 16, perplexity, seed=2)
    Dh, b = D.cpu().numpy(), beta.cpu().numpy()
    rows_gpu = Pc.cpu().numpy()
    # the entropy of every row, against what a float32 emulation of the same search reaches on the CPU
    emulated, _ = LC.perplexity_search(Dh, perplexity, np.float32)
    dev_emulated = np.abs(LC.row_entropy(emulated) - np.log(perplexity)).max()
    dev_gpu = np.abs(LC.row_entropy(rows_gpu) - np.log(perplexity)).max()
    print(f"affinities n={n} perplexity={perplexity:g}: worst |H - ln perplexity| kernel {dev_gpu:.3g}, float32 emulation "
          f"{dev_emulated:.3g} (T_H = 4x)")
    assert dev_gpu <= 4.0 * dev_emulated
    assert not Pc.diagonal().any() and bool((Pc >= 0).all())
    sums = rows_gpu.astype(np.float64).sum(1)
    print(f"  worst |row sum - 1| / ((n + 2) u) = {np.abs(sums - 1).max() / ((n + 2) * U):.3f}")
    assert (np.abs(sums - 1.0) <= (n + 2) * U).all()
    # the rows at the kernel's own beta, then the symmetrised matrix, against float64
    cb = LC.conditional_bound(Dh, b)
    c64 = LC.conditional_at(Dh, b)
    print(f"  worst |p - p64| / bound = {(np.abs(rows_gpu - c64) / cb).max():.3f}")
    assert (np.abs(rows_gpu - c64) <= cb).all()
    P64 = LC.joint(c64)
    pb = (cb + cb.T) / (2.0 * n) + 2.0 * U * P64
    got = P.cpu().numpy().astype(np.float64)
    print(f"  worst |P - P64| / bound = {(np.abs(got - P64)[P64 > 0] / pb[P64 > 0]).max():.3f}; "
          f"{int((P64 <= LC.EPS).sum()) - n} entries at the floor")
    assert (np.abs(got - P64) <= pb).all()
    assert torch.equal(P, P.T) and not P.diagonal().any()
    assert float(P[~torch.eye(n, dtype=torch.bool, device=dev)].min()) >= LC.EPS32
    total = float(np.cumsum(partials.cpu().numpy())[-1])
    assert abs(total - LC.plogp(got)) <= 1e-12 * abs(LC.plogp(got))


def test_affinities_of_equidistant_points_are_uniform(dev, k):
    """Every other point at one distance: no beta reaches the perplexity, the search runs out of steps, the row is uniform."""
    n = 130
    D = torch.full((n, n), 3.0, dtype=F32, device=dev)
    D.fill_diagonal_(0.0)
    beta = torch.empty(n, dtype=F32, device=dev)
    k.tsne_affinities(D, 40.0, beta)
    off = ~torch.eye(n, dtype=torch.bool, device=dev)
    assert not D.diagonal().any() and bool(torch.isfinite(beta).all())
    assert float((D[off].double() - 1.0 / (n - 1)).abs().max()) <= 2 * U / (n - 1)


# ---- 7. forces and the update -------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def joint_257():
    k, dev = _hip.kernels(), _hip.require_gpu("cuda:0")
    return joint_on_gpu(k, dev, 257, 16, 30.0, seed=3)[3:]


@pytest.mark.parametrize("alpha", [1.0, 12.0])
@pytest.mark.parametrize("scale", [1e-4, 10.0])
def test_forces_and_step_within_the_bounds_of_float64(dev, k, scale, alpha):
    n = 257
    P, partials = joint_257()
    Yh = LC.layout_at(n, scale)
    Y = torch.from_numpy(Yh).to(dev)
    F = torch.full((n, 6), float("nan"), dtype=F32, device=dev)
    k.tsne_forces(P, Y, F)
    got = F.cpu().numpy().astype(np.float64)
    P64 = P.cpu().numpy().astype(np.float64)
    ref = LC.forces(P64, Yh.astype(np.float64))
    ba, br, bl = ((n + 8) * U * ref[key] for key in ("abs_attr", "abs_rep", "abs_l"))
    fa, fr = np.abs(got[:, 0:2] - ref["attr"]) / ba, np.abs(got[:, 2:4] - ref["rep"]) / br
    fl = np.abs(got[:, 5] - ref["l"]) / bl
    S64 = ref["s"].sum()
    print(f"forces scale={scale:g}: worst fraction of the bound: attr {fa.max():.3f}, rep {fr.max():.3f}, l {fl.max():.3f}, "
          f"S {abs(got[:, 4].sum() - S64) / (n * U * S64):.3f}")
    assert fa.max() <= 1.0 and fr.max() <= 1.0 and fl.max() <= 1.0
    assert (np.abs(got[:, 4] - ref["s"]) <= n * U * ref["s"]).all()
    # the other instance of the kernel and the variant without the KL terms give the same bits
    F2 = torch.empty_like(F)
    k.tsne_forces(P, Y, F2, cached=True)
    assert torch.equal(F2, F)
    k.tsne_forces(P, Y, F2, kl=False)
    assert torch.equal(F2[:, :5], F[:, :5]) and not F2[:, 5].any()

    # one update: gains in [0.5, 2) with a few about to hit the floor, velocities of both signs and some zeros
    gen = torch.Generator().manual_seed(9)
    V0 = torch.randn(n, 2, generator=gen) * float(scale) * 0.1
    V0[::7] = 0.0
    G0 = torch.rand(n, 2, generator=gen) * 1.5 + 0.5
    G0[::7] = 0.011
    momentum, lr = 0.5, 50.0
    plogp = float(np.cumsum(partials.cpu().numpy())[-1])
    V, G = V0.to(dev), G0.to(dev)
    Yn = torch.full_like(Y, float("nan"))
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    k.tsne_step(F, Y, alpha, momentum, lr, plogp, V, G, Yn, stats)
    kl, gnorm, S, L = stats.tolist()
    assert abs(S - S64) <= n * U * S64
    kl64, g64, _ = LC.objective(P64, Yh.astype(np.float64), alpha)
    kl_bound = bl.sum() + n * U + 1e-12 * abs(kl64)
    print(f"  KL {kl:.9g} vs {kl64:.9g}: |diff| / bound = {abs(kl - kl64) / kl_bound:.3f}")
    assert abs(kl - kl64) <= kl_bound
    g_bound = 4.0 * (alpha * ba + br / S64 + np.abs(ref["rep"]) / S64 * 2 * n * U)
    assert abs(gnorm - np.linalg.norm(g64)) <= np.linalg.norm(g_bound) + 1e-12 * np.linalg.norm(g64)
    Y64, V64, G64 = LC.update(g64, Yh.astype(np.float64), V0.double().numpy(), G0.double().numpy(), momentum, lr)
    sure = (V0.numpy() == 0) | (np.abs(g64) > g_bound)          # the sign of v g is the same in both
    print(f"  the update's sign test is decided for {sure.mean():.4f} of the coordinates")
    assert sure.mean() >= 0.99 and sure[::7].all()
    Gg, Vg, Yg = (t.cpu().numpy().astype(np.float64) for t in (G, V, Yn))
    assert (np.abs(Gg - G64)[sure] <= 2 * U * G64[sure]).all()
    assert (Gg[::7] == np.float32(0.01)).all()                   # 0.011 * 0.8 is below the floor
    v_bound = lr * G64 * g_bound + 2 * U * (np.abs(V64) + lr * G64 * np.abs(g64))
    assert (np.abs(Vg - V64)[sure] <= v_bound[sure]).all()
    assert (np.abs(Yg - Y64)[sure] <= (v_bound + U * (np.abs(Y64) + np.abs(V64)))[sure]).all()
    assert torch.equal(Y.cpu(), torch.from_numpy(Yh))            # the operand was not written


# ---- the fit ---------------------------------------------------------------------------------------------------------------
def ring_engine(X, dtype, dev, step=1):
    V = X.shape[0]
    csr = HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + step) % V).astype(np.int32))
    return SweepEngine(csr, torch.as_tensor(X).to(dtype), dev)


def fit_rows(eng, n, dev, init=None, **kw):
    t = layout.TSNE(eng, **kw)
    tab, rows = t.table_and_rows(torch.arange(n), "Z")
    return t.fit(tab, rows, init=init), t


def test_two_fits_give_the_same_bits_whatever_else_is_in_the_table(dev):
    X = LC.gaussian(500, 16, seed=4)
    with torch.cuda.device(dev):
        a, _ = fit_rows(ring_engine(X[:300], F32, dev), 300, dev, max_iter=60)
        b, _ = fit_rows(ring_engine(X[:300], F32, dev), 300, dev, max_iter=60)
        assert a.iterations == 60 and len(a.kl_trace) == 1
        assert torch.equal(a.Y, b.Y) and a.kl_trace == b.kl_trace and torch.equal(a.beta, b.beta)
        assert (a.kl, a.kl_init, a.grad_norm) == (b.kl, b.kl_init, b.grad_norm)
        c, _ = fit_rows(ring_engine(X, F32, dev), 300, dev, max_iter=60)
        assert torch.equal(c.beta, a.beta) and torch.equal(c.Y, a.Y)


def test_ten_iterations_follow_the_float64_restatement(dev, k):
    """Y after 10 iterations from a given layout against the float64 restatement on the kernel's own P; allowed: 10 times
    what a float32 numpy emulation of the same 10 iterations deviates by (the sums' orders differ)."""
    n = 300
    X = LC.gaussian(n, 16, seed=2)
    Y0 = LC.layout_at(n, 1e-4, seed=5)
    with torch.cuda.device(dev):
        eng = ring_engine(X, F32, dev)
        fit, t = fit_rows(eng, n, dev, init=torch.from_numpy(Y0), max_iter=10)
        tab, rows = t.table_and_rows(torch.arange(n), "Z")
        P, _, _ = t.joint_probabilities(tab, rows)
    assert fit.iterations == 10
    P64 = P.cpu().numpy().astype(np.float64)
    lr = t.learning_rate_for(n)
    Y64 = LC.trajectory(P64, Y0, 10, 12.0, 0.5, lr)
    Y32 = LC.trajectory(P64, Y0, 10, 12.0, 0.5, lr, np.float32)
    allowed = 10.0 * np.abs(Y32.astype(np.float64) - Y64).max()
    err = np.abs(fit.Y.cpu().numpy().astype(np.float64) - Y64).max()
    print(f"10 iterations: max |Y - Y64| = {err:.3g}, float32 emulation {allowed / 10:.3g}, max |Y64| = {np.abs(Y64).max():.3g}")
    assert err <= allowed


# ---- 10. end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=str)
def test_three_blobs_come_apart(dev, dtype):
    X, y = LC.blobs()
    with torch.cuda.device(dev):
        fit, _ = fit_rows(ring_engine(X, dtype, dev), 300, dev, max_iter=500)
    agreement = layout.neighbour_agreement(fit.Y, torch.from_numpy(y).to(dev), k=5)
    print(f"blobs {dtype}: KL {fit.kl_init:.4f} -> {fit.kl:.4f} in {fit.iterations} iterations, agreement {agreement}")
    assert fit.iterations == 500 and len(fit.kl_trace) == 10 and tuple(fit.Y.shape) == (300, 2)
    assert fit.kl < fit.kl_init
    assert agreement == 1.0


def class_graph(X, step=3):
    V = X.shape[0]
    return HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + step) % V).astype(np.int32))


def test_graph_layout_reads_the_table_and_changes_nothing(dev):
    X, y = LC.blobs()
    g = Graph.from_csr(class_graph(X), torch.from_numpy(X))
    eng = g.engine()
    Z0 = eng.get_Z()
    names = [f"c{c}" for c in y]
    Y, vertices, info = g.layout(labels=names, max_iter=500)
    assert tuple(Y.shape) == (300, 2) and not Y.is_cuda and torch.equal(vertices, torch.arange(300))
    assert info["n"] == 300 and info["sampled"] is False and info["table"] == "Z" and info["perplexity"] == 30.0
    assert info["iterations"] == 500 and len(info["kl_trace"]) == 10 and info["kl"] < info["kl_init"]
    assert info["classes"] == names and info["neighbour_agreement"] == 1.0
    with torch.cuda.device(dev):
        direct, _ = fit_rows(eng, 300, dev, max_iter=500)
    assert torch.equal(direct.Y.cpu(), Y)
    # a sample: seeded, sorted, Y in its order; labels for a subset only
    Ys, vs, infos = g.layout(table="X", max_points=100, seed=4, max_iter=50, labels=([0, 1, 2], ["a", "b", "a"]))
    expect, _ = layout.sample_vertices(300, 100, 4)
    assert torch.equal(vs, expect) and tuple(Ys.shape) == (100, 2) and infos["sampled"] is True and infos["n"] == 100
    assert infos["neighbour_agreement"] is None and infos["iterations"] == 50
    with torch.cuda.device(dev):
        t = layout.TSNE(eng, max_iter=50)
        again = t.fit(*t.table_and_rows(expect, "X"))
    assert torch.equal(again.Y.cpu(), Ys)
    assert torch.equal(eng.get_Z(), Z0)
    with pytest.raises(ValueError, match="must be below n = 20"):
        g.layout(vertices=list(range(20)))


CONFIG = ("graph:\n  embedding_dim: 16\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")
REPORT_KEYS = {"n", "sampled", "perplexity", "iterations", "kl", "kl_init", "grad_norm", "kl_trace"}


def test_cli_writes_the_layout(dev, tmp_path):
    import clane_amd.__main__ as M
    X, y = LC.blobs()
    ids = [f"v{i}" for i in range(300)]
    src, dst = ids, [ids[(i + 3) % 300] for i in range(300)]         # every edge stays inside its class
    root = write_data_root(tmp_path / "blobs", ids, src, dst, X)
    (root / "Y").write_text("".join(f"{ids[i]}\tclass{y[i]}\n" for i in range(300)))

    def run(extra, out):
        cfg = tmp_path / f"{out}.yaml"
        cfg.write_text(CONFIG + extra)
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg), "--gpu"]))
        return tmp_path / out
    out = run("\nlayout:\n  max_iter: 500\n  labels: Y\n  baseline: true\n", "full")
    rep = json.loads((out / "layout.json").read_text())
    assert set(rep) == REPORT_KEYS | {"neighbour_agreement", "baseline"}
    assert set(rep["baseline"]) == REPORT_KEYS | {"neighbour_agreement"}
    assert rep["n"] == 300 and rep["sampled"] is False and rep["perplexity"] == 30.0 and rep["iterations"] == 500
    assert len(rep["kl_trace"]) == 10 and rep["kl"] < rep["kl_init"] and rep["baseline"]["kl"] < rep["baseline"]["kl_init"]
    assert rep["baseline"]["neighbour_agreement"] == 1.0            # X is the blobs themselves
    assert 0.9 < rep["neighbour_agreement"] <= 1.0                  # Z: every vertex pulled towards its own class
    for name in ("layout.tsv", "layout_X.tsv"):
        lines = (out / name).read_text().splitlines()
        assert len(lines) == 300
        for i, line in enumerate(lines):
            vid, xs, ys, cls = line.split("\t")
            assert vid == ids[i] and cls == f"class{y[i]}" and np.isfinite(float(xs)) and np.isfinite(float(ys))
    Z = torch.from_numpy(np.load(out / "Z.npy"))
    xy = np.array([[float(f) for f in line.split("\t")[1:3]] for line in (out / "layout.tsv").read_text().splitlines()])
    g = Graph.from_csr(class_graph(X), torch.from_numpy(X))
    g.set_Z(Z)
    Yg, _, _ = g.layout(max_iter=500)
    assert np.array_equal(xy.astype(np.float32), Yg.numpy())          # the file holds what Graph.layout returns

    some = run("\nlayout:\n  max_points: 100\n  seed: 4\n  max_iter: 50\n", "sample")
    rep = json.loads((some / "layout.json").read_text())
    assert set(rep) == REPORT_KEYS and rep["sampled"] is True and rep["n"] == 100 and rep["iterations"] == 50
    expect, _ = layout.sample_vertices(300, 100, 4)
    lines = (some / "layout.tsv").read_text().splitlines()
    assert [line.split("\t")[0] for line in lines] == [ids[v] for v in expect.tolist()]
    assert all(len(line.split("\t")) == 3 for line in lines) and not (some / "layout_X.tsv").exists()
    plain = run("", "plain")
    assert (plain / "Z.npy").exists() and not (plain / "layout.json").exists() and not (plain / "layout.tsv").exists()
    assert (plain / "Z.npy").read_bytes() == (out / "Z.npy").read_bytes()


# ---- 11. refusals -------------------------------------------------------------------------------------------------------------
class NoKernels:
    def __getattr__(self, name):
        raise AssertionError(f"kernel {name} was reached")


class EngineView:
    """What TSNE looks at, with kernels that must not be reached."""
    world, columns, halo, exchange, d = 1, False, False, "none", 16

    def __init__(self, dev):
        self.device, self.k = dev, NoKernels()


def test_refusals_come_before_any_kernel(dev):
    Z = torch.zeros(8, 16, dtype=F32, device=dev)

    def rows(n):
        return torch.zeros(n, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="perplexity = 300 must be below n = 300"):
        layout.TSNE(EngineView(dev), perplexity=300).fit(Z, rows(300))
    with pytest.raises(ValueError, match="at least 4 points, got n = 3"):
        layout.TSNE(EngineView(dev), perplexity=2).fit(Z, rows(3))
    before = torch.cuda.memory_allocated(dev)
    t = layout.TSNE(EngineView(dev))
    with pytest.raises(ValueError, match="n = 65537 exceeds 65536 points"):
        t.check_points(65537)                                    # arithmetic only
    with pytest.raises(ValueError, match="n = 65537 exceeds 65536 points"):
        t.fit(Z, torch.empty(65537, dtype=torch.int32, device="meta"))
    assert torch.cuda.memory_allocated(dev) == before
    with pytest.raises(ValueError, match=r"init must be \[300, 2\]"):
        layout.TSNE(EngineView(dev)).fit(Z, rows(300), init=torch.zeros(300, 3))

    class Divided(EngineView):
        world, exchange = 2, "halo"
    with pytest.raises(NotImplementedError, match="t-SNE runs on ONE GPU only"):
        layout.TSNE(Divided(dev))


def test_a_fit_that_cannot_fit_says_how_many_points_would(dev, monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d=None: (1 << 30, 1 << 30))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda d=None: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda d=None: 0)
    with pytest.raises(_hip.ClaneHipError, match=r"about 15\d\d\d points would fit"):
        layout.TSNE(EngineView(dev))._check_memory(40000, dev)
