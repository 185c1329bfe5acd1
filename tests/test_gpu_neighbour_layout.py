"""The neighbour-sparse 2-D layout on the GPU (clane_amd/layout.py NeighbourTSNE / KNeighbours, csrc/tsne_nn.h): the
neighbour search against the exact path's own bits, every other kernel against the float64 restatement of
tests/neighbour_layout_cases.py within a bound that is derived there or measured here on the CPU from a float32
emulation, the bit promises (symmetry, reproducibility, independence of n_slabs), and the surface above the kernels
(Graph.layout(method="neighbours"), Graph.neighbours, the CLI's `layout:` section).  Observed fractions of the bounds on
an MI355X: DESIGN 6.18."""
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

from clane_amd import _hip, layout
from clane_amd.graph import Graph

from . import layout_cases as LC
from . import neighbour_layout_cases as NC
from .conftest import write_data_root
from .test_gpu_layout import (CONFIG, REPORT_KEYS, EngineView, class_graph, column_mean, padded_table, ring_engine,
                              run_sqdist)

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
U = LC.U


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


def run_knn(k, table, d, rows, kk, n_slabs=1, poison=True):
    """(ids, sqdist) of the raw kernel; the outputs and the candidate workspace start as NaN / a poison index."""
    n, dev = rows.numel(), table.device
    ids = torch.full((n, kk), -7, dtype=torch.int32, device=dev)
    sqd = torch.full((n, kk), float("nan"), dtype=F32, device=dev)
    ci = cd = None
    if n_slabs > 1:
        ci = torch.full((n * n_slabs * kk,), -7, dtype=torch.int32, device=dev)
        cd = torch.full((n * n_slabs * kk,), float("nan"), dtype=F32, device=dev)
    k.knn_sqdist(table, d, rows, column_mean(k, table, d, rows), torch.empty(n, dtype=F32, device=dev), ids, sqd, n_slabs,
                 ci, cd)
    return ids, sqd


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ---- 1. the neighbour search against the exact path's bits -------------------------------------------------------------------
@lru_cache(maxsize=None)
def search_case(dtype):
    """n = 257 listed rows (three candidate tiles, the last with one row) of a 400-row table, d = 33 (two k slices and one
    column), one index outside the table, ten table rows listed twice -- their distances tie bit for bit, so the order
    by position decides; (table, rows, D of the exact path on the host)."""
    k, dev = _hip.kernels(), _hip.require_gpu("cuda:0")
    n, d = 257, 33
    table = padded_table(LC.gaussian(400, d, seed=11, scale=2.0, offset=0.5), dtype, dev)
    rows = torch.randperm(400, generator=torch.Generator().manual_seed(5))[:n].to(torch.int32)
    rows[100] = 405
    rows[200:210] = rows[20:30]
    rows = rows.to(dev)
    D, _ = run_sqdist(k, table, d, rows)
    return table, rows, D.cpu().numpy()


@pytest.mark.parametrize("kk", [7, 90, 192])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=str)
def test_knn_is_the_top_k_of_the_exact_distances_bit_for_bit(dev, k, dtype, kk):
    """k = 7, 90, 192: the three query tiles (128, 64, 32 queries per workgroup); one slab and three."""
    table, rows, D = search_case(dtype)
    want_ids, want_sq = NC.knn(D, kk)
    ties = (want_sq[:, 1:] == want_sq[:, :-1]).sum()
    assert ties >= 10 or kk == 7
    out = {}
    for n_slabs in (1, 3):
        ids, sqd = run_knn(k, table, 33, rows, kk, n_slabs)
        out[n_slabs] = (ids, sqd)
        assert np.array_equal(ids.cpu().numpy(), want_ids)
        assert same_bits(sqd.cpu().numpy(), want_sq)
    assert torch.equal(out[1][0], out[3][0]) and torch.equal(out[1][1], out[3][1])
    print(f"knn {dtype} k={kk}: {int(ties)} ties by position among the listed neighbours")


@pytest.mark.parametrize("kk", [4, 7])
def test_knn_of_five_rows_marks_the_places_it_cannot_fill(dev, k, kk):
    table = padded_table(LC.gaussian(5, 6, seed=1), F32, dev)
    rows = torch.arange(5, dtype=torch.int32, device=dev)
    D, _ = run_sqdist(k, table, 6, rows)
    want_ids, want_sq = NC.knn(D.cpu().numpy(), kk)
    for n_slabs in (1, 2):
        ids, sqd = run_knn(k, table, 6, rows, kk, n_slabs)
        assert np.array_equal(ids.cpu().numpy(), want_ids) and same_bits(sqd.cpu().numpy(), want_sq)
    if kk == 7:
        assert bool((ids[:, 4:] == -1).all()) and bool(torch.isinf(sqd[:, 4:]).all()) and bool((ids[:, :4] >= 0).all())


# ---- 2, 3. affinities and the joint probabilities ----------------------------------------------------------------------------
def neighbours_of_gaussian(k, dev, n, d, kk, seed):
    table = padded_table(LC.gaussian(n, d, seed=seed), F32, dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    return run_knn(k, table, d, rows, kk, layout.knn_slabs(n, kk))


def conditionals_on_gpu(k, dev, n, d, kk, perplexity, seed):
    ids, sqd = neighbours_of_gaussian(k, dev, n, d, kk, seed)
    p = torch.full_like(sqd, float("nan"))
    beta = torch.empty(n, dtype=F32, device=dev)
    k.tsne_nn_affinities(sqd, ids, perplexity, p, beta)
    return ids, sqd, p, beta


def plogp_on_gpu(k, P):
    row = torch.full((P.n,), float("nan"), dtype=torch.float64, device=P.val.device)
    k.tsne_nn_plogp(P.rowptr, P.val, row)
    return float(np.cumsum(row.cpu().numpy())[-1])


@pytest.mark.parametrize("n,kk,perplexity", [(300, 90, 30.0), (300, 15, 5.0), (130, 129, 40.0)])
def test_affinities_and_the_sparse_joint_probabilities(dev, k, n, kk, perplexity):
    ids, sqd, p, beta = conditionals_on_gpu(k, dev, n, 16, kk, perplexity, seed=2)
    idh, sqh, b, rows_gpu = ids.cpu().numpy(), sqd.cpu().numpy(), beta.cpu().numpy(), p.cpu().numpy()
    assert (idh >= 0).all()
    # the entropy of every row, against what a float32 emulation of the same search reaches on the CPU
    emulated, _ = NC.perplexity_search(sqh, idh, perplexity, np.float32)
    dev_emulated = np.abs(LC.row_entropy(emulated) - np.log(perplexity)).max()
    dev_gpu = np.abs(LC.row_entropy(rows_gpu) - np.log(perplexity)).max()
    print(f"nn affinities n={n} k={kk} perplexity={perplexity:g}: worst |H - ln perplexity| kernel {dev_gpu:.3g}, float32 "
          f"emulation {dev_emulated:.3g} (T_H = 4x)")
    assert dev_gpu <= 4.0 * dev_emulated
    assert bool((p >= 0).all())
    sums = rows_gpu.astype(np.float64).sum(1)
    print(f"  worst |row sum - 1| / ((k + 2) u) = {np.abs(sums - 1).max() / ((kk + 2) * U):.3f}")
    assert (np.abs(sums - 1.0) <= (kk + 2) * U).all()
    cb = NC.conditional_bound(sqh, idh, b)
    c64 = NC.conditional_at(sqh, idh, b)
    print(f"  worst |p - p64| / bound = {(np.abs(rows_gpu - c64) / cb).max():.3f}")
    assert (np.abs(rows_gpu - c64) <= cb).all()

    # the joint probabilities: structure, symmetry in bits, values, sum p ln p
    P = layout.sparse_joint(ids, p)
    rowptr, cols = P.rowptr.cpu().numpy(), P.cols.cpu().numpy()
    assert P.rowptr.dtype == torch.int64 and P.cols.dtype == torch.int32 and P.val.dtype == F32
    assert rowptr[0] == 0 and rowptr[-1] == P.nnz == cols.size and (np.diff(rowptr) >= 0).all()
    r = np.repeat(np.arange(n), np.diff(rowptr))
    assert (np.diff(r.astype(np.int64) * n + cols) > 0).all()             # ascending within every row, no place twice
    assert (cols != r).all() and cols.min() >= 0 and cols.max() < n
    P64, union = NC.joint(idh, c64)
    got32, stored = NC.csr_dense(rowptr, cols, P.val.cpu().numpy(), np.float32)
    assert np.array_equal(stored, union) and P.nnz == int(union.sum())
    assert same_bits(got32, got32.T)
    cbd, _ = NC.scatter(idh, cb)
    pb = (cbd + cbd.T) / (2.0 * n) + 2.0 * U * P64
    got = got32.astype(np.float64)
    print(f"  worst |P - P64| / bound = {(np.abs(got - P64)[union] / pb[union]).max():.3f}; nnz {P.nnz} of {2 * n * kk}")
    assert (np.abs(got - P64) <= pb).all() and (got[union] > 0).all()
    total = plogp_on_gpu(k, P)
    assert abs(total - LC.plogp(got)) <= 1e-12 * abs(LC.plogp(got))


def test_affinities_of_equidistant_neighbours_are_uniform(dev, k):
    """Every neighbour at one distance: no beta reaches the perplexity, the search runs out of steps, the row is uniform --
    over the neighbours there are: the last five places of every other row hold none."""
    n, kk = 130, 129
    sqd = torch.full((n, kk), 3.0, dtype=F32, device=dev)
    ids = torch.arange(1, kk + 1, dtype=torch.int32, device=dev).repeat(n, 1)
    ids[::2, -5:] = -1
    sqd[::2, -5:] = float("inf")
    p = torch.full_like(sqd, float("nan"))
    beta = torch.empty(n, dtype=F32, device=dev)
    k.tsne_nn_affinities(sqd, ids, 40.0, p, beta)
    assert bool(torch.isfinite(beta).all()) and not p[::2, -5:].any()
    assert float((p[1::2].double() - 1.0 / kk).abs().max()) <= 2 * U / kk
    assert float((p[::2, :-5].double() - 1.0 / (kk - 5)).abs().max()) <= 2 * U / (kk - 5)


# ---- 4. forces and the update ---------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def joint_257():
    k, dev = _hip.kernels(), _hip.require_gpu("cuda:0")
    ids, _, p, _ = conditionals_on_gpu(k, dev, 257, 16, 90, 30.0, seed=3)
    P = layout.sparse_joint(ids, p)
    return P, plogp_on_gpu(k, P)


def run_forces(k, P, Y, kl=True):
    F = torch.full((Y.shape[0], 6), float("nan"), dtype=F32, device=Y.device)
    k.tsne_nn_attract(P.rowptr, P.cols, P.val, Y, F, kl=kl)
    k.tsne_repulse(Y, F)
    return F


@pytest.mark.parametrize("scale", [1e-4, 10.0])
def test_forces_and_step_within_the_bounds_of_float64(dev, k, scale):
    n = 257
    P, plogp = joint_257()
    Yh = LC.layout_at(n, scale)
    Y = torch.from_numpy(Yh).to(dev)
    F = run_forces(k, P, Y)
    got = F.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    P64, _ = NC.csr_dense(P.rowptr.cpu().numpy(), P.cols.cpu().numpy(), P.val.cpu().numpy())
    ref = LC.forces(P64, Yh.astype(np.float64))
    nnz_row = np.diff(P.rowptr.cpu().numpy()).astype(np.float64)
    ba, bl = (nnz_row[:, None] + 8) * U * ref["abs_attr"], (nnz_row + 8) * U * ref["abs_l"]
    br, bs = (n + 8) * U * ref["abs_rep"], (n + 8) * U * ref["s"]
    fa, fr = np.abs(got[:, 0:2] - ref["attr"]) / ba, np.abs(got[:, 2:4] - ref["rep"]) / br
    fl, fs = np.abs(got[:, 5] - ref["l"]) / bl, np.abs(got[:, 4] - ref["s"]) / bs
    print(f"nn forces scale={scale:g}: worst fraction of the bound: attr {fa.max():.3f}, rep {fr.max():.3f}, "
          f"l {fl.max():.3f}, s {fs.max():.3f}")
    assert fa.max() <= 1.0 and fr.max() <= 1.0 and fl.max() <= 1.0 and fs.max() <= 1.0
    # without the KL terms: the same bits elsewhere, zeros in column 5; and a second call gives the same bits
    F2 = run_forces(k, P, Y, kl=False)
    assert torch.equal(F2[:, :5], F[:, :5]) and not F2[:, 5].any()
    assert torch.equal(run_forces(k, P, Y), F)

    # one update through the existing kernel: KL of the sparse P against the float64 objective
    S64 = ref["s"].sum()
    V, G = torch.zeros_like(Y), torch.ones_like(Y)
    Yn = torch.full_like(Y, float("nan"))
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    k.tsne_step(F, Y, 1.0, 0.5, 50.0, plogp, V, G, Yn, stats)
    kl, gnorm, S, L = stats.tolist()
    assert abs(S - S64) <= (n + 8) * U * S64
    kl64, g64, _ = LC.objective(P64, Yh.astype(np.float64), 1.0)
    kl_bound = bl.sum() + n * U + 1e-12 * abs(kl64)
    print(f"  KL {kl:.9g} vs {kl64:.9g}: |diff| / bound = {abs(kl - kl64) / kl_bound:.3f}")
    assert abs(kl - kl64) <= kl_bound
    g_bound = 4.0 * (ba + br / S64 + np.abs(ref["rep"]) / S64 * 2 * n * U)
    assert abs(gnorm - np.linalg.norm(g64)) <= np.linalg.norm(g_bound) + 1e-12 * np.linalg.norm(g64)
    assert bool(torch.isfinite(Yn).all()) and torch.equal(Y.cpu(), torch.from_numpy(Yh))


def test_repulsion_across_the_chunk_boundary(dev, k):
    """n = 2050: two points past the 2048 staged in LDS at a time; the rows of the last workgroup see their own chunk last."""
    n = 2050
    Yh = LC.layout_at(n, 3.0, seed=2)
    Y = torch.from_numpy(Yh).to(dev)
    F = torch.full((n, 6), float("nan"), dtype=F32, device=dev)
    k.tsne_repulse(Y, F)
    assert bool(torch.isnan(F[:, [0, 1, 5]]).all())                    # the attraction's columns are left alone
    got = F[:, 2:5].cpu().numpy().astype(np.float64)
    Y64 = Yh.astype(np.float64)
    diff = Y64[:, None, :] - Y64[None, :, :]
    q = 1.0 / (1.0 + (diff * diff).sum(2))
    rep, abs_rep = ((q * q)[:, :, None] * diff).sum(1), ((q * q)[:, :, None] * np.abs(diff)).sum(1)
    s = q.sum(1) - 1.0
    fr = np.abs(got[:, 0:2] - rep) / ((n + 8) * U * abs_rep)
    fs = np.abs(got[:, 2] - s) / ((n + 8) * U * s)
    print(f"repulsion n={n}: worst fraction of the bound: rep {fr.max():.3f}, s {fs.max():.3f}")
    assert fr.max() <= 1.0 and fs.max() <= 1.0
    F2 = torch.zeros_like(F)
    k.tsne_repulse(Y, F2)
    assert torch.equal(F2[:, 2:5], F[:, 2:5])


# ---- 5. the fit --------------------------------------------------------------------------------------------------------------
def fit_rows(eng, n, init=None, **kw):
    t = layout.NeighbourTSNE(eng, **kw)
    tab, rows = t.table_and_rows(torch.arange(n), "Z")
    return t.fit(tab, rows, init=init), t


def test_two_fits_give_the_same_bits_whatever_else_is_in_the_table(dev):
    X = LC.gaussian(500, 16, seed=4)
    with torch.cuda.device(dev):
        a, _ = fit_rows(ring_engine(X[:300], F32, dev), 300, max_iter=60)
        b, _ = fit_rows(ring_engine(X[:300], F32, dev), 300, max_iter=60)
        assert a.iterations == 60 and len(a.kl_trace) == 1 and a.neighbours == 90 and 300 * 90 <= a.nnz <= 2 * 300 * 90
        assert torch.equal(a.Y, b.Y) and a.kl_trace == b.kl_trace and torch.equal(a.beta, b.beta) and a.nnz == b.nnz
        assert (a.kl, a.kl_init, a.grad_norm) == (b.kl, b.kl_init, b.grad_norm)
        c, _ = fit_rows(ring_engine(X, F32, dev), 300, max_iter=60)
        assert torch.equal(c.beta, a.beta) and torch.equal(c.Y, a.Y)


def test_ten_iterations_follow_the_float64_restatement(dev, k):
    """Y after 10 iterations from a given layout against the float64 restatement on the kernel's own CSR; allowed: 10 times
    what a float32 numpy emulation of the same 10 iterations deviates by (the sums' orders differ)."""
    n = 300
    X = LC.gaussian(n, 16, seed=2)
    Y0 = LC.layout_at(n, 1e-4, seed=5)
    with torch.cuda.device(dev):
        eng = ring_engine(X, F32, dev)
        fit, t = fit_rows(eng, n, init=torch.from_numpy(Y0), max_iter=10)
        tab, rows = t.table_and_rows(torch.arange(n), "Z")
        P, _, _ = t.joint_probabilities(tab, rows)
    assert fit.iterations == 10 and fit.nnz == P.nnz
    P64, _ = NC.csr_dense(P.rowptr.cpu().numpy(), P.cols.cpu().numpy(), P.val.cpu().numpy())
    lr = t.learning_rate_for(n)
    Y64 = NC.trajectory(P64, Y0, 10, 12.0, 0.5, lr)
    Y32 = NC.trajectory(P64, Y0, 10, 12.0, 0.5, lr, np.float32)
    allowed = 10.0 * np.abs(Y32.astype(np.float64) - Y64).max()
    err = np.abs(fit.Y.cpu().numpy().astype(np.float64) - Y64).max()
    print(f"nn 10 iterations: max |Y - Y64| = {err:.3g}, float32 emulation {allowed / 10:.3g}, max |Y64| = "
          f"{np.abs(Y64).max():.3g}")
    assert err <= allowed


@pytest.mark.parametrize("dtype", [F32, BF16], ids=str)
def test_three_blobs_come_apart(dev, dtype):
    """LC.blobs() at its own spread: the float64 restatement alone reaches agreement 1.0 on these inputs (checked on the
    CPU when this was written)."""
    X, y = LC.blobs()
    with torch.cuda.device(dev):
        fit, _ = fit_rows(ring_engine(X, dtype, dev), 300, max_iter=500)
    agreement = layout.neighbour_agreement(fit.Y, torch.from_numpy(y).to(dev), k=5)
    print(f"nn blobs {dtype}: KL {fit.kl_init:.4f} -> {fit.kl:.4f} in {fit.iterations} iterations, agreement {agreement}")
    assert fit.iterations == 500 and len(fit.kl_trace) == 10 and tuple(fit.Y.shape) == (300, 2)
    assert fit.kl < fit.kl_init
    assert agreement == 1.0


# ---- 6. past the dense cap ---------------------------------------------------------------------------------------------------------
def test_a_layout_past_the_dense_cap(dev):
    n = 66000
    X = LC.gaussian(n, 8, seed=6)
    g = Graph.from_csr(class_graph(X), torch.from_numpy(X))
    Y, vertices, info = g.layout(method="neighbours", max_points=n, max_iter=10)
    assert tuple(Y.shape) == (n, 2) and bool(torch.isfinite(Y).all()) and torch.equal(vertices, torch.arange(n))
    assert info["n"] == n and info["method"] == "neighbours" and info["neighbours"] == 90 and info["iterations"] == 10
    assert np.isfinite(info["kl"]) and np.isfinite(info["kl_init"]) and n * 90 <= info["nnz"] <= 2 * n * 90
    with pytest.raises(ValueError, match="n = 66000 exceeds 65536 points"):
        g.layout(max_points=n, max_iter=10)


# ---- 7. the surface ------------------------------------------------------------------------------------------------------------------
def test_graph_layout_and_neighbours(dev, k):
    X, y = LC.blobs()
    g = Graph.from_csr(class_graph(X), torch.from_numpy(X))
    eng = g.engine()
    Z0 = eng.get_Z()
    Y, vertices, info = g.layout(method="neighbours", neighbours=60, max_iter=100, labels=[f"c{c}" for c in y])
    assert tuple(Y.shape) == (300, 2) and not Y.is_cuda and torch.equal(vertices, torch.arange(300))
    assert info["method"] == "neighbours" and info["neighbours"] == 60 and 300 * 60 <= info["nnz"] <= 2 * 300 * 60
    assert info["iterations"] == 100 and info["perplexity"] == 30.0 and "neighbour_agreement" in info
    with torch.cuda.device(dev):
        direct, _ = fit_rows(eng, 300, max_iter=100, neighbours=60)
    assert torch.equal(direct.Y.cpu(), Y) and direct.nnz == info["nnz"]
    exact = g.layout(max_iter=50)[2]
    assert not {"method", "neighbours", "nnz"} & set(exact)
    # Graph.neighbours: the order of the search, in vertex numbering
    pool = torch.randperm(300, generator=torch.Generator().manual_seed(2))[:120]
    idx, dist = g.neighbours(7, vertices=pool.tolist())
    tab, rows = layout.TSNE(eng).table_and_rows(pool, "Z")
    D, _ = run_sqdist(k, tab, 16, rows)
    want_ids, want_sq = NC.knn(D.cpu().numpy(), 7)
    assert idx.dtype == torch.int64 and not idx.is_cuda and np.array_equal(idx.numpy(), pool.numpy()[want_ids])
    assert same_bits(dist.numpy(), want_sq)
    idx_all, _ = g.neighbours(3, table="X")
    assert tuple(idx_all.shape) == (300, 3) and bool((y[idx_all.numpy()] == y[:, None]).all())    # blobs: same class
    idx5, dist5 = g.neighbours(6, vertices=[4, 9, 200, 17, 3])
    assert bool((idx5[:, 4:] == -1).all()) and bool(torch.isinf(dist5[:, 4:]).all())
    assert set(idx5[0, :4].tolist()) == {9, 200, 17, 3}
    assert torch.equal(eng.get_Z(), Z0)


def test_cli_writes_the_new_keys_only_when_asked(dev, tmp_path):
    import clane_amd.__main__ as M
    X, y = LC.blobs()
    ids = [f"v{i}" for i in range(300)]
    root = write_data_root(tmp_path / "blobs", ids, ids, [ids[(i + 3) % 300] for i in range(300)], X)

    def run(extra, out):
        cfg = tmp_path / f"{out}.yaml"
        cfg.write_text(CONFIG + extra)
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg), "--gpu"]))
        return tmp_path / out
    out = run("\nlayout:\n  max_iter: 60\n  method: neighbours\n  neighbours: 45\n", "sparse")
    rep = json.loads((out / "layout.json").read_text())
    assert set(rep) == REPORT_KEYS | {"method", "neighbours", "nnz"}
    assert rep["method"] == "neighbours" and rep["neighbours"] == 45 and 300 * 45 <= rep["nnz"] <= 2 * 300 * 45
    assert rep["n"] == 300 and rep["iterations"] == 60 and len((out / "layout.tsv").read_text().splitlines()) == 300

    # without the new keys: the files are, byte for byte, the exact method's report and table as they always were written
    plain = run("\nlayout:\n  max_iter: 60\n", "plain")
    g = Graph.from_csr(class_graph(X), torch.from_numpy(X), vertex_ids=ids)
    g.set_Z(torch.from_numpy(np.load(plain / "Z.npy")))
    Yg, vs, info = g.layout(max_iter=60)
    report = {key: info[key] for key in ("n", "sampled", "perplexity", "iterations", "kl", "kl_init", "grad_norm",
                                         "kl_trace")}
    assert set(report) == REPORT_KEYS
    assert (plain / "layout.json").read_text() == json.dumps(report, indent=1) + "\n"
    assert (plain / "layout.tsv").read_text() == "".join(
        f"{ids[v]}\t{float(Yg[i, 0])!r}\t{float(Yg[i, 1])!r}\n" for i, v in enumerate(vs.tolist()))
    same = run("\nlayout:\n  max_iter: 60\n  method: exact\n", "named")
    assert (same / "layout.json").read_bytes() == (plain / "layout.json").read_bytes()
    assert (same / "layout.tsv").read_bytes() == (plain / "layout.tsv").read_bytes()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_kernel(dev):
    Z = torch.zeros(8, 16, dtype=F32, device=dev)

    def rows(n):
        return torch.zeros(n, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="neighbours = 193 must be above perplexity = 30 and at most 192"):
        layout.NeighbourTSNE(EngineView(dev), neighbours=193)
    with pytest.raises(ValueError, match="neighbours = 30 must be above perplexity = 30"):
        layout.NeighbourTSNE(EngineView(dev), neighbours=30)
    with pytest.raises(ValueError, match="neighbours = 5 must be above perplexity = 8"):
        layout.NeighbourTSNE(EngineView(dev), perplexity=8, neighbours=5)
    with pytest.raises(ValueError, match=r"neighbours = 120 must be above .* at most 99"):
        layout.NeighbourTSNE(EngineView(dev), neighbours=120).fit(Z, rows(100))
    before = torch.cuda.memory_allocated(dev)
    t = layout.NeighbourTSNE(EngineView(dev))
    with pytest.raises(ValueError, match="n = 1048577 exceeds 1048576 points"):
        t.fit(Z, torch.empty((1 << 20) + 1, dtype=torch.int32, device="meta"))
    with pytest.raises(ValueError, match="at least 4 points, got n = 3"):
        layout.NeighbourTSNE(EngineView(dev), perplexity=2).fit(Z, rows(3))
    with pytest.raises(ValueError, match=r"init must be \[300, 2\]"):
        t.fit(Z, rows(300), init=torch.zeros(300, 3))
    with pytest.raises(ValueError, match="k must be an integer in"):
        layout.KNeighbours(EngineView(dev)).search(Z, rows(300), 193)
    with pytest.raises(ValueError, match="n_slabs must be at least 1"):
        layout.KNeighbours(EngineView(dev)).search(Z, rows(300), 7, n_slabs=0)
    assert torch.cuda.memory_allocated(dev) == before

    class Divided(EngineView):
        world, exchange = 2, "halo"
    with pytest.raises(NotImplementedError, match="t-SNE runs on ONE GPU only"):
        layout.NeighbourTSNE(Divided(dev))
    with pytest.raises(NotImplementedError, match="neighbour search runs on ONE GPU only"):
        layout.KNeighbours(Divided(dev))

    X = LC.gaussian(40, 8)
    g = Graph.from_csr(class_graph(X), torch.from_numpy(X))

    class Attached(EngineView):                                   # an engine whose kernels must not be reached
        cosine_mode = "reference"
    g._attach_engine(Attached(dev))
    with pytest.raises(ValueError, match="method must be one of"):
        g.layout(method="tree")
    with pytest.raises(ValueError, match="neighbours = 12 needs method"):
        g.layout(neighbours=12)
    with pytest.raises(ValueError, match="layout: neighbours = 12 needs method: neighbours"):
        layout.check_section({"method": "exact", "neighbours": 12})
    with pytest.raises(ValueError, match="neighbours = 193"):
        g.layout(method="neighbours", neighbours=193)


def test_a_fit_that_cannot_fit_says_how_many_points_would(dev, monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d=None: (1 << 30, 1 << 30))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda d=None: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda d=None: 0)
    t = layout.NeighbourTSNE(EngineView(dev))
    per_point = t.workspace_bytes(500000) // 500000 + 1
    fits = ((1 << 30) - (64 << 20)) // per_point
    with pytest.raises(_hip.ClaneHipError, match=rf"the 90 neighbours .* about {fits} points would fit"):
        t._check_memory(500000, dev)
    t._check_memory(fits, dev)
