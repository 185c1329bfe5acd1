"""The bilinear similarity on the card: the MFMA row projection against a CPU fp64 product, the pair K1 against the
fp64 restatement over every row binning the engine can choose, the reference's own fixture (g13) through Graph.build_P
and Embedder.iterate, and a sampled check at the config-3 shape."""
import numpy as np
import pytest
import torch

from clane_amd import _hip, synth
from clane_amd.embedder import Embedder
from clane_amd.engine import SweepEngine
from clane_amd.graph import Graph
from clane_amd.partition import HostCSR
from clane_amd.similarity import AsymmertricSimilarity
from oracle import clane_oracle as O

from .conftest import load_golden, write_data_root
from .test_bilinear_host import GOLD, _sim, bilinear_P

pytestmark = pytest.mark.gpu

EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


# ---- project_rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_project_rows_against_fp64(dev, k, dtype):
    """|Y - Z W^T| <= 2 d eps_acc (|Z| |W|^T) elementwise (a k-ordered fma chain of d terms in the accumulate type; bf16
    tables are exact in f32), with padded leading dimensions; a second call gives the same bits."""
    acc = _hip.acc_dtype(dtype)
    gen = torch.Generator().manual_seed(5)
    for d in (1, 2, 5, 16, 64, 128, 130, 256, 512):
        W = (torch.randn(2 * d, d, generator=gen, dtype=torch.float64) / d ** 0.5).to(acc)
        for rows in (1, 17, 1000, 100_003):
            if rows == 100_003 and d > 256 and dtype != torch.float32:
                continue                                   # the big-row case once per width class is enough
            Zc = torch.randn(rows, d, generator=gen, dtype=torch.float64).to(dtype)
            ldz, ldy = d + 3, 2 * d + 5                    # neither a multiple of a pack: the general case
            Zbuf = torch.zeros(rows, ldz, dtype=dtype, device=dev)
            Zbuf[:, :d] = Zc.to(dev)
            Ybuf = torch.full((rows, ldy), float("nan"), dtype=acc, device=dev)
            Wd = W.to(dev).contiguous()
            k.project_rows(Zbuf, d, Wd, Ybuf)
            Y1 = Ybuf.clone()
            k.project_rows(Zbuf, d, Wd, Ybuf)
            assert torch.equal(Y1[:, :2 * d], Ybuf[:, :2 * d]), (dtype, d, rows)    # bit-reproducible
            assert torch.isnan(Ybuf[:, 2 * d:]).all(), (dtype, d, rows)             # nothing beyond 2d is written
            sel = torch.arange(rows) if rows <= 1000 else torch.cat(
                [torch.randint(0, rows, (2000,), generator=gen), torch.arange(rows - 130, rows)])
            Z64, W64 = Zc[sel].double(), W.double()
            want = Z64 @ W64.T
            bound = 2 * d * EPS[acc] * (Z64.abs() @ W64.abs().T) + 1e-300
            got = Y1[sel.to(dev), :2 * d].cpu().double()
            assert bool(((got - want).abs() <= bound).all()), (dtype, d, rows, float(((got - want).abs() / bound).max()))


# ---- pair K1 over every binning ----------------------------------------------------------------------------
def _hub_csr(V, hubs, seed, max_deg=6):
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, max_deg + 1, size=V)
    deg[rng.choice(V, size=len(hubs), replace=False)] = hubs
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    cols = np.concatenate([np.sort(rng.choice(V, size=int(g), replace=False)) for g in deg] + [np.empty(0, int)])
    return HostCSR(V, rowptr, cols.astype(np.int32))


def _golden_csr(name):
    g = load_golden(name)
    idx = g["A_indices"]
    V = g["X"].shape[0]
    rowptr, colidx = O.build_csr(V, idx[0], idx[1])
    return HostCSR(V, rowptr, colidx.astype(np.int32)), torch.from_numpy(g["X"])


CASES = {
    # name: (csr + X maker, engine keyword arguments, what the case must exercise)
    "g11_hubs": (lambda: _golden_csr("g11_hubs320_d8_g0.9.npz"), {}, "class"),
    "g12_hubs": (lambda: _golden_csr("g12_hubs150_d256_g0.76.npz"), {}, "class"),
    "long_rows_d8": (lambda: (_hub_csr(3000, [300, 900, 2500], 3), None), {"class_threshold": 0, "long_threshold": 64},
                     "long"),
    "long_rows_d256": (lambda: (_hub_csr(3000, [300, 900, 2500], 4), None), {"class_threshold": 0, "long_threshold": 64},
                       "long"),
    "class_rows_d40": (lambda: (_hub_csr(5000, [100, 400, 1500, 4000], 5), None),
                       {"class_threshold": 32, "class_chunk": 64}, "class"),
}
WIDTH = {"long_rows_d8": 8, "long_rows_d256": 256, "class_rows_d40": 40}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", sorted(CASES))
def test_pair_k1_every_binning(dev, dtype, case):
    make, kw, must = CASES[case]
    csr, X = make()
    if X is None:
        X = torch.from_numpy(np.random.default_rng(7).standard_normal((csr.num_vertices, WIDTH[case])))
    X = X.to(dtype)
    d = X.shape[1]
    gen = torch.Generator().manual_seed(len(case))
    W = (torch.randn(2 * d, d, generator=gen, dtype=torch.float64) / d ** 0.75).to(dtype)     # scores O(1)
    with torch.cuda.device(dev):
        eng = SweepEngine(csr, X, dev, **kw)
        if must == "long":
            assert any(lr is not None and lr.numel() > 0 for lr in eng.k1_long_rows), case
        else:
            assert eng.class_k1 and any(c is not None for c in eng.class_rows), case
        eng.build_P_bilinear(W)
        P1 = eng.P_global()
        eng.build_P_bilinear(W)
        assert torch.equal(P1, eng.P_global()), case                       # repeat runs: same bits
    want = bilinear_P(csr.rowptr, csr.colidx, X, W[:d], W[d:])
    rtol = 1e-5 if dtype == torch.float32 else 1e-12
    np.testing.assert_allclose(P1.double().numpy(), want.numpy(), rtol=rtol, atol=rtol * 1e-2, err_msg=case)
    cs = np.concatenate([[0.0], np.cumsum(P1.double().numpy())])
    deg = np.diff(csr.rowptr)
    sums = cs[csr.rowptr[1:]] - cs[csr.rowptr[:-1]]
    assert np.abs(sums[deg > 0] - 1).max() < 1e-4                          # every row scored and soft-maxed once


# ---- the reference's fixture on the card -------------------------------------------------------------------------
def _gpu_graph(tmp_path, gold, dtype):
    k = load_golden("g2_karate_csr.npz")
    root = write_data_root(tmp_path / "karate_asym", k["vertex_ids"], k["edge_src"], k["edge_dst"], gold["X"])
    return Graph(root, embedding_dim=int(gold["X"].shape[1]), dtype=dtype)


def test_golden_build_P_and_iterate_f32(dev, tmp_path):
    gold = load_golden(GOLD)
    g = _gpu_graph(tmp_path, gold, "float32")
    sim = _sim(gold)
    P = g.build_P(sim)
    np.testing.assert_array_equal(P.indices().numpy(), gold["A_indices"])
    assert np.abs(P.values().numpy() - gold["P_values"]).max() < 1e-5
    emb = Embedder(g, sim, torch.device("cuda"), gamma=float(gold["gamma"]), tolerence=int(gold["tolerence"]),
                   verbose=False)
    emb.iterate()
    assert O.rel_l2(g.Z, torch.from_numpy(gold["Z_final"])) < 1e-5
    assert abs(emb.sweep_counts[0] - int(gold["sweep_counts"][0])) <= 3


def test_golden_build_P_f64(dev, tmp_path):
    """fp64 tables and weights: P within 1e-12 of the fp64 restatement, and within the fp32 reference's own rounding of
    the reference's values."""
    gold = load_golden(GOLD)
    g = _gpu_graph(tmp_path, gold, "float64")
    sim = _sim(gold, torch.float64)
    P = g.build_P(sim).values().numpy()
    idx = gold["A_indices"]
    rowptr, colidx = O.build_csr(34, idx[0], idx[1])
    want = bilinear_P(rowptr, colidx, gold["X"], gold["Phi_src"], gold["Phi_dst"]).numpy()
    assert np.abs(P - want).max() < 1e-12
    assert np.abs(P - gold["P_values"]).max() < 1e-5


# ---- config-3 shape ---------------------------------------------------------------------------------------------------
def test_config3_shape_sampled_rows(dev):
    """R-MAT 2M / 40M / d = 256 fp32: build_P_bilinear against the fp64 restatement on 10 000 sampled rows (the heaviest
    hubs among them), then one sweep from that P checked on the same rows."""
    V, E, d = 2_000_000, 40_000_000, 256
    csr = synth.rmat_csr(V, E, seed=3, device=str(dev))
    X = synth.gaussian_X(V, d, seed=4)
    torch.manual_seed(0)
    sim = AsymmertricSimilarity(d)
    with torch.cuda.device(dev):
        eng = SweepEngine(csr, X, dev)
        eng.build_P_bilinear(sim.stacked_weight(torch.float32, dev))
        P = eng.P_global().numpy()
        delta = eng.sweep(0.76)
        Z1 = eng.get_Z()
    deg = np.diff(csr.rowptr)
    rng = np.random.default_rng(1)
    rows = np.unique(np.concatenate([rng.choice(V, size=9990, replace=False), np.argsort(deg)[-10:]]))
    Xd = X.to(dev, torch.float64)
    Ws = sim.Phi_src.weight.detach().to(dev, torch.float64)
    Wd = sim.Phi_dst.weight.detach().to(dev, torch.float64)
    P64 = torch.from_numpy(P).double()
    checked = 0
    for r in rows:
        a, b = int(csr.rowptr[r]), int(csr.rowptr[r + 1])
        if b == a:
            assert torch.equal(Z1[r], X[r])
            continue
        cols = torch.from_numpy(csr.colidx[a:b].astype(np.int64)).to(dev)
        s = (Xd[cols] @ Wd.T) @ (Ws @ Xd[int(r)])
        want = torch.softmax(s, 0).cpu()
        got = P64[a:b]
        # scores of d = 256 gaussian rows through xavier weights are O(16): an fp32 dot's rounding moves P by ~1e-4
        assert float((got - want).norm()) <= 2e-3 * float(want.norm()), (r, b - a)
        z1 = X[r].double() + 0.76 * (got.to(dev) @ Xd[cols]).cpu()
        assert float((Z1[r].double() - z1).norm()) <= 1e-5 * float(z1.norm()), r
        checked += 1
    assert checked > 5000 and np.isfinite(delta) and delta > 0
