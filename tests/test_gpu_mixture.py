"""Soft clusters on the card: the two kernels of csrc/mixture.h against float64 with a-priori bounds and bit for bit on
integer data, the fitted mixtures against the float64 reference EM of tests/mixture_cases.py, and the public surface
(Graph.soft_cluster, MixtureModel, the CLI section)."""
import json
import math

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.engine import SweepEngine
from clane_amd.graph import Graph
from clane_amd.mixture import GaussianMixture, MixtureModel
from clane_amd.partition import HostCSR

from . import mixture_cases as mc

pytestmark = pytest.mark.gpu

EPS = mc.EPS
DTYPES = [torch.float32, torch.bfloat16, torch.float64]
# (n, d, K, R): R * Kp = 152 crosses the 128-column tile; depth 2 d = 260 and 512; K = 1; K = 64 fills the wave
ESTEP_SHAPES = [(1, 1, 1, 1), (127, 5, 3, 3), (129, 16, 7, 19), (5000, 130, 17, 3), (5000, 256, 64, 3), (127, 130, 2, 19),
                (129, 3, 1, 2)]
TIE_SHAPES = [(129, 5, 3, 19), (127, 16, 17, 3), (200, 4, 64, 2)]
# (n, R * Kp, d)
MSTEP_SHAPES = [(1, 8, 1), (2047, 152, 5), (2049, 8, 16), (10000, 152, 130), (2049, 152, 256)]
# The planted seed per shape for the float32 / bfloat16 fits: chosen on the CPU so that at most 1 % of the rows have a
# REFERENCE top-two responsibility margin below 1e-2 on the dtype-rounded data (float32 / bfloat16 counts per shape:
# 0 / 0 of 600, 0 / 0 of 1000, 0 / 0 of 300 at the seeds of mixture_cases.SHAPES, which are kept).
FIT_SEEDS = {s: s[4] for s in mc.SHAPES}


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


def _padded(values, dtype, dev, pad=3):
    buf = torch.zeros(values.shape[0], values.shape[1] + pad, dtype=dtype, device=dev)
    buf[:, :values.shape[1]] = values.to(dtype).to(dev)
    return buf[:, :values.shape[1]]                     # leading dimension d + pad


# ---- E-step -----------------------------------------------------------------------------------------------------
def _estep_case(n, d, K, R, dtype, dev, integers=False):
    gen = torch.Generator().manual_seed(1000 * n + 10 * d + K + R)
    acc = _hip.acc_dtype(dtype)
    Kp = _hip.mixture_padded_components(K)
    table_rows = max(3, n // 2)                         # rows repeat
    Wm = torch.full((R, Kp, 2 * d), 7.0, dtype=torch.float64)          # pad components: rows that would win if read
    cst = torch.full((R, Kp), 1e30, dtype=torch.float64)
    if integers:
        # x in -2..2 with three entries in four zero, and one integer const per restart: a logit is a sum of few small
        # terms, so in EVERY restart more than n / 4 rows hold a tie of the maximum (counted on the CPU, per restart:
        # at least 54 of 129, 41 of 127 and 186 of 200 rows at the three shapes)
        Zv = torch.randint(-2, 3, (table_rows, d), generator=gen).double()
        Zv = Zv * (torch.rand(table_rows, d, generator=gen) < 0.25)
        mean = torch.zeros(d, dtype=torch.float64)
        Wm[:, :K, :d] = -0.5 * torch.randint(1, 3, (R, K, d), generator=gen).double()      # -a/2 in {-1/2, -1}
        Wm[:, :K, d:] = torch.randint(-1, 2, (R, K, d), generator=gen).double()
        cst[:, :K] = torch.randint(-1, 2, (R, 1), generator=gen).double()
    else:
        Zv = torch.randn(table_rows, d, generator=gen, dtype=torch.float64)
        mean = 0.25 * torch.randn(d, generator=gen, dtype=torch.float64)
        var = 0.5 + torch.rand(R, K, d, generator=gen, dtype=torch.float64)
        mu = torch.randn(R, K, d, generator=gen, dtype=torch.float64)
        w = torch.rand(R, K, generator=gen, dtype=torch.float64) + 0.1
        w = w / w.sum(1, keepdim=True)
        a = 1.0 / var
        Wm[:, :K, :d], Wm[:, :K, d:] = -0.5 * a, mu * a
        cst[:, :K] = torch.log(w) - 0.5 * (d * math.log(2 * math.pi) + (torch.log(var) + mu * mu * a).sum(2))
    Z = _padded(Zv, dtype, dev)
    rows = torch.randint(0, table_rows, (n,), generator=gen).to(torch.int32)
    rows[n // 2] = table_rows                           # one index past the table: a zero row, centred like any row
    return dict(Z=Z, rows=rows.to(dev), mean=mean.to(acc).to(dev), Wm=Wm.view(R * Kp, 2 * d).to(acc).to(dev).contiguous(),
                cst=cst.view(R * Kp).to(acc).to(dev).contiguous(), n=n, d=d, K=K, Kp=Kp, R=R, acc=acc,
                table_rows=table_rows)


def _run_estep(k, c, dev, restart=None):
    n, R, Kp, d = c["n"], c["R"], c["Kp"], c["d"]
    Wm, cst = c["Wm"], c["cst"]
    if restart is not None:                             # restart r alone
        Wm, cst, R = Wm[restart * Kp:(restart + 1) * Kp], cst[restart * Kp:(restart + 1) * Kp], 1
    resp = torch.full((n * R * Kp,), float("nan"), dtype=c["acc"], device=dev)
    ll = torch.full((R,), float("nan"), dtype=torch.float64, device=dev)
    ws = torch.zeros(k.mixture_ll_ws_len(n, R), dtype=torch.float64, device=dev)
    assign = torch.full((n, R + 1), -7, dtype=torch.int32, device=dev)
    k.mixture_estep(c["Z"], d, c["rows"], c["mean"], Wm, cst, R, c["K"], ws, ll, resp=resp, assign=assign[:, :R])
    torch.cuda.synchronize()
    return resp.view(n, R, Kp), ll, assign


def _estep64(c):
    """float64 logits [n, R, K] of the values the kernel reads, and the bound b per logit: 2 (2 d) eps (sum |xc^2| |a/2|
    + sum |xc| |b| + |const|) plus the single rounding of xc carried through (eps on xc, 2 eps on xc^2)."""
    n, R, Kp, K, d = c["n"], c["R"], c["Kp"], c["K"], c["d"]
    r = c["rows"].long()
    inside = (r >= 0) & (r < c["table_rows"])
    xc = c["Z"].double()[r.clamp(0, c["table_rows"] - 1)] * inside[:, None] - c["mean"].double()
    Wm, cst = c["Wm"].double(), c["cst"].double()
    sq, lin = (xc * xc) @ Wm[:, :d].T, xc @ Wm[:, d:].T
    asq, alin = (xc * xc) @ Wm[:, :d].abs().T, xc.abs() @ Wm[:, d:].abs().T
    eps = EPS[c["acc"]]
    logits = (sq + lin + cst).view(n, R, Kp)[:, :, :K]
    b = (2 * (2 * d) * eps * (asq + alin + cst.abs()) + eps * alin + 2 * eps * asq).view(n, R, Kp)[:, :, :K]
    return logits, b, eps


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", ESTEP_SHAPES, ids=str)
def test_estep_against_float64(k, dev, dtype, shape):
    n, d, K, R = shape
    c = _estep_case(n, d, K, R, dtype, dev)
    resp, ll, assign = _run_estep(k, c, dev)
    logits, b, eps = _estep64(c)
    bmax = b.amax(2)                                                    # [n, R]
    lse = torch.logsumexp(logits, 2)
    err = (resp[:, :, :K].double() - torch.exp(logits - lse[:, :, None])).abs()
    tol = 2 * bmax[:, :, None] + 8 * eps
    print(f"estep {shape} {dtype}: max |r - r64| / bound = {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())
    assert bool((resp[:, :, K:] == 0).all())                            # pad columns
    ll_tol = (2 * bmax).sum(0) + n * eps * lse.abs().sum(0)
    ll_err = (ll - lse.sum(0)).abs()
    print(f"estep {shape} {dtype}: max ll error / bound = {float((ll_err / ll_tol).max()):.3f}")
    assert bool((ll_err <= ll_tol).all())
    if K > 1:
        top2 = logits.topk(2, 2).values
        clear = (top2[:, :, 0] - top2[:, :, 1]) > 2 * bmax
    else:
        clear = torch.ones(n, R, dtype=torch.bool, device=dev)
    assert bool(clear.any())
    assert torch.equal(assign[:, :R][clear].long(), logits.argmax(2)[clear])
    assert bool((assign[:, R] == -7).all())                             # nothing written past the R columns
    assert bool(((assign[:, :R] >= 0) & (assign[:, :R] < K)).all())
    resp2, ll2, assign2 = _run_estep(k, c, dev)                         # a second call: equal bits
    assert torch.equal(resp, resp2) and torch.equal(ll, ll2) and torch.equal(assign, assign2)
    for r in sorted({0, R - 1}):                                        # restart r alone: equal bits
        resp1, ll1, assign1 = _run_estep(k, c, dev, restart=r)
        assert torch.equal(resp1[:, 0], resp[:, r]) and torch.equal(ll1[0], ll[r])
        assert torch.equal(assign1[:, 0], assign[:, r])


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", TIE_SHAPES, ids=str)
def test_estep_ties_go_to_the_lowest_component(k, dev, dtype, shape):
    n, d, K, R = shape
    c = _estep_case(n, d, K, R, dtype, dev, integers=True)              # logits exact in every dtype, many ties
    _, _, assign = _run_estep(k, c, dev)
    logits, _, _ = _estep64(c)
    top = logits.amax(2, keepdim=True)
    idx = torch.arange(K, device=dev).expand_as(logits)
    lowest = torch.where(logits == top, idx, torch.full_like(idx, K)).amin(2)
    tied = (logits == top).sum(2) > 1                                   # [n, R]
    per_restart = tied.sum(0)
    inside = c["rows"].long() < c["table_rows"]
    busy = (c["Z"].double()[c["rows"].long().clamp(max=c["table_rows"] - 1)] != 0).any(1) & inside   # rows not all zero
    wrong = int((assign[:, :R].long() != lowest).sum())
    print(f"ties {shape} {dtype}: rows holding a tie per restart min {int(per_restart.min())} max {int(per_restart.max())} "
          f"(n / 4 = {n / 4}), {int((tied & busy[:, None]).sum())} of the pairs in rows with a non-zero entry; "
          f"{wrong} assignments differ from the lowest maximal component")
    assert int(per_restart.min()) > n / 4                               # in every restart more than n / 4 ROWS hold a tie
    assert int((tied & busy[:, None]).any(1).sum()) > 0
    assert wrong == 0 and torch.equal(assign[:, :R].long(), lowest)


# ---- M-step -----------------------------------------------------------------------------------------------------
def _run_mstep(k, Z, d, rows, mean, resp, dev):
    acc, n, K = resp.dtype, rows.numel(), resp.shape[1]
    ws = torch.full((k.mixture_mstep_ws_len(n, K, d),), float("nan"), dtype=acc, device=dev)
    S = torch.full((K, 2 * d), float("nan"), dtype=acc, device=dev)
    nk = torch.full((K,), float("nan"), dtype=acc, device=dev)
    k.mixture_mstep(Z, d, rows, mean, resp.view(-1), ws, S, nk)
    torch.cuda.synchronize()
    return S, nk


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", MSTEP_SHAPES, ids=str)
def test_mstep_against_float64(k, dev, dtype, shape):
    n, K, d = shape
    gen = torch.Generator().manual_seed(n + K + d)
    acc = _hip.acc_dtype(dtype)
    table_rows = max(3, n // 2)
    Z = _padded(torch.randn(table_rows, d, generator=gen, dtype=torch.float64), dtype, dev)
    rows = torch.randint(0, table_rows, (n,), generator=gen).to(torch.int32)
    rows[n // 2] = table_rows
    rows = rows.to(dev)
    mean = (0.25 * torch.randn(d, generator=gen, dtype=torch.float64)).to(acc).to(dev)
    resp = torch.rand(n, K, generator=gen, dtype=torch.float64).to(acc).to(dev)
    S, nk = _run_mstep(k, Z, d, rows, mean, resp, dev)
    xc = Z.double()[rows.long().clamp(max=table_rows - 1)] * (rows.long() < table_rows)[:, None] - mean.double()
    phi = torch.cat([xc * xc, xc], 1)
    r64 = resp.double()
    eps = EPS[acc]
    tol_S = 2 * n * eps * (r64.abs().T @ phi.abs())
    tol_nk = 2 * n * eps * r64.abs().sum(0)
    err_S, err_nk = (S.double() - r64.T @ phi).abs(), (nk.double() - r64.sum(0)).abs()
    print(f"mstep {shape} {dtype}: max error / bound S {float((err_S / tol_S.clamp(min=1e-300)).max()):.3f} "
          f"nk {float((err_nk / tol_nk.clamp(min=1e-300)).max()):.3f}")
    assert bool((err_S <= tol_S).all()) and bool((err_nk <= tol_nk).all())
    S2, nk2 = _run_mstep(k, Z, d, rows, mean, resp, dev)
    assert torch.equal(S, S2) and torch.equal(nk, nk2)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(10000, 152, 130), (2049, 8, 5)], ids=str)
def test_mstep_is_exact_on_integer_data(k, dev, dtype, shape):
    n, K, d = shape                                     # r <= 2, |xc| <= 3: every sum below 18 n < 2^24
    gen = torch.Generator().manual_seed(7)
    acc = _hip.acc_dtype(dtype)
    table_rows = n // 3
    Zi = torch.randint(-2, 3, (table_rows, d), generator=gen)
    ri = torch.randint(0, 3, (n, K), generator=gen)
    mi = torch.randint(-1, 2, (d,), generator=gen)
    rows = torch.randint(0, table_rows, (n,), generator=gen)
    S, nk = _run_mstep(k, _padded(Zi.double(), dtype, dev), d, rows.to(torch.int32).to(dev), mi.to(acc).to(dev),
                       ri.to(acc).to(dev), dev)
    xc = Zi[rows] - mi
    want = ri.T @ torch.cat([xc * xc, xc], 1)
    print(f"mstep integers {shape} {dtype}: {int((S.cpu().double() != want.double()).sum())} of {want.numel()} entries of S "
          f"and {int((nk.cpu().double() != ri.sum(0).double()).sum())} of {K} of nk differ from the integer reference "
          f"(largest |S| {int(want.abs().max())} < 2^24)")
    assert torch.equal(S.cpu().long(), want) and torch.equal(nk.cpu().long(), ri.sum(0))
    assert torch.equal(S.cpu().double(), want.double())                 # integers, not values near them


# ---- the fit ----------------------------------------------------------------------------------------------------
def _ring_engine(X, dtype, dev):
    V = X.shape[0]
    csr = HostCSR(V, np.arange(V + 1, dtype=np.int64), ((np.arange(V) + 1) % V).astype(np.int32))
    return SweepEngine(csr, X.to(dtype), dev)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _spread(X, resp0, iterations=8):
    """The reference's own relative spread between summing the rows forwards and backwards over the iterations."""
    fwd = mc.reference_em(X, resp0=resp0, tol=0.0, max_iter=iterations)
    bwd = mc.reference_em(X, resp0=resp0, tol=0.0, max_iter=iterations, reverse=True)
    return fwd, max(_rel(bwd[f], fwd[f]) for f in ("weights", "centred_means", "variances", "lower_bounds"))


@pytest.mark.parametrize("shape", mc.SHAPES, ids=str)
def test_fit_float64_follows_the_reference(dev, shape):
    """Eight iterations in float64 from the reference's initial responsibilities.  The margin is not fixed in advance:
    1000 x the reference's own forwards / backwards row-order spread -- both are rounding differences carried through the
    same EM map, and the card's order differs more than a reversal.

    Recorded on an MI355X, relative, worst of weights, centred means, variances and the eight lower bounds -- the
    reference's spread / the card's error: (600, 5, 4) 6.3e-14 / 1.8e-14; (1000, 16, 7) 7.0e-14 / 1.6e-14; (300, 3, 2)
    1.6e-14 / 3.2e-15 (the variances are the worst quantity every time)."""
    n, d, K, sep, seed = shape
    X, y, _, _ = mc.planted(n, d, K, sep, seed)
    resp0 = mc.noisy_start(y, K, seed)
    ref, spread = _spread(X, resp0)
    with torch.cuda.device(dev):
        eng = _ring_engine(torch.from_numpy(X), torch.float64, dev)
        gm = GaussianMixture(eng, tol=0.0, max_iter=8)
        rows = eng.pos[torch.arange(n, device=dev)].to(torch.int32)
        fit = gm.fit(eng.Zcur, rows, K, init=torch.from_numpy(resp0)[None])
    lbs = torch.stack(gm.history)[:, 0].cpu().numpy()
    errs = {"weights": _rel(fit.weights[0].cpu(), ref["weights"]),
            "centred_means": _rel(fit.centred_means[0].cpu(), ref["centred_means"]),
            "variances": _rel(fit.variances[0].cpu(), ref["variances"]), "lower_bounds": _rel(lbs, ref["lower_bounds"])}
    print(f"fit64 {shape}: reference spread {spread:.2e}, allowed {1000 * spread:.2e}, observed {errs}")
    assert spread > 0 and fit.iterations.tolist() == [8] and len(lbs) == 8
    assert max(errs.values()) <= 1000 * spread
    drop = lbs[:-1] - lbs[1:]
    assert bool((drop <= n * EPS[torch.float64] * np.abs(lbs[1:])).all())       # the bound never falls by more


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("shape", mc.SHAPES, ids=str)
def test_fit_float32_and_bfloat16_reach_the_reference(dev, dtype, shape):
    """tol = 1e-6, max_iter = 500 from the reference's start.  The card's final parameters are scored in float64 on the
    CPU on the dtype-rounded data and compared with the reference converged from the same start.  The allowed gap in the
    mean log-likelihood is not fixed in advance: 10 x what the reference's own bound still gains between stopping at tol
    and at tol / 10, plus the E-step's a-priori bound per row (the mean over the rows of 2 max_k b + eps |lse|).

    Recorded on an MI355X -- the reference's gain / the a-priori bound / the observed gap, float32 then bfloat16:
    (600, 5, 4) 4.4e-07 / 2.1e-04 / 4.0e-07 and 4.5e-07 / 2.1e-04 / 2.2e-07; (1000, 16, 7) 0 / 4.1e-03 / 2.1e-10 and
    0 / 4.1e-03 / 9.0e-09; (300, 3, 2) 0 / 1.8e-04 / 5.5e-12 and 0 / 1.8e-04 / 2.8e-10.  The card stops within one
    iteration of the reference (14, 16 / 15; 4, 3 / 3; 4, 4 / 4), and no row has a reference margin below 1e-2."""
    n, d, K, sep, _ = shape
    X, y, _, _ = mc.planted(n, d, K, sep, FIT_SEEDS[shape])
    Xr = torch.from_numpy(X).to(dtype).double().numpy()                 # the data both sides see
    resp0 = mc.noisy_start(y, K, FIT_SEEDS[shape])
    ref = mc.reference_em(Xr, resp0=resp0, tol=1e-6, max_iter=500)
    finer = mc.reference_em(Xr, resp0=resp0, tol=1e-7, max_iter=500)
    gain = abs(finer["log_likelihood"] - ref["log_likelihood"])
    with torch.cuda.device(dev):
        eng = _ring_engine(torch.from_numpy(X), dtype, dev)
        gm = GaussianMixture(eng, tol=1e-6, max_iter=500)
        rows = eng.pos[torch.arange(n, device=dev)].to(torch.int32)
        fit = gm.fit(eng.Zcur, rows, K, init=torch.from_numpy(resp0)[None])
    w, mu, var = fit.weights[0].cpu().numpy(), fit.means[0].cpu().numpy(), fit.variances[0].cpu().numpy()
    got = mc.score(Xr, w, mu, var)
    # the E-step's a-priori bound at the card's parameters, per row
    eps = EPS[dtype]
    xc = Xr - fit.mean.cpu().numpy()
    a, muc = 1.0 / var, fit.centred_means[0].cpu().numpy()
    const = np.log(w) - 0.5 * (d * math.log(2 * math.pi) + (np.log(var) + muc * muc * a).sum(1))
    asq, alin = (xc * xc) @ (0.5 * a).T, np.abs(xc) @ np.abs(muc * a).T
    b = 2 * (2 * d) * eps * (asq + alin + np.abs(const)) + eps * alin + 2 * eps * asq
    lse = mc.e_step(xc, w, muc, var)[0]
    apriori = float((2 * b.max(1) + eps * np.abs(lse)).mean())
    gap = abs(got - ref["log_likelihood"])
    print(f"fit {shape} {dtype}: iterations {fit.iterations.tolist()} (reference {ref['n_iter']}), gap {gap:.3e}, "
          f"allowed 10 x {gain:.3e} + {apriori:.3e}")
    assert ref["converged"] and gap <= 10 * gain + apriori
    assert abs(float(fit.log_likelihood[0]) - got) <= apriori           # what the card reports is what its parameters score
    top2 = np.sort(ref["resp"], 1)[:, ::-1][:, :2] if K > 1 else np.stack([np.ones(n), np.zeros(n)], 1)
    unclear = (top2[:, 0] - top2[:, 1]) < 1e-2
    print(f"fit {shape} {dtype}: {int(unclear.sum())} of {n} rows have a reference margin below 1e-2")
    assert int(unclear.sum()) <= 0.01 * n                               # a condition on the data and the reference alone
    assert np.array_equal(fit.assign.cpu().numpy()[~unclear], ref["assign"][~unclear])


# ---- the surface ------------------------------------------------------------------------------------------------
def _fresh(n, d, K, sep, seed, m, fresh_seed):
    """m fresh rows of the planted mixture of ``seed``: the same means and sigmas, new classes and noise."""
    _, _, means, sigma = mc.planted(n, d, K, sep, seed)
    rng = np.random.default_rng(fresh_seed)
    y = rng.integers(0, K, m)
    return means[y] + sigma[y] * rng.standard_normal((m, d)), y


def test_soft_cluster_picks_the_planted_count_and_the_model_assigns_fresh_rows(dev):
    """Graph.soft_cluster on planted content (table "X") over K - 2 .. K + 2 and MixtureModel.predict_rows on 500 fresh
    rows of the same mixture: on the CPU the float64 reference (converged from the planted partition on the
    float32-rounded data) assigns 97.4 % of them (487) to their component at this shape (sep = 3)."""
    n, d, K, sep, seed = mc.SHAPES[0]
    X, y, _, _ = mc.planted(n, d, K, sep, seed)
    csr = HostCSR(n, np.arange(n + 1, dtype=np.int64), ((np.arange(n) + 1) % n).astype(np.int32))
    g = Graph.from_csr(csr, torch.from_numpy(X.astype(np.float32)))
    g.engine(dev)
    kw = dict(k=list(range(K - 2, K + 3)), labels=y.tolist(), restarts=3, seed=0, table="X", return_memberships=True)
    out = g.soft_cluster(**kw)
    cands = out["selection"]["candidates"]
    print("soft_cluster: bic", [(c["clusters"], round(c["bic"], 1)) for c in cands], "nmi", out["nmi"])
    assert out["selection"]["chosen"] == K == out["clusters"] and out["selection"]["criterion"] == "bic"
    assert [c["clusters"] for c in cands] == list(range(K - 2, K + 3))
    assert out["nmi"] > 0.9 and out["converged"] and out["empty"] == 0 and sum(out["sizes"]) == n
    member = out["memberships"]
    assert member.shape == (n, K) and float(np.abs(member.sum(1) - 1.0).max()) <= 64 * EPS[torch.float32]
    assert np.array_equal(member.argmax(1), np.asarray(out["assignments"]))
    assert out["bic"] == min(c["bic"] for c in cands) and 0.0 <= out["mean_entropy"] <= 0.2 and out["confident"] > 0.9
    again = g.soft_cluster(**kw)                                        # the same dict on a second run
    plain = lambda r: {key: v for key, v in r.items() if key not in ("memberships", "model")}    # noqa: E731
    assert plain(again) == plain(out) and np.array_equal(again["memberships"], member)
    model = out["model"]
    assert isinstance(model, MixtureModel) and model.table == "X" and model.K == K and model.n_train == n
    # fresh rows of the same mixture go to the component that holds their class
    owner = np.array([np.bincount(np.asarray(out["assignments"])[y == c], minlength=K).argmax() for c in range(K)])
    Xf, yf = _fresh(n, d, K, sep, seed, 500, 77)
    comp, prob = model.predict_rows(g.engine(), torch.from_numpy(Xf.astype(np.float32)).to(dev), top=3)
    share = float((comp[:, 0] == owner[yf]).mean())
    print(f"predict_rows: {share:.3f} of 500 fresh rows go to their component")
    assert share >= 0.95 and comp.shape == (500, 3) and bool((prob[:, :-1] >= prob[:, 1:]).all())
    assert bool(((prob[:, 0] > 0) & (prob.sum(1) <= 1.0 + 64 * EPS[torch.float32])).all())


def test_cli_section_writes_its_files_and_assigns_the_arrivals(dev, tmp_path):
    import clane_amd.__main__ as M
    from .conftest import GOLDEN, load_golden, write_data_root
    from .new_vertex_cases import CONFIG, write_arrivals
    kar = load_golden("g2_karate_csr.npz")
    rng = np.random.default_rng(0)
    root = write_data_root(tmp_path / "karate", kar["vertex_ids"], kar["edge_src"], kar["edge_dst"],
                           rng.standard_normal((34, 4)).astype(np.float32))
    labelled = (GOLDEN / "g2_karate_Y.tsv").read_text().splitlines()[::2][::-1]      # half the vertices, not in vertex order
    (root / "Y").write_text("\n".join(labelled) + "\n")
    ids = [str(v) for v in kar["vertex_ids"]]
    new_ids = ["new-b", "new-a", "new-c"]
    write_arrivals(root / "arrivals", V="\n".join(new_ids) + "\n",
                   E=f"new-b\t{ids[3]}\nnew-b\t{ids[9]}\nnew-a\t{ids[0]}\n", C_=rng.standard_normal((3, 4)).astype(np.float32))

    def run(cfg_text, out):
        cfg = tmp_path / f"{out}.yaml"
        cfg.write_text(cfg_text)
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg), "--gpu"]))
        return tmp_path / out
    section = ("\nsoft_clustering:\n  clusters: [1, 2, 3]\n  labels: Y\n  restarts: 3\n  criterion: aic\n  baseline: true\n"
               "  memberships: true\n  top: 2\n")
    out = run(CONFIG + section, "mix")
    assert sorted(p.name for p in out.iterdir()) == ["Z.npy", "memberships.tsv", "mixture_metrics.json", "mixture_model.npz"]
    got = json.loads((out / "mixture_metrics.json").read_text())
    assert got["clustered"] == len(labelled) == 17 and got["criterion"] == "aic" and set(got["tables"]) == {"Z", "X"}
    assert "assigned_new" not in got and got["tables"]["Z"]["selection"]["criterion"] == "aic"
    model = MixtureModel.load(out / "mixture_model.npz", d=4)
    assert model.K == got["clusters"] == got["tables"]["Z"]["selection"]["chosen"]
    rows = [r.split("\t") for r in (out / "memberships.tsv").read_text().splitlines()]
    assert [r[0] for r in rows] == ids                                  # every vertex, in vertex order
    assert all(len(r) == 1 + 2 * min(2, model.K) and repr(float(r[2])) == r[2] for r in rows)
    new = run(CONFIG + section + "\nnew_vertices:\n  root: arrivals\n", "new")
    assert (new / "Z.npy").read_bytes() == (out / "Z.npy").read_bytes()
    assert (new / "memberships.tsv").read_bytes() == (out / "memberships.tsv").read_bytes()
    got_new = json.loads((new / "mixture_metrics.json").read_text())
    assert got_new["assigned_new"] == 3 and {k_: v for k_, v in got_new.items() if k_ != "assigned_new"} == got
    lines = [r.split("\t") for r in (new / "memberships_new.tsv").read_text().splitlines()]
    assert [r[0] for r in lines] == new_ids and all(0 <= int(r[1]) < model.K and 0.0 < float(r[2]) <= 1.0 for r in lines)
    # the arrivals' memberships are the saved model's E-step on their embeddings
    g = Graph(data_root=root, embedding_dim=4)
    g.set_Z(torch.from_numpy(np.load(new / "Z.npy")))
    eng = g.engine(dev)
    comp, prob = model.predict_rows(eng, torch.from_numpy(np.load(new / "Z_new.npy")).to(dev), top=2)
    assert [int(r[1]) for r in lines] == comp[:, 0].tolist() and [float(r[2]) for r in lines] == prob[:, 0].tolist()
    comp, prob = model.predict(eng, top=2)                              # and memberships.tsv its E-step on the table
    print(f"cli: {len(rows)} membership lines in vertex order, {len(lines)} arrivals; components used "
          f"{sorted(set(comp[:, 0].tolist()))} of {model.K}")
    assert [int(r[1]) for r in rows] == comp[:, 0].tolist() and [float(r[2]) for r in rows] == prob[:, 0].tolist()
