"""Soft clusters, the parts that need no GPU: the float64 reference EM and the driver (on the CPU double of the two
kernels of csrc/mixture.h) against scikit-learn where it is installed, the driver's freezing, grouping and choice of the
best restart, the kept model, the refusals, the ABI's new symbols and their argument checks, and the CLI section."""
import ctypes as C
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.engine import SweepEngine

from . import mixture_cases as mc

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ([f"clane_mixture_{w}_{s}" for w in ("estep", "mstep") for s in ("f32", "f64", "bf16")]
               + ["clane_mixture_ll_ws_len", "clane_mixture_mstep_ws_len"])


def _rows(n):
    return torch.arange(n, dtype=torch.int32)


def _fit(X, K, init=None, kernels=None, **kw):
    from clane_amd.mixture import GaussianMixture
    fit_kw = {key: kw.pop(key) for key in ("restarts", "seed") if key in kw}
    eng = mc.cpu_engine(torch.as_tensor(X), kernels)
    gm = GaussianMixture(eng, **kw)
    return gm, gm.fit(eng.Zcur, _rows(X.shape[0]), K, init=init, **fit_kw)


def _same(a, b, r_a, r_b):
    """Restart r_a of fit a and restart r_b of fit b hold the same bits."""
    for f in ("weights", "means", "variances", "lower_bound", "log_likelihood", "iterations", "converged", "clamped",
              "empty"):
        if not torch.equal(getattr(a, f)[r_a], getattr(b, f)[r_b]):
            return False
    return True


# ---- against scikit-learn -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: f"n{s[0]}_d{s[1]}_K{s[2]}")
def test_reference_and_driver_against_scikit_learn(shape):
    """From the same initial parameters the numpy reference and the driver on the CPU double reproduce scikit-learn's
    n_iter_, lower_bound_, weights, means, variances, BIC and AIC to 1e-10 relative (observed <= 2e-14)."""
    sk = pytest.importorskip("sklearn.mixture")
    n, d, K, sep, seed = shape
    X, y, _, _ = mc.planted(n, d, K, sep, seed)
    w0, mu0, var0 = mc.m_step(X, mc.noisy_start(y, K, seed), 1e-6)
    want = sk.GaussianMixture(K, covariance_type="diag", weights_init=w0, means_init=mu0, precisions_init=1.0 / var0,
                              tol=1e-3, max_iter=100, reg_covar=1e-6).fit(X)
    ref = mc.reference_em(X, params0=(w0, mu0, var0))
    _, fit = _fit(X, K, init={"weights": w0[None], "means": mu0[None], "variances": var0[None]})
    got = {"reference": (ref["n_iter"], ref["lower_bounds"][-1], ref["weights"], ref["means"], ref["variances"],
                         ref["bic"], ref["aic"]),
           "driver": (int(fit.iterations[0]), float(fit.lower_bound[0]), fit.weights[0].numpy(), fit.means[0].numpy(),
                      fit.variances[0].numpy(), fit.bic(), fit.aic())}
    for name, (it, lb, w, mu, var, bic, aic) in got.items():
        errs = [abs(lb - want.lower_bound_) / abs(want.lower_bound_), np.abs(w - want.weights_).max() / want.weights_.max(),
                np.abs(mu - want.means_).max() / np.abs(want.means_).max(),
                np.abs(var - want.covariances_).max() / want.covariances_.max(), abs(bic - want.bic(X)) / abs(want.bic(X)),
                abs(aic - want.aic(X)) / abs(want.aic(X))]
        print(name, it, want.n_iter_, errs)
        assert it == want.n_iter_ and want.converged_, name
        assert max(errs) <= 1e-10, (name, errs)


# ---- the driver -------------------------------------------------------------------------------------------------
def _two_starts(shape):
    n, d, K, sep, seed = shape
    X, y, _, _ = mc.planted(n, d, K, sep, seed)
    done = mc.reference_em(X, resp0=mc.one_hot(y, K), tol=1e-9, max_iter=500)["resp"]      # converges at once
    return X, K, torch.from_numpy(np.stack([done, mc.noisy_start(y, K, seed)]))


def test_a_converged_restart_is_frozen_and_restarts_do_not_depend_on_each_other():
    X, K, init = _two_starts(mc.SHAPES[0])
    gm, both = _fit(X, K, init=init)
    it = both.iterations.tolist()
    assert it[0] < it[1] and both.converged.tolist() == [True, True], it
    for r in range(2):                                      # fitted alone: the same bits, the early one included
        _, alone = _fit(X, K, init=init[r:r + 1])
        assert _same(both, alone, r, 0), r
    # after its last iteration restart 0's lower bound stays what it was while restart 1 goes on
    hist = torch.stack(gm.history)
    assert hist.shape[0] == it[1] and bool((hist[it[0] - 1:, 0] == both.lower_bound[0]).all())
    assert bool((hist[1:, 1] >= hist[:-1, 1] - 1e-12).all())           # EM never lowers the bound
    # swapped places: a restart's results do not depend on where it stands
    _, swapped = _fit(X, K, init=init.flip(0))
    assert _same(both, swapped, 0, 1) and _same(both, swapped, 1, 0)


def test_grouping_restarts_changes_no_bit():
    n, d, K, sep, seed = mc.SHAPES[2]
    X, _, _, _ = mc.planted(n, d, K, sep, seed)
    gm_one, one = _fit(X, K, restarts=5, seed=3)
    Kp = mc.padded(K)
    budget = 2 * n * Kp * 8                                 # two restarts' float64 responsibilities per group
    gm_grp, grouped = _fit(X, K, restarts=5, seed=3, resp_budget_bytes=budget)
    assert gm_grp.groups(n, 5, Kp, torch.float64) == [(0, 2), (2, 4), (4, 5)]
    assert gm_one.groups(n, 5, Kp, torch.float64) == [(0, 5)]
    assert all(_same(one, grouped, r, r) for r in range(5)) and one.best == grouped.best
    assert torch.equal(one.assign, grouped.assign) and torch.equal(one.resp, grouped.resp)
    assert gm_grp.passes["estep"] > gm_one.passes["estep"]


def test_best_restart_is_the_highest_lower_bound_ties_to_the_lowest_index():
    X, K, init = _two_starts(mc.SHAPES[2])
    far = torch.from_numpy(mc.one_hot(np.arange(X.shape[0]) % K, K))   # a poor start: rows dealt round robin
    _, fit = _fit(X, K, init=torch.stack([far, init[1], init[1]]), max_iter=2, tol=0.0)
    lb = fit.lower_bound.tolist()
    assert lb[1] == lb[2] and lb[1] > lb[0] and fit.best == 1
    want = mc.e_step(X - fit.mean.numpy(), fit.weights[1].numpy(), fit.centred_means[1].numpy(), fit.variances[1].numpy())
    assert np.abs(fit.resp.numpy() - want[1]).max() <= 1e-12 and np.array_equal(fit.assign.numpy(), want[1].argmax(1))
    assert fit.iterations.tolist() == [2, 2, 2] and fit.converged.tolist() == [False] * 3
    assert float(fit.log_likelihood[1]) == pytest.approx(want[0].mean(), rel=1e-13)
    p = 2 * K * X.shape[1] + K - 1
    n = X.shape[0]
    assert fit.bic() == pytest.approx(-2 * want[0].sum() + p * np.log(n), rel=1e-13)
    assert fit.aic() == pytest.approx(-2 * want[0].sum() + 2 * p, rel=1e-13)


def test_one_component_is_the_sample_mean_and_variance():
    X, _, _, _ = mc.planted(300, 3, 2, 4.0, 2)
    _, fit = _fit(X, 1, restarts=2)
    assert fit.weights.tolist() == [[1.0], [1.0]] and fit.converged.tolist() == [True, True]
    assert np.abs(fit.means[0, 0].numpy() - X.mean(0)).max() <= 1e-13
    assert np.abs(fit.variances[0, 0].numpy() - (X.var(0) + 1e-6)).max() <= 1e-12
    assert bool((fit.resp == 1.0).all()) and bool((fit.assign == 0).all()) and fit.iterations.tolist() == [2, 2]


def test_identical_rows_leave_an_empty_component_and_nothing_is_nan():
    """n identical rows, K = 2: every variance is reg_covar; the component k-means left without rows is counted in
    ``empty``; a rounding that makes S2 / nk - mu^2 negative is clamped and counted."""
    X = np.tile(np.array([[0.5, -1.25, 3.0]]), (40, 1))
    _, fit = _fit(X, 2, restarts=2, reg_covar=1e-4)
    for t in (fit.weights, fit.means, fit.variances, fit.lower_bound, fit.log_likelihood, fit.resp):
        assert bool(torch.isfinite(t).all())
    assert bool((fit.variances == 1e-4).all()) and fit.empty.tolist() == [1, 1] and fit.clamped.tolist() == [0, 0]
    assert np.abs(fit.means[:, 0].numpy() - X[0]).max() <= 1e-15

    class Short(mc.MixtureOracleKernels):                   # S2 comes out a rounding short of nk mu^2
        def mixture_mstep(self, Z, d, rows, mean, resp, ws, S, nk):
            super().mixture_mstep(Z, d, rows, mean, resp, ws, S, nk)
            S.view(-1, 2 * d)[:, :d] -= 1e-9
    _, fit = _fit(X[:, :1], 1, kernels=Short(), restarts=1)
    assert fit.clamped.tolist() == [1] and fit.variances.tolist() == [[[1e-6]]] and bool(torch.isfinite(fit.lower_bound).all())


# ---- the kept model ---------------------------------------------------------------------------------------------
def test_model_round_trip_and_prediction(tmp_path):
    from clane_amd.mixture import GaussianMixture, MixtureModel
    n, d, K, sep, seed = mc.SHAPES[0]
    X, _, _, _ = mc.planted(n, d, K, sep, seed)
    eng = mc.cpu_engine(torch.from_numpy(X))
    gm = GaussianMixture(eng)
    fit = gm.fit(eng.Zcur, _rows(n), K, restarts=2)
    model = fit.model()
    path = model.save(tmp_path / "m.npz")
    with np.load(path) as z:                                # numpy alone, no pickle
        assert sorted(z.files) == sorted(["weights", "centred_means", "variances", "mean", "d", "table", "n_train",
                                          "lower_bound", "iterations", "converged", "reg_covar"])
    back = MixtureModel.load(path, d=d)
    for f in ("weights", "centred_means", "variances", "mean"):
        assert np.array_equal(getattr(back, f), getattr(model, f))
    assert (back.d, back.table, back.n_train, back.iterations, back.converged) == (d, "Z", n, int(fit.iterations[fit.best]),
                                                                                    True)
    assert np.array_equal(back.means, fit.means[fit.best].numpy())
    with pytest.raises(ValueError, match="not 7"):
        MixtureModel.load(path, d=7)
    (tmp_path / "junk.npz").write_bytes(b"no archive")
    with pytest.raises(ValueError, match="is no mixture model"):
        MixtureModel.load(tmp_path / "junk.npz")
    # predict_rows is the E-step: the fit's own memberships for the fitted rows, fresh rows through the same formulas
    comp, prob, proba = back.predict_rows(eng, eng.Zcur, top=3, proba=True)
    assert np.array_equal(proba, fit.resp.numpy()) and np.array_equal(comp[:, 0], fit.assign.numpy())
    order = np.argsort(-proba, axis=1, kind="stable")[:, :3]
    assert np.array_equal(comp, order) and np.array_equal(prob, np.take_along_axis(proba, order, 1))
    comp_v, prob_v = back.predict(eng, vertices=[5, 0, 7], top=1)
    assert np.array_equal(comp_v[:, 0], fit.assign.numpy()[[5, 0, 7]]) and prob_v.shape == (3, 1)
    fresh = torch.from_numpy(mc.planted(50, d, K, sep, seed + 10)[0])
    _, _, proba_f = back.predict_rows(eng, fresh, proba=True)
    want = mc.e_step(fresh.numpy() - model.mean, model.weights, model.centred_means, model.variances)[1]
    assert np.abs(proba_f - want).max() <= 1e-12
    # top beyond K: -1 / 0
    comp8, prob8 = back.predict_rows(eng, fresh, top=8)
    assert comp8.shape == (50, 8) and bool((comp8[:, K:] == -1).all()) and bool((prob8[:, K:] == 0).all())
    assert bool((np.sort(comp8[:, :K], 1) == np.arange(K)).all())
    with pytest.raises(ValueError, match="top must be"):
        back.predict_rows(eng, fresh, top=9)
    with pytest.raises(ValueError, match="Z_new must be"):
        back.predict_rows(eng, fresh.numpy())


# ---- refusals ---------------------------------------------------------------------------------------------------
def test_refusals():
    from clane_amd.mixture import GaussianMixture, check_component_counts
    X = torch.from_numpy(mc.planted(60, 4, 2, 3.0, 0)[0])
    eng = mc.cpu_engine(X)
    gm = GaussianMixture(eng)
    for k in (0, 65):
        with pytest.raises(ValueError, match="1..64 components"):
            gm.fit(eng.Zcur, _rows(60), k)
    with pytest.raises(ValueError, match="must be an integer"):
        gm.fit(eng.Zcur, _rows(60), 2.5)
    with pytest.raises(ValueError, match="at least one row"):
        gm.fit(eng.Zcur, _rows(0), 2)
    with pytest.raises(ValueError, match="init responsibilities must be floating point"):
        gm.fit(eng.Zcur, _rows(60), 2, init=torch.zeros(1, 60, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="init responsibilities"):
        gm.fit(eng.Zcur, _rows(60), 2, init=torch.zeros(1, 59, 2))
    with pytest.raises(ValueError, match="init parameters must be"):
        gm.fit(eng.Zcur, _rows(60), 2, init={"weights": torch.ones(1, 2), "means": torch.zeros(1, 2, 3),
                                            "variances": torch.ones(1, 2, 3)})
    with pytest.raises(ValueError, match="max_iter"):
        GaussianMixture(eng, max_iter=0)
    with pytest.raises(TypeError, match="float32, float64 and bfloat16"):
        gm.fit(eng.Zcur.to(torch.float16), _rows(60), 2)
    for bad in (0, 65, True, 2.0, [], [2, 2], [1, 70]):
        with pytest.raises(ValueError, match="1..64"):
            check_component_counts(bad)
    assert check_component_counts(64) == ([64], False) and check_component_counts([1, 3]) == ([1, 3], True)
    class NoMixture(mc.MixtureOracleKernels):               # a backend without the two kernels: an error, never a fall-back
        mixture_estep = _hip.KernelBackend.mixture_estep
        mixture_mstep = _hip.KernelBackend.mixture_mstep
    with pytest.raises(NotImplementedError, match="NoMixture has no mixture_mstep"):
        GaussianMixture(mc.cpu_engine(X, NoMixture())).fit(eng.Zcur, _rows(60), 2, init=torch.ones(1, 60, 2) / 2)
    eng.columns = True                                       # a column division
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        GaussianMixture(eng)
    eng.columns, eng.world = False, 2
    with pytest.raises(NotImplementedError, match="ONE GPU"):
        GaussianMixture(eng)


# ---- the ABI ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    text = (ROOT / "include" / "clane_hip.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _hip.load_library()
    assert len(NEW_SYMBOLS) == 8
    for name in NEW_SYMBOLS:
        decl = re.search(rf"\b(?:int|int64_t) {name}\s*\(([^;]*)\);", header)
        assert decl and name in _hip.SIGNATURES, name
        assert len(_hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
        assert getattr(lib, name) is not None
    assert re.search(r"#define CLANE_ABI_VERSION 5\b", header) and lib.clane_abi_version() == 5
    assert "clane_mixture_estep_*" in text and "clane_mixture_mstep_ws_len" in text.split("#define CLANE_OK")[0]
    assert re.search(r"#define CLANE_MIXTURE_MAX_COMPONENTS 64\b", header) and _hip.MIXTURE_MAX_COMPONENTS == 64
    # one double per (128-row tile, restart); per 2048-row chunk K rows of [S2 | S1] and one nk
    assert lib.clane_mixture_ll_ws_len(1, 1) == 1 and lib.clane_mixture_ll_ws_len(129, 19) == 2 * 19
    assert lib.clane_mixture_mstep_ws_len(1, 8, 1) == 8 * 3 and lib.clane_mixture_mstep_ws_len(2049, 152, 5) == 2 * 152 * 11
    for name in ("mixture_estep", "mixture_mstep", "mixture_ll_ws_len", "mixture_mstep_ws_len"):
        assert callable(getattr(_hip.HipKernels, name))
    assert [_hip.mixture_padded_components(k) for k in (1, 2, 3, 17, 64)] == [1, 2, 4, 32, 64]


def test_argument_validation_reaches_last_error():
    lib = _hip.load_library()                   # refused on the host before any launch: safe without a GPU
    p = C.cast((C.c_float * 64)(), C.c_void_p)

    def estep(fn=lib.clane_mixture_estep_f32, d=4, ldz=4, n=2, R=2, K=3, flags=3, resp=p, assign=p, ld_assign=2, Z=p,
              mean=p, ll=p, ll_ws=p):
        return fn(Z, 8, d, ldz, p, n, mean, p, p, R, K, flags, resp, ll_ws, ll, assign, ld_assign, None)
    wide = 1 << 29                              # 2 d + 16 would no longer be an int: the one bound on d
    for bad, text in ((dict(d=0), b"bad shape"), (dict(ldz=3), b"bad shape"), (dict(n=-1), b"bad shape"),
                      (dict(d=wide, ldz=wide), b"bad shape"), (dict(K=0), b"K must be in [1, 64]"), (dict(K=65), b"K must be in [1, 64]"),
                      (dict(R=0), b"bad number of restarts"), (dict(flags=4), b"unknown flags"),
                      (dict(ld_assign=1), b"ld_assign"), (dict(ll=None), b"null likelihood"),
                      (dict(ll_ws=None), b"null likelihood"), (dict(Z=None), b"null pointer"),
                      (dict(mean=None), b"null pointer"), (dict(resp=None), b"needs resp"),
                      (dict(assign=None), b"needs assign")):
        assert estep(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"mixture_estep" in lib.clane_last_error()
    assert estep(fn=lib.clane_mixture_estep_bf16, K=-1) == -1 and estep(fn=lib.clane_mixture_estep_f64, d=-1) == -1

    def mstep(fn=lib.clane_mixture_mstep_f32, d=4, ldz=4, n=2, K=8, ws=p, S=p, nk=p, resp=p, mean=p, rows=p):
        return fn(p, 8, d, ldz, rows, n, mean, resp, K, ws, S, nk, None)
    for bad, text in ((dict(d=0), b"bad shape"), (dict(ldz=2), b"bad shape"), (dict(n=-1), b"bad shape"),
                      (dict(d=wide, ldz=wide), b"bad shape"), (dict(K=0), b"bad shape"), (dict(ws=None), b"null workspace"), (dict(S=None), b"null workspace"),
                      (dict(nk=None), b"null workspace"), (dict(resp=None), b"null pointer"),
                      (dict(mean=None), b"null pointer"), (dict(rows=None), b"null pointer")):
        assert mstep(**bad) == -1 and text in lib.clane_last_error(), bad
        assert b"mixture_mstep" in lib.clane_last_error()
    assert mstep(fn=lib.clane_mixture_mstep_bf16, K=-2) == -1 and mstep(fn=lib.clane_mixture_mstep_f64, d=0) == -1


# ---- the CLI section --------------------------------------------------------------------------------------------
CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


def test_the_section_is_validated_before_the_graph_is_loaded(monkeypatch, tmp_path):
    import clane_amd.__main__ as M

    def touched(*a, **k):
        raise AssertionError("the run went on to set up devices")
    monkeypatch.setattr(M, "_distributed_setup", touched)
    monkeypatch.setattr(M, "Graph", touched)
    cfg = tmp_path / "config.yaml"
    args = M.get_parser().parse_args(["--data_root", str(tmp_path), "--output_root", str(tmp_path / "o"),
                                      "--config_file", str(cfg)])
    monkeypatch.setenv("WORLD_SIZE", "2")
    cfg.write_text(CONFIG + "\nsoft_clustering:\n  clusters: 3\n")
    with pytest.raises(NotImplementedError, match="soft_clustering: .* ONE GPU"):
        M.embedding(args)
    monkeypatch.setenv("WORLD_SIZE", "1")
    (tmp_path / "Y").write_text("a\t0\n")
    bad = {"soft_clustering: 7\n": "expected a mapping",
           "soft_clustering:\n  restarts: 3\n": "needs 'clusters'",
           "soft_clustering:\n  clusters: 3\n  colour: red\n": r"unknown keys \['colour'\]",
           "soft_clustering:\n  clusters: 0\n": "1..64", "soft_clustering:\n  clusters: 65\n": "1..64",
           "soft_clustering:\n  clusters: [2, 65]\n": "1..64", "soft_clustering:\n  clusters: 2.5\n": "1..64",
           "soft_clustering:\n  clusters: [2, 2]\n": "distinct",
           "soft_clustering:\n  clusters: 3\n  top: 0\n": "top must be", "soft_clustering:\n  clusters: 3\n  top: 9\n": "top must be",
           "soft_clustering:\n  clusters: 3\n  restarts: 0\n": "restarts must be",
           "soft_clustering:\n  clusters: 3\n  seed: x\n": "seed must be",
           "soft_clustering:\n  clusters: 3\n  max_iter: 0\n": "max_iter must be",
           "soft_clustering:\n  clusters: 3\n  tol: -1\n": "tol must be",
           "soft_clustering:\n  clusters: 3\n  reg_covar: no\n": "reg_covar must be",
           "soft_clustering:\n  clusters: 3\n  criterion: icl\n": "criterion must be",
           "soft_clustering:\n  clusters: 3\n  baseline: 1\n": "baseline must be true or false",
           "soft_clustering:\n  clusters: 3\n  memberships: yes please\n": "memberships must be true or false",
           "soft_clustering:\n  clusters: 3\n  labels: 4\n": "labels must be a file name"}
    for section, text in bad.items():
        cfg.write_text(CONFIG + "\n" + section)
        with pytest.raises(ValueError, match=text):
            M.embedding(args)
    cfg.write_text(CONFIG + "\nsoft_clustering:\n  labels: nowhere\n")
    with pytest.raises(FileNotFoundError, match="labels file .*nowhere"):
        M.embedding(args)
    for section in ("soft_clustering:\n  clusters: 3\n", "soft_clustering:\n  labels: Y\n",
                    "soft_clustering:\n  clusters: [1, 2, 64]\n  criterion: aic\n  top: 8\n  tol: 0.01\n"):
        cfg.write_text(CONFIG + "\n" + section)
        with pytest.raises(AssertionError, match="went on"):            # a valid section passes the validation
            M.embedding(args)
    assert set(vars(M.get_parser().parse_args([]))) == {                # no new flag
        "command", "data_root", "output_root", "config_file", "save_history", "num_workers", "init_Z", "exchange",
        "train_similarity", "predict_links", "link_sources", "gpu"}


def test_the_cli_section_end_to_end_and_a_config_without_it(tmp_path, monkeypatch, capsys):
    import clane_amd.__main__ as M
    from clane_amd.graph import Graph
    from clane_amd.mixture import MixtureModel
    from .conftest import GOLDEN, load_golden, write_data_root
    k = load_golden("g2_karate_csr.npz")
    X = np.random.default_rng(0).standard_normal((34, 4)).astype(np.float32)
    root = write_data_root(tmp_path / "karate", k["vertex_ids"], k["edge_src"], k["edge_dst"], X)
    lines = (GOLDEN / "g2_karate_Y.tsv").read_text().splitlines()
    labelled = lines[::2][::-1]                             # half the vertices, NOT in vertex order
    (root / "Y").write_text("\n".join(labelled) + "\n")

    def cpu_engine(self, device=None, cosine_mode="reference", **kw):
        if self._engine is None:
            self._attach_engine(SweepEngine(self.csr, self.X, "cpu", mc.MixtureOracleKernels(), cosine_mode=cosine_mode))
        if self._dirty:
            self._engine.set_Z(self._Z_host)
            self._dirty = False
        return self._engine
    monkeypatch.setattr(Graph, "engine", cpu_engine)

    def run(cfg_text, out):
        cfg = tmp_path / f"{out}.yaml"
        cfg.write_text(cfg_text)
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg)]))
        return capsys.readouterr().out
    monkeypatch.delitem(sys.modules, "clane_amd.mixture", raising=False)
    plain = run(CONFIG, "plain")
    assert "clane_amd.mixture" not in sys.modules
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["Z.npy"]      # exactly what it wrote before
    with_section = run(CONFIG + "\nsoft_clustering:\n  clusters: [1, 2, 3]\n  labels: Y\n  restarts: 3\n  seed: 1\n"
                                "  baseline: true\n  memberships: true\n  top: 2\n", "mix")
    assert "clane_amd.mixture" in sys.modules
    assert np.array_equal(np.load(tmp_path / "plain" / "Z.npy"), np.load(tmp_path / "mix" / "Z.npy"))
    assert sorted(p.name for p in (tmp_path / "mix").iterdir()) == ["Z.npy", "memberships.tsv", "mixture_metrics.json",
                                                                    "mixture_model.npz"]
    strip = lambda text, out: text.replace(str(tmp_path / out), "O")     # noqa: E731
    lines, base = strip(with_section, "mix").splitlines(), strip(plain, "plain").splitlines()
    assert lines[:len(base)] == base and len(lines) == len(base) + 1 and "17 vertices into" in lines[-1]
    got = json.loads((tmp_path / "mix" / "mixture_metrics.json").read_text())
    assert set(got) == {"labels", "clustered", "class_names", "clusters", "restarts", "seed", "criterion", "tables"}
    assert got["clustered"] == len(labelled) == 17 and got["restarts"] == 3 and got["seed"] == 1 and got["criterion"] == "bic"
    assert set(got["tables"]) == {"Z", "X"}
    for t in got["tables"].values():
        assert set(t) == {"clusters", "log_likelihood", "lower_bound", "bic", "aic", "iterations", "converged",
                          "best_restart", "weights", "soft_sizes", "sizes", "empty", "clamped", "mean_entropy", "confident",
                          "nmi", "ari", "purity", "selection"}
        sel = t["selection"]
        assert sel["criterion"] == "bic" and [c["clusters"] for c in sel["candidates"]] == [1, 2, 3]
        assert sel["chosen"] == t["clusters"] == min(sel["candidates"], key=lambda c: (c["bic"], c["clusters"]))["clusters"]
        assert sum(t["sizes"]) == 17 and sum(t["soft_sizes"]) == pytest.approx(17.0, abs=1e-3)
        assert sum(t["weights"]) == pytest.approx(1.0, abs=1e-12) and 0.0 <= t["mean_entropy"] <= 1.0
        assert 0.0 <= t["confident"] <= 1.0 and 0.0 <= t["nmi"] <= 1.0 and -1.0 <= t["ari"] <= 1.0
    assert got["clusters"] == got["tables"]["Z"]["clusters"]
    model = MixtureModel.load(tmp_path / "mix" / "mixture_model.npz", d=4)
    assert model.K == got["clusters"] and model.table == "Z" and model.n_train == 17
    # memberships.tsv: EVERY vertex, in vertex order (not the labels file's), under the saved model
    rows = [r.split("\t") for r in (tmp_path / "mix" / "memberships.tsv").read_text().splitlines()]
    assert [r[0] for r in rows] == [str(i) for i in k["vertex_ids"]]
    g = Graph(data_root=root, embedding_dim=4)
    g.set_Z(torch.from_numpy(np.load(tmp_path / "mix" / "Z.npy")))
    comp, prob = model.predict(g.engine(), top=2)
    assert [int(r[1]) for r in rows] == comp[:, 0].tolist() and [float(r[2]) for r in rows] == prob[:, 0].tolist()
    width = 1 + 2 * min(2, model.K)
    assert all(len(r) == width and 0 <= int(r[1]) < model.K and repr(float(r[2])) == r[2] for r in rows)
    assert all(float(r[2]) >= float(r[4]) for r in rows if len(r) > 3)
