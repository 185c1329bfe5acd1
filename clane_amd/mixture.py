"""Soft clusters on a SweepEngine: diagonal-covariance Gaussian mixtures fitted by EM on the embeddings, every restart
advancing at once on the card -- per-vertex membership probabilities, a likelihood (and with it BIC / AIC, a model-based
way to choose the number of components) and a kept model that assigns new rows without refitting.  The model is
scikit-learn's ``GaussianMixture(covariance_type="diag")``: the same E-step expansion, M-step, stop test and
``init_params="kmeans"``.

One EM iteration is two kernels of csrc/mixture.h.  The rows are centred by their float64 column mean, rounded once to
the accumulate type, inside the kernels' loaders; both steps contract the 2 d wide operand [xc^2 | xc] on the matrix
cores: the E-step against the stacked [-a/2 | mu a] with the log-sum-exp, the responsibilities and the arg-max fused in
(the logits never exist), the M-step over the rows, giving S1 = r^T xc, S2 = r^T xc^2 and nk.  What remains for torch is
the finish in float64 -- pi = nk / sum nk, mu = S1 / nk, var = max(S2 / nk - mu^2, 0) + reg_covar -- the stop test and the
freezing of converged restarts.

Everything works on TABLE ROWS of the engine's tables.  One GPU only: a fit reads arbitrary rows of the table.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from .classify import table_and_rows
from .train import require_one_gpu

RESP_BUDGET_BYTES = 8 << 30         # the [n, Rg * Kp] responsibilities of one group of restarts
CRITERIA = ("bic", "aic")
MODEL_KEYS = ("weights", "centred_means", "variances", "mean", "d", "table", "n_train", "lower_bound", "iterations",
              "converged", "reg_covar")
_EPS64 = float(torch.finfo(torch.float64).eps)


def _per_restart(fn, t: torch.Tensor) -> torch.Tensor:
    """``fn`` of every restart's slice, restart by restart: a reduction sees the same shape whatever R is."""
    return torch.stack([fn(t[r]) for r in range(t.shape[0])])


def stack_parameters(weights: torch.Tensor, mu: torch.Tensor, var: torch.Tensor, Kp: int, acc: torch.dtype):
    """(Wm [R * Kp, 2 d], cst [R * Kp]) in ``acc`` from float64 weights [R, K], CENTRED means and variances [R, K, d]:
    a = 1 / var, Wm = [-a / 2 | mu a], cst = log pi - (d log 2 pi + sum log var + sum mu^2 a) / 2, computed in float64 and
    rounded once; the rows of pad components are zero."""
    R, K, d = mu.shape
    a = 1.0 / var
    quad = _per_restart(lambda t: t.sum(-1), torch.log(var) + mu * mu * a)
    const = torch.log(weights) - 0.5 * (d * math.log(2.0 * math.pi) + quad)
    Wm = torch.zeros(R, Kp, 2 * d, dtype=torch.float64, device=mu.device)
    Wm[:, :K, :d] = -0.5 * a
    Wm[:, :K, d:] = mu * a
    cst = torch.zeros(R, Kp, dtype=torch.float64, device=mu.device)
    cst[:, :K] = const
    return Wm.view(R * Kp, 2 * d).to(acc).contiguous(), cst.view(R * Kp).to(acc).contiguous()


def finish_mstep(S: torch.Tensor, nk: torch.Tensor, R: int, K: int, Kp: int, d: int, reg_covar: float):
    """(weights [R, K], centred means, variances [R, K, d], clamped [R], empty [R]) in float64 from the M-step's sums
    S [R * Kp, 2 d] = [S2 | S1] and nk [R * Kp]: nk += 10 eps, pi = nk / sum nk, mu = S1 / nk, var = max(S2 / nk - mu^2,
    0) + reg_covar.  ``clamped`` counts the entries the max acted on, ``empty`` the components with nk < 1."""
    S = S.double().view(R, Kp, 2 * d)[:, :K]
    raw = nk.double().view(R, Kp)[:, :K]
    n_k = raw + 10.0 * _EPS64
    total = _per_restart(lambda t: t.sum(), n_k)
    mu = S[:, :, d:] / n_k[:, :, None]
    diff = S[:, :, :d] / n_k[:, :, None] - mu * mu
    clamped = (diff < 0).sum((1, 2))
    var = diff.clamp(min=0.0) + reg_covar
    return n_k / total[:, None], mu, var, clamped, (raw < 1.0).sum(1)


def parameter_count(K: int, d: int) -> int:
    """Free parameters of a diagonal mixture: K d means, K d variances, K - 1 weights."""
    return 2 * K * d + K - 1


def check_component_counts(k, what: str = "soft_cluster") -> Tuple[List[int], bool]:
    """(the list of component counts, whether ``k`` was a sequence): one integer in 1..64 or a non-empty sequence of
    distinct ones."""
    def ok(v):
        return not isinstance(v, bool) and isinstance(v, int) and 1 <= v <= _hip.MIXTURE_MAX_COMPONENTS
    if isinstance(k, torch.Tensor):
        k = k.tolist()
    if isinstance(k, (list, tuple, range)):
        ks = list(k)
        if not ks or not all(ok(v) for v in ks) or len(set(ks)) != len(ks):
            raise ValueError(f"{what}: a list of component counts needs distinct integers in "
                             f"1..{_hip.MIXTURE_MAX_COMPONENTS}, got {k!r}")
        return ks, True
    if not ok(k):
        raise ValueError(f"{what}: the number of components must be an integer in 1..{_hip.MIXTURE_MAX_COMPONENTS} or a "
                         f"list of them, got {k!r}")
    return [k], False


# ---- the kept model ---------------------------------------------------------------------------------------------
@dataclass
class MixtureModel:
    """One fitted mixture, on the host: what ``MixtureFit.model`` returns, a file keeps and ``predict*`` apply."""
    weights: np.ndarray         # [K] float64
    centred_means: np.ndarray   # [K, d] float64: the means about ``mean``
    variances: np.ndarray       # [K, d] float64
    mean: np.ndarray            # [d] float64: the centring the kernels subtract (exact in the accumulate type)
    d: int
    table: str = "Z"
    n_train: int = 0
    lower_bound: float = float("nan")
    iterations: int = 0
    converged: bool = False
    reg_covar: float = 1e-6

    def __post_init__(self):
        w, mu, var, m = (np.asarray(getattr(self, f), dtype=np.float64) for f in ("weights", "centred_means",
                                                                                   "variances", "mean"))
        K = w.shape[0] if w.ndim == 1 else -1
        if not 1 <= K <= _hip.MIXTURE_MAX_COMPONENTS or mu.shape != (K, int(self.d)) or var.shape != mu.shape \
                or m.shape != (int(self.d),):
            raise ValueError(f"MixtureModel: weights {w.shape}, means {mu.shape}, variances {var.shape} and mean {m.shape} "
                             f"are no mixture of 1..{_hip.MIXTURE_MAX_COMPONENTS} components for d = {self.d}")
        if not (var > 0).all():
            raise ValueError("MixtureModel: variances must be positive")
        if self.table not in ("Z", "X"):
            raise ValueError(f"MixtureModel: table must be 'Z' or 'X', got {self.table!r}")
        self.weights, self.centred_means, self.variances, self.mean = w, mu, var, m

    @property
    def K(self) -> int:
        return int(self.weights.shape[0])

    @property
    def means(self) -> np.ndarray:
        """[K, d] float64: the components' means in the table's coordinates."""
        return self.centred_means + self.mean[None, :]

    def save(self, path) -> Path:
        """One ``.npz`` of MODEL_KEYS, read with numpy alone."""
        path = Path(path)
        with open(path, "wb") as io:
            np.savez(io, weights=self.weights, centred_means=self.centred_means, variances=self.variances, mean=self.mean,
                     d=np.int64(self.d), table=np.str_(self.table), n_train=np.int64(self.n_train),
                     lower_bound=np.float64(self.lower_bound), iterations=np.int64(self.iterations),
                     converged=np.bool_(self.converged), reg_covar=np.float64(self.reg_covar))
        return path

    @classmethod
    def load(cls, path, d: Optional[int] = None) -> "MixtureModel":
        """The model of ``save``; ``d``: the width it must have.  A file that is no such archive is a ValueError."""
        name = os.fspath(path)
        missing = []
        try:
            with np.load(name) as z:
                missing = [key for key in MODEL_KEYS if key not in z.files]
                fields = None if missing else dict(weights=np.array(z["weights"]), centred_means=np.array(z["centred_means"]),
                              variances=np.array(z["variances"]), mean=np.array(z["mean"]), d=int(z["d"]),
                              table=str(z["table"]), n_train=int(z["n_train"]), lower_bound=float(z["lower_bound"]),
                              iterations=int(z["iterations"]), converged=bool(z["converged"]),
                              reg_covar=float(z["reg_covar"]))
        except Exception as e:                              # a truncated or foreign file: zipfile / numpy errors
            raise ValueError(f"MixtureModel.load: {name!r} is no mixture model: {type(e).__name__}: {e}") from None
        if missing:
            raise ValueError(f"MixtureModel.load: {name!r} lacks {missing}")
        model = cls(**fields)
        if d is not None and int(d) != model.d:
            raise ValueError(f"MixtureModel.load: {name!r} holds a model for d = {model.d}, not {int(d)}")
        return model

    # ---- applying it: the E-step alone --------------------------------------------------------------------------
    def _apply(self, engine, Z, rows, top: int, proba: bool):
        if isinstance(top, bool) or int(top) != top or not 1 <= int(top) <= _hip.PREDICT_MAX_TOP:
            raise ValueError(f"predict: top must be an integer in 1..{_hip.PREDICT_MAX_TOP}, got {top!r}")
        if Z.dim() != 2 or int(Z.shape[1]) < self.d or int(engine.d) != self.d:
            raise ValueError(f"the model was fitted for d = {self.d}; the engine has d = {engine.d} and the table rows of "
                             f"{tuple(Z.shape)[1:]}")
        gm = GaussianMixture(engine)
        dev = Z.device
        resp, assign, _ = gm.responsibilities(
            Z, rows, torch.from_numpy(self.weights).to(dev)[None], torch.from_numpy(self.centred_means).to(dev)[None],
            torch.from_numpy(self.variances).to(dev)[None], torch.from_numpy(self.mean).to(dev))
        comp, prob = top_components(resp[:, :self.K], assign[:, 0], int(top))
        res = (comp.cpu().numpy(), prob.double().cpu().numpy())
        return res + (resp[:, :self.K].double().cpu().numpy(),) if proba else res

    def predict(self, engine, vertices=None, top: int = 3, proba: bool = False):
        """(components [m, top] int32, probs [m, top] float64[, proba [m, K]]) on the host for the vertices (default:
        all, in vertex order) from the engine's table ``self.table``: the ``top`` components of highest responsibility,
        best first, ties to the lowest component, -1 / 0 where K < top."""
        if vertices is None:
            vertices = torch.arange(engine.V)
        Z, rows = table_and_rows(engine, vertices, self.table)
        return self._apply(engine, Z, rows, top, proba)

    def predict_rows(self, engine, Z_new: torch.Tensor, top: int = 3, proba: bool = False):
        """The same for the rows of ``Z_new`` [m, d], a device tensor of a table dtype (the embeddings of new vertices,
        say: rows that are in no table), read with identity rows."""
        if not isinstance(Z_new, torch.Tensor) or Z_new.dim() != 2 or \
                Z_new.dtype not in (torch.float32, torch.float64, torch.bfloat16):
            raise ValueError("predict_rows: Z_new must be a [m, d] tensor of dtype float32, float64 or bfloat16")
        rows = torch.arange(Z_new.shape[0], dtype=torch.int32, device=Z_new.device)
        return self._apply(engine, Z_new, rows, top, proba)


def top_components(resp: torch.Tensor, assign: torch.Tensor, top: int):
    """(components [n, top] int32, probs [n, top]) from responsibilities [n, K] and the kernel's arg-max [n]: the arg-max
    first, then the others by responsibility descending, ties to the lowest component; -1 / 0 where K < top."""
    n, K = resp.shape
    key = resp.clone()
    if n:
        key[torch.arange(n, device=resp.device), assign.long()] = 2.0        # above every probability
    order = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :top]
    comp = torch.full((n, top), -1, dtype=torch.int32, device=resp.device)
    prob = torch.zeros(n, top, dtype=resp.dtype, device=resp.device)
    comp[:, :order.shape[1]] = order.to(torch.int32)
    prob[:, :order.shape[1]] = resp.gather(1, order)
    return comp, prob


# ---- the fit ----------------------------------------------------------------------------------------------------
@dataclass
class MixtureFit:
    weights: torch.Tensor           # [R, K] float64, on the device
    means: torch.Tensor             # [R, K, d] float64: in the table's coordinates (the centring mean added back)
    variances: torch.Tensor         # [R, K, d] float64
    lower_bound: torch.Tensor       # [R] float64: the mean log-likelihood per row of the last E-step of the loop
    log_likelihood: torch.Tensor    # [R] float64: the mean log-likelihood per row under the FINAL parameters
    iterations: torch.Tensor        # [R] int64
    converged: torch.Tensor         # [R] bool
    clamped: torch.Tensor           # [R] int64: variance entries the max(., 0) acted on in the restart's last M-step
    empty: torch.Tensor             # [R] int64: components with nk < 1 in the restart's last M-step
    best: int                       # highest lower_bound, ties to the lowest index
    assign: torch.Tensor            # [n] int32: the best restart's arg-max component, ties to the lowest
    resp: torch.Tensor              # [n, K] accumulate dtype: the best restart's responsibilities
    centred_means: torch.Tensor     # [R, K, d] float64: the means about ``mean``
    mean: torch.Tensor              # [d] float64: the centring, exact in the accumulate dtype
    n: int
    reg_covar: float = 1e-6

    @property
    def K(self) -> int:
        return int(self.weights.shape[1])

    @property
    def d(self) -> int:
        return int(self.means.shape[2])

    def bic(self, restart: Optional[int] = None) -> float:
        r = self.best if restart is None else int(restart)
        return -2.0 * float(self.log_likelihood[r]) * self.n + parameter_count(self.K, self.d) * math.log(self.n)

    def aic(self, restart: Optional[int] = None) -> float:
        r = self.best if restart is None else int(restart)
        return -2.0 * float(self.log_likelihood[r]) * self.n + 2.0 * parameter_count(self.K, self.d)

    def model(self, restart: Optional[int] = None, table: str = "Z") -> MixtureModel:
        r = self.best if restart is None else int(restart)
        return MixtureModel(weights=self.weights[r].cpu().numpy(), centred_means=self.centred_means[r].cpu().numpy(),
                            variances=self.variances[r].cpu().numpy(), mean=self.mean.cpu().numpy(), d=self.d, table=table,
                            n_train=self.n, lower_bound=float(self.lower_bound[r]), iterations=int(self.iterations[r]),
                            converged=bool(self.converged[r]), reg_covar=self.reg_covar)


class GaussianMixture:
    """EM for diagonal Gaussian mixtures on rows of a table of ``engine``, ``restarts`` runs at once.  Per restart, in
    scikit-learn's order: E-step, M-step, lb = ll / n, converged when |lb - lb_prev| < tol; a converged restart is
    frozen -- its parameters, lower bound and iteration count no longer change while the others go on.  If the
    responsibilities ``resp [n, R Kp]`` would exceed ``resp_budget_bytes`` the kernel passes run in groups of restarts;
    the state is one tensor for all restarts either way, and the kernels give a restart the same bits whatever shares its
    call, so the grouping changes no result."""

    def __init__(self, engine, reg_covar: float = 1e-6, tol: float = 1e-3, max_iter: int = 100,
                 resp_budget_bytes: int = RESP_BUDGET_BYTES):
        try:
            require_one_gpu(engine)
        except NotImplementedError:
            raise NotImplementedError(
                f"the Gaussian mixture runs on ONE GPU only: a fit reads arbitrary rows of the table, which this engine "
                f"divides over {engine.world} ranks (exchange={engine.exchange!r}); several GPUs are out of scope") from None
        if not reg_covar >= 0 or not tol >= 0 or isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 1 \
                or resp_budget_bytes < 1:
            raise ValueError("GaussianMixture: reg_covar >= 0, tol >= 0, max_iter an integer >= 1, resp_budget_bytes >= 1")
        self.eng, self.k = engine, engine.k
        self.reg_covar, self.tol, self.max_iter = float(reg_covar), float(tol), int(max_iter)
        self.resp_budget_bytes = int(resp_budget_bytes)
        self.passes = {"estep": 0, "mstep": 0}      # kernel calls of the last fit()
        self.history: List[torch.Tensor] = []       # the lower bounds [R] after every iteration of the last fit()

    def table_and_rows(self, vertices, table: str = "Z"):
        """(table, int32 rows) for vertex indices: the current embeddings ("Z") or the content embeddings ("X")."""
        return table_and_rows(self.eng, vertices, table)

    def groups(self, n: int, R: int, Kp: int, acc: torch.dtype) -> List[Tuple[int, int]]:
        per = max(1, self.resp_budget_bytes // max(1, n * Kp * torch.empty(0, dtype=acc).element_size()))
        return [(a, min(a + per, R)) for a in range(0, R, per)]

    # ---- pieces -------------------------------------------------------------------------------------------------
    def column_mean(self, Z, rows) -> torch.Tensor:
        """The float64 column mean of the listed rows through the library's deterministic column sums, rounded once to the
        accumulate dtype (and returned as the float64 holding exactly that value)."""
        d, n = self.eng.d, int(rows.numel())
        ws = torch.empty(max(1, self.k.column_sums_ws_len(n, d)), dtype=torch.float64, device=Z.device)
        sums = torch.empty(d, dtype=torch.float64, device=Z.device)
        self.k.column_sums(Z, d, rows, ws, sums)
        return (sums / n).to(_hip.acc_dtype(Z.dtype)).double()

    def _estep(self, Z, rows, mean_acc, Wm, cst, R, K, ll, resp=None, assign=None):
        n = int(rows.numel())
        ll_ws = torch.empty(max(1, self.k.mixture_ll_ws_len(n, R)), dtype=torch.float64, device=Z.device)
        self.k.mixture_estep(Z, self.eng.d, rows, mean_acc, Wm, cst, R, K, ll_ws, ll, resp=resp, assign=assign)
        self.passes["estep"] += 1

    def _mstep(self, Z, rows, mean_acc, resp, S, nk):
        n, d = int(rows.numel()), self.eng.d
        ws = torch.empty(max(1, self.k.mixture_mstep_ws_len(n, int(nk.numel()), d)), dtype=S.dtype, device=Z.device)
        self.k.mixture_mstep(Z, d, rows, mean_acc, resp, ws, S, nk)
        self.passes["mstep"] += 1

    def responsibilities(self, Z, rows, weights, mu, var, mean):
        """(resp [n, R * Kp], assign [n, R] int32, ll [R] float64) of the rows under float64 parameters [R, K(, d)] with
        CENTRED means and the centring ``mean`` [d]: one E-step per group of restarts."""
        dev, acc = Z.device, _hip.acc_dtype(Z.dtype)
        rows = rows.to(dev, torch.int32).contiguous()
        n, (R, K, d) = int(rows.numel()), mu.shape
        if d != self.eng.d:
            raise ValueError(f"responsibilities: the parameters have d = {d}, the engine {self.eng.d}")
        Kp = _hip.mixture_padded_components(K)
        Wm, cst = stack_parameters(weights.double(), mu.double(), var.double(), Kp, acc)
        mean_acc = mean.to(dev, acc).contiguous()
        resp = torch.empty(n, R * Kp, dtype=acc, device=dev)
        assign = torch.empty(n, R, dtype=torch.int32, device=dev)
        ll = torch.zeros(R, dtype=torch.float64, device=dev)
        if n == 0:
            return resp, assign, ll
        for a, b in self.groups(n, R, Kp, acc):
            part = torch.empty(n, (b - a) * Kp, dtype=acc, device=dev)
            part_assign = torch.empty(n, b - a, dtype=torch.int32, device=dev)
            self._estep(Z, rows, mean_acc, Wm[a * Kp:b * Kp], cst[a * Kp:b * Kp], b - a, K, ll[a:b], part, part_assign)
            resp[:, a * Kp:b * Kp] = part
            assign[:, a:b] = part_assign
        return resp, assign, ll

    # ---- the batched fit ----------------------------------------------------------------------------------------
    def fit(self, Z: torch.Tensor, rows: torch.Tensor, k: int, restarts: int = 10, seed: int = 0, init=None) -> MixtureFit:
        """Fit ``k`` components to the rows ``rows`` (int32 table rows of ``Z``), ``restarts`` times.  The initial state is
        the M-step of the one-hot partitions of ``KMeans(engine).fit(Z, rows, k, restarts=restarts, seed=seed)``
        (scikit-learn's ``init_params="kmeans"``), of explicit responsibilities ``init`` ([R, n, k]), or the explicit
        parameters ``init = {"weights": [R, k], "means": [R, k, d], "variances": [R, k, d]}`` (means in the table's
        coordinates)."""
        eng, dev, d = self.eng, Z.device, self.eng.d
        acc = _hip.acc_dtype(Z.dtype)
        rows = rows.to(dev, torch.int32).contiguous()
        n = int(rows.numel())
        if isinstance(k, bool) or int(k) != k:
            raise ValueError(f"fit: the number of components must be an integer, got {k!r}")
        K = int(k)
        Kp = _hip.mixture_padded_components(K)              # refuses K outside 1..64
        if n < 1:
            raise ValueError("fit: at least one row")
        self.passes = {"estep": 0, "mstep": 0}
        self.history = []
        mean = self.column_mean(Z, rows)
        mean_acc = mean.to(acc).contiguous()

        params = None
        if isinstance(init, dict):
            if set(init) != {"weights", "means", "variances"}:
                raise ValueError("fit: init parameters are {'weights', 'means', 'variances'}")
            w0 = torch.as_tensor(init["weights"]).to(dev, torch.float64)
            m0 = torch.as_tensor(init["means"]).to(dev, torch.float64)
            v0 = torch.as_tensor(init["variances"]).to(dev, torch.float64)
            if w0.dim() != 2 or w0.shape[1] != K or tuple(m0.shape) != (w0.shape[0], K, d) or v0.shape != m0.shape:
                raise ValueError(f"fit: init parameters must be weights [R, {K}], means and variances [R, {K}, {d}]")
            if not bool((v0 > 0).all()) or not bool((w0 > 0).all()):
                raise ValueError("fit: init weights and variances must be positive")
            R = int(w0.shape[0])
            params = (w0, m0 - mean[None, None, :], v0)
        elif init is not None:
            init = torch.as_tensor(init)
            if init.dim() != 3 or init.shape[1] != n or init.shape[2] != K or not init.dtype.is_floating_point:
                raise ValueError(f"fit: init responsibilities must be floating point [R, n = {n}, k = {K}], got "
                                 f"{tuple(init.shape)} {init.dtype}")
            R = int(init.shape[0])
        else:
            if isinstance(restarts, bool) or int(restarts) != restarts or restarts < 1:
                raise ValueError("fit: restarts must be an integer >= 1")
            R = int(restarts)
        groups = self.groups(n, R, Kp, acc)
        width = max(b - a for a, b in groups) * Kp
        resp = torch.empty(n * width, dtype=acc, device=dev)
        S = torch.empty(R * Kp, 2 * d, dtype=acc, device=dev)
        nk = torch.empty(R * Kp, dtype=acc, device=dev)
        ll = torch.zeros(R, dtype=torch.float64, device=dev)

        if params is None:                                  # the M-step of the initial responsibilities
            part = None
            if init is None:
                from .cluster import KMeans
                part = KMeans(eng).fit(Z, rows, K, restarts=R, seed=seed).assign        # [n, R] int32
            for a, b in groups:
                buf = resp[:n * (b - a) * Kp].view(n, b - a, Kp)
                buf.zero_()
                if part is not None:
                    buf.scatter_(2, part[:, a:b].long()[:, :, None], 1.0)
                else:
                    buf[:, :, :K] = init[a:b].to(dev, acc).permute(1, 0, 2)
                self._mstep(Z, rows, mean_acc, resp[:n * (b - a) * Kp], S[a * Kp:b * Kp], nk[a * Kp:b * Kp])
            weights, mu, var, clamped, empty = finish_mstep(S, nk, R, K, Kp, d, self.reg_covar)
        else:
            weights, mu, var = params
            clamped = torch.zeros(R, dtype=torch.int64, device=dev)
            empty = torch.zeros(R, dtype=torch.int64, device=dev)

        active = torch.ones(R, dtype=torch.bool, device=dev)
        converged = torch.zeros(R, dtype=torch.bool, device=dev)
        lb = torch.full((R,), -math.inf, dtype=torch.float64, device=dev)
        iterations = torch.zeros(R, dtype=torch.int64, device=dev)
        live = [True] * R
        for it in range(1, self.max_iter + 1):
            Wm, cst = stack_parameters(weights, mu, var, Kp, acc)
            for a, b in groups:
                if not any(live[a:b]):                      # every restart of the group is frozen
                    continue
                flat = resp[:n * (b - a) * Kp]
                self._estep(Z, rows, mean_acc, Wm[a * Kp:b * Kp], cst[a * Kp:b * Kp], b - a, K, ll[a:b], resp=flat)
                self._mstep(Z, rows, mean_acc, flat, S[a * Kp:b * Kp], nk[a * Kp:b * Kp])
            w_new, mu_new, var_new, cl_new, em_new = finish_mstep(S, nk, R, K, Kp, d, self.reg_covar)
            lb_new = ll / n
            upd = active
            weights = torch.where(upd[:, None], w_new, weights)
            mu = torch.where(upd[:, None, None], mu_new, mu)
            var = torch.where(upd[:, None, None], var_new, var)
            clamped, empty = torch.where(upd, cl_new, clamped), torch.where(upd, em_new, empty)
            done_now = upd & ((lb_new - lb).abs() < self.tol)
            lb = torch.where(upd, lb_new, lb)
            iterations = torch.where(upd, torch.full_like(iterations, it), iterations)
            converged = converged | done_now
            active = active & ~done_now
            self.history.append(lb.clone())
            live = active.tolist()                          # the one host read of the iteration
            if not any(live):
                break

        # the final E-step under the final parameters: every restart's likelihood, the best one's memberships
        scores = [(-math.inf if v != v else v) for v in lb.tolist()]
        best = max(range(R), key=lambda r: (scores[r], -r))
        Wm, cst = stack_parameters(weights, mu, var, Kp, acc)
        ll_final = torch.zeros(R, dtype=torch.float64, device=dev)
        for a, b in groups:
            self._estep(Z, rows, mean_acc, Wm[a * Kp:b * Kp], cst[a * Kp:b * Kp], b - a, K, ll_final[a:b])
        best_resp = torch.empty(n, Kp, dtype=acc, device=dev)
        best_assign = torch.empty(n, 1, dtype=torch.int32, device=dev)
        self._estep(Z, rows, mean_acc, Wm[best * Kp:(best + 1) * Kp], cst[best * Kp:(best + 1) * Kp], 1, K,
                    torch.zeros(1, dtype=torch.float64, device=dev), resp=best_resp, assign=best_assign)
        return MixtureFit(weights=weights, means=mu + mean[None, None, :], variances=var, lower_bound=lb,
                          log_likelihood=ll_final / n, iterations=iterations, converged=converged, clamped=clamped,
                          empty=empty, best=best, assign=best_assign[:, 0].contiguous(),
                          resp=best_resp[:, :K].contiguous(), centred_means=mu, mean=mean, n=n, reg_covar=self.reg_covar)


# ---- the experiment ---------------------------------------------------------------------------------------------
SELECTION_FIELDS = ("clusters", "log_likelihood", "lower_bound", "bic", "aic", "iterations", "converged", "empty")


def describe_fit(fit: MixtureFit, table: str, restarts: int, seed: int) -> dict:
    """The result dict of one fitted component count: the best restart's scores and what its memberships look like."""
    b, K, n = fit.best, fit.K, fit.n
    r = fit.resp.double()
    plogp = torch.where(r > 0, r * torch.log(r.clamp(min=1e-300)), torch.zeros_like(r))
    entropy = -plogp.sum(1) / math.log(K) if K > 1 else torch.zeros(n, dtype=torch.float64, device=r.device)
    return {"table": table, "clustered": n, "clusters": K, "restarts": int(restarts), "seed": int(seed),
            "log_likelihood": float(fit.log_likelihood[b]), "lower_bound": float(fit.lower_bound[b]),
            "bic": fit.bic(), "aic": fit.aic(), "iterations": int(fit.iterations[b]), "converged": bool(fit.converged[b]),
            "best_restart": b, "weights": fit.weights[b].tolist(), "soft_sizes": r.sum(0).tolist(),
            "sizes": torch.bincount(fit.assign.long(), minlength=K).tolist(), "empty": int(fit.empty[b]),
            "clamped": int(fit.clamped[b]), "mean_entropy": float(entropy.sum() / n),
            "confident": float((r.max(1).values >= 0.9).double().sum() / n)}


def select_components(results: Sequence[dict], criterion: str) -> dict:
    """The result of lowest ``criterion``, ties to the smaller count, with ``selection = {criterion, candidates,
    chosen}`` added."""
    best = None
    for i, r in enumerate(results):
        v = r[criterion]
        if v != v:
            continue
        if best is None or v < results[best][criterion] or \
                (v == results[best][criterion] and r["clusters"] < results[best]["clusters"]):
            best = i
    if best is None:
        raise ValueError("soft_cluster: no candidate has a finite criterion")
    out = dict(results[best])
    out["selection"] = {"criterion": criterion, "candidates": [{f: r.get(f) for f in SELECTION_FIELDS} for r in results],
                        "chosen": int(results[best]["clusters"])}
    return out


# ---- the CLI section `soft_clustering` ----------------------------------------------------------------------------
SECTION_KEYS = ("clusters", "labels", "restarts", "seed", "max_iter", "tol", "reg_covar", "criterion", "baseline",
                "memberships", "top")


def check_section(section, data_root, world_size: int = 1) -> dict:
    """The validated ``soft_clustering`` section of a config, the labels file resolved against ``data_root``.  Before any
    graph is read."""
    if world_size > 1:
        raise NotImplementedError(
            "soft_clustering: fitting a Gaussian mixture runs on ONE GPU only (WORLD_SIZE > 1): several GPUs are out of "
            "scope")
    if not isinstance(section, dict):
        raise ValueError("soft_clustering: expected a mapping with the key `clusters` or `labels`")
    unknown = sorted(set(section) - set(SECTION_KEYS))
    if unknown:
        raise ValueError(f"soft_clustering: unknown keys {unknown}; known: {list(SECTION_KEYS)}")
    labels = section.get("labels")
    if labels is not None and (not isinstance(labels, str) or not labels):
        raise ValueError(f"soft_clustering: labels must be a file name, got {labels!r}")
    if labels is not None:
        labels = Path(labels) if Path(labels).is_absolute() else Path(data_root) / labels
    clusters = section.get("clusters")
    if clusters is None and labels is None:
        raise ValueError("soft_clustering: the section needs 'clusters', the number of components (or a list), or 'labels', "
                         "whose number of classes it defaults to")
    if clusters is not None:
        check_component_counts(clusters, "soft_clustering: clusters")
    whole = lambda v: isinstance(v, int) and not isinstance(v, bool)    # noqa: E731
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)   # noqa: E731
    restarts, seed, max_iter = section.get("restarts", 10), section.get("seed", 0), section.get("max_iter", 100)
    if not whole(restarts) or restarts < 1:
        raise ValueError(f"soft_clustering: restarts must be an integer >= 1, got {restarts!r}")
    if not whole(seed):
        raise ValueError(f"soft_clustering: seed must be an integer, got {seed!r}")
    if not whole(max_iter) or max_iter < 1:
        raise ValueError(f"soft_clustering: max_iter must be an integer >= 1, got {max_iter!r}")
    tol, reg_covar = section.get("tol", 1e-3), section.get("reg_covar", 1e-6)
    if not number(tol) or tol < 0:
        raise ValueError(f"soft_clustering: tol must be a number >= 0, got {tol!r}")
    if not number(reg_covar) or reg_covar < 0:
        raise ValueError(f"soft_clustering: reg_covar must be a number >= 0, got {reg_covar!r}")
    criterion = section.get("criterion", "bic")
    if criterion not in CRITERIA:
        raise ValueError(f"soft_clustering: criterion must be one of {list(CRITERIA)}, got {criterion!r}")
    for key in ("baseline", "memberships"):
        if not isinstance(section.get(key, False), bool):
            raise ValueError(f"soft_clustering: {key} must be true or false, got {section[key]!r}")
    top = section.get("top", 3)
    if not whole(top) or not 1 <= top <= _hip.PREDICT_MAX_TOP:
        raise ValueError(f"soft_clustering: top must be an integer in 1..{_hip.PREDICT_MAX_TOP}, got {top!r}")
    if labels is not None and not labels.is_file():
        raise FileNotFoundError(f"soft_clustering: the labels file {str(labels)!r} is missing")
    return {"clusters": clusters, "labels": labels, "restarts": restarts, "seed": seed, "max_iter": max_iter,
            "tol": float(tol), "reg_covar": float(reg_covar), "criterion": criterion,
            "baseline": bool(section.get("baseline", False)), "memberships": bool(section.get("memberships", False)),
            "top": top}


def write_memberships_tsv(path, ids: Sequence[str], components: np.ndarray, probs: np.ndarray) -> int:
    """``id<TAB>component<TAB>prob[<TAB>component<TAB>prob]...`` per row, best first, probabilities as ``repr`` of the
    float; slots without a component (-1) are left out.  Returns the number of lines."""
    with open(path, "w") as io:
        for vid, cs, ps in zip(ids, components.tolist(), probs.tolist()):
            io.write("\t".join([str(vid)] + [f"{c}\t{float(q)!r}" for c, q in zip(cs, ps) if c >= 0]) + "\n")
    return len(ids)


def write_report(output_root, report: dict) -> Path:
    out = Path(output_root) / "mixture_metrics.json"
    with open(out, "w") as io:
        json.dump(report, io, indent=1)
        io.write("\n")
    return out


def run_section(cfg: dict, graph, output_root) -> Tuple[MixtureModel, dict]:
    """What the CLI does for a checked ``soft_clustering`` section after ``Z.npy``: fit the embeddings (and, with
    ``baseline``, the content), write ``mixture_model.npz`` and, with ``memberships``, ``memberships.tsv`` (every vertex
    in vertex order under the model of "Z" -- with ``labels`` the vertices the fit did not see as well); returns
    (the model of "Z", the report that becomes ``mixture_metrics.json`` -- the caller adds the arrivals' count and writes
    it)."""
    output_root = Path(output_root)
    kw = {key: cfg[key] for key in ("restarts", "seed", "max_iter", "tol", "reg_covar", "criterion")}
    kw.update(k=cfg["clusters"], labels=cfg["labels"], return_memberships=True)
    tables = {"Z": graph.soft_cluster(table="Z", **kw)}
    if cfg["baseline"]:
        tables["X"] = graph.soft_cluster(table="X", **kw)
    first = tables["Z"]
    model = first["model"]
    model.save(output_root / "mixture_model.npz")
    if cfg["memberships"]:                              # EVERY vertex, in vertex order: the model's E-step on the table
        comp, prob = model.predict(graph.engine(), top=cfg["top"])
        write_memberships_tsv(output_root / "memberships.tsv", graph.vertex_ids, comp, prob)
    hidden = ("vertices", "assignments", "memberships", "model", "class_names", "table", "clustered", "restarts", "seed")
    report = {"labels": None if cfg["labels"] is None else str(cfg["labels"]), "clustered": first["clustered"],
              "class_names": first.get("class_names"), "clusters": first["clusters"], "restarts": first["restarts"],
              "seed": first["seed"], "criterion": cfg["criterion"],
              "tables": {name: {key: v for key, v in t.items() if key not in hidden} for name, t in tables.items()}}
    return model, report
