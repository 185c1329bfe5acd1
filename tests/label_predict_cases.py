"""Shared by the host and the GPU tests of label prediction: probe_predict of csrc/label_predict.h restated in torch as a
subclass of the existing kernel doubles, the selection rule on its own, and the inputs of the kernel cases."""
import numpy as np
import torch

from clane_amd import _hip

from .test_multilabel_host import MultilabelOracleKernels
from .test_new_vertices_host import InductOracleKernels


def select_top(val: torch.Tensor, p: torch.Tensor, top: int):
    """(classes [n, top] int32, probs [n, top]) from values and probabilities [n, C]: the ``top`` columns of highest
    value, best first, ties to the lowest class, a NaN or -inf value never; -1 / 0 where nothing is left."""
    n, C = val.shape
    ok = val > float("-inf")                                        # False for NaN
    key = torch.where(ok, val, torch.full_like(val, float("-inf")))
    order = torch.sort(key, dim=1, descending=True, stable=True).indices       # stable: equal values keep class order
    order = torch.cat([order, torch.zeros(n, max(0, top - C), dtype=order.dtype)], 1)[:, :top]
    taken = torch.gather(ok, 1, order) & (torch.arange(top)[None, :] < C)
    classes = torch.where(taken, order, torch.full_like(order, -1)).to(torch.int32)
    probs = torch.where(taken, torch.gather(p, 1, order), torch.zeros(n, top, dtype=p.dtype))
    return classes, probs


def values_and_probabilities(logits: torch.Tensor, sigmoid: bool, state=None):
    """(val, p) [n, C] of one model from its logits, by the formulas of the kernel's header comment."""
    if not sigmoid:
        return logits, torch.softmax(logits, 1)
    inf = torch.full_like(logits, float("inf"))
    fitted, low = (state == 0)[None, :], (state < 0)[None, :]
    p = torch.where(fitted, torch.sigmoid(logits), torch.where(low, torch.zeros_like(logits), torch.ones_like(logits)))
    return torch.where(fitted, logits, torch.where(low, -inf, inf)), p


class PredictOracleKernels(MultilabelOracleKernels, InductOracleKernels):
    """The doubles of both probes and of the new-vertex calls, plus probe_predict (the same formulas, no attempt at the
    same rounding)."""

    def probe_predict(self, Z, d, rows, W, bias, F, C_, top_class, top_prob, proba=None, sigmoid=False, col_state=None):
        Cp = _hip.ovr_padded_classes(C_) if sigmoid else _hip.probe_padded_classes(C_)
        assert 1 <= top_class.shape[2] <= 8 and top_class.shape == top_prob.shape
        Zg = self._gathered(Z, d, rows, W.dtype)
        for f in range(F):                                  # fit by fit: a fit gets the same bits whatever shares the call
            logits = Zg @ W[f * Cp:f * Cp + C_].T + bias[f * Cp:f * Cp + C_]
            val, p = values_and_probabilities(logits, sigmoid, col_state[f * Cp:f * Cp + C_] if sigmoid else None)
            top_class[:, f], top_prob[:, f] = select_top(val, p, top_class.shape[2])
            if proba is not None:
                proba[:, f] = p


def planted(n, d, C, sep, seed, noise=0.0):
    """Rows around C class centres at distance ``sep``; a share ``noise`` of the labels is redrawn at random."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, n)
    y[:C] = np.arange(C)
    X = rng.standard_normal((C, d))[y] * sep + rng.standard_normal((n, d))
    flip = rng.random(n) < noise
    y = np.where(flip, rng.integers(0, C, n), y)
    return torch.from_numpy(X), torch.from_numpy(y)


# ---- the kernel cases of the GPU suite ------------------------------------------------------------------------------
# (n, d, C, F, top, dtype name, sigmoid, seed).  Between them: n in {1, 127, 129, 5000}; d in {1, 5, 16, 130, 256}; C in
# {2, 3, 7, 17, 64} (Cp = 2, 4, 8, 32, 64: every branch of probe_fit_reduce) plus 16; F in {1, 3, 19} (F = 19 at Cp = 8
# and 16 crosses the 128-column workgroup tile); top in {1, 3, 8} with top > C; the three dtypes; both modes.  The seed is
# the first for which the float64 reference alone (clear_rows below, on the CPU) leaves out at most 1 % of the (row, fit)
# pairs of the case from the class comparison; what it leaves out is recorded beside it.
KERNEL_CASES = [
    # n, d, C, F, top, dtype, sigmoid, seed      left out of the class comparison (rows x fits)
    (1, 1, 2, 1, 1, "f32", False, 0),          # 0 of 1
    (127, 5, 3, 3, 3, "f32", False, 0),        # 0 of 381
    (129, 16, 7, 19, 3, "f32", False, 0),      # 0 of 2451
    (129, 130, 17, 3, 8, "f32", False, 1),     # 2 of 387 (seed 0: 6)
    (5000, 256, 64, 1, 3, "f32", False, 0),    # 32 of 5000
    (127, 16, 2, 19, 8, "f64", False, 0),      # 0 of 2413
    (129, 130, 7, 3, 1, "f64", False, 0),      # 0 of 387
    (5000, 5, 16, 19, 3, "f64", True, 0),      # 0 of 95000
    (129, 256, 17, 1, 3, "bf16", False, 1),    # 0 of 129 (seed 0: 2)
    (127, 130, 3, 19, 8, "bf16", True, 0),     # 0 of 2413
    (1, 5, 64, 3, 8, "bf16", False, 0),        # 0 of 3
    (129, 1, 7, 1, 3, "f32", True, 0),         # 0 of 129
]
DTYPES = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}


def kernel_case(n, d, C, F, top, dtype, sigmoid, seed, integer=False):
    """The operands of one case, on the CPU: a table with a padded leading dimension, repeated rows and one index past the
    table (a zero row), as ``_forward_case`` of tests/test_gpu_classify.py builds them.  ``integer``: Z in {-2..2}, W and
    bias in {-1, 0, 1} -- every logit exact in every dtype at these sizes -- and one all-zero row of Z."""
    g = torch.Generator().manual_seed(1000 * seed + n + 7 * d + 13 * C + F)
    T = DTYPES[dtype]
    acc = _hip.acc_dtype(T)
    V, ld = max(4, n // 2 + 3), d + 3
    Cp = _hip.ovr_padded_classes(C) if sigmoid else _hip.probe_padded_classes(C)
    if integer:
        table = torch.randint(-2, 3, (V, ld), generator=g).to(T)
        table[1] = 0
        W = torch.randint(-1, 2, (F, Cp, d), generator=g).to(acc)
        bias = torch.randint(-1, 2, (F, Cp), generator=g).to(acc)
    else:
        table = torch.randn(V, ld, generator=g, dtype=torch.float64).to(T)
        W = (torch.randn(F, Cp, d, generator=g, dtype=torch.float64) * (0.5 / d ** 0.5)).to(acc)
        bias = (2.0 * torch.randn(F, Cp, generator=g, dtype=torch.float64)).to(acc)
    rows = torch.randint(0, V, (n,), generator=g).to(torch.int32)
    if n > 2:
        rows[n // 2] = V                                    # one index past the table: a zero row
        rows[-1] = rows[0]                                  # a repeated row
    if integer and n > 1:
        rows[1] = 1                                         # the zero row of the table: every logit is the bias
    state = torch.zeros(F, Cp, dtype=torch.int8)
    if sigmoid:
        state[:, :C] = torch.randint(-1, 2, (F, C), generator=g).to(torch.int8) * (torch.rand(F, C, generator=g) < 0.3)
    return {"table": table, "Z": table[:, :d], "rows": rows, "W": W.view(F * Cp, d), "bias": bias.view(-1),
            "state": state.view(-1), "Cp": Cp, "acc": acc}


def reference64(case, n, d, C, F, sigmoid):
    """(logits, bound b, val, p) [n, F, C] in float64 from the values the kernel reads; b = 2 d eps (|Z| |W|^T + |bias|), eps
    the unit roundoff of the accumulate type (2^-24 / 2^-53), as in tests/test_gpu_classify.py."""
    Cp, acc = case["Cp"], case["acc"]
    r = case["rows"].long()
    inside = (r >= 0) & (r < case["table"].shape[0])
    Zg = case["table"][r.clamp(0, case["table"].shape[0] - 1), :d].double() * inside[:, None].double()
    W = case["W"].double().view(F, Cp, d)[:, :C]
    b = case["bias"].double().view(F, Cp)[:, :C]
    logits = torch.einsum("nd,fcd->nfc", Zg, W) + b
    bound = 2.0 * d * (0.5 * torch.finfo(acc).eps) * (torch.einsum("nd,fcd->nfc", Zg.abs(), W.abs()) + b.abs())
    state = case["state"].view(F, Cp)[:, :C]
    val, p = torch.empty_like(logits), torch.empty_like(logits)
    for f in range(F):
        val[:, f], p[:, f] = values_and_probabilities(logits[:, f], sigmoid, state[f] if sigmoid else None)
    return logits, bound, val, p


def clear_rows(val, bound, top):
    """bool [n, F]: rows whose reference top-(top + 1) values are pairwise more than 4 max_c b apart (+-inf values of
    constant columns are apart from everything but each other)."""
    n, F, C = val.shape
    m = min(top + 1, C)
    head = torch.sort(val, dim=2, descending=True).values[:, :, :m]
    gap = head[:, :, :-1] - head[:, :, 1:] if m > 1 else torch.full((n, F, 1), float("inf"), dtype=val.dtype)
    # inf - inf: two constant columns of one kind.  Their order is exact (the lowest class first; -inf is never chosen)
    gap = torch.nan_to_num(gap, nan=float("inf"), posinf=float("inf"))
    return (gap > 4.0 * bound.amax(2, keepdim=True)).all(2)
