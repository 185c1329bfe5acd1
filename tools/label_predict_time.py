#!/usr/bin/env python3
"""Times label prediction (csrc/label_predict.h, clane_amd/classify.py) on one MI355X, beside the fit kernel's forward.

    python tools/label_predict_time.py [--shapes f32_c7 f32_c64 bf16_c40] [--repeats 7] [--end-to-end] > profiles/r20_label_predict.md

Per shape (n = 2 097 152, d = 256, fp32 at C = 7 and C = 64; n = 10 485 760, d = 128, bf16 at C = 40; F = 1), in one
process, after a warm-up of every call, medians of `--repeats` interleaved repeats timed with device events:
  * probe_predict with top = 3, no proba,
  * the same with proba,
  * probe_forward with CLANE_PROBE_WRITE_PRED only on the same operands -- the yardstick: the same contraction, the
    arg-max in place of the probabilities and the selection rounds.
The rows are a random permutation of the table (every operand row is a gather).  The contraction is 2 n d Cp FLOP.
`--end-to-end`: LabelProbe.train with l2 = [0.01, 0.1, 1, 10] (5 folds) on a tenth of the vertices of the config-3 shape
(2 000 000 x 256, fp32, C = 7, planted classes) and the prediction of the others, timed with a host clock around a
device synchronise.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from clane_amd import _hip                                  # noqa: E402
from clane_amd.classify import LabelProbe                   # noqa: E402
from clane_amd.engine import SweepEngine                    # noqa: E402
from clane_amd.partition import HostCSR                     # noqa: E402

SHAPES = {"f32_c7": (2_097_152, 256, torch.float32, 7), "f32_c64": (2_097_152, 256, torch.float32, 64),
          "bf16_c40": (10_485_760, 128, torch.bfloat16, 40), "small": (20_000, 64, torch.float32, 7)}
TOP = 3


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_times(k, dev, name, repeats):
    n, d, dtype, C = SHAPES[name]
    Cp = _hip.probe_padded_classes(C)
    acc = _hip.acc_dtype(dtype)
    g = torch.Generator(device=dev).manual_seed(0)
    Z = torch.randn(n, d, device=dev, generator=g).to(dtype)
    rows = torch.randperm(n, device=dev, generator=g).to(torch.int32)
    W = (torch.randn(Cp, d, device=dev, generator=g) * (1.0 / d ** 0.5)).to(acc)
    bias = torch.randn(Cp, device=dev, generator=g).to(acc)
    y = torch.zeros(n, dtype=torch.int32, device=dev)
    split = torch.ones(n, 1, dtype=torch.uint8, device=dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    loss_ws = torch.empty(k.probe_loss_ws_len(n, 1), dtype=torch.float64, device=dev)
    pred = torch.empty(n, 1, dtype=torch.int32, device=dev)
    cls = torch.empty(n, 1, TOP, dtype=torch.int32, device=dev)
    pr = torch.empty(n, 1, TOP, dtype=acc, device=dev)
    full = torch.empty(n, 1, C, dtype=acc, device=dev)
    runs = {
        f"probe_predict, top = {TOP}": lambda: k.probe_predict(Z, d, rows, W, bias, 1, C, cls, pr),
        f"probe_predict, top = {TOP}, proba": lambda: k.probe_predict(Z, d, rows, W, bias, 1, C, cls, pr, proba=full),
        "probe_forward, pred only (the yardstick)": lambda: k.probe_forward(Z, d, rows, y, split, W, bias, 1, C, loss_ws,
                                                                             loss, pred=pred),
    }
    for fn in runs.values():                                # warm-up: code objects, every shape of the timed window
        fn()
        fn()
    torch.cuda.synchronize()
    times = {key: [] for key in runs}
    for _ in range(repeats):                                # interleaved
        for key, fn in runs.items():
            times[key].append(event_ms(fn))
    assert torch.equal(cls[:, :, 0], pred)                  # the same arg-max from both kernels
    med = {key: statistics.median(v) for key, v in times.items()}
    keys = list(runs)
    flop = 2.0 * n * d * Cp
    print(f"## {name}: n = {n}, d = {d}, {str(dtype).split('.')[-1]}, F = 1, C = {C} (Cp = {Cp})\n")
    print("| call | ms (median) | min .. max | contraction, TFLOP/s |\n|---|---|---|---|")
    for key in keys:
        print(f"| {key} | {med[key]:.3f} | {min(times[key]):.3f} .. {max(times[key]):.3f} | {flop / med[key] / 1e9:.1f} |")
    print(f"\nprobe_predict / probe_forward = {med[keys[0]] / med[keys[2]]:.3f} without proba, "
          f"{med[keys[1]] / med[keys[2]]:.3f} with.\n", flush=True)


def end_to_end(dev):
    n, d, C = 2_000_000, 256, 7
    rng = np.random.default_rng(0)
    y_np = rng.integers(0, C, n)
    X = torch.from_numpy((rng.standard_normal((C, d), dtype=np.float32)[y_np] * 0.3)) + torch.randn(n, d)
    csr = HostCSR(n, np.arange(n + 1, dtype=np.int64), ((np.arange(n) + 1) % n).astype(np.int32))
    with torch.cuda.device(dev):
        eng = SweepEngine(csr, X, dev)
        del X
        labelled = np.sort(rng.choice(n, n // 10, replace=False))
        others = np.setdiff1d(np.arange(n), labelled)
        probe = LabelProbe(eng)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model = probe.train(labelled, y_np[labelled], C, l2=[0.01, 0.1, 1.0, 10.0], folds=5, seed=0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        classes, probs = model.predict_table(eng, others, top=3)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
    acc = float((classes[:, 0] == y_np[others]).mean())
    print(f"## End to end: config-3 shape, n = {n}, d = {d}, fp32, C = {C}, {len(labelled)} labelled\n")
    print(f"train (20 cross-validation fits at once, then the final fit): {t1 - t0:.2f} s; l2 chosen {model.l2}, final fit "
          f"{model.iterations} L-BFGS steps, converged {model.converged}.")
    print(f"predict_table of the other {len(others)} vertices, top = 3, host arrays included: {t2 - t1:.2f} s; top-1 "
          f"accuracy on them {acc:.3f}.")
    print("cv: " + "; ".join(f"l2 {r['l2']}: log-loss {r['log_loss']:.4f}, accuracy {r['accuracy']:.3f}, ece {r['ece']:.4f}"
                             for r in model.cv["rows"]) + "\n", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["f32_c7", "f32_c64", "bf16_c40"], choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--end-to-end", action="store_true")
    args = ap.parse_args()
    dev = _hip.require_gpu("cuda:0")
    k = _hip.kernels()
    print("# Label prediction: probe_predict beside probe_forward\n")
    print(f"{torch.cuda.get_device_name(dev)}, medians of {args.repeats} interleaved repeats after a warm-up, device events "
          f"around each call, one process.\n")
    with torch.cuda.device(dev):
        for name in args.shapes:
            kernel_times(k, dev, name, args.repeats)
            torch.cuda.empty_cache()
    if args.end_to_end:
        end_to_end(dev)


if __name__ == "__main__":
    main()
