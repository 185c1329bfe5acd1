#!/usr/bin/env python3
"""Times the multi-label probe (csrc/multilabel_probe.h, LabelProbe.fit_multilabel) on one MI355X, beside the soft-max
pass at the same K and the same pass in torch.  The sibling of tools/label_probe_time.py.

    python tools/multilabel_probe_time.py [--shapes config2 config3] [--repeats 5] [--table-runs 10] [--no-table]
        > profiles/r12_multilabel_probe.md

Per shape (config 2: 200k x 128, config 3: 2M x 256; C = 39 -- BlogCatalog's class count --, Cp = 64, F = 9 x
`--table-runs`, fp32), medians of `--repeats` interleaved repeats on a synchronised step:
  * one forward + grad pass: clane_probe_forward_ovr_f32 with G, clane_probe_grad_f32,
  * the soft-max forward (clane_probe_forward_f32 with G) + the same grad pass at the same K -- the ratio is recorded,
    not asserted,
  * the same pass in torch (Z[rows] @ W.T, binary_cross_entropy_with_logits, G.T @ Z[rows]), a group of fits at a time,
  * the prediction pass (top-k masks, no G), and unless --no-table the whole table of LabelProbe.evaluate(multilabel=True).
A shape whose G [n, F Cp] would exceed --g-bytes is timed on the first fits that fit into it (the probe itself groups
the fits in the same way)."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from clane_amd import _hip                                  # noqa: E402
from clane_amd.classify import LabelProbe, column_states, make_splits      # noqa: E402
from clane_amd.engine import SweepEngine                    # noqa: E402
from clane_amd.partition import HostCSR                     # noqa: E402

SHAPES = {"config2": (200_000, 128), "config3": (2_000_000, 256), "small": (20_000, 64)}
C, RATIOS = 39, (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["config2", "config3"], choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--table-runs", type=int, default=10)
    ap.add_argument("--g-bytes", type=int, default=8 << 30)
    ap.add_argument("--no-table", action="store_true")
    args = ap.parse_args()
    dev = _hip.require_gpu("cuda:0")
    k = _hip.kernels()
    Cp = _hip.ovr_padded_classes(C)
    print("# Multi-label probe: one forward + grad pass, the prediction pass and the whole F1 table\n")
    print(f"{torch.cuda.get_device_name(dev)}, fp32, C = {C}, Cp = {Cp}, medians of {args.repeats} interleaved repeats.\n")
    for name in args.shapes:
        n, d = SHAPES[name]
        F_all = len(RATIOS) * args.table_runs
        F = max(1, min(F_all, args.g_bytes // (n * Cp * 4)))
        K = F * Cp
        rng = np.random.default_rng(0)
        freq = 1.0 / (1.0 + np.arange(C))
        Y_np = rng.random((n, C)) < (1.4 * freq / freq.sum())[None, :]          # about 1.4 classes per vertex
        Y_np[np.arange(n), rng.integers(0, C, n)] |= ~Y_np.any(1)               # at least one
        X = torch.from_numpy((Y_np.astype(np.float32) @ rng.standard_normal((C, d), dtype=np.float32)) * 0.3) + torch.randn(n, d)
        masks = torch.from_numpy((Y_np.astype(np.int64) << np.arange(C)).sum(1))
        csr = HostCSR(n, np.arange(n + 1, dtype=np.int64), ((np.arange(n) + 1) % n).astype(np.int32))
        with torch.cuda.device(dev):
            eng = SweepEngine(csr, X, dev)
            del X
            Z = eng.Zcur
            rows = eng.pos.to(torch.int32).contiguous()
            ymask = masks.to(dev)
            y = torch.from_numpy(Y_np.argmax(1)).to(dev, torch.int32)           # the soft-max pass needs one class per row
            split_all, _ = make_splits(n, RATIOS, args.table_runs, 0)
            split = split_all[:, :F].contiguous().to(dev)
            state = torch.zeros(F, Cp, dtype=torch.int8, device=dev)
            state[:, :C] = column_states(ymask, split, C)
            state = state.view(-1)
            max_labels = int(Y_np.sum(1).max())
            W = torch.randn(K, d, device=dev) * 0.05
            bias = torch.zeros(K, device=dev)
            G = torch.empty(n * K, device=dev)
            loss = torch.zeros(F, dtype=torch.float64, device=dev)
            loss_ws = torch.empty(k.probe_loss_ws_len(n, F), dtype=torch.float64, device=dev)
            grad_ws = torch.empty(k.probe_grad_ws_len(n, K, d), device=dev)
            dW, db = torch.empty(K * d, device=dev), torch.empty(K, device=dev)
            pred = torch.zeros(n, F, dtype=torch.int64, device=dev)
            rl = rows.long()
            Yd = torch.from_numpy(Y_np).to(dev)

            def ovr_forward():
                k.probe_forward_ovr(Z, d, rows, ymask, split, W, bias, state, F, C, max_labels, loss_ws, loss, G=G)

            def ovr_predict():
                k.probe_forward_ovr(Z, d, rows, ymask, split, W, bias, state, F, C, max_labels, loss_ws, loss, pred=pred)

            def softmax_forward():
                k.probe_forward(Z, d, rows, y, split, W, bias, F, C, loss_ws, loss, G=G)

            def grad():
                k.probe_grad(Z, d, rows, G, grad_ws, dW, db)

            def torch_pass(group=8):
                Zg = Z[rl, :d]
                for a in range(0, F, group):
                    b = min(F, a + group)
                    logits = (Zg @ W[a * Cp:b * Cp].T + bias[a * Cp:b * Cp]).view(n, b - a, Cp)[:, :, :C]
                    target = Yd[:, None, :].expand(n, b - a, C).float()
                    live = (split[:, a:b] != 0)[:, :, None]
                    torch.nn.functional.binary_cross_entropy_with_logits(logits, target, reduction="none").mul_(live).sum((0, 2))
                    g = ((torch.sigmoid(logits) - target) * live).reshape(n, -1)
                    g.T @ Zg, g.sum(0)

            runs = {"one-vs-rest forward": ovr_forward, "grad": grad, "soft-max forward": softmax_forward,
                    "one-vs-rest prediction (top-k)": ovr_predict, "torch, 8 fits at a time": torch_pass}
            for fn in runs.values():
                fn()                                            # warm-up
            times = {key: [] for key in runs}
            for _ in range(args.repeats):                       # interleaved
                for key, fn in runs.items():
                    times[key].append(timed(fn))
            med = {key: statistics.median(v) for key, v in times.items()}
            flop = 4.0 * n * d * K
            fused = med["one-vs-rest forward"] + med["grad"]
            soft = med["soft-max forward"] + med["grad"]
            print(f"## {name}: n = {n}, d = {d}, F = {F} of {F_all}, K = {K}, max_labels = {max_labels}\n")
            print("| pass | ms | TF/s |\n|---|---|---|")
            print(f"| one-vs-rest forward + grad | {fused:.3f} | {flop / fused / 1e9:.1f} |")
            print(f"| soft-max forward + grad | {soft:.3f} | {flop / soft / 1e9:.1f} |")
            for key in runs:
                share = flop if key.startswith("torch") else flop / 2
                print(f"| {key} | {med[key]:.3f} | {share / med[key] / 1e9:.1f} |")
            print(f"\nOne-vs-rest / soft-max (forward + grad) = {fused / soft:.3f}; forward alone = "
                  f"{med['one-vs-rest forward'] / med['soft-max forward']:.3f}.  One-vs-rest / torch = "
                  f"{fused / med['torch, 8 fits at a time']:.3f}.\n", flush=True)
            del G, grad_ws, pred, Yd
            torch.cuda.empty_cache()
            if not args.no_table:
                probe = LabelProbe(eng)
                t = timed(lambda: probe.evaluate(torch.arange(n), masks, C, RATIOS, args.table_runs, 0, multilabel=True))
                out = probe.evaluate(torch.arange(n), masks, C, RATIOS, args.table_runs, 0, multilabel=True)
                its = out["fits"]["iterations"]
                print(f"Whole 9 x {args.table_runs} table: {t / 1e3:.2f} s (L-BFGS steps per fit {min(its)}..{max(its)}, "
                      f"converged {sum(out['fits']['converged'])} / {F_all}, constant columns {out['constant_columns']}, "
                      f"kernel passes {probe.passes}).  micro-F1 at 10 % / 90 %: {out['rows'][0]['micro_f1']:.3f} / "
                      f"{out['rows'][-1]['micro_f1']:.3f}.\n", flush=True)
                del probe
            del eng, Z
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
