#!/usr/bin/env python3
"""Times the label probe (csrc/label_probe.h, clane_amd/classify.py) on one MI355X, beside the same pass in torch.

    python tools/label_probe_time.py [--shapes config2 config3] [--repeats 5] [--table-runs 10] > profiles/r10_label_probe.md

Per shape (config 2: 200k x 128, config 3: 2M x 256; C = 7, F = 90, fp32), medians of `--repeats` interleaved repeats:
  * one forward + grad pass of the fused kernels (clane_probe_forward_f32 with G, clane_probe_grad_f32),
  * the same pass in torch with all 90 fits at once (Z[rows] @ W.T, log_softmax, G.T @ Z) and fit by fit,
  * the whole 9 x `--table-runs` table of LabelProbe.evaluate on planted labels.
The pass is 4 n d K FLOP (K = F * Cp = 720); clane_project_rows_f32 runs at 104.8 TF/s.
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
from clane_amd.classify import LabelProbe, make_splits      # noqa: E402
from clane_amd.engine import SweepEngine                    # noqa: E402
from clane_amd.partition import HostCSR                     # noqa: E402

SHAPES = {"config2": (200_000, 128), "config3": (2_000_000, 256), "small": (20_000, 64)}
C, RATIOS = 7, (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)


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
    args = ap.parse_args()
    dev = _hip.require_gpu("cuda:0")
    k = _hip.kernels()
    print("# Label probe: one forward + grad pass and the whole F1 table\n")
    print(f"{torch.cuda.get_device_name(dev)}, fp32, C = {C}, Cp = 8, medians of {args.repeats} interleaved repeats.\n")
    for name in args.shapes:
        n, d = SHAPES[name]
        F = len(RATIOS) * args.table_runs
        Cp = _hip.probe_padded_classes(C)
        K = F * Cp
        rng = np.random.default_rng(0)
        y_np = rng.integers(0, C, n)
        X = torch.from_numpy((rng.standard_normal((C, d), dtype=np.float32)[y_np] * 0.3)) + torch.randn(n, d)
        csr = HostCSR(n, np.arange(n + 1, dtype=np.int64), ((np.arange(n) + 1) % n).astype(np.int32))
        with torch.cuda.device(dev):
            eng = SweepEngine(csr, X, dev)
            del X
            Z = eng.Zcur
            rows = eng.pos.to(torch.int32).contiguous()
            y = torch.from_numpy(y_np).to(dev, torch.int32)
            split, _ = make_splits(n, RATIOS, args.table_runs, 0)
            split = split.to(dev)
            W = torch.randn(K, d, device=dev) * 0.05
            bias = torch.zeros(K, device=dev)
            G = torch.empty(n * K, device=dev)
            loss = torch.zeros(F, dtype=torch.float64, device=dev)
            loss_ws = torch.empty(k.probe_loss_ws_len(n, F), dtype=torch.float64, device=dev)
            grad_ws = torch.empty(k.probe_grad_ws_len(n, K, d), device=dev)
            dW, db = torch.empty(K * d, device=dev), torch.empty(K, device=dev)

            def fused_forward():
                k.probe_forward(Z, d, rows, y, split, W, bias, F, C, loss_ws, loss, G=G)

            def fused_grad():
                k.probe_grad(Z, d, rows, G, grad_ws, dW, db)

            yl, rl = y.long(), rows.long()
            real = (torch.arange(K, device=dev) % Cp) < C

            def torch_batched():
                Zg = Z[rl, :d]
                logits = (Zg @ W.T + bias).view(n, F, Cp)
                logits[:, :, C:] = float("-inf")
                logp = torch.log_softmax(logits, 2)
                g = logp.exp()
                g[torch.arange(n, device=dev), :, yl] -= 1.0
                g *= (split != 0)[:, :, None]
                g = g.view(n, K)
                return g.T @ Zg, g.sum(0), real

            def torch_per_fit():
                for f in range(F):
                    Zg = Z[rl, :d]
                    logp = torch.log_softmax(Zg @ W[f * Cp:f * Cp + C].T + bias[f * Cp:f * Cp + C], 1)
                    g = logp.exp()
                    g[torch.arange(n, device=dev), yl] -= 1.0
                    g *= (split[:, f] != 0)[:, None]
                    g.T @ Zg, g.sum(0)

            runs = {"fused forward": fused_forward, "fused grad": fused_grad, "torch, 90 fits at once": torch_batched,
                    "torch, fit by fit": torch_per_fit}
            for fn in runs.values():
                fn()                                            # warm-up
            times = {key: [] for key in runs}
            for _ in range(args.repeats):                       # interleaved
                for key, fn in runs.items():
                    times[key].append(timed(fn))
            med = {key: statistics.median(v) for key, v in times.items()}
            flop = 4.0 * n * d * K
            fused = med["fused forward"] + med["fused grad"]
            print(f"## {name}: n = {n}, d = {d}, F = {F}, K = {K}\n")
            print("| pass | ms | TF/s (4 n d K) |\n|---|---|---|")
            print(f"| fused forward + grad | {fused:.3f} | {flop / fused / 1e9:.1f} |")
            for key in runs:
                share = flop / 2 if key.startswith("fused") else flop
                print(f"| {key} | {med[key]:.3f} | {share / med[key] / 1e9:.1f} |")
            print(f"\nclane_project_rows_f32: 104.8 TF/s.  Fused / torch batched = {fused / med['torch, 90 fits at once']:.2f}.\n")
            del G, grad_ws
            torch.cuda.empty_cache()
            probe = LabelProbe(eng)
            table = []
            for _ in range(max(1, args.repeats // 2)):
                table.append(timed(lambda: probe.evaluate(torch.arange(n), y_np.tolist(), C, RATIOS, args.table_runs, 0)))
            out = probe.evaluate(torch.arange(n), y_np.tolist(), C, RATIOS, args.table_runs, 0)
            its = out["fits"]["iterations"]
            print(f"Whole 9 x {args.table_runs} table: {statistics.median(table) / 1e3:.2f} s "
                  f"(L-BFGS steps per fit {min(its)}..{max(its)}, converged {sum(out['fits']['converged'])} / {F}, "
                  f"kernel passes {probe.passes}).  micro-F1 at 10 % / 90 %: {out['rows'][0]['micro_f1']:.3f} / "
                  f"{out['rows'][-1]['micro_f1']:.3f}.\n", flush=True)
            del eng, Z, probe
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
