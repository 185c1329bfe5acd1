#!/usr/bin/env python3
"""Time one training step of the bilinear similarity: (a) the HIP step (SimilarityTrainer.step: pair_project, pair_loss,
pair_grad, adam_step) against (b) the torch step that was the only way before -- Z[src], Z[dst] by torch indexing on the
device, AsymmertricSimilarity.forward, the reference's loss lines (embedder.py:276-283), backward and
torch.optim.Adam.step, including its `mask.any()` host read.

Shapes: 2M table rows, d = 256 fp32 (configs 2 / 3) and d = 128 bf16 (config 4), B in {4, 4096, 262144}.  Warm-up, then
the two variants alternate for several repeats; the median of the per-repeat means is reported (wall clock around a
device synchronisation, so launch overhead and the host read count).  For B = 262144 the TF/s of forward (4 B d^2 flop)
and backward (4 B d^2 flop) of the HIP step come from HIP events around those two calls.
Per-kernel times: run this script under `rocprofv3 --kernel-trace --stats -- python tools/train_step_time.py --hip-only`.

Usage: python tools/train_step_time.py [--out profiles/r07_train_step.jsonl] [--rows 2000000] [--hip-only]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from clane_amd import _hip                                   # noqa: E402
from clane_amd.similarity import AsymmertricSimilarity       # noqa: E402
from clane_amd.train import SimilarityTrainer                # noqa: E402


class _Table:
    """The little of a SweepEngine that SimilarityTrainer reads: a table and its description."""

    def __init__(self, rows, d, dtype, dev):
        self.k, self.device, self.dtype, self.acc_dtype = _hip.kernels(), dev, dtype, _hip.acc_dtype(dtype)
        self.d, self.world, self.columns, self.halo, self.exchange = d, 1, False, False, "none"
        self.Zcur = torch.randn(rows, d, device=dev, dtype=torch.float32).to(dtype)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true")
    args = ap.parse_args()
    dev = _hip.require_gpu("cuda:0")
    records = []
    for name, d, dtype in (("config2/3 d=256 fp32", 256, torch.float32), ("config4 d=128 bf16", 128, torch.bfloat16)):
        eng = _Table(args.rows, d, dtype, dev)
        torch.manual_seed(0)
        sim = AsymmertricSimilarity(d).to(dev)
        for B in (4, 4096, 262_144):
            gen = torch.Generator(device=dev).manual_seed(B)
            src = torch.randint(0, args.rows, (B,), generator=gen, device=dev, dtype=torch.int32)
            dst = torch.randint(0, args.rows, (B,), generator=gen, device=dev, dtype=torch.int32)
            linked = (torch.rand(B, generator=gen, device=dev) < 0.5).to(torch.uint8)
            u = torch.rand(B, generator=gen, device=dev, dtype=eng.acc_dtype)
            tr = SimilarityTrainer(eng, sim.stacked_weight(eng.acc_dtype, dev), 1e-4, B)
            opt = torch.optim.Adam(sim.parameters(), lr=1e-4)
            srcl, dstl, lk = src.long(), dst.long(), linked.bool()

            def hip_step():
                tr.step(src, dst, linked, u)

            def torch_step():
                opt.zero_grad()
                prob = sim(eng.Zcur[srcl].float(), eng.Zcur[dstl].float()).sigmoid()
                loss = prob.where(lk, 1 - prob).add(1e-10).log().neg()
                mask = lk.logical_xor(u < prob)
                if ~mask.any():
                    return
                loss.masked_select(mask).mean().backward()
                opt.step()

            n = 200 if B <= 4096 else 10

            def timed(fn):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                torch.cuda.synchronize(dev)
                return (time.perf_counter() - t0) / n * 1e3

            variants = [("hip", hip_step)] + ([] if args.hip_only else [("torch", torch_step)])
            for _, fn in variants:                       # warm-up
                for _ in range(3):
                    fn()
            ms = {v: [] for v, _ in variants}
            for _ in range(args.repeats):                # alternate the variants
                for v, fn in variants:
                    ms[v].append(timed(fn))
            rec = {"shape": name, "rows": args.rows, "d": d, "dtype": str(dtype), "B": B, "steps_per_timing": n,
                   "repeats": args.repeats}
            for v in ms:
                med = statistics.median(ms[v])
                rec[f"{v}_ms_per_step"] = med
                rec[f"{v}_steps_per_s"] = 1e3 / med
                rec[f"{v}_ms_all"] = ms[v]
            if B == 262_144:                             # forward / backward of the HIP step alone, by HIP events
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                fwd, bwd = [], []
                for _ in range(10):
                    ev[0].record()
                    tr.k.pair_project(eng.Zcur, d, src, dst, tr.W, tr.A, tr.Bm)
                    ev[1].record()
                    tr.k.pair_grad(eng.Zcur, d, src, dst, tr.A, tr.Bm, tr.g, tr.stats, tr.grad_ws, tr.dW)
                    ev[2].record()
                    torch.cuda.synchronize(dev)
                    fwd.append(ev[0].elapsed_time(ev[1]))
                    bwd.append(ev[1].elapsed_time(ev[2]))
                flop = 4.0 * B * d * d
                rec["forward_ms"], rec["backward_ms"] = statistics.median(fwd), statistics.median(bwd)
                rec["forward_tflops"] = flop / (rec["forward_ms"] * 1e-3) / 1e12
                rec["backward_tflops"] = flop / (rec["backward_ms"] * 1e-3) / 1e12
            print(json.dumps(rec), flush=True)
            records.append(rec)
        del eng
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as f:
            for r in records:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
