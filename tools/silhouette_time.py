#!/usr/bin/env python3
"""Times the silhouette's two kernels (csrc/silhouette.h) on one MI355X, beside tsne_sqdist at the same n and d.

    python tools/silhouette_time.py [--points 16384 65536] [--dims 128 256] [--clusters 8 64] [--repeats 5] \\
        > profiles/r18_silhouette.md

Per (n, d) (fp32, Gaussian blobs, K clusters of equal size; both metrics), medians of `--repeats` interleaved repeats,
timed with HIP events around the call:
  * clane_silhouette_norms_f32 and clane_silhouette_sums_f32 over all n positions in one block;
  * the fp32 MFMA rate the sums call achieves: every 128 x 128 x (d rounded up to 16) tile product it executes counts
    2 * 128 * 128 * k flops, against the 157.3 TFLOP/s fp32 peak of the matrix cores;
  * clane_tsne_sqdist_f32 at the same n and d: half the tile pairs (D is symmetric), but n^2 floats written.
No threshold is set: nobody had measured this kernel.

Every (n, d) is a child process of its own under `--step-timeout` seconds; the first that fails or runs out of time ends
the run -- nothing more is started on the card after it.
"""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
MFMA_F32_PEAK = 157.3e12
TILE = 128


def timed(torch, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def one(n: int, d: int, clusters, repeats: int) -> None:
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from clane_amd import _hip

    dev = _hip.require_gpu("cuda:0")
    k = _hip.kernels()
    rng = np.random.default_rng(0)
    f32 = torch.float32
    with torch.cuda.device(dev):
        Z = (torch.from_numpy((4.0 * rng.standard_normal((64, d)))[rng.integers(0, 64, n)].astype(np.float32))
             + torch.randn(n, d)).to(dev)
        rows = torch.randperm(n).to(torch.int32).to(dev)     # a gather: the sorted rows lie anywhere in the table
        mu = Z.double().mean(0).to(f32)
        zero = torch.zeros(d, dtype=f32, device=dev)
        nrm = {m: torch.empty(n, dtype=f32, device=dev) for m in ("euclidean", "cosine")}
        shift = {"euclidean": mu, "cosine": zero}
        runs, flops = {}, {}
        for K in clusters:
            seg = torch.tensor([n * c // K for c in range(K + 1)], dtype=torch.int64, device=dev)
            S = torch.empty(n, K, dtype=torch.float64, device=dev)
            col_tiles = sum(-(-(n * (c + 1) // K - n * c // K) // TILE) for c in range(K))
            for m in ("euclidean", "cosine"):
                key = f"sums, K = {K}, {m}"
                runs[key] = (lambda seg=seg, S=S, m=m: timed(
                    torch, lambda: k.silhouette_sums(Z, d, rows, seg, shift[m], nrm[m], m, 0, n, S)))
                flops[key] = 2.0 * TILE * TILE * (-(-d // 16) * 16) * (-(-n // TILE)) * col_tiles
        for m in ("euclidean", "cosine"):
            runs[f"norms, {m}"] = (lambda m=m: timed(torch, lambda: k.silhouette_norms(Z, d, rows, shift[m], m, nrm[m])))
        Dm = torch.empty(n, n, dtype=f32, device=dev)
        sq = torch.empty(n, dtype=f32, device=dev)
        runs["tsne_sqdist (the yardstick)"] = lambda: timed(torch, lambda: k.tsne_sqdist(Z, d, rows, mu, sq, Dm))
        tiles = -(-n // TILE)
        flops["tsne_sqdist (the yardstick)"] = 2.0 * TILE * TILE * (-(-d // 16) * 16) * tiles * (tiles + 1) / 2
        order = [key for key in runs if key.startswith("norms")] + [key for key in runs if not key.startswith("norms")]
        for key in order:
            runs[key]()                                       # warm-up; the norms first: the sums read them
        times = {key: [] for key in order}
        for _ in range(repeats):                              # interleaved
            for key in order:
                times[key].append(runs[key]())
        print(f"## n = {n}, d = {d}\n")
        print("| call | ms | tile products, TFLOP | fp32 MFMA rate | of 157.3 TFLOP/s |\n|---|---|---|---|---|")
        for key in order:
            ms = statistics.median(times[key])
            if key in flops:
                rate = flops[key] / (ms * 1e-3)
                print(f"| {key} | {ms:.3f} | {flops[key] / 1e12:.3f} | {rate / 1e12:.1f} TFLOP/s | "
                      f"{100 * rate / MFMA_F32_PEAK:.0f} % |")
            else:
                print(f"| {key} | {ms:.3f} | | | |")
        print(flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", nargs="+", type=int, default=[16384, 65536])
    ap.add_argument("--dims", nargs="+", type=int, default=[128, 256])
    ap.add_argument("--clusters", nargs="+", type=int, default=[8, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--one", nargs=2, type=int, metavar=("N", "D"), help="(internal) time one (n, d) in this process")
    args = ap.parse_args()
    if args.one:
        one(args.one[0], args.one[1], args.clusters, args.repeats)
        return
    print("# Silhouette: the norms and the sums kernel, beside tsne_sqdist\n")
    print(f"fp32, medians of {args.repeats} interleaved repeats, HIP-event times; every (n, d) in a process of its own.\n",
          flush=True)
    for n in args.points:
        for d in args.dims:
            cmd = [sys.executable, __file__, "--one", str(n), str(d), "--repeats", str(args.repeats), "--clusters",
                   *[str(c) for c in args.clusters]]
            try:
                done = subprocess.run(cmd, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print(f"\nn = {n}, d = {d}: not finished within {args.step_timeout} s; stopping here.")
                sys.exit(124)
            if done.returncode != 0:
                print(f"\nn = {n}, d = {d}: exit status {done.returncode}; stopping here.")
                sys.exit(done.returncode)


if __name__ == "__main__":
    main()
