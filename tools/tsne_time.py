#!/usr/bin/env python3
"""Times the 2-D layout (csrc/tsne.h, clane_amd/layout.py) on one MI355X.

    python tools/tsne_time.py [--points 8192 32768] [--repeats 5] [--fit-iters 1000] > profiles/r17_tsne.md

Per n (d = 128, fp32, Gaussian blobs), medians of `--repeats` interleaved repeats:
  * every kernel of a fit: clane_tsne_sqdist_f32, clane_tsne_affinities_f32 (perplexity 30), clane_tsne_symmetrize_f32,
    clane_tsne_forces_f32 in its three forms (with and without the KL terms; with cached instead of non-temporal loads of
    P), clane_tsne_step_f32;
  * the forces kernel's n^2 * 4 B / time -- P is read exactly once -- against the 8 TB/s peak of the HBM;
  * a whole fit of `--fit-iters` iterations from the PCA initialisation, early stops off.
No threshold is set: the numbers are what they are.

Every n is a child process of its own under `--step-timeout` seconds; the first that fails or runs out of time ends the
run -- nothing more is started on the card after it.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HBM_PEAK = 8.0e12
D = 128


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def one(n: int, repeats: int, fit_iters: int) -> None:
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from clane_amd import _hip
    from clane_amd.engine import SweepEngine
    from clane_amd.layout import TSNE
    from clane_amd.partition import HostCSR

    dev = _hip.require_gpu("cuda:0")
    k = _hip.kernels()
    rng = np.random.default_rng(0)
    y = rng.integers(0, 10, n)
    X = torch.from_numpy((4.0 * rng.standard_normal((10, D)))[y].astype(np.float32)) + torch.randn(n, D)
    csr = HostCSR(n, np.arange(n + 1, dtype=np.int64), ((np.arange(n) + 1) % n).astype(np.int32))
    with torch.cuda.device(dev):
        eng = SweepEngine(csr, X, dev)
        del X
        tsne = TSNE(eng, max_iter=fit_iters, min_grad_norm=0.0, n_iter_without_progress=fit_iters)
        Z, rows = tsne.table_and_rows(torch.arange(n), "Z")
        mu = tsne.column_mean(Z, rows)
        f32 = torch.float32
        Dm = torch.empty(n, n, dtype=f32, device=dev)
        P = torch.empty(n, n, dtype=f32, device=dev)
        sq, beta = torch.empty(n, dtype=f32, device=dev), torch.empty(n, dtype=f32, device=dev)
        partials = torch.empty(k.tsne_symmetrize_ws_len(n), dtype=torch.float64, device=dev)
        Y = tsne.pca_init(Z, rows) * 1e4                      # a layout of unit scale: what most iterations see
        Yn, V, G = torch.empty_like(Y), torch.zeros_like(Y), torch.ones_like(Y)
        F = torch.empty(n, 6, dtype=f32, device=dev)
        stats = torch.zeros(4, dtype=torch.float64, device=dev)

        def affinities():                                     # in place: every repeat starts from the distances again
            P.copy_(Dm)
            return timed(torch, lambda: k.tsne_affinities(P, 30.0, beta))

        def symmetrize():                                     # (a second pass over a symmetrised P costs the same)
            return timed(torch, lambda: k.tsne_symmetrize(P, partials))

        runs = {
            "sqdist": lambda: timed(torch, lambda: k.tsne_sqdist(Z, D, rows, mu, sq, Dm)),
            "affinities (perplexity 30)": affinities,
            "symmetrize": symmetrize,
            "forces, KL terms, non-temporal P": lambda: timed(torch, lambda: k.tsne_forces(P, Y, F, kl=True)),
            "forces, no KL terms, non-temporal P": lambda: timed(torch, lambda: k.tsne_forces(P, Y, F, kl=False)),
            "forces, no KL terms, cached P": lambda: timed(torch, lambda: k.tsne_forces(P, Y, F, kl=False, cached=True)),
            "step": lambda: timed(torch, lambda: k.tsne_step(F, Y, 1.0, 0.8, 200.0, 0.0, V, G, Yn, stats)),
        }
        for fn in runs.values():
            fn()                                              # warm-up, in the order the steps depend on each other
        times = {key: [] for key in runs}
        for _ in range(repeats):                              # interleaved
            for key, fn in runs.items():
                times[key].append(fn())
        med = {key: statistics.median(v) for key, v in times.items()}
        print(f"## n = {n}, d = {D}: P is {4 * n * n / 2 ** 30:.2f} GiB\n")
        print("| kernel | ms | n^2 * 4 B / time | of 8 TB/s |\n|---|---|---|---|")
        for key in runs:
            if key.startswith("forces"):
                rate = 4.0 * n * n / (med[key] * 1e-3)
                print(f"| {key} | {med[key]:.3f} | {rate / 1e12:.2f} TB/s | {100 * rate / HBM_PEAK:.0f} % |")
            else:
                print(f"| {key} | {med[key]:.3f} | | |")
        print(flush=True)
        del Dm, P
        torch.cuda.empty_cache()
        state = {}
        fit_ms = timed(torch, lambda: state.update(fit=tsne.fit(Z, rows)))
        fit = state["fit"]
        print(f"Whole fit, PCA initialisation, {fit.iterations} iterations: {fit_ms / 1e3:.2f} s "
              f"(KL {fit.kl_init:.4f} -> {fit.kl:.4f}, |g| {fit.grad_norm:.3g}).\n", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", nargs="+", type=int, default=[8192, 32768])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fit-iters", type=int, default=1000)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--one", type=int, metavar="N", help="(internal) time one n in this process")
    args = ap.parse_args()
    if args.one:
        one(args.one, args.repeats, args.fit_iters)
        return
    print("# t-SNE: every kernel of a fit, and a whole fit\n")
    print(f"fp32, d = {D}, medians of {args.repeats} interleaved repeats; every n in a process of its own.\n", flush=True)
    for n in args.points:
        cmd = [sys.executable, __file__, "--one", str(n), "--repeats", str(args.repeats), "--fit-iters",
               str(args.fit_iters)]
        try:
            done = subprocess.run(cmd, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"\nn = {n}: not finished within {args.step_timeout} s; stopping here.")
            sys.exit(124)
        if done.returncode != 0:
            print(f"\nn = {n}: exit status {done.returncode}; stopping here.")
            sys.exit(done.returncode)


if __name__ == "__main__":
    main()
