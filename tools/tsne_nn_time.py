#!/usr/bin/env python3
"""Times the neighbour-sparse 2-D layout (csrc/tsne_nn.h, layout.NeighbourTSNE) next to the exact one on one MI355X.

    python tools/tsne_nn_time.py [--points 20000 65536 262144] [--repeats 5] [--fit-iters 50] > profiles/r19_tsne_nn.md

Per n (d = 128, fp32, Gaussian blobs, perplexity 30, k = 90), medians of `--repeats` interleaved repeats, each between two
device synchronisations:
  * method "neighbours": clane_knn_sqdist_f32, clane_tsne_nn_affinities_f32, the sort that builds the CSR (torch),
    clane_tsne_nn_plogp_f32, clane_tsne_nn_attract_f32 with and without the KL terms, clane_tsne_repulse_f32 and its pair
    rate n^2 / time -- 13 flops a pair -- against the 157.3 TFLOP/s fp32 vector peak, clane_tsne_step_f32; the whole
    `joint_probabilities`; an iteration = attract (no KL terms) + repulse + step; the peak of torch's allocator over
    `joint_probabilities` and a fit of `--fit-iters` iterations;
  * method "exact", where P [n, n] fits (n <= 65536): the whole `joint_probabilities`, clane_tsne_forces_f32 without the
    KL terms, the step; an iteration = forces + step.  These kernels are not touched by the neighbour method.
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
FP32_VECTOR_PEAK = 157.3e12
PAIR_FLOPS = 13          # 2 subtractions, mul + fma, 1 + d2, the reciprocal, q * q, two fma, s += q
D = 128


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def medians(torch, runs, repeats):
    for fn in runs.values():
        fn()                                                  # warm-up, in the order the steps depend on each other
    times = {key: [] for key in runs}
    for _ in range(repeats):                                  # interleaved
        for key, fn in runs.items():
            times[key].append(timed(torch, fn))
    return {key: statistics.median(v) for key, v in times.items()}


def one(n: int, repeats: int, fit_iters: int) -> None:
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from clane_amd import _hip, layout
    from clane_amd.engine import SweepEngine
    from clane_amd.partition import HostCSR

    dev = _hip.require_gpu("cuda:0")
    k = _hip.kernels()
    rng = np.random.default_rng(0)
    y = rng.integers(0, 10, n)
    X = torch.from_numpy((4.0 * rng.standard_normal((10, D)))[y].astype(np.float32)) + torch.randn(n, D)
    csr = HostCSR(n, np.arange(n + 1, dtype=np.int64), ((np.arange(n) + 1) % n).astype(np.int32))
    f32 = torch.float32
    with torch.cuda.device(dev):
        eng = SweepEngine(csr, X, dev)
        del X
        nn = layout.NeighbourTSNE(eng, max_iter=fit_iters, min_grad_norm=0.0, n_iter_without_progress=fit_iters)
        Z, rows = nn.table_and_rows(torch.arange(n), "Z")
        kk = nn.neighbours_for(n)
        slabs = layout.knn_slabs(n, kk)
        mu = nn.column_mean(Z, rows)
        ids = torch.empty(n, kk, dtype=torch.int32, device=dev)
        sqd, p = torch.empty(n, kk, dtype=f32, device=dev), torch.empty(n, kk, dtype=f32, device=dev)
        ci = cd = None
        if slabs > 1:
            ci = torch.empty(n * slabs * kk, dtype=torch.int32, device=dev)
            cd = torch.empty(n * slabs * kk, dtype=f32, device=dev)
        sq, beta = torch.empty(n, dtype=f32, device=dev), torch.empty(n, dtype=f32, device=dev)
        row_plogp = torch.empty(n, dtype=torch.float64, device=dev)
        Y = nn.pca_init(Z, rows) * 1e4                        # a layout of unit scale: what most iterations see
        Yn, V, G = torch.empty_like(Y), torch.zeros_like(Y), torch.ones_like(Y)
        F = torch.empty(n, 6, dtype=f32, device=dev)
        stats = torch.zeros(4, dtype=torch.float64, device=dev)
        state = {}

        def joint():
            state["P"] = layout.sparse_joint(ids, p)

        runs = {
            f"knn_sqdist (k = {kk}, {slabs} slab{'s' if slabs > 1 else ''})":
                lambda: k.knn_sqdist(Z, D, rows, mu, sq, ids, sqd, slabs, ci, cd),
            "nn_affinities (perplexity 30)": lambda: k.tsne_nn_affinities(sqd, ids, 30.0, p, beta),
            "sparse_joint (torch: sort, add, divide, CSR)": joint,
            "nn_plogp": lambda: k.tsne_nn_plogp(state["P"].rowptr, state["P"].val, row_plogp),
            "nn_attract, KL terms": lambda: k.tsne_nn_attract(state["P"].rowptr, state["P"].cols, state["P"].val, Y, F, kl=True),
            "nn_attract, no KL terms": lambda: k.tsne_nn_attract(state["P"].rowptr, state["P"].cols, state["P"].val, Y, F,
                                                                 kl=False),
            "repulse": lambda: k.tsne_repulse(Y, F),
            "step": lambda: k.tsne_step(F, Y, 1.0, 0.8, 200.0, 0.0, V, G, Yn, stats),
            "joint_probabilities, whole": lambda: nn.joint_probabilities(Z, rows),
        }
        med = medians(torch, runs, repeats)
        nnz = state["P"].nnz
        longest = int((state["P"].rowptr[1:] - state["P"].rowptr[:-1]).max())
        print(f"## n = {n}, d = {D}\n")
        print(f"### method neighbours: k = {kk}, nnz = {nnz} ({nnz / (2 * n * kk):.2f} of 2nk), longest row {longest}\n")
        print("| step | ms | |\n|---|---|---|")
        for key in runs:
            note = ""
            if key == "repulse":
                rate = float(n) * n / (med[key] * 1e-3)
                note = (f"{rate / 1e12:.2f} T pairs/s; x {PAIR_FLOPS} flops = {rate * PAIR_FLOPS / 1e12:.1f} TFLOP/s, "
                        f"{100 * rate * PAIR_FLOPS / FP32_VECTOR_PEAK:.0f} % of the fp32 vector peak")
            print(f"| {key} | {med[key]:.3f} | {note} |")
        it_nn = med["nn_attract, no KL terms"] + med["repulse"] + med["step"]
        print(f"| an iteration: attract (no KL terms) + repulse + step | {it_nn:.3f} | |")
        print(flush=True)
        del ids, sqd, p, ci, cd
        state.clear()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fit_ms = timed(torch, lambda: state.update(fit=nn.fit(Z, rows)))
        peak = torch.cuda.max_memory_allocated(dev) - base
        fit = state.pop("fit")
        print(f"Whole fit, PCA initialisation, {fit.iterations} iterations: {fit_ms / 1e3:.2f} s (KL {fit.kl_init:.4f} -> "
              f"{fit.kl:.4f}); peak of the allocator above the table: {peak / 2 ** 30:.2f} GiB "
              f"(workspace_bytes says {nn.workspace_bytes(n) / 2 ** 30:.2f} GiB).\n", flush=True)
        del fit
        torch.cuda.empty_cache()

        if n > layout.MAX_POINTS:
            print("### method exact: P [n, n] does not fit the method's limit.\n", flush=True)
            return
        ex = layout.TSNE(eng, max_iter=fit_iters, min_grad_norm=0.0, n_iter_without_progress=fit_iters)

        def exact_joint():
            state["PB"] = None
            state["PB"] = ex.joint_probabilities(Z, rows)

        runs = {
            "joint_probabilities, whole": exact_joint,
            "forces, no KL terms": lambda: k.tsne_forces(state["PB"][0], Y, F, kl=False),
            "forces, KL terms": lambda: k.tsne_forces(state["PB"][0], Y, F, kl=True),
            "step": lambda: k.tsne_step(F, Y, 1.0, 0.8, 200.0, 0.0, V, G, Yn, stats),
        }
        med = medians(torch, runs, repeats)
        print(f"### method exact: P is {4 * n * n / 2 ** 30:.2f} GiB\n")
        print("| step | ms |\n|---|---|")
        for key in runs:
            print(f"| {key} | {med[key]:.3f} |")
        it_ex = med["forces, no KL terms"] + med["step"]
        print(f"| an iteration: forces (no KL terms) + step | {it_ex:.3f} |")
        print(f"\nAn iteration of method neighbours takes {it_nn / it_ex:.2f} of an exact one.\n", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", nargs="+", type=int, default=[20000, 65536, 262144])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fit-iters", type=int, default=50)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--one", type=int, metavar="N", help="(internal) time one n in this process")
    args = ap.parse_args()
    if args.one:
        one(args.one, args.repeats, args.fit_iters)
        return
    print("# Neighbour-sparse t-SNE next to the exact one: every step of a fit\n")
    print(f"fp32, d = {D}, perplexity 30, medians of {args.repeats} interleaved repeats; every n in a process of its own.\n",
          flush=True)
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
