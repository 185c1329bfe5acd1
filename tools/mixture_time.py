#!/usr/bin/env python3
"""Times the Gaussian mixture (csrc/mixture.h, clane_amd/mixture.py) on one MI355X, beside a Lloyd iteration of the
unchanged k-means at the same shape.

    python tools/mixture_time.py [--rows 200000 2000000] [--clusters 8 64] [--dtypes f32 bf16] [--repeats 5]

Per (n, K, dtype) at d = 128 and R = 10 restarts, medians of `--repeats` interleaved repeats:
  * one E-step (clane_mixture_estep_*, responsibilities written) and one M-step (clane_mixture_mstep_*) of all R restarts,
  * one Lloyd iteration of all R restarts: clane_kmeans_assign_*, the stable sort + bincount (torch), clane_kmeans_update_*,
  * a whole fit of R restarts from k-means (`--fit-iters` caps the EM iterations).
By bytes an EM iteration reads the rows twice and writes and reads resp [n, R Kp] once; a Lloyd iteration reads the rows
twice.  The contractions are 2 n (R Kp) (2 d) FLOP per step.

Every (n, K, dtype) is a child process of its own under `--step-timeout` seconds; the first that fails or runs out of
time ends the run -- nothing more is started on the card after it.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
D = 128


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def one(n: int, K: int, dtype_name: str, repeats: int, restarts: int, fit_iters: int) -> None:
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from clane_amd import _hip
    from clane_amd.cluster import KMeans
    from clane_amd.engine import SweepEngine
    from clane_amd.mixture import GaussianMixture, stack_parameters
    from clane_amd.partition import HostCSR

    d, R = D, restarts
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]
    acc = _hip.acc_dtype(dtype)
    dev = _hip.require_gpu("cuda:0")
    k = _hip.kernels()
    rng = np.random.default_rng(0)
    y = rng.integers(0, K, n)
    X = torch.from_numpy(rng.standard_normal((K, d), dtype=np.float32)[y] * 3.0) + torch.randn(n, d)
    csr = HostCSR(n, np.arange(n + 1, dtype=np.int64), ((np.arange(n) + 1) % n).astype(np.int32))
    with torch.cuda.device(dev):
        eng = SweepEngine(csr, X.to(dtype), dev)
        del X
        Z = eng.Zcur
        rows = eng.pos.to(torch.int32).contiguous()
        gm = GaussianMixture(eng, max_iter=fit_iters)
        Kp = _hip.mixture_padded_components(K)
        mean = gm.column_mean(Z, rows).to(acc).contiguous()
        pick = torch.stack([torch.randperm(n, device=dev)[:K] for _ in range(R)])
        mu = Z[rows.long()[pick], :d].double() - mean.double()
        Wm, cst = stack_parameters(torch.full((R, K), 1.0 / K, dtype=torch.float64, device=dev), mu,
                                   torch.ones(R, K, d, dtype=torch.float64, device=dev), Kp, acc)
        resp = torch.empty(n * R * Kp, dtype=acc, device=dev)
        ll = torch.empty(R, dtype=torch.float64, device=dev)
        ll_ws = torch.empty(k.mixture_ll_ws_len(n, R), dtype=torch.float64, device=dev)
        S = torch.empty(R * Kp, 2 * d, dtype=acc, device=dev)
        nk = torch.empty(R * Kp, dtype=acc, device=dev)
        ws = torch.empty(k.mixture_mstep_ws_len(n, R * Kp, d), dtype=acc, device=dev)
        centres = (mu + mean.double()).to(acc).contiguous()
        csq = (centres * centres).sum(2)
        assign = torch.empty(n, R, dtype=torch.int32, device=dev)
        best = torch.empty(n, R, dtype=acc, device=dev)
        new, csq_new = torch.empty_like(centres), torch.empty_like(csq)
        kws = torch.empty(k.kmeans_update_ws_len(n, R, K, d), dtype=acc, device=dev)
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        offset = (torch.arange(R, device=dev) * K)[:, None]
        state = {}

        def estep():
            k.mixture_estep(Z, d, rows, mean, Wm, cst, R, K, ll_ws, ll, resp=resp)

        def mstep():
            k.mixture_mstep(Z, d, rows, mean, resp, ws, S, nk)

        def lloyd_assign():
            k.kmeans_assign(Z, d, rows, centres, csq, assign, best)

        def lloyd_sort():
            key = (assign.T.long() + offset).reshape(-1)
            state["order"] = rows[torch.sort(key, stable=True).indices % n].contiguous()
            state["seg"] = torch.cat([zero, torch.bincount(key, minlength=R * K).cumsum(0)])

        def lloyd_update():
            k.kmeans_update(Z, d, state["order"], state["seg"], centres, kws, new, csq_new)

        runs = {"E-step": estep, "M-step": mstep, "Lloyd: assign": lloyd_assign, "Lloyd: sort + bincount (torch)": lloyd_sort,
                "Lloyd: update": lloyd_update}
        for fn in runs.values():
            fn()                                            # warm-up, in the order the steps depend on each other
        times = {key: [] for key in runs}
        for _ in range(repeats):                            # interleaved
            for key, fn in runs.items():
                times[key].append(timed(torch, fn))
        med = {key: statistics.median(v) for key, v in times.items()}
        flop = 2.0 * n * (R * Kp) * (2 * d)
        em = med["E-step"] + med["M-step"]
        lloyd = med["Lloyd: assign"] + med["Lloyd: sort + bincount (torch)"] + med["Lloyd: update"]
        elem = torch.empty(0, dtype=dtype).element_size()
        em_bytes = 2.0 * n * d * elem + 2.0 * n * R * Kp * torch.empty(0, dtype=acc).element_size()
        print(f"## n = {n}, d = {d}, K = {K} (Kp = {Kp}), R = {R}, {dtype_name}\n")
        print("| step | ms | TF/s (2 n R Kp 2 d) |\n|---|---|---|")
        for key in runs:
            rate = f"{flop / med[key] / 1e9:.1f}" if key in ("E-step", "M-step") else ""
            print(f"| {key} | {med[key]:.3f} | {rate} |")
        print(f"| one EM iteration | {em:.3f} | |\n| one Lloyd iteration | {lloyd:.3f} | |")
        print(f"\nEM / Lloyd = {em / lloyd:.2f}; by bytes (rows twice + resp written and read over rows twice) "
              f"{em_bytes / (2.0 * n * d * elem):.2f}; the EM iteration moves {em_bytes / 1e9:.2f} GB, "
              f"{em_bytes / em / 1e6:.0f} GB/s.\n")
        fit_ms = timed(torch, lambda: state.update(fit=gm.fit(Z, rows, K, restarts=R, seed=0)))
        fit = state["fit"]
        print(f"Whole fit, {R} restarts from k-means, at most {fit_iters} EM iterations: {fit_ms / 1e3:.2f} s "
              f"(iterations per restart {fit.iterations.tolist()}, converged {int(fit.converged.sum())} / {R}, kernel "
              f"calls {gm.passes}, empty components {fit.empty.tolist()}, clamped {fit.clamped.tolist()}).\n", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="+", type=int, default=[200_000, 2_000_000])
    ap.add_argument("--clusters", nargs="+", type=int, default=[8, 64])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--restarts", type=int, default=10)
    ap.add_argument("--fit-iters", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--one", nargs=3, metavar=("N", "K", "DTYPE"), help="(internal) time one case in this process")
    args = ap.parse_args()
    if args.one:
        one(int(args.one[0]), int(args.one[1]), args.one[2], args.repeats, args.restarts, args.fit_iters)
        return
    print("# Gaussian mixture: one EM iteration, one Lloyd iteration and a whole fit\n")
    print(f"d = {D}, medians of {args.repeats} interleaved repeats; every (n, K, dtype) in a process of its own.\n", flush=True)
    for n in args.rows:
        for K in args.clusters:
            for dtype in args.dtypes:
                cmd = [sys.executable, __file__, "--one", str(n), str(K), dtype, "--repeats", str(args.repeats),
                       "--restarts", str(args.restarts), "--fit-iters", str(args.fit_iters)]
                try:
                    done = subprocess.run(cmd, timeout=args.step_timeout)
                except subprocess.TimeoutExpired:
                    print(f"\nn = {n}, K = {K}, {dtype}: not finished within {args.step_timeout} s; stopping here.")
                    sys.exit(124)
                if done.returncode != 0:
                    print(f"\nn = {n}, K = {K}, {dtype}: exit status {done.returncode}; stopping here.")
                    sys.exit(done.returncode)


if __name__ == "__main__":
    main()
