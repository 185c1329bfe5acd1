#!/usr/bin/env python3
"""Times k-means (csrc/kmeans.h, clane_amd/cluster.py) on one MI355X, beside the same iteration in torch.

    python tools/kmeans_time.py [--shapes config2 config3] [--clusters 8 64 1024] [--repeats 5] > profiles/r11_kmeans.md

Per shape (config 2: 200k x 128, config 3: 2M x 256; fp32) and K, medians of `--repeats` interleaved repeats:
  * one Lloyd iteration of ONE restart, its three steps separately: clane_kmeans_assign_f32, the stable sort + bincount
    (torch), clane_kmeans_update_f32,
  * the same iteration in torch on the same card: chunked Z @ C.T, argmin, index_add_,
  * a whole fit of 10 restarts from k-means++ (`--fit-iters` caps the updates).
The assignment is 2 n K d FLOP per restart; clane_project_rows_f32 runs at 104.8 TF/s.

Every (shape, K) is a child process of its own under `--step-timeout` seconds; the first that fails or runs out of time
ends the run -- nothing more is started on the card after it.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = {"config2": (200_000, 128), "config3": (2_000_000, 256), "small": (20_000, 64)}
TORCH_CHUNK = 1 << 16       # rows per Z @ C.T slab of the torch iteration: n x K never exists there either


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def one(name: str, K: int, repeats: int, restarts: int, fit_iters: int) -> None:
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from clane_amd import _hip
    from clane_amd.cluster import KMeans
    from clane_amd.engine import SweepEngine
    from clane_amd.partition import HostCSR

    n, d = SHAPES[name]
    dev = _hip.require_gpu("cuda:0")
    k = _hip.kernels()
    rng = np.random.default_rng(0)
    y = rng.integers(0, K, n)
    X = torch.from_numpy(rng.standard_normal((K, d), dtype=np.float32)[y]) + torch.randn(n, d)
    csr = HostCSR(n, np.arange(n + 1, dtype=np.int64), ((np.arange(n) + 1) % n).astype(np.int32))
    with torch.cuda.device(dev):
        eng = SweepEngine(csr, X, dev)
        del X
        Z = eng.Zcur
        rows = eng.pos.to(torch.int32).contiguous()
        rl = rows.long()
        centres = Z[rl[torch.randperm(n, device=dev)[:K]], :d].float().reshape(1, K, d).contiguous()
        csq = (centres * centres).sum(2)
        assign = torch.empty(n, 1, dtype=torch.int32, device=dev)
        best = torch.empty(n, 1, device=dev)
        new, csq_new = torch.empty_like(centres), torch.empty_like(csq)
        ws = torch.empty(k.kmeans_update_ws_len(n, 1, K, d), device=dev)
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        state = {}

        def fused_assign():
            k.kmeans_assign(Z, d, rows, centres, csq, assign, best)

        def sort_step():
            key = assign[:, 0].long()
            state["order"] = rows[torch.sort(key, stable=True).indices].contiguous()
            state["seg"] = torch.cat([zero, torch.bincount(key, minlength=K).cumsum(0)])

        def fused_update():
            k.kmeans_update(Z, d, state["order"], state["seg"], centres, ws, new, csq_new)

        def torch_iteration():
            c = centres[0]
            out = torch.empty(n, dtype=torch.int64, device=dev)
            for a in range(0, n, TORCH_CHUNK):
                zc = Z[rl[a:a + TORCH_CHUNK], :d]
                out[a:a + TORCH_CHUNK] = (csq[0][None, :] - 2.0 * (zc @ c.T)).argmin(1)
            sums = torch.zeros(K, d, device=dev).index_add_(0, out, Z[rl, :d])
            counts = torch.bincount(out, minlength=K).clamp(min=1)
            return sums / counts[:, None]

        runs = {"assign (fused)": fused_assign, "sort + bincount (torch)": sort_step, "update (fused)": fused_update,
                "torch: chunked Z @ C.T, argmin, index_add_": torch_iteration}
        for fn in runs.values():
            fn()                                            # warm-up, in the order the steps depend on each other
        times = {key: [] for key in runs}
        for _ in range(repeats):                            # interleaved
            for key, fn in runs.items():
                times[key].append(timed(torch, fn))
        med = {key: statistics.median(v) for key, v in times.items()}
        flop = 2.0 * n * K * d
        ours = med["assign (fused)"] + med["sort + bincount (torch)"] + med["update (fused)"]
        print(f"## {name}: n = {n}, d = {d}, K = {K}\n")
        print("| step | ms | TF/s (2 n K d) |\n|---|---|---|")
        for key in runs:
            rate = f"{flop / med[key] / 1e9:.1f}" if "assign" in key or key.startswith("torch") else ""
            print(f"| {key} | {med[key]:.3f} | {rate} |")
        print(f"| one iteration, the three steps | {ours:.3f} | {flop / ours / 1e9:.1f} |")
        print(f"\nclane_project_rows_f32: 104.8 TF/s.  Ours / torch = "
              f"{ours / med['torch: chunked Z @ C.T, argmin, index_add_']:.2f}.\n")
        km = KMeans(eng, max_iter=fit_iters)
        fit_ms = timed(torch, lambda: state.update(fit=km.fit(Z, rows, K, restarts=restarts, seed=0)))
        fit = state["fit"]
        print(f"Whole fit, {restarts} restarts from k-means++, at most {fit_iters} updates: {fit_ms / 1e3:.2f} s "
              f"(updates per restart {fit.iterations.tolist()}, converged {int(fit.converged.sum())} / {restarts}, "
              f"kernel calls {km.passes}, empty centres {fit.empty.tolist()}).\n", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["config2", "config3"], choices=sorted(SHAPES))
    ap.add_argument("--clusters", nargs="+", type=int, default=[8, 64, 1024])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--restarts", type=int, default=10)
    ap.add_argument("--fit-iters", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--one", nargs=2, metavar=("SHAPE", "K"), help="(internal) time one shape and K in this process")
    args = ap.parse_args()
    if args.one:
        one(args.one[0], int(args.one[1]), args.repeats, args.restarts, args.fit_iters)
        return
    print("# k-means: one Lloyd iteration and a whole fit\n")
    print(f"fp32, medians of {args.repeats} interleaved repeats; every (shape, K) in a process of its own.\n", flush=True)
    for name in args.shapes:
        for K in args.clusters:
            cmd = [sys.executable, __file__, "--one", name, str(K), "--repeats", str(args.repeats), "--restarts",
                   str(args.restarts), "--fit-iters", str(args.fit_iters)]
            try:
                done = subprocess.run(cmd, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print(f"\n{name}, K = {K}: not finished within {args.step_timeout} s; stopping here.")
                sys.exit(124)
            if done.returncode != 0:
                print(f"\n{name}, K = {K}: exit status {done.returncode}; stopping here.")
                sys.exit(done.returncode)


if __name__ == "__main__":
    main()
