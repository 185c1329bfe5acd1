#!/usr/bin/env python3
"""Times the content reduction (csrc/content_pca.h, clane_amd/reduce.py) on one MI355X, beside torch on the same card and
numpy on the host.

    python tools/content_pca_time.py [--shapes cora200k config3wide] [--repeats 5] > profiles/r15_content_pca.md

Per shape (200k x 1433 -> 128 and 2M x 1024 -> 256; fp32), medians of `--repeats` interleaved repeats, each step between
two device synchronisations:
  * from device-resident input, in ContentPCA's blocks: clane_column_sums_f32, clane_gram_f32 (with ACCUMULATE over the
    blocks; TF/s of the n d^2 multiply-adds = 2 n d^2 / 2 FLOP that a symmetric Gram needs), clane_project_affine_f32,
  * the host eigh of the d x d Gram in float64,
  * the upload of X alone (pageable host memory, block by block, as fit() does it),
  * the whole ContentPCA.fit_transform from the host matrix and from the device-resident one,
  * the same Gram as (X - mu).T @ (X - mu) through torch on the same card (the centred copy is made before the clock
    starts; fp32 matmul as torch ships it),
  * the whole PCA through numpy on the host (mean, centring, X^T X, eigh, projection), `--host-repeats` times.

Every shape is a child process of its own under `--step-timeout` seconds; the first that fails or runs out of time ends
the run -- nothing more is started on the card after it.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = {"cora200k": (200_000, 1433, 128), "config3wide": (2_000_000, 1024, 256), "small": (20_000, 300, 16)}


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def one(name: str, repeats: int, host_repeats: int) -> None:
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from clane_amd import _hip
    from clane_amd.reduce import ContentPCA, default_block_rows, principal_axes

    n, d, m = SHAPES[name]
    dev = _hip.require_gpu("cuda:0")
    k = _hip.kernels()
    g = torch.Generator().manual_seed(0)
    X = torch.empty(n, d)
    step_gen = 1 << 17
    scale = torch.linspace(3.0, 0.3, d)
    for a in range(0, n, step_gen):                          # a decaying spectrum with an offset, made in slabs
        b = min(a + step_gen, n)
        X[a:b] = torch.randn(b - a, d, generator=g) * scale + 1.0
    step = default_block_rows(d, torch.float32)
    with torch.cuda.device(dev):
        Xd = X.to(dev)
        rows = torch.arange(min(step, n), dtype=torch.int32, device=dev)
        sums = torch.zeros(d, dtype=torch.float64, device=dev)
        ws_s = torch.empty(k.column_sums_ws_len(min(step, n), d), dtype=torch.float64, device=dev)
        ws_g = torch.empty(k.gram_ws_len(min(step, n), d), device=dev)
        G = torch.zeros(d, d, device=dev)
        Y = torch.empty(n, m, device=dev)
        state = {}

        def blocks():
            for a in range(0, n, step):
                yield a, min(a + step, n)

        def column_sums():
            for a, b in blocks():
                k.column_sums(Xd[a:b], d, rows[:b - a], ws_s, sums, accumulate=a > 0)
            state["mu"] = (sums / n).float()

        def gram():
            for a, b in blocks():
                k.gram(Xd[a:b], d, rows[:b - a], state["mu"], ws_g, G, accumulate=a > 0)

        def eigh():
            comp = principal_axes(G.cpu(), n, m)[0]
            state["W"] = torch.from_numpy(comp).float().to(dev)

        def project():
            for a, b in blocks():
                k.project_affine(Xd[a:b], d, rows[:b - a], state["mu"], state["W"], Y[a:b])

        def upload():
            for a, b in blocks():
                state["blk"] = X[a:b].to(dev)

        def fit_transform_host():
            state["Yh"] = ContentPCA(m).fit_transform(X)

        def fit_transform_device():
            state["Yd"] = ContentPCA(m).fit_transform(Xd)

        def torch_gram():
            state["Gt"] = state["Xc"].T @ state["Xc"]

        runs = {"column sums (device-resident)": column_sums, "Gram (device-resident)": gram,
                "eigh, float64 on the host (incl. G to the host)": eigh, "projection (device-resident)": project,
                "upload of X, block by block": upload, "fit_transform, host input": fit_transform_host,
                "fit_transform, device input": fit_transform_device}
        for fn in runs.values():
            fn()                                             # warm-up, in the order the steps depend on each other
        state["Xc"] = Xd - state["mu"]
        runs["torch: Xc.T @ Xc on the same card"] = torch_gram
        torch_gram()
        times = {key: [] for key in runs}
        for _ in range(repeats):                             # interleaved
            for key, fn in runs.items():
                times[key].append(timed(torch, fn))
        med = {key: statistics.median(v) for key, v in times.items()}
        rel = float((G - state["Gt"]).abs().max() / state["Gt"].abs().max())
        del state["Xc"], state["Gt"]

    host = []
    for _ in range(host_repeats):
        t0 = time.perf_counter()
        Xn = X.numpy()
        mu = Xn.mean(0, dtype=np.float64).astype(np.float32)
        Xc = Xn - mu
        lam, vec = np.linalg.eigh((Xc.T @ Xc).astype(np.float64))
        Yn = Xc @ vec[:, ::-1][:, :m].astype(np.float32)
        host.append((time.perf_counter() - t0) * 1e3)
        del Xc, Yn

    flop_gram = float(n) * d * d                             # 2 n d^2 / 2
    flop_proj = 2.0 * n * d * m
    print(f"## {name}: n = {n}, d = {d} -> {m}, fp32, blocks of {step} rows ({-(-n // step)} per pass)\n")
    print("| step | ms (median) | min .. max | rate |\n|---|---|---|---|")
    for key in runs:
        rate = ""
        if key.startswith("Gram") or key.startswith("torch"):
            rate = f"{flop_gram / med[key] / 1e9:.1f} TF/s of n d^2"
        elif key.startswith("projection"):
            rate = f"{flop_proj / med[key] / 1e9:.1f} TF/s of 2 n d m"
        elif key.startswith("column sums"):
            rate = f"{n * d * 4 / med[key] / 1e9:.2f} TB/s"
        elif key.startswith("upload"):
            rate = f"{n * d * 4 / med[key] / 1e6:.1f} GB/s"
        print(f"| {key} | {med[key]:.2f} | {min(times[key]):.2f} .. {max(times[key]):.2f} | {rate} |")
    print(f"| numpy on the host, whole PCA ({host_repeats} run{'s' if host_repeats > 1 else ''}) | "
          f"{statistics.median(host):.0f} | {min(host):.0f} .. {max(host):.0f} | |")
    kernels = med["column sums (device-resident)"] + med["Gram (device-resident)"] + med["projection (device-resident)"]
    print(f"\nThe three device passes: {kernels:.2f} ms; fit_transform from the host matrix: "
          f"{med['fit_transform, host input']:.0f} ms, of which {kernels / med['fit_transform, host input'] * 100:.1f} % are the "
          f"passes' kernels; max |G - G_torch| / max |G_torch| = {rel:.2e}.\n", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["cora200k", "config3wide"], choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=500)
    ap.add_argument("--one", metavar="SHAPE", help="(internal) time one shape in this process")
    args = ap.parse_args()
    if args.one:
        one(args.one, args.repeats, args.host_repeats)
        return
    print("# Content reduction: column sums, centred Gram, projection, and the whole fit_transform\n")
    print(f"fp32, one MI355X, medians of {args.repeats} interleaved repeats, every step between two device "
          f"synchronisations; every shape in a process of its own.\n", flush=True)
    for name in args.shapes:
        cmd = [sys.executable, __file__, "--one", name, "--repeats", str(args.repeats), "--host-repeats",
               str(args.host_repeats)]
        try:
            done = subprocess.run(cmd, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"\n{name}: not finished within {args.step_timeout} s; stopping here.")
            sys.exit(124)
        if done.returncode != 0:
            print(f"\n{name}: exit status {done.returncode}; stopping here.")
            sys.exit(done.returncode)


if __name__ == "__main__":
    main()
