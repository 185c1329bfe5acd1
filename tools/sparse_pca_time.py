#!/usr/bin/env python3
"""Times the sparse content reduction (csrc/sparse_rows.h, ContentPCA.fit_sparse) on one MI355X, beside scikit-learn's
randomized_svd of the same matrix on the host.

    python tools/sparse_pca_time.py [--shapes bow200k] [--repeats 5] > profiles/sparse_pca.md

Per shape (a synthetic bag of words: every row draws its words from one of `topics` Zipf distributions; the counts are the
values; fp32), medians of `--repeats` repeats, each step between two device synchronisations:
  * the transpose (SparseRows.transposed: torch's stable sort),
  * clane_csr_spmm_f32 on S (Y = S Omega - 1 s^T) and on S^T (Z = S^T Q - mu s^T) at the fit's sketch width l, with the
    achieved bytes/s of the algorithmic nnz (4 l + 8) bytes per product (a gathered row of B and one col / val pair per
    non-zero; the output and the row pointers are left out),
  * clane_csr_row_sums_f32 on S^T,
  * the whole ContentPCA.fit_sparse (defaults: oversample 16, 4 power iterations) and transform_sparse from the
    device-resident matrix,
  * sklearn.utils.extmath.randomized_svd (n_oversamples 16, n_iter 4, QR normaliser) of the same matrix as scipy CSR on
    the host, once.  It does not centre: a comparison of the work, not of the result.

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
# name: (n, D, topics, words per row, dim)
SHAPES = {"small": (20_000, 2_000, 12, 40, 16), "bow200k": (200_000, 10_000, 50, 100, 64),
          "bow2m": (2_000_000, 10_000, 50, 100, 128)}


def bag_of_words(np, n, D, topics, words, seed=0, noise=0.15):
    """(indptr, indices, data) with duplicates: every row `words` draws (Poisson) by inverse CDF from its topic's Zipf
    distribution over a permutation of the vocabulary, or (with probability `noise`) from the global one."""
    g = np.random.default_rng(seed)
    cdf = np.cumsum(1.0 / np.arange(1, D + 1) ** 1.1)
    cdf /= cdf[-1]
    perms = np.stack([g.permutation(D) for _ in range(topics)]).astype(np.int32)
    lengths = np.maximum(1, g.poisson(words, size=n))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    row = np.repeat(np.arange(n), lengths)
    rank = np.searchsorted(cdf, g.random(row.shape[0])).astype(np.int32)
    topic = g.integers(topics, size=n)[row]
    col = np.where(g.random(row.shape[0]) < noise, rank, perms[topic, rank])
    return indptr, col.astype(np.int32), np.ones(row.shape[0], dtype=np.float32)


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def one(name: str, repeats: int, host: bool) -> None:
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from clane_amd import _hip
    from clane_amd.reduce import ContentPCA
    from clane_amd.sparse import SparseRows

    n, D, topics, words, dim = SHAPES[name]
    dev = _hip.require_gpu("cuda:0")
    k = _hip.kernels()
    t0 = time.perf_counter()
    S = SparseRows(*bag_of_words(np, n, D, topics, words), (n, D))          # sorts the rows, sums the duplicates
    made = time.perf_counter() - t0
    l = -(-min(dim + 16, D, n) // 4) * 4
    med = statistics.median
    with torch.cuda.device(dev):
        Sd = S.to(dev)
        St = Sd.transposed()
        Sd.segments(), St.segments()
        g = torch.Generator().manual_seed(0)
        Omega, Q = torch.randn(D, l, generator=g).to(dev), torch.randn(n, l, generator=g).to(dev)
        s, mu = torch.randn(l, generator=g).to(dev), torch.randn(D, generator=g).to(dev)
        Y, Z = torch.empty(n, l, device=dev), torch.empty(D, l, device=dev)
        sums = torch.empty(D, dtype=torch.float64, device=dev)
        ws = torch.empty(max(1, St.segments()[2].numel()) * l, device=dev)
        steps = {"transpose": lambda: Sd.transposed(),
                 "csr_spmm S": lambda: k.csr_spmm(Sd, Omega, l, Y, s=s),
                 "csr_spmm S^T": lambda: k.csr_spmm(St, Q, l, Z, a=mu, s=s, ws=ws),
                 "csr_row_sums S^T": lambda: k.csr_row_sums(St, sums),
                 "fit_sparse": lambda: ContentPCA(dim).fit_sparse(Sd)}
        for fn in steps.values():                                           # warm-up: code objects, the allocator
            fn()
        t = {key: med([timed(torch, fn) for _ in range(repeats)]) for key, fn in steps.items()}
        pca = ContentPCA(dim).fit_sparse(Sd)
        t["transform_sparse"] = med([timed(torch, lambda: pca.transform_sparse(Sd)) for _ in range(repeats)])
    nnz = S.nnz
    lens_t = (St.rowptr[1:] - St.rowptr[:-1])
    product = nnz * (4 * l + 8)
    print(f"## {name}: n = {n}, D = {D}, nnz = {nnz} ({nnz / n:.1f} per row), dim = {dim}, l = {l}; the longest row of "
          f"S^T: {int(lens_t.max())} non-zeros, {St.segments()[2].numel()} segments in {St.segments()[0].numel()} long "
          f"rows (host: made in {made:.1f} s)")
    print("| step | ms | GB/s of nnz (4 l + 8) |")
    print("|---|---|---|")
    for key, ms in t.items():
        rate = f"{product / ms / 1e6:.0f}" if key.startswith("csr_spmm") else ""
        print(f"| {key} | {ms:.3f} | {rate} |")
    print(f"explained variance ratio kept: {pca.explained_variance_ratio_.sum():.4f}")
    if host:
        import scipy.sparse as sp
        from sklearn.utils.extmath import randomized_svd
        X = sp.csr_matrix((S.val.numpy(), S.col.numpy(), S.rowptr.numpy()), shape=(n, D))
        t0 = time.perf_counter()
        randomized_svd(X, n_components=dim, n_oversamples=16, n_iter=4, power_iteration_normalizer="QR", random_state=0)
        print(f"host: sklearn randomized_svd (uncentred, {torch.get_num_threads()} threads): "
              f"{(time.perf_counter() - t0) * 1e3:.0f} ms")
    sys.stdout.flush()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["bow200k"], choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip scikit-learn on the host")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        one(args.child, args.repeats, not args.no_host)
        return 0
    for name in args.shapes:
        cmd = [sys.executable, __file__, "--child", name, "--repeats", str(args.repeats)] + \
            (["--no-host"] if args.no_host else [])
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {args.step_timeout} s; nothing more is started", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"{name}: exit status {rc}; nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
