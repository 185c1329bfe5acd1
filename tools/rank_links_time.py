#!/usr/bin/env python3
"""Timing of link ranking (LinkRanker.top_k, csrc/link_rank.h) on one GPU: one JSON line per (workload, Q).

With HIP events after a warm-up, medians of --reps repeats in which the routes take turns (native, torch, native, ...):
  * LinkRanker.top_k of one batch of Q sources (rank_scores + rank_merge, existing out-neighbours and self excluded),
    and the two kernels on their own, with the achieved 2 Q V d FLOP/s of the fused kernel;
  * beside it, on the same card and the same tables, torch's (S[q] @ N.T).topk(k) in column chunks that fit memory,
    the per-chunk winners merged by one more topk (no exclusion: the plain route).
The points of comparison are the torch route and what clane_project_rows_f32 reaches with the same tiling
(tools/bilinear_build_p_time.py).  Usage: python tools/rank_links_time.py [--workloads rmat200k,rmat2m] [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from clane_amd import _hip, plan, synth  # noqa: E402
from clane_amd.graph import Graph  # noqa: E402
from clane_amd.links import LinkRanker  # noqa: E402
from clane_amd.similarity import AsymmertricSimilarity, CosineSimilarity  # noqa: E402
from clane_amd.train import sorted_adjacency  # noqa: E402

SHAPES = {"rmat200k": (200_000, 4_000_000, 128, 1, 2), "rmat2m": (2_000_000, 40_000_000, 256, 3, 4)}
CHUNK_BYTES = 4 << 30           # the torch route's [Q, chunk] score block


def once(fn) -> float:
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z)


def interleaved(fns: dict, reps: int) -> dict:
    """Median milliseconds per route; one warm-up each, then the routes take turns."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ts[name].append(once(fn))
    return {name: sorted(v)[len(v) // 2] for name, v in ts.items()}


def torch_route(S, N, q_rows, k: int):
    Sq = S[q_rows.long()]
    step = max(1, CHUNK_BYTES // (Sq.shape[0] * Sq.element_size()))
    best_s, best_i = [], []
    for a in range(0, N.shape[0], step):
        s, i = (Sq @ N[a:a + step].T).topk(min(k, N[a:a + step].shape[0]), dim=1)
        best_s.append(s)
        best_i.append(i + a)
    s, pick = torch.cat(best_s, 1).topk(k, dim=1)
    return s, torch.gather(torch.cat(best_i, 1), 1, pick)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rmat200k,rmat2m")
    ap.add_argument("--queries", default="128,4096")
    ap.add_argument("--similarity", default="bilinear", choices=["bilinear", "cosine"])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = _hip.require_gpu("cuda:0")
    for name in args.workloads.split(","):
        V, E, d, gseed, xseed = SHAPES[name]
        csr = synth.rmat_csr(V, E, seed=gseed, device=str(dev))
        X = synth.gaussian_X(V, d, seed=xseed)
        torch.manual_seed(0)
        sim = AsymmertricSimilarity(d).to(dev) if args.similarity == "bilinear" else CosineSimilarity(mode="per_edge")
        with torch.cuda.device(dev):
            g = Graph.from_csr(csr, X)
            eng = g.engine(dev, cosine_mode="per_edge" if args.similarity == "cosine" else "reference")
            ranker = LinkRanker(eng, sim)
            ranker.prepare()
            rowptr, colidx, _ = sorted_adjacency(eng)
            rows, kern, k = ranker.rows, eng.k, args.k
            for Q in (int(q) for q in args.queries.split(",")):
                src = torch.randperm(V, generator=torch.Generator().manual_seed(7))[:Q].to(dev)
                q_rows = eng.pos[src].to(torch.int32).contiguous()
                n_slabs = plan.rank_slabs(Q, rows, ranker.query_tile)
                cand_s = torch.empty(Q * n_slabs * k, dtype=eng.acc_dtype, device=dev)
                cand_i = torch.empty(Q * n_slabs * k, dtype=torch.int32, device=dev)
                out_s = torch.empty(Q, k, dtype=eng.acc_dtype, device=dev)
                out_i = torch.empty(Q, k, dtype=torch.int32, device=dev)
                S = ranker.S.contiguous() if args.similarity == "bilinear" else ranker.S[:, :d]
                N = ranker.N.contiguous() if args.similarity == "bilinear" else ranker.N[:, :d]
                t = interleaved({
                    "top_k_ms": lambda: ranker.top_k(k, src, batch=Q, refresh=False),
                    "torch_matmul_topk_ms": lambda: torch_route(S, N, q_rows, k),
                    "rank_scores_ms": lambda: kern.rank_scores(ranker.S, ranker.N, rows, d, q_rows, ranker.mode, ranker.sums2,
                                                               ranker.sq, ranker.label, rowptr, colidx, True, k, n_slabs,
                                                               cand_s, cand_i),
                    "rank_scores_no_exclusion_ms": lambda: kern.rank_scores(ranker.S, ranker.N, rows, d, q_rows, ranker.mode,
                                                                            ranker.sums2, ranker.sq, ranker.label, None, None,
                                                                            True, k, n_slabs, cand_s, cand_i),
                    "rank_merge_ms": lambda: kern.rank_merge(cand_s, cand_i, n_slabs, k, out_s, out_i),
                }, args.reps)
                flop = 2.0 * Q * rows * d
                rec = {"workload": name, "V": V, "table_rows": rows, "E": int(csr.num_edges), "d": d, "dtype": "f32",
                       "similarity": args.similarity, "Q": Q, "k": k, "n_slabs": n_slabs, "reps": args.reps,
                       "gpu": torch.cuda.get_device_name(dev), **t,
                       "rank_scores_tflops": flop / (t["rank_scores_ms"] * 1e-3) / 1e12,
                       "top_k_tflops": flop / (t["top_k_ms"] * 1e-3) / 1e12,
                       "torch_tflops": flop / (t["torch_matmul_topk_ms"] * 1e-3) / 1e12,
                       "speedup_vs_torch": t["torch_matmul_topk_ms"] / t["top_k_ms"]}
                print(json.dumps(rec), flush=True)
                del cand_s, cand_i
            del ranker, eng, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
