#!/usr/bin/env python3
"""Timing of held-out link evaluation (LinkRanker.rank_pairs, csrc/link_eval.h) on one GPU: one JSON line per
(workload, B).

With HIP events after a warm-up, medians of --reps repeats in which the routes take turns (count, top-k, torch, count, ...):
  * clane_rank_count_* of one batch of B pairs (existing out-neighbours, self and the target excluded) with its achieved
    2 B V d FLOP/s;
  * the same batch's queries through clane_rank_scores_* with k = 10 -- the same MFMAs with the top-k insertion in the
    place of the counting;
  * torch's chunked (S[q] @ N.T) followed by a compare with the pair's score and a sum (no exclusion: the plain route).
The expectation this tool tests: rank_count is not slower than rank_scores at equal B, V, d; a difference below the
spread of the repeats (max - min of either route) counts as equal.
Usage: python tools/link_eval_time.py [--workloads rmat200k,rmat2m] [--reps 5]
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
CHUNK_BYTES = 4 << 30           # the torch route's [B, chunk] score block


def once(fn) -> float:
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z)


def interleaved(fns: dict, reps: int) -> dict:
    """All repeats in milliseconds per route; one warm-up each, then the routes take turns."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ts[name].append(once(fn))
    return ts


def median(v) -> float:
    return sorted(v)[len(v) // 2]


def torch_route(S, N, q_rows, t_rows):
    Sq = S[q_rows.long()]
    thr = (Sq * N[t_rows.long()]).sum(1, keepdim=True)
    step = max(1, CHUNK_BYTES // (Sq.shape[0] * Sq.element_size()))
    greater = torch.zeros(Sq.shape[0], dtype=torch.int64, device=S.device)
    for a in range(0, N.shape[0], step):
        greater += ((Sq @ N[a:a + step].T) > thr).sum(1)
    return greater


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rmat200k,rmat2m")
    ap.add_argument("--pairs", default="128,4096")
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
            for B in (int(b) for b in args.pairs.split(",")):
                gen = torch.Generator().manual_seed(7)
                src = torch.randperm(V, generator=gen)[:B].to(dev)
                dst = torch.randint(0, V, (B,), generator=gen).to(dev)
                q_rows = eng.pos[src].to(torch.int32).contiguous()
                t_rows = eng.pos[dst].to(torch.int32).contiguous()
                n_slabs = plan.rank_slabs(B, rows, ranker.query_tile)
                counts = torch.empty(B, n_slabs, 4, dtype=torch.int32, device=dev)
                score = torch.empty(B, dtype=eng.acc_dtype, device=dev)
                cand_s = torch.empty(B * n_slabs * k, dtype=eng.acc_dtype, device=dev)
                cand_i = torch.empty(B * n_slabs * k, dtype=torch.int32, device=dev)
                S = ranker.S.contiguous() if args.similarity == "bilinear" else ranker.S[:, :d]
                N = ranker.N.contiguous() if args.similarity == "bilinear" else ranker.N[:, :d]
                ts = interleaved({
                    "rank_count_ms": lambda: kern.rank_count(ranker.S, ranker.N, rows, d, q_rows, t_rows, ranker.mode,
                                                             ranker.sums2, ranker.sq, ranker.label, rowptr, colidx, True,
                                                             n_slabs, score, counts),
                    "rank_scores_ms": lambda: kern.rank_scores(ranker.S, ranker.N, rows, d, q_rows, ranker.mode, ranker.sums2,
                                                               ranker.sq, ranker.label, rowptr, colidx, True, k, n_slabs,
                                                               cand_s, cand_i),
                    "torch_matmul_compare_ms": lambda: torch_route(S, N, q_rows, t_rows),
                    "rank_pairs_ms": lambda: ranker.rank_pairs(src, dst, batch=B, refresh=False),
                }, args.reps)
                t = {name: median(v) for name, v in ts.items()}
                spread = max(max(ts[n]) - min(ts[n]) for n in ("rank_count_ms", "rank_scores_ms"))
                diff = t["rank_count_ms"] - t["rank_scores_ms"]
                flop = 2.0 * B * rows * d
                rec = {"workload": name, "V": V, "table_rows": rows, "E": int(csr.num_edges), "d": d, "dtype": "f32",
                       "similarity": args.similarity, "B": B, "k": k, "n_slabs": n_slabs, "reps": args.reps,
                       "gpu": torch.cuda.get_device_name(dev), **t,
                       "rank_count_tflops": flop / (t["rank_count_ms"] * 1e-3) / 1e12,
                       "rank_scores_tflops": flop / (t["rank_scores_ms"] * 1e-3) / 1e12,
                       "torch_tflops": flop / (t["torch_matmul_compare_ms"] * 1e-3) / 1e12,
                       "spread_ms": spread, "count_minus_scores_ms": diff,
                       "count_vs_scores": "equal" if abs(diff) <= spread else ("faster" if diff < 0 else "slower")}
                print(json.dumps(rec), flush=True)
                del counts, cand_s, cand_i
            del ranker, eng, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
