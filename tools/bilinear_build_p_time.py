#!/usr/bin/env python3
"""Timing of the bilinear build_P (AsymmertricSimilarity) on one GPU: one JSON line per workload.

Times, with HIP events after a warm-up (median of --reps): the MFMA projection alone (project_rows over the whole table),
the pair K1 alone (every block's one-(sub-)wave / long-row / class-row launches), the whole
SweepEngine.build_P_bilinear, and the cosine SweepEngine.build_P for scale.  At config 2 also the route the bilinear
similarity took before it had a path of its own: Graph.build_P's plug-in branch with a `batchwise` copy of the module,
whose forward runs on gathered Z[src] / Z[dst] chunks.
Usage: python tools/bilinear_build_p_time.py [--workloads rmat200k,rmat2m] [--reps 5]
"""
from __future__ import annotations

import argparse
import copy
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from clane_amd import _hip, synth  # noqa: E402
from clane_amd.engine import SweepEngine  # noqa: E402
from clane_amd.graph import Graph  # noqa: E402
from clane_amd.similarity import AsymmertricSimilarity  # noqa: E402

SHAPES = {"rmat200k": (200_000, 4_000_000, 128, 1, 2), "rmat2m": (2_000_000, 40_000_000, 256, 3, 4)}


def timed(fn, reps: int) -> float:
    """Median milliseconds of `fn` between two events on the current stream, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        z.synchronize()
        ts.append(a.elapsed_time(z))
    return sorted(ts)[len(ts) // 2]


def pair_k1(eng: SweepEngine):
    Y, d, k = eng._Y, eng.d, eng.k
    S, N = Y[:, :d], Y[:, d:2 * d]
    for i, b in enumerate(eng.blocks):
        rp = eng.rowptr[b.local_start:]
        k.edge_score_pair(rp, eng.colidx, b.nrows, b.row0, S, N, d, eng.P, eng.k1_threshold, eng.k1_long_rows[i],
                          fuse_softmax=True)
        if eng.class_k1 and eng.class_rows[i] is not None:
            rows_c, slot_ptr, it_e0, it_len, it_slot, it_row, ipb = eng.class_rows[i]
            k.edge_score_class_pair(rp, eng.colidx, it_e0, it_len, it_slot, it_row, ipb, rows_c, slot_ptr, b.row0, S, N,
                                    d, eng.P, eng.slabs[i % len(eng.slabs)], fuse_softmax=True,
                                    n_slots=eng.class_slots[i], row_parts=eng.softmax_row_parts)


class _PluginRoute:
    """What Graph.build_P did with the module before the bilinear path: a plug-in callable (not an AsymmertricSimilarity
    instance, so the plug-in branch takes it) that vouches for `batchwise` and runs the module's forward per chunk."""
    batchwise = True

    def __init__(self, module):
        self.module = module

    def __call__(self, z_src, z_dst):
        with torch.no_grad():
            return self.module(z_src, z_dst)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rmat200k,rmat2m")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = _hip.require_gpu("cuda:0")
    for name in args.workloads.split(","):
        V, E, d, gseed, xseed = SHAPES[name]
        csr = synth.rmat_csr(V, E, seed=gseed, device=str(dev))
        X = synth.gaussian_X(V, d, seed=xseed)
        torch.manual_seed(0)
        sim = AsymmertricSimilarity(d).to(dev)
        rec = {"workload": name, "V": V, "E": int(csr.num_edges), "d": d, "dtype": "f32", "reps": args.reps,
               "gpu": torch.cuda.get_device_name(dev)}
        with torch.cuda.device(dev):
            g = Graph.from_csr(csr, X)
            eng = g.engine(dev)
            W = sim.stacked_weight(torch.float32, dev)
            eng.build_P_bilinear(W)                           # allocates Y
            rows = eng.Zcur.shape[0]
            t_proj = timed(lambda: eng.k.project_rows(eng.Zcur, d, W, eng._Y), args.reps)
            rec["project_rows_ms"] = t_proj
            rec["project_rows_tflops"] = 2.0 * rows * d * 2 * d / (t_proj * 1e-3) / 1e12
            rec["project_rows_fraction_of_155tf"] = rec["project_rows_tflops"] / 155.0
            rec["pair_k1_ms"] = timed(lambda: pair_k1(eng), args.reps)
            rec["build_P_bilinear_ms"] = timed(lambda: eng.build_P_bilinear(sim.stacked_weight(torch.float32, dev)),
                                               args.reps)
            rec["build_P_cosine_ms"] = timed(eng.build_P, args.reps)
            rec["Y_bytes"] = eng._Y.numel() * eng._Y.element_size()
            if name == "rmat200k":
                old = _PluginRoute(copy.deepcopy(sim))         # the plug-in branch's chunked route
                rec["plugin_route_ms"] = timed(lambda: g.build_P(old), max(1, args.reps // 2))
                rec["graph_build_P_bilinear_ms"] = timed(lambda: g.build_P(sim), max(1, args.reps // 2))
                rec["speedup_engine_vs_plugin"] = rec["plugin_route_ms"] / rec["build_P_bilinear_ms"]
                rec["speedup_graph_vs_plugin"] = rec["plugin_route_ms"] / rec["graph_build_P_bilinear_ms"]
        print(json.dumps(rec), flush=True)
        del eng, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
