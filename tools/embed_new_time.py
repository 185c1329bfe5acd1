#!/usr/bin/env python3
"""Times the embedding of new vertices (csrc/new_rows.h, clane_amd/induct.py) on one MI355X, beside what the project
offered before: rebuilding the engine on the augmented graph and iterating all of it again.

    python tools/embed_new_time.py [--shapes config2 config3] [--repeats 7] [--skip-rebuild] > profiles/r14_embed_new.md

Per shape (config 2's table: rmat 200k x 128 fp32; config 3's: rmat 2M x 256 fp32; per-edge cosine) the batch is 100 000
new rows of 20 distinct random neighbours each, seeded.  The table is first brought to its own fixed point
(Embedder.iterate), so that the arrivals see a finished graph.  Reported:
  * clane_embed_rows_f32: device-event time per launch -- median, min and max of `--repeats` launches after 2 warm-up
    launches -- mean / max rounds, rows not converged, and the bytes the launch gathers computed from the shapes
    (sum over rows of rounds x degree x row bytes) with the rate that makes;
  * prepare(): K0 where needed (the one pass over the table a batch costs besides the launch);
  * the rebuild route: engine construction on the augmented graph + set_Z(old Z, x for the arrivals) + iterate(), in
    seconds of wall time, the rel_l2 drift of the OLD rows it causes and the rel_l2 between its new rows and
    embed_rows' (the two agree where nobody links to the arrivals and the old rows were at their fixed point).
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
SHAPES = {"config2": (200_000, 4_000_000, 128, 1, 2), "config3": (2_000_000, 40_000_000, 256, 3, 4),
          "small": (20_000, 200_000, 64, 7, 8)}                      # V, E, d, graph seed, X seed
NEW_ROWS, NEW_DEGREE, GAMMA, TOLERENCE, MAX_ROUNDS = 100_000, 20, 0.76, 10, 64


def one(name: str, repeats: int, skip_rebuild: bool) -> None:
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from clane_amd import _hip, synth
    from clane_amd.embedder import Embedder
    from clane_amd.graph import Graph
    from clane_amd.induct import NewVertexEmbedder
    from clane_amd.partition import HostCSR
    from clane_amd.similarity import CosineSimilarity

    V, E, d, gseed, xseed = SHAPES[name]
    m = NEW_ROWS if name != "small" else 5_000
    dev = _hip.require_gpu("cuda:0")
    sim = CosineSimilarity(mode="per_edge")
    csr = synth.rmat_csr(V, E, seed=gseed, device=str(dev))
    X = synth.gaussian_X(V, d, seed=xseed)
    rng = np.random.default_rng(99)
    # 20 distinct neighbours per arrival: sorted uniform draws, a repeat redrawn by shifting (no repeats at V >> 20)
    cols = np.sort(rng.integers(0, V, size=(m, NEW_DEGREE)), axis=1)
    for _ in range(4):
        rep = np.zeros_like(cols, dtype=bool)
        rep[:, 1:] = cols[:, 1:] == cols[:, :-1]
        cols[rep] = (cols[rep] + rng.integers(1, V, size=int(rep.sum()))) % V
        cols = np.sort(cols, axis=1)
    rowptr = np.arange(m + 1, dtype=np.int64) * NEW_DEGREE
    X_new = torch.from_numpy(rng.standard_normal((m, d), dtype=np.float32))

    g = Graph.from_csr(csr, X)
    t0 = time.perf_counter()
    emb = Embedder(graph=g, similarity_measure=sim, device=dev, gamma=GAMMA, tolerence=TOLERENCE, verbose=False)
    emb.iterate()
    torch.cuda.synchronize()
    t_first = time.perf_counter() - t0
    eng = g.engine(cosine_mode="per_edge")
    Z_old = eng.get_Z()
    with torch.cuda.device(dev):
        nv = NewVertexEmbedder(eng, sim)
        eng.sq_ok[eng.cur] = False
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        nv.prepare()
        ev[1].record()
        torch.cuda.synchronize()
        t_prepare = ev[0].elapsed_time(ev[1])
        res = nv.embed(X_new, rowptr, cols.reshape(-1), GAMMA, TOLERENCE, MAX_ROUNDS, refresh=False)
        # the launch alone, on the arrays embed() hands it
        rp = res.rowptr
        ci = eng.pos[res.cols].to(torch.int32).contiguous()
        Xd = torch.zeros(m, eng.ld, dtype=eng.dtype, device=dev)
        Xd[:, :d] = X_new.to(dev)
        Zo, rounds = torch.zeros_like(Xd), torch.zeros(m, dtype=torch.int32, device=dev)
        delta = torch.zeros(m, dtype=eng.acc_dtype, device=dev)
        times = []
        for i in range(2 + repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.k.embed_rows(rp, ci, Xd, eng.Zcur, int(eng.Zcur.shape[0]), d, _hip.SCORE_PER_EDGE, None, nv.sq, None,
                             GAMMA, TOLERENCE, MAX_ROUNDS, Zo, rounds, delta)
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                times.append(a.elapsed_time(b))
        assert torch.equal(Zo[:, :d], res.Z) and torch.equal(rounds, res.rounds)
    r = res.rounds.double()
    row_bytes = d * X.element_size()
    gathered = float((r * NEW_DEGREE).sum()) * row_bytes
    med = statistics.median(times)
    print(f"| {name} | {V} x {d} | {m} x {NEW_DEGREE} | {med:.3f} | {min(times):.3f} | {max(times):.3f} | "
          f"{float(r.mean()):.2f} | {int(r.max())} | {int((~res.converged).sum())} | {gathered / 1e9:.2f} | "
          f"{gathered / (med * 1e-3) / 1e12:.2f} | {m * NEW_DEGREE * row_bytes / 1e9:.2f} | {t_prepare:.3f} |", flush=True)
    print(f"<!-- {name}: first iterate() of the table {t_first:.2f} s -->", flush=True)
    if skip_rebuild:
        return
    # what the project offered before: the augmented graph, all of it, again
    Z_new_rows = res.Z.cpu()
    del g, eng, nv, emb
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    aug = HostCSR(V + m, np.concatenate([csr.rowptr, csr.rowptr[-1] + rowptr[1:]]),
                  np.concatenate([csr.colidx, cols.reshape(-1).astype(np.int32)]))
    g2 = Graph.from_csr(aug, torch.cat([X, X_new]))
    g2.set_Z(torch.cat([Z_old, X_new]))
    emb2 = Embedder(graph=g2, similarity_measure=sim, device=dev, gamma=GAMMA, tolerence=TOLERENCE, verbose=False)
    emb2.iterate()
    torch.cuda.synchronize()
    t_rebuild = time.perf_counter() - t0
    Z2 = g2.Z
    drift = float((Z2[:V].double() - Z_old.double()).norm() / Z_old.double().norm())
    agree = float((Z2[V:].double() - Z_new_rows.double()).norm() / Z_new_rows.double().norm())
    print(f"| {name} rebuild + iterate() | {t_rebuild:.2f} s | old rows drift rel_l2 {drift:.3e} | new rows vs embed_rows "
          f"rel_l2 {agree:.3e} |", flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["config2", "config3"], choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-rebuild", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:
        one(args.one, args.repeats, args.skip_rebuild)
        return 0
    print("# Embedding new vertices: clane_embed_rows_f32 against rebuild + iterate()\n")
    print("| shape | table | batch | ms / launch (median) | min | max | mean rounds | max rounds | not converged | "
          "GB gathered (from shapes) | TB/s | GB compulsory | prepare() ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for name in args.shapes:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--one", name, "--repeats", str(args.repeats)]
        if args.skip_rebuild:
            cmd.append("--skip-rebuild")
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"\n{name}: no result within {args.step_timeout} s; nothing more is started", flush=True)
            return 1
        if rc != 0:
            print(f"\n{name}: exit status {rc}; nothing more is started", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
