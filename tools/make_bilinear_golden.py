#!/usr/bin/env python3
"""Generate tests/golden/g13_karate_asym_d16.npz by running the REAL reference with its AsymmertricSimilarity.

TEST INFRASTRUCTURE, like oracle/make_goldens.py: runs only where the reference is mounted read-only at /root/reference
and never travels to the GPU box; only the resulting arrays are committed.  Karate (the V / E of g2_karate_csr.npz,
i.e. the reference's tests/data_root), embedding_dim = 16, seeded X and a seeded AsymmertricSimilarity(16).  Records the
two weight matrices, A's indices, the reference's ``graph.build_P(sim)`` values and the Z that
``Embedder(graph, sim, 'cpu').iterate()`` ends at, with its per-round sweep counts.

The reference needs one in-process alias to import under NumPy 2 (``from numpy import Inf`` at clane/embedder.py:1).
Usage: python tools/make_bilinear_golden.py
"""
from __future__ import annotations

import contextlib
import io
import sys
import tempfile
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "g13_karate_asym_d16.npz"
D, X_SEED, PHI_SEED, GAMMA, TOL = 16, 13, 7, 0.76, 10


def main() -> None:
    import torch
    np.Inf = np.inf  # noqa: NPY201 -- alias the reference needs (embedder.py:1)
    sys.path.insert(0, str(REF))
    import clane.embedder as E
    import clane.graph as G
    import clane.similarity as S

    karate = np.load(OUT.parent / "g2_karate_csr.npz", allow_pickle=True)
    root = Path(tempfile.mkdtemp(prefix="clane_bilinear_gold_"))
    (root / "V").write_text("\n".join(str(v) for v in karate["vertex_ids"]) + "\n")
    (root / "E").write_text("\n".join(f"{s}\t{d}" for s, d in zip(karate["edge_src"], karate["edge_dst"])) + "\n")
    X = torch.normal(0, 1, [len(karate["vertex_ids"]), D], generator=torch.Generator().manual_seed(X_SEED))
    np.save(root / "C.npy", X.numpy())

    torch.manual_seed(PHI_SEED)                       # xavier_normal_ draws from the global generator
    sim = S.AsymmertricSimilarity(D)
    g = G.Graph(root, embedding_dim=D)
    with torch.no_grad():
        P = g.build_P(sim)
    emb = E.Embedder(g, sim, torch.device("cpu"), gamma=GAMMA, tolerence=TOL, save_history=True)
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        emb.iterate()
    np.savez_compressed(
        OUT,
        X=X.numpy(),
        Phi_src=sim.Phi_src.weight.detach().numpy(),
        Phi_dst=sim.Phi_dst.weight.detach().numpy(),
        A_indices=g.A.indices().numpy(),
        P_values=P.values().detach().numpy(),
        Z_final=g.Z.numpy(),
        sweep_counts=np.array([len(h) for h in emb.history["Z"]]),
        gamma=np.float64(GAMMA), tolerence=np.int64(TOL),
    )
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): {len(emb.history['Z'])} rounds, sweeps {[len(h) for h in emb.history['Z']]}")


if __name__ == "__main__":
    main()
