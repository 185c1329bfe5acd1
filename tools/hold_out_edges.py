#!/usr/bin/env python3
"""Hold a random part of a graph's edges out for link evaluation (host only).

Writes to OUT_ROOT a copy of DATA_ROOT (``V``, ``C.npy`` / ``C.pt``) whose ``E`` lacks a seeded Bernoulli(--fraction)
sample of the edges, and the sample as ``held_out.tsv`` -- what the ``link_evaluation`` section of a config names as
``pairs``.  A vertex never loses its last out-edge.  Usage: python tools/hold_out_edges.py DATA_ROOT OUT_ROOT --fraction 0.1 --seed 0
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from clane_amd.links import hold_out_edges  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("data_root", type=Path)
    ap.add_argument("out_root", type=Path)
    ap.add_argument("--fraction", type=float, default=0.1, help="share of the distinct edges to hold out, in [0, 1)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    kept, held = hold_out_edges(args.data_root, args.out_root, args.fraction, args.seed)
    print(f"{kept} edges kept in {args.out_root / 'E'}, {held} held out in {args.out_root / 'held_out.tsv'}")


if __name__ == "__main__":
    main()
