#!/usr/bin/env python3
"""A/B of the fused column-tile launches (spmm_update*_tiles: one launch per pass for all tiles) and of the owned
epilogue's look-ahead against the per-tile plan on ONE engine's tables: the variants are switched with
SweepEngine.set_fused_tiles() between timed blocks, alternating in rounds (A B C ... A B C ...), so every variant runs on
the same physical pages (the method of tools/owned_class_ab.py).  Each of the four pieces -- row pass, chunk + combine,
owned pass, look-ahead -- is switched on its own, then all together.  Per variant: sweep ms (median over the rounds,
min .. max) and the HIP-event times of the class pass and of the row pass.  The first sweep of every variant must be
BITWISE the per-tile plan's.
Usage: tools/fused_tiles_ab.py [--workload rmat2m] [--rounds 3] [--steps 30] [--variants NAME,...] [--out FILE.md]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from benchkit.common import DTYPES, WORKLOADS                       # noqa: E402
from clane_amd import _hip, synth                                    # noqa: E402
from clane_amd.engine import SweepEngine                             # noqa: E402

VARIANTS = {     # name: (fused passes, look-ahead)
    "per tile": ((), False),
    "row": (("row",), False),
    "class": (("class",), False),
    "owned": (("owned",), False),
    "ahead": ((), True),
    "owned+ahead": (("owned",), True),
    "all": (("row", "class", "owned"), True),
    "all, no ahead": (("row", "class", "owned"), False),
    "per tile (again)": ((), False),        # the baseline a second time per round: what the box alone moves
}

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="rmat2m")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--gamma", type=float, default=0.76)
ap.add_argument("--variants", default=None, help="comma-separated names out of: " + ", ".join(VARIANTS))
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = _hip.require_gpu("cuda:0")
gen, V, E, d, dt, gseed, xseed = WORKLOADS[args.workload]
make = {"rmat": synth.rmat_csr, "powerlaw": synth.powerlaw_csr, "uniform": synth.uniform_random_csr}[gen]
csr = make(V, E, seed=gseed, device=str(dev))
X = synth.gaussian_X(V, d, seed=xseed).to(DTYPES[dt])
names = list(VARIANTS) if args.variants is None else args.variants.split(",")
eng = SweepEngine(csr, X, dev, fused_tiles=False, owned_ahead=False)
if not eng.fused_possible:
    sys.exit(f"{args.workload}: the fused calls do not apply to this engine (tiles {eng.tiles})")
eng.build_P()


def switch(name):
    passes, ahead = VARIANTS[name]
    eng.set_fused_tiles(passes, ahead=ahead)


def block(steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ticket = eng.sweep_launch(args.gamma)
    for _ in range(steps - 1):
        following = eng.sweep_launch(args.gamma)
        eng.sweep_wait(ticket)
        ticket = following
    eng.sweep_wait(ticket)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


info, ref = {}, None
for name in names:                              # results first: one sweep from the same start, bit for bit
    eng.set_Z(X)
    eng.P_valid = True                          # P is untouched by set_Z; build_P ran on X
    switch(name)
    delta = eng.sweep(args.gamma)
    if ref is None:
        ref = (delta, eng.Zcur.clone(), eng.partials.clone())
    assert delta == ref[0] and torch.equal(eng.Zcur, ref[1]) and torch.equal(eng.partials, ref[2]), name
    info[name] = {"first_delta": delta, "bitwise_equal_to_first_variant": True}
runs = {n: [] for n in names}
split = {n: [] for n in names}


def timed_passes():
    """HIP-event times of the class pass (marks 0 -> 4) and the row pass (2 -> 3) over 24 sweeps
    (SweepEngine.MAX_TIMED_SWEEPS allows 32): the MEDIAN sweep, not kernel_times_ms()'s mean -- in three runs of this tool
    one round's mean read a pass 0.02-0.11 ms high (a late sweep among the timed ones), more than any piece here gains
    (profiles/r16_fused_tiles.md)."""
    eng.time_kernels, eng.kernel_events = True, []
    block(24)
    eng.time_kernels = False
    t = np.array([(e0.elapsed_time(e4), e2.elapsed_time(e3)) for _, e0, e1, e2, e3, e4 in eng.kernel_events])
    eng.kernel_events = []
    t = t.reshape(-1, len(eng.blocks), 2).sum(1)
    return {"split": float(np.median(t[:, 0])), "main": float(np.median(t[:, 1]))}


for name in names:      # one untimed round, events included: the first blocks and the first events of a process
    switch(name)
    block(args.steps)
    timed_passes()
for rnd in range(args.rounds):
    for name in names:
        switch(name)
        block(5)
        runs[name].append(float(np.median([block(args.steps) for _ in range(3)])))
        split[name].append(timed_passes())
for name in names:
    ms = runs[name]
    cp, rp = [s["split"] for s in split[name]], [s["main"] for s in split[name]]
    info[name].update(sweep_ms=round(float(np.median(ms)), 4), sweep_ms_min=round(min(ms), 4), sweep_ms_max=round(max(ms), 4),
                      class_pass_ms=round(float(np.median(cp)), 4), class_pass_min=round(min(cp), 4),
                      class_pass_max=round(max(cp), 4), row_pass_ms=round(float(np.median(rp)), 4),
                      row_pass_min=round(min(rp), 4), row_pass_max=round(max(rp), 4),
                      fused=list(VARIANTS[name][0]), ahead=VARIANTS[name][1],
                      rounds={"sweep_ms": [round(x, 4) for x in ms], "class_pass_ms": [round(x, 4) for x in cp],
                              "row_pass_ms": [round(x, 4) for x in rp]})
    print(json.dumps({"variant": name, **info[name]}), flush=True)
lines = [f"# Fused column tiles A/B on {args.workload} (`tools/fused_tiles_ab.py`)", "",
         f"One engine, variants switched between blocks; {args.rounds} interleaved rounds after an untimed one, each the median of 3 "
         f"blocks of {args.steps} sweeps.  class pass / row pass: HIP events (all column tiles; the median of 24 sweeps), median (min .. max) "
         "over the rounds.  Every variant's first sweep is bitwise the per-tile plan's.", "",
         "| variant | sweep ms (median) | min .. max | class pass ms | row pass ms |", "|---|---|---|---|---|"]
for name in names:
    v = info[name]
    lines.append(f"| {name} | {v['sweep_ms']:.4f} | {v['sweep_ms_min']:.4f} .. {v['sweep_ms_max']:.4f} | "
                 f"{v['class_pass_ms']:.4f} ({v['class_pass_min']:.4f} .. {v['class_pass_max']:.4f}) | "
                 f"{v['row_pass_ms']:.4f} ({v['row_pass_min']:.4f} .. {v['row_pass_max']:.4f}) |")
# each piece against the per-tile plan on its OWN pass's HIP-event time: the gain must exceed three times the larger
# max - min of the two variants' rounds
base = names[0]
lines += ["", f"| piece | pass | {base} ms | with the piece | gain | 3 x the larger max - min | clears the bar |", "|---|---|---|---|---|---|---|"]
for name in [n for n in names[1:] if VARIANTS[n] != VARIANTS[base]]:
    for key, label in (("row_pass", "row"), ("class_pass", "class")):
        if (label == "row") != (VARIANTS[name][0] == ("row",)) and name not in ("all", "all, no ahead"):
            continue
        a, b = info[base], info[name]
        gain = a[key + "_ms"] - b[key + "_ms"]
        bar = 3 * max(a[key + "_max"] - a[key + "_min"], b[key + "_max"] - b[key + "_min"])
        lines.append(f"| {name} | {label} | {a[key + '_ms']:.4f} | {b[key + '_ms']:.4f} | {gain:.4f} | {bar:.4f} | "
                     f"{'yes' if gain > bar else 'no'} |")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
print("\n".join(lines))
