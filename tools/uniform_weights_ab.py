#!/usr/bin/env python3
"""A/B of one weight per row (spmm_update*_rw, SweepEngine(uniform_weights=...)) against one weight per edge on ONE
engine's tables: the variants are switched with SweepEngine.set_uniform_weights() between timed blocks, alternating in
rounds, so both run on the same physical pages (the method of tools/fused_tiles_ab.py).  Per variant: sweep ms (median
over the rounds, min .. max) and the HIP-event times of the class pass and of the row pass (the median sweep of 24).  The
first sweep of every variant must be BITWISE the per-edge plan's.  Also the cost of the detection pass (row_weight_kernel),
which runs once per build_P.
Usage: tools/uniform_weights_ab.py [--workload rmat2m] [--rounds 3] [--steps 30] [--out FILE.md]"""
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

VARIANTS = {"per edge": False, "per row": True, "per edge (again)": False}

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="rmat2m")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--gamma", type=float, default=0.76)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = _hip.require_gpu("cuda:0")
gen, V, E, d, dt, gseed, xseed = WORKLOADS[args.workload]
make = {"rmat": synth.rmat_csr, "powerlaw": synth.powerlaw_csr, "uniform": synth.uniform_random_csr}[gen]
csr = make(V, E, seed=gseed, device=str(dev))
X = synth.gaussian_X(V, d, seed=xseed).to(DTYPES[dt])
names = list(VARIANTS)
eng = SweepEngine(csr, X, dev, uniform_weights="auto")
if not eng.uniform_possible:
    sys.exit(f"{args.workload}: the per-row-weight calls do not apply to this engine")
eng.build_P()
eng.sweep(args.gamma)
if not eng._uniform:
    sys.exit(f"{args.workload}: build_P left rows of P with different weights")


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


def timed_passes():
    eng.time_kernels, eng.kernel_events = True, []
    block(24)
    eng.time_kernels = False
    t = np.array([(e0.elapsed_time(e4), e2.elapsed_time(e3)) for _, e0, e1, e2, e3, e4 in eng.kernel_events])
    eng.kernel_events = []
    t = t.reshape(-1, len(eng.blocks), 2).sum(1)
    return {"split": float(np.median(t[:, 0])), "main": float(np.median(t[:, 1]))}


# the detection pass: HIP events around 20 runs of it, after one untimed
from clane_amd import uniform                                        # noqa: E402
uniform.scan(eng)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
ev[0].record()
for i in range(20):
    uniform.scan(eng)
    ev[i + 1].record()
torch.cuda.synchronize()
scan_us = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(20))
detection = {"row_weight_us_median": round(scan_us[10], 1), "min": round(scan_us[0], 1), "max": round(scan_us[-1], 1)}
print(json.dumps({"detection": detection}), flush=True)

info, ref = {}, None
for name in names:                              # results first: one sweep from the same start, bit for bit
    eng.set_uniform_weights(VARIANTS[name])
    eng.set_Z(X)
    eng.P_valid = True                          # P is untouched by set_Z; build_P ran on X
    delta = eng.sweep(args.gamma)
    assert bool(eng._uniform) == VARIANTS[name], name
    if ref is None:
        ref = (delta, eng.Zcur.clone(), eng.partials.clone())
    assert delta == ref[0] and torch.equal(eng.Zcur, ref[1]) and torch.equal(eng.partials, ref[2]), name
    info[name] = {"first_delta": delta, "bitwise_equal_to_first_variant": True}
runs = {n: [] for n in names}
split = {n: [] for n in names}


def switch(name):
    eng.set_uniform_weights(VARIANTS[name])
    eng.sweep(args.gamma)                       # reads the detection's answer outside the timed blocks


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
                      rounds={"sweep_ms": [round(x, 4) for x in ms], "class_pass_ms": [round(x, 4) for x in cp],
                              "row_pass_ms": [round(x, 4) for x in rp]})
    print(json.dumps({"variant": name, **info[name]}), flush=True)
lines = [f"# One weight per row A/B on {args.workload} (`tools/uniform_weights_ab.py`)", "",
         f"One engine, variants switched between blocks; {args.rounds} interleaved rounds after an untimed one, each the median of 3 "
         f"blocks of {args.steps} sweeps.  class pass / row pass: HIP events (the median of 24 sweeps), median (min .. max) over the "
         "rounds.  Every variant's first sweep is bitwise the per-edge plan's.  Detection pass (row_weight_kernel, once per "
         f"build_P): {detection['row_weight_us_median']} us (min {detection['min']}, max {detection['max']}).", "",
         "| variant | sweep ms (median) | min .. max | class pass ms | row pass ms |", "|---|---|---|---|---|"]
for name in names:
    v = info[name]
    lines.append(f"| {name} | {v['sweep_ms']:.4f} | {v['sweep_ms_min']:.4f} .. {v['sweep_ms_max']:.4f} | "
                 f"{v['class_pass_ms']:.4f} ({v['class_pass_min']:.4f} .. {v['class_pass_max']:.4f}) | "
                 f"{v['row_pass_ms']:.4f} ({v['row_pass_min']:.4f} .. {v['row_pass_max']:.4f}) |")
a, b = info[names[0]], info[names[1]]
spread = max(info[n]["sweep_ms_max"] - info[n]["sweep_ms_min"] for n in names)
lines += ["", f"Gain {a['sweep_ms'] - b['sweep_ms']:.4f} ms per sweep; three times the largest max - min of a variant's rounds: "
          f"{3 * spread:.4f} ms."]
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
print("\n".join(lines))
