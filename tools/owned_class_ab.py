#!/usr/bin/env python3
"""A/B of the owned class pass (spmm_owned_kernel) against chunk + combine on ONE engine's tables: the variants are
switched with SweepEngine.set_owned() between timed blocks, alternating in rounds (A B C ... A B C ...), so every
variant runs on the same physical pages and nothing is released in between (the method of
tools/threshold_robustness.py).  Per variant: sweep ms (median over the rounds, min .. max), the HIP-event time of the
class pass ("split" bucket: owned kernel + chunk + combine of the rows above owned_max_edges), the plan's shape and
how evenly its steps are dealt.  The first sweep of every variant is checked against the chunk + combine result.
Usage: tools/owned_class_ab.py [--workload rmat2m] [--rounds 3] [--steps 30] [--variants NAME,...] [--out FILE.md]"""
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

VARIANTS = {     # name: settings of set_owned (None: chunk + combine, the parent's class pass)
    "chunk+combine": None,
    "owned default": {},
    "owned 512x768": {"groups": 512, "block_threads": 768, "lds_bytes": 72 * 1024},
    "owned 512x512": {"groups": 512, "block_threads": 512, "lds_bytes": 72 * 1024},
    "owned 256x1024": {"groups": 256, "block_threads": 1024, "lds_bytes": 144 * 1024},
    "owned 256x1024 loads 8": {"groups": 256, "block_threads": 1024, "lds_bytes": 144 * 1024, "loads": 8},
    "owned 256x1024 loads 12": {"groups": 256, "block_threads": 1024, "lds_bytes": 144 * 1024, "loads": 12},
    "owned 256x1024 H=512": {"groups": 256, "block_threads": 1024, "lds_bytes": 152 * 1024, "max_edges": 512},
    "owned 256x1024 H=512 loads 12": {"groups": 256, "block_threads": 1024, "lds_bytes": 152 * 1024, "max_edges": 512,
                                      "loads": 12},
    "owned 256x768 H=512": {"groups": 256, "block_threads": 768, "lds_bytes": 152 * 1024, "max_edges": 512},
    "owned 256x1024 H=256": {"groups": 256, "block_threads": 1024, "lds_bytes": 152 * 1024, "max_edges": 256},
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
eng = SweepEngine(csr, X, dev, class_owned=False)
if not eng.owned_possible:
    sys.exit(f"{args.workload}: this engine has no owned pass")
eng.build_P()
defaults = dict(max_edges=eng.owned_max_edges, row_edges=eng.owned_row_edges, groups=eng.owned_groups,
                block_threads=eng.owned_block_threads, chunk=eng.owned_chunk, lds_bytes=eng._lds_bytes,
                loads=eng.owned_loads)


def switch(name):
    kw = VARIANTS[name]
    eng.set_owned(kw is not None, **dict(defaults, **(kw or {})))


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
for name in names:                              # results first: one sweep from the same start
    eng.set_Z(X)
    eng.P_valid = True                          # P is untouched by set_Z; build_P ran on X
    switch(name)
    delta = eng.sweep(args.gamma)
    Z1 = eng.Zcur.clone()
    if ref is None:
        ref = (delta, Z1)
    err = float((Z1.double() - ref[1].double()).norm() / ref[1].double().norm())
    assert err < 2e-6 and abs(delta - ref[0]) <= 1e-5 * ref[0], (name, err, delta, ref[0])
    info[name] = {"first_sweep_rel_l2_vs_first_variant": err, "first_delta": delta}
    if eng.class_owned:
        plan, rest, n_rest = next(o for o in eng.owned_rows if o is not None)
        steps = eng.owned_balance.astype(np.float64)
        cum = np.cumsum(steps, 1)
        info[name].update(owned_rows=plan.n_rows, rows_above=n_rest, steps=plan.n_steps,
                          batches=int(plan.arrays["bat_vrow_ptr"].numel() - 1), max_batch_vrows=plan.max_batch_vrows,
                          virtual_rows=int(plan.arrays["row_vptr"][-1]), segments=int(plan.arrays["seg_len"].numel()),
                          step_edges_rel_std=float((steps.std(0) / np.maximum(steps.mean(0), 1)).max()),
                          drift_in_steps=float(((cum.max(0) - cum.min(0)) / np.maximum(steps.mean(0), 1)).max()))
    del Z1
runs = {n: [] for n in names}
split = {n: [] for n in names}
for rnd in range(args.rounds):
    for name in names:
        switch(name)
        block(5)
        runs[name].append(float(np.median([block(args.steps) for _ in range(3)])))
        eng.time_kernels, eng.kernel_events = True, []
        block(8)
        eng.time_kernels = False
        split[name].append(eng.kernel_times_ms())
for name in names:
    ms = runs[name]
    info[name].update(sweep_ms=round(float(np.median(ms)), 4), sweep_ms_min=round(min(ms), 4), sweep_ms_max=round(max(ms), 4),
                      class_pass_ms=round(float(np.median([s["split"] for s in split[name]])), 4),
                      row_pass_ms=round(float(np.median([s["main"] for s in split[name]])), 4),
                      settings=VARIANTS[name])
    print(json.dumps({"variant": name, **info[name]}), flush=True)
lines = [f"# Owned class pass A/B on {args.workload} (`tools/owned_class_ab.py`)", "",
         f"One engine, variants switched between blocks; {args.rounds} interleaved rounds, each the median of 3 blocks of "
         f"{args.steps} sweeps.  class pass / row pass: HIP events per sweep (both column tiles).", "",
         "| variant | sweep ms (median) | min .. max | class pass ms | row pass ms | owned rows | above H | batches | segments | "
         "step std | drift (steps) |", "|---|---|---|---|---|---|---|---|---|---|---|"]
for name in names:
    v = info[name]
    lines.append(f"| {name} | {v['sweep_ms']:.3f} | {v['sweep_ms_min']:.3f} .. {v['sweep_ms_max']:.3f} | {v['class_pass_ms']:.3f} | "
                 f"{v['row_pass_ms']:.3f} | {v.get('owned_rows', '')} | {v.get('rows_above', '')} | {v.get('batches', '')} | "
                 f"{v.get('segments', '')} | {v.get('step_edges_rel_std', float('nan')):.3f} | "
                 f"{v.get('drift_in_steps', float('nan')):.2f} |")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
print("\n".join(lines))
