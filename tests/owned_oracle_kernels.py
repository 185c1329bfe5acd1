"""The CPU test double (tests/oracle_kernels.py) with the owned class pass: ``spmm_update_owned`` walked exactly as
include/clane_hip.h describes it -- groups, batches, steps, segments, pieces from zero, virtual rows in order -- while
checking the contract the kernel relies on.  Like its base it is only ever handed to an engine by a test."""
import numpy as np
import torch

from clane_amd._hip import OWNED_MAX_STEPS
from clane_amd.plan import lanes_per_row
from clane_amd.xcd import xcd_class

from .oracle_kernels import OracleKernels as _Base


class OracleKernels(_Base):
    def has_spmm_owned(self, dtype, d):
        return dtype in (torch.float32, torch.float64) and d > 0

    def make_owned_plan(self, plan, chunk, device):
        return dict(plan, chunk=int(chunk))

    def spmm_update_owned(self, colidx, P, plan, block_threads, row0, Z_old, X, gamma, Z_new, d, partials,
                          beyond_cache=False, loads=0):
        assert block_threads % 64 == 0 and 64 <= block_threads <= 1024 and plan["chunk"] % 64 == 0
        # the kernel's instances (csrc/clane_abi.hip): 6, 8 or 12 row loads in flight at 32 lanes per row, 8 or 12 at 64
        assert loads in (0, 8, 12) or (loads == 6 and lanes_per_row(d, Z_old.dtype) == 32), f"no instance with {loads} loads"
        assert 1 <= plan["n_steps"] <= OWNED_MAX_STEPS
        acc, S, chunk = P.dtype, plan["n_steps"], plan["chunk"]
        gb, bv, br, bs = (plan[k] for k in ("grp_bat_ptr", "bat_vrow_ptr", "bat_row_ptr", "bat_seg_ptr"))
        assert gb.size == plan["n_groups"] + 1 and gb[-1] == bv.size - 1 and S == plan["steps"].size
        written = set()
        for g in range(plan["n_groups"]):
            for b in range(gb[g], gb[g + 1]):
                nv = int(bv[b + 1] - bv[b])
                assert 0 < nv <= plan["max_batch_vrows"]
                sums = torch.zeros(nv, d, dtype=acc)
                for s in range(S):
                    seen = set()
                    for k in range(bs[b * S + s], bs[b * S + s + 1]):
                        e0, ln, v = int(plan["seg_e0"][k]), int(plan["seg_len"][k]), int(plan["seg_vrow"][k])
                        assert ln > 0 and 0 <= v < nv and v not in seen       # one segment per virtual row and step
                        seen.add(v)
                        cols = colidx[e0:e0 + ln].long()
                        assert bool((xcd_class(cols) == int(plan["steps"][s]) % 8).all()), "segment outside its step's class"
                        for p in range(e0, e0 + ln, chunk):                   # pieces from zero, added in order
                            q = min(p + chunk, e0 + ln)
                            sums[v] = sums[v] + (P[p:q].unsqueeze(1) * Z_old[colidx[p:q].long(), :d].to(acc)).sum(0)
                for j in range(br[b], br[b + 1]):
                    va, vb = int(plan["row_vptr"][j] - bv[b]), int(plan["row_vptr"][j + 1] - bv[b])
                    assert 0 <= va < vb <= nv
                    agg = sums[va].clone()
                    for v in range(va + 1, vb):
                        agg = agg + sums[v]
                    r = int(plan["row_id"][j])
                    own = Z_old[row0 + r, :d]
                    new = (X[r, :d].to(acc) + gamma * agg).to(Z_new.dtype)
                    Z_new[r, :d] = new
                    assert r not in written
                    written.add(r)
                    partials[int(plan["row_part"][j])] = float((new.to(acc) - own.to(acc)).abs().sum())
        assert len(written) == plan["row_id"].size
