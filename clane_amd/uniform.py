"""One weight per row instead of one per edge (csrc/spmm_update.h UNIFORM, csrc/build_p.h row_weight_kernel; the
reference's loop reads P per edge for every row alike, embedder.py:84-92): which engines can take it, the pass that looks
at the rows of P, the answer.  ``has_row_weight`` / ``row_weight`` and the ``spmm_update*_rw`` calls are the kernel
backend's optional calls (``KernelBackend`` gives them a body that says no): a backend without them keeps one weight per
edge.  The binders that pick the ``_rw`` calls are in fused.py and owned.py."""
from __future__ import annotations

import torch


def possible(eng) -> bool:
    """One GPU (no mirrored launches), fp32 tables, something to compute, and a backend that has the calls."""
    return bool(eng.world == 1 and not eng._forced and eng.dtype == torch.float32 and eng.d > 0
                and eng.k.has_row_weight(eng.dtype))


def scan(eng) -> None:
    """One pass over P: the rows' first weights into `eng.row_w`, and on the device (`eng._w_mixed`) whether any row holds
    two different floats.  Nothing is read back here."""
    if getattr(eng, "row_w", None) is None:
        eng.row_w = torch.zeros(eng.part.n_local, dtype=eng.acc_dtype, device=eng.device)
        eng._w_mixed = torch.zeros(1, dtype=torch.int32, device=eng.device)
    eng.k.row_weight(eng.rowptr, eng.P, eng.part.n_local, eng.row_w, eng._w_mixed)


def resolve(eng) -> bool:
    """Whether the sweeps of the current P read one weight per row: the pass over P and 4 bytes read back, once per P,
    when the first sweep on that P (or kernel_config()) asks.  Pass and read-back go to the stream that is current THEN --
    the sweep's own, on which the bound calls read `row_w` -- and, like the sweep's reads of P itself, they rely on
    whatever wrote P having been queued on that stream or finished."""
    if eng.uniform_weights is False or eng.E_loc == 0:
        return False
    scan(eng)
    uniform = int(eng._w_mixed.item()) == 0
    if eng.uniform_weights is True and not uniform:
        raise ValueError("uniform_weights=True, but a row of P holds different weights")
    return uniform
