"""build_P of the bilinear similarity (AsymmertricSimilarity, reference similarity.py:40-57 + graph.py:118-128) on a
SweepEngine: one row projection on the matrix cores (``project_rows``), then the pair K1 with its fused softmax
(``edge_score_pair`` / ``edge_score_class_pair``) over the engine's blocks, long rows and class rows.  These three calls
are the kernel backend's optional ones (``KernelBackend`` gives them a body that raises): a backend without them still
serves every other path."""
from __future__ import annotations

import torch

from . import _hip
from .plan import _round_up


def project_table(eng, W: torch.Tensor):
    """Y = Z W^T for EVERY row of ``eng``'s current table, into the engine's kept ``_Y`` buffer (allocated by the first
    call): returns (Y[:, :d], Y[:, d:2d]) = (Phi_src z, Phi_dst z) per table row.  ``build_P_bilinear`` scores the edges
    from them, ``LinkRanker`` (links.py) every pair."""
    if eng.columns:
        raise NotImplementedError(
            f"the bilinear similarity needs whole rows of Z; this engine divides the COLUMNS over the GPUs "
            f"(exchange={eng.exchange!r}). Build the graph's engine with a row division first: "
            f"graph.engine(exchange='halo') (or 'allgather' / 'allgather_all'), CLI --exchange halo")
    d = eng.d
    if tuple(W.shape) != (2 * d, d):
        raise ValueError(f"build_P_bilinear: W must be [2d, d] = [{2 * d}, {d}], got {tuple(W.shape)}")
    W = W.detach().to(eng.device, eng.acc_dtype).contiguous()
    eng._sync_quiet_rows()              # every table row is projected: the other ranks' quiet rows too
    Z = eng.Zcur
    if eng._Y is None:
        eng._Y = torch.empty(Z.shape[0], _round_up(2 * d, _hip.VEC_ELEMS[eng.acc_dtype]), dtype=eng.acc_dtype,
                             device=eng.device)
    Y = eng._Y
    eng.k.project_rows(Z, d, W, Y)
    return Y[:, :d], Y[:, d:2 * d]


def build_P_bilinear(eng, W: torch.Tensor) -> None:
    """``SweepEngine.build_P_bilinear``: P of the rows ``eng`` owns, from W = cat(Phi_src.weight, Phi_dst.weight)."""
    S, N = project_table(eng, W)
    d, kern = eng.d, eng.k
    if eng.E_loc > 0:
        for i, (b, rows) in enumerate(zip(eng.blocks, eng.block_rows)):
            rp = eng.rowptr[b.local_start:]
            kern.edge_score_pair(rp, eng.colidx, b.nrows, b.row0, S, N, d, eng.P, eng.k1_threshold,
                                 rows.k1_long, fuse_softmax=True)
            if eng.class_k1 and rows.klass is not None:
                it = rows.klass
                kern.edge_score_class_pair(rp, eng.colidx, it.e0, it.len, it.slot, it.row, it.items_per_block, it.rows,
                                           it.slot_ptr, b.row0, S, N, d, eng.P, eng.slabs[i % len(eng.slabs)],
                                           fuse_softmax=True, n_slots=rows.n_slots, row_parts=eng.softmax_row_parts)
    eng.P_valid = True
