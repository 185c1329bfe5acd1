"""ctypes binding of ``libclane_hip.so`` (C ABI: ``include/clane_hip.h``).

This is the only door between the Python host code and the gfx950 kernels.  There is no
CPU implementation behind it: if the library is missing or a call fails, it raises.

``HipKernels`` exposes one method per ABI entry point, taking torch tensors (device memory
is owned by torch -- plumbing only) and picking the ``_f32`` / ``_f64`` / ``_bf16`` symbol
from the tensor dtype.  Work is enqueued on torch's current HIP stream.
"""
from __future__ import annotations

import abc
import ctypes as C
import os
import threading
from pathlib import Path
from typing import Optional

import torch

LIB_NAME = "libclane_hip.so"
LIB_PATH = Path(__file__).resolve().parent / LIB_NAME
ABI_VERSION = 5

SCORE_REFERENCE, SCORE_PER_EDGE, SCORE_RAW_DOT = 0, 1, 2
SPMM_SINKS_UNTOUCHED = 1
SPMM_TABLE_BEYOND_CACHE = 2
OWNED_EPILOGUE_AHEAD = 1 << 16      # CLANE_OWNED_EPILOGUE_AHEAD
SCORE_FUSE_SOFTMAX = 1
SCORE_MODES = {"reference": SCORE_REFERENCE, "per_edge": SCORE_PER_EDGE, "raw_dot": SCORE_RAW_DOT}

_p, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# symbol -> (restype, argtypes); every symbol include/clane_hip.h declares.
SIGNATURES = {
    "clane_abi_version": (C.c_int, []),
    "clane_last_error": (C.c_char_p, []),
    "clane_build_info": (C.c_char_p, []),
    "clane_xcc_ids": (C.c_int, [_p, _i64, _i32, _p]),
    "clane_check_csr": (C.c_int, [_p, _p, _i64, _i64, _i64, _p, _p]),
    "clane_spmm_partials_len": (_i64, [_i64, _i64]),
    "clane_reduce_ws_len": (_i64, []),
    "clane_reduce_partials": (C.c_int, [_p, _i64, _p, _p, _p]),
    "clane_spmm_split_slab_len": (_i64, [_i64, _i32]),
    "clane_spmm_class_slab_len": (_i64, [_i64, _i32]),
    "clane_device_alloc": (C.c_int, [_i64, C.POINTER(_p)]),
    "clane_device_alloc_contiguous": (C.c_int, [_i64, C.POINTER(_p)]),
    "clane_device_free": (C.c_int, [_p]),
    "clane_ipc_export": (C.c_int, [_p, _p]),
    "clane_ipc_open": (C.c_int, [_p, C.POINTER(_p)]),
    "clane_ipc_close": (C.c_int, [_p]),
}
IPC_HANDLE_BYTES = 64
for _s in ("f32", "f64", "bf16"):
    SIGNATURES[f"clane_row_sqnorm_{_s}"] = (C.c_int, [_p, _i64, _i32, _i64, _p, _p])
    SIGNATURES[f"clane_edge_score_{_s}"] = (
        C.c_int, [_p, _p, _i64, _i64, _p, _i64, _i32, _i32, _p, _p, _p, _i32, _i64, _p, _i64, _p])
    _g = C.c_double if _s == "f64" else C.c_float
    SIGNATURES[f"clane_spmm_update_{_s}"] = (
        C.c_int, [_p, _p, _p, _i64, _i64, _p, _i64, _p, _i64, _g, _p, _i64, _i32, _i64, _i32, _p, _p, _p])
    SIGNATURES[f"clane_spmm_update_long_{_s}"] = (
        C.c_int, [_p, _p, _p, _p, _i64, _i32, _i64, _p, _i64, _p, _i64, _g, _p, _i64, _i32, _p, _p, _p])
    SIGNATURES[f"clane_spmm_update_split_{_s}"] = (
        C.c_int,
        [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p, _i64, _p, _i64, _g, _p, _i64, _i32, _p, _p, _p, _p])
    SIGNATURES[f"clane_spmm_update_class_{_s}"] = (
        C.c_int,
        [_p, _p, _p, _p, _p, _i64, _i32, _p, _p, _i64, _i64, _p, _i64, _p, _i64, _g, _p, _i64, _i32, _i32, _p, _p, _p, _p])
    SIGNATURES[f"clane_edge_score_class_{_s}"] = (
        C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _p, _p, _i64, _i64, _p, _i64, _i32, _i32, _p, _p, _p, _i32, _p, _p])
    SIGNATURES[f"clane_gather_rows_{_s}"] = (C.c_int, [_p, _i64, _p, _i64, _i32, _p, _i64, _p])
    SIGNATURES[f"clane_l1_distance_{_s}"] = (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p, _p])
SIGNATURES["clane_spmm_update_owned_f32"] = (
    C.c_int, [_p, _p, _p, _i32, _i64, _p, _i64, _p, _i64, C.c_float, _p, _i64, _i32, _i32, _p, _p])
# every column tile of a K3 pass in one launch (csrc/spmm_update.h, the *_tiles_kernel forms)
SIGNATURES["clane_spmm_update_tiles_f32"] = (
    C.c_int, [_p, _p, _p, _i64, _i64, _p, _i64, _p, _i64, C.c_float, _p, _i64, _i32, _i32, _i64, _i32, _p, _i64, _p])
SIGNATURES["clane_spmm_update_class_tiles_f32"] = (
    C.c_int, [_p, _p, _p, _p, _p, _i64, _i32, _p, _p, _i64, _i64, _i64, _p, _i64, _p, _i64, C.c_float, _p, _i64, _i32, _i32,
              _i32, _p, _p, _i64, _p])
SIGNATURES["clane_spmm_update_owned_tiles_f32"] = (
    C.c_int, [_p, _p, _p, _i32, _i64, _p, _i64, _p, _i64, C.c_float, _p, _i64, _i32, _i32, _i32, _p, _i64, _p])
# one weight per row instead of one per edge (csrc/spmm_update.h, UNIFORM): the calls above with `row_weight` for P
SIGNATURES["clane_row_weight_f32"] = SIGNATURES["clane_row_weight_f64"] = (C.c_int, [_p, _p, _i64, _p, _p, _p])
SIGNATURES["clane_spmm_update_rw_f32"] = (
    C.c_int, [_p, _p, _p, _i64, _i64, _p, _i64, _p, _i64, C.c_float, _p, _i64, _i32, _i64, _i32, _p, _p])
SIGNATURES["clane_spmm_update_tiles_rw_f32"] = SIGNATURES["clane_spmm_update_tiles_f32"]
SIGNATURES["clane_spmm_update_class_rw_f32"] = (
    C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _p, _p, _i64, _i64, _p, _i64, _p, _i64, C.c_float, _p, _i64, _i32, _i32, _p,
              _p, _p])
SIGNATURES["clane_spmm_update_class_tiles_rw_f32"] = (
    C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _p, _p, _i64, _i64, _i64, _p, _i64, _p, _i64, C.c_float, _p, _i64, _i32,
              _i32, _i32, _p, _p, _i64, _p])
SIGNATURES["clane_spmm_update_owned_rw_f32"] = (
    C.c_int, [_p, _p, _p, _p, _i32, _i64, _p, _i64, _p, _i64, C.c_float, _p, _i64, _i32, _i32, _p, _p])
SIGNATURES["clane_spmm_update_owned_tiles_rw_f32"] = (
    C.c_int, [_p, _p, _p, _p, _i32, _i64, _p, _i64, _p, _i64, C.c_float, _p, _i64, _i32, _i32, _i32, _p, _i64, _p])
for _s in ("f32", "f64"):
    SIGNATURES[f"clane_degree_weighted_sums_{_s}"] = (C.c_int, [_p, _p, _p, _i64, _p, _p, _p])
    SIGNATURES[f"clane_edge_score_finalize_{_s}"] = (C.c_int, [_p, _p, _i64, _i64, _i32, _p, _p, _p, _p])
    SIGNATURES[f"clane_segment_softmax_{_s}"] = (C.c_int, [_p, _i64, _p, _i64, _i64, _p, _i64, _p])
    SIGNATURES[f"clane_pair_cosine_{_s}"] = (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p])
    SIGNATURES[f"clane_edge_score_pair_{_s}"] = (
        C.c_int, [_p, _p, _i64, _i64, _p, _i64, _p, _i64, _i32, _p, _i32, _i64, _p, _i64, _p])
    SIGNATURES[f"clane_edge_score_class_pair_{_s}"] = (
        C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _p, _p, _i64, _i64, _p, _i64, _p, _i64, _i32, _p, _i32, _p, _p])
for _s in ("f32", "f64", "bf16"):
    SIGNATURES[f"clane_project_rows_{_s}"] = (C.c_int, [_p, _i64, _i32, _i64, _p, _p, _i64, _p])
    # training the bilinear similarity (csrc/pair_train.h)
    SIGNATURES[f"clane_pair_project_{_s}"] = (C.c_int, [_p, _i64, _i32, _i64, _p, _p, _i64, _p, _p, _p, _p])
    SIGNATURES[f"clane_pair_grad_{_s}"] = (C.c_int, [_p, _i64, _i32, _i64, _p, _p, _i64, _p, _p, _p, _p, _p, _p, _p])
for _s in ("f32", "f64"):
    SIGNATURES[f"clane_pair_loss_{_s}"] = (C.c_int, [_p, _p, _i64, _i32, _p, _p, _p, _p, _p, _p, _p])
    SIGNATURES[f"clane_adam_step_{_s}"] = (C.c_int, [_p, _p, _p, _p, _i64, C.c_double, _p, _p, _p])
SIGNATURES["clane_pair_grad_ws_len"] = (_i64, [_i64, _i32])
RANK_MAX_K = 32                     # CLANE_RANK_MAX_K
for _s in ("f32", "f64", "bf16"):   # link prediction (csrc/link_rank.h)
    SIGNATURES[f"clane_rank_scores_{_s}"] = (
        C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _i64, _i32, _p, _p, _p, _p, _p, _i32, _i32, _i32, _p, _p, _p])
    SIGNATURES[f"clane_pair_score_{_s}"] = (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _i64, _i32, _p, _p, _p, _p])
    SIGNATURES[f"clane_rank_count_{_s}"] = (      # held-out link evaluation (csrc/link_eval.h)
        C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _i64, _i32, _p, _p, _p, _p, _p, _i32, _i32, _p, _p, _p])
for _s in ("f32", "f64"):
    SIGNATURES[f"clane_rank_merge_{_s}"] = (C.c_int, [_p, _p, _i64, _i32, _i32, _p, _p, _p])
SIGNATURES["clane_pair_labels"] = (C.c_int, [_p, _p, _i64, _p, _p, _i64, _p, _p])
PROBE_MAX_CLASSES = 64              # CLANE_PROBE_MAX_CLASSES
PROBE_WRITE_G, PROBE_WRITE_PRED = 1, 2
PROBE_PRED_TOPK = 4                 # CLANE_PROBE_PRED_TOPK (one-vs-rest probe only)
for _s in ("f32", "f64", "bf16"):   # node classification probe (csrc/label_probe.h)
    SIGNATURES[f"clane_probe_forward_{_s}"] = (
        C.c_int, [_p, _i64, _i32, _i64, _p, _p, _i64, _p, _i64, _p, _p, _i32, _i32, _i32, _p, _p, _p, _p, _i64, _p])
    SIGNATURES[f"clane_probe_grad_{_s}"] = (C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _p, _i32, _p, _p, _p, _p])
    SIGNATURES[f"clane_probe_forward_ovr_{_s}"] = (      # multi-label probe (csrc/multilabel_probe.h)
        C.c_int, [_p, _i64, _i32, _i64, _p, _p, _i64, _p, _i64, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _i64, _p])
    SIGNATURES[f"clane_probe_predict_{_s}"] = (          # applying fitted probes (csrc/label_predict.h)
        C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p])
PREDICT_SIGMOID, PREDICT_WRITE_PROBA = 1, 2     # CLANE_PREDICT_*
PREDICT_MAX_TOP = 8                 # CLANE_PREDICT_MAX_TOP
SIGNATURES["clane_probe_loss_ws_len"] = (_i64, [_i64, _i32])
SIGNATURES["clane_probe_grad_ws_len"] = (_i64, [_i64, _i32, _i32])
for _s in ("f32", "f64", "bf16"):   # node clustering (csrc/kmeans.h)
    SIGNATURES[f"clane_kmeans_assign_{_s}"] = (
        C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _p, _p, _i32, _i32, _p, _i64, _p, _i64, _p])
    SIGNATURES[f"clane_kmeans_update_{_s}"] = (
        C.c_int, [_p, _i64, _i32, _i64, _p, _p, _i64, _i32, _i32, _p, _p, _p, _p, _p])
SIGNATURES["clane_kmeans_update_ws_len"] = (_i64, [_i64, _i32, _i32, _i32])
MIXTURE_MAX_COMPONENTS = 64         # CLANE_MIXTURE_MAX_COMPONENTS
MIXTURE_WRITE_RESP, MIXTURE_WRITE_ASSIGN = 1, 2
for _s in ("f32", "f64", "bf16"):   # Gaussian mixtures (csrc/mixture.h)
    SIGNATURES[f"clane_mixture_estep_{_s}"] = (
        C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _p, _p, _p, _i32, _i32, _i32, _p, _p, _p, _p, _i64, _p])
    SIGNATURES[f"clane_mixture_mstep_{_s}"] = (C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _p, _p, _i32, _p, _p, _p, _p])
SIGNATURES["clane_mixture_ll_ws_len"] = (_i64, [_i64, _i32])
SIGNATURES["clane_mixture_mstep_ws_len"] = (_i64, [_i64, _i32, _i32])
for _s in ("f32", "f64", "bf16"):   # new vertices against the finished table (csrc/new_rows.h)
    _g = C.c_double if _s == "f64" else C.c_float
    SIGNATURES[f"clane_embed_rows_{_s}"] = (
        C.c_int, [_p, _p, _i64, _p, _i64, _p, _i64, _i64, _i32, _i32, _p, _p, _p, _i64, _g, _i32, _i32, _i32, _p, _i64,
                  _p, _p, _p, _p])

PCA_ACCUMULATE = 1                  # CLANE_PCA_ACCUMULATE
for _s in ("f32", "f64", "bf16"):   # content reduction (csrc/content_pca.h)
    SIGNATURES[f"clane_column_sums_{_s}"] = (C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _i32, _p, _p, _p])
    SIGNATURES[f"clane_gram_{_s}"] = (C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _p, _i32, _p, _p, _p])
    SIGNATURES[f"clane_project_affine_{_s}"] = (C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _p, _p, _i32, _p, _i64, _p])
SIGNATURES["clane_column_sums_ws_len"] = (_i64, [_i64, _i32])
SIGNATURES["clane_gram_ws_len"] = (_i64, [_i64, _i32])
CSR_MAX_L = 512                     # CLANE_CSR_MAX_L; sparse content (csrc/sparse_rows.h)
SIGNATURES["clane_csr_spmm_segment"] = (C.c_int, [])
SIGNATURES["clane_csr_spmm_ws_len"] = (_i64, [_i64, _i64, _i32])
SIGNATURES["clane_csr_spmm_f32"] = (
    C.c_int, [_p, _p, _p, _i64, _i64, _p, _i64, _i64, _i32, _p, _p, _p, _p, _p, _i64, _i64, _p, _i64, _p, _i64, _p])
SIGNATURES["clane_csr_row_sums_f32"] = (C.c_int, [_p, _p, _i64, _i64, _p, _p, _p, _i64, _i64, _p, _i64, _p, _p])
TSNE_MAX_POINTS = 65536             # CLANE_TSNE_MAX_POINTS; 2-D layout (csrc/tsne.h)
TSNE_FORCES_KL, TSNE_FORCES_CACHED = 1, 2
for _s in ("f32", "bf16"):
    SIGNATURES[f"clane_tsne_sqdist_{_s}"] = (C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _p, _p, _p, _p])
SIGNATURES["clane_tsne_affinities_f32"] = (C.c_int, [_p, _i64, C.c_float, _p, _p])
SIGNATURES["clane_tsne_symmetrize_ws_len"] = (_i64, [_i64])
SIGNATURES["clane_tsne_symmetrize_f32"] = (C.c_int, [_p, _i64, _p, _p])
SIGNATURES["clane_tsne_forces_f32"] = (C.c_int, [_p, _p, _i64, _i32, _p, _p])
SIGNATURES["clane_tsne_step_f32"] = (
    C.c_int, [_p, _p, _i64, C.c_double, C.c_double, C.c_double, C.c_double, _p, _p, _p, _p, _p])
KNN_MAX_K = 192                     # CLANE_KNN_MAX_K; neighbour-sparse 2-D layout (csrc/tsne_nn.h)
TSNE_NN_MAX_POINTS = 1 << 20        # CLANE_TSNE_NN_MAX_POINTS
for _s in ("f32", "bf16"):
    SIGNATURES[f"clane_knn_sqdist_{_s}"] = (
        C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _p, _p, _i32, _i32, _p, _p, _p, _p, _p])
SIGNATURES["clane_tsne_nn_affinities_f32"] = (C.c_int, [_p, _p, _i64, _i32, C.c_float, _p, _p, _p])
SIGNATURES["clane_tsne_nn_plogp_f32"] = (C.c_int, [_p, _p, _i64, _i64, _p, _p])
SIGNATURES["clane_tsne_nn_attract_f32"] = (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i32, _p, _p])
SIGNATURES["clane_tsne_repulse_f32"] = (C.c_int, [_p, _i64, _p, _p])
SILHOUETTE_METRICS = {"euclidean": 0, "cosine": 1}      # CLANE_SILHOUETTE_*; silhouette (csrc/silhouette.h)
for _s in ("f32", "f64", "bf16"):
    SIGNATURES[f"clane_silhouette_norms_{_s}"] = (C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _p, _i32, _p, _p])
    SIGNATURES[f"clane_silhouette_sums_{_s}"] = (
        C.c_int, [_p, _i64, _i32, _i64, _p, _i64, _p, _i32, _p, _p, _i32, _i64, _i64, _p, _p])


def probe_padded_classes(C_: int) -> int:
    """Cp: the columns a fit takes in the stacked weights -- C rounded up to a power of two."""
    if not 2 <= int(C_) <= PROBE_MAX_CLASSES:
        raise ValueError(f"the label probe handles 2..{PROBE_MAX_CLASSES} classes, got {C_}")
    return 1 << (int(C_) - 1).bit_length()


def ovr_padded_classes(C_: int) -> int:
    """Cp of the one-vs-rest probe: as ``probe_padded_classes``, but one class is a problem too (1..64)."""
    if not 1 <= int(C_) <= PROBE_MAX_CLASSES:
        raise ValueError(f"the multi-label probe handles 1..{PROBE_MAX_CLASSES} classes, got {C_}")
    return 1 << (int(C_) - 1).bit_length()


def mixture_padded_components(K_: int) -> int:
    """Kp: the columns a restart takes in the stacked mixture parameters -- K rounded up to a power of two (1..64)."""
    if not 1 <= int(K_) <= MIXTURE_MAX_COMPONENTS:
        raise ValueError(f"the Gaussian mixture handles 1..{MIXTURE_MAX_COMPONENTS} components, got {K_}")
    return 1 << (int(K_) - 1).bit_length()


_SUFFIX = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16"}
_ACC = {torch.float32: torch.float32, torch.float64: torch.float64, torch.bfloat16: torch.float32}
VEC_ELEMS = {torch.float32: 4, torch.float64: 2, torch.bfloat16: 8}  # elements per 16-byte pack


class ClaneHipError(RuntimeError):
    pass


class _MirrorStruct(C.Structure):       # clane_mirror_t
    _fields_ = [("row_ptr", _p), ("slot", _p), ("bufs", _p), ("ld", _i64), ("aligned16", _i32)]


MIRROR_ROW_BITS = 28


class Mirror:
    """Further destinations of the rows an spmm_update* call finishes (``clane_mirror_t``): row r of the call is
    also stored at the places ``slot[row_ptr[r]:row_ptr[r+1]]``, a place being ``buffer << 28 | row`` into
    ``bufs`` (one tensor, or up to 8 of equal leading dimension -- e.g. other GPUs' tables).  Holds them alive."""

    def __init__(self, row_ptr: torch.Tensor, slot: torch.Tensor, bufs):
        if row_ptr.dtype != torch.int64 or slot.dtype != torch.int32 or not (row_ptr.is_contiguous()
                                                                             and slot.is_contiguous()):
            raise ValueError("Mirror: row_ptr must be contiguous int64 and slot contiguous int32")
        bufs = [bufs] if isinstance(bufs, (torch.Tensor, PeerMatrix)) else list(bufs)
        if not 1 <= len(bufs) <= 8:
            raise ValueError("Mirror: 1 to 8 destination buffers")
        mats = [_mat(b, "mirror buffer") for b in bufs]
        if len({ld for _, ld in mats}) != 1 or len({b.dtype for b in bufs}) != 1:
            raise ValueError("Mirror: the buffers must share dtype and leading dimension")
        if max(b.shape[0] for b in bufs) > (1 << MIRROR_ROW_BITS):
            raise ValueError("Mirror: a buffer has more than 2^28 rows")
        self.row_ptr, self.slot, self.bufs = row_ptr, slot, bufs
        self.buf = bufs[0]
        self.bases = torch.tensor([ptr for ptr, _ in mats], dtype=torch.int64, device=row_ptr.device)
        self.c = _MirrorStruct(row_ptr.data_ptr(), slot.data_ptr(), self.bases.data_ptr(), mats[0][1],
                               int(all(ptr % 16 == 0 for ptr, _ in mats)))


class _RawDeviceMemory:
    """What torch.as_tensor needs to view foreign device memory without copying it."""

    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


class PeerMatrix:
    """Address + shape of a row-major matrix in ANOTHER process's (GPU's) memory, mapped here.  Not a torch tensor
    on purpose: torch would attribute it to the owning device; only kernels of this library touch it, by address."""

    def __init__(self, ptr: int, shape, dtype: torch.dtype):
        self._ptr, self.shape, self.dtype = ptr, tuple(shape), dtype

    def data_ptr(self) -> int:
        return self._ptr

    def dim(self) -> int:
        return len(self.shape)

    def stride(self, i: Optional[int] = None):
        st = (self.shape[1], 1)
        return st if i is None else st[i]


class DeviceBuffer:
    """A matrix in device memory that is its OWN allocation (hipMalloc through the C ABI), so that another process
    can map it (hipIpc works on allocation bases; torch sub-allocates) -- or such a mapping of another process's
    matrix (`DeviceBuffer.open`).  `.tensor` views it; torch neither owns nor frees it: this object does."""

    def __init__(self, lib, shape, dtype: torch.dtype, device, _mapped_from: Optional[bytes] = None,
                 contiguous: bool = False):
        """``contiguous``: physically contiguous backing (clane_device_alloc_contiguous); raises ClaneHipError when
        the driver has no such range free -- the caller falls back to an ordinary allocation."""
        self.lib, self.shape, self.dtype = lib, tuple(int(x) for x in shape), dtype
        self.nbytes = max(16, int(torch.empty(0, dtype=dtype).element_size()) * int(torch.Size(self.shape).numel()))
        self.mapped = _mapped_from is not None
        ptr = _p()
        with torch.cuda.device(device):
            if self.mapped:
                rc = lib.clane_ipc_open(_mapped_from, C.byref(ptr))
            elif contiguous:
                rc = lib.clane_device_alloc_contiguous(self.nbytes, C.byref(ptr))
            else:
                rc = lib.clane_device_alloc(self.nbytes, C.byref(ptr))
        if rc != 0:
            raise ClaneHipError(f"{'clane_ipc_open' if self.mapped else 'clane_device_alloc'} failed ({rc}): "
                                f"{lib.clane_last_error().decode()}")
        self.ptr = ptr.value
        if self.mapped:
            self.tensor = PeerMatrix(self.ptr, self.shape, dtype)
        else:
            raw = torch.as_tensor(_RawDeviceMemory(self.ptr, self.nbytes), device=torch.device(device))
            n = int(torch.Size(self.shape).numel()) * torch.empty(0, dtype=dtype).element_size()
            self.tensor = raw[:n].view(dtype).view(self.shape)
            self.tensor.zero_()

    def export(self) -> bytes:
        handle = C.create_string_buffer(IPC_HANDLE_BYTES)
        rc = self.lib.clane_ipc_export(self.ptr, handle)
        if rc != 0:
            raise ClaneHipError(f"clane_ipc_export failed ({rc}): {self.lib.clane_last_error().decode()}")
        return handle.raw

    @classmethod
    def open(cls, lib, handle: bytes, shape, dtype: torch.dtype, device) -> "DeviceBuffer":
        return cls(lib, shape, dtype, device, _mapped_from=handle)

    def close(self) -> None:
        if self.ptr:
            (self.lib.clane_ipc_close if self.mapped else self.lib.clane_device_free)(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown: the process is about to give everything back anyway
            pass


class _OwnedPlanStruct(C.Structure):    # clane_owned_plan_t
    _fields_ = [(name, _p) for name in ("grp_bat_ptr", "bat_vrow_ptr", "bat_row_ptr", "bat_seg_ptr", "seg_e0", "seg_len",
                                        "seg_vrow", "row_id", "row_part", "row_vptr")] + \
               [(name, _i32) for name in ("n_groups", "n_steps", "chunk", "max_batch_vrows")]


OWNED_PLAN_ARRAYS = {"grp_bat_ptr": torch.int32, "bat_vrow_ptr": torch.int32, "bat_row_ptr": torch.int32,
                     "bat_seg_ptr": torch.int32, "seg_e0": torch.int64, "seg_len": torch.int32, "seg_vrow": torch.int32,
                     "row_id": torch.int32, "row_part": torch.int32, "row_vptr": torch.int32}
OWNED_MAX_STEPS = 64
OWNED_LDS_LIMIT = 159 * 1024         # 160 KiB per CU less what the kernel keeps beside the sums


class OwnedPlan:
    """The plan of an spmm_update_owned call on the device (``clane_owned_plan_t``): `plan` is what
    ``xcd.owned_plan`` returns (numpy), `chunk` the piece length.  Holds the arrays alive."""

    def __init__(self, plan: dict, chunk: int, device):
        self.n_groups, self.n_steps = int(plan["n_groups"]), int(plan["n_steps"])
        self.chunk, self.max_batch_vrows = int(chunk), int(plan["max_batch_vrows"])
        self.n_rows = int(plan["row_id"].shape[0])
        self.arrays = {}
        for name, dtype in OWNED_PLAN_ARRAYS.items():
            t = torch.as_tensor(plan[name])
            if t.dtype != dtype or t.dim() != 1:
                raise ValueError(f"OwnedPlan: {name} must be a 1-D {dtype} array")
            self.arrays[name] = t.contiguous().to(device)
        a = {k: v.cpu() for k, v in self.arrays.items()}            # checked once, on the host: the kernel trusts them
        B = a["bat_vrow_ptr"].numel() - 1
        ok = (a["grp_bat_ptr"].numel() == self.n_groups + 1 and int(a["grp_bat_ptr"][0]) == 0
              and int(a["grp_bat_ptr"][-1]) == B and bool((a["grp_bat_ptr"].diff() >= 0).all())
              and a["bat_row_ptr"].numel() == B + 1 and a["bat_seg_ptr"].numel() == B * self.n_steps + 1
              and int(a["bat_vrow_ptr"][0]) == 0 and int(a["bat_row_ptr"][0]) == 0 and int(a["bat_seg_ptr"][0]) == 0
              and bool((a["bat_vrow_ptr"].diff() >= 0).all()) and bool((a["bat_row_ptr"].diff() >= 0).all())
              and bool((a["bat_seg_ptr"].diff() >= 0).all()) and int(a["bat_row_ptr"][-1]) == self.n_rows
              and a["row_vptr"].numel() == self.n_rows + 1 and a["row_part"].numel() == self.n_rows
              and int(a["row_vptr"][0]) == 0 and bool((a["row_vptr"].diff() >= 1).all())
              and int(a["row_vptr"][-1]) == int(a["bat_vrow_ptr"][-1])
              and bool((a["row_vptr"][a["bat_row_ptr"].long()] == a["bat_vrow_ptr"]).all())
              and int(a["bat_vrow_ptr"].diff().max() if B else 0) <= self.max_batch_vrows
              and a["seg_e0"].numel() == a["seg_len"].numel() == a["seg_vrow"].numel() == int(a["bat_seg_ptr"][-1])
              and 1 <= self.n_steps <= OWNED_MAX_STEPS and self.chunk >= 64 and self.chunk % 64 == 0)
        if ok and a["seg_len"].numel():
            per_batch = a["bat_seg_ptr"][self.n_steps::self.n_steps] - a["bat_seg_ptr"][:-1:self.n_steps]
            seg_bat = torch.repeat_interleave(torch.arange(B), per_batch.long())
            ok = bool((a["seg_len"] > 0).all()) and bool((a["seg_e0"] >= 0).all()) and bool((a["seg_vrow"] >= 0).all()) \
                and bool((a["seg_vrow"] < a["bat_vrow_ptr"].diff()[seg_bat]).all())
        if not ok:
            raise ValueError("OwnedPlan: the arrays do not describe a plan (see include/clane_hip.h)")
        # every segment's row (relative to the call's first row, as row_id is): what the per-row-weight calls index by
        self.seg_row = torch.zeros(0, dtype=torch.int32, device=device)
        if a["seg_len"].numel():
            vrow = a["bat_vrow_ptr"][seg_bat].long() + a["seg_vrow"].long()
            owner = torch.searchsorted(a["row_vptr"].long(), vrow, right=True) - 1
            self.seg_row = a["row_id"][owner].contiguous().to(device)
        self.max_edge = int((a["seg_e0"] + a["seg_len"]).max()) if a["seg_len"].numel() else 0
        self.max_row = int(a["row_id"].max()) if self.n_rows else -1
        self.max_part = int(a["row_part"].max()) if self.n_rows else -1
        self.c = _OwnedPlanStruct(*[self.arrays[name].data_ptr() for name in OWNED_PLAN_ARRAYS], self.n_groups,
                                  self.n_steps, self.chunk, self.max_batch_vrows)


def _mirror_arg(mirror: Optional["Mirror"], dtype: torch.dtype):
    if mirror is None:
        return None
    if mirror.buf.dtype != dtype:
        raise ValueError("mirror.buf must have the dtype of Z_new")
    return C.cast(C.pointer(mirror.c), _p)


def load_library(path: Optional[Path] = None) -> C.CDLL:
    """dlopen the library and bind every declared symbol.  Raises if anything is missing."""
    if path is None and os.environ.get("CLANE_HIP_LIB"):      # A/B builds of the same ABI (tools/ab_variants.py)
        path = os.environ["CLANE_HIP_LIB"]
    path = Path(path) if path is not None else LIB_PATH
    if not path.exists():
        raise ClaneHipError(
            f"{path} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `make -C clane_amd/csrc`) -- clane_amd has no CPU fallback.")
    lib = C.CDLL(str(path))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype, fn.argtypes = res, args
    got = lib.clane_abi_version()
    if got != ABI_VERSION:
        raise ClaneHipError(f"{path}: ABI version {got}, expected {ABI_VERSION}")
    return lib


def acc_dtype(dtype: torch.dtype) -> torch.dtype:
    """dtype of P / scores / squared norms for a given storage dtype of Z."""
    try:
        return _ACC[dtype]
    except KeyError:
        raise TypeError(f"clane_amd supports float32, float64 and bfloat16 embeddings, not {dtype}") from None


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _mat(t: torch.Tensor, name: str):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: need a row-major 2-D tensor with unit column stride, got {tuple(t.shape)} "
                         f"strides {t.stride()}")
    return t.data_ptr(), t.stride(0)


def _vec(t: torch.Tensor, dtype: torch.dtype, name: str):
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: need a contiguous {dtype} tensor, got {t.dtype} contiguous={t.is_contiguous()}")
    return t.data_ptr()


class KernelBackend(abc.ABC):
    """Every call ``SweepEngine`` / ``Graph`` / ``CosineSimilarity`` make on their kernel object -- the contract
    between the host logic and whatever executes the kernels.  ``HipKernels`` (the C ABI) is the product's only
    implementation; the CPU suite's test double (tests/oracle_kernels.py) implements the same list.  An
    implementation that lacks one of these cannot be instantiated, so nothing the engine relies on (the CSR check
    that keeps a bad index from faulting the GPU, say) can be skipped silently: the engine calls them
    unconditionally."""

    # sizes
    @abc.abstractmethod
    def spmm_partials_len(self, nrows: int, n_long: int) -> int: ...
    @abc.abstractmethod
    def reduce_ws_len(self) -> int: ...
    @abc.abstractmethod
    def spmm_split_slab_len(self, n_segments: int, d: int) -> int: ...
    @abc.abstractmethod
    def spmm_class_slab_len(self, n_slots: int, d: int) -> int: ...
    # input check, build description
    @abc.abstractmethod
    def check_csr(self, rowptr, colidx, nrows: int, n_edges: int, table_rows: int) -> None: ...
    @abc.abstractmethod
    def build_info(self) -> str: ...
    # K0 / K1 / K2
    @abc.abstractmethod
    def row_sqnorm(self, Z, d: int, sq): ...
    @abc.abstractmethod
    def degree_weighted_sums(self, sq, rowptr, indeg, nrows: int, ws, out2): ...
    @abc.abstractmethod
    def edge_score(self, rowptr, colidx, nrows, row0, Z, d, mode, sums2, sq, scores, long_threshold=0, long_rows=None,
                   fuse_softmax=False): ...
    @abc.abstractmethod
    def edge_score_class(self, rowptr, colidx, item_e0, item_len, item_slot, item_row, items_per_block, class_rows,
                         slot_ptr, row0, Z, d, mode, sums2, sq, scores, stats=None, fuse_softmax=False,
                         n_slots=None, row_parts=1): ...
    @abc.abstractmethod
    def edge_score_finalize(self, rowptr, colidx, nrows, row0, mode, sums2, sq, scores): ...
    @abc.abstractmethod
    def segment_softmax(self, rowptr, nrows, vals, min_degree=0, max_degree=0, long_rows=None): ...
    @abc.abstractmethod
    def pair_cosine(self, A, B, d, out, ws): ...
    # K3
    @abc.abstractmethod
    def spmm_update(self, rowptr, colidx, P, nrows, row0, Z_old, X, gamma, Z_new, d, long_threshold, partials,
                    sinks_untouched=False, mirror=None, beyond_cache=False): ...
    @abc.abstractmethod
    def spmm_update_long(self, rowptr, colidx, P, long_rows, waves_per_row, row0, Z_old, X, gamma, Z_new, d, partials,
                         mirror=None): ...
    @abc.abstractmethod
    def spmm_update_split(self, rowptr, colidx, P, split_rows, seg_ptr, seg_row, edges_per_segment, row0, Z_old, X,
                          gamma, Z_new, d, slab, partials, mirror=None): ...
    @abc.abstractmethod
    def spmm_update_class(self, colidx, P, item_e0, item_len, item_slot, items_per_block, class_rows, slot_ptr, row0,
                          Z_old, X, gamma, Z_new, d, slab, partials, mirror=None, beyond_cache=False): ...
    @abc.abstractmethod
    def reduce_partials(self, partials, n, ws, out): ...
    @abc.abstractmethod
    def l1_distance(self, A, B, d, ws, out, sq_a=None): ...
    @abc.abstractmethod
    def gather_rows(self, src, idx, d, dst): ...
    # further destinations of finished rows, tables other processes map
    @abc.abstractmethod
    def make_mirror(self, row_ptr, slot, bufs): ...
    @abc.abstractmethod
    def shareable_matrix(self, shape, dtype, device): ...
    @abc.abstractmethod
    def contiguous_matrix(self, shape, dtype, device): ...
    @abc.abstractmethod
    def open_shared_matrix(self, handle, shape, dtype, device): ...

    # bilinear similarity (AsymmertricSimilarity): not abstract -- a backend without them still serves every other path,
    # and SweepEngine.build_P_bilinear is the only caller
    def project_rows(self, Z, d: int, W, Y):
        """Y[:, :2d] = Z[:, :d] . W^T for every row of Z (W: [2d, d], accumulate dtype)."""
        raise NotImplementedError(f"{type(self).__name__} has no project_rows")

    def edge_score_pair(self, rowptr, colidx, nrows, row0, S, N, d, scores, long_threshold=0, long_rows=None,
                        fuse_softmax=False):
        """edge_score with two tables: the raw dot of S[row0 + r, :d] and N[col, :d]."""
        raise NotImplementedError(f"{type(self).__name__} has no edge_score_pair")

    def edge_score_class_pair(self, rowptr, colidx, item_e0, item_len, item_slot, item_row, items_per_block,
                              class_rows, slot_ptr, row0, S, N, d, scores, stats=None, fuse_softmax=False,
                              n_slots=None, row_parts=1):
        """edge_score_class with two tables, as edge_score_pair."""
        raise NotImplementedError(f"{type(self).__name__} has no edge_score_class_pair")

    # training the bilinear similarity (train.py): optional in the same way -- SimilarityTrainer / PairSampler are the
    # only callers.  Pairs are TABLE ROWS (int32), linked / mask uint8, u / A / Bm / g / W / dW in the accumulate dtype.
    def pair_project(self, Z, d: int, src, dst, W, A, Bm):
        """A[k] = W[:d] . Z[src[k], :d], Bm[k] = W[d:] . Z[dst[k], :d] for the src.numel() pairs (A, Bm: [B, d])."""
        raise NotImplementedError(f"{type(self).__name__} has no pair_project")

    def pair_loss(self, A, Bm, d: int, linked, u, g, mask, ws, stats):
        """Per pair s = A[k] . Bm[k], the masked log loss of embedder.py:276-282 and g = d loss / d s; stats = {sum of
        the masked losses, M} (float64 [2]); ws: reduce_ws_len() float64."""
        raise NotImplementedError(f"{type(self).__name__} has no pair_loss")

    def pair_grad_ws_len(self, B: int, d: int) -> int:
        raise NotImplementedError(f"{type(self).__name__} has no pair_grad_ws_len")

    def pair_grad(self, Z, d: int, src, dst, A, Bm, g, stats, ws, dW):
        """dW [2d, d] = the gradient of the mean masked loss; M = stats[1] is read on the device, M = 0 gives zeros."""
        raise NotImplementedError(f"{type(self).__name__} has no pair_grad")

    def adam_step(self, W, m, v, dW, lr: float, stats, state):
        """One torch.optim.Adam (defaults) step; state = {steps taken, sum of step losses} (float64 [2]); stats[1] == 0:
        nothing changes."""
        raise NotImplementedError(f"{type(self).__name__} has no adam_step")

    def pair_labels(self, rowptr, colidx, nrows: int, src, dst, linked):
        """linked[k] = dst[k] is a column of row src[k] of a CSR with sorted, unique rows."""
        raise NotImplementedError(f"{type(self).__name__} has no pair_labels")

    # link prediction (links.py): optional in the same way -- LinkRanker is the only caller.  Rows are TABLE ROWS (int32).
    def rank_scores(self, S, N, table_rows: int, d: int, q_rows, mode: int, sums2, sq, label, excl_rowptr, excl_colidx,
                    exclude_self: bool, k: int, n_slabs: int, cand_score, cand_id):
        """The k best candidates of every query row in each of n_slabs ranges of the table: cand_score / cand_id
        [Q, n_slabs, k], unused places -inf / -1."""
        raise NotImplementedError(f"{type(self).__name__} has no rank_scores")

    def rank_merge(self, cand_score, cand_id, n_slabs: int, k: int, out_score, out_id):
        """[Q, n_slabs, k] candidates -> [Q, k], score descending, ties by id ascending."""
        raise NotImplementedError(f"{type(self).__name__} has no rank_merge")

    def pair_score(self, S, N, table_rows: int, d: int, src, dst, mode: int, sums2, sq, out):
        """out[i] = score(src[i], dst[i]); an index outside the table reads as a zero row."""
        raise NotImplementedError(f"{type(self).__name__} has no pair_score")

    def rank_count(self, S, N, table_rows: int, d: int, q_rows, t_rows, mode: int, sums2, sq, label, excl_rowptr,
                   excl_colidx, exclude_self: bool, n_slabs: int, target_score, counts):
        """For pair i = (q_rows[i], t_rows[i]): target_score[i], the pair's score as rank_scores computes it, and counts
        [B, n_slabs, 4] = (greater, equal_lower, equal_higher, eligible) among each slab's candidates; a pair without a
        rank: -1 / -inf."""
        raise NotImplementedError(f"{type(self).__name__} has no rank_count")

    # node classification (classify.py): optional in the same way -- LabelProbe is the only caller.  rows are TABLE ROWS
    # (int32), y int32 classes, split uint8 [n, >= F]; W [F * Cp, d], bias, G [n, F * Cp], dW, db in the accumulate dtype.
    def probe_loss_ws_len(self, n: int, F: int) -> int:
        raise NotImplementedError(f"{type(self).__name__} has no probe_loss_ws_len")

    def probe_forward(self, Z, d: int, rows, y, split, W, bias, F: int, C: int, loss_ws, loss, G=None, pred=None):
        """loss[f] = sum over the rows that train fit f (split[i, f] != 0) of the cross-entropy of softmax(Z[rows[i], :d] .
        W_f^T + bias_f) against y[i] (float64 [F]); with ``G`` also G[i, f Cp + c] = split (p_c - [c == y_i]), with
        ``pred`` (int32, [n, >= F]) the arg-max class of EVERY row, ties to the lowest class."""
        raise NotImplementedError(f"{type(self).__name__} has no probe_forward")

    def probe_forward_ovr(self, Z, d: int, rows, ymask, split, W, bias, col_state, F: int, C: int, max_labels: int,
                          loss_ws, loss, G=None, pred=None, top_k: bool = True):
        """The one-vs-rest forward of the multi-label probe.  ymask int64 [n]: the bits of the row's class set (bit c:
        class c; the tensor holds the uint64 pattern); col_state int8 [F * Cp]: 0 fitted, -1 / +1 constant-negative /
        -positive.  loss[f] = sum over the rows that train fit f and its fitted columns of softplus(l) - y l (float64 [F]);
        with ``G`` also G[i, f Cp + c] = sigmoid(l) - y there and 0 elsewhere; with ``pred`` (int64, [n, >= F]) the mask
        of predicted classes of EVERY row: ``top_k`` the popcount(ymask[i]) columns of highest value (l, or -inf / +inf
        for a constant column; ties to the lowest class, -inf and NaN never), else the columns of value > 0."""
        raise NotImplementedError(f"{type(self).__name__} has no probe_forward_ovr")

    def probe_grad_ws_len(self, n: int, K: int, d: int) -> int:
        raise NotImplementedError(f"{type(self).__name__} has no probe_grad_ws_len")

    def probe_grad(self, Z, d: int, rows, G, ws, dW, db):
        """dW [K, d] = G^T . Z[rows, :d], db [K] = the column sums of G."""
        raise NotImplementedError(f"{type(self).__name__} has no probe_grad")

    def probe_predict(self, Z, d: int, rows, W, bias, F: int, C: int, top_class, top_prob, proba=None,
                      sigmoid: bool = False, col_state=None):
        """Apply F stacked models to the rows: top_class (int32) / top_prob (accumulate dtype) [n, F, top_m], 1 <= top_m
        <= 8, the classes of highest value best first (ties to the lowest class, NaN and -inf never, the rest -1 / 0);
        with ``proba`` [n, F, C] every class's probability.  Soft-max over a fit's C classes with the value the logit, or
        (``sigmoid``, one-vs-rest models) a sigmoid per column with ``col_state`` int8 [F * Cp]: a column of state -1 /
        +1 has value -inf / +inf and probability 0 / 1."""
        raise NotImplementedError(f"{type(self).__name__} has no probe_predict")

    # node clustering (cluster.py): optional in the same way -- KMeans is the only caller.  rows / order are TABLE ROWS
    # (int32); centres [R, K, d], csq [R, K], best and the workspace in the accumulate dtype.
    def kmeans_assign(self, Z, d: int, rows, centres, csq, assign, best):
        """assign[i, r] (int32, [n, >= R]) = the centre of restart r nearest to Z[rows[i], :d], ties to the lowest index;
        best[i, r] = min_j (csq[r, j] - 2 z_i . c[r, j]): the squared distance without |z_i|^2."""
        raise NotImplementedError(f"{type(self).__name__} has no kmeans_assign")

    def kmeans_update_ws_len(self, n: int, R: int, K: int, d: int) -> int:
        raise NotImplementedError(f"{type(self).__name__} has no kmeans_update_ws_len")

    def kmeans_update(self, Z, d: int, order, seg, centres_old, ws, centres_new, csq_new):
        """centres_new[r, j] = the mean of the table rows order[seg[r K + j] : seg[r K + j + 1]] (the old centre where
        the segment is empty), csq_new its squared norm.  order holds restart r's n rows at [r n, (r + 1) n)."""
        raise NotImplementedError(f"{type(self).__name__} has no kmeans_update")

    # soft clusters (mixture.py): optional in the same way -- GaussianMixture is the only caller.  rows are TABLE ROWS
    # (int32); mean [d], Wm [R * Kp, 2 d], cst [R * Kp], resp [n, R * Kp], S and nk in the accumulate dtype.
    def mixture_ll_ws_len(self, n: int, R: int) -> int:
        raise NotImplementedError(f"{type(self).__name__} has no mixture_ll_ws_len")

    def mixture_estep(self, Z, d: int, rows, mean, Wm, cst, R: int, K: int, ll_ws, ll, resp=None, assign=None):
        """With xc = Z[rows[i], :d] - mean and l = [xc^2 | xc] . Wm_r^T + cst_r over restart r's K real components:
        ll[r] = sum_i logsumexp(l) (float64 [R]); with ``resp`` ([n, R * Kp]) also the responsibilities exp(l - lse), pad
        columns 0; with ``assign`` (int32, [n, >= R]) the arg-max component, ties to the lowest."""
        raise NotImplementedError(f"{type(self).__name__} has no mixture_estep")

    def mixture_mstep_ws_len(self, n: int, K: int, d: int) -> int:
        raise NotImplementedError(f"{type(self).__name__} has no mixture_mstep_ws_len")

    def mixture_mstep(self, Z, d: int, rows, mean, resp, ws, S, nk):
        """S [K, 2 d] = resp^T . [xc^2 | xc] and nk [K] = the column sums of resp, K = the columns of resp."""
        raise NotImplementedError(f"{type(self).__name__} has no mixture_mstep")

    # content reduction (reduce.py): optional in the same way -- ContentPCA is the only caller.  rows are TABLE ROWS
    # (int32; an entry outside the table is an absent row); mu, W, G and the Gram's workspace in the accumulate dtype.
    def column_sums_ws_len(self, n: int, d: int) -> int:
        raise NotImplementedError(f"{type(self).__name__} has no column_sums_ws_len")

    def column_sums(self, Z, d: int, rows, ws, sums, accumulate: bool = False):
        """sums [d] (float64) = the column sums of Z[rows, :d], rows in chunks of 2048, the chunks in order; with
        ``accumulate`` on top of what sums holds."""
        raise NotImplementedError(f"{type(self).__name__} has no column_sums")

    def gram_ws_len(self, n: int, d: int) -> int:
        raise NotImplementedError(f"{type(self).__name__} has no gram_ws_len")

    def gram(self, Z, d: int, rows, mu, ws, G, accumulate: bool = False):
        """G [d, d] = sum_i (z_i - mu)(z_i - mu)^T over Z[rows, :d] (mu None: no centring), bitwise symmetric; with
        ``accumulate`` on top of what G holds."""
        raise NotImplementedError(f"{type(self).__name__} has no gram")

    def project_affine(self, Z, d: int, rows, mu, W, Y):
        """Y[i, :m] = W (Z[rows[i], :d] - mu), W [m, d]; Y in Z's dtype, rounded once."""
        raise NotImplementedError(f"{type(self).__name__} has no project_affine")

    # sparse content (sparse.py, ContentPCA.fit_sparse): optional in the same way.  S is a sparse.SparseRows on the device
    # (validated CSR, its long rows listed in segments of csr_spmm_segment() non-zeros); everything dense is float32.
    def csr_spmm_segment(self) -> int:
        raise NotImplementedError(f"{type(self).__name__} has no csr_spmm_segment")

    def csr_spmm_ws_len(self, n_rows: int, nnz: int, l: int) -> int:
        raise NotImplementedError(f"{type(self).__name__} has no csr_spmm_ws_len")

    def csr_spmm(self, S, B, l: int, out, a=None, s=None, ws=None):
        """out[r, :l] = sum_e val[e] B[col[e], :l] - a[r] s[:l] over the non-zeros of row r (a None: ones; s None: no
        epilogue); l a multiple of 4 up to 512; columns past l of B and out are neither read nor written."""
        raise NotImplementedError(f"{type(self).__name__} has no csr_spmm")

    def csr_row_sums(self, S, sums, ws=None):
        """sums[r] (float64) = the sum of the values of row r, in a fixed order."""
        raise NotImplementedError(f"{type(self).__name__} has no csr_row_sums")

    # 2-D layout (layout.py): optional in the same way -- TSNE is the only caller.  D / P [n, n], Y / V / G [n, 2], F [n, 6]
    # float32 and contiguous; everything but sqdist's table is float32 whatever the table's dtype.
    def tsne_sqdist(self, Z, d: int, rows, mu, sq, D):
        """D[i, j] = max(0, |a_i|^2 + |a_j|^2 - 2 a_i . a_j) with a = Z[rows, :d] - mu (a row outside the table: z = 0);
        bitwise symmetric, the diagonal exactly 0; sq [n]: the squared norms, a workspace."""
        raise NotImplementedError(f"{type(self).__name__} has no tsne_sqdist")

    def tsne_affinities(self, D, perplexity: float, beta):
        """In place: row i of D becomes the conditional affinities p_{j|i} at the beta_i of the given perplexity."""
        raise NotImplementedError(f"{type(self).__name__} has no tsne_affinities")

    def tsne_symmetrize_ws_len(self, n: int) -> int:
        raise NotImplementedError(f"{type(self).__name__} has no tsne_symmetrize_ws_len")

    def tsne_symmetrize(self, P, partials):
        """In place: P = max((P + P^T) / 2n, 2.220446e-16), 0 on the diagonal; partials: sum p ln p per tile pair."""
        raise NotImplementedError(f"{type(self).__name__} has no tsne_symmetrize")

    def tsne_forces(self, P, Y, F, kl: bool = True, cached: bool = False):
        """F[i] = (attraction x, y; repulsion x, y; sum_{j != i} q_ij; with ``kl`` sum_j P_ij log1p(|y_i - y_j|^2))."""
        raise NotImplementedError(f"{type(self).__name__} has no tsne_forces")

    def tsne_step(self, F, Y, alpha: float, momentum: float, lr: float, plogp: float, V, G, Y_next, stats):
        """scikit-learn's gradient-descent update from the force sums; stats (float64 [4]) = KL, |g|, S, sum l."""
        raise NotImplementedError(f"{type(self).__name__} has no tsne_step")

    # neighbour-sparse 2-D layout (layout.py): optional in the same way -- KNeighbours and NeighbourTSNE are the only
    # callers.  ids int32 / sqdist, p float32 [n, k]; the joint P as CSR (rowptr int64 [n + 1], cols int32, val float32).
    def knn_sqdist(self, Z, d: int, rows, mu, sq, ids, sqdist, n_slabs: int = 1, cand_ids=None, cand_sqdist=None):
        """ids[i] = the positions in ``rows`` of the k nearest other listed rows of row i (distance ascending, ties by
        position), sqdist[i] their squared distances: tsne_sqdist's bits; -1 / +inf past the n - 1 other rows."""
        raise NotImplementedError(f"{type(self).__name__} has no knn_sqdist")

    def tsne_nn_affinities(self, sqdist, ids, perplexity: float, p, beta):
        """p[i] = the conditional affinities of row i over its k neighbours at the beta_i of the given perplexity."""
        raise NotImplementedError(f"{type(self).__name__} has no tsne_nn_affinities")

    def tsne_nn_plogp(self, rowptr, val, row_plogp):
        """row_plogp[i] (float64) = sum p ln p over CSR row i, in a fixed order."""
        raise NotImplementedError(f"{type(self).__name__} has no tsne_nn_plogp")

    def tsne_nn_attract(self, rowptr, cols, val, Y, F, kl: bool = True):
        """Columns 0, 1 (attraction) and 5 (with ``kl`` sum_j P_ij log1p(|y_i - y_j|^2), else 0) of F from the CSR rows."""
        raise NotImplementedError(f"{type(self).__name__} has no tsne_nn_attract")

    def tsne_repulse(self, Y, F):
        """Columns 2, 3 (repulsion) and 4 (sum_{j != i} q_ij) of F over all pairs."""
        raise NotImplementedError(f"{type(self).__name__} has no tsne_repulse")

    # silhouette (cluster.py): optional in the same way -- Silhouette is the only caller.  order: TABLE ROWS (int32) grouped
    # by cluster, seg int64 [K + 1] the clusters' starts in it; mu and nrm in the accumulate dtype.
    def silhouette_norms(self, Z, d: int, order, mu, metric: str, nrm):
        """nrm[p] of a_p = Z[order[p], :d] - mu: |a_p|^2 ("euclidean") or 1 / |a_p|, 0 for a zero row ("cosine"), the
        squared norm taken through the very contraction the dots of silhouette_sums run through."""
        raise NotImplementedError(f"{type(self).__name__} has no silhouette_norms")

    def silhouette_sums(self, Z, d: int, order, seg, mu, nrm, metric: str, p0: int, p1: int, S):
        """S[p - p0, c] (float64, [>= p1 - p0, K]) = the sum over the positions j of cluster c of dist(p, j), p in
        [p0, p1); the term j == p is exactly 0, an empty cluster's column zeros; the same bits for every [p0, p1)."""
        raise NotImplementedError(f"{type(self).__name__} has no silhouette_sums")

    # owned class rows (csrc/spmm_update.h, spmm_owned_kernel): optional in the same way -- a backend without them keeps
    # every class row on spmm_update_class, and SweepEngine asks `has_spmm_owned` before it plans for them
    def has_spmm_owned(self, dtype, d: int) -> bool:
        """Whether spmm_update_owned has an instance for tables of `dtype` and rows of `d` elements."""
        return False

    def make_owned_plan(self, plan: dict, chunk: int, device):
        """What spmm_update_owned takes as `plan`: xcd.owned_plan's arrays where the kernels read them."""
        raise NotImplementedError(f"{type(self).__name__} has no make_owned_plan")

    def spmm_update_owned(self, colidx, P, plan, block_threads: int, row0: int, Z_old, X, gamma: float, Z_new, d: int,
                          partials, beyond_cache: bool = False, loads: int = 0, ahead: bool = False):
        """The class rows of `plan` summed in LDS by row-owning workgroups, then the usual epilogue; writes
        partials[row_part[j]] for every row of the plan.  `ahead`: the epilogue requests the next rows' x / z_old before
        it finishes the current ones (no result depends on it; a backend may ignore it)."""
        raise NotImplementedError(f"{type(self).__name__} has no spmm_update_owned")

    # every column tile of a pass in one launch (csrc/spmm_update.h, the *_tiles_kernel forms): optional in the same way --
    # a backend without them keeps one launch per tile, and SweepEngine asks `has_spmm_tiles` before it plans for them.
    # Each takes the WHOLE tables (d columns) and `tile_cols`; tile t's partials start at partials[t * partials_stride].
    def has_spmm_tiles(self, dtype, d: int, tile_cols: int) -> bool:
        """Whether the spmm_update*_tiles calls take tables of `dtype`, `d` columns wide, in tiles of `tile_cols`."""
        return False

    owned_epilogue_ahead = False        # whether spmm_update_owned* take `ahead`: only then is it ever passed

    def spmm_update_tiles(self, rowptr, colidx, P, nrows: int, row0: int, Z_old, X, gamma: float, Z_new, d: int,
                          tile_cols: int, long_threshold: int, partials, partials_stride: int,
                          sinks_untouched: bool = False, beyond_cache: bool = False):
        """spmm_update for every column tile, one launch."""
        raise NotImplementedError(f"{type(self).__name__} has no spmm_update_tiles")

    def spmm_update_class_tiles(self, colidx, P, item_e0, item_len, item_slot, items_per_block: int, class_rows, slot_ptr,
                                n_slots: int, row0: int, Z_old, X, gamma: float, Z_new, d: int, tile_cols: int, slab,
                                partials, partials_stride: int, beyond_cache: bool = False):
        """spmm_update_class for every column tile: one chunk launch and one combine launch; `slab` holds
        tiles * spmm_class_slab_len(n_slots, tile_cols) elements."""
        raise NotImplementedError(f"{type(self).__name__} has no spmm_update_class_tiles")

    def spmm_update_owned_tiles(self, colidx, P, plan, block_threads: int, row0: int, Z_old, X, gamma: float, Z_new,
                                d: int, tile_cols: int, partials, partials_stride: int, beyond_cache: bool = False,
                                loads: int = 0, ahead: bool = False):
        """spmm_update_owned for every column tile, the tile loop inside the persistent workgroups."""
        raise NotImplementedError(f"{type(self).__name__} has no spmm_update_owned_tiles")

    # one weight per row instead of one per edge (csrc/spmm_update.h, UNIFORM): optional in the same way -- a backend
    # without them keeps the per-edge calls, and SweepEngine asks `has_row_weight` before it looks at P's rows.  Every
    # ``*_rw`` call is the call of the same name without the suffix with `row_weight` (one weight per row of the call)
    # where that takes P; the class calls also take `item_row` (after item_slot), the owned calls read the plan's seg_row.
    def has_row_weight(self, dtype) -> bool:
        """Whether row_weight and the spmm_update*_rw calls exist for tables of `dtype`."""
        return False

    def row_weight(self, rowptr, P, nrows: int, w, mixed):
        """w[r] = the first weight of row r (0 without edges); mixed[0] = 1 if a row of P holds two different bit
        patterns, else 0."""
        raise NotImplementedError(f"{type(self).__name__} has no row_weight")

    def bind(self, method: str, *args, **kwargs):
        """A zero-argument callable that makes the call ``method(*args, **kwargs)``; an implementation may
        pre-marshal it (HipKernels does)."""
        fn = getattr(self, method)
        return lambda: fn(*args, **kwargs)

    # new vertices (induct.py): optional in the same way -- NewVertexEmbedder is the only caller
    def embed_rows(self, rowptr, colidx, X_new, Z, table_rows: int, d: int, mode: int, sums2, sq, S, gamma: float,
                   tolerence: int, max_rounds: int, Z_out, rounds, delta, P_out=None, flags: int = 0):
        """The per-row fixed point of build_P + update on the frozen table Z for the rows of the CSR (rowptr, colidx =
        table rows): Z_out, rounds, delta and, where wanted, the soft-max weights P_out (csrc/new_rows.h)."""
        raise NotImplementedError(f"{type(self).__name__} has no embed_rows")


class HipKernels(KernelBackend):
    """Tensor-level view of the C ABI.  One instance per process is enough (stateless)."""

    owned_epilogue_ahead = True         # spmm_update_owned* take `ahead` (CLANE_OWNED_EPILOGUE_AHEAD)

    def __init__(self, lib: Optional[C.CDLL] = None):
        self.lib = lib if lib is not None else load_library()
        self._tls = threading.local()          # bind() records per thread: one instance serves every thread

    # -- helpers ------------------------------------------------------------------------
    def _invoke(self, fn, what: str, *cargs):
        """Call an ABI function now -- or, inside bind(), only record the bound call."""
        rec = getattr(self._tls, "recording", None)
        if rec is not None:
            rec.append((fn, cargs, what))
        else:
            self._check(fn(*cargs), what)

    def bind(self, method: str, *args, **kwargs):
        """The ABI call `method(*args, **kwargs)` would make, pre-marshalled: returns a zero-argument callable.
        Pointers, sizes and the CURRENT stream are captured now, so a sweep can replay a flat list of such
        calls without re-slicing tensors or re-checking arguments (host time per launch: ~3 us instead of ~25)."""
        self._tls.recording = []
        try:
            getattr(self, method)(*args, **kwargs)
            (fn, cargs, what), = self._tls.recording
        finally:
            self._tls.recording = None
        check = self._check
        return lambda: check(fn(*cargs), what)

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise ClaneHipError(f"{what} failed ({rc}): {self.lib.clane_last_error().decode()}")

    @staticmethod
    def _stream(t: torch.Tensor):
        if not t.is_cuda:
            raise ClaneHipError("HipKernels needs tensors in GPU memory (got a CPU tensor); there is no CPU path")
        return torch.cuda.current_stream(t.device).cuda_stream

    def _fn(self, base: str, dtype: torch.dtype):
        try:
            return getattr(self.lib, f"{base}_{_SUFFIX[dtype]}")
        except KeyError:
            raise TypeError(f"{base}: unsupported dtype {dtype}") from None

    # -- sizes --------------------------------------------------------------------------
    def spmm_partials_len(self, nrows: int, n_long: int) -> int:
        return int(self.lib.clane_spmm_partials_len(nrows, n_long))

    def xcc_ids(self, n_blocks: int, block_threads: int = 256, device=None) -> torch.Tensor:
        """XCD each workgroup of an n_blocks-workgroup launch ran on (int32 tensor on the device)."""
        out = torch.full((n_blocks,), -1, dtype=torch.int32, device=device if device is not None else "cuda")
        self._check(self.lib.clane_xcc_ids(out.data_ptr(), n_blocks, block_threads, self._stream(out)), "clane_xcc_ids")
        return out

    def check_csr(self, rowptr: torch.Tensor, colidx: torch.Tensor, nrows: int, n_edges: int, table_rows: int) -> None:
        """Raise ValueError unless rowptr[0..nrows] is non-decreasing within [0, n_edges] and colidx[:n_edges] holds
        rows of a table of ``table_rows`` rows (one pass on the device; blocks until it is done)."""
        if rowptr.dtype != torch.int64 or colidx.dtype != torch.int32 or rowptr.numel() < nrows + 1 or colidx.numel() < n_edges:
            raise ValueError("check_csr: rowptr must be int64 [nrows + 1], colidx int32 [n_edges]")
        status = torch.zeros(1, dtype=torch.int32, device=rowptr.device)
        self._check(self.lib.clane_check_csr(rowptr.data_ptr(), colidx.data_ptr(), nrows, n_edges, table_rows,
                                             status.data_ptr(), self._stream(rowptr)), "clane_check_csr")
        bad = int(status.item())
        if bad:
            what = [w for bit, w in ((1, "rowptr is not a non-decreasing sequence within [0, n_edges]"),
                                     (2, f"colidx holds entries outside [0, {table_rows})")) if bad & bit]
            raise ValueError("the CSR handed to the kernels is not valid: " + "; ".join(what))

    def build_info(self) -> str:
        return self.lib.clane_build_info().decode()

    def make_mirror(self, row_ptr, slot, bufs) -> Mirror:
        return Mirror(row_ptr, slot, bufs)

    def reduce_ws_len(self) -> int:
        return int(self.lib.clane_reduce_ws_len())

    def contiguous_matrix(self, shape, dtype: torch.dtype, device) -> DeviceBuffer:
        """A zeroed matrix of its own, physically contiguous allocation (raises ClaneHipError when none is to be had)."""
        return DeviceBuffer(self.lib, shape, dtype, device, contiguous=True)

    def shareable_matrix(self, shape, dtype: torch.dtype, device) -> DeviceBuffer:
        """Zero-filled device matrix that other processes can map (DeviceBuffer.export / .open)."""
        return DeviceBuffer(self.lib, shape, dtype, device)

    def open_shared_matrix(self, handle: bytes, shape, dtype: torch.dtype, device) -> DeviceBuffer:
        return DeviceBuffer.open(self.lib, handle, shape, dtype, device)

    # -- K0 -----------------------------------------------------------------------------
    def row_sqnorm(self, Z: torch.Tensor, d: int, sq: torch.Tensor):
        zp, ldz = _mat(Z, "Z")
        self._check(self._fn("clane_row_sqnorm", Z.dtype)(
            zp, Z.shape[0], d, ldz, _vec(sq, acc_dtype(Z.dtype), "sq"), self._stream(Z)), "clane_row_sqnorm")

    def degree_weighted_sums(self, sq, rowptr, indeg, nrows: int, ws, out2):
        self._check(self._fn("clane_degree_weighted_sums", sq.dtype)(
            _ptr(sq), _vec(rowptr, torch.int64, "rowptr"), _vec(indeg, torch.int32, "indeg"), nrows,
            _vec(ws, torch.float64, "ws"), _vec(out2, torch.float64, "out2"), self._stream(out2)),
            "clane_degree_weighted_sums")

    # -- K1 / K2 ------------------------------------------------------------------------
    def edge_score(self, rowptr, colidx, nrows: int, row0: int, Z, d: int, mode: int, sums2, sq, scores,
                   long_threshold: int = 0, long_rows=None, fuse_softmax: bool = False):
        zp, ldz = _mat(Z, "Z")
        n_long = 0 if long_rows is None else long_rows.numel()
        self._check(self._fn("clane_edge_score", Z.dtype)(
            _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"), nrows, row0, zp, ldz, d, mode,
            _ptr(sums2), _ptr(sq), _vec(scores, acc_dtype(Z.dtype), "scores"),
            SCORE_FUSE_SOFTMAX if fuse_softmax else 0, long_threshold,
            None if n_long == 0 else _vec(long_rows, torch.int32, "long_rows"), n_long,
            self._stream(Z)), "clane_edge_score")

    def edge_score_class(self, rowptr, colidx, item_e0, item_len, item_slot, item_row, items_per_block: int, class_rows,
                         slot_ptr, row0: int, Z, d: int, mode: int, sums2, sq, scores, stats=None,
                         fuse_softmax: bool = False, n_slots: Optional[int] = None, row_parts: int = 1):
        """K1 over the class rows' work items (XCD-affine gathers); with `fuse_softmax` every listed row leaves
        soft-maxed (stats: 2 accumulate-type elements per slot).  ``n_slots`` = slot_ptr[-1] when the caller knows it
        on the host (the engine does): without it the size check of `stats` reads it back from the device, which
        blocks the host on everything queued before this call."""
        zp, ldz = _mat(Z, "Z")
        n_blocks = self._item_blocks("edge_score_class", items_per_block, item_e0, item_len, item_slot, item_row)
        if fuse_softmax and (stats is None or stats.numel() < 2 * (int(slot_ptr[-1]) if n_slots is None else n_slots)):
            raise ValueError("edge_score_class: stats needs 2 elements per slot")
        acc = acc_dtype(Z.dtype)
        self._check(self._fn("clane_edge_score_class", Z.dtype)(
            _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"),
            _vec(item_e0, torch.int64, "item_e0"), _vec(item_len, torch.int32, "item_len"),
            _vec(item_slot, torch.int32, "item_slot"), _vec(item_row, torch.int32, "item_row"),
            n_blocks, items_per_block, _vec(class_rows, torch.int32, "class_rows"),
            _vec(slot_ptr, torch.int64, "slot_ptr"), class_rows.numel(), row0, zp, ldz, d, mode, _ptr(sums2), _ptr(sq),
            _vec(scores, acc, "scores"),
            (SCORE_FUSE_SOFTMAX | ((max(1, min(255, int(row_parts))) & 0xff) << 8)) if fuse_softmax else 0,
            None if stats is None else _vec(stats, acc, "stats"), self._stream(Z)), "clane_edge_score_class")

    def edge_score_finalize(self, rowptr, colidx, nrows: int, row0: int, mode: int, sums2, sq, scores):
        """RAW_DOT scores summed over the GPUs of a column-split run -> scores of `mode`, in place."""
        self._check(self._fn("clane_edge_score_finalize", scores.dtype)(
            _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"), nrows, row0, mode,
            _ptr(sums2), _ptr(sq), scores.data_ptr(), self._stream(scores)), "clane_edge_score_finalize")

    def segment_softmax(self, rowptr, nrows: int, vals, min_degree: int = 0, max_degree: int = 0, long_rows=None):
        n_long = 0 if long_rows is None else long_rows.numel()
        self._check(self._fn("clane_segment_softmax", vals.dtype)(
            _vec(rowptr, torch.int64, "rowptr"), nrows, vals.data_ptr(), min_degree, max_degree,
            None if n_long == 0 else _vec(long_rows, torch.int32, "long_rows"), n_long, self._stream(vals)),
            "clane_segment_softmax")

    # -- K3 -----------------------------------------------------------------------------
    @staticmethod
    def _sq_arg(sq: Optional[torch.Tensor], dtype: torch.dtype):
        return None if sq is None else _vec(sq, acc_dtype(dtype), "sq_a")

    @staticmethod
    def _tables(name: str, Z_old, X, Z_new, f32_only: bool = False):
        """The three tables of a K3 call, checked: (zo, ldz, xp, ldx, zn, ldo)."""
        zo, ldz = _mat(Z_old, "Z_old")
        xp, ldx = _mat(X, "X")
        zn, ldo = _mat(Z_new, "Z_new")
        if f32_only and not (Z_old.dtype == X.dtype == Z_new.dtype == torch.float32):
            raise TypeError(f"{name}: float32 tables only")
        if not (Z_old.dtype == X.dtype == Z_new.dtype):
            raise ValueError(f"{name}: Z_old, X, Z_new must share a dtype")
        return zo, ldz, xp, ldx, zn, ldo

    @staticmethod
    def _item_blocks(name: str, items_per_block: int, item_e0, *per_item) -> int:
        """The item blocks of a class pass whose arrays hold `items_per_block` items per block."""
        n_items = item_e0.numel()
        if n_items % items_per_block or any(t.numel() != n_items for t in per_item):
            raise ValueError(f"{name}: the item arrays must hold whole blocks of items_per_block items")
        return n_items // items_per_block

    @staticmethod
    def _spmm_flags(sinks_untouched: bool = False, beyond_cache: bool = False, loads: int = 0, ahead: bool = False) -> int:
        """The flag word of a K3 call (CLANE_SPMM_*; the owned pass: CLANE_OWNED_LOADS(n), CLANE_OWNED_EPILOGUE_AHEAD)."""
        return ((SPMM_SINKS_UNTOUCHED if sinks_untouched else 0) | (SPMM_TABLE_BEYOND_CACHE if beyond_cache else 0)
                | ((int(loads) & 0xff) << 8) | (OWNED_EPILOGUE_AHEAD if ahead else 0))

    @staticmethod
    def _owned_plan_fits(name: str, plan: OwnedPlan, width: int, colidx, P, row0: int, Z_old, X, Z_new, partials=None):
        """The sums of a batch fit the LDS at rows of `width` columns, and the plan stays inside what the call is given
        (`partials`: where the caller has not checked them tile by tile)."""
        lanes = 32 if width <= 128 else 64
        if plan.max_batch_vrows * lanes * 16 > OWNED_LDS_LIMIT:
            raise ValueError(f"{name}: {plan.max_batch_vrows} virtual rows per batch do not fit the LDS")
        if (plan.max_edge > min(colidx.numel(), P.numel()) or plan.max_row >= min(X.shape[0], Z_new.shape[0])
                or row0 + plan.max_row >= Z_old.shape[0] or (partials is not None and plan.max_part >= partials.numel())):
            raise ValueError(f"{name}: the plan reaches outside colidx / P, the tables or the partials")

    def spmm_update(self, rowptr, colidx, P, nrows: int, row0: int, Z_old, X, gamma: float, Z_new, d: int,
                    long_threshold: int, partials, sinks_untouched: bool = False, mirror: Optional[Mirror] = None,
                    beyond_cache: bool = False):
        """Main pass: every row of <= long_threshold edges (0 = all rows).  With `sinks_untouched` rows
        without out-edges are neither read nor written (caller keeps Z_new == Z_old there).  `beyond_cache`: the hint
        CLANE_SPMM_TABLE_BEYOND_CACHE (the table is far beyond the caches; results do not depend on it)."""
        zo, ldz, xp, ldx, zn, ldo = self._tables("spmm_update", Z_old, X, Z_new)
        self._invoke(self._fn("clane_spmm_update", Z_old.dtype), "clane_spmm_update",
                     _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"),
                     _vec(P, acc_dtype(Z_old.dtype), "P"), nrows, row0, zo, ldz, xp, ldx, gamma, zn, ldo, d,
                     long_threshold, self._spmm_flags(sinks_untouched, beyond_cache),
                     _mirror_arg(mirror, Z_new.dtype), _vec(partials, torch.float64, "partials"), self._stream(Z_old))

    def spmm_update_long(self, rowptr, colidx, P, long_rows, waves_per_row: int, row0: int, Z_old, X, gamma: float,
                         Z_new, d: int, partials, mirror: Optional[Mirror] = None):
        """Row-split pass: one workgroup of `waves_per_row` (4 | 16) waves per listed row; writes
        long_rows.numel() partials."""
        zo, ldz, xp, ldx, zn, ldo = self._tables("spmm_update_long", Z_old, X, Z_new)
        self._invoke(self._fn("clane_spmm_update_long", Z_old.dtype), "clane_spmm_update_long",
                     _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"),
                     _vec(P, acc_dtype(Z_old.dtype), "P"), _vec(long_rows, torch.int32, "long_rows"),
                     long_rows.numel(), waves_per_row, row0, zo, ldz, xp, ldx, gamma, zn, ldo, d,
                     _mirror_arg(mirror, Z_new.dtype), _vec(partials, torch.float64, "partials"), self._stream(Z_old))

    def spmm_split_slab_len(self, n_segments: int, d: int) -> int:
        return int(self.lib.clane_spmm_split_slab_len(n_segments, d))

    def spmm_update_split(self, rowptr, colidx, P, split_rows, seg_ptr, seg_row, edges_per_segment: int, row0: int,
                          Z_old, X, gamma: float, Z_new, d: int, slab, partials, mirror: Optional[Mirror] = None):
        """Hub rows cut into segments over several workgroups + fixed-order combine; writes split_rows.numel()
        partials."""
        zo, ldz, xp, ldx, zn, ldo = self._tables("spmm_update_split", Z_old, X, Z_new)
        self._invoke(self._fn("clane_spmm_update_split", Z_old.dtype), "clane_spmm_update_split",
                     _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"),
                     _vec(P, acc_dtype(Z_old.dtype), "P"), _vec(split_rows, torch.int32, "split_rows"),
                     _vec(seg_ptr, torch.int64, "seg_ptr"), _vec(seg_row, torch.int32, "seg_row"),
                     split_rows.numel(), seg_row.numel(), edges_per_segment, row0, zo, ldz, xp, ldx, gamma, zn, ldo, d,
                     _vec(slab, acc_dtype(Z_old.dtype), "slab"), _mirror_arg(mirror, Z_new.dtype),
                     _vec(partials, torch.float64, "partials"), self._stream(Z_old))

    def spmm_class_slab_len(self, n_slots: int, d: int) -> int:
        return int(self.lib.clane_spmm_class_slab_len(n_slots, d))

    def spmm_update_class(self, colidx, P, item_e0, item_len, item_slot, items_per_block: int, class_rows, slot_ptr,
                          row0: int, Z_old, X, gamma: float, Z_new, d: int, slab, partials,
                          mirror: Optional[Mirror] = None, beyond_cache: bool = False):
        """XCD-affine pass over the listed long rows (edges sorted by (XCD class of the column, column), cut into items; item
        blocks of class b at block index 8 j + b) + fixed-order combine; writes class_rows.numel() partials."""
        zo, ldz, xp, ldx, zn, ldo = self._tables("spmm_update_class", Z_old, X, Z_new)
        n_blocks = self._item_blocks("spmm_update_class", items_per_block, item_e0, item_len, item_slot)
        self._invoke(self._fn("clane_spmm_update_class", Z_old.dtype), "clane_spmm_update_class",
                     _vec(colidx, torch.int32, "colidx"), _vec(P, acc_dtype(Z_old.dtype), "P"),
                     _vec(item_e0, torch.int64, "item_e0"), _vec(item_len, torch.int32, "item_len"),
                     _vec(item_slot, torch.int32, "item_slot"), n_blocks, items_per_block,
                     _vec(class_rows, torch.int32, "class_rows"), _vec(slot_ptr, torch.int64, "slot_ptr"),
                     class_rows.numel(), row0, zo, ldz, xp, ldx, gamma, zn, ldo, d,
                     self._spmm_flags(beyond_cache=beyond_cache), _vec(slab, acc_dtype(Z_old.dtype), "slab"),
                     _mirror_arg(mirror, Z_new.dtype), _vec(partials, torch.float64, "partials"), self._stream(Z_old))

    def has_spmm_owned(self, dtype, d: int) -> bool:
        return dtype == torch.float32 and 64 < d <= 256        # 16-byte packs at 32 or 64 lanes per row

    def make_owned_plan(self, plan: dict, chunk: int, device) -> OwnedPlan:
        return OwnedPlan(plan, chunk, device)

    def spmm_update_owned(self, colidx, P, plan: OwnedPlan, block_threads: int, row0: int, Z_old, X, gamma: float,
                          Z_new, d: int, partials, beyond_cache: bool = False, loads: int = 0, ahead: bool = False):
        """Class rows summed in LDS by row-owning workgroups (no slab, no combine); writes partials[row_part[j]].
        `loads`: CLANE_OWNED_LOADS, row loads in flight per wave (0 = the chunk kernel's choice); `ahead`:
        CLANE_OWNED_EPILOGUE_AHEAD."""
        zo, ldz, xp, ldx, zn, ldo = self._tables("spmm_update_owned", Z_old, X, Z_new, f32_only=True)
        self._owned_plan_fits("spmm_update_owned", plan, d, colidx, P, row0, Z_old, X, Z_new, partials)
        self._invoke(self.lib.clane_spmm_update_owned_f32, "clane_spmm_update_owned",
                     _vec(colidx, torch.int32, "colidx"), _vec(P, torch.float32, "P"), C.cast(C.pointer(plan.c), _p),
                     int(block_threads), row0, zo, ldz, xp, ldx, gamma, zn, ldo, d,
                     self._spmm_flags(beyond_cache=beyond_cache, loads=loads, ahead=ahead),
                     _vec(partials, torch.float64, "partials"), self._stream(Z_old))

    # -- every column tile of a pass in one launch ----------------------------------------------------------
    def has_spmm_tiles(self, dtype, d: int, tile_cols: int) -> bool:
        """fp32, tiles of whole 16-byte packs, and a last tile with the lane layout of a full one (the fused launch runs
        one kernel instance for all tiles)."""
        if dtype != torch.float32 or not 0 < tile_cols <= d or tile_cols % 4:
            return False
        lanes = lambda w: next(n for n in (8, 16, 32, 64) if -(-w // 4) <= n or n == 64)       # noqa: E731
        return lanes(d - (-(-d // tile_cols) - 1) * tile_cols) == lanes(tile_cols)

    def _tile_args(self, name, Z_old, X, Z_new, d, tile_cols, partials, partials_stride, per_tile):
        """The three whole tables of a fused call and its partials, checked: (zo, ldz, xp, ldx, zn, ldo)."""
        tables = self._tables(name, Z_old, X, Z_new, f32_only=True)
        if not self.has_spmm_tiles(torch.float32, d, tile_cols) or min(Z_old.shape[1], X.shape[1], Z_new.shape[1]) < d:
            raise ValueError(f"{name}: no fused launch for d={d} in tiles of {tile_cols} columns")
        tiles = -(-d // tile_cols)
        if (tiles > 1 and partials_stride < per_tile) or partials.numel() < (tiles - 1) * partials_stride + per_tile:
            raise ValueError(f"{name}: the tiles' partials overlap or end outside `partials`")
        return tables

    def spmm_update_tiles(self, rowptr, colidx, P, nrows: int, row0: int, Z_old, X, gamma: float, Z_new, d: int,
                          tile_cols: int, long_threshold: int, partials, partials_stride: int,
                          sinks_untouched: bool = False, beyond_cache: bool = False):
        """The row pass of every column tile in one launch: a tile-major grid of tiles x workgroups."""
        zo, ldz, xp, ldx, zn, ldo = self._tile_args("spmm_update_tiles", Z_old, X, Z_new, d, tile_cols, partials,
                                                    partials_stride, self.spmm_partials_len(nrows, 0))
        self._invoke(self.lib.clane_spmm_update_tiles_f32, "clane_spmm_update_tiles",
                     _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"), _vec(P, torch.float32, "P"),
                     nrows, row0, zo, ldz, xp, ldx, gamma, zn, ldo, d, tile_cols, long_threshold,
                     self._spmm_flags(sinks_untouched, beyond_cache),
                     _vec(partials, torch.float64, "partials"), partials_stride, self._stream(Z_old))

    def spmm_update_class_tiles(self, colidx, P, item_e0, item_len, item_slot, items_per_block: int, class_rows, slot_ptr,
                                n_slots: int, row0: int, Z_old, X, gamma: float, Z_new, d: int, tile_cols: int, slab,
                                partials, partials_stride: int, beyond_cache: bool = False):
        """Chunk + combine of every column tile, one launch each; tile t's chunk sums at
        slab[t * spmm_class_slab_len(n_slots, tile_cols):]."""
        zo, ldz, xp, ldx, zn, ldo = self._tile_args("spmm_update_class_tiles", Z_old, X, Z_new, d, tile_cols, partials,
                                                    partials_stride, class_rows.numel())
        n_blocks = self._item_blocks("spmm_update_class_tiles", items_per_block, item_e0, item_len, item_slot)
        if slab.numel() < -(-d // tile_cols) * self.spmm_class_slab_len(n_slots, tile_cols):
            raise ValueError("spmm_update_class_tiles: the slab does not hold every tile's chunk sums")
        self._invoke(self.lib.clane_spmm_update_class_tiles_f32, "clane_spmm_update_class_tiles",
                     _vec(colidx, torch.int32, "colidx"), _vec(P, torch.float32, "P"),
                     _vec(item_e0, torch.int64, "item_e0"), _vec(item_len, torch.int32, "item_len"),
                     _vec(item_slot, torch.int32, "item_slot"), n_blocks, items_per_block,
                     _vec(class_rows, torch.int32, "class_rows"), _vec(slot_ptr, torch.int64, "slot_ptr"),
                     class_rows.numel(), n_slots, row0, zo, ldz, xp, ldx, gamma, zn, ldo, d, tile_cols,
                     self._spmm_flags(beyond_cache=beyond_cache), _vec(slab, torch.float32, "slab"),
                     _vec(partials, torch.float64, "partials"), partials_stride, self._stream(Z_old))

    def spmm_update_owned_tiles(self, colidx, P, plan: OwnedPlan, block_threads: int, row0: int, Z_old, X, gamma: float,
                                Z_new, d: int, tile_cols: int, partials, partials_stride: int, beyond_cache: bool = False,
                                loads: int = 0, ahead: bool = False):
        """The owned pass of every column tile in one launch: the tile loop runs inside the persistent workgroups."""
        zo, ldz, xp, ldx, zn, ldo = self._tile_args("spmm_update_owned_tiles", Z_old, X, Z_new, d, tile_cols, partials,
                                                    partials_stride, plan.max_part + 1)
        if not self.has_spmm_owned(torch.float32, tile_cols):
            raise ValueError(f"spmm_update_owned_tiles: no owned instance for tiles of {tile_cols} columns")
        self._owned_plan_fits("spmm_update_owned_tiles", plan, tile_cols, colidx, P, row0, Z_old, X, Z_new)
        self._invoke(self.lib.clane_spmm_update_owned_tiles_f32, "clane_spmm_update_owned_tiles",
                     _vec(colidx, torch.int32, "colidx"), _vec(P, torch.float32, "P"), C.cast(C.pointer(plan.c), _p),
                     int(block_threads), row0, zo, ldz, xp, ldx, gamma, zn, ldo, d, tile_cols,
                     self._spmm_flags(beyond_cache=beyond_cache, loads=loads, ahead=ahead),
                     _vec(partials, torch.float64, "partials"), partials_stride, self._stream(Z_old))

    # -- one weight per row instead of one per edge --------------------------------------------------------------
    def has_row_weight(self, dtype) -> bool:
        return dtype == torch.float32

    def row_weight(self, rowptr, P, nrows: int, w, mixed):
        if w.dtype != P.dtype or w.numel() < nrows or rowptr.numel() < nrows + 1:
            raise ValueError("row_weight: w must hold one weight of P's dtype per row of rowptr")
        self._invoke(self._fn("clane_row_weight", P.dtype), "clane_row_weight", _vec(rowptr, torch.int64, "rowptr"),
                     _vec(P, P.dtype, "P"), nrows, _vec(w, P.dtype, "w"), _vec(mixed, torch.int32, "mixed"),
                     self._stream(P))

    @staticmethod
    def _row_weights(name: str, w, rows: int):
        """The `row_weight` argument of a *_rw call that reads the weights of rows [0, rows)."""
        if w.numel() < rows:
            raise ValueError(f"{name}: row_weight holds {w.numel()} rows, the call reads {rows}")
        return _vec(w, torch.float32, "row_weight")

    def spmm_update_rw(self, rowptr, colidx, row_weight, nrows: int, row0: int, Z_old, X, gamma: float, Z_new, d: int,
                       long_threshold: int, partials, sinks_untouched: bool = False, beyond_cache: bool = False):
        zo, ldz, xp, ldx, zn, ldo = self._tables("spmm_update_rw", Z_old, X, Z_new, f32_only=True)
        self._invoke(self.lib.clane_spmm_update_rw_f32, "clane_spmm_update_rw",
                     _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"),
                     self._row_weights("spmm_update_rw", row_weight, nrows), nrows, row0, zo, ldz, xp, ldx, gamma, zn, ldo,
                     d, long_threshold, self._spmm_flags(sinks_untouched, beyond_cache),
                     _vec(partials, torch.float64, "partials"), self._stream(Z_old))

    def spmm_update_tiles_rw(self, rowptr, colidx, row_weight, nrows: int, row0: int, Z_old, X, gamma: float, Z_new,
                             d: int, tile_cols: int, long_threshold: int, partials, partials_stride: int,
                             sinks_untouched: bool = False, beyond_cache: bool = False):
        zo, ldz, xp, ldx, zn, ldo = self._tile_args("spmm_update_tiles_rw", Z_old, X, Z_new, d, tile_cols, partials,
                                                    partials_stride, self.spmm_partials_len(nrows, 0))
        self._invoke(self.lib.clane_spmm_update_tiles_rw_f32, "clane_spmm_update_tiles_rw",
                     _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"),
                     self._row_weights("spmm_update_tiles_rw", row_weight, nrows), nrows, row0, zo, ldz, xp, ldx, gamma,
                     zn, ldo, d, tile_cols, long_threshold, self._spmm_flags(sinks_untouched, beyond_cache),
                     _vec(partials, torch.float64, "partials"), partials_stride, self._stream(Z_old))

    def spmm_update_class_rw(self, colidx, row_weight, item_e0, item_len, item_slot, item_row, items_per_block: int,
                             class_rows, slot_ptr, row0: int, Z_old, X, gamma: float, Z_new, d: int, slab, partials,
                             beyond_cache: bool = False):
        zo, ldz, xp, ldx, zn, ldo = self._tables("spmm_update_class_rw", Z_old, X, Z_new, f32_only=True)
        n_blocks = self._item_blocks("spmm_update_class_rw", items_per_block, item_e0, item_len, item_slot, item_row)
        rows = int(class_rows.max()) + 1 if class_rows.numel() else 0          # item_row holds class rows only
        self._invoke(self.lib.clane_spmm_update_class_rw_f32, "clane_spmm_update_class_rw",
                     _vec(colidx, torch.int32, "colidx"), self._row_weights("spmm_update_class_rw", row_weight, rows),
                     _vec(item_e0, torch.int64, "item_e0"), _vec(item_len, torch.int32, "item_len"),
                     _vec(item_slot, torch.int32, "item_slot"), _vec(item_row, torch.int32, "item_row"), n_blocks,
                     items_per_block, _vec(class_rows, torch.int32, "class_rows"), _vec(slot_ptr, torch.int64, "slot_ptr"),
                     class_rows.numel(), row0, zo, ldz, xp, ldx, gamma, zn, ldo, d,
                     self._spmm_flags(beyond_cache=beyond_cache), _vec(slab, torch.float32, "slab"),
                     _vec(partials, torch.float64, "partials"), self._stream(Z_old))

    def spmm_update_class_tiles_rw(self, colidx, row_weight, item_e0, item_len, item_slot, item_row, items_per_block: int,
                                   class_rows, slot_ptr, n_slots: int, row0: int, Z_old, X, gamma: float, Z_new, d: int,
                                   tile_cols: int, slab, partials, partials_stride: int, beyond_cache: bool = False):
        zo, ldz, xp, ldx, zn, ldo = self._tile_args("spmm_update_class_tiles_rw", Z_old, X, Z_new, d, tile_cols, partials,
                                                    partials_stride, class_rows.numel())
        n_blocks = self._item_blocks("spmm_update_class_tiles_rw", items_per_block, item_e0, item_len, item_slot, item_row)
        if slab.numel() < -(-d // tile_cols) * self.spmm_class_slab_len(n_slots, tile_cols):
            raise ValueError("spmm_update_class_tiles_rw: the slab does not hold every tile's chunk sums")
        rows = int(class_rows.max()) + 1 if class_rows.numel() else 0
        self._invoke(self.lib.clane_spmm_update_class_tiles_rw_f32, "clane_spmm_update_class_tiles_rw",
                     _vec(colidx, torch.int32, "colidx"), self._row_weights("spmm_update_class_tiles_rw", row_weight, rows),
                     _vec(item_e0, torch.int64, "item_e0"), _vec(item_len, torch.int32, "item_len"),
                     _vec(item_slot, torch.int32, "item_slot"), _vec(item_row, torch.int32, "item_row"), n_blocks,
                     items_per_block, _vec(class_rows, torch.int32, "class_rows"), _vec(slot_ptr, torch.int64, "slot_ptr"),
                     class_rows.numel(), n_slots, row0, zo, ldz, xp, ldx, gamma, zn, ldo, d, tile_cols,
                     self._spmm_flags(beyond_cache=beyond_cache), _vec(slab, torch.float32, "slab"),
                     _vec(partials, torch.float64, "partials"), partials_stride, self._stream(Z_old))

    def spmm_update_owned_rw(self, colidx, row_weight, plan: OwnedPlan, block_threads: int, row0: int, Z_old, X,
                             gamma: float, Z_new, d: int, partials, beyond_cache: bool = False, loads: int = 0,
                             ahead: bool = False):
        zo, ldz, xp, ldx, zn, ldo = self._tables("spmm_update_owned_rw", Z_old, X, Z_new, f32_only=True)
        self._owned_plan_fits("spmm_update_owned_rw", plan, d, colidx, colidx, row0, Z_old, X, Z_new, partials)
        self._invoke(self.lib.clane_spmm_update_owned_rw_f32, "clane_spmm_update_owned_rw",
                     _vec(colidx, torch.int32, "colidx"),
                     self._row_weights("spmm_update_owned_rw", row_weight, plan.max_row + 1),
                     C.cast(C.pointer(plan.c), _p), _vec(plan.seg_row, torch.int32, "seg_row"), int(block_threads), row0,
                     zo, ldz, xp, ldx, gamma, zn, ldo, d,
                     self._spmm_flags(beyond_cache=beyond_cache, loads=loads, ahead=ahead),
                     _vec(partials, torch.float64, "partials"), self._stream(Z_old))

    def spmm_update_owned_tiles_rw(self, colidx, row_weight, plan: OwnedPlan, block_threads: int, row0: int, Z_old, X,
                                   gamma: float, Z_new, d: int, tile_cols: int, partials, partials_stride: int,
                                   beyond_cache: bool = False, loads: int = 0, ahead: bool = False):
        zo, ldz, xp, ldx, zn, ldo = self._tile_args("spmm_update_owned_tiles_rw", Z_old, X, Z_new, d, tile_cols, partials,
                                                    partials_stride, plan.max_part + 1)
        if not self.has_spmm_owned(torch.float32, tile_cols):
            raise ValueError(f"spmm_update_owned_tiles_rw: no owned instance for tiles of {tile_cols} columns")
        self._owned_plan_fits("spmm_update_owned_tiles_rw", plan, tile_cols, colidx, colidx, row0, Z_old, X, Z_new)
        self._invoke(self.lib.clane_spmm_update_owned_tiles_rw_f32, "clane_spmm_update_owned_tiles_rw",
                     _vec(colidx, torch.int32, "colidx"),
                     self._row_weights("spmm_update_owned_tiles_rw", row_weight, plan.max_row + 1),
                     C.cast(C.pointer(plan.c), _p), _vec(plan.seg_row, torch.int32, "seg_row"), int(block_threads), row0,
                     zo, ldz, xp, ldx, gamma, zn, ldo, d, tile_cols,
                     self._spmm_flags(beyond_cache=beyond_cache, loads=loads, ahead=ahead),
                     _vec(partials, torch.float64, "partials"), partials_stride, self._stream(Z_old))

    def reduce_partials(self, partials, n: int, ws, out):
        self._invoke(self.lib.clane_reduce_partials, "clane_reduce_partials",
                     _vec(partials, torch.float64, "partials"), n, _vec(ws, torch.float64, "ws"),
                     _vec(out, torch.float64, "out"), self._stream(out))

    def l1_distance(self, A, B, d: int, ws, out, sq_a: Optional[torch.Tensor] = None):
        """out[0] = sum|A - B|; with `sq_a` also the squared norm of every row of A (bit for bit row_sqnorm's)."""
        ap, lda = _mat(A, "A")
        bp, ldb = _mat(B, "B")
        self._check(self._fn("clane_l1_distance", A.dtype)(
            ap, lda, bp, ldb, A.shape[0], d, self._sq_arg(sq_a, A.dtype), _vec(ws, torch.float64, "ws"),
            _vec(out, torch.float64, "out"), self._stream(A)), "clane_l1_distance")

    def gather_rows(self, src, idx, d: int, dst):
        """dst[i, :] = src[idx[i], :] (send-buffer packing of the halo exchange)."""
        sp, lds = _mat(src, "src")
        dp, ldd = _mat(dst, "dst")
        self._invoke(self._fn("clane_gather_rows", src.dtype), "clane_gather_rows",
                     sp, lds, _vec(idx, torch.int32, "idx"), idx.numel(), d, dp, ldd, self._stream(src))

    # -- bilinear similarity -------------------------------------------------------------
    def project_rows(self, Z, d: int, W, Y):
        """Y[r, :2d] = W . Z[r, :d] for every row r of Z (MFMA).  W: [2d, d] contiguous, Y: [rows(Z), >= 2d], both in
        the accumulate dtype of Z."""
        zp, ldz = _mat(Z, "Z")
        yp, ldy = _mat(Y, "Y")
        acc = acc_dtype(Z.dtype)
        if tuple(W.shape) != (2 * d, d):
            raise ValueError(f"project_rows: W must be [2d, d] = [{2 * d}, {d}], got {tuple(W.shape)}")
        if Y.dtype != acc or Y.shape[0] < Z.shape[0]:
            raise ValueError(f"project_rows: Y must be {acc} with at least {Z.shape[0]} rows")
        self._check(self._fn("clane_project_rows", Z.dtype)(
            zp, Z.shape[0], d, ldz, _vec(W, acc, "W"), yp, ldy, self._stream(Z)), "clane_project_rows")

    def edge_score_pair(self, rowptr, colidx, nrows: int, row0: int, S, N, d: int, scores, long_threshold: int = 0,
                        long_rows=None, fuse_softmax: bool = False):
        """K1 with two tables: score of edge (r, c) = dot(S[row0 + r, :d], N[c, :d]) (S = Y[:, :d], N = Y[:, d:]
        for the bilinear similarity); long rows and fused softmax as edge_score."""
        sp, lds = _mat(S, "S")
        np_, ldn = _mat(N, "N")
        if S.dtype != N.dtype:
            raise ValueError("edge_score_pair: S and N must share a dtype")
        n_long = 0 if long_rows is None else long_rows.numel()
        self._check(self._fn("clane_edge_score_pair", S.dtype)(
            _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"), nrows, row0, sp, lds, np_, ldn, d,
            _vec(scores, S.dtype, "scores"), SCORE_FUSE_SOFTMAX if fuse_softmax else 0, long_threshold,
            None if n_long == 0 else _vec(long_rows, torch.int32, "long_rows"), n_long,
            self._stream(S)), "clane_edge_score_pair")

    def edge_score_class_pair(self, rowptr, colidx, item_e0, item_len, item_slot, item_row, items_per_block: int,
                              class_rows, slot_ptr, row0: int, S, N, d: int, scores, stats=None,
                              fuse_softmax: bool = False, n_slots: Optional[int] = None, row_parts: int = 1):
        """edge_score_class with two tables, as edge_score_pair."""
        sp, lds = _mat(S, "S")
        np_, ldn = _mat(N, "N")
        if S.dtype != N.dtype:
            raise ValueError("edge_score_class_pair: S and N must share a dtype")
        n_blocks = self._item_blocks("edge_score_class_pair", items_per_block, item_e0, item_len, item_slot, item_row)
        if fuse_softmax and (stats is None or stats.numel() < 2 * (int(slot_ptr[-1]) if n_slots is None else n_slots)):
            raise ValueError("edge_score_class_pair: stats needs 2 elements per slot")
        self._check(self._fn("clane_edge_score_class_pair", S.dtype)(
            _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"),
            _vec(item_e0, torch.int64, "item_e0"), _vec(item_len, torch.int32, "item_len"),
            _vec(item_slot, torch.int32, "item_slot"), _vec(item_row, torch.int32, "item_row"),
            n_blocks, items_per_block, _vec(class_rows, torch.int32, "class_rows"),
            _vec(slot_ptr, torch.int64, "slot_ptr"), class_rows.numel(), row0, sp, lds, np_, ldn, d,
            _vec(scores, S.dtype, "scores"),
            (SCORE_FUSE_SOFTMAX | ((max(1, min(255, int(row_parts))) & 0xff) << 8)) if fuse_softmax else 0,
            None if stats is None else _vec(stats, S.dtype, "stats"), self._stream(S)), "clane_edge_score_class_pair")

    # -- training the bilinear similarity ------------------------------------------------
    @staticmethod
    def _pairs(src, dst, what: str) -> int:
        if src.numel() != dst.numel():
            raise ValueError(f"{what}: src and dst must have one entry per pair")
        return src.numel()

    def _pair_mats(self, A, Bm, B: int, d: int, acc, what: str):
        for t, name in ((A, "A"), (Bm, "Bm")):
            if t.dtype != acc or not t.is_contiguous() or t.numel() < B * d:
                raise ValueError(f"{what}: {name} must be a contiguous {acc} tensor of at least B * d elements")
        return A.data_ptr(), Bm.data_ptr()

    def pair_project(self, Z, d: int, src, dst, W, A, Bm):
        zp, ldz = _mat(Z, "Z")
        acc = acc_dtype(Z.dtype)
        B = self._pairs(src, dst, "pair_project")
        if tuple(W.shape) != (2 * d, d):
            raise ValueError(f"pair_project: W must be [2d, d] = [{2 * d}, {d}], got {tuple(W.shape)}")
        ap, bp = self._pair_mats(A, Bm, B, d, acc, "pair_project")
        self._invoke(self._fn("clane_pair_project", Z.dtype), "clane_pair_project",
                     zp, Z.shape[0], d, ldz, _vec(src, torch.int32, "src"), _vec(dst, torch.int32, "dst"), B,
                     _vec(W, acc, "W"), ap, bp, self._stream(Z))

    def pair_loss(self, A, Bm, d: int, linked, u, g, mask, ws, stats):
        B = linked.numel()
        acc = A.dtype
        ap, bp = self._pair_mats(A, Bm, B, d, acc, "pair_loss")
        if u.numel() != B or g.numel() < B or mask.numel() < B or stats.numel() < 2 or ws.numel() < self.reduce_ws_len():
            raise ValueError("pair_loss: u, g, mask need one entry per pair, stats 2 and ws reduce_ws_len() doubles")
        self._invoke(self._fn("clane_pair_loss", acc), "clane_pair_loss",
                     ap, bp, B, d, _vec(linked, torch.uint8, "linked"), _vec(u, acc, "u"), _vec(g, acc, "g"),
                     _vec(mask, torch.uint8, "mask"), _vec(ws, torch.float64, "ws"), _vec(stats, torch.float64, "stats"),
                     self._stream(A))

    def pair_grad_ws_len(self, B: int, d: int) -> int:
        return int(self.lib.clane_pair_grad_ws_len(B, d))

    def pair_grad(self, Z, d: int, src, dst, A, Bm, g, stats, ws, dW):
        zp, ldz = _mat(Z, "Z")
        acc = acc_dtype(Z.dtype)
        B = self._pairs(src, dst, "pair_grad")
        ap, bp = self._pair_mats(A, Bm, B, d, acc, "pair_grad")
        if g.numel() < B or ws.numel() < self.pair_grad_ws_len(B, d) or dW.numel() != 2 * d * d:
            raise ValueError("pair_grad: g needs one entry per pair, ws pair_grad_ws_len(B, d) elements, dW 2 d^2")
        self._invoke(self._fn("clane_pair_grad", Z.dtype), "clane_pair_grad",
                     zp, Z.shape[0], d, ldz, _vec(src, torch.int32, "src"), _vec(dst, torch.int32, "dst"), B, ap, bp,
                     _vec(g, acc, "g"), _vec(stats, torch.float64, "stats"), _vec(ws, acc, "ws"), _vec(dW, acc, "dW"),
                     self._stream(Z))

    def adam_step(self, W, m, v, dW, lr: float, stats, state):
        if not (W.numel() == m.numel() == v.numel() == dW.numel()) or state.numel() < 2:
            raise ValueError("adam_step: W, m, v, dW must have one length, state 2 doubles")
        self._invoke(self._fn("clane_adam_step", W.dtype), "clane_adam_step",
                     _vec(W, W.dtype, "W"), _vec(m, W.dtype, "m"), _vec(v, W.dtype, "v"), _vec(dW, W.dtype, "dW"),
                     W.numel(), float(lr), _vec(stats, torch.float64, "stats"), _vec(state, torch.float64, "state"),
                     self._stream(W))

    def pair_labels(self, rowptr, colidx, nrows: int, src, dst, linked):
        B = self._pairs(src, dst, "pair_labels")
        if rowptr.numel() < nrows + 1 or linked.numel() < B:
            raise ValueError("pair_labels: rowptr needs nrows + 1 entries, linked one per pair")
        self._invoke(self.lib.clane_pair_labels, "clane_pair_labels",
                     _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"), nrows,
                     _vec(src, torch.int32, "src"), _vec(dst, torch.int32, "dst"), B,
                     _vec(linked, torch.uint8, "linked"), self._stream(linked))

    # -- link prediction -----------------------------------------------------------------
    @staticmethod
    def _two_tables(S, N, table_rows: int, d: int, what: str):
        sp, lds = _mat(S, "S")
        np_, ldn = _mat(N, "N")
        if S.dtype != N.dtype:
            raise ValueError(f"{what}: S and N must share a dtype")
        if S.shape[0] < table_rows or N.shape[0] < table_rows or S.shape[1] < d or N.shape[1] < d:
            raise ValueError(f"{what}: S and N must hold at least {table_rows} rows of {d} columns")
        return sp, lds, np_, ldn

    def rank_scores(self, S, N, table_rows: int, d: int, q_rows, mode: int, sums2, sq, label, excl_rowptr, excl_colidx,
                    exclude_self: bool, k: int, n_slabs: int, cand_score, cand_id):
        sp, lds, np_, ldn = self._two_tables(S, N, table_rows, d, "rank_scores")
        acc, Q = acc_dtype(S.dtype), q_rows.numel()
        for t, n, name in ((sq, table_rows, "sq"), (label, table_rows, "label"), (excl_rowptr, table_rows + 1, "excl_rowptr")):
            if t is not None and t.numel() < n:
                raise ValueError(f"rank_scores: {name} needs {n} entries")
        need = Q * max(int(n_slabs), 0) * max(int(k), 0)
        if cand_score.numel() < need or cand_id.numel() < need:
            raise ValueError("rank_scores: cand_score and cand_id need Q * n_slabs * k entries")
        self._invoke(self._fn("clane_rank_scores", S.dtype), "clane_rank_scores",
                     sp, lds, np_, ldn, table_rows, d, _vec(q_rows, torch.int32, "q_rows"), Q, mode, _ptr(sums2),
                     None if sq is None else _vec(sq, acc, "sq"),
                     None if label is None else _vec(label, torch.int32, "label"),
                     None if excl_rowptr is None else _vec(excl_rowptr, torch.int64, "excl_rowptr"),
                     None if excl_colidx is None else _vec(excl_colidx, torch.int32, "excl_colidx"),
                     int(bool(exclude_self)), k, n_slabs, _vec(cand_score, acc, "cand_score"),
                     _vec(cand_id, torch.int32, "cand_id"), self._stream(S))

    def rank_merge(self, cand_score, cand_id, n_slabs: int, k: int, out_score, out_id):
        Q = out_id.numel() // max(int(k), 1)
        if out_score.numel() != out_id.numel() or cand_score.numel() < Q * n_slabs * k or cand_id.numel() < Q * n_slabs * k:
            raise ValueError("rank_merge: out_* must be [Q, k] and cand_* [Q, n_slabs, k]")
        self._invoke(self._fn("clane_rank_merge", cand_score.dtype), "clane_rank_merge",
                     _vec(cand_score, cand_score.dtype, "cand_score"), _vec(cand_id, torch.int32, "cand_id"), Q, n_slabs,
                     k, _vec(out_score, cand_score.dtype, "out_score"), _vec(out_id, torch.int32, "out_id"),
                     self._stream(cand_score))

    def pair_score(self, S, N, table_rows: int, d: int, src, dst, mode: int, sums2, sq, out):
        sp, lds, np_, ldn = self._two_tables(S, N, table_rows, d, "pair_score")
        acc = acc_dtype(S.dtype)
        B = self._pairs(src, dst, "pair_score")
        if out.numel() < B or (sq is not None and sq.numel() < table_rows):
            raise ValueError("pair_score: out needs one entry per pair, sq one per table row")
        self._invoke(self._fn("clane_pair_score", S.dtype), "clane_pair_score",
                     sp, lds, np_, ldn, table_rows, d, _vec(src, torch.int32, "src"), _vec(dst, torch.int32, "dst"), B,
                     mode, _ptr(sums2), None if sq is None else _vec(sq, acc, "sq"), _vec(out, acc, "out"),
                     self._stream(S))

    def rank_count(self, S, N, table_rows: int, d: int, q_rows, t_rows, mode: int, sums2, sq, label, excl_rowptr,
                   excl_colidx, exclude_self: bool, n_slabs: int, target_score, counts):
        sp, lds, np_, ldn = self._two_tables(S, N, table_rows, d, "rank_count")
        acc = acc_dtype(S.dtype)
        B = self._pairs(q_rows, t_rows, "rank_count")
        for t, n, name in ((sq, table_rows, "sq"), (label, table_rows, "label"), (excl_rowptr, table_rows + 1, "excl_rowptr")):
            if t is not None and t.numel() < n:
                raise ValueError(f"rank_count: {name} needs {n} entries")
        if target_score.numel() < B or counts.numel() < B * max(int(n_slabs), 0) * 4:
            raise ValueError("rank_count: target_score needs B entries and counts B * n_slabs * 4")
        self._invoke(self._fn("clane_rank_count", S.dtype), "clane_rank_count",
                     sp, lds, np_, ldn, table_rows, d, _vec(q_rows, torch.int32, "q_rows"),
                     _vec(t_rows, torch.int32, "t_rows"), B, mode, _ptr(sums2),
                     None if sq is None else _vec(sq, acc, "sq"),
                     None if label is None else _vec(label, torch.int32, "label"),
                     None if excl_rowptr is None else _vec(excl_rowptr, torch.int64, "excl_rowptr"),
                     None if excl_colidx is None else _vec(excl_colidx, torch.int32, "excl_colidx"),
                     int(bool(exclude_self)), n_slabs, _vec(target_score, acc, "target_score"),
                     _vec(counts, torch.int32, "counts"), self._stream(S))

    # -- node classification probe -------------------------------------------------------
    def probe_loss_ws_len(self, n: int, F: int) -> int:
        return int(self.lib.clane_probe_loss_ws_len(n, F))

    def probe_grad_ws_len(self, n: int, K: int, d: int) -> int:
        return int(self.lib.clane_probe_grad_ws_len(n, K, d))

    def probe_forward(self, Z, d: int, rows, y, split, W, bias, F: int, C: int, loss_ws, loss, G=None, pred=None):
        zp, ldz = _mat(Z, "Z")
        acc = acc_dtype(Z.dtype)
        n = rows.numel()
        K = F * probe_padded_classes(C)
        sp, lds = _mat(split, "split")
        if split.dtype != torch.uint8 or split.shape[0] < n or split.shape[1] < F or y.numel() != n:
            raise ValueError("probe_forward: split must be uint8 [n, >= F], y one class per row")
        if tuple(W.shape) != (K, d) or bias.numel() != K:
            raise ValueError(f"probe_forward: W must be [F * Cp, d] = [{K}, {d}] and bias [{K}], got {tuple(W.shape)}, "
                             f"{tuple(bias.shape)}")
        if loss.numel() < F or loss_ws.numel() < self.probe_loss_ws_len(n, F):
            raise ValueError("probe_forward: loss needs F doubles, loss_ws probe_loss_ws_len(n, F)")
        flags, gp, pp, ldp = 0, None, None, 0
        if G is not None:
            if G.numel() < n * K:
                raise ValueError("probe_forward: G needs n * K elements")
            flags, gp = flags | PROBE_WRITE_G, _vec(G, acc, "G")
        if pred is not None:
            pp, ldp = _mat(pred, "pred")
            if pred.dtype != torch.int32 or pred.shape[0] < n or pred.shape[1] < F:
                raise ValueError("probe_forward: pred must be int32 [n, >= F]")
            flags |= PROBE_WRITE_PRED
        self._invoke(self._fn("clane_probe_forward", Z.dtype), "clane_probe_forward",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), _vec(y, torch.int32, "y"), n, sp, lds,
                     _vec(W, acc, "W"), _vec(bias, acc, "bias"), F, C, flags, gp, _vec(loss_ws, torch.float64, "loss_ws"),
                     _vec(loss, torch.float64, "loss"), pp, ldp, self._stream(Z))

    def probe_forward_ovr(self, Z, d: int, rows, ymask, split, W, bias, col_state, F: int, C: int, max_labels: int,
                          loss_ws, loss, G=None, pred=None, top_k: bool = True):
        zp, ldz = _mat(Z, "Z")
        acc = acc_dtype(Z.dtype)
        n = rows.numel()
        K = F * ovr_padded_classes(C)
        sp, lds = _mat(split, "split")
        if split.dtype != torch.uint8 or split.shape[0] < n or split.shape[1] < F or ymask.numel() != n:
            raise ValueError("probe_forward_ovr: split must be uint8 [n, >= F], ymask one mask per row")
        if tuple(W.shape) != (K, d) or bias.numel() != K or col_state.numel() != K:
            raise ValueError(f"probe_forward_ovr: W must be [F * Cp, d] = [{K}, {d}], bias and col_state [{K}], got "
                             f"{tuple(W.shape)}, {tuple(bias.shape)}, {tuple(col_state.shape)}")
        if loss.numel() < F or loss_ws.numel() < self.probe_loss_ws_len(n, F):
            raise ValueError("probe_forward_ovr: loss needs F doubles, loss_ws probe_loss_ws_len(n, F)")
        flags, gp, pp, ldp = 0, None, None, 0
        if G is not None:
            if G.numel() < n * K:
                raise ValueError("probe_forward_ovr: G needs n * K elements")
            flags, gp = flags | PROBE_WRITE_G, _vec(G, acc, "G")
        if pred is not None:
            pp, ldp = _mat(pred, "pred")
            if pred.dtype != torch.int64 or pred.shape[0] < n or pred.shape[1] < F:
                raise ValueError("probe_forward_ovr: pred must be int64 [n, >= F]")
            flags |= PROBE_WRITE_PRED | (PROBE_PRED_TOPK if top_k else 0)
        self._invoke(self._fn("clane_probe_forward_ovr", Z.dtype), "clane_probe_forward_ovr",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), _vec(ymask, torch.int64, "ymask"), n, sp, lds,
                     _vec(W, acc, "W"), _vec(bias, acc, "bias"), _vec(col_state, torch.int8, "col_state"), F, C,
                     int(max_labels), flags, gp, _vec(loss_ws, torch.float64, "loss_ws"),
                     _vec(loss, torch.float64, "loss"), pp, ldp, self._stream(Z))

    def probe_grad(self, Z, d: int, rows, G, ws, dW, db):
        zp, ldz = _mat(Z, "Z")
        acc = acc_dtype(Z.dtype)
        n, K = rows.numel(), db.numel()
        if G.numel() < n * K or dW.numel() != K * d or ws.numel() < self.probe_grad_ws_len(n, K, d):
            raise ValueError("probe_grad: G needs n * K elements, dW K * d, db K, ws probe_grad_ws_len(n, K, d)")
        self._invoke(self._fn("clane_probe_grad", Z.dtype), "clane_probe_grad",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), n, _vec(G, acc, "G"), K,
                     _vec(ws, acc, "ws"), _vec(dW, acc, "dW"), _vec(db, acc, "db"), self._stream(Z))

    def probe_predict(self, Z, d: int, rows, W, bias, F: int, C: int, top_class, top_prob, proba=None,
                      sigmoid: bool = False, col_state=None):
        zp, ldz = _mat(Z, "Z")
        acc = acc_dtype(Z.dtype)
        n = rows.numel()
        K = F * (ovr_padded_classes(C) if sigmoid else probe_padded_classes(C))
        if Z.shape[1] < d or rows.dim() != 1:
            raise ValueError(f"probe_predict: Z must have at least d = {d} columns and rows be a vector")
        if tuple(W.shape) != (K, d) or bias.numel() != K:
            raise ValueError(f"probe_predict: W must be [F * Cp, d] = [{K}, {d}] and bias [{K}], got {tuple(W.shape)}, "
                             f"{tuple(bias.shape)}")
        if sigmoid and (col_state is None or col_state.numel() != K):
            raise ValueError(f"probe_predict: sigmoid needs col_state [{K}]")
        if top_class.dim() != 3 or tuple(top_class.shape[:2]) != (n, F) or top_class.dtype != torch.int32 \
                or not 1 <= top_class.shape[2] <= PREDICT_MAX_TOP or top_prob.shape != top_class.shape:
            raise ValueError(f"probe_predict: top_class (int32) and top_prob must be [n, F, 1..{PREDICT_MAX_TOP}]")
        flags = PREDICT_SIGMOID if sigmoid else 0
        pp = None
        if proba is not None:
            if tuple(proba.shape) != (n, F, C):
                raise ValueError(f"probe_predict: proba must be [n, F, C] = [{n}, {F}, {C}]")
            flags, pp = flags | PREDICT_WRITE_PROBA, _vec(proba, acc, "proba")
        if n == 0:
            return
        self._invoke(self._fn("clane_probe_predict", Z.dtype), "clane_probe_predict",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), n, _vec(W, acc, "W"),
                     _vec(bias, acc, "bias"), _vec(col_state, torch.int8, "col_state") if sigmoid else None, F, C,
                     int(top_class.shape[2]), flags, _vec(top_class, torch.int32, "top_class"),
                     _vec(top_prob, acc, "top_prob"), pp, self._stream(Z))

    # -- node clustering -------------------------------------------------------------------
    def kmeans_update_ws_len(self, n: int, R: int, K: int, d: int) -> int:
        return int(self.lib.clane_kmeans_update_ws_len(n, R, K, d))

    def kmeans_assign(self, Z, d: int, rows, centres, csq, assign, best):
        zp, ldz = _mat(Z, "Z")
        acc = acc_dtype(Z.dtype)
        n = rows.numel()
        if centres.dim() != 3 or centres.shape[2] != d or tuple(csq.shape) != tuple(centres.shape[:2]):
            raise ValueError(f"kmeans_assign: centres must be [R, K, d = {d}] and csq [R, K], got {tuple(centres.shape)}, "
                             f"{tuple(csq.shape)}")
        R, K = int(centres.shape[0]), int(centres.shape[1])
        ap, lda = _mat(assign, "assign")
        bp, ldb = _mat(best, "best")
        if assign.dtype != torch.int32 or best.dtype != acc or min(assign.shape[0], best.shape[0]) < n \
                or min(assign.shape[1], best.shape[1]) < R:
            raise ValueError(f"kmeans_assign: assign must be int32 [n, >= R] and best {acc} [n, >= R]")
        self._invoke(self._fn("clane_kmeans_assign", Z.dtype), "clane_kmeans_assign",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), n, _vec(centres, acc, "centres"),
                     _vec(csq, acc, "csq"), R, K, ap, lda, bp, ldb, self._stream(Z))

    def kmeans_update(self, Z, d: int, order, seg, centres_old, ws, centres_new, csq_new):
        zp, ldz = _mat(Z, "Z")
        acc = acc_dtype(Z.dtype)
        if centres_old.dim() != 3 or centres_old.shape[2] != d or centres_new.shape != centres_old.shape \
                or tuple(csq_new.shape) != tuple(centres_old.shape[:2]):
            raise ValueError(f"kmeans_update: centres_old / centres_new must be [R, K, d = {d}] and csq_new [R, K]")
        R, K = int(centres_old.shape[0]), int(centres_old.shape[1])
        if order.numel() % R or seg.numel() != R * K + 1:
            raise ValueError("kmeans_update: order needs R * n rows and seg R * K + 1 offsets")
        n = order.numel() // R
        if ws.numel() < self.kmeans_update_ws_len(n, R, K, d):
            raise ValueError("kmeans_update: ws needs kmeans_update_ws_len(n, R, K, d) elements")
        self._invoke(self._fn("clane_kmeans_update", Z.dtype), "clane_kmeans_update",
                     zp, Z.shape[0], d, ldz, _vec(order, torch.int32, "order"), _vec(seg, torch.int64, "seg"), n, R, K,
                     _vec(centres_old, acc, "centres_old"), _vec(ws, acc, "ws"), _vec(centres_new, acc, "centres_new"),
                     _vec(csq_new, acc, "csq_new"), self._stream(Z))

    # -- soft clusters ---------------------------------------------------------------------
    def mixture_ll_ws_len(self, n: int, R: int) -> int:
        return int(self.lib.clane_mixture_ll_ws_len(n, R))

    def mixture_mstep_ws_len(self, n: int, K: int, d: int) -> int:
        return int(self.lib.clane_mixture_mstep_ws_len(n, K, d))

    def mixture_estep(self, Z, d: int, rows, mean, Wm, cst, R: int, K: int, ll_ws, ll, resp=None, assign=None):
        zp, ldz = _mat(Z, "Z")
        acc = acc_dtype(Z.dtype)
        n = rows.numel()
        Kt = R * mixture_padded_components(K)
        if Z.shape[1] < d or rows.dim() != 1 or mean.numel() != d:
            raise ValueError(f"mixture_estep: Z must have at least d = {d} columns, rows be a vector and mean [{d}]")
        if tuple(Wm.shape) != (Kt, 2 * d) or cst.numel() != Kt:
            raise ValueError(f"mixture_estep: Wm must be [R * Kp, 2 d] = [{Kt}, {2 * d}] and cst [{Kt}], got "
                             f"{tuple(Wm.shape)}, {tuple(cst.shape)}")
        if ll.numel() < R or ll_ws.numel() < self.mixture_ll_ws_len(n, R):
            raise ValueError("mixture_estep: ll needs R doubles, ll_ws mixture_ll_ws_len(n, R)")
        flags, rp, ap, lda = 0, None, None, 0
        if resp is not None:
            if resp.numel() < n * Kt:
                raise ValueError("mixture_estep: resp needs n * R * Kp elements")
            flags, rp = flags | MIXTURE_WRITE_RESP, _vec(resp, acc, "resp")
        if assign is not None:
            ap, lda = _mat(assign, "assign")
            if assign.dtype != torch.int32 or assign.shape[0] < n or assign.shape[1] < R:
                raise ValueError("mixture_estep: assign must be int32 [n, >= R]")
            flags |= MIXTURE_WRITE_ASSIGN
        self._invoke(self._fn("clane_mixture_estep", Z.dtype), "clane_mixture_estep",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), n, _vec(mean, acc, "mean"),
                     _vec(Wm, acc, "Wm"), _vec(cst, acc, "cst"), R, K, flags, rp, _vec(ll_ws, torch.float64, "ll_ws"),
                     _vec(ll, torch.float64, "ll"), ap, lda, self._stream(Z))

    def mixture_mstep(self, Z, d: int, rows, mean, resp, ws, S, nk):
        zp, ldz = _mat(Z, "Z")
        acc = acc_dtype(Z.dtype)
        n, K = rows.numel(), nk.numel()
        if Z.shape[1] < d or rows.dim() != 1 or mean.numel() != d:
            raise ValueError(f"mixture_mstep: Z must have at least d = {d} columns, rows be a vector and mean [{d}]")
        if resp.numel() < n * K or S.numel() != K * 2 * d or ws.numel() < self.mixture_mstep_ws_len(n, K, d):
            raise ValueError("mixture_mstep: resp needs n * K elements, S K * 2 d, nk K, ws mixture_mstep_ws_len(n, K, d)")
        self._invoke(self._fn("clane_mixture_mstep", Z.dtype), "clane_mixture_mstep",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), n, _vec(mean, acc, "mean"),
                     _vec(resp, acc, "resp"), K, _vec(ws, acc, "ws"), _vec(S, acc, "S"), _vec(nk, acc, "nk"),
                     self._stream(Z))

    # -- content reduction -----------------------------------------------------------------
    def column_sums_ws_len(self, n: int, d: int) -> int:
        return int(self.lib.clane_column_sums_ws_len(n, d))

    def gram_ws_len(self, n: int, d: int) -> int:
        return int(self.lib.clane_gram_ws_len(n, d))

    def column_sums(self, Z, d: int, rows, ws, sums, accumulate: bool = False):
        zp, ldz = _mat(Z, "Z")
        n = rows.numel()
        if sums.numel() != d or ws.numel() < self.column_sums_ws_len(n, d):
            raise ValueError("column_sums: sums needs d doubles, ws column_sums_ws_len(n, d)")
        self._invoke(self._fn("clane_column_sums", Z.dtype), "clane_column_sums",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), n, PCA_ACCUMULATE if accumulate else 0,
                     _vec(ws, torch.float64, "ws"), _vec(sums, torch.float64, "sums"), self._stream(Z))

    def gram(self, Z, d: int, rows, mu, ws, G, accumulate: bool = False):
        zp, ldz = _mat(Z, "Z")
        acc = acc_dtype(Z.dtype)
        n = rows.numel()
        if tuple(G.shape) != (d, d) or ws.numel() < self.gram_ws_len(n, d) or (mu is not None and mu.numel() != d):
            raise ValueError(f"gram: G must be [{d}, {d}], mu [{d}] or None, ws gram_ws_len(n, d) elements")
        self._invoke(self._fn("clane_gram", Z.dtype), "clane_gram",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), n,
                     None if mu is None else _vec(mu, acc, "mu"), PCA_ACCUMULATE if accumulate else 0,
                     _vec(ws, acc, "ws"), _vec(G, acc, "G"), self._stream(Z))

    def project_affine(self, Z, d: int, rows, mu, W, Y):
        zp, ldz = _mat(Z, "Z")
        yp, ldy = _mat(Y, "Y")
        acc = acc_dtype(Z.dtype)
        n = rows.numel()
        if W.dim() != 2 or W.shape[1] != d or W.shape[0] < 1 or (mu is not None and mu.numel() != d):
            raise ValueError(f"project_affine: W must be [m, d = {d}] and mu [{d}] or None, got {tuple(W.shape)}")
        m = int(W.shape[0])
        if Y.dtype != Z.dtype or Y.shape[0] < n or Y.shape[1] < m:
            raise ValueError(f"project_affine: Y must be {Z.dtype} with at least {n} rows of {m} columns")
        self._invoke(self._fn("clane_project_affine", Z.dtype), "clane_project_affine",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), n,
                     None if mu is None else _vec(mu, acc, "mu"), _vec(W, acc, "W"), m, yp, ldy, self._stream(Z))

    # -- sparse content ---------------------------------------------------------------------
    def csr_spmm_segment(self) -> int:
        return int(self.lib.clane_csr_spmm_segment())

    def csr_spmm_ws_len(self, n_rows: int, nnz: int, l: int) -> int:
        return int(self.lib.clane_csr_spmm_ws_len(n_rows, nnz, l))

    @staticmethod
    def _csr_items(S, what: str):
        long_rows, seg_ptr, item_long = S.segments()
        if long_rows.dtype != torch.int32 or seg_ptr.dtype != torch.int64 or item_long.dtype != torch.int32 \
                or seg_ptr.numel() != long_rows.numel() + 1:
            raise ValueError(f"{what}: the segment list must be (int32 long_rows, int64 seg_ptr, int32 item_long)")
        return long_rows, seg_ptr, item_long

    def csr_spmm(self, S, B, l: int, out, a=None, s=None, ws=None):
        bp, ldb = _mat(B, "B")
        op, ldo = _mat(out, "out")
        n, D = S.shape
        f32 = torch.float32
        if B.dtype != f32 or out.dtype != f32 or B.shape[0] < D or B.shape[1] < l or out.shape[0] < n or out.shape[1] < l:
            raise ValueError(f"csr_spmm: B must be float32 with at least {D} rows and out with at least {n} rows of "
                             f"{l} columns")
        if l < 4 or l % 4 or l > CSR_MAX_L:
            raise ValueError(f"csr_spmm: l must be a multiple of 4 in [4, {CSR_MAX_L}], got {l}")
        if (a is not None and a.numel() != n) or (s is not None and s.numel() < l):
            raise ValueError(f"csr_spmm: a needs {n} entries and s {l}")
        long_rows, seg_ptr, item_long = self._csr_items(S, "csr_spmm")
        n_items = item_long.numel()
        if n_items and ws is None:
            ws = torch.empty(n_items * l, dtype=f32, device=out.device)
        if n_items and ws.numel() < n_items * l:
            raise ValueError(f"csr_spmm: ws needs {n_items * l} elements")
        self._invoke(self.lib.clane_csr_spmm_f32, "clane_csr_spmm",
                     _vec(S.rowptr, torch.int64, "rowptr"), _vec(S.col, torch.int32, "col"), _vec(S.val, f32, "val"),
                     n, S.nnz, bp, D, ldb, l, None if a is None else _vec(a, f32, "a"),
                     None if s is None else _vec(s, f32, "s"), _ptr(long_rows), _ptr(seg_ptr), _ptr(item_long),
                     long_rows.numel(), n_items, None if not n_items else _vec(ws, f32, "ws"),
                     0 if not n_items else ws.numel(), op, ldo, self._stream(out))

    def csr_row_sums(self, S, sums, ws=None):
        n = S.shape[0]
        if sums.numel() != n:
            raise ValueError(f"csr_row_sums: sums needs {n} doubles")
        long_rows, seg_ptr, item_long = self._csr_items(S, "csr_row_sums")
        n_items = item_long.numel()
        if n_items and ws is None:
            ws = torch.empty(n_items, dtype=torch.float64, device=sums.device)
        if n_items and ws.numel() < n_items:
            raise ValueError(f"csr_row_sums: ws needs {n_items} doubles")
        self._invoke(self.lib.clane_csr_row_sums_f32, "clane_csr_row_sums",
                     _vec(S.rowptr, torch.int64, "rowptr"), _vec(S.val, torch.float32, "val"), n, S.nnz,
                     _ptr(long_rows), _ptr(seg_ptr), _ptr(item_long), long_rows.numel(), n_items,
                     None if not n_items else _vec(ws, torch.float64, "ws"), 0 if not n_items else ws.numel(),
                     _vec(sums, torch.float64, "sums"), self._stream(sums))

    # -- 2-D layout ---------------------------------------------------------------------------
    @staticmethod
    def _tsne_square(M, what: str) -> int:
        if M.dim() != 2 or M.shape[0] != M.shape[1] or M.dtype != torch.float32 or not M.is_contiguous():
            raise ValueError(f"{what}: need a contiguous float32 [n, n] matrix, got {tuple(M.shape)} {M.dtype}")
        return int(M.shape[0])

    def tsne_sqdist(self, Z, d: int, rows, mu, sq, D):
        zp, ldz = _mat(Z, "Z")
        if Z.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"tsne_sqdist: float32 and bfloat16 tables, not {Z.dtype}")
        n = self._tsne_square(D, "tsne_sqdist")
        if rows.numel() != n or mu.numel() != d or sq.numel() != n:
            raise ValueError(f"tsne_sqdist: D must be [n, n] for the n = {rows.numel()} rows, mu [{d}], sq [n]")
        f32 = torch.float32
        self._invoke(self._fn("clane_tsne_sqdist", Z.dtype), "clane_tsne_sqdist",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), n, _vec(mu, f32, "mu"), _vec(sq, f32, "sq"),
                     D.data_ptr(), self._stream(D))

    def tsne_affinities(self, D, perplexity: float, beta):
        n = self._tsne_square(D, "tsne_affinities")
        if beta.numel() != n:
            raise ValueError(f"tsne_affinities: beta needs {n} entries")
        self._invoke(self.lib.clane_tsne_affinities_f32, "clane_tsne_affinities",
                     D.data_ptr(), n, float(perplexity), _vec(beta, torch.float32, "beta"), self._stream(D))

    def tsne_symmetrize_ws_len(self, n: int) -> int:
        return int(self.lib.clane_tsne_symmetrize_ws_len(n))

    def tsne_symmetrize(self, P, partials):
        n = self._tsne_square(P, "tsne_symmetrize")
        if partials.numel() != self.tsne_symmetrize_ws_len(n):
            raise ValueError("tsne_symmetrize: partials needs tsne_symmetrize_ws_len(n) doubles")
        self._invoke(self.lib.clane_tsne_symmetrize_f32, "clane_tsne_symmetrize",
                     P.data_ptr(), n, _vec(partials, torch.float64, "partials"), self._stream(P))

    @staticmethod
    def _tsne_points(n: int, what: str, **arrays):
        for name, t in arrays.items():
            cols = 6 if name == "F" else 2
            if tuple(t.shape) != (n, cols):
                raise ValueError(f"{what}: {name} must be [{n}, {cols}], got {tuple(t.shape)}")

    def tsne_forces(self, P, Y, F, kl: bool = True, cached: bool = False):
        n = self._tsne_square(P, "tsne_forces")
        self._tsne_points(n, "tsne_forces", Y=Y, F=F)
        f32 = torch.float32
        self._invoke(self.lib.clane_tsne_forces_f32, "clane_tsne_forces",
                     P.data_ptr(), _vec(Y, f32, "Y"), n, (TSNE_FORCES_KL if kl else 0) | (TSNE_FORCES_CACHED if cached else 0),
                     _vec(F, f32, "F"), self._stream(P))

    def tsne_step(self, F, Y, alpha: float, momentum: float, lr: float, plogp: float, V, G, Y_next, stats):
        n = int(Y.shape[0])
        self._tsne_points(n, "tsne_step", F=F, Y=Y, V=V, G=G, Y_next=Y_next)
        if stats.numel() != 4:
            raise ValueError("tsne_step: stats needs 4 doubles")
        f32 = torch.float32
        self._invoke(self.lib.clane_tsne_step_f32, "clane_tsne_step",
                     _vec(F, f32, "F"), _vec(Y, f32, "Y"), n, float(alpha), float(momentum), float(lr), float(plogp),
                     _vec(V, f32, "V"), _vec(G, f32, "G"), _vec(Y_next, f32, "Y_next"), _vec(stats, torch.float64, "stats"),
                     self._stream(Y))

    # -- neighbour-sparse 2-D layout ------------------------------------------------------------
    @staticmethod
    def _nn_lists(what: str, n: int, **arrays) -> int:
        k = None
        for name, t in arrays.items():
            want = torch.int32 if name.endswith("ids") else torch.float32
            if t.dim() != 2 or t.shape[0] != n or t.dtype != want or not t.is_contiguous() or (k is not None
                                                                                              and t.shape[1] != k):
                raise ValueError(f"{what}: {name} must be a contiguous {want} [{n}, k], got {tuple(t.shape)} {t.dtype}")
            k = int(t.shape[1])
        if not 1 <= k <= KNN_MAX_K:
            raise ValueError(f"{what}: k must be in [1, {KNN_MAX_K}], got {k}")
        return k

    def knn_sqdist(self, Z, d: int, rows, mu, sq, ids, sqdist, n_slabs: int = 1, cand_ids=None, cand_sqdist=None):
        zp, ldz = _mat(Z, "Z")
        if Z.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"knn_sqdist: float32 and bfloat16 tables, not {Z.dtype}")
        n, n_slabs = int(rows.numel()), int(n_slabs)
        if n > TSNE_NN_MAX_POINTS:
            raise ValueError(f"knn_sqdist: n = {n} exceeds {TSNE_NN_MAX_POINTS} rows")
        k = self._nn_lists("knn_sqdist", n, ids=ids, sqdist=sqdist)
        if mu.numel() != d or sq.numel() != n:
            raise ValueError(f"knn_sqdist: mu needs d = {d} entries and sq one per listed row ({n})")
        if n_slabs < 1:
            raise ValueError(f"knn_sqdist: n_slabs must be at least 1, got {n_slabs}")
        ci = cd = None
        if n_slabs > 1:
            if cand_ids is None or cand_sqdist is None or cand_ids.numel() != n * n_slabs * k \
                    or cand_sqdist.numel() != n * n_slabs * k:
                raise ValueError(f"knn_sqdist: n_slabs = {n_slabs} needs cand_ids and cand_sqdist of n * n_slabs * k = "
                                 f"{n * n_slabs * k} elements")
            ci, cd = _vec(cand_ids, torch.int32, "cand_ids"), _vec(cand_sqdist, torch.float32, "cand_sqdist")
        f32 = torch.float32
        self._invoke(self._fn("clane_knn_sqdist", Z.dtype), "clane_knn_sqdist",
                     zp, Z.shape[0], d, ldz, _vec(rows, torch.int32, "rows"), n, _vec(mu, f32, "mu"), _vec(sq, f32, "sq"),
                     k, n_slabs, cd, ci, sqdist.data_ptr(), ids.data_ptr(), self._stream(ids))

    def tsne_nn_affinities(self, sqdist, ids, perplexity: float, p, beta):
        n = int(sqdist.shape[0])
        self._nn_lists("tsne_nn_affinities", n, sqdist=sqdist, ids=ids, p=p)
        if beta.numel() != n:
            raise ValueError(f"tsne_nn_affinities: beta needs {n} entries")
        self._invoke(self.lib.clane_tsne_nn_affinities_f32, "clane_tsne_nn_affinities",
                     sqdist.data_ptr(), ids.data_ptr(), n, int(sqdist.shape[1]), float(perplexity), p.data_ptr(),
                     _vec(beta, torch.float32, "beta"), self._stream(p))

    @staticmethod
    def _nn_csr(what: str, rowptr, cols, val) -> tuple:
        n, nnz = int(rowptr.numel()) - 1, int(val.numel())
        if n < 1 or (cols is not None and cols.numel() != nnz):
            raise ValueError(f"{what}: rowptr needs n + 1 >= 2 entries, cols and val one per non-zero")
        return n, nnz

    def tsne_nn_plogp(self, rowptr, val, row_plogp):
        n, nnz = self._nn_csr("tsne_nn_plogp", rowptr, None, val)
        if row_plogp.numel() != n:
            raise ValueError(f"tsne_nn_plogp: row_plogp needs {n} doubles")
        self._invoke(self.lib.clane_tsne_nn_plogp_f32, "clane_tsne_nn_plogp",
                     _vec(rowptr, torch.int64, "rowptr"), _vec(val, torch.float32, "val") if nnz else None, n, nnz,
                     _vec(row_plogp, torch.float64, "row_plogp"), self._stream(row_plogp))

    def tsne_nn_attract(self, rowptr, cols, val, Y, F, kl: bool = True):
        n, nnz = self._nn_csr("tsne_nn_attract", rowptr, cols, val)
        self._tsne_points(n, "tsne_nn_attract", Y=Y, F=F)
        f32 = torch.float32
        self._invoke(self.lib.clane_tsne_nn_attract_f32, "clane_tsne_nn_attract",
                     _vec(rowptr, torch.int64, "rowptr"), _vec(cols, torch.int32, "cols") if nnz else None,
                     _vec(val, f32, "val") if nnz else None, _vec(Y, f32, "Y"), n, nnz, TSNE_FORCES_KL if kl else 0,
                     _vec(F, f32, "F"), self._stream(F))

    def tsne_repulse(self, Y, F):
        n = int(Y.shape[0])
        self._tsne_points(n, "tsne_repulse", Y=Y, F=F)
        self._invoke(self.lib.clane_tsne_repulse_f32, "clane_tsne_repulse",
                     _vec(Y, torch.float32, "Y"), n, _vec(F, torch.float32, "F"), self._stream(F))

    # -- silhouette -------------------------------------------------------------------------
    def _silhouette_args(self, what: str, Z, d: int, order, mu, metric: str, nrm):
        if metric not in SILHOUETTE_METRICS:
            raise ValueError(f"{what}: metric must be one of {sorted(SILHOUETTE_METRICS)}, got {metric!r}")
        acc = acc_dtype(Z.dtype)
        n = order.numel()
        if mu.numel() != d or nrm.numel() != n:
            raise ValueError(f"{what}: mu needs d = {d} entries and nrm one per position ({n})")
        zp, ldz = _mat(Z, "Z")
        return (zp, Z.shape[0], d, ldz, _vec(order, torch.int32, "order"), n), _vec(mu, acc, "mu"), _vec(nrm, acc, "nrm")

    def silhouette_norms(self, Z, d: int, order, mu, metric: str, nrm):
        head, mup, np_ = self._silhouette_args("silhouette_norms", Z, d, order, mu, metric, nrm)
        self._invoke(self._fn("clane_silhouette_norms", Z.dtype), "clane_silhouette_norms",
                     *head, mup, SILHOUETTE_METRICS[metric], np_, self._stream(Z))

    def silhouette_sums(self, Z, d: int, order, seg, mu, nrm, metric: str, p0: int, p1: int, S):
        head, mup, np_ = self._silhouette_args("silhouette_sums", Z, d, order, mu, metric, nrm)
        n, K = order.numel(), seg.numel() - 1
        p0, p1 = int(p0), int(p1)
        if K < 1 or not 0 <= p0 <= p1 <= n:
            raise ValueError(f"silhouette_sums: seg needs K + 1 >= 2 offsets and 0 <= p0 <= p1 <= n = {n}, got K = {K}, "
                             f"[{p0}, {p1})")
        if S.dtype != torch.float64 or S.dim() != 2 or S.shape[1] != K or S.shape[0] < p1 - p0 or not S.is_contiguous():
            raise ValueError(f"silhouette_sums: S must be contiguous float64 [>= {p1 - p0}, {K}], got {tuple(S.shape)} "
                             f"{S.dtype}")
        self._invoke(self._fn("clane_silhouette_sums", Z.dtype), "clane_silhouette_sums",
                     *head, _vec(seg, torch.int64, "seg"), K, mup, np_, SILHOUETTE_METRICS[metric], p0, p1, S.data_ptr(),
                     self._stream(Z))

    # -- CosineSimilarity on explicit pairs ------------------------------------------------
    def pair_cosine(self, A, B, d: int, out, ws):
        ap, lda = _mat(A, "A")
        bp, ldb = _mat(B, "B")
        self._check(self._fn("clane_pair_cosine", A.dtype)(
            ap, lda, bp, ldb, A.shape[0], d, _vec(out, acc_dtype(A.dtype), "out"), _vec(ws, torch.float64, "ws"),
            self._stream(A)), "clane_pair_cosine")

    # -- new vertices ---------------------------------------------------------------------
    def embed_rows(self, rowptr, colidx, X_new, Z, table_rows: int, d: int, mode: int, sums2, sq, S, gamma: float,
                   tolerence: int, max_rounds: int, Z_out, rounds, delta, P_out=None, flags: int = 0):
        xp, ldx = _mat(X_new, "X_new")
        zp, ldz = _mat(Z, "Z")
        op, ldo = _mat(Z_out, "Z_out")
        acc, m = acc_dtype(Z.dtype), X_new.shape[0]
        if X_new.dtype != Z.dtype or Z_out.dtype != Z.dtype:
            raise ValueError("embed_rows: X_new, Z and Z_out must share a dtype")
        if Z.shape[0] < table_rows or min(Z.shape[1], X_new.shape[1], Z_out.shape[1]) < d or Z_out.shape[0] < m:
            raise ValueError(f"embed_rows: Z needs {table_rows} rows, X_new / Z / Z_out {d} columns, Z_out {m} rows")
        if rowptr.numel() < m + 1 or rounds.numel() < m or delta.numel() < m:
            raise ValueError("embed_rows: rowptr needs m + 1 entries, rounds and delta one per new row")
        if sq is not None and sq.numel() < table_rows:
            raise ValueError("embed_rows: sq needs one entry per table row")
        sp, lds = (None, 0)
        if S is not None:
            sp, lds = _mat(S, "S")
            if S.dtype != acc or S.shape[0] < table_rows or S.shape[1] < d:
                raise ValueError(f"embed_rows: S must be {acc} with at least {table_rows} rows of {d} columns")
        self._invoke(self._fn("clane_embed_rows", Z.dtype), "clane_embed_rows",
                     _vec(rowptr, torch.int64, "rowptr"), _vec(colidx, torch.int32, "colidx"), m, xp, ldx, zp,
                     table_rows, ldz, d, mode, _ptr(sums2), None if sq is None else _vec(sq, acc, "sq"), sp, lds,
                     float(gamma), int(tolerence), int(max_rounds), int(flags), op, ldo,
                     _vec(rounds, torch.int32, "rounds"), _vec(delta, acc, "delta"),
                     None if P_out is None else _vec(P_out, acc, "P_out"), self._stream(Z))


_kernels: Optional[HipKernels] = None


def kernels() -> HipKernels:
    """Process-wide HipKernels; raises ClaneHipError when the library is not built."""
    global _kernels
    if _kernels is None:
        _kernels = HipKernels()
    return _kernels


def require_gpu(device=None) -> torch.device:
    """The device the hot path runs on.  Raises (never falls back) when there is none."""
    if not torch.cuda.is_available():
        raise ClaneHipError("clane_amd runs its embedding loop in HIP kernels on an MI355X; no GPU is visible "
                            "to this process and there is no CPU fallback.")
    if device is None or torch.device(device).type != "cuda":
        return torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
