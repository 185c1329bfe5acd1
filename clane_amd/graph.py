"""Graph -- the reference's ``clane/graph.py`` surface over CSR arrays and GPU-resident state.

Same constructor, attributes and methods as the reference (``Graph(data_root, embedding_dim)``,
``d, vertex_ids, X, V, E, dispense_pair, A, get_nbrs, build_P, Z, set_Z, len()``), same files
(``V``: ids one per line; ``E``: ``src\\tdst`` per line; optional ``C.npy`` / ``C.pt``), same
exceptions.  What differs is the representation: one O(|E|) parse into CSR instead of a Python
``Edge`` object per line and an O(|V|) ``list.index`` per endpoint (graph.py:79-89), and the
embeddings live in HBM inside a ``SweepEngine`` instead of one tensor per ``Vertex``.
"""
from __future__ import annotations

from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _hip
from .partition import HostCSR


# ---- file parsing (graph.py:43-47, 72-81) ---------------------------------------------------
def read_vertex_ids(data_root: Path) -> List[str]:
    with open(Path(data_root).joinpath("V"), "r") as io:          # FileNotFoundError propagates
        return io.read().strip().split("\n")


def read_edge_indices(data_root: Path, vertex_ids: Sequence[str]):
    """-> (src, dst) int64 arrays, one entry per line of ``E`` (duplicates kept).

    An id resolves to the index of its FIRST occurrence in ``V`` (``list.index``,
    graph.py:81); an unknown id or a line without exactly one tab raises ValueError.
    Parsed by the native loader (csrc/host_loader.cpp, O(|V| + |E|)) when libclane_host.so is
    built, else by the equivalent Python loop below.
    """
    data_root = Path(data_root)
    with open(data_root.joinpath("E"), "r"):                    # FileNotFoundError propagates, as upstream
        pass
    native = _native_parse_edges(data_root)
    if native is not None:
        return native
    return _python_parse_edges(data_root, vertex_ids)


def _python_parse_edges(data_root: Path, vertex_ids: Sequence[str]):
    with open(Path(data_root).joinpath("E"), "r") as io:
        lines = io.read().strip().split("\n")
    first = {}
    for i, vid in enumerate(vertex_ids):
        first.setdefault(vid, i)
    src = np.empty(len(lines), dtype=np.int64)
    dst = np.empty(len(lines), dtype=np.int64)
    for k, line in enumerate(lines):
        parts = line.split("\t")
        if len(parts) != 2:
            raise ValueError(f"E line {k + 1}: expected 'src\\tdst', got {line!r}")
        try:
            src[k], dst[k] = first[parts[0]], first[parts[1]]
        except KeyError as exc:
            raise ValueError(f"{exc.args[0]!r} is not in list") from None
    return src, dst


_HOST_LIB = None


def _host_lib():
    """ctypes handle of libclane_host.so (host-side parser), or None when it has not been built."""
    global _HOST_LIB
    if _HOST_LIB is None:
        import ctypes as C
        path = Path(__file__).resolve().parent / "libclane_host.so"
        if not path.exists():
            _HOST_LIB = False
        else:
            lib = C.CDLL(str(path))
            lib.clane_count_lines.restype = C.c_int64
            lib.clane_count_lines.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
            lib.clane_parse_edges.restype = C.c_int64
            lib.clane_parse_edges.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p,
                                              C.c_int]
            _HOST_LIB = lib
    return _HOST_LIB or None


def _native_parse_edges(data_root: Path):
    lib = _host_lib()
    if lib is None:
        return None
    import ctypes as C
    err = C.create_string_buffer(256)
    e_path, v_path = str(data_root / "E").encode(), str(data_root / "V").encode()
    n = lib.clane_count_lines(e_path, err, len(err))
    if n < 0:
        raise OSError(err.value.decode())
    src = np.empty(n, dtype=np.int64)
    dst = np.empty(n, dtype=np.int64)
    got = lib.clane_parse_edges(v_path, e_path, src.ctypes.data, dst.ctypes.data, n, err, len(err))
    if got == -4:           # not valid UTF-8: the Python loop opens the files in text mode and raises what upstream raises
        return None
    if got in (-2, -3):
        raise ValueError(err.value.decode(errors="replace"))
    if got < 0:
        raise OSError(err.value.decode())
    return src[:got], dst[:got]


def _cached_edge_indices(data_root: Path, vertex_ids: Sequence[str]):
    """read_edge_indices() through a small binary cache beside the text files."""
    stamp = np.array([[p.stat().st_size, p.stat().st_mtime_ns] for p in (data_root / "V", data_root / "E")],
                     dtype=np.int64)
    path = data_root / ".clane_edges.npz"
    if path.exists():
        try:
            with np.load(path) as z:
                if np.array_equal(z["stamp"], stamp):
                    return z["src"], z["dst"]
        except Exception:
            pass                                            # unreadable / stale cache: parse again
    src, dst = read_edge_indices(data_root, vertex_ids)
    try:
        np.savez(path, stamp=stamp, src=src, dst=dst)
    except OSError:
        pass                                                # read-only data_root: no cache, same result
    return src, dst


def csr_from_edges(num_vertices: int, src: np.ndarray, dst: np.ndarray, device="auto") -> HostCSR:
    """Coalesced adjacency (graph.py:104-110): sorted by (src, dst), duplicates merged, self-loops kept.
    One sort of the (src, dst) keys.  Large edge lists are sorted on a GPU (40M edges: 5.4 s with numpy, 2.4 s with
    torch on 8 host cores, 0.2 s on the card including both copies); a host utility either way.  ``device``: the card
    to borrow -- "auto" (the current one, when there is one: the embedding loop needs it anyway), a device, or None /
    "cpu" for the host.  A card without room for the keys and the sort's scratch (several times 8 bytes per edge)
    is not an error: the host sorts instead."""
    n = int(num_vertices)
    key = (torch.from_numpy(np.ascontiguousarray(src, dtype=np.int64)) * n
           + torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int64)))
    if device == "auto":
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    on_card = (device is not None and torch.device(device).type == "cuda" and key.numel() >= GPU_SORT_MIN_EDGES)
    if on_card:
        try:
            return _csr_from_keys(n, _sorted_unique(key.to(device), 0, n * n))
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
    return _csr_from_keys(n, _sorted_unique(key, 0, n * n))


def _csr_from_keys(n: int, key: torch.Tensor) -> HostCSR:
    rows = torch.div(key, n, rounding_mode="floor")
    counts = torch.bincount(rows, minlength=n).cpu().numpy()
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=rowptr[1:])
    return HostCSR(n, rowptr, (key - rows * n).to(torch.int32).cpu().numpy())


def _sorted_unique(key: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
    """torch.unique (sorted) of int64 keys in [lo, hi); lists beyond what one torch sort takes (2^31 - 1 elements)
    are split at the middle of the key range and the halves done one after the other."""
    if key.numel() <= SORT_MAX_ELEMENTS or hi - lo < 2:
        return torch.unique(key)
    mid = (lo + hi) // 2
    low = key < mid
    return torch.cat([_sorted_unique(key[low], lo, mid), _sorted_unique(key[~low], mid, hi)])


GPU_SORT_MIN_EDGES = 1 << 20
SORT_MAX_ELEMENTS = (1 << 31) - 1


def _parse_dtype(dtype) -> torch.dtype:
    if isinstance(dtype, torch.dtype):
        return dtype
    names = {"float32": torch.float32, "fp32": torch.float32, "f32": torch.float32,
             "float64": torch.float64, "fp64": torch.float64, "f64": torch.float64, "double": torch.float64,
             "bfloat16": torch.bfloat16, "bf16": torch.bfloat16}
    try:
        return names[str(dtype).lower().replace("torch.", "")]
    except KeyError:
        raise ValueError(f"unsupported embedding dtype {dtype!r} (float32, float64 or bfloat16)") from None


# ---- object-model facade ----------------------------------------------------------------------
class Vertex(object):
    """View of one vertex (reference graph.py:9-21).  ``x`` / ``z`` are rows of the graph's matrices."""
    __slots__ = ("_g", "idx", "id_")

    def __init__(self, graph: "Graph", idx: int, id_) -> None:
        self._g, self.idx, self.id_ = graph, idx, id_

    @property
    def x(self) -> torch.Tensor:
        return self._g.X[self.idx]

    @property
    def z(self) -> torch.Tensor:
        return self._g._host_Z()[self.idx]

    @z.setter
    def z(self, value: torch.Tensor) -> None:
        self._g._set_row(self.idx, value)

    @property
    def outgoing_indices(self) -> List[int]:
        return self._g._raw_neighbours(self.idx, out=True)

    @property
    def incoming_indices(self) -> List[int]:
        return self._g._raw_neighbours(self.idx, out=False)


class Edge(object):
    """reference graph.py:24-30."""
    __slots__ = ("src", "dst")

    def __init__(self, src: Vertex, dst: Vertex) -> None:
        self.src, self.dst = src, dst


class _LazySeq:
    """len()/index/iterate without materialising one Python object per element."""

    def __init__(self, n: int, make):
        self._n, self._make = n, make

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._make(j) for j in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        return self._make(i)

    def __iter__(self):
        return (self._make(i) for i in range(self._n))


class Graph(torch.utils.data.Dataset):
    # plug-in similarity callables (build_P): edge batches of a `batchwise` callable are gathered this many bytes
    # at a time; any other callable gets the reference's single call, refused above this size (None: 80 % of the
    # free HBM at the time of the call)
    PLUGIN_CHUNK_BYTES = 1 << 30
    PLUGIN_SINGLE_CALL_MAX_BYTES = None
    PLUGIN_EXCHANGE = "halo"        # division of an engine first created for a plug-in similarity (needs whole rows)

    def __init__(self, data_root: Path, embedding_dim: int = 128, dtype=None, cache: bool = False) -> None:
        """``dtype`` (extension, default None = keep what the files hold, as upstream): storage type of the
        embeddings on the GPU -- "float32", "float64" or "bfloat16" (bf16 storage, fp32 accumulate and P).
        ``cache`` (extension, default off): keep the parsed edge list in ``data_root/.clane_edges.npz`` and reuse
        it while ``V`` and ``E`` are unchanged (size + mtime), so a 40M-edge graph is parsed once."""
        super().__init__()
        data_root = Path(data_root)
        self.d = embedding_dim
        self.vertex_ids = read_vertex_ids(data_root)

        # Content embeddings C: C.npy -> C.pt -> N(0,1) (graph.py:50-58).  dtype is preserved.
        try:
            self.X = torch.from_numpy(np.load(data_root.joinpath("C.npy")))
        except FileNotFoundError:
            try:
                self.X = torch.load(data_root.joinpath("C.pt"))
            except FileNotFoundError:
                self.X = torch.normal(0, 1, [len(self.vertex_ids), self.d])
        if dtype is not None:
            self.X = self.X.to(_parse_dtype(dtype))
        if self.X.dim() != 2 or self.X.shape[0] != len(self.vertex_ids):
            raise ValueError(f"content embeddings have shape {tuple(self.X.shape)}, expected "
                             f"[{len(self.vertex_ids)}, d]")

        self._raw_src, self._raw_dst = (_cached_edge_indices(data_root, self.vertex_ids) if cache
                                        else read_edge_indices(data_root, self.vertex_ids))
        self.csr = csr_from_edges(len(self.vertex_ids), self._raw_src, self._raw_dst)

        self.V = _LazySeq(len(self.vertex_ids), lambda i: Vertex(self, i, self.vertex_ids[i]))
        self.E = _LazySeq(len(self._raw_src),
                          lambda k: Edge(self.V[int(self._raw_src[k])], self.V[int(self._raw_dst[k])]))
        self.dispense_pair = False

        self._Z_host: Optional[torch.Tensor] = None   # authoritative only while no engine exists / when dirty
        self._dirty = False
        self._engine = None
        self._raw_order = {}

    @classmethod
    def from_csr(cls, csr: HostCSR, X: torch.Tensor, vertex_ids=None) -> "Graph":
        """A Graph over an adjacency that already is a CSR in memory (synthetic inputs of bench.py and the
        tests; extension -- upstream only reads ``data_root``).  ``E`` then lists the CSR's edges."""
        if X.dim() != 2 or X.shape[0] != csr.num_vertices:
            raise ValueError(f"content embeddings have shape {tuple(X.shape)}, expected [{csr.num_vertices}, d]")
        g = cls.__new__(cls)
        torch.utils.data.Dataset.__init__(g)
        n = csr.num_vertices
        g.d, g.X, g.csr = int(X.shape[1]), X, csr
        g.vertex_ids = vertex_ids if vertex_ids is not None else _LazySeq(n, str)
        g._raw_src = np.repeat(np.arange(n, dtype=np.int64), csr.outdeg())
        g._raw_dst = csr.colidx.astype(np.int64)
        g.V = _LazySeq(n, lambda i: Vertex(g, i, g.vertex_ids[i]))
        g.E = _LazySeq(csr.num_edges, lambda k: Edge(g.V[int(g._raw_src[k])], g.V[int(g._raw_dst[k])]))
        g.dispense_pair = False
        g._Z_host, g._dirty, g._engine, g._raw_order = None, False, None, {}
        return g

    # ---- Dataset protocol ---------------------------------------------------------------
    def __len__(self):
        return len(self.vertex_ids)

    def __getitem__(self, idx):
        if self.dispense_pair:
            raise NotImplementedError("negative-pair sampling serves only the reference's trainable-similarity "
                                      "path (IterativeEmbedder), which is outside this package's scope")
        return idx

    # ---- adjacency (graph.py:104-116) -----------------------------------------------------
    def _edge_index(self) -> torch.Tensor:
        rows = np.repeat(np.arange(len(self), dtype=np.int64), self.csr.outdeg())
        return torch.from_numpy(np.stack([rows, self.csr.colidx.astype(np.int64)]))

    @property
    def A(self) -> torch.Tensor:
        idx = self._edge_index()
        return torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1]), size=(len(self), len(self)),
                                       is_coalesced=True)

    def get_nbrs(self, idx: int) -> torch.LongTensor:
        a, b = self.csr.rowptr[idx], self.csr.rowptr[idx + 1]
        return torch.from_numpy(self.csr.colidx[a:b].astype(np.int64))

    def _raw_neighbours(self, idx: int, out: bool) -> List[int]:
        key, val = (self._raw_src, self._raw_dst) if out else (self._raw_dst, self._raw_src)
        if out not in self._raw_order:
            order = np.argsort(key, kind="stable")
            ptr = np.zeros(len(self) + 1, dtype=np.int64)
            np.cumsum(np.bincount(key, minlength=len(self)), out=ptr[1:])
            self._raw_order[out] = (order, ptr)
        order, ptr = self._raw_order[out]
        return val[order[ptr[idx]:ptr[idx + 1]]].tolist()

    # ---- GPU engine ---------------------------------------------------------------------
    def engine(self, device=None, cosine_mode: str = "reference", **engine_kwargs):
        """The SweepEngine holding this graph's state in HBM (created on first use).

        Raises ``ClaneHipError`` when no GPU / HIP library is available: there is no CPU path.
        """
        from .engine import SweepEngine
        if self._engine is None:
            dev = _hip.require_gpu(device)
            pg = engine_kwargs.pop("process_group", None)
            if pg is None:
                import torch.distributed as dist
                if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                    pg = dist.group.WORLD
            with torch.cuda.device(dev):
                self._engine = SweepEngine(self.csr, self.X, dev, cosine_mode=cosine_mode, process_group=pg,
                                           **engine_kwargs)
        eng = self._engine
        if self._dirty:
            eng.set_Z(self._Z_host)
            self._dirty = False
        if eng.cosine_mode != cosine_mode:
            eng.cosine_mode, eng.P_valid = cosine_mode, False
        return eng

    def _attach_engine(self, engine) -> None:
        """Use an already-built engine (tests inject one with substitute kernels)."""
        self._engine = engine
        if self._dirty:
            engine.set_Z(self._Z_host)
            self._dirty = False

    # ---- embeddings (graph.py:130-138) ----------------------------------------------------
    def _host_Z(self) -> torch.Tensor:
        if self._engine is not None and not self._dirty:
            return self._engine.get_Z()
        if self._Z_host is None:
            self._Z_host = self.X.clone()      # Vertex.z starts as x (graph.py:19)
        return self._Z_host

    @property
    def Z(self) -> torch.Tensor:
        """Fresh [V, d] tensor; callers may mutate it freely (like the reference's torch.stack)."""
        z = self._host_Z()
        return z if (self._engine is not None and not self._dirty) else z.clone()

    def set_Z(self, Z: torch.Tensor) -> None:
        if tuple(Z.shape) != tuple(self.X.shape):
            raise ValueError(f"set_Z: expected {tuple(self.X.shape)}, got {tuple(Z.shape)}")
        self._Z_host = Z.detach().to("cpu", self.X.dtype).clone()
        self._dirty = True

    def _set_row(self, idx: int, value: torch.Tensor) -> None:
        z = self._host_Z().clone() if not self._dirty else self._Z_host
        z[idx] = value.detach().to("cpu", z.dtype)
        self._Z_host, self._dirty = z, True

    # ---- P (graph.py:118-128) -------------------------------------------------------------
    def build_P(self, similarity) -> torch.Tensor:
        """Row-softmax of per-edge similarity as a coalesced sparse [V, V] tensor (CPU).

        ``CosineSimilarity`` takes the fused HIP path (K0 + K1 + K2, nothing materialised).
        ``AsymmertricSimilarity`` takes the bilinear path (``SweepEngine.build_P_bilinear``: every row projected once
        with the module's current weights, then the pair K1 with its fused softmax; ``forward`` is not called).
        Any other callable follows the plugin protocol literally: it is called ONCE with the
        gathered ``Z[src]``, ``Z[dst]`` batches (GPU tensors) and its scores are normalised by
        the HIP segmented softmax.
        """
        from .similarity import AsymmertricSimilarity, CosineSimilarity
        if isinstance(similarity, CosineSimilarity):
            eng = self.engine(cosine_mode=similarity.mode)
            eng.build_P()
        elif isinstance(similarity, AsymmertricSimilarity):
            eng = self.engine(exchange=self.PLUGIN_EXCHANGE) if self._engine is None else self.engine()
            self._build_P_bilinear(eng, similarity)
        else:
            # Several GPUs: a plug-in needs WHOLE rows (all d columns of z_src and z_dst), so the rows are divided
            # (halo tables: every row a rank's edges read is in its table) and each rank scores the edges of its own
            # rows.  That is only the reference's single batched call (graph.py:120-121) when a pair's score does not
            # depend on the other pairs of the batch -- the callable says so with `batchwise = True`; a batch-global
            # measure would see 1/N of its batch on every rank and is refused.
            eng = self.engine(exchange=self.PLUGIN_EXCHANGE) if self._engine is None else self.engine()
            if eng.world > 1 and eng.columns:
                raise NotImplementedError(
                    f"custom similarity callables need whole rows of Z; this engine divides the COLUMNS over the GPUs "
                    f"(exchange={eng.exchange!r}). Build the graph's engine with a row division first: "
                    f"graph.engine(exchange='halo') (or 'allgather' / 'allgather_all'), CLI --exchange halo")
            if eng.world > 1 and not getattr(similarity, "batchwise", False):
                raise NotImplementedError(
                    "on several GPUs every rank scores the edges of its own rows, so a custom similarity callable must "
                    "score each pair independently of the rest of the batch and say so with `batchwise = True`; a "
                    "batch-global measure (like the reference's CosineSimilarity, similarity.py:37) is supported on a "
                    "single GPU only")
            rows = torch.repeat_interleave(torch.arange(eng.part.n_local, device=eng.device),
                                           eng.rowptr[1:] - eng.rowptr[:-1])
            Zd = eng.Zcur[:, :eng.d]
            # table row of every own row: a halo table starts with the own rows; a RowPartition places them
            own_pos = (torch.arange(eng.part.n_local, device=eng.device) if eng.halo
                       else torch.from_numpy(eng.part.local_positions()).to(eng.device))
            src_pos = own_pos[rows]
            dst_pos = eng.colidx[:eng.E_loc].long()
            pair_bytes = 2 * eng.E_loc * eng.d * Zd.element_size()          # the two gathered [E, d] batches
            if getattr(similarity, "batchwise", False):
                # the callable vouches that a pair's score does not depend on the other pairs of the batch:
                # gather and score PLUGIN_CHUNK_BYTES at a time (2 x 41 GB at config 3 never exists at once)
                step = max(1, self.PLUGIN_CHUNK_BYTES // max(1, 2 * eng.d * Zd.element_size()))
                for a in range(0, eng.E_loc, step):
                    b = min(a + step, eng.E_loc)
                    part = similarity(Zd[src_pos[a:b]], Zd[dst_pos[a:b]])
                    eng.P[a:b].copy_(part.detach().to(eng.acc_dtype).reshape(-1))
            else:
                limit = self.PLUGIN_SINGLE_CALL_MAX_BYTES
                if limit is None and eng.device.type == "cuda":
                    limit = int(0.8 * torch.cuda.mem_get_info(eng.device)[0])
                if limit is not None and pair_bytes > limit:
                    raise ValueError(
                        f"similarity plugin: the single batched call of the reference's protocol (graph.py:120-121) "
                        f"needs Z[src] and Z[dst] of all {eng.E_loc} edges at once = {pair_bytes / 2**30:.1f} GiB, more "
                        f"than the {limit / 2**30:.1f} GiB available. If a pair's score does not depend on the rest of "
                        f"the batch, set `batchwise = True` on the callable and it is scored in "
                        f"{self.PLUGIN_CHUNK_BYTES >> 20} MiB chunks; a batch-global measure (like the reference's "
                        f"CosineSimilarity) has to come as one call.")
                scores = similarity(Zd[src_pos], Zd[dst_pos]).detach().to(eng.acc_dtype).reshape(-1)
                eng.P[:eng.E_loc].copy_(scores)
            for i, b in enumerate(eng.blocks):        # rows above the engine's threshold: a workgroup per row
                lr = eng.long_rows[i]
                eng.k.segment_softmax(eng.rowptr[b.local_start:], b.nrows, eng.P, 0,
                                      eng.score_threshold if lr is not None else 0, lr)
            eng.P_valid = True
        values = self._gather_P(eng)
        return torch.sparse_coo_tensor(self._edge_index(), values, size=(len(self), len(self)), is_coalesced=True)

    def predict_links(self, similarity, k: int = 10, sources=None, exclude_existing: bool = True):
        """(ids [Q, k] int64, scores [Q, k]) as host tensors (extension; the reference stops at Z): for every source
        vertex index (None: all vertices, in order) the ``k`` vertices it is most likely to link to under ``similarity``
        and the CURRENT embeddings, best first, ties by vertex index; itself never, its existing out-neighbours unless
        ``exclude_existing`` is off; places beyond the eligible vertices hold -1 / -inf.  ``CosineSimilarity`` (its
        ``mode``) and ``AsymmertricSimilarity`` (its current weights) are scored on the GPU against all vertices at once
        (links.py); any other callable raises NotImplementedError.  One GPU only."""
        from .links import SUPPORTED, LinkRanker
        from .similarity import AsymmertricSimilarity, CosineSimilarity
        if isinstance(similarity, CosineSimilarity):
            eng = self.engine(cosine_mode=similarity.mode)
        elif isinstance(similarity, AsymmertricSimilarity):
            eng = self.engine()
        else:
            raise NotImplementedError(
                f"predict_links scores with {SUPPORTED}; a plug-in similarity ({type(similarity).__name__}) has no "
                f"kernel to score all pairs with")
        ids, scores = LinkRanker(eng, similarity).top_k(k, sources, exclude_existing)
        return ids.cpu(), scores.cpu()

    def evaluate_links(self, similarity, src, dst, hits=(1, 3, 10), filter_existing: bool = True) -> dict:
        """How well ``similarity`` and the CURRENT embeddings predict the held-out pairs (src[i], dst[i]) of vertex indices
        (extension): the exact rank of dst[i] among all vertices src[i] does not link to yet (``filter_existing``; itself
        and dst[i] never count), and from the ranks ``{"pairs", "skipped", "mrr", "mean_rank", "hits": {K: ..}, "auc"}``
        (links.LinkMetrics.as_dict) on the host.  Similarities and engines as ``predict_links``: any other callable,
        several GPUs and a column division raise NotImplementedError."""
        from .links import SUPPORTED, LinkRanker
        from .similarity import AsymmertricSimilarity, CosineSimilarity
        if isinstance(similarity, CosineSimilarity):
            eng = self.engine(cosine_mode=similarity.mode)
        elif isinstance(similarity, AsymmertricSimilarity):
            eng = self.engine()
        else:
            raise NotImplementedError(
                f"evaluate_links scores with {SUPPORTED}; a plug-in similarity ({type(similarity).__name__}) has no "
                f"kernel to score all pairs with")
        return LinkRanker(eng, similarity).evaluate(src, dst, hits, filter_existing).as_dict()

    def embed_new(self, similarity, X_new, neighbours, gamma: float = 0.76, tolerence: int = 10, max_rounds: int = 64,
                  weights: bool = False):
        """Embeddings of vertices that are NOT in the graph, against the CURRENT embeddings, which do not move
        (extension, induct.py): vertex i has content ``X_new[i]`` and out-edges to the existing vertices
        ``neighbours[i]`` -- a sequence of per-vertex collections of vertex indices, or a tuple ``(rowptr, colidx)`` of
        two arrays.  The reference's loop restricted to such a row is the fixed point ``z <- x + gamma * sum_v
        softmax_v(score(z, z_v)) z_v`` on frozen ``Z``, iterated per row with the reference's ``Tolerence`` and at most
        ``max_rounds`` rounds.  Returns ``induct.NewRows`` on the host (``Z`` in ``X``'s dtype, ``rounds``, ``delta``,
        ``converged``, the coalesced ``rowptr`` / ``cols`` and with ``weights`` the soft-max weights ``P``).  A repeated
        neighbour counts once; an index outside ``[0, V)`` is a ValueError, so new vertices cannot link to each other.
        Similarities and engines as ``predict_links``."""
        from .induct import SUPPORTED, NewVertexEmbedder, normalize_neighbours
        from .similarity import AsymmertricSimilarity, CosineSimilarity
        X_new = torch.as_tensor(X_new)
        if X_new.dim() != 2 or X_new.shape[1] != self.X.shape[1]:
            raise ValueError(f"embed_new: X_new must be [m, {self.X.shape[1]}], got {tuple(X_new.shape)}")
        rowptr, cols = normalize_neighbours(neighbours, int(X_new.shape[0]))
        if isinstance(similarity, CosineSimilarity):
            eng = self.engine(cosine_mode=similarity.mode)
        elif isinstance(similarity, AsymmertricSimilarity):
            eng = self.engine()
        else:
            raise NotImplementedError(
                f"embed_new scores with {SUPPORTED}; a plug-in similarity ({type(similarity).__name__}) has no kernel "
                f"to iterate a row with")
        res = NewVertexEmbedder(eng, similarity).embed(X_new.to(self.X.dtype), rowptr, cols, gamma, tolerence, max_rounds,
                                                       weights).cpu()
        res.Z = res.Z.to(self.X.dtype).contiguous()
        return res

    def _resolve_labels(self, labels, multilabel: bool, what: str):
        """(vertex indices, classes or class-set masks, sorted class names) from the three forms ``evaluate_labels``
        takes."""
        from .classify import index_classes, read_labels
        if isinstance(labels, (str, Path)):
            return read_labels(Path(labels), self.vertex_ids, multilabel=bool(multilabel))
        if isinstance(labels, tuple) and len(labels) == 2:
            vertices, raw = list(labels[0]), list(labels[1])
        else:
            raw = list(labels)
            vertices = list(range(len(self)))
        if len(raw) != len(vertices):
            raise ValueError(f"{what}: one class per labelled vertex")
        item = lambda c: c.item() if isinstance(c, torch.Tensor) else c     # noqa: E731
        if multilabel:
            if any(isinstance(s, (str, bytes)) or not hasattr(s, "__iter__") for s in raw):
                raise ValueError(f"{what}: multilabel needs a collection of classes per labelled vertex")
            sets = [[item(c) for c in s] for s in raw]
            names = sorted({c for s in sets for c in s})
            if len(names) > 64:
                raise ValueError(f"{what}: {len(names)} classes; the multi-label probe handles at most 64")
            index = {c: i for i, c in enumerate(names)}
            y = [sum(1 << index[c] for c in set(s)) for s in sets]
        else:
            y, names = index_classes([item(c) for c in raw])
        return vertices, y, names

    def evaluate_labels(self, labels, ratios=(0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9), runs: int = 10, seed: int = 0,
                        l2: float = 1.0, table: str = "Z", multilabel: bool = False, predict: str = "top_k") -> dict:
        """The reference README's node-classification table for the CURRENT embeddings (extension): a soft-max regression
        on the labelled vertices' rows per (train share, random split), all fits at once on the GPU (classify.py), micro
        and macro F1 on each fit's test rows, averaged over the runs of a share.  ``labels``: a file of ``id<TAB>class``
        lines (any subset of the vertices), a pair ``(vertex indices, classes)``, or one class per vertex; class names
        are indexed in sorted order.  ``table="X"`` probes the content embeddings instead (the README's bag-of-words
        row).  Returns ``{"table", "labelled", "classes", "class_names", "rows": [{"ratio", "micro_f1", "macro_f1",
        "runs_used"}], "fits": {...per fit: ratio, run, iterations, converged, objective, skipped, micro_f1, macro_f1},
        ...}``.  Several GPUs and a column division raise NotImplementedError.

        ``multilabel=True`` (DeepWalk's protocol for BlogCatalog-like data): a vertex has a SET of classes -- in the file
        a repeated id adds a class, in the Python forms every entry is a collection of classes -- at most 64 in all; the
        fits are one-vs-rest logistic regressions, and a test vertex with k true classes is given the k classes of
        highest score (``predict="top_k"``) or those of positive score (``"threshold"``).  The result also has
        ``"multilabel"``, ``"predict"`` and ``"constant_columns"`` (class columns of a fit that no or every training
        vertex has: not fitted, predicted never / always)."""
        from .classify import LabelProbe
        if predict not in ("top_k", "threshold"):
            raise ValueError(f"evaluate_labels: predict must be 'top_k' or 'threshold', got {predict!r}")
        vertices, y, names = self._resolve_labels(labels, multilabel, "evaluate_labels")
        kw = dict(multilabel=True, predict=predict) if multilabel else {}
        out = LabelProbe(self.engine(), l2=l2).evaluate(vertices, y, len(names), ratios=tuple(ratios), runs=runs,
                                                        seed=seed, table=table, **kw)
        out["class_names"] = [str(c) for c in names]
        return out

    def fit_labels(self, labels, l2=1.0, folds: int = 5, seed: int = 0, table: str = "Z", multilabel: bool = False):
        """A kept classifier on the CURRENT embeddings (extension, classify.py): a soft-max regression (``multilabel``:
        one-vs-rest regressions) on ALL labelled vertices, returned as a ``classify.LabelModel`` with ``save`` / ``load``.
        ``labels`` as ``evaluate_labels`` takes them.  ``l2``: a number, or a list -- then the value of lowest mean
        held-out log-loss over ``folds`` folds (one permutation seeded ``seed``) is chosen, every fold and value fitted
        at once, and the model's ``cv`` holds the table.  Several GPUs and a column division raise
        NotImplementedError."""
        from .classify import LabelProbe
        vertices, y, names = self._resolve_labels(labels, multilabel, "fit_labels")
        l2 = list(l2) if isinstance(l2, (list, tuple)) else float(l2)
        return LabelProbe(self.engine()).train(vertices, y, len(names), l2=l2, folds=folds, seed=seed, table=table,
                                               multilabel=bool(multilabel), class_names=[str(c) for c in names])

    def predict_labels(self, model, vertices=None, top: int = 3, table: Optional[str] = None, proba: bool = False):
        """(vertex indices, classes [m, top], probs [m, top][, proba [m, C]]) on the host: the ``top`` most probable
        classes of the vertices (default: all) under ``model`` (``fit_labels`` / ``LabelModel.load``), best first, as
        indices into ``model.class_names``; -1 / 0 where the model has fewer classes to give.  Probabilities are a
        soft-max over the classes, or per-class sigmoids that do not sum to 1 for a multi-label model.  ``table``: the
        model's own by default.  A model of another width is a ValueError; several GPUs raise NotImplementedError."""
        from .classify import LabelProbe
        d = int(self.X.shape[1])
        if int(model.d) != d:
            raise ValueError(f"predict_labels: the model was fitted for d = {model.d}, this graph has d = {d}")
        eng = self.engine()
        LabelProbe(eng)                                     # the probe's refusals: one GPU, no column division
        v = np.arange(len(self), dtype=np.int64) if vertices is None else np.asarray(list(vertices), dtype=np.int64)
        return (v,) + tuple(model.predict_table(eng, v, table=model.table if table is None else table, top=top,
                                                proba=proba))

    def cluster(self, k=None, labels=None, vertices=None, restarts: int = 10, seed: int = 0, max_iter: int = 300,
                table: str = "Z", return_assignments: bool = False, silhouette: bool = False,
                silhouette_metric: str = "euclidean", silhouette_points: Optional[int] = 65536) -> dict:
        """Node clustering of the CURRENT embeddings (extension): k-means, every restart at once on the GPU
        (cluster.py), the restart of lowest inertia reported.  With ``labels`` -- the three forms ``evaluate_labels``
        takes -- the labelled vertices are clustered, ``k`` defaults to the number of classes and the result carries
        ``nmi``, ``ari``, ``purity``, ``per_restart`` and ``class_names``; without, ``vertices`` (default: all) are
        clustered into ``k`` clusters.  ``table="X"`` clusters the content embeddings instead.  Returns ``{"table",
        "clustered", "clusters", "restarts", "seed", "inertia", "iterations", "converged", "empty", "best_restart",
        "sizes", ...}``; with ``return_assignments`` also ``"vertices"`` and ``"assignments"`` (the best restart's
        cluster per clustered vertex).  Several GPUs and a column division raise NotImplementedError.

        ``silhouette=True`` scores the best restart (still chosen by inertia) without labels: ``silhouette`` (the mean
        of the exact per-row silhouette under ``silhouette_metric``, csrc/silhouette.h; over at most ``silhouette_points``
        vertices, sampled as ``layout`` samples, ``None``: all), ``silhouette_per_cluster``, ``calinski_harabasz`` and
        ``davies_bouldin``; centres without rows are left out of all three.  ``k`` may be a sequence of counts: every one
        is fitted with the same seeds and scored on the same sample, the result is that of the count with the highest mean
        silhouette (ties to the smaller) and carries ``selection = {criterion, candidates: [{clusters, inertia,
        silhouette, calinski_harabasz, davies_bouldin, empty}], chosen}``."""
        from .classify import index_classes, read_labels
        if k is None and labels is None:
            raise ValueError("cluster: give k, the number of clusters, or labels whose classes it defaults to")
        ks, listed = [k], False
        if isinstance(k, (list, tuple, range)) or (isinstance(k, torch.Tensor) and k.dim() > 0):
            from .cluster import check_cluster_counts
            ks, listed = check_cluster_counts(k)
        silhouette = bool(silhouette) or listed
        if silhouette:
            from .cluster import SILHOUETTE_METRICS
            if silhouette_metric not in SILHOUETTE_METRICS:
                raise ValueError(f"cluster: silhouette_metric must be one of {SILHOUETTE_METRICS}, got {silhouette_metric!r}")
            if silhouette_points is not None and (isinstance(silhouette_points, bool)
                                                  or int(silhouette_points) != silhouette_points or silhouette_points < 2):
                raise ValueError(f"cluster: silhouette_points must be an integer >= 2 or None, got {silhouette_points!r}")
        y = names = None
        if labels is not None:
            if isinstance(labels, (str, Path)):
                vertices, y, names = read_labels(Path(labels), self.vertex_ids)
            else:
                if isinstance(labels, tuple) and len(labels) == 2:
                    vertices, raw = list(labels[0]), list(labels[1])
                else:
                    raw = list(labels)
                    vertices = list(range(len(self)))
                if len(raw) != len(vertices):
                    raise ValueError("cluster: one class per labelled vertex")
                raw = [c.item() if isinstance(c, torch.Tensor) else c for c in raw]
                y, names = index_classes(raw)
        elif vertices is None:
            vertices = list(range(len(self)))
        from .cluster import KMeans
        km = KMeans(self.engine(), max_iter=max_iter)
        sil = pick = None
        if silhouette:
            from .cluster import Silhouette, score_fit, select_clusters
            from .layout import sample_vertices
            sil = Silhouette(self.engine(), metric=silhouette_metric)
            if silhouette_points is not None:                   # one sample for every candidate
                pick, sampled = sample_vertices(len(vertices), int(silhouette_points), seed)
                pick = pick if sampled else None

        def run(k_one):
            out = km.evaluate(vertices, k=k_one, y=y, n_classes=None if names is None else len(names), restarts=restarts,
                              seed=seed, table=table)
            if names is not None:
                out["class_names"] = [str(c) for c in names]
            if sil is not None:
                tab, rows = km.table_and_rows(vertices, table)
                out.update(score_fit(km, sil, tab, rows, km.last_fit, pick))
                out["silhouette_metric"] = silhouette_metric
                out["silhouette_scored"] = len(vertices) if pick is None else int(pick.numel())
            if return_assignments:
                out["vertices"] = [int(v) for v in vertices]
                out["assignments"] = km.last_fit.assign[:, out["best_restart"]].tolist()
            return out
        return select_clusters(ks, run) if listed else run(ks[0])

    def soft_cluster(self, k=None, labels=None, vertices=None, restarts: int = 10, seed: int = 0, max_iter: int = 100,
                     tol: float = 1e-3, reg_covar: float = 1e-6, criterion: str = "bic", table: str = "Z",
                     return_memberships: bool = False) -> dict:
        """Soft clusters of the CURRENT embeddings (extension, mixture.py): a diagonal-covariance Gaussian mixture fitted
        by EM as scikit-learn's ``GaussianMixture(covariance_type="diag")`` defines it, every restart at once on the GPU
        from the partitions of ``cluster``'s k-means, the restart of highest lower bound reported.  ``labels``,
        ``vertices`` and ``table`` as ``cluster`` takes them; ``k`` (1..64) defaults to the number of classes.  Returns
        ``{"table", "clustered", "clusters", "restarts", "seed", "log_likelihood" (mean per row), "lower_bound", "bic",
        "aic", "iterations", "converged", "best_restart", "weights", "soft_sizes", "sizes", "empty", "clamped",
        "mean_entropy" (the mean of -sum r log r / log K, 0 for K = 1), "confident" (the share of rows whose top
        responsibility is >= 0.9)}``, with labels also ``nmi``, ``ari``, ``purity`` of the hard assignment and
        ``class_names``; with ``return_memberships`` also ``"vertices"``, ``"assignments"``, ``"memberships"`` (float64
        numpy [n, K]) and ``"model"`` (a ``mixture.MixtureModel`` with ``save`` / ``load`` / ``predict``).  ``k`` may be a
        sequence of counts: every one is fitted with the same seeds, the result is that of the lowest ``criterion``
        ("bic" / "aic", ties to the smaller count) and carries ``selection = {criterion, candidates, chosen}``.  Reads
        the engine's table where it lies and changes no state.  Several GPUs and a column division raise
        NotImplementedError."""
        from .cluster import clustering_scores, contingency
        from .mixture import CRITERIA, GaussianMixture, check_component_counts, describe_fit, select_components
        if k is None and labels is None:
            raise ValueError("soft_cluster: give k, the number of components, or labels whose classes it defaults to")
        if criterion not in CRITERIA:
            raise ValueError(f"soft_cluster: criterion must be one of {CRITERIA}, got {criterion!r}")
        y = names = None
        if labels is not None:
            vertices, y, names = self._resolve_labels(labels, False, "soft_cluster")
        elif vertices is None:
            vertices = list(range(len(self)))
        ks, listed = check_component_counts(len(names) if k is None else k)
        gm = GaussianMixture(self.engine(), reg_covar=reg_covar, tol=tol, max_iter=max_iter)
        tab, rows = gm.table_and_rows(vertices, table)

        def run(k_one):
            fit = gm.fit(tab, rows, k_one, restarts=restarts, seed=seed)
            out = describe_fit(fit, table, restarts, seed)
            if names is not None:
                yt = torch.as_tensor(y, dtype=torch.int64).reshape(-1).to(tab.device)
                nmi, ari, purity = clustering_scores(contingency(yt, fit.assign, len(names), k_one))
                out.update({"nmi": float(nmi), "ari": float(ari), "purity": float(purity),
                            "class_names": [str(c) for c in names]})
            if return_memberships:
                out["vertices"] = [int(v) for v in vertices]
                out["assignments"] = fit.assign.tolist()
                out["memberships"] = fit.resp.double().cpu().numpy()
                out["model"] = fit.model(table=table)
            return out
        return select_components([run(int(v)) for v in ks], criterion) if listed else run(ks[0])

    def silhouette(self, partition=None, labels=None, vertices=None, table: str = "Z", metric: str = "euclidean",
                   max_points: Optional[int] = 65536, seed: int = 0) -> dict:
        """The exact silhouette of a partition of the CURRENT embeddings (extension; ``table="X"``: of the content):
        ``partition`` -- one integer per vertex of ``vertices`` (default: all), a k-means assignment say -- or ``labels``
        -- the three forms ``cluster`` takes; it scores how well the true classes separate in the embedding.  More than
        ``max_points`` rows: the first ``max_points`` of a torch permutation seeded with ``seed``, sorted, as ``layout``
        samples; ``None`` means all.  Returns ``{"mean", "per_cluster", "sizes", "n", "sampled", "metric", "table",
        "clusters"}`` (``clusters``: the distinct partition values or class names, in the order of ``per_cluster`` and
        ``sizes``).  The n x K sums of distances are formed on the GPU (csrc/silhouette.h), never the n x n distances.
        Reads the engine's table where it lies and changes no state.  One GPU only."""
        from .classify import index_classes, read_labels
        from .cluster import Silhouette, dense_partition
        from .layout import sample_vertices
        if (partition is None) == (labels is None):
            raise ValueError("silhouette: give partition, one integer per vertex, or labels -- one of the two")
        if max_points is not None and (isinstance(max_points, bool) or int(max_points) != max_points or max_points < 2):
            raise ValueError(f"silhouette: max_points must be an integer >= 2 or None, got {max_points!r}")
        if labels is not None:
            if isinstance(labels, (str, Path)):
                vertices, y, names = read_labels(Path(labels), self.vertex_ids)
            else:
                if isinstance(labels, tuple) and len(labels) == 2:
                    vertices, raw = list(labels[0]), list(labels[1])
                else:
                    raw = list(labels)
                    vertices = list(range(len(self)))
                if len(raw) != len(vertices):
                    raise ValueError("silhouette: one class per labelled vertex")
                y, names = index_classes([c.item() if isinstance(c, torch.Tensor) else c for c in raw])
            own = torch.as_tensor(y, dtype=torch.int64).reshape(-1)
            names = [str(c) for c in names]
        else:
            if vertices is None:
                vertices = list(range(len(self)))
            ids, own = dense_partition(torch.as_tensor(partition).reshape(-1).cpu())
            if own.numel() != len(vertices):
                raise ValueError(f"silhouette: one cluster per vertex, got {own.numel()} for {len(vertices)} vertices")
            names = ids.tolist()
        sil = Silhouette(self.engine(), metric=metric)
        pool = torch.as_tensor(vertices, dtype=torch.int64).reshape(-1)
        pick, sampled = sample_vertices(int(pool.numel()), int(pool.numel() if max_points is None else max_points), seed)
        tab, rows = sil.table_and_rows(pool[pick], table)
        res = sil.samples(tab, rows, own[pick], k=len(names))
        return {"mean": res.mean, "per_cluster": [None if v != v else v for v in res.per_cluster.tolist()],
                "sizes": res.sizes.tolist(), "n": int(pick.numel()), "sampled": bool(sampled), "metric": metric,
                "table": table, "clusters": names}

    def reduce_content(self, dim: int, center: bool = True, whiten: bool = False, block_rows=None, transform=None):
        """Replace the content embeddings ``X`` (and ``d``) by their ``dim`` principal components (extension, reduce.py:
        column sums, centred Gram and projection on the GPU, the ``d x d`` eigen-problem on the host) and keep the
        fitted ``ContentPCA`` as ``self.content_transform`` -- new vertices' content has to go through the same one.
        ``transform``: apply this fitted / loaded ``ContentPCA`` instead of fitting.  Before the first use of the
        engine only: its tables have the width it was built with.  Returns the ``ContentPCA``."""
        from .reduce import ContentPCA
        if self._engine is not None:
            raise RuntimeError("reduce_content: this graph's engine exists already and its tables have the content's "
                               "width; reduce the content before the first build_P / iterate / engine()")
        if self._Z_host is not None:
            raise RuntimeError("reduce_content: embeddings were set (set_Z / Vertex.z) at the content's width; reduce "
                               "the content first")
        pca = transform if transform is not None else ContentPCA(dim, center=center, whiten=whiten, block_rows=block_rows)
        X = self.X if self.X.is_contiguous() else self.X.contiguous()
        Y = pca.transform(X) if transform is not None else pca.fit_transform(X)
        self.X, self.d, self.content_transform = Y.contiguous(), int(Y.shape[1]), pca
        return pca

    def reduce_sparse_content(self, S, dim: int, center: bool = True, whiten: bool = False, oversample: int = 16,
                              power_iterations: int = 4, seed: int = 0, transform=None):
        """As ``reduce_content`` for content that is a ``sparse.SparseRows`` [len(self), D] (a bag of words as CSR): the
        randomized fit ``ContentPCA.fit_sparse`` and one CSR product replace ``X`` (whatever it held: without a dense
        content file it is the constructor's N(0, 1) placeholder) and ``d``; the matrix is never made dense.
        ``transform``: apply this fitted / loaded ``ContentPCA`` instead of fitting.  Returns the ``ContentPCA``."""
        from .reduce import ContentPCA
        from .sparse import SparseRows
        if self._engine is not None:
            raise RuntimeError("reduce_sparse_content: this graph's engine exists already and its tables have the "
                               "content's width; reduce the content before the first build_P / iterate / engine()")
        if self._Z_host is not None:
            raise RuntimeError("reduce_sparse_content: embeddings were set (set_Z / Vertex.z) at the content's width; "
                               "reduce the content first")
        if not isinstance(S, SparseRows):
            raise ValueError(f"reduce_sparse_content: expected a SparseRows, got {type(S).__name__}")
        if S.shape[0] != len(self):
            raise ValueError(f"reduce_sparse_content: the content has {S.shape[0]} rows, the graph {len(self)} vertices")
        if transform is not None:
            pca = transform
        else:
            pca = ContentPCA(dim, center=center, whiten=whiten)
            pca._check_fit_shape(*S.shape)                       # before the upload
        from . import _hip
        Sd = S if S.device.type == "cuda" else S.to(_hip.require_gpu(None))
        if transform is None:
            pca.fit_sparse(Sd, oversample=oversample, power_iterations=power_iterations, seed=seed)
            pca.sparse_fit_ = {"nnz": S.nnz, "oversample": int(oversample), "power_iterations": int(power_iterations),
                               "seed": int(seed)}
        Y = pca.transform_sparse(Sd, dtype=self.X.dtype).to(self.X.device)
        self.X, self.d, self.content_transform = Y.contiguous(), int(Y.shape[1]), pca
        return pca

    def project(self, dim: int = 2, table: str = "Z", vertices=None, whiten: bool = False):
        """``(Y [len(vertices), dim] on the host in vertex order, the fitted ContentPCA)``: the principal components of
        the CURRENT embeddings (``table="X"``: of the content) of ``vertices`` (default: all) -- the picture of an
        embedding (extension).  Reads the engine's table where it lies and changes no state.  One GPU only."""
        from .reduce import ContentPCA
        eng = self.engine()
        pca = ContentPCA(dim, whiten=whiten).fit_table(eng, table, vertices)
        return pca.transform_table(eng, table, vertices).cpu(), pca

    def layout(self, table: str = "Z", vertices=None, max_points: int = 20000, seed: int = 0, labels=None,
               method: str = "exact", neighbours=None, **tsne_kwargs):
        """``(Y [n, 2] on the host, the laid-out vertex indices, info)``: the exact t-SNE layout (extension, layout.py:
        distances, perplexity search and every iteration on the GPU) of the CURRENT embeddings (``table="X"``: of the
        content) of ``vertices`` (default: all).  More than ``max_points`` of them: the first ``max_points`` of a torch
        permutation seeded with ``seed``, sorted; ``Y`` is in the order of the returned indices.  ``labels`` -- a file of
        ``id<TAB>class`` lines, one class per vertex of the graph, or ``(vertices, classes)`` -- adds ``"classes"`` (per
        laid-out vertex, None where unlabelled) and ``"neighbour_agreement"`` (k = 5, over the labelled ones) to
        ``info``, next to ``n, sampled, table, perplexity, iterations, kl, kl_init, grad_norm, kl_trace``.
        ``tsne_kwargs`` go to ``layout.TSNE``.  Reads the engine's table where it lies and changes no state.  One GPU only.

        ``method="neighbours"`` lays out up to 2^20 points (``layout.NeighbourTSNE``: P on every point's ``neighbours``
        nearest neighbours -- None: ``3 * perplexity`` -- and the repulsion exact); ``info`` then also carries ``method``,
        ``neighbours`` and ``nnz``.  ``"exact"`` keeps all of ``P [n, n]`` and stops at 65 536 points."""
        from .classify import read_labels
        from .layout import METHODS, MIN_POINTS, TSNE, NeighbourTSNE, neighbour_agreement, sample_vertices
        if method not in METHODS:
            raise ValueError(f"layout: method must be one of {list(METHODS)}, got {method!r}")
        if neighbours is not None and method != "neighbours":
            raise ValueError(f"layout: neighbours = {neighbours!r} needs method=\"neighbours\" (method {method!r} keeps "
                             f"all of P)")
        if isinstance(max_points, bool) or int(max_points) != max_points or int(max_points) < MIN_POINTS:
            raise ValueError(f"layout: max_points must be an integer >= {MIN_POINTS}, got {max_points!r}")
        cls_of = None
        if labels is not None:
            if isinstance(labels, (str, Path)):
                lv, ly, names = read_labels(Path(labels), self.vertex_ids)
                lc = [names[c] for c in ly]
            elif isinstance(labels, tuple) and len(labels) == 2:
                lv, lc = list(labels[0]), list(labels[1])
            else:
                lc = list(labels)
                lv = list(range(len(self)))
            if len(lv) != len(lc):
                raise ValueError("layout: one class per labelled vertex")
            cls_of = {int(v): (c.item() if isinstance(c, torch.Tensor) else c) for v, c in zip(lv, lc)}
        pool = torch.arange(len(self)) if vertices is None else torch.as_tensor(vertices, dtype=torch.int64).reshape(-1)
        pick, sampled = sample_vertices(int(pool.numel()), int(max_points), seed)
        chosen = pool[pick]
        if method == "neighbours":
            tsne = NeighbourTSNE(self.engine(), neighbours=neighbours, **tsne_kwargs)
        else:
            tsne = TSNE(self.engine(), **tsne_kwargs)
        tsne.check_points(int(chosen.numel()))                  # before the table is touched
        tab, rows = tsne.table_and_rows(chosen, table)
        fit = tsne.fit(tab, rows, seed=seed)
        Y = fit.Y.cpu()
        info = {"n": int(chosen.numel()), "sampled": bool(sampled), "table": table, "perplexity": tsne.perplexity,
                "iterations": fit.iterations, "kl": fit.kl, "kl_init": fit.kl_init, "grad_norm": fit.grad_norm,
                "kl_trace": list(fit.kl_trace)}
        if method == "neighbours":
            info.update(method=method, neighbours=fit.neighbours, nnz=fit.nnz)
        if cls_of is not None:
            classes = [cls_of.get(int(v)) for v in chosen.tolist()]
            known = [i for i, c in enumerate(classes) if c is not None]
            index = {c: i for i, c in enumerate(sorted({classes[i] for i in known}, key=str))}
            info["classes"] = classes
            info["neighbour_agreement"] = (neighbour_agreement(Y[known], [index[classes[i]] for i in known], k=5)
                                           if len(known) > 5 else None)
        return Y, chosen, info

    def neighbours(self, k: int, vertices=None, table: str = "Z"):
        """``(indices [m, k] int64, distances [m, k] float32)`` on the host: for every vertex of ``vertices`` (default:
        all) its ``k`` nearest OTHER vertices of ``vertices`` in the CURRENT embeddings (``table="X"``: in the content),
        as vertex indices, nearest first, ties to the earlier place in ``vertices``; squared Euclidean distances of the
        rows centred by their column mean -- the distances of ``layout`` (extension, layout.KNeighbours: distances and
        selection in one kernel, never the m x m matrix).  With ``k >= m`` the places past the ``m - 1`` others hold
        ``-1`` and ``inf``.  Euclidean only.  Reads the engine's table where it lies and changes no state.  One GPU only."""
        from .classify import table_and_rows
        from .layout import KNeighbours
        pool = torch.arange(len(self)) if vertices is None else torch.as_tensor(vertices, dtype=torch.int64).reshape(-1)
        KNeighbours.check(int(pool.numel()), k)                  # before the table is touched
        knn = KNeighbours(self.engine())
        tab, rows = table_and_rows(knn.eng, pool, table)
        ids, sqdist = knn.search(tab, rows, k)
        ids = ids.cpu().to(torch.int64)
        return torch.where(ids >= 0, pool[ids.clamp(min=0)], ids), sqdist.cpu()

    def _build_P_bilinear(self, eng, similarity) -> None:
        """P of an AsymmertricSimilarity on the engine, from the module's weights as they are NOW (copied to the device on
        every call: a caller that changes Phi between rounds gets the new P)."""
        n_dim = similarity.Phi_src.in_features
        if n_dim != eng.d_full or similarity.Phi_dst.in_features != eng.d_full:
            raise ValueError(f"AsymmertricSimilarity(n_dim={n_dim}) does not fit embeddings of dimension {eng.d_full}")
        eng.build_P_bilinear(similarity.stacked_weight(eng.acc_dtype, eng.device))

    def _gather_P(self, eng) -> torch.Tensor:
        """P values of every rank, put back into the global (row, col)-sorted edge order."""
        out = torch.empty(self.csr.num_edges, dtype=eng.acc_dtype)
        local = (torch.from_numpy(eng.local.edge_origin), eng.P[:eng.E_loc].to("cpu"))
        # rows divided: the ranks that hold the same columns have the rows of P between them
        pieces = [local] if eng.row_world == 1 else eng.comm.all_gather_object(local)
        for origin, vals in pieces:
            out[origin] = vals
        return out
