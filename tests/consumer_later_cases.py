"""The consumers that merged after tests/consumer_exact_cases.py, held to the same two relations -- helpers of
tests/test_gpu_consumer_exact.py (the HIP kernels) and tests/test_consumer_exact_host.py (the fixtures' teeth, on the CPU).

``Silhouette.samples`` (cluster.py), ``ContentPCA.fit_table`` / ``transform_table`` (reduce.py), ``KNeighbours.search``,
``TSNE.fit``, ``NeighbourTSNE.fit`` (layout.py), ``LabelProbe.predict`` / ``LabelModel.predict_table`` (classify.py) and
``GaussianMixture.fit`` / ``MixtureModel.predict`` (mixture.py) all reach the engine's table through
``classify.table_and_rows``.  Their kernels are pinned to the bit elsewhere (dense bits, distance bits); the layer that
decides WHICH table, WHICH rows and WHICH leading dimension a kernel is handed had only met one-block engines.  Every
one of them lists its rows in vertex order through ``rows`` and promises bits that do not depend on where a row stands
in the table, so the strong check needs no tolerance.

A.8 ``check_layout_independence``: on ``LaterCase`` (the random normal ``FloatCase`` plus a vertex list that is neither
in vertex order nor in table-row order, a partition, initial responsibilities, an initial layout and fixed weights) every
output under every plan of ``LATER_RUNS`` must be torch.equal to the LAYOUT-FREE result: the same kind of consumer object
run on ``Z_plain`` -- the host ``Z0`` in the case's dtype as a plain contiguous ``[V, d]`` device tensor -- with the
vertex list itself as rows.  Nothing of ``pos``, of padding rows or of the engine's leading dimension enters it.  Three
consumers take an ENGINE, not a table: their layout-free result comes from the public calls that take a plain matrix --
``ContentPCA.fit(Z_plain[list])`` / ``transform(Z_plain)``, ``LabelModel.predict_rows`` and ``MixtureModel.predict_rows``
on ``Z_plain[list]`` (rows 0 .. n - 1 of a gathered copy).  Under ``chunks3_overlap`` the silhouette, the k-NN, the PCA
and the mixture run again on ``table="X"`` against the layout-free result on the host ``X``.

Left out per dtype: ``KNeighbours``, ``TSNE`` and ``NeighbourTSNE`` have float32 and bfloat16 instances only
(_hip.knn_sqdist / tsne_sqdist refuse float64), so the float64 case runs the silhouette, the PCA, the predictions and the
mixture.  ``ContentPCA(whiten=True)`` runs in the bfloat16 cases, ``whiten=False`` in the others.

What the plans of ``LATER_RUNS`` really change for a consumer (asserted in tests/test_consumer_exact_host.py): every
plan but ``chunks3_vertex_order`` permutes the rows (``defaults``, the tile plans and ``contiguous_tables`` through
``hot_rows_first``), the three-block plans hold 702 table rows for 700 vertices.  Column tiles do NOT widen the leading
dimension -- a tile is a column range of ONE table, and at d = 128, 64 and 300 ``ld == d`` -- so ``PADDED_CASES`` add
``tiles2`` at (fp32, 130) and (bf16, 70), where the table's rows are 132 and 72 elements long and ``Z_plain``'s 130 and
70: there a consumer that passed ``d`` for the leading dimension reads other rows.

B ``Later``: what ``consumer_exact_cases.run_current_table`` compares with a fresh engine after each of its six
steps, on the HIP kernels: the k-NN (not in the float64 "sequence" runs), the euclidean silhouette, fit_table +
transform_table, ``LabelProbe.predict`` with fixed weights, a three-iteration mixture fit and the two kept models'
predictions -- once for consumer objects and models made before any sweep, once for objects made at that step.  t-SNE
stays out of B for the time it takes.

``check_wrong_inputs`` proves that the comparisons bite: under ``chunks3_overlap`` every consumer is fed the vertex list
NOT mapped through ``pos``, then the table before the last sweep, and every data output must differ from the layout-free
result.  On one GPU ``X_loc``'s local-row order IS the table-row order (``local.vertex`` inverts ``pos``: asserted on
the host), so ``pos``-mapped rows into ``X_loc`` are the right rows, not a mistake; the check records that they compare
equal and feeds ``table="X"`` the unmapped list and the Z table instead.

Every comparison is torch.equal or ==."""
import contextlib
import functools

import torch

from clane_amd import classify as classify_mod
from clane_amd import mixture as mixture_mod
from clane_amd.classify import LabelModel, LabelProbe
from clane_amd.cluster import Silhouette
from clane_amd.layout import KNeighbours, NeighbourTSNE, TSNE
from clane_amd.mixture import GaussianMixture
from clane_amd.reduce import ContentPCA

from . import consumer_exact_cases as CX
from . import engine_exact_cases as X
from .exact_cases import BF16, F32, F64

LATER_PLANS = ("defaults", "chunks3_overlap", "chunks3_vertex_order", "chunks3_class", "contiguous_tables", "tiles2")
THREE_BLOCK_PLANS = ("chunks3_overlap", "chunks3_vertex_order", "chunks3_class")
IN_VERTEX_ORDER = ("chunks3_vertex_order",)                  # the one plan whose pos is the identity
PADDED_CASES = [(F32, 130), (BF16, 70)]                      # ld = 132 and 72: wider than d
LATER_RUNS = ([(c, p) for c in X.ONE_PER_DTYPE for p in LATER_PLANS] + [((F32, 300), "tiles3")]
              + [(c, "tiles2") for c in PADDED_CASES])
WRONG_RUN = ((F32, 128), "chunks3_overlap")

N_LISTED = 333                                               # odd; 3 candidate tiles of 128, more than k = 192
# the vertices on both sides of the two block edges (table rows 233 | 234 and 467 | 468) under the three-block plans:
# chunks3_vertex_order, chunks3_overlap (seed 11), chunks3_class and the sequence plans (seeds 12 and 11) --
# test_consumer_exact_host recomputes them from the engines
EDGE_VERTICES = (233, 234, 467, 468, 236, 189, 276, 256, 169, 241, 91, 356)
PERPLEXITY, TSNE_ITERS, NEIGHBOURS = 10.0, 20, 30
PCA_DIM, TOP, CLUSTERS, MODELS = 5, 3, 6, 2
X_CONSUMERS = ("knn7", "knn192", "silhouette-euclidean", "silhouette-cosine", "pca", "mixture")
B_CONSUMERS = ("knn7", "silhouette-euclidean", "pca", "predict-softmax", "mixture", "label-model", "mixture-model")
# outputs that may coincide although the rows read are others: integer summaries and the (empty: 20 < 50 iterations) trace
MAY_COINCIDE = ("sizes", "classes", "assign", "kl_trace")


@functools.lru_cache(maxsize=None)
def vertex_list(V=700):
    """int64 [N_LISTED]: a seeded subset of the vertices in a seeded order, with vertex 0, vertex V - 1 and the
    neighbours of every block edge in it."""
    gen = torch.Generator().manual_seed(8800)
    forced = torch.tensor(sorted({0, V - 1, *EDGE_VERTICES}))
    rest = torch.ones(V, dtype=torch.bool)
    rest[forced] = False
    rest = rest.nonzero().flatten()
    chosen = torch.cat([forced, rest[torch.randperm(rest.numel(), generator=gen)[:N_LISTED - forced.numel()]]])
    chosen = chosen[torch.randperm(N_LISTED, generator=gen)]
    assert chosen.unique().numel() == N_LISTED and not bool((chosen[1:] > chosen[:-1]).all())
    return chosen


class LaterCase:
    """``FloatCase`` (dtype, d, seed) and what the later consumers need on top of it; host tensors nobody writes to."""

    def __init__(self, dtype, d, seed=0):
        self.base = c = CX.float_case(dtype, d, seed)
        self.dtype, self.d, self.acc = dtype, d, c.acc
        self.vertices = L = vertex_list(c.Z0.shape[0])
        n = L.numel()
        gen = torch.Generator().manual_seed(9900 + d + seed)
        self.part = torch.randint(0, CLUSTERS, (n,), generator=gen)
        assert int(torch.bincount(self.part, minlength=CLUSTERS).min()) >= 2
        self.resp0 = torch.softmax(2.0 * torch.randn(3, n, c.K, generator=gen, dtype=F64), dim=2)    # restarts = 3, k = 7
        self.Y0 = (1e-2 * torch.randn(n, 2, generator=gen, dtype=F64)).float()
        self.Wp = torch.randn(MODELS, c.C, d, generator=gen, dtype=F64) / d ** 0.5
        self.bp = torch.randn(MODELS, c.C, generator=gen, dtype=F64)
        self.col_state = torch.tensor([[0, 0, -1, 0, 1], [0, 0, 0, 0, 0]], dtype=torch.int8)
        self.y = c.y[L]
        self.whiten = dtype == BF16
        self.has_distances = dtype != F64                   # knn_sqdist / tsne_sqdist: float32 and bfloat16 only


@functools.lru_cache(maxsize=None)
def later_case(dtype, d, seed=0):
    return LaterCase(dtype, d, seed)


# ---- the consumers ---------------------------------------------------------------------------------------------------------
def make_objects(eng, em_iters=5):
    """One consumer object of every kind on ``eng``."""
    return {"knn": KNeighbours(eng), "silhouette-euclidean": Silhouette(eng, "euclidean"),
            "silhouette-cosine": Silhouette(eng, "cosine"),
            "tsne": TSNE(eng, perplexity=PERPLEXITY, max_iter=TSNE_ITERS),
            "ntsne": NeighbourTSNE(eng, perplexity=PERPLEXITY, max_iter=TSNE_ITERS, neighbours=NEIGHBOURS),
            "probe": LabelProbe(eng, max_iter=20), "mixture": GaussianMixture(eng, max_iter=em_iters, tol=0.0)}


def _scalar(v):
    return torch.tensor(float(v), dtype=F64)


def table_results(objs, Z, rows, L, only):
    """name -> tensor of every consumer of ``only`` that takes (table, rows)."""
    out = {}
    for k, slabs in ((7, None), (192, 3)):
        if f"knn{k}" in only:
            out[f"knn{k} ids"], out[f"knn{k} sqdist"] = objs["knn"].search(Z, rows, k, n_slabs=slabs)
    for name in ("silhouette-euclidean", "silhouette-cosine"):
        if name in only:
            res = objs[name].samples(Z, rows, L.part)
            out.update({f"{name} samples": res.samples, f"{name} per_cluster": res.per_cluster, f"{name} sizes": res.sizes,
                        f"{name} mean": _scalar(res.mean)})
    for name in ("tsne", "ntsne"):
        if name in only:
            fit = objs[name].fit(Z, rows, init=L.Y0)
            out.update({f"{name} Y": fit.Y, f"{name} kl": _scalar(fit.kl), f"{name} kl_trace": torch.tensor(fit.kl_trace, dtype=F64)})
    for name, multilabel in (("predict-softmax", False), ("predict-sigmoid", True)):
        if name in only:
            p = objs["probe"].predict(Z, rows, L.Wp, L.bp, L.base.C, top=TOP, proba=True, multilabel=multilabel,
                                      col_state=L.col_state if multilabel else None)
            out.update({f"{name} classes": p.classes, f"{name} probs": p.probs, f"{name} proba": p.proba})
    if "mixture" in only:
        fit = objs["mixture"].fit(Z, rows, L.base.K, init=L.resp0)
        out.update({"mixture resp": fit.resp, "mixture assign": fit.assign, "mixture weights": fit.weights,
                    "mixture means": fit.means, "mixture variances": fit.variances, "mixture lower_bound": fit.lower_bound})
        out["_mixture_fit"] = fit
    return out


def _pca_outputs(pca, Y):
    return {"pca mean": torch.from_numpy(pca.mean_), "pca components": torch.from_numpy(pca.components_),
            "pca variance": torch.from_numpy(pca.explained_variance_), "pca Y": Y}


def _model_outputs(name, res):
    return {f"{name} classes": torch.from_numpy(res[0]), f"{name} probs": torch.from_numpy(res[1]),
            f"{name} proba": torch.from_numpy(res[2])}


def engine_results(eng, L, models, only, table="Z"):
    """name -> tensor of the consumers of ``only`` that take an ENGINE: the PCA fitted on the list and applied to every
    vertex, the kept models applied to the list."""
    out = {}
    if "pca" in only:
        pca = ContentPCA(PCA_DIM, whiten=L.whiten).fit_table(eng, table, L.vertices)
        out.update(_pca_outputs(pca, pca.transform_table(eng, table)))
    if "label-model" in only:
        out.update(_model_outputs("label-model", models["label"].predict_table(eng, L.vertices, top=TOP, proba=True)))
    if "mixture-model" in only:
        out.update(_model_outputs("mixture-model", models["mixture"].predict(eng, L.vertices, top=TOP, proba=True)))
    return out


def plain_engine_results(eng, Zp, L, models, only):
    """The layout-free counterpart of ``engine_results``: the public calls that take a plain matrix."""
    out = {}
    listed = Zp[L.vertices.to(Zp.device)].contiguous()
    if "pca" in only:
        pca = ContentPCA(PCA_DIM, whiten=L.whiten).fit(listed)
        out.update(_pca_outputs(pca, pca.transform(Zp)))
    if "label-model" in only:
        out.update(_model_outputs("label-model", models["label"].predict_rows(eng, listed, top=TOP, proba=True)))
    if "mixture-model" in only:
        out.update(_model_outputs("mixture-model", models["mixture"].predict_rows(eng, listed, top=TOP, proba=True)))
    return out


def consumers_of(L, table="Z"):
    """The consumers a case runs on a table: all of them on Z (without the distance kernels' in float64), X_CONSUMERS on
    X."""
    names = (["knn7", "knn192", "tsne", "ntsne"] if L.has_distances else []) + \
        ["silhouette-euclidean", "silhouette-cosine", "predict-softmax", "predict-sigmoid", "mixture", "pca", "label-model",
         "mixture-model"]
    return tuple(n for n in names if table == "Z" or n in X_CONSUMERS)


def _finish(out):
    out.pop("_mixture_fit", None)
    return {name: t.detach().cpu().clone() for name, t in out.items()}


def label_model_from(fit, L, table="Z"):
    """What ``LabelProbe.train`` keeps of a one-column fit."""
    return LabelModel(W=fit.W[0].cpu().numpy(), b=fit.b[0].cpu().numpy(), class_names=[str(c) for c in range(L.base.C)],
                      multilabel=False, l2=1.0, col_state=None, d=L.d, table=table, n_train=int(L.vertices.numel()),
                      objective=float(fit.objective[0]), iterations=int(fit.iterations[0]), converged=bool(fit.converged[0]))


def layout_free(eng, objs, host_table, L, only, models=None, table="Z"):
    """(name -> CPU tensor, models) from a table no engine made: ``host_table`` [V, d] in the case's dtype as a plain
    contiguous device tensor, the vertex list itself as rows.  ``models`` None: the kept models are fitted here, on the
    plain table -- a 20-iteration probe fit on the list and the mixture fit's best restart."""
    Zp = host_table.to(L.dtype).to(eng.device).contiguous()
    rows = L.vertices.to(eng.device, torch.int32)
    assert tuple(Zp.shape) == (eng.V, L.d) and Zp.stride() == (L.d, 1)
    out = table_results(objs, Zp, rows, L, only)
    if models is None and table == "Z":
        ones = torch.ones(rows.numel(), 1, dtype=torch.uint8)
        models = {"label": label_model_from(objs["probe"].fit(Zp, rows, L.y, ones, L.base.C, l2=[1.0]), L),
                  "mixture": out["_mixture_fit"].model()}
    out.update(plain_engine_results(eng, Zp, L, models, only))
    return _finish(out), models


def through_the_engine(eng, objs, L, only, models, table="Z"):
    """name -> CPU tensor of the same consumers on ``table_and_rows(eng, list, table)`` and on the engine itself."""
    T, rows = classify_mod.table_and_rows(eng, L.vertices, table)
    out = table_results(objs, T, rows, L, only)
    out.update(engine_results(eng, L, models, only, table))
    return _finish(out)


def record_all(checks, tag, got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for name, t in got.items():
        same = t.dtype == want[name].dtype and torch.equal(t, want[name])
        checks.record(f"{tag} {name}", same, "rows that differ",
                      CX._rows_that_differ(t, want[name])[:6].tolist() if t.numel() and t.dim() and t.shape == want[name].shape else None)


# ---- A.8 -------------------------------------------------------------------------------------------------------------------
_plain = {}


def _cached_layout_free(eng, objs, L, key, table):
    if (key, table) not in _plain:
        c = L.base
        models = None if table == "Z" else _plain[(key, "Z")][1]
        _plain[(key, table)] = layout_free(eng, objs, c.Z0 if table == "Z" else c.X, L, consumers_of(L, table), models, table)
    return _plain[(key, table)]


def run_layout_independence(kernels, dev, case, plan_name):
    """The `Checks` of A.8 for one (case, plan)."""
    L = later_case(*case)
    settings, route = X.PLANS[plan_name]
    checks = X.Checks(f"A8 {X.plan_id((case, plan_name))}")
    with X.device_ctx(dev):
        eng = X.make_engine(kernels, dev, L.base, **settings)
        route(eng, dev)
        objs = make_objects(eng)
        key = (str(dev), case)
        want, models = _cached_layout_free(eng, objs, L, key, "Z")
        record_all(checks, "A8 Z", through_the_engine(eng, objs, L, consumers_of(L), models), want)
        ran = {n.split()[2] for n in checks.names}
        checks.record("A8 every consumer was compared", ran == set(consumers_of(L)) and len(checks.names) >= 3 * len(ran),
                      sorted(ran))
        if plan_name == "chunks3_overlap":
            want, _ = _cached_layout_free(eng, objs, L, key, "X")
            record_all(checks, "A8 X", through_the_engine(eng, objs, L, consumers_of(L, "X"), models, "X"), want)
    return checks


def check_layout_independence(kernels, dev, case, plan_name):
    run_layout_independence(kernels, dev, case, plan_name).assert_none_failed()


# ---- B: what run_current_table compares on top of the rankers ------------------------------------------------------------
class Later:
    """The later consumers of one run of B: the objects and models made before any sweep, and ``results`` of any engine
    holding the same table."""

    def __init__(self, eng, dtype, d):
        self.L = L = later_case(dtype, d, seed=3)
        self.only = tuple(n for n in B_CONSUMERS if L.has_distances or n != "knn7")
        self.old = make_objects(eng, em_iters=3)
        Z, rows = classify_mod.table_and_rows(eng, L.vertices)
        ones = torch.ones(rows.numel(), 1, dtype=torch.uint8)
        self.models = {"label": label_model_from(self.old["probe"].fit(Z, rows, L.y, ones, L.base.C, l2=[1.0]), L),
                       "mixture": self.old["mixture"].fit(Z, rows, L.base.K, init=L.resp0).model()}

    def results(self, eng, objs=None):
        objs = make_objects(eng, em_iters=3) if objs is None else objs
        return through_the_engine(eng, objs, self.L, self.only, self.models)


# ---- the comparisons bite ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def rows_from(fn):
    """``table_and_rows`` replaced by ``fn(eng, vertices, table)`` wherever a later consumer looks it up."""
    real = classify_mod.table_and_rows
    classify_mod.table_and_rows = mixture_mod.table_and_rows = fn
    try:
        yield real
    finally:
        classify_mod.table_and_rows = mixture_mod.table_and_rows = real


def _unmapped(eng, vertices, table="Z"):
    v = torch.as_tensor(vertices, dtype=torch.int64, device=eng.device).reshape(-1)
    return (eng.Zcur if table == "Z" else eng.X_loc), v.to(torch.int32).contiguous()


def record_all_differ(checks, tag, got, want, only):
    """Every data output of every consumer of ``only`` must DIFFER from the layout-free result."""
    seen = set()
    for name, t in got.items():
        consumer, output = name.split()
        if output in MAY_COINCIDE:
            continue
        seen.add(consumer)
        checks.record(f"{tag} {name} differs", not torch.equal(t, want[name]))
    checks.record(f"{tag} reached every consumer", seen == set(only), sorted(set(only) - seen))


def run_wrong_inputs(kernels, dev, run=WRONG_RUN):
    """The `Checks` of the GPU self-check: right inputs compare equal, each wrong input unequal, for every consumer."""
    case, plan_name = run
    L = later_case(*case)
    settings, route = X.PLANS[plan_name]
    checks = X.Checks(f"wrong inputs {X.plan_id(run)}")
    with X.device_ctx(dev):
        eng = X.make_engine(kernels, dev, L.base, **settings)
        route(eng, dev)
        pos_host = eng.pos.cpu()
        assert int((pos_host[L.vertices] != L.vertices).sum()) > L.vertices.numel() // 2
        assert eng.Zcur.shape[0] > int(L.vertices.max()) and eng.X_loc.shape[0] > int(L.vertices.max())   # nothing faults
        objs, key = make_objects(eng), (str(dev), case)
        on_Z, on_X = consumers_of(L), consumers_of(L, "X")
        want, models = _cached_layout_free(eng, objs, L, key, "Z")
        want_X, _ = _cached_layout_free(eng, objs, L, key, "X")
        # 1: the list not mapped through pos
        with rows_from(_unmapped):
            record_all_differ(checks, "unmapped Z", through_the_engine(eng, objs, L, on_Z, models), want, on_Z)
            record_all_differ(checks, "unmapped X", through_the_engine(eng, objs, L, on_X, models, "X"), want_X, on_X)
        # pos-mapped rows into X_loc: what looks like a mistake is, on one GPU, the right rows
        with rows_from(lambda e, v, table="Z": (e.X_loc, e.pos[torch.as_tensor(v, device=e.device).long()].to(torch.int32))):
            record_all(checks, "pos rows into X_loc ARE the right rows:", through_the_engine(eng, objs, L, on_X, models, "X"),
                       want_X)
        # 3: a mistake that exists -- the Z table where X was asked for
        with rows_from(lambda e, v, table="Z": (e.Zcur, e.pos[torch.as_tensor(v, device=e.device).long()].to(torch.int32))):
            record_all_differ(checks, "Z for X", through_the_engine(eng, objs, L, on_X, models, "X"), want_X, on_X)
        # 2: the table before the last sweep
        eng.sweep(X.GAMMA)
        assert eng.cur == 1 and eng._prev_cur == 0
        now, _ = layout_free(eng, objs, eng.get_Z().double(), L, on_Z, models)
        record_all(checks, "after a sweep", through_the_engine(eng, objs, L, on_Z, models), now)
        with rows_from(lambda e, v, table="Z": (e.Zbuf[e._prev_cur], e.pos[torch.as_tensor(v, device=e.device).long()].to(torch.int32))):
            record_all_differ(checks, "stale table", through_the_engine(eng, objs, L, on_Z, models), now, on_Z)
    return checks


def check_wrong_inputs(kernels, dev):
    run_wrong_inputs(kernels, dev).assert_none_failed()
