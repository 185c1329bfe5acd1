"""New vertices against a finished table -- helpers of tests/test_gpu_new_vertices.py (the HIP kernel) and
tests/test_new_vertices_host.py (the same checks through the CPU test double, plus the checks' self-checks).

The table is the 700-vertex ragged graph of tests/engine_exact_cases.py under the engine's own launch plans; the batch is
48 new rows of out-degrees {0, 1, 2, 3, 8, 63, 64, 65, 128, 129, 257, 700} (four of each; one list repeats a neighbour).
Every check takes the kernel object and the device: HipKernels on the card, the oracle-backed double on the host.

Bounds: rel_l2 of Z fp32 1e-5, fp64 1e-12, bf16 8e-3; weights within 2e-6 of the restated P.  The
float64 restatement is the reference's own round -- oracle.build_P_values / oracle.sweep on the augmented CSR whose only
edges are the new rows' -- iterated from the same rounded inputs.
"""
import functools
import json

import numpy as np
import torch

from clane_amd import _hip
from clane_amd.engine import SweepEngine
from clane_amd.induct import NewVertexEmbedder
from clane_amd.partition import HostCSR
from clane_amd.similarity import AsymmertricSimilarity, CosineSimilarity
from oracle import clane_oracle as O

from . import engine_exact_cases as X
from .exact_cases import BF16, F32, F64

V = 700
DEGREES = (0, 1, 2, 3, 8, 63, 64, 65, 128, 129, 257, 700)
M = 4 * len(DEGREES)
GAMMA = 0.76
Z_BOUND = {F32: 1e-5, F64: 1e-12, BF16: 8e-3}
P_BOUND = 2e-6
WIDTHS = {F32: (3, 24, 130, 300), F64: (3, 24, 130, 300), BF16: (3, 24, 130, 300, 520)}
CASES = [(t, d) for t in (F32, F64, BF16) for d in WIDTHS[t]]
SCORES = ("reference", "per_edge", "bilinear")


def case_id(case):
    return f"{_hip._SUFFIX[case[0]]}-d{case[1]}"


@functools.lru_cache(maxsize=None)
def batch(nv=V, seed=5):
    """The 48 neighbour lists over vertices [0, nv) as given by a user (list 15, of three neighbours, repeats its first
    one), and the coalesced CSR (rowptr int64, cols int64: sorted, unique) the embedder makes of them."""
    rng = np.random.default_rng(seed)
    lists = [np.sort(rng.choice(nv, size=min(dg, nv), replace=False)) for dg in DEGREES * 4]
    order = rng.permutation(M)                      # the degrees in no particular order over the batch
    lists = [rng.permutation(lists[i]) for i in order]
    dup = next(i for i, l in enumerate(lists) if l.size == 3)
    lists[dup] = np.concatenate([lists[dup], lists[dup][:1]])
    rowptr = np.zeros(M + 1, dtype=np.int64)
    uniq = [np.unique(l) for l in lists]
    np.cumsum([u.size for u in uniq], out=rowptr[1:])
    return lists, rowptr, np.concatenate(uniq).astype(np.int64), dup


class Table:
    """Float data for the table and the arrivals at (dtype, d), rounded to the dtype once; host tensors.  The bilinear
    similarity's Xavier weights are scaled by 0.3: |z| |z_v| is about d / 2 here, which leaves raw scores of 10..20, and a
    float32 score s carries an error of a few 2^-24 |s| sqrt(d) -- P's error is P times that, so the 2e-6 bound on the
    weights (set for cosines, |s| <= 1) only means something for scores of order 1."""

    def __init__(self, dtype, d, nv=V):
        rng = np.random.default_rng(4000 + d)
        self.dtype, self.d, self.acc, self.nv = dtype, d, _hip.acc_dtype(dtype), nv
        self.Z = torch.from_numpy(0.5 * rng.standard_normal((V, d))).to(dtype)[:nv]
        self.X = torch.from_numpy(rng.standard_normal((V, d))).to(dtype)[:nv]        # the table graph's own content
        self.X_new = torch.from_numpy(rng.standard_normal((M, d))).to(dtype)
        torch.manual_seed(77 + d)
        self.sim = AsymmertricSimilarity(n_dim=d)
        with torch.no_grad():
            self.sim.Phi_src.weight.mul_(0.3)
            self.sim.Phi_dst.weight.mul_(0.3)


@functools.lru_cache(maxsize=None)
def table(dtype, d, nv=V):
    return Table(dtype, d, nv)


def table_csr(nv=V):
    g = X.graph()
    if nv == V:
        return HostCSR(V, g.rowptr, g.sorted_colidx)
    rows = np.repeat(np.arange(V), g.deg)
    keep = (rows < nv) & (g.sorted_colidx < nv)
    rowptr = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=nv)[:nv], out=rowptr[1:])
    return HostCSR(nv, rowptr, g.sorted_colidx[keep].astype(np.int32))


def make_engine(kernels, dev, t, mode="reference", Z=None, csr=None, X_table=None, **settings):
    with X.device_ctx(dev):
        eng = SweepEngine(table_csr(t.nv) if csr is None else csr, t.X if X_table is None else X_table, dev, kernels,
                          cosine_mode=mode, **settings)
        eng.set_Z(t.Z if Z is None else Z)
    return eng


def similarity(t, score):
    return t.sim if score == "bilinear" else CosineSimilarity(mode=score)


def embed(kernels, dev, t, score, eng=None, X_new=None, lists=None, **kw):
    """NewVertexEmbedder on a fresh engine (or `eng`) for the batch (or `lists`); host results."""
    eng = make_engine(kernels, dev, t, "reference" if score == "bilinear" else score) if eng is None else eng
    if lists is None:
        lists = batch(t.nv)[0]
    from clane_amd.induct import normalize_neighbours
    X_new = t.X_new if X_new is None else X_new
    rowptr, cols = normalize_neighbours(lists, X_new.shape[0])
    with X.device_ctx(dev):
        return NewVertexEmbedder(eng, similarity(t, score)).embed(X_new, rowptr, cols, **kw).cpu()


# ---- the float64 restatement -------------------------------------------------------------------------------------------
def old_denominator(t):
    csr = table_csr(t.nv)
    return O.global_denominator(csr.rowptr, csr.colidx, t.Z.double())


def restated_round(t, score, rowptr, cols, z, X_new=None, Zt=None, denom=None):
    """One round of the reference on the augmented graph, new rows only, in float64: (z_new [m, d], P)."""
    Zt = t.Z.double() if Zt is None else Zt
    Xn = (t.X_new if X_new is None else X_new).double()
    nv = Zt.shape[0]
    rp = np.concatenate([np.zeros(nv, dtype=np.int64), rowptr])
    ci = cols.astype(np.int64)
    Zaug = torch.cat([Zt, z])
    if score == "bilinear":
        Ws, Wd = t.sim.Phi_src.weight.detach().double(), t.sim.Phi_dst.weight.detach().double()
        P = O.build_P_values(rp, ci, Zaug, similarity=lambda a, b: ((a @ Ws.T) * (b @ Wd.T)).sum(1))
    elif score == "per_edge":
        P = O.build_P_values(rp, ci, Zaug, "per_edge")
    else:                                           # the OLD graph's global denominator: the table is frozen
        D = old_denominator(t) if denom is None else denom
        P = O.segment_softmax(rp, O.edge_dots(rp, ci, Zaug) / D)
    new, _ = O.sweep(rp, ci, P, torch.cat([Zt, Xn]), Zaug, GAMMA)
    return new[nv:], P


def restated(t, score, n_rounds, X_new=None, lists=None, **kw):
    _, rowptr, cols, _ = batch(t.nv)
    if lists is not None:
        uniq = [np.unique(l) for l in lists]
        rowptr = np.concatenate([[0], np.cumsum([u.size for u in uniq])]).astype(np.int64)
        cols = np.concatenate(uniq).astype(np.int64) if uniq else np.zeros(0, dtype=np.int64)
    z = (t.X_new if X_new is None else X_new).double()
    P = None
    for _ in range(n_rounds):
        z, P = restated_round(t, score, rowptr, cols, z, X_new, **kw)
    return z, P


# ---- 1: against float64 ------------------------------------------------------------------------------------------------
def check_rounds(kernels, dev, case, score, n_rounds, embed_fn=embed, **ref_kw):
    t = table(*case)
    res = embed_fn(kernels, dev, t, score, gamma=GAMMA, tolerence=n_rounds + 1, max_rounds=n_rounds, weights=True)
    want, P = restated(t, score, n_rounds, **ref_kw)
    deg = np.diff(batch()[1])
    err = O.rel_l2(res.Z.double(), want)
    assert res.P.numel() == P.numel() and res.rowptr.tolist() == batch()[1].tolist()      # coalesced: repeats count once
    p_err = float((res.P.double() - P).abs().max())
    print(f"{case_id(case)} {score} rounds={n_rounds}: rel_l2(Z) = {err:.3e}, max |P - P64| = {p_err:.3e}")
    # exactly n_rounds (tolerence > max_rounds), unless the iterate reproduced itself before: a row of degree one does so
    # in round 2, and stopping there changes no bit
    rounds, at_rest = res.rounds.numpy(), res.delta.numpy() == 0
    assert (rounds[deg == 0] == 0).all() and (rounds[deg == 1] == min(n_rounds, 2)).all()
    assert ((rounds[deg > 0] == n_rounds) | ((rounds[deg > 0] < n_rounds) & at_rest[deg > 0])).all(), rounds.tolist()
    assert err <= Z_BOUND[case[0]], (err, Z_BOUND[case[0]])
    assert p_err <= P_BOUND, p_err
    assert res.Z.dtype == case[0] and res.P.dtype == t.acc and res.delta.dtype == t.acc
    return err, p_err


# ---- 3: exact ------------------------------------------------------------------------------------------------------------
POW2 = (1, 2, 4, 8, 16, 32, 64, 128, 256)


class IntegerCase:
    """max_rounds = 1, gamma = 1/2, power-of-two degrees: the table is non-zero integers in [-4, 4] in its first d - 2
    columns and zero in the last two; X_new is non-zero only there.  Every score is then exactly 0, P exactly 1 / deg,
    and z = x + sum(z_v) / (2 deg) a multiple of 2^-9 below 8: exact in all three dtypes, whatever the order."""

    def __init__(self, dtype, d):
        assert d >= 3
        rng = np.random.default_rng(6000 + d)
        self.dtype, self.d, self.acc, self.nv = dtype, d, _hip.acc_dtype(dtype), V
        Z = torch.from_numpy(rng.integers(1, 5, size=(V, d)) * rng.choice([-1, 1], size=(V, d))).double()
        Z[:, d - 2:] = 0
        Xn = torch.zeros(len(POW2) * 2, d, dtype=torch.float64)
        Xn[:, d - 2:] = torch.from_numpy(rng.integers(1, 5, size=(len(POW2) * 2, 2))).double()
        self.Z, self.X, self.X_new = Z.to(dtype), Z.to(dtype), Xn.to(dtype)
        self.lists = [np.sort(rng.choice(V, size=dg, replace=False)) for dg in POW2 * 2]
        self.sim = None
        # int64 reference: 2 deg z = 2 deg x + sum z_v
        num = torch.stack([2 * l.size * Xn[i].long() + Z[torch.from_numpy(l)].long().sum(0)
                           for i, l in enumerate(self.lists)])
        den = torch.tensor([2 * l.size for l in self.lists]).double().unsqueeze(1)
        ref = num.double() / den                                    # dyadic, exact in float64
        self.expect = ref.to(dtype)                                 # rounded once
        assert self.expect.double().equal(ref) or dtype == BF16
        self.delta = (ref - Xn).abs().sum(1)
        self.P = torch.cat([torch.full((l.size,), 1.0 / l.size, dtype=torch.float64) for l in self.lists])


@functools.lru_cache(maxsize=None)
def integer_case(dtype, d):
    return IntegerCase(dtype, d)


def check_integers(kernels, dev, case, score, embed_fn=embed):
    c = integer_case(*case)
    res = embed_fn(kernels, dev, c, score, lists=c.lists, gamma=0.5, tolerence=10, max_rounds=1, weights=True)
    assert torch.equal(res.Z, c.expect), (res.Z.double() - c.expect.double()).abs().max()
    assert torch.equal(res.P.double(), c.P)
    assert res.rounds.tolist() == [1] * len(c.lists)
    assert torch.equal(res.delta.double(), c.delta)   # taken in the accumulate type, before the final rounding


def same_bits(a, b, rows_a, rows_b, what):
    """The listed vertices' results in two runs are the same bits: Z, rounds, delta and weights."""
    for name in ("Z", "rounds", "delta"):
        x, y = getattr(a, name)[rows_a], getattr(b, name)[rows_b]
        assert torch.equal(x, y) or bool(((x == y) | ((x != x) & (y != y))).all()), (what, name)
    for i, j in zip(rows_a, rows_b):
        pa = a.P[int(a.rowptr[i]):int(a.rowptr[i + 1])]
        pb = b.P[int(b.rowptr[j]):int(b.rowptr[j + 1])]
        assert torch.equal(pa, pb), (what, "P", i, j)


def check_position(kernels, dev, case, score, embed_fn=embed):
    t = table(*case)
    lists = batch()[0]
    kw = dict(gamma=GAMMA, tolerence=3, max_rounds=12, weights=True)
    base = embed_fn(kernels, dev, t, score, **kw)
    assert len(set(base.rounds.tolist())) > 2                        # rows stop at different rounds
    perm = np.random.default_rng(9).permutation(M)
    moved = embed_fn(kernels, dev, t, score, X_new=t.X_new[torch.from_numpy(perm)], lists=[lists[i] for i in perm], **kw)
    same_bits(base, moved, perm.tolist(), list(range(M)), "permuted")
    for i in (int(np.argmax([l.size for l in lists])), batch()[3], 0):
        alone = embed_fn(kernels, dev, t, score, X_new=t.X_new[i:i + 1], lists=[lists[i]], **kw)
        same_bits(base, alone, [i], [0], f"alone {i}")
    pad = [lists[(7 * i) % M] for i in range(37)]                    # other rows in front and behind: another workgroup
    Xp = t.X_new[torch.tensor([(5 * i) % M for i in range(37)])]
    padded = embed_fn(kernels, dev, t, score, X_new=torch.cat([Xp, t.X_new, Xp]), lists=pad + list(lists) + pad, **kw)
    same_bits(base, padded, list(range(M)), list(range(37, 37 + M)), "padded")


def check_degree_one_and_none(kernels, dev, case, score, embed_fn=embed):
    t = table(*case)
    res = embed_fn(kernels, dev, t, score, gamma=GAMMA, tolerence=10, max_rounds=64, weights=True)
    deg = np.diff(batch()[1])
    for i in np.nonzero(deg == 1)[0]:
        assert int(res.rounds[i]) == 2 and float(res.delta[i]) == 0.0
        assert float(res.P[int(res.rowptr[i])]) == 1.0
    none = np.nonzero(deg == 0)[0]
    assert none.size == 4
    for i in none:
        assert int(res.rounds[i]) == 0 and torch.equal(res.Z[i], t.X_new[i]) and float(res.delta[i]) == 0.0


# ---- 4: stopping ---------------------------------------------------------------------------------------------------------
def check_stopping(kernels, dev, case, score, embed_fn=embed):
    t = table(*case)
    res = embed_fn(kernels, dev, t, score, gamma=GAMMA, tolerence=10, max_rounds=200)
    assert bool(res.converged.all()), res.rounds.tolist()
    _, rowptr, cols, _ = batch()
    z = res.Z.double()
    Fz, _ = restated_round(t, score, rowptr, cols, z)
    has = torch.from_numpy(np.diff(rowptr) > 0)
    resid = ((Fz - z).abs().sum(1) / z.abs().sum(1))[has]
    print(f"{case_id(case)} {score}: rounds {int(res.rounds.min())}..{int(res.rounds.max())}, "
          f"residual max {float(resid.max()):.3e}")
    assert float(resid.max()) <= Z_BOUND[case[0]], float(resid.max())
    return res


# ---- 5: the table that is current ----------------------------------------------------------------------------------------
def moved_engines(kernels, dev, t, mode, settings):
    """(name, engine) in the three states in which nobody has left the current table's norms behind."""
    def fresh():
        eng = make_engine(kernels, dev, t, mode, **settings)
        eng.build_P()
        return eng
    with X.device_ctx(dev):
        a = fresh()
        a.sweep(GAMMA)
        yield "after a sweep", a
        b = fresh()
        b.snapshot()
        b.sweep(GAMMA)
        yield "after snapshot + sweep", b
        c = fresh()
        c.sweep(GAMMA)
        c.set_Z(t.Z.flip(0))
        yield "after set_Z", c


def check_current_table(kernels, dev, case, score, settings):
    t = table(*case)
    mode = "reference" if score == "bilinear" else score
    kw = dict(gamma=GAMMA, tolerence=3, max_rounds=8, weights=True)
    for name, eng in moved_engines(kernels, dev, t, mode, settings):
        assert not eng.sq_ok[eng.cur], name                      # K0 has to run
        with X.device_ctx(dev):
            Zc = eng.get_Z()
        got = embed(kernels, dev, t, score, eng=eng, **kw)
        want = embed(kernels, dev, t, score, eng=make_engine(kernels, dev, t, mode, Z=Zc), **kw)
        assert not torch.equal(Zc, t.Z), name                    # the table did move
        same_bits(got, want, list(range(M)), list(range(M)), name)


# ---- 6: the CLI ----------------------------------------------------------------------------------------------------------
CONFIG = ("graph:\n  embedding_dim: 4\n\nsimilarity:\n  method: \"CosineSimilarity\"\n  kwargs: {}\n\n"
          "embedder:\n  gamma: 0.76\n  tolerence: 3\n")


def write_arrivals(root, V="n0\nn1\n", E="n0\ta\nn1\tb\nn1\ta\n", C_=np.zeros((2, 4), dtype=np.float32), pt=False):
    root.mkdir(parents=True, exist_ok=True)
    for name in ("V", "E", "C.npy", "C.pt"):
        if (root / name).exists():
            (root / name).unlink()
    if V is not None:
        (root / "V").write_text(V)
    if E is not None:
        (root / "E").write_text(E)
    if C_ is not None:
        if pt:
            torch.save(torch.from_numpy(C_), root / "C.pt")
        else:
            np.save(root / "C.npy", C_)
    return root


def run_cli_case(tmp_path, monkeypatch, kernels=None):
    """The CLI with the section on the karate graph (`kernels`: a test double's engine on the host; None: the GPU): the files it writes, the row
    order of root/V, and Z_new.npy == Graph.embed_new on the same inputs.  Shared with the GPU suite."""
    import clane_amd.__main__ as M
    from clane_amd.graph import Graph
    from .conftest import load_golden, write_data_root
    k = load_golden("g2_karate_csr.npz")
    rng = np.random.default_rng(0)
    Xc = rng.standard_normal((34, 4)).astype(np.float32)
    root = write_data_root(tmp_path / "karate", k["vertex_ids"], k["edge_src"], k["edge_dst"], Xc)
    ids = [str(v) for v in k["vertex_ids"]]
    new_ids = ["new-b", "new-a", "new-c", "new-d"]
    lists = [[3, 9, 3], [0], [], list(range(34))]
    Xn = rng.standard_normal((4, 4)).astype(np.float32)
    write_arrivals(root / "arrivals", V="\n".join(new_ids) + "\n",
              E="".join(f"{new_ids[i]}\t{ids[v]}\n" for i in (3, 0, 1) for v in lists[i]), C_=Xn)
    gpu = kernels is None
    if not gpu:
        def cpu_engine(self, device=None, cosine_mode="reference", **kw):
            if self._engine is None:
                self._attach_engine(SweepEngine(self.csr, self.X, "cpu", kernels, cosine_mode=cosine_mode))
            if self._dirty:
                self._engine.set_Z(self._Z_host)
                self._dirty = False
            return self._engine
        monkeypatch.setattr(Graph, "engine", cpu_engine)

    def run(cfg_text, out):
        cfg = tmp_path / f"{out}.yaml"
        cfg.write_text(cfg_text)
        M.embedding(M.get_parser().parse_args(["--data_root", str(root), "--output_root", str(tmp_path / out),
                                               "--config_file", str(cfg)] + (["--gpu"] if gpu else [])))
    run(CONFIG, "plain")
    assert not (tmp_path / "plain" / "Z_new.npy").exists() and not (tmp_path / "plain" / "new_vertices.json").exists()
    run(CONFIG + "\nnew_vertices:\n  root: arrivals\n  max_rounds: 40\n  weights: true\n", "new")
    out = tmp_path / "new"
    assert (tmp_path / "plain" / "Z.npy").read_bytes() == (out / "Z.npy").read_bytes()
    got = json.loads((out / "new_vertices.json").read_text())
    assert set(got) == {"new_vertices", "edges", "max_rounds", "rounds_histogram", "not_converged", "without_neighbours",
                        "similarity"}
    assert got["new_vertices"] == 4 and got["edges"] == 2 + 1 + 34 and got["without_neighbours"] == 1
    assert got["similarity"] == "CosineSimilarity" and got["max_rounds"] == 40 and got["not_converged"] == 0
    assert sum(got["rounds_histogram"].values()) == 4 and got["rounds_histogram"]["0"] == 1 and got["rounds_histogram"]["2"] == 1
    Z_new = np.load(out / "Z_new.npy")
    g = Graph(data_root=root, embedding_dim=4)
    g.set_Z(torch.from_numpy(np.load(out / "Z.npy")))
    res = g.embed_new(CosineSimilarity(), torch.from_numpy(Xn), lists, gamma=0.76, tolerence=3, max_rounds=40, weights=True)
    assert np.array_equal(Z_new, res.Z.numpy()) and np.array_equal(Z_new[2], Xn[2])          # rows in root/V order
    rows = [l.split("\t") for l in (out / "P_new.tsv").read_text().splitlines()]
    assert [r[0] for r in rows] == ["new-b"] * 2 + ["new-a"] + ["new-d"] * 34
    assert [r[1] for r in rows[:3]] == [ids[3], ids[9], ids[0]]
    assert np.allclose([float(r[2]) for r in rows], res.P.double().numpy(), rtol=1e-8)
    run(CONFIG + "\nnew_vertices:\n  root: arrivals\n", "noweights")
    assert not (tmp_path / "noweights" / "P_new.tsv").exists()
    assert (tmp_path / "noweights" / "Z_new.npy").read_bytes() == (out / "Z_new.npy").read_bytes()


