"""New vertices against a finished table on the GPU: clane_embed_rows_* through NewVertexEmbedder / Graph.embed_new and the
CLI.  The checks are those of tests/new_vertex_cases.py (shared with the host suite's CPU double): against the float64
restatement of the reference's round, against the engine's own build_P + sweep, exact on integer data, bit-identical
whatever the position in the batch, the stop rule, and the table that is current under the engine's launch plans."""
import numpy as np
import pytest
import torch

from clane_amd import _hip
from clane_amd.engine import SweepEngine
from clane_amd.links import LinkRanker
from clane_amd.partition import HostCSR
from clane_amd.similarity import CosineSimilarity
from oracle import clane_oracle as O

from . import engine_exact_cases as X
from . import new_vertex_cases as N
from .exact_cases import BF16, F32, F64

pytestmark = pytest.mark.gpu

ONE_PER_LAYOUT = [(F32, 24), (F32, 300), (F64, 130), (F64, 300), (BF16, 3), (BF16, 520)]


@pytest.fixture(scope="module")
def dev():
    return _hip.require_gpu("cuda:0")


@pytest.fixture(scope="module")
def k():
    return _hip.kernels()


# ---- 1: against float64 on the CPU -----------------------------------------------------------------------------------
@pytest.mark.parametrize("score", N.SCORES)
@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_rounds_against_float64(k, dev, case, score):
    for n in (1, 2, 6):
        N.check_rounds(k, dev, case, score, n)


# ---- 2: against the engine itself ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(F32, 130), (F64, 24), (BF16, 300)], ids=N.case_id)
def test_one_round_is_the_engines_build_P_and_sweep(k, dev, case):
    """The full graph: the last 48 vertices have out-edges into the first 652 and no in-edges."""
    nv = N.V - N.M
    t = N.table(case[0], case[1], nv)
    lists, rowptr, cols, _ = N.batch(nv)
    old = N.table_csr(nv)
    full = HostCSR(N.V, np.concatenate([old.rowptr, old.rowptr[-1] + rowptr[1:]]),
                   np.concatenate([old.colidx, cols.astype(np.int32)]))
    with torch.cuda.device(dev):
        eng = SweepEngine(full, torch.cat([t.X, t.X_new]), dev, k, cosine_mode="per_edge")
        eng.set_Z(torch.cat([t.Z, t.X_new]))                 # z^0 = x for the arrivals
        eng.build_P()
        P = eng.P_global()[int(old.rowptr[-1]):].cpu()
        eng.sweep(N.GAMMA)
        Z = eng.get_Z()[nv:].cpu()
    res = N.embed(k, dev, t, "per_edge", gamma=N.GAMMA, tolerence=10, max_rounds=1, weights=True)
    err, p_err = O.rel_l2(res.Z.double(), Z.double()), float((res.P.double() - P.double()).abs().max())
    print(f"{N.case_id(case)}: rel_l2 = {err:.3e}, max |P - P_engine| = {p_err:.3e}")
    assert res.rowptr.tolist() == rowptr.tolist() and res.cols.tolist() == cols.tolist()
    assert err <= N.Z_BOUND[case[0]] and p_err <= N.P_BOUND


# ---- 3: exact --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score", ("reference", "per_edge"))
@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_integer_data_is_exact(k, dev, case, score):
    N.check_integers(k, dev, case, score)


@pytest.mark.parametrize("score", N.SCORES)
@pytest.mark.parametrize("case", ONE_PER_LAYOUT, ids=N.case_id)
def test_position_in_the_batch_changes_no_bit(k, dev, case, score):
    N.check_position(k, dev, case, score)


@pytest.mark.parametrize("score", N.SCORES)
@pytest.mark.parametrize("case", ONE_PER_LAYOUT, ids=N.case_id)
def test_degree_one_and_no_neighbours(k, dev, case, score):
    N.check_degree_one_and_none(k, dev, case, score)


def test_unaligned_operands_take_the_scalar_layout(k, dev):
    """Odd leading dimensions straight through the binding: the one-element-per-lane instances give the packed ones'
    result within the bound (another summation order), pads zero."""
    t = N.table(F32, 130)
    _, rowptr, cols, _ = N.batch()
    with torch.cuda.device(dev):
        eng = N.make_engine(k, dev, t, "per_edge")
        k.row_sqnorm(eng.Zcur, eng.d, eng.sq_pp[eng.cur])
        rp, ci = torch.from_numpy(rowptr).to(dev), eng.pos[torch.from_numpy(cols).to(dev)].to(torch.int32)
        out = {}
        for ld in (132, 131):
            Xd = torch.zeros(N.M, ld, device=dev)
            Xd[:, :130] = t.X_new.to(dev)
            Zo = torch.full((N.M, ld), 9.0, device=dev)
            rounds = torch.zeros(N.M, dtype=torch.int32, device=dev)
            delta = torch.zeros(N.M, device=dev)
            k.embed_rows(rp, ci, Xd, eng.Zcur, eng.Zcur.shape[0], 130, _hip.SCORE_PER_EDGE, None, eng.sq_pp[eng.cur], None,
                         N.GAMMA, 10, 3, Zo, rounds, delta)
            assert bool((Zo[:, 130:] == 0).all())
            out[ld] = Zo[:, :130].cpu()
    assert O.rel_l2(out[131], out[132]) <= N.Z_BOUND[F32] and not torch.equal(out[131], out[132])
    want, _ = N.restated(t, "per_edge", 3)
    assert O.rel_l2(out[131].double(), want) <= N.Z_BOUND[F32]


# ---- 4: stopping -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score", N.SCORES)
@pytest.mark.parametrize("case", [(F32, 24), (F32, 300), (F64, 130), (BF16, 24), (BF16, 520)], ids=N.case_id)
def test_every_row_stops_at_its_fixed_point(k, dev, case, score):
    N.check_stopping(k, dev, case, score)


# ---- 5: the table that is current ------------------------------------------------------------------------------------
PLANS = ("defaults", "chunks3_overlap", "tiles2_class")


@pytest.mark.parametrize("score", N.SCORES)
@pytest.mark.parametrize("plan", PLANS)
def test_the_current_table_under_the_engines_plans(k, dev, plan, score):
    settings, route = X.PLANS[plan]
    t = N.table(F32, 128)
    route(N.make_engine(k, dev, t, **settings), dev)
    N.check_current_table(k, dev, (F32, 128), score, settings)


@pytest.mark.parametrize("score", N.SCORES)
def test_a_prepared_link_ranker_stays_valid(k, dev, score):
    t = N.table(F32, 128)
    sim = N.similarity(t, score)
    with torch.cuda.device(dev):
        eng = N.make_engine(k, dev, t, "reference" if score == "bilinear" else score, **X.PLANS["chunks3_overlap"][0])
        ranker = LinkRanker(eng, sim)
        ids, scores = ranker.top_k(5, sources=[0, 3, 10, 699])
        N.embed(k, dev, t, score, eng=eng, gamma=N.GAMMA, weights=True)
        ids2, scores2 = ranker.top_k(5, sources=[0, 3, 10, 699], refresh=False)
    assert torch.equal(ids, ids2) and torch.equal(scores, scores2)


# ---- 6: the CLI ------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(dev, tmp_path, monkeypatch):
    N.run_cli_case(tmp_path, monkeypatch)


def test_graph_embed_new_returns_host_tensors_in_the_contents_dtype(dev):
    from clane_amd.graph import Graph
    t = N.table(BF16, 24)
    g = Graph.from_csr(N.table_csr(), t.X)
    g.set_Z(t.Z)
    lists = N.batch()[0]
    res = g.embed_new(CosineSimilarity(mode="per_edge"), t.X_new.float(), lists, gamma=N.GAMMA, max_rounds=6, tolerence=7)
    assert res.Z.dtype == BF16 and res.Z.device.type == "cpu" and res.P is None and res.Z.shape == (N.M, 24)
    want, _ = N.restated(t, "per_edge", 6)
    assert O.rel_l2(res.Z.double(), want) <= N.Z_BOUND[BF16]
    with pytest.raises(NotImplementedError, match="plug-in"):
        g.embed_new(lambda a, b: (a * b).sum(1), t.X_new, lists)
    with pytest.raises(ValueError, match="existing vertex"):
        g.embed_new(CosineSimilarity(), t.X_new[:1], [[N.V]])
