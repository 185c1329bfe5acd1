"""The float-data cases of tests/dense_bits_cases.py, without a GPU: the tests of tests/test_gpu_dense_bits.py must be
able to fail.

* the expectation functions (top-k lists, rank counts, arg-min and arg-max with ties to the lowest index) against plain
  Python loops on 20 x 40 inputs full of ties;
* mutation: every relation's comparison, fed with "kernel" results from dots summed in ascending k and "anchor" dots
  summed in descending k on the CPU, raises AssertionError;
* order sensitivity of the fixtures: the share of dots whose bits differ between two summation orders reaches a stated
  threshold, so an order change cannot hide in data that happen to sum exactly;
* composition: the planted ties exist, enough list indices fall outside the table, and at d = 130 no two candidates of a
  query tie unless they were planted."""
import pytest
import torch

from clane_amd import _hip

from . import dense_bits_cases as D

F32, F64, BF16 = D.F32, D.F64, D.BF16


# ---- the expectation functions against brute force ---------------------------------------------------------------------------
def _tied_inputs(seed, Q=20, V=40):
    g = torch.Generator().manual_seed(seed)
    scores = torch.randint(-3, 4, (Q, V), generator=g).float() / 4          # 7 values: every row is full of ties
    eligible = torch.rand(Q, V, generator=g) < 0.7
    eligible[3] = False                                                     # a query without candidates
    eligible[4, 5:] = False                                                 # ... and one with fewer than k
    label = torch.randperm(V, generator=g).to(torch.int32)
    label[7::9] = -1
    eligible &= (label >= 0)[None, :]
    return scores, eligible, label


@pytest.mark.parametrize("kk", [1, 10, 32])
def test_expect_topk_against_a_python_sort(kk):
    scores, eligible, label = _tied_inputs(1)
    got_s, got_i = D.expect_topk(scores, eligible, label, kk)
    for q in range(scores.shape[0]):
        cand = sorted((-float(scores[q, v]), int(label[v])) for v in range(scores.shape[1]) if eligible[q, v])[:kk]
        want_s = [-s for s, _ in cand] + [float("-inf")] * (kk - len(cand))
        want_i = [l for _, l in cand] + [-1] * (kk - len(cand))
        assert got_s[q].tolist() == want_s and got_i[q].tolist() == want_i, q


def test_expect_counts_against_python_loops():
    scores, eligible, label = _tied_inputs(2)
    Q, V = scores.shape
    g = torch.Generator().manual_seed(3)
    pair_q = torch.arange(Q).repeat_interleave(4)
    t_rows = torch.randint(0, V, (4 * Q,), generator=g).to(torch.int32)
    t_rows[5], t_rows[9] = -1, D.ROWS + 5                                   # targets outside the table
    unlabelled = int((label < 0).nonzero()[0])
    t_rows[13] = unlabelled
    got_t, got_c = D.expect_counts(scores, eligible, label, pair_q, t_rows)
    some_equal = 0
    for b in range(4 * Q):
        q, t = int(pair_q[b]), int(t_rows[b])
        if not (0 <= t < V) or label[t] < 0 or not bool(eligible[q].any()):
            assert got_c[b].tolist() == [-1] * 4 and float(got_t[b]) == float("-inf"), b
            continue
        c = [0, 0, 0, 0]
        for v in range(V):
            if not eligible[q, v] or v == t:
                continue
            c[3] += 1
            if scores[q, v] > scores[q, t]:
                c[0] += 1
            elif scores[q, v] == scores[q, t]:
                c[1 if label[v] < label[t] else 2] += 1
        assert got_c[b].tolist() == c and float(got_t[b]) == float(scores[q, t]), b
        some_equal += c[1] > 0 and c[2] > 0
    assert some_equal > 10


def test_expect_kmeans_and_expect_pred_take_the_lowest_index_among_equals():
    g = torch.Generator().manual_seed(4)
    dots = torch.randint(-2, 3, (2, 20, 40), generator=g).float()
    csq = torch.randint(0, 3, (2, 40), generator=g).float()
    assign, best = D.expect_kmeans(dots, csq)
    ties = 0
    for r in range(2):
        for i in range(20):
            vals = [float(csq[r, j] - 2 * dots[r, i, j]) for j in range(40)]
            assert float(best[i, r]) == min(vals) and int(assign[i, r]) == vals.index(min(vals))
            ties += vals.count(min(vals)) > 1
    assert ties > 10
    F, Cp, C = 5, 8, 7
    bias = torch.randint(-1, 2, (F, Cp), generator=g).float()
    bias[:, C:] = 100.0                                                     # a pad column never wins, whatever it holds
    pred = D.expect_pred(dots[0], bias, C)
    ties = 0
    for i in range(20):
        for f in range(F):
            vals = [float(dots[0, i, f * Cp + c] + bias[f, c]) for c in range(C)]
            assert int(pred[i, f]) == vals.index(max(vals))
            ties += vals.count(max(vals)) > 1
    assert ties > 10


# ---- mutation: each relation's comparison raises when the dots come from another order -------------------------------------------
def _two_orders(A, B):
    up, down = D.ascending(A, B), D.descending(A, B)
    assert not torch.equal(up, down)
    return up, down


def test_relation_1_pair_project_fails_on_another_order():
    d = 130
    Z, W = D.anchor_case(d, F32)
    up, down = _two_orders(Z, W)
    src, dst = D.row_list(3, 300), D.row_list(4, 300)
    D.assert_pair_project(*D.expect_pair_project(up, src, dst, d), up, src, dst, d)
    with pytest.raises(AssertionError):
        D.assert_pair_project(*D.expect_pair_project(up, src, dst, d), down, src, dst, d)


def _rank_orders(dtype):
    c = D.rank_case(130, dtype)
    up, down = _two_orders(D.gather(c.S, c.q_rows), c.N.to(_hip.acc_dtype(dtype)))
    return c, c.eligible(), up, down


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
def test_relation_2_top_k_fails_on_another_order(dtype):
    c, el, up, down = _rank_orders(dtype)
    for kk in D.RANK_K:
        D.assert_topk(*D.expect_topk(up, el, c.label, kk), up, el, c.label, kk)
        with pytest.raises(AssertionError):
            D.assert_topk(*D.expect_topk(up, el, c.label, kk), down, el, c.label, kk)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
def test_relation_3_rank_counts_fail_on_another_order(dtype):
    c, el, up, down = _rank_orders(dtype)
    t_rows = D.count_targets(c, up, el)
    pair_q = torch.arange(D.RANK_Q).repeat_interleave(D.TARGETS)
    got_t, got_c = D.expect_counts(up, el, c.label, pair_q, t_rows)
    assert int((got_c[:, 1] > 0).sum()) >= 1 and int((got_c[:, 2] > 0).sum()) >= 1      # the equal rows are counted
    slabs = torch.stack([got_c, torch.where(got_c < 0, got_c, torch.zeros_like(got_c))], dim=1)    # as two slabs
    D.assert_counts(got_t, slabs, up, el, c.label, pair_q, t_rows)
    with pytest.raises(AssertionError):
        D.assert_counts(got_t, slabs, down, el, c.label, pair_q, t_rows)


@pytest.mark.parametrize("K", D.KMEANS_K)
def test_relation_4_kmeans_fails_on_another_order(K):
    d = 130
    Z, rows = D.table(41, d, F32), D.row_list(42, 300)
    centres, csq, copies = D.kmeans_case(d, F32, K)
    both = [_two_orders(D.gather(Z, rows), centres[r]) for r in range(D.KMEANS_R)]
    up, down = torch.stack([b[0] for b in both]), torch.stack([b[1] for b in both])
    assign, best = D.expect_kmeans(up, csq)
    assert int((assign == D.DUP_CENTRES[0]).sum()) >= 1 and not bool(torch.isin(assign, torch.tensor(copies)).any())
    D.assert_kmeans(assign, best, up, csq)
    with pytest.raises(AssertionError):
        D.assert_kmeans(assign, best, down, csq)


def _near_tied_classes(seed, d, Cp, F):
    """Class weights that agree to about 2^-20: a uniform change of the order moves a decision only where two logits lie
    within rounding of each other, and these make such pairs common.  (On the card it is the planted EXACT ties that
    catch an order which depends on the tile; the next two tests model that.)"""
    w0 = D.randn(seed, (1, 1, d), F32, 0.3)
    W = w0 * (1 + D.randn(seed + 1, (F, Cp, d), F32, 2.0 ** -20))
    return W, torch.zeros(F, Cp)


def test_relation_5_arg_max_fails_on_another_order():
    d, C, Cp, F = 130, 7, 8, 19
    W, bias = _near_tied_classes(50, d, Cp, F)
    up, down = _two_orders(D.table(11, d, F32), W.view(F * Cp, d))
    D.assert_pred(D.expect_pred(up, bias, C), up, bias, C)
    with pytest.raises(AssertionError):
        D.assert_pred(D.expect_pred(up, bias, C), down, bias, C)


def _order_by_tile(A, B):
    """Dots whose order depends on the 16-column tile: ascending in the first tile of every 64 columns, descending in
    the others -- what mfma_tile.h rules out."""
    up, down = _two_orders(A, B)
    first = (torch.arange(B.shape[0]) % 64) < 16
    return up, torch.where(first[None, :], up, down)


def test_relation_5_arg_max_fails_when_the_order_depends_on_the_tile():
    d, (C, F) = 130, D.PROBE_SHAPES[2]
    c = D.softmax_case(d, F32, C, F)
    up, mixed = _order_by_tile(D.gather(c["Z"], c["rows"]), c["W"].view(F * c["Cp"], d))
    with pytest.raises(AssertionError):                                     # class 17 no longer ties with class 1
        D.assert_pred(D.expect_pred(mixed, c["bias"], C), up, c["bias"], C)


@pytest.mark.parametrize("top_k", [True, False], ids=["top_k", "threshold"])
def test_relation_6_label_masks_fail_on_another_order(top_k):
    d, C, Cp, F = 130, 7, 8, 19
    W, _ = _near_tied_classes(60, d, Cp, F)
    Z = D.table(11, d, F32)
    up, down = _two_orders(Z, W.view(F * Cp, d))
    # threshold mode decides on the sign: a bias that puts row 0's logits within rounding of 0
    bias = torch.zeros(F, Cp) if top_k else -up[0].view(F, Cp)
    Y = D.randint(20, 0, 4, (D.ROWS, C)) == 0
    state = torch.zeros(F, Cp, dtype=torch.int8)
    D.assert_masks(D.expect_masks(up, bias, state, Y, C, top_k), up, bias, state, Y, C, top_k)
    with pytest.raises(AssertionError):
        D.assert_masks(D.expect_masks(up, bias, state, Y, C, top_k), down, bias, state, Y, C, top_k)


def test_relation_6_label_masks_fail_when_the_order_depends_on_the_tile():
    d, (C, F) = 130, D.PROBE_SHAPES[2]
    c = D.ovr_case(d, F32, C, F)
    up, mixed = _order_by_tile(D.gather(c["Z"], c["rows"]), c["W"].view(F * c["Cp"], d))
    with pytest.raises(AssertionError):
        D.assert_masks(D.expect_masks(mixed, c["bias"], c["state"], c["Y"], C, True), up, c["bias"], c["state"], c["Y"],
                       C, True)


def test_relation_7_probe_grad_fails_on_another_order():
    d, n, K = 17, 300, 152
    Zg = D.gather(D.widen(D.table(11, d, BF16)), D.row_list(12, n))
    G = D.randn(17, (n, K), F32, 0.5)
    up, down = _two_orders(G.T.contiguous(), Zg.T.contiguous())
    dW, db = D.expect_probe_grad([up], G)
    D.assert_probe_grad(dW, db, [up], G)
    with pytest.raises(AssertionError):
        D.assert_probe_grad(dW, db, [down], G)
    with pytest.raises(AssertionError):                                     # db: the rows in one sequence, not by parity
        D.assert_probe_grad(dW, D.sum_in_order(list(G)), [up], G)


def test_expect_probe_grad_adds_chunks_in_order_and_rows_by_parity():
    G = D.randn(18, (2100, 3), F32)
    parts = [D.randn(19, (3, 5), F32), D.randn(20, (3, 5), F32)]
    dW, db = D.expect_probe_grad(parts, G)
    assert torch.equal(dW, parts[0] + parts[1])
    want = torch.zeros(3)
    for a, b in ((0, 2048), (2048, 2100)):
        halves = []
        for first in (a, a + 1):
            s = torch.zeros(3)
            for i in range(first, b, 2):
                s = s + G[i]
            halves.append(s)
        want = want + (halves[0] + halves[1])
    assert torch.equal(db, want) and D.chunks(2100) == [(0, 2048), (2048, 2100)]


def test_relation_8_pair_grad_fails_on_another_order():
    d, B = 17, 300
    Zw = D.widen(D.table(1, d, BF16))
    src, dst = D.row_list(5, B), D.row_list(6, B)
    PA, PB, g = D.randn(7, (B, d), F32), D.randn(8, (B, d), F32), D.randn(9, (B,), F32, 0.5)
    top = _two_orders((g[:, None] * PB).T.contiguous(), D.gather(Zw, src).T.contiguous())
    bottom = _two_orders((g[:, None] * PA).T.contiguous(), D.gather(Zw, dst).T.contiguous())
    dW = D.expect_pair_grad([top[0]], [bottom[0]])
    D.assert_pair_grad(dW, [top[0]], [bottom[0]])
    with pytest.raises(AssertionError):
        D.assert_pair_grad(dW, [top[1]], [bottom[0]])
    with pytest.raises(AssertionError):
        D.assert_pair_grad(dW, [top[0]], [bottom[1]])


# ---- order sensitivity of the fixtures: a condition, not a measurement -----------------------------------------------------------
def _share(A, B):
    """Share of the dots of A's rows with B's rows whose bits differ between ascending k and the slice order."""
    up = D.ascending(A, B)
    sliced = D.cpu_dots(A, B, D.slice_order(A.shape[1]))
    return float((up != sliced).float().mean())


def test_slice_order_is_a_permutation_that_differs_from_ascending():
    for d in D.RANK_D + (16, 33):
        order = D.slice_order(d)
        assert sorted(order) == list(range(d))
        assert (order != list(range(d))) == (d > 4)
    assert D.slice_order(17)[:5] == [0, 4, 8, 12, 1] and D.slice_order(17)[-1] == 16


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
@pytest.mark.parametrize("d,need", [(5, 1 / 4), (17, 1 / 2), (130, 1 / 2)])
def test_dots_with_a_full_mantissa_operand_depend_on_the_order(dtype, d, need):
    """f32 / f64 accumulation with W, centres, G in the accumulate dtype: 78 000 (d = 130) to 3 000 (d = 5) dots."""
    Z, W = D.anchor_case(d, dtype)
    share = _share(Z, W)
    print(f"order sensitivity {D.case_id(dtype)} d={d}: {share:.3f} of the dots differ (required {need:.2f})")
    assert share >= need


@pytest.mark.parametrize("d,need", [(130, 1 / 5), (17, None), (5, None), (1, None)])
def test_bf16_by_bf16_dots_of_the_ranking_kernels_depend_on_the_order_at_d_130(d, need):
    """Both operands bf16: every product is exact in f32 and a short sum of such products nearly always is, so at d <= 17
    the ranking cases are nearly exact BY CONSTRUCTION (d = 1 has no order at all) and are exempt from a threshold; they
    still run on the card, where the tie rule and the eligibility logic are what they test."""
    c = D.rank_case(d, BF16)
    share = _share(D.gather(c.S, c.q_rows), c.N.to(F32))
    print(f"order sensitivity bf16 x bf16 d={d}: {share:.3f} of the dots differ")
    assert need is None or share >= need


# ---- composition of the fixtures ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
def test_the_planted_ties_exist(dtype):
    acc = _hip.acc_dtype(dtype)
    for d in D.RANK_D:
        for seed in (1, 11, 31, 32, 41):
            Z = D.table(seed, d, dtype)
            assert Z.dtype == dtype and all(torch.equal(Z[r], Z[5]) for r in D.DUP_ROWS)
            assert d == 1 or int((Z == Z[5]).all(1).sum()) == 3
            assert not bool((Z.double() == Z.double().round()).all())       # not integer data
    for K in D.KMEANS_K:
        centres, csq, copies = D.kmeans_case(17, dtype, K)
        assert centres.dtype == acc and copies == ([7, 131] if K > 131 else [6])
        for j in copies:
            assert torch.equal(centres[:, j], centres[:, 3]) and torch.equal(csq[:, j], csq[:, 3])
    for C, F in D.PROBE_SHAPES:
        for W, bias in (D.probe_weights(14, 17, acc, _hip.probe_padded_classes(C), F),
                        D.probe_weights(18, 17, acc, _hip.ovr_padded_classes(C), F)):
            assert torch.equal(W[:, 2], W[:, 1]) and torch.equal(bias[:, 2], bias[:, 1])
            if W.shape[1] == 64:
                assert torch.equal(W[:, 40], W[:, 3]) and torch.equal(bias[:, 40], bias[:, 3])
                assert torch.equal(W[:, 17], W[:, 1]) and torch.equal(bias[:, 17], bias[:, 1])
        st = D.ovr_case(17, dtype, C, F)["state"]
        assert bool((st[:, [1, 2, 3]] == 0).all()) and bool((st == 1).any()) and bool((st == -1).any())


def test_row_lists_leave_the_table_and_hold_the_equal_rows():
    for seed in (3, 4, 5, 6, 12, 42):
        for n in D.LIST_N:
            idx = D.row_list(seed, n)
            assert idx.dtype == torch.int32 and idx.numel() == n
            assert int((idx == -1).sum()) >= 10 and int((idx == D.ROWS + 5).sum()) >= 10
            assert int((~D.inside(idx)).sum()) >= 20
            assert set(D.DUP_ROWS) <= set(idx.tolist())
            assert not bool(D.inside(idx[[63, 64, 127, 128]]).any())         # the tile edges read zero rows
    q = D.row_list(36, D.RANK_Q)
    assert int((~D.inside(q)).sum()) >= 8 and int(D.inside(q).sum()) > 100
    Z = D.table(1, 5, F32)
    rows = D.gather(Z, D.row_list(3, 300))
    assert float(rows[~D.inside(D.row_list(3, 300))].abs().sum()) == 0.0 and torch.equal(rows[0], Z[5])


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
@pytest.mark.parametrize("d", D.RANK_D)
def test_the_planted_ties_reach_a_decision(dtype, d):
    """What the card's checks assert about their fixtures before they compare, here with dots summed on the CPU: the
    equal rows meet in a top-k list and are counted on both sides of a target, pairs without a rank exist, rows choose the
    repeated centre, and a repeated class is some row's maximum."""
    acc = _hip.acc_dtype(dtype)
    c = D.rank_case(d, dtype)
    scores, el = D.ascending(D.gather(c.S, c.q_rows), c.N.to(acc)), c.eligible()
    _, ids32 = D.expect_topk(scores, el, c.label, 32)
    assert bool((ids32[D.inside(c.q_rows)] >= 0).all()) and D.duplicate_runs(ids32, c.label) >= 1
    pair_q = torch.arange(D.RANK_Q).repeat_interleave(D.TARGETS)
    _, counts = D.expect_counts(scores, el, c.label, pair_q, D.count_targets(c, scores, el))
    assert int((counts[:, 0] < 0).sum()) >= 6 * D.TARGETS
    assert int((counts[:, 1] > 0).sum()) >= 1 and int((counts[:, 2] > 0).sum()) >= 1
    if d == 1:
        return
    for K in D.KMEANS_K:
        centres, csq, _ = D.kmeans_case(d, dtype, K)
        rows = D.gather(D.table(41, d, dtype), D.row_list(42, 300))
        assign, _ = D.expect_kmeans(torch.stack([D.ascending(rows, centres[r]) for r in range(D.KMEANS_R)]), csq)
        assert int((assign == D.DUP_CENTRES[0]).sum()) >= 1
    for C, F in D.PROBE_SHAPES:
        c = D.softmax_case(d, dtype, C, F)
        l = D.logits_of(D.ascending(D.gather(c["Z"], c["rows"]), c["W"].view(-1, d)), c["bias"])[:, :, :C]
        assert int(((l == l.amax(2, keepdim=True)).sum(2) >= 2).sum()) >= 1


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
def test_ranking_ties_come_from_the_plants_only(dtype):
    """d = 130: the float64 scores of one query's candidates, the copies of row 5 left out, never coincide."""
    c = D.rank_case(130, dtype)
    valid = D.inside(c.q_rows)
    scores = D.gather(c.S, c.q_rows).double() @ c.N.double().T
    keep = torch.ones(D.ROWS, dtype=torch.bool)
    keep[list(D.DUP_ROWS[1:])] = False
    ranked = scores[valid][:, keep].sort(1).values
    assert bool((ranked[:, 1:] > ranked[:, :-1]).all())
    assert torch.equal(scores[:, 133], scores[:, 5]) and torch.equal(scores[:, 290], scores[:, 5])
    assert all(int(c.label[r]) >= 0 for r in D.DUP_ROWS) and int((c.label < 0).sum()) >= 5
    assert sorted(c.label[c.label >= 0].tolist()) == sorted(set(c.label[c.label >= 0].tolist()))
    rowptr, colidx = c.csr()
    for r in range(D.ROWS):                                                 # sorted, unique: what the kernels search
        cols = colidx[rowptr[r]:rowptr[r + 1]].long()
        assert bool((cols[1:] > cols[:-1]).all()) and bool(c.excl[r, cols].all())
    assert int(rowptr[-1]) == int(c.excl.sum()) > D.ROWS
    moved = c.rolled(D.ROLL)
    assert torch.equal(moved.N[(5 + D.ROLL) % D.ROWS], c.N[5]) and torch.equal(moved.eligible(), c.eligible().roll(D.ROLL, 1))
