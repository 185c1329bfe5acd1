"""The float-data cases of tests/distance_bits_cases.py, without a GPU: the tests of tests/test_gpu_distance_bits.py
must be able to fail.

* the expectation functions against plain Python on small inputs full of ties: the neighbour order, the knock-out rounds
  with fills, and the silhouette sum order against a literal lane-by-lane walk of the kernel's loops;
* the one-rounding fma (float32 and float64) and the fused cosine step against exact rationals;
* mutation: every relation's comparison, fed with "kernel" results from dots summed in ascending k and "anchor" dots
  summed in descending k on the CPU, raises AssertionError, once per dtype that has the instance;
* the sum order of relation 10: in float64 the documented order and the plain ascending order give other bits in at
  least a quarter of the cells with two or more members; in float32 the double sums are exact in ANY order (they equal
  math.fsum), so those dtypes pin the distances and float64 alone pins the order;
* composition: the planted ties and near-duplicates exist and reach the clusters, the lists and the clamp."""
import math
from fractions import Fraction

import pytest
import torch

from clane_amd import _hip

from . import dense_bits_cases as D
from . import distance_bits_cases as X

F32, F64, BF16 = D.F32, D.F64, D.BF16
ORDERS = {"ascending": D.ascending, "descending": D.descending}


def _operand(dtype, d=130, mu_kind="random", n=D.ROWS):
    acc = _hip.acc_dtype(dtype)
    return X.operand(X.dist_table(d, dtype), X.positions(n), X.mu_case(d, acc, mu_kind))


def _two_orders(a):
    up, down = D.ascending(a, a), D.descending(a, a)
    assert not torch.equal(up, down)
    return up, down


# ---- the expectation functions against plain Python ---------------------------------------------------------------------------
@pytest.mark.parametrize("kk", [1, 7, 12])
def test_expect_knn_against_a_python_sort(kk):
    n = 10
    g = torch.Generator().manual_seed(1)
    Dm = torch.randint(0, 4, (n, n), generator=g).float() / 4              # 4 values: every row is full of ties
    ids, sqd = X.expect_knn(Dm, kk)
    for i in range(n):
        cand = sorted((float(Dm[i, j]), j) for j in range(n) if j != i)[:kk]
        assert ids[i].tolist() == [j for _, j in cand] + [-1] * (kk - len(cand)), i
        assert sqd[i].tolist() == [s for s, _ in cand] + [float("inf")] * (kk - len(cand)), i
    assert X.tied_places(sqd) > 0 or kk == 1


def test_expect_top_against_literal_knock_out_rounds():
    n, F, C = 20, 3, 7
    g = torch.Generator().manual_seed(2)
    values = torch.randint(-2, 3, (n, F, C), generator=g).float() / 2      # 5 values: ties in every list
    values[:, 0, 4] = float("nan")
    values[:, 1, 5] = float("-inf")
    values[:, 2, 0] = float("inf")
    values[:, 2, 3] = float("inf")
    values[3, 2, :] = float("-inf")                                         # a fit without an open column
    got = X.expect_top(values, 8)
    fills = 0
    for i in range(n):
        for f in range(F):
            is_open = [bool(values[i, f, c] > float("-inf")) for c in range(C)]
            want = []
            for _ in range(8):                                              # label_predict.h: max, lowest class among equals
                live = [c for c in range(C) if is_open[c]]
                if not live:
                    want.append(-1)
                    continue
                best = max(float(values[i, f, c]) for c in live)
                win = min(c for c in live if float(values[i, f, c]) == best)
                is_open[win] = False
                want.append(win)
            assert got[i, f].tolist() == want, (i, f)
            fills += want.count(-1)
    assert fills >= 8 + 2 * n and not bool((got[:, 0] == 4).any()) and not bool((got[:, 1] == 5).any())
    assert torch.equal(X.expect_top(values, 3), got[:, :, :3]) and X.tied_choices(values, got) > n


def _lane_walk(row, beg, end):
    """silhouette_sums_kernel's loops for one row, literally: 32 lanes (wn, li) with a running sum each; a lane's column
    of tile j0 and step ni is j0 + wn + 16 ni + li; butterfly over li; the two column halves meet."""
    run = {(wn, li): 0.0 for wn in (0, 64) for li in range(16)}
    for j0 in range(beg, end, 128):
        for ni in range(4):
            for wn, li in run:
                j = j0 + wn + 16 * ni + li
                run[wn, li] += float(row[j]) if j < end else 0.0
    halves = []
    for wn in (0, 64):
        v = [run[wn, li] for li in range(16)]
        for mask in (8, 4, 2, 1):
            v = [v[li] + v[li ^ mask] for li in range(16)]
        halves.append(v[0])
    return halves[0] + halves[1]


@pytest.mark.parametrize("seg", [X.SEG, (0, 300), (0, 7, 7, 136, 300)], ids=str)
def test_documented_sums_against_a_lane_by_lane_walk(seg):
    dist = D.randn(3, (4, 300), F64).abs()
    S = X.documented_sums(dist, seg)
    other = 0
    for p in range(4):
        for c in range(len(seg) - 1):
            assert float(S[p, c]) == _lane_walk(dist[p], seg[c], seg[c + 1]), (p, c)
            other += float(S[p, c]) != float(X.ascending_sums(dist, seg)[p, c])
    assert other >= 4                                                       # and it is not the plain order


# ---- the one-rounding steps against exact rationals --------------------------------------------------------------------------
def _rounded(fr, dtype):
    """The float of `dtype` nearest to the rational fr, ties to even: Python rounds int / int correctly to float64; for
    float32 the candidates are the float32 neighbours of that double, compared exactly."""
    x = fr.numerator / fr.denominator
    if dtype == F64:
        return x
    c = torch.tensor(x, dtype=F64).float()
    inf = torch.tensor(float("inf"))
    cands = [float(torch.nextafter(c, -inf)), float(c), float(torch.nextafter(c, inf))]
    best = min(cands, key=lambda v: (abs(Fraction(v) - fr), int(torch.tensor(v, dtype=F32).view(torch.int32)) & 1))
    return best


@pytest.mark.parametrize("dtype,count", [(F32, 20000), (F64, 4000)], ids=["f32", "f64"])
def test_fma_acc_rounds_once(dtype, count):
    """x y + z with z cancelling the rounded product, 2^-30 .. 2^30 times its size, or of its size: in more than a tenth
    of the values two roundings and one disagree."""
    x, y = D.randn(4, (count,), dtype), D.randn(5, (count,), dtype)
    z = D.randn(6, (count,), dtype)
    near = -(x * y)                                                         # cancels all but the product's rounding error
    scale = 2.0 ** torch.randint(-30, 30, (count,), generator=torch.Generator().manual_seed(7)).to(dtype)
    z = torch.where(torch.arange(count) % 3 == 0, near, torch.where(torch.arange(count) % 3 == 1, z * scale, z))
    got = X.fma_acc(x, y, z)
    twice = x * y + z
    differ = 0
    for i in range(count):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        assert float(got[i]) == _rounded(exact, dtype), i
        differ += float(twice[i]) != float(got[i])
    assert differ > count // 10                                             # the check can tell one rounding from two


def test_sqnorm_chain_and_fused_cosine_step_against_exact_rationals():
    a = _operand(BF16, 17)[:40]
    sq = X.expect_sqnorm(a)
    for i in range(a.shape[0]):
        s = 0.0
        for kk in range(a.shape[1]):
            s = _rounded(Fraction(float(a[i, kk])) ** 2 + Fraction(s), F32)
        assert float(sq[i]) == s, i
    for dtype in (F32, F64):
        aa = _operand(dtype, 17)[:30]
        dots = D.ascending(aa, aa)
        nrm = X.expect_norms(dots, "cosine")
        fused = X.expect_distances(dots, nrm, "cosine", fused=True)
        apart = X.expect_distances(dots, nrm, "cosine", fused=False)
        assert not torch.equal(fused, apart)
        for i in range(30):
            for j in range(30):
                t = dots[i, j] * nrm[i]
                want = _rounded(1 - Fraction(float(t)) * Fraction(float(nrm[j])), dtype) if i != j else 0.0
                assert float(fused[i, j]) == max(want, 0.0), (i, j)


def test_norms_and_euclidean_steps_are_single_roundings():
    """1 / sqrt in two correctly rounded steps and s - 2 dot in one, against exact rationals / the float64 route."""
    for dtype in (F32, F64):
        a = _operand(dtype, 17)[:60]
        dots = D.ascending(a, a)
        r = X.expect_norms(dots, "cosine")
        sq = X.expect_norms(dots, "euclidean")
        roots = X.sqrt_acc(sq)
        for i in range(60):
            root = float(roots[i])
            lo = float(torch.nextafter(roots[i], torch.tensor(0.0, dtype=dtype)))
            hi = float(torch.nextafter(roots[i], torch.tensor(float("inf"), dtype=dtype)))
            # correctly rounded: sq lies between the squares of the midpoints to the two neighbours
            assert ((Fraction(lo) + Fraction(root)) / 2) ** 2 < Fraction(float(sq[i])) < ((Fraction(root) + Fraction(hi)) / 2) ** 2
            assert float(r[i]) == _rounded(1 / Fraction(root), dtype), i
        v = (sq[:, None] + sq[None, :]) - 2 * dots
        route = ((sq[:, None] + sq[None, :]).double() + (-2 * dots).double()).to(dtype)    # exact in float64, cast once
        assert torch.equal(v, route)
    z = torch.zeros(3, 3)
    assert torch.equal(X.expect_norms(z, "cosine"), torch.zeros(3)) and torch.equal(X.expect_norms(z, "euclidean"), torch.zeros(3))


# ---- mutation: each relation's comparison raises when the dots come from another order -----------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
@pytest.mark.parametrize("metric", X.METRICS)
def test_relation_9_norms_fail_on_another_order(dtype, metric):
    up, down = _two_orders(_operand(dtype))
    X.assert_norms(X.expect_norms(up, metric), up, metric)
    with pytest.raises(AssertionError):
        X.assert_norms(X.expect_norms(up, metric), down, metric)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
@pytest.mark.parametrize("metric", X.METRICS)
def test_relation_10_sums_fail_on_another_order_of_the_dots_and_of_the_sum(dtype, metric):
    up, down = _two_orders(_operand(dtype))
    nrm = X.expect_norms(up, metric)
    for form in X.SUM_FORMS[metric]:
        S = X.expect_sums(up, nrm, metric, form)
        assert form in X.assert_sums(S, up, nrm, metric)
        assert X.assert_sums(S[37:205], up, nrm, metric, 37, 205)
        with pytest.raises(AssertionError):
            X.assert_sums(S, down, nrm, metric)
        with pytest.raises(AssertionError):                                 # one cell, one unit in the last place
            wrong = S.clone()
            wrong[200, 4] = torch.nextafter(wrong[200, 4], torch.tensor(float("inf"), dtype=F64))
            X.assert_sums(wrong, up, nrm, metric)
    if dtype == F64:                                                        # a wrong partial order: float64 sees it
        with pytest.raises(AssertionError):
            X.assert_sums(X.ascending_sums(X.expect_distances(up, nrm, metric)), up, nrm, metric)
    if metric == "cosine":                                                  # a build that mixes the two forms fails
        mixed = X.expect_sums(up, nrm, metric, "separate")
        mixed[150:] = X.expect_sums(up, nrm, metric, "fused")[150:]
        with pytest.raises(AssertionError):
            X.assert_sums(mixed, up, nrm, metric)


@pytest.mark.parametrize("dtype", X.FLOAT_DTYPES, ids=D.case_id)
def test_relation_11_sqdist_fails_on_another_order_mirror_or_clamp(dtype):
    a = _operand(dtype)
    up, down = _two_orders(a)
    sq = X.expect_sqnorm(a)
    Dm = X.expect_sqdist(sq, up)
    X.assert_sqdist(sq, Dm, a, up)
    with pytest.raises(AssertionError):
        X.assert_sqdist(sq, Dm, a, down)
    with pytest.raises(AssertionError):                                     # sq summed in the contraction's order instead
        X.assert_sqdist(up.diagonal().clone(), Dm, a, up)
    with pytest.raises(AssertionError):                                     # a mirrored element from another value
        wrong = Dm.clone()
        wrong[200, 3] = torch.nextafter(wrong[200, 3], torch.tensor(float("inf")))
        X.assert_sqdist(sq, wrong, a, up)
    with pytest.raises(AssertionError):                                     # no clamp
        X.assert_sqdist(sq, X.unclamped(sq, up).fill_diagonal_(0), a, up)
    with pytest.raises(AssertionError):                                     # the clamp before the rounding: s - 2 dot in double
        v = (sq[:, None] + sq[None, :]).double() - 2 * D.ascending(a.double(), a.double())
        X.assert_sqdist(sq, v.clamp_min(0).float().fill_diagonal_(0), a, up)


@pytest.mark.parametrize("dtype", X.FLOAT_DTYPES, ids=D.case_id)
@pytest.mark.parametrize("kk", X.KNN_K)
def test_relation_12_knn_fails_on_another_order_and_on_ties_by_anything_else(dtype, kk):
    a = _operand(dtype)
    up, down = _two_orders(a)
    sq = X.expect_sqnorm(a)
    Du, Dd = X.expect_sqdist(sq, up), X.expect_sqdist(sq, down)
    ids, sqd = X.expect_knn(Du, kk)
    X.assert_knn(ids, sqd, Du, kk)
    with pytest.raises(AssertionError):
        X.assert_knn(ids, sqd, Dd, kk)
    assert X.tied_places(sqd) >= 1
    # ties broken by the highest position instead: the same distances, other ids
    flipped = torch.sort(Du.clone().fill_diagonal_(float("inf")).flip(1), dim=1, stable=True).indices[:, :kk]
    wrong = (D.ROWS - 1 - flipped).to(torch.int32)
    assert torch.equal(Du.gather(1, wrong.long()), sqd)
    with pytest.raises(AssertionError):
        X.assert_knn(wrong, sqd, Du, kk)


def test_relation_12_five_rows_end_in_fills():
    a = _operand(F32, 17, n=5)
    ids, sqd = X.expect_knn(X.expect_sqdist(X.expect_sqnorm(a), D.ascending(a, a)), 7)
    assert bool((ids[:, 4:] == -1).all()) and bool(torch.isinf(sqd[:, 4:]).all()) and bool((ids[:, :4] >= 0).all())
    # positions 0, 2 and 4 hold the equal rows: one distance (rounding noise or 0), the lower position first
    assert sorted(ids[0, :4].tolist()) == [1, 2, 3, 4] and ids[0, :2].tolist() == [2, 4] and float(sqd[0, 0]) == float(sqd[0, 1])


def _near_tied_weights(seed, d, Cp, F, acc):
    """Class weights that agree to about 16 units in the last place: a uniform change of the order moves a choice only
    where two values lie within rounding of each other, and these make such pairs common."""
    w0 = D.randn(seed, (1, 1, d), acc, 0.3)
    return w0 * (1 + D.randn(seed + 1, (F, Cp, d), acc, 16 * D.UNIT[acc]))


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
@pytest.mark.parametrize("sigmoid", [False, True], ids=["soft-max", "sigmoid"])
def test_relation_13_top_classes_fail_on_another_order(dtype, sigmoid):
    """assert_predict can fail on a UNIFORM change of the order -- shown on stand-in weights whose classes nearly tie.  The
    card's fixture (softmax_case / ovr_case: random weights, logits about 0.3 apart) has no two unplanted values within
    rounding of each other, so there a uniform change moves no choice: on the card relation 13 detects an order that
    differs between tiles or positions through the planted equal classes (the next test, on the real fixture, every dtype
    and both links), and a uniformly changed order is relation 1..12's to find."""
    d, (C, F) = 130, D.PROBE_SHAPES[0]
    c = X.predict_case(d, dtype, C, F, sigmoid)
    W = _near_tied_weights(70, d, c["Cp"], F, c["acc"]).view(F * c["Cp"], d)
    rows = D.gather(c["Z"], c["rows"])
    up, down = D.ascending(rows, W), D.descending(rows, W)
    proba = D.randn(71, (c["n"], F, C), c["acc"]).abs()
    proba[:, 0, 4] = float("nan")
    bias = torch.zeros_like(c["bias"])                                      # no bias between the near-equal logits
    bias[X.NAN_AT], bias[X.NEG_INF_AT] = float("nan"), float("-inf")
    for top_m in X.TOP_M:
        cls = X.expect_top(X.column_values(up, bias, c["state"], C), top_m)
        prob = torch.where(cls < 0, torch.zeros((), dtype=c["acc"]), proba.gather(2, cls.clamp_min(0).long()))
        X.assert_predict(cls, prob, proba, up, bias, c["state"], C, top_m)
        with pytest.raises(AssertionError):
            X.assert_predict(cls, prob, proba, down, bias, c["state"], C, top_m)
        with pytest.raises(AssertionError):                                 # a probability from another column
            X.assert_predict(cls, prob.roll(1, 0), proba, up, bias, c["state"], C, top_m)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
@pytest.mark.parametrize("sigmoid", [False, True], ids=["soft-max", "sigmoid"])
@pytest.mark.parametrize("CF", D.PROBE_SHAPES[1:], ids=str)
def test_relation_13_fails_when_the_order_depends_on_the_tile(dtype, sigmoid, CF):
    """The card's own fixture, Cp = 64.  Dots ascending in the first 16-column tile of every 64 and descending in the
    others: class 17 (and 40) no longer ties with class 1 (3), and the planted twins part or change places."""
    d, (C, F) = 130, CF
    c = X.predict_case(d, dtype, C, F, sigmoid)
    rows, W = D.gather(c["Z"], c["rows"]), c["W"].view(F * c["Cp"], d)
    up, down = D.ascending(rows, W), D.descending(rows, W)
    mixed = torch.where(((torch.arange(W.shape[0]) % 64) < 16)[None, :], up, down)
    cls = X.expect_top(X.column_values(mixed, c["bias"], c["state"], C), 8)
    proba = torch.zeros(c["n"], F, C, dtype=c["acc"])
    with pytest.raises(AssertionError):
        X.assert_predict(cls, torch.zeros(cls.shape, dtype=c["acc"]), proba, up, c["bias"], c["state"], C, 8)


# ---- the sum order of relation 10 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("metric", X.METRICS)
@pytest.mark.parametrize("d", D.DENSE_D)
def test_float64_sums_depend_on_the_documented_order(order, metric, d):
    a = _operand(F64, d)
    dots = ORDERS[order](a, a)
    dist = X.expect_distances(dots, X.expect_norms(dots, metric), metric)
    cells = torch.tensor([b - a_ >= 2 for a_, b in zip(X.SEG, X.SEG[1:])])[None, :].expand(D.ROWS, -1)
    share = float((X.documented_sums(dist) != X.ascending_sums(dist))[cells].float().mean())
    print(f"sum order f64 d={d} {metric} {order}: {share:.3f} of the cells with two or more members differ (required 0.25)")
    assert share >= 0.25


@pytest.mark.parametrize("dtype", X.FLOAT_DTYPES, ids=D.case_id)
@pytest.mark.parametrize("metric", X.METRICS)
@pytest.mark.parametrize("d", D.DENSE_D)
def test_float32_sums_are_exact_in_any_order(dtype, metric, d):
    """Up to 171 float32 distances of one binade or so: their double sum has bits to spare, so these dtypes pin every
    distance but cannot see the order."""
    a = _operand(dtype, d)
    for order in ORDERS.values():
        dots = order(a, a)
        dist = X.expect_distances(dots, X.expect_norms(dots, metric), metric)
        S = X.documented_sums(dist)
        rows = dist.double().tolist()
        for p in range(D.ROWS):
            for c in range(len(X.SEG) - 1):
                assert float(S[p, c]) == math.fsum(rows[p][X.SEG[c]:X.SEG[c + 1]]), (p, c)


# ---- composition of the fixtures -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
@pytest.mark.parametrize("d", D.DENSE_D)
def test_the_table_holds_equal_rows_and_near_duplicates(dtype, d):
    Z = X.dist_table(d, dtype)
    assert Z.dtype == dtype and all(torch.equal(Z[r], Z[5]) for r in D.DUP_ROWS) and D.DUP_ROWS == (5, 133, 290)
    pairs = X.near_pairs()
    assert len(pairs) == X.NEAR + 1 and len({r for p in pairs[:-1] for r in p} | {pairs[-1][1]}) == 2 * X.NEAR + 1
    assert pairs[-1][0] == 5 and not ({r for p in pairs for r in p} - {5}) & set(D.DUP_ROWS)
    unit = {F32: 2.0 ** -23, F64: 2.0 ** -52, BF16: 2.0 ** -7}[dtype]
    chosen = X.clamp_pairs(d, dtype)
    assert len(chosen) == X.CLAMP and len({c[1] for c in chosen}) == X.CLAMP
    assert not {c[1] for c in chosen} & ({r for p in pairs for r in p} | set(D.DUP_ROWS) | {c[0] for c in chosen})
    assert {r for c in chosen for r in c[:2]} <= set(X.positions().tolist())
    for src, dst in pairs + tuple(c[:2] for c in chosen):
        moved = (Z[src] != Z[dst]).nonzero().flatten()
        assert moved.numel() == 1
        x, y = float(Z[src, moved[0]]), float(Z[dst, moved[0]])
        assert unit / 2 <= abs(x - y) / 2.0 ** math.floor(math.log2(abs(x))) <= unit      # one unit in the last place


def test_the_positions_put_ties_and_near_duplicates_inside_and_across_clusters():
    pos = X.positions()
    assert D.ROWS == X.SEG[-1] == pos.numel() and [b - a for a, b in zip(X.SEG, X.SEG[1:])] == [1, 0, 63, 65, 171]
    assert int((pos == -1).sum()) >= 10 and int((pos == D.ROWS + 5).sum()) >= 10
    assert not bool(D.inside(pos[[63, 64, 127, 128]]).any())
    assert [int(pos[p]) for p in (0, 130, 299)] == list(D.DUP_ROWS)
    assert [X.cluster_of(p) for p in (0, 130, 299)] == [0, 4, 4]            # the equal rows: across, and inside one
    assert [X.cluster_of(p) for p in (0, 1, 63, 64, 128, 129, 299)] == [0, 2, 2, 3, 3, 4, 4]
    where = {}
    for p, r in enumerate(pos.tolist()):
        where.setdefault(r, []).append(X.cluster_of(p))
    same = sum(1 for s, t in X.near_pairs() if set(where[s]) & set(where[t]))
    across = sum(1 for s, t in X.near_pairs() if any(u != v for u in where[s] for v in where[t]))
    assert same >= 5 and across >= 5
    for n in (5, 129):
        q = X.positions(n).tolist()
        assert q[0] == 5 and q[-1] == 290 and 133 in q
    assert X.positions(1).tolist() == [290]
    assert {X.knn_tile(kk) for kk in X.KNN_K} == {4, 2, 1}


@pytest.mark.parametrize("dtype", X.FLOAT_DTYPES, ids=D.case_id)
@pytest.mark.parametrize("d", D.DENSE_D)
@pytest.mark.parametrize("mu_kind", X.MU_KINDS)
def test_the_clamp_decides_pairs_and_the_lists_hold_ties(dtype, d, mu_kind):
    a = _operand(dtype, d, mu_kind)
    sq, dots = X.expect_sqnorm(a), D.descending(a, a)
    clamped = X.clamped_pairs(sq, dots)
    print(f"clamp {D.case_id(dtype)} d={d} mu={mu_kind}: {clamped} off-diagonal pairs are negative before the clamp")
    assert clamped >= 1
    Dm = X.expect_sqdist(sq, dots)
    for kk in X.KNN_K:
        assert X.tied_places(X.expect_knn(Dm, kk)[1]) >= 1
    if mu_kind == "zero":
        assert int((sq == 0).sum()) >= 20                                   # the positions outside the table


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.case_id)
@pytest.mark.parametrize("CF", D.PROBE_SHAPES, ids=str)
@pytest.mark.parametrize("sigmoid", [False, True], ids=["soft-max", "sigmoid"])
def test_the_predict_cases_hold_ties_fills_and_closed_columns(dtype, CF, sigmoid):
    (C, F), d = CF, 17
    c = X.predict_case(d, dtype, C, F, sigmoid)
    assert math.isnan(float(c["bias"][X.NAN_AT])) and float(c["bias"][X.NEG_INF_AT]) == float("-inf")
    assert torch.equal(c["W"][:, 2], c["W"][:, 1]) and bool((c["state"][:, [1, 2]] == 0).all())
    if sigmoid:
        assert bool((c["state"][:, :C] == 1).any()) and bool((c["state"][:, :C] == -1).any())
    values = X.column_values(D.ascending(D.gather(c["Z"], c["rows"]), c["W"].view(-1, d)), c["bias"], c["state"], C)
    top = X.expect_top(values, 8)
    assert X.tied_choices(values, top) >= 1
    assert not bool((top[:, 0] == 4).any()) and not bool((top[:, 1] == 5).any())
    assert (C > 7) or bool((top[:, :, 7] == -1).all())
