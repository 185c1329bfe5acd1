"""Float-data cases that hold the distance kernels and probe_predict to the anchor of tests/dense_bits_cases.py --
relations 9..13, helpers of tests/test_gpu_distance_bits.py (the HIP kernels) and tests/test_distance_bits_host.py (the
fixtures' and the expectation functions' self-checks).  The layout is that module's: `expect_*` computes on the CPU, from
dots, what the kernel must return; `assert_*` compares; `check_*(k, dev, ...)` runs the kernel and the anchor.

 9  silhouette_norms   |a|^2 is the diagonal of the anchor; cosine: 1 / sqrt of it, two correctly rounded steps
10  silhouette_sums    every distance from the anchor's dots, summed in double in the order silhouette.h documents
11  tsne_sqdist        sq: the chain of fmaf in ascending k, restated exactly; D: one rounding, the clamp, the mirror
12  knn_sqdist         the k nearest of relation 11's D for the three query tiles and 1 / 3 slabs, ties by position
13  probe_predict      the top-m classes of the anchor's logits, knocked out round by round, and their probabilities

The distance kernels contract a = z - mu with itself, a formed in the accumulate type by the operand loaders.  The
anchor's operand is that a, computed on the CPU (`operand`: one subtraction, one rounding, the loader's own operation),
and it goes through the ACCUMULATE type's instance of project_rows.  For a bf16 table that is the f32 instance, on an
operand the bf16 instance cannot hold: mfma_tile.h promises one order "for every kernel", so the f32 instance's dots are
the bits a bf16 distance kernel must form, and this is intended.

Fixture: 300 positions (dense_bits_cases.row_list: indices outside the table read as z = 0, so a = -mu; both sides of
the 64- and 128-row tile edges; the equal rows 5 = 133 = 290 at positions 0, 130 and 299) into a table that also holds
NEAR + 1 + CLAMP near-duplicates: a row that is another row with ONE element moved by one unit in the last place of the
table's dtype.  For equal and near-duplicate rows sq_i + sq_j - 2 dot is rounding noise (sq is summed in ascending k, the
dot in the contraction's order): which of them the clamp at zero catches is decided by single bits.  NEAR + 1 pairs are
drawn at random; CLAMP are chosen on the CPU among the neighbours that the clamp catches (clamp_pairs), so that every
dtype and d has some at mu = 0 too.
"""
import bisect
import functools

import numpy as np
import torch

from clane_amd import _hip

from .dense_bits_cases import (BF16, DENSE_D, DTYPES, DUP_ROWS, F32, F64, PROBE_SHAPES, ROWS, anchor_dots, case_id,
                               gather, logits_of, ovr_case, place, randn, row_list, slice_order, softmax_case, table)

FLOAT_DTYPES = (F32, BF16)                                 # tsne_sqdist, knn_sqdist: no f64 instance
METRICS = ("euclidean", "cosine")
MU_KINDS = ("zero", "random")
INT_OF = {F32: torch.int32, F64: torch.int64, BF16: torch.int16}
POS_SEED, TABLE_SEED, MU_SEED, NEAR_SEED = 51, 52, 53, 54
NEAR = 20                                                  # near-duplicate pairs, and one more next to the equal rows
CLAMP, CLAMP_ELEMS = 3, 8                                  # chosen near-duplicates: clamp_pairs
SEG = (0, 1, 1, 64, 129, 300)                              # K = 5 clusters of 1, 0, 63, 65 and 171 positions
SUM_RANGES = ((0, 300), (37, 205))                         # [p0, p1) of silhouette_sums
TSNE_N = (1, 129, 300)                                     # 300: the six tile pairs -- diagonal, off-diagonal, partial
KNN_K = (7, 90, 192)                                       # the 128-, 64- and 32-query tile
KNN_SLABS = (1, 3)
TOP_M = (1, 3, 8)                                          # 8 > C = 7: fills
NAN_AT, NEG_INF_AT = (0, 4), (1, 5)                        # (fit, class) of the NaN and the -inf bias


# ---- fixtures: host tensors, seeded, never written to ------------------------------------------------------------------
def positions(n=ROWS):
    return row_list(POS_SEED, n)


def cluster_of(p, seg=SEG):
    return bisect.bisect_right(seg, p) - 1


@functools.lru_cache(maxsize=None)
def near_pairs():
    """NEAR + 1 (source row, copy row) of table rows, all distinct and none an equal row but the last source, which is
    row 5.  The pairs are drawn from two positions of positions(300) that lie, alternately, in one cluster of SEG and in
    two, so the list meets near-duplicates both inside a cluster and across."""
    pos = positions().tolist()
    g = torch.Generator().manual_seed(NEAR_SEED)
    used, pairs = set(DUP_ROWS), []
    while len(pairs) < NEAR:
        pa, pb = torch.randint(0, ROWS, (2,), generator=g).tolist()
        ra, rb = pos[pa], pos[pb]
        if not (0 <= ra < ROWS and 0 <= rb < ROWS) or ra == rb or ra in used or rb in used:
            continue
        if (cluster_of(pa) == cluster_of(pb)) != (len(pairs) % 2 == 0):
            continue
        used |= {ra, rb}
        pairs.append((ra, rb))
    spare = next(r for r in pos[140:] if 0 <= r < ROWS and r not in used)
    return tuple(pairs) + ((DUP_ROWS[0], spare),)


def dots_by_row(a, b, order):
    """[n] dots of a's rows with b's rows, the k terms added one at a time in `order` (dense_bits_cases.cpu_dots' model)."""
    s = torch.zeros(a.shape[0], dtype=a.dtype)
    for kk in order:
        s = s + a[:, kk] * b[:, kk]
    return s


def _planted(Z, dtype, src, dst, elem, step):
    Z[dst] = Z[src]
    Z.view(INT_OF[dtype])[dst, elem] += step


def _with_near_pairs(d, dtype):
    Z = table(TABLE_SEED, d, dtype).clone()
    for i, (src, dst) in enumerate(near_pairs()):
        _planted(Z, dtype, src, dst, (7 * i) % d, 1 if i % 2 == 0 else -1)
    return Z


@functools.lru_cache(maxsize=None)
def clamp_pairs(d, dtype):
    """CLAMP more near-duplicates (source row, copy row, element, +1 / -1 unit), CHOSEN so that the clamp has work at
    mu = 0 whatever the dtype and d: a random one-unit neighbour is clamped only where rounding noise outweighs the tiny
    true distance, which for a bf16 table at d = 5 (16-bit products, five of them) happens for 1 neighbour in 150, so no
    number of random pairs that fits 300 rows reaches it.  Of the listed rows' neighbours in one of their first
    CLAMP_ELEMS elements, these have v = (sq_i + sq_j) - 2 dot < 0 with the dot summed in descending k, and of those in
    the most of the three orders descending / ascending / mfma_slice's -- in the order (rows, element, unit).  The copies
    overwrite listed rows that hold no other plant."""
    Z = _with_near_pairs(d, dtype)
    acc = _hip.acc_dtype(dtype)
    pos = positions().tolist()
    listed = sorted({r for r in pos if 0 <= r < ROWS})
    cands = [(src, e, step) for src in listed for e in range(min(d, CLAMP_ELEMS)) for step in (1, -1)]
    src = torch.tensor([c[0] for c in cands])
    Zc = Z[src].clone()
    bits = Zc.view(INT_OF[dtype])
    for e in range(min(d, CLAMP_ELEMS)):
        for step in (1, -1):
            sel = torch.tensor([c[1] == e and c[2] == step for c in cands])
            bits[sel, e] += step
    a, b = Z[src].to(acc), Zc.to(acc)
    s = expect_sqnorm(a) + expect_sqnorm(b)
    orders = (range(d - 1, -1, -1), range(d), slice_order(d))
    neg = torch.stack([s - 2 * dots_by_row(a, b, o) < 0 for o in orders])
    best = sorted((-int(neg[:, i].sum()), cands[i]) for i in range(len(cands)) if bool(neg[0, i]))[:CLAMP]
    assert len(best) == CLAMP, "too few neighbours that the clamp catches: widen CLAMP_ELEMS"
    taken = {r for p in near_pairs() for r in p} | set(DUP_ROWS) | {c[0] for _, c in best}
    spare = [r for r in listed if r not in taken]
    return tuple((c[0], spare[i], c[1], c[2]) for i, (_, c) in enumerate(best))


@functools.lru_cache(maxsize=None)
def dist_table(d, dtype):
    """dense_bits_cases.table (rows 133 and 290 repeat row 5) with the copies of near_pairs(): element (7 i) % d of pair
    i one unit in the last place further from zero (even i) or nearer (odd i); then the copies of clamp_pairs(d, dtype)."""
    Z = _with_near_pairs(d, dtype)
    for src, dst, elem, step in clamp_pairs(d, dtype):
        _planted(Z, dtype, src, dst, elem, step)
    return Z


def mu_case(d, acc, kind):
    return torch.zeros(d, dtype=acc) if kind == "zero" else randn(MU_SEED, (d,), acc, 0.5)


def operand(Z, idx, mu):
    """a = z - mu in mu's (the accumulate) dtype, z = 0 outside the table: the operand loaders' one subtraction."""
    return gather(Z, idx).to(mu.dtype) - mu[None, :]


_ANCHOR = {}


def anchor_case(k, dev, dtype, d, mu_kind, n=ROWS):
    """(Z, positions, mu, a, dots): the fixture and the anchor's [n, n] dots of a with itself, computed once.  f32 and
    bf16 tables share nothing but the code: their operands differ."""
    key = (dtype, d, mu_kind, n)
    if key not in _ANCHOR:
        acc = _hip.acc_dtype(dtype)
        Z, idx, mu = dist_table(d, dtype), positions(n), mu_case(d, acc, mu_kind)
        a = operand(Z, idx, mu)
        _ANCHOR[key] = (Z, idx, mu, a, anchor_dots(k, a, a, dev))
    return _ANCHOR[key]


def same_bits(x, y):
    """torch.equal on the bit patterns: a NaN equals itself, -0.0 does not equal 0.0."""
    return x.dtype == y.dtype and torch.equal(x.contiguous().view(INT_OF[x.dtype]), y.contiguous().view(INT_OF[y.dtype]))


# ---- correctly rounded steps on the CPU ----------------------------------------------------------------------------------
def two_sum(x, y):
    """(s, e): s = fl(x + y) and x + y = s + e exactly (Knuth)."""
    s = x + y
    yy = s - x
    return s, (x - (s - yy)) + (y - yy)


def two_prod(x, y):
    """(p, e) of float64: p = fl(x y) and x y = p + e exactly (Dekker, Veltkamp's split by 2^27 + 1)."""
    def split(v):
        t = v * 134217729.0
        hi = t - (t - v)
        return hi, v - hi
    p = x * y
    xh, xl = split(x)
    yh, yl = split(y)
    return p, ((xh * yh - p) + xh * yl + xl * yh) + xl * yl


def odd_sum(x, y):
    """x + y of float64 rounded to odd: the exact sum if it is a float64, else its neighbour with the odd last bit."""
    s, e = two_sum(x, y)
    even = (s.contiguous().view(torch.int64) & 1) == 0
    away = torch.where(e > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    return torch.where((e != 0) & even, torch.nextafter(s, away), s)


def fma_acc(x, y, z):
    """fma(x, y, z) of float32 or float64 tensors, ONE rounding.  float32: the product is exact in float64, the sum is
    rounded to odd there and cast once (53 >= 24 + 2, so the cast rounds as if from the exact value).  float64: Boldo and
    Melquiond's emulation -- the exact product (ph, pl), (th, tl) = two_sum(z, ph), th + odd(tl + pl).
    test_distance_bits_host.py holds both to exact rationals."""
    x, y, z = torch.broadcast_tensors(x, y, z)
    if x.dtype == F32:
        return odd_sum(x.double() * y.double(), z.double()).float()
    ph, pl = two_prod(x, y)
    th, tl = two_sum(z, ph)
    return th + odd_sum(tl, pl)


def sqrt_acc(v):
    """The correctly rounded square root: float32 through float64 (53 >= 2 * 24 + 2: the second rounding is innocent).
    numpy's, which is the hardware's: torch.sqrt of float64 on a CPU may be a vector routine that is one unit off."""
    root = torch.from_numpy(np.sqrt(v.double().contiguous().numpy()))
    return root if v.dtype == F64 else root.float()


def recip_acc(v):
    return 1.0 / v if v.dtype == F64 else (1.0 / v.double()).float()


# ---- 9. silhouette_norms ---------------------------------------------------------------------------------------------------
def expect_norms(dots, metric):
    """nrm [n] from the [n, n] dots: the diagonal; cosine: 1 / sqrt(dot) in two correctly rounded steps, 0 for dot <= 0."""
    sq = dots.diagonal().clone()
    if metric == "euclidean":
        return sq
    pos = sq > 0
    r = recip_acc(sqrt_acc(torch.where(pos, sq, torch.ones_like(sq))))
    return torch.where(pos, r, torch.zeros_like(sq))


def assert_norms(nrm, dots, metric):
    want = expect_norms(dots, metric)
    assert torch.equal(nrm, want), ("silhouette_norms", metric, (nrm != want).nonzero().flatten()[:8].tolist())


def run_norms(k, dev, Z, d, idx, mu, metric):
    nrm = torch.full((idx.numel(),), float("nan"), dtype=mu.dtype, device=dev)
    k.silhouette_norms(place(Z, dev), d, idx.to(dev), mu.to(dev), metric, nrm)
    return nrm


def check_norms(k, dev, dtype, d, metric, mu_kind):
    Z, idx, mu, a, dots = anchor_case(k, dev, dtype, d, mu_kind)
    nrm = run_norms(k, dev, Z, d, idx, mu, metric).cpu()
    assert_norms(nrm, dots, metric)
    zero_rows = int((nrm == 0).sum())
    assert (zero_rows >= 10) == (mu_kind == "zero"), "the positions outside the table are the zero rows"


# ---- 10. silhouette_sums ---------------------------------------------------------------------------------------------------
def expect_distances(dots, nrm, metric, fused=False):
    """[n, n] distances in the accumulate dtype as silhouette_sums_kernel forms them; the same POSITION: 0.
    euclidean: sqrt(max(0, fma(-2, dot, sq_i + sq_j))) -- 2 dot is exact, so the fma is the one rounding of s - 2 dot,
    which is this dtype's own subtraction; the square root correctly rounded.
    cosine: max(0, 1 - ((dot r_i) r_j)), the last multiply rounded on its own or (fused) contracted into the subtraction."""
    zero = torch.zeros((), dtype=dots.dtype)
    if metric == "euclidean":
        v = (nrm[:, None] + nrm[None, :]) - 2 * dots
        dist = sqrt_acc(torch.where(v > 0, v, zero))
    else:
        t = dots * nrm[:, None]
        dist = fma_acc(-t, nrm[None, :], torch.ones((), dtype=dots.dtype)) if fused else 1 - t * nrm[None, :]
        dist = torch.where(dist > 0, dist, zero)
    dist.fill_diagonal_(0)
    return dist


def documented_sums(dist, seg=SEG):
    """S [n, K] float64 in the order of silhouette.h's header: the columns of cluster c numbered q = j - seg[c]; partial
    (h, l), h = (q % 128) / 64, l = q % 16, adds its columns in ascending q from 0.0; the 16 partials of one h are folded
    by the xor butterfly over l (masks 8, 4, 2, 1); the result is fold(h = 0) + fold(h = 1)."""
    n, lanes = dist.shape[0], torch.arange(16)
    S = torch.zeros(n, len(seg) - 1, dtype=F64)
    for c in range(len(seg) - 1):
        part = torch.zeros(n, 2, 16, dtype=F64)
        for q, j in enumerate(range(seg[c], seg[c + 1])):
            part[:, (q % 128) // 64, q % 16] += dist[:, j].double()
        for mask in (8, 4, 2, 1):
            part = part + part[:, :, lanes ^ mask]
        S[:, c] = part[:, 0, 0] + part[:, 1, 0]
    return S


def ascending_sums(dist, seg=SEG):
    """The same sums with a cluster's columns added one after the other -- another order, for the host file."""
    S = torch.zeros(dist.shape[0], len(seg) - 1, dtype=F64)
    for c in range(len(seg) - 1):
        for j in range(seg[c], seg[c + 1]):
            S[:, c] = S[:, c] + dist[:, j].double()
    return S


SUM_FORMS = {"euclidean": ("exact",), "cosine": ("separate", "fused")}


def expect_sums(dots, nrm, metric, form, seg=SEG):
    return documented_sums(expect_distances(dots, nrm, metric, fused=form == "fused"), seg)


def assert_sums(S, dots, nrm, metric, p0=0, p1=None, seg=SEG):
    """S [p1 - p0, K] equals rows [p0, p1) of ONE restatement, whole; returns the forms it equals."""
    agree = {}
    for form in SUM_FORMS[metric]:
        want = expect_sums(dots, nrm, metric, form, seg)[p0:p1]
        assert S.shape == want.shape
        agree[form] = int((S == want).sum())
    held = [form for form, cells in agree.items() if cells == S.numel()]
    assert held, ("silhouette_sums", metric, (p0, p1), f"cells equal to each form, of {S.numel()}", agree)
    return held


def run_sums(k, dev, Z, d, idx, mu, nrm, metric, p0, p1, seg=SEG):
    S = torch.full((p1 - p0, len(seg) - 1), float("nan"), dtype=F64, device=dev)
    k.silhouette_sums(place(Z, dev), d, idx.to(dev), torch.tensor(seg, dtype=torch.int64, device=dev), mu.to(dev), nrm,
                      metric, p0, p1, S)
    return S.cpu()


def check_sums(k, dev, dtype, d, metric, mu_kind):
    Z, idx, mu, a, dots = anchor_case(k, dev, dtype, d, mu_kind)
    nrm = run_norms(k, dev, Z, d, idx, mu, metric)
    assert_norms(nrm.cpu(), dots, metric)
    (p0, p1), part_range = SUM_RANGES
    full = run_sums(k, dev, Z, d, idx, mu, nrm, metric, p0, p1)
    held = assert_sums(full, dots, nrm.cpu(), metric)
    print(f"silhouette_sums {case_id(dtype)} d={d} {metric} mu={mu_kind}: equals the form(s) {held}")
    part = run_sums(k, dev, Z, d, idx, mu, nrm, metric, *part_range)
    assert torch.equal(part, full[part_range[0]:part_range[1]]), "S of [37, 205) is not rows 37..204 of S of [0, 300)"
    assert bool((full[:, 1] == 0).all()) and float(full[0, 0]) == 0.0       # the empty cluster; the singleton's own sum
    return held


# ---- 11. tsne_sqdist -------------------------------------------------------------------------------------------------------
def expect_sqnorm(a):
    """sq [n]: s = fmaf(a_k, a_k, s) for k = 0 .. d - 1 from 0, every step one rounding (tsne_sqnorm_kernel)."""
    s = torch.zeros(a.shape[0], dtype=a.dtype)
    for kk in range(a.shape[1]):
        s = fma_acc(a[:, kk], a[:, kk], s)
    return s


def unclamped(sq, dots):
    """v [n, n] = (sq_i + sq_j) - 2 dot in float32: 2 dot is exact, so the subtraction rounds once whether or not the
    compiler contracts it into an fma."""
    return (sq[:, None] + sq[None, :]) - 2 * dots


def clamped_pairs(sq, dots):
    """Off-diagonal (i, j) whose v is negative: the pairs the clamp changes."""
    v = unclamped(sq, dots)
    v.fill_diagonal_(0)
    return int((v < 0).sum())


def expect_sqdist(sq, dots):
    v = unclamped(sq, dots)
    D = torch.where(v > 0, v, torch.zeros((), dtype=v.dtype))
    D.fill_diagonal_(0)
    return D


def assert_sqdist(sq, D, a, dots):
    want_sq = expect_sqnorm(a)
    assert torch.equal(sq, want_sq), ("tsne_sqnorm sq", (sq != want_sq).nonzero().flatten()[:8].tolist())
    want = expect_sqdist(want_sq, dots)
    assert torch.equal(D, want), ("tsne_sqdist D", int((D != want).sum()), (D != want).nonzero()[:4].tolist())
    assert same_bits(D, D.T.contiguous()), "tsne_sqdist: D is not its transpose bit for bit"
    assert same_bits(D.diagonal().contiguous(), torch.zeros(D.shape[0])), "tsne_sqdist: the diagonal"


def run_sqdist(k, dev, Z, d, idx, mu):
    n = idx.numel()
    sq = torch.full((n,), float("nan"), dtype=F32, device=dev)
    D = torch.full((n, n), float("nan"), dtype=F32, device=dev)
    k.tsne_sqdist(place(Z, dev), d, idx.to(dev), mu.to(dev), sq, D)
    return sq.cpu(), D.cpu()


def check_sqdist(k, dev, dtype, d, n, mu_kind):
    Z, idx, mu, a, dots = anchor_case(k, dev, dtype, d, mu_kind, n)
    sq, D = run_sqdist(k, dev, Z, d, idx, mu)
    assert_sqdist(sq, D, a, dots)
    print(f"tsne_sqdist {case_id(dtype)} d={d} n={n} mu={mu_kind}: the anchor clamps {clamped_pairs(sq, dots)} of "
          f"{n * (n - 1)} off-diagonal pairs")


# ---- 12. knn_sqdist --------------------------------------------------------------------------------------------------------
def knn_tile(kk):
    """MI of the query tile (32 MI queries) that tsne_nn.h's knn_tile_mi picks for lists of kk places."""
    return 4 if kk <= 40 else 2 if kk <= 96 else 1


def expect_knn(D, kk):
    """(ids [n, kk] int32, sqdist [n, kk]): per row the kk other positions in the order (distance ascending, position
    ascending); the places past n - 1: -1 / +inf."""
    n = D.shape[0]
    Dm = D.clone()
    Dm.fill_diagonal_(float("inf"))                         # a distance is finite: the row itself sorts last
    order = torch.sort(Dm, dim=1, stable=True).indices      # stable: position order among equals
    take = min(kk, n - 1)
    ids = torch.full((n, kk), -1, dtype=torch.int32)
    sqd = torch.full((n, kk), float("inf"), dtype=D.dtype)
    ids[:, :take] = order[:, :take].to(torch.int32)
    sqd[:, :take] = Dm.gather(1, order[:, :take])
    return ids, sqd


def assert_knn(ids, sqd, D, kk, tag=""):
    want_i, want_d = expect_knn(D, kk)
    assert torch.equal(ids, want_i), ("knn ids", tag, (ids != want_i).any(1).nonzero().flatten()[:8].tolist())
    assert torch.equal(sqd, want_d), ("knn sqdist", tag, int((sqd != want_d).sum()))


def run_knn(k, dev, Z, d, idx, mu, kk, n_slabs):
    n = idx.numel()
    sq = torch.full((n,), float("nan"), dtype=F32, device=dev)
    ids = torch.full((n, kk), -7, dtype=torch.int32, device=dev)
    sqd = torch.full((n, kk), float("nan"), dtype=F32, device=dev)
    ci = cd = None
    if n_slabs > 1:
        ci = torch.full((n * n_slabs * kk,), -7, dtype=torch.int32, device=dev)
        cd = torch.full((n * n_slabs * kk,), float("nan"), dtype=F32, device=dev)
    k.knn_sqdist(place(Z, dev), d, idx.to(dev), mu.to(dev), sq, ids, sqd, n_slabs, ci, cd)
    return sq.cpu(), ids.cpu(), sqd.cpu()


def tied_places(sqd):
    """Places of the lists that hold the distance of the place before them: where only the position decides."""
    return int((torch.isfinite(sqd[:, 1:]) & (sqd[:, 1:] == sqd[:, :-1])).sum())


def check_knn(k, dev, dtype, d, mu_kind, n=ROWS, ks=KNN_K):
    Z, idx, mu, a, dots = anchor_case(k, dev, dtype, d, mu_kind, n)
    want_sq = expect_sqnorm(a)
    D = expect_sqdist(want_sq, dots)
    for kk in ks:
        assert tied_places(expect_knn(D, kk)[1]) >= 1, "no list holds an exact tie: nothing tests the tie rule"
        for n_slabs in KNN_SLABS:
            sq, ids, sqd = run_knn(k, dev, Z, d, idx, mu, kk, n_slabs)
            assert torch.equal(sq, want_sq), ("knn_sqdist sq", kk, n_slabs)
            assert_knn(ids, sqd, D, kk, (kk, n_slabs))
            if kk > n - 1:
                assert bool((ids[:, n - 1:] == -1).all()) and bool(torch.isinf(sqd[:, n - 1:]).all())


# ---- 13. probe_predict -----------------------------------------------------------------------------------------------------
def predict_case(d, dtype, C, F, sigmoid):
    """softmax_case / ovr_case of dense_bits_cases (their weights, biases, planted equal classes and, sigmoid, col_state)
    with a NaN bias in fit 0 and a -inf bias in fit 1, on classes that are no planted twin."""
    c = dict(ovr_case(d, dtype, C, F) if sigmoid else softmax_case(d, dtype, C, F))
    bias = c["bias"].clone()
    bias[NAN_AT], bias[NEG_INF_AT] = float("nan"), float("-inf")
    c["bias"] = bias
    if sigmoid:
        state = c["state"].clone()
        state[NAN_AT], state[NEG_INF_AT] = 0, 0             # fitted columns: their value is the logit
        c["state"] = state
    else:
        c["state"] = torch.zeros(F, c["Cp"], dtype=torch.int8)
    return c


def column_values(dots, bias, state, C):
    """[n, F, C]: a column's value -- acc(dot + bias); a col_state -1 / +1 column -inf / +inf."""
    l = logits_of(dots, bias)[:, :, :C]
    st = state[None, :, :C].expand_as(l)
    inf = torch.full((), float("inf"), dtype=l.dtype)
    return torch.where(st < 0, -inf, torch.where(st > 0, inf, l))


def expect_top(values, top_m):
    """top_class [n, F, top_m] int32: the columns with value > -inf (so never a NaN) by (value descending, class
    ascending); -1 where they run out."""
    n, F, C = values.shape
    is_open = values > float("-inf")
    key = torch.where(is_open, values, torch.full((), float("-inf"), dtype=values.dtype))
    order = torch.sort(key, dim=2, descending=True, stable=True).indices[:, :, :top_m]     # stable: class order among equals
    cls = torch.where(is_open.gather(2, order), order, torch.tensor(-1)).to(torch.int32)
    out = torch.full((n, F, top_m), -1, dtype=torch.int32)
    out[:, :, :cls.shape[2]] = cls
    return out


def assert_predict(top_class, top_prob, proba, dots, bias, state, C, top_m, tag=""):
    want = expect_top(column_values(dots, bias, state, C), top_m)
    bad = (top_class != want).any(2)
    assert torch.equal(top_class, want), ("probe_predict top_class", tag, int(bad.sum()), bad.nonzero()[:4].tolist())
    assert_top_prob(top_class, top_prob, proba, tag)


def assert_top_prob(top_class, top_prob, proba, tag=""):
    """top_prob is proba at the kernel's OWN top_class bit for bit (a NaN included), +0 at a fill: stands on its own."""
    at = top_class.long().clamp(0, proba.shape[2] - 1)
    prob = torch.where(top_class < 0, torch.zeros((), dtype=proba.dtype), proba.gather(2, at))
    assert same_bits(top_prob, prob), ("probe_predict top_prob is not proba at top_class", tag)


def run_predict(k, dev, c, top_m, sigmoid):
    n, F, C, Cp, d = c["n"], c["F"], c["C"], c["Cp"], c["d"]
    cls = torch.full((n, F, top_m), -7, dtype=torch.int32, device=dev)
    pr = torch.full((n, F, top_m), float("nan"), dtype=c["acc"], device=dev)
    full = torch.full((n, F, C), float("nan"), dtype=c["acc"], device=dev)
    k.probe_predict(place(c["Z"], dev), d, c["rows"].to(dev), c["W"].view(F * Cp, d).to(dev), c["bias"].view(-1).to(dev),
                    F, C, cls, pr, proba=full, sigmoid=sigmoid,
                    col_state=c["state"].view(-1).to(dev) if sigmoid else None)
    return cls.cpu(), pr.cpu(), full.cpu()


def tied_choices(values, top_class):
    """Places of the lists whose class has the value of the class before it: an equal class following its twin (or one
    +inf column another), where only the class number decides."""
    taken = top_class >= 0
    v = values.gather(2, top_class.clamp_min(0).long())
    return int((taken[:, :, 1:] & (v[:, :, 1:] == v[:, :, :-1])).sum())


def check_predict(k, dev, dtype, d, C, F, sigmoid):
    """The fixture's unplanted logits lie about 0.3 apart, never within rounding of each other (ascending and descending
    CPU dots give the same lists in every case), so what detects a wrong order HERE are the planted equal classes -- an
    order that differs between two column tiles or positions parts them; a uniformly wrong order is relations 1..12's."""
    c = predict_case(d, dtype, C, F, sigmoid)
    dots = anchor_dots(k, gather(c["Z"], c["rows"]), c["W"].view(F * c["Cp"], d), dev)
    values = column_values(dots, c["bias"], c["state"], C)
    assert tied_choices(values, expect_top(values, max(TOP_M))) >= 1, "no list holds an exact tie"
    for top_m in TOP_M:
        cls, pr, proba = run_predict(k, dev, c, top_m, sigmoid)
        assert_predict(cls, pr, proba, dots, c["bias"], c["state"], C, top_m, (top_m, "sigmoid" if sigmoid else "soft-max"))
        assert not bool((cls[:, NAN_AT[0]] == NAN_AT[1]).any()) and not bool((cls[:, NEG_INF_AT[0]] == NEG_INF_AT[1]).any())
        if top_m > C:                                       # C - 1 open columns at most in fits 0 and 1, C elsewhere
            assert bool((cls[:, :2, C - 1:] == -1).all()) and bool((cls[:, :, C:] == -1).all())
