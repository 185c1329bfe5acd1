// Applying fitted probes: class probabilities and the top-m classes of rows of a table under F stacked models, all at once.
//
// label_probe.h and multilabel_probe.h fit the stacked weights W_all [K = F * Cp, d] and keep a score; this kernel is the
// other half of a classifier -- given weights, say what a row is and how sure the model is.  It is one more instance of
// the shared tile contraction with the probes' operand loaders (rows of any table gathered through `rows`, an index
// outside [0, table_rows) a zero row) and no y, no split and no loss.  In the accumulators, per (row, fit), with
// l = acc + bias:
//
//   soft-max  p_c = exp(l_c - max) / sum exp(l - max) over the fit's C real columns (pad columns count as -inf), by the
//             probe_fit_reduce butterflies, exp_acc and the order of operations of probe_forward_kernel: p_c - [c == y]
//             is bit for bit what that kernel writes into G for a training row.  A column's VALUE is l_c.
//   sigmoid   (kPredictSigmoid, one-vs-rest models) p_c = 1 / (1 + e) for l >= 0, e / (1 + e) for l < 0, e = exp(-|l|),
//             per column -- probe_forward_ovr_kernel's form; a column of col_state -1 / +1 has value -inf / +inf and
//             p = 0 / 1, a fitted column value l_c.
//
// Selection: top_m rounds of a (value, class) arg-max over the fit's lanes -- one probe_fit_reduce max on the value among
// the columns still open, one min on the class among the equal (ties: the lowest class) -- knocking out each winner.  A
// column is open at the start iff it is real and `value > -inf`, so a NaN and a -inf value are never chosen.  The winner's
// lane writes top_class [n, F, top_m] (int32) and top_prob [n, F, top_m] (accumulate type), best first; a round without
// an open column writes -1 and 0 from the fit's lane of class 0.  kPredictWriteProba: proba [n, F, C] holds every real
// class's probability.  The logits never reach memory.
//
// Orders are fixed and there are no atomics: two calls give the same bits, and a fit's outputs do not depend on where in
// W_all it stands or on which fits share the call.
#pragma once

#include "label_probe.h"

namespace clane {

constexpr int kPredictSigmoid = 1;      // CLANE_PREDICT_SIGMOID
constexpr int kPredictWriteProba = 2;   // CLANE_PREDICT_WRITE_PROBA
constexpr int kPredictMaxTop = 8;       // CLANE_PREDICT_MAX_TOP

template <int I>
struct PredictIndex {
    static constexpr int value = I;
};

template <typename T, typename A>
__global__ __launch_bounds__(kBlock, sizeof(A) == 4 ? 2 : 1) void probe_predict_kernel(
    const T *__restrict__ Z, int64_t table_rows, int d, int64_t ldz, const int32_t *__restrict__ rows, int64_t n,
    const A *__restrict__ W, const A *__restrict__ bias, const int8_t *__restrict__ col_state, int F, int C, int cp_log,
    int top_m, int flags, int32_t *__restrict__ top_class, A *__restrict__ top_prob, A *__restrict__ proba,
    int n_tiles) {
    using Tile = MfmaTile<A, 4>;
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];

    const int Cp = 1 << cp_log, K = F << cp_log;
    const Tile t(threadIdx.x);
    const int64_t tile = blockIdx.x;
    const int n0 = int(tile % n_tiles) * Tile::BN;
    const int64_t m0 = (tile / n_tiles) * Tile::BM;

    // ---- the logits, as in probe_forward_kernel --------------------------------------------------------------------
    int64_t roff[Tile::PER_A];                            // gathered rows of this thread's staging slots; < 0: none
    mfma_gather_offsets(rows, m0, n, table_rows, ldz, roff);

    typename Tile::acc4 acc[4][4];
    mfma_zero<A>(acc);
    mfma_tile_product(
        t, As, Bs, d, acc,
        [&](int s, int, int k) { return (k < d && roff[s] >= 0) ? A(Elem<T>::to_acc(Z[roff[s] + k])) : A(0); },
        [&](int, int i, int k) {
            const int j = n0 + i;
            return (k < d && j < K) ? W[int64_t(j) * d + k] : A(0);
        });

    // ---- epilogue: a lane holds column n0 + wn + 16 ni + li of 16 rows; the 16 lanes of one g share a row ----------
    const A neg_inf = -__builtin_huge_val(), pos_inf = __builtin_huge_val();
    const ProbeCols<A> pc(t, n0, K, C, cp_log, bias);
    const bool sigmoid = (flags & kPredictSigmoid) != 0;                  // uniform over the launch
    int state[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) state[ni] = (sigmoid && pc.real[ni]) ? int(col_state[n0 + t.col(ni)]) : 0;
    auto op_max = [](A u, A v) { return u > v ? u : v; };
    auto op_add = [](A u, A v) { return u + v; };
    auto op_min = [](int u, int v) { return u < v ? u : v; };
    // Per row (mi, reg) of the lane: the probabilities, then the rounds.  Every lane of the wave runs every round.  The
    // row indices are template constants (PredictIndex), not `#pragma unroll` loops: hipcc of ROCm 7.2 at -O3 left such loops
    // rolled around the run-time rounds' loop and indexed the accumulators in scratch (272 bytes per lane in
    // -Rpass-analysis=kernel-resource-usage; 0 as written).  A plain unrolled loop may return once that report shows 0.
    auto row_body = [&](auto MI, auto REG) {
        constexpr int mi = decltype(MI)::value, reg = decltype(REG)::value;
        const int64_t r = m0 + t.row(mi, reg);
        const bool in_n = r < n;
        A l[4], p[4], val[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) l[ni] = acc[mi][ni][reg] + pc.bcol[ni];
        if (sigmoid) {
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const A e = exp_acc<A>(l[ni] < A(0) ? l[ni] : -l[ni]);
                const A den = A(1) + e;
                const A s = l[ni] >= A(0) ? A(1) / den : e / den;
                p[ni] = state[ni] == 0 ? s : (state[ni] < 0 ? A(0) : A(1));
                val[ni] = state[ni] == 0 ? l[ni] : (state[ni] < 0 ? neg_inf : pos_inf);
            }
        } else {
            A mx[4], e[4], se[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) mx[ni] = pc.real[ni] ? l[ni] : neg_inf;
            probe_fit_reduce(mx, Cp, op_max);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                e[ni] = pc.real[ni] ? exp_acc<A>(l[ni] - mx[ni]) : A(0);
                se[ni] = e[ni];
            }
            probe_fit_reduce(se, Cp, op_add);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                p[ni] = e[ni] / se[ni];
                val[ni] = l[ni];
            }
        }
        bool open[4];                                                     // the lane's column ni can still be taken
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            open[ni] = pc.real[ni] && val[ni] > neg_inf;                  // NaN, -inf: never taken
            if ((flags & kPredictWriteProba) && in_n && pc.real[ni]) proba[(r * F + pc.fit[ni]) * C + pc.cls[ni]] = p[ni];
        }
        for (int round = 0; round < top_m; ++round) {
            A mx[4];
            int am[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) mx[ni] = open[ni] ? val[ni] : neg_inf;
            probe_fit_reduce(mx, Cp, op_max);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) am[ni] = (open[ni] && val[ni] == mx[ni]) ? pc.cls[ni] : INT_MAX;
            probe_fit_reduce(am, Cp, op_min);                             // ties: the lowest class
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const bool wins = open[ni] && am[ni] == pc.cls[ni];
                const bool fills = am[ni] == INT_MAX && pc.cls[ni] == 0;
                if (wins) open[ni] = false;
                if (in_n && pc.in_k[ni] && (wins || fills)) {
                    const int64_t o = (r * F + pc.fit[ni]) * top_m + round;
                    top_class[o] = wins ? pc.cls[ni] : -1;
                    top_prob[o] = wins ? p[ni] : A(0);
                }
            }
        }
    };
    auto rows_of = [&](auto MI) {
        row_body(MI, PredictIndex<0>{});
        row_body(MI, PredictIndex<1>{});
        row_body(MI, PredictIndex<2>{});
        row_body(MI, PredictIndex<3>{});
    };
    rows_of(PredictIndex<0>{});
    rows_of(PredictIndex<1>{});
    rows_of(PredictIndex<2>{});
    rows_of(PredictIndex<3>{});
}

}  // namespace clane
