// Multi-label node classification probe: F one-vs-rest logistic regressions on rows of the embedding table, all at once.
//
// The protocol of DeepWalk and the papers after it (BlogCatalog, Flickr, PPI, Wikipedia POS): a vertex carries a SET of
// classes, one binary logistic regression per class and (train share, split), and a test vertex with k_i true classes is
// given the k_i classes of highest score.  Everything of label_probe.h stays: the stacked weights W_all [K = F * Cp, d],
// the gathered A operand, split [n, ld_split], loss_ws [row tiles, F] followed by probe_loss_reduce_kernel, G [n, K]
// row-major for probe_grad_kernel.  Only the epilogue differs: no log-sum-exp couples a fit's columns; per (row, fit,
// real class column), with l = acc + bias, y = bit c of ymask[row] and e = exp(-|l|):
//
//   loss term  softplus(l) - y l = max(l, 0) + log(1 + e) - y l
//   gradient   G = sigmoid(l) - y,  sigmoid(l) = 1 / (1 + e) for l >= 0, e / (1 + e) for l < 0
//
// both only where the row trains the fit and the column is FITTED (col_state == 0); elsewhere G = 0 and nothing is added
// to the loss.  e <= 1, so neither form overflows at any l.  col_state -1 / +1 marks a column whose class no / every
// training row of the fit has: its weights stay 0 and its prediction value is -inf / +inf in place of l.
//
// Orders (fixed, no atomics): a row's loss terms are summed over the fit's Cp columns in the accumulate type by
// probe_fit_reduce (Cp >= 32: the wave's 16-column tiles pairwise in registers, then the butterflies 8, 4, 2, 1 within a
// tile), THEN converted to double and added per lane over the lane's 16 rows in (mi, reg) order, the four row groups of
// the wave, the two waves of the columns -- label_probe.h's order from there on.  Two calls give the same bits, and a
// fit's G, loss and pred do not depend on where in W_all it stands or on which fits share the call.
//
// Prediction (kOvrWritePred): pred [n, ld_pred] holds one uint64 mask per (row, fit), bit c = class c predicted, written
// by the fit's lane of class 0 after an OR over the fit's lanes.  Threshold: bit c iff the value > 0.  Top-k
// (kOvrPredTopk): max_labels rounds, wave-uniform; in round t every row with popcount(ymask) > t takes the not yet taken
// real column of highest value, ties to the lowest class (one probe_fit_reduce max on the value, one min on the class
// among the equal).  A NaN and a -inf value are never taken (the comparison `value > -inf` is false), so a row can end
// with fewer than popcount(ymask) bits; a row with mask 0 predicts nothing.  The logits never reach memory.
#pragma once

#include "label_probe.h"

namespace clane {

constexpr int kOvrWriteG = 1;          // CLANE_PROBE_WRITE_G
constexpr int kOvrWritePred = 2;       // CLANE_PROBE_WRITE_PRED
constexpr int kOvrPredTopk = 4;        // CLANE_PROBE_PRED_TOPK

template <typename T, typename A>
__global__ __launch_bounds__(kBlock, sizeof(A) == 4 ? 2 : 1) void probe_forward_ovr_kernel(
    const T *__restrict__ Z, int64_t table_rows, int d, int64_t ldz, const int32_t *__restrict__ rows,
    const uint64_t *__restrict__ ymask, int64_t n, const uint8_t *__restrict__ split, int64_t ld_split,
    const A *__restrict__ W, const A *__restrict__ bias, const int8_t *__restrict__ col_state, int F, int C, int cp_log,
    int max_labels, int flags, A *__restrict__ G, double *__restrict__ loss_ws, uint64_t *__restrict__ pred,
    int64_t ld_pred, int n_tiles) {
    using Tile = MfmaTile<A, 4>;
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];
    __shared__ double Ls[kWavesPerBlock][kWave];

    const int Cp = 1 << cp_log, K = F << cp_log;
    const Tile t(threadIdx.x);
    const int64_t tile = blockIdx.x;
    const int n0 = int(tile % n_tiles) * Tile::BN;
    const int64_t row_tile = tile / n_tiles, m0 = row_tile * Tile::BM;

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
    int state[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) state[ni] = pc.real[ni] ? int(col_state[n0 + t.col(ni)]) : 0;
    double lsum[4] = {0.0, 0.0, 0.0, 0.0};
    auto op_max = [](A u, A v) { return u > v ? u : v; };
    auto op_add = [](A u, A v) { return u + v; };
    auto op_min = [](int u, int v) { return u < v ? u : v; };
    auto op_or = [](int u, int v) { return u | v; };
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t r = m0 + t.row(mi, reg);
            const bool in_n = r < n;
            const uint64_t ym = in_n ? ymask[r] : uint64_t(0);
            A l[4], term[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                l[ni] = acc[mi][ni][reg] + pc.bcol[ni];
                term[ni] = A(0);
                const bool live = in_n && pc.real[ni] && state[ni] == 0 && split[r * ld_split + pc.fit[ni]] != 0;
                A gv = A(0);
                if (live) {
                    const A yv = ((ym >> pc.cls[ni]) & 1) ? A(1) : A(0);
                    const A e = exp_acc<A>(l[ni] < A(0) ? l[ni] : -l[ni]);
                    const A den = A(1) + e;
                    term[ni] = (l[ni] > A(0) ? l[ni] : A(0)) + log_acc<A>(den) - yv * l[ni];
                    gv = (l[ni] >= A(0) ? A(1) / den : e / den) - yv;
                }
                if ((flags & kOvrWriteG) && in_n && pc.in_k[ni]) G[r * int64_t(K) + (n0 + t.col(ni))] = gv;
            }
            probe_fit_reduce(term, Cp, op_add);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) lsum[ni] += double(term[ni]);
        }

    if (flags & kOvrWritePred) {                                          // uniform over the launch
        // bit (4 mi + reg) * 4 + ni of `open`: the lane's column ni of its row (mi, reg) can still be taken; of `sel`: it
        // is predicted.  The rounds are the outer loop, so every index into the accumulators stays a constant.
        auto value = [&](int mi, int reg, int ni) -> A {
            return state[ni] == 0 ? A(acc[mi][ni][reg] + pc.bcol[ni]) : (state[ni] < 0 ? neg_inf : pos_inf);
        };
        uint64_t open = 0, sel = 0;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const uint64_t bit = uint64_t(1) << ((4 * mi + reg) * 4 + ni);
                    const A v = value(mi, reg, ni);
                    if (flags & kOvrPredTopk) {
                        if (pc.real[ni] && v > neg_inf) open |= bit;         // NaN, -inf: never taken
                    } else {
                        if (pc.real[ni] && v > A(0)) sel |= bit;
                    }
                }
        if (flags & kOvrPredTopk)
            for (int round = 0; round < max_labels; ++round) {
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int64_t r = m0 + t.row(mi, reg);
                        const bool takes = r < n && __popcll(ymask[r]) > round;
                        A v[4], mx[4];
                        int am[4];
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni) {
                            v[ni] = value(mi, reg, ni);
                            mx[ni] = ((open >> ((4 * mi + reg) * 4 + ni)) & 1) ? v[ni] : neg_inf;
                        }
                        probe_fit_reduce(mx, Cp, op_max);
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni)
                            am[ni] = (((open >> ((4 * mi + reg) * 4 + ni)) & 1) && v[ni] == mx[ni]) ? pc.cls[ni] : INT_MAX;
                        probe_fit_reduce(am, Cp, op_min);                 // ties: the lowest class
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni) {
                            const uint64_t bit = uint64_t(1) << ((4 * mi + reg) * 4 + ni);
                            if (takes && (open & bit) && am[ni] == pc.cls[ni]) {
                                sel |= bit;
                                open &= ~bit;
                            }
                        }
                    }
            }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t r = m0 + t.row(mi, reg);
                int lo[4], hi[4];
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const uint64_t m = ((sel >> ((4 * mi + reg) * 4 + ni)) & 1) ? uint64_t(1) << pc.cls[ni] : uint64_t(0);
                    lo[ni] = int(uint32_t(m));
                    hi[ni] = int(uint32_t(m >> 32));
                }
                probe_fit_reduce(lo, Cp, op_or);
                probe_fit_reduce(hi, Cp, op_or);
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    if (r < n && pc.in_k[ni] && pc.cls[ni] == 0)
                        pred[r * ld_pred + pc.fit[ni]] = (uint64_t(uint32_t(hi[ni])) << 32) | uint64_t(uint32_t(lo[ni]));
            }
    }
    probe_tile_loss(t, lsum, Ls, n0, K, F, cp_log, row_tile, loss_ws);
}

}  // namespace clane
