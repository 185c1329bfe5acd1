// Diagonal-covariance Gaussian mixtures by EM on rows of the embedding table, R restarts at once.
//
// The rows are centred by `mean` [d] (accumulate type) in the operand loaders, as tsne.h and content_pca.h centre:
// xc = A(x) - mean.  A row index outside [0, table_rows) is a zero row of the table, centred like any row.  Both steps
// contract the same 2 d wide operand phi(x) = [xc^2 | xc]: element k < d is xc_k^2, element d <= k < 2 d is xc_{k-d}.
//
//   mixture_estep : l = phi(Z[rows]) . Wm^T + cst on the matrix cores, Wm [R * Kp, 2 d] = [-a/2 | mu a] per component,
//                   Kp = K rounded up to a power of two (label_probe.h's stacking: restart r's component c in row
//                   r * Kp + c).  In the accumulators, per (row, restart): the log-sum-exp over the K real components
//                   (pad components count as -inf), the responsibilities exp(l - lse) and the arg-max.  The logits
//                   never reach memory.  ll[r] = sum_i lse_i in double, per row tile and then over the tiles in order.
//   mixture_mstep : S [R * Kp, 2 d] = resp^T . phi(Z[rows]) and nk [R * Kp] = the column sums of resp: probe_grad's
//                   scheme -- chunks of kGradChunk rows, the chunks' partial tiles summed in chunk order.
//
// Every sum runs in a fixed order (no atomics): two calls give the same bits, and what a restart gets does not depend on
// where in Wm it stands or on which other restarts share the call.
#pragma once

#include "label_probe.h"

namespace clane {

constexpr int kMixtureWriteResp = 1;     // CLANE_MIXTURE_WRITE_RESP
constexpr int kMixtureWriteAssign = 2;   // CLANE_MIXTURE_WRITE_ASSIGN

// Element k of phi(x) from the table's element x = x_{k mod d}: the centring is one rounding, the square a second.
template <typename A>
__device__ __forceinline__ A mixture_feature(A x, A mu, bool square) {
    const A xc = x - mu;
    return square ? xc * xc : xc;
}

// ---- E-step ------------------------------------------------------------------------------------------------------
// probe_forward_kernel's launch shape: block b is column tile b % n_tiles of row tile b / n_tiles; ll_ws [row tiles, R].
// resp is [n, R * Kp] contiguous (pad columns 0), assign [n, >= R] with leading dimension ld_assign.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void mixture_estep_kernel(
    const T *__restrict__ Z, int64_t table_rows, int d, int64_t ldz, const int32_t *__restrict__ rows, int64_t n,
    const A *__restrict__ mean, const A *__restrict__ Wm, const A *__restrict__ cst, int R, int C, int cp_log, int flags,
    A *__restrict__ resp, double *__restrict__ ll_ws, int32_t *__restrict__ assign, int64_t ld_assign, int n_tiles) {
    using Tile = MfmaTile<A, 4>;
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];
    __shared__ double Ls[kWavesPerBlock][kWave];

    const int Cp = 1 << cp_log, K = R << cp_log, d2 = 2 * d;
    const Tile t(threadIdx.x);
    const int64_t tile = blockIdx.x;
    const int n0 = int(tile % n_tiles) * Tile::BN;
    const int64_t row_tile = tile / n_tiles, m0 = row_tile * Tile::BM;

    int64_t roff[Tile::PER_A];                               // < 0: a zero row (rows past the list are never written)
    mfma_gather_offsets(rows, m0, n, table_rows, ldz, roff);

    typename Tile::acc4 acc[4][4];
    mfma_zero<A>(acc);
    mfma_tile_product(
        t, As, Bs, d2, acc,
        [&](int s, int, int k) {
            if (k >= d2) return A(0);
            const int j = k < d ? k : k - d;
            const A x = roff[s] >= 0 ? A(Elem<T>::to_acc(Z[roff[s] + j])) : A(0);
            return mixture_feature<A>(x, mean[j], k < d);
        },
        [&](int, int i, int k) {
            const int j = n0 + i;
            return (k < d2 && j < K) ? Wm[int64_t(j) * d2 + k] : A(0);
        });

    // ---- epilogue: label_probe.h's -- a lane holds column n0 + wn + 16 ni + li of 16 rows ---------------------------
    const A neg_inf = -__builtin_huge_val();
    const ProbeCols<A> pc(t, n0, K, C, cp_log, cst);
    double lsum[4] = {0.0, 0.0, 0.0, 0.0};
    auto op_max = [](A u, A v) { return u > v ? u : v; };
    auto op_add = [](A u, A v) { return u + v; };
    auto op_min = [](int u, int v) { return u < v ? u : v; };
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t r = m0 + t.row(mi, reg);
            const bool in_n = r < n;
            A l[4], mx[4], e[4], se[4];
            int am[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                l[ni] = acc[mi][ni][reg] + pc.bcol[ni];
                mx[ni] = pc.real[ni] ? l[ni] : neg_inf;
            }
            probe_fit_reduce(mx, Cp, op_max);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                e[ni] = pc.real[ni] ? exp_acc<A>(l[ni] - mx[ni]) : A(0);
                se[ni] = e[ni];
                am[ni] = (pc.real[ni] && l[ni] == mx[ni]) ? pc.cls[ni] : INT_MAX;      // ties: the lowest component
            }
            probe_fit_reduce(se, Cp, op_add);
            probe_fit_reduce(am, Cp, op_min);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                if (!(in_n && pc.in_k[ni])) continue;
                const int col = n0 + t.col(ni);
                if (flags & kMixtureWriteResp) resp[r * int64_t(K) + col] = pc.real[ni] ? e[ni] / se[ni] : A(0);
                lsum[ni] += double(mx[ni] + log_acc<A>(se[ni]));
                if ((flags & kMixtureWriteAssign) && pc.cls[ni] == 0) assign[r * ld_assign + pc.fit[ni]] = am[ni];
            }
        }
    probe_tile_loss(t, lsum, Ls, n0, K, R, cp_log, row_tile, ll_ws);
}

// ---- M-step ------------------------------------------------------------------------------------------------------
// probe_grad_kernel with phi in the B operand: blockIdx = (tile of S: K tiles x 2 d tiles, chunk).  The partials of
// chunk z go to ws + z * K * (2 d + 1): [K, 2 d] of S, then [K] of nk (summed by the workgroups of the first column
// tile as probe_grad sums db).
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void mixture_mstep_kernel(const T *__restrict__ Z, int64_t table_rows, int d,
                                                               int64_t ldz, const int32_t *__restrict__ rows, int64_t n,
                                                               const A *__restrict__ mean, const A *__restrict__ resp,
                                                               int K, A *__restrict__ ws, int n_tiles) {
    using Tile = MfmaTile<A, 4>;
    constexpr int BM = Tile::BM, KS = Tile::KS;
    static_assert(kGradChunk % Tile::BK == 0, "a chunk is whole slices");
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];
    __shared__ A Db[KS][BM];

    const Tile t(threadIdx.x);
    const int d2 = 2 * d;
    const int o0 = int(blockIdx.x / n_tiles) * Tile::BM, i0 = int(blockIdx.x % n_tiles) * Tile::BN;
    const int64_t kbeg = int64_t(blockIdx.y) * kGradChunk;
    const int64_t kend = kbeg + kGradChunk < n ? kbeg + kGradChunk : n;

    const int so = int(threadIdx.x) % BM, sk = int(threadIdx.x) / BM;     // the staged row / column, the k lane
    const bool o_ok = o0 + so < K, i_ok = i0 + so < d2;
    const int feat = i0 + so, j = feat < d ? feat : feat - d;             // this thread's element of phi
    const A mu = i_ok ? mean[j] : A(0);

    typename Tile::acc4 acc[4][4];
    mfma_zero<A>(acc);
    A dbs = A(0);
    mfma_tile_product_transposed(
        t, As, Bs, kbeg, kend, acc,
        [&](int64_t k, A &a, A &b) {
            int64_t r = rows[k];
            if (r >= table_rows) r = -1;
            if (o_ok) a = resp[k * K + o0 + so];
            if (i_ok) b = mixture_feature<A>(r >= 0 ? A(Elem<T>::to_acc(Z[r * ldz + j])) : A(0), mu, feat < d);
        },
        [&](A a) { dbs += a; });

    A *__restrict__ out = ws + int64_t(blockIdx.y) * K * (int64_t(d2) + 1);
    mfma_for_each(t, acc, [&](int r, int c, A v) {
        const int o = o0 + r, i = i0 + c;
        if (o < K && i < d2) out[int64_t(o) * d2 + i] = v;
    });
    if (i0 == 0) {                                        // uniform over the workgroup
        Db[sk][so] = dbs;
        __syncthreads();
        if (sk == 0 && o_ok) {
            A s = Db[0][so];
#pragma unroll
            for (int q = 1; q < KS; ++q) s += Db[q][so];
            out[int64_t(K) * d2 + o0 + so] = s;
        }
    }
}

}  // namespace clane
