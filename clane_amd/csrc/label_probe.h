// Node classification probe: F multi-class logistic regressions on rows of the embedding table, all at once.
//
// Reference being replaced: the experiment of the reference's README (README.md:51-73) -- a logistic regression on Z per
// (train share, random split), 90 independent fits, each reading Z again.  The fits differ only in which rows train
// them, so their weights are stacked: W_all [K, d] with K = F * Cp, fit f's class c in row f * Cp + c, Cp = C rounded up
// to a power of two (a fit's classes never straddle a 16-column MFMA tile, a wave's 64 columns or a 128-column
// workgroup tile).  One pass over the labelled rows is then
//
//   probe_forward : logits = Z[rows] . W_all^T + b_all on the matrix cores; in the accumulators, per (row, fit): the
//                   log-sum-exp over the fit's C real columns (pad columns count as -inf), the soft-max gradient
//                   G = split * (p - onehot(y)), the loss split * (lse - logit[y]) and the arg-max.  The logits never
//                   reach memory.
//   probe_grad    : dW_all = G^T . Z[rows] and db_all = sum_i G[i, :], an MFMA contraction over the rows in chunks of
//                   kGradChunk, the chunks' partial tiles summed in chunk order.
//
// Every sum runs in a fixed order (no atomics): two calls give the same bits, and what a fit gets does not depend on
// where in W_all it stands or on which other fits share the call.
//
// Table rows outside [0, table_rows) are read as zero rows -- an index never leaves the table.
#pragma once

#include <climits>

#include "device_utils.h"
#include "mfma_tile.h"
#include "pair_train.h"

namespace clane {

constexpr int kProbeMaxClasses = 64;   // Cp <= a wave's 64 columns: the log-sum-exp needs no LDS crossbar
constexpr int kProbeWriteG = 1;        // CLANE_PROBE_WRITE_G
constexpr int kProbeWritePred = 2;     // CLANE_PROBE_WRITE_PRED

__host__ __device__ __forceinline__ int probe_cp_log(int C) {
    int l = 0;
    while ((1 << l) < C) ++l;
    return l;
}

// Reduction of v[ni] (the wave's four 16-column tiles of one row) over every fit's Cp columns: Cp >= 32 first combines
// the tiles in registers, then the 16 (or Cp < 16: Cp) lanes of a tile reduce by butterflies.  Every lane of a fit ends
// with the same bits.  `op` must be commutative.  All 64 lanes take part.
template <typename V, typename Op>
__device__ __forceinline__ void probe_fit_reduce(V (&v)[4], int Cp, Op op) {
    if (Cp >= 32) {
        V a = op(v[0], v[1]), b = op(v[2], v[3]);
        if (Cp >= 64) {
            a = op(a, b);
            b = a;
        }
        v[0] = v[1] = a;
        v[2] = v[3] = b;
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        if (Cp >= 16) v[ni] = op(v[ni], lane_xor<8>(v[ni]));
        if (Cp >= 8) v[ni] = op(v[ni], lane_xor<4>(v[ni]));
        if (Cp >= 4) v[ni] = op(v[ni], lane_xor<2>(v[ni]));
        if (Cp >= 2) v[ni] = op(v[ni], lane_xor<1>(v[ni]));
    }
}

// What a lane knows about its four columns n0 + wn + 16 ni + li of W_all: the fit, the class within the fit, whether the
// column exists (col < K) and is a real class of its fit (not padding up to Cp), and its bias.
template <typename A>
struct ProbeCols {
    int fit[4], cls[4];
    bool in_k[4], real[4];
    A bcol[4];
    __device__ __forceinline__ ProbeCols(const MfmaTile<A, 4> &t, int n0, int K, int C, int cp_log,
                                         const A *__restrict__ bias) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int col = n0 + t.col(ni);
            fit[ni] = col >> cp_log;
            cls[ni] = col & ((1 << cp_log) - 1);
            in_k[ni] = col < K;
            real[ni] = in_k[ni] && cls[ni] < C;
            bcol[ni] = in_k[ni] ? bias[col] : A(0);
        }
    }
};

// The tile's loss per fit from lsum[ni], a lane's sum over its 16 rows in (mi, reg) order: the four row groups of the
// wave, then the two waves that share the columns.  loss_ws [row tiles, F].  Every thread of the workgroup calls it.
template <typename A>
__device__ __forceinline__ void probe_tile_loss(const MfmaTile<A, 4> &t, const double (&lsum)[4],
                                                double (&Ls)[kWavesPerBlock][kWave], int n0, int K, int F, int cp_log,
                                                int64_t row_tile, double *__restrict__ loss_ws) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        double v = lsum[ni];
        v += lane_xor<16>(v);
        v += lane_xor<32>(v);
        if (t.g == 0) Ls[tid / kWave][16 * ni + t.li] = v;
    }
    __syncthreads();
    if (tid < kProjBN) {
        const int col = n0 + tid, q = tid / 64, within = tid % 64;
        if (col < K && (col & ((1 << cp_log) - 1)) == 0)
            loss_ws[row_tile * F + (col >> cp_log)] = Ls[2 * q][within] + Ls[2 * q + 1][within];
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------
// mfma_tile_product (mfma_tile.h) with the rows of the A operand taken through `rows` and n_out = K.  Block b: column
// tile b % n_tiles of row tile b / n_tiles.  loss_ws
// [row tiles, F]: the tile's sum of split * (lse - logit[y]) per fit, in double.  split is [n, >= F] with leading
// dimension ld_split, pred [n, >= F] with ld_pred: a caller that fits in groups hands in a column slice of each.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void probe_forward_kernel(
    const T *__restrict__ Z, int64_t table_rows, int d, int64_t ldz, const int32_t *__restrict__ rows,
    const int32_t *__restrict__ y, int64_t n, const uint8_t *__restrict__ split, int64_t ld_split,
    const A *__restrict__ W, const A *__restrict__ bias, int F, int C, int cp_log, int flags, A *__restrict__ G,
    double *__restrict__ loss_ws, int32_t *__restrict__ pred, int64_t ld_pred, int n_tiles) {
    using Tile = MfmaTile<A, 4>;
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];
    __shared__ double Ls[kWavesPerBlock][kWave];

    const int Cp = 1 << cp_log, K = F << cp_log;
    const Tile t(threadIdx.x);
    const int64_t tile = blockIdx.x;
    const int n0 = int(tile % n_tiles) * Tile::BN;
    const int64_t row_tile = tile / n_tiles, m0 = row_tile * Tile::BM;

    int64_t roff[Tile::PER_A];                               // gathered rows of this thread's staging slots; < 0: none
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
    const A neg_inf = -__builtin_huge_val();
    const ProbeCols<A> pc(t, n0, K, C, cp_log, bias);
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
            const int yr = in_n ? y[r] : -1;
            A l[4], mx[4], e[4], se[4], ly[4];
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
                ly[ni] = (pc.real[ni] && pc.cls[ni] == yr) ? l[ni] : A(0);
                am[ni] = (pc.real[ni] && l[ni] == mx[ni]) ? pc.cls[ni] : INT_MAX;      // ties: the lowest class
            }
            probe_fit_reduce(se, Cp, op_add);
            probe_fit_reduce(ly, Cp, op_add);
            probe_fit_reduce(am, Cp, op_min);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                if (!(in_n && pc.in_k[ni])) continue;
                const int col = n0 + t.col(ni);
                const bool trains = split[r * ld_split + pc.fit[ni]] != 0;
                if (flags & kProbeWriteG) {
                    A gv = A(0);
                    if (trains && pc.real[ni]) gv = e[ni] / se[ni] - (pc.cls[ni] == yr ? A(1) : A(0));
                    G[r * int64_t(K) + col] = gv;
                }
                if (trains) lsum[ni] += double(mx[ni] + log_acc<A>(se[ni]) - ly[ni]);
                if ((flags & kProbeWritePred) && pc.cls[ni] == 0) pred[r * ld_pred + pc.fit[ni]] = am[ni];
            }
        }
    probe_tile_loss(t, lsum, Ls, n0, K, F, cp_log, row_tile, loss_ws);
}

// loss[f] = the sum over the row tiles, in tile order within a thread's slice and the slices in a fixed order.
__global__ __launch_bounds__(kBlock) void probe_loss_reduce_kernel(const double *__restrict__ loss_ws, int64_t row_tiles,
                                                                   int F, double *__restrict__ loss) {
    __shared__ double smem[kBlock];
    const int f = blockIdx.x;
    const int64_t per = ceil_div(row_tiles, kBlock);
    const int64_t a = per * threadIdx.x, b = a + per < row_tiles ? a + per : row_tiles;
    double s = 0.0;
    for (int64_t t = a; t < b; ++t) s += loss_ws[t * F + f];
    smem[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int t = 0; t < kBlock; ++t) total += smem[t];
        loss[f] = total;
    }
}

// ---- backward --------------------------------------------------------------------------------------------------
// Partial dW of one chunk of rows: out[o, c] = sum_i G[i, o] Z[rows[i], c] -- pair_grad_kernel's scheme (the A operand
// is G^T, the B operand the gathered rows of Z, mfma_tile_product_transposed).  blockIdx = (tile of dW: K tiles x d
// tiles, chunk).  The
// workgroups of the first d tile also sum their G columns: a thread adds what it stages, in row order, and the two
// threads of a column are added at the end -- db's partial.  The partials of chunk z go to ws + z * K * (d + 1):
// [K, d] of dW, then [K] of db.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void probe_grad_kernel(const T *__restrict__ Z, int64_t table_rows, int d,
                                                            int64_t ldz, const int32_t *__restrict__ rows, int64_t n,
                                                            const A *__restrict__ G, int K, A *__restrict__ ws,
                                                            int n_tiles) {
    using Tile = MfmaTile<A, 4>;
    constexpr int BM = Tile::BM, KS = Tile::KS;
    static_assert(kGradChunk % Tile::BK == 0, "a chunk is whole slices");
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];
    __shared__ A Db[KS][BM];

    const Tile t(threadIdx.x);
    const int o0 = int(blockIdx.x / n_tiles) * Tile::BM, i0 = int(blockIdx.x % n_tiles) * Tile::BN;
    const int64_t kbeg = int64_t(blockIdx.y) * kGradChunk;
    const int64_t kend = kbeg + kGradChunk < n ? kbeg + kGradChunk : n;

    const int so = int(threadIdx.x) % BM, sk = int(threadIdx.x) / BM;     // the staged row / column, the k lane
    const bool o_ok = o0 + so < K, i_ok = i0 + so < d;

    typename Tile::acc4 acc[4][4];
    mfma_zero<A>(acc);
    A dbs = A(0);
    mfma_tile_product_transposed(
        t, As, Bs, kbeg, kend, acc,
        [&](int64_t k, A &a, A &b) {
            int64_t r = rows[k];
            if (r >= table_rows) r = -1;
            if (o_ok) a = G[k * K + o0 + so];
            if (i_ok && r >= 0) b = A(Elem<T>::to_acc(Z[r * ldz + i0 + so]));
        },
        [&](A a) { dbs += a; });

    A *__restrict__ out = ws + int64_t(blockIdx.y) * K * (int64_t(d) + 1);
    mfma_for_each(t, acc, [&](int r, int c, A v) {
        const int o = o0 + r, i = i0 + c;
        if (o < K && i < d) out[int64_t(o) * d + i] = v;
    });
    if (i0 == 0) {                                        // uniform over the workgroup
        Db[sk][so] = dbs;
        __syncthreads();
        if (sk == 0 && o_ok) {
            A s = Db[0][so];
#pragma unroll
            for (int j = 1; j < KS; ++j) s += Db[j][so];
            out[int64_t(K) * d + o0 + so] = s;
        }
    }
}

// dW[e] / db[e - K d] = the sum over the chunks, in chunk order, of ws[c * len + e], len = K (d + 1).
template <typename A>
__global__ __launch_bounds__(kBlock) void probe_grad_reduce_kernel(const A *__restrict__ ws, int64_t n_chunks, int64_t len,
                                                                   int64_t n_dw, A *__restrict__ dW, A *__restrict__ db) {
    const int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= len) return;
    A s = A(0);
    for (int64_t c = 0; c < n_chunks; ++c) s += ws[c * len + e];
    if (e < n_dw) dW[e] = s;
    else db[e - n_dw] = s;
}

}  // namespace clane
