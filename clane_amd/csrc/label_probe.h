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
#include "pair_train.h"
#include "projection.h"

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

// ---- forward ---------------------------------------------------------------------------------------------------
// The tiling of project_rows_kernel (projection.h) with the rows of the A operand taken through `rows`, as
// pair_project_kernel does, and n_out = K.  Block b: column tile b % n_tiles of row tile b / n_tiles.  loss_ws
// [row tiles, F]: the tile's sum of split * (lse - logit[y]) per fit, in double.  split is [n, >= F] with leading
// dimension ld_split, pred [n, >= F] with ld_pred: a caller that fits in groups hands in a column slice of each.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void probe_forward_kernel(
    const T *__restrict__ Z, int64_t table_rows, int d, int64_t ldz, const int32_t *__restrict__ rows,
    const int32_t *__restrict__ y, int64_t n, const uint8_t *__restrict__ split, int64_t ld_split,
    const A *__restrict__ W, const A *__restrict__ bias, int F, int C, int cp_log, int flags, A *__restrict__ G,
    double *__restrict__ loss_ws, int32_t *__restrict__ pred, int64_t ld_pred, int n_tiles) {
    using M = ProjMfma<A>;
    using acc4 = typename M::acc4;
    constexpr int BM = kProjBM, BN = kProjBN, BK = kProjBK;
    constexpr int LD = BK + 16 / int(sizeof(A));
    constexpr int PER = BM * BK / kBlock;
    __shared__ __attribute__((aligned(16))) A As[BM * LD];
    __shared__ __attribute__((aligned(16))) A Bs[BN * LD];
    __shared__ double Ls[kWavesPerBlock][kWave];

    const int Cp = 1 << cp_log, K = F << cp_log;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t tile = blockIdx.x;
    const int n0 = int(tile % n_tiles) * BN;
    const int64_t row_tile = tile / n_tiles, m0 = row_tile * BM;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    const int g = lane >> 4, li = lane & 15;

    const int sk = tid % BK, si = tid / BK;
    int64_t roff[PER];                                    // gathered rows of this thread's staging slots; < 0: none
#pragma unroll
    for (int s = 0; s < PER; ++s) {
        const int64_t r = m0 + si + s * (kBlock / BK);
        int64_t t = -1;
        if (r < n) {
            t = rows[r];
            if (t >= table_rows) t = -1;
        }
        roff[s] = t < 0 ? -1 : t * ldz;
    }
    A ra[PER], rb[PER];
    auto fetch = [&](int k0) {
        const int k = k0 + sk;
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            const int j = n0 + si + s * (kBlock / BK);
            ra[s] = (k < d && roff[s] >= 0) ? A(Elem<T>::to_acc(Z[roff[s] + k])) : A(0);
            rb[s] = (k < d && j < K) ? W[int64_t(j) * d + k] : A(0);
        }
    };

    acc4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = acc4{A(0), A(0), A(0), A(0)};

    fetch(0);
    for (int k0 = 0; k0 < d; k0 += BK) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            const int i = si + s * (kBlock / BK);
            As[i * LD + sk] = ra[s];
            Bs[i * LD + sk] = rb[s];
        }
        __syncthreads();
        if (k0 + BK < d) fetch(k0 + BK);
        A a[4][4], b[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                a[t][kk] = As[(wm + 16 * t + li) * LD + 4 * g + kk];
                b[t][kk] = Bs[(wn + 16 * t + li) * LD + 4 * g + kk];
            }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = M::mma(a[mi][kk], b[ni][kk], acc[mi][ni]);
    }

    // ---- epilogue: a lane holds column n0 + wn + 16 ni + li of 16 rows; the 16 lanes of one g share a row ----------
    const A neg_inf = -__builtin_huge_val();
    int fit[4], cls[4];
    bool in_k[4], real[4];
    A bcol[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int col = n0 + wn + 16 * ni + li;
        fit[ni] = col >> cp_log;
        cls[ni] = col & (Cp - 1);
        in_k[ni] = col < K;
        real[ni] = in_k[ni] && cls[ni] < C;
        bcol[ni] = in_k[ni] ? bias[col] : A(0);
    }
    double lsum[4] = {0.0, 0.0, 0.0, 0.0};
    auto op_max = [](A u, A v) { return u > v ? u : v; };
    auto op_add = [](A u, A v) { return u + v; };
    auto op_min = [](int u, int v) { return u < v ? u : v; };
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t r = m0 + wm + 16 * mi + M::row(lane, reg);
            const bool in_n = r < n;
            const int yr = in_n ? y[r] : -1;
            A l[4], mx[4], e[4], se[4], ly[4];
            int am[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                l[ni] = acc[mi][ni][reg] + bcol[ni];
                mx[ni] = real[ni] ? l[ni] : neg_inf;
            }
            probe_fit_reduce(mx, Cp, op_max);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                e[ni] = real[ni] ? exp_acc<A>(l[ni] - mx[ni]) : A(0);
                se[ni] = e[ni];
                ly[ni] = (real[ni] && cls[ni] == yr) ? l[ni] : A(0);
                am[ni] = (real[ni] && l[ni] == mx[ni]) ? cls[ni] : INT_MAX;      // ties: the lowest class
            }
            probe_fit_reduce(se, Cp, op_add);
            probe_fit_reduce(ly, Cp, op_add);
            probe_fit_reduce(am, Cp, op_min);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                if (!(in_n && in_k[ni])) continue;
                const int col = n0 + wn + 16 * ni + li;
                const bool trains = split[r * ld_split + fit[ni]] != 0;
                if (flags & kProbeWriteG) {
                    A gv = A(0);
                    if (trains && real[ni]) gv = e[ni] / se[ni] - (cls[ni] == yr ? A(1) : A(0));
                    G[r * int64_t(K) + col] = gv;
                }
                if (trains) lsum[ni] += double(mx[ni] + log_acc<A>(se[ni]) - ly[ni]);
                if ((flags & kProbeWritePred) && cls[ni] == 0) pred[r * ld_pred + fit[ni]] = am[ni];
            }
        }
    // the tile's loss per fit: a lane's 16 rows (above, in (mi, reg) order), the four row groups of the wave, then the
    // two waves that share the columns
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        double t = lsum[ni];
        t += lane_xor<16>(t);
        t += lane_xor<32>(t);
        if (g == 0) Ls[wave][16 * ni + li] = t;
    }
    __syncthreads();
    if (tid < BN) {
        const int col = n0 + tid, q = tid / 64, within = tid % 64;
        if (col < K && (col & (Cp - 1)) == 0)
            loss_ws[row_tile * F + (col >> cp_log)] = Ls[2 * q][within] + Ls[2 * q + 1][within];
    }
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
// is G^T, the B operand the gathered rows of Z, both staged k-contiguous per output row; memory is row-major in i, so
// a thread stages one o / c of 8 rows of each 16-row slice).  blockIdx = (tile of dW: K tiles x d tiles, chunk).  The
// workgroups of the first d tile also sum their G columns: a thread adds what it stages, in row order, and the two
// threads of a column are added at the end -- db's partial.  The partials of chunk z go to ws + z * K * (d + 1):
// [K, d] of dW, then [K] of db.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void probe_grad_kernel(const T *__restrict__ Z, int64_t table_rows, int d,
                                                            int64_t ldz, const int32_t *__restrict__ rows, int64_t n,
                                                            const A *__restrict__ G, int K, A *__restrict__ ws,
                                                            int n_tiles) {
    using M = ProjMfma<A>;
    using acc4 = typename M::acc4;
    constexpr int BM = kProjBM, BN = kProjBN, BK = kProjBK;
    constexpr int LD = BK + 16 / int(sizeof(A));
    constexpr int KS = kBlock / BM;                       // rows of a slice staged side by side (2)
    constexpr int PER = BK / KS;                          // rows per thread and slice (8)
    static_assert(BM == BN && kBlock % BM == 0 && BK % KS == 0 && kGradChunk % BK == 0, "staging layout");
    __shared__ __attribute__((aligned(16))) A As[BM * LD];
    __shared__ __attribute__((aligned(16))) A Bs[BN * LD];
    __shared__ A Db[KS][BM];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int o0 = int(blockIdx.x / n_tiles) * BM, i0 = int(blockIdx.x % n_tiles) * BN;
    const int64_t kbeg = int64_t(blockIdx.y) * kGradChunk;
    const int64_t kend = kbeg + kGradChunk < n ? kbeg + kGradChunk : n;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    const int g = lane >> 4, li = lane & 15;

    const int so = tid % BM, sk = tid / BM;
    const bool o_ok = o0 + so < K, i_ok = i0 + so < d;
    A ra[PER], rb[PER];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            const int64_t k = k0 + sk + KS * s;
            ra[s] = A(0);
            rb[s] = A(0);
            if (k < kend) {
                int64_t t = rows[k];
                if (t >= table_rows) t = -1;
                if (o_ok) ra[s] = G[k * K + o0 + so];
                if (i_ok && t >= 0) rb[s] = A(Elem<T>::to_acc(Z[t * ldz + i0 + so]));
            }
        }
    };

    acc4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = acc4{A(0), A(0), A(0), A(0)};
    A dbs = A(0);

    fetch(kbeg);
    for (int64_t k0 = kbeg; k0 < kend; k0 += BK) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            As[so * LD + sk + KS * s] = ra[s];
            Bs[so * LD + sk + KS * s] = rb[s];
            dbs += ra[s];
        }
        __syncthreads();
        if (k0 + BK < kend) fetch(k0 + BK);
        A a[4][4], b[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                a[t][kk] = As[(wm + 16 * t + li) * LD + 4 * g + kk];
                b[t][kk] = Bs[(wn + 16 * t + li) * LD + 4 * g + kk];
            }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = M::mma(a[mi][kk], b[ni][kk], acc[mi][ni]);
    }

    A *__restrict__ out = ws + int64_t(blockIdx.y) * K * (int64_t(d) + 1);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int i = i0 + wn + 16 * ni + li;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int o = o0 + wm + 16 * mi + M::row(lane, reg);
                if (o < K && i < d) out[int64_t(o) * d + i] = acc[mi][ni][reg];
            }
        }
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
