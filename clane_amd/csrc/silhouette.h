// Silhouette of a partition of rows of a table: per position p of the rows sorted by cluster and per cluster c, the sum
// of the distances from p to the members of c -- the n x K sums the score is made of, never the n x n distances.
//
// Reference being replaced: nothing in the reference -- scikit-learn's silhouette_samples on the host, whose definition
// the sums follow (pairwise distances "euclidean" and "cosine", a = mean to the own cluster without the point itself,
// b = the lowest mean to another cluster).  A score calls, in this order,
//
//   norms : nrm[p] of the row a_p = Z[order[p]] - mu (mu is subtracted in the operand loaders, as tsne_sqdist_kernel
//           does): a workgroup contracts a 128-row tile WITH ITSELF through mfma_tile_product and keeps the diagonal, so
//           |a_p|^2 is the very MFMA chain (mfma_slice's k order) that a_p . a_j is.  euclidean keeps sq = |a|^2, cosine
//           r = 1 / sqrt(sq), r = 0 for a zero row.  O(n 128 d).
//   sums  : S[p - p0, c] (double) = sum over j in [seg[c], seg[c + 1]) of dist(p, j) for the positions p in [p0, p1):
//           a workgroup owns one 128-position row tile and ONE cluster and walks the cluster's 128-column tiles, both
//           operands gathered through `order`; after each tile the accumulators become distances and are added to
//           per-row running sums in registers.  The grid is cluster-major (blockIdx.x = c * row_tiles + row tile): the
//           workgroups that run together read the same columns.
//
// Distances (A = the accumulate type: fp32 for fp32 and bf16 tables, fp64 for fp64):
//   euclidean : sqrt(max(0, fma(-2, a_i . a_j, sq_i + sq_j))); the square root is __builtin_sqrtf / __builtin_sqrt, i.e.
//               llvm.sqrt, which hipcc expands correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt, its default;
//               NOT __fsqrt_rn, which HIP maps to the approximate native square root).  Two positions whose
//               table rows hold the same bits have sq_i = sq_j = a_i . a_j bit for bit, (s + s) and 2 s are exact, and the
//               distance is exactly 0.
//   cosine    : max(0, 1 - ((a_i . a_j) r_i) r_j); a zero row is at distance 1 from everything, itself excepted.
//   The element with p == j (the same POSITION) contributes exactly 0 in both.
//
// Order of a sum S[p, c] -- a function of seg alone, never of p0, p1, the grid or the row tile p falls in: the columns
// of cluster c are numbered from the segment's start, q = j - seg[c]; partial (h, l) of 2 x 16 (h = (q % 128) / 64,
// l = q % 16) adds, in double, the distances of its columns in ascending q, starting from 0.0; the 16 partials of one h
// are folded by the xor butterfly over l (masks 8, 4, 2, 1); the result is fold(h = 0) + fold(h = 1).  No atomics: two
// calls give the same bits, and so does any division of the positions into blocks.
//
// Table rows outside [0, table_rows) are read as zero rows (a = -mu) -- an index never leaves the table; seg is clamped
// to [0, n], so a position never leaves `order`.
#pragma once

#include "device_utils.h"
#include "mfma_tile.h"

namespace clane {

constexpr int kSilEuclidean = 0;   // CLANE_SILHOUETTE_EUCLIDEAN
constexpr int kSilCosine = 1;      // CLANE_SILHOUETTE_COSINE

__device__ __forceinline__ float sil_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double sil_sqrt(double x) { return __builtin_sqrt(x); }
__device__ __forceinline__ float sil_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double sil_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// ---- norms ---------------------------------------------------------------------------------------------------------
// Row tile blockIdx.x of the positions [0, n): the tile times itself, the diagonal kept.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock, sizeof(A) == 8 ? 1 : 2) void silhouette_norms_kernel(
    const T *__restrict__ Z, int64_t table_rows, int d, int64_t ldz, const int32_t *__restrict__ order, int64_t n,
    const A *__restrict__ mu, int metric, A *__restrict__ nrm) {
    using Tile = MfmaTile<A, 4>;
    static_assert(Tile::BM == Tile::BN && Tile::PER_A == Tile::PER_B, "square tiles: a tile times itself");
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];

    const Tile t(threadIdx.x);
    const int64_t m0 = int64_t(blockIdx.x) * Tile::BM;
    int64_t ra[Tile::PER_A];
    mfma_gather_offsets(order, m0, n, table_rows, ldz, ra);

    typename Tile::acc4 acc[4][4];
    mfma_zero<A>(acc);
    auto load = [&](int s, int, int k) {
        return k < d ? (ra[s] >= 0 ? A(Elem<T>::to_acc(Z[ra[s] + k])) : A(0)) - mu[k] : A(0);
    };
    mfma_tile_product(t, As, Bs, d, acc, load, load);

    mfma_for_each(t, acc, [&](int r, int c, A dot) {
        if (r != c || m0 + r >= n) return;
        A v = dot;
        if (metric == kSilCosine) v = dot > A(0) ? A(1) / sil_sqrt(dot) : A(0);
        nrm[m0 + r] = v;
    });
}

// ---- sums ----------------------------------------------------------------------------------------------------------
// blockIdx.x = c * row_tiles + rt: the positions p0 + 128 rt .. of cluster c's columns.  S [p1 - p0, K].
template <typename T, typename A>
__global__ __launch_bounds__(kBlock, sizeof(A) == 8 ? 1 : 2) void silhouette_sums_kernel(
    const T *__restrict__ Z, int64_t table_rows, int d, int64_t ldz, const int32_t *__restrict__ order, int64_t n,
    const int64_t *__restrict__ seg, int K, const A *__restrict__ mu, const A *__restrict__ nrm, int metric, int64_t p0,
    int64_t p1, int row_tiles, double *__restrict__ S) {
    using Tile = MfmaTile<A, 4>;
    constexpr int BM = Tile::BM, BN = Tile::BN;
    __shared__ __attribute__((aligned(16))) A As[BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[BN * Tile::LD];
    __shared__ double Sh[2][BM];
    __shared__ A Nr[BM];

    const Tile t(threadIdx.x);
    const int c = int(blockIdx.x) / row_tiles, rt = int(blockIdx.x) % row_tiles;
    const int64_t m0 = p0 + int64_t(rt) * BM;
    int64_t beg = seg[c], end = seg[c + 1];
    if (beg < 0) beg = 0;
    if (end > n) end = n;

    int64_t ra[Tile::PER_A], rb[Tile::PER_B];
    mfma_gather_offsets(order, m0, p1, table_rows, ldz, ra);

    // sq or r of the tile's rows: in LDS, not in 16 registers a lane (the first barrier of a tile's product comes before
    // the first read)
    if (threadIdx.x < BM) Nr[threadIdx.x] = m0 + threadIdx.x < p1 ? nrm[m0 + threadIdx.x] : A(0);
    double run[4][4];                                         // [mi][reg]: running sums of this lane's columns, 16 rows
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) run[mi][reg] = 0.0;

    for (int64_t j0 = beg; j0 < end; j0 += BN) {
        mfma_gather_offsets(order, j0, end, table_rows, ldz, rb);
        typename Tile::acc4 acc[4][4];
        mfma_zero<A>(acc);
        mfma_tile_product(
            t, As, Bs, d, acc,
            [&](int s, int, int k) { return k < d ? (ra[s] >= 0 ? A(Elem<T>::to_acc(Z[ra[s] + k])) : A(0)) - mu[k] : A(0); },
            [&](int s, int, int k) { return k < d ? (rb[s] >= 0 ? A(Elem<T>::to_acc(Z[rb[s] + k])) : A(0)) - mu[k] : A(0); });
        // a lane holds column j0 + wn + 16 ni + li of 16 rows; the columns of one lane come in ascending order
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int64_t j = j0 + t.col(ni);
            const bool live = j < end;
            const A nj = live ? nrm[j] : A(0);
            const int64_t self = j - m0;                      // the tile row that IS column j
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const A dot = acc[mi][ni][reg];
                    A dist;
                    if (metric == kSilCosine) {
                        dist = A(1) - (dot * Nr[t.row(mi, reg)]) * nj;
                        dist = dist > A(0) ? dist : A(0);
                    } else {
                        A v = sil_fma(A(-2), dot, Nr[t.row(mi, reg)] + nj);
                        v = v > A(0) ? v : A(0);
                        dist = sil_sqrt(v);
                    }
                    if (!live || self == int64_t(t.row(mi, reg))) dist = A(0);
                    run[mi][reg] += double(dist);
                }
        }
    }

    // the 16 lanes of one g share a row: butterfly over l; then the two column halves meet in LDS
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const double v = group_sum<16>(run[mi][reg]);
            if (t.li == 0) Sh[t.wn / 64][t.row(mi, reg)] = v;
        }
    __syncthreads();
    if (threadIdx.x < BM) {
        const int64_t i = m0 + threadIdx.x;
        if (i < p1) S[(i - p0) * K + c] = Sh[0][threadIdx.x] + Sh[1][threadIdx.x];
    }
}

}  // namespace clane
