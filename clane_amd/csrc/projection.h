// Row projection for the bilinear similarity -- Y = Z . W^T on the matrix cores.
//
// Reference being replaced: the two bias-free nn.Linear of AsymmertricSimilarity (clane/similarity.py:40-57), which
// the reference applies to z_src and z_dst of EVERY edge (graph.py:119-121: E d^2 multiply-adds twice).  Here every
// table row is projected once:  W = cat(Phi_src.weight, Phi_dst.weight) is [2d, d] row-major (nn.Linear stores
// [out, in]), so Y[r, 0:d) = Phi_src z_r and Y[r, d:2d) = Phi_dst z_r, one GEMM for both.  The pair K1
// (edge_score.h, PAIR instances) then scores edge (r, c) as dot(Y[r, 0:d), Y[c, d:2d)).
//
// The contraction is mfma_tile.h's (tiling, staging, the fixed k order); this kernel adds the two row-major operands.
//
// Any shape: K is zero-padded past d (guarded loads), partial row / column tiles are guarded on store, and the
// leading dimensions ldz >= d, ldy >= 2d are free.
#pragma once

#include "device_utils.h"
#include "mfma_tile.h"

namespace clane {

// Y[rows, n_out] (ld ldy) = Z[rows, d] (ld ldz) . W[n_out, d]^T (W row-major, ld d).  One-dimensional grid: block b
// computes column tile b % n_tiles of row tile b / n_tiles, so the workgroups that read one slice of Z run together
// and Z comes from HBM once.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void project_rows_kernel(const T *__restrict__ Z, int64_t rows, int d, int64_t ldz,
                                                              const A *__restrict__ W, int n_out, A *__restrict__ Y,
                                                              int64_t ldy, int n_tiles) {
    using Tile = MfmaTile<A, 4>;
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];

    const Tile t(threadIdx.x);
    const int64_t tile = blockIdx.x;
    const int n0 = int(tile % n_tiles) * Tile::BN;
    const int64_t m0 = (tile / n_tiles) * Tile::BM;

    typename Tile::acc4 acc[4][4];
    mfma_zero<A>(acc);
    mfma_tile_product(
        t, As, Bs, d, acc,
        [&](int, int i, int k) {
            const int64_t r = m0 + i;
            return (k < d && r < rows) ? A(Elem<T>::to_acc(Z[r * ldz + k])) : A(0);
        },
        [&](int, int i, int k) {
            const int j = n0 + i;
            return (k < d && j < n_out) ? W[int64_t(j) * d + k] : A(0);
        });

    mfma_for_each(t, acc, [&](int i, int j, A v) {
        const int64_t r = m0 + i;
        const int col = n0 + j;
        if (r < rows && col < n_out) Y[r * ldy + col] = v;
    });
}

}  // namespace clane
