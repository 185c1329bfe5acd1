// Training step of the bilinear similarity (AsymmertricSimilarity) on explicit pairs.
//
// Reference being replaced: IterativeEmbedder.update_similarity_measure (clane/embedder.py:249-289) -- per step
// Z[src_idx], Z[dst_idx] by indexing, the two nn.Linear, sigmoid, the masked log loss, autograd and torch.optim.Adam,
// with one host decision per step (`if ~mask.any(): continue`).  Here a step is
//
//   pair_project : A[k,:] = Phi_src z_src[k],  Bm[k,:] = Phi_dst z_dst[k]      gathered-row MFMA projection
//   pair_loss    : s, p = sigmoid(s), q = sigmoid(-s), mask, loss_k, g_k = d loss_k / d s; {sum loss, M} on the device
//   pair_grad    : dW = (1/M) sum_k g_k {Bm[k]^T z_src[k] ; A[k]^T z_dst[k]}   MFMA contraction over k, in chunks
//   adam_step    : torch.optim.Adam's defaults; M == 0 changes nothing (the reference's `continue`)
//
// and the host reads nothing back.  pair_labels answers "is (src, dst) an edge" by binary search in a sorted CSR.
// The pairs, the labels and the uniforms u are INPUTS: the reference's random streams cannot be replayed from seeds.
// Every sum runs in a fixed order (no atomics): two calls give the same bits.
//
// Table rows outside [0, table_rows) are read as zero rows -- an index never leaves the table.
#pragma once

#include "device_utils.h"
#include "mfma_tile.h"

namespace clane {

constexpr int kGradChunk = 2048;   // pairs per workgroup of pair_grad_kernel (a multiple of kProjBK)
constexpr int kPairLanes = 16;     // lanes that share one pair in pair_loss_kernel (one DPP row)

template <typename A>
__device__ __forceinline__ A log_acc(A v);
template <>
__device__ __forceinline__ float log_acc<float>(float v) {
    return logf(v);
}
template <>
__device__ __forceinline__ double log_acc<double>(double v) {
    return log(v);
}

// ---- forward ---------------------------------------------------------------------------------------------------
// Out_side[k, 0:d) = W_side . Z[idx_side[k], 0:d)  for side 0 (src, Phi_src = W[0:d]) and side 1 (dst, Phi_dst = W[d:2d]).
// mfma_tile_product (mfma_tile.h) with the rows of the A operand taken through the index list and n_out = d;
// blockIdx.y is the side.  Outputs are [B, d] contiguous.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void pair_project_kernel(const T *__restrict__ Z, int64_t table_rows, int d,
                                                              int64_t ldz, const int32_t *__restrict__ src,
                                                              const int32_t *__restrict__ dst, int64_t B,
                                                              const A *__restrict__ W, A *__restrict__ PA,
                                                              A *__restrict__ PB, int n_tiles) {
    using Tile = MfmaTile<A, 4>;
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];

    const int side = blockIdx.y;
    const int32_t *__restrict__ idx = side ? dst : src;
    const A *__restrict__ Ws = W + int64_t(side) * d * d;
    A *__restrict__ Y = side ? PB : PA;

    const Tile t(threadIdx.x);
    const int64_t tile = blockIdx.x;
    const int n0 = int(tile % n_tiles) * Tile::BN;
    const int64_t m0 = (tile / n_tiles) * Tile::BM;

    int64_t roff[Tile::PER_A];                               // gathered rows of this thread's staging slots; < 0: none
    mfma_gather_offsets(idx, m0, B, table_rows, ldz, roff);

    typename Tile::acc4 acc[4][4];
    mfma_zero<A>(acc);
    mfma_tile_product(
        t, As, Bs, d, acc,
        [&](int s, int, int k) { return (k < d && roff[s] >= 0) ? A(Elem<T>::to_acc(Z[roff[s] + k])) : A(0); },
        [&](int, int i, int k) {
            const int j = n0 + i;
            return (k < d && j < d) ? Ws[int64_t(j) * d + k] : A(0);
        });

    mfma_for_each(t, acc, [&](int i, int j, A v) {
        const int64_t r = m0 + i;
        const int col = n0 + j;
        if (r < B && col < d) Y[r * d + col] = v;
    });
}

// ---- loss ------------------------------------------------------------------------------------------------------
// Per pair (embedder.py:276-282): s = A[k] . Bm[k]; p = sigmoid(s) and q = sigmoid(-s) from one exp(-|s|), so that
// 1 - p never is a subtraction; mask = linked XOR (u < p) (u < p: the Bernoulli trial with probability p);
// loss_k = -log((linked ? p : q) + 1e-10); g_k = d loss_k / d s = linked ? -p q / (p + 1e-10) : p q / (q + 1e-10),
// zero where mask is 0.  ws[b] / ws[gridDim.x + b]: workgroup b's sums of mask * loss_k and of mask, in double.
template <typename A>
__global__ __launch_bounds__(kBlock) void pair_loss_kernel(const A *__restrict__ PA, const A *__restrict__ PB, int64_t B,
                                                           int d, const uint8_t *__restrict__ linked,
                                                           const A *__restrict__ u, A *__restrict__ g,
                                                           uint8_t *__restrict__ mask, double *__restrict__ ws) {
    __shared__ double smem[kWavesPerBlock];
    constexpr int GROUPS = kBlock / kPairLanes;
    const int sub = threadIdx.x % kPairLanes, grp = threadIdx.x / kPairLanes;
    double loss_sum = 0.0, count = 0.0;
    for (int64_t k = int64_t(blockIdx.x) * GROUPS + grp; k < B; k += int64_t(gridDim.x) * GROUPS) {
        const A *__restrict__ a = PA + k * d;
        const A *__restrict__ b = PB + k * d;
        A s = A(0);
        for (int c = sub; c < d; c += kPairLanes) s += a[c] * b[c];
        s = group_sum<kPairLanes>(s);
        if (sub == 0) {
            const A e = exp_acc<A>(s < A(0) ? s : -s);
            const A hi = A(1) / (A(1) + e), lo = e / (A(1) + e);
            const A p = s >= A(0) ? hi : lo, q = s >= A(0) ? lo : hi;
            const bool lk = linked[k] != 0;
            const bool trial = u[k] < p;
            const bool mk = lk != trial;
            const A loss = -log_acc<A>((lk ? p : q) + A(1e-10));
            const A gk = lk ? -(p * q) / (p + A(1e-10)) : (p * q) / (q + A(1e-10));
            g[k] = mk ? gk : A(0);
            mask[k] = mk ? 1 : 0;
            if (mk) {
                loss_sum += double(loss);
                count += 1.0;
            }
        }
    }
    const double t0 = block_sum_fixed(loss_sum, smem);
    const double t1 = block_sum_fixed(count, smem);
    if (threadIdx.x == 0) {
        ws[blockIdx.x] = t0;
        ws[gridDim.x + blockIdx.x] = t1;
    }
}

// ---- backward --------------------------------------------------------------------------------------------------
// Partial dW of one chunk of pairs: side 0 (rows [0, d) of dW): out[o, i] = sum_k g_k Bm[k, o] Z[src_k, i];
// side 1 (rows [d, 2d)): out[o, i] = sum_k g_k A[k, o] Z[dst_k, i].  A GEMM whose contraction index is the pair: the
// A operand is (g . projected)^T, the B operand the gathered rows of Z; memory is pair-major, so the slices are staged
// by mfma_tile_product_transposed (mfma_tile.h).  blockIdx = (tile of dW's side, side, chunk); the partial tile goes to
// ws[(chunk * 2 + side) * d * d + o * d + i].
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void pair_grad_kernel(const T *__restrict__ Z, int64_t table_rows, int d,
                                                           int64_t ldz, const int32_t *__restrict__ src,
                                                           const int32_t *__restrict__ dst, int64_t B,
                                                           const A *__restrict__ PA, const A *__restrict__ PB,
                                                           const A *__restrict__ gvec, A *__restrict__ ws, int n_tiles) {
    using Tile = MfmaTile<A, 4>;
    static_assert(kGradChunk % Tile::BK == 0, "a chunk is whole slices");
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];

    const int side = blockIdx.y;
    const int32_t *__restrict__ idx = side ? dst : src;
    const A *__restrict__ Op = side ? PA : PB;

    const Tile t(threadIdx.x);
    const int o0 = int(blockIdx.x / n_tiles) * Tile::BM, i0 = int(blockIdx.x % n_tiles) * Tile::BN;
    const int64_t kbeg = int64_t(blockIdx.z) * kGradChunk;
    const int64_t kend = kbeg + kGradChunk < B ? kbeg + kGradChunk : B;

    const int so = int(threadIdx.x) % Tile::BM;              // the output row / column this thread stages
    const bool o_ok = o0 + so < d, i_ok = i0 + so < d;

    typename Tile::acc4 acc[4][4];
    mfma_zero<A>(acc);
    mfma_tile_product_transposed(
        t, As, Bs, kbeg, kend, acc,
        [&](int64_t k, A &a, A &b) {
            const A gk = gvec[k];
            int64_t r = idx[k];
            if (r >= table_rows) r = -1;
            if (o_ok) a = gk * Op[k * d + o0 + so];
            if (i_ok && r >= 0) b = A(Elem<T>::to_acc(Z[r * ldz + i0 + so]));
        },
        [](A) {});

    A *__restrict__ out = ws + (int64_t(blockIdx.z) * 2 + side) * d * d;
    mfma_for_each(t, acc, [&](int r, int c, A v) {
        const int o = o0 + r, i = i0 + c;
        if (o < d && i < d) out[int64_t(o) * d + i] = v;
    });
}

// dW[e] = (sum over the chunks, in chunk order, of ws[c * n + e]) / M, M = stats[1]; M == 0: dW = 0.
template <typename A>
__global__ __launch_bounds__(kBlock) void pair_grad_reduce_kernel(const A *__restrict__ ws, int64_t n_chunks, int64_t n,
                                                                  const double *__restrict__ stats,
                                                                  A *__restrict__ dW) {
    const int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= n) return;
    const double m = stats[1];
    A s = A(0);
    for (int64_t c = 0; c < n_chunks; ++c) s += ws[c * n + e];
    dW[e] = m > 0.0 ? s / A(m) : A(0);
}

// ---- Adam ------------------------------------------------------------------------------------------------------
// torch.optim.Adam with its defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad), the operations in the
// order of its single-tensor form: m += (g - m)(1 - b1); v = v b2 + (1 - b2) g g; W += (-lr / (1 - b1^t)) m /
// (sqrt(v) / sqrt(1 - b2^t) + eps) with t = state[0] + 1; the bias corrections are computed in double as torch computes
// them in Python floats.  stats[1] == 0 (no pair took part in the loss): nothing is touched.
template <typename A>
__global__ __launch_bounds__(kBlock) void adam_step_kernel(A *__restrict__ W, A *__restrict__ m, A *__restrict__ v,
                                                           const A *__restrict__ grad, int64_t n, double lr,
                                                           const double *__restrict__ stats,
                                                           const double *__restrict__ state) {
    if (!(stats[1] > 0.0)) return;
    const int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= n) return;
    const double t = state[0] + 1.0;
    const double bc1 = 1.0 - pow(0.9, t), bc2 = 1.0 - pow(0.999, t);
    const A step_size = A(-(lr / bc1)), bc2_sqrt = A(sqrt(bc2));
    const A gi = grad[e];
    const A mi = m[e] + (gi - m[e]) * A(1.0 - 0.9);
    const A vi = v[e] * A(0.999) + A(1.0 - 0.999) * gi * gi;
    const A denom = sqrt(vi) / bc2_sqrt + A(1e-8);
    m[e] = mi;
    v[e] = vi;
    W[e] = W[e] + step_size * mi / denom;
}

// After adam_step_kernel: state[0] (steps taken) += 1 and state[1] (sum of the step losses of the epoch) +=
// stats[0] / M -- unless M == 0, the skipped step of embedder.py:280-281.
__global__ void adam_finish_kernel(const double *__restrict__ stats, double *__restrict__ state) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && stats[1] > 0.0) {
        state[0] += 1.0;
        state[1] += stats[0] / stats[1];
    }
}

// ---- labels ----------------------------------------------------------------------------------------------------
// linked[k] = dst[k] in colidx[rowptr[src[k]] .. rowptr[src[k] + 1]): binary search, rows sorted and unique.
__global__ __launch_bounds__(kBlock) void pair_labels_kernel(const int64_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ colidx, int64_t nrows,
                                                             const int32_t *__restrict__ src,
                                                             const int32_t *__restrict__ dst, int64_t B,
                                                             uint8_t *__restrict__ linked) {
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < B; k += int64_t(gridDim.x) * kBlock) {
        const int64_t s = src[k];
        const int32_t want = dst[k];
        uint8_t found = 0;
        if (s >= 0 && s < nrows) {
            int64_t lo = rowptr[s], hi = rowptr[s + 1];
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                const int32_t c = colidx[mid];
                if (c < want) lo = mid + 1;
                else hi = mid;
            }
            found = (lo < rowptr[s + 1] && colidx[lo] == want) ? 1 : 0;
        }
        linked[k] = found;
    }
}

}  // namespace clane
