// Node clustering: the two halves of one Lloyd iteration of k-means on rows of the embedding table, R restarts at once.
//
//   kmeans_assign : per (row i of the list, restart r) the centre j that minimises csq[r, j] - 2 z_i . c[r, j] (the
//                   squared distance without the row's own |z_i|^2, which no centre changes) and that minimum.  The
//                   dots are mfma_tile_product's (mfma_tile.h) with the A operand's rows taken through `rows`; a
//                   workgroup owns 128 rows of ONE restart and walks every
//                   128-column tile of that restart's centres, keeping the running (best, id) of its rows in registers.
//                   The n x K distances never reach memory.
//   kmeans_update : centre = (sum of its segment's rows) / count, from the rows sorted by assigned centre.  The
//                   memory-bound half: one gather of the listed rows per restart.
//
// Order rule of the arg-min: value ascending, ties by centre index ascending -- a total order, so what a row gets does
// not depend on which tile, wave or lane met a centre first.  A (row, centre) dot is the same MFMA chain in
// mfma_slice's k order (mfma_tile.h) wherever the pair falls in the tiling, so two calls give the same bits and a restart gets the
// same bits whatever else shares the call.
//
// Sums of the update run in a fixed order (no atomics): a segment is cut into chunks of kKmChunk rows counted from the
// segment's own start; inside a chunk row slot s (of S, a function of d alone) adds rows s, s + S, ... in order, the
// slots are added in slot order, and the chunks in chunk order.
//
// Table rows outside [0, table_rows) are read as zero rows -- an index never leaves the table.
#pragma once

#include <climits>

#include "device_utils.h"
#include "mfma_tile.h"

namespace clane {

constexpr int kKmChunk = 2048;     // rows of a segment summed by one workgroup
constexpr int kKmInFlight = 4;     // gathered rows in flight per thread of kmeans_chunk_kernel

// (v, j) < (bv, bj) in the order rule.  A NaN never wins.
template <typename A>
__device__ __forceinline__ void km_take(A v, int j, A &bv, int &bj) {
    if (v < bv || (v == bv && j < bj)) {
        bv = v;
        bj = j;
    }
}
template <int M, typename A>
__device__ __forceinline__ void km_xor_step(A &bv, int &bj) {
    const A ov = lane_xor<M>(bv);
    const int oj = lane_xor<M>(bj);
    km_take(ov, oj, bv, bj);
}

// ---- assignment ------------------------------------------------------------------------------------------------
// grid = (row tiles, R).  centres [R, K, d], csq [R, K] in the accumulate type; assign [n, ld_assign], best [n, ld_best].
// Two waves per SIMD for the f32 accumulators (256 registers a lane); the f64 tile alone is 128 and takes the whole file.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock, sizeof(A) == 8 ? 1 : 2) void kmeans_assign_kernel(
    const T *__restrict__ Z, int64_t table_rows, int d, int64_t ldz, const int32_t *__restrict__ rows, int64_t n,
    const A *__restrict__ centres, const A *__restrict__ csq, int K, int32_t *__restrict__ assign, int64_t ld_assign,
    A *__restrict__ best, int64_t ld_best) {
    using Tile = MfmaTile<A, 4>;
    constexpr int BM = Tile::BM, BN = Tile::BN;
    __shared__ __attribute__((aligned(16))) A As[BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[BN * Tile::LD];
    __shared__ A Sv[2][BM];
    __shared__ int Sj[2][BM];

    const Tile t(threadIdx.x);
    const int tid = threadIdx.x;
    const int64_t m0 = int64_t(blockIdx.x) * BM;
    const int rst = blockIdx.y;
    const A *__restrict__ Cr = centres + int64_t(rst) * K * d;
    const A *__restrict__ cq = csq + int64_t(rst) * K;

    int64_t roff[Tile::PER_A];                            // gathered rows of this thread's staging slots; < 0: none
    mfma_gather_offsets(rows, m0, n, table_rows, ldz, roff);

    const A inf = __builtin_huge_val();
    A bv[4][4];                                           // [mi][reg]: running minimum of 16 rows over this lane's columns
    int bj[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            bv[mi][reg] = inf;
            bj[mi][reg] = INT_MAX;
        }

    for (int n0 = 0; n0 < K; n0 += BN) {
        typename Tile::acc4 acc[4][4];
        mfma_zero<A>(acc);
        mfma_tile_product(
            t, As, Bs, d, acc,
            [&](int s, int, int k) { return (k < d && roff[s] >= 0) ? A(Elem<T>::to_acc(Z[roff[s] + k])) : A(0); },
            [&](int, int i, int k) {
                const int j = n0 + i;
                return (k < d && j < K) ? Cr[int64_t(j) * d + k] : A(0);
            });
        // a lane holds column n0 + wn + 16 ni + li of 16 rows; pad columns count as +inf: they are never taken
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int col = n0 + t.col(ni);
            if (col < K) {
                const A cc = cq[col];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) km_take(cc - A(2) * acc[mi][ni][reg], col, bv[mi][reg], bj[mi][reg]);
            }
        }
    }

    // the 16 lanes of one g share a row; then the two waves that share the rows meet in LDS
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            km_xor_step<8>(bv[mi][reg], bj[mi][reg]);
            km_xor_step<4>(bv[mi][reg], bj[mi][reg]);
            km_xor_step<2>(bv[mi][reg], bj[mi][reg]);
            km_xor_step<1>(bv[mi][reg], bj[mi][reg]);
            if (t.li == 0) {
                const int i = t.row(mi, reg);
                Sv[t.wn / 64][i] = bv[mi][reg];
                Sj[t.wn / 64][i] = bj[mi][reg];
            }
        }
    __syncthreads();
    if (tid < BM) {
        const int64_t r = m0 + tid;
        if (r < n) {
            A v = Sv[0][tid];
            int j = Sj[0][tid];
            km_take(Sv[1][tid], Sj[1][tid], v, j);
            assign[r * ld_assign + rst] = j < K ? j : 0;  // every value a NaN: centre 0, best stays +inf
            best[r * ld_best + rst] = v;
        }
    }
}

// ---- update ----------------------------------------------------------------------------------------------------
// Thread layout of a chunk's sum, the same whether the rows are read as 16-byte packs or element by element (so the
// table's alignment changes no bit): lpr = the row's packs rounded up to a power of two (at most kBlock) lanes side by
// side, S = kBlock / lpr row slots; a thread owns the VEC columns of pack `pass * lpr + tid % lpr`.
template <typename T>
__host__ __device__ __forceinline__ int km_lpr_log(int d) {
    const int packs = int(ceil_div(d, Elem<T>::kVec));
    int l = 0;
    while ((1 << l) < packs && (1 << l) < kBlock) ++l;
    return l;
}

// Workgroup b sums every chunk whose first row lies in positions [b kKmChunk, (b + 1) kKmChunk) of `order`: chunk c of
// segment s starts at seg[s] + c kKmChunk.  A segment of one chunk leaves its sum in centres_new[s] (kmeans_finish_kernel
// divides it); of a segment with more, at most two chunks start in one window -- a later chunk of a segment that began
// before the window (slot 0) and the first chunk of one that begins in it (slot 1): ws[(2 b + slot) d ...].
template <typename T, typename A, bool VECLOAD>
__global__ __launch_bounds__(kBlock) void kmeans_chunk_kernel(const T *__restrict__ Z, int64_t table_rows, int d,
                                                              int64_t ldz, const int32_t *__restrict__ order,
                                                              int64_t total, const int64_t *__restrict__ seg,
                                                              int64_t n_seg, int lpr_log, A *__restrict__ centres_new,
                                                              A *__restrict__ ws) {
    constexpr int VEC = Elem<T>::kVec;
    constexpr int U = kKmInFlight;
    __shared__ A red[kBlock * VEC];

    const int tid = threadIdx.x;
    const int lpr = 1 << lpr_log, S = kBlock >> lpr_log;
    const int cl = tid & (lpr - 1), slot = tid >> lpr_log;
    const int passes = int(ceil_div(ceil_div(d, VEC), lpr));
    const int64_t lo = int64_t(blockIdx.x) * kKmChunk;
    const int64_t hi = lo + kKmChunk < total ? lo + kKmChunk : total;

    int64_t a = 0, b = n_seg;                             // the first segment that ends beyond lo
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (seg[m + 1] > lo) b = m;
        else a = m + 1;
    }
    for (int64_t s = a; s < n_seg; ++s) {
        const int64_t beg = seg[s];
        int64_t end = seg[s + 1];
        if (beg >= hi) break;
        if (end > total) end = total;
        if (beg < 0 || end <= beg) continue;
        const int64_t start = beg >= lo ? beg : beg + ceil_div(lo - beg, int64_t(kKmChunk)) * kKmChunk;
        if (start >= end || start >= hi) continue;
        const int len = int(end - start < kKmChunk ? end - start : kKmChunk);
        const bool single = end - beg <= kKmChunk;
        A *__restrict__ out = single ? centres_new + s * d : ws + (2 * int64_t(blockIdx.x) + (start == beg ? 1 : 0)) * d;
        const int32_t *__restrict__ list = order + start;

        for (int pass = 0; pass < passes; ++pass) {
            const int c0 = (pass * lpr + cl) * VEC;
            A sum[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) sum[v] = A(0);
            if (c0 < d) {
                for (int i0 = slot; i0 < len; i0 += U * S) {
                    Pack<T, VEC> p[U];
                    bool ok[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {         // U rows in flight before the first is used
                        const int i = i0 + u * S;
                        int64_t t = -1;
                        if (i < len) {
                            t = list[i];
                            if (t >= table_rows) t = -1;
                        }
                        ok[u] = t >= 0;
                        if (ok[u]) {
                            const T *__restrict__ src = Z + t * ldz + c0;
                            if constexpr (VECLOAD) {
                                p[u] = load_pack<T, VEC>(src);
                            } else {
#pragma unroll
                                for (int v = 0; v < VEC; ++v)
                                    if (c0 + v < d) p[u].v[v] = src[v];
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (ok[u]) {
#pragma unroll
                            for (int v = 0; v < VEC; ++v)
                                if (c0 + v < d) sum[v] += A(Elem<T>::to_acc(p[u].v[v]));
                        }
                }
            }
            __syncthreads();                              // red is free again
#pragma unroll
            for (int v = 0; v < VEC; ++v) red[tid * VEC + v] = sum[v];
            __syncthreads();
            if (slot == 0 && c0 < d) {
                for (int q = 1; q < S; ++q)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) sum[v] += red[((q << lpr_log) + cl) * VEC + v];
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (c0 + v < d) out[c0 + v] = sum[v];
            }
        }
    }
}

// One workgroup per segment: the chunk sums in chunk order, ONE division by the count, and the new centre's squared norm
// (a thread's columns in ascending order, then the threads in order).  An empty segment keeps its old centre's bits.
template <typename A>
__global__ __launch_bounds__(kBlock) void kmeans_finish_kernel(const int64_t *__restrict__ seg, int64_t total, int d,
                                                               const A *__restrict__ centres_old, const A *__restrict__ ws,
                                                               A *__restrict__ centres_new, A *__restrict__ csq_new) {
    __shared__ A part[kBlock];
    const int64_t s = blockIdx.x;
    const int64_t beg = seg[s];
    int64_t end = seg[s + 1];
    if (end > total) end = total;
    const int64_t count = (beg < 0 || end <= beg) ? 0 : end - beg;
    const int64_t chunks = ceil_div(count, int64_t(kKmChunk));
    A sq = A(0);
    for (int c = threadIdx.x; c < d; c += kBlock) {
        A v;
        if (count == 0) {
            v = centres_old[s * d + c];
        } else {
            A sum;
            if (chunks == 1) {
                sum = centres_new[s * d + c];
            } else {
                sum = ws[(2 * (beg / kKmChunk) + 1) * d + c];
                for (int64_t k = 1; k < chunks; ++k) sum += ws[(2 * ((beg + k * kKmChunk) / kKmChunk)) * d + c];
            }
            v = sum / A(count);
        }
        centres_new[s * d + c] = v;
        sq += v * v;
    }
    part[threadIdx.x] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int m = d < kBlock ? d : kBlock;
        A t = part[0];
        for (int i = 1; i < m; ++i) t += part[i];
        csq_new[s] = t;
    }
}

}  // namespace clane
