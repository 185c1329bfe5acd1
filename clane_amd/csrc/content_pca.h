// Content reduction (PCA) on rows of a table: deterministic column sums, the centred Gram on the matrix cores and an
// affine row projection.
//
// Reference being replaced: nothing in the reference -- its users run a host PCA on C.npy before the graph is loaded
// (the README's Cora experiment has 1433 bag-of-words columns).  Here the three device passes of a PCA are
//
//   column_sums    : sums[c] = sum_i Z[rows[i], c] in double, rows in chunks of kGradChunk, one partial per (chunk,
//                    column), the chunks added in chunk order.
//   gram           : G = sum_i (z_i - mu)(z_i - mu)^T -- probe_grad_kernel's scheme (label_probe.h) with BOTH operands
//                    the gathered row, centred while it is staged; only the tile pairs ti <= tj are computed, the
//                    reduce over the chunks writes the mirrored element.
//   project_affine : Y[i, :] = W (z_rows[i] - mu) -- project_rows_kernel's contraction (projection.h) with gathered
//                    rows and the centring in the A-operand loader; rounded once to the table type.
//
// The contraction is mfma_tile.h's: a (row, column) element's k terms run in mfma_slice's order, inside a chunk for the
// Gram.  So on the same operands G has the bits of probe_grad_kernel given the centred rows as its G and as its table,
// K = d, and Y those of project_rows_kernel on the centred table.  No atomics: two calls give the same bits.
//
// A `rows` entry outside [0, table_rows) is an absent row: nothing is read for it, it adds nothing to the sums or the
// Gram, and its Y row is zeros.  Columns [d, ldz) are never read.
#pragma once

#include "device_utils.h"
#include "mfma_tile.h"
#include "pair_train.h"

namespace clane {

constexpr int kPcaAccumulate = 1;      // CLANE_PCA_ACCUMULATE
constexpr int kSumRowLanes = 16;       // threads that share a column of a chunk: thread rl takes rows rl, rl + 16, ...
constexpr int kSumColLanes = kBlock / kSumRowLanes;
constexpr int kSumInFlight = 4;        // row groups loaded before the first is used (stream_rows of a 64-lane row)

// ---- column sums -----------------------------------------------------------------------------------------------
// blockIdx = (column strip of kSumColLanes * VEC columns, chunk).  Thread (rl, cl) owns VEC columns of the strip: one
// 16-byte pack at cl * VEC (PACKED: Z and ldz are 16-byte aligned), else the elements cl + 16 v.  It adds its rows in
// row order, kSumInFlight of them loaded at a time; the 16 threads of a column are then added in rl order.  Which
// thread owns a column does not enter the order of a column's sum, so both layouts give the same bits.
// ws [chunks, d].
template <typename T, int VEC, bool PACKED>
__global__ __launch_bounds__(kBlock) void column_sums_kernel(const T *__restrict__ Z, int64_t table_rows, int d,
                                                             int64_t ldz, const int32_t *__restrict__ rows, int64_t n,
                                                             double *__restrict__ ws) {
    __shared__ double Ss[kSumRowLanes][kSumColLanes * VEC + 1];
    const int rl = int(threadIdx.x) / kSumColLanes, cl = int(threadIdx.x) % kSumColLanes;
    const int c0 = int(blockIdx.x) * (kSumColLanes * VEC);
    const int64_t kbeg = int64_t(blockIdx.y) * kGradChunk;
    const int64_t kend = kbeg + kGradChunk < n ? kbeg + kGradChunk : n;
    auto col = [&](int v) { return PACKED ? c0 + cl * VEC + v : c0 + cl + kSumColLanes * v; };
    const bool whole = PACKED && c0 + cl * VEC + VEC <= d;      // the pack lies inside [0, d): one 16-byte load

    double s[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) s[v] = 0.0;
    for (int64_t k0 = kbeg + rl; k0 < kend; k0 += kSumRowLanes * kSumInFlight) {
        Pack<T, VEC> z[kSumInFlight];
        bool have[kSumInFlight];
#pragma unroll
        for (int j = 0; j < kSumInFlight; ++j) {
            const int64_t k = k0 + j * kSumRowLanes;
            int64_t r = -1;
            if (k < kend) {
                r = rows[k];
                if (r >= table_rows) r = -1;
            }
            have[j] = r >= 0;
            z[j] = Pack<T, VEC>{};
            if (have[j]) {
                const T *p = Z + r * ldz;
                if (whole) {
                    z[j] = load_pack_stream<T, VEC>(p + c0 + cl * VEC);
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v)
                        if (col(v) < d) z[j].v[v] = p[col(v)];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kSumInFlight; ++j)
            if (have[j]) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) s[v] += double(Elem<T>::to_acc(z[j].v[v]));
            }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) Ss[rl][PACKED ? cl * VEC + v : cl + kSumColLanes * v] = s[v];
    __syncthreads();
    for (int j = int(threadIdx.x); j < kSumColLanes * VEC; j += kBlock) {
        if (c0 + j >= d) continue;
        double t = Ss[0][j];
#pragma unroll
        for (int r = 1; r < kSumRowLanes; ++r) t += Ss[r][j];
        ws[int64_t(blockIdx.y) * d + c0 + j] = t;
    }
}

// sums[c] = (accumulate ? sums[c] : 0) + the chunks' partials in chunk order.
__global__ __launch_bounds__(kBlock) void column_sums_reduce_kernel(const double *__restrict__ ws, int64_t n_chunks,
                                                                    int d, int accumulate, double *__restrict__ sums) {
    const int c = int(blockIdx.x) * kBlock + threadIdx.x;
    if (c >= d) return;
    double s = accumulate ? sums[c] : 0.0;
    for (int64_t z = 0; z < n_chunks; ++z) s += ws[z * d + c];
    sums[c] = s;
}

// ---- centred Gram ----------------------------------------------------------------------------------------------
// Tile pair p of the upper triangle, rows of pairs in turn: (0, 0) .. (0, nt - 1), (1, 1) .. -- uniform, nt steps.
__device__ __forceinline__ void gram_tile_pair(int p, int nt, int &ti, int &tj) {
    ti = 0;
    while (p >= nt - ti) {
        p -= nt - ti;
        ++ti;
    }
    tj = ti + p;
}

// Partial Gram of one chunk of rows: out[o, c] = sum_i (Z[rows[i], o] - mu[o]) (Z[rows[i], c] - mu[c]) for the tile
// pair (ti <= tj) of blockIdx.x and the chunk of blockIdx.y, into ws + chunk * d * d (a [d, d] matrix of which only the
// upper tile pairs are written).  probe_grad_kernel with the A operand gathered like the B operand.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void gram_kernel(const T *__restrict__ Z, int64_t table_rows, int d, int64_t ldz,
                                                      const int32_t *__restrict__ rows, int64_t n,
                                                      const A *__restrict__ mu, A *__restrict__ ws, int n_tiles) {
    using Tile = MfmaTile<A, 4>;
    static_assert(kGradChunk % Tile::BK == 0, "a chunk is whole slices");
    static_assert(Tile::BM == Tile::BN, "square tiles: a tile pair and its mirror");
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];
    __shared__ int32_t Rs[kGradChunk];

    const Tile t(threadIdx.x);
    int ti, tj;
    gram_tile_pair(int(blockIdx.x), n_tiles, ti, tj);
    const int o0 = ti * Tile::BM, i0 = tj * Tile::BN;
    const int64_t kbeg = int64_t(blockIdx.y) * kGradChunk;
    const int64_t kend = kbeg + kGradChunk < n ? kbeg + kGradChunk : n;

    const int so = int(threadIdx.x) % Tile::BM;              // the staged column of either operand
    const bool o_ok = o0 + so < d, i_ok = i0 + so < d, diag = ti == tj;
    const A mo = (mu != nullptr && o_ok) ? mu[o0 + so] : A(0), mi = (mu != nullptr && i_ok) ? mu[i0 + so] : A(0);

    // The chunk's table rows, once, into LDS (-1: absent): a slice's fetch then starts from an LDS read, not from a
    // global load whose latency would stand in front of every slice's element loads.
    for (int i = int(threadIdx.x); i < kGradChunk; i += kBlock) {
        int32_t r = -1;
        if (kbeg + i < kend) {
            r = rows[kbeg + i];
            if (r >= table_rows) r = -1;
        }
        Rs[i] = r;
    }
    __syncthreads();

    typename Tile::acc4 acc[4][4];
    mfma_zero<A>(acc);
    mfma_tile_product_transposed(
        t, As, Bs, kbeg, kend, acc,
        [&](int64_t k, A &a, A &b) {
            const int32_t r = Rs[int(k - kbeg)];
            if (r < 0) return;
            const T *z = Z + int64_t(r) * ldz;
            if (o_ok) a = A(Elem<T>::to_acc(z[o0 + so])) - mo;
            if (diag) b = a;
            else if (i_ok) b = A(Elem<T>::to_acc(z[i0 + so])) - mi;
        },
        [](A) {});

    A *__restrict__ out = ws + int64_t(blockIdx.y) * d * int64_t(d);
    mfma_for_each(t, acc, [&](int r, int c, A v) {
        const int o = o0 + r, i = i0 + c;
        if (o < d && i < d) out[int64_t(o) * d + i] = v;
    });
}

// G[i, j] = (accumulate ? G[i, j] : 0) + the chunks' partials in chunk order, for every element of an upper tile pair;
// an element of an off-diagonal pair is also written to G[j, i].
template <typename A>
__global__ __launch_bounds__(kBlock) void gram_reduce_kernel(const A *__restrict__ ws, int64_t n_chunks, int d,
                                                             int accumulate, A *__restrict__ G) {
    const int64_t len = int64_t(d) * d;
    const int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= len) return;
    const int i = int(e / d), j = int(e % d);
    const int ti = i / kProjBM, tj = j / kProjBN;
    if (ti > tj) return;
    A s = accumulate ? G[e] : A(0);
    for (int64_t c = 0; c < n_chunks; ++c) s += ws[c * len + e];
    G[e] = s;
    if (ti != tj) G[int64_t(j) * d + i] = s;
}

// ---- affine projection -----------------------------------------------------------------------------------------
// Y[i, 0:m) (ld ldy, table type) = W[m, d] (z_rows[i] - mu).  Block b: column tile b % n_tiles of row tile b / n_tiles.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void project_affine_kernel(const T *__restrict__ Z, int64_t table_rows, int d,
                                                                int64_t ldz, const int32_t *__restrict__ rows, int64_t n,
                                                                const A *__restrict__ mu, const A *__restrict__ W, int m,
                                                                T *__restrict__ Y, int64_t ldy, int n_tiles) {
    using Tile = MfmaTile<A, 4>;
    __shared__ __attribute__((aligned(16))) A As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) A Bs[Tile::BN * Tile::LD];

    const Tile t(threadIdx.x);
    const int64_t tile = blockIdx.x;
    const int n0 = int(tile % n_tiles) * Tile::BN;
    const int64_t m0 = (tile / n_tiles) * Tile::BM;

    int64_t roff[Tile::PER_A];                               // gathered rows of this thread's staging slots; < 0: none
    mfma_gather_offsets(rows, m0, n, table_rows, ldz, roff);

    typename Tile::acc4 acc[4][4];
    mfma_zero<A>(acc);
    mfma_tile_product(
        t, As, Bs, d, acc,
        [&](int s, int, int k) {
            if (!(k < d && roff[s] >= 0)) return A(0);
            const A x = A(Elem<T>::to_acc(Z[roff[s] + k]));
            return mu != nullptr ? x - mu[k] : x;
        },
        [&](int, int i, int k) {
            const int j = n0 + i;
            return (k < d && j < m) ? W[int64_t(j) * d + k] : A(0);
        });

    mfma_for_each(t, acc, [&](int i, int j, A v) {
        const int64_t r = m0 + i;
        const int col = n0 + j;
        if (r < n && col < m) Y[r * ldy + col] = Elem<T>::from_acc(v);
    });
}

}  // namespace clane
