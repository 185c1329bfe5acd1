// Exact t-SNE of rows of a table in two dimensions: the all-pairs squared distances on the matrix cores, the perplexity
// search, the joint probabilities, and the two kernels of a gradient-descent iteration.
//
// Reference being replaced: nothing in the reference -- the 2-D picture of an embedding is made on the host, by
// scikit-learn's TSNE(method="exact"), whose formulas these kernels follow (_binary_search_perplexity,
// _joint_probabilities, _kl_divergence, _gradient_descent).  A fit calls, in this order,
//
//   sqnorm + sqdist : D[i, j] = max(0, |a_i|^2 + |a_j|^2 - 2 a_i . a_j), a = z - mu formed in the operand loaders; the
//                     dots are mfma_tile_product's (mfma_tile.h).  Only the 128 x 128 tile pairs ti <= tj are computed:
//                     the workgroup writes D[i, j] and D[j, i] from ONE value, and the diagonal as 0.
//   affinities      : row i of D becomes p_{j|i} at the beta_i that gives the row the entropy ln(perplexity); one
//                     workgroup per row, the row streamed from memory (L2) on every step of the search.
//   symmetrize      : P = max((p_{j|i} + p_{i|j}) / 2n, 2.220446e-16) in place, 64 x 64 tile pairs through LDS, and one
//                     partial of sum p ln p (double) per tile pair.
//   forces          : per row the four sums of an iteration over P[i, :] (read once) and Y (through LDS).
//   step            : S = sum s_i, the gradient, scikit-learn's gains / momentum update, KL and the gradient norm; one
//                     workgroup.
//
// Orders: every sum's order is a function of n alone (never of the grid, the addresses or the vector width); there are no
// atomics: two calls give the same bits.
#pragma once

#include "content_pca.h"
#include "device_utils.h"
#include "mfma_tile.h"

namespace clane {

constexpr int kTsneMaxPoints = 65536;                 // CLANE_TSNE_MAX_POINTS: P [n, n] fp32 is 16 GiB there
constexpr int kTsneSearchSteps = 100;                 // scikit-learn's n_steps
constexpr double kTsneEntropyTol = 1e-5;              // scikit-learn's PERPLEXITY_TOLERANCE
constexpr float kTsneMinP = 2.220446e-16f;            // scikit-learn's MACHINE_EPSILON
constexpr int kTsneSymTile = 64;                      // symmetrize: a workgroup owns tiles (I, J) and (J, I)
constexpr int kTsneRowsPerWave = 4;                   // forces: rows of P a wave sums side by side
constexpr int kTsneRowsPerBlock = kTsneRowsPerWave * kWavesPerBlock;
constexpr int kTsneChunk = 2048;                      // forces: points of Y staged in LDS at a time (16 KiB)
constexpr int kTsneStepBlock = 1024;                  // step: threads of its one workgroup
constexpr int kTsneForceCols = 6;                     // F[i] = attr.x, attr.y, rep.x, rep.y, s, l
constexpr int kTsneForcesKL = 1;                      // CLANE_TSNE_FORCES_KL
constexpr int kTsneForcesCached = 2;                  // CLANE_TSNE_FORCES_CACHED

// Sum of `v` over the workgroup, in every thread: lane butterfly, then the waves in wave order.  smem: one double per
// wave.
__device__ __forceinline__ double tsne_block_sum(double v, double *smem) {
    v = group_sum<kWave>(v);
    if (lane_id() == 0) smem[threadIdx.x / kWave] = v;
    __syncthreads();
    double s = 0.0;
    const int nw = blockDim.x / kWave;
    for (int w = 0; w < nw; ++w) s += smem[w];
    __syncthreads();
    return s;
}

// ---- squared distances ---------------------------------------------------------------------------------------------
// sq[i] = sum_k a_ik^2 by one fmaf per k in k order, a = z - mu; a row outside the table is z = 0.
template <typename T>
__global__ __launch_bounds__(kBlock) void tsne_sqnorm_kernel(const T *__restrict__ Z, int64_t table_rows, int d,
                                                             int64_t ldz, const int32_t *__restrict__ rows, int64_t n,
                                                             const float *__restrict__ mu, float *__restrict__ sq) {
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t r = rows[i];
    const T *z = (r >= 0 && r < table_rows) ? Z + r * ldz : nullptr;
    float s = 0.f;
    for (int k = 0; k < d; ++k) {
        const float a = (z != nullptr ? Elem<T>::to_acc(z[k]) : 0.f) - mu[k];
        s = fmaf(a, a, s);
    }
    sq[i] = s;
}

// Tile pair (ti <= tj) of blockIdx.x: D[i, j] and D[j, i] of its elements; in a diagonal pair the element i < j writes
// both places and i == j writes 0.
template <typename T>
__global__ __launch_bounds__(kBlock, 2) void tsne_sqdist_kernel(const T *__restrict__ Z, int64_t table_rows, int d,
                                                                int64_t ldz, const int32_t *__restrict__ rows, int64_t n,
                                                                const float *__restrict__ mu,
                                                                const float *__restrict__ sq, float *__restrict__ D,
                                                                int n_tiles) {
    using Tile = MfmaTile<float, 4>;
    static_assert(Tile::BM == Tile::BN && Tile::PER_A == Tile::PER_B, "square tiles: a tile pair and its mirror");
    __shared__ __attribute__((aligned(16))) float As[Tile::BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) float Bs[Tile::BN * Tile::LD];

    const Tile t(threadIdx.x);
    int ti, tj;
    gram_tile_pair(int(blockIdx.x), n_tiles, ti, tj);
    const int64_t i0 = int64_t(ti) * Tile::BM, j0 = int64_t(tj) * Tile::BN;

    int64_t ra[Tile::PER_A], rb[Tile::PER_B];                // gathered rows of this thread's staging slots; < 0: z = 0
    mfma_gather_offsets(rows, i0, n, table_rows, ldz, ra);
    mfma_gather_offsets(rows, j0, n, table_rows, ldz, rb);

    typename Tile::acc4 acc[4][4];
    mfma_zero<float>(acc);
    mfma_tile_product(
        t, As, Bs, d, acc,
        [&](int s, int, int k) { return k < d ? (ra[s] >= 0 ? Elem<T>::to_acc(Z[ra[s] + k]) : 0.f) - mu[k] : 0.f; },
        [&](int s, int, int k) { return k < d ? (rb[s] >= 0 ? Elem<T>::to_acc(Z[rb[s] + k]) : 0.f) - mu[k] : 0.f; });

    const bool diag = ti == tj;
    mfma_for_each(t, acc, [&](int r, int c, float dot) {
        const int64_t i = i0 + r, j = j0 + c;
        if (i >= n || j >= n || (diag && i > j)) return;
        float v = 0.f;
        if (i != j) v = fmaxf((sq[i] + sq[j]) - 2.f * dot, 0.f);
        D[i * n + j] = v;
        if (i != j) D[j * n + i] = v;
    });
}

// ---- conditional affinities ----------------------------------------------------------------------------------------
// Row blockIdx.x, in place.  Thread t takes j = t, t + 256, .. in j order (fp32 partials), the 256 partials are added in
// double by tsne_block_sum; every thread then takes the same step of the search on the same two sums.
__global__ __launch_bounds__(kBlock) void tsne_affinities_kernel(float *__restrict__ D, int64_t n, float perplexity,
                                                                 float *__restrict__ beta_out) {
    __shared__ double red[kWavesPerBlock];
    __shared__ float redf[kWavesPerBlock];
    const int64_t i = blockIdx.x;
    float *__restrict__ row = D + i * n;
    const int tid = threadIdx.x;

    float m = -__builtin_huge_valf();                        // max of -D over j != i
    for (int64_t j = tid; j < n; j += kBlock)
        if (j != i) m = fmaxf(m, -row[j]);
    m = group_max<kWave>(m);
    if (lane_id() == 0) redf[tid / kWave] = m;
    __syncthreads();
    m = redf[0];
    for (int w = 1; w < kWavesPerBlock; ++w) m = fmaxf(m, redf[w]);
    const float dmin = -m;

    const double target = log(double(perplexity));
    const float inf = __builtin_huge_valf();
    float beta = 1.f, beta_min = -inf, beta_max = inf;
    double sum_p = 1.0;
    for (int step = 0; step < kTsneSearchSteps; ++step) {
        float sp = 0.f, sdp = 0.f;
        for (int64_t j = tid; j < n; j += kBlock)
            if (j != i) {
                const float dd = row[j] - dmin;
                const float e = expf(-beta * dd);
                sp += e;
                sdp = fmaf(dd, e, sdp);
            }
        sum_p = tsne_block_sum(double(sp), red);
        const double sum_dp = tsne_block_sum(double(sdp), red);
        const double diff = log(sum_p) + double(beta) * sum_dp / sum_p - target;
        if (fabs(diff) <= kTsneEntropyTol || step == kTsneSearchSteps - 1) break;
        if (diff > 0.0) {
            beta_min = beta;
            beta = beta_max == inf ? beta * 2.f : (beta + beta_max) * 0.5f;
        } else {
            beta_max = beta;
            beta = beta_min == -inf ? beta * 0.5f : (beta + beta_min) * 0.5f;
        }
    }
    // the row at the beta the sums above were taken at: the same exponentials, divided by their sum
    const float denom = float(sum_p);
    for (int64_t j = tid; j < n; j += kBlock) row[j] = j == i ? 0.f : expf(-beta * (row[j] - dmin)) / denom;
    if (tid == 0) beta_out[i] = beta;
}

// ---- joint probabilities -------------------------------------------------------------------------------------------
// Tile pair (ti <= tj) of 64 x 64 tiles: both tiles into LDS, then both written.  (a + b) is one fp32 add of the two
// conditionals and commutes, so P[i, j] and P[j, i] get the same bits.  partials[pair] = sum over the pair's elements of
// p ln p in double: thread t adds its elements e = t, t + 256, .. of the tile in e order, tsne_block_sum adds the
// threads, an off-diagonal pair counts twice.
__global__ __launch_bounds__(kBlock) void tsne_symmetrize_kernel(float *__restrict__ P, int64_t n, int n_tiles,
                                                                 double *__restrict__ partials) {
    constexpr int TS = kTsneSymTile;
    __shared__ float A[TS][TS + 1];
    __shared__ float B[TS][TS + 1];
    __shared__ double red[kWavesPerBlock];
    int ti, tj;
    gram_tile_pair(int(blockIdx.x), n_tiles, ti, tj);
    const int64_t r0 = int64_t(ti) * TS, c0 = int64_t(tj) * TS;
    const bool diag = ti == tj;
    for (int e = threadIdx.x; e < TS * TS; e += kBlock) {
        const int r = e / TS, c = e % TS;
        A[r][c] = (r0 + r < n && c0 + c < n) ? P[(r0 + r) * n + c0 + c] : 0.f;
        if (!diag) B[r][c] = (c0 + r < n && r0 + c < n) ? P[(c0 + r) * n + r0 + c] : 0.f;
    }
    __syncthreads();
    const float two_n = float(2 * n);
    double acc = 0.0;
    for (int e = threadIdx.x; e < TS * TS; e += kBlock) {
        const int r = e / TS, c = e % TS;
        const int64_t i = r0 + r, j = c0 + c;
        if (i < n && j < n) {
            const float v = i == j ? 0.f : fmaxf((A[r][c] + (diag ? A[c][r] : B[c][r])) / two_n, kTsneMinP);
            P[i * n + j] = v;
            if (i != j) acc += double(v) * log(double(v));
        }
        if (!diag && c0 + r < n && r0 + c < n)               // element (r, c) of the mirrored tile (tj, ti)
            P[(c0 + r) * n + r0 + c] = fmaxf((B[r][c] + A[c][r]) / two_n, kTsneMinP);
    }
    const double s = tsne_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = diag ? s : 2.0 * s;
}

// ---- forces ----------------------------------------------------------------------------------------------------------
// A workgroup owns 16 consecutive rows, each wave 4 of them.  Y goes through LDS kTsneChunk points at a time; lane l of a
// wave takes the columns c0 + 4 l + 256 m + u (u = 0..3) of every chunk in that order into fp32 partials, the 64 lanes
// are added by the xor butterfly: the order of a row's terms depends on n alone.  VEC: P's rows are 16-byte aligned (n a
// multiple of 4) and a lane's four columns are one load; NT: that load is non-temporal (P is read once per iteration and
// is far larger than the caches; Y is re-read by every workgroup and should stay in them).
// Registers: 158, three waves per SIMD; held to 128 (four waves) the compiler spills 27 of them to scratch.
template <bool VEC, bool NT>
__global__ __launch_bounds__(kBlock) void tsne_forces_kernel(const float *__restrict__ P, const float *__restrict__ Y,
                                                             int64_t n, int want_l, float *__restrict__ F) {
    constexpr int RW = kTsneRowsPerWave;
    __shared__ __attribute__((aligned(16))) float Ys[2 * kTsneChunk];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int64_t r0 = int64_t(blockIdx.x) * kTsneRowsPerBlock + (tid / kWave) * RW;

    float yi[RW][2], acc[RW][kTsneForceCols];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const bool ok = r0 + r < n;
        yi[r][0] = ok ? Y[2 * (r0 + r)] : 0.f;
        yi[r][1] = ok ? Y[2 * (r0 + r) + 1] : 0.f;
#pragma unroll
        for (int c = 0; c < kTsneForceCols; ++c) acc[r][c] = 0.f;
    }

    for (int64_t c0 = 0; c0 < n; c0 += kTsneChunk) {
        __syncthreads();                                      // the previous chunk has been read by every wave
        for (int e = tid; e < 2 * kTsneChunk; e += kBlock) Ys[e] = 2 * c0 + e < 2 * n ? Y[2 * c0 + e] : 0.f;
        __syncthreads();
        if (r0 >= n) continue;                                // a wave without rows only helps staging
        const int cn = int(n - c0 < kTsneChunk ? n - c0 : kTsneChunk);
        for (int jj = 4 * lane; jj < cn; jj += 4 * kWave) {
            float yx[4], yy[4], p[RW][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                yx[u] = Ys[2 * (jj + u)];
                yy[u] = Ys[2 * (jj + u) + 1];
            }
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const int64_t i = r0 + r;
#pragma unroll
                for (int u = 0; u < 4; ++u) p[r][u] = 0.f;
                if (i < n) {
                    const float *src = P + i * n + c0 + jj;
                    if constexpr (VEC) {
                        const Pack<float, 4> v = NT ? load_pack_stream<float, 4>(src) : load_pack<float, 4>(src);
#pragma unroll
                        for (int u = 0; u < 4; ++u) p[r][u] = v.v[u];
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (jj + u < cn) p[r][u] = NT ? __builtin_nontemporal_load(src + u) : src[u];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t j = c0 + jj + u;
                const bool valid = jj + u < cn;
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    const float dx = yi[r][0] - yx[u], dy = yi[r][1] - yy[u];
                    const float d2 = fmaf(dx, dx, dy * dy);
                    const float q = valid ? __builtin_amdgcn_rcpf(1.f + d2) : 0.f;
                    const float pq = p[r][u] * q, qq = q * q;
                    acc[r][0] = fmaf(pq, dx, acc[r][0]);
                    acc[r][1] = fmaf(pq, dy, acc[r][1]);
                    acc[r][2] = fmaf(qq, dx, acc[r][2]);
                    acc[r][3] = fmaf(qq, dy, acc[r][3]);
                    acc[r][4] += j == r0 + r ? 0.f : q;
                    if (want_l) acc[r][5] = fmaf(p[r][u], log1pf(d2), acc[r][5]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int c = 0; c < kTsneForceCols; ++c) {
            const float v = group_sum<kWave>(acc[r][c]);
            if (lane == 0 && r0 + r < n) F[(r0 + r) * kTsneForceCols + c] = v;
        }
}

// ---- the update --------------------------------------------------------------------------------------------------------
// One workgroup of kTsneStepBlock threads; thread t takes the points t, t + 1024, .. in that order, tsne_block_sum adds
// the threads.  S, the gradient and the update are formed in double from the fp32 force sums and stored as fp32.
// stats: KL, |g|, S, sum l_i.
__global__ __launch_bounds__(kTsneStepBlock) void tsne_step_kernel(const float *__restrict__ F,
                                                                   const float *__restrict__ Y, int64_t n, double alpha,
                                                                   double momentum, double lr, double plogp,
                                                                   float *__restrict__ V, float *__restrict__ G,
                                                                   float *__restrict__ Yn, double *__restrict__ stats) {
    __shared__ double red[kTsneStepBlock / kWave];
    double s = 0.0, l = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kTsneStepBlock) {
        s += double(F[i * kTsneForceCols + 4]);
        l += double(F[i * kTsneForceCols + 5]);
    }
    const double S = tsne_block_sum(s, red);
    const double L = tsne_block_sum(l, red);
    double g2 = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kTsneStepBlock)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double g = 4.0 * (alpha * double(F[i * kTsneForceCols + c]) - double(F[i * kTsneForceCols + 2 + c]) / S);
            const double v = double(V[2 * i + c]);
            double gain = double(G[2 * i + c]);
            gain = v * g < 0.0 ? gain + 0.2 : gain * 0.8;
            if (gain < 0.01) gain = 0.01;
            const float vn = float(momentum * v - lr * gain * g);
            G[2 * i + c] = float(gain);
            V[2 * i + c] = vn;
            Yn[2 * i + c] = Y[2 * i + c] + vn;
            g2 += g * g;
        }
    const double G2 = tsne_block_sum(g2, red);
    if (threadIdx.x == 0) {
        stats[0] = plogp + L + log(S);
        stats[1] = sqrt(G2);
        stats[2] = S;
        stats[3] = L;
    }
}

}  // namespace clane
