// Neighbour-sparse t-SNE: P kept on each point's k nearest neighbours, the repulsion exact.  What tsne.h does with
// P [n, n] in memory stops at 65 536 points; here nothing is n x n:
//
//   knn_sqdist      : for every listed row its k nearest other listed rows.  tsne_sqdist_kernel's distances --
//                     max(0, (sq[i] + sq[j]) - 2 dot), a = z - mu formed in the operand loaders, the dot from
//                     mfma_tile_product in mfma_slice's k order: a neighbour's distance is the bits of the exact path's
//                     D[i, j] -- with the selection fused as in rank_scores_kernel (link_rank.h): a workgroup owns a tile
//                     of queries and a slab of candidate tiles and keeps every query's sorted list in LDS; the n x n
//                     distances never exist.  knn_merge_kernel combines the slabs.
//   nn_affinities   : tsne_affinities_kernel's perplexity search over a row's k distances, one wave per row.
//   (joint)         : the union of the neighbour pairs, sorted into CSR, is torch plumbing (layout.py); nn_plogp gives
//                     sum p ln p of every CSR row.
//   nn_attract      : per CSR row the attraction sums and sum p log1p(d^2): columns 0, 1, 5 of F [n, 6].
//   repulse         : the exact all-pairs repulsion sums and s_i = sum_{j != i} q: columns 2, 3, 4 of F; Y through LDS,
//                     P not read.  The cost of an iteration.
//   step            : tsne_step_kernel (tsne.h), unchanged: it only reads F.
//
// Orders: every sum's order is a function of n (and of k, or of the CSR) alone; no atomics: two calls give the same bits.
// The order of a neighbour list is total -- distance ascending, ties by position ascending, the row itself excluded --
// so the merged lists do not depend on n_slabs.
#pragma once

#include "device_utils.h"
#include "mfma_tile.h"
#include "tsne.h"

namespace clane {

constexpr int kKnnMaxK = 192;                         // CLANE_KNN_MAX_K: 3 x perplexity up to 64
constexpr int kTsneNnMaxPoints = 1 << 20;             // CLANE_TSNE_NN_MAX_POINTS
constexpr int kKnnEmpty = 0x7fffffff;                 // an empty place of a list in LDS: (+inf, kKnnEmpty) sorts last
constexpr int kNnRowsPerBlock = kWavesPerBlock;       // affinities, plogp, attract: one wave per row
constexpr int kRepulseRowsPerWave = 4;                // repulse: rows a wave sums side by side from one LDS read
constexpr int kRepulseRowsPerBlock = kRepulseRowsPerWave * kWavesPerBlock;

// (s, l) comes before (ps, pl) in a neighbour list
__device__ __forceinline__ bool knn_before(float s, int l, float ps, int pl) { return s < ps || (s == ps && l < pl); }

// The 16 lanes of a query row's group put (s, pos) into the row's sorted list sc / id of k places together, if it comes
// before the last one: lane l owns the places l, l + 16, .. (PL of them at most), reads each with the place before it, and
// then writes what the place holds after the insertion -- the old entry, the new one, or the entry that was one place
// ahead.  Every read is issued before any write (one wave, program order), so no lane sees a half-shifted list.
template <int PL>
__device__ __forceinline__ void knn_group_insert(volatile float *sc, volatile int *id, int k, float s, int pos, int l) {
    if (!knn_before(s, pos, sc[k - 1], id[k - 1])) return;
    float d0[PL], dp[PL];
    int i0[PL], ip[PL];
#pragma unroll
    for (int u = 0; u < PL; ++u) {
        const int j = l + 16 * u;
        d0[u] = dp[u] = 0.f;
        i0[u] = ip[u] = 0;
        if (j < k) {
            d0[u] = sc[j];
            i0[u] = id[j];
            if (j > 0) {
                dp[u] = sc[j - 1];
                ip[u] = id[j - 1];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < PL; ++u) {
        const int j = l + 16 * u;
        if (j < k) {
            float nd = d0[u];
            int ni = i0[u];
            if (j > 0 && knn_before(s, pos, dp[u], ip[u])) {    // the new entry goes in further ahead: one place back
                nd = dp[u];
                ni = ip[u];
            } else if (knn_before(s, pos, d0[u], i0[u])) {      // ... goes in here
                nd = s;
                ni = pos;
            }
            if (ni != i0[u]) {                                   // (an empty place moved onto an empty place: the same)
                sc[j] = nd;
                id[j] = ni;
            }
        }
    }
}

// The query tile: the lists (32 MI x k places of 8 bytes, dynamic LDS) and the staged slices (static) of a workgroup stay
// within the 64 KiB a workgroup has without asking for more: 128 queries up to k = 40, 64 up to 96, 32 up to 192.
constexpr int knn_tile_mi(int k) { return k <= 40 ? 4 : k <= 96 ? 2 : 1; }
constexpr int knn_places_per_lane(int mi) { return mi == 4 ? 3 : mi == 2 ? 6 : kKnnMaxK / 16; }    // ceil(k / 16) at most
static_assert(knn_places_per_lane(4) * 16 >= 40 && knn_places_per_lane(2) * 16 >= 96, "a lane's places cover the list");
constexpr size_t knn_list_bytes(int mi, int k) { return size_t(32 * mi) * k * (sizeof(float) + sizeof(int)); }
constexpr size_t knn_static_bytes(int mi) {
    return (size_t(32 * mi) + kProjBN) * (kProjBK + 4) * sizeof(float) + size_t(32 * mi) * sizeof(float);
}
static_assert(knn_list_bytes(4, 40) + knn_static_bytes(4) <= 65536 && knn_list_bytes(2, 96) + knn_static_bytes(2) <= 65536 &&
                  knn_list_bytes(1, kKnnMaxK) + knn_static_bytes(1) <= 65536,
              "lists + staging pass the LDS of a workgroup");

// blockIdx.x = slab * q_tiles + query tile.  Slab s holds the candidate tiles [s * tiles_per_slab, (s + 1) *
// tiles_per_slab) of 128 positions of the row list -- none at all when n_slabs is more than there are tiles; such a
// workgroup only writes its empty lists.  Selection as in rank_scores_kernel: a threshold compare with the query's k-th
// distance first; survivors go into the list one at a time -- the two waves that share the query rows take turns (a barrier
// between), inside a wave the candidates of the 16 lanes of one query row go one by one, each put in place by the 16 lanes
// together (knn_group_insert; the four row groups of a wave work on different queries side by side).
// Registers (hipcc 6.x, gfx950): see DESIGN 6.18; the bound of 2 waves per SIMD is the one LDS allows at MI = 1, 2.
template <typename T, int MI>
__global__ __launch_bounds__(kBlock, 2) void knn_sqdist_kernel(const T *__restrict__ Z, int64_t table_rows, int d,
                                                               int64_t ldz, const int32_t *__restrict__ rows, int64_t n,
                                                               const float *__restrict__ mu,
                                                               const float *__restrict__ sq, int k, int n_slabs,
                                                               int64_t q_tiles, int64_t tiles_per_slab,
                                                               float *__restrict__ cand_d, int32_t *__restrict__ cand_id) {
    using Tile = MfmaTile<float, MI>;
    using M = typename Tile::M;
    constexpr int BM = Tile::BM, BN = Tile::BN;
    __shared__ __attribute__((aligned(16))) float As[BM * Tile::LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * Tile::LD];
    __shared__ float s_sq[BM];                               // |a|^2 of the tile's queries
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_dyn[];
    volatile float *l_d = reinterpret_cast<volatile float *>(knn_dyn);
    volatile int *l_id = reinterpret_cast<volatile int *>(knn_dyn + size_t(BM) * k * sizeof(float));

    const Tile t(threadIdx.x);
    const int tid = threadIdx.x, wave = tid / kWave;
    const int64_t slab = blockIdx.x / q_tiles;
    const int64_t m0 = (blockIdx.x % q_tiles) * BM;
    const int64_t tiles_total = ceil_div(n, int64_t(BN));
    const int64_t t0 = slab * tiles_per_slab < tiles_total ? slab * tiles_per_slab : tiles_total;
    const int64_t t1 = t0 + tiles_per_slab < tiles_total ? t0 + tiles_per_slab : tiles_total;

    for (int i = tid; i < BM * k; i += kBlock) {
        l_d[i] = __builtin_huge_valf();
        l_id[i] = kKnnEmpty;
    }
    for (int i = tid; i < BM; i += kBlock) s_sq[i] = m0 + i < n ? sq[m0 + i] : 0.f;

    int64_t ra[Tile::PER_A];                                 // gathered rows of the staging slots; < 0: z = 0
    mfma_gather_offsets(rows, m0, n, table_rows, ldz, ra);

    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t n0 = tile * BN;
        int64_t rb[Tile::PER_B];
        mfma_gather_offsets(rows, n0, n, table_rows, ldz, rb);
        float csq[4];                                        // the tile's column norms: requested now, used after the MFMAs
        bool col_ok[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int64_t v = n0 + t.col(ni);
            col_ok[ni] = v < n;
            csq[ni] = col_ok[ni] ? sq[v] : 0.f;
        }
        typename Tile::acc4 acc[MI][4];
        mfma_zero<float>(acc);
        mfma_tile_product(
            t, As, Bs, d, acc,
            [&](int s, int, int kk) { return kk < d ? (ra[s] >= 0 ? Elem<T>::to_acc(Z[ra[s] + kk]) : 0.f) - mu[kk] : 0.f; },
            [&](int s, int, int kk) { return kk < d ? (rb[s] >= 0 ? Elem<T>::to_acc(Z[rb[s] + kk]) : 0.f) - mu[kk] : 0.f; });

        // ---- selection: the waves of the first column half, a barrier, those of the second
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {
            int kq = k, lq = t.lane;                          // opaque copies, as in rank_scores_kernel
            asm volatile("" : "+s"(kq), "+v"(lq));
            if ((wave >> 1) == half) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int ql = t.wm + 16 * mi + M::row(lq, reg);
                        const int64_t qpos = m0 + ql;
                        const float thr = l_d[ql * kq + kq - 1];
                        const float sqq = s_sq[ql];
                        float dd[4];
                        bool pass[4], mine = false;
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni) {
                            dd[ni] = fmaxf((sqq + csq[ni]) - 2.f * acc[mi][ni][reg], 0.f);
                            pass[ni] = col_ok[ni] && dd[ni] <= thr && qpos < n && n0 + t.wn + 16 * ni + (lq & 15) != qpos;
                            mine = mine || pass[ni];
                        }
                        if (!__any(mine)) continue;           // wave-uniform: the common case after the first tiles
                        const unsigned long long m = __ballot(mine);
                        unsigned turns = unsigned((m | (m >> 16) | (m >> 32) | (m >> 48)) & 0xffffu);
                        while (turns) {                       // the candidates of one lane of each 16-lane row group at a time
                            const int src = (lq & 48) | (__ffs(turns) - 1);
                            turns &= turns - 1;
#pragma unroll 1
                            for (int c = 0; c < 4; ++c) {     // one copy of the insertion: the values by select
                                const bool pc = c == 0 ? pass[0] : c == 1 ? pass[1] : c == 2 ? pass[2] : pass[3];
                                const float dv = c == 0 ? dd[0] : c == 1 ? dd[1] : c == 2 ? dd[2] : dd[3];
                                const int has = __shfl(int(pc), src, kWave);
                                const float cd = __shfl(dv, src, kWave);
                                const int cp = int(n0) + t.wn + 16 * c + (src & 15);
                                if (has) knn_group_insert<knn_places_per_lane(MI)>(l_d + ql * kq, l_id + ql * kq, kq, cd, cp, lq & 15);
                            }
                        }
                    }
            }
            if (half == 0) __syncthreads();
        }
    }

    __syncthreads();
    for (int i = tid; i < BM * k; i += kBlock) {
        const int64_t qi = m0 + i / k;
        if (qi < n) {
            const int64_t o = (qi * n_slabs + slab) * k + i % k;
            const int id = l_id[i];
            cand_d[o] = l_d[i];
            cand_id[o] = id == kKnnEmpty ? -1 : id;
        }
    }
}

// One wave per query: k rounds, each the first candidate that comes after the one emitted before it.  The order is
// total (a position occurs once among a query's candidates), so the result depends on the SET of candidates alone.  Lane
// l looks at the places l, l + 64, .. of the query's n_slabs * k candidates; places past the candidates: (+inf, -1).
__global__ __launch_bounds__(kBlock) void knn_merge_kernel(const float *__restrict__ cand_d,
                                                           const int32_t *__restrict__ cand_id, int64_t n, int n_slabs,
                                                           int k, float *__restrict__ out_d, int32_t *__restrict__ out_id) {
    const int lane = lane_id();
    const int64_t q = int64_t(blockIdx.x) * kWavesPerBlock + threadIdx.x / kWave;
    if (q >= n) return;                                       // wave-uniform; no barrier below
    const int64_t nc = int64_t(n_slabs) * k;
    const float *__restrict__ cs = cand_d + q * nc;
    const int32_t *__restrict__ ci = cand_id + q * nc;
    float ps = 0.f;
    int pl = -1;                                              // < 0: nothing emitted yet
    bool done = false;
    for (int r = 0; r < k; ++r) {
        float bs = __builtin_huge_valf();
        int bl = -1;
        if (!done) {
            for (int64_t i = lane; i < nc; i += kWave) {
                const int l = ci[i];
                const float s = cs[i];
                if (l < 0 || (pl >= 0 && !knn_before(ps, pl, s, l))) continue;    // empty, or not after the previous one
                if (bl < 0 || knn_before(s, l, bs, bl)) {
                    bs = s;
                    bl = l;
                }
            }
            auto fold = [&](float os, int ol) {
                if (ol >= 0 && (bl < 0 || knn_before(os, ol, bs, bl))) {
                    bs = os;
                    bl = ol;
                }
            };
            fold(lane_xor<32>(bs), lane_xor<32>(bl));
            fold(lane_xor<16>(bs), lane_xor<16>(bl));
            fold(lane_xor<8>(bs), lane_xor<8>(bl));
            fold(lane_xor<4>(bs), lane_xor<4>(bl));
            fold(lane_xor<2>(bs), lane_xor<2>(bl));
            fold(lane_xor<1>(bs), lane_xor<1>(bl));
            if (bl < 0) {
                done = true;
                bs = __builtin_huge_valf();
            } else {
                ps = bs;
                pl = bl;
            }
        }
        if (lane == 0) {
            out_d[q * k + r] = bs;
            out_id[q * k + r] = bl;
        }
    }
}

// ---- conditional affinities over the neighbours ----------------------------------------------------------------------
// One wave per row.  Lane l holds the places l, l + 64, l + 128 of the row and adds them in that order (fp32 partials);
// the 64 partials are added in double by the xor butterfly; every lane then takes the same step of
// tsne_affinities_kernel's search on the same two sums.  A place without a neighbour (id < 0) gets p = 0.
__global__ __launch_bounds__(kBlock) void tsne_nn_affinities_kernel(const float *__restrict__ sqd,
                                                                    const int32_t *__restrict__ ids, int64_t n, int k,
                                                                    float perplexity, float *__restrict__ p,
                                                                    float *__restrict__ beta_out) {
    constexpr int PER = kKnnMaxK / kWave;
    static_assert(PER * kWave == kKnnMaxK, "a lane's places");
    const int lane = lane_id();
    const int64_t i = int64_t(blockIdx.x) * kNnRowsPerBlock + threadIdx.x / kWave;
    if (i >= n) return;                                       // wave-uniform; no barrier below
    float dd[PER];
    bool ok[PER];
    float m = -__builtin_huge_valf();                        // max of -d over the neighbours
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int j = lane + kWave * u;
        ok[u] = j < k && ids[i * k + j] >= 0;
        dd[u] = ok[u] ? sqd[i * k + j] : 0.f;
        if (ok[u]) m = fmaxf(m, -dd[u]);
    }
    m = group_max<kWave>(m);
    const float dmin = -m;
#pragma unroll
    for (int u = 0; u < PER; ++u) dd[u] = dd[u] - dmin;

    const double target = log(double(perplexity));
    const float inf = __builtin_huge_valf();
    float beta = 1.f, beta_min = -inf, beta_max = inf;
    double sum_p = 1.0;
    for (int step = 0; step < kTsneSearchSteps; ++step) {
        float sp = 0.f, sdp = 0.f;
#pragma unroll
        for (int u = 0; u < PER; ++u)
            if (ok[u]) {
                const float e = expf(-beta * dd[u]);
                sp += e;
                sdp = fmaf(dd[u], e, sdp);
            }
        sum_p = group_sum<kWave>(double(sp));
        const double sum_dp = group_sum<kWave>(double(sdp));
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
    const float denom = float(sum_p);
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int j = lane + kWave * u;
        if (j < k) p[i * k + j] = ok[u] ? expf(-beta * dd[u]) / denom : 0.f;
    }
    if (lane == 0) beta_out[i] = beta;
}

// The extent of CSR row i, held inside [0, nnz] whatever rowptr says.
__device__ __forceinline__ void nn_row_extent(const int64_t *__restrict__ rowptr, int64_t i, int64_t nnz, int64_t &e0,
                                              int64_t &e1) {
    e0 = rowptr[i];
    e1 = rowptr[i + 1];
    e0 = e0 < 0 ? 0 : e0 > nnz ? nnz : e0;
    e1 = e1 < e0 ? e0 : e1 > nnz ? nnz : e1;
}

// out[i] = sum p ln p over CSR row i in double: lane l of the row's wave adds the entries l, l + 64, .. of the row in
// column order, the lanes are added by the xor butterfly.
__global__ __launch_bounds__(kBlock) void tsne_nn_plogp_kernel(const int64_t *__restrict__ rowptr,
                                                               const float *__restrict__ val, int64_t n, int64_t nnz,
                                                               double *__restrict__ out) {
    const int lane = lane_id();
    const int64_t i = int64_t(blockIdx.x) * kNnRowsPerBlock + threadIdx.x / kWave;
    if (i >= n) return;
    int64_t e0, e1;
    nn_row_extent(rowptr, i, nnz, e0, e1);
    double acc = 0.0;
    for (int64_t e = e0 + lane; e < e1; e += kWave) {
        const float v = val[e];
        if (v > 0.f) acc += double(v) * log(double(v));
    }
    acc = group_sum<kWave>(acc);
    if (lane == 0) out[i] = acc;
}

// ---- attraction ------------------------------------------------------------------------------------------------------
// One wave per CSR row, however long: lane l adds the entries l, l + 64, .. of the row in column order (fp32), the lanes
// are added by the xor butterfly.  F[i, 0:2] = sum P_ij q_ij (y_i - y_j), F[i, 5] = sum P_ij log1p(d^2) (0 without
// want_l).  A column outside [0, n) is skipped.
__global__ __launch_bounds__(kBlock) void tsne_nn_attract_kernel(const int64_t *__restrict__ rowptr,
                                                                 const int32_t *__restrict__ cols,
                                                                 const float *__restrict__ val,
                                                                 const float *__restrict__ Y, int64_t n, int64_t nnz,
                                                                 int want_l, float *__restrict__ F) {
    const int lane = lane_id();
    const int64_t i = int64_t(blockIdx.x) * kNnRowsPerBlock + threadIdx.x / kWave;
    if (i >= n) return;
    int64_t e0, e1;
    nn_row_extent(rowptr, i, nnz, e0, e1);
    const float yx = Y[2 * i], yy = Y[2 * i + 1];
    float ax = 0.f, ay = 0.f, al = 0.f;
    for (int64_t e = e0 + lane; e < e1; e += kWave) {
        const int64_t j = cols[e];
        if (j < 0 || j >= n) continue;
        const float pv = val[e];
        const float dx = yx - Y[2 * j], dy = yy - Y[2 * j + 1];
        const float d2 = fmaf(dx, dx, dy * dy);
        const float pq = pv * __builtin_amdgcn_rcpf(1.f + d2);
        ax = fmaf(pq, dx, ax);
        ay = fmaf(pq, dy, ay);
        if (want_l) al = fmaf(pv, log1pf(d2), al);
    }
    ax = group_sum<kWave>(ax);
    ay = group_sum<kWave>(ay);
    al = group_sum<kWave>(al);
    if (lane == 0) {
        F[i * kTsneForceCols + 0] = ax;
        F[i * kTsneForceCols + 1] = ay;
        F[i * kTsneForceCols + 5] = al;
    }
}

// ---- repulsion -------------------------------------------------------------------------------------------------------
// The terms of one staged chunk.  CHECK: the chunk holds one of the workgroup's own rows or ends before kTsneChunk
// points; otherwise every staged point is a point and none is the row itself, and the two tests per pair are left out.
template <bool CHECK>
__device__ __forceinline__ void tsne_repulse_chunk(const float *Ys, int cn, int lane, int64_t c0, int64_t r0,
                                                   const float (&yi)[kRepulseRowsPerWave][2],
                                                   float (&acc)[kRepulseRowsPerWave][3]) {
    constexpr int RW = kRepulseRowsPerWave;
    for (int jj = 4 * lane; jj < cn; jj += 4 * kWave) {
        float yx[4], yy[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            yx[u] = Ys[2 * (jj + u)];
            yy[u] = Ys[2 * (jj + u) + 1];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t j = c0 + jj + u;
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const float dx = yi[r][0] - yx[u], dy = yi[r][1] - yy[u];
                const float d2 = fmaf(dx, dx, dy * dy);
                float q = __builtin_amdgcn_rcpf(1.f + d2);
                if (CHECK) q = jj + u < cn ? q : 0.f;
                const float qq = q * q;
                acc[r][0] = fmaf(qq, dx, acc[r][0]);
                acc[r][1] = fmaf(qq, dy, acc[r][1]);
                acc[r][2] += (CHECK && j == r0 + r) ? 0.f : q;
            }
        }
    }
}

// A workgroup owns 16 consecutive rows, each wave 4 of them: one LDS read of a point serves the wave's 4 rows.  Y goes
// through LDS kTsneChunk points at a time; lane l takes the columns c0 + 4 l + 256 m + u (u = 0..3) of every chunk in
// that order into fp32 partials, the 64 lanes are added by the xor butterfly -- tsne_forces_kernel's order, a function of
// n alone.  F[i, 2:4] = sum_j q^2 (y_i - y_j), F[i, 4] = sum_{j != i} q.
__global__ __launch_bounds__(kBlock) void tsne_repulse_kernel(const float *__restrict__ Y, int64_t n,
                                                              float *__restrict__ F) {
    constexpr int RW = kRepulseRowsPerWave;
    __shared__ __attribute__((aligned(16))) float Ys[2 * kTsneChunk];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int64_t b0 = int64_t(blockIdx.x) * kRepulseRowsPerBlock;
    const int64_t r0 = b0 + (tid / kWave) * RW;

    float yi[RW][2], acc[RW][3];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const bool ok = r0 + r < n;
        yi[r][0] = ok ? Y[2 * (r0 + r)] : 0.f;
        yi[r][1] = ok ? Y[2 * (r0 + r) + 1] : 0.f;
        acc[r][0] = acc[r][1] = acc[r][2] = 0.f;
    }
    for (int64_t c0 = 0; c0 < n; c0 += kTsneChunk) {
        __syncthreads();                                      // the previous chunk has been read by every wave
        for (int e = tid; e < 2 * kTsneChunk; e += kBlock) Ys[e] = 2 * c0 + e < 2 * n ? Y[2 * c0 + e] : 0.f;
        __syncthreads();
        if (r0 >= n) continue;                                // a wave without rows only helps staging
        const int cn = int(n - c0 < kTsneChunk ? n - c0 : kTsneChunk);
        const bool own = b0 < c0 + cn && b0 + kRepulseRowsPerBlock > c0;
        if (cn < kTsneChunk || own) tsne_repulse_chunk<true>(Ys, cn, lane, c0, r0, yi, acc);
        else tsne_repulse_chunk<false>(Ys, cn, lane, c0, r0, yi, acc);
    }
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = group_sum<kWave>(acc[r][c]);
            if (lane == 0 && r0 + r < n) F[(r0 + r) * kTsneForceCols + 2 + c] = v;
        }
}

}  // namespace clane
