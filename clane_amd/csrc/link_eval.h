// Held-out link evaluation -- for B pairs (query row, target row) the score of the pair and, among ALL rows of the
// table, how many eligible candidates score above the target, how many tie with it on either side of its label, and
// how many are eligible at all (rank_count_kernel).  From the counts the host forms the filtered rank, MRR, Hits@K, AUC.
//
// The smaller sibling of rank_scores_kernel (link_rank.h): the same tiling, the same MFMA chain in mfma_slice's k
// order (mfma_tile.h), the same scaling (acc * rq) * cs -- so a pair scores the SAME BITS here as in the top-k lists, and
// 1 + greater + equal_lower is the target's place in top_k's order (score descending, ties by label ascending).  The
// insertion is replaced by counting, which has no writer turns and no lists.
//
// The target's score: before its slab, a workgroup runs ONE tile whose B-operand rows are the targets of its own pairs
// (gathered through t_rows); the diagonal of that tile is score(query i, target i), kept in LDS as pair i's threshold.
// Every slab's workgroup recomputes it (identical bits); slab 0 writes it out.
//
// Eligibility of candidate v for pair (q, t): label[v] >= 0, v != t, v != q under exclude_self, v not in row q of the
// exclusion CSR.  The column part (label, v < table_rows) is one load per tile column.  The per-pair part is a bit
// mask in LDS, 128 bits per pair and tile, written by ONE thread per pair: it keeps a cursor into the pair's CSR row
// (placed by one binary search at the slab's first row) and advances it over the entries that fall in the tile's 128
// rows -- O(1 + those entries) per (pair, tile), the next entry already in flight.  Two mask buffers alternate, so the
// writer of tile t + 1 never meets a reader of tile t (the barriers of the k loop lie between).
//
// Counters: after a tile every thread has, for each of its 4 MI query rows, the four counts of its 4 columns packed in
// one int (8 bits each); a butterfly over the 16 lanes that share the query row sums them (at most 64 per field), and
// lane li keeps the totals of the li-th query row in four int registers.  At the end the two waves that share the query
// rows meet in LDS.  No atomics, no float reduction: the counts do not depend on n_slabs or the launch.
#pragma once

#include "device_utils.h"
#include "edge_score.h"
#include "link_rank.h"
#include "mfma_tile.h"

namespace clane {

// Like rank_scores_kernel, rank_count_kernel keeps its own text of the staged k loop (through the shared loop it measured
// slower at the largest shape: profiles/r13_mfma_tile_times.md); mfma_slice (mfma_tile.h) is the contract for its k
// order: step kk gives lane group g = lane / 16 the k index 4 g + kk, and the MFMAs run in the order kk, mi, ni.
#ifndef CLANE_COUNT_MIN_WAVES
#define CLANE_COUNT_MIN_WAVES 2   // rank_count_kernel: __launch_bounds__ 2nd argument (waves per SIMD)
#endif
// blockIdx.x = slab * q_tiles + pair tile, slabs as in rank_scores_kernel.
// counts [B, n_slabs, 4] = {greater, equal_lower, equal_higher, eligible} of the slab's rows; a pair without a rank
// (query or target outside the table, or a target with a negative label): four -1 in every slab, target_score -inf.
template <typename T, typename A, int MI>
__global__ __launch_bounds__(kBlock, CLANE_COUNT_MIN_WAVES) void rank_count_kernel(
    const T *__restrict__ S, int64_t lds, const T *__restrict__ N, int64_t ldn, int64_t table_rows, int d,
    const int32_t *__restrict__ q_rows, const int32_t *__restrict__ t_rows, int64_t B, int mode,
    const double *__restrict__ sums2, const A *__restrict__ sq, const int32_t *__restrict__ label,
    const int64_t *__restrict__ excl_rowptr, const int32_t *__restrict__ excl_colidx, int exclude_self, int n_slabs,
    int64_t q_tiles, int64_t tiles_per_slab, A *__restrict__ target_score, int32_t *__restrict__ counts) {
    using M = ProjMfma<A>;
    using acc4 = typename M::acc4;
    constexpr int BM = 32 * MI, BN = kRankBN, BK = kProjBK;
    constexpr int LD = BK + 16 / int(sizeof(A));
    constexpr int PER_A = BM * BK / kBlock, PER_B = BN * BK / kBlock;
    static_assert(BM * BK % kBlock == 0 && BN == 128 && kBlock == 256 && BM <= BN && BM <= kBlock, "staging layout");
    static_assert(4 * MI <= 16, "one lane of a 16-lane row group per query row of the thread");
    __shared__ __attribute__((aligned(16))) A As[BM * LD];
    __shared__ __attribute__((aligned(16))) A Bs[BN * LD];
    __shared__ A s_rq[BM];          // the query's factor: 1, 1 / D, or 1 / |s_q|
    __shared__ A s_thr[BM];         // score(query, target): the threshold of the pair
    __shared__ int s_qrow[BM];      // the query's table row; < 0: outside the table, or past B
    __shared__ int s_trow[BM];      // the target's
    __shared__ int s_tlab[BM];      // the target's label; < 0: the pair has no rank
    __shared__ unsigned long long s_mask[2][BM][2];     // [buffer][pair][column half]: bit c = column c is not eligible
    __shared__ int s_cnt[2][BM][4];                     // [column half][pair]: the two waves' totals

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t slab = blockIdx.x / q_tiles;
    const int64_t m0 = (blockIdx.x % q_tiles) * BM;
    const int wm = (wave & 1) * (16 * MI), wn = (wave >> 1) * 64;
    const int li = lane & 15;

    const int64_t tiles_total = ceil_div(table_rows, int64_t(BN));
    const int64_t t0 = slab * tiles_per_slab < tiles_total ? slab * tiles_per_slab : tiles_total;
    const int64_t t1 = t0 + tiles_per_slab < tiles_total ? t0 + tiles_per_slab : tiles_total;
    const int64_t n_tiles = t1 - t0;

    // ---- the pairs of this workgroup; thread i < BM owns pair i's mask and its cursor into the exclusion row
    int my_q = -1, my_t = -1;
    int64_t cur = 0;                                      // the cursor: the row's first entry not yet behind the tiles
    int left = 0, nxt = 0;                                // entries from cur to the row's end; excl_colidx[cur] while left > 0
    if (tid < BM) {
        int64_t q = -1, t = -1;
        if (m0 + tid < B) {
            q = q_rows[m0 + tid];
            t = t_rows[m0 + tid];
            if (q >= table_rows) q = -1;
            if (t >= table_rows) t = -1;
        }
        int tl = -1;
        if (q >= 0 && t >= 0) tl = label ? label[t] : int(t);
        if (tl < 0) q = t = -1;                           // no rank: the pair takes no further part
        A f = A(1);
        if (mode == kScoreReference) f = rank_rdenominator<A>(sums2);
        if (mode == kScorePerEdge) f = q >= 0 ? rank_rnorm<A>(sq[q]) : A(0);
        my_q = q < 0 ? -1 : int(q);
        my_t = t < 0 ? -1 : int(t);
        s_qrow[tid] = my_q;
        s_trow[tid] = my_t;
        s_tlab[tid] = tl;
        s_rq[tid] = f;
        s_thr[tid] = -A(INFINITY);
        if (excl_rowptr && my_q >= 0 && n_tiles > 0) {    // first entry of the row at or after the slab's first row
            int64_t lo = excl_rowptr[my_q];
            const int64_t end = excl_rowptr[my_q + 1];
            int64_t hi = end;
            const int64_t first = t0 * BN;
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (excl_colidx[mid] < first) lo = mid + 1;
                else hi = mid;
            }
            cur = lo;
            left = int(end - lo);                         // unique int32 columns: a row has fewer than 2^31 entries
            if (left > 0) nxt = excl_colidx[cur];
        }
    }
    __syncthreads();

    // staging: thread t moves k = t % BK of rows t / BK + 16 s
    const int sk = tid % BK, si = tid / BK;
    int64_t roff[PER_A];
#pragma unroll
    for (int s = 0; s < PER_A; ++s) {
        const int r = s_qrow[si + s * (kBlock / BK)];
        roff[s] = r < 0 ? -1 : r * lds;
    }
    A ra[PER_A], rb[PER_B];
    // diag: the B rows are the targets of the workgroup's own pairs (rows past BM, or without a target: zero)
    auto fetch = [&](bool diag, int64_t n0, int k0) {
        const int kc = k0 + sk;
#pragma unroll
        for (int s = 0; s < PER_A; ++s)
            ra[s] = (kc < d && roff[s] >= 0) ? A(Elem<T>::to_acc(S[roff[s] + kc])) : A(0);
#pragma unroll
        for (int s = 0; s < PER_B; ++s) {
            const int i = si + s * (kBlock / BK);
            int64_t j = n0 + i;
            if (diag) j = i < BM ? int64_t(s_trow[i]) : -1;
            rb[s] = (kc < d && j >= 0 && j < table_rows) ? A(Elem<T>::to_acc(N[j * ldn + kc])) : A(0);
        }
    };

    int c_gt = 0, c_lo = 0, c_hi = 0, c_el = 0;          // lane li: the totals of this thread's li-th query row
    acc4 acc[MI][4];
    fetch(true, 0, 0);
    for (int64_t it = -1; it < n_tiles; ++it) {
        const bool diag = it < 0;
        const int64_t n0 = diag ? 0 : (t0 + it) * BN;
        const int buf = int(it & 1);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = acc4{A(0), A(0), A(0), A(0)};
        // the tile's columns: factor, label, validity -- requested now, used after the MFMAs
        A cs[4];
        int lab[4];                                       // < 0: not a candidate (padding row, past the table)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int64_t v = n0 + wn + 16 * ni + li;
            cs[ni] = A(1);
            lab[ni] = -1;
            if (!diag && v < table_rows) {
                if (mode == kScorePerEdge) cs[ni] = rank_rnorm<A>(sq[v]);
                lab[ni] = label ? label[v] : int(v);
            }
        }
        // the tile's mask rows: what the pair itself rules out among columns [n0, n0 + BN)
        if (!diag && tid < BM) {
            unsigned long long m[2] = {0ull, 0ull};
            auto rule_out = [&](int64_t v) {
                if (v >= n0 && v < n0 + BN) {
                    const int c = int(v - n0);
                    if (c < 64) m[0] |= 1ull << c;
                    else m[1] |= 1ull << (c - 64);
                }
            };
            while (left > 0 && nxt < n0 + BN) {           // sorted row: the entries of this tile, then stop
                rule_out(nxt);
                ++cur;
                --left;
                if (left > 0) nxt = excl_colidx[cur];     // used by the next tile at the earliest: in flight till then
            }
            if (exclude_self) rule_out(my_q);
            rule_out(my_t);                               // the target never is a candidate (my_t < 0: n0 >= 0 skips it)
            s_mask[buf][tid][0] = m[0];
            s_mask[buf][tid][1] = m[1];
        }

        for (int k0 = 0; k0 < d; k0 += BK) {
            __syncthreads();                              // the previous slice has been read by every wave
#pragma unroll
            for (int s = 0; s < PER_A; ++s) As[(si + s * (kBlock / BK)) * LD + sk] = ra[s];
#pragma unroll
            for (int s = 0; s < PER_B; ++s) Bs[(si + s * (kBlock / BK)) * LD + sk] = rb[s];
            __syncthreads();
            if (k0 + BK < d) fetch(diag, n0, k0 + BK);    // in flight while the MFMAs below run
            else if (it + 1 < n_tiles) fetch(false, (t0 + it + 1) * BN, 0);     // ... the next tile's during the counting
            A a[MI][4], b[4][4];                          // [tile][kk]: k = 4 g + kk of rows li + 16 tile
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
                for (int t = 0; t < MI; ++t) a[t][kk] = As[(wm + 16 * t + li) * LD + 4 * (lane >> 4) + kk];
#pragma unroll
                for (int t = 0; t < 4; ++t) b[t][kk] = Bs[(wn + 16 * t + li) * LD + 4 * (lane >> 4) + kk];
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = M::mma(a[mi][kk], b[ni][kk], acc[mi][ni]);
        }

        if (diag) {
            // ---- the diagonal: column c of this tile is pair c's target
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int ql = wm + 16 * mi + M::row(lane, reg);
                        if (ql != wn + 16 * ni + li) continue;
                        const int tr = s_trow[ql];
                        if (tr < 0) continue;             // no rank: stays -inf
                        const A ct = mode == kScorePerEdge ? rank_rnorm<A>(sq[tr]) : A(1);
                        s_thr[ql] = (acc[mi][ni][reg] * s_rq[ql]) * ct;
                    }
            continue;                                     // read after the barriers of the next tile / the final one
        }

        // ---- counting
        // an opaque copy of the thread index: the 4 MI query rows' LDS addresses (threshold, factor, mask, label) are
        // loop invariants that would otherwise be formed once and held in registers across the MFMA loop
        int tq = tid;
        asm volatile("" : "+v"(tq));
        const int lq = tq & (kWave - 1), half = tq / (2 * kWave), wmq = ((tq / kWave) & 1) * (16 * MI);
        int mine = 0;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int ql = wmq + 16 * mi + M::row(lq, reg);
                const A thr = s_thr[ql];
                const A rq = s_rq[ql];
                const unsigned long long out = s_mask[buf][ql][half] >> li;
                int p = 0;
                bool eq[4], any_eq = false;
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const A s = (acc[mi][ni][reg] * rq) * cs[ni];
                    const bool el = lab[ni] >= 0 && !((out >> (16 * ni)) & 1ull);
                    eq[ni] = el && s == thr;
                    any_eq = any_eq || eq[ni];
                    p += (el ? 1 << 24 : 0) + ((el && s > thr) ? 1 : 0);
                }
                if (__any(any_eq)) {                      // wave-uniform; rare on float data
                    const int tl = s_tlab[ql];
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni)
                        if (eq[ni]) p += lab[ni] < tl ? 1 << 8 : 1 << 16;
                }
                p += lane_xor<8>(p);                      // the 16 lanes of the query row: at most 64 per field
                p += lane_xor<4>(p);
                p += lane_xor<2>(p);
                p += lane_xor<1>(p);
                if (li == mi * 4 + reg) mine = p;
            }
        c_gt += mine & 0xff;
        c_lo += (mine >> 8) & 0xff;
        c_hi += (mine >> 16) & 0xff;
        c_el += (mine >> 24) & 0xff;
    }

    if (li < 4 * MI) {
        const int ql = wm + 16 * (li >> 2) + M::row(lane, li & 3);
        int *c = s_cnt[wave >> 1][ql];
        c[0] = c_gt;
        c[1] = c_lo;
        c[2] = c_hi;
        c[3] = c_el;
    }
    __syncthreads();
    if (tid < BM && m0 + tid < B) {
        const bool ranked = s_tlab[tid] >= 0;
        int32_t *o = counts + ((m0 + tid) * n_slabs + slab) * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = ranked ? s_cnt[0][tid][c] + s_cnt[1][tid][c] : -1;
        if (slab == 0) target_score[m0 + tid] = s_thr[tid];
    }
}

}  // namespace clane
