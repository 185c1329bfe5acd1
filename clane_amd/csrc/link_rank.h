// Link prediction -- scores of a batch of query rows against EVERY row of a table with the top-k selection fused in
// (rank_scores_kernel), the merge of the per-slab candidates (rank_merge_kernel) and scores of explicit pairs
// (pair_score_kernel).
//
// No reference counterpart: the reference stops at Z.npy.  The score is the model's own -- the bilinear
// (Phi_src z_u) . (Phi_dst z_v) of AsymmertricSimilarity (similarity.py:40-57; S = Y, N = Y + d of the projected table,
// projection.h) or the cosine of CosineSimilarity (similarity.py:26-37; S = N = Z, the modes of edge_score.h).
//
// rank_scores_kernel is mfma_tile.h's contraction with the A operand's rows taken through the query list and the B
// operand the rows of N with a leading dimension: a 256-thread workgroup
// owns one tile of 32 MI queries (128 for f32 / bf16, 64 for f64: the lists below have to fit the LDS beside the
// staged slices) and one slab of candidate rows, walks the slab's 128-row tiles and keeps every query's running top-k
// in LDS, so the Q x V score matrix never exists.  A pair's dot always is the same MFMA chain in the fixed k order of
// mfma_slice -- it does not depend on the tile, the slab or the lane it falls in -- so the merged result is
// bit-identical for every n_slabs.
//
// Selection, after a tile's MFMAs: every accumulator is scaled (mode) and compared with its query's current k-th score
// (one LDS read per query row); only survivors are checked for eligibility (label, self, binary search in the
// exclusion CSR) and inserted into the query's sorted list by ONE thread.  Writers of one list take turns: the two
// waves that share the query rows run their selection one after the other (a barrier between), and inside a wave the
// 16 lanes that hold one query row's candidates insert one lane at a time (the four row groups of a wave work on
// different queries side by side).  The order is total -- score descending, ties by label ascending -- so the list
// after a tile does not depend on who went first.  After the first few tiles nearly every candidate fails the
// threshold compare and the selection is the 64 multiplies and compares per thread.
#pragma once

#include "device_utils.h"
#include "edge_score.h"
#include "mfma_tile.h"

namespace clane {

constexpr int kRankMaxK = 32;
constexpr int kRankBN = 128;      // candidate rows per tile

// (s, l) comes before (ps, pl) in the result order
template <typename A>
__device__ __forceinline__ bool rank_before(A s, int l, A ps, int pl) {
    return s > ps || (s == ps && l < pl);
}

// 1 / sqrt(x) for the per-edge cosine, 0 for a zero row (its pairs score 0); formed in double so that the two factors
// and the two multiplies stay within 3 eps of dot / (sqrt(sq_q) sqrt(sq_v))
template <typename A>
__device__ __forceinline__ A rank_rnorm(A x) {
    return x > A(0) ? A(1.0 / sqrt(double(x))) : A(0);
}
template <typename A>
__device__ __forceinline__ A rank_rdenominator(const double *__restrict__ sums2) {
    return A(1.0 / sqrt(sums2[0] * sums2[1]));
}

// One thread puts (s, lab) into the sorted list sc / id of k places, if it comes before the last one.
template <typename A>
__device__ __forceinline__ void rank_insert(volatile A *sc, volatile int *id, int k, A s, int lab) {
    if (!rank_before<A>(s, lab, sc[k - 1], id[k - 1])) return;
    int j = k - 1;
    while (j > 0) {
        const A ps = sc[j - 1];
        const int pl = id[j - 1];
        if (!rank_before<A>(s, lab, ps, pl)) break;
        sc[j] = ps;
        id[j] = pl;
        --j;
    }
    sc[j] = s;
    id[j] = lab;
}

// is `want` a column of row r of the CSR (rows sorted and unique: pair_labels_kernel's search)
__device__ __forceinline__ bool rank_excluded(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                              int64_t r, int32_t want) {
    int64_t lo = rowptr[r];
    const int64_t end = rowptr[r + 1];
    int64_t hi = end;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (colidx[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && colidx[lo] == want;
}

// Dynamic LDS: the lists, BM * k scores then BM * k ids.
template <typename A>
constexpr size_t rank_list_bytes(int bm, int k) { return size_t(bm) * k * (sizeof(A) + sizeof(int)); }

// blockIdx.x = slab * q_tiles + query tile: the workgroups that read one slab of N run together.
// Slab s holds the candidate tiles [s * tiles_per_slab, (s + 1) * tiles_per_slab) -- none at all when n_slabs is more
// than the table has tiles; such a workgroup only writes its empty lists.
// rank_scores_kernel keeps its own text of the staged k loop (through the shared loop it measured slower:
// profiles/r13_mfma_tile_times.md).  mfma_slice (mfma_tile.h) is the contract for its k order all the same: step kk
// gives lane group g = lane / 16 the k index 4 g + kk, and the MFMAs run in the order kk, mi, ni.  A change there is a
// change here.
#ifndef CLANE_RANK_MIN_WAVES
#define CLANE_RANK_MIN_WAVES 2    // rank_scores_kernel: __launch_bounds__ 2nd argument (waves per SIMD)
#endif
template <typename T, typename A, int MI>
__global__ __launch_bounds__(kBlock, CLANE_RANK_MIN_WAVES) void rank_scores_kernel(
    const T *__restrict__ S, int64_t lds, const T *__restrict__ N, int64_t ldn, int64_t table_rows, int d,
    const int32_t *__restrict__ q_rows, int64_t Q, int mode, const double *__restrict__ sums2,
    const A *__restrict__ sq, const int32_t *__restrict__ label, const int64_t *__restrict__ excl_rowptr,
    const int32_t *__restrict__ excl_colidx, int exclude_self, int k, int n_slabs, int64_t q_tiles,
    int64_t tiles_per_slab, A *__restrict__ cand_score, int32_t *__restrict__ cand_id) {
    using M = ProjMfma<A>;
    using acc4 = typename M::acc4;
    constexpr int BM = 32 * MI, BN = kRankBN, BK = kProjBK;
    constexpr int LD = BK + 16 / int(sizeof(A));
    constexpr int PER_A = BM * BK / kBlock, PER_B = BN * BK / kBlock;
    static_assert(BM * BK % kBlock == 0 && BN == 128 && kBlock == 256, "staging layout");
    __shared__ __attribute__((aligned(16))) A As[BM * LD];
    __shared__ __attribute__((aligned(16))) A Bs[BN * LD];
    __shared__ A s_rq[BM];          // the query's factor: 1, 1 / D, or 1 / |s_q|
    __shared__ int s_qrow[BM];      // its table row; < 0: no such query (past Q, or a row outside the table)
    extern __shared__ __attribute__((aligned(16))) unsigned char rank_dyn[];
    volatile A *l_sc = reinterpret_cast<volatile A *>(rank_dyn);
    volatile int *l_id = reinterpret_cast<volatile int *>(rank_dyn + size_t(BM) * k * sizeof(A));

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t slab = blockIdx.x / q_tiles;
    const int64_t m0 = (blockIdx.x % q_tiles) * BM;
    const int wm = (wave & 1) * (16 * MI), wn = (wave >> 1) * 64;
    const int g = lane >> 4, li = lane & 15;
    (void)g;

    const int64_t tiles_total = ceil_div(table_rows, int64_t(BN));
    const int64_t t0 = slab * tiles_per_slab < tiles_total ? slab * tiles_per_slab : tiles_total;
    const int64_t t1 = t0 + tiles_per_slab < tiles_total ? t0 + tiles_per_slab : tiles_total;

    for (int i = tid; i < BM * k; i += kBlock) {
        l_sc[i] = -A(INFINITY);
        l_id[i] = -1;
    }
    for (int i = tid; i < BM; i += kBlock) {
        int64_t r = -1;
        if (m0 + i < Q) {
            r = q_rows[m0 + i];
            if (r >= table_rows) r = -1;
        }
        A f = A(1);
        if (mode == kScoreReference) f = rank_rdenominator<A>(sums2);
        if (mode == kScorePerEdge) f = r >= 0 ? rank_rnorm<A>(sq[r]) : A(0);
        s_qrow[i] = r < 0 ? -1 : int(r);
        s_rq[i] = f;
    }

    // staging: thread t moves k = t % BK of rows t / BK + 16 s
    const int sk = tid % BK, si = tid / BK;
    int64_t roff[PER_A];
#pragma unroll
    for (int s = 0; s < PER_A; ++s) {
        const int64_t qi = m0 + si + s * (kBlock / BK);
        int64_t r = -1;
        if (qi < Q) {
            r = q_rows[qi];
            if (r >= table_rows) r = -1;
        }
        roff[s] = r < 0 ? -1 : r * lds;
    }
    A ra[PER_A], rb[PER_B];
    auto fetch = [&](int64_t n0, int k0) {
        const int kc = k0 + sk;
#pragma unroll
        for (int s = 0; s < PER_A; ++s)
            ra[s] = (kc < d && roff[s] >= 0) ? A(Elem<T>::to_acc(S[roff[s] + kc])) : A(0);
#pragma unroll
        for (int s = 0; s < PER_B; ++s) {
            const int64_t j = n0 + si + s * (kBlock / BK);
            rb[s] = (kc < d && j < table_rows) ? A(Elem<T>::to_acc(N[j * ldn + kc])) : A(0);
        }
    };

    acc4 acc[MI][4];
    if (t0 < t1) fetch(t0 * BN, 0);
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t n0 = tile * BN;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = acc4{A(0), A(0), A(0), A(0)};
        // the tile's column factors: requested now, used after the MFMAs
        A cs[4];
        bool col_ok[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int64_t v = n0 + wn + 16 * ni + li;
            col_ok[ni] = v < table_rows;
            cs[ni] = A(1);
            if (mode == kScorePerEdge) cs[ni] = col_ok[ni] ? rank_rnorm<A>(sq[v]) : A(0);
        }

        for (int k0 = 0; k0 < d; k0 += BK) {
            __syncthreads();                              // the previous slice has been read by every wave
#pragma unroll
            for (int s = 0; s < PER_A; ++s) As[(si + s * (kBlock / BK)) * LD + sk] = ra[s];
#pragma unroll
            for (int s = 0; s < PER_B; ++s) Bs[(si + s * (kBlock / BK)) * LD + sk] = rb[s];
            __syncthreads();
            if (k0 + BK < d) fetch(n0, k0 + BK);          // in flight while the MFMAs below run
            else if (tile + 1 < t1) fetch(n0 + BN, 0);    // ... and the next tile's first slice during the selection
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

        // ---- selection: the waves of the first column half, a barrier, those of the second
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {
            // opaque copies: 16 query rows x {list, factor, row} addresses per thread are loop invariants that would
            // otherwise be formed once and held in registers across the MFMA loop (a third of the register file)
            int kq = k, lq = lane;
            asm volatile("" : "+s"(kq), "+v"(lq));
            if ((wave >> 1) == half) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int ql = wm + 16 * mi + M::row(lq, reg);
                        const A thr = l_sc[ql * kq + kq - 1];
                        const A rq = s_rq[ql];
                        A s[4];
                        bool pass[4], any = false;
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni) {
                            s[ni] = (acc[mi][ni][reg] * rq) * cs[ni];
                            pass[ni] = col_ok[ni] && s[ni] >= thr;
                            any = any || pass[ni];
                        }
                        if (!__any(any)) continue;        // wave-uniform: the common case after the first tiles
                        const int qr = s_qrow[ql];
                        int lab[4];
                        bool mine = false;
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni) {
                            bool ok = pass[ni] && qr >= 0;
                            lab[ni] = -1;
                            if (ok) {
                                const int v = int(n0) + wn + 16 * ni + li;
                                lab[ni] = label ? label[v] : v;
                                ok = lab[ni] >= 0 && !(exclude_self && v == qr);
                                if (ok && excl_rowptr) ok = !rank_excluded(excl_rowptr, excl_colidx, qr, v);
                            }
                            pass[ni] = ok;
                            mine = mine || ok;
                        }
                        const unsigned long long m = __ballot(mine);
                        unsigned turns = unsigned((m | (m >> 16) | (m >> 32) | (m >> 48)) & 0xffffu);
                        while (turns) {                   // one lane of each 16-lane row group at a time
                            const int t = __ffs(turns) - 1;
                            turns &= turns - 1;
                            if (li == t && mine) {
#pragma unroll 1
                                for (int c = 0; c < 4; ++c) {     // one copy of the insertion: the values by select
                                    const bool pc = c == 0 ? pass[0] : c == 1 ? pass[1] : c == 2 ? pass[2] : pass[3];
                                    const A sv = c == 0 ? s[0] : c == 1 ? s[1] : c == 2 ? s[2] : s[3];
                                    const int lv = c == 0 ? lab[0] : c == 1 ? lab[1] : c == 2 ? lab[2] : lab[3];
                                    if (pc) rank_insert<A>(l_sc + ql * kq, l_id + ql * kq, kq, sv, lv);
                                }
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
        if (qi < Q) {
            const int64_t o = (qi * n_slabs + slab) * k + i % k;
            cand_score[o] = l_sc[i];
            cand_id[o] = l_id[i];
        }
    }
}

// One wave per query: k rounds, each the best candidate that comes after the one emitted before it.  The order is
// total (labels are unique among eligible rows), so "after the previous one" needs no bookkeeping per slab, and the
// result depends on the SET of candidates alone.  Lane l looks at the places l, l + 64, ... of the query's
// n_slabs * k candidates.
template <typename A>
__global__ __launch_bounds__(kBlock) void rank_merge_kernel(const A *__restrict__ cand_score,
                                                            const int32_t *__restrict__ cand_id, int64_t Q, int n_slabs,
                                                            int k, A *__restrict__ out_score,
                                                            int32_t *__restrict__ out_id) {
    const int lane = lane_id();
    const int64_t q = int64_t(blockIdx.x) * kWavesPerBlock + threadIdx.x / kWave;
    if (q >= Q) return;                                   // wave-uniform; no barrier below
    const int64_t n = int64_t(n_slabs) * k;
    const A *__restrict__ cs = cand_score + q * n;
    const int32_t *__restrict__ ci = cand_id + q * n;
    A ps = A(INFINITY);
    int pl = -1;
    bool done = false;
    for (int r = 0; r < k; ++r) {
        A bs = -A(INFINITY);
        int bl = -1;
        if (!done) {
            for (int64_t i = lane; i < n; i += kWave) {
                const int l = ci[i];
                const A s = cs[i];
                if (l < 0 || !rank_before<A>(ps, pl, s, l)) continue;       // empty, or not after the previous one
                if (bl < 0 || rank_before<A>(s, l, bs, bl)) {
                    bs = s;
                    bl = l;
                }
            }
            auto fold = [&](A os, int ol) {
                if (ol >= 0 && (bl < 0 || rank_before<A>(os, ol, bs, bl))) {
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
                bs = -A(INFINITY);
            }
            ps = bs;
            pl = bl;
        }
        if (lane == 0) {
            out_score[q * k + r] = bs;
            out_id[q * k + r] = bl;
        }
    }
}

// out[i] = score(src[i], dst[i]): a sub-wave of LPR lanes per pair, 16-byte packs when the layout allows, the
// butterfly of group_sum.  An index outside [0, table_rows) reads as a zero row (score 0).
template <typename T, int VEC, int LPR>
__global__ __launch_bounds__(kBlock) void pair_score_kernel(const T *__restrict__ S, int64_t lds,
                                                            const T *__restrict__ N, int64_t ldn, int64_t table_rows,
                                                            int d, const int32_t *__restrict__ src,
                                                            const int32_t *__restrict__ dst, int64_t B, int mode,
                                                            const double *__restrict__ sums2,
                                                            const typename Elem<T>::acc_t *__restrict__ sq,
                                                            typename Elem<T>::acc_t *__restrict__ out) {
    using A = typename Elem<T>::acc_t;
    constexpr int RPW = kWave / LPR;
    const int lane = lane_id();
    const int sub = lane / LPR, sl = lane % LPR;
    const int64_t wave = int64_t(blockIdx.x) * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t nwaves = int64_t(gridDim.x) * kWavesPerBlock;
    const A rD = mode == kScoreReference ? rank_rdenominator<A>(sums2) : A(1);
    for (int64_t base = wave * RPW; base < B; base += nwaves * RPW) {
        const int64_t i = base + sub;
        int64_t s = -1, t = -1;
        if (i < B) {
            s = src[i];
            t = dst[i];
        }
        const bool ok = s >= 0 && s < table_rows && t >= 0 && t < table_rows;
        A dot = A(0);
        if (ok) {
            const T *__restrict__ a = S + s * lds;
            const T *__restrict__ b = N + t * ldn;
            for (int c0 = sl * VEC; c0 < d; c0 += LPR * VEC) {
                const Pack<T, VEC> x = load_pack<T, VEC>(a + c0);
                const Pack<T, VEC> y = load_pack<T, VEC>(b + c0);
#pragma unroll
                for (int c = 0; c < VEC; ++c) dot = fma(Elem<T>::to_acc(x.v[c]), Elem<T>::to_acc(y.v[c]), dot);
            }
        }
        dot = group_sum<LPR>(dot);
        if (i < B && sl == 0) {
            A f = rD, h = A(1);
            if (mode == kScorePerEdge) {
                f = ok ? rank_rnorm<A>(sq[s]) : A(0);
                h = ok ? rank_rnorm<A>(sq[t]) : A(0);
            }
            out[i] = (dot * f) * h;
        }
    }
}

}  // namespace clane
