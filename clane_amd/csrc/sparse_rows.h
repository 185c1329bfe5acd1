// Sparse rows times a dense matrix -- the products of a randomized PCA on CSR content (reduce.py, ContentPCA.fit_sparse):
//
//     out[r, 0:l] = sum_e val[e] * B[col[e], 0:l]  -  a[r] * s[0:l]        e in [rowptr[r], rowptr[r + 1])
//
// and the rows' value sums in double.  fp32 only.  Nothing in the reference does this.
//
// Mapping to gfx950 (HBM-bound gathers of 16-byte packs, no MFMA: the K3 row pass of spmm_update.h without X + gamma, without
// the delta, with a value per non-zero and a rank-one epilogue):
//  * one wave64 owns one row (or one segment of a long row).  A row of l floats is covered by LPR lanes of one 16-byte pack
//    each: l <= 64: LPR = 16, l <= 128: 32, l <= 256: 64, l <= 512: 64 lanes of TWO packs (columns c and 256 + c).  With
//    LPR < 64 the wave gathers EPW = 64 / LPR rows of B with one instruction: sub-wave `sub` takes every EPW-th non-zero.
//  * col / val are read 64 non-zeros at a time, coalesced, then broadcast (v_readlane when the index is wave-uniform).
//  * U row loads of B are issued back to back before the first FMA; non-zeros past the end are exec-masked loads.
//  * a workgroup owns consecutive rows and its waves claim them from an LDS counter.
//  * a row of more than kCsrSegment non-zeros (the transpose of a bag of words has rows of up to n: stop words) is cut
//    into segments of kCsrSegment; every segment is a work item of its own (the first workgroups of the launch, one item
//    per wave) and writes its partial sum to the workspace; csr_spmm_combine_kernel adds a row's partials.
//
// The order of every element's sum, whatever the grid and whatever other rows the call holds:
//  1. inside a segment (a short row is one segment) sub-wave `sub` starts from +0 and adds the non-zeros k = sub, sub + EPW,
//     .. (k counted from the segment's start) in ascending k, each by one fmaf(val, B, acc);
//  2. the EPW sub-wave sums are folded by a butterfly: (s0 + s2) + (s1 + s3) for EPW = 4, s0 + s1 for EPW = 2;
//  3. a long row's segments are added in segment order, starting from the first segment's sum;
//  4. the epilogue is one fmaf(-a[r], s[c], sum)  (a NULL: a[r] = 1; s NULL: no epilogue).
// LPR and EPW depend on l alone, segments start at the row's own first non-zero: the same row gives the same bits in any
// matrix.  No atomics on memory, plain vector stores only.
//
// Row sums: lane t of the wave adds a segment's values t, t + 64, .. in double in that order, the 64 lane sums are folded by
// the butterfly group_sum<64>, a long row's segments are added in segment order.
#pragma once

#include "device_utils.h"

#ifndef CLANE_CSR_U
#define CLANE_CSR_U 8             // rows of B in flight per wave before the first FMA (4 with two packs per lane)
#endif

namespace clane {

constexpr int kCsrSegment = 2048;   // non-zeros of one work item; a multiple of 64
constexpr int kCsrMaxL = 512;
constexpr int kCsrTile = 256;       // columns one pack per lane covers

// acc = the sum of steps 1 and 2 over the non-zeros [e0, e1), e1 - e0 <= kCsrSegment.  Called by all 64 lanes.
template <int LPR, int NP>
__device__ __forceinline__ void csr_segment_sum(const int32_t *__restrict__ col, const float *__restrict__ val, int64_t e0,
                                                int64_t e1, const float *__restrict__ bcol, int64_t ldb,
                                                const bool (&ok)[NP], float (&acc)[NP][4]) {
    constexpr int EPW = kWave / LPR;
    constexpr int U = NP == 1 ? CLANE_CSR_U : (CLANE_CSR_U / 2 > 0 ? CLANE_CSR_U / 2 : 1);
    const int lane = lane_id();
    const int sub = lane / LPR;
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[p][k] = 0.0f;
    for (int64_t e = e0; e < e1; e += kWave) {
        const int64_t left = e1 - e;
        const int n = left < kWave ? int(left) : kWave;
        int c = 0;
        float v = 0.0f;
        if (lane < n) {
            c = col[e + lane];
            v = val[e + lane];
        }
        for (int j = 0; j < n; j += EPW * U) {
            Pack<float, 4> z[U][NP];
            float pj[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = j + u * EPW + sub;
                int cj;
                float pv;
                if constexpr (LPR == kWave) {
                    cj = lane_get_uniform(c, idx & (kWave - 1));
                    pv = lane_get_uniform(v, idx & (kWave - 1));
                } else {
                    cj = lane_get(c, idx & (kWave - 1));
                    pv = lane_get(v, idx & (kWave - 1));
                }
                const bool in_row = idx < n;
                pj[u] = in_row ? pv : 0.0f;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    z[u][p] = Pack<float, 4>{};
                    if (in_row && ok[p]) z[u][p] = load_pack<float, 4>(bcol + int64_t(cj) * ldb + p * kCsrTile);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < NP; ++p)
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[p][k] = fmaf(pj[u], z[u][p].v[k], acc[p][k]);
        }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (LPR <= 32) acc[p][k] += lane_xor<32>(acc[p][k]);
            if constexpr (LPR <= 16) acc[p][k] += lane_xor<16>(acc[p][k]);
        }
}

// The next row of the workgroup for the calling wave (wave-uniform).  Called at ONE place per loop, with all 64 lanes
// active: a `continue` in front of it gives the loop a second back edge, and the compiler then re-reads the lanes' stale
// zero instead of taking a new ticket.
__device__ __forceinline__ int csr_claim(int *s_next) {
    int v = 0;
    if (lane_id() == 0) v = atomicAdd(s_next, 1);
    return __builtin_amdgcn_readfirstlane(v);
}

// step 4 on one pack
__device__ __forceinline__ Pack<float, 4> csr_epilogue(const float (&acc)[4], const float *__restrict__ s, float ar,
                                                       int c) {
    Pack<float, 4> o;
    if (s) {
        const Pack<float, 4> sv = load_pack<float, 4>(s + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) o.v[k] = fmaf(-ar, sv.v[k], acc[k]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o.v[k] = acc[k];
    }
    return o;
}

// Workgroups [0, item_blocks): one segment of a long row per wave -> ws[item, 0:l].  The others: rows_per_block consecutive
// rows each, claimed by the waves; rows of more than kCsrSegment non-zeros are left to the items.
template <int LPR, int NP>
__global__ __launch_bounds__(kBlock) void csr_spmm_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int64_t n_rows,
    const float *__restrict__ B, int64_t ldb, int l, const float *__restrict__ a, const float *__restrict__ s,
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ seg_ptr, const int32_t *__restrict__ item_long,
    int64_t n_items, int64_t item_blocks, int rows_per_block, float *__restrict__ ws, float *__restrict__ out,
    int64_t ldo) {
    __shared__ int s_next;
    const int lane = lane_id();
    const int wave = threadIdx.x / kWave;
    const int c0 = (lane % LPR) * 4;
    bool ok[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) ok[p] = c0 + p * kCsrTile < l;
    const float *bcol = B + c0;
    float acc[NP][4];

    if (int64_t(blockIdx.x) < item_blocks) {
        const int64_t it = int64_t(blockIdx.x) * kWavesPerBlock + wave;
        if (it >= n_items) return;
        const int j = item_long[it];
        const int64_t r = long_rows[j];
        const int64_t e0 = rowptr[r] + (it - seg_ptr[j]) * kCsrSegment;
        const int64_t end = rowptr[r + 1];
        const int64_t e1 = e0 + kCsrSegment < end ? e0 + kCsrSegment : end;
        csr_segment_sum<LPR, NP>(col, val, e0, e1, bcol, ldb, ok, acc);
        if (lane < LPR) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (ok[p]) {
                    Pack<float, 4> o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o.v[k] = acc[p][k];
                    store_pack<float, 4>(ws + it * int64_t(l) + c0 + p * kCsrTile, o);
                }
        }
        return;
    }

    const int64_t r0 = (int64_t(blockIdx.x) - item_blocks) * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    if (threadIdx.x == 0) s_next = 0;
    __syncthreads();
    const int nb = int(r1 - r0);
    int cur = csr_claim(&s_next);                      // LDS: which wave takes which row changes no bit
    while (cur < nb) {                                 // one back edge, the claim at its end: as the K3 row pass
        const int64_t r = r0 + cur;
        const int64_t e0 = rowptr[r], e1 = rowptr[r + 1];
        if (e1 - e0 <= kCsrSegment) {
            csr_segment_sum<LPR, NP>(col, val, e0, e1, bcol, ldb, ok, acc);
            if (lane < LPR) {
                const float ar = a ? a[r] : 1.0f;
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    if (ok[p])
                        store_pack<float, 4>(out + r * ldo + c0 + p * kCsrTile,
                                             csr_epilogue(acc[p], s, ar, c0 + p * kCsrTile));
            }
        }
        cur = csr_claim(&s_next);
    }
}

// One wave per long row: steps 3 and 4.
__global__ __launch_bounds__(kBlock) void csr_spmm_combine_kernel(
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ seg_ptr, int64_t n_long, int l,
    const float *__restrict__ a, const float *__restrict__ s, const float *__restrict__ ws, float *__restrict__ out,
    int64_t ldo) {
    const int64_t j = int64_t(blockIdx.x) * kWavesPerBlock + threadIdx.x / kWave;
    if (j >= n_long) return;
    const int64_t r = long_rows[j];
    const int64_t k0 = seg_ptr[j], k1 = seg_ptr[j + 1];
    const float ar = a ? a[r] : 1.0f;
    for (int c = lane_id() * 4; c < l; c += kCsrTile) {
        const float *w = ws + c;
        const Pack<float, 4> first = load_pack<float, 4>(w + k0 * int64_t(l));
        float t[4] = {first.v[0], first.v[1], first.v[2], first.v[3]};
        for (int64_t k = k0 + 1; k < k1; k += 4) {
            Pack<float, 4> p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                p[u] = Pack<float, 4>{};
                if (k + u < k1) p[u] = load_pack<float, 4>(w + (k + u) * int64_t(l));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (k + u < k1) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) t[q] += p[u].v[q];
                }
        }
        store_pack<float, 4>(out + r * ldo + c, csr_epilogue(t, s, ar, c));
    }
}

// ---- row sums ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double csr_segment_value_sum(const float *__restrict__ val, int64_t e0, int64_t e1) {
    double acc = 0.0;
    for (int64_t e = e0 + lane_id(); e < e1; e += kWave) acc += double(val[e]);
    return group_sum<kWave>(acc);
}

__global__ __launch_bounds__(kBlock) void csr_row_sums_kernel(
    const int64_t *__restrict__ rowptr, const float *__restrict__ val, int64_t n_rows,
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ seg_ptr, const int32_t *__restrict__ item_long,
    int64_t n_items, int64_t item_blocks, int rows_per_block, double *__restrict__ ws, double *__restrict__ sums) {
    __shared__ int s_next;
    const int lane = lane_id();
    const int wave = threadIdx.x / kWave;
    if (int64_t(blockIdx.x) < item_blocks) {
        const int64_t it = int64_t(blockIdx.x) * kWavesPerBlock + wave;
        if (it >= n_items) return;
        const int j = item_long[it];
        const int64_t r = long_rows[j];
        const int64_t e0 = rowptr[r] + (it - seg_ptr[j]) * kCsrSegment;
        const int64_t end = rowptr[r + 1];
        const double v = csr_segment_value_sum(val, e0, e0 + kCsrSegment < end ? e0 + kCsrSegment : end);
        if (lane == 0) ws[it] = v;
        return;
    }
    const int64_t r0 = (int64_t(blockIdx.x) - item_blocks) * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    if (threadIdx.x == 0) s_next = 0;
    __syncthreads();
    const int nb = int(r1 - r0);
    int cur = csr_claim(&s_next);
    while (cur < nb) {
        const int64_t r = r0 + cur;
        const int64_t e0 = rowptr[r], e1 = rowptr[r + 1];
        if (e1 - e0 <= kCsrSegment) {
            const double v = csr_segment_value_sum(val, e0, e1);
            if (lane == 0) sums[r] = v;
        }
        cur = csr_claim(&s_next);
    }
}

__global__ __launch_bounds__(kBlock) void csr_row_sums_combine_kernel(const int32_t *__restrict__ long_rows,
                                                                      const int64_t *__restrict__ seg_ptr, int64_t n_long,
                                                                      const double *__restrict__ ws,
                                                                      double *__restrict__ sums) {
    const int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (j >= n_long) return;
    const int64_t k0 = seg_ptr[j], k1 = seg_ptr[j + 1];
    double t = ws[k0];
    for (int64_t k = k0 + 1; k < k1; ++k) t += ws[k];
    sums[long_rows[j]] = t;
}

}  // namespace clane
