// Row projection for the bilinear similarity -- Y = Z . W^T on the matrix cores.
//
// Reference being replaced: the two bias-free nn.Linear of AsymmertricSimilarity (clane/similarity.py:40-57), which
// the reference applies to z_src and z_dst of EVERY edge (graph.py:119-121: E d^2 multiply-adds twice).  Here every
// table row is projected once:  W = cat(Phi_src.weight, Phi_dst.weight) is [2d, d] row-major (nn.Linear stores
// [out, in]), so Y[r, 0:d) = Phi_src z_r and Y[r, d:2d) = Phi_dst z_r, one GEMM for both.  The pair K1
// (edge_score.h, PAIR instances) then scores edge (r, c) as dot(Y[r, 0:d), Y[c, d:2d)).
//
// Tiling: a 256-thread workgroup computes a 128 x 128 tile of Y; each of its 4 waves a 64 x 64 quarter as 4 x 4
// tiles of 16 x 16 with v_mfma_f32_16x16x4_f32 (fp32 and bf16 tables; bf16 is widened to f32 while it is staged,
// W stays f32) or v_mfma_f64_16x16x4_f64 (fp64).  K advances 16 at a time through LDS: Z's and W's 128 x 16 slices
// are staged k-contiguous per row (a lane's four k of one step are one 16-byte LDS read, conflict-free with the
// 20-word row stride), and the next slices are fetched into registers while the MFMAs run on the current ones.
// Step kk of a slice gives lane group g = lane / 16 the k index 4 g + kk, the same for the A and the B operand: the
// order in which the k terms are accumulated is a fixed permutation, identical for every element and every call.
// No atomics, no split-K: results are bit-reproducible.
//
// Any shape: K is zero-padded past d (guarded loads), partial row / column tiles are guarded on store, and the
// leading dimensions ldz >= d, ldy >= 2d are free.
#pragma once

#include "device_utils.h"

namespace clane {

constexpr int kProjBM = 128;   // rows of Z per workgroup
constexpr int kProjBN = 128;   // output columns (rows of W) per workgroup
constexpr int kProjBK = 16;    // k per LDS stage

template <typename A>
struct ProjMfma;

template <>
struct ProjMfma<float> {
    using acc4 = float __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc4 mma(float a, float b, acc4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    // C/D map of the f32 16x16x4 form: column lane & 15, row 4 (lane >> 4) + reg
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) * 4 + reg; }
};

template <>
struct ProjMfma<double> {
    using acc4 = double __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc4 mma(double a, double b, acc4 c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    // C/D map of the f64 16x16x4 form: column lane & 15, row (lane >> 4) + 4 reg
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};

// Y[rows, n_out] (ld ldy) = Z[rows, d] (ld ldz) . W[n_out, d]^T (W row-major, ld d).  One-dimensional grid: block b
// computes column tile b % n_tiles of row tile b / n_tiles, so the workgroups that read one slice of Z run together
// and Z comes from HBM once.
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void project_rows_kernel(const T *__restrict__ Z, int64_t rows, int d, int64_t ldz,
                                                              const A *__restrict__ W, int n_out, A *__restrict__ Y,
                                                              int64_t ldy, int n_tiles) {
    using M = ProjMfma<A>;
    using acc4 = typename M::acc4;
    constexpr int BM = kProjBM, BN = kProjBN, BK = kProjBK;
    constexpr int LD = BK + 16 / int(sizeof(A));          // 20 floats / 18 doubles per staged row
    constexpr int PER = BM * BK / kBlock;                 // staged elements of each operand per thread (8)
    static_assert(BM == BN && BM * BK % kBlock == 0 && kBlock % BK == 0, "staging layout");
    __shared__ __attribute__((aligned(16))) A As[BM * LD];
    __shared__ __attribute__((aligned(16))) A Bs[BN * LD];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t tile = blockIdx.x;
    const int n0 = int(tile % n_tiles) * BN;
    const int64_t m0 = (tile / n_tiles) * BM;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    const int g = lane >> 4, li = lane & 15;

    // staging: thread t moves k = t % BK of rows t / BK + (kBlock / BK) s, s < PER
    const int sk = tid % BK, si = tid / BK;
    A ra[PER], rb[PER];
    auto fetch = [&](int k0) {
        const int k = k0 + sk;
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            const int i = si + s * (kBlock / BK);
            const int64_t r = m0 + i;
            const int j = n0 + i;
            ra[s] = (k < d && r < rows) ? A(Elem<T>::to_acc(Z[r * ldz + k])) : A(0);
            rb[s] = (k < d && j < n_out) ? W[int64_t(j) * d + k] : A(0);
        }
    };

    acc4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = acc4{A(0), A(0), A(0), A(0)};

    fetch(0);
    for (int k0 = 0; k0 < d; k0 += BK) {
        __syncthreads();                                  // the previous slice has been read by every wave
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            const int i = si + s * (kBlock / BK);
            As[i * LD + sk] = ra[s];
            Bs[i * LD + sk] = rb[s];
        }
        __syncthreads();
        if (k0 + BK < d) fetch(k0 + BK);                  // in flight while the MFMAs below run
        A a[4][4], b[4][4];                               // [tile][kk]: k = 4 g + kk of rows li + 16 tile
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                a[t][kk] = As[(wm + 16 * t + li) * LD + 4 * g + kk];
                b[t][kk] = Bs[(wn + 16 * t + li) * LD + 4 * g + kk];
            }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = M::mma(a[mi][kk], b[ni][kk], acc[mi][ni]);
    }

#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int col = n0 + wn + 16 * ni + li;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t r = m0 + wm + 16 * mi + M::row(lane, reg);
                if (r < rows && col < n_out) Y[r * ldy + col] = acc[mi][ni][reg];
            }
        }
}

}  // namespace clane
