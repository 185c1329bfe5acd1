// The dense tile contraction of the library's MFMA kernels: geometry, LDS staging, the k loop and the slice step.  A
// kernel brings its operand loaders and its epilogue; the order in which the k terms of a dot are accumulated is fixed
// HERE (mfma_slice).  The two ranking kernels (link_rank.h, link_eval.h) keep their own text of the loop, which walks
// candidate tiles with the next tile's first slice in flight, and name mfma_slice as their contract.
//
// Tiling: a 256-thread workgroup computes a 32 MI x 128 tile; each of its 4 waves a 16 MI x 64 quarter as MI x 4
// tiles of 16 x 16 with v_mfma_f32_16x16x4_f32 (fp32 and bf16 tables; bf16 is widened to f32 while it is staged) or
// v_mfma_f64_16x16x4_f64 (fp64).  K advances 16 at a time through LDS: the two operands' slices are staged
// k-contiguous per row (a lane's four k of one step are one 16-byte LDS read, conflict-free with the 20-word /
// 18-double row stride), and the next slices are fetched into registers while the MFMAs run on the current ones.
// No atomics, no split-K: results are bit-reproducible.
#pragma once

#include "device_utils.h"

namespace clane {

constexpr int kProjBM = 128;   // rows of the A operand per workgroup (MI = 4)
constexpr int kProjBN = 128;   // rows of the B operand (output columns) per workgroup
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

// Geometry of a workgroup's tile and this thread's place in it (tid = threadIdx.x).
template <typename A, int MI>
struct MfmaTile {
    using M = ProjMfma<A>;
    using acc4 = typename M::acc4;
    static constexpr int BM = 32 * MI, BN = kProjBN, BK = kProjBK;
    static constexpr int LD = BK + 16 / int(sizeof(A));   // 20 floats / 18 doubles per staged row
    static constexpr int ROWS = kBlock / BK;              // rows staged side by side (16)
    static constexpr int PER_A = BM * BK / kBlock;        // staged elements per thread: 2 MI of A, 8 of B
    static constexpr int PER_B = BN * BK / kBlock;
    static constexpr int KS = kBlock / BN;                // transposed staging: k staged side by side (2) ...
    static constexpr int PER_T = BK / KS;                 // ... and k per thread and slice (8)
    static_assert(kBlock == 4 * kWave && BN == 128 && kBlock % BK == 0 && BM * BK % kBlock == 0 && BK % KS == 0,
                  "staging layout");

    int lane, wm, wn, g, li;
    __device__ __forceinline__ explicit MfmaTile(int tid)
        : lane(tid & (kWave - 1)), wm(((tid / kWave) & 1) * (16 * MI)), wn((tid / (2 * kWave)) * 64),
          g((tid & (kWave - 1)) >> 4), li(tid & 15) {}
    // tile-local (row, column) of accumulator element acc[mi][ni][reg]
    __device__ __forceinline__ int row(int mi, int reg) const { return wm + 16 * mi + M::row(lane, reg); }
    __device__ __forceinline__ int col(int ni) const { return wn + 16 * ni + li; }
};

template <typename A, int MI>
__device__ __forceinline__ void mfma_zero(typename ProjMfma<A>::acc4 (&acc)[MI][4]) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = typename ProjMfma<A>::acc4{A(0), A(0), A(0), A(0)};
}

// f(row, col, value) for every accumulator element of the thread, tile-local coordinates.
template <typename A, int MI, typename F>
__device__ __forceinline__ void mfma_for_each(const MfmaTile<A, MI> &t, const typename ProjMfma<A>::acc4 (&acc)[MI][4],
                                              F f) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int col = t.col(ni);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) f(t.row(mi, reg), col, acc[mi][ni][reg]);
        }
}

// The slice step: one staged 16-wide k slice into the accumulators.  Step kk gives lane group g = lane / 16 the k index
// 4 g + kk, the same for the A and the B operand, and the steps run kk = 0..3 for every accumulator: the order in which
// the k terms of a dot are accumulated is a fixed permutation, identical for every element, every kernel and every
// call.  It does not depend on the tile, the slab or the lane a (row, column) pair falls in -- what the library
// promises about equal bits (link_rank.h, link_eval.h, label_probe.h, kmeans.h) rests on this one loop.
template <typename A, int MI>
__device__ __forceinline__ void mfma_slice(const MfmaTile<A, MI> &t, const A *As, const A *Bs,
                                           typename ProjMfma<A>::acc4 (&acc)[MI][4]) {
    using Tile = MfmaTile<A, MI>;
    A a[MI][4], b[4][4];                                  // [tile][kk]: k = 4 g + kk of rows li + 16 tile
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
        for (int i = 0; i < MI; ++i) a[i][kk] = As[(t.wm + 16 * i + t.li) * Tile::LD + 4 * t.g + kk];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i][kk] = Bs[(t.wn + 16 * i + t.li) * Tile::LD + 4 * t.g + kk];
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = Tile::M::mma(a[mi][kk], b[ni][kk], acc[mi][ni]);
}

// acc += A-operand . B-operand^T over k in [0, d), both operands staged row-major: thread t moves k = t % BK of rows
// t / BK + 16 s.  The loaders load_a / load_b(slot s, staged row, k) return the guarded element (zero past d, past the
// operand's rows); the slot index lets a kernel keep per-slot offsets of gathered rows.
template <typename A, int MI, typename LA, typename LB>
__device__ __forceinline__ void mfma_tile_product(const MfmaTile<A, MI> &t, A *As, A *Bs, int d,
                                                  typename ProjMfma<A>::acc4 (&acc)[MI][4], LA load_a, LB load_b) {
    using Tile = MfmaTile<A, MI>;
    const int sk = int(threadIdx.x) % Tile::BK, si = int(threadIdx.x) / Tile::BK;
    A ra[Tile::PER_A], rb[Tile::PER_B];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int s = 0; s < Tile::PER_A; ++s) ra[s] = load_a(s, si + s * Tile::ROWS, k0 + sk);
#pragma unroll
        for (int s = 0; s < Tile::PER_B; ++s) rb[s] = load_b(s, si + s * Tile::ROWS, k0 + sk);
    };
    fetch(0);
    for (int k0 = 0; k0 < d; k0 += Tile::BK) {
        __syncthreads();                                  // the previous slice has been read by every wave
#pragma unroll
        for (int s = 0; s < Tile::PER_A; ++s) As[(si + s * Tile::ROWS) * Tile::LD + sk] = ra[s];
#pragma unroll
        for (int s = 0; s < Tile::PER_B; ++s) Bs[(si + s * Tile::ROWS) * Tile::LD + sk] = rb[s];
        __syncthreads();
        if (k0 + Tile::BK < d) fetch(k0 + Tile::BK);      // in flight while the MFMAs below run
        mfma_slice(t, As, Bs, acc);
    }
}

// The transposed staging of the gradient kernels (MI = 4): the contraction index k runs over [kbeg, kend) in memory's
// slow direction, so thread t stages row t % 128 of both operands for k = t / 128 + 2 s of each slice (consecutive
// threads: consecutive rows of one k -- coalesced).  load(k, a, b) fills the two elements of an existing k (they are
// zero otherwise); staged(a) sees every A element the thread stages, in k order.
template <typename A, typename Load, typename Staged>
__device__ __forceinline__ void mfma_tile_product_transposed(const MfmaTile<A, 4> &t, A *As, A *Bs, int64_t kbeg,
                                                             int64_t kend, typename ProjMfma<A>::acc4 (&acc)[4][4],
                                                             Load load, Staged staged) {
    using Tile = MfmaTile<A, 4>;
    const int so = int(threadIdx.x) % Tile::BM, sk = int(threadIdx.x) / Tile::BM;
    A ra[Tile::PER_T], rb[Tile::PER_T];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int s = 0; s < Tile::PER_T; ++s) {
            const int64_t k = k0 + sk + Tile::KS * s;
            ra[s] = A(0);
            rb[s] = A(0);
            if (k < kend) load(k, ra[s], rb[s]);
        }
    };
    fetch(kbeg);
    for (int64_t k0 = kbeg; k0 < kend; k0 += Tile::BK) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < Tile::PER_T; ++s) {
            As[so * Tile::LD + sk + Tile::KS * s] = ra[s];
            Bs[so * Tile::LD + sk + Tile::KS * s] = rb[s];
            staged(ra[s]);
        }
        __syncthreads();
        if (k0 + Tile::BK < kend) fetch(k0 + Tile::BK);
        mfma_slice(t, As, Bs, acc);
    }
}

// Offsets of the gathered A-operand rows of this thread's staging slots: row m0 + (staged row) of the list idx[0, n),
// times the leading dimension; < 0: no such row (past the list, or an index outside [0, table_rows)).
template <int PER>
__device__ __forceinline__ void mfma_gather_offsets(const int32_t *__restrict__ idx, int64_t m0, int64_t n,
                                                    int64_t table_rows, int64_t ld, int64_t (&roff)[PER]) {
#pragma unroll
    for (int s = 0; s < PER; ++s) {
        const int64_t r = m0 + int(threadIdx.x) / kProjBK + s * (kBlock / kProjBK);
        int64_t t = -1;
        if (r < n) {
            t = idx[r];
            if (t >= table_rows) t = -1;
        }
        roff[s] = t < 0 ? -1 : t * ld;
    }
}

}  // namespace clane
