// extern "C" surface of libclane_hip.so (see include/clane_hip.h): argument validation,
// lane-layout selection and kernel launches.  No allocation, no synchronisation, no state.
#include "../../include/clane_hip.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "build_p.h"
#include "content_pca.h"
#include "edge_score.h"
#include "device_utils.h"
#include "kmeans.h"
#include "label_predict.h"
#include "label_probe.h"
#include "multilabel_probe.h"
#include "new_rows.h"
#include "link_eval.h"
#include "link_rank.h"
#include "mixture.h"
#include "pair_train.h"
#include "projection.h"
#include "sparse_rows.h"
#include "spmm_update.h"
#include "silhouette.h"
#include "tsne.h"
#include "tsne_nn.h"

namespace {

using namespace clane;

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CLANE_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return CLANE_OK;
}

constexpr int kReduceGrid = 1024;              // partial blocks of the two-stage reductions
constexpr int64_t kReduceWs = 2 * kReduceGrid + 2;  // + the two finished sums
#ifndef CLANE_LONG_U
#define CLANE_LONG_U CLANE_SPMM_U    // neighbour-row loads in flight per wave of the workgroup-per-row kernels
#endif
#ifndef CLANE_SUBROW_U32
#define CLANE_SUBROW_U32 4        // CLANE_SPMM_TABLE_BEYOND_CACHE: row loads in flight in spmm_update_subrow_kernel, two fp32 rows per instruction
#endif
#ifndef CLANE_CLASS_U16B
#define CLANE_CLASS_U16B 4        // ... and in its instance with four bf16 rows per instruction (config 4)
#endif
#ifndef CLANE_CLASS_U32
#define CLANE_CLASS_U32 6         // ... and in spmm_class_chunk_kernel (72 registers: 7 waves per SIMD instead of 5)
#endif
#ifndef CLANE_LONG_WAVES
#define CLANE_LONG_WAVES 16         // waves of the workgroup-per-row kernels (A/B builds: 8)
#endif
constexpr int kLongWaves = CLANE_LONG_WAVES;
#ifndef CLANE_ROWS_PER_BLOCK
#define CLANE_ROWS_PER_BLOCK 32   // minimum consecutive rows per workgroup of the row kernels
#endif

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Row kernels (K1, K2, K3): a workgroup owns `rows_per_block` consecutive rows.  The grid aims at ~32k workgroups
// (>> the 2048 resident ones, so the dispatcher load-balances skewed rows) of at least CLANE_ROWS_PER_BLOCK rows:
// a workgroup's start-up -- rowptr slice to LDS, barrier, first claims -- is a chain of dependent round trips, and
// with 8 rows per wave-instruction (128-byte rows) 32 rows are ONE row per sub-wave.  Measured
// (profiles/r02_ab_rows_per_block.md): 2M rows x 128 B 0.760 -> 0.712 ms at 64 rows; 10M rows bf16 8.6 -> 8.2 ms at
// 256; a 200k-row graph loses 12 % above 32 (too few workgroups), 2M rows lose 30 % at 256.
#ifndef CLANE_TARGET_GRID
#define CLANE_TARGET_GRID 32768
#endif
inline int rows_per_block(int64_t nrows) {
    const int64_t r = ceil_div(ceil_div(nrows, CLANE_TARGET_GRID), kWavesPerBlock) * kWavesPerBlock;
    return int(r < CLANE_ROWS_PER_BLOCK ? CLANE_ROWS_PER_BLOCK : r > kMaxRowsPerBlock ? kMaxRowsPerBlock : r);
}
inline int row_grid(int64_t nrows) { return int(ceil_div(nrows > 0 ? nrows : 1, rows_per_block(nrows))); }

inline int grid_for_waves(int64_t nwaves_wanted) {
    int64_t g = ceil_div(nwaves_wanted, kWavesPerBlock);
    if (g > kMaxGrid) g = kMaxGrid;
    if (g < 1) g = 1;
    return int(g);
}

// Lane layout: 16-byte packs when every operand allows it, else one element per lane.
struct Layout {
    bool vec;  // 16-byte path
    int lpr;   // lanes per row (power of two)
};

template <typename T>
Layout pick_layout(int d, std::initializer_list<const void *> ptrs, std::initializer_list<int64_t> lds) {
    constexpr int KV = Elem<T>::kVec;
    bool vec = true;
    for (const void *p : ptrs) vec = vec && aligned16(p);
    for (int64_t ld : lds) vec = vec && (ld % KV == 0);
    Layout L;
    L.vec = vec;
    if (vec) {
        const int packs = int(ceil_div(d, KV));
        L.lpr = packs <= 8 ? 8 : packs <= 16 ? 16 : packs <= 32 ? 32 : 64;
    } else {
        L.lpr = d <= 4 ? 4 : d <= 16 ? 16 : 64;
    }
    return L;
}

// Calls f.template operator()<VEC, LPR>() for the chosen layout.
template <typename T, typename F>
void dispatch_layout(const Layout &L, F &&f) {
    constexpr int KV = Elem<T>::kVec;
    if (L.vec) {
        switch (L.lpr) {
            case 8: f.template operator()<KV, 8>(); break;
            case 16: f.template operator()<KV, 16>(); break;
            case 32: f.template operator()<KV, 32>(); break;
            default: f.template operator()<KV, 64>(); break;
        }
    } else {
        switch (L.lpr) {
            case 4: f.template operator()<1, 4>(); break;
            case 16: f.template operator()<1, 16>(); break;
            default: f.template operator()<1, 64>(); break;
        }
    }
}

template <typename T>
Mirror<T> make_mirror(const clane_mirror_t *m) {
    if (m == nullptr || m->row_ptr == nullptr) return Mirror<T>{nullptr, nullptr, nullptr, 0};
    return Mirror<T>{m->row_ptr, m->slot, reinterpret_cast<T *const *>(m->bufs), m->ld};
}
// The bases live in device memory: the caller vouches for their alignment; a mirror that is not 16-byte
// aligned sends the call down the scalar path (an odd address in the alignment check).
inline const void *mirror_alignment_probe(const clane_mirror_t *m, const void *aligned) {
    return (m && m->row_ptr && !m->aligned16) ? reinterpret_cast<const void *>(uintptr_t(1)) : aligned;
}
inline bool mirror_ok(const clane_mirror_t *m, int d) {
    return m == nullptr || m->row_ptr == nullptr || (m->slot != nullptr && m->bufs != nullptr && m->ld >= d);
}

// The tables of a K3 call: Z_new = f(Z_old, X, gamma) over d columns, copied to the mirror's places where there is one.
// Every K3 launcher asks its questions of this one place; each reports them under its own name, in its own order.
template <typename T>
struct Tables {
    const T *Z_old;
    int64_t ldz;
    const T *X;
    int64_t ldx;
    typename Elem<T>::acc_t gamma;
    T *Z_new;
    int64_t ldo;
    int32_t d;
    const clane_mirror_t *mirror;

    bool mirror_complete() const { return mirror_ok(mirror, d); }
    bool wide_enough() const { return ldz >= d && ldx >= d && ldo >= d; }
    bool present() const { return Z_old && X && Z_new; }
    bool aliased() const { return (const void *)Z_new == (const void *)Z_old; }
    Mirror<T> mir() const { return make_mirror<T>(mirror); }
    // the lane layout of a launch over `width` columns a tile (the whole d of a per-tile call)
    Layout layout(int width) const {
        return pick_layout<T>(width, {Z_old, X, Z_new, mirror_alignment_probe(mirror, Z_new)},
                              {ldz, ldx, ldo, mirror && mirror->row_ptr ? mirror->ld : ldo});
    }
};
template <typename T, typename CT, typename GT>
Tables<T> tables(const CT *Z_old, int64_t ldz, const CT *X, int64_t ldx, GT gamma, CT *Z_new, int64_t ldo, int32_t d,
                 const clane_mirror_t *mirror = nullptr) {
    return {reinterpret_cast<const T *>(Z_old), ldz, reinterpret_cast<const T *>(X), ldx, gamma,
            reinterpret_cast<T *>(Z_new), ldo, d, mirror};
}

#define REQUIRE(cond, ...) \
    do {                   \
        if (!(cond)) return fail(CLANE_ERR_INVALID_ARGUMENT, __VA_ARGS__); \
    } while (0)

// ---------------------------------------------------------------------------------------------
template <typename T>
int row_sqnorm(const T *Z, int64_t nrows, int32_t d, int64_t ldz, typename Elem<T>::acc_t *sq, void *stream) {
    REQUIRE(nrows >= 0 && d > 0 && ldz >= d, "row_sqnorm: bad shape nrows=%lld d=%d ldz=%lld", (long long)nrows, d,
            (long long)ldz);
    if (nrows == 0) return CLANE_OK;
    REQUIRE(Z && sq, "row_sqnorm: null pointer");
    const Layout L = pick_layout<T>(d, {Z}, {ldz});
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        const int grid = grid_for_waves(ceil_div(nrows, (kWave / LPR) * stream_rows(LPR)));
        row_sqnorm_kernel<T, VEC, LPR><<<grid, kBlock, 0, (hipStream_t)stream>>>(Z, nrows, d, ldz, sq);
    });
    return check_launch("row_sqnorm");
}

template <typename A>
int degree_weighted_sums(const A *sq, const int64_t *rowptr, const int32_t *indeg, int64_t nrows, double *ws,
                         double *out2, void *stream) {
    REQUIRE(nrows >= 0, "degree_weighted_sums: nrows < 0");
    REQUIRE(ws && out2, "degree_weighted_sums: null workspace/output");
    REQUIRE(nrows == 0 || (sq && rowptr && indeg), "degree_weighted_sums: null pointer");
    int grid = int(ceil_div(nrows > 0 ? nrows : 1, kBlock));
    if (grid > kReduceGrid) grid = kReduceGrid;
    degree_weighted_kernel<A><<<grid, kBlock, 0, (hipStream_t)stream>>>(sq, rowptr, indeg, nrows, ws);
    reduce_fixed_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(ws, grid, grid, 2, out2);
    return check_launch("degree_weighted_sums");
}

template <typename T>
int edge_score(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0, const T *Z, int64_t ldz,
               int32_t d, int32_t mode, const double *sums2, const typename Elem<T>::acc_t *sq,
               typename Elem<T>::acc_t *scores, int32_t flags, int64_t long_threshold, const int32_t *long_rows,
               int64_t n_long, void *stream) {
    REQUIRE(nrows >= 0 && row0 >= 0 && d > 0 && ldz >= d, "edge_score: bad shape");
    REQUIRE(mode == CLANE_SCORE_REFERENCE || mode == CLANE_SCORE_PER_EDGE || mode == CLANE_SCORE_RAW_DOT,
            "edge_score: unknown mode %d", mode);
    REQUIRE(long_threshold >= 0 && n_long >= 0 && n_long <= INT32_MAX, "edge_score: bad long-row parameters");
    REQUIRE(n_long == 0 || (long_rows && long_threshold > 0), "edge_score: long_rows needs a list and a threshold");
    if (nrows == 0) return CLANE_OK;
    REQUIRE(rowptr && colidx && Z && scores, "edge_score: null pointer");
    REQUIRE(mode != CLANE_SCORE_REFERENCE || sums2, "edge_score: mode REFERENCE needs sums2");
    REQUIRE(mode != CLANE_SCORE_PER_EDGE || sq, "edge_score: mode PER_EDGE needs sq");
    const Layout L = pick_layout<T>(d, {Z}, {ldz});
    const bool fuse = (flags & CLANE_SCORE_FUSE_SOFTMAX) != 0;
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        constexpr int U = VEC > 1 ? 8 : 4;
        if constexpr (LPR < kWave && VEC > 1)      // narrow rows: one sub-wave per source row
            edge_score_subrow_kernel<T, VEC, LPR, U><<<row_grid(nrows), kBlock, 0, (hipStream_t)stream>>>(
                rowptr, colidx, nrows, row0, Z, ldz, d, mode, sums2, sq, scores, long_threshold, fuse,
                rows_per_block(nrows));
        else
            edge_score_kernel<T, VEC, LPR, U><<<row_grid(nrows), kBlock, 0, (hipStream_t)stream>>>(
                rowptr, colidx, nrows, row0, Z, ldz, d, mode, sums2, sq, scores, long_threshold, fuse,
                rows_per_block(nrows));
        if (n_long > 0)
            edge_score_long_kernel<T, VEC, LPR, U, kLongWaves>
                <<<unsigned(n_long), kLongWaves * kWave, 0, (hipStream_t)stream>>>(
                    rowptr, colidx, long_rows, row0, Z, ldz, d, mode, sums2, sq, scores, fuse);
    });
    return check_launch("edge_score");
}

template <typename T>
int edge_score_class(const int64_t *rowptr, const int32_t *colidx, const int64_t *item_e0, const int32_t *item_len,
                     const int32_t *item_slot, const int32_t *item_row, int64_t n_blocks, int32_t items_per_block,
                     const int32_t *class_rows, const int64_t *slot_ptr, int64_t n_rows, int64_t row0, const T *Z,
                     int64_t ldz, int32_t d, int32_t mode, const double *sums2, const typename Elem<T>::acc_t *sq,
                     typename Elem<T>::acc_t *scores, int32_t flags, typename Elem<T>::acc_t *stats, void *stream) {
    REQUIRE(n_blocks >= 0 && n_blocks <= INT32_MAX && n_rows >= 0 && n_rows <= INT32_MAX && row0 >= 0 && d > 0 &&
                ldz >= d,
            "edge_score_class: bad shape");
    REQUIRE(items_per_block >= kWavesPerBlock && items_per_block <= kMaxItemsPerBlock,
            "edge_score_class: items_per_block must be in [%d, %d]", kWavesPerBlock, kMaxItemsPerBlock);
    REQUIRE(mode == CLANE_SCORE_REFERENCE || mode == CLANE_SCORE_PER_EDGE || mode == CLANE_SCORE_RAW_DOT,
            "edge_score_class: unknown mode %d", mode);
    if (n_rows == 0 || n_blocks == 0) return CLANE_OK;
    const bool fuse = (flags & CLANE_SCORE_FUSE_SOFTMAX) != 0;
    REQUIRE(colidx && item_e0 && item_len && item_slot && item_row && Z && scores, "edge_score_class: null pointer");
    REQUIRE(!fuse || (rowptr && class_rows && slot_ptr && stats),
            "edge_score_class: CLANE_SCORE_FUSE_SOFTMAX needs rowptr, class_rows, slot_ptr and stats");
    REQUIRE(mode != CLANE_SCORE_REFERENCE || sums2, "edge_score_class: mode REFERENCE needs sums2");
    REQUIRE(mode != CLANE_SCORE_PER_EDGE || sq, "edge_score_class: mode PER_EDGE needs sq");
    const Layout L = pick_layout<T>(d, {Z}, {ldz});
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        constexpr int U = VEC > 1 ? 8 : 4;
        edge_score_class_kernel<T, VEC, LPR, U><<<unsigned(n_blocks), kBlock, 0, (hipStream_t)stream>>>(
            colidx, item_e0, item_len, item_slot, item_row, items_per_block, row0, Z, ldz, d, mode, sums2, sq, scores,
            fuse ? stats : nullptr);
    });
    if (fuse) {
        int parts = (flags >> 8) & 0xff;        // CLANE_SCORE_ROW_PARTS(n): workgroups per row of the rescale pass
        if (parts < 1) parts = 1;
        edge_softmax_class_kernel<typename Elem<T>::acc_t>
            <<<dim3(unsigned(n_rows), unsigned(parts)), kBlock, 0, (hipStream_t)stream>>>(rowptr, class_rows, slot_ptr,
                                                                                            stats, scores);
    }
    return check_launch("edge_score_class");
}

// ---- bilinear similarity: projection + pair K1 ----------------------------------------------------------------
template <typename T, typename A>
int project_rows(const T *Z, int64_t rows, int32_t d, int64_t ldz, const A *W, A *Y, int64_t ldy, void *stream) {
    REQUIRE(rows >= 0 && d > 0 && d <= INT32_MAX / 2 && ldz >= d && ldy >= 2 * int64_t(d),
            "project_rows: bad shape rows=%lld d=%d ldz=%lld ldy=%lld", (long long)rows, d, (long long)ldz,
            (long long)ldy);
    if (rows == 0) return CLANE_OK;
    REQUIRE(Z && W && Y, "project_rows: null pointer");
    const int n_out = 2 * d;
    const int n_tiles = int(ceil_div(int64_t(n_out), int64_t(kProjBN)));
    const int64_t blocks = ceil_div(rows, int64_t(kProjBM)) * n_tiles;
    REQUIRE(blocks <= INT32_MAX, "project_rows: %lld rows is too many for one launch", (long long)rows);
    project_rows_kernel<T, A><<<unsigned(blocks), kBlock, 0, (hipStream_t)stream>>>(Z, rows, d, ldz, W, n_out, Y, ldy,
                                                                                     n_tiles);
    return check_launch("project_rows");
}

template <typename T>
int edge_score_pair(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0, const T *S, int64_t lds,
                    const T *N, int64_t ldn, int32_t d, T *scores, int32_t flags, int64_t long_threshold,
                    const int32_t *long_rows, int64_t n_long, void *stream) {
    REQUIRE(nrows >= 0 && row0 >= 0 && d > 0 && lds >= d && ldn >= d, "edge_score_pair: bad shape");
    REQUIRE(long_threshold >= 0 && n_long >= 0 && n_long <= INT32_MAX, "edge_score_pair: bad long-row parameters");
    REQUIRE(n_long == 0 || (long_rows && long_threshold > 0), "edge_score_pair: long_rows needs a list and a threshold");
    if (nrows == 0) return CLANE_OK;
    REQUIRE(rowptr && colidx && S && N && scores, "edge_score_pair: null pointer");
    const Layout L = pick_layout<T>(d, {S, N}, {lds, ldn});
    const bool fuse = (flags & CLANE_SCORE_FUSE_SOFTMAX) != 0;
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        constexpr int U = VEC > 1 ? 8 : 4;
        if constexpr (LPR < kWave && VEC > 1)
            edge_score_pair_subrow_kernel<T, VEC, LPR, U><<<row_grid(nrows), kBlock, 0, (hipStream_t)stream>>>(
                rowptr, colidx, nrows, row0, S, lds, N, ldn, d, scores, long_threshold, fuse, rows_per_block(nrows));
        else
            edge_score_pair_kernel<T, VEC, LPR, U><<<row_grid(nrows), kBlock, 0, (hipStream_t)stream>>>(
                rowptr, colidx, nrows, row0, S, lds, N, ldn, d, scores, long_threshold, fuse, rows_per_block(nrows));
        if (n_long > 0)
            edge_score_pair_long_kernel<T, VEC, LPR, U, kLongWaves>
                <<<unsigned(n_long), kLongWaves * kWave, 0, (hipStream_t)stream>>>(rowptr, colidx, long_rows, row0, S,
                                                                                   lds, N, ldn, d, scores, fuse);
    });
    return check_launch("edge_score_pair");
}

template <typename T>
int edge_score_class_pair(const int64_t *rowptr, const int32_t *colidx, const int64_t *item_e0, const int32_t *item_len,
                          const int32_t *item_slot, const int32_t *item_row, int64_t n_blocks, int32_t items_per_block,
                          const int32_t *class_rows, const int64_t *slot_ptr, int64_t n_rows, int64_t row0, const T *S,
                          int64_t lds, const T *N, int64_t ldn, int32_t d, T *scores, int32_t flags, T *stats,
                          void *stream) {
    REQUIRE(n_blocks >= 0 && n_blocks <= INT32_MAX && n_rows >= 0 && n_rows <= INT32_MAX && row0 >= 0 && d > 0 &&
                lds >= d && ldn >= d,
            "edge_score_class_pair: bad shape");
    REQUIRE(items_per_block >= kWavesPerBlock && items_per_block <= kMaxItemsPerBlock,
            "edge_score_class_pair: items_per_block must be in [%d, %d]", kWavesPerBlock, kMaxItemsPerBlock);
    if (n_rows == 0 || n_blocks == 0) return CLANE_OK;
    const bool fuse = (flags & CLANE_SCORE_FUSE_SOFTMAX) != 0;
    REQUIRE(colidx && item_e0 && item_len && item_slot && item_row && S && N && scores,
            "edge_score_class_pair: null pointer");
    REQUIRE(!fuse || (rowptr && class_rows && slot_ptr && stats),
            "edge_score_class_pair: CLANE_SCORE_FUSE_SOFTMAX needs rowptr, class_rows, slot_ptr and stats");
    const Layout L = pick_layout<T>(d, {S, N}, {lds, ldn});
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        constexpr int U = VEC > 1 ? 8 : 4;
        edge_score_pair_class_kernel<T, VEC, LPR, U><<<unsigned(n_blocks), kBlock, 0, (hipStream_t)stream>>>(
            colidx, item_e0, item_len, item_slot, item_row, items_per_block, row0, S, lds, N, ldn, d, scores,
            fuse ? stats : nullptr);
    });
    if (fuse) {
        int parts = (flags >> 8) & 0xff;
        if (parts < 1) parts = 1;
        edge_softmax_class_kernel<T><<<dim3(unsigned(n_rows), unsigned(parts)), kBlock, 0, (hipStream_t)stream>>>(
            rowptr, class_rows, slot_ptr, stats, scores);
    }
    return check_launch("edge_score_class_pair");
}

template <typename A>
int segment_softmax(const int64_t *rowptr, int64_t nrows, A *vals, int64_t min_degree, int64_t max_degree,
                    const int32_t *long_rows, int64_t n_long, void *stream) {
    REQUIRE(nrows >= 0 && min_degree >= 0 && max_degree >= 0 && n_long >= 0 && n_long <= INT32_MAX,
            "segment_softmax: negative argument");
    REQUIRE(n_long == 0 || (long_rows && max_degree > 0), "segment_softmax: long_rows needs a list and max_degree");
    if (nrows == 0) return CLANE_OK;
    REQUIRE(rowptr && vals, "segment_softmax: null pointer");
    if (!(max_degree > 0 && max_degree <= min_degree))
        segment_softmax_kernel<A><<<row_grid(nrows), kBlock, 0, (hipStream_t)stream>>>(
            rowptr, nrows, vals, min_degree, max_degree, rows_per_block(nrows));
    if (n_long > 0)
        segment_softmax_long_kernel<A, kLongWaves><<<unsigned(n_long), kLongWaves * kWave, 0, (hipStream_t)stream>>>(
            rowptr, long_rows, vals, min_degree);
    return check_launch("segment_softmax");
}

template <typename A>
int edge_score_finalize(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0, int32_t mode,
                        const double *sums2, const A *sq, A *scores, void *stream) {
    REQUIRE(nrows >= 0 && row0 >= 0, "edge_score_finalize: bad shape");
    REQUIRE(mode == CLANE_SCORE_REFERENCE || mode == CLANE_SCORE_PER_EDGE || mode == CLANE_SCORE_RAW_DOT,
            "edge_score_finalize: unknown mode %d", mode);
    if (nrows == 0 || mode == CLANE_SCORE_RAW_DOT) return CLANE_OK;
    REQUIRE(rowptr && colidx && scores, "edge_score_finalize: null pointer");
    REQUIRE(mode != CLANE_SCORE_REFERENCE || sums2, "edge_score_finalize: reference mode needs sums2");
    REQUIRE(mode != CLANE_SCORE_PER_EDGE || sq, "edge_score_finalize: per_edge mode needs sq");
    edge_score_finalize_kernel<A><<<row_grid(nrows), kBlock, 0, (hipStream_t)stream>>>(
        rowptr, colidx, nrows, row0, mode, sums2, sq, scores, rows_per_block(nrows));
    return check_launch("edge_score_finalize");
}

// One weight per row where build_P left a row uniform (build_p.h, row_weight_kernel); mixed[0] = 0 before, |= 1 by the kernel.
template <typename A>
int row_weights(const int64_t *rowptr, const A *P, int64_t nrows, A *w, int32_t *mixed, void *stream) {
    REQUIRE(nrows >= 0, "row_weight: bad shape nrows=%lld", (long long)nrows);
    REQUIRE(mixed, "row_weight: null mixed");
    const hipError_t e = hipMemsetAsync(mixed, 0, sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) return fail(CLANE_ERR_LAUNCH, "row_weight: %s", hipGetErrorString(e));
    if (nrows == 0) return CLANE_OK;
    REQUIRE(rowptr && P && w, "row_weight: null pointer");
    row_weight_kernel<A><<<row_grid(nrows), kBlock, 0, (hipStream_t)stream>>>(rowptr, P, nrows, w, mixed,
                                                                             rows_per_block(nrows));
    return check_launch("row_weight");
}

inline int64_t spmm_main_grid(int64_t nrows) { return row_grid(nrows); }

// Column tiles of a pass: tile t covers columns [t * cols, min(d, (t + 1) * cols)).  Each pass has ONE launcher, and the
// per-tile call is its one-tile case {d, 0}: the same checks, the same kernel instance (picked by the width of a full
// tile) and the same grid arithmetic, which is what makes a fused launch bit for bit the per-tile launches.  FUSED, a
// template parameter that only the three *_tiles_f32 entry points set, decides nothing but which kernel entry receives
// the arguments: the plain kernel with MIRRORED, or the *_tiles_kernel with a TileGrid (float, 16-byte packs only).
struct Tiles {
    int32_t cols;           // columns of every tile but the last, which takes what is left of d
    int64_t part_stride;    // between the tiles' delta partials
};
inline int tile_count(int d, int tile_cols) { return int(ceil_div(d, tile_cols)); }
// One instance serves all tiles of a fused launch, so the last (narrower) tile must have the lane layout of a full one.
template <typename T>
bool tiles_share_layout(int d, int tile_cols) {
    constexpr int KV = Elem<T>::kVec;
    auto lanes = [](int w) { const int p = int(ceil_div(w, KV)); return p <= 8 ? 8 : p <= 16 ? 16 : p <= 32 ? 32 : 64; };
    return tile_cols % KV == 0 && lanes(d - (tile_count(d, tile_cols) - 1) * tile_cols) == lanes(tile_cols);
}
#define REQUIRE_TILES(T, d, tiles, what, and_ok, and_text)                                                             \
    REQUIRE((tiles).cols > 0 && (tiles).cols <= (d) && (and_ok) && tiles_share_layout<T>(d, (tiles).cols),            \
            "%s: tile_cols must be a multiple of the 16-byte pack in (0, d] whose last tile keeps the lane layout"    \
            and_text " (d=%d tile_cols=%d)", what, d, (tiles).cols)

// The row pass's kernel entries, per tile and fused: one sub-wave per row for the short rows of narrow matrices
template <typename T, typename PT, int VEC, int LPR, int U, bool MIRRORED, bool UNIFORM>
constexpr auto row_kernel() {
    if constexpr (LPR < kWave && VEC > 1) return &spmm_update_subrow_kernel<T, PT, VEC, LPR, U, MIRRORED, UNIFORM>;
    else return &spmm_update_kernel<T, PT, VEC, LPR, U, MIRRORED, UNIFORM>;
}
template <typename T, typename PT, int VEC, int LPR, int U, bool UNIFORM>
constexpr auto row_tiles_kernel() {
    if constexpr (LPR < kWave) return &spmm_update_subrow_tiles_kernel<T, PT, VEC, LPR, U, UNIFORM>;
    else return &spmm_update_tiles_kernel<T, PT, VEC, LPR, U, UNIFORM>;
}

// UNIFORM, in the three K3 launchers that take it (the *_rw_f32 entry points): `P` holds one weight per ROW of the call
// (clane_row_weight_* found every row of P uniform), the kernels are the UNIFORM instances of spmm_update.h, there is no
// mirror.  Everything else -- checks, instance choice, grids -- is the per-edge call's, which is what keeps the two bit for bit.
template <typename T, typename PT, bool FUSED, bool UNIFORM = false>
int spmm_update_impl(const char *what, const int64_t *rowptr, const int32_t *colidx, const PT *P, int64_t nrows,
                     int64_t row0, const Tables<T> &t, Tiles tiles, int64_t long_threshold, int32_t flags,
                     double *delta_partials, void *stream) {
    const int32_t d = t.d;
    REQUIRE(nrows >= 0 && row0 >= 0 && d > 0, "%s: bad shape nrows=%lld row0=%lld d=%d", what, (long long)nrows,
            (long long)row0, d);
    if constexpr (FUSED) REQUIRE_TILES(T, d, tiles, what, true, "");
    REQUIRE(t.mirror_complete(), "%s: incomplete mirror descriptor", what);
    if constexpr (UNIFORM) REQUIRE(t.mirror == nullptr, "%s: no mirror with per-row weights", what);
    REQUIRE(t.wide_enough(), "%s: leading dimension < d", what);
    REQUIRE(long_threshold >= 0, "%s: negative long_threshold", what);
    REQUIRE(delta_partials, "%s: null delta_partials", what);
    const int n_tiles = tile_count(d, tiles.cols);
    const int per_tile = int(spmm_main_grid(nrows));
    REQUIRE(tiles.part_stride >= (n_tiles > 1 ? per_tile : 0), "%s: the tiles' partials overlap", what);
    REQUIRE(int64_t(n_tiles) * per_tile <= INT32_MAX, "%s: grid too large", what);
    if (nrows == 0) return CLANE_OK;
    REQUIRE(rowptr && colidx && P && t.present(), "%s: null pointer", what);
    REQUIRE(!t.aliased(), "%s: Z_new must not alias Z_old (Jacobi sweep)", what);
    const Layout L = t.layout(tiles.cols);
    if constexpr (FUSED) REQUIRE(L.vec, "%s: the tables must allow 16-byte packs", what);
    const unsigned grid = unsigned(n_tiles) * unsigned(per_tile);
    const bool sinks = (flags & CLANE_SPMM_SINKS_UNTOUCHED) != 0, beyond = (flags & CLANE_SPMM_TABLE_BEYOND_CACHE) != 0;
    const Mirror<T> mir = t.mir();
    const TileGrid tg{per_tile, tiles.cols, tiles.part_stride};
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        auto launch = [&]<int U>() {
            auto go = [&](auto *kernel, auto... how) {
                kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(rowptr, colidx, P, nrows, row0, t.Z_old, t.ldz, t.X, t.ldx,
                                                                 t.gamma, t.Z_new, t.ldo, d, long_threshold, sinks,
                                                                 rows_per_block(nrows), how..., delta_partials);
            };
            if constexpr (FUSED) {
                if constexpr (VEC > 1) go(row_tiles_kernel<T, PT, VEC, LPR, U, UNIFORM>(), beyond, tg);
            } else if constexpr (UNIFORM) {
                go(row_kernel<T, PT, VEC, LPR, U, false, true>(), mir, beyond);
            } else if (mir.row_ptr != nullptr) {   // the mirrored instances prefetch a row's places (spmm_update.h)
                go(row_kernel<T, PT, VEC, LPR, U, true, false>(), mir, beyond);
            } else {
                go(row_kernel<T, PT, VEC, LPR, U, false, false>(), mir, beyond);
            }
        };
        // two fp32 rows per instruction (512-byte rows: the column tiles, config 2, the N = 2 column slices): with the
        // table far beyond the caches 4 row loads in flight and 8 waves per SIMD beat 8 and 6 (config 3 in two
        // tiles: row pass 1.58 -> 1.52 ms); a cache-resident table wants the 8 (config 2: 0.103 vs 0.120 ms)
        if constexpr (LPR == 32 && VEC == 4 && sizeof(T) == 4) {
            if (beyond) return launch.template operator()<CLANE_SUBROW_U32>();
        }
        launch.template operator()<(VEC > 1 ? CLANE_SPMM_U : 4)>();
    });
    return check_launch(what);
}

template <typename T, typename PT>
int spmm_update_long(const int64_t *rowptr, const int32_t *colidx, const PT *P, const int32_t *long_rows,
                     int64_t n_long, int32_t waves_per_row, int64_t row0, const Tables<T> &t, double *delta_partials,
                     void *stream) {
    const int32_t d = t.d;
    REQUIRE(n_long >= 0 && n_long <= INT32_MAX && row0 >= 0 && d > 0, "spmm_update_long: bad shape");
    REQUIRE(t.mirror_complete(), "spmm_update_long: incomplete mirror descriptor");
    REQUIRE(t.wide_enough(), "spmm_update_long: leading dimension < d");
    if (n_long == 0) return CLANE_OK;
    REQUIRE(rowptr && colidx && P && long_rows && t.present() && delta_partials, "spmm_update_long: null pointer");
    REQUIRE(!t.aliased(), "spmm_update_long: Z_new must not alias Z_old");
    const Layout L = t.layout(d);
    REQUIRE(waves_per_row == 4 || waves_per_row == 16, "spmm_update_long: waves_per_row must be 4 or 16");
    const Mirror<T> mir = t.mir();
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        constexpr int U = VEC > 1 ? CLANE_LONG_U : 4;
        if (waves_per_row == 4)
            spmm_long_kernel<T, PT, VEC, LPR, U, 4><<<int(n_long), 4 * kWave, 0, (hipStream_t)stream>>>(
                rowptr, colidx, P, long_rows, row0, t.Z_old, t.ldz, t.X, t.ldx, t.gamma, t.Z_new, t.ldo, d, mir,
                delta_partials);
        else
            spmm_long_kernel<T, PT, VEC, LPR, U, kLongWaves>
                <<<int(n_long), kLongWaves * kWave, 0, (hipStream_t)stream>>>(
                    rowptr, colidx, P, long_rows, row0, t.Z_old, t.ldz, t.X, t.ldx, t.gamma, t.Z_new, t.ldo, d, mir,
                    delta_partials);
    });
    return check_launch("spmm_update_long");
}

template <typename T, typename PT>
int spmm_update_split(const int64_t *rowptr, const int32_t *colidx, const PT *P, const int32_t *split_rows,
                      const int64_t *seg_ptr, const int32_t *seg_row, int64_t n_split, int64_t n_segments,
                      int64_t edges_per_segment, int64_t row0, const Tables<T> &t, typename Elem<T>::acc_t *slab,
                      double *delta_partials, void *stream) {
    const int32_t d = t.d;
    REQUIRE(t.mirror_complete(), "spmm_update_split: incomplete mirror descriptor");
    REQUIRE(n_split >= 0 && n_split <= INT32_MAX && n_segments >= n_split && n_segments <= INT32_MAX && row0 >= 0 &&
                d > 0 && edges_per_segment >= kWave && edges_per_segment % kWave == 0,
            "spmm_update_split: bad shape (edges_per_segment must be a positive multiple of 64)");
    REQUIRE(t.wide_enough(), "spmm_update_split: leading dimension < d");
    if (n_split == 0) return CLANE_OK;
    REQUIRE(rowptr && colidx && P && split_rows && seg_ptr && seg_row && t.present() && slab && delta_partials,
            "spmm_update_split: null pointer");
    REQUIRE(!t.aliased(), "spmm_update_split: Z_new must not alias Z_old");
    REQUIRE(aligned16(slab), "spmm_update_split: slab must be 16-byte aligned");
    const Layout L = t.layout(d);
    const int64_t ld_slab = ceil_div(d, 8) * 8;
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        constexpr int U = VEC > 1 ? CLANE_LONG_U : 4;
        spmm_split_segment_kernel<T, PT, VEC, LPR, U, kLongWaves>
            <<<unsigned(n_segments), kLongWaves * kWave, 0, (hipStream_t)stream>>>(
                rowptr, colidx, P, split_rows, seg_ptr, seg_row, edges_per_segment, t.Z_old, t.ldz, d, slab, ld_slab);
        // a row's segments sit in the slab like a class row's slots: the same fixed-order combine + epilogue
        spmm_class_combine_kernel<T, VEC, LPR>
            <<<unsigned(ceil_div(n_split, kWave / LPR)), kCombineWaves * kWave, 0, (hipStream_t)stream>>>(
                split_rows, seg_ptr, n_split, row0, slab, ld_slab, t.Z_old, t.ldz, t.X, t.ldx, t.gamma, t.Z_new, t.ldo, d,
                t.mir(), false, delta_partials);
    });
    return check_launch("spmm_update_split");
}

// The class pass over column tiles: chunk sums into the slab (tile t's at slab + t * n_slots * ld_slab, all tiles' at
// the same time), then the fixed-order combine + epilogue.  The per-tile call has no use for n_slots and passes 0.
// UNIFORM: see spmm_update_impl; `item_row` (every item's row, relative to the call's first row) is then required.
template <typename T, typename PT, bool FUSED, bool UNIFORM = false>
int spmm_update_class_impl(const char *what, const int32_t *colidx, const PT *P, const int64_t *item_e0,
                           const int32_t *item_len, const int32_t *item_slot, int64_t n_blocks, int32_t items_per_block,
                           const int32_t *class_rows, const int64_t *slot_ptr, int64_t n_rows, int64_t n_slots,
                           int64_t row0, const Tables<T> &t, Tiles tiles, int32_t flags,
                           typename Elem<T>::acc_t *slab, double *delta_partials, void *stream,
                           const int32_t *item_row = nullptr) {
    const int32_t d = t.d;
    constexpr int kPad = FUSED ? 8 : 1;      // fused: block 8 j + b of every tile on XCD class b, so the count is rounded up
    REQUIRE(t.mirror_complete(), "%s: incomplete mirror descriptor", what);
    REQUIRE(n_blocks >= 0 && n_blocks <= INT32_MAX - (FUSED ? 8 : 0) && n_rows >= 0 && n_rows <= INT32_MAX &&
                n_slots >= 0 && row0 >= 0 && d > 0, "%s: bad shape", what);
    if constexpr (FUSED) REQUIRE_TILES(T, d, tiles, what, true, "");
    REQUIRE(items_per_block >= kWavesPerBlock && items_per_block <= kMaxItemsPerBlock,
            "%s: items_per_block must be in [%d, %d]", what, kWavesPerBlock, kMaxItemsPerBlock);
    REQUIRE(t.wide_enough(), "%s: leading dimension < d", what);
    const int n_tiles = tile_count(d, tiles.cols);
    REQUIRE(tiles.part_stride >= (n_tiles > 1 ? n_rows : 0), "%s: the tiles' partials overlap", what);
    if (n_rows == 0) return CLANE_OK;
    REQUIRE(colidx && P && item_e0 && item_len && item_slot && class_rows && slot_ptr && t.present() && slab &&
                delta_partials, "%s: null pointer", what);
    if constexpr (UNIFORM) REQUIRE(item_row && t.mirror == nullptr, "%s: per-row weights need item_row and no mirror", what);
    REQUIRE(!t.aliased(), "%s: Z_new must not alias Z_old", what);
    REQUIRE(aligned16(slab), "%s: slab must be 16-byte aligned", what);
    const Layout L = t.layout(tiles.cols);
    if constexpr (FUSED) REQUIRE(L.vec, "%s: the tables must allow 16-byte packs", what);
    const int64_t ld_slab = ceil_div(tiles.cols, 8) * 8;
    const int64_t slab_stride = n_slots * ld_slab;         // clane_spmm_class_slab_len(n_slots, tile_cols) per tile
    const int chunk_blocks = int(ceil_div(n_blocks, kPad) * kPad);
    const bool beyond = (flags & CLANE_SPMM_TABLE_BEYOND_CACHE) != 0;
    REQUIRE(int64_t(n_tiles) * chunk_blocks <= INT32_MAX, "%s: grid too large", what);
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        constexpr int U = VEC > 1 ? CLANE_LONG_U : 4;
        // CLANE_SPMM_TABLE_BEYOND_CACHE: fewer row loads in flight, more waves -- where it was measured to pay (see
        // spmm_update_impl): two fp32 rows per instruction (6: config 3 in tiles), four bf16 rows (4: config 4's class
        // pass 2.48 -> 2.36 ms, 98 -> 74 registers)
        constexpr int kDeepU = (LPR == 32 && VEC == 4 && sizeof(T) == 4) ? CLANE_CLASS_U32
                               : (LPR == 16 && VEC == 8 && sizeof(T) == 2) ? CLANE_CLASS_U16B : 0;
        const unsigned chunk_grid = unsigned(n_tiles) * unsigned(chunk_blocks);
        const int combine_blocks = int(ceil_div(n_rows, kWave / LPR));
        const unsigned combine_grid = unsigned(n_tiles) * unsigned(combine_blocks);
        auto chunks = [&]<int CU>() {
            if constexpr (!FUSED)
                spmm_class_chunk_kernel<T, PT, VEC, LPR, CU, UNIFORM><<<chunk_grid, kBlock, 0, (hipStream_t)stream>>>(
                    colidx, P, item_e0, item_len, item_slot, items_per_block, t.Z_old, t.ldz, d, slab, ld_slab, item_row);
            else if constexpr (VEC > 1)
                spmm_class_chunk_tiles_kernel<T, PT, VEC, LPR, CU, UNIFORM><<<chunk_grid, kBlock, 0, (hipStream_t)stream>>>(
                    colidx, P, item_e0, item_len, item_slot, int(n_blocks), items_per_block, t.Z_old, t.ldz, d, slab,
                    ld_slab, slab_stride, TileGrid{chunk_blocks, tiles.cols, 0}, item_row);
        };
        if (n_blocks > 0 && kDeepU > 0 && beyond) chunks.template operator()<(kDeepU > 0 ? kDeepU : U)>();
        else if (n_blocks > 0) chunks.template operator()<U>();
        if constexpr (!FUSED)
            spmm_class_combine_kernel<T, VEC, LPR><<<combine_grid, kCombineWaves * kWave, 0, (hipStream_t)stream>>>(
                class_rows, slot_ptr, n_rows, row0, slab, ld_slab, t.Z_old, t.ldz, t.X, t.ldx, t.gamma, t.Z_new, t.ldo, d,
                t.mir(), beyond, delta_partials);
        else if constexpr (VEC > 1)
            spmm_class_combine_tiles_kernel<T, VEC, LPR><<<combine_grid, kCombineWaves * kWave, 0, (hipStream_t)stream>>>(
                class_rows, slot_ptr, n_rows, row0, slab, ld_slab, slab_stride, t.Z_old, t.ldz, t.X, t.ldx, t.gamma,
                t.Z_new, t.ldo, d, beyond, TileGrid{combine_blocks, tiles.cols, tiles.part_stride}, delta_partials);
    });
    return check_launch(what);
}

// LDS of spmm_owned_kernel beyond its sums (the step counters), rounded up generously
constexpr int64_t kOwnedLdsReserve = 1024;
constexpr int64_t kLdsPerCU = 160 * 1024;
constexpr int64_t kLdsDefaultLimit = 64 * 1024;

// The owned class pass over the column tiles of a table t.d wide.  Its kernel has one entry for both forms, so there is
// no FUSED here; everything but the tiles themselves is reported as spmm_update_owned, whichever entry point was called.
// UNIFORM: see spmm_update_impl; `seg_row` (every segment's row, relative to the call's first row) is then required.
template <typename T, typename PT, bool UNIFORM = false>
int spmm_update_owned_impl(const char *what, const int32_t *colidx, const PT *P, const clane_owned_plan_t *plan,
                           int32_t block_threads, int64_t row0, const Tables<T> &t, Tiles tiles, bool fused, int32_t flags,
                           double *delta_partials, void *stream, const int32_t *seg_row = nullptr) {
    using A = typename Elem<T>::acc_t;
    const int32_t d = tiles.cols;          // what the instance and the LDS sums are sized by: one full tile
    if (fused) REQUIRE_TILES(T, t.d, tiles, what, tiles.part_stride >= 0, ", the partials' stride >= 0");
    REQUIRE(plan, "spmm_update_owned: null plan");
    REQUIRE(plan->n_groups >= 0 && row0 >= 0 && d > 0, "spmm_update_owned: bad shape");
    REQUIRE(plan->n_steps >= 1 && plan->n_steps <= kOwnedMaxSteps, "spmm_update_owned: n_steps must be in [1, %d]",
            kOwnedMaxSteps);
    REQUIRE(plan->chunk >= kWave && plan->chunk % kWave == 0, "spmm_update_owned: chunk must be a positive multiple of 64");
    REQUIRE(block_threads >= kWave && block_threads <= kOwnedMaxBlock && block_threads % kWave == 0,
            "spmm_update_owned: block_threads must be a multiple of 64 in [64, %d]", kOwnedMaxBlock);
    REQUIRE(t.wide_enough(), "spmm_update_owned: leading dimension < d");
    REQUIRE(plan->max_batch_vrows >= 0, "spmm_update_owned: negative max_batch_vrows");
    if (plan->n_groups == 0) return CLANE_OK;
    REQUIRE(colidx && P && plan->grp_bat_ptr && plan->bat_vrow_ptr && plan->bat_row_ptr && plan->bat_seg_ptr &&
                plan->seg_e0 && plan->seg_len && plan->seg_vrow && plan->row_id && plan->row_part && plan->row_vptr &&
                t.present() && delta_partials,
            "spmm_update_owned: null pointer");
    if constexpr (UNIFORM) REQUIRE(seg_row, "spmm_update_owned: per-row weights need seg_row");
    REQUIRE(!t.aliased(), "spmm_update_owned: Z_new must not alias Z_old");
    const Layout L = t.layout(d);
    REQUIRE(L.vec && (L.lpr == 32 || L.lpr == 64) && d <= L.lpr * Elem<T>::kVec,
            "spmm_update_owned: no instance for d=%d with these operands (16-byte packs, 17..64 packs per row)", d);
    const int64_t lds = int64_t(plan->max_batch_vrows) * L.lpr * Elem<T>::kVec * int64_t(sizeof(A));
    REQUIRE(lds + kOwnedLdsReserve <= kLdsPerCU, "spmm_update_owned: %lld virtual rows per batch need %lld bytes of LDS",
            (long long)plan->max_batch_vrows, (long long)lds);
    const OwnedPlan op{plan->grp_bat_ptr, plan->bat_vrow_ptr, plan->bat_row_ptr, plan->bat_seg_ptr, plan->seg_e0,
                       plan->seg_len, plan->seg_vrow, plan->row_id, plan->row_part, plan->row_vptr, plan->n_steps,
                       plan->chunk};
    const bool beyond = (flags & CLANE_SPMM_TABLE_BEYOND_CACHE) != 0;
    int rc = CLANE_OK;
    auto launch = [&]<int VEC, int LPR, int U>() {
        auto *kernel = spmm_owned_kernel<T, PT, VEC, LPR, U, UNIFORM>;
        if (lds > kLdsDefaultLimit) {      // above the default per-workgroup limit: ask for it, once per size
            static int64_t granted = 0;
            if (lds > granted) {
                const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
                if (e != hipSuccess) {
                    rc = fail(CLANE_ERR_LAUNCH, "spmm_update_owned: %lld bytes of LDS: %s", (long long)lds,
                              hipGetErrorString(e));
                    return;
                }
                granted = lds;
            }
        }
        kernel<<<unsigned(plan->n_groups), unsigned(block_threads), size_t(lds), (hipStream_t)stream>>>(
            colidx, P, op, row0, t.Z_old, t.ldz, t.X, t.ldx, t.gamma, t.Z_new, t.ldo, t.d, tiles.cols, tiles.part_stride,
            (flags & CLANE_OWNED_EPILOGUE_AHEAD) != 0, beyond, delta_partials, seg_row);
    };
    constexpr int KV = Elem<T>::kVec;
    // Row loads in flight per wave.  Asked for through CLANE_OWNED_LOADS(n) (the instances: 6, 8, 12 at two rows per
    // instruction; 8, 12 at one), else the chunk kernel's: CLANE_CLASS_U32 at two rows per instruction beyond the caches.
    const int asked = (flags >> 8) & 0xff;
    REQUIRE(asked == 0 || asked == 8 || asked == 12 || (L.lpr == 32 && asked == 6),
            "spmm_update_owned: no instance with %d row loads in flight", asked);
    const int loads = asked ? asked : (L.lpr == 32 && beyond) ? CLANE_CLASS_U32 : CLANE_LONG_U;
    if (L.lpr == 32) {
        if (loads == 6) launch.template operator()<KV, 32, 6>();
        else if (loads == 12) launch.template operator()<KV, 32, 12>();
        else launch.template operator()<KV, 32, 8>();
    } else {
        if (loads == 12) launch.template operator()<KV, 64, 12>();
        else launch.template operator()<KV, 64, 8>();
    }
    if (rc != CLANE_OK) return rc;
    return check_launch(what);
}

template <typename T>
int l1_distance(const T *A, int64_t lda, const T *B, int64_t ldb, int64_t nrows, int32_t d,
                typename Elem<T>::acc_t *sq_a, double *ws, double *out, void *stream) {
    REQUIRE(nrows >= 0 && d > 0 && lda >= d && ldb >= d, "l1_distance: bad shape");
    REQUIRE(ws && out, "l1_distance: null workspace/output");
    REQUIRE(nrows == 0 || (A && B), "l1_distance: null pointer");
    const Layout L = pick_layout<T>(d, {A, B}, {lda, ldb});
    if (sq_a != nullptr) {      // sq_a must be bit for bit row_sqnorm's, whose lane layout follows from A alone
        const Layout LA = pick_layout<T>(d, {A}, {lda});
        REQUIRE(LA.vec == L.vec && LA.lpr == L.lpr,
                "l1_distance: sq_a needs B as aligned as A (the lane layout of row_sqnorm on A)");
    }
    int grid = 1;
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        grid = grid_for_waves(ceil_div(nrows > 0 ? nrows : 1, (kWave / LPR) * stream_rows(LPR)));
        if (grid > kReduceGrid) grid = kReduceGrid;
        l1_distance_kernel<T, VEC, LPR><<<grid, kBlock, 0, (hipStream_t)stream>>>(A, lda, B, ldb, nrows, d, sq_a, ws);
    });
    reduce_fixed_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(ws, grid, grid, 1, out);
    return check_launch("l1_distance");
}

template <typename T>
int gather_rows(const T *src, int64_t lds, const int32_t *idx, int64_t n, int32_t d, T *dst, int64_t ldd, void *stream) {
    REQUIRE(n >= 0 && d > 0 && lds >= d && ldd >= d, "gather_rows: bad shape");
    if (n == 0) return CLANE_OK;
    REQUIRE(src && idx && dst, "gather_rows: null pointer");
    const Layout L = pick_layout<T>(d, {src, dst}, {lds, ldd});
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        const int grid = grid_for_waves(ceil_div(n, kWave / LPR));
        gather_rows_kernel<T, VEC, LPR><<<grid, kBlock, 0, (hipStream_t)stream>>>(src, lds, idx, n, d, dst, ldd);
    });
    return check_launch("gather_rows");
}

template <typename T>
int pair_cosine(const T *A, int64_t lda, const T *B, int64_t ldb, int64_t nrows, int32_t d,
                typename Elem<T>::acc_t *out, double *ws, void *stream) {
    REQUIRE(nrows >= 0 && d > 0 && lda >= d && ldb >= d, "pair_cosine: bad shape");
    if (nrows == 0) return CLANE_OK;
    REQUIRE(A && B && out && ws, "pair_cosine: null pointer");
    const Layout L = pick_layout<T>(d, {A, B}, {lda, ldb});
    int grid = 1;
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        grid = grid_for_waves(ceil_div(nrows, kWave / LPR));
        if (grid > kReduceGrid) grid = kReduceGrid;
        pair_dot_kernel<T, VEC, LPR><<<grid, kBlock, 0, (hipStream_t)stream>>>(A, lda, B, ldb, nrows, d, out, ws);
    });
    double *sums2 = ws + 2 * kReduceGrid;
    reduce_fixed_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(ws, grid, grid, 2, sums2);
    int sgrid = int(ceil_div(nrows, kBlock));
    if (sgrid > kMaxGrid) sgrid = kMaxGrid;
    pair_scale_kernel<typename Elem<T>::acc_t><<<sgrid, kBlock, 0, (hipStream_t)stream>>>(out, nrows, sums2);
    return check_launch("pair_cosine");
}

// ---- training step of the bilinear similarity (pair_train.h) -----------------------------------------------------
template <typename T, typename A>
int pair_project(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *src, const int32_t *dst,
                 int64_t B, const A *W, A *PA, A *PB, void *stream) {
    REQUIRE(table_rows >= 0 && B >= 0 && d > 0 && d <= 32768 && ldz >= d, "pair_project: bad shape rows=%lld B=%lld d=%d ldz=%lld",
            (long long)table_rows, (long long)B, d, (long long)ldz);
    if (B == 0) return CLANE_OK;
    REQUIRE(Z && src && dst && W && PA && PB, "pair_project: null pointer");
    const int n_tiles = int(ceil_div(int64_t(d), int64_t(kProjBN)));
    const int64_t blocks = ceil_div(B, int64_t(kProjBM)) * n_tiles;
    REQUIRE(blocks <= INT32_MAX, "pair_project: %lld pairs is too many for one launch", (long long)B);
    pair_project_kernel<T, A><<<dim3(unsigned(blocks), 2), kBlock, 0, (hipStream_t)stream>>>(
        Z, table_rows, d, ldz, src, dst, B, W, PA, PB, n_tiles);
    return check_launch("pair_project");
}

template <typename A>
int pair_loss(const A *PA, const A *PB, int64_t B, int32_t d, const uint8_t *linked, const A *u, A *g, uint8_t *mask,
              double *ws, double *stats, void *stream) {
    REQUIRE(B >= 0 && d > 0, "pair_loss: bad shape B=%lld d=%d", (long long)B, d);
    REQUIRE(ws && stats, "pair_loss: null workspace/output");
    REQUIRE(B == 0 || (PA && PB && linked && u && g && mask), "pair_loss: null pointer");
    int grid = int(ceil_div(B > 0 ? B : 1, kBlock / kPairLanes));
    if (grid > kReduceGrid) grid = kReduceGrid;
    pair_loss_kernel<A><<<grid, kBlock, 0, (hipStream_t)stream>>>(PA, PB, B, d, linked, u, g, mask, ws);
    reduce_fixed_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(ws, grid, grid, 2, stats);
    return check_launch("pair_loss");
}

inline int64_t pair_grad_chunks(int64_t B) { return ceil_div(B > 0 ? B : 1, int64_t(kGradChunk)); }

template <typename T, typename A>
int pair_grad(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *src, const int32_t *dst, int64_t B,
              const A *PA, const A *PB, const A *g, const double *stats, A *ws, A *dW, void *stream) {
    REQUIRE(table_rows >= 0 && B >= 0 && d > 0 && d <= 32768 && ldz >= d, "pair_grad: bad shape rows=%lld B=%lld d=%d ldz=%lld",
            (long long)table_rows, (long long)B, d, (long long)ldz);
    REQUIRE(stats && ws && dW, "pair_grad: null stats/workspace/output");
    REQUIRE(B == 0 || (Z && src && dst && PA && PB && g), "pair_grad: null pointer");
    const int64_t n_chunks = B > 0 ? pair_grad_chunks(B) : 0;
    REQUIRE(n_chunks <= 65535, "pair_grad: %lld pairs is too many for one launch", (long long)B);
    const int n_tiles = int(ceil_div(int64_t(d), int64_t(kProjBN)));
    const int64_t n = 2 * int64_t(d) * d;
    if (n_chunks > 0)
        pair_grad_kernel<T, A><<<dim3(unsigned(n_tiles * n_tiles), 2, unsigned(n_chunks)), kBlock, 0,
                                 (hipStream_t)stream>>>(Z, table_rows, d, ldz, src, dst, B, PA, PB, g, ws, n_tiles);
    pair_grad_reduce_kernel<A><<<unsigned(ceil_div(n, kBlock)), kBlock, 0, (hipStream_t)stream>>>(ws, n_chunks, n, stats,
                                                                                               dW);
    return check_launch("pair_grad");
}

template <typename A>
int adam_step(A *W, A *m, A *v, const A *dW, int64_t n, double lr, const double *stats, double *state, void *stream) {
    REQUIRE(n >= 0 && n <= int64_t(INT32_MAX) * kBlock, "adam_step: bad length %lld", (long long)n);
    REQUIRE(stats && state, "adam_step: null stats/state");
    REQUIRE(n == 0 || (W && m && v && dW), "adam_step: null pointer");
    if (n > 0)
        adam_step_kernel<A><<<unsigned(ceil_div(n, kBlock)), kBlock, 0, (hipStream_t)stream>>>(W, m, v, dW, n, lr, stats,
                                                                                            state);
    adam_finish_kernel<<<1, kWave, 0, (hipStream_t)stream>>>(stats, state);
    return check_launch("adam_step");
}

// ---- link prediction (link_rank.h) ---------------------------------------------------------------------------------
inline bool score_mode_ok(int32_t mode) {
    return mode == CLANE_SCORE_REFERENCE || mode == CLANE_SCORE_PER_EDGE || mode == CLANE_SCORE_RAW_DOT;
}

template <typename T, typename A>
int rank_scores(const T *S, int64_t lds, const T *N, int64_t ldn, int64_t table_rows, int32_t d, const int32_t *q_rows,
                int64_t Q, int32_t mode, const double *sums2, const A *sq, const int32_t *label,
                const int64_t *excl_rowptr, const int32_t *excl_colidx, int32_t exclude_self, int32_t k,
                int32_t n_slabs, A *cand_score, int32_t *cand_id, void *stream) {
    constexpr int MI = sizeof(A) == 8 ? 2 : 4;
    static_assert(kRankMaxK == CLANE_RANK_MAX_K, "header and kernel disagree");
    REQUIRE(d >= 1 && lds >= d && ldn >= d && Q >= 0 && table_rows >= 0 && table_rows <= INT32_MAX,
            "rank_scores: bad shape rows=%lld Q=%lld d=%d lds=%lld ldn=%lld", (long long)table_rows, (long long)Q, d,
            (long long)lds, (long long)ldn);
    REQUIRE(k >= 1 && k <= CLANE_RANK_MAX_K, "rank_scores: k must be in [1, %d], got %d", CLANE_RANK_MAX_K, k);
    REQUIRE(n_slabs >= 1, "rank_scores: n_slabs must be at least 1, got %d", n_slabs);
    REQUIRE(score_mode_ok(mode), "rank_scores: unknown mode %d", mode);
    REQUIRE(mode != CLANE_SCORE_REFERENCE || sums2, "rank_scores: mode REFERENCE needs sums2");
    REQUIRE(mode != CLANE_SCORE_PER_EDGE || sq, "rank_scores: mode PER_EDGE needs sq");
    REQUIRE((excl_rowptr == nullptr) == (excl_colidx == nullptr),
            "rank_scores: excl_rowptr and excl_colidx come together or not at all");
    if (Q == 0) return CLANE_OK;
    REQUIRE(S && N && q_rows && cand_score && cand_id, "rank_scores: null pointer");
    const int64_t q_tiles = ceil_div(Q, int64_t(32 * MI));
    const int64_t blocks = q_tiles * n_slabs;
    REQUIRE(blocks <= INT32_MAX, "rank_scores: %lld queries x %d slabs is too many for one launch", (long long)Q, n_slabs);
    const int64_t tiles_total = ceil_div(table_rows, int64_t(kRankBN));
    const int64_t tiles_per_slab = ceil_div(tiles_total > 0 ? tiles_total : 1, int64_t(n_slabs));
    rank_scores_kernel<T, A, MI><<<unsigned(blocks), kBlock, rank_list_bytes<A>(32 * MI, k), (hipStream_t)stream>>>(
        S, lds, N, ldn, table_rows, d, q_rows, Q, mode, sums2, sq, label, excl_rowptr, excl_colidx, exclude_self, k,
        n_slabs, q_tiles, tiles_per_slab, cand_score, cand_id);
    return check_launch("rank_scores");
}

template <typename T, typename A>
int rank_count(const T *S, int64_t lds, const T *N, int64_t ldn, int64_t table_rows, int32_t d, const int32_t *q_rows,
               const int32_t *t_rows, int64_t B, int32_t mode, const double *sums2, const A *sq, const int32_t *label,
               const int64_t *excl_rowptr, const int32_t *excl_colidx, int32_t exclude_self, int32_t n_slabs,
               A *target_score, int32_t *counts, void *stream) {
    constexpr int MI = sizeof(A) == 8 ? 2 : 4;
    REQUIRE(d >= 1 && lds >= d && ldn >= d && B >= 0 && table_rows >= 0 && table_rows <= INT32_MAX,
            "rank_count: bad shape rows=%lld B=%lld d=%d lds=%lld ldn=%lld", (long long)table_rows, (long long)B, d,
            (long long)lds, (long long)ldn);
    REQUIRE(n_slabs >= 1, "rank_count: n_slabs must be at least 1, got %d", n_slabs);
    REQUIRE(score_mode_ok(mode), "rank_count: unknown mode %d", mode);
    REQUIRE(mode != CLANE_SCORE_REFERENCE || sums2, "rank_count: mode REFERENCE needs sums2");
    REQUIRE(mode != CLANE_SCORE_PER_EDGE || sq, "rank_count: mode PER_EDGE needs sq");
    REQUIRE((excl_rowptr == nullptr) == (excl_colidx == nullptr),
            "rank_count: excl_rowptr and excl_colidx come together or not at all");
    if (B == 0) return CLANE_OK;
    REQUIRE(S && N && q_rows && t_rows && target_score && counts, "rank_count: null pointer");
    const int64_t q_tiles = ceil_div(B, int64_t(32 * MI));
    const int64_t blocks = q_tiles * n_slabs;
    REQUIRE(blocks <= INT32_MAX, "rank_count: %lld pairs x %d slabs is too many for one launch", (long long)B, n_slabs);
    const int64_t tiles_total = ceil_div(table_rows, int64_t(kRankBN));
    const int64_t tiles_per_slab = ceil_div(tiles_total > 0 ? tiles_total : 1, int64_t(n_slabs));
    rank_count_kernel<T, A, MI><<<unsigned(blocks), kBlock, 0, (hipStream_t)stream>>>(
        S, lds, N, ldn, table_rows, d, q_rows, t_rows, B, mode, sums2, sq, label, excl_rowptr, excl_colidx, exclude_self,
        n_slabs, q_tiles, tiles_per_slab, target_score, counts);
    return check_launch("rank_count");
}

template <typename A>
int rank_merge(const A *cand_score, const int32_t *cand_id, int64_t Q, int32_t n_slabs, int32_t k, A *out_score,
               int32_t *out_id, void *stream) {
    REQUIRE(Q >= 0 && Q <= int64_t(INT32_MAX) * kWavesPerBlock, "rank_merge: bad shape Q=%lld", (long long)Q);
    REQUIRE(k >= 1 && k <= CLANE_RANK_MAX_K, "rank_merge: k must be in [1, %d], got %d", CLANE_RANK_MAX_K, k);
    REQUIRE(n_slabs >= 1, "rank_merge: n_slabs must be at least 1, got %d", n_slabs);
    if (Q == 0) return CLANE_OK;
    REQUIRE(cand_score && cand_id && out_score && out_id, "rank_merge: null pointer");
    rank_merge_kernel<A><<<unsigned(ceil_div(Q, kWavesPerBlock)), kBlock, 0, (hipStream_t)stream>>>(
        cand_score, cand_id, Q, n_slabs, k, out_score, out_id);
    return check_launch("rank_merge");
}

template <typename T>
int pair_score(const T *S, int64_t lds, const T *N, int64_t ldn, int64_t table_rows, int32_t d, const int32_t *src,
               const int32_t *dst, int64_t B, int32_t mode, const double *sums2, const typename Elem<T>::acc_t *sq,
               typename Elem<T>::acc_t *out, void *stream) {
    REQUIRE(d >= 1 && lds >= d && ldn >= d && B >= 0 && table_rows >= 0,
            "pair_score: bad shape rows=%lld B=%lld d=%d lds=%lld ldn=%lld", (long long)table_rows, (long long)B, d,
            (long long)lds, (long long)ldn);
    REQUIRE(score_mode_ok(mode), "pair_score: unknown mode %d", mode);
    REQUIRE(mode != CLANE_SCORE_REFERENCE || sums2, "pair_score: mode REFERENCE needs sums2");
    REQUIRE(mode != CLANE_SCORE_PER_EDGE || sq, "pair_score: mode PER_EDGE needs sq");
    if (B == 0) return CLANE_OK;
    REQUIRE(S && N && src && dst && out, "pair_score: null pointer");
    const Layout L = pick_layout<T>(d, {S, N}, {lds, ldn});
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        pair_score_kernel<T, VEC, LPR><<<grid_for_waves(ceil_div(B, kWave / LPR)), kBlock, 0, (hipStream_t)stream>>>(
            S, lds, N, ldn, table_rows, d, src, dst, B, mode, sums2, sq, out);
    });
    return check_launch("pair_score");
}

// ---- new vertices against the finished table (new_rows.h) ------------------------------------------------------------
template <typename T, typename GT>
int embed_rows(const int64_t *rowptr, const int32_t *colidx, int64_t m, const T *X_new, int64_t ldx, const T *Z,
               int64_t table_rows, int64_t ldz, int32_t d, int32_t mode, const double *sums2,
               const typename Elem<T>::acc_t *sq, const typename Elem<T>::acc_t *S, int64_t lds, GT gamma,
               int32_t tolerence, int32_t max_rounds, int32_t flags, T *Z_out, int64_t ldo, int32_t *rounds,
               typename Elem<T>::acc_t *delta, typename Elem<T>::acc_t *P_out, void *stream) {
    using A = typename Elem<T>::acc_t;
    REQUIRE(m >= 0, "embed_rows: m = %lld is negative", (long long)m);
    REQUIRE(table_rows >= 0, "embed_rows: table_rows = %lld is negative", (long long)table_rows);
    REQUIRE(d >= 1, "embed_rows: d = %d must be at least 1", d);
    REQUIRE(ldx >= d && ldz >= d && ldo >= d, "embed_rows: ldx = %lld, ldz = %lld and ldo = %lld must be at least d = %d",
            (long long)ldx, (long long)ldz, (long long)ldo, d);
    REQUIRE(score_mode_ok(mode), "embed_rows: unknown mode %d", mode);
    REQUIRE(S == nullptr || mode == CLANE_SCORE_RAW_DOT, "embed_rows: S (the projected table) goes with mode RAW_DOT only");
    REQUIRE(S != nullptr || mode != CLANE_SCORE_RAW_DOT, "embed_rows: mode RAW_DOT needs S (the projected table)");
    REQUIRE(S == nullptr || lds >= d, "embed_rows: lds = %lld must be at least d = %d", (long long)lds, d);
    REQUIRE(mode != CLANE_SCORE_REFERENCE || sums2, "embed_rows: mode REFERENCE needs sums2");
    REQUIRE(mode != CLANE_SCORE_PER_EDGE || sq, "embed_rows: mode PER_EDGE needs sq");
    REQUIRE(tolerence >= 1, "embed_rows: tolerence = %d must be at least 1", tolerence);
    REQUIRE(max_rounds >= 1, "embed_rows: max_rounds = %d must be at least 1", max_rounds);
    REQUIRE(flags == 0, "embed_rows: unknown flags %d", flags);
    REQUIRE(Z_out && rounds && delta, "embed_rows: null output (Z_out, rounds, delta)");
    if (m == 0) return CLANE_OK;
    REQUIRE(rowptr && X_new, "embed_rows: null rowptr / X_new");
    REQUIRE(table_rows == 0 || (colidx && Z), "embed_rows: null colidx / Z");
    constexpr int KV = Elem<T>::kVec;
    Layout L = pick_layout<T>(d, {X_new, Z, Z_out}, {ldx, ldz, ldo});
    if (S != nullptr && L.vec && ((reinterpret_cast<uintptr_t>(S) % (sizeof(A) * KV)) != 0 || lds % KV != 0)) {
        L.vec = false;                       // score rows are read as packs of KV accumulate-type elements
        L.lpr = d <= 4 ? 4 : d <= 16 ? 16 : 64;
    }
    const int width = L.lpr * (L.vec ? KV : 1);
    const bool wide = d > width;
    const int dpad = int(ceil_div(d, width)) * width;
    REQUIRE(!wide || int64_t(dpad) * 2 * int64_t(sizeof(A)) <= kEmbedWideLdsPerWave,
            "embed_rows: d = %d is more than this layout keeps per row (%d)", d,
            int(kEmbedWideLdsPerWave / (2 * sizeof(A)) / width * width));
    const int rpb = rows_per_block(m);
    const unsigned grid = unsigned(row_grid(m));
    const A g = A(gamma);
    auto launch = [&]<int VEC, int LPR, bool PAIR, bool WIDE>() {
        constexpr int U = VEC > 1 ? 8 : 4;
        const size_t lds_bytes = WIDE ? size_t(kWavesPerBlock) * 2 * dpad * sizeof(A) : 0;
        embed_rows_kernel<T, VEC, LPR, U, PAIR, WIDE><<<grid, kBlock, lds_bytes, (hipStream_t)stream>>>(
            rowptr, colidx, m, X_new, ldx, Z, ldz, d, mode, sums2, sq, S, lds, g, tolerence, max_rounds, Z_out, ldo,
            rounds, delta, P_out, rpb, dpad);
    };
    dispatch_layout<T>(L, [&]<int VEC, int LPR>() {
        if constexpr (LPR == kWave) {
            if (wide) {
                if (S) launch.template operator()<VEC, LPR, true, true>();
                else launch.template operator()<VEC, LPR, false, true>();
                return;
            }
        }
        if (S) launch.template operator()<VEC, LPR, true, false>();
        else launch.template operator()<VEC, LPR, false, false>();
    });
    return check_launch("embed_rows");
}

// ---- node classification probe (label_probe.h) ----------------------------------------------------------------------
inline int64_t probe_row_tiles(int64_t n) { return ceil_div(n > 0 ? n : 1, int64_t(kProjBM)); }
inline int64_t probe_grad_chunks(int64_t n) { return ceil_div(n > 0 ? n : 1, int64_t(kGradChunk)); }

template <typename T, typename A>
int probe_forward(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, const int32_t *y, int64_t n,
                  const uint8_t *split, int64_t ld_split, const A *W, const A *bias, int32_t F, int32_t C, int32_t flags,
                  A *G, double *loss_ws, double *loss, int32_t *pred, int64_t ld_pred, void *stream) {
    static_assert(kProbeWriteG == CLANE_PROBE_WRITE_G && kProbeWritePred == CLANE_PROBE_WRITE_PRED &&
                      kProbeMaxClasses == CLANE_PROBE_MAX_CLASSES,
                  "header and kernel disagree");
    REQUIRE(table_rows >= 0 && n >= 0 && d > 0 && d <= 32768 && ldz >= d,
            "probe_forward: bad shape rows=%lld n=%lld d=%d ldz=%lld", (long long)table_rows, (long long)n, d,
            (long long)ldz);
    REQUIRE(C >= 2 && C <= kProbeMaxClasses, "probe_forward: C must be in [2, %d], got %d", kProbeMaxClasses, C);
    const int cp_log = probe_cp_log(C);
    REQUIRE(F >= 1 && F <= (INT32_MAX >> 7), "probe_forward: bad number of fits %d", F);
    REQUIRE(ld_split >= F, "probe_forward: ld_split %lld < F = %d", (long long)ld_split, F);
    REQUIRE((flags & ~(CLANE_PROBE_WRITE_G | CLANE_PROBE_WRITE_PRED)) == 0, "probe_forward: unknown flags %d", flags);
    REQUIRE(!(flags & CLANE_PROBE_WRITE_PRED) || ld_pred >= F, "probe_forward: ld_pred %lld < F = %d", (long long)ld_pred, F);
    REQUIRE(loss_ws && loss, "probe_forward: null loss workspace/output");
    REQUIRE(n == 0 || (Z && rows && y && split && W && bias), "probe_forward: null pointer");
    REQUIRE(n == 0 || !(flags & CLANE_PROBE_WRITE_G) || G, "probe_forward: CLANE_PROBE_WRITE_G needs G");
    REQUIRE(n == 0 || !(flags & CLANE_PROBE_WRITE_PRED) || pred, "probe_forward: CLANE_PROBE_WRITE_PRED needs pred");
    const int K = F << cp_log;
    const int n_tiles = int(ceil_div(int64_t(K), int64_t(kProjBN)));
    const int64_t row_tiles = n > 0 ? probe_row_tiles(n) : 0;
    const int64_t blocks = row_tiles * n_tiles;
    REQUIRE(blocks <= INT32_MAX, "probe_forward: %lld rows x %d fits is too many for one launch", (long long)n, F);
    if (blocks > 0)
        probe_forward_kernel<T, A><<<unsigned(blocks), kBlock, 0, (hipStream_t)stream>>>(
            Z, table_rows, d, ldz, rows, y, n, split, ld_split, W, bias, F, C, cp_log, flags, G, loss_ws, pred, ld_pred,
            n_tiles);
    probe_loss_reduce_kernel<<<unsigned(F), kBlock, 0, (hipStream_t)stream>>>(loss_ws, row_tiles, F, loss);
    return check_launch("probe_forward");
}

// One-vs-rest probe (multilabel_probe.h): the same launch shape, the sigmoid / top-k epilogue.
template <typename T, typename A>
int probe_forward_ovr(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, const uint64_t *ymask,
                      int64_t n, const uint8_t *split, int64_t ld_split, const A *W, const A *bias, const int8_t *col_state,
                      int32_t F, int32_t C, int32_t max_labels, int32_t flags, A *G, double *loss_ws, double *loss,
                      uint64_t *pred, int64_t ld_pred, void *stream) {
    static_assert(kOvrWriteG == CLANE_PROBE_WRITE_G && kOvrWritePred == CLANE_PROBE_WRITE_PRED &&
                      kOvrPredTopk == CLANE_PROBE_PRED_TOPK,
                  "header and kernel disagree");
    REQUIRE(table_rows >= 0 && n >= 0 && d > 0 && d <= 32768 && ldz >= d,
            "probe_forward_ovr: bad shape rows=%lld n=%lld d=%d ldz=%lld", (long long)table_rows, (long long)n, d,
            (long long)ldz);
    REQUIRE(C >= 1 && C <= kProbeMaxClasses, "probe_forward_ovr: C must be in [1, %d], got %d", kProbeMaxClasses, C);
    REQUIRE(max_labels >= 0 && max_labels <= C, "probe_forward_ovr: max_labels must be in [0, C = %d], got %d", C,
            max_labels);
    const int cp_log = probe_cp_log(C);
    REQUIRE(F >= 1 && F <= (INT32_MAX >> 7), "probe_forward_ovr: bad number of fits %d", F);
    REQUIRE(ld_split >= F, "probe_forward_ovr: ld_split %lld < F = %d", (long long)ld_split, F);
    REQUIRE((flags & ~(CLANE_PROBE_WRITE_G | CLANE_PROBE_WRITE_PRED | CLANE_PROBE_PRED_TOPK)) == 0,
            "probe_forward_ovr: unknown flags %d", flags);
    REQUIRE(!(flags & CLANE_PROBE_WRITE_PRED) || ld_pred >= F, "probe_forward_ovr: ld_pred %lld < F = %d",
            (long long)ld_pred, F);
    REQUIRE(loss_ws && loss, "probe_forward_ovr: null loss workspace/output");
    REQUIRE(n == 0 || (Z && rows && ymask && split && W && bias && col_state), "probe_forward_ovr: null pointer");
    REQUIRE(n == 0 || !(flags & CLANE_PROBE_WRITE_G) || G, "probe_forward_ovr: CLANE_PROBE_WRITE_G needs G");
    REQUIRE(n == 0 || !(flags & CLANE_PROBE_WRITE_PRED) || pred, "probe_forward_ovr: CLANE_PROBE_WRITE_PRED needs pred");
    const int K = F << cp_log;
    const int n_tiles = int(ceil_div(int64_t(K), int64_t(kProjBN)));
    const int64_t row_tiles = n > 0 ? probe_row_tiles(n) : 0;
    const int64_t blocks = row_tiles * n_tiles;
    REQUIRE(blocks <= INT32_MAX, "probe_forward_ovr: %lld rows x %d fits is too many for one launch", (long long)n, F);
    if (blocks > 0)
        probe_forward_ovr_kernel<T, A><<<unsigned(blocks), kBlock, 0, (hipStream_t)stream>>>(
            Z, table_rows, d, ldz, rows, ymask, n, split, ld_split, W, bias, col_state, F, C, cp_log, max_labels, flags, G,
            loss_ws, pred, ld_pred, n_tiles);
    probe_loss_reduce_kernel<<<unsigned(F), kBlock, 0, (hipStream_t)stream>>>(loss_ws, row_tiles, F, loss);
    return check_launch("probe_forward_ovr");
}

template <typename T, typename A>
int probe_grad(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n, const A *G,
               int32_t K, A *ws, A *dW, A *db, void *stream) {
    REQUIRE(table_rows >= 0 && n >= 0 && d > 0 && d <= 32768 && ldz >= d && K >= 1,
            "probe_grad: bad shape rows=%lld n=%lld d=%d ldz=%lld K=%d", (long long)table_rows, (long long)n, d,
            (long long)ldz, K);
    REQUIRE(ws && dW && db, "probe_grad: null workspace/output");
    REQUIRE(n == 0 || (Z && rows && G), "probe_grad: null pointer");
    const int64_t n_chunks = n > 0 ? probe_grad_chunks(n) : 0;
    REQUIRE(n_chunks <= 65535, "probe_grad: %lld rows is too many for one launch", (long long)n);
    const int64_t d_tiles = ceil_div(int64_t(d), int64_t(kProjBN)), k_tiles = ceil_div(int64_t(K), int64_t(kProjBM));
    REQUIRE(d_tiles * k_tiles <= INT32_MAX, "probe_grad: K=%d x d=%d is too many tiles for one launch", K, d);
    const int64_t len = int64_t(K) * (int64_t(d) + 1);
    if (n_chunks > 0)
        probe_grad_kernel<T, A><<<dim3(unsigned(d_tiles * k_tiles), unsigned(n_chunks)), kBlock, 0, (hipStream_t)stream>>>(
            Z, table_rows, d, ldz, rows, n, G, K, ws, int(d_tiles));
    probe_grad_reduce_kernel<A><<<unsigned(ceil_div(len, kBlock)), kBlock, 0, (hipStream_t)stream>>>(
        ws, n_chunks, len, int64_t(K) * d, dW, db);
    return check_launch("probe_grad");
}

// Applying fitted probes (label_predict.h): probe_forward's launch shape, probabilities and the top-m classes out.
template <typename T, typename A>
int probe_predict(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n, const A *W,
                  const A *bias, const int8_t *col_state, int32_t F, int32_t C, int32_t top_m, int32_t flags,
                  int32_t *top_class, A *top_prob, A *proba, void *stream) {
    static_assert(kPredictSigmoid == CLANE_PREDICT_SIGMOID && kPredictWriteProba == CLANE_PREDICT_WRITE_PROBA &&
                      kPredictMaxTop == CLANE_PREDICT_MAX_TOP,
                  "header and kernel disagree");
    REQUIRE(table_rows >= 0 && n >= 0 && d > 0 && d <= 32768 && ldz >= d,
            "probe_predict: bad shape rows=%lld n=%lld d=%d ldz=%lld", (long long)table_rows, (long long)n, d,
            (long long)ldz);
    REQUIRE((flags & ~(CLANE_PREDICT_SIGMOID | CLANE_PREDICT_WRITE_PROBA)) == 0, "probe_predict: unknown flags %d", flags);
    const bool sigmoid = (flags & CLANE_PREDICT_SIGMOID) != 0;
    REQUIRE(C >= (sigmoid ? 1 : 2) && C <= kProbeMaxClasses, "probe_predict: C must be in [%d, %d], got %d",
            sigmoid ? 1 : 2, kProbeMaxClasses, C);
    REQUIRE(top_m >= 1 && top_m <= kPredictMaxTop, "probe_predict: top_m must be in [1, %d], got %d", kPredictMaxTop,
            top_m);
    const int cp_log = probe_cp_log(C);
    REQUIRE(F >= 1 && F <= (INT32_MAX >> 7), "probe_predict: bad number of fits %d", F);
    REQUIRE(Z && rows && W && bias && top_class && top_prob, "probe_predict: null pointer");
    REQUIRE(!sigmoid || col_state, "probe_predict: CLANE_PREDICT_SIGMOID needs col_state");
    REQUIRE(!(flags & CLANE_PREDICT_WRITE_PROBA) || proba, "probe_predict: CLANE_PREDICT_WRITE_PROBA needs proba");
    const int K = F << cp_log;
    const int n_tiles = int(ceil_div(int64_t(K), int64_t(kProjBN)));
    const int64_t row_tiles = n > 0 ? probe_row_tiles(n) : 0;
    const int64_t blocks = row_tiles * n_tiles;
    REQUIRE(blocks <= INT32_MAX, "probe_predict: %lld rows x %d fits is too many for one launch", (long long)n, F);
    if (blocks == 0) return CLANE_OK;
    probe_predict_kernel<T, A><<<unsigned(blocks), kBlock, 0, (hipStream_t)stream>>>(
        Z, table_rows, d, ldz, rows, n, W, bias, col_state, F, C, cp_log, top_m, flags, top_class, top_prob, proba,
        n_tiles);
    return check_launch("probe_predict");
}

// ---- Gaussian mixtures (mixture.h): the probes' launch shapes over the 2 d wide operand [xc^2 | xc] --------------------
template <typename T, typename A>
int mixture_estep(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n, const A *mean,
                  const A *Wm, const A *cst, int32_t R, int32_t K, int32_t flags, A *resp, double *ll_ws, double *ll,
                  int32_t *assign, int64_t ld_assign, void *stream) {
    static_assert(kMixtureWriteResp == CLANE_MIXTURE_WRITE_RESP && kMixtureWriteAssign == CLANE_MIXTURE_WRITE_ASSIGN &&
                      kProbeMaxClasses == CLANE_MIXTURE_MAX_COMPONENTS,
                  "header and kernel disagree");
    // any d >= 1 whose depth 2 d, and the k loop's 2 d + 16, is an int
    REQUIRE(table_rows >= 0 && n >= 0 && d >= 1 && d <= (INT32_MAX >> 2) && ldz >= d,
            "mixture_estep: bad shape rows=%lld n=%lld d=%d ldz=%lld", (long long)table_rows, (long long)n, d,
            (long long)ldz);
    REQUIRE(K >= 1 && K <= kProbeMaxClasses, "mixture_estep: K must be in [1, %d], got %d", kProbeMaxClasses, K);
    const int cp_log = probe_cp_log(K);
    REQUIRE(R >= 1 && R <= (INT32_MAX >> 7), "mixture_estep: bad number of restarts %d", R);
    REQUIRE((flags & ~(CLANE_MIXTURE_WRITE_RESP | CLANE_MIXTURE_WRITE_ASSIGN)) == 0, "mixture_estep: unknown flags %d",
            flags);
    REQUIRE(!(flags & CLANE_MIXTURE_WRITE_ASSIGN) || ld_assign >= R, "mixture_estep: ld_assign %lld < R = %d",
            (long long)ld_assign, R);
    REQUIRE(ll_ws && ll, "mixture_estep: null likelihood workspace/output");
    REQUIRE(n == 0 || (Z && rows && mean && Wm && cst), "mixture_estep: null pointer");
    REQUIRE(n == 0 || !(flags & CLANE_MIXTURE_WRITE_RESP) || resp, "mixture_estep: CLANE_MIXTURE_WRITE_RESP needs resp");
    REQUIRE(n == 0 || !(flags & CLANE_MIXTURE_WRITE_ASSIGN) || assign,
            "mixture_estep: CLANE_MIXTURE_WRITE_ASSIGN needs assign");
    const int Kt = R << cp_log;
    const int n_tiles = int(ceil_div(int64_t(Kt), int64_t(kProjBN)));
    const int64_t row_tiles = n > 0 ? probe_row_tiles(n) : 0;
    const int64_t blocks = row_tiles * n_tiles;
    REQUIRE(blocks <= INT32_MAX, "mixture_estep: %lld rows x %d restarts is too many for one launch", (long long)n, R);
    if (blocks > 0)
        mixture_estep_kernel<T, A><<<unsigned(blocks), kBlock, 0, (hipStream_t)stream>>>(
            Z, table_rows, d, ldz, rows, n, mean, Wm, cst, R, K, cp_log, flags, resp, ll_ws, assign, ld_assign, n_tiles);
    probe_loss_reduce_kernel<<<unsigned(R), kBlock, 0, (hipStream_t)stream>>>(ll_ws, row_tiles, R, ll);
    return check_launch("mixture_estep");
}

template <typename T, typename A>
int mixture_mstep(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n, const A *mean,
                  const A *resp, int32_t K, A *ws, A *S, A *nk, void *stream) {
    REQUIRE(table_rows >= 0 && n >= 0 && d >= 1 && d <= (INT32_MAX >> 2) && ldz >= d && K >= 1,
            "mixture_mstep: bad shape rows=%lld n=%lld d=%d ldz=%lld K=%d", (long long)table_rows, (long long)n, d,
            (long long)ldz, K);
    REQUIRE(ws && S && nk, "mixture_mstep: null workspace/output");
    REQUIRE(n == 0 || (Z && rows && mean && resp), "mixture_mstep: null pointer");
    const int64_t n_chunks = n > 0 ? probe_grad_chunks(n) : 0;
    REQUIRE(n_chunks <= 65535, "mixture_mstep: %lld rows is too many for one launch", (long long)n);
    const int64_t d_tiles = ceil_div(int64_t(2 * d), int64_t(kProjBN)), k_tiles = ceil_div(int64_t(K), int64_t(kProjBM));
    REQUIRE(d_tiles * k_tiles <= INT32_MAX, "mixture_mstep: K=%d x d=%d is too many tiles for one launch", K, d);
    const int64_t len = int64_t(K) * (2 * int64_t(d) + 1);
    if (n_chunks > 0)
        mixture_mstep_kernel<T, A><<<dim3(unsigned(d_tiles * k_tiles), unsigned(n_chunks)), kBlock, 0,
                                     (hipStream_t)stream>>>(Z, table_rows, d, ldz, rows, n, mean, resp, K, ws,
                                                            int(d_tiles));
    probe_grad_reduce_kernel<A><<<unsigned(ceil_div(len, kBlock)), kBlock, 0, (hipStream_t)stream>>>(
        ws, n_chunks, len, int64_t(K) * 2 * d, S, nk);
    return check_launch("mixture_mstep");
}

// ---- node clustering (kmeans.h) ---------------------------------------------------------------------------------------
inline int64_t kmeans_windows(int64_t n, int64_t R) { return ceil_div(n > 0 && R > 0 ? n * R : 1, int64_t(kKmChunk)); }

template <typename T, typename A>
int kmeans_assign(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n, const A *centres,
                  const A *csq, int32_t R, int32_t K, int32_t *assign, int64_t ld_assign, A *best, int64_t ld_best,
                  void *stream) {
    REQUIRE(table_rows >= 0 && n >= 0 && d >= 1 && ldz >= d, "kmeans_assign: bad shape rows=%lld n=%lld d=%d ldz=%lld",
            (long long)table_rows, (long long)n, d, (long long)ldz);
    REQUIRE(K >= 1, "kmeans_assign: K must be at least 1, got %d", K);
    REQUIRE(R >= 1 && R <= 65535, "kmeans_assign: R must be in [1, 65535], got %d", R);
    REQUIRE(ld_assign >= R, "kmeans_assign: ld_assign %lld < R = %d", (long long)ld_assign, R);
    REQUIRE(ld_best >= R, "kmeans_assign: ld_best %lld < R = %d", (long long)ld_best, R);
    REQUIRE(assign && best, "kmeans_assign: null output");
    REQUIRE(n == 0 || (Z && rows && centres && csq), "kmeans_assign: null pointer");
    if (n == 0) return CLANE_OK;
    const int64_t row_tiles = ceil_div(n, int64_t(kProjBM));
    REQUIRE(row_tiles <= INT32_MAX, "kmeans_assign: %lld rows is too many for one launch", (long long)n);
    kmeans_assign_kernel<T, A><<<dim3(unsigned(row_tiles), unsigned(R)), kBlock, 0, (hipStream_t)stream>>>(
        Z, table_rows, d, ldz, rows, n, centres, csq, K, assign, ld_assign, best, ld_best);
    return check_launch("kmeans_assign");
}

template <typename T, typename A>
int kmeans_update(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order, const int64_t *seg,
                  int64_t n, int32_t R, int32_t K, const A *centres_old, A *ws, A *centres_new, A *csq_new, void *stream) {
    REQUIRE(table_rows >= 0 && n >= 0 && d >= 1 && ldz >= d, "kmeans_update: bad shape rows=%lld n=%lld d=%d ldz=%lld",
            (long long)table_rows, (long long)n, d, (long long)ldz);
    REQUIRE(K >= 1, "kmeans_update: K must be at least 1, got %d", K);
    REQUIRE(R >= 1, "kmeans_update: R must be at least 1, got %d", R);
    REQUIRE(int64_t(R) * K <= INT32_MAX, "kmeans_update: R=%d x K=%d is too many centres for one launch", R, K);
    REQUIRE(n <= INT64_MAX / R && kmeans_windows(n, R) <= INT32_MAX, "kmeans_update: %lld rows x %d restarts is too many "
            "for one launch", (long long)n, R);
    REQUIRE(ws && centres_new && csq_new, "kmeans_update: null workspace/output");
    REQUIRE(seg && centres_old, "kmeans_update: null pointer");
    REQUIRE(n == 0 || (Z && order), "kmeans_update: null pointer");
    const int64_t total = n * R, n_seg = int64_t(R) * K;
    if (total > 0) {
        const int lpr_log = km_lpr_log<T>(d);
        const unsigned grid = unsigned(kmeans_windows(n, R));
        if (aligned16(Z) && ldz % Elem<T>::kVec == 0 && d % Elem<T>::kVec == 0)
            kmeans_chunk_kernel<T, A, true><<<grid, kBlock, 0, (hipStream_t)stream>>>(
                Z, table_rows, d, ldz, order, total, seg, n_seg, lpr_log, centres_new, ws);
        else
            kmeans_chunk_kernel<T, A, false><<<grid, kBlock, 0, (hipStream_t)stream>>>(
                Z, table_rows, d, ldz, order, total, seg, n_seg, lpr_log, centres_new, ws);
    }
    kmeans_finish_kernel<A><<<unsigned(n_seg), kBlock, 0, (hipStream_t)stream>>>(seg, total, d, centres_old, ws,
                                                                                centres_new, csq_new);
    return check_launch("kmeans_update");
}

// ---- content reduction (content_pca.h) --------------------------------------------------------------------------------
inline int64_t pca_chunks(int64_t n) { return n > 0 ? ceil_div(n, int64_t(kGradChunk)) : 0; }

template <typename T>
int column_sums(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n, int32_t flags,
                double *ws, double *sums, void *stream) {
    static_assert(kPcaAccumulate == CLANE_PCA_ACCUMULATE, "header and kernel disagree");
    REQUIRE(table_rows >= 0 && n >= 0 && d > 0 && d <= 32768 && ldz >= d,
            "column_sums: bad shape rows=%lld n=%lld d=%d ldz=%lld", (long long)table_rows, (long long)n, d,
            (long long)ldz);
    REQUIRE((flags & ~CLANE_PCA_ACCUMULATE) == 0, "column_sums: unknown flags %d", flags);
    REQUIRE(ws && sums, "column_sums: null workspace/output");
    REQUIRE(n == 0 || (Z && rows), "column_sums: null pointer");
    const int64_t n_chunks = pca_chunks(n);
    REQUIRE(n_chunks <= 65535, "column_sums: %lld rows is too many for one launch", (long long)n);
    constexpr int KV = Elem<T>::kVec;
    const unsigned strips = unsigned(ceil_div(int64_t(d), int64_t(kSumColLanes * KV)));
    if (n_chunks > 0) {
        if (aligned16(Z) && ldz % KV == 0)
            column_sums_kernel<T, KV, true><<<dim3(strips, unsigned(n_chunks)), kBlock, 0, (hipStream_t)stream>>>(
                Z, table_rows, d, ldz, rows, n, ws);
        else
            column_sums_kernel<T, KV, false><<<dim3(strips, unsigned(n_chunks)), kBlock, 0, (hipStream_t)stream>>>(
                Z, table_rows, d, ldz, rows, n, ws);
    }
    column_sums_reduce_kernel<<<unsigned(ceil_div(int64_t(d), int64_t(kBlock))), kBlock, 0, (hipStream_t)stream>>>(
        ws, n_chunks, d, flags & CLANE_PCA_ACCUMULATE, sums);
    return check_launch("column_sums");
}

template <typename T, typename A>
int gram(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n, const A *mu,
         int32_t flags, A *ws, A *G, void *stream) {
    REQUIRE(table_rows >= 0 && n >= 0 && d > 0 && d <= 32768 && ldz >= d,
            "gram: bad shape rows=%lld n=%lld d=%d ldz=%lld", (long long)table_rows, (long long)n, d, (long long)ldz);
    REQUIRE((flags & ~CLANE_PCA_ACCUMULATE) == 0, "gram: unknown flags %d", flags);
    REQUIRE(ws && G, "gram: null workspace/output");
    REQUIRE(n == 0 || (Z && rows), "gram: null pointer");
    const int64_t n_chunks = pca_chunks(n);
    REQUIRE(n_chunks <= 65535, "gram: %lld rows is too many for one launch", (long long)n);
    const int64_t nt = ceil_div(int64_t(d), int64_t(kProjBN));
    const int64_t len = int64_t(d) * d;
    if (n_chunks > 0)
        gram_kernel<T, A><<<dim3(unsigned(nt * (nt + 1) / 2), unsigned(n_chunks)), kBlock, 0, (hipStream_t)stream>>>(
            Z, table_rows, d, ldz, rows, n, mu, ws, int(nt));
    gram_reduce_kernel<A><<<unsigned(ceil_div(len, int64_t(kBlock))), kBlock, 0, (hipStream_t)stream>>>(
        ws, n_chunks, d, flags & CLANE_PCA_ACCUMULATE, G);
    return check_launch("gram");
}

template <typename T, typename A>
int project_affine(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n, const A *mu,
                   const A *W, int32_t m, T *Y, int64_t ldy, void *stream) {
    REQUIRE(table_rows >= 0 && n >= 0 && d > 0 && d <= 32768 && ldz >= d && m >= 1 && ldy >= m,
            "project_affine: bad shape rows=%lld n=%lld d=%d ldz=%lld m=%d ldy=%lld", (long long)table_rows,
            (long long)n, d, (long long)ldz, m, (long long)ldy);
    if (n == 0) return CLANE_OK;
    REQUIRE(Z && rows && W && Y, "project_affine: null pointer");
    const int n_tiles = int(ceil_div(int64_t(m), int64_t(kProjBN)));
    const int64_t blocks = ceil_div(n, int64_t(kProjBM)) * n_tiles;
    REQUIRE(blocks <= INT32_MAX, "project_affine: %lld rows x %d columns is too many for one launch", (long long)n, m);
    project_affine_kernel<T, A><<<unsigned(blocks), kBlock, 0, (hipStream_t)stream>>>(Z, table_rows, d, ldz, rows, n, mu,
                                                                                       W, m, Y, ldy, n_tiles);
    return check_launch("project_affine");
}

// ---- 2-D layout (tsne.h) ------------------------------------------------------------------------------------------------
inline int64_t tsne_sym_tiles(int64_t n) { return ceil_div(n > 0 ? n : 1, int64_t(kTsneSymTile)); }

template <typename T>
int tsne_sqdist(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n, const float *mu,
                float *sq, float *D, void *stream) {
    static_assert(kTsneMaxPoints == CLANE_TSNE_MAX_POINTS, "header and kernel disagree");
    REQUIRE(table_rows >= 0 && n >= 0 && n <= kTsneMaxPoints && d > 0 && ldz >= d,
            "tsne_sqdist: bad shape rows=%lld n=%lld d=%d ldz=%lld", (long long)table_rows, (long long)n, d,
            (long long)ldz);
    if (n == 0) return CLANE_OK;
    REQUIRE(rows && mu && sq && D && (Z || table_rows == 0), "tsne_sqdist: null pointer");
    const int64_t nt = ceil_div(n, int64_t(kProjBM));
    tsne_sqnorm_kernel<T><<<unsigned(ceil_div(n, int64_t(kBlock))), kBlock, 0, (hipStream_t)stream>>>(
        Z, table_rows, d, ldz, rows, n, mu, sq);
    tsne_sqdist_kernel<T><<<unsigned(nt * (nt + 1) / 2), kBlock, 0, (hipStream_t)stream>>>(Z, table_rows, d, ldz, rows, n,
                                                                                           mu, sq, D, int(nt));
    return check_launch("tsne_sqdist");
}

// ---- neighbour-sparse 2-D layout (tsne_nn.h) --------------------------------------------------------------------------------
template <typename T>
int knn_sqdist(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n, const float *mu,
               float *sq, int32_t k, int32_t n_slabs, float *cand_sqdist, int32_t *cand_ids, float *sqdist, int32_t *ids,
               void *stream) {
    static_assert(kKnnMaxK == CLANE_KNN_MAX_K && kTsneNnMaxPoints == CLANE_TSNE_NN_MAX_POINTS, "header and kernel disagree");
    REQUIRE(table_rows >= 0 && n >= 0 && n <= kTsneNnMaxPoints && d > 0 && ldz >= d,
            "knn_sqdist: bad shape rows=%lld n=%lld d=%d ldz=%lld", (long long)table_rows, (long long)n, d, (long long)ldz);
    REQUIRE(k >= 1 && k <= CLANE_KNN_MAX_K, "knn_sqdist: k must be in [1, %d], got %d", CLANE_KNN_MAX_K, k);
    REQUIRE(n_slabs >= 1 && n_slabs <= 65536, "knn_sqdist: n_slabs must be in [1, 65536], got %d", n_slabs);
    if (n == 0) return CLANE_OK;
    REQUIRE(rows && mu && sq && sqdist && ids && (Z || table_rows == 0), "knn_sqdist: null pointer");
    REQUIRE(n_slabs == 1 || (cand_sqdist && cand_ids), "knn_sqdist: n_slabs > 1 needs the candidate workspace");
    const int mi = knn_tile_mi(k);
    const int64_t q_tiles = ceil_div(n, int64_t(32 * mi));
    const int64_t blocks = q_tiles * n_slabs;
    REQUIRE(blocks <= INT32_MAX, "knn_sqdist: %lld rows x %d slabs is too many for one launch", (long long)n, n_slabs);
    const int64_t tiles_total = ceil_div(n, int64_t(kProjBN));
    const int64_t tiles_per_slab = ceil_div(tiles_total, int64_t(n_slabs));
    float *out_d = n_slabs == 1 ? sqdist : cand_sqdist;     // one slab: its lists are the result
    int32_t *out_i = n_slabs == 1 ? ids : cand_ids;
    tsne_sqnorm_kernel<T><<<unsigned(ceil_div(n, int64_t(kBlock))), kBlock, 0, (hipStream_t)stream>>>(
        Z, table_rows, d, ldz, rows, n, mu, sq);
    auto launch = [&]<int MI>() {
        knn_sqdist_kernel<T, MI><<<unsigned(blocks), kBlock, knn_list_bytes(MI, k), (hipStream_t)stream>>>(
            Z, table_rows, d, ldz, rows, n, mu, sq, k, n_slabs, q_tiles, tiles_per_slab, out_d, out_i);
    };
    if (mi == 4) launch.template operator()<4>();
    else if (mi == 2) launch.template operator()<2>();
    else launch.template operator()<1>();
    if (n_slabs > 1)
        knn_merge_kernel<<<unsigned(ceil_div(n, int64_t(kWavesPerBlock))), kBlock, 0, (hipStream_t)stream>>>(
            cand_sqdist, cand_ids, n, n_slabs, k, sqdist, ids);
    return check_launch("knn_sqdist");
}

// ---- silhouette (silhouette.h) ------------------------------------------------------------------------------------------
inline int silhouette_check(const char *what, int64_t table_rows, int64_t n, int32_t d, int64_t ldz, int32_t metric) {
    static_assert(kSilEuclidean == CLANE_SILHOUETTE_EUCLIDEAN && kSilCosine == CLANE_SILHOUETTE_COSINE,
                  "header and kernel disagree");
    REQUIRE(table_rows >= 0 && n >= 0 && d >= 1 && ldz >= d, "%s: bad shape rows=%lld n=%lld d=%d ldz=%lld", what,
            (long long)table_rows, (long long)n, d, (long long)ldz);
    REQUIRE(metric == CLANE_SILHOUETTE_EUCLIDEAN || metric == CLANE_SILHOUETTE_COSINE, "%s: unknown metric %d", what,
            metric);
    return CLANE_OK;
}

template <typename T, typename A>
int silhouette_norms(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order, int64_t n, const A *mu,
                     int32_t metric, A *nrm, void *stream) {
    if (int rc = silhouette_check("silhouette_norms", table_rows, n, d, ldz, metric)) return rc;
    if (n == 0) return CLANE_OK;
    REQUIRE(order && mu && nrm && (Z || table_rows == 0), "silhouette_norms: null pointer");
    const int64_t tiles = ceil_div(n, int64_t(kProjBM));
    REQUIRE(tiles <= INT32_MAX, "silhouette_norms: %lld rows is too many for one launch", (long long)n);
    silhouette_norms_kernel<T, A><<<unsigned(tiles), kBlock, 0, (hipStream_t)stream>>>(Z, table_rows, d, ldz, order, n, mu,
                                                                                       metric, nrm);
    return check_launch("silhouette_norms");
}

template <typename T, typename A>
int silhouette_sums(const T *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order, int64_t n,
                    const int64_t *seg, int32_t K, const A *mu, const A *nrm, int32_t metric, int64_t p0, int64_t p1,
                    double *S, void *stream) {
    if (int rc = silhouette_check("silhouette_sums", table_rows, n, d, ldz, metric)) return rc;
    REQUIRE(K >= 1, "silhouette_sums: K must be at least 1, got %d", K);
    REQUIRE(p0 >= 0 && p0 <= p1 && p1 <= n, "silhouette_sums: positions [%lld, %lld) are not within [0, n = %lld]",
            (long long)p0, (long long)p1, (long long)n);
    if (p1 == p0) return CLANE_OK;
    REQUIRE(order && seg && mu && nrm && S && (Z || table_rows == 0), "silhouette_sums: null pointer");
    const int64_t row_tiles = ceil_div(p1 - p0, int64_t(kProjBM));
    REQUIRE(row_tiles * K <= INT32_MAX, "silhouette_sums: %lld positions x %d clusters is too many for one launch",
            (long long)(p1 - p0), K);
    silhouette_sums_kernel<T, A><<<unsigned(row_tiles * K), kBlock, 0, (hipStream_t)stream>>>(
        Z, table_rows, d, ldz, order, n, seg, K, mu, nrm, metric, p0, p1, int(row_tiles), S);
    return check_launch("silhouette_sums");
}

// ---- sparse rows (sparse_rows.h) ----------------------------------------------------------------------------------------
inline int64_t csr_max_items(int64_t nnz) { return nnz > kCsrSegment ? 2 * (nnz / kCsrSegment) : 0; }

inline int csr_check_items(const char *what, int64_t n_rows, int64_t nnz, const void *long_rows, const void *seg_ptr,
                           const void *item_long, int64_t n_long, int64_t n_items) {
    REQUIRE(n_long >= 0 && n_items >= n_long && n_long <= n_rows && n_items <= csr_max_items(nnz) &&
                (n_long == 0 || n_items >= 2 * n_long),
            "%s: %lld long rows in %lld segments cannot belong to %lld rows of %lld non-zeros", what, (long long)n_long,
            (long long)n_items, (long long)n_rows, (long long)nnz);
    REQUIRE(n_long == 0 || (long_rows && seg_ptr && item_long), "%s: null segment list", what);
    return CLANE_OK;
}

int csr_spmm(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows, int64_t nnz, const float *B,
             int64_t b_rows, int64_t ldb, int32_t l, const float *a, const float *s, const int32_t *long_rows,
             const int64_t *seg_ptr, const int32_t *item_long, int64_t n_long, int64_t n_items, float *ws, int64_t ws_len,
             float *out, int64_t ldo, void *stream) {
    static_assert(kCsrSegment == CLANE_CSR_SEGMENT && kCsrMaxL == CLANE_CSR_MAX_L && kCsrSegment % kWave == 0,
                  "header and kernel disagree");
    REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX && nnz >= 0 && b_rows >= 0 && b_rows <= INT32_MAX && l >= 4 &&
                l <= kCsrMaxL && l % 4 == 0 && ldb >= l && ldo >= l,
            "csr_spmm: bad shape rows=%lld nnz=%lld b_rows=%lld l=%d ldb=%lld ldo=%lld", (long long)n_rows, (long long)nnz,
            (long long)b_rows, l, (long long)ldb, (long long)ldo);
    if (const int rc = csr_check_items("csr_spmm", n_rows, nnz, long_rows, seg_ptr, item_long, n_long, n_items)) return rc;
    if (n_rows == 0) return CLANE_OK;
    REQUIRE(rowptr && out && (nnz == 0 || (col && val && B)), "csr_spmm: null pointer");
    REQUIRE(n_items == 0 || (ws && ws_len >= n_items * int64_t(l)), "csr_spmm: the workspace needs %lld elements",
            (long long)(n_items * int64_t(l)));
    REQUIRE(aligned16(B) && aligned16(out) && aligned16(ws) && aligned16(s) && ldb % 4 == 0 && ldo % 4 == 0,
            "csr_spmm: B, out, ws and s must be 16-byte aligned, ldb and ldo multiples of 4");
    const int rpb = rows_per_block(n_rows);
    const int64_t item_blocks = ceil_div(n_items, int64_t(kWavesPerBlock));
    const int64_t grid = item_blocks + ceil_div(n_rows, int64_t(rpb));
    REQUIRE(grid <= INT32_MAX, "csr_spmm: %lld rows and %lld segments are too many for one launch", (long long)n_rows,
            (long long)n_items);
#define CLANE_CSR_LAUNCH(LPR, NP)                                                                                      \
    csr_spmm_kernel<LPR, NP><<<unsigned(grid), kBlock, 0, (hipStream_t)stream>>>(                                      \
        rowptr, col, val, n_rows, B, ldb, l, a, s, long_rows, seg_ptr, item_long, n_items, item_blocks, rpb, ws, out, ldo)
    if (l <= 64) CLANE_CSR_LAUNCH(16, 1);
    else if (l <= 128) CLANE_CSR_LAUNCH(32, 1);
    else if (l <= 256) CLANE_CSR_LAUNCH(64, 1);
    else CLANE_CSR_LAUNCH(64, 2);
#undef CLANE_CSR_LAUNCH
    if (n_long > 0)
        csr_spmm_combine_kernel<<<unsigned(ceil_div(n_long, int64_t(kWavesPerBlock))), kBlock, 0, (hipStream_t)stream>>>(
            long_rows, seg_ptr, n_long, l, a, s, ws, out, ldo);
    return check_launch("csr_spmm");
}

int csr_row_sums(const int64_t *rowptr, const float *val, int64_t n_rows, int64_t nnz, const int32_t *long_rows,
                 const int64_t *seg_ptr, const int32_t *item_long, int64_t n_long, int64_t n_items, double *ws,
                 int64_t ws_len, double *sums, void *stream) {
    REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX && nnz >= 0, "csr_row_sums: bad shape rows=%lld nnz=%lld",
            (long long)n_rows, (long long)nnz);
    if (const int rc = csr_check_items("csr_row_sums", n_rows, nnz, long_rows, seg_ptr, item_long, n_long, n_items))
        return rc;
    if (n_rows == 0) return CLANE_OK;
    REQUIRE(rowptr && sums && (nnz == 0 || val), "csr_row_sums: null pointer");
    REQUIRE(n_items == 0 || (ws && ws_len >= n_items), "csr_row_sums: the workspace needs %lld doubles",
            (long long)n_items);
    const int rpb = rows_per_block(n_rows);
    const int64_t item_blocks = ceil_div(n_items, int64_t(kWavesPerBlock));
    const int64_t grid = item_blocks + ceil_div(n_rows, int64_t(rpb));
    REQUIRE(grid <= INT32_MAX, "csr_row_sums: %lld rows and %lld segments are too many for one launch", (long long)n_rows,
            (long long)n_items);
    csr_row_sums_kernel<<<unsigned(grid), kBlock, 0, (hipStream_t)stream>>>(rowptr, val, n_rows, long_rows, seg_ptr,
                                                                            item_long, n_items, item_blocks, rpb, ws, sums);
    if (n_long > 0)
        csr_row_sums_combine_kernel<<<unsigned(ceil_div(n_long, int64_t(kBlock))), kBlock, 0, (hipStream_t)stream>>>(
            long_rows, seg_ptr, n_long, ws, sums);
    return check_launch("csr_row_sums");
}


}  // namespace

// ---------------------------------------------------------------------------------------------
extern "C" {

int clane_abi_version(void) { return CLANE_ABI_VERSION; }
const char *clane_last_error(void) { return g_err; }
#define CLANE_STR2(x) #x
#define CLANE_STR(x) CLANE_STR2(x)
const char *clane_build_info(void) {
    return "arch=gfx950;SPMM_U=" CLANE_STR(CLANE_SPMM_U) ";LONG_U=" CLANE_STR(CLANE_LONG_U) ";LONG_WAVES=" CLANE_STR(
        CLANE_LONG_WAVES) ";ROWS_PER_BLOCK=" CLANE_STR(CLANE_ROWS_PER_BLOCK) ";NT_STREAM=" CLANE_STR(CLANE_NT_STREAM) ";NT_SLAB=" CLANE_STR(CLANE_NT_SLAB)
        ";TARGET_GRID=" CLANE_STR(CLANE_TARGET_GRID) ";SPMM_DYNAMIC=" CLANE_STR(CLANE_SPMM_DYNAMIC) ";SPMM_PREFETCH=" CLANE_STR(CLANE_SPMM_PREFETCH)
        ";COMBINE_WAVES=" CLANE_STR(CLANE_COMBINE_WAVES) ";XOR_DPP=" CLANE_STR(CLANE_XOR_DPP) ";COMBINE_LOADS=" CLANE_STR(CLANE_COMBINE_LOADS) ";SUBROW_U32=" CLANE_STR(CLANE_SUBROW_U32) ";CLASS_U32=" CLANE_STR(CLANE_CLASS_U32) ";CLASS_U16B=" CLANE_STR(CLANE_CLASS_U16B);
}

int clane_xcc_ids(int32_t *out, int64_t n_blocks, int32_t block_threads, void *stream) {
    if (!out || n_blocks <= 0 || n_blocks > INT32_MAX || block_threads < 64 || block_threads > 1024 || block_threads % 64)
        return fail(CLANE_ERR_INVALID_ARGUMENT, "xcc_ids: bad arguments");
    xcc_ids_kernel<<<unsigned(n_blocks), unsigned(block_threads), 0, (hipStream_t)stream>>>(out);
    return check_launch("xcc_ids");
}

int clane_check_csr(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t n_edges, int64_t table_rows,
                    int32_t *status, void *stream) {
    if (!rowptr || !status || nrows < 0 || n_edges < 0 || table_rows < 0 || (n_edges > 0 && !colidx))
        return fail(CLANE_ERR_INVALID_ARGUMENT, "check_csr: bad arguments");
    const int64_t work = n_edges > nrows + 1 ? n_edges : nrows + 1;
    const int64_t blocks = ceil_div(work, int64_t(kBlock) * 8);
    check_csr_kernel<<<unsigned(blocks < 1 ? 1 : blocks > 65536 ? 65536 : blocks), kBlock, 0, (hipStream_t)stream>>>(
        rowptr, colidx, nrows, n_edges, table_rows, status);
    return check_launch("check_csr");
}

int64_t clane_spmm_partials_len(int64_t nrows, int64_t n_long) {
    return spmm_main_grid(nrows > 0 ? nrows : 1) + (n_long > 0 ? n_long : 0);
}
int64_t clane_reduce_ws_len(void) { return kReduceWs; }

// ---- device memory that other processes can map (peer-to-peer halo rows) -----------------------------------
#define HIP_REQUIRE(call, what)                                                                  \
    do {                                                                                         \
        const hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                                  \
            return fail(CLANE_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e_));                \
        }                                                                                        \
    } while (0)

int clane_device_alloc(int64_t bytes, void **ptr) {
    REQUIRE(bytes > 0 && ptr, "device_alloc: bad arguments");
    HIP_REQUIRE(hipMalloc(ptr, size_t(bytes)), "hipMalloc");
    return CLANE_OK;
}
int clane_device_alloc_contiguous(int64_t bytes, void **ptr) {
    REQUIRE(bytes > 0 && ptr, "device_alloc_contiguous: bad arguments");
    HIP_REQUIRE(hipExtMallocWithFlags(ptr, size_t(bytes), hipDeviceMallocContiguous), "hipExtMallocWithFlags(contiguous)");
    return CLANE_OK;
}
int clane_device_free(void *ptr) {
    HIP_REQUIRE(hipFree(ptr), "hipFree");
    return CLANE_OK;
}
int clane_ipc_export(void *ptr, void *handle64) {
    static_assert(sizeof(hipIpcMemHandle_t) == CLANE_IPC_HANDLE_BYTES, "handle size");
    REQUIRE(ptr && handle64, "ipc_export: null pointer");
    hipIpcMemHandle_t h;
    HIP_REQUIRE(hipIpcGetMemHandle(&h, ptr), "hipIpcGetMemHandle");
    std::memcpy(handle64, &h, sizeof h);
    return CLANE_OK;
}
int clane_ipc_open(const void *handle64, void **ptr) {
    REQUIRE(ptr && handle64, "ipc_open: null pointer");
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle64, sizeof h);
    HIP_REQUIRE(hipIpcOpenMemHandle(ptr, h, hipIpcMemLazyEnablePeerAccess), "hipIpcOpenMemHandle");
    return CLANE_OK;
}
int clane_ipc_close(void *ptr) {
    HIP_REQUIRE(hipIpcCloseMemHandle(ptr), "hipIpcCloseMemHandle");
    return CLANE_OK;
}

int clane_row_sqnorm_f32(const float *Z, int64_t nrows, int32_t d, int64_t ldz, float *sq, void *stream) {
    return row_sqnorm<float>(Z, nrows, d, ldz, sq, stream);
}
int clane_row_sqnorm_f64(const double *Z, int64_t nrows, int32_t d, int64_t ldz, double *sq, void *stream) {
    return row_sqnorm<double>(Z, nrows, d, ldz, sq, stream);
}
int clane_row_sqnorm_bf16(const uint16_t *Z, int64_t nrows, int32_t d, int64_t ldz, float *sq, void *stream) {
    return row_sqnorm<bf16_t>(reinterpret_cast<const bf16_t *>(Z), nrows, d, ldz, sq, stream);
}

int clane_degree_weighted_sums_f32(const float *sq, const int64_t *rowptr, const int32_t *indeg, int64_t nrows,
                                   double *ws, double *out2, void *stream) {
    return degree_weighted_sums<float>(sq, rowptr, indeg, nrows, ws, out2, stream);
}
int clane_degree_weighted_sums_f64(const double *sq, const int64_t *rowptr, const int32_t *indeg, int64_t nrows,
                                   double *ws, double *out2, void *stream) {
    return degree_weighted_sums<double>(sq, rowptr, indeg, nrows, ws, out2, stream);
}

#define CLANE_EDGE_SCORE_WRAPPER(SUF, CT, T, AT)                                                                      \
    int clane_edge_score_##SUF(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0,             \
                               const CT *Z, int64_t ldz, int32_t d, int32_t mode, const double *sums2, const AT *sq,  \
                               AT *scores, int32_t flags, int64_t long_threshold, const int32_t *long_rows,           \
                               int64_t n_long, void *stream) {                                                        \
        return edge_score<T>(rowptr, colidx, nrows, row0, reinterpret_cast<const T *>(Z), ldz, d, mode, sums2, sq,    \
                             scores, flags, long_threshold, long_rows, n_long, stream);                               \
    }
CLANE_EDGE_SCORE_WRAPPER(f32, float, float, float)
CLANE_EDGE_SCORE_WRAPPER(f64, double, double, double)
CLANE_EDGE_SCORE_WRAPPER(bf16, uint16_t, bf16_t, float)
#undef CLANE_EDGE_SCORE_WRAPPER
#define CLANE_EDGE_SCORE_CLASS_WRAPPER(SUF, CT, T, AT)                                                                \
    int clane_edge_score_class_##SUF(const int64_t *rowptr, const int32_t *colidx, const int64_t *item_e0,            \
                                     const int32_t *item_len, const int32_t *item_slot, const int32_t *item_row,      \
                                     int64_t n_blocks, int32_t items_per_block, const int32_t *class_rows,            \
                                     const int64_t *slot_ptr, int64_t n_rows, int64_t row0, const CT *Z, int64_t ldz, \
                                     int32_t d, int32_t mode, const double *sums2, const AT *sq, AT *scores,          \
                                     int32_t flags, AT *stats, void *stream) {                                        \
        return edge_score_class<T>(rowptr, colidx, item_e0, item_len, item_slot, item_row, n_blocks, items_per_block, \
                                   class_rows, slot_ptr, n_rows, row0, reinterpret_cast<const T *>(Z), ldz, d, mode,  \
                                   sums2, sq, scores, flags, stats, stream);                                          \
    }
CLANE_EDGE_SCORE_CLASS_WRAPPER(f32, float, float, float)
CLANE_EDGE_SCORE_CLASS_WRAPPER(f64, double, double, double)
CLANE_EDGE_SCORE_CLASS_WRAPPER(bf16, uint16_t, bf16_t, float)
#undef CLANE_EDGE_SCORE_CLASS_WRAPPER

int clane_project_rows_f32(const float *Z, int64_t rows, int32_t d, int64_t ldz, const float *W, float *Y, int64_t ldy,
                           void *stream) {
    return project_rows<float, float>(Z, rows, d, ldz, W, Y, ldy, stream);
}
int clane_project_rows_f64(const double *Z, int64_t rows, int32_t d, int64_t ldz, const double *W, double *Y,
                           int64_t ldy, void *stream) {
    return project_rows<double, double>(Z, rows, d, ldz, W, Y, ldy, stream);
}
int clane_project_rows_bf16(const uint16_t *Z, int64_t rows, int32_t d, int64_t ldz, const float *W, float *Y,
                            int64_t ldy, void *stream) {
    return project_rows<bf16_t, float>(reinterpret_cast<const bf16_t *>(Z), rows, d, ldz, W, Y, ldy, stream);
}

#define CLANE_EDGE_SCORE_PAIR_WRAPPERS(SUF, T)                                                                         \
    int clane_edge_score_pair_##SUF(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0,         \
                                    const T *S, int64_t lds, const T *N, int64_t ldn, int32_t d, T *scores,            \
                                    int32_t flags, int64_t long_threshold, const int32_t *long_rows, int64_t n_long,   \
                                    void *stream) {                                                                    \
        return edge_score_pair<T>(rowptr, colidx, nrows, row0, S, lds, N, ldn, d, scores, flags, long_threshold,      \
                                  long_rows, n_long, stream);                                                          \
    }                                                                                                                  \
    int clane_edge_score_class_pair_##SUF(const int64_t *rowptr, const int32_t *colidx, const int64_t *item_e0,        \
                                          const int32_t *item_len, const int32_t *item_slot, const int32_t *item_row,  \
                                          int64_t n_blocks, int32_t items_per_block, const int32_t *class_rows,        \
                                          const int64_t *slot_ptr, int64_t n_rows, int64_t row0, const T *S,           \
                                          int64_t lds, const T *N, int64_t ldn, int32_t d, T *scores, int32_t flags,   \
                                          T *stats, void *stream) {                                                    \
        return edge_score_class_pair<T>(rowptr, colidx, item_e0, item_len, item_slot, item_row, n_blocks,             \
                                        items_per_block, class_rows, slot_ptr, n_rows, row0, S, lds, N, ldn, d,       \
                                        scores, flags, stats, stream);                                                 \
    }
CLANE_EDGE_SCORE_PAIR_WRAPPERS(f32, float)
CLANE_EDGE_SCORE_PAIR_WRAPPERS(f64, double)
#undef CLANE_EDGE_SCORE_PAIR_WRAPPERS

int clane_edge_score_finalize_f32(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0,
                                  int32_t mode, const double *sums2, const float *sq, float *scores, void *stream) {
    return edge_score_finalize<float>(rowptr, colidx, nrows, row0, mode, sums2, sq, scores, stream);
}
int clane_edge_score_finalize_f64(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0,
                                  int32_t mode, const double *sums2, const double *sq, double *scores, void *stream) {
    return edge_score_finalize<double>(rowptr, colidx, nrows, row0, mode, sums2, sq, scores, stream);
}
int clane_segment_softmax_f32(const int64_t *rowptr, int64_t nrows, float *vals, int64_t min_degree,
                              int64_t max_degree, const int32_t *long_rows, int64_t n_long, void *stream) {
    return segment_softmax<float>(rowptr, nrows, vals, min_degree, max_degree, long_rows, n_long, stream);
}
int clane_segment_softmax_f64(const int64_t *rowptr, int64_t nrows, double *vals, int64_t min_degree,
                              int64_t max_degree, const int32_t *long_rows, int64_t n_long, void *stream) {
    return segment_softmax<double>(rowptr, nrows, vals, min_degree, max_degree, long_rows, n_long, stream);
}

// K3: a per-tile call is its pass's launcher on one tile of d columns; TABLES packs what every K3 call spells the same way
#define TABLES(T, ...) tables<T>(Z_old, ldz, X, ldx, gamma, Z_new, ldo, d __VA_OPT__(, ) __VA_ARGS__)
#define CLANE_SPMM_WRAPPERS(SUF, CT, T, PT, GT)                                                                        \
    int clane_spmm_update_##SUF(const int64_t *rowptr, const int32_t *colidx, const PT *P, int64_t nrows,             \
                                int64_t row0, const CT *Z_old, int64_t ldz, const CT *X, int64_t ldx, GT gamma,       \
                                CT *Z_new, int64_t ldo, int32_t d, int64_t long_threshold, int32_t flags,             \
                                const clane_mirror_t *mirror, double *delta_partials, void *stream) {                \
        return spmm_update_impl<T, PT, false>("spmm_update", rowptr, colidx, P, nrows, row0, TABLES(T, mirror),       \
                                              Tiles{d, 0}, long_threshold, flags, delta_partials, stream);            \
    }                                                                                                                 \
    int clane_spmm_update_long_##SUF(const int64_t *rowptr, const int32_t *colidx, const PT *P,                       \
                                     const int32_t *long_rows, int64_t n_long, int32_t waves_per_row, int64_t row0,   \
                                     const CT *Z_old, int64_t ldz, const CT *X, int64_t ldx, GT gamma, CT *Z_new,     \
                                     int64_t ldo, int32_t d, const clane_mirror_t *mirror, double *delta_partials,    \
                                     void *stream) {                                                                  \
        return spmm_update_long<T, PT>(rowptr, colidx, P, long_rows, n_long, waves_per_row, row0, TABLES(T, mirror),  \
                                       delta_partials, stream);                                                       \
    }                                                                                                                 \
    int clane_spmm_update_split_##SUF(const int64_t *rowptr, const int32_t *colidx, const PT *P,                      \
                                      const int32_t *split_rows, const int64_t *seg_ptr, const int32_t *seg_row,      \
                                      int64_t n_split, int64_t n_segments, int64_t edges_per_segment, int64_t row0,   \
                                      const CT *Z_old, int64_t ldz, const CT *X, int64_t ldx, GT gamma, CT *Z_new,    \
                                      int64_t ldo, int32_t d, GT *slab, const clane_mirror_t *mirror,                 \
                                      double *delta_partials, void *stream) {                                         \
        return spmm_update_split<T, PT>(rowptr, colidx, P, split_rows, seg_ptr, seg_row, n_split, n_segments,         \
                                        edges_per_segment, row0, TABLES(T, mirror), slab, delta_partials, stream);    \
    }                                                                                                                 \
    int clane_spmm_update_class_##SUF(const int32_t *colidx, const PT *P, const int64_t *item_e0,                     \
                                      const int32_t *item_len, const int32_t *item_slot, int64_t n_blocks,            \
                                      int32_t items_per_block, const int32_t *class_rows, const int64_t *slot_ptr,    \
                                      int64_t n_rows, int64_t row0, const CT *Z_old, int64_t ldz, const CT *X,        \
                                      int64_t ldx, GT gamma, CT *Z_new, int64_t ldo, int32_t d, int32_t flags,        \
                                      GT *slab, const clane_mirror_t *mirror, double *delta_partials, void *stream) { \
        return spmm_update_class_impl<T, PT, false>("spmm_update_class", colidx, P, item_e0, item_len, item_slot,     \
                                                    n_blocks, items_per_block, class_rows, slot_ptr, n_rows, 0, row0, \
                                                    TABLES(T, mirror), Tiles{d, 0}, flags, slab, delta_partials,      \
                                                    stream);                                                          \
    }
int clane_spmm_update_owned_f32(const int32_t *colidx, const float *P, const clane_owned_plan_t *plan,
                                int32_t block_threads, int64_t row0, const float *Z_old, int64_t ldz, const float *X,
                                int64_t ldx, float gamma, float *Z_new, int64_t ldo, int32_t d, int32_t flags,
                                double *delta_partials, void *stream) {
    return spmm_update_owned_impl<float, float>("spmm_update_owned", colidx, P, plan, block_threads, row0, TABLES(float),
                                                Tiles{d, 0}, false, flags, delta_partials, stream);
}
// ---- every column tile of a pass in one launch (csrc/spmm_update.h, spmm_update_tiles_kernel): float only ----------
int clane_spmm_update_tiles_f32(const int64_t *rowptr, const int32_t *colidx, const float *P, int64_t nrows, int64_t row0,
                                const float *Z_old, int64_t ldz, const float *X, int64_t ldx, float gamma, float *Z_new,
                                int64_t ldo, int32_t d, int32_t tile_cols, int64_t long_threshold, int32_t flags,
                                double *delta_partials, int64_t partials_tile_stride, void *stream) {
    return spmm_update_impl<float, float, true>("spmm_update_tiles", rowptr, colidx, P, nrows, row0, TABLES(float),
                                                Tiles{tile_cols, partials_tile_stride}, long_threshold, flags,
                                                delta_partials, stream);
}
int clane_spmm_update_class_tiles_f32(const int32_t *colidx, const float *P, const int64_t *item_e0,
                                      const int32_t *item_len, const int32_t *item_slot, int64_t n_blocks,
                                      int32_t items_per_block, const int32_t *class_rows, const int64_t *slot_ptr,
                                      int64_t n_rows, int64_t n_slots, int64_t row0, const float *Z_old, int64_t ldz,
                                      const float *X, int64_t ldx, float gamma, float *Z_new, int64_t ldo, int32_t d,
                                      int32_t tile_cols, int32_t flags, float *slab, double *delta_partials,
                                      int64_t partials_tile_stride, void *stream) {
    return spmm_update_class_impl<float, float, true>("spmm_update_class_tiles", colidx, P, item_e0, item_len, item_slot,
                                                      n_blocks, items_per_block, class_rows, slot_ptr, n_rows, n_slots,
                                                      row0, TABLES(float), Tiles{tile_cols, partials_tile_stride}, flags,
                                                      slab, delta_partials, stream);
}
int clane_spmm_update_owned_tiles_f32(const int32_t *colidx, const float *P, const clane_owned_plan_t *plan,
                                      int32_t block_threads, int64_t row0, const float *Z_old, int64_t ldz,
                                      const float *X, int64_t ldx, float gamma, float *Z_new, int64_t ldo, int32_t d,
                                      int32_t tile_cols, int32_t flags, double *delta_partials,
                                      int64_t partials_tile_stride, void *stream) {
    return spmm_update_owned_impl<float, float>("spmm_update_owned_tiles", colidx, P, plan, block_threads, row0,
                                                TABLES(float), Tiles{tile_cols, partials_tile_stride}, true, flags,
                                                delta_partials, stream);
}
// ---- one weight per row instead of one per edge (csrc/spmm_update.h, UNIFORM): float only, no mirror ----------------
int clane_row_weight_f32(const int64_t *rowptr, const float *P, int64_t nrows, float *row_weight, int32_t *mixed,
                         void *stream) {
    return row_weights<float>(rowptr, P, nrows, row_weight, mixed, stream);
}
int clane_row_weight_f64(const int64_t *rowptr, const double *P, int64_t nrows, double *row_weight, int32_t *mixed,
                         void *stream) {
    return row_weights<double>(rowptr, P, nrows, row_weight, mixed, stream);
}
int clane_spmm_update_rw_f32(const int64_t *rowptr, const int32_t *colidx, const float *row_weight, int64_t nrows,
                             int64_t row0, const float *Z_old, int64_t ldz, const float *X, int64_t ldx, float gamma,
                             float *Z_new, int64_t ldo, int32_t d, int64_t long_threshold, int32_t flags,
                             double *delta_partials, void *stream) {
    return spmm_update_impl<float, float, false, true>("spmm_update_rw", rowptr, colidx, row_weight, nrows, row0,
                                                       TABLES(float), Tiles{d, 0}, long_threshold, flags, delta_partials,
                                                       stream);
}
int clane_spmm_update_tiles_rw_f32(const int64_t *rowptr, const int32_t *colidx, const float *row_weight, int64_t nrows,
                                   int64_t row0, const float *Z_old, int64_t ldz, const float *X, int64_t ldx, float gamma,
                                   float *Z_new, int64_t ldo, int32_t d, int32_t tile_cols, int64_t long_threshold,
                                   int32_t flags, double *delta_partials, int64_t partials_tile_stride, void *stream) {
    return spmm_update_impl<float, float, true, true>("spmm_update_tiles_rw", rowptr, colidx, row_weight, nrows, row0,
                                                      TABLES(float), Tiles{tile_cols, partials_tile_stride}, long_threshold,
                                                      flags, delta_partials, stream);
}
int clane_spmm_update_class_rw_f32(const int32_t *colidx, const float *row_weight, const int64_t *item_e0,
                                   const int32_t *item_len, const int32_t *item_slot, const int32_t *item_row,
                                   int64_t n_blocks, int32_t items_per_block, const int32_t *class_rows,
                                   const int64_t *slot_ptr, int64_t n_rows, int64_t row0, const float *Z_old, int64_t ldz,
                                   const float *X, int64_t ldx, float gamma, float *Z_new, int64_t ldo, int32_t d,
                                   int32_t flags, float *slab, double *delta_partials, void *stream) {
    return spmm_update_class_impl<float, float, false, true>("spmm_update_class_rw", colidx, row_weight, item_e0, item_len,
                                                             item_slot, n_blocks, items_per_block, class_rows, slot_ptr,
                                                             n_rows, 0, row0, TABLES(float), Tiles{d, 0}, flags, slab,
                                                             delta_partials, stream, item_row);
}
int clane_spmm_update_class_tiles_rw_f32(const int32_t *colidx, const float *row_weight, const int64_t *item_e0,
                                         const int32_t *item_len, const int32_t *item_slot, const int32_t *item_row,
                                         int64_t n_blocks, int32_t items_per_block, const int32_t *class_rows,
                                         const int64_t *slot_ptr, int64_t n_rows, int64_t n_slots, int64_t row0,
                                         const float *Z_old, int64_t ldz, const float *X, int64_t ldx, float gamma,
                                         float *Z_new, int64_t ldo, int32_t d, int32_t tile_cols, int32_t flags,
                                         float *slab, double *delta_partials, int64_t partials_tile_stride,
                                         void *stream) {
    return spmm_update_class_impl<float, float, true, true>("spmm_update_class_tiles_rw", colidx, row_weight, item_e0,
                                                            item_len, item_slot, n_blocks, items_per_block, class_rows,
                                                            slot_ptr, n_rows, n_slots, row0, TABLES(float),
                                                            Tiles{tile_cols, partials_tile_stride}, flags, slab,
                                                            delta_partials, stream, item_row);
}
int clane_spmm_update_owned_rw_f32(const int32_t *colidx, const float *row_weight, const clane_owned_plan_t *plan,
                                   const int32_t *seg_row, int32_t block_threads, int64_t row0, const float *Z_old,
                                   int64_t ldz, const float *X, int64_t ldx, float gamma, float *Z_new, int64_t ldo,
                                   int32_t d, int32_t flags, double *delta_partials, void *stream) {
    return spmm_update_owned_impl<float, float, true>("spmm_update_owned_rw", colidx, row_weight, plan, block_threads, row0,
                                                      TABLES(float), Tiles{d, 0}, false, flags, delta_partials, stream,
                                                      seg_row);
}
int clane_spmm_update_owned_tiles_rw_f32(const int32_t *colidx, const float *row_weight, const clane_owned_plan_t *plan,
                                         const int32_t *seg_row, int32_t block_threads, int64_t row0, const float *Z_old,
                                         int64_t ldz, const float *X, int64_t ldx, float gamma, float *Z_new, int64_t ldo,
                                         int32_t d, int32_t tile_cols, int32_t flags, double *delta_partials,
                                         int64_t partials_tile_stride, void *stream) {
    return spmm_update_owned_impl<float, float, true>("spmm_update_owned_tiles_rw", colidx, row_weight, plan, block_threads,
                                                      row0, TABLES(float), Tiles{tile_cols, partials_tile_stride}, true,
                                                      flags, delta_partials, stream, seg_row);
}

int64_t clane_spmm_class_slab_len(int64_t n_slots, int32_t d) { return n_slots * (ceil_div(d, 8) * 8); }
int64_t clane_spmm_split_slab_len(int64_t n_segments, int32_t d) { return n_segments * (ceil_div(d, 8) * 8); }

CLANE_SPMM_WRAPPERS(f32, float, float, float, float)
CLANE_SPMM_WRAPPERS(f64, double, double, double, double)
CLANE_SPMM_WRAPPERS(bf16, uint16_t, bf16_t, float, float)
#undef CLANE_SPMM_WRAPPERS
#undef TABLES

int clane_reduce_partials(const double *partials, int64_t n, double *ws, double *out, void *stream) {
    if (n < 0 || !out || !ws || (n > 0 && !partials))
        return fail(CLANE_ERR_INVALID_ARGUMENT, "reduce_partials: bad arguments");
    if (n <= 8192) {
        reduce_fixed_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(partials, n, n, 1, out);
    } else {  // two stages, both in a fixed order: kReduceGrid slice sums, then their sum
        const int64_t slice = ceil_div(n, kReduceGrid);
        const int grid = int(ceil_div(n, slice));
        reduce_slices_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(partials, n, slice, ws);
        reduce_fixed_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(ws, grid, grid, 1, out);
    }
    return check_launch("reduce_partials");
}

int clane_l1_distance_f32(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t nrows, int32_t d,
                          float *sq_a, double *ws, double *out, void *stream) {
    return l1_distance<float>(A, lda, B, ldb, nrows, d, sq_a, ws, out, stream);
}
int clane_l1_distance_f64(const double *A, int64_t lda, const double *B, int64_t ldb, int64_t nrows, int32_t d,
                          double *sq_a, double *ws, double *out, void *stream) {
    return l1_distance<double>(A, lda, B, ldb, nrows, d, sq_a, ws, out, stream);
}
int clane_l1_distance_bf16(const uint16_t *A, int64_t lda, const uint16_t *B, int64_t ldb, int64_t nrows, int32_t d,
                           float *sq_a, double *ws, double *out, void *stream) {
    return l1_distance<bf16_t>(reinterpret_cast<const bf16_t *>(A), lda, reinterpret_cast<const bf16_t *>(B), ldb,
                               nrows, d, sq_a, ws, out, stream);
}

int clane_gather_rows_f32(const float *src, int64_t lds, const int32_t *idx, int64_t n, int32_t d, float *dst,
                          int64_t ldd, void *stream) {
    return gather_rows<float>(src, lds, idx, n, d, dst, ldd, stream);
}
int clane_gather_rows_f64(const double *src, int64_t lds, const int32_t *idx, int64_t n, int32_t d, double *dst,
                          int64_t ldd, void *stream) {
    return gather_rows<double>(src, lds, idx, n, d, dst, ldd, stream);
}
int clane_gather_rows_bf16(const uint16_t *src, int64_t lds, const int32_t *idx, int64_t n, int32_t d, uint16_t *dst,
                           int64_t ldd, void *stream) {
    return gather_rows<bf16_t>(reinterpret_cast<const bf16_t *>(src), lds, idx, n, d,
                               reinterpret_cast<bf16_t *>(dst), ldd, stream);
}

int clane_pair_cosine_f32(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t nrows, int32_t d,
                          float *out, double *ws, void *stream) {
    return pair_cosine<float>(A, lda, B, ldb, nrows, d, out, ws, stream);
}
int clane_pair_cosine_f64(const double *A, int64_t lda, const double *B, int64_t ldb, int64_t nrows, int32_t d,
                          double *out, double *ws, void *stream) {
    return pair_cosine<double>(A, lda, B, ldb, nrows, d, out, ws, stream);
}

#define CLANE_PAIR_TRAIN_WRAPPERS(SUF, CT, T, AT)                                                                      \
    int clane_pair_project_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *src,         \
                                 const int32_t *dst, int64_t B, const AT *W, AT *A, AT *Bm, void *stream) {           \
        return pair_project<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, src, dst, B, W, A, Bm,         \
                                   stream);                                                                           \
    }                                                                                                                 \
    int clane_pair_grad_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *src,            \
                              const int32_t *dst, int64_t B, const AT *A, const AT *Bm, const AT *g,                  \
                              const double *stats, AT *ws, AT *dW, void *stream) {                                    \
        return pair_grad<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, src, dst, B, A, Bm, g, stats, ws, \
                                dW, stream);                                                                          \
    }
CLANE_PAIR_TRAIN_WRAPPERS(f32, float, float, float)
CLANE_PAIR_TRAIN_WRAPPERS(f64, double, double, double)
CLANE_PAIR_TRAIN_WRAPPERS(bf16, uint16_t, bf16_t, float)
#undef CLANE_PAIR_TRAIN_WRAPPERS
#define CLANE_PAIR_LOSS_WRAPPERS(SUF, AT)                                                                              \
    int clane_pair_loss_##SUF(const AT *A, const AT *Bm, int64_t B, int32_t d, const uint8_t *linked, const AT *u,    \
                              AT *g, uint8_t *mask, double *ws, double *stats, void *stream) {                        \
        return pair_loss<AT>(A, Bm, B, d, linked, u, g, mask, ws, stats, stream);                                     \
    }                                                                                                                 \
    int clane_adam_step_##SUF(AT *W, AT *m, AT *v, const AT *dW, int64_t n, double lr, const double *stats,           \
                              double *state, void *stream) {                                                          \
        return adam_step<AT>(W, m, v, dW, n, lr, stats, state, stream);                                               \
    }
CLANE_PAIR_LOSS_WRAPPERS(f32, float)
CLANE_PAIR_LOSS_WRAPPERS(f64, double)
#undef CLANE_PAIR_LOSS_WRAPPERS
int64_t clane_pair_grad_ws_len(int64_t B, int32_t d) { return pair_grad_chunks(B) * 2 * int64_t(d) * d; }
int clane_pair_labels(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, const int32_t *src,
                      const int32_t *dst, int64_t B, uint8_t *linked, void *stream) {
    REQUIRE(nrows >= 0 && B >= 0, "pair_labels: bad shape nrows=%lld B=%lld", (long long)nrows, (long long)B);
    if (B == 0) return CLANE_OK;
    REQUIRE(rowptr && colidx && src && dst && linked, "pair_labels: null pointer");
    pair_labels_kernel<<<grid_for_waves(ceil_div(B, kWave)), kBlock, 0, (hipStream_t)stream>>>(rowptr, colidx, nrows,
                                                                                              src, dst, B, linked);
    return check_launch("pair_labels");
}

#define CLANE_LINK_WRAPPERS(SUF, CT, T, AT)                                                                            \
    int clane_rank_scores_##SUF(const CT *S, int64_t lds, const CT *N, int64_t ldn, int64_t table_rows, int32_t d,    \
                                const int32_t *q_rows, int64_t Q, int32_t mode, const double *sums2, const AT *sq,    \
                                const int32_t *label, const int64_t *excl_rowptr, const int32_t *excl_colidx,         \
                                int32_t exclude_self, int32_t k, int32_t n_slabs, AT *cand_score, int32_t *cand_id,   \
                                void *stream) {                                                                       \
        return rank_scores<T, AT>(reinterpret_cast<const T *>(S), lds, reinterpret_cast<const T *>(N), ldn,           \
                                  table_rows, d, q_rows, Q, mode, sums2, sq, label, excl_rowptr, excl_colidx,         \
                                  exclude_self, k, n_slabs, cand_score, cand_id, stream);                             \
    }                                                                                                                 \
    int clane_rank_count_##SUF(const CT *S, int64_t lds, const CT *N, int64_t ldn, int64_t table_rows, int32_t d,     \
                               const int32_t *q_rows, const int32_t *t_rows, int64_t B, int32_t mode,                 \
                               const double *sums2, const AT *sq, const int32_t *label, const int64_t *excl_rowptr,   \
                               const int32_t *excl_colidx, int32_t exclude_self, int32_t n_slabs, AT *target_score,   \
                               int32_t *counts, void *stream) {                                                       \
        return rank_count<T, AT>(reinterpret_cast<const T *>(S), lds, reinterpret_cast<const T *>(N), ldn,            \
                                 table_rows, d, q_rows, t_rows, B, mode, sums2, sq, label, excl_rowptr, excl_colidx,  \
                                 exclude_self, n_slabs, target_score, counts, stream);                                \
    }                                                                                                                 \
    int clane_pair_score_##SUF(const CT *S, int64_t lds, const CT *N, int64_t ldn, int64_t table_rows, int32_t d,     \
                               const int32_t *src, const int32_t *dst, int64_t B, int32_t mode, const double *sums2,  \
                               const AT *sq, AT *out, void *stream) {                                                 \
        return pair_score<T>(reinterpret_cast<const T *>(S), lds, reinterpret_cast<const T *>(N), ldn, table_rows, d, \
                             src, dst, B, mode, sums2, sq, out, stream);                                              \
    }
CLANE_LINK_WRAPPERS(f32, float, float, float)
CLANE_LINK_WRAPPERS(f64, double, double, double)
CLANE_LINK_WRAPPERS(bf16, uint16_t, bf16_t, float)
#undef CLANE_LINK_WRAPPERS
int clane_rank_merge_f32(const float *cand_score, const int32_t *cand_id, int64_t Q, int32_t n_slabs, int32_t k,
                         float *out_score, int32_t *out_id, void *stream) {
    return rank_merge<float>(cand_score, cand_id, Q, n_slabs, k, out_score, out_id, stream);
}
int clane_rank_merge_f64(const double *cand_score, const int32_t *cand_id, int64_t Q, int32_t n_slabs, int32_t k,
                         double *out_score, int32_t *out_id, void *stream) {
    return rank_merge<double>(cand_score, cand_id, Q, n_slabs, k, out_score, out_id, stream);
}

#define CLANE_EMBED_WRAPPERS(SUF, CT, T, AT, GT)                                                                        \
    int clane_embed_rows_##SUF(const int64_t *rowptr, const int32_t *colidx, int64_t m, const CT *X_new, int64_t ldx,   \
                               const CT *Z, int64_t table_rows, int64_t ldz, int32_t d, int32_t mode,                   \
                               const double *sums2, const AT *sq, const AT *S, int64_t lds, GT gamma,                   \
                               int32_t tolerence, int32_t max_rounds, int32_t flags, CT *Z_out, int64_t ldo,            \
                               int32_t *rounds, AT *delta, AT *P_out, void *stream) {                                   \
        return embed_rows<T, GT>(rowptr, colidx, m, reinterpret_cast<const T *>(X_new), ldx,                            \
                                 reinterpret_cast<const T *>(Z), table_rows, ldz, d, mode, sums2, sq, S, lds, gamma,    \
                                 tolerence, max_rounds, flags, reinterpret_cast<T *>(Z_out), ldo, rounds, delta, P_out, \
                                 stream);                                                                               \
    }
CLANE_EMBED_WRAPPERS(f32, float, float, float, float)
CLANE_EMBED_WRAPPERS(f64, double, double, double, double)
CLANE_EMBED_WRAPPERS(bf16, uint16_t, bf16_t, float, float)
#undef CLANE_EMBED_WRAPPERS

#define CLANE_PROBE_WRAPPERS(SUF, CT, T, AT)                                                                           \
    int clane_probe_forward_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,        \
                                  const int32_t *y, int64_t n, const uint8_t *split, int64_t ld_split, const AT *W,    \
                                  const AT *bias, int32_t F, int32_t C, int32_t flags, AT *G, double *loss_ws,         \
                                  double *loss, int32_t *pred, int64_t ld_pred, void *stream) {                        \
        return probe_forward<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, rows, y, n, split, ld_split,   \
                                    W, bias, F, C, flags, G, loss_ws, loss, pred, ld_pred, stream);                    \
    }                                                                                                                  \
    int clane_probe_forward_ovr_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,    \
                                      const uint64_t *ymask, int64_t n, const uint8_t *split, int64_t ld_split,        \
                                      const AT *W, const AT *bias, const int8_t *col_state, int32_t F, int32_t C,      \
                                      int32_t max_labels, int32_t flags, AT *G, double *loss_ws, double *loss,         \
                                      uint64_t *pred, int64_t ld_pred, void *stream) {                                 \
        return probe_forward_ovr<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, rows, ymask, n, split,     \
                                        ld_split, W, bias, col_state, F, C, max_labels, flags, G, loss_ws, loss, pred, \
                                        ld_pred, stream);                                                              \
    }                                                                                                                  \
    int clane_probe_grad_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,           \
                               int64_t n, const AT *G, int32_t K, AT *ws, AT *dW, AT *db, void *stream) {              \
        return probe_grad<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, rows, n, G, K, ws, dW, db,        \
                                 stream);                                                                              \
    }                                                                                                                  \
    int clane_probe_predict_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,        \
                                  int64_t n, const AT *W, const AT *bias, const int8_t *col_state, int32_t F,          \
                                  int32_t C, int32_t top_m, int32_t flags, int32_t *top_class, AT *top_prob,           \
                                  AT *proba, void *stream) {                                                           \
        return probe_predict<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, rows, n, W, bias, col_state,   \
                                    F, C, top_m, flags, top_class, top_prob, proba, stream);                           \
    }
CLANE_PROBE_WRAPPERS(f32, float, float, float)
CLANE_PROBE_WRAPPERS(f64, double, double, double)
CLANE_PROBE_WRAPPERS(bf16, uint16_t, bf16_t, float)
#undef CLANE_PROBE_WRAPPERS
int64_t clane_probe_loss_ws_len(int64_t n, int32_t F) { return probe_row_tiles(n) * (F > 0 ? F : 0); }
int64_t clane_probe_grad_ws_len(int64_t n, int32_t K, int32_t d) {
    return probe_grad_chunks(n) * (K > 0 ? K : 0) * (int64_t(d > 0 ? d : 0) + 1);
}

#define CLANE_MIXTURE_WRAPPERS(SUF, CT, T, AT)                                                                         \
    int clane_mixture_estep_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,        \
                                  int64_t n, const AT *mean, const AT *Wm, const AT *cst, int32_t R, int32_t K,        \
                                  int32_t flags, AT *resp, double *ll_ws, double *ll, int32_t *assign,                 \
                                  int64_t ld_assign, void *stream) {                                                   \
        return mixture_estep<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, rows, n, mean, Wm, cst, R, K,  \
                                    flags, resp, ll_ws, ll, assign, ld_assign, stream);                                \
    }                                                                                                                  \
    int clane_mixture_mstep_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,        \
                                  int64_t n, const AT *mean, const AT *resp, int32_t K, AT *ws, AT *S, AT *nk,         \
                                  void *stream) {                                                                      \
        return mixture_mstep<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, rows, n, mean, resp, K, ws, S, \
                                    nk, stream);                                                                       \
    }
CLANE_MIXTURE_WRAPPERS(f32, float, float, float)
CLANE_MIXTURE_WRAPPERS(f64, double, double, double)
CLANE_MIXTURE_WRAPPERS(bf16, uint16_t, bf16_t, float)
#undef CLANE_MIXTURE_WRAPPERS
int64_t clane_mixture_ll_ws_len(int64_t n, int32_t R) { return probe_row_tiles(n) * (R > 0 ? R : 0); }
int64_t clane_mixture_mstep_ws_len(int64_t n, int32_t K, int32_t d) {
    return probe_grad_chunks(n) * (K > 0 ? K : 0) * (2 * int64_t(d > 0 ? d : 0) + 1);
}

#define CLANE_KMEANS_WRAPPERS(SUF, CT, T, AT)                                                                          \
    int clane_kmeans_assign_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,        \
                                  int64_t n, const AT *centres, const AT *csq, int32_t R, int32_t K, int32_t *assign,  \
                                  int64_t ld_assign, AT *best, int64_t ld_best, void *stream) {                        \
        return kmeans_assign<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, rows, n, centres, csq, R, K,   \
                                    assign, ld_assign, best, ld_best, stream);                                         \
    }                                                                                                                  \
    int clane_kmeans_update_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order,       \
                                  const int64_t *seg, int64_t n, int32_t R, int32_t K, const AT *centres_old, AT *ws,  \
                                  AT *centres_new, AT *csq_new, void *stream) {                                        \
        return kmeans_update<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, order, seg, n, R, K,           \
                                    centres_old, ws, centres_new, csq_new, stream);                                    \
    }
CLANE_KMEANS_WRAPPERS(f32, float, float, float)
CLANE_KMEANS_WRAPPERS(f64, double, double, double)
CLANE_KMEANS_WRAPPERS(bf16, uint16_t, bf16_t, float)
#undef CLANE_KMEANS_WRAPPERS
int64_t clane_kmeans_update_ws_len(int64_t n, int32_t R, int32_t K, int32_t d) {
    (void)K;                                     /* two chunk sums per window of the sorted list, whatever K */
    return 2 * kmeans_windows(n, R) * int64_t(d > 0 ? d : 0);
}

#define CLANE_PCA_WRAPPERS(SUF, CT, T, AT)                                                                             \
    int clane_column_sums_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,          \
                                int64_t n, int32_t flags, double *ws, double *sums, void *stream) {                    \
        return column_sums<T>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, rows, n, flags, ws, sums, stream);   \
    }                                                                                                                  \
    int clane_gram_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,      \
                         const AT *mu, int32_t flags, AT *ws, AT *G, void *stream) {                                   \
        return gram<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, rows, n, mu, flags, ws, G, stream);     \
    }                                                                                                                  \
    int clane_project_affine_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,       \
                                   int64_t n, const AT *mu, const AT *W, int32_t m, CT *Y, int64_t ldy,                \
                                   void *stream) {                                                                     \
        return project_affine<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, rows, n, mu, W, m,            \
                                     reinterpret_cast<T *>(Y), ldy, stream);                                           \
    }
CLANE_PCA_WRAPPERS(f32, float, float, float)
CLANE_PCA_WRAPPERS(f64, double, double, double)
CLANE_PCA_WRAPPERS(bf16, uint16_t, bf16_t, float)
#undef CLANE_PCA_WRAPPERS
int64_t clane_column_sums_ws_len(int64_t n, int32_t d) { return (pca_chunks(n) > 0 ? pca_chunks(n) : 1) * int64_t(d > 0 ? d : 0); }
int64_t clane_gram_ws_len(int64_t n, int32_t d) {
    return (pca_chunks(n) > 0 ? pca_chunks(n) : 1) * int64_t(d > 0 ? d : 0) * int64_t(d > 0 ? d : 0);
}

int clane_csr_spmm_segment(void) { return kCsrSegment; }
int64_t clane_csr_spmm_ws_len(int64_t n_rows, int64_t nnz, int32_t l) {
    (void)n_rows;                                /* a row of more than a segment is cut into fewer than 2 len / segment */
    const int64_t items = csr_max_items(nnz > 0 ? nnz : 0);
    return (items > 0 ? items : 1) * int64_t(l > 0 ? l : 0);
}
int clane_csr_spmm_f32(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows, int64_t nnz,
                       const float *B, int64_t b_rows, int64_t ldb, int32_t l, const float *a, const float *s,
                       const int32_t *long_rows, const int64_t *seg_ptr, const int32_t *item_long, int64_t n_long,
                       int64_t n_items, float *ws, int64_t ws_len, float *out, int64_t ldo, void *stream) {
    return csr_spmm(rowptr, col, val, n_rows, nnz, B, b_rows, ldb, l, a, s, long_rows, seg_ptr, item_long, n_long, n_items,
                    ws, ws_len, out, ldo, stream);
}
int clane_csr_row_sums_f32(const int64_t *rowptr, const float *val, int64_t n_rows, int64_t nnz, const int32_t *long_rows,
                           const int64_t *seg_ptr, const int32_t *item_long, int64_t n_long, int64_t n_items, double *ws,
                           int64_t ws_len, double *sums, void *stream) {
    return csr_row_sums(rowptr, val, n_rows, nnz, long_rows, seg_ptr, item_long, n_long, n_items, ws, ws_len, sums, stream);
}

int clane_tsne_sqdist_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                          const float *mu, float *sq, float *D, void *stream) {
    return tsne_sqdist<float>(Z, table_rows, d, ldz, rows, n, mu, sq, D, stream);
}
int clane_tsne_sqdist_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                           const float *mu, float *sq, float *D, void *stream) {
    return tsne_sqdist<bf16_t>(reinterpret_cast<const bf16_t *>(Z), table_rows, d, ldz, rows, n, mu, sq, D, stream);
}
int clane_tsne_affinities_f32(float *D, int64_t n, float perplexity, float *beta, void *stream) {
    REQUIRE(n >= 2 && n <= kTsneMaxPoints, "tsne_affinities: n must be in [2, %d], got %lld", kTsneMaxPoints, (long long)n);
    REQUIRE(perplexity > 0.f && perplexity < float(n), "tsne_affinities: perplexity %g is not in (0, n = %lld)",
            double(perplexity), (long long)n);
    REQUIRE(D && beta, "tsne_affinities: null pointer");
    tsne_affinities_kernel<<<unsigned(n), kBlock, 0, (hipStream_t)stream>>>(D, n, perplexity, beta);
    return check_launch("tsne_affinities");
}
int64_t clane_tsne_symmetrize_ws_len(int64_t n) { return tsne_sym_tiles(n) * (tsne_sym_tiles(n) + 1) / 2; }
int clane_tsne_symmetrize_f32(float *P, int64_t n, double *partials, void *stream) {
    REQUIRE(n >= 1 && n <= kTsneMaxPoints, "tsne_symmetrize: n must be in [1, %d], got %lld", kTsneMaxPoints, (long long)n);
    REQUIRE(P && partials, "tsne_symmetrize: null pointer");
    const int64_t nt = tsne_sym_tiles(n);
    tsne_symmetrize_kernel<<<unsigned(nt * (nt + 1) / 2), kBlock, 0, (hipStream_t)stream>>>(P, n, int(nt), partials);
    return check_launch("tsne_symmetrize");
}
int clane_tsne_forces_f32(const float *P, const float *Y, int64_t n, int32_t flags, float *F, void *stream) {
    static_assert(kTsneForcesKL == CLANE_TSNE_FORCES_KL && kTsneForcesCached == CLANE_TSNE_FORCES_CACHED,
                  "header and kernel disagree");
    REQUIRE(n >= 1 && n <= kTsneMaxPoints, "tsne_forces: n must be in [1, %d], got %lld", kTsneMaxPoints, (long long)n);
    REQUIRE((flags & ~(CLANE_TSNE_FORCES_KL | CLANE_TSNE_FORCES_CACHED)) == 0, "tsne_forces: unknown flags %d", flags);
    REQUIRE(P && Y && F, "tsne_forces: null pointer");
    REQUIRE((const void *)Y != (const void *)F, "tsne_forces: Y must not be the array being written");
    const unsigned grid = unsigned(ceil_div(n, int64_t(kTsneRowsPerBlock)));
    const int want_l = flags & CLANE_TSNE_FORCES_KL;
    const bool vec = aligned16(P) && n % 4 == 0, nt = !(flags & CLANE_TSNE_FORCES_CACHED);
    if (vec && nt) tsne_forces_kernel<true, true><<<grid, kBlock, 0, (hipStream_t)stream>>>(P, Y, n, want_l, F);
    else if (vec) tsne_forces_kernel<true, false><<<grid, kBlock, 0, (hipStream_t)stream>>>(P, Y, n, want_l, F);
    else if (nt) tsne_forces_kernel<false, true><<<grid, kBlock, 0, (hipStream_t)stream>>>(P, Y, n, want_l, F);
    else tsne_forces_kernel<false, false><<<grid, kBlock, 0, (hipStream_t)stream>>>(P, Y, n, want_l, F);
    return check_launch("tsne_forces");
}
int clane_tsne_step_f32(const float *F, const float *Y, int64_t n, double alpha, double momentum, double lr, double plogp,
                        float *V, float *G, float *Y_next, double *stats, void *stream) {
    REQUIRE(n >= 1 && n <= kTsneNnMaxPoints, "tsne_step: n must be in [1, %d], got %lld", kTsneNnMaxPoints, (long long)n);
    REQUIRE(F && Y && V && G && Y_next && stats, "tsne_step: null pointer");
    REQUIRE(Y != Y_next, "tsne_step: Y must not be the array being written");
    tsne_step_kernel<<<1, kTsneStepBlock, 0, (hipStream_t)stream>>>(F, Y, n, alpha, momentum, lr, plogp, V, G, Y_next,
                                                                    stats);
    return check_launch("tsne_step");
}

int clane_knn_sqdist_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                         const float *mu, float *sq, int32_t k, int32_t n_slabs, float *cand_sqdist, int32_t *cand_ids,
                         float *sqdist, int32_t *ids, void *stream) {
    return knn_sqdist<float>(Z, table_rows, d, ldz, rows, n, mu, sq, k, n_slabs, cand_sqdist, cand_ids, sqdist, ids, stream);
}
int clane_knn_sqdist_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                          const float *mu, float *sq, int32_t k, int32_t n_slabs, float *cand_sqdist, int32_t *cand_ids,
                          float *sqdist, int32_t *ids, void *stream) {
    return knn_sqdist<bf16_t>(reinterpret_cast<const bf16_t *>(Z), table_rows, d, ldz, rows, n, mu, sq, k, n_slabs,
                              cand_sqdist, cand_ids, sqdist, ids, stream);
}
int clane_tsne_nn_affinities_f32(const float *sqdist, const int32_t *ids, int64_t n, int32_t k, float perplexity, float *p,
                                 float *beta, void *stream) {
    REQUIRE(n >= 2 && n <= kTsneNnMaxPoints, "tsne_nn_affinities: n must be in [2, %d], got %lld", kTsneNnMaxPoints,
            (long long)n);
    REQUIRE(k >= 1 && k <= CLANE_KNN_MAX_K, "tsne_nn_affinities: k must be in [1, %d], got %d", CLANE_KNN_MAX_K, k);
    REQUIRE(perplexity > 0.f && perplexity < float(k), "tsne_nn_affinities: perplexity %g is not in (0, k = %d)",
            double(perplexity), k);
    REQUIRE(sqdist && ids && p && beta, "tsne_nn_affinities: null pointer");
    tsne_nn_affinities_kernel<<<unsigned(ceil_div(n, int64_t(kNnRowsPerBlock))), kBlock, 0, (hipStream_t)stream>>>(
        sqdist, ids, n, k, perplexity, p, beta);
    return check_launch("tsne_nn_affinities");
}
int clane_tsne_nn_plogp_f32(const int64_t *rowptr, const float *val, int64_t n, int64_t nnz, double *row_plogp,
                            void *stream) {
    REQUIRE(n >= 1 && n <= kTsneNnMaxPoints && nnz >= 0, "tsne_nn_plogp: bad shape n=%lld nnz=%lld", (long long)n,
            (long long)nnz);
    REQUIRE(rowptr && row_plogp && (val || nnz == 0), "tsne_nn_plogp: null pointer");
    tsne_nn_plogp_kernel<<<unsigned(ceil_div(n, int64_t(kNnRowsPerBlock))), kBlock, 0, (hipStream_t)stream>>>(
        rowptr, val, n, nnz, row_plogp);
    return check_launch("tsne_nn_plogp");
}
int clane_tsne_nn_attract_f32(const int64_t *rowptr, const int32_t *cols, const float *val, const float *Y, int64_t n,
                              int64_t nnz, int32_t flags, float *F, void *stream) {
    REQUIRE(n >= 1 && n <= kTsneNnMaxPoints && nnz >= 0, "tsne_nn_attract: bad shape n=%lld nnz=%lld", (long long)n,
            (long long)nnz);
    REQUIRE((flags & ~CLANE_TSNE_FORCES_KL) == 0, "tsne_nn_attract: unknown flags %d", flags);
    REQUIRE(rowptr && Y && F && ((cols && val) || nnz == 0), "tsne_nn_attract: null pointer");
    REQUIRE((const void *)Y != (const void *)F, "tsne_nn_attract: Y must not be the array being written");
    tsne_nn_attract_kernel<<<unsigned(ceil_div(n, int64_t(kNnRowsPerBlock))), kBlock, 0, (hipStream_t)stream>>>(
        rowptr, cols, val, Y, n, nnz, flags & CLANE_TSNE_FORCES_KL, F);
    return check_launch("tsne_nn_attract");
}
int clane_tsne_repulse_f32(const float *Y, int64_t n, float *F, void *stream) {
    REQUIRE(n >= 1 && n <= kTsneNnMaxPoints, "tsne_repulse: n must be in [1, %d], got %lld", kTsneNnMaxPoints, (long long)n);
    REQUIRE(Y && F, "tsne_repulse: null pointer");
    REQUIRE((const void *)Y != (const void *)F, "tsne_repulse: Y must not be the array being written");
    tsne_repulse_kernel<<<unsigned(ceil_div(n, int64_t(kRepulseRowsPerBlock))), kBlock, 0, (hipStream_t)stream>>>(Y, n, F);
    return check_launch("tsne_repulse");
}

#define CLANE_SILHOUETTE_WRAPPERS(SUF, CT, T, AT)                                                                      \
    int clane_silhouette_norms_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order,    \
                                     int64_t n, const AT *mu, int32_t metric, AT *nrm, void *stream) {                 \
        return silhouette_norms<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, order, n, mu, metric, nrm,  \
                                       stream);                                                                        \
    }                                                                                                                  \
    int clane_silhouette_sums_##SUF(const CT *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order,     \
                                    int64_t n, const int64_t *seg, int32_t K, const AT *mu, const AT *nrm,             \
                                    int32_t metric, int64_t p0, int64_t p1, double *S, void *stream) {                 \
        return silhouette_sums<T, AT>(reinterpret_cast<const T *>(Z), table_rows, d, ldz, order, n, seg, K, mu, nrm,   \
                                      metric, p0, p1, S, stream);                                                      \
    }
CLANE_SILHOUETTE_WRAPPERS(f32, float, float, float)
CLANE_SILHOUETTE_WRAPPERS(f64, double, double, double)
CLANE_SILHOUETTE_WRAPPERS(bf16, uint16_t, bf16_t, float)
#undef CLANE_SILHOUETTE_WRAPPERS

}  // extern "C"
