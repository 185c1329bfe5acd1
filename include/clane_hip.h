/*
 * clane_hip.h -- C ABI of libclane_hip.so: CLANE's iterative embedding loop on MI355X (gfx950).
 *
 * The reference (helloybz/CLANE @ v2) is pure Python on PyTorch-CPU and has no FFI.  This
 * header is the boundary a maintainer would bind (ctypes) underneath
 * the reference's own Python surface.  Each entry point names the reference code it
 * replaces (paths are relative to the reference checkout).
 *
 * Conventions
 *  - Every function returns 0 on success, <0 on error (CLANE_ERR_*); the text of the last
 *    error on the calling thread is clane_last_error().
 *  - All array arguments are DEVICE pointers to caller-owned memory.  The library never
 *    allocates, frees or retains them, keeps no global mutable state, and never
 *    synchronises: work is enqueued on `stream` (a hipStream_t, NULL = default stream).
 *  - Matrices are row-major with a leading dimension in ELEMENTS (ldz, ldx, ldo >= d).
 *    FAST PATH: when every matrix base pointer is 16-byte aligned and every leading
 *    dimension is a multiple of 16/sizeof(T), rows are moved with 16-byte accesses and the
 *    columns [d, roundup(d, 16/sizeof(T))) of each row are read AND written: they must be
 *    zero on entry (they stay zero).  Otherwise a 1-element-per-lane path is taken.
 *  - CSR: rowptr int64 [nrows+1], offsets into colidx / P; colidx int32, GLOBAL column ids
 *    (rows of the full Z), sorted and unique within a row (reference: graph.py:104-110,
 *    sparse_coo_tensor(...).coalesce(): row = source, col = destination).
 *  - `row0` is the global row id of local row 0 (row-partitioned multi-GPU runs hand each
 *    rank a contiguous block of rows; on one GPU row0 = 0).
 *  - Suffix _f32: T = float,  accumulate float,  P/scores float.
 *    Suffix _f64: T = double, accumulate double, P/scores double (C.npy may be float64 and
 *                 the reference keeps that dtype: graph.py:51).
 *    Suffix _bf16: T = bf16 storage for Z/X, accumulate float, P/scores float.
 *  - Reductions that feed control flow (the L1 delta) are deterministic: one partial per workgroup /
 *    listed row, summed in index order, no float atomics -- two launches give bitwise equal results.
 */
#ifndef CLANE_HIP_H_
#define CLANE_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLANE_ABI_VERSION 5 /* 2: + clane_build_info, clane_xcc_ids, clane_check_csr, clane_spmm_update_class_*, clane_edge_score_class_*
                             * 3: clane_l1_distance_* takes `sq_a` (the rows' squared norms from the outer-delta pass: free),
                             *    clane_device_alloc_contiguous; every clane_spmm_update* took `sq_out` (the same norms out of K3)
                             * 4: `sq_out` is gone again: it cost every sweep 1.1-1.4 % to save one 0.34 ms pass per build_P, and a
                             *    propagate runs >= 11 sweeps per build_P (profiles/r04_fused_norms_ab.jsonl);
                             *    clane_spmm_update_class_* takes `flags` (CLANE_SPMM_TABLE_BEYOND_CACHE, also a flag of clane_spmm_update_*)
                             * 5: + clane_project_rows_*, clane_edge_score_pair_*, clane_edge_score_class_pair_* (bilinear
                             *    similarity: AsymmertricSimilarity's P without a per-edge projection)
                             * 5, additions that change no existing call (the number stays: every v5 caller keeps working):
                             *    + clane_pair_project_*, clane_pair_loss_*, clane_pair_grad_*, clane_pair_grad_ws_len,
                             *    clane_adam_step_*, clane_pair_labels (training the bilinear similarity on the device)
                             *    + clane_rank_scores_*, clane_rank_merge_*, clane_pair_score_* (link prediction: top-k
                             *    candidates of query rows against the whole table, scores of explicit pairs)
                             *    + clane_rank_count_* (held-out link evaluation: a pair's score and how many eligible rows of
                             *    the whole table score above it or tie with it -- the filtered rank without a score matrix)
                             *    + clane_probe_forward_*, clane_probe_grad_*, clane_probe_loss_ws_len,
                             *    clane_probe_grad_ws_len (node classification: F stacked soft-max regressions on rows of the
                             *    table, loss / gradient / arg-max fused into the logits' contraction)
                             *    + clane_kmeans_assign_*, clane_kmeans_update_*, clane_kmeans_update_ws_len (node clustering:
                             *    batched k-means on rows of the table, the arg-min fused into the distances' contraction)
                             *    + clane_probe_forward_ovr_* (multi-label node classification: F stacked one-vs-rest
                             *    regressions, sigmoid loss / gradient and the top-k label masks fused into the logits'
                             *    contraction; workspaces and clane_probe_grad_* as for the soft-max probe)
                             *    + clane_embed_rows_* (new vertices embedded against the finished table: the per-row fixed
                             *    point of build_P + update on frozen Z, one launch, every row stopping on its own)
                             *    + clane_column_sums_*, clane_gram_*, clane_project_affine_*, clane_column_sums_ws_len,
                             *    clane_gram_ws_len (content reduction: the device passes of a PCA on rows of a table --
                             *    deterministic column sums, the centred Gram on the matrix cores, an affine projection)
                             *    + clane_spmm_update_owned_f32 (class rows summed in LDS by row-owning workgroups: no slab,
                             *    no combine pass; embedder.py:90-92)
                             *    + clane_csr_spmm_f32, clane_csr_row_sums_f32, clane_csr_spmm_segment, clane_csr_spmm_ws_len
                             *    (sparse content: CSR rows times a dense matrix with a rank-one epilogue and the rows'
                             *    value sums -- the products of a randomized PCA on a bag of words)
                             *    + clane_spmm_update_tiles_f32, clane_spmm_update_class_tiles_f32,
                             *    clane_spmm_update_owned_tiles_f32 (every column tile of a K3 pass in ONE launch, bit for
                             *    bit the per-tile calls) and the flag CLANE_OWNED_EPILOGUE_AHEAD of the owned calls
                             *    + clane_tsne_sqdist_*, clane_tsne_affinities_f32, clane_tsne_symmetrize_f32,
                             *    clane_tsne_symmetrize_ws_len, clane_tsne_forces_f32, clane_tsne_step_f32 (2-D layout: exact
                             *    t-SNE of rows of the table -- all-pairs distances on the matrix cores, the perplexity
                             *    search, the joint probabilities and the two kernels of an iteration)
                             *    + clane_silhouette_norms_*, clane_silhouette_sums_* (silhouette of a partition of rows of
                             *    the table: the n x K sums of distances on the matrix cores, never the n x n distances)
                             *    + clane_knn_sqdist_*, clane_tsne_nn_affinities_f32, clane_tsne_nn_plogp_f32,
                             *    clane_tsne_nn_attract_f32, clane_tsne_repulse_f32 (neighbour-sparse 2-D layout: the k
                             *    nearest listed rows of every listed row with the selection fused into the distances, P
                             *    on those neighbours only, the repulsion exact; clane_tsne_step_f32 takes up to
                             *    CLANE_TSNE_NN_MAX_POINTS points)
                             *    + clane_probe_predict_* (applying fitted probes: class probabilities and the top-m classes
                             *    of rows of the table under F stacked soft-max or one-vs-rest models, fused into the logits'
                             *    contraction)
                             *    + clane_mixture_estep_*, clane_mixture_mstep_*, clane_mixture_ll_ws_len,
                             *    clane_mixture_mstep_ws_len (soft clusters: R stacked diagonal Gaussian mixtures on centred
                             *    rows of the table -- responsibilities, log-likelihood and arg-max fused into the logits'
                             *    contraction, the sufficient statistics one contraction over the rows)
                             *    + clane_row_weight_*, clane_spmm_update_rw_f32, clane_spmm_update_class_rw_f32,
                             *    clane_spmm_update_owned_rw_f32 and their *_tiles_rw_f32 forms (K3 with one weight per row
                             *    instead of one per edge where every row of P is uniform: bit for bit the per-edge calls) */

#define CLANE_OK 0
#define CLANE_ERR_INVALID_ARGUMENT (-1)
#define CLANE_ERR_LAUNCH (-2)

/* score modes of clane_edge_score_* */
#define CLANE_SCORE_REFERENCE 0 /* dot / (||Z[src_all]||_F * ||Z[dst_all]||_F)  -- what similarity.py:37 computes */
#define CLANE_SCORE_PER_EDGE 1  /* dot / (||z_src|| * ||z_dst||)                 -- what its docstring describes  */
#define CLANE_SCORE_RAW_DOT 2   /* dot                                           -- stage test                     */

/* flags of clane_edge_score_* */
#define CLANE_SCORE_FUSE_SOFTMAX 1
/* clane_edge_score_class_* with CLANE_SCORE_FUSE_SOFTMAX: n (1..255) workgroups share the final rescale pass of each
 * listed row -- for graphs with rows of millions of edges; results do not depend on n; 0 means 1 */
#define CLANE_SCORE_ROW_PARTS(n) (((n) & 0xff) << 8)

/* flags of clane_spmm_update_* and clane_spmm_update_class_* */
#define CLANE_SPMM_SINKS_UNTOUCHED 1
/* A hint, never a change of results: the embedding table is far beyond the caches (the engine: more than twice the
 * 256 MiB Infinity Cache).  The instances with two fp32 rows per instruction (512-byte rows: column tiles / slices)
 * then keep 4 (row kernel) / 6 (class chunks) row loads in flight per wave instead of 8 and run 8 / 7 waves per SIMD
 * instead of 6 / 5 -- config 3 in two column tiles 3.79 -> 3.71 ms per sweep; a cache-resident table (config 2) loses
 * 18 % with it.  The class chunks with four bf16 rows per instruction keep 4 (config 4: 7.10 -> 6.99 ms).  With the
 * hint every finished row of z_new is also stored non-temporal (config 3 another 0.8 %; on a cache-resident table the
 * next sweep gathers what this one wrote and non-temporal stores cost 4 %). */
#define CLANE_SPMM_TABLE_BEYOND_CACHE 2

/* Optional further destinations of the rows a clane_spmm_update* call finishes: row r (relative to the call's
 * first row) is also stored at the places slot[row_ptr[r] .. row_ptr[r+1]); a place is (buffer << 28 | row) into
 * `bufs`, a DEVICE array of up to 8 matrix base addresses (leading dimension ld, element type of Z_new).
 * One buffer: the send buffer of the multi-GPU halo exchange gets packed by the kernel that produces a row
 * instead of by a separate gather pass.  Several: the other GPUs' tables mapped into this process (IPC) -- rows
 * go straight over xGMI.  aligned16: the caller vouches that every base is 16-byte aligned (the library cannot
 * look into device memory); 0 selects the scalar path.  NULL, or row_ptr == NULL: no mirror. */
typedef struct {
    const int64_t *row_ptr; /* [rows of the call + 1] */
    const int32_t *slot;
    void *const *bufs;
    int64_t ld;
    int32_t aligned16;
} clane_mirror_t;

int clane_abi_version(void);
const char *clane_last_error(void);
/* Compile-time tuning of this build as "KEY=value;..." (neighbour rows in flight per wave, waves and rows per
 * workgroup, non-temporal streams): measurements stored beside a benchmark (profiles/traffic.json) carry it, so a
 * number taken with another build is recognised as stale.  No reference counterpart. */
const char *clane_build_info(void);
/* Diagnostic: out[w] = the XCD (0..7, HW_REG_XCC_ID) that workgroup w of a launch of n_blocks workgroups of
 * block_threads threads ran on.  clane_spmm_update_class_* / clane_edge_score_class_* get their speed -- not their
 * results -- from workgroup w running on XCD (w + c) % 8 with c the same for the whole launch; the GPU test suite checks that with this call. */
int clane_xcc_ids(int32_t *out, int64_t n_blocks, int32_t block_threads, void *stream);
/* Validates on the device what every gather kernel below takes on trust -- call it once per graph before the first
 * sweep: rowptr[0..nrows] must be non-decreasing within [0, n_edges], every colidx[e] (e < n_edges) a row of a table of
 * table_rows rows.  *status (device int32, zeroed by the caller) gets bit 0 for a bad rowptr entry, bit 1 for a column
 * out of range; nothing else is touched.  (The reference cannot go wrong here: torch.sparse validates its indices,
 * graph.py:104-110.  A HIP kernel gathering through a bad index faults the GPU.) */
int clane_check_csr(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t n_edges, int64_t table_rows,
                    int32_t *status, void *stream);

/* Doubles written by clane_spmm_update_*(nrows) plus clane_spmm_update_long_*(n_long). */
int64_t clane_spmm_partials_len(int64_t nrows, int64_t n_long);
/* Doubles of scratch needed by clane_degree_weighted_sums_* / clane_pair_cosine_*. */
int64_t clane_reduce_ws_len(void);

/* ---- Device memory that another process can map.  Everything else in this library works on memory the caller
 * owns; these five exist because a halo table that other GPUs store into (clane_mirror_t with several buffers)
 * must be its own allocation (hipIpcGetMemHandle works on allocation bases) and must be opened with peer access
 * from the device that is current in the calling process.  No reference counterpart (one process upstream).
 *   clane_device_alloc / _free : hipMalloc / hipFree on the current device.
 *   clane_ipc_export(ptr, handle)  : handle = CLANE_IPC_HANDLE_BYTES bytes to hand to the other process.
 *   clane_ipc_open(handle, &ptr)   : map it (hipIpcMemLazyEnablePeerAccess); clane_ipc_close(ptr) unmaps. */
#define CLANE_IPC_HANDLE_BYTES 64
int clane_device_alloc(int64_t bytes, void **ptr);
/* The same with PHYSICALLY CONTIGUOUS backing (hipExtMallocWithFlags, hipDeviceMallocContiguous): for the big gather
 * tables -- a random row gather over a 2 GB table runs up to 7 % slower when the driver backs it with scattered pages
 * (profiles/r04_placement_probe_*.jsonl).  Fails (CLANE_ERR_LAUNCH) when no contiguous range is free: fall back to
 * clane_device_alloc.  Freed with clane_device_free. */
int clane_device_alloc_contiguous(int64_t bytes, void **ptr);
int clane_device_free(void *ptr);
int clane_ipc_export(void *ptr, void *handle64);
int clane_ipc_open(const void *handle64, void **ptr);
int clane_ipc_close(void *ptr);

/* ---- K0: sq[v] = sum_k Z[v,k]^2.  Replaces the two `pow(2).sum()` of similarity.py:37
 * (together with clane_degree_weighted_sums_*). */
int clane_row_sqnorm_f32(const float *Z, int64_t nrows, int32_t d, int64_t ldz, float *sq, void *stream);
int clane_row_sqnorm_f64(const double *Z, int64_t nrows, int32_t d, int64_t ldz, double *sq, void *stream);
int clane_row_sqnorm_bf16(const uint16_t *Z, int64_t nrows, int32_t d, int64_t ldz, float *sq, void *stream);

/* out2[0] = sum_v outdeg_v*sq_v, out2[1] = sum_v indeg_v*sq_v over the local rows, in double
 * (= ||Z[src_all]||_F^2 and ||Z[dst_all]||_F^2 of similarity.py:37 for the edges built at
 * graph.py:119-120).  outdeg_v = rowptr[v+1]-rowptr[v]; indeg is caller-provided [nrows].
 * ws: clane_reduce_ws_len() doubles.  Multi-GPU: all-reduce out2 (sum) afterwards. */
int clane_degree_weighted_sums_f32(const float *sq, const int64_t *rowptr, const int32_t *indeg, int64_t nrows,
                                   double *ws, double *out2, void *stream);
int clane_degree_weighted_sums_f64(const double *sq, const int64_t *rowptr, const int32_t *indeg, int64_t nrows,
                                   double *ws, double *out2, void *stream);

/* ---- K1: per-edge similarity score in CSR order.  Replaces the gather + similarity call
 * of graph.py:119-121 and CosineSimilarity.__call__ (similarity.py:26-37) without
 * materialising Z[edges].  Source row of local row i is Z[row0+i].
 *   mode REFERENCE: sums2 = the (all-reduced) pair from clane_degree_weighted_sums_*; sq unused.
 *   mode PER_EDGE : sq = squared norms of ALL rows of Z; sums2 unused.
 *   mode RAW_DOT  : both unused.
 * Rows with more than `long_threshold` edges (0 = never) are cut into per-wave slices by a
 * second launch over `long_rows` (local row ids, n_long of them; one 16-wave workgroup per row);
 * pass n_long = 0 to have every row walked by a single wave.
 * flags & CLANE_SCORE_FUSE_SOFTMAX: every row this call scores is soft-maxed by it as well (graph.py:122-123):
 * a row walked by one wave in registers or with a running max / sum, a listed row by its workgroup ({max, sum}
 * per wave combined through LDS in wave order).  No clane_segment_softmax_* call is needed afterwards. */
int clane_edge_score_f32(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0, const float *Z,
                         int64_t ldz, int32_t d, int32_t mode, const double *sums2, const float *sq, float *scores,
                         int32_t flags, int64_t long_threshold, const int32_t *long_rows, int64_t n_long, void *stream);
int clane_edge_score_f64(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0, const double *Z,
                         int64_t ldz, int32_t d, int32_t mode, const double *sums2, const double *sq, double *scores,
                         int32_t flags, int64_t long_threshold, const int32_t *long_rows, int64_t n_long, void *stream);
int clane_edge_score_bf16(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0,
                          const uint16_t *Z, int64_t ldz, int32_t d, int32_t mode, const double *sums2,
                          const float *sq, float *scores, int32_t flags, int64_t long_threshold,
                          const int32_t *long_rows, int64_t n_long, void *stream);

/* ---- K1b (column-split multi-GPU runs): scores holds RAW_DOT results summed over the GPUs (each GPU scored
 * its own columns); divide them by the denominators of `mode` exactly as clane_edge_score_* would have
 * (similarity.py:37).  sums2 / sq as for clane_edge_score_*, already summed over the GPUs.  RAW_DOT: no-op. */
int clane_edge_score_finalize_f32(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0,
                                  int32_t mode, const double *sums2, const float *sq, float *scores, void *stream);
int clane_edge_score_finalize_f64(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0,
                                  int32_t mode, const double *sums2, const double *sq, double *scores, void *stream);

/* ---- K2: in-place softmax of vals within each CSR row.  Replaces the per-row boolean-mask
 * loop of graph.py:122-123.  Rows with min_degree < deg <= max_degree (max_degree 0 = no upper
 * limit) are normalised by one wave each; the rows listed in `long_rows` (deg > min_degree) by one
 * 16-wave workgroup each.  Empty rows are skipped; max_degree <= min_degree (both > 0) disables the
 * one-wave pass.  Not needed after clane_edge_score_* with CLANE_SCORE_FUSE_SOFTMAX; used after
 * clane_edge_score_finalize_* and for plug-in scores. */
int clane_segment_softmax_f32(const int64_t *rowptr, int64_t nrows, float *vals, int64_t min_degree,
                              int64_t max_degree, const int32_t *long_rows, int64_t n_long, void *stream);
int clane_segment_softmax_f64(const int64_t *rowptr, int64_t nrows, double *vals, int64_t min_degree,
                              int64_t max_degree, const int32_t *long_rows, int64_t n_long, void *stream);

/* ---- K3: one Jacobi sweep over the local rows, fused with the L1 delta.  Replaces the
 * per-vertex loop embedder.py:84-92 and the reduction embedder.py:94:
 *     Z_new[i,:] = X[i,:] + gamma * sum_e P[e] * Z_old[colidx[e],:]     rowptr[i] <= e < rowptr[i+1]
 *     Z_new[i,:] = Z_old[row0+i,:]                                       if the row has no out-edge (embedder.py:88-89)
 *     delta_partials[b] = partial sums of |Z_new[i,:] - Z_old[row0+i,:]| (fixed order; reduce with clane_reduce_partials)
 * Z_new must not alias Z_old.
 *  clane_spmm_update_*      : one wave per row; rows with more than `long_threshold` edges (0 = never)
 *                             are skipped.  Writes clane_spmm_partials_len(nrows, 0) doubles.
 *                             flags & CLANE_SPMM_SINKS_UNTOUCHED: rows without out-edges are neither read
 *                             nor written -- the caller guarantees Z_new already equals Z_old there (they
 *                             never change, so two ping-pong buffers initialised alike stay alike).
 *  clane_spmm_update_long_* : the skipped rows, one workgroup of `waves_per_row` (4 or 16) waves per row,
 *                             each wave gathering a 64-aligned slice of the row, slices folded in wave
 *                             order; `long_rows` holds the local row ids (the caller bins rows by degree
 *                             once per graph: 4 waves suit rows of up to a few hundred edges, 16 the
 *                             hubs).  Writes n_long doubles.
 * Calls touch disjoint rows of Z_new and may run on different streams. */
int clane_spmm_update_f32(const int64_t *rowptr, const int32_t *colidx, const float *P, int64_t nrows, int64_t row0,
                          const float *Z_old, int64_t ldz, const float *X, int64_t ldx, float gamma, float *Z_new,
                          int64_t ldo, int32_t d, int64_t long_threshold, int32_t flags, const clane_mirror_t *mirror,
                          double *delta_partials, void *stream);
int clane_spmm_update_f64(const int64_t *rowptr, const int32_t *colidx, const double *P, int64_t nrows, int64_t row0,
                          const double *Z_old, int64_t ldz, const double *X, int64_t ldx, double gamma, double *Z_new,
                          int64_t ldo, int32_t d, int64_t long_threshold, int32_t flags, const clane_mirror_t *mirror,
                          double *delta_partials, void *stream);
int clane_spmm_update_bf16(const int64_t *rowptr, const int32_t *colidx, const float *P, int64_t nrows, int64_t row0,
                           const uint16_t *Z_old, int64_t ldz, const uint16_t *X, int64_t ldx, float gamma,
                           uint16_t *Z_new, int64_t ldo, int32_t d, int64_t long_threshold, int32_t flags,
                           const clane_mirror_t *mirror, double *delta_partials, void *stream);
int clane_spmm_update_long_f32(const int64_t *rowptr, const int32_t *colidx, const float *P, const int32_t *long_rows,
                               int64_t n_long, int32_t waves_per_row, int64_t row0, const float *Z_old, int64_t ldz, const float *X,
                               int64_t ldx, float gamma, float *Z_new, int64_t ldo, int32_t d,
                               const clane_mirror_t *mirror, double *delta_partials, void *stream);
int clane_spmm_update_long_f64(const int64_t *rowptr, const int32_t *colidx, const double *P,
                               const int32_t *long_rows, int64_t n_long, int32_t waves_per_row, int64_t row0, const double *Z_old,
                               int64_t ldz, const double *X, int64_t ldx, double gamma, double *Z_new, int64_t ldo,
                               int32_t d, const clane_mirror_t *mirror, double *delta_partials, void *stream);
int clane_spmm_update_long_bf16(const int64_t *rowptr, const int32_t *colidx, const float *P,
                                const int32_t *long_rows, int64_t n_long, int32_t waves_per_row, int64_t row0, const uint16_t *Z_old,
                                int64_t ldz, const uint16_t *X, int64_t ldx, float gamma, uint16_t *Z_new,
                                int64_t ldo, int32_t d, const clane_mirror_t *mirror, double *delta_partials,
                                void *stream);

/*  clane_spmm_update_split_* : hub rows, each cut into segments of `edges_per_segment` edges (a multiple of 64)
 *                             that are gathered by separate 16-wave workgroups; segment sums go to `slab`
 *                             (clane_spmm_split_slab_len(n_segments, d) accumulate-type elements) and are added
 *                             per row in segment order, then the usual epilogue.  split_rows[n_split] local row
 *                             ids; seg_ptr[n_split+1] prefix sums of the rows' segment counts
 *                             (ceil(deg / edges_per_segment)); seg_row[n_segments] = index into split_rows of the
 *                             row each segment belongs to.  Writes n_split doubles to delta_partials. */
int64_t clane_spmm_split_slab_len(int64_t n_segments, int32_t d);
int clane_spmm_update_split_f32(const int64_t *rowptr, const int32_t *colidx, const float *P, const int32_t *split_rows,
                                const int64_t *seg_ptr, const int32_t *seg_row, int64_t n_split, int64_t n_segments,
                                int64_t edges_per_segment, int64_t row0, const float *Z_old, int64_t ldz,
                                const float *X, int64_t ldx, float gamma, float *Z_new, int64_t ldo, int32_t d,
                                float *slab, const clane_mirror_t *mirror, double *delta_partials, void *stream);
int clane_spmm_update_split_f64(const int64_t *rowptr, const int32_t *colidx, const double *P,
                                const int32_t *split_rows, const int64_t *seg_ptr, const int32_t *seg_row,
                                int64_t n_split, int64_t n_segments, int64_t edges_per_segment, int64_t row0,
                                const double *Z_old, int64_t ldz, const double *X, int64_t ldx, double gamma,
                                double *Z_new, int64_t ldo, int32_t d, double *slab, const clane_mirror_t *mirror,
                                double *delta_partials, void *stream);
int clane_spmm_update_split_bf16(const int64_t *rowptr, const int32_t *colidx, const float *P,
                                 const int32_t *split_rows, const int64_t *seg_ptr, const int32_t *seg_row,
                                 int64_t n_split, int64_t n_segments, int64_t edges_per_segment, int64_t row0,
                                 const uint16_t *Z_old, int64_t ldz, const uint16_t *X, int64_t ldx, float gamma,
                                 uint16_t *Z_new, int64_t ldo, int32_t d, float *slab, const clane_mirror_t *mirror,
                                 double *delta_partials, void *stream);

/*  clane_edge_score_class_* : K1 (graph.py:119-123 + similarity.py:26-37) over the listed long rows with XCD-affine
 *                             gathers -- the build_P counterpart of clane_spmm_update_class_* below, over the SAME item
 *                             arrays plus item_row (local row id of each item's source row).  A wave scores the edges
 *                             of one item (modes and `sums2` / `sq` as clane_edge_score_*).  With
 *                             CLANE_SCORE_FUSE_SOFTMAX every item leaves {max, sum exp} in stats[2 * slot] (2 *
 *                             n_slots accumulate-type elements) and each listed row is then soft-maxed from its
 *                             slots, combined in slot order; without it rowptr / class_rows / slot_ptr / stats may be
 *                             NULL and the raw scores stay (column-split runs all-reduce them first). */
int clane_edge_score_class_f32(const int64_t *rowptr, const int32_t *colidx, const int64_t *item_e0,
                               const int32_t *item_len, const int32_t *item_slot, const int32_t *item_row,
                               int64_t n_blocks, int32_t items_per_block, const int32_t *class_rows,
                               const int64_t *slot_ptr, int64_t n_rows, int64_t row0, const float *Z, int64_t ldz,
                               int32_t d, int32_t mode, const double *sums2, const float *sq, float *scores,
                               int32_t flags, float *stats, void *stream);
int clane_edge_score_class_f64(const int64_t *rowptr, const int32_t *colidx, const int64_t *item_e0,
                               const int32_t *item_len, const int32_t *item_slot, const int32_t *item_row,
                               int64_t n_blocks, int32_t items_per_block, const int32_t *class_rows,
                               const int64_t *slot_ptr, int64_t n_rows, int64_t row0, const double *Z, int64_t ldz,
                               int32_t d, int32_t mode, const double *sums2, const double *sq, double *scores,
                               int32_t flags, double *stats, void *stream);
int clane_edge_score_class_bf16(const int64_t *rowptr, const int32_t *colidx, const int64_t *item_e0,
                                const int32_t *item_len, const int32_t *item_slot, const int32_t *item_row,
                                int64_t n_blocks, int32_t items_per_block, const int32_t *class_rows,
                                const int64_t *slot_ptr, int64_t n_rows, int64_t row0, const uint16_t *Z, int64_t ldz,
                                int32_t d, int32_t mode, const double *sums2, const float *sq, float *scores,
                                int32_t flags, float *stats, void *stream);

/*  clane_spmm_update_class_* : long rows whose gathers are kept XCD-affine (no reference counterpart: the reference's
 *                             loop is embedder.py:84-92 for every row alike).  MI355X has 8 XCDs with a private 4 MiB
 *                             L2 each and deals workgroups to them round-robin (workgroup w -> XCD (w + c) % 8, c fixed within a launch).  The caller
 *                             gives every table row a CLASS 0..7 (the engine: an xor-fold of the row number's 3-bit groups -- not row % 8,
 *                             which would pin low address bits and use only part of an L2), sorts the edges of each listed row by
 *                             (class of the column, column) and cuts every class segment
 *                             into ITEMS of a few hundred edges; item arrays are laid out in blocks of
 *                             `items_per_block` (4..64) items of ONE class, block j of class b at block index
 *                             8 j + b (n_blocks blocks, padding items have item_len = 0), so XCD b only gathers rows
 *                             of class b and the eight L2s cache different eighths of the hot rows.
 *                             item_e0 / item_len: edge range of an item in colidx / P; item_slot: where its partial
 *                             sum goes in `slab` (clane_spmm_class_slab_len(n_slots, d) accumulate-type elements,
 *                             16-byte aligned).  The ORDER of the blocks is the caller's too: the engine puts the
 *                             pieces of its heaviest rows first, sub-class by sub-class, so that an XCD's hot
 *                             working set at any moment is a fraction of its class (clane_amd/xcd.py).
 *                             class_rows[n_rows] local row ids; slot_ptr[n_rows+1]: the slots of
 *                             row i are [slot_ptr[i], slot_ptr[i+1]) and are added in that order (reproducible),
 *                             then the usual epilogue.  Writes n_rows doubles to delta_partials.
 *                             flags: CLANE_SPMM_TABLE_BEYOND_CACHE or 0. */
int64_t clane_spmm_class_slab_len(int64_t n_slots, int32_t d);
int clane_spmm_update_class_f32(const int32_t *colidx, const float *P, const int64_t *item_e0, const int32_t *item_len,
                                const int32_t *item_slot, int64_t n_blocks, int32_t items_per_block,
                                const int32_t *class_rows, const int64_t *slot_ptr, int64_t n_rows, int64_t row0,
                                const float *Z_old, int64_t ldz, const float *X, int64_t ldx, float gamma, float *Z_new,
                                int64_t ldo, int32_t d, int32_t flags, float *slab, const clane_mirror_t *mirror,
                                double *delta_partials, void *stream);
int clane_spmm_update_class_f64(const int32_t *colidx, const double *P, const int64_t *item_e0, const int32_t *item_len,
                                const int32_t *item_slot, int64_t n_blocks, int32_t items_per_block,
                                const int32_t *class_rows, const int64_t *slot_ptr, int64_t n_rows, int64_t row0,
                                const double *Z_old, int64_t ldz, const double *X, int64_t ldx, double gamma,
                                double *Z_new, int64_t ldo, int32_t d, int32_t flags, double *slab, const clane_mirror_t *mirror,
                                double *delta_partials, void *stream);
int clane_spmm_update_class_bf16(const int32_t *colidx, const float *P, const int64_t *item_e0, const int32_t *item_len,
                                 const int32_t *item_slot, int64_t n_blocks, int32_t items_per_block,
                                 const int32_t *class_rows, const int64_t *slot_ptr, int64_t n_rows, int64_t row0,
                                 const uint16_t *Z_old, int64_t ldz, const uint16_t *X, int64_t ldx, float gamma,
                                 uint16_t *Z_new, int64_t ldo, int32_t d, int32_t flags, float *slab, const clane_mirror_t *mirror,
                                 double *delta_partials, void *stream);

/*  clane_spmm_update_owned_f32 : class rows whose sums never leave the CU (the reference's loop is embedder.py:90-92
 *                             for every row alike; no counterpart of the schedule).  clane_spmm_update_class_* sends
 *                             every partial sum of a row through `slab`, because the row's items run on eight XCDs.
 *                             Here one persistent workgroup per GROUP owns a set of the rows for the whole launch,
 *                             keeps their sums in LDS and walks the rows' (phase, class) segments STEP by step: all
 *                             groups gather columns of the same step at about the same time, so each XCD's L2 holds
 *                             that step's hot rows -- in time what the item blocks above do in space.  Nothing
 *                             synchronises the groups; the caller deals the rows so that the groups' edges agree.
 *                             The plan (device arrays, built by the caller: clane_amd/xcd.py owned_plan):
 *                             a row of many edges is cut into VIRTUAL rows, each with an LDS sum of its own; group g
 *                             takes its rows in the batches [grp_bat_ptr[g], grp_bat_ptr[g+1]), each through all
 *                             n_steps steps; batch b holds the virtual rows [bat_vrow_ptr[b], bat_vrow_ptr[b+1]) (at
 *                             most max_batch_vrows) and the rows [bat_row_ptr[b], bat_row_ptr[b+1]); the segments of
 *                             (batch b, step s) are [bat_seg_ptr[b n_steps + s], bat_seg_ptr[b n_steps + s + 1]):
 *                             seg_e0 / seg_len an edge range in colidx / P, seg_vrow the virtual row WITHIN the batch
 *                             (at most one segment per virtual row and step).  A segment is gathered in pieces of
 *                             `chunk` edges (a multiple of 64), each from zero, added to the virtual row's sum in
 *                             order.  Row j (batch order) is local row row_id[j], its virtual rows are
 *                             [row_vptr[j], row_vptr[j+1]) and are added in that order, then the usual epilogue; its
 *                             |delta| goes to delta_partials[row_part[j]].  So a row's sum is fixed by the plan's
 *                             (virtual row, step, piece) order alone: the number of groups, the batches, block_threads
 *                             and the timing do not change a bit.
 *                             block_threads: 64..1024, a multiple of 64.  d must fit one pass of the lane layout (fp32,
 *                             16-byte packs: d <= 256) and Z_old / X / Z_new must allow 16-byte packs; anything else
 *                             is CLANE_ERR_INVALID_ARGUMENT -- the caller keeps clane_spmm_update_class_* for it, as
 *                             for bf16 / fp64 tables and mirrored launches.  max_batch_vrows LDS sums of a whole row
 *                             (512 bytes up to d = 128, else 1 KiB) must fit 160 KiB less 1 KiB.
 *                             flags: CLANE_SPMM_TABLE_BEYOND_CACHE or 0, and CLANE_OWNED_LOADS(n): n row loads in flight
 *                             per wave (6, 8, 12 up to d = 128; 8, 12 above; 0 = the chunk kernel's choice).  Neither
 *                             changes a result. */
#define CLANE_OWNED_LOADS(n) (((n) & 0xff) << 8)
/* flag of the owned calls: a wave requests x / z_old of the next row group (and the ids of the one after) before it
 * finishes the current one, instead of one chain of dependent loads per group.  Changes no result. */
#define CLANE_OWNED_EPILOGUE_AHEAD (1 << 16)
typedef struct {
    const int32_t *grp_bat_ptr;
    const int32_t *bat_vrow_ptr;
    const int32_t *bat_row_ptr;
    const int32_t *bat_seg_ptr;
    const int64_t *seg_e0;
    const int32_t *seg_len;
    const int32_t *seg_vrow;
    const int32_t *row_id;
    const int32_t *row_part;
    const int32_t *row_vptr;
    int32_t n_groups;
    int32_t n_steps;
    int32_t chunk;
    int32_t max_batch_vrows;
} clane_owned_plan_t;
int clane_spmm_update_owned_f32(const int32_t *colidx, const float *P, const clane_owned_plan_t *plan,
                                int32_t block_threads, int64_t row0, const float *Z_old, int64_t ldz, const float *X,
                                int64_t ldx, float gamma, float *Z_new, int64_t ldo, int32_t d, int32_t flags,
                                double *delta_partials, void *stream);

/*  Every COLUMN TILE of a K3 pass in one launch (fp32, no mirror).  A sweep may be run as passes over column tiles of
 *  the same tables (the update is independent per column, embedder.py:92); calling clane_spmm_update_f32 /
 *  _class_f32 / _owned_f32 once per tile puts a drain and a ramp between the tiles of a pass on an in-order stream,
 *  although nothing orders them.  These take the WHOLE table (d columns) and `tile_cols`: tile t covers columns
 *  [t tile_cols, min(d, (t + 1) tile_cols)) -- the last may be narrower -- and is computed exactly as the per-tile call on
 *  (Z_old + t tile_cols, X + t tile_cols, Z_new + t tile_cols, width of the tile) computes it, with the kernel
 *  instance of a full tile's width and the flags; tile t's delta partials start at
 *  delta_partials + t * partials_tile_stride and are laid out as the per-tile call lays them out.  Bit for bit the
 *  per-tile calls: Z_new, every partial.  tile_cols must be a multiple of 4 (16-byte packs), Z_old / X / Z_new must
 *  allow 16-byte packs, and the last tile must take the lane layout of a full one (8 / 16 / 32 / 64 lanes for up to
 *  32 / 64 / 128 / more columns); anything else is CLANE_ERR_INVALID_ARGUMENT -- the caller keeps the per-tile calls.
 *   clane_spmm_update_tiles_f32        the row pass: a 1-D grid of tiles x workgroups, tile-major.
 *   clane_spmm_update_class_tiles_f32  chunk + combine, each ONE launch over all tiles.  The chunk grid is tiles x
 *                                      (n_blocks rounded up to a multiple of 8), so item block 8 j + b of every tile
 *                                      runs on XCD class b; n_slots = slot_ptr[n_rows]; tile t's chunk sums live at
 *                                      slab + t * clane_spmm_class_slab_len(n_slots, tile_cols): slab holds
 *                                      tiles * that many elements.
 *   clane_spmm_update_owned_tiles_f32  the persistent workgroups walk the tiles one after the other: the same plan, LDS
 *                                      sums (sized by tile_cols) and steps per tile. */
int clane_spmm_update_tiles_f32(const int64_t *rowptr, const int32_t *colidx, const float *P, int64_t nrows, int64_t row0,
                                const float *Z_old, int64_t ldz, const float *X, int64_t ldx, float gamma, float *Z_new,
                                int64_t ldo, int32_t d, int32_t tile_cols, int64_t long_threshold, int32_t flags,
                                double *delta_partials, int64_t partials_tile_stride, void *stream);
int clane_spmm_update_class_tiles_f32(const int32_t *colidx, const float *P, const int64_t *item_e0,
                                      const int32_t *item_len, const int32_t *item_slot, int64_t n_blocks,
                                      int32_t items_per_block, const int32_t *class_rows, const int64_t *slot_ptr,
                                      int64_t n_rows, int64_t n_slots, int64_t row0, const float *Z_old, int64_t ldz,
                                      const float *X, int64_t ldx, float gamma, float *Z_new, int64_t ldo, int32_t d,
                                      int32_t tile_cols, int32_t flags, float *slab, double *delta_partials,
                                      int64_t partials_tile_stride, void *stream);
int clane_spmm_update_owned_tiles_f32(const int32_t *colidx, const float *P, const clane_owned_plan_t *plan,
                                      int32_t block_threads, int64_t row0, const float *Z_old, int64_t ldz,
                                      const float *X, int64_t ldx, float gamma, float *Z_new, int64_t ldo, int32_t d,
                                      int32_t tile_cols, int32_t flags, double *delta_partials,
                                      int64_t partials_tile_stride, void *stream);

/*  ONE WEIGHT PER ROW.  In reference mode the scores share one global denominator (similarity.py:37); on a graph of a few
 *  million edges every score is O(1e-9), its exp is exactly 1 and build_P (graph.py:118-128) leaves P[e] == 1 / deg, bit for
 *  bit, on every edge of every row.  Reading that weight per edge is then 4 bytes per edge and column tile for nothing.
 *   clane_row_weight_*   row_weight[r] = P[rowptr[r]] (0 for a row without edges) for the nrows rows of rowptr, and
 *                        mixed[0] = 1 if some edge's weight differs from its row's first in any bit, else 0.  To be run
 *                        after everything that writes P; one pass over P.
 *   clane_spmm_update_rw_f32, _class_rw_f32, _owned_rw_f32 and their _tiles_ forms
 *                        the calls of the same names without `_rw`, for a P of which clane_row_weight_* said mixed[0] == 0:
 *                        they take `row_weight` (one float per row of the call: rowptr's rows; for the class and owned
 *                        calls the rows that class_rows / plan->row_id are relative to) where those take P, and read no
 *                        per-edge weight.  The class calls also take item_row (every item's row, as
 *                        clane_edge_score_class_* takes it), the owned calls seg_row (every segment's row, in the order
 *                        of plan->seg_e0).  No mirror.  Z_new and every delta partial are bit for bit those of the
 *                        per-edge call on the P the weights were taken from: the same fma per edge in the same order. */
int clane_row_weight_f32(const int64_t *rowptr, const float *P, int64_t nrows, float *row_weight, int32_t *mixed,
                         void *stream);
int clane_row_weight_f64(const int64_t *rowptr, const double *P, int64_t nrows, double *row_weight, int32_t *mixed,
                         void *stream);
int clane_spmm_update_rw_f32(const int64_t *rowptr, const int32_t *colidx, const float *row_weight, int64_t nrows,
                             int64_t row0, const float *Z_old, int64_t ldz, const float *X, int64_t ldx, float gamma,
                             float *Z_new, int64_t ldo, int32_t d, int64_t long_threshold, int32_t flags,
                             double *delta_partials, void *stream);
int clane_spmm_update_tiles_rw_f32(const int64_t *rowptr, const int32_t *colidx, const float *row_weight, int64_t nrows,
                                   int64_t row0, const float *Z_old, int64_t ldz, const float *X, int64_t ldx, float gamma,
                                   float *Z_new, int64_t ldo, int32_t d, int32_t tile_cols, int64_t long_threshold,
                                   int32_t flags, double *delta_partials, int64_t partials_tile_stride, void *stream);
int clane_spmm_update_class_rw_f32(const int32_t *colidx, const float *row_weight, const int64_t *item_e0,
                                   const int32_t *item_len, const int32_t *item_slot, const int32_t *item_row,
                                   int64_t n_blocks, int32_t items_per_block, const int32_t *class_rows,
                                   const int64_t *slot_ptr, int64_t n_rows, int64_t row0, const float *Z_old, int64_t ldz,
                                   const float *X, int64_t ldx, float gamma, float *Z_new, int64_t ldo, int32_t d,
                                   int32_t flags, float *slab, double *delta_partials, void *stream);
int clane_spmm_update_class_tiles_rw_f32(const int32_t *colidx, const float *row_weight, const int64_t *item_e0,
                                         const int32_t *item_len, const int32_t *item_slot, const int32_t *item_row,
                                         int64_t n_blocks, int32_t items_per_block, const int32_t *class_rows,
                                         const int64_t *slot_ptr, int64_t n_rows, int64_t n_slots, int64_t row0,
                                         const float *Z_old, int64_t ldz, const float *X, int64_t ldx, float gamma,
                                         float *Z_new, int64_t ldo, int32_t d, int32_t tile_cols, int32_t flags,
                                         float *slab, double *delta_partials, int64_t partials_tile_stride,
                                         void *stream);
int clane_spmm_update_owned_rw_f32(const int32_t *colidx, const float *row_weight, const clane_owned_plan_t *plan,
                                   const int32_t *seg_row, int32_t block_threads, int64_t row0, const float *Z_old,
                                   int64_t ldz, const float *X, int64_t ldx, float gamma, float *Z_new, int64_t ldo,
                                   int32_t d, int32_t flags, double *delta_partials, void *stream);
int clane_spmm_update_owned_tiles_rw_f32(const int32_t *colidx, const float *row_weight, const clane_owned_plan_t *plan,
                                         const int32_t *seg_row, int32_t block_threads, int64_t row0, const float *Z_old,
                                         int64_t ldz, const float *X, int64_t ldx, float gamma, float *Z_new, int64_t ldo,
                                         int32_t d, int32_t tile_cols, int32_t flags, double *delta_partials,
                                         int64_t partials_tile_stride, void *stream);

/* out[0] = sum of partials[0..n) in a fixed order (bitwise reproducible).  Finishes embedder.py:94 / :60.
 * ws: clane_reduce_ws_len() doubles. */
int clane_reduce_partials(const double *partials, int64_t n, double *ws, double *out, void *stream);

/* sum|A - B| over an [nrows, d] matrix pair -> out[0] (outer-loop delta, embedder.py:60).
 * sq_a (accumulate type, [nrows]; NULL: not wanted): also |A[i,:]|^2 for every row, bit for bit what clane_row_sqnorm_*
 * gives on A -- the pass reads every row of A anyway, so with A = the new embeddings the next build_P of the outer loop
 * (embedder.py:59 after :60) gets its norms (similarity.py:37) for no extra traffic.
 * ws: clane_reduce_ws_len() doubles. */
int clane_l1_distance_f32(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t nrows, int32_t d,
                          float *sq_a, double *ws, double *out, void *stream);
int clane_l1_distance_f64(const double *A, int64_t lda, const double *B, int64_t ldb, int64_t nrows, int32_t d,
                          double *sq_a, double *ws, double *out, void *stream);
int clane_l1_distance_bf16(const uint16_t *A, int64_t lda, const uint16_t *B, int64_t ldb, int64_t nrows, int32_t d,
                           float *sq_a, double *ws, double *out, void *stream);

/* dst[i,:] = src[idx[i],:] for i < n: packs the rows other ranks read into the send buffer of the
 * multi-GPU halo exchange (no counterpart in the single-process reference). */
int clane_gather_rows_f32(const float *src, int64_t lds, const int32_t *idx, int64_t n, int32_t d, float *dst,
                          int64_t ldd, void *stream);
int clane_gather_rows_f64(const double *src, int64_t lds, const int32_t *idx, int64_t n, int32_t d, double *dst,
                          int64_t ldd, void *stream);
int clane_gather_rows_bf16(const uint16_t *src, int64_t lds, const int32_t *idx, int64_t n, int32_t d, uint16_t *dst,
                           int64_t ldd, void *stream);

/* ---- CosineSimilarity.__call__ on explicit pairs (similarity.py:26-37):
 *   out[i] = dot(A[i,:], B[i,:]) / (||A||_F * ||B||_F)      -- global denominators.
 * ws: clane_reduce_ws_len() doubles. */
int clane_pair_cosine_f32(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t nrows, int32_t d,
                          float *out, double *ws, void *stream);
int clane_pair_cosine_f64(const double *A, int64_t lda, const double *B, int64_t ldb, int64_t nrows, int32_t d,
                          double *out, double *ws, void *stream);

/* ---- Bilinear similarity (AsymmertricSimilarity, similarity.py:40-57): build_P (graph.py:118-128) as one row projection
 * on the matrix cores and one pair K1 -- instead of gathering z_src / z_dst of every edge and projecting both per edge.
 *
 *  clane_project_rows_* : Y[r, :] = W . Z[r, :] for r < rows, i.e. Y = Z W^T.  Z: [rows, d] (leading dimension
 *                         ldz >= d) in the table dtype; W: [2d, d] row-major in the accumulate dtype,
 *                         W = cat(Phi_src.weight, Phi_dst.weight) (nn.Linear stores [out, in]); Y: [rows, 2d]
 *                         (ldy >= 2d) in the accumulate dtype, columns [0, d) = Phi_src z, [d, 2d) = Phi_dst z.
 *                         fp32 / bf16 tables: f32-input MFMA (bf16 widened on staging, W stays f32); fp64: f64 MFMA.
 *                         Any d >= 1 and rows >= 0; no atomics, no split-K: bit-reproducible. */
int clane_project_rows_f32(const float *Z, int64_t rows, int32_t d, int64_t ldz, const float *W, float *Y, int64_t ldy,
                           void *stream);
int clane_project_rows_f64(const double *Z, int64_t rows, int32_t d, int64_t ldz, const double *W, double *Y,
                           int64_t ldy, void *stream);
int clane_project_rows_bf16(const uint16_t *Z, int64_t rows, int32_t d, int64_t ldz, const float *W, float *Y,
                            int64_t ldy, void *stream);

/*  clane_edge_score_pair_* : K1 of clane_edge_score_* with two tables -- the score of edge (r, c) is the raw dot of
 *                            S[row0 + r, 0:d) and N[c, 0:d) (the bilinear score (Phi_src z_r) . (Phi_dst z_c) when
 *                            S = Y, N = Y + d, lds = ldn = ldy), no denominators.  rowptr / colidx / long rows /
 *                            flags (CLANE_SCORE_FUSE_SOFTMAX) exactly as clane_edge_score_*.  No bf16 instance: Y is
 *                            always in the accumulate dtype.
 *  clane_edge_score_class_pair_* : the same over the class rows' work items, as clane_edge_score_class_*. */
int clane_edge_score_pair_f32(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0, const float *S,
                              int64_t lds, const float *N, int64_t ldn, int32_t d, float *scores, int32_t flags,
                              int64_t long_threshold, const int32_t *long_rows, int64_t n_long, void *stream);
int clane_edge_score_pair_f64(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, int64_t row0,
                              const double *S, int64_t lds, const double *N, int64_t ldn, int32_t d, double *scores,
                              int32_t flags, int64_t long_threshold, const int32_t *long_rows, int64_t n_long,
                              void *stream);
int clane_edge_score_class_pair_f32(const int64_t *rowptr, const int32_t *colidx, const int64_t *item_e0,
                                    const int32_t *item_len, const int32_t *item_slot, const int32_t *item_row,
                                    int64_t n_blocks, int32_t items_per_block, const int32_t *class_rows,
                                    const int64_t *slot_ptr, int64_t n_rows, int64_t row0, const float *S, int64_t lds,
                                    const float *N, int64_t ldn, int32_t d, float *scores, int32_t flags, float *stats,
                                    void *stream);
int clane_edge_score_class_pair_f64(const int64_t *rowptr, const int32_t *colidx, const int64_t *item_e0,
                                    const int32_t *item_len, const int32_t *item_slot, const int32_t *item_row,
                                    int64_t n_blocks, int32_t items_per_block, const int32_t *class_rows,
                                    const int64_t *slot_ptr, int64_t n_rows, int64_t row0, const double *S,
                                    int64_t lds, const double *N, int64_t ldn, int32_t d, double *scores,
                                    int32_t flags, double *stats, void *stream);

/* ---- Training the bilinear similarity (IterativeEmbedder.update_similarity_measure, embedder.py:249-289) on explicit
 * pairs, without a host decision per step.  A batch is B pairs (src[k], dst[k]) of TABLE ROWS (int32; a row outside
 * [0, table_rows) is read as a zero row), linked[k] (uint8: the pair is an edge), u[k] (accumulate dtype, uniform in
 * [0, 1): the Bernoulli trial of embedder.py:278 succeeds where u < p; a recorded trial is replayed with u = 0 for a
 * success and u = 1 for a failure).  W = cat(Phi_src.weight, Phi_dst.weight), [2d, d] row-major, accumulate dtype.
 * No allocation, no atomics, every sum in a fixed order: two calls give the same bits.
 *
 *  clane_pair_project_* : A[k, :] = Phi_src . Z[src[k], 0:d), Bm[k, :] = Phi_dst . Z[dst[k], 0:d), both [B, d]
 *                         contiguous in the accumulate dtype.  The MFMA tiling of clane_project_rows_* with the rows
 *                         taken through the index lists: nothing of the size of the table is touched.
 *  clane_pair_loss_*    : s = A[k] . Bm[k], p = sigmoid(s), q = sigmoid(-s) (never 1 - p), mask = linked XOR (u < p),
 *                         loss_k = -log((linked ? p : q) + 1e-10) (embedder.py:276-279);
 *                         g[k] = d loss_k / d s = linked ? -p q / (p + 1e-10) : p q / (q + 1e-10), 0 where mask is 0;
 *                         stats[0] = sum of mask * loss_k, stats[1] = M = sum of mask, in double.
 *                         ws: clane_reduce_ws_len() doubles.
 *  clane_pair_grad_*    : the gradient of mean over the masked pairs of loss_k (embedder.py:282-283):
 *                         dW[0:d, :] = (1/M) sum_k g_k Bm[k, :]^T Z[src[k], :], dW[d:2d, :] = (1/M) sum_k g_k A[k, :]^T
 *                         Z[dst[k], :], M read from stats[1] on the device; M = 0 gives dW = 0.  Chunks of 2048 pairs are
 *                         contracted by separate workgroups (MFMA) into ws (clane_pair_grad_ws_len(B, d) accumulate-
 *                         dtype elements) and added in chunk order.
 *  clane_adam_step_*    : one step of torch.optim.Adam with its defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay,
 *                         no amsgrad) on W, m, v of n elements (embedder.py:259, :285).  state[0] = steps taken so far,
 *                         state[1] = sum of the step losses since the caller zeroed it (embedder.py:286): the step adds
 *                         1 and stats[0] / M.  stats[1] == 0: nothing changes at all -- the `continue` of
 *                         embedder.py:280-281 without the host looking.
 *  clane_pair_labels    : linked[k] = dst[k] in colidx[rowptr[src[k]] .. rowptr[src[k] + 1]) by binary search -- what
 *                         graph.py:99 means; the rows of this CSR must be sorted and unique (src outside [0, nrows): 0). */
int clane_pair_project_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *src,
                           const int32_t *dst, int64_t B, const float *W, float *A, float *Bm, void *stream);
int clane_pair_project_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *src,
                           const int32_t *dst, int64_t B, const double *W, double *A, double *Bm, void *stream);
int clane_pair_project_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *src,
                            const int32_t *dst, int64_t B, const float *W, float *A, float *Bm, void *stream);
int clane_pair_loss_f32(const float *A, const float *Bm, int64_t B, int32_t d, const uint8_t *linked, const float *u,
                        float *g, uint8_t *mask, double *ws, double *stats, void *stream);
int clane_pair_loss_f64(const double *A, const double *Bm, int64_t B, int32_t d, const uint8_t *linked, const double *u,
                        double *g, uint8_t *mask, double *ws, double *stats, void *stream);
int64_t clane_pair_grad_ws_len(int64_t B, int32_t d);
int clane_pair_grad_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *src,
                        const int32_t *dst, int64_t B, const float *A, const float *Bm, const float *g,
                        const double *stats, float *ws, float *dW, void *stream);
int clane_pair_grad_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *src,
                        const int32_t *dst, int64_t B, const double *A, const double *Bm, const double *g,
                        const double *stats, double *ws, double *dW, void *stream);
int clane_pair_grad_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *src,
                         const int32_t *dst, int64_t B, const float *A, const float *Bm, const float *g,
                         const double *stats, float *ws, float *dW, void *stream);
int clane_adam_step_f32(float *W, float *m, float *v, const float *dW, int64_t n, double lr, const double *stats,
                        double *state, void *stream);
int clane_adam_step_f64(double *W, double *m, double *v, const double *dW, int64_t n, double lr, const double *stats,
                        double *state, void *stream);
int clane_pair_labels(const int64_t *rowptr, const int32_t *colidx, int64_t nrows, const int32_t *src,
                      const int32_t *dst, int64_t B, uint8_t *linked, void *stream);

/* ---- Link prediction: which rows does a query row score highest against, and what does an explicit pair score.  No
 * reference counterpart (the reference stops at Z.npy); the score is the model's own: the bilinear
 * (Phi_src z_u) . (Phi_dst z_v) of AsymmertricSimilarity (similarity.py:40-57) or the cosine of CosineSimilarity
 * (similarity.py:26-37).  S (leading dimension lds) is the query table, N (ldn) the candidate table, both of
 * table_rows rows of type T; only columns [0, d) are read.  Bilinear: S = Y, N = Y + d, lds = ldn = ldy of the table
 * clane_project_rows_* leaves (f32 / f64 instance).  Cosine: S = N = Z.  mode / sums2 / sq exactly as
 * clane_edge_score_* takes them, sq indexed by table row: RAW_DOT the dot; PER_EDGE dot / (sqrt(sq[q]) sqrt(sq[v])),
 * 0 where sq[q] sq[v] == 0; REFERENCE dot / sqrt(sums2[0] sums2[1]).  Inputs are assumed finite.  No allocation, no
 * synchronisation, no atomics on memory; two calls give the same bits.
 *
 *  clane_rank_scores_* : for query i = row q_rows[i] (int32, repeats allowed; a row outside the table has no
 *                        candidates) the k best candidates of every one of n_slabs contiguous ranges of the table's
 *                        rows: cand_score (accumulate dtype) and cand_id (int32), both [Q, n_slabs, k], unused places
 *                        -inf / -1.  The Q x table_rows scores never exist in memory: the MFMA tiling of
 *                        clane_project_rows_* with the query rows gathered, the selection fused behind each tile.
 *                        label (int32 [table_rows], NULL = the row itself): the id reported for a candidate and the
 *                        key that breaks ties; label[v] < 0: row v never is a candidate (padding rows).
 *                        excl_rowptr (int64 [table_rows + 1]) / excl_colidx (int32): a CSR in table-row numbering with
 *                        sorted, unique rows (what clane_pair_labels searches); candidate v is skipped for query row r
 *                        when v is in row r.  Both NULL: nothing is skipped this way.  exclude_self != 0 also skips
 *                        v == r.  k in 1..CLANE_RANK_MAX_K.  n_slabs >= 1 lets a small Q fill the card; more slabs
 *                        than the table has 128-row tiles leave the surplus empty.
 *  clane_rank_merge_*  : out_score / out_id [Q, k] from the [Q, n_slabs, k] candidates, score descending, ties by
 *                        label ascending -- a total order, labels being unique among eligible rows; fewer than k
 *                        eligible candidates: the tail is -inf / -1.  A pair's score comes out of the same accumulation
 *                        chain whatever slab it falls in: the result is bit-identical for every n_slabs.
 *  clane_pair_score_*  : out[i] = score(src[i], dst[i]) for B explicit pairs of table rows (int32; an index outside
 *                        [0, table_rows) reads as a zero row: score 0) -- held-out evaluation touches nothing of the
 *                        size of the table.  The lane layout of clane_edge_score_* (a sub-wave per pair).
 *  clane_rank_count_*  : for pair i = (query row q_rows[i], target row t_rows[i]) (int32, repeats allowed) the filtered
 *                        rank's ingredients.  target_score[B] (accumulate dtype) is the score the pair gets INSIDE
 *                        clane_rank_scores_* -- the same accumulation chain and scaling, bit for bit.  counts
 *                        [B, n_slabs, 4] (int32) holds for the candidate rows of slab s, in this order: greater (eligible
 *                        candidates that score above the target), equal_lower / equal_higher (eligible candidates whose
 *                        score equals the target's and whose label is below / above the target's) and eligible (all
 *                        eligible candidates).  The caller sums over the slabs (integers: the sums do not depend on
 *                        n_slabs); 1 + greater + equal_lower is the target's place in the order of clane_rank_merge_*.
 *                        Candidate v is eligible for the pair under the rules of clane_rank_scores_* (label, excl_*,
 *                        exclude_self, all taken the same way) and when it is not the target itself: the target never
 *                        is a candidate and never is filtered -- a target inside the query's exclusion row (an edge
 *                        still in the graph) is ranked among the non-edges.  A pair whose query or target lies outside
 *                        the table, or whose target has a negative label, has no rank: four -1 in every slab and -inf in
 *                        target_score.  The exclusion rows are walked by a cursor per pair, not searched per candidate.
 *                        No atomics on memory; two calls give the same bits. */
#define CLANE_RANK_MAX_K 32
int clane_rank_scores_f32(const float *S, int64_t lds, const float *N, int64_t ldn, int64_t table_rows, int32_t d,
                          const int32_t *q_rows, int64_t Q, int32_t mode, const double *sums2, const float *sq,
                          const int32_t *label, const int64_t *excl_rowptr, const int32_t *excl_colidx,
                          int32_t exclude_self, int32_t k, int32_t n_slabs, float *cand_score, int32_t *cand_id,
                          void *stream);
int clane_rank_scores_f64(const double *S, int64_t lds, const double *N, int64_t ldn, int64_t table_rows, int32_t d,
                          const int32_t *q_rows, int64_t Q, int32_t mode, const double *sums2, const double *sq,
                          const int32_t *label, const int64_t *excl_rowptr, const int32_t *excl_colidx,
                          int32_t exclude_self, int32_t k, int32_t n_slabs, double *cand_score, int32_t *cand_id,
                          void *stream);
int clane_rank_scores_bf16(const uint16_t *S, int64_t lds, const uint16_t *N, int64_t ldn, int64_t table_rows,
                           int32_t d, const int32_t *q_rows, int64_t Q, int32_t mode, const double *sums2,
                           const float *sq, const int32_t *label, const int64_t *excl_rowptr,
                           const int32_t *excl_colidx, int32_t exclude_self, int32_t k, int32_t n_slabs,
                           float *cand_score, int32_t *cand_id, void *stream);
int clane_rank_merge_f32(const float *cand_score, const int32_t *cand_id, int64_t Q, int32_t n_slabs, int32_t k,
                         float *out_score, int32_t *out_id, void *stream);
int clane_rank_merge_f64(const double *cand_score, const int32_t *cand_id, int64_t Q, int32_t n_slabs, int32_t k,
                         double *out_score, int32_t *out_id, void *stream);
int clane_pair_score_f32(const float *S, int64_t lds, const float *N, int64_t ldn, int64_t table_rows, int32_t d,
                         const int32_t *src, const int32_t *dst, int64_t B, int32_t mode, const double *sums2,
                         const float *sq, float *out, void *stream);
int clane_pair_score_f64(const double *S, int64_t lds, const double *N, int64_t ldn, int64_t table_rows, int32_t d,
                         const int32_t *src, const int32_t *dst, int64_t B, int32_t mode, const double *sums2,
                         const double *sq, double *out, void *stream);
int clane_pair_score_bf16(const uint16_t *S, int64_t lds, const uint16_t *N, int64_t ldn, int64_t table_rows,
                          int32_t d, const int32_t *src, const int32_t *dst, int64_t B, int32_t mode,
                          const double *sums2, const float *sq, float *out, void *stream);
int clane_rank_count_f32(const float *S, int64_t lds, const float *N, int64_t ldn, int64_t table_rows, int32_t d,
                         const int32_t *q_rows, const int32_t *t_rows, int64_t B, int32_t mode, const double *sums2,
                         const float *sq, const int32_t *label, const int64_t *excl_rowptr,
                         const int32_t *excl_colidx, int32_t exclude_self, int32_t n_slabs, float *target_score,
                         int32_t *counts, void *stream);
int clane_rank_count_f64(const double *S, int64_t lds, const double *N, int64_t ldn, int64_t table_rows, int32_t d,
                         const int32_t *q_rows, const int32_t *t_rows, int64_t B, int32_t mode, const double *sums2,
                         const double *sq, const int32_t *label, const int64_t *excl_rowptr,
                         const int32_t *excl_colidx, int32_t exclude_self, int32_t n_slabs, double *target_score,
                         int32_t *counts, void *stream);
int clane_rank_count_bf16(const uint16_t *S, int64_t lds, const uint16_t *N, int64_t ldn, int64_t table_rows, int32_t d,
                         const int32_t *q_rows, const int32_t *t_rows, int64_t B, int32_t mode, const double *sums2,
                         const float *sq, const int32_t *label, const int64_t *excl_rowptr,
                         const int32_t *excl_colidx, int32_t exclude_self, int32_t n_slabs, float *target_score,
                         int32_t *counts, void *stream);

/* ---- node classification probe (csrc/label_probe.h) ------------------------------------------------------------------
 * F multi-class logistic regressions on the rows `rows[0..n)` of the table Z (an index outside [0, table_rows) reads as a
 * zero row), classes y[i] in [0, C), 2 <= C <= CLANE_PROBE_MAX_CLASSES.  The fits' weights are stacked: W [K, d] and
 * bias [K] in the accumulate type, K = F * Cp, fit f's class c in row f * Cp + c, Cp = C rounded up to a power of two
 * (rows of pad classes are ignored).  split [n, ld_split >= F] (uint8): row i trains fit f where split[i, f] != 0.
 *
 * forward: logits = Z[rows] . W^T + bias never reach memory; per (row, fit) the log-sum-exp over the C real classes gives
 *   loss[f] = sum_i split[i, f] (lse - logit[y_i])                (always; double; loss_ws: probe_loss_ws_len doubles)
 *   G[i, f Cp + c] = split[i, f] (p_c - [c == y_i]), pad columns 0   (CLANE_PROBE_WRITE_G; G is [n, K] contiguous)
 *   pred[i, f] = argmax_c, ties to the lowest class, every row      (CLANE_PROBE_WRITE_PRED; pred is [n, ld_pred >= F])
 * grad: dW [K, d] = G^T . Z[rows], db [K] = sum_i G[i, :] (ws: probe_grad_ws_len elements of the accumulate type).
 * No atomics: two calls give the same bits, and a fit's results do not depend on the other fits of the call. */
#define CLANE_PROBE_MAX_CLASSES 64
#define CLANE_PROBE_WRITE_G 1
#define CLANE_PROBE_WRITE_PRED 2
int clane_probe_forward_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,
                            const int32_t *y, int64_t n, const uint8_t *split, int64_t ld_split, const float *W,
                            const float *bias, int32_t F, int32_t C, int32_t flags, float *G, double *loss_ws,
                            double *loss, int32_t *pred, int64_t ld_pred, void *stream);
int clane_probe_forward_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,
                            const int32_t *y, int64_t n, const uint8_t *split, int64_t ld_split, const double *W,
                            const double *bias, int32_t F, int32_t C, int32_t flags, double *G, double *loss_ws,
                            double *loss, int32_t *pred, int64_t ld_pred, void *stream);
int clane_probe_forward_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,
                             const int32_t *y, int64_t n, const uint8_t *split, int64_t ld_split, const float *W,
                             const float *bias, int32_t F, int32_t C, int32_t flags, float *G, double *loss_ws,
                             double *loss, int32_t *pred, int64_t ld_pred, void *stream);
int clane_probe_grad_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                         const float *G, int32_t K, float *ws, float *dW, float *db, void *stream);
int clane_probe_grad_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                         const double *G, int32_t K, double *ws, double *dW, double *db, void *stream);
int clane_probe_grad_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                          const float *G, int32_t K, float *ws, float *dW, float *db, void *stream);
int64_t clane_probe_loss_ws_len(int64_t n, int32_t F);
int64_t clane_probe_grad_ws_len(int64_t n, int32_t K, int32_t d);

/* ---- multi-label probe (csrc/multilabel_probe.h) -----------------------------------------------------------------------
 * F one-vs-rest logistic regressions per class on the same stacked layout (W [K, d], bias [K], K = F * Cp, Cp = C rounded up
 * to a power of two), 1 <= C <= CLANE_PROBE_MAX_CLASSES.  ymask [n] (uint64): bit c set where row i has class c.
 * col_state [K] (int8): 0 a fitted column, -1 / +1 a column whose class no / every training row of its fit has (pad
 * columns: ignored).  With l the logit, y the row's bit and "live" = split[i, f] != 0 and col_state == 0:
 *   loss[f] = sum over live (i, c) of softplus(l) - y l            (always; double; loss_ws: probe_loss_ws_len doubles)
 *   G[i, f Cp + c] = sigmoid(l) - y where live, else 0              (CLANE_PROBE_WRITE_G; G is [n, K] contiguous)
 *   pred[i, f] = a uint64 mask of predicted classes, every row      (CLANE_PROBE_WRITE_PRED; pred is [n, ld_pred >= F])
 *     a column's value is l, -inf (state -1) or +inf (state +1); without CLANE_PROBE_PRED_TOPK bit c is set iff the value
 *     is > 0; with it a row with k = popcount(ymask[i]) <= max_labels classes gets the k columns of highest value, ties to
 *     the lowest class, a NaN or -inf value never (so fewer than k bits may be set).  0 <= max_labels <= C bounds the
 *     rounds: it must be at least the largest popcount of ymask.
 * The gradient of the weights is clane_probe_grad_* on this G.  No atomics: two calls give the same bits, and a fit's results
 * do not depend on the other fits of the call. */
#define CLANE_PROBE_PRED_TOPK 4
int clane_probe_forward_ovr_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,
                                const uint64_t *ymask, int64_t n, const uint8_t *split, int64_t ld_split, const float *W,
                                const float *bias, const int8_t *col_state, int32_t F, int32_t C, int32_t max_labels,
                                int32_t flags, float *G, double *loss_ws, double *loss, uint64_t *pred, int64_t ld_pred,
                                void *stream);
int clane_probe_forward_ovr_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,
                                const uint64_t *ymask, int64_t n, const uint8_t *split, int64_t ld_split, const double *W,
                                const double *bias, const int8_t *col_state, int32_t F, int32_t C, int32_t max_labels,
                                int32_t flags, double *G, double *loss_ws, double *loss, uint64_t *pred, int64_t ld_pred,
                                void *stream);
int clane_probe_forward_ovr_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,
                                 const uint64_t *ymask, int64_t n, const uint8_t *split, int64_t ld_split, const float *W,
                                 const float *bias, const int8_t *col_state, int32_t F, int32_t C, int32_t max_labels,
                                 int32_t flags, float *G, double *loss_ws, double *loss, uint64_t *pred, int64_t ld_pred,
                                 void *stream);

/* ---- applying fitted probes (csrc/label_predict.h) ---------------------------------------------------------------------
 * Class probabilities and the top_m classes of the rows `rows[0..n)` of the table Z (an index outside [0, table_rows) reads
 * as a zero row) under F stacked models: W [K, d] and bias [K] as above, K = F * Cp.  The logits never reach memory.
 *   soft-max (default, 2 <= C): p_c = exp(l_c - max) / sum exp(l - max) over the C real classes, with the reductions and the
 *     order of operations of clane_probe_forward_*: p_c - [c == y] equals its G for a training row bit for bit.  A class's
 *     value is l_c.
 *   CLANE_PREDICT_SIGMOID (one-vs-rest models, 1 <= C): p_c = sigmoid(l_c) per column as in clane_probe_forward_ovr_*;
 *     col_state [K] (int8) as there: a column of state -1 / +1 has value -inf / +inf and p = 0 / 1.
 *   top_class [n, F, top_m] (int32) and top_prob [n, F, top_m] (accumulate type), 1 <= top_m <= CLANE_PREDICT_MAX_TOP: the
 *     classes of highest value, best first, ties to the lowest class, a NaN or -inf value never; where fewer than top_m
 *     classes are eligible the rest is -1 and 0.
 *   proba [n, F, C] (accumulate type; CLANE_PREDICT_WRITE_PROBA): the probability of every real class.
 * No atomics: two calls give the same bits, and a fit's results do not depend on the other fits of the call. */
#define CLANE_PREDICT_SIGMOID 1
#define CLANE_PREDICT_WRITE_PROBA 2
#define CLANE_PREDICT_MAX_TOP 8
int clane_probe_predict_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                            const float *W, const float *bias, const int8_t *col_state, int32_t F, int32_t C,
                            int32_t top_m, int32_t flags, int32_t *top_class, float *top_prob, float *proba,
                            void *stream);
int clane_probe_predict_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                            const double *W, const double *bias, const int8_t *col_state, int32_t F, int32_t C,
                            int32_t top_m, int32_t flags, int32_t *top_class, double *top_prob, double *proba,
                            void *stream);
int clane_probe_predict_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                             const float *W, const float *bias, const int8_t *col_state, int32_t F, int32_t C,
                             int32_t top_m, int32_t flags, int32_t *top_class, float *top_prob, float *proba,
                             void *stream);

/* ---- Gaussian mixtures (csrc/mixture.h) --------------------------------------------------------------------------------
 * One EM iteration of R diagonal-covariance Gaussian mixtures of K components, 1 <= K <= CLANE_MIXTURE_MAX_COMPONENTS, on the
 * rows `rows[0..n)` of the table Z (an index outside [0, table_rows) reads as a zero row).  Every row is centred in the
 * loaders: xc = x - mean, mean [d] in the accumulate type (a zero row is centred like any row).  Both steps contract the
 * 2 d wide operand phi(x) = [xc^2 | xc].  The restarts are stacked as the probes' fits are: Kp = K rounded up to a power of
 * two, restart r's component c in row r * Kp + c (rows of pad components are ignored).
 *
 * estep: Wm [R * Kp, 2 d] = [-a/2 | mu a] with a = 1 / variance, cst [R * Kp] = log pi - (d log 2 pi + sum log variance +
 *   sum mu^2 a) / 2, both in the accumulate type.  The logits l = phi . Wm^T + cst never reach memory; per (row, restart)
 *   the log-sum-exp over the K real components gives
 *   ll[r] = sum_i lse_i                                  (always; double; ll_ws: mixture_ll_ws_len doubles)
 *   resp[i, r Kp + c] = exp(l_c - lse_i), pad columns 0   (CLANE_MIXTURE_WRITE_RESP; resp is [n, R * Kp] contiguous)
 *   assign[i, r] = argmax_c, ties to the lowest component (CLANE_MIXTURE_WRITE_ASSIGN; assign is [n, ld_assign >= R])
 * mstep: S [K, 2 d] = resp^T . phi(Z[rows]) and nk [K] = sum_i resp[i, :], K = R * Kp here, the rows in chunks whose partial
 *   tiles are summed in chunk order (ws: mixture_mstep_ws_len elements of the accumulate type).
 * No atomics: two calls give the same bits, and a restart's results do not depend on the other restarts of the call. */
#define CLANE_MIXTURE_MAX_COMPONENTS 64
#define CLANE_MIXTURE_WRITE_RESP 1
#define CLANE_MIXTURE_WRITE_ASSIGN 2
int clane_mixture_estep_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                            const float *mean, const float *Wm, const float *cst, int32_t R, int32_t K, int32_t flags,
                            float *resp, double *ll_ws, double *ll, int32_t *assign, int64_t ld_assign, void *stream);
int clane_mixture_estep_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                            const double *mean, const double *Wm, const double *cst, int32_t R, int32_t K, int32_t flags,
                            double *resp, double *ll_ws, double *ll, int32_t *assign, int64_t ld_assign, void *stream);
int clane_mixture_estep_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                             const float *mean, const float *Wm, const float *cst, int32_t R, int32_t K, int32_t flags,
                             float *resp, double *ll_ws, double *ll, int32_t *assign, int64_t ld_assign, void *stream);
int clane_mixture_mstep_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                            const float *mean, const float *resp, int32_t K, float *ws, float *S, float *nk, void *stream);
int clane_mixture_mstep_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                            const double *mean, const double *resp, int32_t K, double *ws, double *S, double *nk,
                            void *stream);
int clane_mixture_mstep_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                             const float *mean, const float *resp, int32_t K, float *ws, float *S, float *nk, void *stream);
int64_t clane_mixture_ll_ws_len(int64_t n, int32_t R);
int64_t clane_mixture_mstep_ws_len(int64_t n, int32_t K, int32_t d);

/* ---- node clustering (csrc/kmeans.h) ----------------------------------------------------------------------------------
 * One Lloyd iteration of k-means for R restarts at once on the rows `rows[0..n)` of the table Z (an index outside
 * [0, table_rows) reads as a zero row).  centres [R, K, d] and csq [R, K] = |c|^2 in the accumulate type, R, K >= 1.
 *
 * assign: assign[i, r] = argmin_j (csq[r, j] - 2 z_i . c[r, j]) (int32, [n, ld_assign >= R]), value ascending, ties to the
 *   lowest centre; best[i, r] = that minimum (accumulate type, [n, ld_best >= R]) -- the squared distance without |z_i|^2,
 *   which the caller adds.  The n x K distances never reach memory.  R <= 65535.
 * update: order [R n] (int32): for each restart in turn the n TABLE ROWS of its list sorted by assigned centre (stably: a
 *   centre's rows in list order); seg [R K + 1] (int64): segment offsets into order, non-decreasing, seg[R K] = R n.
 *   centres_new[r, j] = (sum of segment r K + j's rows) / count -- the sum in a fixed order, one IEEE division -- or
 *   centres_old[r, j], bit for bit, where the segment is empty; csq_new[r, j] = |centres_new[r, j]|^2.
 *   ws: clane_kmeans_update_ws_len(n, R, K, d) elements of the accumulate type.
 * No atomics: two calls give the same bits, and a restart's results do not depend on the other restarts of the call. */
int clane_kmeans_assign_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                            const float *centres, const float *csq, int32_t R, int32_t K, int32_t *assign,
                            int64_t ld_assign, float *best, int64_t ld_best, void *stream);
int clane_kmeans_assign_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                            const double *centres, const double *csq, int32_t R, int32_t K, int32_t *assign,
                            int64_t ld_assign, double *best, int64_t ld_best, void *stream);
int clane_kmeans_assign_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                             const float *centres, const float *csq, int32_t R, int32_t K, int32_t *assign,
                             int64_t ld_assign, float *best, int64_t ld_best, void *stream);
int clane_kmeans_update_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order,
                            const int64_t *seg, int64_t n, int32_t R, int32_t K, const float *centres_old, float *ws,
                            float *centres_new, float *csq_new, void *stream);
int clane_kmeans_update_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order,
                            const int64_t *seg, int64_t n, int32_t R, int32_t K, const double *centres_old, double *ws,
                            double *centres_new, double *csq_new, void *stream);
int clane_kmeans_update_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order,
                             const int64_t *seg, int64_t n, int32_t R, int32_t K, const float *centres_old, float *ws,
                             float *centres_new, float *csq_new, void *stream);
int64_t clane_kmeans_update_ws_len(int64_t n, int32_t R, int32_t K, int32_t d);

/* ---- new vertices against a finished table (csrc/new_rows.h) ------------------------------------------------------------
 * A vertex that was not in V, with content x and out-edges to EXISTING vertices only: nothing reads it, so Graph.build_P
 * (graph.py:118-128) followed by the update of propagate (embedder.py:84-92), restricted to that row on a table that is
 * held fixed, is the per-row fixed point  z <- x + gamma * sum_v softmax_v(score(z, z_v)) z_v,  v in nbrs, z^0 = x.
 * One launch embeds m such rows; each iterates and stops on its own.
 *   rowptr (int64 [m + 1]) / colidx (int32): the new rows' neighbours as TABLE ROWS of Z (not checked here:
 *     clane_check_csr); a repeated neighbour counts as often as it is listed.
 *   X_new [m, ldx], Z [table_rows, ldz], Z_out [m, ldo] in the table type; only columns [0, d) are read, Z_out's columns
 *     [d, ldo) are written as zeros.
 *   Score, with z the iterate in the accumulate type:
 *     S == NULL, mode REFERENCE: z . z_v / sqrt(sums2[0] sums2[1]);  PER_EDGE: z . z_v / (|z| sqrt(sq[v])), |z| recomputed
 *       from the iterate every round.  sums2 / sq are the EXISTING graph's (clane_degree_weighted_sums_*,
 *       clane_row_sqnorm_*): the table is frozen, the new edges are NOT counted into the global denominator.
 *     S != NULL (accumulate type, [table_rows, lds]), mode RAW_DOT: z . S_v -- the bilinear (Phi_src z) . (Phi_dst z_v)
 *       with S = Z M^T, M = Phi_src.weight^T Phi_dst.weight (the first d columns of clane_project_rows_* with M stacked
 *       on zeros).  Values always come from Z.
 *   A round is one pass over the row's neighbours with an online soft-max.  Stop rule, the reference's Tolerence per row:
 *     a round whose delta = sum |z_new - z| is a new minimum of the row resets the counter to `tolerence`, any other round
 *     decrements it; the row ends at counter 0, after max_rounds rounds, or at delta == 0.
 *   rounds (int32 [m]): rounds run, 0 for a row without neighbours, which returns x (embedder.py:88-89);
 *   delta ([m], accumulate type): the last round's; P_out ([rowptr[m]], accumulate type, or NULL): the soft-max weights
 *   that produced the returned z, in colidx order.  z is rounded to the table type once, on the store.
 *   flags: 0.  d beyond 64 packs per row (vector layout) is kept in LDS: at most 2048 (f32, bf16) / 1024 (f64) columns.
 * No allocation, no synchronisation, no atomics on memory; a row's results do not depend on where it sits in the batch
 * or on what else is in it, and two calls give the same bits. */
int clane_embed_rows_f32(const int64_t *rowptr, const int32_t *colidx, int64_t m, const float *X_new, int64_t ldx,
                         const float *Z, int64_t table_rows, int64_t ldz, int32_t d, int32_t mode, const double *sums2,
                         const float *sq, const float *S, int64_t lds, float gamma, int32_t tolerence,
                         int32_t max_rounds, int32_t flags, float *Z_out, int64_t ldo, int32_t *rounds, float *delta,
                         float *P_out, void *stream);
int clane_embed_rows_f64(const int64_t *rowptr, const int32_t *colidx, int64_t m, const double *X_new, int64_t ldx,
                         const double *Z, int64_t table_rows, int64_t ldz, int32_t d, int32_t mode, const double *sums2,
                         const double *sq, const double *S, int64_t lds, double gamma, int32_t tolerence,
                         int32_t max_rounds, int32_t flags, double *Z_out, int64_t ldo, int32_t *rounds, double *delta,
                         double *P_out, void *stream);
int clane_embed_rows_bf16(const int64_t *rowptr, const int32_t *colidx, int64_t m, const uint16_t *X_new, int64_t ldx,
                          const uint16_t *Z, int64_t table_rows, int64_t ldz, int32_t d, int32_t mode,
                          const double *sums2, const float *sq, const float *S, int64_t lds, float gamma,
                          int32_t tolerence, int32_t max_rounds, int32_t flags, uint16_t *Z_out, int64_t ldo,
                          int32_t *rounds, float *delta, float *P_out, void *stream);

/* ---- content reduction (csrc/content_pca.h) -----------------------------------------------------------------------------
 * The device passes of a PCA on the rows `rows[0..n)` of the table Z [table_rows, ldz >= d].  The same calls serve a plain
 * [n, d] matrix (rows = 0 .. n - 1) and an engine's permuted, padded table.  A rows entry outside [0, table_rows) is an
 * ABSENT row: nothing is read for it, it adds nothing to the sums or the Gram, and its Y row is zeros.  Columns [d, ldz)
 * are never read.  mu [d] (accumulate type) may be NULL: no centring.  flags: 0 or CLANE_PCA_ACCUMULATE.
 *
 * column_sums: sums[c] = sum_i Z[rows[i], c], in double.  Rows are taken in chunks of 2048: inside a chunk thread t of 16
 *   adds rows t, t + 16, .. in row order and the 16 threads are added in thread order; the chunks' partials are added in
 *   chunk order, starting from 0 or, with CLANE_PCA_ACCUMULATE, from the value already in sums -- so streaming a matrix
 *   in blocks of a multiple of 2048 rows gives the bits of one call.  16-byte loads where Z and ldz allow them, single
 *   elements otherwise: the same bits.  ws: clane_column_sums_ws_len(n, d) doubles.
 * gram: G [d, d] contiguous (accumulate type) = sum_i (z_i - mu)(z_i - mu)^T, z - mu[col] formed in the accumulate type
 *   by one subtraction.  Only the 128 x 128 tile pairs (ti <= tj) are computed, per chunk of 2048 rows; the chunks'
 *   partials are added in chunk order (from 0, or from G with CLANE_PCA_ACCUMULATE, which must then be symmetric) and the
 *   element of an off-diagonal pair is also written to G[j, i].  A (row, column) element's k terms run in the order of
 *   the library's one tile contraction (mfma_slice) inside a chunk: on the same operands G has the bits of
 *   clane_probe_grad_* called with its G = the centred rows ([n, d], accumulate type), its table = the same rows and
 *   K = d.  G is bitwise symmetric.  ws: clane_gram_ws_len(n, d) elements of the accumulate type.
 * project_affine: Y[i, 0:m) = W (z_rows[i] - mu), W [m, d] contiguous (accumulate type), Y [n, ldy >= m] in the TABLE
 *   type, rounded once on the store; columns [m, ldy) of Y are not written.  On the same operands the accumulated value
 *   has the bits of clane_project_rows_* on the centred table.
 * No allocation, no synchronisation, no atomics on memory; two calls give the same bits. */
#define CLANE_PCA_ACCUMULATE 1
int clane_column_sums_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                          int32_t flags, double *ws, double *sums, void *stream);
int clane_column_sums_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                          int32_t flags, double *ws, double *sums, void *stream);
int clane_column_sums_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                           int32_t flags, double *ws, double *sums, void *stream);
int64_t clane_column_sums_ws_len(int64_t n, int32_t d);
int clane_gram_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                   const float *mu, int32_t flags, float *ws, float *G, void *stream);
int clane_gram_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                   const double *mu, int32_t flags, double *ws, double *G, void *stream);
int clane_gram_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                    const float *mu, int32_t flags, float *ws, float *G, void *stream);
int64_t clane_gram_ws_len(int64_t n, int32_t d);
int clane_project_affine_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                             const float *mu, const float *W, int32_t m, float *Y, int64_t ldy, void *stream);
int clane_project_affine_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                             const double *mu, const double *W, int32_t m, double *Y, int64_t ldy, void *stream);
int clane_project_affine_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows,
                              int64_t n, const float *mu, const float *W, int32_t m, uint16_t *Y, int64_t ldy,
                              void *stream);

/* ---- sparse rows (csrc/sparse_rows.h) -----------------------------------------------------------------------------------
 * A CSR matrix of n_rows rows and nnz non-zeros: rowptr int64 [n_rows + 1] (rowptr[0] may be any offset into col / val: a
 * slice of another matrix's rowptr describes a sub-matrix), col int32 (rows of B, in [0, b_rows): NOT checked here, the
 * caller validates), val fp32.  n_rows and b_rows are below 2^31.
 *
 * csr_spmm: out[r, 0:l) = sum_e val[e] B[col[e], 0:l) - a[r] s[0:l), e in [rowptr[r], rowptr[r + 1]).  a NULL: a[r] = 1;
 *   s NULL: no epilogue.  B [b_rows, ldb >= l], out [n_rows, ldo >= l]; columns past l are never read or written.  l is a
 *   multiple of 4 in [4, CLANE_CSR_MAX_L]; B, out, s and ws 16-byte aligned, ldb and ldo multiples of 4.
 * A row of more than CLANE_CSR_SEGMENT (= clane_csr_spmm_segment()) non-zeros is cut into segments of that length (the
 *   last one shorter), listed by the caller: long_rows int32 [n_long] the long rows ascending, seg_ptr int64 [n_long + 1]
 *   the prefix sums of their segment counts ceil(len / segment), item_long int32 [n_items] the index into long_rows of
 *   every segment (n_items = seg_ptr[n_long]).  Segments write partial sums to ws (n_items * l floats, at most
 *   clane_csr_spmm_ws_len(n_rows, nnz, l)); a second kernel adds them in segment order and applies the epilogue.
 * Order of every element's sum: inside a segment (a short row is one) the wave's EPW sub-waves (EPW = 4 for l <= 64, 2
 *   for l <= 128, else 1) each add the non-zeros k = sub, sub + EPW, .. of the segment in ascending k by one fmaf onto +0;
 *   the sub-wave sums are folded (s0 + s2) + (s1 + s3) resp. s0 + s1; segments are added in order onto the first one;
 *   the epilogue is one fmaf(-a[r], s[c], sum).  The bits of a row depend on the row and on l alone: not on the grid,
 *   not on the other rows of the call.
 * csr_row_sums: sums[r] (double) = the sum of the row's values: lane t of 64 adds a segment's values t, t + 64, .. in
 *   order, the lanes are folded by the xor butterfly (32, 16, .., 1), segments are added in order.  ws: n_items doubles.
 * No allocation, no synchronisation, no atomics on memory; two calls give the same bits. */
#define CLANE_CSR_SEGMENT 2048
#define CLANE_CSR_MAX_L 512
int clane_csr_spmm_segment(void);
int64_t clane_csr_spmm_ws_len(int64_t n_rows, int64_t nnz, int32_t l);
int clane_csr_spmm_f32(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows, int64_t nnz,
                       const float *B, int64_t b_rows, int64_t ldb, int32_t l, const float *a, const float *s,
                       const int32_t *long_rows, const int64_t *seg_ptr, const int32_t *item_long, int64_t n_long,
                       int64_t n_items, float *ws, int64_t ws_len, float *out, int64_t ldo, void *stream);
int clane_csr_row_sums_f32(const int64_t *rowptr, const float *val, int64_t n_rows, int64_t nnz, const int32_t *long_rows,
                           const int64_t *seg_ptr, const int32_t *item_long, int64_t n_long, int64_t n_items, double *ws,
                           int64_t ws_len, double *sums, void *stream);

/* ---- 2-D layout: exact t-SNE (csrc/tsne.h) ------------------------------------------------------------------------------
 * The formulas are scikit-learn's TSNE(method="exact"); n points, 2 <= n <= CLANE_TSNE_MAX_POINTS; D / P [n, n] fp32
 * contiguous; Y, V, G [n, 2] fp32 contiguous.  A fit calls them in this order.  No allocation, no synchronisation, no
 * atomics; the order of every sum is a function of n alone: two calls give the same bits.
 *
 * tsne_sqdist: D[i, j] = max(0, |a_i|^2 + |a_j|^2 - 2 a_i . a_j), a_i = Z[rows[i], 0:d) - mu formed by one fp32
 *   subtraction (a `rows` entry outside [0, table_rows) is the row z = 0); mu [d] fp32, the caller's column mean of the
 *   listed rows (clane_column_sums_*).  |a|^2 is one fmaf per k in k order (sq [n] fp32: workspace, left filled); the
 *   dots run in the order of the library's one tile contraction (mfma_slice).  Only the 128 x 128 tile pairs ti <= tj are
 *   computed and each value is written to D[i, j] and D[j, i]: D is bitwise symmetric, its diagonal exactly 0.
 * tsne_affinities: in place, row i of D becomes p_{j|i} = exp(-beta_i (D_ij - min_j D_ij)) / sum, 0 on the diagonal;
 *   beta_i by scikit-learn's _binary_search_perplexity in fp32: from 1, doubled / halved until bracketed, then bisected,
 *   at most 100 steps, until |H_i - ln(perplexity)| <= 1e-5; beta [n] = the beta_i the row was written with.  One
 *   workgroup per row: thread t of 256 adds j = t, t + 256, .. in order (fp32), the threads are added in double.
 * tsne_symmetrize: in place, P_ij = max((p_{j|i} + p_{i|j}) / 2n, 2.220446e-16), 0 on the diagonal; bitwise symmetric.
 *   partials [clane_tsne_symmetrize_ws_len(n)] doubles: sum p ln p of each pair of 64 x 64 tiles, pairs in the order
 *   (0, 0), (0, 1), .., (1, 1), ..; their sum in that order is the constant of the KL below.
 * tsne_forces: F [n, 6] fp32 = per row i, with q_ij = 1 / (1 + |y_i - y_j|^2):
 *   F[i, 0:2] = sum_j P_ij q_ij (y_i - y_j), F[i, 2:4] = sum_j q_ij^2 (y_i - y_j), F[i, 4] = sum_{j != i} q_ij and, with
 *   CLANE_TSNE_FORCES_KL, F[i, 5] = sum_j P_ij log1p(|y_i - y_j|^2) (0 without).  P is read once, Y through LDS; lane l of
 *   64 adds the columns 2048 c + 256 m + 4 l + u in (c, m, u) order, the lanes are folded by the xor butterfly.
 *   CLANE_TSNE_FORCES_CACHED: plain loads of P instead of non-temporal ones -- the same bits.
 * tsne_step: S = sum_i F[i, 4] (double; thread t of 1024 adds i = t, t + 1024, .., the threads in order),
 *   g_i = 4 (alpha F[i, 0:2] - F[i, 2:4] / S); scikit-learn's _gradient_descent per coordinate in double, stored fp32:
 *   gain += 0.2 where v g < 0, else gain *= 0.8, floor 0.01; v = momentum v - lr gain g; Y_next = Y + v.  V and G are
 *   updated in place; Y_next must not be Y.  stats [4] doubles: KL = plogp + sum_i F[i, 5] + ln S (plogp: the sum of
 *   tsne_symmetrize's partials; valid at alpha = 1 and when the forces were taken with CLANE_TSNE_FORCES_KL), |g|, S,
 *   sum_i F[i, 5].  tsne_step alone takes n up to CLANE_TSNE_NN_MAX_POINTS: the neighbour-sparse path below shares it. */
#define CLANE_TSNE_MAX_POINTS 65536
#define CLANE_TSNE_FORCES_KL 1
#define CLANE_TSNE_FORCES_CACHED 2
int clane_tsne_sqdist_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                          const float *mu, float *sq, float *D, void *stream);
int clane_tsne_sqdist_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                           const float *mu, float *sq, float *D, void *stream);
int clane_tsne_affinities_f32(float *D, int64_t n, float perplexity, float *beta, void *stream);
int64_t clane_tsne_symmetrize_ws_len(int64_t n);
int clane_tsne_symmetrize_f32(float *P, int64_t n, double *partials, void *stream);
int clane_tsne_forces_f32(const float *P, const float *Y, int64_t n, int32_t flags, float *F, void *stream);
int clane_tsne_step_f32(const float *F, const float *Y, int64_t n, double alpha, double momentum, double lr, double plogp,
                        float *V, float *G, float *Y_next, double *stats, void *stream);

/* ---- neighbour-sparse 2-D layout (csrc/tsne_nn.h) ---------------------------------------------------------------------------
 * t-SNE with P kept on every point's k nearest neighbours and the repulsion exact: nothing is n x n, 2 <= n <=
 * CLANE_TSNE_NN_MAX_POINTS.  No allocation, no synchronisation, no atomics; the order of every sum is a function of n (and
 * of k, or of the CSR) alone: two calls give the same bits.
 *
 * knn_sqdist: for every listed row i its k nearest OTHER listed rows: ids [n, k] int32 -- positions in `rows` -- and
 *   sqdist [n, k] fp32, by distance ascending, ties by position ascending.  The distances are tsne_sqdist's own (the same
 *   centring, norms, contraction and expression): sqdist[i, r] is bit for bit D[i, ids[i, r]] of the exact path.  Places
 *   past the n - 1 other rows hold id -1 and +inf.  1 <= k <= CLANE_KNN_MAX_K.  sq [n] fp32: workspace, left filled with
 *   the squared norms.  The candidate positions are cut into n_slabs slabs of whole 128-position tiles, each slab's lists
 *   go to cand_sqdist / cand_ids [n, n_slabs, k] and a merge kernel combines them (n_slabs = 1: neither is read and both
 *   may be null); the result does not depend on n_slabs.  A workgroup keeps the lists of 128 (k <= 40), 64 (k <= 96) or
 *   32 queries in LDS.
 * tsne_nn_affinities: tsne_affinities' perplexity search over the k distances of every row (the same steps, tolerance,
 *   shift by the row's minimum, fp32 partials added in double): p [n, k] the conditionals, 0 where ids < 0; beta [n].
 *   One wave per row: lane l adds the places l, l + 64, l + 128 in order, the lanes by the xor butterfly.
 *   0 < perplexity < k.
 * tsne_nn_plogp: row_plogp[i] (double) = sum p ln p over row i of a CSR (rowptr int64 [n + 1], val fp32 [nnz]): lane l of
 *   the row's wave adds the entries l, l + 64, .. in column order, the lanes by the xor butterfly.
 * tsne_nn_attract: F[i, 0:2] = sum_j P_ij q_ij (y_i - y_j) over the entries of CSR row i (cols int32, a column outside
 *   [0, n) is skipped) and, with CLANE_TSNE_FORCES_KL, F[i, 5] = sum_j P_ij log1p(|y_i - y_j|^2) (0 without); the other
 *   columns of F [n, 6] are left alone.  One wave per row however long, in the order of tsne_nn_plogp.
 * tsne_repulse: F[i, 2:4] = sum_j q_ij^2 (y_i - y_j), F[i, 4] = sum_{j != i} q_ij over ALL j, Y through LDS, in
 *   tsne_forces' order; the other columns are left alone.  attract + repulse fill what tsne_step reads. */
#define CLANE_KNN_MAX_K 192
#define CLANE_TSNE_NN_MAX_POINTS 1048576
int clane_knn_sqdist_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                         const float *mu, float *sq, int32_t k, int32_t n_slabs, float *cand_sqdist, int32_t *cand_ids,
                         float *sqdist, int32_t *ids, void *stream);
int clane_knn_sqdist_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *rows, int64_t n,
                          const float *mu, float *sq, int32_t k, int32_t n_slabs, float *cand_sqdist, int32_t *cand_ids,
                          float *sqdist, int32_t *ids, void *stream);
int clane_tsne_nn_affinities_f32(const float *sqdist, const int32_t *ids, int64_t n, int32_t k, float perplexity, float *p,
                                 float *beta, void *stream);
int clane_tsne_nn_plogp_f32(const int64_t *rowptr, const float *val, int64_t n, int64_t nnz, double *row_plogp,
                            void *stream);
int clane_tsne_nn_attract_f32(const int64_t *rowptr, const int32_t *cols, const float *val, const float *Y, int64_t n,
                              int64_t nnz, int32_t flags, float *F, void *stream);
int clane_tsne_repulse_f32(const float *Y, int64_t n, float *F, void *stream);

/* ---- silhouette of a partition (csrc/silhouette.h) -------------------------------------------------------------------------
 * order [n] int32: table rows grouped by cluster; seg [K + 1] int64: cluster c is the positions [seg[c], seg[c + 1]) of
 * `order` (clamped to [0, n]; an empty cluster is an empty range).  a_p = Z[order[p], 0:d) - mu, one subtraction in the
 * accumulate type (fp32 for the _f32 and _bf16 tables, fp64 for _f64); an `order` entry outside [0, table_rows) is the row
 * z = 0.  mu [d]: the caller's column mean for CLANE_SILHOUETTE_EUCLIDEAN (any shift leaves the distances unchanged and
 * keeps the Gram trick's cancellation small), zeros for CLANE_SILHOUETTE_COSINE.  No allocation, no synchronisation, no
 * atomics.
 *
 * silhouette_norms: nrm [n], accumulate type.  euclidean: |a_p|^2; cosine: 1 / sqrt(|a_p|^2), 0 for a zero row.  |a_p|^2 is
 *   the dot a_p . a_p in the order of the library's one tile contraction (mfma_slice) -- the chain a_p . a_j runs through.
 * silhouette_sums: S [p1 - p0, K] doubles, S[p - p0, c] = sum over j in cluster c of dist(p, j) for the positions p in
 *   [p0, p1) -- the caller walks the positions in blocks, S is as large as a block.  nrm: what silhouette_norms left for
 *   the same order, mu and metric.
 *     euclidean: dist = sqrt(max(0, fma(-2, a_p . a_j, nrm_p + nrm_j))), the square root correctly rounded.  Two positions
 *       whose table rows hold the same bits are at distance exactly 0.
 *     cosine:    dist = max(0, 1 - ((a_p . a_j) nrm_p) nrm_j): a zero row is at distance 1 from every other position.
 *   The term j == p is exactly 0.  An empty cluster's column is zeros.  Order of a sum: with q = j - seg[c], partial
 *   (h, l) = ((q % 128) / 64, q % 16) adds its distances in double in ascending q; the 16 partials of one h are folded by the
 *   xor butterfly over l (8, 4, 2, 1), the result is fold(0) + fold(1) -- a function of seg alone: S[p, c] has the same bits
 *   for every [p0, p1) that holds p, and in every call. */
#define CLANE_SILHOUETTE_EUCLIDEAN 0
#define CLANE_SILHOUETTE_COSINE 1
int clane_silhouette_norms_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order, int64_t n,
                               const float *mu, int32_t metric, float *nrm, void *stream);
int clane_silhouette_norms_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order, int64_t n,
                               const double *mu, int32_t metric, double *nrm, void *stream);
int clane_silhouette_norms_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order,
                                int64_t n, const float *mu, int32_t metric, float *nrm, void *stream);
int clane_silhouette_sums_f32(const float *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order, int64_t n,
                              const int64_t *seg, int32_t K, const float *mu, const float *nrm, int32_t metric, int64_t p0,
                              int64_t p1, double *S, void *stream);
int clane_silhouette_sums_f64(const double *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order, int64_t n,
                              const int64_t *seg, int32_t K, const double *mu, const double *nrm, int32_t metric,
                              int64_t p0, int64_t p1, double *S, void *stream);
int clane_silhouette_sums_bf16(const uint16_t *Z, int64_t table_rows, int32_t d, int64_t ldz, const int32_t *order,
                               int64_t n, const int64_t *seg, int32_t K, const float *mu, const float *nrm, int32_t metric,
                               int64_t p0, int64_t p1, double *S, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CLANE_HIP_H_ */
