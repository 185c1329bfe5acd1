// Embedding NEW vertices against a finished table -- the reference's loop restricted to rows nobody reads.
//
// A new vertex u has content x_u and out-edges to EXISTING vertices only; no row of the table reads u.  Graph.build_P
// (clane/graph.py:118-128) followed by the update of IterativeEmbedder.propagate (clane/embedder.py:84-92), restricted
// to row u with the table held fixed, is the per-row fixed point
//     z  <-  x_u + gamma * sum_v softmax_v( score(z, z_v) ) z_v ,     v in nbrs(u),  z^0 = x_u .
// With P frozen a second inner sweep of propagate() changes nothing, so the outer rounds are the whole iteration.
//
// FROZEN means: the table Z, its norms `sq` and, in reference cosine mode, the two global Frobenius sums `sums2`
// (similarity.py:37) are the EXISTING graph's.  The new edges are not counted into the global denominator and no
// existing row moves.  Only the source norm |z| of the per-edge cosine follows the iterate: it is recomputed from z every
// round (K0's order: one fma per element, the butterfly over the row's lanes).
//
// One launch embeds a batch.  The lane layout is the row kernels' (Pack / LPR lanes per row): a SUB-WAVE of LPR lanes
// owns one row at a time and claims rows from the workgroup's LDS counter, as K1 / K3 do; rows have ragged degrees
// and stop at different rounds.  (The sub-waves of a wave claim together, once per turn of a wave-uniform loop: a
// sub-wave that is done with its row waits for the slowest of its wave -- nothing at 64 lanes per row.)  A round is ONE
// pass over the neighbours with an online soft-max, a group of U neighbours at a time:
//   1. U neighbour rows are loaded (their columns from a buffered chunk of LPR edges, one per lane);
//   2. their dots with z are reduced together (transpose_reduce8, or group_sum on the scalar layouts), finished exactly
//      as finalize_score() does, and handed to every lane of the sub-wave;
//   3. running max / sum are updated, the accumulator rescaled, and the SAME rows added from the registers they are
//      still in, weighted exp(score - max);
//   4. after the last group: z_new = x + gamma * acc / sum, delta = sum |z_new - z|.
// z lives in the accumulate type between rounds and is rounded to T once, on the final store.
//
// Rows of more than one pack per lane (d > 64 * VEC; WIDE instances, one wave per row) keep z and the accumulator in
// lane-private LDS slots instead of registers and read a group's rows a second time for step 3 (an L1 hit: the group
// was loaded a few hundred cycles earlier).
//
// Bilinear score (PAIR): (Phi_src z) . (Phi_dst z_v) = z . (M z_v),  M = Phi_src.weight^T Phi_dst.weight.  The host
// projects the table once, S = Z M^T (accumulate type), and the kernel takes score rows from S, value rows from Z.
//
// Stop rule -- the reference's Tolerence (embedder.py:45-56, 60-69) applied per row: a round whose delta is a new
// minimum for the row resets the counter to `tolerence`, any other round decrements it; the row ends when the counter
// reaches 0, after max_rounds rounds, or at a delta of exactly 0 (the iterate reproduces itself bit for bit from there
// on, so stopping changes no result).  A row without neighbours returns x with rounds = 0 (embedder.py:88-89).
// Zero norms get no special case: NaN scores propagate, as in K1.
//
// No atomics on memory, no cross-row arithmetic: a row's Z_out / rounds / delta / P_out depend on the row alone -- not on
// where it sits in the batch nor on what else is in it.
#pragma once

#include "device_utils.h"
#include "edge_score.h"

namespace clane {

// Bytes of LDS one wave of a WIDE instance may use for z and the accumulator (4 waves: the 64 KiB a launch gets without
// asking for more).
constexpr int kEmbedWideLdsPerWave = 16384;

template <typename T, int VEC, int LPR, int U, bool PAIR, bool WIDE>
__global__ __launch_bounds__(kBlock) void embed_rows_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t m, const T *__restrict__ X,
    int64_t ldx, const T *__restrict__ Z, int64_t ldz, int d, int mode, const double *__restrict__ sums2,
    const typename Elem<T>::acc_t *__restrict__ sq, const typename Elem<T>::acc_t *__restrict__ S, int64_t lds,
    typename Elem<T>::acc_t gamma, int tolerence, int max_rounds, T *__restrict__ Z_out, int64_t ldo,
    int32_t *__restrict__ rounds_out, typename Elem<T>::acc_t *__restrict__ delta_out,
    typename Elem<T>::acc_t *P_out, int rows_per_block, int dpad) {
    using A = typename Elem<T>::acc_t;
    static_assert(!WIDE || LPR == kWave, "wide rows take a whole wave");
    static_assert(LPR % U == 0, "a chunk of LPR edges is whole groups");
    constexpr bool kTransposed = (U == 8 && LPR >= 8);
    constexpr int W = LPR * VEC;             // columns a sub-wave covers per tile
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ int s_next;
    const int lane = lane_id();
    const int sub = lane / LPR, sl = lane % LPR, sub_base = sub * LPR;
    const int64_t row_begin = int64_t(blockIdx.x) * rows_per_block;
    const int nb = int((row_begin + rows_per_block < m ? row_begin + rows_per_block : m) - row_begin);
    const A D = global_denominator<A>(mode, sums2);
    const int c0 = sl * VEC;
    const int c0s = c0 < d ? c0 : 0;         // lanes past the row read column 0 and keep zeros
    const int ntiles = WIDE ? dpad / W : 1;
    // WIDE: this wave's z and accumulator, element (t, sl, k) at t * W + sl * VEC + k -- every slot private to one lane
    A *zl = nullptr, *al = nullptr;
    if constexpr (WIDE) {
        zl = reinterpret_cast<A *>(s_dyn) + int64_t(threadIdx.x / kWave) * 2 * dpad;
        al = zl + dpad;
    }
    // the lane that holds finished score u of a group after the reduction, and which one it holds
    const bool server = kTransposed ? (sl % (LPR / 8) == 0) : (sl < U);
    const int u_serve = kTransposed ? sl / (LPR / 8) : sl % U;

    if (threadIdx.x == 0) s_next = 0;
    __syncthreads();

    // The claim loop is WAVE-uniform: all 64 lanes meet at its head every turn and leave together, once no sub-wave got a
    // row (a scalar branch on a ballot, as K1's sub-row kernel leaves on __all(done)).  A loop that each sub-wave left on
    // its own, with the leader's stores as the last thing in its body, was split by the compiler into one loop for the
    // leaders and one for the other lanes: those ran ahead, read the claim of a leader that was masked off (0) and
    // embedded row 0 for ever.  Inside a turn the sub-waves diverge freely; no lane-divergent branch ends a loop body.
    for (;;) {
        int claimed = 0;
        if (sl == 0) claimed = atomicAdd(&s_next, 1);
        const int row = lane_get(claimed, sub_base);
        const bool has_row = row < nb;
        if (!__any(has_row)) break;
        if (has_row) {
            const int64_t r = row_begin + row;
            const int64_t e0 = rowptr[r];
            const int64_t deg = rowptr[r + 1] - e0;
            const T *xr = X + r * ldx;
            T *zo = Z_out + r * ldo;

            A x[VEC], z[VEC];                     // !WIDE: the row's content and the iterate
#pragma unroll
            for (int k = 0; k < VEC; ++k) x[k] = z[k] = A(0);
            if constexpr (WIDE) {
                for (int t = 0; t < ntiles; ++t) {
                    const int c = t * W + c0;
                    Pack<T, VEC> p{};
                    if (c < d) p = load_pack<T, VEC>(xr + c);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) zl[c + k] = (c + k < d) ? Elem<T>::to_acc(p.v[k]) : A(0);
                }
            } else {
                Pack<T, VEC> p{};
                if (c0 < d) p = load_pack<T, VEC>(xr + c0);
#pragma unroll
                for (int k = 0; k < VEC; ++k) x[k] = z[k] = (c0 + k < d) ? Elem<T>::to_acc(p.v[k]) : A(0);
            }

            int rounds = 0, left = tolerence;
            A delta = A(0), best = A(INFINITY), run_m = -A(INFINITY), run_s = A(0);
            while (deg > 0) {
                // |z| of the per-edge cosine, from the iterate (K0's order)
                A nsrc = A(0);
                if (mode == kScorePerEdge) {
                    A q = A(0);
                    if constexpr (WIDE) {
                        for (int t = 0; t < ntiles; ++t) {
#pragma unroll
                            for (int k = 0; k < VEC; ++k) {
                                const A v = zl[t * W + c0 + k];
                                q = fma(v, v, q);
                            }
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < VEC; ++k) q = fma(z[k], z[k], q);
                    }
                    nsrc = sqrt(group_sum<LPR>(q));
                }
                run_m = -A(INFINITY);
                run_s = A(0);
                A acc[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = A(0);
                if constexpr (WIDE) {
                    for (int t = 0; t < ntiles; ++t) {
#pragma unroll
                        for (int k = 0; k < VEC; ++k) al[t * W + c0 + k] = A(0);
                    }
                }

                for (int64_t eb = 0; eb < deg; eb += LPR) {
                    const int n = deg - eb < LPR ? int(deg - eb) : LPR;
                    int c = 0;
                    if (sl < n) c = colidx[e0 + eb + sl];
                    c = sl < n ? c : lane_get(c, sub_base);          // lanes past the row: the chunk's first column
                    for (int j = 0; j < n; j += U) {
                        int cj[U];
                        A part[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            cj[u] = lane_get(c, sub_base + j + u);
                            part[u] = A(0);
                        }
                        Pack<T, VEC> zp[U];       // !WIDE: the group's value rows, kept for step 3
                        if constexpr (WIDE) {
                            for (int t = 0; t < ntiles; ++t) {
                                const int ct = t * W + c0;
                                const int cts = ct < d ? ct : 0;     // zl is zero there
                                if constexpr (PAIR) {
                                    Pack<A, VEC> sp[U];
#pragma unroll
                                    for (int u = 0; u < U; ++u) sp[u] = load_pack<A, VEC>(S + int64_t(cj[u]) * lds + cts);
#pragma unroll
                                    for (int u = 0; u < U; ++u) {
#pragma unroll
                                        for (int k = 0; k < VEC; ++k) part[u] = fma(zl[ct + k], sp[u].v[k], part[u]);
                                    }
                                } else {
                                    Pack<T, VEC> zt[U];
#pragma unroll
                                    for (int u = 0; u < U; ++u) zt[u] = load_pack<T, VEC>(Z + int64_t(cj[u]) * ldz + cts);
#pragma unroll
                                    for (int u = 0; u < U; ++u) {
#pragma unroll
                                        for (int k = 0; k < VEC; ++k)
                                            part[u] = fma(zl[ct + k], Elem<T>::to_acc(zt[u].v[k]), part[u]);
                                    }
                                }
                            }
                        } else {
#pragma unroll
                            for (int u = 0; u < U; ++u) zp[u] = load_pack<T, VEC>(Z + int64_t(cj[u]) * ldz + c0s);
                            if constexpr (PAIR) {
                                Pack<A, VEC> sp[U];
#pragma unroll
                                for (int u = 0; u < U; ++u) sp[u] = load_pack<A, VEC>(S + int64_t(cj[u]) * lds + c0s);
#pragma unroll
                                for (int u = 0; u < U; ++u) {
#pragma unroll
                                    for (int k = 0; k < VEC; ++k) part[u] = fma(z[k], sp[u].v[k], part[u]);
                                }
                            } else {
#pragma unroll
                                for (int u = 0; u < U; ++u) {
#pragma unroll
                                    for (int k = 0; k < VEC; ++k)
                                        part[u] = fma(z[k], Elem<T>::to_acc(zp[u].v[k]), part[u]);
                                }
                            }
                        }
                        // the U dots, finished as K1 finishes them, then handed to every lane of the sub-wave
                        A serve;
                        if constexpr (kTransposed) {
                            serve = transpose_reduce8<LPR>(part, sl);
                        } else {
                            serve = A(0);
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                const A dot = group_sum<LPR>(part[u]);
                                if (u == u_serve) serve = dot;
                            }
                        }
                        int col_serve = 0;
                        if (mode == kScorePerEdge) col_serve = lane_get(c, sub_base + j + u_serve);
                        serve = finalize_score<A>(serve, mode, D, nsrc, sq, col_serve);
                        if (P_out != nullptr && server && j + u_serve < n)
                            P_out[e0 + eb + j + u_serve] = serve;                   // raw; rescaled after the last round
                        A sc[U];
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            sc[u] = lane_get(serve, sub_base + (kTransposed ? u * (LPR / 8) : u));
                        A new_m = run_m;
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            if (j + u < n) new_m = fmax(new_m, sc[u]);
                        const A scale = exp_acc<A>(run_m - new_m);   // first group: exp(-inf) = 0 on a zero accumulator
                        A w[U];
                        run_s *= scale;
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            w[u] = (j + u < n) ? exp_acc<A>(sc[u] - new_m) : A(0);
                            run_s += w[u];
                        }
                        run_m = new_m;
                        if constexpr (WIDE) {
                            for (int t = 0; t < ntiles; ++t) {
                                const int ct = t * W + c0;
                                if (ct >= d) continue;
                                Pack<T, VEC> zt[U];
#pragma unroll
                                for (int u = 0; u < U; ++u) zt[u] = load_pack<T, VEC>(Z + int64_t(cj[u]) * ldz + ct);
#pragma unroll
                                for (int k = 0; k < VEC; ++k) {
                                    A a = al[ct + k] * scale;
#pragma unroll
                                    for (int u = 0; u < U; ++u) a = fma(w[u], Elem<T>::to_acc(zt[u].v[k]), a);
                                    al[ct + k] = a;
                                }
                            }
                        } else {
#pragma unroll
                            for (int k = 0; k < VEC; ++k) {
                                A a = acc[k] * scale;
#pragma unroll
                                for (int u = 0; u < U; ++u) a = fma(w[u], Elem<T>::to_acc(zp[u].v[k]), a);
                                acc[k] = a;
                            }
                        }
                    }
                }
                // z_new = x + gamma * acc / sum (embedder.py:92), delta against z
                A dl = A(0);
                if constexpr (WIDE) {
                    for (int t = 0; t < ntiles; ++t) {
                        const int ct = t * W + c0;
                        if (ct >= d) continue;
                        const Pack<T, VEC> p = load_pack<T, VEC>(xr + ct);
#pragma unroll
                        for (int k = 0; k < VEC; ++k) {
                            if (ct + k < d) {
                                const A zn = Elem<T>::to_acc(p.v[k]) + gamma * (al[ct + k] / run_s);
                                dl += fabs(zn - zl[ct + k]);
                                zl[ct + k] = zn;
                            }
                        }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        if (c0 + k < d) {
                            const A zn = x[k] + gamma * (acc[k] / run_s);
                            dl += fabs(zn - z[k]);
                            z[k] = zn;
                        }
                    }
                }
                delta = group_sum<LPR>(dl);
                ++rounds;
                if (best > delta) {               // embedder.py:62-66
                    left = tolerence;
                    best = delta;
                } else {
                    --left;
                }
                if (left == 0 || rounds >= max_rounds || delta == A(0)) break;
            }

            // the weights that produced the returned z: every serving lane rescales the raw scores it stored itself
            if (P_out != nullptr && server) {
                for (int64_t e = u_serve; e < deg; e += U) P_out[e0 + e] = exp_acc<A>(P_out[e0 + e] - run_m) / run_s;
            }
            // final store: rounded to T once, pad columns zero
            for (int64_t cc = c0; cc < ldo; cc += W) {
                if (cc + VEC <= ldo || VEC == 1) {
                    Pack<T, VEC> p;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        A v = A(0);
                        if (cc + k < d) {
                            if constexpr (WIDE) v = zl[cc + k];
                            else v = z[k];
                        }
                        p.v[k] = Elem<T>::from_acc(v);
                    }
                    store_pack<T, VEC>(zo + cc, p);
                }
            }
            rounds_out[r] = rounds;              // every lane of the sub-wave, the same bits to the same place: one write
            delta_out[r] = delta;
        }
    }
}

}  // namespace clane
