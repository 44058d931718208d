// Device code of a Sequential's training-mode forward that two units inline: gnn_train_net.hip (one launch per kernel and body: k_mlp_fwd,
// k_bn_stats, k_bn_apply, k_act_fwd) and gnn_train_small.hip (every body of a small batch in ONE persistent launch: k_train_small).  The
// persistent kernel is bit-identical to the per-body kernels because it runs THESE functions on the same rows in the same lane layout;
// what differs is where a value is read from (global memory or the workgroup's LDS copy of it) and how it is stored (plain, or
// write-through where another workgroup reads it inside the launch).  All of it is forced inline or a template: a kernel's code does not
// depend on the unit it is compiled in.  Internal, not installed.
#pragma once
#include "gnn_train.h"
#include "gnn_fused.h"            // GNN_FUSED_MAXL: k_mlp_fwd takes a Sequential of up to one layer more

namespace gnn_train GNN_INTERNAL {

// COH: the word is written by another workgroup inside this launch - an L1-bypassing (sc1) load / a write-through (sc1) store on the global
// address space (relaxed, agent scope), the two halves of the hand-off of gnn_small_common.h, arrive_and_gate.  Otherwise plain.
#define GNN_TRAIN_GLOBAL __attribute__((address_space(1)))
template <bool COH>
__device__ __forceinline__ float tload(const float *p)
{
    if constexpr (COH) return __hip_atomic_load(const_cast<GNN_TRAIN_GLOBAL float *>((const GNN_TRAIN_GLOBAL float *)p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
template <bool COH>
__device__ __forceinline__ void tstore(float *p, float v)
{
    if constexpr (COH) __hip_atomic_store((GNN_TRAIN_GLOBAL float *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// Row chunks.  Every reduction over the rows of a matrix (BatchNormalization statistics, bias / weight / gamma / beta gradients)
// is done per chunk of rows_per_block(n) rows; a chunk leaves a partial result and the partials are added in a fixed order
// (k_sum_parts, or by the consumer itself): run-to-run identical sums without float atomics.
// Thread layout of the column reductions: 256 threads = CW columns x (256 / CW) row lanes, CW = 2^cw_shift >= min(F, 32), so that
// narrow matrices (F = 14, 16) still use the whole block; rows are read four at a time (independent loads in flight).
inline int column_shift(int F) { int s = 0; while ((1 << s) < F && s < 5) ++s; return s; }

// BatchNormalization, training mode, forward statistics of the row chunk [r0, r1) for the CW columns from jb on: part[j] = chunk mean,
// part[F + j] = sum over the chunk of (x - chunk mean)^2 (two passes over the chunk's rows).  h(r, j): element (row r, column j) of the
// matrix.  s0 [256], mu [32]: LDS.  Every thread of the 256 calls it (it contains barriers).
template <bool COH, class H>
__device__ __forceinline__ void bn_chunk_stats(int F, int cw_shift, int jb, int64_t r0, int64_t r1, H h, float *part, float *s0, float *mu)
{
    const int CW = 1 << cw_shift, RL = 256 >> cw_shift;
    const int c = threadIdx.x & (CW - 1), ry = threadIdx.x >> cw_shift;
    const int j = jb + c;
    float a0 = 0.0f;
    if (j < F) {
        int64_t r = r0 + ry;
        for (; r + 3 * RL < r1; r += 4 * RL) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = h(r + q * RL, j);
#pragma unroll
            for (int q = 0; q < 4; ++q) a0 += v[q];
        }
        for (; r < r1; r += RL) a0 += h(r, j);
    }
    s0[threadIdx.x] = a0;
    __syncthreads();
    if (ry == 0) {
        for (int t = 1; t < RL; ++t) a0 += s0[t * CW + c];
        mu[c] = a0 / (float)(r1 - r0);
    }
    __syncthreads();
    const float m = mu[c];
    a0 = 0.0f;
    if (j < F) {
        int64_t r = r0 + ry;
        for (; r + 3 * RL < r1; r += 4 * RL) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = h(r + q * RL, j) - m;
#pragma unroll
            for (int q = 0; q < 4; ++q) a0 += v[q] * v[q];
        }
        for (; r < r1; r += RL) { const float dv = h(r, j) - m; a0 += dv * dv; }
    }
    __syncthreads();
    s0[threadIdx.x] = a0;
    __syncthreads();
    if (ry == 0 && j < F) {
        for (int t = 1; t < RL; ++t) a0 += s0[t * CW + c];
        tstore<COH>(part + j, m);
        tstore<COH>(part + F + j, a0);
    }
}

// (count, mean, M2) of two disjoint sets of rows -> of their union (exact in real arithmetic; the order of the calls is fixed)
__device__ __forceinline__ void stats_merge(float &cnt, float &mean, float &m2, float cb, float mb, float qb)
{
    if (cb == 0.0f) return;
    const float delta = mb - mean, tot = cnt + cb;
    mean = mean + delta * (cb / tot);
    m2 = m2 + qb + delta * delta * (cnt * cb / tot);
    cnt = tot;
}

// batch mean / 1 / sqrt(biased batch variance + eps) of every column from the chunk statistics part [parts][2 F] of n rows in chunks of
// rows_per_block: sm [F], sinv [F] (LDS).  256 / CW lanes per column take every (256 / CW)-th chunk, the lanes are merged in order.
// stats != NULL: [mean | var] is left there for the backward pass and the moving statistics.  sc [3][256]: LDS.  Every thread of the 256
// calls it (it contains barriers; sm / sinv are complete behind the last one).
template <bool COH>
__device__ __forceinline__ void bn_merge_chunks(int64_t n, int F, int cw_shift, const float *part, int parts, int64_t rows_per_block, float eps,
                                                float *stats, float *sm, float *sinv, float (*sc)[256])
{
    const int CW = 1 << cw_shift, ZL = 256 >> cw_shift;
    const int c = threadIdx.x & (CW - 1), zl = threadIdx.x >> cw_shift;
    for (int jb = 0; jb < F; jb += CW) {
        const int j = jb + c;
        float cnt = 0.0f, mean = 0.0f, m2 = 0.0f;
        if (j < F) {
#pragma unroll 4
            for (int z = zl; z < parts; z += ZL) {
                const int64_t r0 = (int64_t)z * rows_per_block;
                const float nz = (float)((r0 + rows_per_block < n ? r0 + rows_per_block : n) - r0);
                stats_merge(cnt, mean, m2, nz, tload<COH>(part + (size_t)z * 2 * F + j), tload<COH>(part + (size_t)z * 2 * F + F + j));
            }
        }
        sc[0][threadIdx.x] = cnt; sc[1][threadIdx.x] = mean; sc[2][threadIdx.x] = m2;
        __syncthreads();
        if (zl == 0 && j < F) {
            for (int t = 1; t < ZL; ++t) stats_merge(cnt, mean, m2, sc[0][t * CW + c], sc[1][t * CW + c], sc[2][t * CW + c]);
            const float var = m2 / (float)n;
            sm[j] = mean;
            sinv[j] = 1.0f / sqrtf(var + eps);
            if (stats) { stats[j] = mean; stats[F + j] = var; }
        }
        __syncthreads();
    }
}

// xhat = (h - mean) / sqrt(var + eps), y = gamma xhat + beta of one element
__device__ __forceinline__ void bn_normalize(float hv, float mean, float inv, float gamma, float beta, float *xhat, float *y)
{
    const float xh = (hv - mean) * inv;
    *xhat = xh;
    *y = gamma * xh + beta;
}

// softmax of one row (z and a may be the same row)
__device__ __forceinline__ void softmax_row(int F, const float *zr, float *ar)
{
    float m = zr[0];
    for (int j = 1; j < F; ++j) m = zr[j] > m ? zr[j] : m;
    float s = 0.0f;
    for (int j = 0; j < F; ++j) { const float e = gnn_expf(zr[j] - m); ar[j] = e; s = s + e; }
    for (int j = 0; j < F; ++j) ar[j] = __fdiv_rn(ar[j], s);
}

// Dense products of the training step, Y[r, j] = sum_k X[r, k] M[k, j] on R rows per block: 256 threads = CW output columns x KG
// slices of the k range (CW = 2^cshift >= min(columns, 64)); every thread runs the fmaf chain of its slice (one to a few iterations
// even for narrow layers: the loop over k is a chain of L2 round trips), the KG partial sums of an output are added in slice order
// through LDS.  xs: R rows of X, padded to a multiple of 4 (zeros); ps: [KG][R][CW] partials.  fin(r, j, value) stores an output.
// (The value of an output does not depend on R: the slices and the order of their sums are a function of n_k and cshift alone.)
template <int R, class Fin>
__device__ __forceinline__ void dense_rows(int n_k, int n_k_pad, int n_cols, int cshift, const float *__restrict__ M, const float *xs, float *ps, Fin fin)
{
    const int CW = 1 << cshift, KG = 256 >> cshift;
    const int c = threadIdx.x & (CW - 1), kg = threadIdx.x >> cshift;
    const int slice = ((n_k + KG - 1) / KG + 3) & ~3;
    const int k0 = kg * slice, k1 = k0 + slice < n_k ? k0 + slice : n_k;
    for (int jb = 0; jb < n_cols; jb += CW) {
        const int j = jb + c;
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0f;
        if (j < n_cols) {
            int k = k0;
            for (; k + 4 <= k1; k += 4) {
                const float w0 = M[(size_t)(k + 0) * n_cols + j], w1 = M[(size_t)(k + 1) * n_cols + j];
                const float w2 = M[(size_t)(k + 2) * n_cols + j], w3 = M[(size_t)(k + 3) * n_cols + j];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 x = *reinterpret_cast<const float4 *>(&xs[r * n_k_pad + k]);
                    acc[r] = __builtin_fmaf(x.x, w0, acc[r]);
                    acc[r] = __builtin_fmaf(x.y, w1, acc[r]);
                    acc[r] = __builtin_fmaf(x.z, w2, acc[r]);
                    acc[r] = __builtin_fmaf(x.w, w3, acc[r]);
                }
            }
            for (; k < k1; ++k) {
                const float wk = M[(size_t)k * n_cols + j];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(xs[r * n_k_pad + k], wk, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) ps[(kg * R + r) * CW + c] = acc[r];
        __syncthreads();
        if (j < n_cols)
            for (int r = kg; r < R; r += KG) {
                float v = ps[r * CW + c];
                for (int g = 1; g < KG; ++g) v += ps[(g * R + r) * CW + c];
                fin(r, j, v);
            }
        __syncthreads();
    }
}

inline int dense_cshift(int cols) { int s = 2; while ((1 << s) < cols && s < 6) ++s; return s; }     // CW = 4 .. 64
inline size_t dense_lds_bytes(int R, int k_pad) { return sizeof(float) * ((size_t)R * k_pad + (size_t)256 * R); }

// ALL Dense layers of a Sequential on a row tile in one launch (few rows: a MUTAG-sized step is bound by the number of launches): the
// tile's activations go from layer to layer through LDS, every layer's output is also written out (the backward pass reads it); the
// arithmetic per layer is that of k_dense_fwd (same dense_rows chains: identical bits).  No Dropout between the layers, softmax only as
// the last activation (applied by the caller).  LDS: 2 R maxpad + 256 R floats.
struct MlpFwd {
    int64_t n;
    int L, maxpad;
    int dims[GNN_FUSED_MAXL + 2], pad[GNN_FUSED_MAXL + 2], cshift[GNN_FUSED_MAXL + 1], act[GNN_FUSED_MAXL + 1];
    const float *W[GNN_FUSED_MAXL + 1], *b[GNN_FUSED_MAXL + 1];
    const float *X;
    float *Y[GNN_FUSED_MAXL + 1];
    // build != 0 (net_state of a loop body, no Dropout in front of the first layer): the input rows are not read from X but BUILT here -
    // the concat of k_train_input (GNN.py:223-239: own state | template columns | aggregated neighbour states, the fmaf chain over the
    // arcs in stored order) - written to X_out for the backward pass, and the body's gate (GNN.py:202-220) is evaluated per row
    int build, Ds, c_aggs;
    const float *tmpl, *state, *own, *own_prev;
    const int32_t *indptr, *adj_src;
    const float *adj_w;
    float *X_out;
    float thr;
    int *flag;
};

// the while-condition of a body for one row (k_train_input's chain: ascending-feature sums): cur(q) / old(q) = feature q of the row's
// state / of its state one body earlier
template <class Cur, class Old>
__device__ __forceinline__ int mlp_row_moved(int Ds, float thr, Cur cur, Old old)
{
    float dist = 0.0f, nrm = 0.0f;
    for (int q = 0; q < Ds; ++q) {
        const float o = old(q);
        const float df = cur(q) - o;
        dist = dist + df * df;
        nrm = nrm + o * o;
    }
    return sqrtf(dist) > thr * sqrtf(nrm) ? 1 : 0;
}

// the concat rows of the tile from row i0 (MlpFwd::build) into `in` [R][pad[0]] and X_out.  COH: the state rows were written by other
// workgroups of this launch.  GATE: the thread of column 0 also evaluates the body's while-condition for its row; returns whether it moves.
template <int R, bool COH, bool GATE>
__device__ __forceinline__ int mlp_build_rows(const MlpFwd &p, int64_t i0, float *in)
{
    const int in_s = p.dims[0], Ds = p.Ds, c_aggs = p.c_aggs;
    int moved = 0;
    for (int t = threadIdx.x; t < R * p.pad[0]; t += blockDim.x) {
        const int r = t / p.pad[0], c = t - r * p.pad[0];
        const int64_t row = i0 + r;
        float v = 0.0f;
        if (c < in_s && row < p.n) {
            if (c < Ds) v = tload<COH>(p.own + row * Ds + c);
            else if (c >= c_aggs && c < c_aggs + Ds) {
                const int cc = c - c_aggs;
                const int32_t e1 = p.indptr[row + 1];
                for (int32_t e = p.indptr[row]; e < e1; e += 4) {          // four arcs per step: their loads are in flight together
                    float w[4], x[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool in_ = e + u < e1;
                        w[u] = in_ ? p.adj_w[e + u] : 0.0f;
                        x[u] = in_ ? tload<COH>(p.state + (int64_t)p.adj_src[e + u] * Ds + cc) : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (e + u < e1) v = __builtin_fmaf(w[u], x[u], v);
                }
            } else
                v = p.tmpl[row * in_s + c];
            p.X_out[row * in_s + c] = v;
            if (GATE && c == 0) {                      // the while-condition of this body for the row
                const float *own = p.own + row * Ds, *prev = p.own_prev ? p.own_prev + row * Ds : nullptr;
                moved |= mlp_row_moved(Ds, p.thr, [&](int q) { return tload<COH>(own + q); }, [&](int q) { return prev ? tload<COH>(prev + q) : 1.0f; });
            }
        }
        in[t] = v;
    }
    return moved;
}

// the Dense layers on the tile whose input rows are in `in` [R][pad[0]]; returns the LDS rows [R][pad[L]] of the last layer's output.
// COH_LAST: the last layer's output is read by other workgroups inside this launch (write-through stores).
template <int R, bool COH_LAST>
__device__ __forceinline__ float *mlp_layers(const MlpFwd &p, int64_t i0, float *in, float *out, float *ps)
{
    for (int l = 0; l < p.L; ++l) {
        const int no = p.dims[l + 1], npad = p.pad[l + 1], act = p.act[l];
        for (int t = threadIdx.x; t < R * npad; t += blockDim.x) out[t] = 0.0f;          // (the padding columns of the next input)
        __syncthreads();
        const float *bl = p.b[l];
        float *Yl = p.Y[l];
        const bool last = l == p.L - 1;
        dense_rows<R>(p.dims[l], p.pad[l], no, p.cshift[l], p.W[l], in, ps, [&](int r, int j, float v) {
            v = v + bl[j];
            if (act != GNN_ACT_SOFTMAX) v = gnn_act(v, act);
            out[r * npad + j] = v;
            if (i0 + r < p.n) {
                if (COH_LAST && last) tstore<true>(Yl + (i0 + r) * no + j, v);
                else Yl[(i0 + r) * no + j] = v;
            }
        });
        float *t_ = in; in = out; out = t_;          // (dense_rows ends with a barrier)
    }
    return in;
}

// host: the fields of an MlpFwd that the net alone decides (everything but n, X / X_out, Y and the build fields)
inline void mlp_fwd_describe(MlpFwd &p, const gnn_mlp *m, int maxpad)
{
    const int L = m->n_layers;
    p.L = L; p.maxpad = maxpad;
    for (int q = 0; q <= L; ++q) { p.dims[q] = m->dims[q]; p.pad[q] = (m->dims[q] + 3) & ~3; }
    for (int q = 0; q < L; ++q) { p.cshift[q] = dense_cshift(m->dims[q + 1]); p.act[q] = m->acts[q]; p.W[q] = m->W[q]; p.b[q] = m->b[q]; }
}

}   // namespace gnn_train
