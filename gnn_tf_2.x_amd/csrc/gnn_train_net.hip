// One Sequential in training mode: Dropout, activations, BatchNormalization, the per-layer and small fused Dense kernels, the state
// gradient behind net_state's backward pass; net_setup / net_forward / net_backward (see gnn_train.hip for the step).
#include <stdlib.h>

#include "gnn_train.h"
#include "gnn_train_dev.h"        // what the persistent forward of small batches (gnn_train_small.hip) runs too

using namespace gnn_train;

namespace {

// Dropout forward: keep[i] = injected mask or own RNG (stream `key`, element idx0 + i: idx0 is added to the hashed index only, not to
// addresses); y = x * keep / (1 - rate); keep bytes are stored for the backward pass
__global__ void k_dropout_fwd(int64_t n, const float *x, const uint8_t *mask_in, float rate, uint64_t key, int64_t idx0, uint8_t *keep, float *y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float r = fabsf(rate);
    uint8_t kp;
    if (mask_in) kp = mask_in[i] != 0;
    else kp = dropout_keep(key, (uint64_t)(idx0 + i), r);
    keep[i] = kp;
    if (rate < 0.0f) {
        float a, b, ap;
        alpha_dropout_coeffs(r, &a, &b, &ap);
        y[i] = a * (kp ? x[i] : ap) + b;
    } else
        y[i] = kp ? x[i] / (1.0f - rate) : 0.0f;
}

__global__ void k_dropout_bwd(int64_t n, const uint8_t *keep, float rate, float *d)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (rate < 0.0f) {
        float a, b, ap;
        alpha_dropout_coeffs(-rate, &a, &b, &ap);
        d[i] = keep[i] ? d[i] * a : 0.0f;
    } else
        d[i] = keep[i] ? d[i] / (1.0f - rate) : 0.0f;
}

__global__ void k_act_fwd(int64_t n, int F, const float *z, int act, float *a)
{
    if (act == GNN_ACT_SOFTMAX) {
        const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (r >= n) return;
        softmax_row(F, z + r * F, a + r * F);
    } else {
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n * F) a[i] = gnn_act(z[i], act);
    }
}

// dz = da * act'(z) (softmax: a * (da - sum da a) per row); in place on d
__global__ void k_act_bwd(int64_t n, int F, float *d, const float *a, int act)
{
    if (act == GNN_ACT_SOFTMAX) {
        const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (r >= n) return;
        float s = 0.0f;
        for (int j = 0; j < F; ++j) s += d[r * F + j] * a[r * F + j];
        for (int j = 0; j < F; ++j) d[r * F + j] = a[r * F + j] * (d[r * F + j] - s);
        return;
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * F) return;
    d[i] = d[i] * act_grad(a[i], act);
}

// (Row chunks and the thread layout of the column reductions, column_shift: gnn_train_dev.h)

// partial sums of x * y and x over the rows of chunk blockIdx.y: out0 / out1 [chunk * ostride + j]
__global__ void __launch_bounds__(256) k_colreduce2(int64_t n, int F, int cw_shift, const float *__restrict__ x, const float *__restrict__ y, float *out0,
                                                    float *out1, int64_t ostride, int64_t rows_per_block)
{
    __shared__ float s0[256], s1[256];
    const int CW = 1 << cw_shift, RL = 256 >> cw_shift;
    const int c = threadIdx.x & (CW - 1), ry = threadIdx.x >> cw_shift;
    const int j = blockIdx.x * CW + c;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    float a0 = 0.0f, a1 = 0.0f;
    if (j < F) {
        int64_t r = r0 + ry;
        for (; r + 3 * RL < r1; r += 4 * RL) {
            float xv[4], yv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { xv[q] = x[(r + q * RL) * F + j]; yv[q] = y[(r + q * RL) * F + j]; }
#pragma unroll
            for (int q = 0; q < 4; ++q) { a0 += xv[q] * yv[q]; a1 += xv[q]; }
        }
        for (; r < r1; r += RL) { const float v = x[r * F + j]; a0 += v * y[r * F + j]; a1 += v; }
    }
    s0[threadIdx.x] = a0; s1[threadIdx.x] = a1;
    __syncthreads();
    if (ry == 0 && j < F) {
        for (int t = 1; t < RL; ++t) { a0 += s0[t * CW + c]; a1 += s1[t * CW + c]; }
        out0[(size_t)blockIdx.y * ostride + j] = a0;
        out1[(size_t)blockIdx.y * ostride + j] = a1;
    }
}

// out[t] += part[0][t] + part[1][t] + ... for the 64 columns of block `bid`: four lanes per column take every fourth chunk, their
// sums are added in lane order
__device__ __forceinline__ void sum_parts_block(int bid, int parts, int64_t count, const float *__restrict__ part, float *out, float *sp /* [256] */)
{
    const int c = threadIdx.x & 63, zl = threadIdx.x >> 6;
    const int64_t t = (int64_t)bid * 64 + c;
    float acc = 0.0f;
    if (t < count) {
#pragma unroll 8
        for (int z = zl; z < parts; z += 4) acc += part[(size_t)z * count + t];
    }
    sp[threadIdx.x] = acc;
    __syncthreads();
    if (zl == 0 && t < count) out[t] += ((acc + sp[64 + c]) + sp[128 + c]) + sp[192 + c];
}

__global__ void __launch_bounds__(256) k_sum_parts(int parts, int64_t count, const float *part, float *out)
{
    __shared__ float sp[256];
    sum_parts_block(blockIdx.x, parts, count, part, out, sp);
}

// out[j] = sum over the chunks z (ascending) of base[z * stride + j], j < count: a rank's own share of sums that the sharded backward
// pass exchanges (BatchNormalization: sum d y xhat | sum d y)
__global__ void __launch_bounds__(256) k_sum_strided(int parts, int64_t stride, const float *__restrict__ base, int count, float *out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    float acc = 0.0f;
    for (int z = 0; z < parts; ++z) acc += base[(size_t)z * stride + j];
    out[j] = acc;
}

// BatchNormalization, training mode, forward statistics of one row chunk: part[chunk][j] = chunk mean, part[chunk][F + j] =
// sum over the chunk of (x - chunk mean)^2 (bn_chunk_stats)
__global__ void __launch_bounds__(256) k_bn_stats(int64_t n, int F, int cw_shift, const float *__restrict__ h, float *part, int64_t rows_per_block)
{
    __shared__ float s0[256];
    __shared__ float mu[32];
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    bn_chunk_stats<false>(F, cw_shift, blockIdx.x << cw_shift, r0, r1, [&](int64_t r, int j) { return h[r * F + j]; }, part + (size_t)blockIdx.y * 2 * F, s0, mu);
}

// batch mean / biased batch variance from the chunk statistics, then xhat = (h - mean) / sqrt(var + eps), y = gamma xhat + beta.
// Every block combines the chunks itself (256 / CW lanes per column take every (256 / CW)-th chunk, the lanes are merged in order);
// block 0 leaves [mean | var] in stats for the backward pass and the moving statistics.  Dynamic LDS: 2 F floats.
// XHAT = false (the state-only first pass of the recomputing step): xhat, which only the backward pass reads, is not written.
template <bool XHAT>
__global__ void __launch_bounds__(256) k_bn_apply(int64_t n, int F, int cw_shift, const float *__restrict__ h, const float *__restrict__ part, int parts,
                                                  int64_t rows_per_block, float eps, const float *gamma, const float *beta, float *xhat, float *y, float *stats)
{
    extern __shared__ float bsh[];
    __shared__ float sc[3][256];
    float *sm = bsh, *sinv = bsh + F;
    bn_merge_chunks<false>(n, F, cw_shift, part, parts, rows_per_block, eps, blockIdx.x == 0 ? stats : nullptr, sm, sinv, sc);
    const int64_t total = n * F, step = (int64_t)gridDim.x * blockDim.x;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int j = small ? (int)((unsigned)i % (unsigned)F) : (int)(i % F);
        float xh;
        bn_normalize(h[i], sm[j], sinv[j], gamma[j], beta[j], &xh, &y[i]);
        if constexpr (XHAT) xhat[i] = xh;
    }
}

// (Round 3 tried BatchNormalization of a small batch as ONE single-block launch per direction - statistics + apply, column sums + apply,
//  matrices staged in LDS, tree-reduced column sums - to save two launches per call: SLOWER than the two multi-block kernels at MUTAG size,
//  0.85 against 0.76 ms per 10-body step and 3.0 against 2.6 ms per 50-body step: one workgroup's latency chain against a few microseconds
//  of launch.  Removed.)
// ---- BatchNormalization statistics over the rows of ALL ranks (sharded training forward) ----------------------------------------------
// k_bn_local: the rank's chunk statistics merged in chunk order into ONE triple per feature, tri = [count | mean | M2] (3 F floats);
// the triples of all ranks are all-gathered (3 F floats per rank and call - the review's "2 H floats" plus the count) and
// k_bn_apply_ext merges them in RANK order - every rank the same numbers - before it normalises its own rows.
__global__ void __launch_bounds__(256) k_bn_local(int64_t n, int F, const float *__restrict__ part, int parts, int64_t rows_per_block, float *tri)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= F) return;
    float cnt = 0.0f, mean = 0.0f, m2 = 0.0f;
    for (int z = 0; z < parts; ++z) {
        const int64_t r0 = (int64_t)z * rows_per_block;
        const float nz = (float)((r0 + rows_per_block < n ? r0 + rows_per_block : n) - r0);
        stats_merge(cnt, mean, m2, nz, part[(size_t)z * 2 * F + j], part[(size_t)z * 2 * F + F + j]);
    }
    tri[j] = cnt; tri[F + j] = mean; tri[2 * F + j] = m2;
}

__global__ void __launch_bounds__(256) k_bn_apply_ext(int64_t n, int F, const float *__restrict__ h, const float *__restrict__ tri_all, int world, float eps,
                                                      const float *gamma, const float *beta, float *xhat, float *y, float *stats)
{
    extern __shared__ float bsh[];
    float *sm = bsh, *sinv = bsh + F;
    for (int j = threadIdx.x; j < F; j += blockDim.x) {
        float cnt = 0.0f, mean = 0.0f, m2 = 0.0f;
        for (int p = 0; p < world; ++p) stats_merge(cnt, mean, m2, tri_all[(size_t)p * 3 * F + j], tri_all[(size_t)p * 3 * F + F + j], tri_all[(size_t)p * 3 * F + 2 * F + j]);
        const float var = cnt > 0.0f ? m2 / cnt : 0.0f;
        sm[j] = mean;
        sinv[j] = 1.0f / sqrtf(var + eps);
        if (blockIdx.x == 0) { stats[j] = mean; stats[F + j] = var; }
    }
    __syncthreads();
    const int64_t total = n * F, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int j = (int)(i % F);
        const float xh = (h[i] - sm[j]) * sinv[j];
        xhat[i] = xh;
        y[i] = gamma[j] * xh + beta[j];
    }
}

// d x = inv / n * (n * dxh - sum dxh - xhat * sum(dxh * xhat)), dxh = d y * gamma, with sum d y * xhat / sum d y added up from the
// chunk partials p_dyx / p_dy [chunk * pstride + j] (the same numbers k_sum_parts adds into the gamma / beta gradients);
// then, fused, the derivative of the layer's activation: d <- d x * act'(a) (act < 0: none).  Dynamic LDS: 2 F floats.
__global__ void __launch_bounds__(256) k_bn_bwd_apply(int64_t n, int F, int cw_shift, float *d, const float *__restrict__ xhat, const float *gamma,
                                                      const float *stats, float eps, const float *__restrict__ p_dyx, const float *__restrict__ p_dy,
                                                      int64_t pstride, int parts, const float *__restrict__ a, int act, int64_t n_stat = 0)
{
    // n_stat: rows the batch statistics were taken over (sharded backward: the rows of ALL ranks, the partial sums are then one pair per rank); 0: n
    extern __shared__ float bsh[];
    __shared__ float sc[2][256];
    float *s_dyx = bsh, *s_dy = bsh + F;
    const int CW = 1 << cw_shift, ZL = 256 >> cw_shift;
    const int c = threadIdx.x & (CW - 1), zl = threadIdx.x >> cw_shift;
    for (int jb = 0; jb < F; jb += CW) {
        const int j = jb + c;
        float a0 = 0.0f, a1 = 0.0f;
        if (j < F) {
#pragma unroll 4
            for (int z = zl; z < parts; z += ZL) { a0 += p_dyx[(size_t)z * pstride + j]; a1 += p_dy[(size_t)z * pstride + j]; }
        }
        sc[0][threadIdx.x] = a0; sc[1][threadIdx.x] = a1;
        __syncthreads();
        if (zl == 0 && j < F) {
            for (int t = 1; t < ZL; ++t) { a0 += sc[0][t * CW + c]; a1 += sc[1][t * CW + c]; }
            s_dyx[j] = a0; s_dy[j] = a1;
        }
        __syncthreads();
    }
    const int64_t total = n * F, step = (int64_t)gridDim.x * blockDim.x;
    const float m = (float)(n_stat > 0 ? n_stat : n);
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int j = small ? (int)((unsigned)i % (unsigned)F) : (int)(i % F);
        const float inv = 1.0f / sqrtf(stats[F + j] + eps), g = gamma[j];
        float v = inv / m * (m * d[i] * g - g * s_dy[j] - xhat[i] * g * s_dyx[j]);
        if (act >= 0) v = v * act_grad(a[i], act);
        d[i] = v;
    }
}

// ---- BatchNormalization on its MOVING statistics (the fixed-point gradient with GNN_ADJOINT_FROZEN_BN) -------------------------------------
// A per-row affine map, the one the inference Loop iterates: no statistics kernel, no chunk merge, and a Jacobian that is a per-column scale.
// k_bn_frozen_prepare, once per step: frozen = [inv_j = 1 / sqrtf(var_mov_j + eps) | s_j = gamma_j inv_j]; raw: the MLP's [gamma | beta | mean | var].
__global__ void k_bn_frozen_prepare(int F, float eps, const float *raw, const float *gamma, float *frozen)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= F) return;
    const float inv = 1.0f / sqrtf(raw[3 * F + j] + eps);
    frozen[j] = inv;
    frozen[F + j] = gamma[j] * inv;
}

// the recorded body: xhat = (h - mean_mov) inv, y = gamma xhat + beta (bn_normalize, as k_bn_apply on batch statistics)
__global__ void __launch_bounds__(256) k_bn_apply_frozen(int64_t n, int F, const float *__restrict__ h, const float *__restrict__ mean, const float *__restrict__ inv,
                                                         const float *__restrict__ gamma, const float *__restrict__ beta, float *xhat, float *y)
{
    const int64_t total = n * F, step = (int64_t)gridDim.x * blockDim.x;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int j = small ? (int)((unsigned)i % (unsigned)F) : (int)(i % F);
        bn_normalize(h[i], mean[j], inv[j], gamma[j], beta[j], &xhat[i], &y[i]);
    }
}

// the way back: d <- d s_j, then, fused, the derivative of the layer's activation: d <- d act'(a) (act < 0: none) - in the place of
// k_bn_bwd_apply behind k_colreduce2 (weight pass), or alone in the place of k_act_bwd (an adjoint iteration)
__global__ void __launch_bounds__(256) k_bn_bwd_frozen(int64_t n, int F, float *d, const float *__restrict__ scale, const float *__restrict__ a, int act)
{
    const int64_t total = n * F, step = (int64_t)gridDim.x * blockDim.x;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int j = small ? (int)((unsigned)i % (unsigned)F) : (int)(i % F);
        float v = d[i] * scale[j];
        if (act >= 0) v = v * act_grad(a[i], act);
        d[i] = v;
    }
}

// Weight and bias gradient of one Dense layer over one row chunk: part[chunk * pstride + i * n_out + j] = sum_r H'[r, i] DZ[r, j]
// with H' = [H | 1] (row i = n_in is the bias gradient: dW and db are adjacent in the gradient vector).  32 x 32 outputs per
// block, 2 x 2 per thread (one 8-byte LDS read of each operand per four products), 64 rows staged per step, the next step's
// rows fetched into registers while this step's products run.  lds: 2 x 64 x 34 floats.
#define GNN_WG_TILE 32
#define GNN_WG_LD 34
__device__ __forceinline__ void wgrad_block(int bx, int by, int bz, int64_t n, int n_in, int n_out, const float *__restrict__ H,
                                            const float *__restrict__ DZ, float *part, int64_t pstride, int64_t rows_per_block, float *lds)
{
    float *sh = lds, *sz = lds + 64 * GNN_WG_LD;
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;            // outputs (i0 + 2 ti + {0, 1}, j0 + 2 tj + {0, 1})
    const int lr = threadIdx.x >> 5, lc = threadIdx.x & 31;            // loader: rows lr + 8 q, column lc
    const int i0 = bx * GNN_WG_TILE, j0 = by * GNN_WG_TILE;
    const int64_t r0 = (int64_t)bz * rows_per_block, r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    float a00 = 0.0f, a01 = 0.0f, a10 = 0.0f, a11 = 0.0f;
    float hv[8], zv[8];
    auto fetch = [&](int64_t r) {                  // this thread's share of the 64-row step at r, into registers
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int64_t row = r + lr + 8 * q;
            const bool in = row < r1;
            hv[q] = !in ? 0.0f : (i0 + lc < n_in ? H[row * n_in + i0 + lc] : (i0 + lc == n_in ? 1.0f : 0.0f));
            zv[q] = (in && j0 + lc < n_out) ? DZ[row * n_out + j0 + lc] : 0.0f;
        }
    };
    if (r0 < r1) fetch(r0);
    for (int64_t r = r0; r < r1; r += 64) {
#pragma unroll
        for (int q = 0; q < 8; ++q) { sh[(lr + 8 * q) * GNN_WG_LD + lc] = hv[q]; sz[(lr + 8 * q) * GNN_WG_LD + lc] = zv[q]; }
        __syncthreads();
        if (r + 64 < r1) fetch(r + 64);            // the next step's loads fly during this step's products
#pragma unroll 16
        for (int q = 0; q < 64; ++q) {
            const float2 hq = *reinterpret_cast<const float2 *>(sh + q * GNN_WG_LD + 2 * ti);
            const float2 zq = *reinterpret_cast<const float2 *>(sz + q * GNN_WG_LD + 2 * tj);
            a00 = __builtin_fmaf(hq.x, zq.x, a00); a01 = __builtin_fmaf(hq.x, zq.y, a01);
            a10 = __builtin_fmaf(hq.y, zq.x, a10); a11 = __builtin_fmaf(hq.y, zq.y, a11);
        }
        __syncthreads();
    }
    float *out = part + (size_t)bz * pstride;
    const int i = i0 + 2 * ti, j = j0 + 2 * tj;
    if (i <= n_in) {
        if (j < n_out) out[(size_t)i * n_out + j] = a00;
        if (j + 1 < n_out) out[(size_t)i * n_out + j + 1] = a01;
    }
    if (i + 1 <= n_in) {
        if (j < n_out) out[(size_t)(i + 1) * n_out + j] = a10;
        if (j + 1 < n_out) out[(size_t)(i + 1) * n_out + j + 1] = a11;
    }
}

// (dense_rows, dense_cshift, dense_lds_bytes: gnn_train_dev.h)

// d h_in = d z . W^T, then (fused) the way back through what produced h_in: Dropout (keep != NULL) and the previous layer's
// activation (act >= 0: d <- d * act'(a_prev))
template <int R>
__device__ __forceinline__ void dense_bwd_block(int64_t bid, int64_t n, int n_out, int n_out_pad, int n_in, int cshift, const float *__restrict__ DZ,
                                                const float *__restrict__ WT, const uint8_t *__restrict__ keep, float rate,
                                                const float *__restrict__ a_prev, int act, float *__restrict__ dprev, float *xs)
{
    const int64_t i0 = bid * R;
    for (int t = threadIdx.x; t < R * n_out_pad; t += blockDim.x) {
        const int r = t / n_out_pad, k = t - r * n_out_pad;
        xs[t] = (k < n_out && i0 + r < n) ? DZ[(i0 + r) * n_out + k] : 0.0f;
    }
    __syncthreads();
    dense_rows<R>(n_out, n_out_pad, n_in, cshift, WT, xs, xs + R * n_out_pad, [&](int r, int j, float v) {
        if (i0 + r >= n) return;
        const int64_t o = (i0 + r) * n_in + j;
        if (keep) v = dropout_grad(v, keep[o], rate);
        if (act >= 0) v = v * act_grad(a_prev[o], act);
        dprev[o] = v;
    });
}

// a = act(h . W + b), training-mode forward of one Dense layer (softmax is applied by the caller)
template <int R>
__global__ void __launch_bounds__(256) k_dense_fwd(int64_t n, int n_in, int n_in_pad, int n_out, int cshift, const float *__restrict__ X,
                                                   const float *__restrict__ W, const float *__restrict__ b, int act, float *__restrict__ Y)
{
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int64_t i0 = (int64_t)blockIdx.x * R;
    for (int t = threadIdx.x; t < R * n_in_pad; t += blockDim.x) {
        const int r = t / n_in_pad, k = t - r * n_in_pad;
        xs[t] = (k < n_in && i0 + r < n) ? X[(i0 + r) * n_in + k] : 0.0f;
    }
    __syncthreads();
    dense_rows<R>(n_in, n_in_pad, n_out, cshift, W, xs, xs + R * n_in_pad, [&](int r, int j, float v) {
        if (i0 + r >= n) return;
        v = v + b[j];
        if (act != GNN_ACT_SOFTMAX) v = gnn_act(v, act);
        Y[(i0 + r) * n_out + j] = v;
    });
}

// ALL Dense layers of a Sequential on a row tile in one launch (MlpFwd, mlp_build_rows, mlp_layers: gnn_train_dev.h)
template <int R>
__global__ void __launch_bounds__(256) k_mlp_fwd(const MlpFwd p)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *in = lds, *out = lds + (size_t)R * p.maxpad, *ps = lds + (size_t)2 * R * p.maxpad;
    const int64_t i0 = (int64_t)blockIdx.x * R;
    if (p.build) {
        const int moved = mlp_build_rows<R, false, true>(p, i0, in);
        if (__any(moved) && (threadIdx.x & 63) == 0) gnn_flag_raise(p.flag);
    } else {
        for (int t = threadIdx.x; t < R * p.pad[0]; t += blockDim.x) {
            const int r = t / p.pad[0], k = t - r * p.pad[0];
            in[t] = (k < p.dims[0] && i0 + r < p.n) ? p.X[(i0 + r) * p.dims[0] + k] : 0.0f;
        }
    }
    mlp_layers<R, false>(p, i0, in, out, ps);
}


// One Dense layer of the backward pass in one launch: the blocks of the weight / bias gradient (first wg_blocks ids: the heavier
// ones) and the blocks of d h_in run side by side; both read d z, neither reads the other's result.
struct LayerBwd {
    int64_t n, rows_per_block, pstride;
    int n_in, n_out, n_out_pad, act, wg_bx, wg_by, wg_blocks, cshift;
    float rate;
    const float *H, *DZ, *WT, *a_prev;
    const uint8_t *keep;
    float *part, *dprev;
};

template <int R>
__global__ void __launch_bounds__(256) k_layer_bwd(const LayerBwd p)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if ((int)blockIdx.x < p.wg_blocks) {
        const int id = blockIdx.x, bx = id % p.wg_bx, by = (id / p.wg_bx) % p.wg_by, bz = id / (p.wg_bx * p.wg_by);
        wgrad_block(bx, by, bz, p.n, p.n_in, p.n_out, p.H, p.DZ, p.part, p.pstride, p.rows_per_block, lds);
    } else
        dense_bwd_block<R>((int64_t)blockIdx.x - p.wg_blocks, p.n, p.n_out, p.n_out_pad, p.n_in, p.cshift, p.DZ, p.WT, p.keep, p.rate, p.a_prev, p.act, p.dprev, lds);
}

// End of one body of the backward pass in one launch.  Blocks < sg_blocks: aggregated_states = Adjacency^T . state  =>
// d state[r] = d inp[r, :Ds] + sum over arcs (r -> dst) of w * d inp[dst, c_aggs:] (own-state columns of the concat + the transposed
// aggregation over the by-source CSR).  The other blocks: the net's gradient vector += this call's chunk partials (sum_parts_block).
__global__ void __launch_bounds__(256) k_state_grad_sum(int sg_blocks, int64_t n, int Ds, int in_s, int c_aggs, const float *__restrict__ d_inp,
                                                        const int32_t *__restrict__ sip, const int32_t *__restrict__ sdst, const float *__restrict__ sw,
                                                        float *__restrict__ d_state, int parts, int64_t count, const float *part, float *out)
{
    __shared__ float sp[256];
    if ((int)blockIdx.x >= sg_blocks) {
        sum_parts_block(blockIdx.x - sg_blocks, parts, count, part, out, sp);
        return;
    }
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * Ds) return;
    const int64_t r = n * Ds < ((int64_t)1 << 31) ? (int64_t)((unsigned)t / (unsigned)Ds) : t / Ds;
    const int c = (int)(t - r * Ds);
    float acc = 0.0f;
    const int32_t e1 = sip[r + 1];
    for (int32_t e = sip[r]; e < e1; e += 4) {                  // four arcs per step: their loads are in flight together
        float w[4], x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = e + u < e1;
            w[u] = in ? sw[e + u] : 0.0f;
            x[u] = in ? d_inp[(int64_t)sdst[e + u] * in_s + c_aggs + c] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) if (e + u < e1) acc = __builtin_fmaf(w[u], x[u], acc);
    }
    d_state[t] = d_inp[r * in_s + c] + acc;
}


// The transposed aggregation of k_state_grad_sum for many rows (state width a multiple of 4, <= 64): 16 lanes per source row, four columns
// per lane, four arcs in flight per lane (sixteen dependent-free loads), same fmaf chain per element; the sum of the chunk partials runs as
// its own launch then.  (One thread per element: 1.14 ms per body at 1 M rows x 64, profiles/r03_train_c3.txt.)
__global__ void __launch_bounds__(256) k_state_grad_rows(int64_t n, int Ds, int in_s, int c_aggs, const float *__restrict__ d_inp, const int32_t *__restrict__ sip,
                                                         const int32_t *__restrict__ sdst, const float *__restrict__ sw, float *__restrict__ d_state)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 4;
    const int cc = 4 * (int)(t & 15);
    if (r >= n || cc >= Ds) return;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int32_t e1 = sip[r + 1];
    for (int32_t e = sip[r]; e < e1; e += 4) {
        float w[4], x[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = e + u < e1;
            w[u] = in ? sw[e + u] : 0.0f;
            const float *q = d_inp + (int64_t)(in ? sdst[e + u] : 0) * in_s + c_aggs + cc;
#pragma unroll
            for (int v = 0; v < 4; ++v) x[u][v] = in ? q[v] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e + u < e1) {
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[v] = __builtin_fmaf(w[u], x[u][v], acc[v]);
            }
    }
    const float *own = d_inp + r * in_s + cc;
    *reinterpret_cast<float4 *>(d_state + r * Ds + cc) = float4{own[0] + acc[0], own[1] + acc[1], own[2] + acc[2], own[3] + acc[3]};
}

// The same from the aligned copy k_bwd3_split leaves (dsg [n, 2 Ds] = [d inp[:, :Ds] | d inp[:, c_aggs : c_aggs + Ds]]): 16-byte loads, eight arcs in
// flight per lane, same fmaf chain per element.
__global__ void __launch_bounds__(256) k_state_grad_rows_al(int64_t n, int Ds, const float *__restrict__ dsg, const int32_t *__restrict__ sip,
                                                            const int32_t *__restrict__ sdst, const float *__restrict__ sw, float *__restrict__ d_state)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 4;
    const int cc = 4 * (int)(t & 15);
    if (r >= n || cc >= Ds) return;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int32_t e1 = sip[r + 1];
    for (int32_t e = sip[r]; e < e1; e += 8) {
        float w[8];
        float4 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int32_t ee = e + u < e1 ? e + u : e;                   // clamp: a real entry, result unused
            w[u] = sw[ee];
            x[u] = *reinterpret_cast<const float4 *>(dsg + (int64_t)sdst[ee] * 2 * Ds + Ds + cc);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (e + u < e1) {
                acc[0] = __builtin_fmaf(w[u], x[u].x, acc[0]); acc[1] = __builtin_fmaf(w[u], x[u].y, acc[1]);
                acc[2] = __builtin_fmaf(w[u], x[u].z, acc[2]); acc[3] = __builtin_fmaf(w[u], x[u].w, acc[3]);
            }
    }
    const float4 own = *reinterpret_cast<const float4 *>(dsg + r * 2 * Ds + cc);
    *reinterpret_cast<float4 *>(d_state + r * Ds + cc) = float4{own.x + acc[0], own.y + acc[1], own.z + acc[2], own.w + acc[3]};
}

__global__ void k_transpose(int ni, int no, const float *W, float *WT)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ni * no) return;
    const int i = t / no, j = t - i * no;
    WT[(size_t)j * ni + i] = W[t];
}

}   // namespace

namespace gnn_train {

// The form of this step's forward and backward calls on n rows each (Net::small_fused .. wide_bwd).  producer_dropout: the producer of
// the input rows applies the Dropout in front of the first Dense layer (net_state: k_train_input hands its mask over as keep0) and,
// where there is none and the rows are few, leaves the rows themselves to k_mlp_fwd.
void net_decide_form(Net &net, int64_t n, bool producer_dropout)
{
    const gnn_mlp *m = net.m;
    const int L = m->n_layers;
    const bool many = n > 0 && tg_many_rows(n);
    net.rows = n;
    // few rows, no Dropout between the layers, softmax at most as the last activation: all Dense layers in one launch (k_mlp_fwd)
    net.small_fused = L >= 2 && L <= GNN_FUSED_MAXL + 1 && n > 0 && !tg_many_rows(n);
    int maxpad = (m->dims[0] + 3) & ~3;
    for (int q = 1; q <= L; ++q) {
        if (q < L && (net.rate[q] != 0.0f || m->acts[q - 1] == GNN_ACT_SOFTMAX)) net.small_fused = false;
        maxpad = std::max(maxpad, (m->dims[q] + 3) & ~3);
    }
    net.small_maxpad = maxpad;
    net.small_lds = sizeof(float) * ((size_t)2 * 8 * maxpad + (size_t)256 * 8);
    if (net.small_lds > 64 * 1024) net.small_fused = false;
    // a 3-layer net without Dropout behind its first layer, on many rows: the three Dense layers in one pass (k_fwd3_split)
    net.fwd3 = many && fwd3_covers(m) && net.rate[1] == 0.0f && net.rate[2] == 0.0f && (net.rate[0] == 0.0f || producer_dropout);
    // ... and without any Dropout, every weight gradient on the matrix cores: the whole backward chain in one pass (k_bwd3_split)
    net.bwd3 = many && L == 3 && bwd3_covers(m) && net.rate[0] == 0.0f && net.rate[1] == 0.0f && net.rate[2] == 0.0f;
    for (int l = 0; l < 3 && net.bwd3; ++l) net.bwd3 = tg_wide(m->dims[l + 1], m->dims[l]) && tg_wgrad_covers(m->dims[l], m->dims[l + 1]);
#ifdef GNN_DIAG
    static const bool small_off = getenv("GNN_TRAIN_MLP_FUSED") && atoi(getenv("GNN_TRAIN_MLP_FUSED")) == 0;
    static const bool fuse_off = getenv("GNN_TRAIN_FWD3") && atoi(getenv("GNN_TRAIN_FWD3")) == 0;
    static const bool chain_off = getenv("GNN_TRAIN_BWD3") && atoi(getenv("GNN_TRAIN_BWD3")) == 0;
    if (small_off) net.small_fused = false;
    if (fuse_off) net.fwd3 = false;
    if (chain_off) net.bwd3 = false;
#endif
    net.build_input = net.small_fused && producer_dropout && net.rate[0] == 0.0f;
    // otherwise layer by layer; a wide layer on many rows: matrix cores (softmax needs the whole row: not as an epilogue)
    net.wide_fwd.assign(L, 0); net.wide_bwd.assign(L, 0);
    for (int l = 0; l < L; ++l) {
        const int ni = m->dims[l], no = m->dims[l + 1];
        net.wide_fwd[l] = many && tg_wide(ni, no) && m->acts[l] != GNN_ACT_SOFTMAX;
        net.wide_bwd[l] = many && tg_wide(no, ni) && tg_wgrad_covers(ni, no) && !(l > 0 && m->acts[l - 1] == GNN_ACT_SOFTMAX);
    }
}

// What net_forward / net_backward launch for a decided form, layer by layer (read-only: the tests' view of the decision)
void net_forms(const Net &net, int *out)
{
    const gnn_mlp *m = net.m;
    const int L = m->n_layers;
    out[0] = L; out[1] = net.build_input ? 1 : 0; out[2] = (int)tg_sweep_rows();
    for (int l = 0; l < L; ++l) {
        int *o = out + 3 + 3 * l;
        o[0] = o[1] = o[2] = GNN_FORM_PER_OP;
        if (net.rows <= 0) continue;                                     // no rows: nothing is launched
        if (net.fwd3) o[0] = GNN_FORM_CHAIN3;
        else if (net.small_fused) o[0] = GNN_FORM_MLP_FWD;
        else if (net.wide_fwd[l]) o[0] = GNN_FORM_WIDE;
        if (net.bwd3 || net.wide_bwd[l]) {
            o[1] = net.bwd3 ? GNN_FORM_CHAIN3 : GNN_FORM_WIDE;
            o[2] = tg_wgrad_bf(m->dims[l + 1]) ? GNN_FORM_WGRAD_BF : GNN_FORM_WGRAD_F32;
        }
    }
}

// zero_mem: net_zero_floats() floats the caller has zeroed (one memset for everything a step needs zeroed); rows, producer_dropout: net_decide_form
int net_setup(hipStream_t st, Buf &buf, Net &net, const gnn_mlp *m, const float *rates, const float *bn_gamma_beta_host, int max_calls, float *zero_mem,
              int64_t rows, bool producer_dropout)
{
    net.m = m;
    net.max_calls = max_calls;
    const int L = m->n_layers;
    net.rate.assign(rates, rates + L + 1);
    net_decide_form(net, rows, producer_dropout);
    net.WT.assign(L, nullptr);
    size_t off = 0;
    int rc;
    for (int l = 0; l < L; ++l) {
        const int ni = m->dims[l], no = m->dims[l + 1];
        if ((rc = buf.get(&net.WT[l], (size_t)ni * no))) return rc;
        hipLaunchKernelGGL(k_transpose, cdiv((int64_t)ni * no, 256), 256, 0, st, ni, no, m->W[l], net.WT[l]);
        HIPCHK(hipGetLastError());
        net.g_off.push_back(off); off += (size_t)ni * no;
        net.g_off.push_back(off); off += (size_t)no;
    }
    if (m->has_bn) {
        const int F = m->dims.back();
        // gamma | beta: the caller's arrays, or (NULL) the MLP's own device copy (the one the device-side optimizer updates)
        if (bn_gamma_beta_host) {
            if ((rc = buf.get(&net.gamma, (size_t)2 * F))) return rc;
            net.beta = net.gamma + F;
            HIPCHK(hipMemcpyAsync(net.gamma, bn_gamma_beta_host, sizeof(float) * 2 * F, hipMemcpyHostToDevice, st));
        } else { net.gamma = m->bn_raw; net.beta = m->bn_raw + F; }
        net.g_off.push_back(off); off += F;
        net.g_off.push_back(off); off += F;
        net.stats_all = zero_mem + off;
    }
    net.g_total = off;
    net.grads = zero_mem;
    return GNN_OK;
}

int net_freeze_bn(hipStream_t st, Buf &buf, Net &net)
{
    const gnn_mlp *m = net.m;
    if (!m->has_bn) return GNN_OK;
    const int F = m->dims.back();
    int rc;
    if ((rc = buf.get(&net.frozen, (size_t)2 * F))) return rc;
    hipLaunchKernelGGL(k_bn_frozen_prepare, cdiv(F, 64), 64, 0, st, F, m->eps, m->bn_raw, net.gamma, net.frozen);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

// training-mode forward of one Sequential on its net.rows rows (x: [rows, dims[0]]); *y_out: [rows, dims.back()].  keep0 != NULL: the Dropout
// in front of the first Dense layer has been applied by the producer of x (k_train_input), its mask is keep0.  rng: the streams of the
// masks that are not injected (masks == NULL).
// comm != NULL (sharded forward, one process per rank): the BatchNormalization statistics are those of the rows of ALL ranks.
// net.build_input: x has NOT been filled - k_mlp_fwd builds the concat rows itself (and writes them to x for the backward pass) from *build.
int net_forward(hipStream_t st, Buf &buf, Net &net, float *x, uint8_t *keep0, const uint8_t *masks, const MaskStream &rng, NetCache &c, float **y_out,
                gnn_comm *comm, const InputBuild *build, const FwdMode &mode)
{
    const gnn_mlp *m = net.m;
    const int L = m->n_layers;
    const int64_t n = net.rows;
    c.n = n;
    c.hin.assign(L, nullptr); c.a.assign(L, nullptr); c.keep.assign(L + 1, nullptr);
    float *h = x;
    size_t mask_off = 0;
    int rc;
    int l_start = 0;
    // the array that is the call's output (mode.y_dst takes its place): BatchNormalization's, else the Dropout's behind the last Dense layer, else that layer's
    const bool out_is_drop = !m->has_bn && net.rate[L] != 0.0f, out_is_dense = !m->has_bn && net.rate[L] == 0.0f;
    auto get_a = [&](int l) -> int {
        if (l == L - 1 && out_is_dense && mode.y_dst) { c.a[l] = mode.y_dst; return GNN_OK; }
        return buf.get(&c.a[l], (size_t)n * m->dims[l + 1]);
    };
    if (net.fwd3) {                                // the three Dense layers in one pass (k_fwd3_split)
        if (net.rate[0] != 0.0f) { c.keep[0] = keep0; mask_off += (size_t)n * m->dims[0]; }
        const bool keep = !mode.cacheless;         // (cache-less: a0 and a1 are neither allocated nor written)
        for (int l = keep ? 0 : 2; l < 3; ++l)
            if ((rc = get_a(l))) return rc;
        c.hin[0] = x; c.hin[1] = c.a[0]; c.hin[2] = c.a[1];
        if ((rc = launch_fwd3(st, buf, m, n, x, c.a[0], c.a[1], c.a[2]))) return rc;
        if (!keep && mode.cacheless_chain) *mode.cacheless_chain = 1;
        h = c.a[2];
        l_start = L;
    }
    for (int l = l_start; l <= L; ++l) {
        const int width = m->dims[l];
        if (net.rate[l] != 0.0f) {
            if (l == 0 && keep0) c.keep[0] = keep0;
            else {
                float *hd = l == L && out_is_drop ? mode.y_dst : nullptr;
                if ((!hd && (rc = buf.get(&hd, (size_t)n * width))) || (rc = buf.get(&c.keep[l], (size_t)n * width))) return rc;
                if (n > 0) {
                    hipLaunchKernelGGL(k_dropout_fwd, cdiv(n * width, 256), 256, 0, st, n * width, h, masks ? masks + mask_off : nullptr, net.rate[l],
                                       dropout_key(rng.seed, rng.net, rng.body, l), rng.row0 * width, c.keep[l], hd);
                    HIPCHK(hipGetLastError());
                }
                h = hd;
            }
            mask_off += (size_t)n * width;
        }
        if (l == L) break;
        // few rows, no Dropout between the layers: every Dense layer of the net in one launch (k_mlp_fwd)
        if (l == 0 && net.small_fused) {
            constexpr int R = 8;
            MlpFwd p{};
            if (net.build_input) {
                p.build = 1; p.X_out = h;
                p.Ds = build->Ds; p.c_aggs = build->c_aggs; p.tmpl = build->tmpl; p.state = build->state; p.own = build->own; p.own_prev = build->own_prev;
                p.indptr = build->indptr; p.adj_src = build->adj_src; p.adj_w = build->adj_w; p.thr = build->thr; p.flag = build->flag;
            }
            p.n = n; p.X = h;
            mlp_fwd_describe(p, m, net.small_maxpad);
            for (int q = 0; q < L; ++q) {
                if ((rc = get_a(q))) return rc;
                p.Y[q] = c.a[q];
                c.hin[q] = q == 0 ? h : c.a[q - 1];
            }
            hipLaunchKernelGGL((k_mlp_fwd<R>), cdiv(n, R), 256, net.small_lds, st, p);
            HIPCHK(hipGetLastError());
            if (m->acts[L - 1] == GNN_ACT_SOFTMAX) {
                hipLaunchKernelGGL(k_act_fwd, cdiv(n, 256), 256, 0, st, n, m->dims[L], c.a[L - 1], m->acts[L - 1], c.a[L - 1]);
                HIPCHK(hipGetLastError());
            }
            h = c.a[L - 1];
            l = L - 1;               // (the loop goes on with index L: the Dropout in front of BatchNormalization, if any)
            continue;
        }
        const int no = m->dims[l + 1];
        c.hin[l] = h;
        if ((rc = get_a(l))) return rc;
        const bool sm = m->acts[l] == GNN_ACT_SOFTMAX;          // softmax needs the whole row: separate pass, in place
        if (net.wide_fwd[l]) {                     // wide layer on many rows: matrix cores
            if ((rc = launch_gemm_f32(st, buf, n, width, no, h, m->W[l], m->b[l], m->acts[l], 0, nullptr, 0.0f, nullptr, c.a[l]))) return rc;
        } else if (n > 0) {
            constexpr int R = 8;
            const int ni_pad = (width + 3) & ~3;
            const size_t lds = dense_lds_bytes(R, ni_pad);
            if (lds > 64 * 1024) return gnn_fail(GNN_ERR_UNSUPPORTED, "layer input width %d too large", width);
            hipLaunchKernelGGL((k_dense_fwd<R>), cdiv(n, R), 256, lds, st, n, width, ni_pad, no, dense_cshift(no), h, m->W[l], m->b[l],
                               sm ? GNN_ACT_LINEAR : m->acts[l], c.a[l]);
            HIPCHK(hipGetLastError());
        }
        if (n > 0 && sm) {
            hipLaunchKernelGGL(k_act_fwd, cdiv(n, 256), 256, 0, st, n, no, c.a[l], m->acts[l], c.a[l]);
            HIPCHK(hipGetLastError());
        }
        h = c.a[l];
    }
    if (m->has_bn && net.frozen) {                 // on the moving statistics: no call is counted, no statistics are left
        const int F = m->dims.back();
        float *y = mode.y_dst;
        if (comm || mode.cacheless || mode.replay_call >= 0) return gnn_fail(GNN_ERR_STATE, "internal: a frozen BatchNormalization is one recorded body on one GPU");
        if ((rc = buf.get(&c.xhat, (size_t)n * F)) || (!y && (rc = buf.get(&y, (size_t)n * F)))) return rc;
        if (n > 0) {
            hipLaunchKernelGGL(k_bn_apply_frozen, elementwise_grid(n * F), 256, 0, st, n, F, h, m->bn_raw + 2 * F, net.frozen, net.gamma, net.beta, c.xhat, y);
            HIPCHK(hipGetLastError());
        }
        h = y;
    } else if (m->has_bn) {
        const int F = m->dims.back();
        float *y = mode.y_dst, *stats_out = nullptr;
        const bool want_xhat = !mode.cacheless || comm;
        if ((want_xhat && (rc = buf.get(&c.xhat, (size_t)n * F))) || (!y && (rc = buf.get(&y, (size_t)n * F)))) return rc;
        if (mode.replay_call >= 0) {               // a repeated call: its slot as the first pass left it, the recomputed statistics to scratch
            if (mode.replay_call >= net.calls || comm) return gnn_fail(GNN_ERR_STATE, "internal: replay of BatchNormalization call %d of %d", mode.replay_call, net.calls);
            c.stats = net.stats_all + (size_t)mode.replay_call * 2 * F;
            if ((rc = buf.get(&stats_out, (size_t)2 * F))) return rc;
        } else {
            if (net.calls >= std::max(1, net.max_calls)) return gnn_fail(GNN_ERR_STATE, "more BatchNormalization calls than announced");
            c.stats = stats_out = net.stats_all + (size_t)net.calls++ * 2 * F;
        }
        if (comm) {
            // every rank takes part in the exchange, also one without rows (count 0)
            float *tri = nullptr, *tri_all = nullptr;
            if ((rc = buf.get(&tri, (size_t)3 * F)) || (rc = buf.get(&tri_all, (size_t)3 * F * comm->world))) return rc;
            const int64_t rpb = n > 0 ? rows_per_block(n) : 1;
            const int parts = n > 0 ? (int)cdiv(n, rpb) : 0;
            float *part = nullptr;
            if ((rc = buf.get(&part, (size_t)std::max(parts, 1) * 2 * F))) return rc;
            if (n > 0) {
                const int cs = column_shift(F);
                hipLaunchKernelGGL(k_bn_stats, dim3(cdiv(F, 1 << cs), parts), 256, 0, st, n, F, cs, h, part, rpb);
            }
            hipLaunchKernelGGL(k_bn_local, cdiv(F, 256), 256, 0, st, n, F, part, parts, rpb, tri);
            HIPCHK(hipGetLastError());
            if ((rc = gnn_comm_allgather32(comm, tri, tri_all, (size_t)3 * F, st))) return rc;
            hipLaunchKernelGGL(k_bn_apply_ext, n > 0 ? elementwise_grid(n * F) : 1, 256, sizeof(float) * 2 * F, st, n, F, h, tri_all, comm->world, m->eps, net.gamma,
                               net.beta, c.xhat, y, c.stats);
            HIPCHK(hipGetLastError());
        } else if (n > 0) {
            const int64_t rpb = rows_per_block(n);
            const int parts = (int)cdiv(n, rpb);
            float *part = nullptr;
            if ((rc = buf.get(&part, (size_t)parts * 2 * F))) return rc;
            const int cs = column_shift(F);
            hipLaunchKernelGGL(k_bn_stats, dim3(cdiv(F, 1 << cs), parts), 256, 0, st, n, F, cs, h, part, rpb);
            if (want_xhat)
                hipLaunchKernelGGL(k_bn_apply<true>, elementwise_grid(n * F), 256, sizeof(float) * 2 * F, st, n, F, cs, h, part, parts, rpb, m->eps, net.gamma,
                                   net.beta, c.xhat, y, stats_out);
            else
                hipLaunchKernelGGL(k_bn_apply<false>, elementwise_grid(n * F), 256, sizeof(float) * 2 * F, st, n, F, cs, h, part, parts, rpb, m->eps, net.gamma,
                                   net.beta, static_cast<float *>(nullptr), y, stats_out);
            HIPCHK(hipGetLastError());
        }
        h = y;
    }
    *y_out = h;
    return GNN_OK;
}

// back-propagation through one Sequential: d is d loss / d y on entry ([n, dims.back()], overwritten); on return *dx_out is
// d loss / d x ([n, dims[0]]); weight gradients are ADDED into net.grads (one sum over the call's chunk partials)
// comm != NULL (sharded backward, one process per rank): the sums of BatchNormalization's backward pass are those of the rows of ALL
// ranks (n_global of them); the weight gradients stay this rank's share (train_backward adds the shares up at the end).
// wgrad = false (an adjoint iteration of the fixed-point gradient, gnn_train_adjoint.hip): d x alone - after the chain no weight-gradient
// kernel, of a wide layer only the product with W^T, of k_layer_bwd only its row blocks, and no sum of the chunk partials.
int net_backward(hipStream_t st, Buf &buf, Net &net, const NetCache &c, float *d, float **dx_out, const StateGradJob *job,
                 gnn_comm *comm, int64_t n_global, bool wgrad)
{
    const gnn_mlp *m = net.m;
    const int L = m->n_layers;
    const int64_t n = c.n;
    int rc;
    if (n <= 0) {                              // no rows: no gradient; d x is empty
        if (comm && m->has_bn) {               // ... but the other ranks wait for this one's (zero) share of the sums
            const int F = m->dims.back();
            float *loc = nullptr, *all = nullptr;
            if ((rc = buf.get(&loc, (size_t)2 * F)) || (rc = buf.get(&all, (size_t)2 * F * comm->world))) return rc;
            HIPCHK(hipMemsetAsync(loc, 0, sizeof(float) * 2 * F, st));
            if ((rc = gnn_comm_allgather32(comm, loc, all, (size_t)2 * F, st))) return rc;
        }
        *dx_out = d;
        return GNN_OK;
    }
    const int64_t rpb = rows_per_block(n);
    const int parts = (int)cdiv(n, rpb);
    const bool frozen = m->has_bn && net.frozen != nullptr;
    if (!wgrad && m->has_bn && !frozen) return gnn_fail(GNN_ERR_STATE, "internal: an input-gradient-only backward pass through BatchNormalization");
    if (wgrad && net.part_rows != n) {
        if ((rc = buf.get(&net.part, (size_t)parts * net.g_total))) return rc;
        net.part_rows = n;
    }
    const int64_t ps = (int64_t)net.g_total;
    const int act_last = m->acts[L - 1];
    // the derivative of the last activation rides on the BatchNormalization pass when nothing sits between them
    bool last_act_done = false;
    if (frozen) {
        // d gamma / d beta from the chunk partials as below (weight pass only); d h = d s_j has no mean or variance terms
        const int F = m->dims.back(), cs = column_shift(F);
        const bool fuse = net.rate[L] == 0.0f && act_last != GNN_ACT_SOFTMAX;
        if (comm) return gnn_fail(GNN_ERR_STATE, "internal: a frozen BatchNormalization is single-GPU");
        if (wgrad) hipLaunchKernelGGL(k_colreduce2, dim3(cdiv(F, 1 << cs), parts), 256, 0, st, n, F, cs, d, c.xhat, net.part + net.g_off[2 * L], net.part + net.g_off[2 * L + 1], ps, rpb);
        hipLaunchKernelGGL(k_bn_bwd_frozen, elementwise_grid(n * F), 256, 0, st, n, F, d, net.frozen + F, c.a[L - 1], fuse ? act_last : -1);
        HIPCHK(hipGetLastError());
        last_act_done = fuse;
    } else if (m->has_bn) {
        const int F = m->dims.back(), cs = column_shift(F);
        float *p_dyx = net.part + net.g_off[2 * L], *p_dy = net.part + net.g_off[2 * L + 1];
        const bool fuse = net.rate[L] == 0.0f && act_last != GNN_ACT_SOFTMAX;
        hipLaunchKernelGGL(k_colreduce2, dim3(cdiv(F, 1 << cs), parts), 256, 0, st, n, F, cs, d, c.xhat, p_dyx, p_dy, ps, rpb);
        if (comm) {
            // this rank's sums [sum d y xhat | sum d y] (adjacent in the gradient vector: they ARE the gamma / beta gradients), those of
            // all ranks all-gathered, added in rank order by every block of the apply kernel
            float *loc = nullptr, *all = nullptr;
            if ((rc = buf.get(&loc, (size_t)2 * F)) || (rc = buf.get(&all, (size_t)2 * F * comm->world))) return rc;
            hipLaunchKernelGGL(k_sum_strided, cdiv(2 * F, 256), 256, 0, st, parts, ps, p_dyx, 2 * F, loc);
            HIPCHK(hipGetLastError());
            if ((rc = gnn_comm_allgather32(comm, loc, all, (size_t)2 * F, st))) return rc;
            hipLaunchKernelGGL(k_bn_bwd_apply, elementwise_grid(n * F), 256, sizeof(float) * 2 * F, st, n, F, cs, d, c.xhat, net.gamma, c.stats, m->eps,
                               all, all + F, (int64_t)2 * F, comm->world, c.a[L - 1], fuse ? act_last : -1, n_global);
        } else
            hipLaunchKernelGGL(k_bn_bwd_apply, elementwise_grid(n * F), 256, sizeof(float) * 2 * F, st, n, F, cs, d, c.xhat, net.gamma, c.stats, m->eps,
                               p_dyx, p_dy, ps, parts, c.a[L - 1], fuse ? act_last : -1, (int64_t)0);
        HIPCHK(hipGetLastError());
        last_act_done = fuse;
    }
    if (net.rate[L] != 0.0f) {
        const int F = m->dims.back();
        hipLaunchKernelGGL(k_dropout_bwd, cdiv(n * F, 256), 256, 0, st, n * F, c.keep[L], net.rate[L], d);
        HIPCHK(hipGetLastError());
    }
    if (!last_act_done) {
        const int no = m->dims[L];
        const bool sm = act_last == GNN_ACT_SOFTMAX;
        if (sm || act_last != GNN_ACT_LINEAR) {
            hipLaunchKernelGGL(k_act_bwd, cdiv(sm ? n : n * no, 256), 256, 0, st, n, no, d, c.a[L - 1], act_last);
            HIPCHK(hipGetLastError());
        }
    }
    // d is d loss / d z of layer l at the top of every pass
    // a 3-layer net without Dropout on many rows: the whole chain d z2 -> d z1 -> d z0 -> d inp in one pass (k_bwd3_split), then the three weight gradients
    float *dsg = nullptr;
    const bool chain3 = net.bwd3;
    if (chain3) {
        float *dz1 = nullptr, *dz0 = nullptr, *dinp = nullptr;
        if ((rc = buf.get(&dz1, (size_t)n * m->dims[2])) || (rc = buf.get(&dz0, (size_t)n * m->dims[1])) || (rc = buf.get(&dinp, (size_t)n * m->dims[0]))) return rc;
        // the state gradient of this body reads two column blocks of d inp: the chain leaves them once more as aligned rows
        if (job && job->N == n && state_rows16(job->Ds, job->N) && job->in_s == m->dims[0] && (rc = buf.get(&dsg, (size_t)n * 2 * job->Ds))) return rc;
        if ((rc = launch_bwd3(st, buf, m, net.WT.data(), n, d, c.a[1], c.a[0], dz1, dz0, dinp, dsg, job ? job->Ds : 0, job ? job->c_aggs : 0))) return rc;
        const float *dzs[3] = {dz0, dz1, d};
        for (int l = 2; l >= 0 && wgrad; --l)
            if ((rc = launch_wgrad_f32(st, n, rpb, parts, ps, m->dims[l], m->dims[l + 1], c.hin[l], dzs[l], net.part + net.g_off[2 * l]))) return rc;
        d = dinp;
    }
    for (int l = chain3 ? -1 : L - 1; l >= 0; --l) {
        const int ni = m->dims[l], no = m->dims[l + 1];
        float *dprev = nullptr;
        if ((rc = buf.get(&dprev, (size_t)n * ni))) return rc;
        // weight + bias gradient tiles and d h_in = d z . W^T (back through Dropout l and, l > 0, the activation of layer l - 1) in one launch
        const int act_prev = l > 0 ? m->acts[l - 1] : -1;
        const bool prev_sm = act_prev == GNN_ACT_SOFTMAX;
        if (net.wide_bwd[l]) {                     // both products of a wide layer on the matrix cores
            if (wgrad && (rc = launch_wgrad_f32(st, n, rpb, parts, ps, ni, no, c.hin[l], d, net.part + net.g_off[2 * l]))) return rc;
            if ((rc = launch_gemm_f32(st, buf, n, no, ni, d, net.WT[l], nullptr, act_prev, 1, net.rate[l] != 0.0f ? c.keep[l] : nullptr, net.rate[l],
                                      l > 0 ? c.a[l - 1] : nullptr, dprev))) return rc;
            d = dprev;
            continue;
        }
        constexpr int R = 8;
        LayerBwd p;
        p.n = n; p.rows_per_block = rpb; p.pstride = ps;
        p.n_in = ni; p.n_out = no; p.n_out_pad = (no + 3) & ~3; p.act = prev_sm ? -1 : act_prev;
        p.wg_bx = (int)cdiv(ni + 1, GNN_WG_TILE); p.wg_by = (int)cdiv(no, GNN_WG_TILE); p.wg_blocks = wgrad ? p.wg_bx * p.wg_by * parts : 0;
        p.rate = net.rate[l];
        p.H = c.hin[l]; p.DZ = d; p.WT = net.WT[l]; p.a_prev = l > 0 ? c.a[l - 1] : nullptr;
        p.keep = net.rate[l] != 0.0f ? c.keep[l] : nullptr;
        p.part = wgrad ? net.part + net.g_off[2 * l] : nullptr; p.dprev = dprev;
        p.cshift = dense_cshift(ni);
        const size_t lds = std::max(dense_lds_bytes(R, p.n_out_pad), sizeof(float) * 2 * 64 * GNN_WG_LD);
        if (lds > 64 * 1024) return gnn_fail(GNN_ERR_UNSUPPORTED, "layer width %d too large", no);
        hipLaunchKernelGGL((k_layer_bwd<R>), (unsigned)(p.wg_blocks + cdiv(n, R)), 256, lds, st, p);
        if (prev_sm) hipLaunchKernelGGL(k_act_bwd, cdiv(n, 256), 256, 0, st, n, ni, dprev, c.a[l - 1], act_prev);
        HIPCHK(hipGetLastError());
        d = dprev;
    }
    const unsigned sum_blocks = cdiv((int64_t)net.g_total, 64);
    if (job && job->pw_inv) {                      // an iteration of the contraction estimate: z_next = the state gradient * *pw_inv, with its squared norm
        if (wgrad) return gnn_fail(GNN_ERR_STATE, "internal: a power iteration takes no weight gradients");
        if ((rc = launch_power_gather(st, *job, dsg ? dsg : d, dsg != nullptr, job->form_out))) return rc;
    } else if (job && job->g && job->anderson) {   // an iteration of the Anderson-accelerated adjoint solve: G = g + the state gradient, residual, slot, gate, partial dots
        if (wgrad) return gnn_fail(GNN_ERR_STATE, "internal: an adjoint iteration takes no weight gradients");
        if ((rc = launch_anderson_gather(st, *job, dsg ? dsg : d, dsg != nullptr, job->form_out))) return rc;
    } else if (job && job->g) {                    // an adjoint iteration: z_next = g + the state gradient, with the iteration's gate
        if (wgrad) return gnn_fail(GNN_ERR_STATE, "internal: an adjoint iteration takes no weight gradients");
        if ((rc = launch_adjoint_gather(st, *job, dsg ? dsg : d, dsg != nullptr, job->form_out))) return rc;
    } else if (!wgrad) {
        if (job) return gnn_fail(GNN_ERR_STATE, "internal: a state gradient without weight gradients is an adjoint iteration");
    } else if (job && dsg) {
        hipLaunchKernelGGL(k_state_grad_rows_al, cdiv(job->N * 16, 256), 256, 0, st, job->N, job->Ds, dsg, job->sip, job->sdst, job->sw, job->d_state);
        hipLaunchKernelGGL(k_sum_parts, sum_blocks, 256, 0, st, parts, (int64_t)net.g_total, net.part, net.grads);
    } else if (job && state_rows16(job->Ds, job->N)) {
        hipLaunchKernelGGL(k_state_grad_rows, cdiv(job->N * 16, 256), 256, 0, st, job->N, job->Ds, job->in_s, job->c_aggs, d, job->sip, job->sdst, job->sw, job->d_state);
        hipLaunchKernelGGL(k_sum_parts, sum_blocks, 256, 0, st, parts, (int64_t)net.g_total, net.part, net.grads);
    } else if (job && job->N > 0) {
        const int sg = (int)cdiv(job->N * job->Ds, 256);
        hipLaunchKernelGGL(k_state_grad_sum, sg + sum_blocks, 256, 0, st, sg, job->N, job->Ds, job->in_s, job->c_aggs, d, job->sip, job->sdst, job->sw,
                           job->d_state, parts, (int64_t)net.g_total, net.part, net.grads);
    } else
        hipLaunchKernelGGL(k_sum_parts, sum_blocks, 256, 0, st, parts, (int64_t)net.g_total, net.part, net.grads);
    HIPCHK(hipGetLastError());
    *dx_out = d;
    return GNN_OK;
}

int net_sum_parts(hipStream_t st, int parts, int64_t count, const float *part, float *out)
{
    hipLaunchKernelGGL(k_sum_parts, cdiv(count, 64), 256, 0, st, parts, count, part, out);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

}   // namespace gnn_train

// The form a net of this description would take on n_rows rows (include/gnn_hip.h): host code, no device
extern "C" int gnn_train_forms(int n_layers, const int *dims, const int *acts, const float *rates, int64_t n_rows, int producer_dropout, int *out)
{
    ARGCHK(n_layers >= 1 && n_layers <= 16 && dims && acts && rates && n_rows >= 0 && out, "bad arguments");
    gnn_mlp m;
    m.n_layers = n_layers;
    m.dims.assign(dims, dims + n_layers + 1);
    m.acts.assign(acts, acts + n_layers);
    for (int l = 0; l <= n_layers; ++l) ARGCHK(m.dims[l] >= 1, "bad layer width");
    for (int l = 0; l < n_layers; ++l) ARGCHK(m.acts[l] >= GNN_ACT_LINEAR && m.acts[l] <= GNN_ACT_SOFTMAX, "bad activation code");
    gnn_train::Net net;
    net.m = &m;
    net.rate.assign(rates, rates + n_layers + 1);
    gnn_train::net_decide_form(net, n_rows, producer_dropout != 0);
    gnn_train::net_forms(net, out);
    return GNN_OK;
}

// Whether a net_state of this description takes the persistent training forward on n_rows rows and max_iter bodies, as far as the net,
// the rows and the byte cap decide (include/gnn_hip.h): host code, no device
extern "C" int gnn_train_persistent_form(int n_layers, const int *dims, const int *acts, const float *rates, int64_t n_rows, int max_iter, int *out)
{
    ARGCHK(n_layers >= 1 && n_layers <= 16 && dims && acts && rates && n_rows >= 0 && max_iter >= 0 && out, "bad arguments");
    gnn_mlp m;
    m.n_layers = n_layers;
    m.dims.assign(dims, dims + n_layers + 1);
    m.acts.assign(acts, acts + n_layers);
    for (int l = 0; l <= n_layers; ++l) ARGCHK(m.dims[l] >= 1, "bad layer width");
    for (int l = 0; l < n_layers; ++l) ARGCHK(m.acts[l] >= GNN_ACT_LINEAR && m.acts[l] <= GNN_ACT_SOFTMAX, "bad activation code");
    gnn_train::Net net;
    net.m = &m;
    net.rate.assign(rates, rates + n_layers + 1);
    gnn_train::net_decide_form(net, n_rows, true);
    const gnn_train::SmallTrainForm f = gnn_train::small_train_form(net, max_iter);
    out[0] = f.ok ? 1 : 0;
    out[1] = f.ok ? f.grid : 0;
    out[2] = f.ok ? f.rows : 0;
    out[3] = f.ok ? (int)f.lds : 0;
    out[4] = (int)std::min<size_t>(f.cap_body_bytes, 0x7fffffff);
    return GNN_OK;
}
