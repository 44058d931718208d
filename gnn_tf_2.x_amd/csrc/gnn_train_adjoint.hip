// The gradient at the fixed point (gradient mode 1 of a loop, include/gnn_hip.h: gnn_loop_set_gradient_mode): the hot path of its backward
// pass is the adjoint iteration z <- g + J^T z on ONE recorded body of net_state.  J^T z is that body's input-gradient-only backward pass
// (net_backward with wgrad = false, gnn_train_net.hip) followed by the gather of this unit, which folds the own-state columns and the
// aggregated-state columns of d concat back onto the state rows over the adjacency by source, adds g, and evaluates the iteration's gate
// in the same pass.  The step itself (forward through the inference Loop, the recorded body, the host's look at the gates, the one
// weight-gradient pass with z_final) is train_forward / train_backward of gnn_train.hip.
//
// Arithmetic: per element the fmaf chain over the arcs in stored order that k_state_grad_rows / _al / _sum run (acc starts at 0), then
// z_next = g + (own + acc).  The gate is the forward condition's: a node moves when sqrt(sum (z_next - z_prev)^2) > thr sqrt(sum z_prev^2);
// the two sums of a row are partial sums of its 16 lanes (ascending columns within a lane) added by a fixed butterfly, so the bits depend
// on neither grid nor timing.  No float atomics.
#include <cmath>

#include "gnn_train.h"

using namespace gnn_train;

namespace {

struct AdjGather {
    int64_t n;
    int Ds, in_s, c_aggs;
    const float *u;               // d concat [n, in_s], or (aligned form) dsg [n, 2 Ds] = [own-state columns | aggregated-state columns]
    const int32_t *sip, *sdst;
    const float *sw;
    const float *g, *z_prev;
    float *z_next, *work;
    float thr;
    const int *gate_prev;
    int *gate;
};

// the sums of a row's 16 lanes, the same bits in every lane (each step adds the two halves of a pair: a + b == b + a)
__device__ __forceinline__ float row16_sum(float v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 16);
    return v;
}

// State rows of whole 16-byte pieces (Ds % 4 == 0, Ds <= 64): 16 lanes per row, four columns per lane.  ALIGNED: u is the dsg copy of
// k_bwd3_split (16-byte loads, eight arcs in flight per lane, as k_state_grad_rows_al); else the two column blocks of d concat itself (four
// arcs in flight, as k_state_grad_rows).
template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_adjoint_gather_rows(const AdjGather p)
{
    const bool open = gnn_gate_open_block(p.gate_prev, 1);          // (every thread: it holds barriers)
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 4;
    const int cc = 4 * (int)(t & 15), Ds = p.Ds;
    float dist = 0.0f, nrm = 0.0f;
    if (r < p.n && cc < Ds) {
        const float4 zp = *reinterpret_cast<const float4 *>(p.z_prev + r * Ds + cc);
        float4 zn = zp;
        if (open) {
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            float4 own;
            const int32_t e1 = p.sip[r + 1];
            if (ALIGNED) {
                for (int32_t e = p.sip[r]; e < e1; e += 8) {
                    float w[8];
                    float4 x[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int32_t ee = e + q < e1 ? e + q : e;       // clamp: a real entry, result unused
                        w[q] = p.sw[ee];
                        x[q] = *reinterpret_cast<const float4 *>(p.u + (int64_t)p.sdst[ee] * 2 * Ds + Ds + cc);
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (e + q < e1) {
                            acc[0] = __builtin_fmaf(w[q], x[q].x, acc[0]); acc[1] = __builtin_fmaf(w[q], x[q].y, acc[1]);
                            acc[2] = __builtin_fmaf(w[q], x[q].z, acc[2]); acc[3] = __builtin_fmaf(w[q], x[q].w, acc[3]);
                        }
                }
                own = *reinterpret_cast<const float4 *>(p.u + r * 2 * Ds + cc);
            } else {
                for (int32_t e = p.sip[r]; e < e1; e += 4) {
                    float w[4], x[4][4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bool in = e + q < e1;
                        w[q] = in ? p.sw[e + q] : 0.0f;
                        const float *src = p.u + (int64_t)(in ? p.sdst[e + q] : 0) * p.in_s + p.c_aggs + cc;
#pragma unroll
                        for (int v = 0; v < 4; ++v) x[q][v] = in ? src[v] : 0.0f;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (e + q < e1) {
#pragma unroll
                            for (int v = 0; v < 4; ++v) acc[v] = __builtin_fmaf(w[q], x[q][v], acc[v]);
                        }
                }
                const float *o = p.u + r * p.in_s + cc;
                own = float4{o[0], o[1], o[2], o[3]};
            }
            const float4 g4 = *reinterpret_cast<const float4 *>(p.g + r * Ds + cc);
            zn = float4{g4.x + (own.x + acc[0]), g4.y + (own.y + acc[1]), g4.z + (own.z + acc[2]), g4.w + (own.w + acc[3])};
        }
        *reinterpret_cast<float4 *>(p.z_next + r * Ds + cc) = zn;
        *reinterpret_cast<float4 *>(p.work + r * Ds + cc) = zn;
        const float d0 = zn.x - zp.x, d1 = zn.y - zp.y, d2 = zn.z - zp.z, d3 = zn.w - zp.w;
        dist = dist + d0 * d0; nrm = nrm + zp.x * zp.x;
        dist = dist + d1 * d1; nrm = nrm + zp.y * zp.y;
        dist = dist + d2 * d2; nrm = nrm + zp.z * zp.z;
        dist = dist + d3 * d3; nrm = nrm + zp.w * zp.w;
    }
    dist = row16_sum(dist); nrm = row16_sum(nrm);
    const int moved = open && r < p.n && sqrtf(dist) > p.thr * sqrtf(nrm);
    if (__any(moved) && (threadIdx.x & 63) == 0) gnn_flag_raise(p.gate);
}

// Any state width: 16 lanes per row, lane j takes the columns j, j + 16, ...; per column the chain of k_state_grad_sum (four arcs in flight).
__global__ void __launch_bounds__(256) k_adjoint_gather(const AdjGather p)
{
    const bool open = gnn_gate_open_block(p.gate_prev, 1);
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 4;
    const int j = (int)(t & 15), Ds = p.Ds;
    float dist = 0.0f, nrm = 0.0f;
    if (r < p.n) {
        const int32_t e0 = p.sip[r], e1 = p.sip[r + 1];
        for (int c = j; c < Ds; c += 16) {
            const float zp = p.z_prev[r * Ds + c];
            float zn = zp;
            if (open) {
                float acc = 0.0f;
                for (int32_t e = e0; e < e1; e += 4) {
                    float w[4], x[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bool in = e + q < e1;
                        w[q] = in ? p.sw[e + q] : 0.0f;
                        x[q] = in ? p.u[(int64_t)p.sdst[e + q] * p.in_s + p.c_aggs + c] : 0.0f;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) if (e + q < e1) acc = __builtin_fmaf(w[q], x[q], acc);
                }
                zn = p.g[r * Ds + c] + (p.u[r * p.in_s + c] + acc);
            }
            p.z_next[r * Ds + c] = zn;
            p.work[r * Ds + c] = zn;
            const float d = zn - zp;
            dist = dist + d * d;
            nrm = nrm + zp * zp;
        }
    }
    dist = row16_sum(dist); nrm = row16_sum(nrm);
    const int moved = open && r < p.n && sqrtf(dist) > p.thr * sqrtf(nrm);
    if (__any(moved) && (threadIdx.x & 63) == 0) gnn_flag_raise(p.gate);
}

// ---- power iteration on J^T (the contraction estimate, include/gnn_hip.h: gnn_loop_contraction_estimate) ------------------------------------------
// w_t = (J^T w_{t-1}) * inv with inv = 1 / |w_{t-1}| read from one device float: the gathers above without g, z_prev and the gate.  The squared
// norm of w_t is formed in the same pass, in a fixed order: per lane over its ascending columns, the 16 lanes of a row by row16_sum, the 16 rows of a
// block in row order through LDS - ONE float per block; k_power_finalize adds the blocks' floats in block order, in double.  No float atomics.
struct PowGather {
    int64_t n;
    int Ds, in_s, c_aggs;
    const float *u;               // as AdjGather::u
    const int32_t *sip, *sdst;
    const float *sw;
    const float *inv;
    float *w_next, *work, *part;
};

// the block's 16 row sums (the same bits in the 16 lanes of a row) -> part[block], rows in ascending order; every thread of the block calls it
__device__ __forceinline__ void power_block_sum(float row_sq, float *part)
{
    __shared__ float rows[16];
    if ((threadIdx.x & 15) == 0) rows[threadIdx.x >> 4] = row_sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = rows[0];
#pragma unroll
        for (int q = 1; q < 16; ++q) s = s + rows[q];
        part[blockIdx.x] = s;
    }
}

// the shapes of k_adjoint_gather_rows<ALIGNED>
template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_power_gather_rows(const PowGather p)
{
    const float inv = *p.inv;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 4;
    const int cc = 4 * (int)(t & 15), Ds = p.Ds;
    float sq = 0.0f;
    if (r < p.n && cc < Ds) {
        if (inv != 0.0f) {
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            float4 own;
            const int32_t e1 = p.sip[r + 1];
            if (ALIGNED) {
                for (int32_t e = p.sip[r]; e < e1; e += 8) {
                    float w[8];
                    float4 x[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int32_t ee = e + q < e1 ? e + q : e;       // clamp: a real entry, result unused
                        w[q] = p.sw[ee];
                        x[q] = *reinterpret_cast<const float4 *>(p.u + (int64_t)p.sdst[ee] * 2 * Ds + Ds + cc);
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (e + q < e1) {
                            acc[0] = __builtin_fmaf(w[q], x[q].x, acc[0]); acc[1] = __builtin_fmaf(w[q], x[q].y, acc[1]);
                            acc[2] = __builtin_fmaf(w[q], x[q].z, acc[2]); acc[3] = __builtin_fmaf(w[q], x[q].w, acc[3]);
                        }
                }
                own = *reinterpret_cast<const float4 *>(p.u + r * 2 * Ds + cc);
            } else {
                for (int32_t e = p.sip[r]; e < e1; e += 4) {
                    float w[4], x[4][4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bool in = e + q < e1;
                        w[q] = in ? p.sw[e + q] : 0.0f;
                        const float *src = p.u + (int64_t)(in ? p.sdst[e + q] : 0) * p.in_s + p.c_aggs + cc;
#pragma unroll
                        for (int v = 0; v < 4; ++v) x[q][v] = in ? src[v] : 0.0f;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (e + q < e1) {
#pragma unroll
                            for (int v = 0; v < 4; ++v) acc[v] = __builtin_fmaf(w[q], x[q][v], acc[v]);
                        }
                }
                const float *o = p.u + r * p.in_s + cc;
                own = float4{o[0], o[1], o[2], o[3]};
            }
            const float4 wn = float4{(own.x + acc[0]) * inv, (own.y + acc[1]) * inv, (own.z + acc[2]) * inv, (own.w + acc[3]) * inv};
            *reinterpret_cast<float4 *>(p.w_next + r * Ds + cc) = wn;
            *reinterpret_cast<float4 *>(p.work + r * Ds + cc) = wn;
            sq = sq + wn.x * wn.x; sq = sq + wn.y * wn.y; sq = sq + wn.z * wn.z; sq = sq + wn.w * wn.w;
        } else
            *reinterpret_cast<float4 *>(p.work + r * Ds + cc) = float4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    power_block_sum(row16_sum(sq), p.part);
}

// the shape of k_adjoint_gather
__global__ void __launch_bounds__(256) k_power_gather(const PowGather p)
{
    const float inv = *p.inv;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 4;
    const int j = (int)(t & 15), Ds = p.Ds;
    float sq = 0.0f;
    if (r < p.n) {
        const int32_t e0 = p.sip[r], e1 = p.sip[r + 1];
        for (int c = j; c < Ds; c += 16) {
            if (inv == 0.0f) { p.work[r * Ds + c] = 0.0f; continue; }
            float acc = 0.0f;
            for (int32_t e = e0; e < e1; e += 4) {
                float w[4], x[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool in = e + q < e1;
                    w[q] = in ? p.sw[e + q] : 0.0f;
                    x[q] = in ? p.u[(int64_t)p.sdst[e + q] * p.in_s + p.c_aggs + c] : 0.0f;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) if (e + q < e1) acc = __builtin_fmaf(w[q], x[q], acc);
            }
            const float wn = (p.u[r * p.in_s + c] + acc) * inv;
            p.w_next[r * Ds + c] = wn;
            p.work[r * Ds + c] = wn;
            sq = sq + wn * wn;
        }
    }
    power_block_sum(row16_sum(sq), p.part);
}

// w_0: lane j of a row takes the columns j, j + 16, ...; fill: element i = r Ds + c is a normal draw of the counter RNG (mix64 of gnn_train.h, Box-Muller
// on the two 24-bit halves of one word), else v holds the caller's vector; copied to `work`, with the block's partial squared norm
__global__ void __launch_bounds__(256) k_power_start(int64_t n, int Ds, int fill, uint64_t seed, float *v, float *work, float *part)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 4;
    const int j = (int)(t & 15);
    float sq = 0.0f;
    if (r < n)
        for (int c = j; c < Ds; c += 16) {
            const int64_t i = r * Ds + c;
            float x;
            if (fill) {
                const uint64_t h = mix64(mix64(seed) ^ mix64((uint64_t)i));
                const float u1 = ((float)(uint32_t)(h >> 40) + 1.0f) * (1.0f / 16777217.0f);
                const float u2 = (float)(uint32_t)((h >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);
                x = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
                v[i] = x;
            } else
                x = v[i];
            work[i] = x;
            sq = sq + x * x;
        }
    power_block_sum(row16_sum(sq), part);
}

// One block.  Thread i adds the partials of blocks [i c, (i + 1) c), c = ceil(blocks / 256), in block order in double; thread 0 adds the 256 sums
// in thread order: the blocks in ascending order, in 256 runs.  norm = sqrt(sum); *inv = 1 / norm for the next gather, 0 when the norm is 0 or
// not finite - the iteration stops there, and every later gather hands nothing on.
__global__ void __launch_bounds__(256) k_power_finalize(unsigned blocks, const float *part, float *norm_out, float *inv)
{
    __shared__ double sums[256];
    const unsigned c = (blocks + 255) / 256, b0 = threadIdx.x * c, b1 = b0 + c < blocks ? b0 + c : blocks;
    double s = 0.0;
    for (unsigned b = b0; b < b1; ++b) s = s + (double)part[b];
    sums[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = sums[0];
        for (int q = 1; q < 256; ++q) tot = tot + sums[q];
        const float norm = (float)sqrt(tot);
        *norm_out = norm;
        const float r = norm > 0.0f && norm <= 3.402823466e+38f ? (float)(1.0 / (double)norm) : 0.0f;
        *inv = r <= 3.402823466e+38f ? r : 0.0f;                   // (a subnormal norm: its reciprocal is no float)
    }
}

// One launch per adjoint iteration for narrow nets (at most three Dense layers of at most 64 outputs behind a concat of at most 96 columns,
// fewer than 4,096 rows: the step is bound by its launch count there).  Launch L: a block of 256 threads owns ADJ_NARROW_ROWS = 16 rows, 16 lanes
// per row.  (1) gather != 0: z_L of its rows = g + (u_{L-1}[r, :Ds] + sum over the arcs r -> dst of w u_{L-1}[dst, Ds:]) from the PREVIOUS
// launch's u [n, 2 Ds] (lane j: columns j, j + 16, ..; the chain of k_adjoint_gather), stored to z_cur, with the gate of iteration L - 1
// against z_prev; behind a closed gate_prev z_L = z_prev and nothing is raised.  gather == 0: z_L is read from z_cur.  (2) the whole chain
// d = z_L (.) act'(a_last), then per layer from the last to the first d <- (d . W^T) (.) act'(a of the layer below) with the layer's transposed
// weights staged in LDS (one layer at a time: 24 KB at most) and d in LDS, float32 fmaf over ascending k; of the first layer only the own-state
// and aggregated-state columns are produced, straight into u_out [n, 2 Ds] (the other buffer of the pair).  No grid barrier: an iteration is a launch.
__global__ void __launch_bounds__(256) k_adjoint_narrow(const AdjNarrow p)
{
    __shared__ float wt[ADJ_NARROW_MAXIN * ADJ_NARROW_MAXW];
    __shared__ float db[2][ADJ_NARROW_ROWS * ADJ_NARROW_MAXW];
    const int lr = threadIdx.x >> 4, j = threadIdx.x & 15;
    const int64_t r = (int64_t)blockIdx.x * ADJ_NARROW_ROWS + lr;
    const int Ds = p.Ds, L = p.L;
    const bool live = r < p.n;
    bool open = true;
    if (p.gather) open = gnn_gate_open_block(p.gate_prev, 1);       // (uniform branch; every thread: it holds barriers)
    float dist = 0.0f, nrm = 0.0f;
    for (int c = j; c < Ds; c += 16) {
        float zc = 0.0f;
        if (live) {
            if (p.gather) {
                const float zp = p.z_prev[r * Ds + c];
                zc = zp;
                if (open) {
                    float acc = 0.0f;
                    const int32_t e1 = p.sip[r + 1];
                    for (int32_t e = p.sip[r]; e < e1; e += 4) {
                        float w[4], x[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const bool in = e + q < e1;
                            w[q] = in ? p.sw[e + q] : 0.0f;
                            x[q] = in ? p.u_prev[(int64_t)p.sdst[e + q] * 2 * Ds + Ds + c] : 0.0f;
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) if (e + q < e1) acc = __builtin_fmaf(w[q], x[q], acc);
                    }
                    zc = p.g[r * Ds + c] + (p.u_prev[r * 2 * Ds + c] + acc);
                }
                p.z_cur[r * Ds + c] = zc;
                const float d = zc - zp;
                dist = dist + d * d;
                nrm = nrm + zp * zp;
            } else
                zc = p.z_cur[r * Ds + c];
            if (p.colscale) zc = zc * p.colscale[c];                    // frozen BatchNormalization behind the last layer: d h = d s_j
            zc = zc * act_grad(p.a[L - 1][r * Ds + c], p.acts[L - 1]);
        }
        db[0][lr * ADJ_NARROW_MAXW + c] = zc;
    }
    if (p.gather) {
        dist = row16_sum(dist); nrm = row16_sum(nrm);
        const int moved = open && live && sqrtf(dist) > p.thr * sqrtf(nrm);
        if (__any(moved) && (threadIdx.x & 63) == 0) gnn_flag_raise(p.gate);
    }
    int cur = 0;
    for (int l = L - 1; l >= 0; --l) {
        const int ni = p.dims[l], no = p.dims[l + 1];
        __syncthreads();                                            // d of this layer is complete, the weights of the layer above are spent
        for (int t = threadIdx.x; t < ni * no; t += 256) wt[t] = p.WT[l][t];
        __syncthreads();
        const float *d = db[cur] + lr * ADJ_NARROW_MAXW;
        if (l > 0) {
            for (int i = j; i < ni; i += 16) {
                float v = 0.0f;
                for (int k = 0; k < no; ++k) v = __builtin_fmaf(d[k], wt[k * ni + i], v);
                db[cur ^ 1][lr * ADJ_NARROW_MAXW + i] = live ? v * act_grad(p.a[l - 1][r * ni + i], p.acts[l - 1]) : 0.0f;
            }
        } else {
            for (int q = j; q < 2 * Ds; q += 16) {
                const int i = q < Ds ? q : p.c_aggs + (q - Ds);
                float v = 0.0f;
                for (int k = 0; k < no; ++k) v = __builtin_fmaf(d[k], wt[k * ni + i], v);
                if (live) p.u_out[r * 2 * Ds + q] = v;
            }
        }
        cur ^= 1;
    }
}

}   // namespace

namespace gnn_train {

int launch_adjoint_narrow(hipStream_t st, const AdjNarrow &p)
{
    if (p.n <= 0) return GNN_OK;
    if (p.L < 1 || p.L > 3 || p.dims[0] > ADJ_NARROW_MAXIN || p.c_aggs + p.Ds > p.dims[0] || p.dims[p.L] != p.Ds)
        return gnn_fail(GNN_ERR_STATE, "internal: the narrow adjoint launch does not cover this net");
    for (int l = 1; l <= p.L; ++l) if (p.dims[l] > ADJ_NARROW_MAXW) return gnn_fail(GNN_ERR_STATE, "internal: the narrow adjoint launch does not cover this net");
    hipLaunchKernelGGL(k_adjoint_narrow, cdiv(p.n, ADJ_NARROW_ROWS), 256, 0, st, p);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

int launch_adjoint_gather(hipStream_t st, const StateGradJob &job, const float *u, bool aligned, int *form)
{
    const bool rows = adjoint_rows16(job.Ds);
    if (form) *form = rows ? (aligned ? ADJ_GATHER_ROWS_ALIGNED : ADJ_GATHER_ROWS) : ADJ_GATHER_GENERIC;
    if (aligned && !rows) return gnn_fail(GNN_ERR_STATE, "internal: aligned state-gradient rows with state width %d", job.Ds);
    if (job.N <= 0) return GNN_OK;
    const AdjGather p{job.N, job.Ds, job.in_s, job.c_aggs, u, job.sip, job.sdst, job.sw, job.g, job.z_prev, job.z_next, job.work, job.thr, job.gate_prev, job.gate};
    const unsigned grid = cdiv(job.N * 16, 256);
    if (rows && aligned) hipLaunchKernelGGL(k_adjoint_gather_rows<true>, grid, 256, 0, st, p);
    else if (rows) hipLaunchKernelGGL(k_adjoint_gather_rows<false>, grid, 256, 0, st, p);
    else hipLaunchKernelGGL(k_adjoint_gather, grid, 256, 0, st, p);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

int launch_power_gather(hipStream_t st, const StateGradJob &job, const float *u, bool aligned, int *form)
{
    const bool rows = adjoint_rows16(job.Ds);
    if (form) *form = rows ? (aligned ? ADJ_GATHER_ROWS_ALIGNED : ADJ_GATHER_ROWS) : ADJ_GATHER_GENERIC;
    if (aligned && !rows) return gnn_fail(GNN_ERR_STATE, "internal: aligned state-gradient rows with state width %d", job.Ds);
    if (!job.pw_inv || !job.pw_part || !job.z_next || !job.work) return gnn_fail(GNN_ERR_STATE, "internal: a power gather without its buffers");
    if (job.N <= 0) return GNN_OK;
    const PowGather p{job.N, job.Ds, job.in_s, job.c_aggs, u, job.sip, job.sdst, job.sw, job.pw_inv, job.z_next, job.work, job.pw_part};
    const unsigned grid = power_blocks(job.N);
    if (rows && aligned) hipLaunchKernelGGL(k_power_gather_rows<true>, grid, 256, 0, st, p);
    else if (rows) hipLaunchKernelGGL(k_power_gather_rows<false>, grid, 256, 0, st, p);
    else hipLaunchKernelGGL(k_power_gather, grid, 256, 0, st, p);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

int launch_power_start(hipStream_t st, int64_t n, int Ds, int fill, uint64_t seed, float *v, float *work, float *part)
{
    if (n <= 0) return GNN_OK;
    hipLaunchKernelGGL(k_power_start, power_blocks(n), 256, 0, st, n, Ds, fill, seed, v, work, part);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

int launch_power_finalize(hipStream_t st, unsigned blocks, const float *part, float *norm_out, float *inv)
{
    hipLaunchKernelGGL(k_power_finalize, 1, 256, 0, st, blocks, part, norm_out, inv);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

}   // namespace gnn_train

extern "C" int gnn_adjoint_form_ex(int n_layers, const int *dims, const int *acts, const float *rates, int has_bn, int flags, int64_t n_rows, int *out)
{
    ARGCHK((flags & ~(GNN_ADJOINT_FROZEN_BN | GNN_ADJOINT_LABEL_GRADIENTS)) == 0, "flags: GNN_ADJOINT_FROZEN_BN, GNN_ADJOINT_LABEL_GRADIENTS, both or 0");
    ARGCHK(n_layers >= 1 && n_layers <= 16 && dims && acts && rates && n_rows >= 0 && out, "bad arguments");
    gnn_mlp m;
    m.n_layers = n_layers;
    m.dims.assign(dims, dims + n_layers + 1);
    m.acts.assign(acts, acts + n_layers);
    m.has_bn = has_bn != 0;
    for (int l = 0; l <= n_layers; ++l) ARGCHK(m.dims[l] >= 1, "bad layer width");
    for (int l = 0; l < n_layers; ++l) ARGCHK(m.acts[l] >= GNN_ACT_LINEAR && m.acts[l] <= GNN_ACT_SOFTMAX, "bad activation code");
    Net net;
    net.m = &m;
    net.rate.assign(rates, rates + n_layers + 1);
    net_decide_form(net, n_rows, true);
    const int Ds = m.dims[n_layers];
    out[1] = adjoint_refusal(&m, rates, flags);
    out[0] = out[1] == 0;
    // (the chain leaves its aligned rows where state_rows16 holds: with its many rows, wherever the state rows are 16-byte pieces)
    out[2] = adjoint_rows16(Ds) ? (net.bwd3 && n_rows > 0 ? ADJ_GATHER_ROWS_ALIGNED : ADJ_GATHER_ROWS) : ADJ_GATHER_GENERIC;
    for (int l = 0; l < n_layers; ++l) out[3 + l] = n_rows <= 0 ? GNN_FORM_PER_OP : net.bwd3 ? GNN_FORM_CHAIN3 : net.wide_bwd[l] ? GNN_FORM_WIDE : GNN_FORM_PER_OP;
    // the one-launch iteration of narrow nets replaces both where it applies
    out[3 + n_layers] = adjoint_narrow_why(&m, n_rows);
    if (out[3 + n_layers] == 0) {
        out[2] = ADJ_GATHER_NARROW;
        for (int l = 0; l < n_layers; ++l) out[3 + l] = GNN_FORM_ADJ_NARROW;
    }
    return GNN_OK;
}

extern "C" int gnn_adjoint_form(int n_layers, const int *dims, const int *acts, const float *rates, int has_bn, int64_t n_rows, int *out)
{
    return gnn_adjoint_form_ex(n_layers, dims, acts, rates, has_bn, 0, n_rows, out);
}

extern "C" int gnn_loop_set_gradient_mode_ex(gnn_loop *l, int mode, int adjoint_max_iter, float adjoint_threshold, int flags, int *used)
{
    ARGCHK(l, "loop is NULL");
    ARGCHK((flags & ~(GNN_ADJOINT_FROZEN_BN | GNN_ADJOINT_LABEL_GRADIENTS)) == 0, "flags: GNN_ADJOINT_FROZEN_BN, GNN_ADJOINT_LABEL_GRADIENTS, both or 0");
    ARGCHK(mode >= 0 && mode <= 2, "gradient mode: 0 unrolled, 1 fixed point, 2 fixed point without the one-launch iteration of narrow nets");
    ARGCHK(adjoint_max_iter >= 0 && !std::isnan(adjoint_threshold), "adjoint_max_iter must be >= 0 (0: the loop's max_iter), adjoint_threshold a number (< 0: the loop's threshold)");
    if (mode && l->world > 1) return gnn_fail(GNN_ERR_UNSUPPORTED, "the fixed-point gradient is single-GPU (this loop is rank %d of %d)", l->rank, l->world);
    if (mode && l->st->has_bn && !(flags & GNN_ADJOINT_FROZEN_BN))
        return gnn_fail(GNN_ERR_UNSUPPORTED, "the fixed-point gradient needs a net_state without BatchNormalization (its training-mode forward must be the inference forward)");
    l->train.adjoint.mode = mode;
    l->train.adjoint.flags = mode ? flags : 0;
    l->train.adjoint.max_iter = adjoint_max_iter;
    l->train.adjoint.thr = adjoint_threshold;
    if (used) *used = mode;
    return GNN_OK;
}

extern "C" int gnn_loop_set_gradient_mode(gnn_loop *l, int mode, int adjoint_max_iter, float adjoint_threshold, int *used)
{
    return gnn_loop_set_gradient_mode_ex(l, mode, adjoint_max_iter, adjoint_threshold, 0, used);
}

extern "C" int gnn_loop_adjoint_info(const gnn_loop *l, int *iterations, int *converged, int *form)
{
    ARGCHK(l, "loop is NULL");
    if (iterations) *iterations = l->train.adjoint.iterations;
    if (converged) *converged = l->train.adjoint.converged;
    if (form) *form = l->train.adjoint.gather;
    return GNN_OK;
}

// z_final of the last backward pass of modes 1 / 2 (the z buffer its last iteration wrote; the step's scratch lives until the next forward)
extern "C" int gnn_loop_adjoint_z(gnn_loop *l, float *z_host)
{
    ARGCHK(l && z_host, "bad arguments");
    const gnn_train_ctx *cx = l->train_ctx;
    if (!cx || !cx->fixed_point || !cx->backward_done || !cx->adjoint_z) return gnn_fail(GNN_ERR_STATE, "no backward pass of a fixed-point gradient mode to take z from");
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipStreamSynchronize(l->stream));
    if (cx->N > 0) HIPCHK(hipMemcpy(z_host, cx->adjoint_z, sizeof(float) * (size_t)cx->N * l->Ds, hipMemcpyDeviceToHost));
    return GNN_OK;
}

// w_done of the last contraction estimate (gnn_train.hip: it lives in the step's scratch until the next training forward or estimate)
extern "C" int gnn_loop_contraction_vector(gnn_loop *l, float *w_host)
{
    ARGCHK(l && w_host, "bad arguments");
    if (!l->train.power.w) return gnn_fail(GNN_ERR_STATE, "no contraction estimate of this loop to take the vector from (a training forward since ends its life)");
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipStreamSynchronize(l->stream));
    if (l->train.power.rows > 0) HIPCHK(hipMemcpy(w_host, l->train.power.w, sizeof(float) * (size_t)l->train.power.rows * l->Ds, hipMemcpyDeviceToHost));
    return GNN_OK;
}

extern "C" int gnn_loop_train_arena_bytes(const gnn_loop *l, int64_t *bytes)
{
    ARGCHK(l && bytes, "bad arguments");
    *bytes = l->train_arena ? (int64_t)l->train_arena->peak : 0;
    return GNN_OK;
}
