// Anderson-accelerated adjoint solve (include/gnn_hip.h: gnn_loop_set_adjoint_solver): the backward pass of gradient modes 1 / 2 solves
// (I - J^T) z = g; with solver 1 the iterates of z <- g + J^T z are mixed over a window of m difference pairs.  Iteration t:
//   G_t = g + J^T z_t (net_backward with wgrad = false, then the gather below with the arithmetic of gnn_train_adjoint.hip), f_t = G_t - z_t,
//   gate t = the Picard gate of z_next = G_t; closed: z_final = G_t.
//   t >= 1: slot s = hist mod m receives dF_s = f_t - f_{t-1}, dG_s = G_t - G_{t-1} (hist = pairs stored since the last restart, live = min(hist + 1, m));
//   H_ij = dF_i . dF_j (row / column s new), b_i = dF_i . f_t in double; (H + lambda I) gamma = b, lambda = 2^-40 trace(H) / live, by Cholesky;
//   z_{t+1} = G_t - sum_i gamma_i dG_i.  A pivot that is not > 0 or a value that is not finite restarts the window (gamma = 0, hist = 0).
// Three kernels per iteration behind net_backward: the gather (G_t, f_t, the slot, the gate, the block's partial dots), k_anderson_solve (one
// block) and k_anderson_mix.  Order of every sum: per lane over its ascending columns, the 16 lanes of a row by a fixed butterfly, the 16 rows of a
// block in row order through LDS, the blocks in block order in 256 runs (k_power_finalize's scheme).  No float atomics.
#include <cmath>

#include "gnn_train.h"

using namespace gnn_train;

namespace {

struct AndGather {
    int64_t n;
    int Ds, in_s, c_aggs;
    const float *u;               // as AdjGather::u of gnn_train_adjoint.hip
    const int32_t *sip, *sdst;
    const float *sw;
    const float *g, *z_prev;
    float *z_next, *work;
    float thr;
    const int *gate_prev;
    int *gate;
    int first, m;                 // first: iteration 0 (no history: z_next = work = G_0, no partials)
    float *G, *f, *dF, *dG;       // G_{t-1} / f_{t-1} in, G_t / f_t out (in place); the rings, slot j at + j * stride
    size_t stride;
    const AndersonState *state;
    double *part;                 // [ANDERSON_PARTS][blocks]
};

__device__ __forceinline__ float row16_sum(float v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 16);
    return v;
}

__device__ __forceinline__ double row16_sum(double v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 16);
    return v;
}

// One element behind its G: f, the two difference rows into slot s, its terms of H[s][.] and b[.] (ascending columns per lane), G and f in place.
__device__ __forceinline__ void anderson_element(const AndGather &p, int64_t i, float G, float zp, int s, int live, double *ph, double *pb,
                                                 float &dist, float &nrm)
{
    const float f = G - zp;
    if (!p.first) {
        const float dFs = f - p.f[i], dGs = G - p.G[i];
        p.dF[(size_t)s * p.stride + i] = dFs;
        p.dG[(size_t)s * p.stride + i] = dGs;
#pragma unroll
        for (int j = 0; j < ANDERSON_MAX_WINDOW; ++j)
            if (j < live) {
                const float dj = j == s ? dFs : p.dF[(size_t)j * p.stride + i];
                ph[j] = ph[j] + (double)dFs * (double)dj;
                pb[j] = pb[j] + (double)dj * (double)f;
            }
    } else {
        p.z_next[i] = G;
        p.work[i] = G;
    }
    p.G[i] = G;
    p.f[i] = f;
    dist = dist + f * f;
    nrm = nrm + zp * zp;
}

// the same for four neighbouring columns of a row of 16-byte pieces: every array is read and written in 16-byte pieces
__device__ __forceinline__ void anderson_element4(const AndGather &p, int64_t i, const float4 G4, const float4 zp4, int s, int live, double *ph,
                                                  double *pb, float &dist, float &nrm)
{
    const float G[4] = {G4.x, G4.y, G4.z, G4.w}, zp[4] = {zp4.x, zp4.y, zp4.z, zp4.w};
    float f[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) f[v] = G[v] - zp[v];
    if (!p.first) {
        const float4 fp = *reinterpret_cast<const float4 *>(p.f + i), Gp = *reinterpret_cast<const float4 *>(p.G + i);
        const float dFs[4] = {f[0] - fp.x, f[1] - fp.y, f[2] - fp.z, f[3] - fp.w};
        *reinterpret_cast<float4 *>(p.dF + (size_t)s * p.stride + i) = float4{dFs[0], dFs[1], dFs[2], dFs[3]};
        *reinterpret_cast<float4 *>(p.dG + (size_t)s * p.stride + i) = float4{G[0] - Gp.x, G[1] - Gp.y, G[2] - Gp.z, G[3] - Gp.w};
#pragma unroll
        for (int j = 0; j < ANDERSON_MAX_WINDOW; ++j)
            if (j < live) {
                float dj[4] = {dFs[0], dFs[1], dFs[2], dFs[3]};
                if (j != s) {
                    const float4 d4 = *reinterpret_cast<const float4 *>(p.dF + (size_t)j * p.stride + i);
                    dj[0] = d4.x; dj[1] = d4.y; dj[2] = d4.z; dj[3] = d4.w;
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    ph[j] = ph[j] + (double)dFs[v] * (double)dj[v];
                    pb[j] = pb[j] + (double)dj[v] * (double)f[v];
                }
            }
    } else {
        *reinterpret_cast<float4 *>(p.z_next + i) = G4;
        *reinterpret_cast<float4 *>(p.work + i) = G4;
    }
    *reinterpret_cast<float4 *>(p.G + i) = G4;
    *reinterpret_cast<float4 *>(p.f + i) = float4{f[0], f[1], f[2], f[3]};
#pragma unroll
    for (int v = 0; v < 4; ++v) { dist = dist + f[v] * f[v]; nrm = nrm + zp[v] * zp[v]; }
}

// The block's partial dots: the 16 lanes of a row by the butterfly, then the block's 16 rows in row order; part[q][block], q < live: H[s][q],
// ANDERSON_MAX_WINDOW + q: b[q].  Every thread of the block calls it.
__device__ __forceinline__ void anderson_block_sum(double *ph, double *pb, int live, double *part)
{
    __shared__ double rows[16][ANDERSON_PARTS];
#pragma unroll
    for (int j = 0; j < ANDERSON_MAX_WINDOW; ++j) {
        double h = 0.0, b = 0.0;
        if (j < live) { h = row16_sum(ph[j]); b = row16_sum(pb[j]); }          // (live is the same in every thread)
        if ((threadIdx.x & 15) == 0) {
            rows[threadIdx.x >> 4][j] = h;
            rows[threadIdx.x >> 4][ANDERSON_MAX_WINDOW + j] = b;
        }
    }
    __syncthreads();
    if (threadIdx.x < ANDERSON_PARTS) {
        double s = rows[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < 16; ++q) s = s + rows[q][threadIdx.x];
        part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
    }
}

// the shapes of k_adjoint_gather_rows<ALIGNED> (gnn_train_adjoint.hip), the same chain per element
template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_anderson_gather_rows(const AndGather p)
{
    const bool open = gnn_gate_open_block(p.gate_prev, 1);          // (every thread: it holds barriers)
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 4;
    const int cc = 4 * (int)(t & 15), Ds = p.Ds;
    const int hist = p.first ? 0 : p.state->hist, s = hist % p.m, live = p.first ? 0 : (hist + 1 < p.m ? hist + 1 : p.m);
    float dist = 0.0f, nrm = 0.0f;
    double ph[ANDERSON_MAX_WINDOW], pb[ANDERSON_MAX_WINDOW];
#pragma unroll
    for (int j = 0; j < ANDERSON_MAX_WINDOW; ++j) ph[j] = pb[j] = 0.0;
    if (r < p.n && cc < Ds) {
        const float4 zp = *reinterpret_cast<const float4 *>(p.z_prev + r * Ds + cc);
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
            const float4 G = float4{g4.x + (own.x + acc[0]), g4.y + (own.y + acc[1]), g4.z + (own.z + acc[2]), g4.w + (own.w + acc[3])};
            anderson_element4(p, r * Ds + cc, G, zp, s, live, ph, pb, dist, nrm);
        } else {                                                    // behind a closed gate: z is handed on, nothing else changes
            *reinterpret_cast<float4 *>(p.z_next + r * Ds + cc) = zp;
            *reinterpret_cast<float4 *>(p.work + r * Ds + cc) = zp;
        }
    }
    dist = row16_sum(dist); nrm = row16_sum(nrm);
    const int moved = open && r < p.n && sqrtf(dist) > p.thr * sqrtf(nrm);
    if (__any(moved) && (threadIdx.x & 63) == 0) gnn_flag_raise(p.gate);
    if (open && !p.first) anderson_block_sum(ph, pb, live, p.part);            // (the same branch in every thread of the block)
}

// the shape of k_adjoint_gather: any state width, lane j takes the columns j, j + 16, ...
__global__ void __launch_bounds__(256) k_anderson_gather(const AndGather p)
{
    const bool open = gnn_gate_open_block(p.gate_prev, 1);
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 4;
    const int j = (int)(t & 15), Ds = p.Ds;
    const int hist = p.first ? 0 : p.state->hist, s = hist % p.m, live = p.first ? 0 : (hist + 1 < p.m ? hist + 1 : p.m);
    float dist = 0.0f, nrm = 0.0f;
    double ph[ANDERSON_MAX_WINDOW], pb[ANDERSON_MAX_WINDOW];
#pragma unroll
    for (int q = 0; q < ANDERSON_MAX_WINDOW; ++q) ph[q] = pb[q] = 0.0;
    if (r < p.n) {
        const int32_t e0 = p.sip[r], e1 = p.sip[r + 1];
        for (int c = j; c < Ds; c += 16) {
            const float zp = p.z_prev[r * Ds + c];
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
                const float G = p.g[r * Ds + c] + (p.u[r * p.in_s + c] + acc);
                anderson_element(p, r * Ds + c, G, zp, s, live, ph, pb, dist, nrm);
            } else {
                p.z_next[r * Ds + c] = zp;
                p.work[r * Ds + c] = zp;
            }
        }
    }
    dist = row16_sum(dist); nrm = row16_sum(nrm);
    const int moved = open && r < p.n && sqrtf(dist) > p.thr * sqrtf(nrm);
    if (__any(moved) && (threadIdx.x & 63) == 0) gnn_flag_raise(p.gate);
    if (open && !p.first) anderson_block_sum(ph, pb, live, p.part);
}

// One block, behind the gather of iteration t >= 1.  Nothing happens behind a closed gate (gate_prev: the iteration before converged; gate: this one
// did, z_final = G_t).  Else: the blocks' partials in block order in 256 runs (thread i: blocks [i c, (i + 1) c), c = ceil(blocks / 256); thread q of
// the first 16 adds the 256 sums of quantity q in thread order), row and column s of H, b, and in thread 0 the regularised Cholesky solve.
__global__ void __launch_bounds__(256) k_anderson_solve(unsigned blocks, const double *part, int m, AndersonState *st, const int *gate_prev, const int *gate)
{
    __shared__ double sums[ANDERSON_PARTS][256];
    __shared__ double tot[ANDERSON_PARTS];
    if (!gnn_gate_open(gate_prev, 1) || !gnn_gate_open(gate, 1)) return;        // (the same words in every thread)
    const int hist = st->hist, s = hist % m, live = hist + 1 < m ? hist + 1 : m;
    const unsigned c = (blocks + 255) / 256, b0 = threadIdx.x * c, b1 = b0 + c < blocks ? b0 + c : blocks;
    for (int q = 0; q < ANDERSON_PARTS; ++q) {
        double v = 0.0;
        if ((q & (ANDERSON_MAX_WINDOW - 1)) < live)
            for (unsigned b = b0; b < b1; ++b) v = v + part[(size_t)q * blocks + b];
        sums[q][threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x < ANDERSON_PARTS) {
        double v = sums[threadIdx.x][0];
        for (int q = 1; q < 256; ++q) v = v + sums[threadIdx.x][q];
        tot[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int j = 0; j < live; ++j) st->H[s][j] = st->H[j][s] = tot[j];
    double L[ANDERSON_MAX_WINDOW][ANDERSON_MAX_WINDOW], y[ANDERSON_MAX_WINDOW], gam[ANDERSON_MAX_WINDOW];
    double tr = 0.0;
    for (int j = 0; j < live; ++j) tr = tr + st->H[j][j];
    const double lambda = tr * 9.094947017729282e-13 / (double)live;           // 2^-40 trace(H) / live
    bool ok = std::isfinite(lambda);
    for (int i = 0; ok && i < live; ++i)
        for (int j = 0; ok && j <= i; ++j) {
            double v = st->H[i][j] + (i == j ? lambda : 0.0);
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            if (i == j) {
                if (!(v > 0.0) || !std::isfinite(v)) ok = false;
                else L[i][i] = sqrt(v);
            } else
                L[i][j] = v / L[j][j];
        }
    for (int i = 0; ok && i < live; ++i) {
        double v = tot[ANDERSON_MAX_WINDOW + i];
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = live - 1; ok && i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < live; ++k) v = v - L[k][i] * gam[k];
        gam[i] = v / L[i][i];
    }
    for (int i = 0; ok && i < live; ++i) if (!std::isfinite(gam[i]) || !std::isfinite((float)gam[i])) ok = false;
    for (int i = 0; i < ANDERSON_MAX_WINDOW; ++i) st->gamma[i] = ok && i < live ? (float)gam[i] : 0.0f;
    st->live = ok ? live : 0;
    st->hist = ok ? hist + 1 : 0;
    if (!ok) st->restarts = st->restarts + 1;
}

struct AndMix {
    int64_t total;                // n Ds floats (VEC: a multiple of 4)
    int m;
    size_t stride;
    const float *G, *dG;
    const AndersonState *state;
    float *z_next, *work;
    const int *gate_prev, *gate;
};

// z_{t+1} = G_t - (the fmaf chain of gamma_i dG_i over ascending slots) into the z buffer and `work`; behind this iteration's closed gate G_t itself
// (z_final, which the weight-gradient pass finds in `work`); behind a closed gate_prev nothing.  VEC: 16-byte pieces.
template <bool VEC>
__global__ void __launch_bounds__(256) k_anderson_mix(const AndMix p)
{
    __shared__ int any[2];
    if (threadIdx.x < 2) any[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x < 2 * GNN_FLAG_SLOTS) {
        const int *gw = threadIdx.x < GNN_FLAG_SLOTS ? p.gate_prev : p.gate;
        if (!gw || gw[(threadIdx.x & (GNN_FLAG_SLOTS - 1)) * GNN_FLAG_STRIDE]) any[threadIdx.x >= GNN_FLAG_SLOTS] = 1;
    }
    __syncthreads();
    if (!any[0]) return;
    const int live = any[1] ? p.state->live : 0;
    float gam[ANDERSON_MAX_WINDOW];
#pragma unroll
    for (int j = 0; j < ANDERSON_MAX_WINDOW; ++j) gam[j] = j < live ? p.state->gamma[j] : 0.0f;
    const int64_t step = (int64_t)gridDim.x * blockDim.x * (VEC ? 4 : 1);
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * (VEC ? 4 : 1); i < p.total; i += step) {
        if (VEC) {
            const float4 G = *reinterpret_cast<const float4 *>(p.G + i);
            float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < ANDERSON_MAX_WINDOW; ++j)
                if (j < live) {
                    const float4 d = *reinterpret_cast<const float4 *>(p.dG + (size_t)j * p.stride + i);
                    a[0] = __builtin_fmaf(gam[j], d.x, a[0]); a[1] = __builtin_fmaf(gam[j], d.y, a[1]);
                    a[2] = __builtin_fmaf(gam[j], d.z, a[2]); a[3] = __builtin_fmaf(gam[j], d.w, a[3]);
                }
            const float4 z = float4{G.x - a[0], G.y - a[1], G.z - a[2], G.w - a[3]};
            *reinterpret_cast<float4 *>(p.z_next + i) = z;
            *reinterpret_cast<float4 *>(p.work + i) = z;
        } else {
            float a = 0.0f;
#pragma unroll
            for (int j = 0; j < ANDERSON_MAX_WINDOW; ++j) if (j < live) a = __builtin_fmaf(gam[j], p.dG[(size_t)j * p.stride + i], a);
            const float z = p.G[i] - a;
            p.z_next[i] = z;
            p.work[i] = z;
        }
    }
}

}   // namespace

namespace gnn_train {

int launch_anderson_gather(hipStream_t st, const StateGradJob &job, const float *u, bool aligned, int *form)
{
    const AndersonJob *a = job.anderson;
    const bool rows = adjoint_rows16(job.Ds);
    if (form) *form = rows ? (aligned ? ADJ_GATHER_ROWS_ALIGNED : ADJ_GATHER_ROWS) : ADJ_GATHER_GENERIC;
    if (aligned && !rows) return gnn_fail(GNN_ERR_STATE, "internal: aligned state-gradient rows with state width %d", job.Ds);
    if (!a || a->window < 1 || a->window > ANDERSON_MAX_WINDOW || !a->G || !a->f || !a->dF || !a->dG || !a->state || !a->part || !job.g || !job.z_prev ||
        !job.z_next || !job.work || !job.gate)
        return gnn_fail(GNN_ERR_STATE, "internal: an Anderson gather without its buffers");
    if (job.N <= 0) return GNN_OK;
    const AndGather p{job.N, job.Ds, job.in_s, job.c_aggs, u, job.sip, job.sdst, job.sw, job.g, job.z_prev, job.z_next, job.work, job.thr, job.gate_prev, job.gate,
                      a->first, a->window, a->G, a->f, a->dF, a->dG, a->stride, a->state, a->part};
    const unsigned grid = anderson_blocks(job.N);
    if (rows && aligned) hipLaunchKernelGGL(k_anderson_gather_rows<true>, grid, 256, 0, st, p);
    else if (rows) hipLaunchKernelGGL(k_anderson_gather_rows<false>, grid, 256, 0, st, p);
    else hipLaunchKernelGGL(k_anderson_gather, grid, 256, 0, st, p);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

int launch_anderson_solve_mix(hipStream_t st, const StateGradJob &job)
{
    const AndersonJob *a = job.anderson;
    if (!a || a->first || !a->state || !a->part || !a->G || !a->dG || !job.z_next || !job.work || !job.gate)
        return gnn_fail(GNN_ERR_STATE, "internal: an Anderson mix without its buffers");
    if (job.N <= 0) return GNN_OK;
    hipLaunchKernelGGL(k_anderson_solve, 1, 256, 0, st, anderson_blocks(job.N), a->part, a->window, a->state, job.gate_prev, job.gate);
    const int64_t total = job.N * job.Ds;
    const AndMix p{total, a->window, a->stride, a->G, a->dG, a->state, job.z_next, job.work, job.gate_prev, job.gate};
    if ((job.Ds & 3) == 0) hipLaunchKernelGGL(k_anderson_mix<true>, elementwise_grid(total / 4), 256, 0, st, p);
    else hipLaunchKernelGGL(k_anderson_mix<false>, elementwise_grid(total), 256, 0, st, p);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

}   // namespace gnn_train

extern "C" int gnn_loop_set_adjoint_solver(gnn_loop *l, int solver, int window, int *used)
{
    ARGCHK(l, "loop is NULL");
    ARGCHK(solver == 0 || solver == 1, "adjoint solver: 0 Picard (z <- g + J^T z), 1 Anderson mixing");
    ARGCHK(window >= 1 && window <= gnn_train::ANDERSON_MAX_WINDOW, "window must lie in [1, 8] (got %d)", window);
    if (solver && l->world > 1) return gnn_fail(GNN_ERR_UNSUPPORTED, "the fixed-point gradient is single-GPU (this loop is rank %d of %d)", l->rank, l->world);
    l->train.adjoint.solver = solver;
    l->train.adjoint.window = window;
    if (used) *used = solver;
    return GNN_OK;
}

extern "C" int gnn_loop_adjoint_solver_info(const gnn_loop *l, int *solver, int *window, int *restarts)
{
    ARGCHK(l, "loop is NULL");
    if (solver) *solver = l->train.adjoint.solver;
    if (window) *window = l->train.adjoint.window;
    if (restarts) *restarts = l->train.adjoint.restarts;
    return GNN_OK;
}
