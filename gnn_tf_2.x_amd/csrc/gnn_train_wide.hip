// The matrix-core products of the training step and their launchers (see gnn_train.hip for the step, gnn_train.h for what crosses the units).
// The only training unit that sees the fused inference kernels' device code.
#include <stdlib.h>

#include "gnn_train.h"
#include "gnn_fused_kernel.h"     // layer_from_lds / f32x16: the f32-MFMA K-step pipeline of the exact fused path, reused by the wide dense products

using namespace gnn_train;

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Wide layers (round 3): the three dense products of a Dense layer on the matrix cores (v_mfma_f32_32x32x2_f32: f32 in, f32
// accumulate, every product exact, the k-ordered fmaf chain of the per-op kernels - so results do not depend on the grid).
//   forward      a      = act(h . W + b)                        k_gemm_f32, weights as the A operand, 32 rows of h per wave as B
//   backward     d h_in = d z . W^T (x Dropout / act' epilogue)   k_gemm_f32 on W^T
//                [dW; db] = [h | 1]^T . d z                      k_wgrad_f32: rows are the K dimension; per-chunk partials, added in
//                                                               chunk order afterwards like every other reduction of the step
// BASELINE configs[2] shape (1 M rows, 135 -> 128 -> 128 -> 64): k_dense_fwd 1.08 ms and k_layer_bwd 2.02 ms per layer on the FP32
// ALUs before (profiles/r03_train_c3.txt).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int TG_WAVES = 8;
constexpr int TG_MAX_GRID = 256;                       // blocks of the persistent kernels (k_gemm_*, k_fwd3_split, k_bwd3_split): a wave takes tile after tile beyond that
constexpr int64_t GNN_TRAIN_MFMA_MIN_ROWS = 4096;      // below that a step is launch-bound (MUTAG batches: 570 rows) and the per-op kernels are as fast

// packed A operand of layer_from_lds for output columns [col0, col0 + 32 NO) of M [K, n_cols]: wp[(kk 64 + lane) NO + j] =
// M[2 kk + (lane >> 5)][col0 + 32 j + (lane & 31)], zero outside the matrix (K-steps up to kk_total: the pipeline's look-ahead)
__global__ void k_pack_exact(int K, int n_cols, int col0, int NO, int kk_total, const float *__restrict__ M, float *__restrict__ wp)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= kk_total * 64 * NO) return;
    const int j = t % NO, lane = (t / NO) & 63, kk = t / (64 * NO);
    const int k = 2 * kk + (lane >> 5), c = col0 + 32 * j + (lane & 31);
    wp[t] = (k < K && c < n_cols) ? M[(size_t)k * n_cols + c] : 0.0f;
}

struct GemmArgs {
    int64_t n;
    int K, KP, kk, n_cols, col0, act, mode, spread;       // mode 0: forward (bias + activation); 1: backward (Dropout / act' of the producer)
    float rate;
    const float *X, *wp, *bias, *a_prev;
    const uint8_t *keep;
    float *Y;
};

// Y[r, col0 .. col0 + 32 NO) = epilogue(X[r, :] . M[:, col0 ..]) for all rows; X dense [n, K], Y dense [n, n_cols].
// One wave = 32 rows: rows staged in LDS (odd row stride: conflict-free column reads), K-steps through layer_from_lds.  All pieces of a
// tile (up to 18 x 16 B per lane) are requested before the first is written to LDS: one round trip per tile, covered by the SIMD's other
// wave.  (Measured, profiles/r03_train_c3.txt: a staging loop with a load per iteration - 17 dependent round trips - 0.89 ms per
// 1 M x 135 x 128 product; the NEXT tile's rows held in registers across the K-steps: 256 VGPRs + 163 spilled, 1.06 ms.)
constexpr int TG_MAXQ = 18;                        // 16-byte pieces per lane of a 32 x 144 tile

template <int ACT, int NO>
__device__ __forceinline__ void gemm_store_fwd(const GemmArgs &p, f32x16 (&acc)[NO], int64_t row, int half, bool vec)
{
    using namespace gnn_fused_dev;
#pragma unroll
    for (int jt = 0; jt < NO; ++jt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f0 = p.col0 + 32 * jt + 8 * q + 4 * half;
            const int64_t o = row * p.n_cols + f0;
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = f0 + u < p.n_cols ? act_t<ACT>(acc[jt][4 * q + u] + p.bias[f0 + u]) : 0.0f;
            if (vec && f0 + 4 <= p.n_cols) *reinterpret_cast<GNN_GLOBAL v4f *>(gptr_w(p.Y) + o) = v4f{v[0], v[1], v[2], v[3]};
            else
                for (int u = 0; u < 4; ++u) if (f0 + u < p.n_cols) gptr_w(p.Y)[o + u] = v[u];
        }
}

template <int NO>
__global__ void __launch_bounds__(64 * TG_WAVES, 2) k_gemm_f32(const GemmArgs p)
{
    using namespace gnn_fused_dev;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = p.K, KP = p.KP;
    float *X = lds + (size_t)wave * 32 * KP;
    for (int t = lane; t < 32 * (KP - K); t += 64) X[(t / (KP - K)) * KP + K + t % (KP - K)] = 0.0f;      // columns >= K: zero, once
    const int64_t n_tiles = (p.n + 31) / 32;
    const float inv_k = 1.0f / (float)K;
    const int half = lane >> 5, node = lane & 31;
    const int64_t stride = (int64_t)gridDim.x * TG_WAVES;
    const bool vec = (p.n_cols & 3) == 0;
    v4f nxt[TG_MAXQ];
    auto request = [&](int64_t tile) {                                   // rows of `tile` -> registers (zeros past the matrix)
        const int64_t i0 = tile * 32;
        const int total = tile < n_tiles ? (int)((p.n - i0) < 32 ? (p.n - i0) : 32) * K : 0;
        const float *src = p.X + i0 * K;
#pragma unroll
        for (int q = 0; q < TG_MAXQ; ++q) {
            const int e = lane * 4 + 256 * q;
            nxt[q] = v4f{0.f, 0.f, 0.f, 0.f};
            if (e + 4 <= total) nxt[q] = gload4(src + e);
            else if (e < total) {                                        // tail of a partial last tile
                float t4[4] = {0.f, 0.f, 0.f, 0.f};
                for (int u = 0; u < 4; ++u) if (e + u < total) t4[u] = gload1(src + e + u);
                nxt[q] = v4f{t4[0], t4[1], t4[2], t4[3]};
            }
        }
    };
    for (int64_t tile = (int64_t)blockIdx.x * TG_WAVES + wave; tile < n_tiles; tile += stride) {
        const int64_t i0 = tile * 32;
        const int nvalid = (int)((p.n - i0) < 32 ? (p.n - i0) : 32);
        request(tile);
        int lane_o = lane;                      // opaque per tile: the 72 (row, column) pairs below are loop-invariant and would otherwise be
        asm volatile("" : "+v"(lane_o));        // hoisted out of the tile loop and kept in registers across the K-steps (163 spills)
#pragma unroll
        for (int q = 0; q < TG_MAXQ; ++q) {
            const int e = lane_o * 4 + 256 * q;
            if (e < 32 * K) {
                const float v[4] = {nxt[q].x, nxt[q].y, nxt[q].z, nxt[q].w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int ee = e + u, r = (int)(((float)ee + 0.5f) * inv_k), c = ee - r * K;
                    X[r * KP + c] = v[u];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        f32x16 acc[NO];
        zero_acc<NO>(acc);
        layer_from_lds<NO>(X + node * KP + half, p.wp + (size_t)lane * NO, p.kk, acc, 1);
        int half_o = half;                      // (opaque per tile as well: the 64 bias values / output offsets of the epilogue are loop-invariant too)
        asm volatile("" : "+v"(half_o));
        if (node < nvalid) {
            const int64_t row = i0 + node;
            const int half = half_o;
            if (p.mode == 0) {
                switch (p.act) {
                case GNN_ACT_RELU: gemm_store_fwd<GNN_ACT_RELU, NO>(p, acc, row, half, vec); break;
                case GNN_ACT_SELU: gemm_store_fwd<GNN_ACT_SELU, NO>(p, acc, row, half, vec); break;
                case GNN_ACT_ELU: gemm_store_fwd<GNN_ACT_ELU, NO>(p, acc, row, half, vec); break;
                case GNN_ACT_TANH: gemm_store_fwd<GNN_ACT_TANH, NO>(p, acc, row, half, vec); break;
                case GNN_ACT_SIGMOID: gemm_store_fwd<GNN_ACT_SIGMOID, NO>(p, acc, row, half, vec); break;
                default: gemm_store_fwd<GNN_ACT_LINEAR, NO>(p, acc, row, half, vec); break;       // (softmax is applied by the caller)
                }
            } else {
#pragma unroll
                for (int jt = 0; jt < NO; ++jt)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int f0 = p.col0 + 32 * jt + 8 * q + 4 * half;
                        const int64_t o = row * p.n_cols + f0;
                        float v[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            float x = acc[jt][4 * q + u];
                            if (f0 + u < p.n_cols) {
                                if (p.keep) x = dropout_grad(x, p.keep[o + u], p.rate);
                                if (p.act >= 0) x = x * act_grad(p.a_prev[o + u], p.act);
                            }
                            v[u] = x;
                        }
                        if (vec && f0 + 4 <= p.n_cols) *reinterpret_cast<GNN_GLOBAL v4f *>(gptr_w(p.Y) + o) = v4f{v[0], v[1], v[2], v[3]};
                        else
                            for (int u = 0; u < 4; ++u) if (f0 + u < p.n_cols) gptr_w(p.Y)[o + u] = v[u];
                    }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // the next tile re-uses this wave's LDS region
    }
}

// The same product in the split arithmetic of the fused inference kernel (gnn_fused_kernel.h: every fp32 operand cut into three exact
// bf16 pieces, six piece products per term on v_mfma_f32_32x32x16_bf16, fp32 accumulation): 2.7 x fewer matrix-pipe cycles than the f32
// MFMA, and the bf16 MFMA overlaps the wave's VALU work.  Packed operand: [K = 16 chunk][out tile][piece][lane][8 bf16] + two zero chunks.
// hidden: the k order of a layer whose input is the previous layer's accumulators (gnn_fused_kernel.h: chunk c, element i of k half h is
// feature 32 (c >> 1) + (r & 3) + 8 (r >> 2) + 4 h, r = 8 (c & 1) + i); fold: factor on every weight (the folded SELU of the fused chain)
__global__ void k_pack_split(int K, int n_cols, int col0, int NO, int chunks_img, const float *__restrict__ M, uint32_t *__restrict__ out, int hidden = 0,
                             float fold = 1.0f)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;                 // one thread per (chunk, tile, lane, element pair): three dwords (pieces)
    if (t >= chunks_img * NO * 64 * 4) return;
    const int j2 = t & 3, lane = (t >> 2) & 63, jt = (t >> 8) % NO, c = (t >> 8) / NO;
    uint32_t d[3] = {0u, 0u, 0u};
    for (int e = 0; e < 2; ++e) {
        const int i = 2 * j2 + e, h = lane >> 5, r = 8 * (c & 1) + i, col = col0 + 32 * jt + (lane & 31);
        const int k = hidden ? 32 * (c >> 1) + (r & 3) + 8 * (r >> 2) + 4 * h : 16 * c + 8 * h + i;
        float v = (k < K && col < n_cols) ? M[(size_t)k * n_cols + col] * fold : 0.0f;
        for (int pc = 0; pc < 3; ++pc) {                                 // truncation split: v == p0 + p1 + p2 exactly
            const uint32_t hi = __float_as_uint(v) & 0xffff0000u;
            v = v - __uint_as_float(hi);
            d[pc] |= e ? hi : (hi >> 16);
        }
    }
    for (int pc = 0; pc < 3; ++pc) out[((((size_t)c * NO + jt) * 3 + pc) * 64 + lane) * 4 + j2] = d[pc];
}

template <int NO>
__global__ void __launch_bounds__(64 * TG_WAVES, 2) k_gemm_split(const GemmArgs p)
{
    using namespace gnn_fused_dev;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = p.K, KP = p.KP;                                        // KP: a multiple of 4 with KP / 4 odd (16-byte rows, conflict-free b128 column reads)
    float *X = lds + (size_t)wave * 32 * KP;
    float *bias_lds = lds + (size_t)TG_WAVES * 32 * KP + 32;             // [32 NO]: the accumulators start from it (zeros in backward mode)
    for (int t = threadIdx.x; t < 32 * NO; t += blockDim.x) bias_lds[t] = (p.mode == 0 && p.col0 + t < p.n_cols) ? p.bias[p.col0 + t] : 0.0f;
    for (int t = lane; t < 32 * (KP - K); t += 64) X[(t / (KP - K)) * KP + K + t % (KP - K)] = 0.0f;      // columns >= K: zero, once
    __syncthreads();
    const int64_t n_tiles = (p.n + 31) / 32;
    const float inv_k = 1.0f / (float)K;
    const int half = lane >> 5, node = lane & 31;
    const int64_t stride = (int64_t)gridDim.x * TG_WAVES;
    const bool vec = (p.n_cols & 3) == 0, kvec = (K & 3) == 0;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wp), 0, p.kk, 0x00020000);      // (kk: bytes of the packed image here)
    // start-up spread (as k_fused): all waves run the same phases - load, K-steps, store - on tiles of equal cost; started together they
    // would load together and compute together.  Every wave waits a different fraction of about one tile period first.
    if (n_tiles >= 4 * stride) {
        const int rounds = (int)((((unsigned)blockIdx.x * TG_WAVES + (unsigned)wave) * 0x9E3779B1u) >> 16) % (unsigned)(p.spread + 1);
        for (int i = 0; i < rounds; ++i) __builtin_amdgcn_s_sleep(127);
    }
    v4f nxt[TG_MAXQ];
    for (int64_t tile = (int64_t)blockIdx.x * TG_WAVES + wave; tile < n_tiles; tile += stride) {
        const int64_t i0 = tile * 32;
        const int nvalid = (int)((p.n - i0) < 32 ? (p.n - i0) : 32);
        const int total = nvalid * K;
        const float *src = p.X + i0 * K;
#pragma unroll
        for (int q = 0; q < TG_MAXQ; ++q) {                              // all pieces of the tile requested before the first is used
            const int e = lane * 4 + 256 * q;
            nxt[q] = v4f{0.f, 0.f, 0.f, 0.f};
            if (e + 4 <= total) nxt[q] = gload4(src + e);
            else if (e < total) {                                        // tail of a partial last tile
                float t4[4] = {0.f, 0.f, 0.f, 0.f};
                for (int u = 0; u < 4; ++u) if (e + u < total) t4[u] = gload1(src + e + u);
                nxt[q] = v4f{t4[0], t4[1], t4[2], t4[3]};
            }
        }
        int lane_o = lane;                      // opaque per tile (see k_gemm_f32)
        asm volatile("" : "+v"(lane_o));
        if (K < 32 * NO) {                      // the previous tile's output pass left values in columns [K, 32 NO): zero again (0 x Inf would poison the sums)
            const int zw = 32 * NO - K;
            for (int t = lane_o; t < 32 * zw; t += 64) X[(t / zw) * KP + K + t % zw] = 0.0f;
        }
#pragma unroll
        for (int q = 0; q < TG_MAXQ; ++q) {
            const int e = lane_o * 4 + 256 * q;
            if (e < 32 * K) {
                if (kvec) {                                              // rows are whole 16-byte pieces
                    const int r = (int)(((float)e + 0.5f) * inv_k), c = e - r * K;
                    *reinterpret_cast<v4f *>(X + r * KP + c) = nxt[q];
                } else {
                    const float v[4] = {nxt[q].x, nxt[q].y, nxt[q].z, nxt[q].w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int ee = e + u, r = (int)(((float)ee + 0.5f) * inv_k), c = ee - r * K;
                        X[r * KP + c] = v[u];
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        f32x16 acc[NO];
        layer0_split<NO, true>(X + node * KP + 8 * half, wrs, lane * 16, 0, (K + 15) / 16, acc, bias_lds, half);
        // Epilogue in two steps, so that every global access is a whole row piece: (1) the accumulators (feature on the register, row on
        // the lane) go to the wave's LDS tile as [row][column] (16-byte pieces, row stride KP: KP / 4 odd, conflict-free); (2) lanes take
        // consecutive 16-byte pieces of consecutive rows - 512 contiguous bytes per 32 lanes for a 128-wide pass - read the matching
        // pieces of the producer's activation / Dropout mask, apply bias-included activation or the derivative, and store.  (Stores of
        // 16-byte pieces straight from the accumulator layout touch 32 rows per instruction: 0.63 ms per product whatever K.)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // all B-operand reads of the tile are done: its LDS region is free
        int half_o = half;
        asm volatile("" : "+v"(half_o));
#pragma unroll
        for (int jt = 0; jt < NO; ++jt)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<v4f *>(X + node * KP + 32 * jt + 8 * q + 4 * half_o) = v4f{acc[jt][4 * q], acc[jt][4 * q + 1], acc[jt][4 * q + 2], acc[jt][4 * q + 3]};
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        constexpr int PPR = 8 * NO;                                      // 16-byte pieces per row of this pass
        int lane_p = lane;
        asm volatile("" : "+v"(lane_p));
#pragma unroll
        for (int u = 0; u < 32 * PPR / 64; ++u) {
            const int idx = lane_p + 64 * u, r = idx / PPR, c = (idx % PPR) * 4;
            const int f0 = p.col0 + c;
            if (r < nvalid && f0 < p.n_cols) {
                const v4f a4 = *reinterpret_cast<const v4f *>(X + r * KP + c);
                float v[4] = {a4.x, a4.y, a4.z, a4.w};
                const int64_t o = (i0 + r) * p.n_cols + f0;
                const bool full = vec && f0 + 4 <= p.n_cols;
                if (p.mode == 0) {
                    // hardware transcendentals (v_exp_f32 / v_rcp_f32, 1 ulp: act_fast of the fused inference path); the backward pass
                    // differentiates from the stored activation, so forward and backward stay consistent
                    switch (p.act) {
                    case GNN_ACT_RELU: for (int t = 0; t < 4; ++t) v[t] = act_fast<GNN_ACT_RELU>(v[t]); break;
                    case GNN_ACT_SELU: for (int t = 0; t < 4; ++t) v[t] = act_fast<GNN_ACT_SELU>(v[t]); break;
                    case GNN_ACT_ELU: for (int t = 0; t < 4; ++t) v[t] = act_fast<GNN_ACT_ELU>(v[t]); break;
                    case GNN_ACT_TANH: for (int t = 0; t < 4; ++t) v[t] = act_fast<GNN_ACT_TANH>(v[t]); break;
                    case GNN_ACT_SIGMOID: for (int t = 0; t < 4; ++t) v[t] = act_fast<GNN_ACT_SIGMOID>(v[t]); break;
                    default: break;
                    }
                } else {
                    if (p.keep)
                        for (int t = 0; t < 4; ++t) if (f0 + t < p.n_cols) v[t] = dropout_grad(v[t], p.keep[o + t], p.rate);
                    if (p.act >= 0) {
                        if (full) {
                            const v4f ap = gload4(p.a_prev + o);
                            v[0] *= act_grad(ap.x, p.act); v[1] *= act_grad(ap.y, p.act); v[2] *= act_grad(ap.z, p.act); v[3] *= act_grad(ap.w, p.act);
                        } else
                            for (int t = 0; t < 4; ++t) if (f0 + t < p.n_cols) v[t] *= act_grad(p.a_prev[o + t], p.act);
                    }
                }
                if (full) *reinterpret_cast<GNN_GLOBAL v4f *>(gptr_w(p.Y) + o) = v4f{v[0], v[1], v[2], v[3]};
                else
                    for (int t = 0; t < 4; ++t) if (f0 + t < p.n_cols) gptr_w(p.Y)[o + t] = v[t];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // the next tile re-uses this wave's LDS region
    }
}

// The three Dense layers of a 3-layer net_state in ONE pass over the rows (round 3): the chain of the fused inference kernel - layer 0 from
// the LDS tile, the hidden layers from the previous accumulators without leaving registers (layer_split_from_regs, folded SELU) - with
// the activations the backward pass differentiates written out on the way (a0, a1 after the layer that consumes them has cut them into
// pieces, a2 at the end), each through the wave's LDS tile as whole row pieces.  Saves re-reading a0 and a1 (2 x 512 MB at 1 M rows) and
// two stagings.  Shape: hidden width <= 128 (four 32-feature tiles), last width <= 64 (two).
struct Fwd3Args {
    int64_t n;
    int K, KP, chunks0, w1, w2, w3, act;
    int img_bytes, off1, off2;               // one packed image for the three layers: byte offsets of layers 1 and 2
    const float *X, *b0, *b1, *b2;
    const uint32_t *img;
    float *A0, *A1, *A2;
};

// KEEP = false (the state-only first pass of the recomputing step, gnn_loop_set_train_recompute): a0 and a1 are neither staged nor stored - the
// same products and epilogues, so a2 holds the same bits; p.A0 / p.A1 are not read.
template <int ACT, bool KEEP = true>
__global__ void __launch_bounds__(64 * TG_WAVES, 2) k_fwd3_split(const Fwd3Args p)
{
    using namespace gnn_fused_dev;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr bool FOLD = ACT == GNN_ACT_SELU;
    constexpr float LOG2E = 1.44269504088896341f, UNFOLD = FOLD ? 1.0507009873554805f / LOG2E : 1.0f;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = p.K, KP = p.KP;
    float *X = lds + (size_t)wave * 32 * KP;
    float *hb = lds + (size_t)TG_WAVES * 32 * KP + 32;                   // biases: layer 0 [128] | layer 1 [128] | layer 2 [64]
    for (int t = threadIdx.x; t < 320; t += blockDim.x) {
        float v = 0.0f;
        if (t < 128) v = t < p.w1 ? p.b0[t] * (FOLD ? LOG2E : 1.0f) : 0.0f;
        else if (t < 256) v = t - 128 < p.w2 ? p.b1[t - 128] * (FOLD ? LOG2E : 1.0f) : 0.0f;
        else v = t - 256 < p.w3 ? p.b2[t - 256] : 0.0f;
        hb[t] = v;
    }
    __syncthreads();
    const int64_t n_tiles = (p.n + 31) / 32, stride = (int64_t)gridDim.x * TG_WAVES;
    const float inv_k = 1.0f / (float)K;
    const int half = lane >> 5, node = lane & 31;
    const bool kvec = (K & 3) == 0;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(p.img), 0, p.img_bytes, 0x00020000);
    // rows of one activation array through the LDS tile: accumulator layout -> [row][column] -> whole row pieces to memory
    auto store_rows = [&](auto &h, auto NTc, float *dst, int width, int nvalid, int64_t i0, float scale, bool activate) {
        constexpr int NTT = decltype(NTc)::value;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        int half_o = half;
        asm volatile("" : "+v"(half_o));
#pragma unroll
        for (int jt = 0; jt < NTT; ++jt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v4f v = {h[jt][4 * q], h[jt][4 * q + 1], h[jt][4 * q + 2], h[jt][4 * q + 3]};
                if (activate) v = v4f{act_fast<ACT>(v.x), act_fast<ACT>(v.y), act_fast<ACT>(v.z), act_fast<ACT>(v.w)};
                *reinterpret_cast<v4f *>(X + node * KP + 32 * jt + 8 * q + 4 * half_o) = v * scale;
            }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        constexpr int PPR = 8 * NTT;
        const bool vec = (width & 3) == 0;
        int lane_p = lane;
        asm volatile("" : "+v"(lane_p));
#pragma unroll
        for (int u = 0; u < 32 * PPR / 64; ++u) {
            const int idx = lane_p + 64 * u, r = idx / PPR, c = (idx % PPR) * 4;
            if (r < nvalid && c < width) {
                const v4f a4 = *reinterpret_cast<const v4f *>(X + r * KP + c);
                const int64_t o = (i0 + r) * width + c;
                if (vec) *reinterpret_cast<GNN_GLOBAL v4f *>(gptr_w(dst) + o) = a4;
                else {
                    const float v[4] = {a4.x, a4.y, a4.z, a4.w};
                    for (int t = 0; t < 4; ++t) if (c + t < width) gptr_w(dst)[o + t] = v[t];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    };
    v4f nxt[TG_MAXQ];
    for (int64_t tile = (int64_t)blockIdx.x * TG_WAVES + wave; tile < n_tiles; tile += stride) {
        const int64_t i0 = tile * 32;
        const int nvalid = (int)((p.n - i0) < 32 ? (p.n - i0) : 32);
        const int total = nvalid * K;
        const float *src = p.X + i0 * K;
#pragma unroll
        for (int q = 0; q < TG_MAXQ; ++q) {
            const int e = lane * 4 + 256 * q;
            nxt[q] = v4f{0.f, 0.f, 0.f, 0.f};
            if (e + 4 <= total) nxt[q] = gload4(src + e);
            else if (e < total) {
                float t4[4] = {0.f, 0.f, 0.f, 0.f};
                for (int u = 0; u < 4; ++u) if (e + u < total) t4[u] = gload1(src + e + u);
                nxt[q] = v4f{t4[0], t4[1], t4[2], t4[3]};
            }
        }
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
        // (the stores of the previous tile left values in columns [K, KP) of the tile region: zero them again - 0 x Inf would poison the sums)
        for (int t = lane_o; t < 32 * (KP - K); t += 64) X[(t / (KP - K)) * KP + K + t % (KP - K)] = 0.0f;
#pragma unroll
        for (int q = 0; q < TG_MAXQ; ++q) {
            const int e = lane_o * 4 + 256 * q;
            if (e < 32 * K) {
                if (kvec) {
                    const int r = (int)(((float)e + 0.5f) * inv_k), c = e - r * K;
                    *reinterpret_cast<v4f *>(X + r * KP + c) = nxt[q];
                } else {
                    const float v[4] = {nxt[q].x, nxt[q].y, nxt[q].z, nxt[q].w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int ee = e + u, r = (int)(((float)ee + 0.5f) * inv_k), c = ee - r * K;
                        X[r * KP + c] = v[u];
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        f32x16 h1[4], h2[4], out[2];
        layer0_split<4, true>(X + node * KP + 8 * half, wrs, lane * 16, 0, p.chunks0, h1, hb, half);
        layer_split_from_regs<4, 4, ACT>(h1, hb + 128, half, h2, wrs, lane * 16, p.off1);       // h1 now holds the (folded) activations of layer 0
        if constexpr (KEEP) store_rows(h1, std::integral_constant<int, 4>{}, p.A0, p.w1, nvalid, i0, UNFOLD, false);
        layer_split_from_regs<4, 2, ACT>(h2, hb + 256, half, out, wrs, lane * 16, p.off2);
        if constexpr (KEEP) store_rows(h2, std::integral_constant<int, 4>{}, p.A1, p.w2, nvalid, i0, UNFOLD, false);
        store_rows(out, std::integral_constant<int, 2>{}, p.A2, p.w3, nvalid, i0, 1.0f, true);
    }
}

}   // namespace

namespace gnn_train {

// K-steps of the wide products: a multiple of 12 (layer_from_lds consumes groups of 3 x 4) plus its look-ahead of 8
inline int tg_kk(int K) { return ((K + 1) / 2 + 11) / 12 * 12; }
inline int tg_kp(int K) { return std::max(2 * tg_kk(K), (K + 15) / 16 * 16) + 1; }
bool tg_many_rows(int64_t n)
{
#ifdef GNN_DIAG      // GNN_TRAIN_MFMA=0: the round-2 kernels everywhere (accuracy / timing comparison)
    static const bool off = getenv("GNN_TRAIN_MFMA") && atoi(getenv("GNN_TRAIN_MFMA")) == 0;
    if (off) return false;
#endif
    return n >= GNN_TRAIN_MFMA_MIN_ROWS;
}
bool tg_wide(int n_in, int n_out) { return n_in >= 64 && n_out >= 32 && n_in <= 144; }      // (TG_MAXQ pieces of a 32-row tile per lane)

// Y = epilogue(X . M) over all column passes of M [K, n_cols]; scratch for the packed operand comes from the step's arena
inline int tg_kps(int K) { int kp = ((K + 15) / 16 * 16 + 3) / 4 * 4; if ((kp / 4) % 2 == 0) kp += 4; return kp; }

int launch_gemm_f32(hipStream_t st, Buf &buf, int64_t n, int K, int n_cols, const float *X, const float *M, const float *bias, int act, int mode,
                    const uint8_t *keep, float rate, const float *a_prev, float *Y)
{
    static bool lds_raised[64] = {false};
    const void *ks[6] = {reinterpret_cast<const void *>(&k_gemm_f32<4>), reinterpret_cast<const void *>(&k_gemm_f32<2>), reinterpret_cast<const void *>(&k_gemm_f32<1>),
                         reinterpret_cast<const void *>(&k_gemm_split<4>), reinterpret_cast<const void *>(&k_gemm_split<2>), reinterpret_cast<const void *>(&k_gemm_split<1>)};
    (void)gnn_raise_dynamic_lds(ks, 6, 160 * 1024, lds_raised);
    bool split = true;                             // shipped: the split-bf16 products; the f32-MFMA form stays as the exact-chain cross-check
#ifdef GNN_DIAG
    static const bool f32_env = getenv("GNN_TRAIN_GEMM_F32") != nullptr;
    split = !f32_env;
#endif
    GemmArgs p{};
    p.n = n; p.K = K; p.n_cols = n_cols; p.act = act; p.mode = mode; p.rate = rate;
    p.X = X; p.bias = bias; p.a_prev = a_prev; p.keep = keep; p.Y = Y;
    p.spread = 0;                                  // (measured: 0 .. 8 rounds of start-up spread change nothing here, profiles/r03_train_c3.txt)
#ifdef GNN_DIAG
    static const int spread_env = getenv("GNN_TRAIN_SPREAD") ? atoi(getenv("GNN_TRAIN_SPREAD")) : 0;
    p.spread = spread_env;
#endif
    p.KP = split ? std::max(tg_kps(K), tg_kps(std::min(128, (n_cols + 31) / 32 * 32))) : tg_kp(K);      // (split: the tile is re-used for the pass's output columns)
    const size_t lds = sizeof(float) * ((size_t)TG_WAVES * 32 * p.KP + 32 + 128) + 16;
    if (lds > 160 * 1024) return gnn_fail(GNN_ERR_UNSUPPORTED, "layer input width %d too large for the matrix-core path", K);
    const int64_t n_tiles = (n + 31) / 32;
    const unsigned grid = (unsigned)std::min<int64_t>(TG_MAX_GRID, (n_tiles + TG_WAVES - 1) / TG_WAVES);
    for (int col0 = 0; col0 < n_cols;) {
        const int left = (n_cols - col0 + 31) / 32, NO = left >= 4 ? 4 : (left >= 2 ? 2 : 1);
        int rc;
        p.col0 = col0;
        if (split) {
            const int chunks_img = (K + 15) / 16 + 2;
            uint32_t *img = nullptr;
            if ((rc = buf.get(&img, (size_t)chunks_img * NO * 3 * 256))) return rc;
            hipLaunchKernelGGL(k_pack_split, cdiv((int64_t)chunks_img * NO * 256, 256), 256, 0, st, K, n_cols, col0, NO, chunks_img, M, img);
            p.wp = reinterpret_cast<const float *>(img);
            p.kk = (int)((size_t)chunks_img * NO * 3 * 256 * sizeof(uint32_t));      // bytes of the image (buffer descriptor)
            if (NO == 4) hipLaunchKernelGGL((k_gemm_split<4>), grid, 64 * TG_WAVES, lds, st, p);
            else if (NO == 2) hipLaunchKernelGGL((k_gemm_split<2>), grid, 64 * TG_WAVES, lds, st, p);
            else hipLaunchKernelGGL((k_gemm_split<1>), grid, 64 * TG_WAVES, lds, st, p);
        } else {
            p.kk = tg_kk(K);
            float *wp = nullptr;
            const int kk_img = p.kk + 8;
            if ((rc = buf.get(&wp, (size_t)kk_img * 64 * NO))) return rc;
            hipLaunchKernelGGL(k_pack_exact, cdiv((int64_t)kk_img * 64 * NO, 256), 256, 0, st, K, n_cols, col0, NO, kk_img, M, wp);
            p.wp = wp;
            if (NO == 4) hipLaunchKernelGGL((k_gemm_f32<4>), grid, 64 * TG_WAVES, lds, st, p);
            else if (NO == 2) hipLaunchKernelGGL((k_gemm_f32<2>), grid, 64 * TG_WAVES, lds, st, p);
            else hipLaunchKernelGGL((k_gemm_f32<1>), grid, 64 * TG_WAVES, lds, st, p);
        }
        HIPCHK(hipGetLastError());
        col0 += 32 * NO;
    }
    return GNN_OK;
}

bool fwd3_covers(const gnn_mlp *m)
{
    if (m->n_layers != 3) return false;
    const int a = m->acts[0];
    if (a == GNN_ACT_SOFTMAX || m->acts[1] != a || m->acts[2] != a) return false;
    return m->dims[0] >= 64 && m->dims[0] <= 144 && m->dims[1] > 64 && m->dims[1] <= 128 && m->dims[2] > 64 && m->dims[2] <= 128 && m->dims[3] > 32 && m->dims[3] <= 64;
}

int launch_fwd3(hipStream_t st, Buf &buf, const gnn_mlp *m, int64_t n, const float *x, float *a0, float *a1, float *a2)
{
    static bool lds_raised[64] = {false};
    const void *ks[6] = {reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_LINEAR>), reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_RELU>),
                         reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_SELU>), reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_ELU>),
                         reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_TANH>), reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_SIGMOID>)};
    (void)gnn_raise_dynamic_lds(ks, 6, 160 * 1024, lds_raised);
    const bool keep = a0 != nullptr || a1 != nullptr;
    if (keep && !(a0 && a1)) return gnn_fail(GNN_ERR_STATE, "internal: the three-layer chain stores both hidden activations or neither");
    if (!keep) {
        static bool lds_raised_nk[64] = {false};
        const void *nk[6] = {reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_LINEAR, false>), reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_RELU, false>),
                             reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_SELU, false>), reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_ELU, false>),
                             reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_TANH, false>), reinterpret_cast<const void *>(&k_fwd3_split<GNN_ACT_SIGMOID, false>)};
        (void)gnn_raise_dynamic_lds(nk, 6, 160 * 1024, lds_raised_nk);
    }
    Fwd3Args p{};
    p.n = n; p.K = m->dims[0]; p.w1 = m->dims[1]; p.w2 = m->dims[2]; p.w3 = m->dims[3]; p.act = m->acts[0];
    p.KP = std::max(tg_kps(p.K), tg_kps(128));
    p.chunks0 = (p.K + 15) / 16;
    const size_t blk = 3 * 256;                                          // dwords per (chunk, tile)
    const size_t d0 = (size_t)(p.chunks0 + 2) * 4 * blk, d1 = (size_t)8 * 4 * blk, d2 = (size_t)8 * 2 * blk;
    uint32_t *img = nullptr;
    int rc = buf.get(&img, d0 + d1 + d2);
    if (rc) return rc;
    const bool fold = p.act == GNN_ACT_SELU;
    const float LOG2E = 1.44269504088896341f, SCALE = 1.0507009873554805f;
    hipLaunchKernelGGL(k_pack_split, cdiv((int64_t)(p.chunks0 + 2) * 4 * 256, 256), 256, 0, st, p.K, p.w1, 0, 4, p.chunks0 + 2, m->W[0], img, 0, fold ? LOG2E : 1.0f);
    hipLaunchKernelGGL(k_pack_split, cdiv((int64_t)8 * 4 * 256, 256), 256, 0, st, p.w1, p.w2, 0, 4, 8, m->W[1], img + d0, 1, fold ? SCALE : 1.0f);
    hipLaunchKernelGGL(k_pack_split, cdiv((int64_t)8 * 2 * 256, 256), 256, 0, st, p.w2, p.w3, 0, 2, 8, m->W[2], img + d0 + d1, 1, fold ? SCALE / LOG2E : 1.0f);
    p.img = img; p.img_bytes = (int)((d0 + d1 + d2) * sizeof(uint32_t)); p.off1 = (int)(d0 * sizeof(uint32_t)); p.off2 = (int)((d0 + d1) * sizeof(uint32_t));
    p.X = x; p.b0 = m->b[0]; p.b1 = m->b[1]; p.b2 = m->b[2]; p.A0 = a0; p.A1 = a1; p.A2 = a2;
    const size_t lds = sizeof(float) * ((size_t)TG_WAVES * 32 * p.KP + 32 + 320) + 16;
    if (lds > 160 * 1024) return gnn_fail(GNN_ERR_UNSUPPORTED, "fused forward: LDS");
    const int64_t n_tiles = (n + 31) / 32;
    const unsigned grid = (unsigned)std::min<int64_t>(TG_MAX_GRID, (n_tiles + TG_WAVES - 1) / TG_WAVES);
    if (keep)
        switch (p.act) {
        case GNN_ACT_LINEAR: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_LINEAR>), grid, 64 * TG_WAVES, lds, st, p); break;
        case GNN_ACT_RELU: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_RELU>), grid, 64 * TG_WAVES, lds, st, p); break;
        case GNN_ACT_SELU: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_SELU>), grid, 64 * TG_WAVES, lds, st, p); break;
        case GNN_ACT_ELU: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_ELU>), grid, 64 * TG_WAVES, lds, st, p); break;
        case GNN_ACT_TANH: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_TANH>), grid, 64 * TG_WAVES, lds, st, p); break;
        default: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_SIGMOID>), grid, 64 * TG_WAVES, lds, st, p); break;
        }
    else
        switch (p.act) {
        case GNN_ACT_LINEAR: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_LINEAR, false>), grid, 64 * TG_WAVES, lds, st, p); break;
        case GNN_ACT_RELU: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_RELU, false>), grid, 64 * TG_WAVES, lds, st, p); break;
        case GNN_ACT_SELU: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_SELU, false>), grid, 64 * TG_WAVES, lds, st, p); break;
        case GNN_ACT_ELU: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_ELU, false>), grid, 64 * TG_WAVES, lds, st, p); break;
        case GNN_ACT_TANH: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_TANH, false>), grid, 64 * TG_WAVES, lds, st, p); break;
        default: hipLaunchKernelGGL((k_fwd3_split<GNN_ACT_SIGMOID, false>), grid, 64 * TG_WAVES, lds, st, p); break;
        }
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

}   // namespace gnn_train

namespace {

// The backward chain of the same 3-layer net in ONE pass over the rows (round 5): d z2 (the gradient at the last layer's pre-activation) ->
//     d z1 = (d z2 . W2^T) * act'(a1)  ->  d z0 = (d z1 . W1^T) * act'(a0)  ->  d inp = d z0 . W0^T
// with the chain of the fused kernels - the first product from the wave's LDS tile, the following ones from the previous accumulators without
// leaving registers (layer_split_from_regs with the identity in place of the activation) - and d z1, d z0 (operands of the weight gradients)
// and d inp written out on the way, each through the LDS tile as whole row pieces.  The stored activations a1 / a0 pass through the same tile
// (coalesced rows in, accumulator layout out).  Replaces three k_gemm_split passes (+ the narrow fourth for columns >= 128 of d inp): d z1 and
// d z0 are no longer re-read and re-staged (2 x 512 MB at 1 M rows), one launch instead of four.
struct Bwd3Args {
    int64_t n;
    int K0, w1, w2, w3, KP, chunksA, act;
    int img_bytes, offB, offC, offD;         // one packed image: W2^T (from LDS, 4 tiles) | W1^T (from registers, 4 tiles) | W0^T columns [0, 128) | [128, K0)
    const float *DZ2, *A1, *A0;
    const uint32_t *img;
    float *DZ1, *DZ0, *DINP;
    // optional (DSG != nullptr): the two column blocks of d inp the state gradient reads - own state [0, Ds) and aggregated state [c_aggs, c_aggs + Ds) -
    // once more as 16-byte aligned rows [n, 2 Ds] (the concat's rows are 135 floats long and its aggregate block starts at column 67: k_state_grad_rows
    // gathers ten rows of it per node with 4-byte loads; from the aligned copy with 16-byte loads)
    float *DSG;
    int Ds, c_aggs;
};

__global__ void __launch_bounds__(64 * TG_WAVES, 2) k_bwd3_split(const Bwd3Args p)
{
    using namespace gnn_fused_dev;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KP = p.KP;
    float *X = lds + (size_t)wave * 32 * KP;
    float *zb = lds + (size_t)TG_WAVES * 32 * KP + 32;                   // [128] zeros: the accumulators start from it (no bias in a backward product)
    for (int t = threadIdx.x; t < 128; t += blockDim.x) zb[t] = 0.0f;
    __syncthreads();
    const int64_t n_tiles = (p.n + 31) / 32, stride = (int64_t)gridDim.x * TG_WAVES;
    const int half = lane >> 5, node = lane & 31;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(p.img), 0, p.img_bytes, 0x00020000);
    // 32 rows of a dense [n, width] array (width a multiple of 4, <= 128) into the tile as [row][column]: all pieces requested before the first is
    // written (one round trip, covered by the SIMD's other wave); columns [width, zero_to) are zeroed
    auto stage_rows = [&](const float *src_all, int width, int zero_to, int nvalid, int64_t i0) {
        constexpr int MAXQ = 16;                                         // 32 x 128 floats = 16 pieces of 16 bytes per lane
        v4f nxt[MAXQ];
        const int total = nvalid * width;
        const float *src = src_all + i0 * width;
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) {
            const int e = lane * 4 + 256 * q;
            nxt[q] = v4f{0.f, 0.f, 0.f, 0.f};
            if (e < total) nxt[q] = gload4(src + e);
        }
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
        const float inv_w = 1.0f / (float)width;
        if (zero_to > width) {
            const int zw = zero_to - width;
            for (int t = lane_o; t < 32 * zw; t += 64) X[(t / zw) * KP + width + t % zw] = 0.0f;
        }
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) {
            const int e = lane_o * 4 + 256 * q;
            if (e < 32 * width) {
                const int r = (int)(((float)e + 0.5f) * inv_w), c = e - r * width;
                *reinterpret_cast<v4f *>(X + r * KP + c) = nxt[q];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    };
    // accumulators (feature on the register, row on the lane) times act'(stored activation), the activations read from the tile in the same layout
    auto times_act_grad = [&](f32x16 (&h)[4]) {
        int half_o = half;
        asm volatile("" : "+v"(half_o));
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4f a4 = *reinterpret_cast<const v4f *>(X + node * KP + 32 * jt + 8 * q + 4 * half_o);
                h[jt][4 * q] *= act_grad(a4.x, p.act); h[jt][4 * q + 1] *= act_grad(a4.y, p.act);
                h[jt][4 * q + 2] *= act_grad(a4.z, p.act); h[jt][4 * q + 3] *= act_grad(a4.w, p.act);
            }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    };
    // NTT accumulator tiles -> [row][column] in the tile -> whole row pieces to columns [col0, col0 + 32 NTT) of dst [n, width]
    auto store_rows = [&](auto &h, auto NTc, float *dst, int width, int col0, int nvalid, int64_t i0) {
        constexpr int NTT = decltype(NTc)::value;
        int half_o = half;
        asm volatile("" : "+v"(half_o));
#pragma unroll
        for (int jt = 0; jt < NTT; ++jt)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<v4f *>(X + node * KP + 32 * jt + 8 * q + 4 * half_o) = v4f{h[jt][4 * q], h[jt][4 * q + 1], h[jt][4 * q + 2], h[jt][4 * q + 3]};
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        constexpr int PPR = 8 * NTT;
        const bool vec = (width & 3) == 0 && (col0 & 3) == 0;
        int lane_p = lane;
        asm volatile("" : "+v"(lane_p));
#pragma unroll
        for (int u = 0; u < 32 * PPR / 64; ++u) {
            const int idx = lane_p + 64 * u, r = idx / PPR, c = (idx % PPR) * 4;
            if (r < nvalid && col0 + c < width) {
                const v4f a4 = *reinterpret_cast<const v4f *>(X + r * KP + c);
                const int64_t o = (i0 + r) * width + col0 + c;
                if (vec && col0 + c + 4 <= width) *reinterpret_cast<GNN_GLOBAL v4f *>(gptr_w(dst) + o) = a4;
                else {
                    const float v[4] = {a4.x, a4.y, a4.z, a4.w};
                    for (int t = 0; t < 4; ++t) if (col0 + c + t < width) gptr_w(dst)[o + t] = v[t];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    };
    for (int64_t tile = (int64_t)blockIdx.x * TG_WAVES + wave; tile < n_tiles; tile += stride) {
        const int64_t i0 = tile * 32;
        const int nvalid = (int)((p.n - i0) < 32 ? (p.n - i0) : 32);
        f32x16 g[4], acc[4];
        // d z2 tile -> d h2 = d z2 . W2^T
        stage_rows(p.DZ2, p.w3, 16 * p.chunksA, nvalid, i0);
        layer0_split<4, true>(X + node * KP + 8 * half, wrs, lane * 16, 0, p.chunksA, g, zb, half);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        stage_rows(p.A1, p.w2, 128, nvalid, i0);
        times_act_grad(g);                                               // g = d z1
        store_rows(g, std::integral_constant<int, 4>{}, p.DZ1, p.w2, 0, nvalid, i0);
        layer_split_from_regs<4, 4, GNN_ACT_LINEAR>(g, zb, half, acc, wrs, lane * 16, p.offB);
        stage_rows(p.A0, p.w1, 128, nvalid, i0);
        times_act_grad(acc);                                             // acc = d z0
        store_rows(acc, std::integral_constant<int, 4>{}, p.DZ0, p.w1, 0, nvalid, i0);
        layer_split_from_regs<4, 4, GNN_ACT_LINEAR>(acc, zb, half, g, wrs, lane * 16, p.offC);
        f32x16 tail[1];
        if (p.K0 > 128) layer_split_from_regs<4, 1, GNN_ACT_LINEAR>(acc, zb, half, tail, wrs, lane * 16, p.offD);
        // d inp: all K0 columns into the tile, then the tile's rows as ONE flat run of nvalid x K0 floats - it starts on a 16-byte boundary whatever
        // K0 is (32 K0 floats per tile), so memory is written in aligned 16-byte pieces even for K0 = 135 (a piece may straddle two tile rows)
        {
            int half_o = half;
            asm volatile("" : "+v"(half_o));
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<v4f *>(X + node * KP + 32 * jt + 8 * q + 4 * half_o) = v4f{g[jt][4 * q], g[jt][4 * q + 1], g[jt][4 * q + 2], g[jt][4 * q + 3]};
            if (p.K0 > 128) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (128 + 8 * q + 4 * half_o + 4 <= KP)
                        *reinterpret_cast<v4f *>(X + node * KP + 128 + 8 * q + 4 * half_o) = v4f{tail[0][4 * q], tail[0][4 * q + 1], tail[0][4 * q + 2], tail[0][4 * q + 3]};
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const int K0 = p.K0, total = nvalid * K0;
            const float inv_k = 1.0f / (float)K0;
            float *dst = p.DINP + i0 * K0;
            int lane_p = lane;
            asm volatile("" : "+v"(lane_p));
            for (int e = 4 * lane_p; e < total; e += 256) {
                float v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int ee = e + t < total ? e + t : total - 1;
                    const int r = (int)(((float)ee + 0.5f) * inv_k), c = ee - r * K0;
                    v[t] = X[r * KP + c];
                }
                if (e + 4 <= total) *reinterpret_cast<GNN_GLOBAL v4f *>(gptr_w(dst) + e) = v4f{v[0], v[1], v[2], v[3]};
                else
                    for (int t = 0; t < 4; ++t) if (e + t < total) gptr_w(dst)[e + t] = v[t];
            }
            if (p.DSG) {                                                 // [own | aggregate] column blocks as aligned rows
                const int Ds = p.Ds, ppr = Ds >> 1;                      // 16-byte pieces per row of the copy (2 Ds floats)
                float *sg = p.DSG + i0 * 2 * Ds;
                for (int idx = lane_p; idx < nvalid * ppr; idx += 64) {
                    const int r = idx / ppr, q = idx - r * ppr, c = 4 * q < Ds ? 4 * q : p.c_aggs + (4 * q - Ds);
                    const float *x = X + r * KP + c;
                    *reinterpret_cast<GNN_GLOBAL v4f *>(gptr_w(sg) + r * 2 * Ds + 4 * q) = v4f{x[0], x[1], x[2], x[3]};
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
    }
}

}   // namespace

namespace gnn_train {

bool bwd3_covers(const gnn_mlp *m)
{
    return fwd3_covers(m) && (m->dims[1] & 3) == 0 && (m->dims[2] & 3) == 0 && (m->dims[3] & 3) == 0 && m->dims[0] <= 160;
}

// WT[l]: the transposed kernels [n_out, n_in] of the three layers (Net::WT)
int launch_bwd3(hipStream_t st, Buf &buf, const gnn_mlp *m, float *const *WT, int64_t n, const float *dz2, const float *a1, const float *a0, float *dz1,
                float *dz0, float *dinp, float *dsg, int Ds, int c_aggs)
{
    static bool lds_raised[64] = {false};
    (void)gnn_raise_dynamic_lds(reinterpret_cast<const void *>(&k_bwd3_split), 160 * 1024, lds_raised);
    Bwd3Args p{};
    p.n = n; p.K0 = m->dims[0]; p.w1 = m->dims[1]; p.w2 = m->dims[2]; p.w3 = m->dims[3]; p.act = m->acts[0];
    p.KP = std::max(tg_kps(128), tg_kps(p.K0));
    p.chunksA = (p.w3 + 15) / 16;
    const size_t blk = 3 * 256;                                          // dwords per (chunk, tile)
    const size_t dA = (size_t)(p.chunksA + 2) * 4 * blk, dB = (size_t)8 * 4 * blk, dC = (size_t)8 * 4 * blk, dD = (size_t)8 * 1 * blk;
    uint32_t *img = nullptr;
    int rc = buf.get(&img, dA + dB + dC + dD);
    if (rc) return rc;
    // W2^T: [K = w3, n_cols = w2] from the tile (plain k order); W1^T: [w2, w1] and W0^T: [w1, K0] from the accumulators (hidden k order)
    hipLaunchKernelGGL(k_pack_split, cdiv((int64_t)(p.chunksA + 2) * 4 * 256, 256), 256, 0, st, p.w3, p.w2, 0, 4, p.chunksA + 2, WT[2], img, 0, 1.0f);
    hipLaunchKernelGGL(k_pack_split, cdiv((int64_t)8 * 4 * 256, 256), 256, 0, st, p.w2, p.w1, 0, 4, 8, WT[1], img + dA, 1, 1.0f);
    hipLaunchKernelGGL(k_pack_split, cdiv((int64_t)8 * 4 * 256, 256), 256, 0, st, p.w1, p.K0, 0, 4, 8, WT[0], img + dA + dB, 1, 1.0f);
    hipLaunchKernelGGL(k_pack_split, cdiv((int64_t)8 * 1 * 256, 256), 256, 0, st, p.w1, p.K0, 128, 1, 8, WT[0], img + dA + dB + dC, 1, 1.0f);
    p.img = img; p.img_bytes = (int)((dA + dB + dC + dD) * sizeof(uint32_t));
    p.offB = (int)(dA * sizeof(uint32_t)); p.offC = (int)((dA + dB) * sizeof(uint32_t)); p.offD = (int)((dA + dB + dC) * sizeof(uint32_t));
    p.DZ2 = dz2; p.A1 = a1; p.A0 = a0; p.DZ1 = dz1; p.DZ0 = dz0; p.DINP = dinp;
    p.DSG = dsg; p.Ds = Ds; p.c_aggs = c_aggs;
    const size_t lds = sizeof(float) * ((size_t)TG_WAVES * 32 * p.KP + 32 + 128) + 16;
    if (lds > 160 * 1024) return gnn_fail(GNN_ERR_UNSUPPORTED, "fused backward: LDS");
    const int64_t n_tiles = (n + 31) / 32;
    const unsigned grid = (unsigned)std::min<int64_t>(TG_MAX_GRID, (n_tiles + TG_WAVES - 1) / TG_WAVES);
    hipLaunchKernelGGL(k_bwd3_split, grid, 64 * TG_WAVES, lds, st, p);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

}   // namespace gnn_train

namespace {

// [dW; db] partials of one row chunk: D[hf, zf] = sum over the chunk's rows of [H | 1][r, hf] d z[r, zf].  Rows are the K dimension of
// the 32x32x2 MFMA: lane (m, k half) loads H[r0 + 2 kk + k half][32 mt + m] and d z[..][32 nt + m] - whole 128-byte row pieces per
// half-wave, straight from memory, no staging.  Block = 4 waves, each a quarter of the chunk's rows, MT tiles of [H | 1] columns x up to
// two tiles of d z columns; the four partial tiles are added in wave order through LDS (fixed order: run-to-run identical).
struct WgradArgs {
    int64_t n, rows_per_block, pstride;
    int n_in, n_out;
    const float *H, *DZ;
    float *part;
};

template <int MT, int NT2>
__global__ void __launch_bounds__(256, 2) k_wgrad_f32(const WgradArgs p)
{
    using namespace gnn_fused_dev;
    __shared__ float red[3][1024];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 31, kh = lane >> 5;
    const int64_t c0 = (int64_t)blockIdx.x * p.rows_per_block, c1 = c0 + p.rows_per_block < p.n ? c0 + p.rows_per_block : p.n;
    const int64_t quarter = ((c1 - c0 + 3) / 4 + 1) & ~(int64_t)1;                 // even: K-steps are row pairs
    const int64_t r0 = c0 + wave * quarter, r1 = r0 + quarter < c1 ? r0 + quarter : c1;
    const int nt0 = blockIdx.y * NT2;
    f32x16 acc[MT][NT2];
#pragma unroll
    for (int a = 0; a < MT; ++a) zero_acc<NT2>(acc[a]);
    constexpr int PF = 4;
    float av[PF][MT], bv[PF][NT2];
    auto load = [&](int slot, int64_t r) {
        const int64_t rr = r + kh;
        const bool in = rr < r1;
#pragma unroll
        for (int a = 0; a < MT; ++a) {
            const int hf = 32 * a + m;
            av[slot][a] = in ? (hf < p.n_in ? gload1(p.H + rr * p.n_in + hf) : (hf == p.n_in ? 1.0f : 0.0f)) : 0.0f;
        }
#pragma unroll
        for (int b = 0; b < NT2; ++b) {
            const int zf = 32 * (nt0 + b) + m;
            bv[slot][b] = (in && zf < p.n_out) ? gload1(p.DZ + rr * p.n_out + zf) : 0.0f;
        }
    };
#pragma unroll
    for (int s = 0; s < PF; ++s) load(s, r0 + 2 * s);
    for (int64_t r = r0; r < r1; r += 2 * PF) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
            float a_[MT], b_[NT2];
#pragma unroll
            for (int a = 0; a < MT; ++a) a_[a] = av[s][a];
#pragma unroll
            for (int b = 0; b < NT2; ++b) b_[b] = bv[s][b];
            load(s, r + 2 * (s + PF));                                               // rows past r1 load zeros
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
                for (int b = 0; b < NT2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_[a], b_[b], acc[a][b], 0, 0, 0);
        }
    }
    // D[row hf = 32 a + (r & 3) + 8 (r >> 2) + 4 kh][col zf = 32 (nt0 + b) + m]
    float *out = p.part + (size_t)blockIdx.x * p.pstride;
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT2; ++b) {
            if (wave > 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) red[wave - 1][r * 64 + lane] = acc[a][b][r];
            }
            __syncthreads();
            if (wave == 0) {
                const int zf = 32 * (nt0 + b) + m;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[a][b][r];
                    v = v + red[0][r * 64 + lane]; v = v + red[1][r * 64 + lane]; v = v + red[2][r * 64 + lane];
                    const int hf = 32 * a + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    if (hf <= p.n_in && zf < p.n_out) out[(size_t)hf * p.n_out + zf] = v;
                }
            }
            __syncthreads();
        }
}

// The same partials in the split arithmetic of the dense layers (round 5): every fp32 operand cut into three exact bf16 pieces, six piece
// products per term on v_mfma_f32_32x32x16_bf16, fp32 accumulation (error per product <= 3 * 2^-24: fp32-class, run-to-run identical).  Rows are
// the K dimension, 16 per step: lane (m, k half) takes H[r + 8 k half + i][32 a + m], i < 8 - eight coalesced 128-byte row pieces per operand
// tile, no transposition - and cuts them in registers.  What the round-3 experiment of this (below, 0.92 ms against 0.42) lacked: its 5 x 2
// accumulator tiles (160 registers) left no room to have the next step's rows in flight.  Here a block is EIGHT waves: wave w owns d z tile
// w % NT for ALL tiles of [H | 1] (MT x 16 accumulator registers) on rows part w / NT of the chunk, the next step's 8 (MT + 1) row pieces are
// requested before the current step's products, and the 8 / NT partial tiles of an output are added in part order through LDS.
template <int MT, int NT>
__global__ void __launch_bounds__(512, 2) k_wgrad_bf(const WgradArgs p)
{
    using namespace gnn_fused_dev;
    __shared__ float red[8][1024];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 31, kh = lane >> 5;
    constexpr int NP = 8 / NT;                                                     // row parts of a chunk
    const int b = wave % NT, part = wave / NT;
    const int64_t c0 = (int64_t)blockIdx.x * p.rows_per_block, c1 = c0 + p.rows_per_block < p.n ? c0 + p.rows_per_block : p.n;
    const int64_t span = ((c1 - c0 + NP - 1) / NP + 15) & ~(int64_t)15;             // whole K = 16 steps
    const int64_t r0 = c0 + part * span, r1 = r0 + span < c1 ? r0 + span : c1;
    const int zf = 32 * b + m;
    const bool zok = zf < p.n_out;
    f32x16 acc[MT];
    zero_acc<MT>(acc);
    // ONE register set: a tile's eight row pieces are requested again for the NEXT step as soon as this step has cut them into pieces, i.e. a
    // whole step (6 MT MFMAs) ahead of their use (two sets, loaded a step ahead as a block: 28 registers spilled at MT = 5)
    float hv[MT][8], zv[8];
    auto load_z = [&](int64_t r) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t rr = r + 8 * kh + i;
            zv[i] = (rr < r1 && zok) ? gload1(p.DZ + rr * p.n_out + zf) : 0.0f;
        }
    };
    auto load_h = [&](int a, int64_t r) {
        const int hf = 32 * a + m;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t rr = r + 8 * kh + i;
            hv[a][i] = rr < r1 ? (hf < p.n_in ? gload1(p.H + rr * p.n_in + hf) : (hf == p.n_in ? 1.0f : 0.0f)) : 0.0f;
        }
    };
    constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
    if (r0 < r1) {
        load_z(r0);
#pragma unroll
        for (int a = 0; a < MT; ++a) load_h(a, r0);
    }
    for (int64_t r = r0; r < r1; r += 16) {
        v4i pb[3];
        split8(zv, pb[0], pb[1], pb[2]);
        load_z(r + 16);                                                             // (rows past r1 load zeros: no guard around the requests)
#pragma unroll
        for (int a = 0; a < MT; ++a) {
            v4i pa[3];
            split8(hv[a], pa[0], pa[1], pa[2]);
            load_h(a, r + 16);
#pragma unroll
            for (int term = 0; term < 6; ++term) acc[a] = mfma_bf16(pa[PA[term]], pb[PB[term]], acc[a]);
        }
    }
    // D[row hf = 32 a + (r & 3) + 8 (r >> 2) + 4 kh][col zf]
    float *out = p.part + (size_t)blockIdx.x * p.pstride;
#pragma unroll
    for (int a = 0; a < MT; ++a) {
        if (part > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) red[wave][r * 64 + lane] = acc[a][r];
        }
        __syncthreads();
        if (part == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[a][r];
#pragma unroll
                for (int q = 1; q < NP; ++q) v = v + red[b + NT * q][r * 64 + lane];
                const int hf = 32 * a + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (hf <= p.n_in && zok) out[(size_t)hf * p.n_out + zf] = v;
            }
        }
        __syncthreads();
    }
}

#ifdef GNN_DIAG
// EXPERIMENT (diagnostic build, GNN_TRAIN_WGRAD_SPLIT=1; round 3): the same partials in split arithmetic (three exact bf16 pieces per
// operand, six piece products on v_mfma_f32_32x32x16_bf16): rows are the K dimension, 16 per step - lane (m, k half) holds
// H[r + 8 k half + i][32 a + m], i < 8, eight coalesced row pieces per operand tile, cut into pieces in registers.  60 bf16 MFMAs
// (1,920 matrix-pipe cycles) per 16 rows instead of 80 f32 MFMAs (5,120) - and measured SLOWER: 0.92 ms against 0.42 ms per
// 1 M x 129 x 128 gradient (256 VGPRs + 33 spilled; fifty-six dependent row-piece loads per K-step).  Correct (the training tests pass with it).
template <int MT, int NT2>
__global__ void __launch_bounds__(256, 2) k_wgrad_split(const WgradArgs p)
{
    using namespace gnn_fused_dev;
    __shared__ float red[3][1024];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 31, kh = lane >> 5;
    const int64_t c0 = (int64_t)blockIdx.x * p.rows_per_block, c1 = c0 + p.rows_per_block < p.n ? c0 + p.rows_per_block : p.n;
    const int64_t quarter = ((c1 - c0 + 3) / 4 + 15) & ~(int64_t)15;                // whole K = 16 steps
    const int64_t r0 = c0 + wave * quarter, r1 = r0 + quarter < c1 ? r0 + quarter : c1;
    const int nt0 = blockIdx.y * NT2;
    f32x16 acc[MT][NT2];
#pragma unroll
    for (int a = 0; a < MT; ++a) zero_acc<NT2>(acc[a]);
    constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
    auto load_a = [&](int a, int64_t r, float (&v)[8]) {
        const int hf = 32 * a + m;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t rr = r + 8 * kh + i;
            v[i] = rr < r1 ? (hf < p.n_in ? gload1(p.H + rr * p.n_in + hf) : (hf == p.n_in ? 1.0f : 0.0f)) : 0.0f;
        }
    };
    for (int64_t r = r0; r < r1; r += 16) {
        v4i pb[NT2][3];
#pragma unroll
        for (int b = 0; b < NT2; ++b) {
            const int zf = 32 * (nt0 + b) + m;
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t rr = r + 8 * kh + i;
                v[i] = (rr < r1 && zf < p.n_out) ? gload1(p.DZ + rr * p.n_out + zf) : 0.0f;
            }
            split8(v, pb[b][0], pb[b][1], pb[b][2]);
        }
        float va[8], vn[8];
        load_a(0, r, va);
#pragma unroll
        for (int a = 0; a < MT; ++a) {
            if (a + 1 < MT) load_a(a + 1, r, vn);                                    // the next tile's rows are on their way during these MFMAs
            v4i pa[3];
            split8(va, pa[0], pa[1], pa[2]);
#pragma unroll
            for (int term = 0; term < 6; ++term)
#pragma unroll
                for (int b = 0; b < NT2; ++b) acc[a][b] = mfma_bf16(pa[PA[term]], pb[b][PB[term]], acc[a][b]);
#pragma unroll
            for (int i = 0; i < 8; ++i) va[i] = vn[i];
        }
    }
    float *out = p.part + (size_t)blockIdx.x * p.pstride;
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT2; ++b) {
            if (wave > 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) red[wave - 1][r * 64 + lane] = acc[a][b][r];
            }
            __syncthreads();
            if (wave == 0) {
                const int zf = 32 * (nt0 + b) + m;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[a][b][r];
                    v = v + red[0][r * 64 + lane]; v = v + red[1][r * 64 + lane]; v = v + red[2][r * 64 + lane];
                    const int hf = 32 * a + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    if (hf <= p.n_in && zf < p.n_out) out[(size_t)hf * p.n_out + zf] = v;
                }
            }
            __syncthreads();
        }
}

#endif

}   // namespace

namespace gnn_train {

int launch_wgrad_f32(hipStream_t st, int64_t n, int64_t rpb, int parts, int64_t pstride, int n_in, int n_out, const float *H, const float *DZ, float *part)
{
    WgradArgs p{n, rpb, pstride, n_in, n_out, H, DZ, part};
    const int mt = (n_in + 1 + 31) / 32, nt = (n_out + 31) / 32;
    const int nt2 = nt >= 2 ? 2 : 1;
    if (tg_wgrad_bf(n_out)) {
#define GNN_WGB_CASE(M_, N_) if (mt == M_ && nt == N_) { hipLaunchKernelGGL((k_wgrad_bf<M_, N_>), dim3((unsigned)parts), 512, 0, st, p); HIPCHK(hipGetLastError()); return GNN_OK; }
        GNN_WGB_CASE(3, 1) GNN_WGB_CASE(3, 2) GNN_WGB_CASE(3, 4) GNN_WGB_CASE(4, 1) GNN_WGB_CASE(4, 2) GNN_WGB_CASE(4, 4) GNN_WGB_CASE(5, 1) GNN_WGB_CASE(5, 2) GNN_WGB_CASE(5, 4)
#undef GNN_WGB_CASE
    }
    const dim3 grid((unsigned)parts, (unsigned)((nt + nt2 - 1) / nt2));
#ifdef GNN_DIAG
    static const bool split = getenv("GNN_TRAIN_WGRAD_SPLIT") != nullptr;
#define GNN_WG_LAUNCH(M_, N_) if (split) hipLaunchKernelGGL((k_wgrad_split<M_, N_>), grid, 256, 0, st, p); else hipLaunchKernelGGL((k_wgrad_f32<M_, N_>), grid, 256, 0, st, p);
#else
#define GNN_WG_LAUNCH(M_, N_) hipLaunchKernelGGL((k_wgrad_f32<M_, N_>), grid, 256, 0, st, p);
#endif
#define GNN_WG_CASE(M_, N_)                                                                         \
    if (mt == M_ && nt2 == N_) {                                                                    \
        GNN_WG_LAUNCH(M_, N_)                                                                       \
        HIPCHK(hipGetLastError());                                                                  \
        return GNN_OK;                                                                              \
    }
    GNN_WG_CASE(3, 1) GNN_WG_CASE(3, 2) GNN_WG_CASE(4, 1) GNN_WG_CASE(4, 2) GNN_WG_CASE(5, 1) GNN_WG_CASE(5, 2)
#undef GNN_WG_CASE
#undef GNN_WG_LAUNCH
    return gnn_fail(GNN_ERR_UNSUPPORTED, "no matrix-core weight-gradient instantiation for %d x %d tiles", mt, nt2);
}
bool tg_wgrad_covers(int n_in, int n_out) { const int mt = (n_in + 1 + 31) / 32; return mt >= 3 && mt <= 5 && n_out >= 32; }
// split-bf16 form (k_wgrad_bf) when the d z tiles divide the eight waves of a block; the f32-MFMA form (k_wgrad_f32) otherwise
bool tg_wgrad_bf(int n_out)
{
    const int nt = (n_out + 31) / 32;
#ifdef GNN_DIAG
    static const bool bf_off = getenv("GNN_TRAIN_WGRAD_BF") && atoi(getenv("GNN_TRAIN_WGRAD_BF")) == 0;
    if (bf_off) return false;
#endif
    return nt == 1 || nt == 2 || nt == 4;
}
// rows the persistent kernels cover before a wave takes its second tile
int64_t tg_sweep_rows() { return (int64_t)32 * TG_WAVES * TG_MAX_GRID; }

}   // namespace gnn_train
