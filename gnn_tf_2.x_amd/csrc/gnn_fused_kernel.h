// Fused iteration kernels for gfx950 (device code): k_fused_full (state width 64) and k_fused_generic (every other width).  Where a comment
// elsewhere says k_fused it means the two together.  Included by gnn_fused_{l,s}{1,2,3}.hip and gnn_fused_m{l,s}{2,3}.hip, one translation
// unit per layer count, arithmetic mode and "the last layer has its own activation", so that the instantiations compile in parallel.
//
// One launch = one iteration of GNN.Loop (reference GNN/GNN.py:223-242 + :202-220):
// CSR neighbour gather -> net_state (all Dense layers + BatchNormalization) -> convergence test.
//
// Design (DESIGN.md "Fused kernel"):
//   * one wavefront owns a tile of 32 destination nodes from gather to store; the 4 waves of a workgroup never
//     synchronise with each other (no s_barrier in the kernel);
//   * gather: groups of `lpr` lanes walk the CSR rows of 64/lpr nodes at a time, 16 B per lane per neighbour row, up to
//     4 rows in flight per lane, fmaf chain in stored order (bit-identical to the oracle); source ids / weights of a row
//     are fetched coalesced by the group and broadcast with ds_bpermute;
//   * the concat [state | labels | aggregated state | aggregated labels] of the 32 nodes lives only in LDS
//     (32 x KP floats per wave, KP odd => conflict-free column reads), never in HBM;
//   * layers run on v_mfma_f32_32x32x2_f32 in the transposed form H^T = W^T . X^T: weights are the A operand (streamed
//     from L2 in a pre-packed lane order, 16 B per lane per K step for 4 feature tiles, software-pipelined), node
//     activations the B operand.  The accumulator of layer l (feature on the register, node on the lane) becomes the B
//     operand of layer l+1 after 8 v_permlane32_swap per 32x32 tile, so hidden activations never leave registers.
//     MFMA f32 evaluates the same k-ordered fmaf chain as the oracle, hence bit-identical results;
//   * epilogue: BatchNormalization, new state to LDS, per-node relative-L2 test in the oracle's summation order,
//     coalesced 256 B row stores, one slotted atomicOr per wave that still moves.
//
// Template parameters: LAYERS Dense layers; NT 32-wide feature tiles of every hidden layer; NTL tiles of the last layer;
// ACT the activation of the hidden layers (gnn_activation); ACTL that of the last layer: ACT (a net with one activation for all layers) or
// GNN_ACTL_FROM_ARGS (a net whose last layer has its own: GnnFusedArgs::act_last, read in the last-layer epilogue only).
#pragma once
#include <utility>

#include "gnn_common.h"
#include "gnn_fused.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace gnn_fused_dev {

// The tile loop launders its pointers through empty asm statements (fused_opaque_pointers); that hides from the compiler that they
// are global-memory pointers, and it would fall back to flat_load/flat_store (which also tie up the LDS counter).  All
// memory accesses below therefore go through explicit address_space(1) pointers.
#define GNN_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ const GNN_GLOBAL T *gptr(const T *p) { return (const GNN_GLOBAL T *)p; }
template <class T>
__device__ __forceinline__ GNN_GLOBAL T *gptr_w(T *p) { return (GNN_GLOBAL T *)p; }
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef int v4i_ __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4f gload4(const float *p) { return *(const GNN_GLOBAL v4f *)p; }
// Cache policy of the new-state row stores: 0 default, 2 nt, 16 sc1, 1 sc0 (bits of the buffer instructions' aux operand).  Round 5
// (profiles/r05_ab_store_policy.txt, BASELINE size, ms per launch): default 0.681, nt 0.666, sc1 0.678, sc0 sc1 0.679, nt sc1 0.664, sc0 nt 0.661,
// all three 0.663 - every variant with nt gains 2 - 3 %: the rows written for the NEXT iteration no longer displace the table the gather of
// THIS iteration re-reads ten times.  (The once-read CSR ids / weights as nt loads: +1 %, not adopted.)
#ifndef GNN_STORE_AUX
#define GNN_STORE_AUX 2
#endif
// 16 bytes of a new-state row at base (wave-uniform) + off floats (per lane)
__device__ __forceinline__ void gstore_row4(float *base, int64_t off, v4f v)
{
#if GNN_STORE_AUX == 0
    *reinterpret_cast<GNN_GLOBAL v4f *>(gptr_w(base) + off) = v;
#elif GNN_STORE_AUX == 2
    __builtin_nontemporal_store(v, reinterpret_cast<GNN_GLOBAL v4f *>(gptr_w(base) + off));
#else
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7ffffff0, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i_, v), rs, (int)(off * 4), 0, GNN_STORE_AUX);
#endif
}
__device__ __forceinline__ void gstore_row1(float *p, float v)       // one float of a new-state row (exact path: lane = feature)
{
#if GNN_STORE_AUX & 2
    __builtin_nontemporal_store(v, gptr_w(p));
#else
    *gptr_w(p) = v;
#endif
}
// the once-read streams of a tile (CSR ids / weights, row pointers); as non-temporal loads they measured 1 % slower (round 5)
__device__ __forceinline__ float gstream1(const float *p) { return *(const GNN_GLOBAL float *)p; }
__device__ __forceinline__ int gstream1(const int *p) { return *(const GNN_GLOBAL int *)p; }
__device__ __forceinline__ v2f gload2(const float *p) { return *(const GNN_GLOBAL v2f *)p; }
__device__ __forceinline__ float gload1(const float *p) { return *(const GNN_GLOBAL float *)p; }
__device__ __forceinline__ int gload1(const int *p) { return *(const GNN_GLOBAL int *)p; }

// State rows that ANOTHER workgroup of the same launch has written (the persistent small-graph loop, k_small_loop): loads and
// stores that bypass this CU's L1 / write through the XCD's L2 (global_load / global_store ... sc1), the form under which the
// hand-off needs no cache fences (cdna_hip_programming.md Guideline 16, R1; MI355X_MICROARCH.md hand-off table, row 1).
template <bool COH>
__device__ __forceinline__ float sload1(const float *p)
{
    if constexpr (COH) return __hip_atomic_load(const_cast<GNN_GLOBAL float *>((const GNN_GLOBAL float *)p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return gload1(p);
}
template <bool COH>
__device__ __forceinline__ void sstore1(float *p, float v)
{
    if constexpr (COH) __hip_atomic_store((GNN_GLOBAL float *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *(GNN_GLOBAL float *)p = v;
}

__device__ __forceinline__ float shfl_f(float v, int src_lane)
{
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(v)));
}
__device__ __forceinline__ int shfl_i(int v, int src_lane) { return __builtin_amdgcn_ds_bpermute(src_lane << 2, v); }

// lane J of every 16-lane row broadcast to the whole row: one VALU move (DPP row_newbcast), no LDS crossbar, no wait
template <int J>
__device__ __forceinline__ int row_bcast_i(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, 0x150 + J, 0xf, 0xf, true);   // bound_ctrl: no "old" value to materialise
}
template <int J>
__device__ __forceinline__ float row_bcast_f(float v) { return __int_as_float(row_bcast_i<J>(__float_as_int(v))); }

// after this, for q = 0..3: registers {4q, 4q+2, 4q+1, 4q+3} hold, in that order, the k pairs (8q, 8q+1), (8q+2, 8q+3),
// (8q+4, 8q+5), (8q+6, 8q+7) of the tile: lower half-wave the even k, upper half-wave the odd k (MFMA B-operand order)
__device__ __forceinline__ void acc_to_operand(f32x16 &h)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int r0 = 4 * q + 2 * t, r1 = r0 + 1;
            auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(h[r0]), __float_as_uint(h[r1]), false, false);
            h[r0] = __uint_as_float(sw[0]);
            h[r1] = __uint_as_float(sw[1]);
        }
    }
}

template <int N>
__device__ __forceinline__ void load_w(const float *p, float (&w)[N])
{
    if constexpr (N == 4) {
        const v4f t = gload4(p);
        w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
    } else if constexpr (N == 2) {
        const v2f t = gload2(p);
        w[0] = t.x; w[1] = t.y;
    } else {
        w[0] = gload1(p);
    }
}

template <int ACT>
__device__ __forceinline__ float act_t(float v)
{
    if constexpr (ACT == GNN_ACT_SELU) {
        // gnn_act(v, SELU) with the parts of gnn_expf that cannot influence the result removed: exp is only used for
        // v <= 0 (no overflow side), NaN propagates through the arithmetic, and below the underflow threshold both forms
        // give e - 1 == -1.  On every input this returns the same bits as the generic form.
        const float u = v * 1.44269504088896341f;
        const float n = __builtin_rintf(u);
        const float f = u - n;
        float p = 0.0013218672247603536f;
        p = __builtin_fmaf(p, f, 0.009671698324382305f);
        p = __builtin_fmaf(p, f, 0.05550893023610115f);
        p = __builtin_fmaf(p, f, 0.24022237956523895f);
        p = __builtin_fmaf(p, f, 0.6931468844413757f);
        p = __builtin_fmaf(p, f, 1.0f);
        const float e = __builtin_ldexpf(p, (int)n);
        const float neg = 1.6732632423543772f * (e - 1.0f);
        return 1.0507009873554805f * (v > 0.0f ? v : neg);
    } else {
        return gnn_act(v, ACT);     // ACT is a compile-time constant: the switch folds
    }
}

// act_t on a PAIR of elements with the arithmetic on packed float2 operands (v_pk_mul / add / fma_f32: two IEEE results per issue
// slot, the same bits as the scalar instructions in the same order)
template <int ACT>
__device__ __forceinline__ v2f act_t2(v2f v)
{
    if constexpr (ACT == GNN_ACT_SELU) {
        auto splat = [](float c) { return v2f{c, c}; };
        const v2f u = v * splat(1.44269504088896341f);
        const v2f n = v2f{__builtin_rintf(u.x), __builtin_rintf(u.y)};
        const v2f f = u - n;
        v2f p = __builtin_elementwise_fma(splat(0.0013218672247603536f), f, splat(0.009671698324382305f));
        p = __builtin_elementwise_fma(p, f, splat(0.05550893023610115f));
        p = __builtin_elementwise_fma(p, f, splat(0.24022237956523895f));
        p = __builtin_elementwise_fma(p, f, splat(0.6931468844413757f));
        p = __builtin_elementwise_fma(p, f, splat(1.0f));
        v2f e = v2f{__builtin_ldexpf(p.x, (int)n.x), __builtin_ldexpf(p.y, (int)n.y)};
        e = splat(1.6732632423543772f) * (e - splat(1.0f));
        return splat(1.0507009873554805f) * v2f{v.x > 0.0f ? v.x : e.x, v.y > 0.0f ? v.y : e.y};
    } else {
        return v2f{act_t<ACT>(v.x), act_t<ACT>(v.y)};
    }
}

// Activations of the split-arithmetic path (tolerance-based parity, so the hardware transcendentals are admissible):
// v_exp_f32 / v_rcp_f32 are accurate to 1 ulp; the formulas are those of gnn_act.
template <int ACT>
__device__ __forceinline__ float act_fast(float v)
{
    constexpr float LOG2E = 1.44269504088896341f, SCALE = 1.0507009873554805f, ALPHA = 1.6732632423543772f;
    if constexpr (ACT == GNN_ACT_SELU) {
        const float e = __builtin_amdgcn_exp2f(v * LOG2E);
        return v > 0.0f ? SCALE * v : __builtin_fmaf(e, SCALE * ALPHA, -(SCALE * ALPHA));
    } else if constexpr (ACT == GNN_ACT_ELU) {
        return v > 0.0f ? v : __builtin_amdgcn_exp2f(v * LOG2E) - 1.0f;
    } else if constexpr (ACT == GNN_ACT_SIGMOID) {
        return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -LOG2E));
    } else if constexpr (ACT == GNN_ACT_TANH) {
        const float t = __builtin_amdgcn_exp2f(__builtin_fabsf(v) * (-2.0f * LOG2E));
        const float q = (1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t);
        return v < 0.0f ? -q : q;
    } else {
        return gnn_act(v, ACT);
    }
}

// bias + activation (+ BatchNormalization when BN) on one accumulator tile; feature of register r on this lane:
// 32 jt + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
// LDS: the three vectors were staged in LDS at kernel start (last layer of the tile loop: no global round trips per tile)
// NOBIAS: the accumulator was started from the bias (split arithmetic, bias_tile)
// fmax: features >= fmax are padding of the tile (never stored): groups of registers that hold only such features are skipped
// us: scale of the accumulator undone first (NOBIAS: the fp16-piece format's 2^-(e_w + e_x), else 1)
template <int ACT, bool BN, bool FAST = false, bool LDS = false, bool NOBIAS = false>
__device__ __forceinline__ void tile_epilogue(f32x16 &a, const float *bias, const float *bn_scale, const float *bn_shift,
                                              int jt, int half, int fmax = 1 << 30, float us = 1.0f)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (32 * jt + 8 * q >= fmax) continue;           // (wave-uniform)
        const int f0 = 32 * jt + 8 * q + 4 * half;
        v4f b = {0.f, 0.f, 0.f, 0.f};
        if constexpr (!NOBIAS) b = LDS ? *reinterpret_cast<const v4f *>(bias + f0) : gload4(bias + f0);
        const float bb[4] = {b.x, b.y, b.z, b.w};
        float sc[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
        if (BN) {
            const v4f s4 = LDS ? *reinterpret_cast<const v4f *>(bn_scale + f0) : gload4(bn_scale + f0);
            const v4f h4 = LDS ? *reinterpret_cast<const v4f *>(bn_shift + f0) : gload4(bn_shift + f0);
            sc[0] = s4.x; sc[1] = s4.y; sc[2] = s4.z; sc[3] = s4.w;
            sh[0] = h4.x; sh[1] = h4.y; sh[2] = h4.z; sh[3] = h4.w;
        }
        if constexpr (FAST) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float v = NOBIAS ? a[4 * q + t] * us : a[4 * q + t] + bb[t];
                v = act_fast<ACT>(v);
                if (BN) { const float m = v * sc[t]; v = m + sh[t]; }
                a[4 * q + t] = v;
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; t += 2) {             // pairs: packed arithmetic, the same bits
                v2f v = v2f{a[4 * q + t], a[4 * q + t + 1]};
                if constexpr (!NOBIAS) v = v + v2f{bb[t], bb[t + 1]};
                v = act_t2<ACT>(v);
                if (BN) { const v2f m = v * v2f{sc[t], sc[t + 1]}; v = m + v2f{sh[t], sh[t + 1]}; }
                a[4 * q + t] = v.x;
                a[4 * q + t + 1] = v.y;
            }
        }
    }
}

// The LAST layer's epilogue.  ACTL a gnn_activation: tile_epilogue<ACTL>.  ACTL == GNN_ACTL_FROM_ARGS: the same forms - act_t2 (exact) /
// act_fast (split) of the activation act_last - behind a wave-uniform switch (act_last is a kernel argument), so one instantiation per
// hidden activation serves every last activation with the bits of the instantiation that has it as a constant.
template <int ACTL, bool BN, bool FAST = false, bool LDS = false, bool NOBIAS = false>
__device__ __forceinline__ void tile_epilogue_last(int act_last, f32x16 &a, const float *bias, const float *bn_scale, const float *bn_shift,
                                                   int jt, int half, int fmax = 1 << 30, float us = 1.0f)
{
    if constexpr (ACTL != GNN_ACTL_FROM_ARGS) {
        tile_epilogue<ACTL, BN, FAST, LDS, NOBIAS>(a, bias, bn_scale, bn_shift, jt, half, fmax, us);
    } else {
        switch (act_last) {
        case GNN_ACT_RELU: tile_epilogue<GNN_ACT_RELU, BN, FAST, LDS, NOBIAS>(a, bias, bn_scale, bn_shift, jt, half, fmax, us); break;
        case GNN_ACT_SELU: tile_epilogue<GNN_ACT_SELU, BN, FAST, LDS, NOBIAS>(a, bias, bn_scale, bn_shift, jt, half, fmax, us); break;
        case GNN_ACT_ELU: tile_epilogue<GNN_ACT_ELU, BN, FAST, LDS, NOBIAS>(a, bias, bn_scale, bn_shift, jt, half, fmax, us); break;
        case GNN_ACT_TANH: tile_epilogue<GNN_ACT_TANH, BN, FAST, LDS, NOBIAS>(a, bias, bn_scale, bn_shift, jt, half, fmax, us); break;
        case GNN_ACT_SIGMOID: tile_epilogue<GNN_ACT_SIGMOID, BN, FAST, LDS, NOBIAS>(a, bias, bn_scale, bn_shift, jt, half, fmax, us); break;
        default: tile_epilogue<GNN_ACT_LINEAR, BN, FAST, LDS, NOBIAS>(a, bias, bn_scale, bn_shift, jt, half, fmax, us); break;
        }
    }
}

// Dense layer whose input is the LDS tile X (layer 0).  KK (multiple of 12) K-steps in groups of 4 with three register
// sets: the weight loads / LDS reads of group g+2 are issued before the MFMAs of group g, i.e. 8 K-steps (2048 matrix
// cycles) ahead.  Reads past the end land in the zero slack of the packed image / LDS (see gnn_fused.hip) and are unused.
template <int NO>
__device__ __forceinline__ void layer_from_lds(const float *xb, const float *wp, int kk_total, f32x16 (&acc)[NO], int wstride)
{
    constexpr int PF = 4;
    float wa[PF][NO], wb[PF][NO], wc[PF][NO], ba[PF], bb[PF], bc[PF];
#define GNN_L0_LOAD(W, B, K0)                                                                       \
    _Pragma("unroll") for (int u = 0; u < PF; ++u) {                                                \
        load_w<NO>(wp + (size_t)((K0) + u) * 64 * NO * wstride, W[u]);                                        \
        B[u] = xb[2 * ((K0) + u)];                                                                  \
    }                                                                                               \
    __builtin_amdgcn_sched_barrier(0);
#define GNN_L0_MFMA(W, B)                                                                           \
    _Pragma("unroll") for (int u = 0; u < PF; ++u)                                                  \
        _Pragma("unroll") for (int jt = 0; jt < NO; ++jt)                                           \
            acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(W[u][jt], B[u], acc[jt], 0, 0, 0);       \
    __builtin_amdgcn_sched_barrier(0);
    GNN_L0_LOAD(wa, ba, 0)
    GNN_L0_LOAD(wb, bb, PF)
    for (int kk = 0; kk < kk_total; kk += 3 * PF) {
        GNN_L0_LOAD(wc, bc, kk + 2 * PF)
        GNN_L0_MFMA(wa, ba)
        GNN_L0_LOAD(wa, ba, kk + 3 * PF)
        GNN_L0_MFMA(wb, bb)
        GNN_L0_LOAD(wb, bb, kk + 4 * PF)
        GNN_L0_MFMA(wc, bc)
    }
#undef GNN_L0_LOAD
#undef GNN_L0_MFMA
}

// Activation of a PAIR of accumulator elements, split into eight stages so that it can be issued in the shadow of
// consecutive MFMAs (the wave issues in order, so VALU work has to sit BETWEEN the MFMAs to overlap with anything).  The
// arithmetic runs on packed float2 operands (v_pk_mul/add/fma_f32: two IEEE results per issue slot, the same bits as the
// scalar instructions).  The concatenation of the stages is exactly act_t<ACT>(v + bias) on both elements.
template <int ACT>
struct ActPipe2 {
    v2f t, u, n, f, p, e;
    static __device__ __forceinline__ v2f splat(float c) { return v2f{c, c}; }
    __device__ __forceinline__ void stage(int st, float v0, float v1, float b0, float b1, float &o0, float &o1)
    {
        if constexpr (ACT == GNN_ACT_SELU) {
            switch (st) {
            case 0: t = v2f{v0, v1} + v2f{b0, b1}; u = t * splat(1.44269504088896341f); break;
            case 1: n = v2f{__builtin_rintf(u.x), __builtin_rintf(u.y)}; f = u - n; break;
            case 2: p = __builtin_elementwise_fma(splat(0.0013218672247603536f), f, splat(0.009671698324382305f));
                    p = __builtin_elementwise_fma(p, f, splat(0.05550893023610115f)); break;
            case 3: p = __builtin_elementwise_fma(p, f, splat(0.24022237956523895f));
                    p = __builtin_elementwise_fma(p, f, splat(0.6931468844413757f)); break;
            case 4: p = __builtin_elementwise_fma(p, f, splat(1.0f)); break;
            case 5: e = v2f{__builtin_ldexpf(p.x, (int)n.x), __builtin_ldexpf(p.y, (int)n.y)}; e = e - splat(1.0f); break;
            case 6: e = e * splat(1.6732632423543772f); break;
            case 7: {
                const v2f r = v2f{t.x > 0.0f ? t.x : e.x, t.y > 0.0f ? t.y : e.y} * splat(1.0507009873554805f);
                o0 = r.x; o1 = r.y;
            } break;
            }
        } else {
            if (st == 0) t = v2f{v0, v1} + v2f{b0, b1};
            if (st == 7) { o0 = gnn_act(t.x, ACT); o1 = gnn_act(t.y, ACT); }
        }
    }
};

// Dense layer whose input is the RAW accumulator of the previous layer (hin).  The previous layer's epilogue (bias +
// activation, then the half-wave exchange that turns an accumulator tile into B operands) is applied here and
// software-pipelined against this layer's MFMAs in plain program order: K-step ss of input tile ti issues NO MFMAs, and
// BETWEEN them (the wave issues in order, so that is the only place where VALU work overlaps the matrix pipe) sit the
// stages of the epilogue of element ss of input tile ti + 1 (ActPipe; on odd ss also the exchange of the pair).  Only the
// epilogue of tile 0 is exposed.  16 NI K-steps, fully unrolled; weight loads are issued DEPTH steps ahead of their MFMAs; a sched_barrier after
// every step pins this order.
template <int NI, int NO, int ACT>
__device__ __forceinline__ void layer_from_regs(f32x16 (&hin)[NI], const float *bias_prev, int half, f32x16 (&acc)[NO],
                                                const float *wp, int wstride)
{
    constexpr int STEPS = 16 * NI, DEPTH = 8;
    float w[STEPS][NO];
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) load_w<NO>(wp + (size_t)s * 64 * NO * wstride, w[s]);
    tile_epilogue<ACT, false>(hin[0], bias_prev, nullptr, nullptr, 0, half);
    acc_to_operand(hin[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ti = 0; ti < NI; ++ti) {
        float nb[16];                                   // biases of the 16 features this lane holds of tile ti + 1
        if (ti + 1 < NI) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4f b4 = gload4(bias_prev + 32 * (ti + 1) + 8 * q + 4 * half);
                nb[4 * q] = b4.x; nb[4 * q + 1] = b4.y; nb[4 * q + 2] = b4.z; nb[4 * q + 3] = b4.w;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        ActPipe2<ACT> ap;
#pragma unroll
        for (int ss = 0; ss < 16; ++ss) {
            const int s = 16 * ti + ss;
            if (s + DEPTH < STEPS) load_w<NO>(wp + (size_t)(s + DEPTH) * 64 * NO * wstride, w[s + DEPTH]);
            const int reg = 4 * (ss >> 2) + ((ss & 3) == 1 ? 2 : (ss & 3) == 2 ? 1 : (ss & 3));
            const float b = hin[ti][reg];
            const bool epi = ti + 1 < NI;
            const int pe = ss & ~1;                                  // the pair (pe, pe + 1) spans steps pe and pe + 1
#pragma unroll
            for (int jt = 0; jt < NO; ++jt) {
                acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[s][jt], b, acc[jt], 0, 0, 0);
                if (epi) {      // stages of the epilogue of elements (pe, pe + 1) of tile ti + 1, in the shadow of this MFMA
                    constexpr int SPM = 4 / NO;                      // stages per MFMA: NO = 4 -> 1, 2 -> 2, 1 -> 4
#pragma unroll
                    for (int q = jt * SPM; q < (jt + 1) * SPM; ++q) {
                        const int st = (ss & 1) * 4 + q;             // even step: stages 0..3, odd step: stages 4..7
                        float o0 = 0.0f, o1 = 0.0f;
                        ap.stage(st, hin[ti + 1][pe], hin[ti + 1][pe + 1], nb[pe], nb[pe + 1], o0, o1);
                        if (st == 7) {
                            auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(o0), __float_as_uint(o1), false, false);
                            hin[ti + 1][pe] = __uint_as_float(sw[0]);
                            hin[ti + 1][pe + 1] = __uint_as_float(sw[1]);
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// SPLIT arithmetic (impl 2): fp32 operands as three bf16 pieces on v_mfma_f32_32x32x16_bf16.
//
// The f32 MFMA of gfx950 issues at the f32 VALU rate and shares its pipe; the bf16 MFMA is 13x faster per K and overlaps
// the partner wave's VALU work.  Every fp32 value v is cut, by truncation, into p0 + p1 + p2 == v EXACTLY (8 + 8 + 8
// mantissa bits; the remainders v - p0 and v - p0 - p1 are exact in fp32), products of pieces are exact in the fp32
// accumulator, and of the nine piece products of x * w the six of relative weight >= 2^-16 are accumulated
// (p0q0, p0q1, p1q0, p1q1, p0q2, p2q0); the dropped ones are <= 3 * 2^-24 |x w|, the size of one fp32 rounding.  What
// differs from the oracle's fmaf chain is therefore only the accumulation order inside the matrix unit: results agree
// to fp32 rounding noise (tests: 1e-5 against the float64 oracle), not bit for bit.  The exact f32-MFMA path stays
// available as impl 1.
//
// Operand layout of the 32x32x16 MFMA: lane l carries 8 consecutive k of row / column l & 31, k group l >> 5.  Which k
// sits where is free as long as weights (A) and activations (B) agree, so the k order of a hidden layer is simply the
// order in which the previous layer's accumulator already holds the features (no cross-lane exchange at all):
//   layer 0, chunk c:                  k(h, i) = 16 c + 8 h + i                      (LDS tile column)
//   hidden, chunk c = 2 ti + q:        k(h, i) = 32 ti + (r & 3) + 8 (r >> 2) + 4 h,  r = 8 q + i   (accumulator register r)
// gnn_fused.hip packs the weight pieces in the same order: [chunk][out tile][piece][lane][8 bf16].
// ---------------------------------------------------------------------------------------------------------------------
typedef int v4i __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ v4i gload4i(const int *p) { return *(const GNN_GLOBAL v4i *)p; }

// weight pieces through the image's buffer descriptor: vector offset = 16 * lane (the same register for every load), everything
// else in the scalar offset, so an unrolled layer issues no vector address arithmetic at all
__device__ __forceinline__ v4i bload4i(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    return __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
// Running scalar offset of a weight stream that is read strictly in image order, 1 KiB per load: four loads share one
// value of the offset (immediate offsets 0 / 1 / 2 / 3 KiB), then ONE scalar add moves it on.  The add is opaque to the compiler
// on purpose: as plain constants the ~200 offsets of an unrolled layer are hoisted out of the tile loop, spilled and fetched
// back with a v_readlane each.
struct WStream {
    int soff, n;
    __device__ __forceinline__ WStream(int start) : soff(start), n(0) {}
    __device__ __forceinline__ v4i next(__amdgpu_buffer_rsrc_t r, int voff)
    {
        // (s_add_u32 writes SCC: without the clobber the compiler kept a loop's s_cmp result live across this statement and the loop of
        // layer0_split16 ran once - found in round 3; the 32-node layers happened to have no SCC value live here)
        if (n == 4) { asm volatile("s_add_u32 %0, %0, 0x1000" : "+s"(soff) : : "scc"); n = 0; }
        return bload4i(r, voff + 1024 * n++, soff);
    }
};

// bias of the 16 features this lane holds of output tile jt, laid out as an accumulator tile: the split-arithmetic layers START
// their accumulators from the bias (4 LDS reads per tile) instead of adding it to every element afterwards (16 VALU adds)
__device__ __forceinline__ f32x16 bias_tile(const float *bias_lds, int jt, int half)
{
    f32x16 t;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const v4f b = *reinterpret_cast<const v4f *>(bias_lds + 32 * jt + 8 * q + 4 * half);
        t[4 * q] = b.x; t[4 * q + 1] = b.y; t[4 * q + 2] = b.z; t[4 * q + 3] = b.w;
    }
    return t;
}

__device__ __forceinline__ void split8(const float (&v)[8], v4i &p0, v4i &p1, v4i &p2)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned a = __float_as_uint(v[2 * j]), b = __float_as_uint(v[2 * j + 1]);
        const float ar = v[2 * j] - __uint_as_float(a & 0xffff0000u), br = v[2 * j + 1] - __uint_as_float(b & 0xffff0000u);
        const unsigned aru = __float_as_uint(ar), bru = __float_as_uint(br);
        const float ar2 = ar - __uint_as_float(aru & 0xffff0000u), br2 = br - __uint_as_float(bru & 0xffff0000u);
        // high halves of (even, odd) element into the (low, high) half of one dword
        p0[j] = (int)__builtin_amdgcn_perm(b, a, 0x07060302u);
        p1[j] = (int)__builtin_amdgcn_perm(bru, aru, 0x07060302u);
        p2[j] = (int)__builtin_amdgcn_perm(__float_as_uint(br2), __float_as_uint(ar2), 0x07060302u);
    }
}

__device__ __forceinline__ f32x16 mfma_bf16(v4i a, v4i b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// one (even, odd) element pair of split8: pieces of v0, v1 into dword j of the three operands
__device__ __forceinline__ void split_pair(float v0, float v1, int &p0, int &p1, int &p2)
{
    const unsigned a = __float_as_uint(v0), b = __float_as_uint(v1);
    const float ar = v0 - __uint_as_float(a & 0xffff0000u), br = v1 - __uint_as_float(b & 0xffff0000u);
    const unsigned aru = __float_as_uint(ar), bru = __float_as_uint(br);
    const float ar2 = ar - __uint_as_float(aru & 0xffff0000u), br2 = br - __uint_as_float(bru & 0xffff0000u);
    p0 = (int)__builtin_amdgcn_perm(b, a, 0x07060302u);
    p1 = (int)__builtin_amdgcn_perm(bru, aru, 0x07060302u);
    p2 = (int)__builtin_amdgcn_perm(__float_as_uint(br2), __float_as_uint(ar2), 0x07060302u);
}

// ---- piece format 2 (the default): fp32 operands as two fp16 pieces on v_mfma_f32_32x32x16_f16 ----
// A value is scaled by a power of two s (exact), then cut with round-to-nearest-even: p0 = f16(v s), p1 = f16(v s - p0) (the remainder is
// exact in fp32); p0 + p1 carries 22 - 24 significant bits, and of the four piece products the three of relative weight >= 2^-12 are
// accumulated (p1 q0, p0 q1, p0 q0); the dropped p1 q1 is <= 2^-24 |x w|.  Weights are scaled per layer (gnn_fused_pack: max |W s| in
// [2^14, 2^15)), activations by the fixed 2^GNN_F16_EX.  p1 is an fp16 subnormal for every |x| < 2^-7 (and for some x up to 2^-3); the
// conversion and the MFMA keep subnormals (tests/test_fp16_edges.py, bit for bit), so the cut's error there is at most 2^-29 absolute:
// relative max(2^-23, 2^-29 / |x|), 2^-19 at |x| = 1e-3, 2^-23 from 2^-6 on.  The accumulator,
// started from the bias times the same 2^(e_w + e_x), is scaled back by 2^-(e_w + e_x) (exact) where the activation reads it.  A scaled
// activation of magnitude >= GNN_F16_LIMIT would round to an fp16 infinity: the wave raises the range word of its flag slot, and the host
// repeats the Loop in format 3 (run_loops).  The fp16 operand lane map is the bf16 one, so the k orders above hold unchanged.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x16 mfma_f16(v4i a, v4i b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// one (even, odd) element pair: scale, fp16 pieces of both into dword j of the two operands (v_pk_mul_f32, v_cvt_pk_f16_f32, 2 v_cvt_f32_f16,
// v_pk_add_f32, v_cvt_pk_f16_f32), and the running max |scaled value| of the range guard (one v_max3_f32 with |abs| modifiers)
__device__ __forceinline__ void split_pair_f16(float v0, float v1, int &p0, int &p1, float &mx)
{
    constexpr float S = (float)(1 << GNN_F16_EX);
    const v2f s = v2f{v0, v1} * v2f{S, S};
    mx = __builtin_fmaxf(mx, __builtin_fmaxf(__builtin_fabsf(s.x), __builtin_fabsf(s.y)));
    const f16x2 h0 = __builtin_convertvector(s, f16x2);
    const v2f r = s - __builtin_convertvector(h0, v2f);
    const f16x2 h1 = __builtin_convertvector(r, f16x2);
    p0 = __builtin_bit_cast(int, h0);
    p1 = __builtin_bit_cast(int, h1);
}
__device__ __forceinline__ void split8_f16(const float (&v)[8], v4i &p0, v4i &p1, float &mx)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int q0, q1;
        split_pair_f16(v[2 * j], v[2 * j + 1], q0, q1, mx);
        p0[j] = q0; p1[j] = q1;
    }
}
// Range guard of a hidden layer's operand: max |accumulator| x us x 2^GNN_F16_EX bounds every scaled activation the cut will see (every
// activation has |act(v)| <= max(|v|, 2.5): the folded SELU's negative branch stays above -2.42), so it is taken once over the accumulators
// instead of inside the cut, by the kernels between the layers (a running maximum threaded through the pipelined cuts, or this check at the top
// of layer_split_from_regs, raised the register peak of the headline instantiation past 256: 180 - 272 bytes of scratch).
template <int NI>
__device__ __forceinline__ float hidden_range(const f32x16 (&h)[NI], float us)
{
    float m = 0.0f;
#pragma unroll
    for (int t = 0; t < NI; ++t)
#pragma unroll
        for (int r = 0; r < 16; r += 2) m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fabsf(h[t][r]), __builtin_fabsf(h[t][r + 1])));
    return m * (us * (float)(1 << GNN_F16_EX));
}

// Product terms of one chunk, smallest first, for piece format PC: weight piece PA[t] times activation piece PB[t]
template <int PC> struct SplitTerms;
template <> struct SplitTerms<3> {
    static constexpr int N = 6;
    static constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
};
template <> struct SplitTerms<2> {
    static constexpr int N = 3;
    static constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
};
template <int PC>
__device__ __forceinline__ f32x16 mfma_piece(v4i a, v4i b, f32x16 c)
{
    if constexpr (PC == 2) return mfma_f16(a, b, c);
    else return mfma_bf16(a, b, c);
}
// the operand pieces of 8 consecutive elements in format PC (mx: range guard of format 2, untouched by format 3)
template <int PC>
__device__ __forceinline__ void split8_pc(const float (&v)[8], v4i (&p)[PC], float &mx)
{
    if constexpr (PC == 2) split8_f16(v, p[0], p[1], mx);
    else split8(v, p[0], p[1], p[2]);
}
// a wave whose cuts met an out-of-range value raises word 3 of its flag slot (exchanged between ranks with the gate words)
__device__ __forceinline__ void gnn_flag_raise_range(int *flag_rank_base, float mx)
{
    if (__any(mx >= GNN_F16_LIMIT) && (threadIdx.x & 63) == 0) {
        int *w = flag_rank_base + (blockIdx.x & (GNN_FLAG_SLOTS - 1)) * GNN_FLAG_STRIDE + 3;
        if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(w, 1);
    }
}

// the six piece products of one K = 16 chunk on T output tiles; consecutive MFMAs go to different accumulators
template <int T>
__device__ __forceinline__ void mfma_split(const v4i (&w)[T][3], v4i b0, v4i b1, v4i b2, f32x16 *acc)
{
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = mfma_bf16(w[t][0], b2, acc[t]);      // smallest terms first
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = mfma_bf16(w[t][2], b0, acc[t]);
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = mfma_bf16(w[t][1], b1, acc[t]);
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = mfma_bf16(w[t][0], b1, acc[t]);
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = mfma_bf16(w[t][1], b0, acc[t]);
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = mfma_bf16(w[t][0], b0, acc[t]);
}

// layer 0: input = LDS tile.  xr = X + (lane & 31) * KP + 8 * (lane >> 5); wl = split image of the layer + 4 * lane.
// Two register sets: the weights / tile values of chunk c + 1 are requested before the MFMAs of chunk c.  The image has
// two zero chunks of slack and the LDS allocation 128 B, so the look-ahead never leaves them; it is never consumed.
// SEED (label projection): acc arrives holding the tile's seed - the label terms and the bias of the layer, already at the accumulator's
// scale (seed_tiles) - and the first MFMA of every output tile takes it as C; bias_lds is not read.
template <int NO, bool AL16, int PC = 3, bool SEED = false>
__device__ __forceinline__ void layer0_split(const float *xr, __amdgpu_buffer_rsrc_t wrs, int voff, int soff, int n_chunks, f32x16 (&acc)[NO],
                                             const float *bias_lds, int half, float &mx)
{
    using TM = SplitTerms<PC>;
    v4i wa[NO][PC], wb[NO][PC];
    float xa[8], xb[8];
    v4i pa[PC], pb[PC];                                // operand pieces of the chunk whose weights sit in wa / wb
    WStream ws(soff);                                  // chunks are requested in ascending order: 0, 1, 2, ...
#define GNN_S0_LOAD(W, XV, C)                                                                       \
    _Pragma("unroll") for (int jt = 0; jt < NO; ++jt)                                               \
        _Pragma("unroll") for (int pc = 0; pc < PC; ++pc)                                           \
            W[jt][pc] = ws.next(wrs, voff);                                                         \
    if constexpr (AL16) {                                                                           \
        const v4f lo_ = *reinterpret_cast<const v4f *>(xr + 16 * (C)), hi_ = *reinterpret_cast<const v4f *>(xr + 16 * (C) + 4);   \
        XV[0] = lo_.x; XV[1] = lo_.y; XV[2] = lo_.z; XV[3] = lo_.w; XV[4] = hi_.x; XV[5] = hi_.y; XV[6] = hi_.z; XV[7] = hi_.w;    \
    } else {                                                                                        \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) XV[i] = xr[16 * (C) + i];                     \
    }                                                                                               \
    __builtin_amdgcn_sched_barrier(0);
    // the piece products of the chunk in W / P; after the first NO MFMAs the pieces of the NEXT chunk (values XN, already in registers)
    // are cut in the shadow of the matrix pipe: format 3 one element pair per following MFMA, format 2 (2 NO MFMAs left) spread evenly
#define GNN_S0_MFMA(W, P, XN, PN, Z, LIVE)                                                          \
    {                                                                                               \
        float mn_ = 0.0f;                                                                           \
        _Pragma("unroll") for (int term = 0; term < TM::N; ++term)                                  \
            _Pragma("unroll") for (int t = 0; t < NO; ++t) {                                        \
                acc[t] = mfma_piece<PC>(W[t][TM::PA[term]], P[TM::PB[term]], (!SEED && Z && term == 0) ? bias_tile(bias_lds, t, half) : acc[t]);   \
                const int m = term * NO + t;                                                        \
                constexpr int SL = TM::N * NO - NO;                                                 \
                _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                     \
                    const bool due = PC == 3 ? (m == NO + j) : (m >= NO && (m - NO) == j * SL / 4); \
                    if (due) {                                                                      \
                        if constexpr (PC == 3) {                                                    \
                            int q0, q1, q2;                                                         \
                            split_pair(XN[2 * j], XN[2 * j + 1], q0, q1, q2);                       \
                            PN[0][j] = q0; PN[1][j] = q1; PN[PC - 1][j] = q2;                       \
                        } else {                                                                    \
                            int q0, q1;                                                             \
                            split_pair_f16(XN[2 * j], XN[2 * j + 1], q0, q1, mn_);                  \
                            PN[0][j] = q0; PN[1][j] = q1;                                           \
                        }                                                                           \
                    }                                                                               \
                }                                                                                   \
                __builtin_amdgcn_sched_barrier(0);                                                  \
            }                                                                                       \
        if (PC == 2 && (LIVE)) mx = __builtin_fmaxf(mx, mn_);   /* (the look-ahead past the last chunk is not guarded) */   \
    }
    GNN_S0_LOAD(wa, xa, 0)
    split8_pc<PC>(xa, pa, mx);
    GNN_S0_LOAD(wb, xb, 1)
    GNN_S0_MFMA(wa, pa, xb, pb, true, 1 < n_chunks)    // chunk 0 starts the accumulators from the layer's bias
    for (int c = 1; c < n_chunks; c += 2) {
        GNN_S0_LOAD(wa, xa, c + 1)
        GNN_S0_MFMA(wb, pb, xa, pa, false, c + 1 < n_chunks)
        GNN_S0_LOAD(wb, xb, c + 2)
        if (c + 1 < n_chunks) GNN_S0_MFMA(wa, pa, xb, pb, false, c + 2 < n_chunks)
    }
#undef GNN_S0_LOAD
#undef GNN_S0_MFMA
}

// format 3 without the range guard (the training kernels of gnn_train_wide.hip)
template <int NO, bool AL16>
__device__ __forceinline__ void layer0_split(const float *xr, __amdgpu_buffer_rsrc_t wrs, int voff, int soff, int n_chunks, f32x16 (&acc)[NO],
                                             const float *bias_lds, int half)
{
    float mx = 0.0f;
    layer0_split<NO, AL16, 3>(xr, wrs, voff, soff, n_chunks, acc, bias_lds, half, mx);
}

// hidden / last layer: input = accumulator tiles of the previous layer; its epilogue (bias + activation; bias_prev points to the
// copy staged in LDS at kernel start) is applied here,
// software-pipelined in program order against this layer's MFMAs (the wave issues in order; VALU work placed right after
// an MFMA runs while the matrix pipe executes it): while the 6 NO MFMAs of chunk c are issued, the 8 elements of chunk
// c + 2 get bias + activation (E) and the elements of chunk c + 1 are cut into bf16 pieces (S), one task per few MFMAs.
// Units of (chunk, pair of output tiles), fully unrolled, weights requested DEPTH units ahead.
// PC: piece format (3 = bf16 x 3, 2 = fp16 x 2: hin holds the previous layer's accumulators times 2^(e_w + e_x); us = 2^-(e_w + e_x)).
template <int NI, int NO, int ACT, int PC = 3>
__device__ __forceinline__ void layer_split_from_regs(f32x16 (&hin)[NI], const float *bias_lds, int half, f32x16 (&acc)[NO],
                                                      __amdgpu_buffer_rsrc_t wrs, int voff, int soff, float us, float &mx)
{
    using TM = SplitTerms<PC>;
    constexpr int TPU = NO >= 2 ? 2 : 1, UPC = NO / TPU, CH = 2 * NI, U = CH * UPC;
    // 24 VGPRs per unit in flight next to 16 (NI + NO) of activations (128 -> 128: depth 2 spills ~40 VGPRs and is slower in the bf16 format;
    // the fp16 pieces leave room for it: GNN_S1_DEPTH_WIDE, an A/B switch)
#ifndef GNN_S1_DEPTH_WIDE
#define GNN_S1_DEPTH_WIDE 1
#endif
    constexpr int DEPTH = (NI + NO >= 8) ? (PC == 2 ? GNN_S1_DEPTH_WIDE : 1) : 3;
    constexpr int NM = TM::N * NO, NTASK = 12;              // MFMAs per chunk; VALU tasks per chunk: 8 E elements, then 4 S pairs (late:
                                                        // the pieces of chunk c + 1 become live when b2 / b1 of chunk c are dead)
    v4i w[U][TPU][PC];
    int bp[2][PC][4];                                    // operand pieces of chunk c (bp[c & 1]) and c + 1
    WStream ws(soff);                                   // units are requested in ascending order = image order
#define GNN_S1_LOAD(UU)                                                                             \
    _Pragma("unroll") for (int t = 0; t < TPU; ++t)                                                 \
        _Pragma("unroll") for (int pc = 0; pc < PC; ++pc) w[UU][t][pc] = ws.next(wrs, voff);
    // (the previous layer's accumulators already contain its bias: bias_tile)
#define GNN_S1_H(C, I) hin[(C) >> 1][8 * ((C) & 1) + (I)]
    // SELU between dense layers, folded (gnn_fused_pack scales the split image to match): the accumulator holds v' = log2(e) v, the
    // operand handed to the next layer is x' = v' (v > 0) or log2(e) alpha (2^v' - 1), and the next layer's weights carry the factor
    // scale / log2(e).  Four instructions per element (exp2, compare, fma, select) instead of six.
#define GNN_S1_E(C, I)                                                                              \
    if constexpr (ACT == GNN_ACT_SELU) {                                                            \
        constexpr float AL2_ = 1.6732632423543772f * 1.44269504088896341f;                          \
        const float v_ = PC == 2 ? GNN_S1_H(C, I) * us : GNN_S1_H(C, I);                            \
        GNN_S1_H(C, I) = v_ > 0.0f ? v_ : __builtin_fmaf(__builtin_amdgcn_exp2f(v_), AL2_, -AL2_);  \
    } else GNN_S1_H(C, I) = act_fast<ACT>(PC == 2 ? GNN_S1_H(C, I) * us : GNN_S1_H(C, I));
#define GNN_S1_S(C, J, DST)                                                                         \
    if constexpr (PC == 2) { float mz_ = 0.0f; split_pair_f16(GNN_S1_H(C, 2 * (J)), GNN_S1_H(C, 2 * (J) + 1), DST[0][J], DST[1][J], mz_); }   \
    else split_pair(GNN_S1_H(C, 2 * (J)), GNN_S1_H(C, 2 * (J) + 1), DST[0][J], DST[1][J], DST[PC - 1][J]);
    // (Halving the tasks - one half per MFMA gap instead of a whole task after every second MFMA - was measured: 5 % slower.)
#pragma unroll
    for (int u = 0; u < DEPTH && u < U; ++u) { GNN_S1_LOAD(u) }
    {   // prologue: E(0), S(0), E(1)
#pragma unroll
        for (int i = 0; i < 8; ++i) { GNN_S1_E(0, i) }
#pragma unroll
        for (int j = 0; j < 4; ++j) { GNN_S1_S(0, j, bp[0]) }
#pragma unroll
        for (int i = 0; i < 8; ++i) { GNN_S1_E(1, i) }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
        for (int up = 0; up < UPC; ++up) {
            const int u = c * UPC + up;
            if (u + DEPTH < U) { GNN_S1_LOAD(u + DEPTH) }
            // term order as mfma_split: smallest products first
#pragma unroll
            for (int term = 0; term < TM::N; ++term) {
#pragma unroll
                for (int t = 0; t < TPU; ++t) {
                    const int *bq = bp[c & 1][TM::PB[term]];
                    // the first MFMA of an accumulator takes the layer's bias as C (no zeroed register tile, no bias add later)
                    acc[up * TPU + t] = mfma_piece<PC>(w[u][t][TM::PA[term]], v4i{bq[0], bq[1], bq[2], bq[3]},
                                                  (c == 0 && term == 0) ? bias_tile(bias_lds, up * TPU + t, half) : acc[up * TPU + t]);
                    // VALU tasks due after MFMA number m of the chunk: [(m - 1) NTASK / NM, m NTASK / NM).  (Grouping the tasks of 2 or 4
                    // consecutive MFMAs behind the last of them was measured in round 4: no effect, DESIGN.md appendix.)
                    const int m = (up * TM::N + term) * TPU + t + 1;
                    const int k0 = (m - 1) * NTASK / NM, k1 = m * NTASK / NM;
#pragma unroll
                    for (int k = 0; k < NTASK; ++k) {
                        if (k >= k0 && k < k1) {
                            if (k < 8) { if (c + 2 < CH) { GNN_S1_E(c + 2, k) } }
                            else { if (c + 1 < CH) { GNN_S1_S(c + 1, k - 8, bp[(c + 1) & 1]) } }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
#undef GNN_S1_LOAD
#undef GNN_S1_E
#undef GNN_S1_S
#undef GNN_S1_H
}

template <int NI, int NO, int ACT>
__device__ __forceinline__ void layer_split_from_regs(f32x16 (&hin)[NI], const float *bias_lds, int half, f32x16 (&acc)[NO],
                                                      __amdgpu_buffer_rsrc_t wrs, int voff, int soff)
{
    float mx = 0.0f;
    layer_split_from_regs<NI, NO, ACT, 3>(hin, bias_lds, half, acc, wrs, voff, soff, 1.0f, mx);
}

// ---------------------------------------------------------------------------------------------------------------------
// tile load + gather.  X[32][KP] columns: [state | nodes? | aggregated state | aggregated nodes? | aggregated arcs | 0 pad]
// ---------------------------------------------------------------------------------------------------------------------

// label columns [nodes | agg nodes | agg arcs] of inv[n_rows][IW] -> columns Ds.., 2Ds+NLc.., 2Ds+2NLc..
__device__ __forceinline__ int label_col(int c, int Ds, int NLc, int c_aggs)
{
    return c < NLc ? Ds + c : c_aggs + Ds + (c - NLc);      // [nodes] behind the state, [agg nodes | agg arcs] behind the aggregated state
}

// (row, column) of the flat index lane, lane + 64, lane + 128, ... of a [rows, width] block: one division per tile instead
// of one per element (the generic paths are latency chains of small graphs; an integer division is ~40 instructions)
struct RowCol {
    int i, c, qi, qc, width;
    __device__ __forceinline__ RowCol(int lane, int width_) : width(width_)
    {
        i = lane / width; c = lane - i * width;
        qi = 64 / width; qc = 64 - qi * width;
    }
    __device__ __forceinline__ void next()
    {
        i += qi; c += qc;
        if (c >= width) { c -= width; ++i; }
    }
};

__device__ __forceinline__ void zero_pad_columns(const GnnFusedArgs &a, float *X, int lane, int KP)
{
    const int padw = KP - a.in_s;
    RowCol rc(lane, padw);
    for (int t = lane; t < 32 * padw; t += 64, rc.next()) X[rc.i * KP + a.in_s + rc.c] = 0.0f;
    const int hole0 = a.Ds + a.NLc, holew = a.c_aggs - hole0;      // alignment hole in front of the aggregated-state block (0 - 3 columns)
    if (holew > 0 && lane < 32)
        for (int c = 0; c < holew; ++c) X[lane * KP + hole0 + c] = 0.0f;
}

// Generic shapes (any Ds, partial tiles).  Correct for everything, tuned for nothing: small graphs are launch-bound.
// COH: the state rows are read with L1-bypassing loads (see sload1).
// own_from_lds (k_small_loop, bodies > 0): the tile is still in LDS from the previous body - zero padding and label columns are
// unchanged, the new own state sits in columns c_aggs.. and only has to move to columns 0..
// RND: entries per round of the narrow gather (ids / weights, then rows of RND entries requested together)
// ecache_src / ecache_w (k_small_loop): the tile's arc ids / weights, entries [ecache_base, ...), already in LDS - the narrow gather then
// pays one memory round trip per round (the rows) instead of two (ids, then rows)
template <bool COH = false, int RND = 4>
__device__ __forceinline__ void load_tile_generic(const GnnFusedArgs &a, float *X, const int *ipt, int64_t i0, int lane,
                                               int nvalid, int KP, int c_aggs, bool own_from_lds = false, const int *ecache_src = nullptr,
                                               const float *ecache_w = nullptr, int ecache_base = 0, bool skip_gather = false)
{
    const int Ds = a.Ds, NLc = a.NLc;
    if (!own_from_lds) {
        zero_pad_columns(a, X, lane, KP);
        if (nvalid < 32) {
            RowCol rc(lane, a.in_s);
            for (int t = lane; t < (32 - nvalid) * a.in_s; t += 64, rc.next()) X[(nvalid + rc.i) * KP + rc.c] = 0.0f;
        }
    }
    if (own_from_lds) {
        const int total = nvalid * Ds;
        RowCol rc(lane, Ds);
        for (int t = lane; t < total; t += 64, rc.next()) X[rc.i * KP + rc.c] = X[rc.i * KP + c_aggs + rc.c];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // before the aggregated state overwrites those columns
    } else {   // own state rows (contiguous in HBM) into columns [0, Ds)
        const float *src = a.state_cur + (a.row_begin + i0) * Ds;
        const int total = nvalid * Ds;
        RowCol rc(lane, Ds);
        for (int t = lane; t < total; t += 64, rc.next()) X[rc.i * KP + rc.c] = sload1<COH>(src + t);
    }
    if (a.IW > 0 && !own_from_lds) {
        const float *src = a.inv + i0 * a.IW;
        const int total = nvalid * a.IW;
        RowCol rc(lane, a.IW);
        for (int t = lane; t < total; t += 64, rc.next()) X[rc.i * KP + label_col(rc.c, Ds, NLc, c_aggs)] = gload1(src + t);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (skip_gather) return;       // k_small_loop: the aggregate comes from the padded exchange rows (small_gather_padded)
    if (a.agg_in) {        // feature-sliced exchange: the aggregate of the owned rows was computed outside (contiguous rows, no gather)
        const float *src = a.agg_in + i0 * Ds;
        const int total = nvalid * Ds;
        RowCol rc(lane, Ds);
        for (int t = lane; t < total; t += 64, rc.next()) X[rc.i * KP + c_aggs + rc.c] = gload1(src + t);
        return;
    }
    if (Ds <= 32) {
        // narrow rows (small label-sized states): lane = (node, column half); all 32 nodes walk their entries at once, so
        // the latency chain is max-degree long instead of 32 / groups passes long
        const int node = lane & 31, hf = lane >> 5;
        const int cbeg = hf ? (Ds + 1) / 2 : 0, cend = hf ? Ds : (Ds + 1) / 2;
        const int beg = ipt[node], end = ipt[node + 1];
        float acc[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = 0.0f;
        // RND entries per round: their ids / weights are requested together, then their rows, then the fmaf chain in stored
        // order - two memory latencies per round instead of two per entry
        for (int e = beg; e < end; e += RND) {
            float w[RND];
            const float *xp[RND];
#pragma unroll
            for (int u = 0; u < RND; ++u) {
                const int ee = e + u < end ? e + u : e;        // clamp: a real entry, result unused
                w[u] = ecache_w ? ecache_w[ee - ecache_base] : gload1(a.adj_w + ee);
                xp[u] = a.state_cur + (int64_t)(ecache_src ? ecache_src[ee - ecache_base] : gload1(a.adj_src + ee)) * Ds + cbeg;
            }
            float x[RND][16];
#pragma unroll
            for (int u = 0; u < RND; ++u)
#pragma unroll
                for (int c = 0; c < 16; ++c) x[u][c] = (cbeg + c < cend) ? sload1<COH>(xp[u] + c) : 0.0f;
#pragma unroll
            for (int u = 0; u < RND; ++u)
                if (e + u < end) {
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (cbeg + c < cend) acc[c] = __builtin_fmaf(w[u], x[u][c], acc[c]);
                }
        }
        if (node < nvalid) {
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (cbeg + c < cend) X[node * KP + c_aggs + cbeg + c] = acc[c];
        }
        return;
    }
    // gather: groups of lpr lanes, one node per group per pass, one column chunk per lane (lpr * vec >= Ds); the entries
    // of a row are consumed four at a time (ids, weights and rows of the four requested before the first fmaf)
    const int lpr = a.lpr, gl = lane & (lpr - 1), grp = lane >> a.lpr_log2, groups = 64 >> a.lpr_log2;
    const bool colok = gl * a.vec < Ds;
    const int c0 = colok ? gl * a.vec : 0;
    for (int pass = 0; pass * groups < 32; ++pass) {
        const int i = pass * groups + grp;                 // < 32 because groups divides 32 (lpr >= 2)
        const int beg = ipt[i], end = ipt[i + 1];          // rows past nvalid: beg == end
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int e = beg; e < end; e += 4) {
            float w[4];
            v4f x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ee = e + u < end ? e + u : e;    // clamp: a real entry, result unused
                w[u] = gload1(a.adj_w + ee);
                const float *xp = a.state_cur + (int64_t)gload1(a.adj_src + ee) * Ds + c0;
                if (a.vec == 4) {
                    if constexpr (COH) x[u] = v4f{sload1<true>(xp), sload1<true>(xp + 1), sload1<true>(xp + 2), sload1<true>(xp + 3)};
                    else x[u] = gload4(xp);
                } else x[u] = v4f{sload1<COH>(xp), 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (e + u < end) {
                    acc[0] = __builtin_fmaf(w[u], x[u].x, acc[0]);
                    if (a.vec == 4) {
                        acc[1] = __builtin_fmaf(w[u], x[u].y, acc[1]); acc[2] = __builtin_fmaf(w[u], x[u].z, acc[2]);
                        acc[3] = __builtin_fmaf(w[u], x[u].w, acc[3]);
                    }
                }
            }
        }
        if (i < nvalid && colok) {
            float *x = X + i * KP + c_aggs + c0;
            x[0] = acc[0];
            if (a.vec == 4) { x[1] = acc[1]; x[2] = acc[2]; x[3] = acc[3]; }
        }
    }
}

// one entry of the Ds == 64 gather: acc += w * row piece (4 floats per lane), the oracle's fmaf chain.  Four v_fma_f32, as inline asm so that
// the compiler does not pair them into two v_pk_fma_f32 (same bits): MI355X_MICROARCH.md prices a packed f32 operation beside the SIMD partner's
// MFMAs at +22 cycles over the scalar pair; A/B of round 5 at BASELINE size: 0.683 against 0.687 ms per launch (profiles/r05_ab_gather_fma.txt).
__device__ __forceinline__ void gather_fma(v2f &acc01, v2f &acc23, float w, v4f x)
{
    float a0 = acc01.x, a1 = acc01.y, a2 = acc23.x, a3 = acc23.y;
    asm("v_fma_f32 %0, %1, %2, %0" : "+v"(a0) : "v"(w), "v"(x.x));
    asm("v_fma_f32 %0, %1, %2, %0" : "+v"(a1) : "v"(w), "v"(x.y));
    asm("v_fma_f32 %0, %1, %2, %0" : "+v"(a2) : "v"(w), "v"(x.z));
    asm("v_fma_f32 %0, %1, %2, %0" : "+v"(a3) : "v"(w), "v"(x.w));
    acc01 = v2f{a0, a1}; acc23 = v2f{a2, a3};
}

// one batch of the Ds == 64 gather: entry J of the group's batch (held by lane J of the 16-lane row) is broadcast to the
// row, and the 16 lanes request the 256-byte neighbour row, 16 B each
template <int GB, int... J>
__device__ __forceinline__ void gather_batch(int my_src, float my_w, __amdgpu_buffer_rsrc_t rsrc, int voff0, float (&w)[GB],
                                             v4f (&x)[GB], std::integer_sequence<int, J...>)
{
    ((w[J] = row_bcast_f<J>(my_w),
      x[J] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (row_bcast_i<J>(my_src) << 8) + voff0, 0, 0))), ...);
}

// Ds == 64, full tile.  Lane group g (16 lanes, 16 B per lane = one 256 B state row per group and instruction) owns the
// 8 consecutive nodes 8g..8g+7 and walks their contiguous CSR entries in batches of GB: ids/weights of a batch are fetched
// coalesced by the group (and those of the next batch prefetched), the GB neighbour rows are all requested before the
// first is consumed (GB x 4 groups x 256 B = 16 KiB in flight per wave), and the fmaf chain runs in stored order,
// flushing to LDS at every row boundary.
// AL16: rows of the tile and the aggregated-state block are 16-byte aligned (split arithmetic): one ds_write_b128 per row piece
// The zero padding of the tile (columns behind the concat, alignment hole) is already in place: nothing in a tile's life writes those
// columns, so the kernel zeroes them once per wave instead of once per tile
// (Two batches of GB rows in flight per lane group were measured in round 2: 4 % slower, DESIGN.md appendix.)
// Own state rows and label columns of a full Ds == 64 tile: 8 x 16 B + 4 floats per lane requested in front of the gather, written to
// LDS behind it (their latency hides behind the gather)
template <bool AL16>
struct TileOwn64 {
    v4f own[8];
    float lab[4];
    __device__ __forceinline__ void request(const GnnFusedArgs &a, int64_t i0, int lane)
    {
        const float *src = a.state_cur + (a.row_begin + i0) * 64 + lane * 4;
#pragma unroll
        for (int u = 0; u < 8; ++u) own[u] = gload4(src + u * 256);      // (as non-temporal loads: +2.5 %, round 5 - these rows are other tiles' neighbour rows too)
        const int IW = a.IW, nlab = 32 * IW;
        const float *lsrc = a.inv + i0 * IW;
#pragma unroll
        for (int u = 0; u < 4; ++u) lab[u] = (lane + 64 * u < nlab) ? gload1(lsrc + lane + 64 * u) : 0.0f;
    }
    __device__ __forceinline__ void write(const GnnFusedArgs &a, float *X, int64_t i0, int lane, int KP, int c_aggs) const
    {
        constexpr int Ds = 64;
        const int IW = a.IW, nlab = 32 * IW;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float *x = X + (4 * u + (lane >> 4)) * KP + (lane & 15) * 4;         // flat element 256 u + 4 lane = row 4u + lane/16
            if constexpr (AL16) *reinterpret_cast<v4f *>(x) = own[u];
            else { x[0] = own[u].x; x[1] = own[u].y; x[2] = own[u].z; x[3] = own[u].w; }
        }
        const float inv_iw = 1.0f / (float)(IW > 0 ? IW : 1);                    // t / IW without an integer division: exact for t < 2^16
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = lane + 64 * u;
            if (t < nlab) {
                const int i = (int)(((float)t + 0.5f) * inv_iw), c = t - i * IW;
                X[i * KP + label_col(c, Ds, a.NLc, c_aggs)] = lab[u];
            }
        }
        if (nlab > 256)                                                          // wide label blocks: the rest, plainly
            for (int t = 256 + lane; t < nlab; t += 64) {
                const int i = t / IW, c = t - i * IW;
                X[i * KP + label_col(c, Ds, a.NLc, c_aggs)] = gload1(a.inv + i0 * IW + t);
            }
    }
};

template <bool AL16>
__device__ __forceinline__ void load_tile_fast64(const GnnFusedArgs &a, float *X, const int *ipt, int64_t i0, int lane,
                                                 int KP, int c_aggs, int my_src, float my_w)
{
    constexpr int GB = 16;
    const int gl = lane & 15, grp = lane >> 4;
    TileOwn64<AL16> own;
    own.request(a, i0, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                   // ipt visible to the whole wave

    int node = grp * 8;
    const int node_end = node + 8;
    const int e_begin = ipt[node], e_end = ipt[node_end];
    int next_end = ipt[node + 1];
    v2f acc01 = {0.f, 0.f}, acc23 = {0.f, 0.f};
    // neighbour rows through a buffer descriptor: 32-bit byte offsets (src * 256 + 16 * lane-in-row) instead of 64-bit
    // pointer arithmetic per row; the state replica is < 2 GiB by the fused path's precondition (gnn_loop_decide_form)
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.state_cur), 0, (int)a.state_bytes, 0x00020000);
    const int voff0 = gl * 16;
    float *xo = X + c_aggs + gl * 4;
#define GNN_ROW_BOUNDARY(e)                                                                     \
    while ((e) >= next_end) {                                                                   \
        float *xr = xo + node * KP;                                                             \
        if constexpr (AL16) *reinterpret_cast<v4f *>(xr) = v4f{acc01.x, acc01.y, acc23.x, acc23.y};   \
        else { xr[0] = acc01.x; xr[1] = acc01.y; xr[2] = acc23.x; xr[3] = acc23.y; }            \
        acc01 = v2f{0.f, 0.f}; acc23 = v2f{0.f, 0.f};                                           \
        ++node;                                                                                 \
        next_end = ipt[node + 1];                                                               \
    }
    // (my_src, my_w): ids / weights of the group's first batch, requested during the previous tile (tile_first_ids)
    int base = e_begin;
    for (; base + GB <= e_end; base += GB) {                                 // full batches: no guards
        float w[GB];
        v4f x[GB];
        gather_batch<GB>(my_src, my_w, rsrc, voff0, w, x, std::make_integer_sequence<int, GB>{});
        const int nb = base + GB + gl;                                       // ids / weights of the next batch
        my_src = 0; my_w = 0.0f;
        if (nb < e_end) { my_src = gstream1(a.adj_src + nb); my_w = gstream1(a.adj_w + nb); }
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            GNN_ROW_BOUNDARY(base + u)
            gather_fma(acc01, acc23, w[u], x[u]);
        }
    }
    {                                                                        // tail batch: cnt in [0, GB)
        const int cnt = e_end - base;
        float w[GB];
        v4f x[GB];
        // all GB slots are requested (slots >= cnt re-read whatever id the lane holds: entry of this batch or 0 = row 0,
        // always a valid row) and only the first cnt are consumed
        gather_batch<GB>(my_src, my_w, rsrc, voff0, w, x, std::make_integer_sequence<int, GB>{});
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            if (u < cnt) {
                GNN_ROW_BOUNDARY(base + u)
                gather_fma(acc01, acc23, w[u], x[u]);
            }
        }
    }
#undef GNN_ROW_BOUNDARY
    for (; node < node_end; ++node) {                                        // last row with entries, then empty rows
        float *xr = xo + node * KP;
        if constexpr (AL16) *reinterpret_cast<v4f *>(xr) = v4f{acc01.x, acc01.y, acc23.x, acc23.y};
        else { xr[0] = acc01.x; xr[1] = acc01.y; xr[2] = acc23.x; xr[3] = acc23.y; }
        acc01 = v2f{0.f, 0.f}; acc23 = v2f{0.f, 0.f};
    }
    own.write(a, X, i0, lane, KP, c_aggs);                                   // own state and label columns into the tile
}

// ---- wide rows: Ds % 4 == 0, 64 < Ds <= 128, full tile, CSR walk (the wide-state form of k_fused_generic, gnn_loop_set_wide_state) ----
// one batch: entry J of the group's batch (held by lane J of BOTH 16-lane DPP rows of the 32-lane group) is broadcast to its row, and
// the 32 lanes request the neighbour's state row, 16 B each.  rowb: bytes of a state row for the lanes that hold a piece of it, 0 for the
// lanes behind column Ds, whose voff0 is GNN_GP_NOROW - past the descriptor's range, the load returns zeros.  Source ids are below 2^23
// (a replica under 2 GiB of rows over 256 B), so the 24-bit multiply is exact.
template <int GB, int... J>
__device__ __forceinline__ void gather_batch_wide(int my_src, float my_w, __amdgpu_buffer_rsrc_t rsrc, unsigned rowb, int voff0, float (&w)[GB],
                                                  v4f (&x)[GB], std::integer_sequence<int, J...>)
{
    ((w[J] = row_bcast_f<J>(my_w),
      x[J] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)__umul24((unsigned)row_bcast_i<J>(my_src), rowb) + voff0, 0, 0))), ...);
}

// Lane group g (32 lanes, 16 B per lane = one state row of up to 512 B per group and instruction) owns the 16 consecutive nodes
// 16g .. 16g+15 and walks their contiguous CSR entries in batches of 16, as load_tile_fast64 does with four groups of 16 lanes: ids and
// weights of a batch fetched coalesced - by both DPP rows of the group, so that row_bcast serves unchanged - and those of the next batch
// prefetched, all 16 neighbour rows requested before the first is consumed (64 VGPRs in flight per lane), the v_fma_f32 chain per element
// in stored order from +0, flushed to LDS at every row boundary (an empty row writes +0): the C oracle's chain, bit for bit.
// The tile's rows are not 16-byte aligned (KP is odd): four ds_write_b32 per row piece.
// Own state rows: 32 Ds / 4 <= 1,024 pieces of 16 B, up to 16 per lane, requested first of all and written to LDS behind the request for
// the first batch's ids and weights: vector-memory results return in issue order, so the rows are there before the ids are - the wait
// is the one the gather starts with anyway - and their 64 registers are free again when the gather's 64 are needed.  Label columns
// (few, and none in the seeded form) and the zero padding: load_tile_generic's way, in front.
// A partial tile and a given aggregate keep load_tile_generic (k_fused_generic).
__device__ __forceinline__ void load_tile_wide(const GnnFusedArgs &a, float *X, const int *ipt, int64_t i0, int lane, int KP, int c_aggs)
{
    constexpr int GB = 16;
    // (a fresh, compiler-opaque lane id per tile, as fused_opaque_pointers: everything below that depends on the lane and the shapes alone -
    // the row / column of 16 own pieces, the group's offsets - is otherwise computed once per kernel and held across the dense layers)
    // - and likewise the shapes: the kernels stand at 106 scalar registers, and a hoisted scalar is a spill into a vector register
    int Ds = a.Ds;
    asm volatile("" : "+v"(lane));
    asm volatile("" : "+s"(Ds), "+s"(KP), "+s"(c_aggs));
    const int gl = lane & 31, grp = lane >> 5;
    zero_pad_columns(a, X, lane, KP);
    // own state rows, contiguous in HBM: piece t = lane + 64 u of the tile's 8 Ds pieces is columns 4 (t mod Ds / 4) .. of row t / (Ds / 4)
    const int qw = Ds >> 2, n_own = 8 * Ds;
    v4f own[16];
    {
        const float *src = a.state_cur + (a.row_begin + i0) * Ds + lane * 4;
#pragma unroll
        for (int u = 0; u < 16; ++u) own[u] = (lane + 64 * u < n_own) ? gload4(src + u * 256) : v4f{0.f, 0.f, 0.f, 0.f};
    }
    if (a.IW > 0) {
        const float *src = a.inv + i0 * a.IW;
        const int total = 32 * a.IW;
        RowCol rc(lane, a.IW);
        for (int t = lane; t < total; t += 64, rc.next()) X[rc.i * KP + label_col(rc.c, Ds, a.NLc, c_aggs)] = gload1(src + t);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                   // ipt visible to the whole wave

    int node = grp * 16;
    const int node_end = node + 16;
    const int e_begin = ipt[node], e_end = ipt[node_end];
    int next_end = ipt[node + 1];
    int my_src = 0;
    float my_w = 0.0f;
    if (e_begin + (lane & 15) < e_end) { my_src = gstream1(a.adj_src + e_begin + (lane & 15)); my_w = gstream1(a.adj_w + e_begin + (lane & 15)); }
    {   // own state into columns [0, Ds)
        RowCol rc(lane, qw);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (lane + 64 * u < n_own) {
                float *x = X + rc.i * KP + rc.c * 4;
                x[0] = own[u].x; x[1] = own[u].y; x[2] = own[u].z; x[3] = own[u].w;
            }
            rc.next();
        }
    }
    v2f acc01 = {0.f, 0.f}, acc23 = {0.f, 0.f};
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.state_cur), 0, (int)a.state_bytes, 0x00020000);
    const bool colok = gl * 4 < Ds;
    const unsigned rowb = colok ? (unsigned)Ds * 4u : 0u;
    const int voff0 = colok ? gl * 16 : (int)GNN_GP_NOROW;
    float *xo = X + c_aggs + gl * 4;
#define GNN_ROW_BOUNDARY(e)                                                                     \
    while ((e) >= next_end) {                                                                   \
        if (colok) { float *xr = xo + node * KP; xr[0] = acc01.x; xr[1] = acc01.y; xr[2] = acc23.x; xr[3] = acc23.y; }   \
        acc01 = v2f{0.f, 0.f}; acc23 = v2f{0.f, 0.f};                                           \
        ++node;                                                                                 \
        next_end = ipt[node + 1];                                                               \
    }
    int base = e_begin;
    for (; base + GB <= e_end; base += GB) {                                 // full batches: no guards
        float w[GB];
        v4f x[GB];
        gather_batch_wide<GB>(my_src, my_w, rsrc, rowb, voff0, w, x, std::make_integer_sequence<int, GB>{});
        const int nb = base + GB + (lane & 15);                              // ids / weights of the next batch
        my_src = 0; my_w = 0.0f;
        if (nb < e_end) { my_src = gstream1(a.adj_src + nb); my_w = gstream1(a.adj_w + nb); }
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            GNN_ROW_BOUNDARY(base + u)
            gather_fma(acc01, acc23, w[u], x[u]);
        }
    }
    {                                                                        // tail batch: cnt in [0, GB)
        const int cnt = e_end - base;
        float w[GB];
        v4f x[GB];
        // all GB slots are requested (slots >= cnt re-read whatever id the lane holds: an entry of this batch or 0 = row 0, always a
        // valid row) and only the first cnt are consumed
        gather_batch_wide<GB>(my_src, my_w, rsrc, rowb, voff0, w, x, std::make_integer_sequence<int, GB>{});
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            if (u < cnt) {
                GNN_ROW_BOUNDARY(base + u)
                gather_fma(acc01, acc23, w[u], x[u]);
            }
        }
    }
#undef GNN_ROW_BOUNDARY
    for (; node < node_end; ++node) {                                        // last row with entries, then empty rows
        if (colok) { float *xr = xo + node * KP; xr[0] = acc01.x; xr[1] = acc01.y; xr[2] = acc23.x; xr[3] = acc23.y; }
        acc01 = v2f{0.f, 0.f}; acc23 = v2f{0.f, 0.f};
    }
}

// ---- the same tile from the graph's gather program (gather form 2; gnn_gather_program_build) ----
// The CSR structure never changes after the graph is created, so it is walked once, on the host: per tile and lane group the program holds
// the (source word, weight) entries in the order the group consumes them, all four streams padded to the same number of 16-entry batches.
// The tile's 32 rows are split into four contiguous ranges of near-equal entry count (rows whole, entries in CSR order: every row's fmaf
// chain is the one load_tile_fast64 evaluates), the trip count is wave-uniform, and a row end is a bit of the entry: no row pointers, no
// tail batch, no loop inside the batch.
// one entry: the fmaf chain, and at a row end the aggregate to the tile and a fresh accumulator
template <bool AL16, int J>
__device__ __forceinline__ void prog_consume(int words, float w, v4f x, v2f &acc01, v2f &acc23, float *xo, int KP)
{
    gather_fma(acc01, acc23, w, x);
    const unsigned t = (unsigned)row_bcast_i<J>(words);                      // entry J's word again (one DPP move; not kept across the batch)
    if (t & GNN_GP_ROW_END) {                                                // uniform per lane group
        float *xr = xo + __umul24(t & GNN_GP_ROW_MASK, (unsigned)KP);
        if constexpr (AL16) *reinterpret_cast<v4f *>(xr) = v4f{acc01.x, acc01.y, acc23.x, acc23.y};
        else { xr[0] = acc01.x; xr[1] = acc01.y; xr[2] = acc23.x; xr[3] = acc23.y; }
        acc01 = v2f{0.f, 0.f}; acc23 = v2f{0.f, 0.f};
    }
}
template <bool AL16, int GB, int... J>
__device__ __forceinline__ void prog_batch(int words, float my_w, __amdgpu_buffer_rsrc_t rsrc, int voff0, float (&w)[GB], v4f (&x)[GB],
                                           std::integer_sequence<int, J...>)
{
    ((w[J] = row_bcast_f<J>(my_w),
      x[J] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (row_bcast_i<J>(words) & ~0xff) | voff0, 0, 0))), ...);
}
template <bool AL16, int GB, int... J>
__device__ __forceinline__ void prog_consume_all(int words, const float (&w)[GB], const v4f (&x)[GB], v2f &acc01, v2f &acc23, float *xo, int KP,
                                                 std::integer_sequence<int, J...>)
{
    (prog_consume<AL16, J>(words, w[J], x[J], acc01, acc23, xo, KP), ...);
}
typedef int v2i __attribute__((ext_vector_type(2)));
// slot header {first batch, batches, tile id, 0} of the launch's tile schedule (a.gp_slot; gnn_tile_schedule_build): the tile that ticket
// `slot` stands for and the header of its program - the same 16 bytes for every lane, one load.  The partial last tile of the graph is an
// ordinary slot.  A slot at or past gp_slots is "no such tile" (a ticket past the end, the look-ahead of a wave's last tile): zero batches and
// a tile id whose first row is at or past n_rows.
__device__ __forceinline__ v4i prog_header_request(const GnnFusedArgs &a, int slot)
{
    v4i h = {0, 0, a.gp_slots, 0};
    if (slot < a.gp_slots) h = *reinterpret_cast<const GNN_GLOBAL v4i *>(gptr(a.gp_slot) + 4 * (int64_t)slot);
    return h;
}
// ---- the two entry formats of the program (GNN_PROG_ENT8 / GNN_PROG_ENT4; gnn_gather_program_compact) ----
// ENT, a lane's entry of a batch as the loaders hold it: v2i {source word, weight} in the 8-byte format, int - the source word - in the
// 4-byte one, where the weight is the entry's ROW's: all entries of a destination row carry one weight, so the program holds it once per
// tile-local row, and a lane holds the 32 weights of the tile it works on in one register (roww: lane l has row l & 31's, one dword load
// per tile beside the slot header).  From the weight on, both formats run the same instructions: the same DPP broadcast, the same
// v_fma_f32 chain, the same flush at a row end.
template <int PROG> using prog_ent_t = std::conditional_t<PROG == GNN_PROG_ENT4, int, v2i>;
template <class ENT> __device__ __forceinline__ ENT prog_ent_make(int word) { if constexpr (std::is_same_v<ENT, int>) return word; else return v2i{word, 0}; }
__device__ __forceinline__ int prog_word(v2i e) { return e.x; }
__device__ __forceinline__ int prog_word(int e) { return e; }
// the weight of this lane's entry: its second half, or row (word & 31)'s of the tile - one ds_bpermute_b32 per batch (the word of padding
// names row 0: whatever that row weighs, what padding accumulates is never written; an empty row weighs +0, as its entry did)
__device__ __forceinline__ float prog_weight(v2i e, int) { return __int_as_float(e.y); }
__device__ __forceinline__ float prog_weight(int e, int roww) { return __int_as_float(__builtin_amdgcn_ds_bpermute((e & (int)GNN_GP_ROW_MASK) << 2, roww)); }
// this lane's entry of batch b of the program
template <class ENT>
__device__ __forceinline__ ENT prog_entry(const GnnFusedArgs &a, int b, int lane)
{
    if constexpr (std::is_same_v<ENT, int>) return *(gptr(a.gp_ent) + ((int64_t)b * 64 + lane));
    else return *reinterpret_cast<const GNN_GLOBAL v2i *>(gptr(a.gp_ent) + ((int64_t)b * 64 + lane) * 2);
}
// 4-byte format: the row weights of the tile that ticket `slot` stands for, [gp_slots][32] floats in slot order behind the slot headers -
// an address from the ticket alone, so the load goes out with the header's; 0 for a slot at or past gp_slots, and in the 8-byte format
template <class ENT>
__device__ __forceinline__ int prog_roww_request(const GnnFusedArgs &a, int slot, int lane)
{
    int w = 0;
    if constexpr (std::is_same_v<ENT, int>) {
        if (slot < a.gp_slots) w = *(gptr(a.gp_slot) + 4 * (int64_t)a.gp_slots + 32 * (int64_t)slot + (lane & 31));
    }
    return w;
}
// first / nb: the tile's header; ent: this lane's entry of the first batch, requested during the previous tile; roww: the tile's row
// weights (4-byte format)
template <bool AL16, class ENT>
__device__ __forceinline__ void load_tile_prog64(const GnnFusedArgs &a, float *X, int64_t i0, int lane, int KP, int c_aggs, int first, int nb, ENT ent, int roww)
{
    constexpr int GB = 16;
    const int gl = lane & 15;
    TileOwn64<AL16> own;
    own.request(a, i0, lane);
    v2f acc01 = {0.f, 0.f}, acc23 = {0.f, 0.f};
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.state_cur), 0, (int)a.state_bytes, 0x00020000);
    const int voff0 = gl * 16;
    float *xo = X + c_aggs + gl * 4;
    for (int b = 0; b < nb; ++b) {
        float w[GB];
        v4f x[GB];
        const int words = prog_word(ent);
        prog_batch<AL16, GB>(words, prog_weight(ent, roww), rsrc, voff0, w, x, std::make_integer_sequence<int, GB>{});
        if (b + 1 < nb) ent = prog_entry<ENT>(a, first + b + 1, lane);      // (wave-uniform)
        prog_consume_all<AL16, GB>(words, w, x, acc01, acc23, xo, KP, std::make_integer_sequence<int, GB>{});
    }
    own.write(a, X, i0, lane, KP, c_aggs);
}

// ---- the tile's first batch a tile ahead (GNN_FIRST_BATCH_AHEAD) ----
// Every batch is a dependent round trip, and the first of a tile has nothing to hide behind.  Its 16 rows are therefore requested during the
// PREVIOUS tile, behind the last weight loads of the dense layers (vector-memory results return in issue order: in front of them the rows
// would hold up every weight wait), and stay in 64 registers across the epilogue, the condition and the row stores, where the dense layers'
// registers are free.  The entry they are requested from comes with the previous tile's last gather batch (the header of this tile is back
// by then) and is held across the dense layers: two registers.  A tile that does not exist has the entry {GNN_GP_NOROW, 0}: offsets past the
// end of the buffer descriptor, for which the texture unit returns zeros without asking memory for anything - so the requests need no branch,
// and the waits in front of the epilogue's gate words and of the first row count past all sixteen on every path.
#ifndef GNN_FIRST_BATCH_AHEAD
#define GNN_FIRST_BATCH_AHEAD 1
#endif
template <int GB, int... J>
__device__ __forceinline__ void prog_rows_request(int words, __amdgpu_buffer_rsrc_t rsrc, int voff0, v4f (&x)[GB], std::integer_sequence<int, J...>)
{
    ((x[J] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (row_bcast_i<J>(words) & ~0xff) | voff0, 0, 0))), ...);
}
template <bool AL16, int GB, int... J>
__device__ __forceinline__ void prog_consume_first(int words, float my_w, const v4f (&x)[GB], v2f &acc01, v2f &acc23, float *xo, int KP, std::integer_sequence<int, J...>)
{
    (prog_consume<AL16, J>(words, row_bcast_f<J>(my_w), x[J], acc01, acc23, xo, KP), ...);
}
// the entry of batch 1 of the tile with header (first, nb), if it has one, and the rows of its batch 0 from that batch's entry ent0.  The
// conditional request goes FIRST: the compiler counts a wait down from the path with the fewest requests behind what it waits for, so behind
// the rows it would make every wait in front of them (the gate words') reach one request further - to the first row.
template <class ENT>
__device__ __forceinline__ void prog_first_batch_request(const GnnFusedArgs &a, int first, int nb, ENT ent0, int lane, v4f (&x0)[16], ENT &ent1)
{
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.state_cur), 0, (int)a.state_bytes, 0x00020000);
    if (nb > 1) ent1 = prog_entry<ENT>(a, first + 1, lane);                 // (wave-uniform)
    __builtin_amdgcn_sched_barrier(0);
    prog_rows_request<16>(prog_word(ent0), rsrc, (lane & 15) * 16, x0, std::make_integer_sequence<int, 16>{});
}
// The loader that starts by consuming that batch.  ent0 / x0: entry and rows of batch 0; ent: entry of batch 1 (nb > 1).  hdr_next_raw: the
// next tile's slot header, requested at the top of this tile; with the last batch of this tile it is read (first_next, nb_next, tid_next) and the entry of
// the next tile's batch 0 requested (ent_next; {GNN_GP_NOROW, 0} when there is no such tile).  A one-batch tile waits for the header.
// roww: this tile's row weights (4-byte format): the weights of batch 0 are fetched from them here, where the batch is consumed - across
// the previous tile's epilogue the batch is its rows and its source word.
template <bool AL16, class ENT>
__device__ __forceinline__ void load_tile_prog64_ahead(const GnnFusedArgs &a, float *X, int64_t i0, int lane, int KP, int c_aggs, int first, int nb,
                                                       ENT ent0, const v4f (&x0)[16], ENT ent, int roww, v4i hdr_next_raw, int &first_next, int &nb_next,
                                                       int &tid_next, ENT &ent_next)
{
    constexpr int GB = 16;
    const int gl = lane & 15;
    TileOwn64<AL16> own;
    own.request(a, i0, lane);
    v2f acc01 = {0.f, 0.f}, acc23 = {0.f, 0.f};
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.state_cur), 0, (int)a.state_bytes, 0x00020000);
    const int voff0 = gl * 16;
    float *xo = X + c_aggs + gl * 4;
    // (one variable for "the entry requested with this batch" - the next batch's, or behind the last batch the next tile's first: a second
    // one made the compiler copy it inside the loop, behind a wait for the batch's rows)
    auto request_next = [&]() {
        first_next = __builtin_amdgcn_readfirstlane(hdr_next_raw.x); nb_next = __builtin_amdgcn_readfirstlane(hdr_next_raw.y);
        tid_next = __builtin_amdgcn_readfirstlane(hdr_next_raw.z);
        ent = prog_ent_make<ENT>((int)GNN_GP_NOROW);
        if (nb_next > 0) ent = prog_entry<ENT>(a, first_next, lane);        // (wave-uniform)
    };
    if (nb <= 1) request_next();
    prog_consume_first<AL16, GB>(prog_word(ent0), prog_weight(ent0, roww), x0, acc01, acc23, xo, KP, std::make_integer_sequence<int, GB>{});
    for (int b = 1; b < nb; ++b) {
        float w[GB];
        v4f x[GB];
        const int words = prog_word(ent);
        prog_batch<AL16, GB>(words, prog_weight(ent, roww), rsrc, voff0, w, x, std::make_integer_sequence<int, GB>{});
        if (b + 1 < nb) ent = prog_entry<ENT>(a, first + b + 1, lane);      // (wave-uniform)
        else request_next();
        prog_consume_all<AL16, GB>(words, w, x, acc01, acc23, xo, KP, std::make_integer_sequence<int, GB>{});
    }
    ent_next = ent;
    own.write(a, X, i0, lane, KP, c_aggs);
}

// Ds == 64, full tile, aggregate GIVEN (a.agg_in: rows of the aggregated state computed by another kernel): three coalesced row
// copies - own state, aggregate, label columns - instead of the gather.
template <bool AL16>
__device__ __forceinline__ void load_tile_given64(const GnnFusedArgs &a, float *X, int64_t i0, int lane, int KP, int c_aggs)
{
    constexpr int Ds = 64;
    v4f own[8], agg[8];
    {
        const float *src = a.state_cur + (a.row_begin + i0) * Ds + lane * 4;
        const float *sag = a.agg_in + i0 * Ds + lane * 4;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            own[u] = gload4(src + u * 256);
            agg[u] = gload4(sag + u * 256);
        }
    }
    float lab[4];
    const int IW = a.IW, nlab = 32 * IW;
    {
        const float *src = a.inv + i0 * IW;
#pragma unroll
        for (int u = 0; u < 4; ++u) lab[u] = (lane + 64 * u < nlab) ? gload1(src + lane + 64 * u) : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float *x = X + (4 * u + (lane >> 4)) * KP + (lane & 15) * 4;         // flat element 256 u + 4 lane = row 4u + lane/16
        if constexpr (AL16) { *reinterpret_cast<v4f *>(x) = own[u]; *reinterpret_cast<v4f *>(x + c_aggs) = agg[u]; }
        else {
            x[0] = own[u].x; x[1] = own[u].y; x[2] = own[u].z; x[3] = own[u].w;
            x[c_aggs] = agg[u].x; x[c_aggs + 1] = agg[u].y; x[c_aggs + 2] = agg[u].z; x[c_aggs + 3] = agg[u].w;
        }
    }
    const float inv_iw = 1.0f / (float)(IW > 0 ? IW : 1);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = lane + 64 * u;
        if (t < nlab) {
            const int i = (int)(((float)t + 0.5f) * inv_iw), c = t - i * IW;
            X[i * KP + label_col(c, Ds, a.NLc, c_aggs)] = lab[u];
        }
    }
    if (nlab > 256)
        for (int t = 256 + lane; t < nlab; t += 64) {
            const int i = t / IW, c = t - i * IW;
            X[i * KP + label_col(c, Ds, a.NLc, c_aggs)] = gload1(a.inv + i0 * IW + t);
        }
}

// condition() for the next body + coalesced store of the new rows.  New state sits in columns [c_aggs, c_aggs + Ds).
// lanes 0..31 sum (new - old)^2, lanes 32..63 sum old^2, ascending feature order, unfused (oracle order).
// moved_out != nullptr: the verdict "some node of the tile still moves" is returned there instead of raised in a.flag_out
// STORE == false: the condition only (k_small_loop stores the rows itself, into its padded exchange buffer)
template <bool COH = false, bool STORE = true>
__device__ __forceinline__ void check_store_generic(const GnnFusedArgs &a, float *X, int64_t i0, int lane, int nvalid, int KP,
                                                 int c_aggs, int *moved_out = nullptr)
{
    const int Ds = a.Ds, half = lane >> 5;
    if constexpr (STORE) {   // the row stores first: they drain while the condition is evaluated
        float *dst = a.state_nxt + i0 * Ds;
        const int total = nvalid * Ds;
        RowCol rc(lane, Ds);
        for (int t = lane; t < total; t += 64, rc.next()) sstore1<COH>(dst + t, X[rc.i * KP + c_aggs + rc.c]);
    }
    const float *xo = X + (lane & 31) * KP, *xn = xo + c_aggs;
    float s_ = 0.0f;
    for (int f = 0; f < Ds; ++f) {
        const float o = xo[f];
        const float d = half ? o : (xn[f] - o);
        const float dd = d * d;
        s_ = s_ + dd;
    }
    const float root = sqrtf(s_);
    const float nrm = shfl_f(root, (lane & 31) + 32);
    const float rhs = a.thr * nrm;
    const bool voter = (half == 0) && ((lane & 31) < nvalid);
    const int moved = voter && (root > rhs);
    if (moved_out) *moved_out = __any(moved) ? 1 : 0;
    else if (a.certify) {      // split arithmetic: certified gate
        const float band = GNN_BAND_ABS * nrm + GNN_BAND_REL * rhs;
        const int robust = voter && (root > rhs + band), border = voter && gnn_gate_borderline(root, rhs, band);
        const bool am = __any(moved), ar = __any(robust), ab = __any(border);
        if (lane == 0) gnn_flag_raise_certified(a.flag_out, am, ar, ab);
    }
    else if (__any(moved) && lane == 0) gnn_flag_raise(a.flag_out);
}

__device__ __forceinline__ void check_store_fast64(const GnnFusedArgs &a, float *X, int64_t i0, int lane, int KP, int c_aggs)
{
    constexpr int Ds = 64;
    const int half = lane >> 5;
    const float *xo = X + (lane & 31) * KP, *xn = xo + c_aggs;
    float s_ = 0.0f;
#pragma unroll
    for (int f = 0; f < Ds; f += 16) {
        float o[16], nw[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { o[u] = xo[f + u]; nw[u] = xn[f + u]; }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float d = half ? o[u] : (nw[u] - o[u]);
            const float dd = d * d;
            s_ = s_ + dd;
        }
    }
    const float root = sqrtf(s_);
    const float nrm = shfl_f(root, (lane & 31) + 32);
    const float rhs = a.thr * nrm;
    const int moved = (half == 0) && (root > rhs);
    if (__any(moved) && lane == 0) gnn_flag_raise(a.flag_out);
    float *dst = a.state_nxt + i0 * Ds + lane;
    const float *xs = X + c_aggs + lane;                                     // row i, feature lane
#pragma unroll
    for (int i = 0; i < 32; i += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = xs[(i + u) * KP];
#pragma unroll
        for (int u = 0; u < 8; ++u) gstore_row1(dst + (i + u) * Ds, v[u]);
    }
}

// Split arithmetic, Ds == 64, full tile: last-layer epilogue output (already activated / normalised, in registers: lane = (node,
// half), 4 consecutive features per register quad) -> condition() for the next body and coalesced row stores.  Each lane sums
// its 32 features of (new - old)^2 and old^2 (old state: aligned 16-byte reads of the tile), the two halves of a node are added
// across lanes l / l + 32.  The summation order differs from the oracle's ascending-feature chain; on this path the state
// itself already differs from the oracle in the last bits, so that is within the same tolerance (k is compared in the tests).
// peek: the gate words of this wave's slot, requested by lane 0 behind the last weight loads (gnn_flag_peek)
// LATE: the words are first looked at HERE.  Without it the compiler compares them with zero in the block that requests them (the other
// lanes' constant zeros invite it to) and waits for them there, in front of the epilogue instead of behind it.
template <bool LATE = false>
__device__ __forceinline__ void finish_fast64_aligned(const GnnFusedArgs &a, float *X, f32x16 (&out)[2], int64_t i0, int lane, int KP, int c_aggs,
                                                      GnnFlagPeek peek)
{
    const int half = lane >> 5;
    float *xrow = X + (lane & 31) * KP;
    float d2 = 0.0f, o2 = 0.0f;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f0 = 32 * jt + 8 * q + 4 * half;
            const v4f o = *reinterpret_cast<const v4f *>(xrow + f0);
            const v4f nw = {out[jt][4 * q], out[jt][4 * q + 1], out[jt][4 * q + 2], out[jt][4 * q + 3]};
            *reinterpret_cast<v4f *>(xrow + c_aggs + f0) = nw;
            const v4f d = nw - o;
            d2 = __builtin_fmaf(d.x, d.x, d2); d2 = __builtin_fmaf(d.y, d.y, d2); d2 = __builtin_fmaf(d.z, d.z, d2); d2 = __builtin_fmaf(d.w, d.w, d2);
            o2 = __builtin_fmaf(o.x, o.x, o2); o2 = __builtin_fmaf(o.y, o.y, o2); o2 = __builtin_fmaf(o.z, o.z, o2); o2 = __builtin_fmaf(o.w, o.w, o2);
        }
    d2 = d2 + shfl_f(d2, lane ^ 32);
    o2 = o2 + shfl_f(o2, lane ^ 32);
    const float root = sqrtf(d2), nrm = sqrtf(o2);
    {   // certified gate (gnn_common.h): both half-lanes of a node hold the same sums
        const float rhs = a.thr * nrm, band = GNN_BAND_ABS * nrm + GNN_BAND_REL * rhs;
        const bool am = __any(root > rhs), ar = __any(root > rhs + band), ab = __any(gnn_gate_borderline(root, rhs, band));
        if constexpr (LATE) asm volatile("" : "+v"(peek.c0), "+v"(peek.c1), "+v"(peek.c2));
        if (lane == 0) gnn_flag_raise_peeked(a.flag_out, peek, am, ar, ab);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int64_t dst = i0 * 64 + lane * 4;                                  // flat element 256 u + 4 lane = row 4u + lane/16
    const float *xs = X + (lane >> 4) * KP + c_aggs + (lane & 15) * 4;
    v4f v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const v4f *>(xs + 4 * u * KP);
#pragma unroll
    for (int u = 0; u < 8; ++u) gstore_row4(a.state_nxt, dst + 256 * u, v[u]);
}

// The same two for the LAST tile of a range whose row count is not a multiple of 32 (wave-uniform branch in the full-tile kernel: a
// second, one-tile launch of the general kernel for that tile cost 70 - 100 us per iteration).  Rows >= nvalid of the tile exist
// in memory (the buffers are padded to whole tiles) and have no arcs; what they compute stays in LDS: their lanes do not vote in
// condition() and their rows are not stored.
__device__ __forceinline__ void check_store_fast64_partial(const GnnFusedArgs &a, float *X, int64_t i0, int lane, int KP, int c_aggs, int nvalid)
{
    constexpr int Ds = 64;
    const int half = lane >> 5;
    const float *xo = X + (lane & 31) * KP, *xn = xo + c_aggs;
    float s_ = 0.0f;
#pragma unroll
    for (int f = 0; f < Ds; f += 16) {
        float o[16], nw[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { o[u] = xo[f + u]; nw[u] = xn[f + u]; }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float d = half ? o[u] : (nw[u] - o[u]);
            const float dd = d * d;
            s_ = s_ + dd;
        }
    }
    const float root = sqrtf(s_);
    const float nrm = shfl_f(root, (lane & 31) + 32);
    const float rhs = a.thr * nrm;
    const int moved = (half == 0) && (lane < nvalid) && (root > rhs);
    if (__any(moved) && lane == 0) gnn_flag_raise(a.flag_out);
    float *dst = a.state_nxt + i0 * Ds + lane;
    const float *xs = X + c_aggs + lane;                                     // row i, feature lane
    for (int i = 0; i < nvalid; ++i) gptr_w(dst)[i * Ds] = xs[i * KP];
}

__device__ __forceinline__ void finish_fast64_partial(const GnnFusedArgs &a, float *X, f32x16 (&out)[2], int64_t i0, int lane, int KP, int c_aggs,
                                                      int nvalid)
{
    const int half = lane >> 5;
    float *xrow = X + (lane & 31) * KP;
    float d2 = 0.0f, o2 = 0.0f;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f0 = 32 * jt + 8 * q + 4 * half;
            const v4f o = *reinterpret_cast<const v4f *>(xrow + f0);
            const v4f nw = {out[jt][4 * q], out[jt][4 * q + 1], out[jt][4 * q + 2], out[jt][4 * q + 3]};
            *reinterpret_cast<v4f *>(xrow + c_aggs + f0) = nw;
            const v4f d = nw - o;
            d2 = __builtin_fmaf(d.x, d.x, d2); d2 = __builtin_fmaf(d.y, d.y, d2); d2 = __builtin_fmaf(d.z, d.z, d2); d2 = __builtin_fmaf(d.w, d.w, d2);
            o2 = __builtin_fmaf(o.x, o.x, o2); o2 = __builtin_fmaf(o.y, o.y, o2); o2 = __builtin_fmaf(o.z, o.z, o2); o2 = __builtin_fmaf(o.w, o.w, o2);
        }
    d2 = d2 + shfl_f(d2, lane ^ 32);
    o2 = o2 + shfl_f(o2, lane ^ 32);
    const float root = sqrtf(d2), nrm = sqrtf(o2);
    {   // certified gate (gnn_common.h); rows past the end of the range do not vote
        const bool voter = (lane & 31) < nvalid;
        const float rhs = a.thr * nrm, band = GNN_BAND_ABS * nrm + GNN_BAND_REL * rhs;
        const bool am = __any(voter && root > rhs), ar = __any(voter && root > rhs + band), ab = __any(voter && gnn_gate_borderline(root, rhs, band));
        if (lane == 0) gnn_flag_raise_certified(a.flag_out, am, ar, ab);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    float *dst = a.state_nxt + i0 * 64 + lane * 4;                           // flat element 256 u + 4 lane = row 4u + lane/16
    const float *xs = X + (lane >> 4) * KP + c_aggs + (lane & 15) * 4;
    for (int u = 0; u < 8; ++u)
        if (4 * u + (lane >> 4) < nvalid) *reinterpret_cast<GNN_GLOBAL v4f *>(gptr_w(dst) + 256 * u) = *reinterpret_cast<const v4f *>(xs + 4 * u * KP);
}

// ---- cross-tile prefetch of the dependent loads that open a tile: ticket -> row pointers -> ids of the first gather batch ----
// Each of them is a full memory round trip in front of the first neighbour row; requested one tile ahead they cost three VGPRs.
__device__ __forceinline__ int tile_rowptr_request(const GnnFusedArgs &a, int tile, int lane)
{
    const int64_t i0 = (int64_t)tile * 32;
    if (i0 >= a.n_rows) return 0;
    const int nvalid = (int)((a.n_rows - i0) < 32 ? (a.n_rows - i0) : 32);
    return (lane <= nvalid) ? gstream1(a.indptr + i0 + lane) : 0;
}
// rows past the end of a partial tile get the last pointer (empty rows); lanes 33.. hold it too
__device__ __forceinline__ int tile_rowptr_clamp(const GnnFusedArgs &a, int tile, int lane, int raw)
{
    const int64_t i0 = (int64_t)tile * 32;
    if (i0 >= a.n_rows) return 0;
    const int nvalid = (int)((a.n_rows - i0) < 32 ? (a.n_rows - i0) : 32);
    const int last_ip = shfl_i(raw, nvalid);
    return lane <= nvalid ? raw : last_ip;
}
// lane group g = lane >> 4 owns rows 8g .. 8g+7: ids / weights of its first 16 entries (Ds == 64 gather)
__device__ __forceinline__ void tile_first_ids(const GnnFusedArgs &a, int ip, int lane, int &src, float &w)
{
    const int gl = lane & 15, grp = lane >> 4;
    const int e_begin = shfl_i(ip, grp * 8), e_end = shfl_i(ip, grp * 8 + 8);
    src = 0; w = 0.0f;
    if (e_begin + gl < e_end) { src = gstream1(a.adj_src + e_begin + gl); w = gstream1(a.adj_w + e_begin + gl); }
}

template <int N>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[N])
{
#pragma unroll
    for (int jt = 0; jt < N; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[jt][r] = 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------------
// The fused body is two kernels: k_fused_full (state width 64: program or CSR gather, 16-byte tile accesses, the first batch a tile ahead)
// and k_fused_generic (every other width).  The phases below are the same in both; they are forced inline, so each kernel's instruction
// stream is the one of the phases written out in place.
// ---------------------------------------------------------------------------------------------------------------------

// diagnostics only (GNN_FUSED_STAMPS): s_memtime of lane 0 into slot `slot` of the tile's stamps; `stamp` and `lane` are the caller's
#ifndef GNN_DIAG
#define GNN_STAMP(slot) do { } while (0)
#else
#define GNN_STAMP(slot)                                                                      \
    do {                                                                                     \
        if (stamp) {                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                               \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();                      \
            if (lane == 0) stamp[slot] = t_;                                                 \
            __builtin_amdgcn_sched_barrier(0);                                               \
        }                                                                                    \
    } while (0)
#endif

// GNN_POISON=1 (diagnostic build): NaN over the whole LDS allocation (tiles, alignment holes, look-ahead slack, staged vectors) before anything is staged
__device__ __forceinline__ void fused_poison_lds([[maybe_unused]] const GnnFusedArgs &a, [[maybe_unused]] float *lds)
{
#ifdef GNN_DIAG
    if (a.lds_floats) {
        for (int t = threadIdx.x; t < a.lds_floats; t += blockDim.x) lds[t] = __builtin_nanf("");
        __syncthreads();
    }
#endif
}

// last-layer bias and BatchNormalization scale / shift (ep, behind the row-pointer slots) and the hidden layers' biases (hb, split path:
// [LAYERS - 1][32 NT]): staged once per workgroup
template <int LAYERS, int NT, int NTL, int ACT, bool SPLIT>
__device__ __forceinline__ void fused_stage_vectors(const GnnFusedArgs &a, float *ep, float *hb)
{
    for (int t = threadIdx.x; t < 3 * 32 * NTL; t += blockDim.x) {
        const int which = t / (32 * NTL), f = t - which * 32 * NTL;
        ep[t] = which == 0 ? a.bias[LAYERS - 1][f] * (SPLIT ? a.bsc[LAYERS - 1] : 1.0f) : (a.bn_scale ? (which == 1 ? a.bn_scale[f] : a.bn_shift[f]) : 0.0f);
    }
    if constexpr (SPLIT && LAYERS > 1)                // (x 2^(e_w + e_x) of the layer in the fp16-piece format: bsc)
        for (int t = threadIdx.x; t < (LAYERS - 1) * 32 * NT; t += blockDim.x)
            hb[t] = a.bias[t / (32 * NT)][t % (32 * NT)] * (ACT == GNN_ACT_SELU ? 1.44269504088896341f : 1.0f) * a.bsc[t / (32 * NT)];   // folded SELU: see GNN_S1_E
    __syncthreads();
}

// Start-up spread.  All waves of the chip run the same phases on tiles of similar cost: started together they gather together
// (HBM saturated, 3-4 us per round trip) and compute together (HBM idle).  Every wave therefore waits a different fraction of
// one tile period before its first tile; the dynamic tickets keep the load balanced.  variant bit 2: the old two-cluster
// stagger (waves 4-7 delayed by a fixed amount).  waves: waves per workgroup of the launch (k_fused_generic passes its own).
__device__ __forceinline__ void fused_startup_spread(const GnnFusedArgs &a, int wave, int waves = GNN_FUSED_WAVES)
{
    if (a.stagger > 0) {
        int rounds = 0;
        if (a.variant & 4) rounds = wave >= waves / 2 ? a.stagger : 0;
        else rounds = (int)((((unsigned)blockIdx.x * (unsigned)waves + (unsigned)wave) * 0x9E3779B1u) >> 16) % (unsigned)(a.stagger + 1);
        for (int i = 0; i < rounds; ++i) __builtin_amdgcn_s_sleep(127);
    }
}

// Fresh, compiler-opaque copies of the pointers for every tile (a: the tile's own copy of the arguments): without this the loop-invariant
// address arithmetic of the unrolled layers is hoisted out of the tile loop and spills (256 VGPRs + scratch instead of ~190).
__device__ __forceinline__ void fused_opaque_pointers(GnnFusedArgs &a)
{
    asm volatile("" : "+s"(a.Wp[0]), "+s"(a.Wp[1]), "+s"(a.Wp[2]), "+s"(a.bias[0]), "+s"(a.bias[1]), "+s"(a.bias[2]));
    asm volatile("" : "+s"(a.bn_scale), "+s"(a.bn_shift), "+s"(a.state_cur), "+s"(a.state_nxt), "+s"(a.inv), "+s"(a.adj_src), "+s"(a.adj_w));
}

// Label projection (gnn_loop_set_label_projection): the seed of the tile's layer-0 accumulators, P[node, feature] of GnnFusedArgs::seed - four
// 1 KiB wave loads per feature tile straight into the accumulator registers, which are dead until layer 0 starts - times sc, the scale of
// the accumulator: bsc[0] of the piece format, and log2(e) where the layer's output feeds the folded SELU (as gnn_fused_pack folds its weights and
// fused_stage_vectors its bias).  Called behind the tile's gather and in front of layer 0's first weight request: vector-memory results
// return in issue order, so in front of the gather these loads would sit in every wait of it.
// Through a buffer descriptor of the tile's block (scalar registers) with the weight loads' vector offset 16 * lane: no vector register
// beyond the accumulators.  SCALE false (format 3 in front of anything but the folded SELU: sc == 1): no multiplication.
template <int NO, bool SCALE>
__device__ __forceinline__ void seed_tiles(const GnnFusedArgs &a, int64_t i0, int lane, float sc, f32x16 (&acc)[NO])
{
    const float *sp = a.seed;
    asm volatile("" : "+s"(sp));                      // (per tile, as fused_opaque_pointers)
    const int tile_bytes = a.seed_nt * 4096;
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(sp + (size_t)(i0 >> 5) * (size_t)(a.seed_nt * 1024)), 0,
                                                                         tile_bytes, 0x00020000);
    const int sv = lane * 16;
#pragma unroll
    for (int jt = 0; jt < NO; ++jt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const v4f s = __builtin_bit_cast(v4f, bload4i(srs, sv, (jt * 4 + q) * 1024));
            acc[jt][4 * q] = s.x; acc[jt][4 * q + 1] = s.y; acc[jt][4 * q + 2] = s.z; acc[jt][4 * q + 3] = s.w;
        }
    if constexpr (SCALE) {
#pragma unroll
        for (int jt = 0; jt < NO; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[jt][r] *= sc;
    }
}

// ---- B: net_state.  H^T[feature][node] = W^T . X^T on MFMA f32 32x32x2 (exact) or on the piece products (SPLIT, format PC) ----
// Declares half, out (the last layer's raw accumulators) and mx in the kernel's tile loop; a, X, KP, lane, i0, ep, hb and stamp are the kernel's.
// SEED (the kernel's template parameter; split arithmetic only): layer 0 starts from the tile's label projection (seed_tiles), not from its bias.
// AL16: layer 0 of a net with hidden layers reads the tile in 16-byte pieces (the full-tile kernel's tile layout).
// WAIT: 12 wait states behind layer 0 of the split arithmetic.  Its chunk loop ends in a branch, what follows reads its accumulators, and
// hipcc (ROCm 7.2) pads nothing across a basic-block edge (persistent small-graph loop): k_fused_generic, where a one-tile layer
// leaves 11 instructions between the two.  k_fused_full's listings pass the Makefile's scan (tools/scan_mfma_hazard.py) without.
// A macro, not a function like the other phases: as a forced-inline function the same text gave every full-tile instantiation another
// register allocation (16 of 648 with one vector register more or less, code sizes - 1.3 .. + 0.5 KB; profiles/fused_two_kernels.txt).
#define GNN_FUSED_DENSE_LAYERS(AL16, WAIT) \
    const int half = lane >> 5;                                                                                                                                 \
    const float *xb = X + (lane & 31) * KP + half;                                                                                                              \
    f32x16 out[NTL];                                                                                                                                            \
    float mx = 0.0f;                                  /* range guard of the fp16-piece format: max |scaled operand| of this tile's cuts */                      \
    if constexpr (SPLIT) {                                                                                                                                      \
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int *>(a.Ws_base), 0, a.ws_bytes, 0x00020000);                          \
        const int wv = lane * 16;                                                                                                                               \
        const float *xr = X + (lane & 31) * KP + 8 * half;                                                                                                      \
        if constexpr (LAYERS == 1) {                                                                                                                            \
            if constexpr (SEED) seed_tiles<NTL, PC == 2>(a, i0, lane, a.bsc[0], out);                                                                           \
            layer0_split<NTL, false, PC, SEED>(xr, wrs, wv, a.ws_off[0], a.chunks0, out, ep, half, mx);                                                         \
        } else {                                                                                                                                                \
            f32x16 h1[NT];                                                                                                                                      \
            if constexpr (SEED) seed_tiles<NT, PC == 2 || ACT == GNN_ACT_SELU>(a, i0, lane, a.bsc[0] * (ACT == GNN_ACT_SELU ? 1.44269504088896341f : 1.0f), h1); \
            layer0_split<NT, AL16, PC, SEED>(xr, wrs, wv, a.ws_off[0], a.chunks0, h1, hb, half, mx);                                                            \
            if constexpr (WAIT) { asm volatile("s_nop 7\n\ts_nop 3" ::: "memory"); __builtin_amdgcn_sched_barrier(0); }                                         \
            GNN_STAMP(3);                                                                                                                                       \
            GNN_STAMP(4);                                                                                                                                       \
            if constexpr (PC == 2) { asm volatile("" : "+v"(mx)); mx = __builtin_fmaxf(mx, hidden_range<NT>(h1, a.usc[0])); asm volatile("" : "+v"(mx)); }      \
            if constexpr (LAYERS == 2) {                                                                                                                        \
                layer_split_from_regs<NT, NTL, ACT, PC>(h1, ep, half, out, wrs, wv, a.ws_off[1], a.usc[0], mx);                                                 \
            } else {                                                                                                                                            \
                f32x16 h2[NT];                                                                                                                                  \
                layer_split_from_regs<NT, NT, ACT, PC>(h1, hb + 32 * NT, half, h2, wrs, wv, a.ws_off[1], a.usc[0], mx);                                         \
                if constexpr (PC == 2) { asm volatile("" : "+v"(mx)); mx = __builtin_fmaxf(mx, hidden_range<NT>(h2, a.usc[1])); asm volatile("" : "+v"(mx)); }  \
                layer_split_from_regs<NT, NTL, ACT, PC>(h2, ep, half, out, wrs, wv, a.ws_off[2], a.usc[1], mx);                                                 \
            }                                                                                                                                                   \
        }                                                                                                                                                       \
    } else if constexpr (LAYERS == 1) {                                                                                                                         \
        zero_acc<NTL>(out);                                                                                                                                     \
        layer_from_lds<NTL>(xb, a.Wp[0] + (size_t)lane * NTL, a.kk0, out, a.wstride);                                                                           \
    } else {                                                                                                                                                    \
        f32x16 h1[NT];                                                                                                                                          \
        zero_acc<NT>(h1);                                                                                                                                       \
        layer_from_lds<NT>(xb, a.Wp[0] + (size_t)lane * NT, a.kk0, h1, a.wstride);                                                                              \
        GNN_STAMP(3);                                                                                                                                           \
        GNN_STAMP(4);                                                                                                                                           \
        if constexpr (LAYERS == 2) {                                                                                                                            \
            zero_acc<NTL>(out);                                                                                                                                 \
            layer_from_regs<NT, NTL, ACT>(h1, a.bias[0], half, out, a.Wp[1] + (size_t)lane * NTL, a.wstride);                                                   \
        } else {                                                                                                                                                \
            f32x16 h2[NT];                                                                                                                                      \
            zero_acc<NT>(h2);                                                                                                                                   \
            layer_from_regs<NT, NT, ACT>(h1, a.bias[0], half, h2, a.Wp[1] + (size_t)lane * NT, a.wstride);                                                      \
            zero_acc<NTL>(out);                                                                                                                                 \
            layer_from_regs<NT, NTL, ACT>(h2, a.bias[1], half, out, a.Wp[2] + (size_t)lane * NTL, a.wstride);                                                   \
        }                                                                                                                                                       \
    }

// Tiles: the first TWO rounds are assigned statically - wave w of the launch (wave-major over the workgroups, so that a partial round
// spreads over all CUs) takes tiles w and w + W, W = waves of the launch - and only from the third round on does a wave draw tickets
// from the iteration's counter, one tile ahead (at the end of the previous tile's dense layers), early enough to have that tile's row
// pointers and first gather ids requested.  (Until round 4 every wave drew its first two tickets at kernel start: 4,096 atomic adds on
// ONE word, which the memory side serves at about 88 per microsecond - up to 46 us before the last wave knew its first tile, a third
// of an iteration at 125 k nodes.  Serving the tickets heaviest-tile-first was measured in round 2: 1 % slower on the BASELINE graph.)
// third_round (wave-uniform): tiles beyond 2 W exist - no draw without them, two static tiles per wave cover the launch.
// fused_draw_ticket: lane 0's ticket for the tile after next (0x3fffffff: none); fused_next_tile: the wave's first look at it, at the end
// of the tile.
// AHEAD (a tile's first batch is requested during the previous tile): the counter's address through a vector register.  An atomic at a
// wave-uniform address inside divergent code is rewritten by the compiler into "one lane adds, v_readfirstlane hands the result round" -
// and that read waits for the ticket on the spot, with the rows requested behind it queued behind the wait.  The only read of the ticket is
// fused_next_tile's, which also adds the 2 W.
template <bool AHEAD>
__device__ __forceinline__ int fused_draw_ticket(const GnnFusedArgs &a0, bool third_round, int W_launch, int lane)
{
    int next2_tile = 0x3fffffff;
    if (third_round) {
        int64_t ctr_off = 0;
        if constexpr (AHEAD) asm volatile("" : "+v"(ctr_off));
        if constexpr (AHEAD) { if (lane == 0) next2_tile = atomicAdd(a0.tile_ctr + ctr_off, 1); }      // (+ 2 W where it is read)
        else if (lane == 0) next2_tile = atomicAdd(a0.tile_ctr, 1) + 2 * W_launch;
    }
    return next2_tile;
}
template <bool AHEAD>
__device__ __forceinline__ int fused_next_tile(const GnnFusedArgs &a0, int next2_tile, bool third_round, int W_launch)
{
    if constexpr (AHEAD) {
        asm volatile("" : "+v"(next2_tile));                    // first look at the ticket: here
        return __builtin_amdgcn_readfirstlane(next2_tile) + (third_round ? 2 * W_launch : 0) + a0.tile_base;
    } else return __builtin_amdgcn_readfirstlane(next2_tile) + a0.tile_base;
}

// The fused body for every state width but 64.  Persistent workgroup of 8 waves (one per CU): every wave pulls 32-node tiles from a
// device-wide counter until none is left; the waves never synchronise with each other after the staging.  The tile load is
// load_tile_generic (any width, partial tiles, a given aggregate a.agg_in), the epilogue writes the new state to the tile and
// check_store_generic tests and stores it.
// Wide-state form (gnn_loop_set_wide_state): the same kernel on a workgroup of 4 to 7 waves, as many as a wider tile leaves room for
// in LDS - every LDS offset and the ticket arithmetic follow blockDim - with load_tile_wide on the full tiles.
// PC: piece format of the split arithmetic (3 = bf16 x 3, 2 = fp16 x 2; gnn_loop_set_pieces)
// ACTL: the last layer's activation (tile_epilogue_last); used in section C only.
// SEED: the seeded form of the label projection (GNN_FUSED_DENSE_LAYERS; the arguments describe the net over [state | aggregated state]).
template <int LAYERS, int NT, int NTL, int ACT, bool SPLIT, int PC, int ACTL, bool SEED = false>
__global__ void __launch_bounds__(GNN_FUSED_THREADS, 2) k_fused_generic(const GnnFusedArgs a0)
{
    static_assert(!SEED || SPLIT, "the label projection is a form of the split arithmetic");
    const GnnFusedArgs &a = a0;      // (shadowed inside the tile loop)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (!gnn_gate_open(a.gate, a.world)) return;
    fused_poison_lds(a, lds);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KP = a.KP, Ds = a.Ds;
    float *X = lds + (size_t)wave * 32 * KP;
    const int c_aggs = a.c_aggs;                      // column of the aggregated state block (Ds + NLc + alignment hole)
    const int waves = (int)(blockDim.x >> 6);         // waves of THIS launch's workgroup: 8, or 4 .. 7 in the wide-state form (gnn_loop_set_wide_state)
    const int W_launch = (int)gridDim.x * waves;      // (tiles and tickets: fused_draw_ticket)
    const int w_launch = wave * (int)gridDim.x + (int)blockIdx.x;
    const bool third_round = (int64_t)2 * W_launch * 32 < a.n_rows;
    int tile = w_launch + a.tile_base, next_tile = w_launch + W_launch + a.tile_base;
    const int ip_first_raw = tile_rowptr_request(a, tile, lane);      // on its way while the workgroup stages its vectors below
    float *ep = lds + (size_t)waves * 32 * KP + 32 + waves * 36;
    float *hb = ep + 3 * 32 * NTL;
    fused_stage_vectors<LAYERS, NT, NTL, ACT, SPLIT>(a, ep, hb);
    fused_startup_spread(a, wave, waves);
    int ip_cur = tile_rowptr_clamp(a, tile, lane, ip_first_raw);
  for (;;) {
    const int64_t i0 = (int64_t)tile * 32;
    if (i0 >= a.n_rows) break;                        // wave-uniform; no workgroup barrier anywhere in the tile loop
    const int nvalid = (int)((a0.n_rows - i0) < 32 ? (a0.n_rows - i0) : 32);
    GnnFusedArgs a = a0;
    if constexpr (SEED) { a.IW = 0; a.NLc = 0; a.AL = 0; }      // (the shadow net has no label columns: as constants, so that the tile loaders' label paths fold away)
    fused_opaque_pointers(a);
#ifdef GNN_DIAG
    unsigned long long *stamp = a.stamps ? a.stamps + ((size_t)tile << 3) : nullptr;
#endif
    GNN_STAMP(0);

    // the tile's 33 row pointers go through LDS: the gather re-reads them inside divergent code, where a cross-lane
    // broadcast from lanes of another group would not be safe
    int *ipt = reinterpret_cast<int *>(lds + (size_t)waves * 32 * KP + 32) + wave * 36;
    if (lane <= 32) ipt[lane] = ip_cur;               // requested during the previous tile
    const int ip_next_raw = tile_rowptr_request(a, next_tile, lane);      // row pointers of the NEXT tile: on their way during the gather
    // the gather is a chain of few instructions and long memory waits: with a raised priority its loads are issued ahead of the
    // SIMD partner's dense VALU / MFMA stream instead of behind it
    if (a.variant & 1) __builtin_amdgcn_s_setprio(3);
    // NTL == 4 is a state wider than 64: only those instantiations hold the wide-row loader, and only a launch of the wide-state form
    // (variant bit 3, wave-uniform; Ds % 4 == 0, no given aggregate) takes it - for its full tiles
    if constexpr (NTL == 4) {
        if ((a.variant & 8) && nvalid == 32) load_tile_wide(a, X, ipt, i0, lane, KP, c_aggs);
        else load_tile_generic(a, X, ipt, i0, lane, nvalid, KP, c_aggs);
    } else load_tile_generic(a, X, ipt, i0, lane, nvalid, KP, c_aggs);
    if (a.variant & 1) __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    GNN_STAMP(2);

    GNN_FUSED_DENSE_LAYERS(false, true)
    // The epilogue reads the last MFMA's result a few instructions on, across the basic-block edges of the ticket draw, and hipcc (ROCm 7.2)
    // pads no wait states across an edge (persistent small-graph loop; small16_layer): the 19 that the 16-pass
    // v_mfma_f32_32x32x2_f32 needs are issued here.  The Makefile's scan of every listing (tools/scan_mfma_hazard.py) is the guard.
    asm volatile("s_nop 15\n\ts_nop 2" ::: "memory");
    // ---- C: last-layer epilogue, new state to LDS (over the aggregated-state columns, no longer needed) ---------------
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    GNN_STAMP(5);
    // Requests for the tile after next (ticket) and for the next tile (its row pointers): issued HERE, behind the last weight loads,
    // because vector-memory results return in issue order - in front of the dense layers these HBM-latency loads would hold up every
    // weight wait - and the epilogue / norm / stores below cover their latency.
    const int next2_tile = fused_draw_ticket<false>(a0, third_round, W_launch, lane);
    const int ip_next = tile_rowptr_clamp(a, next_tile, lane, ip_next_raw);
    if constexpr (SPLIT && PC == 2) gnn_flag_raise_range(a.flag_out, mx);
#pragma unroll
    for (int jt = 0; jt < NTL; ++jt) {
        const float us = SPLIT ? a.usc[LAYERS - 1] : 1.0f;
        if (a.bn_scale) tile_epilogue_last<ACTL, true, SPLIT, true, SPLIT>(a.act_last, out[jt], ep, ep + 32 * NTL, ep + 64 * NTL, jt, half, 1 << 30, us);
        else tile_epilogue_last<ACTL, false, SPLIT, true, SPLIT>(a.act_last, out[jt], ep, nullptr, nullptr, jt, half, 1 << 30, us);
        float *x = X + (lane & 31) * KP + c_aggs;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = 32 * jt + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (f < Ds) x[f] = out[jt][r];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    GNN_STAMP(6);
    check_store_generic(a, X, i0, lane, nvalid, KP, c_aggs);
    GNN_STAMP(7);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the next tile re-uses this wave's LDS region
    tile = next_tile;
    next_tile = fused_next_tile<false>(a0, next2_tile, third_round, W_launch);
    ip_cur = ip_next;
  }
}

// The fused body for state width 64 (two feature tiles in the last layer): the tuned 32-node tile paths only - 16-byte accesses to a tile
// whose padding is zeroed once per wave, unguarded row copies; a partial last tile takes their masked branch.  None of the guarded paths
// of k_fused_generic is compiled in, which frees registers and scalar registers for the tuned ones.
// GIVEN: the aggregated states come from a.agg_in (feature-sliced exchange) - row copies instead of the gather.  A template parameter,
// not a branch: a wave-uniform branch in the tile loop of this kernel cost 3 % (0.700 -> 0.721 ms).
// PC: piece format of the split arithmetic (3 = bf16 x 3, 2 = fp16 x 2; gnn_loop_set_pieces)
// PROG (not GIVEN; GNN_PROG_NONE: the CSR walk): every tile is gathered from the graph's gather program (load_tile_prog64; gnn_loop_set_gather_form), the partial
// last tile of the graph too (an ordinary slot of the tile schedule, prog_header_request): no CSR walk is compiled in.  A template parameter for the same reason as
// GIVEN.  With GNN_FIRST_BATCH_AHEAD a tile's first batch is requested during the previous tile (load_tile_prog64_ahead).
// GNN_PROG_ENT8 / GNN_PROG_ENT4: the program's entry format, one per graph (prog_ent_t).  In the 4-byte format a tile's 32 row weights are
// one dword per lane, requested with the tile's slot header - a tile ahead, in front of the start-up spread for a wave's first tile - where
// the first batch is requested ahead, and with the next tile's first entry behind the dense layers where it is not (those instantiations
// have no register to carry them across).
// ACTL: the last layer's activation (tile_epilogue_last); used in section C only.
// SEED: the seeded form of the label projection (GNN_FUSED_DENSE_LAYERS; the arguments describe the net over [state | aggregated state]).
template <int LAYERS, int NT, int ACT, bool SPLIT, bool GIVEN, int PC, int PROG, int ACTL, bool SEED = false>
__global__ void __launch_bounds__(GNN_FUSED_THREADS, 2) k_fused_full(const GnnFusedArgs a0)
{
    static_assert(!SEED || (SPLIT && !GIVEN), "the label projection is a form of the split arithmetic, and of the gathering kernels");
    static_assert(PROG == GNN_PROG_NONE || PROG == GNN_PROG_ENT8 || PROG == GNN_PROG_ENT4, "CSR walk, or the program in one of its two entry formats");
    constexpr bool PROGRAM = PROG != GNN_PROG_NONE;
    using ENT = prog_ent_t<PROG>;
    constexpr int NTL = 2;
    const GnnFusedArgs &a = a0;      // (shadowed inside the tile loop)
    // Persistent workgroup of 8 waves (one per CU): every wave pulls 32-node tiles from a device-wide counter until none
    // is left.  Waves w and w + 4 share a SIMD; the second half starts late so that, in steady state, one partner streams
    // neighbour rows from HBM while the other runs its MFMA / activation phases (without the offset all waves of a CU
    // gather at once and then compute at once: HBM idles during compute, the matrix pipe during the gather).
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (!gnn_gate_open(a.gate, a.world)) return;
    fused_poison_lds(a, lds);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KP = a.KP, Ds = a.Ds;                   // (Ds: 64)
    float *X = lds + (size_t)wave * 32 * KP;
    const int c_aggs = a.c_aggs;                      // column of the aggregated state block (Ds + NLc + alignment hole)
    const int W_launch = (int)gridDim.x * (int)(blockDim.x >> 6);            // (tiles and tickets: fused_draw_ticket)
    const int w_launch = wave * (int)gridDim.x + (int)blockIdx.x;
    const bool third_round = (int64_t)2 * W_launch * 32 < a.n_rows;
    // PROG: tile / next_tile / the tickets are SLOTS of the launch's tile schedule; the tile a slot stands for comes with its header (tid)
    int tile = w_launch + a.tile_base, next_tile = w_launch + W_launch + a.tile_base;
    int ip_first_raw = 0;
    v4i hdr_first_raw = {0, 0, 0, 0};
    int roww_cur = 0, roww_next = 0;                  // 4-byte entries: the row weights of the current / the next tile (prog_weight)
    if constexpr (PROGRAM) { hdr_first_raw = prog_header_request(a, tile); roww_cur = prog_roww_request<ENT>(a, tile, lane); }
    else ip_first_raw = tile_rowptr_request(a, tile, lane);           // on its way while the workgroup stages its vectors below
    float *ep = lds + (size_t)GNN_FUSED_WAVES * 32 * KP + 32 + GNN_FUSED_WAVES * 36;
    float *hb = ep + 3 * 32 * NTL;
    fused_stage_vectors<LAYERS, NT, NTL, ACT, SPLIT>(a, ep, hb);
    fused_startup_spread(a, wave);
    int ip_cur = 0, src_cur = 0;
    float w_cur = 0.0f;
    // PROG: header of the current tile (wave-uniform) and this lane's entry of its first batch; AHEAD: the rows of that batch and the entry of
    // the second too
    // (not the bf16-piece format on 128-wide hidden layers: those instantiations stand at 254 - 255 registers without it and spill with it)
    constexpr bool AHEAD = PROGRAM && GNN_FIRST_BATCH_AHEAD && !(SPLIT && PC == 3 && NT == 4);
    int hdr_first = 0, hdr_nb = 0, tid = 0;
    ENT ent_cur = prog_ent_make<ENT>(AHEAD ? (int)GNN_GP_NOROW : 0), ent_second = prog_ent_make<ENT>(0);
    v4f x_first[16];
    if constexpr (PROGRAM) {
        hdr_first = __builtin_amdgcn_readfirstlane(hdr_first_raw.x); hdr_nb = __builtin_amdgcn_readfirstlane(hdr_first_raw.y);
        tid = __builtin_amdgcn_readfirstlane(hdr_first_raw.z);
        if (hdr_nb > 0) ent_cur = prog_entry<ENT>(a, hdr_first, lane);
        if constexpr (AHEAD) prog_first_batch_request(a, hdr_first, hdr_nb, ent_cur, lane, x_first, ent_second);
    } else {
        ip_cur = tile_rowptr_clamp(a, tile, lane, ip_first_raw);
        tile_first_ids(a, ip_cur, lane, src_cur, w_cur);
    }
    zero_pad_columns(a, X, lane, KP);                 // once: no tile ever writes the padding columns
  for (;;) {
    const int64_t i0 = (int64_t)(PROGRAM ? tid : tile) * 32;
    if (PROGRAM ? tile >= a.gp_slots : i0 >= a.n_rows) break;        // wave-uniform; no workgroup barrier anywhere in the tile loop
    const int nvalid = (int)((a0.n_rows - i0) < 32 ? (a0.n_rows - i0) : 32);
    GnnFusedArgs a = a0;
    if constexpr (SEED) { a.IW = 0; a.NLc = 0; a.AL = 0; }      // (the shadow net has no label columns: as constants, so that the tile loaders' label paths fold away)
    fused_opaque_pointers(a);
#ifdef GNN_DIAG
    unsigned long long *stamp = a.stamps ? a.stamps + ((size_t)(PROGRAM ? tid : tile) << 3) : nullptr;      // (by tile id, whatever the schedule)
#endif
    GNN_STAMP(0);

    // the tile's 33 row pointers go through LDS: the gather re-reads them inside divergent code, where a cross-lane
    // broadcast from lanes of another group would not be safe
    [[maybe_unused]] int *ipt = reinterpret_cast<int *>(lds + (size_t)GNN_FUSED_WAVES * 32 * KP + 32) + wave * 36;
    int ip_next_raw = 0;
    int hdr_first_next = 0, hdr_nb_next = 0, tid_next = 0;
    ENT ent_next = prog_ent_make<ENT>(0);
    v4i hdr_next_raw = {0, 0, 0, 0};
    if constexpr (PROGRAM) {
        hdr_next_raw = prog_header_request(a, next_tile);     // program header of the NEXT tile: on its way during the gather
        if constexpr (AHEAD) roww_next = prog_roww_request<ENT>(a, next_tile, lane);      // ... and with it that tile's row weights
    }
    else {
        if (lane <= 32) ipt[lane] = ip_cur;           // requested during the previous tile
        ip_next_raw = tile_rowptr_request(a, next_tile, lane);            // row pointers of the NEXT tile: on their way during the gather
    }
    // the gather is a chain of few instructions and long memory waits: with a raised priority its loads are issued ahead of the
    // SIMD partner's dense VALU / MFMA stream instead of behind it
    if (a.variant & 1) __builtin_amdgcn_s_setprio(3);
    if constexpr (GIVEN) load_tile_given64<SPLIT>(a, X, i0, lane, KP, c_aggs);      // feature-sliced exchange: no gather (a.agg_in)
    else if constexpr (AHEAD)
        load_tile_prog64_ahead<SPLIT>(a, X, i0, lane, KP, c_aggs, hdr_first, hdr_nb, ent_cur, x_first, ent_second, roww_cur, hdr_next_raw, hdr_first_next, hdr_nb_next, tid_next, ent_next);
    else if constexpr (PROGRAM) {
        load_tile_prog64<SPLIT>(a, X, i0, lane, KP, c_aggs, hdr_first, hdr_nb, ent_cur, roww_cur);      // (every tile of the launch has a program)
        // the next tile's slot header came back in front of the gather's rows: read here, it crosses the dense layers in scalar registers
        // (these instantiations have no vector register to spare: the bf16-piece format on 128-wide hidden layers)
        hdr_first_next = __builtin_amdgcn_readfirstlane(hdr_next_raw.x); hdr_nb_next = __builtin_amdgcn_readfirstlane(hdr_next_raw.y);
        tid_next = __builtin_amdgcn_readfirstlane(hdr_next_raw.z);
    }
    else load_tile_fast64<SPLIT>(a, X, ipt, i0, lane, KP, c_aggs, src_cur, w_cur);
    if (a.variant & 1) __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    GNN_STAMP(2);

    GNN_FUSED_DENSE_LAYERS(true, false)
    // ---- C: last-layer epilogue, new state to LDS (over the aggregated-state columns, no longer needed) ---------------
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    GNN_STAMP(5);
    // Requests for the tile after next (ticket) and for the next tile (ids / weights of its first gather batch): issued HERE,
    // behind the last weight loads, because vector-memory results return in issue order - in front of the dense layers these
    // HBM-latency loads would hold up every weight wait - and the epilogue / norm / stores below cover their latency.
    // AHEAD: the range flag first (it waits for its word when it is raised), then the ticket and the gate words, and only behind them the
    // next tile's second entry and first batch: what is read first is requested first, so that no wait in the epilogue reaches the sixteen rows.
    if constexpr (AHEAD && SPLIT && PC == 2) gnn_flag_raise_range(a.flag_out, mx);
    int next2_tile = fused_draw_ticket<AHEAD>(a0, third_round, W_launch, lane);
    int ip_next = 0, src_next = 0;
    float w_next = 0.0f;
    if constexpr (AHEAD) { }                                  // (header and batch-0 entry of the next tile: read with this tile's last gather batch)
    else if constexpr (PROGRAM) {
        if (hdr_nb_next > 0) ent_next = prog_entry<ENT>(a, hdr_first_next, lane);      // (header of the next tile: read behind the gather)
        roww_next = prog_roww_request<ENT>(a, next_tile, lane);
    } else {
        ip_next = tile_rowptr_clamp(a, next_tile, lane, ip_next_raw);
        tile_first_ids(a, ip_next, lane, src_next, w_next);
    }
    if constexpr (!AHEAD && SPLIT && PC == 2) gnn_flag_raise_range(a.flag_out, mx);
    GnnFlagPeek peek = {0, 0, 0};                             // the gate words of this wave's slot: on their way across the epilogue arithmetic
    if (SPLIT && lane == 0) peek = gnn_flag_peek(a.flag_out);
    if constexpr (AHEAD) {
        __builtin_amdgcn_sched_barrier(0);                    // (the scheduler is free to move a load in front of an earlier one)
        prog_first_batch_request(a, hdr_first_next, hdr_nb_next, ent_next, lane, x_first, ent_second);
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (SPLIT) {                                    // registers -> norms, LDS (16-byte pieces), row stores
#pragma unroll
        for (int jt = 0; jt < NTL; ++jt) {
            if (a.bn_scale) tile_epilogue_last<ACTL, true, true, true, true>(a.act_last, out[jt], ep, ep + 32 * NTL, ep + 64 * NTL, jt, half, 1 << 30, a.usc[LAYERS - 1]);
            else tile_epilogue_last<ACTL, false, true, true, true>(a.act_last, out[jt], ep, nullptr, nullptr, jt, half, 1 << 30, a.usc[LAYERS - 1]);
        }
        GNN_STAMP(6);
        if (nvalid == 32) finish_fast64_aligned<AHEAD>(a, X, out, i0, lane, KP, c_aggs, peek);
        else finish_fast64_partial(a, X, out, i0, lane, KP, c_aggs, nvalid);       // (the range's last, partial tile)
    } else {
#pragma unroll
        for (int jt = 0; jt < NTL; ++jt) {
            if (a.bn_scale) tile_epilogue_last<ACTL, true, false, true, false>(a.act_last, out[jt], ep, ep + 32 * NTL, ep + 64 * NTL, jt, half, 1 << 30, 1.0f);
            else tile_epilogue_last<ACTL, false, false, true, false>(a.act_last, out[jt], ep, nullptr, nullptr, jt, half, 1 << 30, 1.0f);
            float *x = X + (lane & 31) * KP + c_aggs;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * jt + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (f < Ds) x[f] = out[jt][r];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        GNN_STAMP(6);
        if (nvalid == 32) check_store_fast64(a, X, i0, lane, KP, c_aggs);
        else check_store_fast64_partial(a, X, i0, lane, KP, c_aggs, nvalid);
    }
    GNN_STAMP(7);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the next tile re-uses this wave's LDS region
    tile = next_tile;
    next_tile = fused_next_tile<AHEAD>(a0, next2_tile, third_round, W_launch);
    ip_cur = ip_next; src_cur = src_next; w_cur = w_next;
    hdr_first = hdr_first_next; hdr_nb = hdr_nb_next; tid = tid_next; ent_cur = ent_next; roww_cur = roww_next;
  }
}
#undef GNN_STAMP
#undef GNN_FUSED_DENSE_LAYERS

// ---- launchers: one short chain per kernel, dispatching on the form of the launch (GnnFusedLaunch, gnn_fused.h) ----
template <auto KERNEL>
inline void launch_kernel(const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st)
{
    static bool lds_raised[64] = {false};   // (one table per instantiation)
    (void)gnn_raise_dynamic_lds(reinterpret_cast<const void *>(KERNEL), 160 * 1024, lds_raised);
    hipLaunchKernelGGL(KERNEL, grid, a.threads ? a.threads : GNN_FUSED_THREADS, lds_bytes, st, a);      // (a.threads: the wide-state form of k_fused_generic)
}

// k_fused_generic in the piece format of the launch (the exact path has one)
template <int LAYERS, int NT, int NTL, int ACT, bool SPLIT, int ACTL, bool SEED = false>
inline void launch_generic_pc(const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st)
{
    if (SPLIT && how.pieces == 2) launch_kernel<k_fused_generic<LAYERS, NT, NTL, ACT, SPLIT, 2, ACTL, SEED>>(a, grid, lds_bytes, st);
    else launch_kernel<k_fused_generic<LAYERS, NT, NTL, ACT, SPLIT, 3, ACTL, SEED>>(a, grid, lds_bytes, st);
}
// (NT, NTL) pairs that are instantiated; gnn_fused.hip rounds every net up to one of them
template <int LAYERS, int ACT, bool SPLIT, int ACTL, bool SEED = false>
inline bool launch_generic(int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st)
{
    // unreachable: make_plan sets NTL = round_tiles(Ds), so a state width of 64 has NTL == 2, and gnn_loop_decide_form gives every such
    // loop the full-tile or the pair kernel.  k_fused_generic has none of the width-64 paths.
    if (a.Ds == 64) return false;
    if constexpr (LAYERS == 1) {
        if (ntl == 1) launch_generic_pc<1, 1, 1, ACT, SPLIT, ACTL, SEED>(how, a, grid, lds_bytes, st);
        else if (ntl == 2) launch_generic_pc<1, 2, 2, ACT, SPLIT, ACTL, SEED>(how, a, grid, lds_bytes, st);
        else if (ntl == 4) launch_generic_pc<1, 4, 4, ACT, SPLIT, ACTL, SEED>(how, a, grid, lds_bytes, st);
        else return false;
    } else {
        if (nt == 1 && ntl == 1) launch_generic_pc<LAYERS, 1, 1, ACT, SPLIT, ACTL, SEED>(how, a, grid, lds_bytes, st);
        else if (nt == 2 && ntl == 2) launch_generic_pc<LAYERS, 2, 2, ACT, SPLIT, ACTL, SEED>(how, a, grid, lds_bytes, st);
        else if (nt == 4 && ntl == 2) launch_generic_pc<LAYERS, 4, 2, ACT, SPLIT, ACTL, SEED>(how, a, grid, lds_bytes, st);
        else if (nt == 4 && ntl == 4) launch_generic_pc<LAYERS, 4, 4, ACT, SPLIT, ACTL, SEED>(how, a, grid, lds_bytes, st);
        else return false;
    }
    return true;
}

// k_fused_full in the launch's gather form - a given aggregate, the graph's program in the entry format the graph holds, or the CSR walk -
// and piece format
// (SEED: no instantiation with a given aggregate - launch_full refuses it)
template <int LAYERS, int NT, int ACT, bool SPLIT, int ACTL, bool SEED = false>
inline void launch_full_form(const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st)
{
    auto gather_form = [&](auto P) {
        constexpr int PC = P.value;
        if constexpr (SEED) {
            if (how.program && how.entries == 4) launch_kernel<k_fused_full<LAYERS, NT, ACT, SPLIT, false, PC, GNN_PROG_ENT4, ACTL, true>>(a, grid, lds_bytes, st);
            else if (how.program) launch_kernel<k_fused_full<LAYERS, NT, ACT, SPLIT, false, PC, GNN_PROG_ENT8, ACTL, true>>(a, grid, lds_bytes, st);
            else launch_kernel<k_fused_full<LAYERS, NT, ACT, SPLIT, false, PC, GNN_PROG_NONE, ACTL, true>>(a, grid, lds_bytes, st);
        } else {
            if (how.given) launch_kernel<k_fused_full<LAYERS, NT, ACT, SPLIT, true, PC, GNN_PROG_NONE, ACTL>>(a, grid, lds_bytes, st);
            else if (how.program && how.entries == 4) launch_kernel<k_fused_full<LAYERS, NT, ACT, SPLIT, false, PC, GNN_PROG_ENT4, ACTL>>(a, grid, lds_bytes, st);
            else if (how.program) launch_kernel<k_fused_full<LAYERS, NT, ACT, SPLIT, false, PC, GNN_PROG_ENT8, ACTL>>(a, grid, lds_bytes, st);
            else launch_kernel<k_fused_full<LAYERS, NT, ACT, SPLIT, false, PC, GNN_PROG_NONE, ACTL>>(a, grid, lds_bytes, st);
        }
    };
    if (SPLIT && how.pieces == 2) gather_form(std::integral_constant<int, 2>{});
    else gather_form(std::integral_constant<int, 3>{});      // (the exact path has one)
}
// the last layer has 2 tiles; hidden layers of 2 or 4
template <int LAYERS, int ACT, bool SPLIT, int ACTL, bool SEED = false>
inline bool launch_full(int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st)
{
    if (ntl != 2) return false;
    if (SEED && how.given) return false;
    if constexpr (LAYERS == 1) launch_full_form<1, 2, ACT, SPLIT, ACTL, SEED>(how, a, grid, lds_bytes, st);
    else {
        if (nt == 2) launch_full_form<LAYERS, 2, ACT, SPLIT, ACTL, SEED>(how, a, grid, lds_bytes, st);
        else if (nt == 4) launch_full_form<LAYERS, 4, ACT, SPLIT, ACTL, SEED>(how, a, grid, lds_bytes, st);
        else return false;
    }
    return true;
}

// The activation id act as a template argument: f(std::integral_constant<int, ACT>); false for an id without instantiations
template <class F>
inline bool dispatch_act(int act, F &&f)
{
    switch (act) {
    case GNN_ACT_LINEAR: return f(std::integral_constant<int, GNN_ACT_LINEAR>{});
    case GNN_ACT_RELU: return f(std::integral_constant<int, GNN_ACT_RELU>{});
    case GNN_ACT_SELU: return f(std::integral_constant<int, GNN_ACT_SELU>{});
    case GNN_ACT_ELU: return f(std::integral_constant<int, GNN_ACT_ELU>{});
    case GNN_ACT_TANH: return f(std::integral_constant<int, GNN_ACT_TANH>{});
    case GNN_ACT_SIGMOID: return f(std::integral_constant<int, GNN_ACT_SIGMOID>{});
    default: return false;
    }
}

// The entry of a translation unit: the instantiations of LAYERS layers in one arithmetic mode, for every hidden activation act.
// MIXED: the last layer reads its activation from a.act_last (a net whose last layer has its own), else it is act
template <int LAYERS, bool SPLIT, bool MIXED = false>
inline bool launch_fused(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st)
{
    static_assert(!MIXED || LAYERS >= 2, "a one-layer net has one activation");
    return dispatch_act(act, [&](auto A) {
        constexpr int ACT = A.value, ACTL = MIXED ? GNN_ACTL_FROM_ARGS : ACT;
        return how.full ? launch_full<LAYERS, ACT, SPLIT, ACTL>(nt, ntl, how, a, grid, lds_bytes, st)
                        : launch_generic<LAYERS, ACT, SPLIT, ACTL>(nt, ntl, how, a, grid, lds_bytes, st);
    });
}

// The entry of a seeded translation unit (label projection): split arithmetic, the last layer's activation always from a.act_last - one
// family per hidden activation serves nets with and without a last activation of their own
template <int LAYERS>
inline bool launch_fused_seeded(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st)
{
    if (!a.seed) return false;
    if constexpr (LAYERS == 1) act = GNN_ACT_LINEAR;      // (no hidden layer: ACT is read nowhere, one family serves all)
    return dispatch_act(act, [&](auto A) {
        constexpr int ACT = LAYERS == 1 ? GNN_ACT_LINEAR : A.value;
        return how.full ? launch_full<LAYERS, ACT, true, GNN_ACTL_FROM_ARGS, true>(nt, ntl, how, a, grid, lds_bytes, st)
                        : launch_generic<LAYERS, ACT, true, GNN_ACTL_FROM_ARGS, true>(nt, ntl, how, a, grid, lds_bytes, st);
    });
}

}   // namespace gnn_fused_dev
