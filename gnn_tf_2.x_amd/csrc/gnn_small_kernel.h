// Persistent small-graph loop on 32-node tiles: the gather and the dense layers of k_small_loop.  The hand-off protocol and every phase
// the two tile forms share are in gnn_small_common.h; the 16-node form is gnn_small16_kernel.h.  Instantiated by gnn_small.hip (one
// activation for all layers) and gnn_small_m.hip (the last layer has its own).
// Arithmetic: the exact f32-MFMA chain of k_fused (bit-identical to oracle/gnn_oracle.c) for both fused modes.
#pragma once
#include "gnn_small_common.h"

namespace gnn_fused_dev {

// Dense layers with the packed A operands (gnn_fused_pack, exact image: [K-step][lane][tile]) held in REGISTERS for the whole
// launch: the same v_mfma_f32_32x32x2_f32 chains as layer_from_lds / layer_from_regs with one 32-feature tile (NT == 1), i.e.
// the oracle's k-ordered fmaf chains, without a weight load per body.
template <int KK>
__device__ __forceinline__ void small_layer0(const float *xb, const float (&w)[KK], f32x16 &acc)
{
    float b[KK];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) b[kk] = xb[2 * kk];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[kk], b[kk], acc, 0, 0, 0);
}

template <int ACT>
__device__ __forceinline__ void small_layer(f32x16 &hin, const float *bias_prev, int half, const float (&w)[16], f32x16 &acc)
{
    tile_epilogue<ACT, false, false, true>(hin, bias_prev, nullptr, nullptr, 0, half);     // bias_prev: staged in LDS at kernel start
    acc_to_operand(hin);
#pragma unroll
    for (int ss = 0; ss < 16; ++ss) {
        const int reg = 4 * (ss >> 2) + ((ss & 3) == 1 ? 2 : (ss & 3) == 2 ? 1 : (ss & 3));       // K-step ss <-> register (acc_to_operand)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[ss], hin[reg], acc, 0, 0, 0);
    }
}


// KK0: K-steps of layer 0 kept in registers (one of GnnSmallKK0, covering the concat width)
// ACT / ACTL: activation of the hidden layers / of the last layer (as k_fused: ACT, or GNN_ACTL_FROM_ARGS = a0.act_last)
template <int LAYERS, int ACT, int KK0, int ACTL = ACT>
__global__ void __launch_bounds__(64) k_small_loop(const GnnFusedArgs a0, const GnnSmallCtl c)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    SMALL_DIAG_BEGIN();
    SMALL_STAMP();
    const int KP = a0.KP, Ds = a0.Ds, c_aggs = a0.c_aggs, half = lane >> 5;
    using L = GnnSmallLds<32>;
    float *X = lds, *tail = lds + 32 * KP;
    int *ipt = reinterpret_cast<int *>(tail + L::IPT);
    float *ep = tail + L::EP, *hb = tail + L::HB, *hw = tail + L::HW, *scr = tail + L::SCR;
    int *ec_src = reinterpret_cast<int *>(tail + L::EC_SRC);
    float *ec_w = tail + L::EC_W;
    small_stage_vectors<LAYERS>(a0, c, ep, hb, hw, lane);
    const int64_t i0 = (int64_t)blockIdx.x * 32;
    const int nvalid = (int)((a0.n_rows - i0) < 32 ? (a0.n_rows - i0) : 32);
    int my_ip, out_pos;
    float v_init[16];
    bool out_on;
    small_upfront_reads<32>(a0, c, i0, nvalid, scr, lane, my_ip, v_init, out_on, out_pos);
    small_store_rowptrs<32>(ipt, my_ip, nvalid, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    int e_base;
    const bool ecached = small_cache_arcs<32>(a0, c, ipt, ec_src, ec_w, lane, e_base);
    // weights: once, into registers
    float w0[KK0], w1[16], w2[16];
#pragma unroll
    for (int kk = 0; kk < KK0; ++kk) w0[kk] = gload1(a0.Wp[0] + (size_t)kk * 64 + lane);
    if constexpr (LAYERS >= 2) {
#pragma unroll
        for (int ss = 0; ss < 16; ++ss) w1[ss] = gload1(a0.Wp[1] + (size_t)ss * 64 + lane);
    }
    if constexpr (LAYERS >= 3) {
#pragma unroll
        for (int ss = 0; ss < 16; ++ss) w2[ss] = gload1(a0.Wp[2] + (size_t)ss * 64 + lane);
    }
    small_clear_next_words(c, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    SMALL_STAMP();                                                   // 1: set-up loads issued (weights, row pointers)
    __amdgpu_buffer_rsrc_t xs_rs[2];
    small_exchange_rsrc<32>(c, xs_rs);
    // ---- state <- initial state (GNN.py:262 / :265) for the owned rows, then the first condition -------------------------------------
    int go;
    {
        float *own0 = c.state0 + (a0.row_begin + i0) * Ds;
        const int total = nvalid * Ds;                          // <= 32 x 32: sixteen values per lane at most (requested at kernel start)
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (lane + 64 * u < total) { *gptr_w(own0 + lane + 64 * u) = v_init[u]; X[lane + 64 * u] = v_init[u]; }      // replica 0: read by nobody in this launch (k == 0: the final state)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int moved = small_first_condition<32>(a0, c, xs_rs[0], i0, X, nvalid, lane);     // (the tile itself is built by body 0)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        SMALL_STAMP();                                               // 2: initial state copied, first condition
        go = arrive_and_gate(c, 0, __any(moved), lane);
        SMALL_STAMP();                                               // 3: gate 0
    }
    int k = 0;
    for (; k < c.max_iter && go == 1; ++k) {
        GnnFusedArgs a = a0;
        a.state_cur = c.init - a0.row_begin * Ds;                    // (body 0 builds the tile skeleton: own rows from the read-only initial state)
        a.state_nxt = nullptr;
        load_tile_generic<false, 4>(a, X, ipt, i0, lane, nvalid, KP, c_aggs, k > 0, nullptr, nullptr, 0, true);     // k > 0: the tile skeleton is still in LDS; no gather here
        small_gather32(a0, c, xs_rs[k & 1], X, ipt, lane, nvalid, KP, ecached ? ec_src : nullptr, ecached ? ec_w : nullptr, e_base);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        SMALL_STAMP();                                               // body + 0: tile loaded (gather)
        const float *xb = X + (lane & 31) * KP + half;
        f32x16 out;
        if constexpr (LAYERS == 1) {
            out = f32x16{};
            small_layer0<KK0>(xb, w0, out);
        } else {
            f32x16 h1 = {};
            small_layer0<KK0>(xb, w0, h1);
            if constexpr (LAYERS == 2) {
                out = f32x16{};
                small_layer<ACT>(h1, hb, half, w1, out);
            } else {
                f32x16 h2 = {};
                small_layer<ACT>(h1, hb, half, w1, h2);
                out = f32x16{};
                small_layer<ACT>(h2, hb + 32, half, w2, out);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (a.bn_scale) tile_epilogue_last<ACTL, true, false, true>(a.act_last, out, ep, ep + 32, ep + 64, 0, half, Ds);      // features >= Ds: padding of the tile
        else tile_epilogue_last<ACTL, false, false, true>(a.act_last, out, ep, nullptr, nullptr, 0, half, Ds);
        {
            float *x = X + (lane & 31) * KP + c_aggs;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = (r & 3) + 8 * (r >> 2) + 4 * half;
                if (f < Ds) x[f] = out[r];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        SMALL_STAMP();                                               // body + 1: dense layers, new state in LDS
        int moved = 0;
        // the new rows first (they drain while the condition is evaluated), then the condition
        small_store_rows<32>(c.DP, xs_rs[(k & 1) ^ 1], i0, X + c_aggs, KP, 32, Ds, lane);
        check_store_generic<false, false>(a, X, i0, lane, nvalid, KP, c_aggs, &moved);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        SMALL_STAMP();                                               // body + 2: condition, row stores drained
        go = arrive_and_gate(c, k + 1, moved, lane);
        SMALL_STAMP();                                               // body + 3: barrier + gate
    }
    if (go < 0) return;                      // (status words already set, see arrive_and_gate; this tile's output rows stay stale: the host repeats the Loop)
    small_finish_state(a0, c, X, nullptr, KP, c_aggs, i0, nvalid, k, lane);
    if (c.out) {
        // the tile's final state rows are still in LDS: the new-state columns of the last body, or (k == 0) the staged initial rows
        const int ns = nvalid * Ds;                                       // <= 1024 (Ds <= 32)
        RowCol rc(lane, Ds);
        for (int t = lane; t < ns; t += 64, rc.next()) scr[t] = k > 0 ? X[rc.i * KP + c_aggs + rc.c] : X[t];
        small_output_stage<32>(c, scr, hw, Ds, out_on, out_pos, lane);
    }
    SMALL_STAMP();                                                   // last: output stage
    small_graph_readout(c, lane);
}

}   // namespace gnn_fused_dev
