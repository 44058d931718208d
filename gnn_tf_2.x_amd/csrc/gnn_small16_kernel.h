// Persistent small-graph loop on 16-node tiles: k_small16, its dense layers and the phases of its body.  The hand-off protocol and every
// phase the two tile sizes share are in gnn_small_common.h; the 32-node form is gnn_small_kernel.h.  Instantiated by gnn_small16.hip (one
// activation for all layers) and gnn_small16_m.hip (the last layer has its own) for nets with every layer <= 32 wide, and with WIDE by
// gnn_small16w.hip / gnn_small16w_m.hip for two- and three-layer nets with hidden layers up to 64 wide.
//
// A body of the persistent loop is a chain of latencies, not of throughput: one wave per tile walks gather -> three dependent dense
// layers -> condition -> barrier, and with 32 nodes per wave the dense layers alone are 48 dependent v_mfma_f32_32x32x2_f32 (64 cycles
// each) plus 16 activations per lane and layer.  Batches of up to 4,096 nodes therefore run on 16-node tiles: twice the workgroups,
// v_mfma_f32_16x16x4_f32 (32 cycles, four k per instruction, accumulated in k order like the 32x32x2 form: the parity tests compare
// every bit with the C oracle's k-ordered fmaf chain), 8 activations per lane and layer, one 16-byte load per lane and arc.
//   * layer inputs are the B operand (k = 4 s + lane / 16, node = lane % 16): layer 0 reads it from the LDS tile, deeper layers from
//     a small LDS copy of the previous activations (the accumulator holds features 16 j + 4 (lane / 16) + r, so the hop through LDS
//     is the transpose);
//   * weights are the A operand, read once per launch from the Keras-layout kernels (W[k][f], k = 4 s + lane / 16,
//     f = 16 j + lane % 16) and kept in registers.
// WIDE differs in the dense layers only:
//   * a hidden layer is FOUR 16-feature tiles, whatever its width (33 .. 63, or a narrow layer beside a wide one: the weights and the
//     bias behind the width are zeros, so the padded features are act(0), finite, and meet zero weights in the next layer): layer 0 is
//     S0 K-steps x 4 tiles, a hidden -> hidden layer 16 x 4, the last layer 16 K-steps x 1 or 2 tiles (state width <= 32) - at most
//     96 + 64 + 32 weight registers per lane, which a one-wave workgroup's unified 512-entry VGPR + AGPR file holds;
//   * the four chains of a hidden layer are independent and issued K-step by K-step (tile 0 .. 3 of step s, then step s + 1): each
//     accumulator still sees its products in k order, and no MFMA waits for the one in front of it;
//   * the LDS copy of the hidden activations is [16][GNN_SMALL16W_HP] with all 64 columns written in every body (bank argument of the
//     stride: gnn_fused.h).
#pragma once
#include "gnn_small_common.h"

namespace gnn_fused_dev {

static_assert(GnnSmallLds<16, true>::LABELS == GnnSmallLds<16>::LABELS, "the shared phases address the label rows through GnnSmallLds<16>");

// A operand of (K-step s, feature tile j) from the Keras-layout kernel W[din][dout]
__device__ __forceinline__ float small16_w(const float *W, int din, int dout, int s, int j, int lane)
{
    const int k = 4 * s + (lane >> 4), f = 16 * j + (lane & 15);
    return (k < din && f < dout) ? gload1(W + (size_t)k * dout + f) : 0.0f;
}
template <int STEPS, int NT>
__device__ __forceinline__ void small16_weights(float (&w)[STEPS][NT], const GnnSmallCtl &c, int layer, int lane)
{
    const float *W = c.Wraw[layer];                                  // once per layer: read inside the loops, the control block's words are
    const int din = c.din[layer], dout = c.dout[layer];              // fetched again (scalar load + wait) in front of every weight load
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
        for (int j = 0; j < NT; ++j) w[s][j] = small16_w(W, din, dout, s, j, lane);
}

// bias + activation of a hidden layer's NT accumulators (features 16 j + 4 (lane / 16) + r of node lane % 16), written to the LDS copy
// H[node][feature] the next layer reads its B operand from: [16][GNN_SMALL16_HP] with 16-byte stores for two tiles, [16][GNN_SMALL16W_HP]
// (rows 8-byte aligned) with 8-byte stores for four
template <int ACT, int NT>
__device__ __forceinline__ void small16_hidden(const v4f (&acc)[NT], const float *bias, float *H, int lane)
{
    const int n = lane & 15, g = lane >> 4;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const v4f bb = *reinterpret_cast<const v4f *>(bias + 16 * j + 4 * g);
        const v2f p0 = act_t2<ACT>(v2f{acc[j].x, acc[j].y} + v2f{bb.x, bb.y});
        const v2f p1 = act_t2<ACT>(v2f{acc[j].z, acc[j].w} + v2f{bb.z, bb.w});
        if constexpr (NT == 2) {
            *reinterpret_cast<v4f *>(H + n * GNN_SMALL16_HP + 16 * j + 4 * g) = v4f{p0.x, p0.y, p1.x, p1.y};
        } else {
            float *h = H + n * GNN_SMALL16W_HP + 16 * j + 4 * g;
            *reinterpret_cast<v2f *>(h) = p0;
            *reinterpret_cast<v2f *>(h + 2) = p1;
        }
    }
}

template <int STEPS>
__device__ __forceinline__ void small16_layer(const float *b_base, const float (&w)[STEPS][2], v4f (&acc)[2], bool second)
{
    float b[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) b[s] = b_base[4 * s];
    acc[0] = v4f{0.f, 0.f, 0.f, 0.f};
    acc[1] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < STEPS; ++s) acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s][0], b[s], acc[0], 0, 0, 0);
    if (second) {
#pragma unroll
        for (int s = 0; s < STEPS; ++s) acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s][1], b[s], acc[1], 0, 0, 0);
    } else {
        // The branch around the second chain puts the first chain's last MFMA directly in front of whatever reads acc[0] next, in
        // another basic block - and hipcc (ROCm 7.2) then inserts no wait states between an 8-pass MFMA and the v_accvgpr_read of its
        // last destination register: with the linear activation (the read follows at once) feature 3 of every node came out stale
        // (found by test_persistent_small_graph_loop_random_shapes).  Sixteen wait states here cover the 8-pass result.
        // Guard: every object's rule in the Makefile scans its ISA listing (tools/scan_mfma_hazard.py, -save-temps=obj) and fails the build
        // if such an edge reappears.  Tying the wait to the data instead - acc[0] as an in / out operand of this statement,
        // "+v" or "+a" - was tried in round 4 and RE-CREATES the hazard: the compiler then copies the accumulator for the operand
        // (v_accvgpr_read / v_accvgpr_mov) as the first instruction of this block, in front of the s_nop (108 hits in the scan).
        asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
    }
}

// a layer with a 64-wide (padded) output: STEPS K-steps x 4 feature tiles.  Straight-line code: the accumulators are read in the basic
// block of their last MFMA, where the compiler inserts the wait states itself (the s_nop guard of small16_layer is for a chain that ends
// a block; the last layer of the wide form goes through small16_layer and keeps it)
template <int STEPS>
__device__ __forceinline__ void small16w_layer(const float *b_base, const float (&w)[STEPS][4], v4f (&acc)[4])
{
    float b[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) b[s] = b_base[4 * s];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s][j], b[s], acc[j], 0, 0, 0);
}

// the last layer's activation on a pair of accumulators: act_t2<ACTL>, or for ACTL == GNN_ACTL_FROM_ARGS act_t2 of act_last behind a
// wave-uniform switch (as tile_epilogue_last)
template <int ACTL>
__device__ __forceinline__ void small16_act_last(int act_last, v2f &p0, v2f &p1)
{
    if constexpr (ACTL != GNN_ACTL_FROM_ARGS) {
        p0 = act_t2<ACTL>(p0); p1 = act_t2<ACTL>(p1);
    } else {
        switch (act_last) {
        case GNN_ACT_RELU: p0 = act_t2<GNN_ACT_RELU>(p0); p1 = act_t2<GNN_ACT_RELU>(p1); break;
        case GNN_ACT_SELU: p0 = act_t2<GNN_ACT_SELU>(p0); p1 = act_t2<GNN_ACT_SELU>(p1); break;
        case GNN_ACT_ELU: p0 = act_t2<GNN_ACT_ELU>(p0); p1 = act_t2<GNN_ACT_ELU>(p1); break;
        case GNN_ACT_TANH: p0 = act_t2<GNN_ACT_TANH>(p0); p1 = act_t2<GNN_ACT_TANH>(p1); break;
        case GNN_ACT_SIGMOID: p0 = act_t2<GNN_ACT_SIGMOID>(p0); p1 = act_t2<GNN_ACT_SIGMOID>(p1); break;
        default: p0 = act_t2<GNN_ACT_LINEAR>(p0); p1 = act_t2<GNN_ACT_LINEAR>(p1); break;
        }
    }
}

// ---- phases of the body, in the order the kernel walks them -----------------------------------------------------------------------

// state <- initial state (GNN.py:262 / :265): the rows requested at kernel start into replica 0, scr ([row][Ds] order) and the tile's
// own-state columns, and through small_first_condition into exchange buffer 0.  Returns whether a row of the lane moves.
__device__ __forceinline__ int small16_initial_state(const GnnFusedArgs &a0, const GnnSmallCtl &c, __amdgpu_buffer_rsrc_t rs0, float *X, float *scr,
                                                     int KP, int64_t i0, int nvalid, const float (&v_init)[8], int lane)
{
    const int Ds = a0.Ds;
    float *own0 = c.state0 + (a0.row_begin + i0) * Ds;
    const int total = nvalid * Ds;
    RowCol rc(lane, Ds);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (lane + 64 * u < total) {
            *gptr_w(own0 + lane + 64 * u) = v_init[u];              // replica 0: read by nobody in this launch (k == 0: the final state)
            scr[lane + 64 * u] = v_init[u];
            X[rc.i * KP + rc.c] = v_init[u];                        // the tile's own-state columns
        }
        rc.next();
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int moved = small_first_condition<16>(a0, c, rs0, i0, scr, nvalid, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    return moved;
}

// start of a body > 0: the new state of the last body becomes the own state
__device__ __forceinline__ void small16_new_to_own(float *X, int KP, int c_aggs, int Ds, int nvalid, int lane)
{
    const int total = nvalid * Ds;
    RowCol rc(lane, Ds);
    for (int t = lane; t < total; t += 64, rc.next()) X[rc.i * KP + rc.c] = X[rc.i * KP + c_aggs + rc.c];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // before the aggregated state overwrites those columns
}

// last layer: bias, activation, BatchNormalization (ep [3][32]); the new state into the aggregated-state columns (no longer needed)
template <int ACTL>
__device__ __forceinline__ void small16_last_epilogue(const GnnFusedArgs &a0, const v4f (&out)[2], bool last_two, const float *ep, float *X, int KP, int lane)
{
    const int n = lane & 15, g = lane >> 4, Ds = a0.Ds;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j == 1 && !last_two) break;
        const int f0 = 16 * j + 4 * g;
        const v4f bb = *reinterpret_cast<const v4f *>(ep + f0);
        v2f p0 = v2f{out[j].x, out[j].y} + v2f{bb.x, bb.y};
        v2f p1 = v2f{out[j].z, out[j].w} + v2f{bb.z, bb.w};
        small16_act_last<ACTL>(a0.act_last, p0, p1);
        if (a0.bn_scale) {
            const v4f sc = *reinterpret_cast<const v4f *>(ep + 32 + f0), sh = *reinterpret_cast<const v4f *>(ep + 64 + f0);
            const v2f m0 = p0 * v2f{sc.x, sc.y}, m1 = p1 * v2f{sc.z, sc.w};
            p0 = m0 + v2f{sh.x, sh.y};
            p1 = m1 + v2f{sh.z, sh.w};
        }
        float *x = X + n * KP + a0.c_aggs + f0;
        if (f0 < Ds) x[0] = p0.x;
        if (f0 + 1 < Ds) x[1] = p0.y;
        if (f0 + 2 < Ds) x[2] = p1.x;
        if (f0 + 3 < Ds) x[3] = p1.y;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// the condition of GNN.py:202-220 in k_check's order: lanes 0-15 sum (new - old)^2, lanes 16-31 sum old^2, ascending feature, unfused.
// Returns (wave-uniform) whether a node of the tile still moves.
__device__ __forceinline__ int small16_condition(const GnnFusedArgs &a0, const float *X, int KP, int nvalid, int lane)
{
    const int n = lane & 15, g = lane >> 4;
    const float *xo = X + n * KP, *xn = xo + a0.c_aggs;
    float s_ = 0.0f;
    if (g < 2)
        for (int f = 0; f < a0.Ds; ++f) {
            const float o = xo[f];
            const float d = g ? o : (xn[f] - o);
            const float dd = d * d;
            s_ = s_ + dd;
        }
    const float root = sqrtf(s_);
    const float nrm = shfl_f(root, n + 16);
    const float rhs = a0.thr * nrm;
    const int moved = __any((g == 0) && (n < nvalid) && (root > rhs)) ? 1 : 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    return moved;
}

// S0: K-steps (of 4) of layer 0 kept in registers (one of GnnSmall16S0, covering the concat width)
// ACT / ACTL: activation of the hidden layers / of the last layer (as k_fused: ACT, or GNN_ACTL_FROM_ARGS = a0.act_last)
// WIDE: hidden layers of four 16-feature tiles (up to 64 wide) instead of two
template <int LAYERS, int ACT, int S0, int ACTL = ACT, bool WIDE = false>
__global__ void __launch_bounds__(64) k_small16(const GnnFusedArgs a0, const GnnSmallCtl c)
{
    static_assert(!WIDE || LAYERS == 2 || LAYERS == 3, "a wide hidden layer needs two or three layers");
    constexpr int HT = WIDE ? 4 : 2, HS = WIDE ? 16 : 8, HP = WIDE ? GNN_SMALL16W_HP : GNN_SMALL16_HP;     // hidden layers: tiles, K-steps, LDS stride
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x, n = lane & 15, g = lane >> 4;
    SMALL_DIAG_BEGIN();
    SMALL_STAMP();
    const int KP = c.KP16, Ds = a0.Ds, c_aggs = a0.c_aggs;
    using L = GnnSmallLds<16, WIDE>;
    float *X = lds;                                               // the tile [16][KP]: own state | labels | aggregated state | aggregated labels | zeros
    float *tail = lds + 16 * KP, *H = tail + L::H;
    int *ipt = reinterpret_cast<int *>(tail + L::IPT);
    float *ep = tail + L::EP, *hb = tail + L::HB, *hw = tail + L::HW, *scr = tail + L::SCR;
    int *ec_src = reinterpret_cast<int *>(tail + L::EC_SRC);
    float *ec_w = tail + L::EC_W;
    small_stage_vectors<LAYERS, L::HBW>(a0, c, ep, hb, hw, lane);
    const int64_t i0 = (int64_t)blockIdx.x * 16;
    const int nvalid = (int)((a0.n_rows - i0) < 16 ? (a0.n_rows - i0) : 16);
    int my_ip, out_pos;
    float v_init[8];
    bool out_on;
    small_upfront_reads<16>(a0, c, i0, nvalid, scr, lane, my_ip, v_init, out_on, out_pos);
    // weights: once, into registers (A operands).  w0: layer 0 (a one-layer net: the last layer); w1: hidden -> hidden (three layers);
    // wl: the last layer of a deeper net
    float w0[S0][LAYERS == 1 ? 2 : HT], w1[LAYERS == 3 ? HS : 1][HT], wl[LAYERS >= 2 ? HS : 1][2];
    small16_weights(w0, c, 0, lane);
    if constexpr (LAYERS == 3) small16_weights(w1, c, 1, lane);
    if constexpr (LAYERS >= 2) small16_weights(wl, c, LAYERS - 1, lane);
    // the tile skeleton: zeros everywhere, then the label columns (they never change)
    for (int t = lane; t < 16 * KP; t += 64) X[t] = 0.0f;
    small_store_rowptrs<16>(ipt, my_ip, nvalid, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (a0.IW > 0) {
        const float *src = a0.inv + i0 * a0.IW;
        const int total = nvalid * a0.IW;
        RowCol rc(lane, a0.IW);
        for (int t = lane; t < total; t += 64, rc.next()) X[rc.i * KP + label_col(rc.c, Ds, a0.NLc, c_aggs)] = gload1(src + t);
    }
    int e_base;
    const bool ecached = small_cache_arcs<16>(a0, c, ipt, ec_src, ec_w, lane, e_base);
    small_clear_next_words(c, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    SMALL_STAMP();                                                   // 1: set-up
    __amdgpu_buffer_rsrc_t xs_rs[2];
    small_exchange_rsrc<16>(c, xs_rs);
    const int moved0 = small16_initial_state(a0, c, xs_rs[0], X, scr, KP, i0, nvalid, v_init, lane);
    SMALL_STAMP();                                                   // 2: initial state, first condition
    int go = arrive_and_gate(c, 0, __any(moved0), lane);
    SMALL_STAMP();                                                   // 3: gate 0
    const bool last_two = Ds > 16;                                   // the last layer needs its second feature tile
    int k = 0;
    for (; k < c.max_iter && go == 1; ++k) {
        if (k > 0) small16_new_to_own(X, KP, c_aggs, Ds, nvalid, lane);
        small_gather16(a0, c, xs_rs[k & 1], X, ipt, lane, nvalid, KP, ecached ? ec_src : nullptr, ecached ? ec_w : nullptr, e_base);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        SMALL_STAMP();                                               // body + 0: gather
        v4f out[2];
        const float *xb = X + n * KP + g, *hbp = H + n * HP + g;
        if constexpr (LAYERS == 1) {
            small16_layer<S0>(xb, w0, out, last_two);
        } else {
            v4f h[HT];
            if constexpr (WIDE) small16w_layer<S0>(xb, w0, h);
            else small16_layer<S0>(xb, w0, h, true);
            small16_hidden<ACT>(h, hb, H, lane);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if constexpr (LAYERS == 3) {
                if constexpr (WIDE) small16w_layer<HS>(hbp, w1, h);
                else small16_layer<HS>(hbp, w1, h, true);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the B operands were read before H is rewritten)
                small16_hidden<ACT>(h, hb + L::HBW, H, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
            small16_layer<HS>(hbp, wl, out, last_two);
        }
        small16_last_epilogue<ACTL>(a0, out, last_two, ep, X, KP, lane);
        SMALL_STAMP();                                               // body + 1: dense layers, new state in LDS
        // the new rows first (they drain while the condition is evaluated), then the condition
        small_store_rows<16>(c.DP, xs_rs[(k & 1) ^ 1], i0, X + c_aggs, KP, 16, Ds, lane);
        const int moved = small16_condition(a0, X, KP, nvalid, lane);
        SMALL_STAMP();                                               // body + 2: row stores issued, condition
        go = arrive_and_gate(c, k + 1, moved, lane);
        SMALL_STAMP();                                               // body + 3: barrier + gate
    }
    if (go < 0) return;                      // (status word set; the host repeats the Loop with one launch per body)
    small_finish_state(a0, c, X, scr, KP, c_aggs, i0, nvalid, k, lane);          // (scr: [row][Ds] order for the output stage; k == 0: the initial rows are there already)
    if (c.out) small_output_stage<16>(c, scr, hw, Ds, out_on, out_pos, lane);
    SMALL_STAMP();                                                   // last: output stage
    small_graph_readout(c, lane);
}

}   // namespace gnn_fused_dev
