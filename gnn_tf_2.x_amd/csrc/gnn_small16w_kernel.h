// Persistent small-graph loop on 16-node tiles for nets with hidden layers up to 64 wide: the dense layers of k_small16w.  The third form
// of the launch, beside k_small16 (gnn_small16_kernel.h, every layer <= 32 wide) and k_small_loop (gnn_small_kernel.h); the hand-off
// protocol and every other phase are those of gnn_small_common.h, unchanged.  Instantiated by gnn_small16w.hip (one activation for all
// layers) and gnn_small16w_m.hip (the last layer has its own); two or three layers (a one-layer net has no hidden layer to be wide).
//
// As k_small16: one wave per 16-node tile, v_mfma_f32_16x16x4_f32 accumulated in k order (the oracle's fmaf chain), layer inputs as the B
// operand (k = 4 s + lane / 16, node = lane % 16), weights as the A operand, read once per launch from the Keras-layout kernels
// (small16_w) and kept in registers.  What differs:
//   * a hidden layer is FOUR 16-feature tiles, whatever its width (33 .. 63, or a narrow layer beside a wide one: the weights and the
//     bias behind the width are zeros, so the padded features are act(0), finite, and meet zero weights in the next layer): layer 0 is
//     S0 K-steps x 4 tiles, a hidden -> hidden layer 16 x 4, the last layer 16 K-steps x 1 or 2 tiles (state width <= 32) - at most
//     96 + 64 + 32 weight registers per lane, which a one-wave workgroup's unified 512-entry VGPR + AGPR file holds;
//   * the four chains of a hidden layer are independent and issued K-step by K-step (tile 0 .. 3 of step s, then step s + 1): each
//     accumulator still sees its products in k order, and no MFMA waits for the one in front of it;
//   * the LDS copy of the hidden activations the next layer reads its B operand from is [16][GNN_SMALL16W_HP] with all 64 columns
//     written in every body (bank argument of the stride: gnn_fused.h).
#pragma once
#include "gnn_small16_kernel.h"

namespace gnn_fused_dev {

static_assert(GnnSmallLds<16, true>::LABELS == GnnSmallLds<16>::LABELS, "the shared phases address the label rows through GnnSmallLds<16>");

// bias + activation of a hidden layer's four accumulators (features 16 j + 4 (lane / 16) + r of node lane % 16), written to the LDS copy
// H[node][feature]; rows of H are 8-byte aligned
template <int ACT>
__device__ __forceinline__ void small16w_hidden(const v4f (&acc)[4], const float *bias, float *H, int lane)
{
    const int n = lane & 15, g = lane >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const v4f bb = *reinterpret_cast<const v4f *>(bias + 16 * j + 4 * g);
        float *h = H + n * GNN_SMALL16W_HP + 16 * j + 4 * g;
        *reinterpret_cast<v2f *>(h) = act_t2<ACT>(v2f{acc[j].x, acc[j].y} + v2f{bb.x, bb.y});
        *reinterpret_cast<v2f *>(h + 2) = act_t2<ACT>(v2f{acc[j].z, acc[j].w} + v2f{bb.z, bb.w});
    }
}

// a layer with a 64-wide (padded) output: STEPS K-steps x 4 feature tiles.  Straight-line code: the accumulators are read in the basic
// block of their last MFMA, where the compiler inserts the wait states itself (the s_nop guard of small16_layer is for a chain that ends
// a block; the last layer below goes through small16_layer and keeps it)
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

// S0: K-steps (of 4) of layer 0 kept in registers (one of GnnSmall16S0, covering the concat width)
// ACT / ACTL: activation of the hidden layers / of the last layer (as k_small16)
template <int LAYERS, int ACT, int S0, int ACTL = ACT>
__global__ void __launch_bounds__(64) k_small16w(const GnnFusedArgs a0, const GnnSmallCtl c)
{
    static_assert(LAYERS == 2 || LAYERS == 3, "a wide hidden layer needs two or three layers");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x, n = lane & 15, g = lane >> 4;
    SMALL_DIAG_BEGIN();
    SMALL_STAMP();
    const int KP = c.KP16, Ds = a0.Ds, c_aggs = a0.c_aggs;
    using L = GnnSmallLds<16, true>;
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
    // weights: once, into registers (A operands).  w1: the second hidden layer (three layers); wl: the last layer
    float w0[S0][4], w1[16][4], wl[16][2];
#pragma unroll
    for (int s = 0; s < S0; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) w0[s][j] = small16_w(c.Wraw[0], c.din[0], c.dout[0], s, j, lane);
    if constexpr (LAYERS == 3) {
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) w1[s][j] = small16_w(c.Wraw[1], c.din[1], c.dout[1], s, j, lane);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int j = 0; j < 2; ++j) wl[s][j] = small16_w(c.Wraw[LAYERS - 1], c.din[LAYERS - 1], c.dout[LAYERS - 1], s, j, lane);
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
    const int xs_bytes = (int)gridDim.x * 16 * c.DP * 4;
    const __amdgpu_buffer_rsrc_t xs_rs[2] = {__builtin_amdgcn_make_buffer_rsrc(c.xs, 0, xs_bytes, 0x00020000),
                                             __builtin_amdgcn_make_buffer_rsrc(c.xs + (size_t)gridDim.x * 16 * c.DP, 0, xs_bytes, 0x00020000)};
    // ---- state <- initial state (GNN.py:262 / :265), then the first condition -----------------------------------------------------
    int go;
    {
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
        const int moved = small_first_condition<16>(a0, c, xs_rs[0], i0, scr, nvalid, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        SMALL_STAMP();                                               // 2: initial state, first condition
        go = arrive_and_gate(c, 0, __any(moved), lane);
        SMALL_STAMP();                                               // 3: gate 0
    }
    const bool last_two = Ds > 16;                                   // the last layer needs its second feature tile
    int k = 0;
    for (; k < c.max_iter && go == 1; ++k) {
        if (k > 0) {                                                 // the new state of the last body becomes the own state
            const int total = nvalid * Ds;
            RowCol rc(lane, Ds);
            for (int t = lane; t < total; t += 64, rc.next()) X[rc.i * KP + rc.c] = X[rc.i * KP + c_aggs + rc.c];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // before the aggregated state overwrites those columns
        }
        {
            const __amdgpu_buffer_rsrc_t rs = xs_rs[k & 1];
            const int *es = ecached ? ec_src : nullptr;
            const float *ew = ecached ? ec_w : nullptr;
            if (c.DP == 32) {
                if (c.rnd == 8) small_gather<16, 8, 8>(rs, X, ipt, lane, nvalid, KP, c_aggs, Ds, a0.adj_src, a0.adj_w, es, ew, e_base);
                else small_gather<16, 8, 4>(rs, X, ipt, lane, nvalid, KP, c_aggs, Ds, a0.adj_src, a0.adj_w, es, ew, e_base);
            } else {
                if (c.rnd == 8) small_gather<16, 4, 8>(rs, X, ipt, lane, nvalid, KP, c_aggs, Ds, a0.adj_src, a0.adj_w, es, ew, e_base);
                else small_gather<16, 4, 4>(rs, X, ipt, lane, nvalid, KP, c_aggs, Ds, a0.adj_src, a0.adj_w, es, ew, e_base);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        SMALL_STAMP();                                               // body + 0: gather
        v4f out[2];
        {
            const float *xb = X + n * KP + g, *hbp = H + n * GNN_SMALL16W_HP + g;
            v4f h[4];
            small16w_layer<S0>(xb, w0, h);
            small16w_hidden<ACT>(h, hb, H, lane);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if constexpr (LAYERS == 3) {
                small16w_layer<16>(hbp, w1, h);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the B operands were read before H is rewritten)
                small16w_hidden<ACT>(h, hb + L::HBW, H, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
            small16_layer<16>(hbp, wl, out, last_two);
        }
        // last layer: bias, activation, BatchNormalization; the new state into the aggregated-state columns (no longer needed)
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
            float *x = X + n * KP + c_aggs + f0;
            if (f0 < Ds) x[0] = p0.x;
            if (f0 + 1 < Ds) x[1] = p0.y;
            if (f0 + 2 < Ds) x[2] = p1.x;
            if (f0 + 3 < Ds) x[3] = p1.y;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        SMALL_STAMP();                                               // body + 1: dense layers, new state in LDS
        // the new rows first (they drain while the condition is evaluated), then the condition of GNN.py:202-220 in k_check's order:
        // lanes 0-15 sum (new - old)^2, lanes 16-31 sum old^2, ascending feature, unfused
        small_store_rows<16>(c.DP, xs_rs[(k & 1) ^ 1], i0, X + c_aggs, KP, 16, Ds, lane);
        int moved;
        {
            const float *xo = X + n * KP, *xn = xo + c_aggs;
            float s_ = 0.0f;
            if (g < 2)
                for (int f = 0; f < Ds; ++f) {
                    const float o = xo[f];
                    const float d = g ? o : (xn[f] - o);
                    const float dd = d * d;
                    s_ = s_ + dd;
                }
            const float root = sqrtf(s_);
            const float nrm = shfl_f(root, n + 16);
            const float rhs = a0.thr * nrm;
            moved = __any((g == 0) && (n < nvalid) && (root > rhs)) ? 1 : 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
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
