// Shared phases of the persistent small-graph loop: ONE launch runs every body of a GNN.Loop (reference GNN/GNN.py:271, tf.while_loop
// of condition :202-220 and convergence :223-242) when the batch is small enough for all of its tiles to be resident at once (BASELINE
// configs[0] / [1]: a few hundred to a few thousand nodes, nets no wider than 32).  It has two kernels that differ in the
// set-up of the tile and the dense layers only: k_small_loop on 32-node tiles (gnn_small_kernel.h) and k_small16 on 16-node tiles
// (gnn_small16_kernel.h), the latter with a WIDE form for hidden layers up to 64 wide; everything else is here, templated on the rows
// per tile (ROWS = 32 or 16) where it depends on it, with the LDS layout (GnnSmallLds) and the instantiation lists in gnn_fused.h.
//
// Such loops are latency bound: a body is one short chain of dependent loads and narrow MFMAs per tile, and as one launch per body it is
// mostly launch gap, cold caches and host gating.  Here every tile is a one-wave workgroup that keeps its row pointers in LDS, its weights
// in registers, and meets the other tiles at a grid barrier after each body (arrive_and_gate):
//   * new state rows are stored write-through (sc1), every wave drains its stores (s_waitcnt vmcnt(0)), one lane adds to the body's
//     barrier word with a relaxed agent-scope atomic, polls it with relaxed agent-scope (L1-bypassing) loads, and only then reads state
//     rows, all of them with sc1 loads - the fence-free hand-off of cdna_hip_programming.md Guideline 16 (R1) / MI355X_MICROARCH.md
//     hand-off table, row 1;
//   * the same word carries the convergence verdict (high half: workgroups with a node that still moves), so every workgroup reads the
//     same gate with the poll it does anyway and all of them leave the loop at the same body;
//   * weights stay in registers, row pointers, label columns and the tile's own new state in LDS from body to body;
//   * every spin is bounded (1 << 22 polls, s_sleep(1) between them): on a timeout (e.g. the grid could not become resident beside
//     another stream's work) the kernel sets the status word host_result[1] and the host repeats the Loop with one launch per body.
// Arithmetic: the oracle's k-ordered fmaf chains (bit-identical to oracle/gnn_oracle.c) for both fused modes; at these sizes the matrix
// work is a few microseconds either way.
#pragma once
#include "gnn_fused_kernel.h"

namespace gnn_fused_dev {

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// Diagnostic build only (GNN_DIAG): SMALL_DIAG_BEGIN() opens a kernel body - GNN_POISON=1 fills the whole LDS allocation with NaN before
// anything is staged (one-wave workgroup: program order is enough) - and SMALL_STAMP() records s_memtime of workgroup 0 at every phase
// boundary (GNN_SMALL_STAMPS=<file>).  Both expect a0, lds and lane in scope.
#ifdef GNN_DIAG
#define SMALL_DIAG_BEGIN()                                                                              \
    int stamp_n = 0;                                                                                    \
    if (a0.lds_floats) {                                                                                \
        for (int t = lane; t < a0.lds_floats; t += 64) lds[t] = __builtin_nanf("");                     \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                                          \
    }
#define SMALL_STAMP()                                                                                   \
    do {                                                                                                \
        if (a0.stamps && blockIdx.x == 0) {                                                             \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                 \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();                                 \
            if (lane == 0 && stamp_n < 250) a0.stamps[stamp_n] = t_;                                    \
            ++stamp_n;                                                                                  \
        }                                                                                               \
    } while (0)
#else
#define SMALL_DIAG_BEGIN() do { } while (0)
#define SMALL_STAMP() do { } while (0)
#endif

// Grid barrier + gate in ONE word per body: after its write-through stores have drained, every workgroup adds 1 (+ 0x10000 when one of
// its nodes still moves) to word[b]; the word is complete when its low half reaches the number of workgroups, and body b runs iff its
// high half is non-zero (GNN.py:218-220: reduce_any over all nodes).  One atomic and one bounded poll per body, by lane 0; the word it
// saw is broadcast to the wave with readfirstlane, so the verdict is wave-uniform.  Returns 1 = run body b, 0 = converged, -1 = gave up.
__device__ __forceinline__ int arrive_and_gate(const GnnSmallCtl &c, int b, int moved, int lane)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned n_wg = gridDim.x;
    unsigned seen = 0;
    if (lane == 0) {
        GNN_GLOBAL unsigned *word = (GNN_GLOBAL unsigned *)(c.flags + b);
        __hip_atomic_fetch_add(word, 1u + (moved ? 0x10000u : 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (unsigned spins = 0;; ++spins) {
            seen = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((seen & 0xffffu) >= n_wg) break;
            if (spins > (1u << 22)) { seen = 0xffffffffu; break; }       // give up: the host falls back to per-body launches
            __builtin_amdgcn_s_sleep(1);
        }
    }
    seen = (unsigned)__builtin_amdgcn_readfirstlane((int)seen);
    if (seen == 0xffffffffu) {
        // STICKY failure: the kernel only ever SETS the status word (pinned host memory; the host clears it before the launch, gnn_small_run).  A
        // workgroup that gives up has already added itself to the barrier word, so a late arrival can still complete that barrier
        // for the others; if it is the last one they finish normally - and must not overwrite this 1 with a 0.
        if (lane == 0) c.host_result[1] = 1;
        return -1;
    }
    return (seen >> 16) ? 1 : 0;
}

// Start of the launch: the last-layer bias and BatchNormalization scale / shift (ep [3][32]), the biases of the hidden layers (hb [2][HBW],
// HBW = 32 or, for the wide k_small16, 64 floats of the bias image, which is zero behind the layer's width) and, with the output stage folded in,
// the net_output head (hw: W [wf * T <= 512], then b | BN scale | BN shift [3][8]) into LDS
template <int LAYERS, int HBW = 32>
__device__ __forceinline__ void small_stage_vectors(const GnnFusedArgs &a0, const GnnSmallCtl &c, float *ep, float *hb, float *hw, int lane)
{
    static_assert(HBW == 32 || HBW == 64, "hidden layers of one or two 32-feature tiles");
    for (int t = lane; t < 3 * 32; t += 64) {
        const int which = t >> 5, f = t & 31;
        ep[t] = which == 0 ? a0.bias[LAYERS - 1][f] : (a0.bn_scale ? (which == 1 ? a0.bn_scale[f] : a0.bn_shift[f]) : 0.0f);
    }
    if constexpr (LAYERS >= 2 && HBW == 32) {
        if (lane < 32 * (LAYERS - 1)) hb[lane] = a0.bias[lane >> 5][lane & 31];      // 64 lanes = 2 x 32 features
    }
    if constexpr (LAYERS >= 2 && HBW == 64) {
#pragma unroll
        for (int q = 0; q < LAYERS - 1; ++q) hb[64 * q + lane] = a0.bias[q][lane];
    }
    if (c.out) {
        const int nw = (a0.Ds + c.NLc) * c.T;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (lane + 64 * u < nw) hw[lane + 64 * u] = c.ow[lane + 64 * u];
        if (lane < 24) {
            const int which = lane >> 3, q = lane & 7;
            float v = which == 1 ? 1.0f : 0.0f;
            if (q < c.T) v = which == 0 ? c.ob[q] : (c.obn_scale ? (which == 1 ? c.obn_scale[q] : c.obn_shift[q]) : v);
            hw[512 + lane] = v;
        }
    }
}

// Everything the launch reads from read-only memory is requested HERE, at once (one round trip for all of it): the row pointer of lane
// (<= nvalid), the tile's initial rows ([row][Ds] order, ROWS / 2 values per lane), and what the output stage needs at the very end:
// mask and output position of the lane's row, and the label rows, which go to scr + GnnSmallLds<ROWS>::LABELS at once (scr is not
// touched again before the output stage)
template <int ROWS>
__device__ __forceinline__ void small_upfront_reads(const GnnFusedArgs &a0, const GnnSmallCtl &c, int64_t i0, int nvalid, float *scr, int lane,
                                                    int &my_ip, float (&v_init)[ROWS / 2], bool &out_on, int &out_pos)
{
    my_ip = (lane <= nvalid) ? gload1(a0.indptr + i0 + lane) : 0;
    {
        const float *init = c.init + i0 * a0.Ds;
#pragma unroll
        for (int u = 0; u < ROWS / 2; ++u) v_init[u] = (lane + 64 * u < nvalid * a0.Ds) ? gload1(init + lane + 64 * u) : 0.0f;
    }
    out_on = false;
    out_pos = 0;
    if (c.out) {
        const int nl = c.NLc ? nvalid * c.NL : 0;                   // <= 32 ROWS (NL <= 32)
        const float *nod = c.nodes_own + i0 * c.NL;
        float lv[ROWS / 2];
#pragma unroll
        for (int u = 0; u < ROWS / 2; ++u) lv[u] = (lane + 64 * u < nl) ? gload1(nod + lane + 64 * u) : 0.0f;
        out_on = lane < nvalid && c.mask[i0 + (lane < nvalid ? lane : 0)];
        out_pos = out_on ? c.mask_pos[i0 + lane] : 0;
#pragma unroll
        for (int u = 0; u < ROWS / 2; ++u)
            if (lane + 64 * u < nl) scr[GnnSmallLds<ROWS>::LABELS + lane + 64 * u] = lv[u];
    }
}

// the tile's row pointers [ROWS + 1], kept in LDS for every body (rows past nvalid: empty)
template <int ROWS>
__device__ __forceinline__ void small_store_rowptrs(int *ipt, int my_ip, int nvalid, int lane)
{
    const int last_ip = shfl_i(my_ip, nvalid);
    if (lane <= ROWS) ipt[lane] = lane <= nvalid ? my_ip : last_ip;
}

// The tile's arcs (contiguous CSR entries of its rows): ids and weights once into LDS when they fit - every body's gather then needs one
// memory round trip per round (the neighbour rows) instead of two.  Returns whether the arcs are cached; e_base: the tile's first arc.
template <int ROWS>
__device__ __forceinline__ bool small_cache_arcs(const GnnFusedArgs &a0, const GnnSmallCtl &c, const int *ipt, int *ec_src, float *ec_w, int lane, int &e_base)
{
    e_base = ipt[0];
    const int e_cnt = ipt[ROWS] - e_base;
    const bool ecached = e_cnt <= c.ecache;
    if (ecached)
        for (int t = lane; t < e_cnt; t += 64) { ec_src[t] = gload1(a0.adj_src + e_base + t); ec_w[t] = gload1(a0.adj_w + e_base + t); }
    return ecached;
}

// the gate words of the NEXT run (the other half of the double buffer): nobody reads them during this launch
__device__ __forceinline__ void small_clear_next_words(const GnnSmallCtl &c, int lane)
{
    if (blockIdx.x == 0)
        for (int t = lane; t < c.n_words; t += 64) c.zero_words[t] = 0;
}

// ---- padded exchange rows ------------------------------------------------------------------------------------------------------
// Between bodies the state travels through a buffer of its own, xs[2][tiles * ROWS][DP] with DP = 16 or 32 floats per row (a 64- or
// 128-byte line piece per node), not through the [N, Ds] state replicas: a tile publishes its new rows as ONE contiguous block of 16-byte
// write-through stores (a 4-byte sc1 store is a fabric write of its own, MI355X_MICROARCH.md "stores of each flavour") and a neighbour
// row is fetched with 16-byte sc1 loads.  The [N, Ds] replicas get the initial and the final state only.

// The tile's ROWS rows -> its block of the padded buffer.  Source element (row, col) at src[row * rs_ + col]; rows >= nrows and columns
// >= Ds are stored as zeros (never read back into a result: a gather only keeps columns < Ds of rows that exist)
template <int ROWS, int DP>
__device__ __forceinline__ void small_store_padded(__amdgpu_buffer_rsrc_t rs, int64_t i0, const float *src, int rs_, int nrows, int Ds, int lane)
{
    constexpr int QR = DP / 4;                       // 16-byte pieces per row
#pragma unroll
    for (int u = 0; u < (ROWS * QR) / 64; ++u) {
        const int q = lane + 64 * u, row = q / QR, c4 = (q % QR) * 4;
        const float *x = src + row * rs_ + c4;
        const bool rok = row < nrows;
        v4f v;
        v.x = (rok && c4 < Ds) ? x[0] : 0.0f;
        v.y = (rok && c4 + 1 < Ds) ? x[1] : 0.0f;
        v.z = (rok && c4 + 2 < Ds) ? x[2] : 0.0f;
        v.w = (rok && c4 + 3 < Ds) ? x[3] : 0.0f;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), rs, (int)(i0 * DP + 4 * q) * 4, 0, 16);       // aux 16 = sc1: write-through
    }
}
template <int ROWS>
__device__ __forceinline__ void small_store_rows(int DP, __amdgpu_buffer_rsrc_t rs, int64_t i0, const float *src, int rs_, int nrows, int Ds, int lane)
{
    if (DP == 16) small_store_padded<ROWS, 16>(rs, i0, src, rs_, nrows, Ds, lane);
    else small_store_padded<ROWS, 32>(rs, i0, src, rs_, nrows, Ds, lane);
}

// Aggregated neighbour states of the tile's rows from the padded exchange rows: 64 / ROWS lanes per node, HW floats per lane (DP = HW * 64
// / ROWS), PR arcs per round.  The fmaf chain per column runs over the arcs in stored order.
template <int ROWS, int HW, int PR>
__device__ __forceinline__ void small_gather(__amdgpu_buffer_rsrc_t rs, float *X, const int *ipt, int lane, int nvalid, int KP, int c_aggs, int Ds,
                                             const int *adj_src, const float *adj_w, const int *ec_src, const float *ec_w, int ec_base)
{
    constexpr int PARTS = 64 / ROWS;
    const int node = lane & (ROWS - 1), part = lane / ROWS;
    const int beg = ipt[node], end = ipt[node + 1];
    float acc[HW];
#pragma unroll
    for (int c = 0; c < HW; ++c) acc[c] = 0.0f;
    for (int e = beg; e < end; e += PR) {
        float w[PR];
        int off[PR];
#pragma unroll
        for (int u = 0; u < PR; ++u) {
            const int ee = e + u < end ? e + u : e;            // clamp: a real entry, result unused
            w[u] = ec_w ? ec_w[ee - ec_base] : gload1(adj_w + ee);
            const int src = ec_src ? ec_src[ee - ec_base] : gload1(adj_src + ee);
            off[u] = (src * (PARTS * HW) + part * HW) * 4;
        }
        v4f x[PR][HW / 4];
#pragma unroll
        for (int u = 0; u < PR; ++u)
#pragma unroll
            for (int j = 0; j < HW / 4; ++j) x[u][j] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rs, off[u] + 16 * j, 0, 16));    // aux 16 = sc1
#pragma unroll
        for (int u = 0; u < PR; ++u)
            if (e + u < end) {
#pragma unroll
                for (int j = 0; j < HW / 4; ++j) {
                    acc[4 * j] = __builtin_fmaf(w[u], x[u][j].x, acc[4 * j]);
                    acc[4 * j + 1] = __builtin_fmaf(w[u], x[u][j].y, acc[4 * j + 1]);
                    acc[4 * j + 2] = __builtin_fmaf(w[u], x[u][j].z, acc[4 * j + 2]);
                    acc[4 * j + 3] = __builtin_fmaf(w[u], x[u][j].w, acc[4 * j + 3]);
                }
            }
    }
    if (node < nvalid) {
        float *x = X + node * KP + c_aggs + part * HW;
#pragma unroll
        for (int c = 0; c < HW; ++c)
            if (part * HW + c < Ds) x[c] = acc[c];
    }
}

// the two exchange buffers xs[2][tiles * ROWS][DP] as buffer resources (16-byte sc1 loads / stores): body k gathers from rs[k & 1] and
// publishes to the other
template <int ROWS>
__device__ __forceinline__ void small_exchange_rsrc(const GnnSmallCtl &c, __amdgpu_buffer_rsrc_t (&rs)[2])
{
    const int xs_bytes = (int)gridDim.x * ROWS * c.DP * 4;
    rs[0] = __builtin_amdgcn_make_buffer_rsrc(c.xs, 0, xs_bytes, 0x00020000);
    rs[1] = __builtin_amdgcn_make_buffer_rsrc(c.xs + (size_t)gridDim.x * ROWS * c.DP, 0, xs_bytes, 0x00020000);
}

// The gather instantiation of (c.DP, c.rnd), per tile size: HW = DP * ROWS / 64 floats per lane, c.rnd = 8 or 4 arcs per round (a 32-node
// tile with 128-byte rows takes 4).  ec_src / ec_w: the tile's arcs in LDS when they are cached (small_cache_arcs), else nullptr - chosen
// by the kernel, not here: with the choice inside this function the compiler tests it per arc instead of once per gather.
__device__ __forceinline__ void small_gather16(const GnnFusedArgs &a0, const GnnSmallCtl &c, __amdgpu_buffer_rsrc_t rs, float *X, const int *ipt, int lane,
                                               int nvalid, int KP, const int *ec_src, const float *ec_w, int e_base)
{
    const int c_aggs = a0.c_aggs, Ds = a0.Ds;
    if (c.DP == 32) {
        if (c.rnd == 8) small_gather<16, 8, 8>(rs, X, ipt, lane, nvalid, KP, c_aggs, Ds, a0.adj_src, a0.adj_w, ec_src, ec_w, e_base);
        else small_gather<16, 8, 4>(rs, X, ipt, lane, nvalid, KP, c_aggs, Ds, a0.adj_src, a0.adj_w, ec_src, ec_w, e_base);
    } else {
        if (c.rnd == 8) small_gather<16, 4, 8>(rs, X, ipt, lane, nvalid, KP, c_aggs, Ds, a0.adj_src, a0.adj_w, ec_src, ec_w, e_base);
        else small_gather<16, 4, 4>(rs, X, ipt, lane, nvalid, KP, c_aggs, Ds, a0.adj_src, a0.adj_w, ec_src, ec_w, e_base);
    }
}
__device__ __forceinline__ void small_gather32(const GnnFusedArgs &a0, const GnnSmallCtl &c, __amdgpu_buffer_rsrc_t rs, float *X, const int *ipt, int lane,
                                               int nvalid, int KP, const int *ec_src, const float *ec_w, int e_base)
{
    const int c_aggs = a0.c_aggs, Ds = a0.Ds;
    if (c.DP == 32) small_gather<32, 16, 4>(rs, X, ipt, lane, nvalid, KP, c_aggs, Ds, a0.adj_src, a0.adj_w, ec_src, ec_w, e_base);
    else if (c.rnd == 8) small_gather<32, 8, 8>(rs, X, ipt, lane, nvalid, KP, c_aggs, Ds, a0.adj_src, a0.adj_w, ec_src, ec_w, e_base);
    else small_gather<32, 8, 4>(rs, X, ipt, lane, nvalid, KP, c_aggs, Ds, a0.adj_src, a0.adj_w, ec_src, ec_w, e_base);
}

// The initial rows (staged in LDS as rows[nvalid][Ds]) -> exchange buffer 0, which body 0 gathers from behind gate 0; then the first
// condition against ones (GNN.py:266, :271) in the oracle's order (k_check: ascending feature, unfused, one lane per row).  Returns
// whether a row of the lane moves.
template <int ROWS>
__device__ __forceinline__ int small_first_condition(const GnnFusedArgs &a0, const GnnSmallCtl &c, __amdgpu_buffer_rsrc_t rs0, int64_t i0,
                                                     const float *rows, int nvalid, int lane)
{
    const int Ds = a0.Ds;
    small_store_rows<ROWS>(c.DP, rs0, i0, rows, Ds, nvalid, Ds, lane);
    int moved = 0;
    if (lane < nvalid) {
        float dist = 0.0f, nrm = 0.0f;
        for (int f = 0; f < Ds; ++f) {
            const float df = rows[lane * Ds + f] - 1.0f;
            const float dd = df * df;
            dist = dist + dd;
            nrm = nrm + 1.0f;
        }
        moved = sqrtf(dist) > a0.thr * sqrtf(nrm);
    }
    return moved;
}

// End of the loop: the final state of the tile's rows (the new-state columns of the last body) into the [N, Ds] replica the host expects
// it in (k & 1; k == 0: replica 0 holds it already) - and into rows[nvalid][Ds] when given - and the executed bodies (GNN.py:267; every
// workgroup agrees) by workgroup 0.  The status words are NOT touched here.
__device__ __forceinline__ void small_finish_state(const GnnFusedArgs &a0, const GnnSmallCtl &c, const float *X, float *rows, int KP, int c_aggs,
                                                   int64_t i0, int nvalid, int k, int lane)
{
    if (k > 0) {
        const int Ds = a0.Ds;
        float *dst = ((k & 1) ? c.state1 : c.state0) + (a0.row_begin + i0) * Ds;
        const int total = nvalid * Ds;
        RowCol rc(lane, Ds);
        for (int t = lane; t < total; t += 64, rc.next()) {
            const float v = X[rc.i * KP + c_aggs + rc.c];
            *gptr_w(dst + t) = v;
            if (rows) rows[t] = v;
        }
    }
    if (blockIdx.x == 0 && lane == 0) {
        c.kfinal[0] = k;
        c.host_result[0] = k;
    }
}

// ---- apply_filters + one-layer net_output on the tile's masked rows (GNN.py:275-279), arithmetic as k_out1: k-ordered fmaf chain per
// output, bias, softmax / activation, BatchNormalization.  The tile's final state rows are in scr [row][Ds] order, its label rows at
// scr + LABELS (staged at kernel start), the head's weights in hw (staged at kernel start) --------------------------------------------
template <int ROWS>
__device__ __forceinline__ void small_output_stage(const GnnSmallCtl &c, const float *scr, const float *hw, int Ds, bool out_on, int out_pos, int lane)
{
    const int wf = Ds + c.NLc, T = c.T, NL = c.NL;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (out_on) {
        float y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = 0.0f;
        for (int kk = 0; kk < wf; ++kk) {                            // k-ordered fmaf chain per output, as k_out1
            const float x = kk < Ds ? scr[lane * Ds + kk] : scr[GnnSmallLds<ROWS>::LABELS + lane * NL + (kk - Ds)];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < T) y[j] = __builtin_fmaf(x, hw[kk * T + j], y[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < T) y[j] = y[j] + hw[512 + j];
        float v[8];
        if (c.oact == GNN_ACT_SOFTMAX) {
            float mx = y[0];
#pragma unroll
            for (int q = 1; q < 8; ++q)
                if (q < T) mx = y[q] > mx ? y[q] : mx;
            float sum = 0.0f;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < T) { v[q] = gnn_expf(y[q] - mx); sum = sum + v[q]; }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < T) v[q] = __fdiv_rn(v[q], sum);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < T) v[q] = gnn_act(y[q], c.oact);
        }
        float *o = c.out + (int64_t)out_pos * T;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (q < T) {
                float r = v[q];
                if (c.obn_scale) { const float t2 = r * hw[520 + q]; r = t2 + hw[528 + q]; }
                sstore1<true>(o + q, r);                         // write-through: workgroup 0 may read it below (graph readout)
            }
    }
}

// Graph readout (GNN.py:331-332, arithmetic of k_readout): out_graph[g, t] = sum over the (node, w) of graph g, ascending, fmaf(w, out[node,
// t]), one lane per (g, t), by workgroup 0 after one more grid barrier behind the output stage; the result goes straight to pinned host
// memory.  The entries of a graph are taken eight at a time: their (node, w) pairs are requested together, then the eight output values
// (sc1 loads: other workgroups wrote them in this launch), then the eight fmaf in stored order - two round trips per eight nodes instead of
// two per node (a MUTAG graph has 18: 36 dependent round trips were 36 us of a 128 us Loop).
__device__ __forceinline__ void small_graph_readout(const GnnSmallCtl &c, int lane)
{
    if (!c.ng_ip || arrive_and_gate(c, c.ro_word, 0, lane) < 0 || blockIdx.x != 0) return;
    for (int t = lane; t < c.G * c.T; t += 64) {
        const int gi = t / c.T, ci = t - gi * c.T;
        const int e0 = gload1(c.ng_ip + gi), e1 = gload1(c.ng_ip + gi + 1);
        float acc = 0.0f;
        for (int e = e0; e < e1; e += 8) {
            int node[8];
            float w[8], v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int ee = e + u < e1 ? e + u : e;          // clamp: a real entry, result unused
                node[u] = gload1(c.ng_node + ee);
                w[u] = gload1(c.ng_w + ee);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = sload1<true>(c.out + (int64_t)node[u] * c.T + ci);
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (e + u < e1) acc = __builtin_fmaf(w[u], v[u], acc);
        }
        c.ng_host[t] = acc;
    }
}

// Host side: the kernel of (layers, act, steps) from a form's instantiation list STEPS (gnn_fused.h) - launch(L, A, S) with integral
// constants; false when there is none
template <int... V, class F>
inline bool dispatch_steps(int v, GnnSteps<V...>, F &&f)
{
    return ((v == V && (f(std::integral_constant<int, V>{}), true)) || ...);
}
template <class STEPS, class F>
inline bool small_dispatch(int layers, int act, int steps, F &&launch)
{
    auto with = [&](auto L) {
        return dispatch_act(act, [&](auto A) { return dispatch_steps(steps, STEPS{}, [&](auto S) { launch(L, A, S); }); });
    };
    if (layers == 1) return with(std::integral_constant<int, 1>{});
    if (layers == 2) return with(std::integral_constant<int, 2>{});
    if (layers == 3) return with(std::integral_constant<int, 3>{});
    return false;
}

}   // namespace gnn_fused_dev
