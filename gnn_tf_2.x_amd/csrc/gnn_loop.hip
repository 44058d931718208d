// The Loop handle of the gfx950 engine: creation and setters, the phases of one Loop, the run functions and the readouts.
//
// Reference call sites replaced (paths relative to the reference root):
//   k_feats       apply_filters()                 GNN/GNN.py:245-248
//   k_readout     tf.matmul(nodegraph, out, transpose_a=True)   GNN/GNN.py:331-332, GNN/LGNN.py:278
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gnn_engine.h"

// ---------------------------------------------------------------------------------------------------------------------
// kernels of the Loop's ends
// ---------------------------------------------------------------------------------------------------------------------
// k_final = number of executed bodies = first k whose gate is closed (or max_iter); one wave, 64 gates per pass
__global__ void k_finalize(const int *flags, int world, int max_iter, int *kfinal)
{
    const int lane = threadIdx.x;
    int k_final = max_iter;
    for (int k0 = 0; k0 < max_iter; k0 += 64) {
        const int k = k0 + lane;
        const bool closed = k < max_iter && !gnn_gate_open(flags + (size_t)k * world * GNN_FLAG_WORDS, world);
        const unsigned long long m = __ballot(closed);
        if (m) { k_final = k0 + __builtin_ctzll(m); break; }
    }
    if (lane == 0) { kfinal[0] = k_final; kfinal[1] = 0; }      // (word 1: status of the persistent loop, which never comes here)
    // certified gate of the split-arithmetic path (gnn_common.h, gnn_flag_raise_certified): gates 1 .. k_final that decided this run (the
    // gate of body max_iter is never consulted; gate 0 is the first condition, the same arithmetic on every path).  Not certified: no node
    // moved robustly AND some node was borderline.  The exact paths never raise words 1 / 2, so this stays 0 for them.
    int amb = 0;
    const int last = k_final < max_iter ? k_final : max_iter - 1;
    for (int k = 1 + lane; k <= last; k += 64) {
        const int *gate = flags + (size_t)k * world * GNN_FLAG_WORDS;
        int robust = 0, border = 0;
#pragma unroll 16      // (independent loads: sixteen slots' words in flight per lane instead of one dependent round trip per slot)
        for (int p = 0; p < world * GNN_FLAG_SLOTS; ++p) { robust |= gate[p * GNN_FLAG_STRIDE + 1]; border |= gate[p * GNN_FLAG_STRIDE + 2]; }
        amb |= (!robust && border) ? 1 : 0;
    }
    amb = __any(amb) ? 1 : 0;
    if (lane == 0) kfinal[2] = amb;
    // range guard of the fp16-piece format (gnn_fused_kernel.h, gnn_flag_raise_range): word 3 of the gates 1 .. k_final written by the bodies
    // that ran.  The other arithmetic never raises it.
    int range = 0;
    for (int k = 1 + lane; k <= k_final && k <= max_iter; k += 64) {
        const int *gate = flags + (size_t)k * world * GNN_FLAG_WORDS;
        for (int p = 0; p < world * GNN_FLAG_SLOTS; ++p) range |= gate[p * GNN_FLAG_STRIDE + 3];
    }
    range = __any(range) ? 1 : 0;
    if (lane == 0) kfinal[3] = range;
}

// apply_filters(): feats[m] = [state_final[row_m] | nodes[row_m] (iff D > 0)]
__global__ void k_feats(int64_t n_masked, const int32_t *__restrict__ masked_rows, GnnStateTabs tabs,
                        const int *kfinal, int Ds, const float *__restrict__ nodes_own, int NL, int NLc,
                        float *__restrict__ feats)
{
    const int wf = Ds + NLc;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_masked * wf) return;
    const float *state = gnn_state_after(tabs, *kfinal);
    const int64_t m = t / wf;
    const int c = (int)(t - m * wf);
    const int64_t row = masked_rows[m];
    feats[t] = c < Ds ? state[row * Ds + c] : nodes_own[row * NL + (c - Ds)];
}

// GNNedgeBased.apply_filters(): feats[m] = [F[dst(e)] | F[src(e)] | arc_labels[e]], e = m-th masked arc, F = [state | nodes?]
__global__ void k_feats_edge(int64_t n_masked, const int32_t *__restrict__ rows, const int32_t *__restrict__ entry_dst,
                             const int32_t *__restrict__ adj_src, GnnStateTabs tabs, const int *kfinal, int Ds,
                             const float *__restrict__ nodes, int NL, int NLc, const float *__restrict__ arc_labels, int AL,
                             float *__restrict__ feats, int64_t own_off)
{
    const int wn = Ds + NLc, wf = 2 * wn + AL;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_masked * wf) return;
    const float *state = gnn_state_after(tabs, *kfinal);
    const int64_t m = t / wf;
    int c = (int)(t - m * wf);
    const int64_t e = rows[m];
    float v;
    if (c < 2 * wn) {
        const int64_t node = c < wn ? own_off + entry_dst[e] : adj_src[e];      // destination: owned row -> row of the replica; source: already in the replica's index space
        if (c >= wn) c -= wn;
        v = c < Ds ? state[node * Ds + c] : nodes[node * NL + (c - Ds)];
    } else {
        v = arc_labels[e * AL + (c - 2 * wn)];
    }
    feats[t] = v;
}

// apply_filters + a ONE-layer net_output with few outputs (the usual classifier head, T <= 8) in one pass over the masked
// rows.  A one-wave block stages 64 feature rows [state | labels] into its LDS tile: 16-byte pieces of the rows, a lane's pieces all in
// flight at once, 16-byte LDS stores where widths and strides allow.  Lane r then runs row r alone: the k-ordered fmaf chain of every
// output j (same order as k_dense; the weights are wave-uniform reads), softmax / activation / BatchNormalization as k_softmax_bn.
// Saves materialising [M, NL + D] features and two more launches.  ld: row stride of the tile, a multiple of 4 with ld / 4 odd, so that
// the 16-byte row reads of 16 lanes fall on all banks.
#define GNN_OUT1_ROWS 64
static inline int out1_ld(int wf) { const int ld = (wf + 3) & ~3; return ((ld >> 2) & 1) ? ld : ld + 4; }

// columns [col0, col0 + w) of the tile <- src[rows[r] * stride + 0 .. w) for r < live
__device__ __forceinline__ void out1_stage(const float *__restrict__ src, int stride, int w, int col0, const int *rows, int live, float *tile, int ld, int lane)
{
    if (w == 0) return;
    if (((w | stride | col0) & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int q = w >> 2, dr = GNN_OUT1_ROWS / q, dc = GNN_OUT1_ROWS - dr * q, n = live * q;
        int r = lane / q, c = lane - r * q;
#pragma unroll 8
        for (int idx = lane; idx < n; idx += GNN_OUT1_ROWS) {
            const float4 v = *reinterpret_cast<const float4 *>(src + (int64_t)rows[r] * stride + 4 * c);
            *reinterpret_cast<float4 *>(tile + r * ld + col0 + 4 * c) = v;
            r += dr; c += dc;
            if (c >= q) { c -= q; ++r; }
        }
    } else {
        const int dr = GNN_OUT1_ROWS / w, dc = GNN_OUT1_ROWS - dr * w, n = live * w;
        int r = lane / w, c = lane - r * w;
#pragma unroll 8
        for (int idx = lane; idx < n; idx += GNN_OUT1_ROWS) {
            tile[r * ld + col0 + c] = src[(int64_t)rows[r] * stride + c];
            r += dr; c += dc;
            if (c >= w) { c -= w; ++r; }
        }
    }
}

template <int T>
__global__ void __launch_bounds__(GNN_OUT1_ROWS) k_out1(int64_t n_masked, const int32_t *__restrict__ masked_rows, GnnStateTabs tabs,
                       const int *kfinal, int Ds, const float *__restrict__ nodes_own, int NL, int NLc, int ld,
                       const float *__restrict__ W, const float *__restrict__ b, int act,
                       const float *__restrict__ bn_scale, const float *__restrict__ bn_shift, float *__restrict__ out)
{
    extern __shared__ float osh[];
    float *tile = osh;                                     // [64, ld]
    int *rows = reinterpret_cast<int *>(osh + GNN_OUT1_ROWS * ld);      // [64] table rows of the block's masked rows
    const int lane = threadIdx.x, wf = Ds + NLc;
    const float *state = gnn_state_after(tabs, *kfinal);
    const int64_t base = (int64_t)blockIdx.x * GNN_OUT1_ROWS, m = base + lane;
    const int live = n_masked - base < GNN_OUT1_ROWS ? (int)(n_masked - base) : GNN_OUT1_ROWS;
    rows[lane] = lane < live ? masked_rows[m] : 0;
    __syncthreads();
    out1_stage(state, Ds, Ds, 0, rows, live, tile, ld, lane);
    out1_stage(nodes_own, NL, NLc, Ds, rows, live, tile, ld, lane);
    __syncthreads();
    if (lane >= live) return;
    float y[T];
#pragma unroll
    for (int j = 0; j < T; ++j) y[j] = 0.0f;
    const float *x = tile + lane * ld;
    int k = 0;
    for (; k + 4 <= wf; k += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(x + k);
        const float xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < T; ++j) y[j] = __builtin_fmaf(xs[u], W[(k + u) * T + j], y[j]);
    }
    for (; k < wf; ++k)
#pragma unroll
        for (int j = 0; j < T; ++j) y[j] = __builtin_fmaf(x[k], W[k * T + j], y[j]);
#pragma unroll
    for (int j = 0; j < T; ++j) y[j] = y[j] + b[j];
    if (act == GNN_ACT_SOFTMAX) {
        float mx = y[0];
#pragma unroll
        for (int q = 1; q < T; ++q) mx = y[q] > mx ? y[q] : mx;
        float sum = 0.0f;
#pragma unroll
        for (int q = 0; q < T; ++q) { y[q] = gnn_expf(y[q] - mx); sum = sum + y[q]; }
#pragma unroll
        for (int j = 0; j < T; ++j) y[j] = __fdiv_rn(y[j], sum);
    } else {
#pragma unroll
        for (int j = 0; j < T; ++j) y[j] = gnn_act(y[j], act);
    }
#pragma unroll
    for (int j = 0; j < T; ++j) {
        float v = y[j];
        if (bn_scale) { const float t2 = v * bn_scale[j]; v = t2 + bn_shift[j]; }
        out[m * T + j] = v;
    }
}

// graph readout: out_graph[g, t] = sum over the stored (node, w) of graph g, ascending node, fmaf(w, out_nodes[node, t])
// Sharded: a rank sums the nodes it owns ([row_begin, row_begin + n_rows), out_nodes indexed from row_begin); the partial
// results are then added in rank order by k_sum_partials (exact when no graph straddles two shards: x + 0 == x).
__global__ void k_readout(int G, int T, const int32_t *__restrict__ indptr, const int32_t *__restrict__ node,
                          const float *__restrict__ w, const float *__restrict__ out_nodes, int64_t row_begin, int64_t n_rows,
                          float *__restrict__ out_graph)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= G * T) return;
    const int g = t / T, c = t - g * T;
    float acc = 0.0f;
    for (int e = indptr[g]; e < indptr[g + 1]; ++e) {
        const int64_t i = (int64_t)node[e] - row_begin;
        if (i >= 0 && i < n_rows) acc = __builtin_fmaf(w[e], out_nodes[i * T + c], acc);
    }
    out_graph[t] = acc;
}

__global__ void k_sum_partials(int count, int world, const float *__restrict__ partial, float *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    float acc = partial[t];
    for (int p = 1; p < world; ++p) acc = acc + partial[(size_t)p * count + t];
    out[t] = acc;
}

// own RNG for the initial state when none is injected (tf.random.normal(stddev=0.1), GNN.py:262, cannot be matched)
__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ void k_randn(int64_t count, int64_t offset, uint64_t seed, float stddev, float *out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint64_t h = splitmix64(seed ^ splitmix64((uint64_t)(t + offset)));
    const float u1 = ((float)(uint32_t)(h >> 40) + 1.0f) * (1.0f / 16777217.0f);
    const float u2 = (float)(uint32_t)((h >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);
    out[t] = stddev * sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

int gnn_launch_feats_edge(hipStream_t st, const gnn_loop *l, const float *state, float *feats)
{
    if (!l->n_edge_masked) return GNN_OK;
    const gnn_graph *g = l->g;
    const int64_t tot = l->n_edge_masked * l->ou->dims[0];
    hipLaunchKernelGGL(k_feats_edge, cdiv(tot, 256), 256, 0, st, l->n_edge_masked, l->edge_rows, l->edge_dst, g->sh->adj_src, GnnStateTabs{state, state, state},
                       l->kfinal_dev, l->Ds, g->nodes, g->NL, l->NLc, g->arc_labels_orig_own ? g->arc_labels_orig_own : l->edge_labels, g->AL, feats, l->own_off);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// loop
// ---------------------------------------------------------------------------------------------------------------------
static size_t loop_flag_words(const gnn_loop *l) { return (size_t)(l->max_iter + 2) * l->world * GNN_FLAG_WORDS; }
static size_t loop_ctr_words(const gnn_loop *l) { return (2 * ((size_t)l->max_iter + 1) + 3) & ~(size_t)3; }

extern "C" int gnn_loop_create(gnn_graph *g, gnn_mlp *net_state, gnn_mlp *net_output, int state_dim, int max_iter,
                               float threshold, gnn_comm *comm, gnn_loop **out)
{
    ARGCHK(out, "out is NULL");
    *out = nullptr;
    ARGCHK(g && net_state && net_output, "graph and both MLPs are required");
    ARGCHK(state_dim >= 0, "param <state_vect_dim> must be int>=0");           // GNN/GNN.py:53
    ARGCHK(max_iter >= 0 && max_iter <= 100000, "max_iteration=%d out of range", max_iter);
    ARGCHK(g->device == net_state->device && g->device == net_output->device, "handles live on different devices");
    const int Ds = state_dim ? state_dim : g->NL;
    const int NLc = state_dim ? g->NL : 0;
    const int in_s = Ds + NLc + Ds + NLc + g->AL;                              // GNN/MLP.py:104
    ARGCHK(net_state->dims[0] == in_s, "net_state input width %d != AL + 2*(NL + D) = %d", net_state->dims[0], in_s);
    ARGCHK(net_state->dims.back() == Ds, "net_state output width %d != state width %d", net_state->dims.back(), Ds);
    const bool edge_width = net_output->dims[0] == 2 * (Ds + NLc) + g->AL && net_output->dims[0] != Ds + NLc;
    ARGCHK(net_output->dims[0] == Ds + NLc || edge_width, "net_output input width %d is neither NL + D = %d (node/graph based) nor 2 (NL + D) + AL = %d (edge based)",
           net_output->dims[0], Ds + NLc, 2 * (Ds + NLc) + g->AL);
    const int world = comm ? comm->world : 1, rank = comm ? comm->rank : 0;
    ARGCHK(!g->halo_world || (g->halo_world == world && g->halo_rank == rank), "boundary-exchange shard of rank %d/%d used with rank %d/%d",
           g->halo_rank, g->halo_world, rank, world);
    ARGCHK(!comm || !comm->grp || !comm->grp->member[rank], "loopback rank %d already has a loop (one loop per rank and group)", rank);
    int64_t rb = 0, nr = 0;
    gnn_shard_range(g->N_global, rank, world, &rb, &nr);
    ARGCHK(rb == g->row_begin && nr == g->n_rows, "graph owns rows [%lld,+%lld) but rank %d/%d must own [%lld,+%lld)",
           (long long)g->row_begin, (long long)g->n_rows, rank, world, (long long)rb, (long long)nr);
    ARGCHK(!comm || comm->device == g->device, "communicator and graph live on different devices");

    HIPCHK(hipSetDevice(g->device));
    gnn_loop *l = new gnn_loop();
    if (comm) comm->loops++;                 // (gnn_loop_destroy, also on the failure paths below, gives it back)
    l->g = g; l->st = net_state; l->ou = net_output; l->comm = comm; l->device = g->device; l->rank = rank; l->world = world;
    l->D = state_dim; l->Ds = Ds; l->NLc = NLc; l->in_s = in_s; l->wf = Ds + NLc; l->T = net_output->dims.back();
    l->max_iter = max_iter; l->thr = threshold;
    l->edge_expected = edge_width;
    l->shard_rows = ((g->N_global + world - 1) / world + 31) / 32 * 32;
    l->N_pad = g->halo_world ? g->N : l->shard_rows * world;                  // rows of the state replica
    l->own_off = g->halo_world ? 0 : l->shard_rows * rank;
    int rc = 0;
    if (comm) l->stream = comm->stream;
    else {
        hipError_t e = hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { gnn_loop_destroy(l); return gnn_fail(GNN_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    }
    int maxw_s = 1, maxw_o = 1;
    for (int i = 1; i <= net_state->n_layers; ++i) maxw_s = std::max(maxw_s, net_state->dims[i]);
    for (int i = 1; i <= net_output->n_layers; ++i) maxw_o = std::max(maxw_o, net_output->dims[i]);
    for (int b = 0; b < 2 && !rc; ++b) {
        rc = dev_alloc(&l->state[b], (size_t)l->N_pad * Ds);
        if (!rc) rc = zero_on_stream(l->state[b], sizeof(float) * (size_t)l->N_pad * Ds, l->stream);      // ordered before everything this loop ever queues
    }
    // gate words, then one ticket counter per body (the second half is spare: a partial last tile used to get a launch of its own) in the
    // same block, so that loop_begin clears both with one fill; + barrier counter / status of the persistent loop
    if (!rc) rc = dev_alloc(&l->flags, loop_flag_words(l) + loop_ctr_words(l) + 4);
    if (!rc) l->tile_ctr = l->flags + loop_flag_words(l);
    if (!rc) rc = dev_alloc(&l->kfinal_dev, 4);        // k, status word of the persistent loop, "gate not certified", pad
    if (!rc && hipHostMalloc((void **)&l->kfinal_host, 4 * sizeof(int)) != hipSuccess) rc = gnn_fail(GNN_ERR_HIP, "hipHostMalloc");
    if (!rc) l->kfinal_host[1] = l->kfinal_host[2] = l->kfinal_host[3] = 0;
    if (!rc && hipHostMalloc((void **)&l->gate_host, sizeof(int) * (size_t)world * GNN_FLAG_WORDS) != hipSuccess) rc = gnn_fail(GNN_ERR_HIP, "hipHostMalloc");
    if (!edge_width) {      // the edge-based buffers are sized in gnn_loop_set_edge_readout
        if (!rc) rc = dev_alloc(&l->feats, (size_t)g->n_masked * l->wf);
        if (!rc) rc = dev_alloc(&l->out, (size_t)g->n_masked * l->T);
        for (int b = 0; b < 2 && !rc; ++b) rc = dev_alloc(&l->otmp[b], (size_t)g->n_masked * maxw_o);
    }
    if (!rc && hipEventCreateWithFlags(&l->ev_gate, hipEventDisableTiming) != hipSuccess) rc = gnn_fail(GNN_ERR_HIP, "hipEventCreate");
    if (!rc && hipEventCreate(&l->ev_total[0]) != hipSuccess) rc = gnn_fail(GNN_ERR_HIP, "hipEventCreate");
    if (!rc && hipEventCreate(&l->ev_total[1]) != hipSuccess) rc = gnn_fail(GNN_ERR_HIP, "hipEventCreate");
    if (rc) { gnn_loop_destroy(l); return rc; }
    l->impl_req = 2;            // fastest supported path by default; gnn_loop_set_impl(1) selects the bit-exact f32 MFMA
    (void)maxw_s;
    if (comm && comm->grp) comm->grp->member[rank] = l;
    *out = l;
    return GNN_OK;
}

static int loop_ensure_unfused(gnn_loop *l)
{
    if (l->inp) return GNN_OK;
    int maxw = 1;
    for (int i = 1; i <= l->st->n_layers; ++i) maxw = std::max(maxw, l->st->dims[i]);
    int rc = dev_alloc(&l->inp, (size_t)l->g->n_rows * l->in_s);
    for (int b = 0; b < 2 && !rc; ++b) rc = dev_alloc(&l->tmp[b], (size_t)l->g->n_rows * maxw);
    return rc;
}

extern "C" int gnn_loop_set_impl(gnn_loop *l, int impl, int *used)
{
    ARGCHK(l && impl >= 0 && impl <= 2, "impl must be 0 (unfused), 1 (fused, exact f32 MFMA) or 2 (fused, split bf16 MFMA)");
    l->impl_req = impl;
    const int rc = gnn_loop_decide_form(l);
    if (used) *used = gnn_loop_impl_used(l);
    return rc;
}

extern "C" int gnn_loop_set_pieces(gnn_loop *l, int pieces, int *used)
{
    ARGCHK(l && (pieces == 2 || pieces == 3), "pieces must be 2 (fp16 x 2) or 3 (bf16 x 3)");
    l->pieces = pieces;
    if (used) *used = pieces;
    return GNN_OK;
}

extern "C" int gnn_loop_range_info(const gnn_loop *l, int *last_run_repeated, int *repeats_total)
{
    ARGCHK(l, "loop is NULL");
    if (last_run_repeated) *last_run_repeated = l->last_run_range_rerun ? 1 : 0;
    if (repeats_total) *repeats_total = l->range_reruns;
    return GNN_OK;
}

extern "C" int gnn_loop_gate_info(const gnn_loop *l, int *last_run_repeated, int *repeats_total)
{
    ARGCHK(l, "loop is NULL");
    if (last_run_repeated) *last_run_repeated = l->last_run_rerun ? 1 : 0;
    if (repeats_total) *repeats_total = l->certified_reruns;
    return GNN_OK;
}

// forget the loop-invariant label aggregates (GNN.py:259, :263) kept from the previous run: the next run rebuilds them, as every
// Loop() call of the reference does
extern "C" int gnn_loop_drop_cached_aggregates(gnn_loop *l)
{
    ARGCHK(l, "loop is NULL");
    l->inv_version = 0;
    l->proj_labels = 0;         // the label projection is built from the block
    return GNN_OK;
}

// Label projection (include/gnn_hip.h): layer 0 of net_state split by rows of its kernel - the label terms inv . W1_label + b1 once per
// Loop (gnn_label_project.hip), every body's layer 0 over [state | aggregated state] only, started from them (seeded kernels, gnn_fused_ps*.hip)
extern "C" int gnn_loop_set_label_projection(gnn_loop *l, int mode, int *used)
{
    ARGCHK(l && mode >= 0 && mode <= 2, "mode must be 0 (off), 1 (where the fused path needs it) or 2 (wherever applicable)");
    l->label_projection = mode;
    const int rc = gnn_loop_decide_form(l);
    if (used) *used = l->form.path == GNN_PATH_BODIES && l->form.seeded ? 1 : 0;
    return rc;
}

// Wide-state form (include/gnn_hip.h): one launch per body for a net_state whose tile of eight waves does not fit one workgroup's LDS -
// k_fused_generic on 4 to 7 waves (gnn_fused.hip, wide_waves)
extern "C" int gnn_loop_set_wide_state(gnn_loop *l, int mode, int *used)
{
    ARGCHK(l && mode >= 0 && mode <= 2, "mode must be 0 (off), 1 (where it is faster than one kernel per op) or 2 (wherever covered)");
    l->wide_state = mode;
    const int rc = gnn_loop_decide_form(l);
    if (used) *used = l->form.path == GNN_PATH_BODIES && l->form.wide ? 1 : 0;
    return rc;
}

// test entry point: the tile loader of the wide-state form's full tiles - 0 load_tile_wide (the default), 1 load_tile_generic
extern "C" int gnn_loop_set_wide_loader(gnn_loop *l, int loader, int *used)
{
    ARGCHK(l && (loader == 0 || loader == 1), "loader must be 0 (load_tile_wide) or 1 (load_tile_generic)");
    l->wide_loader = loader;
    const int rc = gnn_loop_decide_form(l);
    if (used) *used = l->form.path == GNN_PATH_BODIES && l->form.wide && (l->form.args.variant & 8) ? 1 : 0;      // load_tile_wide in use
    return rc;
}

// test entry point: {waves per workgroup, grid} of the launch per body of the last form decision - a setter's or a run's ({0, 0}: no such launch)
extern "C" int gnn_loop_body_launch(const gnn_loop *l, int *out)
{
    ARGCHK(l && out, "bad arguments");
    const bool bodies = l->form.path == GNN_PATH_BODIES;
    out[0] = bodies ? l->form.waves : 0;
    out[1] = bodies ? (int)l->form.grid : 0;
    return GNN_OK;
}

// test entry point: at most max_workgroups workgroups per k_fused_generic launch (0: the library's choice)
extern "C" int gnn_loop_set_grid_limit(gnn_loop *l, int max_workgroups, int *used)
{
    ARGCHK(l && max_workgroups >= 0, "max_workgroups must be >= 0");
    l->grid_limit = max_workgroups;
    const int rc = gnn_loop_decide_form(l);
    if (used) *used = l->form.path == GNN_PATH_BODIES ? (int)l->form.grid : 0;
    return rc;
}

// test hook: the projection the last run used, P [n_rows, H1] row-major (H1: width of net_state's first layer)
extern "C" int gnn_loop_get_label_projection(gnn_loop *l, float *out)
{
    ARGCHK(l && out, "bad arguments");
    if (!l->ran || !l->form.seeded || !l->proj || l->proj_labels != l->g->label_version || l->proj_weights != l->st->version)
        return gnn_fail(GNN_ERR_STATE, "the last run of this loop did not use a label projection");
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipStreamSynchronize(l->stream));
    std::vector<float> host(l->proj_floats);
    HIPCHK(hipMemcpy(host.data(), l->proj, host.size() * sizeof(float), hipMemcpyDeviceToHost));
    const int h1 = l->st->dims[1], nt = l->proj_nt;
    for (int64_t i = 0; i < l->g->n_rows; ++i)
        for (int j = 0; j < h1; ++j) {
            // tile order [row tile][feature tile][q][lane = 32 half + node][4]: feature 32 jt + 8 q + 4 half + e (GnnFusedArgs::seed)
            const int jt = j >> 5, q = (j >> 3) & 3, half = (j >> 2) & 1, e = j & 3;
            out[(size_t)i * h1 + j] = host[((((size_t)(i >> 5) * nt + jt) * 4 + q) * 64 + 32 * half + (i & 31)) * 4 + e];
        }
    return GNN_OK;
}

// small graphs run all bodies of a Loop inside one persistent launch (gnn_small_common.h); enable = 0 keeps to one launch per body
extern "C" int gnn_loop_set_persistent(gnn_loop *l, int enable, int *used)
{
    ARGCHK(l, "loop is NULL");
    l->small_disabled = enable == 0;
    const int rc = gnn_loop_decide_form(l);
    if (used) *used = l->form.path == GNN_PATH_PERSISTENT ? 1 : 0;
    return rc;
}

extern "C" int gnn_loop_set_tile_form(gnn_loop *l, int form, int *used)
{
    ARGCHK(l && form >= 0 && form <= 2, "form must be 0 (library's choice), 1 (one wave per tile) or 2 (wave pair per tile)");
    l->tile_form = form;
    const int rc = gnn_loop_decide_form(l);
    if (used) *used = l->form.path == GNN_PATH_UNFUSED ? 0 : (l->form.kernel == GNN_BODY_PAIR ? 2 : 1);
    return rc;
}

extern "C" int gnn_loop_body_kernel(gnn_loop *l, int *kernel)
{
    ARGCHK(l && kernel, "bad arguments");
    const int rc = gnn_loop_decide_form(l);
    *kernel = l->form.path == GNN_PATH_UNFUSED ? 0 : l->form.kernel + 1;
    return rc;
}

extern "C" int gnn_loop_set_gather_form(gnn_loop *l, int form, int *used)
{
    ARGCHK(l && form >= 0 && form <= 2, "form must be 0 (library's choice), 1 (walk the CSR) or 2 (the graph's gather program)");
    l->gather_form = form;
    const int rc = gnn_loop_decide_form(l);
    if (used) *used = l->form.path == GNN_PATH_UNFUSED ? 0 : (l->form.program ? 2 : 1);
    return rc;
}

extern "C" int gnn_loop_set_tile_schedule(gnn_loop *l, int kind, int *used)
{
    ARGCHK(l && kind >= 0 && kind <= 2, "kind must be 0 (library's choice), 1 (ascending tile order) or 2 (balanced tile order)");
    l->tile_schedule = kind;
    const int rc = gnn_loop_decide_form(l);
    if (used) *used = l->form.path != GNN_PATH_UNFUSED && l->form.program ? l->form.schedule : 0;
    return rc;
}

extern "C" int gnn_loop_set_profiling(gnn_loop *l, int enable)
{
    ARGCHK(l, "loop is NULL");
    l->profiling = enable != 0;
    return GNN_OK;
}

extern "C" int gnn_loop_get_timing(const gnn_loop *l, float *total_ms, float *avg_iter_ms, int *n_iter_timed)
{
    ARGCHK(l, "loop is NULL");
    if (!l->ran) return gnn_fail(GNN_ERR_STATE, "gnn_loop_run has not been called");
    if (total_ms) *total_ms = l->total_ms;
    if (avg_iter_ms) *avg_iter_ms = l->avg_iter_ms;
    if (n_iter_timed) *n_iter_timed = l->n_iter_timed;
    return GNN_OK;
}

extern "C" int gnn_loop_get_exchange_timing(const gnn_loop *l, float *avg_between_bodies_ms)
{
    ARGCHK(l && avg_between_bodies_ms, "bad arguments");
    if (!l->ran) return gnn_fail(GNN_ERR_STATE, "gnn_loop_run has not been called");
    *avg_between_bodies_ms = l->avg_gap_ms;
    return GNN_OK;
}

extern "C" int gnn_counters_get(const gnn_loop *l, double *bytes_per_iteration, double *flops_per_iteration, int *iterations, float *total_ms,
                                float *avg_iteration_ms)
{
    ARGCHK(l, "loop is NULL");
    const gnn_graph *g = l->g;
    const double n = (double)g->n_rows, e = (double)g->E, ds = (double)l->Ds;
    if (bytes_per_iteration) *bytes_per_iteration = e * (4.0 * ds + 8.0) + 4.0 * (n + 1.0) + n * (8.0 * ds + 4.0 * (2.0 * l->NLc + g->AL));
    if (flops_per_iteration) {
        double f = 0.0;
        for (int i = 0; i < l->st->n_layers; ++i) f += 2.0 * (double)l->st->dims[i] * (double)l->st->dims[i + 1];
        *flops_per_iteration = n * f + 2.0 * e * ds;
    }
    if (iterations) *iterations = l->ran ? l->kfinal : 0;
    if (total_ms) *total_ms = l->ran ? l->total_ms : 0.f;
    if (avg_iteration_ms) *avg_iteration_ms = l->ran ? l->avg_iter_ms : 0.f;
    return GNN_OK;
}

extern "C" int gnn_loop_set_state0(gnn_loop *l, const float *state0, uint64_t seed)
{
    ARGCHK(l, "loop is NULL");
    HIPCHK(hipSetDevice(l->device));
    const gnn_graph *g = l->g;
    const size_t cnt = (size_t)g->n_rows * l->Ds;
    if (!l->state_init && l->D) {
        // One GPU: a drop-in table for body 0's gather (loop_begin) - the replica's padded row count, the tail zeroed once and never written again.
        const size_t rows = l->world == 1 ? (size_t)std::max<int64_t>(l->N_pad, g->n_rows) : (size_t)g->n_rows;
        int rc = dev_alloc(&l->state_init, rows * l->Ds);
        if (!rc && rows > (size_t)g->n_rows) rc = zero_on_stream(l->state_init + cnt, sizeof(float) * (rows - (size_t)g->n_rows) * l->Ds, l->stream);
        if (rc) return rc;
    }
    float *own = l->state_init;
    if (l->D == 0) {   // state <- node labels (GNN.py:265); taken from the graph at run time
        l->have_state0 = true;
        return GNN_OK;
    }
    if (state0) {
        HIPCHK(hipMemcpyAsync(own, state0, cnt * sizeof(float), hipMemcpyHostToDevice, l->stream));
        HIPCHK(hipStreamSynchronize(l->stream));
    } else if (cnt) {
        hipLaunchKernelGGL(k_randn, cdiv((int64_t)cnt, 256), 256, 0, l->stream, (int64_t)cnt, (int64_t)g->row_begin * l->Ds, seed, 0.1f, own);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(l->stream));
    }
    l->have_state0 = true;
    return GNN_OK;
}

extern "C" int gnn_loop_set_slice_exchange(gnn_loop *l, int on)
{
    ARGCHK(l, "loop is NULL");
    if (!on) { l->slice_mode = false; return GNN_OK; }
    ARGCHK(l->world > 1, "the feature-sliced exchange needs a communicator");
    ARGCHK(l->Ds % l->world == 0, "state width %d is not a multiple of the world size %d", l->Ds, l->world);
    ARGCHK(l->g->sh->full_indptr, "call gnn_graph_set_full_adjacency first (on this graph or on the graph it was derived from)");
    ARGCHK(!l->g->halo_world, "not on a boundary-exchange shard");
    HIPCHK(hipSetDevice(l->device));
    l->Cs = l->Ds / l->world;
    if (!l->sl_send) {
        const size_t slice = (size_t)l->N_pad * l->Cs;           // == world * shard_rows * Cs
        int rc = dev_alloc(&l->sl_send, slice);
        if (!rc) rc = dev_alloc(&l->sl_state, slice);
        if (!rc) rc = dev_alloc(&l->sl_agg, slice);
        if (!rc) rc = dev_alloc(&l->sl_recv, slice);
        if (!rc) rc = dev_alloc(&l->agg_own, (size_t)l->shard_rows * l->Ds);
        if (rc) return rc;
        if ((rc = zero_on_stream(l->sl_agg, sizeof(float) * std::max<size_t>(slice, 1), l->stream))) return rc;      // rows past N_global are never written
        // rows past n_rows of a short shard are never written either (k_slice_unpack), and the full-tile kernel copies all 32 rows of its last
        // tile (load_tile_given64): layer 0 cuts them, and the fp16 range guard reads what it cuts - stale values there repeated Loops at random
        if ((rc = zero_on_stream(l->agg_own, sizeof(float) * std::max<size_t>((size_t)l->shard_rows * l->Ds, 1), l->stream))) return rc;
    }
    l->slice_mode = true;
    l->sl_pipeline = on != 2;          // 2: the whole slice is aggregated, then one grouped all-to-all (round-2 form; kept for comparison)
    return GNN_OK;
}

static int unfused_iteration(gnn_loop *l, int k)
{
    const gnn_graph *g = l->g;
    const int cur = k & 1, nxt = cur ^ 1, P = l->world;
    const int *gate = l->flags + (size_t)k * P * GNN_FLAG_WORDS;
    const float *rep_cur = gnn_loop_state_after(l, k, 0), *own_cur = rep_cur + (size_t)l->own_off * l->Ds;
    float *own_nxt = l->state[nxt] + (size_t)l->own_off * l->Ds;
    // node_components (GNN.py:228): own state into columns [0, Ds) of the concat
    int rc = gnn_launch_copy_cols(l->stream, g->n_rows, l->Ds, own_cur, l->Ds, l->inp, l->in_s, gate, P);
    if (rc) return rc;
    // aggregated_states (GNN.py:234) into columns [Ds + NLc, +Ds)
    if (l->slice_mode) rc = gnn_launch_copy_cols(l->stream, g->n_rows, l->Ds, l->agg_own, l->Ds, l->inp + l->Ds + l->NLc, l->in_s, gate, P);
    else rc = gnn_launch_spmm(l->stream, g->n_rows, g->sh->indptr, g->sh->adj_src, g->sh->adj_w, rep_cur, l->Ds, l->Ds,
                              l->inp + l->Ds + l->NLc, l->in_s, gate, P);
    if (rc) return rc;
    // net_state (GNN.py:240)
    rc = launch_mlp(l->stream, l->st, g->n_rows, l->inp, l->in_s, own_nxt, l->Ds, l->tmp[0], l->tmp[1], gate, P);
    if (rc) return rc;
    // condition for the next body (GNN.py:206-218)
    return launch_check(l->stream, g->n_rows, l->Ds, own_nxt, own_cur, l->thr, l->flags + ((size_t)(k + 1) * P + l->rank) * GNN_FLAG_WORDS, gate, P);
}

// ---- phases of one Loop; gnn_loop_run runs them for one rank, gnn_loop_run_group rank by rank for a loopback group ----------
// state <- initial state, first condition against ones (GNN.py:262-271), loop-invariant aggregates (GNN.py:259, :263)
static int loop_begin(gnn_loop *l)
{
    gnn_graph *g = l->g;
    const int P = l->world;
    hipStream_t st = l->stream;
    int rc = 0;
    HIPCHK(hipMemsetAsync(l->flags, 0, sizeof(int) * (loop_flag_words(l) + loop_ctr_words(l)), st));      // gate words and tile counters, one fill
    l->small_words_clean = false;       // the persistent loop's gate words share this block
    // One GPU, D > 0: body 0 gathers from state_init itself (a table of N_pad rows, gnn_loop_set_state0) and writes state[1]; no run writes
    // state_init.  Shards exchange rows inside state[0], and with D == 0 the initial state is the unpadded label table: those keep the copy.
    l->init_in_place = P == 1 && !l->comm && l->D > 0 && !l->slice_mode && !g->halo_world && l->own_off == 0;
    float *own0 = l->state[0] + (size_t)l->own_off * l->Ds;
    if (g->n_rows && !l->init_in_place)   // state <- nodes (GNN.py:265) or the injected / drawn initial state (GNN.py:262)
        HIPCHK(hipMemcpyAsync(own0, l->D ? l->state_init : g->nodes + (size_t)g->own_off * g->NL,
                              sizeof(float) * (size_t)g->n_rows * l->Ds, hipMemcpyDeviceToDevice, st));
    // first condition: state vs ones (GNN.py:266, :271)
    if ((rc = launch_check_first(st, g->n_rows, l->Ds, gnn_loop_state_after(l, 0, (size_t)l->own_off), l->thr, l->flags + (size_t)l->rank * GNN_FLAG_WORDS))) return rc;
    if (l->form.path == GNN_PATH_UNFUSED) {
        const int c_nodes = l->Ds, c_aggn = l->Ds + l->NLc + l->Ds, c_agga = c_aggn + l->NLc;
        rc = gnn_launch_spmm(st, g->n_rows, g->sh->indptr, nullptr, g->sh->arc_w, gnn_graph_arc_labels(g), g->AL, g->AL, l->inp + c_agga, l->in_s, nullptr, 1);
        if (rc) return rc;
        if (l->D) {
            rc = gnn_launch_spmm(st, g->n_rows, g->sh->indptr, g->sh->adj_src, g->sh->adj_w, g->nodes, g->NL, g->NL, l->inp + c_aggn, l->in_s, nullptr, 1);
            if (rc) return rc;
            rc = gnn_launch_copy_cols(st, g->n_rows, g->NL, g->nodes + (size_t)g->own_off * g->NL, g->NL, l->inp + c_nodes, l->in_s, nullptr, 1);
            if (rc) return rc;
        }
    }
    return GNN_OK;
}

static int loop_body(gnn_loop *l, int k)
{
    if (l->profiling) HIPCHK(hipEventRecord(l->ev[2 * k], l->stream));
    int rc = l->form.path == GNN_PATH_UNFUSED ? unfused_iteration(l, k) : gnn_fused_iteration(l, k);
    if (rc) return rc;
    if (l->profiling) HIPCHK(hipEventRecord(l->ev[2 * k + 1], l->stream));
    return GNN_OK;
}

// gate of body k -> host, in two steps, so that further bodies can be queued behind the copy before the host waits for it; every rank
// reads the same exchanged gate, so all ranks stop at the same body
static int loop_gate_fetch(gnn_loop *l, int k)
{
    const size_t words = (size_t)l->world * GNN_FLAG_WORDS;
    HIPCHK(hipMemcpyAsync(l->gate_host, l->flags + (size_t)k * words, sizeof(int) * words, hipMemcpyDeviceToHost, l->stream));
    HIPCHK(hipEventRecord(l->ev_gate, l->stream));
    return GNN_OK;
}

static int loop_gate_closed(gnn_loop *l, bool *closed)
{
    const size_t words = (size_t)l->world * GNN_FLAG_WORDS;
    HIPCHK(hipEventSynchronize(l->ev_gate));
    int any = 0;
    for (size_t i = 0; i < words; i += GNN_FLAG_STRIDE) any |= l->gate_host[i];
    *closed = !any;
    return GNN_OK;
}

// k, apply_filters + net_output on the owned masked rows (GNN.py:275-279)
static int loop_finish(gnn_loop *l)
{
    gnn_graph *g = l->g;
    hipStream_t st = l->stream;
    int rc = 0;
    const bool persistent = l->form.path == GNN_PATH_PERSISTENT, output_done = persistent && l->form.fold_output;
    if (!persistent) {     // (the persistent small-graph loop has written k itself)
        hipLaunchKernelGGL(k_finalize, 1, 64, 0, st, l->flags, l->world, l->max_iter, l->kfinal_dev);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(l->kfinal_host, l->kfinal_dev, 4 * sizeof(int), hipMemcpyDeviceToHost, st));      // k, 0, "a gate was not certified", "out of fp16 range"
    }
    if (output_done) return GNN_OK;     // (the persistent loop wrote k into the pinned host words and ran the output stage itself)
    const GnnStateTabs own = gnn_loop_state_tabs(l, (size_t)l->own_off);
    const float *nodes_own = g->nodes + (size_t)g->own_off * g->NL;

    if (l->edge_mode) {      // GNNedgeBased.apply_filters + net_output on the masked arcs (GNN.py:289-302, :279)
        if (l->n_edge_masked) {
            const int we = l->ou->dims[0];
            const int64_t tot = l->n_edge_masked * we;
            hipLaunchKernelGGL(k_feats_edge, cdiv(tot, 256), 256, 0, st, l->n_edge_masked, l->edge_rows, l->edge_dst, g->sh->adj_src, gnn_loop_state_tabs(l, 0),
                               l->kfinal_dev, l->Ds, g->nodes, g->NL, l->NLc, g->arc_labels_orig_own ? g->arc_labels_orig_own : l->edge_labels, g->AL, l->feats, l->own_off);
            HIPCHK(hipGetLastError());
            rc = launch_mlp(st, l->ou, l->n_edge_masked, l->feats, we, l->out, l->T, l->otmp[0], l->otmp[1], nullptr, 1);
            if (rc) return rc;
        }
        return GNN_OK;
    }
    // (the conditions of the fused output stage are those of its first form, whose block also held W and the outputs in LDS; the tile of this one is never larger than 64 KB under them)
    const size_t out1_cond = sizeof(float) * ((size_t)(l->wf + 1) * l->T + (size_t)GNN_OUT1_ROWS * (l->wf | 1) + (size_t)GNN_OUT1_ROWS * l->T);
    const int ld = out1_ld(l->wf);
    const size_t out1_lds = sizeof(float) * GNN_OUT1_ROWS * ((size_t)ld + 1);
    if (g->n_masked && l->ou->n_layers == 1 && l->T <= 8 && out1_cond <= 64 * 1024 && out1_lds <= 64 * 1024) {
        const gnn_mlp *ou = l->ou;
#define GNN_OUT1_LAUNCH(T_)                                                                                                                        \
    case T_:                                                                                                                                       \
        hipLaunchKernelGGL(k_out1<T_>, cdiv(g->n_masked, GNN_OUT1_ROWS), GNN_OUT1_ROWS, out1_lds, st, g->n_masked, g->sh->masked_rows, own,       \
                           l->kfinal_dev, l->Ds, nodes_own, g->NL, l->NLc, ld, ou->W[0], ou->b[0], ou->acts[0],                                    \
                           ou->has_bn ? ou->bn_scale : (const float *)nullptr, ou->has_bn ? ou->bn_shift : (const float *)nullptr, l->out);        \
        break;
        switch (l->T) {
            GNN_OUT1_LAUNCH(1) GNN_OUT1_LAUNCH(2) GNN_OUT1_LAUNCH(3) GNN_OUT1_LAUNCH(4) GNN_OUT1_LAUNCH(5) GNN_OUT1_LAUNCH(6) GNN_OUT1_LAUNCH(7) GNN_OUT1_LAUNCH(8)
        default: return gnn_fail(GNN_ERR_UNSUPPORTED, "no output-stage instantiation for %d outputs", l->T);
        }
#undef GNN_OUT1_LAUNCH
        HIPCHK(hipGetLastError());
    } else if (g->n_masked) {
        const int64_t tot = g->n_masked * l->wf;
        hipLaunchKernelGGL(k_feats, cdiv(tot, 256), 256, 0, st, g->n_masked, g->sh->masked_rows, own, l->kfinal_dev, l->Ds, nodes_own, g->NL, l->NLc, l->feats);
        HIPCHK(hipGetLastError());
        rc = launch_mlp(st, l->ou, g->n_masked, l->feats, l->wf, l->out, l->T, l->otmp[0], l->otmp[1], nullptr, 1);
        if (rc) return rc;
    }
    return GNN_OK;
}

static int loop_prepare(gnn_loop *l)
{
    if (!l->have_state0) {
        if (l->D == 0) l->have_state0 = true;
        else return gnn_fail(GNN_ERR_STATE, "state_vect_dim > 0: call gnn_loop_set_state0 first");
    }
    if (l->edge_expected && !l->edge_mode)
        return gnn_fail(GNN_ERR_STATE, "net_output has the edge-based input width: call gnn_loop_set_edge_readout first");
    HIPCHK(hipSetDevice(l->device));
    l->ng_inlaunch = false;          // (set again by gnn_small_run when its form folds the graph readout into the launch)
    l->init_in_place = false;        // (set again by loop_begin when this run's body 0 reads state_init itself)
    ++l->out_runs;                   // this run rewrites l->out: a readout folded into an earlier launch is stale from here on
    if (!l->graph_ready_seen) {      // a derived graph's creation-time fills (gnn_graph_derive) come before the first read of its labels
        int rcw = gnn_graph_wait_ready(l->g, l->stream);
        if (rcw) return rcw;
        l->graph_ready_seen = true;
    }
    int rc = gnn_loop_decide_form(l);           // afresh for every run: any of its inputs may have changed since the last one
    if (!rc) rc = l->form.path == GNN_PATH_UNFUSED ? loop_ensure_unfused(l) : gnn_fused_prepare(l);
    if (rc) return rc;
    if (l->profiling && (int)l->ev.size() < 2 * l->max_iter) {
        const size_t old = l->ev.size();
        l->ev.resize(2 * (size_t)l->max_iter, nullptr);
        for (size_t i = old; i < l->ev.size(); ++i) HIPCHK(hipEventCreate(&l->ev[i]));
    }
    return GNN_OK;
}

static int loop_collect(gnn_loop *l, float *k_out)
{
    l->kfinal = *l->kfinal_host;
    l->ran = true;
    l->total_ms = 0.f;
    if (l->profiling) HIPCHK(hipEventElapsedTime(&l->total_ms, l->ev_total[0], l->ev_total[1]));
    l->avg_iter_ms = 0.f;
    l->n_iter_timed = 0;
    if (l->profiling) {
        double sum = 0;
        for (int k = 0; k < l->kfinal; ++k) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, l->ev[2 * k], l->ev[2 * k + 1]));
            sum += ms;
        }
        l->n_iter_timed = l->kfinal;
        l->avg_iter_ms = l->kfinal ? (float)(sum / l->kfinal) : 0.f;
        // what sits between two bodies on the stream: the exchange of the sharded layouts (all-gather of rows / boundary rows + flags, or
        // pack -> all-to-all -> slice aggregation -> all-to-all -> unpack), a few microseconds of launch gap on a single GPU
        double gap = 0;
        for (int k = 0; k + 1 < l->kfinal; ++k) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, l->ev[2 * k + 1], l->ev[2 * k + 2]));
            gap += ms;
        }
        l->avg_gap_ms = l->kfinal > 1 ? (float)(gap / (l->kfinal - 1)) : 0.f;
    }
    if (k_out) *k_out = (float)l->kfinal;
    return GNN_OK;
}

// Everything the ranks in `ls` put on their streams for one Loop, and the wait for it.  Bodies are enqueued without waiting for each
// other; every GNN_BODY_CHUNK bodies the gate of the next body is copied to the host and checked, so that a loop that converged
// does not pay for max_iteration - k empty launches (about 3 us each).  The host looks at the copy only GNN_BODY_LOOKAHEAD bodies later:
// those are queued behind it first, so the stream does not run dry while the host wakes up (behind a closed gate they return at once, and
// k comes from the gate words: k_finalize).  n == 1: one rank of an RCCL job (or a single GPU);
// n == world: all ranks of a loopback group, stepped phase by phase on the group's stream.  The path of every rank is its form's
// (the persistent path only exists for world == 1, i.e. n == 1).
static int run_loops_once(gnn_loop **ls, int n)
{
    int rc = 0;
    for (int r = 0; r < n; ++r) if ((rc = loop_prepare(ls[r]))) return rc;
    if (ls[0]->form.path == GNN_PATH_PERSISTENT) {
        // small graphs: the initial state, the first condition and every body inside ONE persistent launch (gnn_small_kernel.h)
        if ((rc = gnn_small_run(ls[0]))) return rc;             // (never a profiled run: no event to record)
    } else {
        const int max_iter = ls[0]->max_iter;
        for (int r = 0; r < n; ++r) {
            if (ls[r]->profiling) HIPCHK(hipEventRecord(ls[r]->ev_total[0], ls[r]->stream));
            if ((rc = loop_begin(ls[r]))) return rc;
        }
        // (feature-sliced exchange: no rank ever needs another rank's state rows, only the gates travel)
        for (int r = 0; r < n; ++r) if ((rc = loop_exchange(ls[r], ls[r]->slice_mode ? -1 : 0, 0))) return rc;
        int fetched = -1;       // the body whose gate is on its way to the host
        for (int k = 0; k < max_iter; ++k) {
            if (fetched >= 0 && k == fetched + GNN_BODY_LOOKAHEAD) {
                bool closed = false, c = false;
                for (int r = 0; r < n; ++r) {
                    if ((rc = loop_gate_closed(ls[r], &c))) return rc;
                    if (r == 0) closed = c;
                    else if (c != closed) return gnn_fail(GNN_ERR_STATE, "ranks disagree on the gate of body %d", fetched);
                }
                if (closed) break;
                fetched = -1;
            }
            if (ls[0]->slice_mode) {
                for (int r = 0; r < n; ++r) if ((rc = slice_step_pack(ls[r], k))) return rc;
                for (int r = 0; r < n; ++r) if ((rc = slice_step_aggregate(ls[r], k))) return rc;
                for (int r = 0; r < n; ++r) if ((rc = slice_step_unpack(ls[r], k))) return rc;
            }
            for (int r = 0; r < n; ++r) if ((rc = loop_body(ls[r], k))) return rc;
            for (int r = 0; r < n; ++r)
                if ((rc = loop_exchange(ls[r], ls[r]->slice_mode ? -1 : (k & 1) ^ 1, (size_t)(k + 1) * ls[r]->world * GNN_FLAG_WORDS))) return rc;
            if ((k + 1) % GNN_BODY_CHUNK == 0 && k + 1 < max_iter) {
                for (int r = 0; r < n; ++r) if ((rc = loop_gate_fetch(ls[r], k + 1))) return rc;
                fetched = k + 1;
            }
        }
    }
    for (int r = 0; r < n; ++r) {
        if ((rc = loop_finish(ls[r]))) return rc;
        if (ls[r]->profiling) HIPCHK(hipEventRecord(ls[r]->ev_total[1], ls[r]->stream));
    }
    for (int r = 0; r < n; ++r) HIPCHK(hipStreamSynchronize(ls[r]->stream));
    return GNN_OK;
}

// One Loop and the re-run policy around it: what the finished run left in kfinal_host[1..3] can send the Loop round again, on other settings.
static int run_loops(gnn_loop **ls, int n, float *k_out)
{
    int rc = run_loops_once(ls, n);
    if (rc) return rc;
    const LoopForm &form = ls[0]->form;         // of the run that just finished
    if (form.path == GNN_PATH_PERSISTENT && ls[0]->kfinal_host[1] != 0) {       // a barrier spin gave up (grid not resident?): repeat with one launch per body
        ls[0]->ng_inlaunch = false;
        ls[0]->small_disabled = true;
        ls[0]->small_words_clean = false;
        return run_loops(ls, n, k_out);
    }
    // Certified gate (gnn_common.h): a gate of this impl-2 run was decided by a borderline node and no robust mover - its k is not
    // guaranteed to be the bit-exact chain's.  The Loop is repeated on impl 1 and THAT run's k / state / output are what the caller gets.
    // Every rank reads the same exchanged flag words, so all ranks of a sharded job take this branch together.
    for (int r = 0; r < n; ++r) ls[r]->last_run_rerun = ls[r]->last_run_range_rerun = false;
    // Range guard of the fp16-piece format: some body of this run cut an operand past the fp16 range (its results may hold infinities).  The
    // Loop is repeated in the bf16-piece format, which takes the whole fp32 range; that run applies the certified gate below itself.  The flag
    // words are exchanged like the gate words, so every rank takes this branch together.
    const bool split_bodies = form.path == GNN_PATH_BODIES && form.split;
    if (split_bodies && form.pieces == 2 && ls[0]->kfinal_host[3] != 0) {
        static bool told_range = false;
        if (!told_range && !getenv("GNN_QUIET")) {
            told_range = true;
            fprintf(stderr, "libgnn_hip: an activation of a default-path Loop left the range of the fp16-piece arithmetic: the Loop is repeated with bf16 "
                            "pieces (gnn_loop_range_info counts these)\n");
        }
        for (int r = 0; r < n; ++r) ls[r]->pieces = 3;
        rc = run_loops(ls, n, k_out);
        for (int r = 0; r < n; ++r) {
            ls[r]->pieces = 2;
            if (rc == GNN_OK) { ls[r]->last_run_range_rerun = true; ++ls[r]->range_reruns; }
        }
        return rc;
    }
    if (split_bodies && ls[0]->kfinal_host[2] != 0) {
        static bool told = false;       // once per process: the caller gets the exact path's results, at the exact path's price
        if (!told && !getenv("GNN_QUIET")) {
            told = true;
            fprintf(stderr, "libgnn_hip: a gate of a default-path Loop was decided by a borderline node (no robust mover): the Loop is repeated on the "
                            "bit-exact path and its k / state / output are returned (gnn_loop_gate_info counts these; gnn_loop_set_impl(l, 1) avoids the double run)\n");
        }
        for (int r = 0; r < n; ++r) ls[r]->impl_req = 1;
        rc = run_loops(ls, n, k_out);
        for (int r = 0; r < n; ++r) {
            ls[r]->impl_req = 2;
            if (rc == GNN_OK) { ls[r]->last_run_rerun = true; ++ls[r]->certified_reruns; }
        }
        return rc;
    }
    for (int r = 0; r < n; ++r) {
        float k = 0.f;
        if ((rc = loop_collect(ls[r], &k))) return rc;
        if (r && ls[r]->kfinal != ls[0]->kfinal) return gnn_fail(GNN_ERR_STATE, "ranks disagree on the iteration count (%d vs %d)", ls[r]->kfinal, ls[0]->kfinal);
        if (r == 0 && k_out) *k_out = k;
    }
    return GNN_OK;
}

extern "C" int gnn_loop_run(gnn_loop *l, int training, float *k_out)
{
    ARGCHK(l, "loop is NULL");
    if (training) return gnn_fail(GNN_ERR_UNSUPPORTED, "gnn_loop_run is the inference Loop; the training-mode Loop is gnn_loop_train_forward / gnn_loop_train_step");
    if (l->comm && l->comm->grp && l->world > 1)
        return gnn_fail(GNN_ERR_STATE, "this loop belongs to a loopback group of %d ranks: run all of them with gnn_loop_run_group", l->world);
    return run_loops(&l, 1, k_out);
}

// Several INDEPENDENT loops (batches of a dataset: reference GNN_BaseClass.py:165-189 evaluates them one after the other) in one call.
// Small graphs take the persistent one-launch path, and such a launch occupies a few dozen of the 256 CUs: all of them are queued, each on
// its own loop's stream, before the first is waited for, so that they run side by side; the others run one after the other (each
// fills the GPU by itself).  The results are those of n separate gnn_loop_run calls.
extern "C" int gnn_loop_run_many(gnn_loop **loops, int n, float *k_out /* [n] */)
{
    ARGCHK(loops && n >= 1 && k_out, "bad arguments");
    for (int i = 0; i < n; ++i) {
        ARGCHK(loops[i], "loop %d is NULL", i);
        ARGCHK(loops[i]->world == 1, "loop %d is one rank of a sharded job: gnn_loop_run / gnn_loop_run_group", i);
        for (int j = 0; j < i; ++j) ARGCHK(loops[j] != loops[i], "loop %d is listed twice", i);
    }
    std::vector<char> queued((size_t)n, 0), done((size_t)n, 0);
    int rc = 0;
    // (an error part-way: nothing queued is left running behind the caller's back - EVERY early return below goes through drain)
    auto drain = [&](int rc_) { for (int i = 0; i < n; ++i) if (queued[(size_t)i] && !done[(size_t)i]) (void)hipStreamSynchronize(loops[i]->stream); return rc_; };
    // Residency: the persistent launches synchronise through a grid barrier, so every workgroup of every launch in flight must be
    // resident at once.  A launch's workgroup is one wave with 10 - 40 KB of LDS: at least four fit on a CU; launches are queued side by
    // side only while their workgroups sum to no more than three per CU, then the queued ones are collected before the next is queued
    // (the barrier's spin time-out stays as the safety net, it is no longer the mechanism).
    // The wide form of k_small16 keeps the rule: its largest instantiations allocate 256 VGPRs + up to 72 AGPRs of the SIMD's 512, so such
    // a wave is alone on its SIMD and a CU holds four of them - one more than the cap - and even if every narrow workgroup in flight took a
    // SIMD of its own, 3 x CUs workgroups leave each of them one of the 4 x CUs SIMDs.  LDS: at most 16 x 100 + 4,920 words = 26 KB per
    // wide workgroup, six per 160 KB.
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, loops[0]->device) != hipSuccess || n_cu <= 0) n_cu = 64;
    const long cap = 3L * n_cu;
    long in_flight = 0;
    // wait for the queued launches and take their results; one whose barrier gave up runs again, alone, one launch per body
    auto collect = [&]() -> int {
        int first_rc = GNN_OK;
        for (int i = 0; i < n; ++i) {
            if (!queued[(size_t)i] || done[(size_t)i]) continue;
            gnn_loop *l = loops[i];
            hipError_t e = hipSetDevice(l->device);
            if (e == hipSuccess) e = hipStreamSynchronize(l->stream);
            done[(size_t)i] = 1;
            if (e != hipSuccess) { if (!first_rc) first_rc = gnn_fail(GNN_ERR_HIP, "hipStreamSynchronize -> %s", hipGetErrorString(e)); continue; }
            if (first_rc) continue;                  // (keep waiting for the others, report the first error)
            int r = GNN_OK;
            if (l->kfinal_host[1] != 0) {            // a barrier spin gave up: this one again, alone, one launch per body
                l->ng_inlaunch = false;
                l->small_disabled = true;
                l->small_words_clean = false;
                r = run_loops(&loops[i], 1, &k_out[i]);
                l->small_disabled = false;           // (alone it would have been resident: only this call falls back)
            } else r = loop_collect(l, &k_out[i]);
            if (r) first_rc = r;
        }
        in_flight = 0;
        return first_rc;
    };
    for (int i = 0; i < n; ++i) {
        gnn_loop *l = loops[i];
        if ((rc = loop_prepare(l))) return drain(rc);
        l->last_run_rerun = l->last_run_range_rerun = false;      // (the persistent path is exact arithmetic and never repeats; run_loops sets it for the others)
        if (l->form.path != GNN_PATH_PERSISTENT) continue;
        const long wgs = (long)((l->g->n_rows + 15) / 16);      // upper bound of the launch's grid (16- or 32-node tiles)
        if (in_flight && in_flight + wgs > cap && (rc = collect())) return drain(rc);
        if ((rc = gnn_small_run(l))) return drain(rc);
        queued[(size_t)i] = 1;
        in_flight += wgs;
        if ((rc = loop_finish(l))) return drain(rc);
    }
    for (int i = 0; i < n; ++i)
        if (!queued[(size_t)i] && (rc = run_loops(&loops[i], 1, &k_out[i]))) return drain(rc);
    if ((rc = collect())) return drain(rc);
    return GNN_OK;
}

extern "C" int gnn_loop_run_group(gnn_loop **loops, int n, float *k_out)
{
    ARGCHK(loops && n >= 1, "bad arguments");
    for (int r = 0; r < n; ++r) {
        ARGCHK(loops[r] && loops[r]->comm && loops[r]->comm->grp, "loops[%d] was not created on a loopback communicator", r);
        ARGCHK(loops[r]->comm->grp == loops[0]->comm->grp && loops[r]->world == n && loops[r]->rank == r, "loops must be the %d ranks of one loopback group, in rank order", n);
        ARGCHK(loops[r]->max_iter == loops[0]->max_iter && loops[r]->thr == loops[0]->thr && loops[r]->Ds == loops[0]->Ds, "ranks were configured differently");
        // the exchange protocol of the whole group follows rank 0: a rank on another layout / arithmetic would skip or misread an exchange
        ARGCHK(loops[r]->slice_mode == loops[0]->slice_mode && loops[r]->Cs == loops[0]->Cs && loops[r]->impl_req == loops[0]->impl_req &&
               (!loops[0]->slice_mode || loops[r]->sl_pipeline == loops[0]->sl_pipeline) &&
               (loops[r]->g->halo_world != 0) == (loops[0]->g->halo_world != 0),
               "rank %d uses another exchange layout or arithmetic (slice %d/%d, impl %d/%d) than rank 0", r, (int)loops[r]->slice_mode, (int)loops[0]->slice_mode,
               loops[r]->impl_req, loops[0]->impl_req);
    }
    return run_loops(loops, n, k_out);
}

extern "C" int gnn_loop_get_state(const gnn_loop *l, float *state_out)
{
    ARGCHK(l && state_out, "bad arguments");
    if (!l->ran) return gnn_fail(GNN_ERR_STATE, "gnn_loop_run has not been called");
    HIPCHK(hipSetDevice(l->device));
    const float *src = gnn_loop_state_after(l, l->kfinal, (size_t)l->own_off);
    HIPCHK(hipMemcpy(state_out, src, sizeof(float) * (size_t)l->g->n_rows * l->Ds, hipMemcpyDeviceToHost));
    return GNN_OK;
}

extern "C" int gnn_loop_get_output(const gnn_loop *l, float *out, int64_t *n_masked)
{
    ARGCHK(l, "loop is NULL");
    if (!l->ran) return gnn_fail(GNN_ERR_STATE, "gnn_loop_run has not been called");
    const int64_t m = l->edge_mode ? l->n_edge_masked : l->g->n_masked;
    if (n_masked) *n_masked = m;
    if (out && m) {
        HIPCHK(hipSetDevice(l->device));
        HIPCHK(hipMemcpy(out, l->out, sizeof(float) * (size_t)m * l->T, hipMemcpyDeviceToHost));
    }
    return GNN_OK;
}

extern "C" int gnn_loop_set_edge_readout(gnn_loop *l, const int32_t *entry_dst, const float *arc_labels, const uint8_t *arc_mask)
{
    ARGCHK(l && (l->g->E == 0 || (entry_dst && arc_mask && (arc_labels || l->g->AL == 0 || l->g->arc_labels_orig_own))), "bad arguments");
    ARGCHK(l->edge_expected, "net_output input width %d is not the edge-based 2 (NL + D) + AL", l->ou->dims[0]);
    // Sharded loops (round 3): a rank reads out the arcs of its OWN CSR rows - entry_dst are owned-row indices, the source endpoint is in
    // the replica's index space like every adj_src - so the per-rank outputs, in rank order, are the unsharded output.  (Training and
    // the arc-side LGNN relabelling stay single-GPU.)
    const gnn_graph *g = l->g;
    std::vector<int32_t> rows;
    for (int64_t e = 0; e < g->E; ++e) {
        ARGCHK(entry_dst[e] >= 0 && entry_dst[e] < g->n_rows, "entry_dst[%lld]=%d outside the %lld owned rows", (long long)e, entry_dst[e], (long long)g->n_rows);
        if (arc_mask[e]) rows.push_back((int32_t)e);
    }
    HIPCHK(hipSetDevice(l->device));
    (void)hipFree(l->edge_dst); (void)hipFree(l->edge_rows); (void)hipFree(l->edge_labels); (void)hipFree(l->edge_inc_ptr); (void)hipFree(l->edge_inc);
    (void)hipFree(l->feats); (void)hipFree(l->out); (void)hipFree(l->otmp[0]); (void)hipFree(l->otmp[1]);
    l->feats = l->out = l->otmp[0] = l->otmp[1] = nullptr;
    l->edge_dst = l->edge_rows = nullptr; l->edge_labels = nullptr; l->edge_inc_ptr = l->edge_inc = nullptr;
    l->n_edge_masked = (int64_t)rows.size();
    int maxw_o = 1;
    for (int i = 1; i <= l->ou->n_layers; ++i) maxw_o = std::max(maxw_o, l->ou->dims[i]);
    int rc = dev_upload(&l->edge_dst, entry_dst, (size_t)g->E);
    if (!rc) rc = dev_upload(&l->edge_rows, rows.data(), rows.size());
    if (!rc && !g->arc_labels_orig_own) rc = dev_upload(&l->edge_labels, arc_labels, (size_t)g->E * g->AL);   // derived graphs own theirs
    if (!rc && l->world == 1 && g->n_rows == g->N) {      // masked arcs by endpoint (ascending masked-arc index): what the (single-GPU) training backward gathers per node
        std::vector<int32_t> src((size_t)g->E);
        if (g->E) HIPCHK(hipMemcpy(src.data(), g->sh->adj_src, sizeof(int32_t) * (size_t)g->E, hipMemcpyDeviceToHost));
        std::vector<int32_t> ptr((size_t)g->N + 1, 0), inc(2 * rows.size());
        for (int32_t e : rows) { ++ptr[(size_t)entry_dst[e] + 1]; ++ptr[(size_t)src[e] + 1]; }
        for (int64_t i = 0; i < g->N; ++i) ptr[i + 1] += ptr[i];
        std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
        for (size_t q = 0; q < rows.size(); ++q) {
            const int32_t e = rows[q];
            inc[fill[entry_dst[e]]++] = (int32_t)(q << 1);
            inc[fill[src[e]]++] = (int32_t)(q << 1) | 1;
        }
        rc = dev_upload(&l->edge_inc_ptr, ptr.data(), ptr.size());
        if (!rc) rc = dev_upload(&l->edge_inc, inc.data(), inc.size());
    }
    if (!rc) rc = dev_alloc(&l->feats, rows.size() * (size_t)l->ou->dims[0]);
    if (!rc) rc = dev_alloc(&l->out, rows.size() * (size_t)l->T);
    for (int b = 0; b < 2 && !rc; ++b) rc = dev_alloc(&l->otmp[b], rows.size() * (size_t)maxw_o);
    if (rc) return rc;
    l->edge_mode = true;
    l->ran = false;
    return GNN_OK;
}

// NodeGraph^T on the device (kept with the loop, re-uploaded only when it changes) + the partial readout of the owned rows
static int readout_partial(gnn_loop *lm, int G, const int32_t *ng_indptr, const int32_t *ng_node, const float *ng_w)
{
    ARGCHK(lm && G > 0 && ng_indptr, "bad arguments");
    if (!lm->ran) return gnn_fail(GNN_ERR_STATE, "gnn_loop_run has not been called");
    ARGCHK(!lm->edge_mode, "graph readout of an edge-based loop");
    const gnn_graph *g = lm->g;
    ARGCHK(g->n_masked == g->n_rows, "graph-based readout needs all-true masks (GNN.py:275-276, :332): %lld of %lld owned rows are masked in",
           (long long)g->n_masked, (long long)g->n_rows);
    const int nnz = ng_indptr[G];
    ARGCHK(ng_indptr[0] == 0 && nnz >= 0 && (nnz == 0 || (ng_node && ng_w)), "bad NodeGraph CSR");
    for (int e = 0; e < nnz; ++e)
        ARGCHK(ng_node[e] >= 0 && ng_node[e] < g->N_global, "NodeGraph row %d but the graph has %lld nodes", ng_node[e], (long long)g->N_global);
    HIPCHK(hipSetDevice(lm->device));
    std::vector<int32_t> key(ng_indptr, ng_indptr + G + 1);
    key.insert(key.end(), ng_node, ng_node + nnz);
    const bool same = lm->ng_key == key && lm->ng_w_host.size() == (size_t)nnz &&
                      (nnz == 0 || memcmp(lm->ng_w_host.data(), ng_w, sizeof(float) * nnz) == 0);
    int rc = GNN_OK;
    if (same && gnn_loop_ng_folded(lm) && lm->ng_G == G) return GNN_OK;      // the persistent launch of this run has already computed it (gnn_small_kernel.h)
    if (!same) {
        lm->ng_inlaunch = false;
        (void)hipFree(lm->ng_ip); (void)hipFree(lm->ng_node); (void)hipFree(lm->ng_w); (void)hipFree(lm->ng_out); (void)hipFree(lm->ng_part);
        lm->ng_ip = lm->ng_node = nullptr; lm->ng_w = lm->ng_out = lm->ng_part = nullptr;
        lm->ng_key.clear();
        rc = dev_upload(&lm->ng_ip, ng_indptr, (size_t)G + 1);
        if (!rc) rc = dev_upload(&lm->ng_node, ng_node, (size_t)nnz);
        if (!rc) rc = dev_upload(&lm->ng_w, ng_w, (size_t)nnz);
        if (!rc) rc = dev_alloc(&lm->ng_out, (size_t)G * lm->T);
        if (!rc && lm->world > 1) rc = dev_alloc(&lm->ng_part, (size_t)lm->world * G * lm->T);
        if (rc) return rc;
        lm->ng_key = key;
        lm->ng_w_host.assign(ng_w, ng_w + nnz);
        lm->ng_G = G;
    }
    float *dst = lm->world > 1 ? lm->ng_part + (size_t)lm->rank * G * lm->T : lm->ng_out;
    hipLaunchKernelGGL(k_readout, cdiv((int64_t)G * lm->T, 64), 64, 0, lm->stream, G, lm->T, lm->ng_ip, lm->ng_node, lm->ng_w, lm->out, g->row_begin, g->n_rows, dst);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

static int readout_combine(gnn_loop *lm, int G, float *out_graph)
{
    if (gnn_loop_ng_folded(lm) && lm->ng_G == G && lm->world == 1) {      // folded into the persistent launch: the result is in pinned host memory
        memcpy(out_graph, lm->ng_host, sizeof(float) * (size_t)G * lm->T);
        return GNN_OK;
    }
    if (lm->world > 1) {
        hipLaunchKernelGGL(k_sum_partials, cdiv((int64_t)G * lm->T, 64), 64, 0, lm->stream, G * lm->T, lm->world, lm->ng_part, lm->ng_out);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out_graph, lm->ng_out, sizeof(float) * (size_t)G * lm->T, hipMemcpyDeviceToHost, lm->stream));
    HIPCHK(hipStreamSynchronize(lm->stream));
    return GNN_OK;
}

extern "C" int gnn_loop_readout(const gnn_loop *l, int G, const int32_t *ng_indptr, const int32_t *ng_node,
                                const float *ng_w, float *out_graph)
{
    ARGCHK(l && out_graph, "bad arguments");
    gnn_loop *lm = const_cast<gnn_loop *>(l);
    if (lm->comm && lm->comm->grp && lm->world > 1) return gnn_fail(GNN_ERR_STATE, "loopback group: use gnn_loop_readout_group");
    int rc = readout_partial(lm, G, ng_indptr, ng_node, ng_w);
    if (rc) return rc;
    if (lm->world > 1) {       // every rank gets every rank's [G, T] partial (a few KB), then adds them in rank order
        const size_t cnt = (size_t)G * lm->T;
        NCCLCHK(g_rccl.AllGather(lm->ng_part + cnt * lm->rank, lm->ng_part, cnt, NCCL_FLOAT32, lm->comm->nccl, lm->stream));
    }
    return readout_combine(lm, G, out_graph);
}

extern "C" int gnn_loop_readout_group(gnn_loop **loops, int n, int G, const int32_t *ng_indptr, const int32_t *ng_node, const float *ng_w,
                                      float *out_graph)
{
    ARGCHK(loops && n >= 1 && out_graph, "bad arguments");
    for (int r = 0; r < n; ++r)
        ARGCHK(loops[r] && loops[r]->comm && loops[r]->comm->grp && loops[r]->comm->grp == loops[0]->comm->grp && loops[r]->world == n && loops[r]->rank == r,
               "loops must be the %d ranks of one loopback group, in rank order", n);
    int rc = 0;
    for (int r = 0; r < n; ++r) if ((rc = readout_partial(loops[r], G, ng_indptr, ng_node, ng_w))) return rc;
    const size_t cnt = (size_t)G * loops[0]->T;
    for (int r = 0; r < n; ++r)
        for (int p = 0; p < n; ++p)
            if (p != r) HIPCHK(hipMemcpyAsync(loops[p]->ng_part + cnt * r, loops[r]->ng_part + cnt * r, sizeof(float) * cnt, hipMemcpyDeviceToDevice, loops[r]->stream));
    std::vector<float> first(cnt), other(cnt);
    for (int r = 0; r < n; ++r) {
        if ((rc = readout_combine(loops[r], G, r ? other.data() : first.data()))) return rc;
        if (r && memcmp(first.data(), other.data(), sizeof(float) * cnt) != 0) return gnn_fail(GNN_ERR_STATE, "ranks disagree on the graph readout");
    }
    memcpy(out_graph, first.data(), sizeof(float) * cnt);
    return GNN_OK;
}

extern "C" int gnn_lgnn_run(gnn_loop *const *loops, gnn_graph *const *graphs, int n_layers, int get_state, int get_output, float *k_out)
{
    ARGCHK(loops && graphs && n_layers >= 1 && k_out, "bad arguments");
    for (int i = 0; i < n_layers; ++i) {
        ARGCHK(loops[i] && graphs[i] && loops[i]->g == graphs[i], "loops[%d] was not created on graphs[%d]", i, i);
        ARGCHK(i == 0 || graphs[i]->sh == graphs[0]->sh, "graphs[%d] is not derived from graphs[0]", i);
    }
    ARGCHK(graphs[0]->NL == graphs[0]->base_NL && !graphs[0]->arc_labels_own, "graphs[0] must be the original (underived) graph (LGNN.py:287)");
    for (int i = 0; i < n_layers; ++i) {
        int rc = gnn_loop_run(loops[i], 0, &k_out[i]);
        if (rc) return rc;
        if (i + 1 < n_layers && (rc = gnn_graph_update_labels(graphs[i + 1], graphs[0], loops[i], get_state, get_output))) return rc;
    }
    return GNN_OK;
}

extern "C" int gnn_loop_destroy(gnn_loop *l)
{
    if (!l) return GNN_OK;
    (void)hipSetDevice(l->device);
    if (l->comm && l->comm->grp && l->comm->grp->member[l->rank] == l) l->comm->grp->member[l->rank] = nullptr;
    gnn_train_ctx_free(l);
    gnn_train_arena_free(l);
    for (int b = 0; b < 2; ++b) { (void)hipFree(l->state[b]); (void)hipFree(l->tmp[b]); (void)hipFree(l->otmp[b]); }
    (void)hipFree(l->inp); (void)hipFree(l->inv); (void)hipFree(l->proj); (void)hipFree(l->state_init); (void)hipFree(l->feats); (void)hipFree(l->out); (void)hipFree(l->flags); (void)hipFree(l->kfinal_dev);      // (tile_ctr lives in the flag block)
    if (l->kfinal_host) (void)hipHostFree(l->kfinal_host);
    (void)hipFree(l->small_xs);
    for (hipEvent_t e : l->ev) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) if (l->ev_total[i]) (void)hipEventDestroy(l->ev_total[i]);
    if (l->gate_host) (void)hipHostFree(l->gate_host);
    if (l->ev_gate) (void)hipEventDestroy(l->ev_gate);
    if (l->ng_host) (void)hipHostFree(l->ng_host);
    (void)hipFree(l->edge_dst); (void)hipFree(l->edge_rows); (void)hipFree(l->edge_labels); (void)hipFree(l->edge_inc_ptr); (void)hipFree(l->edge_inc);
    (void)hipFree(l->sl_send); (void)hipFree(l->sl_state); (void)hipFree(l->sl_agg); (void)hipFree(l->sl_recv); (void)hipFree(l->agg_own);
    for (hipEvent_t ev : l->sl_ev) if (ev) (void)hipEventDestroy(ev);
    if (l->sl_done) (void)hipEventDestroy(l->sl_done);
    (void)hipFree(l->ng_ip); (void)hipFree(l->ng_node); (void)hipFree(l->ng_w); (void)hipFree(l->ng_out); (void)hipFree(l->ng_part);
    if (!l->comm && l->stream) (void)hipStreamDestroy(l->stream);
    gnn_comm *comm = l->comm;
    delete l;
    if (comm && --comm->loops == 0 && comm->closed) return gnn_comm_destroy(comm);
    return GNN_OK;
}
