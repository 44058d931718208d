// The graph handle of the gfx950 engine: creation (whole graphs, row shards, boundary-exchange shards), derived graphs of LGNN stacks and
// their relabelling.
//
// Reference call sites replaced (paths relative to the reference root):
//   k_relabel     LGNN.update_graph               GNN/LGNN.py:227-260
#include <stdlib.h>
#include <string.h>

#include "gnn_engine.h"

// ---------------------------------------------------------------------------------------------------------------------
// creation-time fills
// ---------------------------------------------------------------------------------------------------------------------
// Creation-time fills are STREAM-ORDERED (round 3).  hipMemset on device memory is queued on the null stream and returns before
// the fill has run (tools/memset_probe.hip); the loops work on hipStreamNonBlocking streams, which the null stream does not order,
// so a fill queued at creation time may land AFTER data that such a stream wrote later (tools/memset_race_probe.hip reproduces
// it: derive -> relabel).  Hence:
//   * buffers of a handle that has a stream (gnn_loop: state ping-pong, slice aggregate) are zeroed with hipMemsetAsync on THAT
//     stream - every later kernel / copy of the handle is behind the fill by stream order, nothing waits on the host;
//   * buffers of a handle without a stream (derived graphs: labels) are zeroed on the engine's per-device fill stream and the
//     handle keeps an event; every stream that touches the labels first waits for it ON THE DEVICE (gnn_graph_wait_ready:
//     hipStreamWaitEvent), host readers synchronise on the event.  No device-wide synchronisation anywhere.
static hipStream_t g_fill_stream[64] = {nullptr};

static int fill_stream(int device, hipStream_t *st)
{
    if (device < 0 || device >= 64) return gnn_fail(GNN_ERR_ARG, "device %d out of range", device);
    if (!g_fill_stream[device]) HIPCHK(hipStreamCreateWithFlags(&g_fill_stream[device], hipStreamNonBlocking));
    *st = g_fill_stream[device];
    return GNN_OK;
}

// queue the zero fill of a fresh graph-owned buffer and (re)record the graph's ready event behind it
static int graph_zero_fill(gnn_graph *g, void *p, size_t bytes)
{
    hipStream_t st = nullptr;
    int rc = fill_stream(g->device, &st);
    if (rc) return rc;
#ifdef GNN_DIAG      // diagnostic build only: the creation-time fill as it was before round 3 (null stream, unordered) - exists to show that
    // tests/test_gpu_full_size.py::test_relabelling_is_ordered_behind_the_creation_fill fails without the ordering
    static const bool legacy = getenv("GNN_LEGACY_NULL_MEMSET") != nullptr;
    if (legacy) { HIPCHK(hipMemset(p, 0, bytes)); return GNN_OK; }
#endif
    if (!g->ready) HIPCHK(hipEventCreateWithFlags(&g->ready, hipEventDisableTiming));
    if ((rc = zero_on_stream(p, bytes, st))) return rc;
    HIPCHK(hipEventRecord(g->ready, st));
    return GNN_OK;
}

// device-side wait: work queued on `st` after this call runs after the graph's creation-time fills
int gnn_graph_wait_ready(const gnn_graph *g, hipStream_t st)
{
    if (g && g->ready) HIPCHK(hipStreamWaitEvent(st, g->ready, 0));
    return GNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// kernels of the label relabelling
// ---------------------------------------------------------------------------------------------------------------------
// LGNN.update_graph: dst[i] = [base[i, :NLb] | state[i] (if get_state) | mask[i] ? out[pos(i)] : 0 (if get_output)]
__global__ void k_relabel(int64_t N, int NLb, const float *__restrict__ base_nodes, int Ds, GnnStateTabs tabs,
                          const int *kfinal, int get_state, int T, const float *__restrict__ out,
                          const uint8_t *__restrict__ mask, const int32_t *__restrict__ mask_pos, int get_output,
                          float *__restrict__ dst, int NLd)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * NLd) return;
    const int64_t i = t / NLd;
    int c = (int)(t - i * NLd);
    float v;
    if (c < NLb) {
        v = base_nodes[i * NLb + c];
    } else {
        c -= NLb;
        if (get_state && c < Ds) {
            const float *state = gnn_state_after(tabs, *kfinal);
            v = state[i * Ds + c];
        } else {
            if (get_state) c -= Ds;
            v = mask[i] ? out[(int64_t)mask_pos[i] * T + c] : 0.0f;
        }
    }
    dst[t] = v;
}

// arc side of LGNN.update_graph (LGNN.py:253-254), original arc order: dst[p] = [base labels of arc p | 0 ...]; the output rows
// are then scattered over the masked positions by k_arc_scatter
__global__ void k_arc_base(int64_t E, int ALb, const float *__restrict__ base, int ALd, float *__restrict__ dst)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= E * ALd) return;
    const int64_t p = t / ALd;
    const int c = (int)(t - p * ALd);
    dst[t] = c < ALb ? base[p * ALb + c] : 0.0f;
}

__global__ void k_arc_scatter(int64_t M, int T, const int32_t *__restrict__ rows, const float *__restrict__ out, int ALb, int ALd, float *__restrict__ dst)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M * T) return;
    const int64_t m = t / T;
    const int c = (int)(t - m * T);
    dst[(int64_t)rows[m] * ALd + ALb + c] = out[t];
}

// ArcNode^T order: entry q carries the labels of arc arc_id[q]
__global__ void k_arc_permute(int64_t E, int AL, const int32_t *__restrict__ arc_id, const float *__restrict__ orig, float *__restrict__ csr)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= E * AL) return;
    const int64_t q = t / AL;
    const int c = (int)(t - q * AL);
    csr[t] = orig[(int64_t)arc_id[q] * AL + c];
}

// ---------------------------------------------------------------------------------------------------------------------
// graph
// ---------------------------------------------------------------------------------------------------------------------
static void graph_release_shared(gnn_graph_shared *sh)
{
    if (!sh || --sh->refs > 0) return;
    (void)hipFree(sh->indptr); (void)hipFree(sh->adj_src); (void)hipFree(sh->masked_rows);
    (void)hipFree(sh->adj_w); (void)hipFree(sh->arc_w); (void)hipFree(sh->arc_labels); (void)hipFree(sh->mask);
    (void)hipFree(sh->src_indptr); (void)hipFree(sh->src_dst); (void)hipFree(sh->src_w);
    (void)hipFree(sh->arc_id); (void)hipFree(sh->arc_labels_orig);
    (void)hipFree(sh->full_indptr); (void)hipFree(sh->full_src); (void)hipFree(sh->full_w);
    (void)hipFree(sh->gp_hdr); (void)hipFree(sh->gp_ent); (void)hipFree(sh->gp_slot[0]); (void)hipFree(sh->gp_slot[1]);
    delete sh;
}

static int graph_create_impl(int64_t n_index, int64_t n_global, int64_t row_begin, int64_t own_off, int64_t n_rows, int64_t n_arcs,
                             const int32_t *indptr, const int32_t *adj_src, const float *adj_w, const float *arc_w,
                             const float *arc_labels, int dim_arc_label, const float *nodes, int dim_node_label,
                             const uint8_t *mask, int device, gnn_graph **out)
{
    ARGCHK(out, "out is NULL");
    *out = nullptr;
    ARGCHK(n_index > 0 && n_index < (int64_t)1 << 31 && n_global > 0 && n_global < (int64_t)1 << 31, "n_nodes=%lld out of range", (long long)n_global);
    ARGCHK(row_begin >= 0 && n_rows >= 0 && row_begin + n_rows <= n_global && own_off >= 0 && own_off + n_rows <= n_index,
           "owned rows [%lld,+%lld) outside [0,%lld)", (long long)row_begin, (long long)n_rows, (long long)n_global);
    ARGCHK(n_arcs >= 0 && n_arcs < (int64_t)1 << 31, "n_arcs=%lld out of range", (long long)n_arcs);
    ARGCHK(dim_node_label > 0 && dim_arc_label >= 0, "label dims must be NL>0, AL>=0");
    ARGCHK(indptr && nodes && mask, "indptr/nodes/mask are required");
    ARGCHK(n_arcs == 0 || (adj_src && adj_w && arc_w && (arc_labels || dim_arc_label == 0)), "arc arrays are required");
    ARGCHK(indptr[0] == 0 && indptr[n_rows] == n_arcs, "indptr[0]=%d, indptr[n_rows]=%d, n_arcs=%lld", indptr[0],
           indptr[n_rows], (long long)n_arcs);
    int maxdeg = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int d = indptr[r + 1] - indptr[r];
        ARGCHK(d >= 0, "indptr not monotone at row %lld", (long long)r);
        maxdeg = std::max(maxdeg, d);
    }
    for (int64_t e = 0; e < n_arcs; ++e)
        ARGCHK(adj_src[e] >= 0 && adj_src[e] < n_index, "adj_src[%lld]=%d outside [0,%lld)", (long long)e, adj_src[e], (long long)n_index);

    HIPCHK(hipSetDevice(device));
    gnn_graph *g = new gnn_graph();
    g->device = device; g->N = n_index; g->N_global = n_global; g->row_begin = row_begin; g->own_off = own_off; g->n_rows = n_rows; g->E = n_arcs;
    g->NL = dim_node_label; g->AL = dim_arc_label; g->base_NL = dim_node_label; g->base_AL = dim_arc_label;
    g->nodes_rows = n_index;
    g->sh = new gnn_graph_shared();
    g->sh->max_degree = maxdeg;
    // masked_rows holds [n_masked] owned-row indices with mask set, followed by [n_rows] exclusive positions
    std::vector<int32_t> rows, pos((size_t)n_rows);
    for (int64_t r = 0; r < n_rows; ++r) { pos[r] = (int32_t)rows.size(); if (mask[r]) rows.push_back((int32_t)r); }
    g->n_masked = (int64_t)rows.size();
    std::vector<int32_t> both(rows);
    both.insert(both.end(), pos.begin(), pos.end());
    int rc = 0;
    if ((rc = dev_upload(&g->sh->indptr, indptr, (size_t)n_rows + 1)) || (rc = dev_upload(&g->sh->adj_src, adj_src, (size_t)n_arcs)) ||
        (rc = dev_upload(&g->sh->adj_w, adj_w, (size_t)n_arcs)) || (rc = dev_upload(&g->sh->arc_w, arc_w, (size_t)n_arcs)) ||
        (rc = dev_upload(&g->sh->arc_labels, arc_labels, (size_t)n_arcs * dim_arc_label)) ||
        (rc = dev_upload(&g->sh->mask, mask, (size_t)n_rows)) || (rc = dev_upload(&g->sh->masked_rows, both.data(), both.size())) ||
        (rc = dev_upload(&g->nodes, nodes, (size_t)n_index * dim_node_label))) {
        gnn_graph_destroy(g);
        return rc;
    }
    *out = g;
    return GNN_OK;
}

extern "C" int gnn_graph_create(int64_t n_nodes, int64_t row_begin, int64_t n_rows, int64_t n_arcs,
                                const int32_t *indptr, const int32_t *adj_src, const float *adj_w, const float *arc_w,
                                const float *arc_labels, int dim_arc_label, const float *nodes, int dim_node_label,
                                const uint8_t *mask, int device, gnn_graph **out)
{
    return graph_create_impl(n_nodes, n_nodes, row_begin, row_begin, n_rows, n_arcs, indptr, adj_src, adj_w, arc_w, arc_labels, dim_arc_label,
                             nodes, dim_node_label, mask, device, out);
}

// Shard with a BOUNDARY exchange ("halo"): the state replica of rank r holds its own shard followed by one block per rank
// with only the rows that some OTHER rank reads (gnn_halo_plan computes the blocks from the whole graph), so the
// per-iteration all-gather moves boundary rows instead of whole shards.  Index space of adj_src / nodes:
//   [0, shard)                           owned rows (shard = rows per rank of gnn_shard_range, the last shard may be short)
//   shard + q * block + j                j-th boundary row of rank q (ascending global id), j < count_q <= block
extern "C" int gnn_graph_create_halo(int64_t n_nodes_global, int rank, int world, int64_t halo_block, int64_t n_send, const int32_t *send_rows,
                                     int64_t n_arcs, const int32_t *indptr, const int32_t *adj_src_replica, const float *adj_w,
                                     const float *arc_w, const float *arc_labels, int dim_arc_label, const float *nodes_replica,
                                     int dim_node_label, const uint8_t *mask, int device, gnn_graph **out)
{
    ARGCHK(out, "out is NULL");
    *out = nullptr;
    ARGCHK(world >= 2 && rank >= 0 && rank < world && halo_block >= 0 && n_send >= 0 && n_send <= halo_block && (n_send == 0 || send_rows), "bad halo description");
    int64_t rb = 0, nr = 0;
    int rc = gnn_shard_range(n_nodes_global, rank, world, &rb, &nr);
    if (rc) return rc;
    const int64_t shard = ((n_nodes_global + world - 1) / world + 31) / 32 * 32;
    for (int64_t j = 0; j < n_send; ++j)
        ARGCHK(send_rows[j] >= 0 && send_rows[j] < nr && (j == 0 || send_rows[j] > send_rows[j - 1]), "send_rows must be ascending owned-row indices");
    const int64_t n_index = shard + (int64_t)world * halo_block;
    rc = graph_create_impl(n_index, n_nodes_global, rb, 0, nr, n_arcs, indptr, adj_src_replica, adj_w, arc_w, arc_labels, dim_arc_label, nodes_replica,
                           dim_node_label, mask, device, out);
    if (rc) return rc;
    gnn_graph *g = *out;
    g->halo_world = world; g->halo_rank = rank; g->halo_block = halo_block; g->halo_count = n_send;
    rc = dev_upload(&g->halo_send, send_rows, (size_t)n_send);
    if (rc) { gnn_graph_destroy(g); *out = nullptr; return rc; }
    return GNN_OK;
}

// Host helper for gnn_graph_create_halo: from the CSR-by-destination of the WHOLE graph, the boundary rows of every rank.
// is_boundary[v] = 1 iff some arc v -> d has owner(d) != owner(v); counts[q] = boundary rows owned by rank q;
// slot[v] = position of v among the boundary rows of its owner (ascending id), -1 otherwise.  *block = max_q counts[q].
extern "C" int gnn_halo_plan(int64_t n_nodes, int world, const int32_t *indptr, const int32_t *adj_src, int32_t *slot, int64_t *counts, int64_t *block)
{
    ARGCHK(n_nodes > 0 && world >= 1 && indptr && slot && counts && block, "bad arguments");
    const int64_t shard = ((n_nodes + world - 1) / world + 31) / 32 * 32;
    std::vector<uint8_t> bnd((size_t)n_nodes, 0);
    for (int64_t d = 0; d < n_nodes; ++d) {
        const int64_t od = d / shard;
        for (int32_t e = indptr[d]; e < indptr[d + 1]; ++e) {
            const int32_t v = adj_src[e];
            ARGCHK(v >= 0 && v < n_nodes, "adj_src[%d]=%d outside [0,%lld)", e, v, (long long)n_nodes);
            if (v / shard != od) bnd[v] = 1;
        }
    }
    int64_t mx = 0;
    for (int q = 0; q < world; ++q) {
        int64_t c = 0;
        const int64_t b = std::min<int64_t>(n_nodes, shard * q), e = std::min<int64_t>(n_nodes, shard * (q + 1));
        for (int64_t v = b; v < e; ++v) slot[v] = bnd[v] ? (int32_t)c++ : -1;
        counts[q] = c;
        mx = std::max(mx, c);
    }
    *block = mx;
    return GNN_OK;
}

static inline const int32_t *graph_mask_pos(const gnn_graph *g) { return g->sh->masked_rows + g->n_masked; }

// rows allocated for the node labels of a derived graph: the sharded relabelling all-gathers whole shards in place, and
// shard * world <= N + 33 * world
static inline int64_t derived_node_rows(int64_t n) { return n + 33 * 64; }

extern "C" int gnn_graph_derive(const gnn_graph *base, int extra, gnn_graph **out)
{
    ARGCHK(base && out && extra >= 0, "bad arguments");
    *out = nullptr;
    HIPCHK(hipSetDevice(base->device));
    gnn_graph *g = new gnn_graph(*base);
    g->sh->refs++;
    g->NL = base->base_NL + extra;
    g->nodes = nullptr;
    g->arc_labels_own = g->arc_labels_orig_own = nullptr;      // never share the owned arc labels of a derived base
    g->halo_send_owned = false;                                // (boundary-exchange shards: same shard, same boundary rows; the base outlives its derived graphs' use of them)
    g->AL = base->base_AL;
    g->nodes_rows = derived_node_rows(g->N);
    g->ready = nullptr;                                        // (the base's event, if any, stays the base's)
    int rc = dev_alloc(&g->nodes, (size_t)g->nodes_rows * g->NL);
    if (!rc) rc = graph_zero_fill(g, g->nodes, (size_t)g->nodes_rows * g->NL * sizeof(float));
    if (rc) { gnn_graph_destroy(g); return rc; }
    *out = g;
    return GNN_OK;
}

extern "C" int gnn_graph_set_arc_order(gnn_graph *g, const int32_t *arc_id, const float *arc_labels_orig)
{
    ARGCHK(g && (g->E == 0 || (arc_id && (arc_labels_orig || g->AL == 0))), "bad arguments");
    ARGCHK(g->NL == g->base_NL && !g->arc_labels_own, "set the arc order on the original (underived) graph");
    HIPCHK(hipSetDevice(g->device));
    std::vector<uint8_t> seen((size_t)g->E, 0);
    for (int64_t q = 0; q < g->E; ++q) {
        ARGCHK(arc_id[q] >= 0 && arc_id[q] < g->E && !seen[arc_id[q]], "arc_id is not a permutation of the arcs at entry %lld", (long long)q);
        seen[arc_id[q]] = 1;
    }
    (void)hipFree(g->sh->arc_id); (void)hipFree(g->sh->arc_labels_orig);
    g->sh->arc_id = nullptr; g->sh->arc_labels_orig = nullptr;
    int rc = dev_upload(&g->sh->arc_id, arc_id, (size_t)g->E);
    if (!rc) rc = dev_upload(&g->sh->arc_labels_orig, arc_labels_orig, (size_t)g->E * g->AL);
    return rc;
}

extern "C" int gnn_graph_derive_edge(const gnn_graph *base, int extra_nodes, int extra_arcs, gnn_graph **out)
{
    ARGCHK(base && out && extra_nodes >= 0 && extra_arcs >= 0, "bad arguments");
    ARGCHK(base->sh->arc_id, "call gnn_graph_set_arc_order on the base graph first");
    ARGCHK(base->n_rows == base->N, "edge-based LGNN stacks are single-GPU only");
    int rc = gnn_graph_derive(base, extra_nodes, out);
    if (rc) return rc;
    gnn_graph *g = *out;
    *out = nullptr;
    g->AL = base->base_AL + extra_arcs;
    g->arc_labels_own = g->arc_labels_orig_own = nullptr;
    rc = dev_alloc(&g->arc_labels_own, (size_t)g->E * g->AL);
    if (!rc) rc = dev_alloc(&g->arc_labels_orig_own, (size_t)g->E * g->AL);
    if (!rc) rc = graph_zero_fill(g, g->arc_labels_own, std::max<size_t>(1, (size_t)g->E * g->AL) * sizeof(float));
    if (!rc) rc = graph_zero_fill(g, g->arc_labels_orig_own, std::max<size_t>(1, (size_t)g->E * g->AL) * sizeof(float));
    if (rc) { gnn_graph_destroy(g); return rc; }
    *out = g;
    return GNN_OK;
}

extern "C" int gnn_graph_get_nodes(const gnn_graph *g, float *nodes_out)
{
    ARGCHK(g && nodes_out, "bad arguments");
    HIPCHK(hipSetDevice(g->device));
    if (g->ready) HIPCHK(hipEventSynchronize(g->ready));
    HIPCHK(hipMemcpy(nodes_out, g->nodes, (size_t)g->N * g->NL * sizeof(float), hipMemcpyDeviceToHost));   // index-space rows (all nodes for full replicas)
    return GNN_OK;
}

extern "C" int gnn_graph_dims(const gnn_graph *g, int64_t *n_nodes, int64_t *n_rows, int64_t *n_arcs, int *nl, int *al,
                              int64_t *n_masked)
{
    ARGCHK(g, "graph is NULL");
    if (n_nodes) *n_nodes = g->N;
    if (n_rows) *n_rows = g->n_rows;
    if (n_arcs) *n_arcs = g->E;
    if (nl) *nl = g->NL;
    if (al) *al = g->AL;
    if (n_masked) *n_masked = g->n_masked;
    return GNN_OK;
}

extern "C" int gnn_graph_set_full_adjacency(gnn_graph *g, int64_t n_global, const int32_t *indptr, const int32_t *adj_src, const float *adj_w)
{
    ARGCHK(g && indptr && n_global > 0, "bad arguments");
    ARGCHK(n_global == g->N_global, "the shard belongs to a graph of %lld nodes, not %lld", (long long)g->N_global, (long long)n_global);
    ARGCHK(!g->halo_world, "a boundary-exchange shard numbers its sources in its own compact space: use a full-replica shard");
    const int64_t e = indptr[n_global];
    ARGCHK(indptr[0] == 0 && e >= 0 && (e == 0 || (adj_src && adj_w)), "bad CSR");
    for (int64_t i = 0; i < n_global; ++i) ARGCHK(indptr[i] <= indptr[i + 1], "indptr must be non-decreasing");
    for (int64_t q = 0; q < e; ++q) ARGCHK(adj_src[q] >= 0 && adj_src[q] < n_global, "adj_src[%lld] out of range", (long long)q);
    HIPCHK(hipSetDevice(g->device));
    gnn_graph_shared *sh = g->sh;                  // shared with the graphs derived from g
    (void)hipFree(sh->full_indptr); (void)hipFree(sh->full_src); (void)hipFree(sh->full_w);
    sh->full_indptr = nullptr; sh->full_src = nullptr; sh->full_w = nullptr; sh->full_rows = 0;
    int rc = dev_upload(&sh->full_indptr, indptr, (size_t)n_global + 1);
    if (!rc) rc = dev_upload(&sh->full_src, adj_src, (size_t)e);
    if (!rc) rc = dev_upload(&sh->full_w, adj_w, (size_t)e);
    if (rc) return rc;
    sh->full_rows = n_global;
    return GNN_OK;
}

extern "C" int gnn_graph_destroy(gnn_graph *g)
{
    if (!g) return GNN_OK;
    (void)hipSetDevice(g->device);
    (void)hipFree(g->arc_labels_own); (void)hipFree(g->arc_labels_orig_own);
    if (g->halo_send_owned) (void)hipFree(g->halo_send);
    (void)hipFree(g->nodes);
    if (g->ready) (void)hipEventDestroy(g->ready);
    graph_release_shared(g->sh);
    delete g;
    return GNN_OK;
}

// LGNN.update_graph on the owned rows of `dst` (reference GNN/LGNN.py:227-260); nothing is synchronised here
static int relabel_own(gnn_graph *dst, const gnn_graph *base, const gnn_loop *from, int get_state, int get_output)
{
    ARGCHK(dst && base && from, "bad arguments");
    ARGCHK(dst->sh == base->sh, "dst must be derived from base");
    if (!from->ran) return gnn_fail(GNN_ERR_STATE, "the source loop has not run");
    ARGCHK(from->g->sh == base->sh, "the source loop ran on an unrelated graph");
    ARGCHK(!base->halo_world || (dst->halo_world == base->halo_world && dst->halo_block == base->halo_block), "dst is not a boundary-exchange shard like base");
    // edge-based layers put the output on the ARC labels (LGNN.py:253-254), node/graph-based ones on the node labels (:256)
    const bool arc_side = from->edge_mode;
    ARGCHK(!arc_side || from->world == 1, "edge-based LGNN stacks are single-GPU only");
    const int out_nodes = (get_output && !arc_side) ? from->T : 0, out_arcs = (get_output && arc_side) ? from->T : 0;
    const int extra = (get_state ? from->Ds : 0) + out_nodes;
    ARGCHK(dst->NL == base->base_NL + extra, "dst label width %d != %d + %d", dst->NL, base->base_NL, extra);
    HIPCHK(hipSetDevice(dst->device));
    // base labels are the first base_NL columns of base->nodes only when base is not itself derived
    ARGCHK(base->NL == base->base_NL, "base must be the original (underived) graph (LGNN.py:287)");
    const int64_t rows = base->n_rows, off = base->own_off;
    const int64_t tot = rows * dst->NL;
    int rcw = gnn_graph_wait_ready(dst, from->stream);          // the creation-time zero fill of dst's labels is ordered BEFORE the relabelling
    if (rcw) return rcw;
    if (tot)
        hipLaunchKernelGGL(k_relabel, cdiv(tot, 256), 256, 0, from->stream, rows, base->NL, base->nodes + (size_t)off * base->NL, from->Ds,
                           gnn_loop_state_tabs(from, (size_t)from->own_off), from->kfinal_dev, get_state, from->T,
                           from->out, base->sh->mask, graph_mask_pos(base), out_nodes ? 1 : 0, dst->nodes + (size_t)off * dst->NL, dst->NL);
    if (arc_side) {
        ARGCHK(dst->arc_labels_own && dst->arc_labels_orig_own && base->sh->arc_id, "dst must come from gnn_graph_derive_edge");
        ARGCHK(dst->AL == base->base_AL + out_arcs, "dst arc label width %d != %d + %d", dst->AL, base->base_AL, out_arcs);
        const int64_t E = dst->E;
        if (E && dst->AL) {
            hipLaunchKernelGGL(k_arc_base, cdiv(E * dst->AL, 256), 256, 0, from->stream, E, base->base_AL, base->sh->arc_labels_orig, dst->AL, dst->arc_labels_orig_own);
            if (out_arcs && from->n_edge_masked)
                hipLaunchKernelGGL(k_arc_scatter, cdiv(from->n_edge_masked * from->T, 256), 256, 0, from->stream, from->n_edge_masked, from->T, from->edge_rows,
                                   from->out, base->base_AL, dst->AL, dst->arc_labels_orig_own);
            hipLaunchKernelGGL(k_arc_permute, cdiv(E * dst->AL, 256), 256, 0, from->stream, E, dst->AL, base->sh->arc_id, dst->arc_labels_orig_own, dst->arc_labels_own);
        }
    }
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

// boundary-exchange shards: the rank's boundary rows of the NEW labels go into its block of the index space (then every rank's block is
// exchanged like the state rows of an iteration: all-gather of blocks / device copies in a loopback group)
static int relabel_pack_boundary(gnn_graph *dst, const gnn_loop *from)
{
    if (!dst->halo_world || !dst->halo_count) return GNN_OK;
    float *block = dst->nodes + ((size_t)from->shard_rows + (size_t)dst->halo_rank * dst->halo_block) * dst->NL;
    return gnn_launch_pack_rows(from->stream, dst->halo_count, dst->NL, dst->halo_send, dst->nodes, block);
}

extern "C" int gnn_graph_update_labels(gnn_graph *dst, const gnn_graph *base, const gnn_loop *from, int get_state, int get_output)
{
    ARGCHK(from, "bad arguments");
    if (from->comm && from->comm->grp && from->world > 1) return gnn_fail(GNN_ERR_STATE, "loopback group: use gnn_graph_update_labels_group");
    int rc = relabel_own(dst, base, from, get_state, get_output);
    if (rc) return rc;
    if (from->world > 1 && dst->halo_world) {      // boundary-exchange shards: all-gather of the boundary blocks of the new labels, in place
        if ((rc = relabel_pack_boundary(dst, from))) return rc;
        const size_t cnt = (size_t)dst->halo_block * dst->NL;
        float *blocks = dst->nodes + (size_t)from->shard_rows * dst->NL;
        if (cnt) NCCLCHK(g_rccl.AllGather(blocks + cnt * from->rank, blocks, cnt, NCCL_FLOAT32, from->comm->nccl, from->stream));
    } else if (from->world > 1) {      // every rank relabelled its own rows: all-gather whole shards of the new label rows, in place
        const size_t cnt = (size_t)from->shard_rows * dst->NL;
        ARGCHK((int64_t)from->shard_rows * from->world <= dst->nodes_rows, "derived graph too small for the sharded relabelling");
        NCCLCHK(g_rccl.AllGather(dst->nodes + cnt * from->rank, dst->nodes, cnt, NCCL_FLOAT32, from->comm->nccl, from->stream));
    }
    HIPCHK(hipStreamSynchronize(from->stream));
    dst->label_version++;
    return GNN_OK;
}

extern "C" int gnn_graph_update_labels_group(gnn_graph **dsts, gnn_graph *const *bases, gnn_loop *const *froms, int n, int get_state, int get_output)
{
    ARGCHK(dsts && bases && froms && n >= 1, "bad arguments");
    for (int r = 0; r < n; ++r)
        ARGCHK(froms[r] && froms[r]->comm && froms[r]->comm->grp && froms[r]->comm->grp == froms[0]->comm->grp && froms[r]->world == n && froms[r]->rank == r,
               "froms must be the %d ranks of one loopback group, in rank order", n);
    int rc = 0;
    for (int r = 0; r < n; ++r) if ((rc = relabel_own(dsts[r], bases[r], froms[r], get_state, get_output))) return rc;
    if (dsts[0]->halo_world) {          // boundary-exchange shards: every rank's block of boundary label rows into every other rank's copy
        for (int r = 0; r < n; ++r) {
            ARGCHK(dsts[r]->halo_world == n && dsts[r]->halo_block == dsts[0]->halo_block && dsts[r]->NL == dsts[0]->NL, "ranks hold differently shaped boundary-exchange shards");
            if ((rc = relabel_pack_boundary(dsts[r], froms[r]))) return rc;
        }
        const size_t cnt = (size_t)dsts[0]->halo_block * dsts[0]->NL;
        for (int r = 0; r < n && cnt; ++r) {
            const size_t off = ((size_t)froms[r]->shard_rows + (size_t)r * dsts[r]->halo_block) * dsts[r]->NL;
            for (int p = 0; p < n; ++p)
                if (p != r) HIPCHK(hipMemcpyAsync(dsts[p]->nodes + off, dsts[r]->nodes + off, sizeof(float) * cnt, hipMemcpyDeviceToDevice, froms[r]->stream));
        }
        HIPCHK(hipStreamSynchronize(froms[0]->stream));
        for (int r = 0; r < n; ++r) dsts[r]->label_version++;
        return GNN_OK;
    }
    for (int r = 0; r < n; ++r) {
        const size_t cnt = (size_t)froms[r]->shard_rows * dsts[r]->NL;
        ARGCHK((int64_t)froms[r]->shard_rows * n <= dsts[r]->nodes_rows, "derived graph too small for the sharded relabelling");
        for (int p = 0; p < n; ++p)
            if (p != r) HIPCHK(hipMemcpyAsync(dsts[p]->nodes + cnt * r, dsts[r]->nodes + cnt * r, sizeof(float) * cnt, hipMemcpyDeviceToDevice, froms[r]->stream));
    }
    HIPCHK(hipStreamSynchronize(froms[0]->stream));
    for (int r = 0; r < n; ++r) dsts[r]->label_version++;
    return GNN_OK;
}
