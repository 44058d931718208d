// Device-side graph build: arc list (COO) -> the transposed, row-major reordered sparse operands of the loop.
//
// Replaces, for graphs where minutes of Python would be spent on it, the host chain
//   GraphObject.buildArcNode / buildAdiacency           reference GNN/graph_class.py:90-121
//   GraphTensor.COO2SparseTransposedTensor              reference GNN/graph_class.py:365-372 (transpose + tf.sparse.reorder)
// with two stable radix sorts (hipCUB) and a histogram:
//   Adjacency^T  entries of destination d ordered by source   = arcs sorted by the key (dst, src)
//   ArcNode^T    entries of destination d ordered by arc id   = arc ids stably sorted by dst
//   indptr       exclusive scan of the in-degree histogram (shared by both: same entries per destination)
//   value of arc a: 1 ('sum'), float(1 / n_arcs) ('normalized', the reference divides by the number of ARCS),
//                   float(1 / indegree(dst(a))) ('average'); the division is done in double like NumPy's.
#include <hipcub/hipcub.hpp>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "gnn_common.h"
#include "gnn_fused.h"

namespace {

inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

__global__ void k_keys(int64_t e, const int32_t *src, const int32_t *dst, unsigned long long *key, int32_t *id, int32_t *indeg)
{
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= e) return;
    key[a] = ((unsigned long long)(uint32_t)dst[a] << 32) | (uint32_t)src[a];
    id[a] = (int32_t)a;
    atomicAdd(indeg + dst[a], 1);
}

__global__ void k_values(int64_t e, const int32_t *dst, const int32_t *indeg, int mode, float *w)
{
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= e) return;
    float v = 1.0f;
    if (mode == 1) v = (float)(1.0 / (double)e);
    else if (mode == 2) v = (float)(1.0 / (double)indeg[dst[a]]);
    w[a] = v;
}

// entry q of the sorted order is arc perm[q]
__global__ void k_permute_adj(int64_t e, const int32_t *perm, const int32_t *src, const float *w, int32_t *adj_src, float *adj_w)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= e) return;
    const int32_t a = perm[q];
    adj_src[q] = src[a];
    adj_w[q] = w[a];
}

__global__ void k_permute_arc(int64_t e, int AL, const int32_t *perm, const float *w, const float *labels, float *arc_w, float *arc_labels)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int width = AL > 0 ? AL : 1;
    if (t >= e * width) return;
    const int64_t q = t / width;
    const int c = (int)(t - q * width);
    const int32_t a = perm[q];
    if (c == 0) arc_w[q] = w[a];
    if (AL > 0) arc_labels[q * AL + c] = labels[(int64_t)a * AL + c];
}

struct Scratch {
    std::vector<void *> p;
    template <typename T>
    int get(T **out, size_t count)
    {
        *out = nullptr;
        if (gnn_dev_malloc((void **)out, std::max<size_t>(1, count) * sizeof(T)) != hipSuccess) return gnn_fail(GNN_ERR_HIP, "hipMalloc of %zu bytes failed", count * sizeof(T));
        p.push_back(*out);
        return GNN_OK;
    }
    ~Scratch() { for (void *q : p) (void)hipFree(q); }
};

template <typename T>
int keep(T **dst, size_t count)
{
    *dst = nullptr;
    if (gnn_dev_malloc((void **)dst, std::max<size_t>(1, count) * sizeof(T)) != hipSuccess) return gnn_fail(GNN_ERR_HIP, "hipMalloc of %zu bytes failed", count * sizeof(T));
    return GNN_OK;
}

}   // namespace

extern "C" int gnn_graph_create_from_arcs(int64_t n_nodes, int64_t n_arcs, const int32_t *arc_src, const int32_t *arc_dst,
                                          const float *arc_labels, int dim_arc_label, int aggregation_mode, const float *nodes,
                                          int dim_node_label, const uint8_t *mask, int device, gnn_graph **out,
                                          int32_t *indptr_out, int32_t *adj_src_out, float *adj_w_out, int32_t *arc_id_out,
                                          float *arc_w_out)
{
    ARGCHK(out, "out is NULL");
    *out = nullptr;
    ARGCHK(n_nodes > 0 && n_nodes < (int64_t)1 << 31, "n_nodes=%lld out of range", (long long)n_nodes);
    ARGCHK(n_arcs >= 0 && n_arcs < (int64_t)1 << 31, "n_arcs=%lld out of range", (long long)n_arcs);
    ARGCHK(dim_node_label > 0 && dim_arc_label >= 0, "label dims must be NL>0, AL>=0");
    ARGCHK(aggregation_mode >= 0 && aggregation_mode <= 2, "aggregation_mode: 0 sum, 1 normalized, 2 average");   // graph_class.py:86
    ARGCHK(nodes && mask, "nodes/mask are required");
    ARGCHK(n_arcs == 0 || (arc_src && arc_dst && (arc_labels || dim_arc_label == 0)), "arc arrays are required");
    for (int64_t a = 0; a < n_arcs; ++a)
        ARGCHK(arc_src[a] >= 0 && arc_src[a] < n_nodes && arc_dst[a] >= 0 && arc_dst[a] < n_nodes, "arc %lld = (%d, %d) outside [0,%lld)",
               (long long)a, arc_src[a], arc_dst[a], (long long)n_nodes);
    HIPCHK(hipSetDevice(device));
    const int64_t N = n_nodes, E = n_arcs;
    const int AL = dim_arc_label;
    Scratch tmp;
    int32_t *d_src = nullptr, *d_dst = nullptr, *d_id = nullptr, *d_perm1 = nullptr, *d_perm2 = nullptr, *d_indeg = nullptr, *d_dst_sorted = nullptr;
    unsigned long long *d_key = nullptr, *d_key_sorted = nullptr;
    float *d_lab = nullptr, *d_w = nullptr;
    int rc;
    if ((rc = tmp.get(&d_src, E)) || (rc = tmp.get(&d_dst, E)) || (rc = tmp.get(&d_id, E)) || (rc = tmp.get(&d_perm1, E)) ||
        (rc = tmp.get(&d_perm2, E)) || (rc = tmp.get(&d_indeg, N + 1)) || (rc = tmp.get(&d_dst_sorted, E)) || (rc = tmp.get(&d_key, E)) ||
        (rc = tmp.get(&d_key_sorted, E)) || (rc = tmp.get(&d_lab, (size_t)E * AL)) || (rc = tmp.get(&d_w, E)))
        return rc;
    if (E) {
        HIPCHK(hipMemcpy(d_src, arc_src, sizeof(int32_t) * E, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_dst, arc_dst, sizeof(int32_t) * E, hipMemcpyHostToDevice));
        if (AL) HIPCHK(hipMemcpy(d_lab, arc_labels, sizeof(float) * E * AL, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(d_indeg, 0, sizeof(int32_t) * (N + 1)));

    gnn_graph *g = new gnn_graph();
    g->device = device; g->N = N; g->N_global = N; g->nodes_rows = N; g->row_begin = 0; g->own_off = 0; g->n_rows = N; g->E = E;
    g->NL = dim_node_label; g->AL = AL; g->base_NL = dim_node_label; g->base_AL = AL;
    g->sh = new gnn_graph_shared();
    gnn_graph_shared *sh = g->sh;
    auto fail = [&](int code) { gnn_graph_destroy(g); return code; };
    // from here on a failing HIP call releases the half-built handle (HIPCHK alone would leak it)
#define HIPCHK_G(expr)                                                                                         \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return fail(gnn_fail(GNN_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e_)));    \
    } while (0)
    if ((rc = keep(&sh->indptr, N + 1)) || (rc = keep(&sh->adj_src, E)) || (rc = keep(&sh->adj_w, E)) || (rc = keep(&sh->arc_w, E)) ||
        (rc = keep(&sh->arc_labels, (size_t)E * AL)))
        return fail(rc);

    if (E) {
        hipLaunchKernelGGL(k_keys, cdiv(E, 256), 256, 0, 0, E, d_src, d_dst, d_key, d_id, d_indeg);
        hipLaunchKernelGGL(k_values, cdiv(E, 256), 256, 0, 0, E, d_dst, d_indeg, aggregation_mode, d_w);
    }
    // indptr = exclusive scan of the in-degrees (the extra last element makes indptr[N] = E)
    {
        size_t bytes = 0;
        if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_indeg, sh->indptr, (int)(N + 1)) != hipSuccess) return fail(gnn_fail(GNN_ERR_HIP, "hipcub scan sizing failed"));
        void *ws = nullptr;
        if ((rc = tmp.get((char **)&ws, bytes))) return fail(rc);
        if (hipcub::DeviceScan::ExclusiveSum(ws, bytes, d_indeg, sh->indptr, (int)(N + 1)) != hipSuccess) return fail(gnn_fail(GNN_ERR_HIP, "hipcub scan failed"));
    }
    if (E) {
        int node_bits = 1;
        while (((int64_t)1 << node_bits) < N) ++node_bits;
        size_t b1 = 0, b2 = 0;
        // Adjacency^T order: (dst, src) ascending; ArcNode^T order: dst ascending, arc id ascending (the sort is stable)
        if (hipcub::DeviceRadixSort::SortPairs(nullptr, b1, d_key, d_key_sorted, d_id, d_perm1, (int)E, 0, 32 + node_bits) != hipSuccess ||
            hipcub::DeviceRadixSort::SortPairs(nullptr, b2, d_dst, d_dst_sorted, d_id, d_perm2, (int)E, 0, node_bits) != hipSuccess)
            return fail(gnn_fail(GNN_ERR_HIP, "hipcub sort sizing failed"));
        void *ws = nullptr;
        if ((rc = tmp.get((char **)&ws, std::max(b1, b2)))) return fail(rc);
        if (hipcub::DeviceRadixSort::SortPairs(ws, b1, d_key, d_key_sorted, d_id, d_perm1, (int)E, 0, 32 + node_bits) != hipSuccess ||
            hipcub::DeviceRadixSort::SortPairs(ws, b2, d_dst, d_dst_sorted, d_id, d_perm2, (int)E, 0, node_bits) != hipSuccess)
            return fail(gnn_fail(GNN_ERR_HIP, "hipcub sort failed"));
        hipLaunchKernelGGL(k_permute_adj, cdiv(E, 256), 256, 0, 0, E, d_perm1, d_src, d_w, sh->adj_src, sh->adj_w);
        hipLaunchKernelGGL(k_permute_arc, cdiv(E * (AL > 0 ? AL : 1), 256), 256, 0, 0, E, AL, d_perm2, d_w, d_lab, sh->arc_w, sh->arc_labels);
        HIPCHK_G(hipGetLastError());
    }
    HIPCHK_G(hipStreamSynchronize(nullptr));        // everything above ran on the null stream, in order: no device-wide wait

    // what stays on the host side of the handle: the row list of the mask and the maximum in-degree
    std::vector<int32_t> indptr((size_t)N + 1);
    HIPCHK_G(hipMemcpy(indptr.data(), sh->indptr, sizeof(int32_t) * (N + 1), hipMemcpyDeviceToHost));
    if (indptr[N] != E) return fail(gnn_fail(GNN_ERR_HIP, "device build: indptr[N]=%d but %lld arcs", indptr[N], (long long)E));
    int maxdeg = 0;
    for (int64_t r = 0; r < N; ++r) maxdeg = std::max(maxdeg, indptr[r + 1] - indptr[r]);
    sh->max_degree = maxdeg;
    std::vector<int32_t> rows, pos((size_t)N);
    for (int64_t r = 0; r < N; ++r) { pos[r] = (int32_t)rows.size(); if (mask[r]) rows.push_back((int32_t)r); }
    g->n_masked = (int64_t)rows.size();
    std::vector<int32_t> both(rows);
    both.insert(both.end(), pos.begin(), pos.end());
    if ((rc = keep(&sh->mask, N)) || (rc = keep(&sh->masked_rows, both.size())) || (rc = keep(&g->nodes, (size_t)N * dim_node_label))) return fail(rc);
    HIPCHK_G(hipMemcpy(sh->mask, mask, (size_t)N, hipMemcpyHostToDevice));
    HIPCHK_G(hipMemcpy(sh->masked_rows, both.data(), sizeof(int32_t) * both.size(), hipMemcpyHostToDevice));
    HIPCHK_G(hipMemcpy(g->nodes, nodes, sizeof(float) * (size_t)N * dim_node_label, hipMemcpyHostToDevice));

    // host mirrors for the caller (GraphTensor keeps them like the reference keeps its SparseTensors); any may be NULL
    if (indptr_out) memcpy(indptr_out, indptr.data(), sizeof(int32_t) * (N + 1));
    if (E) {
        if (adj_src_out) HIPCHK_G(hipMemcpy(adj_src_out, sh->adj_src, sizeof(int32_t) * E, hipMemcpyDeviceToHost));
        if (adj_w_out) HIPCHK_G(hipMemcpy(adj_w_out, sh->adj_w, sizeof(float) * E, hipMemcpyDeviceToHost));
        if (arc_id_out) HIPCHK_G(hipMemcpy(arc_id_out, d_perm2, sizeof(int32_t) * E, hipMemcpyDeviceToHost));
        if (arc_w_out) HIPCHK_G(hipMemcpy(arc_w_out, sh->arc_w, sizeof(float) * E, hipMemcpyDeviceToHost));
    }
    *out = g;
    return GNN_OK;
#undef HIPCHK_G
}

// ---------------------------------------------------------------------------------------------------------------------
// Gather program of the full-tile fused kernel (gather form 2; gnn_fused_kernel.h: load_tile_prog64).  Host code.
//
// A lane group of the kernel consumes one entry per slot; a row takes as many slots as it has entries, an empty row one (a zero-weight
// entry without a source, so that its aggregate is written as an exact +0).  The 32 rows of a tile go to the four lane groups as
// contiguous ranges that minimise the largest group's slot count (a group may get no row at all); all four streams are padded to that
// count, rounded up to whole batches of 16.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

// rows [start[g], start[g + 1]) of the tile to lane group g: the smallest possible largest slot count, groups filled front to back
void gather_program_split(const int (&slots)[32], int (&start)[5], int &longest)
{
    int lo = 0, hi = 0;
    for (int r = 0; r < 32; ++r) { lo = std::max(lo, slots[r]); hi += slots[r]; }
    auto groups_needed = [&](int cap) {
        int n = 1, fill = 0;
        for (int r = 0; r < 32; ++r) {
            if (fill + slots[r] > cap) { ++n; fill = 0; }
            fill += slots[r];
        }
        return n;
    };
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (groups_needed(mid) <= 4) hi = mid; else lo = mid + 1;
    }
    int g = 0, fill = 0;
    start[0] = 0;
    for (int r = 0; r < 32; ++r) {
        if (fill + slots[r] > lo) { start[++g] = r; fill = 0; }
        fill += slots[r];
    }
    while (g < 4) start[++g] = 32;
    longest = lo;
}

}   // namespace

extern "C" int gnn_gather_program_build(int64_t n_rows, const int32_t *indptr, const int32_t *adj_src, const float *adj_w, int32_t *hdr,
                                        int32_t *ent, int64_t *n_batches)
{
    ARGCHK(n_rows >= 0 && indptr && n_batches, "n_rows / indptr / n_batches are required");
    const int64_t tiles = n_rows / 32;
    ARGCHK(indptr[tiles * 32] == 0 || (adj_src && adj_w), "arc arrays are required");
    int64_t batch = 0;
    for (int64_t t = 0; t < tiles; ++t) {
        const int32_t *ip = indptr + t * 32;
        int slots[32], start[5], longest = 0;
        for (int r = 0; r < 32; ++r) {
            ARGCHK(ip[r + 1] >= ip[r], "indptr not monotone at row %lld", (long long)(t * 32 + r));
            slots[r] = std::max(1, ip[r + 1] - ip[r]);
        }
        gather_program_split(slots, start, longest);
        const int nb = (longest + 15) / 16;
        ARGCHK(batch + nb < ((int64_t)1 << 31) / 64, "gather program too large");
        if (hdr) { hdr[2 * t] = (int32_t)batch; hdr[2 * t + 1] = nb; }
        if (ent) {
            for (int g = 0; g < 4; ++g) {
                int s = 0;
                auto put = [&](uint32_t word, float w) {
                    int32_t *e = ent + (((batch + s / 16) * 64 + 16 * g + s % 16) * 2);
                    memcpy(e, &word, 4);
                    memcpy(e + 1, &w, 4);
                    ++s;
                };
                for (int r = start[g]; r < start[g + 1]; ++r) {
                    if (ip[r + 1] == ip[r]) put(GNN_GP_NOROW | GNN_GP_ROW_END | (uint32_t)r, 0.0f);
                    for (int32_t e = ip[r]; e < ip[r + 1]; ++e) {
                        if (adj_src[e] < 0 || adj_src[e] >= (1 << 23))
                            return gnn_fail(GNN_ERR_UNSUPPORTED, "adj_src[%d]=%d does not fit a gather-program source word", e, adj_src[e]);
                        put((uint32_t)adj_src[e] << 8 | (e + 1 == ip[r + 1] ? GNN_GP_ROW_END : 0u) | (uint32_t)r, adj_w[e]);
                    }
                }
                while (s < 16 * nb) put(GNN_GP_NOROW, 0.0f);      // behind the group's last row end: whatever it accumulates is never written
            }
        }
        batch += nb;
    }
    *n_batches = batch;
    return GNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Compact format of the program (entry format 4; gnn_fused_kernel.h: prog_weight).  Host code.
//
// The weights of one destination row are equal in every graph the reference builds ('sum' 1, 'average' 1 / in-degree, 'normalized'
// 1 / arcs), so half of an 8-byte entry repeats a value that one float per row carries: words[b][l] = the source word of entry l of batch
// b, unchanged; roww[t][r] = the bit pattern all entries of tile-local row r of tile t share, +0 for an empty row (its single entry had
// weight +0).  Padding needs no weight: it sits behind its group's last row end, and what it accumulates is never written.
// false: some row holds two entries whose weights differ as bit patterns (+0 beside -0 included) - nothing of such a graph is compacted.
// ---------------------------------------------------------------------------------------------------------------------
static bool gather_program_compact(int64_t tiles, const int32_t *hdr, const int32_t *ent, int32_t *words, float *roww)
{
    for (int64_t t = 0; t < tiles; ++t) {
        uint32_t bits[32] = {0};
        bool seen[32] = {false};
        const int64_t first = hdr[2 * t], nb = hdr[2 * t + 1];
        for (int64_t s = first * 64; s < (first + nb) * 64; ++s) {
            uint32_t word, wb;
            memcpy(&word, ent + 2 * s, 4);
            memcpy(&wb, ent + 2 * s + 1, 4);
            words[s] = ent[2 * s];
            if ((word & GNN_GP_NOROW) == GNN_GP_NOROW) continue;      // no source: padding, or an empty row's entry (weight +0)
            const int r = (int)(word & GNN_GP_ROW_MASK);
            if (seen[r] && bits[r] != wb) return false;
            seen[r] = true; bits[r] = wb;
        }
        memcpy(roww + 32 * t, bits, sizeof(bits));
    }
    return true;
}

extern "C" int gnn_gather_program_compact(int64_t tiles, const int32_t *hdr, int64_t n_batches, const int32_t *ent, int32_t *words, float *roww)
{
    ARGCHK(tiles >= 0 && n_batches >= 0 && (tiles == 0 || (hdr && roww)) && (n_batches == 0 || (ent && words)), "hdr / ent / words / roww are required");
    for (int64_t t = 0; t < tiles; ++t)
        ARGCHK(hdr[2 * t] >= 0 && hdr[2 * t + 1] >= 0 && (int64_t)hdr[2 * t] + hdr[2 * t + 1] <= n_batches, "header of tile %lld outside the program", (long long)t);
    if (!gather_program_compact(tiles, hdr, ent, words, roww))
        return gnn_fail(GNN_ERR_UNSUPPORTED, "not compactable: a row holds entries of different weights");
    return GNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Tile schedule of the program kernel: the order in which a launch works through its tiles.  Host code.
//
// order[slot] = the tile that ticket `slot` stands for.  Kind 0: the identity.  Kind 1, the balanced order, from the tiles sorted by cost
// descending (ties by tile id ascending, so the result is a function of the arguments alone):
//   tail  the lightest K = min(2 waves, slots / 2) tiles come last, heaviest first - the launch ends on its cheapest tiles;
//   body  the rest is cut into S strata of ceil(M / S) consecutive sorted tiles and dealt column-wise: one tile of every stratum, then the
//         next of every stratum, ... - every stretch of a few times S slots holds the same mix of heavy and light tiles.
// S = 61: a prime that does not divide a CU count, so that the first tiles of the eight waves of a workgroup (slots wave x grid + block)
// come from eight different strata.
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int gnn_tile_schedule_build(int64_t slots, const int64_t *cost, int64_t waves, int kind, int32_t *order)
{
    ARGCHK(slots >= 0 && slots < (int64_t)1 << 31 && order && (cost || kind == 0 || slots == 0), "slots / cost / order are required");
    ARGCHK(waves > 0 && (kind == 0 || kind == 1), "waves must be positive, kind 0 (identity) or 1 (balanced)");
    if (kind == 0) {
        for (int64_t s = 0; s < slots; ++s) order[s] = (int32_t)s;
        return GNN_OK;
    }
    try {
        std::vector<int32_t> sorted((size_t)slots);
        for (int64_t s = 0; s < slots; ++s) sorted[s] = (int32_t)s;
        std::sort(sorted.begin(), sorted.end(), [&](int32_t x, int32_t y) { return cost[x] != cost[y] ? cost[x] > cost[y] : x < y; });
        const int64_t K = std::min(2 * waves, slots / 2), M = slots - K;
        const int64_t S = GNN_TILE_SCHEDULE_STRATA, C = (M + S - 1) / S;
        int64_t p = 0;
        for (int64_t q = 0; q < C; ++q)
            for (int64_t r = 0; r < S; ++r)
                if (r * C + q < M) order[p++] = sorted[r * C + q];
        for (int64_t t = M; t < slots; ++t) order[p++] = sorted[t];
    } catch (const std::bad_alloc &) { return gnn_fail(GNN_ERR_HIP, "no host memory for a schedule of %lld tiles", (long long)slots); }
    return GNN_OK;
}

// Slot headers of schedule `kind` (0 identity, 1 balanced) of g's program on g's device: gp_slot[kind] [slots][4] = {first batch, batches,
// tile id, 0}, from the headers and costs gnn_gather_program_ensure kept on the host.  The identity's array is built with the program (a
// graph without it has no program); the balanced one on first demand, once per graph and device CU count.  false: no such array (no
// program, or no memory - the launch then keeps the ascending order).
bool gnn_tile_schedule_ensure(const gnn_graph *g, int kind, int64_t waves)
{
    gnn_graph_shared *sh = g->sh;
    if (!sh->gp_ent || kind < 0 || kind > 1) return false;
    if (sh->gp_slot[kind]) return kind == 0 || sh->gp_sched_waves == waves;      // (one device per graph: the CU count does not change)
    if (kind == 1 && sh->gp_sched_tried) return false;
    if (kind == 1) sh->gp_sched_tried = true;
    const int64_t slots = (int64_t)sh->gp_cost.size();
    int dev_before = -1;
    if (hipGetDevice(&dev_before) != hipSuccess || hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return false; }
    const auto t0 = std::chrono::steady_clock::now();
    int32_t *d_slot = nullptr;
    bool ok = false;
    try {
        // entry format 4: the row weights of every slot's tile behind the headers, in slot order - a launch finds them from its ticket alone
        const bool roww = sh->gp_entries == 4;
        std::vector<int32_t> order((size_t)slots), slot((size_t)slots * (roww ? 36 : 4));
        ok = gnn_tile_schedule_build(slots, sh->gp_cost.data(), waves, kind, order.data()) == GNN_OK;
        for (int64_t s = 0; ok && s < slots; ++s) {
            const int32_t t = order[s];
            slot[4 * s] = sh->gp_hdr_host[2 * (size_t)t]; slot[4 * s + 1] = sh->gp_hdr_host[2 * (size_t)t + 1]; slot[4 * s + 2] = t; slot[4 * s + 3] = 0;
            if (roww) memcpy(&slot[4 * (size_t)slots + 32 * (size_t)s], &sh->gp_roww_host[32 * (size_t)t], 32 * sizeof(float));
        }
        ok = ok && gnn_dev_malloc((void **)&d_slot, sizeof(int32_t) * std::max<size_t>(4, slot.size())) == hipSuccess &&
             hipMemcpy(d_slot, slot.data(), sizeof(int32_t) * slot.size(), hipMemcpyHostToDevice) == hipSuccess;
    } catch (const std::bad_alloc &) { ok = false; }
    if (ok) {
        sh->gp_slot[kind] = d_slot;
        if (kind == 1) {
            sh->gp_sched_waves = waves;
            sh->gp_sched_tail = std::min(2 * waves, slots / 2);
            sh->gp_sched_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
    } else {
        (void)hipFree(d_slot);
        (void)hipGetLastError();
    }
    (void)hipSetDevice(dev_before);
    return ok;
}

extern "C" int gnn_graph_tile_schedule_info(const gnn_graph *g, int64_t *slots, int *kind, int64_t *body, int64_t *tail, float *build_ms)
{
    ARGCHK(g, "graph is NULL");
    const gnn_graph_shared *sh = g->sh;
    const bool have = sh->gp_ent != nullptr, balanced = have && sh->gp_slot[1] != nullptr;
    const int64_t n = have ? (int64_t)sh->gp_cost.size() : 0;
    if (slots) *slots = n;
    if (kind) *kind = balanced ? 2 : (have ? 1 : 0);
    if (body) *body = balanced ? n - sh->gp_sched_tail : n;
    if (tail) *tail = balanced ? sh->gp_sched_tail : 0;
    if (build_ms) *build_ms = balanced ? sh->gp_sched_ms : 0.0f;
    return GNN_OK;
}

// The program of g's graph on g's device, built once (with the first fused Loop, or the first gnn_loop_set_gather_form, that takes gather
// form 2).  Never an error: a graph whose program cannot be built or kept keeps walking the CSR (sh->gp_ent stays nullptr).  The attempt is
// made ONCE per graph (gp_tried): a graph that failed for want of memory is not tried again when memory has become free.
// A partial last tile gets a program too: the builder on that tile's 33 row pointers, the rows past the end repeating the last offset - empty
// rows, one GNN_GP_NOROW | GNN_GP_ROW_END slot each, an exact +0 aggregate as the CSR walk gives them.  Its batches follow the full tiles'
// in gp_ent; its header stays on the host (gp_last_first, gp_last_nb), so that gp_hdr / gp_tiles keep describing the full tiles only, and
// reaches the kernel as the last slot of the ascending tile schedule (gnn_tile_schedule_ensure), an ordinary slot of the balanced one.
// The device holds ONE entry format per graph (gp_entries): the 8-byte program is built on the host, compacted where every row's weights
// are one bit pattern (gather_program_compact; the partial last tile's program too), and only the format taken is copied to the device.
int gnn_gather_program_ensure(const gnn_graph *g)
{
    gnn_graph_shared *sh = g->sh;
    if (sh->gp_tried) return GNN_OK;
    sh->gp_tried = true;
    const int64_t tiles = g->n_rows / 32, rem = g->n_rows % 32;
    if (tiles == 0) return GNN_OK;
    // the caller may be a setter outside any run: the copies and allocations below belong on the graph's device, whatever device is current
    int dev_before = -1;
    if (hipGetDevice(&dev_before) != hipSuccess || hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return GNN_OK; }
    const auto t0 = std::chrono::steady_clock::now();
    int32_t *d_hdr = nullptr, *d_ent = nullptr;
    int64_t batches = 0, last_batches = 0;
    int32_t last_hdr[2] = {0, 0};
    std::vector<int32_t> hdr_host;
    std::vector<int64_t> cost;
    std::vector<float> roww_host;
    int entries = 8;
    bool ok = false;
    try {
        std::vector<int32_t> indptr((size_t)g->n_rows + 1), hdr((size_t)tiles * 2), src, ent;
        std::vector<float> w;
        ok = hipMemcpy(indptr.data(), sh->indptr, sizeof(int32_t) * indptr.size(), hipMemcpyDeviceToHost) == hipSuccess;
        const size_t E = ok ? (size_t)indptr.back() : 0;
        if (rem) indptr.resize((size_t)(tiles + 1) * 32 + 1, indptr.back());
        src.resize(E); w.resize(E);
        ok = ok && (E == 0 || (hipMemcpy(src.data(), sh->adj_src, sizeof(int32_t) * E, hipMemcpyDeviceToHost) == hipSuccess &&
                               hipMemcpy(w.data(), sh->adj_w, sizeof(float) * E, hipMemcpyDeviceToHost) == hipSuccess));
        // what the builder would refuse is looked for here, so that a graph without a program leaves no error text behind a Loop that succeeds
        for (size_t e = 0; ok && e < E; ++e) ok = src[e] >= 0 && src[e] < (1 << 23);
        const int32_t *last_ip = indptr.data() + tiles * 32;          // the partial tile's 33 row pointers (offsets into the same arc arrays)
        ok = ok && gnn_gather_program_build(tiles * 32, indptr.data(), src.data(), w.data(), hdr.data(), nullptr, &batches) == GNN_OK;
        if (ok && rem) ok = gnn_gather_program_build(32, last_ip, src.data(), w.data(), last_hdr, nullptr, &last_batches) == GNN_OK;
        ok = ok && batches + last_batches < ((int64_t)1 << 31) / 64;
        if (ok) {
            ent.resize((size_t)(batches + last_batches) * 128);
            ok = gnn_gather_program_build(tiles * 32, indptr.data(), src.data(), w.data(), nullptr, ent.data(), &batches) == GNN_OK;
            if (ok && rem) ok = gnn_gather_program_build(32, last_ip, src.data(), w.data(), nullptr, ent.data() + (size_t)batches * 128, &last_batches) == GNN_OK;
        }
        // the compact format where every row's weights are one bit pattern (and gnn_graph_set_program_entries did not ask for 8): the
        // device then holds the source words alone, the partial last tile's behind the full tiles' as before.  (A graph without arcs has no
        // weight to share - its program is empty rows' entries and padding - and keeps the 8-byte format unless 4 is asked for.)
        if (ok && sh->gp_entries_req != 8 && (E > 0 || sh->gp_entries_req == 4)) {
            std::vector<int32_t> words(ent.size() / 2);
            roww_host.assign((size_t)(tiles + (rem ? 1 : 0)) * 32, 0.0f);
            const int32_t last_rel[2] = {0, (int32_t)last_batches};
            if (gather_program_compact(tiles, hdr.data(), ent.data(), words.data(), roww_host.data()) &&
                (!rem || gather_program_compact(1, last_rel, ent.data() + (size_t)batches * 128, words.data() + (size_t)batches * 64, roww_host.data() + (size_t)tiles * 32))) {
                ent.swap(words);
                entries = 4;
            } else roww_host.clear();
        }
        ok = ok && gnn_dev_malloc((void **)&d_hdr, sizeof(int32_t) * hdr.size()) == hipSuccess &&
             gnn_dev_malloc((void **)&d_ent, sizeof(int32_t) * ent.size()) == hipSuccess &&
             hipMemcpy(d_hdr, hdr.data(), sizeof(int32_t) * hdr.size(), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(d_ent, ent.data(), sizeof(int32_t) * ent.size(), hipMemcpyHostToDevice) == hipSuccess;
        if (ok) {   // what a tile schedule is built from: header and real entries (arcs) of every slot, the partial last tile an ordinary one
            hdr_host = hdr;
            if (rem) { hdr_host.push_back((int32_t)batches); hdr_host.push_back(last_hdr[1]); }
            cost.resize((size_t)(tiles + (rem ? 1 : 0)));
            for (size_t t = 0; t < cost.size(); ++t) cost[t] = (int64_t)indptr[(t + 1) * 32] - indptr[t * 32];
        }
    } catch (const std::bad_alloc &) { ok = false; }
    if (ok) {
        sh->gp_hdr = d_hdr; sh->gp_ent = d_ent; sh->gp_tiles = tiles; sh->gp_batches = batches + last_batches;
        sh->gp_rows = g->n_rows; sh->gp_last_first = (int32_t)batches; sh->gp_last_nb = (int32_t)last_batches;
        sh->gp_hdr_host.swap(hdr_host); sh->gp_cost.swap(cost);
        sh->gp_entries = entries; sh->gp_roww_host.swap(roww_host);
        // the kernel finds every tile through a slot header: a program without the ascending schedule's array is no program
        if (!gnn_tile_schedule_ensure(g, 0, 1)) {
            (void)hipFree(d_hdr); (void)hipFree(d_ent);
            sh->gp_hdr = sh->gp_ent = nullptr; sh->gp_tiles = sh->gp_batches = 0; sh->gp_entries = 0;
            (void)hipGetLastError();
        }
        sh->gp_build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    } else {
        (void)hipFree(d_hdr); (void)hipFree(d_ent);
        (void)hipGetLastError();                                   // (an allocation failure is not this Loop's error)
    }
    (void)hipSetDevice(dev_before);
    return GNN_OK;
}

extern "C" int gnn_graph_gather_program_info(const gnn_graph *g, int64_t *tiles, int64_t *batches, int64_t *bytes, float *build_ms)
{
    ARGCHK(g, "graph is NULL");
    const gnn_graph_shared *sh = g->sh;
    const bool have = sh->gp_ent != nullptr;
    if (tiles) *tiles = have ? sh->gp_tiles : 0;
    if (batches) *batches = have ? sh->gp_batches : 0;
    // (entry format 4: 256 bytes per batch, and the row-weight block of one tile schedule, 128 bytes per slot)
    if (bytes) *bytes = !have ? 0 : sh->gp_entries == 4 ? sh->gp_tiles * 8 + sh->gp_batches * 256 + (int64_t)sh->gp_cost.size() * 128
                                                        : sh->gp_tiles * 8 + sh->gp_batches * 512;
    if (build_ms) *build_ms = have ? sh->gp_build_ms : 0.0f;
    return GNN_OK;
}

extern "C" int gnn_graph_gather_program_format(const gnn_graph *g, int *entries)
{
    ARGCHK(g && entries, "graph / entries are NULL");
    *entries = g->sh->gp_ent ? g->sh->gp_entries : 0;
    return GNN_OK;
}

// Drops the graph's program and its tile schedules (the next form decision of a Loop rebuilds them) and records the entry format to
// build.  Where the graph had a program, or a format is asked for, the program is rebuilt at once, so that *used is the format the graph
// holds from now on.  The caller's Loops on this graph (and on the graphs derived from it) are idle: hipFree waits for the device.
extern "C" int gnn_graph_set_program_entries(gnn_graph *g, int entries, int *used)
{
    ARGCHK(g, "graph is NULL");
    ARGCHK(entries == 0 || entries == 4 || entries == 8, "entries must be 0 (the library's choice), 4 or 8");
    gnn_graph_shared *sh = g->sh;
    const bool had = sh->gp_ent != nullptr;
    int dev_before = -1;
    HIPCHK(hipGetDevice(&dev_before));
    HIPCHK(hipSetDevice(g->device));
    (void)hipFree(sh->gp_hdr); (void)hipFree(sh->gp_ent); (void)hipFree(sh->gp_slot[0]); (void)hipFree(sh->gp_slot[1]);
    (void)hipSetDevice(dev_before);
    sh->gp_hdr = sh->gp_ent = sh->gp_slot[0] = sh->gp_slot[1] = nullptr;
    sh->gp_tiles = sh->gp_batches = sh->gp_rows = 0;
    sh->gp_last_first = sh->gp_last_nb = 0;
    sh->gp_hdr_host.clear(); sh->gp_cost.clear(); sh->gp_roww_host.clear();
    sh->gp_sched_waves = sh->gp_sched_tail = 0;
    sh->gp_tried = sh->gp_sched_tried = false;
    sh->gp_entries = 0;
    sh->gp_entries_req = entries;
    if (had || entries) gnn_gather_program_ensure(g);
    if (used) *used = sh->gp_ent ? sh->gp_entries : 0;
    return GNN_OK;
}
