// Communicators of the gfx950 engine and the exchange steps of the sharded Loop: whole rows, boundary rows, feature slices.  The RCCL table
// they call through is loaded by gnn_engine.hip (rccl_load).
#include <stdlib.h>
#include <string.h>

#include "gnn_engine.h"

extern "C" int gnn_comm_unique_id(uint8_t id[128])
{
    ARGCHK(id, "id is NULL");
    int rc = rccl_load();
    if (rc) return rc;
    NCCLCHK(g_rccl.GetUniqueId(id));
    return GNN_OK;
}

extern "C" int gnn_comm_create(const uint8_t id[128], int rank, int world, int device, gnn_comm **out)
{
    ARGCHK(id && out && world >= 1 && rank >= 0 && rank < world, "bad arguments");
    *out = nullptr;
    int rc = rccl_load();
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    gnn_comm *c = new gnn_comm();
    c->rank = rank; c->world = world; c->device = device;
    Id128 uid;
    memcpy(uid.b, id, 128);
    int r = g_rccl.CommInitRank(&c->nccl, world, uid, rank);
    if (r != 0) { delete c; return gnn_fail(GNN_ERR_COMM, "ncclCommInitRank -> %s", g_rccl.GetErrorString(r)); }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || gnn_dev_malloc((void **)&c->scratch, sizeof(double)) != hipSuccess) {
        gnn_comm_destroy(c);
        return gnn_fail(GNN_ERR_HIP, "communicator stream / scratch allocation failed");
    }
    *out = c;
    return GNN_OK;
}

// `world` communicators on ONE device sharing one stream (see gnn_comm_group): the sharded engine path on a single GPU.
extern "C" int gnn_comm_create_loopback(int world, int device, gnn_comm **out /* [world] */)
{
    ARGCHK(out && world >= 1 && world <= 64, "bad arguments");
    for (int r = 0; r < world; ++r) out[r] = nullptr;
    HIPCHK(hipSetDevice(device));
    gnn_comm_group *grp = new gnn_comm_group();
    grp->world = world;
    grp->member.assign((size_t)world, nullptr);
    hipError_t e = hipStreamCreateWithFlags(&grp->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete grp; return gnn_fail(GNN_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    for (int r = 0; r < world; ++r) {
        gnn_comm *c = new gnn_comm();
        c->rank = r; c->world = world; c->device = device; c->grp = grp; c->stream = grp->stream;
        grp->refs++;
        out[r] = c;
    }
    return GNN_OK;
}

extern "C" int gnn_comm_allreduce_max(gnn_comm *c, double *value)
{
    ARGCHK(c && value, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    if (c->grp) { HIPCHK(hipStreamSynchronize(c->stream)); return GNN_OK; }   // one process: the value is already the maximum
    HIPCHK(hipMemcpyAsync(c->scratch, value, sizeof(double), hipMemcpyHostToDevice, c->stream));
    NCCLCHK(g_rccl.AllReduce(c->scratch, c->scratch, 1, NCCL_FLOAT64, NCCL_MAX, c->nccl, c->stream));
    HIPCHK(hipMemcpyAsync(value, c->scratch, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GNN_OK;
}

int gnn_comm_allgather32(gnn_comm *c, const void *send, void *recv, size_t count, hipStream_t st)
{
    if (!c || c->grp || !c->nccl) return gnn_fail(GNN_ERR_UNSUPPORTED, "this exchange needs an RCCL communicator (one process per rank), not a loopback group");
    NCCLCHK(g_rccl.AllGather(send, recv, count, NCCL_INT32, c->nccl, st));
    return GNN_OK;
}

extern "C" int gnn_comm_destroy(gnn_comm *c)
{
    if (!c) return GNN_OK;
    if (c->loops > 0) { c->closed = true; return GNN_OK; }      // released by the last gnn_loop_destroy
    (void)hipSetDevice(c->device);
    if (c->grp) {
        if (--c->grp->refs == 0) { (void)hipStreamDestroy(c->grp->stream); delete c->grp; }
        if (c->xstream) (void)hipStreamDestroy(c->xstream);
        delete c;
        return GNN_OK;
    }
    if (c->nccl && g_rccl.CommDestroy) g_rccl.CommDestroy(c->nccl);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->xstream) (void)hipStreamDestroy(c->xstream);
    (void)hipFree(c->scratch);
    delete c;
    return GNN_OK;
}

extern "C" int gnn_shard_range(int64_t n_nodes, int rank, int world, int64_t *row_begin, int64_t *n_rows)
{
    ARGCHK(n_nodes > 0 && world >= 1 && rank >= 0 && rank < world && row_begin && n_rows, "bad arguments");
    const int64_t shard = ((n_nodes + world - 1) / world + 31) / 32 * 32;   // whole 32-node tiles per rank
    const int64_t b = std::min<int64_t>(n_nodes, shard * rank), e = std::min<int64_t>(n_nodes, shard * (rank + 1));
    *row_begin = b;
    *n_rows = e - b;
    return GNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// exchange step of the sharded loop (reference: the reads of `state` at GNN/GNN.py:234 and the global reduce_any at :218
// span all nodes; here every rank owns a node range).  One call = "everybody gets the owned state rows of buffer `b` and the
// flag words at int offset `flag_off` of every rank".  b < 0 / flag_off == NO_FLAGS skip that part.
//   RCCL communicator      one grouped call: in-place all-gather of the owned rows (full replicas) or of the packed
//                          boundary rows (halo shards) + all-gather of the rank's flag block
//   loopback communicator  the same data movement as device-to-device copies into the other members' buffers, on the
//                          group's single stream (so ordering is program order)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_pack_rows(int64_t count, int Ds, const int32_t *__restrict__ rows, const float *__restrict__ own, float *__restrict__ dst)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * Ds) return;
    const int64_t r = t / Ds;
    const int c = (int)(t - r * Ds);
    dst[t] = own[(int64_t)rows[r] * Ds + c];
}

int gnn_launch_pack_rows(hipStream_t st, int64_t count, int Ds, const int32_t *rows, const float *own, float *dst)
{
    hipLaunchKernelGGL(k_pack_rows, cdiv(count * Ds, 256), 256, 0, st, count, Ds, rows, own, dst);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

// replica segment this rank publishes: [seg_off, seg_off + seg_rows) rows of the state replica
static inline void loop_segment(const gnn_loop *l, int rank, size_t *off_rows, size_t *rows)
{
    const gnn_graph *g = l->g;
    if (g->halo_world) { *off_rows = (size_t)l->shard_rows + (size_t)rank * g->halo_block; *rows = (size_t)g->halo_block; }
    else { *off_rows = (size_t)l->shard_rows * rank; *rows = (size_t)l->shard_rows; }
}

int loop_exchange(gnn_loop *l, int b, size_t flag_off)
{
    if (l->world == 1) return GNN_OK;
    const gnn_graph *g = l->g;
    size_t off = 0, rows = 0;
    loop_segment(l, l->rank, &off, &rows);
    if (b >= 0 && g->halo_world && g->halo_count) {      // boundary rows of the owned range -> this rank's block of the replica
        int rc = gnn_launch_pack_rows(l->stream, g->halo_count, l->Ds, g->halo_send, l->state[b] + (size_t)l->own_off * l->Ds, l->state[b] + off * l->Ds);
        if (rc) return rc;
    }
    if (l->comm->grp) {
        gnn_comm_group *grp = l->comm->grp;
        for (int p = 0; p < l->world; ++p) {
            gnn_loop *peer = grp->member[p];
            if (p == l->rank) continue;
            if (!peer) return gnn_fail(GNN_ERR_STATE, "loopback rank %d has no loop: create one loop per rank and run them with gnn_loop_run_group", p);
            if (b >= 0 && rows)
                HIPCHK(hipMemcpyAsync(peer->state[b] + off * l->Ds, l->state[b] + off * l->Ds, sizeof(float) * rows * l->Ds, hipMemcpyDeviceToDevice, l->stream));
            if (flag_off != NO_FLAGS)
                HIPCHK(hipMemcpyAsync(peer->flags + flag_off + (size_t)l->rank * GNN_FLAG_WORDS, l->flags + flag_off + (size_t)l->rank * GNN_FLAG_WORDS,
                                      sizeof(int) * GNN_FLAG_WORDS, hipMemcpyDeviceToDevice, l->stream));
        }
        return GNN_OK;
    }
    size_t base = 0, unused = 0;
    loop_segment(l, 0, &base, &unused);
    NCCLCHK(g_rccl.GroupStart());
    if (b >= 0 && rows)
        NCCLCHK(g_rccl.AllGather(l->state[b] + off * l->Ds, l->state[b] + base * l->Ds, rows * l->Ds, NCCL_FLOAT32, l->comm->nccl, l->stream));
    if (flag_off != NO_FLAGS)
        NCCLCHK(g_rccl.AllGather(l->flags + flag_off + (size_t)l->rank * GNN_FLAG_WORDS, l->flags + flag_off, GNN_FLAG_WORDS, NCCL_INT32, l->comm->nccl, l->stream));
    NCCLCHK(g_rccl.GroupEnd());
    return GNN_OK;
}

// ---- feature-sliced exchange --------------------------------------------------------------------------------------------
// The aggregation state_agg = Adjacency^T . state (GNN.py:234) is independent per COLUMN of the state.  Instead of handing every
// rank every row of the state (full or boundary replicas: (P - 1) / P of N Ds floats received per rank and iteration), rank q
// aggregates columns [q Cs, (q + 1) Cs), Cs = Ds / P, for ALL nodes over the whole graph's adjacency, and two all-to-all steps move
// column slices in and aggregated slices back: 2 (P - 1) / P of (N / P) Ds floats per rank and iteration, P / 2 times less
// (56 MB instead of 224 MB at N = 1 M, Ds = 64, P = 8).  The fmaf chain of an aggregated element is the same CSR-ordered chain
// as in the replicated layouts, so the results are bit-identical.
// VEC = 4 when Cs is a multiple of 4 (16-byte pieces), else 1; one thread per piece
template <int VEC>
__global__ void k_slice_pack(int64_t n_rows, int64_t shard_rows, int Ds, int Cs, const float *__restrict__ own, float *__restrict__ send,
                             const int *gate, int world)
{
    if (!gnn_gate_open_block(gate, world)) return;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int pr = Ds / VEC;                                        // pieces per row
    if (t >= shard_rows * pr) return;
    const int64_t r = t / pr;
    const int f = (int)(t - r * pr) * VEC, q = f / Cs, c = f - q * Cs;
    float *dst = send + ((size_t)q * shard_rows + r) * Cs + c;
    if (VEC == 4) *reinterpret_cast<float4 *>(dst) = r < n_rows ? *reinterpret_cast<const float4 *>(own + r * Ds + f) : float4{0.f, 0.f, 0.f, 0.f};
    else *dst = r < n_rows ? own[r * Ds + f] : 0.0f;               // padding rows of a short shard travel as zeros
}

template <int VEC>
__global__ void k_slice_unpack(int64_t n_rows, int64_t shard_rows, int Ds, int Cs, const float *__restrict__ recv, float *__restrict__ agg,
                               const int *gate, int world)
{
    if (!gnn_gate_open_block(gate, world)) return;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int pr = Ds / VEC;
    if (t >= n_rows * pr) return;
    const int64_t r = t / pr;
    const int f = (int)(t - r * pr) * VEC, q = f / Cs, c = f - q * Cs;
    const float *src = recv + ((size_t)q * shard_rows + r) * Cs + c;
    if (VEC == 4) *reinterpret_cast<float4 *>(agg + r * Ds + f) = *reinterpret_cast<const float4 *>(src);
    else agg[r * Ds + f] = *src;
}

// all-to-all of equal blocks: block q of `send` goes to rank q, which stores it as block `rank` of its `recv`
// (which: 0 = sl_send -> peers' sl_state, 1 = sl_agg -> peers' sl_recv)
static int slice_alltoall(gnn_loop *l, int which)
{
    const size_t block = (size_t)l->shard_rows * l->Cs;
    float *send = which == 0 ? l->sl_send : l->sl_agg;
    if (l->comm->grp) {
        gnn_comm_group *grp = l->comm->grp;
        for (int p = 0; p < l->world; ++p) {
            gnn_loop *peer = grp->member[p];
            if (!peer) return gnn_fail(GNN_ERR_STATE, "loopback rank %d has no loop: create one loop per rank and run them with gnn_loop_run_group", p);
            if (!peer->slice_mode) return gnn_fail(GNN_ERR_STATE, "rank %d does not use the feature-sliced exchange", p);
            float *dst = (which == 0 ? peer->sl_state : peer->sl_recv) + (size_t)l->rank * block;
            HIPCHK(hipMemcpyAsync(dst, send + (size_t)p * block, sizeof(float) * block, hipMemcpyDeviceToDevice, l->stream));
        }
        return GNN_OK;
    }
    float *recv = which == 0 ? l->sl_state : l->sl_recv;
    // the rank's own block is a device copy; the other P - 1 pairs are one grouped send / receive each
    HIPCHK(hipMemcpyAsync(recv + (size_t)l->rank * block, send + (size_t)l->rank * block, sizeof(float) * block, hipMemcpyDeviceToDevice, l->stream));
    NCCLCHK(g_rccl.GroupStart());
    for (int p = 0; p < l->world; ++p) {
        if (p == l->rank) continue;
        NCCLCHK(g_rccl.Send(send + (size_t)p * block, block, NCCL_FLOAT32, p, l->comm->nccl, l->stream));
        NCCLCHK(g_rccl.Recv(recv + (size_t)p * block, block, NCCL_FLOAT32, p, l->comm->nccl, l->stream));
    }
    NCCLCHK(g_rccl.GroupEnd());
    return GNN_OK;
}

// the three steps of the sliced aggregation of body k; between them the other ranks of a loopback group take their turn
int slice_step_pack(gnn_loop *l, int k)
{
    const int *gate = l->flags + (size_t)k * l->world * GNN_FLAG_WORDS;
    const float *own = l->state[k & 1] + (size_t)l->own_off * l->Ds;
    if (l->Cs % 4 == 0)
        hipLaunchKernelGGL((k_slice_pack<4>), cdiv(l->shard_rows * (l->Ds / 4), 256), 256, 0, l->stream, l->g->n_rows, l->shard_rows, l->Ds, l->Cs, own,
                           l->sl_send, gate, l->world);
    else
        hipLaunchKernelGGL((k_slice_pack<1>), cdiv(l->shard_rows * l->Ds, 256), 256, 0, l->stream, l->g->n_rows, l->shard_rows, l->Ds, l->Cs, own,
                           l->sl_send, gate, l->world);
    HIPCHK(hipGetLastError());
    return slice_alltoall(l, 0);
}

// Aggregation of the rank's column slice + the return all-to-all.  Pipelined form (default): the rows are aggregated in P blocks, one per
// destination rank, in the order rank + 1, rank + 2, ..., rank (every step of the schedule is a permutation: at step t rank r sends
// to r + 1 + t and receives from r - 1 - t, so no link carries two blocks at once), and block t travels on the communicator's second
// stream while block t + 1 is aggregated on the loop's stream; only the last block (the rank's own: a device copy) is exposed.
int slice_step_aggregate(gnn_loop *l, int k)
{
    const gnn_graph *g = l->g;
    const int P = l->world;
    const int *gate = l->flags + (size_t)k * P * GNN_FLAG_WORDS;
    if (!l->sl_pipeline) {
        int rc = gnn_launch_spmm(l->stream, g->sh->full_rows, g->sh->full_indptr, g->sh->full_src, g->sh->full_w, l->sl_state, l->Cs, l->Cs, l->sl_agg, l->Cs, gate, P);
        if (rc) return rc;
        return slice_alltoall(l, 1);
    }
    gnn_comm *cm = l->comm;
    if (!cm->xstream) HIPCHK(hipStreamCreateWithFlags(&cm->xstream, hipStreamNonBlocking));
    if ((int)l->sl_ev.size() < P) {
        const size_t old = l->sl_ev.size();
        l->sl_ev.resize((size_t)P, nullptr);
        for (size_t i = old; i < l->sl_ev.size(); ++i) HIPCHK(hipEventCreateWithFlags(&l->sl_ev[i], hipEventDisableTiming));
    }
    if (!l->sl_done) HIPCHK(hipEventCreateWithFlags(&l->sl_done, hipEventDisableTiming));
    const size_t block = (size_t)l->shard_rows * l->Cs;
    for (int t = 0; t < P; ++t) {
        const int q = (l->rank + 1 + t) % P, from = ((l->rank - 1 - t) % P + P) % P;
        const int64_t r0 = (int64_t)q * l->shard_rows, r1 = std::min<int64_t>(r0 + l->shard_rows, g->sh->full_rows);
        if (r1 > r0) {
            int rc = gnn_launch_spmm(l->stream, r1 - r0, g->sh->full_indptr + r0, g->sh->full_src, g->sh->full_w, l->sl_state, l->Cs, l->Cs,
                                     l->sl_agg + (size_t)r0 * l->Cs, l->Cs, gate, P);
            if (rc) return rc;
        }
        HIPCHK(hipEventRecord(l->sl_ev[t], l->stream));
        HIPCHK(hipStreamWaitEvent(cm->xstream, l->sl_ev[t], 0));
        const float *src = l->sl_agg + (size_t)q * block;
        if (cm->grp) {
            gnn_loop *peer = cm->grp->member[q];
            if (!peer) return gnn_fail(GNN_ERR_STATE, "loopback rank %d has no loop: create one loop per rank and run them with gnn_loop_run_group", q);
            if (!peer->slice_mode) return gnn_fail(GNN_ERR_STATE, "rank %d does not use the feature-sliced exchange", q);
            HIPCHK(hipMemcpyAsync(peer->sl_recv + (size_t)l->rank * block, src, sizeof(float) * block, hipMemcpyDeviceToDevice, cm->xstream));
        } else if (q == l->rank) {
            HIPCHK(hipMemcpyAsync(l->sl_recv + (size_t)l->rank * block, src, sizeof(float) * block, hipMemcpyDeviceToDevice, cm->xstream));
        } else {
            NCCLCHK(g_rccl.GroupStart());
            NCCLCHK(g_rccl.Send(src, block, NCCL_FLOAT32, q, cm->nccl, cm->xstream));
            NCCLCHK(g_rccl.Recv(l->sl_recv + (size_t)from * block, block, NCCL_FLOAT32, from, cm->nccl, cm->xstream));
            NCCLCHK(g_rccl.GroupEnd());
        }
    }
    HIPCHK(hipEventRecord(l->sl_done, cm->xstream));
    return GNN_OK;
}

int slice_step_unpack(gnn_loop *l, int k)
{
    const int *gate = l->flags + (size_t)k * l->world * GNN_FLAG_WORDS;
    if (l->sl_pipeline) {          // the blocks of this rank's rows have arrived: its own transfers (RCCL: each carries the matching receive), or every member's (loopback: they push)
        if (l->comm->grp) {
            for (int p = 0; p < l->world; ++p) {
                gnn_loop *peer = l->comm->grp->member[p];
                if (peer && peer->sl_done) HIPCHK(hipStreamWaitEvent(l->stream, peer->sl_done, 0));
            }
        } else if (l->sl_done) HIPCHK(hipStreamWaitEvent(l->stream, l->sl_done, 0));
    }
    if (l->g->n_rows) {
        if (l->Cs % 4 == 0)
            hipLaunchKernelGGL((k_slice_unpack<4>), cdiv(l->g->n_rows * (l->Ds / 4), 256), 256, 0, l->stream, l->g->n_rows, l->shard_rows, l->Ds, l->Cs,
                               l->sl_recv, l->agg_own, gate, l->world);
        else
            hipLaunchKernelGGL((k_slice_unpack<1>), cdiv(l->g->n_rows * l->Ds, 256), 256, 0, l->stream, l->g->n_rows, l->shard_rows, l->Ds, l->Cs,
                               l->sl_recv, l->agg_own, gate, l->world);
        HIPCHK(hipGetLastError());
    }
    return GNN_OK;
}
