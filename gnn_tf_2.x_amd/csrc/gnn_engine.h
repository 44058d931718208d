// What crosses a unit boundary of the inference engine (gnn_engine.hip: errors, allocation, the primitive kernels and their launchers, the
// MLP handle, the RCCL table; gnn_graph.hip: the graph handle and the LGNN relabelling; gnn_comm.hip: communicators and the three exchange
// layouts; gnn_loop.hip: the Loop handle and its run functions).  Internal, not installed.
#pragma once
#include <algorithm>

#include "gnn_common.h"

static inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

template <typename T>
static int dev_alloc(T **p, size_t count)
{
    *p = nullptr;
    if (count == 0) count = 1;
    HIPCHK(gnn_dev_malloc((void **)p, count * sizeof(T)));
    return GNN_OK;
}

template <typename T>
static int dev_upload(T **p, const T *host, size_t count)
{
    int rc = dev_alloc(p, count);
    if (rc) return rc;
    if (count) HIPCHK(hipMemcpy(*p, host, count * sizeof(T), hipMemcpyHostToDevice));
    return GNN_OK;
}

static inline int zero_on_stream(void *p, size_t bytes, hipStream_t st)
{
    if (!bytes) return GNN_OK;
    HIPCHK(hipMemsetAsync(p, 0, bytes, st));
    return GNN_OK;
}

// "The state after k bodies" of a loop's last run, for every reader (host and device).  Bodies ping-pong between state[0] and state[1]:
// body k writes state[(k + 1) & 1], so k >= 1 bodies leave the state in state[k & 1].  k == 0 is the initial state: a per-body run on one
// GPU with D > 0 reads it where gnn_loop_set_state0 put it (l->init_in_place: state_init is then a full table of N_pad rows with a
// zeroed tail, never written by a run); every other run - sharded, D == 0, persistent, training - has copied it into state[0].
struct GnnStateTabs { const float *init, *s0, *s1; };
__host__ __device__ __forceinline__ const float *gnn_state_after(const GnnStateTabs &t, int k) { return k == 0 ? t.init : ((k & 1) ? t.s1 : t.s0); }
// the three tables from replica row `row_off` on (l->own_off: the owned rows; 0: the replica)
static inline GnnStateTabs gnn_loop_state_tabs(const gnn_loop *l, size_t row_off)
{
    const size_t o = row_off * (size_t)l->Ds;
    return GnnStateTabs{(l->init_in_place ? l->state_init : l->state[0]) + o, l->state[0] + o, l->state[1] + o};
}
static inline const float *gnn_loop_state_after(const gnn_loop *l, int k, size_t row_off) { return gnn_state_after(gnn_loop_state_tabs(l, row_off), k); }

// gnn_engine.hip
GNN_INTERNAL int launch_check(hipStream_t st, int64_t n_rows, int d, const float *s, const float *so, float thr, int *flag_out, const int *gate, int world);
GNN_INTERNAL int launch_check_first(hipStream_t st, int64_t n_rows, int d, const float *s, float thr, int *flag_out);
GNN_INTERNAL int launch_mlp(hipStream_t st, const gnn_mlp *m, int64_t n, const float *X, int64_t ldx, float *Y, int64_t ldy, float *t0, float *t1,
                            const int *gate, int world);

// gnn_engine.hip: RCCL, loaded lazily so that the library itself has no link-time dependency on it
struct Id128 { char b[128]; };   // ncclUniqueId, passed by value
struct GNN_INTERNAL Rccl {
    void *h = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, Id128, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
GNN_INTERNAL extern Rccl g_rccl;
GNN_INTERNAL int rccl_load();
enum { NCCL_INT32 = 2, NCCL_FLOAT32 = 7, NCCL_FLOAT64 = 8, NCCL_MAX = 2 };

#define NCCLCHK(expr)                                                                                   \
    do {                                                                                                \
        int r_ = (expr);                                                                                \
        if (r_ != 0) return gnn_fail(GNN_ERR_COMM, "%s -> %s", #expr, g_rccl.GetErrorString(r_));      \
    } while (0)

// the exchange steps of the sharded loop (gnn_comm.hip); flag_off == NO_FLAGS: no flag words travel
static const size_t NO_FLAGS = ~(size_t)0;
GNN_INTERNAL int loop_exchange(gnn_loop *l, int b, size_t flag_off);
GNN_INTERNAL int slice_step_pack(gnn_loop *l, int k);
GNN_INTERNAL int slice_step_aggregate(gnn_loop *l, int k);
GNN_INTERNAL int slice_step_unpack(gnn_loop *l, int k);
// dst[r, :] = own[rows[r], :] for r < count: the boundary rows of a halo shard, packed for the exchange (state rows, relabelled node labels)
GNN_INTERNAL int gnn_launch_pack_rows(hipStream_t st, int64_t count, int Ds, const int32_t *rows, const float *own, float *dst);
