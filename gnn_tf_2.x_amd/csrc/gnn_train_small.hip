// Persistent training forward of small batches: the `while` of train_forward (gnn_train.hip, Forward::bodies_by_launch) for every body
// 0 .. max_iter - 1 of net_state in ONE launch, leaving exactly the per-body caches (NetCache) that the unchanged backward pass consumes.
//
// Shape: one 256-thread workgroup per BatchNormalization chunk of R = rows_per_block(n) rows (32, 48 or 64; at most 64 workgroups, one per
// CU).  Per body a workgroup
//   1. builds the concat rows of its R rows (template + own state + gather of the neighbours' state) - mlp_build_rows, k_mlp_fwd's code;
//   2. runs all Dense layers on them - mlp_layers, the dense_rows chains of k_mlp_fwd (an output's value does not depend on the rows per
//      tile) - and writes the concat rows and every layer's activations into THAT body's cache block;
//   3. with a trailing BatchNormalization: the statistics of its own chunk from LDS (bn_chunk_stats = k_bn_stats) -> grid barrier -> the
//      merge of all chunks in k_bn_apply's lane and chunk order (bn_merge_chunks), xhat and the new state of its rows, the [mean | var] row;
//   4. evaluates gate b + 1 = condition(state_{b+1}, state_b) for its rows and meets the others at the grid barrier that also publishes
//      the new state rows; the barrier word carries the verdict, so every workgroup leaves at the same body.
// That is one barrier per body (two with BatchNormalization) plus one in front of body 0 for gate 0.  Bodies behind the first closed gate
// are never computed.
//
// Hand-offs between workgroups (the new state rows; the chunk statistics) follow gnn_small_common.h, arrive_and_gate: write-through (sc1)
// stores, every storing wave drains them (s_waitcnt vmcnt(0)), workgroup barrier, ONE lane adds to the body's word with a relaxed
// agent-scope atomic and polls it (bounded: 1 << 22 polls, then the sticky status word in pinned host memory and return), workgroup
// barrier, and EVERY load of handed-off bytes is an sc1 load (tload<true>): cdna_hip_programming.md Guideline 16 (R1), MI355X_MICROARCH.md
// hand-off table, row 1.  Everything else a body writes (concat rows, hidden activations, xhat, statistics row) is read after the launch only.
#include "gnn_train.h"
#include "gnn_train_dev.h"
#include "gnn_small_common.h"

using namespace gnn_train;

namespace {

struct TrainSmall {
    MlpFwd m;                     // the net and the loop-invariant build fields; state / own / own_prev / X_out / Y are set per body
    const float *state0;          // the state body 0 reads
    float *cache;                 // body b's block: cache + b * body_floats
    size_t body_floats, off_a[GNN_FUSED_MAXL + 1], off_xhat, off_y, off_part;
    int max_iter, has_bn, softmax_last, cw_shift;
    float eps;
    const float *gamma, *beta;
    float *stats_all;             // [max_iter][2 F]
    int *words;                   // [1 + 2 max_iter] barrier + gate words, zeroed before the launch
    int *host_result;             // pinned host memory: [k, status]
};

// Grid barrier of the whole workgroup around arrive_and_gate (one-wave form): every wave drains its write-through stores, the workgroup
// meets, wave 0 arrives for it - `moved` of any thread enters the word - and polls; the verdict reaches the other waves through LDS behind
// a second workgroup barrier, which is also the barrier between the poll and their loads.  1 = go on, 0 = gate closed, -1 = gave up.
__device__ __forceinline__ int grid_arrive(const GnnSmallCtl &c, int word, int moved, int *verdict)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int any = __syncthreads_or(moved);
    if (threadIdx.x < 64) {
        const int r = gnn_fused_dev::arrive_and_gate(c, word, any, (int)threadIdx.x);
        if (threadIdx.x == 0) *verdict = r;
    }
    __syncthreads();
    return *verdict;
}

template <int R>
__global__ void __launch_bounds__(256) k_train_small(const TrainSmall a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int verdict;
    MlpFwd p = a.m;
    float *in = lds, *out = lds + (size_t)R * p.maxpad, *ps = lds + (size_t)2 * R * p.maxpad;
    // BatchNormalization's scratch takes the place of dense_rows' partial sums: s0 [256] | mu [32] | sc [3][256] | mean [F] | 1 / sqrt [F]
    float *s0 = ps, *mu = ps + 256, *sm = ps + 288 + 768, *sinv = sm + p.dims[p.L];
    float(*sc)[256] = reinterpret_cast<float(*)[256]>(ps + 288);
    const int64_t n = p.n, i0 = (int64_t)blockIdx.x * R, i1 = i0 + R < n ? i0 + R : n;
    const int Ds = p.Ds, F = p.dims[p.L], npad = p.pad[p.L];
    GnnSmallCtl ctl{};
    ctl.flags = a.words; ctl.host_result = a.host_result;
    const float *state = a.state0, *prev = nullptr;

    // gate 0 = condition(state_0, ones) (GNN.py:266, :271)
    int moved = 0;
    if ((int)threadIdx.x < R && i0 + threadIdx.x < n) {
        const float *own = state + (i0 + threadIdx.x) * Ds;
        moved = mlp_row_moved(Ds, p.thr, [&](int q) { return tload<true>(own + q); }, [](int) { return 1.0f; });
    }
    int run = grid_arrive(ctl, 0, moved, &verdict);
    int k = 0;
    while (run > 0) {
        float *blk = a.cache + (size_t)k * a.body_floats;
        p.state = state; p.own = state; p.own_prev = prev; p.X_out = blk;
        for (int l = 0; l < p.L; ++l) p.Y[l] = blk + a.off_a[l];
        mlp_build_rows<R, true, false>(p, i0, in);
        // (the last layer's output is the new state when nothing follows it: written through)
        float *h = (a.has_bn || a.softmax_last) ? mlp_layers<R, false>(p, i0, in, out, ps) : mlp_layers<R, true>(p, i0, in, out, ps);
        float *y_glob = p.Y[p.L - 1];
        if (a.softmax_last) {                      // k_act_fwd behind k_mlp_fwd: the row's softmax, in place
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (the pre-activations are stored before the rows are stored again)
            __syncthreads();
            if ((int)threadIdx.x < R && i0 + threadIdx.x < n) {
                float *hr = h + threadIdx.x * npad, *yr = y_glob + (i0 + threadIdx.x) * F;
                softmax_row(F, hr, hr);
                for (int j = 0; j < F; ++j) {
                    if (a.has_bn) yr[j] = hr[j];
                    else tstore<true>(yr + j, hr[j]);
                }
            }
            __syncthreads();
        }
        if (a.has_bn) {
            float *xhat = blk + a.off_xhat, *part = blk + a.off_part;
            y_glob = blk + a.off_y;
            for (int jb = 0; jb < F; jb += 1 << a.cw_shift) {
                if (jb) __syncthreads();           // (a state wider than 32: the column block before this one is done with s0 / mu)
                bn_chunk_stats<true>(F, a.cw_shift, jb, i0, i1, [&](int64_t r, int j) { return h[(r - i0) * npad + j]; }, part + (size_t)blockIdx.x * 2 * F, s0, mu);
            }
            if ((run = grid_arrive(ctl, 1 + 2 * k, 0, &verdict)) < 0) break;
            bn_merge_chunks<true>(n, F, a.cw_shift, part, (int)gridDim.x, R, a.eps, blockIdx.x == 0 ? a.stats_all + (size_t)k * 2 * F : nullptr, sm, sinv, sc);
            for (int t = threadIdx.x; t < (int)(i1 - i0) * F; t += blockDim.x) {
                const int r = t / F, j = t - r * F;
                float xh, y;
                bn_normalize(h[r * npad + j], sm[j], sinv[j], a.gamma[j], a.beta[j], &xh, &y);
                xhat[(i0 + r) * F + j] = xh;
                tstore<true>(y_glob + (i0 + r) * F + j, y);
                h[r * npad + j] = y;
            }
            __syncthreads();
        }
        // gate k + 1 = condition(state_{k+1}, state_k) for the workgroup's rows: the new rows from LDS, the old ones as body k read them
        moved = 0;
        if ((int)threadIdx.x < R && i0 + threadIdx.x < n) {
            const float *cur = h + threadIdx.x * npad, *old = state + (i0 + threadIdx.x) * Ds;
            moved = mlp_row_moved(Ds, p.thr, [&](int q) { return cur[q]; }, [&](int q) { return tload<true>(old + q); });
        }
        prev = state;
        state = y_glob;
        ++k;
        if (k == a.max_iter) break;
        run = grid_arrive(ctl, 2 * k, moved, &verdict);
    }
    if (run >= 0 && blockIdx.x == 0 && threadIdx.x == 0) a.host_result[0] = k;
}

template <int R>
const void *kernel_of() { return reinterpret_cast<const void *>(&k_train_small<R>); }

const void *kernel_for(int rows) { return rows == 32 ? kernel_of<32>() : rows == 48 ? kernel_of<48>() : rows == 64 ? kernel_of<64>() : nullptr; }

}   // namespace

namespace gnn_train {

int small_train_resident(int device, const SmallTrainForm &f, bool *ok)
{
    *ok = false;
    const void *kern = kernel_for(f.rows);
    if (!kern || device < 0 || device >= 64) return GNN_OK;
    static int n_cu[64] = {0};
    static bool raised[64] = {false};
    if (!n_cu[device]) {
        int v = 0;
        HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device));
        n_cu[device] = std::max(1, v);
    }
    if (!raised[device]) {
        for (int rows : {32, 48, 64}) HIPCHK(hipFuncSetAttribute(kernel_for(rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GNN_TRAIN_PERSISTENT_MAX_LDS));
        raised[device] = true;
    }
    int per_cu = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, f.lds));
    // (the launch asks for more than half a CU's LDS: a CU takes one workgroup, as the hand-off's measured form wants it)
    *ok = per_cu >= 1 && (int64_t)f.grid <= (int64_t)std::min(per_cu, 1) * n_cu[device];
    return GNN_OK;
}

int small_train_launch(hipStream_t st, const Net &net, const SmallTrainForm &f, const InputBuild &build, int max_iter, float *cache, int *words, int *host_result)
{
    const gnn_mlp *m = net.m;
    const int L = m->n_layers;
    TrainSmall a{};
    a.m.n = net.rows;
    mlp_fwd_describe(a.m, m, net.small_maxpad);
    a.m.build = 1; a.m.Ds = build.Ds; a.m.c_aggs = build.c_aggs; a.m.tmpl = build.tmpl; a.m.indptr = build.indptr; a.m.adj_src = build.adj_src;
    a.m.adj_w = build.adj_w; a.m.thr = build.thr;
    a.state0 = build.state;
    a.cache = cache; a.body_floats = f.body_floats;
    for (int l = 0; l < L; ++l) a.off_a[l] = f.off_a[l];
    a.off_xhat = f.off_xhat; a.off_y = f.off_y; a.off_part = f.off_part;
    a.max_iter = max_iter; a.has_bn = m->has_bn ? 1 : 0; a.softmax_last = m->acts[L - 1] == GNN_ACT_SOFTMAX ? 1 : 0;
    a.cw_shift = column_shift(m->dims[L]);
    a.eps = m->eps; a.gamma = net.gamma; a.beta = net.beta; a.stats_all = net.stats_all;
    a.words = words; a.host_result = host_result;
    switch (f.rows) {
    case 32: hipLaunchKernelGGL((k_train_small<32>), f.grid, 256, f.lds, st, a); break;
    case 48: hipLaunchKernelGGL((k_train_small<48>), f.grid, 256, f.lds, st, a); break;
    case 64: hipLaunchKernelGGL((k_train_small<64>), f.grid, 256, f.lds, st, a); break;
    default: return gnn_fail(GNN_ERR_STATE, "internal: no persistent training forward for %d rows per workgroup", f.rows);
    }
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

}   // namespace gnn_train
