// Host-side types and the functions that cross a unit boundary of the training step (gnn_train.hip: the step; gnn_train_net.hip: one
// Sequential in training mode; gnn_train_wide.hip: the matrix-core products; gnn_train_update.hip: clipping, regularizers, optimizer).
// Internal, not installed.
#pragma once
#include <algorithm>
#include <array>
#include <vector>

#include "gnn_engine.h"

// ---------------------------------------------------------------------------------------------------------------------
// Device scratch of the training step: a bump allocator over slabs that stay with the loop from step to step (a step makes
// a few hundred allocations; hipMalloc / hipFree for each of them dominated the step time).  reset() at the next forward.
struct GNN_INTERNAL gnn_train_arena {
    struct Slab { char *p; size_t size; };
    std::vector<Slab> slabs;
    size_t cur = 0, off = 0;
    void reset() { cur = 0; off = 0; peak = 0; }
    // scratch that is needed again and again (the adjoint iterations of gnn_train_adjoint.hip; the bodies of the recomputing step, gnn_train.hip): everything allocated after mark() is handed out
    // again after rewind() - the work that used it runs earlier on the same stream.  INVARIANT: nothing allocated between mark() and rewind()
    // may be remembered beyond it (a pointer cached on a Net, such as Net::part, would then alias later allocations): net_backward with
    // wgrad = false allocates per-call scratch only; the recomputing step allocates Net::part ahead of its mark
    struct Mark { size_t cur, off; };
    Mark mark() const { return Mark{cur, off}; }
    void rewind(const Mark &m) { cur = m.cur; off = m.off; }
    void *alloc(size_t bytes)
    {
        bytes = (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
        for (; cur < slabs.size(); ++cur, off = 0)
            if (off + bytes <= slabs[cur].size) {
                void *r = slabs[cur].p + off;
                off += bytes;
                note_peak();
                return r;
            }
        Slab s{nullptr, std::max<size_t>(bytes, (size_t)32 << 20)};
        if (gnn_dev_malloc((void **)&s.p, s.size) != hipSuccess) return nullptr;
        slabs.push_back(s);
        cur = slabs.size() - 1;
        off = bytes;
        note_peak();
        return s.p;
    }
    size_t peak = 0;              // most bytes in use since the last reset(): the slabs in front of the current one and its filled part
    void note_peak()
    {
        size_t used = off;
        for (size_t i = 0; i < cur; ++i) used += slabs[i].size;
        peak = std::max(peak, used);
    }
    struct Pinned {               // grow-only pinned host buffer
        void *p = nullptr;
        size_t bytes = 0;
        void *get(size_t want)
        {
            if (want > bytes) {
                if (p) (void)hipHostFree(p);
                p = nullptr; bytes = 0;
                if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return nullptr;
                bytes = want;
            }
            return p;
        }
        ~Pinned() { if (p) (void)hipHostFree(p); }
    };
    Pinned host;                  // pinned host words for the results the host waits for (iteration gates, loss partials)
    Pinned gates;                 // pinned words for the gates of the adjoint iterations (the backward pass of gradient mode 1 waits for them while `host` holds the step's loss partials)
    Pinned stage;                 // pinned staging for the small per-step uploads (targets, sample weights, NodeGraph CSR): packed by the host, one transfer
    ~gnn_train_arena() { for (Slab &s : slabs) (void)hipFree(s.p); }
};

namespace gnn_train GNN_INTERNAL {

using ::cdiv;

// rows handled by one block of the column reductions / weight-gradient tiles: about 64 blocks along the rows, so that small
// batches (a few hundred rows) still spread over the chip; a multiple of 16 (k_wgrad's row tile), at most 1024
inline int64_t rows_per_block(int64_t n)
{
    const int64_t r = ((n + 63) / 64 + 15) / 16 * 16;
    const int64_t capped = std::min<int64_t>(1024, std::max<int64_t>(32, r));
    // at most 256 row chunks: every chunk leaves a partial result that a second pass adds up in chunk order
    return std::max<int64_t>(capped, ((n + 255) / 256 + 15) / 16 * 16);
}

inline unsigned elementwise_grid(int64_t total) { return (unsigned)std::min<int64_t>(std::max<int64_t>(1, (total + 255) / 256), 2048); }

// ---- device code that two units inline ---------------------------------------------------------------------------------
// mix64, dropout_key, dropout_keep, alpha_dropout_coeffs: the Dropout masks of k_dropout_fwd (gnn_train_net.hip) and of k_train_input (gnn_train.hip: the Dropout in
// front of net_state's first layer rides on the concat) are one generator.  act_grad, dropout_grad: the way back through an activation /
// a Dropout is the epilogue of k_act_bwd, k_bn_bwd_apply, k_layer_bwd (gnn_train_net.hip) and of k_gemm_f32, k_gemm_split, k_bwd3_split
// (gnn_train_wide.hip).  All four are forced inline: a kernel's code does not depend on the unit it is compiled in.
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// One stream of mask bits per use: the key of the Dropout at position `pos` of net `net` (0 net_state, 1 net_output) in body `body`
// (net_output: 0) of a step with `seed`.  Element `index` of that mask - its flat index in the [rows of ALL ranks, width] matrix - is kept
// when the top 24 bits of mix64(key ^ mix64(index)) / 2^24 >= rate (dropout_keep).  The key is HASHED from its parts: keys made by adding
// multiples of constants to the seed met each other (seed + 7919 in body e drew the masks of seed in body e + 1), and neighbouring seeds
// are what callers pass.
__host__ __device__ __forceinline__ uint64_t dropout_key(uint64_t seed, int net, int body, int pos)
{
    return mix64(mix64(seed) ^ ((uint64_t)net << 56 | (uint64_t)(uint32_t)body << 16 | (uint64_t)(uint32_t)pos));
}

__device__ __forceinline__ uint8_t dropout_keep(uint64_t key, uint64_t index, float rate)
{
    return ((mix64(key ^ mix64(index)) >> 40) * (1.0f / 16777216.0f)) >= rate;
}

// AlphaDropout (Keras; reference GNN/MLP.py:59-61 with alphadropout=True) is passed as a NEGATIVE rate: dropped units are set to
// alpha' = -selu_scale * selu_alpha and the result is mapped by a x + b so that mean and variance of selu activations are kept:
//   a = ((1 - r)(1 + r alpha'^2))^-1/2,  b = -a alpha' r,  y = a (x keep + alpha' (1 - keep)) + b,  dy/dx = a keep
__device__ __forceinline__ void alpha_dropout_coeffs(float r, float *a, float *b, float *alpha_p)
{
    const float ap = -1.0507009873554805f * 1.6732632423543772f;
    const float aa = 1.0f / sqrtf((1.0f - r) * (1.0f + r * ap * ap));
    *a = aa; *b = -aa * ap * r; *alpha_p = ap;
}

// act'(z) as a function of the OUTPUT a alone (selu: z > 0 <=> a > 0 and scale * alpha * e^z = a + scale * alpha; elu: e^z = a + 1),
// so z is not kept.  Softmax is not elementwise: k_act_bwd.
__device__ __forceinline__ float act_grad(float aa, int act)
{
    switch (act) {
    case GNN_ACT_RELU: return aa > 0.0f ? 1.0f : 0.0f;
    case GNN_ACT_SELU: return aa > 0.0f ? 1.0507009873554805f : aa + 1.0507009873554805f * 1.6732632423543772f;
    case GNN_ACT_ELU: return aa > 0.0f ? 1.0f : aa + 1.0f;
    case GNN_ACT_TANH: return 1.0f - aa * aa;
    case GNN_ACT_SIGMOID: return aa * (1.0f - aa);
    default: return 1.0f;
    }
}

__device__ __forceinline__ float dropout_grad(float d, uint8_t keep, float rate)
{
    if (rate < 0.0f) {
        float a, b, ap;
        alpha_dropout_coeffs(-rate, &a, &b, &ap);
        return keep ? d * a : 0.0f;
    }
    return keep ? d / (1.0f - rate) : 0.0f;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct Buf {                      // typed front end of the arena
    gnn_train_arena *arena = nullptr;
    template <typename T>
    int get(T **p, size_t count)
    {
        *p = static_cast<T *>(arena->alloc(count * sizeof(T)));
        if (!*p) return gnn_fail(GNN_ERR_HIP, "hipMalloc of %zu bytes failed", count * sizeof(T));
        return GNN_OK;
    }
};

// Where the masks of one net_forward call come from when none are injected: the step's seed, which net and body this call is
// (dropout_key) and the row of the whole graph's matrix that the call's first row is (0 on one GPU; on shards the rows / masked rows of
// the lower ranks, so that a seed draws the same masks for any number of ranks).
struct MaskStream {
    uint64_t seed = 0;
    int net = 0, body = 0;
    int64_t row0 = 0;
};

struct NetCache {                 // what one training-mode forward of a Sequential leaves for the backward pass
    std::vector<float *> hin, a;
    std::vector<uint8_t *> keep;  // per dropout index 0..L (nullptr when no dropout there)
    float *xhat = nullptr, *stats = nullptr;
    int64_t n = 0;
};

struct Net {
    const gnn_mlp *m = nullptr;
    std::vector<float *> WT;      // W^T per layer
    float *gamma = nullptr, *beta = nullptr;
    std::vector<float> rate;      // [L + 1] dropout rate in front of Dense l (index L: in front of BatchNormalization)
    float *grads = nullptr;       // flat: dW1, db1, ..., dgamma, dbeta
    std::vector<size_t> g_off;
    size_t g_total = 0;
    float *part = nullptr;        // [chunks of the rows][g_total]: the partial gradients of ONE net_backward call
    int64_t part_rows = -1;
    // BatchNormalization on its MOVING statistics (the fixed-point gradient with GNN_ADJOINT_FROZEN_BN; net_freeze_bn): frozen [2 F] =
    // inv_j = 1 / sqrtf(var_mov_j + eps) | s_j = gamma_j inv_j, made once per step; no call is counted, stats_all stays zero
    float *frozen = nullptr;
    float *stats_all = nullptr;   // [max forward calls][2 F]: batch mean | biased batch variance of every BatchNormalization call, in call order
    int calls = 0, max_calls = 0;
    // The form every forward / backward call of this step takes, decided once by net_setup for the `rows` rows of each call:
    int64_t rows = 0;
    bool small_fused = false;     // forward: all Dense layers in one launch (k_mlp_fwd) with small_lds bytes of LDS and row stride small_maxpad ...
    size_t small_lds = 0;
    int small_maxpad = 0;
    bool build_input = false;     // ... which also builds the concat rows and evaluates the body's gate (net_state: the caller leaves x unfilled, InputBuild)
    bool fwd3 = false, bwd3 = false;          // the three-layer chains on the matrix cores (k_fwd3_split / k_bwd3_split)
    std::vector<uint8_t> wide_fwd, wide_bwd;  // otherwise per layer: the layer's products on the matrix cores (else k_dense_fwd / k_layer_bwd)
};

// what k_mlp_fwd builds the concat rows of a body from where Net::build_input is set (the build fields of its MlpFwd)
struct InputBuild {
    int Ds, c_aggs;
    const float *tmpl, *state, *own, *own_prev;
    const int32_t *indptr, *adj_src;
    const float *adj_w;
    float thr;
    int *flag;
};

// what follows the last layer of net_state's backward pass in the same launch as the sum of the chunk partials (k_state_grad_sum)
struct StateGradJob {
    int64_t N;
    int Ds, in_s, c_aggs;
    const int32_t *sip, *sdst;
    const float *sw;
    float *d_state;               // out: d loss / d state of the body's input
    // adjoint iteration of the fixed-point gradient (g != NULL; gnn_train_adjoint.hip) instead: z_next[r] = g[r] + that sum, also written to
    // `work` (the next net_backward call consumes its incoming gradient in place), with the gate of the iteration against z_prev:
    // gate_prev closed (NULL: open) = the iteration has converged before, z_next = z_prev and no word is raised
    const float *g = nullptr, *z_prev = nullptr;
    float *z_next = nullptr, *work = nullptr;
    float thr = 0.0f;
    const int *gate_prev = nullptr;
    int *gate = nullptr;
    int *form_out = nullptr;      // receives the ADJ_GATHER_* form the gather took
    // power iteration of the contraction estimate (pw_inv != NULL; gnn_train_adjoint.hip) instead: z_next[r] = that sum * *pw_inv, also written to
    // `work`, and ONE partial squared norm of z_next per block of the gather in pw_part; *pw_inv == 0 (the iteration has stopped): z_next stays,
    // `work` and the partials are zero.  g, z_prev and the gates are not read
    const float *pw_inv = nullptr;
    float *pw_part = nullptr;
    // Anderson-accelerated adjoint iteration (anderson != NULL, beside g; gnn_train_anderson.hip) instead: the gather forms G = g + that sum, the residual
    // f = G - z_prev with the gate, the difference rows of the window's slot and the block's partial dots; z_next and `work` are written by the
    // mix that follows (by the gather itself in iteration 0, and behind a closed gate_prev as above)
    const struct AndersonJob *anderson = nullptr;
};

// floats of a net's trainable arrays = of its gradient vector: dW1, db1, ..., dgamma, dbeta
inline size_t net_grad_floats(const gnn_mlp *m)
{
    size_t t = 0;
    for (int l = 0; l < m->n_layers; ++l) t += (size_t)m->dims[l] * m->dims[l + 1] + (size_t)m->dims[l + 1];
    return t + (m->has_bn ? (size_t)2 * m->dims.back() : 0);
}

// floats of zero-initialised memory a Net needs: the gradient vector and the BatchNormalization statistics of every call
inline size_t net_zero_floats(const gnn_mlp *m, int max_calls)
{
    const size_t t = net_grad_floats(m) + (m->has_bn ? (size_t)std::max(1, max_calls) * 2 * m->dims.back() : 0);
    return (t + 63) & ~(size_t)63;
}

// gnn_train_wide.hip: the matrix-core products.  The predicates say what the launchers cover (and hold the GNN_DIAG switches).
bool tg_many_rows(int64_t n);
bool tg_wide(int n_in, int n_out);
bool tg_wgrad_covers(int n_in, int n_out);
bool tg_wgrad_bf(int n_out);      // which of the two weight-gradient kernels launch_wgrad_f32 takes
int64_t tg_sweep_rows();
bool fwd3_covers(const gnn_mlp *m);
bool bwd3_covers(const gnn_mlp *m);
int launch_gemm_f32(hipStream_t st, Buf &buf, int64_t n, int K, int n_cols, const float *X, const float *M, const float *bias, int act, int mode,
                    const uint8_t *keep, float rate, const float *a_prev, float *Y);
// a0 == a1 == NULL: the cache-less instantiation (k_fwd3_split<ACT, false>), which writes the last layer's output alone
int launch_fwd3(hipStream_t st, Buf &buf, const gnn_mlp *m, int64_t n, const float *x, float *a0, float *a1, float *a2);
int launch_bwd3(hipStream_t st, Buf &buf, const gnn_mlp *m, float *const *WT, int64_t n, const float *dz2, const float *a1, const float *a0, float *dz1,
                float *dz0, float *dinp, float *dsg = nullptr, int Ds = 0, int c_aggs = 0);
int launch_wgrad_f32(hipStream_t st, int64_t n, int64_t rpb, int parts, int64_t pstride, int n_in, int n_out, const float *H, const float *DZ, float *part);

// the gather / scatter between the state and the concat with 16 lanes per state row (k_train_input_rows; the dsg rows of k_bwd3_split,
// k_state_grad_rows): state rows of whole 16-byte pieces, at most 16 of them, on many rows
inline bool state_rows16(int Ds, int64_t n) { return (Ds & 3) == 0 && Ds <= 64 && tg_many_rows(n); }

// ---- persistent training forward of small batches (gnn_train_small.hip: k_train_small) ------------------------------------------------
// Every body of net_state in ONE launch: one workgroup per BatchNormalization chunk of rows_per_block(n) rows (32, 48 or 64 below
// GNN_TRAIN_MFMA_MIN_ROWS rows: at most 64 workgroups), which runs k_mlp_fwd's tile code on its rows and k_bn_stats / k_bn_apply's on its
// chunk, with the grid barrier of gnn_small_common.h between the bodies.  The caches of ALL max_iter bodies are one arena block laid out
// body after body (the kernel finds body b's arrays at b * body_floats): it must fit GNN_TRAIN_PERSISTENT_MAX_BYTES (include/gnn_hip.h).
constexpr size_t GNN_TRAIN_PERSISTENT_MAX_LDS = (size_t)156 * 1024;      // of the 160 KiB a workgroup can have: the kernel's static words beside it
constexpr size_t GNN_TRAIN_PERSISTENT_MIN_LDS = (size_t)84 * 1024;       // asked for at least: more than half a CU's LDS, so ONE workgroup per CU

struct SmallTrainForm {
    bool ok = false;
    int rows = 0, grid = 0, barriers = 0;         // rows per workgroup, workgroups, grid barriers per body
    size_t lds = 0;                               // dynamic LDS of the launch
    // floats of one body's cache block and where its arrays start: concat rows at 0, the Dense outputs, xhat / new state / chunk statistics
    size_t body_floats = 0, off_a[GNN_FUSED_MAXL + 1] = {}, off_xhat = 0, off_y = 0, off_part = 0;
    size_t cap_body_bytes = 0, cap_bytes = 0;     // what the byte cap is compared with: one block WITH the BatchNormalization arrays, max_iter of them
};

// The part of the decision that the net, the rows and max_iter make (gnn_train_persistent_form, include/gnn_hip.h); net: decided by
// net_decide_form for net_state (producer_dropout).  The loop's part (one GPU, not disabled, not profiling, co-resident): gnn_train.hip.
inline SmallTrainForm small_train_form(const Net &net, int max_iter)
{
    SmallTrainForm f;
    const gnn_mlp *m = net.m;
    const int L = m->n_layers;
    const int64_t n = net.rows;
    if (n < 1) return f;
    auto pad64 = [](size_t floats) { return (floats + 63) & ~(size_t)63; };
    const int F = m->dims[L];
    f.rows = (int)rows_per_block(n);
    f.grid = (int)cdiv(n, f.rows);
    f.barriers = m->has_bn ? 2 : 1;
    size_t off = pad64((size_t)n * m->dims[0]);
    for (int l = 0; l < L && l <= GNN_FUSED_MAXL; ++l) { f.off_a[l] = off; off += pad64((size_t)n * m->dims[l + 1]); }
    const size_t bn_floats = 2 * pad64((size_t)n * F) + pad64((size_t)f.grid * 2 * F);
    if (m->has_bn) {
        f.off_xhat = off; f.off_y = f.off_xhat + pad64((size_t)n * F); f.off_part = f.off_y + pad64((size_t)n * F);
        f.body_floats = off + bn_floats;
    } else
        f.body_floats = off;
    f.cap_body_bytes = sizeof(float) * (off + bn_floats);
    f.cap_bytes = f.cap_body_bytes * (size_t)std::max(max_iter, 0);
    // LDS: two row tiles of the widest layer, the partial sums of dense_rows (BatchNormalization's scratch takes their place afterwards)
    const size_t need = sizeof(float) * ((size_t)2 * f.rows * net.small_maxpad + (size_t)256 * f.rows);
    f.lds = std::max(need, GNN_TRAIN_PERSISTENT_MIN_LDS);
    f.ok = net.build_input && net.rate[L] == 0.0f && max_iter >= 1 && f.rows <= 64 && f.grid <= 64 && need <= GNN_TRAIN_PERSISTENT_MAX_LDS &&
           (size_t)4 * F + 1100 <= (size_t)256 * f.rows && f.cap_bytes <= GNN_TRAIN_PERSISTENT_MAX_BYTES;
    return f;
}

// can the launch's grid be resident at once on the device (occupancy query x compute units)?
int small_train_resident(int device, const SmallTrainForm &f, bool *ok);
// the launch: body 0 reads build.state (== build.own), body b's cache block is cache + b * f.body_floats, words [1 + 2 max_iter] zeroed,
// host_result: pinned [k, status] (status cleared by the caller)
int small_train_launch(hipStream_t st, const Net &net, const SmallTrainForm &f, const InputBuild &build, int max_iter, float *cache, int *words, int *host_result);

// gnn_train_net.hip: one Sequential in training mode
void net_decide_form(Net &net, int64_t n, bool producer_dropout);
int net_setup(hipStream_t st, Buf &buf, Net &net, const gnn_mlp *m, const float *rates, const float *bn_gamma_beta_host, int max_calls, float *zero_mem,
              int64_t rows, bool producer_dropout);
// behind net_setup: this step runs the net's BatchNormalization on its moving statistics (Net::frozen)
int net_freeze_bn(hipStream_t st, Buf &buf, Net &net);
// How a body of the recomputing step (gnn_loop_set_train_recompute) calls net_forward; the default is the ordinary call.
//   y_dst: where the call's output goes (the one array of a state-only body that outlives it; NULL: allocated like the others)
//   cacheless: the first pass may take the forms that do not store what only the backward pass reads (a0 / a1 of the three-layer chain, xhat);
//              *cacheless_chain is set when the cache-less chain was launched
//   replay_call >= 0: the call REPEATS BatchNormalization call `replay_call` of this step - it is not counted, c.stats is that call's slot of
//              stats_all (left as the first pass wrote it), and the statistics it recomputes (same bits) go to scratch
struct FwdMode {
    float *y_dst = nullptr;
    bool cacheless = false;
    int replay_call = -1;
    int *cacheless_chain = nullptr;
};
int net_forward(hipStream_t st, Buf &buf, Net &net, float *x, uint8_t *keep0, const uint8_t *masks, const MaskStream &rng, NetCache &c, float **y_out,
                gnn_comm *comm = nullptr, const InputBuild *build = nullptr, const FwdMode &mode = FwdMode());
// wgrad = false: d x alone (no weight-gradient tiles or kernels, no sum of the chunk partials; net.grads and net.part are not touched)
int net_backward(hipStream_t st, Buf &buf, Net &net, const NetCache &c, float *d, float **dx_out, const StateGradJob *job = nullptr,
                 gnn_comm *comm = nullptr, int64_t n_global = 0, bool wgrad = true);
// the form net_setup decided, as the ints of gnn_train_forms (include/gnn_hip.h): out[3 + 3 n_layers]
void net_forms(const Net &net, int *out);
// out[t] += part[0][t] + ... + part[parts - 1][t], t < count (k_sum_parts)
int net_sum_parts(hipStream_t st, int parts, int64_t count, const float *part, float *out);

// gnn_train_adjoint.hip: the gradient at the fixed point (include/gnn_hip.h, gnn_loop_set_gradient_mode)
enum { ADJ_GATHER_GENERIC = 0, ADJ_GATHER_ROWS = 1, ADJ_GATHER_ROWS_ALIGNED = 2, ADJ_GATHER_NARROW = 3 };
// state rows of whole 16-byte pieces, at most 16 of them: 16 lanes per row take four columns each (else: every 16th column)
inline bool adjoint_rows16(int Ds) { return (Ds & 3) == 0 && Ds <= 64; }
// why a net_state cannot take gradient mode 1 (0: it can): 1 BatchNormalization, 2 a Dropout rate != 0
// (flags: gnn_loop_set_gradient_mode_ex - with GNN_ADJOINT_FROZEN_BN the BatchNormalization runs on its moving statistics and is accepted)
inline int adjoint_refusal(const gnn_mlp *m, const float *rates, int flags = 0)
{
    if (m->has_bn && !(flags & GNN_ADJOINT_FROZEN_BN)) return 1;
    for (int l = 0; l <= m->n_layers; ++l) if (rates[l] != 0.0f) return 2;
    return 0;
}
// the gather of one adjoint iteration (job.g != NULL) from u = d inp [n, in_s], or (aligned) from the dsg rows [n, 2 Ds] k_bwd3_split left;
// returns the ADJ_GATHER_* form it took through *form (may be NULL)
int launch_adjoint_gather(hipStream_t st, const StateGradJob &job, const float *u, bool aligned, int *form);
// The power iteration w_t = (J^T w_{t-1}) / |w_{t-1}| of the contraction estimate (include/gnn_hip.h: gnn_loop_contraction_estimate).  Its gather
// (job.pw_inv != NULL) has the three shapes of the adjoint's, without g, z_prev and the gate: per element the same fmaf chain, then (own + acc) * *pw_inv,
// and one partial sum of squares per block of 16 rows.  power_blocks: the partials a vector of n rows leaves.
inline unsigned power_blocks(int64_t n) { return cdiv(n * 16, 256); }
int launch_power_gather(hipStream_t st, const StateGradJob &job, const float *u, bool aligned, int *form);
// w_0: v [n, Ds] filled with normal draws of the counter RNG keyed on seed (fill != 0), copied to `work`, with its partials
int launch_power_start(hipStream_t st, int64_t n, int Ds, int fill, uint64_t seed, float *v, float *work, float *part);
// one block: norm = sqrt(part[0] + part[1] + ... in double), *norm_out = norm, *inv = 1 / norm - or 0 when norm is 0 or not finite
int launch_power_finalize(hipStream_t st, unsigned blocks, const float *part, float *norm_out, float *inv);

// gnn_train_anderson.hip: the Anderson-accelerated adjoint solve (include/gnn_hip.h: gnn_loop_set_adjoint_solver).  An iteration t >= 1 is
// net_backward (wgrad = false) with the Anderson gather, then launch_anderson_solve_mix with the same job.
constexpr int ANDERSON_MAX_WINDOW = 8, ANDERSON_PARTS = 2 * ANDERSON_MAX_WINDOW;
// device-resident state of one backward pass (zeroed in front of it): H over the slots, gamma of the last solve with the slots it covers (live; 0
// behind a restart), hist = difference pairs stored since the last restart, restarts
struct AndersonState {
    double H[ANDERSON_MAX_WINDOW][ANDERSON_MAX_WINDOW];
    float gamma[ANDERSON_MAX_WINDOW];
    int hist, live, restarts, pad;
};
struct AndersonJob {
    int first, window;            // first: iteration 0 (no history: the gather writes z_next and `work` itself; no solve, no mix)
    float *G, *f;                 // [N, Ds]: G_{t-1} / f_{t-1} in, G_t / f_t out
    float *dF, *dG;               // the rings, [window][stride]
    size_t stride;
    AndersonState *state;
    double *part;                 // [ANDERSON_PARTS][anderson_blocks(N)]
};
inline unsigned anderson_blocks(int64_t n) { return cdiv(n * 16, 256); }
int launch_anderson_gather(hipStream_t st, const StateGradJob &job, const float *u, bool aligned, int *form);
int launch_anderson_solve_mix(hipStream_t st, const StateGradJob &job);

// One launch per adjoint iteration for narrow nets (k_adjoint_narrow): a block owns ADJ_NARROW_ROWS rows, forms z_L of them by the gather from the
// PREVIOUS launch's u (with the gate of iteration L - 1), then runs the whole chain d z -> . W^T (.) act'(a) -> ... down to the own-state and
// aggregated-state columns of d concat, u_L [n, 2 Ds].  Why a net does not take it (0: it does): 3 more than three Dense layers, 4 a layer wider
// than 64, 5 a concat wider than 96, 6 4,096 rows or more (or none), 7 a softmax in net_state.
constexpr int ADJ_NARROW_ROWS = 16, ADJ_NARROW_MAXW = 64, ADJ_NARROW_MAXIN = 96;
inline int adjoint_narrow_why(const gnn_mlp *m, int64_t n)
{
    if (m->n_layers > 3) return 3;
    for (int l = 1; l <= m->n_layers; ++l) if (m->dims[l] > ADJ_NARROW_MAXW) return 4;
    if (m->dims[0] > ADJ_NARROW_MAXIN) return 5;
    if (n < 1 || !(n < 4096)) return 6;
    for (int l = 0; l < m->n_layers; ++l) if (m->acts[l] == GNN_ACT_SOFTMAX) return 7;
    return 0;
}
struct AdjNarrow {
    int64_t n;
    int Ds, c_aggs, L, gather;    // gather: form z_L from u_prev / z_prev / g and evaluate the gate (else z_L is read from z_cur)
    int dims[4], acts[3];
    const float *WT[3], *a[3];
    const float *colscale;        // frozen BatchNormalization behind the last layer: s_j = gamma_j inv_j [Ds] (NULL: none)
    const int32_t *sip, *sdst;
    const float *sw, *g, *z_prev, *u_prev;
    float *z_cur, *u_out;
    float thr;
    const int *gate_prev;
    int *gate;
};
int launch_adjoint_narrow(hipStream_t st, const AdjNarrow &p);

}   // namespace gnn_train

// What gnn_loop_train_forward leaves for gnn_loop_train_backward (owned by the loop; replaced by the next forward)
struct GNN_INTERNAL gnn_train_ctx {
    gnn_train::Buf buf;
    gnn_train::Net ns, no_;
    std::vector<gnn_train::NetCache> caches;
    gnn_train::NetCache co;
    int32_t *d_sip = nullptr, *d_sdst = nullptr;
    float *d_sw = nullptr;
    float *state = nullptr, *out_nodes = nullptr;
    int k = 0;
    // what a body is rebuilt from (the recomputing step replays body `it` in front of its backward pass; Forward fills them in every mode):
    // states[i] = the state body i reads (row 0 of a replica; states[0] is read in place), the template of the concat, the injected masks of
    // net_state (NULL: own generator) with the bytes of one body, the step's seed.  The rates are Net::rate.
    std::vector<float *> states;
    float *tmpl = nullptr;
    uint8_t *d_masks_s = nullptr;
    size_t mask_iter_bytes = 0;
    uint64_t seed = 0;
    bool recompute = false;       // the forward ran state-only: `caches` holds k empty entries until train_backward rebuilds them one at a time
    int replayed = 0;             // ... bodies rebuilt by the backward pass
    int cacheless_chain = 0;      // ... the first pass launched the cache-less three-layer chain (else the ordinary kernels on rewound scratch)
    float *adjoint_z = nullptr;   // gradient modes 1 and 2, behind the backward pass: z_final [N, Ds] (gnn_loop_adjoint_z)
    // label gradients the last backward pass kept on the device (gnn_loop_train_backward_chained with keep_label_gradients): d loss / d node
    // labels [N, NL] and / or, edge-based, d loss / d arc labels [E, AL] in original arc order (NULL: not asked for); scratch of this step,
    // alive until the next forward
    float *kept_d_nodes = nullptr, *kept_d_arcs = nullptr;
    bool fixed_point = false;     // gradient mode 1: `caches` holds ONE recorded body at the converged state `state` (k bodies of the inference Loop led there)
    bool persistent = false;      // the bodies ran in the persistent launch (k_train_small) ...
    int workgroups = 0, barriers = 0;     // ... of that many workgroups, with that many grid barriers per body
    int64_t N = 0, M = 0;
    int64_t N_global = 0, M_global = 0;   // sharded forward: the rows / masked rows of all ranks
    int64_t M_before = 0;                 // ... and the masked rows of the lower ranks
    bool backward_done = false;   // the gradients are complete (and the activations spent)
    bool applied = false;         // gnn_loop_optimizer_step has consumed them
    // regularizer penalty, per-block partials of k_grad_prepare: net_state's blocks, then net_output's (0 blocks: no regularizer there)
    double *pen_part = nullptr;
    unsigned pen_blocks[2] = {0, 0};
    // gradient clipping (clip_prepare): per-block partial sums of squares of both nets, their sums per array [2][CLIP_SLOTS] and
    // over all arrays [1], and the factor of every array [2][CLIP_SLOTS]
    double *sq_part[2] = {nullptr, nullptr}, *sq = nullptr;
    float *factor = nullptr;
};

namespace gnn_train GNN_INTERNAL {

// both nets of the loop with what differs between them: BatchNormalization calls of this step's forward (their statistics rows in
// Net::stats_all), index 0 net_state, 1 net_output
struct LoopNet { gnn_mlp *m; Net *net; int calls; };
// (gradient modes 1 and 2: the k bodies were the inference Loop's - net_state made no BatchNormalization call, its moving statistics stay)
inline std::array<LoopNet, 2> loop_nets(gnn_loop *l, gnn_train_ctx *cx) { return {{{l->st, &cx->ns, cx->fixed_point ? 0 : cx->k}, {l->ou, &cx->no_, cx->M > 0 ? 1 : 0}}}; }

// gnn_train_update.hip: between the backward pass and the update
int grad_prepare(gnn_loop *l, gnn_train_ctx *cx, hipStream_t st);
int update_both(gnn_loop *l, gnn_train_ctx *cx, hipStream_t st, int kind, const float *h, float gscale_state, float mom_s, float mom_o, bool own_global, double extra);

}   // namespace gnn_train
