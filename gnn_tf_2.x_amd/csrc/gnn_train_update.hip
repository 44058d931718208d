// What happens to the gradients of a training step: regularizers, clipping, the optimizer rules, the moving statistics (see gnn_train.hip).
#include <cmath>

#include "gnn_train.h"

using namespace gnn_train;

// ---------------------------------------------------------------------------------------------------------------------
// Between the backward pass and the update, on the device: the regularizer terms of the taped loss (reference
// GNN_BaseClass.py:223-235) and the gradient clipping of tf.keras optimizers (clipvalue, clipnorm, global_clipnorm).
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int CLIP_SLOTS = 35;    // arrays of one net: 16 layers x (W, b) + gamma + beta at most

struct ParamMap {                 // gradient vector index -> parameter array
    int n = 0;
    int goff[CLIP_SLOTS + 1];     // [n + 1]
    float *p[CLIP_SLOTS];
};

ParamMap param_map(const gnn_mlp *m, const Net &net)
{
    ParamMap mp;
    const int L = m->n_layers;
    for (int l = 0; l < L; ++l) {
        mp.goff[2 * l] = (int)net.g_off[2 * l]; mp.p[2 * l] = m->W[l];
        mp.goff[2 * l + 1] = (int)net.g_off[2 * l + 1]; mp.p[2 * l + 1] = m->b[l];
    }
    mp.n = 2 * L;
    if (m->has_bn) {
        const int F = m->dims.back();
        mp.goff[mp.n] = (int)net.g_off[2 * L]; mp.p[mp.n] = m->bn_raw; ++mp.n;
        mp.goff[mp.n] = (int)net.g_off[2 * L + 1]; mp.p[mp.n] = m->bn_raw + F; ++mp.n;
    }
    mp.goff[mp.n] = (int)net.g_total;
    return mp;
}

struct RegCoef { double l1[CLIP_SLOTS], l2[CLIP_SLOTS]; };

// sum of the 256 values of a block, the same tree in every run; the result is valid in thread 0
__device__ inline double block_sum256(double *red, double v)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// g <- g + l1 sign(w) + 2 l2 w (sign(0) = 0; the term is rounded to float first, like the host mirror GNN/regularizers.py), and the
// block's share of the penalty l1 sum |w| + l2 sum w^2 (GNN_BaseClass.py:223-228) -> pen_part[block]
__global__ void __launch_bounds__(256) k_grad_prepare(ParamMap mp, RegCoef rc, float *g, double *pen_part)
{
    __shared__ double red[256];
    const int j = blockIdx.x * 256 + threadIdx.x;
    double pen = 0.0;
    if (j < mp.goff[mp.n]) {
        int a = 0;
        while (j >= mp.goff[a + 1]) ++a;
        const double l1 = rc.l1[a], l2 = rc.l2[a];
        if (l1 != 0.0 || l2 != 0.0) {
            const double w = (double)mp.p[a][j - mp.goff[a]];
            const double sgn = w > 0.0 ? 1.0 : (w < 0.0 ? -1.0 : 0.0);
            g[j] += (float)(l1 * sgn + 2.0 * l2 * w);
            pen = l1 * fabs(w) + l2 * w * w;
        }
    }
    pen = block_sum256(red, pen);
    if (threadIdx.x == 0) pen_part[blockIdx.x] = pen;
}

__device__ inline float clip_value(float v, float c) { return c > 0.0f ? (v > c ? c : (v < -c ? -c : v)) : v; }

// Segmented sum of squares of the scaled and value-clipped gradients: block b leaves, for every array a with entries in
// [256 b, 256 b + 256), their sum of squares in part[a * gridDim.x + b] (the other entries of part are never read).
__global__ void __launch_bounds__(256) k_grad_sqnorm(ParamMap mp, const float *g, float gscale, float clipvalue, double *part)
{
    __shared__ double red[256];
    const int b0 = blockIdx.x * 256, j = b0 + threadIdx.x, total = mp.goff[mp.n];
    int a = -1;
    double sq = 0.0;
    if (j < total) {
        a = 0;
        while (j >= mp.goff[a + 1]) ++a;
        const float v = clip_value(g[j] * gscale, clipvalue);
        sq = (double)v * (double)v;
    }
    const int last = min(b0 + 256, total) - 1;       // the arrays of this block: first .. until (the same in every thread)
    int first = 0;
    while (b0 >= mp.goff[first + 1]) ++first;
    int until = first;
    while (last >= mp.goff[until + 1]) ++until;
    for (int s = first; s <= until; ++s) {
        const double r = block_sum256(red, a == s ? sq : 0.0);
        if (threadIdx.x == 0) part[(size_t)s * gridDim.x + blockIdx.x] = r;
    }
}

struct ClipJob {
    int n[2], blocks[2];
    int goff[2][CLIP_SLOTS + 1];
    const double *part[2];
};

// One block: the partials of every array added in block order -> sq[net * CLIP_SLOTS + a], all of them in index order ->
// sq[2 CLIP_SLOTS]; factor of array a = clipnorm / max(|g_a|, clipnorm) * global / max(|g|, global) * extra (a threshold of 0: 1)
__global__ void __launch_bounds__(128) k_clip_factors(ClipJob cj, double clipnorm, double global_clipnorm, double extra, double *sq, float *factor)
{
    __shared__ double s_sq[2 * CLIP_SLOTS];
    for (int idx = threadIdx.x; idx < 2 * CLIP_SLOTS; idx += blockDim.x) {
        const int net = idx / CLIP_SLOTS, a = idx - net * CLIP_SLOTS;
        double s = 0.0;
        if (a < cj.n[net] && cj.goff[net][a + 1] > cj.goff[net][a]) {
            const int bf = cj.goff[net][a] / 256, bl = (cj.goff[net][a + 1] - 1) / 256;
            for (int b = bf; b <= bl; ++b) s += cj.part[net][(size_t)a * cj.blocks[net] + b];
        }
        s_sq[idx] = s;
        sq[idx] = s;
    }
    __syncthreads();
    double tot = 0.0;
    for (int idx = 0; idx < 2 * CLIP_SLOTS; ++idx) tot += s_sq[idx];
    if (threadIdx.x == 0) sq[2 * CLIP_SLOTS] = tot;
    for (int idx = threadIdx.x; idx < 2 * CLIP_SLOTS; idx += blockDim.x) {
        double f = extra;
        if (clipnorm > 0.0) f *= clipnorm / fmax(sqrt(s_sq[idx]), clipnorm);
        if (global_clipnorm > 0.0) f *= global_clipnorm / fmax(sqrt(tot), global_clipnorm);
        factor[idx] = (float)f;
    }
}

}   // namespace

// the regularizer terms of both nets, behind the backward pass and in front of every reader of the gradients
int gnn_train::grad_prepare(gnn_loop *l, gnn_train_ctx *cx, hipStream_t st)
{
    auto nets = loop_nets(l, cx);
    unsigned blocks[2] = {0, 0};
    for (int i = 0; i < 2; ++i)
        if (!nets[i].m->reg_l1.empty()) blocks[i] = cdiv((int64_t)nets[i].net->g_total, 256);
    if (!blocks[0] && !blocks[1]) return GNN_OK;
    ARGCHK(l->st->n_layers <= 16 && l->ou->n_layers <= 16, "too many layers");
    int rc;
    if ((rc = cx->buf.get(&cx->pen_part, (size_t)blocks[0] + blocks[1]))) return rc;
    for (int i = 0; i < 2; ++i) {
        cx->pen_blocks[i] = blocks[i];
        if (!blocks[i]) continue;
        const gnn_mlp *m = nets[i].m;
        RegCoef co;
        for (int a = 0; a < CLIP_SLOTS; ++a) {
            const bool dense = a < 2 * m->n_layers;        // BatchNormalization's gamma / beta carry no regularizer
            co.l1[a] = dense ? m->reg_l1[a] : 0.0; co.l2[a] = dense ? m->reg_l2[a] : 0.0;
        }
        hipLaunchKernelGGL(k_grad_prepare, blocks[i], 256, 0, st, param_map(m, *nets[i].net), co, nets[i].net->grads, cx->pen_part + (i ? blocks[0] : 0));
        HIPCHK(hipGetLastError());
    }
    return GNN_OK;
}

namespace {
// cx->sq and cx->factor from the gradients as they are now (net_state's scaled by gscale_state), on the stream
int clip_prepare(gnn_loop *l, gnn_train_ctx *cx, hipStream_t st, float gscale_state, float clipvalue, double clipnorm, double global_clipnorm, double extra)
{
    auto nets = loop_nets(l, cx);
    const float gscale[2] = {gscale_state, 1.0f};
    ClipJob cj;
    int rc;
    if (!cx->sq && ((rc = cx->buf.get(&cx->sq, (size_t)2 * CLIP_SLOTS + 1)) || (rc = cx->buf.get(&cx->factor, (size_t)2 * CLIP_SLOTS)))) return rc;
    for (int i = 0; i < 2; ++i) {
        const ParamMap mp = param_map(nets[i].m, *nets[i].net);
        const unsigned blocks = cdiv((int64_t)nets[i].net->g_total, 256);
        if (!cx->sq_part[i] && (rc = cx->buf.get(&cx->sq_part[i], (size_t)mp.n * blocks))) return rc;
        hipLaunchKernelGGL(k_grad_sqnorm, blocks, 256, 0, st, mp, nets[i].net->grads, gscale[i], clipvalue, cx->sq_part[i]);
        HIPCHK(hipGetLastError());
        cj.n[i] = mp.n; cj.blocks[i] = (int)blocks; cj.part[i] = cx->sq_part[i];
        for (int a = 0; a <= mp.n; ++a) cj.goff[i][a] = mp.goff[a];
    }
    hipLaunchKernelGGL(k_clip_factors, 1, 128, 0, st, cj, clipnorm, global_clipnorm, extra, cx->sq, cx->factor);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}
}   // namespace

// ---------------------------------------------------------------------------------------------------------------------
// Optimizer step on the device (reference GNN_BaseClass.py:243-247: optimizer.apply_gradients on the trainable variables of
// both nets; Keras BatchNormalization moving statistics): the weights, the optimizer slots and the gradients never leave HBM.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// kind 0, SGD: h = {learning rate, momentum}: v <- momentum v - lr g, p <- p + v
// kind 1, Adam (Keras): h = {lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), b1, b2, epsilon}: m, v updated, p <- p - lr_t m / (sqrt(v) + epsilon)
//   (h[2] != 0: Nesterov momentum, p <- p + momentum v - lr g with the new v)
// kind 2, Adam with amsgrad: h as kind 1; m, v as Adam, vhat <- max(vhat, v) (slot c), p <- p - lr_t m / (sqrt(vhat) + epsilon)
// kind 3, RMSprop: h = {lr, rho, momentum, epsilon}: r <- rho r + (1 - rho) g^2 (slot a); momentum == 0: p <- p - lr g / (sqrt(r) + epsilon);
//         momentum > 0: q <- momentum q + lr g / sqrt(r + epsilon) (slot b), p <- p - q
// kind 4, centered RMSprop: also a <- rho a + (1 - rho) g (slot c), and max(r - a^2, 0) in place of r in both branches (r - a^2 cancels
//         in float32 and may come out below zero: the clamp is part of the rule)
// kind 5, Adagrad: h = {lr, initial_accumulator_value, epsilon}: s <- s + g^2 (slot a, from zero), p <- p - lr g / (sqrt(initial + s) + epsilon)
// kind 6, Adamax: h = {lr / (1 - b1^t), b1, b2, epsilon}: m <- b1 m + (1 - b1) g (slot a), u <- max(b2 u, |g|) (slot b), p <- p - h0 m / (u + epsilon)
// CLIP: the scaled gradient is clipped by value and multiplied by its array's factor (k_clip_factors) first
enum { OPT_SGD = 0, OPT_ADAM = 1, OPT_AMSGRAD = 2, OPT_RMSPROP = 3, OPT_RMSPROP_CENTERED = 4, OPT_ADAGRAD = 5, OPT_ADAMAX = 6, OPT_KINDS = 7 };

template <bool CLIP>
__global__ void k_optimizer(ParamMap mp, const float *g, float gscale, float clipvalue, const float *factor, float *sa, float *sb, float *sc, int kind,
                            float h0, float h1, float h2, float h3)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= mp.goff[mp.n]) return;
    int a = 0;
    while (j >= mp.goff[a + 1]) ++a;
    float *p = mp.p[a] + (j - mp.goff[a]);
    float gr = g[j] * gscale;
    if (CLIP) gr = clip_value(gr, clipvalue) * factor[a];
    if (kind == OPT_ADAM || kind == OPT_AMSGRAD) {
        const float m = h1 * sa[j] + (1.0f - h1) * gr;
        const float v = h2 * sb[j] + (1.0f - h2) * gr * gr;
        sa[j] = m; sb[j] = v;
        float den = v;
        if (kind == OPT_AMSGRAD) { den = fmaxf(sc[j], v); sc[j] = den; }
        *p = *p - h0 * m / (sqrtf(den) + h3);
    } else if (kind == OPT_RMSPROP || kind == OPT_RMSPROP_CENTERED) {
        const float r = h1 * sa[j] + (1.0f - h1) * gr * gr;
        sa[j] = r;
        float den = r;
        if (kind == OPT_RMSPROP_CENTERED) {
            const float mean = h1 * sc[j] + (1.0f - h1) * gr;
            sc[j] = mean;
            den = fmaxf(r - mean * mean, 0.0f);
        }
        if (h2 > 0.0f) {
            const float q = h2 * sb[j] + h0 * gr / sqrtf(den + h3);
            sb[j] = q;
            *p = *p - q;
        } else
            *p = *p - h0 * gr / (sqrtf(den) + h3);
    } else if (kind == OPT_ADAGRAD) {
        const float s = sa[j] + gr * gr;
        sa[j] = s;
        *p = *p - h0 * gr / (sqrtf(h1 + s) + h2);
    } else if (kind == OPT_ADAMAX) {
        const float m = h1 * sa[j] + (1.0f - h1) * gr;
        const float u = fmaxf(h2 * sb[j], fabsf(gr));
        sa[j] = m; sb[j] = u;
        *p = *p - h0 * m / (u + h3);
    } else {
        const float v = h1 * sa[j] - h0 * gr;
        sa[j] = v;
        *p = h2 != 0.0f ? *p + (h1 * v - h0 * gr) : *p + v;
    }
}

// what optimizer_step / gnn_loop_arm_optimizer accept: a known kind, and a finite value >= 0 wherever a new rule divides by it
// (kinds 0 and 1 take their hyper-parameters as they always did)
const char *optimizer_args_error(int kind, const float *h)
{
    if (kind < 0 || kind >= OPT_KINDS)
        return "kind: 0 SGD, 1 Adam, 2 Adam(amsgrad), 3 RMSprop, 4 RMSprop(centered), 5 Adagrad, 6 Adamax";
    auto ok = [](float v) { return std::isfinite(v) && v >= 0.0f; };
    if ((kind == OPT_AMSGRAD || kind == OPT_ADAMAX) && !ok(h[3])) return "epsilon must be finite and >= 0";
    if ((kind == OPT_RMSPROP || kind == OPT_RMSPROP_CENTERED) && !(ok(h[3]) && ok(h[2]))) return "RMSprop: momentum and epsilon must be finite and >= 0";
    if (kind == OPT_ADAGRAD && !(ok(h[1]) && ok(h[2]))) return "Adagrad: initial_accumulator_value and epsilon must be finite and >= 0";
    return nullptr;
}

// moving <- moving * momentum + batch * (1 - momentum), once per BatchNormalization call, in call order
__global__ void k_bn_moving(int F, int calls, const float *stats_all, float momentum, float *raw)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= F) return;
    float mean = raw[2 * F + j], var = raw[3 * F + j];
    for (int c = 0; c < calls; ++c) {
        mean = mean * momentum + stats_all[(size_t)c * 2 * F + j] * (1.0f - momentum);
        var = var * momentum + stats_all[(size_t)c * 2 * F + F + j] * (1.0f - momentum);
    }
    raw[2 * F + j] = mean; raw[3 * F + j] = var;
}

// factor: the per-array clip factors of this net on the device (clip_prepare), NULL = no clipping
int optimizer_apply(hipStream_t st, gnn_mlp *m, const Net &net, int calls, int kind, const float *h, float gscale, float bn_momentum, float clipvalue = 0.0f,
                    const float *factor = nullptr)
{
    const size_t total = net.g_total;
    if (!m->opt_a) {
        if (gnn_dev_malloc((void **)&m->opt_a, sizeof(float) * total) != hipSuccess || gnn_dev_malloc((void **)&m->opt_b, sizeof(float) * total) != hipSuccess)
            return gnn_fail(GNN_ERR_HIP, "hipMalloc of the optimizer slots failed");
        HIPCHK(hipMemsetAsync(m->opt_a, 0, sizeof(float) * total, st));
        HIPCHK(hipMemsetAsync(m->opt_b, 0, sizeof(float) * total, st));
        m->opt_kind = kind;
    }
    const bool third = kind == OPT_AMSGRAD || kind == OPT_RMSPROP_CENTERED;
    if (m->opt_kind != kind) {                     // another rule wrote these slots: it starts from zero, like a new optimizer
        HIPCHK(hipMemsetAsync(m->opt_a, 0, sizeof(float) * total, st));
        HIPCHK(hipMemsetAsync(m->opt_b, 0, sizeof(float) * total, st));
        if (m->opt_c && third) HIPCHK(hipMemsetAsync(m->opt_c, 0, sizeof(float) * total, st));
        m->opt_kind = kind;
    }
    if (third && !m->opt_c) {
        if (gnn_dev_malloc((void **)&m->opt_c, sizeof(float) * total) != hipSuccess) return gnn_fail(GNN_ERR_HIP, "hipMalloc of the optimizer slots failed");
        HIPCHK(hipMemsetAsync(m->opt_c, 0, sizeof(float) * total, st));
    }
    const ParamMap mp = param_map(m, net);
    if (factor)
        hipLaunchKernelGGL(k_optimizer<true>, cdiv((int64_t)total, 256), 256, 0, st, mp, net.grads, gscale, clipvalue, factor, m->opt_a, m->opt_b, m->opt_c, kind,
                           h[0], h[1], h[2], h[3]);
    else
        hipLaunchKernelGGL(k_optimizer<false>, cdiv((int64_t)total, 256), 256, 0, st, mp, net.grads, gscale, 0.0f, nullptr, m->opt_a, m->opt_b, m->opt_c, kind,
                           h[0], h[1], h[2], h[3]);
    HIPCHK(hipGetLastError());
    if (m->has_bn) {
        const int F = m->dims.back();
        if (calls > 0) hipLaunchKernelGGL(k_bn_moving, cdiv(F, 64), 64, 0, st, F, calls, net.stats_all, bn_momentum, m->bn_raw);
        HIPCHK(hipGetLastError());
        int rc = gnn_mlp_refresh_bn(m, st);
        if (rc) return rc;
    }
    m->version++;
    m->pack_dirty = true;
    return GNN_OK;
}

// The update of both nets with the loop's clipping (gnn_loop_set_clipping): the norms of both nets are on the device before either
// net changes.  own_global: the loop's global_clipnorm applies (else the caller's norm spans more than this loop: `extra` carries it).
}   // namespace

int gnn_train::update_both(gnn_loop *l, gnn_train_ctx *cx, hipStream_t st, int kind, const float *h, float gscale_state, float mom_s, float mom_o, bool own_global, double extra)
{
    const float cv = l->train.clip.value;
    const double cn = l->train.clip.norm, cg = own_global ? l->train.clip.global : 0.0;
    const bool clip = cv > 0.0f || cn > 0.0 || cg > 0.0 || extra != 1.0;
    int rc;
    if (clip && (rc = clip_prepare(l, cx, st, gscale_state, cv, cn, cg, extra))) return rc;
    auto nets = loop_nets(l, cx);
    const float gscale[2] = {gscale_state, 1.0f}, mom[2] = {mom_s, mom_o};
    for (int i = 0; i < 2; ++i)
        if ((rc = optimizer_apply(st, nets[i].m, *nets[i].net, nets[i].calls, kind, h, gscale[i], mom[i], cv, clip ? cx->factor + i * CLIP_SLOTS : nullptr))) return rc;
    return GNN_OK;
}

namespace {
int optimizer_step(gnn_loop *l, int kind, const float *hyper, float state_grad_scale, float bn_momentum_state, float bn_momentum_output, bool own_global, double extra)
{
    ARGCHK(l && hyper, "bad arguments");
    if (const char *why = optimizer_args_error(kind, hyper)) return gnn_fail(GNN_ERR_ARG, "%s", why);
    gnn_train_ctx *cx = l->train_ctx;
    if (!cx || !cx->backward_done || cx->applied) return gnn_fail(GNN_ERR_STATE, "no fresh gradients: run gnn_loop_train_step (or forward + backward) first");
    ARGCHK(l->st->n_layers <= 16 && l->ou->n_layers <= 16, "too many layers");
    HIPCHK(hipSetDevice(l->device));
    hipStream_t st = l->stream;
    int rc = update_both(l, cx, st, kind, hyper, state_grad_scale, bn_momentum_state, bn_momentum_output, own_global, extra);
    cx->applied = true;
    if (!rc) HIPCHK(hipStreamSynchronize(st));   // other loops (other streams) may use these weights next
    return rc;
}
}   // namespace

extern "C" int gnn_loop_optimizer_step(gnn_loop *l, int kind, const float *hyper, float state_grad_scale, float bn_momentum_state,
                                       float bn_momentum_output)
{
    return optimizer_step(l, kind, hyper, state_grad_scale, bn_momentum_state, bn_momentum_output, true, 1.0);
}

extern "C" int gnn_loop_optimizer_step_scaled(gnn_loop *l, int kind, const float *hyper, float state_grad_scale, double grad_scale,
                                              float bn_momentum_state, float bn_momentum_output)
{
    ARGCHK(std::isfinite(grad_scale) && grad_scale > 0.0, "grad_scale must be finite and > 0");
    return optimizer_step(l, kind, hyper, state_grad_scale, bn_momentum_state, bn_momentum_output, false, grad_scale);
}

extern "C" int gnn_loop_set_clipping(gnn_loop *l, double clipvalue, double clipnorm, double global_clipnorm)
{
    ARGCHK(l, "loop is NULL");
    ARGCHK(std::isfinite(clipvalue) && std::isfinite(clipnorm) && std::isfinite(global_clipnorm) && clipvalue >= 0.0 && clipnorm >= 0.0 && global_clipnorm >= 0.0,
           "clipvalue, clipnorm and global_clipnorm must be finite and >= 0 (0 = off)");
    ARGCHK(clipvalue == 0.0 || (float)clipvalue > 0.0f, "clipvalue is below the float32 range of the gradients");
    ARGCHK(!(clipnorm > 0.0 && global_clipnorm > 0.0), "clipnorm and global_clipnorm exclude each other (as in tf.keras)");
    l->train.clip.value = (float)clipvalue; l->train.clip.norm = clipnorm; l->train.clip.global = global_clipnorm;
    return GNN_OK;
}

extern "C" int gnn_loop_set_loss_params(gnn_loop *l, double label_smoothing, double huber_delta)
{
    ARGCHK(l, "loop is NULL");
    ARGCHK(label_smoothing >= 0.0 && label_smoothing <= 1.0, "label_smoothing must lie in [0, 1]");
    ARGCHK(std::isfinite(huber_delta) && huber_delta > 0.0, "huber_delta must be finite and > 0");
    l->train.loss.smoothing = label_smoothing; l->train.loss.delta = huber_delta;
    return GNN_OK;
}

extern "C" int gnn_loop_grad_sqnorm(gnn_loop *l, float state_grad_scale, double *sqnorm, double *penalty)
{
    ARGCHK(l && (sqnorm || penalty), "bad arguments");
    gnn_train_ctx *cx = l->train_ctx;
    if (!cx || !cx->backward_done || cx->applied) return gnn_fail(GNN_ERR_STATE, "no fresh gradients: run gnn_loop_train_step (or forward + backward) first");
    ARGCHK(l->st->n_layers <= 16 && l->ou->n_layers <= 16, "too many layers");
    HIPCHK(hipSetDevice(l->device));
    hipStream_t st = l->stream;
    int rc;
    if (sqnorm) {
        if ((rc = clip_prepare(l, cx, st, state_grad_scale, l->train.clip.value, 0.0, 0.0, 1.0))) return rc;
        HIPCHK(hipMemcpyAsync(sqnorm, cx->sq + 2 * CLIP_SLOTS, sizeof(double), hipMemcpyDeviceToHost, st));
    }
    const unsigned pb = cx->pen_blocks[0] + cx->pen_blocks[1];
    std::vector<double> part(pb);
    if (penalty && pb) HIPCHK(hipMemcpyAsync(part.data(), cx->pen_part, sizeof(double) * pb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (penalty) {
        *penalty = 0.0;
        for (unsigned b = 0; b < pb; ++b) *penalty += part[b];
    }
    return GNN_OK;
}

extern "C" int gnn_loop_update_moving_statistics(gnn_loop *l, float bn_momentum_state, float bn_momentum_output)
{
    ARGCHK(l, "loop is NULL");
    gnn_train_ctx *cx = l->train_ctx;
    if (!cx || cx->applied) return gnn_fail(GNN_ERR_STATE, "no training-mode forward pass to take the batch statistics from");
    HIPCHK(hipSetDevice(l->device));
    hipStream_t st = l->stream;
    auto nets = loop_nets(l, cx);
    const float mom[2] = {bn_momentum_state, bn_momentum_output};
    for (LoopNet &n : nets) {
        if (!n.m->has_bn || n.calls <= 0) continue;
        const int F = n.m->dims.back();
        hipLaunchKernelGGL(k_bn_moving, cdiv(F, 64), 64, 0, st, F, n.calls, n.net->stats_all, mom[&n - nets.data()], n.m->bn_raw);
        HIPCHK(hipGetLastError());
        int rc = gnn_mlp_refresh_bn(n.m, st);
        if (rc) return rc;
        n.m->version++;
        n.m->pack_dirty = true;
    }
    cx->applied = true;                           // once per forward pass
    HIPCHK(hipStreamSynchronize(st));
    return GNN_OK;
}

extern "C" int gnn_loop_arm_optimizer(gnn_loop *l, int kind, const float *hyper, int mean, float bn_momentum_state, float bn_momentum_output)
{
    ARGCHK(l && hyper, "bad arguments");
    if (const char *why = optimizer_args_error(kind, hyper)) return gnn_fail(GNN_ERR_ARG, "%s", why);
    ARGCHK(l->st->n_layers <= 16 && l->ou->n_layers <= 16, "too many layers");
    l->train.opt.armed = true; l->train.opt.kind = kind; l->train.opt.mean = mean != 0;
    for (int i = 0; i < 4; ++i) l->train.opt.h[i] = hyper[i];
    l->train.opt.mom_s = bn_momentum_state; l->train.opt.mom_o = bn_momentum_output;
    return GNN_OK;
}
