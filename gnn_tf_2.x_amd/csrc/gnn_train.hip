// One training step on the device: training-mode forward through the unrolled state loop, loss, back-propagation through
// all executed iterations, optimizer update (reference GNN/GNN_BaseClass.py:231-247 around GNN/GNN.py:180-199, :251-280).
// The step returns the loss, the iteration count, the raw gradients and the BatchNormalization batch statistics of every
// executed body; with gnn_loop_arm_optimizer the Adam / SGD update and the moving statistics are applied on the device too
// (weights, optimizer slots and gradients never leave HBM) and the host waits for the device once per TRAIN_CHUNK bodies
// of the forward pass and once at the end of the step.
//
// Keras training semantics (not in the reference repository; restated in oracle/gnn_train_oracle.py):
//   Dropout: y = x * mask / (1 - rate), fresh mask per call (negative rate: AlphaDropout);  BatchNormalization: batch mean / biased batch variance;
//   categorical_crossentropy(from_logits=False): p = out / sum(out), clip to [1e-7, 1 - 1e-7], -sum t log p.
// Launch structure (the graphs of a training batch are small: the step is bound by the NUMBER of launches, so every body is few,
// fused kernels): forward body = concat + gather + Dropout + gate (k_train_input), one k_dense_fwd per layer, two
// BatchNormalization kernels; backward body = two BatchNormalization kernels, one k_layer_bwd per layer (weight / bias gradient
// tiles beside d h_in, with the Dropout / activation derivative as its epilogue), one k_state_grad_sum.  float32; every
// reduction over rows leaves per-chunk partials that are added in a fixed order (no float atomics, run-to-run identical), so
// results are compared with the float64 oracle to a tolerance, not bit for bit.
//
// Opt-in (gnn_loop_set_train_recompute): the forward keeps of every body its output state, statistics and gate alone, and train_backward rebuilds
// a body's cache (body_forward, the function the first pass ran) right before that body's backward pass - same bits, one body's cache alive.
//
// This unit is the step itself: the concat and the gather / scatter between the state and net_output, the loss, the label gradients,
// train_forward / train_backward and their entry points.  gnn_train_net.hip: one Sequential in training mode (net_setup, which also
// decides once per step which kernels the net's calls take, net_forward, net_backward).  gnn_train_wide.hip: the matrix-core products
// and their launchers.  gnn_train_update.hip: regularizers, clipping, optimizer rules, moving statistics.  gnn_train.h: what they share.
#include <stdlib.h>
#include <string.h>

#include <cmath>

#include "gnn_train.h"

using namespace gnn_train;

namespace {

// The concat of one body (reference GNN/GNN.py:223-239) in one pass: [state | node labels | aggregated states | aggregated labels |
// aggregated arc labels].  Everything but the state columns and their aggregate is loop-invariant and comes from the template.
// Dropout in front of the first Dense layer (rate != 0) is applied on the way out (own masks: stream `key`, element idx0 + i - idx0, the
// elements of the lower ranks' rows, enters the hashed index only).  The thread of column 0 also evaluates the
// while-condition of THIS body for its node (reference GNN/GNN.py:202-220: condition(state, state_old), ascending-feature sums as
// k_check; so == NULL: ones) and raises the body's gate.
// state: row 0 of the state REPLICA (the sources of the arcs are replica rows); own: the first OWNED row of it (== state on one GPU)
__global__ void __launch_bounds__(256) k_train_input(int64_t n, int in_s, int Ds, int c_aggs, const float *__restrict__ tmpl, const float *__restrict__ state,
                                                     const float *__restrict__ own,
                                                     const int32_t *__restrict__ indptr, const int32_t *__restrict__ adj_src,
                                                     const float *__restrict__ adj_w, float rate, const uint8_t *mask_in, uint64_t key, int64_t idx0, uint8_t *keep,
                                                     float *__restrict__ inp, const float *__restrict__ so, float thr, int *flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int f = 0;
    if (i < n * in_s) {
        // (a 64-bit division is some forty instructions: the 32-bit one when the matrix has fewer than 2^31 elements)
        const int64_t r = n * in_s < ((int64_t)1 << 31) ? (int64_t)((unsigned)i / (unsigned)in_s) : i / in_s;
        const int c = (int)(i - r * in_s);
        float v;
        bool skip = false;                         // Ds % 4 == 0: the thread of every fourth aggregate column gathers and writes four
        if (c < Ds) v = own[r * Ds + c];
        else if (c >= c_aggs && c < c_aggs + Ds) {
            const int cc = c - c_aggs;
            v = 0.0f;
            if ((Ds & 3) == 0 && rate == 0.0f) {
                skip = true;
                if ((cc & 3) == 0) {
                    float4 a4 = {0.0f, 0.0f, 0.0f, 0.0f};
                    const int32_t e1 = indptr[r + 1];
                    for (int32_t e = indptr[r]; e < e1; e += 4) {          // four arcs per step: their loads are in flight together
                        float w[4];
                        float4 x[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const bool in = e + u < e1;
                            w[u] = in ? adj_w[e + u] : 0.0f;
                            x[u] = in ? *reinterpret_cast<const float4 *>(state + (int64_t)adj_src[e + u] * Ds + cc) : float4{0.0f, 0.0f, 0.0f, 0.0f};
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (e + u < e1) {
                                a4.x = __builtin_fmaf(w[u], x[u].x, a4.x); a4.y = __builtin_fmaf(w[u], x[u].y, a4.y);
                                a4.z = __builtin_fmaf(w[u], x[u].z, a4.z); a4.w = __builtin_fmaf(w[u], x[u].w, a4.w);
                            }
                    }
                    inp[i] = a4.x; inp[i + 1] = a4.y; inp[i + 2] = a4.z; inp[i + 3] = a4.w;
                }
            } else {
                const int32_t e1 = indptr[r + 1];
                for (int32_t e = indptr[r]; e < e1; e += 4) {
                    float w[4], x[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool in = e + u < e1;
                        w[u] = in ? adj_w[e + u] : 0.0f;
                        x[u] = in ? state[(int64_t)adj_src[e + u] * Ds + cc] : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (e + u < e1) v = __builtin_fmaf(w[u], x[u], v);
                }
            }
        } else
            v = tmpl[i];
        if (rate != 0.0f) {
            const float rr = fabsf(rate);
            uint8_t kp;
            if (mask_in) kp = mask_in[i] != 0;
            else kp = dropout_keep(key, (uint64_t)(idx0 + i), rr);
            keep[i] = kp;
            if (rate < 0.0f) {
                float a, b, ap;
                alpha_dropout_coeffs(rr, &a, &b, &ap);
                v = a * (kp ? v : ap) + b;
            } else
                v = kp ? v / (1.0f - rate) : 0.0f;
        }
        if (!skip) inp[i] = v;
        if (c == 0) {
            float dist = 0.0f, nrm = 0.0f;
            if ((Ds & 3) == 0) {
#pragma unroll 4
                for (int q = 0; q < Ds; q += 4) {
                    const float4 sv = *reinterpret_cast<const float4 *>(own + r * Ds + q);
                    const float4 ov = so ? *reinterpret_cast<const float4 *>(so + r * Ds + q) : float4{1.0f, 1.0f, 1.0f, 1.0f};
                    const float d0 = sv.x - ov.x, d1 = sv.y - ov.y, d2 = sv.z - ov.z, d3 = sv.w - ov.w;
                    dist = dist + d0 * d0; nrm = nrm + ov.x * ov.x;
                    dist = dist + d1 * d1; nrm = nrm + ov.y * ov.y;
                    dist = dist + d2 * d2; nrm = nrm + ov.z * ov.z;
                    dist = dist + d3 * d3; nrm = nrm + ov.w * ov.w;
                }
            } else
                for (int q = 0; q < Ds; ++q) {
                    const float o = so ? so[r * Ds + q] : 1.0f;
                    const float df = own[r * Ds + q] - o;
                    dist = dist + df * df;
                    nrm = nrm + o * o;
                }
            f = sqrtf(dist) > thr * sqrtf(nrm);
        }
    }
    if (__any(f) && (threadIdx.x & 63) == 0) gnn_flag_raise(flag);
}

// The same concat for many rows without Dropout in front of the first layer (state width a multiple of 4, <= 64): 16 lanes per row,
// each gathering four aggregate columns (four arcs in flight, the fmaf chain in stored order) and copying four state columns and the
// template columns; the while-condition of the body is evaluated by k_check (gnn_launch_check: same ascending-feature sums) beside it.
// k_train_input gave the condition to the thread of column 0 - a 64-step chain that the other 63 lanes of its wave waited for - and ran
// one thread per element: 3.2 ms per body at 1 M rows x 135 columns, this one about a quarter of that (profiles/r03_train_c3.txt).
__global__ void __launch_bounds__(256) k_train_input_rows(int64_t n, int in_s, int Ds, int c_aggs, const float *__restrict__ tmpl, const float *__restrict__ state,
                                                          const float *__restrict__ own_rows,
                                                          const int32_t *__restrict__ indptr, const int32_t *__restrict__ adj_src,
                                                          const float *__restrict__ adj_w, float *__restrict__ inp)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 4;
    const int j = (int)(t & 15);
    if (r >= n) return;
    float *row = inp + r * in_s;
    const int cc = 4 * j;
    if (cc < Ds) {
        const float4 own = *reinterpret_cast<const float4 *>(own_rows + r * Ds + cc);
        float4 a4 = {0.0f, 0.0f, 0.0f, 0.0f};
        const int32_t e1 = indptr[r + 1];
        for (int32_t e = indptr[r]; e < e1; e += 4) {
            float w[4];
            float4 x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool in = e + u < e1;
                w[u] = in ? adj_w[e + u] : 0.0f;
                x[u] = in ? *reinterpret_cast<const float4 *>(state + (int64_t)adj_src[e + u] * Ds + cc) : float4{0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e + u < e1) {
                    a4.x = __builtin_fmaf(w[u], x[u].x, a4.x); a4.y = __builtin_fmaf(w[u], x[u].y, a4.y);
                    a4.z = __builtin_fmaf(w[u], x[u].z, a4.z); a4.w = __builtin_fmaf(w[u], x[u].w, a4.w);
                }
        }
        row[cc] = own.x; row[cc + 1] = own.y; row[cc + 2] = own.z; row[cc + 3] = own.w;
        float *ag = row + c_aggs + cc;
        ag[0] = a4.x; ag[1] = a4.y; ag[2] = a4.z; ag[3] = a4.w;
    }
    // template columns: [Ds, c_aggs) and [c_aggs + Ds, in_s)
    const int n1 = c_aggs - Ds, nt = n1 + (in_s - c_aggs - Ds);
    for (int q = j; q < nt; q += 16) {
        const int c = q < n1 ? Ds + q : c_aggs + Ds + (q - n1);
        row[c] = tmpl[r * in_s + c];
    }
}

__global__ void k_gather_feats(int64_t m, const int32_t *rows, const float *state, int Ds, const float *nodes, int NL, int NLc, float *feats)
{
    const int wf = Ds + NLc;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * wf) return;
    const int64_t q = t / wf;
    const int c = (int)(t - q * wf);
    const int64_t row = rows[q];
    feats[t] = c < Ds ? state[row * Ds + c] : nodes[row * NL + (c - Ds)];
}

__global__ void k_scatter_rows(int64_t m, const int32_t *rows, const float *d_feats, int wf, int Ds, float *d_state)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * Ds) return;
    const int64_t q = t / Ds;
    const int c = (int)(t - q * Ds);
    d_state[(int64_t)rows[q] * Ds + c] = d_feats[q * wf + c];
}

// One target row of the loss: returns w L(t, o) and writes d / d o [T], arithmetic in double.  `smooth` is label_smoothing (applied to
// the targets first: t <- t (1 - s) + s / T for the categorical kinds, + s / 2 for the binary ones), `delta` the Huber threshold.
//   0 categorical_crossentropy (probabilities, renormalised, clipped to [1e-7, 1 - 1e-7]: no gradient where clipped)
//   1 mean_squared_error        2 categorical_crossentropy(from_logits=True): softmax inside the loss, no clipping
//   3 binary_crossentropy (probabilities, clipped like 0)       4 binary_crossentropy(from_logits=True)
//   5 mean_absolute_error (sign(0) = 0)                          6 huber (quadratic up to and including |e| = delta)
enum { LOSS_KINDS = 7 };
#define LOSS_KIND_TEXT "loss_kind: 0 categorical_crossentropy, 1 mean_squared_error, 2 categorical_crossentropy(from_logits=True), 3 binary_crossentropy, " \
                       "4 binary_crossentropy(from_logits=True), 5 mean_absolute_error, 6 huber"

__host__ __device__ inline double loss_row(int kind, int T, const float *ti, const float *oi, double wi, double smooth, double delta, float *d)
{
    const double keep = 1.0 - smooth, add = (kind == 3 || kind == 4) ? smooth / 2 : smooth / T;
    double li = 0.0;
    if (kind == 0) {
        double s = 0.0, gp = 0.0;
        for (int j = 0; j < T; ++j) s += oi[j];
        for (int j = 0; j < T; ++j) {
            const double tj = ti[j] * keep + add, pj = oi[j] / s;
            const bool in = pj >= 1e-7 && pj <= 1.0 - 1e-7;
            const double pc = fmin(fmax(pj, 1e-7), 1.0 - 1e-7);
            li -= tj * log(pc);
            gp += (in ? -tj / pc : 0.0) * pj;
        }
        for (int j = 0; j < T; ++j) {
            const double tj = ti[j] * keep + add, pj = oi[j] / s;
            const bool in = pj >= 1e-7 && pj <= 1.0 - 1e-7;
            const double pc = fmin(fmax(pj, 1e-7), 1.0 - 1e-7);
            d[j] = (float)(wi * ((in ? -tj / pc : 0.0) - gp) / s);
        }
        return wi * li;
    }
    if (kind == 2) {
        double mx = oi[0], s = 0.0, st = 0.0;
        for (int j = 1; j < T; ++j) mx = fmax(mx, (double)oi[j]);
        for (int j = 0; j < T; ++j) { s += exp(oi[j] - mx); st += ti[j] * keep + add; }
        for (int j = 0; j < T; ++j) {
            const double tj = ti[j] * keep + add, logp = (oi[j] - mx) - log(s);
            li -= tj * logp;
            d[j] = (float)(wi * (exp(logp) * st - tj));
        }
        return wi * li;
    }
    for (int j = 0; j < T; ++j) {
        const double o = oi[j];
        if (kind == 3) {
            const double tj = ti[j] * keep + add;
            const bool in = o >= 1e-7 && o <= 1.0 - 1e-7;
            const double pc = fmin(fmax(o, 1e-7), 1.0 - 1e-7);
            li -= tj * log(pc) + (1.0 - tj) * log(1.0 - pc);
            d[j] = (float)(in ? wi * ((1.0 - tj) / (1.0 - pc) - tj / pc) / T : 0.0);
        } else if (kind == 4) {
            const double tj = ti[j] * keep + add, en = exp(-fabs(o));
            li += fmax(o, 0.0) - o * tj + log1p(en);
            const double sig = o >= 0.0 ? 1.0 / (1.0 + en) : en / (1.0 + en);
            d[j] = (float)(wi * (sig - tj) / T);
        } else if (kind == 5) {
            const double e = o - ti[j];
            li += fabs(e);
            d[j] = (float)(wi * (e > 0.0 ? 1.0 : e < 0.0 ? -1.0 : 0.0) / T);
        } else if (kind == 6) {
            const double e = o - ti[j], ae = fabs(e);
            li += ae <= delta ? 0.5 * e * e : delta * (ae - 0.5 * delta);
            d[j] = (float)(wi * (ae <= delta ? e : (e > 0.0 ? delta : -delta)) / T);
        } else {
            const double e = o - ti[j];
            li += e * e;
            d[j] = (float)(wi * 2.0 * e / T);
        }
    }
    return wi * li / T;
}

// host side of the loss (rows are few): sum_i w_i L(t_i, o_i) and d / d o
void loss_host(int kind, int64_t n, int T, const float *t, const float *o, const float *w, double smooth, double delta, double *loss, std::vector<float> &d_o)
{
    d_o.assign((size_t)n * T, 0.0f);
    double total = 0.0;
    for (int64_t i = 0; i < n; ++i) total += loss_row(kind, T, t + i * T, o + i * T, w[i], smooth, delta, d_o.data() + i * T);
    *loss = total;
}

// The same on the device, one thread per target row: d_o [n, T] and, per block of 256 rows, the sum of w_i L_i (fixed tree, double)
__global__ void __launch_bounds__(256) k_loss_rows(int kind, int64_t n, int T, const float *t, const float *o, const float *w, double smooth, double delta,
                                                   float *d_o, double *loss_part)
{
    __shared__ double sl[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double lw = 0.0;
    if (i < n) lw = loss_row(kind, T, t + i * T, o + i * T, w[i], smooth, delta, d_o + i * T);
    sl[threadIdx.x] = lw;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sl[threadIdx.x] += sl[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_part[blockIdx.x] = sl[0];
}

// GNNgraphBased readout inside the step: og = NodeGraph^T . out_nodes (GNN.py:331-332) over the CSR by graph, one wave per graph
// (lanes take every 64th entry, then a fixed butterfly adds the lanes), and its transpose
__global__ void __launch_bounds__(256) k_graph_out(int n_graphs, int T, const int32_t *__restrict__ ng_indptr, const int32_t *__restrict__ ng_node,
                                                   const float *__restrict__ ng_w, const float *__restrict__ out_nodes, float *og)
{
    const int gi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (gi >= n_graphs) return;
    const int e0 = ng_indptr[gi], e1 = ng_indptr[gi + 1];
    for (int c = 0; c < T; ++c) {
        float acc = 0.0f;
        for (int e = e0 + lane; e < e1; e += 64) acc += ng_w[e] * out_nodes[(int64_t)ng_node[e] * T + c];
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if (lane == 0) og[gi * T + c] = acc;
    }
}

// d out_nodes[node, c] = w * d og[graph of the entry, c]: one thread per entry and column, the entry's graph by bisection
__global__ void k_graph_out_bwd(int n_graphs, int T, const int32_t *__restrict__ ng_indptr, const int32_t *__restrict__ ng_node,
                                const float *__restrict__ ng_w, const float *__restrict__ d_og, float *d_nodes)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int ne = ng_indptr[n_graphs];
    if (t >= ne * T) return;
    const int e = t / T, c = t - e * T;
    int lo = 0, hi = n_graphs;                 // largest lo with ng_indptr[lo] <= e
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ng_indptr[mid] <= e) lo = mid; else hi = mid; }
    // a node belongs to one graph: the adds of different threads do not meet (atomic only so that a malformed NodeGraph stays defined)
    atomicAdd(&d_nodes[(int64_t)ng_node[e] * T + c], ng_w[e] * d_og[lo * T + c]);
}

// d_nodes[r, c] += d_inp[r, c_nodes + c] + via[r, c]   (direct label columns of the concat + transposed aggregated_nodes)
__global__ void k_nodes_grad(int64_t n, int NL, const float *d_inp, int in_s, int c_nodes, const float *via, float *d_nodes)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * NL) return;
    const int64_t r = t / NL;
    const int c = (int)(t - r * NL);
    d_nodes[t] += d_inp[r * in_s + c_nodes + c] + via[t];
}

// d_nodes[rows[q], c] += d_feats[q, Ds + c]   (label columns of net_output's input; rows are unique)
__global__ void k_scatter_label_grad(int64_t m, const int32_t *rows, const float *d_feats, int wf, int Ds, int NL, float *d_nodes)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * NL) return;
    const int64_t q = t / NL;
    const int c = (int)(t - q * NL);
    d_nodes[(int64_t)rows[q] * NL + c] += d_feats[q * wf + Ds + c];
}

// GNNedgeBased backward: row q of d_feats = d [F[dst(e)] | F[src(e)] | arc label], e = rows[q]; F = [state | labels?].  Both endpoints
// receive their half.  Several arcs share a node: every (node, column) is one thread that adds the halves of the node's masked arcs in
// ascending arc order (gnn_loop_set_edge_readout builds the incidence lists) on top of what d_state / d_nodes hold - no float atomics,
// so edge-based steps are run-to-run identical like the others (round 3; the scatter with atomicAdd was not).
__global__ void k_gather_edge_grad(int64_t n, const int32_t *__restrict__ inc_ptr, const int32_t *__restrict__ inc, const float *__restrict__ d_feats, int we,
                                   int wn, int Ds, int NL, float *d_state, float *d_nodes)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * wn) return;
    const int64_t node = t / wn;
    const int c = (int)(t - node * wn);
    float *dst = c < Ds ? d_state + node * Ds + c : (d_nodes ? d_nodes + node * NL + (c - Ds) : nullptr);
    if (!dst) return;
    float v = *dst;
    for (int32_t i = inc_ptr[node]; i < inc_ptr[node + 1]; ++i) {
        const int32_t x = inc[i];
        v = v + d_feats[(int64_t)(x >> 1) * we + (x & 1) * wn + c];
    }
    *dst = v;
}

// acc[r, c] += d_inp[r, col0 + c]   (the loop-invariant aggregated arc labels receive gradient from every body)
__global__ void k_add_cols(int64_t n, int width, const float *d_inp, int in_s, int col0, float *acc)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * width) return;
    const int64_t r = t / width;
    const int c = (int)(t - r * width);
    acc[t] += d_inp[r * in_s + col0 + c];
}

// out[q, c] += src[rows[q], col0 + c]   (a chained backward pass: the rows of the layer above's label gradient that carry this loop's masked
// outputs, added onto d loss / d out_nodes; one thread per element of out)
__global__ void k_add_masked_cols(int64_t m, int width, const int32_t *__restrict__ rows, const float *__restrict__ src, int stride, int col0, float *out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * width) return;
    const int64_t q = t / width;
    const int c = (int)(t - q * width);
    out[t] += src[(int64_t)rows[q] * stride + col0 + c];
}

// d arc labels, ORIGINAL arc order.  (a) label columns of the per-arc readout rows: row m <-> arc position rows[m];
// (b) ArcNode^T . arc labels: entry q of destination dst carries arc arc_id[q] with weight arc_w[q].  Targets are unique.
__global__ void k_arc_grad_readout(int64_t m, int AL, const int32_t *rows, const float *d_feats, int we, int col0, float *d_arcs)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * AL) return;
    const int64_t q = t / AL;
    const int c = (int)(t - q * AL);
    d_arcs[(int64_t)rows[q] * AL + c] += d_feats[q * we + col0 + c];
}

__global__ void k_arc_grad_agg(int64_t e, int AL, const int32_t *entry_dst, const int32_t *arc_id, const float *arc_w, const float *d_agg, float *d_arcs)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= e * AL) return;
    const int64_t q = t / AL;
    const int c = (int)(t - q * AL);
    d_arcs[(int64_t)arc_id[q] * AL + c] += arc_w[q] * d_agg[(int64_t)entry_dst[q] * AL + c];
}

__global__ void k_axpy1(int64_t n, const float *x, float *y)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) y[t] += x[t];
}

constexpr int TRAIN_CHUNK = 5;     // bodies enqueued between two looks at the iteration gates (see train_forward)

}   // namespace

void gnn_train_ctx_free(gnn_loop *l)
{
    if (l) { delete l->train_ctx; l->train_ctx = nullptr; }
}

void gnn_train_arena_free(gnn_loop *l)
{
    if (l) { delete l->train_arena; l->train_arena = nullptr; }
}

// the loop's arena; created on first use
static gnn_train_arena *loop_arena(gnn_loop *l)
{
    if (!l->train_arena) l->train_arena = new gnn_train_arena();
    return l->train_arena;
}

extern "C" int gnn_loss_grad_ex(int loss_kind, int64_t n_rows, int n_out, const float *targets, const float *out, const float *sample_weights,
                                double label_smoothing, double huber_delta, double *loss, float *d_out)
{
    ARGCHK((n_rows == 0 || (targets && out && sample_weights)) && loss && n_out > 0 && n_rows >= 0, "bad arguments");
    ARGCHK(loss_kind >= 0 && loss_kind < LOSS_KINDS, LOSS_KIND_TEXT);
    ARGCHK(label_smoothing >= 0.0 && label_smoothing <= 1.0, "label_smoothing must lie in [0, 1]");
    ARGCHK(std::isfinite(huber_delta) && huber_delta > 0.0, "huber_delta must be finite and > 0");
    std::vector<float> d;
    loss_host(loss_kind, n_rows, n_out, targets, out, sample_weights, label_smoothing, huber_delta, loss, d);
    if (d_out && n_rows) memcpy(d_out, d.data(), sizeof(float) * d.size());
    return GNN_OK;
}

extern "C" int gnn_loss_grad(int loss_kind, int64_t n_rows, int n_out, const float *targets, const float *out, const float *sample_weights,
                             double *loss, float *d_out)
{
    return gnn_loss_grad_ex(loss_kind, n_rows, n_out, targets, out, sample_weights, 0.0, 1.0, loss, d_out);
}

// owned rows [n_rows, Ds] -> a fresh replica [N_pad, Ds] with the rows of all ranks (all-gather in place); sharded training only
static int train_replicate(gnn_loop *l, Buf &buf, hipStream_t st, const float *own_rows, float **replica)
{
    const int Ds = l->Ds;
    const size_t replica_floats = (size_t)l->N_pad * Ds, shard_floats = (size_t)l->shard_rows * Ds;
    int rc;
    if ((rc = buf.get(replica, replica_floats))) return rc;
    HIPCHK(hipMemsetAsync(*replica, 0, sizeof(float) * replica_floats, st));        // rows past the last shard's end are never read, but stay finite
    if (l->g->n_rows) HIPCHK(hipMemcpyAsync(*replica + (size_t)l->own_off * Ds, own_rows, sizeof(float) * (size_t)l->g->n_rows * Ds, hipMemcpyDeviceToDevice, st));
    return gnn_comm_allgather32(l->comm, *replica + (size_t)l->rank * shard_floats, *replica, shard_floats, st);
}

// the caller's by-source CSR (N rows, Es arcs, checked by the caller) on the device: cx->d_sip / d_sdst / d_sw
static int upload_by_source(gnn_train_ctx *cx, int64_t N, int64_t Es, const int32_t *src_indptr, const int32_t *src_dst, const float *src_w)
{
    int rc;
    if ((rc = cx->buf.get(&cx->d_sip, (size_t)N + 1)) || (rc = cx->buf.get(&cx->d_sdst, (size_t)Es)) || (rc = cx->buf.get(&cx->d_sw, (size_t)Es))) return rc;
    HIPCHK(hipMemcpy(cx->d_sip, src_indptr, sizeof(int32_t) * (N + 1), hipMemcpyHostToDevice));
    if (Es) { HIPCHK(hipMemcpy(cx->d_sdst, src_dst, sizeof(int32_t) * Es, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(cx->d_sw, src_w, sizeof(float) * Es, hipMemcpyHostToDevice)); }
    return GNN_OK;
}

// the graph's own by-source copy of its adjacency (gnn_graph_shared::src_*), built once from its CSR by destination (a stable counting
// sort by source keeps destinations ascending)
static int graph_by_source(gnn_graph *g)
{
    gnn_graph_shared *sh = g->sh;
    if (sh->src_indptr) return GNN_OK;
    const int64_t N = g->n_rows, E = g->E;
    std::vector<int32_t> ip((size_t)N + 1), src((size_t)E), sip((size_t)N + 1, 0), sdst((size_t)E);
    std::vector<float> w((size_t)E), sw((size_t)E);
    HIPCHK(hipMemcpy(ip.data(), sh->indptr, sizeof(int32_t) * (N + 1), hipMemcpyDeviceToHost));
    if (E) { HIPCHK(hipMemcpy(src.data(), sh->adj_src, sizeof(int32_t) * E, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(w.data(), sh->adj_w, sizeof(float) * E, hipMemcpyDeviceToHost)); }
    for (int64_t e = 0; e < E; ++e) ++sip[(size_t)src[e] + 1];
    for (int64_t i = 0; i < N; ++i) sip[i + 1] += sip[i];
    std::vector<int32_t> fill(sip.begin(), sip.end() - 1);
    for (int64_t d = 0; d < N; ++d)
        for (int32_t e = ip[d]; e < ip[d + 1]; ++e) { const int32_t q = fill[src[e]]++; sdst[q] = (int32_t)d; sw[q] = w[e]; }
    if (gnn_dev_malloc((void **)&sh->src_indptr, sizeof(int32_t) * (N + 1)) != hipSuccess || gnn_dev_malloc((void **)&sh->src_dst, sizeof(int32_t) * std::max<int64_t>(E, 1)) != hipSuccess ||
        gnn_dev_malloc((void **)&sh->src_w, sizeof(float) * std::max<int64_t>(E, 1)) != hipSuccess)
        return gnn_fail(GNN_ERR_HIP, "hipMalloc of the by-source adjacency failed");
    HIPCHK(hipMemcpy(sh->src_indptr, sip.data(), sizeof(int32_t) * (N + 1), hipMemcpyHostToDevice));
    if (E) { HIPCHK(hipMemcpy(sh->src_dst, sdst.data(), sizeof(int32_t) * E, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(sh->src_w, sw.data(), sizeof(float) * E, hipMemcpyHostToDevice)); }
    return GNN_OK;
}

// Body `it` of net_state from cx->states[it]: the concat by the input kernel the rows and rates ask for (with the body's gate, where
// check_gate is set), then net_forward; c: the body's cache, *y: its output state.  The first pass and the replay of the recomputing step
// (train_backward) are this one function: same kernels, same mask stream MaskStream{seed, 0, it, row0} or slice of the injected masks.
// check_gate = false (a replayed body): no gate is evaluated - gnn_launch_check is skipped, and the kernels that evaluate a gate in passing
// (k_train_input, k_mlp_fwd) raise the scratch block `gate`.
static int body_forward(gnn_loop *l, gnn_train_ctx *cx, hipStream_t st, int it, int *gate, bool check_gate, NetCache &c, float **y, gnn_comm *comm,
                        const FwdMode &mode)
{
    gnn_graph *g = l->g;
    Buf &buf = cx->buf;
    const bool sharded = l->world > 1;
    const int64_t N = cx->N;
    const size_t own_off = sharded ? (size_t)l->own_off : 0;
    const int Ds = l->Ds, in_s = l->in_s, c_aggs = Ds + l->NLc;
    int rc;
    float *inp = nullptr;
    uint8_t *keep0 = nullptr;
    const float r0 = cx->ns.rate[0];
    if ((rc = buf.get(&inp, (size_t)N * in_s))) return rc;
    if (r0 != 0.0f && (rc = buf.get(&keep0, (size_t)N * in_s))) return rc;
    const uint8_t *mk = cx->d_masks_s ? cx->d_masks_s + cx->mask_iter_bytes * (size_t)it : nullptr;
    const MaskStream rng{cx->seed, 0, it, sharded ? g->row_begin : 0};
    const float *state = cx->states[it], *own_cur = state + own_off * Ds, *own_prev = it ? cx->states[it - 1] + own_off * Ds : (const float *)nullptr;
    // few rows: k_mlp_fwd builds the concat rows itself (one launch for input + all Dense layers) and evaluates the gate
    const InputBuild build{Ds, c_aggs, cx->tmpl, state, own_cur, own_prev, g->sh->indptr, g->sh->adj_src, g->sh->adj_w, l->thr, gate};
    if (cx->ns.build_input || N == 0) {
        // (a rank without rows: nothing to compute, it only takes part in the exchanges below)
    } else if (r0 == 0.0f && state_rows16(Ds, N)) {
        // many rows: the concat 16 lanes per row, gate i = condition(state_i, state_{i-1}) by k_check beside it
        hipLaunchKernelGGL(k_train_input_rows, cdiv(N * 16, 256), 256, 0, st, N, in_s, Ds, c_aggs, cx->tmpl, state, own_cur, g->sh->indptr, g->sh->adj_src,
                           g->sh->adj_w, inp);
        HIPCHK(hipGetLastError());
        if (check_gate && (rc = gnn_launch_check(st, N, Ds, own_cur, own_prev, l->thr, gate))) return rc;
    } else {
        // the input kernel of body i also evaluates gate i = condition(state_i, state_{i-1})
        hipLaunchKernelGGL(k_train_input, cdiv(N * in_s, 256), 256, 0, st, N, in_s, Ds, c_aggs, cx->tmpl, state, own_cur, g->sh->indptr, g->sh->adj_src,
                           g->sh->adj_w, r0, mk, dropout_key(cx->seed, 0, it, 0), rng.row0 * in_s, keep0, inp, own_prev, l->thr, gate);
        HIPCHK(hipGetLastError());
    }
    return net_forward(st, buf, cx->ns, inp, keep0, mk, rng, c, y, comm, &build, mode);
}

// One training-mode forward: what its steps (below, in the order train_forward takes them) share
struct Forward {
    gnn_loop *l;
    gnn_train_ctx *cx;
    hipStream_t st;
    bool sharded;
    gnn_comm *comm;               // sharded: the loop's communicator
    int64_t N, M;
    size_t own_off;               // replica row of the first owned row
    const float *dropout_state;
    uint64_t seed;
    size_t flag_words;
    int *flags, *hflags, *flags_all;      // the iteration gates: device, pinned host copy, (sharded) those of all ranks
    uint8_t *d_masks_o;           // injected Dropout masks of net_output (else nullptr: own generator)
    // (the state tables, the template of the concat and net_state's injected masks: gnn_train_ctx - a replayed body reads them again)

    // Adjacency by source for the transposed aggregation of the backward pass: the caller's arrays, or (NULL) the graph's own copy
    int by_source(const int32_t *src_indptr, const int32_t *src_dst, const float *src_w)
    {
        const int64_t E = l->g->E;
        int rc;
        if (sharded) {
            // the backward pass on shards needs the arcs that LEAVE the owned rows (by-source CSR over the owned rows, destinations as
            // replica rows): the caller's arrays, or none - gnn_loop_train_backward is then refused
            if (src_indptr) {
                const int64_t Es = src_indptr[N];
                ARGCHK(src_indptr[0] == 0 && Es >= 0 && (Es == 0 || (src_dst && src_w)), "bad by-source CSR");
                if ((rc = upload_by_source(cx, N, Es, src_indptr, src_dst, src_w))) return rc;
            }
            // rows and masked rows of all ranks (BatchNormalization's backward pass divides by them)
            int *cnt = nullptr, *cnt_all = nullptr;
            if ((rc = cx->buf.get(&cnt, (size_t)4)) || (rc = cx->buf.get(&cnt_all, (size_t)4 * l->world))) return rc;
            const int mine[4] = {(int)N, (int)M, 0, 0};
            HIPCHK(hipMemcpy(cnt, mine, sizeof(mine), hipMemcpyHostToDevice));
            if ((rc = gnn_comm_allgather32(comm, cnt, cnt_all, 4, st))) return rc;
            std::vector<int> all((size_t)4 * l->world);
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipMemcpy(all.data(), cnt_all, sizeof(int) * all.size(), hipMemcpyDeviceToHost));
            for (int p = 0; p < l->world; ++p) {
                cx->N_global += all[(size_t)4 * p]; cx->M_global += all[(size_t)4 * p + 1];
                if (p < l->rank) cx->M_before += all[(size_t)4 * p + 1];
            }
        } else if (src_indptr) {
            ARGCHK(src_indptr[0] == 0 && src_indptr[N] == E && (E == 0 || (src_dst && src_w)), "bad by-source CSR");
            if ((rc = upload_by_source(cx, N, E, src_indptr, src_dst, src_w))) return rc;
        } else {
            if ((rc = graph_by_source(l->g))) return rc;
            cx->d_sip = l->g->sh->src_indptr; cx->d_sdst = l->g->sh->src_dst; cx->d_sw = l->g->sh->src_w;
        }
        return GNN_OK;
    }

    // template of the concat with the loop-invariant columns filled in (GNN.py:259, :263)
    int concat_template()
    {
        gnn_graph *g = l->g;
        const int in_s = l->in_s, c_nodes = l->Ds, c_aggn = l->Ds + l->NLc + l->Ds, c_agga = c_aggn + l->NLc;
        int rc;
        float *tmpl = cx->tmpl;
        if ((rc = gnn_launch_spmm(st, N, g->sh->indptr, nullptr, g->sh->arc_w, gnn_graph_arc_labels(g), g->AL, g->AL, tmpl + c_agga, in_s, nullptr, 1))) return rc;
        if (l->D) {
            if ((rc = gnn_launch_spmm(st, N, g->sh->indptr, g->sh->adj_src, g->sh->adj_w, g->nodes, g->NL, g->NL, tmpl + c_aggn, in_s, nullptr, 1))) return rc;
            if ((rc = gnn_launch_copy_cols(st, N, g->NL, g->nodes + (size_t)g->own_off * g->NL, g->NL, tmpl + c_nodes, in_s, nullptr, 1))) return rc;
        }
        return GNN_OK;
    }

    // the caller's Dropout masks on the device
    int upload_masks(const float *dropout_output, const uint8_t *masks_state, const uint8_t *masks_output)
    {
        Buf &buf = cx->buf;
        size_t &mask_iter_bytes = cx->mask_iter_bytes;
        uint8_t *&d_masks_s = cx->d_masks_s;
        int rc;
        // masks of one iteration of net_state: sum over the dropout positions of N * width bytes
        for (int i = 0; i <= l->st->n_layers; ++i) if (dropout_state[i] != 0.0f) mask_iter_bytes += (size_t)N * l->st->dims[i];
        size_t mask_out_bytes = 0;
        for (int i = 0; i <= l->ou->n_layers; ++i) if (dropout_output[i] != 0.0f) mask_out_bytes += (size_t)M * l->ou->dims[i];
        if (masks_state && mask_iter_bytes) {
            if ((rc = buf.get(&d_masks_s, mask_iter_bytes * (size_t)l->max_iter))) return rc;
            HIPCHK(hipMemcpy(d_masks_s, masks_state, mask_iter_bytes * (size_t)l->max_iter, hipMemcpyHostToDevice));
        }
        if (masks_output && mask_out_bytes) {
            if ((rc = buf.get(&d_masks_o, mask_out_bytes))) return rc;
            HIPCHK(hipMemcpy(d_masks_o, masks_output, mask_out_bytes, hipMemcpyHostToDevice));
        }
        return GNN_OK;
    }

    // body `enq`: the concat of states[enq] with its gate, net_state on it, the new state appended to states.
    // Recomputing step (cx->recompute): the new state table is allocated first and is all the arena keeps of the body - its concat, Dense
    // outputs, xhat, keep bytes and weight images are handed out again for the next body (the statistics and the gate live in the zeroed block)
    int enqueue_body(int enq)
    {
        Buf &buf = cx->buf;
        int rc;
        float *y = nullptr;
        int *gate = flags + (size_t)enq * GNN_FLAG_WORDS;
        if (cx->recompute) {
            FwdMode mode;
            NetCache scratch;
            if ((rc = buf.get(&mode.y_dst, (size_t)std::max<int64_t>(N, 1) * l->Ds))) return rc;
            mode.cacheless = l->train.recompute == 1;
            mode.cacheless_chain = &cx->cacheless_chain;
            const gnn_train_arena::Mark mark = buf.arena->mark();
            if ((rc = body_forward(l, cx, st, enq, gate, true, scratch, &y, nullptr, mode))) return rc;
            buf.arena->rewind(mark);
            cx->states.push_back(y);
            return GNN_OK;
        }
        cx->caches.emplace_back();
        if ((rc = body_forward(l, cx, st, enq, gate, true, cx->caches.back(), &y, comm, FwdMode()))) return rc;
        if (sharded) {                               // the new rows of all ranks: what the next body gathers from
            float *rep = nullptr;
            if ((rc = train_replicate(l, buf, st, y, &rep))) return rc;
            y = rep;
        }
        cx->states.push_back(y);
        return GNN_OK;
    }

    // one synchronisation: the gates of the `enq` bodies enqueued so far; *k = the first closed one (else it stays < 0)
    int read_gates(int enq, int *k)
    {
        int rc;
        if (sharded) {                               // the gates of all ranks (GNN.py:218: reduce_any over ALL nodes)
            if ((rc = gnn_comm_allgather32(comm, flags, flags_all, flag_words, st))) return rc;
            HIPCHK(hipMemcpyAsync(hflags, flags_all, sizeof(int) * flag_words, hipMemcpyDeviceToHost, st));     // rank 0's block first; the others below
        } else
            HIPCHK(hipMemcpyAsync(hflags, flags, sizeof(int) * (size_t)enq * GNN_FLAG_WORDS, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::vector<int> others;
        if (sharded && l->world > 1) {
            others.resize(flag_words * (size_t)(l->world - 1));
            HIPCHK(hipMemcpy(others.data(), flags_all + flag_words, sizeof(int) * others.size(), hipMemcpyDeviceToHost));
        }
        for (int i = 0; i < enq && *k < 0; ++i) {      // gates 0 .. enq - 1 are known; gate enq belongs to the next chunk's first body
            int any = 0;
            for (int w = 0; w < GNN_FLAG_WORDS; w += GNN_FLAG_STRIDE) any |= hflags[(size_t)i * GNN_FLAG_WORDS + w];
            for (int p = 1; sharded && p < l->world; ++p)
                for (int w = 0; w < GNN_FLAG_WORDS; w += GNN_FLAG_STRIDE) any |= others[(size_t)(p - 1) * flag_words + (size_t)i * GNN_FLAG_WORDS + w];
            if (!any) *k = i;
        }
        return GNN_OK;
    }

    // The bodies, one launch per kernel and body.  Gate i = condition(state_i, state_{i-1}) decides whether body i runs; it is evaluated by
    // the body's own first kernel.  The bodies are enqueued TRAIN_CHUNK at a time without waiting for their gates; the host then reads the
    // gates of the chunk in one synchronisation, and the bodies enqueued from a closed gate on (at most TRAIN_CHUNK of them) are dropped:
    // their results are never read.  *k: the executed bodies; cx->caches holds theirs, states[*k] the final state.
    int bodies_by_launch(int *k_out)
    {
        const int max_iter = l->max_iter;
        int enq = 0, k = -1, rc;
        if ((!sharded && N == 0) || max_iter == 0) k = 0;  // no node can raise a gate / no body allowed (a rank without rows still follows the others)
        if (sharded && (rc = cx->buf.get(&flags_all, flag_words * (size_t)l->world))) return rc;
        while (k < 0) {
            // the first look at the gates comes behind as many bodies as the loop's last training forward ran, plus one (a batch's iteration
            // count moves slowly from epoch to epoch: k = 11 is then one synchronisation and one dropped body instead of three and four)
            int chunk = enq == 0 && l->train.k_hint >= TRAIN_CHUNK ? l->train.k_hint + 1 : TRAIN_CHUNK;
#ifdef GNN_DIAG
            static const bool hint_off = getenv("GNN_TRAIN_K_HINT") && atoi(getenv("GNN_TRAIN_K_HINT")) == 0;
            if (hint_off) chunk = TRAIN_CHUNK;
#endif
            for (const int target = std::min(max_iter, enq + chunk); enq < target; ++enq)
                if ((rc = enqueue_body(enq))) return rc;
            if ((rc = read_gates(enq, &k))) return rc;
            if (k < 0 && enq == max_iter) k = max_iter;
        }
        cx->caches.resize((size_t)k);          // (recomputing step: k empty entries, rebuilt one at a time by train_backward)
        *k_out = k;
        return GNN_OK;
    }

    // The bodies in ONE persistent launch (gnn_train_small.hip), which stops at the first closed gate: the caches of all max_iter bodies are
    // one block, the host reads k and the status word in one synchronisation and keeps the first k caches.  *gave_up: a barrier spin of the
    // kernel ran out (the grid was not resident at once?) - nothing of this forward is valid, the caller repeats it launch by launch.
    int bodies_persistent(const SmallTrainForm &pf, int *k_out, bool *gave_up)
    {
        gnn_graph *g = l->g;
        Net &ns = cx->ns;
        const gnn_mlp *m = ns.m;
        const int Ds = l->Ds, L = m->n_layers, F = m->dims[L];
        float *cache = nullptr;
        int rc;
        if ((rc = cx->buf.get(&cache, pf.body_floats * (size_t)l->max_iter))) return rc;
        hflags[0] = 0; hflags[1] = 0;                  // [k, status]: the status word is cleared HERE, the kernel only ever sets it
        const InputBuild build{Ds, Ds + l->NLc, cx->tmpl, cx->states[0], cx->states[0], nullptr, g->sh->indptr, g->sh->adj_src, g->sh->adj_w, l->thr, nullptr};
        if ((rc = small_train_launch(st, ns, pf, build, l->max_iter, cache, flags, hflags))) return rc;
        HIPCHK(hipStreamSynchronize(st));
        if (hflags[1] != 0) { *gave_up = true; return GNN_OK; }
        const int k = hflags[0];
        if (k < 0 || k > l->max_iter) return gnn_fail(GNN_ERR_STATE, "internal: the persistent training forward reports %d bodies", k);
        for (int b = 0; b < k; ++b) {
            float *blk = cache + (size_t)b * pf.body_floats;
            cx->caches.emplace_back();
            NetCache &c = cx->caches.back();
            c.n = N;
            c.hin.assign(L, nullptr); c.a.assign(L, nullptr); c.keep.assign(L + 1, nullptr);
            for (int q = 0; q < L; ++q) { c.a[q] = blk + pf.off_a[q]; c.hin[q] = q == 0 ? blk : c.a[q - 1]; }
            if (m->has_bn) { c.xhat = blk + pf.off_xhat; c.stats = ns.stats_all + (size_t)b * 2 * F; }
            cx->states.push_back(m->has_bn ? blk + pf.off_y : c.a[L - 1]);
        }
        if (m->has_bn) ns.calls = k;
        cx->persistent = true; cx->workgroups = pf.grid; cx->barriers = pf.barriers;
        *k_out = k;
        return GNN_OK;
    }

    // net_output on the masked rows of `state`
    int output(const float *state)
    {
        gnn_graph *g = l->g;
        const int Ds = l->Ds, wf = l->ou->dims[0];
        float *feats = nullptr;
        int rc;
        if ((rc = cx->buf.get(&feats, (size_t)M * wf))) return rc;
        if (l->edge_mode) {
            if ((rc = gnn_launch_feats_edge(st, l, state, feats))) return rc;
        } else if (M) {
            hipLaunchKernelGGL(k_gather_feats, cdiv(M * wf, 256), 256, 0, st, M, g->sh->masked_rows, state + own_off * Ds, Ds, g->nodes + (size_t)g->own_off * g->NL, g->NL, l->NLc, feats);
            HIPCHK(hipGetLastError());
        }
        return net_forward(st, cx->buf, cx->no_, feats, nullptr, d_masks_o, MaskStream{seed, 1, 0, cx->M_before}, cx->co, &cx->out_nodes, comm, nullptr);
    }

    // publish the training-mode state / outputs as the loop's result: gnn_loop_get_state / get_output / readout and
    // gnn_graph_update_labels (LGNN stacking) read them exactly like an inference run's
    int publish(const float *state, float *out_nodes_host, bool final_sync)
    {
        gnn_graph *g = l->g;
        const int Ds = l->Ds, T = l->T;
        l->init_in_place = false;                        // published as "k == 0 bodies" with the state in state[0] (gnn_engine.h, gnn_state_after)
        if (sharded) {                                  // the whole replica, as after an inference Loop (k == 0 with D == 0: the label rows there are)
            const size_t replica_floats = (size_t)l->N_pad * Ds, have = state == g->nodes ? (size_t)g->nodes_rows * Ds : replica_floats;
            HIPCHK(hipMemcpyAsync(l->state[0], state, sizeof(float) * std::min(have, replica_floats), hipMemcpyDeviceToDevice, st));
        }
        else if (N) HIPCHK(hipMemcpyAsync(l->state[0], state, sizeof(float) * (size_t)N * Ds, hipMemcpyDeviceToDevice, st));
        // (l->out changes here without loop_prepare: a graph readout that an earlier inference run folded into its persistent launch -
        // ng_host - must not be handed out for these outputs)
        l->ng_inlaunch = false;
        ++l->out_runs;
        if (M) HIPCHK(hipMemcpyAsync(l->out, cx->out_nodes, sizeof(float) * (size_t)M * T, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemsetAsync(l->kfinal_dev, 0, sizeof(int), st));
        if (out_nodes_host && M) HIPCHK(hipMemcpyAsync(out_nodes_host, cx->out_nodes, sizeof(float) * (size_t)M * T, hipMemcpyDeviceToHost, st));
        if (final_sync) HIPCHK(hipStreamSynchronize(st));
        l->kfinal = 0;
        *l->kfinal_host = 0;
        l->ran = true;
        return GNN_OK;
    }
};

// The loop's part of the decision for the persistent training forward (the net's, the rows' and the byte cap's part: small_train_form):
// one GPU, allowed (gnn_loop_set_train_persistent) and never timed out on this loop, the conditions gnn_loop_decide_form applies to the
// persistent inference launch (not disabled, not profiling), the whole grid resident at once.  f->ok says whether it is taken.
static int train_persistent_decide(gnn_loop *l, const Net &ns, SmallTrainForm *f)
{
    *f = SmallTrainForm{};
    if (l->world != 1 || !l->train.persistent.allowed || l->train.persistent.failed || l->small_disabled || l->profiling) return GNN_OK;
    SmallTrainForm t = small_train_form(ns, l->max_iter);
    if (!t.ok) return GNN_OK;
    bool resident = false;
    const int rc = small_train_resident(l->device, t, &resident);
    if (rc) return rc;
    if (resident) *f = t;
    return GNN_OK;
}

// One training-mode Loop from a fresh arena.  allow_persistent: the bodies may run in the persistent launch where it is eligible;
// *gave_up: that launch timed out at a barrier - nothing was published, the caller repeats the forward without it.  Everything else -
// an ineligible loop, a repeat after a time-out - runs the bodies launch by launch (Forward::bodies_by_launch).
// final_sync: wait for the published state / outputs (and out_nodes_host) before returning.
static int train_forward_once(gnn_loop *l, const int32_t *src_indptr, const int32_t *src_dst, const float *src_w, const float *dropout_state,
                              const float *dropout_output, const uint8_t *masks_state, const uint8_t *masks_output, uint64_t seed,
                              const float *bn_state, const float *bn_output, float *k_out, float *out_nodes_host, bool final_sync,
                              bool allow_persistent, bool *gave_up)
{
    ARGCHK(l && dropout_state && dropout_output && k_out, "bad arguments");
    // Sharded FORWARD (round 3): node-range shards with full-replica numbering, one process per rank - the state rows are all-gathered
    // after every body, the BatchNormalization statistics and the iteration gates are those of all ranks.  gnn_loop_train_backward
    // continues on the shards when the by-source adjacency of the owned rows was given here.
    const bool sharded = l->world > 1;
    if (sharded) {
        ARGCHK(l->comm && !l->comm->grp, "training forward on shards: one process per rank (an RCCL communicator), not a loopback group");
        ARGCHK(!l->g->halo_world && !l->slice_mode && !l->edge_mode, "training forward on shards: node-range shards with full-replica numbering, node- or graph-based");
    }
    ARGCHK(l->edge_mode == l->edge_expected, "edge-based net_output: call gnn_loop_set_edge_readout first");
    if (!l->have_state0 && l->D) return gnn_fail(GNN_ERR_STATE, "state_vect_dim > 0: call gnn_loop_set_state0 first");
    gnn_graph *g = l->g;
    const int64_t N = g->n_rows, M = l->edge_mode ? l->n_edge_masked : g->n_masked;
    int rc;
    HIPCHK(hipSetDevice(l->device));
    hipStream_t st = l->stream;
    // Gradient mode 1 (the gradient at the fixed point, include/gnn_hip.h): the bodies are those of the INFERENCE Loop, with the loop's own
    // arithmetic and launch form; what follows records one training-mode body at the state it converged to.
    const bool fixed_point = l->train.adjoint.mode != 0;
    // Recomputation of the bodies' activations (gnn_loop_set_train_recompute): the bodies keep their output state alone and run launch by
    // launch; gradient modes 1 and 2 record one body anyway and ignore it
    const bool recompute = l->train.recompute != 0 && !fixed_point;
    if (recompute && sharded) return gnn_fail(GNN_ERR_UNSUPPORTED, "recomputation of the bodies' activations is single-GPU");
    float k_inference = 0.0f;
    if (fixed_point) {
        if (sharded) return gnn_fail(GNN_ERR_UNSUPPORTED, "the fixed-point gradient is single-GPU");
        const int why = adjoint_refusal(l->st, dropout_state, l->train.adjoint.flags);
        if (why) return gnn_fail(GNN_ERR_UNSUPPORTED, "the fixed-point gradient needs a net_state whose training-mode forward is the inference forward: this one has %s",
                                 why == 1 ? "a BatchNormalization" : "a Dropout rate != 0");
        if ((rc = gnn_loop_run(l, 0, &k_inference))) return rc;
    }
    if (!l->graph_ready_seen) {      // creation-time fills of a derived graph's labels come before their first read (gnn_graph_wait_ready)
        if ((rc = gnn_graph_wait_ready(g, st))) return rc;
        l->graph_ready_seen = true;
    }
    gnn_train_ctx_free(l);
    l->train.power = {};              // (the vector of a contraction estimate lived in the scratch that is handed out again from here on)
    gnn_train_arena *arena = loop_arena(l);
    arena->reset();
    gnn_train_ctx *cx = l->train_ctx = new gnn_train_ctx();
    cx->buf.arena = arena;
    cx->N = N; cx->M = M;
    cx->recompute = recompute;
    Buf &buf = cx->buf;
    Forward f{l, cx, st, sharded, sharded ? l->comm : nullptr, N, M, sharded ? (size_t)l->own_off : 0, dropout_state, seed};
    // everything the step needs zeroed, in one block and one memset: gradients and BatchNormalization statistics of both nets, the
    // iteration gates, the template of the concat
    // (mode 1 records ONE body whatever max_iter is: one gate block - never read - and one call of net_state)
    const int max_iter = fixed_point ? 1 : l->max_iter;
    f.flag_words = (size_t)(max_iter + 1) * GNN_FLAG_WORDS;
    const size_t z_s = net_zero_floats(l->st, max_iter), z_o = net_zero_floats(l->ou, 1), z_f = (f.flag_words + 63) & ~(size_t)63;
    const size_t z_total = z_s + z_o + z_f + (size_t)N * l->in_s;
    float *zero_mem = nullptr;
    if ((rc = buf.get(&zero_mem, z_total))) return rc;
    HIPCHK(hipMemsetAsync(zero_mem, 0, sizeof(float) * std::max<size_t>(1, z_total), st));
    if ((rc = net_setup(st, buf, cx->ns, l->st, dropout_state, bn_state, max_iter, zero_mem, N, true)) ||
        (rc = net_setup(st, buf, cx->no_, l->ou, dropout_output, bn_output, 1, zero_mem + z_s, M, false))) return rc;
    // (gradient modes 1 and 2 reach this line with a BatchNormalization in net_state only under GNN_ADJOINT_FROZEN_BN: adjoint_refusal above)
    if (fixed_point && l->st->has_bn && (rc = net_freeze_bn(st, buf, cx->ns))) return rc;
    f.flags = reinterpret_cast<int *>(zero_mem + z_s + z_o);
    cx->tmpl = zero_mem + z_s + z_o + z_f;
    cx->seed = seed;
    if ((rc = f.by_source(src_indptr, src_dst, src_w)) || (rc = f.concat_template()) ||
        (rc = f.upload_masks(dropout_output, masks_state, masks_output))) return rc;

    // ---- while condition: state <- net_state(concat), training mode (GNN.py:271 with training=True) ----------------------
    // small batches: every body in ONE persistent launch (decided once per forward, here beside net_setup); else launch by launch
    SmallTrainForm pf;
    if (allow_persistent && !sharded && !fixed_point && !recompute && (rc = train_persistent_decide(l, cx->ns, &pf))) return rc;
    f.hflags = static_cast<int *>(arena->host.get(std::max<size_t>(sizeof(int) * f.flag_words, 4096)));
    if (!f.hflags) return gnn_fail(GNN_ERR_HIP, "hipHostMalloc failed");
    if (sharded && l->D) {
        float *rep0 = nullptr;
        if ((rc = train_replicate(l, buf, st, l->state_init, &rep0))) return rc;
        cx->states.push_back(rep0);
    } else
        cx->states.push_back(const_cast<float *>(l->D ? l->state_init : g->nodes));      // (D == 0: the node labels, a replica already)
    int k = 0;
    if (fixed_point) {
        // p = the state after the k bodies of the inference Loop, copied out of the loop's tables (publish() below rewrites them); the recorded
        // body reads p, its gate block and its output state are not used
        float *p = nullptr;
        if ((rc = buf.get(&p, (size_t)std::max<int64_t>(N, 1) * l->Ds))) return rc;
        k = (int)k_inference;
        if (N) HIPCHK(hipMemcpyAsync(p, gnn_loop_state_after(l, l->kfinal, 0), sizeof(float) * (size_t)N * l->Ds, hipMemcpyDeviceToDevice, st));
        cx->states[0] = p;
        if ((rc = f.enqueue_body(0))) return rc;
        cx->fixed_point = true;
        cx->state = p;
    } else {
        if (pf.ok) {
            if ((rc = f.bodies_persistent(pf, &k, gave_up))) return rc;
            if (*gave_up) return GNN_OK;
        } else if ((rc = f.bodies_by_launch(&k)))
            return rc;
        cx->state = cx->states[(size_t)k];
        l->train.k_hint = k;
    }
    if ((rc = f.output(cx->state))) return rc;
    cx->k = k;
    if ((rc = f.publish(cx->state, out_nodes_host, final_sync))) return rc;
    *k_out = (float)k;
    return GNN_OK;
}

// Training-mode Loop: with the persistent forward where it is eligible; after a time-out of its barrier the arena is reset and the whole
// forward repeated with one launch per kernel and body (fresh launches in this process), the event is counted and the loop keeps to
// per-body launches until gnn_loop_set_train_persistent is called again.
static int train_forward(gnn_loop *l, const int32_t *src_indptr, const int32_t *src_dst, const float *src_w, const float *dropout_state,
                         const float *dropout_output, const uint8_t *masks_state, const uint8_t *masks_output, uint64_t seed,
                         const float *bn_state, const float *bn_output, float *k_out, float *out_nodes_host, bool final_sync)
{
    bool gave_up = false;
    const int rc = train_forward_once(l, src_indptr, src_dst, src_w, dropout_state, dropout_output, masks_state, masks_output, seed, bn_state, bn_output, k_out,
                                      out_nodes_host, final_sync, true, &gave_up);
    if (rc || !gave_up) return rc;
    ++l->train.persistent.timeouts;
    l->train.persistent.failed = true;
    return train_forward_once(l, src_indptr, src_dst, src_w, dropout_state, dropout_output, masks_state, masks_output, seed, bn_state, bn_output, k_out,
                              out_nodes_host, final_sync, false, &gave_up);
}

// allow / forbid the persistent training forward; *used: whether a forward WITHOUT Dropout in net_state would take it on this loop now
extern "C" int gnn_loop_set_train_persistent(gnn_loop *l, int enable, int *used)
{
    ARGCHK(l, "loop is NULL");
    l->train.persistent.allowed = enable != 0;
    l->train.persistent.failed = false;
    if (used) {
        *used = 0;
        if (l->world == 1 && l->g->n_rows >= 1) {
            HIPCHK(hipSetDevice(l->device));
            Net net;
            net.m = l->st;
            net.rate.assign((size_t)l->st->n_layers + 1, 0.0f);
            net_decide_form(net, l->g->n_rows, true);
            SmallTrainForm f;
            const int rc = train_persistent_decide(l, net, &f);
            if (rc) return rc;
            *used = f.ok ? 1 : 0;
        }
    }
    return GNN_OK;
}

// out[4]: the last training forward ran persistently (0 / 1), its workgroups, its grid barriers per body; time-out fall-backs of this loop so far
extern "C" int gnn_loop_train_info(const gnn_loop *l, int *out)
{
    ARGCHK(l && out, "bad arguments");
    const gnn_train_ctx *cx = l->train_ctx;
    out[0] = cx && cx->persistent ? 1 : 0;
    out[1] = cx ? cx->workgroups : 0;
    out[2] = cx ? cx->barriers : 0;
    out[3] = l->train.persistent.timeouts;
    return GNN_OK;
}

// Recomputation of the bodies' activations in the unrolled step (include/gnn_hip.h).  enable: 0 off, 1 on, 2 on with the caching kernels in
// the first pass (A/B runs); *used: whether a training forward of this loop would take the mode now
extern "C" int gnn_loop_set_train_recompute(gnn_loop *l, int enable, int *used)
{
    ARGCHK(l, "loop is NULL");
    if (enable != 0 && l->world > 1)
        return gnn_fail(GNN_ERR_UNSUPPORTED, "recomputation of the bodies' activations is single-GPU, like the training step: this loop is rank %d of %d", l->rank, l->world);
    l->train.recompute = enable == 0 ? 0 : (enable == 2 ? 2 : 1);
    if (used) *used = enable != 0 && l->train.adjoint.mode == 0 ? 1 : 0;
    return GNN_OK;
}

// out[3]: the last training forward ran state-only; bodies replayed by the last backward pass; 1 when the first pass launched the cache-less chain
extern "C" int gnn_loop_train_recompute_info(const gnn_loop *l, int *out)
{
    ARGCHK(l && out, "bad arguments");
    const gnn_train_ctx *cx = l->train_ctx;
    out[0] = cx && cx->recompute ? 1 : 0;
    out[1] = cx ? cx->replayed : 0;
    out[2] = cx ? cx->cacheless_chain : 0;
    return GNN_OK;
}

extern "C" int gnn_loop_train_forward(gnn_loop *l, const int32_t *src_indptr, const int32_t *src_dst, const float *src_w,
                                      const float *dropout_state, const float *dropout_output, const uint8_t *masks_state,
                                      const uint8_t *masks_output, uint64_t seed, const float *bn_state, const float *bn_output,
                                      float *k_out, float *out_nodes_host)
{
    return train_forward(l, src_indptr, src_dst, src_w, dropout_state, dropout_output, masks_state, masks_output, seed, bn_state, bn_output, k_out,
                         out_nodes_host, true);
}

// Gradient mode 1 behind net_output's backward pass: g = d loss / d p (d_state, left intact) -> z_final by the adjoint iteration
// z_0 = g, z_{t+1} = g + J^T z_t on the ONE recorded body (cx->caches[0]), then that body's weight gradients for the incoming gradient z_final.
// An iteration = net_backward without weight gradients + the gather of gnn_train_adjoint.hip, which writes z_{t+1} twice (z buffer (t + 1) & 1
// and `work`, which the next net_backward consumes in place) and raises gate t when a node moved.  The iterations are enqueued TRAIN_CHUNK at
// a time on scratch that every iteration reuses; the host then reads the chunk's gates in one wait.  Iteration t finds gate t - 1 of its
// chunk on the device: behind a closed gate it hands z on unchanged and raises nothing, so the first closed gate gives the count and the
// last buffer written holds z of that count - nothing is recomputed.
// *u_out = d concat [N, in_s] of the weight-gradient pass: its label columns are (d body / d labels)^T z_final (GNN_ADJOINT_LABEL_GRADIENTS).
static int adjoint_backward(gnn_loop *l, gnn_train_ctx *cx, hipStream_t st, float *g_state, float **u_out)
{
    gnn_train_arena *arena = cx->buf.arena;
    Buf &buf = cx->buf;
    Net &ns = cx->ns;
    auto &adj = l->train.adjoint;
    const int64_t N = cx->N;
    const int Ds = l->Ds;
    const int t_max = adj.max_iter > 0 ? adj.max_iter : l->max_iter;
    const float thr = adj.thr >= 0.0f ? adj.thr : l->thr;
    const size_t zf = (size_t)std::max<int64_t>(N, 1) * Ds;
    int rc;
    // the first look at the gates comes behind as many iterations as the loop's last step ran, plus one (as k_hint for the forward's bodies:
    // a batch's count moves slowly from step to step, and every look is a wait for the device)
    const int first_chunk = adj.iterations >= TRAIN_CHUNK ? std::min(t_max, adj.iterations + 1) : TRAIN_CHUNK;
    const size_t gate_blocks = (size_t)std::max(first_chunk, (int)TRAIN_CHUNK);
    adj.iterations = 0; adj.converged = 1;
    adj.gather = adjoint_rows16(Ds) ? ADJ_GATHER_ROWS : ADJ_GATHER_GENERIC;       // (without an iteration; else what the launches report)
    // narrow nets: one launch per iteration (k_adjoint_narrow), decided once per step; mode 2 keeps to the per-kernel chain
    // (the Anderson solver keeps to the per-kernel chain as well: its gather carries the window's bookkeeping)
    const bool anderson = adj.solver == 1;
    const bool narrow = adj.mode == 1 && !anderson && adjoint_narrow_why(ns.m, N) == 0;
    adj.restarts = 0;
    if (cx->caches.size() != 1) return gnn_fail(GNN_ERR_STATE, "internal: the fixed-point gradient needs one recorded body, not %zu", cx->caches.size());
    float *zb[2] = {nullptr, nullptr}, *work = nullptr;
    int *gates = nullptr;
    if ((rc = buf.get(&zb[0], zf)) || (rc = buf.get(&zb[1], zf)) || (rc = buf.get(&work, zf)) || (rc = buf.get(&gates, gate_blocks * GNN_FLAG_WORDS))) return rc;
    // (not arena->host: gnn_loop_train_step has this step's loss partials on their way into it)
    int *hgates = static_cast<int *>(arena->gates.get(sizeof(int) * (gate_blocks * GNN_FLAG_WORDS + 16)));      // (+ the Anderson solver's restart count)
    if (!hgates) return gnn_fail(GNN_ERR_HIP, "hipHostMalloc failed");
    if (N) HIPCHK(hipMemcpyAsync(work, g_state, sizeof(float) * (size_t)N * Ds, hipMemcpyDeviceToDevice, st));
    if (N > 0 && t_max > 0) adj.converged = 0;
    float *ub[2] = {nullptr, nullptr};             // narrow form: u of launch L, [N, 2 Ds] = [own-state columns | aggregated-state columns] of d concat
    if (narrow && ((rc = buf.get(&ub[0], 2 * zf)) || (rc = buf.get(&ub[1], 2 * zf)))) return rc;
    // Anderson solver: G and f of the iteration before, the two rings of `window` difference rows (2 window + 2 buffers of [N, Ds]), the blocks'
    // partial dots and the window's device state
    AndersonJob aj{};
    if (anderson) {
        double *part = nullptr, *state_mem = nullptr;
        aj.window = adj.window; aj.stride = zf;
        if ((rc = buf.get(&aj.G, zf)) || (rc = buf.get(&aj.f, zf)) || (rc = buf.get(&aj.dF, zf * aj.window)) || (rc = buf.get(&aj.dG, zf * aj.window)) ||
            (rc = buf.get(&part, (size_t)ANDERSON_PARTS * std::max(anderson_blocks(N), 1u))) || (rc = buf.get(&state_mem, (sizeof(AndersonState) + 7) / 8))) return rc;
        aj.part = part; aj.state = reinterpret_cast<AndersonState *>(state_mem);
        HIPCHK(hipMemsetAsync(aj.state, 0, sizeof(AndersonState), st));
    }
    const gnn_train_arena::Mark mark = arena->mark();
    for (int t = 0; N > 0 && t < t_max && !adj.converged;) {
        const int t0 = t, t1 = std::min(t_max, t0 + (t0 == 0 ? first_chunk : (int)TRAIN_CHUNK));
        HIPCHK(hipMemsetAsync(gates, 0, sizeof(int) * (size_t)(t1 - t0) * GNN_FLAG_WORDS, st));
        auto gate_of = [&](int it) { return it >= t0 ? gates + (size_t)(it - t0) * GNN_FLAG_WORDS : (int *)nullptr; };     // gate of iteration `it` (z_{it+1} against z_it) of this chunk
        auto z_of = [&](int it) { return it == 0 ? g_state : zb[it & 1]; };
        if (narrow) {
            // Launch L forms z_L from launch L - 1's u (gate L - 1) and leaves u_L; the chunk's first launch finds z_{t0} formed (g, or the gather
            // that closed the chunk before), and one gather of the ordinary kind closes the chunk: z_{t1}, gate t1 - 1, `work`.
            const gnn_mlp *m = ns.m;
            const NetCache &c = cx->caches[0];
            for (; t < t1; ++t) {
                AdjNarrow p{};
                p.n = N; p.Ds = Ds; p.c_aggs = Ds + l->NLc; p.L = m->n_layers; p.gather = t > t0;
                for (int q = 0; q <= m->n_layers; ++q) p.dims[q] = m->dims[q];
                for (int q = 0; q < m->n_layers; ++q) { p.acts[q] = m->acts[q]; p.WT[q] = ns.WT[q]; p.a[q] = c.a[q]; }
                p.colscale = ns.frozen ? ns.frozen + Ds : nullptr;
                p.sip = cx->d_sip; p.sdst = cx->d_sdst; p.sw = cx->d_sw;
                p.g = g_state; p.z_prev = t > 0 ? z_of(t - 1) : nullptr; p.u_prev = ub[(t + 1) & 1]; p.z_cur = z_of(t); p.u_out = ub[t & 1];
                p.thr = thr; p.gate_prev = gate_of(t - 2); p.gate = gate_of(t - 1);
                if ((rc = launch_adjoint_narrow(st, p))) return rc;
            }
            StateGradJob job{N, Ds, 2 * Ds, Ds, cx->d_sip, cx->d_sdst, cx->d_sw, nullptr};
            job.g = g_state; job.z_prev = z_of(t1 - 1); job.z_next = zb[t1 & 1]; job.work = work; job.thr = thr;
            job.gate_prev = gate_of(t1 - 2); job.gate = gate_of(t1 - 1);
            if ((rc = launch_adjoint_gather(st, job, ub[(t1 - 1) & 1], false, nullptr))) return rc;
            adj.gather = ADJ_GATHER_NARROW;
        }
        for (; t < t1; ++t) {
            arena->rewind(mark);
            StateGradJob job{N, Ds, l->in_s, Ds + l->NLc, cx->d_sip, cx->d_sdst, cx->d_sw, nullptr};
            job.g = g_state; job.z_prev = t == 0 ? g_state : zb[t & 1]; job.z_next = zb[(t + 1) & 1]; job.work = work; job.thr = thr;
            job.gate_prev = t > t0 ? gates + (size_t)(t - t0 - 1) * GNN_FLAG_WORDS : nullptr;
            job.gate = gates + (size_t)(t - t0) * GNN_FLAG_WORDS;
            job.form_out = &adj.gather;
            if (anderson) { aj.first = t == 0; job.anderson = &aj; }
            float *u = nullptr;
            if ((rc = net_backward(st, buf, ns, cx->caches[0], work, &u, &job, nullptr, 0, false))) return rc;
            if (anderson && t > 0 && (rc = launch_anderson_solve_mix(st, job))) return rc;
        }
        HIPCHK(hipMemcpyAsync(hgates, gates, sizeof(int) * (size_t)(t1 - t0) * GNN_FLAG_WORDS, hipMemcpyDeviceToHost, st));
        if (anderson) HIPCHK(hipMemcpyAsync(hgates + gate_blocks * GNN_FLAG_WORDS, &aj.state->restarts, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (anderson) adj.restarts = hgates[gate_blocks * GNN_FLAG_WORDS];
        adj.iterations = t1;
        for (int i = 0; i < t1 - t0; ++i) {
            int any = 0;
            for (int w = 0; w < GNN_FLAG_WORDS; w += GNN_FLAG_STRIDE) any |= hgates[(size_t)i * GNN_FLAG_WORDS + w];
            if (!any) { adj.iterations = t0 + i + 1; adj.converged = 1; break; }
        }
    }
    arena->rewind(mark);
    cx->adjoint_z = adj.iterations == 0 ? g_state : zb[adj.iterations & 1];
    // `work` holds z_final (the last gather wrote it beside its z buffer; without an iteration it is the copy of g)
    return net_backward(st, buf, ns, cx->caches[0], work, u_out, nullptr, nullptr, 0, true);
}

// Contraction estimate at the fixed point (include/gnn_hip.h): power iteration on J^T of the ONE recorded body - the J of adjoint_backward, always
// with BatchNormalization on its moving statistics.  Forward as gradient mode 1 takes it (the inference Loop to p, one body recorded at p) without
// net_output; then w_0 (the caller's, or normal draws keyed on seed) with its norm, and per iteration net_backward without weight gradients on the
// per-kernel chain with the power gather (gnn_train_adjoint.hip: w_t = J^T w_{t-1} / n_{t-1}, one partial squared norm per block) and
// k_power_finalize (n_t into growth, 1 / n_t for the next gather; 0 stops the iteration on the device).  Scratch is rewound per iteration as the
// adjoint's; the host waits once, for growth.  The loop's gradient mode is neither read nor written; the context of a pending training forward ends.
extern "C" int gnn_loop_contraction_estimate(gnn_loop *l, const int32_t *src_indptr, const int32_t *src_dst, const float *src_w, const float *dropout_state,
                                             const float *bn_state, int iterations, const float *v0, uint64_t seed, float *growth, int *done, float *k_out)
{
    ARGCHK(l && dropout_state && growth && done && k_out, "bad arguments");
    ARGCHK(iterations >= 1 && iterations <= 1024, "iterations must lie in [1, 1024] (got %d)", iterations);
    if (l->world > 1) return gnn_fail(GNN_ERR_UNSUPPORTED, "the contraction estimate is single-GPU (this loop is rank %d of %d)", l->rank, l->world);
    if (l->D == 0) return gnn_fail(GNN_ERR_UNSUPPORTED, "the contraction estimate needs state_vect_dim > 0 (with 0 the loop iterates on the node labels themselves)");
    if (adjoint_refusal(l->st, dropout_state, GNN_ADJOINT_FROZEN_BN))
        return gnn_fail(GNN_ERR_UNSUPPORTED, "the contraction estimate needs a net_state without Dropout (the map the inference Loop iterates): this one has a Dropout rate != 0");
    ARGCHK(l->edge_mode == l->edge_expected, "edge-based net_output: call gnn_loop_set_edge_readout first");
    if (!l->have_state0) return gnn_fail(GNN_ERR_STATE, "state_vect_dim > 0: call gnn_loop_set_state0 first");
    gnn_graph *g = l->g;
    const int64_t N = g->n_rows;
    const int Ds = l->Ds;
    int rc;
    HIPCHK(hipSetDevice(l->device));
    hipStream_t st = l->stream;
    float k_inference = 0.0f;
    if ((rc = gnn_loop_run(l, 0, &k_inference))) return rc;
    if (!l->graph_ready_seen) {
        if ((rc = gnn_graph_wait_ready(g, st))) return rc;
        l->graph_ready_seen = true;
    }
    gnn_train_ctx_free(l);
    l->train.power = {};
    gnn_train_arena *arena = loop_arena(l);
    arena->reset();
    // (the context lives for this call alone: it holds no net_output, so nothing behind a training forward may find it)
    struct Scoped { gnn_loop *l; ~Scoped() { gnn_train_ctx_free(l); } } scoped{l};
    gnn_train_ctx *cx = l->train_ctx = new gnn_train_ctx();
    cx->buf.arena = arena;
    cx->N = N; cx->M = 0;
    cx->backward_done = true; cx->applied = true;
    Buf &buf = cx->buf;
    Forward f{l, cx, st, false, nullptr, N, 0, 0, dropout_state, seed};
    f.flag_words = (size_t)2 * GNN_FLAG_WORDS;
    const size_t z_s = net_zero_floats(l->st, 1), z_f = (f.flag_words + 63) & ~(size_t)63, z_total = z_s + z_f + (size_t)N * l->in_s;
    float *zero_mem = nullptr;
    if ((rc = buf.get(&zero_mem, z_total))) return rc;
    HIPCHK(hipMemsetAsync(zero_mem, 0, sizeof(float) * std::max<size_t>(1, z_total), st));
    if ((rc = net_setup(st, buf, cx->ns, l->st, dropout_state, bn_state, 1, zero_mem, N, true))) return rc;
    if (l->st->has_bn && (rc = net_freeze_bn(st, buf, cx->ns))) return rc;
    f.flags = reinterpret_cast<int *>(zero_mem + z_s);
    cx->tmpl = zero_mem + z_s + z_f;
    cx->seed = seed;
    if ((rc = f.by_source(src_indptr, src_dst, src_w)) || (rc = f.concat_template())) return rc;
    float *p = nullptr;
    if ((rc = buf.get(&p, (size_t)std::max<int64_t>(N, 1) * Ds))) return rc;
    if (N) HIPCHK(hipMemcpyAsync(p, gnn_loop_state_after(l, l->kfinal, 0), sizeof(float) * (size_t)N * Ds, hipMemcpyDeviceToDevice, st));
    cx->states.push_back(p);
    if ((rc = f.enqueue_body(0))) return rc;
    cx->fixed_point = true;
    cx->state = p;
    cx->k = (int)k_inference;

    const size_t zf = (size_t)std::max<int64_t>(N, 1) * Ds;
    const unsigned blocks = power_blocks(N);
    float *w = nullptr, *work = nullptr, *part = nullptr, *norms = nullptr, *inv = nullptr;        // norms [iterations + 1]: n_0, then growth
    if ((rc = buf.get(&w, zf)) || (rc = buf.get(&work, zf)) || (rc = buf.get(&part, (size_t)std::max(blocks, 1u))) || (rc = buf.get(&norms, (size_t)iterations + 1)) ||
        (rc = buf.get(&inv, (size_t)1))) return rc;
    float *hnorms = static_cast<float *>(arena->host.get(std::max<size_t>(sizeof(float) * ((size_t)iterations + 1), 4096)));
    if (!hnorms) return gnn_fail(GNN_ERR_HIP, "hipHostMalloc failed");
    for (int t = 0; t < iterations; ++t) growth[t] = 0.0f;
    *done = 0;
    *k_out = k_inference;
    if (N == 0) { HIPCHK(hipStreamSynchronize(st)); return GNN_OK; }
    if (v0) HIPCHK(hipMemcpyAsync(w, v0, sizeof(float) * (size_t)N * Ds, hipMemcpyHostToDevice, st));
    if ((rc = launch_power_start(st, N, Ds, v0 ? 0 : 1, seed, w, work, part)) || (rc = launch_power_finalize(st, blocks, part, norms, inv))) return rc;
    const gnn_train_arena::Mark mark = arena->mark();
    for (int t = 1; t <= iterations; ++t) {
        arena->rewind(mark);
        StateGradJob job{N, Ds, l->in_s, Ds + l->NLc, cx->d_sip, cx->d_sdst, cx->d_sw, nullptr};
        job.z_next = w; job.work = work; job.pw_inv = inv; job.pw_part = part;
        float *u = nullptr;
        if ((rc = net_backward(st, buf, cx->ns, cx->caches[0], work, &u, &job, nullptr, 0, false)) ||
            (rc = launch_power_finalize(st, blocks, part, norms + t, inv))) return rc;
    }
    arena->rewind(mark);
    HIPCHK(hipMemcpyAsync(hnorms, norms, sizeof(float) * ((size_t)iterations + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // done = the first t whose n_t is 0 or not finite (its entry is kept as measured, the later ones are 0), else all of them
    int t_done = iterations;
    for (int t = 0; t <= iterations; ++t)
        if (!(hnorms[t] > 0.0f) || !std::isfinite(hnorms[t])) { t_done = t; break; }
    for (int t = 1; t <= iterations; ++t) growth[t - 1] = t <= t_done ? hnorms[t] : 0.0f;
    *done = t_done;
    l->train.power.w = w; l->train.power.rows = N;
    return GNN_OK;
}

// gnn_loop_train_backward_chained: the label gradients stay on the device.  keep_nodes / keep_arcs: compute d_nodes / d_arc_labels and leave them
// with the context; next: the loop of the layer above, whose kept label gradients carry this loop's extra state gradient (get_state) and extra
// output gradient (get_output)
struct Chain { gnn_loop *next; bool get_state, get_output, keep_nodes, keep_arcs; };

// d_out_dev: d loss / d out_nodes already on the device (gnn_loop_train_step), else d_out_host is uploaded
static int train_backward(gnn_loop *l, float *d_out_dev, const float *d_out_host, const float *d_state_extra, float *grads_state,
                          float *grads_output, float *bn_batch_state, float *bn_batch_output, float *d_nodes_host, float *d_arcs_host, bool sync,
                          const Chain *chain = nullptr)
{
    ARGCHK(l && grads_state && grads_output, "bad arguments");
    gnn_train_ctx *cx = l->train_ctx;
    if (!cx || cx->backward_done) return gnn_fail(GNN_ERR_STATE, "gnn_loop_train_forward has not been called (one backward per forward)");
    const bool keep_nodes = chain && chain->keep_nodes, keep_arcs = chain && chain->keep_arcs && l->edge_mode, keep = keep_nodes || keep_arcs;
    const gnn_train_ctx *nx = chain && chain->next && (chain->get_state || chain->get_output) ? chain->next->train_ctx : nullptr;
    int NLb = 0, ALb = 0;          // the label widths of the base graph: next's labels are [base | this loop's state? | this loop's outputs?]
    if (chain && chain->next && (chain->get_state || chain->get_output)) {
        const gnn_loop *nl = chain->next;
        ARGCHK(l->world == 1 && nl->world == 1, "a chained backward pass is single-GPU");
        ARGCHK(nl != l && nl->device == l->device, "chained backward: next must be another loop on the same device");
        if (!nx || !nx->backward_done) return gnn_fail(GNN_ERR_STATE, "chained backward: next has no finished backward pass");
        ARGCHK(nl->g->n_rows == l->g->n_rows && nl->edge_mode == l->edge_mode, "chained backward: next runs on %lld rows, this loop on %lld (or one is edge-based, the other not)",
               (long long)nl->g->n_rows, (long long)l->g->n_rows);
        const bool on_arcs = chain->get_output && l->edge_mode;
        NLb = nl->g->NL - (chain->get_state ? l->Ds : 0) - (chain->get_output && !on_arcs ? l->T : 0);
        ALb = nl->g->AL - (on_arcs ? l->T : 0);
        ARGCHK(NLb >= 0 && ALb >= 0, "chained backward: next's labels (%d node, %d arc columns) do not hold this loop's state / outputs", nl->g->NL, nl->g->AL);
        // (the sizes of the masks: the rows themselves are the caller's - gnn_graph_update_labels put this loop's outputs on ITS masked rows)
        ARGCHK(!on_arcs || (nl->g->E == l->g->E && nl->n_edge_masked == l->n_edge_masked), "chained backward: next has another number of arcs or of masked arcs");
        ARGCHK(!chain->get_output || on_arcs || nl->g->n_masked == l->g->n_masked, "chained backward: next has another number of masked rows");
        if ((chain->get_state || (chain->get_output && !on_arcs)) && !nx->kept_d_nodes)
            return gnn_fail(GNN_ERR_STATE, "chained backward: next's last backward pass kept no d_nodes (keep_label_gradients)");
        if (on_arcs && !nx->kept_d_arcs) return gnn_fail(GNN_ERR_STATE, "chained backward: next's last backward pass kept no d_arc_labels (keep_label_gradients)");
    }
    // Sharded backward (round 3; after a sharded gnn_loop_train_forward that was given the by-source adjacency of the owned rows): per
    // body the gradient of the aggregated-state columns is all-gathered like the state in the forward pass and every rank adds up, for
    // its own rows, what its out-arcs carry back; BatchNormalization's sums are those of all ranks; at the end the ranks' shares of the
    // weight gradients are all-gathered and added in rank order, so every rank returns the same, complete gradients.
    const bool sharded = l->world > 1;
    gnn_comm *comm = sharded ? l->comm : nullptr;
    if (sharded) {
        ARGCHK(cx->d_sip, "backward on shards: gnn_loop_train_forward needs the by-source adjacency of the owned rows (src_indptr / src_dst / src_w)");
        ARGCHK(!d_state_extra && !d_nodes_host && !d_arcs_host && !l->edge_mode, "backward on shards: no extra state gradient, label or arc-label gradients, node- or graph-based only");
    }
    if (cx->fixed_point && (d_nodes_host || d_arcs_host || keep)) {
        if (!(l->train.adjoint.flags & GNN_ADJOINT_LABEL_GRADIENTS))
            return gnn_fail(GNN_ERR_UNSUPPORTED, "the fixed-point gradient returns no d_nodes / d_arc_labels (the joint LGNN modes need the unrolled gradient)");
        if (!l->D)
            return gnn_fail(GNN_ERR_UNSUPPORTED, "the fixed-point gradient returns no d_nodes / d_arc_labels with state_vect_dim == 0: the unrolled d_nodes is the "
                                                 "gradient of the INITIAL state there, which a fixed point does not depend on");
    }
    gnn_graph *g = l->g;
    const int64_t N = g->n_rows, M = l->edge_mode ? l->n_edge_masked : g->n_masked;
    // (mode 1: cx->k bodies of the inference Loop led to the state; the backward pass below walks none of them)
    const int Ds = l->Ds, NLc = l->NLc, in_s = l->in_s, T = l->T, wf = l->ou->dims[0], NL = g->NL, k = cx->fixed_point ? 0 : cx->k;
    ARGCHK(M == 0 || d_out_dev || d_out_host, "d_out_nodes is NULL");
    HIPCHK(hipSetDevice(l->device));
    hipStream_t st = l->stream;
    Buf &buf = cx->buf;
    Net &ns = cx->ns, &no_ = cx->no_;
    const int c_nodes = Ds, c_aggs = Ds + NLc, c_aggn = c_aggs + Ds;
    int rc;
    float *d_out = d_out_dev, *d_feats = nullptr, *d_state = nullptr, *tmp = nullptr, *d_nodes = nullptr, *via = nullptr;
    if ((!d_out && (rc = buf.get(&d_out, (size_t)M * T))) || (rc = buf.get(&d_state, (size_t)N * Ds))) return rc;
    if (!d_out_dev && M) HIPCHK(hipMemcpyAsync(d_out, d_out_host, sizeof(float) * (size_t)M * T, hipMemcpyHostToDevice, st));
    // chained: the extra output gradient from the label gradient the layer above kept (one float32 addition per element, as the host makes it)
    if (nx && chain->get_output && M) {
        if (l->edge_mode) hipLaunchKernelGGL(k_add_masked_cols, cdiv(M * T, 256), 256, 0, st, M, T, l->edge_rows, nx->kept_d_arcs, chain->next->g->AL, ALb, d_out);
        else hipLaunchKernelGGL(k_add_masked_cols, cdiv(M * T, 256), 256, 0, st, M, T, g->sh->masked_rows, nx->kept_d_nodes, chain->next->g->NL,
                                NLb + (chain->get_state ? Ds : 0), d_out);
        HIPCHK(hipGetLastError());
    }
    if ((rc = net_backward(st, buf, no_, cx->co, d_out, &d_feats, nullptr, comm, cx->M_global))) return rc;
    const bool chained_state = nx && chain->get_state;         // ... and the extra state gradient, in the place of an uploaded d_state_extra
    const bool state_extra = d_state_extra || chained_state;
    if (chained_state) { if (N && (rc = gnn_launch_copy_cols(st, N, Ds, nx->kept_d_nodes + NLb, chain->next->g->NL, d_state, Ds, nullptr, 1))) return rc; }
    else if (d_state_extra) { if (N) HIPCHK(hipMemcpyAsync(d_state, d_state_extra, sizeof(float) * (size_t)N * Ds, hipMemcpyHostToDevice, st)); }
    else HIPCHK(hipMemsetAsync(d_state, 0, sizeof(float) * std::max<size_t>(1, (size_t)N * Ds), st));
    const bool want_nodes = d_nodes_host != nullptr || keep_nodes;
    const bool want_arcs = (d_arcs_host != nullptr || keep_arcs) && g->AL > 0;
    const int AL = g->AL, c_agga = c_aggn + NLc;
    float *d_arcs = nullptr, *d_aa = nullptr;
    if (want_arcs) {
        ARGCHK(l->edge_mode && g->sh->arc_id, "d_arc_labels: edge-based loop on a graph with gnn_graph_set_arc_order required");
        if ((rc = buf.get(&d_arcs, (size_t)g->E * AL)) || (rc = buf.get(&d_aa, (size_t)N * AL))) return rc;
        HIPCHK(hipMemsetAsync(d_arcs, 0, sizeof(float) * std::max<size_t>(1, (size_t)g->E * AL), st));
        HIPCHK(hipMemsetAsync(d_aa, 0, sizeof(float) * std::max<size_t>(1, (size_t)N * AL), st));
    }
    if (want_nodes && l->D) {
        if ((rc = buf.get(&d_nodes, (size_t)N * NL)) || (rc = buf.get(&via, (size_t)N * NL))) return rc;
        HIPCHK(hipMemsetAsync(d_nodes, 0, sizeof(float) * std::max<size_t>(1, (size_t)N * NL), st));
    }
    if (l->edge_mode) {
        if (M) {
            const int wn = Ds + NLc;
            hipLaunchKernelGGL(k_gather_edge_grad, cdiv(N * wn, 256), 256, 0, st, N, l->edge_inc_ptr, l->edge_inc, d_feats, wf, wn, Ds, NL, d_state, d_nodes);
            HIPCHK(hipGetLastError());
        }
    } else if (M) {
        if (state_extra) {          // extra + scattered rows: scatter into a zero buffer, then add
            if ((rc = buf.get(&tmp, (size_t)N * Ds))) return rc;
            HIPCHK(hipMemsetAsync(tmp, 0, sizeof(float) * (size_t)N * Ds, st));
            hipLaunchKernelGGL(k_scatter_rows, cdiv(M * Ds, 256), 256, 0, st, M, g->sh->masked_rows, d_feats, wf, Ds, tmp);
            hipLaunchKernelGGL(k_axpy1, cdiv(N * Ds, 256), 256, 0, st, N * Ds, tmp, d_state);
        } else
            hipLaunchKernelGGL(k_scatter_rows, cdiv(M * Ds, 256), 256, 0, st, M, g->sh->masked_rows, d_feats, wf, Ds, d_state);
        HIPCHK(hipGetLastError());
    }
    if (d_nodes && !l->edge_mode) {
        if (M) {
            hipLaunchKernelGGL(k_scatter_label_grad, cdiv(M * NL, 256), 256, 0, st, M, g->sh->masked_rows, d_feats, wf, Ds, NL, d_nodes);
            HIPCHK(hipGetLastError());
        }
    }
    // what one body's d concat gives the labels: the aggregated-arc columns (ArcNode^T follows at the end), the own node columns and the
    // aggregated-node columns over the adjacency by source (GNN.py:228, :263).  Mode 0: every body; modes 1 and 2: the recorded body, once
    auto label_terms = [&](const float *d_inp) -> int {
        if (want_arcs && N) {
            hipLaunchKernelGGL(k_add_cols, cdiv(N * AL, 256), 256, 0, st, N, AL, d_inp, in_s, c_agga, d_aa);
            HIPCHK(hipGetLastError());
        }
        if (want_nodes && l->D && N) {
            int rc2;
            if ((rc2 = gnn_launch_spmm(st, N, cx->d_sip, cx->d_sdst, cx->d_sw, d_inp + c_aggn, NL, in_s, via, NL, nullptr, 1))) return rc2;
            hipLaunchKernelGGL(k_nodes_grad, cdiv(N * NL, 256), 256, 0, st, N, NL, d_inp, in_s, c_nodes, via, d_nodes);
            HIPCHK(hipGetLastError());
        }
        return GNN_OK;
    };
    if (cx->fixed_point) {
        float *u = nullptr;         // d concat of the weight-gradient pass with z_final: (d body / d labels)^T z_final in its label columns
        if ((rc = adjoint_backward(l, cx, st, d_state, &u)) || (rc = label_terms(u))) return rc;
    }
    // Recomputing step: body `it` is rebuilt from states[it] on scratch that every body reuses, immediately before its backward pass - the same
    // kernels on the same inputs in the same fixed order, so the rebuilt cache holds the first pass's bits.  All that outlives a body's
    // rewind is allocated here, ahead of the mark: the two d_prev buffers used in turn, net_state's chunk partials (Net::part is remembered
    // from call to call) and the scratch gate block of the kernels that evaluate a gate in passing.
    const bool replay = cx->recompute && k > 0;
    float *d_turn[2] = {nullptr, nullptr};
    int *scratch_gate = nullptr;
    gnn_train_arena::Mark body_mark{};
    if (replay) {
        if ((rc = buf.get(&d_turn[0], (size_t)N * Ds)) || (rc = buf.get(&d_turn[1], (size_t)N * Ds)) || (rc = buf.get(&scratch_gate, (size_t)GNN_FLAG_WORDS))) return rc;
        if (N > 0 && ns.part_rows != N) {
            if ((rc = buf.get(&ns.part, (size_t)cdiv(N, rows_per_block(N)) * ns.g_total))) return rc;
            ns.part_rows = N;
        }
        body_mark = buf.arena->mark();
    }
    for (int it = k - 1; it >= 0; --it) {
        // net_backward consumes d_state (d loss / d state_{it+1}) in place; its last launch also writes d loss / d state_it into a new buffer
        float *d_inp = nullptr, *d_prev = nullptr;
        if (replay) {
            buf.arena->rewind(body_mark);
            float *y = nullptr;
            FwdMode mode;
            mode.replay_call = l->st->has_bn ? it : -1;
            if ((rc = body_forward(l, cx, st, it, scratch_gate, false, cx->caches[it], &y, nullptr, mode))) return rc;
            ++cx->replayed;
            d_prev = d_turn[(k - 1 - it) & 1];
        } else if ((rc = buf.get(&d_prev, (size_t)N * Ds))) return rc;
        if (sharded) {
            if ((rc = net_backward(st, buf, ns, cx->caches[it], d_state, &d_inp, nullptr, comm, cx->N_global))) return rc;
            // d state_it[r] = d inp[r, :Ds] + sum over the arcs r -> dst of w * d inp[dst, c_aggs:]: the aggregate columns of all ranks first
            float *dagg = nullptr, *rep = nullptr;
            if ((rc = buf.get(&dagg, (size_t)std::max<int64_t>(N, 1) * Ds))) return rc;
            if (N && (rc = gnn_launch_copy_cols(st, N, Ds, d_inp + c_aggs, in_s, dagg, Ds, nullptr, 1))) return rc;
            if ((rc = train_replicate(l, buf, st, dagg, &rep))) return rc;
            if (N) {
                if ((rc = gnn_launch_spmm(st, N, cx->d_sip, cx->d_sdst, cx->d_sw, rep, Ds, Ds, d_prev, Ds, nullptr, 1))) return rc;
                hipLaunchKernelGGL(k_add_cols, cdiv(N * Ds, 256), 256, 0, st, N, Ds, d_inp, in_s, 0, d_prev);
                HIPCHK(hipGetLastError());
            }
        } else {
            const StateGradJob job{N, Ds, in_s, c_aggs, cx->d_sip, cx->d_sdst, cx->d_sw, d_prev};
            if ((rc = net_backward(st, buf, ns, cx->caches[it], d_state, &d_inp, &job, nullptr, 0))) return rc;
        }
        d_state = d_prev;
        if ((rc = label_terms(d_inp))) return rc;
    }
    if (sharded) {          // the ranks' shares of the weight gradients -> their sum in rank order, on every rank (and in place: gnn_loop_optimizer_step reads it)
        for (const LoopNet &n : loop_nets(l, cx)) {
            Net *net = n.net;
            float *all = nullptr;
            if ((rc = buf.get(&all, net->g_total * (size_t)l->world))) return rc;
            if ((rc = gnn_comm_allgather32(comm, net->grads, all, net->g_total, st))) return rc;
            HIPCHK(hipMemsetAsync(net->grads, 0, sizeof(float) * net->g_total, st));
            if ((rc = net_sum_parts(st, l->world, (int64_t)net->g_total, all, net->grads))) return rc;
        }
    }
    if ((rc = grad_prepare(l, cx, st))) return rc;     // the gradients the caller gets include the regularizer terms (gnn_mlp_set_regularizers)
    HIPCHK(hipMemcpyAsync(grads_state, ns.grads, sizeof(float) * ns.g_total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(grads_output, no_.grads, sizeof(float) * no_.g_total, hipMemcpyDeviceToHost, st));
    if (bn_batch_state && l->st->has_bn && k > 0)      // the statistics of the calls are adjacent, in call order
        HIPCHK(hipMemcpyAsync(bn_batch_state, ns.stats_all, sizeof(float) * (size_t)k * 2 * Ds, hipMemcpyDeviceToHost, st));
    if (bn_batch_output && l->ou->has_bn && M) HIPCHK(hipMemcpyAsync(bn_batch_output, cx->co.stats, sizeof(float) * 2 * T, hipMemcpyDeviceToHost, st));
    if (want_arcs && g->E) {
        if (M) hipLaunchKernelGGL(k_arc_grad_readout, cdiv(M * AL, 256), 256, 0, st, M, AL, l->edge_rows, d_feats, wf, 2 * (Ds + NLc), d_arcs);
        hipLaunchKernelGGL(k_arc_grad_agg, cdiv(g->E * AL, 256), 256, 0, st, g->E, AL, l->edge_dst, g->sh->arc_id, g->sh->arc_w, d_aa, d_arcs);
        HIPCHK(hipGetLastError());
        if (d_arcs_host) HIPCHK(hipMemcpyAsync(d_arcs_host, d_arcs, sizeof(float) * (size_t)g->E * AL, hipMemcpyDeviceToHost, st));
    }
    if (d_nodes_host && N)      // D == 0: state_0 = nodes (GNN.py:265), so the gradient of the initial state IS the label gradient
        HIPCHK(hipMemcpyAsync(d_nodes_host, l->D ? d_nodes : d_state, sizeof(float) * (size_t)N * NL, hipMemcpyDeviceToHost, st));
    if (keep_nodes) cx->kept_d_nodes = l->D ? d_nodes : d_state;
    if (keep_arcs && want_arcs) cx->kept_d_arcs = d_arcs;
    if (sync) HIPCHK(hipStreamSynchronize(st));
    cx->backward_done = true;
    return GNN_OK;
}

extern "C" int gnn_loop_train_backward(gnn_loop *l, const float *d_out_nodes, const float *d_state_extra, float *grads_state,
                                       float *grads_output, float *bn_batch_state, float *bn_batch_output, float *d_nodes_host,
                                       float *d_arcs_host)
{
    // the context stays (its gradients feed gnn_loop_optimizer_step) until the next forward; a second backward is refused
    return train_backward(l, nullptr, d_out_nodes, d_state_extra, grads_state, grads_output, bn_batch_state, bn_batch_output, d_nodes_host, d_arcs_host, true);
}

extern "C" int gnn_loop_train_backward_chained(gnn_loop *l, const float *d_out_nodes, gnn_loop *next, int get_state, int get_output, float *grads_state,
                                               float *grads_output, float *bn_batch_state, float *bn_batch_output, int keep_label_gradients)
{
    ARGCHK(l, "loop is NULL");
    ARGCHK(l->world == 1, "a chained backward pass is single-GPU (this loop is rank %d of %d)", l->rank, l->world);
    ARGCHK(keep_label_gradients >= 0 && keep_label_gradients <= (GNN_KEEP_D_NODES | GNN_KEEP_D_ARC_LABELS), "keep_label_gradients: GNN_KEEP_D_NODES, GNN_KEEP_D_ARC_LABELS, both or 0");
    const Chain chain{next, get_state != 0, get_output != 0, (keep_label_gradients & GNN_KEEP_D_NODES) != 0, (keep_label_gradients & GNN_KEEP_D_ARC_LABELS) != 0};
    return train_backward(l, nullptr, d_out_nodes, nullptr, grads_state, grads_output, bn_batch_state, bn_batch_output, nullptr, nullptr, true, &chain);
}

// what the last training forward decided for one of the loop's nets (the context outlives the backward pass: until the next forward)
extern "C" int gnn_loop_train_forms(const gnn_loop *l, int net, int *out)
{
    ARGCHK(l && out && (net == 0 || net == 1), "bad arguments");
    const gnn_train_ctx *cx = l->train_ctx;
    if (!cx) return gnn_fail(GNN_ERR_STATE, "gnn_loop_train_forward has not been called");
    gnn_train::net_forms(net == 0 ? cx->ns : cx->no_, out);
    return GNN_OK;
}

// the keep bytes of one Dropout of the last training forward (they live in the arena, which only the next forward resets: neither the
// backward pass nor the optimizer step nor an inference run writes them)
extern "C" int gnn_loop_train_mask(const gnn_loop *l, int net, int body, int pos, uint8_t *out, int64_t *count)
{
    ARGCHK(l && count && (net == 0 || net == 1), "bad arguments");
    const gnn_train_ctx *cx = l->train_ctx;
    if (!cx) return gnn_fail(GNN_ERR_STATE, "gnn_loop_train_forward has not been called");
    const Net &n = net == 0 ? cx->ns : cx->no_;
    ARGCHK(net == 1 || (body >= 0 && body < cx->k), "body %d: the last training forward ran %d", body, cx->k);
    ARGCHK(pos >= 0 && pos <= n.m->n_layers && n.rate[pos] != 0.0f, "no Dropout at position %d of this net", pos);
    if (net == 0 && cx->recompute)
        return gnn_fail(GNN_ERR_STATE, "the last training forward recomputes its activations (gnn_loop_set_train_recompute): net_state's keep bytes are scratch, not alive");
    const NetCache &c = net == 0 ? cx->caches[(size_t)body] : cx->co;
    if ((size_t)pos >= c.keep.size() || !c.keep[pos]) return gnn_fail(GNN_ERR_STATE, "internal: no mask recorded at position %d", pos);
    *count = n.rows * n.m->dims[pos];
    if (out && *count) {
        HIPCHK(hipSetDevice(l->device));
        HIPCHK(hipStreamSynchronize(l->stream));
        HIPCHK(hipMemcpy(out, c.keep[pos], (size_t)*count, hipMemcpyDeviceToHost));
    }
    return GNN_OK;
}

extern "C" int gnn_loop_train_step(gnn_loop *l, const int32_t *src_indptr, const int32_t *src_dst, const float *src_w,
                                   const float *targets, const float *sample_weights, int64_t n_targets, int loss_kind,
                                   int n_graphs, const int32_t *ng_indptr, const int32_t *ng_node, const float *ng_w,
                                   const float *dropout_state, const float *dropout_output, const uint8_t *masks_state,
                                   const uint8_t *masks_output, uint64_t seed, const float *bn_state, const float *bn_output,
                                   float *loss_out, float *k_out, float *grads_state, float *grads_output,
                                   float *bn_batch_state, float *bn_batch_output)
{
    ARGCHK(l && targets && sample_weights && loss_out && k_out && grads_state && grads_output, "bad arguments");
    ARGCHK(l->world == 1, "a training step is single-GPU (only the training-mode forward runs on shards: gnn_loop_train_forward)");
    ARGCHK(loss_kind >= 0 && loss_kind < LOSS_KINDS, LOSS_KIND_TEXT);
    const int64_t M = l->edge_mode ? l->n_edge_masked : l->g->n_masked;
    const int T = l->T;
    ARGCHK(!(l->edge_mode && n_graphs > 0), "an edge-based loop has no graph readout");
    ARGCHK(n_targets == (n_graphs > 0 ? n_graphs : M), "%lld target rows but %lld outputs", (long long)n_targets, (long long)(n_graphs > 0 ? n_graphs : M));
    ARGCHK(n_graphs <= 0 || (ng_indptr && ng_node && ng_w), "NodeGraph^T CSR required for a graph-based step");
    int rc = train_forward(l, src_indptr, src_dst, src_w, dropout_state, dropout_output, masks_state, masks_output, seed, bn_state, bn_output, k_out,
                           nullptr, false);
    if (rc) return rc;
    // loss and d loss / d out_nodes on the device, enqueued behind the forward pass: the step waits for the device once more, at its end
    gnn_train_ctx *cx = l->train_ctx;
    gnn_train_arena *arena = l->train_arena;
    Buf &buf = cx->buf;
    hipStream_t st = l->stream;
    float *d_t = nullptr, *d_w = nullptr, *d_o = nullptr, *d_dnodes = nullptr;
    double *d_lp = nullptr;
    const int64_t nt = n_targets;
    const unsigned lblocks = nt ? cdiv(nt, 256) : 0;
    double loss = 0.0;
    // (behind the loss partials: the penalty partials of the regularizers, gnn_mlp_set_regularizers - at most one per 256 trainable floats)
    const size_t pen_max = (l->st->reg_l1.empty() ? 0 : cdiv((int64_t)net_grad_floats(l->st), 256)) + (l->ou->reg_l1.empty() ? 0 : cdiv((int64_t)net_grad_floats(l->ou), 256));
    double *h_lp = static_cast<double *>(arena->host.get(std::max<size_t>(sizeof(double) * (lblocks + pen_max), 4096)));
    if (!h_lp) return gnn_fail(GNN_ERR_HIP, "hipHostMalloc failed");
    // the step's small inputs, packed into pinned memory and uploaded in one transfer: targets | sample weights | NodeGraph^T CSR
    const int64_t ne = n_graphs > 0 ? ng_indptr[n_graphs] : 0;
    auto pad4 = [](size_t words) { return (words + 63) & ~(size_t)63; };
    const size_t o_t = 0, o_w = o_t + pad4((size_t)nt * T), o_ip = o_w + pad4((size_t)nt), o_nd = o_ip + pad4(n_graphs > 0 ? (size_t)n_graphs + 1 : 0),
                 o_nw = o_nd + pad4((size_t)ne), up_words = o_nw + pad4((size_t)ne);
    float *up = nullptr;
    if (up_words) {
        float *hs = static_cast<float *>(arena->stage.get(sizeof(float) * up_words));
        if (!hs) return gnn_fail(GNN_ERR_HIP, "hipHostMalloc failed");
        if ((rc = buf.get(&up, up_words))) return rc;
        if (nt) { memcpy(hs + o_t, targets, sizeof(float) * (size_t)nt * T); memcpy(hs + o_w, sample_weights, sizeof(float) * (size_t)nt); }
        if (n_graphs > 0) {
            memcpy(hs + o_ip, ng_indptr, sizeof(int32_t) * ((size_t)n_graphs + 1));
            if (ne) { memcpy(hs + o_nd, ng_node, sizeof(int32_t) * (size_t)ne); memcpy(hs + o_nw, ng_w, sizeof(float) * (size_t)ne); }
        }
        HIPCHK(hipMemcpyAsync(up, hs, sizeof(float) * up_words, hipMemcpyHostToDevice, st));
        d_t = up + o_t; d_w = up + o_w;
    }
    if (nt && ((rc = buf.get(&d_o, (size_t)nt * T)) || (rc = buf.get(&d_lp, (size_t)lblocks)))) return rc;
    if (n_graphs > 0) {                            // GNNgraphBased: out = NodeGraph^T . out_nodes (GNN.py:331-332)
        const int32_t *d_ip = reinterpret_cast<const int32_t *>(up + o_ip), *d_nd = reinterpret_cast<const int32_t *>(up + o_nd);
        const float *d_nw = up + o_nw;
        float *og = nullptr;
        if ((rc = buf.get(&og, (size_t)n_graphs * T)) || (rc = buf.get(&d_dnodes, (size_t)M * T))) return rc;
        HIPCHK(hipMemsetAsync(d_dnodes, 0, sizeof(float) * std::max<size_t>(1, (size_t)M * T), st));
        hipLaunchKernelGGL(k_graph_out, cdiv(n_graphs, 4), 256, 0, st, n_graphs, T, d_ip, d_nd, d_nw, cx->out_nodes, og);
        hipLaunchKernelGGL(k_loss_rows, lblocks, 256, 0, st, loss_kind, nt, T, d_t, og, d_w, l->train.loss.smoothing, l->train.loss.delta, d_o, d_lp);
        if (ne) hipLaunchKernelGGL(k_graph_out_bwd, cdiv(ne * T, 256), 256, 0, st, n_graphs, T, d_ip, d_nd, d_nw, d_o, d_dnodes);
        HIPCHK(hipGetLastError());
    } else if (nt) {
        hipLaunchKernelGGL(k_loss_rows, lblocks, 256, 0, st, loss_kind, nt, T, d_t, cx->out_nodes, d_w, l->train.loss.smoothing, l->train.loss.delta, d_o, d_lp);
        HIPCHK(hipGetLastError());
        d_dnodes = d_o;
    }
    if (lblocks) HIPCHK(hipMemcpyAsync(h_lp, d_lp, sizeof(double) * lblocks, hipMemcpyDeviceToHost, st));
    rc = train_backward(l, d_dnodes, nullptr, nullptr, grads_state, grads_output, bn_batch_state, bn_batch_output, nullptr, nullptr, false);
    if (rc) return rc;
    const unsigned pblocks = cx->pen_blocks[0] + cx->pen_blocks[1];       // the penalty is part of the loss (GNN_BaseClass.py:223-235)
    if (pblocks > pen_max) return gnn_fail(GNN_ERR_STATE, "internal: more penalty partials than announced");
    if (pblocks) HIPCHK(hipMemcpyAsync(h_lp + lblocks, cx->pen_part, sizeof(double) * pblocks, hipMemcpyDeviceToHost, st));
    if (l->train.opt.armed) {                      // gnn_loop_arm_optimizer: the update rides on this step's stream work
        const auto &opt = l->train.opt;
        l->train.opt.armed = false;
        // (mode 1: net_state's gradients are no sum over bodies, `mean` has nothing to average)
        const float gscale = (opt.mean && cx->k > 0 && !cx->fixed_point) ? 1.0f / (float)cx->k : 1.0f;
        if ((rc = update_both(l, cx, st, opt.kind, opt.h, gscale, opt.mom_s, opt.mom_o, true, 1.0))) return rc;
        cx->applied = true;
    }
    HIPCHK(hipStreamSynchronize(st));
    for (unsigned b = 0; b < lblocks + pblocks; ++b) loss += h_lp[b];
    *loss_out = (float)loss;
    return GNN_OK;
}
