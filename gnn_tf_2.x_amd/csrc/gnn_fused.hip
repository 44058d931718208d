// Host side of the fused iteration kernel (device code: gnn_fused_kernel.h): which nets it covers, the packed weight
// image, the loop-invariant label block, the launch form of a run (gnn_loop_decide_form) and the per-iteration launch.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "gnn_engine.h"
#include "gnn_fused.h"

namespace {

constexpr int MAXL = GNN_FUSED_MAXL;
constexpr int K_GROUP = 12;     // layer-0 K-steps are consumed in pipelined groups of 3 x 4 (layer_from_lds)
constexpr int K_SLACK = 8;      // zero K-steps after the layer-0 block: the pipeline prefetches two groups past the end

constexpr int GNN_FUSED_VARIANT_DEFAULT = 1;      // bit 0: raised wave priority during the gather (measured: -1 %)
// start-up spread: every wave waits 0 .. n x 8k cycles before its first tile.  Round 2 / 3 (two tickets per wave drawn at kernel start, which
// already spread the waves by up to 46 us): 20 rounds, 12 for grids with one to four tiles per wave.  Round 4 (static first two rounds of
// tiles, no atomics at start; profiles/r04_midsize.txt): 8 and 6.
#ifndef GNN_FUSED_SPREAD_DEFAULT      // (a macro so that an A/B build can turn it)
#define GNN_FUSED_SPREAD_DEFAULT 8
#endif
constexpr int GNN_FUSED_SPREAD_SMALL_DEFAULT = 6;
// gather form of the full-tile kernel when the loop leaves the choice to the library (gnn_loop_set_gather_form(l, 0)): 1 walks the CSR, 2 reads
// the graph's gather program.  A macro so that an A/B build (tools/ab_build.sh) can turn it; the measurement behind the shipped value:
// docs/DESIGN_appendix.md A.1, profiles/r10_gather_program.txt
#ifndef GNN_GATHER_FORM_DEFAULT
#define GNN_GATHER_FORM_DEFAULT 2
#endif
// tile schedule of the program kernel when the loop leaves the choice to the library (gnn_loop_set_tile_schedule(l, 0)): 1 tiles in ascending
// order, 2 the balanced order (gnn_tile_schedule_build) - taken only by launches of at least four tiles per wave; below that, the latency
// regime, nothing about it has been measured and the order stays ascending.  The measurement behind the shipped value:
// profiles/tile_schedule.txt
#ifndef GNN_TILE_SCHEDULE_DEFAULT
#define GNN_TILE_SCHEDULE_DEFAULT 2
#endif
constexpr int S_SLACK = 2;      // zero chunks after the layer-0 block of the split image (layer0_split looks two chunks ahead)

int round_tiles(int width) { return width <= 32 ? 1 : (width <= 64 ? 2 : 4); }

// The nets the fused paths cover: one to three Dense layers no wider than 128, no softmax, ONE activation for all hidden layers (p.act) and
// any of the six for the last layer (p.act_last; a one-layer net has act == act_last).  Three layers with two different hidden activations
// are not covered.  Feature tiles of 32: NTL = tiles of the last layer (width <= 32: 1, <= 64: 2, else 4), NT = tiles of the widest
// hidden layer, at least NTL; of these only (NT, NTL) = (1,1) (2,2) (4,2) (4,4) are instantiated, so (2,1) and (4,1) become (2,2), (4,2).
bool make_plan(const gnn_mlp *m, int nlc, FusedPlan &p)
{
    if (m->n_layers < 1 || m->n_layers > MAXL) return false;
    p.layers = m->n_layers;
    p.act_last = m->acts[m->n_layers - 1];
    p.act = m->n_layers > 1 ? m->acts[0] : p.act_last;
    int hid = 0;
    for (int l = 0; l < m->n_layers; ++l) {
        if (m->acts[l] < GNN_ACT_LINEAR || m->acts[l] >= GNN_ACT_SOFTMAX) return false;
        if (l < m->n_layers - 1 && m->acts[l] != p.act) return false;              // one activation for all hidden layers
        if (m->dims[l + 1] > 128) return false;
        if (l < m->n_layers - 1) hid = std::max(hid, m->dims[l + 1]);
    }
    p.NTL = round_tiles(m->dims.back());
    if (p.layers == 1) {
        p.NT = p.NTL;
    } else {
        p.NT = std::max(round_tiles(hid), p.NTL);
        if (p.NT > 1 && p.NTL == 1) p.NTL = 2;          // instantiated pairs: (1,1) (2,2) (4,2) (4,4)
    }
    p.kk0 = ((m->dims[0] + 1) / 2 + K_GROUP - 1) / K_GROUP * K_GROUP;
    p.KP = std::max(2 * p.kk0, (m->dims[0] + 15) / 16 * 16) + 1;      // odd: conflict-free column reads
    size_t off = 0;
    for (int l = 0; l < p.layers; ++l) {
        p.nt[l] = l == p.layers - 1 ? p.NTL : p.NT;
        p.kk[l] = l == 0 ? p.kk0 : 16 * p.NT;
        p.w_off[l] = off;
        off += (size_t)(p.kk[l] + (l == 0 ? K_SLACK : 0)) * 64 * p.nt[l];
    }
    for (int l = 0; l < p.layers; ++l) { p.b_off[l] = off; off += 32 * (size_t)p.nt[l]; }
    p.bn_off = off;
    off += 2 * 32 * (size_t)p.NTL;
    p.total = off;
    const int ds = m->dims.back();
    p.pad = ds == 64 ? (4 - (ds + nlc) % 4) % 4 : 0;
    p.KPs = p.KP;
    if (ds == 64) {
        p.KPs = (std::max(2 * p.kk0, (m->dims[0] + p.pad + 15) / 16 * 16) + 3) / 4 * 4;
        if ((p.KPs / 4) % 2 == 0) p.KPs += 4;
    }
    size_t soff = 0;
    for (int l = 0; l < p.layers; ++l) {
        p.chunks[l] = l == 0 ? (m->dims[0] + p.pad + 15) / 16 : 2 * p.NT;
        p.s_off[l] = soff;
        soff += (size_t)(p.chunks[l] + (l == 0 ? S_SLACK : 0)) * p.nt[l] * 3 * 256;
    }
    for (int l = 0; l < p.layers; ++l) {
        p.h_off[l] = soff;
        soff += (size_t)(p.chunks[l] + (l == 0 ? S_SLACK : 0)) * p.nt[l] * 2 * 256;
    }
    p.s_total = soff;
    return true;
}

// LDS of a workgroup of `waves` waves: waves wave tiles [32][KP], 128 B of slack (the layer-0 pipeline reads two groups past the last tile), waves x 36 row pointers
size_t lds_bytes(const FusedPlan &p, int waves = GNN_FUSED_WAVES)
{
    // ... and the last layer's bias / BatchNormalization scale / shift (3 x 32 NTL floats) and the hidden biases (2 x 32 NT)
    return (size_t)waves * 32 * std::max(p.KP, p.KPs) * sizeof(float) + 128 + waves * 36 * sizeof(int) + (3 + 2) * 32 * 4 * sizeof(float) + 16;
}

// Wide-state form (gnn_loop_set_wide_state): k_fused_generic on a workgroup of fewer than eight waves, for a plan whose eight tiles do not
// fit one workgroup's LDS.  State widths 68 .. 128 in multiples of 4 (load_tile_wide's rows; up to 64 the label projection is the answer,
// and width 64 is k_fused_full's, which keeps eight waves).  Returns the waves per workgroup - the most that fit, at least 4, one per
// SIMD - or 0: not taken (mode 0, a plan that eight waves cover, another width, no room for four tiles, or mode 1 below its row floor).
// mode 1 ('auto') takes the form where profiles/wide_state.txt measured it faster than one kernel per op: from GNN_WIDE_AUTO_MIN_ROWS owned rows.
constexpr int64_t GNN_WIDE_AUTO_MIN_ROWS = 1;
int wide_waves(const FusedPlan &p, int ds, int mode, int64_t n_rows)
{
    if (mode == 0 || ds % 4 != 0 || ds <= 64 || ds > 128 || n_rows < 1) return 0;
    if (lds_bytes(p) <= 160 * 1024) return 0;
    if (mode == 1 && n_rows < GNN_WIDE_AUTO_MIN_ROWS) return 0;
    int w = GNN_FUSED_WAVES - 1;
    while (w >= 4 && lds_bytes(p, w) > 160 * 1024) --w;
    return w >= 4 ? w : 0;
}

// the wave-pair form (gnn_fused_pair_kernel.h) covers the tuned shape family only: split arithmetic, state width 64, two or three layers, 128-wide
// hidden layers, a concat of nine K = 16 chunks, one activation for all layers
constexpr int PAIR_CH0 = 9;
bool pair_covers(const FusedPlan &p, int ds)
{
    return ds == 64 && p.NTL == 2 && p.NT == 4 && (p.layers == 2 || p.layers == 3) && p.chunks[0] == PAIR_CH0 && p.act_last == p.act;
}
int pair_xs(const FusedPlan &p)       // row stride of a pair's gather tile X' (the LDS columns behind the own state), a multiple of 4 with XS / 4 odd
{
    int xs = 16 * p.chunks[0] - 64 + 4;
    if ((xs / 4) % 2 == 0) xs += 4;
    return xs;
}
// four pairs x (X'[32][XS] + P[CH0][3][64] x 16 B), 16 control words, 8 x 20 row pointers, staged vectors, slack
size_t pair_lds_bytes(const FusedPlan &p)
{
    return sizeof(float) * ((size_t)4 * (32 * pair_xs(p) + p.chunks[0] * 768) + 16 + GNN_FUSED_WAVES * 20 + 3 * 32 * 2 + 2 * 32 * 4) + 128;
}
// The persistent small-graph launch (gnn_small_common.h) a net takes on n_rows owned rows, as far as the net and the row count decide it
// (gnn_loop_decide_form adds what depends on the loop and the device: single GPU, not disabled, not profiling); m is covered by p.
//   narrow: every layer one 32-feature tile - 16-node tiles (k_small16) up to 4,096 rows, 32-node tiles (k_small_loop) up to 8,192;
//   wide:   two or three layers, every hidden layer <= 64 and at least one > 32, state <= 32 - 16-node tiles (k_small16, WIDE) up to 4,096 rows
//           (256 one-wave workgroups); there is no 32-node wide form, so a wide net on more rows takes one launch per body.
// Both need the concat (layer-0 K) within 96 columns: the largest instantiated step count, 24 x 4 = 48 x 2.  From the net's real widths:
// make_plan turns the tiles (NT, NTL) = (2, 1) of a wide net into (2, 2).
struct SmallForm {
    int tile = 0;            // 0: not persistent; 16 / 32 rows per tile
    bool wide = false;
    int steps = 0;           // instantiated layer-0 K-steps: of 4 on 16-node tiles (GnnSmall16S0), of 2 on 32-node tiles (GnnSmallKK0)
};
SmallForm small_form(const gnn_mlp *m, const FusedPlan &p, int64_t n_rows)
{
    SmallForm f;
    const int concat = m->dims[0];
    if (n_rows < 1 || concat > 96) return f;
    int hid = 0;
    for (int l = 1; l < m->n_layers; ++l) hid = std::max(hid, m->dims[l]);
    const bool narrow = hid <= 32 && m->dims.back() <= 32;
    const bool wide = !narrow && (m->n_layers == 2 || m->n_layers == 3) && hid <= 64 && m->dims.back() <= 32;
    if (!(narrow && n_rows <= 32 * 256) && !(wide && n_rows <= 16 * 256)) return f;
    // K-steps of layer 0 the kernels keep in registers: the smallest instantiated count that covers the concat width (32-node tiles: the
    // packed image has p.kk0 >= that many; the steps dropped are zero rows of the image)
    if (n_rows <= 16 * 256) {
        // 16-node tiles while twice the workgroups are still resident at once: a body is a chain of latencies, and a 16-node tile's dense
        // layers and activations are half as long
        f.tile = 16;
        f.wide = wide;
        for (int cand : GnnSmall16S0::values)
            if (4 * cand >= concat) { f.steps = cand; break; }
    } else {
        f.tile = 32;
        f.steps = p.kk0;
        for (int cand : GnnSmallKK0::values)
            if (2 * cand >= concat && cand <= p.kk0) { f.steps = cand; break; }
    }
    return f;
}

int device_cus(int device)
{
    static int n_cu_dev[64] = {0};
    if (device < 0 || device >= 64) return 256;
    if (!n_cu_dev[device]) {
        hipDeviceProp_t prop;
        n_cu_dev[device] = hipGetDeviceProperties(&prop, device) == hipSuccess ? std::max(1, prop.multiProcessorCount) : 256;
    }
    return n_cu_dev[device];
}

}   // namespace

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// fp16 x 2 pieces (piece format 2, gnn_fused_kernel.h): the exponent e of a layer's weight scale 2^e puts max |W| 2^e into [2^14, 2^15) - the
// largest scaled weight stays a factor 2 below the fp16 maximum 65504, the smallest normal fp16 piece (2^-14) sits 2^28 - 2^29 below the
// largest weight.  A zero layer keeps e = 0.
extern "C" int gnn_split_f16_exponent(float max_abs)
{
    if (!(max_abs > 0.0f) || !std::isfinite(max_abs)) return 0;
    int e2 = 0;
    (void)std::frexp(max_abs, &e2);          // max_abs = f 2^e2, f in [0.5, 1): max_abs 2^(15 - e2) in [2^14, 2^15)
    return std::min(60, std::max(-60, 15 - e2));      // (bounded: the bias times 2^(e + GNN_F16_EX) stays far inside the fp32 range)
}
// pieces of n values at scale 2^e, round-to-nearest-even: p0 = fp16(v 2^e), p1 = fp16(v 2^e - p0) (the difference is exact in fp32)
extern "C" void gnn_split_f16(const float *v, int n, int e, uint16_t *p0, uint16_t *p1)
{
    for (int i = 0; i < n; ++i) {
        const float s = std::ldexp(v[i], e);
        const _Float16 h0 = (_Float16)s;
        const _Float16 h1 = (_Float16)(s - (float)h0);
        memcpy(p0 + i, &h0, 2);
        memcpy(p1 + i, &h1, 2);
    }
}

int gnn_fused_pack(gnn_mlp *m, int nlc)
{
    FusedPlan p;
    if (!make_plan(m, nlc, p)) { gnn_fused_release(m); return GNN_OK; }
    m->pack_nlc = nlc;
    const int lab = m->dims.back() + nlc;      // [state | nodes] columns in front of the alignment hole
    std::vector<float> img(p.total, 0.0f);
    std::vector<uint32_t> simg(p.s_total, 0u);
    std::vector<float> W, b;
    for (int l = 0; l < m->n_layers; ++l) {
        const int n_in = m->dims[l], n_out = m->dims[l + 1];
        W.resize((size_t)n_in * n_out);
        b.resize(n_out);
        HIPCHK(hipMemcpy(W.data(), m->W[l], W.size() * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(b.data(), m->b[l], b.size() * sizeof(float), hipMemcpyDeviceToHost));
        float *wp = img.data() + p.w_off[l];
        const int nt = p.nt[l];
        for (int kk = 0; kk < p.kk[l]; ++kk)
            for (int lane = 0; lane < 64; ++lane)
                for (int jt = 0; jt < nt; ++jt) {
                    const int k = 2 * kk + (lane >> 5), j = 32 * jt + (lane & 31);
                    wp[((size_t)kk * 64 + lane) * nt + jt] = (k < n_in && j < n_out) ? W[(size_t)k * n_out + j] : 0.0f;
                }
        for (int j = 0; j < n_out; ++j) img[p.b_off[l] + j] = b[j];
        // split image: [chunk][out tile][piece][lane][8 bf16]; element i of lane (m, h) is k(h, i) of gnn_fused_kernel.h
        // Folded SELU between the dense layers of the split path (gnn_fused_kernel.h, GNN_S1_E): a layer whose OUTPUT feeds the
        // folded activation is scaled by log2(e) (so is its bias, at staging), a layer whose INPUT comes from it by scale / log2(e).
        // Keyed on the HIDDEN activation: the last layer's output (its own activation, p.act_last) is never folded.
        float fold = 1.0f;
        if (p.act == GNN_ACT_SELU && m->n_layers > 1) {
            const double LOG2E = 1.44269504088896341, SCALE = 1.0507009873554805;
            const bool in_folded = l > 0, out_folded = l < m->n_layers - 1;
            fold = (float)((in_folded ? SCALE / LOG2E : 1.0) * (out_folded ? LOG2E : 1.0));
        }
        uint32_t *sp = simg.data() + p.s_off[l];
        std::vector<float> wf((size_t)p.chunks[l] * nt * 64 * 8);      // the folded weights in image order
        for (int c = 0; c < p.chunks[l]; ++c)
            for (int jt = 0; jt < nt; ++jt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 8; ++i) {
                        const int h = lane >> 5, r = 8 * (c & 1) + i;
                        int k = l == 0 ? 16 * c + 8 * h + i : 32 * (c >> 1) + (r & 3) + 8 * (r >> 2) + 4 * h;
                        if (l == 0 && p.pad) k = k < lab ? k : (k < lab + p.pad ? n_in : k - p.pad);   // LDS column -> concat column (hole: zero)
                        const int j = 32 * jt + (lane & 31);
                        float v = (k < n_in && j < n_out) ? W[(size_t)k * n_out + j] : 0.0f;
                        v *= fold;
                        wf[(((size_t)c * nt + jt) * 64 + lane) * 8 + i] = v;
                        for (int pc = 0; pc < 3; ++pc) {          // truncation split: v == p0 + p1 + p2 exactly
                            uint32_t bits;
                            memcpy(&bits, &v, 4);
                            const uint32_t hi = bits & 0xffff0000u;
                            float piece;
                            memcpy(&piece, &hi, 4);
                            v = v - piece;
                            uint32_t &d = sp[((((size_t)c * nt + jt) * 3 + pc) * 64 + lane) * 4 + i / 2];
                            d |= (i & 1) ? hi : (hi >> 16);
                        }
                    }
        // fp16 x 2 image of the same (folded) weights in the same order: [chunk][out tile][piece][lane][8 fp16], at the layer's scale 2^e
        float mw = 0.0f;
        for (float v : wf) mw = std::max(mw, std::fabs(v));
        const int e = gnn_split_f16_exponent(mw);
        m->split_exp[l] = e;
        std::vector<uint16_t> h0(wf.size()), h1(wf.size());
        gnn_split_f16(wf.data(), (int)wf.size(), e, h0.data(), h1.data());
        uint16_t *hp = reinterpret_cast<uint16_t *>(simg.data() + p.h_off[l]);
        for (int c = 0; c < p.chunks[l]; ++c)
            for (int jt = 0; jt < nt; ++jt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 8; ++i) {
                        const size_t src = (((size_t)c * nt + jt) * 64 + lane) * 8 + i;
                        hp[((((size_t)c * nt + jt) * 2 + 0) * 64 + lane) * 8 + i] = h0[src];
                        hp[((((size_t)c * nt + jt) * 2 + 1) * 64 + lane) * 8 + i] = h1[src];
                    }
    }
    if (m->has_bn) {
        const int f = m->dims.back();
        HIPCHK(hipMemcpy(img.data() + p.bn_off, m->bn_scale, f * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(img.data() + p.bn_off + 32 * p.NTL, m->bn_shift, f * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (m->packed_floats != p.total) {
        gnn_fused_release(m);
        HIPCHK(gnn_dev_malloc((void **)&m->packed, p.total * sizeof(float)));
        m->packed_floats = p.total;
    }
    HIPCHK(hipMemcpy(m->packed, img.data(), p.total * sizeof(float), hipMemcpyHostToDevice));
    if (m->packed_split_dwords != p.s_total) {
        if (m->packed_split) (void)hipFree(m->packed_split);
        m->packed_split = nullptr;
        HIPCHK(gnn_dev_malloc((void **)&m->packed_split, p.s_total * sizeof(uint32_t)));
        m->packed_split_dwords = p.s_total;
    }
    HIPCHK(hipMemcpy(m->packed_split, simg.data(), p.s_total * sizeof(uint32_t), hipMemcpyHostToDevice));
    return GNN_OK;
}

// What the fused paths make of a net of this description (include/gnn_hip.h): make_plan itself, host code, no device
extern "C" int gnn_fused_net_form(int n_layers, const int *dims, const int *acts, int n_label_cols_in_concat, int *out)
{
    ARGCHK(n_layers >= 1 && n_layers <= 16 && dims && acts && n_label_cols_in_concat >= 0 && out, "bad arguments");
    gnn_mlp m;
    m.n_layers = n_layers;
    m.dims.assign(dims, dims + n_layers + 1);
    m.acts.assign(acts, acts + n_layers);
    for (int l = 0; l <= n_layers; ++l) ARGCHK(m.dims[l] >= 1, "bad layer width");
    for (int l = 0; l < n_layers; ++l) ARGCHK(m.acts[l] >= GNN_ACT_LINEAR && m.acts[l] <= GNN_ACT_SOFTMAX, "bad activation code");
    FusedPlan p;
    const bool covered = make_plan(&m, n_label_cols_in_concat, p);
    for (int i = 0; i < 6; ++i) out[i] = 0;
    if (!covered) return GNN_OK;
    out[0] = 1; out[1] = p.act; out[2] = p.act_last; out[3] = p.NT; out[4] = p.NTL; out[5] = p.act_last != p.act ? 1 : 0;
    return GNN_OK;
}

// Which persistent small-graph launch a net of this description takes on n_rows owned rows (include/gnn_hip.h): small_form itself, host
// code, no device
extern "C" int gnn_small_form(int n_layers, const int *dims, const int *acts, int n_label_cols_in_concat, int64_t n_rows, int *out)
{
    ARGCHK(n_layers >= 1 && n_layers <= 16 && dims && acts && n_label_cols_in_concat >= 0 && n_rows >= 0 && out, "bad arguments");
    gnn_mlp m;
    m.n_layers = n_layers;
    m.dims.assign(dims, dims + n_layers + 1);
    m.acts.assign(acts, acts + n_layers);
    for (int l = 0; l <= n_layers; ++l) ARGCHK(m.dims[l] >= 1, "bad layer width");
    for (int l = 0; l < n_layers; ++l) ARGCHK(m.acts[l] >= GNN_ACT_LINEAR && m.acts[l] <= GNN_ACT_SOFTMAX, "bad activation code");
    FusedPlan p;
    out[0] = out[1] = out[2] = 0;
    if (!make_plan(&m, n_label_cols_in_concat, p)) return GNN_OK;
    const SmallForm f = small_form(&m, p, n_rows);
    out[0] = f.tile; out[1] = f.wide ? 1 : 0; out[2] = f.steps;
    return GNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// label projection (gnn_loop_set_label_projection): layer 0 of net_state split by rows of W1
//   state rows [0, Ds), aggregated-state rows [Ds + NLc, 2 Ds + NLc): the "shadow" net over [state | aggregated state], an ordinary plan
//   with dims[0] = 2 Ds and no label columns, run by the seeded kernels;
//   label rows (everything else, in the column order of l->inv): P = inv . W1_label + b1 once per Loop (gnn_label_project.hip).
// ---------------------------------------------------------------------------------------------------------------------
namespace {

// description of the shadow net of m for state width ds (host only: widths and activations)
void shadow_describe(const gnn_mlp *m, int ds, gnn_mlp &s)
{
    s.n_layers = m->n_layers;
    s.dims = m->dims;
    s.dims[0] = 2 * ds;
    s.acts = m->acts;
}

// The shape part of the projection decision: the shadow plan, and whether the fused kernels cover it (make_plan, one workgroup's LDS, the
// gather's column chunks - as gnn_fused_supported).  m->dims[0] must be the concat [state | nodes | agg state | agg nodes | agg arcs].
// waves: the waves per workgroup the shadow plan runs on - eight, or with a wide-state mode (wide_mode, on n_rows rows) wide_waves' count
bool projection_plan(const gnn_mlp *m, int ds, int nlc, int al, FusedPlan &sp, int wide_mode = 0, int64_t n_rows = 0, int *waves = nullptr)
{
    if (2 * nlc + al <= 0 || ds < 1 || m->dims.back() != ds || m->dims[0] != 2 * ds + 2 * nlc + al) return false;
    gnn_mlp s;
    shadow_describe(m, ds, s);
    if (!make_plan(&s, 0, sp)) return false;
    if (!((ds % 4 == 0 && ds <= 256) || ds <= 64)) return false;
    int w = GNN_FUSED_WAVES;
    if (lds_bytes(sp) > 160 * 1024 && !(w = wide_waves(sp, ds, wide_mode, n_rows))) return false;
    if (waves) *waves = w;
    return true;
}

void projection_release(gnn_mlp *m)
{
    if (m->proj) {
        gnn_fused_release(m->proj);
        if (m->proj->slab) (void)hipFree(m->proj->slab);
        delete m->proj;
    }
    if (m->proj_wl) (void)hipFree(m->proj_wl);
    m->proj = nullptr;
    m->proj_wl = nullptr;
    m->proj_wl_floats = 0;
    m->proj_version = ~(uint64_t)0;
}

// The shadow net's images and the label rows of W1, rebuilt when the weights (m->version) or the concat layout changed since they were built
int projection_ensure(gnn_mlp *m, int ds, int nlc, int al, const FusedPlan &sp)
{
    if (m->proj && m->proj_version == m->version && m->proj_ds == ds && m->proj_nlc == nlc && m->proj_al == al) return GNN_OK;
    const int n_in = m->dims[0], h1 = m->dims[1], iw = 2 * nlc + al, hp = 32 * sp.nt[0];
    std::vector<float> W((size_t)n_in * h1), b(h1);
    HIPCHK(hipMemcpy(W.data(), m->W[0], W.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(b.data(), m->b[0], b.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<float> ws((size_t)2 * ds * h1), wl((size_t)(iw + 2) * hp, 0.0f);      // (label rows, one zero row, the bias)
    int rs = 0, rl = 0;
    for (int k = 0; k < n_in; ++k) {
        const bool label = (k >= ds && k < ds + nlc) || k >= 2 * ds + nlc;      // [nodes] | [agg nodes | agg arcs]: the column order of l->inv
        if (label) memcpy(wl.data() + (size_t)rl++ * hp, W.data() + (size_t)k * h1, sizeof(float) * h1);
        else memcpy(ws.data() + (size_t)rs++ * h1, W.data() + (size_t)k * h1, sizeof(float) * h1);
    }
    memcpy(wl.data() + (size_t)(iw + 1) * hp, b.data(), sizeof(float) * h1);
    if (!m->proj) m->proj = new gnn_mlp;
    gnn_mlp *s = m->proj;
    if (s->slab_floats != ws.size()) {
        if (s->slab) (void)hipFree(s->slab);
        s->slab = nullptr; s->slab_floats = 0;
        HIPCHK(gnn_dev_malloc((void **)&s->slab, ws.size() * sizeof(float)));
        s->slab_floats = ws.size();
    }
    HIPCHK(hipMemcpy(s->slab, ws.data(), ws.size() * sizeof(float), hipMemcpyHostToDevice));
    shadow_describe(m, ds, *s);
    s->device = m->device;
    s->W = m->W; s->b = m->b;
    s->W[0] = s->slab;
    s->has_bn = m->has_bn; s->bn_scale = m->bn_scale; s->bn_shift = m->bn_shift;      // (borrowed, like W[1..] and b: only slab and the images are the shadow's own)
    if (m->proj_wl_floats != wl.size()) {
        if (m->proj_wl) (void)hipFree(m->proj_wl);
        m->proj_wl = nullptr; m->proj_wl_floats = 0;
        HIPCHK(gnn_dev_malloc((void **)&m->proj_wl, wl.size() * sizeof(float)));
        m->proj_wl_floats = wl.size();
    }
    HIPCHK(hipMemcpy(m->proj_wl, wl.data(), wl.size() * sizeof(float), hipMemcpyHostToDevice));
    m->proj_version = ~(uint64_t)0;               // (until the images stand)
    int rc = gnn_fused_pack(s, 0);
    if (rc) return rc;
    if (!s->packed || !s->packed_split) return gnn_fail(GNN_ERR_STATE, "label projection: the shadow net has no weight images");
    s->pack_dirty = false;
    m->proj_version = m->version; m->proj_ds = ds; m->proj_nlc = nlc; m->proj_al = al;
    return GNN_OK;
}

}   // namespace

// What the projection decision answers from shapes alone (include/gnn_hip.h): host code, no device.  The loop's part - impl 2, no
// feature-sliced exchange, a single GPU not profiling for the persistent small-graph loop - is taken at its defaults.
extern "C" int gnn_label_projection_form(int n_layers, const int *dims, const int *acts, int state_dim, int n_label_cols_in_concat, int arc_label_dim,
                                         int64_t n_rows, int mode, int *out)
{
    ARGCHK(n_layers >= 1 && n_layers <= 16 && dims && acts && state_dim >= 1 && n_label_cols_in_concat >= 0 && arc_label_dim >= 0 && n_rows >= 0 &&
           mode >= 0 && mode <= 2 && out, "bad arguments");
    gnn_mlp m;
    m.n_layers = n_layers;
    m.dims.assign(dims, dims + n_layers + 1);
    m.acts.assign(acts, acts + n_layers);
    for (int l = 0; l <= n_layers; ++l) ARGCHK(m.dims[l] >= 1, "bad layer width");
    for (int l = 0; l < n_layers; ++l) ARGCHK(m.acts[l] >= GNN_ACT_LINEAR && m.acts[l] <= GNN_ACT_SOFTMAX, "bad activation code");
    for (int i = 0; i < 4; ++i) out[i] = 0;
    if (mode == 0 || n_rows < 1) return GNN_OK;
    FusedPlan p, sp;
    const int ds = state_dim;
    const bool base_ok = make_plan(&m, n_label_cols_in_concat, p) && lds_bytes(p) <= 160 * 1024 && ((ds % 4 == 0 && ds <= 256) || ds <= 64);
    if (base_ok && small_form(&m, p, n_rows).tile != 0) return GNN_OK;      // the persistent small-graph loop: exact arithmetic, stays as it is
    if (mode == 1 && base_ok) return GNN_OK;                                // covered without it
    if (!projection_plan(&m, ds, n_label_cols_in_concat, arc_label_dim, sp)) return GNN_OK;
    out[0] = 1;
    out[1] = (ds == 64 && sp.NTL == 2 ? GNN_BODY_FULL_TILE : GNN_BODY_GENERIC) + 1;      // as gnn_loop_body_kernel
    out[2] = 2 * n_label_cols_in_concat + arc_label_dim;
    out[3] = sp.nt[0];
    return GNN_OK;
}

// What the wide-state decision answers from shapes alone (include/gnn_hip.h): host code, no device.  The loop's part is taken at its
// defaults, as in gnn_label_projection_form: impl 2 (the label projection is a form of it; impl 1 takes the same decision without it), no
// feature-sliced exchange.  The same steps as gnn_loop_decide_form.
extern "C" int gnn_wide_state_form(int n_layers, const int *dims, const int *acts, int state_dim, int n_label_cols_in_concat, int arc_label_dim,
                                   int64_t n_rows, int mode, int label_projection_mode, int *out)
{
    ARGCHK(n_layers >= 1 && n_layers <= 16 && dims && acts && state_dim >= 1 && n_label_cols_in_concat >= 0 && arc_label_dim >= 0 && n_rows >= 0 &&
           mode >= 0 && mode <= 2 && label_projection_mode >= 0 && label_projection_mode <= 2 && out, "bad arguments");
    gnn_mlp m;
    m.n_layers = n_layers;
    m.dims.assign(dims, dims + n_layers + 1);
    m.acts.assign(acts, acts + n_layers);
    for (int l = 0; l <= n_layers; ++l) ARGCHK(m.dims[l] >= 1, "bad layer width");
    for (int l = 0; l < n_layers; ++l) ARGCHK(m.acts[l] >= GNN_ACT_LINEAR && m.acts[l] <= GNN_ACT_SOFTMAX, "bad activation code");
    for (int i = 0; i < 4; ++i) out[i] = 0;
    if (mode == 0 || n_rows < 1) return GNN_OK;
    FusedPlan p, sp;
    const int ds = state_dim, lpm = label_projection_mode;
    if ((int64_t)n_rows * ds * (int64_t)sizeof(float) >= ((int64_t)1 << 31)) return GNN_OK;      // 32-bit row offsets
    const bool shape_ok = make_plan(&m, n_label_cols_in_concat, p) && m.dims.back() == ds && ((ds % 4 == 0 && ds <= 256) || ds <= 64);
    const bool base_ok = shape_ok && lds_bytes(p) <= 160 * 1024;
    const int base_wide = shape_ok && !base_ok ? wide_waves(p, ds, mode, n_rows) : 0;
    int sw = 0;
    const bool seeded = lpm && (lpm == 2 || !base_ok) && !(base_ok && small_form(&m, p, n_rows).tile != 0) &&
                        projection_plan(&m, ds, n_label_cols_in_concat, arc_label_dim, sp, mode, n_rows, &sw) &&
                        (sw == GNN_FUSED_WAVES || !base_wide || lpm == 2);
    const int waves = seeded ? sw : (!base_ok && base_wide ? base_wide : GNN_FUSED_WAVES);
    if (waves == GNN_FUSED_WAVES) return GNN_OK;
    out[0] = 1;
    out[1] = GNN_BODY_GENERIC + 1;                    // as gnn_loop_body_kernel: the form is k_fused_generic's
    out[2] = waves;
    out[3] = seeded ? 1 : 0;
    return GNN_OK;
}

void gnn_fused_release(gnn_mlp *m)
{
    projection_release(m);
    if (m->packed) (void)hipFree(m->packed);
    if (m->packed_split) (void)hipFree(m->packed_split);
    m->packed = nullptr;
    m->packed_split = nullptr;
    m->packed_floats = 0;
    m->packed_split_dwords = 0;
}

// The feasibility part of the form decision: the plan of the loop's net_state, its weight images - packed HERE when the weights (or the
// concat layout) changed since they were built - and the shape limits of the kernels.
// wide: set to the waves per workgroup of the wide-state form where everything but one workgroup's LDS admits the net and the loop's
// mode takes the form (wide_waves), else to 0
static bool gnn_fused_supported(gnn_loop *l, FusedPlan &p, int &wide)
{
    wide = 0;
    if (!make_plan(l->st, l->NLc, p)) return false;
    if (l->st->pack_dirty || l->st->pack_nlc != l->NLc) {
        if (gnn_fused_pack(l->st, l->NLc) != GNN_OK) return false;
        l->st->pack_dirty = false;
    }
    if (!l->st->packed) return false;
    const int Ds = l->Ds;
    if (!((Ds % 4 == 0 && Ds <= 256) || Ds <= 64)) return false;           // one column chunk per lane in the gather
    if ((int64_t)l->N_pad * Ds * (int64_t)sizeof(float) >= ((int64_t)1 << 31)) return false;   // 32-bit row offsets
    if (l->g->n_rows <= 0) return false;
    if (lds_bytes(p) > 160 * 1024) {                                        // one 8-wave workgroup per CU
        wide = wide_waves(p, Ds, l->wide_state, l->g->n_rows);
        return false;
    }
    return true;
}

// label block [n_rows, IW]; rows padded to whole 32-node tiles and zeroed: the full-tile kernel reads the label columns of a partial last
// tile unguarded
static size_t inv_floats(const gnn_loop *l) { return std::max<size_t>(1, (size_t)((l->g->n_rows + 31) / 32 * 32) * (2 * l->NLc + l->g->AL)); }

static int fused_build_inv(gnn_loop *l);

// the loop-invariant label block of a fused run (allocated by the form decision), and the label projection of a seeded one
int gnn_fused_prepare(gnn_loop *l)
{
    const gnn_graph *g = l->g;
    const int IW = 2 * l->NLc + g->AL;
    if (!l->inv_zeroed) {
        HIPCHK(hipMemsetAsync(l->inv, 0, inv_floats(l) * sizeof(float), l->stream));
        l->inv_zeroed = true;
    }
    if (IW == 0) return GNN_OK;
    // [nodes | Adjacency^T . nodes | ArcNode^T . arc labels]  (GNN.py:263, :259): loop-invariant, and unchanged from run to run
    // unless gnn_graph_update_labels rewrote the labels in between (LGNN stacks)
    int rc = GNN_OK;
    if (l->inv_version != g->label_version) rc = fused_build_inv(l);
    // label projection: P from the block, cached with it - and rebuilt when net_state's weights changed (gnn_mlp_set_weights, optimizer step)
    if (!rc && l->form.seeded && (l->proj_labels != g->label_version || l->proj_weights != l->st->version)) {
        const gnn_mlp *m = l->st;
        rc = gnn_label_project_launch(l->stream, g->n_rows, IW, l->proj_nt, l->inv, m->proj_wl, m->proj_wl + (size_t)(IW + 1) * 32 * l->proj_nt, l->proj);
        if (!rc) { l->proj_labels = g->label_version; l->proj_weights = m->version; }
    }
    return rc;
}

static int fused_build_inv(gnn_loop *l)
{
    const gnn_graph *g = l->g;
    const int IW = 2 * l->NLc + g->AL;
    l->inv_version = g->label_version;
    int rc = gnn_launch_spmm(l->stream, g->n_rows, g->sh->indptr, nullptr, g->sh->arc_w, gnn_graph_arc_labels(g), g->AL, g->AL,
                             l->inv + 2 * l->NLc, IW, nullptr, 1);
    if (rc) return rc;
    if (l->NLc) {
        rc = gnn_launch_spmm(l->stream, g->n_rows, g->sh->indptr, g->sh->adj_src, g->sh->adj_w, g->nodes, g->NL, g->NL,
                             l->inv + l->NLc, IW, nullptr, 1);
        if (rc) return rc;
        rc = gnn_launch_copy_cols(l->stream, g->n_rows, g->NL, g->nodes + (size_t)g->own_off * g->NL, g->NL, l->inv, IW, nullptr, 1);
        if (rc) return rc;
    }
    return GNN_OK;
}

// the kernel arguments that depend neither on the body nor on the launch geometry; split: arithmetic mode / tile layout
// seeded (label projection): the arguments of the shadow net over [state | aggregated state] - its images, no label columns - and the seed
static void fill_args(const gnn_loop *l, const FusedPlan &p, bool split, GnnFusedArgs &a, bool seeded = false)
{
    const gnn_graph *g = l->g;
    const gnn_mlp *m = seeded ? l->st->proj : l->st;
    const int nlc = seeded ? 0 : l->NLc, al = seeded ? 0 : g->AL, in_s = seeded ? 2 * l->Ds : l->in_s;
    a = GnnFusedArgs{};
    a.n_rows = g->n_rows; a.row_begin = l->own_off;     // replica row of the first owned row
    a.indptr = g->sh->indptr; a.adj_src = g->sh->adj_src; a.adj_w = g->sh->adj_w;
    a.inv = l->inv;
    a.state_bytes = (int64_t)l->N_pad * l->Ds * (int64_t)sizeof(float);
    const int pad = split ? p.pad : 0;
    a.Ds = l->Ds; a.NLc = nlc; a.AL = al; a.IW = 2 * nlc + al; a.in_s = in_s + pad; a.c_aggs = l->Ds + nlc + pad;
    if (seeded) { a.seed = l->proj; a.seed_nt = p.nt[0]; }
    a.KP = split ? p.KPs : p.KP; a.kk0 = p.kk0;
    a.vec = (l->Ds % 4 == 0) ? 4 : 1;
    int lpr = 1, lg = 0;
    while ((lpr * a.vec < l->Ds || lpr < 2) && lpr < 64) { lpr <<= 1; ++lg; }
    a.lpr = lpr; a.lpr_log2 = lg;
    for (int i = 0; i < p.layers; ++i) {
        a.Wp[i] = m->packed + p.w_off[i];
        a.bias[i] = m->packed + p.b_off[i];
    }
    for (int i = 0; i < p.layers; ++i) a.Ws[i] = m->packed_split + p.s_off[i];
    a.chunks0 = p.chunks[0];
    a.Ws_base = m->packed_split;
    a.ws_bytes = (int)(p.s_total * sizeof(uint32_t));
    // piece format (gnn_loop_set_pieces): the image of the format, and in format 2 the scales of every layer's accumulator, 2^(e_w + e_x)
    a.pieces = l->pieces == 2 ? 2 : 3;
    for (int i = 0; i < p.layers; ++i) {
        a.ws_off[i] = (int)((a.pieces == 2 ? p.h_off[i] : p.s_off[i]) * sizeof(uint32_t));
        const int e = a.pieces == 2 ? m->split_exp[i] + GNN_F16_EX : 0;
        a.bsc[i] = std::ldexp(1.0f, e);
        a.usc[i] = std::ldexp(1.0f, -e);
    }
    a.variant = GNN_FUSED_VARIANT_DEFAULT;
    a.bn_scale = m->has_bn ? m->packed + p.bn_off : nullptr;
    a.bn_shift = m->has_bn ? m->packed + p.bn_off + 32 * p.NTL : nullptr;
    a.thr = l->thr;
    a.world = l->world;
    a.certify = split ? 1 : 0;
    a.agg_in = l->slice_mode ? l->agg_own : nullptr;
    a.wstride = 1;
    a.act_last = p.act_last;
}

// the five fields of the arguments that depend on the body
static void body_args(const gnn_loop *l, int k, GnnFusedArgs &a)
{
    const int cur = k & 1, P = l->world;
    a.state_cur = gnn_loop_state_after(l, k, 0);         // (body 0 of a one-GPU run gathers from state_init itself)
    a.state_nxt = l->state[cur ^ 1] + (size_t)l->own_off * l->Ds;
    a.gate = l->flags + (size_t)k * P * GNN_FLAG_WORDS;
    a.flag_out = l->flags + ((size_t)(k + 1) * P + l->rank) * GNN_FLAG_WORDS;
    a.tile_ctr = l->tile_ctr + k;
}

// geometry of a run with one launch per body: grid, LDS, start-up spread, and what the recorded kernel takes beyond the common arguments
static void decide_bodies(const gnn_loop *l, LoopForm &f, int n_cu)
{
    const gnn_graph *g = l->g;
    const FusedPlan &p = f.plan;
    GnnFusedArgs &a = f.args;
    fill_args(l, p, f.split, a, f.seeded);
    const size_t n_tiles = (size_t)((g->n_rows + 31) / 32);
#ifdef GNN_DIAG   // diagnostic build only (make DIAG=1): timing experiments; never in the shipped library
    static const int variant_env = getenv("GNN_FUSED_VARIANT") ? atoi(getenv("GNN_FUSED_VARIANT")) : GNN_FUSED_VARIANT_DEFAULT;
    a.variant = variant_env;
    static const int debug = getenv("GNN_FUSED_DEBUG") ? atoi(getenv("GNN_FUSED_DEBUG")) : 0;
    a.wstride = (debug & 1) ? 0 : 1;                                  // 0: every K-step re-reads step 0 (results meaningless)
#endif
    // one workgroup per CU; small graphs spread their tiles over as many CUs as they have tiles (a tile alone on a CU runs
    // faster than eight sharing its L1 / LDS / SIMDs; the waves without a tile leave at once)
    unsigned grid = (unsigned)std::min<size_t>((size_t)n_cu, n_tiles);
    // test entry point (gnn_loop_set_grid_limit): fewer workgroups, so that a few hundred rows reach a wave's second static tile and the
    // ticket counter; the spread and the ticket fields below follow the capped grid
    if (l->grid_limit > 0 && f.kernel == GNN_BODY_GENERIC) grid = std::min(grid, (unsigned)l->grid_limit);
    const size_t waves = (size_t)f.waves;                             // per workgroup of this launch: eight, fewer in the wide-state form
    int stagger_rounds = GNN_FUSED_SPREAD_DEFAULT;
#ifdef GNN_DIAG
    static const int stagger_env = getenv("GNN_FUSED_STAGGER") ? atoi(getenv("GNN_FUSED_STAGGER")) : GNN_FUSED_SPREAD_DEFAULT;   // tuning experiments
    stagger_rounds = stagger_env;
#endif
    // start-up spread (k_fused): the full amount when every wave has four or more tiles; the small one between one and four tiles per wave
    // (tools/bench_midsize.py, profiles/r04_midsize.txt); none when no wave has a second tile
    a.stagger = n_tiles >= 4 * waves * grid ? stagger_rounds : (n_tiles > waves * grid ? GNN_FUSED_SPREAD_SMALL_DEFAULT : 0);
#ifdef GNN_DIAG      // experiment: small grids (1 - 4 tiles per wave) with the two-cluster offset (variant bit 2): waves 4-7 start GNN_FUSED_STAGGER_SMALL x 8k cycles late
    static const int stagger_small = getenv("GNN_FUSED_STAGGER_SMALL") ? atoi(getenv("GNN_FUSED_STAGGER_SMALL")) : 0;
    const bool small_grid = n_tiles > waves * grid && n_tiles < 4 * waves * grid;
    if (small_grid && stagger_small > 0) { a.stagger = stagger_small; a.variant |= 4; }
    static const int spread_small = getenv("GNN_FUSED_SPREAD_SMALL") ? atoi(getenv("GNN_FUSED_SPREAD_SMALL")) : -1;      // ... or the hashed spread 0 .. n rounds
    if (small_grid && spread_small >= 0) a.stagger = spread_small;
#endif
    // fewer tiles than waves: a wave that drew two tickets at start would run two tiles one after the other while another wave of the
    // launch gets none (N = 31k: 488 of 2,048 waves did all the work) - the look-ahead ticket is only drawn when every wave has a tile
    a.single_ticket = n_tiles <= waves * grid ? 1 : 0;
    f.grid = grid;
    f.lds = lds_bytes(p, f.waves);
    if (f.wide) {
        a.threads = 64 * f.waves;
        // the wide-row loader on the full tiles, unless the aggregate is given or the loop asks for load_tile_generic (gnn_loop_set_wide_loader)
        if (!a.agg_in && l->wide_loader == 0) a.variant |= 8;
    }
    if (f.kernel == GNN_BODY_PAIR) {
        // wave-pair form: four pairs per workgroup, one workgroup per CU; the tile counters, gates and flags are k_fused's
        const int64_t n_tiles64 = (int64_t)n_tiles;
        a.KP = pair_xs(p);
        a.full_tiles = 1;
        f.grid = (unsigned)std::min<int64_t>((int64_t)n_cu, (n_tiles64 + 3) / 4);
        a.stagger = n_tiles64 >= (int64_t)4 * 4 * f.grid ? stagger_rounds : (n_tiles64 > (int64_t)4 * f.grid ? GNN_FUSED_SPREAD_SMALL_DEFAULT : 0);
        f.lds = pair_lds_bytes(p);
    } else if (f.kernel == GNN_BODY_FULL_TILE) {
        // k_fused_full (none of the generic paths compiled in) on every tile; a partial last tile takes a wave-uniform
        // branch with masked row stores / condition votes (the row buffers are padded to whole tiles, rows past n_rows have no arcs)
        a.full_tiles = 1;
        if (f.program) {
            a.gp_hdr = g->sh->gp_hdr; a.gp_ent = g->sh->gp_ent; a.gp_tiles = (int)g->sh->gp_tiles;
            a.gp_last_first = g->sh->gp_last_first; a.gp_last_nb = g->sh->gp_last_nb;
            a.gp_slot = g->sh->gp_slot[f.schedule == 2 ? 1 : 0]; a.gp_slots = (int)g->sh->gp_cost.size();
        }
    }
    // the instantiation's form.  A program without a full tile (a graph of fewer than 32 rows) is not gathered from: the launch walks the CSR
    f.launch.full = f.kernel == GNN_BODY_FULL_TILE;
    f.launch.given = f.launch.full && a.agg_in != nullptr;
    f.launch.program = f.launch.full && f.program && g->sh->gp_tiles > 0;
    f.launch.entries = g->sh->gp_entries == 4 ? 4 : 8;
    f.launch.pieces = f.pieces;
    f.launch.seed = f.seeded;
    a.lds_floats = gnn_poison_enabled() ? (int)(f.lds / sizeof(float)) : 0;
}

// geometry and control block of the persistent small-graph loop (device code: gnn_small_common.h, gnn_small_kernel.h, gnn_small16_kernel.h)
static int decide_persistent(gnn_loop *l, LoopForm &f, const SmallForm &sf)
{
    const gnn_graph *g = l->g;
    const FusedPlan &p = f.plan;
    GnnFusedArgs &a = f.args;
    fill_args(l, p, false, a);                                        // exact f32-MFMA arithmetic, unpadded tile layout; no gates, no tickets
    a.state_cur = l->state[0];
    a.state_nxt = l->state[1] + (size_t)l->own_off * l->Ds;
    GnnSmallCtl &c = f.ctl;
    c.state0 = l->state[0]; c.state1 = l->state[1];
    c.init = l->D ? l->state_init : g->nodes + (size_t)g->own_off * g->NL;      // D == 0: NL == Ds (GNN.py:265)
    c.kfinal = l->kfinal_dev;
    c.host_result = l->kfinal_host;                                   // pinned, device-visible: no copy back
    // tile rows, narrow or wide, and the layer-0 K-steps the kernel keeps in registers: small_form's
    bool tile16 = sf.tile == 16;
    f.small_wide = sf.wide;
    if (tile16) f.s0 = sf.steps; else f.kk_small = sf.steps;
#ifdef GNN_DIAG
    static const int tile_env = getenv("GNN_SMALL_TILE") ? atoi(getenv("GNN_SMALL_TILE")) : 0;
    if (tile_env == 32 && !sf.wide) {                                // (the 32-node form of the same net, for comparison)
        tile16 = false;
        f.kk_small = small_form(l->st, p, 16 * 256 + 1).steps;
    }
#endif
    f.small_tile = tile16 ? 16 : 32;
    f.grid = (unsigned)((g->n_rows + f.small_tile - 1) / f.small_tile);
    c.DP = l->Ds <= 16 ? 16 : 32;
    {   // padded exchange rows: allocated with the first persistent form of the loop, never initialised (every row is written before it is read)
        const size_t need = (size_t)2 * f.grid * f.small_tile * c.DP;
        if (l->small_xs_floats < need) {
            if (l->small_xs) (void)hipFree(l->small_xs);
            l->small_xs = nullptr; l->small_xs_floats = 0;
            HIPCHK(gnn_dev_malloc((void **)&l->small_xs, need * sizeof(float)));
            l->small_xs_floats = need;
        }
        c.xs = l->small_xs;
    }
    c.max_iter = l->max_iter;
    c.ecache = GNN_SMALL_ECACHE;
#ifdef GNN_DIAG
    static const int ecache_env = getenv("GNN_SMALL_ECACHE") ? atoi(getenv("GNN_SMALL_ECACHE")) : GNN_SMALL_ECACHE;
    c.ecache = std::min(GNN_SMALL_ECACHE, ecache_env);
#endif
    c.n_words = (int)(((size_t)l->max_iter + 3 + 3) & ~(size_t)3);      // gate of every body, + 1, + the barrier in front of the folded graph readout
    // output stage inside the launch when it is the usual one-layer head (same condition as k_out1)
    const gnn_mlp *ou = l->ou;
    if (!l->edge_mode && g->n_masked && ou->n_layers == 1 && l->T <= 8 && l->Ds + l->NLc <= 64 && l->Ds <= 32 && g->NL <= 32) {
        c.out = l->out; c.mask = g->sh->mask; c.mask_pos = g->sh->masked_rows + g->n_masked;
        c.nodes_own = g->nodes + (size_t)g->own_off * g->NL;
        c.ow = ou->W[0]; c.ob = ou->b[0];
        c.obn_scale = ou->has_bn ? ou->bn_scale : nullptr; c.obn_shift = ou->has_bn ? ou->bn_shift : nullptr;
        c.NL = g->NL; c.NLc = l->NLc; c.T = l->T; c.oact = ou->acts[0];
        f.fold_output = true;
        // graph readout in the same launch when a NodeGraph is already cached with the loop (gnn_loop_readout uploaded it after an earlier run)
        if (l->ng_ip && l->ng_G > 0 && g->n_masked == g->n_rows) {
            if (l->ng_host_floats < l->ng_G * l->T) {
                if (l->ng_host) (void)hipHostFree(l->ng_host);
                l->ng_host = nullptr; l->ng_host_floats = 0;
                if (hipHostMalloc((void **)&l->ng_host, sizeof(float) * (size_t)l->ng_G * l->T) == hipSuccess) l->ng_host_floats = l->ng_G * l->T;
            }
            if (l->ng_host) {
                c.ng_ip = l->ng_ip; c.ng_node = l->ng_node; c.ng_w = l->ng_w; c.ng_host = l->ng_host; c.G = l->ng_G; c.ro_word = l->max_iter + 1;
                f.fold_readout = true;
            }
        }
    }
    c.rnd = g->sh->max_degree > 8 ? 8 : 4;                       // entries per gather round
    if (tile16) {
        const gnn_mlp *m = l->st;
        for (int q = 0; q < p.layers; ++q) { c.Wraw[q] = m->W[q]; c.din[q] = m->dims[q]; c.dout[q] = m->dims[q + 1]; }
        c.KP16 = std::max((a.in_s + 3) / 4 * 4, 4 * f.s0);
        if (c.KP16 % 8 == 0) c.KP16 += 4;                            // rows 16 bytes apart in the banks: the B-operand column reads do not conflict
        f.lds = sf.wide ? GnnSmallLds<16, true>::bytes(c.KP16) : GnnSmallLds<16>::bytes(c.KP16);
    } else
        f.lds = GnnSmallLds<32>::bytes(p.KP);
    a.lds_floats = gnn_poison_enabled() ? (int)(f.lds / sizeof(float)) : 0;
    return GNN_OK;
}

// The launch form of the loop's next run (LoopForm, gnn_fused.h), from the loop's settings as they are now.
//
// Per-body kernel of the default path, the library's choice (gnn_loop_set_tile_form(l, 0)): the wave pair while no pair of the launch gets a
// second tile (tiles <= 4 x CUs: the launch is one tile latency long and a pair's tile takes about half as long as a wave's: N = 4 k .. 32 k:
// 7 - 11 % less time per iteration), one wave per tile beyond (N = 41 k: +13 %, BASELINE size: 0.78 against 0.68 ms - the seven meetings of
// a pair per tile cost more than its shorter matrix phases return; profiles/r05_midsize_forms.txt, r05_pair_stamps.txt).  The pair exists for
// nets with one activation for all layers (pair_covers): a net whose last layer has its own takes one wave per tile there too.
// Gather form (gnn_loop_set_gather_form): the bodies read the graph's program when the launch is k_fused_full and gathers
// (state width 64, a net with a 64-wide last layer, no feature-sliced exchange, not the wave pair) and the graph has a program - it is
// built here, on first demand.
int gnn_loop_decide_form(gnn_loop *l)
{
    LoopForm &f = l->form;
    f = LoopForm{};
    if (l->impl_req < 1) return GNN_OK;
    HIPCHK(hipSetDevice(l->device));
    int base_wide = 0;                                                // waves of the wide-state form of the net as it stands, or 0
    const bool base_ok = gnn_fused_supported(l, f.plan, base_wide);   // (side effect 1: the weight images)
    const gnn_graph *g = l->g;
    // small graphs: the initial state, the first condition and every body inside ONE persistent launch - nets no wider than 32 (one
    // 32-feature tile per layer) or, up to 4,096 rows, with hidden layers up to 64 wide (small_form), layer-0 weights kept in registers,
    // every tile resident at once (one wave each) with a wide margin
    const SmallForm sf = base_ok ? small_form(l->st, f.plan, g->n_rows) : SmallForm{};
    const bool persistent = base_ok && l->world == 1 && !l->small_disabled && !l->profiling && sf.tile != 0;
    // Label projection (gnn_loop_set_label_projection): impl 2 with one launch per body only - mode 1 where the net as it stands is not
    // covered and the net over [state | aggregated state] is, mode 2 wherever that one is.  Not the feature-sliced exchange (no seeded
    // instantiation with a given aggregate), not the persistent small-graph loop and not impl 1 (exact arithmetic: they stay as they are).
    if (l->label_projection && l->impl_req == 2 && !persistent && !l->slice_mode && (l->label_projection == 2 || !base_ok) && g->n_rows > 0 &&
        (int64_t)l->N_pad * l->Ds * (int64_t)sizeof(float) < ((int64_t)1 << 31)) {
        // Both forms on: a shadow plan that needs the wide-state form too is taken where the net as it stands has no wide-state form of
        // its own, or where the projection is asked for wherever it applies (mode 2).
        FusedPlan sp;
        int sw = 0;
        if (projection_plan(l->st, l->Ds, l->NLc, g->AL, sp, l->wide_state, g->n_rows, &sw) &&
            (sw == GNN_FUSED_WAVES || !base_wide || l->label_projection == 2)) {
            const int rcp = projection_ensure(l->st, l->Ds, l->NLc, g->AL, sp);      // (side effect 1b: the shadow net's images, the label rows of W1)
            if (rcp) return rcp;
            f.plan = sp;
            f.seeded = true;
            f.waves = sw;
        }
    }
    // Wide-state form (gnn_loop_set_wide_state) of the net as it stands: either impl, any exchange - with the feature-sliced one the
    // aggregate is given and the tile load is load_tile_generic's
    if (!base_ok && !f.seeded && base_wide) f.waves = base_wide;
    f.wide = f.waves != GNN_FUSED_WAVES;
    if (!base_ok && !f.seeded && !f.wide) return GNN_OK;
    if (l->device < 0 || l->device >= 64) return gnn_fail(GNN_ERR_ARG, "device %d out of range", l->device);
    const FusedPlan &p = f.plan;
    const int n_cu = device_cus(l->device);
    const int64_t n_tiles = (g->n_rows + 31) / 32;
    f.split = l->impl_req == 2;
    f.pieces = l->pieces == 2 ? 2 : 3;
    const bool pair = !f.seeded && f.split && !l->slice_mode && pair_covers(p, l->Ds) && pair_lds_bytes(p) <= 160 * 1024 &&
                      (l->tile_form ? l->tile_form == 2 : n_tiles <= (int64_t)4 * n_cu);
    f.kernel = pair ? GNN_BODY_PAIR : (l->Ds == 64 && p.NTL == 2 ? GNN_BODY_FULL_TILE : GNN_BODY_GENERIC);
    if (f.kernel == GNN_BODY_FULL_TILE && !l->slice_mode && (l->gather_form ? l->gather_form : GNN_GATHER_FORM_DEFAULT) == 2 &&
        gnn_gather_program_ensure(g) == GNN_OK)                       // (side effect 2: the graph's gather program)
        // the program kernel has no CSR walk: every tile of the launch must be a tile of the program.  A launch covers the rows [0, n_rows)
        // of its graph from tile 0 (tile_base stays 0), so it can only end inside the graph's last tile when it has the rows the program was
        // built for - a graph that shares the arrays but not the row count keeps form 1.
        f.program = g->sh->gp_ent != nullptr && g->sh->gp_rows == g->n_rows;
    if (f.program) {
        // tile schedule (gnn_loop_set_tile_schedule): the balanced order where it is asked for, or where the choice is the library's and
        // every wave of a launch on this device has four tiles or more; its slot headers are built here, on first demand
        const int64_t waves = (int64_t)f.waves * n_cu;                 // (the program kernel is k_fused_full: eight)
        const int want = l->tile_schedule ? l->tile_schedule : (n_tiles >= 4 * waves ? GNN_TILE_SCHEDULE_DEFAULT : 1);
        f.schedule = want == 2 && gnn_tile_schedule_ensure(g, 1, waves) ? 2 : 1;
    }
    f.path = persistent ? GNN_PATH_PERSISTENT : GNN_PATH_BODIES;
    // (side effect 3: the label block - the arguments point to it; gnn_fused_prepare zeroes and fills it when the loop runs)
    if (!l->inv) HIPCHK(gnn_dev_malloc((void **)&l->inv, inv_floats(l) * sizeof(float)));
    if (f.seeded) {                                                   // (side effect 4: the projection's block, whole row and feature tiles)
        const size_t need = (size_t)n_tiles * p.nt[0] * 1024;
        if (l->proj_floats != need || l->proj_nt != p.nt[0]) {
            if (l->proj) (void)hipFree(l->proj);
            l->proj = nullptr; l->proj_floats = 0;
            HIPCHK(gnn_dev_malloc((void **)&l->proj, need * sizeof(float)));
            l->proj_floats = need; l->proj_nt = p.nt[0];
            l->proj_labels = 0;
        }
    }
    if (persistent) return decide_persistent(l, f, sf);
    decide_bodies(l, f, n_cu);
    return GNN_OK;
}

// the recorded per-body kernel; false: no instantiation
static bool launch_body(const LoopForm &f, const GnnFusedArgs &a, hipStream_t st)
{
    const FusedPlan &p = f.plan;
    if (f.seeded)                                                     // label projection: split arithmetic, never the wave pair; the last activation from a.act_last
        return p.layers == 1 ? gnn_fused_launch_ps1(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st)
             : p.layers == 2 ? gnn_fused_launch_ps2(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st)
                             : gnn_fused_launch_ps3(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st);
    if (p.act_last != p.act) {                                        // the last layer's own activation: a.act_last (never the wave pair)
        if (f.kernel == GNN_BODY_PAIR || p.layers < 2) return false;
        if (f.split) return p.layers == 2 ? gnn_fused_launch_ms2(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st) : gnn_fused_launch_ms3(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st);
        return p.layers == 2 ? gnn_fused_launch_ml2(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st) : gnn_fused_launch_ml3(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st);
    }
    if (f.kernel == GNN_BODY_PAIR)
        return p.layers == 2 ? gnn_fused_launch_p2(p.act, f.pieces, a, f.grid, f.lds, st) : gnn_fused_launch_p3(p.act, f.pieces, a, f.grid, f.lds, st);
    if (f.split) {
        if (p.layers == 1) return gnn_fused_launch_s1(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st);
        if (p.layers == 2) return gnn_fused_launch_s2(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st);
        return gnn_fused_launch_s3(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st);
    }
    if (p.layers == 1) return gnn_fused_launch_l1(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st);
    if (p.layers == 2) return gnn_fused_launch_l2(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st);
    return gnn_fused_launch_l3(p.act, p.NT, p.NTL, f.launch, a, f.grid, f.lds, st);
}

// body k of a run whose form is one launch per body
int gnn_fused_iteration(gnn_loop *l, int k)
{
    const LoopForm &f = l->form;
    GnnFusedArgs a = f.args;
    body_args(l, k, a);
#ifdef GNN_DIAG   // diagnostic build only (make DIAG=1): per-wave phase stamps of body 1; never in the shipped library
    static const char *stamp_file = getenv("GNN_FUSED_STAMPS");
    static unsigned long long *stamp_buf = nullptr;
    const size_t n_waves = (size_t)((l->g->n_rows + 31) / 32);
    if (stamp_file && k == 1) {
        if (!stamp_buf) HIPCHK(gnn_dev_malloc((void **)&stamp_buf, n_waves * 16 * sizeof(unsigned long long)));      // (8 slots per tile: k_fused; 16: k_fused_pair)
        HIPCHK(hipMemsetAsync(stamp_buf, 0, n_waves * 16 * sizeof(unsigned long long), l->stream));
        a.stamps = stamp_buf;
    }
#endif
    const FusedPlan &p = f.plan;
    if (!launch_body(f, a, l->stream))
        return gnn_fail(GNN_ERR_UNSUPPORTED, "no fused instantiation for %d layers, tiles (%d,%d), activations %d / %d", p.layers, p.NT, p.NTL, p.act, p.act_last);
#ifdef GNN_DIAG
    if (a.stamps) {
        std::vector<unsigned long long> host(n_waves * (f.kernel == GNN_BODY_PAIR ? 16 : 8));
        HIPCHK(hipStreamSynchronize(l->stream));
        HIPCHK(hipMemcpy(host.data(), stamp_buf, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE *f_ = fopen(stamp_file, "wb")) { fwrite(host.data(), sizeof(unsigned long long), host.size(), f_); fclose(f_); }
    }
#endif
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// persistent small-graph loop (device code: gnn_small_common.h, gnn_small_kernel.h, gnn_small16_kernel.h)
// ---------------------------------------------------------------------------------------------------------------------
int gnn_small_run(gnn_loop *l)
{
    const LoopForm &f = l->form;
    const FusedPlan &p = f.plan;
    GnnFusedArgs a = f.args;
    GnnSmallCtl c = f.ctl;
    // Gate words: one per body, double-buffered by run parity at the start of the flag block.  This launch polls its own half
    // and zeroes the other half for the next run, so a run costs no memset; both halves are cleared by the host only after
    // something else (a per-body run) has used the block.
    const size_t n_words = (size_t)c.n_words;
    l->kfinal_host[1] = 0;                                            // status: cleared HERE, only ever set by the kernel (sticky)
    if (!l->small_words_clean) {
        HIPCHK(hipMemsetAsync(l->flags, 0, sizeof(int) * 2 * n_words, l->stream));
        l->small_words_clean = true;
        l->small_runs = 0;
    }
    c.flags = l->flags + (l->small_runs & 1) * n_words;
    c.zero_words = l->flags + ((l->small_runs & 1) ^ 1) * n_words;
    ++l->small_runs;
    l->ng_inlaunch = f.fold_readout;                                  // (cleared again by run_loops if the launch gives up)
    if (f.fold_readout) l->ng_inlaunch_run = l->out_runs;             // ... and valid for THIS run's outputs only
#ifdef GNN_DIAG
    static const char *small_stamp_file = getenv("GNN_SMALL_STAMPS");
    static unsigned long long *small_stamp_buf = nullptr;
    if (small_stamp_file) {
        if (!small_stamp_buf) HIPCHK(gnn_dev_malloc((void **)&small_stamp_buf, 256 * sizeof(unsigned long long)));
        HIPCHK(hipMemsetAsync(small_stamp_buf, 0, 256 * sizeof(unsigned long long), l->stream));
        a.stamps = small_stamp_buf;
    }
#endif
    static GnnSmallLaunch *const launchers[3][2] = {{gnn_small_launch, gnn_small_launch_mixed},            // [32 / 16 / 16 wide][mixed]
                                                    {gnn_small16_launch, gnn_small16_launch_mixed},
                                                    {gnn_small16w_launch, gnn_small16w_launch_mixed}};
    const int tile_form = f.small_wide ? 2 : f.small_tile == 16 ? 1 : 0;
    if (!launchers[tile_form][p.act_last != p.act](p.layers, p.act, tile_form ? f.s0 : f.kk_small, a, c, f.grid, f.lds, l->stream))
        return gnn_fail(GNN_ERR_UNSUPPORTED, "no persistent-loop instantiation for %d layers, activations %d / %d", p.layers, p.act, p.act_last);
    HIPCHK(hipGetLastError());
#ifdef GNN_DIAG
    if (small_stamp_file) {
        unsigned long long host[256];
        HIPCHK(hipStreamSynchronize(l->stream));
        HIPCHK(hipMemcpy(host, small_stamp_buf, sizeof(host), hipMemcpyDeviceToHost));
        if (FILE *fs = fopen(small_stamp_file, "wb")) { fwrite(host, sizeof(unsigned long long), 256, fs); fclose(fs); }
    }
#endif
    return GNN_OK;      // k and the status word are written straight into the pinned host words
}
