// Host/device interface of the fused iteration kernel (gnn_fused_kernel.h).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int GNN_FUSED_MAXL = 3;
constexpr int GNN_FUSED_WAVES = 8;                 // waves per (persistent) workgroup; w and w + 4 share a SIMD
constexpr int GNN_FUSED_THREADS = 64 * GNN_FUSED_WAVES;
// fp16-piece format of the split arithmetic (gnn_fused_kernel.h): activations are cut at the fixed scale 2^GNN_F16_EX, and a scaled activation
// of magnitude >= GNN_F16_LIMIT (the largest finite fp16) sends the Loop back to the bf16-piece format
#define GNN_F16_EX 4
#define GNN_F16_LIMIT 65504.0f
// Source word of a gather-program entry: the byte offset of the neighbour's 256-byte state row (source id << 8; the replica is < 2 GiB by the
// fused path's precondition, gnn_loop_decide_form), in the low byte the tile-local row the entry belongs to and "this entry ends its row".
// GNN_GP_NOROW is an offset no replica reaches (any offset >= 2^31 would do; this one keeps the 16-byte access of the last lane, 0xfffffef0
// .. 0xfffffeff, clear of the 2^32 wrap): a raw buffer load past the descriptor's range returns zeros (padding, and the single entry of an
// empty row).  That such a load costs no memory fetch is the ISA's description of the range check, not something a counter run has shown.
#define GNN_GP_ROW_MASK 31u
#define GNN_GP_ROW_END 32u
#define GNN_GP_NOROW 0xfffffe00u
// Gather form of a k_fused_full instantiation (its PROG template parameter): the CSR walk, or the graph's program with 8-byte entries
// {source word, weight} or with 4-byte entries (the source word; one weight per tile-local row, gnn_gather_program_compact)
constexpr int GNN_PROG_NONE = 0, GNN_PROG_ENT8 = 1, GNN_PROG_ENT4 = 2;
// Last-layer activation of the kernels' ACTL template parameter for a net whose last layer has an activation of its own: "read
// GnnFusedArgs::act_last" (one instantiation per hidden activation serves all last activations).  Library-internal, not a gnn_activation.
constexpr int GNN_ACTL_FROM_ARGS = -1;

struct GnnFusedArgs {
    // graph
    int64_t n_rows, row_begin;
    const int32_t *indptr, *adj_src;
    const float *adj_w;
    const float *inv;        // [n_rows, IW] = [nodes | aggregated nodes | aggregated arcs] (label columns of the concat)
    // state
    const float *state_cur;  // [N_pad, Ds] all nodes
    float *state_nxt;        // owned rows
    int64_t state_bytes;     // size of the replica state_cur points to
    // shapes
    // in_s: columns of the LDS tile in use (concat width + alignment hole); c_aggs: first column of the aggregated-state block
    int Ds, NLc, AL, IW, in_s, c_aggs, KP, lpr, lpr_log2, vec, kk0;
    // layers: packed weights [kk][lane][tiles of the layer], biases padded to whole tiles
    const float *Wp[GNN_FUSED_MAXL];
    const float *bias[GNN_FUSED_MAXL];
    const float *bn_scale, *bn_shift;   // padded to whole tiles, or nullptr
    // control
    float thr;
    const int *gate;
    int *flag_out;
    int world;
    int certify;             // 1 (split arithmetic): also raise the "robust" / "borderline" words of the certified gate (gnn_flag_raise_certified)
    int *tile_ctr;           // device-wide tile counter of this iteration (zeroed at the start of gnn_loop_run)
    int wstride;             // 1 normally; 0 (GNN_FUSED_DEBUG=1, timing experiments only) makes every K-step re-read step 0
    int stagger;             // s_sleep(127) rounds the second half of the waves waits before its first tile
    // split arithmetic (impl 2): per layer the piece weight image [chunk][out tile][piece][lane][8 bf16 / fp16], and the number
    // of K = 16 chunks of layer 0
    const int *Ws[GNN_FUSED_MAXL];
    int chunks0;
    // piece format (gnn_loop_set_pieces): 3 = three bf16 pieces, 2 = two fp16 pieces.  Format 2 scales weights and activations by powers of
    // two: bsc[l] = 2^(e_w + e_x) multiplies layer l's bias where its accumulator starts, usc[l] = 2^-(e_w + e_x) undoes it (1 in format 3)
    int pieces;
    float bsc[GNN_FUSED_MAXL], usc[GNN_FUSED_MAXL];
    // the same image through one buffer descriptor: base pointer, size and the byte offset of every layer, so that the weight
    // loads of the unrolled layers are buffer_load(rsrc, lane * 16, scalar offset) without any per-load vector address arithmetic
    const int *Ws_base;
    int ws_bytes, ws_off[GNN_FUSED_MAXL];
    int tile_base;           // first tile of this launch (tickets count from it)
    int full_tiles;          // 1: state width 64 - launch the full-tile specialisation of the kernel (a partial last tile takes its masked branch)
    int variant;             // tuning switches (bit 0: raised wave priority during the gather); fixed in the shipped build.  Bit 3: the wide-state form's full tiles through load_tile_wide
    // feature-sliced exchange: aggregated states of the owned rows [n_rows, Ds], computed outside the kernel (no gather), else nullptr
    const float *agg_in;
    // gather program of the graph (gnn_gather_program_build; gather form 2 of the full-tile kernel), or gp_tiles == 0: walk the CSR.
    // gp_hdr [gp_tiles][2] = {first batch, batches} of every full 32-row tile; gp_ent [batches][64][2] = {source word, weight} of lane
    // 16 g + j: entry j of lane group g in that batch, in the order the group consumes them
    // gp_last_first / gp_last_nb: the same header for tile gp_tiles, the partial last tile of the graph (gp_last_nb == 0: it has none);
    // host-side record only - the kernel reads every header, this one included, from gp_slot
    // gp_slot [gp_slots][4] = {first batch, batches, tile id, 0}: the program kernel's tile schedule (gnn_tile_schedule_build) - ticket s of
    // the launch stands for the tile of slot s, the partial last tile an ordinary slot; the program kernel reads its headers from here
    // Entry format 4 (GNN_PROG_ENT4 instantiations; gnn_gather_program_compact): gp_ent [batches][64] = the source words alone, and behind
    // gp_slot's headers [gp_slots][32] floats: the weight of every tile-local row of the slot's tile (all entries of a row share it)
    const int32_t *gp_hdr, *gp_ent, *gp_slot;
    int gp_tiles, gp_last_first, gp_last_nb, gp_slots;
    int threads;             // threads per workgroup of the launch (0: GNN_FUSED_THREADS); 256 .. 448 in the wide-state form of k_fused_generic
    int single_ticket;       // 1: the launch has no more tiles than waves - a wave draws ONE ticket at start (no look-ahead tile)
    // diagnostics only (GNN_FUSED_STAMPS=<file>): s_memtime stamps per wave at the phase boundaries, else nullptr
    unsigned long long *stamps;
    // diagnostics only (GNN_POISON=1, diagnostic build): floats of the launch's dynamic LDS allocation that every workgroup fills with NaN
    // before its first tile (a read of a never-written LDS word then shows as a NaN instead of a stale value), else 0
    int lds_floats;
    // activation of the last layer (gnn_activation, never softmax): read by the instantiations with ACTL == GNN_ACTL_FROM_ARGS only
    int act_last;
    // label projection (gnn_loop_set_label_projection), read by the seeded instantiations only: P = inv . W1_label + b1 of the owned rows,
    // unscaled fp32, in accumulator-tile order [row tile][seed_nt feature tiles][q][lane][4] (gnn_label_project.hip) - the four features
    // 32 jt + 8 q + 4 (lane >> 5) + 0..3 of node lane & 31, so that a register quad of a layer-0 accumulator tile is one 1 KiB wave load
    const float *seed;
    int seed_nt;
};

// control block of the persistent small-graph loop (gnn_small_common.h)
struct GnnSmallCtl {
    float *state0, *state1;  // the two state replicas (ping-pong), all rows
    const float *init;       // initial state of the owned rows [n_rows, Ds] (injected / drawn state, or the node labels for D == 0)
    int *kfinal;             // receives the number of executed bodies
    int *flags;              // word [b]: barrier + gate of body b (low half arrivals, high half movers), zeroed before the launch
    int *host_result;        // pinned host memory (zero-copy): [k, status]; status: set to 1 by a workgroup whose barrier spin gave up, never cleared by the
                             // kernel (sticky), zeroed by the host before the launch
    float *xs;               // padded exchange rows [2][tiles * rows per tile][DP] (gnn_small_common.h, small_gather): the state between bodies
    int DP;                  // 16 (Ds <= 16) or 32 floats per exchange row
    int rnd;                 // arcs per gather round for DP == 16 (4, or 8 when some row has more than 8 arcs)
    // 16-node-tile form (gnn_small16_kernel.h): the Keras-layout kernels W[din][dout] (its A operands are read from them directly) and the
    // row stride of its LDS tile
    const float *Wraw[GNN_FUSED_MAXL];
    int din[GNN_FUSED_MAXL], dout[GNN_FUSED_MAXL];
    int KP16;
    int *zero_words;         // the OTHER run's gate words (double-buffered by run parity): zeroed here for the next run
    int n_words;
    int max_iter;
    // output stage folded into the launch (apply_filters + a one-layer net_output, GNN.py:275-279; as k_out1), or out == nullptr
    float *out;              // [n_masked, T]
    const uint8_t *mask;     // [n_rows]
    const int32_t *mask_pos; // [n_rows] position of a masked row among the masked rows
    const float *nodes_own;  // node labels of the owned rows [n_rows, NL]
    const float *ow, *ob, *obn_scale, *obn_shift;   // net_output: W [wf, T], b [T], BatchNormalization scale / shift or nullptr
    int NL, NLc, T, oact;
    // graph readout folded into the launch (NodeGraph^T . out, GNN.py:331-332; as k_readout), or ng_ip == nullptr: CSR over graphs of
    // (node, weight), result [G, T] written to pinned host memory by workgroup 0 after one more grid barrier (word ro_word of `flags`)
    const int32_t *ng_ip, *ng_node;
    const float *ng_w;
    float *ng_host;
    int G, ro_word;
    int ecache;              // arcs of a tile whose ids / weights may be kept in LDS (GNN_SMALL_ECACHE; 0: none)
};

// Layout of a net_state's packed weight images and of the kernels' LDS tile (gnn_fused.hip, make_plan): a function of the net's widths and
// activations and of the loop's node-label columns alone.
struct FusedPlan {
    int layers = 0, NT = 0, NTL = 0, KP = 0, kk0 = 0;
    int act = 0, act_last = 0;       // activation of the hidden layers (one for all of them) / of the last layer; one layer: the same
    // split arithmetic, state width 64 (the tuned shape): the LDS tile is laid out for 16-byte accesses - rows 16-byte aligned
    // (KPs a multiple of 4 with KPs / 4 odd: ds_read_b128 down a column stays bank-conflict free) and the aggregated-state block
    // starting on a multiple of 4 columns, i.e. after a hole of `pad` zero columns behind [state | nodes]
    int pad = 0, KPs = 0;
    int nt[GNN_FUSED_MAXL] = {0, 0, 0};       // tiles of each layer's output
    int kk[GNN_FUSED_MAXL] = {0, 0, 0};       // K-steps of each layer
    size_t w_off[GNN_FUSED_MAXL] = {0, 0, 0}, b_off[GNN_FUSED_MAXL] = {0, 0, 0}, bn_off = 0, total = 0;
    // split arithmetic (impl 2): K = 16 chunks per layer and the dword offsets of the piece images, bf16 x 3 (s_off) and fp16 x 2 (h_off),
    // one after the other in one buffer
    int chunks[GNN_FUSED_MAXL] = {0, 0, 0};
    size_t s_off[GNN_FUSED_MAXL] = {0, 0, 0}, h_off[GNN_FUSED_MAXL] = {0, 0, 0}, s_total = 0;
};

// The launch form of one run of a Loop: everything about its launches that cannot change between the first body and the last.  Decided by
// gnn_loop_decide_form (gnn_fused.hip) in every loop_prepare - its inputs (the requested impl / pieces / tile form / gather form, the
// exchange layout, profiling, "the persistent loop gave up", the weights, the graph's labels) may all have changed since the last run, so
// nothing of it is kept from run to run - and by the setters, which answer `used` from it.
enum GnnLoopPath { GNN_PATH_UNFUSED = 0, GNN_PATH_BODIES = 1, GNN_PATH_PERSISTENT = 2 };      // one kernel per TF op / one launch per body / all bodies in one launch
enum GnnBodyKernel { GNN_BODY_GENERIC = 0, GNN_BODY_FULL_TILE = 1, GNN_BODY_PAIR = 2 };       // k_fused_generic / k_fused_full / k_fused_pair
// What the launchers of gnn_fused_kernel.h pick an instantiation by, beyond the net's shape.  Host side only: no kernel sees it.
// (GnnFusedArgs still carries full_tiles, gp_tiles and pieces, which no kernel and no launcher reads, beside six more unread fields -
// `threads` is the launcher's block size since the wide-state form -:
// taking fields out moves every kernel's argument offsets, and with them the register allocation of instantiations that stand at 256
// registers - three of them spilled, one k_small16 lost a wave of occupancy; profiles/fused_two_kernels.txt.)
struct GnnFusedLaunch {
    bool full = false;               // k_fused_full (state width 64) rather than k_fused_generic
    bool given = false;              // ... whose aggregate is given (GnnFusedArgs::agg_in: feature-sliced exchange): no gather
    bool program = false;            // ... or which gathers from the graph's program (gp_ent / gp_slot) rather than walking the CSR
    int entries = 8;                 // ... whose entries are 8 bytes {source word, weight} or 4 (source word; the weights per row behind gp_slot's headers)
    int pieces = 3;                 // piece format of the split arithmetic
    bool seed = false;               // the seeded instantiations (label projection): layer 0 over [state | aggregated state], started from GnnFusedArgs::seed
};
struct LoopForm {
    int path = GNN_PATH_UNFUSED;
    // the per-body kernel of a fused loop (on the persistent path: what a run with one launch per body would take; the setters report it)
    int kernel = GNN_BODY_GENERIC;
    bool split = false;              // split arithmetic (impl 2) rather than the exact f32 MFMA (impl 1)
    int pieces = 3;                  // piece format of the split arithmetic
    bool program = false;            // the full-tile kernel gathers from the graph's program
    bool seeded = false;             // label projection in use: plan and args are those of the shadow net over [state | aggregated state]
    bool wide = false;               // wide-state form (gnn_loop_set_wide_state): k_fused_generic on a workgroup of `waves` < 8 waves
    int waves = GNN_FUSED_WAVES;     // waves per workgroup of a launch per body
    int schedule = 0;                // ... working through its tiles in 1 ascending / 2 the balanced order (0: no program)
    // launch constants of the path's launches
    FusedPlan plan;
    unsigned grid = 0;
    size_t lds = 0;                  // dynamic LDS bytes
    GnnFusedLaunch launch;           // one launch per body, k_fused_generic / k_fused_full: the instantiation's form
    // every field that is constant for the run; a body sets state_cur, state_nxt, gate, flag_out and tile_ctr (the start-up spread and
    // single_ticket are in it).  Persistent path: the arguments of that launch (exact arithmetic, unpadded tile, no gates)
    GnnFusedArgs args;
    // persistent path: 16- or 32-node tiles, the instantiated layer-0 K-step count (kk_small of k_small_loop / s0 of k_small16), and
    // whether the output stage and the graph readout run inside the launch; ctl holds everything but the run-parity gate words
    int small_tile = 0, kk_small = 0, s0 = 0;
    bool small_wide = false;         // 16-node tiles with hidden layers up to 64 wide (k_small16 with WIDE)
    bool fold_output = false, fold_readout = false;
    GnnSmallCtl ctl;
};

// LDS layout of the persistent small-graph loop (gnn_small_common.h), in 4-byte words, for ROWS = 32 (k_small_loop) or 16 (k_small16, and
// with WIDE its form for hidden layers up to 64 wide) rows per tile: the tile [ROWS][KP] at the start of the dynamic allocation, everything
// else at the constant offsets below from the tile's end.  The kernels carve their pointers from it; the host sizes the allocation with
// bytes(KP).
constexpr int GNN_SMALL_ECACHE = 1024;             // arcs of a tile whose ids / weights are kept in LDS
constexpr int GNN_SMALL16_HP = 36;                 // row stride of k_small16's hidden-activation copy (floats): 16-byte rows, (4 n + g) banks
// Row stride of the wide k_small16's 64-feature hidden-activation copy (floats).  Lane (n = lane % 16, g = lane / 16) reads its B operand of K-step
// s from word 66 n + g + 4 s with ds_read_b32, whose bank is the word address mod 32 and whose conflict groups are the two 32-lane halves
// (g in {0, 1} and g in {2, 3}): 66 n + g = 2 n + g (mod 32) takes every value 0 .. 31 (2 .. 33) exactly once over the 32 lanes of a half,
// so a column read costs one LDS cycle per half.  64 + 4 would put nodes n and n + 8 on one bank.  Rows are 8-byte aligned: the copy is
// written with 8-byte stores.
constexpr int GNN_SMALL16W_HP = 66;
template <int ROWS, bool WIDE = false>
struct GnnSmallLds {
    static_assert(ROWS == 16 || ROWS == 32, "16- or 32-node tiles");
    static_assert(!WIDE || ROWS == 16, "the wide form works on 16-node tiles");
    static constexpr int H = 0;                                         // k_small16: hidden activations [16][GNN_SMALL16_HP / GNN_SMALL16W_HP]
    static constexpr int IPT = ROWS == 16 ? 16 * (WIDE ? GNN_SMALL16W_HP : GNN_SMALL16_HP) : 32;   // row pointers [ROWS + 1] (+3); k_small_loop: behind 32 words of slack
    static constexpr int EP = IPT + ROWS + 4;                           // last-layer bias, BatchNormalization scale / shift [3][32]
    static constexpr int HBW = WIDE ? 64 : 32;                          // floats per hidden layer's bias
    static constexpr int HB = EP + 96;                                  // biases of the hidden layers [2][HBW]
    static constexpr int HW = HB + 2 * HBW;                             // net_output head: W [wf * T <= 512], then b | BN scale | BN shift [3][8]
    static constexpr int SCR = HW + 544;                                // scratch: [ROWS][32] the tile's rows in [row][Ds] order (initial / final state),
    static constexpr int LABELS = 32 * ROWS;                            // ... then from scr + LABELS its label rows [ROWS][32]
    static constexpr int EC_SRC = SCR + 2 * LABELS;                     // the tile's arc ids / weights [GNN_SMALL_ECACHE] each, kept for every body
    static constexpr int EC_W = EC_SRC + GNN_SMALL_ECACHE;
    static constexpr int END = EC_W + GNN_SMALL_ECACHE + 4;
    static constexpr size_t bytes(int KP) { return sizeof(float) * ((size_t)ROWS * KP + END); }
};

// Instantiated K-step counts of layer 0 (the host picks the smallest that covers the concat width, the launcher dispatches on the same list)
template <int... V> struct GnnSteps { static constexpr int values[] = {V...}; };
using GnnSmallKK0 = GnnSteps<8, 12, 16, 24, 32, 36, 40, 48>;     // k_small_loop: K-steps of 2 (v_mfma_f32_32x32x2_f32)
using GnnSmall16S0 = GnnSteps<4, 8, 12, 16, 20, 24>;             // k_small16: K-steps of 4 (v_mfma_f32_16x16x4_f32)

// One launcher per translation unit gnn_small{,16,16w}{,_m}.hip: 32-node tiles, 16-node tiles, 16-node tiles with hidden layers up to 64
// wide (k_small16 with WIDE; layers 2 or 3); _mixed: the same kernels for a net whose last layer has its own activation (a.act_last;
// layers 2 or 3).  steps: kk0 of k_small_loop / s0 of k_small16.  false = no instantiation for (layers, act, steps)
typedef bool GnnSmallLaunch(int layers, int act, int steps, const GnnFusedArgs &a, const GnnSmallCtl &c, unsigned grid, size_t lds_bytes, hipStream_t st);
GnnSmallLaunch gnn_small_launch, gnn_small_launch_mixed, gnn_small16_launch, gnn_small16_launch_mixed, gnn_small16w_launch, gnn_small16w_launch_mixed;

// k_fused_generic / k_fused_full (how.full), one launcher per translation unit gnn_fused_l{1,2,3}.hip; false = no instantiation for (act, nt, ntl)
bool gnn_fused_launch_l1(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
// split-arithmetic instantiations: gnn_fused_s{1,2,3}.hip
bool gnn_fused_launch_s1(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
bool gnn_fused_launch_s2(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
bool gnn_fused_launch_s3(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
// wave-pair form (gnn_fused_pair_kernel.h: split arithmetic, state width 64, 128-wide hidden layers, 9 layer-0 chunks): gnn_fused_p{2,3}.hip
bool gnn_fused_launch_p2(int act, int pieces, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
bool gnn_fused_launch_p3(int act, int pieces, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
bool gnn_fused_launch_l2(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
bool gnn_fused_launch_l3(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
// the same two kernels for a net whose last layer has its own activation (act: the hidden layers'; a.act_last): gnn_fused_ml{2,3}.hip (exact),
// gnn_fused_ms{2,3}.hip (split)
bool gnn_fused_launch_ml2(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
bool gnn_fused_launch_ml3(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
bool gnn_fused_launch_ms2(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
bool gnn_fused_launch_ms3(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
// the seeded split-arithmetic instantiations (label projection; how.seed): one family per hidden activation, the last layer's activation from
// a.act_last whether it is the net's own or not: gnn_fused_ps{1,2,3}.hip
bool gnn_fused_launch_ps1(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
bool gnn_fused_launch_ps2(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
bool gnn_fused_launch_ps3(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st);
// P of n_rows rows in the layout of GnnFusedArgs::seed (gnn_label_project.hip): inv [rows padded to 32][IW], wl [IW + 1][32 nt] (last row zero) and bias [32 nt]
// (columns past H1 zero); every element of the padded P is written
int gnn_label_project_launch(hipStream_t st, int64_t n_rows, int IW, int nt, const float *inv, const float *wl, const float *bias, float *P);
