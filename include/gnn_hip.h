/*
 * gnn_hip.h - C ABI of the MI355X (gfx950) engine for the GNN fixed-point state-propagation loop.
 *
 * The reference (sailab-code/GNN_tf_2.x) has no FFI / plugin boundary: the path is Python calling TensorFlow ops
 * (SURVEY.md 8b).  The entry points below are what a binding for that path needs; each one names the reference
 * interface it replaces (paths relative to the reference root).  The reference-side ctypes stub is in INTEGRATION.md;
 * the Python mirror of the reference classes lives in gnn_tf_2.x_amd/GNN/.
 *
 * Conventions
 *   - every function returns 0 on success, a negative gnn_status otherwise; gnn_last_error() gives the text
 *     (thread-local, valid until the next failing call on the thread).  Nothing throws or aborts across the ABI.
 *   - host buffers are caller-owned, C-contiguous, float32 / int32 / uint8, and only read during the call;
 *     outputs are written into caller-allocated buffers.
 *   - device memory is owned by the handles (create .. destroy).  Handles are not thread-safe; different handles may
 *     be used from different host threads.  All work of a loop runs on that loop's HIP stream.
 *   - sparse operands are the TRANSPOSED, row-major reordered matrices of GraphTensor (GNN/graph_class.py:355-372)
 *     in CSR form "by destination node": one indptr shared by Adjacency^T (inner order: ascending source id) and
 *     ArcNode^T (inner order: ascending arc id).
 */
#ifndef GNN_HIP_H
#define GNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GNN_OK = 0,
    GNN_ERR_ARG = -1,      /* bad argument / inconsistent dimensions (reference: ValueError / TypeError) */
    GNN_ERR_HIP = -2,      /* HIP runtime error (no device, out of memory, launch failure) */
    GNN_ERR_STATE = -3,    /* call order (e.g. fetching results before gnn_loop_run) */
    GNN_ERR_COMM = -4,     /* RCCL error */
    GNN_ERR_UNSUPPORTED = -5
} gnn_status;

/* activation codes of Dense layers built by GNN/MLP.py:11-64 (Keras names) */
typedef enum {
    GNN_ACT_LINEAR = 0, GNN_ACT_RELU = 1, GNN_ACT_SELU = 2, GNN_ACT_ELU = 3,
    GNN_ACT_TANH = 4, GNN_ACT_SIGMOID = 5, GNN_ACT_SOFTMAX = 6
} gnn_activation;

typedef struct gnn_graph gnn_graph;   /* device-resident GraphTensor (GNN/graph_class.py:330-372) */
typedef struct gnn_mlp gnn_mlp;       /* device-resident Sequential built by GNN/MLP.py:11-64 */
typedef struct gnn_loop gnn_loop;     /* one configured GNN.Loop (GNN/GNN.py:251-280) with its workspaces */
typedef struct gnn_comm gnn_comm;     /* RCCL communicator for node-range sharding (no reference counterpart) */

const char *gnn_last_error(void);
int gnn_version(void);                               /* ABI version, currently 1 */
int gnn_device_count(int *count);                    /* number of visible HIP devices (0 is not an error) */
int gnn_device_synchronize(int device);

/* ---- graph ------------------------------------------------------------------------------------------------------
 * Replaces GraphTensor.__init__ / fromGraphObject (GNN/graph_class.py:331-363).
 *   n_nodes            N, global node count
 *   row_begin, n_rows  destination rows owned by this handle ([0, N) unless sharded across GPUs)
 *   indptr[n_rows+1]   CSR row pointers of the owned rows, indptr[0] == 0
 *   adj_src, adj_w     Adjacency^T entries of the owned rows: global source id and weight, ascending source id
 *   arc_w, arc_labels  ArcNode^T entries of the owned rows in ascending arc id order: weight and the arc's label
 *                      row arcs[arc, 2:] (already permuted into this order), [n_arcs, dim_arc_label]
 *   nodes              node labels of ALL N nodes [N, dim_node_label] (neighbour labels are aggregated, GNN.py:263)
 *   mask               set_mask & output_mask of the owned rows (GNN.py:275), uint8 [n_rows]
 */
int gnn_graph_create(int64_t n_nodes, int64_t row_begin, int64_t n_rows, int64_t n_arcs, const int32_t *indptr,
                     const int32_t *adj_src, const float *adj_w, const float *arc_w, const float *arc_labels,
                     int dim_arc_label, const float *nodes, int dim_node_label, const uint8_t *mask, int device,
                     gnn_graph **out);
/* Builds the same graph from its arc list on the device (replaces GraphObject.buildArcNode / buildAdiacency and
 * GraphTensor.COO2SparseTransposedTensor, reference GNN/graph_class.py:90-121, :365-372, for graphs where the host build
 * would take minutes): arc a goes from arc_src[a] to arc_dst[a] with labels arc_labels[a, :] (ORIGINAL arc order);
 * aggregation_mode 0 = 'sum', 1 = 'normalized' (1 / number of arcs), 2 = 'average' (1 / in-degree of the destination).
 * Two stable radix sorts give Adjacency^T (entries of a destination by ascending source) and ArcNode^T (by ascending arc
 * id).  Single GPU: the handle owns all rows.  The optional outputs (any may be NULL) return the host mirrors:
 * indptr [n_nodes + 1], adj_src / adj_w [n_arcs] in Adjacency^T order, arc_id / arc_w [n_arcs] in ArcNode^T order. */
int gnn_graph_create_from_arcs(int64_t n_nodes, int64_t n_arcs, const int32_t *arc_src, const int32_t *arc_dst,
                               const float *arc_labels, int dim_arc_label, int aggregation_mode, const float *nodes,
                               int dim_node_label, const uint8_t *mask, int device, gnn_graph **out,
                               int32_t *indptr_out, int32_t *adj_src_out, float *adj_w_out, int32_t *arc_id_out,
                               float *arc_w_out);
/* LGNN.update_graph (GNN/LGNN.py:227-260) for node/graph-based layers, on the device:
 * dst.nodes <- [base.nodes | state of `from` (if get_state) | scatter(mask, output of `from`) (if get_output)].
 * `dst` must have been created by gnn_graph_derive(base, extra) with extra = get_state*Ds + get_output*T. */
int gnn_graph_derive(const gnn_graph *base, int extra_node_label_dims, gnn_graph **out);
/* Sharded graphs: every rank relabels its own rows, then the new label rows are exchanged - whole shards (full-replica shards) or
 * the rank's boundary rows into its block (gnn_graph_create_halo shards) - RCCL communicator: call on every rank; loopback group:
 * gnn_graph_update_labels_group below.  A derived graph's labels are zero until then; that fill is ordered on the device before
 * whatever touches the labels first (no call waits for it on the host). */
int gnn_graph_update_labels(gnn_graph *dst, const gnn_graph *base, const gnn_loop *from, int get_state, int get_output);
/* Edge-based LGNN (reference GNN/LGNN.py:253-254: the output of an edge-based layer widens the ARC labels, its state the
 * node labels).  gnn_graph_set_arc_order gives the original graph what the arc side needs: arc_id [n_arcs] = arc of every
 * ArcNode^T entry (the permutation COO2SparseTransposedTensor applied) and the arc labels in ORIGINAL arc order.
 * gnn_graph_derive_edge is gnn_graph_derive with extra arc-label columns; gnn_graph_update_labels then fills node labels
 * [base | state?] and arc labels [base | scatter(out) over the arc mask?] when `from` is an edge-based loop, and loops
 * created on the derived graph read their per-arc readout labels from it (gnn_loop_set_edge_readout: arc_labels = NULL). */
int gnn_graph_set_arc_order(gnn_graph *g, const int32_t *arc_id, const float *arc_labels_orig);
int gnn_graph_derive_edge(const gnn_graph *base, int extra_nodes, int extra_arcs, gnn_graph **out);
int gnn_graph_get_nodes(const gnn_graph *g, float *nodes_out /* [N, dim_node_label] */);
int gnn_graph_dims(const gnn_graph *g, int64_t *n_nodes, int64_t *n_rows, int64_t *n_arcs, int *dim_node_label,
                   int *dim_arc_label, int64_t *n_masked);
int gnn_graph_destroy(gnn_graph *g);

/* ---- MLP --------------------------------------------------------------------------------------------------------
 * Replaces the Keras Sequential of GNN/MLP.py:62-64 at inference: Dense(act) x n_layers [+ BatchNormalization].
 * Weights in Keras get_weights() layout (GNN/GNN.py:163-165): W[l] row-major [dims[l], dims[l+1]], b[l] [dims[l+1]];
 * bn = [gamma | beta | moving_mean | moving_variance], each dims[n_layers] long, or NULL without BatchNormalization. */
int gnn_mlp_create(int n_layers, const int32_t *dims, const int32_t *acts, const float *const *W, const float *const *b,
                   const float *bn, float bn_eps, int device, gnn_mlp **out);
int gnn_mlp_set_weights(gnn_mlp *m, const float *const *W, const float *const *b, const float *bn);   /* GNN.py:168-172 */
int gnn_mlp_forward(gnn_mlp *m, int64_t n_rows, const float *x, float *y);
/* Sequential.get_weights(): W[l] [dims[l] x dims[l+1]], b[l] [dims[l+1]], bn [4 x width] = gamma | beta | moving_mean |
 * moving_variance (NULL without BatchNormalization); waits for the device first (a device-side optimizer step may be running) */
int gnn_mlp_get_weights(gnn_mlp *m, float *const *W, float *const *b, float *bn);
/* forget the slots (Adam moments / SGD velocity) of the device-side optimizer: a NEW optimizer object starts from zero, as a
 * tf.keras optimizer creates its slot variables on first use (reference starter.py:81) */
int gnn_mlp_reset_optimizer(gnn_mlp *m);   /* Sequential.__call__(x, training=False) */
int gnn_mlp_destroy(gnn_mlp *m);

/* ---- loop -------------------------------------------------------------------------------------------------------
 * Replaces GNNnodeBased.Loop (GNN/GNN.py:251-280): condition :202-220, convergence :223-242, apply_filters :245-248.
 *   state_dim      state_vect_dim (0: state is initialised with the node labels, GNN.py:265)
 *   max_iter, thr  max_iteration, state_threshold (GNN.py:61-62)
 * gnn_loop_set_state0: injected initial state [n_rows owned, state_dim] (the reference draws tf.random.normal(stddev=0.1),
 * GNN.py:262, whose stream cannot be reproduced); NULL draws N(0, 0.1^2) from the engine's own counter RNG with `seed`.  The loop keeps
 * the state in a table of its own, which only this call writes: on one GPU the first body of every later run reads it where it lies (no
 * run copies or modifies it), so it stays byte for byte what was set until the next gnn_loop_set_state0.
 * gnn_loop_run: runs the whole loop on the device.  Bodies are enqueued 16 at a time without waiting for them (a body whose gate is
 * closed returns at once); after each 16 the next body's gate is copied to the host, which looks at it four bodies later (those are
 * queued behind the copy first), so that a converged loop stops enqueuing, and it synchronises once at the end. Small graphs (all tiles resident, nets <= 32 wide) take ONE persistent launch for the whole loop,
 * the output stage and - once a NodeGraph is cached with the loop by an earlier gnn_loop_readout - the graph readout.  *k_out = number of executed iterations as float (GNN.py:267).  This is the
 * inference Loop (training=False); training != 0 is GNN_ERR_UNSUPPORTED here: the training-mode Loop and its backward pass
 * are gnn_loop_train_forward / gnn_loop_train_backward / gnn_loop_train_step below.
 */
int gnn_loop_create(gnn_graph *g, gnn_mlp *net_state, gnn_mlp *net_output, int state_dim, int max_iter, float threshold,
                    gnn_comm *comm /* NULL: single GPU */, gnn_loop **out);
int gnn_loop_set_state0(gnn_loop *l, const float *state0, uint64_t seed);
int gnn_loop_run(gnn_loop *l, int training, float *k_out);
/* n independent loops (the batches of a dataset, which GNN_BaseClass.evaluate - reference GNN_BaseClass.py:165-189 - runs one after the
 * other) in one call: the persistent launches of small graphs are all queued, each on its loop's stream, before the first is waited
 * for, and run side by side on the GPU; larger graphs run one after the other.  k_out [n]; results as of n gnn_loop_run calls. */
int gnn_loop_run_many(gnn_loop **loops, int n, float *k_out);
int gnn_loop_get_state(const gnn_loop *l, float *state_out /* [n_rows, Ds] */);
int gnn_loop_get_output(const gnn_loop *l, float *out /* [n_masked, T] */, int64_t *n_masked);
/* GNNgraphBased.Loop readout (GNN/GNN.py:331-332, LGNN.py:278): out_graph = NodeGraph^T . out_nodes.
 * NodeGraph^T is passed in CSR form over graphs: ng_indptr[G+1], ng_node (ascending), ng_w.  The arrays are kept with the loop (and
 * compared on every call): when the persistent small-graph launch of the last run has already computed the readout for the same
 * NodeGraph, the call only copies the result. */
int gnn_loop_readout(const gnn_loop *l, int n_graphs, const int32_t *ng_indptr, const int32_t *ng_node,
                     const float *ng_w, float *out_graph /* [G, T] */);
/* GNNedgeBased.apply_filters (GNN/GNN.py:289-302): switches the output stage of this loop to the per-arc readout.  Row e of
 * the readout is [F[i0(e)] | F[i1(e)] | arc_labels[e]] with F = [state | nodes (iff state_dim > 0)], (i0, i1) the e-th index
 * pair of the transposed, reordered Adjacency (i0 = entry_dst[e], the CSR row of entry e; i1 = adj_src[e]) and arc_labels in
 * ORIGINAL arc order: the reference pairs the two by position (consistent for symmetric, lexicographically sorted arc
 * lists; SURVEY.md 8a quirk 6, reproduced as is).  arc_mask = set_mask & output_mask over arcs.  net_output must take
 * 2 (NL [D>0] + Ds) + AL inputs (GNN/MLP.py:109).  Single GPU only. */
int gnn_loop_set_edge_readout(gnn_loop *l, const int32_t *entry_dst, const float *arc_labels, const uint8_t *arc_mask);
/* One training step without the optimizer (reference GNN/GNN_BaseClass.py:231-247: GradientTape around
 * evaluate_single_graph(training=True), GNN/GNN.py:180-199): training-mode forward through the unrolled loop (Dropout masks,
 * BatchNormalization batch statistics), loss = sum_i w_i L(t_i, out_i), back-propagation through every executed body.
 *   src_*            Adjacency in CSR form BY SOURCE (rows = source node, inner = destination ascending): the transposed
 *                    aggregation of the backward pass; all NULL = derived from the graph's own CSR on first use and kept
 *   targets, sample_weights, n_targets   rows = masked nodes (node-based) or graphs (graph-based); loss_kind 0 =
 *                    categorical_crossentropy(from_logits=False), 1 = mean_squared_error, 2 = categorical_crossentropy(from_logits=True)
 *                    3 = binary_crossentropy (probabilities p clipped to [1e-7, 1 - 1e-7], L = mean_j -(t log p + (1 - t) log(1 - p)), no
 *                    gradient where p was clipped, as kind 0), 4 = binary_crossentropy(from_logits=True) (L = mean_j max(z, 0) - z t +
 *                    log(1 + exp(-|z|)), d = (sigmoid(z) - t) / T), 5 = mean_absolute_error (d = sign(o - t) / T, sign(0) = 0),
 *                    6 = huber (e = o - t: mean_j of e^2 / 2 where |e| <= delta, delta (|e| - delta / 2) beyond); label smoothing and
 *                    delta: gnn_loop_set_loss_params
 *   n_graphs, ng_*   NodeGraph^T in CSR form (as gnn_loop_readout) for GNNgraphBased, n_graphs = 0 otherwise
 *   dropout_state / dropout_output   [n_layers + 1] Dropout rate in front of Dense l (0 = none; last entry: in front of
 *                    BatchNormalization), i.e. GNN/MLP.py:54-55 after its position shift; a NEGATIVE value -r is an AlphaDropout
 *                    of rate r (MLP(..., alphadropout=True), GNN/MLP.py:59-61)
 *   masks_*          injected keep-masks (uint8, 1 = keep): for net_state max_iter blocks, each the concatenation over the
 *                    dropout positions of [N, width]; for net_output one such block over the masked rows; NULL = engine RNG(seed)
 *   seed             defines every mask the engine draws in this step.  Each Dropout use - (net, body, position) - has a stream of its own,
 *                    keyed by HASHING: key = mix64(mix64(seed) ^ tag), tag = net << 56 | body << 16 | position (net 0 = net_state, 1 =
 *                    net_output with body 0; mix64 = the splitmix64 finalizer); element i of the mask, i its flat index in the
 *                    [rows of the WHOLE graph, width] matrix, is kept when the top 24 bits of mix64(key ^ mix64(i)) / 2^24 >= rate.
 *                    Neighbouring seeds, bodies and positions therefore draw unrelated masks, and because i counts the rows (net_output:
 *                    the masked rows) of the lower ranks too, a seed defines the step whatever the number of ranks: the masks of a
 *                    sharded gnn_loop_train_forward are the rows of the unsharded one's.  gnn_loop_train_mask reads them back.
 *   bn_state / bn_output   [gamma | beta] of the trailing BatchNormalization (NULL without one)
 * Outputs: *loss_out, *k_out (executed bodies), grads_* flat in get_weights() order of the TRAINABLE arrays
 * [dW1, db1, ..., dgamma, dbeta] (raw sums over the iterations: the division by k of :241 is the caller's), bn_batch_state
 * [k][2][Ds] and bn_batch_output [2][T] = batch mean / biased batch variance of every BatchNormalization call (the caller
 * applies the moving-average updates).  Single GPU, node/graph-based. */
int gnn_loop_train_step(gnn_loop *l, const int32_t *src_indptr, const int32_t *src_dst, const float *src_w,
                        const float *targets, const float *sample_weights, int64_t n_targets, int loss_kind,
                        int n_graphs, const int32_t *ng_indptr, const int32_t *ng_node, const float *ng_w,
                        const float *dropout_state, const float *dropout_output, const uint8_t *masks_state,
                        const uint8_t *masks_output, uint64_t seed, const float *bn_state, const float *bn_output,
                        float *loss_out, float *k_out, float *grads_state, float *grads_output,
                        float *bn_batch_state, float *bn_batch_output);
/* The two halves of gnn_loop_train_step, for models whose loss spans several loops (LGNN 'parallel' / 'residual'
 * training, reference GNN/LGNN.py:201-224 inside GNN_BaseClass.py:231-247, where layer i + 1's labels contain layer
 * i's state / output, LGNN.py:227-260).
 *   gnn_loop_train_forward   training-mode Loop; out_nodes [n_masked, T] (may be NULL) are the node-level outputs.  The
 *                    training-mode state / outputs become the loop's result (gnn_loop_get_state / get_output / readout,
 *                    gnn_graph_update_labels), and the context of the backward pass stays with the loop.
 *                    On node-range shards with full-replica numbering (one process per rank, an RCCL communicator; round 3) this
 *                    half also runs sharded: the state rows are all-gathered after every body, and the BatchNormalization batch
 *                    statistics (reference GNN/MLP.py:62-63, training=True) and the gate of reduce_any (GNN.py:218) are those of
 *                    the rows of ALL ranks - 3 F floats per rank and BatchNormalization call.  Give src_indptr / src_dst / src_w = the
 *                    arcs that LEAVE the owned rows (CSR over the owned rows, destinations as replica rows) for the backward half.
 *   gnn_loop_train_backward  d_out_nodes [n_masked, T] = d loss / d out_nodes; d_state_extra [N, Ds] (or NULL) = an extra
 *                    gradient on the final state; d_nodes [N, NL] (or NULL) receives d loss / d node labels; d_arc_labels
 *                    [n_arcs, AL] (or NULL; edge-based loops after gnn_graph_set_arc_order) d loss / d arc labels in
 *                    ORIGINAL arc order (LGNN.py:253-254).  One backward per forward.  On shards (after a sharded forward that was
 *                    given the by-source adjacency; node- / graph-based, no d_state_extra / d_nodes / d_arc_labels): per body the
 *                    gradient of the aggregated-state columns is all-gathered and every rank sums what its out-arcs carry back, the
 *                    sums of BatchNormalization's backward pass are those of all ranks, and the ranks' shares of the weight
 *                    gradients are added in rank order - every rank returns the same, complete gradients.  gnn_loop_train_step (one
 *                    call with the loss inside) stays single-GPU.
 *   gnn_loss_grad    host helper: *loss = sum_i w_i L(t_i, out_i) and d_out = d loss / d out (may be NULL), every loss_kind of
 *                    gnn_loop_train_step with label_smoothing 0 and huber_delta 1; gnn_loss_grad_ex takes the two as arguments. */
int gnn_loop_train_forward(gnn_loop *l, const int32_t *src_indptr, const int32_t *src_dst, const float *src_w,
                           const float *dropout_state, const float *dropout_output, const uint8_t *masks_state,
                           const uint8_t *masks_output, uint64_t seed, const float *bn_state, const float *bn_output,
                           float *k_out, float *out_nodes);
int gnn_loop_train_backward(gnn_loop *l, const float *d_out_nodes, const float *d_state_extra, float *grads_state,
                            float *grads_output, float *bn_batch_state, float *bn_batch_output, float *d_nodes,
                            float *d_arc_labels);
/* gnn_loop_train_backward for a stack of loops whose label gradients stay on the device (LGNN's joint steps; every gradient mode).
 *   keep_label_gradients   GNN_KEEP_D_NODES: d_nodes [N, NL], GNN_KEEP_D_ARC_LABELS (edge-based loops; ignored by others): d_arc_labels [n_arcs, AL] -
 *                    what is named is computed and left in the loop's training scratch, valid until this loop's next training forward; there is
 *                    no host copy.  A caller names what the layer below will read: d_nodes for get_state and for the outputs of a node- or
 *                    graph-based layer, d_arc_labels for the outputs of an edge-based one; 0 computes neither.
 *   next (or NULL)   the loop of the layer above, whose last backward pass kept its label gradients; its labels are [base labels | this loop's
 *                    state? | this loop's scattered outputs?] (gnn_graph_update_labels).  With NLb / ALb the base widths, in front of anything else:
 *                    get_state  != 0: d_state = next.d_nodes[:, NLb : NLb + Ds], in the place of an uploaded d_state_extra;
 *                    get_output != 0: d_out[q] += next.d_nodes[masked row q, c : c + T], c = NLb + (get_state ? Ds : 0); edge-based loops:
 *                                     d_out[q] += next.d_arc_labels[masked arc q, ALb : ALb + T].
 *                    One float32 addition per element, as a host that chains the two calls makes: every result equals the host-chained one bit
 *                    for bit.  A mismatch of device, row count, the NUMBER of masked rows / arcs or label widths between l and next is
 *                    GNN_ERR_ARG (which rows are masked is the caller's: next's labels were filled from this loop by gnn_graph_update_labels). */
enum { GNN_KEEP_D_NODES = 1, GNN_KEEP_D_ARC_LABELS = 2 };
int gnn_loop_train_backward_chained(gnn_loop *l, const float *d_out_nodes, gnn_loop *next, int get_state, int get_output, float *grads_state,
                                    float *grads_output, float *bn_batch_state, float *bn_batch_output, int keep_label_gradients);
/* Gradient mode of a loop's training step.  mode 0 (default): back-propagation through the unrolled loop, as described above.
 * mode 1 ("fixed point"): the gradient at the converged state (Almeida-Pineda; Scarselli et al. 2009, section III).  With Ds the state width:
 *   Forward        the INFERENCE Loop runs with the loop's own settings (arithmetic, persistent or per-body form, certified gate) and gives
 *                  k and p = x_k, the state after k bodies.
 *   Recorded body  ONE training-mode body of net_state at p (the concat and the forward of mode 0); its output state is discarded.  The
 *                  step's scratch holds one body's activations whatever max_iter is.
 *   Outputs, loss  unchanged: training-mode net_output on the rows of p (Dropout, BatchNormalization, moving statistics, graph and edge
 *                  readouts), published as the loop's result like those of mode 0.
 *   g              d loss / d p as mode 0 builds it (d_state_extra included).
 *   Adjoint        z_0 = g, z_{t+1} = g + J^T z_t; J = d body / d state at p over the own-state columns of the concat AND the aggregated-
 *                  state columns through the adjacency by source:  z_{t+1}[r] = g[r] + (u[r, :Ds] + sum over the arcs r -> dst, in stored
 *                  order, of w u[dst, c_aggs : c_aggs + Ds]),  u = d concat of the recorded body for the incoming gradient z_t.  It stops after
 *                  iteration t + 1 when NO node has |z_{t+1}[r] - z_t[r]| > theta_adj |z_t[r]| (L2 over the row, strict '>': the rule of the
 *                  forward condition; a zero row that stays zero does not move), or after adjoint_max_iter iterations.  Not converging is not
 *                  an error: the truncated sum is returned, and gnn_loop_adjoint_info reports it.  The host reads the gates once per five
 *                  iterations; an iteration queued behind a closed gate sees that gate on the device, hands z on unchanged and raises
 *                  nothing, so the count - the first closed gate - decides what is returned, and nothing is computed twice.
 *   net_state gradients   ONE weight-gradient pass of the recorded body with incoming gradient z_final.  They are NOT a sum over bodies:
 *                  a caller that averages (`mean`) must NOT divide them by k, and a step armed with mean != 0 applies them with scale 1.
 *   Everything behind the gradients (regularizers, clipping, optimizer kinds, net_output's moving statistics) is untouched.
 * Refused with GNN_ERR_UNSUPPORTED by the training forward / step / backward of a loop in mode 1: a net_state with BatchNormalization or any
 * Dropout rate != 0 (its training-mode forward is then not the inference forward), world > 1, and requests for d_nodes / d_arc_labels
 * (without GNN_ADJOINT_LABEL_GRADIENTS, below; with state_vect_dim == 0 always).
 * No float atomics: two identical steps return identical bits.
 * Narrow nets (net_state of 1 - 3 Dense layers of at most 64 outputs, no softmax, a concat of at most 96 columns, fewer than 4,096 rows - the regime where
 * a step is bound by its launch count) run an adjoint iteration as ONE launch: a block owns 16 rows, forms their z from the previous launch's u with
 * the gate of the previous iteration, and runs the whole chain through W^T with the weights staged in LDS (same sums, float32 fmaf).  mode 2 is mode 1
 * without that form (the per-kernel chain everywhere): for A/B runs and tests.
 * gnn_loop_set_gradient_mode_ex with GNN_ADJOINT_FROZEN_BN in flags (opt-in; flags 0 IS gnn_loop_set_gradient_mode): a net_state that ends in
 * BatchNormalization is accepted in modes 1 and 2, on its MOVING statistics - the per-row affine map the inference Loop iterates:
 *   Forward        unchanged (the inference Loop folds the moving statistics into scale and shift already).
 *   Recorded body  behind the Dense chain: inv_j = 1 / sqrtf(var_mov_j + eps), xhat = (h - mean_mov_j) inv_j, y = gamma_j xhat + beta_j; no batch
 *                  statistics are taken, xhat is kept for the weight pass alone.
 *   Adjoint        z is scaled per column by s_j = gamma_j inv_j (one vector of Ds floats per step) in front of act'(a_last): d h = d s_j.  There
 *                  are no mean or variance terms.
 *   net_state gradients   d gamma_j = sum_r d[r, j] xhat[r, j], d beta_j = sum_r d[r, j] (fixed-order chunk partials), d h = d s_j, then the
 *                  Dense chain as without BatchNormalization.  gamma and beta train like any other array.
 *   Moving statistics of net_state   NOT touched: not by the armed step, gnn_loop_optimizer_step or gnn_loop_update_moving_statistics, and
 *                  bn_batch_state is left unwritten (there are no batch statistics of net_state).  net_output's are updated as in mode 0.
 * Dropout in net_state, world > 1 and d_nodes / d_arc_labels stay refused.
 * GNN_ADJOINT_LABEL_GRADIENTS in flags (opt-in; combines with GNN_ADJOINT_FROZEN_BN): gnn_loop_train_backward of modes 1 and 2 accepts d_nodes and,
 * for edge-based loops after gnn_graph_set_arc_order, d_arc_labels.  With p = F(p, l) the fixed point and l the labels,
 *   d loss / d l = (the direct part through net_output / the edge readout) + (d F / d l)^T z_final,
 * and (d F / d l)^T z_final is the label columns of the recorded body's d concat for the incoming gradient z_final - the pass that gives net_state's
 * weight gradients - scattered as mode 0 scatters ONE body's label columns: own node columns directly, aggregated-node columns over the adjacency
 * by source, aggregated-arc columns through ArcNode^T.  No sum over bodies.  Without the flag nothing changes.  Refused in modes 1 and 2 whatever
 * the flags: Dropout in net_state, world > 1, and d_nodes / d_arc_labels of a loop with state_vect_dim == 0 (mode 0 returns the gradient of the
 * INITIAL state there, which a fixed point does not depend on).
 * adjoint_max_iter = 0 / adjoint_threshold < 0: the loop's own max_iter / threshold.  *used (may be NULL) = the mode now set.
 * gnn_loop_adjoint_info: iterations and converged (0 / 1) of the last backward pass of mode 1, and the form of its gather (0: any Ds, every
 * 16th column per lane; 1: 16-byte pieces, Ds % 4 == 0 and Ds <= 64; 2: the same from the aligned rows the three-layer chain leaves; 3: inside the
 * one-launch iteration of narrow nets);
 * any pointer may be NULL. */
int gnn_loop_set_gradient_mode(gnn_loop *l, int mode, int adjoint_max_iter, float adjoint_threshold, int *used);
enum { GNN_ADJOINT_FROZEN_BN = 1, GNN_ADJOINT_LABEL_GRADIENTS = 2 };
int gnn_loop_set_gradient_mode_ex(gnn_loop *l, int mode, int adjoint_max_iter, float adjoint_threshold, int flags, int *used);
int gnn_loop_adjoint_info(const gnn_loop *l, int *iterations, int *converged, int *form);
/* What an adjoint iteration of mode 1 launches for a net_state of this description (arguments as gnn_train_forms; the state width is
 * the net's last width) on n_rows rows - host code, no device, the decision the step itself takes.  out receives 4 + n_layers ints: out[0] = 1
 * eligible / 0 refused; out[1] = reason of a refusal (1 BatchNormalization - pass has_bn, 2 a Dropout rate != 0; 0 otherwise);
 * out[2] = gather form as gnn_loop_adjoint_info; out[3 + l] = backward form of Dense layer l (GNN_FORM_PER_OP: the row blocks of
 * k_layer_bwd alone, GNN_FORM_WIDE, GNN_FORM_CHAIN3, or GNN_FORM_ADJ_NARROW for every layer); no weight-gradient kernel runs in an iteration;
 * out[3 + n_layers] = why the one-launch iteration of narrow nets is NOT taken (0: it is; 3 more than three layers, 4 a layer wider than 64, 5 a concat
 * wider than 96, 6 4,096 rows or more, or none, 7 a softmax in net_state). */
int gnn_adjoint_form(int n_layers, const int *dims, const int *acts, const float *rates, int has_bn, int64_t n_rows, int *out);
/* The same for a loop set with `flags` (gnn_loop_set_gradient_mode_ex): with GNN_ADJOINT_FROZEN_BN a net with has_bn != 0 is eligible (out[1] = 0)
 * and the forms are those of its Dense chain - the frozen BatchNormalization pass takes the place of the last activation's derivative pass and is
 * inside the one-launch iteration of narrow nets.  GNN_ADJOINT_LABEL_GRADIENTS is accepted and changes no form.  flags 0: gnn_adjoint_form. */
int gnn_adjoint_form_ex(int n_layers, const int *dims, const int *acts, const float *rates, int has_bn, int flags, int64_t n_rows, int *out);
/* z_final [n_rows, Ds] of the last backward pass of mode 1 / 2, to host memory (test entry point; GNN_ERR_STATE without such a pass). */
int gnn_loop_adjoint_z(gnn_loop *l, float *z_host);
/* Solver of the adjoint system (I - J^T) z = g of modes 1 / 2 (opt-in; solver 0, the default, is the iteration z <- g + J^T z above with every launch,
 * allocation and bit as without this call).  solver 1: Anderson mixing over a window of m = `window` difference pairs - on a linear map a
 * GMRES-like method that needs only the operator the plain iteration applies; its count grows far slower than 1 / (1 - rho(J)).  z_0 = g; for t = 0, 1, ...:
 *   G_t, f_t       G_t = g + J^T z_t with the arithmetic of the plain iteration (the input-gradient-only backward pass on the per-kernel chain, the
 *                  gather's fmaf chain over the arcs in stored order, g + (own + acc)); f_t = G_t - z_t in float32.
 *   Gate t         the plain iteration's rule on the residual: a node moves when sqrt(sum f_t[r]^2) > theta_adj sqrt(sum z_t[r]^2) (strict; with
 *                  z_next = G_t this IS the Picard gate).  Closed: z_final = G_t, iterations = t + 1, converged.
 *   Window         with hist = difference pairs stored since the last restart (0 at t = 0), an iteration t >= 1 writes slot s = hist mod m:
 *                  dF_s = f_t - f_{t-1}, dG_s = G_t - G_{t-1} in float32; live = min(hist + 1, m).
 *   Gram           H_ij = dF_i . dF_j and b_i = dF_i . f_t over the live slots, products and sums in double, in a fixed order: per lane over its
 *                  ascending columns, the 16 lanes of a row by a fixed butterfly, the 16 rows of a block in row order, the blocks in block order in
 *                  256 runs.  Row and column s of H are new per iteration, the rest stays in a device-resident double matrix; b is recomputed whole.
 *   Solve          (H + lambda I) gamma = b with lambda = 2^-40 trace(H) / live, by Cholesky in double in one thread.  A pivot that is not > 0, or any
 *                  value that is not finite, RESTARTS the window: gamma = 0, hist = 0, and the restart is counted.
 *   Mix            z_{t+1} = G_t - sum_i gamma_i dG_i, gamma rounded to float, the sum a float fmaf chain over ascending slots.
 * Three kernels per iteration behind the backward pass (gather with residual, slot, gate and the blocks' partial dots; a one-block solve; the mix);
 * the one-launch iteration of narrow nets is not used.  Control stays on the device as above: iterations are enqueued five at a time, kernels behind a
 * closed gate change nothing.  No float atomics: two identical steps return identical bits.  Scratch: 2 m + 2 more [n_rows, Ds] float buffers.
 * The bits of the gradients differ from solver 0's (both lie within the adjoint threshold of the solution).  The method presumes what the mode
 * presumes, a contraction: without one the forward Loop has no fixed point and the gradient means nothing, whatever this solver returns.
 * window outside 1 .. 8 or solver outside 0 / 1: GNN_ERR_ARG; solver 1 with world > 1: GNN_ERR_UNSUPPORTED, as the mode.  *used (may be NULL) = the
 * solver now set.  gnn_loop_adjoint_solver_info: the solver and window set, and the restarts of the last backward pass; any pointer may be NULL. */
int gnn_loop_set_adjoint_solver(gnn_loop *l, int solver, int window, int *used);
int gnn_loop_adjoint_solver_info(const gnn_loop *l, int *solver, int *window, int *restarts);
/* Contraction estimate at the fixed point: how far net_state's map is from a contraction at the state the Loop finds - the condition under which the
 * adjoint iteration of modes 1 / 2 (and the inference Loop near its fixed point) converges.  With p the state the inference Loop stops at, F one body of
 * net_state at p (BatchNormalization on its moving statistics, always) and J = dF/dp over the own-state and aggregated-state columns - the J of the
 * adjoint iteration above - power iteration on J^T from w_0 [N, Ds], n_0 = |w_0|_2:
 *   for t = 1 .. iterations:   w_t = (J^T w_{t-1}) * (1 / n_{t-1});   n_t = |w_t|_2;   growth[t - 1] = n_t
 * so growth[t - 1] = |J^T v_{t-1}| for the unit vector v_{t-1} = w_{t-1} / |w_{t-1}|.  Its late entries approach the spectral radius of J when the
 * dominant eigenvalue is real; their geometric mean is the Gelfand estimate otherwise.  If some n_t is 0 or not finite the iteration stops there:
 * *done = t, growth[t - 1] is what was measured, the later entries are 0 (otherwise *done = iterations).
 *   Forward        as the training forward of mode 1: the inference Loop with the loop's own settings (state0, arithmetic, launch form, certified
 *                  gate) gives *k and p, ONE body is recorded at p.  net_output does not run.
 *   Iteration      the input-gradient-only backward pass of the recorded body on the per-kernel chain (as mode 2), then a gather with the adjoint
 *                  gather's three shapes and its fmaf chain over the arcs in stored order: w_t[r] = (u[r, :Ds] + sum w u[dst, c_aggs : c_aggs + Ds]) * inv,
 *                  inv = 1 / n_{t-1} read from one device float.  The same pass leaves one partial squared norm per block of 16 rows (per lane over
 *                  ascending columns, the 16 lanes of a row by a fixed butterfly, the rows in order); one block adds the partials in block order in
 *                  double, writes n_t and the next inv (0 stops every later gather on the device).  No float atomics: two calls return the same
 *                  bits.  The host waits once, at the end.
 *   src_*, dropout_state, bn_state   as gnn_loop_train_forward takes them for net_state; iterations: 1 .. 1024 (else GNN_ERR_ARG);
 *   v0 [N, Ds]     w_0, or NULL: normal draws of the engine's counter RNG keyed on seed (element i: mix64(mix64(seed) ^ mix64(i)), Box-Muller).
 * Works in every gradient mode and leaves the mode as it is.  Like any forward it ends the life of a pending training forward's context: a
 * gnn_loop_train_backward behind it is refused (GNN_ERR_STATE).  The loop's state / outputs are those of the inference Loop it ran.
 * GNN_ERR_UNSUPPORTED, with the reason in gnn_last_error: a Dropout rate != 0 in net_state, state_vect_dim == 0, world > 1.
 * A graph without rows: *done = 0, growth all zero. */
int gnn_loop_contraction_estimate(gnn_loop *l, const int32_t *src_indptr, const int32_t *src_dst, const float *src_w, const float *dropout_state,
                                  const float *bn_state, int iterations, const float *v0, uint64_t seed, float *growth, int *done, float *k_out);
/* w_done [n_rows, Ds] of the last gnn_loop_contraction_estimate, to host memory (test entry point, not part of the supported interface; GNN_ERR_STATE
 * without an estimate, or after a training forward since). */
int gnn_loop_contraction_vector(gnn_loop *l, float *w_host);
/* Bytes handed out from the step's scratch by the last training forward / backward of this loop (test entry point). */
int gnn_loop_train_arena_bytes(const gnn_loop *l, int64_t *bytes);
/* Optimizer step on the device (reference GNN_BaseClass.py:243-247, optimizer.apply_gradients on the trainable variables of
 * both nets, and the moving statistics Keras BatchNormalization updates in training mode): weights, optimizer slots (kept with
 * the gnn_mlp) and gradients stay in HBM.  hyper is always four floats; per entry, in float32, on the gradient g after the
 * regularizer terms, the division by k and the clipping:
 *   kind 0 SGD              {learning_rate, momentum, nesterov (0 / 1), -}: v <- momentum v - lr g; p <- p + v, or with nesterov
 *                           p <- p + momentum v - lr g
 *   kind 1 Adam             {lr_t = lr sqrt(1 - beta_2^t) / (1 - beta_1^t), beta_1, beta_2, epsilon} (the caller counts t):
 *                           m <- beta_1 m + (1 - beta_1) g, v <- beta_2 v + (1 - beta_2) g^2, p <- p - lr_t m / (sqrt(v) + epsilon)
 *   kind 2 Adam, amsgrad    as kind 1, with vhat <- max(vhat, v) in place of v in the denominator
 *   kind 3 RMSprop          {learning_rate, rho, momentum, epsilon}: r <- rho r + (1 - rho) g^2; momentum == 0:
 *                           p <- p - lr g / (sqrt(r) + epsilon); momentum > 0: q <- momentum q + lr g / sqrt(r + epsilon), p <- p - q
 *   kind 4 RMSprop, centered  also a <- rho a + (1 - rho) g, and max(r - a^2, 0) in place of r in both branches (the difference
 *                           cancels in float32: the clamp is part of the rule)
 *   kind 5 Adagrad          {learning_rate, initial_accumulator_value, epsilon, -}: s <- s + g^2 (s starts at 0),
 *                           p <- p - lr g / (sqrt(initial_accumulator_value + s) + epsilon)
 *   kind 6 Adamax           {learning_rate / (1 - beta_1^t), beta_1, beta_2, epsilon}: m <- beta_1 m + (1 - beta_1) g,
 *                           u <- max(beta_2 u, |g|), p <- p - hyper[0] m / (u + epsilon)
 * Any other kind is GNN_ERR_ARG, and so is, for kinds 2 - 6, a negative or non-finite value where the rule divides by it (epsilon,
 * RMSprop's momentum, Adagrad's initial_accumulator_value).  These rules - the two places of RMSprop's epsilon among them - are
 * definitions of this library, written down from memory of tf.keras 2.x; they have not been checked against TensorFlow.
 * Slots: every net has up to three arrays laid out like its gradient vector, the third only once a kind that uses it (2, 4) has
 * run.  All slots start at zero, and a step whose kind differs from the kind that last wrote a net's slots restarts them from zero
 * (gnn_mlp_reset_optimizer does the same for a new optimizer object of the same kind).
 *   gnn_loop_arm_optimizer   one-shot: the NEXT gnn_loop_train_step applies the update behind its backward pass, before the
 *                            step's single wait for the device; mean != 0 divides the net_state gradients by the iteration
 *                            count (GNN_BaseClass.py:241).  The gradients returned by that step are the raw ones.
 *   gnn_loop_optimizer_step  the same as a call of its own, after gnn_loop_train_step or forward + backward (once per backward);
 *                            state_grad_scale multiplies the net_state gradients.
 * With bn_state / bn_output NULL in the train calls, gamma / beta are the gnn_mlp's own device copy (the one updated here).
 * gnn_mlp_get_weights (above) reads the current arrays back. */
/* Keras BatchNormalization in training mode also updates its moving statistics when no gradient is taken (a Loop(training=True)
 * call, reference GNN/GNN.py:251-280 with training=True): moving <- moving * momentum + batch * (1 - momentum) per call, from the
 * batch statistics of the last gnn_loop_train_forward, on the device.  Once per forward pass; not after an optimizer step. */
int gnn_loop_update_moving_statistics(gnn_loop *l, float bn_momentum_state, float bn_momentum_output);
int gnn_loop_arm_optimizer(gnn_loop *l, int kind, const float *hyper, int mean, float bn_momentum_state, float bn_momentum_output);
int gnn_loop_optimizer_step(gnn_loop *l, int kind, const float *hyper, float state_grad_scale, float bn_momentum_state,
                            float bn_momentum_output);
int gnn_loss_grad(int loss_kind, int64_t n_rows, int n_out, const float *targets, const float *out,
                  const float *sample_weights, double *loss, float *d_out);
int gnn_loss_grad_ex(int loss_kind, int64_t n_rows, int n_out, const float *targets, const float *out,
                     const float *sample_weights, double label_smoothing, double huber_delta, double *loss, float *d_out);
/* Parameters of the loss inside gnn_loop_train_step, sticky per loop like gnn_loop_set_clipping (defaults 0 and 1).
 * label_smoothing s in [0, 1], applied to the targets before anything else: t <- t (1 - s) + s / T for loss_kind 0 and 2,
 * t <- t (1 - s) + s / 2 for 3 and 4, ignored by the others.  huber_delta > 0 and finite: the threshold of loss_kind 6.  A value
 * outside these ranges is GNN_ERR_ARG and leaves the setting as it was. */
int gnn_loop_set_loss_params(gnn_loop *l, double label_smoothing, double huber_delta);
/* Kernel / bias regularizers on the device (reference starter.py:55-66 hands them to MLP(), GNN/MLP.py:11-13; their penalties are
 * summed into the taped loss, GNN_BaseClass.py:223-235).  l1 / l2: [2 n_layers] coefficients per array in [W1, b1, W2, b2, ...]
 * order (BatchNormalization's gamma / beta never carry one); both NULL clears them; a negative or non-finite coefficient is
 * GNN_ERR_ARG.  From then on every backward pass of a loop with this net (gnn_loop_train_step, gnn_loop_train_backward) adds
 * l1 sign(w) + 2 l2 w (sign(0) = 0, w = the array before the update) to the gradient of every array before the gradients are
 * copied back or applied - the returned gradients include the term, still raw (not divided by k) - and gnn_loop_train_step adds the
 * penalty sum_a l1_a sum |w| + l2_a sum w^2 to *loss_out (its partial sums are read at the step's one wait). */
int gnn_mlp_set_regularizers(gnn_mlp *m, const double *l1, const double *l2);
/* Gradient clipping of the device-side update, as tf.keras optimizers define it (reference starter.py:81 takes any Keras
 * optimizer; the update is GNN_BaseClass.py:243-247).  0 = off; clipnorm together with global_clipnorm, a negative or a
 * non-finite value is GNN_ERR_ARG.  Applies to every later armed gnn_loop_train_step and every gnn_loop_optimizer_step of this
 * loop until changed.  On the gradients after the regularizer terms and after the division of net_state's by k (:241), in this
 * order: clipvalue c: g <- min(max(g, -c), c) per entry; clipnorm c: g_a <- g_a c / max(|g_a|_2, c) per array; global_clipnorm
 * c: g <- g c / max(|g|_2, c) with the norm over ALL arrays of both nets.  (The order value, norm, global is a definition of
 * this library, written down from memory of Keras' OptimizerV2; it has not been checked against TensorFlow.)  clipvalue is applied
 * as a float32 (the gradients' format), the two norm thresholds in double.  The sums of
 * squares are accumulated in double, per block and then in block order (the same bits in every run), and stay on the device:
 * the armed step gains no wait for the device. */
int gnn_loop_set_clipping(gnn_loop *l, double clipvalue, double clipnorm, double global_clipnorm);
/* For one optimizer step over SEVERAL loops (the LGNN joint step, reference GNN_BaseClass.py:244-247 over the variables of every
 * layer) with a global norm that spans them:
 *   gnn_loop_grad_sqnorm            after the backward pass: *sqnorm = sum of squares of this loop's gradients (both nets;
 *                                   net_state's times state_grad_scale; after the loop's clipvalue), *penalty = the regularizer
 *                                   penalty of both nets (either may be NULL).  Waits for the device.
 *   gnn_loop_optimizer_step_scaled  gnn_loop_optimizer_step with every clipped gradient multiplied by grad_scale (> 0) in place
 *                                   of the loop's own global_clipnorm: the caller's c / max(sqrt(sum of the loops' sqnorm), c). */
int gnn_loop_grad_sqnorm(gnn_loop *l, float state_grad_scale, double *sqnorm, double *penalty);
int gnn_loop_optimizer_step_scaled(gnn_loop *l, int kind, const float *hyper, float state_grad_scale, double grad_scale,
                                   float bn_momentum_state, float bn_momentum_output);
/* selects the implementation:
 *   0 = unfused reference kernels (one kernel per TF op), bit-identical to oracle/gnn_oracle.c;
 *   1 = fused gather + MLP kernel with the dense layers on the f32 MFMA: the same k-ordered fmaf chains, bit-identical
 *       to the oracle;
 *   2 = (default) fused kernel with the dense layers on the 16-bit MFMA: every fp32 operand is scaled by a power of two (exact) and
 *       cut into two fp16 pieces (round to nearest even, 22 - 24 bits together) and the three leading piece products are accumulated
 *       in fp32 on v_mfma_f32_32x32x16_f16 (dropped term <= 2^-24 per product, i.e. fp32 rounding level); activations through
 *       v_exp_f32 / v_rcp_f32; results within fp32 rounding noise of 0 / 1 (tests: 1e-5 against the float64 oracle, the
 *       tolerance of BASELINE.json), not bit for bit.  A Loop in which an activation leaves the fp16 range is repeated with
 *       three bf16 pieces per operand (six products on v_mfma_f32_32x32x16_bf16), the format of earlier releases
 *       (gnn_loop_set_pieces, gnn_loop_range_info).
 * 1 and 2 fall back to 0 when the net is not covered.  *used (may be NULL) reports the choice.  Covered: a net_state of one to three Dense
 * layers no wider than 128 whose hidden layers share ONE activation; the last layer may have any other of linear / relu / selu / elu /
 * tanh / sigmoid (['selu', 'selu', 'tanh'], ['relu', 'sigmoid'], ...) and runs the same kernels with the same arithmetic per mode.  Not
 * covered (impl 0): two different hidden activations (['relu', 'tanh', 'tanh']), softmax in net_state, a wider layer.  (Training is a
 * separate decision: a net whose activations differ keeps the per-layer matrix-core forms, not the three-layer chains k_fwd3_split /
 * k_bwd3_split.)
 * k contract of impl 2 (reference GNN/GNN.py:202-220: `distance > threshold * norm`, reduce_any, k < max_iteration): its iteration count
 * is the bit-exact chain's.  Every body also records whether some node moved by a margin ("robust") and whether some node's test lay
 * within a guard band of the threshold ("borderline"; band = 1e-5 norm + 1e-3 threshold norm); a gate with a robust mover, or without
 * a borderline node, is decided identically by both arithmetics.  When a gate of a run is neither, gnn_loop_run repeats that Loop on
 * impl 1 before it returns, and k, state and output are THAT run's (bit-identical to the oracle).  threshold 0 with moving states never
 * triggers it. */
int gnn_loop_set_impl(gnn_loop *l, int impl, int *used);
/* Outcome of the certified gate: *last_run_repeated = 1 when the last gnn_loop_run / _run_group / _run_many of this loop was repeated on
 * impl 1 (its results are the exact path's), *repeats_total = how often that has happened on this handle.  Either pointer may be NULL. */
int gnn_loop_gate_info(const gnn_loop *l, int *last_run_repeated, int *repeats_total);
/* Piece format of impl 2, for A/B measurements and tests (not a user-facing mode): 2 = two fp16 pieces per operand (default), 3 = three
 * bf16 pieces.  Format 2 takes |activation| < 65504 / 16 (4094): a Loop in which some body cut a larger one (or an infinity) raises a flag
 * word beside the gate words, and gnn_loop_run repeats that Loop in format 3 before it returns; k, state and output are then THAT run's.
 * *used (may be NULL) = the format set. */
int gnn_loop_set_pieces(gnn_loop *l, int pieces, int *used);
/* Outcome of the range guard: *last_run_repeated = 1 when the last run of this loop was repeated in format 3, *repeats_total = how often
 * that has happened on this handle.  Either pointer may be NULL. */
int gnn_loop_range_info(const gnn_loop *l, int *last_run_repeated, int *repeats_total);
/* Host-side piece cut of format 2 (exported for tests): the weight-scale exponent e of a layer with max |W| = max_abs (max_abs 2^e in
 * [2^14, 2^15)), and the pieces p0 = fp16(v 2^e), p1 = fp16(v 2^e - p0) of n values (round to nearest even). */
int gnn_split_f16_exponent(float max_abs);
void gnn_split_f16(const float *v, int n, int e, uint16_t *p0, uint16_t *p1);
/* Small graphs on a single GPU run the whole tf.while_loop of GNN/GNN.py:271 - initial state, first condition, every body with a grid
 * barrier in between - in ONE persistent launch when impl is 1 or 2 (exact f32-MFMA arithmetic in both cases, bit-identical to the
 * oracle).  The launch needs every tile resident at once and the net's weights in registers:
 *   - a net_state no wider than 32 (every layer), concat width <= 96: up to 8,192 owned nodes;
 *   - a net_state of two or three layers with hidden layers up to 64 wide (at least one above 32), state width <= 32, concat width
 *     <= 96: up to 4,096 owned nodes.
 * Everything else - a wide net on 4,097 .. 8,192 nodes, a state wider than 32, a concat wider than 96, 128-wide layers, more nodes, several
 * ranks, profiling - takes one launch per body.  enable = 0 keeps such a loop to one launch per body too; *used (may be NULL) tells
 * whether the persistent launch will be taken.  The nets are those of gnn_loop_set_impl: a last layer with an activation of its own takes
 * the persistent launch too, two different hidden activations or a softmax do not (per-op kernels). */
int gnn_loop_set_persistent(gnn_loop *l, int enable, int *used);
/* Which form of the fused iteration kernel runs the bodies of GNN/GNN.py:223-242 on the default path (impl 2) when both cover the
 * net (state width 64, two or three Dense layers, 128-wide hidden layers, concat width 129 .. 144, no feature-sliced exchange):
 *   form 1  one wave owns a 32-node tile from gather to store (k_fused_full);
 *   form 2  a wave PAIR shares the tile, each wave gathering 16 of its nodes and producing half of every layer's output features
 *           (k_fused_pair);
 *   form 0  the library's choice (default).
 * The wave pair exists for nets with one activation for ALL layers only: a net whose last layer has its own activation takes form 1
 * whatever is asked for (*used = 1).
 * The two forms evaluate the same arithmetic per node: states, outputs and k are identical bit for bit.  *used (may be NULL) = the form
 * the next run will take (1 or 2; 0 when the fused path does not cover the loop at all). */
int gnn_loop_set_tile_form(gnn_loop *l, int form, int *used);
/* The per-body kernel the next run takes as the loop's settings stand (on the persistent path: what a run with one launch per body would
 * take): *kernel = 0 the fused path does not cover the loop, 1 k_fused_generic (any state width but 64), 2 k_fused_full (state width 64),
 * 3 k_fused_pair.  A loop with state width 64 never reports 1: k_fused_generic has none of the width-64 paths. */
int gnn_loop_body_kernel(gnn_loop *l, int *kernel);
/* How the full-tile form-1 kernel (state width 64, impl 1 or 2, no feature-sliced exchange) finds a tile's neighbour rows:
 *   form 1  it walks the CSR: row pointers, then ids / weights in batches of 16 per lane group of 8 rows, row ends found by comparison;
 *   form 2  it reads the graph's gather program: the CSR walked once per graph and stored per tile and lane group in the order of
 *           consumption, the tile's rows split into four contiguous ranges of near-equal entry count (gnn_gather_program_build).  The
 *           program is built with the first Loop that takes this form, shared by the graphs derived from the same graph, and costs
 *           about 5.5 bytes per arc of device memory where the weights of every destination row are equal (all of the reference's
 *           aggregation modes: 4-byte entries and one weight per row), about 9.2 otherwise (8-byte entries); a graph for which it
 *           cannot be built (no memory, no full tile) runs form 1;
 *   form 0  the library's choice (default).
 * Every row's fmaf chain is the same in both forms: states, outputs and k are identical bit for bit.  *used (may be NULL) = the form the
 * next run will take (0 when the fused path does not cover the loop at all); asking for the form builds the program if it is needed. */
int gnn_loop_set_gather_form(gnn_loop *l, int form, int *used);
/* The order in which a launch of the program kernel (gather form 2) works through its tiles.  Waves take tiles by ticket; the schedule says
 * which tile a ticket stands for:
 *   kind 1  ascending: ticket s is tile s;
 *   kind 2  balanced by gather load (gnn_tile_schedule_build, kind 1 there): every stretch of the launch holds the same mix of heavy and
 *           light tiles, and the lightest tiles come last.  Built once per graph, on first demand, from the program's own figures;
 *   kind 0  the library's choice (default): GNN_TILE_SCHEDULE_DEFAULT for launches of at least four tiles per wave, ascending below.
 * A node's arithmetic does not depend on when its tile runs: states, outputs and k are identical bit for bit.  *used (may be NULL) = the
 * order the next run will take; 0 where its launches read no program. */
int gnn_loop_set_tile_schedule(gnn_loop *l, int kind, int *used);
/* Label projection: a fused Loop for wide node / arc labels.  The fused kernels hold the whole concat [state | nodes | agg state | agg nodes
 * | agg arcs] of 32 nodes in LDS, which caps it at about 144 columns; the label columns do not change during a Loop.  With the projection,
 * layer 0 of net_state is split by rows of its kernel W1: the label terms P = [nodes | agg nodes | agg arcs] . W1_label + b1 are computed
 * once per Loop (fp32 operands and accumulation on v_mfma_f32_32x32x2_f32, k ascending, run-to-run identical bits), and every body runs
 * layer 0 over [state | agg state] only - K = 2 x state width - with its accumulators started from P[node, :] instead of from the bias.
 *   mode 0  off (default): the Loop runs exactly as without this call, bit for bit;
 *   mode 1  where needed: taken when the fused path does not cover the net as it stands and covers the net over [state | agg state];
 *   mode 2  wherever applicable (A/B runs, tests on narrow labels).
 * A form of the default arithmetic (impl 2, both piece formats, CSR walk and gather program) with one launch per body only: impl 1 and
 * impl 0, the persistent small-graph loop and the feature-sliced exchange run as without it, and so does the bit-exact repeat of a Loop
 * whose gate was not certified (per-op kernels where the net is too wide for the exact fused kernel).  The label part of layer 0 is an
 * fp32 sum in another order than the oracle's, about 1e-7 relative: states and outputs stay within the default path's 1e-5, k is the exact
 * chain's under the certified gate.  P is cached across runs like the label aggregates, rebuilt when the graph's labels or net_state's
 * weights change, and dropped by gnn_loop_drop_cached_aggregates.  Training-mode runs never take it.
 * *used (may be NULL) = 1 when the next run takes the seeded kernels, else 0. */
int gnn_loop_set_label_projection(gnn_loop *l, int mode, int *used);
/* Test entry points of the label projection, not part of the supported interface.
 * The projection the last run of l used, as P [n_rows, H1] row-major (H1 = width of net_state's first layer); GNN_ERR_STATE when that run
 * used none. */
int gnn_loop_get_label_projection(gnn_loop *l, float *out);
/* What gnn_loop_set_label_projection(mode) answers from shapes alone - host code, no device: dims [n_layers + 1] (dims[0] the whole
 * concat), acts [n_layers], state width, node-label columns in the concat, arc-label width, owned rows; impl 2, a single GPU, no
 * feature-sliced exchange, not profiling are the loop's part, taken at their defaults.  out receives 4 ints: out[0] = 1 seeded / 0 not
 * (then the rest is 0); out[1] = per-body kernel as gnn_loop_body_kernel (1 k_fused_generic, 2 k_fused_full); out[2] = projected label
 * columns IW; out[3] = 32-feature tiles of P per 32-row tile. */
int gnn_label_projection_form(int n_layers, const int *dims, const int *acts, int state_dim, int n_label_cols_in_concat, int arc_label_dim,
                              int64_t n_rows, int mode, int *out);
/* Wide-state form: one launch per body for state widths 68 .. 128.  The fused kernels hold the concat of 32 nodes per wave in LDS, eight
 * waves per workgroup; [state | agg state] alone is past that for a state wider than 72.  With this form k_fused_generic runs on a
 * workgroup of 4 to 7 waves - as many 32-node tiles as fit 160 KiB of LDS, at least one wave per SIMD - and loads the full tiles with a
 * loader for rows of 68 to 128 floats (load_tile_wide: one row per 32-lane group and instruction, 16 rows in flight per lane).
 *   mode 0  off (default): the Loop runs exactly as without this call, bit for bit;
 *   mode 1  where profiles/wide_state.txt measured the form faster than one kernel per op;
 *   mode 2  wherever it is covered and the eight-wave path is not.
 * Covered: a state width that is a multiple of 4 in 68 .. 128 and a net_state the fused path refuses ONLY for its LDS (layers up to 128
 * wide, no softmax, one activation for all hidden layers) whose tile fits at four waves - a 128-wide state with about a dozen label
 * columns; with the label projection on (gnn_loop_set_label_projection), the net over [state | agg state] likewise, whatever the labels'
 * width.  impl 1 and impl 2, both piece formats, the certified-gate and range-guard repeats, row-exchange shards; with the feature-sliced
 * exchange the same launch with the given aggregate (load_tile_generic).  The arithmetic per node is the eight-wave kernel's: impl 1 is
 * bit-identical to the C oracle.  The persistent small-graph loop and training-mode runs never take it.
 * *used (may be NULL) = 1 when the next run takes the form, else 0. */
int gnn_loop_set_wide_state(gnn_loop *l, int mode, int *used);
/* What gnn_loop_set_wide_state(mode) answers from shapes alone, with the label projection in label_projection_mode - host code, no device;
 * arguments and the loop's part as gnn_label_projection_form.  out receives 4 ints: out[0] = 1 taken / 0 not (then the rest is 0);
 * out[1] = per-body kernel as gnn_loop_body_kernel (always 1, k_fused_generic); out[2] = waves per workgroup (4 .. 7); out[3] = 1 when the
 * launch is the seeded one of the label projection. */
int gnn_wide_state_form(int n_layers, const int *dims, const int *acts, int state_dim, int n_label_cols_in_concat, int arc_label_dim,
                        int64_t n_rows, int mode, int label_projection_mode, int *out);
/* Test entry points of the launch per body, not part of the supported interface.
 * out[0] = waves per workgroup, out[1] = workgroups of the launch per body of the loop's last form decision - a setter's or a run's
 * (0, 0: the loop takes no such launch). */
int gnn_loop_body_launch(const gnn_loop *l, int *out);
/* At most max_workgroups workgroups per k_fused_generic launch (0, the default: the library's choice), so that a few hundred rows reach a
 * wave's second static tile and the ticket counter.  Results do not depend on it.  *used (may be NULL) = the grid of the next run's launch. */
int gnn_loop_set_grid_limit(gnn_loop *l, int max_workgroups, int *used);
/* The tile loader of the wide-state form's full tiles: 0 load_tile_wide (default), 1 load_tile_generic - same bits, for A/B runs.
 * *used (may be NULL) = 1 when the next run's launches use load_tile_wide. */
int gnn_loop_set_wide_loader(gnn_loop *l, int loader, int *used);
/* ---- Test and diagnostic entry points of gather form 2: not part of the supported interface, they may change with the program's layout. ----
 * The gather program of rows [0, n_rows) of a CSR graph (host code; tests/test_gather_program.py).  Per full 32-row tile t: hdr[2 t] = first
 * 64-entry batch, hdr[2 t + 1] = batches; ent[(64 b + 16 g + j) 2 + {0, 1}] = {source word, weight bits} of entry j of lane group g in
 * batch b.  Source word: adj_src << 8 | row-end bit 32 | tile-local row (low 5 bits); 0xfffffe00 | ... for an entry without a source (the
 * one entry of an empty row, weight 0; padding behind a group's last row end, no row-end bit).  hdr ([2 (n_rows / 32)]) and ent may be
 * NULL: *n_batches is always set, so a first call sizes ent.  Returns GNN_ERR_UNSUPPORTED when a source id does not fit (>= 2^23). */
int gnn_gather_program_build(int64_t n_rows, const int32_t *indptr, const int32_t *adj_src, const float *adj_w, int32_t *hdr, int32_t *ent,
                             int64_t *n_batches);
/* Size and host build time of the program of g's graph: 0 tiles when it has none (yet).  Any pointer may be NULL.  bytes: 8 tiles + 512
 * batches in entry format 8; 8 tiles + 256 batches + 128 slots (the row weights of one tile schedule) in entry format 4. */
int gnn_graph_gather_program_info(const gnn_graph *g, int64_t *tiles, int64_t *batches, int64_t *bytes, float *build_ms);
/* The compact form of a program (host code; tests/test_gather_program_compact.py): words[64 b + l] = the source word of entry l of batch b,
 * unchanged; roww[32 t + r] = the weight all entries of tile-local row r of tile t share, +0 for an empty row.  hdr [tiles][2] as built by
 * gnn_gather_program_build, ent [n_batches][64][2].  Returns GNN_ERR_UNSUPPORTED - "not compactable" - when a row holds two entries whose
 * weights differ as bit patterns. */
int gnn_gather_program_compact(int64_t tiles, const int32_t *hdr, int64_t n_batches, const int32_t *ent, int32_t *words, float *roww);
/* The entry format of the program g's graph holds on its device: *entries = 0 none (yet), 8 {source word, weight} pairs, 4 source words
 * and one weight per row. */
int gnn_graph_gather_program_format(const gnn_graph *g, int *entries);
/* The entry format to build, for A/B runs and tests: 0 the library's choice (4 where every row's weights are one bit pattern, else 8), 8,
 * or 4.  Drops the program and the tile schedules the graph (and the graphs derived from it) holds, so that the next form-2 Loop rebuilds
 * them, and rebuilds at once where there was a program or a format is asked for.  *used (may be NULL) = the format held from now on:
 * asking for 4 on a graph with a non-uniform row keeps 8 (not available); 0 = no program.  Results do not depend on the format. */
int gnn_graph_set_program_entries(gnn_graph *g, int entries, int *used);
/* A tile schedule (host code; tests/test_tile_schedule_host.py): order[slot] = the tile that ticket `slot` stands for, for `slots` tiles of
 * cost[t] real entries (arcs) each and launches of `waves` waves.  kind 0: the identity.  kind 1: tiles sorted by cost descending (ties by
 * id ascending); the lightest min(2 waves, slots / 2) last, heaviest of them first; the rest dealt column-wise over 61 strata of the sorted
 * order, so that every window of `waves` slots has about the mean cost and the first tiles of a workgroup's waves differ. */
int gnn_tile_schedule_build(int64_t slots, const int64_t *cost, int64_t waves, int kind, int32_t *order);
/* Schedules of g's program: slots (0 without a program), kind built so far (1 ascending only, 2 the balanced order too), body and tail
 * sizes of the balanced order and its host build time.  Any pointer may be NULL. */
int gnn_graph_tile_schedule_info(const gnn_graph *g, int64_t *slots, int *kind, int64_t *body, int64_t *tail, float *build_ms);
/* ---- Test entry points of the training step: read-only, not part of the supported interface. ----
 * Which kernels the Dense layers of a net take in a training-mode forward / backward pass on n_rows rows per call (the decision of
 * gnn_loop_train_forward; few rows: the per-op kernels or one launch for all layers, 4,096 rows and more: wide layers on the matrix cores).
 * out receives 3 + 3 n_layers ints:
 *   out[0] = n_layers; out[1] = 1 when the first forward kernel also builds the concat rows of a body; out[2] = rows the persistent
 *   matrix-core kernels cover before a wave takes a second 32-row tile;
 *   out[3 + 3 l] = forward form of Dense layer l: GNN_FORM_PER_OP (k_dense_fwd), GNN_FORM_MLP_FWD (all layers in k_mlp_fwd), GNN_FORM_WIDE (its
 *   own matrix-core product, k_gemm_split) or GNN_FORM_CHAIN3 (inside k_fwd3_split);
 *   out[4 + 3 l] = backward form: GNN_FORM_PER_OP (k_layer_bwd), GNN_FORM_WIDE (k_gemm_split on W^T) or GNN_FORM_CHAIN3 (inside k_bwd3_split);
 *   out[5 + 3 l] = weight-gradient kernel: GNN_FORM_PER_OP (the tiles of k_layer_bwd), GNN_FORM_WGRAD_BF (k_wgrad_bf) or GNN_FORM_WGRAD_F32.
 * gnn_train_forms (host code, no device): a net described by dims [n_layers + 1], acts [n_layers] (gnn_activation codes) and the Dropout
 * rates [n_layers + 1] in front of every Dense layer and of BatchNormalization; producer_dropout != 0: net_state (the concat kernel applies
 * the Dropout in front of the first layer), 0: net_output.  gnn_loop_train_forms: what the last gnn_loop_train_forward / gnn_loop_train_step
 * of this loop decided for net 0 (net_state) or 1 (net_output); GNN_ERR_STATE before the first one. */
enum { GNN_FORM_PER_OP = 0, GNN_FORM_MLP_FWD = 1, GNN_FORM_WIDE = 2, GNN_FORM_CHAIN3 = 3, GNN_FORM_WGRAD_BF = 4, GNN_FORM_WGRAD_F32 = 5,
       GNN_FORM_ADJ_NARROW = 6 /* gnn_adjoint_form only: inside the one-launch adjoint iteration of narrow nets */ };
int gnn_train_forms(int n_layers, const int *dims, const int *acts, const float *rates, int64_t n_rows, int producer_dropout, int *out);
int gnn_loop_train_forms(const gnn_loop *l, int net, int *out);
/* Small batches on a single GPU run the training-mode forward of ALL bodies of net_state - the `while` of gnn_loop_train_forward /
 * gnn_loop_train_step - in ONE persistent launch (one workgroup per BatchNormalization row chunk of 32 to 64 rows, one grid barrier per body,
 * two with BatchNormalization), bit-identical to one launch per kernel and body: same k, state, outputs, loss, statistics and gradients.  The
 * backward pass, net_output, the loss and the optimizer are launched as ever.  It is OPT-IN (off until gnn_loop_set_train_persistent(l, 1, ..):
 * on MUTAG batches of 32 it measured slower than the per-body launches) and then taken when all of this holds:
 *   - net_state has 2 to 4 Dense layers, fewer than 4,096 rows, no softmax before its last layer and no Dropout anywhere (in front of a
 *     Dense layer or of BatchNormalization); at least one row, max_iter >= 1;
 *   - the caches of max_iter bodies fit GNN_TRAIN_PERSISTENT_MAX_BYTES: per body the arrays [rows, width] of the concat, of every Dense
 *     output and, counted whether or not the net has a BatchNormalization, two more of the state width and [chunks, 2 width], each rounded
 *     up to 64 floats (the arena holds max_iter bodies then, not k + a few); its row tiles fit a workgroup's LDS;
 *   - one GPU, not disabled by gnn_loop_set_persistent(l, 0), not profiling, every workgroup resident at once (occupancy query x CUs).
 * Everything else takes one launch per kernel and body.  A launch whose barrier times out (bounded spins) only sets a status word: the
 * host resets the step's scratch, repeats the forward launch by launch, counts the event and keeps this loop to per-body launches until
 * the next gnn_loop_set_train_persistent.  enable = 0 forbids the persistent forward; *used (may be NULL): whether a forward without
 * Dropout in net_state would take it on this loop now. */
#define GNN_TRAIN_PERSISTENT_MAX_BYTES (256u << 20)
int gnn_loop_set_train_persistent(gnn_loop *l, int enable, int *used);
/* The part of that decision that the net, the rows and the byte cap make - host code, no device; arguments as gnn_train_forms (net_state).
 * out receives 5 ints: out[0] = 1 taken / 0 not (then out[1 .. 3] are 0); out[1] = workgroups; out[2] = rows per workgroup; out[3] = bytes
 * of LDS per workgroup; out[4] = bytes one body counts towards the cap. */
int gnn_train_persistent_form(int n_layers, const int *dims, const int *acts, const float *rates, int64_t n_rows, int max_iter, int *out);
/* What the last training forward of this loop did: out[0] = 1 when its bodies ran in the persistent launch, out[1] = workgroups and
 * out[2] = grid barriers per body of that launch (0 otherwise); out[3] = time-out fall-backs of this loop so far. */
int gnn_loop_train_info(const gnn_loop *l, int *out);
/* Recomputation of the bodies' activations in the UNROLLED training step (opt-in, off by default; with it off every launch, allocation and
 * result is unchanged).  Back-propagation through the unrolled loop otherwise keeps every body's cache - concat, Dense outputs, Dropout keep
 * bytes, xhat - from the forward pass until the backward pass reaches it.  With the mode on, the bodies of gnn_loop_train_forward /
 * gnn_loop_train_step run launch by launch (same chunks, gates and k) and keep only: the body's output state table, its BatchNormalization
 * batch statistics and its gate words; everything else is scratch that the next body reuses.  gnn_loop_train_backward rebuilds body i's cache
 * from the state body i read, immediately before that body's backward pass: the same input kernel, the same forward form, the same Dropout
 * stream (seed, net 0, body i) or slice of the injected masks.  Every reduction has a fixed order, so the rebuilt cache holds the first
 * pass's bits and every result of the step - loss, k, gradients, statistics, d_nodes, d_arc_labels - equals the default step's bit for bit.
 * A replayed body is no BatchNormalization call (call count, recorded statistics and moving statistics are the first pass's; it recomputes
 * the statistics into scratch) and evaluates no gate.  It is the reference's gradient, for every net the unrolled step handles.
 *   enable   0 off; 2 on with the ordinary (caching) kernels in the first pass instead of the cache-less forms (A/B runs); any other value on
 *   *used    (may be NULL) whether a training forward of this loop would take the mode now
 * enable != 0 on a loop of world > 1: GNN_ERR_UNSUPPORTED (the mode is single-GPU, like the training step).  In gradient modes 1 and 2
 * (gnn_loop_set_gradient_mode) the setting is accepted and has no effect (*used = 0): one body is recorded there anyway.  With the mode on,
 * the persistent training forward is not taken (gnn_loop_train_info reports 0), and gnn_loop_train_mask for net 0 returns GNN_ERR_STATE
 * after such a forward: the keep bytes of net_state are not alive (net 1 and gnn_loop_train_forms answer as ever). */
int gnn_loop_set_train_recompute(gnn_loop *l, int enable, int *used);
/* out[3]: out[0] = 1 when the last training forward of this loop ran state-only; out[1] = bodies replayed by the last backward pass (k after
 * a complete one); out[2] = the form of net_state in the first pass: 1 when the cache-less three-layer chain (k_fwd3_split without its a0 / a1
 * stores) was launched, 0 when the ordinary kernels ran on scratch. */
int gnn_loop_train_recompute_info(const gnn_loop *l, int *out);
/* Introspection for tests: the keep bytes (1 = kept) that the last gnn_loop_train_forward / gnn_loop_train_step of this loop recorded for the
 * Dropout at position pos (0 .. n_layers, the index of dropout_state / dropout_output) of net 0 (net_state, in body `body` < k) or 1
 * (net_output, body ignored) - the mask that was APPLIED, whether injected or drawn.  *count = rows * width of that position (this rank's rows /
 * masked rows); out [*count] may be NULL to ask for the count alone.  Valid from the forward until the next training forward of the loop:
 * the bytes stay intact through gnn_loop_train_backward, the optimizer step and inference runs (they live in the step's scratch, which
 * only the next training forward reuses).  GNN_ERR_STATE before the first training forward; GNN_ERR_ARG for body >= k, a position whose
 * rate is 0, a net other than 0 / 1. */
int gnn_loop_train_mask(const gnn_loop *l, int net, int body, int pos, uint8_t *out, int64_t *count);
/* What the fused inference paths (impl 1 / 2, the persistent launch) make of a net_state of this description - dims [n_layers + 1], acts
 * [n_layers] (gnn_activation codes), node-label columns in the concat; host code, no device, the decision the loops themselves take.
 * out receives 6 ints: out[0] = 1 covered / 0 not (then the rest is 0); out[1] = activation of the hidden layers; out[2] = activation of
 * the last layer; out[3], out[4] = 32-feature tiles of the hidden layers and of the last layer in the instantiated kernel (NT, NTL);
 * out[5] = 1 when the last layer's activation differs from the hidden one. */
int gnn_fused_net_form(int n_layers, const int *dims, const int *acts, int n_label_cols_in_concat, int *out);
/* Which persistent launch (gnn_loop_set_persistent) a net_state of this description takes on n_rows owned nodes, as far as the net and
 * the node count decide it - host code, no device, the decision the loops themselves take; single GPU, "not disabled" and "not profiling"
 * are the loop's part.  out receives 3 ints: out[0] = nodes per tile of the launch, 16 or 32, or 0 = no persistent launch (then the
 * rest is 0); out[1] = 1 for the form with hidden layers up to 64 wide, 0 for the form with every layer <= 32; out[2] = K-steps of
 * the first layer the kernel keeps in registers (of 4 concat columns on 16-node tiles, of 2 on 32-node tiles). */
int gnn_small_form(int n_layers, const int *dims, const int *acts, int n_label_cols_in_concat, int64_t n_rows, int *out);
/* per-kernel HIP-event timing of the last gnn_loop_run when profiling was enabled:
 * avg_iter_ms = mean duration of the per-iteration kernel(s), total_ms = whole loop on the stream. */
int gnn_loop_set_profiling(gnn_loop *l, int enable);
/* The label aggregates ArcNode^T . arc labels and Adjacency^T . node labels (GNN/GNN.py:259, :263) do not depend on the state:
 * the fused path builds them on the first run and keeps them until the labels change (gnn_graph_update_labels).  This call
 * drops them - and the label projection built from them (gnn_loop_set_label_projection) - so that the next gnn_loop_run pays for them
 * like every Loop() of the reference does (bench.py: cold figure). */
int gnn_loop_drop_cached_aggregates(gnn_loop *l);
int gnn_loop_get_timing(const gnn_loop *l, float *total_ms, float *avg_iter_ms, int *n_iter_timed);
/* With profiling on: mean time on the loop's stream between the end of one body's kernel(s) and the start of the next body's, over the last
 * run - on shards that is the per-iteration exchange (the reads of `state` at reference GNN/GNN.py:234 and the reduce_any of :218 that span
 * all nodes: all-gather of state rows / boundary rows + flag block, or the sliced layout's pack, all-to-all, aggregation, all-to-all, unpack);
 * a few microseconds of launch gap on one GPU.  0 unless gnn_loop_set_profiling was on. */
int gnn_loop_get_exchange_timing(const gnn_loop *l, float *avg_between_bodies_ms);
/* Work counters of one iteration of this loop on this rank and the timing of its last run (SURVEY.md 8b "gnn_counters_get"):
 * algorithmic bytes per iteration = E (4 Ds + 8) + 4 (n_rows + 1) + n_rows (8 Ds + 4 (2 NL + AL)) over the OWNED rows (SURVEY.md
 * 8d: fp32 values, int32 indices, no cache credit, fused iteration), FLOPs per iteration = n_rows 2 sum_l in_l out_l + 2 E Ds;
 * iterations / total_ms / avg_iteration_ms as gnn_loop_get_timing (the times are 0 unless gnn_loop_set_profiling was on).
 * Any output pointer may be NULL. */
int gnn_counters_get(const gnn_loop *l, double *bytes_per_iteration, double *flops_per_iteration, int *iterations, float *total_ms,
                     float *avg_iteration_ms);
/* LGNN.Loop (reference GNN/LGNN.py:263-290) in one call: loops[i] was created on graphs[i]; graphs[0] is the ORIGINAL graph `base`,
 * graphs[i > 0] derived from it (gnn_graph_derive / _derive_edge; the same derived graph may serve several layers).  Runs layer 0,
 * relabels graphs[1] from `base` with layer 0's state / output (gnn_graph_update_labels: LGNN.py:227-260, :287), runs layer 1, ...
 * k_out[n_layers] receives the iteration count of every layer (K of the reference); state / outputs of every layer stay readable
 * through gnn_loop_get_state / gnn_loop_get_output (or gnn_loop_readout) of its loop.  Single GPU or one rank of an RCCL job. */
int gnn_lgnn_run(gnn_loop *const *loops, gnn_graph *const *graphs, int n_layers, int get_state, int get_output, float *k_out);
/* A loop created on a communicator may be destroyed before or after it: gnn_comm_destroy with loops alive only marks the
 * communicator closed, the last gnn_loop_destroy releases it. */
int gnn_loop_destroy(gnn_loop *l);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) -------------------------------------------------------------
 * No reference counterpart: the reference is single-device.  What is sharded is the row-wise work of convergence()
 * (GNN/GNN.py:223-242: sparse_dense_matmul(adjacency, state) at :234 needs neighbour rows of other ranks) and the global
 * reduce_any of condition() (:218).  Nodes are sharded by contiguous ranges; every iteration ends with one grouped RCCL
 * all-gather of the owned state rows (or, for shards created by gnn_graph_create_halo, of the owned BOUNDARY rows only)
 * and the owned convergence flag.  The 128-byte id is produced on rank 0 and handed to the other ranks by the caller
 * (file, socket, torch.distributed store ...). */
int gnn_shard_range(int64_t n_nodes, int rank, int world, int64_t *row_begin, int64_t *n_rows);   /* owned rows of a rank */
int gnn_comm_unique_id(uint8_t id[128]);
int gnn_comm_create(const uint8_t id[128], int rank, int world, int device, gnn_comm **out);
int gnn_comm_allreduce_max(gnn_comm *c, double *value);   /* barrier + max over ranks (bench timing) */
int gnn_comm_destroy(gnn_comm *c);
/* Boundary ("halo") exchange.  gnn_halo_plan (host only, needs the CSR-by-destination of the WHOLE graph): slot[v] =
 * position of node v among the boundary rows of its owner (rows read by another rank), -1 for interior nodes; counts[q] =
 * boundary rows of rank q; *block = max count.  gnn_graph_create_halo builds rank r's shard in the compact index space
 *   [0, shard) owned rows | shard + q * block + slot: boundary rows of rank q
 * (adj_src_replica and the rows of nodes_replica are given in that space; send_rows = ascending owned-row indices of this
 * rank's boundary rows).  Loops on such a graph all-gather `block` rows per rank and iteration instead of whole shards.
 * LGNN relabelling and the edge-based readout are not available on halo shards. */
int gnn_halo_plan(int64_t n_nodes, int world, const int32_t *indptr, const int32_t *adj_src, int32_t *slot /* [n_nodes] */,
                  int64_t *counts /* [world] */, int64_t *block);
int gnn_graph_create_halo(int64_t n_nodes_global, int rank, int world, int64_t halo_block, int64_t n_send, const int32_t *send_rows,
                          int64_t n_arcs, const int32_t *indptr, const int32_t *adj_src_replica, const float *adj_w,
                          const float *arc_w, const float *arc_labels, int dim_arc_label, const float *nodes_replica,
                          int dim_node_label, const uint8_t *mask, int device, gnn_graph **out);
/* Feature-sliced exchange for node-range shards with full-replica numbering (an alternative to exchanging state ROWS).  The
 * aggregation tf.sparse.sparse_dense_matmul(adjacency, state) (reference GNN/GNN.py:234) is independent per state column, so rank q
 * aggregates columns [q Ds / P, (q + 1) Ds / P) for ALL nodes over the whole graph's adjacency, and two all-to-all steps per
 * iteration move column slices of the owned rows in and aggregated slices back: 2 (P - 1) / P^2 of N Ds floats received per rank
 * and iteration instead of (P - 1) / P (56 MB instead of 224 MB at N = 1 M, Ds = 64, P = 8).  Bit-identical results.
 *   gnn_graph_set_full_adjacency  the whole graph's CSR by destination (global ids) beside the shard's own rows
 *   gnn_loop_set_slice_exchange   on != 0: use it (Ds must be a multiple of the world size); every rank of the job alike.
 *                                 on == 1: the slice is aggregated in P row blocks (one per destination rank, in the order rank + 1, ...,
 *                                 rank) and block t is sent on a second stream while block t + 1 is aggregated - the return all-to-all is
 *                                 hidden behind the aggregation except for the rank's own block; on == 2: the whole slice, then one grouped
 *                                 all-to-all (kept for comparison) */
int gnn_graph_set_full_adjacency(gnn_graph *g, int64_t n_global, const int32_t *indptr, const int32_t *adj_src, const float *adj_w);
int gnn_loop_set_slice_exchange(gnn_loop *l, int on);
/* In-process LOOPBACK group: `world` communicators on ONE device sharing one stream; the exchange steps become
 * device-to-device copies between the members' buffers.  It runs the sharded code path (row offsets, padded replicas,
 * per-rank flag slots, every exchange call site) on a single GPU; used by the parity tests, never for speed.  One loop per
 * rank and group; the ranks of a group are driven together by the *_group entry points (k, readout: rank 0's values, after
 * checking that all ranks agree). */
int gnn_comm_create_loopback(int world, int device, gnn_comm **out /* [world] */);
int gnn_loop_run_group(gnn_loop **loops, int n, float *k_out);
int gnn_loop_readout_group(gnn_loop **loops, int n, int n_graphs, const int32_t *ng_indptr, const int32_t *ng_node,
                           const float *ng_w, float *out_graph);
int gnn_graph_update_labels_group(gnn_graph **dsts, gnn_graph *const *bases, gnn_loop *const *froms, int n, int get_state,
                                  int get_output);

#ifdef __cplusplus
}
#endif
#endif /* GNN_HIP_H */
