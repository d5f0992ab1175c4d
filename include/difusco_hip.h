/*
 * difusco_hip.h - C ABI of the MI355X-native (gfx950) DIFUSCO denoise-step library.
 *
 * Drop-in boundary.  The reference has no FFI: its boundary is two Python methods,
 *   TSPModel.categorical_denoise_step / gaussian_denoise_step   (difusco/pl_tsp_model.py:122-151)
 *   MISModel.categorical_denoise_step / gaussian_denoise_step   (difusco/pl_mis_model.py:118-140)
 * which call GNNEncoder.forward (difusco/models/gnn_encoder.py:452-462) and
 * COMetaModel.categorical_posterior / gaussian_posterior (difusco/pl_meta_model.py:102-175).
 * This header declares what a binding for that path needs: plain pointers and sizes, no torch types.
 * All device pointers are HIP device memory of the current device; `stream` is a hipStream_t.
 * Every function returns 0 on success, a negative DIFUSCO_E* code otherwise; difusco_last_error()
 * gives the message of the calling thread's last failure.
 *
 * The binding a reference maintainer would add (ctypes) is shown in INTEGRATION.md; the in-tree
 * Python host side is difusco_amd/ (same method names and argument meaning as the reference).
 */
#ifndef DIFUSCO_HIP_H
#define DIFUSCO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIFUSCO_ABI_VERSION 13

enum {
  DIFUSCO_OK = 0,
  DIFUSCO_EINVAL = -1,      /* bad argument (shape, null pointer, unsupported hidden size ...) */
  DIFUSCO_EWORKSPACE = -2,  /* workspace too small */
  DIFUSCO_EHIP = -3,        /* a HIP runtime call failed */
  DIFUSCO_EUNSUPPORTED = -4, /* a combination the library has no kernel for */
  DIFUSCO_ENONFINITE = -5    /* DIFUSCO_FLAG_CHECK_FINITE: the step produced inf / nan */
};

enum { DIFUSCO_TASK_TSP = 0, DIFUSCO_TASK_MIS = 1 };            /* edge features | node features only */
enum { DIFUSCO_CATEGORICAL = 0, DIFUSCO_GAUSSIAN = 1 };
/* neighbourhood aggregation of the GNN layers (--aggregation, train.py:52; gnn_encoder.py:170-191): every published run uses sum.
 * MAX combines messages with fmaxf, which returns the non-NaN operand: a NaN message is DROPPED where torch.max / segment_csr(max)
 * would propagate it into h.  A non-finite state still surfaces through e (and DIFUSCO_FLAG_CHECK_FINITE sees it there). */
enum { DIFUSCO_AGG_SUM = 0, DIFUSCO_AGG_MEAN = 1, DIFUSCO_AGG_MAX = 2 };
enum {
  DIFUSCO_PREC_FP32 = 0,   /* E-row linears on v_mfma_f32_32x32x2_f32: exact fp32 (k-ordered fma chain) */
  DIFUSCO_PREC_BF16X3 = 1, /* 2 bf16 planes, 3 products: ~2^-17 relative per product                    */
  DIFUSCO_PREC_BF16X6 = 2, /* 3 bf16 planes, 6 products: all 24 significand bits, fp32-class accuracy    */
  DIFUSCO_PREC_FP16X3 = 3, /* 2 fp16 planes, 3 products, operands pre-scaled by exact powers of two into the upper
                              binades of fp16 (weights per matrix / per row on the host, activations per row or per
                              32-edge tile on the device): 22 significand bits for elements within 2^-17 of the
                              largest element of their scaling group, an absolute floor of 2^-39 of that largest
                              element below; any finite fp32 operand scale (no |x| < 65504 restriction)            */
  DIFUSCO_PREC_FP16X1 = 4  /* half-precision edge GEMMs (the reference's --fp16, Trainer(precision=16), rounds the operands
                              of these Linears to fp16 under autocast): every product of the edge-row GEMMs of the
                              layers, C and per_layer_out[l][2] (gnn_encoder.py:104,344), takes ONE fp16 product.  Both
                              operands are scaled by the powers of two of FP16X3 (weights: the hi fp16 plane of the
                              existing planes, no layout change; activations: per row, per 32-edge tile, or for the fused kernel's
                              second GEMM per layer from the bound of DIFUSCO_WL_FUSED_SCALES), rounded once
                              to fp16 (RNE), multiplied exactly and accumulated in fp32; the outputs stay fp32.  Layer 0
                              on the two-row table (the L0 fold, difusco_prepare) follows the same rule.  Everything else
                              - edge embedding, node linears, time MLP, head, posteriors - runs as FP16X3; e / h stay
                              fp32.  difusco_edge_embed does not take it (the embedding has no FP16X1 form). */
};
enum {
  DIFUSCO_RAND_NONE = 0,     /* no draw: categorical final step (target_t == 0) or DDIM */
  DIFUSCO_RAND_INJECTED = 1, /* caller supplies uniforms (categorical) / normals (gaussian DDPM) */
  DIFUSCO_RAND_PHILOX = 2,   /* on-device Philox4x32-10 keyed by (seed, offset, element) */
  DIFUSCO_RAND_PHILOX_INSTANCES = 3 /* ABI 13: Philox keyed per instance of a batched call: output row r of instance b
                                       draws with (instance_seeds[b], offset, r - instance_rows[b]), the draw of a solo
                                       call of that instance with seed = instance_seeds[b] (difusco_step_args) */
};

int difusco_abi_version(void);
const char* difusco_last_error(void);

/* ---- weights ---------------------------------------------------------------------------------
 * The packed fp32 blob holds every tensor of the reference GNNEncoder state_dict
 * (gnn_encoder.py:303-347; key set in SURVEY.md section 5) plus three host-computed constant
 * tables (timestep frequencies nn.py:114-116, the two `dim_t` vectors gnn_encoder.py:215,243).
 * difusco_weights_layout() is the single source of truth for the offsets (in floats). */
enum {
  DIFUSCO_W_NODE_EMBED_W = 0, DIFUSCO_W_NODE_EMBED_B,
  DIFUSCO_W_EDGE_EMBED_W, DIFUSCO_W_EDGE_EMBED_B,
  DIFUSCO_W_TIME0_W, DIFUSCO_W_TIME0_B, DIFUSCO_W_TIME2_W, DIFUSCO_W_TIME2_B,
  DIFUSCO_W_OUT_GN_W, DIFUSCO_W_OUT_GN_B, DIFUSCO_W_OUT_CONV_W, DIFUSCO_W_OUT_CONV_B,
  DIFUSCO_W_TIME_FREQS,  /* [H/2]  exp(-ln(1e4) k/(H/2))                      */
  DIFUSCO_W_DIMT_POS,    /* [H/2]  1e4^(2(k/2)/(H/2))  PositionEmbeddingSine   */
  DIFUSCO_W_DIMT_SCALAR, /* [H]    1e4^(2(k/2)/H)      ScalarEmbeddingSine(1D).  REQUIRED: entries 2j and 2j+1 are EQUAL (the
                            reference's table, gnn_encoder.py:243): the generated-input kernels (edge_embed.hip, the GEN path of
                            linear_split.hip) take ONE sincos of x / dim_t[2j] for the (sin, cos) feature pair (2j, 2j+1); a blob
                            with another table diverges from scalar_embed_kernel.  pack_state_dict() asserts it. */
  DIFUSCO_W_EDGE_EMBED_PLANES, /* bf16 split planes of edge_embed.weight, see below */
  DIFUSCO_W_GLOBAL_COUNT
};
enum {                       /* per layer l, index = GLOBAL_COUNT + l*LAYER_COUNT + id */
  DIFUSCO_WL_NODE4_W = 0,    /* [4H,H] rows: U | V | A | B  (gnn_encoder.py:52-55)  */
  DIFUSCO_WL_NODE4_B,        /* [4H]                                                */
  DIFUSCO_WL_C_W, DIFUSCO_WL_C_B,
  DIFUSCO_WL_NORM_H_W, DIFUSCO_WL_NORM_H_B, DIFUSCO_WL_NORM_E_W, DIFUSCO_WL_NORM_E_B,
  DIFUSCO_WL_TIME_W, DIFUSCO_WL_TIME_B,      /* time_embed_layers[l].1 : [H,H/2],[H] */
  DIFUSCO_WL_OUT_LN_W, DIFUSCO_WL_OUT_LN_B,  /* per_layer_out[l].0                   */
  DIFUSCO_WL_OUT_W, DIFUSCO_WL_OUT_B,        /* per_layer_out[l].2 : [H,H],[H]       */
  DIFUSCO_WL_C_PLANES, DIFUSCO_WL_OUT_PLANES, /* split planes of C / per_layer_out[l].2 */
  DIFUSCO_WL_NODE4_PLANES,                    /* split planes of the [4H,H] node linear (U|V|A|B) */
  DIFUSCO_WL_FUSED_SCALES,                    /* 8 floats: operand scales of the fused edge kernel, see below */
  DIFUSCO_WL_NODE4_FUSED_B,                   /* [4H]   bias of the node linear as the FUSED edge kernel wants its rows, see below (ABI 11) */
  DIFUSCO_WL_NODE4_FUSED_S,                   /* [2][4H] column scales of the node linear for the fused path: fp16 planes | bf16 planes   */
  DIFUSCO_WL_COUNT
};
/* "*_PLANES" entries: the [H,H] weight w decomposed on the host into five 16-bit planes
 *   bf16: hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid)      (round to nearest even)
 *   fp16: hi = fp16(w), lo = fp16(w - hi)
 * stored back to back in that order (plane stride H*H elements), each plane laid out
 * [H/16 slabs][H rows][16] with slab position j holding k = 16 s + {0..3, 8..11, 4..7, 12..15}[j]
 * (the order in which an MFMA accumulator feeds the next MFMA, see linear_split.hip).
 * The fp16 planes are those of the SCALED matrix w[f][:] * 2^k_f, k_f chosen on the host so that the largest scaled
 * magnitude of the scaling group lies in [2^14, 2^15) (one group per matrix for C / per_layer_out / edge_embed, one per
 * output row for the node linear); the n_out floats that follow the five planes hold 2^-k_f.  Without the scale the
 * low plane of any |w| < 2^-3 would be an fp16 subnormal with an absolute 2^-25 floor.  The bf16 planes are unscaled
 * (bf16 has the fp32 exponent range).
 * 5*n_out*k 16-bit elements + n_out floats = 2.5*n_out*k + n_out floats of blob space per matrix.  They feed the
 * split-precision MFMA paths selected by difusco_step_args.precision.
 * DIFUSCO_WL_FUSED_SCALES = {log2(e) 2^-kc, 2^-(ko+ka) / log2(e), log2(e), 2^-ka, 0, 0, 0, 0}: kc / ko the plane scales of C /
 * per_layer_out[l][2]; 2^ka the scale under which the fused kernel produces the GEMM 2 operand a log2(e), a = SiLU(LN_o(.)), from
 * the bound |a| <= max(16 max|g_o| + max|b_o|, 0.2785) (|LayerNorm| <= sqrt(H-1) < 16).  difusco_amd/weights.py computes
 * all of it (fused_scales); the e operand of GEMM 1 is scaled per 32-edge tile on the device.
 * ABI 11, "log2(e) domain": the fused edge kernel carries the gate pre-activation e' = A h[j] + B h[i] + C e + b_C as e' log2(e)
 * (sigmoid = 1 / (1 + exp2(-.)) without a multiply; LayerNorm is scale invariant).  Its neighbour-table rows node4[:, 2H:4H]
 * therefore hold (A h + b_A + b_C) log2(e) | (B h + b_B) log2(e): on the fused path the node linear is run with
 * DIFUSCO_WL_NODE4_FUSED_B = {b_U, b_V, (b_A + b_C) log2(e), b_B log2(e)} as its bias and with the per-column accumulator scales
 * DIFUSCO_WL_NODE4_FUSED_S (row 0: 2^-k_f of the fp16 planes, times log2(e) on the A | B columns; row 1, unscaled bf16 planes:
 * 1 | 1 | log2(e) | log2(e)).  The U | V columns are unchanged.  The unfused kernels read node4 as the reference defines it. */
/* Fills offsets[0 .. GLOBAL_COUNT + n_layers*WL_COUNT) (floats from blob start) and *total_floats.
 * Returns the number of entries, or a negative error. */
int difusco_weights_layout(int hidden, int n_layers, int out_channels,
                           int64_t* offsets, int max_entries, int64_t* total_floats);

/* ---- graph -----------------------------------------------------------------------------------
 * HOST helper (no GPU needed): COO int64 edge list (2 x E, reference layout
 * co_datasets/tsp_graph_dataset.py:53-62, mis_dataset.py:43-48, duplicate_edge_index
 * pl_meta_model.py:177-184) -> CSR over the centre node edge_index[0], stable in the caller's edge
 * order.  rowptr[n_nodes+1], col[E] (= edge_index[1] in CSR order), row[E], perm[E] (CSR slot ->
 * caller edge id).  *identity = 1 when the input was already row-sorted (perm[s] == s). */
int difusco_csr_from_coo_host(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes,
                              int32_t* rowptr, int32_t* col, int32_t* row, int32_t* perm,
                              int* identity);

/* The same conversion on the DEVICE, with the optional node renumbering of difusco_amd/graph.py (build_csr): the outputs are bit
 * for bit the arrays the host path produces for the same input.  edge_index: DEVICE int64 [2, n_edges] (row 0 = centre node);
 * points: DEVICE [n_nodes, 2], float32 (points_f64 = 0) or float64 (points_f64 = 1), or NULL = no renumbering.  With points the
 * nodes are renumbered first (graph.py locality_node_order): inside every block of node ids that no edge leaves (_id_blocks) by
 * the 2 x 16-bit Morton key of the coordinates over the bounding box of the call, computed in float64 (_morton_keys), ties in id
 * order; node_order[new] = old (DEVICE int64 [n_nodes]).  As on the host the renumbering is skipped (node_order not written, the
 * ORDER_IDENTITY flag set) when points is NULL, n_nodes <= 1 or n_edges == 0.  rowptr [n_nodes + 1], col / row / perm [n_edges]:
 * DEVICE int32, the stable sort of the edges by (renumbered) centre node, perm[slot] = caller edge id, col renumbered.
 * flags_out: HOST uint32 [2]: [0] = DIFUSCO_GRAPH_* bits, [1] = the smallest edge id with an endpoint outside [0, n_nodes) when
 * DIFUSCO_GRAPH_BAD_EDGE is set.  Such an edge is never used as an index; the call then returns DIFUSCO_EINVAL (the message
 * names the edge like the host helper's) and the outputs are unspecified.  Runs on `stream`, copies the flags back (the one
 * device-to-host copy of the call) and synchronises the stream: on return the arrays are complete.  Limits as the host helper:
 * n_edges <= INT32_MAX, n_nodes < INT32_MAX.  DIFUSCO_EINVAL before any GPU work on: a negative or too large size, a null
 * rowptr / flags_out / workspace, a null edge_index / col / row / perm with n_edges > 0, a null node_order when the renumbering
 * runs, points_f64 outside {0, 1}, a workspace smaller than difusco_graph_build_workspace_bytes (with_points: points != NULL). */
#define DIFUSCO_GRAPH_PERM_IDENTITY 1u  /* perm[s] == s for every slot: the input was row-sorted (after the renumbering) */
#define DIFUSCO_GRAPH_ORDER_IDENTITY 2u /* node_order[i] == i for every node, or no renumbering ran */
#define DIFUSCO_GRAPH_BAD_EDGE 4u
int difusco_graph_build_workspace_bytes(int64_t n_nodes, int64_t n_edges, int with_points, size_t* bytes);
int difusco_graph_build(int64_t n_nodes, int64_t n_edges, const int64_t* edge_index, const void* points, int points_f64,
                        int32_t* rowptr, int32_t* col, int32_t* row, int32_t* perm, int64_t* node_order, uint32_t* flags_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- the denoise step -------------------------------------------------------------------------- */
typedef struct difusco_step_args {
  uint32_t struct_size;   /* = sizeof(difusco_step_args), checked */
  uint32_t abi_version;   /* = DIFUSCO_ABI_VERSION */

  /* model */
  int32_t hidden;         /* 64 | 128 | 256 (reference default 256, train.py:50) */
  int32_t n_layers;
  int32_t out_channels;   /* 2 categorical | 1 gaussian (pl_meta_model.py:28-35) */
  int32_t task;           /* DIFUSCO_TASK_* */
  const float* weights;   /* device, packed per difusco_weights_layout */

  /* graph: disjoint union of the graphs of this call, CSR over centre node (device) */
  int32_t n_nodes, n_edges;
  const int32_t* rowptr;  /* [n_nodes+1] */
  const int32_t* col;     /* [n_edges] */
  const int32_t* perm;    /* [n_edges] CSR slot -> caller edge id, or NULL (identity) */
  /* statistic segments of the head GroupNorm over output rows (edges for TSP, nodes for MIS), in
   * CSR-slot / node order.  n_segments = 1, seg_ptr = {0, rows} reproduces the reference's sparse
   * call (one statistic over ALL graphs of the call, gnn_encoder.py:400-401); one
   * segment per graph reproduces the dense path (gnn_encoder.py:380).  Device pointer; may be
   * NULL when n_segments == 1. */
  int32_t n_segments;
  const int32_t* seg_ptr; /* device, [n_segments+1] */

  /* inputs (device) */
  const float* points;    /* [n_nodes,2]  TSP only */
  const float* xt;        /* TSP: [n_edges] caller edge order;  MIS: [n_nodes] */
  float t;                /* diffusion time t (shared by the whole call, pl_tsp_model.py:124) */
  int32_t xt_is_binary;   /* 1: xt is exactly 0/1 (categorical inference): 2-row embedding table */

  /* posterior */
  int32_t diffusion;      /* DIFUSCO_CATEGORICAL | DIFUSCO_GAUSSIAN */
  /* categorical: post[0..3] = c0[xt=0], c0[xt=1], c1[xt=0], c1[xt=1] with
   *   p(x_s=1) = c0[xt]*p0 + c1[xt]*p1   (pl_meta_model.py:125-137; host computes them in fp32)
   *   post[4] = 1 if target_t > 0 (Bernoulli draw) else 0 (clamp(min=0), :139-142)
   * gaussian : x_s = post[0]*(xt - post[1]*pred) + post[2]*pred + post[3]*z  (:161-172) */
  float post[8];
  int32_t rand_mode;      /* DIFUSCO_RAND_* */
  const float* rand;      /* injected uniforms / normals, caller order, or NULL */
  uint64_t seed, offset;  /* Philox key / per-call offset */

  /* outputs (device) */
  float* xt_out;          /* same shape/order as xt */
  float* pred_out;        /* optional: logits [rows,2] (categorical) or eps [rows] (gaussian) */
  float* prob_out;        /* optional, categorical: p(x_s=1) before clamping/sampling, [rows] */

  void* workspace;        /* device, >= difusco_workspace_bytes(...) */
  size_t workspace_bytes;
  void* stream;           /* hipStream_t */
  int32_t precision;      /* DIFUSCO_PREC_*: arithmetic of the E-row linears (node rows stay exact fp32) */
  int32_t no_fusion;      /* 0: use the fused edge-layer kernel when available (hidden == 256 and precision
                             BF16X3 / FP16X3); 1: always run the unfused kernel sequence (A/B and parity tests) */
  const int32_t* row;     /* [n_edges] centre node of each CSR slot (device); required for the fused kernel,
                             may be NULL otherwise */
  /* Head GroupNorm statistics across several calls (one per GPU of a sharded batch), SURVEY 8(e) option "global
   * statistics" = the reference's single call over all graphs.  gn_phase 0: the whole step in one call (statistics
   * of THIS call's rows).  1: run up to the statistics, write the 32 x (sum, sum of squares) of this call's rows
   * and the row count to gn_sums[0..63], gn_sums[64] (device doubles) and return; the caller adds gn_sums over the
   * shards (e.g. one all-reduce of 65 doubles).  2: finish the step of the preceding phase-1 call (same arguments,
   * same workspace) with the statistics in gn_sums.  Needs n_segments == 1. */
  int32_t gn_phase;
  int32_t flags;          /* DIFUSCO_FLAG_*: per-call A/B switches of the fused path (results equal to rounding) */
  double* gn_sums;
  /* Optional PREPARED STATE (ABI 9).  Both NULL = the stateless step: everything is computed from the arguments above.
   * A sampling loop calls the step 50 times with the same weights, graph and coordinates (pl_tsp_model.py:207-217); what
   * does not depend on x_t or t is then computed ONCE and handed back in:
   *   prepared  (TSP, fused path): the buffer difusco_prepare() filled for THIS (weights, precision, graph, points): the
   *             node embedding h0 = node_embed(pos_embed(points)) (gnn_encoder.py:394), layer 0's U|V|A|B rows of it and the
   *             two-row edge-input table of a categorical step - the step then skips those launches.  Ignored on the
   *             unfused path and for MIS (whose h0 is the embedding of x_t).
   *   tbias     [n_layers, hidden] time-bias rows of THIS t (difusco_time_bias_rows(); gnn_encoder.py:396,329-337,442) - the
   *             step skips the time MLP.
   * Same kernels, same operands: a step with prepared state is bit-identical to the stateless one (GPU test). */
  const void* prepared;
  const float* tbias;
  /* ABI 10.  DIFUSCO_AGG_*: h_i = U h_i + Aggr_j(gate_ij * V h_j) over the edges of centre node i (gnn_encoder.py:115,144-191).
   * SUM: torch_sparse.sum / torch.sum(dim=2).  MEAN: the sum divided by the number of edges of the row (torch_sparse.mean =
   * segment mean; the dense layer divides by sum(ones) = V).  MAX: the maximum over the row's edges (torch_sparse.max /
   * torch.max(dim=2)[0]); an empty row aggregates to 0 in all three.  MEAN runs the fused layers (the division happens where the
   * pieces of a row are added); MAX has fused instantiations of its own (the per-tile pieces of a row are maxima); only a MAX call
   * with n_nodes >= 2^20 takes the unfused kernel sequence. */
  int32_t aggregation;
  int32_t reserved0;      /* 0 */
  /* ABI 12.  Optional GENERATED-INPUT TABLE (TSP, fused path, hidden 256): the buffer difusco_gen_table_build() filled for THESE weights.
   * A step whose edge input is not a two-row lookup (Gaussian diffusion; a categorical x_t that is not exactly {0,1}) computes
   * e0 = edge_embed(ScalarEmbeddingSine(x_t)) (gnn_encoder.py:230-249,:304,:395): a function of ONE scalar per edge.  With the table,
   * every 32-edge tile whose x_t all lie in [-8, 8) is evaluated by degree-7 interpolation of eight sampled rows (interpolation error
   * 2e-9, far below the fp32 rounding of the contraction it replaces; csrc/edge_embed.hip) instead of 64 sincos + a K = 256 contraction
   * per edge; tiles with an edge outside the table or a non-finite x_t, and NULL, take the contraction.  Results differ from the
   * table-free step by fp32 rounding only. */
  const float* gen_table;
  /* ABI 13.  Per-instance random streams of a call that batches several INSTANCES (each with its own parallel samples):
   * read with rand_mode == DIFUSCO_RAND_PHILOX_INSTANCES only, ignored otherwise.  instance_rows [n_instances + 1] (device)
   * are the output-row boundaries of the instances in CALLER order (edges for TSP, nodes for MIS; instance_rows[0] = 0,
   * instance_rows[n_instances] = rows), instance_seeds [n_instances] (device) their Philox keys.  The head statistics are
   * not affected: give every instance a statistic segment of its own (n_segments / seg_ptr) to reproduce its solo call. */
  int32_t n_instances;
  const int64_t* instance_rows;
  const uint64_t* instance_seeds;
} difusco_step_args;

enum {
  DIFUSCO_FLAG_NO_L0_FOLD = 1,   /* first layer: write e0 to memory and run the general kernel (no 2-row table fold) */
  DIFUSCO_FLAG_NO_TAIL_FOLD = 2, /* last layer: general kernel + separate GroupNorm statistics pass over e */
  DIFUSCO_FLAG_CHECK_FINITE = 4  /* debugging aid: after the step, count the non-finite values of xt_out, of the head's GroupNorm
                                    statistics (nan as soon as the final state holds an inf / nan) and of pred_out / prob_out
                                    when given, synchronise the stream and return DIFUSCO_ENONFINITE if there are any.  The
                                    arithmetic has no operand-range restriction (any finite fp32 weights / inputs), so inf / nan
                                    can only come in with the inputs or from genuine fp32 overflow of the network itself. */
};

size_t difusco_workspace_bytes(int hidden, int n_layers, int n_nodes, int n_edges, int n_segments);

/* ---- prepared state (optional, see difusco_step_args.prepared / .tbias) -------------------------------------------
 * difusco_prepared_bytes(): size of the buffer for a call shape.  difusco_prepare(): fills it from args->{hidden, n_layers,
 * out_channels, task (TSP), weights, precision, n_nodes, n_edges, points, workspace, stream} - the graph arrays, x_t and
 * the outputs are not read.  `points` must be in the node numbering of the graph arrays the later steps pass.
 * difusco_time_bias_rows(): out[i] = the [n_layers, hidden] rows of t_host[i] (HOST array, n_t values), DEVICE
 * out [n_t, n_layers, hidden]; one launch per 64 values.  All asynchronous on the stream. */
size_t difusco_prepared_bytes(int hidden, int n_nodes);
int difusco_prepare(const difusco_step_args* args, void* prepared, size_t prepared_bytes);
int difusco_time_bias_rows(int hidden, int n_layers, int out_channels, const float* weights, const float* t_host, int n_t,
                           float* out, void* stream);

/* e0 = edge_embed(ScalarEmbeddingSine(x_t)) (difusco/models/gnn_encoder.py:230-249 the features, :304,:395 the linear) for a
 * GENERAL x_t (Gaussian diffusion; a categorical x_t that is not exactly {0,1}) - the kernel the fused step runs for such inputs,
 * exported for parity tests.  hidden = 256; precision = DIFUSCO_PREC_BF16X3 | _FP16X3.  xt [n_edges] in caller order, perm (or
 * NULL) maps CSR slot -> caller index; e_tiled: the TILED edge state (layout at difusco_edge_layer_fused below), padded to a multiple of 256 rows
 * (only the n_edges real rows are written); tile_max (or NULL): one float per 32-edge tile of the padded range = max |e0| of the
 * tile (0 for tiles past the end); gen_table (or NULL): the table of difusco_gen_table_build - tiles inside its range interpolate
 * (stand-alone entry: at most 581,632 edges per call with a table; the tile flags live in the table buffer's scratch). */
int difusco_edge_embed(int hidden, int n_layers, int out_channels, const float* weights, int precision, const float* xt,
                       const int32_t* perm, int64_t n_edges, float* e_tiled, float* tile_max, const float* gen_table, void* stream);

/* The generated-input table of difusco_step_args.gen_table (ABI 12): 71 rows of e0(x) at x = -8 + (r - 3) / 4, computed with the exact
 * fp32 kernels (precise sin / cos features, fp32-MFMA linear) from the blob's edge_embed weights; depends on the weights only - build once
 * per blob.  difusco_gen_table_bytes(): size of the buffer (rows + build scratch); hidden must be 256.  Asynchronous on the stream. */
size_t difusco_gen_table_bytes(int hidden);
int difusco_gen_table_build(int hidden, int n_layers, int out_channels, const float* weights, float* table, size_t table_bytes,
                            void* stream);

/* One reverse-diffusion step: GNN denoiser forward + posterior (+ sample).  Asynchronous on
 * args->stream.  Replaces {categorical,gaussian}_denoise_step of pl_tsp_model.py / pl_mis_model.py. */
int difusco_denoise_step(const difusco_step_args* args);

/* difusco_denoise_step with a device-side shift of the Philox offset: every Philox draw of the step (categorical Bernoulli,
 * Gaussian DDPM normal; rand_mode DIFUSCO_RAND_PHILOX and DIFUSCO_RAND_PHILOX_INSTANCES) uses args->offset + *offset_shift.
 * offset_shift: device pointer to one uint64_t, read by the kernels when they run (never on the host), so a step captured
 * into a HIP graph draws fresh numbers on each replay once the caller rewrites that word; NULL = difusco_denoise_step.
 * Additive at ABI 13: difusco_denoise_step(a) is difusco_denoise_step_shifted(a, NULL). */
int difusco_denoise_step_shifted(const difusco_step_args* args, const uint64_t* offset_shift);

/* ---- single kernels, exported for parity tests and profiling ------------------------------------ */
/* Y[m, ldy] (cols [0,n_out)) = X[m,k] * W[n_out,k]^T + bias (+ residual, same layout as Y).
 * k in {32,64,128,256}; n_out multiple of 32.  fp32 MFMA (v_mfma_f32_32x32x2_f32). */
int difusco_linear_rows(const float* x, const float* w, const float* bias, const float* residual,
                        float* y, int64_t m, int k, int n_out, int64_t ldy, void* stream);
/* Same contract on the split-precision path: `planes` = the five 16-bit planes of W[n_out,k] in the
 * *_PLANES layout above (planes + inverse scales); precision = DIFUSCO_PREC_BF16X3 | _BF16X6 | _FP16X3.
 * k == n_out in {64,128,256}, or k = 256 with n_out a multiple of 256 (the node-row shape, n_out = 1024: a row-major y with
 * ldy == n_out and no residual then takes the register-resident kernel of node_linear.hip).  row_scale_scratch (device, m floats, or NULL): with FP16X3 the rows of x are scaled
 * individually by a power of two computed in an extra pass (any finite |x|); NULL skips that pass and then needs
 * 2^-3 <= |x| < 65504 for the full 22 bits. */
int difusco_linear_rows_split(const float* x, const void* planes, int precision, const float* bias,
                              const float* residual, float* y, int64_t m, int k, int n_out, int64_t ldy,
                              float* row_scale_scratch, void* stream);

/* One gated-GCN message-passing pass (gnn_encoder.py:110-135 + :445-448 + per_layer_out LN/SiLU):
 *   e' = Ah[j]+Bh[i]+Ce ; h[i] += ReLU(LN_h(Uh[i] + sum_j sigmoid(e')*Vh[j])) (+tbias, MIS)
 *   ce_act[s] <- SiLU(LN_o(ReLU(LN_e(e')) (+tbias, TSP)))      (in place over Ce)
 * node4 = [n_nodes,4H] rows U|V|A|B.  ln = {norm_h w,b, norm_e w,b, out_ln w,b} device pointers. */
int difusco_edge_gate_aggregate(int hidden, int n_nodes, const int32_t* rowptr, const int32_t* col,
                                const float* node4, float* ce_act, float* h,
                                const float* norm_h_w, const float* norm_h_b,
                                const float* norm_e_w, const float* norm_e_b,
                                const float* out_ln_w, const float* out_ln_b,
                                const float* tbias, int time_on_edge, void* stream);
/* The same pass with the neighbour aggregation chosen: aggregation = DIFUSCO_AGG_* (sum / mean / max over the edges of the
 * row; an empty row aggregates to 0).  Additive at ABI 13: difusco_edge_gate_aggregate(..) is this with DIFUSCO_AGG_SUM. */
int difusco_edge_gate_aggregate_ex(int hidden, int n_nodes, const int32_t* rowptr, const int32_t* col,
                                   const float* node4, float* ce_act, float* h,
                                   const float* norm_h_w, const float* norm_h_b,
                                   const float* norm_e_w, const float* norm_e_b,
                                   const float* out_ln_w, const float* out_ln_b,
                                   const float* tbias, int time_on_edge, int aggregation, void* stream);

/* The fused edge pass of one layer + node update (edge_layer.hip), H = 256 only:
 *   e <- e + W_o SiLU(LN_o(ReLU(LN_e(Ah[j]+Bh[i]+C e)) (+t))) + b_o ;  h_i += ReLU(LN_h(Uh_i + sum gate*Vh_j)) (+t)
 * e is in the TILED layout of the fused path: rows padded to a multiple of 256 edges (pad = 0), 32-edge
 * tiles of 8192 floats ordered [f/16][(f/8)%2][((f/4)%2)*32 + s%32][f%4] (csrc/kernels.h edge_tiled_offset,
 * difusco_amd.graph.to_tiled) - every wavefront access is then one contiguous KiB.
 * planes_c / planes_o: the five 16-bit planes of C / per_layer_out[l][2] (see *_PLANES above);
 * precision = DIFUSCO_PREC_BF16X3 | DIFUSCO_PREC_FP16X3.  scales: the layer's DIFUSCO_WL_FUSED_SCALES record (device,
 * 8 floats; required for FP16X3, ignored for BF16X3).  scratch: >= difusco_fused_scratch_bytes().
 * node4 is the REFERENCE's U h | V h | A h | B h (gnn_encoder.py:94-103); this entry converts the A | B rows into the kernel's
 * log2(e) domain itself (a copy in the scratch, ABI 11) - the step driver has no such pass, its node linear writes them so. */
size_t difusco_fused_scratch_bytes(int n_nodes, int n_edges);
int difusco_edge_layer_fused(int precision, int n_nodes, int n_edges, const int32_t* rowptr, const int32_t* row,
                             const int32_t* col, const float* node4, float* e, float* h, const void* planes_c,
                             const void* planes_o, const float* b_c, const float* norm_h_w, const float* norm_h_b,
                             const float* norm_e_w, const float* norm_e_b, const float* out_ln_w,
                             const float* out_ln_b, const float* b_out, const float* tbias, int time_on_edge,
                             const float* scales, void* scratch, void* stream);
/* The same layer with the two choices the step driver makes for it: aggregation = DIFUSCO_AGG_* (the kernel's max kinds and
 * node_finalize's sum / mean / max) and reg_gather = 0 | 1 (1: the register-gather instantiations that a step uses for calls with
 * n_nodes >= 2^20; valid at any size).  reg_gather = 1 with DIFUSCO_AGG_MAX is refused (DIFUSCO_EINVAL), as in the step.
 * Additive at ABI 13: difusco_edge_layer_fused(..) is this with (DIFUSCO_AGG_SUM, n_nodes >= 2^20). */
int difusco_edge_layer_fused_ex(int precision, int n_nodes, int n_edges, const int32_t* rowptr, const int32_t* row,
                                const int32_t* col, const float* node4, float* e, float* h, const void* planes_c,
                                const void* planes_o, const float* b_c, const float* norm_h_w, const float* norm_h_b,
                                const float* norm_e_w, const float* norm_e_b, const float* out_ln_w,
                                const float* out_ln_b, const float* b_out, const float* tbias, int time_on_edge,
                                const float* scales, void* scratch, int aggregation, int reg_gather, void* stream);

/* Elementwise posteriors on already computed predictions (pl_meta_model.py:102-175).  rand_mode 0-2 (the per-instance
 * mode needs the instance tables of difusco_step_args and is refused here). */
int difusco_categorical_posterior(const float* logits, const float* xt, const float* post,
                                  int rand_mode, const float* rand, uint64_t seed, uint64_t offset,
                                  float* xt_out, float* prob_out, int64_t n, void* stream);
int difusco_gaussian_posterior(const float* pred, const float* xt, const float* post,
                               int rand_mode, const float* rand, uint64_t seed, uint64_t offset,
                               float* xt_out, int64_t n, void* stream);

/* ---- k-NN graph in the reference's layout: co_datasets/tsp_graph_dataset.py:53-62
 * (sklearn KDTree(points).query(points, k) on float64 coordinates).  points: DEVICE float64 [n_nodes,2]; writes
 * edge_row0[i*k + r] = node_offset + i and edge_row1[i*k + r] = node_offset + (r-th nearest neighbour of i, self
 * first, ties by lower index) - DEVICE int64, i.e. the graph's slice of a [2, E_tot] edge_index of a disjoint-union
 * batch (pl_meta_model.py:177-184).  1 <= k <= min(n_nodes, 1024).  Asynchronous on `stream`. */
int difusco_knn_graph_workspace_bytes(int n_nodes, int k, size_t* bytes);
int difusco_knn_graph(int n_nodes, int k, const double* points, int64_t node_offset, int64_t* edge_row0,
                      int64_t* edge_row1, void* workspace, size_t workspace_bytes, void* stream);

/* ---- greedy MIS decode: difusco/utils/mis_utils.py:3-18 (mis_decode_np).  rowptr/col: DEVICE CSR of
 * the symmetric adjacency of the whole call (self loops allowed, as in co_datasets/mis_dataset.py:43-48; the
 * graphs of a batch are independent components); scores: DEVICE float32 [n_nodes] (the final x_t, + 1e-6 or
 * * 0.5 + 0.5 applied); solution: DEVICE int32 [n_nodes], 1 = in the independent set.  Visiting order = decreasing
 * score, equal scores by increasing node id.  *rounds_out (HOST, optional) = parallel rounds used.  Blocks.
 *   order     numpy's argsort(-scores, kind="stable"): -0.0 and +0.0 are one value, every NaN (either sign, any payload)
 *             ranks after everything else including -inf, equal scores and the NaNs among themselves by increasing node id.
 *             The library sorts a key of its own (mis_sort_key, csrc/kernels.h), not the float bit patterns.
 *   rounds    level(v) = 1 + max level(u) over the neighbours u != v that rank before v, 1 without one; a node of level l has
 *             decided by the end of round l, and the host polls after every fourth round, so
 *             4 <= *rounds_out <= 4 * ceil(max level / 4) and *rounds_out % 4 == 0.
 *   symmetry  the adjacency must be symmetric: a node reads its OWN row for the neighbours that can exclude it, where the
 *             reference excludes through the row of the node it takes.  Not checked.  Self entries are skipped, duplicate
 *             entries change nothing, rows may be empty.
 *   col       must not be null even when no row has an entry (it is not read then): a caller without entries passes any
 *             device address, as the Python wrappers do.  The same holds for the two MIS searches below. */
int difusco_mis_decode_workspace_bytes(int n_nodes, size_t* bytes);
int difusco_mis_decode(int n_nodes, const int32_t* rowptr, const int32_t* col, const float* scores, int32_t* solution,
                       void* workspace, size_t workspace_bytes, int32_t* rounds_out, void* stream);

/* ---- (1,2)-swap local search for MIS solutions (additive to ABI 13; not in the reference, whose MIS path ends at the greedy
 * decode).  rowptr/col/scores: as difusco_mis_decode (DEVICE; the symmetric adjacency of the whole call, self loops allowed and
 * ignored, rows may be empty).  solution: DEVICE int32 [n_nodes], in/out: an independent set (non-zero = chosen), not
 * necessarily maximal, all zeros allowed; on return 0/1.
 *   rank[v]   position of v in the stable descending sort of the scores - the order of difusco_mis_decode, equal scores by
 *             increasing node id; a smaller rank is a higher priority.
 *   tight[v]  on the current set S: the number of neighbours u != v of v in S.  A node outside S is FREE with tight = 0 and a
 *             CANDIDATE of its one solution neighbour with tight = 1; L(x) is the set of candidates of x in S.
 *   insertion phase  insert the lexicographically first maximal independent set, by rank, of the subgraph the free nodes
 *             induce: a free node goes in iff all its higher-priority free neighbours stay out.
 * One insertion phase, then rounds until a round proposes nothing (that round is not counted) or max_rounds rounds ran:
 *   1. proposal  every x in S takes the pair (u, w), u and w in L(x), not adjacent, rank[u] < rank[w], that is smallest in
 *                (rank[u], rank[w]); without such a pair x proposes nothing;
 *   2. conflict  proposals x != y conflict iff a node of {u_x, w_x} is adjacent to a node of {u_y, w_y}; x is applied iff
 *                rank[u_x] < rank[u_y] for every conflicting y (the keys are distinct: candidate sets are disjoint; the
 *                smallest key always applies, so a counted round applies a swap and there are at most n_nodes rounds);
 *   3. apply     all winners at once: x leaves S, u_x and w_x enter;
 *   4. an insertion phase (the third leaf of a claw; nodes whose two solution neighbours both left).
 * The result is independent and maximal, |S_out| = |S_in| + swaps + inserts, and with max_rounds high enough no x has a
 * proposal left.  Every step is local to a connected component and round r of a union is round r of every component, so a
 * call on a disjoint union gives every component the nodes its own call gives, capped or not.  Duplicate entries in a
 * neighbour list can only make the search find fewer swaps, never a dependent set.
 * counters: HOST int32 [3] = rounds, swaps, inserts of the whole call.  max_rounds = 0 runs the first insertion phase only.
 * DIFUSCO_EINVAL on a null array, n_nodes < 1, max_rounds < 0, a workspace below _workspace_bytes, and on an input set that
 * is not independent: one checking pass sets a device flag and solution is left unchanged.  All per-round work runs on the
 * device behind a phase word in the workspace; the host polls it once per group of four rounds.  Blocks. */
int difusco_mis_local_search_workspace_bytes(int n_nodes, int64_t n_edges, size_t* bytes);
int difusco_mis_local_search(int n_nodes, const int32_t* rowptr, const int32_t* col, const float* scores,
                             int32_t* solution /* in/out, device */, int32_t max_rounds, void* workspace,
                             size_t workspace_bytes, int32_t counters[3] /* host: rounds, swaps, inserts */, void* stream);

/* ---- iterated (1,2)-swap search for MIS solutions: seeded random kicks between descents (additive to ABI 13; not in the
 * reference).  Graph, scores, solution and max_rounds: as difusco_mis_local_search.  THE DESCENT below is that search exactly:
 * one insertion phase, then swap rounds until a round proposes nothing or max_rounds rounds ran; the ranks come from `scores`.
 * The instance table (DEVICE, the types of difusco_step_args): instance_rows int64 [n_instances + 1], non-decreasing node
 * offsets from 0 to n_nodes (empty instances allowed); instance_seeds, instance_offsets uint64 [n_instances].  No edge joins two
 * instances: the caller guarantees it, it is not checked.  kicks >= 0, kick_size >= 1.
 *   1. The descent on the input set gives the incumbent I.
 *   2. For t = 0 .. kicks - 1, synchronously over the whole call:
 *      draw     node v of instance b, local index r = v - instance_rows[b], draws
 *               w_v = (word 0 of Philox4x32-10(key instance_seeds[b], offset instance_offsets[b] + t, index r)) >> 8,
 *               the project's 24-bit uniform kept as an integer;
 *      kicked   m_b = the number of nodes of b outside I; v is kicked iff v is outside I and w_v * m_b < kick_size * 2^24,
 *               evaluated exactly in uint64 (the left side stays below 2^55): about kick_size nodes of every instance;
 *      entered  a kicked v enters iff no kicked neighbour u != v has (w_u, u) < (w_v, v); entered nodes are pairwise
 *               non-adjacent by construction;
 *      evict    C = I minus every member adjacent to an entered node, plus the entered nodes (self loops are ignored);
 *      descend  the descent on C (its leading insertion phase re-fills around the evicted nodes);
 *      keep     per instance: if |C_b| >= |I_b| then I_b <- C_b (plateau moves are kept), otherwise I_b stays.
 *   3. solution <- I.
 * kicks = 0 returns exactly what difusco_mis_local_search returns, set and counters alike.  The result is independent and
 * maximal, and |out_b| >= the swap descent's |S_b| for every instance.  Every step is local to an instance and step t of a
 * union is step t of each instance, so a call on a union gives every instance exactly what its own call gives with the same
 * seed and offset, capped by max_rounds or not.
 * counters: HOST int32 [3] = rounds, swaps, inserts summed over all descents, the restored ones included.  per_instance: HOST
 * int32 [4 * n_instances], may be NULL; for instance b: [4b] entered = the kicks in which at least one node of b entered,
 * [4b + 1] accepted = those of them that were kept, [4b + 2] size_before = |I_b| after step 1, [4b + 3] size_after.
 * DIFUSCO_EINVAL on a null array, n_nodes < 1, n_instances < 1, max_rounds < 0, kicks < 0, kick_size < 1, a workspace below
 * _workspace_bytes, a malformed table (checked on the device) and an input set that is not independent; solution is then
 * left unchanged.  The kick loop runs on the device behind the phase word of the descent (two more phases); the host enqueues
 * groups of 8 x (2 rounds of the descent, one kick) launches and polls once per group, so a call makes at most `kicks` more
 * host synchronisations than the kicks = 0 call unless the descents after the kicks average more than 16 rounds.  Blocks.
 * difusco_mis_search_host_syncs: the host synchronisations of the calling thread's last difusco_mis_local_search or
 * difusco_mis_iterated_search call. */
int difusco_mis_iterated_search_workspace_bytes(int n_nodes, int64_t n_edges, int n_instances, size_t* bytes);
int difusco_mis_iterated_search(int n_nodes, const int32_t* rowptr, const int32_t* col, const float* scores,
                                int32_t* solution /* in/out, device */, int n_instances, const int64_t* instance_rows,
                                const uint64_t* instance_seeds, const uint64_t* instance_offsets, int32_t kicks,
                                int32_t kick_size, int32_t max_rounds, void* workspace, size_t workspace_bytes,
                                int32_t counters[3] /* host */, int32_t* per_instance /* host, optional */, void* stream);
int difusco_mis_search_host_syncs(void);

/* ---- the iterated search above with one resident GPU block per instance (additive to ABI 13).  The arguments of
 * difusco_mis_iterated_search up to max_rounds, and THE SAME RULE: for every input that entry accepts and whose instances all
 * have at most difusco_mis_resident_max_nodes() nodes (a constant of the build, >= 2048), solution, counters and per_instance
 * come back exactly as that entry returns them; kicks = 0 is difusco_mis_local_search.  What differs is the execution: after
 * the launched search's own start (sort, ranks, working copy, the independence and table checks) one block per table row runs
 * its instance from the first descent to the last keep with the per-node state in LDS, and the host enqueues
 * ceil(kicks / kicks_per_launch) launches (at least one) back to back without reading anything in between; the incumbent and
 * the counters stay in the workspace between launches.  kicks_per_launch bounds the run time of one launch; 0 = the library's
 * default (256).  One copy-out and ONE host synchronisation per call, whatever kicks is: difusco_mis_search_host_syncs reports
 * this entry too.  counters[0], the rounds of the call, is the sum over the kicks + 1 descents of the rounds of the instance
 * that descended longest, which is what a union's descent counts; that array is why _workspace_bytes takes kicks.  The
 * workspace is never smaller than difusco_mis_iterated_search_workspace_bytes for the same call.
 * DIFUSCO_EINVAL as difusco_mis_iterated_search and on kicks_per_launch < 0; DIFUSCO_EUNSUPPORTED when an instance has more
 * nodes than the limit (checked on the device before anything is written; the message names the instance and the limit).
 * solution is left unchanged by every refusal.  Blocks. */
int difusco_mis_resident_max_nodes(void);
int difusco_mis_resident_search_workspace_bytes(int n_nodes, int64_t n_edges, int n_instances, int32_t kicks, size_t* bytes);
int difusco_mis_resident_search(int n_nodes, const int32_t* rowptr, const int32_t* col, const float* scores,
                                int32_t* solution /* in/out, device */, int n_instances, const int64_t* instance_rows,
                                const uint64_t* instance_seeds, const uint64_t* instance_offsets, int32_t kicks,
                                int32_t kick_size, int32_t max_rounds, int32_t kicks_per_launch /* 0 = default */,
                                void* workspace, size_t workspace_bytes, int32_t counters[3] /* host */,
                                int32_t* per_instance /* host, optional */, void* stream);

/* ---- heatmap -> tour: the greedy edge insertion the reference runs on the host right after the
 * sampling loop, difusco/utils/tsp_utils.py:89-145 (merge_tours) + utils/cython_merge/cython_merge.pyx:19-104
 * (merge_cython), restricted to the E entries of the sparse heatmap instead of the N x N densification.
 * ONE graph per call, node ids 0..n_nodes-1 (the caller slices a batch).  row/col/heat/points/workspace are DEVICE
 * pointers: row[e] -> col[e] are the directed edges of the sparse graph in any order, heat[e] the final x_t
 * (+1e-6 / *0.5+0.5 already applied, pl_tsp_model.py:219-222), points [n_nodes,2] float32.  tour_out (HOST,
 * n_nodes + 1 ints) receives the closed tour starting and ending at node 0 (tsp_utils.py:134-141);
 * *merge_iterations the reference's counter over its dense sorted list; *completed = 1 when the N-1 insertions
 * were found among candidate pairs with a positive score (the regime in which the result is pinned to the
 * reference), 0 when the fallback had to finish the tour.  Blocks until done (synchronises `stream`). */
int difusco_tsp_merge_workspace_bytes(int64_t n_edges, size_t* bytes);
int difusco_tsp_merge_tour(int n_nodes, int64_t n_edges, const int32_t* row, const int32_t* col, const float* heat,
                           const float* points, void* workspace, size_t workspace_bytes, int32_t* tour_out,
                           int64_t* merge_iterations, int32_t* completed, void* stream);
/* The `parallel_sampling` samples of ONE graph in one call (the loop of tsp_utils.py:100-145 over adj_mat[i]):
 * heat [n_samples][n_edges] DEVICE, tours_out [n_samples][n_nodes + 1] HOST, merge_iterations / completed [n_samples]
 * HOST (optional).  The pair keys depend on the graph only, so their sort runs once per call; the workspace is the
 * one of difusco_tsp_merge_workspace_bytes.  Results per sample equal difusco_tsp_merge_tour's. */
int difusco_tsp_merge_tours(int n_nodes, int64_t n_edges, const int32_t* row, const int32_t* col, const float* heat,
                            const float* points, int n_samples, void* workspace, size_t workspace_bytes,
                            int32_t* tours_out, int64_t* merge_iterations, int32_t* completed, void* stream);

/* Batched merge (additive to ABI 13): the heatmaps of `graphs` graphs of ANY sizes, graph g with graph_samples[g] samples,
 * in one launch sequence; the greedy insertion runs on the GPU, one 64-lane wave per (graph, sample).  graph_n, graph_edges,
 * graph_samples: HOST tables [graphs].  row / col: DEVICE, the graphs' directed edge lists back to back, node ids local to
 * their graph (0 .. n_g - 1); row == col == NULL: every graph is complete, entry (i, j) at i * n_g + j, graph_edges[g] = n_g^2.
 * heat: DEVICE, graph after graph [P_g][E_g]; points: DEVICE float32, the [n_g, 2] blocks back to back.  tours_out (HOST):
 * the closed tours back to back in (graph, sample) order, n_g + 1 ints each; merge_iterations / completed (HOST, optional):
 * one entry per sample in the same order.  Every (graph, sample) gets exactly what difusco_tsp_merge_tours gives that graph
 * alone: tour, merge_iterations and completed.  A sample whose positive scores end before its n_g - 1 insertions (completed
 * = 0) is finished on the host by the code the per-graph entries use.  flags: DIFUSCO_MERGE_STATE_GLOBAL keeps the per-node
 * path state (12 bytes per node) in the workspace at any size; without it a sample's state lives in LDS when 12 * n_g <= 160 KiB
 * (n_g <= 13653).  DIFUSCO_EINVAL before any GPU work on: graphs < 1, a null required array, only one of row / col null, an
 * n_g < 3, an E_g <= 0 or above 2^32, a complete graph with E_g != n_g^2, a P_g < 1, an unknown flag bit, a workspace below
 * _workspace_bytes; also on more than 2^32 list entries (the sum of P_g * E_g) in one call, or when the graph index and the
 * largest pair key n_g^2 do not fit 64 bits together.  Blocks until done. */
#define DIFUSCO_MERGE_STATE_GLOBAL 1u
int difusco_tsp_merge_batch_workspace_bytes(int graphs, const int32_t* graph_n, const int64_t* graph_edges,
                                            const int32_t* graph_samples, size_t* bytes);
int difusco_tsp_merge_batch(int graphs, const int32_t* graph_n, const int64_t* graph_edges, const int32_t* graph_samples,
                            const int32_t* row, const int32_t* col, const float* heat, const float* points, uint32_t flags,
                            void* workspace, size_t workspace_bytes, int32_t* tours_out, int64_t* merge_iterations,
                            int32_t* completed, void* stream);

/* ---- batched 2-opt: difusco/utils/tsp_utils.py:12-49 (batched_two_opt_torch).  points: DEVICE
 * float64 [n_nodes,2]; tours: DEVICE int32 [batch, n_nodes+1] closed tours, refined in place.  Every iteration
 * finds, per tour, the move (i,j), j >= i+2, that minimises d(t_i,t_j) + d(t_i+1,t_j+1) - d(t_i,t_i+1) - d(t_j,t_j+1)
 * (float64, the reference's operation order, first flat index on ties) and reverses tour[i+1..j]; it stops when the
 * best change over the whole batch is >= -1e-6 or after max_iterations applied moves.  *iterations_out (HOST) =
 * the reference's `iterator`.  Blocks until done.  The call is one group of `batch` tours of the grouped entry below and
 * reserves what difusco_tsp_two_opt_grouped_workspace_bytes(n_nodes, 1, batch) does. */
int difusco_tsp_two_opt_workspace_bytes(int n_nodes, int batch, size_t* bytes);
int difusco_tsp_two_opt(int n_nodes, int batch, const double* points, int32_t* tours, int64_t max_iterations,
                        void* workspace, size_t workspace_bytes, int64_t* iterations_out, void* stream);

/* Grouped 2-opt (ABI 13): `groups` independent instances of the same n_nodes, each with `per_group` tours.  points: DEVICE
 * float64 [groups, n_nodes, 2]; tours: DEVICE int32 [groups * per_group, n_nodes + 1], the tours of group g at rows
 * g * per_group .. (g + 1) * per_group - 1, refined in place.  Every group follows difusco_tsp_two_opt on its own tours
 * exactly (its stop test looks at its own tours only); a group that has stopped costs no further work.
 * iterations_out: HOST int64 [groups], the applied moves of every group.  Blocks until every group is done. */
int difusco_tsp_two_opt_grouped_workspace_bytes(int n_nodes, int groups, int per_group, size_t* bytes);
int difusco_tsp_two_opt_grouped(int n_nodes, int groups, int per_group, const double* points, int32_t* tours,
                                int64_t max_iterations, void* workspace, size_t workspace_bytes, int64_t* iterations_out,
                                void* stream);

/* Screened 2-opt (additive to ABI 13): the arguments, semantics and results of difusco_tsp_two_opt / _grouped - the same moves,
 * tours and iteration counts, bit for bit.  Every pair is first evaluated in float32; only a pair that the float32 value cannot
 * rule out, given the proven bound |c32 - c64| <= eps(M), is evaluated in float64 (M = the largest |coordinate| of the
 * instance, reduced on the device once per call).  exact_pairs_out (HOST, optional): the number of pairs of the whole call that
 * took the float64 path.  The workspaces are larger than the exact entries' (their own _workspace_bytes).  At most 65535 tours
 * per call.
 * difusco_tsp_two_opt_screen_bound is a HOST function (no GPU): returns 1 and *eps = the margin the kernels use for an instance
 * whose largest |coordinate| is max_abs_coord, 0 (and *eps = 0) when no bound exists - max_abs_coord not finite or outside
 * [2^-32, 2^60], where float32 under- or overflows; a screened call with such a group runs the exact sweep instead, with the
 * same results.  Negative on a null pointer. */
int difusco_tsp_two_opt_screen_bound(double max_abs_coord, double* eps);
int difusco_tsp_two_opt_screened_workspace_bytes(int n_nodes, int batch, size_t* bytes);
int difusco_tsp_two_opt_screened(int n_nodes, int batch, const double* points, int32_t* tours, int64_t max_iterations,
                                 void* workspace, size_t workspace_bytes, int64_t* iterations_out, int64_t* exact_pairs_out,
                                 void* stream);
int difusco_tsp_two_opt_grouped_screened_workspace_bytes(int n_nodes, int groups, int per_group, size_t* bytes);
int difusco_tsp_two_opt_grouped_screened(int n_nodes, int groups, int per_group, const double* points, int32_t* tours,
                                         int64_t max_iterations, void* workspace, size_t workspace_bytes,
                                         int64_t* iterations_out, int64_t* exact_pairs_out, void* stream);

/* Ragged 2-opt (additive to ABI 13): the grouped entries for groups of DIFFERENT sizes.  group_n, group_tours: HOST int32
 * [groups], the nodes and the number of tours of every group.  points: DEVICE float64, the groups' [n_g, 2] blocks back to back;
 * tours: DEVICE int32, back to back in group order, every tour of group g n_g + 1 long, refined in place.  Group g gets exactly
 * what difusco_tsp_two_opt(n_g, group_tours[g], ...) gives its tours alone: its own stop test and iteration count, the flat
 * index i * n_g + j of its own size on ties, the shared max_iterations.  method: 0 the exact sweep, 1 the screened one (eps from
 * the group's own largest |coordinate|; one group without a bound sends the whole call to the exact sweep).
 * iterations_out: HOST int64 [groups].  exact_pairs_out (HOST, optional): the pairs of the call evaluated in float64 (method 0,
 * or no bound: every pair of every sweep).  DIFUSCO_EINVAL before any GPU work on: groups < 1, a null array, an n_g < 4 or above
 * 65535 * 16, a group without tours, more than 65535 tours, a method other than 0 / 1, a workspace below _workspace_bytes. */
int difusco_tsp_two_opt_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int method,
                                               size_t* bytes);
int difusco_tsp_two_opt_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                               int32_t* tours, int64_t max_iterations, int method, void* workspace, size_t workspace_bytes,
                               int64_t* iterations_out, int64_t* exact_pairs_out, void* stream);

/* Resident 2-opt (additive to ABI 13): difusco_tsp_two_opt_ragged with one resident GPU block per group.  The arrays and
 * conventions of that entry, and THE SAME RULE: group g ends with exactly the tours and iterations_out[g] that
 * difusco_tsp_two_opt_ragged gives it, with either method.  What differs is the execution: a block keeps the tours of its group,
 * their points in tour order, the edge lengths and (method 1) the float32 copies in LDS and runs move after move - sweep,
 * argmin per tour, group minimum, stop test, reversals - between block barriers, without a launch or a host read per move.
 * A group fits if group_tours[g] * (group_n[g] + 1) <= difusco_tsp_two_opt_resident_max_cells(), a constant of the build for
 * both methods, >= 2048 (TSP-500 with 4 tours: 2004 cells).  The sizes are host arrays, so a group above the limit is refused
 * on the host before any GPU work: DIFUSCO_EUNSUPPORTED, the message names the group, its cells and the limit, `tours` is
 * untouched; there is no fallback to the launched entry.
 * method: 0 the exact sweep, 1 the screened one under the bound of difusco_tsp_two_opt_screen_bound with the group's own largest
 * |coordinate|, reduced inside its block.  A group without a bound takes the exact sweep FOR ITSELF ONLY; in
 * difusco_tsp_two_opt_ragged one such group sends the whole call to the exact sweep.  The tours and iteration counts are the same
 * either way; only exact_pairs_out can tell the difference.
 * moves_per_launch: a launch applies at most that many moves per group; 0 = the library's default (1024).  The tours, the counts
 * and the stop flags stay in global memory between launches, a stopped group's block returns at once.  The host enqueues
 * ceil(max(max_iterations, 1) / moves_per_launch) launches at most and reads the state once after each: that read tells whether
 * another launch is needed and, after the last one, is the result.  Hence one host synchronisation per launch that ran, none
 * inside a launch; host_syncs_out (HOST, optional) reports the number.
 * exact_pairs_out (HOST, optional): the pairs of the call evaluated in float64, counted by the kernel - with method 0, and for a
 * group without a bound, every pair of every sweep; with method 1 never more than that.
 * workspace: _workspace_bytes, a few bytes per group.  DIFUSCO_EINVAL before any GPU work on everything
 * difusco_tsp_two_opt_ragged refuses and on moves_per_launch < 0.  Blocks until every group is done. */
int difusco_tsp_two_opt_resident_max_cells(void);
int difusco_tsp_two_opt_resident_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int method,
                                                 size_t* bytes);
int difusco_tsp_two_opt_resident(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                 int32_t* tours, int64_t max_iterations, int method, int32_t moves_per_launch /* 0 = default */,
                                 void* workspace, size_t workspace_bytes, int64_t* iterations_out /* host */,
                                 int64_t* exact_pairs_out /* host, optional */, int32_t* host_syncs_out /* host, optional */,
                                 void* stream);

/* Local search, 2-opt + Or-opt (additive to ABI 13): the arrays, conventions and limits of difusco_tsp_two_opt_ragged.  Every
 * group runs rounds of two phases on its own tours, independent of the other groups:
 *   2-opt phase   exactly difusco_tsp_two_opt(n_g, group_tours[g], ...) with max_iterations (the exact sweep) -> a moves;
 *   Or-opt phase  per iteration every tour applies its own best Or-opt move if its delta < -1e-6; an iteration counts if a
 *                 tour of the group moved; the phase ends after an iteration without a move or after max_iterations counted
 *                 iterations (none with max_iterations = 0) -> b;
 * and stops after a round with b = 0 or after max_rounds rounds.  An Or-opt candidate (v, i, j) moves the segment at positions
 * i+1 .. i+L of the closed tour, 0 <= i <= n-1-L (positions 0 and n never move), between positions j and j+1, 0 <= j <= n-1,
 * j outside [i, i+L]; (L, reversed) = variant v of [(1,no), (2,no), (2,yes), (3,no), (3,yes)].  With P_k the point at position
 * k, d_k = |P_k P_k+1| and (a, b) = (P_i+1, P_i+L), swapped when reversed:
 *   delta = ((|P_i P_i+L+1| + |P_j a|) + |b P_j+1|) - ((d_i + d_i+L) + d_j)
 * in float64, every operation rounded on its own, distances as in the 2-opt (two products, one sum, a square root).  The best
 * move is the lowest delta, ties to the lowest flat index (v n + i) n + j.  Applied: tour[:i+1] + tour[i+L+1:j+1] + seg +
 * tour[j+1:] for j > i+L, tour[:j+1] + seg + tour[j+1:i+1] + tour[i+L+1:] for j < i.  The first 2-opt phase is the plain 2-opt
 * and every later move shortens a tour by more than 1e-6, so no tour ends longer than difusco_tsp_two_opt_ragged leaves it.
 * two_opt_iterations_out, or_opt_iterations_out: HOST int64 [groups], the sums of a and b; rounds_out: HOST int32 [groups], the
 * rounds started.  DIFUSCO_EINVAL before any GPU work on the conditions of difusco_tsp_two_opt_ragged, a null output array and
 * max_rounds < 1.  Blocks until every group is done. */
int difusco_tsp_local_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes);
int difusco_tsp_local_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                    int32_t* tours, int64_t max_iterations, int max_rounds, void* workspace, size_t workspace_bytes,
                                    int64_t* two_opt_iterations_out, int64_t* or_opt_iterations_out, int32_t* rounds_out, void* stream);

/* Resident local search (additive to ABI 13): difusco_tsp_local_search_ragged with one resident GPU block per group.  The arrays
 * and conventions of that entry, and THE SAME RULE: group g ends with exactly the tours, two_opt_iterations_out[g],
 * or_opt_iterations_out[g] and rounds_out[g] that difusco_tsp_local_search_ragged gives it - the rounds of (exact 2-opt phase,
 * Or-opt phase), max_iterations per phase, the threshold -1e-6, the flat-index ties, the one evaluated 2-opt move at
 * max_iterations = 0, the stop after a round with b = 0 or after max_rounds rounds.  What differs is the execution: a block keeps
 * the tours of its group, their points in tour order, the group's points, the edge lengths, the best move of every tour and the
 * stretch an Or-opt move shifts in LDS and runs step after step - sweep, argmin per tour, group minimum, stop test, moves, switch
 * of phase and round - between block barriers, without a launch or a host read per step.  A STEP is one 2-opt move of the group
 * or one counted Or-opt iteration.
 * A group fits if group_tours[g] * (group_n[g] + 1) <= difusco_tsp_local_search_resident_max_cells(), a constant of the build,
 * >= 2048 (TSP-500 with 4 tours: 2004 cells).  The sizes are host arrays, so a group above the limit is refused on the host
 * before any GPU work: DIFUSCO_EUNSUPPORTED, the message names the group, its cells and the limit, `tours` is untouched; there
 * is no fallback to the launched entry.
 * steps_per_launch: a launch applies at most that many steps per group; 0 = the library's default (1024).  The tours and the
 * state of every group (phase, round, iterations of the phase, the counters) stay in global memory between launches, a stopped
 * group's block returns at once.  A launch ends for a group when the group stops or when a sweep finds a move after
 * steps_per_launch steps; the next launch repeats that sweep.  The host reads the state once after each launch and enqueues
 * another one only if a group still runs: one host synchronisation per launch that ran, none inside a launch, and
 * max(1, ceil(steps of the slowest group / steps_per_launch)) launches per call; host_syncs_out (HOST, optional) reports the
 * number.
 * workspace: _workspace_bytes, a few bytes per group.  DIFUSCO_EINVAL before any GPU work on everything
 * difusco_tsp_local_search_ragged refuses, on steps_per_launch < 0 and on a workspace below _workspace_bytes.  Blocks until every
 * group is done. */
int difusco_tsp_local_search_resident_max_cells(void);
int difusco_tsp_local_search_resident_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes);
int difusco_tsp_local_search_resident(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                      int32_t* tours, int64_t max_iterations, int max_rounds, int32_t steps_per_launch /* 0 = default */,
                                      void* workspace, size_t workspace_bytes, int64_t* two_opt_iterations_out /* host */,
                                      int64_t* or_opt_iterations_out /* host */, int32_t* rounds_out /* host */,
                                      int32_t* host_syncs_out /* host, optional */, void* stream);

/* Multi-move 2-opt (additive to ABI 13; not in the reference, which applies one move per sweep): the arrays, conventions and
 * limits of difusco_tsp_two_opt_ragged.  Every TOUR runs on its own.  With P_k the point at position k of the closed tour
 * (P_n = P_0) and d_k = |P_k P_k+1|, one SWEEP of a tour of n nodes is:
 *   1. Row proposals.  Row i = 0 .. n-3 evaluates change(i, j) = ((|P_i P_j| + |P_i+1 P_j+1|) - d_i) - d_j for i+2 <= j <= n-1 in
 *      float64, every operation rounded on its own, distances as two products, one sum, a square root: the changes of
 *      difusco_tsp_two_opt, bit for bit.  The row keeps its lowest change, ties to the lowest j, and proposes (i, j_i) if that
 *      change is < -1e-6.  The proposal's key is (change, i), ordered lexicographically (keys are distinct); its range is the
 *      half-open position interval [i, j_i + 1).
 *   2. Selection, in at most select_rounds rounds.  In a round a live proposal wins if its key is lower than the key of every
 *      other live proposal whose range intersects its own.  After the round the winners leave the live set, and every live
 *      proposal whose range intersects a winner's range is dropped for this sweep.  Selection ends early when nothing is live.
 *      With select_rounds unbounded this is the greedy choice in key order.
 *   3. Apply.  Every winner reverses tour[i+1 .. j_i]; the ranges are disjoint, so the order does not matter.  Positions 0 and n
 *      never move.
 *   4. Stop test.  A tour with no proposal is done and costs no further work.  A sweep counts for a group if one of its tours
 *      moved.  A group stops when all its tours are done or after max_iterations counted sweeps; with max_iterations = 0 no
 *      sweep counts and nothing is applied.
 * So: the best pair of the exact 2-opt (lowest change, lowest flat index i n + j) is always a winner of round 1; every counted
 * sweep shortens every moved tour by more than 1e-6 per move; a tour that stops before the cap has no improving 2-opt move left;
 * a tour's result does not depend on which other tours or groups share the call.
 * sweeps_out, moves_out: HOST int64 [groups], the counted sweeps and the moves applied over all tours of the group.
 * DIFUSCO_EINVAL before any GPU work on the conditions of difusco_tsp_two_opt_ragged, a null output array and select_rounds < 1.
 * Blocks until every group is done. */
int difusco_tsp_multi_two_opt_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes);
int difusco_tsp_multi_two_opt_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                     int32_t* tours, int64_t max_iterations, int select_rounds, void* workspace,
                                     size_t workspace_bytes, int64_t* sweeps_out, int64_t* moves_out, void* stream);

/* Neighbour-list multi-move 2-opt with a closing full descent (additive to ABI 13; not in the reference): the arrays,
 * conventions and limits of difusco_tsp_multi_two_opt_ragged, and its notation.  New inputs:
 *   neighbors  DEVICE int32: for every group g [group_n[g], K] entries, the groups concatenated.  An entry of city a is a city
 *              index local to the group.  An entry outside 0 .. n-1, or equal to a, is a pad and is skipped; no kernel indexes
 *              memory with it.  Duplicate entries are allowed.  N(a) = the non-pad entries of city a.
 *   K >= 1, closing in {0, 1}.
 * Every TOUR runs on its own and keeps its own phase.  A tour starts in the neighbour phase.  One NEIGHBOUR SWEEP of a tour of n
 * nodes (tour[k] = the city at position k, tour[n] = tour[0]):
 *   1. Candidates.  For i+2 <= j <= n-1, column j is a candidate of row i (0 .. n-3) iff tour[j] in N(tour[i]) or tour[i] in
 *      N(tour[j]) or tour[j+1] in N(tour[i+1]) or tour[i+1] in N(tour[j+1]): the pairs whose new head edge (tour[i], tour[j]) or
 *      new tail edge (tour[i+1], tour[j+1]) joins a city to one of its listed neighbours, in either direction.  Position n is
 *      position 0: the pair (i, n-1) has the tail edge (tour[i+1], tour[0]).
 *   2. Row proposals.  Row i evaluates change(i, j) of difusco_tsp_multi_two_opt_ragged, bit for bit, for its candidate columns
 *      only, keeps the lowest change, ties to the lowest j, and proposes (i, j_i) iff that change is < -1e-6.  Key (change, i),
 *      range [i, j_i + 1), as there.
 *   3. Selection and apply: steps 2 and 3 of difusco_tsp_multi_two_opt_ragged, unchanged.
 *   4. Closing.  A tour whose neighbour sweep has no proposal is done if closing = 0.  With closing = 1 it moves to the full
 *      phase: from its next sweep on its sweeps are those of difusco_tsp_multi_two_opt_ragged (every column is a candidate),
 *      until one of them has no proposal; then the tour is done.  The switch is made per tour on the device.
 *   5. Stop test.  A sweep counts for a group if one of its tours moved, and counts as a full sweep as well if one of the tours
 *      that moved was in the full phase.  A group stops when all its tours are done or after max_iterations counted sweeps, over
 *      both phases; with max_iterations = 0 no sweep counts and nothing is applied.
 * So: with lists that name every other city every column is a candidate, and tours, sweeps and moves equal
 * difusco_tsp_multi_two_opt_ragged bit for bit; a tour is never longer than its start, every move shortens it by more than 1e-6;
 * with closing = 1 a tour that stops before the cap has no improving 2-opt move left; a tour's result does not depend on which
 * other tours or groups share the call, nor on how the threads are scheduled (a row's lowest (change, j) is combined with
 * atomic minima, whose result does not depend on their order).
 * sweeps_out, full_sweeps_out, moves_out: HOST int64 [groups]: the counted sweeps, the part of them counted as full sweeps, and
 * the moves applied over all tours of the group.  DIFUSCO_EINVAL before any GPU work on the conditions of
 * difusco_tsp_multi_two_opt_ragged, null neighbors, K < 1, closing outside {0, 1} and a short workspace.  Blocks until every
 * group is done.  The workspace holds what difusco_tsp_multi_two_opt_ragged's holds plus a position and a key per city and tour;
 * a tour's done and phase words are one state word, so _workspace_bytes returns 256 * ceil(4 tours / 256) bytes less than it did
 * while they were two (callers size the workspace by the function, so nothing else moves). */
int difusco_tsp_nbr_two_opt_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int K, int closing,
                                                   size_t* bytes);
int difusco_tsp_nbr_two_opt_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                   int32_t* tours, const int32_t* neighbors, int K, int closing, int64_t max_iterations,
                                   int select_rounds, void* workspace, size_t workspace_bytes, int64_t* sweeps_out,
                                   int64_t* full_sweeps_out, int64_t* moves_out, void* stream);

/* Multi-move local search, 2-opt + Or-opt (additive to ABI 13; not in the reference): the arrays, conventions and limits of
 * difusco_tsp_two_opt_ragged, the notation of the two comments above: the tour is closed (tour[n] == tour[0]), P_k is the point at
 * position k, d_k = |P_k P_k+1|, everything is float64 with every operation rounded on its own, a distance is two products, one
 * sum and a square root, the threshold is -1e-6, positions 0 and n never move.  Every TOUR runs on its own and keeps its own
 * phase, round and counters.  A tour runs ROUNDS of two phases:
 *   2-opt phase   the sweeps of difusco_tsp_multi_two_opt_ragged, exactly - steps 1-3 of its comment with the same
 *                 select_rounds -, until a sweep has no proposal;
 *   Or-opt phase  sweeps of three steps, until a sweep has no proposal:
 *     1. Row proposals.  Row i = 0 .. n-2 evaluates the candidates (v, i, j) of difusco_tsp_local_search_ragged that start at i:
 *        (L, reversed) = variant v of [(1,no), (2,no), (2,yes), (3,no), (3,yes)] with i <= n-1-L, 0 <= j <= n-1, j outside
 *        [i, i+L]; each with that comment's delta, bit for bit.  The row keeps its lowest delta, ties to the lowest v and then
 *        the lowest j (the flat-index order (v n + i) n + j within one row), and proposes if that delta is < -1e-6.  The key is
 *        (delta, i) (keys are distinct); the range is the half-open position interval [min(i, j), hi + 1) with hi = j for
 *        j > i+L and hi = i+L for j < i: from the first position of the lowest of the three edges the move touches to the first
 *        position of the highest, the convention of the 2-opt range [i, j+1).
 *     2. Selection.  Step 2 of the multi-move 2-opt, verbatim, over these keys and ranges.
 *     3. Apply.  Every winner applies its move as difusco_tsp_local_search_ragged defines it.  Only positions inside its range are
 *        rewritten and the winners' ranges are disjoint, so the order does not matter.
 * Stopping.  A tour is done after a round whose Or-opt phase applied nothing, after max_rounds rounds, or when it has moved in
 * max_iterations sweeps, both kinds counted together (with max_iterations = 0 nothing is applied).  The cap is per tour, so a
 * tour's result never depends on which other tours or groups share the call.  A done tour costs no further work; a group is done
 * when all its tours are.
 * So: the first 2-opt phase is the multi-move 2-opt - a tour on which the first Or-opt phase proposes nothing ends exactly as
 * difusco_tsp_multi_two_opt_ragged (without a binding cap) leaves it; every move shortens its tour by more than 1e-6, and no tour
 * ends longer than the multi-move 2-opt leaves it; a tour that stops below both caps has no improving 2-opt move and no improving
 * Or-opt move left.
 * Outputs, HOST arrays [groups]: two_opt_sweeps_out, or_opt_sweeps_out (int64) and rounds_out (int32) are the maxima over the
 * group's tours of the tour's own counts - the sweeps in which it moved, by kind, and the rounds it started (every tour starts
 * round 1); two_opt_moves_out, or_opt_moves_out (int64) are the sums over the group's tours of the moves applied.
 * DIFUSCO_EINVAL before any GPU work on the conditions of difusco_tsp_two_opt_ragged, a null output array, max_rounds < 1 and
 * select_rounds < 1.  Blocks until every group is done. */
int difusco_tsp_multi_local_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes);
int difusco_tsp_multi_local_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                          int32_t* tours, int64_t max_iterations, int max_rounds, int select_rounds, void* workspace,
                                          size_t workspace_bytes, int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out,
                                          int32_t* rounds_out, int64_t* two_opt_moves_out, int64_t* or_opt_moves_out, void* stream);

/* Neighbour-list multi-move local search, 2-opt + Or-opt, with a closing full descent (additive to ABI 13; not in the
 * reference): the arrays, conventions, limits and notation of difusco_tsp_multi_local_search_ragged, plus neighbors (DEVICE int32,
 * [group_n[g], K] per group, the groups concatenated), K >= 1 and closing in {0, 1} with exactly the conventions of
 * difusco_tsp_nbr_two_opt_ragged: city ids local to the group; an entry outside 0 .. n-1, or equal to its city, is a pad, is
 * skipped and never indexes memory; duplicates are allowed; N(a) = the non-pad entries of city a.
 * Every TOUR runs on its own and keeps its own stage (neighbour or full), phase, round and counters on the device.
 * NEIGHBOUR STAGE (every tour starts in it): the rounds of difusco_tsp_multi_local_search_ragged with candidate sweeps:
 *   2-opt phase   the neighbour sweep of difusco_tsp_nbr_two_opt_ragged, its steps 1-3 unchanged, until a sweep has no proposal;
 *   Or-opt phase  sweeps of three steps, until a sweep has no proposal:
 *     1. Candidates.  For the candidate (v, i, j) of difusco_tsp_local_search_ragged, (L, reversed) = variant v, let a and b be the
 *        cities at positions i+1 and i+L, swapped when reversed: the move creates the insertion edges (tour[j], a) and
 *        (b, tour[j+1]); position n is position 0.  Column j is a candidate of (v, i) iff tour[j] in N(a) or a in N(tour[j]) or
 *        tour[j+1] in N(b) or b in N(tour[j+1]): one of the two insertion edges joins a city to one of its listed neighbours, in
 *        either direction.  The gap edge (P_i, P_i+L+1) does not depend on j and defines no candidates.
 *     2. Row proposals.  Row i = 0 .. n-2 keeps the lowest delta over its candidates only - the delta of
 *        difusco_tsp_local_search_ragged, bit for bit -, ties to the lowest v and then the lowest j, and proposes iff that delta is
 *        < -1e-6.  Key (delta, i) and range as in difusco_tsp_multi_local_search_ragged.
 *     3. Selection and apply: steps 2 and 3 of difusco_tsp_multi_local_search_ragged's Or-opt phase, verbatim.
 * CLOSING.  A neighbour-stage round whose Or-opt phase applied nothing ends the neighbour stage.  With closing = 0 the tour is
 * done.  With closing = 1 the tour moves to the FULL STAGE: it goes on with the two phases of
 * difusco_tsp_multi_local_search_ragged (every column is a candidate), and rounds of these, until the Or-opt phase of one of
 * them applies nothing.  The switch is made per tour on the device.  The first pair of full phases takes the place of the stop
 * of the round that ended the neighbour stage and runs under that round's number; every later full round starts a new round.
 * CAPS.  max_iterations and max_rounds are per tour and count over both stages together: max_iterations the sweeps in which the
 * tour moved (with 0 nothing is applied), max_rounds the rounds started.  A tour that hits a cap is done in whatever stage it is
 * in; it does not enter the full stage because of a cap: a tour whose max_rounds-th round applied an Or-opt move is done.
 * So: with lists that name every other city every column is a candidate, and the tours and the five counters shared with
 * difusco_tsp_multi_local_search_ragged equal that entry's bit for bit, with either closing - the full phases then find
 * nothing, full_sweeps is 0 and, for a tour that stops below both caps, full_rounds is 1 -; every move shortens its tour by more than 1e-6; with closing = 1 a tour
 * that stops below both caps has no improving 2-opt move and no improving Or-opt move left; a tour's result depends neither on
 * what shares the call nor on how the threads are scheduled (a row's lowest (delta, v, j) is combined with atomic minima, whose
 * result does not depend on their order).
 * Outputs, HOST arrays [groups]: the five of difusco_tsp_multi_local_search_ragged with its max / sum conventions, over both
 * stages; full_sweeps_out (int64): the maximum over the group's tours of the sweeps in which the tour moved while in the full
 * stage; full_rounds_out (int32): the maximum over the tours of the rounds run in the full stage (0: no tour reached it).
 * DIFUSCO_EINVAL before any GPU work on the conditions of difusco_tsp_multi_local_search_ragged and of
 * difusco_tsp_nbr_two_opt_ragged: null neighbors, K < 1, closing outside {0, 1}, max_rounds < 1, select_rounds < 1, a null
 * output array, a short workspace.  Blocks until every group is done. */
int difusco_tsp_nbr_local_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int K,
                                                        int closing, size_t* bytes);
int difusco_tsp_nbr_local_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                        int32_t* tours, const int32_t* neighbors, int K, int closing, int64_t max_iterations,
                                        int max_rounds, int select_rounds, void* workspace, size_t workspace_bytes,
                                        int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out, int32_t* rounds_out,
                                        int64_t* two_opt_moves_out, int64_t* or_opt_moves_out, int64_t* full_sweeps_out,
                                        int32_t* full_rounds_out, void* stream);

/* Iterated multi-move local search: seeded segment kicks between descents (additive to ABI 13; not in the reference): the
 * arrays, conventions and limits of difusco_tsp_multi_local_search_ragged, plus kicks >= 0, kick_size in 1 .. 64, span >= 1 and
 * tour_seeds / tour_offsets: DEVICE uint64 [T], T = the tours of the call in tour order (group after group): the Philox key and
 * the first Philox offset of every tour (the types of difusco_step_args' instance table).  Every TOUR runs on its own, with its
 * own kick counter, incumbent and counters; nothing a tour does depends on what shares the call.
 *   1. First descent.  The incumbent I is the search of difusco_tsp_multi_local_search_ragged on the input tour with
 *      max_iterations, max_rounds and select_rounds.  The caps are per descent.
 *   2. Kick t = 0 .. kicks-1, drawn from I.  Lc = min(span, (n-1)/2) (integer division; >= 1 since n >= 4).  Draw
 *      c = 0 .. kick_size-1 takes the words w0, w1, w2 of Philox4x32-10 with key seed, counter (c, offset + t) - the offset
 *      modulo 2^64 - and sets, in unsigned 32-bit arithmetic, l1 = 1 + w1 % Lc, l2 = 1 + w2 % Lc, a = 1 + w0 % (n - l1 - l2),
 *      b = a + l1 + l2; so 1 <= a and b <= n: positions 0 and n never move.  Draw c is KEPT iff [a, b) intersects the range of no
 *      kept draw with a lower c, decided in rising c (adjacent ranges do not intersect).  Every kept draw swaps its two adjacent
 *      segments: C[a .. b) = I[a+l1 .. b) ++ I[a .. a+l1), the local double bridge; C = I elsewhere.  The ranges are disjoint and
 *      are read from I, so the order does not matter.
 *   3. Descent of C as in step 1, with fresh caps and round counter.
 *   4. Keep.  len(X) = sum of d_k over the positions k = 0 .. n-1 of the closed tour, d_k = |P_k P_k+1| as above (the
 *      coordinates of position k minus those of position k+1, two products, one sum, one square root), in ONE association:
 *      s_r = the sum of d_r, d_r+1024, d_r+2048, .. in rising k starting from 0.0, r = 0 .. 1023 (0.0 where r >= n); then for
 *      h = 512, 256, .. 1: s_r = s_r + s_r+h for r < h; len = s_0.  I <- C iff len(C) <= len(I) (a plateau result is kept).
 *      len(I) is computed once, when I changes.
 *   5. The output tour is I after the last kick.
 * So: the result is a permutation closed on tour[0]; its len is never above that of the kicks = 0 result under the same caps;
 * the same (seed, offset) gives a tour the same result in a solo, a grouped and a ragged call; different seeds give different
 * kicks.  kicks = 0 returns what difusco_tsp_multi_local_search_ragged returns, tours and counters alike.  With
 * max_iterations = 0 no descent moves a tour and the call is the keeps and kicks alone.
 * Outputs.  The five HOST arrays [groups] of difusco_tsp_multi_local_search_ragged: a tour's sweeps and moves are summed over
 * all its descents and then combined over the group's tours as there (maxima of the sweeps, sums of the moves); rounds_out is
 * the maximum over the group's tours and their descents of the rounds a descent started.  HOST arrays [T] per tour: kicks_kept_out
 * (int32; kicks whose descent ended not longer than the incumbent), kicks_improved_out (int32; strictly shorter),
 * segments_swapped_out (int64; kept draws over all kicks), first_length_out and final_length_out (float64; len of the first
 * descent's result and of the output tour).
 * DIFUSCO_EINVAL before any GPU work on the conditions of difusco_tsp_multi_local_search_ragged, a null new array, kicks < 0,
 * kick_size outside 1 .. 64 and span < 1; a refused call leaves `tours` untouched.  The kick loop runs on the device behind the
 * phase word of the descent: the host enqueues launch sequences (the three launches of a sweep and the keep / kick step) and
 * polls the counter of stopped groups every 8.  Blocks until every group is done.
 * difusco_tsp_search_host_syncs: the host synchronisations of the calling thread's last difusco_tsp_iterated_search_ragged
 * call. */
int difusco_tsp_iterated_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes);
int difusco_tsp_iterated_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                       int32_t* tours, int64_t max_iterations, int max_rounds, int select_rounds, int32_t kicks,
                                       int32_t kick_size, int32_t span, const uint64_t* tour_seeds, const uint64_t* tour_offsets,
                                       void* workspace, size_t workspace_bytes, int64_t* two_opt_sweeps_out,
                                       int64_t* or_opt_sweeps_out, int32_t* rounds_out, int64_t* two_opt_moves_out,
                                       int64_t* or_opt_moves_out, int32_t* kicks_kept_out, int32_t* kicks_improved_out,
                                       int64_t* segments_swapped_out, double* first_length_out, double* final_length_out,
                                       void* stream);
int difusco_tsp_search_host_syncs(void);

/* Iterated multi-move local search with FOCUSED descents after the kicks (additive to ABI 13; not in the reference): the
 * arrays, conventions, limits and rule of difusco_tsp_iterated_search_ragged except for the points below.  Every TOUR runs on
 * its own.
 *   First descent.  The full search of difusco_tsp_multi_local_search_ragged, exactly as there.
 *   Marks.  A tour keeps two sets of CITIES, S (current) and T (touched since the kick).  Position k = 0 .. n-1 of the tour is
 *     ACTIVE iff tour[k] and tour[k+1] are both in S: the edge k -> k+1 is suspect.
 *   After kick t.  T is set to the cities that C holds at positions a-1, a, a+l2-1, a+l2, b-1 and b of every kept draw: the six
 *     end cities of the three edges a kept draw creates.
 *   Descent after a kick.  The rounds, phases, caps and stop tests of difusco_tsp_multi_local_search_ragged (max_iterations and
 *     max_rounds per descent, select_rounds as there).  Each phase begins with S := T.  A sweep evaluates only these candidates:
 *       2-opt   (i, j) iff position i or position j is active;
 *       Or-opt  (v, i, j) iff row i is ROW-ACTIVE - one of the positions i .. i+3, clipped to n-1, is active - or position j is
 *               active.
 *     Within the evaluated candidates everything is that comment's, bit for bit: the changes and deltas, the row's lowest value
 *     with ties to the lowest j (or the lowest v, then j), the threshold -1e-6, the key (value, i), the ranges, the selection
 *     and the apply.  A row without an evaluated candidate does not propose.
 *   Marks after a sweep, with the tour as it was before the apply.  S := the cities at the ends of the removed edges of EVERY
 *     proposal of the sweep, winner or not - 2-opt: positions i, i+1, j, j+1; Or-opt: i, i+1, i+L, i+L+1, j, j+1.  T := T + the
 *     same cities of the winners only.
 *   Closing descent, only when kicks > 0 and max_iterations > 0.  After the keep of the last kick one FULL descent of the
 *     incumbent follows, with fresh caps.  Its result replaces the incumbent iff its len is not larger (the keep rule and the
 *     len of step 4 there); it counts in neither kicks_kept_out nor kicks_improved_out.  The output is the incumbent after that.
 * So: the output is a permutation closed on tour[0]; its len is never above first_length_out; where no cap binds it has no
 * improving 2-opt or Or-opt move left; the same (seed, offset) gives a tour the same result in a solo, a grouped and a ragged
 * call; kicks = 0 returns what difusco_tsp_multi_local_search_ragged returns, tours and counters alike.
 * compact_select_max, 0 .. 1024: a sweep of a focused descent with at most this many proposals is selected by one thread per
 * proposal, every proposal against all (step 2 of the multi-move 2-opt read literally, O(m^2 / 1024) per round); a sweep with
 * more, and every sweep with 0, by the selection of the full descents.  The winners are the same: the argument changes the cost
 * alone.  closing_sweeps_out: HOST int32 [T], the sweeps in which the tour's closing descent moved it; 0: the focused descents
 * missed nothing.  The other outputs are those of difusco_tsp_iterated_search_ragged; the group counters sum all descents, the
 * closing one included.
 * DIFUSCO_EINVAL before any GPU work on the conditions of difusco_tsp_iterated_search_ragged, compact_select_max out of range
 * and a null closing_sweeps_out; a refused call leaves `tours` untouched.  The host enqueues launch sequences (five launches:
 * the three of a sweep, the focused row-best and the keep / kick step) and polls the counter of stopped groups every 8; at most
 * (the bound of a descent) x (kicks + 2) sequences.  Blocks until every group is done.  difusco_tsp_search_host_syncs also
 * reports this call. */
int difusco_tsp_focused_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, size_t* bytes);
int difusco_tsp_focused_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                      int32_t* tours, int64_t max_iterations, int max_rounds, int select_rounds, int32_t kicks,
                                      int32_t kick_size, int32_t span, const uint64_t* tour_seeds, const uint64_t* tour_offsets,
                                      int32_t compact_select_max, void* workspace, size_t workspace_bytes,
                                      int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out, int32_t* rounds_out,
                                      int64_t* two_opt_moves_out, int64_t* or_opt_moves_out, int32_t* kicks_kept_out,
                                      int32_t* kicks_improved_out, int64_t* segments_swapped_out, double* first_length_out,
                                      double* final_length_out, int32_t* closing_sweeps_out, void* stream);

/* Iterated multi-move local search with HEAT-BIASED kicks (additive to ABI 13; not in the reference): the arrays, conventions,
 * limits and rule of difusco_tsp_iterated_search_ragged (descent = 0) or of difusco_tsp_focused_search_ragged (descent = 1;
 * compact_select_max is read only then) except for how draw c of kick t gets `a`.  Every TOUR runs on its own.
 *   Inputs.  Group g carries a directed candidate graph in CSR over its n_g cities: row_ptr int32 [n_g + 1] and col int32 [E_g],
 *     E_g = group_edges[g] (HOST [groups]).  Rows may have any degree, 0 included; duplicate (u, v) entries and self edges are
 *     allowed.  Every tour of the group has one heat float32 [E_g] in that edge order.  DEVICE arrays: row_ptr, the groups'
 *     arrays one after the other (sum of n_g + 1 entries); col (sum of E_g); heat (sum of P_g E_g), tour after tour in the
 *     call's tour order.
 *   Quantised heat.  q(e) = (uint32) rint(clamp(heat_e, 0, 1) * 65535.0f): the product in float32, rint to nearest even, the
 *     clamp fminf(fmaxf(h, 0.0f), 1.0f), so a NaN counts as 0.  q(u, v) = the largest q(e) over the entries e of row u with
 *     col[e] == v, 0 if there is none.
 *   Weights, from the incumbent I when kick t is drawn.  Position k = 0 .. n-1 has w_k = 65536 - max(q(I[k], I[k+1]),
 *     q(I[k+1], I[k])), an integer in 1 .. 65536: no position is ever impossible.  W_0 = 0, W_k+1 = W_k + w_k, in uint64.
 *   Draw c.  The words w0 .. w3 of the same Philox call (key seed, counter (c, offset + t)); l1 and l2 from w1 and w2 as there;
 *     M = n - l1 - l2; r = ((uint64) w0 << 32 | w3) mod W_M; p the position with W_p <= r < W_p+1; a = p + 1, so 1 <= a <= M,
 *     the range of the uniform rule.  A cut falls after position p with a probability that rises as the heat of the tour edge
 *     there falls.
 *   Everything else - the kept-draw filter, the segment swap, the marks of a focused descent (they follow from a, l1, l2), the
 *     descents, the keep rule, the counters and outputs - is unchanged.
 * So: the output is a permutation closed on tour[0], never longer than first_length_out; the same (seed, offset, heat) gives a
 * tour the same result in a solo, a grouped and a ragged call; kicks = 0 returns what difusco_tsp_multi_local_search_ragged
 * returns, whatever the heat.  Constant heat is NOT the uniform rule: it takes r mod W_M where that one takes w0 mod M, so the
 * two entries above and this one give different tours on the same seed.
 * closing_sweeps_out may be null when descent = 0 (where it is given it receives zeros).  The workspace size does not depend
 * on descent.  DIFUSCO_EINVAL before any GPU work on the conditions of the entry it extends, a null group_edges / row_ptr /
 * col / heat, group_edges[g] < 0 and descent outside {0, 1}.  Before the search starts one small kernel checks every group's
 * row_ptr (row_ptr[0] = 0, rising, row_ptr[n_g] = E_g) and col (0 <= col < n_g) on the device; its flag comes back with the
 * setup synchronisation, and a bad graph is DIFUSCO_EINVAL instead of a read out of bounds.  A refused call leaves `tours`
 * untouched.  The launch sequences, grid sizes and host polls are those of the entry it extends, with the heat instantiation
 * of the keep / kick kernel: behind the keep copy the tour's block computes w_k (two row scans per position) and W in n + 1
 * uint64 words of the workspace, and one lane per draw searches W_0 .. W_M.  Behind the check one more kernel writes q by
 * (tour, entry) once per call, 16 bits each in the workspace (hence group_edges in _workspace_bytes), with duplicates resolved:
 * the first entry of a pair (u, v) in row u holds q(u, v), so a row scan ends at its first match - a few reads where rows list
 * near cities first, as k-NN rows do.  That pass costs E_g x (degree) reads per tour and call.  difusco_tsp_search_host_syncs
 * also reports this call. */
int difusco_tsp_guided_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours,
                                                     const int32_t* group_edges, size_t* bytes);
int difusco_tsp_guided_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                     int32_t* tours, int64_t max_iterations, int max_rounds, int select_rounds, int32_t kicks,
                                     int32_t kick_size, int32_t span, const uint64_t* tour_seeds, const uint64_t* tour_offsets,
                                     int32_t compact_select_max, int32_t descent, const int32_t* group_edges,
                                     const int32_t* row_ptr, const int32_t* col, const float* heat, void* workspace,
                                     size_t workspace_bytes, int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out,
                                     int32_t* rounds_out, int64_t* two_opt_moves_out, int64_t* or_opt_moves_out,
                                     int32_t* kicks_kept_out, int32_t* kicks_improved_out, int64_t* segments_swapped_out,
                                     double* first_length_out, double* final_length_out, int32_t* closing_sweeps_out,
                                     void* stream);

/* Heatmap-guided sampled k-opt search (additive to ABI 13): a parallel, deterministic restatement of the sampling, selection and
 * weight update of the reference's last TSP stage (tsp_mcts/code/TSP_MCTS.h), not a port of it.  Groups, points (float64), closed
 * int32 tours [n+1], n >= 4, the per-group CSR candidate graph (group_edges HOST [groups], row_ptr, col DEVICE), one heat float32
 * [E_g] per tour, tour_seeds / tour_offsets (DEVICE uint64 [T]) and the device-side graph check are those of
 * difusco_tsp_guided_search_ragged.  New: samples S in 1 .. 4096, depth D in 1 .. 10, max_rounds R >= 0, patience H >= 1, beta
 * (float64, finite, >= 0) and explore: HOST float64 [R], finite and >= 0 - an input, so that no logarithm has to agree between two
 * math libraries (the Python layer fills it with alpha sqrt(log1p(r S))).  Every TOUR runs on its own; nothing it does depends
 * on what shares the call.  All arithmetic is float64 + - x / sqrt without contraction, or integer.
 *   State of a tour.  The incumbent I (positions 0 .. n-1, closed on I[0]).  Entry e of row u is a CANDIDATE of u iff col[e] != u
 *     and no earlier entry of the row has the same column.  Per candidate entry the weight w[e] = 100.0 (double) clamp(heat_e, 0,
 *     1) - the clamp fminf(fmaxf(h, 0), 1), so a NaN counts as 0 - and the count C[e] = 0 (int32).  Per city sw[u] = the sum of w
 *     over the candidates of u in rising e, from 0.0.  len(I) in the association of step 4 of
 *     difusco_tsp_iterated_search_ragged, computed when I changes.  stall = 0.
 *   Round r = 0 .. R-1.  All S simulations of a round read I, w, sw and C as they stood at the start of the round.
 *     Draws.  Simulation s uses the words of Philox4x32-10 with key seed and offset offset + r (mod 2^64); call j has index
 *       (j << 32) | s; step i takes word i mod 4 of call i div 4; the begin position is step 0.
 *     Start.  p = word % n, a1 = I[p], b_1 = I[(p+1) mod n]; path position x = 0 .. n-1 is I[(p+1+x) mod n].  Gain_0 =
 *       d(a1, b_1), d(u, v) = the distance of two_opt's pairs: the coordinate differences, two products, one sum, one square root.
 *     Step i = 1 .. D, head b_i at path position 0.  avg = sw[b_i] / (n-1); if avg is not > 0 the simulation ends.  Candidate e
 *       of b_i with c = col[e] is PROMISING iff c != a1, c is not at current path position 1 and
 *       pot(e) = w[e] / avg + explore[r] / sqrt((double)(C[e] + 1)) >= 1.0.  tot = the sum of pot over the promising entries in
 *       rising e, from 0.0; none: the simulation ends.  Cumulative c_k = c_k-1 + (int)((1000.0 pot_k) / tot), the last promising
 *       entry has c = 1000; the draw is word % 1000 and the first k with draw < c_k is chosen.  y = the current path position of
 *       the chosen city c (2 <= y <= n-2), b_i+1 = the city at position y-1, Gain_i = Gain_i-1 - d(b_i, c) + d(c, b_i+1) (left
 *       to right), Real_i = Gain_i - d(b_i+1, a1).  The path prefix [0, y) is reversed: b_i+1 is the new head.  The simulation
 *       ends after this step if Real_i > 1e-6 or i == D.
 *     Value of a simulation: the largest Real_i, at the lowest such i = i*; a simulation without a step has none.
 *     Counts, after the round: for every step taken by every simulation C of the chosen entry grows by 1, and so does C of the
 *       candidate entry (c, b_i) of row c where it exists.
 *     Best of the round: the largest value, ties to the lowest s.  If it is > 1e-6: the new incumbent is the path after the first
 *       i* reversals of that simulation - path position x becomes tour position x, then the tour is rotated so that the city at
 *       input position 0 is at position 0 again.  x = value / len(I) (before the change), inc = beta (x + (0.5 x) x) in that
 *       association.  For every added edge - (b_i, c_i) for i <= i* and (b_i*+1, a1) -, in step order, and for both of its
 *       orientations (u, v), first as listed: w[entry(u, v)] += inc where that candidate entry exists, sw[u] += inc always.  len
 *       is recomputed and stall = 0.  Otherwise stall += S, and the tour stops when stall >= H n (int64).
 *   Output.  I, or the input tour if len(I) > len(input); reverted_out reports that case (expected: 0).  R = 0 returns the input.
 * So: the output is a permutation closed on tour[0], never longer than the input; the same (seed, offset, heat) gives a tour the
 * same result in a solo, a grouped and a ragged call.
 * Deviations from TSP_MCTS.h.  (1) The simulations of a round run in parallel on frozen counts; the reference is sequential and
 * breaks at the first improving action.  (2) The total simulation count enters through explore[r].  (3) Distances are float64,
 * not integers magnified 10^4.  (4) The improvement threshold is 1e-6.  (5) exp(x) - 1 is replaced by x + x^2 / 2, because exp is
 * not correctly rounded.  (6) Weights live on the sparse candidate entries, with dense row sums.  (7) There is no random restart
 * and no built-in 2-opt stage: the caller's local search runs before it.  (8) Termination is by stall or round cap, not by clock.
 * HOST outputs [T] per tour: rounds_out (int32; rounds run), actions_out (int32; actions applied), depth_sum_out (int64; the sum
 * of their i*), reverted_out (int32), first_length_out and final_length_out (float64; len of the input and of the output).
 * DIFUSCO_EINVAL before any GPU work on the group conditions of difusco_tsp_guided_search_ragged, a null array, samples, depth,
 * max_rounds, patience, beta or an explore entry out of range, group_edges[g] < 0 and a workspace that is too small; a bad CSR
 * is refused by the device check with the setup synchronisation.  A refused call leaves `tours` untouched.  _workspace_bytes
 * takes samples and depth: the workspace holds, per tour, two tours, the inverse, sw, w and C and per simulation its value, i*,
 * step count, begin position and D x (entry, mirror entry, cut).  Launches: per round one thread per simulation over a grid of
 * (tours x ceil(S / 256)) blocks - a single large tour still fills the chip - and one block per tour for the end of the round;
 * no block waits on another.  The host enqueues rounds without synchronising and polls the count of stopped tours every 8.
 * Blocks until every tour is done.  difusco_tsp_search_host_syncs also reports this call. */
int difusco_tsp_kopt_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours,
                                                   const int32_t* group_edges, int32_t samples, int32_t depth, size_t* bytes);
int difusco_tsp_kopt_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                   int32_t* tours, const int32_t* group_edges, const int32_t* row_ptr, const int32_t* col,
                                   const float* heat, const uint64_t* tour_seeds, const uint64_t* tour_offsets, int32_t samples,
                                   int32_t depth, int32_t max_rounds, int32_t patience, double beta, const double* explore,
                                   void* workspace, size_t workspace_bytes, int32_t* rounds_out, int32_t* actions_out,
                                   int64_t* depth_sum_out, int32_t* reverted_out, double* first_length_out,
                                   double* final_length_out, void* stream);

/* Candidate lists for the neighbour-list searches FROM THE HEATMAPS (additive to ABI 13; not in the reference - its search stage
 * lists candidates by heat too, tsp_mcts/code/TSP_Basic_Functions.h:171-212; this is a parallel, deterministic rule of our own).
 *   Inputs.  Those of difusco_tsp_guided_search_ragged: group g has n_g cities, P_g = group_tours[g] tours, points float64, the
 *     directed candidate graph in CSR (row_ptr int32 [n_g + 1], col int32 [E_g], E_g = group_edges[g]; any degrees, 0 included;
 *     duplicate entries and self edges allowed) and one heat float32 [E_g] per tour in that entry order; DEVICE arrays laid out as
 *     there.  No tour is read, so n_g >= 1 suffices here (the searches need n_g >= 4).  New: K, 1 <= K <= 128.
 *   Quantised heat.  q_t(u, v) for tour t of the group exactly as defined there: q(e) = (uint32) rint(clamp(heat_e, 0, 1) *
 *     65535.0f), a NaN counts as 0, q_t(u, v) = the largest q(e) over the entries e of row u with col[e] == v, 0 if there is none.
 *   Score.  S(a, b) = the sum over the group's tours t of (q_t(a, b) + q_t(b, a)), an integer held in 64 bits: symmetric, and
 *     independent of the order of the tours and of the entries.
 *   Candidate set.  C(a) = { b != a : b is a column of row a, or a is a column of row b }.
 *   List of a.  The members of C(a) sorted by (S(a, b) descending, d2(a, b) ascending, b ascending), d2 = dx dx + dy dy in
 *     float64 with every operation rounded on its own (dx, dy the coordinate differences).  The first K go to
 *     neighbors_out[(cities before the group) K + a K + 0 .. K-1] (DEVICE int32), cities local to the group; if |C(a)| < K the
 *     remaining slots hold -1, the pad convention of difusco_tsp_nbr_two_opt_ragged.
 * So: every row holds distinct cities, never the city itself, and pads only at its end; a group's lists depend neither on what
 * shares the call nor on how threads are scheduled; they do not change when the entries inside a row are permuted or the group's
 * tours are reordered; with all-zero heat on a k-NN graph whose rows are in (d2, index) order and pairwise distinct distances
 * per city they are the first K non-self neighbours of every row for K <= k - 1; with K = n - 1 on the complete graph every
 * list names every other city, so the neighbour-list searches sweep what the full sweeps do.
 * Outputs on the host, HOST int64 [groups]: listed_out (the list entries with S > 0, summed over the group's cities) and pads_out
 * (the pad slots).
 * DIFUSCO_EINVAL before any GPU work on null pointers, K outside 1 .. 128, groups < 1, n_g < 1 or above the limit of the
 * searches, P_g < 1, more tours than a call of the searches takes, E_g < 0 and a workspace that is too small.  The graphs pass the
 * device check of the guided search first; its flag comes back with the one synchronisation in front of the work, and a bad
 * graph is DIFUSCO_EINVAL with neighbors_out untouched.  Behind it: the q table of the guided search; one thread per entry for
 * the sums over the tours and the in-degrees (integer atomics); one block per group for the row pointers of the transpose; one
 * thread per entry to scatter the transpose (arbitrary order inside a row - the list order is total); one wave per city for the
 * selection - it gathers the out-row and the in-row, drops the city itself, repeated columns and incoming cities the out-row
 * names, and takes K rounds of a wave-wide lexicographic maximum, so any degree works.  Launch boundaries are the only
 * synchronisation.  _workspace_bytes: per group about 2 P_g E_g (the q table) + 32 E_g (the sums, the transpose and the 2 E_g
 * selection slots of 12 bytes) + 8 n_g bytes.  Blocks until done. */
int difusco_tsp_heat_candidates_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours,
                                                       const int32_t* group_edges, int32_t K, size_t* bytes);
int difusco_tsp_heat_candidates_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const int32_t* group_edges,
                                       const double* points, const int32_t* row_ptr, const int32_t* col, const float* heat,
                                       int32_t K, int32_t* neighbors_out, void* workspace, size_t workspace_bytes,
                                       int64_t* listed_out, int64_t* pads_out, void* stream);

/* WINDOWED iterated multi-move local search: one block per tour window (additive to ABI 13; not in the reference): the arrays,
 * conventions and limits of difusco_tsp_iterated_search_ragged, plus window = W in 16 .. 1024, passes = R >= 1 and kicks = K in
 * 0 .. 1024 per window and pass.  Every TOUR runs on its own; its result never depends on what shares the call.
 *   1. First descent.  The search of difusco_tsp_multi_local_search_ragged on the input tour, exactly: T_-1.
 *   2. Pass r = 0 .. R-1, on T_r-1.  o_r = 0 for even r and W/2 (integer division) for odd r.  The cuts are 0, n and every
 *      o_r + w W with 0 < o_r + w W < n, in rising order c_0 < .. < c_M.  Window w is the open path Q_k = T_r-1[c_w + k],
 *      k = 0 .. m, m = c_w+1 - c_w <= W.  A window with m < 8 is copied unchanged.  Every other window is searched by steps 1-5
 *      of difusco_tsp_iterated_search_ragged's rule, verbatim, with n := m and P_k := the coordinates of Q_k for k = 0 .. m (so
 *      P_m is Q_m, not P_0): a first descent of the path, K kicks, each drawn from the incumbent, descended with fresh caps and
 *      kept iff not longer.  Positions 0 and m never move - no move and no draw of that rule touches them -, so the cities on
 *      the cuts stay.  The caps are those of the call (max_iterations, max_rounds, select_rounds, kick_size, span); the len of
 *      step 4 is that association with n := m; the Philox key is the tour's seed and the first Philox offset is the tour's
 *      offset + (r C + w) K modulo 2^64, C = ceil(n / W) + 1.  The candidate X is the concatenation of the window results.
 *      T_r = X iff len(X) <= len(T_r-1), the tour-level len of step 4 there; otherwise T_r = T_r-1.  (A change inside a window
 *      changes only edges of that window, so X is never longer up to the rounding of the window sums; the pass-level keep makes
 *      "never longer" an exact float64 statement.)
 *   3. Closing.  One full descent of T_R-1 as in step 1, kept iff its len is not larger.
 *   4. The output is that tour.
 * So: the output is a permutation closed on tour[0] with final_length_out <= first_length_out exactly; where no cap binds it has
 * no improving 2-opt or Or-opt move left; the same (seed, offset) gives a tour the same result in a solo, a grouped and a ragged
 * call; for n <= W and R = 1 the tour, both lengths and the kick counters are those of difusco_tsp_iterated_search_ragged with
 * kicks = K (the cuts are 0 and n, the path is the closed tour and the offset is the tour's own) where no cap binds.
 * Outputs.  The five HOST arrays [groups] cover the first and the closing descent: each descent's values, combined over the
 * group's tours as difusco_tsp_multi_local_search_ragged does, are added (rounds_out: the larger of the two).  HOST arrays [T]
 * per tour: first_length_out, final_length_out (float64; len of T_-1 and of the output); passes_kept_out (int32; passes with
 * T_r = X); windows_searched_out (int32; windows with m >= 8, over all passes); kicks_kept_out, kicks_improved_out (int32) and
 * segments_swapped_out (int64) as in difusco_tsp_iterated_search_ragged, summed over windows and passes, kept pass or not;
 * window_sweeps_out, window_moves_out (int64; the sweeps in which a window moved and the moves applied, both kinds together,
 * summed likewise); closing_sweeps_out (int32; the sweeps in which the closing descent moved the tour).
 * DIFUSCO_EINVAL before any GPU work on the conditions of difusco_tsp_iterated_search_ragged, a null new array, window outside
 * 16 .. 1024, passes < 1, kicks outside 0 .. 1024 and a tour with R C max(K, 1) >= 2^32 (the Philox offsets of two tours keyed
 * 2^32 apart could meet); a refused call leaves `tours` untouched.  _workspace_bytes takes `window`: the workspace holds the
 * descents' workspace, one candidate per tour and the window tables of the even and the odd passes.  Launches: the first and
 * the closing descent are those of difusco_tsp_multi_local_search_ragged; between them the host enqueues 2 R launches with no
 * synchronisation - per pass one block of 1024 threads per window, which keeps the window's coordinates, paths, edge lengths,
 * row bests and selection lists in 54 KB of LDS and runs all its descents, kicks and keeps there (at most (K + 1) x
 * (max_iterations + 2 max_rounds) sweeps; no block waits on another), and one block per tour for the pass-level len and keep.
 * Blocks until every tour is done. */
int difusco_tsp_window_search_ragged_workspace_bytes(int groups, const int32_t* group_n, const int32_t* group_tours, int32_t window,
                                                     size_t* bytes);
int difusco_tsp_window_search_ragged(int groups, const int32_t* group_n, const int32_t* group_tours, const double* points,
                                     int32_t* tours, int64_t max_iterations, int max_rounds, int select_rounds, int32_t kicks,
                                     int32_t kick_size, int32_t span, const uint64_t* tour_seeds, const uint64_t* tour_offsets,
                                     int32_t window, int32_t passes, void* workspace, size_t workspace_bytes,
                                     int64_t* two_opt_sweeps_out, int64_t* or_opt_sweeps_out, int32_t* rounds_out,
                                     int64_t* two_opt_moves_out, int64_t* or_opt_moves_out, int32_t* kicks_kept_out,
                                     int32_t* kicks_improved_out, int64_t* segments_swapped_out, double* first_length_out,
                                     double* final_length_out, int32_t* passes_kept_out, int32_t* windows_searched_out,
                                     int64_t* window_sweeps_out, int64_t* window_moves_out, int32_t* closing_sweeps_out,
                                     void* stream);

/* ---- MCTS heatmap rows: the numeric part of tsp_mcts/convert_numpy_to_txt.py:18-47, whose text output
 * (first line N, then N rows of N "%.6f" numbers) tsp_mcts/code/include/TSP_IO.h:461-492 reads.  From the SPARSE heatmap:
 * row/col/heat [n_edges] DEVICE, any order, no duplicate (row, col); points DEVICE float32 [n_nodes,2]; float32 arithmetic
 * in numpy's operation order (no fused multiply-add, numpy's chunked pairwise row sums), so that the rows equal the
 * reference program's bit for bit.  prepare(): CSR of heat and its transpose, the threshold (k-th largest positive value,
 * k = int(N*N*prob), exact radix select; k = 0 selects the smallest positive value like the reference's
 * valid_values[-0]) and the row top-3 - kept in `workspace`; *threshold_out (HOST, optional).  rows(): the normalised
 * rows [row_begin, row_begin + row_count) into out_rows (DEVICE, [row_count, n_nodes]).  n_nodes <= 38000 (a row lives
 * in LDS).  Both block until done. */
/* HOST helper (no GPU): the float32 sum of a[0..n) in the order of the row-sum program the kernels execute (numpy's
 * add.reduce over a contiguous float32 row: 8192-element chunks, pairwise summation inside) - exported so that the CPU
 * tests can hold that program against numpy itself. */
int difusco_host_rowsum_f32(const float* a, int n, float* out);
int difusco_mcts_heatmap_workspace_bytes(int n_nodes, int64_t n_edges, size_t* bytes);
int difusco_mcts_heatmap_prepare(int n_nodes, int64_t n_edges, const int32_t* row, const int32_t* col, const float* heat,
                                 const float* points, double expected_valid_prob, void* workspace, size_t workspace_bytes,
                                 float* threshold_out, void* stream);
int difusco_mcts_heatmap_rows(int n_nodes, int64_t n_edges, const float* points, const void* workspace,
                              size_t workspace_bytes, int row_begin, int row_count, float* out_rows, void* stream);

/* ---- in-library profiler (bench.py): HIP events on the launch stream around every kernel launch of
 * difusco_denoise_step, summed per category.  Categories: 0 edge-row linear (rows = n_edges),
 * 1 node-row linear, 2 edge gate/aggregate, 3 head (GroupNorm+conv+posterior, 3 launches),
 * 4 embeddings / time features / memset.  enable(1, max) (re)arms and pre-creates the events; enable(2, max)
 * brackets category 0 only (every bracket costs a few microseconds of dispatch gap: ~2.7 % of a step for all five);
 * collect() synchronises, fills ms[c] / launches[c] for c < 5, re-arms, returns brackets read. */
#define DIFUSCO_PROFILE_CATEGORIES 5
int difusco_profile_enable(int on, int max_launches);
int difusco_profile_collect(double* ms, int64_t* launches, int n_categories);

#ifdef DIFUSCO_PROFILING
/* Profiling library only (libdifusco_hip_prof.so, built with -DDIFUSCO_PROFILING; `python -m difusco_amd.build --prof`):
 * process-wide knobs that select timing-only variants of the fused edge-layer kernel.  The production library does
 * not export these symbols and holds no such state.
 * key 0: compile-time ablation mask (bit0 skip neighbour-table gathers, bit1 skip the neighbour sum, bit2 skip
 *        LN/activation math, bit3 skip GEMM 2, 16 = production code + phase stamps ...): results are WRONG by design;
 * key 6: extra dynamic LDS bytes (occupancy probe);  key 7: A/B variant of the scheduling options (OPT bits);
 * key 8: k steps of load lookahead in the node-row linear (0, 1 or 4);  key 9: start delay (cycles) of the second-slot workgroups of
 *        the fused kernel's first dispatch generation (experiment of round 3);  key 10: timing-only ablation mask of the node-row
 *        linear (node_linear.hip, 0..31). */
int difusco_debug_set(int key, int value);
/* key 1: device buffer [n_tiles][16] of uint64 receiving s_memtime stamps of the fused kernel's phases (NULL disables) */
int difusco_debug_set_ptr(int key, void* p);
/* Stage-loop laboratory (csrc/stage_lab.hip): GEMM 1 of the fused edge layer alone - out = C e on the tiled e stream
 * (fp16 hi | lo planes of C, 3 MFMA products, weight stages through LDS by LDS-DMA) - in the workgroup geometry /
 * synchronisation scheme `variant` names (EPW/32 * 100000 + WAVES * 10000 + NBUF * 1000 + SYNC * 100 + RING * 10 + PRIO).
 * e / out: DEVICE, tiled [n_edges, 256] (n_edges a multiple of the variant's edges per workgroup); inv_c = 2^-kc of the
 * planes; do_store 0 = timing only; lds_pad = extra dynamic LDS bytes.  scripts/bench_stage_lab.py drives it. */
int difusco_lab_gemm1(int variant, const float* e, const void* planes, float* out, int n_edges, float inv_c, int do_store,
                      int lds_pad, void* stream);
/* Re-read probe: one streaming pass (float4 loads, non-temporal or default policy) over buf[0 .. n_floats); scripts/
 * bench_reread_probe.py times a second pass over the same buffer against the first for several sizes. */
int difusco_lab_reread_pass(const float* buf, long long n_floats, int nontemporal, float* sink, void* stream);
/* the same translation unit compiled without packed fp32 arithmetic (target feature -packed-fp32-ops) */
int difusco_lab_gemm1_nopk(int variant, const float* e, const void* planes, float* out, int n_edges, float inv_c, int do_store,
                           int lds_pad, void* stream);
#endif

#ifdef __cplusplus
}
#endif
#endif /* DIFUSCO_HIP_H */
