/*
 * hydra_mp.h -- C ABI of libhydra_mp.so, the MI355X (gfx950) message-passing engine that replaces the
 * torch_geometric layer stack on Hydra-GNN's room-classification hot path.
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer (HBM) unless stated; sizes are element counts.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises.
 *   - return value: 0 = OK, otherwise an HMP_E_* code; hmp_last_error() gives the message
 *     (thread local).  No entry point falls back to a CPU path.
 *   - features are fp32 row-major with an explicit leading dimension (floats); graph indices are
 *     int32 in the plan, int64 `edge_index[2][E]` on input (the PyG contract: row 0 = source,
 *     row 1 = destination, aggregation at the destination).
 *
 * Each group cites the reference interface it replaces (paths relative to the reference repo;
 * "[PyG]" = torch_geometric 2.3.1 operator the reference calls, restated in SURVEY.md Appendix A).
 */
#ifndef HYDRA_MP_H
#define HYDRA_MP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: round 2 -- hmp_batch grew (plan_valid, d_node_ptr, n_graphs, max_graph_nodes, d_edge_ptr), hmp_train_args::d_step; sections 10-12
 * 3: round 3 -- hmp_comm_query; hmp_net_read_state reports the counter of the last step from the net's own state;
 *    hmp_conv_spec::agg_first; hmp_gemm_bf16_dx / hmp_gemm_bf16_dw
 * 4: hmp_net_spec::tail_act / tail_dropout, hmp_head_targets (hmp_sizeof 7), hmp_net_step2_fwd_bwd / hmp_net_step2_fused /
 *    hmp_net_count_correct2: the fused step of the two-headed task
 *    ABI-4-compatible additions (nothing above changed layout): hmp_linear_heads (hmp_sizeof 8), hmp_linear_head_targets
 *    (hmp_sizeof 9), hmp_net_set_linear_heads / hmp_net_step_heads_fwd_bwd / hmp_net_step_heads_fused /
 *    hmp_net_count_correct_heads: the fused step of two learned linear heads over one final state;
 *    hmp_count_correct_rows / hmp_net_count_correct_rooms: the device-side validation count of the room task;
 *    hmp_net_set_head_pools: the two-headed step / count with each head's CE on the mean over a pool edge type (LeafPool);
 *    hmp_gemm_desc (hmp_sizeof 10), hmp_gemm_grouped: unit-test entry of the grouped GEMM launchers;
 *    section 8: hmp_collate_rows / hmp_collate_item::row_bytes accept any positive row size (byte-wide bool / int8 masks of the
 *    two-headed task ride in the same launch); the one-launch collator holds 40 items (was 24) and carries 264 table words in the
 *    argument block (was 336).  No struct changed layout, no entry was added;
 *    hmp_collator_set_label_filter (room-masked labels in the collation launch), hmp_count_correct_rows_by_graph /
 *    hmp_net_count_correct_rooms_by_graph (per-graph validation counts): new entries, no struct changed layout;
 *    hmp_tail_desc (hmp_sizeof 14), hmp_linear_heads_desc (hmp_sizeof 15), hmp_head_tails / hmp_linear_heads_run: test and
 *    diagnostic entries of the readout tail and linear-head launchers: new entries, no struct changed layout;
 *    hmp_predict_rows, hmp_net_predict_rooms / hmp_net_predict2 / hmp_net_predict_heads (labels instead of counts, for every net
 *    kind), hmp_head_tails_predict / hmp_linear_heads_predict (their test entries): new entries, no struct changed layout;
 *    hmp_topk_rows, hmp_net_topk_rooms / hmp_net_topk2 / hmp_net_topk_heads (top-k labels with their softmax probabilities, for
 *    every net kind), hmp_head_tails_topk / hmp_linear_heads_topk (their test entries): new entries, no struct changed layout;
 *    section 14: hmp_frame_build / hmp_frame_sizes / hmp_frame_host_arrays / hmp_frame_pack / hmp_frame_destroy (host) and
 *    hmp_frame_expand (one launch): scene-graph arrays to model input.  New entries, no struct was added or changed layout;
 *    hmp_frame_build_homogeneous: the same frame laid out as the homogeneous Data (item kinds HMP_FK_EDGE_SEG / HMP_FK_CONST, output
 *    tensors from HMP_FT_HOMOG on).  A new entry; the six entries above, HMP_FRAME_ITEM_WORDS and every earlier number are unchanged;
 *    hmp_frame_batch_build / _items_needed / _sizes / _host_arrays / _pack / _destroy and hmp_frame_expand_batch: many frames per
 *    block and launch (output tensors from HMP_FT_BATCH on).  New entries; a single frame packs what it packed, nothing above changed;
 *    relative_pos = HMP_FRAME_RELPOS_HTREE (item kind HMP_FK_EATTR_HT, output tensors from HMP_FT_HTREL on): a new value of an argument
 *    that was refused before; no entry, struct or earlier number changed, every earlier mode packs what it packed;
 *    hmp_frame_build_flags (HMP_FRAME_NO_ROOM_EDGES: the reference's remove_room_edges_in_dsg in the host stage), item kinds
 *    HMP_SD_COMPACT / HMP_SD_ROWS_ZERO of hmp_store_derive's table and hmp_store_count_kept (the edge-type and clique ablations on a
 *    resident store): new entries and new kinds behind the old ones; hmp_collator_create accepts a null d_src for an item whose
 *    slot is empty in every graph (it was refused before);
 *    hmp_gat_attention / hmp_net_attention (per-edge attention coefficients and the top-k sources per row, from the softmax state
 *    of a forward): new entries, no struct was added or changed layout;
 *    hmp_saliency_seed / hmp_saliency_scores / hmp_saliency_topk / hmp_net_input_gradient / hmp_net_plan (gradient saliency: the gradient of a
 *    chosen class's logit or log-probability with respect to the input features, and its reductions): new entries, no struct was
 *    added or changed layout;
 *    hmp_plan_job (hmp_sizeof 16), hmp_plan_build_many: unit-test entry of the plan builder as the executor calls it (several edge
 *    types per call, need_tpos, clear_first, degf, graph offsets); hmp_plan_build is its one-job call.  A new entry and a new
 *    struct, nothing above changed layout;
 *    hmp_net_set_class_weights, hmp_masked_ce_weighted (class weights of the cross entropy for every step form and the standalone
 *    loss), hmp_label_counts / hmp_balanced_class_weights (the label histogram and balanced weights on the device),
 *    hmp_head_tails_weighted / hmp_linear_heads_run_weighted (their test entries): new entries, no struct was added or changed
 *    layout.  The normaliser of the loss and of Adam's gradient scale is now used as it is when > 0 (it was clamped at 1): the
 *    same bits for the integer-valued counts of unweighted steps;
 *    hmp_seg_mean_rows / hmp_seg_mean_rows_t / hmp_gemm_bf16_dx_gather (test entries of the aggregate-first convs' launchers and of
 *    the gather-add term of the input-gradient GEMM): new entries, no struct was added or changed layout;
 *    hmp_front_seg / hmp_front_prob / hmp_pack_seg (hmp_sizeof 17..19), hmp_front_run / hmp_pack_run: unit-test entries of the
 *    front launch's projection and pack roles and of the stand-alone pack.  New entries and new structs, nothing above changed
 *    layout;
 *    hmp_mc_acc_ld / hmp_mc_accumulate_rows / hmp_mc_finish, hmp_net_mc_rooms / hmp_net_mc2 / hmp_net_mc_heads (Monte-Carlo dropout
 *    uncertainty for every net kind: per-row accumulators of the stochastic samples' softmax, and their mean, standard deviation,
 *    entropy and mutual information), hmp_head_tails_mc / hmp_linear_heads_mc (their test entries): new entries, no struct was added
 *    or changed layout */
#define HMP_ABI_VERSION 4

#define HMP_OK 0
#define HMP_E_ARG 1      /* bad argument (shape / alignment / capacity) */
#define HMP_E_HIP 2      /* a HIP runtime call failed */
#define HMP_E_STATE 3    /* call order violated (e.g. backward without forward) */
#define HMP_E_NODEVICE 4 /* no gfx950 device visible */
#define HMP_E_UNSUPPORTED 5 /* an optional system library (RCCL) is not present on this machine */

#define HMP_MAX_NODE_TYPES 8
#define HMP_MAX_EDGE_TYPES 16
#define HMP_MAX_LAYERS 8
#define HMP_MAX_CONVS 16 /* per layer */

/* ---------------------------------------------------------------------------------------------
 * 0. library
 * ------------------------------------------------------------------------------------------- */
int hmp_abi_version(void);
const char* hmp_last_error(void);
/* sizeof() of the ABI structs: 0 hmp_plan, 1 hmp_gat_args, 2 hmp_conv_spec, 3 hmp_layer_spec, 4 hmp_net_spec,
 * 5 hmp_batch, 6 hmp_train_args, 7 hmp_head_targets, 8 hmp_linear_heads, 9 hmp_linear_head_targets, 10 hmp_gemm_desc,
 * 11 hmp_epoch_ctl, 12 hmp_epoch_row, 13 hmp_epoch_seg, 14 hmp_tail_desc, 15 hmp_linear_heads_desc, 16 hmp_plan_job, 17 hmp_front_seg,
 * 18 hmp_front_prob, 19 hmp_pack_seg (lets a foreign-language binding verify its struct mirror) */
size_t hmp_sizeof(int which);
/* number of visible devices whose gcnArchName starts with "gfx950"; never raises */
int hmp_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * 1. graph plan: CSR by destination + CSC (transpose) by source, stable in edge order.
 *    Replaces the per-call `index_select` / `scatter` index handling of
 *    [PyG] MessagePassing.propagate (called from models/utils.py:14,49 via HeteroConv).
 *    Bit-exact contract: col[rowptr[i] .. rowptr[i+1]) are the sources of the edges whose
 *    destination is i, in ascending original edge id (== torch.sort(dst, stable=True)).
 * ------------------------------------------------------------------------------------------- */
typedef struct hmp_plan {
  int32_t n_src, n_dst;
  int64_t n_edges;
  int32_t* d_rowptr;   /* [n_dst+1]  CSR by destination */
  int32_t* d_col;      /* [E] source node of the k-th CSR entry */
  int32_t* d_eid;      /* [E] original edge id of the k-th CSR entry */
  int32_t* d_t_rowptr; /* [n_src+1]  CSC (edges grouped by source) */
  int32_t* d_t_col;    /* [E] destination node of the k-th CSC entry */
  int32_t* d_t_pos;    /* [E] CSR position of the k-th CSC entry (eid = d_eid[d_t_pos[k]]) */
} hmp_plan;

/* bytes of scratch hmp_plan_build needs for E edges between n_src and n_dst nodes */
size_t hmp_plan_scratch_bytes(int64_t n_edges, int32_t n_src, int32_t n_dst);
/* d_edge_index: int64 [2][E] (row stride = E).  Out-of-range endpoints set bit 0 of *d_status
 * (int32, device, may be NULL) and the edge is dropped from the lists: rowptr[n_dst] = t_rowptr[n_src] = the number of edges kept,
 * and the entries of col / eid / t_col / t_pos at and after that count are unspecified. */
int hmp_plan_build(const int64_t* d_edge_index, hmp_plan plan, void* d_scratch, int32_t* d_status, void* stream);

/* Unit-test entry of the builder as the network executor calls it (ABI-4-compatible addition, hmp_sizeof 16): n edge types in one
 * call, each job copied as it stands; hmp_plan_build is the call with n = 1, need_tpos = 1, clear_first = 1.
 *   d_degf       optional [n_dst] float: 1 / max(in-degree, 1)
 *   d_dst_ptr, d_src_ptr, d_edge_ptr   optional, all three or none: int64 [n_graphs + 1] row offsets of the destination / source
 *                node type and edge offsets of a batch whose edges are listed graph by graph (what hmp_batch::d_node_ptr and
 *                d_edge_ptr vouch for).  Only the single-launch build reads them; offsets that do not describe the list (an edge
 *                with an in-range endpoint outside its graph's rows, edges in a graph without rows for them, last offsets that are
 *                not the row / edge counts) set status bit 2 (value 4) and leave the arrays unspecified, though every access of
 *                the build stays inside the arrays.  An edge with an endpoint out of range breaks no vouching: it is dropped as
 *                above, and the arrays are those of the same call without offsets.
 *   d_scratch    hmp_plan_scratch_bytes(E, n_src, n_dst) bytes per job.  Its first 2 * a(n_dst) + 2 * a(n_src) ints (a rounds up to
 *                64) are counters, zero on entry and left zero on exit; the 64 ints behind them are zero before the first build
 *                and hold what builds leave there afterwards.  clear_first != 0 zeroes all of these before the build.
 *   need_tpos    0: d_t_pos is left untouched.
 * Refused (HMP_E_ARG): n outside 0..HMP_MAX_EDGE_TYPES, null jobs with n > 0, a null scratch, a null output array with E > 0, one
 * or two of the three offset arrays without the rest. */
typedef struct hmp_plan_job {
  const int64_t* d_edge_index;   /* [2][E] */
  hmp_plan plan;                 /* sizes + output arrays */
  float* d_degf;                 /* optional [n_dst] */
  const int64_t *d_dst_ptr, *d_src_ptr, *d_edge_ptr;  /* optional, all three or none: [n_graphs + 1] */
  int32_t n_graphs;
  void* d_scratch;               /* hmp_plan_scratch_bytes(E, n_src, n_dst) */
} hmp_plan_job;
int hmp_plan_build_many(const hmp_plan_job* jobs, int32_t n, int32_t need_tpos, int32_t clear_first, int32_t* d_status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 2. K1 -- segment mean over CSR rows (SAGE neighbour mean, LeafPool).
 *    Replaces [PyG] SAGEConv.propagate(aggr="mean") = index_select + scatter_add x2 + clamp + div
 *     and LeafPool (models/heterogeneous_neural_tree_network.py:18-31).
 *    out[i, 0:F] = (1/max(deg_i,1)) * sum_{k in row i} x[col[k], 0:F]     (zeros for empty rows)
 *    bwd: g_x[j, 0:F] = sum_{k in CSC row j} g_out[t_col[k], 0:F] / max(deg(t_col[k]),1)
 * ------------------------------------------------------------------------------------------- */
int hmp_segment_mean_fwd(const float* d_x, int32_t ldx, int32_t F, hmp_plan plan, float* d_out, int32_t ldo, void* stream);
int hmp_segment_mean_bwd(const float* d_gout, int32_t ldg, int32_t F, hmp_plan plan, float* d_gx, int32_t ldgx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 3. K2 -- dense fp32 projection on the matrix cores (v_mfma_f32_32x32x2_f32, exact fp32 FMA chain).
 *    Replaces F.linear inside [PyG] SAGEConv.lin_l / lin_r and GATConv.lin_src / lin_dst.
 *    C[M,N] = op(A)[M,K] * op(B)[K,N];  trans_a: A stored [K][M];  trans_b: B stored [N][K]
 *    (trans_b = 1 is nn.Linear's weight layout).
 * ------------------------------------------------------------------------------------------- */
/* same problem on the bf16 matrix pipe (operands rounded to bf16, fp32 accumulate); unit-test entry of gemm_bf16.hip */
int hmp_gemm_bf16(const float* d_a, int32_t lda, int32_t trans_a, const float* d_b, int32_t ldb, int32_t trans_b, float* d_c,
                  int32_t ldc, int32_t M, int32_t N, int32_t K, void* stream);
/* C[M, N] = A[M, K] * W[N, K]^T with A STORED as bf16 (the hidden activations of bf16 compute mode, lda in elements, rows 8-byte
 * aligned), W fp32 (rounded to bf16 on the way in), fp32 accumulation, C written as bf16 (c_bf16 != 0, ldc in elements) or fp32.
 * Tall problems (M >= 32768, K <= 256, 16-byte aligned rows) run on the weight-stationary kernel (csrc/gemm_bf16.hip); this is
 * the projection of the reference's SAGEConv.lin_l / lin_r at 10^6 nodes ([PyG] sage_conv.py: `self.lin_l(out)`). */
int hmp_gemm_bf16_a16(const uint16_t* d_a, int32_t lda, const float* d_w, int32_t ldw, void* d_c, int32_t ldc, int32_t c_bf16,
                      int32_t M, int32_t N, int32_t K, void* stream);
int hmp_gemm_f32(const float* d_a, int32_t lda, int32_t trans_a, const float* d_b, int32_t ldb, int32_t trans_b,
                 float* d_c, int32_t ldc, int32_t M, int32_t N, int32_t K, void* stream);
/* The two backward products of that projection in the 10^6-node regime (csrc/gemm_bf16_bwd.hip; unit-test entries of what the
 * executor calls; reference: autograd of F.linear inside [PyG] SAGEConv, models/utils.py:14).  dZ is bf16 [M][lddz]; its columns
 * from `split` on may live in a second bf16 matrix d_dz2 [M][lddz2] (the root block of dZ is the output gradient itself; split = 0:
 * one matrix; otherwise a multiple of 256).
 *   dx: G[M, N] = mask . (dZ[M, K] * W[K, N]), W fp32 [K][ldw] rounded to bf16, fp32 accumulation, G written as bf16; mask from the
 *       stored activations d_h (bf16 [M][ldh], NULL = none): act' of HMP_ACT_*, and with drop_on an element stored as -0 is a dropped
 *       one (factor 0), kept ones are scaled by drop_scale.  Tall problems (M >= 32768, K in {256, 512, 768}, N % 128 == 0) run on
 *       the weight-stationary kernel.
 *   dw: slabs of dW[Mw, F + 1] = dZ[nodes, Mw]^T * [H | 1][nodes, F + 1]: slab z (fp32 [Mw][ldc] at d_slabs + z * slab_stride) holds
 *       the sum over one node range, *n_slabs of them are written (<= max_slabs); H is bf16 or fp32 [nodes][ldh].  Mw % 256 == 0,
 *       F == 256 and nodes >= 65536 run on the output-stationary kernel. */
int hmp_gemm_bf16_dx(const uint16_t* d_dz, int32_t lddz, const uint16_t* d_dz2, int32_t lddz2, int32_t split, const float* d_w,
                     int32_t ldw, const uint16_t* d_h, int32_t ldh, int32_t act, int32_t drop_on, float drop_scale, uint16_t* d_g,
                     int32_t ldg, int32_t M, int32_t N, int32_t K, void* stream);
int hmp_gemm_bf16_dw(const uint16_t* d_dz, int32_t lddz, const uint16_t* d_dz2, int32_t lddz2, int32_t split, const void* d_h,
                     int32_t ldh, int32_t h_bf16, float* d_slabs, int32_t ldc, int64_t slab_stride, int32_t max_slabs,
                     int32_t* n_slabs, int32_t Mw, int32_t F, int32_t nodes, void* stream);
/* Unit-test entries of the aggregate-first SAGE convs (csrc/aggfirst.hip; ABI-4-compatible additions): the launchers as the
 * executor calls them, on raw device int32 CSR arrays instead of an hmp_plan.  Reference: [PyG] SAGEConv evaluated in its own order,
 * out = lin_l(mean_j x_j), and autograd of that mean.
 *   hmp_seg_mean_rows    M[i, 0:F] = (1 / max(deg_i, 1)) * sum_{k in [rowptr[i], rowptr[i+1])} X[col[k], 0:F], fp32 [n_rows][ldm]
 *                        written as whole 4-vectors (columns up to align4(F); ldm % 4 == 0, 16-byte aligned base: refused otherwise).
 *                        X is fp32 or bf16 (x_bf16) [.][ldx]; rows that are not whole aligned 4-vectors (ldx % 4 != 0, ldx <
 *                        align4(F), or an unaligned base) are read element by element.
 *   hmp_seg_mean_rows_t  G[j, 0:F] = mask(H[j, :]) . sum_{k in [t_rowptr[j], t_rowptr[j+1])} dM[t_col[k], 0:F] * degf[t_col[k]]: the
 *                        transpose of that mean (degf[i] = 1 / max(deg_i, 1)) times the activation / dropout factor of the source
 *                        rows.  dM fp32 [.][lddm]; H fp32 or bf16 (h_bf16) [n_rows][ldh], NULL: no mask; with drop_on an element of H
 *                        stored as -0.0 is a dropped one (factor 0); a kept one has the factor dscale (HMP_ACT_NONE), h > 0 ? dscale : 0
 *                        (RELU) or h > 0 ? dscale : h + dscale (ELU: the stored h is dscale * elu(z)).  G fp32 or bf16 (g_bf16)
 *                        [n_rows][ldg].  Everything moves as whole 4-vectors: F, lddm, ldh, ldg multiples of 4 (refused otherwise) --
 *                        except fp32 G at a pitch that is no multiple of 4 (the caller's input-gradient rows: 306 floats at pitch
 *                        306), which takes any F <= ldg and stores exactly F elements per row one by one.
 *   hmp_gemm_bf16_dx_gather   hmp_gemm_bf16_dx with that transposed sum over d_g_rows (fp32 [.][g_ld], g_ld >= N) added to the product
 *                        BEFORE the mask: G = mask . (dZ W + sum_k g_rows[t_col[k], 0:N] * degf[t_col[k]]).  It runs the executor's own
 *                        decision: the term rides in the epilogue of the weight-stationary kernel where that kernel takes the
 *                        problem (g_ld % 4 == 0, 16-byte aligned g_rows), else it is materialised into d_scratch (fp32, at least
 *                        M * g_ld floats) by hmp_seg_mean_rows_t's launcher and added by the tiled kernel (HMP_GEMM_DX=0 forces this). */
int hmp_seg_mean_rows(const void* d_x, int32_t ldx, int32_t x_bf16, int32_t F, const int32_t* d_rowptr, const int32_t* d_col,
                      int32_t n_rows, float* d_m, int32_t ldm, void* stream);
int hmp_seg_mean_rows_t(const float* d_dm, int32_t lddm, int32_t F, const int32_t* d_t_rowptr, const int32_t* d_t_col,
                        const float* d_degf, int32_t n_rows, const void* d_h, int32_t ldh, int32_t h_bf16, int32_t act, int32_t drop_on,
                        float dscale, void* d_g, int32_t ldg, int32_t g_bf16, void* stream);
int hmp_gemm_bf16_dx_gather(const uint16_t* d_dz, int32_t lddz, const uint16_t* d_dz2, int32_t lddz2, int32_t split, const float* d_w,
                            int32_t ldw, const uint16_t* d_h, int32_t ldh, int32_t act, int32_t drop_on, float drop_scale,
                            uint16_t* d_g, int32_t ldg, int32_t M, int32_t N, int32_t K, const int32_t* d_t_rowptr,
                            const int32_t* d_t_col, const float* d_degf, const float* d_g_rows, int32_t g_ld, float* d_scratch,
                            void* stream);
/* Unit-test entry of the grouped launchers as the executor calls them: n <= 8 problems in one launch, each copied as it stands
 * into the launcher's problem table (csrc/gemm.hip); the launcher alone chooses the kernels.  One problem: C[M, N] = op(A) *
 * op([B | 1]) (+ Cadd) (. act'(H) / (1 - drop_p) under epi = 1), fp32 unless a *_bf16 flag says otherwise (route 1 only, ld* then
 * count elements).  B has n_real columns in memory, N = n_real + 1 with the virtual ones column (aug_ones), N = n_real without.
 * Split-K (want_split): slab z of C lies at C + z * slab_stride, the caller sums the slabs.  epi = 1 (EPI_ACTMASK): the result is
 * multiplied by act' (HMP_ACT_*) of the stored activations H [M][ldh]; drop_p > 0: an element of H stored as -0.0 is a dropped
 * one (factor 0), kept ones are scaled by 1 / (1 - drop_p).  Cadd: fp32 [M][ldadd] added to the product before the mask. */
typedef struct hmp_gemm_desc {
  const void *A, *B;
  void* C;
  const void* H;
  const float* Cadd;
  int32_t M, N, K, lda, ldb, ldc, ldh, ldadd, trans_a, trans_b;
  int32_t n_real, aug_ones;
  int64_t slab_stride;
  int32_t epi, act;
  float drop_p;
  int32_t a_bf16, b_bf16, c_bf16, h_bf16;
} hmp_gemm_desc;
/* route 0: the fp32 launcher (tiled, tall TN and x3 kernels), 1: the bf16 launcher (tiled 128 / 256, dx, dw, weight-stationary),
 * 2: the register-direct TN kernel (trans_a = 1, trans_b = 0, fp32, no epilogue, no Cadd).  ksplit_out[i] (may be NULL): the
 * slabs written for problem i; route 2: all 0 when the kernel declined (a problem would need more than max_slabs) and nothing ran */
int hmp_gemm_grouped(const hmp_gemm_desc* d, int32_t n, int32_t route, int32_t want_split, int32_t max_slabs, int32_t* ksplit_out,
                     void* stream);

/* Unit-test entries of the small-batch step's front launch (csrc/front.hip) and of the parameter pack (ABI-4-compatible
 * additions, hmp_sizeof 17..19): the descriptors are copied as they stand into the structures the executor fills, the block maps
 * are the executor's own (pack_seg_blocks / pack_block_map), the plan role is left out (hmp_plan_build_many has it).
 *
 * A projection is C[M, N] = A[M, K] * B^T with the stacked operand B read from the flat parameter buffer: row c of B, for
 * col0 <= c < col0 + rows of a segment, is the sum over q < nsrc of the ld floats at d_params + off[q] + (c - col0) * ld; every
 * other row below N is zero.  The launcher wants 4 <= K <= 384, K, lda, ld and every off even, A 8-byte and d_params 16-byte
 * aligned, 1..6 segments of 1..6 sources.  The entry itself checks what the executor guarantees by construction: ld == K, lda >=
 * K, ldc >= N, segments sorted by col0 without overlap, and every parameter block inside [0, n_params). */
#define HMP_FRONT_MAX_PROB 4
#define HMP_FRONT_MAX_SEG 6
#define HMP_FRONT_MAX_SRC 6
typedef struct hmp_front_seg {
  int32_t col0, rows, nsrc, ld;
  uint32_t off[HMP_FRONT_MAX_SRC];
} hmp_front_seg;
typedef struct hmp_front_prob {
  const float* A;
  float* C;
  int32_t lda, ldc, M, N, K, n_seg;
  hmp_front_seg seg[HMP_FRONT_MAX_SEG];
} hmp_front_prob;
/* One segment of a pack table; all offsets count floats.  Rows [0, rows_pad) x columns [0, ld_dst) at d_packed + dst are all
 * written (what the kind does not define is zero):
 *   HMP_PACK_SUM       row r = sum over q < nsrc, left to right, of the cols floats at d_params + src[q] + r * ld_src   (r < rows)
 *   HMP_PACK_HEADS     row h * Cp + c = the cols floats at d_params + src[0] + (h * C + c) * ld_src                   (h < H, c < C)
 *   HMP_PACK_ATTDOT    row h = sum over c < C of d_params[att + h * C + c] * (row h * C + c of src[0])                 (h < H)
 *   HMP_PACK_ATTDOT_T  element (d, h) = sum over c < C of d_params[att + h * C + c] * d_params[src[0] + (h * C + c) * ld_src + d]
 *                      (d < rows, h < H)
 * ld_dst_t > 0 (HMP_PACK_SUM): element (r, c) of the whole [rows_pad][ld_dst] block is stored a second time at d_packed + dst_t +
 * c * ld_dst_t + col(col_t + r), where col(16 b + 4 u + q) = 16 b + 4 q + u, and col(col_t + rows_pad + p) of the same ld_dst rows
 * is set to zero for p < pad_t. */
#define HMP_PACK_SUM 0
#define HMP_PACK_HEADS 1
#define HMP_PACK_ATTDOT 2
#define HMP_PACK_ATTDOT_T 3
typedef struct hmp_pack_seg {
  int64_t dst;
  int32_t rows, rows_pad, cols, ld_dst, ld_src, nsrc, kind, H, C, Cp;
  int64_t att;
  int64_t src[6];
  int64_t dst_t;
  int32_t ld_dst_t, col_t, pad_t;
} hmp_pack_seg;
/* One front launch: n_prob <= 4 projections (may be 0) and, when n_segs > 0, the pack role over segs (16 items per block through
 * the executor's static map).  d_step (may be NULL): device int32 that the pack role raises by one, leaving the new value in
 * d_step_mirror too (may be NULL).  n_params / n_packed: floats in the two buffers; a descriptor that reaches outside is refused.
 * The table upload is synchronous and the call returns after the launch has finished. */
int hmp_front_run(const hmp_front_prob* probs, int32_t n_prob, const float* d_params, int64_t n_params, const hmp_pack_seg* segs,
                  int32_t n_segs, float* d_packed, int64_t n_packed, int32_t* d_step, int32_t* d_step_mirror, void* stream);
/* The pack alone: route 0 through pack_launch (4 items per block, block -> segment scan), route 1 through the front launch's pack
 * role (hmp_front_run without projections). */
int hmp_pack_run(const hmp_pack_seg* segs, int32_t n_segs, int32_t route, const float* d_params, int64_t n_params, float* d_packed,
                 int64_t n_packed, int32_t* d_step, int32_t* d_step_mirror, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 4. K3 -- GAT edge softmax + weighted aggregation, one row group of lanes per destination row.
 *    Replaces [PyG] GATConv.edge_update + softmax + message/aggregate for ONE conv.
 *    Inputs: h_src [n_src, H*Cp] projected source rows, head h at columns h*Cp (Cp = channels rounded up to 4);
 *    a_src [n_src, >=H] (ld lda_src), a_dst [n_dst, >=H] (ld lda_dst): attention logits halves;
 *    optional edge term <edge_attr[e, 0:edge_dim], v_edge[0:edge_dim, h]> with v_edge [edge_dim][8]
 *    (edge_attr in ORIGINAL edge order; NULL / edge_dim 0 = none).
 *    e_k = leaky_relu(a_src[col_k,h] + a_dst[i,h] + edge term, 0.2); alpha = softmax over the row
 *    (max-subtracted, denominator + 1e-16); out[i, h*C + c] = sum_k dropout(alpha_k,h) * h_src[col_k, h*Cp + c].
 *    With self_loops != 0 entries with col == row are skipped and one loop i->i (edge term 0) is appended per
 *    row i < min(n_src, n_dst).  The softmax is computed online; the per-row running max and denominator are
 *    written to smax / sden [n_dst, 8] for the backward (alpha is recomputed there, never stored in forward).
 *    These two unit entry points upload a small descriptor and SYNCHRONISE the stream (test / integration use;
 *    the network executor below drives the same kernels without synchronising).
 * ------------------------------------------------------------------------------------------- */
typedef struct hmp_gat_args {
  int32_t heads, channels;   /* H <= 8, C <= 256; or H <= 4, C <= 512 */
  int32_t self_loops;
  int32_t edge_dim;          /* 0..4 */
  float dropout_p;           /* attention dropout; 0 = off */
  uint64_t seed;             /* dropout RNG (counter hash, csrc/common.h): element (pos, h) of an [E + n_loop, 8] tensor, */
  uint32_t rng_stream, rng_step; /* pos = CSR position of the edge, loops at E + i (see hmp_dropout_mask) */
} hmp_gat_args;

int hmp_gat_fwd(const float* d_h_src, int32_t ldh, const float* d_a_src, int32_t lda_src, const float* d_a_dst,
                int32_t lda_dst, const float* d_edge_attr, const float* d_v_edge, hmp_plan plan, hmp_gat_args args,
                float* d_smax, float* d_sden, float* d_out, int32_t ldo, void* stream);
/* d_gout [n_dst, H*C].  Outputs: g_h_src [n_src, H*Cp] (ld ldgh), g_a_src [n_src, >=H] (ld ldgas), g_a_dst
 * [n_dst, >=H] (ld ldgad); d_alpha_drop / d_dlogit [E + n_loop, 8] receive alpha after dropout and d loss / d raw
 * logit per CSR position; d_dlogit_orig [E, 8] (may be NULL) the same in original edge order, so that
 * d v_edge = edge_attr^T * dlogit_orig. */
int hmp_gat_bwd(const float* d_gout, int32_t ldg, const float* d_h_src, int32_t ldh, const float* d_a_src, int32_t lda_src,
                const float* d_a_dst, int32_t lda_dst, const float* d_edge_attr, const float* d_v_edge, hmp_plan plan,
                hmp_gat_args args, const float* d_smax, const float* d_sden, float* d_alpha_drop, float* d_dlogit,
                float* d_dlogit_orig, float* d_g_h_src, int32_t ldgh, float* d_g_a_src, int32_t ldgas, float* d_g_a_dst,
                int32_t ldgad, void* stream);
/* Attention export: what [PyG] GATConv.forward(return_attention_weights=True) hands out, from the softmax state d_smax / d_sden
 * [n_dst, 8] (16-byte aligned) a preceding hmp_gat_fwd with the same inputs left.  One launch; synchronises like the two entries
 * above.  args.dropout_p plays no part: the coefficients are the ones before dropout.  (ABI-4-compatible addition.)
 *   d_alpha [E + n_loop, H] float, exactly H columns: row e < E belongs to column e of the edge_index the plan was built from, row
 *   E + i to the appended loop i -> i (n_loop = self_loops ? min(n_src, n_dst) : 0).  Value: expf(e_k - smax[i, h]) / sden[i, h],
 *   the expression the backward differentiates.  An input edge i -> i the conv removes (self_loops != 0) holds 0, and so does an
 *   edge the plan dropped (endpoint out of range, status bit 0) when d_edge_index -- that same int64 [2][E] list -- is given; with
 *   d_edge_index NULL the caller vouches that nothing was dropped (such rows would be left unwritten).
 *   d_top_src [n_dst, k] int64 / d_top_w [n_dst, k] float, 1 <= k <= 8: the k entries of the row with the largest head-mean
 *   coefficient (a_0 + a_1 + ... + a_{H-1}) / H, computed in float32 with the heads added in ascending order; descending, equal means
 *   by ascending CSR position (the plan is stable: ascending original edge id, the appended loop last).  d_top_src holds the source
 *   node (the row itself for the loop); removed and dropped entries are no candidates; columns past the row's live entries hold
 *   -1 / 0.  Every element of both arrays is written.
 *   Any of the three outputs may be NULL (skipped); what one output holds does not depend on which others were requested. */
int hmp_gat_attention(const float* d_a_src, int32_t lda_src, const float* d_a_dst, int32_t lda_dst, const float* d_edge_attr,
                      const float* d_v_edge, const int64_t* d_edge_index, hmp_plan plan, hmp_gat_args args, const float* d_smax,
                      const float* d_sden, float* d_alpha, int32_t k, int64_t* d_top_src, float* d_top_w, void* stream);

/* Gradient saliency, the three stand-alone launches (each is one launch on `stream`, nothing synchronises; ABI-4-compatible
 * additions).  A ROW SELECTION (sel_mode, d_mask, ordinal, d_graph_ptr, n_graphs) names the rows a launch serves:
 *   HMP_SEL_ALL      every row;
 *   HMP_SEL_MASK     the rows whose byte of d_mask [n_rows] is not 0;
 *   HMP_SEL_ORDINAL  row d_graph_ptr[g] + ordinal of every graph g with more than `ordinal` rows; d_graph_ptr is int64 [n_graphs + 1],
 *                    ascending from 0 ([PyG] Batch.ptr of the rows' node type), empty graphs allowed.
 * Arguments a mode does not use are ignored. */
#define HMP_SEL_ALL 0
#define HMP_SEL_MASK 1
#define HMP_SEL_ORDINAL 2
#define HMP_WRT_LOGIT 0
#define HMP_WRT_LOGPROB 1
/* The output gradient that selects what is explained.  Class c of a selected row is d_target[row] where d_target is given and the
 * value lies in [0, n_classes), else the row's first-maximum argmax (bit-equal to hmp_predict_rows).  The row of d_gout is
 * onehot(c) (HMP_WRT_LOGIT: the gradient of logit c) or onehot(c) - softmax(z) (HMP_WRT_LOGPROB: of log softmax(z)[c]; the softmax
 * arithmetic of hmp_topk_rows).  EVERY element of d_gout [n_rows, ld_g] is written: columns at or past n_classes and rows outside
 * the selection hold 0, so the buffer needs no memset.  ld >= n_classes, ld_g >= n_classes; no alignment is asked for. */
int hmp_saliency_seed(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const int64_t* d_target, int32_t sel_mode,
                      const uint8_t* d_mask, int32_t ordinal, const int64_t* d_graph_ptr, int32_t n_graphs, int32_t wrt,
                      float* d_gout, int32_t ld_g, void* stream);
/* An input gradient d_g [n_rows, ld_g] reduced against its input d_x [n_rows, ld_x] over the n_features real columns, per row:
 *   d_gxi [n_rows]              sum_f g * x          (signed gradient x input)
 *   d_gnorm [n_rows]            sqrt(sum_f g^2)
 *   d_groups [n_rows, n_groups] sum of g * x over the columns [lo[i], hi[i]) clipped to [0, n_features); lo >= hi: 0
 * with 0 <= n_groups <= 4 and lo / hi HOST arrays.  Any output may be NULL; what one output holds does not depend on which others
 * were requested.  One wavefront per row, fp32 sums in a fixed order: a rerun gives the same bits.  No alignment is asked for. */
int hmp_saliency_scores(const float* d_g, int32_t ld_g, const float* d_x, int32_t ld_x, int32_t n_rows, int32_t n_features,
                        int32_t n_groups, const int32_t* lo, const int32_t* hi, float* d_gxi, float* d_gnorm, float* d_groups,
                        void* stream);
/* For every selected destination row of `plan`, the k sources (1 <= k <= 8) with the largest |d_score[source]|, descending, equal
 * magnitudes by ascending source index; a source reached by several edges is listed once.  d_top_src [n_dst, k] int64 and
 * d_top_score [n_dst, k] float (the SIGNED score); columns past a row's sources hold -1 / 0; either may be NULL.  Rows outside the
 * selection are left untouched, so repeated HMP_SEL_ORDINAL launches fill one output.  d_score has plan.n_src entries. */
int hmp_saliency_topk(hmp_plan plan, const float* d_score, int32_t k, int32_t sel_mode, const uint8_t* d_mask, int32_t ordinal,
                      const int64_t* d_graph_ptr, int32_t n_graphs, int64_t* d_top_src, float* d_top_score, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 5. loss + optimiser
 *    masked cross entropy: models/utils.py:143-148 with mask = (label != ignored_label)
 *    (base_training_job.py:213-214).  Writes d_out2 = {sum of -log p[label] over valid rows, number of
 *    valid rows}; d_grad [n, ldg] = (softmax - onehot) for valid rows, 0 otherwise, i.e. the gradient
 *    of the SUM loss -- callers scale by 1/count (so that N-GPU averaging is count-weighted).
 *    Adam: torch.optim.Adam(lr, weight_decay) with coupled L2 (base_training_job.py:181-185):
 *    g = grad*grad_scale + wd*p; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;
 *    p -= (lr/(1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps).
 * ------------------------------------------------------------------------------------------- */
int hmp_masked_ce(const float* d_logits, int32_t ldl, int32_t n_rows, int32_t n_classes, const int64_t* d_labels,
                  int64_t ignored_label, float* d_grad, int32_t ldg, float* d_out2, void* stream);
/* hmp_masked_ce with class weights, torch.nn.functional.cross_entropy(weight = w): d_w device float [n_classes] (NULL: hmp_masked_ce
 * bit for bit).  d_out2 = {sum of w[label] * -log p[label], sum of w[label]} over the valid rows and d_grad holds w[label] *
 * (softmax - onehot), so loss_sum / weight_sum is torch's weighted mean.  A row whose label has weight 0 does not count, exactly as
 * an ignored one; w is indexed by labels inside [0, n_classes) only.  The sum of weights is the normaliser of every consumer
 * (hmp_adam_flat's d_count, the fused steps): it is used as it is when > 0 -- a sum below 1 included -- and replaced by 1 when 0.
 * (ABI-4-compatible addition, like the class-weight entries below.) */
int hmp_masked_ce_weighted(const float* d_logits, int32_t ldl, int32_t n_rows, int32_t n_classes, const int64_t* d_labels,
                           int64_t ignored_label, const float* d_w, float* d_grad, int32_t ldg, float* d_out2, void* stream);
/* Label histogram: d_counts (device int64 [n_classes + 1]) ACCUMULATES, over the rows r with (d_mask == NULL || d_mask[r]) &&
 * d_labels[r] != ignored_label, the number of rows of each label in [0, n_classes) and, in slot n_classes, the rows whose label
 * lies outside that range.  One launch; n_rows == 0 launches nothing; nothing synchronises. */
int hmp_label_counts(const int64_t* d_labels, int64_t n_rows, const uint8_t* d_mask, int64_t ignored_label, int32_t n_classes,
                     int64_t* d_counts, void* stream);
/* Balanced class weights from such a histogram (scikit-learn's class_weight = "balanced" over the classes present): with
 * K = #{c : n_c > 0} and N = sum_c n_c over d_counts[0 .. n_classes), d_w[c] = (float)((double)N / ((double)K * n_c)) for n_c > 0 and
 * 0 for an absent class (device float [n_classes]).  One launch behind hmp_label_counts on the same stream: no host read between. */
int hmp_balanced_class_weights(const int64_t* d_counts, int32_t n_classes, float* d_w, void* stream);
/* out[r] = argmax_c x[r, c] (first maximum): the `.argmax(dim=1)` of the inference loop
 * (bin/room_classification_server:286) on the executor's output, so only the labels cross PCIe */
int hmp_argmax_rows(const float* d_x, int32_t ldx, int32_t n_rows, int32_t n_cols, int64_t* d_out, void* stream);
/* validation count of the room task: the per-batch arithmetic of BaseTrainingJob.test (base_training_job.py:269-313) without a
 * sync or a D2H.  pred[r] = first-maximum argmax of d_logits[r, 0:n_classes) (hmp_argmax_rows's rule); row r counts iff
 * (d_members == NULL || d_members[r]) && d_labels[r] != ignored_label (d_members: one byte per row, a torch bool tensor).
 * ACCUMULATES {correct, total} into d_counts (device int64[2]) and, if d_confusion != NULL, confusion[label][pred] += 1 into the
 * device int64 [n_classes][n_classes] matrix.  A counted label outside [0, n_classes) adds to total only (pred.eq(label) is
 * false) and never to the matrix.  One launch; n_rows == 0 launches nothing; nothing synchronises. */
int hmp_count_correct_rows(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const int64_t* d_labels,
                           const uint8_t* d_members, int64_t ignored_label, int64_t* d_counts, int64_t* d_confusion, void* stream);
/* the same count per graph (BaseTrainingJob.test_individual_graph, base_training_job.py:315-339, for a whole batch): the rows of
 * graph g are [d_graph_ptr[g], d_graph_ptr[g + 1]) (device int64 [n_graphs + 1], non-decreasing, d_graph_ptr[n_graphs] == n_rows:
 * [PyG] Batch.ptr of the rows' node type); a row counts under hmp_count_correct_rows's rule and ACCUMULATES into
 * d_counts[g] = {correct, total} (device int64 [n_graphs][2]).  A graph without counted rows (empty, or every label ignored)
 * receives nothing.  No confusion matrix.  One launch; n_rows == 0 launches nothing; nothing synchronises.  (ABI-4-compatible
 * addition, like the two entries marked so below.) */
int hmp_count_correct_rows_by_graph(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const int64_t* d_labels,
                                    const uint8_t* d_members, int64_t ignored_label, const int64_t* d_graph_ptr, int32_t n_graphs,
                                    int64_t* d_counts, void* stream);
/* the prediction hmp_count_correct_rows compares, written out: d_pred[r] (device int64 [n_rows]) = first-maximum argmax of
 * d_logits[r, 0:n_classes), or -1 where d_members[r] == 0 (d_members NULL: every row).  Every row in [0, n_rows) is written.  One
 * launch; n_rows == 0 launches nothing; nothing synchronises.  (ABI-4-compatible addition.) */
int hmp_predict_rows(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const uint8_t* d_members, int64_t* d_pred,
                     void* stream);
/* Top-k labels with their softmax probabilities: for a row's scores s = d_logits[r, 0:n_classes) and 1 <= k <= 8,
 * d_labels[r, j] (device int64 [n_rows][k], row-major) = the class with the j-th largest score -- scores descending, equal scores
 * (+0.0 == -0.0) by ascending class, so column 0 is hmp_predict_rows' label bit for bit -- and d_probs[r, j] (device float
 * [n_rows][k]) = expf(s[c] - m) / sum_c' expf(s[c'] - m) with c = d_labels[r, j], m the row maximum; m and the sum accumulate in
 * the association of the fused cross entropy (per lane of the row's 16 in ascending column order, then an xor butterfly), whatever
 * the pitch.  Columns j >= n_classes hold -1 / 0, and so does every column of a row with d_members[r] == 0 (d_members NULL: every
 * row).  Every element of rows [0, n_rows) is written exactly once, nothing behind them; the outputs need no initialisation.
 * Either output may be NULL (skipped), not both.  NaN scores are unspecified.  One launch; n_rows == 0 launches nothing; nothing
 * synchronises.  (ABI-4-compatible addition.) */
int hmp_topk_rows(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const uint8_t* d_members, int32_t k,
                  int64_t* d_labels, float* d_probs, void* stream);
/* Monte-Carlo dropout uncertainty: T stochastic samples of a row's scores are reduced to the mean predictive distribution, its
 * entropy and the mutual information between prediction and weights (BALD) through per-row accumulators.  (ABI-4-compatible
 * additions.)
 *
 * Accumulators: one caller-owned device float buffer [rows][ld_acc] per head, ld_acc >= hmp_mc_acc_ld(n_classes) (= 2 * Cp + 4 with
 * Cp = n_classes rounded up to 4; 0 for n_classes < 1).  A row holds
 *   A[c] = sum_t p_t[c]   at column c,          c < n_classes
 *   B[c] = sum_t p_t[c]^2 at column Cp + c,     c < n_classes
 *   E    = sum_t h_t      at column 2 * Cp;
 * every other column of the row (the padding behind A and B, everything past 2 * Cp) is never read or written.
 *
 * hmp_mc_accumulate_rows adds ONE sample: for a row's scores s = d_logits[r, 0:n_classes),
 *   p[c] = expf(s[c] - m) / sum_c' expf(s[c'] - m), m the row maximum -- the arithmetic and association of hmp_topk_rows (per lane
 *   of the row's 16 in ascending column order, then an xor butterfly, whatever the pitch): p[c] is bit-equal to the probability
 *   hmp_topk_rows stores for class c on the same scores;
 *   h = -sum_c p[c] * logf(p[c]) in the same association, a term with p[c] == 0 being 0;
 *   A[c] += p[c], B[c] += p[c] * p[c], E += h.  first != 0 STORES the sample instead: the buffer needs no memset and may hold
 *   anything, NaN included.  The row's 16 lanes are its only writer and samples are ordered by the stream: no atomics, results are
 *   bit-reproducible.  Rows with d_members[r] == 0 (d_members NULL: every row) are not touched.  NaN scores are unspecified.  One
 *   launch; n_rows == 0 launches nothing; nothing synchronises. */
int32_t hmp_mc_acc_ld(int32_t n_classes);
int hmp_mc_accumulate_rows(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const uint8_t* d_members, int32_t first,
                           float* d_acc, int32_t ld_acc, void* stream);
/* The statistics of `samples` = T accumulated samples (1 <= T <= 4096, else HMP_E_ARG), one launch over plain buffers:
 *   mean[c] = A[c] / (float)T;   label = first-maximum argmax of mean (hmp_predict_rows' rule);
 *   std = sqrtf(max(0, B[label] / T - mean[label]^2));   entropy = -sum_c mean[c] * logf(mean[c]) (a zero term is 0);
 *   mutual_info = max(0, entropy - E / T).
 * d_labels int64 [n_rows], d_mean float [n_rows][ld_mean] (ld_mean >= n_classes; columns >= n_classes are not written), d_std /
 * d_entropy / d_mi float [n_rows]: each may be NULL (skipped), not all.  A row with d_members[r] == 0 holds -1 / 0 and its
 * accumulators are not read.  Every requested element of rows [0, n_rows) is written exactly once, nothing behind them.  n_rows == 0
 * launches nothing; nothing synchronises. */
int hmp_mc_finish(const float* d_acc, int32_t ld_acc, int32_t n_rows, int32_t n_classes, int32_t samples, const uint8_t* d_members,
                  int64_t* d_labels, float* d_mean, int32_t ld_mean, float* d_std, float* d_entropy, float* d_mi, void* stream);
/* d_count: device float holding the valid-label count or weight sum (grad_scale = 1 / (count > 0 ? count : 1)); NULL => grad_scale = 1 */
int hmp_adam_flat(float* d_p, const float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int32_t step, const float* d_count, void* stream);

/* keep-mask generator of the engine's feature dropout, exposed so tests can replay it in the oracle:
 * element (row, col) of a [n_rows, F] tensor is kept iff mask[row*F+col] != 0 (d_mask: device uint8 [n_rows * F], every element
 * written 0 or 1, nothing behind them; n_rows == 0 or F == 0 writes nothing).
 *
 * The generator (csrc/common.h: hash32, drop_thresh, drop_pair, drop_keep4; every draw site of the library calls the same four).
 * All arithmetic is on 32-bit unsigned words and wraps modulo 2^32; >> is a logical shift.
 *
 *   hash32(x):  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16;  return x
 *
 *   seed words: k0 = seed mod 2^32 (low word), k1 = seed >> 32 (high word)
 *   key  = k0 ^ (rng_stream * 0x9E3779B1) ^ (rng_step * 0x85EBCA77) ^ hash32(k1)
 *          (one word per launch, the same for every element; hash32(0) == 0, so the k1 term vanishes for a seed below 2^32)
 *
 *   The counter is the quad number q, a 32-bit word (a tensor of more than 2^32 quads wraps).  Quad q draws two words
 *     a = hash32(q ^ key)
 *     b = hash32((a + 0x9E3779B9) ^ k1 ^ (q * 0xC2B2AE3D))
 *   and its four elements j = 0 .. 3 draw the 16-bit halves
 *     draw[0] = a & 0xFFFF,   draw[1] = a >> 16,   draw[2] = b & 0xFFFF,   draw[3] = b >> 16.
 *
 *   Keep rule: element j is kept iff draw[j] >= (thresh >> 16), with
 *     thresh = (uint32) min(trunc((double)(float)p * 2^32), 2^32 - 1)
 *   -- p is the C float of the call (a caller holding a double rounds it to float first); the product is exact in double.
 *
 *   Quad numbering of a [n_rows, F] tensor: a row is padded to qpr = (F + 3) >> 2 quads, and element (row, col) is element
 *   j = col & 3 of quad q = row * qpr + (col >> 2), computed as a 32-bit word.  The elements col >= F of a row's last quad are drawn
 *   and discarded: a row always starts a fresh quad, so masks of different F share no layout.
 *   GAT attention dropout numbers the coefficient (pos, head) of edge position pos (CSR position of the edge, self loops at
 *   E + node) as element (pos, head) of a [*, 8] tensor whatever the number of heads: quad q = 2 * pos + (head >> 2), element
 *   j = head & 3; hmp_dropout_mask(seed, step, stream, p, P, 8, ...) replays it.
 *
 * What the 16-bit resolution means: the keep probability is 1 - floor((float)p * 65536) / 65536, not 1 - p, while kept values are
 * scaled by 1.f / (1.f - p) (float arithmetic) at every draw site; the expectation is off by less than 2^-16 / (1 - p) relative.
 * A p below 2^-16 (p == 0 included) drops nothing.  rng_step and rng_stream are full 32-bit words; all 64 bits of the seed count.
 * What the key being one xor-ed word means: two sites whose keys differ by d draw the same first words at permuted quads
 * (a of quad q at one is a of quad q ^ d at the other; the second words differ).  Stream, step and high seed word are spread over
 * the word by their multipliers and the hash, so d exceeds any tensor's quad count in practice; seeds that differ in low bits of
 * the low word only (s and s + 1) give a small d.  Choose seeds at random (the models draw 62 random bits), not consecutively. */
int hmp_dropout_mask(uint64_t seed, uint32_t rng_step, uint32_t rng_stream, float p, int32_t n_rows, int32_t F,
                     uint8_t* d_mask, void* stream);

/* Test and diagnostic entries of the readout launchers (csrc/semisup.hip, csrc/heads.hip) as the fused steps call them: each
 * descriptor is copied as it stands into the launcher's argument struct; the launchers' own argument checks apply and nothing
 * else.  ABI-4-compatible additions (hmp_sizeof 14, 15).  d_state: device int32[5] with the layout of the executor's state
 * block -- word 1 is the status (bit 1: a counted label outside [0, classes)); the other words are not touched.
 * The dropout site (seed, rng_step, rng_stream, p) is the one hmp_dropout_mask(seed, rng_step, rng_stream, p, n_rows, classes or F)
 * replays; p == 0: no dropout.
 *
 * One head's rows for the tail launches.  z [n_rows][ldz] final state, y = dropout(act(z)) over its first `classes` columns;
 * grad [n_rows][ldg] receives d(SUM loss) / d z (columns classes .. ldg written 0), row_lv [rows][2] = {loss, valid} per CE row.
 * Pooled modes: the CE / count rows are the n_pool pooled rows, each the mean of y over its leaves (divisor max(deg, 1)); rowptr /
 * col: CSR by pooled row, t_rowptr / t_col: CSC by leaf (hmp_plan's d_rowptr, d_col, d_t_rowptr, d_t_col); rowptr NULL = identity
 * pool (n_pool == n_rows).  labels, mask and row_lv are then per pooled row; dpool [n_pool][ldp] is scratch (d loss / d pooled / deg,
 * ldp >= ldg). */
typedef struct hmp_tail_desc {
  const float* z;
  const int64_t* labels;
  const uint8_t* mask; /* NULL: every row */
  float* grad;
  float* row_lv;
  const int32_t *rowptr, *col, *t_rowptr, *t_col;
  float* dpool;
  int32_t ldz, n_rows, classes, ldg, slot, n_pool, ldp; /* slot: d_counts[2 * slot] += {correct, total} */
  uint32_t rng_step, rng_stream;
  float p;
  uint64_t seed;
} hmp_tail_desc;
/* n = 1 or 2 heads in one launch.  mode 0: the unpooled CE (any width); 1: the unpooled accuracy count (ACCUMULATES into d_counts,
 * device int64[4]; eval mode: no dropout); 2: the pooled CE launch followed by the leaf-gradient launch (classes <= 256);
 * 3: the pooled accuracy count.  act: HMP_ACT_*.  A count row counts iff its mask byte is set (or mask is NULL). */
int hmp_head_tails(const hmp_tail_desc* d, int32_t n, int32_t mode, int32_t act, int64_t ignored, int32_t* d_state,
                   int64_t* d_counts, void* stream);
/* the same with class weights for the CE modes: d_w[i] device float [d[i].classes] or NULL (d_w NULL: hmp_head_tails) */
int hmp_head_tails_weighted(const hmp_tail_desc* d, int32_t n, const float* const* d_w, int32_t mode, int32_t act, int64_t ignored,
                            int32_t* d_state, int64_t* d_counts, void* stream);
/* The label launch of the same descriptors (eval mode): d_pred[i] (device int64) receives the prediction the count of mode 1
 * (pooled != 0: mode 3) compares, for EVERY row of head i -- its n_rows leaf rows, or its n_pool pooled rows (an empty pooled row
 * predicts 0).  labels, mask, grad, row_lv, dpool, t_rowptr and t_col may be NULL.  One launch for both heads.  (ABI-4-compatible
 * addition, like hmp_linear_heads_predict below.) */
int hmp_head_tails_predict(const hmp_tail_desc* d, int32_t n, int32_t pooled, int32_t act, int64_t* const* d_pred, void* stream);
/* The top-k launch of the same descriptors (eval mode, the contract of hmp_topk_rows on the rows hmp_head_tails_predict walks):
 * d_labels[i] int64 [rows][k] and d_probs[i] float [rows][k] for EVERY row of head i (an empty pooled row is all zeros: labels
 * 0 .. k-1, each 1 / classes).  Of a head's two pointers either may be NULL, both only when the head has no rows.  1 <= k <= 8.
 * One launch for both heads. */
int hmp_head_tails_topk(const hmp_tail_desc* d, int32_t n, int32_t pooled, int32_t act, int32_t k, int64_t* const* d_labels,
                        float* const* d_probs, void* stream);
/* The Monte-Carlo launch of the same descriptors (TRAINING mode: the tail draws at each descriptor's dropout site; the contract of
 * hmp_mc_accumulate_rows on the rows hmp_head_tails_topk walks): d_acc[i] float [rows][ld_acc[i]] for EVERY row of head i (an empty
 * pooled row is all zeros: p = 1 / classes).  d_acc[i] may be NULL only when the head has no rows.  One launch for both heads. */
int hmp_head_tails_mc(const hmp_tail_desc* d, int32_t n, int32_t pooled, int32_t act, int32_t first, float* const* d_acc,
                      const int32_t* ld_acc, void* stream);
/* Two linear heads over one final state z [n_rows][ldz]: logits_h = dropout(act(z)) W_h^T + b_h on the rows of head h (member[0]
 * NULL: every row; member[1] NULL: the complement of member[0], empty when both are NULL), W_h [classes[h]][F] dense.
 * grad [n_rows][ldg], ldg == F rounded up to 4 (columns F .. ldg written 0); row_lv [n_rows][2] = {loss_0 + loss_1, valid_0 + valid_1};
 * workgroup b writes its partial dW [K][ld_slab] then db [K] (K = classes[0] + classes[1], head 0's rows first) at
 * slabs + b * slab_stride; the caller sums the first *n_blocks_out slabs. */
typedef struct hmp_linear_heads_desc {
  const float* z;
  const float* W[2];
  const float* bias[2];
  const int64_t* labels;
  const uint8_t* mask;
  const uint8_t* member[2];
  float* grad;
  float* row_lv;
  float* slabs;
  int64_t slab_stride, ignored;
  uint64_t seed;
  int32_t ldz, n_rows, F, classes[2], act, ldg, ld_slab;
  uint32_t rng_step, rng_stream;
  float p;
} hmp_linear_heads_desc;
/* train = 1: the CE launch; train = 0: the accuracy count (eval mode), ACCUMULATES {correct_0, total_0, correct_1, total_1} into
 * d_counts (device int64[4]).  *n_blocks_out (may be NULL) = the workgroups launched = min(ceil(n_rows / 32), 240). */
int hmp_linear_heads_run(const hmp_linear_heads_desc* d, int32_t train, int32_t* d_state, int64_t* d_counts, int32_t* n_blocks_out,
                         void* stream);
/* the same with class weights for the CE launch: d_w[h] device float [classes[h]] or NULL (d_w NULL: hmp_linear_heads_run) */
int hmp_linear_heads_run_weighted(const hmp_linear_heads_desc* d, const float* const* d_w, int32_t train, int32_t* d_state,
                                  int64_t* d_counts, int32_t* n_blocks_out, void* stream);
/* The label launch (eval mode): d_pred[h] (device int64 [n_rows], NULL: head skipped) = first-maximum argmax of head h's logits
 * for the rows of member[h] (the rule above), -1 elsewhere.  labels, mask, grad, row_lv and slabs may be NULL. */
int hmp_linear_heads_predict(const hmp_linear_heads_desc* d, int64_t* const* d_pred, int32_t* n_blocks_out, void* stream);
/* The top-k launch (eval mode, the contract of hmp_topk_rows on head h's logits): d_labels[h] int64 [n_rows][k], d_probs[h] float
 * [n_rows][k] for the rows of member[h], -1 / 0 elsewhere; a head whose two pointers are both NULL is skipped.  1 <= k <= 8. */
int hmp_linear_heads_topk(const hmp_linear_heads_desc* d, int32_t k, int64_t* const* d_labels, float* const* d_probs,
                          int32_t* n_blocks_out, void* stream);
/* The Monte-Carlo launch (TRAINING mode: the tail draws at the descriptor's dropout site; the contract of hmp_mc_accumulate_rows on
 * head h's logits): d_acc[h] float [n_rows][ld_acc[h]], touched on the rows of member[h] alone; a head with a NULL accumulator is
 * skipped. */
int hmp_linear_heads_mc(const hmp_linear_heads_desc* d, int32_t first, float* const* d_acc, const int32_t* ld_acc, int32_t* n_blocks_out,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * 6. network executor -- the whole HeteroConv layer stack as one native program.
 *    Replaces HeterogeneousNetwork.forward (models/heterogeneous_network.py:99-122),
 *    HeterogeneousNeuralTreeNetwork.forward (models/heterogeneous_neural_tree_network.py:154-185),
 *    HomogeneousNetwork.forward SAGE/GAT branches (models/homogeneous_network.py:122-139) and, for the
 *    fused step, the loop body of BaseTrainingJob.train (base_training_job.py:202-216).
 * ------------------------------------------------------------------------------------------- */
#define HMP_CONV_SAGE 0
#define HMP_CONV_GAT 1
#define HMP_ACT_NONE 0
#define HMP_ACT_RELU 1
#define HMP_ACT_ELU 2

typedef struct hmp_conv_spec {
  int32_t kind;       /* HMP_CONV_* */
  int32_t edge_type;  /* index into hmp_batch edge arrays */
  int32_t src, dst;   /* node type indices */
  int32_t f_out;      /* SAGE: out width; GAT: channels C per head */
  int32_t heads, concat, self_loops, edge_dim; /* GAT only */
  int32_t fill_mean;  /* GAT_edge self-loop attr: 1 = per-destination mean, 0 = zeros */
  int32_t shared_lin; /* GAT built from an int in_channels: lin_dst IS lin_src */
  int32_t active;     /* 0 = output never reaches the loss: skipped in forward and backward */
  int32_t agg_first;  /* SAGE, src != dst: 1 = aggregate the source rows first, then project the (few) destination rows -- the order
                       * [PyG] SAGEConv itself uses (lin_l(mean_j x_j)); exact algebra, chosen by the caller for
                       * convs whose destination type is much smaller than the source type (objects -> rooms at 10^6 objects).
                       * At most one such conv per source type and layer.  0: project every source row, gather the projected rows */
  float att_dropout;  /* GAT: dropout on the attention coefficients (GATConv(dropout=p)), training only */
  /* offsets (floats) into the flat parameter buffer, -1 = absent.
   * SAGE: w0 = lin_l.weight [f_out, f_src], b0 = lin_l.bias [f_out], w1 = lin_r.weight [f_out, f_dst]
   * GAT : w0 = lin_src.weight [H*C, f_src], w1 = lin_dst.weight [H*C, f_dst], a0 = att_src [H*C],
   *       a1 = att_dst [H*C], w2 = lin_edge.weight [H*C, edge_dim], a2 = att_edge [H*C], b0 = bias */
  int64_t w0, w1, w2, a0, a1, a2, b0;
} hmp_conv_spec;

typedef struct hmp_layer_spec {
  int32_t n_convs;
  int32_t act;         /* activation applied to this layer's output (HMP_ACT_NONE on the last) */
  float dropout;       /* feature dropout after the activation (training only) */
  int32_t group_mean;  /* HeteroConv aggr: 0 = sum, 1 = mean over the convs reaching a node type */
  int32_t out_dim[HMP_MAX_NODE_TYPES]; /* output width per node type (0 = type receives nothing) */
  /* layer 0 only: node types the layer does not produce but whose INPUT features stay visible to layer 1
   * (`x_dict.update(pre_mp(...))`, heterogeneous_neural_tree_network.py:158-159); out_dim must equal in_dim */
  int32_t passthrough[HMP_MAX_NODE_TYPES];
  hmp_conv_spec convs[HMP_MAX_CONVS];
} hmp_layer_spec;

typedef struct hmp_net_spec {
  int32_t n_node_types, n_edge_types, n_layers;
  int32_t in_dim[HMP_MAX_NODE_TYPES];
  int32_t edge_src[HMP_MAX_EDGE_TYPES], edge_dst[HMP_MAX_EDGE_TYPES];
  int32_t readout_type;    /* node type whose final state is the output */
  int32_t pool_edge_type;  /* -1, or LeafPool edge type: output = segment mean over it, first n_out rows */
  int32_t aux_readout_type; /* -1, or a SECOND node type whose final state is an output too: the two-headed task
                             * (`return x_dict["rooms"], x_dict["objects"]`, heterogeneous_network.py:123-135); read with
                             * hmp_net_aux_output, its gradient enters through hmp_net_backward2 */
  int64_t n_params;        /* total floats in the flat parameter buffer */
  int64_t n_active_params; /* parameters [0, n_active) receive gradients; the tail is dead weights */
  hmp_layer_spec layers[HMP_MAX_LAYERS];
  /* two-headed task only: the activation (HMP_ACT_*) and feature dropout the model applies to BOTH final states after the last
   * layer (heterogeneous_network.py:124-134).  The program itself ends at the last conv (its layer has act NONE, dropout 0);
   * only the step2 / count_correct2 entries below read these */
  int32_t tail_act;
  float tail_dropout;
} hmp_net_spec;

typedef struct hmp_batch {
  int32_t n_nodes[HMP_MAX_NODE_TYPES];
  const float* d_x[HMP_MAX_NODE_TYPES];   /* [n_nodes, in_dim] */
  int32_t ldx[HMP_MAX_NODE_TYPES];
  int64_t n_edges[HMP_MAX_EDGE_TYPES];
  const int64_t* d_edge_index[HMP_MAX_EDGE_TYPES]; /* [2][E] int64 */
  const float* d_edge_attr[HMP_MAX_EDGE_TYPES];    /* [E, edge_dim] or NULL */
  int32_t n_out;             /* rows of the output (== n_nodes[readout] unless pooled) */
  const int64_t* d_labels;   /* [n_out] int64, or NULL (forward only) */
  int32_t plan_valid;        /* != 0: the caller vouches that every edge list equals the previous call's (same topology, e.g.
                              * consecutive frames of the inference server, bin/room_classification_server:273-299): the CSR /
                              * CSC plan in the workspace is reused instead of rebuilt.  Counts must match the previous call. */
  /* optional: the batch as a disjoint union of graphs ([PyG] Batch.ptr per node type; base_training_job.py:164-168 collates
   * that way); read with d_edge_ptr below.  n_graphs = 0: unknown (any edge structure is accepted). */
  const int64_t* d_node_ptr[HMP_MAX_NODE_TYPES]; /* [n_graphs + 1] int64 row offsets of the node type, or NULL */
  int32_t n_graphs;
  int32_t max_graph_nodes;   /* largest per-graph node count over all types, 0 = unknown: accepted and not read (its reader,
                              * the graph-local launch, was removed) */
  /* optional, with d_node_ptr of both endpoint types: [n_graphs + 1] int64 edge offsets of the edge type -- the caller vouches
   * that the edges of graph g are entries [ptr[g], ptr[g+1]) of the edge list and join nodes of graph g only (what every
   * collation of a list of graphs produces: [PyG] Batch.from_data_list, base_training_job.py:164-168).  The single-launch plan
   * build then reads, per block of rows, only the edges of the graphs that own those rows instead of the whole list.  An edge
   * found outside its graph's rows sets status bit 4.  NULL: no assumption about the edge order. */
  const int64_t* d_edge_ptr[HMP_MAX_EDGE_TYPES];
} hmp_batch;

typedef struct hmp_train_args {
  float lr, beta1, beta2, eps, weight_decay;
  int64_t ignored_label;
  uint64_t seed;
  int32_t training;          /* dropout on */
  int32_t* d_step;           /* device int32 owned by the optimiser state (next to Adam's m / v): the step counter t that
                              * Adam's bias correction and the dropout stream read; bumped once at the head of every
                              * step.  NULL: the net's own counter (one optimiser per net).  torch.optim.Adam keeps
                              * `state['step']` per optimiser in the same way (base_training_job.py:181-185) */
} hmp_train_args;

typedef struct hmp_net hmp_net; /* opaque */

int hmp_net_create(const hmp_net_spec* spec, hmp_net** out);
void hmp_net_destroy(hmp_net* net);
/* device bytes the executor needs for batches up to these capacities */
size_t hmp_net_workspace_bytes(const hmp_net* net, const int32_t* cap_nodes, const int64_t* cap_edges);
int hmp_net_bind_workspace(hmp_net* net, void* d_workspace, size_t bytes, const int32_t* cap_nodes, const int64_t* cap_edges);

/* forward: builds the plan for `batch`, runs every layer; *d_out -> [n_out, out_dim] inside the
 * workspace (ld = *ld_out).  rng_step selects the dropout stream of this call. */
int hmp_net_forward(hmp_net* net, const hmp_batch* batch, const float* d_params, int32_t training, uint64_t seed,
                    uint32_t rng_step, const float** d_out, int32_t* ld_out, void* stream);
/* backward of the last forward: d_gout [n_out, ld_gout] -> flat gradient d_grads[0 : n_active_params)
 * (overwritten, not accumulated).  d_gx[t] (may be NULL) receives d loss / d x[t], ld = ldx[t]. */
int hmp_net_backward(hmp_net* net, const float* d_gout, int32_t ld_gout, const float* d_params, float* d_grads,
                     float* const* d_gx, void* stream);
/* two-headed nets (spec.aux_readout_type >= 0): the final state of the second node type after the last forward
 * ([*n_rows, *ld_out] inside the workspace), and the backward that takes a gradient for both outputs (either may be NULL = zero;
 * d_gout_aux is [n_nodes[aux], ld_aux], any ld >= the type's output width). */
int hmp_net_aux_output(hmp_net* net, const float** d_out, int32_t* ld_out, int32_t* n_rows);
int hmp_net_backward2(hmp_net* net, const float* d_gout, int32_t ld_gout, const float* d_gout_aux, int32_t ld_aux,
                      const float* d_params, float* d_grads, float* const* d_gx, void* stream);

/* fused training step, phase A: plan + forward + masked CE + backward.  Leaves the SUM-loss gradient in
 * d_grads[0 : n_active) and {loss_sum, count} in d_grads[n_active], d_grads[n_active+1] so that ONE
 * all-reduce(sum) over n_active+2 floats averages count-weighted across ranks.  Phase B: Adam on
 * [0, n_active) with grad scale 1/count read from that tail.  The step counter lives on the device so
 * both phases can be replayed from a captured hipGraph. */
int hmp_net_step_fwd_bwd(hmp_net* net, const hmp_batch* batch, const float* d_params, float* d_grads,
                         const hmp_train_args* args, void* stream);
int hmp_net_step_adam(hmp_net* net, float* d_params, const float* d_grads, float* d_m, float* d_v,
                      const hmp_train_args* args, void* stream);
/* single-rank step: phase A + phase B in one call (no collective in between).  Lets the executor fold Adam into the
 * gradient un-pack kernel where the network allows it (SAGE stacks); the result equals A followed by B. */
int hmp_net_step_fused(hmp_net* net, const hmp_batch* batch, float* d_params, float* d_grads, float* d_m, float* d_v,
                       const hmp_train_args* args, void* stream);
/* Two-headed task (spec.aux_readout_type >= 0): the loop body of SemiSupervisedTrainingJob.train
 * (semisupervised_training_job.py:117-147) and the per-batch arithmetic of its test() (:198-257).
 *   Targets: d_labels[0] / d_mask[0] belong to the readout type, [1] to the aux type ([n_nodes[t]] int64 labels, one byte per
 *   node as mask, mask NULL = every row).  A row counts iff (mask == NULL || mask[row]) && label != ignored_label; an in-mask
 *   label outside [0, classes) sets status bit 2 (hmp_net_read_state).
 *   Tail of each type t with final state z (the output of the last conv): y = dropout(act(z)), act = spec.tail_act,
 *   p = spec.tail_dropout (training only), then the masked CE on y; the step writes dL/dz = (softmax(y) - onehot) . keep/(1-p) .
 *   act'(z) where the backward reads the gradient of that type.
 *   Dropout numbering: the keep-mask of type t is tensor 8 * (n_layers - 1) + t of the step's draw number (the device counter
 *   the step bumps at its head, hmp_train_args::d_step), element (row, col) in quad row * ceil(out_dim / 4) + col / 4 -- i.e.
 *   exactly hmp_dropout_mask(seed, step, 8 * (n_layers - 1) + t, p, n_rows, out_dim) and hmp_bias_act_drop_fwd on the same
 *   coordinates.  (The final state is stored at pitch 4 * ceil(out_dim / 4), so the layer epilogues' pitch numbering coincides.)
 *   Loss: {loss_sum, count} are summed over the readout rows, then the aux rows, in a fixed order: one count over both heads,
 *   the normalisation of the reference's list-form cross_entropy_loss.  The flat-gradient contract is the single-head step's:
 *   SUM-loss gradient in d_grads[0 : n_active), {loss_sum, count} in d_grads[n_active], d_grads[n_active + 1]; phase B is
 *   hmp_net_step_adam.  Both phases are capturable.  Nets without aux_readout_type are refused. */
typedef struct hmp_head_targets {
  const int64_t* d_labels[2]; /* [0] readout type, [1] aux type; [n_nodes[t]] int64 */
  const uint8_t* d_mask[2];   /* bool per node, or NULL = every row */
} hmp_head_targets;

int hmp_net_step2_fwd_bwd(hmp_net* net, const hmp_batch* batch, const hmp_head_targets* targets, const float* d_params,
                          float* d_grads, const hmp_train_args* args, void* stream);
int hmp_net_step2_fused(hmp_net* net, const hmp_batch* batch, const hmp_head_targets* targets, float* d_params, float* d_grads,
                        float* d_m, float* d_v, const hmp_train_args* args, void* stream);
/* eval-mode forward, y = act(z) on both final states (no dropout), first-maximum row argmax, compared with the labels under the
 * masks (ignored_label plays no part: the reference's test() counts every masked row).  ACCUMULATES into d_counts (device int64[4])
 * {correct_readout, total_readout, correct_aux, total_aux}; one launch beyond the forward, nothing synchronises. */
int hmp_net_count_correct2(hmp_net* net, const hmp_batch* batch, const hmp_head_targets* targets, const float* d_params,
                           int64_t* d_counts, void* stream);
/* Pooled heads (HeterogeneousNeuralTreeNetwork with output_dim_dict, heterogeneous_neural_tree_network.py:186-205): head h's CE
 * and count read pooled[v] = mean over the edges (leaf -> v) of pool_edge_type_h of dropout(act(z[leaf])) (0 for a v with no
 * edge), one row per node of the edge type's destination, instead of the final state's rows.  The keep-mask stays the one of the
 * leaf rows (the rule above); hmp_head_targets then hold one label / mask byte per DESTINATION row.  -1 = an unpooled head.  The
 * edge type must start at the head's readout type and end at a node type that no last-layer conv writes.  Called once, before the
 * first workspace bind; the two-head entries above change their loss and count launches, nothing else changes.  Both step phases
 * stay capturable, and the gradient is summed without float atomics (bitwise reproducible). */
int hmp_net_set_head_pools(hmp_net* net, int32_t pool_edge_type_readout, int32_t pool_edge_type_aux);
/* Two LEARNED linear heads over one final state (HomogeneousNetwork / HomogeneousNeuralTreeNetwork with output_dim_dict,
 * homogeneous_network.py:122-147, homogeneous_neural_tree_network.py:96-109): the loop body of SemiSupervisedTrainingJob.train
 * (semisupervised_training_job.py:117-147, homogeneous branches) and the per-batch arithmetic of its test() (:198-257).
 *   z = the program's output [n_out][F] (the last conv, or the pooled output with pool_edge_type); y = dropout(act(z)) over EVERY
 *   row, act = spec.tail_act, p = spec.tail_dropout (training only), keep-mask = tensor 8 * (n_layers - 1) of the step's draw
 *   number in quad row * ceil(F / 4) + col / 4 (the hmp_net_step2_* rule above); logits_h = y[rows_h] W_h^T + b_h, with W_h
 *   [classes[h]][F] and b_h [classes[h]] read from the flat parameters at w_off[h] / b_off[h].  A row may be in no head, one or
 *   both.  Loss: the summed CE of both heads over rows_h AND mask AND label != ignored_label, over one total count (the
 *   reference's list-form cross_entropy_loss); an in-mask member label outside [0, classes[h]) sets status bit 2.
 *   The head parameters must lie in [0, n_active): their gradients join the flat gradient (summed per workgroup slab by the
 *   gradient un-pack, no float atomics: bitwise reproducible) and phase B's Adam.  The flat-gradient contract, the two phases and
 *   capturability are hmp_net_step2_*'s.  set_linear_heads is called once, before the first workspace bind; F must equal the
 *   program's output width, 1 <= classes[h] <= 64. */
typedef struct hmp_linear_heads {
  int32_t F;
  int32_t classes[2];         /* [0] room head, [1] object head */
  int64_t w_off[2], b_off[2]; /* float offsets of W_h / b_h in the flat parameter buffer */
} hmp_linear_heads;
typedef struct hmp_linear_head_targets {
  const int64_t* d_labels;    /* [n_out] int64, one label per row */
  const uint8_t* d_mask;      /* bool per row (train / val / test mask), NULL = every row */
  const uint8_t* d_member[2]; /* bool per row: rows of the room / object head; d_member[1] NULL = NOT d_member[0] */
} hmp_linear_head_targets;

int hmp_net_set_linear_heads(hmp_net* net, const hmp_linear_heads* heads);
/* Class weights of the cross entropy of every later training step of `net`, whatever its form (hmp_net_step_*, hmp_net_step2_*,
 * hmp_net_step_heads_*): head 0 = the readout (rooms), head 1 = the aux readout or the second linear head (objects).  d_w is a
 * BORROWED device float vector of n entries that must outlive the steps; n must equal the head's class count (HMP_ERR_ARG names
 * both numbers otherwise; set linear heads first).  d_w == NULL clears the head's weights: the unweighted step, bit for bit.
 * Weighted, a row contributes {w[y] * nll, w[y]} and w[y] * (softmax - onehot): {loss_sum, count} hold the weighted sum and the
 * sum of weights, and Adam divides by that sum.  No launch is added: the vector travels next to the label pointer of each CE
 * launch and an unweighted step issues no load for it.  (ABI-4-compatible addition.) */
int hmp_net_set_class_weights(hmp_net* net, int32_t head, const float* d_w, int32_t n);
int hmp_net_step_heads_fwd_bwd(hmp_net* net, const hmp_batch* batch, const hmp_linear_head_targets* targets, const float* d_params,
                               float* d_grads, const hmp_train_args* args, void* stream);
int hmp_net_step_heads_fused(hmp_net* net, const hmp_batch* batch, const hmp_linear_head_targets* targets, float* d_params,
                             float* d_grads, float* d_m, float* d_v, const hmp_train_args* args, void* stream);
/* eval-mode forward, logits of both heads on act(z) (no dropout), first-maximum argmax, compared with the labels of the member
 * rows under the mask (every masked row counts).  ACCUMULATES {correct_room, total_room, correct_object, total_object} into
 * d_counts (device int64[4]); nothing synchronises. */
int hmp_net_count_correct_heads(hmp_net* net, const hmp_batch* batch, const hmp_linear_head_targets* targets, const float* d_params,
                                int64_t* d_counts, void* stream);
/* Room task (one output, no aux readout, no linear heads): the per-batch arithmetic of BaseTrainingJob.test
 * (base_training_job.py:269-313).  Eval-mode forward (no dropout, no fused CE), then ONE hmp_count_correct_rows launch on the
 * program's output with the labels batch->d_labels over batch->n_out rows, the classes = the output width, the optional row
 * filter d_members [n_out] and ignored_label.  ACCUMULATES {correct, total} into d_counts (device int64[2]) and, if d_confusion !=
 * NULL, the [classes][classes] confusion matrix.  A batch without labels and two-headed nets (hmp_net_count_correct2 /
 * hmp_net_count_correct_heads) are refused.  The activations of the last forward are overwritten; nothing synchronises. */
int hmp_net_count_correct_rooms(hmp_net* net, const hmp_batch* batch, const float* d_params, const uint8_t* d_members,
                                int64_t ignored_label, int64_t* d_counts, int64_t* d_confusion, void* stream);
/* The same per graph: ONE eval-mode forward, then ONE hmp_count_correct_rows_by_graph launch on the program's output.  The graph of
 * an output row comes from the batch itself: batch->n_graphs and batch->d_node_ptr[t] of the output node type t (the pool edge
 * type's destination, else the readout type), which must be set (HMP_E_ARG otherwise; d_edge_ptr is not needed).  ACCUMULATES
 * into d_counts (device int64 [n_graphs][2] = {correct, total} per graph).  Refusals and side effects as
 * hmp_net_count_correct_rooms.  (ABI-4-compatible addition.) */
int hmp_net_count_correct_rooms_by_graph(hmp_net* net, const hmp_batch* batch, const float* d_params, const uint8_t* d_members,
                                         int64_t ignored_label, int64_t* d_counts, void* stream);
/* Label output of every net kind: the eval-mode forward of the count entries, then exactly ONE launch that stores the prediction
 * they compare (int64, first maximum).  No labels are needed in the batch; batch->plan_valid is honoured as hmp_net_forward honours
 * it; the activations of the last forward are overwritten; nothing allocates or synchronises.  Refusals mirror the count entries
 * (wrong net kind, null arguments, unbound workspace).  (ABI-4-compatible additions.)
 * room task (one output): d_pred [n_out] = argmax of the program's output row, -1 where d_members[row] == 0 (d_members NULL: every
 * row).  Two-headed nets are refused. */
int hmp_net_predict_rooms(hmp_net* net, const hmp_batch* batch, const float* d_params, const uint8_t* d_members, int64_t* d_pred,
                          void* stream);
/* two-headed nets with aux readout: d_pred[0] one label per readout row, d_pred[1] per aux row, argmax of act(z); with
 * hmp_net_set_head_pools one label per DESTINATION row of each pooled head (empty row: 0).  Either pointer may be NULL (head
 * skipped). */
int hmp_net_predict2(hmp_net* net, const hmp_batch* batch, const float* d_params, int64_t* const d_pred[2], void* stream);
/* linear heads: d_pred[h] [n_out] = argmax of head h's logits on act(z) for the rows of d_member[h] (hmp_linear_head_targets'
 * member rule, d_member[1] NULL = complement of d_member[0]), -1 elsewhere.  Either d_pred pointer may be NULL (head skipped). */
int hmp_net_predict_heads(hmp_net* net, const hmp_batch* batch, const float* d_params, const uint8_t* const d_member[2],
                          int64_t* const d_pred[2], void* stream);
/* Top-k labels with their softmax probabilities, for every net kind: the eval-mode forward of the predict entries above, then exactly
 * ONE launch (the contract of hmp_topk_rows, on each net kind's score vector = what forward() returns for the row in eval mode).
 * 1 <= k <= 8, else HMP_E_ARG before anything runs.  Outputs are row-major [rows][k]: labels int64, probs float; of each labels /
 * probs pair either may be NULL (that output is skipped).  Column 0 equals the matching predict entry bit for bit.  Everything else
 * -- plan_valid, the overwritten activations, no allocation or synchronisation, the refusals -- is the predict entry's.
 * (ABI-4-compatible additions.)
 * room task: rows = n_out; -1 / 0 in all k columns where d_members[row] == 0.  Not both outputs NULL unless n_out == 0. */
int hmp_net_topk_rooms(hmp_net* net, const hmp_batch* batch, const float* d_params, const uint8_t* d_members, int32_t k,
                       int64_t* d_labels, float* d_probs, void* stream);
/* two-headed nets with aux readout: head 0 per readout row, head 1 per aux row, scores act(z); with hmp_net_set_head_pools per
 * DESTINATION row of each pooled head, scores the LeafPool mean of act(z) (a row without an edge: labels 0 .. k-1, each 1 / C).  A
 * head whose two pointers are both NULL is skipped. */
int hmp_net_topk2(hmp_net* net, const hmp_batch* batch, const float* d_params, int32_t k, int64_t* const d_labels[2],
                  float* const d_probs[2], void* stream);
/* linear heads: head h's logits on act(z) for the rows of d_member[h] (hmp_net_predict_heads' rule), -1 / 0 in all k columns
 * elsewhere.  A head whose two pointers are both NULL is skipped. */
int hmp_net_topk_heads(hmp_net* net, const hmp_batch* batch, const float* d_params, const uint8_t* const d_member[2], int32_t k,
                       int64_t* const d_labels[2], float* const d_probs[2], void* stream);
/* Monte-Carlo dropout, for every net kind: ONE stochastic sample per call -- hmp_net_forward(training = 1, seed, rng_step): feature
 * dropout, GAT attention dropout and the readout's tail dropout all draw at (seed, rng_step) -- then exactly ONE launch (the
 * contract of hmp_mc_accumulate_rows, on each net kind's score vector = what forward() returns for the row in training mode) that
 * adds the sample to the caller's accumulators (first != 0: stores it).  A caller runs T calls with rng_step = first_step + t and
 * then hmp_mc_finish per head.  Everything else -- plan_valid, the overwritten activations, no allocation or synchronisation, the
 * refusals (checked before the forward, an ld_acc below hmp_mc_acc_ld among them) -- is the top-k entry's.  (ABI-4-compatible
 * additions.)
 * room task: rows = n_out; rows with d_members[row] == 0 are not touched. */
int hmp_net_mc_rooms(hmp_net* net, const hmp_batch* batch, const float* d_params, const uint8_t* d_members, uint64_t seed,
                     uint32_t rng_step, int32_t first, float* d_acc, int32_t ld_acc, void* stream);
/* two-headed nets with aux readout: head 0 per readout row, head 1 per aux row, scores dropout(act(z)); with hmp_net_set_head_pools
 * per DESTINATION row of each pooled head, scores the LeafPool mean of dropout(act(z)) (a row without an edge: p = 1 / C).  A head
 * with a NULL accumulator is skipped. */
int hmp_net_mc2(hmp_net* net, const hmp_batch* batch, const float* d_params, uint64_t seed, uint32_t rng_step, int32_t first,
                float* const d_acc[2], const int32_t ld_acc[2], void* stream);
/* linear heads: head h's logits on dropout(act(z)) for the rows of d_member[h] (hmp_net_predict_heads' rule); other rows are not
 * touched.  A head with a NULL accumulator is skipped. */
int hmp_net_mc_heads(hmp_net* net, const hmp_batch* batch, const float* d_params, const uint8_t* const d_member[2], uint64_t seed,
                     uint32_t rng_step, int32_t first, float* const d_acc[2], const int32_t ld_acc[2], void* stream);
/* Attention export of a bound net (any net kind with a GAT layer): the eval-mode forward of `batch` (the predict entries' forward:
 * plan_valid, the overwritten activations, no allocation or synchronisation), then ONE launch -- recorded under profile class 9,
 * gat_fwd -- that writes, for program layer `layer` (0 .. n_layers - 1) and every edge type e with a non-NULL slot, the outputs of
 * hmp_gat_attention for the layer's conv on e: d_alpha[e] [n_edges[e] + n_loop, heads], d_top_src[e] / d_top_w[e]
 * [n_nodes[dst], k], in the order of batch->d_edge_index[e] (whose dropped edges' rows hold 0).  Each of the three arrays of
 * pointers may itself be NULL (= all slots NULL); NULL slots are skipped.  Refused with HMP_E_ARG before anything runs: a layer
 * out of range, a layer that is not GAT, k outside 1 .. 8, a slot on an edge type the layer has no conv for, and a slot whose conv
 * is inactive (hmp_conv_spec::active == 0: its output never reaches the readout, so nothing was computed).
 * (ABI-4-compatible addition.) */
int hmp_net_attention(hmp_net* net, const hmp_batch* batch, const float* d_params, int32_t layer,
                      float* const d_alpha[HMP_MAX_EDGE_TYPES], int32_t k, int64_t* const d_top_src[HMP_MAX_EDGE_TYPES],
                      float* const d_top_w[HMP_MAX_EDGE_TYPES], void* stream);
/* Input gradients of a bound net: the eval-mode forward of `batch` (the predict entries' forward), hmp_saliency_seed over the output
 * rows of `head` into the workspace, then the backward chain WITHOUT the weight gradients down to
 *   d_gx[t] [n_nodes[t], batch->ldx[t]]  =  d (sum over the selected output rows of logit_c or log softmax_c) / d x[t]
 * for every node type t with a non-NULL slot (the real in-dim columns are written; NULL slots are skipped).  head 0: the readout
 * (the pooled rows of a net with pool_edge_type); head 1: the second output of a net with aux_readout_type.  The outputs of such a
 * two-headed net are tail_act(final state), and the gradient chains through that activation.  d_target (NULL: the prediction),
 * the row selection and wrt are hmp_saliency_seed's, over the head's output rows.  No allocation, no synchronisation; overwrites
 * the activations of any earlier forward.  Refused with HMP_E_ARG before anything runs: bf16 compute mode, nets with learned
 * linear heads (hmp_net_set_linear_heads), two-headed nets with pooled heads, a head the net does not have, a d_gx slot of a
 * node type without input rows.  A program with aggregate-first convs (large batches) needs ldx[t] % 4 == 0 for a type whose
 * only live layer-0 conv is aggregate-first.  (ABI-4-compatible addition.) */
int hmp_net_input_gradient(hmp_net* net, const hmp_batch* batch, const float* d_params, int32_t head, const int64_t* d_target,
                           int32_t sel_mode, const uint8_t* d_mask, int32_t ordinal, const int64_t* d_graph_ptr, int32_t n_graphs,
                           int32_t wrt, float* const d_gx[HMP_MAX_NODE_TYPES], void* stream);
/* The plan of `edge_type` as the last forward / step / predict / input-gradient call of the net built it from batch->d_edge_index
 * (CSR by destination, CSC by source; hmp_saliency_topk ranks over it).  Valid until the next such call or workspace re-bind.
 * (ABI-4-compatible addition.) */
int hmp_net_plan(hmp_net* net, int32_t edge_type, hmp_plan* out);
/* diagnosis / tests: where the last forward left the output of layer `layer` (1 .. n_layers) for `node_type`: rows [n_rows, width]
 * at pitch *ld elements, fp32 or (*is_bf16) bfloat16.  A dropped element (training-mode dropout) is stored as -0: its sign bit
 * is the keep-mask the backward reads.  Valid until the next forward / step / workspace re-bind. */
int hmp_net_hidden(hmp_net* net, int32_t layer, int32_t node_type, const void** d_h, int32_t* ld, int32_t* n_rows,
                   int32_t* width, int32_t* is_bf16);
/* compute mode of the dense projections: 0 (default) exact fp32 MFMA everywhere; 1 = GEMM calls in the throughput-bound regime
 * (>= 1024 64x64 output tiles: BASELINE config 5, "hidden=256 bf16") round their operands to bf16 and run on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation; in that regime the intermediates that are only ever gathered or fed to those
 * GEMMs (projected rows Z, their gradient dZ, hidden activations H, input gradients G of 256-wide layers) are also STORED as bf16
 * -- features, logits, parameters, gradients and optimiser state stay fp32.  Not within the 1e-5 parity bar: an explicit
 * precision choice of the caller, checked against oracle/bf16_emul.py (tests/test_gpu_config5.py). */
int hmp_net_set_compute(hmp_net* net, int32_t bf16);
/* host copy of {step counter, status bits}; synchronises the stream */
int hmp_net_read_state(hmp_net* net, int32_t* step, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 7. hipGraph capture of a launch sequence (the step is ~20 short kernels: launch-bound).
 * ------------------------------------------------------------------------------------------- */
typedef struct hmp_graph hmp_graph;
int hmp_graph_begin(void* stream);                   /* stream must not be the null stream */
int hmp_graph_end(void* stream, hmp_graph** out);
int hmp_graph_launch(hmp_graph* g, void* stream);
void hmp_graph_destroy(hmp_graph* g);

/* HIP event timing on the caller's stream (bench.py roofline leg) */
typedef struct hmp_timer hmp_timer;
int hmp_timer_create(hmp_timer** out);
int hmp_timer_start(hmp_timer* t, void* stream);
int hmp_timer_stop(hmp_timer* t, void* stream);
int hmp_timer_elapsed_ms(hmp_timer* t, float* ms); /* synchronises on the stop event */
void hmp_timer_destroy(hmp_timer* t);
/* per-kernel-class device time accumulated by the executor when profiling is on (HIP events around
 * every launch of that class on the executor's stream).  classes: 0 plan, 1 pack, 2 gemm_fwd,
 * 3 aggregate_fwd, 4 loss, 5 aggregate_bwd, 6 gemm_bwd, 7 grad_reduce, 8 adam, 9 gat_fwd, 10 gat_bwd, 11 pool,
 * 12 front (layer-0 projection + plan + pack in one launch, small batches), 13 chain (retired with the graph-local launch,
 * measured slower and removed -- profiles/r02_c_graph_local_chain.md: always 0, kept so that the class count stays 14) */
#define HMP_N_KCLASS 14
int hmp_net_profile(hmp_net* net, int32_t enable);
int hmp_net_profile_read(hmp_net* net, float* ms_sum /*[HMP_N_KCLASS]*/, int32_t* launches /*[HMP_N_KCLASS]*/);

/* ---------------------------------------------------------------------------------------------
 * 8. Device-side collation: replaces [PyG] DataLoader -> Batch.from_data_list + the per-step H2D copy
 *    (base_training_job.py:164-178, :205).  The dataset lives in HBM as packed arrays; a batch = the graphs sel[0..B).
 *    rows:  d_dst[d_dst_off[b] + i] = d_src[d_src_ptr[sel[b]] + i]            (row_bytes per row, any positive size: multiples
 *           of 4 move as 4-byte units and need 4-byte aligned arrays, other sizes -- bool / int8 masks -- move byte by byte)
 *    edges: d_dst[r][d_dst_off[b] + j] = d_src[r][d_edge_ptr[sel[b]] + j] + (r ? d_off_dst : d_off_src)[b]
 *           (d_src is [2][e_total] int64 with graph-local indices, d_dst is [2][e_out])
 * ------------------------------------------------------------------------------------------- */
int hmp_collate_rows(const void* d_src, int64_t row_bytes, const int64_t* d_src_ptr, const int32_t* d_sel,
                     const int64_t* d_dst_off, int32_t B, int64_t n_out_rows, void* d_dst, void* stream);
int hmp_collate_edges(const int64_t* d_src, int64_t e_total, const int64_t* d_edge_ptr, const int32_t* d_sel,
                      const int64_t* d_dst_off, const int64_t* d_off_src, const int64_t* d_off_dst, int32_t B,
                      int64_t e_out, int64_t* d_dst, void* stream);

/* One-launch form: the dataset description is fixed at creation, a batch costs ONE host call and ONE kernel.
 *   slots   the distinct [G + 1] per-graph offset vectors (one per node type and per edge type; host copies are kept);
 *   items   the output arrays: rows (row_bytes > 0: x / y / pos / edge_attr / masks, positioned by `slot`) or an edge_index
 *           (row_bytes == 0: int64 [2][src_total], positioned by `slot`, endpoints shifted by `slot_src` / `slot_dst`).
 * hmp_collator_run: h_sel [B] graph ids (host), d_dst[i] / dst_capacity[i] per item (rows resp. edges), h_totals[slot] receives
 * the batch's node / edge totals (the shapes of the outputs).  No allocation or synchronisation in the steady state.
 * d_offsets_out, when given, is written by every run, a batch in which no item has a row included.
 * (<= 264 words of offsets + selection travel in the kernel's argument block, larger batches through a pinned ring;
 * at most 24 slots and 40 items: the two-headed H-tree dataset with edge attributes has 21 and 39.  Byte-wide rows are a branch
 * of the same kernel: a batch of the two-headed task, labels and masks of both heads included, is still ONE launch.) */
typedef struct hmp_collate_item {
  const void* d_src;         /* null only for a slot that is empty in every graph (no workgroup, nothing written) */
  const int64_t* d_ptr;      /* device copy of the item's [G + 1] offsets */
  int64_t src_total;         /* edges: E_total of the packed edge_index */
  int64_t row_bytes;         /* rows: bytes per row (> 0; not a multiple of 4: copied byte by byte); edges: 0 */
  int32_t slot, slot_src, slot_dst;
} hmp_collate_item;
typedef struct hmp_collator hmp_collator; /* opaque */
int hmp_collator_create(int32_t n_slots, const int64_t* const* h_slot_ptr, int64_t n_graphs, int32_t n_items,
                        const hmp_collate_item* items, hmp_collator** out);
int hmp_collator_run(hmp_collator* c, const int32_t* h_sel, int32_t B, void* const* d_dst, const int64_t* dst_capacity,
                     int64_t* h_totals, int64_t* d_offsets_out /* NULL or [n_slots][offsets_stride]: Batch.ptr of every slot */,
                     int32_t offsets_stride, void* stream);
/* Label filter of the room task on homogeneous graphs (ABI-4-compatible addition: hmp_collate_item keeps its layout).  The fused
 * step reads one int64 label per output row and a homogeneous net has a row per node, so the labels it needs are
 * room_mask[row] ? y[row] : ignored_label.  After this call, item `label_item` (row_bytes == 8: int64 labels) is written by the
 * same launch as  d_member_src[r] != 0 ? src[r] : ignored_label,  r = the row's position in the packed source: d_member_src
 * is the dataset's packed one-byte mask (device), indexed by the per-graph offsets of the label item.  Holds for every later
 * hmp_collator_run, whichever way its tables travel; label_item < 0 clears it.  Host-only: no device call.  HMP_E_ARG for an index
 * outside the items, an item whose rows are not 8 bytes (or not 8-byte aligned) and a null mask. */
int hmp_collator_set_label_filter(hmp_collator* c, int32_t label_item, const uint8_t* d_member_src, int64_t ignored_label);
void hmp_collator_destroy(hmp_collator* c);

/* ---------------------------------------------------------------------------------------------
 * 9. Homogeneous GCN / GIN operators (csrc/homog.hip).  Replace [PyG] GCNConv.propagate + gcn_norm
 *    (models/utils.py:15-16), GINConv.propagate (models/utils.py:17-26) and BatchNorm (models/homogeneous_network.py:93-97).
 *    All take a square plan (n_src == n_dst); projections go through hmp_gemm_f32 BEFORE the neighbourhood sum.
 *    gcn_norm:     dinv[i] = (1 + #{j->i, j != i})^-1/2         (add_remaining_self_loops: one loop of weight 1 per node)
 *    segment_wsum: d_w != NULL (GCN): out_i = w_i ( sum_{j->i, j != i} w_j x_j + w_i x_i )
 *                  d_w == NULL (GIN): out_i = sum_{j->i} x_j + (1 + *d_eps) x_i      (d_eps NULL = 0)
 *                  transpose != 0 runs the same sum over the CSC lists (= the gradient w.r.t. x).
 *    bias_act_drop: y = dropout_p(act(x + bias)), act = HMP_ACT_NONE / RELU / ELU; keep-mask = hmp_dropout_mask(seed, rng_step,
 *                  rng_stream, p, n, F); a dropped element is stored as -0.0f, so the backward needs y only; p > 0 requires an
 *                  activation.
 *    colsum / rowdot_sum: out[c] = sum_r g[r,c];  *out = sum_{r,c} a[r,c] b[r,c]   (fixed summation order)
 *    batchnorm:    torch.nn.BatchNorm1d semantics (training: batch statistics, running stats updated in place with the
 *                  unbiased variance; eval: running statistics).  d_save [2][F] = {mean, 1/sqrt(var+eps)} for the backward.
 * ------------------------------------------------------------------------------------------- */
int hmp_gcn_norm(hmp_plan plan, float* d_dinv, void* stream);
int hmp_segment_wsum(const float* d_x, int32_t ldx, int32_t F, hmp_plan plan, int32_t transpose, const float* d_w,
                     const float* d_eps, float* d_out, int32_t ldo, void* stream);
int hmp_bias_act_drop_fwd(const float* d_x, int32_t ldx, int32_t n_rows, int32_t F, const float* d_bias, int32_t act,
                          float p, uint64_t seed, uint32_t rng_step, uint32_t rng_stream, float* d_y, int32_t ldy,
                          void* stream);
int hmp_bias_act_drop_bwd(const float* d_g, int32_t ldg, const float* d_y, int32_t ldy, int32_t n_rows, int32_t F,
                          int32_t act, float p, float* d_gx, int32_t ldgx, void* stream);
int hmp_colsum(const float* d_g, int32_t ldg, int32_t n_rows, int32_t F, float* d_out, void* stream);
int hmp_rowdot_sum(const float* d_a, int32_t lda, const float* d_b, int32_t ldb, int32_t n_rows, int32_t F, float* d_out,
                   void* stream);
int hmp_batchnorm_fwd(const float* d_x, int32_t ldx, int32_t n_rows, int32_t F, const float* d_gamma, const float* d_beta,
                      float* d_running_mean, float* d_running_var, float momentum, float eps, int32_t training, float* d_y,
                      int32_t ldy, float* d_save, void* stream);
int hmp_batchnorm_bwd(const float* d_g, int32_t ldg, const float* d_x, int32_t ldx, int32_t n_rows, int32_t F,
                      const float* d_gamma, const float* d_save, int32_t training, float* d_gx, int32_t ldgx, float* d_ggamma,
                      float* d_gbeta, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 10. Object connectivity of a room-object scene graph (csrc/dsg.hip).  Replaces the per-frame Python loop
 *     add_object_connectivity (src/hydra_gnn/preprocess_dsgs.py:191-225) with its predicates _is_on / _is_under / _is_near
 *     (:89-180), float64 like numpy.  Objects in the reference's visiting order (ascending node id); d_room[i] = room index or
 *     < 0.  count: d_count[i] = #{j < i in i's room : on | under | near}, d_offset = its exclusive scan (d_offset[n] = total).
 *     fill: d_edges [2][total] = (i, j) pairs ordered by i then j -- the reference's insertion order.
 * ------------------------------------------------------------------------------------------- */
int hmp_object_edges_count(const double* d_pos, const double* d_size, const int32_t* d_room, int32_t n, double threshold_near,
                           double max_near, double max_on, int32_t* d_count, int32_t* d_offset, void* stream);
int hmp_object_edges_fill(const double* d_pos, const double* d_size, const int32_t* d_room, int32_t n, double threshold_near,
                          double max_near, double max_on, const int32_t* d_offset, int32_t* d_edges, int32_t total, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 11. Data-parallel gradient exchange (csrc/comm.hip).  The reference has no multi-GPU code; a batch is a
 *     disjoint union of scene graphs (base_training_job.py:164-168), so ranks exchange nothing but ONE all-reduce(sum) per
 *     step over the flat [gradient sums | loss_sum | count] buffer.  These entry points put that collective on the stream
 *     the step's kernels run on (between hmp_net_step_fwd_bwd and hmp_net_step_adam): RCCL over xGMI, one process per GPU.
 *     Rendezvous: rank 0 calls hmp_comm_unique_id and hands the 128 bytes to the other ranks by any channel the host has
 *     (torch.distributed broadcast, a file, MPI); every rank then calls hmp_comm_create with the device it owns current.
 *     RCCL is resolved at the first call (dlopen): HMP_E_UNSUPPORTED when the machine has none.
 * ------------------------------------------------------------------------------------------- */
#define HMP_COMM_ID_BYTES 128
typedef struct hmp_comm hmp_comm; /* opaque */
int hmp_comm_unique_id(void* id128);
int hmp_comm_create(const void* id128, int32_t rank, int32_t world, hmp_comm** out);
void hmp_comm_destroy(hmp_comm* comm);
/* what RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank): the rank count a benchmark line may quote */
int hmp_comm_query(hmp_comm* comm, int32_t* n_ranks, int32_t* rank);
int hmp_comm_allreduce_sum_f32(hmp_comm* comm, float* d_buf, int64_t n, void* stream);
int hmp_comm_broadcast_f32(hmp_comm* comm, float* d_buf, int64_t n, int32_t root, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 12. H-tree (Neural-Tree) construction on the host (csrc/htree.cpp).  Replaces generate_htree +
 *     add_virtual_nodes_to_htree + the typed extraction of nx_htree_to_torch (src/hydra_gnn/neural_tree/construct.py:241-371,
 *     450-468) and generate_jth / networkx.junction_tree underneath (generate_junction_tree_hierarchies.py:26-116).
 *     Input: a room-object scene graph -- object-object, room-room and room->object edge lists [2][E] int64 (undirected: either
 *     or both directions may be listed).  Output (hmp_htree_sizes, then hmp_htree_fill into caller arrays, all int32):
 *       counts[4]       nodes per type: object, room, object-room, room-room (leaves are COPIES of scene-graph nodes)
 *       object_orig / room_orig   original index (inside its type) of every object / room leaf  == the pool edges o_to_ov / r_to_rv
 *       edges[10]       [2][n] local indices for HTREE_EDGE_TYPES in the reference's order (construct.py:15-26), both directions
 *       init[3]         [2][n] ov_to_or, rv_to_or, rv_to_rr: (original index of the member, clique)
 *     Ties that networkx leaves to Python set order go to the smallest index (see the file header).  Host memory only.
 * ------------------------------------------------------------------------------------------- */
typedef struct hmp_htree hmp_htree; /* opaque */
int hmp_htree_build(int32_t n_objects, int32_t n_rooms, const int64_t* oo_edges, int64_t n_oo, const int64_t* rr_edges,
                    int64_t n_rr, const int64_t* ro_edges, int64_t n_ro, hmp_htree** out);
int hmp_htree_sizes(const hmp_htree* t, int32_t* counts4, int64_t* n_edges10, int64_t* n_init3);
int hmp_htree_fill(const hmp_htree* t, int32_t* object_orig, int32_t* room_orig, int32_t* const* edges10, int32_t* const* init3);
void hmp_htree_destroy(hmp_htree* t);

/* ---------------------------------------------------------------------------------------------
 * 13. Epoch bookkeeping of a training job on the device (csrc/epoch.hip; hydra_gnn_amd/jobs.py).  What BaseTrainingJob.train /
 *     SemiSupervisedTrainingJob.train keep on the host between two steps and two epochs (base_training_job.py:196-246,
 *     semisupervised_training_job.py:112-175): the weighted loss sum, the best validation accuracy, the copy of the best state and
 *     the early-stop counter.  ABI-4-compatible addition (hmp_sizeof 11..13).  accumulate / close / restore only enqueue kernels
 *     (no allocation, no synchronisation, capturable); hmp_epoch_read and hmp_epoch_read_status synchronise.
 *
 *     The record starts zeroed (hipMemset): max_val_acc = 0 and epoch = 0 are the reference's initial values.
 * ------------------------------------------------------------------------------------------- */
#define HMP_EPOCH_STOP 1       /* status bit: early_stop_step == early_stop_window && epoch > early_stop_window */
#define HMP_EPOCH_EMPTY_VAL 2  /* status bit: a validation pass counted no row (the reference divides by zero there) */
#define HMP_EPOCH_MAX_SEGS 64

typedef struct hmp_epoch_ctl {
  double loss_acc;   /* sum over the epoch's steps of loss * weight */
  double weight_acc; /* sum of the weights */
  double max_val_acc;
  int32_t epoch; /* epochs closed so far = index of the next log row */
  int32_t best_epoch;
  int32_t early_stop_step;
  int32_t status;
} hmp_epoch_ctl;

typedef struct hmp_epoch_row {
  double loss;
  double val_acc;
  int64_t correct, total;
  int32_t improved;
  int32_t pad_;
} hmp_epoch_row;

typedef struct hmp_epoch_seg { /* one tensor of the model state and its place in the best-state snapshot (any alignment) */
  const void* src;
  void* dst;
  int64_t bytes;
} hmp_epoch_seg;

/* After a step: loss = d_loss_count ? (double)d_loss[0] / max((double)d_loss_count[0], 1.0) : (double)d_loss[0] -- with the
 * step's flat-gradient tail (d_grads + n_active, d_grads + n_active + 1) that is TrainStep.loss(); w = d_weight ? *d_weight :
 * weight >= 0 ? weight : d_loss_count[0].  loss_acc += loss * w (a rounded product, then a rounded sum); weight_acc += w. */
int hmp_epoch_accumulate(hmp_epoch_ctl* d_ctl, const float* d_loss, const float* d_loss_count, const int64_t* d_weight,
                         double weight, void* stream);
/* After the validation pass: correct / total = the sums of d_counts[0], [2] / [1], [3] (n_counts = 2 or 4).  Writes log row
 * `epoch` (when epoch < log_cap) with loss = loss_acc / (loss_div > 0 ? loss_div : weight_acc); on a strict improvement at
 * epoch >= min_log_epoch copies every segment src -> dst; updates the record; zeroes the accumulators and d_counts.  Two launches:
 * the copy (grid_blocks workgroups, 0 = one) reads the record, the update that follows in stream order writes it. */
int hmp_epoch_close(hmp_epoch_ctl* d_ctl, hmp_epoch_row* d_log, int32_t log_cap, int64_t* d_counts, int32_t n_counts,
                    double loss_div, int32_t min_log_epoch, int32_t early_stop_window, const hmp_epoch_seg* d_segs,
                    int32_t n_segs, int32_t grid_blocks, void* stream);
/* the snapshot back into the model state: every segment dst -> src */
int hmp_epoch_restore(const hmp_epoch_seg* d_segs, int32_t n_segs, int32_t grid_blocks, void* stream);
/* the record and the first min(epoch, log_cap) log rows to the host; *n_rows = that row count.  Synchronises the stream. */
int hmp_epoch_read(const hmp_epoch_ctl* d_ctl, const hmp_epoch_row* d_log, int32_t log_cap, hmp_epoch_ctl* h_ctl,
                   hmp_epoch_row* h_rows, int32_t* n_rows, void* stream);
/* the 4-byte status word alone (the per-epoch read of a job with early stopping).  Synchronises the stream. */
int hmp_epoch_read_status(const hmp_epoch_ctl* d_ctl, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 14. Frame pipeline: the static layers of a scene graph as flat arrays -> every tensor of the HeteroData the models read, for the
 *     baseline room-object graph and for its H-tree (csrc/frame.cpp, csrc/frame.hip; hydra_gnn_amd/dsg.py FramePipeline).  Replaces
 *     GnnModel.convert_graph (bin/room_classification_server:235-271) after the JSON / spark_dsg step: get_room_object_dsg,
 *     add_object_connectivity, to_torch + fill_missing_edge_index, compute_relative_pos and, for H-tree models, generate_htree +
 *     add_virtual_nodes_to_htree + nx_htree_to_torch.
 *
 *     Host stage (host memory only, no GPU needed): hmp_frame_build does all bookkeeping -- the room-object graph in the
 *     reference's visiting order, the object-object predicates in float64 (the function body of section 10), the H-tree topology
 *     (the builder of section 12) -- and lays out ONE staging block and ONE arena.  hmp_frame_pack writes the staging block:
 *       [item table: n_items x HMP_FRAME_ITEM_WORDS int32][sections, each 16-byte aligned: float64 positions and sizes of the
 *        kept objects and the rooms; int32 labels, int64 node ids; int32 one-directional edge lists; for H-trees object_orig,
 *        room_orig, the 10 + 3 edge lists, and the members of every clique]
 *     Device stage: the caller copies the block to the device (one copy) and hmp_frame_expand fills the arena in ONE launch; item i
 *     describes output tensor HMP_FI_TENSOR at byte HMP_FI_DST of the arena, HMP_FI_ROWS x HMP_FI_WIDTH elements.  Every output
 *     element is a function of the staging block and the resident semantic table alone.
 *
 *     Nodes: ids uint64[n], layer int32[n] (2 objects, 3 places, 4 rooms, 5 buildings), pos / bb_min / bb_max float64[n][3],
 *     label int64[n]; undirected edges uint64[2][m] as node ids (self edges and unknown ids are ignored).  Feature rows are
 *     x = [pos | bb size | table[label]] in float32 ((float)double; the float32 table row as is; relative_pos drops the leading 3
 *     columns and adds edge_attr = pos32[dst] - pos32[src], baseline only); rooms take no semantic block.  sem_dim = 0: no table.
 *     With a table a label of a kept object outside [0, n_labels) is refused (HMP_E_ARG, the message names the node id).
 *     clique_dim: width of the H-tree's clique rows (0 = the feature width of the objects / rooms).
 *
 *     Relative positions on an H-tree (the reference's Hydra_mp3d_htree_data.compute_relative_pos, which the server runs after
 *     nx_htree_to_torch for its GAT_edge H-tree models): relative_pos = HMP_FRAME_RELPOS_HTREE with htree = 1.  Every node type's x
 *     loses its three leading columns (a clique row [mean | zeros] becomes clique_dim - 3 zeros; clique_dim 1..3 is refused), the two
 *     clique types get a `pos` (the float32 mean of the member rooms: the three columns their x lost), and every one of the 15 edge
 *     types gets edge_attr = pos[dst] - pos[src] (HMP_FK_EATTR_HT).  The homogeneous layout keeps the edge_attr of the 10 tree edge
 *     types, segment by segment behind edge_index.  relative_pos = 1 with htree stays refused (it never meant this), and
 *     HMP_FRAME_RELPOS_HTREE without htree is refused.
 *
 *     Homogeneous models (HomogeneousNetwork, HomogeneousNeuralTreeNetwork) read the same frame as ONE graph: what
 *     data.heterogeneous_data_to_homogeneous (+ room_mask) makes of the baseline frame, data.heterogeneous_htree_to_homogeneous of
 *     the H-tree (convert_graph's `if homogeneous: to_homogeneous()`).  hmp_frame_build_homogeneous lays the frame out in that form
 *     directly; sizes, host arrays, pack, expand and destroy are the same calls.  Node types are concatenated in store order
 *     (objects, rooms; object, room, object-room, room-room, object_virtual, room_virtual) into one x, zero-padded to the widest
 *     type; every edge type's columns are shifted by the row offsets of its endpoint types and concatenated in edge-type order
 *     (H-tree: the 10 tree types into edge_index / edge_type, the 3 init types into init_edge_index, o_to_ov / r_to_rv into
 *     pool_edge_index -- a split by edge type, so every count is known on the host).  A homogeneous tensor is allocated once
 *     (16-byte aligned) and written by ONE ITEM PER SEGMENT: a node type's rows, or an edge type's columns.  HMP_FI_DST of such an
 *     item is where its segment starts inside the tensor (the first segment's is the tensor's), a row of x is HMP_FI_WIDTH floats
 *     for every segment, and the segments of a tensor follow one another in table order.  An empty segment keeps its item (no
 *     workgroup, no bytes).  Worst case: an H-tree has 6 node and 15 edge types: x 6 + node_type 6 + room_mask 6 + object_mask 6 +
 *     edge_index 10 + edge_type 10 + init 3 + pool 2 = 49 items of the 64 the launch's table holds (baseline: 18).
 * ------------------------------------------------------------------------------------------- */
typedef struct hmp_frame hmp_frame; /* opaque */
int hmp_frame_build(int32_t n, const uint64_t* ids, const int32_t* layer, const double* pos, const double* bb_min,
                    const double* bb_max, const int64_t* label, int64_t m, const uint64_t* edges, double threshold_near,
                    double max_near, double max_on, int32_t htree, int32_t relative_pos, int32_t sem_dim, int32_t n_labels,
                    int32_t clique_dim, hmp_frame** out);
/* the same arguments and refusals; the layout is the homogeneous one (the frame's HMP_FS_* sizes have the same meaning) */
int hmp_frame_build_homogeneous(int32_t n, const uint64_t* ids, const int32_t* layer, const double* pos, const double* bb_min,
                                const double* bb_max, const int64_t* label, int64_t m, const uint64_t* edges, double threshold_near,
                                double max_near, double max_on, int32_t htree, int32_t relative_pos, int32_t sem_dim,
                                int32_t n_labels, int32_t clique_dim, hmp_frame** out);
/* both layouts with `flags`: HMP_FRAME_NO_ROOM_EDGES drops the room-room edges before anything reads them (the reference's
 * Hydra_mp3d_data.remove_room_edges_in_dsg, mp3d_dataset.py:203-208, the `noRE` configurations): rooms_to_rooms is empty and HMP_FS_E_RR
 * is 0; an H-tree is built from the edgeless room layer (every room its own component, no room-room clique).  The result is what
 * the same frame gives with its room-room pairs deleted from `edges`.  flags = 0: hmp_frame_build / hmp_frame_build_homogeneous.
 * The frames of a batch share their flags.  Unknown bits are refused. */
#define HMP_FRAME_NO_ROOM_EDGES 1
int hmp_frame_build_flags(int32_t n, const uint64_t* ids, const int32_t* layer, const double* pos, const double* bb_min,
                          const double* bb_max, const int64_t* label, int64_t m, const uint64_t* edges, double threshold_near,
                          double max_near, double max_on, int32_t htree, int32_t relative_pos, int32_t sem_dim, int32_t n_labels,
                          int32_t clique_dim, int32_t homogeneous, int32_t flags, hmp_frame** out);
#define HMP_FRAME_RELPOS_HTREE 2 /* value of `relative_pos`: relative positions on the edges of an H-tree (htree = 1 only) */
/* sizes[HMP_FS_COUNT] */
#define HMP_FS_KEPT 0          /* kept objects */
#define HMP_FS_DROPPED 1       /* objects with neither a place with a room nor a sibling place with one */
#define HMP_FS_ROOMS 2
#define HMP_FS_E_OO 3          /* object-object edges, one direction */
#define HMP_FS_E_RR 4          /* room-room edges, one direction */
#define HMP_FS_STAGING_BYTES 5 /* what hmp_frame_pack writes */
#define HMP_FS_ARENA_BYTES 6   /* what hmp_frame_expand writes */
#define HMP_FS_ITEMS 7
#define HMP_FS_BLOCKS 8        /* workgroups of the launch */
#define HMP_FS_HT_COUNTS 9     /* +0..3: H-tree nodes per type (object, room, object-room, room-room) */
#define HMP_FS_HT_EDGES 13     /* +0..9: edges per HTREE_EDGE_TYPE */
#define HMP_FS_HT_INIT 23      /* +0..2: init edges ov_to_or, rv_to_or, rv_to_rr */
#define HMP_FS_COUNT 26
/* a frame without a room or without a kept object has HMP_FS_ITEMS = 0: nothing to pack, nothing to launch */
int hmp_frame_sizes(const hmp_frame* f, int64_t* sizes);
/* every pointer may be null: kept / dropped / rooms = indices into the input arrays (visiting order), obj_room[kept],
 * rr_edges [2][E_RR], room_bb [rooms][2][3] (min, max), oo_edges [2][E_OO] (object, earlier object) */
int hmp_frame_host_arrays(const hmp_frame* f, int32_t* kept, int32_t* obj_room, int32_t* dropped, int32_t* rooms, int32_t* rr_edges,
                          double* room_bb, int32_t* oo_edges);
int hmp_frame_pack(const hmp_frame* f, void* staging, int64_t bytes);
void hmp_frame_destroy(hmp_frame* f);

/* words of an item of the staging block's table */
#define HMP_FRAME_ITEM_WORDS 12
#define HMP_FI_KIND 0
#define HMP_FI_TENSOR 1 /* which output tensor (HMP_FT_*) */
#define HMP_FI_ROWS 2
#define HMP_FI_WIDTH 3  /* FEAT / CLIQUE: floats per destination row (a FEAT row's own P0 + 3 + P1 columns, zeros behind them) */
#define HMP_FI_DST 4    /* byte offset in the arena: 16-byte aligned for a whole tensor; a segment of a homogeneous tensor starts
                           at a multiple of its element size (x rows: of the row size) inside a 16-byte aligned tensor */
#define HMP_FI_S0 5     /* byte offsets of source sections in the staging block (-1: none); meaning per kind, see csrc/frame.hip */
#define HMP_FI_S1 6
#define HMP_FI_S2 7
#define HMP_FI_S3 8
#define HMP_FI_P0 9     /* parameters per kind */
#define HMP_FI_P1 10
#define HMP_FI_BLOCK0 11 /* first workgroup of the item (the prefix table of the launch) */
#define HMP_FRAME_MAX_ITEMS 64
/* item kinds */
#define HMP_FK_FEAT 0   /* float32 rows [pos | size | table[label]], optionally gathered through a row-index vector */
#define HMP_FK_POS 1    /* float32 [rows][3] */
#define HMP_FK_I64 2    /* int64 [rows] from an int32 (labels) or int64 (node ids) section */
#define HMP_FK_EDGE 3   /* int64 [2][width] from an int32 list */
#define HMP_FK_EATTR 4  /* float32 [rows][3] = pos32[dst] - pos32[src] */
#define HMP_FK_CLIQUE 5 /* float32 rows [mean float32 position of the member rooms | zeros] without their first P0 columns (0, or
                           3 for the all-zero clique x of an HMP_FRAME_RELPOS_HTREE frame) */
#define HMP_FK_EDGE_SEG 6 /* HMP_FI_WIDTH columns of an int64 [2][S1] tensor from an int32 list (P0, P1 as EDGE): row 1 lies S1
                             elements behind row 0; S2 is added to every source, S3 to every destination (S1..S3: numbers) */
#define HMP_FK_CONST 7  /* HMP_FI_ROWS elements of P1 bytes (8: int64, 1: a bool mask), every one P0 */
#define HMP_FK_EATTR_HT 8 /* float32 [rows][3] = pos[dst] - pos[src] on an H-tree edge list (S0; P0, P1 as EDGE).  S1 is a descriptor
                             section of 2 x HMP_FRAME_END_WORDS int32, source end then destination end: {mode, position section,
                             index or ptr section, member section}.  The three sections are byte offsets RELATIVE TO THE DESCRIPTOR
                             (so a batch moves a frame's sections without touching it; 0 where the mode has none) */
#define HMP_FRAME_END_WORDS 4
#define HMP_FE_DIRECT 0   /* pos32 of row i of a float64 position section */
#define HMP_FE_GATHER 1   /* pos32 of row index[i]: a leaf, through object_orig / room_orig */
#define HMP_FE_CLIQUE 2   /* the float32 mean of the member rooms of clique i (ptr, members): the arithmetic of HMP_FK_CLIQUE */
/* output tensors: baseline 0..15 = {objects, rooms} x {x, pos, label, node_ids}, then edge_index and edge_attr of
 * objects_to_objects, rooms_to_rooms, rooms_to_objects, objects_to_rooms; H-tree 16.. = {object, room} x {x, pos, label},
 * object-room.x, room-room.x, {object_virtual, room_virtual} x {x, pos, label}, the 10 HTREE_EDGE_TYPES, the 3 init edge types,
 * o_to_ov, r_to_rv */
#define HMP_FT_HTREE 16
#define HMP_FT_COUNT 45
/* homogeneous frames (hmp_frame_build_homogeneous) use only these: +0 x, +1 edge_index, +2 node_type, +3 edge_type, +4 room_mask
 * (bytes), +5 edge_attr (relative_pos); H-tree: +6 object_mask (bytes), +7 init_edge_index, +8 pool_edge_index */
#define HMP_FT_HOMOG 45
#define HMP_FT_HOMOG_COUNT 9
/* One launch on `stream`: d_staging = the packed block on the device (16-byte aligned), d_arena >= HMP_FS_ARENA_BYTES (16-byte
 * aligned), d_sem_table float32 [n_labels][sem_dim] (8-byte aligned; null when sem_dim = 0); n_items / n_blocks from hmp_frame_sizes.
 * The item table lives on the device, so this entry cannot compare it with its arguments; the caller owes it three things:
 *   - sem_dim and the table are those hmp_frame_build was given.  A feature item laid out for another sem_dim (its HMP_FI_P1), or a
 *     launch without the table, does not read the table: the semantic columns of that item are written as zeros, nothing is refused;
 *   - the table has at least the n_labels rows hmp_frame_build was given: the row count is not passed to the device, the labels
 *     were checked against n_labels on the host and that check is the only bound of the table reads;
 *   - every launch that uses the same staging block or arena runs on ONE stream (they are ordered by it alone). */
int hmp_frame_expand(const void* d_staging, void* d_arena, const float* d_sem_table, int32_t sem_dim, int32_t n_items,
                     int32_t n_blocks, void* stream);

/* ---- batches of frames: K frames -> ONE block, ONE upload, ONE launch -> the collated batch the models read, or the packed arrays
 *      of a GraphStore, as views of one arena (csrc/frame.cpp, csrc/frame.hip; dsg.FramePipeline.convert_batch,
 *      store.GraphStore.from_frames).
 *
 *     hmp_frame_batch_build takes frames that hmp_frame_build / hmp_frame_build_homogeneous made, all with the SAME configuration
 *     (typed / homogeneous, htree, relative_pos, sem_dim, n_labels, clique_dim; anything else is HMP_E_ARG), and keeps pointers to
 *     them: they must outlive the batch.  A frame with HMP_FS_ITEMS = 0 is skipped (graph_of_frame = -1); the others are the
 *     graphs 0..G-1 in input order.  A batch without a graph has 0 items: nothing to pack, nothing to launch.
 *
 *     HMP_FB_COLLATED is data.collate (typed) / data.collate_homogeneous (homogeneous) of the G single results: every tensor of a
 *     frame becomes the concatenation over the graphs, every edge list has its endpoints shifted by the graph's row offsets of the
 *     endpoint types (homogeneous: the graph's node offset, for edge_index, init_edge_index and pool_edge_index alike).  Typed
 *     batches add the int64 `batch` and `ptr` [G + 1] of every node type and the `ptr` of every edge type.  HMP_FB_STORE is the
 *     same concatenations with graph-local endpoints (what GraphStore keeps): no `batch`, and the offset vectors of the node set(s)
 *     and of every edge list for the homogeneous layout too.
 *
 *     Labels: y[i] = int64 [n] aligned with the INPUT arrays of frame i (y null: no labels; otherwise every frame has one).
 *     Typed baseline: objects.y / rooms.y gathered through kept / rooms; H-tree: object.y / room.y through kept[object_orig] /
 *     rooms[room_orig], object_virtual.y / room_virtual.y as the baseline's; homogeneous: ONE y over all nodes in store order, -1 on
 *     the clique rows.  They are HMP_FK_I64 items with a row-index section (and HMP_FK_CONST -1); no kind is added.
 *
 *     The item table is the frames' items re-addressed, one item per (graph, segment), tensor by tensor and graph by graph inside a
 *     tensor: sections rebased to the batch block, HMP_FI_DST = where the segment starts inside the batched tensor (the first
 *     segment's is the tensor's, 16-byte aligned; segments follow one another), an edge list = HMP_FK_EDGE_SEG with the batched
 *     tensor's pitch and the graph's two shifts, `batch` segments = HMP_FK_CONST with the graph number, offset vectors = HMP_FK_I64
 *     from an int64 section.  An empty segment keeps its item and shares its successor's HMP_FI_BLOCK0 (trailing ones: the block
 *     count).  Offsets are int32: a block or an arena beyond 2^31 - 1 bytes is refused.
 *
 *     Block: [group table: one int32 per HMP_FRAME_MAX_ITEMS items = HMP_FI_BLOCK0 of the group's first item, padded to 16 bytes]
 *            [item table: n_items x HMP_FRAME_ITEM_WORDS int32, padded to 16 bytes][sections, each 16-byte aligned: the frames' own,
 *            graph by graph, then the offset vectors, the label vectors and their row-index vectors].  At most
 *     HMP_FRAME_MAX_ITEMS groups, so HMP_FRAME_BATCH_MAX_ITEMS items; more is refused (the message names the limit). */
typedef struct hmp_frame_batch hmp_frame_batch; /* opaque */
#define HMP_FB_COLLATED 0
#define HMP_FB_STORE 1
#define HMP_FRAME_BATCH_MAX_ITEMS 4096
int hmp_frame_batch_build(int32_t n_frames, const hmp_frame* const* frames, int32_t form, const int64_t* const* y, hmp_frame_batch** out);
/* items a frame of f's configuration adds to a batch, and the items of the batch itself: what a caller cuts chunks by */
int hmp_frame_batch_items_needed(const hmp_frame* f, int32_t form, int32_t with_y, int32_t* per_frame, int32_t* per_batch);
/* sizes[HMP_FBS_COUNT] */
#define HMP_FBS_FRAMES 0          /* input frames */
#define HMP_FBS_GRAPHS 1          /* frames with items: num_graphs */
#define HMP_FBS_MAX_GRAPH_NODES 2 /* most rows of one node type (homogeneous: nodes) in one graph */
#define HMP_FBS_STAGING_BYTES 3   /* what hmp_frame_batch_pack writes */
#define HMP_FBS_ARENA_BYTES 4     /* what hmp_frame_expand_batch writes */
#define HMP_FBS_ITEMS 5
#define HMP_FBS_GROUPS 6
#define HMP_FBS_BLOCKS 7          /* workgroups of the launch */
#define HMP_FBS_NODE_TYPES 8      /* typed: 2 / 6 (store order); homogeneous: 1 */
#define HMP_FBS_EDGE_TYPES 9      /* typed: 4 / 15 (tensor order); homogeneous: edge_index (, init_edge_index, pool_edge_index) */
#define HMP_FBS_TENSORS 10
#define HMP_FBS_COUNT 11
int hmp_frame_batch_sizes(const hmp_frame_batch* b, int64_t* sizes);
/* every pointer may be null: graph_of_frame [FRAMES]; node_ptr [NODE_TYPES][GRAPHS + 1] and edge_ptr [EDGE_TYPES][GRAPHS + 1], the
 * row / column offsets of every graph (data.collate's `ptr`, GraphStore's ptr_host / edge_ptr_host); tensors [TENSORS][4] = tensor
 * number, byte offset in the arena, rows, width (an edge list: 2, columns) of every batched tensor.  kept / dropped / rooms of a
 * frame come from hmp_frame_host_arrays of that frame, as before. */
int hmp_frame_batch_host_arrays(const hmp_frame_batch* b, int32_t* graph_of_frame, int64_t* node_ptr, int64_t* edge_ptr, int64_t* tensors);
int hmp_frame_batch_pack(const hmp_frame_batch* b, void* staging, int64_t bytes);
void hmp_frame_batch_destroy(hmp_frame_batch* b);
/* tensors a batch adds, behind the frames' own: HMP_FT_BATCH + HMP_FTB_BATCH + k = `batch` of node type k, + HMP_FTB_NODE_PTR + k =
 * its `ptr`, + HMP_FTB_EDGE_PTR + k = `ptr` of edge type k, + HMP_FTB_Y + k = y of node type k (homogeneous: k = 0 only) */
#define HMP_FT_BATCH (HMP_FT_HOMOG + HMP_FT_HOMOG_COUNT)
#define HMP_FTB_BATCH 0
#define HMP_FTB_NODE_PTR 6
#define HMP_FTB_EDGE_PTR 12
#define HMP_FTB_Y 27
#define HMP_FT_BATCH_COUNT 33
/* tensors of an HMP_FRAME_RELPOS_HTREE frame, behind everything above: +0 pos of object-room, +1 pos of room-room, +2 + k = edge_attr
 * of H-tree edge type k in the order of the edge_index tensors (10 tree, 3 init, o_to_ov, r_to_rv).  Typed frames: 29 + 17 = 46 items;
 * the homogeneous layout writes edge_attr (HMP_FT_HOMOG + 5) by 10 more segments: 59 items of the 64 the table holds */
#define HMP_FT_HTREL (HMP_FT_BATCH + HMP_FT_BATCH_COUNT)
#define HMP_FT_HTREL_COUNT 17
/* hmp_frame_expand for a batch block: ONE launch of frame_expand_batch_kernel, which finds a workgroup's item through the group
 * table (two dependent 64-lane loads, two ballots) and writes it with the same code as hmp_frame_expand.  The same arguments, the
 * same three things owed by the caller, the same refusals with n_items in [1, HMP_FRAME_BATCH_MAX_ITEMS]. */
int hmp_frame_expand_batch(const void* d_staging, void* d_arena, const float* d_sem_table, int32_t sem_dim, int32_t n_items,
                           int32_t n_blocks, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 15. Derived variants of a device-resident dataset and its node split (csrc/store_derive.hip).  Replaces what the reference's
 *     training scripts do to a loaded dataset in place: compute_relative_pos / to_homogeneous / remove_last_features
 *     (mp3d_dataset.py:29-119, :286-319) and generate_node_split (Stanford3DSG_dataset.py:459-578).  The dataset is the packed form
 *     of section 8: rows of all graphs back to back, graph-LOCAL int64 [2][E] edge lists, [G + 1] offset vectors.
 *
 *     hmp_store_derive: ONE launch runs a table of items that lives in device memory (ABI-4-compatible addition: the table is
 *     plain int64 words, no struct).  Block: [group table: one int64 per 64 items = HMP_SD_BLOCK0 of the group's first item,
 *     padded to an even count][n_items x HMP_SD_ITEM_WORDS].  An item walks the rows of ONE source array; row r of graph g
 *     (HMP_SD_SRC_PTR[g] <= r < HMP_SD_SRC_PTR[g + 1]) goes to destination row HMP_SD_DST_OFF[g] + r - HMP_SD_SRC_PTR[g]:
 *       HMP_SD_ROWS    units of HMP_SD_UNIT bytes (16 / 4 / 1; every width, SKIP and both arrays aligned to it): the destination row
 *                      is DST_W units = source units [SKIP, SKIP + TAKE) of a row of SRC_W units, then zeros
 *       HMP_SD_FILL    the value A0 as int64 (UNIT 8) or one byte (UNIT 1); SRC is unused, SRC_PTR gives the row counts
 *       HMP_SD_EDGES   SRC int64 [2][N] -> DST int64 [2][A3]: row 0 + A0[g], row 1 + A1[g]  (A0 / A1: device int64 [G])
 *       HMP_SD_RELPOS  SRC int64 [2][N] -> DST float [N][3] = A1[(A3[g] + SRC[1][j]) * 3 + c] - A0[(A2[g] + SRC[0][j]) * 3 + c]
 *                      (A0 / A1: float32 positions of the source / destination node type, A2 / A3 their [G + 1] row offsets)
 *     HMP_SD_N = rows (edges) of the source (> 0: a plan leaves empty arrays out), HMP_SD_BLOCK0 = the item's first workgroup; its
 *     workgroups end at the next item's, the last item's at n_blocks, and an item with more work than its workgroups cover in one
 *     pass walks it with a grid stride.  Pointers travel as int64 words.  No atomics: the plan owes that the items tile the outputs.
 *     At most HMP_SD_MAX_ITEMS items (64 groups).
 *     Two kinds select rows by a KEY vector (A0: device int64, one key per source row) and a 64-bit SET (A1: bit k = key k is in
 *     the set; a key outside [0, 64) is in no set) -- the edge-type and clique ablations of the reference (to_homogeneous's
 *     removed_edge_type, mp3d_dataset.py:53-69; x[clique_has == -1] = 0, train_Stanford.py:93-99):
 *       HMP_SD_COMPACT    the rows of graph g whose key is NOT in the set, in source order, back to back from destination row
 *                         DST_OFF[g] (stable).  One wave per graph, 64 rows per sweep, rank = popcount of the ballot below the lane;
 *                         waves stride over the graphs.  Rows of SRC_W = DST_W units of UNIT bytes (8 / 4).  The plan owes DST_OFF from
 *                         the kept rows per graph, which hmp_store_count_kept writes (d_counts [G]; one wave per graph, ballot and
 *                         popcount) and the host reads once.  Every array of one edge list is an item of its own with the same key
 *                         vector: the two rows of edge_index (SRC / DST advanced by the row pitch), edge_type, edge_attr.
 *       HMP_SD_ROWS_ZERO  HMP_SD_ROWS with SKIP 0 and TAKE = SRC_W = DST_W, except that a row whose key is in the set is written as
 *                         zeros (its source is not read).
 *
 *     hmp_store_node_split: one wave per graph writes train / val / test byte rows from d_assign (int8: 0 unassigned, 1 / 2 / 3),
 *     graph g's members starting at d_assign_off[g].  d_member_* null: part a's rows [d_ptr_a[g], d_ptr_a[g + 1]) take the first
 *     assignments, part b's (d_ptr_b, null: none) the following ones.  d_member_* given (one node set, d_ptr_b null): the rows
 *     with d_member_a are ranked first, then those with d_member_b; every other row is written false.
 *     hmp_store_member_counts: d_counts [2][G] = rows with d_member_a / d_member_b per graph.
 * ------------------------------------------------------------------------------------------- */
#define HMP_SD_ITEM_WORDS 16
#define HMP_SD_MAX_ITEMS 4096
#define HMP_SD_KIND 0
#define HMP_SD_BLOCK0 1
#define HMP_SD_SRC 2
#define HMP_SD_DST 3
#define HMP_SD_SRC_PTR 4
#define HMP_SD_DST_OFF 5
#define HMP_SD_N 6
#define HMP_SD_SRC_W 7
#define HMP_SD_SKIP 8
#define HMP_SD_TAKE 9
#define HMP_SD_DST_W 10
#define HMP_SD_A0 11
#define HMP_SD_A1 12
#define HMP_SD_A2 13
#define HMP_SD_A3 14
#define HMP_SD_UNIT 15
#define HMP_SD_ROWS 0
#define HMP_SD_FILL 1
#define HMP_SD_EDGES 2
#define HMP_SD_RELPOS 3
#define HMP_SD_COMPACT 4
#define HMP_SD_ROWS_ZERO 5
int hmp_store_count_kept(const int64_t* d_key, const int64_t* d_ptr, int32_t n_graphs, uint64_t set, int64_t* d_counts, void* stream);
int hmp_store_derive(const int64_t* d_block, int32_t n_items, int32_t n_blocks, int32_t n_graphs, void* stream);
int hmp_store_node_split(const int8_t* d_assign, const int64_t* d_assign_off, int32_t n_graphs, const int64_t* d_ptr_a,
                         const int64_t* d_ptr_b, const uint8_t* d_member_a, const uint8_t* d_member_b, uint8_t* d_train_a,
                         uint8_t* d_val_a, uint8_t* d_test_a, uint8_t* d_train_b, uint8_t* d_val_b, uint8_t* d_test_b, void* stream);
int hmp_store_member_counts(const uint8_t* d_member_a, const uint8_t* d_member_b, const int64_t* d_ptr, int32_t n_graphs,
                            int64_t* d_counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYDRA_MP_H */
