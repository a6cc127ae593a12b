// Network executor: the HeteroConv layer stack of Hydra-GNN's room classifier as one native launch
// sequence (plan -> pack -> per layer {grouped MFMA projection, fused aggregation} -> loss -> per layer
// {transposed aggregation, grouped input-gradient GEMM, grouped split-K weight-gradient GEMM} ->
// gradient un-pack -> Adam).  Shapes come from the batch at call time, every buffer lives in one
// caller-provided workspace, nothing allocates or synchronises, so the whole step can be captured into a
// hipGraph and replayed.
//
// SAGE algebra (exact up to fp32 summation order):
//   HeteroConv-sum over the convs reaching node type t:
//     out_t = sum_e [ W_l,e * mean_e(x_src) + b_e ] + (sum_e W_r,e) * x_t
//   mean and projection commute, so every source type s is projected ONCE per layer by the stacked
//   operand  Wp[l][s] = [ W_l,e1 ; W_l,e2 ; ... ; sum_e W_r,e ]  (Z = x_s * Wp^T), and the aggregation
//   kernel gathers the (narrow) projected rows.  Weight gradients come back de-stacked; every W_r,e of a
//   node type receives the same gradient, every b_e the column sum of the destination gradient.
//
// GAT algebra: the attention logits a_s = <lin_src(x), att_src> = x * V_src with V_src = fold(att_src, W_src)
// (and likewise a_d, and the edge term <lin_edge(e), att_edge> = e * V_edge), so the stacked operand of a source
// type also carries the H rows of V_src^T (and of V_dst^T for the destination role): ONE projection per node
// type yields h_s, a_s and a_d; the chain rule back to lin/att runs in the gradient un-pack kernel.
#include <cstdlib>
#include <vector>

#include "plan_small.h"

using namespace hmp;

namespace {

struct ConvLayout {
  int coff;               // SAGE: column of W_l * x in Z[l][src];  GAT: column of h_s (H*Cp wide)
  int asoff, adoff;       // GAT: columns of a_s in Z[l][src] / a_d in Z[l][dst]
  int H, C, Cp;
  int64_t vedge_off;      // GAT_edge: packed V_edge [GAT_MAX_EDIM][GAT_HMAX]
  int64_t vslab_off;      // GAT_edge: slabs of d V_edge
  bool wd_is_src;         // GAT: the destination role uses lin_src's weights
  // per-conv workspace (GAT)
  float *smax, *sden, *alpha_drop, *dlogit, *dlogit_orig;
  // SAGE, aggregate-first (hmp_conv_spec::agg_first): M = segment mean of the SOURCE rows [n_dst][ld_m] (fp32), projected by
  // W_l [f_out][ldw(src)] at wc_off into columns [aoff, aoff + f_out) of Z[l][dst]; dM its gradient; weight-gradient slabs at cslab_off
  bool agg_first;
  int aoff, ld_m;
  int64_t wc_off, cslab_off;
  float *mrows, *dmrows;
};

struct LayerLayout {
  int kind;
  int n_live;
  int live[HMP_MAX_CONVS];            // indices of live convs
  ConvLayout conv[HMP_MAX_CONVS];
  int n_in[HMP_MAX_NODE_TYPES];       // live convs reaching the node type
  bool reads[HMP_MAX_NODE_TYPES];     // the layer reads this node type's state (ncols > 0, or the source of an aggregate-first conv)
  int aggf_of_src[HMP_MAX_NODE_TYPES];  // the aggregate-first conv whose SOURCE is this node type, -1: none
  int ncols[HMP_MAX_NODE_TYPES];      // width of Z[l][s] (0: type is not read by this layer)
  int roff[HMP_MAX_NODE_TYPES];       // SAGE root segment column in Z[l][t], -1 if none
  int64_t wp_off[HMP_MAX_NODE_TYPES]; // packed weights [ncols][ldw]
  int ldw[HMP_MAX_NODE_TYPES];
  // SAGE layers l >= 1: transposed image WpT [ldw][ldt] of the same weights (columns in the order of wpt_col, kernels.h), ldt =
  // ncols rounded up to 16 with zero padding, written by the pack items that write Wp (PackSeg::dst_t) and read by the fused input gradient; ldt = 0: none
  int64_t wpt_off[HMP_MAX_NODE_TYPES];
  int ldt[HMP_MAX_NODE_TYPES];
  int64_t bias_off[HMP_MAX_NODE_TYPES];
  int64_t slab_off[HMP_MAX_NODE_TYPES];   // packed-gradient slabs [max_slabs][ncols][lddw]
  int lddw[HMP_MAX_NODE_TYPES];
  int64_t bslab_off[HMP_MAX_NODE_TYPES];  // GAT: slabs of the bias column sums [max_slabs][out_dim][4]
  GatLayerS* d_gat;                       // device table (GAT layers)
  GatLayerS h_gat;
};

constexpr int MAX_SLABS = 192;       // split-K slabs per weight-gradient problem (large batches: 256x256 tiles x ~170 node chunks)
static_assert(MAX_SLABS >= GEMM_TALL_SLABS, "the slab buffer must hold what the tall weight-gradient kernel may write");
constexpr int TN_DIRECT_SLABS = 16;  // small batches: more slabs only lengthen the gradient un-pack

struct ProfRec {
  int cls;
  hipEvent_t a, b;
};

}  // namespace

// Test / A-B switches of the executor (environment variables), read ONCE per entry call -- forward, step -- into this block
// (tests flip them between two calls on one net) instead of by getenv() wherever a decision is taken
struct EnvSwitches {
  bool plan_sliced = true;  // HMP_PLAN_SLICED=0: plan parts read the whole edge list (tests compare both builds)
  bool front = true;        // HMP_FRONT=0: separate pack / projection / plan launches
  bool z16 = true;          // HMP_Z16=0: keep fp32 projected rows / gradients in bf16 compute mode
  bool h16 = true;          // HMP_H16=0: keep fp32 activations in bf16 compute mode
  bool rootcopy = false;    // HMP_ROOTCOPY=1: the transposed aggregation copies the root block of dZ
  bool tn_direct = true;    // HMP_TN=0: LDS-staged split-K kernel for the small-batch weight gradients
  bool bf16_all = false;    // HMP_BF16_ALL=1: every GEMM of a bf16-mode net takes the bf16 kernel whatever its size
};

// State of the entry call in progress.  StepGuard sets it up on entry and puts it back to these defaults -- what a plain forward
// and backward see -- on every exit, error returns included; the step driver (run_step) and its loss stages set the rest of the
// inputs.  forward_impl / backward_impl read the inputs and write only the result flags (and consume fin_loss).
struct StepCall {
  // the dropout draw of this call's forward: forward_impl makes it the last forward's once it has accepted the batch
  int training = 0;
  uint64_t seed = 0;
  uint32_t rng_step = 0;
  int* d_step = nullptr;  // training step: its counter (hmp_train_args::d_step or &d_state->step), added to the draw number
  // single-head step: labels for the cross entropy riding in the last aggregation; two-headed step (hmp_net_step2_*): its
  // targets, whose tail + CE ride in that epilogue when it can hold both heads' rows
  const int64_t* ce_labels = nullptr;
  const hmp_head_targets* tgt = nullptr;
  int64_t ce_ignored = 0;
  AdamFuse adam = {};  // fused step: Adam riding in the gradient un-pack
  // backward of a step: the first backward kernel finalises {loss_sum, count} over fin_rows rows of d_row_lv (0: b->n_out);
  // G[L][aux] already written by the loss stage (backward_impl does not stage it); linear heads: workgroup slabs of the
  // head kernel for the gradient un-pack (0: none)
  bool fin_loss = false;
  int fin_rows = 0;
  bool aux_g_ready = false;
  int head_blocks = 0;
  // results: the CE / the heads whose tail + CE rode in the last aggregation's epilogue, Adam ran in the un-pack
  bool ce_done = false;
  bool tail_done[2] = {false, false};
  bool adam_done = false;
};

struct hmp_net {
  hmp_net_spec spec;
  EnvSwitches env;
  int T, ET, L;
  int dim[HMP_MAX_LAYERS + 1][HMP_MAX_NODE_TYPES];  // feature width of H[l][t]
  int ld[HMP_MAX_LAYERS + 1][HMP_MAX_NODE_TYPES];   // leading dimension of our own H/G buffers (l >= 1)
  LayerLayout lay[HMP_MAX_LAYERS];
  int64_t packed_floats, slab_floats;
  int out_dim, out_ld;
  bool any_gat = false;
  bool pass0[HMP_MAX_NODE_TYPES] = {false};  // layer 1 reads the INPUT features of these types (pre_mp passthrough)

  // static device tables (owned)
  PackSeg* d_pack_segs = nullptr;
  int n_pack = 0;
  int64_t pack_rows = 0;
  GradSeg* d_grad_segs = nullptr;
  int n_grad = 0;
  int64_t grad_elems = 0;
  int max_pack_rows = 0;
  int64_t max_grad_elems = 0;
  SegBlocks pack_sb;
  GradRec* d_grad_recs = nullptr;  // grad_reduce_kernel: one record per workgroup (grad_records_build over d_grad_segs)
  int n_grad_recs = 0;
  int2* d_pack_map = nullptr;  // front kernel: pack block (16 items) -> {segment, first item}
  int n_pack_blocks16 = 0;
  char* ws_base = nullptr;
  size_t ws_bytes = 0;
  float* degf[HMP_MAX_EDGE_TYPES];  // 1 / max(in-degree,1) per destination node, by-product of the plan
  bool any_agg_first = false;       // some conv is evaluated aggregate-first (large batches only: never with the small-batch sequence)
  int* d_iota = nullptr;            // 0, 1, 2, ..: row extents AND ids of the identity lists that hand an aggregate-first block to
  float* d_ones = nullptr;          // the aggregation kernels (in-degree 1, weight 1)
  float* d_sadd = nullptr;          // fallback of the gather-add epilogue: the source rows' gradient term as an fp32 matrix (GemmProblem::Cadd)
  int iota_cap = 0;
  int64_t sadd_floats = 0;
  float* d_row_lv = nullptr;        // per output row {loss, valid} of the fused step's loss kernel

  // workspace binding
  bool bound = false;
  int cap_nodes[HMP_MAX_NODE_TYPES];
  int64_t cap_edges[HMP_MAX_EDGE_TYPES];
  NetState* d_state = nullptr;  // owned by the net (NOT part of the re-bindable workspace): status bits and the net's own step counter
  hmp_plan plan[HMP_MAX_EDGE_TYPES];
  int* plan_scratch[HMP_MAX_EDGE_TYPES];
  float* d_packed = nullptr;
  float* d_slabs = nullptr;
  float* H[HMP_MAX_LAYERS + 1][HMP_MAX_NODE_TYPES];
  float* G[HMP_MAX_LAYERS + 1][HMP_MAX_NODE_TYPES];
  bool h16[HMP_MAX_LAYERS + 1][HMP_MAX_NODE_TYPES] = {};  // last forward: H[l][t] was written as bf16 (see forward_impl)
  float* Z[HMP_MAX_LAYERS][HMP_MAX_NODE_TYPES];
  float* dZ[HMP_MAX_LAYERS][HMP_MAX_NODE_TYPES];
  float* d_out = nullptr;   // pooled output [cap_out, out_ld] (only with pool_edge_type)
  float* d_gout = nullptr;  // loss gradient [cap_out, out_ld]
  int cap_out = 0;

  // last forward
  bool have_fwd = false;
  bool plan_ok = false;  // the plan arrays hold the topology of the last batch (cleared by a workspace re-bind)
  hmp_batch batch;
  int training = 0;
  uint64_t seed = 0;
  uint32_t rng_step = 0;
  GradReduceDyn dyn;
  StepCall call;  // the entry call in progress (StepGuard)

  int compute_bf16 = 0;    // hmp_net_set_compute: large grouped GEMMs on the bf16 matrix pipe (fp32 storage and accumulation)
  int fuse_mode = -1;      // HMP_FUSE override (0 / 1), -1 = automatic: row-local GEMMs ride in the aggregation kernels
  bool fuse_now = false;   // decision for the current batch
  bool reuse_plan = false; // this call: hmp_batch::plan_valid accepted
  // linear heads (hmp_net_set_linear_heads): their description and where their per-workgroup slabs start in d_slabs
  bool has_heads = false;
  hmp_linear_heads heads = {};
  int64_t head_slab_off = 0, head_slab_stride = 0;
  int head_ld_slab = 0;
  // pooled heads (hmp_net_set_head_pools): the pool edge type of each head (-1: unpooled), d loss / d pooled per head (the
  // workspace's [cap rows of the pool destination][fpad(classes)] scratch of the pooled CE launch)
  bool has_pools = false;
  int head_pool[2] = {-1, -1};
  float* d_dpool[2] = {nullptr, nullptr};
  // class weights of the cross entropy (hmp_net_set_class_weights): borrowed device vectors, [0] readout / rooms, [1] aux / objects
  // (null: unweighted).  They travel where the labels do: a field of the argument struct, or an argument, of every CE launch.
  const float* class_w[2] = {nullptr, nullptr};

  // profiling
  bool prof = false;
  std::vector<ProfRec> recs;
};

// block maps of a pack table (n <= SEG_MAX): an item is a (packed row, 64-column chunk), one wave each
void hmp::pack_seg_blocks(const PackSeg* ps, int n, SegBlocks& sb) {  // pack_launch: 4 waves per block
  sb.n = n;
  sb.start[0] = 0;
  for (int i = 0; i < n; ++i) sb.start[i + 1] = sb.start[i] + cdiv((int64_t)ps[i].rows_pad * cdiv(ps[i].ld_dst, 64), 4);
}
int hmp::pack_block_map(const PackSeg* ps, int n, int2* pm) {  // front kernel: 16 waves per block; pm == null: only count
  int nb = 0;
  for (int i = 0; i < n; ++i) {
    const int items = ps[i].rows_pad * cdiv(ps[i].ld_dst, 64);
    for (int it = 0; it < items; it += 16, ++nb)
      if (pm) pm[nb] = make_int2(i, it);
  }
  return nb;
}

namespace {

void read_env(hmp_net* n) {
  EnvSwitches e;
  e.plan_sliced = env_switch("HMP_PLAN_SLICED") != '0';
  e.front = env_switch("HMP_FRONT") != '0';
  e.z16 = env_switch("HMP_Z16") != '0';
  e.h16 = env_switch("HMP_H16") != '0';
  e.rootcopy = env_switch("HMP_ROOTCOPY") == '1';
  e.tn_direct = env_switch("HMP_TN") != '0';
  e.bf16_all = env_switch("HMP_BF16_ALL") == '1';
  n->env = e;
}

inline int fpad(int f) { return align4(f); }

// the node type of head h's final state, and the type whose rows carry its labels (the pool destination of a pooled head)
inline int head_type(const hmp_net* n, int h) { return h == 0 ? n->spec.readout_type : n->spec.aux_readout_type; }
inline int label_type(const hmp_net* n, int h) {
  return n->head_pool[h] >= 0 ? n->spec.edge_dst[n->head_pool[h]] : head_type(n, h);
}

int build_layout(hmp_net* n) {
  const hmp_net_spec& S = n->spec;
  n->T = S.n_node_types; n->ET = S.n_edge_types; n->L = S.n_layers;
  HMP_CHECK_ARG(n->T >= 1 && n->T <= HMP_MAX_NODE_TYPES, "net: n_node_types %d", n->T);
  HMP_CHECK_ARG(n->ET >= 1 && n->ET <= HMP_MAX_EDGE_TYPES, "net: n_edge_types %d", n->ET);
  HMP_CHECK_ARG(n->L >= 1 && n->L <= HMP_MAX_LAYERS, "net: n_layers %d", n->L);
  HMP_CHECK_ARG(S.readout_type >= 0 && S.readout_type < n->T, "net: readout_type");
  HMP_CHECK_ARG(S.pool_edge_type >= -1 && S.pool_edge_type < n->ET, "net: pool_edge_type");
  HMP_CHECK_ARG(S.aux_readout_type >= -1 && S.aux_readout_type < n->T && S.aux_readout_type != S.readout_type &&
                    (S.aux_readout_type < 0 || S.pool_edge_type < 0),
                "net: aux_readout_type (a second node type, not with a pooled output)");
  for (int e = 0; e < n->ET; ++e)
    HMP_CHECK_ARG(S.edge_src[e] >= 0 && S.edge_src[e] < n->T && S.edge_dst[e] >= 0 && S.edge_dst[e] < n->T, "net: edge type %d endpoints", e);
  for (int t = 0; t < n->T; ++t) {
    n->dim[0][t] = S.in_dim[t];
    n->ld[0][t] = 0;  // comes with the batch
  }
  int64_t packed = 0, slabs = 0;
  for (int l = 0; l < n->L; ++l) {
    const hmp_layer_spec& Ls = S.layers[l];
    LayerLayout& Y = n->lay[l];
    HMP_CHECK_ARG(Ls.n_convs >= 1 && Ls.n_convs <= HMP_MAX_CONVS, "net: layer %d has %d convs", l, Ls.n_convs);
    Y.kind = Ls.convs[0].kind;
    Y.d_gat = nullptr;
    HMP_CHECK_ARG(Y.kind == HMP_CONV_SAGE || Y.kind == HMP_CONV_GAT, "net: layer %d: unknown conv kind %d", l, Y.kind);
    HMP_CHECK_ARG(Ls.group_mean == 0 || Y.kind == HMP_CONV_GAT, "net: HeteroConv aggr=mean is only supported for GAT layers");
    for (int t = 0; t < n->T; ++t) {
      n->dim[l + 1][t] = Ls.out_dim[t];
      n->ld[l + 1][t] = fpad(Ls.out_dim[t]);
      if (Ls.passthrough[t]) {
        HMP_CHECK_ARG(l == 0 && n->L > 1, "net: passthrough node types are supported on the first layer only");
        HMP_CHECK_ARG(Ls.out_dim[t] == S.in_dim[t], "net: passthrough type %d must keep its input width", t);
        n->pass0[t] = true;
      }
      Y.ncols[t] = 0;
      Y.roff[t] = -1;
      Y.n_in[t] = 0;
      Y.reads[t] = false;
      Y.aggf_of_src[t] = -1;
    }
    Y.n_live = 0;
    int n_outgoing[HMP_MAX_NODE_TYPES] = {0};
    for (int c = 0; c < Ls.n_convs; ++c) {
      const hmp_conv_spec& C = Ls.convs[c];
      ConvLayout& Q = Y.conv[c];
      memset(&Q, 0, sizeof(Q));
      HMP_CHECK_ARG(C.kind == Y.kind, "net: layer %d mixes conv kinds", l);
      HMP_CHECK_ARG(C.edge_type >= 0 && C.edge_type < n->ET, "net: conv edge_type");
      HMP_CHECK_ARG(C.src == S.edge_src[C.edge_type] && C.dst == S.edge_dst[C.edge_type], "net: conv endpoints disagree with edge type");
      HMP_CHECK_ARG(n->dim[l][C.src] > 0 && n->dim[l][C.dst] > 0, "net: layer %d conv %d reads a node type with no features", l, c);
      if (Y.kind == HMP_CONV_SAGE) {
        HMP_CHECK_ARG(C.f_out == Ls.out_dim[C.dst], "net: SAGE f_out must equal the layer's out_dim of the destination type");
      } else {
        HMP_CHECK_ARG(gat_shape_ok(C.heads, C.f_out), "net: GAT heads %d / channels %d unsupported (at most %d channels per head, at most %d heads above 256 channels)",
                      C.heads, C.f_out, GAT_CMAX, GAT_WIDE_HMAX);
        HMP_CHECK_ARG(Ls.out_dim[C.dst] == (C.concat ? C.heads * C.f_out : C.f_out), "net: GAT out_dim mismatch on layer %d conv %d", l, c);
        HMP_CHECK_ARG(C.edge_dim >= 0 && C.edge_dim <= GAT_MAX_EDIM, "net: GAT edge_dim %d > %d", C.edge_dim, GAT_MAX_EDIM);
        HMP_CHECK_ARG(!(C.edge_dim > 0 && C.fill_mean && C.self_loops), "net: fill_value='mean' with edge attributes is not supported (the reference passes zeros)");
        HMP_CHECK_ARG(!C.self_loops || C.src == C.dst, "net: self loops need src == dst (the reference sets add_self_loops = (src == dst))");
      }
      HMP_CHECK_ARG(!C.agg_first || (Y.kind == HMP_CONV_SAGE && C.src != C.dst), "net: agg_first is for SAGE convs between two node types");
      if (!C.active) continue;
      Y.live[Y.n_live++] = c;
      ++Y.n_in[C.dst];
      const bool aggf = C.agg_first != 0;
      ++n_outgoing[aggf ? C.dst : C.src];  // an aggregate-first block is gathered (identity lists) from the DESTINATION type's own Z
      HMP_CHECK_ARG(Y.n_in[C.dst] <= AGG_MAX_IN && n_outgoing[C.src] <= AGG_MAX_IN && n_outgoing[C.dst] <= AGG_MAX_IN,
                    "net: more than %d convs share a node type", AGG_MAX_IN);
      Y.reads[C.src] = Y.reads[C.dst] = true;
      if (Y.kind == HMP_CONV_SAGE) {
        HMP_CHECK_ARG(C.w0 >= 0 && C.b0 >= 0 && C.w1 >= 0, "net: SAGE conv needs lin_l.weight, lin_l.bias, lin_r.weight");
        if (aggf) {
          HMP_CHECK_ARG(Y.aggf_of_src[C.src] < 0, "net: layer %d has two aggregate-first convs from node type %d (at most one)", l, C.src);
          Y.aggf_of_src[C.src] = c;
          Q.agg_first = true;
          Q.ld_m = fpad(n->dim[l][C.src]);
          n->any_agg_first = true;
        } else {
          Q.coff = Y.ncols[C.src];
          Y.ncols[C.src] += fpad(C.f_out);
        }
      } else {
        HMP_CHECK_ARG(C.w0 >= 0 && C.a0 >= 0 && C.a1 >= 0 && C.b0 >= 0, "net: GAT conv needs lin_src, att_src, att_dst, bias");
        HMP_CHECK_ARG(C.edge_dim == 0 || (C.w2 >= 0 && C.a2 >= 0), "net: GAT_edge conv needs lin_edge, att_edge");
        Q.H = C.heads; Q.C = C.f_out; Q.Cp = fpad(C.f_out);
        Q.wd_is_src = (C.src == C.dst) || (C.w1 == C.w0) || (C.w1 < 0);
        HMP_CHECK_ARG(Q.wd_is_src ? (n->dim[l][C.src] == n->dim[l][C.dst]) : true, "net: shared lin with different widths");
        Q.coff = Y.ncols[C.src];
        Y.ncols[C.src] += Q.H * Q.Cp;
        Q.asoff = Y.ncols[C.src];
        Y.ncols[C.src] += fpad(Q.H);
        n->any_gat = true;
      }
    }
    HMP_CHECK_ARG(Y.n_live > 0, "net: layer %d has no live conv", l);
    if (Y.kind == HMP_CONV_SAGE) {
      // column order of Z[l][t]: [blocks of the convs sourced from t] [aggregate-first blocks of convs that END in t] [root]:
      // the root block stays last, where the backward GEMMs can take it from the output gradient in place
      for (int i = 0; i < Y.n_live; ++i) {
        const int c = Y.live[i];
        const hmp_conv_spec& C = Ls.convs[c];
        if (!Y.conv[c].agg_first) continue;
        Y.conv[c].aoff = Y.ncols[C.dst];
        Y.ncols[C.dst] += fpad(C.f_out);
      }
      for (int t = 0; t < n->T; ++t)
        if (Y.n_in[t] > 0) {
          Y.roff[t] = Y.ncols[t];
          Y.ncols[t] += fpad(Ls.out_dim[t]);
        }
    } else {
      for (int i = 0; i < Y.n_live; ++i) {
        const int c = Y.live[i];
        const hmp_conv_spec& C = Ls.convs[c];
        Y.conv[c].adoff = Y.ncols[C.dst];
        Y.ncols[C.dst] += fpad(C.heads);
      }
    }
    for (int t = 0; t < n->T; ++t) {
      Y.ldw[t] = fpad(n->dim[l][t]);
      Y.lddw[t] = fpad(n->dim[l][t] + 1);
      Y.wp_off[t] = packed;
      packed += (int64_t)Y.ncols[t] * Y.ldw[t];
      Y.wpt_off[t] = packed;
      Y.ldt[t] = (l >= 1 && Y.kind == HMP_CONV_SAGE && Y.ncols[t] > 0) ? ((Y.ncols[t] + 15) & ~15) : 0;
      packed += (int64_t)Y.ldw[t] * Y.ldt[t];
      Y.bias_off[t] = packed;
      packed += (Y.n_in[t] > 0) ? fpad(Ls.out_dim[t]) : 0;
      Y.slab_off[t] = slabs;
      slabs += (int64_t)MAX_SLABS * Y.ncols[t] * Y.lddw[t];
      Y.bslab_off[t] = slabs;
      if (Y.kind == HMP_CONV_GAT && Y.n_in[t] > 0) slabs += (int64_t)MAX_SLABS * fpad(Ls.out_dim[t]) * 4;
    }
    for (int i = 0; i < Y.n_live; ++i) {  // aggregate-first convs: their W_l packed on its own, their weight-gradient slabs
      const int c = Y.live[i];
      if (!Y.conv[c].agg_first) continue;
      const hmp_conv_spec& C = Ls.convs[c];
      Y.conv[c].wc_off = packed;
      packed += (int64_t)fpad(C.f_out) * Y.ldw[C.src];
      Y.conv[c].cslab_off = slabs;
      slabs += (int64_t)MAX_SLABS * fpad(C.f_out) * Y.lddw[C.src];
    }
    if (Y.kind == HMP_CONV_GAT) {
      for (int i = 0; i < Y.n_live; ++i) {
        const int c = Y.live[i];
        if (Ls.convs[c].edge_dim > 0) {
          Y.conv[c].vedge_off = packed;
          packed += GAT_MAX_EDIM * GAT_HMAX;
          Y.conv[c].vslab_off = slabs;
          slabs += (int64_t)MAX_SLABS * GAT_MAX_EDIM * GAT_HMAX;
        }
      }
    }
  }
  // liveness must be closed: whatever a live conv produces is consumed by the next layer / the readout
  for (int l = 0; l < n->L; ++l) {
    const LayerLayout& Y = n->lay[l];
    for (int i = 0; i < Y.n_live; ++i) {
      const hmp_conv_spec& C = S.layers[l].convs[Y.live[i]];
      if (l == n->L - 1)
        HMP_CHECK_ARG(C.dst == S.readout_type || C.dst == S.aux_readout_type,
                      "net: last-layer conv %d is active but does not feed a readout type", Y.live[i]);
      else
        HMP_CHECK_ARG(n->lay[l + 1].reads[C.dst], "net: layer %d conv %d is active but layer %d never reads its output", l, Y.live[i], l + 1);
    }
  }
  n->packed_floats = packed;
  n->slab_floats = slabs;
  n->out_dim = n->dim[n->L][S.readout_type];
  n->out_ld = fpad(n->out_dim);
  HMP_CHECK_ARG(n->out_dim > 0, "net: readout type has no output in the last layer");
  HMP_CHECK_ARG(S.aux_readout_type < 0 || n->dim[n->L][S.aux_readout_type] > 0, "net: second readout type has no output in the last layer");
  return HMP_OK;
}

inline int slab_id_w(int l, int t) { return l * SLAB_IDS_PER_LAYER + t; }
inline int slab_id_b(int l, int t) { return l * SLAB_IDS_PER_LAYER + HMP_MAX_NODE_TYPES + t; }
inline int slab_id_v(int l, int c) { return l * SLAB_IDS_PER_LAYER + 2 * HMP_MAX_NODE_TYPES + c; }

GradTerm term(int kind, int slab_id, int64_t src, int ld, int C, int Cp, int inner = 0, int64_t att = 0, int64_t w = 0, int ldw = 0,
              float scale = 1.f) {
  GradTerm t;
  memset(&t, 0, sizeof(t));
  t.kind = kind; t.slab_id = slab_id; t.src = src; t.ld = ld; t.C = C; t.Cp = Cp; t.inner = inner;
  t.att = att; t.w = w; t.ldw = ldw; t.scale = scale;
  return t;
}

// the workgroup records of the gradient un-pack for segment table gs (kernels.h grad_records_build), replacing the net's
int upload_grad_records(hmp_net* n, const std::vector<GradSeg>& gs) {
  int64_t nb = 0;
  for (const GradSeg& g : gs) nb += grad_seg_blocks(g);
  HMP_CHECK_ARG(nb <= INT32_MAX, "net: %lld gradient un-pack workgroups", (long long)nb);
  std::vector<GradRec> recs((size_t)nb);
  const int64_t got = grad_records_build(gs.data(), (int)gs.size(), recs.data());
  HMP_CHECK_ARG(got == nb, "net: gradient record table: %lld records for %lld workgroups", (long long)got, (long long)nb);
  GradRec* d = nullptr;
  if (nb > 0) {
    HMP_HIP(hipMalloc(&d, recs.size() * sizeof(GradRec)));
    if (hipMemcpy(d, recs.data(), recs.size() * sizeof(GradRec), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(d);
      snprintf(err_buf(), 512, "net: copy of the gradient record table failed");
      return HMP_E_HIP;
    }
  }
  if (n->d_grad_recs) (void)hipFree(n->d_grad_recs);
  n->d_grad_recs = d;
  n->n_grad_recs = (int)nb;
  return HMP_OK;
}

// static pack / grad tables ------------------------------------------------------------------------
int build_tables(hmp_net* n) {
  const hmp_net_spec& S = n->spec;
  std::vector<PackSeg> ps;
  std::vector<int64_t> prs;
  std::vector<GradSeg> gs;
  std::vector<int64_t> ges;
  int64_t prow = 0, gel = 0;
  // transposed destination of a PACK_SUM segment that fills rows [coff, coff + rows_pad) of Wp[l][t]: columns of WpT[l][t]; the
  // segment that ends the stack also zeroes the padding columns up to ldt
  auto with_wpt = [&](PackSeg& s, const LayerLayout& Y, int t, int coff) {
    if (Y.ldt[t] == 0) return;
    s.dst_t = Y.wpt_off[t];
    s.col_t = coff;
    s.ld_dst_t = Y.ldt[t];
    s.pad_t = coff + s.rows_pad == Y.ncols[t] ? Y.ldt[t] - Y.ncols[t] : 0;
  };
  auto push_pack = [&](const PackSeg& s) {
    ps.push_back(s); prs.push_back(prow); prow += s.rows_pad;
    if (s.rows_pad > n->max_pack_rows) n->max_pack_rows = s.rows_pad;
  };
  auto push_grad = [&](GradSeg g) {
    gs.push_back(g); ges.push_back(gel); gel += (int64_t)g.rows * g.cols;
    if ((int64_t)g.rows * g.cols > n->max_grad_elems) n->max_grad_elems = (int64_t)g.rows * g.cols;
  };
  for (int l = 0; l < n->L; ++l) {
    const hmp_layer_spec& Ls = S.layers[l];
    const LayerLayout& Y = n->lay[l];
    const float gscale = Ls.group_mean ? 1.f : 1.f;  // weights see the scale through the output gradient; bias below
    (void)gscale;
    for (int i = 0; i < Y.n_live; ++i) {
      const int c = Y.live[i];
      const hmp_conv_spec& C = Ls.convs[c];
      const ConvLayout& Q = Y.conv[c];
      const int fs = n->dim[l][C.src], ft = n->dim[l][C.dst];
      PackSeg s;
      memset(&s, 0, sizeof(s));
      if (Y.kind == HMP_CONV_SAGE) {
        s.kind = PACK_SUM;
        s.dst = Q.agg_first ? Q.wc_off : Y.wp_off[C.src] + (int64_t)Q.coff * Y.ldw[C.src];
        s.rows = C.f_out; s.rows_pad = fpad(C.f_out); s.cols = fs; s.ld_dst = Y.ldw[C.src]; s.ld_src = fs;
        s.nsrc = 1; s.src[0] = C.w0;
        if (!Q.agg_first) with_wpt(s, Y, C.src, Q.coff);
        push_pack(s);
        GradSeg g;
        memset(&g, 0, sizeof(g));
        g.dst = C.w0; g.rows = C.f_out; g.cols = fs; g.n_terms = 1;
        if (Q.agg_first) g.t[0] = term(GT_COPY, slab_id_v(l, c), Q.cslab_off, Y.lddw[C.src], C.f_out, C.f_out);
        else g.t[0] = term(GT_COPY, slab_id_w(l, C.src), Y.slab_off[C.src] + (int64_t)Q.coff * Y.lddw[C.src], Y.lddw[C.src], C.f_out, C.f_out);
        push_grad(g);
        continue;
      }
      // ---- GAT conv -------------------------------------------------------------------------------
      const int HC = Q.H * Q.C;
      const int64_t wd = Q.wd_is_src ? C.w0 : C.w1;
      // h_s rows (heads padded to Cp)
      s.kind = PACK_HEADS; s.H = Q.H; s.C = Q.C; s.Cp = Q.Cp;
      s.dst = Y.wp_off[C.src] + (int64_t)Q.coff * Y.ldw[C.src];
      s.rows = Q.H * Q.Cp; s.rows_pad = Q.H * Q.Cp; s.cols = fs; s.ld_dst = Y.ldw[C.src]; s.ld_src = fs;
      s.nsrc = 1; s.src[0] = C.w0;
      push_pack(s);
      // V_src^T rows
      s.kind = PACK_ATTDOT; s.dst = Y.wp_off[C.src] + (int64_t)Q.asoff * Y.ldw[C.src];
      s.rows = Q.H; s.rows_pad = fpad(Q.H); s.att = C.a0; s.src[0] = C.w0;
      push_pack(s);
      // V_dst^T rows (destination role)
      s.dst = Y.wp_off[C.dst] + (int64_t)Q.adoff * Y.ldw[C.dst];
      s.cols = ft; s.ld_dst = Y.ldw[C.dst]; s.ld_src = ft; s.att = C.a1; s.src[0] = wd;
      push_pack(s);
      if (C.edge_dim > 0) {
        s.kind = PACK_ATTDOT_T; s.dst = Q.vedge_off; s.rows = C.edge_dim; s.rows_pad = GAT_MAX_EDIM; s.cols = Q.H;
        s.ld_dst = GAT_HMAX; s.ld_src = C.edge_dim; s.att = C.a2; s.src[0] = C.w2;
        push_pack(s);
      }
      const int64_t S_hs = Y.slab_off[C.src] + (int64_t)Q.coff * Y.lddw[C.src];
      const int64_t S_as = Y.slab_off[C.src] + (int64_t)Q.asoff * Y.lddw[C.src];
      const int64_t S_ad = Y.slab_off[C.dst] + (int64_t)Q.adoff * Y.lddw[C.dst];
      GradSeg g;
      memset(&g, 0, sizeof(g));
      // lin_src.weight
      g.dst = C.w0; g.rows = HC; g.cols = fs;
      g.t[g.n_terms++] = term(GT_COPY, slab_id_w(l, C.src), S_hs, Y.lddw[C.src], Q.C, Q.Cp);
      g.t[g.n_terms++] = term(GT_ATT_OUTER, slab_id_w(l, C.src), S_as, Y.lddw[C.src], Q.C, Q.C, 0, C.a0);
      if (Q.wd_is_src) g.t[g.n_terms++] = term(GT_ATT_OUTER, slab_id_w(l, C.dst), S_ad, Y.lddw[C.dst], Q.C, Q.C, 0, C.a1);
      push_grad(g);
      if (!Q.wd_is_src) {  // separate lin_dst.weight
        memset(&g, 0, sizeof(g));
        g.dst = C.w1; g.rows = HC; g.cols = ft; g.n_terms = 1;
        g.t[0] = term(GT_ATT_OUTER, slab_id_w(l, C.dst), S_ad, Y.lddw[C.dst], Q.C, Q.C, 0, C.a1);
        push_grad(g);
      }
      memset(&g, 0, sizeof(g));  // att_src
      g.dst = C.a0; g.rows = HC; g.cols = 1; g.n_terms = 1;
      g.t[0] = term(GT_ATT_DOT, slab_id_w(l, C.src), S_as, Y.lddw[C.src], Q.C, Q.C, fs, 0, C.w0, fs);
      push_grad(g);
      memset(&g, 0, sizeof(g));  // att_dst
      g.dst = C.a1; g.rows = HC; g.cols = 1; g.n_terms = 1;
      g.t[0] = term(GT_ATT_DOT, slab_id_w(l, C.dst), S_ad, Y.lddw[C.dst], Q.C, Q.C, ft, 0, wd, ft);
      push_grad(g);
      if (C.edge_dim > 0) {
        memset(&g, 0, sizeof(g));  // lin_edge.weight [HC, D]
        g.dst = C.w2; g.rows = HC; g.cols = C.edge_dim; g.n_terms = 1;
        g.t[0] = term(GT_ATT_OUTER_T, slab_id_v(l, c), Q.vslab_off, GAT_HMAX, Q.C, Q.C, 0, C.a2);
        push_grad(g);
        memset(&g, 0, sizeof(g));  // att_edge
        g.dst = C.a2; g.rows = HC; g.cols = 1; g.n_terms = 1;
        g.t[0] = term(GT_ATT_DOT_T, slab_id_v(l, c), Q.vslab_off, GAT_HMAX, Q.C, Q.C, C.edge_dim, 0, C.w2, C.edge_dim);
        push_grad(g);
      }
      memset(&g, 0, sizeof(g));  // bias: column sums of the destination gradient
      const int wout = Ls.out_dim[C.dst];
      g.dst = C.b0; g.rows = wout; g.cols = 1; g.n_terms = 1;
      g.t[0] = term(GT_COPY, slab_id_b(l, C.dst), Y.bslab_off[C.dst], 4, wout, wout, 0, 0, 0, 0,
                    Ls.group_mean ? 1.f / (float)Y.n_in[C.dst] : 1.f);
      push_grad(g);
    }
    for (int t = 0; t < n->T; ++t) {  // per destination type: SAGE root + bias sums, GAT bias sums
      if (Y.n_in[t] == 0) continue;
      const int fo = Ls.out_dim[t], ft = n->dim[l][t];
      PackSeg s, b;
      memset(&s, 0, sizeof(s));
      memset(&b, 0, sizeof(b));
      s.kind = PACK_SUM; b.kind = PACK_SUM;
      s.dst = Y.wp_off[t] + (int64_t)(Y.roff[t] < 0 ? 0 : Y.roff[t]) * Y.ldw[t];
      s.rows = fo; s.rows_pad = fpad(fo); s.cols = ft; s.ld_dst = Y.ldw[t]; s.ld_src = ft;
      b.dst = Y.bias_off[t];
      b.rows = 1; b.rows_pad = 1; b.cols = fo; b.ld_dst = fpad(fo); b.ld_src = fo;
      for (int i = 0; i < Y.n_live; ++i) {
        const hmp_conv_spec& C = Ls.convs[Y.live[i]];
        if (C.dst != t) continue;
        b.src[b.nsrc++] = C.b0;
        if (Y.kind != HMP_CONV_SAGE) continue;
        s.src[s.nsrc++] = C.w1;
        GradSeg g;
        memset(&g, 0, sizeof(g));
        g.dst = C.w1; g.rows = fo; g.cols = ft; g.n_terms = 1;
        const int64_t root = Y.slab_off[t] + (int64_t)Y.roff[t] * Y.lddw[t];
        g.t[0] = term(GT_COPY, slab_id_w(l, t), root, Y.lddw[t], fo, fo);
        push_grad(g);
        memset(&g, 0, sizeof(g));  // bias: the ones-column (index ft) of the root rows
        g.dst = C.b0; g.rows = fo; g.cols = 1; g.n_terms = 1;
        g.t[0] = term(GT_COPY, slab_id_w(l, t), root + ft, Y.lddw[t], fo, fo);
        push_grad(g);
      }
      if (Y.kind == HMP_CONV_SAGE) {
        with_wpt(s, Y, t, Y.roff[t] < 0 ? 0 : Y.roff[t]);
        push_pack(s);
      }
      push_pack(b);
    }
  }
  prs.push_back(prow);
  ges.push_back(gel);
  n->n_pack = (int)ps.size(); n->pack_rows = prow;
  n->n_grad = (int)gs.size(); n->grad_elems = gel;
  HMP_CHECK_ARG(ps.size() <= (size_t)SEG_MAX && gs.size() <= (size_t)SEG_MAX, "net: too many parameter segments (%zu / %zu > %d)",
                ps.size(), gs.size(), SEG_MAX);
  pack_seg_blocks(ps.data(), (int)ps.size(), n->pack_sb);
  {
    std::vector<int2> pm(pack_block_map(ps.data(), (int)ps.size(), nullptr));
    pack_block_map(ps.data(), (int)ps.size(), pm.data());
    n->n_pack_blocks16 = (int)pm.size();
    if (!pm.empty()) {
      HMP_HIP(hipMalloc(&n->d_pack_map, pm.size() * sizeof(int2)));
      HMP_HIP(hipMemcpy(n->d_pack_map, pm.data(), pm.size() * sizeof(int2), hipMemcpyHostToDevice));
    }
  }
  HMP_HIP(hipMalloc(&n->d_pack_segs, ps.size() * sizeof(PackSeg)));
  HMP_HIP(hipMalloc(&n->d_grad_segs, gs.size() * sizeof(GradSeg)));
  HMP_HIP(hipMemcpy(n->d_pack_segs, ps.data(), ps.size() * sizeof(PackSeg), hipMemcpyHostToDevice));
  HMP_HIP(hipMemcpy(n->d_grad_segs, gs.data(), gs.size() * sizeof(GradSeg), hipMemcpyHostToDevice));
  HMP_TRY(upload_grad_records(n, gs));
  for (int l = 0; l < n->L; ++l)
    if (n->lay[l].kind == HMP_CONV_GAT) HMP_HIP(hipMalloc(&n->lay[l].d_gat, sizeof(GatLayerS)));
  return HMP_OK;
}

// workspace carving: returns bytes; when base != null also assigns pointers ---------------------------
size_t carve(hmp_net* n, char* base, const int32_t* cn, const int64_t* ce) {
  size_t off = 0;
  n->sadd_floats = 0;
  auto take = [&](size_t bytes) -> char* {
    char* p = base ? base + off : nullptr;
    off += align256(bytes);
    return p;
  };
  const hmp_net_spec& S = n->spec;
  for (int e = 0; e < n->ET; ++e) {
    const int ns = cn[S.edge_src[e]], nd = cn[S.edge_dst[e]];
    hmp_plan& P = n->plan[e];
    P.d_rowptr = (int32_t*)take((size_t)(nd + 1) * 4);
    P.d_t_rowptr = (int32_t*)take((size_t)(ns + 1) * 4);
    P.d_col = (int32_t*)take((size_t)ce[e] * 4);
    P.d_eid = (int32_t*)take((size_t)ce[e] * 4);
    P.d_t_col = (int32_t*)take((size_t)ce[e] * 4);
    P.d_t_pos = (int32_t*)take((size_t)ce[e] * 4);
    n->plan_scratch[e] = (int*)take(plan_scratch_ints(ce[e], ns, nd) * 4);
    n->degf[e] = (float*)take((size_t)nd * 4);
  }
  n->d_packed = (float*)take((size_t)n->packed_floats * 4);
  n->d_slabs = (float*)take((size_t)n->slab_floats * 4);
  for (int l = 0; l <= n->L; ++l)
    for (int t = 0; t < n->T; ++t) {
      n->H[l][t] = n->G[l][t] = nullptr;
      if (l >= 1 && n->dim[l][t] > 0 && !(l == 1 && n->pass0[t])) {
        n->H[l][t] = (float*)take((size_t)cn[t] * n->ld[l][t] * 4);
        n->G[l][t] = (float*)take((size_t)cn[t] * n->ld[l][t] * 4);
      }
    }
  for (int l = 0; l < n->L; ++l) {
    LayerLayout& Y = n->lay[l];
    for (int t = 0; t < n->T; ++t) {
      n->Z[l][t] = n->dZ[l][t] = nullptr;
      if (Y.ncols[t] > 0) {
        n->Z[l][t] = (float*)take((size_t)cn[t] * Y.ncols[t] * 4);
        n->dZ[l][t] = (float*)take((size_t)cn[t] * Y.ncols[t] * 4);
      }
    }
    int64_t sf = 0;  // gather-add scratch: one matrix per aggregate-first conv of the layer, side by side
    for (int i = 0; i < Y.n_live; ++i) {
      const int c = Y.live[i];
      ConvLayout& Q = Y.conv[c];
      if (!Q.agg_first) continue;
      const hmp_conv_spec& C = S.layers[l].convs[c];
      Q.mrows = (float*)take((size_t)cn[C.dst] * Q.ld_m * 4);
      Q.dmrows = (float*)take((size_t)cn[C.dst] * Q.ld_m * 4);
      sf += (int64_t)cn[C.src] * Q.ld_m;
    }
    n->sadd_floats = sf > n->sadd_floats ? sf : n->sadd_floats;
    if (Y.kind != HMP_CONV_GAT) continue;
    for (int i = 0; i < Y.n_live; ++i) {
      const int c = Y.live[i];
      const hmp_conv_spec& C = S.layers[l].convs[c];
      ConvLayout& Q = Y.conv[c];
      const size_t nd = (size_t)cn[C.dst], ne = (size_t)ce[C.edge_type] + (C.self_loops ? nd : 0);
      Q.smax = (float*)take(nd * GAT_HMAX * 4);
      Q.sden = (float*)take(nd * GAT_HMAX * 4);
      Q.alpha_drop = (float*)take(ne * GAT_HMAX * 4);
      Q.dlogit = (float*)take(ne * GAT_HMAX * 4);
      Q.dlogit_orig = C.edge_dim > 0 ? (float*)take((size_t)ce[C.edge_type] * GAT_HMAX * 4) : nullptr;
    }
  }
  int cap_out = cn[S.readout_type];
  if (S.pool_edge_type >= 0) cap_out = cn[S.edge_dst[S.pool_edge_type]];
  n->cap_out = cap_out;
  n->d_out = (float*)take((size_t)cap_out * n->out_ld * 4);
  n->d_gout = (float*)take((size_t)cap_out * n->out_ld * 4);
  const int cap_aux = S.aux_readout_type >= 0 ? cn[S.aux_readout_type] : 0;  // the aux rows follow the readout rows
  int64_t lv_rows = cap_out + cap_aux;
  n->d_dpool[0] = n->d_dpool[1] = nullptr;
  if (n->has_pools) {  // pooled heads: one {loss, valid} per label row, the aux head's after the readout head's
    const int64_t pr = (int64_t)cn[label_type(n, 0)] + cn[label_type(n, 1)];
    lv_rows = pr > lv_rows ? pr : lv_rows;
    for (int h = 0; h < 2; ++h)
      n->d_dpool[h] = (float*)take((size_t)cn[label_type(n, h)] * n->ld[n->L][head_type(n, h)] * 4);
  }
  n->d_row_lv = (float*)take((size_t)lv_rows * 2 * 4);
  n->d_iota = nullptr; n->d_ones = nullptr; n->d_sadd = nullptr;
  if (n->any_agg_first) {
    int mx = 1;
    for (int t = 0; t < n->T; ++t) mx = cn[t] > mx ? cn[t] : mx;
    n->iota_cap = mx;
    n->d_iota = (int*)take((size_t)(mx + 1) * 4);
    n->d_ones = (float*)take((size_t)mx * 4);
    n->d_sadd = (float*)take((size_t)n->sadd_floats * 4);
  }
  return off;
}

// device tables of the GAT layers (hold workspace pointers => built when the workspace is bound)
int build_gat_tables(hmp_net* n) {
  const hmp_net_spec& S = n->spec;
  for (int l = 0; l < n->L; ++l) {
    LayerLayout& Y = n->lay[l];
    if (Y.kind != HMP_CONV_GAT) continue;
    const hmp_layer_spec& Ls = S.layers[l];
    GatLayerS& G = Y.h_gat;
    memset(&G, 0, sizeof(G));
    int dst_entry[HMP_MAX_NODE_TYPES];
    for (int t = 0; t < n->T; ++t) {
      dst_entry[t] = -1;
      if (Y.n_in[t] == 0) continue;
      dst_entry[t] = G.n_dst;
      GatDstS& D = G.d[G.n_dst++];
      D.t = t;
      D.out = n->H[l + 1][t]; D.ldo = n->ld[l + 1][t];
      D.bias = n->d_packed + Y.bias_off[t];
      D.act = Ls.act;
      D.drop_p = Ls.dropout;
      D.drop_stream = (uint32_t)(l * HMP_MAX_NODE_TYPES + t);
      D.group_scale = Ls.group_mean ? 1.f / (float)Y.n_in[t] : 1.f;
      const bool top = (l == n->L - 1);
      D.g = (top && t != S.aux_readout_type) ? nullptr : n->G[l + 1][t];  // second readout: its gradient is staged in G[L][aux]
      D.ldg = n->ld[l + 1][t];
      for (int i = 0; i < Y.n_live; ++i) {
        const int c = Y.live[i];
        const hmp_conv_spec& C = Ls.convs[c];
        if (C.dst != t) continue;
        const ConvLayout& Q = Y.conv[c];
        if (D.n_in == 0) { D.H = Q.H; D.C = Q.C; D.Cp = Q.Cp; D.concat = C.concat; }
        HMP_CHECK_ARG(D.H == Q.H && D.C == Q.C && D.concat == C.concat, "net: GAT convs reaching one node type must share heads/channels/concat");
        GatInS& I = D.in[D.n_in++];
        const hmp_plan& P = n->plan[C.edge_type];
        I.et = C.edge_type; I.src_t = C.src;
        I.rowptr = P.d_rowptr; I.col = P.d_col; I.eid = P.d_eid;
        I.t_rowptr = P.d_t_rowptr; I.t_col = P.d_t_col; I.t_pos = P.d_t_pos;
        I.z = n->Z[l][C.src]; I.ldz = Y.ncols[C.src]; I.hoff = Q.coff;
        I.za = I.z; I.ldza = I.ldz; I.asoff = Q.asoff;
        I.zd = n->Z[l][t]; I.ldzd = Y.ncols[t]; I.adoff = Q.adoff;
        I.edim = C.edge_dim;
        I.vedge = C.edge_dim > 0 ? n->d_packed + Q.vedge_off : nullptr;
        I.self_loops = C.self_loops;
        I.smax = Q.smax; I.sden = Q.sden;
        I.adrop_p = C.att_dropout;
        I.adrop_stream = (uint32_t)(1000 + l * HMP_MAX_CONVS + c);
        I.alpha_drop = Q.alpha_drop; I.dlogit = Q.dlogit; I.dlogit_orig = Q.dlogit_orig;
        I.dza_src = n->dZ[l][C.src]; I.lddza_src = Y.ncols[C.src];
        I.dz_dst = n->dZ[l][t]; I.lddz_dst = Y.ncols[t];
      }
    }
    for (int s = 0; s < n->T; ++s) {
      GatSrcS* Sx = nullptr;
      for (int i = 0; i < Y.n_live; ++i) {
        const int c = Y.live[i];
        const hmp_conv_spec& C = Ls.convs[c];
        if (C.src != s) continue;
        if (!Sx) {
          Sx = &G.s[G.n_src++];
          Sx->t = s; Sx->dz = n->dZ[l][s]; Sx->lddz = Y.ncols[s];
        }
        // locate the in-conv index inside the destination entry
        const GatDstS& D = G.d[dst_entry[C.dst]];
        int ii = -1;
        for (int q = 0; q < D.n_in; ++q)
          if (D.in[q].et == C.edge_type) ii = q;
        Sx->out[Sx->n_out].d = dst_entry[C.dst];
        Sx->out[Sx->n_out].i = ii;
        ++Sx->n_out;
      }
    }
    HMP_HIP(hipMemcpy(Y.d_gat, &G, sizeof(G), hipMemcpyHostToDevice));
  }
  return HMP_OK;
}

// profiling helpers ------------------------------------------------------------------------------------
struct Scope {
  hmp_net* n;
  hipStream_t st;
  int idx = -1;
  Scope(hmp_net* n_, int cls, hipStream_t st_) : n(n_), st(st_) {
    if (!n->prof) return;
    ProfRec r;
    r.cls = cls;
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
    (void)hipEventRecord(r.a, st);
    n->recs.push_back(r);
    idx = (int)n->recs.size() - 1;
  }
  ~Scope() {
    if (idx >= 0) (void)hipEventRecord(n->recs[idx].b, st);
  }
};

// profile classes (hmp_net_profile_read); slot 13 (chain) is retired and always 0
enum { KC_PLAN = 0, KC_PACK, KC_GEMM_FWD, KC_AGG_FWD, KC_LOSS, KC_AGG_BWD, KC_GEMM_BWD, KC_GRAD_REDUCE, KC_ADAM, KC_GAT_FWD, KC_GAT_BWD, KC_POOL, KC_FRONT };

DropCfg make_drop(const hmp_net* n, float p, uint32_t stream) {
  DropCfg d;
  d.k0 = (uint32_t)n->seed; d.k1 = (uint32_t)(n->seed >> 32);
  d.step = n->rng_step; d.stream = stream;
  d.thresh = drop_thresh(p); d.scale = 1.f / (1.f - p);
  d.step_dev = n->call.d_step;
  return d;
}

GatDyn make_gat_dyn(const hmp_net* n, const hmp_batch* b) {
  GatDyn d;
  memset(&d, 0, sizeof(d));
  for (int t = 0; t < n->T; ++t) d.n_nodes[t] = b->n_nodes[t];
  for (int e = 0; e < n->ET; ++e) { d.n_edges[e] = b->n_edges[e]; d.edge_attr[e] = b->d_edge_attr[e]; }
  d.training = n->training;
  d.k0 = (uint32_t)n->seed; d.k1 = (uint32_t)(n->seed >> 32);
  d.step = n->rng_step;
  d.step_dev = n->call.d_step;
  return d;
}

int check_batch(const hmp_net* n, const hmp_batch* b) {
  HMP_CHECK_ARG(n->bound, "net: workspace not bound (call hmp_net_bind_workspace)");
  const hmp_net_spec& S = n->spec;
  for (int t = 0; t < n->T; ++t) {
    HMP_CHECK_ARG(b->n_nodes[t] >= 0 && b->n_nodes[t] <= n->cap_nodes[t], "batch: node type %d has %d nodes, capacity %d", t, b->n_nodes[t], n->cap_nodes[t]);
    const bool reads_x = n->lay[0].ncols[t] > 0 || (n->pass0[t] && n->lay[1].ncols[t] > 0);
    if (reads_x && b->n_nodes[t] > 0)
      HMP_CHECK_ARG(b->d_x[t] != nullptr && b->ldx[t] >= n->dim[0][t], "batch: node type %d features missing or ld < %d", t, n->dim[0][t]);
  }
  for (int e = 0; e < n->ET; ++e) {
    HMP_CHECK_ARG(b->n_edges[e] >= 0 && b->n_edges[e] <= n->cap_edges[e], "batch: edge type %d has %lld edges, capacity %lld", e, (long long)b->n_edges[e], (long long)n->cap_edges[e]);
    HMP_CHECK_ARG(b->n_edges[e] == 0 || b->d_edge_index[e] != nullptr, "batch: edge type %d edge_index missing", e);
  }
  for (int l = 0; l < n->L; ++l) {
    const LayerLayout& Y = n->lay[l];
    for (int i = 0; i < Y.n_live; ++i) {
      const hmp_conv_spec& C = S.layers[l].convs[Y.live[i]];
      if (C.kind == HMP_CONV_GAT && C.edge_dim > 0 && b->n_edges[C.edge_type] > 0)
        HMP_CHECK_ARG(b->d_edge_attr[C.edge_type] != nullptr, "batch: edge type %d needs edge_attr [E, %d]", C.edge_type, C.edge_dim);
    }
  }
  const int n_out_expect = S.pool_edge_type >= 0 ? b->n_nodes[S.edge_dst[S.pool_edge_type]] : b->n_nodes[S.readout_type];
  HMP_CHECK_ARG(b->n_out == n_out_expect, "batch: n_out %d != %d", b->n_out, n_out_expect);
  return HMP_OK;
}

// ---- forward -------------------------------------------------------------------------------------------
void fill_plan_batch(hmp_net* n, const hmp_batch* b, PlanBatch& pb) {
  memset(&pb, 0, sizeof(pb));
  pb.n = n->ET;
  pb.need_tpos = n->any_gat ? 1 : 0;
  pb.clear_first = 0;  // counters were zeroed at bind time and every build leaves them zero
  for (int e = 0; e < n->ET; ++e) {
    PlanJob& J = pb.j[e];
    J.degf = n->degf[e];
    hmp_plan& P = n->plan[e];
    P.n_src = b->n_nodes[n->spec.edge_src[e]];
    P.n_dst = b->n_nodes[n->spec.edge_dst[e]];
    P.n_edges = b->n_edges[e];
    J.ei = b->d_edge_index[e];
    J.E = P.n_edges; J.n_src = P.n_src; J.n_dst = P.n_dst;
    J.rowptr = P.d_rowptr; J.col = P.d_col; J.eid = P.d_eid;
    J.t_rowptr = P.d_t_rowptr; J.t_col = P.d_t_col; J.t_pos = P.d_t_pos;
    {  // graph-sorted edge list vouched for by the caller (hmp_batch::d_edge_ptr)
      const int ts = n->spec.edge_src[e], td = n->spec.edge_dst[e];
      const bool on = n->env.plan_sliced;
      if (on && b->n_graphs > 0 && b->d_edge_ptr[e] && b->d_node_ptr[ts] && b->d_node_ptr[td]) {
        J.gp_edge = b->d_edge_ptr[e]; J.gp_src = b->d_node_ptr[ts]; J.gp_dst = b->d_node_ptr[td]; J.n_graphs = b->n_graphs;
      }
    }
    plan_carve(J, n->plan_scratch[e]);
  }
}

int run_plan(hmp_net* n, const hmp_batch* b, hipStream_t st) {
  Scope sc(n, KC_PLAN, st);
  PlanBatch pb;
  fill_plan_batch(n, b, pb);
  return plan_launch(pb, &n->d_state->status, st);
}

// Small (launch-latency-bound) batches (<= 65 536 nodes): the row-local GEMM that follows an aggregation (next layer's projection in the
// forward pass, the input gradient in the backward pass) runs inside the aggregation kernel on 16-row tiles.  Large
// batches keep the stand-alone 64x64-tile GEMM (16-row tiles would re-read the weights from L2 once per 16 rows).
inline bool fuse_small(const hmp_net* n, const hmp_batch* b) {
  if (n->any_agg_first) return false;  // aggregate-first convs exist in the stand-alone launch sequence only (a large-batch choice)
  if (n->fuse_mode >= 0) return n->fuse_mode == 1;
  int64_t total = 0;
  for (int t = 0; t < n->T; ++t) total += b->n_nodes[t];
  // measured crossover on MI355X (tools/fuse_sweep.py, profiles/r02_fuse_sweep.json: config-2 network, hidden 64, batch 32 .. 2048):
  // the small-batch sequence wins up to ~46 000 nodes (batch 512: 0.578 vs 0.586 ms) and loses from ~95 000 on (batch 1024:
  // 1.085 vs 1.016 ms).  What it pays is the stacked weights re-read from L2 once per 16-row tile: that crossover holds for
  // stacked operands of the hidden-64 class (<= 64 KB); wider layers keep round 1's 16 384 (config 4, hidden 128: fused
  // 0.455 ms against 0.634 ms stand-alone at ~10 000 nodes; hidden 256 is the bf16 regime's territory above that).
  int64_t wmax = 1;
  for (int l = 1; l < n->L; ++l)
    for (int t = 0; t < n->T; ++t) {
      const int64_t wb = (int64_t)n->lay[l].ncols[t] * n->lay[l].ldw[t] * 4;
      wmax = wb > wmax ? wb : wmax;
    }
  return total <= (wmax <= 65536 ? 65536 : 16384);
}

inline bool is_input(const hmp_net* n, int l, int t) { return l == 0 || (l == 1 && n->pass0[t]); }
const float* h_ptr(const hmp_net* n, int l, int t) { return is_input(n, l, t) ? n->batch.d_x[t] : n->H[l][t]; }
int h_ld(const hmp_net* n, int l, int t) { return is_input(n, l, t) ? n->batch.ldx[t] : n->ld[l][t]; }

// bf16 compute mode: only the throughput-bound regime (>= 1024 64x64 tiles in the call) leaves the exact fp32 kernel
// HMP_BF16_ALL=1 (tests): every GEMM call of a bf16-mode net takes the bf16 kernel whatever its size, so that a graph the
// float64 oracle can hold (4 x 10^4 objects) runs exactly the decisions of the 10^6-object regime (BASELINE config 5)
bool gemm_takes_bf16(const hmp_net* n, const std::vector<GemmProblem>& ps) {
  const bool allow_bf16 = n->compute_bf16 != 0;
  if (allow_bf16 && n->env.bf16_all) return true;
  int64_t tiles64 = 0;
  double work = 0.0;
  for (const GemmProblem& p : ps) {
    tiles64 += (int64_t)cdiv(p.M, 64) * cdiv(p.N, 64);
    work += (double)p.M * p.N * p.K;
  }
  return allow_bf16 && (tiles64 >= 1024 || work >= 1e9);
}

// launches a list of GEMM problems in groups of GEMM_MAX_PROB; ksplit_out receives the split of each problem
int gemm_many(const hmp_net* n, std::vector<GemmProblem>& ps, bool want_split, hipStream_t st, std::vector<int>* ksplit_out) {
  bool bf16 = gemm_takes_bf16(n, ps);
  for (const GemmProblem& p : ps)
    if (p.a_bf16 || p.c_bf16 || p.b_bf16 || p.h_bf16) {  // bf16-stored operands exist only for the bf16 kernel
      HMP_CHECK_ARG(n->compute_bf16 != 0, "net: bf16-stored GEMM operand outside bf16 compute mode");
      bf16 = true;
    }
  for (size_t base = 0; base < ps.size(); base += GEMM_MAX_PROB) {
    GemmBatch gb;
    memset(&gb, 0, sizeof(gb));
    const size_t cnt = (ps.size() - base) < (size_t)GEMM_MAX_PROB ? (ps.size() - base) : (size_t)GEMM_MAX_PROB;
    for (size_t i = 0; i < cnt; ++i) gb.p[gb.n++] = ps[base + i];
    if (bf16) HMP_TRY(gemm_bf16_launch(gb, want_split, MAX_SLABS, st));
    else HMP_TRY(gemm_launch(gb, want_split, 64, st));
    if (ksplit_out)
      for (size_t i = 0; i < cnt; ++i) ksplit_out->push_back(gb.p[i].ksplit);
  }
  return HMP_OK;
}

// bf16 compute mode: layer j's aggregation (forward) and transposed aggregation (backward) take the one-wavefront-per-row shape
// that reads bf16 rows -- a SAGE layer outside the small-batch sequence whose every written node type is (128, 256] wide
bool rows_kernel_bf16(const hmp_net* n, const hmp_batch* b, int j) {
  const LayerLayout& Y = n->lay[j];
  if (Y.kind == HMP_CONV_GAT || n->fuse_now || !n->env.z16) return false;
  for (int t = 0; t < n->T; ++t) {
    if (Y.roff[t] < 0 || b->n_nodes[t] == 0) continue;
    const int f = fpad(n->spec.layers[j].out_dim[t]);
    if (f <= 128 || f > 256) return false;
  }
  return true;
}

void fill_plan_batch(hmp_net* n, const hmp_batch* b, PlanBatch& pb);

// Front kernel arguments (layer-0 projection + plan + pack in one launch); false when the batch / network does not fit its
// limits (the caller then launches pack, projection and plan separately).
bool build_front(hmp_net* n, const hmp_batch* b, const float* d_params, FrontArgs& fa) {
  if (!n->env.front || !n->d_pack_map) return false;
  const hmp_net_spec& S = n->spec;
  const hmp_layer_spec& Ls = S.layers[0];
  const LayerLayout& Y = n->lay[0];
  // GAT layers: the projection's operand is the pack's OUTPUT (att . W rows), so only plan and pack share the launch (the plan,
  // 19 us at config 3, runs behind the 46 us pack); the link pass (t_pos) follows as its own launch
  const bool proj = Y.kind == HMP_CONV_SAGE && !n->any_gat;
  memset(&fa, 0, sizeof(fa));
  // ---- projection problems
  for (int s = 0; s < n->T && proj; ++s) {
    if (Y.ncols[s] == 0 || b->n_nodes[s] == 0) continue;
    if (fa.n_prob == FR_MAX_PROB) return false;
    FrontProb& P = fa.prob[fa.n_prob++];
    P.A = b->d_x[s]; P.lda = b->ldx[s];
    P.C = n->Z[0][s]; P.ldc = Y.ncols[s];
    P.M = b->n_nodes[s]; P.N = Y.ncols[s]; P.K = n->dim[0][s];
    if (P.K < 4 || P.K > 384 || (P.K & 1) || (P.lda & 1) || (reinterpret_cast<uintptr_t>(P.A) & 7)) return false;
    for (int i = 0; i < Y.n_live; ++i) {
      const int c = Y.live[i];
      const hmp_conv_spec& C = Ls.convs[c];
      if (C.src != s) continue;
      if (P.n_seg == FR_MAX_SEG) return false;
      FrontSeg& G = P.seg[P.n_seg++];
      G.col0 = Y.conv[c].coff; G.rows = C.f_out; G.nsrc = 1; G.ld = P.K;
      G.off[0] = (uint32_t)C.w0;
    }
    if (Y.roff[s] >= 0) {
      if (P.n_seg == FR_MAX_SEG) return false;
      FrontSeg& G = P.seg[P.n_seg++];
      G.col0 = Y.roff[s]; G.rows = Ls.out_dim[s]; G.nsrc = 0; G.ld = P.K;
      for (int i = 0; i < Y.n_live; ++i) {
        const hmp_conv_spec& C = Ls.convs[Y.live[i]];
        if (C.dst != s) continue;
        if (G.nsrc == FR_MAX_SRC) return false;
        G.off[G.nsrc++] = (uint32_t)C.w1;
      }
      if (G.nsrc == 0) return false;
    }
  }
  if ((proj && fa.n_prob == 0) || S.n_params >= ((int64_t)1 << 31)) return false;
  // ---- plan parts
  PlanBatch pb;
  fill_plan_batch(n, b, pb);
  int64_t E = 0;
  for (int e = 0; e < pb.n; ++e) E += pb.j[e].E;
  if (E > PS_MAX_EDGES) return false;
  fa.n_jobs = pb.n;
  fa.need_tpos = pb.need_tpos;
  fa.plan_rc = plan_small_fits_rc(pb) ? 1 : 0;
  fa.plan_blocks = plan_small_layout(pb, fa.part_start, fa.rows_per_part);
  if (n->reuse_plan) fa.plan_blocks = 0;  // same topology as the previous call: no plan role in this launch
  fa.ws = n->ws_base;
  auto woff = [&](const void* p) -> uint32_t { return (uint32_t)((reinterpret_cast<const char*>(p) - n->ws_base) >> 2); };
  if (n->ws_bytes >= ((size_t)1 << 34)) return false;  // 32-bit word offsets
  for (int e = 0; e < pb.n; ++e) {
    const PlanJob& J = pb.j[e];
    FrontJob& F = fa.job[e];
    F.ei = J.ei; F.E = (int)J.E; F.n_src = J.n_src; F.n_dst = J.n_dst;
    F.rowptr = woff(J.rowptr); F.col = woff(J.col); F.eid = woff(J.eid);
    F.t_rowptr = woff(J.t_rowptr); F.t_col = woff(J.t_col); F.t_eid = woff(J.t_eid);
    F.tmp_in = woff(J.tmp_in); F.tmp_out = woff(J.tmp_out); F.pos_of_eid = woff(J.pos_of_eid); F.degf = woff(J.degf); F.flags = woff(J.flags);
    F.gp_dst = J.gp_dst; F.gp_src = J.gp_src; F.gp_edge = J.gp_edge; F.n_graphs = J.n_graphs;
  }
  fa.status = &n->d_state->status;
  // ---- pack blocks
  fa.params = d_params;
  fa.segs = n->d_pack_segs;
  fa.pack_map = n->d_pack_map;
  fa.pack_blocks = n->n_pack_blocks16;
  fa.packed = n->d_packed;
  fa.step_ctr = n->call.d_step;
  fa.step_mirror = &n->d_state->last_step;
  return true;
}

int forward_impl(hmp_net* n, const hmp_batch* b, const float* d_params, hipStream_t st) {
  HMP_TRY(check_batch(n, b));
  const hmp_net_spec& S = n->spec;
  if (b->plan_valid) {
    HMP_CHECK_ARG(n->plan_ok, "batch: plan_valid without a plan from a previous call (first call, or the workspace was re-bound)");
    for (int e = 0; e < n->ET; ++e)
      HMP_CHECK_ARG(n->plan[e].n_edges == b->n_edges[e] && n->plan[e].n_src == b->n_nodes[S.edge_src[e]] && n->plan[e].n_dst == b->n_nodes[S.edge_dst[e]],
                    "batch: plan_valid but edge type %d changed shape since the previous call", e);
  }
  // the batch is accepted: from here on this is the last forward (a refused batch leaves the previous one's state to its backward)
  n->batch = *b;
  n->training = n->call.training; n->seed = n->call.seed; n->rng_step = n->call.rng_step;
  n->reuse_plan = b->plan_valid != 0;
  n->fuse_now = fuse_small(n, b);
  memset(n->h16, 0, sizeof(n->h16));
  // Small batches, SAGE layer 0: projection (reading the stacked weights straight from the flat parameters), plan and pack
  // are roles of ONE launch (front.hip) -- the plan, which has to read whole edge lists through single CUs, hides behind
  // the projection tiles.
  FrontArgs fa;
  const bool front = n->fuse_now && build_front(n, b, d_params, fa);
  if (front) {
    Scope sc(n, KC_FRONT, st);
    HMP_TRY(front_launch(fa, st));
    if (fa.need_tpos && fa.plan_blocks > 0) {
      PlanBatch pb;
      fill_plan_batch(n, b, pb);
      HMP_TRY(plan_link_launch(pb, st));
    }
    for (int e = 0; e < n->ET; ++e) {  // what run_plan records on the host
      hmp_plan& P = n->plan[e];
      P.n_src = b->n_nodes[S.edge_src[e]]; P.n_dst = b->n_nodes[S.edge_dst[e]]; P.n_edges = b->n_edges[e];
    }
  } else {
    Scope sc(n, KC_PACK, st);
    HMP_TRY(pack_launch(n->d_pack_segs, n->pack_sb, d_params, n->d_packed, n->call.d_step, &n->d_state->last_step, st));
  }
  bool z_done = false;
  for (int l = 0; l < n->L; ++l) {
    const hmp_layer_spec& Ls = S.layers[l];
    LayerLayout& Y = n->lay[l];
    bool z16 = false;  // this layer's projected rows are stored as bf16 (decided with the projection, read by the aggregation)
    if (l == 0 && !front && n->any_agg_first && !n->reuse_plan) HMP_TRY(run_plan(n, b, st));  // the segment means of layer 0 read the plan
    if (l == 0 && front && fa.n_prob > 0) {
      // projection, plan and pack already ran in the front kernel
    } else if (!z_done) {  // grouped projection (skipped when the previous layer's aggregation kernel already produced Z[l])
      Scope sc(n, KC_GEMM_FWD, st);
      std::vector<GemmProblem> ps;
      for (int s = 0; s < n->T; ++s) {
        if (Y.ncols[s] == 0 || b->n_nodes[s] == 0) continue;
        GemmProblem p;
        memset(&p, 0, sizeof(p));
        p.A = h_ptr(n, l, s); p.lda = h_ld(n, l, s); p.trans_a = 0;
        p.a_bf16 = n->h16[l][s] ? 1 : 0;
        p.B = n->d_packed + Y.wp_off[s]; p.ldb = Y.ldw[s]; p.trans_b = 1;
        p.C = n->Z[l][s]; p.ldc = Y.ncols[s];
        p.M = b->n_nodes[s]; p.N = Y.ncols[s]; p.K = n->dim[l][s];
        p.n_real = p.N;
        p.epi = EPI_NONE;
        ps.push_back(p);
      }
      // bf16 compute mode, 10^6-row regime: the projected rows are only ever gathered by this layer's aggregation, so they are
      // stored as bf16 (half the projection's write and half the gather's read traffic) -- when the bf16 GEMM runs AND the
      // aggregation reads bf16 rows
      if (rows_kernel_bf16(n, b, l) && gemm_takes_bf16(n, ps)) {
        z16 = true;
        for (GemmProblem& p : ps) z16 = z16 && (p.ldc & 3) == 0;
        if (z16)
          for (GemmProblem& p : ps) p.c_bf16 = 1;
      }
      HMP_TRY(gemm_many(n, ps, false, st, nullptr));
    }
    if (n->any_agg_first && !z_done) {
      // aggregate-first convs: mean of the SOURCE rows per destination row, then the destination-sized projection into the conv's
      // block of Z[l][dst] -- a second launch: the main one wrote that block too (zero weights there)
      std::vector<GemmProblem> pa;
      for (int i = 0; i < Y.n_live; ++i) {
        const int c = Y.live[i];
        const ConvLayout& Q = Y.conv[c];
        if (!Q.agg_first) continue;
        const hmp_conv_spec& C = Ls.convs[c];
        if (b->n_nodes[C.dst] == 0 || b->n_nodes[C.src] == 0 || b->n_edges[C.edge_type] == 0) continue;
        {
          Scope sa(n, KC_AGG_FWD, st);
          const hmp_plan& Pl = n->plan[C.edge_type];
          HMP_TRY(seg_mean_rows_launch(h_ptr(n, l, C.src), h_ld(n, l, C.src), n->h16[l][C.src] ? 1 : 0, n->dim[l][C.src], Pl.d_rowptr, Pl.d_col,
                                       b->n_nodes[C.dst], Q.mrows, Q.ld_m, st));
        }
        GemmProblem p;
        memset(&p, 0, sizeof(p));
        p.A = Q.mrows; p.lda = Q.ld_m; p.trans_a = 0;
        p.B = n->d_packed + Q.wc_off; p.ldb = Y.ldw[C.src]; p.trans_b = 1;
        p.C = z16 ? reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(n->Z[l][C.dst]) + Q.aoff) : n->Z[l][C.dst] + Q.aoff;
        p.c_bf16 = z16 ? 1 : 0;
        p.ldc = Y.ncols[C.dst];
        p.M = b->n_nodes[C.dst]; p.N = fpad(C.f_out); p.K = n->dim[l][C.src];
        p.n_real = p.N;
        p.epi = EPI_NONE;
        pa.push_back(p);
      }
      if (!pa.empty()) {
        Scope sg(n, KC_GEMM_FWD, st);
        HMP_TRY(gemm_many(n, pa, false, st, nullptr));
      }
    }
    z_done = false;
    if (l == 0 && !front && !n->reuse_plan && !n->any_agg_first) HMP_TRY(run_plan(n, b, st));
    if (Y.kind == HMP_CONV_GAT) {
      Scope sc(n, KC_GAT_FWD, st);
      GatDyn dyn = make_gat_dyn(n, b);
      HMP_TRY(gat_fwd_launch(Y.d_gat, Y.h_gat, dyn, st));
      continue;
    }
    {  // fused aggregation + root + bias + activation + dropout
      Scope sc(n, KC_AGG_FWD, st);
      AggArgs a;
      memset(&a, 0, sizeof(a));
      a.mean = 1;
      a.state = n->d_state;
      // two-headed step: both heads' tail (act, dropout) and masked CE in this epilogue when it can hold both rows' widths
      const bool tail_epi = l == n->L - 1 && n->call.tgt && !n->has_pools && n->fuse_now && fpad(Ls.out_dim[S.readout_type]) <= 256 &&
                            fpad(Ls.out_dim[S.aux_readout_type]) <= 256;
      for (int t = 0; t < n->T; ++t) {
        if (Y.roff[t] < 0 || b->n_nodes[t] == 0) continue;
        AggDst& D = a.d[a.n++];
        if (l == n->L - 1 && t == S.readout_type && n->call.ce_labels && S.pool_edge_type < 0 && n->fuse_now && fpad(Ls.out_dim[t]) <= 256) {
          // masked cross entropy in the epilogue of the last aggregation (one kernel less on the step's critical path)
          D.ce_labels = n->call.ce_labels; D.ce_ignored = n->call.ce_ignored; D.ce_classes = n->out_dim;
          D.ce_grad = n->d_gout; D.ce_ldg = n->out_ld; D.ce_row_lv = n->d_row_lv;
          D.ce_weight = n->class_w[0];
          n->call.ce_done = true;
        }
        D.n_rows = b->n_nodes[t];
        D.F = fpad(Ls.out_dim[t]);
        D.out = n->H[l + 1][t]; D.ldo = n->ld[l + 1][t];
        D.zroot = n->Z[l][t]; D.ldzr = Y.ncols[t]; D.roff = Y.roff[t];
        D.bias = n->d_packed + Y.bias_off[t];
        D.act = Ls.act;
        D.drop_on = (n->training && Ls.dropout > 0.f) ? 1 : 0;
        if (D.drop_on) D.drop = make_drop(n, Ls.dropout, (uint32_t)(l * HMP_MAX_NODE_TYPES + t));
        const int head = t == S.readout_type ? 0 : (t == S.aux_readout_type ? 1 : -1);
        if (tail_epi && head >= 0) {
          // the layer runs with the model's tail: its pitch numbering of the keep-mask, row * (ldo / 4) + col / 4, is the tail's
          // row * ceil(out_dim / 4) + col / 4 (ldo = fpad(out_dim)), on the tail's tensor id 8 * (L - 1) + t
          D.act = S.tail_act;
          D.drop_on = (n->training && S.tail_dropout > 0.f) ? 1 : 0;
          if (D.drop_on) D.drop = make_drop(n, S.tail_dropout, (uint32_t)(l * HMP_MAX_NODE_TYPES + t));
          D.ce_labels = n->call.tgt->d_labels[head]; D.ce_mask = n->call.tgt->d_mask[head]; D.ce_tail = 1;
          D.ce_weight = n->class_w[head];
          D.ce_ignored = n->call.ce_ignored; D.ce_classes = Ls.out_dim[t];
          D.ce_grad = head == 0 ? n->d_gout : n->G[n->L][t];
          D.ce_ldg = head == 0 ? n->out_ld : n->ld[n->L][t];
          D.ce_row_lv = n->d_row_lv + (head == 0 ? 0 : 2 * (int64_t)b->n_out);
          n->call.tail_done[head] = true;
        }
        for (int i = 0; i < Y.n_live; ++i) {
          const int c = Y.live[i];
          const hmp_conv_spec& C = Ls.convs[c];
          if (C.dst != t) continue;
          if (b->n_nodes[C.src] == 0 || b->n_edges[C.edge_type] == 0) continue;
          AggIn& I = D.in[D.n_in++];
          if (Y.conv[c].agg_first) {  // the conv's block of this type's own Z, through identity lists (in-degree 1)
            I.rowptr = n->d_iota; I.col = n->d_iota;
            I.z = n->Z[l][t]; I.ldz = Y.ncols[t]; I.coff = Y.conv[c].aoff;
            I.same_type = 0; I.n_src = b->n_nodes[t];
            continue;
          }
          I.rowptr = n->plan[C.edge_type].d_rowptr;
          I.col = n->plan[C.edge_type].d_col;
          I.z = n->Z[l][C.src]; I.ldz = Y.ncols[C.src]; I.coff = Y.conv[c].coff;
          I.same_type = C.src == C.dst ? 1 : 0;
          I.n_src = b->n_nodes[C.src];
          if (n->fuse_now && b->n_edges[C.edge_type] > (int64_t)8 * b->n_nodes[C.dst]) D.tile_rows = 8;  // average in-degree > 8
        }
      }
      // fuse the projection of layer l+1 when every node type it reads is produced right here
      bool fuse = n->fuse_now && l + 1 < n->L;
      if (fuse) {
        const LayerLayout& Yn = n->lay[l + 1];
        for (int t = 0; t < n->T && fuse; ++t) {
          if (Yn.ncols[t] == 0 || b->n_nodes[t] == 0) continue;
          if (Y.roff[t] < 0 || is_input(n, l + 1, t)) fuse = false;                   // not produced by this launch
          if ((n->dim[l + 1][t] & 15) != 0 || n->dim[l + 1][t] > 256) fuse = false;  // kernel limits
        }
        for (int i = 0; i < a.n && fuse; ++i)
          if (a.d[i].F > 256) fuse = false;
      }
      if (fuse) {
        const LayerLayout& Yn = n->lay[l + 1];
        int ai = 0;
        for (int t = 0; t < n->T; ++t) {
          if (Y.roff[t] < 0 || b->n_nodes[t] == 0) continue;
          AggDst& D = a.d[ai++];
          if (Yn.ncols[t] == 0) continue;
          D.pw = n->d_packed + Yn.wp_off[t]; D.pldw = Yn.ldw[t]; D.pncols = Yn.ncols[t]; D.pK = n->dim[l + 1][t];
          D.pz = n->Z[l + 1][t]; D.pldz = Yn.ncols[t];
        }
        HMP_TRY(agg_proj_fwd_launch(a, st));
        z_done = true;
      } else {
        a.zb16 = z16 ? 1 : 0;
        // same regime: the activations H[l+1] of a hidden layer are read only by GEMMs of the bf16 kernel (next projection, its
        // weight gradient, the activation mask of its input gradient), which round them to bf16 on the way into LDS anyway --
        // written as bf16 here the results are bit-identical and every one of those reads, and this write, moves half the bytes.
        // Needs: every output of this launch exactly 256 wide (whole GEMM tiles), the next layer a SAGE layer whose three GEMMs
        // (same M x N x K products) take the bf16 kernel by their own size -- a bf16-stored operand would otherwise force a
        // narrow last-layer projection off the exact fp32 kernel (measured: 40 000 objects x 28 live columns)
        bool hb = z16 && l + 1 < n->L && n->lay[l + 1].kind != HMP_CONV_GAT;
        for (int i = 0; i < a.n && hb; ++i) hb = a.d[i].F == 256 && a.d[i].ldo == 256;
        if (hb) {
          double work = 0.0;
          for (int s = 0; s < n->T; ++s) work += (double)b->n_nodes[s] * n->lay[l + 1].ncols[s] * n->dim[l + 1][s];
          // an aggregate-first conv of the next layer reads its source rows with the segment-mean kernels (both storage forms):
          // counted as the projection it stands for, so that the choice does not depend on the order of evaluation
          for (int i = 0; i < n->lay[l + 1].n_live; ++i) {
            const int c = n->lay[l + 1].live[i];
            if (!n->lay[l + 1].conv[c].agg_first) continue;
            const hmp_conv_spec& C = S.layers[l + 1].convs[c];
            work += (double)b->n_nodes[C.src] * fpad(C.f_out) * n->dim[l + 1][C.src];
          }
          hb = work >= 1e9 || n->env.bf16_all;  // gemm_takes_bf16's work criterion
        }
        if (!n->env.h16) hb = false;
        if (hb) {
          a.hb16 = 1;
          for (int t = 0; t < n->T; ++t)
            if (Y.roff[t] >= 0 && b->n_nodes[t] > 0) n->h16[l + 1][t] = true;
        }
        HMP_TRY(agg_fwd_launch(a, st));
      }
    }
  }
  if (S.pool_edge_type >= 0) {
    Scope sc(n, KC_POOL, st);
    const int rt = S.readout_type;
    HMP_TRY(hmp_segment_mean_fwd(n->H[n->L][rt], n->ld[n->L][rt], n->out_ld, n->plan[S.pool_edge_type], n->d_out, n->out_ld, st));
  }
  n->have_fwd = true;
  n->plan_ok = true;
  return HMP_OK;
}

const float* out_ptr(const hmp_net* n) {
  return n->spec.pool_edge_type >= 0 ? n->d_out : n->H[n->L][n->spec.readout_type];
}

// ---- backward ------------------------------------------------------------------------------------------
// skip_w (the input-gradient entry): the weight-gradient problems, their launch and the gradient un-pack are left out -- only the
// chain down to d_gx runs, d_grads is not touched and may be null.  Every other caller's launches are what they were.
int backward_impl(hmp_net* n, const float* d_gout, int ld_gout, float* d_grads, const float* d_params, float* const* d_gx,
                  hipStream_t st, const float* d_gaux = nullptr, int ld_gaux = 0, bool skip_w = false) {
  HMP_CHECK_ARG(n->have_fwd, "net: backward without a forward");
  if (const int at = n->spec.aux_readout_type; at >= 0) {
    // second readout: stage its gradient in G[L][aux] (zero where the caller passed none, and in the padding columns)
    const int rows = n->batch.n_nodes[at], ld = n->ld[n->L][at], w = n->dim[n->L][at];
    HMP_CHECK_ARG(!d_gaux || ld_gaux >= w, "net: second output gradient narrower than the output (%d < %d)", ld_gaux, w);
    if (rows > 0 && !n->call.aux_g_ready) {
      HMP_HIP(hipMemsetAsync(n->G[n->L][at], 0, (size_t)rows * ld * 4, st));
      if (d_gaux)
        HMP_HIP(hipMemcpy2DAsync(n->G[n->L][at], (size_t)ld * 4, d_gaux, (size_t)ld_gaux * 4, (size_t)w * 4, rows, hipMemcpyDeviceToDevice, st));
    }
  } else {
    HMP_CHECK_ARG(!d_gaux, "net: a second output gradient for a net without aux_readout_type");
  }
  HMP_CHECK_ARG((ld_gout & 3) == 0 && ld_gout >= n->out_ld && (reinterpret_cast<uintptr_t>(d_gout) & 15) == 0,
                "net: output gradient must be 16-byte aligned with ld %% 4 == 0 and ld >= %d", n->out_ld);
  const hmp_net_spec& S = n->spec;
  const hmp_batch* b = &n->batch;
  const int rt = S.readout_type;
  const float* gtop = d_gout;
  int ld_gtop = ld_gout;
  if (S.pool_edge_type >= 0) {
    Scope sc(n, KC_POOL, st);
    HMP_TRY(hmp_segment_mean_bwd(d_gout, ld_gout, n->out_ld, n->plan[S.pool_edge_type], n->G[n->L][rt], n->ld[n->L][rt], st));
    gtop = n->G[n->L][rt];
    ld_gtop = n->ld[n->L][rt];
  }
  memset(&n->dyn, 0, sizeof(n->dyn));
  if (n->call.head_blocks > 0) {  // linear heads: the head kernel's workgroup slabs (rows past the heads' write nothing: 0)
    n->dyn.n_slabs[HEAD_SLAB_ID] = (unsigned char)n->call.head_blocks;
    n->dyn.slab_stride[HEAD_SLAB_ID] = (int)n->head_slab_stride;
  }
  std::vector<GemmProblem> wps;  // weight-gradient problems of all layers (one launch after the loop)
  std::vector<int> wids;
  bool fin_early = false;
  bool g16[HMP_MAX_LAYERS + 2];  // g16[l]: the input gradients G[l][*] were stored as bf16 by layer l's input-gradient GEMM
  for (int i = 0; i < HMP_MAX_LAYERS + 2; ++i) g16[i] = false;
  bool dz16 = false;  // this layer's dZ is written as bf16 by the transposed aggregation (read by both backward GEMMs)
  bool pass_gx[HMP_MAX_NODE_TYPES] = {false};  // d_gx[t] already holds layer 1's share (passthrough types)
  for (int l = n->L - 1; l >= 0; --l) {
    const hmp_layer_spec& Ls = S.layers[l];
    LayerLayout& Y = n->lay[l];
    auto g_of = [&](int t, int& ldg) -> const float* {
      if (l == n->L - 1 && t == rt) { ldg = ld_gtop; return gtop; }
      ldg = n->ld[l + 1][t];
      return n->G[l + 1][t];
    };
    bool dx_fused = false;
    bool rootless = false;  // this layer's GEMMs take the root block of dZ from the output gradient
    dz16 = false;
    if (Y.kind == HMP_CONV_GAT) {
      Scope sc(n, KC_GAT_BWD, st);
      GatDyn dyn = make_gat_dyn(n, b);
      dyn.g_top = gtop; dyn.ld_gtop = ld_gtop;
      HMP_TRY(gat_bwd1_launch(Y.d_gat, Y.h_gat, dyn, st));
      HMP_TRY(gat_bwd2_launch(Y.d_gat, Y.h_gat, dyn, st));
    } else {  // transposed aggregation: gradient of the projected rows
      Scope sc(n, KC_AGG_BWD, st);
      TAggArgs a;
      memset(&a, 0, sizeof(a));
      a.mean = 1;
      if (n->call.fin_loss) {  // first backward kernel of the step: one extra block finalises {loss_sum, count}
        a.fin_row_lv = n->d_row_lv; a.fin_rows = n->call.fin_rows > 0 ? n->call.fin_rows : b->n_out; a.fin_out2 = d_grads + n->spec.n_active_params; a.fin_state = n->d_state;
        n->call.fin_loss = false;
        fin_early = true;
      }
      for (int s = 0; s < n->T; ++s) {
        if (Y.ncols[s] == 0 || b->n_nodes[s] == 0) continue;
        TAggSrc& T = a.s[a.n++];
        T.n_rows = b->n_nodes[s];
        T.dz = n->dZ[l][s]; T.lddz = Y.ncols[s]; T.ncols = Y.ncols[s];
        if (Y.roff[s] >= 0) {
          int ldg;
          T.groot = g_of(s, ldg);
          T.ldgr = ldg; T.roff = Y.roff[s]; T.Froot = fpad(Ls.out_dim[s]);
        }
        for (int i = 0; i < Y.n_live; ++i) {
          const int c = Y.live[i];
          const hmp_conv_spec& C = Ls.convs[c];
          if (Y.conv[c].agg_first) {  // its block of dZ[l][dst] = the destination's own output gradient (identity lists, weight 1)
            if (C.dst != s || b->n_nodes[C.src] == 0 || b->n_edges[C.edge_type] == 0) continue;
            TAggOut& O = T.out[T.n_out++];
            O.t_rowptr = n->d_iota; O.t_col = n->d_iota; O.rowptr = n->d_iota; O.degf = n->d_ones;
            int ldg;
            O.g = g_of(s, ldg);
            O.ldg = ldg; O.coff = Y.conv[c].aoff; O.F = fpad(C.f_out);
            O.same_type = 0; O.n_dst = b->n_nodes[s];
            continue;
          }
          if (C.src != s) continue;
          TAggOut& O = T.out[T.n_out++];
          const hmp_plan& P = n->plan[C.edge_type];
          O.t_rowptr = P.d_t_rowptr; O.t_col = P.d_t_col; O.rowptr = P.d_rowptr; O.degf = n->degf[C.edge_type];
          int ldg;
          O.g = g_of(C.dst, ldg);
          O.ldg = ldg; O.coff = Y.conv[c].coff; O.F = fpad(C.f_out);
          O.same_type = C.src == C.dst ? 1 : 0;
          O.n_dst = b->n_nodes[C.dst];
          if (n->fuse_now && b->n_edges[C.edge_type] > (int64_t)8 * b->n_nodes[C.src]) T.tile_rows = 8;  // average out-degree > 8
        }
      }
      // input gradient of layer l inside the same kernel (row-local GEMM on 16-row tiles) for small batches
      dx_fused = n->fuse_now && l > 0;
      int fmax = 0;
      for (int i = 0; i < a.n && dx_fused; ++i) {
        if (a.s[i].ncols > 896) dx_fused = false;
        for (int o = 0; o < a.s[i].n_out; ++o) fmax = a.s[i].out[o].F > fmax ? a.s[i].out[o].F : fmax;
        if (a.s[i].groot) fmax = a.s[i].Froot > fmax ? a.s[i].Froot : fmax;
      }
      if (fmax > 256) dx_fused = false;
      if (dx_fused) {
        const hmp_layer_spec& Lp = S.layers[l - 1];
        int ai = 0;
        for (int s = 0; s < n->T; ++s) {
          if (Y.ncols[s] == 0 || b->n_nodes[s] == 0) continue;
          TAggSrc& T = a.s[ai++];
          if (!n->G[l][s]) continue;  // passthrough input of layer 1: no gradient wanted
          HMP_CHECK_ARG(Y.ldt[s] > 0, "net: layer %d type %d has no transposed weight image for the fused input gradient", l, s);
          T.xwt = n->d_packed + Y.wpt_off[s]; T.xldt = Y.ldt[s]; T.xN = n->dim[l][s];
          T.xg = n->G[l][s]; T.xldg = n->ld[l][s];
          T.xdrop_on = (n->training && Lp.dropout > 0.f) ? 1 : 0;
          T.xact = Lp.act;
          T.xscale = T.xdrop_on ? 1.f / (1.f - Lp.dropout) : 1.f;
          T.xh = (T.xact != HMP_ACT_NONE || T.xdrop_on) ? n->H[l][s] : nullptr;
          T.xldh = n->ld[l][s];
        }
        HMP_TRY(agg_bwd_dx_launch(a, st));
      } else {
        a.gb16 = g16[l + 1] ? 1 : 0;
        // dZ as bf16 too (it is only read back as the A operand of the two backward GEMMs): needs the bf16-reading kernel
        // above and whole 256-row tiles of every dZ^T (the bf16 operand loader has no edge path)
        dz16 = a.gb16 && n->compute_bf16 != 0;
        for (int s = 0; s < n->T && dz16; ++s)
          if (Y.ncols[s] > 0 && b->n_nodes[s] > 0 && (Y.ncols[s] % 256) != 0) dz16 = false;
        if (!n->env.z16) dz16 = false;
        a.dzb16 = dz16 ? 1 : 0;
        // the root block of dZ is a copy of the output gradient (d out / d z_root = 1): with both stored as bf16 and the block
        // on a 256-column boundary the two backward GEMMs read it where it is (GemmProblem::A2) and the copy -- 1 GB per layer
        // at 10^6 rows -- is not made
        rootless = dz16;
        for (int i = 0; i < a.n && rootless; ++i)
          if (a.s[i].groot && ((a.s[i].roff & 255) != 0 || a.s[i].Froot != 256 || (a.s[i].ldgr & 3) != 0)) rootless = false;
        if (n->env.rootcopy) rootless = false;
        if (rootless)
          for (int i = 0; i < a.n; ++i) a.s[i].groot = nullptr;
        HMP_TRY(agg_bwd_launch(a, st));
      }
    }
    const bool need_dx = !dx_fused && ((l > 0) || (d_gx != nullptr));
    // passthrough types (pre_mp): layer 1 reads their INPUT rows, so its share of d x goes to d_gx first -- layer 0 adds its own
    // on top (GemmProblem::Cadd below).  Only with d_gx: no other caller wants a gradient there (G[1][t] is null)
    if (l == 1 && d_gx) {
      std::vector<GemmProblem> ps;
      for (int s = 0; s < n->T; ++s) {
        if (!n->pass0[s] || !d_gx[s] || Y.ncols[s] == 0 || b->n_nodes[s] == 0) continue;
        GemmProblem p;
        memset(&p, 0, sizeof(p));
        p.A = n->dZ[l][s]; p.lda = Y.ncols[s]; p.trans_a = 0;
        p.a_bf16 = dz16 ? 1 : 0;
        p.B = n->d_packed + Y.wp_off[s]; p.ldb = Y.ldw[s]; p.trans_b = 0;
        p.C = d_gx[s]; p.ldc = b->ldx[s];
        p.M = b->n_nodes[s]; p.N = n->dim[l][s]; p.K = Y.ncols[s];
        p.n_real = p.N;
        p.epi = EPI_NONE;
        ps.push_back(p);
        pass_gx[s] = true;
      }
      if (!ps.empty()) {
        Scope sp(n, KC_GEMM_BWD, st);
        HMP_TRY(gemm_many(n, ps, false, st, nullptr));
      }
    }
    // aggregate-first convs: dM = dZ_block * W_l (destination-sized), ahead of the launch whose epilogue scatters it
    auto dz_at = [&](int t, int col) -> const float* {
      return dz16 ? reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(n->dZ[l][t]) + col) : n->dZ[l][t] + col;
    };
    auto aggf_live = [&](int c) {
      const hmp_conv_spec& C = Ls.convs[c];
      return Y.conv[c].agg_first && b->n_nodes[C.dst] > 0 && b->n_nodes[C.src] > 0 && b->n_edges[C.edge_type] > 0;
    };
    if (need_dx && n->any_agg_first) {
      std::vector<GemmProblem> pp;
      for (int i = 0; i < Y.n_live; ++i) {
        const int c = Y.live[i];
        if (!aggf_live(c)) continue;
        const hmp_conv_spec& C = Ls.convs[c];
        float* want = l > 0 ? n->G[l][C.src] : d_gx[C.src];
        if (!want) continue;
        const ConvLayout& Q = Y.conv[c];
        GemmProblem p;
        memset(&p, 0, sizeof(p));
        p.A = dz_at(C.dst, Q.aoff); p.lda = Y.ncols[C.dst]; p.trans_a = 0; p.a_bf16 = dz16 ? 1 : 0;
        p.B = n->d_packed + Q.wc_off; p.ldb = Y.ldw[C.src]; p.trans_b = 0;
        p.C = Q.dmrows; p.ldc = Q.ld_m;
        p.M = b->n_nodes[C.dst]; p.N = n->dim[l][C.src]; p.K = fpad(C.f_out);
        p.n_real = p.N;
        p.epi = EPI_NONE;
        pp.push_back(p);
      }
      if (!pp.empty()) {
        Scope sp(n, KC_GEMM_BWD, st);
        HMP_TRY(gemm_many(n, pp, false, st, nullptr));
      }
    }
    // the gradient the source rows of aggregate-first conv c receive: the segment mean's transpose of dM
    struct SrcTerm { int c; const hmp_plan* P; const float* degf; };
    auto src_term = [&](int s, SrcTerm& T) -> bool {
      const int c = Y.aggf_of_src[s];
      if (c < 0 || !aggf_live(c)) return false;
      T.c = c; T.P = &n->plan[Ls.convs[c].edge_type]; T.degf = n->degf[Ls.convs[c].edge_type];
      return true;
    };
    if (need_dx) {  // input gradient, masked by the previous layer's activation/dropout derivative
      Scope sc(n, KC_GEMM_BWD, st);
      std::vector<GemmProblem> ps;
      std::vector<int> ps_type;
      for (int s = 0; s < n->T; ++s) {
        if (Y.ncols[s] == 0 || b->n_nodes[s] == 0) continue;
        float* dst = l > 0 ? n->G[l][s] : d_gx[s];
        if (!dst) continue;
        GemmProblem p;
        memset(&p, 0, sizeof(p));
        p.A = n->dZ[l][s]; p.lda = Y.ncols[s]; p.trans_a = 0;
        p.a_bf16 = dz16 ? 1 : 0;
        if (rootless && Y.roff[s] >= 0) { int ldg; p.A2 = g_of(s, ldg); p.lda2 = ldg; p.a_split = Y.roff[s]; }
        p.B = n->d_packed + Y.wp_off[s]; p.ldb = Y.ldw[s]; p.trans_b = 0;
        p.C = dst; p.ldc = l > 0 ? n->ld[l][s] : b->ldx[s];
        p.M = b->n_nodes[s]; p.N = n->dim[l][s]; p.K = Y.ncols[s];
        p.n_real = p.N;
        if (l > 0) {
          const hmp_layer_spec& Lp = S.layers[l - 1];
          p.epi = EPI_ACTMASK;
          p.H = n->H[l][s]; p.ldh = n->ld[l][s]; p.act = Lp.act;
          p.h_bf16 = n->h16[l][s] ? 1 : 0;
          p.drop_on = (n->training && Lp.dropout > 0.f) ? 1 : 0;
          if (p.drop_on) p.drop = make_drop(n, Lp.dropout, (uint32_t)((l - 1) * HMP_MAX_NODE_TYPES + s));
          if (p.act == HMP_ACT_NONE && !p.drop_on) p.epi = EPI_NONE;
        } else if (pass_gx[s]) {
          p.Cadd = dst; p.ldadd = p.ldc;  // in place: a tile starts its sums from the elements it stores
        }
        ps.push_back(p);
        ps_type.push_back(s);
      }
      // bf16 compute mode, 10^6-row regime: G[l] is only ever gathered by layer l-1's transposed aggregation -> stored as bf16
      // when this GEMM runs on the bf16 kernel and that aggregation takes its one-wavefront-per-row shape (see forward_impl)
      // (a large source type whose gradient is the masked transpose alone -- no GEMM in this layer -- counts like the GEMM it replaces)
      bool big_alone = false;
      for (int s = 0; s < n->T; ++s) {
        SrcTerm T;
        if (Y.ncols[s] == 0 && b->n_nodes[s] >= 32768 && src_term(s, T)) big_alone = true;
      }
      if (l > 0 && rows_kernel_bf16(n, b, l - 1) && (gemm_takes_bf16(n, ps) || (n->compute_bf16 != 0 && big_alone))) {
        bool ok = true;
        for (GemmProblem& p : ps) ok = ok && (p.ldc & 3) == 0;
        if (ok) {
          for (GemmProblem& p : ps) p.c_bf16 = 1;
          g16[l] = true;
        }
      }
      // source types of aggregate-first convs: + transpose of the segment mean, before the mask.  Fused into the epilogue of the
      // weight-stationary kernel where that one runs the problem; else as an fp32 matrix the tiled kernels start their sums from
      int64_t sadd_used = 0;
      for (size_t i = 0; i < ps.size(); ++i) {
        SrcTerm T;
        if (!src_term(ps_type[i], T)) continue;
        const ConvLayout& Q = Y.conv[T.c];
        HMP_TRY(gemm_dx_gather_term(ps[i], n->compute_bf16 != 0, T.P->d_t_rowptr, T.P->d_t_col, T.degf, Q.dmrows, Q.ld_m, n->d_sadd,
                                    n->sadd_floats, &sadd_used, st));
      }
      if (!ps.empty()) HMP_TRY(gemm_many(n, ps, false, st, nullptr));
      // source types with NO stacked columns in this layer (their only live conv is the aggregate-first one): no GEMM -- the
      // masked transpose directly
      for (int s = 0; s < n->T; ++s) {
        SrcTerm T;
        if (Y.ncols[s] != 0 || b->n_nodes[s] == 0 || !src_term(s, T)) continue;
        float* dst = l > 0 ? n->G[l][s] : d_gx[s];
        if (!dst) continue;
        const ConvLayout& Q = Y.conv[T.c];
        const hmp_layer_spec* Lp = l > 0 ? &S.layers[l - 1] : nullptr;
        const bool drop_on = Lp && n->training && Lp->dropout > 0.f;
        const int act = Lp ? Lp->act : HMP_ACT_NONE;
        const bool masked = Lp && (act != HMP_ACT_NONE || drop_on);
        bool gb = false;
        if (l > 0 && ps.empty())  // no GEMM decided the storage of G[l]: the same rule (see above)
          g16[l] = n->compute_bf16 != 0 && rows_kernel_bf16(n, b, l - 1) && (n->ld[l][s] & 3) == 0 &&
                   (b->n_nodes[s] >= 32768 || n->env.bf16_all);
        gb = l > 0 && g16[l];
        // the caller's input-gradient rows need not be whole 4-vectors (306 floats at pitch 306): exactly dim columns, element-wise
        const int ldg = l > 0 ? n->ld[l][s] : b->ldx[s];
        const int Fg = (ldg & 3) != 0 ? n->dim[l][s] : fpad(n->dim[l][s]);
        HMP_TRY(seg_mean_rows_t_launch(Q.dmrows, Q.ld_m, Fg, T.P->d_t_rowptr, T.P->d_t_col, T.degf, b->n_nodes[s],
                                       masked ? (const void*)n->H[l][s] : nullptr, n->ld[l][s], n->h16[l][s] ? 1 : 0, act, drop_on ? 1 : 0,
                                       drop_on ? 1.f / (1.f - Lp->dropout) : 1.f, dst, ldg, gb ? 1 : 0, st));
      }
    }
    if (!skip_w) {  // weight + bias gradient: dWp = dZ^T * [H | 1], split over node chunks (+ GAT: bias column sums, d V_edge), launched after the loop
      auto add = [&](int sid, const GemmProblem& p) {
        n->dyn.slab_stride[sid] = (int)p.slab_stride;
        wids.push_back(sid);
        wps.push_back(p);
      };
      for (int s = 0; s < n->T; ++s) {
        if (Y.ncols[s] == 0 || b->n_nodes[s] == 0) continue;  // no nodes: zero gradient (n_slabs stays 0)
        GemmProblem p;
        memset(&p, 0, sizeof(p));
        p.A = n->dZ[l][s]; p.lda = Y.ncols[s]; p.trans_a = 1;
        p.a_bf16 = dz16 ? 1 : 0;
        if (rootless && Y.roff[s] >= 0) { int ldg; p.A2 = g_of(s, ldg); p.lda2 = ldg; p.a_split = Y.roff[s]; }
        p.B = h_ptr(n, l, s); p.ldb = h_ld(n, l, s); p.trans_b = 0;
        p.b_bf16 = n->h16[l][s] ? 1 : 0;
        p.C = n->d_slabs + Y.slab_off[s]; p.ldc = Y.lddw[s];
        p.slab_stride = (int64_t)Y.ncols[s] * Y.lddw[s];
        p.M = Y.ncols[s]; p.N = n->dim[l][s] + 1; p.K = b->n_nodes[s];
        p.n_real = n->dim[l][s]; p.aug_ones = 1;
        add(slab_id_w(l, s), p);
      }
      for (int i = 0; i < Y.n_live; ++i) {  // aggregate-first convs: dW_l = dZ_block^T * M (destination-sized)
        const int c = Y.live[i];
        if (!aggf_live(c)) continue;
        const hmp_conv_spec& C = Ls.convs[c];
        const ConvLayout& Q = Y.conv[c];
        GemmProblem p;
        memset(&p, 0, sizeof(p));
        p.A = dz_at(C.dst, Q.aoff); p.lda = Y.ncols[C.dst]; p.trans_a = 1; p.a_bf16 = dz16 ? 1 : 0;
        p.B = Q.mrows; p.ldb = Q.ld_m; p.trans_b = 0;
        p.C = n->d_slabs + Q.cslab_off; p.ldc = Y.lddw[C.src];
        p.slab_stride = (int64_t)fpad(C.f_out) * Y.lddw[C.src];
        p.M = fpad(C.f_out); p.N = n->dim[l][C.src]; p.K = b->n_nodes[C.dst];
        p.n_real = p.N; p.aug_ones = 0;
        add(slab_id_v(l, c), p);
      }
      if (Y.kind == HMP_CONV_GAT) {
        for (int t = 0; t < n->T; ++t) {  // bias: column sums of the output gradient
          if (Y.n_in[t] == 0 || b->n_nodes[t] == 0) continue;
          int ldg;
          const float* g = g_of(t, ldg);
          GemmProblem p;
          memset(&p, 0, sizeof(p));
          p.A = g; p.lda = ldg; p.trans_a = 1;
          p.B = g; p.ldb = ldg; p.trans_b = 0;  // no real columns are read (n_real = 0): only the ones column
          p.C = n->d_slabs + Y.bslab_off[t]; p.ldc = 4;
          p.slab_stride = (int64_t)fpad(Ls.out_dim[t]) * 4;
          p.M = Ls.out_dim[t]; p.N = 1; p.K = b->n_nodes[t];
          p.n_real = 0; p.aug_ones = 1;
          add(slab_id_b(l, t), p);
        }
        for (int i = 0; i < Y.n_live; ++i) {  // d V_edge = edge_attr^T * d logit (original edge order)
          const int c = Y.live[i];
          const hmp_conv_spec& C = Ls.convs[c];
          if (C.edge_dim == 0 || b->n_edges[C.edge_type] == 0) continue;
          GemmProblem p;
          memset(&p, 0, sizeof(p));
          p.A = b->d_edge_attr[C.edge_type]; p.lda = C.edge_dim; p.trans_a = 1;
          p.B = Y.conv[c].dlogit_orig; p.ldb = GAT_HMAX; p.trans_b = 0;
          p.C = n->d_slabs + Y.conv[c].vslab_off; p.ldc = GAT_HMAX;
          p.slab_stride = GAT_MAX_EDIM * GAT_HMAX;
          p.M = C.edge_dim; p.N = C.heads; p.K = (int)b->n_edges[C.edge_type];
          p.n_real = C.heads;
          add(slab_id_v(l, c), p);
        }
      }
    }
  }
  if (skip_w) return HMP_OK;
  {  // the weight gradients of all layers: one launch with ~1k workgroups instead of L launches
    Scope sc(n, KC_GEMM_BWD, st);
    std::vector<int> ks;
    bool direct = n->fuse_now;
    if (direct) {  // register-direct TN kernel (one memory round trip per <= 192-node chunk); all-or-nothing per call
      if (!n->env.tn_direct) direct = false;
      // weight gradients of >= 10^9 multiply-adds (GAT at its batch size): split-K on the bf16 matrix pipe by the three-way split
      if (direct && !n->compute_bf16 && !wps.empty() && gemm_x3_split_takes(wps.data(), (int)wps.size())) direct = false;
      for (size_t i = 0; i < wps.size() && direct; ++i)
        if (wps[i].K > TN_DIRECT_SLABS * 384 || wps[i].b_bf16 || wps[i].a_bf16) direct = false;
      for (size_t base = 0; base < wps.size() && direct; base += GEMM_MAX_PROB) {
        TnBatch tb;
        memset(&tb, 0, sizeof(tb));
        const size_t cnt = (wps.size() - base) < (size_t)GEMM_MAX_PROB ? (wps.size() - base) : (size_t)GEMM_MAX_PROB;
        for (size_t i = 0; i < cnt; ++i) {
          const GemmProblem& g = wps[base + i];
          TnProblem& P = tb.p[tb.n++];
          P.A = g.A; P.B = g.B; P.C = g.C; P.slab_stride = g.slab_stride;
          P.M = g.M; P.N = g.N; P.K = g.K; P.lda = g.lda; P.ldb = g.ldb; P.ldc = g.ldc;
          P.n_real = g.n_real; P.aug_ones = g.aug_ones;
        }
        int ok = 0;
        HMP_TRY(gemm_tn_direct_launch(tb, TN_DIRECT_SLABS, &ok, st));
        HMP_CHECK_ARG(ok, "net: weight-gradient problem too deep for the direct kernel after the size check");
        for (size_t i = 0; i < cnt; ++i) ks.push_back(tb.p[i].ksplit);
      }
    }
    if (!direct) HMP_TRY(gemm_many(n, wps, true, st, &ks));
    for (size_t i = 0; i < wids.size(); ++i) n->dyn.n_slabs[wids[i]] = (unsigned char)ks[i];
  }
  {
    Scope sc(n, KC_GRAD_REDUCE, st);
    const int64_t na = n->spec.n_active_params;
    // Adam inside the un-pack: needs the valid-label count before the kernel starts (finalised by the first backward
    // kernel) and gradient terms that read no parameters (no GAT layer)
    AdamFuse af = n->call.adam;
    af.on = (af.on && fin_early && !n->any_gat) ? 1 : 0;
    n->call.adam_done = af.on != 0;
    HMP_TRY(grad_reduce_launch(n->d_grad_segs, n->d_grad_recs, n->n_grad_recs, n->dyn, n->d_slabs, d_params, d_grads,
                               n->call.fin_loss ? n->d_row_lv : nullptr, n->call.fin_rows > 0 ? n->call.fin_rows : b->n_out, d_grads + na, n->d_state,
                               af, st));
    n->call.fin_loss = false;
  }
  return HMP_OK;
}

// Sets up n->call for one entry call (the environment switches, the forward's dropout draw, a training step's counter) and puts
// it back to the defaults on every exit
struct StepGuard {
  hmp_net* n;
  StepGuard(hmp_net* net, int training = 0, uint64_t seed = 0, uint32_t rng_step = 0, int* d_step = nullptr) : n(net) {
    read_env(n);
    n->call.training = training; n->call.seed = seed; n->call.rng_step = rng_step;
    n->call.d_step = d_step;
  }
  ~StepGuard() { n->call = StepCall(); }
  StepGuard(const StepGuard&) = delete;
  StepGuard& operator=(const StepGuard&) = delete;
};

// a forward without a loss: hmp_net_forward, and the eval-mode forward of the count entries
int plain_forward(hmp_net* n, const hmp_batch* b, const float* d_params, hipStream_t st, int training = 0, uint64_t seed = 0,
                  uint32_t rng_step = 0) {
  StepGuard guard(n, training, seed, rng_step);
  return forward_impl(n, b, d_params, st);
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" int hmp_net_create(const hmp_net_spec* spec, hmp_net** out) {
  HMP_CHECK_ARG(spec && out, "hmp_net_create: null argument");
  HMP_CHECK_ARG(hmp_device_count() > 0, "hmp_net_create: no gfx950 device visible");
  hmp_net* n = new hmp_net;
  n->spec = *spec;
  int r = build_layout(n);
  if (r == HMP_OK) r = build_tables(n);
  if (r == HMP_OK) {
    // step counter + status bits live outside the workspace: a re-bind (a larger batch arrived) must not restart Adam's t or
    // the dropout sequence, nor lose status bits
    if (hipMalloc(&n->d_state, 256) != hipSuccess || hipMemset(n->d_state, 0, 256) != hipSuccess) {
      snprintf(err_buf(), 512, "hmp_net_create: device allocation of the net state failed");
      r = HMP_E_HIP;
    }
  }
  if (r == HMP_OK) {
    const int fz = env_switch("HMP_FUSE");
    n->fuse_mode = fz < 0 ? -1 : fz == '1' ? 1 : 0;
  }
  if (r != HMP_OK) {
    hmp_net_destroy(n);
    return r;
  }
  *out = n;
  return HMP_OK;
}

extern "C" void hmp_net_destroy(hmp_net* n) {
  if (!n) return;
  for (auto& r : n->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  if (n->d_state) (void)hipFree(n->d_state);
  if (n->d_pack_segs) (void)hipFree(n->d_pack_segs);
  if (n->d_pack_map) (void)hipFree(n->d_pack_map);
  if (n->d_grad_segs) (void)hipFree(n->d_grad_segs);
  if (n->d_grad_recs) (void)hipFree(n->d_grad_recs);
  for (int l = 0; l < HMP_MAX_LAYERS; ++l)
    if (l < n->L && n->lay[l].d_gat) (void)hipFree(n->lay[l].d_gat);
  delete n;
}

extern "C" size_t hmp_net_workspace_bytes(const hmp_net* net, const int32_t* cap_nodes, const int64_t* cap_edges) {
  if (!net || !cap_nodes || !cap_edges) return 0;
  hmp_net tmp = *net;  // carve() writes pointer fields; keep the real object untouched
  tmp.recs.clear();
  return carve(&tmp, nullptr, cap_nodes, cap_edges);
}

extern "C" int hmp_net_bind_workspace(hmp_net* n, void* d_workspace, size_t bytes, const int32_t* cap_nodes, const int64_t* cap_edges) {
  HMP_CHECK_ARG(n && d_workspace && cap_nodes && cap_edges, "hmp_net_bind_workspace: null argument");
  HMP_CHECK_ARG((reinterpret_cast<uintptr_t>(d_workspace) & 255) == 0, "hmp_net_bind_workspace: workspace must be 256-byte aligned");
  const size_t need = carve(n, (char*)d_workspace, cap_nodes, cap_edges);
  HMP_CHECK_ARG(bytes >= need, "hmp_net_bind_workspace: %zu bytes given, %zu needed", bytes, need);
  for (int t = 0; t < n->T; ++t) n->cap_nodes[t] = cap_nodes[t];
  for (int e = 0; e < n->ET; ++e) n->cap_edges[e] = cap_edges[e];
  n->ws_base = (char*)d_workspace;
  n->ws_bytes = need;
  // zero once: padding columns of every buffer stay zero for the lifetime of the binding
  HMP_HIP(hipMemset(d_workspace, 0, need));
  HMP_TRY(build_gat_tables(n));
  if (n->any_agg_first) {  // identity lists of the aggregate-first blocks
    std::vector<int> io((size_t)n->iota_cap + 1);
    for (size_t i = 0; i < io.size(); ++i) io[i] = (int)i;
    std::vector<float> on((size_t)n->iota_cap, 1.0f);
    HMP_HIP(hipMemcpy(n->d_iota, io.data(), io.size() * sizeof(int), hipMemcpyHostToDevice));
    HMP_HIP(hipMemcpy(n->d_ones, on.data(), on.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  n->bound = true;
  n->have_fwd = false;
  n->plan_ok = false;
  return HMP_OK;
}

extern "C" int hmp_net_forward(hmp_net* n, const hmp_batch* batch, const float* d_params, int32_t training, uint64_t seed,
                               uint32_t rng_step, const float** d_out, int32_t* ld_out, void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_out && ld_out, "hmp_net_forward: null argument");
  HMP_TRY(plain_forward(n, batch, d_params, (hipStream_t)stream, training, seed, rng_step));
  *d_out = out_ptr(n);
  *ld_out = n->out_ld;
  return HMP_OK;
}

extern "C" int hmp_net_backward(hmp_net* n, const float* d_gout, int32_t ld_gout, const float* d_params, float* d_grads,
                                float* const* d_gx, void* stream) {
  HMP_CHECK_ARG(n && d_gout && d_grads && d_params, "hmp_net_backward: null argument");
  return backward_impl(n, d_gout, ld_gout, d_grads, d_params, d_gx, (hipStream_t)stream);
}

extern "C" int hmp_net_aux_output(hmp_net* n, const float** d_out, int32_t* ld_out, int32_t* n_rows) {
  HMP_CHECK_ARG(n && d_out && ld_out && n_rows, "hmp_net_aux_output: null argument");
  HMP_CHECK_ARG(n->spec.aux_readout_type >= 0 && n->have_fwd, "hmp_net_aux_output: needs aux_readout_type and a forward");
  const int at = n->spec.aux_readout_type;
  *d_out = n->H[n->L][at];
  *ld_out = n->ld[n->L][at];
  *n_rows = n->batch.n_nodes[at];
  return HMP_OK;
}

extern "C" int hmp_net_hidden(hmp_net* n, int32_t layer, int32_t node_type, const void** d_h, int32_t* ld, int32_t* n_rows,
                              int32_t* width, int32_t* is_bf16) {
  HMP_CHECK_ARG(n && d_h && ld && n_rows && width && is_bf16, "hmp_net_hidden: null argument");
  HMP_CHECK_ARG(n->have_fwd, "hmp_net_hidden: needs a forward");
  HMP_CHECK_ARG(layer >= 1 && layer <= n->L && node_type >= 0 && node_type < n->T && n->H[layer][node_type] != nullptr,
                "hmp_net_hidden: layer %d / node type %d has no stored output", layer, node_type);
  *d_h = n->H[layer][node_type];
  *ld = n->ld[layer][node_type];
  *n_rows = n->batch.n_nodes[node_type];
  *width = n->dim[layer][node_type];
  *is_bf16 = n->h16[layer][node_type] ? 1 : 0;
  return HMP_OK;
}

extern "C" int hmp_net_plan(hmp_net* n, int32_t edge_type, hmp_plan* out) {
  HMP_CHECK_ARG(n && out, "hmp_net_plan: null argument");
  HMP_CHECK_ARG(n->have_fwd && n->plan_ok, "hmp_net_plan: needs a forward");
  HMP_CHECK_ARG(edge_type >= 0 && edge_type < n->ET, "hmp_net_plan: edge type %d out of range (the net has %d)", (int)edge_type, n->ET);
  *out = n->plan[edge_type];
  return HMP_OK;
}

extern "C" int hmp_net_backward2(hmp_net* n, const float* d_gout, int32_t ld_gout, const float* d_gout_aux, int32_t ld_aux,
                                 const float* d_params, float* d_grads, float* const* d_gx, void* stream) {
  HMP_CHECK_ARG(n && d_grads && d_params && (d_gout || d_gout_aux), "hmp_net_backward2: null argument");
  HMP_CHECK_ARG(n->spec.aux_readout_type >= 0, "hmp_net_backward2: the net has one output (use hmp_net_backward)");
  if (!d_gout) {  // no gradient for the first output: a zero block of its shape (G[L][readout] is free in the last layer)
    HMP_CHECK_ARG(n->have_fwd, "net: backward without a forward");
    const int rt = n->spec.readout_type, rows = n->batch.n_nodes[rt];
    if (rows > 0) HMP_HIP(hipMemsetAsync(n->G[n->L][rt], 0, (size_t)rows * n->ld[n->L][rt] * 4, (hipStream_t)stream));
    d_gout = n->G[n->L][rt];
    ld_gout = n->ld[n->L][rt];
  }
  return backward_impl(n, d_gout, ld_gout, d_grads, d_params, d_gx, (hipStream_t)stream, d_gout_aux, ld_aux);
}

extern "C" int hmp_net_set_head_pools(hmp_net* n, int32_t pool_edge_type_readout, int32_t pool_edge_type_aux) {
  HMP_CHECK_ARG(n, "hmp_net_set_head_pools: null net");
  const hmp_net_spec& S = n->spec;
  HMP_CHECK_ARG(!n->has_pools, "hmp_net_set_head_pools: the head pools are already set");
  HMP_CHECK_ARG(!n->bound, "hmp_net_set_head_pools: call before the first workspace bind");
  HMP_CHECK_ARG(S.aux_readout_type >= 0 && S.pool_edge_type < 0 && !n->has_heads,
                "hmp_net_set_head_pools: needs a two-headed net (aux_readout_type, no pool_edge_type, no linear heads)");
  HMP_CHECK_ARG(S.tail_act >= HMP_ACT_NONE && S.tail_act <= HMP_ACT_ELU && S.tail_dropout >= 0.f && S.tail_dropout < 1.f,
                "hmp_net_set_head_pools: spec tail_act %d / tail_dropout %g", S.tail_act, (double)S.tail_dropout);
  const int ets[2] = {pool_edge_type_readout, pool_edge_type_aux};
  for (int h = 0; h < 2; ++h) {
    const int e = ets[h], t = head_type(n, h);
    HMP_CHECK_ARG(e >= -1 && e < n->ET, "hmp_net_set_head_pools: head %d: edge type %d (-1 = unpooled, < %d)", h, e, n->ET);
    HMP_CHECK_ARG(n->dim[n->L][t] >= 1 && n->dim[n->L][t] <= POOL_TAIL_MAX_CLASSES,
                  "hmp_net_set_head_pools: head %d has %d classes (1 .. %d)", h, n->dim[n->L][t], POOL_TAIL_MAX_CLASSES);
    if (e < 0) continue;
    const int d = S.edge_dst[e];
    HMP_CHECK_ARG(S.edge_src[e] == t, "hmp_net_set_head_pools: head %d: edge type %d starts at node type %d, not the head's %d", h,
                  e, S.edge_src[e], t);
    HMP_CHECK_ARG(d != S.readout_type && d != S.aux_readout_type, "hmp_net_set_head_pools: head %d pools into a readout type", h);
    const hmp_layer_spec& Ls = S.layers[n->L - 1];
    for (int c = 0; c < Ls.n_convs; ++c)
      HMP_CHECK_ARG(Ls.convs[c].dst != d, "hmp_net_set_head_pools: head %d: node type %d receives a conv in the last layer", h, d);
  }
  if (ets[0] < 0 && ets[1] < 0) return HMP_OK;  // nothing pooled: the ordinary two-head step
  n->head_pool[0] = ets[0];
  n->head_pool[1] = ets[1];
  n->has_pools = true;
  return HMP_OK;
}

extern "C" int hmp_net_set_class_weights(hmp_net* n, int32_t head, const float* d_w, int32_t n_w) {
  HMP_CHECK_ARG(n, "hmp_net_set_class_weights: null net");
  HMP_CHECK_ARG(head == 0 || head == 1, "hmp_net_set_class_weights: head %d (0 = readout / rooms, 1 = aux / objects)", head);
  if (d_w == nullptr) {
    n->class_w[head] = nullptr;
    return HMP_OK;
  }
  const hmp_net_spec& S = n->spec;
  HMP_CHECK_ARG(head == 0 || n->has_heads || S.aux_readout_type >= 0, "hmp_net_set_class_weights: the net has one head");
  // the head's class count: a linear head's, or the width of the last layer on the head's node type
  const int classes = n->has_heads ? n->heads.classes[head] : (S.aux_readout_type >= 0 ? n->dim[n->L][head_type(n, head)] : n->out_dim);
  HMP_CHECK_ARG(n_w == classes, "hmp_net_set_class_weights: %d weights for head %d, which has %d classes", n_w, head, classes);
  n->class_w[head] = d_w;
  return HMP_OK;
}

extern "C" int hmp_net_set_linear_heads(hmp_net* n, const hmp_linear_heads* h) {
  HMP_CHECK_ARG(n && h, "hmp_net_set_linear_heads: null argument");
  const hmp_net_spec& S = n->spec;
  HMP_CHECK_ARG(!n->has_heads, "hmp_net_set_linear_heads: the heads are already set");
  HMP_CHECK_ARG(!n->bound, "hmp_net_set_linear_heads: call before the first workspace bind");
  HMP_CHECK_ARG(S.aux_readout_type < 0, "hmp_net_set_linear_heads: a net with a second readout type has its own two-head step");
  HMP_CHECK_ARG(h->F == n->out_dim, "hmp_net_set_linear_heads: F = %d, the program's output width is %d", h->F, n->out_dim);
  HMP_CHECK_ARG(h->F <= HEAD_MAX_F, "hmp_net_set_linear_heads: F = %d > %d", h->F, HEAD_MAX_F);
  for (int k = 0; k < 2; ++k) {
    const int c = h->classes[k];
    HMP_CHECK_ARG(c >= 1 && c <= HEAD_MAX_CLASSES, "hmp_net_set_linear_heads: classes[%d] = %d (1 .. %d)", k, c, HEAD_MAX_CLASSES);
    HMP_CHECK_ARG(h->w_off[k] >= 0 && h->w_off[k] + (int64_t)c * h->F <= S.n_active_params && h->b_off[k] >= 0 &&
                      h->b_off[k] + c <= S.n_active_params,
                  "hmp_net_set_linear_heads: head %d parameters must lie in [0, n_active_params = %lld)", k,
                  (long long)S.n_active_params);
  }
  HMP_CHECK_ARG(S.tail_act >= HMP_ACT_NONE && S.tail_act <= HMP_ACT_ELU && S.tail_dropout >= 0.f && S.tail_dropout < 1.f,
                "hmp_net_set_linear_heads: spec tail_act %d / tail_dropout %g", S.tail_act, (double)S.tail_dropout);
  const int K = h->classes[0] + h->classes[1];
  const int ld = fpad(h->F);
  const int64_t stride = align4((int64_t)K * ld + K);
  HMP_CHECK_ARG(n->n_grad + 4 <= SEG_MAX, "hmp_net_set_linear_heads: too many parameter segments");
  // four more gradient segments (W_room, W_object, b_room, b_object), each the sum of the head kernel's workgroup slabs
  std::vector<GradSeg> gs((size_t)n->n_grad + 4);
  if (n->n_grad > 0) HMP_HIP(hipMemcpy(gs.data(), n->d_grad_segs, (size_t)n->n_grad * sizeof(GradSeg), hipMemcpyDeviceToHost));
  const int64_t base = n->slab_floats;
  for (int k = 0; k < 2; ++k) {
    const int c = h->classes[k];
    const int64_t row0 = k == 0 ? 0 : h->classes[0];
    GradSeg& w = gs[(size_t)n->n_grad + k];
    memset(&w, 0, sizeof(w));
    w.dst = h->w_off[k]; w.rows = c; w.cols = h->F; w.n_terms = 1;
    w.t[0] = term(GT_COPY, HEAD_SLAB_ID, base + row0 * ld, ld, c, c);
    GradSeg& b = gs[(size_t)n->n_grad + 2 + k];
    memset(&b, 0, sizeof(b));
    b.dst = h->b_off[k]; b.rows = c; b.cols = 1; b.n_terms = 1;
    b.t[0] = term(GT_COPY, HEAD_SLAB_ID, base + (int64_t)K * ld + row0, 1, c, c);
  }
  GradSeg* d = nullptr;
  HMP_HIP(hipMalloc(&d, gs.size() * sizeof(GradSeg)));
  if (hipMemcpy(d, gs.data(), gs.size() * sizeof(GradSeg), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    snprintf(err_buf(), 512, "hmp_net_set_linear_heads: copy of the gradient table failed");
    return HMP_E_HIP;
  }
  if (const int rc = upload_grad_records(n, gs); rc != HMP_OK) {
    (void)hipFree(d);
    return rc;
  }
  if (n->d_grad_segs) (void)hipFree(n->d_grad_segs);
  n->d_grad_segs = d;
  for (int i = n->n_grad; i < (int)gs.size(); ++i) {
    const int64_t el = (int64_t)gs[i].rows * gs[i].cols;
    n->grad_elems += el;
    if (el > n->max_grad_elems) n->max_grad_elems = el;
  }
  n->n_grad = (int)gs.size();
  n->slab_floats = base + (int64_t)HEAD_MAX_BLOCKS * stride;
  n->head_slab_off = base; n->head_slab_stride = stride; n->head_ld_slab = ld;
  n->heads = *h;
  n->has_heads = true;
  return HMP_OK;
}

namespace {

int check_targets(const hmp_net* n, const hmp_batch* b, const hmp_head_targets* tg, const char* who) {
  const hmp_net_spec& S = n->spec;
  HMP_CHECK_ARG(S.aux_readout_type >= 0, "%s: the net has one output (aux_readout_type < 0): use the single-head entry", who);
  HMP_CHECK_ARG(S.tail_act >= HMP_ACT_NONE && S.tail_act <= HMP_ACT_ELU && S.tail_dropout >= 0.f && S.tail_dropout < 1.f,
                "%s: spec tail_act %d / tail_dropout %g", who, S.tail_act, (double)S.tail_dropout);
  for (int h = 0; h < 2; ++h)  // one label per row of the head's label type (the pool destination of a pooled head)
    HMP_CHECK_ARG(b->n_nodes[label_type(n, h)] == 0 || tg->d_labels[h] != nullptr, "%s: labels of head %d required", who, h);
  return HMP_OK;
}

int check_heads(const hmp_net* n, const hmp_batch* b, const hmp_linear_head_targets* tg, const char* who) {
  HMP_CHECK_ARG(n->has_heads, "%s: the net has no linear heads (hmp_net_set_linear_heads)", who);
  HMP_CHECK_ARG(!n->compute_bf16, "%s: the linear-head step computes in fp32 (bf16 compute mode is not supported)", who);
  HMP_CHECK_ARG(b->n_out == 0 || tg->d_labels != nullptr, "%s: labels required", who);
  return HMP_OK;
}

// the rows of one head for the stand-alone tail kernel (semisup.hip)
void add_tail(hmp_net* n, const hmp_batch* b, const hmp_head_targets* tg, int head, bool ce, TailArgs& ta) {
  const hmp_net_spec& S = n->spec;
  const int t = head == 0 ? S.readout_type : S.aux_readout_type;
  if (b->n_nodes[t] == 0) return;
  HeadTail& T = ta.h[ta.n++];
  memset(&T, 0, sizeof(T));
  T.z = n->H[n->L][t]; T.ldz = n->ld[n->L][t];
  T.n_rows = b->n_nodes[t]; T.classes = n->dim[n->L][t];
  T.labels = tg->d_labels[head]; T.mask = tg->d_mask[head];
  T.slot = head;
  if (!ce) return;
  T.weight = n->class_w[head];
  T.grad = head == 0 ? n->d_gout : n->G[n->L][t];
  T.ldg = head == 0 ? n->out_ld : n->ld[n->L][t];
  T.row_lv = n->d_row_lv + (head == 0 ? 0 : 2 * (int64_t)b->n_out);
  T.drop_on = (n->training && S.tail_dropout > 0.f) ? 1 : 0;
  if (T.drop_on) T.drop = make_drop(n, S.tail_dropout, (uint32_t)((n->L - 1) * HMP_MAX_NODE_TYPES + t));
}

// the rows of one head for the pooled tail launches (semisup.hip): final state of the head's type, its pool plan (none: identity),
// labels / mask / {loss, valid} per pooled row
void add_pool(hmp_net* n, const hmp_batch* b, const hmp_head_targets* tg, int head, bool ce, TailArgs& ta) {
  const hmp_net_spec& S = n->spec;
  const int t = head_type(n, head), lt = label_type(n, head);
  if (b->n_nodes[t] == 0 && b->n_nodes[lt] == 0) return;
  HeadTail& T = ta.h[ta.n++];
  memset(&T, 0, sizeof(T));
  T.z = n->H[n->L][t]; T.ldz = n->ld[n->L][t];
  T.n_rows = b->n_nodes[t]; T.classes = n->dim[n->L][t];
  T.n_pool = b->n_nodes[lt];
  if (n->head_pool[head] >= 0) {
    const hmp_plan& P = n->plan[n->head_pool[head]];
    T.rowptr = P.d_rowptr; T.col = P.d_col; T.t_rowptr = P.d_t_rowptr; T.t_col = P.d_t_col;
  }
  T.labels = tg->d_labels[head]; T.mask = tg->d_mask[head];
  T.slot = head;
  if (!ce) return;
  T.weight = n->class_w[head];
  T.grad = n->G[n->L][t]; T.ldg = n->ld[n->L][t];
  T.dpool = n->d_dpool[head]; T.ldp = n->ld[n->L][t];
  T.row_lv = n->d_row_lv + (head == 0 ? 0 : 2 * (int64_t)b->n_nodes[label_type(n, 0)]);
  T.drop_on = (n->training && S.tail_dropout > 0.f) ? 1 : 0;
  if (T.drop_on) T.drop = make_drop(n, S.tail_dropout, (uint32_t)((n->L - 1) * HMP_MAX_NODE_TYPES + t));
}

// The two heads' rows for one tail launch (semisup.hip): an entry for every wanted head that has rows, pooled or not as the net is.
// tg null: no labels and no masks (predict, top-k).  slot[h] = the entry of head h, -1 where it got none.
TailArgs tail_rows(hmp_net* n, const hmp_batch* b, const hmp_head_targets* tg, bool ce, int64_t ignored, const bool want[2],
                   int slot[2]) {
  static const hmp_head_targets none = {};
  TailArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.act = n->spec.tail_act; ta.ignored = ignored; ta.state = n->d_state;
  for (int h = 0; h < 2; ++h) {
    slot[h] = -1;
    if (!want[h]) continue;
    const int before = ta.n;
    if (n->has_pools) add_pool(n, b, tg ? tg : &none, h, ce, ta);
    else add_tail(n, b, tg ? tg : &none, h, ce, ta);
    if (ta.n > before) slot[h] = before;
  }
  return ta;
}

LinHeadArgs heads_args(hmp_net* n, const hmp_batch* b, const hmp_linear_head_targets* tg, const float* d_params, bool train,
                       int64_t ignored) {
  const hmp_net_spec& S = n->spec;
  LinHeadArgs a;
  memset(&a, 0, sizeof(a));
  a.z = out_ptr(n); a.ldz = n->out_ld; a.n_rows = b->n_out; a.F = n->heads.F;
  a.classes[0] = n->heads.classes[0]; a.classes[1] = n->heads.classes[1]; a.K = a.classes[0] + a.classes[1];
  for (int k = 0; k < 2; ++k) {
    a.W[k] = d_params + n->heads.w_off[k];
    a.bias[k] = d_params + n->heads.b_off[k];
    a.member[k] = tg->d_member[k];
  }
  a.labels = tg->d_labels; a.mask = tg->d_mask; a.ignored = ignored;
  a.act = S.tail_act;
  a.state = n->d_state;
  if (!train) return a;
  a.drop_on = (n->training && S.tail_dropout > 0.f) ? 1 : 0;
  if (a.drop_on) a.drop = make_drop(n, S.tail_dropout, (uint32_t)((n->L - 1) * HMP_MAX_NODE_TYPES + S.readout_type));
  a.grad = n->d_gout; a.ldg = n->out_ld;
  a.row_lv = n->d_row_lv;
  a.weight[0] = n->class_w[0]; a.weight[1] = n->class_w[1];
  a.slabs = n->d_slabs + n->head_slab_off; a.ld_slab = n->head_ld_slab; a.slab_stride = n->head_slab_stride;
  return a;
}

// ---- the loss stages of the training step.  After the forward, each writes d loss / d output (handed back with its ld to the
// backward), {loss, valid} per row, and the backward inputs of n->call that differ from the single head's
// single head: the masked CE over the output rows, unless it rode in the last aggregation's epilogue
int ce_loss(hmp_net* n, const hmp_batch* b, int64_t ignored, hipStream_t st, const float*& g, int& ldg) {
  g = n->d_gout; ldg = n->out_ld;
  if (n->call.ce_done) return HMP_OK;
  Scope sc(n, KC_LOSS, st);
  return masked_ce_rows_launch(out_ptr(n), n->out_ld, b->n_out, n->out_dim, b->d_labels, ignored, n->d_gout, n->out_ld, n->d_row_lv,
                               n->d_state, st, n->class_w[0]);
}

// two heads: the tail + CE of the heads the last epilogue did not serve, in one stand-alone launch over their rows; pooled heads:
// the CE over the pooled rows of both heads (one launch), then d loss / d z of every leaf row (one launch) -> G[L][t].  Both
// gradients are written; {loss_sum, count} sums the readout's rows then the aux rows (one count for both heads).
int two_head_loss(hmp_net* n, const hmp_batch* b, const hmp_head_targets* tg, int64_t ignored, hipStream_t st, const float*& g,
                  int& ldg) {
  StepCall& c = n->call;
  const bool want[2] = {n->has_pools || !c.tail_done[0], n->has_pools || !c.tail_done[1]};
  int slot[2];
  TailArgs ta = tail_rows(n, b, tg, true, ignored, want, slot);
  c.aux_g_ready = true;
  if (!n->has_pools) {
    g = n->d_gout; ldg = n->out_ld;
    c.fin_rows = b->n_out + b->n_nodes[n->spec.aux_readout_type];
    if (ta.n == 0) return HMP_OK;
    Scope sc(n, KC_LOSS, st);
    return tail_ce_launch(ta, st);
  }
  const int rt = n->spec.readout_type;
  g = n->G[n->L][rt]; ldg = n->ld[n->L][rt];
  c.fin_rows = b->n_nodes[label_type(n, 0)] + b->n_nodes[label_type(n, 1)];
  if (ta.n == 0) return HMP_OK;
  {
    Scope sc(n, KC_LOSS, st);
    HMP_TRY(pool_tail_ce_launch(ta, st));
  }
  Scope sc(n, KC_LOSS, st);
  return pool_tail_grad_launch(ta, st);
}

// linear heads in place of the loss kernel: d loss / d z -> d_gout, {loss, valid} per row, dW / db slabs
int heads_loss(hmp_net* n, const hmp_batch* b, const hmp_linear_head_targets* tg, const float* d_params, int64_t ignored,
               hipStream_t st, const float*& g, int& ldg) {
  LinHeadArgs a = heads_args(n, b, tg, d_params, true, ignored);
  g = n->d_gout; ldg = n->out_ld;
  n->call.head_blocks = heads_blocks(b->n_out);
  Scope sc(n, KC_LOSS, st);
  return linear_heads_ce_launch(a, st);
}

// The targets of a step: the two heads', the linear heads', or neither (the single-head CE over hmp_batch::d_labels)
struct StepTargets {
  const hmp_head_targets* two = nullptr;
  const hmp_linear_head_targets* lin = nullptr;
};

// One training step: forward (the single-head CE or the two heads' tail + CE riding in its last aggregation where they fit), the
// loss stage, backward with the loss finalisation ({loss_sum, count} -> d_grads[na], d_grads[na + 1]), and, with moments d_m / d_v
// (the *_fused entries, whose parameters are writable), Adam -- in the gradient un-pack where it can ride, else on its own.
int run_step(hmp_net* n, const hmp_batch* b, const StepTargets& tg, const float* d_params, float* d_grads, float* d_m, float* d_v,
             const hmp_train_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  StepGuard guard(n, args->training, args->seed, 0, args->d_step ? args->d_step : &n->d_state->step);
  StepCall& c = n->call;
  c.ce_labels = tg.two || tg.lin ? nullptr : b->d_labels;
  c.tgt = tg.two;
  c.ce_ignored = args->ignored_label;
  if (d_m) {
    AdamFuse& af = c.adam;
    af.on = n->fuse_mode == 0 ? 0 : 1;
    af.p = const_cast<float*>(d_params); af.m = d_m; af.v = d_v;
    af.lr = args->lr; af.b1 = args->beta1; af.b2 = args->beta2; af.eps = args->eps; af.wd = args->weight_decay;
    af.step_dev = c.d_step;
    af.count = d_grads + n->spec.n_active_params + 1;
  }
  HMP_TRY(forward_impl(n, b, d_params, st));
  const float* g = nullptr;
  int ldg = 0;
  if (tg.lin) HMP_TRY(heads_loss(n, b, tg.lin, d_params, args->ignored_label, st, g, ldg));
  else if (tg.two) HMP_TRY(two_head_loss(n, b, tg.two, args->ignored_label, st, g, ldg));
  else HMP_TRY(ce_loss(n, b, args->ignored_label, st, g, ldg));
  c.fin_loss = true;
  HMP_TRY(backward_impl(n, g, ldg, d_grads, d_params, nullptr, st));
  if (!d_m || c.adam_done) return HMP_OK;
  return hmp_net_step_adam(n, const_cast<float*>(d_params), d_grads, d_m, d_v, args, stream);
}

}  // namespace

extern "C" int hmp_net_step_fwd_bwd(hmp_net* n, const hmp_batch* batch, const float* d_params, float* d_grads,
                                    const hmp_train_args* args, void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_grads && args, "hmp_net_step_fwd_bwd: null argument");
  HMP_CHECK_ARG(n->spec.aux_readout_type < 0, "hmp_net_step_fwd_bwd: the fused step computes one cross entropy (single-output nets)");
  HMP_CHECK_ARG(batch->d_labels != nullptr, "hmp_net_step_fwd_bwd: labels required");
  return run_step(n, batch, {}, d_params, d_grads, nullptr, nullptr, args, stream);
}

extern "C" int hmp_net_step_fused(hmp_net* n, const hmp_batch* batch, float* d_params, float* d_grads, float* d_m, float* d_v,
                                  const hmp_train_args* args, void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_grads && d_m && d_v && args, "hmp_net_step_fused: null argument");
  HMP_CHECK_ARG(n->spec.aux_readout_type < 0, "hmp_net_step_fused: the fused step computes one cross entropy (single-output nets)");
  HMP_CHECK_ARG(batch->d_labels != nullptr, "hmp_net_step_fused: labels required");
  return run_step(n, batch, {}, d_params, d_grads, d_m, d_v, args, stream);
}

extern "C" int hmp_net_step2_fwd_bwd(hmp_net* n, const hmp_batch* batch, const hmp_head_targets* targets, const float* d_params,
                                     float* d_grads, const hmp_train_args* args, void* stream) {
  HMP_CHECK_ARG(n && batch && targets && d_params && d_grads && args, "hmp_net_step2_fwd_bwd: null argument");
  HMP_TRY(check_targets(n, batch, targets, "hmp_net_step2_fwd_bwd"));
  return run_step(n, batch, {targets, nullptr}, d_params, d_grads, nullptr, nullptr, args, stream);
}

extern "C" int hmp_net_step2_fused(hmp_net* n, const hmp_batch* batch, const hmp_head_targets* targets, float* d_params,
                                   float* d_grads, float* d_m, float* d_v, const hmp_train_args* args, void* stream) {
  HMP_CHECK_ARG(n && batch && targets && d_params && d_grads && d_m && d_v && args, "hmp_net_step2_fused: null argument");
  HMP_TRY(check_targets(n, batch, targets, "hmp_net_step2_fused"));
  return run_step(n, batch, {targets, nullptr}, d_params, d_grads, d_m, d_v, args, stream);
}

extern "C" int hmp_net_step_heads_fwd_bwd(hmp_net* n, const hmp_batch* batch, const hmp_linear_head_targets* targets,
                                          const float* d_params, float* d_grads, const hmp_train_args* args, void* stream) {
  HMP_CHECK_ARG(n && batch && targets && d_params && d_grads && args, "hmp_net_step_heads_fwd_bwd: null argument");
  HMP_TRY(check_heads(n, batch, targets, "hmp_net_step_heads_fwd_bwd"));
  return run_step(n, batch, {nullptr, targets}, d_params, d_grads, nullptr, nullptr, args, stream);
}

extern "C" int hmp_net_step_heads_fused(hmp_net* n, const hmp_batch* batch, const hmp_linear_head_targets* targets, float* d_params,
                                        float* d_grads, float* d_m, float* d_v, const hmp_train_args* args, void* stream) {
  HMP_CHECK_ARG(n && batch && targets && d_params && d_grads && d_m && d_v && args, "hmp_net_step_heads_fused: null argument");
  HMP_TRY(check_heads(n, batch, targets, "hmp_net_step_heads_fused"));
  return run_step(n, batch, {nullptr, targets}, d_params, d_grads, d_m, d_v, args, stream);
}

// ---- the readout entries (count, predict, top-k): the eval-mode forward, then ONE launch over the final state.  Every entry checks
// its arguments first -- a refused call launches nothing and leaves the last forward as it was -- and then states its launch.
namespace {

// the targets of a readout call in the net's form; predict and top-k have no labels (two: null, lin: the members alone)
struct ReadoutTargets {
  const hmp_head_targets* two = nullptr;
  const hmp_linear_head_targets* lin = nullptr;
  bool want[2] = {true, true};  // two heads: the heads the launch serves
  // Monte-Carlo dropout: the forward runs in training mode at (seed, rng_step) and the readout's tail draws at the same site
  int training = 0;
  uint64_t seed = 0;
  uint32_t rng_step = 0;
};

// the final state in the net's readout form: the linear heads' arguments, the two heads' tail rows, or (neither filled) the output
// rows out_ptr(n)
struct Readout {
  LinHeadArgs lin;
  TailArgs ta;
  int slot[2];  // head -> entry of ta, -1: none
};

template <class Launch>
int run_readout(hmp_net* n, const hmp_batch* b, const float* d_params, const ReadoutTargets& tg, void* stream, Launch&& launch) {
  hipStream_t st = (hipStream_t)stream;
  HMP_TRY(plain_forward(n, b, d_params, st, tg.training, tg.seed, tg.rng_step));
  const hmp_net_spec& S = n->spec;
  const bool drop = tg.training && S.tail_dropout > 0.f;  // the tail's site: what add_tail / add_pool / heads_args give the CE
  Readout r;
  if (n->has_heads) {
    r.lin = heads_args(n, b, tg.lin, d_params, false, 0);
    r.lin.drop_on = drop ? 1 : 0;
    if (drop) r.lin.drop = make_drop(n, S.tail_dropout, (uint32_t)((n->L - 1) * HMP_MAX_NODE_TYPES + S.readout_type));
  } else if (S.aux_readout_type >= 0) {
    r.ta = tail_rows(n, b, tg.two, false, 0, tg.want, r.slot);
    if (r.ta.n == 0) return HMP_OK;  // no wanted head has rows
    for (int i = 0; i < r.ta.n && drop; ++i) {
      HeadTail& T = r.ta.h[i];
      T.drop_on = 1;
      T.drop = make_drop(n, S.tail_dropout, (uint32_t)((n->L - 1) * HMP_MAX_NODE_TYPES + head_type(n, T.slot)));
    }
  }
  Scope sc(n, KC_LOSS, st);
  return launch(r, st);
}

// the guards on the net's kind; `instead` names the entries that serve the other kinds
int check_single_head(const hmp_net* n, const char* who, const char* instead) {
  HMP_CHECK_ARG(n->spec.aux_readout_type < 0 && !n->has_heads, "%s: a two-headed net %s", who, instead);
  return HMP_OK;
}

int check_tail_act(const hmp_net* n, const char* who) {
  const int act = n->spec.tail_act;
  HMP_CHECK_ARG(act >= HMP_ACT_NONE && act <= HMP_ACT_ELU, "%s: spec tail_act %d", who, act);
  return HMP_OK;
}

int check_two_heads(const hmp_net* n, const char* who, const char* instead) {
  HMP_CHECK_ARG(n->spec.aux_readout_type >= 0, "%s: the net has one output (aux_readout_type < 0): use %s", who, instead);
  return check_tail_act(n, who);
}

int check_label_heads(const hmp_net* n, const char* who) {
  HMP_CHECK_ARG(n->has_heads, "%s: the net has no linear heads (hmp_net_set_linear_heads)", who);
  HMP_CHECK_ARG(!n->compute_bf16, "%s: the linear heads compute in fp32 (bf16 compute mode is not supported)", who);
  return HMP_OK;
}

// the linear heads' targets of a label entry: the members alone
hmp_linear_head_targets members_only(const uint8_t* const d_member[2]) {
  hmp_linear_head_targets tg = {};
  tg.d_member[0] = d_member[0]; tg.d_member[1] = d_member[1];
  return tg;
}

long long* i64(int64_t* p) { return reinterpret_cast<long long*>(p); }

}  // namespace

extern "C" int hmp_net_count_correct2(hmp_net* n, const hmp_batch* batch, const hmp_head_targets* targets, const float* d_params,
                                      int64_t* d_counts, void* stream) {
  HMP_CHECK_ARG(n && batch && targets && d_params && d_counts, "hmp_net_count_correct2: null argument");
  HMP_TRY(check_targets(n, batch, targets, "hmp_net_count_correct2"));
  return run_readout(n, batch, d_params, {targets}, stream, [&](Readout& r, hipStream_t st) {
    return n->has_pools ? pool_tail_count_launch(r.ta, i64(d_counts), st) : tail_count_launch(r.ta, i64(d_counts), st);
  });
}

extern "C" int hmp_net_count_correct_heads(hmp_net* n, const hmp_batch* batch, const hmp_linear_head_targets* targets,
                                           const float* d_params, int64_t* d_counts, void* stream) {
  HMP_CHECK_ARG(n && batch && targets && d_params && d_counts, "hmp_net_count_correct_heads: null argument");
  HMP_TRY(check_heads(n, batch, targets, "hmp_net_count_correct_heads"));
  return run_readout(n, batch, d_params, {nullptr, targets}, stream,
                     [&](Readout& r, hipStream_t st) { return linear_heads_count_launch(r.lin, i64(d_counts), st); });
}

extern "C" int hmp_net_count_correct_rooms(hmp_net* n, const hmp_batch* batch, const float* d_params, const uint8_t* d_members,
                                           int64_t ignored_label, int64_t* d_counts, int64_t* d_confusion, void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_counts, "hmp_net_count_correct_rooms: null argument");
  HMP_TRY(check_single_head(n, "hmp_net_count_correct_rooms", "counts with hmp_net_count_correct2 / hmp_net_count_correct_heads"));
  HMP_CHECK_ARG(batch->n_out == 0 || batch->d_labels, "hmp_net_count_correct_rooms: the batch has no labels");
  return run_readout(n, batch, d_params, {}, stream, [&](Readout&, hipStream_t st) {
    return count_rows_launch(out_ptr(n), n->out_ld, batch->n_out, n->out_dim, batch->d_labels, d_members, ignored_label, i64(d_counts),
                             i64(d_confusion), st);
  });
}

extern "C" int hmp_net_count_correct_rooms_by_graph(hmp_net* n, const hmp_batch* batch, const float* d_params, const uint8_t* d_members,
                                                    int64_t ignored_label, int64_t* d_counts, void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_counts, "hmp_net_count_correct_rooms_by_graph: null argument");
  HMP_TRY(check_single_head(n, "hmp_net_count_correct_rooms_by_graph", "counts with hmp_net_count_correct2 / hmp_net_count_correct_heads"));
  HMP_CHECK_ARG(batch->n_out == 0 || batch->d_labels, "hmp_net_count_correct_rooms_by_graph: the batch has no labels");
  const hmp_net_spec& S = n->spec;
  const int ot = S.pool_edge_type >= 0 ? S.edge_dst[S.pool_edge_type] : S.readout_type;  // the node type of the output rows
  HMP_CHECK_ARG(batch->n_out == 0 || (batch->n_graphs > 0 && batch->d_node_ptr[ot]),
                "hmp_net_count_correct_rooms_by_graph: the batch carries no graph offsets of the output node type (n_graphs, d_node_ptr[%d])", ot);
  return run_readout(n, batch, d_params, {}, stream, [&](Readout&, hipStream_t st) {
    return count_rows_by_graph_launch(out_ptr(n), n->out_ld, batch->n_out, n->out_dim, batch->d_labels, d_members, ignored_label,
                                      batch->d_node_ptr[ot], batch->n_graphs, i64(d_counts), st);
  });
}

// ---- label output: the launch stores the prediction the count entries compare
extern "C" int hmp_net_predict_rooms(hmp_net* n, const hmp_batch* batch, const float* d_params, const uint8_t* d_members,
                                     int64_t* d_pred, void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && (d_pred || batch->n_out == 0), "hmp_net_predict_rooms: null argument");
  HMP_TRY(check_single_head(n, "hmp_net_predict_rooms", "predicts with hmp_net_predict2 / hmp_net_predict_heads"));
  return run_readout(n, batch, d_params, {}, stream, [&](Readout&, hipStream_t st) {
    return predict_rows_launch(out_ptr(n), n->out_ld, batch->n_out, n->out_dim, d_members, d_pred, st);
  });
}

extern "C" int hmp_net_predict2(hmp_net* n, const hmp_batch* batch, const float* d_params, int64_t* const d_pred[2], void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_pred, "hmp_net_predict2: null argument");
  HMP_TRY(check_two_heads(n, "hmp_net_predict2", "hmp_net_predict_rooms"));
  const ReadoutTargets tg = {nullptr, nullptr, {d_pred[0] != nullptr, d_pred[1] != nullptr}};  // a null output skips the head
  return run_readout(n, batch, d_params, tg, stream, [&](Readout& r, hipStream_t st) {
    int64_t* pred[2] = {nullptr, nullptr};
    for (int h = 0; h < 2; ++h)
      if (r.slot[h] >= 0) pred[r.slot[h]] = d_pred[h];
    return tail_predict_launch(r.ta, pred, n->has_pools, st);
  });
}

extern "C" int hmp_net_predict_heads(hmp_net* n, const hmp_batch* batch, const float* d_params, const uint8_t* const d_member[2],
                                     int64_t* const d_pred[2], void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_member && d_pred, "hmp_net_predict_heads: null argument");
  HMP_TRY(check_label_heads(n, "hmp_net_predict_heads"));
  const hmp_linear_head_targets tg = members_only(d_member);
  return run_readout(n, batch, d_params, {nullptr, &tg}, stream,
                     [&](Readout& r, hipStream_t st) { return linear_heads_predict_launch(r.lin, d_pred, st); });
}

// ---- top-k labels with softmax probabilities (tail_fns.h: topk_group).  k is checked before the forward, like everything else.
#define HMP_CHECK_TOPK(who, k) HMP_CHECK_ARG((k) >= 1 && (k) <= TOPK_MAX, who ": k = %d (1 .. %d)", (int)(k), TOPK_MAX)

extern "C" int hmp_net_topk_rooms(hmp_net* n, const hmp_batch* batch, const float* d_params, const uint8_t* d_members, int32_t k,
                                  int64_t* d_labels, float* d_probs, void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && (d_labels || d_probs || batch->n_out == 0), "hmp_net_topk_rooms: null argument");
  HMP_TRY(check_single_head(n, "hmp_net_topk_rooms", "takes hmp_net_topk2 / hmp_net_topk_heads"));
  HMP_CHECK_TOPK("hmp_net_topk_rooms", k);
  return run_readout(n, batch, d_params, {}, stream, [&](Readout&, hipStream_t st) {
    return topk_rows_launch(out_ptr(n), n->out_ld, batch->n_out, n->out_dim, d_members, k, d_labels, d_probs, st);
  });
}

extern "C" int hmp_net_topk2(hmp_net* n, const hmp_batch* batch, const float* d_params, int32_t k, int64_t* const d_labels[2],
                             float* const d_probs[2], void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_labels && d_probs, "hmp_net_topk2: null argument");
  HMP_TRY(check_two_heads(n, "hmp_net_topk2", "hmp_net_topk_rooms"));
  HMP_CHECK_TOPK("hmp_net_topk2", k);
  const ReadoutTargets tg = {nullptr, nullptr, {d_labels[0] || d_probs[0], d_labels[1] || d_probs[1]}};  // no output skips the head
  return run_readout(n, batch, d_params, tg, stream, [&](Readout& r, hipStream_t st) {
    int64_t* labels[2] = {nullptr, nullptr};
    float* probs[2] = {nullptr, nullptr};
    for (int h = 0; h < 2; ++h)
      if (r.slot[h] >= 0) { labels[r.slot[h]] = d_labels[h]; probs[r.slot[h]] = d_probs[h]; }
    return tail_topk_launch(r.ta, k, labels, probs, n->has_pools, st);
  });
}

extern "C" int hmp_net_topk_heads(hmp_net* n, const hmp_batch* batch, const float* d_params, const uint8_t* const d_member[2], int32_t k,
                                  int64_t* const d_labels[2], float* const d_probs[2], void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_member && d_labels && d_probs, "hmp_net_topk_heads: null argument");
  HMP_TRY(check_label_heads(n, "hmp_net_topk_heads"));
  HMP_CHECK_TOPK("hmp_net_topk_heads", k);
  const hmp_linear_head_targets tg = members_only(d_member);
  return run_readout(n, batch, d_params, {nullptr, &tg}, stream,
                     [&](Readout& r, hipStream_t st) { return linear_heads_topk_launch(r.lin, k, d_labels, d_probs, st); });
}

// ---- Monte-Carlo dropout (tail_fns.h: mc_group): ONE stochastic sample -- the training-mode forward at (seed, rng_step), then ONE
// launch that adds the softmax of the sample's scores to the caller's accumulators (first: stores it).  The refusals are the top-k
// siblings', checked before the forward.
namespace {

int check_mc_tail(const hmp_net* n, const char* who) {
  const float p = n->spec.tail_dropout;
  HMP_CHECK_ARG(p >= 0.f && p < 1.f, "%s: spec tail_dropout %g", who, (double)p);
  return HMP_OK;
}

ReadoutTargets mc_targets(const hmp_linear_head_targets* lin, bool want0, bool want1, uint64_t seed, uint32_t rng_step) {
  ReadoutTargets tg;
  tg.lin = lin;
  tg.want[0] = want0; tg.want[1] = want1;
  tg.training = 1; tg.seed = seed; tg.rng_step = rng_step;
  return tg;
}

}  // namespace

extern "C" int hmp_net_mc_rooms(hmp_net* n, const hmp_batch* batch, const float* d_params, const uint8_t* d_members, uint64_t seed,
                                uint32_t rng_step, int32_t first, float* d_acc, int32_t ld_acc, void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && (d_acc || batch->n_out == 0), "hmp_net_mc_rooms: null argument");
  HMP_TRY(check_single_head(n, "hmp_net_mc_rooms", "takes hmp_net_mc2 / hmp_net_mc_heads"));
  HMP_CHECK_ARG(ld_acc > mc_off_e(n->out_dim), "hmp_net_mc_rooms: ld_acc %d (%d classes need hmp_mc_acc_ld = %d)", (int)ld_acc, n->out_dim,
                mc_acc_ld(n->out_dim));
  return run_readout(n, batch, d_params, mc_targets(nullptr, true, true, seed, rng_step), stream, [&](Readout&, hipStream_t st) {
    return mc_rows_launch(out_ptr(n), n->out_ld, batch->n_out, n->out_dim, d_members, first, d_acc, ld_acc, st);
  });
}

extern "C" int hmp_net_mc2(hmp_net* n, const hmp_batch* batch, const float* d_params, uint64_t seed, uint32_t rng_step, int32_t first,
                           float* const d_acc[2], const int32_t ld_acc[2], void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_acc && ld_acc, "hmp_net_mc2: null argument");
  HMP_TRY(check_two_heads(n, "hmp_net_mc2", "hmp_net_mc_rooms"));
  HMP_TRY(check_mc_tail(n, "hmp_net_mc2"));
  for (int h = 0; h < 2; ++h) {
    const int C = n->dim[n->L][head_type(n, h)];
    HMP_CHECK_ARG(!d_acc[h] || ld_acc[h] > mc_off_e(C), "hmp_net_mc2: ld_acc %d of head %d (%d classes need hmp_mc_acc_ld = %d)", (int)ld_acc[h],
                  h, C, mc_acc_ld(C));
  }
  const ReadoutTargets tg = mc_targets(nullptr, d_acc[0] != nullptr, d_acc[1] != nullptr, seed, rng_step);  // no accumulator skips the head
  return run_readout(n, batch, d_params, tg, stream, [&](Readout& r, hipStream_t st) {
    float* acc[2] = {nullptr, nullptr};
    int ld[2] = {0, 0};
    for (int h = 0; h < 2; ++h)
      if (r.slot[h] >= 0) { acc[r.slot[h]] = d_acc[h]; ld[r.slot[h]] = ld_acc[h]; }
    return tail_mc_launch(r.ta, first, acc, ld, n->has_pools, st);
  });
}

extern "C" int hmp_net_mc_heads(hmp_net* n, const hmp_batch* batch, const float* d_params, const uint8_t* const d_member[2], uint64_t seed,
                                uint32_t rng_step, int32_t first, float* const d_acc[2], const int32_t ld_acc[2], void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_member && d_acc && ld_acc, "hmp_net_mc_heads: null argument");
  HMP_TRY(check_label_heads(n, "hmp_net_mc_heads"));
  HMP_TRY(check_mc_tail(n, "hmp_net_mc_heads"));
  for (int h = 0; h < 2; ++h)
    HMP_CHECK_ARG(!d_acc[h] || ld_acc[h] > mc_off_e(n->heads.classes[h]), "hmp_net_mc_heads: ld_acc %d of head %d (%d classes need hmp_mc_acc_ld = %d)",
                  (int)ld_acc[h], h, n->heads.classes[h], mc_acc_ld(n->heads.classes[h]));
  const hmp_linear_head_targets lt = members_only(d_member);
  return run_readout(n, batch, d_params, mc_targets(&lt, true, true, seed, rng_step), stream, [&](Readout& r, hipStream_t st) {
    const int ld[2] = {ld_acc[0], ld_acc[1]};
    return linear_heads_mc_launch(r.lin, first, d_acc, ld, st);
  });
}

// ---- attention export: the eval-mode forward, then ONE launch that writes the coefficients of the requested convs of one GAT
// layer from the softmax state the forward left (gat.hip: gat_attention_kernel).  Everything is checked before the forward.
extern "C" int hmp_net_attention(hmp_net* n, const hmp_batch* batch, const float* d_params, int32_t layer,
                                 float* const d_alpha[HMP_MAX_EDGE_TYPES], int32_t k, int64_t* const d_top_src[HMP_MAX_EDGE_TYPES],
                                 float* const d_top_w[HMP_MAX_EDGE_TYPES], void* stream) {
  HMP_CHECK_ARG(n && batch && d_params, "hmp_net_attention: null argument");
  HMP_CHECK_ARG(n->bound, "hmp_net_attention: workspace not bound (call hmp_net_bind_workspace)");
  HMP_CHECK_ARG(layer >= 0 && layer < n->L, "hmp_net_attention: layer %d out of range (the program has %d layers)", (int)layer, n->L);
  const LayerLayout& Y = n->lay[layer];
  HMP_CHECK_ARG(Y.kind == HMP_CONV_GAT, "hmp_net_attention: layer %d is not a GAT layer: it has no attention coefficients", (int)layer);
  HMP_CHECK_ARG(k >= 1 && k <= GAT_ATT_KMAX, "hmp_net_attention: k = %d (1 .. %d)", (int)k, GAT_ATT_KMAX);
  const hmp_layer_spec& Ls = n->spec.layers[layer];
  GatAttArgs a;
  memset(&a, 0, sizeof(a));
  a.k = k;
  for (int et = 0; et < HMP_MAX_EDGE_TYPES; ++et) {
    float* al = d_alpha ? d_alpha[et] : nullptr;
    int64_t* ts = d_top_src ? d_top_src[et] : nullptr;
    float* tw = d_top_w ? d_top_w[et] : nullptr;
    if (!al && !ts && !tw) continue;
    int c = -1;
    for (int i = 0; i < Ls.n_convs && c < 0; ++i)
      if (Ls.convs[i].edge_type == et) c = i;
    HMP_CHECK_ARG(et < n->ET && c >= 0, "hmp_net_attention: layer %d has no conv on edge type %d", (int)layer, et);
    HMP_CHECK_ARG(Ls.convs[c].active != 0,
                  "hmp_net_attention: the conv of layer %d on edge type %d is inactive (its output never reaches the readout: nothing is computed)",
                  (int)layer, et);
    GatAttReq& R = a.r[a.n];
    R.d = -1;
    for (int d = 0; d < Y.h_gat.n_dst; ++d)
      for (int i = 0; i < Y.h_gat.d[d].n_in; ++i)
        if (Y.h_gat.d[d].in[i].et == et) { R.d = d; R.i = i; }
    HMP_CHECK_ARG(R.d >= 0, "hmp_net_attention: the conv of layer %d on edge type %d is not in the layer table", (int)layer, et);
    R.alpha = al; R.top_src = reinterpret_cast<long long*>(ts); R.top_w = tw;
    R.ei = batch->d_edge_index[et];
    ++a.n;
  }
  hipStream_t st = (hipStream_t)stream;
  HMP_TRY(plain_forward(n, batch, d_params, st));
  if (a.n == 0) return HMP_OK;
  Scope sc(n, KC_GAT_FWD, st);
  GatDyn dyn = make_gat_dyn(n, batch);
  return gat_attention_launch(Y.d_gat, Y.h_gat, dyn, a, st);
}

// ---- input gradients: the eval-mode forward, ONE launch that writes the output gradient selecting what is explained
// (saliency.hip: saliency_seed_kernel) into the workspace, then the backward chain down to d loss / d x[t] without the weight
// gradients.  Everything is checked before the forward.
extern "C" int hmp_net_input_gradient(hmp_net* n, const hmp_batch* batch, const float* d_params, int32_t head, const int64_t* d_target,
                                      int32_t sel_mode, const uint8_t* d_mask, int32_t ordinal, const int64_t* d_graph_ptr,
                                      int32_t n_graphs, int32_t wrt, float* const d_gx[HMP_MAX_NODE_TYPES], void* stream) {
  HMP_CHECK_ARG(n && batch && d_params && d_gx, "hmp_net_input_gradient: null argument");
  HMP_CHECK_ARG(n->bound, "hmp_net_input_gradient: workspace not bound (call hmp_net_bind_workspace)");
  HMP_CHECK_ARG(!n->compute_bf16, "hmp_net_input_gradient: bf16 compute mode is not supported (input gradients are computed in fp32)");
  HMP_CHECK_ARG(!n->has_heads, "hmp_net_input_gradient: nets with learned linear heads are not supported (their outputs are not the "
                               "program's: the homogeneous two-headed task)");
  const hmp_net_spec& S = n->spec;
  const int at = S.aux_readout_type;
  HMP_CHECK_ARG(head == 0 || (head == 1 && at >= 0), "hmp_net_input_gradient: head %d (0: the readout%s)", (int)head,
                at >= 0 ? ", 1: the second output" : "; the net has one output");
  HMP_CHECK_ARG(!n->has_pools, "hmp_net_input_gradient: two-headed nets with pooled heads are not supported");
  HMP_CHECK_ARG(wrt == SAL_WRT_LOGIT || wrt == SAL_WRT_LOGPROB, "hmp_net_input_gradient: wrt = %d (0 logit, 1 log-probability)", (int)wrt);
  HMP_CHECK_ARG(sel_mode == SAL_SEL_ALL || sel_mode == SAL_SEL_MASK || sel_mode == SAL_SEL_ORDINAL,
                "hmp_net_input_gradient: selection mode %d (0 all, 1 mask, 2 ordinal)", (int)sel_mode);
  HMP_CHECK_ARG(sel_mode != SAL_SEL_MASK || d_mask || (head == 0 ? batch->n_out : batch->n_nodes[at]) == 0,
                "hmp_net_input_gradient: the mask selection needs a byte per output row");
  HMP_CHECK_ARG(sel_mode != SAL_SEL_ORDINAL || (d_graph_ptr && n_graphs >= 0 && ordinal >= 0),
                "hmp_net_input_gradient: the ordinal selection needs graph_ptr, n_graphs >= 0 and ordinal >= 0");
  if (at >= 0) HMP_TRY(check_tail_act(n, "hmp_net_input_gradient"));
  for (int t = 0; t < n->T; ++t)
    HMP_CHECK_ARG(!(n->pass0[t] && n->any_agg_first), "hmp_net_input_gradient: passthrough node types next to aggregate-first convs are not supported");
  for (int t = 0; t < n->T; ++t)
    HMP_CHECK_ARG(!d_gx[t] || (batch->d_x[t] && batch->ldx[t] >= n->dim[0][t]), "hmp_net_input_gradient: d_gx[%d] for a node type without input rows", t);
  hipStream_t st = (hipStream_t)stream;
  StepGuard guard(n);
  HMP_TRY(forward_impl(n, batch, d_params, st));
  SalSel sel;
  sel.mode = sel_mode; sel.mask = d_mask; sel.p = ordinal; sel.ptr = d_graph_ptr; sel.n_graphs = n_graphs;
  // two-headed nets: the model's outputs are act(final state) (hmp_net_spec::tail_act), so the seed chains through it
  const int act = at >= 0 ? S.tail_act : HMP_ACT_NONE;
  const float* gaux = nullptr;
  int ld_gaux = 0;
  {
    Scope sc(n, KC_LOSS, st);
    if (head == 0) {
      HMP_TRY(saliency_seed_launch(out_ptr(n), n->out_ld, batch->n_out, n->out_dim, d_target, sel, wrt, n->d_gout, n->out_ld, st, act));
    } else {  // the second output's gradient goes where the loss stages put it; the readout's is a zero block
      if (batch->n_out > 0) HMP_HIP(hipMemsetAsync(n->d_gout, 0, (size_t)batch->n_out * n->out_ld * 4, st));
      HMP_TRY(saliency_seed_launch(n->H[n->L][at], n->ld[n->L][at], batch->n_nodes[at], n->dim[n->L][at], d_target, sel, wrt,
                                   n->G[n->L][at], n->ld[n->L][at], st, act));
      n->call.aux_g_ready = true;
    }
  }
  return backward_impl(n, n->d_gout, n->out_ld, nullptr, d_params, d_gx, st, gaux, ld_gaux, true);
}

extern "C" int hmp_net_step_adam(hmp_net* n, float* d_params, const float* d_grads, float* d_m, float* d_v,
                                 const hmp_train_args* args, void* stream) {
  HMP_CHECK_ARG(n && d_params && d_grads && d_m && d_v && args, "hmp_net_step_adam: null argument");
  HMP_CHECK_ARG(n->bound, "hmp_net_step_adam: workspace not bound");
  hipStream_t st = (hipStream_t)stream;
  const int64_t na = n->spec.n_active_params;
  Scope sc(n, KC_ADAM, st);
  // t = the step counter the pack kernel bumped at the head of this step
  return adam_launch(d_params, d_grads, d_m, d_v, na, args->lr, args->beta1, args->beta2, args->eps, args->weight_decay, 0,
                     args->d_step ? args->d_step : &n->d_state->step, d_grads + na + 1, st);
}

extern "C" int hmp_net_read_state(hmp_net* n, int32_t* step, int32_t* status, void* stream) {
  HMP_CHECK_ARG(n && n->d_state, "hmp_net_read_state: null net");
  NetState h;
  HMP_HIP(hipStreamSynchronize((hipStream_t)stream));
  HMP_HIP(hipMemcpy(&h, n->d_state, sizeof(h), hipMemcpyDeviceToHost));
  // the counter of the last step (its optimiser's, hmp_train_args::d_step, or the net's own) was mirrored into the net's state by
  // the kernel that bumped it: the caller's pointer is not kept beyond the call that passed it
  if (step) *step = h.last_step;
  if (status) *status = h.status;
  return HMP_OK;
}

extern "C" int hmp_net_set_compute(hmp_net* n, int32_t bf16) {
  HMP_CHECK_ARG(n, "hmp_net_set_compute: null net");
  HMP_CHECK_ARG(bf16 == 0 || bf16 == 1, "hmp_net_set_compute: mode %d (0 = fp32, 1 = bf16 MFMA for large GEMMs)", bf16);
  n->compute_bf16 = bf16;
  return HMP_OK;
}

extern "C" int hmp_net_profile(hmp_net* n, int32_t enable) {
  HMP_CHECK_ARG(n, "hmp_net_profile: null net");
  n->prof = enable != 0;
  return HMP_OK;
}

extern "C" int hmp_net_profile_read(hmp_net* n, float* ms_sum, int32_t* launches) {
  HMP_CHECK_ARG(n && ms_sum && launches, "hmp_net_profile_read: null argument");
  for (int i = 0; i < HMP_N_KCLASS; ++i) { ms_sum[i] = 0.f; launches[i] = 0; }
  for (auto& r : n->recs) {
    HMP_HIP(hipEventSynchronize(r.b));
    float ms = 0.f;
    HMP_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    if (r.cls >= 0 && r.cls < HMP_N_KCLASS) { ms_sum[r.cls] += ms; launches[r.cls] += 1; }
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  n->recs.clear();
  return HMP_OK;
}
