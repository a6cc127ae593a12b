// Launch-level interfaces between the translation units (device pointers everywhere).
#pragma once
#include "common.h"

namespace hmp {

// ---------------------------------------------------------------------------------------------
// K2: grouped fp32 MFMA GEMM.  C[M,N] = op(A)[M,K] * op(B)[K,N]
// ---------------------------------------------------------------------------------------------
enum { EPI_NONE = 0, EPI_ACTMASK = 1 };

struct GemmProblem {
  const float* A;
  const float* B;
  float* C;
  const float* H;        // EPI_ACTMASK: activations whose derivative masks C (same shape as C)
  int c_bf16;            // gemm_bf16_kernel: C holds bf16 elements (ldc counts elements)
  int a_bf16;            // gemm_bf16_kernel: A holds bf16 elements (lda counts elements); every tile must take the fast loader
  int b_bf16;            // gemm_bf16_kernel: B holds bf16 elements (activations H as the weight gradient's operand); n_real must be
                         // whole tiles (a multiple of 256), the virtual ones column is the kernel's ONES product
  int h_bf16;            // gemm_bf16_kernel, EPI_ACTMASK: H holds bf16 elements (ldh counts elements)
  const float* A2;       // gemm_bf16_kernel with a_bf16: the slice of A from index a_split on (along its row-contiguous / K
  int lda2, a_split;     // axis: columns of dZ) lives in a second bf16 matrix -- the root block of dZ IS the output gradient,
                         // so nobody copies it.  a_split > 0 and a multiple of 256; 0: A is one matrix
  int64_t slab_stride;   // split-K: slab z is written at C + z*slab_stride
  int M, N, K;
  int lda, ldb, ldc, ldh;
  int trans_a;           // 0: A[m*lda+k]   1: A[k*lda+m]
  int trans_b;           // 0: B[k*ldb+n]   1: B[n*ldb+k]
  int n_real;            // columns of B that exist in memory (N or N-1 when aug_ones)
  int aug_ones;          // B gets a virtual last column of ones (bias gradient = column sums of A)
  int ksplit, kchunk;    // filled by gemm_launch
  int tiles_m, tiles_n, tile_start;
  int epi, act;
  int drop_on;
  DropCfg drop;          // dropout site of H (quad index = row*(ldh/4) + col/4)
  // NN form only: gather-add before the mask -- C[m, :] += sum over the entries k in [g_rowptr[m], g_rowptr[m+1]) of
  // g_rows[g_col[k], 0:N] * g_deg[g_col[k]]: the gradient of an AGGREGATE-FIRST conv's segment mean (net.hip), whose source
  // rows are this problem's output rows; g_rows is fp32 [.][g_ld].  g_rowptr == null: none
  // (gemm_bf16_dx_kernel only; the tiled kernels take the same term as a materialised matrix:)
  const int* g_rowptr;
  const int* g_col;
  const float* g_deg;
  const float* g_rows;
  int g_ld;
  const float* Cadd;     // NN form: fp32 [M][ldadd] added to the product before the mask (null: none)
  int ldadd;
};

constexpr int GEMM_MAX_PROB = 8;
constexpr int GEMM_TALL_SLABS = 192;  // split-K slabs the tall weight-gradient kernel may ask for (== net.hip: MAX_SLABS, the slab buffer's size)
struct GemmBatch {
  int n;
  int total_tiles;
  GemmProblem p[GEMM_MAX_PROB];
};

// Tile grid and split-K layout of a tiled launch with BM x BN tiles and K stages of BK: fills tiles_m, tiles_n, ksplit, kchunk and
// tile_start of every problem and gb.total_tiles (returned).  fold_ones: the virtual ones column rides in the first column tile
// (tiles_n counts the n_real columns).  want(p, all_tiles, tiles_k) is the launcher's wanted split of a problem with tiles, asked
// only for a split-K launch (all_tiles: tiles of the launch; tiles_k: their sum of tiles x K); the K chunk is that split rounded
// up to whole K stages, so the split used is cdiv(K, kchunk) (1 when K == 0).
template <class Want>
int gemm_plan_tiles(GemmBatch& gb, int BM, int BN, int BK, bool fold_ones, bool want_split, Want want) {
  int all_tiles = 0;
  double tiles_k = 0.0;
  for (int i = 0; i < gb.n; ++i) {
    GemmProblem& p = gb.p[i];
    p.tiles_m = cdiv(p.M, BM);
    p.tiles_n = cdiv(fold_ones && p.aug_ones ? (p.n_real > 0 ? p.n_real : 1) : p.N, BN);
    all_tiles += p.tiles_m * p.tiles_n;
    tiles_k += (double)(p.tiles_m * p.tiles_n) * p.K;
  }
  int start = 0;
  for (int i = 0; i < gb.n; ++i) {
    GemmProblem& p = gb.p[i];
    const int tiles = p.tiles_m * p.tiles_n;
    const int ks = (want_split && tiles > 0) ? want(p, all_tiles, tiles_k) : 1;
    int kchunk = cdiv(cdiv(p.K, ks), BK) * BK;
    if (kchunk < BK) kchunk = BK;
    p.ksplit = p.K > 0 ? cdiv(p.K, kchunk) : 1;
    p.kchunk = kchunk;
    p.tile_start = start;
    start += tiles * p.ksplit;
  }
  gb.total_tiles = start;
  return start;
}

// operand form shared by every problem of the launch (the executor's launches are uniform): 0 = NT, 1 = NN, 2 = TN, else 3 (the
// kernels' run-time variant)
inline int launch_form(const GemmBatch& gb) {
  int form = -1;
  for (int i = 0; i < gb.n; ++i) {
    const GemmProblem& p = gb.p[i];
    const int f = (!p.trans_a && p.trans_b) ? 0 : (!p.trans_a && !p.trans_b) ? 1 : (p.trans_a && !p.trans_b) ? 2 : 3;
    form = (form == -1 || form == f) ? f : 3;
  }
  return form;
}

// A batch split between a specialist kernel and the launcher that goes on with the rest: taken[] are the indices of the problems
// the specialist takes, rest holds the others in order and rest_idx[] their indices in the batch
struct GemmPeel {
  int n_taken;
  int taken[GEMM_MAX_PROB];
  int rest_idx[GEMM_MAX_PROB];
  GemmBatch rest;
};
template <class Pred>
void gemm_peel(const GemmBatch& gb, Pred takes, GemmPeel& s) {
  memset(&s, 0, sizeof(s));
  for (int i = 0; i < gb.n; ++i) {
    if (takes(gb.p[i])) {
      s.taken[s.n_taken++] = i;
    } else {
      s.rest_idx[s.rest.n] = i;
      s.rest.p[s.rest.n++] = gb.p[i];
    }
  }
}
// launch(s.rest) for the rest of a peeled batch (nothing when it is empty); the split that launch chose goes back into gb
template <class Launch>
int gemm_launch_rest(GemmBatch& gb, GemmPeel& s, Launch launch) {
  if (s.rest.n == 0) return HMP_OK;
  const int rc = launch(s.rest);
  for (int i = 0; i < s.rest.n; ++i) {
    gb.p[s.rest_idx[i]].ksplit = s.rest.p[i].ksplit;
    gb.p[s.rest_idx[i]].kchunk = s.rest.p[i].kchunk;
  }
  return rc;
}

// Persistent grid of the operand-stationary kernels: row-tile groups in sets of 8 (one per XCD), as many sets as per_cu
// workgroups per CU allow next to n_slices column slices (at least one set), no more groups than the n_tiles row tiles fill
struct XcdGrid {
  int groups, tiles_per_group;
};
inline XcdGrid xcd_set_grid(int per_cu, int n_slices, int n_tiles) {
  int sets = per_cu * device_cu_count() / (8 * n_slices);
  if (sets < 1) sets = 1;
  int groups = 8 * sets;
  if (groups > n_tiles) groups = ((n_tiles + 7) / 8) * 8;
  return {groups, cdiv(n_tiles, groups)};
}

// chooses tile shape + split-K (only when want_split: C is then a stack of slabs) and launches
int gemm_launch(GemmBatch& gb, bool want_split, int max_slabs, hipStream_t st);
// same contract on the bf16 matrix pipe (operands rounded to bf16 on their way into LDS, fp32 accumulate): gemm_bf16.hip
int gemm_bf16_launch(GemmBatch& gb, bool want_split, int max_slabs, hipStream_t st);
// fp32 accuracy on the bf16 matrix pipe (three exact bf16 pieces per operand element, six piece products): gemm_x3.hip; takes =
// every problem of the launch is plain fp32, the launch is big enough, and split-K launches only over < 32 768 nodes (HMP_GEMM_X3=0: never; =2: every split-K launch)
bool gemm_x3_takes(const GemmBatch& gb, bool want_split);
bool gemm_x3_split_takes(const GemmProblem* ps, int n);  // (split-K weight gradients of a step, before the direct TN kernel is chosen)
int gemm_x3_launch(GemmBatch& gb, bool want_split, int max_slabs, hipStream_t st);
// operand-stationary backward kernels of the 10^6-node regime (gemm_bf16_bwd.hip); *_takes: the problem fits the kernel's limits
bool gemm_bf16_dx_takes(const GemmProblem& p, bool want_split);
int gemm_bf16_dx_launch(const GemmProblem& p, hipStream_t st);
bool gemm_bf16_dw_takes(const GemmProblem& p, bool want_split);
int gemm_bf16_dw_launch(const GemmProblem& p, int max_slabs, int* n_slabs, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// front kernel of the small-batch step (front.hip): layer-0 projection tiles + plan parts + pack blocks in one launch
// ---------------------------------------------------------------------------------------------
constexpr int FR_MAX_PROB = 4;
constexpr int FR_MAX_SEG = 6;
constexpr int FR_MAX_SRC = 6;  // == AGG_MAX_IN
struct FrontSeg {    // rows [col0, col0 + rows) of the stacked B operand = sum of nsrc parameter blocks [rows][ld]
  int col0, rows, nsrc, ld;
  uint32_t off[FR_MAX_SRC];  // float offsets into the flat parameter buffer
};
struct FrontProb {   // C[M, N] = A[M, K] * B^T
  const float* A;
  float* C;
  int lda, ldc, M, N, K;
  int n_seg, max_nsrc, vec;
  int blk_start, tiles_m, tiles_n;
  FrontSeg seg[FR_MAX_SEG];
};
struct FrontJob {    // one edge type of the plan; arrays as 4-byte-word offsets from the workspace base
  const int64_t* ei;
  int E, n_src, n_dst;
  uint32_t rowptr, col, eid, t_rowptr, t_col, t_eid, tmp_in, tmp_out, pos_of_eid, degf, flags;
  const int64_t *gp_dst, *gp_src, *gp_edge;  // as PlanJob
  int n_graphs;
};
struct PackSeg;
struct NetState;
struct FrontArgs {
  // roles by block index: [0, gemm_blocks) projection tiles, then plan parts, then pack blocks
  int gemm_blocks, plan_blocks, pack_blocks;
  int n_prob, n_jobs, need_tpos, plan_rc;
  const float* params;
  char* ws;
  int* status;
  const PackSeg* segs;
  const int2* pack_map;  // per pack block: {segment, first item}; 16 items (packed row, 64-column chunk) per block
  float* packed;
  int* step_ctr;         // non-null: the pack role's first block bumps this device step counter
  int* step_mirror;      // ... and leaves the new value here (NetState::last_step: the net never keeps the caller's pointer)
  int prob_start[FR_MAX_PROB];  // prob[i].blk_start again, next to the header fields (front_launch fills it): see karg_warm (common.h)
  int part_start[2 * HMP_MAX_EDGE_TYPES + 1];
  int rows_per_part[2 * HMP_MAX_EDGE_TYPES];
  FrontJob job[HMP_MAX_EDGE_TYPES];
  FrontProb prob[FR_MAX_PROB];
};
int front_launch(FrontArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// register-direct TN GEMM for small batches (gemm_direct.hip)
// ---------------------------------------------------------------------------------------------
struct TnProblem {   // slab z of C[M, N] = sum_{k in chunk z} A[k, m] * [B | 1][k, n]
  const float* A;
  const float* B;
  float* C;
  int64_t slab_stride;
  int M, N, K, lda, ldb, ldc;
  int n_real, aug_ones;
  int ksplit, kchunk, tile_start, tiles_m, tiles_n;
};
struct TnBatch {
  int n, total_tiles;
  TnProblem p[GEMM_MAX_PROB];
};
// *ok = 0 (nothing launched) when a problem would need more than max_slabs slabs
int gemm_tn_direct_launch(TnBatch& tb, int max_slabs, int* ok, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------
struct PlanJob {
  const int64_t* ei;  // [2][E]
  int64_t E;
  int n_src, n_dst;
  int *rowptr, *col, *eid, *t_rowptr, *t_col, *t_pos;
  float* degf;  // optional [n_dst]: 1 / max(in-degree, 1) as float
  // optional (all three or none; single-launch build only): the batch is a union of n_graphs graphs whose edges are listed graph
  // by graph -- int64 [n_graphs + 1] row offsets of the destination / source node type and edge offsets (hmp_batch::d_edge_ptr)
  const int64_t *gp_dst, *gp_src, *gp_edge;
  int n_graphs;
  // scratch
  int *cnt_in, *cnt_out, *cur_in, *cur_out;  // must be zero on entry (one contiguous block); left zero on exit
  int* flags;  // multi-launch build: [0] / [1] = PlanBatch::build_id of the last build that found the list NOT ordered by destination /
               // source (or holding an invalid edge); part of the zeroed block.  An edge list that arrives ordered by destination --
               // what graph builders emit -- IS its CSR (position = edge id): no scatter, no rank pass for that direction.
               // Single-launch build of a graph-sorted list: [32 + 2 * dir] / [33 + 2 * dir] count the parts of a direction that
               // have arrived / that dropped an edge (plan_small_part); zero on entry, left zero
  int *tmp_in, *tmp_out, *t_eid, *pos_of_eid;
  int *tmpc_in, *tmpc_out;  // multi-launch build: the other endpoint of every scratch slot
};
struct PlanBatch {
  int n;
  int need_tpos;   // build t_pos (only GAT's source-major backward reads it)
  int clear_first; // memset the counters before the launch (caller-provided scratch of unknown content)
  int build_id;    // multi-launch build: stamp of this build (see PlanJob::flags)
  int* flags_all;  // [2 * n] = job 0's flag block used for ALL jobs: entry 2 j + dir (one pointer in the batch header: reading a
                   // per-job pointer through a per-lane job index made the compiler copy the 4 KB argument block to scratch)
  int64_t edge_start[HMP_MAX_EDGE_TYPES + 1];
  int64_t row_start[2 * HMP_MAX_EDGE_TYPES + 1];  // rows of (job, dir): dir 0 = by dst, 1 = by src
  PlanJob j[HMP_MAX_EDGE_TYPES];
};
// the plan keeps edge s -> d iff both endpoints exist; every other edge is dropped from the lists and sets status bit 0.  For
// readers of a plan that must know which edges it dropped (the attention export); the plan builds state the same condition in
// their own loops (plan_hist_kernel, plan_small_part), whose code is left as it is
__host__ __device__ inline bool plan_edge_ok(int64_t s, int64_t d, int n_src, int n_dst) {
  return s >= 0 && s < n_src && d >= 0 && d < n_dst;
}
size_t plan_scratch_ints(int64_t E, int n_src, int n_dst);
// carve scratch for job (all int32); zero_begin/zero_ints return the region to memset
void plan_carve(PlanJob& job, int* scratch);
int plan_launch(PlanBatch& pb, int* d_status, hipStream_t st);
int plan_link_launch(PlanBatch& pb, hipStream_t st);  // t_pos only, after a single-launch build that ran elsewhere (front kernel)

// ---------------------------------------------------------------------------------------------
// K1 + fused SAGE aggregation
// ---------------------------------------------------------------------------------------------
constexpr int AGG_MAX_IN = 6;
struct AggIn {
  const int* rowptr;
  const int* col;
  const float* z;  // projected source rows
  int ldz, coff;
  int same_type;   // source node type == destination node type (one index space): candidate for the LDS-windowed gather
  int n_src;       // rows of z
};
struct AggDst {
  int n_rows, F;
  float* out;
  int ldo;
  const float* zroot;  // may be null
  int ldzr, roff;
  const float* bias;   // may be null
  int n_in;
  int act;
  int drop_on;
  DropCfg drop;
  int block_start;
  // fused projection of the NEXT layer (agg_proj_fwd_launch): Z[l+1][t] = out * pw^T, pw = Wp[l+1][t] [pncols][pldw]
  const float* pw;  // null: this node type is not read by the next layer
  float* pz;
  int pldw, pldz, pncols, pK;
  // fused masked cross entropy on the rows of this entry (last layer of the fused training step): gradient of the SUM loss
  // to ce_grad, per-row {loss, valid} to ce_row_lv
  const int64_t* ce_labels;  // null: off
  int64_t ce_ignored;
  int ce_classes, ce_ldg;
  float* ce_grad;
  float* ce_row_lv;
  // two-headed step (hmp_net_step2_*): rows whose mask byte is 0 do not count (null: every row), and with ce_tail set the entry's
  // act / dropout are the model's tail, so the gradient written is d loss / d (pre-activation): . keep/(1-p) . act', read off y
  const uint8_t* ce_mask;
  const float* ce_weight;    // class weights of the entry's head [ce_classes], null: unweighted (tail_fns.h: ce_group)
  int ce_tail;
  int win_in;                // filled by agg_fwd_launch: in-conv served from the LDS window (-1: none)
  int tile_rows;             // agg_proj_fwd_launch: rows per workgroup, 16 or 8.  A launch is as long as its slowest tile and a tile of
                             // high-degree rows (rooms: ~12 objects each) requests twice the lines of the others (tools/ktime_blocks.py:
                             // 7.3 us against 5.8 us): such entries are cut into twice as many tiles of 8 rows (there are idle CUs)
  AggIn in[AGG_MAX_IN];
};
struct AggArgs {
  int n;
  int total_blocks;
  int mean;  // divide every gather by max(deg,1)
  int xcd;   // large launches: consecutive row ranges stay on one XCD (block counts padded to 8 per entry), see agg_fwd_launch
  int zb16;  // the projected rows (AggIn::z, AggDst::zroot) hold bf16 elements (bf16 compute mode, 256-wide rows)
  int hb16;  // with zb16: the outputs (AggDst::out) are WRITTEN as bf16 elements too (activations of a hidden layer, read only by GEMMs)
  NetState* state;  // status bits (fused cross entropy: label out of range)
  int bstart[HMP_MAX_NODE_TYPES];  // d[i].block_start again, in the struct's first lines (filled by the launchers): a workgroup
                                   // finds its entry without touching one argument line per entry, see karg_warm (common.h)
  AggDst d[HMP_MAX_NODE_TYPES];
};
int agg_fwd_launch(AggArgs& a, hipStream_t st);
// same + next-layer projection per 16-row tile (requires F <= 256, pK % 16 == 0, pK <= 256 for every entry with pw)
int agg_proj_fwd_launch(AggArgs& a, hipStream_t st);

struct TAggOut {
  const int* t_rowptr;
  const int* t_col;
  const int* rowptr;  // forward CSR rowptr of the same edge type (for 1/deg of the destination)
  const float* degf;  // 1 / max(deg,1) per destination (plan by-product), null: derive from rowptr
  const float* g;     // gradient rows of the destination type
  int ldg, coff, F;
  int same_type;      // destination node type == source node type: candidate for the LDS-windowed gather
  int n_dst;          // rows of g
};
struct TAggSrc {
  int n_rows;
  float* dz;
  int lddz, ncols;     // ncols (padded): columns not covered by a segment are zeroed
  const float* groot;  // may be null
  int ldgr, roff, Froot;
  int n_out;
  int block_start;
  // fused input gradient (agg_bwd_dx_launch): xg = (dz * Wp[l][s]) . act'(xh), the weights read from their transposed image
  // xwt = WpT[l][s] [fpad(xN)][xldt] (PackSeg::dst_t, columns in the order of wpt_col): xldt = ncols rounded up to 16, padding zero
  const float* xwt;  // null: no input gradient for this node type
  float* xg;
  const float* xh;  // activations whose derivative masks xg (null: none)
  int xldt, xN, xldg, xldh, xact, xdrop_on;
  float xscale;
  int win_out;                // filled by agg_bwd_launch (see AggDst::win_in)
  int tile_rows;              // agg_bwd_dx_launch: rows per workgroup, 16 or 8 (see AggDst::tile_rows)
  TAggOut out[AGG_MAX_IN];
};
struct TAggArgs {
  int n;
  int total_blocks;
  int mean;
  int xcd;  // as AggArgs::xcd
  int gb16; // the gradient rows (TAggOut::g, TAggSrc::groot) hold bf16 elements
  int dzb16; // dz is written as bf16 (requires gb16)
  // one extra block sums the per-row {loss, valid} pairs of the loss in fixed order -> fin_out2 / fin_state (null: off)
  const float* fin_row_lv;
  int fin_rows;
  float* fin_out2;
  NetState* fin_state;
  int bstart[HMP_MAX_NODE_TYPES];  // s[i].block_start again (as AggArgs::bstart)
  TAggSrc s[HMP_MAX_NODE_TYPES];
};
int agg_bwd_launch(TAggArgs& a, hipStream_t st);
// same + the row-local input-gradient GEMM per 16-row tile (requires every segment width <= 256, ncols <= 896)
int agg_bwd_dx_launch(TAggArgs& a, hipStream_t st);

// aggregate-first convs (aggfirst.hip): segment mean of source rows (fp32 or bf16) into fp32 rows, and its transpose with the
// activation / dropout mask of the source rows for source types that have no input-gradient GEMM in the layer
int seg_mean_rows_launch(const void* x, int ldx, int x_bf16, int F, const int* rowptr, const int* col, int n_rows, float* m, int ldm,
                         hipStream_t st);
int seg_mean_rows_t_launch(const float* dm, int lddm, int F, const int* t_rowptr, const int* t_col, const float* degf, int n_rows,
                           const void* h, int ldh, int h_bf16, int act, int drop_on, float dscale, void* g, int ldg, int g_bf16, hipStream_t st);
// The source rows' gradient term of an aggregate-first conv on the input-gradient problem p of its source type (rows of p = source
// rows): p.g_* when the weight-stationary dx kernel takes p that way (bf16 compute mode only), else the term materialised as fp32
// [p.M][g_ld] at scratch + *scratch_used (advanced by what it takes; scratch_floats: the scratch's size) and handed over as p.Cadd
int gemm_dx_gather_term(GemmProblem& p, bool bf16_mode, const int* t_rowptr, const int* t_col, const float* degf, const float* g_rows,
                        int g_ld, float* scratch, int64_t scratch_floats, int64_t* scratch_used, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// parameter packing / gradient un-packing (tables live in device memory, built at bind time)
// ---------------------------------------------------------------------------------------------
// kinds of packed rows
//  PACK_SUM     row r            = sum_q P[src[q]][r, :]                       (SAGE weights, root sums, bias sums)
//  PACK_HEADS   row h*Cp + c     = P[src[0]][h*C + c, :] (c < C), else 0       (GAT lin_src with heads padded to 4)
//  PACK_ATTDOT  row h            = sum_c P[att][h*C + c] * P[src[0]][h*C + c, :]   (V^T = fold of att into lin: a = x * V)
//  PACK_ATTDOT_T element (d, h)  = sum_c P[att][h*C + c] * P[src[0]][(h*C + c), d] (V_edge [edge_dim][H])
enum { PACK_SUM = 0, PACK_HEADS = 1, PACK_ATTDOT = 2, PACK_ATTDOT_T = 3 };
struct PackSeg {
  int64_t dst;      // float offset into the packed buffer
  int rows, rows_pad, cols, ld_dst;
  int ld_src;       // == cols (parameters are dense)
  int nsrc;
  int kind, H, C, Cp;
  int64_t att;      // PACK_ATTDOT*: float offset of the attention vector [H*C]
  int64_t src[AGG_MAX_IN];  // float offsets into the flat parameter buffer (summed)
  // PACK_SUM, ld_dst_t > 0: the same element (r, c) is also stored at dst_t + c * ld_dst_t + wpt_col(col_t + r) -- the transposed
  // image WpT of the stacked weights that the fused input gradient reads (TAggSrc::xwt); dst_t = start of the image, col_t = the
  // segment's first row in the stack.  pad_t: stacked rows behind the segment's own rows_pad that it stores as zeros (the last
  // segment of a stack pads the image to ld_dst_t)
  int64_t dst_t;
  int ld_dst_t, col_t, pad_t;
};
// Column of WpT that holds stacked row k = 16 b + 4 u + q: 16 b + 4 q + u.  The 16 bytes a lane of quarter q loads at column
// 16 b + 4 q are then the rows 16 b + 4 u + q, u = 0..3: MFMA step 4 b + u multiplies rows 16 b + 4 u .. + 3, one per quarter, in
// the order of a walk down Wp itself -- the sum over k is taken in the same order, bit for bit, as from the untransposed operand.
__host__ __device__ inline int wpt_col(int k) { return (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3); }
// block -> segment map of the table-driven kernels: segment i owns blocks [start[i], start[i+1]); passed by value so the
// lookup is a scan of scalar (kernarg) loads instead of a dependent chain of global loads
constexpr int SEG_MAX = 400;
struct SegBlocks {
  int n;
  int start[SEG_MAX + 1];
};
// the two block maps of a pack table (net.hip; build_tables and the unit entry hmp_front_run call the same two): the SegBlocks
// starts of pack_launch, and FrontArgs::pack_map (returns the number of blocks; pm == null: only counts them)
void pack_seg_blocks(const PackSeg* ps, int n, SegBlocks& sb);
int pack_block_map(const PackSeg* ps, int n, int2* pm);
// step_ctr != null: block 0 increments *step_ctr (the fused step starts with the pack)
int pack_launch(const PackSeg* d_segs, const SegBlocks& sb, const float* d_params, float* d_packed, int* step_ctr, int* step_mirror,
                hipStream_t st);

// A parameter gradient element (r, c) is the sum of up to 3 terms read from split-K slabs S (summed over slabs):
//  GT_COPY       S[(r/C*Cp + r%C) * ld + c]                         (rows of the stacked operand; C = Cp: identity)
//  GT_ATT_OUTER  P[att + r] * S[(r/C) * ld + c]                     (d lin from a = x * fold(att, lin))
//  GT_ATT_DOT    sum_f S[(r/C) * ld + f] * P[w + r * ldw + f]       (d att; parameter element r = h*C + c, cols = 1)
//  GT_ATT_OUTER_T  P[att + r] * S[c * ld + r/C]                     (d lin_edge from V_edge [D][H])
//  GT_ATT_DOT_T    sum_d S[d * ld + r/C] * P[w + r * ldw + d]       (d att_edge)
enum { GT_COPY = 0, GT_ATT_OUTER = 1, GT_ATT_DOT = 2, GT_ATT_OUTER_T = 3, GT_ATT_DOT_T = 4 };
struct GradTerm {
  int kind;
  int slab_id;      // index into the per-call n_slabs / slab_stride arrays
  int64_t src;      // float offset of the term's origin inside slab 0
  int ld;
  int C, Cp;
  int inner;        // GT_ATT_DOT*: length of the dot product
  int64_t att, w;   // parameter offsets
  int ldw;
  float scale;
};
struct GradSeg {
  int64_t dst;       // float offset into the flat gradient buffer
  int rows, cols;    // parameter shape (vectors: cols = 1)
  int n_terms;
  GradTerm t[3];
};
// slab ids of layer l: l*SLAB_IDS_PER_LAYER + {t: stacked weights of node type t | 8 + t: bias column sums of
// node type t (GAT) | 16 + c: V_edge of conv c (GAT_edge)}
constexpr int SLAB_IDS_PER_LAYER = 2 * HMP_MAX_NODE_TYPES + HMP_MAX_CONVS;
constexpr int GRAD_MAX_SLAB_IDS = HMP_MAX_LAYERS * SLAB_IDS_PER_LAYER;
// one more id after the layers': the per-workgroup slabs of the linear heads (heads.hip, hmp_net_set_linear_heads)
constexpr int HEAD_SLAB_ID = GRAD_MAX_SLAB_IDS;
struct GradReduceDyn {  // passed by value: keep it small
  unsigned char n_slabs[GRAD_MAX_SLAB_IDS + 1];
  int slab_stride[GRAD_MAX_SLAB_IDS + 1];
};

// Static block -> work map of grad_reduce_kernel (FrontArgs::pack_map is the precedent): one line-aligned record per workgroup
// of the launch, built once per bound network from the segment table and resident in device memory.  A workgroup reads its own
// record with one wave-uniform request instead of searching a block table and walking a 216-byte GradSeg field by field.
//  GR_COPY  every term is GT_COPY: the record holds all a thread needs; element `first + threadIdx.x` of the segment, stored at
//           dst + threadIdx.x, threads >= n_live idle
//  GR_SEG   some term reads parameters (GT_ATT_OUTER*, or a dot product among several terms): thread per element as above, the
//           terms come from segs[seg]
//  GR_WAVE  one GT_ATT_DOT* term: a wavefront per element, 4 elements per workgroup from `first` on, through segs[seg]
enum { GR_COPY = 0, GR_SEG = 1, GR_WAVE = 2 };
struct GradRecTerm {
  int64_t src;  // GradTerm::src
  int ld, C, Cp;
  int slab_id;
  float scale;
  int pad_;
};
struct alignas(128) GradRec {
  int64_t dst;   // flat offset (gradient and parameter buffers) of the workgroup's first element
  int first;     // index of that element inside its segment
  int n_live;    // elements of the workgroup: 1 .. 256 (GR_WAVE: 1 .. 4)
  int cols;
  int kind;      // GR_*
  int seg;       // index into the GradSeg table
  int n_terms;
  GradRecTerm t[3];
};
static_assert(sizeof(GradRec) == 128 && sizeof(GradRecTerm) == 32, "a record is two 64-byte lines");

inline int grad_seg_kind(const GradSeg& g) {
  if (g.n_terms == 1 && (g.t[0].kind == GT_ATT_DOT || g.t[0].kind == GT_ATT_DOT_T)) return GR_WAVE;
  for (int ti = 0; ti < g.n_terms; ++ti)
    if (g.t[ti].kind != GT_COPY) return GR_SEG;
  return GR_COPY;
}
// workgroups of segment g: 256 elements each, 4 in wavefront-per-element mode
inline int64_t grad_seg_blocks(const GradSeg& g) {
  const int64_t el = (int64_t)g.rows * g.cols;
  const int per = grad_seg_kind(g) == GR_WAVE ? 4 : 256;
  return (el + per - 1) / per;
}
// Records of segments gs[0 .. n) in launch order into out[] (room for the sum of grad_seg_blocks); returns how many were
// written.  Host code without a HIP call: tools/grad_records_check.cpp runs it on the CPU.
inline int64_t grad_records_build(const GradSeg* gs, int n, GradRec* out) {
  int64_t nb = 0;
  for (int si = 0; si < n; ++si) {
    const GradSeg& g = gs[si];
    const int64_t el = (int64_t)g.rows * g.cols;
    const int kind = grad_seg_kind(g);
    const int per = kind == GR_WAVE ? 4 : 256;
    for (int64_t first = 0; first < el; first += per) {
      GradRec& R = out[nb++];
      memset(&R, 0, sizeof(R));
      R.dst = g.dst + first;
      R.first = (int)first;
      R.n_live = (int)(el - first < per ? el - first : per);
      R.cols = g.cols;
      R.kind = kind;
      R.seg = si;
      R.n_terms = g.n_terms;
      for (int ti = 0; ti < g.n_terms && kind == GR_COPY; ++ti) {
        const GradTerm& T = g.t[ti];
        GradRecTerm& Q = R.t[ti];
        Q.src = T.src; Q.ld = T.ld; Q.C = T.C; Q.Cp = T.Cp; Q.slab_id = T.slab_id; Q.scale = T.scale;
      }
    }
  }
  return nb;
}

// ---------------------------------------------------------------------------------------------
// K3: GAT edge softmax + aggregation
// ---------------------------------------------------------------------------------------------
constexpr int GAT_HMAX = 8;
constexpr int GAT_MAX_EDIM = 4;
// channels per head: up to 256 a lane of the row group owns one 4-channel slice per head, up to GAT_CMAX two -- with at most
// GAT_WIDE_HMAX heads, so that heads x slices stays within the register footprint of the 8-head class
constexpr int GAT_CMAX = 512;
constexpr int GAT_WIDE_HMAX = 4;
inline bool gat_shape_ok(int heads, int channels) {
  return heads >= 1 && heads <= GAT_HMAX && channels >= 1 && channels <= GAT_CMAX && (channels <= 256 || heads <= GAT_WIDE_HMAX);
}

// Static (per bound network) description of one GAT layer, resident in device memory: the by-value kernel
// argument budget (4 KB) cannot hold it.  Everything that changes with the batch travels in GatDyn.
struct GatInS {
  int et, src_t;
  const int *rowptr, *col, *eid, *t_rowptr, *t_col, *t_pos;
  const float* z;        // projected source rows: h_s (H*Cp) at column hoff
  int ldz, hoff;
  const float* za;       // rows holding a_s (H) at column asoff (the executor: za == z)
  int ldza, asoff;
  const float* zd;       // projected destination rows: a_d (H) at column adoff
  int ldzd, adoff;
  const float* vedge;    // [edim][GAT_HMAX] fold of att_edge into lin_edge, or null
  int edim;
  int self_loops;
  float *smax, *sden;    // [cap_dst, GAT_HMAX] per-row running max / softmax denominator (+1e-16)
  float adrop_p;
  uint32_t adrop_stream;
  float *alpha_drop, *dlogit;  // [cap_E + cap_loop, GAT_HMAX]   (backward)
  float* dlogit_orig;    // [cap_E, GAT_HMAX] original edge order (edge_attr convs only)
  float* dza_src;        // rows receiving d a_s at column asoff (the executor: the source dZ)
  int lddza_src;
  float* dz_dst;         // destination dZ (d a_d at adoff)
  int lddz_dst;
};
struct GatDstS {
  int t;
  int H, C, Cp, concat;
  float* out;
  int ldo;
  const float* bias;     // sum of the convs' biases, width of the output
  int act;
  float drop_p;
  uint32_t drop_stream;
  float group_scale;     // 1 (HeteroConv sum) or 1/n_convs (mean)
  const float* g;        // gradient of this layer's output for type t (null: taken from GatDyn.g_top)
  int ldg;
  int n_in;
  GatInS in[AGG_MAX_IN];
};
struct GatSrcS {
  int t;
  int n_out;
  struct { int d, i; } out[AGG_MAX_IN];  // (destination entry, in-conv index) pairs leaving this source type
  float* dz;
  int lddz;
};
struct GatLayerS {
  int n_dst, n_src;
  GatDstS d[HMP_MAX_NODE_TYPES];
  GatSrcS s[HMP_MAX_NODE_TYPES];
};
struct GatDyn {
  int n_nodes[HMP_MAX_NODE_TYPES];
  long long n_edges[HMP_MAX_EDGE_TYPES];
  const float* edge_attr[HMP_MAX_EDGE_TYPES];
  int block_start[HMP_MAX_NODE_TYPES + 1];
  const float* g_top;    // external output gradient (last layer / autograd path)
  int ld_gtop;
  int training;
  uint32_t k0, k1, step;
  const int* step_dev;
};
int gat_fwd_launch(const GatLayerS* d_tab, const GatLayerS& h_tab, GatDyn& dyn, hipStream_t st);
int gat_bwd1_launch(const GatLayerS* d_tab, const GatLayerS& h_tab, GatDyn& dyn, hipStream_t st);
int gat_bwd2_launch(const GatLayerS* d_tab, const GatLayerS& h_tab, GatDyn& dyn, hipStream_t st);

// Attention export (gat_attention_kernel): the coefficients the backward differentiates, alpha = expf(leaky(raw) - smax) / sden
// from the softmax state of the last forward, written out per conv in the CALLER's edge order, and / or the k entries of every
// destination row with the largest head-mean coefficient.  One launch serves the n requested convs of one layer; a request names
// its conv by (destination entry, in-conv index) of the layer table.  Passed by value next to GatDyn.
constexpr int GAT_ATT_KMAX = 8;
struct GatAttReq {
  int d, i;
  float* alpha;         // [E + n_loop][H] (no head padding): row e < E = edge e of the batch's edge_index, row E + r = the appended
                        // loop of row r; an explicit loop the conv removes and an edge the plan dropped hold 0.  null: skipped
  long long* top_src;   // [n_dst][k] source node of the k largest head means, descending, equal means by ascending CSR position
  float* top_w;         // [n_dst][k] those means; columns past the row's live entries hold -1 / 0.  Either may be null
  const int64_t* ei;    // the [2][E] list the plan was built from: its out-of-range edges (PlanJob's rule) get their alpha rows
                        // zeroed by sweep blocks.  null: the caller vouches that the plan dropped nothing
};
struct GatAttArgs {
  int n, k;
  int block_start[2 * HMP_MAX_EDGE_TYPES + 1];  // request q: row blocks from [2q], sweep blocks from [2q + 1] (filled by the launcher)
  GatAttReq r[HMP_MAX_EDGE_TYPES];
};
int gat_attention_launch(const GatLayerS* d_tab, const GatLayerS& h_tab, GatDyn& dyn, GatAttArgs& a, hipStream_t st);

// Gradient saliency (saliency.hip).  A row selection names the rows a launch serves: all, a byte per row, or -- ORDINAL -- row
// ptr[g] + p of every graph g of the batch with more than p rows (int64 ptr[n_graphs + 1], [PyG] Batch.ptr of the row's node type):
// rows of different graphs do not interact, so one pass per ordinal explains every graph's p-th row exactly.
constexpr int SAL_SEL_ALL = 0, SAL_SEL_MASK = 1, SAL_SEL_ORDINAL = 2;
constexpr int SAL_WRT_LOGIT = 0, SAL_WRT_LOGPROB = 1;
constexpr int SAL_MAX_GROUPS = 4;
constexpr int SAL_TOPK_MAX = 8;  // = GAT_ATT_KMAX: top_salient has top_attended's conventions
struct SalSel {
  int mode;
  const uint8_t* mask;
  int p;
  const int64_t* ptr;
  int n_graphs;
};
// gout[n_rows, ldg] (every element written, padding columns and unselected rows 0): onehot(c) or onehot(c) - softmax(z) per selected
// row, c = target[row] where given and in [0, n_classes), else the first-maximum argmax (predict_rows_launch's prediction)
// act != HMP_ACT_NONE: z is a pre-activation, the rule runs on y = act(z) and the row is multiplied by d y / d z (tail_dydz)
int saliency_seed_launch(const float* z, int ld, int n_rows, int n_classes, const int64_t* target, const SalSel& sel, int wrt, float* gout,
                         int ldg, hipStream_t st, int act = HMP_ACT_NONE);
// per row: gxi = sum_f g*x, gnorm = sqrt(sum_f g^2), groups[row, i] = sum of g*x over columns [lo[i], hi[i]) clipped to F; any output
// may be null.  lo / hi are HOST arrays
int saliency_scores_launch(const float* g, int ldg, const float* x, int ldx, int n_rows, int F, int n_groups, const int* lo, const int* hi,
                           float* gxi, float* gnorm, float* groups, hipStream_t st);
// per selected destination row of plan P: the k sources with the largest |score|, descending, equal magnitudes by ascending source,
// every source once; top_src / top_score [n_dst, k], -1 / 0 past the row's sources; unselected rows are left untouched
int saliency_topk_launch(const hmp_plan& P, const float* score, int k, const SalSel& sel, int64_t* top_src, float* top_score, hipStream_t st);

// Adam riding in the gradient un-pack (single-rank step of networks whose gradient terms read no parameters, i.e. SAGE):
// the thread that produced gradient element i updates parameter i right away.  count = valid labels (device), step = t.
struct AdamFuse {
  int on;
  float* p;
  float* m;
  float* v;
  float lr, b1, b2, eps, wd;
  const int* step_dev;
  const float* count;
};
// grad_reduce_kernel's one by-value argument.  What a workgroup needs to REQUEST its record and Adam's uniform words (recs, adam)
// fills the first two lines; the kernel warms all the others (karg_warm), dyn's among them, while the record is in flight
struct GradReduceArgs {
  const GradRec* recs;
  AdamFuse adam;
  const GradSeg* segs;
  const float* slabs;
  const float* params;
  float* grads;
  const float* row_lv;
  float* out2;
  NetState* state;
  int n_lv_rows;
  GradReduceDyn dyn;
};
static_assert(offsetof(GradReduceArgs, adam) + sizeof(AdamFuse) <= 128, "recs and adam: the two lines requested at entry");
// d_recs: the n_recs workgroup records of d_segs (grad_records_build), one workgroup each.
// row_lv != null: block (0,0) also sums the per-row {loss, valid} pairs (masked_ce_rows_launch) into out2 / state
int grad_reduce_launch(const GradSeg* d_segs, const GradRec* d_recs, int n_recs, const GradReduceDyn& dyn, const float* d_slabs,
                       const float* d_params, float* d_grads, const float* row_lv, int n_lv_rows, float* out2, NetState* state,
                       const AdamFuse& adam, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// loss / adam
// ---------------------------------------------------------------------------------------------
struct NetState {  // device resident
  int step;        // fused steps started so far (bumped by the pack kernel at the head of every step) -- the net's OWN counter;
                   // an optimiser that keeps Adam moments passes its own counter (hmp_train_args::d_step)
  int status;      // bit 0: edge endpoint out of range, bit 1: label out of range
  float loss_sum, count;
  int last_step;   // value of the counter the last started step ran on (its optimiser's, or `step`): what hmp_net_read_state reports
};
// w: class weights [n_classes], null: unweighted.  Weighted, a row's pair is {w[y] * nll, w[y]} and its gradient is scaled by w[y]
int masked_ce_launch(const float* logits, int ldl, int n_rows, int n_classes, const int64_t* labels, int64_t ignored,
                     float* grad, int ldg, float* out2, NetState* state_or_null, hipStream_t st, const float* w = nullptr);
int masked_ce_rows_launch(const float* logits, int ldl, int n_rows, int n_classes, const int64_t* labels, int64_t ignored,
                          float* grad, int ldg, float* row_lv, NetState* state, hipStream_t st, const float* w = nullptr);
// Tail of the two-headed task (semisup.hip): y = dropout(act(z)) on a final state, then the masked CE on y with the gradient written
// as d loss / d z (fused step), or the first-maximum argmax of act(z) compared with the labels (accuracy count).  One launch covers
// the rows of both heads.
struct HeadTail {
  const float* z;           // final state [n_rows][ldz] (output of the last conv, no activation)
  int ldz, n_rows, classes;
  const int64_t* labels;
  const uint8_t* mask;      // null: every row
  const float* weight;      // class weights [classes] (CE only), null: unweighted
  float* grad;              // d loss / d z [n_rows][ldg] (CE only; columns >= classes are written 0)
  int ldg;
  float* row_lv;            // per row {loss, valid} (CE only)
  int slot;                 // 0 readout, 1 aux: counts[2 * slot], counts[2 * slot + 1] (accuracy count)
  int drop_on;
  DropCfg drop;             // quad numbering row * ceil(classes / 4) + col / 4
  int block_start;
  // pooled heads (pool_tail_*_launch, hmp_net_set_head_pools): the CE / count rows are the n_pool rows of the pool edge type's
  // destination, each the mean of dropout(act(z)) over its leaves.  rowptr / col: the pool plan's CSR (by destination), t_rowptr /
  // t_col: its CSC (by leaf); rowptr null = identity (an unpooled head: row v's only leaf is v).  labels, mask and row_lv are per
  // pooled row; dpool [n_pool][ldp] is d loss / d pooled * (1 / deg), read back by the leaf-gradient launch.
  const int* rowptr;
  const int* col;
  const int* t_rowptr;
  const int* t_col;
  int n_pool;
  float* dpool;
  int ldp;
};
struct TailArgs {
  int n;
  int act;
  int64_t ignored;
  NetState* state;
  HeadTail h[2];
};
int tail_ce_launch(TailArgs& a, hipStream_t st);
int tail_count_launch(TailArgs& a, long long* counts, hipStream_t st);
constexpr int POOL_TAIL_MAX_CLASSES = 256;  // pooled rows are held in registers: at most 4 quads per lane
int pool_tail_ce_launch(TailArgs& a, hipStream_t st);
int pool_tail_grad_launch(TailArgs& a, hipStream_t st);
int pool_tail_count_launch(TailArgs& a, long long* counts, hipStream_t st);
// pred[i][row] = the prediction the count launches compare, for every row of entry i (pool: every pooled row; an empty one: 0);
// the entries need no labels, mask or row_lv, and a pooled entry no CSC
int tail_predict_launch(TailArgs& a, int64_t* const* pred, bool pool, hipStream_t st);
// Two learned linear heads over one final state (heads.hip): y = dropout(act(z)), logits_h = y W_h^T + b_h on the rows of head h,
// masked CE of both heads with d loss / d z written to `grad` and per-workgroup partial dW / db slabs (fused step), or the
// first-maximum argmax of both heads compared with the labels (accuracy count, eval mode).
constexpr int HEAD_MAX_CLASSES = 64;
constexpr int HEAD_MAX_F = 1024;
constexpr int HEAD_MAX_BLOCKS = 240;  // workgroups = slabs per element (GradReduceDyn::n_slabs is a byte); one per CU
struct LinHeadArgs {
  const float* z;               // final state [n_rows][ldz]
  int ldz, n_rows, F, K;        // K = classes[0] + classes[1]
  int classes[2];
  const float* W[2];            // [classes[h]][F] inside the flat parameters
  const float* bias[2];
  const int64_t* labels;        // one per row
  const uint8_t* mask;          // null: every row
  const uint8_t* member[2];     // rows of head h; member[1] null: complement of member[0]
  const float* weight[2];       // class weights of head h [classes[h]] (CE only), null: unweighted
  int64_t ignored;
  int act, drop_on;
  DropCfg drop;                 // quad numbering row * ceil(F / 4) + col / 4
  float* grad;                  // d loss / d z [n_rows][ldg] (columns F .. ldg written 0)
  int ldg;                      // == align4(F): the launch refuses any other (its column walk ends at roundup(F, 64))
  float* row_lv;                // per row {loss, valid} (both heads summed)
  NetState* state;
  float* slabs;                 // workgroup b: slabs + b * slab_stride = dW [K][ld_slab], then db [K]
  int ld_slab;
  int64_t slab_stride;
  unsigned long long* counts;   // accuracy count: {correct_0, total_0, correct_1, total_1}
  int64_t* pred[2];             // label output: pred[h][row], -1 outside head h's rows (null: head skipped)
  int n_tiles;
  int64_t* tk_labels[2];        // top-k output: [row][topk] per head (a head with both null is skipped)
  float* tk_probs[2];
  int topk;
  float* mc_acc[2];             // MC-dropout accumulators: [row][mc_ld[h]] per head (null: head skipped)
  int mc_ld[2];
  int mc_first;
};
int heads_blocks(int n_rows);
int linear_heads_ce_launch(LinHeadArgs& a, hipStream_t st);
int linear_heads_count_launch(LinHeadArgs& a, long long* counts, hipStream_t st);
int linear_heads_predict_launch(LinHeadArgs& a, int64_t* const* pred, hipStream_t st);

// Room-task validation count (evaluate.hip): first-maximum row argmax compared with the labels of the counted rows
// ((members == null || members[row]) && label != ignored); ACCUMULATES {correct, total} into counts and, with confusion != null,
// confusion[label][pred] for labels in [0, n_classes).  n_rows == 0 launches nothing.
int count_rows_launch(const float* x, int ld, int n_rows, int n_classes, const int64_t* labels, const uint8_t* members,
                      int64_t ignored, long long* counts, long long* confusion, hipStream_t st);
// the same rule per graph: counts[g] += {correct, total} over the rows [graph_ptr[g], graph_ptr[g + 1]) (int64 [n_graphs + 1])
int count_rows_by_graph_launch(const float* x, int ld, int n_rows, int n_classes, const int64_t* labels, const uint8_t* members,
                               int64_t ignored, const int64_t* graph_ptr, int n_graphs, long long* counts, hipStream_t st);

// pred[row] = first-maximum argmax of x[row, 0:n_classes) (count_rows_launch's prediction), -1 where members[row] == 0
int predict_rows_launch(const float* x, int ld, int n_rows, int n_classes, const uint8_t* members, int64_t* pred, hipStream_t st);

// Top-k labels with their softmax probabilities (tail_fns.h: topk_group), one launch next to each predict launch above: row-major
// labels [rows][k] int64 and probs [rows][k] float (either may be null, not both), 1 <= k <= TOPK_MAX.  Column 0 is the predict
// launch's label; columns at or past the class count, and every column of a row outside the head's rows, hold -1 / 0.
constexpr int TOPK_MAX = 8;
int topk_rows_launch(const float* x, int ld, int n_rows, int n_classes, const uint8_t* members, int k, int64_t* labels, float* probs,
                     hipStream_t st);
// by entry of the launch, as tail_predict_launch's pred; an entry with both pointers null must have no rows
int tail_topk_launch(TailArgs& a, int k, int64_t* const* labels, float* const* probs, bool pool, hipStream_t st);
// by head; a head with both pointers null is skipped
int linear_heads_topk_launch(LinHeadArgs& a, int k, int64_t* const* labels, float* const* probs, hipStream_t st);

// Monte-Carlo dropout accumulators (tail_fns.h: mc_group), one launch next to each top-k launch above, over the scores of ONE
// stochastic sample.  A row of an accumulator buffer [rows][ld_acc] holds, with Cp = align4(classes),
//   A[c] = sum_t p_t[c] at column c,  B[c] = sum_t p_t[c]^2 at column Cp + c  (c < classes),  E = sum_t h_t at column 2 * Cp;
// the columns [classes, Cp), [Cp + classes, 2 * Cp) and past 2 * Cp are never touched.  first != 0 stores the sample instead of
// adding it (the buffer needs no initialisation).  The row group that owns a row is its only writer: no atomics.
constexpr int MC_MAX_SAMPLES = 4096;
__host__ __device__ inline int mc_off_b(int classes) { return (classes + 3) & ~3; }
__host__ __device__ inline int mc_off_e(int classes) { return 2 * ((classes + 3) & ~3); }
inline int mc_acc_ld(int classes) { return mc_off_e(classes) + 4; }  // rows stay 16-byte aligned
int mc_rows_launch(const float* x, int ld, int n_rows, int n_classes, const uint8_t* members, int first, float* acc, int ld_acc,
                   hipStream_t st);
// labels / mean / std / entropy / mutual information of `samples` accumulated samples (any may be null, not all); rows outside
// `members` hold -1 / 0
int mc_finish_launch(const float* acc, int ld_acc, int n_rows, int n_classes, int samples, const uint8_t* members, int64_t* labels,
                     float* mean, int ld_mean, float* std, float* entropy, float* mi, hipStream_t st);
// by entry of the launch (the entries' drop_on / drop say whether and how the tail draws); an entry without accumulator must have no rows
int tail_mc_launch(TailArgs& a, int first, float* const* acc, const int* ld_acc, bool pool, hipStream_t st);
// by head; a head without accumulator is skipped.  a.drop_on / a.drop are the caller's
int linear_heads_mc_launch(LinHeadArgs& a, int first, float* const* acc, const int* ld_acc, hipStream_t st);

// step_dev != null: t = *step_dev is read on the device (graph replay); else t = step_host
int adam_launch(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                int step_host, const int* step_dev, const float* d_count, hipStream_t st);

}  // namespace hmp
