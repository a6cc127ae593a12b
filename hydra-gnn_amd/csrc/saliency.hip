// Gradient saliency: the three small launches around the executor's input-gradient path (net.hip: hmp_net_input_gradient).
//
//   saliency_seed_kernel    the output gradient that selects WHAT is explained: per selected output row onehot(c), or
//                           onehot(c) - softmax(z) for a log-probability, c = the caller's target or the row's prediction
//   saliency_scores_kernel  an input gradient reduced against its input, per node row: sum g*x, sqrt(sum g^2), sum g*x per column range
//   saliency_topk_kernel    per destination row of one edge type, the k sources with the largest |score|
//
// All three are small-row, latency-regime launches like the readout tails (evaluate.hip) and the attention export (gat.hip):
// a group of lanes owns a row, there is no LDS and no atomic, every reduction is an xor butterfly of fixed shape, so a rerun
// computes the same bits.  The seed shares the first-maximum argmax and the softmax association of tail_fns.h (its prediction IS
// predict_labels', its probabilities ARE topk_rows'), the top-k shares the selection network of topk_select.h with the
// attention export.
#include "tail_fns.h"
#include "topk_select.h"

namespace hmp {

namespace {

constexpr int SAL_GS = 16;              // lanes per row (seed, top-k): EV_GS / ATT_GS
constexpr int SAL_RPB = 256 / SAL_GS;   // rows per workgroup and pass
constexpr int SAL_MAX_BLOCKS = 1024;    // grid cap: larger inputs stride over rows

// Is `row` selected?  Uniform over the lanes of a row group.  ORDINAL: row == ptr[g] + p for the graph g that holds the row
// (the last g with ptr[g] <= row: empty graphs in front of it share its start and are skipped by the search).
__device__ __forceinline__ bool sal_selected(const SalSel& s, int row) {
  if (s.mode == SAL_SEL_ALL) return true;
  if (s.mode == SAL_SEL_MASK) return s.mask[row] != 0;
  int lo = 0, hi = s.n_graphs;  // invariant: ptr[lo] <= row (ptr[0] = 0), hi = first index known to have ptr[hi] > row (or G)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s.ptr[mid] <= (int64_t)row) lo = mid; else hi = mid;
  }
  if (s.n_graphs <= 0 || (int64_t)row >= s.ptr[lo + 1] || (int64_t)row < s.ptr[lo]) return false;  // a row behind the last graph
  return (int64_t)row - s.ptr[lo] == (int64_t)s.p;
}

// ---- seed -------------------------------------------------------------------------------------------------------------------------
// One group of 16 lanes per row.  The row's logits are walked as topk_rows_kernel's scalar form walks them (lane i owns the quads
// i, i + 16, ...), so max, argmax and the sum of expf have topk_group's association whatever the pitch.  act != none (the
// two-headed nets, whose outputs are act(final state)): the rule runs on y = act(z) and the row is chained through d y / d z.
__global__ __launch_bounds__(256) void saliency_seed_kernel(const float* __restrict__ z, int ld, int n_rows, int n_classes,
                                                            const int64_t* __restrict__ target, const SalSel sel, int wrt, int act,
                                                            float* __restrict__ gout, int ldg) {
  const int lane = threadIdx.x % SAL_GS;
  for (int row = blockIdx.x * SAL_RPB + (int)threadIdx.x / SAL_GS; row < n_rows; row += gridDim.x * SAL_RPB) {
    float* __restrict__ go = gout + (int64_t)row * ldg;
    if (!sal_selected(sel, row)) {  // the whole group takes the same branch
      for (int c = lane; c < ldg; c += SAL_GS) go[c] = 0.f;
      continue;
    }
    const float* __restrict__ zr = z + (int64_t)row * ld;
    auto quad = [&](int, int c, float (&v)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = c + i < n_classes ? act_drop(zr[c + i], act, false, true, 1.f) : 0.f;  // nothing past the classes is read
    };
    float best = -INFINITY;
    int arg = ARGMAX_NONE;
    lane_quads<SAL_GS, 0>(lane, n_classes, [&](int q, int c) {
      float v[4];
      quad(q, c, v);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c + i < n_classes) argmax_take(v[i], c + i, best, arg);
    });
    argmax_reduce_pair<SAL_GS>(best, arg);
    if (arg == ARGMAX_NONE) arg = 0;
    int cls = arg;
    if (target) {
      const int64_t t = target[row];
      if (t >= 0 && t < (int64_t)n_classes) cls = (int)t;
    }
    float s = 1.f;
    if (wrt == SAL_WRT_LOGPROB) {  // uniform
      s = 0.f;
      lane_quads<SAL_GS, 0>(lane, n_classes, [&](int q, int c) {
        float v[4];
        quad(q, c, v);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c + i < n_classes) s += expf(v[i] - best);
      });
#pragma unroll
      for (int o = SAL_GS / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    }
    for (int c = lane; c < ldg; c += SAL_GS) {
      float g = 0.f;
      if (c < n_classes) {
        const float y = act_drop(zr[c], act, false, true, 1.f);
        g = c == cls ? 1.f : 0.f;
        if (wrt == SAL_WRT_LOGPROB) g -= expf(y - best) / s;
        if (act != HMP_ACT_NONE) g *= tail_dydz(y, act, false, 1.f);
      }
      go[c] = g;
    }
  }
}

// ---- scores -----------------------------------------------------------------------------------------------------------------------
// One wavefront per row.  Lane i owns the columns i, i + 64, ... in ascending order (F = 306: five passes, the last one ragged);
// its fp32 partial sums go through a 64-lane xor butterfly.  All sums are always computed -- which outputs are stored does not
// reach the arithmetic -- and scalar 4-byte loads ask nothing of the pitches.
constexpr int SAL_WAVE = 64;
constexpr int SAL_WPB = 256 / SAL_WAVE;

struct SalRanges {
  int n;
  int lo[SAL_MAX_GROUPS], hi[SAL_MAX_GROUPS];
};

__global__ __launch_bounds__(256) void saliency_scores_kernel(const float* __restrict__ g, int ldg, const float* __restrict__ x, int ldx,
                                                              int n_rows, int F, const SalRanges rg, float* __restrict__ gxi,
                                                              float* __restrict__ gnorm, float* __restrict__ groups) {
  const int lane = threadIdx.x % SAL_WAVE;
  for (int row = blockIdx.x * SAL_WPB + (int)threadIdx.x / SAL_WAVE; row < n_rows; row += gridDim.x * SAL_WPB) {
    const float* __restrict__ gr = g + (int64_t)row * ldg;
    const float* __restrict__ xr = x + (int64_t)row * ldx;
    float a = 0.f, b = 0.f, r[SAL_MAX_GROUPS] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < F; c += SAL_WAVE) {
      const float gv = gr[c];
      const float p = gv * xr[c];
      a += p;
      b += gv * gv;
#pragma unroll
      for (int i = 0; i < SAL_MAX_GROUPS; ++i)
        if (i < rg.n && c >= rg.lo[i] && c < rg.hi[i]) r[i] += p;
    }
#pragma unroll
    for (int o = SAL_WAVE / 2; o > 0; o >>= 1) {
      a += __shfl_xor(a, o);
      b += __shfl_xor(b, o);
#pragma unroll
      for (int i = 0; i < SAL_MAX_GROUPS; ++i) r[i] += __shfl_xor(r[i], o);
    }
    if (lane == 0) {
      if (gxi) gxi[row] = a;
      if (gnorm) gnorm[row] = sqrtf(b);
      if (groups) {
#pragma unroll
        for (int i = 0; i < SAL_MAX_GROUPS; ++i)
          if (i < rg.n) groups[(int64_t)row * rg.n + i] = r[i];
      }
    }
  }
}

// ---- top-k ------------------------------------------------------------------------------------------------------------------------
// A group of 16 lanes per destination row, its lanes split the row's CSR entries (gat_attention_kernel's mapping).  Value = |score|
// of the entry's source, key = the source node: equal magnitudes list the lower source first, and a source reached by several
// edges is one candidate (topk_select.h).  Lane j stores column j: the source and its SIGNED score, -1 / 0 past the row's sources.
__global__ __launch_bounds__(256) void saliency_topk_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, int n_dst,
                                                            const float* __restrict__ score, int k, const SalSel sel,
                                                            long long* __restrict__ top_src, float* __restrict__ top_score) {
  const int row = (int)blockIdx.x * SAL_RPB + (int)threadIdx.x / SAL_GS;
  if (row >= n_dst) return;  // whole groups leave together: the shuffles below stay inside a group
  if (!sal_selected(sel, row)) return;
  const int gl = threadIdx.x % SAL_GS;
  float tv[SAL_TOPK_MAX];
  int tp[SAL_TOPK_MAX];
  topsel_init(tv, tp);
  const int b = rowptr[row], e = rowptr[row + 1];
  for (int i = b + gl; i < e; i += SAL_GS) {
    const int j = col[i];
    if (topsel_holds(tp, j)) continue;
    topsel_insert(tv, tp, fabsf(score[j]), j);
  }
  float rv;
  int rp;
  topsel_rounds<SAL_GS>(tv, tp, k, gl, rv, rp);
  if (gl < k) {
    const bool have = rp != INT_MAX;
    if (top_src) top_src[(int64_t)row * k + gl] = have ? (long long)rp : -1;
    if (top_score) top_score[(int64_t)row * k + gl] = have ? score[rp] : 0.f;
  }
}

int check_sel(const SalSel& s, const char* who) {
  HMP_CHECK_ARG(s.mode == SAL_SEL_ALL || s.mode == SAL_SEL_MASK || s.mode == SAL_SEL_ORDINAL, "%s: selection mode %d (0 all, 1 mask, 2 ordinal)",
                who, s.mode);
  HMP_CHECK_ARG(s.mode != SAL_SEL_MASK || s.mask, "%s: the mask selection needs a byte per row", who);
  HMP_CHECK_ARG(s.mode != SAL_SEL_ORDINAL || (s.ptr && s.n_graphs >= 0 && s.p >= 0),
                "%s: the ordinal selection needs graph_ptr, n_graphs >= 0 and ordinal >= 0", who);
  return HMP_OK;
}

}  // namespace

int saliency_seed_launch(const float* z, int ld, int n_rows, int n_classes, const int64_t* target, const SalSel& sel, int wrt, float* gout,
                         int ldg, hipStream_t st, int act) {
  HMP_CHECK_ARG(n_rows >= 0 && n_classes >= 1 && ld >= n_classes && ldg >= n_classes, "saliency_seed: n_rows %d, n_classes %d, ld %d, ld_g %d",
                n_rows, n_classes, ld, ldg);
  HMP_CHECK_ARG(wrt == SAL_WRT_LOGIT || wrt == SAL_WRT_LOGPROB, "saliency_seed: wrt = %d (0 logit, 1 log-probability)", wrt);
  HMP_CHECK_ARG(act >= HMP_ACT_NONE && act <= HMP_ACT_ELU, "saliency_seed: act = %d", act);
  if (n_rows == 0) return HMP_OK;  // (a mask over no rows has no address)
  HMP_TRY(check_sel(sel, "saliency_seed"));
  HMP_CHECK_ARG(z && gout, "saliency_seed: null logits or output");
  const int blocks = cdiv(n_rows, SAL_RPB) < SAL_MAX_BLOCKS ? cdiv(n_rows, SAL_RPB) : SAL_MAX_BLOCKS;
  hipLaunchKernelGGL(saliency_seed_kernel, dim3(blocks), dim3(256), 0, st, z, ld, n_rows, n_classes, target, sel, wrt, act, gout, ldg);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int saliency_scores_launch(const float* g, int ldg, const float* x, int ldx, int n_rows, int F, int n_groups, const int* lo, const int* hi,
                           float* gxi, float* gnorm, float* groups, hipStream_t st) {
  HMP_CHECK_ARG(n_rows >= 0 && F >= 1 && ldg >= F && ldx >= F, "saliency_scores: n_rows %d, F %d, ld_g %d, ld_x %d", n_rows, F, ldg, ldx);
  HMP_CHECK_ARG(n_groups >= 0 && n_groups <= SAL_MAX_GROUPS && (n_groups == 0 || (lo && hi)), "saliency_scores: %d column ranges (0 .. %d)",
                n_groups, SAL_MAX_GROUPS);
  HMP_CHECK_ARG(!groups || n_groups > 0, "saliency_scores: a groups output without column ranges");
  SalRanges rg;
  memset(&rg, 0, sizeof(rg));
  rg.n = n_groups;
  for (int i = 0; i < n_groups; ++i) {  // clipped to [0, F); lo >= hi: an empty range (its sum is 0)
    rg.lo[i] = lo[i] < 0 ? 0 : lo[i];
    rg.hi[i] = hi[i] > F ? F : hi[i];
  }
  if (n_rows == 0 || (!gxi && !gnorm && !groups)) return HMP_OK;
  HMP_CHECK_ARG(g && x, "saliency_scores: null gradient or input");
  const int blocks = cdiv(n_rows, SAL_WPB) < 4 * SAL_MAX_BLOCKS ? cdiv(n_rows, SAL_WPB) : 4 * SAL_MAX_BLOCKS;
  hipLaunchKernelGGL(saliency_scores_kernel, dim3(blocks), dim3(256), 0, st, g, ldg, x, ldx, n_rows, F, rg, gxi, gnorm, groups);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int saliency_topk_launch(const hmp_plan& P, const float* score, int k, const SalSel& sel, int64_t* top_src, float* top_score, hipStream_t st) {
  HMP_CHECK_ARG(k >= 1 && k <= SAL_TOPK_MAX, "saliency_topk: k = %d (1 .. %d)", k, SAL_TOPK_MAX);
  HMP_CHECK_ARG(P.n_dst >= 0 && P.n_src >= 0, "saliency_topk: plan with %d sources and %d destinations", P.n_src, P.n_dst);
  if (P.n_dst == 0 || (!top_src && !top_score)) return HMP_OK;
  HMP_TRY(check_sel(sel, "saliency_topk"));
  HMP_CHECK_ARG(P.d_rowptr && (P.n_edges == 0 || (P.d_col && score)), "saliency_topk: null plan lists or scores");
  hipLaunchKernelGGL(saliency_topk_kernel, dim3(cdiv(P.n_dst, SAL_RPB)), dim3(256), 0, st, P.d_rowptr, P.d_col, P.n_dst, score, k, sel,
                     reinterpret_cast<long long*>(top_src), top_score);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

}  // namespace hmp

using namespace hmp;

namespace {
SalSel make_sel(int32_t mode, const uint8_t* d_mask, int32_t ordinal, const int64_t* d_graph_ptr, int32_t n_graphs) {
  SalSel s;
  s.mode = mode; s.mask = d_mask; s.p = ordinal; s.ptr = d_graph_ptr; s.n_graphs = n_graphs;
  return s;
}
}  // namespace

extern "C" int hmp_saliency_seed(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const int64_t* d_target,
                                 int32_t sel_mode, const uint8_t* d_mask, int32_t ordinal, const int64_t* d_graph_ptr, int32_t n_graphs,
                                 int32_t wrt, float* d_gout, int32_t ld_g, void* stream) {
  return saliency_seed_launch(d_logits, ld, n_rows, n_classes, d_target, make_sel(sel_mode, d_mask, ordinal, d_graph_ptr, n_graphs), wrt,
                              d_gout, ld_g, (hipStream_t)stream);
}

extern "C" int hmp_saliency_scores(const float* d_g, int32_t ld_g, const float* d_x, int32_t ld_x, int32_t n_rows, int32_t n_features,
                                   int32_t n_groups, const int32_t* lo, const int32_t* hi, float* d_gxi, float* d_gnorm, float* d_groups,
                                   void* stream) {
  return saliency_scores_launch(d_g, ld_g, d_x, ld_x, n_rows, n_features, n_groups, lo, hi, d_gxi, d_gnorm, d_groups, (hipStream_t)stream);
}

extern "C" int hmp_saliency_topk(hmp_plan plan, const float* d_score, int32_t k, int32_t sel_mode, const uint8_t* d_mask, int32_t ordinal,
                                 const int64_t* d_graph_ptr, int32_t n_graphs, int64_t* d_top_src, float* d_top_score, void* stream) {
  return saliency_topk_launch(plan, d_score, k, make_sel(sel_mode, d_mask, ordinal, d_graph_ptr, n_graphs), d_top_src, d_top_score,
                              (hipStream_t)stream);
}
