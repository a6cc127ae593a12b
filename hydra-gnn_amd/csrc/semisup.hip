// Tail of the two-headed (room + object) task: SemiSupervisedTrainingJob's loss (semisupervised_training_job.py:117-147) and
// the per-batch arithmetic of its test() (:198-257), for the node types whose last aggregation epilogue did not already serve them
// (GAT layers, wide outputs, the large-batch launch sequence).  Both heads are rows of ONE launch; a row belongs to a group of 16
// lanes, lane i owns the quads i, i + 16, ... of the row (classes <= 64: one quad per lane).  The arithmetic of a row -- the
// activation and dropout, the masked CE and its association, the first-maximum argmax, the workgroup counters -- is tail_fns.h's;
// this file owns the row sources (a leaf row of the final state, a LeafPool mean of leaf rows), their keep-mask numbering and
// the launches.
#include "tail_fns.h"

namespace hmp {

namespace {

constexpr int TL_GS = 16;
constexpr int TL_RPB = 256 / TL_GS;

// y = dropout(act(z)) of elements c .. c+3 (c % 4 == 0, c < classes) of `row`; the keep-mask numbering of bias_act_drop_kernel
// (homog.hip): quad row * ceil(classes / 4) + c / 4.  Elements at or past `classes` hold padding: callers skip them.
__device__ __forceinline__ void tail_quad(const HeadTail& T, const DropCfg& cfg, int act, int row, int c, float (&y)[4]) {
  const float4 z4 = *reinterpret_cast<const float4*>(T.z + (int64_t)row * T.ldz + c);  // ldz % 4 == 0 and c + 3 < ldz
  bool keep[4] = {true, true, true, true};
  if (T.drop_on) drop_keep4(cfg, (uint32_t)row * (uint32_t)((T.classes + 3) >> 2) + (uint32_t)(c >> 2), keep);
  y[0] = z4.x; y[1] = z4.y; y[2] = z4.z; y[3] = z4.w;
  act_drop4(y, act, T.drop_on != 0, keep, cfg.scale);
}

__device__ __forceinline__ int tail_entry(const TailArgs& a) { return (a.n > 1 && (int)blockIdx.x >= a.h[1].block_start) ? 1 : 0; }
// the row of this thread's row group in entry T's launch range (whole row groups leave together: shuffles stay inside a group)
__device__ __forceinline__ int tail_row(const HeadTail& T) { return ((int)blockIdx.x - T.block_start) * TL_RPB + (int)threadIdx.x / TL_GS; }

__global__ __launch_bounds__(256) void tail_ce_kernel(const TailArgs a) {
  const HeadTail& T = a.h[tail_entry(a)];
  const int row = tail_row(T);
  if (row >= T.n_rows) return;
  const DropCfg cfg = T.drop_on ? drop_resolve(T.drop) : T.drop;
  const int64_t y = T.labels[row];
  const float wy = ce_weight(T.weight, y, T.classes);
  // any width: the row's quads are recomputed from z in each of the CE's passes
  ce_group<TL_GS, 0>(
      threadIdx.x % TL_GS, T.classes, T.ldg, y, a.ignored, T.mask ? T.mask[row] != 0 : true,
      [&](int, int c, float (&v)[4]) { tail_quad(T, cfg, a.act, row, c, v); },
      [&](int c, float (&g)[4], const float (&v)[4]) {  // y is what the CE read: chain back to z
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c + i < T.classes) g[i] *= tail_dydz(v[i], a.act, T.drop_on != 0, cfg.scale);
        *reinterpret_cast<float4*>(T.grad + (int64_t)row * T.ldg + c) = make_float4(g[0], g[1], g[2], g[3]);
      },
      T.row_lv, row, a.state, T.weight, wy);
}

// ---- pooled heads (HeterogeneousNeuralTreeNetwork, reference heterogeneous_neural_tree_network.py:186-205) ------------------
// The CE rows are the virtual nodes: pooled[v] = LeafPool(dropout(act(z)))[v], the mean over v's leaves.  The keep-mask is drawn
// on the LEAF rows with tail_quad's numbering (the masks forward() draws on the final states before its LeafPool).  The CE launch
// writes d loss / d pooled * (1 / deg) per virtual row; the leaf launch GATHERS it over each leaf's out-edges (the pool plan's CSC,
// a fixed order) and chains through tail_dydz.  No float atomics: a leaf with any number of pool edges, 0 and 2 included, is
// reproducible bit for bit.
constexpr int PT_Q = POOL_TAIL_MAX_CLASSES / (TL_GS * 4);  // quads per lane held in registers

// pooled row v, lane's quads c = lane * 4 + q * 64: the sum of the leaves' y in CSR order, then one IEEE division by max(deg, 1) --
// the arithmetic of segment_mean_fwd_kernel (aggregate.hip), which forward()'s LeafPool runs.  Returns deg.
__device__ __forceinline__ int pool_row(const HeadTail& T, const DropCfg& cfg, int act, int v, int lane, float (&p)[PT_Q][4]) {
  int b = v, e = v + 1;
  if (T.rowptr) { b = T.rowptr[v]; e = T.rowptr[v + 1]; }
#pragma unroll
  for (int q = 0; q < PT_Q; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i) p[q][i] = 0.f;
  for (int k = b; k < e; ++k) {
    const int leaf = T.rowptr ? T.col[k] : k;
    lane_quads<TL_GS, PT_Q>(lane, T.classes, [&](int q, int c) {
      float y[4];
      tail_quad(T, cfg, act, leaf, c, y);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c + i < T.classes) p[q][i] += y[i];
    });
  }
  const int deg = e - b;
  const float d = (float)(deg > 1 ? deg : 1);
#pragma unroll
  for (int q = 0; q < PT_Q; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i) p[q][i] = p[q][i] / d;
  return deg;
}

__global__ __launch_bounds__(256) void pool_ce_kernel(const TailArgs a) {
  const HeadTail& T = a.h[tail_entry(a)];
  const int v = tail_row(T);
  if (v >= T.n_pool) return;
  const int lane = threadIdx.x % TL_GS;
  const DropCfg cfg = T.drop_on ? drop_resolve(T.drop) : T.drop;
  const int64_t y = T.labels[v];
  const bool in_mask = T.mask ? T.mask[v] != 0 : true;
  const float wy = ce_weight(T.weight, y, T.classes);  // requested before the pool's gather
  float p[PT_Q][4];
  const int deg = pool_row(T, cfg, a.act, v, lane, p);
  const float r = 1.0f / (float)(deg > 1 ? deg : 1);  // the mean's backward: every leaf edge carries 1 / max(deg, 1)
  ce_group<TL_GS, PT_Q>(
      lane, T.classes, T.ldp, y, a.ignored, in_mask,
      [&](int q, int, float (&l)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) l[i] = p[q][i];
      },
      [&](int c, float (&g)[4], const float (&)[4]) {
        *reinterpret_cast<float4*>(T.dpool + (int64_t)v * T.ldp + c) = make_float4(g[0] * r, g[1] * r, g[2] * r, g[3] * r);
      },
      T.row_lv, v, a.state, T.weight, wy);
}

__global__ __launch_bounds__(256) void pool_grad_kernel(const TailArgs a) {
  const HeadTail& T = a.h[tail_entry(a)];
  const int row = tail_row(T);
  if (row >= T.n_rows) return;
  const int lane = threadIdx.x % TL_GS;
  const DropCfg cfg = T.drop_on ? drop_resolve(T.drop) : T.drop;
  int b = row, e = row + 1;
  if (T.rowptr) { b = T.t_rowptr[row]; e = T.t_rowptr[row + 1]; }
  for (int c = lane * 4; c < T.ldg; c += TL_GS * 4) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < T.classes) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = b; k < e; ++k) {  // the leaf's pool edges in CSC order
        const int v = T.rowptr ? T.t_col[k] : k;
        const float4 d = *reinterpret_cast<const float4*>(T.dpool + (int64_t)v * T.ldp + c);
        acc.x += d.x; acc.y += d.y; acc.z += d.z; acc.w += d.w;
      }
      float y[4];
      tail_quad(T, cfg, a.act, row, c, y);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c + i < T.classes) (&g.x)[i] = (&acc.x)[i] * tail_dydz(y[i], a.act, T.drop_on != 0, cfg.scale);
    }
    *reinterpret_cast<float4*>(T.grad + (int64_t)row * T.ldg + c) = g;
  }
}

// The prediction of row `row` of entry T (eval mode: T.drop is off) by its 16 lanes, every lane returns it: the first-maximum argmax
// of act(z) over a leaf row of any width, or POOL: over the LeafPool mean of the row's leaves (an empty row is all 0 and predicts 0)
template <bool POOL>
__device__ __forceinline__ int tail_pred(const HeadTail& T, int act, int row, int lane) {
  if constexpr (POOL) {
    float p[PT_Q][4];
    pool_row(T, T.drop, act, row, lane, p);
    return argmax_group<TL_GS, PT_Q>(lane, T.classes, [&](int q, int, float (&v)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = p[q][i];
    });
  } else {
    return argmax_group<TL_GS, 0>(lane, T.classes, [&](int, int c, float (&v)[4]) { tail_quad(T, T.drop, act, row, c, v); });
  }
}

// counts[2 * slot] += {#(argmax == label), #rows} over the masked rows of both entries
template <bool POOL>
__device__ __forceinline__ void tail_count(const TailArgs& a, unsigned long long* __restrict__ counts) {
  __shared__ int s_cnt[2];
  count_begin(s_cnt);
  const HeadTail& T = a.h[tail_entry(a)];
  const int row = tail_row(T);
  const int lane = threadIdx.x % TL_GS;
  if (row < (POOL ? T.n_pool : T.n_rows)) {
    const int pred = tail_pred<POOL>(T, a.act, row, lane);
    const bool in_mask = T.mask ? T.mask[row] != 0 : true;
    if (lane == 0 && in_mask) count_row(s_cnt, (int64_t)pred == T.labels[row]);
  }
  count_flush(s_cnt, counts + 2 * T.slot);
}

__global__ __launch_bounds__(256) void tail_count_kernel(const TailArgs a, unsigned long long* __restrict__ counts) { tail_count<false>(a, counts); }
__global__ __launch_bounds__(256) void pool_count_kernel(const TailArgs a, unsigned long long* __restrict__ counts) { tail_count<true>(a, counts); }

// pred[entry][row] = the row's prediction, for every row of both entries: the counts' arithmetic without labels, mask or counters
struct TailPred {
  int64_t* p[2];  // by entry of the launch
};

template <bool POOL>
__device__ __forceinline__ void tail_predict(const TailArgs& a, const TailPred& o) {
  const int e = tail_entry(a);
  const HeadTail& T = a.h[e];
  const int row = tail_row(T);
  if (row >= (POOL ? T.n_pool : T.n_rows)) return;
  int64_t* __restrict__ out = (e ? o.p[1] : o.p[0]) + row;  // independent of the walk below
  const int lane = threadIdx.x % TL_GS;
  const int pred = tail_pred<POOL>(T, a.act, row, lane);
  if (lane == 0) *out = (int64_t)pred;
}

__global__ __launch_bounds__(256) void tail_predict_kernel(const TailArgs a, const TailPred o) { tail_predict<false>(a, o); }
__global__ __launch_bounds__(256) void pool_predict_kernel(const TailArgs a, const TailPred o) { tail_predict<true>(a, o); }

// labels[entry][row][0:k) / probs[entry][row][0:k) = the k largest entries of the row tail_pred walks and their softmax
// probabilities (tail_fns.h: topk_group; column 0 is tail_pred's label), for every row of both entries.  A pooled row stays in
// registers over the rounds; a leaf row is recomputed from z in each.  An empty pooled row is all 0: labels 0 .. k - 1, each 1 / C.
struct TailTopk {
  int64_t* l[2];  // by entry of the launch
  float* p[2];
  int k;
};

template <bool POOL>
__device__ __forceinline__ void tail_topk(const TailArgs& a, const TailTopk& o) {
  const int e = tail_entry(a);
  const HeadTail& T = a.h[e];
  const int row = tail_row(T);
  if (row >= (POOL ? T.n_pool : T.n_rows)) return;
  // independent of the walk below
  int64_t* const lb = e ? o.l[1] : o.l[0];
  float* const pb = e ? o.p[1] : o.p[0];
  int64_t* const lo = lb ? lb + (int64_t)row * o.k : nullptr;
  float* const po = pb ? pb + (int64_t)row * o.k : nullptr;
  const int lane = threadIdx.x % TL_GS;
  if constexpr (POOL) {
    float p[PT_Q][4];
    pool_row(T, T.drop, a.act, row, lane, p);
    topk_group<TL_GS, PT_Q>(lane, T.classes, o.k, [&](int q, int, float (&v)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = p[q][i];
    }, lo, po);
  } else {
    topk_group<TL_GS, 0>(lane, T.classes, o.k, [&](int, int c, float (&v)[4]) { tail_quad(T, T.drop, a.act, row, c, v); }, lo, po);
  }
}

__global__ __launch_bounds__(256) void tail_topk_kernel(const TailArgs a, const TailTopk o) { tail_topk<false>(a, o); }
__global__ __launch_bounds__(256) void pool_topk_kernel(const TailArgs a, const TailTopk o) { tail_topk<true>(a, o); }

// One Monte-Carlo dropout sample of the rows tail_topk walks (tail_fns.h: mc_group), for every row of both entries: the softmax of
// dropout(act(z)) -- the tail draws as the CE kernels do, with the entry's drop -- or of its LeafPool mean is added to the row's
// accumulators acc[entry][row] (kernels.h: the layout).  An empty pooled row is all 0: p = 1 / C.
struct TailMc {
  float* acc[2];  // by entry of the launch
  int ld[2];
  int first;
};

template <bool POOL>
__device__ __forceinline__ void tail_mc(const TailArgs& a, const TailMc& o) {
  const int e = tail_entry(a);
  const HeadTail& T = a.h[e];
  const int row = tail_row(T);
  if (row >= (POOL ? T.n_pool : T.n_rows)) return;
  // independent of the walk below
  float* const ar = (e ? o.acc[1] : o.acc[0]) + (int64_t)row * (e ? o.ld[1] : o.ld[0]);
  const int lane = threadIdx.x % TL_GS;
  const DropCfg cfg = T.drop_on ? drop_resolve(T.drop) : T.drop;
  if constexpr (POOL) {
    float p[PT_Q][4];
    pool_row(T, cfg, a.act, row, lane, p);
    mc_group<TL_GS, PT_Q>(lane, T.classes, [&](int q, int, float (&v)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = p[q][i];
    }, o.first != 0, ar);
  } else {
    mc_group<TL_GS, 0>(lane, T.classes, [&](int, int c, float (&v)[4]) { tail_quad(T, cfg, a.act, row, c, v); }, o.first != 0, ar);
  }
}

__global__ __launch_bounds__(256) void tail_mc_kernel(const TailArgs a, const TailMc o) { tail_mc<false>(a, o); }
__global__ __launch_bounds__(256) void pool_mc_kernel(const TailArgs a, const TailMc o) { tail_mc<true>(a, o); }

// Checks the entries for a launch and lays their row groups out over the grid.  pool: the heads go through a LeafPool (rows in
// registers, CSR / CSC or the identity); leaf_rows: one row group per leaf row, else per pooled row; ce: the launch writes gradients;
// csc: the launch (or its companion) walks the pool plan by leaf -- the predict launch reads the CSR alone.
int tail_layout(TailArgs& a, bool pool, bool leaf_rows, bool ce, int& blocks, bool csc = true) {
  auto aligned = [](const float* p, int ld, int classes) { return (ld & 3) == 0 && ld >= classes && (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const char* who = pool ? "pool tail" : "tail";
  blocks = 0;
  for (int i = 0; i < a.n; ++i) {
    HeadTail& T = a.h[i];
    if (pool) HMP_CHECK_ARG(T.classes >= 1 && T.classes <= POOL_TAIL_MAX_CLASSES, "pool tail: %d classes (1 .. %d)", T.classes, POOL_TAIL_MAX_CLASSES);
    HMP_CHECK_ARG(T.classes >= 1 && aligned(T.z, T.ldz, T.classes),
                  "%s: final state must be 16-byte aligned with ld %% 4 == 0 and ld >= %d", who, T.classes);
    HMP_CHECK_ARG(!ce || (T.grad && aligned(T.grad, T.ldg, T.classes)), "%s: gradient must be 16-byte aligned with ld %% 4 == 0", who);
    if (pool) {
      HMP_CHECK_ARG(T.rowptr ? (T.col && (!csc || (T.t_rowptr && T.t_col))) : T.n_pool == T.n_rows,
                    "pool tail: a pooled head needs the plan's CSR and CSC, an unpooled one a row per leaf");
      HMP_CHECK_ARG(!ce || (T.dpool && aligned(T.dpool, T.ldp, T.classes) && T.ldg <= T.ldp),
                    "pool tail: pooled gradient must be 16-byte aligned with ld %% 4 == 0 and no narrower than the gradient");
    }
    T.block_start = blocks;
    blocks += cdiv(leaf_rows ? T.n_rows : T.n_pool, TL_RPB);
  }
  return HMP_OK;
}

template <class... Extra>
int tail_launch(void (*kernel)(TailArgs, Extra...), TailArgs& a, bool pool, bool leaf_rows, bool ce, bool csc, hipStream_t st,
                Extra... extra) {
  int blocks;
  HMP_TRY(tail_layout(a, pool, leaf_rows, ce, blocks, csc));
  if (blocks == 0) return HMP_OK;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, a, extra...);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

// the label launches: every entry has an output (has(i)) or no row to write
template <class Has>
int check_outputs(const TailArgs& a, bool pool, const char* what, Has has) {
  for (int i = 0; i < a.n; ++i)
    HMP_CHECK_ARG(has(i) || (pool ? a.h[i].n_pool : a.h[i].n_rows) == 0, "%s of entry %d", what, i);
  return HMP_OK;
}

unsigned long long* u64(long long* p) { return reinterpret_cast<unsigned long long*>(p); }

}  // namespace

int tail_ce_launch(TailArgs& a, hipStream_t st) { return tail_launch(tail_ce_kernel, a, false, true, true, true, st); }
int tail_count_launch(TailArgs& a, long long* counts, hipStream_t st) { return tail_launch(tail_count_kernel, a, false, true, false, true, st, u64(counts)); }
int pool_tail_ce_launch(TailArgs& a, hipStream_t st) { return tail_launch(pool_ce_kernel, a, true, false, true, true, st); }
int pool_tail_grad_launch(TailArgs& a, hipStream_t st) { return tail_launch(pool_grad_kernel, a, true, true, true, true, st); }
int pool_tail_count_launch(TailArgs& a, long long* counts, hipStream_t st) { return tail_launch(pool_count_kernel, a, true, false, false, true, st, u64(counts)); }

// labels of every row of the entries (leaf rows, or pool: pooled rows) into pred[entry]; the entries need no labels, mask or row_lv,
// and a pooled head no CSC (the launch reads the plan's CSR alone)
int tail_predict_launch(TailArgs& a, int64_t* const* pred, bool pool, hipStream_t st) {
  HMP_CHECK_ARG(pred != nullptr, "tail predict: null output array");
  TailPred o = {{nullptr, nullptr}};
  for (int i = 0; i < a.n; ++i) o.p[i] = pred[i];
  HMP_TRY(check_outputs(a, pool, "tail predict: null output", [&](int i) { return o.p[i] != nullptr; }));
  return tail_launch(pool ? pool_predict_kernel : tail_predict_kernel, a, pool, !pool, false, false, st, o);
}

// top-k labels and probabilities of every row of the entries (leaf rows, or pool: pooled rows); the layout and checks of
// tail_predict_launch
int tail_topk_launch(TailArgs& a, int k, int64_t* const* labels, float* const* probs, bool pool, hipStream_t st) {
  HMP_CHECK_ARG(labels != nullptr && probs != nullptr, "tail top-k: null output array");
  HMP_CHECK_ARG(k >= 1 && k <= TOPK_MAX, "tail top-k: k = %d (1 .. %d)", k, TOPK_MAX);
  TailTopk o = {{nullptr, nullptr}, {nullptr, nullptr}, k};
  for (int i = 0; i < a.n; ++i) { o.l[i] = labels[i]; o.p[i] = probs[i]; }
  HMP_TRY(check_outputs(a, pool, "tail top-k: no output", [&](int i) { return o.l[i] || o.p[i]; }));
  return tail_launch(pool ? pool_topk_kernel : tail_topk_kernel, a, pool, !pool, false, false, st, o);
}

// one Monte-Carlo dropout sample of every row of the entries (leaf rows, or pool: pooled rows) into acc[entry]; the layout and checks
// of tail_predict_launch
int tail_mc_launch(TailArgs& a, int first, float* const* acc, const int* ld_acc, bool pool, hipStream_t st) {
  HMP_CHECK_ARG(acc != nullptr && ld_acc != nullptr, "tail mc: null accumulator array");
  TailMc o = {{nullptr, nullptr}, {0, 0}, first};
  for (int i = 0; i < a.n; ++i) { o.acc[i] = acc[i]; o.ld[i] = ld_acc[i]; }
  HMP_TRY(check_outputs(a, pool, "tail mc: no accumulator", [&](int i) { return o.acc[i] != nullptr; }));
  for (int i = 0; i < a.n; ++i)
    HMP_CHECK_ARG(!o.acc[i] || o.ld[i] > mc_off_e(a.h[i].classes), "tail mc: ld_acc %d of entry %d (%d classes need more than %d)", o.ld[i], i,
                  a.h[i].classes, mc_off_e(a.h[i].classes));
  return tail_launch(pool ? pool_mc_kernel : tail_mc_kernel, a, pool, !pool, false, false, st, o);
}

}  // namespace hmp

// test / diagnostic entry of the five tail launchers: a plain copy of the descriptors into TailArgs, no choice of its own
// (d_w: the class weights of each head for the CE modes, null: unweighted)
static int head_tails_run(const hmp_tail_desc* d, int32_t n, const float* const* d_w, int32_t mode, int32_t act, int64_t ignored,
                          int32_t* d_state, int64_t* d_counts, void* stream) {
  using namespace hmp;
  static const bool have_device = hmp_device_count() > 0;
  HMP_CHECK_ARG(have_device, "hmp_head_tails: no gfx950 device visible");
  HMP_CHECK_ARG(d && (n == 1 || n == 2) && mode >= 0 && mode <= 3, "hmp_head_tails: %d heads (1 or 2), mode %d (0 .. 3)", n, mode);
  const bool ce = mode == 0 || mode == 2;
  HMP_CHECK_ARG(ce ? d_state != nullptr : d_counts != nullptr, "hmp_head_tails: mode %d needs %s", mode, ce ? "d_state" : "d_counts");
  TailArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.n = n; ta.act = act; ta.ignored = ignored;
  ta.state = reinterpret_cast<NetState*>(d_state);
  for (int i = 0; i < n; ++i) {
    const hmp_tail_desc& q = d[i];
    HMP_CHECK_ARG(q.z && (q.labels || q.n_rows == 0) && (!ce || q.row_lv), "hmp_head_tails: null pointer (head %d)", i);
    HeadTail& T = ta.h[i];
    T.z = q.z; T.ldz = q.ldz; T.n_rows = q.n_rows; T.classes = q.classes;
    T.labels = q.labels; T.mask = q.mask;
    if (ce && d_w) T.weight = d_w[i];
    T.grad = q.grad; T.ldg = q.ldg; T.row_lv = q.row_lv;
    T.slot = q.slot;
    T.rowptr = q.rowptr; T.col = q.col; T.t_rowptr = q.t_rowptr; T.t_col = q.t_col;
    T.n_pool = q.n_pool; T.dpool = q.dpool; T.ldp = q.ldp;
    T.drop_on = (ce && q.p > 0.f) ? 1 : 0;  // the counts run in eval mode (as net.hip: add_tail / add_pool)
    if (T.drop_on) {  // (as net.hip: make_drop)
      T.drop.k0 = (uint32_t)q.seed; T.drop.k1 = (uint32_t)(q.seed >> 32);
      T.drop.step = q.rng_step; T.drop.stream = q.rng_stream;
      T.drop.thresh = drop_thresh(q.p); T.drop.scale = 1.f / (1.f - q.p);
      T.drop.step_dev = nullptr;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  switch (mode) {
    case 0: return tail_ce_launch(ta, st);
    case 1: return tail_count_launch(ta, (long long*)d_counts, st);
    case 2: HMP_TRY(pool_tail_ce_launch(ta, st)); return pool_tail_grad_launch(ta, st);
    default: return pool_tail_count_launch(ta, (long long*)d_counts, st);
  }
}

extern "C" int hmp_head_tails(const hmp_tail_desc* d, int32_t n, int32_t mode, int32_t act, int64_t ignored, int32_t* d_state,
                              int64_t* d_counts, void* stream) {
  return head_tails_run(d, n, nullptr, mode, act, ignored, d_state, d_counts, stream);
}

extern "C" int hmp_head_tails_weighted(const hmp_tail_desc* d, int32_t n, const float* const* d_w, int32_t mode, int32_t act,
                                       int64_t ignored, int32_t* d_state, int64_t* d_counts, void* stream) {
  return head_tails_run(d, n, d_w, mode, act, ignored, d_state, d_counts, stream);
}

// the descriptors of a label / top-k launch (labels, mask, grad, row_lv and dpool may be NULL) as TailArgs, eval mode
static int label_tail_args(const char* who, const hmp_tail_desc* d, int32_t n, int32_t act, hmp::TailArgs& ta) {
  using namespace hmp;
  static const bool have_device = hmp_device_count() > 0;
  HMP_CHECK_ARG(have_device, "%s: no gfx950 device visible", who);
  HMP_CHECK_ARG(d && (n == 1 || n == 2), "%s: null argument or %d heads (1 or 2)", who, n);
  memset(&ta, 0, sizeof(ta));
  ta.n = n; ta.act = act;
  for (int i = 0; i < n; ++i) {
    const hmp_tail_desc& q = d[i];
    HMP_CHECK_ARG(q.z && q.n_rows >= 0 && q.n_pool >= 0, "%s: null state or negative rows (head %d)", who, i);
    HeadTail& T = ta.h[i];
    T.z = q.z; T.ldz = q.ldz; T.n_rows = q.n_rows; T.classes = q.classes;
    T.slot = q.slot;
    T.rowptr = q.rowptr; T.col = q.col; T.t_rowptr = q.t_rowptr; T.t_col = q.t_col;
    T.n_pool = q.n_pool;
  }
  return HMP_OK;
}

// the predict launchers on the same descriptors: d_pred[i] = int64 labels of head i's rows (pooled: of its n_pool rows), eval mode
extern "C" int hmp_head_tails_predict(const hmp_tail_desc* d, int32_t n, int32_t pooled, int32_t act, int64_t* const* d_pred, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_pred, "hmp_head_tails_predict: null output array");
  TailArgs ta;
  HMP_TRY(label_tail_args("hmp_head_tails_predict", d, n, act, ta));
  return tail_predict_launch(ta, d_pred, pooled != 0, (hipStream_t)stream);
}

// the top-k launchers on the same descriptors: d_labels[i] int64 [rows][k], d_probs[i] float [rows][k] of head i's rows
extern "C" int hmp_head_tails_topk(const hmp_tail_desc* d, int32_t n, int32_t pooled, int32_t act, int32_t k, int64_t* const* d_labels,
                                   float* const* d_probs, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_labels && d_probs, "hmp_head_tails_topk: null output array");
  TailArgs ta;
  HMP_TRY(label_tail_args("hmp_head_tails_topk", d, n, act, ta));
  return tail_topk_launch(ta, k, d_labels, d_probs, pooled != 0, (hipStream_t)stream);
}

// the Monte-Carlo launchers on the same descriptors, training mode: the tail draws at the descriptors' dropout site (p == 0: none)
extern "C" int hmp_head_tails_mc(const hmp_tail_desc* d, int32_t n, int32_t pooled, int32_t act, int32_t first, float* const* d_acc,
                                 const int32_t* ld_acc, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_acc && ld_acc, "hmp_head_tails_mc: null accumulator array");
  TailArgs ta;
  HMP_TRY(label_tail_args("hmp_head_tails_mc", d, n, act, ta));
  for (int i = 0; i < n; ++i) {
    const hmp_tail_desc& q = d[i];
    HMP_CHECK_ARG(q.p >= 0.f && q.p < 1.f, "hmp_head_tails_mc: p = %g (head %d)", (double)q.p, i);
    HeadTail& T = ta.h[i];
    T.drop_on = q.p > 0.f ? 1 : 0;
    if (T.drop_on) {  // (as net.hip: make_drop)
      T.drop.k0 = (uint32_t)q.seed; T.drop.k1 = (uint32_t)(q.seed >> 32);
      T.drop.step = q.rng_step; T.drop.stream = q.rng_stream;
      T.drop.thresh = drop_thresh(q.p); T.drop.scale = 1.f / (1.f - q.p);
      T.drop.step_dev = nullptr;
    }
  }
  return tail_mc_launch(ta, first, d_acc, ld_acc, pooled != 0, (hipStream_t)stream);
}
