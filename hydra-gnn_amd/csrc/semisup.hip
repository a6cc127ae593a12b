// Tail of the two-headed (room + object) task: SemiSupervisedTrainingJob's loss (semisupervised_training_job.py:117-147) and
// the per-batch arithmetic of its test() (:198-257), for the node types whose last aggregation epilogue did not already serve them
// (GAT layers, wide outputs, the large-batch launch sequence).  Both heads are rows of ONE launch; a row belongs to a group of 16
// lanes, lane i owns the quads i, i + 16, ... of the row (classes <= 64: one quad per lane).
#include "kernels.h"

namespace hmp {

namespace {

constexpr int TL_GS = 16;
constexpr int TL_RPB = 256 / TL_GS;

// y = dropout(act(z)) of elements c .. c+3 (c % 4 == 0, c < classes) of `row`; the same arithmetic and keep-mask numbering as
// bias_act_drop_kernel (homog.hip): quad row * ceil(classes / 4) + c / 4
__device__ __forceinline__ void tail_quad(const HeadTail& T, const DropCfg& cfg, int act, int row, int c, float (&y)[4], bool (&in)[4]) {
  const float4 z4 = *reinterpret_cast<const float4*>(T.z + (int64_t)row * T.ldz + c);  // ldz % 4 == 0 and c + 3 < ldz
  bool keep[4] = {true, true, true, true};
  if (T.drop_on) drop_keep4(cfg, (uint32_t)row * (uint32_t)((T.classes + 3) >> 2) + (uint32_t)(c >> 2), keep);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    in[i] = c + i < T.classes;
    float v = (&z4.x)[i];
    if (act == HMP_ACT_RELU) v = fmaxf(v, 0.f);
    else if (act == HMP_ACT_ELU) v = v > 0.f ? v : expm1f(v);
    if (T.drop_on) v = keep[i] ? (v * cfg.scale + 0.0f) : -0.0f;
    else if (act != HMP_ACT_NONE) v = v + 0.0f;
    y[i] = in[i] ? v : -INFINITY;
  }
}

__device__ __forceinline__ int tail_entry(const TailArgs& a) { return (a.n > 1 && (int)blockIdx.x >= a.h[1].block_start) ? 1 : 0; }

__global__ __launch_bounds__(256) void tail_ce_kernel(const TailArgs a) {
  const HeadTail& T = a.h[tail_entry(a)];
  const int row = ((int)blockIdx.x - T.block_start) * TL_RPB + (int)threadIdx.x / TL_GS;
  if (row >= T.n_rows) return;  // whole row groups leave together: the shuffles below stay inside a group
  const int lane = threadIdx.x % TL_GS;
  const DropCfg cfg = T.drop_on ? drop_resolve(T.drop) : T.drop;
  const int64_t y = T.labels[row];
  const bool in_mask = T.mask ? T.mask[row] != 0 : true;
  float m = -INFINITY;
  for (int c = lane * 4; c < T.classes; c += TL_GS * 4) {
    float v[4];
    bool in[4];
    tail_quad(T, cfg, a.act, row, c, v, in);
#pragma unroll
    for (int i = 0; i < 4; ++i) m = fmaxf(m, v[i]);
  }
#pragma unroll
  for (int o = TL_GS / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f, ly = 0.f;
  for (int c = lane * 4; c < T.classes; c += TL_GS * 4) {
    float v[4];
    bool in[4];
    tail_quad(T, cfg, a.act, row, c, v, in);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!in[i]) continue;
      s += expf(v[i] - m);
      if ((int64_t)(c + i) == y) ly = v[i];
    }
  }
#pragma unroll
  for (int o = TL_GS / 2; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    ly += __shfl_xor(ly, o);
  }
  const float lse = m + logf(s);
  const bool valid = in_mask && y != a.ignored;
  const bool bad = valid && (y < 0 || y >= T.classes);
  const bool use = valid && !bad;
  for (int c = lane * 4; c < T.ldg; c += TL_GS * 4) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (use && c < T.classes) {
      float v[4];
      bool in[4];
      tail_quad(T, cfg, a.act, row, c, v, in);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (in[i]) (&g.x)[i] = (expf(v[i] - lse) - ((int64_t)(c + i) == y ? 1.f : 0.f)) * tail_dydz(v[i], a.act, T.drop_on != 0, cfg.scale);
    }
    *reinterpret_cast<float4*>(T.grad + (int64_t)row * T.ldg + c) = g;
  }
  if (lane == 0) {
    T.row_lv[2 * row] = use ? (lse - ly) : 0.f;
    T.row_lv[2 * row + 1] = use ? 1.f : 0.f;
    if (bad) atomicOr(&a.state->status, 2);
  }
}

__global__ __launch_bounds__(256) void tail_count_kernel(const TailArgs a, unsigned long long* __restrict__ counts) {
  __shared__ int s_correct, s_total;
  if (threadIdx.x == 0) { s_correct = 0; s_total = 0; }
  __syncthreads();
  const HeadTail& T = a.h[tail_entry(a)];
  const int row = ((int)blockIdx.x - T.block_start) * TL_RPB + (int)threadIdx.x / TL_GS;
  const int lane = threadIdx.x % TL_GS;
  if (row < T.n_rows) {
    // first maximum of act(z) (torch.argmax's rule; ReLU makes ties at 0): in-lane ascending, then the lowest index on equality
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int c = lane * 4; c < T.classes; c += TL_GS * 4) {
      float v[4];
      bool in[4];
      tail_quad(T, T.drop, a.act, row, c, v, in);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (in[i] && (v[i] > best || arg == 0x7fffffff)) { best = v[i]; arg = c + i; }
    }
#pragma unroll
    for (int o = TL_GS / 2; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oa = __shfl_xor(arg, o);
      if (oa != 0x7fffffff && (arg == 0x7fffffff || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
    }
    const bool in_mask = T.mask ? T.mask[row] != 0 : true;
    if (lane == 0 && in_mask) {
      atomicAdd(&s_total, 1);
      if ((int64_t)(arg == 0x7fffffff ? 0 : arg) == T.labels[row]) atomicAdd(&s_correct, 1);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_correct) atomicAdd(&counts[2 * T.slot], (unsigned long long)s_correct);
    if (s_total) atomicAdd(&counts[2 * T.slot + 1], (unsigned long long)s_total);
  }
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
#pragma unroll
    for (int q = 0; q < PT_Q; ++q) {
      const int c = lane * 4 + q * TL_GS * 4;
      if (c >= T.classes) continue;
      float y[4];
      bool in[4];
      tail_quad(T, cfg, act, leaf, c, y, in);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (in[i]) p[q][i] += y[i];
    }
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
  const int v = ((int)blockIdx.x - T.block_start) * TL_RPB + (int)threadIdx.x / TL_GS;
  if (v >= T.n_pool) return;  // whole row groups leave together
  const int lane = threadIdx.x % TL_GS;
  const DropCfg cfg = T.drop_on ? drop_resolve(T.drop) : T.drop;
  const int64_t y = T.labels[v];
  const bool in_mask = T.mask ? T.mask[v] != 0 : true;
  float p[PT_Q][4];
  const int deg = pool_row(T, cfg, a.act, v, lane, p);
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < PT_Q; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (lane * 4 + q * TL_GS * 4 + i < T.classes) m = fmaxf(m, p[q][i]);
#pragma unroll
  for (int o = TL_GS / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f, ly = 0.f;
#pragma unroll
  for (int q = 0; q < PT_Q; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane * 4 + q * TL_GS * 4 + i;
      if (c >= T.classes) continue;
      s += expf(p[q][i] - m);
      if ((int64_t)c == y) ly = p[q][i];
    }
#pragma unroll
  for (int o = TL_GS / 2; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    ly += __shfl_xor(ly, o);
  }
  const float lse = m + logf(s);
  const bool valid = in_mask && y != a.ignored;
  const bool bad = valid && (y < 0 || y >= T.classes);
  const bool use = valid && !bad;
  const float r = 1.0f / (float)(deg > 1 ? deg : 1);  // the mean's backward: every leaf edge carries 1 / max(deg, 1)
#pragma unroll
  for (int q = 0; q < PT_Q; ++q) {
    const int c = lane * 4 + q * TL_GS * 4;
    if (c >= T.ldp) continue;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (use) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c + i < T.classes) (&g.x)[i] = (expf(p[q][i] - lse) - ((int64_t)(c + i) == y ? 1.f : 0.f)) * r;
    }
    *reinterpret_cast<float4*>(T.dpool + (int64_t)v * T.ldp + c) = g;
  }
  if (lane == 0) {
    T.row_lv[2 * v] = use ? (lse - ly) : 0.f;
    T.row_lv[2 * v + 1] = use ? 1.f : 0.f;
    if (bad) atomicOr(&a.state->status, 2);
  }
}

__global__ __launch_bounds__(256) void pool_grad_kernel(const TailArgs a) {
  const HeadTail& T = a.h[tail_entry(a)];
  const int row = ((int)blockIdx.x - T.block_start) * TL_RPB + (int)threadIdx.x / TL_GS;
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
      bool in[4];
      tail_quad(T, cfg, a.act, row, c, y, in);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (in[i]) (&g.x)[i] = (&acc.x)[i] * tail_dydz(y[i], a.act, T.drop_on != 0, cfg.scale);
    }
    *reinterpret_cast<float4*>(T.grad + (int64_t)row * T.ldg + c) = g;
  }
}

__global__ __launch_bounds__(256) void pool_count_kernel(const TailArgs a, unsigned long long* __restrict__ counts) {
  __shared__ int s_correct, s_total;
  if (threadIdx.x == 0) { s_correct = 0; s_total = 0; }
  __syncthreads();
  const HeadTail& T = a.h[tail_entry(a)];
  const int v = ((int)blockIdx.x - T.block_start) * TL_RPB + (int)threadIdx.x / TL_GS;
  const int lane = threadIdx.x % TL_GS;
  if (v < T.n_pool) {
    float p[PT_Q][4];
    pool_row(T, T.drop, a.act, v, lane, p);
    // first maximum (tail_count_kernel's rule): in-lane ascending, then the lowest index on equality; an empty row is all 0 -> 0
    float best = -INFINITY;
    int arg = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < PT_Q; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = lane * 4 + q * TL_GS * 4 + i;
        if (c < T.classes && (p[q][i] > best || arg == 0x7fffffff)) { best = p[q][i]; arg = c; }
      }
#pragma unroll
    for (int o = TL_GS / 2; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oa = __shfl_xor(arg, o);
      if (oa != 0x7fffffff && (arg == 0x7fffffff || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
    }
    const bool in_mask = T.mask ? T.mask[v] != 0 : true;
    if (lane == 0 && in_mask) {
      atomicAdd(&s_total, 1);
      if ((int64_t)(arg == 0x7fffffff ? 0 : arg) == T.labels[v]) atomicAdd(&s_correct, 1);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_correct) atomicAdd(&counts[2 * T.slot], (unsigned long long)s_correct);
    if (s_total) atomicAdd(&counts[2 * T.slot + 1], (unsigned long long)s_total);
  }
}

// leaf = true: one row group per leaf row (gradient launch), else per pooled row
int pool_layout(TailArgs& a, bool leaf, bool ce, int& blocks) {
  blocks = 0;
  for (int i = 0; i < a.n; ++i) {
    HeadTail& T = a.h[i];
    HMP_CHECK_ARG(T.classes >= 1 && T.classes <= POOL_TAIL_MAX_CLASSES, "pool tail: %d classes (1 .. %d)", T.classes,
                  POOL_TAIL_MAX_CLASSES);
    HMP_CHECK_ARG((T.ldz & 3) == 0 && T.ldz >= T.classes && (reinterpret_cast<uintptr_t>(T.z) & 15) == 0,
                  "pool tail: final state must be 16-byte aligned with ld %% 4 == 0 and ld >= %d", T.classes);
    HMP_CHECK_ARG(T.rowptr ? (T.col && T.t_rowptr && T.t_col) : T.n_pool == T.n_rows,
                  "pool tail: a pooled head needs the plan's CSR and CSC, an unpooled one a row per leaf");
    if (ce) {
      HMP_CHECK_ARG(T.dpool && (T.ldp & 3) == 0 && T.ldp >= T.classes && (reinterpret_cast<uintptr_t>(T.dpool) & 15) == 0,
                    "pool tail: pooled gradient must be 16-byte aligned with ld %% 4 == 0");
      HMP_CHECK_ARG(T.grad && (T.ldg & 3) == 0 && T.ldg >= T.classes && T.ldg <= T.ldp &&
                        (reinterpret_cast<uintptr_t>(T.grad) & 15) == 0,
                    "pool tail: gradient must be 16-byte aligned with ld %% 4 == 0");
    }
    T.block_start = blocks;
    blocks += cdiv(leaf ? T.n_rows : T.n_pool, TL_RPB);
  }
  return HMP_OK;
}

int tail_layout(TailArgs& a, int& blocks) {
  blocks = 0;
  for (int i = 0; i < a.n; ++i) {
    HeadTail& T = a.h[i];
    HMP_CHECK_ARG(T.classes >= 1 && (T.ldz & 3) == 0 && T.ldz >= T.classes && (reinterpret_cast<uintptr_t>(T.z) & 15) == 0,
                  "tail: final state must be 16-byte aligned with ld %% 4 == 0 and ld >= %d", T.classes);
    HMP_CHECK_ARG(!T.grad || ((T.ldg & 3) == 0 && T.ldg >= T.classes && (reinterpret_cast<uintptr_t>(T.grad) & 15) == 0),
                  "tail: gradient must be 16-byte aligned with ld %% 4 == 0");
    T.block_start = blocks;
    blocks += cdiv(T.n_rows, TL_RPB);
  }
  return HMP_OK;
}

}  // namespace

int tail_ce_launch(TailArgs& a, hipStream_t st) {
  int blocks;
  HMP_TRY(tail_layout(a, blocks));
  if (blocks == 0) return HMP_OK;
  hipLaunchKernelGGL(tail_ce_kernel, dim3(blocks), dim3(256), 0, st, a);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int tail_count_launch(TailArgs& a, long long* counts, hipStream_t st) {
  int blocks;
  HMP_TRY(tail_layout(a, blocks));
  if (blocks == 0) return HMP_OK;
  hipLaunchKernelGGL(tail_count_kernel, dim3(blocks), dim3(256), 0, st, a, reinterpret_cast<unsigned long long*>(counts));
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int pool_tail_ce_launch(TailArgs& a, hipStream_t st) {
  int blocks;
  HMP_TRY(pool_layout(a, false, true, blocks));
  if (blocks == 0) return HMP_OK;
  hipLaunchKernelGGL(pool_ce_kernel, dim3(blocks), dim3(256), 0, st, a);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int pool_tail_grad_launch(TailArgs& a, hipStream_t st) {
  int blocks;
  HMP_TRY(pool_layout(a, true, true, blocks));
  if (blocks == 0) return HMP_OK;
  hipLaunchKernelGGL(pool_grad_kernel, dim3(blocks), dim3(256), 0, st, a);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int pool_tail_count_launch(TailArgs& a, long long* counts, hipStream_t st) {
  int blocks;
  HMP_TRY(pool_layout(a, false, false, blocks));
  if (blocks == 0) return HMP_OK;
  hipLaunchKernelGGL(pool_count_kernel, dim3(blocks), dim3(256), 0, st, a, reinterpret_cast<unsigned long long*>(counts));
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

}  // namespace hmp
