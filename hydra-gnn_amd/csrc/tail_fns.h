// Readout bodies: what every "tail" behind the executor's last layer does to a row, written once (header-inline, like device_fns.h).
// They carry the engine's bit-level conventions, so a translation unit that needs one calls it here and keeps only its own layout:
//
//   act_drop / act_drop4   y = dropout(act(z)) and the sign-of-zero rule     aggregate.hip, gat.hip, semisup.hip, heads.hip, homog.hip
//   ce_group<GS, NQ>       masked softmax-CE of a row held by GS lanes       aggregate.hip (fused epilogue), semisup.hip (both CE kernels)
//   argmax_group<GS, NQ>,  first-maximum argmax of a row by GS lanes         evaluate.hip, optim.hip (argmax_rows_kernel), semisup.hip
//   argmax_take/_reduce
//   topk_group<GS, NQ>     the k largest entries and their softmax probabilities  evaluate.hip, semisup.hip, heads.hip (top-k kernels)
//   mc_group<GS, NQ>       one Monte-Carlo dropout sample: the row's softmax and entropy added to its accumulators  evaluate.hip, semisup.hip, heads.hip
//   count_begin/row/flush  a workgroup's {correct, total} pair in LDS        semisup.hip, evaluate.hip (count_rows_kernel)
//
// The backward form of act_drop, tail_dydz, is in common.h.
//
// Left alone on purpose, because their floating-point association differs and moving them would change their bits:
//   * ce_row (optim.hip): 64 lanes and scalar columns (the standalone loss entry and the unfused step);
//   * the CE and argmax of linear_heads_kernel (heads.hip): one thread per (row, head), sequential over the classes.
#pragma once
#include "kernels.h"

namespace hmp {

// ---- y = dropout(act(z)) ---------------------------------------------------------------------------------------------------------
// A dropped element is stored as -0.0f and every other zero as +0.0f ("+ 0.0f": a kept or undropped -0.0 becomes +0.0): numerically
// both are 0 for every consumer, and the backward pass (tail_dydz) reads the keep bit off the sign instead of regenerating the draws.
// `keep` is the element's keep bit and `scale` = 1 / (1 - p); both are ignored without dropout.  Which quad of which tensor the
// keep bits are drawn for (drop_keep4's numbering) is the caller's layout.
__device__ __forceinline__ float act_drop(float v, int act, bool drop_on, bool keep, float scale) {
  if (act == HMP_ACT_RELU) v = v > 0.f ? v : 0.f;
  else if (act == HMP_ACT_ELU) v = v > 0.f ? v : expm1f(v);
  if (drop_on) return keep ? (v * scale + 0.0f) : -0.0f;
  return act != HMP_ACT_NONE ? v + 0.0f : v;
}

// the same for 4 consecutive elements v[0 .. 3] with the keep bits of their quad
__device__ __forceinline__ void act_drop4(float* v, int act, bool drop_on, const bool (&keep)[4], float scale) {
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = act_drop(v[i], act, drop_on, keep[i], scale);
}

// ---- rows held by a group of GS lanes ---------------------------------------------------------------------------------------------
// Lane i owns the quads i, i + GS, ... of the row: columns c = 4 * (i + q * GS), q = 0, 1, ...  f(q, c) runs for the lane's quads
// below `width` in ascending order.  NQ > 0: the row has at most NQ quads per lane and the walk is unrolled (q is a constant: the
// caller can hold the quads in registers); NQ == 0: any width.
template <int GS, int NQ, class F>
__device__ __forceinline__ void lane_quads(int lane, int width, F&& f) {
  if constexpr (NQ > 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int c = (lane + q * GS) * 4;
      if (c < width) f(q, c);
    }
  } else {
    int q = 0;
    for (int c = lane * 4; c < width; c += GS * 4, ++q) f(q, c);
  }
}

// Masked cross entropy of one row (models/utils.py:143-148 with mask = in_mask && label != ignored).  quad(q, c, v) hands out the
// row's logits c .. c + 3 (elements at or past `classes` are not read); it is called once per pass, so a caller without the row in
// registers recomputes it.  put(c, g, v) receives d(SUM loss) / d logits of every quad below `ldg` -- 0 for a row that does not
// count and past `classes`, where v is 0 too -- and chains and stores it.  Lane 0 writes the row's {loss, valid} pair and raises
// status bit 1 for a label outside [0, classes).
// Class weights (F.cross_entropy(weight = w)): with w != null the caller hands in wy = ce_weight(w, y, classes), requested wherever
// its label arrives; the gradient quads are multiplied by wy before put and the pair becomes {wy * (lse - ly), wy}, so every
// consumer of {loss_sum, count} computes sum(w * nll) / sum(w).  A row of weight 0 does not count, exactly as an ignored one.
// w == null: wy is not looked at and the bits are those of the unweighted loss.
// Association: max, sum of expf and the label's logit accumulate per lane in ascending column order, then an xor butterfly below
// GS (inside the GS-aligned row group) -- the same whatever NQ, so every caller computes the same bits for the same row.
// w[y] of a label inside [0, classes) -- an unchecked label never indexes w (it has `classes` entries) -- and 1 without weights
__device__ __forceinline__ float ce_weight(const float* __restrict__ w, int64_t y, int classes) {
  return (w && y >= 0 && y < classes) ? w[y] : 1.f;
}

template <int GS, int NQ, class Quad, class Put>
__device__ __forceinline__ void ce_group(int lane, int classes, int ldg, int64_t y, int64_t ignored, bool in_mask, Quad&& quad, Put&& put,
                                         float* __restrict__ row_lv, int row, NetState* state, const float* w = nullptr, float wy = 1.f) {
  float m = -INFINITY;
  lane_quads<GS, NQ>(lane, classes, [&](int q, int c) {
    float v[4];
    quad(q, c, v);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (c + i < classes) m = fmaxf(m, v[i]);
  });
#pragma unroll
  for (int o = GS / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f, ly = 0.f;
  lane_quads<GS, NQ>(lane, classes, [&](int q, int c) {
    float v[4];
    quad(q, c, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (c + i >= classes) continue;
      s += expf(v[i] - m);
      if ((int64_t)(c + i) == y) ly = v[i];
    }
  });
#pragma unroll
  for (int o = GS / 2; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    ly += __shfl_xor(ly, o);
  }
  const float lse = m + logf(s);
  const bool valid = in_mask && y != ignored;
  const bool bad = valid && (y < 0 || y >= classes);
  const bool use = valid && !bad && !(w && wy == 0.f);
  lane_quads<GS, NQ>(lane, ldg, [&](int q, int c) {
    float g[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
    if (use && c < classes) {
      quad(q, c, v);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c + i < classes) g[i] = expf(v[i] - lse) - ((int64_t)(c + i) == y ? 1.f : 0.f);
      if (w) {
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] *= wy;
      }
    }
    put(c, g, v);
  });
  if (lane == 0) {
    row_lv[2 * row] = use ? (w ? wy * (lse - ly) : (lse - ly)) : 0.f;
    row_lv[2 * row + 1] = use ? (w ? wy : 1.f) : 0.f;
    if (bad && state) atomicOr(&state->status, 2);
  }
}

// First-maximum argmax (torch.argmax's rule on finite values; ReLU makes ties at 0): every lane walks its columns in ascending
// order and keeps the first maximum, the group reduction breaks ties by the lower index.  ARGMAX_NONE marks a lane that saw no
// column; a row without columns predicts 0.
constexpr int ARGMAX_NONE = 0x7fffffff;

__device__ __forceinline__ void argmax_take(float v, int c, float& best, int& arg) {
  if (v > best || arg == ARGMAX_NONE) { best = v; arg = c; }
}

// the group reduction in place: afterwards every lane holds the group's {best, arg} (arg ARGMAX_NONE: no lane saw a column)
template <int GS>
__device__ __forceinline__ void argmax_reduce_pair(float& best, int& arg) {
#pragma unroll
  for (int o = GS / 2; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, GS);
    const int oa = __shfl_xor(arg, o, GS);
    if (oa != ARGMAX_NONE && (arg == ARGMAX_NONE || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
  }
}

template <int GS>
__device__ __forceinline__ int argmax_reduce(float best, int arg) {
  argmax_reduce_pair<GS>(best, arg);
  return arg == ARGMAX_NONE ? 0 : arg;
}

// quad walk: quad(q, c, v) as in ce_group
template <int GS, int NQ, class Quad>
__device__ __forceinline__ int argmax_group(int lane, int classes, Quad&& quad) {
  float best = -INFINITY;
  int arg = ARGMAX_NONE;
  lane_quads<GS, NQ>(lane, classes, [&](int q, int c) {
    float v[4];
    quad(q, c, v);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (c + i < classes) argmax_take(v[i], c + i, best, arg);
  });
  return argmax_reduce<GS>(best, arg);
}

// (a row without the quads' alignment is walked by scalar columns i, i + GS, ... with argmax_take and reduced by argmax_reduce:
// the same prediction -- evaluate.hip, optim.hip)

// ---- top-k labels with their softmax probabilities ---------------------------------------------------------------------------------
// The k largest entries of a row in the total order "score descending, equal scores by ascending class" (+0.0 == -0.0), with
// probs[j] = expf(s[c_j] - m) / sum_c expf(s[c] - m).  Round j is the first-maximum argmax above (argmax_take, argmax_reduce_pair)
// restricted to the candidates behind pick j - 1 in that order, v < last_v || (v == last_v && c > last_c): it only compares, so the
// order is exact, it keeps no per-lane state that grows with k, and round 0 has no restriction -- column 0 IS argmax_group's
// prediction.  m is round 0's score (the row maximum; the sign of a zero maximum does not reach expf's result), the sum of expf
// accumulates with ce_group's association (per lane in ascending column order, then the xor butterfly below GS), so every caller
// computes the same bits for the same row.  quad(q, c, v) as in ce_group: it runs once per round and once for the sum, so a caller
// without the row in registers recomputes it.  Lane 0 stores columns [0, k) of `labels` / `probs` (the row's k entries; either may
// be null): columns at or past `classes` hold -1 / 0.  1 <= k; NaN scores are unspecified (as for the argmax) but store in bounds.
// columns [from, k) of a row hold -1 / 0 (lane 0 stores): the columns past the class count, or from = 0: a row outside the head's rows
__device__ __forceinline__ void topk_blank(int lane, int from, int k, int64_t* __restrict__ labels, float* __restrict__ probs) {
  if (lane != 0) return;
  for (int j = from; j < k; ++j) {
    if (labels) labels[j] = -1;
    if (probs) probs[j] = 0.f;
  }
}

template <int GS, int NQ, class Quad>
__device__ __forceinline__ void topk_group(int lane, int classes, int k, Quad&& quad, int64_t* __restrict__ labels, float* __restrict__ probs) {
  const int kk = k < classes ? k : classes;
  float last_v = 0.f, m = 0.f, s = 1.f;
  int last_c = -1;
  for (int j = 0; j < kk; ++j) {
    float best = -INFINITY;
    int arg = ARGMAX_NONE;
    lane_quads<GS, NQ>(lane, classes, [&](int q, int c) {
      float v[4];
      quad(q, c, v);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c + i < classes && (j == 0 || v[i] < last_v || (v[i] == last_v && c + i > last_c))) argmax_take(v[i], c + i, best, arg);
    });
    argmax_reduce_pair<GS>(best, arg);
    if (arg == ARGMAX_NONE) arg = 0;  // NaN scores only: j < classes leaves a candidate in every round otherwise
    if (j == 0) {
      m = best;
      s = 0.f;
      lane_quads<GS, NQ>(lane, classes, [&](int q, int c) {
        float v[4];
        quad(q, c, v);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c + i < classes) s += expf(v[i] - m);
      });
#pragma unroll
      for (int o = GS / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    }
    if (lane == 0) {
      if (labels) labels[j] = (int64_t)arg;
      if (probs) probs[j] = expf(best - m) / s;
    }
    last_v = best;
    last_c = arg;
  }
  topk_blank(lane, kk, k, labels, probs);
}

// ---- Monte-Carlo dropout: one stochastic sample of a row added to the row's accumulators ------------------------------------------
// p[c] = expf(s[c] - m) / sum_c' expf(s[c'] - m) with topk_group's m (the row maximum) and its sum -- per lane in ascending column
// order, then the xor butterfly below GS -- so p[c] has the bits topk_group stores for class c on the same scores;
// h = -sum_c p[c] * logf(p[c]) (a term with p[c] == 0 is 0) in the same association.  The row's accumulators (kernels.h: the
// layout, mc_off_b / mc_off_e) receive A[c] += p[c], B[c] += p[c] * p[c] from the lane that owns column c and E += h from lane 0;
// first: the sample is stored instead (what the buffer held, NaN included, is not read).  quad(q, c, v) as in ce_group: it runs
// once per pass (maximum, sum, probabilities), so a caller without the row in registers recomputes it.  NaN scores are
// unspecified but store in bounds.
template <int GS, int NQ, class Quad>
__device__ __forceinline__ void mc_group(int lane, int classes, Quad&& quad, bool first, float* __restrict__ acc) {
  float* const accb = acc + mc_off_b(classes);
  float* const acce = acc + mc_off_e(classes);
  float m = -INFINITY;
  lane_quads<GS, NQ>(lane, classes, [&](int q, int c) {
    float v[4];
    quad(q, c, v);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (c + i < classes) m = fmaxf(m, v[i]);
  });
#pragma unroll
  for (int o = GS / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f;
  lane_quads<GS, NQ>(lane, classes, [&](int q, int c) {
    float v[4];
    quad(q, c, v);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (c + i < classes) s += expf(v[i] - m);
  });
#pragma unroll
  for (int o = GS / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
  float h = 0.f;
  lane_quads<GS, NQ>(lane, classes, [&](int q, int c) {
    float v[4];
    quad(q, c, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (c + i >= classes) continue;
      const float p = expf(v[i] - m) / s;
      const float pp = p * p;
      h += p > 0.f ? p * logf(p) : 0.f;
      acc[c + i] = first ? p : acc[c + i] + p;
      accb[c + i] = first ? pp : accb[c + i] + pp;
    }
  });
#pragma unroll
  for (int o = GS / 2; o > 0; o >>= 1) h += __shfl_xor(h, o);
  if (lane == 0) *acce = first ? 0.f - h : *acce + (0.f - h);
}

// ---- a workgroup's {correct, total} pair ------------------------------------------------------------------------------------------
// s lives in LDS.  count_begin zeroes it (and is a barrier), count_row adds one counted row, count_flush (a barrier first) adds the
// non-zero counters to the 64-bit pair `out` with one atomic each.  Every thread of the workgroup calls begin and flush.
__device__ __forceinline__ void count_begin(int (&s)[2]) {
  if (threadIdx.x < 2) s[threadIdx.x] = 0;
  __syncthreads();
}
__device__ __forceinline__ void count_row(int (&s)[2], bool correct) {
  atomicAdd(&s[1], 1);
  if (correct) atomicAdd(&s[0], 1);
}
__device__ __forceinline__ void count_flush(int (&s)[2], unsigned long long* __restrict__ out) {
  __syncthreads();
  if (threadIdx.x < 2 && s[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)s[threadIdx.x]);
}

}  // namespace hmp
