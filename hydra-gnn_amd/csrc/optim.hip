// Loss, optimiser and the parameter <-> packed-operand shuffles around the layer kernels.
#include "device_fns.h"
#include "tail_fns.h"

namespace hmp {

// ---------------------------------------------------------------------------------------------
// masked cross entropy (models/utils.py:143-148 with mask = label != ignored).  grad is the gradient of the SUM
// loss.  Unit entry point: one block, one wavefront per row, fixed-order reductions => deterministic.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void ce_row(const float* __restrict__ lr, int n_classes, int64_t y, int64_t ignored, int lane,
                                       float* __restrict__ grow, int ldg, float& loss, float& valid, int& bad,
                                       const float* __restrict__ w) {
  // class weights (tail_fns.h: ce_group's rule): the pair is {w[y] * nll, w[y]}, the gradient is scaled by w[y], a row of weight
  // 0 does not count; w == null: the unweighted bits.  Requested first: it depends on the label alone.
  const float wy = ce_weight(w, y, n_classes);
  const bool is_valid = (y != ignored);
  if (is_valid && (y < 0 || y >= n_classes)) bad = 1;
  float m = -INFINITY;
  for (int c = lane; c < n_classes; c += 64) m = fmaxf(m, lr[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f;
  for (int c = lane; c < n_classes; c += 64) s += expf(lr[c] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float lse = m + logf(s);
  const bool use = is_valid && y >= 0 && y < n_classes && !(w && wy == 0.f);
  if (grow) {
    for (int c = lane; c < ldg; c += 64) {
      float g = 0.f;
      if (use && c < n_classes) {
        g = expf(lr[c] - lse) - (c == (int)y ? 1.f : 0.f);
        if (w) g *= wy;
      }
      grow[c] = g;
    }
  }
  loss = use ? (w ? wy * (lse - lr[y]) : (lse - lr[y])) : 0.f;
  valid = use ? (w ? wy : 1.f) : 0.f;
}

__global__ __launch_bounds__(1024) void masked_ce_kernel(const float* __restrict__ logits, int ldl, int n_rows, int n_classes,
                                                         const int64_t* __restrict__ labels, int64_t ignored, float* __restrict__ grad,
                                                         int ldg, float* __restrict__ out2, NetState* state,
                                                         const float* __restrict__ cw) {
  __shared__ float s_loss[16];
  __shared__ float s_cnt[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float loss = 0.f, cnt = 0.f;
  int bad = 0;
  for (int row = w; row < n_rows; row += 16) {
    float l, v;
    ce_row(logits + (int64_t)row * ldl, n_classes, labels[row], ignored, lane, grad ? grad + (int64_t)row * ldg : nullptr, ldg, l, v, bad, cw);
    loss += l;
    cnt += v;
  }
  if (lane == 0) { s_loss[w] = loss; s_cnt[w] = cnt; }
  if (bad && state) atomicOr(&state->status, 2);
  __syncthreads();
  if (threadIdx.x == 0) {
    float L = 0.f, C = 0.f;
    for (int i = 0; i < 16; ++i) { L += s_loss[i]; C += s_cnt[i]; }
    out2[0] = L;
    out2[1] = C;
    if (state) { state->loss_sum = L; state->count = C; }
  }
}

int masked_ce_launch(const float* logits, int ldl, int n_rows, int n_classes, const int64_t* labels, int64_t ignored, float* grad,
                     int ldg, float* out2, NetState* state, hipStream_t st, const float* w) {
  hipLaunchKernelGGL(masked_ce_kernel, dim3(1), dim3(1024), 0, st, logits, ldl, n_rows, n_classes, labels, ignored, grad, ldg, out2, state, w);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

// executor version: one wavefront per row over many blocks; per-row {loss, valid} go to row_lv[2*row ..] and are summed in
// fixed order by block (0,0) of the gradient un-pack kernel, which runs later in the same step anyway
__global__ __launch_bounds__(256) void masked_ce_rows_kernel(const float* __restrict__ logits, int ldl, int n_rows, int n_classes,
                                                             const int64_t* __restrict__ labels, int64_t ignored, float* __restrict__ grad,
                                                             int ldg, float* __restrict__ row_lv, NetState* state,
                                                             const float* __restrict__ cw) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  float l, v;
  int bad = 0;
  ce_row(logits + (int64_t)row * ldl, n_classes, labels[row], ignored, lane, grad + (int64_t)row * ldg, ldg, l, v, bad, cw);
  if (lane == 0) {
    row_lv[2 * row] = l;
    row_lv[2 * row + 1] = v;
    if (bad) atomicOr(&state->status, 2);
  }
}

int masked_ce_rows_launch(const float* logits, int ldl, int n_rows, int n_classes, const int64_t* labels, int64_t ignored, float* grad,
                          int ldg, float* row_lv, NetState* state, hipStream_t st, const float* w) {
  if (n_rows == 0) return HMP_OK;
  hipLaunchKernelGGL(masked_ce_rows_kernel, dim3(cdiv(n_rows, 4)), dim3(256), 0, st, logits, ldl, n_rows, n_classes, labels, ignored,
                     grad, ldg, row_lv, state, w);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

// ---------------------------------------------------------------------------------------------
// row argmax: the `.argmax(dim=1)` of the inference server (bin/room_classification_server:286); 16 lanes per row, the
// first-maximum rule of tail_fns.h, labels as int64 so the buffer can be handed to the caller as is
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ x, int ld, int n_rows, int n_cols,
                                                          int64_t* __restrict__ out) {
  const int row = blockIdx.x * 16 + ((int)threadIdx.x >> 4);
  const int lane = threadIdx.x & 15;
  float best = -INFINITY;
  int arg = ARGMAX_NONE;
  if (row < n_rows)  // rows past the end walk no column: every lane of the wavefront reaches the group's shuffles
    for (int c = lane; c < n_cols; c += 16) argmax_take(x[(int64_t)row * ld + c], c, best, arg);
  arg = argmax_reduce<16>(best, arg);
  if (row < n_rows && lane == 0) out[row] = arg;
}

// ---------------------------------------------------------------------------------------------
// Adam with coupled L2 (torch.optim.Adam semantics, base_training_job.py:181-185)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                                                   int step_host, const int* __restrict__ step_dev, const float* __restrict__ d_count) {
  const int t = step_dev ? *step_dev : step_host;
  const float bc1 = 1.f - powf(b1, (float)t);
  const float bc2 = 1.f - powf(b2, (float)t);
  const float step_size = lr / bc1;
  const float bc2_sqrt = sqrtf(bc2);
  float gscale = 1.f;
  if (d_count) {
    const float c = *d_count;
    gscale = 1.f / (c > 0.f ? c : 1.f);  // a weight sum below 1 is a normaliser too; integer counts: the same bits
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float pi = p[i];
    const float gi = g[i] * gscale + wd * pi;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi - step_size * (mi / denom);
  }
}

int adam_launch(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                int step_host, const int* step_dev, const float* d_count, hipStream_t st) {
  if (n == 0) return HMP_OK;
  const int64_t want = cdiv(n, 256);
  const int grid = (int)(want > 2048 ? 2048 : want);
  hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, lr, b1, b2, eps, wd, step_host, step_dev, d_count);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

// ---------------------------------------------------------------------------------------------
// dropout keep-mask export (tests replay the engine's masks in the oracle)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dropout_mask_kernel(DropCfg cfg, int n_rows, int F, uint8_t* __restrict__ mask) {
  const int qpr = (F + 3) >> 2;  // quads per row of the padded row
  const int64_t total = (int64_t)n_rows * qpr;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(q / qpr), c = (int)(q % qpr) * 4;
    bool keep[4];
    drop_keep4(cfg, (uint32_t)q, keep);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (c + i < F) mask[(int64_t)row * F + c + i] = keep[i] ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------
// pack: flat parameters -> per-(layer, source type) stacked weight operand.  grid = (row chunks, segments): a block
// reads its segment descriptor once and writes 4 packed rows (64 lanes per row).  Block (0,0) also starts the step:
// it bumps the device step counter that dropout and Adam read later in the same step.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_kernel(const PackSeg* __restrict__ segs, const SegBlocks sb, const float* __restrict__ params,
                                                   float* __restrict__ packed, int* step_ctr, int* step_mirror) {
  pack_block(segs, sb, params, packed, step_ctr, step_mirror, (int)blockIdx.x);
}

int pack_launch(const PackSeg* d_segs, const SegBlocks& sb, const float* d_params, float* d_packed, int* step_ctr, int* step_mirror,
                hipStream_t st) {
  if (sb.n == 0 || sb.start[sb.n] == 0) return HMP_OK;
  hipLaunchKernelGGL(pack_kernel, dim3(sb.start[sb.n]), dim3(256), 0, st, d_segs, sb, d_params, d_packed, step_ctr, step_mirror);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

// ---------------------------------------------------------------------------------------------
// grad reduce: split-K slabs of the packed weight gradients -> flat gradient buffer (fixed slab order), one workgroup per
// record of the bind-time table (kernels.h GradRec).  Block 0 additionally sums the per-row {loss, valid} pairs of the
// loss kernel in fixed order into out2 = {loss_sum, count} (the tail of the flat gradient buffer).
//
// All workgroups of the launch are co-resident, so the launch is as long as its longest chain of dependent requests, and the
// chain is kept short: [kernel arguments] -> [record; the lines of `dyn` and Adam's two uniform words ride the same trip] ->
// [p, m, v and every slab value of the element, GR_BATCH per term] -> stores.  Nothing is consumed before all of it is
// requested; the sums are then taken in the order they always were: slab 0 first, one running sum per term, terms in index order.
// ---------------------------------------------------------------------------------------------
KT_DEFINE(optim)
#ifdef HMP_KTIME
// stamps of thread 0: workgroup 0 into slots 0.., the selected workgroup into slots 8.. (tools/ktime_grad.py); the first
// workgroups of a 16-slab and of an 8-slab segment leave their index in slots 20 / 21 for the selection
#define GKT(i)                                                              \
  do {                                                                      \
    if (threadIdx.x == 0) {                                                 \
      if (blockIdx.x == 0) kt_buf[i] = wall_clock64();                      \
      else if ((int)blockIdx.x == kt_sel) kt_buf[8 + (i)] = wall_clock64(); \
    }                                                                       \
  } while (0)
#define GKT_NOTE(first, ns)                                                          \
  do {                                                                               \
    if (threadIdx.x == 0 && (first) && ((ns) == 16 || (ns) == 8) && blockIdx.x != 0) \
      atomicMin(&kt_buf[(ns) == 16 ? 20 : 21], (unsigned long long)blockIdx.x);      \
  } while (0)
#else
#define GKT(i) \
  do {         \
  } while (0)
#define GKT_NOTE(first, ns) \
  do {                      \
  } while (0)
#endif

// dyn.n_slabs[id], read as the 32-bit word around it: there is no scalar byte load, and a byte indexed by a loaded id would
// come through the vector path -- a round trip of its own that also waits for every load requested before it
__device__ __forceinline__ int dyn_n_slabs(const GradReduceDyn& dyn, int id) {
  static_assert(offsetof(GradReduceDyn, slab_stride) >= ((GRAD_MAX_SLAB_IDS + 4) & ~3), "the last byte's word lies inside the struct");
  const unsigned w = reinterpret_cast<const unsigned*>(dyn.n_slabs)[id >> 2];
  return (int)((w >> ((id & 3) * 8)) & 0xffu);
}

// sum over the split-K slabs of one element, slab 0 first; 8 (clamped) loads in flight per trip instead of one dependent
// load per slab (the segments that go through the GradSeg table)
__device__ __forceinline__ float slab_sum(const float* __restrict__ src, int ns, int64_t stride) {
  float v = 0.f;
  for (int z0 = 0; z0 < ns; z0 += 8) {
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = src[(int64_t)min(z0 + u, ns - 1) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (z0 + u < ns) v += t[u];
  }
  return v;
}

// element (r, c) of a segment with parameter-reading terms, term by term from the segment table
__device__ __forceinline__ float seg_terms(const GradSeg& S, const GradReduceDyn& dyn, const float* __restrict__ slabs,
                                           const float* params, int r, int c) {
  float total = 0.f;
  for (int ti = 0; ti < S.n_terms; ++ti) {
    const GradTerm& T = S.t[ti];
    const int ns = dyn_n_slabs(dyn, T.slab_id);
    const int64_t stride = dyn.slab_stride[T.slab_id];
    const float* base = slabs + T.src;
    float v = 0.f;
    if (T.kind == GT_COPY) {
      v = slab_sum(base + (int64_t)((r / T.C) * T.Cp + (r % T.C)) * T.ld + c, ns, stride);
    } else if (T.kind == GT_ATT_OUTER) {
      v = params[T.att + r] * slab_sum(base + (int64_t)(r / T.C) * T.ld + c, ns, stride);
    } else if (T.kind == GT_ATT_DOT) {
      const float* src = base + (int64_t)(r / T.C) * T.ld;
      const float* w = params + T.w + (int64_t)r * T.ldw;
      for (int f = 0; f < T.inner; ++f) {
        float s = 0.f;
        for (int z = 0; z < ns; ++z) s += src[z * stride + f];
        v += s * w[f];
      }
    } else if (T.kind == GT_ATT_OUTER_T) {
      v = params[T.att + r] * slab_sum(base + (int64_t)c * T.ld + (r / T.C), ns, stride);
    } else {  // GT_ATT_DOT_T
      const float* w = params + T.w + (int64_t)r * T.ldw;
      for (int d = 0; d < T.inner; ++d) {
        float s = 0.f;
        for (int z = 0; z < ns; ++z) s += base[z * stride + (int64_t)d * T.ld + (r / T.C)];
        v += s * w[d];
      }
    }
    total += v * T.scale;
  }
  return total;
}

constexpr int GR_BATCH = 16;  // slab values of one term in flight per lane: what the small-batch launcher writes at most

__global__ __launch_bounds__(256) void grad_reduce_kernel(const GradReduceArgs a) {
  GKT(0);
  const GradReduceDyn& dyn = a.dyn;
  const AdamFuse& adam = a.adam;
  const GradSeg* __restrict__ segs = a.segs;
  const float* __restrict__ slabs = a.slabs;
  const float* params = a.params;
  float* __restrict__ grads = a.grads;
  // the record: two lines behind one wave-uniform pointer, every field requested here
  const GradRec* __restrict__ Rp = a.recs + blockIdx.x;
  const int64_t dst = Rp->dst;
  const int first = Rp->first, n_live = Rp->n_live, cols = Rp->cols, kind = Rp->kind, seg = Rp->seg, n_terms = Rp->n_terms;
  GradRecTerm Q[3];
#pragma unroll
  for (int ti = 0; ti < 3; ++ti) Q[ti] = Rp->t[ti];
  // Adam's two uniform words travel with the record: requested without a branch (adam.on is kernel-uniform; off: a word of the
  // record stands in for the load and is not used) ...
  const float* cnt_p = adam.on ? adam.count : (const float*)Rp;
  const int* step_p = adam.on ? adam.step_dev : (const int*)Rp;
  const float cnt_w = *cnt_p;
  const int step_w = *step_p;
  // ... and so do the other lines of the argument struct: the pointers, and dyn, which the record's slab ids index next
  constexpr int WARM_OFF = 128, WARM_BYTES = (int)sizeof(GradReduceArgs) - WARM_OFF;
  karg_warm<(WARM_BYTES + 63) / 64 + 1>(WARM_OFF, WARM_BYTES);
  const float a_cnt = adam.on ? cnt_w : 1.f;
  const int a_t = adam.on ? step_w : 1;
  asm volatile("" ::"s"(kind), "s"(n_live));
  GKT(1);
  if (kind == GR_WAVE) {
    // attention-vector gradients are long dot products: one WAVEFRONT per element, lanes over the reduction index
    const GradSeg& S = segs[seg];
    const GradTerm& T = S.t[0];
    const int w4 = threadIdx.x >> 6;
    const int64_t r = (int64_t)first + w4;
    const int lane = threadIdx.x & 63;
    if (w4 < n_live) {
      const int ns = dyn_n_slabs(dyn, T.slab_id);
      const int64_t stride = dyn.slab_stride[T.slab_id];
      const float* w = params + T.w + r * T.ldw;
      float part = 0.f;
      if (T.kind == GT_ATT_DOT) {
        const float* src = slabs + T.src + (int64_t)(r / T.C) * T.ld;
        for (int f = lane; f < T.inner; f += 64) part += slab_sum(src + f, ns, stride) * w[f];
      } else {
        const float* base = slabs + T.src + (r / T.C);
        for (int d = lane; d < T.inner; d += 64) part += slab_sum(base + (int64_t)d * T.ld, ns, stride) * w[d];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
      if (lane == 0) grads[S.dst + r] = part * T.scale;
    }
  } else if ((int)threadIdx.x < n_live) {
    const int i = first + (int)threadIdx.x;  // element of the segment
    const int r = i / cols, c = i - r * cols;
    const int64_t e = dst + threadIdx.x;     // element of the flat buffers
    // Adam state of this element, requested before the slab values so that it travels with them
    float a_p = 0.f, a_m = 0.f, a_v = 0.f;
    if (adam.on) {
      a_p = adam.p[e]; a_m = adam.m[e]; a_v = adam.v[e];
    }
    // GR_COPY: the first GR_BATCH slab values of every term, all requested before any is used (clamped addresses: a term of
    // fewer slabs re-reads its last one, the sums below skip it)
    float tv[3][GR_BATCH];
    const float* src[3];
    int ns[3];
    int64_t stride[3];
    if (kind == GR_COPY) {
#pragma unroll
      for (int ti = 0; ti < 3; ++ti) {
        ns[ti] = 0;
        if (ti < n_terms) {
          ns[ti] = dyn_n_slabs(dyn, Q[ti].slab_id);
          stride[ti] = dyn.slab_stride[Q[ti].slab_id];
          const int row = Q[ti].C == Q[ti].Cp ? r : (r / Q[ti].C) * Q[ti].Cp + (r % Q[ti].C);
          src[ti] = slabs + Q[ti].src + (int64_t)row * Q[ti].ld + c;
          if (ti == 0) {
            asm volatile("" ::"v"(src[0]), "s"(ns[0]), "s"(stride[0]));
            GKT(2);
            GKT_NOTE(first == 0, ns[0]);
          }
          if (ns[ti] > 0) {
#pragma unroll
            for (int u = 0; u < GR_BATCH; ++u) tv[ti][u] = src[ti][(int64_t)min(u, ns[ti] - 1) * stride[ti]];
          }
        }
      }
    }
    // Adam's bias corrections are uniform and need the step alone: evaluated while the loads are in flight
    float bc1 = 1.f, bc2 = 1.f, gscale = 1.f;
    if (adam.on) {
      bc1 = 1.f - powf(adam.b1, (float)a_t);
      bc2 = 1.f - powf(adam.b2, (float)a_t);
      gscale = 1.f / (a_cnt > 0.f ? a_cnt : 1.f);  // a weight sum below 1 is a normaliser too; integer counts: the same bits
      asm volatile("" ::"v"(bc1), "v"(bc2), "v"(gscale));
    }
    float total = 0.f;
    if (kind == GR_COPY) {
#pragma unroll
      for (int ti = 0; ti < 3; ++ti) {
        if (ti < n_terms) {
          float v = 0.f;
          if (ns[ti] > 0) {
            asm volatile("" : "+v"(tv[ti][0]));  // the first wait for a loaded value stands here, behind the bias corrections
#pragma unroll
            for (int u = 0; u < GR_BATCH; ++u)
              if (u < ns[ti]) v += tv[ti][u];
          }
          for (int z0 = GR_BATCH; z0 < ns[ti]; z0 += GR_BATCH) {  // deeper split-K (staged launchers, linear heads)
            float t[GR_BATCH];
#pragma unroll
            for (int u = 0; u < GR_BATCH; ++u) t[u] = src[ti][(int64_t)min(z0 + u, ns[ti] - 1) * stride[ti]];
#pragma unroll
            for (int u = 0; u < GR_BATCH; ++u)
              if (z0 + u < ns[ti]) v += t[u];
          }
          total += v * Q[ti].scale;
        }
      }
    } else {
      total = seg_terms(segs[seg], dyn, slabs, params, r, c);
    }
#ifdef HMP_KTIME
    asm volatile("s_waitcnt vmcnt(0)" ::"v"(total) : "memory");
    GKT(3);
#endif
    grads[e] = total;
    if (adam.on) {
      // torch.optim.Adam with coupled L2 on this element (same arithmetic as adam_kernel); only taken when no gradient
      // term of the network reads parameters (SAGE), so updating in place cannot race with another thread's reads
      // Which products are fused into their sums is written out, not left to the compiler (it changes with the code around
      // the expressions): these are the operations this update has always been compiled to, so its bits stay what they were
#pragma clang fp contract(off)
      const float pi = a_p;
      const float gi = __builtin_fmaf(adam.wd, pi, total * gscale);
      const float mi = adam.b1 * a_m + (1.f - adam.b1) * gi;
      const float vi = adam.b2 * a_v + (1.f - adam.b2) * gi * gi;
      adam.m[e] = mi;
      adam.v[e] = vi;
      const float denom = sqrtf(vi) / sqrtf(bc2) + adam.eps;
      adam.p[e] = __builtin_fmaf(-(adam.lr / bc1), mi / denom, pi);
    }
    GKT(4);
  }
  const float* __restrict__ row_lv = a.row_lv;
  if (row_lv != nullptr && blockIdx.x == 0) {
    __shared__ float sl[256], sv[256];
    float* __restrict__ out2 = a.out2;
    NetState* state = a.state;
    float l = 0.f, v = 0.f;
    for (int r = threadIdx.x; r < a.n_lv_rows; r += 256) { l += row_lv[2 * r]; v += row_lv[2 * r + 1]; }
    sl[threadIdx.x] = l;
    sv[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; sv[threadIdx.x] += sv[threadIdx.x + o]; }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      out2[0] = sl[0];
      out2[1] = sv[0];
      if (state) { state->loss_sum = sl[0]; state->count = sv[0]; }
    }
  }
}

int grad_reduce_launch(const GradSeg* d_segs, const GradRec* d_recs, int n_recs, const GradReduceDyn& dyn, const float* d_slabs,
                       const float* d_params, float* d_grads, const float* row_lv, int n_lv_rows, float* out2, NetState* state,
                       const AdamFuse& adam, hipStream_t st) {
  if (n_recs == 0) return HMP_OK;
  GradReduceArgs a;
  memset(&a, 0, sizeof(a));
  a.dyn = dyn;
  a.recs = d_recs; a.segs = d_segs; a.slabs = d_slabs; a.params = d_params; a.grads = d_grads;
  a.row_lv = row_lv; a.out2 = out2; a.state = state; a.n_lv_rows = n_lv_rows;
  a.adam = adam;
  hipLaunchKernelGGL(grad_reduce_kernel, dim3(n_recs), dim3(256), 0, st, a);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

}  // namespace hmp

extern "C" int hmp_masked_ce(const float* d_logits, int32_t ldl, int32_t n_rows, int32_t n_classes, const int64_t* d_labels,
                             int64_t ignored_label, float* d_grad, int32_t ldg, float* d_out2, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_logits && d_labels && d_out2, "hmp_masked_ce: null pointer");
  HMP_CHECK_ARG(n_rows >= 0 && n_classes > 0 && ldl >= n_classes && (d_grad == nullptr || ldg >= n_classes), "hmp_masked_ce: bad shape");
  return masked_ce_launch(d_logits, ldl, n_rows, n_classes, d_labels, ignored_label, d_grad, ldg, d_out2, nullptr, (hipStream_t)stream);
}

extern "C" int hmp_masked_ce_weighted(const float* d_logits, int32_t ldl, int32_t n_rows, int32_t n_classes, const int64_t* d_labels,
                                      int64_t ignored_label, const float* d_w, float* d_grad, int32_t ldg, float* d_out2, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_logits && d_labels && d_out2, "hmp_masked_ce_weighted: null pointer");
  HMP_CHECK_ARG(n_rows >= 0 && n_classes > 0 && ldl >= n_classes && (d_grad == nullptr || ldg >= n_classes), "hmp_masked_ce_weighted: bad shape");
  return masked_ce_launch(d_logits, ldl, n_rows, n_classes, d_labels, ignored_label, d_grad, ldg, d_out2, nullptr, (hipStream_t)stream, d_w);
}

extern "C" int hmp_argmax_rows(const float* d_x, int32_t ldx, int32_t n_rows, int32_t n_cols, int64_t* d_out, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_x && d_out && n_rows >= 0 && n_cols > 0 && ldx >= n_cols, "hmp_argmax_rows: bad argument");
  if (n_rows == 0) return HMP_OK;
  hipLaunchKernelGGL(argmax_rows_kernel, dim3(cdiv(n_rows, 16)), dim3(256), 0, (hipStream_t)stream, d_x, ldx, n_rows, n_cols, d_out);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

extern "C" int hmp_adam_flat(float* d_p, const float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                             float eps, float weight_decay, int32_t step, const float* d_count, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(n >= 0 && (n == 0 || (d_p && d_g && d_m && d_v)), "hmp_adam_flat: null pointer");
  HMP_CHECK_ARG(step >= 1, "hmp_adam_flat: step must be >= 1");
  return adam_launch(d_p, d_g, d_m, d_v, n, lr, beta1, beta2, eps, weight_decay, step, nullptr, d_count, (hipStream_t)stream);
}

extern "C" int hmp_dropout_mask(uint64_t seed, uint32_t rng_step, uint32_t rng_stream, float p, int32_t n_rows, int32_t F,
                                uint8_t* d_mask, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_mask && n_rows >= 0 && F >= 0 && p >= 0.f && p < 1.f, "hmp_dropout_mask: bad argument");
  if (n_rows == 0 || F == 0) return HMP_OK;
  DropCfg cfg;
  cfg.k0 = (uint32_t)seed; cfg.k1 = (uint32_t)(seed >> 32);
  cfg.step = rng_step; cfg.stream = rng_stream;
  cfg.thresh = drop_thresh(p); cfg.scale = 1.f / (1.f - p);
  cfg.step_dev = nullptr;
  const int64_t total = (int64_t)n_rows * ((F + 3) >> 2);
  const int64_t want = cdiv(total, 256);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((int)(want > 2048 ? 2048 : want)), dim3(256), 0, (hipStream_t)stream, cfg, n_rows, F, d_mask);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}
