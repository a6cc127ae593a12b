// Two learned linear heads over one final state (HomogeneousNetwork / HomogeneousNeuralTreeNetwork with output_dim_dict): the
// loop body of SemiSupervisedTrainingJob.train (semisupervised_training_job.py:117-147, homogeneous branches) from the program's
// output z on, and the per-batch arithmetic of its test() (:198-257).
//
//   y = dropout(act(z))  over every row;  logits_h = y @ W_h^T + b_h  for the rows of head h;  masked CE of both heads.
//
// One workgroup owns tiles of HL_RB rows (tile b, b + grid, ...: a fixed assignment, so the result does not depend on timing).
// Per tile:
//   pass 1  logits of BOTH heads for every row of the tile, exact fp32 on the VALU (4 rows x 4 classes per thread), the
//           F axis streamed through LDS in chunks of HL_FC columns (y chunk recomputed from z, W chunk of both heads), a chunk
//           summed by an fmaf chain of its own and the chunk sums added in ascending order;
//   CE      one thread per (row, head): log-sum-exp, {loss, valid}, dlogits in place of the logits (0 outside the head);
//   pass 2  per F chunk: dz = dlogits @ W . keep/(1-p) . act'  -> the output gradient, and dW += dlogits^T y into the
//           workgroup's own slab (db once per tile).  No float atomics: the slabs are summed in a fixed order by the
//           gradient un-pack (grad_reduce_kernel), which sees the heads as four more parameter segments.
#include "tail_fns.h"

namespace hmp {

namespace {

constexpr int HL_RB = 32;             // rows per tile
constexpr int HL_FC = 64;             // F columns per LDS chunk
constexpr int HL_KP = 2 * HEAD_MAX_CLASSES;  // logits per row, both heads
constexpr int HL_PAD = HL_FC + 1;     // LDS row pitch of the chunks (conflict-free column walks)

struct HeadSmem {
  float lg[HL_RB][HL_KP + 1];  // logits, then dlogits
  float ys[HL_RB][HL_PAD];     // y chunk
  float ws[HL_KP][HL_PAD];     // W chunk of both heads (room rows first)
  float hl[2][HL_RB], hv[2][HL_RB];
  int cnt[4];
};

__device__ __forceinline__ bool head_member(const LinHeadArgs& a, int h, int row) {
  if (h == 0) return a.member[0] ? a.member[0][row] != 0 : true;
  if (a.member[1]) return a.member[1][row] != 0;
  return a.member[0] ? a.member[0][row] == 0 : false;  // NULL: complement of head 0
}

// y = dropout(act(z)) of columns c0 .. c0 + HL_FC - 1 of the tile's rows into s.ys (0 outside the rows / columns); the arithmetic
// and keep-mask numbering of bias_act_drop_kernel: quad row * ceil(F / 4) + col / 4
__device__ void stage_y(const LinHeadArgs& a, const DropCfg& cfg, int row0, int c0, HeadSmem& s) {
  const int qpr = (a.F + 3) >> 2;
  for (int q = threadIdx.x; q < HL_RB * (HL_FC / 4); q += 256) {
    const int r = q / (HL_FC / 4), cq = q % (HL_FC / 4);
    const int row = row0 + r, c = c0 + 4 * cq;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < a.n_rows && c < a.F) {
      const float4 z4 = *reinterpret_cast<const float4*>(a.z + (int64_t)row * a.ldz + c);  // ldz % 4 == 0, c + 3 < ldz
      bool keep[4] = {true, true, true, true};
      if (a.drop_on) drop_keep4(cfg, (uint32_t)row * (uint32_t)qpr + (uint32_t)(c >> 2), keep);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = c + i < a.F ? act_drop((&z4.x)[i], a.act, a.drop_on != 0, keep[i], cfg.scale) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s.ys[r][4 * cq + i] = v[i];
  }
}

// W rows of both heads (k < classes[0]: room, then object), columns c0 .. c0 + HL_FC - 1, into s.ws (0 past F)
__device__ void stage_w(const LinHeadArgs& a, int c0, HeadSmem& s) {
  for (int q = threadIdx.x; q < a.K * HL_FC; q += 256) {
    const int k = q / HL_FC, f = q % HL_FC, c = c0 + f;
    const float* w = k < a.classes[0] ? a.W[0] + (int64_t)k * a.F : a.W[1] + (int64_t)(k - a.classes[0]) * a.F;
    s.ws[k][f] = c < a.F ? w[c] : 0.f;
  }
}

// first maximum of lg[0 .. C) (torch.argmax's rule), sequential over the classes
__device__ __forceinline__ int head_argmax(const float* lg, int C) {
  int arg = 0;
  float best = lg[0];
  for (int k = 1; k < C; ++k)
    if (lg[k] > best) { best = lg[k]; arg = k; }
  return arg;
}

// what follows the logits of a tile: the CE and its backward (pass 2), the accuracy count, or the labels themselves
// (or, HL_TOPK, the k largest logits of each head with their softmax probabilities; or, HL_MC, one Monte-Carlo dropout sample
// of each head's softmax added to the row's accumulators -- the one label mode whose tail draws)
enum HeadMode { HL_COUNT = 0, HL_TRAIN = 1, HL_PREDICT = 2, HL_TOPK = 3, HL_MC = 4 };

constexpr int HL_GS = 16;  // HL_TOPK, HL_MC: lanes per (row, head) of the tile

// HL_TOPK: the tile's 2 * HL_RB (row, head) pairs go round the workgroup's groups of HL_GS lanes, each a topk_group walk (tail_fns.h)
// over the head's logits in LDS -- comparisons alone pick the labels, so column 0 is head_argmax's; -1 / 0 outside the head's rows
__device__ __forceinline__ void heads_topk(const LinHeadArgs& a, const HeadSmem& s, int row0) {
  const int lane = threadIdx.x % HL_GS;
  for (int p = (int)threadIdx.x / HL_GS; p < 2 * HL_RB; p += 256 / HL_GS) {  // whole groups take every branch below together
    const int r = p % HL_RB, h = p / HL_RB, row = row0 + r;
    if (row >= a.n_rows || !(a.tk_labels[h] || a.tk_probs[h])) continue;
    // the member byte and the output addresses do not depend on the walk
    const bool member = head_member(a, h, row);
    int64_t* const lo = a.tk_labels[h] ? a.tk_labels[h] + (int64_t)row * a.topk : nullptr;
    float* const po = a.tk_probs[h] ? a.tk_probs[h] + (int64_t)row * a.topk : nullptr;
    const int C = a.classes[h];
    const float* lg = &s.lg[r][h == 0 ? 0 : a.classes[0]];
    if (!member) {
      topk_blank(lane, 0, a.topk, lo, po);
      continue;
    }
    topk_group<HL_GS, 0>(lane, C, a.topk, [&](int, int c, float (&v)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = c + i < C ? lg[c + i] : 0.f;
    }, lo, po);
  }
}

// HL_MC: the same round over the tile's (row, head) pairs, each a mc_group walk (tail_fns.h) over the head's logits in LDS into the
// accumulators of the head's row; rows outside the head's rows are not touched
__device__ __forceinline__ void heads_mc(const LinHeadArgs& a, const HeadSmem& s, int row0) {
  const int lane = threadIdx.x % HL_GS;
  for (int p = (int)threadIdx.x / HL_GS; p < 2 * HL_RB; p += 256 / HL_GS) {  // whole groups take every branch below together
    const int r = p % HL_RB, h = p / HL_RB, row = row0 + r;
    if (row >= a.n_rows || !a.mc_acc[h]) continue;
    // the member byte and the accumulator address do not depend on the walk
    const bool member = head_member(a, h, row);
    float* const ar = a.mc_acc[h] + (int64_t)row * a.mc_ld[h];
    const int C = a.classes[h];
    const float* lg = &s.lg[r][h == 0 ? 0 : a.classes[0]];
    if (!member) continue;
    mc_group<HL_GS, 0>(lane, C, [&](int, int c, float (&v)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = c + i < C ? lg[c + i] : 0.f;
    }, a.mc_first != 0, ar);
  }
}

template <HeadMode MODE>
__global__ __launch_bounds__(256) void linear_heads_kernel(const LinHeadArgs a) {
  constexpr bool TRAIN = MODE == HL_TRAIN;
  __shared__ HeadSmem s;
  const int t = threadIdx.x;
  const DropCfg cfg = a.drop_on ? drop_resolve(a.drop) : a.drop;
  if (MODE == HL_COUNT && t < 4) s.cnt[t] = 0;
  bool first = true;
  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x, first = false) {
    const int row0 = tile * HL_RB;
    // ---- pass 1: logits ----------------------------------------------------------------------------------------------
    const int rg = t & 7, cg = t >> 3;  // rows rg + 8 i, classes 4 cg + j
    const bool live = 4 * cg < a.K;     // whole wavefronts drop out past the classes
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int c0 = 0; c0 < a.F; c0 += HL_FC) {
      __syncthreads();  // the previous chunk / tile is consumed
      stage_y(a, cfg, row0, c0, s);
      stage_w(a, c0, s);
      __syncthreads();
      if (live) {
        // A chunk is summed on its own and then added to the logit: one fmaf chain over all of F rounds every step at the
        // magnitude of the growing logit (F = 1024, logits ~100: 2e-4 off in a row loss, 5 x a blocked float32 sum); a chunk's
        // chain stays at the chunk's magnitude and the logit itself rounds F / HL_FC times.  Sums that are exact in float32
        // (integer-like inputs) keep their bits.
        float part[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) part[i][j] = 0.f;
        const int fe = min(HL_FC, a.F - c0);
        for (int f = 0; f < fe; ++f) {
          float yv[4], wv[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) yv[i] = s.ys[rg + 8 * i][f];
#pragma unroll
          for (int j = 0; j < 4; ++j) wv[j] = s.ws[min(4 * cg + j, HL_KP - 1)][f];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[i][j] = fmaf(yv[i], wv[j], part[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] += part[i][j];
      }
    }
    if (live) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 4 * cg + j;
        if (k >= a.K) continue;
        const float bk = k < a.classes[0] ? a.bias[0][k] : a.bias[1][k - a.classes[0]];
#pragma unroll
        for (int i = 0; i < 4; ++i) s.lg[rg + 8 * i][k] = acc[i][j] + bk;
      }
    }
    __syncthreads();
    if constexpr (MODE == HL_TOPK) {
      heads_topk(a, s, row0);
      continue;
    }
    if constexpr (MODE == HL_MC) {
      heads_mc(a, s, row0);
      continue;
    }
    // ---- CE / argmax: one thread per (row, head) -----------------------------------------------------------------------
    if (t < 2 * HL_RB) {
      const int r = t % HL_RB, h = t / HL_RB, row = row0 + r;
      const int C = a.classes[h], koff = h == 0 ? 0 : a.classes[0];
      float* lg = &s.lg[r][koff];
      const bool in_rows = row < a.n_rows;
      const bool member = in_rows && head_member(a, h, row);
      if (MODE == HL_PREDICT) {  // no labels, no mask: every row of the tile gets its label, -1 outside the head's rows
        int64_t* const out = a.pred[h];
        if (in_rows && out) out[row] = member ? (int64_t)head_argmax(lg, C) : -1;
        continue;
      }
      const bool in_mask = in_rows && (a.mask ? a.mask[row] != 0 : true);
      const int64_t y = in_rows ? a.labels[row] : 0;
      if (TRAIN) {
        const bool valid = member && in_mask && y != a.ignored;
        const bool bad = valid && (y < 0 || y >= C);
        // class weight of the row's label (tail_fns.h: ce_group's rule; never indexed by an unchecked label)
        const float* const hw = a.weight[h];
        const float wy = (hw && valid && !bad) ? hw[y] : 1.f;
        const bool use = valid && !bad && !(hw && wy == 0.f);
        float loss = 0.f;
        if (use) {
          float m = -INFINITY;
          for (int k = 0; k < C; ++k) m = fmaxf(m, lg[k]);
          float sum = 0.f;
          for (int k = 0; k < C; ++k) sum += expf(lg[k] - m);
          const float lse = m + logf(sum);
          loss = lse - lg[y];
          if (hw) loss *= wy;
          for (int k = 0; k < C; ++k) {
            const float g = expf(lg[k] - lse) - (k == (int)y ? 1.f : 0.f);
            lg[k] = hw ? g * wy : g;
          }
        } else {
          for (int k = 0; k < C; ++k) lg[k] = 0.f;
        }
        s.hl[h][r] = loss;
        s.hv[h][r] = use ? (hw ? wy : 1.f) : 0.f;
        if (bad) atomicOr(&a.state->status, 2);
      } else if (member && in_mask) {
        const int arg = head_argmax(lg, C);
        atomicAdd(&s.cnt[2 * h + 1], 1);
        if ((int64_t)arg == y) atomicAdd(&s.cnt[2 * h], 1);
      }
    }
    if (!TRAIN) continue;
    __syncthreads();
    if (t < HL_RB && row0 + t < a.n_rows) {  // {loss, valid} of the row: room head + object head
      a.row_lv[2 * (int64_t)(row0 + t)] = s.hl[0][t] + s.hl[1][t];
      a.row_lv[2 * (int64_t)(row0 + t) + 1] = s.hv[0][t] + s.hv[1][t];
    }
    float* slab = a.slabs + (int64_t)blockIdx.x * a.slab_stride;
    if (t < a.K) {  // db: column sums of dlogits, rows ascending
      float db = 0.f;
      for (int r = 0; r < HL_RB; ++r) db += s.lg[r][t];
      float* d = slab + (int64_t)a.K * a.ld_slab + t;
      *d = first ? db : *d + db;
    }
    // ---- pass 2: dz and dW per F chunk ---------------------------------------------------------------------------------
    const int f = t & (HL_FC - 1), q = t >> 6;  // column f; rows / classes q + 4 i
    for (int c0 = 0; c0 < a.F; c0 += HL_FC) {
      __syncthreads();
      stage_y(a, cfg, row0, c0, s);
      stage_w(a, c0, s);
      __syncthreads();
      const int c = c0 + f;
      float dz[HL_RB / 4];
#pragma unroll
      for (int i = 0; i < HL_RB / 4; ++i) dz[i] = 0.f;
      for (int k = 0; k < a.K; ++k) {
        const float w = s.ws[k][f];
#pragma unroll
        for (int i = 0; i < HL_RB / 4; ++i) dz[i] = fmaf(s.lg[q + 4 * i][k], w, dz[i]);
      }
      if (c < a.ldg) {
#pragma unroll
        for (int i = 0; i < HL_RB / 4; ++i) {
          const int row = row0 + q + 4 * i;
          if (row >= a.n_rows) continue;
          const float g = c < a.F ? dz[i] * tail_dydz(s.ys[q + 4 * i][f], a.act, a.drop_on != 0, cfg.scale) : 0.f;
          a.grad[(int64_t)row * a.ldg + c] = g;
        }
      }
      if (c < a.F) {
        for (int k0 = 0; k0 < a.K; k0 += 4 * 8) {  // classes q + 4 i of this group of 32
          float dw[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) dw[i] = 0.f;
          for (int r = 0; r < HL_RB; ++r) {
            const float yv = s.ys[r][f];
#pragma unroll
            for (int i = 0; i < 8; ++i) dw[i] = fmaf(s.lg[r][min(k0 + q + 4 * i, HL_KP - 1)], yv, dw[i]);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int k = k0 + q + 4 * i;
            if (k >= a.K) continue;
            float* d = slab + (int64_t)k * a.ld_slab + c;
            *d = first ? dw[i] : *d + dw[i];
          }
        }
      }
    }
  }
  if (MODE == HL_COUNT) {
    __syncthreads();
    if (t < 4 && s.cnt[t]) atomicAdd(&a.counts[t], (unsigned long long)s.cnt[t]);
  }
}

int heads_check(const LinHeadArgs& a, bool labels = true) {
  HMP_CHECK_ARG(a.F >= 1 && a.F <= HEAD_MAX_F, "linear heads: F = %d (1 .. %d)", a.F, HEAD_MAX_F);
  HMP_CHECK_ARG(a.classes[0] >= 1 && a.classes[0] <= HEAD_MAX_CLASSES && a.classes[1] >= 1 && a.classes[1] <= HEAD_MAX_CLASSES &&
                    a.K == a.classes[0] + a.classes[1],
                "linear heads: classes %d / %d (1 .. %d each)", a.classes[0], a.classes[1], HEAD_MAX_CLASSES);
  HMP_CHECK_ARG((a.ldz & 3) == 0 && a.ldz >= a.F && (reinterpret_cast<uintptr_t>(a.z) & 15) == 0,
                "linear heads: final state must be 16-byte aligned with ld %% 4 == 0 and ld >= %d", a.F);
  HMP_CHECK_ARG(!labels || a.labels != nullptr || a.n_rows == 0, "linear heads: labels required");
  return HMP_OK;
}

}  // namespace

int heads_blocks(int n_rows) {
  const int tiles = cdiv(n_rows, HL_RB);
  return tiles < HEAD_MAX_BLOCKS ? tiles : HEAD_MAX_BLOCKS;
}

// the launch of every mode: a workgroup per row tile up to the cap, walking n_tiles; only the training and the Monte-Carlo launch drop
template <HeadMode MODE>
static int heads_launch(LinHeadArgs& a, hipStream_t st) {
  a.n_tiles = cdiv(a.n_rows, HL_RB);
  if (MODE != HL_TRAIN && MODE != HL_MC) a.drop_on = 0;
  const int blocks = heads_blocks(a.n_rows);
  if (blocks == 0) return HMP_OK;
  hipLaunchKernelGGL(linear_heads_kernel<MODE>, dim3(blocks), dim3(256), 0, st, a);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int linear_heads_ce_launch(LinHeadArgs& a, hipStream_t st) {
  HMP_TRY(heads_check(a));
  // the kernel walks the gradient's columns by LDS chunk up to roundup(F, HL_FC): a wider ldg would leave columns unwritten
  HMP_CHECK_ARG(a.ldg == align4(a.F), "linear heads: gradient ld %d (F = %d rounded up to 4: %d)", a.ldg, a.F, align4(a.F));
  HMP_CHECK_ARG(a.ld_slab >= a.F && a.slab_stride >= (int64_t)a.K * (a.ld_slab + 1), "linear heads: slab layout");
  return heads_launch<HL_TRAIN>(a, st);
}

int linear_heads_count_launch(LinHeadArgs& a, long long* counts, hipStream_t st) {
  HMP_TRY(heads_check(a));
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  return heads_launch<HL_COUNT>(a, st);
}

// pred[h][row] = argmax of head h's logits on act(z) for the head's rows, -1 elsewhere (eval mode; pred[h] null: head skipped).
// Pass 1 and the tile assignment are the count's; no labels, mask, counters or pass 2.
int linear_heads_predict_launch(LinHeadArgs& a, int64_t* const* pred, hipStream_t st) {
  HMP_CHECK_ARG(pred != nullptr, "linear heads: null output array");
  HMP_TRY(heads_check(a, false));
  a.pred[0] = pred[0]; a.pred[1] = pred[1];
  return heads_launch<HL_PREDICT>(a, st);
}

// labels[h][row][0:k) / probs[h][row][0:k) = the k largest logits of head h on act(z) and their softmax probabilities for the head's
// rows, -1 / 0 elsewhere (eval mode; a head with both pointers null is skipped).  Pass 1 and the tile assignment are the count's.
int linear_heads_topk_launch(LinHeadArgs& a, int k, int64_t* const* labels, float* const* probs, hipStream_t st) {
  HMP_CHECK_ARG(labels != nullptr && probs != nullptr, "linear heads: null output array");
  HMP_CHECK_ARG(k >= 1 && k <= TOPK_MAX, "linear heads: k = %d (1 .. %d)", k, TOPK_MAX);
  HMP_TRY(heads_check(a, false));
  for (int h = 0; h < 2; ++h) {
    a.tk_labels[h] = labels[h];
    a.tk_probs[h] = probs[h];
  }
  a.topk = k;
  return heads_launch<HL_TOPK>(a, st);
}

// one Monte-Carlo dropout sample: the softmax of head h's logits on dropout(act(z)) (a.drop_on / a.drop: the caller's site) added to
// acc[h][row] (kernels.h: the layout) for the head's rows; a head without accumulator is skipped.  Pass 1 and the tile assignment are
// the count's.
int linear_heads_mc_launch(LinHeadArgs& a, int first, float* const* acc, const int* ld_acc, hipStream_t st) {
  HMP_CHECK_ARG(acc != nullptr && ld_acc != nullptr, "linear heads: null accumulator array");
  HMP_TRY(heads_check(a, false));
  for (int h = 0; h < 2; ++h) {
    HMP_CHECK_ARG(!acc[h] || ld_acc[h] > mc_off_e(a.classes[h]), "linear heads: ld_acc %d of head %d (%d classes need more than %d)", ld_acc[h],
                  h, a.classes[h], mc_off_e(a.classes[h]));
    a.mc_acc[h] = acc[h];
    a.mc_ld[h] = ld_acc[h];
  }
  a.mc_first = first;
  return heads_launch<HL_MC>(a, st);
}

}  // namespace hmp

// test / diagnostic entry of the two linear-heads launchers: a plain copy of the descriptor into LinHeadArgs, no choice of its own
// (d_w: the class weights of each head for the CE launch, null: unweighted)
static int linear_heads_run(const hmp_linear_heads_desc* d, const float* const* d_w, int32_t train, int32_t* d_state, int64_t* d_counts,
                            int32_t* n_blocks_out, void* stream) {
  using namespace hmp;
  static const bool have_device = hmp_device_count() > 0;
  HMP_CHECK_ARG(have_device, "hmp_linear_heads_run: no gfx950 device visible");
  HMP_CHECK_ARG(d && d->z && d->W[0] && d->W[1] && d->bias[0] && d->bias[1], "hmp_linear_heads_run: null pointer");
  HMP_CHECK_ARG(train ? (d_state && d->grad && d->row_lv && d->slabs) : d_counts != nullptr,
                "hmp_linear_heads_run: %s", train ? "the CE needs d_state, grad, row_lv and slabs" : "the count needs d_counts");
  LinHeadArgs a;
  memset(&a, 0, sizeof(a));
  a.z = d->z; a.ldz = d->ldz; a.n_rows = d->n_rows; a.F = d->F;
  a.classes[0] = d->classes[0]; a.classes[1] = d->classes[1]; a.K = a.classes[0] + a.classes[1];
  for (int k = 0; k < 2; ++k) {
    a.W[k] = d->W[k];
    a.bias[k] = d->bias[k];
    a.member[k] = d->member[k];
    if (train && d_w) a.weight[k] = d_w[k];
  }
  a.labels = d->labels; a.mask = d->mask; a.ignored = d->ignored;
  a.act = d->act;
  a.state = reinterpret_cast<NetState*>(d_state);
  a.drop_on = (train && d->p > 0.f) ? 1 : 0;
  if (a.drop_on) {  // (as net.hip: make_drop)
    a.drop.k0 = (uint32_t)d->seed; a.drop.k1 = (uint32_t)(d->seed >> 32);
    a.drop.step = d->rng_step; a.drop.stream = d->rng_stream;
    a.drop.thresh = drop_thresh(d->p); a.drop.scale = 1.f / (1.f - d->p);
    a.drop.step_dev = nullptr;
  }
  a.grad = d->grad; a.ldg = d->ldg; a.row_lv = d->row_lv;
  a.slabs = d->slabs; a.ld_slab = d->ld_slab; a.slab_stride = d->slab_stride;
  if (n_blocks_out) *n_blocks_out = heads_blocks(d->n_rows);
  return train ? linear_heads_ce_launch(a, (hipStream_t)stream) : linear_heads_count_launch(a, (long long*)d_counts, (hipStream_t)stream);
}

extern "C" int hmp_linear_heads_run(const hmp_linear_heads_desc* d, int32_t train, int32_t* d_state, int64_t* d_counts,
                                    int32_t* n_blocks_out, void* stream) {
  return linear_heads_run(d, nullptr, train, d_state, d_counts, n_blocks_out, stream);
}

extern "C" int hmp_linear_heads_run_weighted(const hmp_linear_heads_desc* d, const float* const* d_w, int32_t train, int32_t* d_state,
                                             int64_t* d_counts, int32_t* n_blocks_out, void* stream) {
  return linear_heads_run(d, d_w, train, d_state, d_counts, n_blocks_out, stream);
}

// the descriptor of a label / top-k launch (labels, mask, grad, row_lv and slabs may be NULL) as LinHeadArgs, eval mode
static int label_heads_args(const char* who, const hmp_linear_heads_desc* d, int32_t* n_blocks_out, hmp::LinHeadArgs& a) {
  using namespace hmp;
  static const bool have_device = hmp_device_count() > 0;
  HMP_CHECK_ARG(have_device, "%s: no gfx950 device visible", who);
  HMP_CHECK_ARG(d && d->z && d->W[0] && d->W[1] && d->bias[0] && d->bias[1], "%s: null pointer", who);
  memset(&a, 0, sizeof(a));
  a.z = d->z; a.ldz = d->ldz; a.n_rows = d->n_rows; a.F = d->F;
  a.classes[0] = d->classes[0]; a.classes[1] = d->classes[1]; a.K = a.classes[0] + a.classes[1];
  for (int k = 0; k < 2; ++k) {
    a.W[k] = d->W[k];
    a.bias[k] = d->bias[k];
    a.member[k] = d->member[k];
  }
  a.act = d->act;
  if (n_blocks_out) *n_blocks_out = heads_blocks(d->n_rows);
  return HMP_OK;
}

// the predict launcher on the same descriptor
extern "C" int hmp_linear_heads_predict(const hmp_linear_heads_desc* d, int64_t* const* d_pred, int32_t* n_blocks_out, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_pred, "hmp_linear_heads_predict: null pointer");
  LinHeadArgs a;
  HMP_TRY(label_heads_args("hmp_linear_heads_predict", d, n_blocks_out, a));
  return linear_heads_predict_launch(a, d_pred, (hipStream_t)stream);
}

// the top-k launcher on the same descriptor
extern "C" int hmp_linear_heads_topk(const hmp_linear_heads_desc* d, int32_t k, int64_t* const* d_labels, float* const* d_probs,
                                     int32_t* n_blocks_out, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_labels && d_probs, "hmp_linear_heads_topk: null pointer");
  LinHeadArgs a;
  HMP_TRY(label_heads_args("hmp_linear_heads_topk", d, n_blocks_out, a));
  return linear_heads_topk_launch(a, k, d_labels, d_probs, (hipStream_t)stream);
}

// the Monte-Carlo launcher on the same descriptor, training mode: the tail draws at the descriptor's dropout site (p == 0: none)
extern "C" int hmp_linear_heads_mc(const hmp_linear_heads_desc* d, int32_t first, float* const* d_acc, const int32_t* ld_acc,
                                   int32_t* n_blocks_out, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_acc && ld_acc, "hmp_linear_heads_mc: null pointer");
  LinHeadArgs a;
  HMP_TRY(label_heads_args("hmp_linear_heads_mc", d, n_blocks_out, a));
  HMP_CHECK_ARG(d->p >= 0.f && d->p < 1.f, "hmp_linear_heads_mc: p = %g", (double)d->p);
  a.drop_on = d->p > 0.f ? 1 : 0;
  if (a.drop_on) {  // (as net.hip: make_drop)
    a.drop.k0 = (uint32_t)d->seed; a.drop.k1 = (uint32_t)(d->seed >> 32);
    a.drop.step = d->rng_step; a.drop.stream = d->rng_stream;
    a.drop.thresh = drop_thresh(d->p); a.drop.scale = 1.f / (1.f - d->p);
    a.drop.step_dev = nullptr;
  }
  return linear_heads_mc_launch(a, first, d_acc, ld_acc, (hipStream_t)stream);
}
