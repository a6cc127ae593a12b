// Room-task validation count: the per-batch arithmetic of BaseTrainingJob.test (base_training_job.py:269-313) on the device.
//
//   pred = argmax(logits, dim=1) (first maximum);  a row counts iff (members == null || members[row]) && label != ignored;
//   counts += {#(pred == label), #rows};  confusion[label][pred] += 1 for counted rows with label in [0, n_classes).
//
// A row belongs to a group of 16 lanes (argmax_rows_kernel's grouping, optim.hip).  With ld % 4 == 0 and a 16-byte aligned base,
// lane i owns the quads i, i + 16, ... of the row (16-byte loads); otherwise lane i owns the columns i, i + 16, ...  Both are
// walks of the one first-maximum argmax (tail_fns.h), so the prediction is argmax_rows_kernel's (and torch.argmax's on finite
// logits) whatever the layout.
//
// Per-workgroup counters live in LDS (tail_fns.h: count_begin / count_row / count_flush).
// For n_classes <= EV_HIST_MAX the confusion matrix is an LDS histogram too (<= 16 KB of int32), above that rows add to the global
// matrix directly.  Everything is ACCUMULATED (+=): a validation pass sums its batches on the device and reads the totals once.
//
// Per-graph form (BaseTrainingJob.test_individual_graph, base_training_job.py:315-339, for a whole batch in one launch):
// count_rows_by_graph_kernel applies the same rule per row and adds to counts[g] = {correct, total} of the graph g that owns the
// row, found in the batch's [n_graphs + 1] row offsets of the output node type (find_seg: rows of a graph are contiguous).  The
// 16 rows of a workgroup pass are consecutive, so they span few graphs: rows are staged in LDS and the first row of each run of
// equal graphs adds the run's sums with two 64-bit atomics.
#include "device_fns.h"  // find_seg
#include "tail_fns.h"

namespace hmp {

namespace {

constexpr int EV_GS = 16;               // lanes per row
constexpr int EV_RPB = 256 / EV_GS;     // rows per workgroup and pass
constexpr int EV_HIST_MAX = 64;         // largest class count with an LDS confusion histogram
constexpr int EV_MAX_BLOCKS = 1024;     // grid cap: larger inputs stride over rows (fewer histogram flushes)

// the row's prediction by its 16 lanes
template <bool VEC>
__device__ __forceinline__ int ev_argmax(const float* __restrict__ xr, int n_classes, int lane) {
  if (!VEC) {  // lane i owns the columns i, i + 16, ...
    float best = -INFINITY;
    int arg = ARGMAX_NONE;
    for (int c = lane; c < n_classes; c += EV_GS) argmax_take(xr[c], c, best, arg);
    return argmax_reduce<EV_GS>(best, arg);
  }
  return argmax_group<EV_GS, 0>(lane, n_classes, [&](int, int c, float (&v)[4]) {
    const float4 x4 = *reinterpret_cast<const float4*>(xr + c);  // c + 3 < ld: ld % 4 == 0 and c < n_classes <= ld
    v[0] = x4.x; v[1] = x4.y; v[2] = x4.z; v[3] = x4.w;
  });
}

template <bool VEC, bool HIST>
__global__ __launch_bounds__(256) void count_rows_kernel(const float* __restrict__ x, int ld, int n_rows, int n_classes,
                                                         const int64_t* __restrict__ labels, const uint8_t* __restrict__ members,
                                                         int64_t ignored, unsigned long long* __restrict__ counts,
                                                         unsigned long long* __restrict__ confusion) {
  __shared__ int s_cnt[2];
  __shared__ int s_hist[HIST ? EV_HIST_MAX * EV_HIST_MAX : 1];
  const int cc = HIST ? n_classes * n_classes : 0;
  for (int i = threadIdx.x; i < cc; i += 256) s_hist[i] = 0;
  count_begin(s_cnt);
  const int lane = threadIdx.x % EV_GS;
  for (int row = blockIdx.x * EV_RPB + (int)threadIdx.x / EV_GS; row < n_rows; row += gridDim.x * EV_RPB) {
    // the whole group of 16 lanes takes the same branch: the shuffles below stay inside active groups
    const int64_t y = labels[row];
    if ((members && !members[row]) || y == ignored) continue;
    const int pred = ev_argmax<VEC>(x + (int64_t)row * ld, n_classes, lane);
    if (lane == 0) {
      // pred is always inside [0, n_classes), so a label outside it never equals pred: it counts in the total only
      count_row(s_cnt, (int64_t)pred == y);
      if (y >= 0 && y < n_classes) {
        if (HIST) atomicAdd(&s_hist[(int)y * n_classes + pred], 1);
        else if (confusion) atomicAdd(&confusion[y * n_classes + pred], 1ull);
      }
    }
  }
  count_flush(s_cnt, counts);
  for (int i = threadIdx.x; i < cc; i += 256)
    if (s_hist[i]) atomicAdd(&confusion[i], (unsigned long long)s_hist[i]);
}

template <bool VEC>
__global__ __launch_bounds__(256) void count_rows_by_graph_kernel(const float* __restrict__ x, int ld, int n_rows, int n_classes,
                                                                  const int64_t* __restrict__ labels, const uint8_t* __restrict__ members,
                                                                  int64_t ignored, const int64_t* __restrict__ graph_ptr, int n_graphs,
                                                                  unsigned long long* __restrict__ counts) {
  __shared__ int s_graph[EV_RPB];  // graph of the pass's row, -1: the row does not count
  __shared__ int s_hit[EV_RPB];
  const int lane = threadIdx.x % EV_GS, slot = (int)threadIdx.x / EV_GS;
  // every workgroup runs the same number of passes (the barriers below): the row bound is checked inside
  for (int base = blockIdx.x * EV_RPB; base < n_rows; base += gridDim.x * EV_RPB) {
    const int row = base + slot;
    int g = -1, hit = 0;
    if (row < n_rows) {
      const int64_t y = labels[row];
      if (!(members && !members[row]) && y != ignored) {  // the whole group of 16 lanes takes the same branch
        const int pred = ev_argmax<VEC>(x + (int64_t)row * ld, n_classes, lane);
        g = find_seg(graph_ptr, n_graphs, row);  // always inside [0, n_graphs)
        hit = (y >= 0 && y < n_classes && pred == (int)y) ? 1 : 0;  // a label outside [0, n_classes) counts in the total only
      }
    }
    if (lane == 0) { s_graph[slot] = g; s_hit[slot] = hit; }
    __syncthreads();
    // graphs are non-decreasing along the rows: the first counted row of each graph in this pass adds the graph's sums
    if (lane == 0 && g >= 0) {
      bool first = true;
      for (int q = 0; q < slot; ++q) first = first && s_graph[q] != g;
      if (first) {
        int correct = 0, total = 0;
        for (int q = slot; q < EV_RPB; ++q)
          if (s_graph[q] == g) { correct += s_hit[q]; ++total; }
        if (correct) atomicAdd(&counts[2 * (int64_t)g], (unsigned long long)correct);
        atomicAdd(&counts[2 * (int64_t)g + 1], (unsigned long long)total);
      }
    }
    __syncthreads();
  }
}

// pred[row] = the row's prediction, -1 for a row outside `members` (null: every row)
template <bool VEC>
__global__ __launch_bounds__(256) void predict_rows_kernel(const float* __restrict__ x, int ld, int n_rows, int n_classes,
                                                           const uint8_t* __restrict__ members, int64_t* __restrict__ pred) {
  const int lane = threadIdx.x % EV_GS;
  for (int row = blockIdx.x * EV_RPB + (int)threadIdx.x / EV_GS; row < n_rows; row += gridDim.x * EV_RPB) {
    // the member byte and the output address do not depend on the walk; the whole group of 16 lanes takes the same branch
    const bool member = members ? members[row] != 0 : true;
    int64_t* const out = pred + row;
    int p = -1;
    if (member) p = ev_argmax<VEC>(x + (int64_t)row * ld, n_classes, lane);
    if (lane == 0) *out = (int64_t)p;
  }
}

// labels[row][0:k) / probs[row][0:k) = the row's k largest entries and their softmax probabilities (tail_fns.h: topk_group), -1 / 0
// for a row outside `members`.  VEC: 16-byte loads; else the same quads by scalar loads (a pitch or base without the alignment):
// the lanes own the same columns either way, so the probabilities of a row do not depend on its layout.
template <bool VEC>
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ x, int ld, int n_rows, int n_classes,
                                                        const uint8_t* __restrict__ members, int k, int64_t* __restrict__ labels,
                                                        float* __restrict__ probs) {
  const int lane = threadIdx.x % EV_GS;
  for (int row = blockIdx.x * EV_RPB + (int)threadIdx.x / EV_GS; row < n_rows; row += gridDim.x * EV_RPB) {
    // the member byte and the output addresses do not depend on the walk; the whole group of 16 lanes takes the same branch
    const bool member = members ? members[row] != 0 : true;
    int64_t* const lo = labels ? labels + (int64_t)row * k : nullptr;
    float* const po = probs ? probs + (int64_t)row * k : nullptr;
    const float* __restrict__ xr = x + (int64_t)row * ld;
    if (!member) {
      topk_blank(lane, 0, k, lo, po);
    } else if (VEC) {
      topk_group<EV_GS, 0>(lane, n_classes, k, [&](int, int c, float (&v)[4]) {
        const float4 x4 = *reinterpret_cast<const float4*>(xr + c);  // c + 3 < ld: ld % 4 == 0 and c < n_classes <= ld
        v[0] = x4.x; v[1] = x4.y; v[2] = x4.z; v[3] = x4.w;
      }, lo, po);
    } else {
      topk_group<EV_GS, 0>(lane, n_classes, k, [&](int, int c, float (&v)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = c + i < n_classes ? xr[c + i] : 0.f;  // nothing past the row's classes is read
      }, lo, po);
    }
  }
}

// One Monte-Carlo dropout sample (tail_fns.h: mc_group): the row's softmax, its squares and its entropy are added to the row's
// accumulators acc[row] (kernels.h: the layout), or stored with first != 0.  Rows outside `members` are not touched.  VEC / scalar
// as topk_rows_kernel: the lanes own the same columns either way, so a row's probabilities are the top-k kernel's bit for bit.
template <bool VEC>
__global__ __launch_bounds__(256) void mc_rows_kernel(const float* __restrict__ x, int ld, int n_rows, int n_classes,
                                                      const uint8_t* __restrict__ members, int first, float* __restrict__ acc, int ld_acc) {
  const int lane = threadIdx.x % EV_GS;
  for (int row = blockIdx.x * EV_RPB + (int)threadIdx.x / EV_GS; row < n_rows; row += gridDim.x * EV_RPB) {
    // the member byte and the accumulator address do not depend on the walk; the whole group of 16 lanes takes the same branch
    const bool member = members ? members[row] != 0 : true;
    float* const ar = acc + (int64_t)row * ld_acc;
    const float* __restrict__ xr = x + (int64_t)row * ld;
    if (!member) continue;
    if (VEC) {
      mc_group<EV_GS, 0>(lane, n_classes, [&](int, int c, float (&v)[4]) {
        const float4 x4 = *reinterpret_cast<const float4*>(xr + c);  // c + 3 < ld: ld % 4 == 0 and c < n_classes <= ld
        v[0] = x4.x; v[1] = x4.y; v[2] = x4.z; v[3] = x4.w;
      }, first != 0, ar);
    } else {
      mc_group<EV_GS, 0>(lane, n_classes, [&](int, int c, float (&v)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = c + i < n_classes ? xr[c + i] : 0.f;  // nothing past the row's classes is read
      }, first != 0, ar);
    }
  }
}

// The statistics of `samples` accumulated samples, per row by its 16 lanes (lane i owns the quads i, i + 16, ... of the classes):
//   mean[c] = A[c] / T;  label = first-maximum argmax of mean;  std = sqrt(max(0, B[label] / T - mean[label]^2));
//   entropy = -sum_c mean[c] logf(mean[c]) (a zero term is 0; per lane in ascending column order, then the xor butterfly);
//   mutual information = max(0, entropy - E / T).
// Every requested output of every row in [0, n_rows) is written once: a row outside `members` holds -1 / 0; columns of `mean` at
// or past the classes are not written.
__global__ __launch_bounds__(256) void mc_finish_kernel(const float* __restrict__ acc, int ld_acc, int n_rows, int n_classes, int samples,
                                                        const uint8_t* __restrict__ members, int64_t* __restrict__ labels,
                                                        float* __restrict__ mean, int ld_mean, float* __restrict__ sd,
                                                        float* __restrict__ entropy, float* __restrict__ mi) {
  const int lane = threadIdx.x % EV_GS;
  const float T = (float)samples;
  for (int row = blockIdx.x * EV_RPB + (int)threadIdx.x / EV_GS; row < n_rows; row += gridDim.x * EV_RPB) {
    // the member byte and the addresses do not depend on the walk; the whole group of 16 lanes takes the same branch
    const bool member = members ? members[row] != 0 : true;
    const float* __restrict__ ar = acc + (int64_t)row * ld_acc;
    float* const mr = mean ? mean + (int64_t)row * ld_mean : nullptr;
    float best = -INFINITY, h = 0.f;
    int arg = ARGMAX_NONE;
    lane_quads<EV_GS, 0>(lane, n_classes, [&](int, int c) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (c + i >= n_classes) continue;
        const float p = member ? ar[c + i] / T : 0.f;
        if (mr) mr[c + i] = p;
        argmax_take(p, c + i, best, arg);
        h += p > 0.f ? p * logf(p) : 0.f;
      }
    });
    argmax_reduce_pair<EV_GS>(best, arg);
#pragma unroll
    for (int o = EV_GS / 2; o > 0; o >>= 1) h += __shfl_xor(h, o);
    if (lane == 0) {
      if (arg == ARGMAX_NONE) arg = 0;
      const float ent = 0.f - h;
      if (labels) labels[row] = member ? (int64_t)arg : -1;
      if (sd) sd[row] = member ? sqrtf(fmaxf(0.f, ar[mc_off_b(n_classes) + arg] / T - best * best)) : 0.f;
      if (entropy) entropy[row] = member ? ent : 0.f;
      if (mi) mi[row] = member ? fmaxf(0.f, ent - ar[mc_off_e(n_classes)] / T) : 0.f;
    }
  }
}

// ---- label histogram and balanced class weights (the class weights of the weighted cross entropy, computed where the labels live)
// counts[c] += #rows with label c that count ((mask == null || mask[row]) && label != ignored), c in [0, n_classes);
// counts[n_classes] += #counted rows whose label lies outside [0, n_classes).  HIST (n_classes <= LC_HIST_MAX): a per-workgroup
// LDS histogram and one 64-bit atomic per non-zero bin; else every row adds to the global bins directly.
constexpr int LC_HIST_MAX = 256;

template <bool HIST>
__global__ __launch_bounds__(256) void label_count_kernel(const int64_t* __restrict__ labels, int64_t n_rows, const uint8_t* __restrict__ mask,
                                                          int64_t ignored, int n_classes, unsigned long long* __restrict__ counts) {
  __shared__ int s_hist[HIST ? LC_HIST_MAX + 1 : 1];
  if (HIST) {
    for (int i = threadIdx.x; i <= n_classes; i += 256) s_hist[i] = 0;
    __syncthreads();
  }
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * 256) {
    if (mask && !mask[r]) continue;
    const int64_t y = labels[r];
    if (y == ignored) continue;
    const int bin = (y >= 0 && y < n_classes) ? (int)y : n_classes;
    if (HIST) atomicAdd(&s_hist[bin], 1);
    else atomicAdd(&counts[bin], 1ull);
  }
  if (HIST) {
    __syncthreads();
    for (int i = threadIdx.x; i <= n_classes; i += 256)
      if (s_hist[i]) atomicAdd(&counts[i], (unsigned long long)s_hist[i]);
  }
}

// scikit-learn's class_weight = "balanced" over the classes present: with K = #{c : n_c > 0} and N = sum n_c,
// w[c] = (float)((double)N / ((double)K * n_c)) for n_c > 0 and 0 for an absent class.  ONE workgroup; reads counts[0 .. n_classes)
// (the out-of-range slot is not part of N).
__global__ __launch_bounds__(256) void balanced_weights_kernel(const unsigned long long* __restrict__ counts, int n_classes,
                                                               float* __restrict__ w) {
  __shared__ unsigned long long s_n;
  __shared__ int s_k;
  if (threadIdx.x == 0) { s_n = 0ull; s_k = 0; }
  __syncthreads();
  unsigned long long n = 0ull;
  int k = 0;
  for (int c = threadIdx.x; c < n_classes; c += 256) {
    const unsigned long long nc = counts[c];
    n += nc;
    k += nc > 0 ? 1 : 0;
  }
  if (k) { atomicAdd(&s_n, n); atomicAdd(&s_k, k); }  // integer sums: any order gives the same totals
  __syncthreads();
  const double N = (double)s_n, K = (double)s_k;
  for (int c = threadIdx.x; c < n_classes; c += 256) {
    const unsigned long long nc = counts[c];
    w[c] = nc > 0 ? (float)(N / (K * (double)nc)) : 0.f;
  }
}

// ---- launch: one workgroup per EV_RPB rows up to the grid cap; VEC iff every row can be read by 16-byte loads
int ev_blocks(int n_rows) { return cdiv(n_rows, EV_RPB) < EV_MAX_BLOCKS ? cdiv(n_rows, EV_RPB) : EV_MAX_BLOCKS; }
bool ev_vec(const float* x, int ld) { return (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0; }

// launch(grid, std::bool_constant<VEC>) starts the kernel's VEC instantiation
template <class F>
int ev_launch(const float* x, int ld, int n_rows, F&& launch) {
  if (ev_vec(x, ld)) launch(dim3(ev_blocks(n_rows)), std::true_type());
  else launch(dim3(ev_blocks(n_rows)), std::false_type());
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

}  // namespace

int topk_rows_launch(const float* x, int ld, int n_rows, int n_classes, const uint8_t* members, int k, int64_t* labels, float* probs,
                     hipStream_t st) {
  HMP_CHECK_ARG(n_rows >= 0 && n_classes >= 1 && ld >= n_classes, "topk_rows: n_rows %d, n_classes %d, ld %d", n_rows, n_classes, ld);
  HMP_CHECK_ARG(k >= 1 && k <= TOPK_MAX, "topk_rows: k = %d (1 .. %d)", k, TOPK_MAX);
  if (n_rows == 0) return HMP_OK;
  HMP_CHECK_ARG(x && (labels || probs), "topk_rows: null logits or no output");
  return ev_launch(x, ld, n_rows, [&](dim3 grid, auto vec) {
    hipLaunchKernelGGL((topk_rows_kernel<vec()>), grid, dim3(256), 0, st, x, ld, n_rows, n_classes, members, k, labels, probs);
  });
}

int mc_rows_launch(const float* x, int ld, int n_rows, int n_classes, const uint8_t* members, int first, float* acc, int ld_acc,
                   hipStream_t st) {
  HMP_CHECK_ARG(n_rows >= 0 && n_classes >= 1 && ld >= n_classes, "mc_accumulate_rows: n_rows %d, n_classes %d, ld %d", n_rows, n_classes, ld);
  HMP_CHECK_ARG(ld_acc > mc_off_e(n_classes), "mc_accumulate_rows: ld_acc %d (%d classes need more than %d)", ld_acc, n_classes, mc_off_e(n_classes));
  if (n_rows == 0) return HMP_OK;
  HMP_CHECK_ARG(x && acc, "mc_accumulate_rows: null logits or accumulators");
  return ev_launch(x, ld, n_rows, [&](dim3 grid, auto vec) {
    hipLaunchKernelGGL((mc_rows_kernel<vec()>), grid, dim3(256), 0, st, x, ld, n_rows, n_classes, members, first, acc, ld_acc);
  });
}

int mc_finish_launch(const float* acc, int ld_acc, int n_rows, int n_classes, int samples, const uint8_t* members, int64_t* labels,
                     float* mean, int ld_mean, float* sd, float* entropy, float* mi, hipStream_t st) {
  HMP_CHECK_ARG(n_rows >= 0 && n_classes >= 1, "mc_finish: n_rows %d, n_classes %d", n_rows, n_classes);
  HMP_CHECK_ARG(ld_acc > mc_off_e(n_classes), "mc_finish: ld_acc %d (%d classes need more than %d)", ld_acc, n_classes, mc_off_e(n_classes));
  HMP_CHECK_ARG(samples >= 1 && samples <= MC_MAX_SAMPLES, "mc_finish: samples = %d (1 .. %d)", samples, MC_MAX_SAMPLES);
  HMP_CHECK_ARG(!mean || ld_mean >= n_classes, "mc_finish: ld_mean %d below the %d classes", ld_mean, n_classes);
  if (n_rows == 0) return HMP_OK;
  HMP_CHECK_ARG(acc && (labels || mean || sd || entropy || mi), "mc_finish: null accumulators or no output");
  hipLaunchKernelGGL(mc_finish_kernel, dim3(ev_blocks(n_rows)), dim3(256), 0, st, acc, ld_acc, n_rows, n_classes, samples, members, labels,
                     mean, ld_mean, sd, entropy, mi);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int predict_rows_launch(const float* x, int ld, int n_rows, int n_classes, const uint8_t* members, int64_t* pred, hipStream_t st) {
  HMP_CHECK_ARG(n_rows >= 0 && n_classes >= 1 && ld >= n_classes, "predict_rows: n_rows %d, n_classes %d, ld %d", n_rows, n_classes, ld);
  if (n_rows == 0) return HMP_OK;
  HMP_CHECK_ARG(x && pred, "predict_rows: null logits or output");
  return ev_launch(x, ld, n_rows, [&](dim3 grid, auto vec) {
    hipLaunchKernelGGL((predict_rows_kernel<vec()>), grid, dim3(256), 0, st, x, ld, n_rows, n_classes, members, pred);
  });
}

int count_rows_by_graph_launch(const float* x, int ld, int n_rows, int n_classes, const int64_t* labels, const uint8_t* members,
                               int64_t ignored, const int64_t* graph_ptr, int n_graphs, long long* counts, hipStream_t st) {
  HMP_CHECK_ARG(n_rows >= 0 && n_classes >= 1 && ld >= n_classes && n_graphs >= 0, "count_rows_by_graph: n_rows %d, n_classes %d, ld %d, n_graphs %d",
                n_rows, n_classes, ld, n_graphs);
  if (n_rows == 0) return HMP_OK;
  HMP_CHECK_ARG(n_graphs >= 1, "count_rows_by_graph: %d rows and no graph", n_rows);
  HMP_CHECK_ARG(x && labels && counts && graph_ptr, "count_rows_by_graph: null logits, labels, offsets or counts");
  auto* c = reinterpret_cast<unsigned long long*>(counts);
  return ev_launch(x, ld, n_rows, [&](dim3 grid, auto vec) {
    hipLaunchKernelGGL((count_rows_by_graph_kernel<vec()>), grid, dim3(256), 0, st, x, ld, n_rows, n_classes, labels, members, ignored,
                       graph_ptr, n_graphs, c);
  });
}

int count_rows_launch(const float* x, int ld, int n_rows, int n_classes, const int64_t* labels, const uint8_t* members,
                      int64_t ignored, long long* counts, long long* confusion, hipStream_t st) {
  HMP_CHECK_ARG(n_rows >= 0 && n_classes >= 1 && ld >= n_classes, "count_rows: n_rows %d, n_classes %d, ld %d", n_rows, n_classes, ld);
  if (n_rows == 0) return HMP_OK;
  HMP_CHECK_ARG(x && labels && counts, "count_rows: null logits, labels or counts");
  const bool hist = confusion && n_classes <= EV_HIST_MAX;
  auto* c = reinterpret_cast<unsigned long long*>(counts);
  auto* m = reinterpret_cast<unsigned long long*>(confusion);
  return ev_launch(x, ld, n_rows, [&](dim3 grid, auto vec) {
    if (hist) hipLaunchKernelGGL((count_rows_kernel<vec(), true>), grid, dim3(256), 0, st, x, ld, n_rows, n_classes, labels, members, ignored, c, m);
    else hipLaunchKernelGGL((count_rows_kernel<vec(), false>), grid, dim3(256), 0, st, x, ld, n_rows, n_classes, labels, members, ignored, c, m);
  });
}

int label_counts_launch(const int64_t* labels, int64_t n_rows, const uint8_t* mask, int64_t ignored, int n_classes, long long* counts,
                        hipStream_t st) {
  HMP_CHECK_ARG(n_rows >= 0 && n_classes >= 1, "label_counts: n_rows %lld, n_classes %d", (long long)n_rows, n_classes);
  if (n_rows == 0) return HMP_OK;
  HMP_CHECK_ARG(labels && counts, "label_counts: null labels or counts");
  const int64_t want = cdiv(n_rows, (int64_t)256);
  const dim3 grid((unsigned)(want < EV_MAX_BLOCKS ? want : EV_MAX_BLOCKS));
  auto* c = reinterpret_cast<unsigned long long*>(counts);
  if (n_classes <= LC_HIST_MAX) hipLaunchKernelGGL(label_count_kernel<true>, grid, dim3(256), 0, st, labels, n_rows, mask, ignored, n_classes, c);
  else hipLaunchKernelGGL(label_count_kernel<false>, grid, dim3(256), 0, st, labels, n_rows, mask, ignored, n_classes, c);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int balanced_weights_launch(const long long* counts, int n_classes, float* w, hipStream_t st) {
  HMP_CHECK_ARG(counts && w && n_classes >= 1, "balanced_class_weights: null pointer or n_classes %d", n_classes);
  hipLaunchKernelGGL(balanced_weights_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const unsigned long long*>(counts), n_classes, w);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

}  // namespace hmp

extern "C" int hmp_label_counts(const int64_t* d_labels, int64_t n_rows, const uint8_t* d_mask, int64_t ignored_label, int32_t n_classes,
                                int64_t* d_counts, void* stream) {
  using namespace hmp;
  return label_counts_launch(d_labels, n_rows, d_mask, ignored_label, n_classes, reinterpret_cast<long long*>(d_counts), (hipStream_t)stream);
}

extern "C" int hmp_balanced_class_weights(const int64_t* d_counts, int32_t n_classes, float* d_w, void* stream) {
  using namespace hmp;
  return balanced_weights_launch(reinterpret_cast<const long long*>(d_counts), n_classes, d_w, (hipStream_t)stream);
}

extern "C" int hmp_count_correct_rows(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const int64_t* d_labels,
                                      const uint8_t* d_members, int64_t ignored_label, int64_t* d_counts, int64_t* d_confusion,
                                      void* stream) {
  using namespace hmp;
  return count_rows_launch(d_logits, ld, n_rows, n_classes, d_labels, d_members, ignored_label, reinterpret_cast<long long*>(d_counts),
                           reinterpret_cast<long long*>(d_confusion), (hipStream_t)stream);
}

extern "C" int hmp_count_correct_rows_by_graph(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const int64_t* d_labels,
                                               const uint8_t* d_members, int64_t ignored_label, const int64_t* d_graph_ptr,
                                               int32_t n_graphs, int64_t* d_counts, void* stream) {
  using namespace hmp;
  return count_rows_by_graph_launch(d_logits, ld, n_rows, n_classes, d_labels, d_members, ignored_label, d_graph_ptr, n_graphs,
                                    reinterpret_cast<long long*>(d_counts), (hipStream_t)stream);
}

extern "C" int hmp_predict_rows(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const uint8_t* d_members,
                                int64_t* d_pred, void* stream) {
  using namespace hmp;
  return predict_rows_launch(d_logits, ld, n_rows, n_classes, d_members, d_pred, (hipStream_t)stream);
}

extern "C" int hmp_topk_rows(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const uint8_t* d_members, int32_t k,
                             int64_t* d_labels, float* d_probs, void* stream) {
  using namespace hmp;
  return topk_rows_launch(d_logits, ld, n_rows, n_classes, d_members, k, d_labels, d_probs, (hipStream_t)stream);
}

extern "C" int32_t hmp_mc_acc_ld(int32_t n_classes) { return n_classes >= 1 ? hmp::mc_acc_ld(n_classes) : 0; }

extern "C" int hmp_mc_accumulate_rows(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const uint8_t* d_members,
                                      int32_t first, float* d_acc, int32_t ld_acc, void* stream) {
  using namespace hmp;
  return mc_rows_launch(d_logits, ld, n_rows, n_classes, d_members, first, d_acc, ld_acc, (hipStream_t)stream);
}

extern "C" int hmp_mc_finish(const float* d_acc, int32_t ld_acc, int32_t n_rows, int32_t n_classes, int32_t samples,
                             const uint8_t* d_members, int64_t* d_labels, float* d_mean, int32_t ld_mean, float* d_std, float* d_entropy,
                             float* d_mi, void* stream) {
  using namespace hmp;
  return mc_finish_launch(d_acc, ld_acc, n_rows, n_classes, samples, d_members, d_labels, d_mean, ld_mean, d_std, d_entropy, d_mi,
                          (hipStream_t)stream);
}
