// Room-task validation count: the per-batch arithmetic of BaseTrainingJob.test (base_training_job.py:269-313) on the device.
//
//   pred = argmax(logits, dim=1) (first maximum);  a row counts iff (members == null || members[row]) && label != ignored;
//   counts += {#(pred == label), #rows};  confusion[label][pred] += 1 for counted rows with label in [0, n_classes).
//
// A row belongs to a group of 16 lanes (argmax_rows_kernel's grouping, optim.hip).  With ld % 4 == 0 and a 16-byte aligned base,
// lane i owns the quads i, i + 16, ... of the row (16-byte loads); otherwise lane i owns the columns i, i + 16, ...  Both walk
// their columns in ascending order and keep the first maximum, and the group reduction breaks ties by the lower index, so the
// prediction is argmax_rows_kernel's (and torch.argmax's on finite logits) whatever the layout.
//
// Per-workgroup counters live in LDS; each workgroup adds its non-zero counters to the int64 outputs with one 64-bit atomic each.
// For n_classes <= EV_HIST_MAX the confusion matrix is an LDS histogram too (<= 16 KB of int32), above that rows add to the global
// matrix directly.  Everything is ACCUMULATED (+=): a validation pass sums its batches on the device and reads the totals once.
#include "kernels.h"

namespace hmp {

namespace {

constexpr int EV_GS = 16;               // lanes per row
constexpr int EV_RPB = 256 / EV_GS;     // rows per workgroup and pass
constexpr int EV_HIST_MAX = 64;         // largest class count with an LDS confusion histogram
constexpr int EV_MAX_BLOCKS = 1024;     // grid cap: larger inputs stride over rows (fewer histogram flushes)
constexpr int EV_NONE = 0x7fffffff;

__device__ __forceinline__ void ev_take(float v, int c, float& best, int& arg) {
  if (v > best || arg == EV_NONE) { best = v; arg = c; }
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
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x % EV_GS;
  for (int row = blockIdx.x * EV_RPB + (int)threadIdx.x / EV_GS; row < n_rows; row += gridDim.x * EV_RPB) {
    // the whole group of 16 lanes takes the same branch: the shuffles below stay inside active groups
    const int64_t y = labels[row];
    if ((members && !members[row]) || y == ignored) continue;
    float best = -INFINITY;
    int arg = EV_NONE;
    const float* xr = x + (int64_t)row * ld;
    if (VEC) {
      for (int c = lane * 4; c < n_classes; c += EV_GS * 4) {
        const float4 v = *reinterpret_cast<const float4*>(xr + c);  // c + 3 < ld: ld % 4 == 0 and c < n_classes <= ld
        ev_take(v.x, c, best, arg);
        if (c + 1 < n_classes) ev_take(v.y, c + 1, best, arg);
        if (c + 2 < n_classes) ev_take(v.z, c + 2, best, arg);
        if (c + 3 < n_classes) ev_take(v.w, c + 3, best, arg);
      }
    } else {
      for (int c = lane; c < n_classes; c += EV_GS) ev_take(xr[c], c, best, arg);
    }
#pragma unroll
    for (int o = EV_GS / 2; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, EV_GS);
      const int oa = __shfl_xor(arg, o, EV_GS);
      if (oa != EV_NONE && (arg == EV_NONE || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
    }
    if (lane == 0) {
      const int pred = arg == EV_NONE ? 0 : arg;
      atomicAdd(&s_cnt[1], 1);
      // a label outside [0, n_classes) is never predicted: it counts in the total only (pred.eq(label) is false)
      if (y >= 0 && y < n_classes) {
        if (pred == (int)y) atomicAdd(&s_cnt[0], 1);
        if (HIST) atomicAdd(&s_hist[(int)y * n_classes + pred], 1);
        else if (confusion) atomicAdd(&confusion[y * n_classes + pred], 1ull);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
  for (int i = threadIdx.x; i < cc; i += 256)
    if (s_hist[i]) atomicAdd(&confusion[i], (unsigned long long)s_hist[i]);
}

}  // namespace

int count_rows_launch(const float* x, int ld, int n_rows, int n_classes, const int64_t* labels, const uint8_t* members,
                      int64_t ignored, long long* counts, long long* confusion, hipStream_t st) {
  HMP_CHECK_ARG(n_rows >= 0 && n_classes >= 1 && ld >= n_classes, "count_rows: n_rows %d, n_classes %d, ld %d", n_rows, n_classes, ld);
  if (n_rows == 0) return HMP_OK;
  HMP_CHECK_ARG(x && labels && counts, "count_rows: null logits, labels or counts");
  const int blocks = cdiv(n_rows, EV_RPB) < EV_MAX_BLOCKS ? cdiv(n_rows, EV_RPB) : EV_MAX_BLOCKS;
  const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const bool hist = confusion && n_classes <= EV_HIST_MAX;
  auto* c = reinterpret_cast<unsigned long long*>(counts);
  auto* m = reinterpret_cast<unsigned long long*>(confusion);
  if (vec && hist)
    hipLaunchKernelGGL((count_rows_kernel<true, true>), dim3(blocks), dim3(256), 0, st, x, ld, n_rows, n_classes, labels, members, ignored, c, m);
  else if (vec)
    hipLaunchKernelGGL((count_rows_kernel<true, false>), dim3(blocks), dim3(256), 0, st, x, ld, n_rows, n_classes, labels, members, ignored, c, m);
  else if (hist)
    hipLaunchKernelGGL((count_rows_kernel<false, true>), dim3(blocks), dim3(256), 0, st, x, ld, n_rows, n_classes, labels, members, ignored, c, m);
  else
    hipLaunchKernelGGL((count_rows_kernel<false, false>), dim3(blocks), dim3(256), 0, st, x, ld, n_rows, n_classes, labels, members, ignored, c, m);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

}  // namespace hmp

extern "C" int hmp_count_correct_rows(const float* d_logits, int32_t ld, int32_t n_rows, int32_t n_classes, const int64_t* d_labels,
                                      const uint8_t* d_members, int64_t ignored_label, int64_t* d_counts, int64_t* d_confusion,
                                      void* stream) {
  using namespace hmp;
  return count_rows_launch(d_logits, ld, n_rows, n_classes, d_labels, d_members, ignored_label, reinterpret_cast<long long*>(d_counts),
                           reinterpret_cast<long long*>(d_confusion), (hipStream_t)stream);
}
