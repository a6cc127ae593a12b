// Epoch bookkeeping of a training job on the device (include/hydra_mp.h section 13; hydra_gnn_amd/jobs.py).
//
// The host loop of BaseTrainingJob.train (base_training_job.py:196-246) reads the loss after every step, the validation count after
// every epoch and deep-copies the state dict on every improvement.  Here the same numbers live in one small device record:
//
//   accumulate (after a step)          loss_acc += loss * w, weight_acc += w                                  1 thread
//   close      (after the val pass)    launch 1: copy model state -> snapshot iff this epoch improves         grid_blocks x 256
//                                      launch 2: log row, max / best_epoch / early-stop, zero the sums        1 thread
//   restore    (after the loop)        snapshot -> model state                                               grid_blocks x 256
//
// Ordering of close: whether the epoch improves is a function of {d_counts, ctl.max_val_acc, ctl.epoch} and two arguments.  Launch 1
// only READS those words, every workgroup evaluates the same predicate on them and copies its share of the segments; launch 2,
// which follows in stream order, is the only writer.  So no workgroup can see a half-updated record whatever the grid size, and no
// fence, ticket or atomic is needed.  The price is one extra ~1-thread launch per EPOCH.
//
// The sums are double and are formed exactly like the host loop's `total_loss += loss * w`: a rounded product, then a rounded sum
// (__dmul_rn / __dadd_rn keep the compiler from contracting them into one fma), so a job's per-epoch loss is bit-equal to the hand
// loop's.  Only plain vector loads and stores are used.
#include "common.h"

namespace hmp {

namespace {

constexpr int EP_THREADS = 256;
constexpr int EP_MAX_BLOCKS = 1024;

struct EpochCounts {
  long long correct, total;
};

__device__ __forceinline__ EpochCounts epoch_counts(const long long* counts, int n_counts) {
  EpochCounts c{counts[0], counts[1]};
  if (n_counts == 4) {  // rooms + objects (semisupervised_training_job.py:258)
    c.correct += counts[2];
    c.total += counts[3];
  }
  return c;
}

__device__ __forceinline__ bool epoch_improves(const hmp_epoch_ctl* ctl, const EpochCounts& c, int min_log_epoch) {
  if (c.total <= 0) return false;
  const double acc = (double)c.correct / (double)c.total;
  return ctl->epoch >= min_log_epoch && acc > ctl->max_val_acc;
}

// every segment, the workgroups of the grid striding over it: 16-byte units when both ends are 16-byte aligned, the remainder (and
// unaligned segments) byte by byte
template <bool TO_SNAPSHOT>
__device__ __forceinline__ void copy_segments(const hmp_epoch_seg* segs, int n_segs) {
  const int64_t tid = (int64_t)blockIdx.x * EP_THREADS + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * EP_THREADS;
  for (int s = 0; s < n_segs; ++s) {
    const unsigned char* src = static_cast<const unsigned char*>(TO_SNAPSHOT ? segs[s].src : segs[s].dst);
    unsigned char* dst = static_cast<unsigned char*>(TO_SNAPSHOT ? segs[s].dst : const_cast<void*>(segs[s].src));
    const int64_t bytes = segs[s].bytes;
    int64_t done = 0;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
      const int64_t nvec = bytes >> 4;
      const uint4* s4 = reinterpret_cast<const uint4*>(src);
      uint4* d4 = reinterpret_cast<uint4*>(dst);
      for (int64_t i = tid; i < nvec; i += stride) d4[i] = s4[i];
      done = nvec << 4;
    }
    for (int64_t i = done + tid; i < bytes; i += stride) dst[i] = src[i];
  }
}

__global__ __launch_bounds__(EP_THREADS) void epoch_keep_kernel(const hmp_epoch_ctl* ctl, const long long* counts, int n_counts,
                                                               int min_log_epoch, const hmp_epoch_seg* segs, int n_segs) {
  if (!epoch_improves(ctl, epoch_counts(counts, n_counts), min_log_epoch)) return;
  copy_segments<true>(segs, n_segs);
}

__global__ __launch_bounds__(EP_THREADS) void epoch_restore_kernel(const hmp_epoch_seg* segs, int n_segs) {
  copy_segments<false>(segs, n_segs);
}

__global__ void epoch_update_kernel(hmp_epoch_ctl* ctl, hmp_epoch_row* log, int log_cap, long long* counts, int n_counts,
                                    double loss_div, int min_log_epoch, int early_stop_window) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const EpochCounts c = epoch_counts(counts, n_counts);
  const bool improved = epoch_improves(ctl, c, min_log_epoch);
  const int epoch = ctl->epoch;
  const double acc = c.total > 0 ? (double)c.correct / (double)c.total : 0.0;
  if (epoch < log_cap) {
    hmp_epoch_row r;
    r.loss = ctl->loss_acc / (loss_div > 0.0 ? loss_div : ctl->weight_acc);
    r.val_acc = acc;
    r.correct = c.correct;
    r.total = c.total;
    r.improved = improved ? 1 : 0;
    r.pad_ = 0;
    log[epoch] = r;
  }
  int status = ctl->status;
  if (c.total <= 0) status |= HMP_EPOCH_EMPTY_VAL;
  int ess = ctl->early_stop_step + 1;  // base_training_job.py:198
  if (improved) {
    ctl->max_val_acc = acc;
    ctl->best_epoch = epoch;
    ess = 0;  // :236
  }
  if (ess == early_stop_window && epoch > early_stop_window) status |= HMP_EPOCH_STOP;  // :243
  ctl->early_stop_step = ess;
  ctl->status = status;
  ctl->loss_acc = 0.0;
  ctl->weight_acc = 0.0;
  ctl->epoch = epoch + 1;
  for (int i = 0; i < n_counts; ++i) counts[i] = 0;
}

__global__ void epoch_accumulate_kernel(hmp_epoch_ctl* ctl, const float* loss, const float* loss_count, const long long* d_weight,
                                        double weight) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double l = (double)loss[0];
  double cnt = 0.0;
  if (loss_count) {
    cnt = (double)loss_count[0];
    l = l / (cnt > 0.0 ? cnt : 1.0);  // TrainStep.loss(): loss_sum / (count > 0 ? count : 1) on the two floats, in double
  }
  const double w = d_weight ? (double)d_weight[0] : (weight >= 0.0 ? weight : cnt);
  ctl->loss_acc = __dadd_rn(ctl->loss_acc, __dmul_rn(l, w));
  ctl->weight_acc = __dadd_rn(ctl->weight_acc, w);
}

int copy_grid(int grid_blocks) { return grid_blocks < 1 ? 1 : (grid_blocks > EP_MAX_BLOCKS ? EP_MAX_BLOCKS : grid_blocks); }

}  // namespace

}  // namespace hmp

extern "C" {

int hmp_epoch_accumulate(hmp_epoch_ctl* d_ctl, const float* d_loss, const float* d_loss_count, const int64_t* d_weight,
                         double weight, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_ctl && d_loss, "hmp_epoch_accumulate: null record or loss");
  HMP_CHECK_ARG(d_weight || weight >= 0.0 || d_loss_count, "hmp_epoch_accumulate: no weight (d_weight, weight >= 0 or d_loss_count)");
  hipLaunchKernelGGL(epoch_accumulate_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, d_ctl, d_loss, d_loss_count,
                     reinterpret_cast<const long long*>(d_weight), weight);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int hmp_epoch_close(hmp_epoch_ctl* d_ctl, hmp_epoch_row* d_log, int32_t log_cap, int64_t* d_counts, int32_t n_counts,
                    double loss_div, int32_t min_log_epoch, int32_t early_stop_window, const hmp_epoch_seg* d_segs,
                    int32_t n_segs, int32_t grid_blocks, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_ctl && d_counts, "hmp_epoch_close: null record or counters");
  HMP_CHECK_ARG(n_counts == 2 || n_counts == 4, "hmp_epoch_close: n_counts %d (2: room task, 4: two-headed task)", n_counts);
  HMP_CHECK_ARG(log_cap >= 0 && (d_log || log_cap == 0), "hmp_epoch_close: log_cap %d without a log", log_cap);
  HMP_CHECK_ARG(n_segs >= 0 && n_segs <= HMP_EPOCH_MAX_SEGS && (d_segs || n_segs == 0), "hmp_epoch_close: %d segments (at most %d)",
                n_segs, HMP_EPOCH_MAX_SEGS);
  auto* counts = reinterpret_cast<long long*>(d_counts);
  if (n_segs > 0) {
    hipLaunchKernelGGL(epoch_keep_kernel, dim3(copy_grid(grid_blocks)), dim3(EP_THREADS), 0, (hipStream_t)stream, d_ctl, counts,
                       n_counts, min_log_epoch, d_segs, n_segs);
    HMP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(epoch_update_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, d_ctl, d_log, log_cap, counts, n_counts,
                     loss_div, min_log_epoch, early_stop_window);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int hmp_epoch_restore(const hmp_epoch_seg* d_segs, int32_t n_segs, int32_t grid_blocks, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(n_segs >= 0 && n_segs <= HMP_EPOCH_MAX_SEGS && (d_segs || n_segs == 0), "hmp_epoch_restore: %d segments (at most %d)",
                n_segs, HMP_EPOCH_MAX_SEGS);
  if (n_segs == 0) return HMP_OK;
  hipLaunchKernelGGL(epoch_restore_kernel, dim3(copy_grid(grid_blocks)), dim3(EP_THREADS), 0, (hipStream_t)stream, d_segs, n_segs);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int hmp_epoch_read(const hmp_epoch_ctl* d_ctl, const hmp_epoch_row* d_log, int32_t log_cap, hmp_epoch_ctl* h_ctl,
                   hmp_epoch_row* h_rows, int32_t* n_rows, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_ctl && h_ctl, "hmp_epoch_read: null record");
  HMP_HIP(hipStreamSynchronize((hipStream_t)stream));
  HMP_HIP(hipMemcpy(h_ctl, d_ctl, sizeof(hmp_epoch_ctl), hipMemcpyDeviceToHost));
  int n = h_ctl->epoch < log_cap ? h_ctl->epoch : log_cap;
  if (n < 0 || !d_log || !h_rows) n = 0;
  if (n > 0) HMP_HIP(hipMemcpy(h_rows, d_log, (size_t)n * sizeof(hmp_epoch_row), hipMemcpyDeviceToHost));
  if (n_rows) *n_rows = n;
  return HMP_OK;
}

int hmp_epoch_read_status(const hmp_epoch_ctl* d_ctl, int32_t* status, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_ctl && status, "hmp_epoch_read_status: null argument");
  HMP_HIP(hipStreamSynchronize((hipStream_t)stream));
  HMP_HIP(hipMemcpy(status, &d_ctl->status, sizeof(int32_t), hipMemcpyDeviceToHost));
  return HMP_OK;
}

}  // extern "C"
