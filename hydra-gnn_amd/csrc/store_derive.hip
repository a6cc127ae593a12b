// Derived variants of a device-resident dataset (hydra_gnn_amd/store.py GraphStore): the reference derives every configuration
// from one loaded dataset in place -- compute_relative_pos (GAT_edge), to_homogeneous, remove_last_features (mp3d_dataset.py:29-119,
// :286-319) -- and draws the node split of the Stanford protocol per run (Stanford3DSG_dataset.py:459-578).  Here the dataset is
// packed arrays in HBM (all graphs' rows back to back, graph-local edge lists, [G + 1] offset vectors), and a transform is ONE
// launch over the whole store: the host plans an item per (output array, source array) pair plus the [G] destination offsets of
// every item (numpy over the offset vectors it keeps), uploads both in one block, and hmp_store_derive runs the items.
//   rows    dst[dst_off[g] + i][0 .. dst_w) = src[src_ptr[g] + i][skip .. skip + take) then zeros          (units of 16 / 4 / 1 bytes)
//   fill    dst[dst_off[g] + i] = value,  i < src_ptr[g + 1] - src_ptr[g]                                   (int64 or one byte)
//   edges   dst[r][dst_off[g] + j] = src[r][src_ptr[g] + j] + shift_r[g]                                    (graph-local int64 [2][E])
//   relpos  dst[j][c] = pos_dst[ptr_dst[g] + src[1][j]][c] - pos_src[ptr_src[g] + src[0][j]][c],  c < 3     (a plain subtraction)
//   compact   the rows of graph g whose key[row] is NOT in a 64-bit set, in order, from dst row dst_off[g] on  (one wave per graph)
//   rows_zero dst[dst_off[g] + i] = key[row] in the set ? zeros : src[src_ptr[g] + i]                        (units of 16 / 4 / 1 bytes)
// Every item walks its SOURCE rows, so every output element is written exactly once as long as the plan tiles the outputs (the
// planner's job; tests run with outputs pre-filled).  No atomics.  Byte work, HBM-bound.
#include "device_fns.h"  // find_seg

namespace hmp {

template <typename U>
__device__ __forceinline__ U sd_zero() {
  return U(0);
}
template <>
__device__ __forceinline__ uint4 sd_zero<uint4>() {
  return make_uint4(0u, 0u, 0u, 0u);
}

// thread per destination unit; the row's graph comes from a search in the item's [G + 1] source offsets
template <typename U>
__device__ __forceinline__ void sd_rows(const int64_t* __restrict__ I, int G, int64_t first, int64_t stride) {
  const U* __restrict__ src = reinterpret_cast<const U*>(I[HMP_SD_SRC]);
  U* __restrict__ dst = reinterpret_cast<U*>(I[HMP_SD_DST]);
  const int64_t* __restrict__ sp = reinterpret_cast<const int64_t*>(I[HMP_SD_SRC_PTR]);
  const int64_t* __restrict__ dof = reinterpret_cast<const int64_t*>(I[HMP_SD_DST_OFF]);
  const int64_t sw = I[HMP_SD_SRC_W], skip = I[HMP_SD_SKIP], take = I[HMP_SD_TAKE], dw = I[HMP_SD_DST_W];
  const int64_t total = I[HMP_SD_N] * dw;
  for (int64_t idx = first; idx < total; idx += stride) {
    const int64_t row = idx / dw, u = idx - row * dw;
    const int g = find_seg(sp, G, row);
    const int64_t drow = dof[g] + (row - sp[g]);
    dst[drow * dw + u] = u < take ? src[row * sw + skip + u] : sd_zero<U>();
  }
}

template <typename U>
__device__ __forceinline__ void sd_fill(const int64_t* __restrict__ I, int G, int64_t first, int64_t stride) {
  U* __restrict__ dst = reinterpret_cast<U*>(I[HMP_SD_DST]);
  const int64_t* __restrict__ sp = reinterpret_cast<const int64_t*>(I[HMP_SD_SRC_PTR]);
  const int64_t* __restrict__ dof = reinterpret_cast<const int64_t*>(I[HMP_SD_DST_OFF]);
  const U value = (U)I[HMP_SD_A0];
  const int64_t total = I[HMP_SD_N];
  for (int64_t row = first; row < total; row += stride) {
    const int g = find_seg(sp, G, row);
    dst[dof[g] + (row - sp[g])] = value;
  }
}

// a key outside [0, 64) is in no set
__device__ __forceinline__ bool sd_in_set(uint64_t set, int64_t key) {
  return (uint64_t)key < 64u && ((set >> (uint64_t)key) & 1ull) != 0;
}

// rows copied, zeroed where the row's key is in the set: thread per destination unit, as sd_rows (skip 0, take = the whole row)
template <typename U>
__device__ __forceinline__ void sd_rows_zero(const int64_t* __restrict__ I, int G, int64_t first, int64_t stride) {
  const U* __restrict__ src = reinterpret_cast<const U*>(I[HMP_SD_SRC]);
  U* __restrict__ dst = reinterpret_cast<U*>(I[HMP_SD_DST]);
  const int64_t* __restrict__ sp = reinterpret_cast<const int64_t*>(I[HMP_SD_SRC_PTR]);
  const int64_t* __restrict__ dof = reinterpret_cast<const int64_t*>(I[HMP_SD_DST_OFF]);
  const int64_t* __restrict__ key = reinterpret_cast<const int64_t*>(I[HMP_SD_A0]);
  const uint64_t set = (uint64_t)I[HMP_SD_A1];
  const int64_t w = I[HMP_SD_DST_W];
  const int64_t total = I[HMP_SD_N] * w;
  for (int64_t idx = first; idx < total; idx += stride) {
    const int64_t row = idx / w, u = idx - row * w;
    const int g = find_seg(sp, G, row);
    const int64_t drow = dof[g] + (row - sp[g]);
    dst[drow * w + u] = sd_in_set(set, key[row]) ? sd_zero<U>() : src[row * w + u];
  }
}

// rows compacted by a key vector: a wave per graph (waves stride over the graphs), 64 source rows per sweep; a kept row's rank
// among the kept rows of its graph = kept rows of the earlier sweeps + popcount of the ballot below the lane, so the order is the
// source's and every destination row of the graph is written once (the plan's dst_off comes from the same count, store_count_kept)
template <typename U>
__device__ __forceinline__ void sd_compact(const int64_t* __restrict__ I, int G, int nb) {
  const U* __restrict__ src = reinterpret_cast<const U*>(I[HMP_SD_SRC]);
  U* __restrict__ dst = reinterpret_cast<U*>(I[HMP_SD_DST]);
  const int64_t* __restrict__ sp = reinterpret_cast<const int64_t*>(I[HMP_SD_SRC_PTR]);
  const int64_t* __restrict__ dof = reinterpret_cast<const int64_t*>(I[HMP_SD_DST_OFF]);
  const int64_t* __restrict__ key = reinterpret_cast<const int64_t*>(I[HMP_SD_A0]);
  const uint64_t set = (uint64_t)I[HMP_SD_A1];
  const int64_t w = I[HMP_SD_DST_W];
  const int lane = threadIdx.x & 63;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const int64_t wave0 = ((int64_t)blockIdx.x - I[HMP_SD_BLOCK0]) * 4 + (threadIdx.x >> 6);
  for (int64_t g = wave0; g < G; g += (int64_t)nb * 4) {
    const int64_t r0 = sp[g], n = sp[g + 1] - r0;
    int64_t out = dof[g];
    for (int64_t base = 0; base < n; base += 64) {
      const int64_t i = base + lane;
      const bool keep = i < n && !sd_in_set(set, key[r0 + i]);
      const unsigned long long b = __ballot(keep);
      if (keep) {
        const U* s = src + (r0 + i) * w;
        U* d = dst + (out + __popcll(b & below)) * w;
        for (int64_t u = 0; u < w; ++u) d[u] = s[u];
      }
      out += __popcll(b);
    }
  }
}

__device__ __forceinline__ void sd_item(const int64_t* __restrict__ I, int G, int nb) {
  const int64_t first = ((int64_t)blockIdx.x - I[HMP_SD_BLOCK0]) * 256 + threadIdx.x;
  const int64_t stride = (int64_t)nb * 256;
  const int64_t unit = I[HMP_SD_UNIT];
  switch ((int)I[HMP_SD_KIND]) {
    case HMP_SD_ROWS:
      if (unit == 16) sd_rows<uint4>(I, G, first, stride);
      else if (unit == 4) sd_rows<uint32_t>(I, G, first, stride);
      else sd_rows<uint8_t>(I, G, first, stride);
      break;
    case HMP_SD_FILL:
      if (unit == 8) sd_fill<int64_t>(I, G, first, stride);
      else sd_fill<uint8_t>(I, G, first, stride);
      break;
    case HMP_SD_EDGES: {
      const int64_t* __restrict__ src = reinterpret_cast<const int64_t*>(I[HMP_SD_SRC]);
      int64_t* __restrict__ dst = reinterpret_cast<int64_t*>(I[HMP_SD_DST]);
      const int64_t* __restrict__ sp = reinterpret_cast<const int64_t*>(I[HMP_SD_SRC_PTR]);
      const int64_t* __restrict__ dof = reinterpret_cast<const int64_t*>(I[HMP_SD_DST_OFF]);
      const int64_t* __restrict__ s0 = reinterpret_cast<const int64_t*>(I[HMP_SD_A0]);
      const int64_t* __restrict__ s1 = reinterpret_cast<const int64_t*>(I[HMP_SD_A1]);
      const int64_t n = I[HMP_SD_N], pitch = I[HMP_SD_A3];
      for (int64_t j = first; j < n; j += stride) {
        const int g = find_seg(sp, G, j);
        const int64_t d = dof[g] + (j - sp[g]);
        dst[d] = src[j] + s0[g];
        dst[pitch + d] = src[n + j] + s1[g];
      }
      break;
    }
    case HMP_SD_RELPOS: {
      const int64_t* __restrict__ ei = reinterpret_cast<const int64_t*>(I[HMP_SD_SRC]);
      float* __restrict__ dst = reinterpret_cast<float*>(I[HMP_SD_DST]);
      const int64_t* __restrict__ sp = reinterpret_cast<const int64_t*>(I[HMP_SD_SRC_PTR]);
      const float* __restrict__ ps = reinterpret_cast<const float*>(I[HMP_SD_A0]);
      const float* __restrict__ pd = reinterpret_cast<const float*>(I[HMP_SD_A1]);
      const int64_t* __restrict__ ns = reinterpret_cast<const int64_t*>(I[HMP_SD_A2]);
      const int64_t* __restrict__ nd = reinterpret_cast<const int64_t*>(I[HMP_SD_A3]);
      const int64_t n = I[HMP_SD_N];
      for (int64_t j = first; j < n; j += stride) {
        const int g = find_seg(sp, G, j);
        const float* a = ps + (ns[g] + ei[j]) * 3;
        const float* b = pd + (nd[g] + ei[n + j]) * 3;
        float* o = dst + j * 3;
        o[0] = b[0] - a[0];
        o[1] = b[1] - a[1];
        o[2] = b[2] - a[2];
      }
      break;
    }
    case HMP_SD_COMPACT:
      if (unit == 8) sd_compact<uint64_t>(I, G, nb);
      else sd_compact<uint32_t>(I, G, nb);
      break;
    case HMP_SD_ROWS_ZERO:
      if (unit == 16) sd_rows_zero<uint4>(I, G, first, stride);
      else if (unit == 4) sd_rows_zero<uint32_t>(I, G, first, stride);
      else sd_rows_zero<uint8_t>(I, G, first, stride);
      break;
    default:
      break;
  }
}

// Block: [group table: one int64 per 64 items = HMP_SD_BLOCK0 of the group's first item, padded to an even count][item table].
// A workgroup finds its group and then its item the way frame_expand_batch_kernel does: the last one whose first workgroup is
// not behind this one, one 64-lane load and one ballot each (the prefix words increase: every item has work).
__global__ __launch_bounds__(256) void store_derive_kernel(const int64_t* __restrict__ block, int n_items, int n_blocks, int G) {
  const int lane = threadIdx.x & 63;
  const int n_groups = (n_items + 63) / 64;
  const int64_t* items = block + ((n_groups + 1) & ~1);
  const int64_t bx = blockIdx.x;
  const int64_t g0 = lane < n_groups ? block[lane] : INT64_MAX;
  const int gi = __popcll(__ballot(g0 <= bx)) - 1;
  if (gi < 0) return;
  const int it = gi * 64 + lane;
  const int64_t b0 = it < n_items ? items[(int64_t)it * HMP_SD_ITEM_WORDS + HMP_SD_BLOCK0] : INT64_MAX;
  const int ii = gi * 64 + __popcll(__ballot(b0 <= bx)) - 1;
  if (ii < gi * 64) return;
  const int64_t* I = items + (int64_t)ii * HMP_SD_ITEM_WORDS;
  // the item's workgroups end where the next item begins
  const int64_t end = ii + 1 < n_items ? I[HMP_SD_ITEM_WORDS + HMP_SD_BLOCK0] : n_blocks;
  sd_item(I, G, (int)(end - I[HMP_SD_BLOCK0]));
}

// ---- node split ------------------------------------------------------------------------------------------------------------
// One wave per graph.  assign [total] int8 (0 unassigned, 1 train, 2 val, 3 test) in the order the reference walks the graphs;
// assign_off [G + 1] = where a graph's members start.  Typed: part a (objects / object_virtual) then part b (rooms /
// room_virtual), each with its own [G + 1] row offsets and three mask rows.  Homogeneous baseline: part a alone (every node).
// Homogeneous H-tree (members given): the rows of member_a are ranked first, then those of member_b, with ballot prefixes; every
// other row gets false.
struct SplitArgs {
  const int8_t* assign;
  const int64_t* assign_off;
  const int64_t* ptr_a;
  const int64_t* ptr_b;
  const uint8_t* member_a;
  const uint8_t* member_b;
  uint8_t* mask_a[3];
  uint8_t* mask_b[3];
  int G;
};

__device__ __forceinline__ void split_write(uint8_t* const* mask, int64_t row, int a) {
  mask[0][row] = a == 1;
  mask[1][row] = a == 2;
  mask[2][row] = a == 3;
}

__global__ __launch_bounds__(256) void store_node_split_kernel(const SplitArgs A) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= A.G) return;
  const int8_t* as = A.assign + A.assign_off[g];
  const int64_t a0 = A.ptr_a[g], na = A.ptr_a[g + 1] - a0;
  if (A.member_a == nullptr) {
    for (int64_t i = lane; i < na; i += 64) split_write(A.mask_a, a0 + i, as[i]);
    if (A.ptr_b != nullptr) {
      const int64_t b0 = A.ptr_b[g], nb = A.ptr_b[g + 1] - b0;
      for (int64_t i = lane; i < nb; i += 64) split_write(A.mask_b, b0 + i, as[na + i]);
    }
    return;
  }
  // ranked members: count part a's rows first (part b's ranks start behind them)
  int64_t n_obj = 0;
  for (int64_t base = 0; base < na; base += 64) {
    const int64_t i = base + lane;
    n_obj += __popcll(__ballot(i < na && A.member_a[a0 + i] != 0));
  }
  int64_t ra = 0, rb = n_obj;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int64_t base = 0; base < na; base += 64) {
    const int64_t i = base + lane;
    const bool in = i < na;
    const bool ma = in && A.member_a[a0 + i] != 0, mb = in && A.member_b[a0 + i] != 0;
    const unsigned long long ba = __ballot(ma), bb = __ballot(mb);
    // the reference writes the object rows, then the room rows: a row of both sets ends up with its room assignment
    int a = 0;
    if (mb) a = as[rb + __popcll(bb & below)];
    else if (ma) a = as[ra + __popcll(ba & below)];
    if (in) split_write(A.mask_a, a0 + i, a);
    ra += __popcll(ba);
    rb += __popcll(bb);
  }
}

// counts [2][G]: rows of member_a / member_b per graph (what the reference's num_graph_nodes sums on a homogeneous H-tree)
__global__ __launch_bounds__(256) void store_member_counts_kernel(const uint8_t* __restrict__ member_a, const uint8_t* __restrict__ member_b,
                                                                  const int64_t* __restrict__ ptr, int G, int64_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;
  const int64_t r0 = ptr[g], n = ptr[g + 1] - r0;
  int64_t ca = 0, cb = 0;
  for (int64_t base = 0; base < n; base += 64) {
    const int64_t i = base + lane;
    ca += __popcll(__ballot(i < n && member_a[r0 + i] != 0));
    cb += __popcll(__ballot(i < n && member_b[r0 + i] != 0));
  }
  if (lane == 0) {
    counts[g] = ca;
    counts[G + g] = cb;
  }
}

// counts [G]: the rows of a graph whose key is not in the set (what an HMP_SD_COMPACT item keeps)
__global__ __launch_bounds__(256) void store_count_kept_kernel(const int64_t* __restrict__ key, const int64_t* __restrict__ ptr, int G,
                                                               uint64_t set, int64_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < G; g += waves) {
    const int64_t r0 = ptr[g], n = ptr[g + 1] - r0;
    int64_t c = 0;
    for (int64_t base = 0; base < n; base += 64) {
      const int64_t i = base + lane;
      c += __popcll(__ballot(i < n && !sd_in_set(set, key[r0 + i])));
    }
    if (lane == 0) counts[g] = c;
  }
}

}  // namespace hmp

using namespace hmp;

extern "C" int hmp_store_count_kept(const int64_t* d_key, const int64_t* d_ptr, int32_t n_graphs, uint64_t set, int64_t* d_counts,
                                    void* stream) {
  HMP_CHECK_ARG(n_graphs >= 1 && d_ptr && d_counts, "hmp_store_count_kept: null / empty argument");
  // d_key may be null only for a store without a single row (the kernel then reads none)
  hipLaunchKernelGGL(store_count_kept_kernel, dim3(std::min(cdiv(n_graphs, 4), 1024)), dim3(256), 0, (hipStream_t)stream, d_key, d_ptr,
                     n_graphs, set, d_counts);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

extern "C" int hmp_store_derive(const int64_t* d_block, int32_t n_items, int32_t n_blocks, int32_t n_graphs, void* stream) {
  HMP_CHECK_ARG(n_items >= 0 && n_items <= HMP_SD_MAX_ITEMS, "hmp_store_derive: %d items, a launch's group table holds %d", n_items, HMP_SD_MAX_ITEMS);
  HMP_CHECK_ARG(n_blocks >= 0 && n_graphs >= 1, "hmp_store_derive: n_blocks >= 0 and n_graphs >= 1");
  if (n_items == 0 || n_blocks == 0) return HMP_OK;
  HMP_CHECK_ARG(d_block && ((uintptr_t)d_block & 15) == 0, "hmp_store_derive: the block must be a 16-byte aligned device buffer");
  hipLaunchKernelGGL(store_derive_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, d_block, n_items, n_blocks, n_graphs);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

extern "C" int hmp_store_node_split(const int8_t* d_assign, const int64_t* d_assign_off, int32_t n_graphs, const int64_t* d_ptr_a,
                                    const int64_t* d_ptr_b, const uint8_t* d_member_a, const uint8_t* d_member_b, uint8_t* d_train_a,
                                    uint8_t* d_val_a, uint8_t* d_test_a, uint8_t* d_train_b, uint8_t* d_val_b, uint8_t* d_test_b, void* stream) {
  HMP_CHECK_ARG(n_graphs >= 1 && d_assign && d_assign_off && d_ptr_a && d_train_a && d_val_a && d_test_a, "hmp_store_node_split: null / empty argument");
  HMP_CHECK_ARG((d_member_a == nullptr) == (d_member_b == nullptr), "hmp_store_node_split: the member rows come as a pair");
  HMP_CHECK_ARG(!(d_member_a && d_ptr_b), "hmp_store_node_split: ranked members live in one node set (no second part)");
  HMP_CHECK_ARG(!d_ptr_b || (d_train_b && d_val_b && d_test_b), "hmp_store_node_split: the second part has no mask rows");
  SplitArgs A;
  A.assign = d_assign; A.assign_off = d_assign_off; A.ptr_a = d_ptr_a; A.ptr_b = d_ptr_b; A.member_a = d_member_a; A.member_b = d_member_b;
  A.mask_a[0] = d_train_a; A.mask_a[1] = d_val_a; A.mask_a[2] = d_test_a;
  A.mask_b[0] = d_train_b; A.mask_b[1] = d_val_b; A.mask_b[2] = d_test_b;
  A.G = n_graphs;
  hipLaunchKernelGGL(store_node_split_kernel, dim3(cdiv(n_graphs, 4)), dim3(256), 0, (hipStream_t)stream, A);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

extern "C" int hmp_store_member_counts(const uint8_t* d_member_a, const uint8_t* d_member_b, const int64_t* d_ptr, int32_t n_graphs,
                                       int64_t* d_counts, void* stream) {
  HMP_CHECK_ARG(n_graphs >= 1 && d_member_a && d_member_b && d_ptr && d_counts, "hmp_store_member_counts: null / empty argument");
  hipLaunchKernelGGL(store_member_counts_kernel, dim3(cdiv(n_graphs, 4)), dim3(256), 0, (hipStream_t)stream, d_member_a, d_member_b, d_ptr,
                     n_graphs, d_counts);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}
