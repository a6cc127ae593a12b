// Frame pipeline, device stage -- SURVEY 8(f) row 4: ONE launch expands the staging block that frame.cpp packed into every tensor
// of the HeteroData the models read (include/hydra_mp.h section 14), where the torch path issues about a dozen small copies and as
// many cat / flip / stack / index launches (and about thirty more for an H-tree).
//
// Every output element is a function of the staging block and the resident semantic table alone: nothing the launch writes is
// read back inside it (the leaf rows of an H-tree gather from the staging sections, not from the objects' x), so workgroups
// need no ordering, no atomics and no flags.  Workgroups map to items through the prefix word of the item table (HMP_FI_BLOCK0),
// as in collate_batch_kernel; a frame is a few tens of KB, so the launch is latency bound and what counts is that it is one.
//
// A homogeneous frame (hmp_frame_build_homogeneous) is a re-addressing of the same elements: a tensor is written by one item per
// segment (a node type's rows of x, an edge type's columns of edge_index), each at its place inside the tensor, so the rule above
// holds unchanged.  FEAT and CLIQUE rows are `width` floats whatever the type's own width is (zeros behind it), EATTR segments are
// plain sub-ranges, EDGE_SEG and CONST are the two kinds it adds.
//
// A batch of frames (hmp_frame_batch_*, frame.cpp) is the same re-addressing once more, with the frame as one more segment level:
// every batched tensor is written by one item per (graph, segment), `batch` segments are CONST, offset vectors and labels I64.  Up to
// 4096 items come with a group table in front of the item table; frame_expand_batch_kernel finds its item through it and writes it
// with the code of frame_expand_kernel (frame_expand_item), so the rule above holds for both launches.
//
// Item kinds (words S0..S3 are byte offsets of sections in the staging block, -1: none):
//   FEAT    x = [pos (P0 = 3 or 0 columns) | size | table[label] (P1 columns) | zeros up to width]
//           S0 pos f64, S1 size f64, S2 label i32, S3 row index
//           (float)double for the float64 part, the float32 table row as is.  Rows of 32 floats or more: one wavefront per row,
//           8-byte lanes when the head, the table part and the row are even (306 floats = 1224 bytes: 8-byte aligned, not 16; a
//           303-float row of a relative_pos frame is 4-byte aligned: one float per lane); else one thread per element
//   POS     float32 [rows][3]                                                    S0 pos f64, S3 row index
//   I64     int64 [rows]                                                         S0 source (P0 = 4: int32, 8: int64), S3 row index
//   EDGE    int64 [2][width] from an int32 list of P1 entries, form P0           S0 list
//   EATTR   pos32[dst] - pos32[src]: both rounded to float32, one float32 subtraction   S0 list (form P0, P1 entries), S1 pos of the
//           source type, S2 pos of the destination type
//   CLIQUE  [mean float32 position of the member rooms | zeros] without its first P0 columns: summed in ascending init-edge order by
//           one thread per (clique, coordinate), divided by the count (clique_mean)   S0 ptr i32 [rows + 1], S1 members, S2 room pos f64
//   EDGE_SEG  `width` columns of an int64 [2][S1] tensor, as EDGE: row 1 lies S1 elements (the tensor's pitch) behind row 0, the
//           sources are shifted by S2 and the destinations by S3 (the row offsets of their node types)   S0 list; S1..S3 numbers
//   CONST   `rows` elements of P1 bytes, every one P0: the int64 node_type / edge_type segments and the one-byte masks
//   EATTR_HT  pos[dst] - pos[src] on an H-tree edge list (relative positions on an H-tree, HMP_FRAME_RELPOS_HTREE), one float32
//           subtraction of what the same launch writes as `pos` of the two node types.  An end is a leaf (the float64 position of its
//           scene-graph node through object_orig / room_orig), a virtual node (that position directly) or a clique, whose mean is
//           RECOMPUTED here from the ptr / members / room-position sections with clique_mean -- the clique's `pos` item may not have
//           run yet, and nothing the launch writes is read in it.  S0 list (form P0, P1 entries), S1 descriptor: per end
//           {HMP_FE_* mode, position section, index or ptr section, member section} as byte offsets from the descriptor itself
#include "common.h"

namespace hmp {

enum { EV_AS_GIVEN = 0, EV_BOTH = 1, EV_FLIP = 2, EV_VEC_ARANGE = 3, EV_ARANGE_VEC = 4 };

// (source, destination) of output column `col` of an edge list in form `variant` over the int32 list e of E entries:
// as given [2][E]; both directions [e | e.flip(0)]; flipped; (v[k], k); (k, v[k])
__device__ __forceinline__ void edge_ends(const int* __restrict__ e, int variant, int E, int col, int& s, int& d) {
  switch (variant) {
    case EV_AS_GIVEN: s = e[col]; d = e[E + col]; break;
    case EV_BOTH:
      if (col < E) { s = e[col]; d = e[E + col]; }
      else { s = e[col]; d = e[col - E]; }  // e[col] = row 1 of the list at col - E
      break;
    case EV_FLIP: s = e[E + col]; d = e[col]; break;
    case EV_VEC_ARANGE: s = e[col]; d = col; break;
    default: s = col; d = e[col]; break;
  }
}

// column c of the float64 head [pos (npos columns) | size] of source row r
__device__ __forceinline__ float feat_head(const double* __restrict__ pos, const double* __restrict__ size, int npos, int r, int c) {
  return (float)(c < npos ? pos[3 * r + c] : size[3 * r + (c - npos)]);
}

// coordinate c of clique q: the float32 positions of its member rooms summed in ascending member order, one float32 division by
// the count.  The one statement of this arithmetic: a clique's x / pos rows and every edge_attr that ends in it agree bit for bit.
__device__ __forceinline__ float clique_mean(const int* __restrict__ ptr, const int* __restrict__ mem, const double* __restrict__ rpos, int q,
                                             int c) {
  const int b = ptr[q], t = ptr[q + 1];
  float v = 0.f;
  for (int k = b; k < t; ++k) v += (float)rpos[3 * mem[k] + c];
  return v / (float)max(t - b, 1);
}

// float32 coordinate c of node i of an H-tree edge end; E = the end's HMP_FRAME_END_WORDS words of the descriptor at `desc`
__device__ __forceinline__ float tree_end_pos(const char* __restrict__ desc, const int* __restrict__ E, int i, int c) {
  const double* pos = reinterpret_cast<const double*>(desc + E[1]);
  const int* a = reinterpret_cast<const int*>(desc + E[2]);
  if (E[0] == HMP_FE_CLIQUE) return clique_mean(a, reinterpret_cast<const int*>(desc + E[3]), pos, i, c);
  return (float)pos[3 * (E[0] == HMP_FE_GATHER ? a[i] : i) + c];
}

// What a workgroup writes of its item I (the words behind the item lookup): both kernels below call it, so every kind is written once.
__device__ __forceinline__ void frame_expand_item(const char* __restrict__ stg, char* __restrict__ arena, const float* __restrict__ table,
                                                  int sem_dim, const int* __restrict__ I) {
  const int lane = threadIdx.x & 63;
  const int kind = I[HMP_FI_KIND], rows = I[HMP_FI_ROWS], width = I[HMP_FI_WIDTH];
  const int p0 = I[HMP_FI_P0], p1 = I[HMP_FI_P1];
  const int lb = (int)blockIdx.x - I[HMP_FI_BLOCK0];
  char* out = arena + I[HMP_FI_DST];
  auto sec = [&](int w) -> const char* { return I[w] >= 0 ? stg + I[w] : nullptr; };
  const int* idx = reinterpret_cast<const int*>(sec(HMP_FI_S3));
  const int64_t e = (int64_t)lb * 256 + threadIdx.x;  // element of a one-thread-per-element item

  if (kind == HMP_FK_FEAT) {
    const double* pos = reinterpret_cast<const double*>(sec(HMP_FI_S0));
    const double* size = reinterpret_cast<const double*>(sec(HMP_FI_S1));
    // the table is read only when the launch was given the table the frame was laid out for
    const int* label = p1 > 0 && p1 == sem_dim && table ? reinterpret_cast<const int*>(sec(HMP_FI_S2)) : nullptr;
    const int head = p0 + 3, own = head + p1;  // columns [own, width) of a wider destination row are zeros
    float* o = reinterpret_cast<float*>(out);
    if (width >= 32) {
      const int row = lb * 4 + (threadIdx.x >> 6);
      if (row >= rows) return;
      const int r = idx ? idx[row] : row;
      const float* trow = label ? table + (int64_t)label[r] * sem_dim : nullptr;
      float* orow = o + (int64_t)row * width;
      // a table row is read (trow) only with P1 = sem_dim, and never past column own - head = sem_dim of it
      if (((width | head | p1) & 1) == 0) {
        for (int u = lane; u < (width >> 1); u += 64) {
          const int c = 2 * u;
          float2 v = make_float2(0.f, 0.f);
          if (c < head) v = make_float2(feat_head(pos, size, p0, r, c), feat_head(pos, size, p0, r, c + 1));
          else if (trow && c < own) v = reinterpret_cast<const float2*>(trow)[(c - head) >> 1];
          reinterpret_cast<float2*>(orow)[u] = v;
        }
      } else {
        for (int c = lane; c < width; c += 64) orow[c] = c < head ? feat_head(pos, size, p0, r, c) : (trow && c < own ? trow[c - head] : 0.f);
      }
    } else if (e < (int64_t)rows * width) {
      const int row = (int)(e / width), c = (int)(e % width);
      const int r = idx ? idx[row] : row;
      o[e] = c < head ? feat_head(pos, size, p0, r, c) : (label && c < own ? table[(int64_t)label[r] * sem_dim + (c - head)] : 0.f);
    }
  } else if (kind == HMP_FK_POS) {
    if (e < (int64_t)rows * 3) {
      const int row = (int)(e / 3), c = (int)(e % 3);
      const int r = idx ? idx[row] : row;
      reinterpret_cast<float*>(out)[e] = (float)reinterpret_cast<const double*>(sec(HMP_FI_S0))[3 * r + c];
    }
  } else if (kind == HMP_FK_I64) {
    if (e < rows) {
      const int r = idx ? idx[e] : (int)e;
      const char* src = sec(HMP_FI_S0);
      reinterpret_cast<int64_t*>(out)[e] = p0 == 4 ? (int64_t)reinterpret_cast<const int*>(src)[r] : reinterpret_cast<const int64_t*>(src)[r];
    }
  } else if (kind == HMP_FK_EDGE || kind == HMP_FK_EDGE_SEG) {
    if (e < 2 * (int64_t)width) {
      const int row = e >= width ? 1 : 0, col = (int)(e - (int64_t)row * width);
      int s, d;
      edge_ends(reinterpret_cast<const int*>(sec(HMP_FI_S0)), p0, p1, col, s, d);
      // a segment's row 1 lies one pitch of the whole tensor behind its row 0, and its ends count rows of the concatenated x
      const bool seg = kind == HMP_FK_EDGE_SEG;
      const int64_t pitch = seg ? I[HMP_FI_S1] : width;
      const int shift = seg ? I[row ? HMP_FI_S3 : HMP_FI_S2] : 0;
      reinterpret_cast<int64_t*>(out)[row * pitch + col] = (int64_t)(row ? d : s) + shift;
    }
  } else if (kind == HMP_FK_EATTR) {
    if (e < (int64_t)rows * 3) {
      const int col = (int)(e / 3), c = (int)(e % 3);
      int s, d;
      edge_ends(reinterpret_cast<const int*>(sec(HMP_FI_S0)), p0, p1, col, s, d);
      const float ps = (float)reinterpret_cast<const double*>(sec(HMP_FI_S1))[3 * s + c];
      const float pd = (float)reinterpret_cast<const double*>(sec(HMP_FI_S2))[3 * d + c];
      reinterpret_cast<float*>(out)[e] = pd - ps;
    }
  } else if (kind == HMP_FK_CLIQUE) {
    if (e < (int64_t)rows * width) {
      const int q = (int)(e / width), c = (int)(e % width);
      float v = 0.f;
      if (c + p0 < 3)
        v = clique_mean(reinterpret_cast<const int*>(sec(HMP_FI_S0)), reinterpret_cast<const int*>(sec(HMP_FI_S1)),
                        reinterpret_cast<const double*>(sec(HMP_FI_S2)), q, c + p0);
      reinterpret_cast<float*>(out)[e] = v;
    }
  } else if (kind == HMP_FK_EATTR_HT) {
    if (e < (int64_t)rows * 3) {
      const int col = (int)(e / 3), c = (int)(e % 3);
      int s, d;
      edge_ends(reinterpret_cast<const int*>(sec(HMP_FI_S0)), p0, p1, col, s, d);
      const char* desc = sec(HMP_FI_S1);
      const int* E = reinterpret_cast<const int*>(desc);
      const float ps = tree_end_pos(desc, E, s, c);
      const float pd = tree_end_pos(desc, E + HMP_FRAME_END_WORDS, d, c);
      reinterpret_cast<float*>(out)[e] = pd - ps;
    }
  } else if (kind == HMP_FK_CONST) {
    if (e < rows) {
      if (p1 == 8) reinterpret_cast<int64_t*>(out)[e] = p0;
      else reinterpret_cast<unsigned char*>(out)[e] = (unsigned char)p0;
    }
  }
}

__global__ __launch_bounds__(256) void frame_expand_kernel(const char* __restrict__ stg, char* __restrict__ arena,
                                                           const float* __restrict__ table, int sem_dim, int n_items) {
  const int lane = threadIdx.x & 63;
  const int* items = reinterpret_cast<const int*>(stg);
  // the item of this workgroup: the last one whose first workgroup is not behind it (empty items share their successor's word)
  const int b0 = lane < n_items ? items[lane * HMP_FRAME_ITEM_WORDS + HMP_FI_BLOCK0] : 0x7fffffff;
  const int ii = __popcll(__ballot(b0 <= (int)blockIdx.x)) - 1;
  if (ii < 0) return;
  frame_expand_item(stg, arena, table, sem_dim, items + ii * HMP_FRAME_ITEM_WORDS);
}

// A batch block (hmp_frame_batch_pack): [group table | item table | sections], up to 64 groups of 64 items.  The same rule picks
// the group and then the item inside it -- the last one whose first workgroup is not behind this one -- with one 64-lane load and
// one ballot each: the table's prefix words never decrease, so the last such item lies in the last such group.  Both results are
// wave-uniform; lanes past the tables read INT_MAX.
__global__ __launch_bounds__(256) void frame_expand_batch_kernel(const char* __restrict__ stg, char* __restrict__ arena,
                                                                 const float* __restrict__ table, int sem_dim, int n_items) {
  const int lane = threadIdx.x & 63;
  const int n_groups = (n_items + HMP_FRAME_MAX_ITEMS - 1) / HMP_FRAME_MAX_ITEMS;
  const int* groups = reinterpret_cast<const int*>(stg);
  const int* items = reinterpret_cast<const int*>(stg + ((n_groups * 4 + 15) & ~15));
  const int g0 = lane < n_groups ? groups[lane] : 0x7fffffff;
  const int gi = __popcll(__ballot(g0 <= (int)blockIdx.x)) - 1;
  if (gi < 0) return;
  const int it = gi * HMP_FRAME_MAX_ITEMS + lane;
  const int b0 = it < n_items ? items[it * HMP_FRAME_ITEM_WORDS + HMP_FI_BLOCK0] : 0x7fffffff;
  const int ii = gi * HMP_FRAME_MAX_ITEMS + __popcll(__ballot(b0 <= (int)blockIdx.x)) - 1;
  frame_expand_item(stg, arena, table, sem_dim, items + ii * HMP_FRAME_ITEM_WORDS);
}

}  // namespace hmp

using namespace hmp;

extern "C" int hmp_frame_expand(const void* d_staging, void* d_arena, const float* d_sem_table, int32_t sem_dim, int32_t n_items,
                                int32_t n_blocks, void* stream) {
  HMP_CHECK_ARG(d_staging && d_arena && (((uintptr_t)d_staging | (uintptr_t)d_arena) & 15) == 0,
                "hmp_frame_expand: the staging block and the arena must be 16-byte aligned device buffers");
  HMP_CHECK_ARG(n_items >= 1 && n_items <= HMP_FRAME_MAX_ITEMS && n_blocks >= 1, "hmp_frame_expand: n_items in [1, %d] and n_blocks >= 1 (hmp_frame_sizes)",
                HMP_FRAME_MAX_ITEMS);
  HMP_CHECK_ARG(sem_dim >= 0 && (sem_dim == 0 || (d_sem_table && ((uintptr_t)d_sem_table & 7) == 0)),
                "hmp_frame_expand: sem_dim > 0 needs the resident float32 table, 8-byte aligned");
  hipLaunchKernelGGL(frame_expand_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, (const char*)d_staging, (char*)d_arena,
                     d_sem_table, sem_dim, n_items);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

extern "C" int hmp_frame_expand_batch(const void* d_staging, void* d_arena, const float* d_sem_table, int32_t sem_dim, int32_t n_items,
                                      int32_t n_blocks, void* stream) {
  HMP_CHECK_ARG(d_staging && d_arena && (((uintptr_t)d_staging | (uintptr_t)d_arena) & 15) == 0,
                "hmp_frame_expand_batch: the staging block and the arena must be 16-byte aligned device buffers");
  HMP_CHECK_ARG(n_items >= 1 && n_items <= HMP_FRAME_BATCH_MAX_ITEMS && n_blocks >= 1,
                "hmp_frame_expand_batch: n_items in [1, %d] and n_blocks >= 1 (hmp_frame_batch_sizes)", HMP_FRAME_BATCH_MAX_ITEMS);
  HMP_CHECK_ARG(sem_dim >= 0 && (sem_dim == 0 || (d_sem_table && ((uintptr_t)d_sem_table & 7) == 0)),
                "hmp_frame_expand_batch: sem_dim > 0 needs the resident float32 table, 8-byte aligned");
  hipLaunchKernelGGL(frame_expand_batch_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, (const char*)d_staging, (char*)d_arena,
                     d_sem_table, sem_dim, n_items);
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}
