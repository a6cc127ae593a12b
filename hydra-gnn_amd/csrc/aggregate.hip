// K1 -- CSR gather / segment reduce, and the fused per-layer SAGE aggregation built on it.
//
// Work decomposition: one ROW GROUP of GS lanes per destination row (GS = 8/16/32/64, chosen from the
// row width so that each lane owns one float4 of the row; several rows share a wavefront when rows are
// narrower than 256 floats).  A group walks its CSR segment four neighbours at a time: the neighbour
// ids are read with one group-uniform load each, the four source rows are fetched as independent
// 16-byte-per-lane loads (GS*16 contiguous bytes per row: one fully coalesced request), then added in
// edge order, so the sum has the same association as a sequential scatter_add over the edge list.
// No atomics anywhere: the backward pass gathers over the transposed lists (CSC) instead of scattering.
//
// HBM/L2 traffic per row: deg * F * 4 bytes of source rows + 4*deg + 8 bytes of indices + F*4 out.
#include <type_traits>

#include "tail_fns.h"

namespace hmp {

KT_DEFINE(agg)
KT_BLOCKS_DEFINE(agg)

__device__ __forceinline__ int cdiv_dev(int a, int b) { return (a + b - 1) / b; }

// raw buffer descriptor over [base, base + bytes): loads past the end return 0 without touching memory
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

// ----- row access helpers -----------------------------------------------------------------------
// VEC = 4: 16-byte accesses (pointer and ld 16-byte aligned); VEC = 1: scalar fall-back for arbitrary ld.
template <int VEC>
struct Acc;
template <>
struct Acc<4> {
  float4 v;
  __device__ __forceinline__ void zero() { v = make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = v; }
  __device__ __forceinline__ void add(const Acc& o) { v.x += o.v.x; v.y += o.v.y; v.z += o.v.z; v.w += o.v.w; }
  // mean of a segment: sum * (1 / deg), the reciprocal computed ONCE (an IEEE division; wave-uniform where the row is) and applied
  // by explicit fused multiply-adds -- the same form in every kernel, so all of them stay bit-identical to each other (the
  // backward pass multiplies by the same reciprocal: hmp plan's degf).  x / deg per element cost 4 divisions per lane and edge type.
  __device__ __forceinline__ void add_div(const Acc& o, float d) {
    const float r = 1.0f / d;
    v.x = fmaf(o.v.x, r, v.x); v.y = fmaf(o.v.y, r, v.y); v.z = fmaf(o.v.z, r, v.z); v.w = fmaf(o.v.w, r, v.w);
  }
  // explicit fused multiply-adds (two v_pk_fma_f32): left to the compiler, an 8-edge batch became 2 packed multiplies + 2 packed adds per
  // edge and a 2-edge batch 2 packed fmas -- a third more vector instructions, and a rounding that depended on the batch shape
  __device__ __forceinline__ void add_mul(const Acc& o, float r) {
    v.x = fmaf(o.v.x, r, v.x); v.y = fmaf(o.v.y, r, v.y); v.z = fmaf(o.v.z, r, v.z); v.w = fmaf(o.v.w, r, v.w);
  }
  __device__ __forceinline__ void div(float d) { v.x /= d; v.y /= d; v.z /= d; v.w /= d; }
  __device__ __forceinline__ float& at(int i) { return (&v.x)[i]; }
};
template <>
struct Acc<1> {
  float v;
  __device__ __forceinline__ void zero() { v = 0.f; }
  __device__ __forceinline__ void load(const float* p) { v = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v; }
  __device__ __forceinline__ void add(const Acc& o) { v += o.v; }
  __device__ __forceinline__ void add_div(const Acc& o, float d) { v = fmaf(o.v, 1.0f / d, v); }
  __device__ __forceinline__ void add_mul(const Acc& o, float r) { v = fmaf(o.v, r, v); }
  __device__ __forceinline__ void div(float d) { v /= d; }
  __device__ __forceinline__ float& at(int) { return v; }
};

// Projected rows stored as bf16 (bf16 compute mode at 10^6 rows: halves the projection's write and the gather's read traffic):
// ZB = true reads 4 bf16 (8 bytes) at ELEMENT index `idx` of the buffer and widens them; the buffer is typed float* like the
// fp32 one, offsets and leading dimensions count elements either way.
template <bool ZB>
__device__ __forceinline__ void load_z(Acc<4>& a, const float* base, int64_t idx) {
  if constexpr (ZB) {
    const uint2 b = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(base) + idx);
    a.v = make_float4(__uint_as_float(b.x << 16), __uint_as_float(b.x & 0xffff0000u), __uint_as_float(b.y << 16),
                      __uint_as_float(b.y & 0xffff0000u));
  } else {
    a.load(base + idx);
  }
}

// counterpart for buffers WRITTEN as bf16 (round to nearest even): 4 elements at element index `idx`
template <bool ZB>
__device__ __forceinline__ void store_z(const Acc<4>& a, float* base, int64_t idx) {
  if constexpr (ZB) {
    typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
    bf4 b;
    b[0] = (__bf16)a.v.x; b[1] = (__bf16)a.v.y; b[2] = (__bf16)a.v.z; b[3] = (__bf16)a.v.w;
    *reinterpret_cast<bf4*>(reinterpret_cast<uint16_t*>(base) + idx) = b;
  } else {
    a.store(base + idx);
  }
}

// Per-edge weight of a gather, a compile-time policy.  NoW: none -- plain adds.  MeanW: the backward of the mean, every edge carries
// 1 / max(deg(dst), 1).  `degf` (the reciprocal per destination, written by the plan) removes the two dependent rowptr loads per
// edge AND the per-edge fp32 divisions (4 per lane and edge: ~1 ms of the config-5 transposed aggregation); without it (unit entry
// point, unit-test path) the reciprocal is derived from rowptr.  Table or derived, and mean = 0 (a plain sum after all), are
// launch-uniform run-time cases of the one policy: the kernels are not instantiated per case.
struct NoW {
  static constexpr bool weighted = false;
};
struct MeanW {
  static constexpr bool weighted = true;
  const int* rowptr;
  const float* degf;
  int mean;
  __device__ __forceinline__ float derived(int i) const {
    const int deg = rowptr[i + 1] - rowptr[i];
    return 1.f / (float)(deg > 1 ? deg : 1);
  }
};

// sum_{k in [b,e)} w(col[k]) * x[col[k]][c .. c+VEC)   in edge order; NV column chunks per lane (stride GS*VEC).
// Neighbours are processed in batches of UB = 8 (4 for wide rows) with NO tail loop: ids beyond the row are clamped to the
// last valid entry (same address => cache hit) and masked at the add.  A row of degree <= 8 therefore costs three
// dependent memory round trips (extent, ids, rows) instead of one per tail neighbour.
template <int GS, int NV, int VEC, bool ZB = false, class W = NoW>
__device__ __forceinline__ void gather_sum(Acc<VEC> (&acc)[NV], const float* __restrict__ x, int ld, const int* __restrict__ col,
                                           int b, int e, int c0, int F, const W w = W()) {
  constexpr int UB = (NV == 1) ? 8 : 4;
  for (int k = b; k < e; k += UB) {
    int j[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) j[u] = col[min(k + u, e - 1)];
    [[maybe_unused]] float d[UB];
    if constexpr (W::weighted) {
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        d[u] = 1.f;
        if (w.mean) d[u] = w.degf ? w.degf[j[u]] : w.derived(j[u]);
      }
    }
    Acc<VEC> v[UB][NV];
#pragma unroll
    for (int u = 0; u < UB; ++u)
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const int c = c0 + q * GS * VEC;
        if (c < F) {
          if constexpr (ZB && VEC == 4) load_z<true>(v[u][q], x, (int64_t)j[u] * ld + c);
          else v[u][q].load(x + (int64_t)j[u] * ld + c);
        }
      }
    const int cnt = e - k;
#pragma unroll
    for (int u = 0; u < UB; ++u)
      if (u < cnt) {
#pragma unroll
        for (int q = 0; q < NV; ++q) {
          const int c = c0 + q * GS * VEC;
          if (c < F) {
            if constexpr (W::weighted) {
              if (w.mean) acc[q].add_mul(v[u][q], d[u]); else acc[q].add(v[u][q]);
            } else {
              acc[q].add(v[u][q]);
            }
          }
        }
      }
  }
}

// One side of a paired gather: rows x[col[k]] (pitch ld, in elements; a column offset is part of x), k in [b, e), the lane's
// 4 columns valid while c0 < F.
struct GatherSide {
  const float* x;
  int ld;
  const int* col;
  int b, e, F;
};

// Two edge types at a time: the neighbour ids of both types travel together, then the 16 neighbour rows -- three dependent
// round trips (extents, ids, rows) for two edge types instead of five.  A missing partner aliases the first type with an
// empty extent (loads hit the same lines, adds are masked).  a0 / a1 = the two sums, each in the edge order of its type.
// ZB: the rows hold bf16 elements (load_z).  kt: this call stamps the KTIME phases 5 (ids here) and 6 (first rows here).
template <int GS, bool ZB, class W>
__device__ __forceinline__ void gather_pair(const GatherSide& s0, const GatherSide& s1, const W& w0, const W& w1, int c0,
                                            Acc<4> (&a0)[1], Acc<4> (&a1)[1], [[maybe_unused]] bool kt) {
  constexpr int UB = 8;
  const int b0 = s0.b, e0 = s0.e, b1 = s1.b, e1 = s1.e;
  // GS <= 16 (rows of <= 64 floats, the MP3D hidden width): ids of neighbours 0..7 AND 8..15 of both types in the same round
  // trip -- a row of 9..16 neighbours (most 16-row blocks of a scene-graph batch hold one) then needs one more round trip
  // for its second batch of rows instead of two.  Wider rows keep the plain tail: the 16 extra registers cost them a wave
  // per SIMD (config 4: 0.140 -> 0.151 ms).
  constexpr bool PRE = GS <= 16;
  int j0[UB], j1[UB], j0t[PRE ? UB : 1], j1t[PRE ? UB : 1];
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    j0[u] = s0.col[e0 > b0 ? min(b0 + u, e0 - 1) : 0];
    j1[u] = s1.col[e1 > b1 ? min(b1 + u, e1 - 1) : 0];
    if constexpr (PRE) {
      j0t[u] = s0.col[e0 > b0 ? min(b0 + UB + u, e0 - 1) : 0];
      j1t[u] = s1.col[e1 > b1 ? min(b1 + UB + u, e1 - 1) : 0];
    }
  }
  [[maybe_unused]] float d0[UB], d1[UB];
  Acc<4> v0[UB], v1[UB];
  const int cc0 = c0 < s0.F ? c0 : 0, cc1 = c0 < s1.F ? c0 : 0;
  [[maybe_unused]] bool mean = false, dg = false;  // block-uniform
  if constexpr (W::weighted) {
    mean = w0.mean;
    dg = mean && w0.degf && w1.degf;
  }
  a0[0].zero();
  a1[0].zero();
  // 8 rows of each side at ids i0 / i1 (edges off .. off + 7 of the extents), through the same registers every time
  auto batch = [&](const int (&i0)[UB], const int (&i1)[UB], int off, [[maybe_unused]] bool stamp) {
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      if constexpr (W::weighted) {
        d0[u] = dg ? w0.degf[i0[u]] : 1.f;
        d1[u] = dg ? w1.degf[i1[u]] : 1.f;
      }
      load_z<ZB>(v0[u], s0.x, (int64_t)i0[u] * s0.ld + cc0);
      load_z<ZB>(v1[u], s1.x, (int64_t)i1[u] * s1.ld + cc1);
    }
    if (stamp) KTW(6);
    if constexpr (W::weighted) {
      if (mean && !dg) {
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          d0[u] = w0.derived(i0[u]);
          d1[u] = w1.derived(i1[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UB; ++u)
      if (b0 + off + u < e0) {
        if constexpr (W::weighted) a0[0].add_mul(v0[u], d0[u]); else a0[0].add(v0[u]);
      }
#pragma unroll
    for (int u = 0; u < UB; ++u)
      if (b1 + off + u < e1) {
        if constexpr (W::weighted) a1[0].add_mul(v1[u], d1[u]); else a1[0].add(v1[u]);
      }
  };
  if (kt) KTW(5);
  batch(j0, j1, 0, kt);
  int done = UB;
  if constexpr (PRE) {
    if (e0 - b0 > UB || e1 - b1 > UB) batch(j0t, j1t, UB, false);  // second batch (ids already here)
    done = 2 * UB;
  }
  if (e0 - b0 > done) gather_sum<GS, 1, 4, ZB, W>(a0, s0.x, s0.ld, s0.col, b0 + done, e0, c0, s0.F, w0);
  if (e1 - b1 > done) gather_sum<GS, 1, 4, ZB, W>(a1, s1.x, s1.ld, s1.col, b1 + done, e1, c0, s1.F, w1);
}

// ----- K1 unit kernels ----------------------------------------------------------------------------
template <int GS, int NV, int VEC>
__global__ __launch_bounds__(256) void segment_mean_fwd_kernel(const float* __restrict__ x, int ldx, int F, const int* __restrict__ rowptr,
                                                               const int* __restrict__ col, int n_rows, float* __restrict__ out, int ldo) {
  const int rpb = 256 / GS;
  const int row = blockIdx.x * rpb + threadIdx.x / GS;
  if (row >= n_rows) return;
  const int c0 = (threadIdx.x % GS) * VEC;
  Acc<VEC> acc[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) acc[q].zero();
  const int b = rowptr[row], e = rowptr[row + 1];
  gather_sum<GS, NV, VEC>(acc, x, ldx, col, b, e, c0, F);
  const float d = (float)((e - b) > 1 ? (e - b) : 1);
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int c = c0 + q * GS * VEC;
    if (c < F) { acc[q].div(d); acc[q].store(out + (int64_t)row * ldo + c); }
  }
}

template <int GS, int NV, int VEC>
__global__ __launch_bounds__(256) void segment_mean_bwd_kernel(const float* __restrict__ g, int ldg, int F, const int* __restrict__ t_rowptr,
                                                               const int* __restrict__ t_col, const int* __restrict__ rowptr, int n_rows,
                                                               float* __restrict__ gx, int ldgx) {
  const int rpb = 256 / GS;
  const int row = blockIdx.x * rpb + threadIdx.x / GS;
  if (row >= n_rows) return;
  const int c0 = (threadIdx.x % GS) * VEC;
  Acc<VEC> acc[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) acc[q].zero();
  gather_sum<GS, NV, VEC, false, MeanW>(acc, g, ldg, t_col, t_rowptr[row], t_rowptr[row + 1], c0, F, MeanW{rowptr, nullptr, 1});
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int c = c0 + q * GS * VEC;
    if (c < F) acc[q].store(gx + (int64_t)row * ldgx + c);
  }
}

// ----- fused SAGE layer aggregation -----------------------------------------------------------------
// t = dropout(act(t)) for the lane's columns [c, c + 4) of row `row` of entry D (dcfg: D.drop with the step resolved); keep-mask
// quad row * (ldo / 4) + c / 4
__device__ __forceinline__ void agg_act_drop4(const AggDst& D, const DropCfg& dcfg, int row, int c, Acc<4>& t) {
  bool keep[4] = {true, true, true, true};
  if (D.drop_on) drop_keep4(dcfg, (uint32_t)row * (uint32_t)(D.ldo >> 2) + (uint32_t)(c >> 2), keep);
  act_drop4(&t.at(0), D.act, D.drop_on != 0, keep, D.drop.scale);
}

// out[t][i] = dropout(act( zroot[i] + bias + sum_e mean_{k in N_e(i)} z_e[col_k] ))   (one row group, result also in `tot`)
template <int GS, int NV, bool ZB = false, bool HB = false>
__device__ __forceinline__ void agg_row(const AggDst& D, int mean, int row, int c0, Acc<4> (&tot)[NV]) {
  constexpr int VEC = 4;
  // Everything whose address depends on the row alone is requested here, and nothing of it is consumed before the gathers
  // (a use inside one of these branches would put an s_waitcnt in it): the device step counter of the dropout coordinates, the
  // root row and the bias, the row extents of every incoming edge type -- ONE round trip.
  KT(3);
  DropCfg dcfg = D.drop;
  uint32_t step_add = 0;
  if (D.drop_on) step_add = drop_step_vload(D.drop.step_dev);
  Acc<VEC> bs[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int c = c0 + q * GS * VEC;
    tot[q].zero();
    bs[q].zero();
    if (c < D.F) {
      if (D.zroot) load_z<ZB>(tot[q], D.zroot, (int64_t)row * D.ldzr + D.roff + c);
      if (D.bias) bs[q].load(D.bias + c);
    }
  }
  int rb[AGG_MAX_IN], re[AGG_MAX_IN];
#pragma unroll
  for (int ii = 0; ii < AGG_MAX_IN; ++ii) {
    rb[ii] = re[ii] = 0;
    if (ii < D.n_in) { rb[ii] = D.in[ii].rowptr[row]; re[ii] = D.in[ii].rowptr[row + 1]; }
  }
  KTW(4);
#pragma unroll
  for (int q = 0; q < NV; ++q) tot[q].add(bs[q]);  // (root + bias) first, as the sequential code
  if constexpr (NV == 1 && GS == 64) {
    // One wavefront per row (the caller made `row` wave-uniform): the neighbour ids of BOTH edge types of a pair are scalar
    // loads issued together, then 16 rows of the first type in flight, then 16 of the second through the same registers --
    // extents, ids, rows, rows: 4 dependent round trips for in-degrees <= 16 (the 8 + 8 pair batch needed a tail pass from 9
    // neighbours on) and no clamped duplicate loads for the short list of a pair (rooms -> objects: one neighbour).
    constexpr int UB = 16;
    const bool cin = c0 < D.F;
    const int cc = cin ? c0 : 0;
#pragma unroll
    for (int ii = 0; ii < AGG_MAX_IN; ii += 2) {
      if (ii >= D.n_in) break;
      const bool has2 = ii + 1 < D.n_in;
      const AggIn& I0 = D.in[ii];
      const AggIn& I1 = D.in[has2 ? ii + 1 : ii];
      const int b0 = rb[ii], e0 = re[ii];
      const int b1 = has2 ? rb[ii + 1] : b0, e1 = has2 ? re[ii + 1] : b0;
      int j0[UB], j1[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        j0[u] = I0.col[e0 > b0 ? min(b0 + u, e0 - 1) : 0];
        j1[u] = I1.col[e1 > b1 ? min(b1 + u, e1 - 1) : 0];
      }
      Acc<VEC> v[UB], a0[1], a1[1];
      a0[0].zero();
      a1[0].zero();
      if (e0 > b0) {  // wave-uniform
#pragma unroll
        for (int u = 0; u < UB; ++u) load_z<ZB>(v[u], I0.z, I0.coff + (int64_t)j0[u] * I0.ldz + cc);
#pragma unroll
        for (int u = 0; u < UB; ++u)
          if (b0 + u < e0) a0[0].add(v[u]);
      }
      if (e1 > b1) {
#pragma unroll
        for (int u = 0; u < UB; ++u) load_z<ZB>(v[u], I1.z, I1.coff + (int64_t)j1[u] * I1.ldz + cc);
#pragma unroll
        for (int u = 0; u < UB; ++u)
          if (b1 + u < e1) a1[0].add(v[u]);
      }
      // (ZB: the column offset goes into the element index, the base pointer stays the buffer start)
      if (e0 - b0 > UB) gather_sum<GS, 1, VEC, ZB>(a0, ZB ? I0.z : I0.z + I0.coff, I0.ldz, I0.col, b0 + UB, e0, ZB ? c0 + I0.coff : c0, ZB ? D.F + I0.coff : D.F);
      if (e1 - b1 > UB) gather_sum<GS, 1, VEC, ZB>(a1, ZB ? I1.z : I1.z + I1.coff, I1.ldz, I1.col, b1 + UB, e1, ZB ? c0 + I1.coff : c0, ZB ? D.F + I1.coff : D.F);
      if (cin) {
        if (e0 > b0) tot[0].add_div(a0[0], mean ? (float)(e0 - b0) : 1.f);
        if (e1 > b1) tot[0].add_div(a1[0], mean ? (float)(e1 - b1) : 1.f);
      }
    }
  } else if constexpr (NV == 1) {
    // incoming edge types in PAIRS (gather_pair); sums keep the edge order per type and the type order of the sequential code
    static_assert(!ZB, "bf16 rows take their column offset in the element index: the one-wavefront shape only");
#pragma unroll
    for (int ii = 0; ii < AGG_MAX_IN; ii += 2) {
      if (ii >= D.n_in) break;
      const bool has2 = ii + 1 < D.n_in;
      const AggIn& I0 = D.in[ii];
      const AggIn& I1 = D.in[has2 ? ii + 1 : ii];
      const int b0 = rb[ii], e0 = re[ii];
      const int b1 = has2 ? rb[ii + 1] : b0, e1 = has2 ? re[ii + 1] : b0;
      Acc<VEC> a0[1], a1[1];
      gather_pair<GS, false>(GatherSide{I0.z + I0.coff, I0.ldz, I0.col, b0, e0, D.F}, GatherSide{I1.z + I1.coff, I1.ldz, I1.col, b1, e1, D.F},
                             NoW(), NoW(), c0, a0, a1, ii == 0);
      if (c0 < D.F) {
        if (e0 > b0) tot[0].add_div(a0[0], mean ? (float)(e0 - b0) : 1.f);
        if (e1 > b1) tot[0].add_div(a1[0], mean ? (float)(e1 - b1) : 1.f);
      }
    }
  } else {
#pragma unroll
  for (int ii = 0; ii < AGG_MAX_IN; ++ii) {
    if (ii >= D.n_in) break;
    const AggIn& I = D.in[ii];
    const int b = rb[ii], e = re[ii];
    if (e == b) continue;
    Acc<VEC> acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[q].zero();
    gather_sum<GS, NV, VEC>(acc, I.z + I.coff, I.ldz, I.col, b, e, c0, D.F);
    const float d = mean ? (float)(e - b) : 1.f;
#pragma unroll
    for (int q = 0; q < NV; ++q) tot[q].add_div(acc[q], d);
  }
  }
  KTW(7);
  dcfg.step += step_add;
  dcfg.step_dev = nullptr;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int c = c0 + q * GS * VEC;
    if (c >= D.F) continue;
    agg_act_drop4(D, dcfg, row, c, tot[q]);
    if constexpr (HB && VEC == 4) store_z<true>(tot[q], D.out, (int64_t)row * D.ldo + c);
    else tot[q].store(D.out + (int64_t)row * D.ldo + c);
  }
}

// Masked cross entropy of the output row its row group has just computed (lane = 4 consecutive logits in `t`): ce_group over
// the registers, the gradient chained back to z where the CE read y = dropout(act(z)).
template <int GS>
__device__ __forceinline__ void ce_rowgroup(const AggDst& D, NetState* state, int row, int c0, Acc<4>& t, int64_t y, bool in_mask,
                                            float wy) {
  ce_group<GS, 1>(
      c0 >> 2, D.ce_classes, D.ce_ldg, y, D.ce_ignored, in_mask,
      [&](int, int, float (&v)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = t.at(i);
      },
      [&](int c, float (&g)[4], const float (&)[4]) {
        if (D.ce_tail) {  // act' from y, as the hidden layers' backward does
#pragma unroll
          for (int i = 0; i < 4; ++i) g[i] *= tail_dydz(t.at(i), D.act, D.drop_on != 0, D.drop.scale);
        }
        *reinterpret_cast<float4*>(D.ce_grad + (int64_t)row * D.ce_ldg + c) = make_float4(g[0], g[1], g[2], g[3]);
      },
      D.ce_row_lv, row, state, D.ce_weight, wy);
}

template <int GS, int NV, bool ZB = false, bool HB = false>
__global__ __launch_bounds__(256) void agg_fwd_kernel(const AggArgs a) {
  int ti = 0;
  while (ti + 1 < a.n && (int)blockIdx.x >= a.bstart[ti + 1]) ++ti;
  karg_warm<9>((int)offsetof(AggArgs, d) + ti * (int)sizeof(AggDst), (int)sizeof(AggDst));
  const AggDst& D = a.d[ti];
  // rows per workgroup: 256 / GS, or 8 for an entry of heavy rows in a small launch (AggDst::tile_rows; the other row groups idle)
  const int rpb = (D.tile_rows == 8 && 256 / GS > 8) ? 8 : 256 / GS;
  int local = blockIdx.x - D.block_start;
  // workgroups go to the 8 XCDs round robin by block id: give XCD x the x-th contiguous eighth of the rows, so that the
  // neighbour rows a run of consecutive destinations shares (scene graphs: the same room) are fetched into ONE L2, not 8
  if (a.xcd) local = (local & 7) * ((cdiv_dev(D.n_rows, rpb) + 7) >> 3) + (local >> 3);
  if ((int)threadIdx.x / GS >= rpb) return;
  int row = local * rpb + threadIdx.x / GS;
  // GS = 64: the wavefront IS the row group, so the row (and with it every extent / neighbour id) is wave-uniform; saying so
  // moves those loads and the address arithmetic to the scalar unit
  if (GS == 64) row = __builtin_amdgcn_readfirstlane(row);
  if (row >= D.n_rows) return;
  Acc<4> tot[NV];
  const int c0 = (threadIdx.x % GS) * 4;
  // the label is requested before the aggregation (it depends on nothing): one round trip less behind the last gather; so is
  // its class weight, as soon as the label is there (weighted steps only: an unweighted launch issues no load for it)
  int64_t y = 0;
  bool in_mask = true;
  float wy = 1.f;
  if (NV == 1 && D.ce_labels) {
    y = D.ce_labels[row];
    if (D.ce_mask) in_mask = D.ce_mask[row] != 0;
    if (D.ce_weight) wy = ce_weight(D.ce_weight, y, D.ce_classes);
  }
  agg_row<GS, NV, ZB, HB>(D, a.mean, row, c0, tot);
  if constexpr (NV == 1) {
    if (D.ce_labels) ce_rowgroup<GS>(D, a.state, row, c0, tot[0], y, in_mask, wy);
  }
}

// ----- aggregation of layer l FUSED with the projection of layer l+1 --------------------------------------------
// The projection Z[l+1][t] = H[l+1][t] * Wp[l+1][t]^T is row-local, so the block that has just aggregated 16 rows of
// H[l+1][t] keeps them in LDS ([k][row] image, LD 17) and multiplies them on the matrix cores right away
// (v_mfma_f32_16x16x4_f32: 16 rows x 16 packed columns per accumulator, exact fp32).  One kernel (and one ~4 us launch
// floor, one cross-XCD hand-off of H) less per layer; H is still written to HBM for the backward pass.
// Wp is read straight from L2 (it is <= 200 KB and shared by every block): lane (n, kq) loads 16 bytes
// Wp[n0 + n][16 i + 4 kq .. +3] and feeds 4 MFMAs with them; the k order inside a 16-block is permuted identically
// for both operands (k = 16 i + 4 kq + u at step u), which a sum over k does not care about.
typedef float f32x4 __attribute__((ext_vector_type(4)));

// (32-row tiles -- half the per-row weight traffic, two MFMA row halves sharing each B load -- were measured SLOWER on the
// H-tree config 4: 0.585 against 0.474 ms/step; half as many blocks, twice the gather passes per block.)
// one 16-row tile [row0, row0 + 16) of destination entry D, rows below row_end, by the workgroup's 256 threads; LDS image Hs [256][17]
template <int GS>
__device__ __forceinline__ void agg_proj_tile(const AggArgs& a, const AggDst& D, int row0, int row_end, float* Hs) {
  constexpr int TM = 16, LDH = 17;
  constexpr int RPP = 256 / GS;            // rows aggregated per pass
  constexpr int NP = TM / RPP;             // passes (GS = 16: 1, 32: 2, 64: 4)
  const int tid = threadIdx.x & 255;
  const int c0 = (tid % GS) * 4;
  const int lane = threadIdx.x & 63, w = tid >> 6;
  const int n = lane & 15, kq = lane >> 4;
  KT(0);
  // The weights of the projection do not depend on the aggregation: request the first PT column tiles of this wave (first
  // 64-deep k trip each) BEFORE the gather, so their round trip (every block pulls the whole Wp through its CU, ~25 GB/s)
  // overlaps the three round trips of the gather instead of following them.
  constexpr int PT = 3;
  float4 pre[PT][4];
  const int n_ct = D.pw ? (D.pncols + 15) >> 4 : 0;
  if (D.pw) {  // block-uniform
#pragma unroll
    for (int it = 0; it < PT; ++it) {
      const int col = min((w + 4 * it) * 16 + n, D.pncols - 1);  // clamped: tiles past n_ct are never used
      const float* wrow = D.pw + (int64_t)col * D.pldw;
#pragma unroll
      for (int u = 0; u < 4; ++u) pre[it][u] = *reinterpret_cast<const float4*>(wrow + min(16 * u, D.pK - 16) + 4 * kq);
    }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int m = p * RPP + tid / GS;
    const int row = row0 + m;
    Acc<4> tot[1];
    tot[0].zero();
    if (row < row_end) agg_row<GS, 1>(D, a.mean, row, c0, tot);
    if (c0 < D.pK) {
#pragma unroll
      for (int i = 0; i < 4; ++i) Hs[(c0 + i) * LDH + m] = (c0 < D.F && row < row_end) ? tot[0].at(i) : 0.f;
    }
  }
  __syncthreads();
  if (D.pw == nullptr) return;  // block-uniform: this node type is not read by the next layer
  KT(1);
  // one 16-column tile: bv0 = prefetched weights of the first k trip (null: load them here)
  auto tile = [&](int ct, const float4* bv0) {
    const int col = ct * 16 + n;
    const float* wrow = D.pw + (int64_t)min(col, D.pncols - 1) * D.pldw;  // clamped: padded columns are never stored
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // 4 k-blocks of 16 per trip: the 4 (clamped) 16-byte weight loads are in flight together, then 16 MFMAs
    for (int kb = 0; kb < D.pK; kb += 64) {
      float4 bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        bv[u] = (bv0 && kb == 0) ? bv0[u] : *reinterpret_cast<const float4*>(wrow + min(kb + 16 * u, D.pK - 16) + 4 * kq);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (kb + 16 * u >= D.pK) break;
        const float* hp = Hs + (kb + 16 * u + 4 * kq) * LDH + n;  // A operand: row m = lane & 15 of the tile
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hp[0 * LDH], bv[u].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hp[1 * LDH], bv[u].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hp[2 * LDH], bv[u].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hp[3 * LDH], bv[u].w, acc, 0, 0, 0);
      }
    }
    // D layout: column = lane & 15, row = (lane >> 4) * 4 + reg
    if (col < D.pncols) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + kq * 4 + r;
        if (row < row_end) D.pz[(int64_t)row * D.pldz + col] = acc[r];
      }
    }
  };
#pragma unroll
  for (int it = 0; it < PT; ++it)
    if (w + 4 * it < n_ct) tile(w + 4 * it, pre[it]);
  for (int ct = w + 4 * PT; ct < n_ct; ct += 4) tile(ct, nullptr);
  KT(2);
}

// GS >= 32 (H-tree, hidden 128: ~1000 blocks of 16 rows): 4 waves per SIMD = 4 blocks per CU keeps the whole launch resident in
// one round (measured 0.152 -> 0.140 ms over the 4 layers of config 4; the same bound made the backward kernel slower and is
// not applied there)
template <int GS>
__global__ __launch_bounds__(256, GS == 32 ? 3 : (GS == 64 ? 2 : 1)) void agg_proj_fwd_kernel(const AggArgs a) {
  __shared__ float Hs[256 * 17];
  KT_BLOCK_BEGIN();
  KT_SPAN_BEGIN(40);
  int ti = 0;
  while (ti + 1 < a.n && (int)blockIdx.x >= a.bstart[ti + 1]) ++ti;
  karg_warm<9>((int)offsetof(AggArgs, d) + ti * (int)sizeof(AggDst), (int)sizeof(AggDst));
  const AggDst& D = a.d[ti];
  // (an entry of heavy rows is cut into tiles of 8: see AggDst::tile_rows)
  const int row0 = ((int)blockIdx.x - D.block_start) * D.tile_rows;
  agg_proj_tile<GS>(a, D, row0, min(row0 + D.tile_rows, D.n_rows), Hs);
  KT_SPAN_END(40, ti);
  KT_BLOCK_END();
}

// fixed-order sum of the per-row {loss, valid} pairs -> {loss_sum, count}; run by ONE block (256 threads)
__device__ __forceinline__ void finalize_loss(const float* __restrict__ row_lv, int n_rows, float* __restrict__ out2, NetState* state) {
  __shared__ float sl[256], sv[256];
  float l = 0.f, v = 0.f;
  for (int r = threadIdx.x; r < n_rows; r += 256) { l += row_lv[2 * r]; v += row_lv[2 * r + 1]; }
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

// dz[s][j, seg_e] = sum_{k in out_e(j)} g'[dst_k] / deg(dst_k);   dz[s][j, root] = g'[s][j]
// GB: the gradient rows (TAggOut::g, TAggSrc::groot) hold bf16 elements (bf16 compute mode at 10^6 rows, see load_z);
// DZB: so does the output dz (read back by the bf16 GEMMs as their A operand)
// One row of source entry S by its row group of GS lanes (c0 = first column of the lane).  put(v, seg, c) receives every finished
// piece -- a segment sum or the root copy: the lane's 4 elements at column c of the segment that starts at column `seg` of dz --
// and decides where it goes.
// live = false (a row past the entry's end inside a tile): extents read as 0 and the root as zeros, nothing is loaded for the row.
template <int GS, int NV, bool GB, class Sink>
__device__ __forceinline__ void agg_bwd_row(const TAggArgs& a, const TAggSrc& S, int row, bool live, int c0, const Sink& put) {
  constexpr int VEC = 4;
  int rb[AGG_MAX_IN], re[AGG_MAX_IN];
#pragma unroll
  for (int oi = 0; oi < AGG_MAX_IN; ++oi) {
    rb[oi] = re[oi] = 0;
    if (live && oi < S.n_out) { rb[oi] = S.out[oi].t_rowptr[row]; re[oi] = S.out[oi].t_rowptr[row + 1]; }
  }
  // (the 16-wide scalar-id form of agg_row was measured here too: 6.94 -> 7.02 ms at config 5, not kept)
  if constexpr (NV == 1) {
    // outgoing edge types in PAIRS (gather_pair): ids of both, then 1/deg + gradient rows of both
#pragma unroll
    for (int oi = 0; oi < AGG_MAX_IN; oi += 2) {
      if (oi >= S.n_out) break;
      const bool has2 = oi + 1 < S.n_out;
      const TAggOut& O0 = S.out[oi];
      const TAggOut& O1 = S.out[has2 ? oi + 1 : oi];
      const int b0 = rb[oi], e0 = re[oi];
      const int b1 = has2 ? rb[oi + 1] : b0, e1 = has2 ? re[oi + 1] : b0;
      Acc<VEC> a0[1], a1[1];
      gather_pair<GS, GB>(GatherSide{O0.g, O0.ldg, O0.t_col, b0, e0, O0.F}, GatherSide{O1.g, O1.ldg, O1.t_col, b1, e1, O1.F},
                          MeanW{O0.rowptr, O0.degf, a.mean}, MeanW{O1.rowptr, O1.degf, a.mean}, c0, a0, a1, false);
      if (c0 < O0.F) put(a0[0], O0.coff, c0);
      if (has2 && c0 < O1.F) put(a1[0], O1.coff, c0);
    }
  } else {
#pragma unroll
  for (int oi = 0; oi < AGG_MAX_IN; ++oi) {
    if (oi >= S.n_out) break;
    const TAggOut& O = S.out[oi];
    Acc<VEC> acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[q].zero();
    gather_sum<GS, NV, VEC, GB>(acc, O.g, O.ldg, O.t_col, rb[oi], re[oi], c0, O.F, MeanW{O.rowptr, O.degf, a.mean});
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int c = c0 + q * GS * VEC;
      if (c < O.F) put(acc[q], O.coff, c);
    }
  }
  }
  if (S.groot) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int c = c0 + q * GS * VEC;
      if (c < S.Froot) {
        Acc<VEC> v;
        v.zero();
        if (live) load_z<GB>(v, S.groot, (int64_t)row * S.ldgr + c);
        put(v, S.roff, c);
      }
    }
  }
}

template <int GS, int NV, bool GB = false, bool DZB = false>
__global__ __launch_bounds__(256) void agg_bwd_kernel(const TAggArgs a) {
  if ((int)blockIdx.x == a.total_blocks) {  // the extra block (only launched when fin_row_lv is set)
    finalize_loss(a.fin_row_lv, a.fin_rows, a.fin_out2, a.fin_state);
    return;
  }
  int si = 0;
  while (si + 1 < a.n && (int)blockIdx.x >= a.bstart[si + 1]) ++si;
  karg_warm<10>((int)offsetof(TAggArgs, s) + si * (int)sizeof(TAggSrc), (int)sizeof(TAggSrc));
  const TAggSrc& S = a.s[si];
  const int rpb = (S.tile_rows == 8 && 256 / GS > 8) ? 8 : 256 / GS;  // see agg_fwd_kernel
  int local = blockIdx.x - S.block_start;
  if (a.xcd) local = (local & 7) * ((cdiv_dev(S.n_rows, rpb) + 7) >> 3) + (local >> 3);  // see agg_fwd_kernel
  if ((int)threadIdx.x / GS >= rpb) return;
  int row = local * rpb + threadIdx.x / GS;
  if (GS == 64) row = __builtin_amdgcn_readfirstlane(row);  // wave-uniform, see agg_fwd_kernel
  if (row >= S.n_rows) return;
  agg_bwd_row<GS, NV, GB>(a, S, row, true, (int)(threadIdx.x % GS) * 4,
                          [&](Acc<4> v, int seg, int c) { store_z<DZB>(v, S.dz, (int64_t)row * S.lddz + seg + c); });
}

// ----- transposed aggregation of layer l FUSED with its input-gradient GEMM ------------------------------------------
// dH[l][s] = (dZ[l][s] * Wp[l][s]) . act'(H[l][s]) is row-local, so the block that has just gathered 16 rows of dZ keeps
// them in LDS ([k][row] image, LD 17) and multiplies them on the matrix cores (v_mfma_f32_16x16x4_f32, exact fp32): one
// kernel and one hand-off of dZ through L2 less per layer.  dZ is still written to HBM (the weight-gradient GEMM reads it).
// The reduction index k is the stacked column, the ROW index of Wp [ncols][ldw], so the weights are read from the transposed
// image WpT [fpad(xN)][xldt] that the pack writes next to Wp (PackSeg::dst_t; xldt = ncols rounded up to 16, padding zero):
// lane (nn, kq) loads 16 bytes WpT[n0 + nn][16 i + 4 kq .. +3] -- the operand fetch of agg_proj_tile -- and feeds 4 MFMAs with
// them.  The image's columns are interleaved inside every 16 (wpt_col, kernels.h) so that those 16 bytes are the stacked rows
// 16 i + 4 u + kq, u = 0..3: step u multiplies rows 16 i + 4 u .. + 3, the walk down Wp that 4-byte loads from Wp itself make
// (48 dependent-address loads per lane and column tile), and the sum over k comes out bit for bit the same.
// one 16-row tile [row0, row0 + 16) of source entry S, rows below row_end, by the workgroup's 256 threads; LDS image Hs
// [roundup16(ncols)][17], rows past ncols zero
template <int GS>
__device__ __forceinline__ void agg_bwd_dx_tile(const TAggArgs& a, const TAggSrc& S, int row0, int row_end, float* Hs) {
  constexpr int TM = 16, LDH = 17, VEC = 4;
  constexpr int RPP = 256 / GS;  // rows gathered per pass
  constexpr int NP = TM / RPP;   // passes (GS = 16: 1, 32: 2, 64: 4)
  constexpr int WB = 12;         // 16-deep k blocks per trip: 192 stacked columns, the whole operand at hidden width 64
  const int tid = threadIdx.x & 255;
  const int c0 = (tid % GS) * VEC;
  const int lane = threadIdx.x & 63, w = tid >> 6;
  const int nn = lane & 15, kq = lane >> 4;
  const int K = S.ncols, K16 = (K + 15) & ~15;
  KT(8);
  // GS = 16 (one gather pass, a launch of one round of workgroups: latency): the operands of the wave's first column tile that do
  // not depend on the gather are requested ahead of the barrier -- the activations (4 floats per lane) before the gather, the
  // first trip of weights (WB float4 per lane) right behind it, so that they travel while the tile is written to LDS.  The weights
  // BEFORE the gather, or behind its extent loads, were measured: the GEMM phase of workgroup 0 falls to 2.3 us, its gather grows
  // by 1.5 us (loads return in order: the first dependent step of the gather waits for 48 KB of weights per workgroup) and the
  // launch does not move (profiles/bwd_dx_transposed_weights.md).  GS >= 32 (several passes, several rounds of workgroups:
  // throughput) requests nothing early: measured slower there.
  constexpr bool EARLY = GS == 16;
  const int n_ct = S.xwt ? (S.xN + 15) >> 4 : 0;
  float4 pre[WB];
  auto fetch_first = [&]() {
    if (w >= n_ct) return;  // wave-uniform
    const float* wrow = S.xwt + (int64_t)min(w * 16 + nn, S.xN - 1) * S.xldt + 4 * kq;
#pragma unroll
    for (int i = 0; i < WB; ++i) pre[i] = *reinterpret_cast<const float4*>(wrow + min(16 * i, K16 - 16));
  };
  float hv0[4] = {0.f, 0.f, 0.f, 0.f};
  if (EARLY && S.xh && w < n_ct) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      hv0[r] = S.xh[(int64_t)min(row0 + kq * 4 + r, row_end - 1) * S.xldh + min(w * 16 + nn, S.xN - 1)];
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int m = p * RPP + tid / GS;
    const int row = row0 + m;
    const bool live = row < row_end;
    // every piece goes to the LDS image (zeros for a row past the end), and to dz if the row exists
    agg_bwd_row<GS, 1, false>(a, S, row, live, c0, [&](Acc<VEC> v, int seg, int c) {
      if (live) v.store(S.dz + (int64_t)row * S.lddz + seg + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) Hs[(seg + c + i) * LDH + m] = v.at(i);
    });
  }
  if constexpr (EARLY) fetch_first();
  // rows K .. K16 of the image meet the zero padding of WpT in the last k block
  for (int i = tid; i < (K16 - K) * TM; i += 256) Hs[(K + (i >> 4)) * LDH + (i & 15)] = 0.f;
  __syncthreads();
  if (S.xwt == nullptr) return;  // block-uniform
  KT(9);
  // one trip of WB k-blocks of 16 from k = kb on: the 16 bytes of weights the lane holds for a block are its rows k + 4 u + kq,
  // one MFMA each; the steps of the last block past K add products of the zero rows of Hs and the zero padding of WpT
  auto trip = [&](int kb, const float4 (&bv)[WB], f32x4& acc) {
#pragma unroll
    for (int i = 0; i < WB; ++i) {
      const int k = kb + 16 * i;
      if (k >= K) break;
      const float* hp = Hs + (k + kq) * LDH + nn;  // A operand: row m = lane & 15 of the tile
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hp[0 * LDH], bv[i].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hp[4 * LDH], bv[i].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hp[8 * LDH], bv[i].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hp[12 * LDH], bv[i].w, acc, 0, 0, 0);
    }
  };
  // one 16-column tile; first: its activations and the weights of its first trip are the ones requested early
  auto tile = [&](int ct, auto first) {
    const int col = ct * 16 + nn;
    const float* wrow = S.xwt + (int64_t)min(col, S.xN - 1) * S.xldt + 4 * kq;  // clamped: padded columns are never stored
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // activations whose derivative masks this tile's output: requested before the weight loads / MFMA chain instead of after
    float hv[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (decltype(first)::value) {
#pragma unroll
      for (int r = 0; r < 4; ++r) hv[r] = hv0[r];
    } else if (S.xh) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        hv[r] = S.xh[(int64_t)min(row0 + kq * 4 + r, row_end - 1) * S.xldh + min(col, S.xN - 1)];
    }
    int kb = 0;
    if constexpr (decltype(first)::value) {
      trip(0, pre, acc);
      kb = 16 * WB;
    }
    // the (clamped) 16-byte weight loads of a trip are all in flight together, then its MFMA chain runs
    for (; kb < K; kb += 16 * WB) {
      float4 bv[WB];
#pragma unroll
      for (int i = 0; i < WB; ++i) bv[i] = *reinterpret_cast<const float4*>(wrow + min(kb + 16 * i, K16 - 16));
      trip(kb, bv, acc);
    }
    // D layout: column = lane & 15, row = (lane >> 4) * 4 + reg
    if (col < S.xN) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + kq * 4 + r;
        if (row >= row_end) continue;
        float v = acc[r];
        if (S.xh) {
          const float h = hv[r];
          // dropped elements were stored as -0.0f by the forward: the keep bit is the sign of a zero
          const bool keep = !S.xdrop_on || (__float_as_uint(h) != 0x80000000u);
          float f = S.xscale;
          if (!keep) f = 0.f;
          else if (S.xact == HMP_ACT_RELU) f = h > 0.f ? S.xscale : 0.f;
          else if (S.xact == HMP_ACT_ELU) f = h > 0.f ? S.xscale : (h + S.xscale);
          v *= f;
        }
        S.xg[(int64_t)row * S.xldg + col] = v;
      }
    }
  };
  if constexpr (EARLY) {
    if (w < n_ct) tile(w, std::true_type());
    for (int ct = w + 4; ct < n_ct; ct += 4) tile(ct, std::false_type());
  } else {
    for (int ct = w; ct < n_ct; ct += 4) tile(ct, std::false_type());
  }
  KT(10);
}

template <int GS>
__global__ __launch_bounds__(256) void agg_bwd_dx_kernel(const TAggArgs a) {
  extern __shared__ float Hs[];  // [roundup16(ncols)][17]
  if ((int)blockIdx.x == a.total_blocks) {
    finalize_loss(a.fin_row_lv, a.fin_rows, a.fin_out2, a.fin_state);
    return;
  }
  KT_SPAN_BEGIN(48);
  int si = 0;
  while (si + 1 < a.n && (int)blockIdx.x >= a.bstart[si + 1]) ++si;
  karg_warm<10>((int)offsetof(TAggArgs, s) + si * (int)sizeof(TAggSrc), (int)sizeof(TAggSrc));
  const TAggSrc& S = a.s[si];
  const int row0 = ((int)blockIdx.x - S.block_start) * S.tile_rows;  // (tiles of 8 for entries of heavy rows: AggDst::tile_rows)
  agg_bwd_dx_tile<GS>(a, S, row0, min(row0 + S.tile_rows, S.n_rows), Hs);
  KT_SPAN_END(48, si);
}

// ----- LDS sliding-window aggregation for the 10^6-row regime (bf16 rows of 256 elements = 512 bytes) ------------------------
// Scene graphs are local: an object's neighbours are objects of the same room, and a graph builder numbers the objects of a
// room consecutively, so the source rows that a run of consecutive destination rows gathers lie in a narrow index window
// around the run (config 5: 90 % of a row's 16 neighbours inside its room's ~100 rows).  The one-wave-per-row kernels above
// fetch every neighbour row through L2 -> L1 -> registers once per EDGE (17 x 512 B per row, 9 GB per launch at 10^6 rows) and
// -- measured -- are bound by LATENCY x rows in flight, not by bytes: a row is a chain of 4 dependent round trips (extent ->
// neighbour ids -> rows -> more rows) of ~2 us each with ~24 rows in flight per CU.
//
// Here ONE persistent 1024-thread workgroup per CU walks a contiguous range of destination rows in chunks of WR = 64 and keeps
// a RING of WRING = 256 source rows in LDS (128 KiB): the chunk's own rows plus WM = 64 rows of margin either side.  Moving on
// one chunk brings exactly WR new rows in -- into the ring slots the new window no longer covers -- so every source row enters
// the CU ONCE per launch, with coalesced 16-byte loads issued one chunk ahead (they land while the current chunk computes).
// The chunk's CSR slice (row extents and neighbour ids of every incoming edge type: one contiguous range per type) is staged
// in LDS the same way, two / one chunks ahead.  A row then costs LDS reads only, except for the neighbours outside the window
// (the 10 % global edges; the other edge types, e.g. the room row of an object).  Those are requested FIRST, four rows at a time
// (buffer loads at a scalar offset; a descriptor of zero records where there is no such edge), the in-window edges follow in
// batches of eight LDS reads at scalar-computed slots (an out-of-window edge reads the all-zero row there), and the requested rows
// are added LAST (round 3; rounds 1-2 mixed both kinds inside a batch and waited for HBM per batch).  One accumulator per edge type;
// in-window rows in edge order, then the others in edge order.  Only the edge type whose source index space IS the destination's
// (objects -> objects) is windowed -- for bipartite types every source row is used once and staging buys nothing.
constexpr int WIN_THREADS = 1024;
constexpr int WIN_WAVES = WIN_THREADS / 64;
constexpr int WIN_ROW_BYTES = 512;  // 256 bf16
constexpr int WR = 64;              // destination rows per chunk
constexpr int WM = 64;              // margin rows either side
constexpr int WRING = 256;          // ring rows = WR + 2 WM + WR (power of two: slot = row & 255)
constexpr int WG = WR / WIN_WAVES;  // rows per wave and chunk (4)
constexpr int WIDCAP = 3072;        // neighbour ids per chunk staged in LDS (all incoming edge types; avg 64 x 17 = 1088)
constexpr int WRP = WR + 1;
constexpr int WIN_LDS_RING = (WRING + 1) * WIN_ROW_BYTES;  // + one all-zero row (slot WRING): what an out-of-window edge reads from LDS
constexpr int WIN_LDS_IDS = 2 * WIDCAP * 4;
constexpr int WIN_LDS_RP = 3 * AGG_MAX_IN * WRP * 4;
constexpr int WIN_LDS_DEG = WRING * 4;  // backward: reciprocal in-degrees of the ring rows
constexpr int WIN_LDS_FWD = WIN_LDS_RING + WIN_LDS_IDS + WIN_LDS_RP;
constexpr int WIN_LDS_BWD = WIN_LDS_FWD + WIN_LDS_DEG;
static_assert(WIN_LDS_BWD <= 160 * 1024, "LDS budget");
constexpr unsigned WIN_SKIP_OFF = 0xFFFFF000u;  // buffer offset beyond any record: the load returns 0 without touching memory
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// (raw buffers, buf_rsrc: an out-of-range offset reads as zero without a memory access -- lets a batch of edges issue BOTH an LDS
// read and a global read per edge without a branch: the one that does not apply is aimed at the zero row / out of range)

static_assert(AGG_MAX_IN == 6, "sel_q is written for 6 entries");
struct WinFwd {
  AggDst d;  // ONE destination entry, win_in >= 0
  int mean;
  int n_chunks, chunks_per_block;
  int dbg;   // HMP_WIN_DBG=1 (measurement only, wrong results): no edge reads global memory
};
struct WinBwd {
  TAggSrc s;  // ONE source entry, win_out >= 0
  int mean;
  int n_chunks, chunks_per_block;
};

__device__ __forceinline__ void widen_bf16x4(Acc<4>& a, const uint2 b) {
  a.v = make_float4(__uint_as_float(b.x << 16), __uint_as_float(b.x & 0xffff0000u), __uint_as_float(b.y << 16),
                    __uint_as_float(b.y & 0xffff0000u));
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int sel_q(const int (&s)[AGG_MAX_IN], int q) {  // q wave-uniform
  switch (q) {
    case 0: return s[0];
    case 1: return s[1];
    case 2: return s[2];
    case 3: return s[3];
    case 4: return s[4];
    default: return s[5];
  }
}
// Shared chunk pipeline of the forward and the transposed kernel.  WinTopo<E> supplies, per edge type q of the entry, the extent
// array (rowptr) and the id array (col); WinRing the matrix whose rows the ring holds and, for the transposed side, the per-row
// weights staged beside them.
struct WinLds {
  unsigned char* ring;  // [WRING + 1] rows of WIN_ROW_BYTES (slot WRING: the all-zero row)
  int* idbuf;           // [2][WIDCAP]
  int* rpbuf;           // [3][AGG_MAX_IN][WRP]
  float* wdeg;          // [WRING] weights of the ring rows (transposed kernel only)
};
struct WinRing {
  const uint16_t* x;  // rows as bf16 elements (column offset included)
  int ld;
  const float* degf;  // per-row weights travelling with the rows, null: none
};
struct WinStage {  // registers holding what phase A requested for the chunks ahead
  uint4 rows[(WR * 32) / WIN_THREADS];          // 2: the WR new ring rows of chunk c + 1
  int ids[(WIDCAP + WIN_THREADS - 1) / WIN_THREADS];  // 3: ids of chunk c + 1
  int rp;                                        // extents of chunk c + 2
  float deg;                                     // backward: reciprocal degrees of the new ring rows
};

template <class E>  // E: AggDst (forward: in[].rowptr / col) or TAggSrc (transposed: out[].t_rowptr / t_col)
struct WinTopo;
template <>
struct WinTopo<AggDst> {
  static __device__ __forceinline__ int n(const AggDst& D) { return D.n_in; }
  static __device__ __forceinline__ const int* rowptr(const AggDst& D, int q) { return D.in[q].rowptr; }
  static __device__ __forceinline__ const int* col(const AggDst& D, int q) { return D.in[q].col; }
  static __device__ __forceinline__ int rows(const AggDst& D) { return D.n_rows; }
};
template <>
struct WinTopo<TAggSrc> {
  static __device__ __forceinline__ int n(const TAggSrc& S) { return S.n_out; }
  static __device__ __forceinline__ const int* rowptr(const TAggSrc& S, int q) { return S.out[q].t_rowptr; }
  static __device__ __forceinline__ const int* col(const TAggSrc& S, int q) { return S.out[q].t_col; }
  static __device__ __forceinline__ int rows(const TAggSrc& S) { return S.n_rows; }
};

// extents of chunk `ch` -> register (thread t < n * WRP owns element t)
template <class E>
__device__ __forceinline__ int win_load_rp(const E& X, int ch, int n_chunks) {
  const int t = threadIdx.x, nq = WinTopo<E>::n(X);
  if (ch >= n_chunks || t >= nq * WRP) return 0;
  const int q = t / WRP, i = t - q * WRP;
  const int r = min(ch * WR + i, WinTopo<E>::rows(X));
  return WinTopo<E>::rowptr(X, q)[r];
}
// ids of one chunk (its extents already in LDS buffer rp; live = false: no such chunk) -> registers, zeros if they exceed WIDCAP
template <class E>
__device__ __forceinline__ void win_load_ids(const E& X, const int* rp, bool live, int (&ids)[(WIDCAP + WIN_THREADS - 1) / WIN_THREADS]) {
  const int nq = WinTopo<E>::n(X);
  int start[AGG_MAX_IN + 1], eb[AGG_MAX_IN];
  start[0] = 0;
#pragma unroll
  for (int q = 0; q < AGG_MAX_IN; ++q) {
    eb[q] = 0;
    int len = 0;
    if (live && q < nq) { eb[q] = rp[q * WRP]; len = rp[q * WRP + WR] - eb[q]; }
    start[q + 1] = start[q] + len;
  }
  const bool fits = start[AGG_MAX_IN] <= WIDCAP;
#pragma unroll
  for (int it = 0; it < (WIDCAP + WIN_THREADS - 1) / WIN_THREADS; ++it) {
    const int p = (int)threadIdx.x + it * WIN_THREADS;
    ids[it] = 0;
    if (fits && p < start[AGG_MAX_IN]) {
      const int* cq = WinTopo<E>::col(X, 0);
      int ebq = eb[0], stq = 0;
#pragma unroll
      for (int t = 1; t < AGG_MAX_IN; ++t)
        if (t < nq && p >= start[t]) { cq = WinTopo<E>::col(X, t); ebq = eb[t]; stq = start[t]; }
      ids[it] = cq[ebq + (p - stq)];
    }
  }
}
// per-chunk view of the staged CSR slice: id offset of every edge type inside the id buffer; false: the chunk did not fit
__device__ __forceinline__ bool win_offsets(const int* rp, int nq, int (&off)[AGG_MAX_IN], int (&eb)[AGG_MAX_IN]) {
  int acc = 0;
#pragma unroll
  for (int q = 0; q < AGG_MAX_IN; ++q) {
    off[q] = acc;
    eb[q] = 0;
    if (q < nq) { eb[q] = rp[q * WRP]; acc += rp[q * WRP + WR] - eb[q]; }
  }
  return acc <= WIDCAP;
}

// ids in registers -> one half of the LDS id buffer
__device__ __forceinline__ void win_store_ids(int* dst, const int (&ids)[(WIDCAP + WIN_THREADS - 1) / WIN_THREADS]) {
#pragma unroll
  for (int it = 0; it < (WIDCAP + WIN_THREADS - 1) / WIN_THREADS; ++it) {
    const int p = (int)threadIdx.x + it * WIN_THREADS;
    if (p < WIDCAP) dst[p] = ids[it];
  }
}
// prologue: extents of chunks c_begin, c_begin + 1; the zero row; the first window; ids of c_begin
template <class E>
__device__ __forceinline__ void win_prologue(const E& X, const WinRing& R, const WinLds& L, int c_begin, int n_chunks) {
  const int n_rows = WinTopo<E>::rows(X), nq = WinTopo<E>::n(X);
  const int r0 = win_load_rp(X, c_begin, n_chunks), r1 = win_load_rp(X, c_begin + 1, n_chunks);
  if ((int)threadIdx.x < nq * WRP) {
    L.rpbuf[(c_begin % 3) * AGG_MAX_IN * WRP + threadIdx.x] = r0;
    L.rpbuf[((c_begin + 1) % 3) * AGG_MAX_IN * WRP + threadIdx.x] = r1;
  }
  if ((int)threadIdx.x < 32) *reinterpret_cast<uint4*>(L.ring + (size_t)WRING * WIN_ROW_BYTES + threadIdx.x * 16) = make_uint4(0u, 0u, 0u, 0u);
  // rows [lo, hi) of the first window (everything the ring will hold for chunk c_begin)
  const int lo = max(c_begin * WR - WM, 0), hi = min(c_begin * WR + WR + WM, n_rows);
  for (int p = threadIdx.x; p < (hi - lo) * 32; p += WIN_THREADS) {
    const int r = lo + (p >> 5), piece = p & 31;
    const uint4 v = *reinterpret_cast<const uint4*>(R.x + (int64_t)r * R.ld + piece * 8);
    *reinterpret_cast<uint4*>(L.ring + (size_t)(r & (WRING - 1)) * WIN_ROW_BYTES + piece * 16) = v;
  }
  if (R.degf && (int)threadIdx.x < hi - lo) L.wdeg[(lo + threadIdx.x) & (WRING - 1)] = R.degf[lo + threadIdx.x];
  __syncthreads();
  int ids[(WIDCAP + WIN_THREADS - 1) / WIN_THREADS];
  win_load_ids(X, L.rpbuf + (c_begin % 3) * AGG_MAX_IN * WRP, true, ids);
  win_store_ids(L.idbuf + (c_begin & 1) * WIDCAP, ids);
  __syncthreads();
}
// phase A of chunk ch: request what the NEXT chunks need (lands while this chunk computes)
template <class E>
__device__ __forceinline__ void win_request(const E& X, const WinRing& R, const WinLds& L, int ch, int c_end, int n_chunks, WinStage& stg) {
  const int n_rows = WinTopo<E>::rows(X);
  const bool next = ch + 1 < c_end;
  const int nlo = ch * WR + WR + WM;  // new ring rows of chunk ch + 1: [nlo, nlo + WR)
#pragma unroll
  for (int it = 0; it < (WR * 32) / WIN_THREADS; ++it) {
    const int p = (int)threadIdx.x + it * WIN_THREADS;
    const int r = nlo + (p >> 5), piece = p & 31;
    stg.rows[it] = make_uint4(0u, 0u, 0u, 0u);
    if (next && r < n_rows) stg.rows[it] = *reinterpret_cast<const uint4*>(R.x + (int64_t)r * R.ld + piece * 8);
  }
  stg.deg = 0.f;
  if (next && R.degf && (int)threadIdx.x < WR && nlo + (int)threadIdx.x < n_rows) stg.deg = R.degf[nlo + threadIdx.x];
  win_load_ids(X, L.rpbuf + ((ch + 1) % 3) * AGG_MAX_IN * WRP, next, stg.ids);
  stg.rp = (ch + 2 < c_end) ? win_load_rp(X, ch + 2, n_chunks) : 0;
}
// phase D of chunk ch: what phase A requested goes to LDS (ring slots / buffers this chunk did not read)
template <class E>
__device__ __forceinline__ void win_commit(const E& X, const WinRing& R, const WinLds& L, int ch, int c_end, const WinStage& stg) {
  if (ch + 1 >= c_end) return;
  const int n_rows = WinTopo<E>::rows(X), nq = WinTopo<E>::n(X);
  const int nlo = ch * WR + WR + WM;
#pragma unroll
  for (int it = 0; it < (WR * 32) / WIN_THREADS; ++it) {
    const int p = (int)threadIdx.x + it * WIN_THREADS;
    const int r = nlo + (p >> 5), piece = p & 31;
    if (r < n_rows) *reinterpret_cast<uint4*>(L.ring + (size_t)(r & (WRING - 1)) * WIN_ROW_BYTES + piece * 16) = stg.rows[it];
  }
  if (R.degf && (int)threadIdx.x < WR && nlo + (int)threadIdx.x < n_rows) L.wdeg[(nlo + threadIdx.x) & (WRING - 1)] = stg.deg;
  win_store_ids(L.idbuf + ((ch + 1) & 1) * WIDCAP, stg.ids);
  if (ch + 2 < c_end && (int)threadIdx.x < nq * WRP) L.rpbuf[((ch + 2) % 3) * AGG_MAX_IN * WRP + threadIdx.x] = stg.rp;
}

// The rows of one list of <= 64 edges (lane u = edge u), summed into acc.  WT = false (forward): plain adds.  WT = true
// (transposed): every row times the weight of its edge, which lives in lane u of a register and is read by readlane -- add_mul if
// `mean`, else a plain add.
// Far rows (outside the window, or of a list without one): the set bits of fm, up to four in flight.
template <bool WT>
struct WinFar {
  u32x2 fv[4];
  int fu[4];
  // request the next (up to) four set bits of fm: row of edge u at byte offset readlane(gov, u) + voff of the buffer rs
  __device__ __forceinline__ void issue(unsigned long long& fm, __amdgpu_buffer_rsrc_t rs, __amdgpu_buffer_rsrc_t rs_null, int voff, int gov) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      fu[t] = fm ? __builtin_ctzll(fm) : 0;
      fv[t] = __builtin_amdgcn_raw_buffer_load_b64(fm ? rs : rs_null, voff, __builtin_amdgcn_readlane(gov, fu[t]), 0);
      fm &= fm - 1ull;  // (0 stays 0)
    }
  }
  __device__ __forceinline__ void add(Acc<4>& acc, int mean, int wv) const {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      Acc<4> w;
      widen_bf16x4(w, make_uint2(fv[t][0], fv[t][1]));
      if (WT && mean) acc.add_mul(w, __int_as_float(__builtin_amdgcn_readlane(wv, fu[t]))); else acc.add(w);  // (a null read: 0 x a finite weight)
    }
  }
};
// NB in-window rows (edges u0 .. u0 + NB - 1) from the ring: LDS reads at scalar-computed slots (lane u of lov = byte offset of edge u's row)
template <int NB, bool WT>
__device__ __forceinline__ void win_batch(Acc<4>& acc, const unsigned char* ring, int lov, int lane, int u0, int mean, int wv) {
  uint2 va[NB];
#pragma unroll
  for (int t = 0; t < NB; ++t) va[t] = *reinterpret_cast<const uint2*>(ring + __builtin_amdgcn_readlane(lov, u0 + t) + lane * 8);
#pragma unroll
  for (int t = 0; t < NB; ++t) {
    Acc<4> w;
    widen_bf16x4(w, va[t]);
    if (WT && mean) acc.add_mul(w, __int_as_float(__builtin_amdgcn_readlane(wv, u0 + t))); else acc.add(w);
  }
}
// one list: far rows requested FIRST, the in-window edges (wq: the list has a window) follow in batches of eight LDS reads, the
// requested rows are added LAST; more than four far rows: further rounds, each waited for
template <bool WT>
__device__ __forceinline__ void win_sum_list(Acc<4>& acc, unsigned long long fm, bool wq, int cnt, const unsigned char* ring, int lov, int lane,
                                             __amdgpu_buffer_rsrc_t rs, __amdgpu_buffer_rsrc_t rs_null, int voff, int gov, int mean, int wv_ring,
                                             int wv_far) {
  WinFar<WT> far;
  const bool any_far = fm != 0ull;
  if (any_far) far.issue(fm, rs, rs_null, voff, gov);
  if (wq) {
    int u0 = 0;
    for (; cnt - u0 > 2; u0 += 8) win_batch<8, WT>(acc, ring, lov, lane, u0, mean, wv_ring);
    if (u0 < cnt) win_batch<2, WT>(acc, ring, lov, lane, u0, mean, wv_ring);
  }
  if (any_far) {
    far.add(acc, mean, wv_far);
    while (fm) {
      far.issue(fm, rs, rs_null, voff, gov);
      far.add(acc, mean, wv_far);
    }
  }
}

template <bool HB>
__global__ __launch_bounds__(WIN_THREADS) void agg_fwd_win_kernel(const WinFwd a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wlds[];
  const WinLds L = {wlds, reinterpret_cast<int*>(wlds + WIN_LDS_RING), reinterpret_cast<int*>(wlds + WIN_LDS_RING + WIN_LDS_IDS), nullptr};
  const AggDst& D = a.d;
  const int n_rows = D.n_rows, nq = D.n_in;
  const int c_begin = (int)blockIdx.x * a.chunks_per_block;
  const int c_end = min(c_begin + a.chunks_per_block, a.n_chunks);
  if (c_begin >= c_end) return;  // block-uniform
  const int wave = uni((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  const AggIn& IW = D.in[D.win_in];
  const WinRing R = {reinterpret_cast<const uint16_t*>(IW.z) + IW.coff, IW.ldz, nullptr};
  const int c0 = lane * 4;
  DropCfg dcfg = D.drop;
  if (D.drop_on) dcfg = drop_resolve(D.drop);
  Acc<4> biasv;  // the lane's 4 bias columns: the same for every row
  biasv.zero();
  if (D.bias) biasv.load(D.bias + c0);

  win_prologue(D, R, L, c_begin, a.n_chunks);

  for (int i = 20; i < 31; ++i) KT_ZERO(i);
  for (int ch = c_begin; ch < c_end; ++ch) {
    const int r_c = ch * WR;
    const int* rp = L.rpbuf + (ch % 3) * AGG_MAX_IN * WRP;
    const int* idc = L.idbuf + (ch & 1) * WIDCAP;
    [[maybe_unused]] const unsigned long long kt_a = KT_NOW();
    WinStage stg;
    win_request(D, R, L, ch, c_end, a.n_chunks, stg);
    KT_ADD(20, kt_a);
    [[maybe_unused]] const unsigned long long kt_c = KT_NOW();
    // ---- this chunk ----------------------------------------------------------------------------------------------------------
    int off[AGG_MAX_IN], eb[AGG_MAX_IN];
    const bool fits = win_offsets(rp, nq, off, eb);
    const int wlo = max(r_c - WM, 0), whi = min(r_c + WR + WM, n_rows);  // rows the ring holds now
    {  // (!fits, block-uniform: a chunk with more ids than the LDS slice holds reads extents / ids from global memory, no window)
      // Round 3: the counters had the waves of this kernel waiting 57 % of their cycles (SQ_WAIT_ANY / SQ_WAVE_CYCLES) and the vector
      // unit 56 % busy -- a row was a chain of ~7 dependent waits (extents, ids and row batches per edge type).  Now (a) the extents of
      // all of the wave's rows are ONE lane-parallel LDS read per chunk and reach the scalar unit by readlane; (b) the neighbour ids
      // of the NEXT row's window list and of its deferred list are requested while this row computes; (c) the edge type after the
      // window one (rooms -> objects: one or two global rows) has its rows requested BEFORE the window batches and is added after
      // them -- same accumulators, same order of additions (the out-of-window rows of the window list are added behind the in-window
      // ones since the far-first change below: fp32, mostly the same bits).
      const int WQ = D.win_in, DQ = (fits && WQ + 1 < nq) ? WQ + 1 : -1;  // wave-uniform
      int rpv = 0;  // lane 8 q + 2 g + h: extent h of the wave's g-th row, edge type q
      if (fits && (lane >> 3) < nq) rpv = rp[(lane >> 3) * WRP + ((lane & 7) >> 1) * WIN_WAVES + wave + (lane & 1)];
      const int offW = sel_q(off, WQ) - sel_q(eb, WQ), offD = DQ >= 0 ? sel_q(off, DQ) - sel_q(eb, DQ) : 0;  // + extent = id slot
      auto ids_of = [&](int g, int q, int offq) {  // ids 0..63 of row g's list of edge type q (staged chunk only)
        const int b = __builtin_amdgcn_readlane(rpv, q * 8 + g * 2), e = __builtin_amdgcn_readlane(rpv, q * 8 + g * 2 + 1);
        return lane < e - b ? idc[offq + b + lane] : 0;
      };
      int idw = 0, idd = 0;
      if (fits) {
        idw = ids_of(0, WQ, offW);
        if (DQ >= 0) idd = ids_of(0, DQ, offD);
      }
      // phase B: the root row travels one row ahead as well
      auto root_of = [&](int g) {
        const int row = r_c + g * WIN_WAVES + wave;
        uint2 r = make_uint2(0u, 0u);
        if (g < WG && row < n_rows && D.zroot)
          r = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(D.zroot) + (int64_t)row * D.ldzr + D.roff + c0);
        return r;
      };
      uint2 root = root_of(0);
      // phase C: sums in edge order, one accumulator per edge type.  The neighbour id of an edge is wave-uniform (readlane), so
      // its row comes either from the LDS ring (one ds_read_b64 at a scalar-computed slot) or from global memory (scalar base +
      // lane offset): a scalar branch per edge, no per-lane address arithmetic, 16 loads in flight per batch.
#pragma unroll 1
      for (int g = 0; g < WG; ++g) {
        const int rl = g * WIN_WAVES + wave, row = r_c + rl;
        if (row >= n_rows) break;  // rows grow with g
        [[maybe_unused]] const unsigned long long kt_r = KT_NOW();
        const uint2 root_n = root_of(g + 1);
        int idw_n = 0, idd_n = 0;  // (b) the next row's ids: in flight while this row's batches run
        if (fits && g + 1 < WG) {
          idw_n = ids_of(g + 1, WQ, offW);
          if (DQ >= 0) idd_n = ids_of(g + 1, DQ, offD);
        }
        // (c) deferred edge type: a list of one or two rows is requested here and consumed after the window list
        u32x2 vd[2] = {{0u, 0u}, {0u, 0u}};
        int cntD = 0;
        if (DQ >= 0) {
          const int bD = __builtin_amdgcn_readlane(rpv, DQ * 8 + g * 2), eD = __builtin_amdgcn_readlane(rpv, DQ * 8 + g * 2 + 1);
          if (eD - bD >= 1 && eD - bD <= 2) {
            cntD = eD - bD;
            const AggIn& I = D.in[DQ];
            const uint16_t* zq = reinterpret_cast<const uint16_t*>(I.z) + I.coff;
            const __amdgpu_buffer_rsrc_t rs = buf_rsrc(zq, (unsigned)I.n_src * (unsigned)(I.ldz * 2) - (unsigned)(I.coff * 2));
            const __amdgpu_buffer_rsrc_t rs_null = buf_rsrc(zq, 0u);
            const int gov = lane < cntD ? idd * (I.ldz * 2) : 0;
            vd[0] = __builtin_amdgcn_raw_buffer_load_b64(rs, lane * 8, __builtin_amdgcn_readlane(gov, 0), 0);
            vd[1] = __builtin_amdgcn_raw_buffer_load_b64(cntD > 1 ? rs : rs_null, lane * 8, __builtin_amdgcn_readlane(gov, 1), 0);
          }
        }
        Acc<4> tot;
        tot.zero();
        if (D.zroot) widen_bf16x4(tot, root);
        tot.add(biasv);
#pragma unroll 1
        for (int q = 0; q < nq; ++q) {
          const AggIn& I = D.in[q];
          if (q == DQ && cntD) {  // the deferred list: its rows have landed behind the window batches
            Acc<4> acc, w;
            acc.zero();
            widen_bf16x4(w, make_uint2(vd[0][0], vd[0][1]));
            acc.add(w);
            widen_bf16x4(w, make_uint2(vd[1][0], vd[1][1]));
            acc.add(w);
            tot.add_div(acc, a.mean ? (float)cntD : 1.f);
            continue;
          }
          const int b = fits ? __builtin_amdgcn_readlane(rpv, q * 8 + g * 2) : I.rowptr[row];
          const int e = fits ? __builtin_amdgcn_readlane(rpv, q * 8 + g * 2 + 1) : I.rowptr[row + 1];
          if (e == b) continue;
          const uint16_t* zq = reinterpret_cast<const uint16_t*>(I.z) + I.coff;
          const int ldq = I.ldz;
          const __amdgpu_buffer_rsrc_t rs = buf_rsrc(zq, (unsigned)I.n_src * (unsigned)(ldq * 2) - (unsigned)(I.coff * 2));
          const __amdgpu_buffer_rsrc_t rs_null = buf_rsrc(zq, 0u);
          const int offq = fits ? sel_q(off, q) + (b - sel_q(eb, q)) : 0;
          const bool wq = fits && q == WQ;
          Acc<4> acc;
          acc.zero();
          for (int base = 0; base < e - b; base += 64) {
            const int cnt = min(e - b - base, 64);
            int idv = 0;
            if (wq && base == 0) idv = idw;  // requested one row ago
            else if (lane < cnt) idv = fits ? idc[offq + base + lane] : I.col[b + base + lane];
            // Round 3: a row's OUT-OF-WINDOW rows (and the rows of an edge type without a window) are requested first, four at a time,
            // and added last; every batch in between reads LDS only (an out-of-window edge reads the all-zero row there).  Before, an
            // out-of-window edge sat inside its batch of eight -- LDS read OR buffer read per edge, branch-free -- and the batch waited
            // for a random 512-byte row from HBM before the next batch was even issued (profiles/r03_n_matrix_pipe_window_sum.md).
            // fp32 sums: in-window rows in edge order, then the others in edge order -- another association than the plain kernels'.
            const bool inw = lane < cnt && wq && idv >= wlo && idv < whi;
            const int lov = inw ? (idv & (WRING - 1)) * WIN_ROW_BYTES : WRING * WIN_ROW_BYTES;
            const int gov = idv * (ldq * 2);
            const unsigned long long fm = __ballot(lane < cnt && !inw) & (a.dbg ? 0ull : ~0ull);  // (dbg: measurement only -- no global reads)
            win_sum_list<false>(acc, fm, wq, cnt, L.ring, lov, lane, rs, rs_null, lane * 8, gov, 0, 0, 0);
          }
          tot.add_div(acc, a.mean ? (float)(e - b) : 1.f);
        }
        KT_ADD(29, kt_r);
        agg_act_drop4(D, dcfg, row, c0, tot);
        store_z<HB>(tot, D.out, (int64_t)row * D.ldo + c0);
        KT_ADD(30, kt_r);
        idw = idw_n;
        idd = idd_n;
        root = root_n;
      }
    }
    KT_ADD(21, kt_c);
    [[maybe_unused]] const unsigned long long kt_d = KT_NOW();
    win_commit(D, R, L, ch, c_end, stg);
    KT_ADD(22, kt_d);
    [[maybe_unused]] const unsigned long long kt_b = KT_NOW();
    __syncthreads();
    KT_ADD(23, kt_b);
    KT_ADD(24, kt_a);
  }
}

// transposed counterpart: source rows in chunks, ring over the gradient rows G of the destination type (same index space) and
// their reciprocal in-degrees; one accumulator and one output segment per outgoing edge type
template <bool DZB>
__global__ __launch_bounds__(WIN_THREADS) void agg_bwd_win_kernel(const WinBwd a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wlds[];
  const WinLds L = {wlds, reinterpret_cast<int*>(wlds + WIN_LDS_RING), reinterpret_cast<int*>(wlds + WIN_LDS_RING + WIN_LDS_IDS),
                    reinterpret_cast<float*>(wlds + WIN_LDS_FWD)};
  const TAggSrc& S = a.s;
  const int n_rows = S.n_rows, nq = S.n_out;
  const int c_begin = (int)blockIdx.x * a.chunks_per_block;
  const int c_end = min(c_begin + a.chunks_per_block, a.n_chunks);
  if (c_begin >= c_end) return;
  const int wave = uni((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  const TAggOut& OW = S.out[S.win_out];
  // (the weights of the ring rows are staged beside them when the plan's table is there)
  const WinRing R = {reinterpret_cast<const uint16_t*>(OW.g), OW.ldg, a.mean ? OW.degf : nullptr};
  const int c0 = lane * 4;
  win_prologue(S, R, L, c_begin, a.n_chunks);
  for (int ch = c_begin; ch < c_end; ++ch) {
    const int r_c = ch * WR;
    const int* rp = L.rpbuf + (ch % 3) * AGG_MAX_IN * WRP;
    const int* idc = L.idbuf + (ch & 1) * WIDCAP;
    WinStage stg;
    win_request(S, R, L, ch, c_end, a.n_chunks, stg);
    int off[AGG_MAX_IN], eb[AGG_MAX_IN];
    const bool fits = win_offsets(rp, nq, off, eb);
    const int wlo = max(r_c - WM, 0), whi = min(r_c + WR + WM, n_rows);
    // phase C (see agg_fwd_win_kernel): one accumulator and one output segment per outgoing edge type
#pragma unroll 1
    for (int g = 0; g < WG; ++g) {
      const int rl = g * WIN_WAVES + wave, row = r_c + rl;
      if (row >= n_rows) continue;
#pragma unroll 1
      for (int q = 0; q < nq; ++q) {
        const TAggOut& O = S.out[q];
        const int b = fits ? uni(rp[q * WRP + rl]) : O.t_rowptr[row], e = fits ? uni(rp[q * WRP + rl + 1]) : O.t_rowptr[row + 1];
        const bool cin = c0 < O.F;
        const int cc = cin ? c0 : 0;
        const bool dg = a.mean && O.degf != nullptr;
        const uint16_t* gq = reinterpret_cast<const uint16_t*>(O.g);
        const int ldq = O.ldg;
        const __amdgpu_buffer_rsrc_t rs = buf_rsrc(gq, (unsigned)O.n_dst * (unsigned)(ldq * 2));
        const __amdgpu_buffer_rsrc_t rs_null = buf_rsrc(gq, 0u);
        const int offq = fits ? sel_q(off, q) + (b - sel_q(eb, q)) : 0;
        const bool wq = fits && q == S.win_out;
        Acc<4> acc;
        acc.zero();
        for (int base = 0; base < e - b; base += 64) {
          const int cnt = min(e - b - base, 64);
          const int idv = lane < cnt ? (fits ? idc[offq + base + lane] : O.t_col[b + base + lane]) : 0;
          const bool inw = lane < cnt && wq && idv >= wlo && idv < whi;
          const bool farl = lane < cnt && !inw;
          // the edge's weight 1 / deg(dst), lane u = edge u: in-window edges from the ring's table (LDS), the others from global memory --
          // in TWO registers, so that the LDS batches never wait for the global ones (see agg_fwd_win_kernel: out-of-window rows are
          // requested first and added last)
          float dvl = 1.f, dvg = 1.f;
          if (a.mean) {
            if (dg) {
              if (inw) dvl = L.wdeg[idv & (WRING - 1)];
              if (farl) dvg = O.degf[idv];
            } else if (lane < cnt) {
              const int g0 = O.rowptr[idv + 1] - O.rowptr[idv];
              dvl = dvg = 1.f / (float)(g0 > 1 ? g0 : 1);
            }
          }
          const int dvli = __float_as_int(dvl), dvgi = __float_as_int(dvg);
          const int lov = inw ? (idv & (WRING - 1)) * WIN_ROW_BYTES : WRING * WIN_ROW_BYTES;  // see agg_fwd_win_kernel
          const int gov = idv * (ldq * 2);
          win_sum_list<true>(acc, __ballot(farl), wq, cnt, L.ring, lov, lane, rs, rs_null, cc * 2, gov, a.mean, dvli, dvgi);
        }
        if (cin) store_z<DZB>(acc, S.dz, (int64_t)row * S.lddz + O.coff + c0);
      }
      if (S.groot && c0 < S.Froot) {
        Acc<4> v;
        load_z<true>(v, S.groot, (int64_t)row * S.ldgr + c0);
        store_z<DZB>(v, S.dz, (int64_t)row * S.lddz + S.roff + c0);
      }
    }
    win_commit(S, R, L, ch, c_end, stg);
    __syncthreads();
  }
}

// ----- dispatch ---------------------------------------------------------------------------------------
// lanes needed = ceil(F / VEC); GS = next pow2 in [8, 64]; NV = ceil(lanes / GS) <= 4
// Measured at config 5 (10^6 rows of 256 floats, rocprofv3 --pmc): 152 M L2 requests per forward launch (= the 128-byte lines
// of the algorithm: 17 neighbour rows + root + output per row), 70 % hits, 0.1 % memory-unit stalls, VALU 40 % busy, 2.33 ms.
// The microarchitecture guide's gather rates (~18 TB/s from L2, ~6 TB/s beyond it) put the same traffic at ~1.7 ms, so the
// one-row-per-wave kernels run at ~75 % of the practical ceiling.  Tried on top and measured neutral (+-3 %), hence not kept:
// bf16 rows; 6 instead of 4 resident waves per SIMD (80-register shape without pair batching); a streaming form in which a
// wave walks 8 consecutive rows with the index chain of the next two rows in flight (bit-identical, forward 4.62 -> 4.96 ms,
// backward 7.54 -> 7.38 ms).  Kept: the XCD-contiguous row ranges below (neutral here, but it is the mapping that does not
// depend on the Infinity Cache absorbing 8 copies of every shared row).

static inline void pick_shape(int F, int vec, int& gs, int& nv) {
  const int lanes = cdiv(F, vec);
  gs = 8;
  while (gs < 64 && gs < lanes) gs <<= 1;
  nv = cdiv(lanes, gs);
}

#define HMP_DISPATCH_GS_NV(GSV, NVV, MACRO)                                       \
  switch ((GSV) * 8 + (NVV)) {                                                    \
    case 8 * 8 + 1: MACRO(8, 1); break;                                           \
    case 16 * 8 + 1: MACRO(16, 1); break;                                         \
    case 32 * 8 + 1: MACRO(32, 1); break;                                         \
    case 64 * 8 + 1: MACRO(64, 1); break;                                         \
    case 64 * 8 + 2: MACRO(64, 2); break;                                         \
    case 64 * 8 + 3: MACRO(64, 3); break;                                         \
    case 64 * 8 + 4: MACRO(64, 4); break;                                         \
    default: HMP_FAIL(HMP_E_ARG, "row width %d not supported by the aggregation kernels (max %d)", Fmax, 64 * 4 * vec); \
  }

constexpr int64_t AGG_XCD_ROWS = 65536;  // from here on the launch is several waves of blocks deep and L2 locality pays
static bool agg_xcd_enabled() {  // HMP_AGG_XCD=0: plain block order (tests compare both orders bit for bit)
  return env_switch("HMP_AGG_XCD") != '0';
}

// HMP_AGG_WIN=0 turns the LDS sliding-window kernels off (tests compare both forms bit for bit)
static bool agg_win_enabled() { return env_switch("HMP_AGG_WIN") != '0'; }
constexpr int AGG_WIN_MIN_ROWS = 16384;  // below: a persistent grid would leave CUs idle, the plain kernels do as well
static int agg_win_grid(int n_chunks, int& per_block) {
  per_block = cdiv(n_chunks, device_cu_count());
  return cdiv(n_chunks, per_block);
}

static int agg_win_in(const AggDst& D) {  // in-conv to serve from the LDS ring, -1: none
  if (D.F != 256 || D.n_rows < AGG_WIN_MIN_ROWS || D.ce_labels || (D.ldo & 3) || !D.zroot) return -1;
  for (int ii = 0; ii < D.n_in; ++ii)  // every source matrix addressable by a 32-bit buffer offset below WIN_SKIP_OFF
    if ((uint64_t)D.in[ii].n_src * (uint64_t)D.in[ii].ldz * 2 > (uint64_t)WIN_SKIP_OFF) return -1;
  for (int ii = 0; ii < D.n_in; ++ii) {
    const AggIn& I = D.in[ii];
    if (I.same_type && !(I.coff & 7) && !(I.ldz & 7) && !(reinterpret_cast<uintptr_t>(I.z) & 15)) return ii;
  }
  return -1;
}
static int agg_win_out(const TAggSrc& S) {
  if (S.n_rows < AGG_WIN_MIN_ROWS) return -1;
  for (int oi = 0; oi < S.n_out; ++oi)
    if ((uint64_t)S.out[oi].n_dst * (uint64_t)S.out[oi].ldg * 2 > (uint64_t)WIN_SKIP_OFF) return -1;
  for (int oi = 0; oi < S.n_out; ++oi) {
    const TAggOut& O = S.out[oi];
    if (O.same_type && O.F == 256 && !(O.ldg & 7) && !(reinterpret_cast<uintptr_t>(O.g) & 15)) return oi;
  }
  return -1;
}

constexpr int AGG_SMALL_TILES = 224;  // 16-row tiles of a launch up to which heavy entries are cut into tiles of 8 (AggDst::tile_rows)
// the entries of either argument block (they differ in the member name only)
static inline AggDst* agg_entries(AggArgs& a) { return a.d; }
static inline TAggSrc* agg_entries(TAggArgs& a) { return a.s; }
// the compact copy of the entries' first blocks that the kernels search (AggArgs::bstart)
template <class Args>
static inline void sync_bstart(Args& a) {
  for (int i = 0; i < a.n; ++i) a.bstart[i] = agg_entries(a)[i].block_start;
}
// Block layout of a row-group launch (agg_fwd_kernel / agg_bwd_kernel): an entry owns ceil(n_rows / rpb) blocks, rpb = 256 / gs rows
// or 8 for an entry of heavy rows (tile_rows == 8).  xcd: every entry starts at a multiple of 8 and owns whole groups of 8 blocks.
template <class Args>
static int agg_layout_rows(Args& a, int gs) {
  int blocks = 0;
  for (int i = 0; i < a.n; ++i) {
    auto& X = agg_entries(a)[i];
    X.block_start = blocks;
    const int nb = cdiv(X.n_rows, (X.tile_rows == 8 && 256 / gs > 8) ? 8 : 256 / gs);
    blocks += a.xcd ? ((nb + 7) & ~7) : nb;
  }
  a.total_blocks = blocks;
  return blocks;
}
// Tile layout of a fused launch (agg_proj_fwd_kernel / agg_bwd_dx_kernel): one block per tile of 16 rows; tiles of 8 rows for heavy
// entries only while the launch leaves CUs idle (more workgroups in a launch of several rounds only add rounds)
template <class Args>
static int agg_layout_tiles(Args& a) {
  int tiles16 = 0, blocks = 0;
  for (int i = 0; i < a.n; ++i) tiles16 += cdiv(agg_entries(a)[i].n_rows, 16);
  const bool small_launch = tiles16 <= AGG_SMALL_TILES;
  for (int i = 0; i < a.n; ++i) {
    auto& X = agg_entries(a)[i];
    if (X.tile_rows != 8 || !small_launch) X.tile_rows = 16;
    X.block_start = blocks;
    blocks += cdiv(X.n_rows, X.tile_rows);
  }
  a.total_blocks = blocks;
  return blocks;
}
static int agg_tile_gs(int Fmax) {  // row group of the fused kernels: 16, 32 or 64 lanes
  int gs = 16;
  while (gs < 64 && gs * 4 < Fmax) gs <<= 1;
  return gs;
}

static void win_fill(WinFwd& w, const AggDst& D) {
  w.d = D;
  w.d.win_in = agg_win_in(D);
#ifdef HMP_KTIME  // measurement-only switch (wrong results): profiling build only
  const char* dv = getenv("HMP_WIN_DBG");
  w.dbg = dv ? atoi(dv) : 0;
#endif
}
static void win_fill(WinBwd& w, const TAggSrc& S) {
  w.s = S;
  w.s.win_out = agg_win_out(S);
}
// bf16 launches: entries with a same-type edge type over >= 16384 rows go to the sliding-window kernel (one launch each, in entry
// order, persistent grid of one workgroup per CU); the others stay in `a` for the plain launch.  *any: at least one entry went.
template <class Args>
static int agg_win_peel(Args& a, hipStream_t st, bool* any) {
  constexpr bool FWD = std::is_same<Args, AggArgs>::value;
  using Win = typename std::conditional<FWD, WinFwd, WinBwd>::type;
  constexpr int LDS = FWD ? WIN_LDS_FWD : WIN_LDS_BWD;
  void (*k16)(const Win), (*k32)(const Win);  // output written as bf16 / fp32
  bool out16;
  if constexpr (FWD) { k16 = &agg_fwd_win_kernel<true>; k32 = &agg_fwd_win_kernel<false>; out16 = a.hb16; }
  else { k16 = &agg_bwd_win_kernel<true>; k32 = &agg_bwd_win_kernel<false>; out16 = a.dzb16; }
  Args rest = a;
  rest.n = 0;
  *any = false;
  for (int i = 0; i < a.n; ++i) {
    const auto& X = agg_entries(a)[i];
    Win w;
    memset(&w, 0, sizeof(w));
    win_fill(w, X);
    bool win;
    if constexpr (FWD) win = w.d.win_in >= 0; else win = w.s.win_out >= 0;
    if (!win) { agg_entries(rest)[rest.n++] = X; continue; }
    static bool attr_done = false;
    if (!attr_done) {
      HMP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k16), hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
      HMP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k32), hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
      attr_done = true;
    }
    w.mean = a.mean;
    w.n_chunks = cdiv(X.n_rows, WR);
    const int grid = agg_win_grid(w.n_chunks, w.chunks_per_block);
    hipLaunchKernelGGL(out16 ? k16 : k32, dim3(grid), dim3(WIN_THREADS), LDS, st, w);
    HMP_LAUNCH_CHECK();
    *any = true;
  }
  if (*any) a = rest;
  return HMP_OK;
}

int agg_fwd_launch(AggArgs& a, hipStream_t st) {
  int Fmax = 0;
  const int vec = 4;
  for (int i = 0; i < a.n; ++i) Fmax = a.d[i].F > Fmax ? a.d[i].F : Fmax;
  if (a.n == 0 || Fmax == 0) return HMP_OK;
  int gs, nv;
  pick_shape(Fmax, vec, gs, nv);
  int64_t rows_total = 0;
  for (int i = 0; i < a.n; ++i) rows_total += a.d[i].n_rows;
  a.xcd = (rows_total >= AGG_XCD_ROWS && agg_xcd_enabled()) ? 1 : 0;
  for (int i = 0; i < a.n; ++i) {
    AggDst& D = a.d[i];
    HMP_CHECK_ARG((D.ldo & 3) == 0 && (D.F & 3) == 0, "agg_fwd: widths must be padded to 4");
    if (a.xcd || a.zb16 || rows_total > 16 * AGG_SMALL_TILES) D.tile_rows = 0;  // (tiles of 8 rows are a small-launch device)
  }
  int blocks = agg_layout_rows(a, gs);
  if (blocks == 0) return HMP_OK;
  if (a.zb16) {  // bf16 projected rows: only the one-wavefront-per-row shape reads them
    HMP_CHECK_ARG(gs == 64 && nv == 1, "agg_fwd: bf16 projected rows need row widths in (128, 256], got %d", Fmax);
    if (agg_win_enabled()) {
      bool any;
      HMP_TRY(agg_win_peel(a, st, &any));
      if (any) {
        if (a.n == 0) return HMP_OK;
        blocks = agg_layout_rows(a, gs);
      }
    }
    sync_bstart(a);
    if (a.hb16) hipLaunchKernelGGL((agg_fwd_kernel<64, 1, true, true>), dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((agg_fwd_kernel<64, 1, true>), dim3(blocks), dim3(256), 0, st, a);
    HMP_LAUNCH_CHECK();
    return HMP_OK;
  }
  HMP_CHECK_ARG(!a.hb16, "agg_fwd: bf16 outputs need bf16 projected rows (the one-wavefront-per-row kernel)");
  sync_bstart(a);
#define LAUNCH_FWD(GS_, NV_) hipLaunchKernelGGL((agg_fwd_kernel<GS_, NV_>), dim3(blocks), dim3(256), 0, st, a)
  HMP_DISPATCH_GS_NV(gs, nv, LAUNCH_FWD)
#undef LAUNCH_FWD
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int agg_proj_fwd_launch(AggArgs& a, hipStream_t st) {
  int Fmax = 0;
  for (int i = 0; i < a.n; ++i) Fmax = a.d[i].F > Fmax ? a.d[i].F : Fmax;
  if (a.n == 0 || Fmax == 0) return HMP_OK;
  HMP_CHECK_ARG(Fmax <= 256, "agg_proj_fwd: row width %d > 256", Fmax);
  for (int i = 0; i < a.n; ++i) {
    const AggDst& D = a.d[i];
    HMP_CHECK_ARG((D.ldo & 3) == 0 && (D.F & 3) == 0, "agg_proj_fwd: widths must be padded to 4");
    if (D.pw)
      HMP_CHECK_ARG((D.pK & 15) == 0 && D.pK <= 256 && D.pK <= D.F && (D.pldw & 3) == 0 && D.pncols > 0,
                    "agg_proj_fwd: projection K %d / ld %d not supported", D.pK, D.pldw);
  }
  const int blocks = agg_layout_tiles(a);
  if (blocks == 0) return HMP_OK;
  sync_bstart(a);
  switch (agg_tile_gs(Fmax)) {
    case 16: hipLaunchKernelGGL((agg_proj_fwd_kernel<16>), dim3(blocks), dim3(256), 0, st, a); break;
    case 32: hipLaunchKernelGGL((agg_proj_fwd_kernel<32>), dim3(blocks), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((agg_proj_fwd_kernel<64>), dim3(blocks), dim3(256), 0, st, a); break;
  }
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

// widest segment or root width of a transposed launch
static int tagg_fmax(const TAggArgs& a) {
  int Fmax = 0;
  for (int i = 0; i < a.n; ++i) {
    for (int o = 0; o < a.s[i].n_out; ++o) Fmax = a.s[i].out[o].F > Fmax ? a.s[i].out[o].F : Fmax;
    if (a.s[i].groot) Fmax = a.s[i].Froot > Fmax ? a.s[i].Froot : Fmax;
  }
  return Fmax;
}

int agg_bwd_launch(TAggArgs& a, hipStream_t st) {
  const int vec = 4;
  int Fmax = tagg_fmax(a);
  if (a.n == 0 || Fmax == 0) {
    if (!a.fin_row_lv) return HMP_OK;
    Fmax = 4;  // nothing to gather, but the loss still has to be finalised
  }
  int gs, nv;
  pick_shape(Fmax, vec, gs, nv);
  int64_t rows_total = 0;
  for (int i = 0; i < a.n; ++i) rows_total += a.s[i].n_rows;
  a.xcd = (rows_total >= AGG_XCD_ROWS && agg_xcd_enabled()) ? 1 : 0;
  for (int i = 0; i < a.n; ++i)
    if (a.xcd || a.gb16 || rows_total > 16 * AGG_SMALL_TILES) a.s[i].tile_rows = 0;  // (tiles of 8 rows are a small-launch device)
  int blocks = agg_layout_rows(a, gs);
  if (blocks == 0 && !a.fin_row_lv) return HMP_OK;
  if (a.gb16) {  // bf16 gradient rows: only the one-wavefront-per-row shape reads them
    HMP_CHECK_ARG(gs == 64 && nv == 1, "agg_bwd: bf16 gradient rows need row widths in (128, 256], got %d", Fmax);
    if (agg_win_enabled()) {
      bool any;
      HMP_TRY(agg_win_peel(a, st, &any));
      if (any) {
        blocks = agg_layout_rows(a, gs);
        if (blocks == 0 && !a.fin_row_lv) return HMP_OK;
      }
    }
    const int grid = blocks + (a.fin_row_lv ? 1 : 0);
    sync_bstart(a);
    if (a.dzb16) hipLaunchKernelGGL((agg_bwd_kernel<64, 1, true, true>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((agg_bwd_kernel<64, 1, true, false>), dim3(grid), dim3(256), 0, st, a);
    HMP_LAUNCH_CHECK();
    return HMP_OK;
  }
  HMP_CHECK_ARG(!a.dzb16, "agg_bwd: a bf16 dz needs bf16 gradient rows (the one-wavefront-per-row kernel)");
  const int grid = blocks + (a.fin_row_lv ? 1 : 0);
  sync_bstart(a);
#define LAUNCH_BWD(GS_, NV_) hipLaunchKernelGGL((agg_bwd_kernel<GS_, NV_>), dim3(grid), dim3(256), 0, st, a)
  HMP_DISPATCH_GS_NV(gs, nv, LAUNCH_BWD)
#undef LAUNCH_BWD
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

int agg_bwd_dx_launch(TAggArgs& a, hipStream_t st) {
  int Fmax = tagg_fmax(a), kmax = 0;
  for (int i = 0; i < a.n; ++i) {
    kmax = a.s[i].ncols > kmax ? a.s[i].ncols : kmax;
    HMP_CHECK_ARG((a.s[i].ncols & 3) == 0, "agg_bwd_dx: ncols must be padded to 4");
    HMP_CHECK_ARG(!a.s[i].xwt || (a.s[i].xldt == ((a.s[i].ncols + 15) & ~15) && a.s[i].xN > 0),
                  "agg_bwd_dx: transposed weights of %d columns with leading dimension %d", a.s[i].ncols, a.s[i].xldt);
  }
  if (a.n == 0 || Fmax == 0) {
    if (!a.fin_row_lv) return HMP_OK;
    Fmax = 4;
  }
  HMP_CHECK_ARG(Fmax <= 256 && kmax <= 896, "agg_bwd_dx: segment width %d / stacked width %d not supported", Fmax, kmax);
  const int blocks = agg_layout_tiles(a);
  if (blocks == 0 && !a.fin_row_lv) return HMP_OK;
  const int grid = blocks + (a.fin_row_lv ? 1 : 0);
  const size_t smem = (size_t)((kmax + 15) & ~15) * 17 * sizeof(float);  // the last k block of 16 is whole (zero rows)
  sync_bstart(a);
  switch (agg_tile_gs(Fmax)) {
    case 16: hipLaunchKernelGGL((agg_bwd_dx_kernel<16>), dim3(grid), dim3(256), smem, st, a); break;
    case 32: hipLaunchKernelGGL((agg_bwd_dx_kernel<32>), dim3(grid), dim3(256), smem, st, a); break;
    default: hipLaunchKernelGGL((agg_bwd_dx_kernel<64>), dim3(grid), dim3(256), smem, st, a); break;
  }
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

template <bool FWD>
static int segment_mean_dispatch(const float* in, int ldi, int F, const hmp_plan& plan, float* out, int ldo, hipStream_t st) {
  const bool vec_ok = ((ldi & 3) == 0) && ((ldo & 3) == 0) && ((reinterpret_cast<uintptr_t>(in) & 15) == 0) &&
                      ((reinterpret_cast<uintptr_t>(out) & 15) == 0) && ((F & 3) == 0);
  const int vec = vec_ok ? 4 : 1;
  const int Fmax = F;
  const int n_rows = FWD ? plan.n_dst : plan.n_src;
  if (n_rows == 0 || F == 0) return HMP_OK;
  int gs, nv;
  pick_shape(F, vec, gs, nv);
  const int blocks = cdiv(n_rows, 256 / gs);
#define LAUNCH_SM(GS_, NV_)                                                                                                   \
  do {                                                                                                                        \
    if (FWD) {                                                                                                                \
      if (vec_ok) hipLaunchKernelGGL((segment_mean_fwd_kernel<GS_, NV_, 4>), dim3(blocks), dim3(256), 0, st, in, ldi, F, plan.d_rowptr, plan.d_col, n_rows, out, ldo); \
      else hipLaunchKernelGGL((segment_mean_fwd_kernel<GS_, NV_, 1>), dim3(blocks), dim3(256), 0, st, in, ldi, F, plan.d_rowptr, plan.d_col, n_rows, out, ldo); \
    } else {                                                                                                                  \
      if (vec_ok) hipLaunchKernelGGL((segment_mean_bwd_kernel<GS_, NV_, 4>), dim3(blocks), dim3(256), 0, st, in, ldi, F, plan.d_t_rowptr, plan.d_t_col, plan.d_rowptr, n_rows, out, ldo); \
      else hipLaunchKernelGGL((segment_mean_bwd_kernel<GS_, NV_, 1>), dim3(blocks), dim3(256), 0, st, in, ldi, F, plan.d_t_rowptr, plan.d_t_col, plan.d_rowptr, n_rows, out, ldo); \
    }                                                                                                                         \
  } while (0)
  HMP_DISPATCH_GS_NV(gs, nv, LAUNCH_SM)
#undef LAUNCH_SM
  HMP_LAUNCH_CHECK();
  return HMP_OK;
}

}  // namespace hmp

extern "C" int hmp_segment_mean_fwd(const float* d_x, int32_t ldx, int32_t F, hmp_plan plan, float* d_out, int32_t ldo, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_x && d_out && plan.d_rowptr, "hmp_segment_mean_fwd: null pointer");
  HMP_CHECK_ARG(F >= 0 && ldx >= F && ldo >= F, "hmp_segment_mean_fwd: bad widths");
  HMP_CHECK_ARG(plan.n_edges == 0 || plan.d_col, "hmp_segment_mean_fwd: null col");
  // widths beyond one pass are processed in column panels
  const int panel = ((ldx & 3) == 0 && (ldo & 3) == 0 && (F & 3) == 0) ? 1024 : 256;
  for (int c = 0; c < F; c += panel) {
    const int w = (F - c) < panel ? (F - c) : panel;
    HMP_TRY((segment_mean_dispatch<true>(d_x + c, ldx, w, plan, d_out + c, ldo, (hipStream_t)stream)));
  }
  return HMP_OK;
}

extern "C" int hmp_segment_mean_bwd(const float* d_gout, int32_t ldg, int32_t F, hmp_plan plan, float* d_gx, int32_t ldgx, void* stream) {
  using namespace hmp;
  HMP_CHECK_ARG(d_gout && d_gx && plan.d_rowptr && plan.d_t_rowptr, "hmp_segment_mean_bwd: null pointer");
  HMP_CHECK_ARG(F >= 0 && ldg >= F && ldgx >= F, "hmp_segment_mean_bwd: bad widths");
  HMP_CHECK_ARG(plan.n_edges == 0 || plan.d_t_col, "hmp_segment_mean_bwd: null t_col");
  const int panel = ((ldg & 3) == 0 && (ldgx & 3) == 0 && (F & 3) == 0) ? 1024 : 256;
  for (int c = 0; c < F; c += panel) {
    const int w = (F - c) < panel ? (F - c) : panel;
    HMP_TRY((segment_mean_dispatch<false>(d_gout + c, ldg, w, plan, d_gx + c, ldgx, (hipStream_t)stream)));
  }
  return HMP_OK;
}
