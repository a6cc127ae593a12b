// Device-side pieces shared by the tiled grouped GEMM kernels: gemm_kernel (gemm.hip, fp32 MFMA), gemm_bf16_kernel (gemm_bf16.hip,
// bf16 compute mode) and gemm_x3_kernel (gemm_x3.hip, fp32 as three bf16 pieces).  A tiled kernel reads as
//     gemm_tile_walk -> gemm_acc_init -> its own K loop -> gemm_epilogue
// and stages its fp32 operands with tile_load_fast / tile_mask on one slot mapping (TileSlots).  All three kernels use the staging
// pair, the slot mapping and gemm_act_mask; the bf16 and x3 kernels the operand fetch, the walk and the epilogue; the bf16 kernel the
// set-up.  gemm_x3_kernel keeps its own set-up and gemm_kernel its own walk, set-up and epilogue: shared, those cost the one scratch
// and the other speed (measured; BASELINE.md, "Shared GEMM tile code", has the register table, the variants tried and the timings).
// A change to one of those pieces here belongs in the kept copies too.  What is NOT shared by design (the bf16-stored loaders, the
// edge loaders, the three LDS stores, the K loops) stays in the kernel's own file.
// Everything is __forceinline__: the kernels sit at the register ceiling, so a change here is to be checked against
// -Rpass-analysis=kernel-resource-usage for every instantiation.
#pragma once
#include "kernels.h"

namespace hmp {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------------
// tile walk
// ---------------------------------------------------------------------------------------------------------------------------
// Which BM x BN output tile and K chunk of which problem blockIdx.x works on (gemm_plan_tiles laid the block ids out): returns the
// problem's index in gb.p and fills the K chunk z (the split-K slab), the tile's first row / column m0 / n0 and the chunk's K range.
// XCD-aware order (blocks b and b+8 share an XCD and its 4 MB L2; speed only, never correctness):
//  * split-K: the K chunk index is the fastest-varying part of the block id, so with ksplit = 8 (or 16) all tiles
//    of one chunk run on one XCD and its A/B panels are fetched into that L2 once;
//  * otherwise row tiles are grouped by 8 and the column tiles of one row tile are 8 block ids apart, so the row
//    panel of A (the big operand: nodes x features) is fetched once per XCD instead of once per column tile.
// (Results through references and in this order of statements: a by-value struct, or z after t, cost gemm_x3_kernel's and
// gemm_bf16_kernel's spilling instantiations scratch -- BASELINE.md, "Shared GEMM tile code".)
template <int BM, int BN>
__device__ __forceinline__ int gemm_tile_walk(const GemmBatch& gb, int& z, int& m0, int& n0, int& kbeg, int& kend) {
  int pi = 0;
  while (pi + 1 < gb.n && (int)blockIdx.x >= gb.p[pi + 1].tile_start) ++pi;
  const GemmProblem& P = gb.p[pi];
  const int local = blockIdx.x - P.tile_start;
  z = local % P.ksplit;
  const int t = local / P.ksplit;
  const int grp = t / (8 * P.tiles_n), within = t % (8 * P.tiles_n);
  const int rows_in_grp = min(8, P.tiles_m - grp * 8);
  m0 = (grp * 8 + within % rows_in_grp) * BM;
  n0 = (within / rows_in_grp) * BN;
  kbeg = z * P.kchunk;
  kend = min(P.K, kbeg + P.kchunk);
  return pi;
}
// The operand layouts follow from FORM in two lines of each kernel, right after the walk:
//     a_kcontig = FORM == 3 ? (P.trans_a ? 0 : 1) : (FORM == 2 ? 0 : 1);   b_kcontig = FORM == 3 ? (P.trans_b ? 1 : 0) : (FORM == 0 ? 1 : 0);
// 1 = [row][k] in memory (k contiguous), 0 = [k][row].  FORM fixes them at compile time (0: NT = x * W^T, 1: NN = dZ * W, 2: TN =
// dZ^T * [x | 1]; 3: per problem at run time): with run-time layouts the layout branch sits inside the unrolled load / LDS-read loops
// and the loads stop overlapping.  (Produced by the walk, or by helpers of their own, in any form tried, the two values cost
// gemm_x3_kernel's run-time-form instantiations 8 and 20 bytes per lane of scratch and gemm_bf16_kernel<ONES, 128, NT> 8.)

// ---------------------------------------------------------------------------------------------------------------------------
// accumulators: D layout of a 32x32 MFMA tile, set-up, epilogue
// ---------------------------------------------------------------------------------------------------------------------------
// A = [i][k] supplies the rows of C, B = [k][j] its columns; register r of lane l holds D[d_row(r, l)][d_col(l)]
__device__ __forceinline__ int d_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ int d_col(int lane) { return lane & 31; }

// d out / d pre for out = dropout(act(pre)) given the stored out value h
__device__ __forceinline__ float gemm_act_mask(float h, int act, bool keep, float scale) {
  if (!keep) return 0.f;
  if (act == HMP_ACT_RELU) return h > 0.f ? scale : 0.f;
  if (act == HMP_ACT_ELU) return h > 0.f ? scale : (h + scale);  // elu'(pre) = elu(pre) + 1 for pre <= 0
  return scale;
}

// The wave's MI x NI accumulator tiles, whose first element is C[row0][col0]: zero, or -- `first` (block-uniform per K group: the
// first K chunk, the first K group) -- the addend, so that the product accumulates ON TOP of it (GemmProblem::Cadd)
template <int MI, int NI>
__device__ __forceinline__ void gemm_acc_init(f32x16 (&acc)[MI][NI], const GemmProblem& P, bool first, int row0, int col0, int lane) {
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  if (P.Cadd && first) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = row0 + 32 * i + d_row(r, lane);
          const int col = col0 + 32 * j + d_col(lane);
          acc[i][j][r] = (row < P.M && col < P.N) ? P.Cadd[(int64_t)row * P.ldadd + col] : 0.f;
        }
  }
}

// Slab z of C <- the wave's accumulator tiles, times the activation-derivative factor of H under EPI_ACTMASK (the forward stored
// dropped elements as -0.0f: the keep bit is the sign of a zero, no RNG replay needed).
//  BF16IO: H and / or C may hold bf16 elements (GemmProblem::h_bf16, c_bf16; block-uniform) -- gemm_bf16_kernel only, the others
//          compile none of it.
//  ONES:   acc1 holds the products against an all-ones operand; column 0 of them is the virtual ones column C[:, n_real], stored
//          by the waves with ones_here.  ONES_EXCL: the tile's own columns >= n_real are then not stored (gemm_x3_kernel, whose
//          loaders mask them to zero; gemm_bf16_kernel's edge loader supplies the ones and it stores them).
// CONTRACT: no branch between memory operations.  The problem's fields live in registers, the 16 activation values of a 32x32 tile
// are requested together at clamped addresses, and the stores are predicated.  Written element by element with a `continue`, the
// compiler waited for every H load before it issued the next one: 128 dependent round trips per thread.  The bf16 forms are hoisted
// for the same reason: no branch between the 16 loads or stores of either form.
template <int MI, int NI, bool BF16IO, bool ONES, bool ONES_EXCL>
__device__ __forceinline__ void gemm_epilogue(const GemmProblem& P, int z, const f32x16 (&acc)[MI][NI], const f32x16* acc1, bool ones_here,
                                              int row0, int col0, int lane) {
  float* C = P.C + (int64_t)z * P.slab_stride;
  const int Mrows = P.M, Ncols = P.N, ldc = P.ldc, ldh = P.ldh, act = P.act;
  const bool amask = P.epi == EPI_ACTMASK;
  const bool dropon = P.drop_on != 0;
  const bool c16 = BF16IO && P.c_bf16 != 0;
  const float dscale = dropon ? P.drop.scale : 1.f;
  const float* Hp = P.H;
  const bool h16 = BF16IO && P.h_bf16 != 0;  // (the sign of zero survives the bf16 store)
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int col = col0 + 32 * j + d_col(lane);
      const int rbase = row0 + 32 * i;
      const bool cok = col < Ncols && !(ONES && ONES_EXCL && P.aug_ones && col >= P.n_real);
      const int colc = col < Ncols ? col : 0;
      float hv[16];
      if (amask && h16) {
        const uint16_t* Hb = reinterpret_cast<const uint16_t*>(Hp);
        uint16_t hb[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rbase + d_row(r, lane);
          hb[r] = Hb[(int64_t)(row < Mrows ? row : Mrows - 1) * ldh + colc];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) hv[r] = __uint_as_float((uint32_t)hb[r] << 16);
      } else if (amask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rbase + d_row(r, lane);
          hv[r] = Hp[(int64_t)(row < Mrows ? row : Mrows - 1) * ldh + colc];
        }
      }
      float vv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[i][j][r];
        if (amask) {
          const bool keep = !dropon || (__float_as_uint(hv[r]) != 0x80000000u);
          v *= gemm_act_mask(hv[r], act, keep, dscale);
        }
        vv[r] = v;
      }
      if (c16) {  // (ldc counts elements)
        __bf16* C16 = reinterpret_cast<__bf16*>(C);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rbase + d_row(r, lane);
          if (cok && row < Mrows) C16[(int64_t)row * ldc + col] = (__bf16)vv[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rbase + d_row(r, lane);
          if (cok && row < Mrows) C[(int64_t)row * ldc + col] = vv[r];
        }
      }
    }
  if constexpr (ONES) {
    if (ones_here && d_col(lane) == 0) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = row0 + 32 * i + d_row(r, lane);
          if (row < P.M) C[(int64_t)row * P.ldc + P.n_real] = acc1[i][r];
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// bf16 MFMA operand fetch
// ---------------------------------------------------------------------------------------------------------------------------
// MFMA operand (8 consecutive k of row `rowbase + lane % 32`, k half lane / 32) of k step ks of a bf16 LDS image.
//  [row][k] image, PITCH elements per row: one 16-byte read.
//  [k][row] image, RP elements per k row: two hardware-transposed reads (ds_read_b64_tr_b16): inside a 16-lane group, lane 4q+p
//  supplies the address of k row q, columns 4p..4p+3 and receives column (lane % 16), 4 k rows.
//  EXEC must be all ones here (no divergence in the main loop).
template <int PITCH, int RP>
__device__ __forceinline__ bf16x8 mfma_fetch_bf16(const __bf16* __restrict__ s, int kcontig, int rowbase, int ks, int lane) {
  if (kcontig) return *reinterpret_cast<const bf16x8*>(s + (rowbase + (lane & 31)) * PITCH + ks * 16 + 8 * (lane >> 5));
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
  const int k0 = ks * 16 + 8 * (g >> 1);
  const __bf16* a0 = s + (k0 + q) * RP + rowbase + 16 * (g & 1) + 4 * p;
  typedef s16x4 __attribute__((address_space(3))) * lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(a0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(a0 + 4 * RP));
  union { s16x4 h[2]; bf16x8 v; } u;
  u.h[0] = lo;
  u.h[1] = hi;
  return u.v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// staging: global -> registers, issue now / mask later
// ---------------------------------------------------------------------------------------------------------------------------
// A (ROWS x BK) stage of one operand in the registers of NT threads, NV float4 slots per thread; logical element (r, k).
//  k-contiguous operand ([r][k] in memory): slot q covers row q / (BK/4), k = 4 (q % (BK/4)) .. + 3        (slot_rk)
//  row-contiguous operand ([k][r] in memory): slot q covers k = q / (ROWS/4), rows 4 (q % (ROWS/4)) .. + 3  (slot_kr)
template <int NV>
struct StageRegs {
  float4 v[NV];
};
template <int NT_, int ROWS_, int BK_>
struct TileSlots {
  static constexpr int NT = NT_, ROWS = ROWS_, BK = BK_;
  static constexpr int NV = ROWS * BK / 4 / NT;
  static __device__ __forceinline__ void slot_rk(int i, int& r, int& k4) {
    const int q = (int)threadIdx.x + i * NT;
    r = q / (BK / 4);
    k4 = (q % (BK / 4)) * 4;
  }
  static __device__ __forceinline__ void slot_kr(int i, int& k, int& r4) {
    const int q = (int)threadIdx.x + i * NT;
    k = q / (ROWS / 4);
    r4 = (q % (ROWS / 4)) * 4;
  }
};

// The fast loader only ISSUES the stage's loads, and with NO control flow between them (a branchy loader makes hipcc drain vmcnt
// between slots, i.e. one load in flight at a time; so does a run-time choice of VEC around the loads -- a join after every
// operand -- which is why VEC is a template argument).  Out-of-range rows / k are CLAMPED to an in-range address; tile_mask zeroes
// what lies outside the operand when the stage is consumed, one iteration later -- a select on a loaded value right here makes the
// compiler wait for the load before the MFMAs it was meant to overlap with.  So any K stage of a k-contiguous operand (also the
// tail stage) takes this path, and any K stage of a row-contiguous operand whose tile width is fully in range; with CLAMP_COLS a
// VEC 1 load of a row-contiguous operand clamps every column into [0, R) too and takes partial tiles (masked with MASK_COLS).
// VEC: 4 = one 16-byte load (ld and the stage's k are multiples of 4, so the vector ends inside the row), 2 = two 8-byte loads
// (rows only 8-byte aligned, e.g. ld = 306: the first pair ends at gkc + 1 <= ld - 1, the second may start at / after kend and
// re-reads the first then), 1 = four scalar loads, every element clamped below kend on its own.
template <class S, int VEC, bool CLAMP_COLS = false>
__device__ __forceinline__ void tile_load_fast(StageRegs<S::NV>& t, const float* __restrict__ p, int ld, int kcontig, int r0, int R, int k0,
                                               int kend) {
#pragma unroll
  for (int i = 0; i < S::NV; ++i) {
    const float* src;
    int o1 = 1, o2 = 2, o3 = 3;  // element offsets (VEC < 4: clamped so that no access leaves the operand)
    if (kcontig) {
      int r, k4;
      S::slot_rk(i, r, k4);
      const int gr = r0 + r, gk = k0 + k4;
      // clamp: row to the last row; k to the start of the stage (always < kend) when the slot starts out of range
      const int gkc = (gk < kend) ? gk : k0;
      src = p + (int64_t)(gr < R ? gr : R - 1) * ld + gkc;
      if (VEC == 1) { o1 = (gkc + 1 < kend) ? 1 : 0; o2 = (gkc + 2 < kend) ? 2 : 0; o3 = (gkc + 3 < kend) ? 3 : 0; }
      if (VEC == 2) { o2 = (gkc + 2 < kend) ? 2 : 0; }
    } else {
      int k, r4;
      S::slot_kr(i, k, r4);
      const int gk = k0 + k, c = r0 + r4;
      const float* row = p + (int64_t)(gk < kend ? gk : k0) * ld;
      if (CLAMP_COLS && VEC == 1) {
        src = row + (c < R ? c : R - 1);
        o1 = (c + 1 < R) ? 1 : 0; o2 = (c + 2 < R) ? 2 : 0; o3 = (c + 3 < R) ? 3 : 0;
        if (c >= R) o1 = o2 = o3 = 0;
      } else {
        src = row + c;  // whole tile inside the operand (the caller's choice of loader)
      }
    }
    if (VEC == 4) {
      t.v[i] = *reinterpret_cast<const float4*>(src);
    } else if (VEC == 2) {
      const float2 a = *reinterpret_cast<const float2*>(src);
      const float2 b = *reinterpret_cast<const float2*>(src + o2);
      t.v[i] = make_float4(a.x, a.y, b.x, b.y);
    } else {
      t.v[i] = make_float4(src[0], src[o1], src[o2], src[o3]);
    }
  }
}

// zeroes what tile_load_fast fetched from clamped addresses.  A row-contiguous operand: whole slots past kend; with MASK_COLS also
// the columns >= R of a partial tile (the CLAMP_COLS loader's counterpart)
template <class S, bool MASK_COLS = false>
__device__ __forceinline__ void tile_mask(StageRegs<S::NV>& t, int kcontig, int r0, int R, int k0, int kend) {
#pragma unroll
  for (int i = 0; i < S::NV; ++i) {
    if (kcontig) {
      int r, k4;
      S::slot_rk(i, r, k4);
      const int gk = k0 + k4;
      const bool rl = r0 + r < R;
      t.v[i] = make_float4(rl && gk + 0 < kend ? t.v[i].x : 0.f, rl && gk + 1 < kend ? t.v[i].y : 0.f, rl && gk + 2 < kend ? t.v[i].z : 0.f,
                           rl && gk + 3 < kend ? t.v[i].w : 0.f);
    } else {
      int k, r4;
      S::slot_kr(i, k, r4);
      if (MASK_COLS) {
        const int c = r0 + r4;
        const bool kl = k0 + k < kend;
        t.v[i] = make_float4(kl && c + 0 < R ? t.v[i].x : 0.f, kl && c + 1 < R ? t.v[i].y : 0.f, kl && c + 2 < R ? t.v[i].z : 0.f,
                             kl && c + 3 < R ? t.v[i].w : 0.f);
      } else if (k0 + k >= kend) {
        t.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }
}

}  // namespace hmp
