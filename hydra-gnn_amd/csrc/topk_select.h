// Top-k selection over the entries of a row held by a group of GS lanes, written once (header-inline, like tail_fns.h):
// gat.hip (gat_attention_kernel: largest head-mean coefficient) and saliency.hip (saliency_topk_kernel: largest |score|).
//
// Every lane keeps the KMAX best (value, key) pairs of the entries it met, sorted descending in the total order "larger value,
// then smaller key"; k rounds of a GS-lane butterfly then pick the group's best head and its owner pops it.  Lane r of the group
// ends up with result r.  Values are >= 0: -1 marks an empty place and INT_MAX its key.
//
// Keys decide ties, so equal keys must mean equal entries: gat.hip passes the CSR slot (unique; a lane meets its slots in
// ascending order, so among equal values the earlier slot stays ahead), saliency.hip the source node (a duplicate edge repeats a
// key: the caller keeps it out of one lane's list with topsel_holds, and lanes that hold the same head pop it together).
#pragma once
#include <climits>

#include "kernels.h"

namespace hmp {

template <int KMAX>
__device__ __forceinline__ void topsel_init(float (&tv)[KMAX], int (&tp)[KMAX]) {
#pragma unroll
  for (int i = 0; i < KMAX; ++i) { tv[i] = -1.f; tp[i] = INT_MAX; }
}

// is key p in the lane's list?
template <int KMAX>
__device__ __forceinline__ bool topsel_holds(const int (&tp)[KMAX], int p) {
  bool h = false;
#pragma unroll
  for (int i = 0; i < KMAX; ++i) h = h || tp[i] == p;
  return h;
}

// sorted insertion of (v, p); the pair pushed off the end is dropped
template <int KMAX>
__device__ __forceinline__ void topsel_insert(float (&tv)[KMAX], int (&tp)[KMAX], float v, int p) {
#pragma unroll
  for (int i = 0; i < KMAX; ++i) {
    if (v > tv[i] || (v == tv[i] && p < tp[i])) {
      const float fv = tv[i];
      const int fp = tp[i];
      tv[i] = v; tp[i] = p;
      v = fv; p = fp;
    }
  }
}

// k rounds over the group's GS lanes (gl = lane index inside the group): afterwards lane r < k holds result r in (rv, rp);
// rp == INT_MAX: the group had fewer than r + 1 entries (rv is -1 then).  Consumes the lists.
template <int GS, int KMAX>
__device__ __forceinline__ void topsel_rounds(float (&tv)[KMAX], int (&tp)[KMAX], int k, int gl, float& rv, int& rp) {
  rv = -1.f;
  rp = INT_MAX;
  for (int r = 0; r < k; ++r) {
    float v = tv[0];
    int p = tp[0];
#pragma unroll
    for (int o = GS / 2; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o);
      const int op = __shfl_xor(p, o);
      if (ov > v || (ov == v && op < p)) { v = ov; p = op; }
    }
    if (tp[0] == p) {  // the owner pops (groups with nothing left all hold the empty mark: popping it changes nothing)
#pragma unroll
      for (int i = 0; i + 1 < KMAX; ++i) { tv[i] = tv[i + 1]; tp[i] = tp[i + 1]; }
      tv[KMAX - 1] = -1.f; tp[KMAX - 1] = INT_MAX;
    }
    if (gl == r) { rv = v; rp = p; }
  }
}

}  // namespace hmp
