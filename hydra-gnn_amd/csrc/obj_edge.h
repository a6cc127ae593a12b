// The pairwise geometric predicates of the reference's add_object_connectivity (src/hydra_gnn/preprocess_dsgs.py:89-180), written
// once for the device kernels of dsg.hip and the host stage of frame.cpp.  All arithmetic is the reference's, in float64 like numpy,
// without contraction, so both sides give the reference's edge SET bit for bit (tests/golden/dsg_x8F5xyUWy9e_expected.npz).
//
// Everything after this header in a translation unit is compiled without contraction (clang); a g++ build of the host stage
// passes -ffp-contract=off instead.
#pragma once
#include <math.h>

#if defined(__HIP__)
#define HMP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HMP_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#define HMP_UNROLL _Pragma("unroll")
#else
#define HMP_UNROLL
#endif

namespace hmp {

struct ObjGeom {
  const double* pos;   // [n][3]
  const double* size;  // [n][3]  bounding_box.max - bounding_box.min
  const int* room;     // [n]     room index, < 0: no room
  int n;
  double threshold_near, max_near, max_on;
};

HMP_HD bool obj_edge(const ObjGeom& g, int i, int j) {
  if (g.room[i] < 0 || g.room[i] != g.room[j]) return false;
  double p1[3], p2[3], s1[3], s2[3];
  HMP_UNROLL
  for (int k = 0; k < 3; ++k) {
    p1[k] = g.pos[3 * i + k]; p2[k] = g.pos[3 * j + k];
    s1[k] = g.size[3 * i + k]; s2[k] = g.size[3 * j + k];
  }
  const double dx = fabs(p1[0] - p2[0]), dy = fabs(p1[1] - p2[1]), dz = fabs(p1[2] - p2[2]);
  const bool in2 = dx <= s2[0] / 2 && dy <= s2[1] / 2;  // centre of 1 inside 2 on the xy plane
  const bool in1 = dx <= s1[0] / 2 && dy <= s1[1] / 2;
  // _is_on (:89-110)
  const bool above = p1[2] > p2[2];
  const double on_thresh = g.max_on + (s1[2] + s2[2]) / 2;
  const bool is_on = (in2 && above && dz <= on_thresh) || (in1 && !above && dz <= on_thresh);
  // _is_under (:139-158)
  const bool is_under = (in1 || in2) && (p1[2] < p2[2] || p2[2] < p1[2]);
  // _is_near (:161-180)
  bool is_near = true;
  const double d[3] = {dx, dy, dz};
  HMP_UNROLL
  for (int k = 0; k < 3; ++k) {
    const double avg = (s1[k] + s2[k]) / 2.0;
    is_near = is_near && d[k] <= avg * g.threshold_near && d[k] - avg <= g.max_near;
  }
  return is_on || is_under || is_near;
}

}  // namespace hmp
