// Internal interface of the H-tree builder (htree.cpp) for the other host code of the library: the result record behind the opaque
// hmp_htree of include/hydra_mp.h, and the builder on int32 edge lists, so that the frame pipeline (frame.cpp) hands over the lists
// it has just made without widening them for the C entry.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/hydra_mp.h"

struct hmp_htree {
  int32_t counts[4] = {0, 0, 0, 0};
  std::vector<int32_t> object_orig, room_orig;
  std::vector<int32_t> edges[10];  // [2][n] each: row 0 sources, row 1 destinations (local indices inside the node types)
  std::vector<int32_t> init[3];    // ov_to_or, rv_to_or, rv_to_rr: row 0 = virtual (original index inside its type), row 1 = clique
};

namespace hmp {
// hmp_htree_build on int32 lists [2][e]; same checks, same result, same error text
int htree_build_i32(int32_t n_objects, int32_t n_rooms, const int32_t* oo, int64_t e_oo, const int32_t* rr, int64_t e_rr,
                    const int32_t* ro, int64_t e_ro, hmp_htree** out);
}  // namespace hmp
