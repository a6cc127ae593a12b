// Stand-alone driver of the frame-batch host stage for `make frame_batch_check` (AddressSanitizer + UBSan, CPU only): reads flat
// binary frame files (dsg.save_frame_file; layout in frame_check.cpp), which must share one configuration, and runs
// hmp_frame_build / hmp_frame_build_homogeneous on each, then hmp_frame_batch_build (with a label vector per frame),
// hmp_frame_batch_items_needed, hmp_frame_batch_sizes, hmp_frame_batch_host_arrays, hmp_frame_batch_pack and the destroys, for both
// layouts and both forms.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/hydra_mp.h"

namespace {

struct FrameFile {
  int32_t h[7];  // version, n, htree, relative_pos, sem_dim, n_labels, clique_dim
  int64_t m = 0;
  double th[3];
  std::vector<uint64_t> ids, edges;
  std::vector<int32_t> layer;
  std::vector<double> pos, bb_min, bb_max;
  std::vector<int64_t> label, y;
};

template <class T>
bool read_vec(FILE* f, std::vector<T>& v, size_t count) {
  v.resize(count);
  return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}

bool load(const char* path, FrameFile& F) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "%s: cannot open\n", path); return false; }
  char magic[4];
  bool ok = fread(magic, 1, 4, f) == 4 && memcmp(magic, "HMPF", 4) == 0 && fread(F.h, 4, 7, f) == 7 && F.h[0] == 1 && fread(&F.m, 8, 1, f) == 1 &&
            fread(F.th, 8, 3, f) == 3 && F.h[1] >= 0 && F.m >= 0;
  const size_t n = ok ? (size_t)F.h[1] : 0;
  ok = ok && read_vec(f, F.ids, n) && read_vec(f, F.layer, n) && read_vec(f, F.pos, 3 * n) && read_vec(f, F.bb_min, 3 * n) &&
       read_vec(f, F.bb_max, 3 * n) && read_vec(f, F.label, n) && read_vec(f, F.edges, 2 * (size_t)F.m);
  fclose(f);
  if (!ok) { fprintf(stderr, "%s: not a frame file\n", path); return false; }
  F.y.resize(n);
  for (size_t i = 0; i < n; ++i) F.y[i] = (int64_t)(i % 26);
  return true;
}

int run(const std::vector<FrameFile>& files, bool homogeneous, int form) {
  std::vector<hmp_frame*> frames;
  std::vector<const int64_t*> y;
  auto build = homogeneous ? hmp_frame_build_homogeneous : hmp_frame_build;
  int rc = 0;
  for (const FrameFile& F : files) {
    hmp_frame* fr = nullptr;
    rc = build(F.h[1], F.ids.data(), F.layer.data(), F.pos.data(), F.bb_min.data(), F.bb_max.data(), F.label.data(), F.m, F.edges.data(), F.th[0],
               F.th[1], F.th[2], F.h[2], F.h[3], F.h[4], F.h[5], F.h[6], &fr);
    if (rc) break;
    frames.push_back(fr);
    y.push_back(F.y.data());
  }
  hmp_frame_batch* b = nullptr;
  rc = rc || hmp_frame_batch_build((int32_t)frames.size(), frames.data(), form, y.data(), &b);
  int64_t sz[HMP_FBS_COUNT] = {0};
  int32_t per_frame = 0, per_batch = 0;
  if (!rc) rc = hmp_frame_batch_sizes(b, sz) || hmp_frame_batch_items_needed(frames[0], form, 1, &per_frame, &per_batch);
  if (!rc) {
    const size_t G = (size_t)sz[HMP_FBS_GRAPHS];
    std::vector<int32_t> graph_of_frame((size_t)sz[HMP_FBS_FRAMES]);
    std::vector<int64_t> node_ptr((size_t)sz[HMP_FBS_NODE_TYPES] * (G + 1)), edge_ptr((size_t)sz[HMP_FBS_EDGE_TYPES] * (G + 1));
    std::vector<int64_t> tensors((size_t)sz[HMP_FBS_TENSORS] * 4);
    rc = hmp_frame_batch_host_arrays(b, graph_of_frame.data(), node_ptr.data(), edge_ptr.data(), tensors.data());
    std::vector<unsigned char> staging((size_t)sz[HMP_FBS_STAGING_BYTES]);  // exactly to size: a write past the block is caught
    if (!rc && sz[HMP_FBS_ITEMS] > 0) rc = hmp_frame_batch_pack(b, staging.data(), (int64_t)staging.size());
    if (!rc && sz[HMP_FBS_ITEMS] != (int64_t)G * per_frame + (G ? per_batch : 0)) {
      fprintf(stderr, "hmp_frame_batch_items_needed says %d per frame + %d, the batch of %zu graphs has %lld items\n", per_frame, per_batch, G,
              (long long)sz[HMP_FBS_ITEMS]);
      rc = 3;
    }
  }
  hmp_frame_batch_destroy(b);
  for (hmp_frame* fr : frames) hmp_frame_destroy(fr);
  if (rc) { fprintf(stderr, "%s\n", hmp_last_error()); return 1; }
  printf("%s %s: frames %lld graphs %lld items %lld groups %lld blocks %lld staging %lld arena %lld\n", homogeneous ? "homogeneous" : "typed",
         form == HMP_FB_STORE ? "store" : "collated", (long long)sz[HMP_FBS_FRAMES], (long long)sz[HMP_FBS_GRAPHS], (long long)sz[HMP_FBS_ITEMS],
         (long long)sz[HMP_FBS_GROUPS], (long long)sz[HMP_FBS_BLOCKS], (long long)sz[HMP_FBS_STAGING_BYTES], (long long)sz[HMP_FBS_ARENA_BYTES]);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s FRAME_FILE...\n", argv[0]); return 2; }
  std::vector<FrameFile> files(argc - 1);
  for (int i = 1; i < argc; ++i)
    if (!load(argv[i], files[i - 1])) return 2;
  for (int homogeneous = 0; homogeneous < 2; ++homogeneous)
    for (int form : {HMP_FB_COLLATED, HMP_FB_STORE}) {
      const int rc = run(files, homogeneous != 0, form);
      if (rc) return rc;
    }
  printf("FRAME-BATCH-CHECK-OK\n");
  return 0;
}
