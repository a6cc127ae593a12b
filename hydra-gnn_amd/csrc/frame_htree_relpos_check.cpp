// Stand-alone driver of the frame host stage and the frame-batch host stage with relative positions on H-tree edges
// (relative_pos = HMP_FRAME_RELPOS_HTREE) for `make frame_htree_relpos_check` (AddressSanitizer + UBSan, CPU only): reads flat binary
// frame files (dsg.save_frame_file; layout in frame_check.cpp) and, whatever mode a file was saved with, builds every frame as an
// H-tree in the new mode, typed and homogeneous: hmp_frame_build / hmp_frame_build_homogeneous, hmp_frame_sizes, hmp_frame_pack
// into a buffer cut to size; then hmp_frame_batch_build over all frames (with a label vector per frame), _items_needed, _sizes,
// _host_arrays and _pack in both forms; and the refusals of the mode.
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

int build(const FrameFile& F, bool homogeneous, int htree, int relative_pos, int clique_dim, hmp_frame** out) {
  auto fn = homogeneous ? hmp_frame_build_homogeneous : hmp_frame_build;
  return fn(F.h[1], F.ids.data(), F.layer.data(), F.pos.data(), F.bb_min.data(), F.bb_max.data(), F.label.data(), F.m, F.edges.data(), F.th[0],
            F.th[1], F.th[2], htree, relative_pos, F.h[4], F.h[5], clique_dim, out);
}

int run(const std::vector<FrameFile>& files, bool homogeneous) {
  const char* layout = homogeneous ? "homogeneous" : "typed";
  std::vector<hmp_frame*> frames;
  std::vector<const int64_t*> y;
  int rc = 0;
  for (size_t i = 0; i < files.size() && !rc; ++i) {
    const FrameFile& F = files[i];
    hmp_frame* fr = nullptr;
    rc = build(F, homogeneous, 1, HMP_FRAME_RELPOS_HTREE, F.h[6], &fr);
    if (rc) break;
    frames.push_back(fr);
    y.push_back(F.y.data());
    int64_t sz[HMP_FS_COUNT];
    rc = hmp_frame_sizes(fr, sz);
    std::vector<unsigned char> staging(rc ? 0 : (size_t)sz[HMP_FS_STAGING_BYTES]);  // exactly to size: a write past the block is caught
    if (!rc && sz[HMP_FS_ITEMS] > 0) rc = hmp_frame_pack(fr, staging.data(), (int64_t)staging.size());
    if (!rc) printf("%s frame %zu: items %lld blocks %lld staging %lld arena %lld\n", layout, i, (long long)sz[HMP_FS_ITEMS], (long long)sz[HMP_FS_BLOCKS],
                    (long long)sz[HMP_FS_STAGING_BYTES], (long long)sz[HMP_FS_ARENA_BYTES]);
  }
  for (int form : {HMP_FB_COLLATED, HMP_FB_STORE}) {
    if (rc) break;
    hmp_frame_batch* b = nullptr;
    rc = hmp_frame_batch_build((int32_t)frames.size(), frames.data(), form, y.data(), &b);
    int64_t sz[HMP_FBS_COUNT] = {0};
    int32_t per_frame = 0, per_batch = 0;
    if (!rc) rc = hmp_frame_batch_sizes(b, sz) || hmp_frame_batch_items_needed(frames[0], form, 1, &per_frame, &per_batch);
    if (!rc) {
      const size_t G = (size_t)sz[HMP_FBS_GRAPHS];
      std::vector<int32_t> graph_of_frame((size_t)sz[HMP_FBS_FRAMES]);
      std::vector<int64_t> node_ptr((size_t)sz[HMP_FBS_NODE_TYPES] * (G + 1)), edge_ptr((size_t)sz[HMP_FBS_EDGE_TYPES] * (G + 1));
      std::vector<int64_t> tensors((size_t)sz[HMP_FBS_TENSORS] * 4);
      rc = hmp_frame_batch_host_arrays(b, graph_of_frame.data(), node_ptr.data(), edge_ptr.data(), tensors.data());
      std::vector<unsigned char> staging((size_t)sz[HMP_FBS_STAGING_BYTES]);
      if (!rc && sz[HMP_FBS_ITEMS] > 0) rc = hmp_frame_batch_pack(b, staging.data(), (int64_t)staging.size());
      if (!rc && sz[HMP_FBS_ITEMS] != (int64_t)G * per_frame + (G ? per_batch : 0)) {
        fprintf(stderr, "hmp_frame_batch_items_needed says %d per frame + %d, the batch of %zu graphs has %lld items\n", per_frame, per_batch, G,
                (long long)sz[HMP_FBS_ITEMS]);
        rc = 3;
      }
    }
    hmp_frame_batch_destroy(b);
    if (!rc) printf("%s %s: frames %lld graphs %lld items %lld groups %lld blocks %lld staging %lld arena %lld\n", layout,
                    form == HMP_FB_STORE ? "store" : "collated", (long long)sz[HMP_FBS_FRAMES], (long long)sz[HMP_FBS_GRAPHS], (long long)sz[HMP_FBS_ITEMS],
                    (long long)sz[HMP_FBS_GROUPS], (long long)sz[HMP_FBS_BLOCKS], (long long)sz[HMP_FBS_STAGING_BYTES], (long long)sz[HMP_FBS_ARENA_BYTES]);
  }
  // the refusals of the mode leave nothing behind
  if (!rc && !files.empty()) {
    hmp_frame* fr = nullptr;
    const bool refused = build(files[0], homogeneous, 0, HMP_FRAME_RELPOS_HTREE, 0, &fr) == HMP_E_ARG && build(files[0], homogeneous, 1, 1, 6, &fr) == HMP_E_ARG &&
                         build(files[0], homogeneous, 1, HMP_FRAME_RELPOS_HTREE, 3, &fr) == HMP_E_ARG && fr == nullptr;
    if (!refused) { fprintf(stderr, "a refusal of the mode did not hold\n"); rc = 4; }
  }
  for (hmp_frame* fr : frames) hmp_frame_destroy(fr);
  if (rc) { fprintf(stderr, "%s\n", hmp_last_error()); return 1; }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s FRAME_FILE...\n", argv[0]); return 2; }
  std::vector<FrameFile> files(argc - 1);
  for (int i = 1; i < argc; ++i)
    if (!load(argv[i], files[i - 1])) return 2;
  for (int homogeneous = 0; homogeneous < 2; ++homogeneous) {
    const int rc = run(files, homogeneous != 0);
    if (rc) return rc;
  }
  printf("FRAME-HTREE-RELPOS-CHECK-OK\n");
  return 0;
}
