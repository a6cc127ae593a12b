// Stand-alone driver of the frame pipeline's host stage for `make frame_check` (AddressSanitizer + UBSan, CPU only): reads flat
// binary frame files and runs hmp_frame_build, hmp_frame_sizes, hmp_frame_host_arrays, hmp_frame_pack and hmp_frame_destroy on each.
// `--homogeneous` before a file builds it (and every file after it) with hmp_frame_build_homogeneous instead.
//
// File (little endian, dsg.save_frame_file): "HMPF", int32 version = 1, int32 n, int32 htree, int32 relative_pos, int32 sem_dim,
// int32 n_labels, int32 clique_dim, int64 m, float64 threshold_near, max_near, max_on, then ids uint64[n], layer int32[n],
// pos / bb_min / bb_max float64[n][3], label int64[n], edges uint64[2][m].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/hydra_mp.h"

namespace {

template <class T>
bool read_vec(FILE* f, std::vector<T>& v, size_t count) {
  v.resize(count);
  return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}

int run(const char* path, bool homogeneous) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "%s: cannot open\n", path); return 2; }
  char magic[4];
  int32_t h[7];
  int64_t m = 0;
  double th[3];
  bool ok = fread(magic, 1, 4, f) == 4 && memcmp(magic, "HMPF", 4) == 0 && fread(h, 4, 7, f) == 7 && h[0] == 1 && fread(&m, 8, 1, f) == 1 &&
            fread(th, 8, 3, f) == 3 && h[1] >= 0 && m >= 0;
  std::vector<uint64_t> ids, edges;
  std::vector<int32_t> layer;
  std::vector<double> pos, bb_min, bb_max;
  std::vector<int64_t> label;
  const size_t n = ok ? (size_t)h[1] : 0;
  ok = ok && read_vec(f, ids, n) && read_vec(f, layer, n) && read_vec(f, pos, 3 * n) && read_vec(f, bb_min, 3 * n) &&
       read_vec(f, bb_max, 3 * n) && read_vec(f, label, n) && read_vec(f, edges, 2 * (size_t)m);
  fclose(f);
  if (!ok) { fprintf(stderr, "%s: not a frame file\n", path); return 2; }
  hmp_frame* fr = nullptr;
  auto build = homogeneous ? hmp_frame_build_homogeneous : hmp_frame_build;
  if (build((int32_t)n, ids.data(), layer.data(), pos.data(), bb_min.data(), bb_max.data(), label.data(), m, edges.data(), th[0], th[1], th[2],
            h[2], h[3], h[4], h[5], h[6], &fr) != HMP_OK) {
    fprintf(stderr, "%s: %s\n", path, hmp_last_error());
    return 1;
  }
  int64_t sz[HMP_FS_COUNT];
  int rc = hmp_frame_sizes(fr, sz);
  std::vector<int32_t> kept(sz[HMP_FS_KEPT]), obj_room(sz[HMP_FS_KEPT]), dropped(sz[HMP_FS_DROPPED]), rooms(sz[HMP_FS_ROOMS]);
  std::vector<int32_t> rr(2 * sz[HMP_FS_E_RR]), oo(2 * sz[HMP_FS_E_OO]);
  std::vector<double> bb(6 * sz[HMP_FS_ROOMS]);
  rc = rc || hmp_frame_host_arrays(fr, kept.data(), obj_room.data(), dropped.data(), rooms.data(), rr.data(), bb.data(), oo.data());
  std::vector<unsigned char> staging((size_t)sz[HMP_FS_STAGING_BYTES]);  // exactly to size: a write past the block is caught
  if (sz[HMP_FS_ITEMS] > 0) rc = rc || hmp_frame_pack(fr, staging.data(), (int64_t)staging.size());
  hmp_frame_destroy(fr);
  if (rc) { fprintf(stderr, "%s: %s\n", path, hmp_last_error()); return 1; }
  printf("%s%s: kept %lld dropped %lld rooms %lld oo %lld rr %lld items %lld blocks %lld staging %lld arena %lld\n", path,
         homogeneous ? " (homogeneous)" : "", (long long)sz[HMP_FS_KEPT], (long long)sz[HMP_FS_DROPPED], (long long)sz[HMP_FS_ROOMS], (long long)sz[HMP_FS_E_OO], (long long)sz[HMP_FS_E_RR],
         (long long)sz[HMP_FS_ITEMS], (long long)sz[HMP_FS_BLOCKS], (long long)sz[HMP_FS_STAGING_BYTES], (long long)sz[HMP_FS_ARENA_BYTES]);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s [--homogeneous] FRAME_FILE...\n", argv[0]); return 2; }
  bool homogeneous = false;
  for (int i = 1; i < argc; ++i) {
    if (strcmp(argv[i], "--homogeneous") == 0) { homogeneous = true; continue; }
    const int rc = run(argv[i], homogeneous);
    if (rc) return rc;
  }
  printf("FRAME-CHECK-OK\n");
  return 0;
}
