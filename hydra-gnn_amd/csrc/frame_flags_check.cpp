// Stand-alone driver of hmp_frame_build_flags for `make frame_flags_check` (AddressSanitizer + UBSan, CPU only): reads the flat binary
// frame files of frame_check.cpp (the HMPF layout is unchanged: the flag is not part of a file) and builds every file typed and
// homogeneous with the flags given on the command line, then sizes, host arrays, pack, the batch stage over all of them in both forms,
// and destroy.  `--no-room-edges` before a file sets HMP_FRAME_NO_ROOM_EDGES for it and every file after it (the room layer loses its
// edges in the host stage: rr must come out 0); without it the flags are 0 and the entry must do what hmp_frame_build does.
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

int fail(const char* path) {
  fprintf(stderr, "%s: %s\n", path, hmp_last_error());
  return 1;
}

// one file, one layout -> the built frame (the caller destroys it), after sizes / host arrays / pack
int run(const char* path, bool homogeneous, int32_t flags, hmp_frame** out) {
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
  if (hmp_frame_build_flags((int32_t)n, ids.data(), layer.data(), pos.data(), bb_min.data(), bb_max.data(), label.data(), m, edges.data(), th[0],
                            th[1], th[2], h[2], h[3], h[4], h[5], h[6], homogeneous ? 1 : 0, flags, &fr) != HMP_OK)
    return fail(path);
  int64_t sz[HMP_FS_COUNT];
  int rc = hmp_frame_sizes(fr, sz);
  std::vector<int32_t> kept(sz[HMP_FS_KEPT]), obj_room(sz[HMP_FS_KEPT]), dropped(sz[HMP_FS_DROPPED]), rooms(sz[HMP_FS_ROOMS]);
  std::vector<int32_t> rr(2 * sz[HMP_FS_E_RR]), oo(2 * sz[HMP_FS_E_OO]);
  std::vector<double> bb(6 * sz[HMP_FS_ROOMS]);
  rc = rc || hmp_frame_host_arrays(fr, kept.data(), obj_room.data(), dropped.data(), rooms.data(), rr.data(), bb.data(), oo.data());
  std::vector<unsigned char> staging((size_t)sz[HMP_FS_STAGING_BYTES]);  // exactly to size: a write past the block is caught
  if (sz[HMP_FS_ITEMS] > 0) rc = rc || hmp_frame_pack(fr, staging.data(), (int64_t)staging.size());
  if (rc) { hmp_frame_destroy(fr); return fail(path); }
  if ((flags & HMP_FRAME_NO_ROOM_EDGES) && sz[HMP_FS_E_RR] != 0) {
    hmp_frame_destroy(fr);
    fprintf(stderr, "%s: %lld room-room edges left\n", path, (long long)sz[HMP_FS_E_RR]);
    return 1;
  }
  printf("%s%s flags %d: kept %lld dropped %lld rooms %lld oo %lld rr %lld items %lld blocks %lld staging %lld arena %lld\n", path,
         homogeneous ? " (homogeneous)" : "", (int)flags, (long long)sz[HMP_FS_KEPT], (long long)sz[HMP_FS_DROPPED], (long long)sz[HMP_FS_ROOMS],
         (long long)sz[HMP_FS_E_OO], (long long)sz[HMP_FS_E_RR], (long long)sz[HMP_FS_ITEMS], (long long)sz[HMP_FS_BLOCKS],
         (long long)sz[HMP_FS_STAGING_BYTES], (long long)sz[HMP_FS_ARENA_BYTES]);
  *out = fr;
  return 0;
}

// the batch stage over frames of one configuration, both forms
int run_batch(std::vector<hmp_frame*>& frames, const char* what) {
  for (int form : {HMP_FB_COLLATED, HMP_FB_STORE}) {
    hmp_frame_batch* b = nullptr;
    if (hmp_frame_batch_build((int32_t)frames.size(), frames.data(), form, nullptr, &b) != HMP_OK) return fail(what);
    int64_t sz[HMP_FBS_COUNT];
    int rc = hmp_frame_batch_sizes(b, sz);
    std::vector<int32_t> graph_of((size_t)sz[HMP_FBS_FRAMES]);
    std::vector<int64_t> node_ptr((size_t)(sz[HMP_FBS_NODE_TYPES] * (sz[HMP_FBS_GRAPHS] + 1))), edge_ptr((size_t)(sz[HMP_FBS_EDGE_TYPES] * (sz[HMP_FBS_GRAPHS] + 1)));
    std::vector<int64_t> tensors((size_t)(4 * sz[HMP_FBS_TENSORS]));
    rc = rc || hmp_frame_batch_host_arrays(b, graph_of.data(), node_ptr.data(), edge_ptr.data(), tensors.data());
    std::vector<unsigned char> staging((size_t)sz[HMP_FBS_STAGING_BYTES]);
    if (sz[HMP_FBS_ITEMS] > 0) rc = rc || hmp_frame_batch_pack(b, staging.data(), (int64_t)staging.size());
    hmp_frame_batch_destroy(b);
    if (rc) return fail(what);
    printf("%s form %d: graphs %lld items %lld staging %lld\n", what, form, (long long)sz[HMP_FBS_GRAPHS], (long long)sz[HMP_FBS_ITEMS],
           (long long)sz[HMP_FBS_STAGING_BYTES]);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s [--no-room-edges] FRAME_FILE...\n", argv[0]); return 2; }
  int rc = 0;
  for (int homogeneous = 0; homogeneous < 2 && !rc; ++homogeneous) {
    int32_t flags = 0;
    std::vector<hmp_frame*> flagged, plain;
    for (int i = 1; i < argc && !rc; ++i) {
      if (strcmp(argv[i], "--no-room-edges") == 0) { flags = HMP_FRAME_NO_ROOM_EDGES; continue; }
      hmp_frame* fr = nullptr;
      rc = run(argv[i], homogeneous != 0, flags, &fr);
      if (!rc) (flags ? flagged : plain).push_back(fr);
    }
    // the files of a run share their configuration (one batch per flag value: the frames of a batch share their flags)
    if (!rc && !flagged.empty()) rc = run_batch(flagged, homogeneous ? "batch no-room-edges (homogeneous)" : "batch no-room-edges");
    if (!rc && !plain.empty()) rc = run_batch(plain, homogeneous ? "batch (homogeneous)" : "batch");
    if (!rc && !flagged.empty() && !plain.empty()) {  // mixed flags in one batch are refused, and the refusal leaks nothing
      std::vector<hmp_frame*> mixed = {flagged[0], plain[0]};
      hmp_frame_batch* b = nullptr;
      if (hmp_frame_batch_build(2, mixed.data(), HMP_FB_COLLATED, nullptr, &b) == HMP_OK) {
        hmp_frame_batch_destroy(b);
        fprintf(stderr, "a batch of frames with different flags was accepted\n");
        rc = 1;
      }
    }
    for (hmp_frame* f : flagged) hmp_frame_destroy(f);
    for (hmp_frame* f : plain) hmp_frame_destroy(f);
  }
  if (rc) return rc;
  printf("FRAME-FLAGS-CHECK-OK\n");
  return 0;
}
