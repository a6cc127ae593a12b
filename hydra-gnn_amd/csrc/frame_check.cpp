// The stand-alone driver of the frame pipeline's host stage for `make frame_check` (AddressSanitizer + UBSan, CPU only, nothing
// preloaded): reads flat binary frame files and runs the host entries of include/hydra_mp.h section 14 on them, every output into a
// buffer cut exactly to size.  The first argument selects what is run:
//
//   frame_check [--frames] [--homogeneous] FILE...   every file as saved: hmp_frame_build, _sizes, _host_arrays, _pack, _destroy;
//                                                    `--homogeneous` before a file builds it and every file after it with
//                                                    hmp_frame_build_homogeneous
//   frame_check --batch FILE...                      all files (one configuration) as ONE batch, typed and homogeneous, collated and
//                                                    store form, with a label vector (i % 26) per frame: hmp_frame_batch_build,
//                                                    _items_needed, _sizes, _host_arrays, _pack, _destroy
//   frame_check --htree-relpos FILE...               whatever mode a file was saved with, every file rebuilt as an H-tree with
//                                                    relative_pos = HMP_FRAME_RELPOS_HTREE, typed and homogeneous, then the batch stage
//                                                    over all of them in both forms, then the refusals of the mode
//   frame_check --flags [--no-room-edges] FILE...    every file through hmp_frame_build_flags, typed and homogeneous;
//                                                    `--no-room-edges` before a file sets HMP_FRAME_NO_ROOM_EDGES for it and every file
//                                                    after it (rr must come out 0); one batch per flag value in both forms, and a batch
//                                                    that mixes the flag values must be refused
//
// File (little endian, dsg.save_frame_file): "HMPF", int32 version = 1, int32 n, int32 htree, int32 relative_pos, int32 sem_dim,
// int32 n_labels, int32 clique_dim, int64 m, float64 threshold_near, max_near, max_on, then ids uint64[n], layer int32[n],
// pos / bb_min / bb_max float64[n][3], label int64[n], edges uint64[2][m].  The flags are not part of a file.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hydra_mp.h"

namespace {

struct FrameFile {
  std::string path;
  bool switched = false;  // behind the mode's switch (--homogeneous, --no-room-edges) on the command line
  int32_t h[7];           // version, n, htree, relative_pos, sem_dim, n_labels, clique_dim
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

bool load(FrameFile& F) {
  FILE* f = fopen(F.path.c_str(), "rb");
  if (!f) { fprintf(stderr, "%s: cannot open\n", F.path.c_str()); return false; }
  char magic[4];
  bool ok = fread(magic, 1, 4, f) == 4 && memcmp(magic, "HMPF", 4) == 0 && fread(F.h, 4, 7, f) == 7 && F.h[0] == 1 && fread(&F.m, 8, 1, f) == 1 &&
            fread(F.th, 8, 3, f) == 3 && F.h[1] >= 0 && F.m >= 0;
  const size_t n = ok ? (size_t)F.h[1] : 0;
  ok = ok && read_vec(f, F.ids, n) && read_vec(f, F.layer, n) && read_vec(f, F.pos, 3 * n) && read_vec(f, F.bb_min, 3 * n) &&
       read_vec(f, F.bb_max, 3 * n) && read_vec(f, F.label, n) && read_vec(f, F.edges, 2 * (size_t)F.m);
  fclose(f);
  if (!ok) { fprintf(stderr, "%s: not a frame file\n", F.path.c_str()); return false; }
  F.y.resize(n);
  for (size_t i = 0; i < n; ++i) F.y[i] = (int64_t)(i % 26);
  return true;
}

// how a file is built; flags < 0: through hmp_frame_build / hmp_frame_build_homogeneous, the entries without flags
struct Config {
  bool homogeneous;
  int32_t htree, relative_pos, clique_dim, flags;
};

Config as_saved(const FrameFile& F, bool homogeneous, int32_t flags = -1) { return {homogeneous, F.h[2], F.h[3], F.h[6], flags}; }

int build(const FrameFile& F, const Config& c, hmp_frame** out) {
  if (c.flags >= 0)
    return hmp_frame_build_flags(F.h[1], F.ids.data(), F.layer.data(), F.pos.data(), F.bb_min.data(), F.bb_max.data(), F.label.data(), F.m,
                                 F.edges.data(), F.th[0], F.th[1], F.th[2], c.htree, c.relative_pos, F.h[4], F.h[5], c.clique_dim,
                                 c.homogeneous ? 1 : 0, c.flags, out);
  auto fn = c.homogeneous ? hmp_frame_build_homogeneous : hmp_frame_build;
  return fn(F.h[1], F.ids.data(), F.layer.data(), F.pos.data(), F.bb_min.data(), F.bb_max.data(), F.label.data(), F.m, F.edges.data(), F.th[0],
            F.th[1], F.th[2], c.htree, c.relative_pos, F.h[4], F.h[5], c.clique_dim, out);
}

// One frame: build, sizes, host arrays, pack -> the handle (the caller destroys it), or null after a message.  `counts`: the line
// starts with the host stage's counts.
hmp_frame* check_frame(const FrameFile& F, const Config& c, const std::string& label, bool counts) {
  hmp_frame* fr = nullptr;
  int64_t sz[HMP_FS_COUNT] = {0};
  int rc = build(F, c, &fr);
  if (!rc) rc = hmp_frame_sizes(fr, sz);
  if (!rc) {
    std::vector<int32_t> kept(sz[HMP_FS_KEPT]), obj_room(sz[HMP_FS_KEPT]), dropped(sz[HMP_FS_DROPPED]), rooms(sz[HMP_FS_ROOMS]);
    std::vector<int32_t> rr(2 * sz[HMP_FS_E_RR]), oo(2 * sz[HMP_FS_E_OO]);
    std::vector<double> bb(6 * sz[HMP_FS_ROOMS]);
    rc = hmp_frame_host_arrays(fr, kept.data(), obj_room.data(), dropped.data(), rooms.data(), rr.data(), bb.data(), oo.data());
    std::vector<unsigned char> staging((size_t)sz[HMP_FS_STAGING_BYTES]);  // exactly to size: a write past the block is caught
    if (!rc && sz[HMP_FS_ITEMS] > 0) rc = hmp_frame_pack(fr, staging.data(), (int64_t)staging.size());
  }
  if (rc) fprintf(stderr, "%s: %s\n", label.c_str(), hmp_last_error());
  if (!rc && c.flags > 0 && (c.flags & HMP_FRAME_NO_ROOM_EDGES) && sz[HMP_FS_E_RR] != 0) {
    fprintf(stderr, "%s: %lld room-room edges left\n", label.c_str(), (long long)sz[HMP_FS_E_RR]);
    rc = 1;
  }
  if (rc) {
    if (fr) hmp_frame_destroy(fr);
    return nullptr;
  }
  printf("%s:", label.c_str());
  if (counts)
    printf(" kept %lld dropped %lld rooms %lld oo %lld rr %lld", (long long)sz[HMP_FS_KEPT], (long long)sz[HMP_FS_DROPPED], (long long)sz[HMP_FS_ROOMS],
           (long long)sz[HMP_FS_E_OO], (long long)sz[HMP_FS_E_RR]);
  printf(" items %lld blocks %lld staging %lld arena %lld\n", (long long)sz[HMP_FS_ITEMS], (long long)sz[HMP_FS_BLOCKS],
         (long long)sz[HMP_FS_STAGING_BYTES], (long long)sz[HMP_FS_ARENA_BYTES]);
  return fr;
}

// The batch stage over frames of one configuration, in both forms: build (`y`: a label vector per frame, or null), sizes,
// _items_needed against the batch's item count, host arrays, pack, destroy.
int check_batch(const std::vector<hmp_frame*>& frames, const int64_t* const* y, const std::string& label) {
  for (int form : {HMP_FB_COLLATED, HMP_FB_STORE}) {
    hmp_frame_batch* b = nullptr;
    int64_t sz[HMP_FBS_COUNT] = {0};
    int32_t per_frame = 0, per_batch = 0;
    int rc = hmp_frame_batch_build((int32_t)frames.size(), frames.data(), form, y, &b);
    if (!rc) rc = hmp_frame_batch_sizes(b, sz) || hmp_frame_batch_items_needed(frames[0], form, y ? 1 : 0, &per_frame, &per_batch);
    const size_t G = (size_t)sz[HMP_FBS_GRAPHS];
    if (!rc) {
      std::vector<int32_t> graph_of_frame((size_t)sz[HMP_FBS_FRAMES]);
      std::vector<int64_t> node_ptr((size_t)sz[HMP_FBS_NODE_TYPES] * (G + 1)), edge_ptr((size_t)sz[HMP_FBS_EDGE_TYPES] * (G + 1));
      std::vector<int64_t> tensors((size_t)sz[HMP_FBS_TENSORS] * 4);
      rc = hmp_frame_batch_host_arrays(b, graph_of_frame.data(), node_ptr.data(), edge_ptr.data(), tensors.data());
      std::vector<unsigned char> staging((size_t)sz[HMP_FBS_STAGING_BYTES]);  // exactly to size: a write past the block is caught
      if (!rc && sz[HMP_FBS_ITEMS] > 0) rc = hmp_frame_batch_pack(b, staging.data(), (int64_t)staging.size());
    }
    if (rc) {
      fprintf(stderr, "%s: %s\n", label.c_str(), hmp_last_error());
    } else if (sz[HMP_FBS_ITEMS] != (int64_t)G * per_frame + (G ? per_batch : 0)) {
      fprintf(stderr, "%s: hmp_frame_batch_items_needed says %d per frame + %d, the batch of %zu graphs has %lld items\n", label.c_str(), per_frame,
              per_batch, G, (long long)sz[HMP_FBS_ITEMS]);
      rc = 3;
    }
    if (b) hmp_frame_batch_destroy(b);
    if (rc) return 1;
    printf("%s %s: frames %lld graphs %lld items %lld groups %lld blocks %lld staging %lld arena %lld\n", label.c_str(),
           form == HMP_FB_STORE ? "store" : "collated", (long long)sz[HMP_FBS_FRAMES], (long long)sz[HMP_FBS_GRAPHS], (long long)sz[HMP_FBS_ITEMS],
           (long long)sz[HMP_FBS_GROUPS], (long long)sz[HMP_FBS_BLOCKS], (long long)sz[HMP_FBS_STAGING_BYTES], (long long)sz[HMP_FBS_ARENA_BYTES]);
  }
  return 0;
}

void destroy(std::vector<hmp_frame*>& frames) {
  for (hmp_frame* fr : frames) hmp_frame_destroy(fr);
  frames.clear();
}

int run_frames(const std::vector<FrameFile>& files) {
  for (const FrameFile& F : files) {
    hmp_frame* fr = check_frame(F, as_saved(F, F.switched), F.path + (F.switched ? " (homogeneous)" : ""), true);
    if (!fr) return 1;
    hmp_frame_destroy(fr);
  }
  return 0;
}

// every file in one layout, then the batch stage over all of them with their label vectors; `relpos`: rebuilt as an H-tree with
// relative positions on its edges, one line per frame
int run_batch(const std::vector<FrameFile>& files, bool homogeneous, bool relpos) {
  const std::string layout = homogeneous ? "homogeneous" : "typed";
  std::vector<hmp_frame*> frames;
  std::vector<const int64_t*> y;
  int rc = 0;
  for (size_t i = 0; i < files.size() && !rc; ++i) {
    const FrameFile& F = files[i];
    hmp_frame* fr = nullptr;
    if (relpos) {
      fr = check_frame(F, Config{homogeneous, 1, HMP_FRAME_RELPOS_HTREE, F.h[6], -1}, layout + " frame " + std::to_string(i), false);
      rc = fr == nullptr;
    } else if ((rc = build(F, as_saved(F, homogeneous), &fr)) != 0) {
      fprintf(stderr, "%s: %s\n", F.path.c_str(), hmp_last_error());
    }
    if (rc) break;
    frames.push_back(fr);
    y.push_back(F.y.data());
  }
  if (!rc) rc = check_batch(frames, y.data(), layout);
  if (!rc && relpos) {  // the refusals of the mode leave nothing behind
    hmp_frame* fr = nullptr;
    const FrameFile& F = files[0];
    const bool refused = build(F, Config{homogeneous, 0, HMP_FRAME_RELPOS_HTREE, 0, -1}, &fr) == HMP_E_ARG &&
                         build(F, Config{homogeneous, 1, 1, 6, -1}, &fr) == HMP_E_ARG &&
                         build(F, Config{homogeneous, 1, HMP_FRAME_RELPOS_HTREE, 3, -1}, &fr) == HMP_E_ARG && fr == nullptr;
    if (!refused) { fprintf(stderr, "a refusal of the mode did not hold\n"); rc = 4; }
  }
  destroy(frames);
  return rc ? 1 : 0;
}

int run_flags(const std::vector<FrameFile>& files, bool homogeneous) {
  const std::string layout = homogeneous ? " (homogeneous)" : "";
  std::vector<hmp_frame*> flagged, plain;
  int rc = 0;
  for (const FrameFile& F : files) {
    const int32_t flags = F.switched ? HMP_FRAME_NO_ROOM_EDGES : 0;
    hmp_frame* fr = check_frame(F, as_saved(F, homogeneous, flags), F.path + layout + " flags " + std::to_string(flags), true);
    if (!fr) { rc = 1; break; }
    (flags ? flagged : plain).push_back(fr);
  }
  // the files of a run share their configuration (one batch per flag value: the frames of a batch share their flags)
  if (!rc && !flagged.empty()) rc = check_batch(flagged, nullptr, "batch no-room-edges" + layout);
  if (!rc && !plain.empty()) rc = check_batch(plain, nullptr, "batch" + layout);
  if (!rc && !flagged.empty() && !plain.empty()) {  // mixed flags in one batch are refused, and the refusal leaks nothing
    const hmp_frame* mixed[2] = {flagged[0], plain[0]};
    hmp_frame_batch* b = nullptr;
    if (hmp_frame_batch_build(2, mixed, HMP_FB_COLLATED, nullptr, &b) == HMP_OK) {
      hmp_frame_batch_destroy(b);
      fprintf(stderr, "a batch of frames with different flags was accepted\n");
      rc = 1;
    }
  }
  destroy(flagged);
  destroy(plain);
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  const char* modes[] = {"--frames", "--batch", "--htree-relpos", "--flags"};
  const char* switches[] = {"--homogeneous", nullptr, nullptr, "--no-room-edges"};
  int mode = 0, first = 1;
  for (int k = 0; k < 4 && argc > 1; ++k)
    if (strcmp(argv[1], modes[k]) == 0) { mode = k; first = 2; }
  std::vector<FrameFile> files;
  bool switched = false;
  for (int i = first; i < argc; ++i) {
    if (switches[mode] && strcmp(argv[i], switches[mode]) == 0) { switched = true; continue; }
    files.emplace_back();
    files.back().path = argv[i];
    files.back().switched = switched;
    if (!load(files.back())) return 2;
  }
  if (files.empty()) {
    fprintf(stderr, "usage: %s [--frames] [--homogeneous] FILE... | --batch FILE... | --htree-relpos FILE... | --flags [--no-room-edges] FILE...\n", argv[0]);
    return 2;
  }
  int rc = 0;
  if (mode == 0) {
    rc = run_frames(files);
  } else {
    for (int homogeneous = 0; homogeneous < 2 && !rc; ++homogeneous)
      rc = mode == 3 ? run_flags(files, homogeneous != 0) : run_batch(files, homogeneous != 0, mode == 2);
  }
  if (rc) return rc;
  printf("FRAME-CHECK-OK\n");
  return 0;
}
