// The dropout generator's host side (csrc/common.h drop_thresh, drop_pair, drop_keep4) printed for given coordinates, so that a
// restatement of the generator (tests/_dropout_reference.py, written from include/hydra_mp.h) can be compared with this code bit for
// bit without a GPU.
//
//   make -C hydra-gnn_amd/csrc drop_check && hydra-gnn_amd/csrc/build/drop_check
//
// A request is six or seven fields separated by blanks:
//     SEED STEP STREAM PBITS Q0 N [w]
// SEED a 64-bit, STEP / STREAM / Q0 32-bit unsigned decimal numbers, PBITS the bit pattern of the float p as 8 hex digits (the C
// entries take a float: this passes one exactly), N <= 2^20 the number of consecutive quads Q0, Q0 + 1, ... (the counter wraps at
// 2^32 as the kernels' does).  The answer is
//     thresh T              T = drop_thresh(p), decimal
//     keep HHHH...          N hex digits: digit i holds drop_keep4's flags of quad Q0 + i, element j in bit j
//     words AAAAAAAABBBBBBBB...   only with the seventh field: drop_pair's words a, b of each quad, 8 hex digits each
// `drop_check -` answers the requests on stdin, one per line; `drop_check REQUEST...` answers its arguments (one request per
// argument); without arguments it answers a built-in list (seeds below and above 2^32, the largest step, stream and quad numbers,
// thresholds 0, 1 and 65535) -- the run `make drop_check` is for.  A request that does not parse ends the program with status 2.
// The target builds under AddressSanitizer + UBSan; `make drop_check_plain` builds build/drop_check_plain without
// (tests/test_dropout_reference.py).
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../hydra-gnn_amd/csrc/common.h"

using namespace hmp;

namespace {

constexpr uint32_t N_MAX = 1u << 20;

bool answer(const char* req) {
  uint64_t seed;
  uint32_t step, stream, pbits, q0, n;
  char w[4] = {0, 0, 0, 0};
  const int got = sscanf(req, "%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNx32 " %" SCNu32 " %" SCNu32 " %3s", &seed, &step, &stream,
                         &pbits, &q0, &n, w);
  if (got < 6 || n > N_MAX || (got == 7 && strcmp(w, "w") != 0)) {
    fprintf(stderr, "drop_check: bad request '%s'\n", req);
    return false;
  }
  float p;
  memcpy(&p, &pbits, 4);
  DropCfg cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.k0 = (uint32_t)seed; cfg.k1 = (uint32_t)(seed >> 32);  // as every C entry splits its seed
  cfg.step = step; cfg.stream = stream;
  cfg.thresh = drop_thresh(p); cfg.scale = 1.f;
  cfg.step_dev = nullptr;

  std::string keep((size_t)n, '0'), words;
  if (got == 7) words.resize((size_t)n * 16);
  static const char hex[] = "0123456789abcdef";
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t q = q0 + i;  // wraps
    bool k[4];
    drop_keep4(cfg, q, k);
    keep[i] = hex[(k[0] ? 1 : 0) | (k[1] ? 2 : 0) | (k[2] ? 4 : 0) | (k[3] ? 8 : 0)];
    if (got == 7) {
      uint32_t a, b;
      drop_pair(cfg, q, a, b);
      char buf[17];
      snprintf(buf, sizeof(buf), "%08" PRIx32 "%08" PRIx32, a, b);
      memcpy(&words[(size_t)i * 16], buf, 16);
    }
  }
  printf("thresh %" PRIu32 "\nkeep %s\n", cfg.thresh, keep.c_str());
  if (got == 7) printf("words %s\n", words.c_str());
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "-") == 0) {
    std::vector<char> line(256);
    while (fgets(line.data(), (int)line.size(), stdin)) {
      if (line[0] == '\n' || line[0] == 0) continue;
      if (!strchr(line.data(), '\n') && !feof(stdin)) {
        fprintf(stderr, "drop_check: request longer than %zu characters\n", line.size() - 2);
        return 2;
      }
      if (!answer(line.data())) return 2;
    }
    return 0;
  }
  if (argc > 1) {
    for (int i = 1; i < argc; ++i)
      if (!answer(argv[i])) return 2;
    return 0;
  }
  // p = 0, 2^-16, 0.25 and the float below 1
  static const char* const builtin[] = {
      "0 0 0 00000000 0 16 w",
      "1234 1 3 3e800000 0 16 w",
      "4294967296 1 3 3e800000 0 16 w",
      "18446744073709551615 4294967295 4294967295 3f7fffff 4294967288 16 w",
      "2305843009213693957 7 71 37800000 4294967295 64",
  };
  for (const char* r : builtin) {
    printf("request %s\n", r);
    if (!answer(r)) return 2;
  }
  printf("drop_check OK\n");
  return 0;
}
