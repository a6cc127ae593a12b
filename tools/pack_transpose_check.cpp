// Host-side check of the pack's transposed destination (PackSeg::dst_t / ld_dst_t / col_t / pad_t, csrc/device_fns.h pack_lane).
//
//   make -C hydra-gnn_amd/csrc pack_transpose_check && hydra-gnn_amd/csrc/build/pack_transpose_check
//
// Builds, the way build_tables() in net.hip does, the PACK_SUM segments of one SAGE layer with two node types on the CPU,
// runs pack_lane over every (item, lane) the pack kernels would start -- the idle items of the last block included -- under
// AddressSanitizer + UBSan, and compares the transposed image with a plain transpose of the packed weights whose columns are then
// interleaved inside every 16 by a rule written out here a second time (stacked row 16 b + 4 u + q in column 16 b + 4 q + u):
//   WpT[c][col(r)] is bit for bit Wp[r][c], the columns of rows ncols .. ldt are zero, every element of both images is written
//   and nothing outside them is.
// Type A (width 70, ld 72: two 64-column chunks, the second partial) stacks [A->A #1: 7 of 8 rows][A->A #2: 7 of 8][A->B: 2 of
// 4][root: 7 of 8, sum of two sources] = 28 columns, padded to 32 by the root segment.  Type B (width 6, ld 8) stacks its root
// alone: 4 columns, padded to 16 by a segment of 4 rows (pad_t > rows_pad).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../hydra-gnn_amd/csrc/device_fns.h"

using namespace hmp;

namespace {

constexpr uint32_t SENTINEL = 0x7fc0dead;  // a NaN payload no sum produces

int align4i(int x) { return (x + 3) & ~3; }

// column of the image for stacked row k, by digits: k = 16 b + 4 u + q
int col_of(int k) {
  const int b = k / 16, u = (k % 16) / 4, q = k % 4;
  return 16 * b + 4 * q + u;
}

struct Stack {
  int width, ldw, ncols, ldt;
  int64_t wp_off, wpt_off;
};

uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

}  // namespace

int main() {
  const int fA = 70, fB = 6, oA = 7, oB = 2;
  // parameters: lin_l / lin_r weights of the three convs, dense [f_out][f_in]
  std::vector<float> params;
  auto param = [&](int rows, int cols) {
    const int64_t off = (int64_t)params.size();
    for (int i = 0; i < rows * cols; ++i) params.push_back((float)((i * 37 + (int)off * 11) % 1013) / 64.f - 7.f);
    return off;
  };
  const int64_t aa1_l = param(oA, fA), aa1_r = param(oA, fA), aa2_l = param(oA, fA), aa2_r = param(oA, fA);
  const int64_t ab_l = param(oB, fA), ab_r = param(oB, fB);

  Stack A{fA, align4i(fA), 0, 0, 0, 0}, B{fB, align4i(fB), 0, 0, 0, 0};
  const int cA1 = 0, cA2 = align4i(oA), cAB = 2 * align4i(oA), rA = cAB + align4i(oB);
  A.ncols = rA + align4i(oA);
  B.ncols = align4i(oB);
  int64_t packed = 16;  // a margin in front: nothing may be written there
  for (Stack* s : {&A, &B}) {
    s->ldt = (s->ncols + 15) & ~15;
    s->wp_off = packed;
    packed += (int64_t)s->ncols * s->ldw;
    s->wpt_off = packed;
    packed += (int64_t)s->ldw * s->ldt;
  }
  packed += 16;

  std::vector<PackSeg> segs;
  auto seg = [&](const Stack& s, int coff, int rows, std::initializer_list<int64_t> src) {
    PackSeg p;
    memset(&p, 0, sizeof(p));
    p.kind = PACK_SUM;
    p.dst = s.wp_off + (int64_t)coff * s.ldw;
    p.rows = rows; p.rows_pad = align4i(rows); p.cols = s.width; p.ld_dst = s.ldw; p.ld_src = s.width;
    for (int64_t o : src) p.src[p.nsrc++] = o;
    p.dst_t = s.wpt_off;
    p.col_t = coff;
    p.ld_dst_t = s.ldt;
    p.pad_t = coff + p.rows_pad == s.ncols ? s.ldt - s.ncols : 0;
    segs.push_back(p);
  };
  seg(A, cA1, oA, {aa1_l});
  seg(A, cA2, oA, {aa2_l});
  seg(A, cAB, oB, {ab_l});
  seg(A, rA, oA, {aa1_r, aa2_r});
  seg(B, 0, oB, {ab_r});

  std::vector<float> buf((size_t)packed);
  for (float& f : buf) memcpy(&f, &SENTINEL, 4);
  for (const PackSeg& p : segs) {
    const int items = p.rows_pad * ((p.ld_dst + 63) / 64);
    const int blocks = (items + 3) / 4;  // 4 items per block (pack_kernel); the front kernel starts 16 per block
    for (int item = 0; item < ((blocks * 4 + 15) & ~15); ++item)
      for (int lane = 0; lane < 64; ++lane) pack_lane(p, item, lane, params.data(), buf.data());
  }

  int bad = 0;
  auto fail = [&](const char* what, int r, int c) {
    if (bad++ < 10) fprintf(stderr, "FAIL %s at (%d, %d)\n", what, r, c);
  };
  std::vector<char> owned((size_t)packed, 0);
  // expected Wp: the plain sums, source by source in table order, zero padding
  auto expect = [&](const Stack& s, int coff, int rows, std::initializer_list<int64_t> src, int r, int c) {
    (void)coff;
    float v = 0.f;
    if (r < rows && c < s.width)
      for (int64_t o : src) v += params[o + (int64_t)r * s.width + c];
    return v;
  };
  for (const Stack* s : {&A, &B}) {
    const float* wp = buf.data() + s->wp_off;
    const float* wpt = buf.data() + s->wpt_off;
    for (int r = 0; r < s->ncols; ++r)
      for (int c = 0; c < s->ldw; ++c) {
        owned[s->wp_off + (int64_t)r * s->ldw + c] = 1;
        float want;
        if (s == &A) {
          if (r < cA2) want = expect(*s, cA1, oA, {aa1_l}, r - cA1, c);
          else if (r < cAB) want = expect(*s, cA2, oA, {aa2_l}, r - cA2, c);
          else if (r < rA) want = expect(*s, cAB, oB, {ab_l}, r - cAB, c);
          else want = expect(*s, rA, oA, {aa1_r, aa2_r}, r - rA, c);
        } else {
          want = expect(*s, 0, oB, {ab_r}, r, c);
        }
        if (bits(wp[(int64_t)r * s->ldw + c]) != bits(want)) fail("Wp != plain sum", r, c);
        if (bits(wpt[(int64_t)c * s->ldt + col_of(r)]) != bits(wp[(int64_t)r * s->ldw + c])) fail("WpT[c][col(r)] != Wp[r][c]", r, c);
      }
    for (int c = 0; c < s->ldw; ++c)
      for (int r = 0; r < s->ldt; ++r) {
        owned[s->wpt_off + (int64_t)c * s->ldt + r] = 1;
        if (r >= s->ncols && bits(wpt[(int64_t)c * s->ldt + col_of(r)]) != 0u) fail("WpT padding column not +0", r, c);
      }
  }
  for (int64_t i = 0; i < packed; ++i)
    if (!owned[i] && bits(buf[i]) != SENTINEL) fail("write outside the images", (int)i, 0);
  if (bad) {
    fprintf(stderr, "pack_transpose_check: %d mismatches\n", bad);
    return 1;
  }
  printf("pack_transpose_check OK: %zu segments, stacks %dx%d (ldt %d) and %dx%d (ldt %d)\n", segs.size(), A.ncols, A.ldw, A.ldt, B.ncols,
         B.ldw, B.ldt);
  return 0;
}
