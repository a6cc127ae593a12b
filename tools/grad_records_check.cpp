// Host-side check of the gradient un-pack's workgroup records (GradRec, csrc/kernels.h grad_records_build).
//
//   make -C hydra-gnn_amd/csrc grad_records_check && hydra-gnn_amd/csrc/build/grad_records_check
//
// Builds the record table for synthetic segment lists on the CPU and replays the index arithmetic of grad_reduce_kernel
// (csrc/optim.hip) over every (workgroup, thread) the launch starts:
//   - every element of every segment is produced by exactly one (workgroup, thread) and stored at its segment's dst + index,
//     and no thread stores anywhere else;
//   - the element (r, c) a thread derives from its record reads, for every GT_COPY term, the slab address the segment table
//     gives for that element;
//   - the number of records is the number of workgroups of the launch (the sum of grad_seg_blocks), records are 128 bytes and
//     128-byte aligned;
//   - segments with parameter-reading terms carry their segment index and no terms of their own.
// Lists: one segment of 1 element; 255 / 256 / 257 elements; cols = 1, 7, 65, 306, 307; three terms (C != Cp among them); a mix
// with GAT-kind segments (thread per element and wavefront per element) in the middle; SEG_MAX segments.
// The target builds under AddressSanitizer + UBSan; `make grad_records_check_plain` builds build/grad_records_check_plain without.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../hydra-gnn_amd/csrc/kernels.h"

using namespace hmp;

namespace {

GradTerm mk_term(int kind, int slab_id, int64_t src, int ld, int C, int Cp, float scale = 1.f) {
  GradTerm t;
  memset(&t, 0, sizeof(t));
  t.kind = kind; t.slab_id = slab_id; t.src = src; t.ld = ld; t.C = C; t.Cp = Cp; t.scale = scale;
  return t;
}

// a GT_COPY segment of `rows` x `cols` whose n_terms terms read stacks of their own
GradSeg copy_seg(int64_t dst, int rows, int cols, int n_terms, int C = 0, int Cp = 0) {
  GradSeg g;
  memset(&g, 0, sizeof(g));
  g.dst = dst; g.rows = rows; g.cols = cols; g.n_terms = n_terms;
  for (int ti = 0; ti < n_terms; ++ti)
    g.t[ti] = mk_term(GT_COPY, 3 + 5 * ti, 1000 * (ti + 1) + dst, cols + 3 + ti, C ? C : rows, Cp ? Cp : rows, 1.f + (float)ti);
  return g;
}

GradSeg att_seg(int64_t dst, int rows, int cols, int kind, int n_terms = 1) {
  GradSeg g = copy_seg(dst, rows, cols, n_terms);
  g.t[n_terms - 1].kind = kind;
  g.t[n_terms - 1].inner = 5;
  return g;
}

int check(const char* name, const std::vector<GradSeg>& gs) {
  int bad = 0;
  auto fail = [&](const char* what, int64_t a, int64_t b) {
    if (bad++ < 10) fprintf(stderr, "FAIL %s: %s (%lld, %lld)\n", name, what, (long long)a, (long long)b);
  };
  int64_t want_blocks = 0, total = 0;
  for (const GradSeg& g : gs) {
    want_blocks += grad_seg_blocks(g);
    const int64_t end = g.dst + (int64_t)g.rows * g.cols;
    if (end > total) total = end;
  }
  std::vector<GradRec> recs((size_t)want_blocks);  // exactly the launch's size: a record too many is a write past the end
  const int64_t got = grad_records_build(gs.data(), (int)gs.size(), recs.data());
  if (got != want_blocks) fail("record count != workgroups of the launch", got, want_blocks);
  if (sizeof(GradRec) % 64 != 0 || alignof(GradRec) % 64 != 0) fail("record is not whole lines", (int64_t)sizeof(GradRec), (int64_t)alignof(GradRec));
  if (!recs.empty() && (uintptr_t)recs.data() % alignof(GradRec) != 0) fail("table not aligned", 0, 0);

  std::vector<int> hits((size_t)total, 0);
  std::vector<int> owner((size_t)total, -1);  // segment whose element lives at a flat offset
  for (size_t si = 0; si < gs.size(); ++si)
    for (int64_t i = 0; i < (int64_t)gs[si].rows * gs[si].cols; ++i) owner[(size_t)(gs[si].dst + i)] = (int)si;

  for (int64_t b = 0; b < got; ++b) {
    const GradRec& R = recs[(size_t)b];
    if (R.seg < 0 || R.seg >= (int)gs.size()) { fail("segment index out of range", b, R.seg); continue; }
    const GradSeg& S = gs[(size_t)R.seg];
    if (R.kind != grad_seg_kind(S)) fail("kind tag", b, R.kind);
    if (R.cols != S.cols || R.n_terms != S.n_terms) fail("cols / n_terms", b, R.seg);
    if (R.dst != S.dst + R.first) fail("dst != segment dst + first", b, R.dst);
    if (R.n_live < 1 || R.n_live > (R.kind == GR_WAVE ? 4 : 256)) fail("n_live out of range", b, R.n_live);
    for (int tid = 0; tid < 256; ++tid) {
      // grad_reduce_kernel: a wavefront per element in GR_WAVE workgroups (lane 0 stores), else a thread per element
      int64_t i, e;
      if (R.kind == GR_WAVE) {
        if ((tid & 63) != 0 || (tid >> 6) >= R.n_live) continue;
        i = (int64_t)R.first + (tid >> 6);
        e = S.dst + i;
      } else {
        if (tid >= R.n_live) continue;
        i = (int64_t)R.first + tid;
        e = R.dst + tid;
      }
      if (i >= (int64_t)S.rows * S.cols) { fail("element past its segment", b, tid); continue; }
      if (e < 0 || e >= total) { fail("store outside the flat buffer", b, tid); continue; }
      if (e != S.dst + i || owner[(size_t)e] != R.seg) fail("element does not land on its dst", b, tid);
      ++hits[(size_t)e];
      if (R.kind != GR_COPY) {
        for (int ti = 0; ti < 3; ++ti)
          if (R.t[ti].src != 0 || R.t[ti].ld != 0) fail("a parameter-reading segment carries record terms", b, ti);
        continue;
      }
      const int r = (int)i / R.cols, c = (int)i - r * R.cols;
      for (int ti = 0; ti < R.n_terms; ++ti) {
        const GradRecTerm& Q = R.t[ti];
        const GradTerm& T = S.t[ti];
        const int row = Q.C == Q.Cp ? r : (r / Q.C) * Q.Cp + (r % Q.C);
        const int64_t addr = Q.src + (int64_t)row * Q.ld + c;
        const int64_t rr = i / S.cols, cc = i % S.cols;
        const int64_t want = T.src + ((rr / T.C) * T.Cp + (rr % T.C)) * T.ld + cc;
        if (addr != want) fail("slab address of a term", b, tid);
        if (Q.slab_id != T.slab_id || memcmp(&Q.scale, &T.scale, 4) != 0) fail("slab id / scale of a term", b, ti);
      }
    }
  }
  for (int64_t e = 0; e < total; ++e) {
    const int want = owner[(size_t)e] >= 0 ? 1 : 0;
    if (hits[(size_t)e] != want) fail("element covered != once", e, hits[(size_t)e]);
  }
  printf("%-28s %4zu segments, %6lld workgroups, %8lld elements: %s\n", name, gs.size(), (long long)got, (long long)total, bad ? "FAIL" : "ok");
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  bad += check("one element", {copy_seg(0, 1, 1, 1)});
  {
    std::vector<GradSeg> gs;
    int64_t dst = 0;
    for (int el : {255, 256, 257}) { gs.push_back(copy_seg(dst, el, 1, 1)); dst += el; }
    bad += check("255 / 256 / 257 elements", gs);
  }
  {
    std::vector<GradSeg> gs;
    int64_t dst = 5;  // a gap in front: nothing may be stored there
    for (int cols : {1, 7, 65, 306, 307}) { gs.push_back(copy_seg(dst, 11, cols, 1)); dst += 11 * cols + 2; }
    bad += check("cols 1 7 65 306 307", gs);
  }
  bad += check("three terms", {copy_seg(0, 24, 37, 3), copy_seg(24 * 37, 12, 65, 3, 4, 8), copy_seg(24 * 37 + 12 * 65, 300, 1, 2)});
  {
    std::vector<GradSeg> gs;
    int64_t dst = 0;
    gs.push_back(copy_seg(dst, 64, 306, 1)); dst += 64 * 306;
    gs.push_back(att_seg(dst, 16, 70, GT_ATT_OUTER, 3)); dst += 16 * 70;   // thread per element through the segment table
    gs.push_back(att_seg(dst, 18, 1, GT_ATT_DOT)); dst += 18;             // wavefront per element: 4 + 4 + 4 + 4 + 2
    gs.push_back(att_seg(dst, 16, 3, GT_ATT_OUTER_T)); dst += 16 * 3;
    gs.push_back(att_seg(dst, 1, 1, GT_ATT_DOT_T)); dst += 1;
    gs.push_back(att_seg(dst, 9, 1, GT_ATT_DOT, 2)); dst += 9;            // a dot product among two terms: thread per element
    gs.push_back(copy_seg(dst, 64, 1, 1)); dst += 64;
    bad += check("mix with GAT kinds", gs);
  }
  {
    std::vector<GradSeg> gs;
    int64_t dst = 0;
    for (int s = 0; s < SEG_MAX; ++s) {
      const int rows = 1 + (s * 7) % 67, cols = s % 3 == 0 ? 1 : 1 + (s * 13) % 70;
      gs.push_back(copy_seg(dst, rows, cols, 1 + s % 3));
      dst += (int64_t)rows * cols;
    }
    bad += check("400 segments", gs);
  }
  if (bad) {
    fprintf(stderr, "grad_records_check: %d failures\n", bad);
    return 1;
  }
  printf("grad_records_check OK\n");
  return 0;
}
