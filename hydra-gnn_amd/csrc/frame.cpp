// Frame pipeline, host stage -- SURVEY 8(f) row 4: everything GnnModel.convert_graph (bin/room_classification_server:235-271) does
// between the spark_dsg graph and the model call, as index bookkeeping on flat arrays.  Host memory only, no GPU involved.
//
// Restates, procedure for procedure (hydra_gnn_amd/dsg.py and htree.py hold the same steps as Python + torch and stay the parity
// oracle of this file):
//   * get_room_object_dsg          src/hydra_gnn/preprocess_dsgs.py:228-292   (dsg.RoomObjectGraph: same visiting order, same ties)
//   * add_object_connectivity      :191-225 with _is_on / _is_under / _is_near  (obj_edge.h: the function body of the device kernel)
//   * generate_htree + virtual nodes + typed extraction   construct.py:241-483 (the builder of htree.cpp, called directly)
// and lays out what the device stage (frame.hip) needs: ONE staging block [item table | 16-byte aligned sections] and the offsets
// of every output tensor in ONE arena (include/hydra_mp.h section 14).  hmp_frame_build_homogeneous lays the same bookkeeping out as
// the homogeneous Data instead (convert_graph's closing to_homogeneous(): data.heterogeneous_data_to_homogeneous /
// heterogeneous_htree_to_homogeneous are its parity oracle): one tensor per attribute, one item per node-type / edge-type segment.
//
// The object-object predicates run HERE and not on the device on purpose: a frame has 10^1..10^3 objects and only pairs inside a
// room are tested (microseconds of float64 work), while the H-tree builder needs the edge list on the host -- computing it on the
// device forces a round trip in the middle of every H-tree frame.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "htree_build.h"
#include "obj_edge.h"  // float64 without contraction from here on

namespace hmp {
char* err_buf();
}

namespace {
enum { L_OBJECTS = 2, L_PLACES = 3, L_ROOMS = 4 };
enum { EV_AS_GIVEN = 0, EV_BOTH = 1, EV_FLIP = 2, EV_VEC_ARANGE = 3, EV_ARANGE_VEC = 4 };  // frame.hip: edge_ends
inline int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }
}  // namespace

struct hmp_frame {
  std::vector<int32_t> kept, obj_room, dropped, rooms;  // node indices into the input arrays, visiting order
  std::vector<int32_t> rr, oo;                          // [2][E]
  std::vector<double> room_bb;                          // [rooms][2][3]
  hmp_htree* tree = nullptr;
  std::vector<int32_t> items;     // [n_items][HMP_FRAME_ITEM_WORDS], section offsets already relative to the block
  std::vector<uint8_t> sections;  // the block behind the item table
  int64_t arena_bytes = 0;
  int32_t n_blocks = 0;
  ~hmp_frame() { hmp_htree_destroy(tree); }
};

namespace {

// sections and items of one frame while it is laid out
struct Layout {
  hmp_frame& F;
  explicit Layout(hmp_frame& f) : F(f) {}
  int32_t section(const void* p, size_t bytes) {
    const size_t off = (size_t)align16((int64_t)F.sections.size());
    F.sections.resize(off + bytes);
    if (bytes) memcpy(F.sections.data() + off, p, bytes);
    return (int32_t)off;
  }
  template <class T>
  int32_t section(const std::vector<T>& v) { return section(v.data(), v.size() * sizeof(T)); }
  // a 16-byte aligned range of the arena: one output tensor
  int64_t alloc(int64_t bytes) {
    const int64_t off = F.arena_bytes;
    F.arena_bytes = align16(off + bytes);
    return off;
  }
  // `units` = work items of the launch (elements, or rows of a wide feature item), `per_block` of them to a workgroup
  void item_at(int kind, int tensor, int64_t rows, int64_t width, int64_t dst, int s0, int s1, int s2, int s3, int p0, int p1, int64_t units,
               int per_block) {
    const int32_t w[HMP_FRAME_ITEM_WORDS] = {kind, tensor, (int32_t)rows, (int32_t)width, (int32_t)dst, s0, s1, s2, s3, p0, p1, F.n_blocks};
    F.items.insert(F.items.end(), w, w + HMP_FRAME_ITEM_WORDS);
    F.n_blocks += (int32_t)((units + per_block - 1) / per_block);
  }
  // an item that is a whole tensor
  void item(int kind, int tensor, int64_t rows, int64_t width, int64_t out_bytes, int s0, int s1, int s2, int s3, int p0, int p1,
            int64_t units, int per_block) {
    item_at(kind, tensor, rows, width, alloc(out_bytes), s0, s1, s2, s3, p0, p1, units, per_block);
  }
  // feature rows of `width` floats at `dst`; the type's own npos + 3 + sem columns, zeros behind them
  void feat_at(int tensor, int64_t rows, int64_t width, int64_t dst, int s_pos, int s_size, int s_label, int s_idx, int npos, int sem) {
    if (width >= 32) item_at(HMP_FK_FEAT, tensor, rows, width, dst, s_pos, s_size, s_label, s_idx, npos, sem, rows, 4);
    else item_at(HMP_FK_FEAT, tensor, rows, width, dst, s_pos, s_size, s_label, s_idx, npos, sem, rows * width, 256);
  }
  void feat(int tensor, int64_t rows, int s_pos, int s_size, int s_label, int s_idx, int npos, int sem) {
    const int64_t width = npos + 3 + sem;
    feat_at(tensor, rows, width, alloc(rows * width * 4), s_pos, s_size, s_label, s_idx, npos, sem);
  }
  void pos(int tensor, int64_t rows, int s_pos, int s_idx) {
    item(HMP_FK_POS, tensor, rows, 3, rows * 12, s_pos, -1, -1, s_idx, 0, 0, rows * 3, 256);
  }
  void i64(int tensor, int64_t rows, int s_src, int s_idx, int src_bytes) {
    item(HMP_FK_I64, tensor, rows, 1, rows * 8, s_src, -1, -1, s_idx, src_bytes, 0, rows, 256);
  }
  void edge(int tensor, int s_list, int variant, int64_t e) {
    const int64_t eo = variant == EV_BOTH ? 2 * e : e;
    item(HMP_FK_EDGE, tensor, 2, eo, 2 * eo * 8, s_list, -1, -1, -1, variant, (int)e, 2 * eo, 256);
  }
  void eattr(int tensor, int s_list, int variant, int64_t e, int s_pos_src, int s_pos_dst) {
    const int64_t eo = variant == EV_BOTH ? 2 * e : e;
    item(HMP_FK_EATTR, tensor, eo, 3, eo * 12, s_list, s_pos_src, s_pos_dst, -1, variant, (int)e, eo * 3, 256);
  }
  // clique rows: members of clique q = the sources of the init edges whose destination is q, in ascending init-edge order
  void clique(int tensor, int64_t rows, int64_t width, const std::vector<int32_t>& init, int s_room_pos) {
    clique_at(tensor, rows, width, alloc(rows * width * 4), init, s_room_pos);
  }
  void clique_at(int tensor, int64_t rows, int64_t width, int64_t dst, const std::vector<int32_t>& init, int s_room_pos) {
    const size_t e = init.size() / 2;
    std::vector<int32_t> ptr(rows + 1, 0), mem(e);
    for (size_t k = 0; k < e; ++k) ++ptr[init[e + k] + 1];
    for (int64_t q = 0; q < rows; ++q) ptr[q + 1] += ptr[q];
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (size_t k = 0; k < e; ++k) mem[fill[init[e + k]]++] = init[k];
    const int s_ptr = section(ptr), s_mem = section(mem);
    item_at(HMP_FK_CLIQUE, tensor, rows, width, dst, s_ptr, s_mem, s_room_pos, -1, 0, 0, rows * width, 256);
  }

  // ---- segments of a homogeneous tensor: one item per node type (rows) or edge type (columns), at its place inside the tensor
  // columns [col0, col0 + eo) of an int64 [2][pitch] tensor at `base`; endpoints shifted by the row offsets of their node types
  void edge_seg(int tensor, int64_t base, int64_t pitch, int64_t col0, int s_list, int variant, int64_t e, int64_t shift_src, int64_t shift_dst) {
    const int64_t eo = variant == EV_BOTH ? 2 * e : e;
    item_at(HMP_FK_EDGE_SEG, tensor, 2, eo, base + col0 * 8, s_list, (int)pitch, (int)shift_src, (int)shift_dst, variant, (int)e, 2 * eo, 256);
  }
  void eattr_seg(int tensor, int64_t base, int64_t col0, int s_list, int variant, int64_t e, int s_pos_src, int s_pos_dst) {
    const int64_t eo = variant == EV_BOTH ? 2 * e : e;
    item_at(HMP_FK_EATTR, tensor, eo, 3, base + col0 * 12, s_list, s_pos_src, s_pos_dst, -1, variant, (int)e, eo * 3, 256);
  }
  // `rows` elements of `elem` bytes (8: int64, 1: a bool mask), all `value`, from element `row0` of the tensor at `base`
  void fill_seg(int tensor, int64_t base, int64_t row0, int64_t rows, int value, int elem) {
    item_at(HMP_FK_CONST, tensor, rows, 1, base + row0 * elem, -1, -1, -1, -1, value, elem, rows, 256);
  }
};

int fail(const char* m) {
  snprintf(hmp::err_buf(), 512, "hmp_frame_build: %s", m);
  return HMP_E_ARG;
}

}  // namespace

// both entries: the bookkeeping is the same, `homogeneous` picks the layout
static int frame_build(int32_t n, const uint64_t* ids, const int32_t* layer, const double* pos, const double* bb_min, const double* bb_max,
                       const int64_t* label, int64_t m, const uint64_t* edges, double threshold_near, double max_near, double max_on,
                       int32_t htree, int32_t relative_pos, int32_t sem_dim, int32_t n_labels, int32_t clique_dim, bool homogeneous,
                       hmp_frame** out) {
  if (!out || n < 0 || m < 0 || sem_dim < 0 || n_labels < 0 || clique_dim < 0) return fail("bad argument");
  if (n > 0 && (!ids || !layer || !pos || !bb_min || !bb_max || !label)) return fail("null node array");
  if (m > 0 && !edges) return fail("null edge array");
  if (htree && relative_pos) return fail("relative positions on H-tree edges are not produced (generate_htree has none): relative_pos with htree");
  if (htree && clique_dim > 0 && clique_dim < 3) return fail("clique_dim must be 0 or at least 3 (the mean room position)");
  if (sem_dim > 0 && n_labels < 1) return fail("a semantic table needs n_labels >= 1");

  // ---- nodes in ascending id; adjacency as neighbour lists in ascending id (the order of SceneGraph.siblings / .parent)
  std::vector<int> order(n), rank(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ids[a] < ids[b]; });
  for (int k = 0; k < n; ++k) {
    rank[order[k]] = k;
    if (k > 0 && ids[order[k]] == ids[order[k - 1]]) {
      snprintf(hmp::err_buf(), 512, "hmp_frame_build: node id %llu is listed twice", (unsigned long long)ids[order[k]]);
      return HMP_E_ARG;
    }
  }
  auto find = [&](uint64_t id) -> int {
    auto it = std::lower_bound(order.begin(), order.end(), id, [&](int a, uint64_t v) { return ids[a] < v; });
    return it != order.end() && ids[*it] == id ? *it : -1;
  };
  std::vector<std::vector<int>> adj(n);
  for (int64_t k = 0; k < m; ++k) {
    const int a = find(edges[k]), b = find(edges[m + k]);
    if (a < 0 || b < 0 || a == b) continue;  // load_dsg_json: unknown endpoints and self edges are ignored
    adj[a].push_back(b);
    adj[b].push_back(a);
  }
  for (auto& nb : adj) {
    std::sort(nb.begin(), nb.end(), [&](int a, int b) { return rank[a] < rank[b]; });
    nb.erase(std::unique(nb.begin(), nb.end()), nb.end());
  }
  auto parent = [&](int i) -> int {  // the lowest-id neighbour in a higher layer
    for (int j : adj[i]) if (layer[j] > layer[i]) return j;
    return -1;
  };

  hmp_frame* F = new hmp_frame;
  auto bail = [&](const char* msg) { delete F; return fail(msg); };
  std::vector<int> room_index(n, -1);
  for (int i : order) if (layer[i] == L_ROOMS) { room_index[i] = (int)F->rooms.size(); F->rooms.push_back(i); }
  const int n_rooms = (int)F->rooms.size();

  // ---- room-room edges, de-duplicated in visiting order (preprocess_dsgs.py:236-246)
  std::vector<int32_t> rr_src, rr_dst;
  std::set<std::pair<int, int>> seen;
  for (int r : F->rooms)
    for (int s : adj[r]) {
      if (layer[s] != L_ROOMS) continue;
      if (seen.insert({std::min(r, s), std::max(r, s)}).second) { rr_src.push_back(room_index[r]); rr_dst.push_back(room_index[s]); }
    }
  F->rr = rr_src;
  F->rr.insert(F->rr.end(), rr_dst.begin(), rr_dst.end());

  // ---- objects -> rooms (:248-283)
  for (int o : order) {
    if (layer[o] != L_OBJECTS) continue;
    const int place = parent(o);
    if (place < 0) { F->dropped.push_back(o); continue; }
    int room = parent(place);
    if (room < 0) {
      int best = -1;
      double best_d = 0;
      for (int s : adj[place]) {  // siblings in ascending id; the first minimum wins (a stable sort by distance)
        if (layer[s] != layer[place] || parent(s) < 0) continue;
        const double dx = pos[3 * place] - pos[3 * s], dy = pos[3 * place + 1] - pos[3 * s + 1], dz = pos[3 * place + 2] - pos[3 * s + 2];
        const double d = std::sqrt(dx * dx + dy * dy + dz * dz);
        if (best < 0 || d < best_d || (std::isnan(best_d) && !std::isnan(d))) { best = s; best_d = d; }
      }
      if (best < 0) { F->dropped.push_back(o); continue; }
      room = parent(best);
    }
    if (room_index[room] < 0) {
      snprintf(hmp::err_buf(), 512, "hmp_frame_build: object %llu reaches node %llu of layer %d where a room (layer 4) is expected",
               (unsigned long long)ids[o], (unsigned long long)ids[room], (int)layer[room]);
      delete F;
      return HMP_E_ARG;
    }
    F->kept.push_back(o);
    F->obj_room.push_back(room_index[room]);
  }
  const int n_obj = (int)F->kept.size();

  // ---- room boxes: AABB of the positions of the room's places, zeros without one (the stated assumption of dsg.py)
  F->room_bb.assign((size_t)n_rooms * 6, 0.0);
  for (int k = 0; k < n_rooms; ++k) {
    bool first = true;
    double* bb = &F->room_bb[(size_t)k * 6];
    for (int j : adj[F->rooms[k]]) {
      if (layer[j] != L_PLACES) continue;
      for (int c = 0; c < 3; ++c) {
        const double v = pos[3 * j + c];
        bb[c] = first ? v : std::min(bb[c], v);
        bb[3 + c] = first ? v : std::max(bb[3 + c], v);
      }
      first = false;
    }
  }

  // ---- float64 positions and sizes of the kept objects and the rooms; labels, ids
  std::vector<double> opos((size_t)n_obj * 3), osize((size_t)n_obj * 3), rpos((size_t)n_rooms * 3), rsize((size_t)n_rooms * 3);
  std::vector<int32_t> olabel(n_obj), rlabel(n_rooms);
  std::vector<int64_t> oid(n_obj), rid(n_rooms);
  auto label32 = [&](int node, int32_t& dst) -> bool {
    if (label[node] < INT32_MIN || label[node] > INT32_MAX) {
      snprintf(hmp::err_buf(), 512, "hmp_frame_build: label %lld of node %llu does not fit 32 bits", (long long)label[node],
               (unsigned long long)ids[node]);
      return false;
    }
    dst = (int32_t)label[node];
    return true;
  };
  for (int k = 0; k < n_obj; ++k) {
    const int o = F->kept[k];
    for (int c = 0; c < 3; ++c) { opos[3 * k + c] = pos[3 * o + c]; osize[3 * k + c] = bb_max[3 * o + c] - bb_min[3 * o + c]; }
    if (!label32(o, olabel[k])) { delete F; return HMP_E_ARG; }
    if (sem_dim > 0 && (label[o] < 0 || label[o] >= n_labels)) {
      snprintf(hmp::err_buf(), 512, "hmp_frame_build: label %lld of node %llu is outside the semantic table [0, %d)", (long long)label[o],
               (unsigned long long)ids[o], (int)n_labels);
      delete F;
      return HMP_E_ARG;
    }
    oid[k] = (int64_t)ids[o];
  }
  for (int k = 0; k < n_rooms; ++k) {
    const int r = F->rooms[k];
    for (int c = 0; c < 3; ++c) { rpos[3 * k + c] = pos[3 * r + c]; rsize[3 * k + c] = F->room_bb[6 * k + 3 + c] - F->room_bb[6 * k + c]; }
    if (!label32(r, rlabel[k])) { delete F; return HMP_E_ARG; }
    rid[k] = (int64_t)ids[r];
  }

  // ---- object-object edges: every object against the EARLIER objects of its room, by object then by earlier object
  {
    const hmp::ObjGeom g{opos.data(), osize.data(), F->obj_room.data(), n_obj, threshold_near, max_near, max_on};
    std::vector<std::vector<int>> by_room(n_rooms);
    std::vector<int32_t> src, dst;
    for (int i = 0; i < n_obj; ++i) {
      std::vector<int>& earlier = by_room[F->obj_room[i]];
      for (int j : earlier) if (hmp::obj_edge(g, i, j)) { src.push_back(i); dst.push_back(j); }
      earlier.push_back(i);
    }
    F->oo = src;
    F->oo.insert(F->oo.end(), dst.begin(), dst.end());
  }
  const int64_t e_oo = (int64_t)F->oo.size() / 2, e_rr = (int64_t)F->rr.size() / 2;

  if (n_rooms == 0 || n_obj == 0) {  // nothing a model can run on: no items, nothing to pack or launch
    *out = F;
    return HMP_OK;
  }

  // ---- layout: sections of the staging block, items, arena offsets, workgroups
  Layout L(*F);
  const int npos = relative_pos ? 0 : 3;
  const int s_opos = L.section(opos), s_osize = L.section(osize), s_rpos = L.section(rpos), s_rsize = L.section(rsize);
  const int s_olabel = L.section(olabel), s_rlabel = L.section(rlabel);
  const int s_osem = sem_dim > 0 ? s_olabel : -1;
  if (htree) {  // the topology, for either layout
    std::vector<int32_t> ro(F->obj_room);
    for (int k = 0; k < n_obj; ++k) ro.push_back(k);
    const int rc = hmp::htree_build_i32(n_obj, n_rooms, e_oo ? F->oo.data() : nullptr, e_oo, e_rr ? F->rr.data() : nullptr, e_rr, ro.data(),
                                        n_obj, &F->tree);
    if (rc != HMP_OK) { delete F; return rc; }
  }
  if (homogeneous) {
    // What data.heterogeneous_data_to_homogeneous / heterogeneous_htree_to_homogeneous make of the typed frame: node types
    // concatenated in store order into one x of the widest type's width, every edge type's columns shifted by the row offsets of
    // its endpoint types.  Every count is known here, so each tensor is allocated once and written by one item per segment.
    struct EdgeSeg { int s_list, variant; int64_t e; int src, dst, s_pos_src, s_pos_dst; };
    const int wo = npos + 3 + sem_dim, wr = npos + 3, H0 = HMP_FT_HOMOG;
    std::vector<int64_t> n_rows;                // rows per node type
    std::vector<EdgeSeg> main_e, init_e, pool_e;  // edge_index (with edge_type), init_edge_index, pool_edge_index
    int64_t W = std::max(wo, wr);
    int object_type = -1, room_type = 1;  // the types the masks select
    if (!htree) {
      const int s_oo = L.section(F->oo), s_rr = L.section(F->rr), s_oroom = L.section(F->obj_room);
      n_rows = {n_obj, n_rooms};
      main_e = {{s_oo, EV_BOTH, e_oo, 0, 0, s_opos, s_opos}, {s_rr, EV_BOTH, e_rr, 1, 1, s_rpos, s_rpos},
                {s_oroom, EV_VEC_ARANGE, n_obj, 1, 0, s_rpos, s_opos}, {s_oroom, EV_ARANGE_VEC, n_obj, 0, 1, s_opos, s_rpos}};
    } else {
      const hmp_htree& T = *F->tree;
      n_rows = {T.counts[0], T.counts[1], T.counts[2], T.counts[3], n_obj, n_rooms};
      W = std::max<int64_t>(W, clique_dim);  // clique rows are clique_dim wide, or as wide as the objects' / rooms' (clique_dim 0)
      object_type = 4, room_type = 5;
      // (source type, destination type) of the 10 HTREE_EDGE_TYPES, the 3 init and the 2 pool edge types
      static const int ends[15][2] = {{0, 2}, {2, 0}, {1, 2}, {2, 1}, {1, 3}, {3, 1}, {2, 3}, {3, 2}, {2, 2}, {3, 3},
                                      {4, 2}, {5, 2}, {5, 3}, {0, 4}, {1, 5}};
      for (int k = 0; k < 10; ++k) main_e.push_back({L.section(T.edges[k]), EV_AS_GIVEN, (int64_t)T.edges[k].size() / 2, ends[k][0], ends[k][1], -1, -1});
      for (int k = 0; k < 3; ++k) init_e.push_back({L.section(T.init[k]), EV_AS_GIVEN, (int64_t)T.init[k].size() / 2, ends[10 + k][0], ends[10 + k][1], -1, -1});
    }
    const int n_types = (int)n_rows.size();
    std::vector<int64_t> row0(n_types + 1, 0);
    for (int t = 0; t < n_types; ++t) row0[t + 1] = row0[t] + n_rows[t];
    const int64_t N = row0[n_types];

    const int64_t x = L.alloc(N * W * 4);
    auto xrow = [&](int t) { return x + row0[t] * W * 4; };
    if (!htree) {
      L.feat_at(H0 + 0, n_obj, W, xrow(0), s_opos, s_osize, s_osem, -1, npos, sem_dim);
      L.feat_at(H0 + 0, n_rooms, W, xrow(1), s_rpos, s_rsize, -1, -1, npos, 0);
    } else {
      const hmp_htree& T = *F->tree;
      const int s_oorig = L.section(T.object_orig), s_rorig = L.section(T.room_orig);
      L.feat_at(H0 + 0, n_rows[0], W, xrow(0), s_opos, s_osize, s_osem, s_oorig, npos, sem_dim);
      L.feat_at(H0 + 0, n_rows[1], W, xrow(1), s_rpos, s_rsize, -1, s_rorig, npos, 0);
      L.clique_at(H0 + 0, n_rows[2], W, xrow(2), T.init[1], s_rpos);  // [mean | zeros] whatever clique_dim is: zeros up to W
      L.clique_at(H0 + 0, n_rows[3], W, xrow(3), T.init[2], s_rpos);
      L.feat_at(H0 + 0, n_obj, W, xrow(4), s_opos, s_osize, s_osem, -1, npos, sem_dim);
      L.feat_at(H0 + 0, n_rooms, W, xrow(5), s_rpos, s_rsize, -1, -1, npos, 0);
      pool_e = {{s_oorig, EV_ARANGE_VEC, n_rows[0], 0, 4, -1, -1}, {s_rorig, EV_ARANGE_VEC, n_rows[1], 1, 5, -1, -1}};
    }
    auto columns = [](const EdgeSeg& g) { return g.variant == EV_BOTH ? 2 * g.e : g.e; };
    auto edge_tensor = [&](int tensor, const std::vector<EdgeSeg>& segs) {
      int64_t E = 0, col = 0;
      for (const EdgeSeg& g : segs) E += columns(g);
      const int64_t base = L.alloc(2 * E * 8);
      for (const EdgeSeg& g : segs) { L.edge_seg(tensor, base, E, col, g.s_list, g.variant, g.e, row0[g.src], row0[g.dst]); col += columns(g); }
      return E;
    };
    const int64_t E = edge_tensor(H0 + 1, main_e);
    const int64_t node_type = L.alloc(N * 8);
    for (int t = 0; t < n_types; ++t) L.fill_seg(H0 + 2, node_type, row0[t], n_rows[t], t, 8);
    const int64_t edge_type = L.alloc(E * 8);
    int64_t col = 0;
    for (size_t k = 0; k < main_e.size(); ++k) { L.fill_seg(H0 + 3, edge_type, col, columns(main_e[k]), (int)k, 8); col += columns(main_e[k]); }
    const int64_t room_mask = L.alloc(N);  // one byte per node; alloc keeps the next tensor 16-byte aligned
    for (int t = 0; t < n_types; ++t) L.fill_seg(H0 + 4, room_mask, row0[t], n_rows[t], t == room_type, 1);
    if (relative_pos) {
      const int64_t edge_attr = L.alloc(E * 12);
      col = 0;
      for (const EdgeSeg& g : main_e) { L.eattr_seg(H0 + 5, edge_attr, col, g.s_list, g.variant, g.e, g.s_pos_src, g.s_pos_dst); col += columns(g); }
    }
    if (htree) {
      const int64_t object_mask = L.alloc(N);
      for (int t = 0; t < n_types; ++t) L.fill_seg(H0 + 6, object_mask, row0[t], n_rows[t], t == object_type, 1);
      edge_tensor(H0 + 7, init_e);
      edge_tensor(H0 + 8, pool_e);
    }
  } else if (!htree) {
    const int s_oid = L.section(oid), s_rid = L.section(rid);
    const int s_oo = L.section(F->oo), s_rr = L.section(F->rr), s_oroom = L.section(F->obj_room);
    L.feat(0, n_obj, s_opos, s_osize, s_osem, -1, npos, sem_dim);
    L.pos(1, n_obj, s_opos, -1);
    L.i64(2, n_obj, s_olabel, -1, 4);
    L.i64(3, n_obj, s_oid, -1, 8);
    L.feat(4, n_rooms, s_rpos, s_rsize, -1, -1, npos, 0);
    L.pos(5, n_rooms, s_rpos, -1);
    L.i64(6, n_rooms, s_rlabel, -1, 4);
    L.i64(7, n_rooms, s_rid, -1, 8);
    L.edge(8, s_oo, EV_BOTH, e_oo);
    L.edge(9, s_rr, EV_BOTH, e_rr);
    L.edge(10, s_oroom, EV_VEC_ARANGE, n_obj);  // rooms_to_objects: (room of object k, k)
    L.edge(11, s_oroom, EV_ARANGE_VEC, n_obj);  // objects_to_rooms: its flip
    if (relative_pos) {
      L.eattr(12, s_oo, EV_BOTH, e_oo, s_opos, s_opos);
      L.eattr(13, s_rr, EV_BOTH, e_rr, s_rpos, s_rpos);
      L.eattr(14, s_oroom, EV_VEC_ARANGE, n_obj, s_rpos, s_opos);
      L.eattr(15, s_oroom, EV_ARANGE_VEC, n_obj, s_opos, s_rpos);
    }
  } else {
    const hmp_htree& T = *F->tree;
    const int s_oorig = L.section(T.object_orig), s_rorig = L.section(T.room_orig);
    const int T0 = HMP_FT_HTREE;
    L.feat(T0 + 0, T.counts[0], s_opos, s_osize, s_osem, s_oorig, npos, sem_dim);  // leaves gather from the sections, not from x
    L.pos(T0 + 1, T.counts[0], s_opos, s_oorig);
    L.i64(T0 + 2, T.counts[0], s_olabel, s_oorig, 4);
    L.feat(T0 + 3, T.counts[1], s_rpos, s_rsize, -1, s_rorig, npos, 0);
    L.pos(T0 + 4, T.counts[1], s_rpos, s_rorig);
    L.i64(T0 + 5, T.counts[1], s_rlabel, s_rorig, 4);
    L.clique(T0 + 6, T.counts[2], clique_dim ? clique_dim : npos + 3 + sem_dim, T.init[1], s_rpos);
    L.clique(T0 + 7, T.counts[3], clique_dim ? clique_dim : npos + 3, T.init[2], s_rpos);
    L.feat(T0 + 8, n_obj, s_opos, s_osize, s_osem, -1, npos, sem_dim);
    L.pos(T0 + 9, n_obj, s_opos, -1);
    L.i64(T0 + 10, n_obj, s_olabel, -1, 4);
    L.feat(T0 + 11, n_rooms, s_rpos, s_rsize, -1, -1, npos, 0);
    L.pos(T0 + 12, n_rooms, s_rpos, -1);
    L.i64(T0 + 13, n_rooms, s_rlabel, -1, 4);
    for (int k = 0; k < 10; ++k) L.edge(T0 + 14 + k, L.section(T.edges[k]), EV_AS_GIVEN, (int64_t)T.edges[k].size() / 2);
    for (int k = 0; k < 3; ++k) L.edge(T0 + 24 + k, L.section(T.init[k]), EV_AS_GIVEN, (int64_t)T.init[k].size() / 2);
    L.edge(T0 + 27, s_oorig, EV_ARANGE_VEC, T.counts[0]);  // o_to_ov: (leaf, original object)
    L.edge(T0 + 28, s_rorig, EV_ARANGE_VEC, T.counts[1]);
  }
  const int64_t n_items = (int64_t)F->items.size() / HMP_FRAME_ITEM_WORDS;
  const int64_t table_bytes = align16(n_items * HMP_FRAME_ITEM_WORDS * 4);
  if (n_items > HMP_FRAME_MAX_ITEMS) return bail("internal: more items than the launch's prefix table holds");
  if (F->arena_bytes > INT32_MAX || table_bytes + (int64_t)F->sections.size() > INT32_MAX)
    return bail("frame too large: the arena or the staging block exceeds 2 GiB");
  for (int64_t i = 0; i < n_items; ++i) {
    const bool seg = F->items[i * HMP_FRAME_ITEM_WORDS + HMP_FI_KIND] == HMP_FK_EDGE_SEG;  // S1..S3 are numbers, not sections
    for (int w = HMP_FI_S0; w <= (seg ? HMP_FI_S0 : HMP_FI_S3); ++w) {
      int32_t& s = F->items[i * HMP_FRAME_ITEM_WORDS + w];
      if (s >= 0) s += (int32_t)table_bytes;
    }
  }
  *out = F;
  return HMP_OK;
}

extern "C" int hmp_frame_build(int32_t n, const uint64_t* ids, const int32_t* layer, const double* pos, const double* bb_min,
                               const double* bb_max, const int64_t* label, int64_t m, const uint64_t* edges, double threshold_near,
                               double max_near, double max_on, int32_t htree, int32_t relative_pos, int32_t sem_dim, int32_t n_labels,
                               int32_t clique_dim, hmp_frame** out) {
  return frame_build(n, ids, layer, pos, bb_min, bb_max, label, m, edges, threshold_near, max_near, max_on, htree, relative_pos, sem_dim,
                     n_labels, clique_dim, false, out);
}

extern "C" int hmp_frame_build_homogeneous(int32_t n, const uint64_t* ids, const int32_t* layer, const double* pos, const double* bb_min,
                                           const double* bb_max, const int64_t* label, int64_t m, const uint64_t* edges,
                                           double threshold_near, double max_near, double max_on, int32_t htree, int32_t relative_pos,
                                           int32_t sem_dim, int32_t n_labels, int32_t clique_dim, hmp_frame** out) {
  return frame_build(n, ids, layer, pos, bb_min, bb_max, label, m, edges, threshold_near, max_near, max_on, htree, relative_pos, sem_dim,
                     n_labels, clique_dim, true, out);
}

extern "C" int hmp_frame_sizes(const hmp_frame* f, int64_t* sizes) {
  if (!f || !sizes) { snprintf(hmp::err_buf(), 512, "hmp_frame_sizes: null argument"); return HMP_E_ARG; }
  for (int k = 0; k < HMP_FS_COUNT; ++k) sizes[k] = 0;
  const int64_t n_items = (int64_t)f->items.size() / HMP_FRAME_ITEM_WORDS;
  sizes[HMP_FS_KEPT] = (int64_t)f->kept.size();
  sizes[HMP_FS_DROPPED] = (int64_t)f->dropped.size();
  sizes[HMP_FS_ROOMS] = (int64_t)f->rooms.size();
  sizes[HMP_FS_E_OO] = (int64_t)f->oo.size() / 2;
  sizes[HMP_FS_E_RR] = (int64_t)f->rr.size() / 2;
  sizes[HMP_FS_STAGING_BYTES] = n_items ? align16(n_items * HMP_FRAME_ITEM_WORDS * 4) + (int64_t)f->sections.size() : 0;
  sizes[HMP_FS_ARENA_BYTES] = f->arena_bytes;
  sizes[HMP_FS_ITEMS] = n_items;
  sizes[HMP_FS_BLOCKS] = f->n_blocks;
  if (f->tree) {
    for (int k = 0; k < 4; ++k) sizes[HMP_FS_HT_COUNTS + k] = f->tree->counts[k];
    for (int k = 0; k < 10; ++k) sizes[HMP_FS_HT_EDGES + k] = (int64_t)f->tree->edges[k].size() / 2;
    for (int k = 0; k < 3; ++k) sizes[HMP_FS_HT_INIT + k] = (int64_t)f->tree->init[k].size() / 2;
  }
  return HMP_OK;
}

extern "C" int hmp_frame_host_arrays(const hmp_frame* f, int32_t* kept, int32_t* obj_room, int32_t* dropped, int32_t* rooms,
                                     int32_t* rr_edges, double* room_bb, int32_t* oo_edges) {
  if (!f) { snprintf(hmp::err_buf(), 512, "hmp_frame_host_arrays: null frame"); return HMP_E_ARG; }
  auto put = [](void* dst, const void* src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
  put(kept, f->kept.data(), f->kept.size() * 4);
  put(obj_room, f->obj_room.data(), f->obj_room.size() * 4);
  put(dropped, f->dropped.data(), f->dropped.size() * 4);
  put(rooms, f->rooms.data(), f->rooms.size() * 4);
  put(rr_edges, f->rr.data(), f->rr.size() * 4);
  put(room_bb, f->room_bb.data(), f->room_bb.size() * 8);
  put(oo_edges, f->oo.data(), f->oo.size() * 4);
  return HMP_OK;
}

extern "C" int hmp_frame_pack(const hmp_frame* f, void* staging, int64_t bytes) {
  auto bad = [](const char* m) { snprintf(hmp::err_buf(), 512, "hmp_frame_pack: %s", m); return HMP_E_ARG; };
  if (!f || !staging) return bad("null argument");
  if (f->items.empty()) return bad("the frame has no room or no kept object: nothing to pack");
  const size_t table = f->items.size() * 4, table_al = (size_t)align16((int64_t)table);
  if (bytes < (int64_t)(table_al + f->sections.size())) return bad("the staging buffer is smaller than HMP_FS_STAGING_BYTES");
  uint8_t* p = (uint8_t*)staging;
  memcpy(p, f->items.data(), table);
  memset(p + table, 0, table_al - table);
  if (!f->sections.empty()) memcpy(p + table_al, f->sections.data(), f->sections.size());
  return HMP_OK;
}

extern "C" void hmp_frame_destroy(hmp_frame* f) { delete f; }
