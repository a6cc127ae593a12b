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
// With relative_pos = HMP_FRAME_RELPOS_HTREE an H-tree frame is laid out as the server's compute_relative_pos leaves it
// (mp3d_dataset.py:298-319 on Hydra_mp3d_htree_data; data.compute_relative_pos of htree.generate_htree(clique_pos=True) is the
// parity oracle): every x without its three position columns, pos on the clique types, edge_attr on every edge type.
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
// (source, destination) node types, in store order, of the 10 HTREE_EDGE_TYPES, the 3 init and the 2 pool edge types
const int kTreeEnds[15][2] = {{0, 2}, {2, 0}, {1, 2}, {2, 1}, {1, 3}, {3, 1}, {2, 3}, {3, 2}, {2, 2}, {3, 3}, {4, 2}, {5, 2}, {5, 3}, {0, 4}, {1, 5}};
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
  int32_t cfg[7] = {0, 0, 0, 0, 0, 0, 0};  // homogeneous, htree, relative_pos, sem_dim, n_labels, clique_dim, flags: what a batch must share
  int32_t n_input = 0;                  // nodes of the input arrays (the length of a frame's label vector y)
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
  // clique rows: members of clique q = the sources of the init edges whose destination is q, in ascending init-edge order.
  // `drop`: leading columns of [mean | zeros] a row goes without.  Returns the (ptr, members) sections it made
  struct Members { int s_ptr, s_mem; };
  Members clique(int tensor, int64_t rows, int64_t width, const std::vector<int32_t>& init, int s_room_pos, int drop) {
    return clique_at(tensor, rows, width, alloc(rows * width * 4), init, s_room_pos, drop);
  }
  Members clique_at(int tensor, int64_t rows, int64_t width, int64_t dst, const std::vector<int32_t>& init, int s_room_pos, int drop) {
    const size_t e = init.size() / 2;
    std::vector<int32_t> ptr(rows + 1, 0), mem(e);
    for (size_t k = 0; k < e; ++k) ++ptr[init[e + k] + 1];
    for (int64_t q = 0; q < rows; ++q) ptr[q + 1] += ptr[q];
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (size_t k = 0; k < e; ++k) mem[fill[init[e + k]]++] = init[k];
    const Members m{section(ptr), section(mem)};
    item_at(HMP_FK_CLIQUE, tensor, rows, width, dst, m.s_ptr, m.s_mem, s_room_pos, -1, drop, 0, rows * width, 256);
    return m;
  }
  // `pos` of a clique type: the three columns, from sections a clique item already made
  void clique_pos(int tensor, int64_t rows, const Members& m, int s_room_pos) {
    item(HMP_FK_CLIQUE, tensor, rows, 3, rows * 12, m.s_ptr, m.s_mem, s_room_pos, -1, 0, 0, rows * 3, 256);
  }

  // ---- relative positions on H-tree edges: where an end of an edge type finds its position (HMP_FE_*)
  struct End { int mode, s_pos, s_a, s_b; };
  // the descriptor section of an HMP_FK_EATTR_HT item; its offsets count from the descriptor itself, so they hold wherever a batch
  // puts the frame's sections
  int32_t ends_section(const End& src, const End& dst) {
    const int32_t at = (int32_t)align16((int64_t)F.sections.size());  // where section() puts it
    auto rel = [&](int s) { return s >= 0 ? s - at : 0; };
    const int32_t w[2 * HMP_FRAME_END_WORDS] = {src.mode, rel(src.s_pos), rel(src.s_a), rel(src.s_b),
                                                dst.mode, rel(dst.s_pos), rel(dst.s_a), rel(dst.s_b)};
    return section(w, sizeof w);
  }
  void eattr_ht_at(int tensor, int64_t dst, int s_list, int variant, int64_t e, int s_ends) {
    item_at(HMP_FK_EATTR_HT, tensor, e, 3, dst, s_list, s_ends, -1, -1, variant, (int)e, e * 3, 256);
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
                       int32_t flags, hmp_frame** out) {
  if (flags & ~HMP_FRAME_NO_ROOM_EDGES) return fail("unknown flag (HMP_FRAME_NO_ROOM_EDGES is the only one)");
  if (!out || n < 0 || m < 0 || sem_dim < 0 || n_labels < 0 || clique_dim < 0) return fail("bad argument");
  if (n > 0 && (!ids || !layer || !pos || !bb_min || !bb_max || !label)) return fail("null node array");
  if (m > 0 && !edges) return fail("null edge array");
  const bool rel_ht = relative_pos == HMP_FRAME_RELPOS_HTREE;
  if (rel_ht && !htree) return fail("relative_pos = HMP_FRAME_RELPOS_HTREE (relative positions on H-tree edges) needs htree");
  if (htree && relative_pos && !rel_ht)
    return fail("relative_pos = 1 with htree is refused: relative positions on H-tree edges are relative_pos = HMP_FRAME_RELPOS_HTREE");
  if (rel_ht && clique_dim > 0 && clique_dim <= 3)
    return fail("clique_dim must be 0 or more than 3 with relative positions on H-tree edges (a clique row loses its 3 position columns)");
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
  const int32_t cfg[7] = {homogeneous ? 1 : 0, htree ? 1 : 0, rel_ht ? HMP_FRAME_RELPOS_HTREE : (relative_pos ? 1 : 0), sem_dim, n_labels, clique_dim,
                          flags};
  memcpy(F->cfg, cfg, sizeof cfg);
  F->n_input = n;
  auto bail = [&](const char* msg) { delete F; return fail(msg); };
  std::vector<int> room_index(n, -1);
  for (int i : order) if (layer[i] == L_ROOMS) { room_index[i] = (int)F->rooms.size(); F->rooms.push_back(i); }
  const int n_rooms = (int)F->rooms.size();

  // ---- room-room edges, de-duplicated in visiting order (preprocess_dsgs.py:236-246)
  std::vector<int32_t> rr_src, rr_dst;
  std::set<std::pair<int, int>> seen;
  // HMP_FRAME_NO_ROOM_EDGES (remove_room_edges_in_dsg): the room layer loses its edges here, before the layouts and the H-tree read them
  if (!(flags & HMP_FRAME_NO_ROOM_EDGES))
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
  const int npos = relative_pos ? 0 : 3, drop = rel_ht ? 3 : 0;  // leading columns every x / every clique row goes without
  const int s_opos = L.section(opos), s_osize = L.section(osize), s_rpos = L.section(rpos), s_rsize = L.section(rsize);
  const int s_olabel = L.section(olabel), s_rlabel = L.section(rlabel);
  const int s_osem = sem_dim > 0 ? s_olabel : -1;
  // relative positions on H-tree edges: how a node of each H-tree type (store order) finds its position
  Layout::End end_of[6];
  auto tree_ends = [&](int s_oorig, int s_rorig, const Layout::Members& m_or, const Layout::Members& m_rr) {
    end_of[0] = {HMP_FE_GATHER, s_opos, s_oorig, -1};
    end_of[1] = {HMP_FE_GATHER, s_rpos, s_rorig, -1};
    end_of[2] = {HMP_FE_CLIQUE, s_rpos, m_or.s_ptr, m_or.s_mem};
    end_of[3] = {HMP_FE_CLIQUE, s_rpos, m_rr.s_ptr, m_rr.s_mem};
    end_of[4] = {HMP_FE_DIRECT, s_opos, -1, -1};
    end_of[5] = {HMP_FE_DIRECT, s_rpos, -1, -1};
  };
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
      W = std::max<int64_t>(W, clique_dim - drop);  // clique rows are clique_dim wide, or as wide as the objects' / rooms' (clique_dim 0)
      object_type = 4, room_type = 5;
      const auto& ends = kTreeEnds;
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
      const Layout::Members m_or = L.clique_at(H0 + 0, n_rows[2], W, xrow(2), T.init[1], s_rpos, drop);  // [mean | zeros] whatever clique_dim is: zeros up to W
      const Layout::Members m_rr = L.clique_at(H0 + 0, n_rows[3], W, xrow(3), T.init[2], s_rpos, drop);
      tree_ends(s_oorig, s_rorig, m_or, m_rr);
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
      for (const EdgeSeg& g : main_e) {
        if (rel_ht) L.eattr_ht_at(H0 + 5, edge_attr + col * 12, g.s_list, g.variant, g.e, L.ends_section(end_of[g.src], end_of[g.dst]));
        else L.eattr_seg(H0 + 5, edge_attr, col, g.s_list, g.variant, g.e, g.s_pos_src, g.s_pos_dst);
        col += columns(g);
      }
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
    const Layout::Members m_or = L.clique(T0 + 6, T.counts[2], clique_dim ? clique_dim - drop : npos + 3 + sem_dim, T.init[1], s_rpos, drop);
    const Layout::Members m_rr = L.clique(T0 + 7, T.counts[3], clique_dim ? clique_dim - drop : npos + 3, T.init[2], s_rpos, drop);
    L.feat(T0 + 8, n_obj, s_opos, s_osize, s_osem, -1, npos, sem_dim);
    L.pos(T0 + 9, n_obj, s_opos, -1);
    L.i64(T0 + 10, n_obj, s_olabel, -1, 4);
    L.feat(T0 + 11, n_rooms, s_rpos, s_rsize, -1, -1, npos, 0);
    L.pos(T0 + 12, n_rooms, s_rpos, -1);
    L.i64(T0 + 13, n_rooms, s_rlabel, -1, 4);
    int s_list[15], variant[15];
    int64_t n_e[15];
    for (int k = 0; k < 13; ++k) {
      const std::vector<int32_t>& e = k < 10 ? T.edges[k] : T.init[k - 10];
      s_list[k] = L.section(e), variant[k] = EV_AS_GIVEN, n_e[k] = (int64_t)e.size() / 2;
    }
    s_list[13] = s_oorig, variant[13] = EV_ARANGE_VEC, n_e[13] = T.counts[0];  // o_to_ov: (leaf, original object)
    s_list[14] = s_rorig, variant[14] = EV_ARANGE_VEC, n_e[14] = T.counts[1];
    for (int k = 0; k < 15; ++k) L.edge(T0 + 14 + k, s_list[k], variant[k], n_e[k]);
    if (rel_ht) {  // what compute_relative_pos adds to an H-tree: pos of the clique types, edge_attr of every edge type
      const int R0 = HMP_FT_HTREL;
      L.clique_pos(R0 + 0, T.counts[2], m_or, s_rpos);
      L.clique_pos(R0 + 1, T.counts[3], m_rr, s_rpos);
      tree_ends(s_oorig, s_rorig, m_or, m_rr);
      for (int k = 0; k < 15; ++k)
        L.eattr_ht_at(R0 + 2 + k, L.alloc(n_e[k] * 12), s_list[k], variant[k], n_e[k], L.ends_section(end_of[kTreeEnds[k][0]], end_of[kTreeEnds[k][1]]));
    }
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
                     n_labels, clique_dim, false, 0, out);
}

extern "C" int hmp_frame_build_homogeneous(int32_t n, const uint64_t* ids, const int32_t* layer, const double* pos, const double* bb_min,
                                           const double* bb_max, const int64_t* label, int64_t m, const uint64_t* edges,
                                           double threshold_near, double max_near, double max_on, int32_t htree, int32_t relative_pos,
                                           int32_t sem_dim, int32_t n_labels, int32_t clique_dim, hmp_frame** out) {
  return frame_build(n, ids, layer, pos, bb_min, bb_max, label, m, edges, threshold_near, max_near, max_on, htree, relative_pos, sem_dim,
                     n_labels, clique_dim, true, 0, out);
}

extern "C" int hmp_frame_build_flags(int32_t n, const uint64_t* ids, const int32_t* layer, const double* pos, const double* bb_min,
                                     const double* bb_max, const int64_t* label, int64_t m, const uint64_t* edges, double threshold_near,
                                     double max_near, double max_on, int32_t htree, int32_t relative_pos, int32_t sem_dim, int32_t n_labels,
                                     int32_t clique_dim, int32_t homogeneous, int32_t flags, hmp_frame** out) {
  return frame_build(n, ids, layer, pos, bb_min, bb_max, label, m, edges, threshold_near, max_near, max_on, htree, relative_pos, sem_dim,
                     n_labels, clique_dim, homogeneous != 0, flags, out);
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

// ---------------------------------------------------------------------------------------------------------------------------------
// Batches of frames (include/hydra_mp.h section 14, "batches"): K built frames -> ONE block [group table | item table | sections]
// and ONE arena holding either the collated batch the models read (HMP_FB_COLLATED: data.collate / data.collate_homogeneous of the
// K single results) or the packed arrays of a GraphStore (HMP_FB_STORE: the same concatenations with graph-local endpoints).
// A batched tensor is the frames' tensors back to back, so every item of every frame is kept and RE-ADDRESSED: its sections move to
// the frame's place in the block, its destination to the frame's place inside the batched tensor, an edge list becomes an EDGE_SEG
// with the batched tensor's pitch and the frame's two shifts.  Nothing is re-derived from the scene graph, and the frames' sections
// are not copied before hmp_frame_batch_pack writes them to the caller's buffer.
// ---------------------------------------------------------------------------------------------------------------------------------
struct hmp_frame_batch {
  std::vector<const hmp_frame*> frames;  // the frames with items, in graph order (they outlive the batch)
  std::vector<int32_t> graph_of_frame;   // per input frame: its graph, -1 for a skipped one
  std::vector<int64_t> frame_base;       // per graph: where its sections start, relative to the first section of the block
  std::vector<int32_t> groups, items;
  std::vector<uint8_t> sections;         // the batch's own sections (offset vectors, labels, label row indices), behind the frames'
  int64_t own_base = 0;                  // relative to the first section, as frame_base
  std::vector<int64_t> tensors;          // [n][4]: tensor number, byte offset in the arena, rows, width
  std::vector<int64_t> node_ptr, edge_ptr;  // [types][graphs + 1]
  int32_t n_node_types = 0, n_edge_types = 0, n_blocks = 0;
  int64_t arena_bytes = 0, max_graph_nodes = 0;
};

namespace {

int batch_fail(const char* m) {
  snprintf(hmp::err_buf(), 512, "hmp_frame_batch_build: %s", m);
  return HMP_E_ARG;
}

// rows per node type of a frame, in store order: typed {objects, rooms} / the six H-tree stores; the same types are the segments
// of a homogeneous frame's x
int node_rows(const hmp_frame& f, int64_t* rows) {
  const int64_t n_obj = (int64_t)f.kept.size(), n_rooms = (int64_t)f.rooms.size();
  if (!f.tree) { rows[0] = n_obj; rows[1] = n_rooms; return 2; }
  for (int k = 0; k < 4; ++k) rows[k] = f.tree->counts[k];
  rows[4] = n_obj; rows[5] = n_rooms;
  return 6;
}

// node type of a typed node tensor, or (source, destination) types of a typed edge tensor (edge_index and edge_attr alike)
void typed_ends(int tensor, int& src, int& dst) {
  static const int base_ends[4][2] = {{0, 0}, {1, 1}, {1, 0}, {0, 1}};
  if (tensor < HMP_FT_HTREE) { src = base_ends[(tensor - 8) & 3][0]; dst = base_ends[(tensor - 8) & 3][1]; }
  else { src = kTreeEnds[tensor - HMP_FT_HTREE - 14][0]; dst = kTreeEnds[tensor - HMP_FT_HTREE - 14][1]; }
}

// bytes of one row of an item's output (edge lists excepted: they are counted in columns)
int64_t row_bytes(const int32_t* w) {
  switch (w[HMP_FI_KIND]) {
    case HMP_FK_FEAT: case HMP_FK_CLIQUE: return (int64_t)w[HMP_FI_WIDTH] * 4;
    case HMP_FK_POS: case HMP_FK_EATTR: case HMP_FK_EATTR_HT: return 12;
    case HMP_FK_CONST: return w[HMP_FI_P1];
    default: return 8;
  }
}

}  // namespace

extern "C" int hmp_frame_batch_items_needed(const hmp_frame* f, int32_t form, int32_t with_y, int32_t* per_frame, int32_t* per_batch) {
  if (!f || !per_frame || !per_batch || (form != HMP_FB_COLLATED && form != HMP_FB_STORE)) return batch_fail("bad argument (items_needed)");
  const bool homog = f->cfg[0], htree = f->cfg[1], rel = f->cfg[2], rel_ht = f->cfg[2] == HMP_FRAME_RELPOS_HTREE;
  const int n_types = htree ? 6 : 2;
  // items of a frame of this configuration (a frame without items has none to count: the layouts' own counts, as frame_build emits them)
  int frame_items, n_edge_types;
  if (homog) { frame_items = htree ? (rel_ht ? 59 : 49) : (rel ? 18 : 14); n_edge_types = htree ? 3 : 1; }
  else { frame_items = htree ? (rel_ht ? 46 : 29) : (rel ? 16 : 12); n_edge_types = htree ? 15 : 4; }
  if (!f->items.empty()) frame_items = (int)(f->items.size() / HMP_FRAME_ITEM_WORDS);
  *per_frame = frame_items + (!homog && form == HMP_FB_COLLATED ? n_types : 0) + (with_y ? (homog ? n_types : (htree ? 4 : 2)) : 0);
  *per_batch = homog ? (form == HMP_FB_STORE ? 1 + n_edge_types : 0) : n_types + n_edge_types;
  return HMP_OK;
}

extern "C" int hmp_frame_batch_build(int32_t n_frames, const hmp_frame* const* frames, int32_t form, const int64_t* const* y,
                                     hmp_frame_batch** out) {
  if (!out || n_frames < 0 || (n_frames > 0 && !frames)) return batch_fail("bad argument");
  if (form != HMP_FB_COLLATED && form != HMP_FB_STORE) return batch_fail("form must be HMP_FB_COLLATED or HMP_FB_STORE");
  for (int i = 0; i < n_frames; ++i) {
    if (!frames[i]) return batch_fail("null frame");
    if (memcmp(frames[i]->cfg, frames[0]->cfg, sizeof frames[0]->cfg) != 0)
      return batch_fail("the frames were built with different configurations (typed / homogeneous, htree, relative_pos, sem_dim, n_labels, clique_dim)");
    if (y && !y[i] && frames[i]->n_input > 0) return batch_fail("labels are given for every frame or for none: a frame's y is null");
  }
  hmp_frame_batch* B = new hmp_frame_batch;
  auto bail = [&](const char* m) { delete B; return batch_fail(m); };
  B->graph_of_frame.assign(n_frames, -1);
  std::vector<int> input_of;  // graph -> input frame
  for (int i = 0; i < n_frames; ++i)
    if (!frames[i]->items.empty()) { B->graph_of_frame[i] = (int32_t)B->frames.size(); B->frames.push_back(frames[i]); input_of.push_back(i); }
  const int G = (int)B->frames.size();
  if (G == 0) { *out = B; return HMP_OK; }  // nothing to pack, nothing to launch

  const hmp_frame& F0 = *B->frames[0];
  const bool homog = F0.cfg[0] != 0, collated = form == HMP_FB_COLLATED;
  const int W = HMP_FRAME_ITEM_WORDS;
  const int ipf = (int)(F0.items.size() / W);
  for (const hmp_frame* f : B->frames) {
    if ((int)(f->items.size() / W) != ipf) return bail("internal: frames of one configuration differ in their item count");
    for (int j = 0; j < ipf; ++j)
      if (f->items[j * W + HMP_FI_TENSOR] != F0.items[j * W + HMP_FI_TENSOR]) return bail("internal: frames of one configuration differ in their item order");
  }

  // ---- rows of every node type per graph and their running sums; a homogeneous batch has ONE node set (all types of a graph)
  int64_t rows[6];
  const int n_types = node_rows(F0, rows);  // types of a frame: segments of a homogeneous x
  B->n_node_types = homog ? 1 : n_types;
  std::vector<int64_t> type_rows((size_t)G * n_types);
  B->node_ptr.assign((size_t)B->n_node_types * (G + 1), 0);
  for (int g = 0; g < G; ++g) {
    node_rows(*B->frames[g], rows);
    int64_t total = 0;
    for (int t = 0; t < n_types; ++t) { type_rows[(size_t)g * n_types + t] = rows[t]; total += rows[t]; }
    if (homog) {
      B->node_ptr[g + 1] = B->node_ptr[g] + total;
      B->max_graph_nodes = std::max(B->max_graph_nodes, total);
    } else {
      for (int t = 0; t < n_types; ++t) {
        B->node_ptr[(size_t)t * (G + 1) + g + 1] = B->node_ptr[(size_t)t * (G + 1) + g] + rows[t];
        B->max_graph_nodes = std::max(B->max_graph_nodes, rows[t]);
      }
    }
  }
  auto nptr = [&](int t, int g) { return B->node_ptr[(size_t)t * (G + 1) + g]; };

  // ---- where every frame's sections go
  int64_t sec_end = 0;
  for (int g = 0; g < G; ++g) { B->frame_base.push_back(sec_end); sec_end = align16(sec_end + (int64_t)B->frames[g]->sections.size()); }
  B->own_base = sec_end;
  auto own_section = [&](const void* p, size_t bytes) {
    const size_t off = (size_t)align16((int64_t)B->sections.size());
    B->sections.resize(off + bytes);
    if (bytes) memcpy(B->sections.data() + off, p, bytes);
    return (int64_t)off;  // relative to own_base
  };
  auto alloc = [&](int64_t bytes) { const int64_t off = B->arena_bytes; B->arena_bytes = align16(off + bytes); return off; };
  // offsets can pass 2^31 while the table is made; they are checked before they are narrowed
  bool too_large = false;
  auto put_item = [&](const int64_t* w, int64_t blocks) {
    for (int k = 0; k < W - 1; ++k) { if (w[k] > INT32_MAX || w[k] < INT32_MIN) too_large = true; B->items.push_back((int32_t)w[k]); }
    B->items.push_back(B->n_blocks);
    if ((int64_t)B->n_blocks + blocks > INT32_MAX) too_large = true; else B->n_blocks += (int32_t)blocks;
  };
  auto blocks_of = [](int64_t units) { return (units + 255) / 256; };

  // ---- the frames' tensors: a run of items of one tensor number (one item of a typed frame, the segments of a homogeneous one)
  for (int a = 0; a < ipf;) {
    int b = a + 1;
    const int tensor = F0.items[a * W + HMP_FI_TENSOR];
    while (b < ipf && F0.items[b * W + HMP_FI_TENSOR] == tensor) ++b;
    const int kind0 = F0.items[a * W + HMP_FI_KIND];
    const bool edge = kind0 == HMP_FK_EDGE || kind0 == HMP_FK_EDGE_SEG;
    // extent of the tensor in every frame: columns of an edge list, bytes of everything else
    std::vector<int64_t> off(G + 1, 0);
    for (int g = 0; g < G; ++g) {
      int64_t ext = 0;
      for (int j = a; j < b; ++j) {
        const int32_t* w = &B->frames[g]->items[j * W];
        ext += edge ? (int64_t)w[HMP_FI_WIDTH] : (int64_t)w[HMP_FI_ROWS] * row_bytes(w);
      }
      off[g + 1] = off[g] + ext;
    }
    const int64_t base = alloc(edge ? 2 * off[G] * 8 : off[G]);
    if (edge) {
      B->edge_ptr.insert(B->edge_ptr.end(), off.begin(), off.end());
      ++B->n_edge_types;
      const int64_t t4[4] = {tensor, base, 2, off[G]};
      B->tensors.insert(B->tensors.end(), t4, t4 + 4);
    } else {
      const int32_t* w0 = &F0.items[a * W];
      const int64_t rb = row_bytes(w0), width = (kind0 == HMP_FK_FEAT || kind0 == HMP_FK_CLIQUE) ? w0[HMP_FI_WIDTH] : (rb == 12 ? 3 : 1);
      const int64_t t4[4] = {tensor, base, off[G] / rb, width};
      B->tensors.insert(B->tensors.end(), t4, t4 + 4);
    }
    for (int g = 0; g < G; ++g) {
      const hmp_frame& f = *B->frames[g];
      const int64_t tb = align16((int64_t)ipf * W * 4);  // the frame's section offsets count from its own block
      const int64_t frame_dst = f.items[a * W + HMP_FI_DST];
      for (int j = a; j < b; ++j) {
        const int32_t* w = &f.items[j * W];
        int64_t v[HMP_FRAME_ITEM_WORDS];
        for (int k = 0; k < W; ++k) v[k] = w[k];
        const int kind = w[HMP_FI_KIND];
        const bool seg = kind == HMP_FK_EDGE_SEG, list = kind == HMP_FK_EDGE || seg;
        for (int k = HMP_FI_S0; k <= (list ? HMP_FI_S0 : HMP_FI_S3); ++k)
          if (v[k] >= 0) v[k] = v[k] - tb + B->frame_base[g];
        v[HMP_FI_DST] = base + (edge ? off[g] * 8 : off[g]) + (w[HMP_FI_DST] - frame_dst);
        if (list) {
          int64_t s_src = seg ? w[HMP_FI_S2] : 0, s_dst = seg ? w[HMP_FI_S3] : 0;  // a homogeneous frame's type offsets stay
          if (collated) {
            if (homog) { s_src += nptr(0, g); s_dst += nptr(0, g); }
            else { int ts, td; typed_ends(tensor, ts, td); s_src = nptr(ts, g); s_dst = nptr(td, g); }
          }
          v[HMP_FI_KIND] = HMP_FK_EDGE_SEG;
          v[HMP_FI_S1] = off[G];
          v[HMP_FI_S2] = s_src;
          v[HMP_FI_S3] = s_dst;
        }
        const int64_t next = j + 1 < ipf ? f.items[(j + 1) * W + HMP_FI_BLOCK0] : f.n_blocks;
        put_item(v, next - w[HMP_FI_BLOCK0]);
      }
    }
    a = b;
  }

  // ---- what a batch adds: `batch` of every node type (collated, typed), the offset vectors, the labels
  const int FB = HMP_FT_BATCH;
  auto const_item = [&](int tensor, int64_t dst, int64_t n, int64_t value) {
    const int64_t v[HMP_FRAME_ITEM_WORDS] = {HMP_FK_CONST, tensor, n, 1, dst, -1, -1, -1, -1, value, 8, 0};
    put_item(v, blocks_of(n));
  };
  auto i64_item = [&](int tensor, int64_t dst, int64_t n, int64_t s_src, int64_t s_idx) {
    const int64_t v[HMP_FRAME_ITEM_WORDS] = {HMP_FK_I64, tensor, n, 1, dst, B->own_base + s_src, -1, -1, s_idx < 0 ? -1 : B->own_base + s_idx, 8, 0, 0};
    put_item(v, blocks_of(n));
  };
  auto tensor_row = [&](int tensor, int64_t base, int64_t n) {
    const int64_t t4[4] = {tensor, base, n, 1};
    B->tensors.insert(B->tensors.end(), t4, t4 + 4);
  };
  if (collated && !homog)
    for (int t = 0; t < n_types; ++t) {
      const int64_t base = alloc(nptr(t, G) * 8);
      tensor_row(FB + HMP_FTB_BATCH + t, base, nptr(t, G));
      for (int g = 0; g < G; ++g) const_item(FB + HMP_FTB_BATCH + t, base + nptr(t, g) * 8, nptr(t, g + 1) - nptr(t, g), g);
    }
  if (!homog || !collated) {  // data.collate_homogeneous keeps no offset vector
    for (int t = 0; t < B->n_node_types; ++t) {
      const int64_t base = alloc((int64_t)(G + 1) * 8);
      tensor_row(FB + HMP_FTB_NODE_PTR + t, base, G + 1);
      i64_item(FB + HMP_FTB_NODE_PTR + t, base, G + 1, own_section(&B->node_ptr[(size_t)t * (G + 1)], (size_t)(G + 1) * 8), -1);
    }
    int e = 0;
    for (size_t q = 0; q < B->tensors.size() / 4 && e < B->n_edge_types; ++q) {
      const int64_t tensor = B->tensors[q * 4];
      if (tensor >= FB || B->tensors[q * 4 + 2] != 2) continue;
      const bool is_edge = homog ? (tensor == HMP_FT_HOMOG + 1 || tensor >= HMP_FT_HOMOG + 7)
                                 : ((tensor >= 8 && tensor < 12) || tensor >= HMP_FT_HTREE + 14);
      if (!is_edge) continue;
      const int64_t base = alloc((int64_t)(G + 1) * 8);
      tensor_row(FB + HMP_FTB_EDGE_PTR + e, base, G + 1);
      i64_item(FB + HMP_FTB_EDGE_PTR + e, base, G + 1, own_section(&B->edge_ptr[(size_t)e * (G + 1)], (size_t)(G + 1) * 8), -1);
      ++e;
    }
  }
  if (y) {
    // labels: int64 [n] per frame, aligned with the frame's INPUT arrays; a row-index section per labelled node type takes the
    // output row to its input node (kept / rooms, composed with object_orig / room_orig for the leaves of an H-tree)
    std::vector<int64_t> s_y(G);
    std::vector<std::vector<int64_t>> s_idx(G);
    for (int g = 0; g < G; ++g) {
      const hmp_frame& f = *B->frames[g];
      s_y[g] = own_section(y[input_of[g]], (size_t)f.n_input * 8);
      std::vector<int32_t> leaf_o, leaf_r;
      if (f.tree) {
        for (int32_t k : f.tree->object_orig) leaf_o.push_back(f.kept[k]);
        for (int32_t k : f.tree->room_orig) leaf_r.push_back(f.rooms[k]);
        s_idx[g] = {own_section(leaf_o.data(), leaf_o.size() * 4), own_section(leaf_r.data(), leaf_r.size() * 4), -1, -1,
                    own_section(f.kept.data(), f.kept.size() * 4), own_section(f.rooms.data(), f.rooms.size() * 4)};
      } else {
        s_idx[g] = {own_section(f.kept.data(), f.kept.size() * 4), own_section(f.rooms.data(), f.rooms.size() * 4)};
      }
    }
    if (homog) {  // one y over all nodes in store order, -1 on the clique rows
      const int64_t base = alloc(nptr(0, G) * 8);
      tensor_row(FB + HMP_FTB_Y, base, nptr(0, G));
      for (int g = 0; g < G; ++g) {
        int64_t row = nptr(0, g);
        for (int t = 0; t < n_types; ++t) {
          const int64_t n = type_rows[(size_t)g * n_types + t];
          if (s_idx[g][t] < 0) const_item(FB + HMP_FTB_Y, base + row * 8, n, -1);
          else i64_item(FB + HMP_FTB_Y, base + row * 8, n, s_y[g], s_idx[g][t]);
          row += n;
        }
      }
    } else {
      for (int t = 0; t < n_types; ++t) {
        if (s_idx[0][t] < 0) continue;  // clique nodes carry no label
        const int64_t base = alloc(nptr(t, G) * 8);
        tensor_row(FB + HMP_FTB_Y + t, base, nptr(t, G));
        for (int g = 0; g < G; ++g) i64_item(FB + HMP_FTB_Y + t, base + nptr(t, g) * 8, nptr(t, g + 1) - nptr(t, g), s_y[g], s_idx[g][t]);
      }
    }
  }

  // ---- the block: [group table | item table | sections]; section offsets so far count from the first section
  const int64_t n_items = (int64_t)B->items.size() / W;
  if (n_items > HMP_FRAME_BATCH_MAX_ITEMS) {
    snprintf(hmp::err_buf(), 512, "hmp_frame_batch_build: %lld items for %d graphs, the launch's tables hold %d (HMP_FRAME_BATCH_MAX_ITEMS): convert fewer frames at once",
             (long long)n_items, G, HMP_FRAME_BATCH_MAX_ITEMS);
    delete B;
    return HMP_E_ARG;
  }
  const int64_t n_groups = (n_items + HMP_FRAME_MAX_ITEMS - 1) / HMP_FRAME_MAX_ITEMS;
  const int64_t header = align16(n_groups * 4) + align16(n_items * W * 4);
  const int64_t staging = header + B->own_base + (int64_t)B->sections.size();
  if (too_large || B->arena_bytes > INT32_MAX || staging > INT32_MAX) return bail("batch too large: the arena or the staging block exceeds 2^31 - 1 bytes");
  for (int64_t i = 0; i < n_items; ++i) {
    const bool seg = B->items[i * W + HMP_FI_KIND] == HMP_FK_EDGE_SEG;
    for (int k = HMP_FI_S0; k <= (seg ? HMP_FI_S0 : HMP_FI_S3); ++k) {
      int32_t& s = B->items[i * W + k];
      if (s >= 0) s += (int32_t)header;
    }
  }
  for (int64_t g = 0; g < n_groups; ++g) B->groups.push_back(B->items[g * HMP_FRAME_MAX_ITEMS * W + HMP_FI_BLOCK0]);
  *out = B;
  return HMP_OK;
}

extern "C" int hmp_frame_batch_sizes(const hmp_frame_batch* b, int64_t* sizes) {
  if (!b || !sizes) { snprintf(hmp::err_buf(), 512, "hmp_frame_batch_sizes: null argument"); return HMP_E_ARG; }
  const int64_t n_items = (int64_t)b->items.size() / HMP_FRAME_ITEM_WORDS, n_groups = (int64_t)b->groups.size();
  for (int k = 0; k < HMP_FBS_COUNT; ++k) sizes[k] = 0;
  sizes[HMP_FBS_FRAMES] = (int64_t)b->graph_of_frame.size();
  sizes[HMP_FBS_GRAPHS] = (int64_t)b->frames.size();
  sizes[HMP_FBS_MAX_GRAPH_NODES] = b->max_graph_nodes;
  sizes[HMP_FBS_STAGING_BYTES] = n_items ? align16(n_groups * 4) + align16(n_items * HMP_FRAME_ITEM_WORDS * 4) + b->own_base + (int64_t)b->sections.size() : 0;
  sizes[HMP_FBS_ARENA_BYTES] = b->arena_bytes;
  sizes[HMP_FBS_ITEMS] = n_items;
  sizes[HMP_FBS_GROUPS] = n_groups;
  sizes[HMP_FBS_BLOCKS] = b->n_blocks;
  sizes[HMP_FBS_NODE_TYPES] = b->n_node_types;
  sizes[HMP_FBS_EDGE_TYPES] = b->n_edge_types;
  sizes[HMP_FBS_TENSORS] = (int64_t)b->tensors.size() / 4;
  return HMP_OK;
}

extern "C" int hmp_frame_batch_host_arrays(const hmp_frame_batch* b, int32_t* graph_of_frame, int64_t* node_ptr, int64_t* edge_ptr,
                                           int64_t* tensors) {
  if (!b) { snprintf(hmp::err_buf(), 512, "hmp_frame_batch_host_arrays: null batch"); return HMP_E_ARG; }
  auto put = [](void* dst, const void* src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
  put(graph_of_frame, b->graph_of_frame.data(), b->graph_of_frame.size() * 4);
  put(node_ptr, b->node_ptr.data(), b->node_ptr.size() * 8);
  put(edge_ptr, b->edge_ptr.data(), b->edge_ptr.size() * 8);
  put(tensors, b->tensors.data(), b->tensors.size() * 8);
  return HMP_OK;
}

extern "C" int hmp_frame_batch_pack(const hmp_frame_batch* b, void* staging, int64_t bytes) {
  auto bad = [](const char* m) { snprintf(hmp::err_buf(), 512, "hmp_frame_batch_pack: %s", m); return HMP_E_ARG; };
  if (!b || !staging) return bad("null argument");
  if (b->items.empty()) return bad("the batch has no frame with a room and a kept object: nothing to pack");
  const size_t groups = b->groups.size() * 4, groups_al = (size_t)align16((int64_t)groups);
  const size_t table = b->items.size() * 4, table_al = (size_t)align16((int64_t)table);
  const size_t header = groups_al + table_al, total = header + (size_t)b->own_base + b->sections.size();
  if (bytes < (int64_t)total) return bad("the staging buffer is smaller than HMP_FBS_STAGING_BYTES");
  uint8_t* p = (uint8_t*)staging;
  memcpy(p, b->groups.data(), groups);
  memset(p + groups, 0, groups_al - groups);
  memcpy(p + groups_al, b->items.data(), table);
  memset(p + groups_al + table, 0, table_al - table);
  size_t at = header;  // the gaps between sections are alignment padding: zeroed, so that a block is a function of its frames
  for (size_t g = 0; g < b->frames.size(); ++g) {
    const std::vector<uint8_t>& s = b->frames[g]->sections;
    const size_t start = header + (size_t)b->frame_base[g];
    memset(p + at, 0, start - at);
    if (!s.empty()) memcpy(p + start, s.data(), s.size());
    at = start + s.size();
  }
  memset(p + at, 0, header + (size_t)b->own_base - at);
  if (!b->sections.empty()) memcpy(p + header + b->own_base, b->sections.data(), b->sections.size());
  return HMP_OK;
}

extern "C" void hmp_frame_batch_destroy(hmp_frame_batch* b) { delete b; }
