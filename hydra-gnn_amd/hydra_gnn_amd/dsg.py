"""Scene-graph reader: spark_dsg JSON -> room-object graph -> the ``HeteroData`` the models read.

What the reference does per frame in ``GnnModel.convert_graph`` (``bin/room_classification_server:235-271``) and per file in
``Hydra_mp3d_data`` (``src/hydra_gnn/mp3d_dataset.py:130-284``), on the ``spark_dsg`` C++ bindings + numpy:

1. ``get_room_object_dsg`` (``preprocess_dsgs.py:228-292``): keep the rooms and their sibling edges; attach every object to the
   room of its parent place, or -- when that place has no room -- to the room of the nearest sibling place that has one; drop
   objects with neither.  Index bookkeeping over a few hundred nodes: done here on the host, in the reference's visiting order
   (ascending node id) so that ties resolve identically.
2. ``add_object_connectivity`` (``:191-225``): pairwise geometric predicates between the objects of a room, an O(n^2) Python
   loop -> ``hmp_object_edges_count`` / ``hmp_object_edges_fill`` (``csrc/dsg.hip``), float64, bit-exact edge set.
3. ``to_torch`` + ``fill_missing_edge_index`` (``mp3d_dataset.py:267-274``): ``x = [position | bbox size | semantic]``
   (``preprocess_dsgs.py:401-421``), the four ``EDGE_TYPES``; intra-layer edges in both directions, rooms_to_objects one edge
   per object and objects_to_rooms its flip.

Pinned by ``tests/golden/dsg_x8F5xyUWy9e_expected.npz`` -- the reference's own functions run on the reference's test graph
(``tests/golden/make_dsg_fixture.py``).  Not reproducible offline and therefore NOT built: the word2vec block of the object
features (the reference downloads GoogleNews vectors; pass ``semantic`` rows yourself or use the 6-d ``--remove_word2vec``
contract) and ``spark_dsg.add_bounding_boxes_to_layer`` (C++, absent): room boxes are taken as the AABB of the positions of
the room's places, stated here as an assumption.

``FramePipeline`` (below) is the same conversion as one native host stage, one upload and one launch (``csrc/frame.cpp``,
``csrc/frame.hip``), for the baseline graph and for its H-tree; the functions above it stay as they are and are its parity oracle.
"""
from __future__ import annotations

import ctypes as C
import json
import struct
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from .data import HTREE_EDGE_TYPES, HTREE_INIT_EDGE_TYPES, HTREE_POOL_EDGE_TYPES, Data, HeteroData

OBJECTS, PLACES, ROOMS, BUILDINGS = 2, 3, 4, 5
_STATIC = ("ObjectNodeAttributes", "PlaceNodeAttributes", "RoomNodeAttributes", "SemanticNodeAttributes")


class SceneGraph:
    """Static layers of a spark_dsg JSON dump: per node id / layer / position / bounding box / semantic label, and adjacency."""

    def __init__(self, ids, layer, pos, bb_min, bb_max, label, adj):
        self.ids, self.layer, self.pos, self.bb_min, self.bb_max, self.label, self.adj = ids, layer, pos, bb_min, bb_max, label, adj
        self.index = {int(v): i for i, v in enumerate(ids)}

    def of_layer(self, layer: int) -> np.ndarray:
        """node indices of a layer in ascending node id (the iteration order of spark_dsg's layer containers)"""
        idx = np.nonzero(self.layer == layer)[0]
        return idx[np.argsort(self.ids[idx], kind="stable")]

    def parent(self, i: int) -> int:
        """neighbour in a higher layer (a node has at most one; the lowest id wins if the dump holds several), -1: none"""
        ps = [j for j in self.adj[i] if self.layer[j] > self.layer[i]]
        return min(ps, key=lambda j: self.ids[j]) if ps else -1

    def siblings(self, i: int) -> List[int]:
        return sorted((j for j in self.adj[i] if self.layer[j] == self.layer[i]), key=lambda j: self.ids[j])


def load_dsg_json(src: Union[str, dict]) -> SceneGraph:
    """Parse a spark_dsg JSON dump (``DynamicSceneGraph.save``): static nodes only (agent poses share layer id 2 with the
    objects in the dump but live in a dynamic layer of their own), edges among them, mesh ignored."""
    raw = src if isinstance(src, dict) else json.load(open(src))
    nodes = [n for n in raw["nodes"] if n["attributes"].get("type") in _STATIC]
    ids = np.array([n["id"] for n in nodes], dtype=np.uint64)
    index = {int(v): i for i, v in enumerate(ids)}
    adj: List[set] = [set() for _ in nodes]
    for e in raw["edges"]:
        a, b = index.get(e["source"]), index.get(e["target"])
        if a is None or b is None or a == b:
            continue
        adj[a].add(b)
        adj[b].add(a)
    f = lambda key: np.array([key(n["attributes"]) for n in nodes], dtype=np.float64).reshape(len(nodes), 3)
    return SceneGraph(ids, np.array([n["layer"] for n in nodes], dtype=np.int64), f(lambda a: a["position"]),
                      f(lambda a: a["bounding_box"]["min"]), f(lambda a: a["bounding_box"]["max"]),
                      np.array([n["attributes"]["semantic_label"] for n in nodes], dtype=np.int64), adj)


class RoomObjectGraph:
    """``get_room_object_dsg`` result: rooms, kept objects (ascending id), each object's room, room-room edges."""

    def __init__(self, sg: SceneGraph):
        self.sg = sg
        rooms = sg.of_layer(ROOMS)
        room_index = {int(r): k for k, r in enumerate(rooms)}
        rr: List[Tuple[int, int]] = []
        seen = set()
        for r in rooms:  # preprocess_dsgs.py:236-246
            for s in sg.siblings(int(r)):
                key = (min(int(r), s), max(int(r), s))
                if key not in seen:
                    seen.add(key)
                    rr.append((room_index[int(r)], room_index[s]))
        kept, room_of, dropped = [], [], []
        for o in sg.of_layer(OBJECTS):  # :248-283
            place = sg.parent(int(o))
            if place < 0:
                dropped.append(int(o))
                continue
            room = sg.parent(place)
            if room < 0:
                cands = [s for s in sg.siblings(place) if sg.parent(s) >= 0]
                if not cands:
                    dropped.append(int(o))
                    continue
                dist = [float(np.linalg.norm(sg.pos[place] - sg.pos[s])) for s in cands]
                room = sg.parent(cands[int(np.argsort(dist, kind="stable")[0])])  # list.sort by distance is stable
            kept.append(int(o))
            room_of.append(room_index[room])
        self.rooms, self.objects = rooms, np.array(kept, dtype=np.int64)
        self.obj_room = np.array(room_of, dtype=np.int64)
        self.dropped = np.array(dropped, dtype=np.int64)
        self.rr_edges = np.array(rr, dtype=np.int64).reshape(-1, 2).T
        # room boxes: AABB of the positions of the room's places (assumption, see the module docstring)
        self.room_bb = np.zeros((len(rooms), 2, 3))
        for k, r in enumerate(rooms):
            kids = [j for j in sg.adj[int(r)] if sg.layer[j] == PLACES]
            if kids:
                p = sg.pos[kids]
                self.room_bb[k, 0], self.room_bb[k, 1] = p.min(0), p.max(0)

    @property
    def obj_pos(self):
        return self.sg.pos[self.objects]

    @property
    def obj_size(self):
        return self.sg.bb_max[self.objects] - self.sg.bb_min[self.objects]


def object_connectivity(rog: RoomObjectGraph, threshold_near: float = 2.0, max_near: float = 2.0, max_on: float = 0.2,
                        device="cuda:0") -> torch.Tensor:
    """``add_object_connectivity``: int64 ``[2, E]`` on the device, column = (object, earlier object of its room), objects
    indexed in ``rog.objects`` order; the reference's insertion order (by object, then by earlier object)."""
    lib = _lib.require_device()
    dev = torch.device(device)
    n = int(rog.objects.size)
    pos = torch.from_numpy(np.ascontiguousarray(rog.obj_pos)).to(dev)
    size = torch.from_numpy(np.ascontiguousarray(rog.obj_size)).to(dev)
    room = torch.from_numpy(rog.obj_room.astype(np.int32)).to(dev)
    count = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    offset = torch.empty(n + 1, dtype=torch.int32, device=dev)
    args = (pos.data_ptr(), size.data_ptr(), room.data_ptr(), n, float(threshold_near), float(max_near), float(max_on))
    with torch.cuda.device(dev):
        st = _lib.stream_ptr()
        _lib.check(lib.hmp_object_edges_count(*args, count.data_ptr(), offset.data_ptr(), st))
        total = int(offset[n].item())  # the one host round trip: the edge list is allocated to size
        edges = torch.empty((2, total), dtype=torch.int32, device=dev)
        _lib.check(lib.hmp_object_edges_fill(*args, offset.data_ptr(), edges.data_ptr() if total else None, total, st))
    return edges.to(torch.int64)


def to_hetero_data(rog: RoomObjectGraph, oo_edges: torch.Tensor, semantic: Optional[Dict[str, np.ndarray]] = None,
                   device="cuda:0", dtype=torch.float32) -> HeteroData:
    """``to_torch(use_heterogeneous=True)`` + ``fill_missing_edge_index``: x = [position | bbox size | semantic rows if given],
    ``pos``, ``label`` (Hydra semantic id), ``node_ids``; EDGE_TYPES per SURVEY Appendix B.1."""
    sg, dev = rog.sg, torch.device(device)
    g = HeteroData()

    def feats(pos, size, sem):
        cols = [pos, size] + ([sem] if sem is not None else [])
        return torch.from_numpy(np.concatenate(cols, 1)).to(dtype).to(dev)

    sem = semantic or {}
    g["objects"].x = feats(rog.obj_pos, rog.obj_size, sem.get("objects"))
    g["objects"].pos = torch.from_numpy(rog.obj_pos).to(dtype).to(dev)
    g["objects"].label = torch.from_numpy(sg.label[rog.objects]).to(dev)
    g["objects"].node_ids = torch.from_numpy(sg.ids[rog.objects].astype(np.int64)).to(dev)
    rpos = sg.pos[rog.rooms]
    g["rooms"].x = feats(rpos, rog.room_bb[:, 1] - rog.room_bb[:, 0], sem.get("rooms"))
    g["rooms"].pos = torch.from_numpy(rpos).to(dtype).to(dev)
    g["rooms"].label = torch.from_numpy(sg.label[rog.rooms]).to(dev)
    g["rooms"].node_ids = torch.from_numpy(sg.ids[rog.rooms].astype(np.int64)).to(dev)
    both = lambda e: torch.cat([e, e.flip(0)], dim=1)
    rr = torch.from_numpy(rog.rr_edges).to(dev)
    ro = torch.stack([torch.from_numpy(rog.obj_room), torch.arange(rog.objects.size)]).to(dev)
    g["objects", "objects_to_objects", "objects"].edge_index = both(oo_edges.to(dev))
    g["rooms", "rooms_to_rooms", "rooms"].edge_index = both(rr)
    g["rooms", "rooms_to_objects", "objects"].edge_index = ro
    g["objects", "objects_to_rooms", "rooms"].edge_index = ro.flip(0)
    return g


def frame_to_data(src: Union[str, dict], threshold_near: float = 1.5, max_near: float = 2.0, max_on: float = 0.2,
                  semantic: Optional[Dict[str, np.ndarray]] = None, device="cuda:0") -> Tuple[HeteroData, RoomObjectGraph]:
    """``GnnModel.convert_graph`` for the baseline hetero model with the server's thresholds
    (bin/room_classification_server:213-215): JSON frame -> device ``HeteroData`` (6-d features unless ``semantic`` rows are given)."""
    rog = RoomObjectGraph(load_dsg_json(src))
    oo = object_connectivity(rog, threshold_near, max_near, max_on, device)
    return to_hetero_data(rog, oo, semantic, device), rog


# ---------------------------------------------------------------------------------------------------------------------------------
# Frame pipeline (include/hydra_mp.h section 14): flat arrays -> HeteroData, host stage + one copy + one launch
# ---------------------------------------------------------------------------------------------------------------------------------
_OO, _RR = ("objects", "objects_to_objects", "objects"), ("rooms", "rooms_to_rooms", "rooms")
_RO, _OR = ("rooms", "rooms_to_objects", "objects"), ("objects", "objects_to_rooms", "rooms")
# output tensor number (HMP_FI_TENSOR) -> (store key, attribute); store creation follows to_hetero_data / generate_htree
_FRAME_TENSORS = (
    [(t, a) for t in ("objects", "rooms") for a in ("x", "pos", "label", "node_ids")]
    + [(e, "edge_index") for e in (_OO, _RR, _RO, _OR)] + [(e, "edge_attr") for e in (_OO, _RR, _RO, _OR)]
    + [(t, a) for t in ("object", "room") for a in ("x", "pos", "label")] + [("object-room", "x"), ("room-room", "x")]
    + [(t, a) for t in ("object_virtual", "room_virtual") for a in ("x", "pos", "label")]
    + [(tuple(e), "edge_index") for e in list(HTREE_EDGE_TYPES) + list(HTREE_INIT_EDGE_TYPES) + list(HTREE_POOL_EDGE_TYPES)]
)
assert len(_FRAME_TENSORS) == _lib.FT_COUNT
_HTREE_STORES = ["object", "room", "object-room", "room-room", "object_virtual", "room_virtual"]
# what relative positions on an H-tree add (``htree_relative_pos``), by output tensor number - HMP_FT_HTREL
_HTREL_TENSORS = [("object-room", "pos"), ("room-room", "pos")] + [(k, "edge_attr") for k, a in _FRAME_TENSORS[_lib.FT_HTREE:] if a == "edge_index"]
assert len(_HTREL_TENSORS) == _lib.FT_HTREL_COUNT


def _typed_tensor(t: int):
    """(store key, attribute) of output tensor number ``t`` of a typed frame"""
    return _HTREL_TENSORS[t - _lib.FT_HTREL] if t >= _lib.FT_HTREL else _FRAME_TENSORS[t]


def _relpos_mode(who: str, htree, relative_pos, htree_relative_pos, clique_dim) -> int:
    """``hmp_frame_build``'s ``relative_pos`` argument: 0, 1 (the baseline graph's) or ``HMP_FRAME_RELPOS_HTREE``.  Every refusal of
    the three keywords is made here, for the pipeline and the host-stage functions alike."""
    if htree_relative_pos and relative_pos:
        raise _lib.HydraMPError(f"{who}: htree_relative_pos and relative_pos exclude one another (relative_pos is the baseline "
                                f"graph's mode and is refused with htree)")
    if htree and relative_pos:
        raise _lib.HydraMPError(f"{who}: relative_pos is the baseline graph's mode and is refused with htree; relative positions on "
                                f"H-tree edges are htree_relative_pos=True")
    if not htree_relative_pos:
        return int(bool(relative_pos))
    if not htree:
        raise _lib.HydraMPError(f"{who}: htree_relative_pos is relative positions on H-tree edges: it needs htree=True")
    if 0 < int(clique_dim or 0) <= 3:
        raise _lib.HydraMPError(f"{who}: clique_dim {int(clique_dim)} leaves a clique no column once htree_relative_pos drops the three "
                                f"position columns: pass 0 or more than 3")
    return _lib.FRAME_RELPOS_HTREE
# attributes of the homogeneous Data, by output tensor number - HMP_FT_HOMOG
_HOMOG_TENSORS = ("x", "edge_index", "node_type", "edge_type", "room_mask", "edge_attr", "object_mask", "init_edge_index", "pool_edge_index")
assert len(_HOMOG_TENSORS) == _lib.FT_HOMOG_COUNT
# element class of an output tensor: how its (arena byte, rows, width) is viewed - float32 [rows, width], int64 [2, width] (an edge
# list), int64 [rows], bool [rows]
_F32, _EDGE, _I64, _BOOL = range(4)
_ELEMENT_CLASS = {"x": _F32, "pos": _F32, "edge_attr": _F32, "edge_index": _EDGE, "init_edge_index": _EDGE, "pool_edge_index": _EDGE,
                  "label": _I64, "node_ids": _I64, "node_type": _I64, "edge_type": _I64, "batch": _I64, "ptr": _I64, "y": _I64,
                  "room_mask": _BOOL, "object_mask": _BOOL}


def scene_arrays(sg: SceneGraph):
    """A ``SceneGraph`` as the flat arrays the frame pipeline reads: ``(ids, layer, pos, bb_min, bb_max, label, edges)`` with
    ``edges`` uint64 ``[2, m]`` of node ids, every undirected edge of ``sg.adj`` once."""
    pairs = [(i, j) for i, nb in enumerate(sg.adj) for j in nb if i < j]
    idx = np.array(pairs, dtype=np.int64).reshape(-1, 2).T
    return sg.ids, sg.layer, sg.pos, sg.bb_min, sg.bb_max, sg.label, np.asarray(sg.ids, dtype=np.uint64)[idx]


def _frame_args(ids, layer, pos, bb_min, bb_max, label, edges):
    """contiguous arrays of the C entry's types (kept alive by the caller for the duration of the call) and (n, m)"""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    n = int(ids.size)
    f3 = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(n, 3)
    edges = np.ascontiguousarray(edges, dtype=np.uint64).reshape(2, -1)
    arrays = (ids, np.ascontiguousarray(layer, dtype=np.int32).reshape(n), f3(pos), f3(bb_min), f3(bb_max),
              np.ascontiguousarray(label, dtype=np.int64).reshape(n), edges)
    return arrays, n, int(edges.shape[1])


def _frame_build(lib, arrays, n, m, thresholds, htree, relative_pos, sem_dim, n_labels, clique_dim, homogeneous=False,
                 remove_room_edges=False) -> C.c_void_p:
    ids, layer, pos, bb_min, bb_max, label, edges = arrays
    h = C.c_void_p()
    args = (n, ids.ctypes.data, layer.ctypes.data, pos.ctypes.data, bb_min.ctypes.data, bb_max.ctypes.data, label.ctypes.data, m,
            edges.ctypes.data, float(thresholds[0]), float(thresholds[1]), float(thresholds[2]), int(bool(htree)), int(relative_pos),
            int(sem_dim), int(n_labels), int(clique_dim or 0))
    if remove_room_edges:  # the room layer loses its edges in the native host stage (hmp_frame_build_flags)
        _lib.check(lib.hmp_frame_build_flags(*args, int(bool(homogeneous)), _lib.FRAME_NO_ROOM_EDGES, C.byref(h)))
    else:
        _lib.check((lib.hmp_frame_build_homogeneous if homogeneous else lib.hmp_frame_build)(*args, C.byref(h)))
    return h


def frame_host_stage(ids, layer, pos, bb_min, bb_max, label, edges, threshold_near: float = 1.5, max_near: float = 2.0,
                     max_on: float = 0.2, htree: bool = False, relative_pos: bool = False, sem_dim: int = 0, n_labels: int = 0,
                     clique_dim: Optional[int] = None, homogeneous: bool = False, htree_relative_pos: bool = False,
                     remove_room_edges: bool = False) -> Dict[str, object]:
    """The host stage of the frame pipeline on its own (no GPU involved; tests and diagnostics): ``hmp_frame_build``
    (``homogeneous``: ``hmp_frame_build_homogeneous``) and every accessor.  ``kept`` / ``dropped`` / ``rooms`` index the input
    arrays; ``items`` is the staging block's table (int32 ``[n_items, 12]``), ``block`` the packed block (uint8); ``empty``: no room
    or no kept object, nothing was laid out.  ``remove_room_edges``: as ``FramePipeline``'s."""
    lib = _lib.load()
    arrays, n, m = _frame_args(ids, layer, pos, bb_min, bb_max, label, edges)
    rel = _relpos_mode("frame_host_stage", htree, relative_pos, htree_relative_pos, clique_dim)
    h = _frame_build(lib, arrays, n, m, (threshold_near, max_near, max_on), htree, rel, sem_dim, n_labels, clique_dim, homogeneous,
                     remove_room_edges)
    try:
        sz = np.zeros(_lib.FS_COUNT, dtype=np.int64)
        _lib.check(lib.hmp_frame_sizes(h, sz.ctypes.data))
        n_o, n_r = int(sz[_lib.FS_KEPT]), int(sz[_lib.FS_ROOMS])
        out = {"sizes": sz, "kept": np.zeros(n_o, np.int32), "obj_room": np.zeros(n_o, np.int32),
               "dropped": np.zeros(int(sz[_lib.FS_DROPPED]), np.int32), "rooms": np.zeros(n_r, np.int32),
               "rr_edges": np.zeros((2, int(sz[_lib.FS_E_RR])), np.int32), "room_bb": np.zeros((n_r, 2, 3)),
               "oo_edges": np.zeros((2, int(sz[_lib.FS_E_OO])), np.int32)}
        p = lambda k: out[k].ctypes.data if out[k].size else None
        _lib.check(lib.hmp_frame_host_arrays(h, p("kept"), p("obj_room"), p("dropped"), p("rooms"), p("rr_edges"), p("room_bb"), p("oo_edges")))
        n_items = int(sz[_lib.FS_ITEMS])
        out["empty"] = n_items == 0
        block = np.zeros(int(sz[_lib.FS_STAGING_BYTES]), dtype=np.uint8)
        if n_items:
            _lib.check(lib.hmp_frame_pack(h, block.ctypes.data, block.size))
        out["block"] = block
        out["items"] = block[: n_items * _lib.FRAME_ITEM_WORDS * 4].view(np.int32).reshape(n_items, _lib.FRAME_ITEM_WORDS).copy()
    finally:
        lib.hmp_frame_destroy(h)
    return out


def save_frame_file(path: str, ids, layer, pos, bb_min, bb_max, label, edges, threshold_near: float = 1.5, max_near: float = 2.0,
                    max_on: float = 0.2, htree: bool = False, relative_pos: bool = False, sem_dim: int = 0, n_labels: int = 0,
                    clique_dim: int = 0, htree_relative_pos: bool = False) -> None:
    """Flat binary frame file of the stand-alone host-stage driver (``make -C csrc frame_check``; layout in csrc/frame_check.cpp)."""
    arrays, n, m = _frame_args(ids, layer, pos, bb_min, bb_max, label, edges)
    relative_pos = _relpos_mode("save_frame_file", htree, relative_pos, htree_relative_pos, clique_dim)
    with open(path, "wb") as f:
        f.write(b"HMPF" + struct.pack("<7iq3d", 1, n, int(htree), int(relative_pos), sem_dim, n_labels, clique_dim, m,
                                      threshold_near, max_near, max_on))
        for a in arrays:
            f.write(a.tobytes())


# ---- batches of frames (include/hydra_mp.h section 14, "batches of frames") ------------------------------------------------------
def _node_type_names(htree: bool, homogeneous: bool):
    return ["node"] if homogeneous else (list(_HTREE_STORES) if htree else ["objects", "rooms"])


def _edge_type_names(htree: bool, homogeneous: bool, relative_pos: bool = False):
    """edge types of a batch in the order of ``hmp_frame_batch_host_arrays``'s ``edge_ptr``"""
    if homogeneous:
        return ["edge_index", "init_edge_index", "pool_edge_index"] if htree else ["edge_index"]
    return [k for k, a in _FRAME_TENSORS[_lib.FT_HTREE if htree else 0:_lib.FT_COUNT if htree else _lib.FT_HTREE] if a == "edge_index"]


def _build_tensor_table(htree: bool, homogeneous: bool):
    """THE tensor table of a mode: ``table[t] = (store key or None, attribute, element class)`` for every output tensor number the
    library emits in it -- the mode's own range (typed baseline, typed H-tree with HMP_FT_HTREL, or HMP_FT_HOMOG) and HMP_FT_BATCH
    (``batch``, node ``ptr``, edge ``ptr``, ``y`` of this mode's node and edge types).  Every other number, another mode's included,
    holds ``(None, t, None)`` and is refused where a view is asked for."""
    nodes, edges = _node_type_names(htree, homogeneous), _edge_type_names(htree, homogeneous)
    FB = _lib.FT_BATCH
    if homogeneous:
        named = {_lib.FT_HOMOG + k: (None, a) for k, a in enumerate(_HOMOG_TENSORS)}
    elif htree:
        named = {t: _typed_tensor(t) for r in (range(_lib.FT_HTREE, _lib.FT_COUNT), range(_lib.FT_HTREL, _lib.FT_HTREL + _lib.FT_HTREL_COUNT)) for t in r}
    else:
        named = {t: _typed_tensor(t) for t in range(_lib.FT_HTREE)}
    named.update((FB + _lib.FTB_BATCH + k, (t, "batch")) for k, t in enumerate(nodes))
    named.update((FB + _lib.FTB_NODE_PTR + k, (t, "ptr")) for k, t in enumerate(nodes))
    named.update((FB + _lib.FTB_EDGE_PTR + k, (e, "ptr")) for k, e in enumerate(edges))
    named.update((FB + _lib.FTB_Y + k, (None if homogeneous else t, "y")) for k, t in enumerate(nodes))
    return [(*named[t], _ELEMENT_CLASS[named[t][1]]) if t in named else (None, t, None) for t in range(_lib.FT_HTREL + _lib.FT_HTREL_COUNT)]


_TENSOR_TABLES = {(ht, hg): _build_tensor_table(ht, hg) for ht in (False, True) for hg in (False, True)}


def _resolve_views(table, f32, i64, as_bool):
    """A tensor table resolved against one arena (its float32, int64 and bool views): ``resolved[t] = (store key, attribute, base
    view, shift of the arena byte to the base's element, leading dimension)`` -- leading dimension 0: ``[rows, width]``, 2: an edge
    list ``[2, width]``, None: ``[rows]`` -- or None for a number the mode does not define."""
    layout = {_F32: (f32, 2, 0), _EDGE: (i64, 3, 2), _I64: (i64, 3, None), _BOOL: (as_bool, 0, None)}
    return [None if cls is None else (key, attr) + layout[cls] for key, attr, cls in table]


def _arena_view(resolved, t: int, dst: int, rows: int, width: int):
    """The view of output tensor number ``t`` (``rows`` x ``width``) at arena byte ``dst``.  An undefined number is refused."""
    if not 0 <= t < len(resolved) or resolved[t] is None:
        raise _lib.HydraMPError(f"frame pipeline: output tensor number {t} is not a tensor of this mode")
    _, _, base, shift, lead = resolved[t]
    if lead is None:
        return torch.as_strided(base, (rows,), (1,), dst >> shift)
    return torch.as_strided(base, (lead or rows, width), (width, 1), dst >> shift)


def _label_pointers(y, n_frames: int, arrays):
    """(ctypes array of the frames' int64 label vectors or None, what keeps them alive)"""
    if y is None:
        return None, None
    if len(y) != n_frames:
        raise _lib.HydraMPError(f"y holds {len(y)} label vectors for {n_frames} frames")
    keep = []
    for i, v in enumerate(y):
        v = np.ascontiguousarray(v, dtype=np.int64).reshape(-1)
        if v.size != arrays[i][0].size:
            raise _lib.HydraMPError(f"y[{i}] holds {v.size} labels for the {arrays[i][0].size} nodes of its frame")
        keep.append(v)
    return (C.c_void_p * n_frames)(*[v.ctypes.data if v.size else None for v in keep]), keep


def _batch_build(lib, handles, form: int, y_ptrs) -> C.c_void_p:
    hb = C.c_void_p()
    _lib.check(lib.hmp_frame_batch_build(len(handles), (C.c_void_p * max(len(handles), 1))(*handles), int(form), y_ptrs, C.byref(hb)))
    return hb


def _batch_host_arrays(lib, hb) -> Dict[str, object]:
    """``hmp_frame_batch_sizes`` and ``hmp_frame_batch_host_arrays`` of a built batch"""
    sz = np.zeros(_lib.FBS_COUNT, dtype=np.int64)
    _lib.check(lib.hmp_frame_batch_sizes(hb, sz.ctypes.data))
    G = int(sz[_lib.FBS_GRAPHS])
    out = {"sizes": sz, "num_graphs": G, "max_graph_nodes": int(sz[_lib.FBS_MAX_GRAPH_NODES]),
           "graph_of_frame": np.zeros(int(sz[_lib.FBS_FRAMES]), np.int32),
           "node_ptr": np.zeros((int(sz[_lib.FBS_NODE_TYPES]), G + 1), np.int64),
           "edge_ptr": np.zeros((int(sz[_lib.FBS_EDGE_TYPES]), G + 1), np.int64),
           "tensors": np.zeros((int(sz[_lib.FBS_TENSORS]), 4), np.int64)}
    p = lambda k: out[k].ctypes.data if out[k].size else None
    _lib.check(lib.hmp_frame_batch_host_arrays(hb, p("graph_of_frame"), p("node_ptr"), p("edge_ptr"), p("tensors")))
    return out


def frame_batch_host_stage(frames, threshold_near: float = 1.5, max_near: float = 2.0, max_on: float = 0.2, htree: bool = False,
                           relative_pos: bool = False, sem_dim: int = 0, n_labels: int = 0, clique_dim: Optional[int] = None,
                           homogeneous: bool = False, form: int = _lib.FB_COLLATED, y=None,
                           htree_relative_pos: bool = False, remove_room_edges: bool = False) -> Dict[str, object]:
    """The host stage of ``FramePipeline.convert_batch`` / ``GraphStore.from_frames`` on its own (no GPU involved; the batch
    counterpart of ``frame_host_stage``).  ``frames``: a sequence of the 7-tuples ``frame_host_stage`` takes; ``form``:
    ``_lib.FB_COLLATED`` or ``_lib.FB_STORE``; ``y``: one int64 label vector per frame, aligned with its input arrays.  Returns
    ``sizes`` (``hmp_frame_batch_sizes``), ``num_graphs``, ``max_graph_nodes``, ``graph_of_frame``, ``node_ptr`` / ``edge_ptr``
    (int64 ``[types, graphs + 1]``), ``tensors`` (int64 ``[n, 4]``: number, arena offset, rows, width), ``frames`` (per frame
    ``kept`` / ``dropped`` / ``rooms``), and the packed ``block`` (uint8) with its ``groups`` and ``items`` tables."""
    lib = _lib.load()
    rel = _relpos_mode("frame_batch_host_stage", htree, relative_pos, htree_relative_pos, clique_dim)
    built, handles = [], []
    try:
        for fr in frames:
            arrays, n, m = _frame_args(*fr)
            built.append(arrays)
            handles.append(_frame_build(lib, arrays, n, m, (threshold_near, max_near, max_on), htree, rel, sem_dim, n_labels,
                                        clique_dim, homogeneous, remove_room_edges))
        y_ptrs, keep = _label_pointers(y, len(handles), built)
        hb = _batch_build(lib, handles, form, y_ptrs)
        try:
            out = _batch_host_arrays(lib, hb)
            sz = out["sizes"]
            out["frames"] = []
            fsz = np.zeros(_lib.FS_COUNT, dtype=np.int64)
            for h in handles:
                _lib.check(lib.hmp_frame_sizes(h, fsz.ctypes.data))
                kept, dropped, rooms = (np.zeros(int(fsz[k]), np.int32) for k in (_lib.FS_KEPT, _lib.FS_DROPPED, _lib.FS_ROOMS))
                q = lambda a: a.ctypes.data if a.size else None
                _lib.check(lib.hmp_frame_host_arrays(h, q(kept), None, q(dropped), q(rooms), None, None, None))
                out["frames"].append({"kept": kept, "dropped": dropped, "rooms": rooms, "items": int(fsz[_lib.FS_ITEMS])})
            n_items, n_groups = int(sz[_lib.FBS_ITEMS]), int(sz[_lib.FBS_GROUPS])
            block = np.zeros(int(sz[_lib.FBS_STAGING_BYTES]), dtype=np.uint8)
            if n_items:
                _lib.check(lib.hmp_frame_batch_pack(hb, block.ctypes.data, block.size))
            at = (n_groups * 4 + 15) & ~15
            out["block"] = block
            out["groups"] = block[: n_groups * 4].view(np.int32).copy()
            out["items"] = block[at: at + n_items * _lib.FRAME_ITEM_WORDS * 4].view(np.int32).reshape(n_items, _lib.FRAME_ITEM_WORDS).copy()
            del keep
        finally:
            lib.hmp_frame_batch_destroy(hb)
    finally:
        for h in handles:
            lib.hmp_frame_destroy(h)
    return out


class FramePipeline:
    """``GnnModel.convert_graph`` after the JSON step as ONE native host stage, ONE host-to-device copy and ONE launch.

    ``convert(ids, layer, pos, bb_min, bb_max, label, edges)`` takes the static layers of a scene graph as flat arrays (node ids
    uint64 ``[n]``, layer ``[n]``, float64 ``[n, 3]`` position and box corners, semantic label ``[n]``, undirected edges as node
    ids ``[2, m]``) and returns ``(HeteroData, info)``: what ``frame_to_data`` returns (``relative_pos=True``: after
    ``data.compute_relative_pos``), or with ``htree=True`` what ``htree.generate_htree(frame, clique_dim)`` makes of it.
    ``semantic_table`` (float32 ``[n_labels, sem_dim]``, resident on the device) appends ``table[label]`` to the objects' rows;
    rooms take no semantic block.  ``info`` = ``{"object_ids", "dropped_ids", "room_ids"}`` (numpy, the node ids the server maps
    labels back to).  Returns ``None`` for a frame without a room or without a kept object (the server's ``_check_graph`` refuses
    those) without touching the device.

    Every tensor of the result is a view of one device arena that ``hmp_frame_expand`` filled from one uploaded block; nothing
    synchronises (a pinned staging buffer is waited for only if the device is two frames behind).  The tensors are FRESH objects
    on every call -- ``predict`` re-uses a plan for the same edge tensor objects at the same ``_version``, and the kernel's writes
    do not bump ``_version`` -- and, like ``predict``'s pinned label buffer, a result is valid until the next ``convert`` of the
    same pipeline.  ``convert`` runs on torch's current stream and refuses a pipeline whose device is not the current one.  A
    pipeline has ONE device staging buffer and ONE arena, ordered by the stream alone: the stream of the first ``convert`` that
    enqueues anything is the pipeline's, and a ``convert`` under another current stream is refused (keep a pipeline per stream).

    ``htree=True, htree_relative_pos=True`` is the H-tree of the reference's GAT_edge models (``Hydra_mp3d_htree_data`` after
    ``compute_relative_pos``, which the server runs behind ``nx_htree_to_torch``): what ``data.compute_relative_pos`` makes of
    ``htree.generate_htree(frame, clique_dim, clique_pos=True)``.  Every node type's ``x`` loses its three leading columns (a clique
    row is ``clique_dim - 3`` zeros; ``clique_dim`` 1..3 is refused), the two clique types carry ``pos`` (the mean position of their
    member rooms), and every one of the 15 edge types carries ``edge_attr = pos[dst] - pos[src]``, bit-equal to that difference of
    the ``pos`` tensors of the same result (a pool edge's is ``+0.0``).  With ``homogeneous=True`` the ``edge_attr`` of the ten tree
    edge types follows ``edge_index``, as ``data.heterogeneous_htree_to_homogeneous`` keeps it.  ``relative_pos`` is the baseline
    graph's mode: with ``htree`` it stays refused, and ``htree_relative_pos`` without ``htree`` or together with it is refused too.

    ``homogeneous=True`` is ``convert_graph``'s ``if self.model_info.homogeneous: data.to_homogeneous()`` in the same host stage,
    copy and launch: ``convert`` returns ``(data.Data, info)`` with what ``HomogeneousNetwork`` / ``HomogeneousNeuralTreeNetwork``
    read.  Baseline: ``data.heterogeneous_data_to_homogeneous`` of the frame above plus ``room_mask`` (``x`` zero-padded to the
    widest type, ``edge_index``, ``node_type``, ``edge_type``, ``room_mask``, and ``edge_attr`` with ``relative_pos``); with
    ``htree=True``: ``data.heterogeneous_htree_to_homogeneous`` of the H-tree above (``x``, ``node_type``, ``edge_index`` /
    ``edge_type`` of the ten tree edge types, ``init_edge_index``, ``pool_edge_index``, ``room_mask``, ``object_mask``).  The masks
    are ``torch.bool`` views of arena bytes; a frame carries no ``y``.  ``info["room_ids"]`` is in the order of the ``room_mask``
    rows.  Everything said above about views, fresh objects, streams and ``None`` holds for it.

    ``remove_room_edges=True`` is the reference's ``Hydra_mp3d_data.remove_room_edges_in_dsg`` (``mp3d_dataset.py:203-208``, the ``noRE``
    configurations) in the native host stage: the room-room edges are dropped before anything reads them, so ``rooms_to_rooms`` is
    ``[2, 0]`` and an H-tree is built from the edgeless room layer (every room its own component, no ``room-room`` clique).  It holds in
    every mode above, typed and homogeneous, for ``convert``, ``convert_batch`` and ``GraphStore.from_frames``.

    ``convert_batch(frames, y=None)`` converts MANY frames with one host stage, one upload and one launch into the collated batch
    (``data.collate`` / ``data.collate_homogeneous`` of the single results), in every mode above; ``store.GraphStore.from_frames``
    builds a device-resident store the same way.
    """

    def __init__(self, device="cuda:0", semantic_table=None, htree: bool = False, relative_pos: bool = False,
                 clique_dim: Optional[int] = None, threshold_near: float = 1.5, max_near: float = 2.0, max_on: float = 0.2,
                 homogeneous: bool = False, htree_relative_pos: bool = False, remove_room_edges: bool = False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HydraMPError(f"FramePipeline needs a gfx950 device, not {self.device}: hydra_gnn_amd has no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", 0)
        self._relpos = _relpos_mode("FramePipeline", htree, relative_pos, htree_relative_pos, clique_dim)
        self.htree, self.relative_pos, self.clique_dim = bool(htree), bool(relative_pos), int(clique_dim or 0)
        self.htree_relative_pos = bool(htree_relative_pos)
        self.homogeneous = bool(homogeneous)
        self.remove_room_edges = bool(remove_room_edges)
        self.thresholds = (float(threshold_near), float(max_near), float(max_on))
        self._lib = _lib.load()
        self._table_host, self._table = None, None
        self.sem_dim, self.n_labels = 0, 0
        if semantic_table is not None:
            t = torch.as_tensor(semantic_table).detach().to(torch.float32).contiguous()
            if t.dim() != 2 or t.size(0) < 1 or t.size(1) < 1:
                raise _lib.HydraMPError("FramePipeline: semantic_table must be a float32 [n_labels, sem_dim] array")
            self._table_host, self.n_labels, self.sem_dim = t, int(t.size(0)), int(t.size(1))
        self._sizes = np.zeros(_lib.FS_COUNT, dtype=np.int64)
        # device buffers appear with the first frame that has something to convert (an empty frame never touches the device)
        self._pinned, self._pinned_np, self._events, self._slot = [None, None], [None, None], [None, None], 0
        self._d_staging = self._arena = self._resolved = None  # _resolved: the table against the arena (_resolve_views)
        self._tensors = _TENSOR_TABLES[self.htree, self.homogeneous]
        self._stream = None  # hipStream_t of the first convert that enqueued work
        self._batch_max_items = _lib.FRAME_BATCH_MAX_ITEMS  # items of one convert_batch launch

    def _ensure(self, staging_bytes: int, arena_bytes: int) -> None:
        if self._table is None and self._table_host is not None:
            self._lib = _lib.require_device()
            self._table = self._table_host.to(self.device)
        if self._d_staging is None or self._d_staging.numel() < staging_bytes:
            cap = max(1 << 16, 2 * staging_bytes)
            self._lib = _lib.require_device()
            self._d_staging = torch.empty(cap, dtype=torch.uint8, device=self.device)
            for k in range(2):
                self._pinned[k] = torch.empty(cap, dtype=torch.uint8).pin_memory()
                self._pinned_np[k] = self._pinned[k].numpy().view(np.int32)
                self._events[k] = torch.cuda.Event()
        if self._arena is None or self._arena.numel() < arena_bytes:
            self._arena = torch.empty(max(1 << 18, 2 * arena_bytes), dtype=torch.uint8, device=self.device)
            self._resolved = _resolve_views(self._tensors, self._arena.view(torch.float32), self._arena.view(torch.int64),
                                            self._arena.view(torch.bool))

    def _stage_and_expand(self, pack, expand: str, h, staging_bytes: int, arena_bytes: int, n_items: int, n_blocks: int) -> int:
        """The device half of ``convert`` / ``convert_batch``: ``pack`` the block of ``h`` into the next pinned buffer, ONE upload, ONE
        launch of ``expand`` on the pipeline's stream.  Returns the pinned slot that holds the block."""
        if torch.cuda.current_device() != self.device.index:
            raise _lib.HydraMPError(f"FramePipeline.convert: the pipeline lives on {self.device}, the current device is "
                                    f"cuda:{torch.cuda.current_device()}")
        stream = _lib.stream_ptr()
        if self._stream is None:
            self._stream = stream
        elif stream != self._stream:
            raise _lib.HydraMPError("FramePipeline.convert: the current stream is not the stream of this pipeline's earlier frames; "
                                    "its staging buffer and arena are ordered by one stream (keep a pipeline per stream)")
        self._ensure(staging_bytes, arena_bytes)
        lib = self._lib
        slot = self._slot = self._slot ^ 1
        if not self._events[slot].query():  # the upload that last read this pinned buffer has not run yet
            self._events[slot].synchronize()
        pin = self._pinned[slot]
        _lib.check(pack(h, pin.data_ptr(), staging_bytes))
        self._d_staging[:staging_bytes].copy_(pin[:staging_bytes], non_blocking=True)
        self._events[slot].record()
        _lib.check(getattr(lib, expand)(self._d_staging.data_ptr(), self._arena.data_ptr(),
                                        self._table.data_ptr() if self._table is not None else None, self.sem_dim, n_items, n_blocks,
                                        stream))
        return slot

    def convert_scene(self, sg: SceneGraph):
        """``convert`` on a ``SceneGraph`` (``load_dsg_json``): ``sg.adj`` is flattened to an edge array first."""
        return self.convert(*scene_arrays(sg))

    def convert(self, ids, layer, pos, bb_min, bb_max, label, edges):
        lib = self._lib
        arrays, n, m = _frame_args(ids, layer, pos, bb_min, bb_max, label, edges)
        h = _frame_build(lib, arrays, n, m, self.thresholds, self.htree, self._relpos, self.sem_dim, self.n_labels, self.clique_dim,
                         self.homogeneous, self.remove_room_edges)
        try:
            sz = self._sizes
            _lib.check(lib.hmp_frame_sizes(h, sz.ctypes.data))
            n_items = int(sz[_lib.FS_ITEMS])
            if n_items == 0:
                return None
            n_o, n_r, n_d = int(sz[_lib.FS_KEPT]), int(sz[_lib.FS_ROOMS]), int(sz[_lib.FS_DROPPED])
            slot = self._stage_and_expand(lib.hmp_frame_pack, "hmp_frame_expand", h, int(sz[_lib.FS_STAGING_BYTES]),
                                          int(sz[_lib.FS_ARENA_BYTES]), n_items, int(sz[_lib.FS_BLOCKS]))
            lib = self._lib
            kept, dropped, rooms = np.empty(n_o, np.int32), np.empty(n_d, np.int32), np.empty(n_r, np.int32)
            _lib.check(lib.hmp_frame_host_arrays(h, kept.ctypes.data, None, dropped.ctypes.data if n_d else None, rooms.ctypes.data,
                                                 None, None, None))
            items = self._pinned_np[slot][: n_items * _lib.FRAME_ITEM_WORDS].reshape(n_items, _lib.FRAME_ITEM_WORDS).tolist()
        finally:
            lib.hmp_frame_destroy(h)
        ids = arrays[0]
        info = {"object_ids": ids[kept], "dropped_ids": ids[dropped], "room_ids": ids[rooms]}
        if self.homogeneous:
            return self._homogeneous_data(items), info
        g = HeteroData()
        if self.htree:
            for t in _HTREE_STORES:
                g[t]
        resolved, strided = self._resolved, torch.as_strided
        try:
            for _, tensor, n_rows, width, dst, *_ in items:  # the body of _arena_view inline: one lookup and one as_strided per item
                key, attr, base, shift, lead = resolved[tensor]
                if lead is None:
                    t = strided(base, (n_rows,), (1,), dst >> shift)
                else:
                    t = strided(base, (lead or n_rows, width), (width, 1), dst >> shift)
                setattr(g[key], attr, t)
        except (TypeError, IndexError):
            _arena_view(resolved, tensor, dst, n_rows, width)  # an undefined number is refused by name
            raise
        return g, info

    # ---- many frames per launch ----------------------------------------------------------------------------------------------------
    def convert_batch(self, frames, y=None):
        """``frames``: a sequence of the 7-tuples ``convert`` takes -> ``(batch, infos)`` with ONE host stage, ONE pinned block, ONE
        upload and ONE launch for all of them.  ``batch`` is what ``data.collate([clone of convert(f)[0] for f in frames]).to(device)``
        is (``homogeneous``: ``data.collate_homogeneous``), bit for bit and attribute for attribute: ``num_graphs``,
        ``max_graph_nodes``, ``batch`` / ``ptr`` of every node type, ``ptr`` / ``ptr_version`` of every edge type.  ``y``: one int64
        label vector per frame, aligned with the frame's input arrays; it becomes ``objects.y`` / ``rooms.y`` (H-tree: ``object.y``,
        ``room.y``, ``object_virtual.y``, ``room_virtual.y``; homogeneous: one ``y``, -1 on clique rows).  ``infos[i]`` is ``convert``'s
        info dict plus ``"graph"`` (the frame's position in the batch), or ``None`` for a frame without a room or a kept object, which
        the batch skips; with no frame left the result is ``(None, infos)`` and the device is not touched.  Everything ``convert``
        says about views of the arena, fresh tensor objects, the two pinned buffers, the one stream and the lifetime of a result
        (until the next ``convert`` / ``convert_batch``) holds.  More items than one launch's tables hold
        (``_lib.FRAME_BATCH_MAX_ITEMS``) is refused: convert fewer frames at once."""
        built, infos = self._build_frames(frames)
        try:
            run = self._run_batch(built, y, _lib.FB_COLLATED, infos)
        finally:
            for h, _ in built:
                self._lib.hmp_frame_destroy(h)
        if run is None:
            return None, infos
        tensors, host = run
        return self._collated(tensors, host), infos

    def _build_frames(self, frames):
        """host stage of every frame: ([(handle, arrays)], infos) -- the caller destroys the handles"""
        lib, built, infos = self._lib, [], []
        sz = self._sizes
        try:
            for fr in frames:
                arrays, n, m = _frame_args(*fr)
                h = _frame_build(lib, arrays, n, m, self.thresholds, self.htree, self._relpos, self.sem_dim, self.n_labels,
                                 self.clique_dim, self.homogeneous, self.remove_room_edges)
                built.append((h, arrays))
                _lib.check(lib.hmp_frame_sizes(h, sz.ctypes.data))
                if int(sz[_lib.FS_ITEMS]) == 0:
                    infos.append(None)
                    continue
                n_o, n_r, n_d = int(sz[_lib.FS_KEPT]), int(sz[_lib.FS_ROOMS]), int(sz[_lib.FS_DROPPED])
                kept, dropped, rooms = np.empty(n_o, np.int32), np.empty(n_d, np.int32), np.empty(n_r, np.int32)
                _lib.check(lib.hmp_frame_host_arrays(h, kept.ctypes.data, None, dropped.ctypes.data if n_d else None, rooms.ctypes.data,
                                                     None, None, None))
                ids = arrays[0]
                infos.append({"object_ids": ids[kept], "dropped_ids": ids[dropped], "room_ids": ids[rooms]})
        except Exception:
            for h, _ in built:
                lib.hmp_frame_destroy(h)
            raise
        return built, infos

    def _batch_capacity(self, handle, form: int, with_y: bool) -> int:
        """frames with items that fit one launch's tables (``_batch_max_items``: a test hook, at most the library's limit)"""
        per_frame, per_batch = C.c_int32(), C.c_int32()
        _lib.check(self._lib.hmp_frame_batch_items_needed(handle, form, int(with_y), C.byref(per_frame), C.byref(per_batch)))
        return (min(self._batch_max_items, _lib.FRAME_BATCH_MAX_ITEMS) - per_batch.value) // per_frame.value

    def _run_batch(self, built, y, form: int, infos):
        """batch host stage + upload + launch over built frames -> ({tensor number: view of the arena}, host arrays); None if no
        frame has items.  Sets ``infos[i]["graph"]``."""
        lib = self._lib
        live = [i for i, info in enumerate(infos) if info is not None]
        if not live:
            return None
        if len(live) > self._batch_capacity(built[live[0]][0], form, y is not None):
            raise _lib.HydraMPError(f"FramePipeline.convert_batch: {len(live)} frames need more items than one launch's tables hold "
                                    f"({min(self._batch_max_items, _lib.FRAME_BATCH_MAX_ITEMS)}, HMP_FRAME_BATCH_MAX_ITEMS): convert "
                                    f"fewer frames at once")
        y_ptrs, keep = _label_pointers(y, len(built), [a for _, a in built])
        hb = _batch_build(lib, [h for h, _ in built], form, y_ptrs)
        try:
            host = _batch_host_arrays(lib, hb)
            sz = host["sizes"]
            self._stage_and_expand(lib.hmp_frame_batch_pack, "hmp_frame_expand_batch", hb, int(sz[_lib.FBS_STAGING_BYTES]),
                                   int(sz[_lib.FBS_ARENA_BYTES]), int(sz[_lib.FBS_ITEMS]), int(sz[_lib.FBS_BLOCKS]))
        finally:
            self._lib.hmp_frame_batch_destroy(hb)
        del keep
        for i, g in enumerate(host["graph_of_frame"].tolist()):
            if infos[i] is not None:
                infos[i]["graph"] = g
        resolved = self._resolved
        return {t: _arena_view(resolved, t, dst, rows, width) for t, dst, rows, width in host["tensors"].tolist()}, host

    def _collated(self, tensors, host):
        """the views of a collated batch as the HeteroData / Data that data.collate / data.collate_homogeneous build"""
        FB, table = _lib.FT_BATCH, self._tensors
        if self.homogeneous:
            d = Data()
            for t in sorted(tensors):
                key, attr, _ = table[t]
                assert key is None, (t, key, attr)  # a collated Data carries no offset vectors
                setattr(d, attr, tensors[t])
            d.num_graphs = host["num_graphs"]
            return d
        g = HeteroData()
        g.num_graphs = host["num_graphs"]
        node_types = _node_type_names(self.htree, False)
        edge_types = _edge_type_names(self.htree, False)
        for t in node_types:
            g[t]
        for t in sorted(k for k in tensors if k < FB or k >= _lib.FT_HTREL):
            key, attr, _ = table[t]
            setattr(g[key], attr, tensors[t])
            if attr == "edge_index":
                g[key].ptr = tensors[FB + _lib.FTB_EDGE_PTR + edge_types.index(key)]
                g[key].ptr_version = int(tensors[t]._version)
        for k, t in enumerate(node_types):
            if FB + _lib.FTB_Y + k in tensors:
                g[t].y = tensors[FB + _lib.FTB_Y + k]
            g[t].batch = tensors[FB + _lib.FTB_BATCH + k]
            g[t].ptr = tensors[FB + _lib.FTB_NODE_PTR + k]
        g.max_graph_nodes = host["max_graph_nodes"]
        return g

    def _homogeneous_data(self, items) -> Data:
        """Views of the arena for the tensors of a homogeneous frame.  A tensor is written by one item per segment: its first item
        starts where the tensor does, its rows (edge tensors: the pitch every segment carries) add up to the tensor's."""
        at, n_rows, pitch = {}, {}, {}
        for kind, tensor, rows, width, dst, _, s1, *_ in items:
            if tensor not in at:
                at[tensor], n_rows[tensor], pitch[tensor] = dst, 0, s1 if kind == _lib.FK_EDGE_SEG else width
            n_rows[tensor] += rows
        resolved, table = self._resolved, self._tensors
        d = Data()
        for tensor in sorted(at):
            setattr(d, table[tensor][1], _arena_view(resolved, tensor, at[tensor], n_rows[tensor], pitch[tensor]))
        return d
