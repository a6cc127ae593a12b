"""Shared cases of the frame-pipeline tests (tests/test_frame_host.py, tests/test_gpu_frame_pipeline.py): scene graphs as flat
arrays, the ``dsg.SceneGraph`` built from the same arrays (the comparison), the existing conversion path they are checked against,
and a numpy reading of the staging block (what ``hmp_frame_expand`` is specified to write, item by item)."""
import os

import numpy as np
import torch

from hydra_gnn_amd import _lib, dsg, workloads
from hydra_gnn_amd.data import compute_relative_pos
from oracle import dsg_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JSON = os.path.join(GOLD, "dsg_x8F5xyUWy9e.json")
EXP = os.path.join(GOLD, "dsg_x8F5xyUWy9e_expected.npz")
THRESHOLDS = (1.5, 2.0, 0.2)  # the server's (bin/room_classification_server:213-215)
N_LABELS = 41
SIZES = [(1, 1), (7, 2), (65, 1), (300, 3)]  # (objects, rooms)


def scene_graph(arrays) -> dsg.SceneGraph:
    """``dsg.SceneGraph`` from flat arrays, with ``load_dsg_json``'s edge rules (unknown endpoints and self edges are ignored)"""
    ids, layer, pos, bb_min, bb_max, label, edges = arrays
    index = {int(v): i for i, v in enumerate(ids)}
    adj = [set() for _ in ids]
    for a, b in zip(edges[0].tolist(), edges[1].tolist()):
        a, b = index.get(a), index.get(b)
        if a is None or b is None or a == b:
            continue
        adj[a].add(b)
        adj[b].add(a)
    return dsg.SceneGraph(np.asarray(ids, dtype=np.uint64), np.asarray(layer, dtype=np.int64), np.asarray(pos, dtype=np.float64),
                          np.asarray(bb_min, dtype=np.float64), np.asarray(bb_max, dtype=np.float64), np.asarray(label, dtype=np.int64), adj)


def fixture_arrays():
    return dsg.scene_arrays(dsg.load_dsg_json(JSON))


def special_arrays():
    """The (7, 2) frame plus every irregular case of ``get_room_object_dsg``: an object without a place; a place without a room
    whose sibling places have rooms at equal distance (the lower sibling id wins) and at unequal distance (the nearer wins); an
    object whose place has neither a room nor such a sibling; a room without places; a room without objects; duplicate and self
    edges; an edge to an unknown node id."""
    ids, layer, pos, bb_min, bb_max, label, edges = [a.tolist() for a in workloads.synthetic_scene(7, 2, seed=5)]
    sym = lambda c, i: (ord(c) << 56) + i
    e = list(zip(edges[0], edges[1]))

    def node(i, lay, p, lab=3):
        ids.append(i), layer.append(lay), pos.append(list(p)), bb_min.append([p[0] - 0.3, p[1] - 0.2, p[2] - 0.1])
        bb_max.append([p[0] + 0.3, p[1] + 0.2, p[2] + 0.4]), label.append(lab)
        return i

    r0, r1 = sym("R", 0), sym("R", 1)
    node(sym("O", 100), 2, (0, 0, 0))  # no place
    # equal distance: siblings at x = +1 (higher id, room 0) and x = -1 (lower id, room 1)
    pa, hi, lo = node(sym("p", 100), 3, (20, 0, 0)), node(sym("p", 102), 3, (21, 0, 0)), node(sym("p", 101), 3, (19, 0, 0))
    e += [(pa, hi), (pa, lo), (hi, r0), (lo, r1), (node(sym("O", 101), 2, (20, 0.1, 0)), pa), (node(sym("O", 102), 2, (20, 0.2, 0.3)), pa)]
    # unequal distance: the lower sibling id is farther
    pb, far, near = node(sym("p", 110), 3, (30, 0, 0)), node(sym("p", 111), 3, (32, 0, 0)), node(sym("p", 112), 3, (30.5, 0, 0))
    e += [(pb, far), (pb, near), (far, r0), (near, r1), (node(sym("O", 103), 2, (30, 0, 0.2)), pb)]
    # neither: the place has one sibling, which has no room either
    pc, pd = node(sym("p", 120), 3, (40, 0, 0)), node(sym("p", 121), 3, (41, 0, 0))
    e += [(pc, pd), (node(sym("O", 104), 2, (40, 0, 0)), pc)]
    r2 = node(sym("R", 2), 4, (50, 0, 0), 7)  # a room without places (and so without objects)
    r3 = node(sym("R", 3), 4, (60, 0, 0), 8)  # a room with a place and no object
    e += [(r1, r2), (r2, r3), (r3, node(sym("p", 130), 3, (60, 1, 0)))]
    e += [e[0], (e[1][1], e[1][0]), (r0, r0), (pa, pa), (r0, sym("R", 99)), (sym("x", 1), sym("x", 2))]  # duplicates, self, unknown
    return (np.array(ids, dtype=np.uint64), np.array(layer, dtype=np.int32), np.array(pos, dtype=np.float64), np.array(bb_min, dtype=np.float64),
            np.array(bb_max, dtype=np.float64), np.array(label, dtype=np.int64), np.array(e, dtype=np.uint64).reshape(-1, 2).T.copy())


_CACHE = {}


def frame(name):
    """flat arrays of a named case: "fixture", "special", or (objects, rooms)"""
    if name not in _CACHE:
        if name == "fixture":
            _CACHE[name] = fixture_arrays()
        elif name == "special":
            _CACHE[name] = special_arrays()
        else:
            _CACHE[name] = workloads.synthetic_scene(name[0], name[1], seed=11 + name[0])
    return _CACHE[name]


def semantic_table():
    """a random float32 table of 41 rows (the word2vec block is a download: the table is whatever the caller passes)"""
    if "table" not in _CACHE:
        _CACHE["table"] = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).normal(0, 1, (N_LABELS, 300)).astype(np.float32))
    return _CACHE["table"]


def existing_frame(arrays, sem: bool, relative_pos: bool = False, device="cpu"):
    """The existing path on the same arrays: RoomObjectGraph + object edges + to_hetero_data (+ compute_relative_pos).  On the CPU the
    edges come from the oracle's predicates, on a GPU from ``dsg.object_connectivity`` (= ``dsg.frame_to_data``)."""
    rog = dsg.RoomObjectGraph(scene_graph(arrays))
    if str(device) == "cpu":
        oo = torch.from_numpy(dsg_ref.object_edges(rog.obj_pos, rog.obj_size, rog.obj_room, *THRESHOLDS))
    else:
        oo = dsg.object_connectivity(rog, *THRESHOLDS, device=device)
    semantic = {"objects": semantic_table().numpy()[rog.sg.label[rog.objects]]} if sem else None
    data = dsg.to_hetero_data(rog, oo, semantic, device)
    if relative_pos:
        compute_relative_pos(data)
    return data, rog


# ---- a numpy reading of the staging block: what the launch is specified to write, item by item -------------------------------
def _ends(e, variant, n, col):
    if variant == 0:
        return e[col], e[n + col]
    if variant == 1:
        return (e[col], e[n + col]) if col < n else (e[col], e[col - n])
    if variant == 2:
        return e[n + col], e[col]
    return (e[col], col) if variant == 3 else (col, e[col])


def read_block(block: np.ndarray, items: np.ndarray, table=None):
    """{tensor number: array} from a packed block; every source read is checked to lie inside the block"""

    def sec(off, dtype, count):
        nbytes = count * np.dtype(dtype).itemsize
        assert off >= 0 and off % 16 == 0 and off + nbytes <= block.size, (off, count, block.size)
        return block[off:off + nbytes].view(dtype)

    out = {}
    for kind, tensor, rows, width, dst, s0, s1, s2, s3, p0, p1, _ in items.tolist():
        idx = sec(s3, np.int32, rows) if s3 >= 0 else np.arange(rows, dtype=np.int32)
        n_src = int(idx.max()) + 1 if rows else 0
        if kind == _lib.FK_FEAT:
            cols = [sec(s0, np.float64, 3 * n_src).reshape(-1, 3)[idx]] if p0 else []
            cols.append(sec(s1, np.float64, 3 * n_src).reshape(-1, 3)[idx])
            x = np.concatenate(cols, 1).astype(np.float32)
            if p1:
                x = np.concatenate([x, table[sec(s2, np.int32, n_src)[idx]]], 1)
            assert x.shape == (rows, width)
            out[tensor] = x
        elif kind == _lib.FK_POS:
            out[tensor] = sec(s0, np.float64, 3 * n_src).reshape(-1, 3)[idx].astype(np.float32)
        elif kind == _lib.FK_I64:
            out[tensor] = sec(s0, np.int32 if p0 == 4 else np.int64, n_src)[idx].astype(np.int64)
        elif kind in (_lib.FK_EDGE, _lib.FK_EATTR):
            n_out = width if kind == _lib.FK_EDGE else rows
            e = sec(s0, np.int32, (2 if p0 <= 2 else 1) * p1)
            ends = np.array([_ends(e, p0, p1, c) for c in range(n_out)], dtype=np.int64).reshape(-1, 2)
            if kind == _lib.FK_EDGE:
                out[tensor] = ends.T.copy()
            else:
                ps = sec(s1, np.float64, 3 * (int(ends[:, 0].max()) + 1 if n_out else 0)).reshape(-1, 3).astype(np.float32)
                pd = sec(s2, np.float64, 3 * (int(ends[:, 1].max()) + 1 if n_out else 0)).reshape(-1, 3).astype(np.float32)
                out[tensor] = pd[ends[:, 1]] - ps[ends[:, 0]]
        elif kind == _lib.FK_CLIQUE:
            ptr = sec(s0, np.int32, rows + 1)
            mem = sec(s1, np.int32, int(ptr[-1]))
            rpos = sec(s2, np.float64, 3 * (int(mem.max()) + 1 if mem.size else 0)).reshape(-1, 3).astype(np.float32)
            x = np.zeros((rows, width), dtype=np.float32)
            for q in range(rows):
                s = np.zeros(3, dtype=np.float32)
                for k in mem[ptr[q]:ptr[q + 1]]:
                    s = s + rpos[k]
                x[q, :3] = s / np.float32(max(int(ptr[q + 1] - ptr[q]), 1))
            out[tensor] = x
        else:
            raise AssertionError(f"unknown item kind {kind}")
    return out


def tensors_of(data, htree_mode: bool):
    """{tensor number: host array} of a HeteroData of the existing path (only the tensors it holds)"""
    out = {}
    for t, (key, attr) in enumerate(dsg._FRAME_TENSORS):
        if (t >= _lib.FT_HTREE) != htree_mode:
            continue
        store = data[key]
        if attr in store:
            out[t] = getattr(store, attr).cpu().numpy()
    return out


def clique_members(tree, which: int):
    """member rooms of every clique of node type 2 (object-room, init list 1) / 3 (room-room, init list 2), in init-edge order"""
    e = tree[("room_virtual", "rv_to_or", "object-room") if which == 2 else ("room_virtual", "rv_to_rr", "room-room")].edge_index.cpu().numpy()
    n = tree["object-room" if which == 2 else "room-room"].x.size(0)
    return [e[0][e[1] == q] for q in range(n)]

