"""Shared cases of the tests of relative positions on H-tree edges (``FramePipeline(htree=True, htree_relative_pos=True)``;
tests/test_frame_htree_relpos_host.py, tests/test_gpu_frame_htree_relpos.py): the frames, the Python oracle
(``data.compute_relative_pos`` of ``htree.generate_htree(..., clique_pos=True)``), the tolerance rule, and a numpy execution of a
packed block with the item kind the mode adds (``HMP_FK_EATTR_HT``) -- what the one launch is specified to write, item by item."""
import numpy as np
import torch

import _frame_batch_cases as bc
import _frame_cases as fc
from hydra_gnn_amd import _lib, data as hdata, dsg, htree, workloads

CLIQUE_DIM = 6
EDGE_KEYS = [k for k, a in dsg._FRAME_TENSORS[_lib.FT_HTREE:] if a == "edge_index"]  # 10 tree, 3 init, o_to_ov, r_to_rv
POOL_KEYS = EDGE_KEYS[13:]
CLIQUE_TYPES = {"object-room": 2, "room-room": 3}
_CACHE = {}


def frame(name):
    """``fc.frame`` plus "triangle": four rooms 0-1-2-3 in a chain with the chords 0-2 and 1-3, so that the room-room cliques
    {0, 1, 2} and {1, 2, 3} have three members each (and an rr_to_rr edge joins them)"""
    if name != "triangle":
        return bc.frame(name)
    if name not in _CACHE:
        ids, layer, pos, bb_min, bb_max, label, edges = workloads.synthetic_scene(9, 4, seed=23)
        sym = lambda c, i: (ord(c) << 56) + i
        more = np.array([[sym("R", 0), sym("R", 1)], [sym("R", 2), sym("R", 3)]], dtype=np.uint64)
        _CACHE[name] = (ids, layer, pos, bb_min, bb_max, label, np.concatenate([np.asarray(edges, dtype=np.uint64), more], axis=1))
    return _CACHE[name]


# one room (no room-room clique, zero-row tensors): (1, 1), (65, 1); a clique of three rooms: "triangle"; tree edge types without an
# edge: every case but "triangle" has some
CASES = ["fixture", "special", "triangle"] + fc.SIZES
SMALL_CASES = ["fixture", "special", "triangle", (1, 1), (7, 2), (65, 1)]


def host_kwargs(homogeneous, sem=False):
    tn, mn, mo = fc.THRESHOLDS
    return dict(threshold_near=tn, max_near=mn, max_on=mo, htree=True, htree_relative_pos=True, sem_dim=300 if sem else 0,
                n_labels=fc.N_LABELS if sem else 0, clique_dim=CLIQUE_DIM, homogeneous=homogeneous)


def pipeline_kwargs(homogeneous, sem=False):
    return dict(semantic_table=fc.semantic_table() if sem else None, htree=True, htree_relative_pos=True, clique_dim=CLIQUE_DIM,
                homogeneous=homogeneous)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def oracle_typed(arrays, sem=False, device="cpu"):
    """``compute_relative_pos(generate_htree(frame, CLIQUE_DIM, clique_pos=True))`` of the existing path; also returns the tree
    BEFORE the three columns were dropped (its clique members and room positions give the tolerance)"""
    g, _ = fc.existing_frame(arrays, sem, device=device)
    tree = htree.generate_htree(g, clique_dim=CLIQUE_DIM, clique_pos=True)
    members = {t: fc.clique_members(tree, k) for t, k in CLIQUE_TYPES.items()}
    rpos = tree["room_virtual"].pos.cpu().numpy()
    hdata.compute_relative_pos(tree)
    return tree, members, rpos


def clique_bound(members, rpos):
    """per clique: 0 for up to two member rooms (two float32 additions from zero and a division by 1 or 2 have one result in any
    order), else k * 2^-24 * max|coordinate| over its k members -- the bound DESIGN 6.9 states for clique means"""
    return np.array([0.0 if len(m) <= 2 else len(m) * 2.0 ** -24 * float(np.abs(rpos[m]).max()) for m in members], dtype=np.float64)


def assert_close_rows(got, want, bound, what):
    """rows with bound 0 bit for bit, the others within their bound"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    exact = bound == 0
    assert np.array_equal(got[exact], want[exact]), what
    if (~exact).any():
        assert (np.abs(got[~exact].astype(np.float64) - want[~exact]) <= bound[~exact, None]).all(), what


def edge_bound(key, ei, bounds):
    """per edge: the sum of the bounds of its clique ends"""
    b = np.zeros(ei.shape[1], dtype=np.float64)
    for row, t in ((0, key[0]), (1, key[2])):
        if t in bounds:
            b += bounds[t][ei[row]]
    return b


# ---- numpy execution of a block --------------------------------------------------------------------------------------------------
def _section(block, off, dtype, count):
    nbytes = count * np.dtype(dtype).itemsize
    assert off >= 0 and off % 16 == 0 and off + nbytes <= block.size, (off, count, block.size)
    return block[off:off + nbytes].view(dtype)


def _end_pos(block, desc, words, idx):
    """float32 [len(idx), 3]: the positions of nodes ``idx`` of one end of an EATTR_HT item (words = mode, pos, index / ptr, members:
    byte offsets relative to the descriptor at ``desc``); every read is checked to lie inside the block"""
    mode, r_pos, r_a, r_b = words
    if idx.size == 0:
        return np.zeros((0, 3), dtype=np.float32)
    assert r_pos != 0
    top = int(idx.max()) + 1
    if mode == _lib.FE_CLIQUE:
        assert r_a != 0 and r_b != 0
        ptr = _section(block, desc + r_a, np.int32, top + 1)
        assert (np.diff(ptr) >= 0).all() and ptr[0] >= 0
        mem = _section(block, desc + r_b, np.int32, int(ptr[-1]))
        rpos = _section(block, desc + r_pos, np.float64, 3 * (int(mem.max()) + 1 if mem.size else 0)).reshape(-1, 3).astype(np.float32)
        mean = np.zeros((top, 3), dtype=np.float32)
        for q in np.unique(idx).tolist():
            s = np.zeros(3, dtype=np.float32)
            for k in mem[ptr[q]:ptr[q + 1]]:  # ascending member order, float32
                s = s + rpos[k]
            mean[q] = s / np.float32(max(int(ptr[q + 1] - ptr[q]), 1))
        return mean[idx]
    if mode == _lib.FE_GATHER:
        assert r_a != 0
        idx = _section(block, desc + r_a, np.int32, top)[idx]
        assert idx.min() >= 0
    else:
        assert mode == _lib.FE_DIRECT
    return _section(block, desc + r_pos, np.float64, 3 * (int(idx.max()) + 1)).reshape(-1, 3)[idx].astype(np.float32)


def eattr_ht(block, item):
    kind, tensor, rows, width, dst, s0, s1, s2, s3, p0, p1, _ = item
    assert kind == _lib.FK_EATTR_HT and width == 3 and rows == p1 and s2 == -1 and s3 == -1
    if p0 == 0:  # as given
        e = _section(block, s0, np.int32, 2 * p1)
        src, dst_ = e[:p1].astype(np.int64), e[p1:].astype(np.int64)
    else:  # (k, v[k])
        assert p0 == 4
        src, dst_ = np.arange(p1, dtype=np.int64), _section(block, s0, np.int32, p1).astype(np.int64)
    assert (src >= 0).all() and (dst_ >= 0).all()
    d = _section(block, s1, np.int32, 2 * _lib.FRAME_END_WORDS).tolist()
    return _end_pos(block, s1, d[_lib.FRAME_END_WORDS:], dst_) - _end_pos(block, s1, d[:_lib.FRAME_END_WORDS], src)


def expand(block, items, arena_bytes, table=None):
    """The arena (uint8) a launch over this block is specified to write, and the mask of written bytes.  Every section read is
    checked to lie inside the block and to be 16-byte aligned, every write to lie inside the arena at a multiple of its element
    size, and no byte is written twice."""
    arena = np.zeros(arena_bytes, dtype=np.uint8)
    written = np.zeros(arena_bytes, dtype=bool)

    def put(dst, values):
        raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
        assert dst >= 0 and dst % values.dtype.itemsize == 0 and dst + raw.size <= arena_bytes, (dst, raw.size, arena_bytes)
        assert not written[dst:dst + raw.size].any()
        arena[dst:dst + raw.size] = raw
        written[dst:dst + raw.size] = True

    for item in items.tolist():
        kind, tensor, rows, width, dst, s0, s1, s2, s3, p0, p1, _ = item
        one = lambda it: fc.read_block(block, np.array([it], dtype=np.int64), table)[tensor]
        if kind == _lib.FK_EATTR_HT:
            put(dst, eattr_ht(block, item))
        elif kind == _lib.FK_CLIQUE:  # [mean | zeros] without its first p0 columns
            assert p0 in (0, 3)
            put(dst, one([kind, tensor, rows, width + p0, 0, s0, s1, s2, s3, 0, 0, 0])[:, p0:])
        elif kind == _lib.FK_CONST:
            assert p1 in (1, 8)
            put(dst, np.full(rows, p0, dtype=np.int64 if p1 == 8 else np.uint8))
        elif kind in (_lib.FK_EDGE, _lib.FK_EDGE_SEG):
            ends = one([_lib.FK_EDGE, tensor, 2, width, 0, s0, -1, -1, -1, p0, p1, 0])
            pitch, shift = (s1, (s2, s3)) if kind == _lib.FK_EDGE_SEG else (width, (0, 0))
            assert 0 <= width <= pitch
            put(dst, ends[0] + shift[0])
            put(dst + 8 * pitch, ends[1] + shift[1])
        elif kind == _lib.FK_FEAT:
            own = p0 + 3 + p1
            x = np.zeros((rows, width), dtype=np.float32)
            x[:, :own] = one([kind, tensor, rows, own, 0, s0, s1, s2, s3, p0, p1, 0])
            put(dst, x)
        else:
            assert kind in (_lib.FK_POS, _lib.FK_I64), kind  # the mode has no plain EATTR item
            put(dst, one(item))
    return arena, written


def check_prefix(items, n_blocks):
    """the workgroup prefix words are the running sum of the items' workgroups"""
    blocks = np.array([-(-it[_lib.FI_ROWS] * 3 // 256) if it[_lib.FI_KIND] == _lib.FK_EATTR_HT else bc.item_blocks(it) for it in items.tolist()])
    assert np.array_equal(items[:, _lib.FI_BLOCK0], np.concatenate([[0], np.cumsum(blocks)[:-1]])) and blocks.sum() == n_blocks
    return blocks


def typed_views(arena, items):
    """{(store key, attribute): array} of a typed single frame"""
    out = {}
    for kind, tensor, rows, width, dst, *_ in items.tolist():
        assert dst % 16 == 0
        if kind == _lib.FK_I64:
            a = arena[dst:dst + 8 * rows].view(np.int64)
        elif kind == _lib.FK_EDGE:
            a = arena[dst:dst + 16 * width].view(np.int64).reshape(2, width)
        else:
            a = arena[dst:dst + 4 * rows * width].view(np.float32).reshape(rows, width)
        out[dsg._typed_tensor(tensor)] = a
    return out


def homogeneous_views(arena, items):
    """{attribute: array} of a homogeneous single frame (the rule of ``FramePipeline._homogeneous_data``)"""
    at, n_rows, pitch = {}, {}, {}
    for kind, tensor, rows, width, dst, _, s1, *_ in items.tolist():
        if tensor not in at:
            assert dst % 16 == 0
            at[tensor], n_rows[tensor], pitch[tensor] = dst, 0, s1 if kind == _lib.FK_EDGE_SEG else width
        n_rows[tensor] += rows
    out = {}
    for tensor, dst in at.items():
        attr, n, w = dsg._HOMOG_TENSORS[tensor - _lib.FT_HOMOG], n_rows[tensor], pitch[tensor]
        if attr.endswith("edge_index"):
            out[attr] = arena[dst:dst + 16 * w].view(np.int64).reshape(2, w)
        elif attr.endswith("_type"):
            out[attr] = arena[dst:dst + 8 * n].view(np.int64)
        elif attr.endswith("_mask"):
            out[attr] = arena[dst:dst + n].view(np.bool_)
        else:
            out[attr] = arena[dst:dst + 4 * n * w].view(np.float32).reshape(n, w)
    return out


def batch_name(t, homogeneous):
    """(store key or None, attribute) of batched tensor ``t`` in this mode"""
    FB = _lib.FT_BATCH
    if t >= _lib.FT_HTREL or t < _lib.FT_HOMOG:
        return dsg._typed_tensor(t)
    if t < FB:
        return None, dsg._HOMOG_TENSORS[t - _lib.FT_HOMOG]
    k = t - FB
    nodes, edges = dsg._node_type_names(True, homogeneous), dsg._edge_type_names(True, homogeneous)
    if k >= _lib.FTB_Y:
        return (None if homogeneous else nodes[k - _lib.FTB_Y]), "y"
    if k >= _lib.FTB_EDGE_PTR:
        return edges[k - _lib.FTB_EDGE_PTR], "ptr"
    if k >= _lib.FTB_NODE_PTR:
        return nodes[k - _lib.FTB_NODE_PTR], "ptr"
    return nodes[k], "batch"


def batch_views(arena, tensors, homogeneous):
    """{(store key or None, attribute): array} of the batched tensors, through the batch's tensor table"""
    out = {}
    for t, dst, rows, width in tensors.tolist():
        assert dst % 16 == 0
        key, attr = batch_name(t, homogeneous)
        if attr.endswith("edge_index"):
            a = arena[dst:dst + 16 * width].view(np.int64).reshape(2, width)
        elif attr.endswith("_mask"):
            a = arena[dst:dst + rows].view(np.bool_)
        elif attr in ("x", "pos", "edge_attr"):
            a = arena[dst:dst + 4 * rows * width].view(np.float32).reshape(rows, width)
        else:
            a = arena[dst:dst + 8 * rows].view(np.int64)
        assert (key, attr) not in out
        out[(key, attr)] = a
    return out


def typed_graph(views):
    """a ``HeteroData`` from {(key, attr): numpy array} (copies), stores in the pipeline's order"""
    g = hdata.HeteroData()
    for t in dsg._HTREE_STORES:
        g[t]
    for (key, attr), a in views.items():
        setattr(g[key], attr, torch.from_numpy(np.array(a)))
    return g


def store_arrays(graphs, homogeneous):
    """{(key or None, attr): array} of what ``GraphStore.__init__`` cats from a list of graphs (an HMP_FB_STORE block): rows back to
    back, graph-LOCAL edge lists side by side, the [G + 1] offset vectors; no ``batch``"""
    cum = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    g0, out = graphs[0], {}
    if homogeneous:
        for attr, v in vars(g0).items():
            if isinstance(v, torch.Tensor):
                out[(None, attr)] = torch.cat([getattr(g, attr) for g in graphs], dim=1 if "index" in attr else 0).numpy()
        out[("node", "ptr")] = cum([g.num_nodes for g in graphs])
        for k in ("edge_index", "init_edge_index", "pool_edge_index"):
            out[(k, "ptr")] = cum([getattr(g, k).size(1) for g in graphs])
        return out
    for key in g0.node_types + g0.edge_types:
        for attr, v in g0[key].items():
            if isinstance(v, torch.Tensor):
                out[(key, attr)] = torch.cat([getattr(g[key], attr) for g in graphs], dim=1 if attr == "edge_index" else 0).numpy()
        out[(key, "ptr")] = cum([g[key].edge_index.size(1) if isinstance(key, tuple) else g[key].num_nodes for g in graphs])
    return out


def collated_arrays(batch, homogeneous):
    """{(key or None, attr): array} of a ``data.collate`` / ``data.collate_homogeneous`` result (an HMP_FB_COLLATED block)"""
    if homogeneous:
        return {(None, k): v.numpy() for k, v in vars(batch).items() if isinstance(v, torch.Tensor)}
    return {(key, attr): v.numpy() for key in batch.node_types + batch.edge_types for attr, v in batch[key].items() if isinstance(v, torch.Tensor)}
