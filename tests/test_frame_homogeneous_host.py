"""Host stage of the HOMOGENEOUS frame pipeline (csrc/frame.cpp ``hmp_frame_build_homogeneous``; include/hydra_mp.h section 14)
without a device.  The packed block is executed with numpy (tests/_frame_block.py), item by item -- one item per segment of a
tensor, what the one launch is specified to write -- and compared bit for bit with the committed host conversion run on the CPU:
``data.heterogeneous_data_to_homogeneous`` (+ ``room_mask``) of the existing frame, ``data.heterogeneous_htree_to_homogeneous`` of
its H-tree.  Also: the layout of the segments in the arena, the block of a NON-homogeneous frame (unchanged, pinned by hashes taken
before the homogeneous layout existed), the refusals, and the stand-alone sanitizer program."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

import _frame_block as fb
import _frame_cases as fc
from hydra_gnn_amd import _lib, dsg, htree
from hydra_gnn_amd.data import Data, heterogeneous_data_to_homogeneous, heterogeneous_htree_to_homogeneous

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = ["fixture", "special", (1, 1), (7, 2)]
# (name, htree, relative_pos, sem, clique_dim); clique_dim 16 with 6-wide leaves: the clique rows are the widest type
MODES = [("baseline", False, False, False, None), ("relative_pos", False, True, False, None), ("sem300", False, False, True, None),
         ("relative_pos_sem300", False, True, True, None), ("htree_c6", True, False, False, 6), ("htree_cNone", True, False, False, None),
         ("htree_c16", True, False, False, 16), ("htree_sem300_c6", True, False, True, 6), ("htree_sem300_cNone", True, False, True, None)]
MODE_IDS = [m[0] for m in MODES]
H0 = _lib.FT_HOMOG


def host(name, mode, homogeneous=True):
    _, ht, rel, sem, cd = mode
    tn, mn, mo = fc.THRESHOLDS
    return dsg.frame_host_stage(*fc.frame(name), threshold_near=tn, max_near=mn, max_on=mo, htree=ht, relative_pos=rel,
                                sem_dim=300 if sem else 0, n_labels=fc.N_LABELS if sem else 0, clique_dim=cd, homogeneous=homogeneous)


_ORACLE = {}


def oracle(name, mode):
    """the committed host conversion on the CPU: (Data, H-tree or None); computed once and left unchanged"""
    key = (name, mode[0])
    if key not in _ORACLE:
        _, ht, rel, sem, cd = mode
        frame, _ = fc.existing_frame(fc.frame(name), sem, relative_pos=rel)
        if ht:
            tree = htree.generate_htree(frame, clique_dim=cd)
            _ORACLE[key] = (heterogeneous_htree_to_homogeneous(tree), tree)
        else:
            d, types = heterogeneous_data_to_homogeneous(frame)
            d.room_mask = d.node_type == types.index("rooms")  # Hydra_mp3d_data.to_homogeneous
            _ORACLE[key] = (d, None)
    return _ORACLE[key]


def attributes(d: Data):
    return {k: v for k, v in vars(d).items() if k != "_plan_cache"}


# ---- the packed block, item by item ---------------------------------------------------------------------------------------------
def tensor_geometry(items):
    """{tensor: (base byte, rows, pitch)}: a tensor starts where its first item does, its segments' rows add up, and every segment
    of an edge tensor carries the pitch of the whole (S1)"""
    rows = fb.tensor_rows(items)  # asserts one pitch per tensor
    assert all(H0 <= t < H0 + _lib.FT_HOMOG_COUNT and dst % 16 == 0 for t, dst, _, _ in rows), rows
    return {t: (dst, n, pitch) for t, dst, n, pitch in rows}


def read_homogeneous(r, htree_mode, table):
    """{attribute: array} of a homogeneous frame: its block executed with numpy (``fb.expand``: every read inside the block, every
    write inside the arena, no byte twice) and viewed through its item table.  A homogeneous frame holds the five kinds of
    ``fb.HOMOG_KINDS``; every segment starts at a whole row (an edge segment: column) of its tensor and an edge segment lies inside
    the pitch; a CONST item reads no section and writes its tensor's element; and the segments of a tensor cover it exactly once,
    with nothing written outside the tensors."""
    items = r["items"]
    fb.check_kinds(items, fb.HOMOG_KINDS)
    geo = tensor_geometry(items)
    for kind, tensor, rows, width, dst, s0, s1, s2, s3, p0, p1, _ in items.tolist():
        at, attr = dst - geo[tensor][0], dsg._HOMOG_TENSORS[tensor - H0]
        if kind == _lib.FK_EDGE_SEG:
            assert rows == 2 and at % 8 == 0 and 0 <= at // 8 and at // 8 + width <= s1
        elif kind == _lib.FK_CONST:
            assert attr.endswith(("_type", "_mask")) and p1 == (1 if attr.endswith("_mask") else 8) and at % p1 == 0 and s0 == s1 == s2 == s3 == -1
        else:
            assert at >= 0 and at % (4 * width) == 0
    arena, written = fb.expand(r["block"], items, int(r["sizes"][_lib.FS_ARENA_BYTES]), table)
    tensors = fb.tensor_rows(items)
    got = fb.views(arena, tensors, htree_mode, True)
    assert np.array_equal(fb.covered(arena.size, tensors, htree_mode, True), written), "every element is written by exactly one segment"
    return {attr: a for (_, attr), a in got.items()}


def clique_rows(tree):
    """(first row, [member rooms of every clique]) of the object-room and room-room segments of the homogeneous x"""
    n = [tree[t].x.size(0) for t in ("object", "room", "object-room", "room-room")]
    return [(n[0] + n[1], fc.clique_members(tree, 2)), (n[0] + n[1] + n[2], fc.clique_members(tree, 3))]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", FRAMES, ids=str)
def test_packed_block_equals_the_host_conversion(name, mode):
    r = host(name, mode)
    got = read_homogeneous(r, mode[1], fc.semantic_table().numpy())
    d, tree = oracle(name, mode)
    want = {k: v.numpy() for k, v in attributes(d).items()}
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (k, got[k].dtype, got[k].shape, w.dtype, w.shape)
    x, wx = got.pop("x").copy(), want.pop("x").copy()
    if tree is not None:
        # the existing exception (test_frame_host.py): index_add_ has no defined order, so the mean of MORE than two member rooms is
        # not compared; the rest of such a row must be zero
        for first, members in clique_rows(tree):
            for q, m in enumerate(members):
                if len(m) > 2:
                    assert not x[first + q, 3:].any() and not wx[first + q, 3:].any()
                    x[first + q, :3] = wx[first + q, :3] = 0
    assert np.array_equal(x, wx)
    for k, w in want.items():
        assert np.array_equal(got[k], w), k


def test_known_answers_of_the_fixture():
    r = host("fixture", MODES[2])  # baseline, 300-column table
    got = read_homogeneous(r, False, fc.semantic_table().numpy())
    assert got["x"].shape == (67, 306) and got["edge_index"].shape == (2, 482)
    assert np.bincount(got["edge_type"]).tolist() == [356, 2, 62, 62]
    assert got["room_mask"].dtype == np.bool_ and got["room_mask"].sum() == 5 and got["room_mask"][-5:].all()
    assert not got["x"][62:, 6:].any()  # room rows: no semantic block
    assert len(r["items"]) == 14
    r = host("fixture", MODES[7])  # H-tree, clique_dim 6, 300-column table
    got = read_homogeneous(r, True, fc.semantic_table().numpy())
    assert got["x"].shape == (268, 306)
    assert got["edge_index"].shape == (2, 394) and got["init_edge_index"].shape == (2, 195) and got["pool_edge_index"].shape == (2, 166)
    assert got["room_mask"].sum() == 5 and got["object_mask"].sum() == 62
    assert sorted(set(got["edge_type"].tolist())) == [0, 1, 2, 3, 4, 5, 6, 7, 8]  # the fixture's rr_to_rr (type 9) is empty
    assert len(r["items"]) == 49  # 6 + 6 + 6 + 6 node segments, 10 + 10 + 3 + 2 edge segments: the worst case, of 64


def test_empty_segments_cost_nothing_and_shift_nothing():
    """the (1, 1) H-tree has no room-room clique and no edge of four types: their items stay in the table with no workgroup and no
    bytes, and the segments behind them start where they would without them"""
    r = host((1, 1), MODES[4])
    items = r["items"]
    empty = [it for it in items.tolist() if (it[_lib.FI_WIDTH] if it[_lib.FI_KIND] == _lib.FK_EDGE_SEG else it[_lib.FI_ROWS]) == 0]
    assert len(empty) >= 8  # room-room: x, node_type, two masks; the edge types that touch it, twice
    b0 = items[:, _lib.FI_BLOCK0].tolist() + [int(r["sizes"][_lib.FS_BLOCKS])]
    for i, it in enumerate(items.tolist()):
        n_el = it[_lib.FI_WIDTH] if it[_lib.FI_KIND] == _lib.FK_EDGE_SEG else it[_lib.FI_ROWS]
        assert (b0[i + 1] == b0[i]) == (n_el == 0), i
    counts = r["sizes"][_lib.FS_HT_COUNTS:_lib.FS_HT_COUNTS + 4].tolist()
    assert counts[3] == 0  # no room-room clique
    d, _ = oracle((1, 1), MODES[4])
    assert d.x.shape[0] == sum(counts) + 1 + 1 and int(d.room_mask.nonzero()[0]) == sum(counts) + 1


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", FRAMES + [(65, 1), (300, 3)], ids=str)
def test_layout(name, mode):
    """Every segment lies inside the arena; segments are disjoint; tensors start 16-byte aligned and a segment keeps the alignment
    its kind's stores need (8-byte lanes of an even feature row, int64, float32, bytes); the workgroup prefix is the one the
    kernel's mapping expects; the table fits the launch's 64-item lookup."""
    r = host(name, mode)
    items, sz = r["items"], r["sizes"]
    assert 0 < len(items) <= 64 and len(items) == sz[_lib.FS_ITEMS]
    assert len(items) == (49 if mode[1] else 18 if mode[2] else 14)
    arena = int(sz[_lib.FS_ARENA_BYTES])
    geo = tensor_geometry(items)  # asserts the 16-byte alignment of every tensor
    spans, block0 = [], 0
    for kind, tensor, rows, width, dst, s0, s1, s2, s3, p0, p1, b0 in items.tolist():
        assert b0 == block0
        if kind == _lib.FK_EDGE_SEG:
            assert dst % 8 == 0 and s1 >= width and s2 >= 0 and s3 >= 0
            spans += [(dst, dst + 8 * width), (dst + 8 * s1, dst + 8 * (s1 + width))]
            block0 += -(-2 * width // 256)
        elif kind == _lib.FK_CONST:
            assert dst % p1 == 0
            spans.append((dst, dst + rows * p1))
            block0 += -(-rows // 256)
        elif kind == _lib.FK_FEAT:
            head = p0 + 3
            lanes8 = width >= 32 and (width | head | p1) % 2 == 0  # the kernel's condition for float2 stores
            assert dst % (8 if lanes8 else 4) == 0
            spans.append((dst, dst + rows * width * 4))
            block0 += -(-rows // 4) if width >= 32 else -(-rows * width // 256)
        elif kind in (_lib.FK_CLIQUE, _lib.FK_EATTR):
            assert dst % 4 == 0 and (kind == _lib.FK_CLIQUE or width == 3)
            spans.append((dst, dst + rows * width * 4))
            block0 += -(-rows * width // 256)
        else:
            raise AssertionError(kind)
    assert block0 == sz[_lib.FS_BLOCKS]
    spans = sorted(s for s in spans if s[1] > s[0])
    assert spans[0][0] >= 0 and spans[-1][1] <= arena
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    # a byte tensor does not break the alignment of what follows it: every tensor base is a multiple of 16 (tensor_geometry) and
    # the tensors themselves are disjoint
    ext = sorted((base, base + (2 * pitch * 8 if dsg._HOMOG_TENSORS[t - H0].endswith("edge_index") else
                                rows * (8 if dsg._HOMOG_TENSORS[t - H0].endswith("_type") else
                                        1 if dsg._HOMOG_TENSORS[t - H0].endswith("_mask") else 4 * pitch)))
                 for t, (base, rows, pitch) in geo.items())
    assert all(a[1] <= b[0] for a, b in zip(ext, ext[1:])) and ext[-1][1] <= arena


# ---- non-homogeneous frames are what they were ---------------------------------------------------------------------------------
OLD_MODES = ["baseline", "relative_pos", "sem300", "htree", "htree_sem300"]  # test_frame_host.py
# sha256 of the fixture's packed block and (staging bytes, arena bytes, items, workgroups), taken from hmp_frame_build of the commit
# before hmp_frame_build_homogeneous existed
PINNED = {
    "baseline": ("39962c2c7a8af99bb9f70db6532f02153070a609c855541248d6fd7a24e669be", (6328, 11232, 12, 15)),
    "relative_pos": ("3c4e8ef1b076abef99c3ea084d838c799ce4242e8bafc635567f917002149c98", (6520, 16240, 16, 22)),
    "sem300": ("f5bf09f288985f1e838643cdd69a9499139a0d3f247296c4e63ef6b26c5d4362", (6328, 85632, 12, 29)),
    "htree": ("e2d8486e3808226739acdce86b15263d247521bc666c43c416595f380320f7a7", (10672, 23264, 29, 37)),
    "htree_sem300": ("5a7ec5ad71dba0f4e64872d8749356b0d2274af3cbe3b2adea06cc89ad9fe7f7", (10672, 254864, 29, 80)),
}


def old_mode_kw(mode):
    sem, ht = mode.endswith("sem300"), mode.startswith("htree")
    return dict(htree=ht, relative_pos=mode == "relative_pos", sem_dim=300 if sem else 0, n_labels=fc.N_LABELS if sem else 0,
                clique_dim=6 if ht else None)


def direct_build(name, kw):
    """(sizes, block) through hmp_frame_build itself, the entry that did not change, without dsg.frame_host_stage"""
    lib = _lib.load()
    arrays, n, m = dsg._frame_args(*fc.frame(name))
    ids, layer, pos, bb_min, bb_max, label, edges = arrays
    h = C.c_void_p()
    _lib.check(lib.hmp_frame_build(n, ids.ctypes.data, layer.ctypes.data, pos.ctypes.data, bb_min.ctypes.data, bb_max.ctypes.data,
                                   label.ctypes.data, m, edges.ctypes.data, *fc.THRESHOLDS, int(kw["htree"]), int(kw["relative_pos"]),
                                   kw["sem_dim"], kw["n_labels"], kw["clique_dim"] or 0, C.byref(h)))
    try:
        sz = np.zeros(_lib.FS_COUNT, dtype=np.int64)
        _lib.check(lib.hmp_frame_sizes(h, sz.ctypes.data))
        block = np.zeros(int(sz[_lib.FS_STAGING_BYTES]), dtype=np.uint8)
        _lib.check(lib.hmp_frame_pack(h, block.ctypes.data, block.size))
    finally:
        lib.hmp_frame_destroy(h)
    return sz, block


@pytest.mark.parametrize("mode", OLD_MODES)
@pytest.mark.parametrize("name", ["fixture", "special"] + fc.SIZES, ids=str)
def test_non_homogeneous_frames_are_unchanged(name, mode):
    kw = old_mode_kw(mode)
    tn, mn, mo = fc.THRESHOLDS
    r = dsg.frame_host_stage(*fc.frame(name), threshold_near=tn, max_near=mn, max_on=mo, homogeneous=False, **kw)
    sz, block = direct_build(name, kw)
    assert np.array_equal(r["sizes"], sz) and np.array_equal(r["block"], block)
    kinds = set(r["items"][:, _lib.FI_KIND].tolist())
    assert kinds <= set(range(_lib.FK_CLIQUE + 1)) and r["items"][:, _lib.FI_TENSOR].max() < _lib.FT_COUNT  # none of the new numbers
    if name == "fixture":
        sha, sizes = PINNED[mode]
        assert hashlib.sha256(block.tobytes()).hexdigest() == sha
        assert tuple(int(sz[k]) for k in (_lib.FS_STAGING_BYTES, _lib.FS_ARENA_BYTES, _lib.FS_ITEMS, _lib.FS_BLOCKS)) == sizes


def test_the_old_numbers_keep_their_meaning():
    assert _lib.FRAME_ITEM_WORDS == 12 and (_lib.FT_HTREE, _lib.FT_COUNT) == (16, 45) and _lib.FT_HOMOG >= _lib.FT_COUNT
    assert (_lib.FK_FEAT, _lib.FK_POS, _lib.FK_I64, _lib.FK_EDGE, _lib.FK_EATTR, _lib.FK_CLIQUE) == tuple(range(6))
    assert min(_lib.FK_EDGE_SEG, _lib.FK_CONST) > _lib.FK_CLIQUE
    header = open(os.path.join(ROOT, "include", "hydra_mp.h")).read()
    for name, value in (("HMP_FRAME_ITEM_WORDS", 12), ("HMP_FT_HTREE", 16), ("HMP_FT_COUNT", 45), ("HMP_FT_HOMOG", _lib.FT_HOMOG),
                        ("HMP_FT_HOMOG_COUNT", _lib.FT_HOMOG_COUNT), ("HMP_FK_EDGE_SEG", _lib.FK_EDGE_SEG), ("HMP_FK_CONST", _lib.FK_CONST),
                        ("HMP_FRAME_MAX_ITEMS", 64), ("HMP_ABI_VERSION", _lib.ABI_VERSION)):
        assert f"#define {name} {value}" in header.replace("  ", " "), name


# ---- refusals and frames with nothing to convert ---------------------------------------------------------------------------------
def test_relative_positions_on_an_htree_stay_refused():
    with pytest.raises(_lib.HydraMPError, match="relative"):
        dsg.frame_host_stage(*fc.frame((7, 2)), homogeneous=True, htree=True, relative_pos=True)
    with pytest.raises(_lib.HydraMPError, match="relative"):
        dsg.FramePipeline("cuda:0", homogeneous=True, htree=True, relative_pos=True)


@pytest.mark.parametrize("htree_mode", [False, True])
def test_empty_frames_return_none_without_touching_the_device(htree_mode):
    ids, layer, pos, bb_min, bb_max, label, edges = fc.frame((7, 2))
    pipe = dsg.FramePipeline("cuda:0", homogeneous=True, htree=htree_mode, clique_dim=6 if htree_mode else None)
    no_room, no_object = layer != dsg.ROOMS, layer != dsg.OBJECTS
    assert pipe.convert(*[a[no_room] for a in (ids, layer, pos, bb_min, bb_max, label)], edges) is None
    assert pipe.convert(*[a[no_object] for a in (ids, layer, pos, bb_min, bb_max, label)], edges) is None
    assert pipe.convert(ids, layer, pos, bb_min, bb_max, label, edges[:, :0]) is None  # no edges: every object is dropped
    r = dsg.frame_host_stage(ids, layer, pos, bb_min, bb_max, label, edges[:, :0], homogeneous=True, htree=htree_mode)
    assert r["empty"] and r["block"].size == 0 and r["sizes"][_lib.FS_ARENA_BYTES] == 0
    assert pipe._arena is None and pipe._d_staging is None


# ---- the stand-alone sanitizer program -------------------------------------------------------------------------------------------
def test_homogeneous_host_stage_is_clean_under_asan_and_ubsan(tmp_path):
    """`make frame_check`: frame.cpp + htree.cpp + a program with its own main under -fsanitize=address,undefined (CPU only, nothing
    preloaded), run with --homogeneous on the fixture frame and on the (300, 3) frame, baseline (with and without relative
    positions) and H-tree; a version-1 file written by dsg.save_frame_file in front of the flag still runs the existing layout"""
    files = []
    for name in ("fixture", (300, 3)):
        for kw in (dict(sem_dim=300, n_labels=fc.N_LABELS), dict(relative_pos=True, sem_dim=300, n_labels=fc.N_LABELS),
                   dict(htree=True, clique_dim=6), dict(htree=True, clique_dim=16)):
            path = str(tmp_path / f"frame_{len(files)}.bin")
            dsg.save_frame_file(path, *fc.frame(name), **kw)
            files.append(path)
    lines = fb.run_frame_check([files[0], "--homogeneous"] + files).splitlines()
    assert "(homogeneous)" not in lines[0] and "items 12 " in lines[0]  # in front of the flag: the existing layout
    assert sum("(homogeneous): kept 62 dropped 3 rooms 5 oo 178 rr 1" in ln for ln in lines) == 4
    assert sum("(homogeneous): kept 300 dropped 0 rooms 3" in ln for ln in lines) == 4
    assert sum("items 49 " in ln for ln in lines) == 4 and sum("items 14 " in ln for ln in lines) == 2 and sum("items 18 " in ln for ln in lines) == 2
