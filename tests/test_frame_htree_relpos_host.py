"""Relative positions on H-tree edges, host stage (csrc/frame.cpp with ``relative_pos = HMP_FRAME_RELPOS_HTREE``; include/hydra_mp.h
section 14) without a device.  The packed block is executed with numpy, item by item -- what the one launch is specified to write,
``HMP_FK_EATTR_HT`` included -- and compared with the Python oracle on the CPU (``data.compute_relative_pos`` of
``htree.generate_htree(..., clique_pos=True)``, and ``data.heterogeneous_htree_to_homogeneous`` of that), for single frames and for
both forms of a batch.  Also: the refusals, the oracle's own contract, the blocks of every earlier mode (pinned by hashes taken
from the commit before this mode existed), and the stand-alone sanitizer program."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

import _frame_batch_cases as bc
import _frame_block as fb
import _frame_cases as fc
import _frame_htree_relpos_cases as hc
from hydra_gnn_amd import _lib, data as hdata, dsg, htree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SINGLE = {}


def single(name, homogeneous, sem=False):
    """host stage of one frame + the numpy execution of its block: (host result, {name: array}); computed once per case"""
    key = (str(name), homogeneous, sem)
    if key not in _SINGLE:
        r = dsg.frame_host_stage(*hc.frame(name), **hc.host_kwargs(homogeneous, sem))
        fb.check_kinds(r["items"], fb.HTREL_KINDS)  # the mode has no plain EATTR item
        arena, written = fb.expand(r["block"], r["items"], int(r["sizes"][_lib.FS_ARENA_BYTES]), fc.semantic_table().numpy())
        r["written"] = written
        views = fb.views(arena, fb.tensor_rows(r["items"]), True, homogeneous)
        _SINGLE[key] = (r, {attr: a for (_, attr), a in views.items()} if homogeneous else views)
    return _SINGLE[key]


_ORACLE = {}


def oracle(name, sem=False):
    key = (str(name), sem)
    if key not in _ORACLE:
        _ORACLE[key] = hc.oracle_typed(hc.frame(name), sem)
    return _ORACLE[key]


# ---- the oracle's own contract ---------------------------------------------------------------------------------------------------
def test_generate_htree_keeps_its_keys_and_adds_clique_pos_only_on_request():
    g, _ = fc.existing_frame(hc.frame("triangle"), False)
    plain, default, with_pos = htree.generate_htree(g, 6), htree.generate_htree(g, 6, clique_pos=False), htree.generate_htree(g, 6, clique_pos=True)
    want = {"object": ["x", "pos", "label"], "room": ["x", "pos", "label"], "object-room": ["x"], "room-room": ["x"],
            "object_virtual": ["x", "pos", "label"], "room_virtual": ["x", "pos", "label"]}
    for t in (plain, default):
        assert t.node_types == list(want) and t.edge_types == [tuple(e) for e in hc.EDGE_KEYS]
        assert {k: list(t[k].keys()) for k in t.node_types} == want
        assert all(list(t[e].keys()) == ["edge_index"] for e in t.edge_types)
    for k in plain.node_types + plain.edge_types:
        for a, v in plain[k].items():
            assert torch.equal(getattr(with_pos[k], a), v) and torch.equal(getattr(default[k], a), v)
    for k in ("object-room", "room-room"):
        assert sorted(with_pos[k].keys()) == ["pos", "x"] and with_pos[k].x.size(0) > 0
        assert torch.equal(with_pos[k].pos, with_pos[k].x[:, :3])
    with pytest.raises(AttributeError):  # without the clique positions compute_relative_pos cannot run: why the keyword exists
        hdata.compute_relative_pos(plain)
    hdata.compute_relative_pos(with_pos)
    assert len(with_pos.edge_attr_dict) == 15 and with_pos["room-room"].x.shape[1] == 3


def test_the_cases_hold_the_shapes_the_kernel_can_go_wrong_at():
    sizes = {str(n): single(n, False)[0]["sizes"] for n in hc.CASES}
    counts = {n: s[_lib.FS_HT_COUNTS:_lib.FS_HT_COUNTS + 4].tolist() for n, s in sizes.items()}
    edges = {n: s[_lib.FS_HT_EDGES:_lib.FS_HT_EDGES + 10].tolist() for n, s in sizes.items()}
    assert counts["(1, 1)"][3] == 0 and counts["(65, 1)"][3] == 0  # one room: no room-room clique, zero-row tensors
    assert all(0 in e for n, e in edges.items() if n != "(300, 3)") and 0 not in edges["(300, 3)"]  # tree edge types without an edge
    assert max(len(m) for m in oracle("triangle")[1]["room-room"]) >= 3  # a clique of three rooms
    assert max(int(s[_lib.FS_BLOCKS]) for s in sizes.values()) > 64  # more workgroups than one wavefront's prefix lanes


# ---- single frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.CASES, ids=str)
def test_typed_block_equals_the_oracle(name):
    check_typed_block(name, False)


@pytest.mark.parametrize("name", ["fixture", "triangle"])
def test_typed_block_with_a_semantic_table_equals_the_oracle(name):
    check_typed_block(name, True)


def check_typed_block(name, sem):
    r, got = single(name, False, sem)
    items, sz = r["items"], r["sizes"]
    assert len(items) == 46 == sz[_lib.FS_ITEMS] and set(items[:, _lib.FI_KIND].tolist()) == {_lib.FK_FEAT, _lib.FK_POS, _lib.FK_I64, _lib.FK_EDGE, _lib.FK_CLIQUE, _lib.FK_EATTR_HT}
    assert (items[:, _lib.FI_DST] % 16 == 0).all()
    fb.check_prefix(items, int(sz[_lib.FS_BLOCKS]))
    tree, members, rpos = oracle(name, sem)
    bounds = {t: hc.clique_bound(members[t], rpos) for t in hc.CLIQUE_TYPES}
    want = {(k, a): v.numpy() for k in tree.node_types + tree.edge_types for a, v in tree[k].items()}
    assert sorted(map(str, got)) == sorted(map(str, want))
    for (key, attr), w in want.items():
        g = got[(key, attr)]
        if attr == "edge_attr":
            hc.assert_close_rows(g, w, hc.edge_bound(key, want[(key, "edge_index")], bounds), (key, attr))
        elif attr == "pos" and key in bounds:
            hc.assert_close_rows(g, w, bounds[key], (key, attr))
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (key, attr)
    for t in hc.CLIQUE_TYPES:  # CLIQUE_DIM - 3 zeros per row
        assert got[(t, "x")].shape[1] == hc.CLIQUE_DIM - 3 and not got[(t, "x")].any()
    assert got[("object", "x")].shape[1] == (303 if sem else 3) and got[("room", "x")].shape[1] == 3
    # against the block's own pos tensors the edge attributes are exact everywhere, on all 15 edge types
    for key in hc.EDGE_KEYS:
        ei = got[(key, "edge_index")]
        assert np.array_equal(got[(key, "edge_attr")], got[(key[2], "pos")][ei[1]] - got[(key[0], "pos")][ei[0]]), key
    for key in hc.POOL_KEYS:  # a leaf and the node it stands for: exact +0.0
        ea = got[(key, "edge_attr")]
        assert ea.shape[0] > 0 and not ea.any() and not np.signbit(ea).any()


@pytest.mark.parametrize("name", hc.CASES, ids=str)
def test_homogeneous_block_equals_the_oracle(name):
    r, got = single(name, True)
    items, sz = r["items"], r["sizes"]
    assert len(items) == 59 == sz[_lib.FS_ITEMS]
    fb.check_prefix(items, int(sz[_lib.FS_BLOCKS]))
    tree, members, rpos = hc.oracle_typed(hc.frame(name))  # heterogeneous_htree_to_homogeneous edits its argument: a fresh one
    bounds = {t: hc.clique_bound(members[t], rpos) for t in hc.CLIQUE_TYPES}
    eb = np.concatenate([hc.edge_bound(tuple(k), tree[tuple(k)].edge_index.numpy(), bounds) for k in hc.EDGE_KEYS[:10]])
    d = hdata.heterogeneous_htree_to_homogeneous(tree)
    want = {k: v.numpy() for k, v in vars(d).items() if isinstance(v, torch.Tensor)}
    assert sorted(got) == sorted(want) and "edge_attr" in want and want["edge_attr"].shape == (want["edge_index"].shape[1], 3)
    for k, w in want.items():
        if k == "edge_attr":
            hc.assert_close_rows(got[k], w, eb, k)
        else:
            assert got[k].dtype == w.dtype and got[k].shape == w.shape and np.array_equal(got[k], w), k
    # the same values as the typed block's, segment by segment, bit for bit
    typed = single(name, False)[1]
    assert np.array_equal(got["edge_attr"], np.concatenate([typed[(k, "edge_attr")] for k in hc.EDGE_KEYS[:10]]))
    # every written byte once (fb.expand), and the segments of a tensor tile it: no gap inside the tensors either
    x_bytes = got["x"].size * 4
    assert r["written"][:x_bytes].all()


# ---- batches ---------------------------------------------------------------------------------------------------------------------
BATCH_NAMES = bc.FRAME_NAMES + ["triangle"]  # 6 graphs and one skipped frame


def cpu_graphs(names, homogeneous, ys):
    """the per-frame CPU results (the numpy execution of each frame's own block, compared with the oracle above) as graphs with y"""
    graphs = []
    for name, y in zip(names, ys):
        r, views = single(name, False)
        if r["empty"]:
            continue
        g = bc.attach_labels(hc.typed_graph(views), y, r["kept"], r["rooms"], True)
        graphs.append(hdata.heterogeneous_htree_to_homogeneous(g) if homogeneous else g)
    return graphs


def batch_host(names, homogeneous, form, ys=None):
    return dsg.frame_batch_host_stage([hc.frame(n) for n in names], form=form, y=ys, **hc.host_kwargs(homogeneous))


@pytest.mark.parametrize("form", [_lib.FB_COLLATED, _lib.FB_STORE], ids=["collated", "store"])
@pytest.mark.parametrize("homogeneous", [False, True], ids=["typed", "homogeneous"])
def test_batch_block_equals_the_collation_of_the_single_frames(homogeneous, form):
    ys = [bc.labels(hc.frame(n), i) for i, n in enumerate(BATCH_NAMES)]
    r = batch_host(BATCH_NAMES, homogeneous, form, ys)
    sz, items, groups = r["sizes"], r["items"], r["groups"]
    n_items = int(sz[_lib.FBS_ITEMS])
    assert r["num_graphs"] == 6 and r["graph_of_frame"].tolist() == [0, 1, -1, 2, 3, 4, 5]
    assert groups.size == -(-n_items // 64) >= 3 and np.array_equal(groups, items[::64, _lib.FI_BLOCK0])  # several item groups
    blocks = fb.check_prefix(items, int(sz[_lib.FBS_BLOCKS]))
    if not homogeneous and form == _lib.FB_COLLATED:  # a group that ends in empty items, the next one starting with work
        assert any(blocks[64 * g - 1] == 0 and blocks[64 * g:].any() for g in range(1, groups.size)), blocks.tolist()
    for b in range(0, int(sz[_lib.FBS_BLOCKS]), 7):  # the two-level lookup lands on the item that owns the workgroup
        i = fb.lookup(groups, items, n_items, b)
        assert blocks[i] > 0 and items[i, _lib.FI_BLOCK0] <= b < items[i, _lib.FI_BLOCK0] + blocks[i]
    fb.check_kinds(items, fb.HTREL_KINDS)
    arena, written = fb.expand(r["block"], items, int(sz[_lib.FBS_ARENA_BYTES]))
    got = fb.views(arena, r["tensors"], True, homogeneous)
    graphs = cpu_graphs(BATCH_NAMES, homogeneous, ys)
    if form == _lib.FB_COLLATED:
        want = bc.collated_arrays(bc.collate(graphs, homogeneous), homogeneous)
    else:
        want = bc.store_arrays(graphs, homogeneous)
    assert sorted(map(str, got)) == sorted(map(str, want))
    for k, w in want.items():  # the per-frame results are the kernel's own arithmetic: exact everywhere
        assert got[k].dtype == w.dtype and got[k].shape == w.shape and np.array_equal(got[k], w), k
    assert any(a == "edge_attr" for _, a in want) and (homogeneous or sum(a == "edge_attr" for _, a in want) == 15)
    # what hmp_frame_batch_items_needed says is what was packed
    a, n, m = dsg._frame_args(*hc.frame("fixture"))
    h = dsg._frame_build(_lib.load(), a, n, m, fc.THRESHOLDS, True, _lib.FRAME_RELPOS_HTREE, 0, 0, hc.CLIQUE_DIM, homogeneous)
    try:
        per_frame, per_batch = C.c_int32(), C.c_int32()
        _lib.check(_lib.load().hmp_frame_batch_items_needed(h, form, 1, C.byref(per_frame), C.byref(per_batch)))
    finally:
        _lib.load().hmp_frame_destroy(h)
    assert n_items == 6 * per_frame.value + per_batch.value
    assert per_frame.value == (59 + 6 if homogeneous else 46 + 4 + (6 if form == _lib.FB_COLLATED else 0))


def test_more_items_than_the_tables_hold_are_refused():
    frames = [(1, 1)] * 74  # typed, collated, with y: 56 items a frame and 21 for the batch: 74 frames need 4165 > 4096
    ys = [bc.labels(hc.frame(n)) for n in frames]
    with pytest.raises(_lib.HydraMPError, match="4096"):
        batch_host(frames, False, _lib.FB_COLLATED, ys)
    r = batch_host(frames[:72], False, _lib.FB_COLLATED, ys[:72])
    assert int(r["sizes"][_lib.FBS_ITEMS]) == 72 * 56 + 21 <= 4096


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    arrays = hc.frame((7, 2))
    kw = dict(zip(("threshold_near", "max_near", "max_on"), fc.THRESHOLDS))
    for homogeneous in (False, True):
        with pytest.raises(_lib.HydraMPError, match="relative"):  # the baseline's mode on an H-tree stays refused
            dsg.frame_host_stage(*arrays, htree=True, relative_pos=True, homogeneous=homogeneous, **kw)
        with pytest.raises(_lib.HydraMPError, match="htree"):
            dsg.frame_host_stage(*arrays, htree_relative_pos=True, homogeneous=homogeneous, **kw)
        with pytest.raises(_lib.HydraMPError, match="relative_pos"):
            dsg.frame_host_stage(*arrays, htree=True, relative_pos=True, htree_relative_pos=True, homogeneous=homogeneous, **kw)
        for clique_dim in (1, 2, 3):
            with pytest.raises(_lib.HydraMPError, match="clique_dim"):
                dsg.frame_host_stage(*arrays, htree=True, htree_relative_pos=True, clique_dim=clique_dim, homogeneous=homogeneous, **kw)
        assert not dsg.frame_host_stage(*arrays, htree=True, htree_relative_pos=True, clique_dim=4, homogeneous=homogeneous, **kw)["empty"]
        assert not dsg.frame_host_stage(*arrays, htree=True, htree_relative_pos=True, homogeneous=homogeneous, **kw)["empty"]  # clique_dim 0
    with pytest.raises(_lib.HydraMPError, match="relative"):
        dsg.FramePipeline("cuda:0", htree=True, relative_pos=True)
    with pytest.raises(_lib.HydraMPError, match="htree"):
        dsg.FramePipeline("cuda:0", htree_relative_pos=True)
    with pytest.raises(_lib.HydraMPError, match="relative_pos"):
        dsg.FramePipeline("cuda:0", htree=True, relative_pos=True, htree_relative_pos=True)
    with pytest.raises(_lib.HydraMPError, match="clique_dim"):
        dsg.FramePipeline("cuda:0", htree=True, htree_relative_pos=True, clique_dim=3)
    with pytest.raises(_lib.HydraMPError, match="htree"):
        dsg.frame_batch_host_stage([arrays], htree_relative_pos=True)
    # the C entry itself: the mode value without htree
    lib = _lib.load()
    a, n, m = dsg._frame_args(*arrays)
    with pytest.raises(_lib.HydraMPError, match="htree"):
        dsg._frame_build(lib, a, n, m, fc.THRESHOLDS, False, _lib.FRAME_RELPOS_HTREE, 0, 0, 0)


def test_a_batch_that_mixes_modes_is_refused():
    lib = _lib.load()
    a, n, m = dsg._frame_args(*hc.frame((7, 2)))
    plain = dsg._frame_build(lib, a, n, m, fc.THRESHOLDS, True, 0, 0, 0, hc.CLIQUE_DIM)
    rel = dsg._frame_build(lib, a, n, m, fc.THRESHOLDS, True, _lib.FRAME_RELPOS_HTREE, 0, 0, hc.CLIQUE_DIM)
    try:
        for pair in ([plain, rel], [rel, plain]):
            with pytest.raises(_lib.HydraMPError, match="different configurations"):
                dsg._batch_build(lib, pair, _lib.FB_COLLATED, None)
    finally:
        lib.hmp_frame_destroy(plain)
        lib.hmp_frame_destroy(rel)


def test_a_frame_without_a_room_or_a_kept_object_returns_none_without_a_device():
    ids, layer, pos, bb_min, bb_max, label, edges = hc.frame((7, 2))
    for homogeneous in (False, True):
        pipe = dsg.FramePipeline("cuda:0", **hc.pipeline_kwargs(homogeneous))
        assert pipe.convert(*hc.frame("no_room")) is None
        assert pipe.convert(ids, layer, pos, bb_min, bb_max, label, edges[:, :0]) is None
        assert pipe.convert_batch([hc.frame("no_room")])[0] is None
        assert pipe._arena is None and pipe._d_staging is None


# ---- every earlier mode packs what it packed -------------------------------------------------------------------------------------
# sha256 of a packed block and (staging bytes, arena bytes, items, workgroups), taken from the host stage of the commit before
# HMP_FRAME_RELPOS_HTREE existed: the fixture frame alone, and the batch [fixture, (7, 2)] with bc.labels in both forms
PINNED = {
    'typed_baseline': ('39962c2c7a8af99bb9f70db6532f02153070a609c855541248d6fd7a24e669be', (6328, 11232, 12, 15)),
    'typed_baseline_collated': ('7b39be6e12cbab2b07a58c8523d2809820c7beea560d17dc117818f08c38141d', (12856, 13456, 38, 41)),
    'typed_baseline_store': ('762b11b65dc12f8fb3a2137d157e2be222d04fae5125d60c6907ee4e5887ff0a', (12664, 12832, 34, 37)),
    'typed_relative_pos': ('3c4e8ef1b076abef99c3ea084d838c799ce4242e8bafc635567f917002149c98', (6520, 16240, 16, 22)),
    'typed_relative_pos_collated': ('cca3e4be3444447c3a17cc9b792e8610f19033a36f19e845e56ba3d1a12768e4', (13240, 18560, 46, 52)),
    'typed_relative_pos_store': ('aacc0e24e2033f5b08eaf7177cca80a79c75611a639dd14bc9c1ccab0c4c6ecc', (13048, 17936, 42, 48)),
    'typed_sem300': ('f5bf09f288985f1e838643cdd69a9499139a0d3f247296c4e63ef6b26c5d4362', (6328, 85632, 12, 29)),
    'typed_sem300_collated': ('0663772a58feb11358d7e14ea82130b0412aeee1da0e3056b1991ac1e018fa7a', (12856, 96256, 38, 56)),
    'typed_sem300_store': ('95d9a8d97b5f15a0daffc3a99a089137dd5023ed9b4aa8e7cbeb3d6b2ef12d68', (12664, 95632, 34, 52)),
    'typed_htree': ('e2d8486e3808226739acdce86b15263d247521bc666c43c416595f380320f7a7', (10672, 23264, 29, 37)),
    'typed_htree_collated': ('6ce593f569dc68b88476bbc131895c9348910e85b7441e5bfec09b0c660b7218', (21016, 30800, 99, 105)),
    'typed_htree_store': ('f1296020b807136aba40873d8c5ca6f830109734beabdfc0dc2cf381f51a1e06', (20440, 28384, 87, 93)),
    'typed_htree_sem300': ('5a7ec5ad71dba0f4e64872d8749356b0d2274af3cbe3b2adea06cc89ad9fe7f7', (10672, 254864, 29, 80)),
    'typed_htree_sem300_collated': ('e68156a75e70966bf587f824f74ac28f9c08ebb15844065dd4b01cbc5fa9969c', (21016, 279200, 99, 150)),
    'typed_htree_sem300_store': ('de5aefaa21c4f3a68a909930c3270018cf1a67c6249cb5cac291bbe21e36a9a7', (20440, 276784, 87, 138)),
    'homog_baseline': ('7ebc35c9a291345d73f56cd28331140d76dd67c498fe9d72651287e0f27aae3b', (5880, 13808, 14, 18)),
    'homog_baseline_collated': ('d148c72e21a6782e024c445a5f1b3e4a5642bc160c21337dd476352430d9d3a1', (11752, 15120, 32, 36)),
    'homog_baseline_store': ('98e2ba999cf7726b03e66757470a6eb5f774ece6eebeb7bdb6b4e019655f112c', (11912, 15184, 34, 38)),
    'homog_relative_pos': ('1043b7a573d955fb130ac0012369310221c20c8b43eaac3ec2d8c6fa55efd145', (6072, 18800, 18, 25)),
    'homog_relative_pos_collated': ('342acd06a31908f30e93f9b9911b03de3a3c692bd75a1b35a342c9093aefab56', (12136, 20208, 40, 47)),
    'homog_relative_pos_store': ('e0aac10bc1adac34c8c8b2f5cbb54b84177e8d9895184217de1fbf2bd17ec54b', (12296, 20272, 42, 49)),
    'homog_sem300': ('0aea1b7d7203fa44884d6d3007b3e75db599f9ed4f7cd982633f0a858cd4c274', (5880, 94208, 14, 33)),
    'homog_sem300_collated': ('ca2f043a58f3ed4906f991d0897c5ac2499f4902b3d3ca9695a8ca6d137db92d', (11752, 106320, 32, 52)),
    'homog_sem300_store': ('aa920a73fdb0185a854c4bbaad71658c4ec091454a34869df19a23f1b3f65304', (11912, 106384, 34, 54)),
    'homog_htree': ('764192f97210489d15ac4aa5b23d878b555928caa0eaed39c15f3dc3dd231751', (11624, 24352, 49, 55)),
    'homog_htree_collated': ('6e83cc6ac650001425c9e738fed730c4fa1cc375207179d97a86e15994d8512f', (20872, 29312, 110, 112)),
    'homog_htree_store': ('3f69c8a1b4a8f3e6326caea711b1cd194f6601aeac6745589d92ba7a0fa0adef', (21192, 29440, 114, 116)),
    'homog_htree_sem300': ('45b800e07ca127bee84a2a0d49533a3d851d61dc1f832d9449a0899a7ce3cb68', (11624, 345952, 49, 148)),
    'homog_htree_sem300_collated': ('16fc48f652015756071d055351d200e14ab14ecb47b77d0a35f8c9de0462f837', (20872, 388112, 110, 216)),
    'homog_htree_sem300_store': ('be366d0c61864c4ffd8011fe4c824cd850a55f5f954b1eed0360f5a7ce4f0afb', (21192, 388240, 114, 220)),
}
OLD_MODES = {"baseline": (False, False, False), "relative_pos": (False, True, False), "sem300": (False, False, True),
             "htree": (True, False, False), "htree_sem300": (True, False, True)}  # htree, relative_pos, sem


@pytest.mark.parametrize("mode", list(OLD_MODES))
@pytest.mark.parametrize("homogeneous", [False, True], ids=["typed", "homog"])
def test_blocks_of_the_earlier_modes_are_unchanged(homogeneous, mode):
    ht, rel, sem = OLD_MODES[mode]
    tn, mn, mo = fc.THRESHOLDS
    kw = dict(threshold_near=tn, max_near=mn, max_on=mo, htree=ht, relative_pos=rel, sem_dim=300 if sem else 0,
              n_labels=fc.N_LABELS if sem else 0, clique_dim=6 if ht else None, homogeneous=homogeneous)
    name = ("homog_" if homogeneous else "typed_") + mode
    r = dsg.frame_host_stage(*fc.frame("fixture"), **kw)
    sha, sizes = PINNED[name]
    assert hashlib.sha256(r["block"].tobytes()).hexdigest() == sha
    assert tuple(int(r["sizes"][k]) for k in (_lib.FS_STAGING_BYTES, _lib.FS_ARENA_BYTES, _lib.FS_ITEMS, _lib.FS_BLOCKS)) == sizes
    assert _lib.FK_EATTR_HT not in r["items"][:, _lib.FI_KIND] and r["items"][:, _lib.FI_TENSOR].max() < _lib.FT_BATCH
    pair = [fc.frame("fixture"), fc.frame((7, 2))]
    for form, suffix in ((_lib.FB_COLLATED, "_collated"), (_lib.FB_STORE, "_store")):
        b = dsg.frame_batch_host_stage(pair, form=form, y=[bc.labels(a) for a in pair], **kw)
        sha, sizes = PINNED[name + suffix]
        assert hashlib.sha256(b["block"].tobytes()).hexdigest() == sha, suffix
        assert tuple(int(b["sizes"][k]) for k in (_lib.FBS_STAGING_BYTES, _lib.FBS_ARENA_BYTES, _lib.FBS_ITEMS, _lib.FBS_BLOCKS)) == sizes


def test_the_numbers_of_the_mode_lie_behind_every_earlier_one():
    assert _lib.FT_HTREL == _lib.FT_BATCH + _lib.FT_BATCH_COUNT == 87 and _lib.FT_HTREL_COUNT == 17 and _lib.FK_EATTR_HT == 8
    assert (_lib.FT_HTREE, _lib.FT_COUNT, _lib.FT_HOMOG, _lib.FT_HOMOG_COUNT, _lib.FT_BATCH, _lib.FT_BATCH_COUNT) == (16, 45, 45, 9, 54, 33)
    header = open(os.path.join(ROOT, "include", "hydra_mp.h")).read().replace("  ", " ")
    for name, value in (("HMP_FRAME_RELPOS_HTREE", _lib.FRAME_RELPOS_HTREE), ("HMP_FK_EATTR_HT", _lib.FK_EATTR_HT), ("HMP_FT_HTREL_COUNT", 17),
                        ("HMP_FRAME_END_WORDS", _lib.FRAME_END_WORDS), ("HMP_FE_DIRECT", _lib.FE_DIRECT), ("HMP_FE_GATHER", _lib.FE_GATHER),
                        ("HMP_FE_CLIQUE", _lib.FE_CLIQUE), ("HMP_FRAME_ITEM_WORDS", 12), ("HMP_FRAME_MAX_ITEMS", 64), ("HMP_ABI_VERSION", _lib.ABI_VERSION)):
        assert f"#define {name} {value}" in header, name
    assert "#define HMP_FT_HTREL (HMP_FT_BATCH + HMP_FT_BATCH_COUNT)" in header


# ---- the stand-alone sanitizer program -------------------------------------------------------------------------------------------
def test_host_and_batch_stage_are_clean_under_asan_and_ubsan(tmp_path):
    """`make frame_check`, run with --htree-relpos: frame.cpp + htree.cpp + a program with its own main under -fsanitize=address,undefined (CPU
    only, the runtimes linked statically, nothing preloaded).  It builds every frame file in the new mode, typed and homogeneous,
    packs it into a buffer cut to size, and runs the batch stage over all of them in both forms."""
    files = []
    for name in ("fixture", "triangle", (1, 1), "no_room", (300, 3)):
        path = str(tmp_path / f"frame_{len(files)}.bin")
        dsg.save_frame_file(path, *hc.frame(name), htree=True, htree_relative_pos=True, clique_dim=hc.CLIQUE_DIM)
        files.append(path)
    out = fb.run_frame_check(["--htree-relpos"] + files)
    assert "typed frame 0: items 46" in out and "homogeneous frame 0: items 59" in out and "typed frame 3: items 0" in out
    assert "typed collated: frames 5 graphs 4" in out and "homogeneous store: frames 5 graphs 4" in out
