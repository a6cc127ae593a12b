"""Host stage of the frame pipeline (csrc/frame.cpp; include/hydra_mp.h section 14) without a device: the native bookkeeping
against the reference's recorded result, against ``dsg.RoomObjectGraph`` / the oracle's predicates on synthetic frames with every
irregular case, the H-tree topology inside the packed block against ``htree.htree_topology``, the layout of the block and the arena,
the refusals, and the stand-alone sanitizer program.  The block is also read with numpy, item by item (what the one launch is
specified to write), and compared with the existing torch path on the CPU."""

import numpy as np
import pytest
import torch

import _frame_block as fb
import _frame_cases as fc
from hydra_gnn_amd import _lib, dsg, htree
from oracle import dsg_ref

CASES = ["fixture", "special"] + fc.SIZES


def host(name, **kw):
    tn, mn, mo = fc.THRESHOLDS
    return dsg.frame_host_stage(*fc.frame(name), threshold_near=tn, max_near=mn, max_on=mo, **kw)


def read_block(r, htree_mode, table=None):
    """{(store key, attribute): array} of a typed frame: its block executed with numpy"""
    items = r["items"]
    fb.check_typed_frame(items)
    arena, _ = fb.expand(r["block"], items, int(r["sizes"][_lib.FS_ARENA_BYTES]), table)
    return fb.views(arena, fb.tensor_rows(items), htree_mode, False)


def test_fixture_reproduces_the_reference():
    exp = np.load(fc.EXP)
    ids = fc.frame("fixture")[0]
    r = host("fixture")
    assert np.array_equal(ids[r["kept"]], exp["obj_id"]) and r["kept"].size == 62  # in order
    assert np.array_equal(r["obj_room"], exp["obj_room"])
    assert np.array_equal(np.sort(ids[r["dropped"]]), exp["dropped_obj_id"]) and r["dropped"].size == 3
    assert np.array_equal(ids[r["rooms"]], exp["room_id"]) and r["rooms"].size == 5
    assert np.array_equal(r["rr_edges"], exp["rr_edges"]) and r["rr_edges"].shape == (2, 1)
    assert np.array_equal(r["oo_edges"], exp["oo_edges"]) and r["oo_edges"].shape == (2, 178)  # same edges, same order
    sz = r["sizes"]
    assert [int(sz[k]) for k in (_lib.FS_KEPT, _lib.FS_DROPPED, _lib.FS_ROOMS, _lib.FS_E_OO, _lib.FS_E_RR)] == [62, 3, 5, 178, 1]


@pytest.mark.parametrize("name", CASES, ids=str)
def test_host_stage_equals_room_object_graph_and_the_oracle_predicates(name):
    rog = dsg.RoomObjectGraph(fc.scene_graph(fc.frame(name)))
    r = host(name)
    assert np.array_equal(r["kept"], rog.objects) and np.array_equal(r["rooms"], rog.rooms)
    assert np.array_equal(r["obj_room"], rog.obj_room) and np.array_equal(r["dropped"], rog.dropped)
    assert np.array_equal(r["rr_edges"], rog.rr_edges)
    assert r["room_bb"].tobytes() == np.ascontiguousarray(rog.room_bb).tobytes()  # bit for bit
    want = dsg_ref.object_edges(rog.obj_pos, rog.obj_size, rog.obj_room, *fc.THRESHOLDS)
    assert np.array_equal(r["oo_edges"], want)
    if isinstance(name, tuple):
        assert (rog.objects.size, rog.rooms.size) == name and rog.dropped.size == 0
        assert want.shape[1] > 0 or name[0] == 1


def test_special_frame_holds_every_irregular_case():
    arrays = fc.frame("special")
    ids = arrays[0]
    sym = lambda c, i: (ord(c) << 56) + i
    r = host("special")
    room_of = {int(ids[o]): int(ids[r["rooms"][k]]) for o, k in zip(r["kept"], r["obj_room"])}
    assert sorted(int(v) for v in ids[r["dropped"]]) == [sym("O", 100), sym("O", 104)]  # no place; neither room nor sibling with one
    assert room_of[sym("O", 101)] == room_of[sym("O", 102)] == sym("R", 1)  # equal distance: the lower sibling id (p101 -> R1)
    assert room_of[sym("O", 103)] == sym("R", 1)  # unequal distance: the nearer sibling (p112 -> R1), not the lower id (p111 -> R0)
    k2, k3 = [int(np.nonzero(ids[r["rooms"]] == sym("R", q))[0][0]) for q in (2, 3)]
    assert not r["room_bb"][k2].any() and r["room_bb"][k3].any()  # a room without places has a zero box
    assert k2 not in r["obj_room"] and k3 not in r["obj_room"]  # rooms without objects
    assert r["rr_edges"].shape == (2, 3)  # R0-R1, R1-R2, R2-R3 once each: the duplicate and the self edge add nothing


@pytest.mark.parametrize("name", ["fixture", (7, 2), (300, 3)], ids=str)
def test_htree_topology_in_the_packed_block(name):
    r = host(name, htree=True, clique_dim=6)
    n_o, n_r = r["kept"].size, r["rooms"].size
    ro = np.stack([r["obj_room"], np.arange(n_o, dtype=np.int32)])
    want = htree.htree_topology(n_o, n_r, *[torch.from_numpy(e.astype(np.int64)) for e in (r["oo_edges"], r["rr_edges"], ro)])
    sz = r["sizes"]
    assert [int(v) for v in sz[_lib.FS_HT_COUNTS:_lib.FS_HT_COUNTS + 4]] == want["counts"]
    assert [int(v) for v in sz[_lib.FS_HT_EDGES:_lib.FS_HT_EDGES + 10]] == [e.shape[1] for e in want["edges"]]
    assert [int(v) for v in sz[_lib.FS_HT_INIT:_lib.FS_HT_INIT + 3]] == [e.shape[1] for e in want["init"]]
    got = read_block(r, True)
    T0 = _lib.FT_HTREE
    for k in range(10):
        assert np.array_equal(got[dsg._FRAME_TENSORS[T0 + 14 + k]], want["edges"][k]), k
    for k in range(3):
        assert np.array_equal(got[dsg._FRAME_TENSORS[T0 + 24 + k]], want["init"][k]), k
    for t, orig in ((T0 + 27, want["object_orig"]), (T0 + 28, want["room_orig"])):  # the pool lists [arange | orig]
        assert np.array_equal(got[dsg._FRAME_TENSORS[t]], np.stack([np.arange(orig.size), orig]))


@pytest.mark.parametrize("mode", ["baseline", "relative_pos", "sem300", "htree", "htree_sem300"])
@pytest.mark.parametrize("name", CASES, ids=str)
def test_layout_and_block_contents(name, mode):
    """Every item's output lies inside the arena, 16-byte aligned and disjoint from the others; the workgroup prefix is the one
    the kernel's mapping expects; and the block read with numpy equals the existing path on the CPU (H-tree clique means of more
    than two rooms excepted: index_add_ has no defined order)."""
    sem, ht = mode.endswith("sem300"), mode.startswith("htree")
    r = host(name, htree=ht, relative_pos=mode == "relative_pos", sem_dim=300 if sem else 0, n_labels=fc.N_LABELS if sem else 0,
             clique_dim=6 if ht else None)
    items, sz = r["items"], r["sizes"]
    assert 0 < len(items) <= 64 and len(items) == sz[_lib.FS_ITEMS]
    spans, block0 = [], 0
    for kind, tensor, rows, width, dst, s0, s1, s2, s3, p0, p1, b0 in items.tolist():
        elem = 8 if kind in (_lib.FK_I64, _lib.FK_EDGE) else 4
        n_el = 2 * width if kind == _lib.FK_EDGE else rows * width
        assert dst % 16 == 0 and dst + n_el * elem <= sz[_lib.FS_ARENA_BYTES]
        spans.append((dst, dst + n_el * elem))
        assert b0 == block0
        block0 += -(-rows // 4) if kind == _lib.FK_FEAT and width >= 32 else -(-n_el // 256)
    assert block0 == sz[_lib.FS_BLOCKS]
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    table = fc.semantic_table().numpy()
    got = read_block(r, ht, table)
    data, _ = fc.existing_frame(fc.frame(name), sem, relative_pos=mode == "relative_pos")
    if ht:
        data = htree.generate_htree(data, clique_dim=6)
    want = fc.hetero_arrays(data)  # the existing path's own stores and attributes, not the table's
    assert sorted(map(str, got)) == sorted(map(str, want))
    for t, w in want.items():
        if ht and t in (("object-room", "x"), ("room-room", "x")):
            members = fc.clique_members(data, 2 if t[0] == "object-room" else 3)
            small = np.array([len(m) <= 2 for m in members], dtype=bool)
            assert not got[t][:, 3:].any() and np.array_equal(got[t][small], w[small])
            continue
        assert got[t].dtype == w.dtype and got[t].shape == w.shape and np.array_equal(got[t], w), t


def test_refusals():
    ids, layer, pos, bb_min, bb_max, label, edges = fc.frame((7, 2))
    bad = label.copy()
    victim = int(np.nonzero(layer == dsg.OBJECTS)[0][2])
    bad[victim] = fc.N_LABELS
    with pytest.raises(_lib.HydraMPError, match=str(int(ids[victim]))):
        dsg.frame_host_stage(ids, layer, pos, bb_min, bb_max, bad, edges, sem_dim=300, n_labels=fc.N_LABELS)
    bad[victim] = -1
    with pytest.raises(_lib.HydraMPError, match=str(int(ids[victim]))):
        dsg.frame_host_stage(ids, layer, pos, bb_min, bb_max, bad, edges, sem_dim=300, n_labels=fc.N_LABELS)
    assert not dsg.frame_host_stage(ids, layer, pos, bb_min, bb_max, bad, edges)["empty"]  # without a table any label passes
    with pytest.raises(_lib.HydraMPError, match="relative"):
        dsg.frame_host_stage(ids, layer, pos, bb_min, bb_max, label, edges, htree=True, relative_pos=True)
    with pytest.raises(_lib.HydraMPError, match="relative"):
        dsg.FramePipeline("cuda:0", htree=True, relative_pos=True)
    # an output tensor number that a mode does not define (another mode's included) is refused, never viewed as some default type
    arena = torch.zeros(64, dtype=torch.uint8)
    defined = {(False, False): 16 + 10, (True, False): 29 + 17 + 33, (False, True): 9 + 4, (True, True): 9 + 6}  # own range(s) + batch range
    for mode, table in dsg._TENSOR_TABLES.items():
        assert len(table) == _lib.FT_HTREL + _lib.FT_HTREL_COUNT and sum(e[2] is not None for e in table) == defined[mode]
        resolved = dsg._resolve_views(table, arena.view(torch.float32), arena.view(torch.int64), arena.view(torch.bool))
        for t, entry in enumerate(table):
            if entry[2] is None:
                with pytest.raises(_lib.HydraMPError, match=f"number {t} "):
                    dsg._arena_view(resolved, t, 0, 1, 1)
            else:
                assert dsg._arena_view(resolved, t, 16, 2, 2).numel() in (2, 4)
        with pytest.raises(_lib.HydraMPError, match="number 104 "):
            dsg._arena_view(resolved, len(table), 0, 1, 1)
    with pytest.raises(_lib.HydraMPError, match="listed twice"):
        dsg.frame_host_stage(np.concatenate([ids, ids[:1]]), *[np.concatenate([a, a[:1]]) for a in (layer, pos, bb_min, bb_max, label)], edges)


@pytest.mark.parametrize("htree_mode", [False, True])
def test_frames_without_a_room_or_without_kept_objects_return_none(htree_mode):
    """``convert`` returns None for them and does not touch the device: this runs where there is none"""
    ids, layer, pos, bb_min, bb_max, label, edges = fc.frame((7, 2))
    pipe = dsg.FramePipeline("cuda:0", htree=htree_mode, clique_dim=6 if htree_mode else None)
    no_room = layer != dsg.ROOMS
    assert pipe.convert(*[a[no_room] for a in (ids, layer, pos, bb_min, bb_max, label)], edges) is None
    no_object = layer != dsg.OBJECTS
    assert pipe.convert(*[a[no_object] for a in (ids, layer, pos, bb_min, bb_max, label)], edges) is None
    assert pipe.convert(ids, layer, pos, bb_min, bb_max, label, edges[:, :0]) is None  # no edges: every object is dropped
    r = dsg.frame_host_stage(ids, layer, pos, bb_min, bb_max, label, edges[:, :0])
    assert r["empty"] and r["dropped"].size == 7 and r["rooms"].size == 2 and r["block"].size == 0
    assert pipe._arena is None and pipe._d_staging is None


def test_host_stage_is_clean_under_asan_and_ubsan(tmp_path):
    """`make frame_check`: frame.cpp + htree.cpp + a program with its own main under -fsanitize=address,undefined (CPU only, nothing
    preloaded), run on the fixture frame and on the (300, 3) frame, baseline and H-tree"""
    files = []
    for name in ("fixture", (300, 3)):
        for ht in (False, True):
            path = str(tmp_path / f"frame_{len(files)}.bin")
            dsg.save_frame_file(path, *fc.frame(name), htree=ht, sem_dim=0 if ht else 300, n_labels=0 if ht else fc.N_LABELS, clique_dim=6 if ht else 0)
            files.append(path)
    out = fb.run_frame_check(files)
    assert "kept 62 dropped 3 rooms 5 oo 178 rr 1" in out and "kept 300 dropped 0 rooms 3" in out
